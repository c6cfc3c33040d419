/*
 * svgr.h -- C ABI of libsvgr_hip.so, the MI355X (gfx950) anti-aliased path rasterizer.
 *
 * The reference (aslpavel/svgrasterize.py) has no FFI layer: its boundary for this path is three
 * Python call signatures plus the Layer value type.  Each entry point below names the
 * reference interface it stands behind ("S:n" = svgrasterize.py line n).  The Python host classes in
 * svgrasterize.py_amd/ bind these with ctypes; INTEGRATION.md shows the stub a reference maintainer
 * would add.
 *
 * Conventions
 *   - every function returns 0 on success or a negative svgr_status; svgr_last_error() gives the text
 *     (thread local).  No C++ exception crosses the boundary.
 *   - plain pointers and sizes only.  Host pointers are caller-owned; device memory is an opaque
 *     svgr_buf handle (or a raw device pointer wrapped with svgr_buf_wrap, e.g. torch's data_ptr()).
 *   - one svgr_ctx per device; calls on one context are serialised by the caller; all kernels of a
 *     context run on its HIP stream; functions that return host-visible data synchronise that stream.
 *   - coordinates follow the reference: a point is (row, col) in presentation space; a bbox /
 *     viewport is {row0, col0, rows, cols} (S:88-89, S:966-975).
 *   - all pixel arithmetic is IEEE double with the reference's operation order; the canvas can be
 *     stored as float32 (the contract of BASELINE.json: within 1 ULP of float32(reference)) or double.
 */
#ifndef SVGR_H
#define SVGR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: svgr_batch_set_groups, svgr_batch_set_gradients, svgr_batch_plan_many, svgr_batch_render_window added; svgr_gradient.n_stops
 *    no longer capped at 32; SVGR_RENDER_DETERMINISTIC
 * 3: SVGR_RENDER_SAME_GEOMETRY, SVGR_OUT_FILLS_F64, svgr_layer_convert_to, svgr_layer_scale_to, svgr_batch_render_windows added
 *    (nothing changed or removed)
 * 4: svgr_hash_buffers added (nothing changed or removed)
 * 6: svgr_batch_draw, svgr_measure_begin / _end / _launches added (nothing changed or removed)
 * 5: svgr_layer_compose_over / _in, svgr_layer_convert_scale_to, svgr_layer_convolve_ops, svgr_batch_get_extents added (nothing changed
 *    or removed)
 * 6 (later, nothing changed or removed): svgr_layer_turbulence, svgr_layer_component_transfer, svgr_layer_convolve_matrix,
 *    svgr_layer_displacement_map added (filter primitives beyond the reference); svgr_image_upload, svgr_image_fill,
 *    svgr_png_unfilter added (SVG <image>, beyond the reference); svgr_layer_lighting added (feDiffuseLighting,
 *    feSpecularLighting); svgr_layer_mix_blend and SVGR_BLEND_* added (CSS mix-blend-mode); svgr_jpeg_entropy and
 *    svgr_jpeg_decode added (JPEG in SVG <image>); svgr_layer_tile added (feTile); svgr_jpeg_encode,
 *    svgr_jpeg_entropy_encode and svgr_jpeg_symbol_counts added (JPEG output); svgr_png_filter, svgr_deflate and
 *    svgr_deflate_chunk added (the device PNG encoder); svgr_layer_to_tensor, svgr_tensor_to_layer, svgr_tensor_block,
 *    svgr_tensor_run, svgr_stream_wait_for and svgr_stream_signal_to added (tensor output); svgr_quant_distinct,
 *    svgr_quant_bins, svgr_quant_index, svgr_quant_block and svgr_quant_groups added (indexed PNG output); svgr_quant_dither,
 *    svgr_dither_tile_rows and svgr_dither_tile_cols added (dithering); svgr_png_samples, svgr_png_filter_bytes and
 *    svgr_png_filter_span added (grey, RGB and 16-bit PNG output); svgr_cover_forward, svgr_cover_backward, svgr_cover_block
 *    and svgr_cover_scan added (differentiable coverage); svgr_compose_forward, svgr_compose_backward, svgr_compose_block and
 *    svgr_compose_groups added (differentiable compositing); svgr_compose_painted_forward and svgr_compose_painted_backward
 *    added (gradient paints in differentiable compositing); svgr_compose_grouped_forward, svgr_compose_grouped_backward and
 *    svgr_group_depth added (isolated groups in differentiable compositing: opacity and clip paths); svgr_compose_masked_forward
 *    and svgr_compose_masked_backward added (luminance-masked groups in differentiable compositing) */
#define SVGR_ABI_VERSION 6

typedef enum {
    SVGR_OK = 0,
    SVGR_E_INVALID = -1,   /* bad argument (reference raises ValueError, S:945, S:989, S:298) */
    SVGR_E_HIP = -2,       /* HIP runtime error */
    SVGR_E_NOMEM = -3,
    SVGR_E_NODEVICE = -4,  /* no gfx950 device visible */
    SVGR_E_OVERFLOW = -5,  /* internal capacity exceeded (re-plan) or flatten depth cap hit */
    SVGR_E_STATE = -6      /* call order (render before plan, ...) */
} svgr_status;

typedef struct svgr_ctx svgr_ctx;
typedef struct svgr_buf svgr_buf;
typedef struct svgr_batch svgr_batch;

/* segment kinds in svgr_batch_desc.seg_kind */
#define SVGR_SEG_LINE 0   /* PATH_LINE / PATH_CLOSED / PATH_UNCLOSED (S:865-873): 2 points */
#define SVGR_SEG_CUBIC 1  /* PATH_CUBIC, and PATH_QUAD / PATH_ARC after host conversion: 4 points */

/* fill rules (S:874-875, S:984-989) */
#define SVGR_FILL_NONZERO 0
#define SVGR_FILL_EVENODD 1
/* optional flags or-ed into path_rule (canvas outputs only): a CLIP node whose clip and target are single paths
 * (Scene.render RENDER_CLIP, S:698-715: `Layer.compose([mask, image], COMPOSE_IN)`) is two consecutive paths:   */
#define SVGR_PATH_CLIP_SOURCE 2 /* coverage only (Path.mask of the clip path); not painted                        */
#define SVGR_PATH_CLIPPED 4     /* fill multiplied by the coverage of the PREVIOUS path, which must be a clip source */

/* output kinds of svgr_batch_render */
#define SVGR_OUT_CANVAS_F32 0  /* (rows, cols, 4) float32, all paths composited OVER in paint order */
#define SVGR_OUT_CANVAS_F64 1  /* same in double (Layer.image dtype of the reference, S:42) */
#define SVGR_OUT_MASK_F64 2    /* single path: (rows, cols) double coverage = Path.mask().image[..., 0] */
#define SVGR_OUT_FILL_F64 3    /* single path: (rows, cols, 4) double = mask * paint (S:1019) */
#define SVGR_OUT_MASKS_F64 4   /* every path of the batch: its Path.mask (rows_p, cols_p) double, back to back in path order;
                                * layer p starts at sum_{q<p} rows_q*cols_q doubles (clipped bboxes of svgr_batch_get_bboxes,
                                * empty ones count 0).  One launch for all the masks a scene needs (clips, gradient fills). */
#define SVGR_OUT_FILLS_F64 5   /* every path of the batch: its Path.fill layer (rows_p, cols_p, 4) double = mask * paint, back to back in
                                * path order (layer p starts at 4 * sum_{q<p} rows_q*cols_q doubles): the solid fills a document
                                * draws node by node (children of filter / mask nodes) in one launch. */

/* flags of svgr_batch_render */
#define SVGR_RENDER_CLIP01 1u  /* clip RGBA to [0, 1] on store (canvas_merge_at, S:326) */
#define SVGR_RENDER_TIMED 2u   /* bracket the stages with HIP events (svgr_batch_timings) */
/* Bit-reproducible output: the reference's np.cumsum (S:983) adds a row's pieces in one fixed order; the default render
 * adds them in whatever order the LDS atomics of several waves land (results differ in the last bits of a double, i.e.
 * in float32 rounding ties).  With this flag one wave per workgroup does every accumulation, in list order: two
 * renders of the same batch are bit-identical, at roughly half the speed of the geometry and scatter phases. */
#define SVGR_RENDER_DETERMINISTIC 4u
/* svgr_batch_render_window only: this window belongs to the same picture as the window the previous render of this batch drew
 * -- no input of the batch has changed in between --, so the geometry kernels' results are taken as they are instead of being
 * produced again (a document whose runs of fills share one batch draws each run's window from ONE geometry pass).  Ignored
 * (the pass runs) after any svgr_batch_set_* / plan since that render. */
#define SVGR_RENDER_SAME_GEOMETRY 8u

/* -------------------------------------------------------------------------------------------- */
/* context + device memory                                                                      */
/* -------------------------------------------------------------------------------------------- */
int svgr_abi_version(void);
int svgr_tile_rows(void); /* band height: the row granularity of svgr_batch_set_bands */
int svgr_tile_cols(void);
const char* svgr_last_error(void);
int svgr_device_count(void);

int svgr_init(int device_id, svgr_ctx** out);
int svgr_shutdown(svgr_ctx* ctx);
/* run the context's kernels on an existing hipStream_t (e.g. torch.cuda.current_stream().cuda_stream) */
int svgr_set_stream(svgr_ctx* ctx, void* hip_stream);
int svgr_sync(svgr_ctx* ctx);
int svgr_device_name(svgr_ctx* ctx, char* out, size_t cap);
/* Measurement helpers (bench.py; the reference prints one wall-clock figure per render, S:3854-3864 -- these split it).
 * svgr_measure_begin holds the context's stream busy for `hold_ms` (0: not at all) and marks the start behind the hold;
 * svgr_measure_end marks the end, waits for it and returns the milliseconds of DEVICE time between the marks: what the caller
 * enqueued in between has queued up behind the hold and run back to back, however long the host took to issue it (less than the
 * hold).  svgr_measure_launches: kernel launches the library has made in this process so far. */
int svgr_measure_begin(svgr_ctx* ctx, double hold_ms);
int svgr_measure_end(svgr_ctx* ctx, double* ms);
int svgr_measure_launches(uint64_t* out);
/* Host only, no GPU involved: a 64-bit hash over the bytes of `n` host buffers (ptrs[i], nbytes[i]), in order.  What the
 * caller's retained renders guard themselves with: the reference's Scene.render (S:649-752) keeps nothing between calls, so a
 * paint or a segment array edited in place is simply drawn with its new values; a caller that keeps built batches between
 * renders of one document checks this hash of the document's arrays before it reuses them. */
int svgr_hash_buffers(const void* const* ptrs, const int64_t* nbytes, int64_t n, uint64_t* out);

int svgr_buf_alloc(svgr_ctx* ctx, size_t bytes, svgr_buf** out);
int svgr_buf_wrap(svgr_ctx* ctx, void* device_ptr, size_t bytes, svgr_buf** out); /* non-owning */
int svgr_buf_free(svgr_ctx* ctx, svgr_buf* buf);
void* svgr_buf_ptr(const svgr_buf* buf);
size_t svgr_buf_bytes(const svgr_buf* buf);
int svgr_buf_zero(svgr_ctx* ctx, svgr_buf* buf);
int svgr_buf_copy(svgr_ctx* ctx, svgr_buf* dst, const svgr_buf* src, size_t bytes); /* device to device, async */
int svgr_upload(svgr_ctx* ctx, svgr_buf* dst, size_t dst_off, const void* host, size_t bytes);
int svgr_download(svgr_ctx* ctx, const svgr_buf* src, size_t src_off, void* host, size_t bytes); /* syncs */

/* -------------------------------------------------------------------------------------------- */
/* batched paths -> coverage -> paint -> composite                                              */
/*                                                                                              */
/* Stands behind Path.mask (S:922-993), Path.fill solid branch (S:995-1019) and the OVER merge  */
/* of a group of fills (Layer.compose -> canvas_merge_union(full=False), S:177-207, S:366-377):  */
/* rendering paths 0..n-1 into the canvas is the same per-pixel operation sequence as composing */
/* their fill layers in painter's order.                                                        */
/* -------------------------------------------------------------------------------------------- */
typedef struct {
    /* geometry in USER space; the device applies path_m6 in the reference's fma form (S:531-534) */
    const double* segs;          /* n_segs x 8: 4 points (x, y); lines use the first two          */
    const uint8_t* seg_kind;     /* n_segs: SVGR_SEG_*                                            */
    int64_t n_segs;
    const int64_t* path_seg_off; /* n_paths + 1 offsets into segs, paint order                    */
    int64_t n_paths;
    const double* path_m6;       /* n_paths x 6: rows 0-1 of the 3x3 transform {m00,m01,m02,m10,m11,m12} */
    const uint8_t* path_rule;    /* n_paths: SVGR_FILL_* | SVGR_PATH_* flags                       */
    const double* path_paint;    /* n_paths x 4 premultiplied RGBA already in the compositing space
                                    (the host applies S:1015-1018 to the 4-vector), times opacity   */
    int64_t viewport[4];         /* {row0, col0, rows, cols}; rows <= 0 means "no viewport"
                                    (only valid for the single-path outputs)                      */
    double flatness;             /* 0.1 in the reference (S:955)                                   */
} svgr_batch_desc;

/* copies the description to HBM; nothing is rendered yet */
int svgr_batch_create(svgr_ctx* ctx, const svgr_batch_desc* desc, svgr_batch** out);
int svgr_batch_destroy(svgr_batch* batch);

/* replace per-path paints / transforms of an existing batch (same counts) */
int svgr_batch_set_paints(svgr_batch* batch, const double* path_paint);
int svgr_batch_set_transforms(svgr_batch* batch, const double* path_m6);

/* Isolated groups inside one batch (Scene.render CLIP / OPACITY over a GROUP of solid fills, S:674-715; replaces one
 * Scene.render recursion + Layer.compose round trip per group): path_group[p] = the group path p belongs to, or -1; the
 * members of a group are consecutive paths.  When a group closes it is, as a whole, multiplied by the coverage of
 * group_clip_src[g] (a SVGR_PATH_CLIP_SOURCE path right in front of the group's first member; -1: no clip:
 * `Layer.compose([mask, group], COMPOSE_IN)`, S:712) and by group_opacity[g] (`Layer.opacity`, S:171-175; 1: none), then
 * composited OVER what lies under it.  Canvas outputs only; n_groups = 0 removes the groups.  Call before svgr_batch_plan. */
int svgr_batch_set_groups(svgr_batch* batch, const int32_t* path_group, int64_t n_groups, const int32_t* group_clip_src,
                          const double* group_opacity);

/* Multi-GPU sharding: rank `rank` of `world` keeps the strips s with s % world == rank, a strip being
 * `strip_bands` consecutive bands (band = svgr_tile_rows() scanlines).  The rank still computes every path's
 * exact bbox, but only flattens-to-memory, bins and renders what reaches its own bands; its output buffer holds
 * the owned bands packed in increasing order.  Default (0, 1, 1) = everything.  Invalidates the plan.       */
int svgr_batch_set_bands(svgr_batch* batch, int rank, int world, int strip_bands);

/* Geometry pass with host read-backs: flatten, per-path bbox, band binning; sizes every work
 * buffer.  Must run once before svgr_batch_render and again after geometry/viewport changes.
 * Synchronises.                                                                                 */
int svgr_batch_plan(svgr_batch* batch);

/* svgr_batch_plan for many batches behind one wait per stream: a document's per-node route plans dozens of small batches
 * (Scene.render: one per run of fills between two filter nodes, S:674-688), and a plan alone is a device round trip whose
 * kernels are a fraction of it.  Same result and same errors as calling svgr_batch_plan on each (the first error ends it). */
int svgr_batch_plan_many(svgr_batch** batches, int64_t n);

typedef struct {
    int64_t n_edges;        /* flattened edges E                                                 */
    int64_t path_pixels;    /* P = sum over paths of clipped bbox rows*cols (SURVEY 8d unit)      */
    int64_t n_band_segs;    /* edge x band records                                               */
    int64_t n_path_bands;   /* (path, band) pairs                                                */
    int64_t n_nonempty;     /* paths with a non-empty clipped bbox                                */
    int64_t bbox_union[4];  /* union of the non-empty bboxes {row0, col0, rows, cols}             */
    int64_t tile_rows, tile_cols;
} svgr_batch_stats;
int svgr_batch_get_stats(const svgr_batch* batch, svgr_batch_stats* out);
/* per-path clipped integer bbox {row0, col0, rows, cols}; rows <= 0 = empty (Path.mask -> None) */
int svgr_batch_get_bboxes(const svgr_batch* batch, int32_t* out /* n_paths x 4 */);
/* per-path extent of ALL its flattened points, unclipped, in presentation space: {min row, min col, max row, max col} doubles --
 * the bounding box of ConvexHull(lines) (S:993, S:2010-2020) under a transform that keeps the axes apart, i.e. the frame of an
 * objectBoundingBox paint (S:1023-1027) without fetching the hull.  Read from the plan's own geometry pass: valid between
 * svgr_batch_plan and the first render (SVGR_E_STATE otherwise).  A path without edges: {+inf, +inf, -inf, -inf}.
 * (svgr_batch_set_gradients with the same path -> gradient assignment and new descriptions -- those frames -- keeps the plan
 * and its pass.)  Defined for the paths this rank KEEPS: under svgr_batch_set_bands with world > 1 a path none of whose rows can
 * reach an owned band is not flattened here and reports {+inf, +inf, -inf, -inf} like a path without edges. */
int svgr_batch_get_extents(svgr_batch* batch, double* out /* n_paths x 4 */);
/* flattened edges in presentation space, (E, 2, 2) doubles, grouped by path; edge_path may be NULL */
int svgr_batch_get_edges(const svgr_batch* batch, double* edges, int32_t* edge_path, int64_t cap);
/* ALL flattened edges of the batch, also those that cannot reach the viewport: the point set of Path.mask's
 * ConvexHull(lines) (S:993), from which objectBoundingBox clips, gradients and patterns take their frame.  Call with
 * edges == NULL to learn the count (*n_edges), then with a buffer of at least that many (2, 2) doubles.          */
int svgr_batch_all_edges(svgr_batch* batch, double* edges, int32_t* edge_path, int64_t cap, int64_t* n_edges);

/* Hit testing: which paths of the batch hold a point (SVG DOM isPointInFill / isPointInStroke), and which one is on top there
 * (elementFromPoint).  Both entries work on the batch's FULL edge set -- the block svgr_batch_all_edges downloads, edges that
 * cannot reach the viewport included -- which they flatten on the first call, group by path and keep on the device until
 * svgr_batch_set_transforms; the batch needs no plan, and one it has is left as it is.
 *
 * The predicate (csrc/svgr_hit.h is its one home, compiled for host and device without fused multiply-adds): for an edge
 * (a0, b0) -> (a1, b1), `a` being the first coordinate of an edge as svgr_batch_all_edges stores it and `b` the second, and a
 * point (pa, pb) in the same order:
 *     up = b0 <= pb && b1 > pb,  down = b1 <= pb && b0 > pb,  d = (a1 - a0) * (pb - b0) - (pa - a0) * (b1 - b0)
 *     the edge counts +1 if up && d > 0, -1 if down && d < 0, else 0
 * A path's winding number is the sum over its edges; it is inside for w != 0 (SVGR_FILL_NONZERO) or w & 1 (SVGR_FILL_EVENODD).  A
 * point with a NaN or infinite coordinate has winding 0 everywhere: it is outside, not an error.  The edges are the ones the
 * renderer flattens under the batch's transforms and flatness, so "inside" agrees with what is drawn; a point within rounding
 * distance of an edge may fall either way, but falls the same way on host and device and from run to run.
 *
 * The points are either `points`, n_points x 2 host doubles (pa, pb), or -- points == NULL -- the pixel centres of
 * grid = {row0, col0, rows, cols}, rows * cols == n_points: (row0 + r + 0.5, col0 + c + 0.5) in row-major order, made in the
 * kernel.  Exactly one of the two is given (SVGR_E_INVALID otherwise).
 *
 * svgr_batch_winding: winding_out[i * n_paths + p] = the winding number of path p at point i.  SVGR_E_OVERFLOW when
 * n_points * n_paths leaves 31 bits.
 *
 * svgr_batch_pick: the paths are hit regions in paint order.  Path p is clipped by the groups
 * clip_group[clip_off[p] .. clip_off[p + 1]); group g has the sources group_src[group_off[g] .. group_off[g + 1]), paths with a
 * SMALLER index than every path that uses the group:
 *     pass(p) = inside(p) && for every clip group g of p: (some source s of g has pass(s))
 *     top_out[i] = the largest p with pickable[p] != 0 && pass(p) at point i, or -1
 * clip_off holds n_paths + 1 and group_off n_groups + 1 ascending offsets from 0 (clip_group / group_off / group_src may be NULL
 * when nothing refers to them).  Tables that break this -- a clip source whose index is not smaller than its user's among them
 * -- are SVGR_E_INVALID before anything is launched.  bits_out, optional: n_points x ceil(n_paths / 32) words of pass bits (path
 * p: bit p % 32 of word p / 32).  The point-by-path bit matrix lives in device scratch of at most scratch_bytes (0: 256 MiB; never
 * less than one workgroup's rows), and the points are taken in as many passes as that needs: an id map of a large canvas cannot
 * exhaust memory.
 *
 * A batch without paths, and n_points == 0, launch nothing and succeed (top_out is then all -1).  The results come back behind
 * one wait.  svgr_hit_block: points per workgroup (a grid query's workgroup is a square tile of that many pixels);
 * svgr_hit_chunk: edges of a path staged through LDS at a time.                                                              */
int svgr_batch_winding(svgr_batch* batch, const double* points, const int64_t* grid, int64_t n_points, int32_t* winding_out);
int svgr_batch_pick(svgr_batch* batch, const double* points, const int64_t* grid, int64_t n_points, const uint8_t* pickable,
                    const int32_t* clip_off, const int32_t* clip_group, const int32_t* group_off, const int32_t* group_src,
                    int64_t n_groups, size_t scratch_bytes, int32_t* top_out, uint32_t* bits_out);
int svgr_hit_block(void);
int svgr_hit_chunk(void);

/* Signed distance fields: how far every point is from the outline of every path of the batch, on the same kept edges, point
 * forms and workgroup geometry as the hit-testing entries above (no plan is needed, and one the batch has is left as it is).
 *
 * The arithmetic (csrc/svgr_sdf.h is its one home, compiled for host and device without fused multiply-adds): for an edge
 * (a0, b0) -> (a1, b1) and a finite point (pa, pb), in the coordinate order of svgr_batch_all_edges,
 *     x = a1 - a0;  y = b1 - b0;  len2 = x*x + y*y;  inv = len2 > 0 ? 1.0 / len2 : 0.0          (once per edge)
 *     t = clamp(((pa - a0)*x + (pb - b0)*y) * inv, 0, 1);  qa = a0 + t*x;  qb = b0 + t*y
 *     d2 = (pa - qa)*(pa - qa) + (pb - qb)*(pb - qb)
 * A path's unsigned distance is sqrt(min d2) over its edges (an edge of length zero counts as its point; a path without edges
 * is +inf away).  The sign is the inside predicate above under the path's fill rule: NEGATIVE inside, positive outside; with
 * SVGR_SDF_UNSIGNED the result is the unsigned distance.  A point with a NaN or infinite coordinate is +inf away from
 * everything, and outside.  Then d = min(max(d, -spread), spread); `spread` is +inf or finite and > 0.  With a finite spread the
 * kernel skips the paths out of reach of a workgroup's points; that cannot show in a result as long as every path's edges form
 * closed loops (every vertex ends as many edges as it starts), which is what a fill needs anyway and what every path of the
 * library gives: an open subpath carries its closing line, and that line is part of the outline measured here.
 *
 * Encodings (the low bits of `flags`):
 *     SVGR_SDF_F64   double: the clamped distance
 *     SVGR_SDF_F32   float: (float)(0.5 - d / (2*spread)), in [0, 1], 0.5 on the outline, larger inside
 *     SVGR_SDF_U8    uint8: rint((0.5 - d / (2*spread)) * 255) of the double, ties to even, saturated
 * SVGR_SDF_F32 and SVGR_SDF_U8 need a finite spread.
 *
 * out[i * n_paths + p] is path p's value at point i; with SVGR_SDF_UNION out[i] is the minimum over the paths of their signed
 * clamped distances, encoded.  The union is exact outside every path, and its sign is exact everywhere; INSIDE overlapping
 * paths it is the depth in the deepest single path, not the distance to the union's outline.  A union over no paths is all
 * +spread in its encoding.
 *
 * SVGR_E_INVALID, before anything is launched: points together with a grid or neither; a spread that is NaN or <= 0;
 * SVGR_SDF_F32 or SVGR_SDF_U8 with an infinite spread; unknown flag bits.  SVGR_E_OVERFLOW when n_points * n_paths leaves 31
 * bits (not for a union).  n_points == 0 launches nothing and succeeds.  The results of a pass live in device scratch of at
 * most scratch_bytes (0: 256 MiB; never less than one workgroup's points, a grid's row of tiles) and the points are taken in as
 * many passes as that needs; the results come back behind one wait, in the caller's row-major order.                          */
#define SVGR_SDF_F64 0
#define SVGR_SDF_F32 1
#define SVGR_SDF_U8 2
#define SVGR_SDF_ENCODING_MASK 3
#define SVGR_SDF_UNION 4
#define SVGR_SDF_UNSIGNED 8
int svgr_batch_distance(svgr_batch* batch, const double* points, const int64_t* grid, int64_t n_points, double spread, int flags,
                        size_t scratch_bytes, void* out);

/* Multi-channel distance fields: four values to a point, R, G, B and A, on the kept edges, point forms, passes and encodings of
 * svgr_batch_distance.  A is that entry's signed distance; R, G and B each follow the nearest edge of one colour and report the
 * signed distance to that edge's LINE, so that median(R, G, B) keeps a corner sharp where A rounds it.
 *
 * The paths 0 .. group_off[n_groups] of the batch are dealt into groups: group g, one shape, is the paths group_off[g] ..
 * group_off[g + 1] under one fill rule; colour[p] says which channels path p's edges belong to (bit 0 R, bit 1 G, bit 2 B);
 * orient[g] is +1 or -1, chosen so that orient * ((a1 - a0) * (pb - b0) - (pa - a0) * (b1 - b0)) > 0 inside a well-oriented
 * outline.  Paths behind the last group are ignored.  Only a group's edges TOGETHER need to close.
 *
 * The arithmetic (csrc/svgr_msdf.h is its one home, without fused multiply-adds): with x, y, inv of svgr_batch_distance, rl = len2
 * > 0 ? 1.0 / sqrt(len2) : 0.0, da = pa - a0, db = pb - b0, s = da*x + db*y and t = s * inv (not clamped), an edge of len2 > 0 is a
 * candidate with
 *     t <= 0:     d2c = da*da + db*db,                                    se = s
 *     t >= 1:     d2c = (pa - a1)*(pa - a1) + (pb - b1)*(pb - b1),        se = (pa - a1)*x + (pb - b1)*y
 *     otherwise:  d2c = d2 of svgr_batch_distance,                         se = 0
 *     o = (se*se) * inv;  perp = (x*db - da*y) * rl
 * A channel keeps, among the edges of its colour, the candidate with the smallest d2c; ties go to the smaller o, then to the
 * larger perp, so the edges' order does not matter.  Its value is sdf_clamp(-orient * perp); it is A instead when the channel
 * kept nothing, when the point is not finite, or when the spread is finite and d2c >= spread * spread.  Then, with m = median(R,
 * G, B): if ((m < 0) != (A < 0)) R = G = B = A, so the median's side is exactly A's.  Over the groups every channel takes the
 * minimum; a group out of reach of a workgroup's points is skipped and counts as +spread, which is what it would have given.
 * Without groups, or with groups that hold no path, all four are +spread.
 *
 * out[4 * i + {0, 1, 2, 3}] = R, G, B, A of point i in the encoding of the low bits of `flags` (those of svgr_batch_distance).
 *
 * SVGR_E_INVALID, before anything is launched: points together with a grid or neither; a spread that is NaN or <= 0;
 * SVGR_MSDF_F32 or SVGR_MSDF_U8 with an infinite spread; unknown flag bits; a colour (of any path of the batch) outside 1 .. 7;
 * a group_off that does not begin at 0, does not ascend or ends beyond the batch's paths; an orient that is not +1 or -1; a group
 * whose paths differ in fill rule.  n_points == 0 launches nothing and succeeds.  scratch_bytes as for svgr_batch_distance.   */
#define SVGR_MSDF_F64 0
#define SVGR_MSDF_F32 1
#define SVGR_MSDF_U8 2
#define SVGR_MSDF_ENCODING_MASK 3
int svgr_batch_msdf(svgr_batch* batch, const double* points, const int64_t* grid, int64_t n_points, double spread, int flags,
                    const uint8_t* colour, const int32_t* group_off, const int8_t* orient, int64_t n_groups, size_t scratch_bytes,
                    void* out);

/* Full device pipeline, asynchronous on the context stream, no host read-back:
 * transform+flatten -> bbox -> band binning -> tile kernel (LDS delta-coverage scatter, row scan,
 * fill rule, paint, source-over) -> store.  `out` must hold the output kind's bytes:
 *   canvas kinds: owned_rows x viewport cols x 4 (owned_rows = all rows unless bands are restricted,
 *   then the owned bands packed in order); single-path kinds: bbox rows x cols (x 4).            */
int svgr_batch_render(svgr_batch* batch, svgr_buf* out, int out_kind, unsigned flags);
int64_t svgr_batch_owned_rows(const svgr_batch* batch);
/* The same for a window of the canvas: `window` = {row0, col0, rows, cols} in presentation pixels, inside the batch's
 * viewport (or, without one, inside the union bbox the plan found); `out` holds rows x cols x 4 of the canvas kind.
 * Only the tiles the window touches are worked on and nothing outside it is written: the layer `Layer.compose` returns for
 * a run of fills covers the union of their bboxes, not the viewport (canvas_merge_union, S:366-379).  The pixels are
 * those svgr_batch_render writes at the same positions, bit for bit.  Canvas outputs, unsharded batches.            */
int svgr_batch_render_window(svgr_batch* batch, svgr_buf* out, int out_kind, unsigned flags, const int32_t* window);
/* n windows of the same picture -- `windows` = n x {row0, col0, rows, cols}, outs[i] holds window i -- from ONE geometry pass,
 * drawn side by side: a window of a few dozen tiles takes as long as its heaviest tile, and a document's runs of fills are
 * dozens of such windows.  Everything enqueued on the context's stream before the call is in front of the windows, everything
 * enqueued after it behind them.  Canvas outputs, unsharded batches; not with SVGR_RENDER_TIMED / _DETERMINISTIC. */
int svgr_batch_render_windows(svgr_batch* batch, int64_t n, svgr_buf* const* outs, int out_kind, unsigned flags,
                              const int32_t* windows);

/* Plan (when the batch has no valid plan: a new batch, or one whose transforms / bands were set since) AND render, behind ONE
 * host wait: a frame with new geometry -- the reference's only mode: every `Path.mask` flattens and rasterises from scratch
 * (S:948-957), `scene.render` is timed as a whole (S:3854-3864).  The tile kernel is enqueued right behind the plan's full
 * geometry pass and the pass is validated when the call's single wait returns; a batch planned before takes ONE flatten
 * traversal.  When a speculative capacity did not hold, svgr_batch_plan + svgr_batch_render run instead (same picture).
 * On return the picture is in `out`, the stream has drained and the batch is planned (svgr_batch_get_stats / _bboxes are valid);
 * a batch that was planned already is simply rendered, then waited for.  Same arguments as svgr_batch_render.           */
int svgr_batch_draw(svgr_batch* batch, svgr_buf* out, int out_kind, unsigned flags);

/* HIP-event timings accumulated over the SVGR_RENDER_TIMED renders since the last call
 * (synchronises).  ms_geometry = transform/flatten/bbox/binning kernels, ms_tile = the tile
 * kernel (the coverage+composite pass).                                                         */
int svgr_batch_timings(svgr_batch* batch, int* n_renders, double* ms_total, double* ms_geometry, double* ms_tile);

/* -------------------------------------------------------------------------------------------- */
/* Layer operations on double device images (Layer.image stays in HBM until read)               */
/* bbox arguments are {row0, col0, rows, cols}; images are (rows, cols, channels) row-major      */
/* -------------------------------------------------------------------------------------------- */
/* canvas_merge_union(full=False) step, S:366-377 + S:286: dst(4ch) = src + dst*(1-src_a) on the
 * overlap; `first` copies instead (S:374-375).  src_channels 1 broadcasts (S:283-286).          */
int svgr_layer_over(svgr_ctx* ctx, svgr_buf* dst, const int64_t* dst_bbox, const svgr_buf* src,
                    const int64_t* src_bbox, int src_channels, int first);
/* canvas_merge_intersect, S:382-416: `out` (4ch, bbox = intersection) initialised from `first`
 * (1ch broadcast or 4ch crop), then svgr_layer_in multiplies: out = src * out_alpha (S:290).    */
int svgr_layer_crop4(svgr_ctx* ctx, svgr_buf* out, const int64_t* out_bbox, const svgr_buf* first,
                     const int64_t* first_bbox, int first_channels);
int svgr_layer_in(svgr_ctx* ctx, svgr_buf* out, const int64_t* out_bbox, const svgr_buf* src,
                  const int64_t* src_bbox, int src_channels);
/* Layer.opacity, S:171-175: image * opacity */
int svgr_layer_scale(svgr_ctx* ctx, svgr_buf* img, int64_t n_values, double factor);
/* ... into another buffer (dst may be src): Layer.opacity returns a new layer, and a copy followed by the in-place form
 * reads and writes the image twice */
int svgr_layer_scale_to(svgr_ctx* ctx, svgr_buf* dst, const svgr_buf* src, int64_t n_values, double factor);
/* the clip(0, 1) that ends canvas_merge_at (S:326), in place on n_values doubles */
int svgr_layer_clip01(svgr_ctx* ctx, svgr_buf* img, int64_t n_values);
/* Layer.background, S:166-169: premultiplied linear RGBA image OVER the constant colour rgba[4], in place */
int svgr_layer_background(svgr_ctx* ctx, svgr_buf* img, int64_t n_px, const double* rgba);
/* Layer.convert, S:129-164 + S:471-503, in place on n_px RGBA pixels.
 * ops bitmask applied in this order: 1 = premultiplied->straight, 2 = sRGB->linear,
 * 4 = linear->sRGB, 8 = straight->premultiplied                                                */
int svgr_layer_convert(svgr_ctx* ctx, svgr_buf* img, int64_t n_px, unsigned ops);
/* ... into another buffer (dst may be src) */
int svgr_layer_convert_to(svgr_ctx* ctx, svgr_buf* dst, const svgr_buf* src, int64_t n_px, unsigned ops);
/* Layer.opacity of a layer that still needs its Layer.convert (S:171-175: `convert(pre_alpha=True, ...)`, then image * opacity):
 * both in one pass over n_px RGBA pixels, dst may be src */
int svgr_layer_convert_scale_to(svgr_ctx* ctx, svgr_buf* dst, const svgr_buf* src, int64_t n_px, unsigned ops, double factor);
/* Layer.compose(layers, COMPOSE_OVER) as ONE pass (S:177-207 -> canvas_merge_union, S:366-379): `out` (4ch, bbox = the union) is
 * written whole -- no clear in front, no pass per layer.  Source i is (rows, cols, channels[i]) at src_bboxes[4 i ..]; the first
 * is copied where it covers a pixel (S:374-375), the others go OVER (S:286); pixels no source covers are zero.  ops[i] (or NULL):
 * the svgr_layer_convert ops source i still needs, applied to its pixels as they are read (4-channel sources only).            */
int svgr_layer_compose_over(svgr_ctx* ctx, svgr_buf* out, const int64_t* out_bbox, int64_t n, svgr_buf* const* srcs,
                            const int64_t* src_bboxes, const int32_t* channels, const uint32_t* ops);
/* Layer.compose(layers, COMPOSE_IN) as ONE pass (canvas_merge_intersect, S:382-416): `out` (4ch, bbox = the intersection) =
 * the first source cropped (1ch broadcast), then every other source times the alpha of what is there (S:290), in order; ops as above */
int svgr_layer_compose_in(svgr_ctx* ctx, svgr_buf* out, const int64_t* out_bbox, int64_t n, svgr_buf* const* srcs,
                          const int64_t* src_bboxes, const int32_t* channels, const uint32_t* ops);
/* float64 -> float32 (optionally clipping to [0,1]) for presentation */
int svgr_layer_to_f32(svgr_ctx* ctx, svgr_buf* dst_f32, const svgr_buf* src_f64, int64_t n_values, int clip01);

/* -------------------------------------------------------------------------------------------- */
/* gradient paint servers and Gaussian blur (config 5)                                          */
/* -------------------------------------------------------------------------------------------- */
/* The other canvas_compose modes (S:287-297) on the full union canvas (canvas_merge_union(full=True), S:348-361):
 * out(4ch, bbox ob) = blend(out, src zero-extended), every pixel of ob.  mode: 1 OUT, 3 ATOP, 4 XOR (the reference's
 * COMPOSE_* codes, S:48-51), 5 = arithmetic with k4 = {k1, k2, k3, k4}: clip(k1*src*dst + k2*src + k3*dst + k4, 0, 1).
 * (OVER and IN have their own entry points above; an unknown mode is SVGR_E_INVALID like the ValueError of S:298.)  */
int svgr_layer_blend(svgr_ctx* ctx, svgr_buf* out, const int64_t* ob, const svgr_buf* src, const int64_t* sb, int src_channels,
                     int mode, const double* k4);
/* Layer.color_matrix (S:95-104) in place on a straight-alpha linear RGBA image: clip(px @ M[:, :4].T + M[:, 4], 0, 1);
 * m20 = 4 x 5 row-major host matrix.                                                                            */
int svgr_layer_color_matrix(svgr_ctx* ctx, svgr_buf* img, int64_t n_px, const double* m20);
/* Layer.morphology (S:120-127, pooling S:419-468): min (is_max 0) / max pooling, window ky rows x kx columns, stride 1,
 * no padding: out is (rows - ky + 1, cols - kx + 1, 4).                                                          */
int svgr_layer_morphology(svgr_ctx* ctx, svgr_buf* out, const svgr_buf* src, int64_t rows, int64_t cols, int64_t ky, int64_t kx,
                          int is_max);
/* Filter primitives the reference does not implement (filters.py; DESIGN.md "Filter primitives beyond the reference").  All images
 * are (rows, cols, 4) double, linear RGB; the arithmetic is svgr_core.h's (turb_point, transfer_fn) or written out below, in the
 * order given, without contractions.  Every floating-point parameter of svgr_layer_turbulence, _component_transfer,
 * _convolve_matrix and _lighting must be finite, or the entry returns SVGR_E_INVALID before any launch; every clamp to [0, 1]
 * below sends NaN to 0, so a NaN pixel or intermediate never leaves a primitive (DESIGN.md "Filter primitives at the edges of
 * their values").                                                                                                                */
/* feTurbulence (Filter Effects 1): out (bbox[2] x bbox[3] x 4, straight alpha) at device offset (bbox[0], bbox[1]).  Pixel [R, C]
 * is the device point (bbox[0] + R + 0.5, bbox[1] + C + 0.5); inv_m6 (rows 0-1 of the inverse transform) takes it to the user
 * point (x, y) the noise is evaluated at.  tile = {x, y, width, height} of the stitch tile in user space; the lattice is set up
 * on the host from `seed` (svgr::turb_init).  octaves 0..SVGR_TURBULENCE_MAX_OCTAVES, base frequencies >= 0, fractal: 0 turbulence,
 * 1 fractalNoise; stitch: 0 noStitch, 1 stitch.  With stitch the tile must have width > 0 and height > 0 and keep the stitch state
 * of the last octave within 2^53 (svgr::turb_params_valid).  Defined for every finite point, however large.                     */
#define SVGR_TURBULENCE_MAX_OCTAVES 32
int svgr_layer_turbulence(svgr_ctx* ctx, svgr_buf* out, const int64_t* bbox, const double* inv_m6, double base_fx, double base_fy,
                          const double* tile, int64_t seed, int octaves, int fractal, int stitch);
/* feComponentTransfer in place on a straight-alpha image of n_px pixels.  types[4] (R, G, B, A): 0 identity, 1 table, 2 discrete,
 * 3 linear, 4 gamma; params = 4 x 5 {slope, intercept, amplitude, exponent, offset}; n_values[4] table lengths, `values` the
 * four tables back to back (at most SVGR_TRANSFER_MAX_VALUES in all).                                                          */
#define SVGR_TRANSFER_MAX_VALUES 4096
int svgr_layer_component_transfer(svgr_ctx* ctx, svgr_buf* img, int64_t n_px, const int* types, const double* params,
                                  const int64_t* n_values, const double* values);
/* feConvolveMatrix: out (rows, cols, 4) from src (rows, cols, 4); kernel = order_y x order_x row-major; X = column, Y = row:
 * out[Y][X] = (sum_{I < order_y} sum_{J < order_x} src[Y - target_y + I][X - target_x + J] * kernel[order_y-1-I][order_x-1-J])
 *             / divisor + bias, I outer, J inner.  edge_mode: 0 duplicate, 1 wrap, 2 none (zero).  preserve_alpha 0: all four
 * channels of a premultiplied src, alpha clamped to [0, 1], colour to [0, alpha]; 1: colour of a straight src clamped to [0, 1],
 * alpha copied.  out must not be src.                                                                                          */
#define SVGR_CONVOLVE_MATRIX_MAX_ORDER 32
int svgr_layer_convolve_matrix(svgr_ctx* ctx, svgr_buf* out, const svgr_buf* src, int64_t rows, int64_t cols, const double* kernel,
                               int64_t order_x, int64_t order_y, int64_t target_x, int64_t target_y, double divisor, double bias,
                               int edge_mode, int preserve_alpha);
/* feDisplacementMap: out (premultiplied, bbox out_bbox) from the straight-alpha map (same bbox) and the premultiplied src (bbox
 * src_bbox).  d = scale * (map[x_channel] - 0.5, map[y_channel] - 0.5) in user space, lin4 = {m00, m01, m10, m11} the linear
 * part of the transform: out[R, C] = the src pixel containing (out_bbox[0] + R + 0.5 + (m00 d0 + m01 d1),
 * out_bbox[1] + C + 0.5 + (m10 d0 + m11 d1)), transparent outside src.  Channels 0..3 = R, G, B, A.                            */
int svgr_layer_displacement_map(svgr_ctx* ctx, svgr_buf* out, const int64_t* out_bbox, const svgr_buf* map, const svgr_buf* src,
                                const int64_t* src_bbox, const double* lin4, double scale, int x_channel, int y_channel);
/* feDiffuseLighting / feSpecularLighting: out (out_bbox[2] x out_bbox[3] x 4, the filter region at device offset (out_bbox[0],
 * out_bbox[1])) from the alpha channel of src (bbox src_bbox, premultiplied or straight: alpha is the same), read as 0 outside src;
 * src pixels outside the region are not read.  Frame: d0 = row, d1 = column, z up; pixel [R, C] is the device point
 * (out_bbox[0] + R + 0.5, out_bbox[1] + C + 0.5) at height surface_scale * A.  In this order, per pixel (svgr_core.h:
 * light_normal, light_pixel), without contractions:
 *   1. N = normalize(-ss f0 g0, -ss f1 g1, 1), g0 / g1 the Sobel sums along rows / columns over the 3 x 3 alpha neighbourhood
 *      with the kernel and factor of the pixel's place in the region (Filter Effects 1's table: corners, edges, interior; a
 *      line outside the region weighs 0); a region of one row or one column is flat, N = (0, 0, 1).
 *   2. L: light_kind 0 distant, light_params {L0, L1, L2} (unit, device frame); 1 point, {P0, P1, P2}; 2 spot, {P0, P1, P2,
 *      S0, S1, S2 (unit pointsAt - P), spot exponent, cos of the cone angle (-1: no cone)}.  Point and spot:
 *      L = normalize(P - (d0, d1, ss A)), (0, 0, 1) at P itself.
 *   3. Light colour color3 (linear RGB); spot: times pow(-L.S, spot exponent) where -L.S > 0 and -L.S >= the cone's cos, else 0.
 *   4. specular 0: rgb = clamp(constant max(N.L, 0) colour, 0, 1), alpha 1.  specular 1: H = normalize(L + (0, 0, 1)),
 *      rgb = clamp(constant pow(max(N.H, 0), specular_exponent) colour, 0, 1), alpha = max(r, g, b): premultiplied.
 * out must not be src.                                                                                                        */
int svgr_layer_lighting(svgr_ctx* ctx, svgr_buf* out, const int64_t* out_bbox, const svgr_buf* src, const int64_t* src_bbox,
                        int light_kind, const double* light_params, const double* color3, double surface_scale, double constant,
                        double specular_exponent, int specular);
/* mix-blend-mode (W3C Compositing and Blending Level 1, section 5): the source src (src_bbox, src_channels 1 or 4) blended over
 * the backdrop (backdrop_bbox, backdrop_channels 1 or 4), both premultiplied, zero outside their boxes; a single channel is alpha
 * broadcast to all four.  Per pixel (svgr_core.h: mix_blend_px), Cb = cb / ab and Cs = cs / as (0 where the alpha is 0):
 *   co = cs (1 - ab) + cb (1 - as) + as ab B(Cb, Cs),  ao = as + ab (1 - as);
 * SVGR_BLEND_NORMAL is source-over, co = cs + cb (1 - as), bit for bit svgr_layer_compose_over of the two.
 * Out of place (backdrop is not out): every pixel of out (out_bbox, RGBA) is written.  In place (backdrop is out: 4 channels and
 * out_bbox): only the pixels under the source are read and written, the others keep the backdrop (which is what the formula
 * gives where as = 0).  src must not be out.  An unknown mode or a bad box is SVGR_E_INVALID.                                   */
#define SVGR_BLEND_NORMAL 0
#define SVGR_BLEND_MULTIPLY 1
#define SVGR_BLEND_SCREEN 2
#define SVGR_BLEND_OVERLAY 3
#define SVGR_BLEND_DARKEN 4
#define SVGR_BLEND_LIGHTEN 5
#define SVGR_BLEND_COLOR_DODGE 6
#define SVGR_BLEND_COLOR_BURN 7
#define SVGR_BLEND_HARD_LIGHT 8
#define SVGR_BLEND_SOFT_LIGHT 9
#define SVGR_BLEND_DIFFERENCE 10
#define SVGR_BLEND_EXCLUSION 11
#define SVGR_BLEND_HUE 12         /* 12..15 non-separable: Lum / ClipColor / SetLum / Sat / SetSat, weights 0.3 / 0.59 / 0.11 */
#define SVGR_BLEND_SATURATION 13
#define SVGR_BLEND_COLOR 14
#define SVGR_BLEND_LUMINOSITY 15
int svgr_layer_mix_blend(svgr_ctx* ctx, svgr_buf* out, const int64_t* out_bbox, const svgr_buf* backdrop, const int64_t* backdrop_bbox,
                         int backdrop_channels, const svgr_buf* src, const int64_t* src_bbox, int src_channels, int mode);
/* feTile: out (RGBA, out_bbox) is filled with repeats of the tile tile_bbox of src (RGBA, src_bbox; a bbox is {row0, col0, rows, cols} in device pixels):
 *   out[r, c] = tile[(r - tile_row0) mod tile_rows, (c - tile_col0) mod tile_cols]   (floor modulo: out may start before the tile)
 * where tile is src seen through tile_bbox, transparent black where src does not reach (svgr_core.h: tile_wrap, tile_next,
 * tile_source).  A copy: the values are src's bits, whatever its alpha convention and colour space.  Every pixel of out is
 * written once; out needs no clearing.  With tile_bbox == out_bbox nothing repeats: out is src cropped / zero-extended to
 * out_bbox (what svgr_layer_compose_over with this one source writes too; the filter chain cuts a result to its primitive
 * subregion with that entry).  An empty tile or output is SVGR_E_INVALID; out must not be src.                                */
int svgr_layer_tile(svgr_ctx* ctx, svgr_buf* out, const int64_t* out_bbox, const svgr_buf* src, const int64_t* src_bbox,
                    const int64_t* tile_bbox);
/* Luminance of a straight-alpha RGBA image for RENDER_MASK (S:735): out(n_px doubles) = (rgb . {0.2125, 0.7154, 0.072}) * a */
int svgr_layer_luminance(svgr_ctx* ctx, svgr_buf* out_1ch, const svgr_buf* src_rgba, int64_t n_px);

/* Output stage (canvas_to_png, S:262): dst(n_px x 4 uint8) = round-half-even(src(n_px x 4 double) * 255), the
 * quantisation the reference applies to Layer.convert(pre_alpha=False, linear_rgb=False).image before zlib
 * (S:209-213).  Values outside [0, 255] saturate.  The PNG container itself is written on the host.      */
int svgr_layer_to_rgba8(svgr_ctx* ctx, svgr_buf* dst_u8, const svgr_buf* src_f64, int64_t n_px);

/* Path.fill, gradient branch (S:1021-1047): out(rows, cols, 4) = gradient(pixel centre) * mask(rows, cols),
 * GradLinear.fill S:1553-1563, GradRadial.fill S:1577-1650, grad_spread S:1661-1668, grad_interpolate
 * S:1671-1683.  The host supplies what the reference computes once per fill with numpy: the inverse
 * transforms, vec / vec.vec, the focal-circle scalars and the stops already converted to the target
 * colour space (grad_stops_colorspace, S:1686-1695).                                                */
typedef struct {
    int kind;            /* 1 linear, 2 radial (one circle), 3 radial with a focal circle                    */
    int spread;          /* 0 pad, 1 repeat, 2 reflect                                                       */
    int has_gt;          /* apply gt_m6 (gradientTransform inverse) after user_m6                            */
    int n_stops;         /* >= 1; no cap (lists longer than 32 travel in a device buffer, S:1671-1683)        */
    int excl_enabled;    /* fradius != radius: exclude negative r(t) (S:1642-1644)                           */
    double user_m6[6];   /* pixel centre -> user space: rows 0-1 of transform.invert.m (S:1023-1027)          */
    double gt_m6[6];
    double p0[2], vec[2], vv;                       /* linear: p0, p1 - p0, vec . vec                          */
    double center[2], radius;                       /* radial                                                 */
    double fcenter[2], fradius, cd[2], rd, a, frad_rd, frad2, excl_thresh;   /* focal: S:1619-1624, S:1644      */
    const double* stop_off;                         /* n_stops offsets                                        */
    const double* stop_rgba;                        /* n_stops x 4 premultiplied colours                      */
} svgr_gradient;
int svgr_gradient_fill(svgr_ctx* ctx, const svgr_gradient* g, const svgr_buf* mask, const int64_t* bbox, svgr_buf* out_rgba);
/* Gradient paints inside a batch (canvas outputs): path_grad[p] = index into grads or -1 (solid).  One description per
 * gradient-filled path (user_m6 is the fill's own pixel -> user transform), userSpaceOnUse, at most 32 stops; the tile kernel
 * evaluates it per visible pixel with the code of svgr_gradient_fill and multiplies by the coverage and by path_paint[p]
 * (all ones, or the opacity of an OPACITY node directly above the leaf).  n_grads = 0 removes them.  Call before
 * svgr_batch_plan.  The fills of a document then need no Path.mask + svgr_gradient_fill + Layer.compose round trip each. */
int svgr_batch_set_gradients(svgr_batch* batch, const int32_t* path_grad, int64_t n_grads, const svgr_gradient* grads);
/* GradLinear.fill / GradRadial.fill (S:1553-1563, S:1577-1651): the gradient at n_points caller-supplied coordinates
 * (x, y doubles interleaved; user space, i.e. what Path.fill passes after its own user transform: user_m6 is not
 * applied, so that infinite coordinates arrive as given), no mask; out_rgba receives n_points x 4 doubles.        */
int svgr_gradient_eval(svgr_ctx* ctx, const svgr_gradient* g, const svgr_buf* points, int64_t n_points, svgr_buf* out_rgba);

/* Path.fill, pattern branch (S:1049-1094): out_rgba = pattern tile looked up per pixel * mask.  `tile` is the
 * (rows, cols, 4) double image of the pattern's scene rendered once by the caller (Scene.render under the fill's
 * transform without translation, S:1051-1064); this call does the per-pixel part, S:1066-1094: pixel centre ->
 * inv_m6 -> np.remainder by the cell -> fwd_m6 -> astype(int) -> minus min_xy -> tile pixel clipped to [0, 1]
 * (0 outside the tile), times the coverage.  SVGR_E_INVALID if an offset leaves the pattern canvas (numpy: IndexError). */
typedef struct svgr_pattern {
    double inv_m6[6];      /* repeat transform inverted: presentation pixels -> pattern space (S:1066-1071)      */
    double fwd_m6[6];      /* repeat transform, translation removed: pattern space -> pixels                       */
    double cell[4];        /* Pattern.x, y, width, height                                                         */
    int64_t min_xy[2];     /* integer minimum over the transformed cell corners (S:1084)                          */
    int64_t pat_shape[2];  /* (w + 1, h + 1) of the pattern canvas (S:1088)                                       */
    int64_t tile_bbox[4];  /* tile layer inside that canvas: x - min_x, y - min_y, rows, cols (S:1089)            */
} svgr_pattern;
int svgr_pattern_fill(svgr_ctx* ctx, const svgr_pattern* pattern, const svgr_buf* tile, const svgr_buf* mask,
                      const int64_t* bbox, svgr_buf* out_rgba);

/* SVG <image> (beyond the reference): a raster image as a paint.
 * svgr_image_upload: `rgba` is the caller's (h, w, 4) uint8 image, straight alpha, sRGB as stored.  `levels` receives
 * every mip level as float32x4 premultiplied texels, level 0 first, each level right behind the previous one.  Level 0
 * is byte / 255, sRGB -> linear if linear_rgb (the formula of svgr_layer_convert), times alpha.  Level k + 1 is
 * (ceil(h_k / 2), ceil(w_k / 2)): each texel the mean (summed in double) of its 2 x 2 parents, the last row / column
 * reused on odd sizes; the chain ends at 1 x 1.  The sizes are a function of (h, w) alone: the caller allocates for the
 * sum of the levels' texels (16 bytes each). */
int svgr_image_upload(svgr_ctx* ctx, const uint8_t* rgba, int64_t h, int64_t w, int linear_rgb, svgr_buf* levels);
/* svgr_image_fill: out_rgba = image sampled per pixel * mask, over the pixel grid of bbox (as svgr_pattern_fill).  The
 * pixel centre (row + 0.5, col + 0.5) goes through inv_m6 to image space (u along the image's columns, v along its rows;
 * texel (r, c) covers [c, c + 1) x [r, r + 1)).  smooth: trilinear between levels floor(lod) and floor(lod) + 1 (bilinear,
 * texel centres at + 0.5, clamp to edge; level k at (u, v) * 2^-k; level 0 alone if lod == 0); else the level-0 texel
 * (floor v, floor u), clamped.  The result is double, premultiplied.                                                  */
typedef struct svgr_image {
    double inv_m6[6];      /* presentation pixels -> image space: rows 0-1 of (transform @ paint transform).invert      */
    int64_t height, width; /* level 0 of `levels`                                                                        */
    double lod;            /* 0 <= lod <= n_levels - 1: log2 of the larger image-space step of one pixel                */
    int smooth;            /* 1 trilinear, 0 nearest                                                                    */
} svgr_image;
int svgr_image_fill(svgr_ctx* ctx, const svgr_image* image, const svgr_buf* levels, const svgr_buf* mask, const int64_t* bbox,
                    svgr_buf* out_rgba);

/* Layer.convolve (S:106-118): full 2-D convolution of a (rows, cols, 4) double image with a host (kw, kh)
 * kernel (blur_kernel, S:1903-1944, is built on the host); out is (rows + kw - 1, cols + kh - 1, 4).     */
int svgr_layer_convolve(svgr_ctx* ctx, svgr_buf* out, const svgr_buf* src, int64_t rows, int64_t cols, const double* kernel,
                        int64_t kw, int64_t kh);
/* ... of a source that still needs its Layer.convert (the filter's `source.convert(pre_alpha=False, linear_rgb=True)`, S:1803):
 * src_ops = the svgr_layer_convert ops, applied to the source's pixels as the first pass reads them */
int svgr_layer_convolve_ops(svgr_ctx* ctx, svgr_buf* out, const svgr_buf* src, int64_t rows, int64_t cols, const double* kernel,
                            int64_t kw, int64_t kh, unsigned src_ops);

/* -------------------------------------------------------------------------------------------- */
/* Path.stroke (S:1105-1180), host side: stroke outline of a path as a fill path.               */
/* Input and output use the reference's segment codes (S:865-872) with 8 doubles per segment    */
/* (points interleaved x, y; unused slots 0) and per-subpath segment counts, the layout of       */
/* Path.from_segments.  Quadratic / arc segments must be converted to cubics by the caller      */
/* (bezier2_to_bezier3 S:2182, arc_to_bezier3 S:2355, exactly as Path.stroke does, S:1133-1140). */
/* Offsetting: line_offset S:2328, bezier3_offset S:2113-2179; joins S:1495-1522 (miter limit 4), */
/* caps S:1466-1492.  Output segments are LINE (2 points), QUAD (3, round joins) or CUBIC (4).   */
/* -------------------------------------------------------------------------------------------- */
#define SVGR_PATH_LINE 0
#define SVGR_PATH_QUAD 1
#define SVGR_PATH_CUBIC 2
#define SVGR_PATH_ARC 3
#define SVGR_PATH_CLOSED 4
#define SVGR_PATH_UNCLOSED 5
#define SVGR_CAP_BUTT 0    /* STROKE_CAP_BUTT (default, S:1468) */
#define SVGR_CAP_ROUND 1
#define SVGR_CAP_SQUARE 2
#define SVGR_JOIN_MITER 0  /* STROKE_JOIN_MITER (default, S:1497) */
#define SVGR_JOIN_ROUND 1
#define SVGR_JOIN_BEVEL 2
typedef struct svgr_stroke_out svgr_stroke_out;
int svgr_path_stroke(const int32_t* seg_types, const double* seg_params, const int32_t* subpath_sizes, int64_t n_subpaths,
                     double width, int linecap, int linejoin, svgr_stroke_out** out);
int svgr_stroke_out_counts(const svgr_stroke_out* s, int64_t* n_segs, int64_t* n_subpaths);
int svgr_stroke_out_copy(const svgr_stroke_out* s, int32_t* seg_types, double* seg_params, int32_t* subpath_sizes);
void svgr_stroke_out_free(svgr_stroke_out* s);

/* Path.dash (beyond the reference): stroke-dasharray / stroke-dashoffset applied to a path in the layout above, in front of
 * svgr_path_stroke.  Every "on" dash comes back as one open subpath (its pieces in order, then a PATH_UNCLOSED line from its
 * end to its start); a closed subpath that begins and ends inside a dash gets that dash as ONE subpath, and stays closed when
 * a single dash covers it.  Lines (PATH_LINE, PATH_CLOSED) and cubics are dashed, a PATH_UNCLOSED line is not part of the
 * outline; quadratics and arcs are converted by the caller.  `dashes`: n_dashes lengths, used twice over when their count is
 * odd (at most 64 entries then); `offset` may be negative or beyond the period; every subpath restarts the pattern.
 * `path_length` > 0 (SVG pathLength) multiplies the dashes and the offset by (measured length of all subpaths) / path_length.
 * An empty list, a negative or non-finite entry, a zero sum or a list without a gap is a solid stroke: the input comes back
 * unchanged (no device work).  Arc length: a line is sqrt(dx^2 + dy^2); a cubic is 32 equal parameter sub-intervals of 4-point
 * Gauss-Legendre quadrature each (within 5.5e-5 relative of the true length on near-cusp cubics, 1e-14 on smooth ones).
 * SVGR_E_INVALID, before anything is launched, for a coordinate that is not finite or lies beyond +-1e150 (its square would
 * leave the doubles) or an unknown segment type.  SVGR_E_OVERFLOW when the result leaves the 32-bit counts of svgr_stroke_out
 * or one segment alone has more than 2^20 pieces: that is known from the counting kernels, so those have run; nothing is
 * launched after them.  SVGR_E_STATE should the placing kernels meet a place outside the result (the tables disagree: a
 * defect, never an input's doing).  The result is identical from run to run.
 * svgr_dash_scan_segments: the number of segments one workgroup of the dasher's scans covers (its launch seam).            */
int svgr_path_dash(svgr_ctx* ctx, const int32_t* seg_types, const double* seg_params, const int32_t* subpath_sizes,
                   int64_t n_subpaths, const double* dashes, int64_t n_dashes, double offset, double path_length,
                   svgr_stroke_out** out);   /* read with svgr_stroke_out_counts / _copy / _free */
int svgr_dash_scan_segments(void);

/* Path.vertices (beyond the reference): the vertices of a path in the layout above with a unit direction each, for
 * marker-start / marker-mid / marker-end (SVG 2 11.6; directions: SVG 1.1 F.5).  `seg_vertex` (may be NULL: every segment):
 * non-zero where a segment ends at a vertex of the author's path -- the cubics made from one arc carry 0 on all but the last.
 * A trailing PATH_UNCLOSED line is not part of the outline; PATH_CLOSED is a line.  The vertices of a subpath: the start point
 * of its first segment, then the end point of every flagged segment; positions are copies of the input.  Per vertex the
 * result holds x, y, ux, uy and a kind: 0 the first vertex of the path, 2 the last one (of a path with more than one), 1
 * every other.  Segment directions: a line P1 - P0; a cubic the first of P1 - P0, P2 - P0, P3 - P0 that is not (0, 0) at its
 * start and the first of P3 - P2, P3 - P1, P3 - P0 at its end; a segment without one takes both from the end of the nearest
 * earlier segment of its subpath that has one, else from the start of the nearest later one, else (1, 0); no wrap-around.
 * Vertex direction: the first vertex of an open subpath its outgoing, the last its incoming direction; every other one, and
 * both end vertices of a closed subpath (incoming: the closing segment's end, outgoing: the first segment's start),
 * normalise(u_in + u_out), or u_in turned by +90 degrees, (-u_in.y, u_in.x), when neither component of the sum exceeds 2^-40.
 * SVGR_E_INVALID, before anything is launched, for a coordinate that is not finite or lies beyond +-1e150 or an unknown
 * segment type; SVGR_E_OVERFLOW, likewise, when the vertex count leaves 32 bits.  A path without vertices gives an empty
 * result and launches nothing (ctx may then be NULL).  SVGR_E_STATE should a kernel meet a slot outside the result (a
 * defect, never an input's doing).  The result is identical from run to run.
 * svgr_marker_block_segments: segments per workgroup of the pass's own kernels; its scans are the dasher's
 * (svgr_dash_scan_segments).                                                                                             */
typedef struct svgr_marker_out svgr_marker_out;
int svgr_path_markers(svgr_ctx* ctx, const int32_t* seg_types, const double* seg_params, const int32_t* seg_vertex,
                      const int32_t* subpath_sizes, int64_t n_subpaths, svgr_marker_out** out);
int svgr_marker_out_counts(const svgr_marker_out* m, int64_t* n_vertices);
int svgr_marker_out_copy(const svgr_marker_out* m, double* xyuv /* 4 per vertex */, int32_t* kind);
void svgr_marker_out_free(svgr_marker_out* m);
int svgr_marker_block_segments(void);

/* Path.length / Path.point_at and text on a path (beyond the reference; <textPath>, SVG 1.1 10.13): the frame -- point and unit
 * tangent -- of a path in the layout above at arc lengths, and glyph outlines placed in such frames.  The metric is the
 * dasher's: a line's length is sqrt(dx^2 + dy^2), a cubic's the sum of 32 sub-intervals of 4-point Gauss-Legendre; the length
 * runs over all subpaths in order, a move between subpaths has length 0, PATH_CLOSED is a line, a PATH_UNCLOSED line has
 * length 0.  cum[i] is the length in front of segment i, L the total.
 * svgr_path_sample: for each of the `n` arc lengths `s` the result holds x, y, ux, uy (4 per query) and inside = 0 <= s <= L;
 * outside that range s is clamped for the point.  The segment of s is the last one of non-zero length with cum[i] <= s, for
 * s = L the last one of non-zero length, at its end.  A line gives P0 + d r / len and d normalised; a cubic B(t) by de
 * Casteljau and B'(t) normalised at the t of the dasher's inversion -- or, where B'(t) is exactly (0, 0), the segment's
 * direction by svgr_path_markers' rule at its start (t < 0.5) or its end.  A path with L = 0 reports inside = 0 everywhere
 * (the point is then the start of its first segment, the direction (1, 0)).  n = 0 returns only the length
 * (`total_length_out`, may be NULL).
 * svgr_path_place_glyphs: `n_inst` glyph instances on the path.  The atlas holds the segments of each distinct glyph once, in
 * the same layout as a path's, relative to the glyph's origin: glyph g owns atlas segments [glyph_seg_off[g],
 * glyph_seg_off[g + 1]).  Instance k shows glyph inst_glyph[k]; with (P, u) the frame at inst_s_mid[k], an outline point (x, y)
 * goes to  X = Px + ux (x - h) - uy (y + dy),  Y = Py + uy (x - h) + ux (y + dy),  h = inst_half[k], dy = inst_dy[k].
 * `params_out` receives 8 doubles per output segment, in instance order and within an instance in atlas order (unused slots
 * of a line 0); the caller knows every slot, types and subpath sizes from its own tables.  An instance whose s_mid is not inside
 * is hidden: visible_out[k] = 0, and its slots hold 0.
 * Both: SVGR_E_INVALID, before anything is launched, for a coordinate that is not finite or lies beyond +-1e150, an unknown
 * segment type, a glyph id out of range, glyph offsets that decrease, or a query / advance / shift that is not finite;
 * SVGR_E_OVERFLOW, likewise, when a count leaves 32 bits.  A path without segments launches nothing (ctx may then be NULL):
 * L = 0, every flag 0.  SVGR_E_STATE should a lane meet a slot outside the result (a defect, never an input's doing).  The
 * result is identical from run to run.
 * svgr_textpath_block: queries / output segments per workgroup of the pass's own kernels; its scan is the dasher's
 * (svgr_dash_scan_segments).                                                                                             */
int svgr_path_sample(svgr_ctx* ctx, const int32_t* seg_types, const double* seg_params, const int32_t* subpath_sizes,
                     int64_t n_subpaths, const double* s, int64_t n, double* xyuv_out /* 4 per query */, int32_t* inside_out,
                     double* total_length_out);
int svgr_path_place_glyphs(svgr_ctx* ctx, const int32_t* seg_types, const double* seg_params, const int32_t* subpath_sizes,
                           int64_t n_subpaths, const int32_t* atlas_types, const double* atlas_params,
                           const int32_t* glyph_seg_off /* n_glyphs + 1 */, int64_t n_glyphs, const int32_t* inst_glyph,
                           const double* inst_s_mid, const double* inst_half, const double* inst_dy, int64_t n_inst,
                           double* params_out /* 8 per output segment */, int32_t* visible_out, double* total_length_out);
int svgr_textpath_block(void);

/* TrueType outlines (beyond the reference; the `glyf` table of a .ttf): the contours of simple glyphs -- points in font units
 * with an on-curve flag each -- as a path in the layout above.  Table parsing, hinting-free, is the caller's (truetype.py);
 * composite glyphs arrive flattened into parts.
 * The atlas holds every distinct simple glyph once: `pt_xy` (2 int16 per point), `pt_on` (non-zero: on the curve),
 * `contour_off` (n_contours + 1, in points: contour c owns the points [contour_off[c], contour_off[c + 1])) and
 * `glyph_contour_off` (n_glyphs + 1, in contours).  Part k shows glyph part_glyph[k]: a point (x, y) goes to
 * x' = (m00 x + m10 y) + dx, y' = (m01 x + m11 y) + dy with part_m[6 k ..] = m00, m01, m10, m11, dx, dy, then to
 * X = (x' + pen) sx, Y = y' sy -- each product and sum rounded on its own, in this order.
 * A contour p[0 .. n-1], prev and next cyclic within it: n < 2 gives nothing, no subpath either.  Else an off-curve p[i] gives
 * the quadratic from (prev if prev is on the curve, else the midpoint of prev and p[i]) over p[i] to (next if next is on the
 * curve, else the midpoint of p[i] and next); an on-curve p[i] with an on-curve next gives the line p[i] -> next; an on-curve
 * p[i] with an off-curve next gives nothing.  The segments stand in point order and form a closed chain; behind them comes one
 * PATH_CLOSED line of length 0 at the chain's start -- p[0] if it is on the curve, else p[n-1] if that is, else their midpoint
 * -- which is what the path reader leaves for an outline written `... z`.  Midpoints are (a + b) * 0.5 in font units.  A
 * quadratic P0 Q P1 is stored as the PATH_CUBIC P0, (1/3) P0 + (2/3) Q, (2/3) Q + (1/3) P1, P1, made from the transformed
 * points, two products and one sum each; a PATH_LINE has its slots 4..7 zero.
 * The result holds types, params and one subpath size per contour with n >= 2, in part order, then contour order.  One
 * launch, one lane per pair of a part and a point of its glyph; the slot of every segment is a matter of the flags alone and
 * is worked out on the host during the validation walk.
 * SVGR_E_INVALID, before anything is launched, for offsets that decrease, do not begin at 0 or do not end at the sizes given,
 * a part's glyph id out of range, or a matrix entry, pen or scale that is not finite or lies beyond +-1e150; SVGR_E_OVERFLOW,
 * likewise, when a count leaves 32 bits.  Without lanes -- no parts, parts of empty glyphs only -- or without segments the
 * result is empty and nothing is launched (ctx may then be NULL).  SVGR_E_STATE should a lane meet a slot outside the result
 * (a defect, never an input's doing).  The result is identical from run to run.
 * svgr_glyf_block: lanes per workgroup of the pass's kernel.                                                               */
int svgr_glyf_outline(svgr_ctx* ctx, const int16_t* pt_xy /* 2 per point */, const uint8_t* pt_on, int64_t n_points,
                      const int32_t* contour_off /* n_contours + 1 */, int64_t n_contours,
                      const int32_t* glyph_contour_off /* n_glyphs + 1 */, int64_t n_glyphs, const int32_t* part_glyph,
                      const double* part_m /* 6 per part */, const double* part_pen, const double* part_sx,
                      const double* part_sy, int64_t n_parts,
                      svgr_stroke_out** out);   /* read with svgr_stroke_out_counts / _copy / _free */
int svgr_glyf_block(void);

/* Variable fonts (beyond the reference; the `gvar` table of a .ttf): the outlines above at one instance of the font.  Table
 * parsing, axis normalisation and the tuples' scalars are the caller's (truetype_var.py); tuples whose scalar is 0, phantom
 * points and the deltas of composite glyphs' components never arrive here.
 * The atlas is svgr_glyf_outline's.  Glyph g owns the tuples [glyph_tuple_off[g], glyph_tuple_off[g + 1]) in the file's order;
 * tuple t has the scalar tuple_scalar[t] and the entries [tuple_pt_off[t], tuple_pt_off[t + 1]): tp_index[k], a point's index
 * within its glyph, strictly increasing within the tuple, and its delta tp_dxy[2 k], tp_dxy[2 k + 1].
 * The delta of point i of a contour that owns the glyph-local indices [f, l], in one tuple: the tuple's entries with an index
 * in [f, l] are the contour's touched points.  None gives (0, 0); i among them gives its stored delta; else, with p the touched
 * point before i (wrapping to the contour's last touched one) and q the one after (wrapping to the first), per axis and in
 * double, from the int16 coordinates c_p, c_q, c_i and the deltas d_p, d_q: c_p == c_q gives d_p when d_p == d_q, else 0;
 * otherwise, the pair ordered so that c_1 < c_2: d_1 when c_i <= c_1, d_2 when c_i >= c_2, else
 * d_1 + (c_i - c_1) * ((d_2 - d_1) / (c_2 - c_1)), every operation rounded on its own.  D(i) starts at 0.0 and takes
 * D = D + scalar_t * delta_t(i) tuple by tuple; the varied point is (double)int16 + D, never rounded to an integer.
 * svgr_gvar_deltas: D of every atlas point, 2 doubles per point, into `pt_dxy_out`; one launch, one lane per point.  Without
 * points, or without any tuple, the result is zeros and nothing is launched (ctx may then be NULL).
 * svgr_glyf_outline_var: svgr_glyf_outline of the varied points: the delta pass, then the outline pass, on the context's
 * stream -- two launches, one upload, one download, one wait; the deltas stay on the device.  A midpoint of two varied points
 * is (a + b) * 0.5 of the two doubles.  Without any tuple it is svgr_glyf_outline, bytes and launch count.
 * Both: SVGR_E_INVALID, before anything is launched, for what svgr_glyf_outline refuses and for offsets (glyph_tuple_off,
 * tuple_pt_off) that decrease, do not begin at 0 or do not end at the counts given, a tp_index that does not increase strictly
 * within its tuple or is not below its glyph's point count, or a scalar that is not finite or lies outside [-1, 1];
 * SVGR_E_OVERFLOW, likewise, when a count exceeds INT32_MAX / 2.  SVGR_E_STATE should a lane meet a point or slot outside
 * its tables (a defect, never an input's doing).  The result is identical from run to run.
 * svgr_gvar_block: lanes (= atlas points) per workgroup of the delta pass's kernel.                                        */
int svgr_gvar_deltas(svgr_ctx* ctx, const int16_t* pt_xy /* 2 per point */, int64_t n_points,
                     const int32_t* contour_off /* n_contours + 1 */, int64_t n_contours,
                     const int32_t* glyph_contour_off /* n_glyphs + 1 */, int64_t n_glyphs,
                     const int32_t* glyph_tuple_off /* n_glyphs + 1 */, const double* tuple_scalar, int64_t n_tuples,
                     const int32_t* tuple_pt_off /* n_tuples + 1 */, const int32_t* tp_index, const int16_t* tp_dxy /* 2 per entry */,
                     int64_t n_entries, double* pt_dxy_out /* 2 per point */);
int svgr_glyf_outline_var(svgr_ctx* ctx, const int16_t* pt_xy, const uint8_t* pt_on, int64_t n_points, const int32_t* contour_off,
                          int64_t n_contours, const int32_t* glyph_contour_off, int64_t n_glyphs, const int32_t* part_glyph,
                          const double* part_m, const double* part_pen, const double* part_sx, const double* part_sy,
                          int64_t n_parts, const int32_t* glyph_tuple_off, const double* tuple_scalar, int64_t n_tuples,
                          const int32_t* tuple_pt_off, const int32_t* tp_index, const int16_t* tp_dxy, int64_t n_entries,
                          svgr_stroke_out** out);   /* read with svgr_stroke_out_counts / _copy / _free */
int svgr_gvar_block(void);

/* OpenType / CFF outlines (beyond the reference; the `CFF ` table of an .otf): the contours a Type 2 charstring draws --
 * absolute points in font units, in double, with a kind each -- as a path in the layout above.  Table parsing and the
 * charstring machine, hinting-free, are the caller's (opentype_cff.py); CFF has no composites, a part is a placed glyph.
 * The atlas holds every distinct glyph once: `pt_xy` (2 doubles per point), `pt_kind` (0 MOVE, 1 LINE, 2 C1, 3 C2, 4 CURVE: a
 * cubic's two control points and its end point), `contour_off` (n_contours + 1, in points) and `glyph_contour_off`
 * (n_glyphs + 1, in contours).  The parts, and the transform of a point -- x' = (m00 x + m10 y) + dx, y' = (m01 x + m11 y) + dy,
 * X = (x' + pen) sx, Y = y' sy, each product and sum rounded on its own -- are svgr_glyf_outline's.
 * Within a contour p[first .. last] a LINE point a gives the PATH_LINE p[a-1] -> p[a] (slots 4..7 zero), a CURVE point a gives
 * the PATH_CUBIC p[a-3], p[a-2], p[a-1], p[a]; MOVE, C1 and C2 give nothing.  The segments stand in point order; behind the last
 * segment of a contour with at least 2 points comes one PATH_CLOSED line from p[last] to p[first] -- of length 0 when the
 * charstring returned to its start itself, which is what svgr_glyf_outline leaves too.  A contour of a lone MOVE gives nothing,
 * no subpath either.
 * The result holds types, params and one subpath size per contour with segments, in part order, then contour order.  One
 * launch, one lane per OUTPUT segment: which points emit is a matter of the kinds alone, and the table of the atlas'
 * segments -- per segment its end point, or its contour for a closing line -- is made on the host during the validation walk.
 * SVGR_E_INVALID, before anything is launched, for what svgr_glyf_outline refuses for offsets and parts, a contour whose
 * first kind is not MOVE or that holds a second MOVE, a C1 that C2 and CURVE do not follow, a C2 or CURVE without its
 * predecessors, a kind above 4, or a coordinate that is not finite or lies beyond +-1e150; SVGR_E_OVERFLOW, likewise, when a
 * count exceeds INT32_MAX / 2.  Without segments -- no parts, parts of empty glyphs, lone MOVEs only -- the result is empty and
 * nothing is launched (ctx may then be NULL).  SVGR_E_STATE should a lane meet an index outside its tables (a defect, never
 * an input's doing).  The result is identical from run to run.
 * svgr_cff_block: lanes (= output segments) per workgroup of the pass's kernel.                                             */
int svgr_cff_outline(svgr_ctx* ctx, const double* pt_xy /* 2 per point */, const uint8_t* pt_kind, int64_t n_points,
                     const int32_t* contour_off /* n_contours + 1 */, int64_t n_contours,
                     const int32_t* glyph_contour_off /* n_glyphs + 1 */, int64_t n_glyphs, const int32_t* part_glyph,
                     const double* part_m /* 6 per part */, const double* part_pen, const double* part_sx,
                     const double* part_sy, int64_t n_parts,
                     svgr_stroke_out** out);   /* read with svgr_stroke_out_counts / _copy / _free */
int svgr_cff_block(void);

/* PNG scanlines (read_png, host side): reverse the filters None / Sub / Up / Average / Paeth of `rows` filtered rows of
 * 1 + row_bytes bytes each (filter type first) into rows * row_bytes bytes of dst.  bytes_per_pixel is the filter's
 * stride (1 below 8 bits per pixel).  SVGR_E_INVALID on a filter type above 4 or when src_bytes is short; src is never
 * read past src_bytes. */
int svgr_png_unfilter(const uint8_t* src, int64_t src_bytes, int64_t rows, int64_t row_bytes, int64_t bytes_per_pixel,
                      uint8_t* dst);

/* JPEG (read_jpeg): the caller reads the markers; the entropy-coded data is decoded on the host and the pixels are made on
 * the device.  Both entries describe the frame the same way and lay its coefficients out the same way: component after
 * component, each a row-major grid of 8 x 8 blocks of 64 int16 in natural (row-major) order, the grid padded to whole MCUs --
 * with hmax, vmax the largest sampling factors, mcus_x = ceil(width / (8 hmax)), mcus_y = ceil(height / (8 vmax)), component
 * i has mcus_x * h[i] blocks per row and mcus_y * v[i] rows of them. */
#define SVGR_JPEG_GREY 0   /* one component */
#define SVGR_JPEG_YCBCR 1  /* three: JFIF Y, Cb, Cr */
#define SVGR_JPEG_RGB 2    /* three: R, G, B as they are */
typedef struct svgr_jpeg_frame {
    int32_t width, height; /* 1 .. 65535 */
    int32_t n_comp;        /* 1 or 3 */
    int32_t h[3], v[3];    /* sampling factors, 1 or 2 (1 for a lone component) */
    int32_t colour;        /* SVGR_JPEG_* (svgr_jpeg_decode only) */
} svgr_jpeg_frame;
typedef struct svgr_jpeg_scan {
    svgr_jpeg_frame frame;
    int32_t progressive;        /* 0: SOF0 / SOF1, 1: SOF2 */
    int32_t restart_interval;   /* MCUs between restart markers (DRI), 0: none */
    int32_t n_scan;             /* components in this scan */
    int32_t scan_comp[3];       /* their indices in the frame, ascending */
    int32_t dc_table[3], ac_table[3];   /* Huffman table of each, 0 .. 3 */
    int32_t ss, se, ah, al;     /* spectral selection and successive approximation (0, 63, 0, 0 when not progressive) */
} svgr_jpeg_scan;
/* svgr_jpeg_entropy (host only): decode the entropy-coded segment `data` of one scan (from behind the SOS header up to, not
 * including, the next marker that is not RSTn; stuffed bytes and restart markers still in it) into `coef`, which holds
 * n_coef int16 -- the whole frame -- is zero before the frame's first scan and is carried from scan to scan.  The Huffman
 * tables in force: huff_counts[8][16] codes per length and huff_symbols[8][256] in code order, DC tables 0-3 then AC tables
 * 0-3 (all-zero counts: not defined).  Returns SVGR_OK, SVGR_E_INVALID for a description that makes no sense, or one of the
 * SVGR_JPEG_* statuses below for data that does not decode; nothing is read or written outside the arrays. */
#define SVGR_JPEG_TRUNCATED 1    /* the data ended before the scan did */
#define SVGR_JPEG_BAD_CODE 2     /* a Huffman table that is not a prefix code, or bits that are no code of the table */
#define SVGR_JPEG_BAD_RESTART 3  /* the restart marker due is missing or out of sequence */
#define SVGR_JPEG_BAD_INDEX 4    /* a run that leads past the last coefficient of the block or band */
int svgr_jpeg_entropy(const svgr_jpeg_scan* scan, const uint8_t* huff_counts, const uint8_t* huff_symbols, const uint8_t* data,
                      int64_t n_bytes, int16_t* coef, int64_t n_coef);
/* svgr_jpeg_decode: the pixels of a frame from its coefficients (host array, n_coef int16 as above) and each component's
 * quantisation table (quant[n_comp][64], natural order).  Per sample: coefficient * table entry, inverse DCT, + 128, clamp
 * to 0 .. 255.  Per pixel: subsampled components are brought to full resolution with the centred triangle filter (3/4, 1/4
 * per axis, edge sample repeated), YCbCr goes through the JFIF matrix, alpha is 255.  All of it is integer arithmetic
 * (csrc/svgr_core.h), so the result is defined to the bit.  out_rgba receives (height, width, 4) uint8, straight alpha,
 * sRGB as stored: what svgr_image_upload takes. */
int svgr_jpeg_decode(svgr_ctx* ctx, const svgr_jpeg_frame* frame, const int16_t* coef, int64_t n_coef, const uint16_t* quant,
                     svgr_buf* out_rgba);

/* JPEG output (write_jpeg): the same split the other way round -- the device makes the coefficients, the host codes them,
 * the caller writes the markers.
 * svgr_jpeg_encode: the quantised coefficients of a frame from src_rgba8, (height, width, 4) uint8 on the device as
 * svgr_layer_to_rgba8 writes them (alpha is ignored).  frame->colour is SVGR_JPEG_YCBCR (three components, h[0] x v[0] the
 * luma sampling factors, 1 x 1 for both chroma components: 4:4:4, 4:2:2, 4:4:0, 4:2:0) or SVGR_JPEG_GREY (one component, Y
 * alone).  Per pixel: the JFIF matrix in 16-bit fixed point, rounded half up, clamped.  Per chroma sample: the mean of the
 * pixels it covers, rounded half up.  The planes are padded to whole MCUs by repeating the last column and row.  Per block:
 * - 128, forward DCT, each value divided by its table entry (quant[n_comp][64], natural order, entries 1 .. 255) and rounded
 * half away from zero, clamped to -1024 .. 1023 (DC) and -1023 .. 1023 (AC).  Integer arithmetic (csrc/svgr_core.h): the
 * result is defined to the bit.  coef_out is a host array of n_coef int16 in the layout above -- what svgr_jpeg_entropy_encode
 * and svgr_jpeg_decode take.  SVGR_E_INVALID for any other colour model or sampling, a short buffer, an n_coef that is not
 * the frame's, or a table entry outside 1 .. 255. */
int svgr_jpeg_encode(svgr_ctx* ctx, const svgr_jpeg_frame* frame, const svgr_buf* src_rgba8, const uint16_t* quant,
                     int16_t* coef_out, int64_t n_coef);
/* svgr_jpeg_entropy_encode (host only): the entropy-coded segment of one baseline sequential scan (progressive 0, ss 0, se 63,
 * ah 0, al 0) of the frame's coefficients, svgr_jpeg_entropy's inverse: described the same way, tables in the same convention.
 * A scan of all three components is interleaved (MCU by MCU, each component's h x v blocks in turn), a scan of one component
 * walks its own blocks.  DC is coded as the difference from the component's last DC, AC as run / size pairs with ZRL and EOB;
 * an FF byte is followed by a stuffed 00 and the last byte is filled with one bits.  With a restart_interval, RSTn goes
 * between the intervals and the predictors start again.  At most out_cap bytes are written to out; *n_bytes always receives
 * the segment's full length, and the status is SVGR_JPEG_NO_ROOM when that is more than out_cap.  SVGR_JPEG_BAD_CODE when a
 * table is no prefix code or has no code for a symbol the data needs (a DC difference beyond +-2047 and an AC value beyond
 * +-1023 need symbols no baseline table has). */
#define SVGR_JPEG_NO_ROOM 5      /* the output buffer is too small */
int svgr_jpeg_entropy_encode(const svgr_jpeg_scan* scan, const uint8_t* huff_counts, const uint8_t* huff_symbols,
                             const int16_t* coef, int64_t n_coef, uint8_t* out, int64_t out_cap, int64_t* n_bytes);
/* svgr_jpeg_symbol_counts (host only): how often the same walk uses each symbol, for tables made to measure: counts[8][256],
 * DC tables 0-3 then AC tables 0-3 as the scan assigns them to its components; the caller zeroes it (counts add up over calls). */
int svgr_jpeg_symbol_counts(const svgr_jpeg_scan* scan, const int16_t* coef, int64_t n_coef, int64_t* counts);

/* PNG output on the device (Layer.write_png(encoder="device")): the scanline filters and the deflate stream of an 8-bit RGBA
 * image; the caller writes the container (signature, IHDR, IDAT, IEND, the CRCs).
 * svgr_png_filter: out_filtered (device, rows * (1 + 4 * cols) bytes) <- the filtered scanlines of src_rgba8 (device, rows *
 * cols * 4 bytes as svgr_layer_to_rgba8 writes them): per row the filter type, then its bytes under PNG 1.2 section 6 (Sub,
 * Up, Average, Paeth with the tie order a, b, c, modulo 256; the row above row 0 and the pixel left of column 0 are zero).
 * `filter` forces one type, or SVGR_PNG_FILTER_ADAPTIVE chooses per row by libpng's heuristic: the type whose filtered bytes have
 * the smallest sum of min(v, 256 - v), a tie going to the lower type.  Enqueued on the context's stream, no wait.
 * SVGR_E_INVALID for an empty or oversized image, an unknown filter, a short buffer, or out_filtered == src_rgba8.             */
#define SVGR_PNG_FILTER_NONE 0
#define SVGR_PNG_FILTER_SUB 1
#define SVGR_PNG_FILTER_UP 2
#define SVGR_PNG_FILTER_AVERAGE 3
#define SVGR_PNG_FILTER_PAETH 4
#define SVGR_PNG_FILTER_ADAPTIVE 5
int svgr_png_filter(svgr_ctx* ctx, const svgr_buf* src_rgba8, int64_t rows, int64_t cols, int filter, svgr_buf* out_filtered);
/* svgr_deflate: a complete zlib stream (78 01, the deflate blocks, Adler-32) of the first n_bytes of src (device) into out (host).
 * The input is cut into chunks of svgr_deflate_chunk() bytes, one workgroup and one block each; matches reach back across the
 * chunks (distance <= 32768) and are cut at their chunk's end; every chunk but the last ends with an empty stored block, so a
 * chunk begins on a byte boundary.  One code pair serves the whole stream: SVGR_DEFLATE_DYNAMIC counts the symbols on the device,
 * builds length-limited codes on the host (one round trip of 316 counts) and repeats the block header in every chunk;
 * SVGR_DEFLATE_FIXED uses the fixed code of RFC 1951.  Every code written is complete.  The tokens, and so the bytes, are defined
 * sequentially (csrc/svgr_deflate.h) and identical from run to run.  n_bytes == 0 is valid (src may then hold nothing).  At most
 * out_cap bytes are written to out; *n_out always receives the stream's full length, and the status is SVGR_DEFLATE_NO_ROOM when
 * that is more than out_cap (nothing is written then).  SVGR_E_INVALID for a negative or oversized (> 5 GiB) n_bytes, a short
 * src or an unknown mode.  Waits for the device.
 * svgr_deflate_chunk: the bytes of one chunk (the launch seam of the deflate kernels).                                          */
#define SVGR_DEFLATE_FIXED 0
#define SVGR_DEFLATE_DYNAMIC 1
#define SVGR_DEFLATE_NO_ROOM 5   /* the output buffer is too small */
int svgr_deflate(svgr_ctx* ctx, const svgr_buf* src, int64_t n_bytes, int huffman, uint8_t* out, int64_t out_cap, int64_t* n_out);
int svgr_deflate_chunk(void);

/* PNG sample formats (color= and depth= of Layer.write_png; csrc/svgr_png.h has the arithmetic): the colour types 0 grey, 2 RGB,
 * 4 grey + alpha and 6 RGBA at depth 8 or 16, bpp = channels * depth / 8 bytes a pixel.  svgr_deflate takes the filtered stream
 * as it takes svgr_png_filter's.
 * svgr_png_samples: dst (device, rows * cols * bpp bytes) <- the packed samples of src (device), pixel after pixel, a pixel's
 * samples in the file's order, a 16-bit sample most significant byte first.  src_kind says what src holds:
 *   RGBA_F64  rows * cols * 4 doubles, straight alpha, sRGB-encoded (svgr_layer_convert's output; a layer that is to lose its
 *             alpha has been put over its background by the caller)
 *   MASK_F64  rows * cols doubles, one channel; colour type 0 only
 *   RGBA_U8   rows * cols * 4 bytes R, G, B, A; each is v / 255.0
 * A sample is rint(v * M) saturated to [0, M], NaN giving 0, M = 255 or 65535 (at 255 svgr_layer_to_rgba8's rule).  Grey is
 * y = (0.2126 * r + 0.7152 * g) + 0.0722 * b with every product and sum rounded on its own; colour types 0 and 2 drop alpha.
 * Enqueued on the context's stream, no wait.  SVGR_E_INVALID for an unknown kind, colour type or depth, a mask with a colour
 * type other than 0, an empty or oversized image, a short or misaligned buffer, or dst == src.
 * svgr_png_filter_bytes: svgr_png_filter for rows of row_bytes bytes at bpp bytes a pixel (1, 2, 3, 4, 6 or 8): out_filtered
 * (device, rows * (1 + row_bytes) bytes) <- per row the filter type, then its bytes; byte i of a row has the neighbours
 * a = row[i - bpp], b = above[i], c = above[i - bpp], zero outside the image.  At bpp 4 the stream is svgr_png_filter's byte for
 * byte.  Enqueued on the context's stream, no wait.  SVGR_E_INVALID as svgr_png_filter, and for another bpp or a row_bytes that
 * is no multiple of it.
 * svgr_png_filter_span: the bytes of a row that one pass of a workgroup covers (the launch seam of the filter kernel).          */
#define SVGR_PNG_COLOR_GREY 0
#define SVGR_PNG_COLOR_RGB 2
#define SVGR_PNG_COLOR_GREY_ALPHA 4
#define SVGR_PNG_COLOR_RGBA 6
#define SVGR_PNG_SRC_RGBA_F64 0
#define SVGR_PNG_SRC_MASK_F64 1
#define SVGR_PNG_SRC_RGBA_U8 2
int svgr_png_samples(svgr_ctx* ctx, const svgr_buf* src, int src_kind, int64_t rows, int64_t cols, int color, int depth, svgr_buf* dst);
int svgr_png_filter_bytes(svgr_ctx* ctx, const svgr_buf* src, int64_t rows, int64_t row_bytes, int bpp, int filter, svgr_buf* out_filtered);
int svgr_png_filter_span(void);

/* Tensor output (Layer.to_tensor / Layer.to_array, beyond the reference): a layer packed into the element type and layout a
 * framework wants, written by the kernel into memory the caller names -- a svgr_buf of the library's or a wrapped pointer
 * (svgr_buf_wrap of torch's data_ptr()).  Per pixel, in double (csrc/svgr_tensor.h):
 *   source      the RGBA pixel as the caller prepared it (svgr_layer_convert for colour space and alpha state): a float64 RGBA
 *               layer, a float32 RGBA canvas (widened exactly) or a float64 1-channel mask (broadcast to all four channels)
 *   background  has_bg, premultiplied input only: c = c + bg[c] * (1 - a) for the three colours, then a = 1
 *   channels    RGBA (4), RGB (3), ALPHA (1), LUMA (1: svgr_layer_luminance's weights and order, not multiplied by alpha)
 *   affine      y = v * scale[k] + bias[k] per output channel ((v - mean) / std arrives as scale = 1 / std, bias = -mean / std)
 *   dtype       F32: y rounded to nearest-even; F16 / BF16: that float32 rounded to nearest-even again (overflow gives infinity,
 *               subnormals are kept, NaN leaves as the type's quiet NaN); U8: rint(y * 255) saturated to [0, 255], NaN gives 0
 *               (with identity affine, RGBA and straight sRGB input: the bytes of svgr_layer_to_rgba8)
 * The tensor is a rows x cols plane of `channels` elements per pixel, addressed in ELEMENTS: pixel (r, c)'s channel k is element
 * offset + k * stride_c + r * stride_h + c * stride_w.  Planar (CHW): stride_w == 1, stride_h >= cols, stride_c free.
 * Interleaved (HWC): stride_c == 1, stride_w == channels, stride_h >= cols * channels.  So the destination may be one slice of a
 * batch or a window of a larger picture, its rows beginning at any element alignment. */
#define SVGR_TENSOR_SRC_RGBA_F64 0
#define SVGR_TENSOR_SRC_RGBA_F32 1
#define SVGR_TENSOR_SRC_MASK_F64 2
#define SVGR_TENSOR_F32 0
#define SVGR_TENSOR_F16 1
#define SVGR_TENSOR_BF16 2
#define SVGR_TENSOR_U8 3
#define SVGR_TENSOR_RGBA 0
#define SVGR_TENSOR_RGB 1
#define SVGR_TENSOR_ALPHA 2
#define SVGR_TENSOR_LUMA 3
typedef struct {
    int32_t source;    /* SVGR_TENSOR_SRC_*: what the layer side holds (svgr_tensor_to_layer always writes float64) */
    int32_t dtype;     /* SVGR_TENSOR_F32 / F16 / BF16 / U8 */
    int32_t channels;  /* SVGR_TENSOR_RGBA / RGB / ALPHA / LUMA */
    int32_t has_bg;    /* 0 or 1 */
    double bg[3];
    double scale[4], bias[4];   /* per output channel; entries beyond the channel count are ignored (but must be finite) */
    int64_t rows, cols;         /* the plane */
    int64_t stride_c, stride_h, stride_w, offset;   /* in elements */
} svgr_tensor_desc;
/* svgr_layer_to_tensor: dst <- the plane packed as `desc` says; src_bbox {row0, col0, rows, cols} places the source on the plane
 * (negative offsets and partial overlap are fine: outside the box the pixel is (0, 0, 0, 0), which background and affine then
 * see like any other).  Every element of the plane is written, nothing else of dst is touched.  One launch on the context's
 * stream, no wait.  A workgroup packs svgr_tensor_block() consecutive pixels of one row, a lane svgr_tensor_run() of them; the
 * stores of a row's aligned interior are 16 bytes wide.
 * svgr_tensor_to_layer: the inverse, element -> double exactly (U8: v / 255): dst_f64 <- rows * cols pixels of 4 doubles
 * (RGBA; RGB with a = 1) or of 1 double (ALPHA, LUMA); bg, scale and bias are not applied.
 * SVGR_E_INVALID, before anything is launched: an unknown enum, has_bg not 0 / 1, a stride combination that is neither planar nor
 * interleaved, a negative stride, size or offset, a stride_h below the row's elements, a scale, bias or bg that is not finite, a
 * tensor pointer that is not a multiple of the element size, a short layer buffer, and the largest element index -- from
 * strides, sizes and offset -- reaching past svgr_buf_bytes() of the tensor.  rows * cols == 0 launches nothing and succeeds,
 * with ctx == NULL too. */
int svgr_layer_to_tensor(svgr_ctx* ctx, const svgr_tensor_desc* desc, const svgr_buf* src, const int64_t* src_bbox, svgr_buf* dst);
int svgr_tensor_to_layer(svgr_ctx* ctx, const svgr_tensor_desc* desc, const svgr_buf* src, svgr_buf* dst_f64);
int svgr_tensor_block(void);
int svgr_tensor_run(void);
/* Ordering against another stream of the same runtime (torch.cuda.current_stream().cuda_stream) without moving the context
 * onto it (svgr_set_stream drains and destroys the context's own stream).  svgr_stream_wait_for: the context's stream waits for
 * all work enqueued on `other` so far.  svgr_stream_signal_to: `other` waits for all work enqueued on the context's stream so
 * far.  Each through an event the context keeps; neither blocks the host.  other == NULL is the runtime's default stream. */
int svgr_stream_wait_for(svgr_ctx* ctx, void* other);
int svgr_stream_signal_to(svgr_ctx* ctx, void* other);

/* Indexed PNG output (Layer.write_png(palette=...), quantize; beyond the reference): the colour quantiser's device stages over
 * src_rgba8 (device, rows * cols * 4 bytes as svgr_layer_to_rgba8 writes them: a pixel is the little-endian uint32 r | g << 8 |
 * b << 16 | a << 24).  csrc/svgr_quant.h has the arithmetic: a pixel with a == 0 counts as 0 (canonical); X(p) = (r a, g a, b a,
 * 255 a) and D(p, q) = the sum of the squared differences of X, unsigned 64-bit; the bin of a pixel is (r >> 3, g >> 3, b >> 3,
 * a >> 3), r in the highest of its 20 bits.  The palette itself is built by the caller from the bins.  An image is 1 .. 2^16 a
 * side and at most 2^30 pixels (SVGR_E_INVALID beyond: the bins' 64-bit sums, at most 2^30 * 65025 < 2^46, cannot overflow in it).
 * svgr_quant_distinct: the set of distinct canonical pixels if there are at most max_colors (1 .. 256) of them: colors[0 ..
 *   *n_colors - 1], ascending as uint32, and *overflow = 0; otherwise *overflow = 1 and *n_colors = 0.  colors has room for
 *   max_colors values.  Waits for the device.
 * svgr_quant_bins: the non-empty bins in ascending key order: keys[i] and bins[5 * i .. 5 * i + 4] = {pixels, sum of X0, X1, X2, X3}
 *   over the bin's pixels, integer sums and so the same from run to run.  *n_bins always receives their number; with more than
 *   `cap` of them nothing is written and the status is SVGR_E_INVALID (min(rows * cols, 2^20) always suffices).  Waits.
 * svgr_quant_index: per pixel the index of the nearest of the palette's n_palette (1 .. 256) entries (device, uint32 pixels as
 *   above) under D, a tie going to the lowest index.  out_stream (device, or NULL) receives the scanlines of a colour type 3
 *   PNG at depth = the smallest of 1, 2, 4, 8 with 2^depth >= n_palette: per row the filter byte 0 and ceil(cols * depth / 8)
 *   bytes, indices MSB first, the padding bits zero -- ready for svgr_deflate.  out_indices (device, or NULL) receives rows * cols
 *   bytes, an index each.  At least one of the two is given.  Enqueued on the context's stream, no wait.
 * svgr_quant_block: the pixels of one workgroup of the three kernels (their launch seam); a lane takes 8 consecutive ones.
 * svgr_quant_groups: the most workgroups svgr_quant_bins launches; with more blocks than that a workgroup takes several. */
int svgr_quant_distinct(svgr_ctx* ctx, const svgr_buf* src_rgba8, int64_t rows, int64_t cols, int max_colors, uint32_t* colors,
                        int64_t* n_colors, int* overflow);
int svgr_quant_bins(svgr_ctx* ctx, const svgr_buf* src_rgba8, int64_t rows, int64_t cols, uint32_t* keys, uint64_t* bins, int64_t cap,
                    int64_t* n_bins);
int svgr_quant_index(svgr_ctx* ctx, const svgr_buf* src_rgba8, int64_t rows, int64_t cols, const svgr_buf* palette, int n_palette,
                     svgr_buf* out_stream, svgr_buf* out_indices);
int svgr_quant_block(void);
int svgr_quant_groups(void);

/* Dithering for indexed PNG output (dither= of Layer.write_png and quantize; csrc/svgr_dither.h has the arithmetic).
 * svgr_quant_dither: svgr_quant_index -- the same buffers, checks and outputs -- with every pixel matched at a moved target.
 *   mode 1, ordered: the colour coordinates of X move by off = (((2 B + 1) h) >> 7) - (h >> 1), B the 8 x 8 Bayer matrix at
 *   (row & 7, col & 7) and h = amp * a / 255; `amp` (0 .. 65025) belongs to the palette and is computed by the caller.  Enqueued, no
 *   wait.  mode 2, diffusion: Floyd-Steinberg, every row left to right, t = clamp(x + floor((acc + 8) / 16)) with acc the 7, 3, 5,
 *   1 weighted errors of the pixels to the left and above, in int32; a pixel with a == 0 takes the entry nearest to X = 0 and
 *   passes no error on; `amp` is not used.  One launch per front of tiles (block + 2 * strip), in stream order; waits for the
 *   device.  Any other mode is SVGR_E_INVALID.
 * svgr_dither_tile_rows, svgr_dither_tile_cols: a diffusion tile's rows (a strip) and columns (a block): its launch seams. */
int svgr_quant_dither(svgr_ctx* ctx, const svgr_buf* src_rgba8, int64_t rows, int64_t cols, const svgr_buf* palette, int n_palette, int mode,
                      int amp, svgr_buf* out_stream, svgr_buf* out_indices);
int svgr_dither_tile_rows(void);
int svgr_dither_tile_cols(void);

/* Differentiable coverage (svgrasterize_amd.diff, beyond the reference; csrc/svgr_cover.h has the arithmetic, DESIGN.md 7w the
 * derivation): the exact area coverage of n_paths paths over one viewport, and the derivative of sum(grad_out * cover) with
 * respect to the control points and the transforms.  Every array is a DEVICE buffer:
 *   segs          n_segs x 4 x 2 doubles, user space, as svgr_batch_desc.segs (a line uses its first two points)
 *   seg_kind      n_segs uint8, SVGR_SEG_*
 *   path_seg_off  n_paths + 1 int32: path p owns the segments [off[p], off[p + 1])
 *   path_m6       n_paths x 6 doubles;  path_rule  n_paths uint8, SVGR_FILL_*
 *   cover         n_paths x rows x cols of the plane type (double or float): plane p is Path.mask of path p placed on the viewport
 *   slope         n_paths x rows x cols int8: the derivative of the fill rule at the pixel's accumulated signed coverage
 *   grad_out      of cover's shape and type;  grad_segs  n_segs x 4 x 2 doubles;  grad_m6  n_paths x 6 doubles
 *   status        one uint32 the kernels OR into (the caller clears it): bit 0 the flatten depth cap was hit; bit 1 a transformed
 *                 control point is not finite or beyond +-1e9 pixels, or an edge's row reaches beyond them (it adds nothing)
 * svgr_cover_forward: cover and slope are written whole.  The segments add their pieces into a double accumulation plane with
 *   global atomic adds (cover itself for SVGR_COVER_F64, a block of the library's for SVGR_COVER_F32), so cover's last bits may
 *   differ from run to run; one row scan per (path, row) then resolves the plane.
 * svgr_cover_backward: grad_segs and grad_m6 are written whole, from slope and grad_out alone: no atomics, the same bits on
 *   every run.  The derivative is taken at fixed subdivision and is not defined where a pixel sits on a kink of its rule.
 * Both enqueue on the context's stream and never wait; they keep no state.  Before any launch: a count or a viewport side that
 * is not positive (n_segs may be 0), an unknown plane type, a flatness that is not positive and finite, a missing buffer or one
 * too small for the description give SVGR_E_INVALID; n_paths * rows * cols beyond 2^31 - 1 gives SVGR_E_OVERFLOW.  n_segs == 0
 * zeroes the outputs and launches nothing else.
 * svgr_cover_block: the segments of one workgroup of the segment kernels.  svgr_cover_scan: the columns one step of the row scan
 * covers.  Their launch seams. */
#define SVGR_COVER_F64 0
#define SVGR_COVER_F32 1
typedef struct {
    int64_t n_segs, n_paths;
    int64_t viewport[4];   /* {row0, col0, rows, cols} */
    double flatness;
    int32_t plane;         /* SVGR_COVER_F64 / SVGR_COVER_F32 */
    int32_t reserved;      /* 0 */
} svgr_cover_desc;
int svgr_cover_forward(svgr_ctx* ctx, const svgr_cover_desc* desc, const svgr_buf* segs, const svgr_buf* seg_kind,
                       const svgr_buf* path_seg_off, const svgr_buf* path_m6, const svgr_buf* path_rule, svgr_buf* cover, svgr_buf* slope,
                       svgr_buf* status);
int svgr_cover_backward(svgr_ctx* ctx, const svgr_cover_desc* desc, const svgr_buf* segs, const svgr_buf* seg_kind,
                        const svgr_buf* path_seg_off, const svgr_buf* path_m6, const svgr_buf* slope, const svgr_buf* grad_out,
                        svgr_buf* grad_segs, svgr_buf* grad_m6, svgr_buf* status);
int svgr_cover_block(void);
int svgr_cover_scan(void);

/* Differentiable compositing (svgrasterize_amd.diff, beyond the reference; csrc/svgr_compose.h has the arithmetic, DESIGN.md 7x
 * the derivation): n_paths solid fills painted source-over in paint order over one viewport, and the derivative of
 * sum(grad_image * image) with respect to every coverage value and every paint.  Every array is a DEVICE buffer:
 *   cover        n_paths x rows x cols of the plane type (double or float): what svgr_cover_forward writes
 *   paints       n_paths x 4 doubles: PREMULTIPLIED RGBA in the render's colour space (no conversion is done here)
 *   image        rows x cols x 4 of the plane type, premultiplied, 16-byte aligned;  grad_image  of image's shape, type and alignment
 *   grad_cover   of cover's shape and type;  grad_paints  n_paths x 4 doubles
 * svgr_compose_forward: per pixel C = bg (0 without has_bg), then for p = 0 .. n_paths - 1: s = m_p paint_p, C = s + C (1 - s_3),
 *   in double, no clamp, no fused multiply-add; a float image is rounded once at the store.
 * svgr_compose_backward: grad_cover and grad_paints are written whole.  Two walks per pixel and no division (an opaque paint on a
 *   covered pixel is no special case); grad_paints is summed without atomics, per workgroup and then in workgroup order: the same
 *   bits on every run.  bg is a constant: it has no gradient.
 * Both enqueue on the context's stream and never wait; they keep no state.  Before any launch: a count or a side that is not
 * positive, an unknown plane type, has_bg other than 0 or 1, a missing buffer, one too small for the description or an image that
 * is not 16-byte aligned give SVGR_E_INVALID; n_paths * rows * cols beyond 2^31 - 1 gives SVGR_E_OVERFLOW.
 * svgr_compose_block: the pixels of one workgroup step.  svgr_compose_groups: the most workgroups the backward launches (they
 * stride over the pixels).  Their launch seams. */
typedef struct {
    int64_t n_paths, rows, cols;
    double bg[4];          /* premultiplied; read only with has_bg */
    int32_t plane;         /* SVGR_COVER_F64 / SVGR_COVER_F32 */
    int32_t has_bg;        /* 0 / 1 */
} svgr_compose_desc;
int svgr_compose_forward(svgr_ctx* ctx, const svgr_compose_desc* desc, const svgr_buf* cover, const svgr_buf* paints, svgr_buf* image);
int svgr_compose_backward(svgr_ctx* ctx, const svgr_compose_desc* desc, const svgr_buf* cover, const svgr_buf* paints,
                          const svgr_buf* grad_image, svgr_buf* grad_cover, svgr_buf* grad_paints);
int svgr_compose_block(void);
int svgr_compose_groups(void);

/* Gradient paints in differentiable compositing (csrc/svgr_gradpaint.h has the arithmetic, DESIGN.md 7y the derivation): as above,
 * but path p is a solid fill (kind 0) or the renderer's linear (1) or one-circle radial (2) gradient, evaluated at the centre of
 * every pixel and multiplied by the coverage and by paints[p].  The description also holds HOST pointers to the topology, which is
 * validated and copied before the entry returns (the caller may free it then):
 *   kind[n_paths]            0 solid, 1 linear, 2 radial        spread[n_paths]   0 pad, 1 repeat, 2 reflect (ignored for a solid)
 *   path_stop_off[n_paths+1] path p owns the stops path_stop_off[p] : path_stop_off[p + 1]; from 0 to n_stops, never decreasing;
 *                            a solid path owns none, a gradient path 1 to 32
 * DEVICE buffers, all doubles but the planes and images (which are svgr_compose_forward's):
 *   paints      n_paths x 4   a solid path's premultiplied colour; a gradient path's component-wise multiplier (ones, or an opacity)
 *   paint_m6    n_paths x 6   pixel centre (row + row0 + 0.5, col + col0 + 0.5) -> gradient space: the inverse render transform
 *                             followed by the inverse gradientTransform, composed by the caller (unused for a solid)
 *   paint_geom  n_paths x 4   linear: p0x, p0y, p1x, p1y; radial: cx, cy, r and an unused slot
 *   stop_pos    n_stops       non-decreasing per path;   stop_rgba  n_stops x 4  premultiplied, in the render's colour space
 * svgr_compose_painted_forward: s = (colour m_p) paint_p per channel, C = s + C (1 - s_3); a solid path as svgr_compose_forward.
 * svgr_compose_painted_backward: grad_cover (cover's shape and type), grad_paints, grad_m6, grad_geom, grad_stop_pos and
 *   grad_stop_rgba (their inputs' shapes) are written whole; the rows of solid paths in grad_m6 and grad_geom and the unused radial
 *   slot are 0.  Where a derivative is not defined (an offset on a stop, a clamp, a wrap or a fold; the radial centre) one
 *   documented side is taken and nothing is NaN for finite input.  No atomics: the same bits on every run.  Degenerate geometry
 *   (p0 == p1, r <= 0) is not looked at here: it gives NaN or infinities.
 * Both enqueue on the context's stream and never wait; they keep no state.  Before any launch: everything svgr_compose_forward
 * refuses, an unknown kind or spread, a stop table that does not go from 0 to n_stops or decreases, a gradient path without a
 * stop or with more than 32, a solid path with stops and a missing or too small buffer give SVGR_E_INVALID;
 * n_paths * rows * cols beyond 2^31 - 1 gives SVGR_E_OVERFLOW.  With n_stops == 0 the four stop buffers may be NULL. */
typedef struct {
    int64_t n_paths, rows, cols;
    double bg[4];          /* premultiplied; read only with has_bg */
    int32_t plane;         /* SVGR_COVER_F64 / SVGR_COVER_F32 */
    int32_t has_bg;        /* 0 / 1 */
    int64_t row0, col0;    /* the viewport's origin */
    int64_t n_stops;
    const int32_t* kind;
    const int32_t* spread;
    const int32_t* path_stop_off;
} svgr_painted_desc;
int svgr_compose_painted_forward(svgr_ctx* ctx, const svgr_painted_desc* desc, const svgr_buf* cover, const svgr_buf* paints, const svgr_buf* paint_m6,
                                 const svgr_buf* paint_geom, const svgr_buf* stop_pos, const svgr_buf* stop_rgba, svgr_buf* image);
int svgr_compose_painted_backward(svgr_ctx* ctx, const svgr_painted_desc* desc, const svgr_buf* cover, const svgr_buf* paints, const svgr_buf* paint_m6,
                                  const svgr_buf* paint_geom, const svgr_buf* stop_pos, const svgr_buf* stop_rgba, const svgr_buf* grad_image,
                                  svgr_buf* grad_cover, svgr_buf* grad_paints, svgr_buf* grad_m6, svgr_buf* grad_geom, svgr_buf* grad_stop_pos,
                                  svgr_buf* grad_stop_rgba);

/* Isolated groups in differentiable compositing (csrc/svgr_group.h has the arithmetic, DESIGN.md 7z the derivation): the painted
 * composition above, driven by a PROGRAM of n_items items in paint order instead of the flat list of planes.  The description is
 * svgr_painted_desc followed by the program, HOST tables that are validated and copied before the entry returns:
 *   items[n_items x 4]   {0, p, 0, 0}                        FILL: plane p painted on the open canvas, exactly as path p above
 *                        {1, index of its END, 0, 0}         BEGIN: a transparent canvas is opened
 *                        {2, index of its BEGIN, opacity slot or -1, clip or -1}
 *                                                            END: the canvas is closed, multiplied by opacity[slot] (Layer.opacity), then
 *                                                            by the clip's mask (COMPOSE_IN), and painted OVER the canvas below
 *   clip_off, clip_planes   clip c is the planes clip_planes[clip_off[c] : clip_off[c + 1]], at least one, composed OVER in one
 *                           channel in that order (the first copied); there are as many clips as END items name, numbered from 0;
 *                           clip_off goes from 0 to n_clip_planes.  Both may be NULL with n_clip_planes == 0.
 * Every plane is used exactly once, by one FILL or as one clip plane (its rows of paints and of the paint arrays are ignored, its
 * rows of their gradients are 0); every opacity slot and every clip by exactly one END; BEGIN and END match and nest at most
 * svgr_group_depth() (4) deep.  n_items is the number of FILLs plus 2 n_groups, at most 2^24.
 * DEVICE buffers: svgr_compose_painted_forward's, and opacity, n_opacities doubles (may be NULL with none).
 * svgr_compose_grouped_backward writes grad_cover whole, clip planes included, the five arrays of svgr_compose_painted_backward
 * and grad_opacity (n_opacities doubles).  Nothing is divided: an opacity or a mask of 0 and an empty group are ordinary values.
 * No atomics: the same bits on every run.  A program without groups gives svgr_compose_painted_forward / _backward's bits.
 * Both enqueue on the context's stream and never wait; they keep no state.  Before any launch: everything
 * svgr_compose_painted_forward refuses, any violation of the program's rules above and a missing or too small buffer give
 * SVGR_E_INVALID; more than 2^24 items, or n_groups * rows * cols beyond 2^31 - 1, give SVGR_E_OVERFLOW. */
typedef struct {
    int64_t n_paths, rows, cols;
    double bg[4];          /* premultiplied; read only with has_bg */
    int32_t plane;         /* SVGR_COVER_F64 / SVGR_COVER_F32 */
    int32_t has_bg;        /* 0 / 1 */
    int64_t row0, col0;    /* the viewport's origin */
    int64_t n_stops;
    const int32_t* kind;
    const int32_t* spread;
    const int32_t* path_stop_off;
    int64_t n_items, n_groups, n_clip_planes, n_opacities;
    const int32_t* items;
    const int32_t* clip_off;
    const int32_t* clip_planes;
} svgr_grouped_desc;
int svgr_compose_grouped_forward(svgr_ctx* ctx, const svgr_grouped_desc* desc, const svgr_buf* cover, const svgr_buf* paints, const svgr_buf* paint_m6,
                                 const svgr_buf* paint_geom, const svgr_buf* stop_pos, const svgr_buf* stop_rgba, const svgr_buf* opacity, svgr_buf* image);
int svgr_compose_grouped_backward(svgr_ctx* ctx, const svgr_grouped_desc* desc, const svgr_buf* cover, const svgr_buf* paints, const svgr_buf* paint_m6,
                                  const svgr_buf* paint_geom, const svgr_buf* stop_pos, const svgr_buf* stop_rgba, const svgr_buf* opacity,
                                  const svgr_buf* grad_image, svgr_buf* grad_cover, svgr_buf* grad_paints, svgr_buf* grad_m6, svgr_buf* grad_geom,
                                  svgr_buf* grad_stop_pos, svgr_buf* grad_stop_rgba, svgr_buf* grad_opacity);
int svgr_group_depth(void);

/* Luminance-masked groups in differentiable compositing (csrc/svgr_mask.h has the arithmetic, DESIGN.md 7za the derivation): the
 * grouped composition above with the same description and buffers, and a program that may hold two more ops:
 *   {1, index of its closer, 0, 0}                       BEGIN: its closer is an END, a HOLD or an END_MASK
 *   {3, index of its BEGIN, opacity slot or -1, clip or -1}
 *                                                        HOLD: closes the TARGET group like END, but keeps it instead of painting it
 *   {4, index of its BEGIN, 0, 0}                        END_MASK: closes the MASK group; its premultiplied canvas becomes one scalar
 *                                                        per pixel, luminance of the straight colour (divided where alpha > 1e-4, all
 *                                                        four clipped to [0, 1]) times alpha, as Layer.luminance_mask; the held group
 *                                                        is multiplied by it (COMPOSE_IN) and painted OVER the canvas below
 * A HOLD at item i is followed at i + 1 by the BEGIN of a group closed by END_MASK, and nothing else pairs them; a HOLD is never the
 * last item.  Target and mask group sit on the same level, may hold anything (pairs too) and both count as groups: in n_groups,
 * in n_items and towards svgr_group_depth().  A mask has no parameter: the gradients' layout is the grouped one.  The derivative
 * takes one side at every kink (csrc/svgr_mask.h) and is finite for every finite input.  A program without pairs gives
 * svgr_compose_grouped_forward / _backward's bits.  Errors are those of the grouped entries, with the pairing rules among the
 * program's. */
int svgr_compose_masked_forward(svgr_ctx* ctx, const svgr_grouped_desc* desc, const svgr_buf* cover, const svgr_buf* paints, const svgr_buf* paint_m6,
                                const svgr_buf* paint_geom, const svgr_buf* stop_pos, const svgr_buf* stop_rgba, const svgr_buf* opacity, svgr_buf* image);
int svgr_compose_masked_backward(svgr_ctx* ctx, const svgr_grouped_desc* desc, const svgr_buf* cover, const svgr_buf* paints, const svgr_buf* paint_m6,
                                 const svgr_buf* paint_geom, const svgr_buf* stop_pos, const svgr_buf* stop_rgba, const svgr_buf* opacity,
                                 const svgr_buf* grad_image, svgr_buf* grad_cover, svgr_buf* grad_paints, svgr_buf* grad_m6, svgr_buf* grad_geom,
                                 svgr_buf* grad_stop_pos, svgr_buf* grad_stop_rgba, svgr_buf* grad_opacity);

#ifdef __cplusplus
}
#endif
#endif /* SVGR_H */
