// svgr_hip.hip -- MI355X (gfx950 / CDNA4) anti-aliased path rasterizer: HIP kernels + C ABI.
// (What the host remembers between renders -- a plan stands, its slab order, which results a replay finds in place -- is svgr_batch::plan: svgr_plan_state.h.)
// Pipeline of one svgr_batch_render (4 launches of a planned batch on the context stream -- k_band_entries only in a plan's own
// pass, k_path_bbox only in the first replay after a plan: the later ones keep the slab table it wrote --, no host read-back).  A frame with NEW geometry (svgr_batch_draw) runs the same kernels in their unplanned forms -- the
// flatten in one traversal with a decoupled look-back (k_flatten<.., SCAN>), k_path_build<2> on its own per-cell bounds -- with the
// tile kernel enqueued behind the pass and ONE host wait at the end:
//
//   [memsets]       zero-fill of the batch's counter arena and of the tiles' entry bitmasks: only for the first render
//                   after a plan, later ones find both cleared by the previous render's kernels
//   [k_path_rows]   multi-GPU plans only: rows each path's control-point hull can reach (a rank lists its share)
//   k_flatten       32 lanes per segment: transform (fma form), stack-free adaptive subdivision; the edges go to the
//                   plan's per-segment prefix sums -- (path, segment, curve) order, no returning atomic; endpoints
//                   folded into per-path min/max keys
//   k_path_bbox     per path: integer bbox (floor-1 / ceil+1, clipped to the viewport), band range, its (path, band)
//                   pair slots and (path, band, column tile) cells, and its SLABS -- runs of <= 16 bands, <= 80 cells -- at the plan's heaviest-first places
//                   (a replay that finds this table in place does not launch it: k_path_build<1> checks the keys against it)
//   k_band_entries  per band: the paths whose bbox reaches it, in paint order; the band's first item slot
//   k_path_build    per slab, everything in LDS: per edge row the closed-form signed-area pieces (the reference's x
//                   recurrence replayed from the edge's first row), per cell the carry-in of every tile row, its
//                   class (nothing visible / constant per row / has pieces), header, entry-bitmask bits and -- for
//                   the cells with pieces -- its ADD LIST: every piece, carry-in and layer-edge sentinel resolved to
//                   {offset in the tile's delta tile, value}, so that the tile kernel's scatter is one load + one LDS add
//                   (a kept replay's lean form writes only what a replay can change: pieces, carry-in adds and the class-1
//                   cells; the class-2 cells' headers, sentinels and mask bits stand from the last full placed pass --
//                   PlanState::cells (svgr_plan_state.h) says when they do; svgr_batch_set_paints asks for one full pass)
//   k_tile_lists    per band: bitmasks -> per-tile item lists (cell ids in paint order, each with its add list), the
//                   tiles in heaviest-first order, one PAGE per tile (which tile + its first 24 items: one load);
//                   clears the bitmasks for the next render; in a placed replay a band whose bitmasks repeat keeps its lists
//   k_tile_render   one 128-thread workgroup per 16x64 canvas tile, canvas tile resident in registers as
//                   double RGBA; per item in paint order: header and add list prefetched into registers items ahead;
//                   the adds of item k+1 go into one LDS delta tile (ds_add_f64) while item k's is scanned
//                   (8 px per lane serial + DPP row scan across the 8 lanes of a row), fill rule, paint, source-over
//                   (isolated groups in a second register tile); one barrier per item; the finished tile leaves
//                   through an LDS transpose as whole 1-KiB rows (float32, nontemporal) or as double
//
// There is no dense contraction anywhere in this path: no MFMA.  The heavy traffic (delta tile,
// canvas tile) never leaves the CU; HBM sees the edges, the cell headers, the add lists and one canvas store.
//
// gfx950 only.  Compile with -ffp-contract=off (see svgr_core.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdarg>
#include <cstddef>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <ctime>
#include <initializer_list>
#include <new>
#include <string>
#include <type_traits>
#include <vector>
#include <memory>
#include <unordered_map>
#include <utility>

#include "../../include/svgr.h"
#include "svgr_core.h"
#include "svgr_blob.h"
#include "svgr_box.h"

using namespace svgr;

// every kernel launch of the library goes through this: a per-process count of them (svgr_measure_launches: what bench.py's
// `launches` per render is) -- the stream itself has no such counter
static std::atomic<unsigned long long> g_n_launches{0};
#define SVGR_LAUNCH(...) do { g_n_launches.fetch_add(1, std::memory_order_relaxed); hipLaunchKernelGGL(__VA_ARGS__); } while (0)

// ======================================================================================
// tile geometry
// ======================================================================================
constexpr int TR = 16;                     // rows per band / tile
constexpr int PX = 8;                      // pixels per lane (consecutive columns)
constexpr int CH = 8;                      // lanes per tile row: half a 16-lane DPP row
constexpr int TC = CH * PX;                // columns per tile
constexpr int NT = TR * CH;                // threads per workgroup (128 = 2 waves); a wave covers 64 / CH tile rows
constexpr int CHUNK_STRIDE = PX + 2;       // doubles; +16 B makes the b128 lane groups conflict free
constexpr int ROW_STRIDE = CH * CHUNK_STRIDE;
constexpr int DELTA_BYTES = TR * ROW_STRIDE * 8;   // one delta tile in LDS
static_assert(DELTA_BYTES < (1 << 16), "a TileAdd carries its byte offset in 16 bits");
static_assert(TC <= 64, "a TileAdd carries its run length in 6 bits");
constexpr int NW = NT / 64;                // waves per workgroup
constexpr int WAVES_PER_EU = 4;            // register budget of the tile kernel: 512 / 4 = 128 VGPRs
static_assert(NT % 64 == 0 && NT <= 1024, "tile kernel: whole waves, at most 1024 threads");

// One addition into a tile's LDS delta tile: everything the scatter phase of the tile kernel does for it is
// `ds_add_f64 base + offset, v`.  A run of `len` consecutive tile columns with the same value (the middle pieces of a
// long span, S:2286-2287) is one entry.  Written by k_pair_cells, per cell contiguous.
struct TileAdd {
    unsigned where;
    unsigned zero;
    double v;
};
static_assert(sizeof(TileAdd) == 16, "TileAdd is one dwordx4");
__device__ __forceinline__ void store_add(TileAdd* p, unsigned where, double v) {
    TileAdd t;
    t.where = where; t.zero = 0u; t.v = v;
    *p = t;
}
// One (path, band, column tile) CELL = one work item of the tile kernel, written by k_pair_cells.
// `carry[r]` = sum of every piece of the pair's row r that lies LEFT of the tile (the running sum the row
// scan starts from, np.cumsum S:983); `cls` sorts the cells:
//   0  no record reaches the tile and every carry-in is below the 1e-6 cut (S:990): nothing to draw, the tile
//      never sees the cell
//   1  no record reaches the tile but some row's carry-in is visible: coverage is constant along each row
//      (rule(carry)), composite without scatter / scan
//   2  records reach the tile: its add list (carry-ins included) is scattered, then scan + composite
// The first 80 bytes travel to the tile kernel as ONE load instruction (a dword per lane).
struct CellHdr {
    double paint[4];
    int r0, c0, rows, cols;   // the path's layer (clipped bbox)
    int bits;                 // bit 0: fill rule (0 nonzero, 1 evenodd); bits 1-2: SVGR_PATH_* flags >> 1; bits 3-4: class;
                              // bits 5-: gradient index + 1 (0: solid colour)
    int n_add, add0;          // class 2: its add list
    int p;                    // path id
    int group, pad[3];        // isolated group the path belongs to (-1: none)
    double carry[TR];        // class 1 reads them; for class 2 they are in the add list
};
constexpr int HDR_DWORDS = 20;    // everything in front of `carry`
constexpr int HDR_LOAD_DWORDS = HDR_DWORDS + 2 * TR;   // what the tile kernel loads per item: all of it, a dword per lane
static_assert(HDR_LOAD_DWORDS <= 64, "a CellHdr is one dword per lane of one load instruction");
static_assert(sizeof(CellHdr) == 4 * HDR_DWORDS + 8 * TR && offsetof(CellHdr, carry) == 4 * HDR_DWORDS, "CellHdr layout");
constexpr unsigned SPAN_MAX = (1u << 26) - 1;
static_assert(TR <= 64, "row-in-band is stored in 6 bits");

// ======================================================================================
// errors
// ======================================================================================
static thread_local std::string g_err;
static int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}
#define HIPCHK(expr)                                                                              \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess) return fail(SVGR_E_HIP, "%s: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

struct svgr_ctx {
    int device = 0;
    int id = 0;  // > 0, unique in the process: the block cache keeps every context's blocks apart
    hipStream_t stream = nullptr;
    bool own_stream = false;
    char name[128] = {0};
    void* pinned = nullptr;      // page-locked staging for read-backs that must not block the host (svgr_batch_plan_many)
    size_t pinned_bytes = 0;
    // page-locked staging for a batch's input blob (svgr_batch_create, svgr_batch_set_transforms): packed straight into it and copied
    // from it asynchronously -- a fresh pageable vector costs its page faults, its zero fill and the runtime's own staging copy
    // (half of a cold frame's host time).  One upload at a time: `up_ev` marks the last copy enqueued from it.
    void* up_stage = nullptr;
    size_t up_stage_bytes = 0;
    hipEvent_t up_ev = nullptr;
    bool up_busy = false;
    hipEvent_t meas_ev[2] = {nullptr, nullptr};   // svgr_measure_begin / _end
    hipEvent_t pin_ev = nullptr;                  // marks a read-back into `pinned` that the host waits for alone
    struct WorkSpare* spare = nullptr;            // the work arrays of the last large batch destroyed on this context (below)
    int n_cu = 256;              // compute units: the tile kernel's persistent launch is sized by it
    void* trash = nullptr;       // 1 KiB of device memory nobody reads (TileArgs::trash)
    unsigned* tile_ctr = nullptr;  // two sets of eight tile counters (TileArgs::tile_ctr), used alternately by the launches of this stream
    int tile_ctr_set = 0;
    // svgr_batch_render_windows: the windows of one picture are drawn side by side -- each is a launch of a few dozen workgroups
    // whose duration is its heaviest tile's -- on streams of their own, between two events of the context's stream
    static constexpr int N_SIDE = 8;
    hipStream_t side[N_SIDE] = {};
    hipEvent_t side_ev[N_SIDE] = {};
    hipEvent_t fork_ev = nullptr;
    bool side_ready = false;
    hipEvent_t xs_ev[2] = {nullptr, nullptr};    // svgr_stream_wait_for / svgr_stream_signal_to: the mark each records on the stream waited for
};
// the context whose call is running on this thread (set by enter_ctx at the top of every entry point): the block cache
// files what is allocated and released under it
static thread_local int tl_ctx_id = 0;
static hipError_t enter_ctx(const svgr_ctx* c) {
    tl_ctx_id = c->id;
    return hipSetDevice(c->device);
}
struct svgr_buf {
    void* ptr = nullptr;
    size_t bytes = 0;
    bool owned = false;
};

// ======================================================================================
// device memory: a small size-class cache in front of hipMalloc / hipFree.  The per-node route
// creates thousands of short-lived buffers (one batch per path, one image per layer); hipMalloc /
// hipFree cost ~100 us each and hipFree synchronises the device.  A block that is returned can be
// handed out again at once ONLY to the context it came from: every kernel and copy of a context
// runs on that context's stream and its calls are serialised by the caller, so stream order keeps
// the block's users apart.  Two contexts on one device have two streams: their blocks never mix
// (svgr_set_stream drains the outgoing stream before the context moves to another one).
// ======================================================================================
#include <map>
#include <mutex>
#include <set>
namespace {
struct DevPool {
    struct Block { size_t cap; int dev; int ctx; };
    std::mutex mu;
    std::map<int, std::multimap<size_t, void*>> free_by_ctx;  // per context, by capacity
    std::map<void*, Block> cap_of;                             // every block handed out or cached
    std::set<int> live;                                        // contexts that exist
    size_t cached_bytes = 0;
    static constexpr size_t kMaxCached = 64ull << 30;   // (of 288 GB: a 4096-wide document holds dozens of 138 MB layers at a time, and a block given back to the driver costs a hipFree -- which waits for the device -- and a hipMalloc the next time)

    static size_t size_class(size_t n) {
        size_t c = 256;
        while (c < n) c += c < (1u << 20) ? c : c / 4;  // x2 up to 1 MiB, then +25 %
        return c;
    }
    void open(int ctx) { std::lock_guard<std::mutex> lk(mu); live.insert(ctx); }
    // `dev` = the device the block is for (the caller has made it current); -1: whatever is current.  The block belongs to
    // the context running on this thread (enter_ctx).
    hipError_t alloc(void** out, size_t bytes, int dev = -1) {
        const size_t c = size_class(bytes ? bytes : 1);
        const int ctx = tl_ctx_id;
        if (dev < 0) (void)hipGetDevice(&dev);
        {
            std::lock_guard<std::mutex> lk(mu);
            auto& free_blocks = free_by_ctx[ctx];
            auto it = free_blocks.lower_bound(c);
            if (it != free_blocks.end() && it->first <= c + c / 2 && cap_of[it->second].dev == dev) {
                *out = it->second;
                cached_bytes -= it->first;
                free_blocks.erase(it);
                return hipSuccess;
            }
        }
        hipError_t e = hipMalloc(out, c);
        if (e != hipSuccess) {  // give this device's cache back to the driver and retry once
            trim(dev);
            e = hipMalloc(out, c);
        }
        if (e == hipSuccess) {
            std::lock_guard<std::mutex> lk(mu);
            cap_of[*out] = Block{c, dev, ctx};
        }
        return e;
    }
    void release(void* p) {
        if (!p) return;
        std::unique_lock<std::mutex> lk(mu);
        auto it = cap_of.find(p);
        if (it == cap_of.end()) { lk.unlock(); (void)hipFree(p); return; }
        // (a block whose context is gone has nobody to go back to; hipFree waits for the device, so late users are safe)
        if (cached_bytes + it->second.cap > kMaxCached || !live.count(it->second.ctx)) {
            cap_of.erase(it);
            lk.unlock();
            (void)hipFree(p);
            return;
        }
        free_by_ctx[it->second.ctx].emplace(it->second.cap, p);
        cached_bytes += it->second.cap;
    }
    // give cached blocks back to the driver: those of device `dev` (every context's: hipFree waits for the device), or --
    // close() -- those of one context that is going away
    void trim(int dev) { drop([&](const Block& b) { return b.dev == dev; }); }
    void close(int ctx) {
        { std::lock_guard<std::mutex> lk(mu); live.erase(ctx); }
        drop([&](const Block& b) { return b.ctx == ctx; });
    }
    template <class Pred>
    void drop(Pred pred) {
        std::vector<void*> blocks;
        {
            std::lock_guard<std::mutex> lk(mu);
            for (auto& per_ctx : free_by_ctx)
                for (auto it = per_ctx.second.begin(); it != per_ctx.second.end();) {
                    auto info = cap_of.find(it->second);
                    if (info != cap_of.end() && pred(info->second)) {
                        blocks.push_back(it->second);
                        cached_bytes -= it->first;
                        cap_of.erase(info);
                        it = per_ctx.second.erase(it);
                    } else {
                        ++it;
                    }
                }
        }
        for (void* b : blocks) (void)hipFree(b);
    }
};
DevPool g_pool;
}  // namespace

// One scratch block of the pool for the length of a call: the destructor gives it back.  By the pool's stream-order rule
// (above) a block may go back as soon as the last copy or kernel that uses it is enqueued -- its next user is queued behind
// them on the same stream -- so going back at scope end, whatever waits came before, is safe.
struct PoolBlock {
    void* p = nullptr;
    PoolBlock() = default;
    PoolBlock(const PoolBlock&) = delete;
    PoolBlock& operator=(const PoolBlock&) = delete;
    ~PoolBlock() { g_pool.release(p); }
    hipError_t alloc(size_t bytes, int dev = -1) {
        hipError_t e = g_pool.alloc(&p, bytes, dev);
        if (e != hipSuccess) p = nullptr;
        return e;
    }
    template <class T>
    T* as() const { return (T*)p; }
};

struct StreamDrain {   // no block and no host buffer of a call goes away while the stream may still use it
    hipStream_t st;
    ~StreamDrain() { (void)hipStreamSynchronize(st); }
};

// The call frame of a pass entry (svgr_path_dash ... svgr_deflate): arrays of the caller go up in one piece (svgr_blob.h), the
// context's stream works on them, one result block whose last section is the kernels' error flag comes down.  The frame owns all
// the stream may touch -- host blob, device blocks, scratch, the result's host copy -- and `drain` is its LAST member: on every
// way out the stream is waited for before any of them is released.  So scratch comes from scratch(), never from a PoolBlock of
// the entry's own, and a host buffer the stream writes is declared in front of the frame.
struct PassFrame {
    svgr_ctx* ctx;
    hipStream_t st;
    HostBlob blob;              // what upload() sends
    PoolBlock in, out;
    PoolBlock extra[13];        // scratch(): device-only blocks of the call
    int n_extra = 0, err = 0;   // err: the first failure of scratch(), which the entry returns before it launches anything
    std::vector<char> back;     // finish(): the host copy of out's first `out_bytes`
    size_t out_bytes = 0;
    Section<int> bad;           // the error flag, behind the entry's own sections of `out`
    StreamDrain drain;
    explicit PassFrame(svgr_ctx* c) : ctx(c), st(c->stream), drain{c->stream} {}

    // enters the context, enqueues the one upload
    int upload() {
        HIPCHK(enter_ctx(ctx));
        HIPCHK(in.alloc(blob.bytes(), ctx->device));
        HIPCHK(hipMemcpyAsync(in.p, blob.data(), blob.bytes(), hipMemcpyHostToDevice, st));
        return 0;
    }
    // the result block: the sections the entry took from `lay`, the error flag (cleared here), and `device_only` bytes that are
    // never downloaded (behind())
    int result(Layout lay, size_t device_only = 0) {
        bad = lay.take<int>(1);
        out_bytes = lay.bytes();
        HIPCHK(out.alloc(out_bytes + device_only, ctx->device));
        HIPCHK(hipMemsetAsync(bad.on(out.p), 0, sizeof(int), st));
        return 0;
    }
    int begin(Layout lay, size_t device_only = 0) {
        if (int rc = upload()) return rc;
        return result(lay, device_only);
    }
    template <class T>
    T* behind() const { return (T*)(out.as<char>() + out_bytes); }
    template <class T>
    T* scratch(size_t n) {
        if (err) return nullptr;
        if (n_extra == (int)(sizeof extra / sizeof extra[0])) err = fail(SVGR_E_STATE, "PassFrame: out of scratch blocks");
        else if (hipError_t e = extra[n_extra].alloc(n * sizeof(T), ctx->device))
            err = fail(SVGR_E_HIP, "a scratch block of %zu bytes: %s", n * sizeof(T), hipGetErrorString(e));
        return err ? nullptr : extra[n_extra++].as<T>();
    }
    // the one download and the one wait; `what`: `message` if a kernel raised the flag
    int finish(const char* what, const char* message) {
        HIPCHK(hipGetLastError());
        back.resize(out_bytes);
        HIPCHK(hipMemcpyAsync(back.data(), out.p, out_bytes, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (*bad.on(back.data())) return fail(SVGR_E_STATE, "%s: %s", what, message);
        return 0;
    }
};

// a device array that owns its block (unless it is a view); release() frees it early
template <class T>
struct DevArr {
    T* p = nullptr;
    size_t cap = 0;  // elements
    bool view = false;  // p points into somebody else's block (the batch's input blob): never released here
    DevArr() = default;
    DevArr(const DevArr&) = delete;
    DevArr& operator=(const DevArr&) = delete;
    DevArr(DevArr&& o) noexcept : p(o.p), cap(o.cap), view(o.view) { o.p = nullptr; o.cap = 0; o.view = false; }
    DevArr& operator=(DevArr&& o) noexcept {
        if (this != &o) {
            release();
            p = o.p; cap = o.cap; view = o.view;
            o.p = nullptr; o.cap = 0; o.view = false;
        }
        return *this;
    }
    ~DevArr() { release(); }
    void point_at(void* base, size_t byte_off, size_t n) {
        release();
        p = (T*)((char*)base + byte_off);
        cap = n;
        view = true;
    }
    int ensure(size_t n) {
        if (n <= cap) return 0;
        if (p && !view) g_pool.release(p);
        view = false;
        p = nullptr;
        cap = 0;
        size_t want = n + n / 8 + 16;
        hipError_t e = g_pool.alloc((void**)&p, want * sizeof(T));
        if (e != hipSuccess) return fail(SVGR_E_NOMEM, "hipMalloc(%zu bytes): %s", want * sizeof(T), hipGetErrorString(e));
        cap = want;
        return 0;
    }
    void release() {
        if (p && !view) g_pool.release(p);
        p = nullptr;
        cap = 0;
        view = false;
    }
};

// Several arrays out of one device block: first pass (base == nullptr) adds up the sizes, second pass points the arrays at
// their places.  Every array gets the eighth of slack an allocation of its own would have (DevArr::ensure).
struct Carver {
    unsigned char* base = nullptr;
    size_t at = 0;
    template <class T>
    void take(DevArr<T>& a, size_t n) {
        n = n + n / 8 + 16;
        if (base) a.point_at(base, at, n);
        at += (n * sizeof(T) + 255) & ~(size_t)255;
    }
};

// ======================================================================================
// wave-level helpers (wave = 64 lanes)
// ======================================================================================
// Exclusive prefix sum over the 64 lanes (every lane must call it), `total` = the wave's sum.  DPP adds: four
// row_shr steps inside each 16-lane row, then row_bcast:15 / row_bcast:31 carry the row totals upward -- no
// per-lane index registers (the ds_bpermute form of __shfl_up keeps six of them alive across whatever follows).
__device__ __forceinline__ int wave_excl_scan(int v, int lane, int& total) {
    (void)lane;
    int x = v;
    x += __builtin_amdgcn_update_dpp(0, x, 0x111, 0xf, 0xf, true);  // row_shr:1
    x += __builtin_amdgcn_update_dpp(0, x, 0x112, 0xf, 0xf, true);  // row_shr:2
    x += __builtin_amdgcn_update_dpp(0, x, 0x114, 0xf, 0xf, true);  // row_shr:4
    x += __builtin_amdgcn_update_dpp(0, x, 0x118, 0xf, 0xf, true);  // row_shr:8
    x += __builtin_amdgcn_update_dpp(0, x, 0x142, 0xa, 0xf, true);  // row_bcast:15 into rows 1 and 3
    x += __builtin_amdgcn_update_dpp(0, x, 0x143, 0xc, 0xf, true);  // row_bcast:31 into rows 2 and 3
    total = __builtin_amdgcn_readlane(x, 63);
    return x - v;
}

// number of set bits of `m` below the calling lane (v_mbcnt: no 64-bit lane mask to keep in registers)
__device__ __forceinline__ int mask_rank(unsigned long long m) {
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

// every lane of the wave must call this; reserves `n` consecutive slots for the calling lane with a
// single atomic per wave and returns the lane's first slot
__device__ __forceinline__ int wave_alloc(int* cursor, int n, int lane) {
    int total;
    int excl = wave_excl_scan(n, lane, total);
    int base = 0;
    if (lane == 0 && total > 0) base = atomicAdd(cursor, total);
    return __shfl(base, 0) + excl;
}

// Runs of consecutive active lanes with equal keys.  For an active lane: `head` = first lane of its
// run, `len` = length of the run.  Every lane of the wave must call this.
__device__ __forceinline__ void wave_runs(int key, bool active, int lane, int& head, int& len) {
    int prev = __shfl_up(key, 1);
    int prev_act = __shfl_up((int)active, 1);
    bool is_head = active && (lane == 0 || !prev_act || prev != key);
    unsigned long long H = __ballot(is_head), A = __ballot(active);
    unsigned long long B = H | ~A;  // a run cannot continue across these lanes
    unsigned long long below = H & (lane == 63 ? ~0ull : ((2ull << lane) - 1ull));
    head = below ? 63 - __clzll(below) : lane;
    unsigned long long above = (B >> head) >> 1;
    len = above ? __ffsll((long long)above) : 64 - head;
}

// ======================================================================================
// band ownership (multi-GPU): rank r of `world` owns the strips s with s % world == r, a strip being
// `strip` consecutive bands.  world == 1 owns everything.
// ======================================================================================
struct Owner {
    int rank, world, strip;
};
__host__ __device__ __forceinline__ bool owns_band(const Owner o, int band) {
    return o.world <= 1 || (band / o.strip) % o.world == o.rank;
}
// k-th owned band (k = 0, 1, ...) in increasing order
__host__ __device__ __forceinline__ int owned_band_at(const Owner o, int k) {
    if (o.world <= 1) return k;
    return ((k / o.strip) * o.world + o.rank) * o.strip + (k % o.strip);
}
// does [ba, bb] contain an owned band?
__host__ __device__ __forceinline__ bool owns_any(const Owner o, int ba, int bb) {
    if (o.world <= 1) return true;
    const int sa = ba / o.strip, sb = bb / o.strip;
    if (sb - sa + 1 >= o.world) return true;
    for (int s = sa; s <= sb; ++s)
        if (s % o.world == o.rank) return true;
    return false;
}
static int count_owned_bands(const Owner o, int n_bands) {
    int n = 0;
    for (int b = 0; b < n_bands; ++b) n += owns_band(o, b) ? 1 : 0;
    return n;
}

// ======================================================================================
// geometry kernels
// ======================================================================================
// Device-side scalars of a batch; lives at the start of the zeroed arena, so every field's
// "nothing yet" value is 0 (minima are stored as biased maxima).
constexpr int UNION_BIAS = 1 << 30;
struct BatchDev {
    int err;            // bit 0: flatten depth cap, bit 1: edge capacity, bit 2: (path,band) capacity,
                        // bit 3: band-seg capacity, bit 4: bbox beyond int range, bit 5: cell capacity,
                        // bit 6: add / item capacity
    int n_nonempty;
    unsigned long long path_pixels;
    int edge_spare;
    int pb_cursor;      // (path, band) pairs
    int bseg_cursor;    // band segments
    int entry_cursor;   // band list entries
    unsigned umin_r, umin_c, umax_r, umax_c;  // union bbox: max(BIAS - lo), max(BIAS + hi)
    int cell_cursor;    // (path, band, column tile) cells
    int max_band_entries;  // longest band list (sizes the tiles' entry bitmasks)
    unsigned long long spare8;
    int item_cursor;    // tile-list slots reserved (one per cell of a listed pair)
    int slab_cursor;    // work items of k_path_build (k_path_bbox cuts every path's cells into slabs)
    int pad[14];
    // Flattened edges are reserved in NSH independent shards (wave w of the flatten uses shard w % NSH): one hot
    // cursor serves only ~90 returning atomics per microsecond chip-wide, sixteen serve every wave of the launch.
    // One 128-byte line per cursor.
    struct ShardLine {
        int cursor;         // edges (k_flatten)
        int add_cursor;     // add slots (k_path_build: the slabs of path p reserve in shard p % n)
        unsigned rows_crossed;   // the plan's counting pass: rows the kept edges cross, + 1 per edge (sizes the add lists' first guess)
        unsigned cols_crossed;   // ... and columns
        int pad[28];
    } shard[16];
};
constexpr int NSH = 16;
static_assert(sizeof(BatchDev) == 128 + NSH * 128, "BatchDev is the head of the zero arena");

// Where the shards live in the edge arrays: shard s owns [base[s], base[s] + cap[s]); the capacities are the exact
// counts found by svgr_batch_plan, so for unchanged input the shards are full and the edge array is dense.
struct EdgeShards {
    int base[NSH];
    int cap[NSH];
};
// the same for the add slots k_path_build reserves (the slabs of path p in shard p % n; capacities measured by the plan)
struct AddShards {
    int base[NSH];
    int cap[NSH];
    int n;          // shards in use (1 .. NSH)
};
// is edge slot e filled?  (bases ascend; empty shards share a base with their successor)
__device__ __forceinline__ bool edge_live(int e, const EdgeShards& sh, const BatchDev* __restrict__ bd) {
    int s = 0;
#pragma unroll
    for (int k = 1; k < NSH; ++k) s += e >= sh.base[k] ? 1 : 0;
    const int filled = bd->shard[s].cursor < sh.cap[s] ? bd->shard[s].cursor : sh.cap[s];
    return e - sh.base[s] < filled;
}

__device__ __forceinline__ void store_edge(double* __restrict__ edges, int at, double r0, double c0, double r1, double c1) {
    typedef double f64x2e_t __attribute__((ext_vector_type(2)));
    f64x2e_t lo = {r0, c0}, hi = {r1, c1};
    f64x2e_t* e = (f64x2e_t*)(edges + 4 * (size_t)at);
    e[0] = lo; e[1] = hi;
}
__device__ __forceinline__ void load_seg_points(const double* __restrict__ segs, int s, const double* __restrict__ m6,
                                                int npts, double* c) {
    for (int k = 0; k < npts; ++k) {
        double px = segs[8 * (size_t)s + 2 * k], py = segs[8 * (size_t)s + 2 * k + 1];
        xform_point(m6, px, py, c[2 * k], c[2 * k + 1]);
    }
}

// Multi-GPU pre-pass: the rows a path can reach, from the hull of its transformed control points (a cubic and
// its de Casteljau halves stay inside it; +-1 row of slack for rounding, plus the bbox margin of S:966-975).
// prow[2p] = max(BIAS - lo), prow[2p + 1] = max(BIAS + hi): zero-initialised like the rest of the arena.
// k_flatten then skips every segment of a path that cannot reach one of this rank's bands: such a path has no
// pixel here, and skipping it whole is what lets the flatten scale with 1/ranks.
__global__ __launch_bounds__(256) void k_path_rows(const double* __restrict__ segs, const uint8_t* __restrict__ kind,
                                                   const int* __restrict__ seg_path, const double* __restrict__ path_m6,
                                                   int n_segs, unsigned* __restrict__ prow) {
    const int seg = blockIdx.x * blockDim.x + threadIdx.x;
    if (seg >= n_segs) return;
    const int p = seg_path[seg];
    const int npts = kind[seg] == SVGR_SEG_LINE ? 2 : 4;
    double c[8];
    load_seg_points(segs, seg, path_m6 + 6 * (size_t)p, npts, c);
    double rlo = c[0], rhi = c[0];
    bool finite = c[0] - c[0] == 0.0;
    for (int k = 1; k < npts; ++k) {
        rlo = c[2 * k] < rlo ? c[2 * k] : rlo;
        rhi = c[2 * k] > rhi ? c[2 * k] : rhi;
        finite = finite && (c[2 * k] - c[2 * k] == 0.0);
    }
    int lo = -(1 << 29), hi = 1 << 29;  // not finite: keep the path everywhere (the flatten reports it)
    if (finite) {
        lo = clamp_to_int(floor(rlo));
        hi = clamp_to_int(ceil(rhi));
        lo = lo < -(1 << 29) ? -(1 << 29) : lo;
        hi = hi > (1 << 29) ? (1 << 29) : hi;
    }
    atomicMax(&prow[2 * (size_t)p], (unsigned)(UNION_BIAS - lo));
    atomicMax(&prow[2 * (size_t)p + 1], (unsigned)(UNION_BIAS + hi));
}

// Multi-GPU, at plan time: the segments this rank has to flatten at all -- those of the paths whose row reach (k_path_rows)
// touches one of its bands -- as a compact list, so that a render's flatten launches over a rank's share of the drawing
// instead of over all of it (the reach of a path depends on the transforms alone: svgr_batch_set_transforms invalidates the
// plan).  The same distribution decision synth.rows_subscene makes on the host for the weak-scaling drawing.
__global__ __launch_bounds__(256) void k_seg_select(const int* __restrict__ seg_path, int n_segs, const unsigned* __restrict__ prow,
                                                    Owner own, int vr0, int n_bands, int* __restrict__ seg_list,
                                                    int* __restrict__ cursor) {
    const int seg = blockIdx.x * blockDim.x + threadIdx.x, lane = threadIdx.x & 63;
    bool take = false;
    if (seg < n_segs) {
        const int p = seg_path[seg];
        const int lo = UNION_BIAS - (int)prow[2 * (size_t)p], hi = (int)prow[2 * (size_t)p + 1] - UNION_BIAS;
        int ba = (lo - 2 - vr0) / TR, bb = (hi + 2 - vr0) / TR;
        ba = lo - 2 - vr0 < 0 ? 0 : ba;
        bb = bb > n_bands - 1 ? n_bands - 1 : bb;
        take = ba <= bb && owns_any(own, ba, bb);
    }
    const int at = wave_alloc(cursor, take ? 1 : 0, lane);
    if (take) seg_list[at] = seg;
}

// 32 lanes per segment.  Lane j owns the depth-5 node whose path bits are j (if the five ancestors
// above it are not flat; an ancestor that is flat is emitted by the lane whose remaining bits are 0).
// Per-path keys: {~key(min_r), ~key(min_c), key(max_r), key(max_c)}, all folded with atomicMax.
constexpr int FL_SUB = 5;                 // 32 lanes per segment: the longest lane bounds the kernel, so cut subtrees small
constexpr int FL_BLOCK = 256;     // (the waves are independent up to the last step: the segments of a workgroup fold their extents per path)
// PLACED (with EMIT): the pass stores the edges at the places the plan's counting pass left PER LANE (`lane_off`: a lane's first
// edge inside its segment's slots) -- one traversal that stores as it goes: no remembered end points, no prefix sum over the
// lanes, no second traversal for the lanes with many pieces.  The count a lane finds is checked against its place's size.
// SUB: log2 of the lanes a segment is cut over.  5 (32 lanes, two segments per wave) when the launch fills the chip: more lanes
// per segment repeat the upper levels for nothing (64 lanes: 39 against 28.8 us on the bench scene, round 4).  6 (a wave per
// segment) when it does NOT -- a drawing of a few thousand segments, one rank's share of a large one: the launch then lasts as
// long as its longest lane, and a lane of a 64-way cut has half the subtree (the tiger @ 2048: 31.5 us for 3 000 segments).
// SCAN (with EMIT, not PLACED): ONE traversal for a drawing whose edge places are not known yet -- a re-plan after
// svgr_batch_set_transforms.  The counting flatten + k_seg_scan + the placed flatten become one launch: a workgroup counts its
// lanes' pieces, finds where its segments' edges start by a decoupled look-back over the workgroups in front of it (`scan_state`:
// per workgroup {1 | its own total} as soon as it is counted, {2 | the total of everything up to and including it} once known;
// a wave reads 64 predecessors at a time), stores the edges there and leaves `seg_cnt / seg_off / lane_off` for the planned
// renders that follow.  Workgroups are dispatched in index order, so the lowest unfinished one is always resident and finds every
// predecessor finished: the chain cannot stall.  (A dead-man count ends a look-back that does not return all the same: error bit
// 2, the staged plan takes over.)
// LEAN (with EMIT and PLACED): the placed pass of a replay that keeps its slab table (run_geometry).  Nobody reads what such a pass
// leaves beside the edges -- k_path_bbox, the keys' only consumer, is not launched; the shard cursors are zeroed unread by the tile
// kernel -- and its inputs are those of the full placed pass in front of it, whose counts were compared with the plan's: no
// min / max keys (no fold, no LDS, no barrier, no atomics), no row reach, no counting atomic, no comparison of the counts.  The
// traversal is the full form's, and every store stays inside the lane's own place and the array: `at < n_plan`, `edge_cap`.
constexpr int FL_WAVES = 1;
template <bool EMIT, bool PLACED = false, int SUB = FL_SUB, bool SCAN = false, bool LEAN = false>
__global__ __launch_bounds__(FL_BLOCK, FL_WAVES) void k_flatten(const double* __restrict__ segs, const uint8_t* __restrict__ kind,
                                                 const int* __restrict__ seg_path, const double* __restrict__ path_m6,
                                                 int n_segs, double thr, double* __restrict__ edges,
                                                 int* __restrict__ edge_path, const EdgeShards sh,
                                                 unsigned long long* __restrict__ pkeys, BatchDev* __restrict__ bd,
                                                 Owner own, int vr0, int n_bands, const unsigned* __restrict__ prow,
                                                 const int* __restrict__ seg_list, int n_list,
                                                 int* __restrict__ seg_cnt, const int* __restrict__ seg_off, int edge_cap,
                                                 int* __restrict__ lane_off, int* __restrict__ seg_off_w = nullptr,
                                                 unsigned long long* __restrict__ scan_state = nullptr) {
    static_assert(!PLACED || EMIT, "places are what an emitting pass takes");
    static_assert(!SCAN || (EMIT && !PLACED), "the scanning pass counts, places and stores");
    static_assert(!LEAN || (EMIT && PLACED), "the lean form is a placed pass");
    // Where the edges go.  `seg_off` given (the renders and the plan's later passes): segment s owns the slots
    // [seg_off[s], seg_off[s + 1]) -- the exclusive prefix sums of the per-segment counts the plan's counting pass left in
    // `seg_cnt` -- and its lanes take them in curve order.  The edge array is then in (path, segment, curve) order whatever
    // the order the waves run in: the edges of a path are one contiguous range (k_path_build walks it), the array is the
    // same from render to render, and the kernel makes no returning atomic.  Without it (svgr_batch_all_edges): a
    // reservation per wave in one of NSH sharded cursors.
    const int gtid = blockIdx.x * FL_BLOCK + threadIdx.x;
    const int item = gtid >> SUB, sub = gtid & ((1 << SUB) - 1);
    // (multi-GPU: the plan's list of the segments this rank needs; else every segment)
    const int seg = seg_list ? (item < n_list ? seg_list[item] : n_segs) : item;
    bool seg_ok = seg < n_segs;
    // (where the segment's edges go: asked for here, with the segment itself -- behind the traversal it is a round trip of its own)
    const int so0 = seg_off && seg_ok ? seg_off[seg] : 0, so1 = seg_off && seg_ok ? seg_off[seg + 1] : 0;
    double node[8];
    int mode = 0;  // 0 nothing, 1 one edge node[0..1] -> node[6..7], 2 subtree under node
    int p = 0;
    if (seg_ok) p = seg_path[seg];
    if (seg_ok && prow) {
        // multi-GPU: a path none of whose rows can reach this rank's bands is skipped whole (k_path_rows)
        const int lo = UNION_BIAS - (int)prow[2 * (size_t)p], hi = (int)prow[2 * (size_t)p + 1] - UNION_BIAS;
        int ba = (lo - 2 - vr0) / TR, bb = (hi + 2 - vr0) / TR;
        ba = lo - 2 - vr0 < 0 ? 0 : ba;
        bb = bb > n_bands - 1 ? n_bands - 1 : bb;
        seg_ok = ba <= bb && owns_any(own, ba, bb);
    }
    if (seg_ok) {
        const double* m6 = path_m6 + 6 * (size_t)p;
        if (kind[seg] == SVGR_SEG_LINE) {
            if (sub == 0) {
                double c[4];
                load_seg_points(segs, seg, m6, 2, c);
                node[0] = c[0]; node[1] = c[1]; node[6] = c[2]; node[7] = c[3];
                mode = 1;
            }
        } else {
            load_seg_points(segs, seg, m6, 4, node);
            mode = 2;
            for (int l = 0; l < SUB; ++l) {
                if (cubic_flatness(node) < thr) {
                    mode = (sub & ((1 << (SUB - l)) - 1)) == 0 ? 1 : 0;
                    break;
                }
                if ((sub >> (SUB - 1 - l)) & 1) cubic_right_inplace(node); else cubic_left_inplace(node);
            }
        }
    }
    // Multi-GPU: a rank needs the exact bbox of every path it keeps (so the first traversal always runs and
    // tracks min/max over ALL segments of such a path), but it only stores the edges of segments that can
    // reach one of its own bands (the curve stays inside the row range of its control points; +-1 row of slack).
    bool keep = true;
    if (!LEAN && n_bands > 0 && mode != 0) {  // (also drops what lies entirely above / below the viewport)
        double rlo = node[0] < node[6] ? node[0] : node[6], rhi = node[0] < node[6] ? node[6] : node[0];
        if (mode == 2) {
            rlo = fmin(rlo, fmin(node[2], node[4]));
            rhi = fmax(rhi, fmax(node[2], node[4]));
        }
        // (rows far outside the viewport are brought to its border in double: the integer arithmetic below stays in range)
        const double v_lo = (double)vr0 - 4.0, v_hi = (double)vr0 + (double)n_bands * TR + 4.0;
        rlo = rlo < v_lo ? v_lo : (rlo > v_hi ? v_hi : rlo);
        rhi = rhi < v_lo ? v_lo : (rhi > v_hi ? v_hi : rhi);
        int ba = (clamp_to_int(floor(rlo)) - 1 - vr0) / TR, bb = (clamp_to_int(ceil(rhi)) + 1 - vr0) / TR;
        ba = clamp_to_int(floor(rlo)) - 1 - vr0 < 0 ? 0 : ba;
        bb = bb > n_bands - 1 ? n_bands - 1 : bb;
        keep = ba <= bb && owns_any(own, ba, bb);
    }
    double mnr = INFINITY, mnc = INFINITY, mxr = -INFINITY, mxc = -INFINITY;
    auto track = [&](double r, double c) {
        if constexpr (LEAN) return;
        mnr = r < mnr ? r : mnr; mxr = r > mxr ? r : mxr;
        mnc = c < mnc ? c : mnc; mxc = c > mxc ? c : mxc;
    };
    int cnt = 0;
    bool ovf = false;
    constexpr int FL_ENDS = 4;  // pieces a lane remembers from its counting traversal (a wave skips the second one when all its lanes fit)
    double qe[2 * FL_ENDS];
    for (int k = 0; k < 2 * FL_ENDS; ++k) qe[k] = 0.0;
    // (the plan's counting pass also adds up the rows and columns the kept pieces cross: what the first guess of the add lists'
    //  size is made from -- batch_plan_two_pass)
    constexpr int SEGL_ = 1 << SUB;  // lanes per segment
    if constexpr (PLACED) {
        // this lane's place: [first, first + n_plan) of its segment's slots
        int first = seg_ok ? lane_off[(size_t)seg * SEGL_ + sub] : 0;
        int nxt = __shfl_down(first, 1);
        if (sub == SEGL_ - 1) nxt = so1 - so0;
        const int n_plan = seg_ok ? nxt - first : 0;
        const int base_p = so0 + first;
        int n_found = 0;
        if (mode == 1) {
            track(node[0], node[1]);
            track(node[6], node[7]);
            n_found = 1;
            if (n_plan >= 1 && base_p < edge_cap) {
                store_edge(edges, base_p, node[0], node[1], node[6], node[7]);
                if (edge_path) edge_path[base_p] = p;   // (null in a replay: the plan's pass has written it)
            }
        } else if (mode == 2) {
            track(node[0], node[1]);
            int at = 0;
            n_found = flatten_subtree<1>(node, thr, kMaxFlattenDepth - SUB, [&](double r0_, double c0_, double r1, double c1) {
                track(r1, c1);
                if (at < n_plan && base_p + at < edge_cap) {
                    store_edge(edges, base_p + at, r0_, c0_, r1, c1);
                    if (edge_path) edge_path[base_p + at] = p;
                }
                ++at;
            }, ovf);
        }
        if (ovf) atomicOr(&bd->err, 1);
        // (a lane whose pieces cannot reach this rank's rows has an empty place; any other count that differs is not the plan's geometry)
        if (!LEAN && keep && n_found != n_plan) atomicOr(&bd->err, 2);
        // (the shard cursors only count: their sum is the number of edges the pass kept)
        if (!LEAN && seg_ok && sub == 0 && so1 > so0) atomicAdd(&bd->shard[(int)((blockIdx.x * (FL_BLOCK / 64) + (threadIdx.x >> 6)) % NSH)].cursor, so1 - so0);
    } else {
    const bool census = !EMIT && seg_cnt != nullptr;
    double rows_x = 0.0, cols_x = 0.0;
    if (mode == 1) {
        cnt = 1;
        track(node[0], node[1]);
        track(node[6], node[7]);
        if (census) { rows_x = fabs(node[6] - node[0]); cols_x = fabs(node[7] - node[1]); }
    } else if (mode == 2) {
        // pieces come in curve order and share end points: track the first start and every end.  The ends of the
        // first two pieces are remembered: nearly every lane has one or two, and then the second traversal is skipped.
        track(node[0], node[1]);
        cnt = flatten_subtree<FL_ENDS>(node, thr, kMaxFlattenDepth - SUB, [&](double r0_, double c0_, double r1, double c1) {
            track(r1, c1);
            if (census) { rows_x += fabs(r1 - r0_); cols_x += fabs(c1 - c0_); }
        }, ovf, qe);
    }
    if (ovf) atomicOr(&bd->err, 1);
    if (!keep) { cnt = 0; rows_x = 0.0; cols_x = 0.0; }
    const int shard = (int)((blockIdx.x * (FL_BLOCK / 64) + (threadIdx.x >> 6)) % NSH);
    if (census) {
        // (a piece crosses |dr| + 1 rows at most; what lies outside the viewport's rows is counted too: a guess's upper side)
        const double cap = (double)(n_bands > 0 ? (n_bands * TR + 8) * (cnt > 0 ? cnt : 1) : 1 << 22);
        const int mine = cnt > 0 ? (int)(rows_x < cap ? rows_x : cap) + cnt : 0;
        int wrows;
        (void)wave_excl_scan(mine < (1 << 24) ? mine : (1 << 24), threadIdx.x & 63, wrows);
        if ((threadIdx.x & 63) == 0 && wrows > 0) atomicAdd(&bd->shard[shard].rows_crossed, (unsigned)wrows);
        // (columns: a piece cannot make adds beyond the viewport's columns -- what lies left of it folds into column 0, what lies right
        //  of the layer is dropped --; `edge_cap`, unused by a counting pass, carries the viewport's width)
        const double ccap = (double)(edge_cap > 0 ? (edge_cap + 8) * (cnt > 0 ? cnt : 1) : 1 << 22);
        const int minec = cnt > 0 ? (int)(cols_x < ccap ? cols_x : ccap) : 0;
        int wcols;
        (void)wave_excl_scan(minec < (1 << 24) ? minec : (1 << 24), threadIdx.x & 63, wcols);
        if ((threadIdx.x & 63) == 0 && wcols > 0) atomicAdd(&bd->shard[shard].cols_crossed, (unsigned)wcols);
    }
    int base;
    bool fits;
    if constexpr (SCAN) {
        const int lane = threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
        constexpr int NWV = FL_BLOCK / 64;
        __shared__ int s_wt[NWV];
        __shared__ int s_base;
        int wtot;
        const int excl = wave_excl_scan(cnt, lane, wtot);
        constexpr int SEGL = 1 << SUB;  // lanes per segment
        const int seg_first = __shfl(excl, lane & ~(SEGL - 1)), seg_total = __shfl(excl + cnt, lane | (SEGL - 1)) - seg_first;
        if (lane == 0) s_wt[wave] = wtot;
        if (lane == 0 && wtot > 0) atomicAdd(&bd->shard[shard].cursor, wtot);   // (the shard cursors only count: their sum = the edges kept)
        __syncthreads();
        int before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < NWV; ++w) { before += w < wave ? s_wt[w] : 0; all += s_wt[w]; }
        if (wave == 0) {
            const int me = (int)blockIdx.x;
            if (lane == 0)
                __hip_atomic_store(&scan_state[me], ((me == 0 ? 2ull : 1ull) << 32) | (unsigned long long)(unsigned)all, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            int acc = 0;
            if (me > 0) {
                int j0 = me - 1;
                unsigned spins = 0;
                bool dead = false;
                for (;;) {
                    // (one window of 64 predecessors per step; two per step with both loads in flight and no pause between polls measured
                    //  SLOWER, 55 against 49 us: the polls of a thousand resident workgroups are what the counting ones wait behind)
                    const int j = j0 - lane;
                    const unsigned long long sv = j >= 0 ? __hip_atomic_load(&scan_state[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : (2ull << 32);
                    const unsigned status = (unsigned)(sv >> 32);
                    const unsigned long long m2 = __ballot(status == 2u), m0 = __ballot(status == 0u);
                    const int first2 = m2 ? __ffsll((long long)m2) - 1 : 64;   // the nearest predecessor whose running total is known
                    const unsigned long long need = first2 >= 63 ? ~0ull : ((2ull << first2) - 1ull);
                    if (m0 & need) {   // (somebody in front of it has not counted yet)
                        if (++spins > (1u << 20)) { dead = true; break; }
                        __builtin_amdgcn_s_sleep(8);
                        continue;
                    }
                    int tot;
                    (void)wave_excl_scan(lane <= first2 ? (int)(unsigned)sv : 0, lane, tot);
                    acc += tot;
                    if (first2 < 64) break;
                    j0 -= 64;
                }
                if (dead) { if (lane == 0) atomicOr(&bd->err, 2); acc = 0x3fffffff; }   // (nothing of this workgroup fits; the successors do not wait)
                if (lane == 0)
                    __hip_atomic_store(&scan_state[me], (2ull << 32) | (unsigned long long)(unsigned)(acc + all), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            if (lane == 0) s_base = acc;
        }
        __syncthreads();
        const int wg_base = s_base;
        base = wg_base + before + excl;
        fits = base + cnt <= edge_cap && wg_base < 0x3fffffff;
        if (seg_ok && sub == 0) { seg_cnt[seg] = seg_total; seg_off_w[seg] = wg_base + before + seg_first; }
        if (seg_ok) lane_off[(size_t)seg * SEGL + sub] = excl - seg_first;
        if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) seg_off_w[n_segs] = wg_base + all;
    } else if (seg_cnt || seg_off) {
        // this lane's place among the edges of its segment (the 32 lanes of a segment are half a wave), the segment's count
        const int lane = threadIdx.x & 63;
        int wtot;
        const int excl = wave_excl_scan(cnt, lane, wtot);
        constexpr int SEGL = 1 << SUB;  // lanes per segment
        const int seg_first = __shfl(excl, lane & ~(SEGL - 1)), seg_total = __shfl(excl + cnt, lane | (SEGL - 1)) - seg_first;
        if (seg_cnt && seg_ok && sub == 0) seg_cnt[seg] = seg_total;
        if (seg_cnt && lane_off && seg_ok) lane_off[(size_t)seg * SEGL + sub] = excl - seg_first;   // (the lane's place inside its segment's slots)
        const int s0 = so0, s1 = so1;
        base = s0 + (excl - seg_first);
        fits = base + cnt <= s1 && base + cnt <= edge_cap;
        // (the shard cursors only count here: their sum is the number of edges the pass kept)
        if (lane == 0 && wtot > 0) atomicAdd(&bd->shard[shard].cursor, wtot);
    } else {
        // one reservation per wave, in the wave's shard
        const int in_shard = wave_alloc(&bd->shard[shard].cursor, cnt, threadIdx.x & 63);
        base = sh.base[shard] + in_shard;
        fits = in_shard + cnt <= sh.cap[shard];
    }

    if (EMIT && cnt > 0) {
        if (!fits) {
            atomicOr(&bd->err, 2);
        } else if (mode == 1) {
            store_edge(edges, base, node[0], node[1], node[6], node[7]);
            edge_path[base] = p;
        } else if (cnt <= FL_ENDS) {
            store_edge(edges, base, node[0], node[1], qe[0], qe[1]);
            edge_path[base] = p;
#pragma unroll
            for (int k = 1; k < FL_ENDS; ++k)
                if (k < cnt) {
                    store_edge(edges, base + k, qe[2 * k - 2], qe[2 * k - 1], qe[2 * k], qe[2 * k + 1]);
                    edge_path[base + k] = p;
                }
        } else {
            {
            int i = 0;
            bool o2 = false;
            flatten_subtree(node, thr, kMaxFlattenDepth - SUB, [&](double r0, double c0, double r1, double c1) {
                if (i < cnt) {
                    store_edge(edges, base + i, r0, c0, r1, c1);
                    edge_path[base + i] = p;
                }
                ++i;
            }, o2);
            }
        }
    }
    }  // (!PLACED)
    if constexpr (!LEAN) {
    // fold the lanes of a segment, then one set of atomics per segment
#pragma unroll
    for (int d = 1; d < (1 << SUB); d <<= 1) {
        double a = __shfl_xor(mnr, d), b = __shfl_xor(mnc, d), c = __shfl_xor(mxr, d), e = __shfl_xor(mxc, d);
        mnr = a < mnr ? a : mnr; mnc = b < mnc ? b : mnc;
        mxr = c > mxr ? c : mxr; mxc = e > mxc ? e : mxc;
    }
    // ... then the workgroup's segments of ONE path together (they are consecutive): a path of hundreds of segments -- the
    // tiger's outlines -- made hundreds of atomics on the same four addresses, which the memory side serves one after the other:
    // 25 of the 31 us the tiger's flatten took (round 5: the same launch without the atomics 8.8 us)
    constexpr int NSEG = FL_BLOCK >> SUB;   // segments of a workgroup
    __shared__ double s_mm[NSEG][4];
    __shared__ int s_mp[NSEG];
    const int sidx = (int)threadIdx.x >> SUB;
    if (sub == 0) {
        s_mp[sidx] = seg_ok && mnr <= mxr ? p : -1;
        s_mm[sidx][0] = mnr; s_mm[sidx][1] = mnc; s_mm[sidx][2] = mxr; s_mm[sidx][3] = mxc;
    }
    __syncthreads();
    if (sub == 0 && s_mp[sidx] >= 0 && (sidx == 0 || s_mp[sidx - 1] != s_mp[sidx])) {   // (the first segment of a run of one path's)
        for (int j = sidx + 1; j < NSEG && s_mp[j] == p; ++j) {
            mnr = s_mm[j][0] < mnr ? s_mm[j][0] : mnr; mnc = s_mm[j][1] < mnc ? s_mm[j][1] : mnc;
            mxr = s_mm[j][2] > mxr ? s_mm[j][2] : mxr; mxc = s_mm[j][3] > mxc ? s_mm[j][3] : mxc;
        }
        unsigned long long* k = pkeys + 4 * (size_t)p;
        atomicMax(&k[0], ~f64_key(mnr));
        atomicMax(&k[1], ~f64_key(mnc));
        atomicMax(&k[2], f64_key(mxr));
        atomicMax(&k[3], f64_key(mxc));
    }
    }  // (!LEAN)
}

// ======================================================================================
// Hit testing kernels (svgr_batch_winding, svgr_batch_pick: the entries are at the end of the file).  They stand here, in front
// of the tile kernel: its out-of-line class-1 bodies sit at the END of the text section and are reached by 16-bit branches, so
// nothing may grow between it and that end.
// ======================================================================================
#include "svgr_hit.h"

// Grouping the flattened edges by path (the flatten leaves them in sixteen shards, in the order its waves came by): count per
// path, place by a cursor per path (the order inside a path is whatever the atomics give: a winding number is an integer sum),
// then the extents, a wave per path.
__global__ __launch_bounds__(256) void k_hit_count(const int* __restrict__ edge_path, long long n, int n_paths, int* __restrict__ cnt) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const int p = edge_path[e];
    if (p >= 0 && p < n_paths) atomicAdd(&cnt[p], 1);
}
__global__ __launch_bounds__(256) void k_hit_place(const double* __restrict__ in, const int* __restrict__ edge_path, long long n, int n_paths,
                                                   const int* __restrict__ off, int* __restrict__ cur, double* __restrict__ out) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const int p = edge_path[e];
    if (p < 0 || p >= n_paths) return;
    const int at = off[p] + atomicAdd(&cur[p], 1);
    if (at >= off[p + 1]) return;   // (cannot be: the counts are this array's own)
    const double2* src = (const double2*)(in + 4 * e);
    double2* dst = (double2*)(out + 4 * (size_t)at);
    dst[0] = src[0]; dst[1] = src[1];
}
__global__ __launch_bounds__(64) void k_hit_extent(const double* __restrict__ edges, const int* __restrict__ off, int n_paths, double* __restrict__ ext) {
    const int p = blockIdx.x;
    if (p >= n_paths) return;
    double mna = INFINITY, mnb = INFINITY, mxa = -INFINITY, mxb = -INFINITY;
    for (int e = off[p] + (int)threadIdx.x; e < off[p + 1]; e += 64) {
        const double2 q0 = ((const double2*)(edges + 4 * (size_t)e))[0], q1 = ((const double2*)(edges + 4 * (size_t)e))[1];
        mna = fmin(mna, fmin(q0.x, q1.x)); mxa = fmax(mxa, fmax(q0.x, q1.x));
        mnb = fmin(mnb, fmin(q0.y, q1.y)); mxb = fmax(mxb, fmax(q0.y, q1.y));
    }
    for (int d = 32; d > 0; d >>= 1) {
        mna = fmin(mna, __shfl_xor(mna, d)); mnb = fmin(mnb, __shfl_xor(mnb, d));
        mxa = fmax(mxa, __shfl_xor(mxa, d)); mxb = fmax(mxb, __shfl_xor(mxb, d));
    }
    if (threadIdx.x == 0) { ext[4 * p] = mna; ext[4 * p + 1] = mnb; ext[4 * p + 2] = mxa; ext[4 * p + 3] = mxb; }
}

// Where the lanes of a workgroup find their points: an array on the device, HIT_BLOCK consecutive points to a workgroup, or the
// pixel centres of a grid, a HIT_TILE x HIT_TILE tile to a workgroup (compact, so that the cull below bites).  `id` is the
// point's place in the caller's row-major order.
struct HitQuery {
    const double* pts;
    long long n;
    long long row0, col0, rows, cols, tiles_x;
};
__device__ __forceinline__ bool hit_point(const HitQuery& q, long long group, int lane, double& pa, double& pb, long long& id) {
    if (q.pts) {
        id = group * HIT_BLOCK + lane;
        if (id >= q.n) return false;
        pa = q.pts[2 * id]; pb = q.pts[2 * id + 1];
        return true;
    }
    const long long r = (group / q.tiles_x) * HIT_TILE + lane / HIT_TILE, c = (group % q.tiles_x) * HIT_TILE + lane % HIT_TILE;
    if (r >= q.rows || c >= q.cols) return false;
    id = r * q.cols + c;
    pa = (double)(q.row0 + r) + 0.5; pb = (double)(q.col0 + c) + 0.5;
    return true;
}

// ---- The workgroup frame of the point queries: k_hit_winding, k_sdf_distance and k_msdf_distance are these four pieces around
// what each of them keeps per point.  A workgroup has HIT_BLOCK points and meets every path: the points' box is reduced once;
// the paths are taken HIT_BLOCK at a time, a lane each, and tested against the box (the kernel's cull); the edges of a path that
// stays go through LDS HIT_CHUNK at a time, prepared by the staging lane, and every lane reads the same address (a broadcast)
// and keeps what it accumulates for its own point in registers.  The pieces take the kernel's parts as callables and know nothing
// of the kernel that calls them; every barrier of the three kernels is in here.

// The lane's point, and whether the lane has one.  A lane without a point and a point with a NaN or infinite coordinate go on
// as NaN: every compare with an edge is false and every d2 is NaN, which fmin drops -- winding 0, +inf away, nothing kept.
__device__ __forceinline__ bool hit_point_or_nan(const HitQuery& q, long long group, int lane, double& pa, double& pb, long long& id) {
    pa = pb = 0.0;
    id = 0;
    const bool live = hit_point(q, group, lane, pa, pb, id);
    if (!live || !hit_finite(pa, pb)) pa = pb = NAN;
    return live;
}

// The box of the workgroup's finite points and their smallest |pb| (svgr_hit.h's HitBox), the same in every lane: shuffles
// inside a wave, a row of `s_red` per value across the waves.
__device__ __forceinline__ HitBox hit_point_box(double pa, double pb, int lane, double (*s_red)[HIT_BLOCK / 64]) {
    const bool fin = pa == pa;
    double lo_a = fin ? pa : INFINITY, hi_a = fin ? pa : -INFINITY, lo_b = fin ? pb : INFINITY, hi_b = fin ? pb : -INFINITY;
    double min_absb = fin ? fabs(pb) : INFINITY;
    for (int d = 32; d > 0; d >>= 1) {
        lo_a = fmin(lo_a, __shfl_xor(lo_a, d)); hi_a = fmax(hi_a, __shfl_xor(hi_a, d));
        lo_b = fmin(lo_b, __shfl_xor(lo_b, d)); hi_b = fmax(hi_b, __shfl_xor(hi_b, d));
        min_absb = fmin(min_absb, __shfl_xor(min_absb, d));
    }
    if ((lane & 63) == 0) {
        s_red[0][lane >> 6] = lo_a; s_red[1][lane >> 6] = hi_a; s_red[2][lane >> 6] = lo_b; s_red[3][lane >> 6] = hi_b;
        s_red[4][lane >> 6] = min_absb;
    }
    __syncthreads();
    for (int k = 0; k < HIT_BLOCK / 64; ++k) {
        lo_a = fmin(lo_a, s_red[0][k]); hi_a = fmax(hi_a, s_red[1][k]); lo_b = fmin(lo_b, s_red[2][k]); hi_b = fmax(hi_b, s_red[3][k]);
        min_absb = fmin(min_absb, s_red[4][k]);
    }
    return HitBox{lo_a, hi_a, lo_b, hi_b, min_absb};
}

// The table rounds.  The lane of path p asks `keep(p, e0, e1)` about its edges e0 .. e1 (a path not kept goes into the table
// without edges); then every lane calls `path(p, j, e0, e1)` for the round's paths in order, j the path's place in the table
// and e0, e1 scalars.  What a kernel tables of its own beside s_e0 / s_e1 it stores in `keep` and reads in `path`, at j.
template <class Keep, class Path>
__device__ __forceinline__ void hit_table_rounds(const int* __restrict__ off, int n_paths, int lane, int* s_e0, int* s_e1, Keep&& keep, Path&& path) {
    for (int base = 0; base < n_paths; base += HIT_BLOCK) {
        __syncthreads();   // (the previous round's table has been read)
        {
            const int p = base + lane;
            int e0 = 0, e1 = 0;
            if (p < n_paths) {
                e0 = off[p]; e1 = off[p + 1];
                if (!keep(p, e0, e1)) e1 = e0;
            }
            s_e0[lane] = e0; s_e1[lane] = e1;
        }
        __syncthreads();
        const int n_here = n_paths - base < HIT_BLOCK ? n_paths - base : HIT_BLOCK;
        for (int j = 0; j < n_here; ++j)
            path(base + j, j, __builtin_amdgcn_readfirstlane(s_e0[j]), __builtin_amdgcn_readfirstlane(s_e1[j]));
    }
}

// The chunk walk over the edges e0 .. e1 of one path (scalars).  The staging lane loads its edge, `prepare(a0, b0, a1, b1, pe)`
// makes the ED doubles of it that the walk wants, and `each(staged)` sees every staged edge as ED / 2 double2 of LDS.
template <int ED, class Prepare, class Each>
__device__ __forceinline__ void hit_chunk_walk(const double* __restrict__ edges, int e0, int e1, int lane, double* s_e, Prepare&& prepare, Each&& each) {
    static_assert(ED % 2 == 0, "a staged edge is whole double2");
    for (int c0 = e0; c0 < e1; c0 += HIT_CHUNK) {
        const int n = e1 - c0 < HIT_CHUNK ? e1 - c0 : HIT_CHUNK;
        __syncthreads();   // (the previous chunk has been read)
        if (lane < n) {
            const double2* src = (const double2*)(edges + 4 * (size_t)(c0 + lane));
            const double2 q0 = src[0], q1 = src[1];
            double pe[ED];
            prepare(q0.x, q0.y, q1.x, q1.y, pe);
            double2* dst = (double2*)s_e + (ED / 2) * lane;
#pragma unroll
            for (int i = 0; i < ED / 2; ++i) dst[i] = make_double2(pe[2 * i], pe[2 * i + 1]);
        }
        __syncthreads();
        for (int k = 0; k < n; ++k) each((const double2*)s_e + (ED / 2) * k);
    }
}

// Winding numbers.  The cull: a path is skipped when its b range misses the points' (no edge is then `up` or `down` for any of
// them) or when it lies wholly at a <= min(pa) (every d of an `up` edge is then <= 0 and of a `down` edge >= 0, in the rounded
// arithmetic as well: the differences and products of svgr_hit.h are monotone).  A lane keeps its point's winding number.
// BITS: one inside bit per (point, path) into row `slot` of `bits` (32 paths to a word); else the winding numbers into wind[id].
template <bool BITS>
__global__ __launch_bounds__(HIT_BLOCK) void k_hit_winding(const double* __restrict__ edges, const int* __restrict__ off, const double* __restrict__ ext,
                                                           const uint8_t* __restrict__ rule, int n_paths, const HitQuery q, long long group0,
                                                           int* __restrict__ wind, uint32_t* __restrict__ bits, int words) {
    __shared__ __align__(16) double s_e[4 * HIT_CHUNK];
    __shared__ double s_red[5][HIT_BLOCK / 64];
    __shared__ int s_e0[HIT_BLOCK], s_e1[HIT_BLOCK];
    const int lane = threadIdx.x;
    double pa, pb;
    long long id;
    const bool live = hit_point_or_nan(q, group0 + blockIdx.x, lane, pa, pb, id);
    const HitBox box = hit_point_box(pa, pb, lane, s_red);
    const size_t row = (size_t)((long long)blockIdx.x * HIT_BLOCK + lane) * (size_t)words;
    uint32_t word = 0u;
    hit_table_rounds(
        off, n_paths, lane, s_e0, s_e1,
        [&](int p, int e0, int e1) {
            const double mnb = ext[4 * p + 1], mxa = ext[4 * p + 2], mxb = ext[4 * p + 3];
            // (& between the three: with && the compiler loads the numbers one behind the other's compare)
            return e1 > e0 && ((box.hi_b >= mnb) & (box.lo_b < mxb) & (mxa > box.lo_a));
        },
        [&](int p, int, int e0, int e1) {
            int w = 0;
            hit_chunk_walk<4>(
                edges, e0, e1, lane, s_e, [](double a0, double b0, double a1, double b1, double* pe) { pe[0] = a0; pe[1] = b0; pe[2] = a1; pe[3] = b1; },
                [&](const double2* s) {
                    const double2 q0 = s[0], q1 = s[1];
                    w += hit_edge_term(q0.x, q0.y, q1.x, q1.y, pa, pb);
                });
            if constexpr (BITS) {
                if (hit_inside(w, rule[p] & 1)) word |= 1u << (p & 31);
                if ((p & 31) == 31 || p == n_paths - 1) {
                    if (live) bits[row + (size_t)(p >> 5)] = word;
                    word = 0u;
                }
            } else {
                if (live) wind[(size_t)id * (size_t)n_paths + (size_t)p] = w;
            }
        });
}

// a lane per point: the clips and the paint order over its row of bits (svgr_hit.h), in place
__global__ __launch_bounds__(HIT_BLOCK) void k_hit_resolve(uint32_t* __restrict__ bits, int words, int n_paths, const HitQuery q, long long group0,
                                                           const uint8_t* __restrict__ pickable, const int32_t* __restrict__ clip_off,
                                                           const int32_t* __restrict__ clip_group, const int32_t* __restrict__ group_off,
                                                           const int32_t* __restrict__ group_src, int32_t* __restrict__ top) {
    double pa, pb;
    long long id;
    if (!hit_point(q, group0 + blockIdx.x, threadIdx.x, pa, pb, id)) return;
    uint32_t* row = bits + (size_t)((long long)blockIdx.x * HIT_BLOCK + threadIdx.x) * (size_t)words;
    top[id] = hit_resolve(row, n_paths, pickable, clip_off, clip_group, group_off, group_src);
}

// ======================================================================================
// Signed distance fields (svgr_batch_distance: the entry is at the end of the file; the arithmetic: svgr_sdf.h).
// In front of the tile kernel for the same reason as the hit kernels.
// ======================================================================================
#include "svgr_sdf.h"

// one value in the encoding OUT (SDF_*) to element `at` of `out`
template <int OUT>
__device__ __forceinline__ void sdf_store(void* __restrict__ out, size_t at, double v, double spread) {
    if constexpr (OUT == SDF_F64) ((double*)out)[at] = v;
    else if constexpr (OUT == SDF_F32) ((float*)out)[at] = sdf_encode_f32(v, spread);
    else ((uint8_t*)out)[at] = sdf_encode_u8(v, spread);
}

// Distances, on the point queries' frame (above).  The staging lane works out x, y and inv once per edge (sdf_edge_prepare), so
// that the walk over the points has no division.  A lane keeps its point's min d2 and winding number and takes one sqrt per path.
// The cull is sdf_out_of_reach of svgr_sdf.h on the path's extent (finite `cull_spread` only; the host passes +inf for an
// infinite spread and for one below 2^-100): a path out of reach is skipped and counts as +spread, which DESIGN.md 7r shows to
// be what the walk gives every point of the workgroup as well, so the cull cannot show.
// OUT: the encoding (SDF_*).  UNION: one value per point, the minimum over the paths; else one per (point, path).  Results go to
// out[(id - id0) * stride + p] in elements of the encoding: the caller's row-major order, the pass beginning at point id0.
template <int OUT, bool UNION>
__global__ __launch_bounds__(HIT_BLOCK) void k_sdf_distance(const double* __restrict__ edges, const int* __restrict__ off, const double* __restrict__ ext,
                                                            const uint8_t* __restrict__ rule, int n_paths, const HitQuery q, long long group0,
                                                            long long id0, double spread, double cull_spread, int is_signed, void* __restrict__ out) {
    __shared__ __align__(16) double s_e[SDF_EDGE_DOUBLES * HIT_CHUNK];
    __shared__ double s_red[5][HIT_BLOCK / 64];
    __shared__ int s_e0[HIT_BLOCK], s_e1[HIT_BLOCK];
    const int lane = threadIdx.x;
    double pa, pb;
    long long id;
    const bool live = hit_point_or_nan(q, group0 + blockIdx.x, lane, pa, pb, id);
    const HitBox box = hit_point_box(pa, pb, lane, s_red);
    const size_t stride = UNION ? 1 : (size_t)n_paths;
    const size_t at = (size_t)(id - id0) * stride;
    double best = spread;   // (UNION: a skipped path counts as +spread, and no path can give more)
    hit_table_rounds(
        off, n_paths, lane, s_e0, s_e1, [&](int p, int e0, int e1) { return !(e1 > e0 && sdf_out_of_reach(ext + 4 * p, box, cull_spread)); },
        [&](int p, int, int e0, int e1) {
            double v = spread;
            if (e1 > e0) {
                double m = INFINITY;
                int w = 0;
                hit_chunk_walk<SDF_EDGE_DOUBLES>(
                    edges, e0, e1, lane, s_e, [](double a0, double b0, double a1, double b1, double* pe) { sdf_edge_prepare(a0, b0, a1, b1, pe); },
                    [&](const double2* s) {
                        const double2 ab = s[0], xy = s[1], ib = s[2];
                        const double da = pa - ab.x, db = pb - ab.y;
                        m = fmin(m, sdf_edge_d2(ab.x, ab.y, xy.x, xy.y, ib.x, pa, pb, da, db));
                        w += sdf_edge_term(ab.y, ib.y, xy.x, xy.y, pb, da, db);
                    });
                v = sdf_finish(m, w, rule[p] & 1, is_signed, spread);
            }
            if constexpr (UNION) best = fmin(best, v);
            else if (live) sdf_store<OUT>(out, at + (size_t)p, v, spread);
        });
    if constexpr (UNION)
        if (live) sdf_store<OUT>(out, at, best, spread);
}

// ======================================================================================
// Multi-channel distance fields (svgr_batch_msdf: the entry is at the end of the file; the arithmetic: svgr_msdf.h).
// ======================================================================================
#include "svgr_msdf.h"

// what the host says of a path in k_msdf_distance's table: its colour mask in bits 0 .. 2, and of the group it belongs to
constexpr int MSDF_PATH_LAST = 8, MSDF_PATH_NEGATIVE = 16, MSDF_PATH_EVENODD = 32;   // the group ends here; sigma = -1; its fill rule

// a lane per group: the union of its paths' extents (a path without edges has the empty extent +inf .. -inf, which changes nothing)
__global__ __launch_bounds__(256) void k_msdf_group_extent(const double* __restrict__ ext, const int32_t* __restrict__ group_off, int n_groups,
                                                            double* __restrict__ gext) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= n_groups) return;
    double mna = INFINITY, mnb = INFINITY, mxa = -INFINITY, mxb = -INFINITY;
    for (int p = group_off[g]; p < group_off[g + 1]; ++p) {
        mna = fmin(mna, ext[4 * p]); mnb = fmin(mnb, ext[4 * p + 1]); mxa = fmax(mxa, ext[4 * p + 2]); mxb = fmax(mxb, ext[4 * p + 3]);
    }
    gext[4 * g] = mna; gext[4 * g + 1] = mnb; gext[4 * g + 2] = mxa; gext[4 * g + 3] = mxb;
}

// Multi-channel distances, on the point queries' frame, over GROUPS of paths: the paths 0 .. n_paths of the table are the groups'
// runs one after the other, path_info[p] has the path's colour mask and MSDF_PATH_* of its group (tabled in s_info beside the
// edges), path_group[p] the group.  The staging lane prepares 8 doubles per edge (msdf_edge_prepare).  The cull is
// sdf_out_of_reach on the union of the group's extents (gext): it skips a group as a whole, never a single path of one, because
// only the group's edges together close (colour_edges deals a subpath's segments out to several paths) and because a channel may
// keep an edge of any of them.  DESIGN.md 7s: the spread guard of msdf_finish makes the skipped group's four values exactly the
// +spread they count as.
// A lane keeps one MsdfState in registers: A's min d2 and winding number and (d2, o, perp) for each of the three channels.  It
// lives across the rounds of the table, as a group may straddle two; at a group's last path the lane takes the one sqrt, the
// repair and the union.  A path's mask is wave-uniform, so the channel updates of msdf_edge sit behind scalar branches.
// Results: out[4 * (id - id0) + {0, 1, 2, 3}] = R, G, B, A in elements of the encoding.
template <int OUT>
__global__ __launch_bounds__(HIT_BLOCK) void k_msdf_distance(const double* __restrict__ edges, const int* __restrict__ off, const double* __restrict__ gext,
                                                             const uint8_t* __restrict__ path_info, const int32_t* __restrict__ path_group, int n_paths,
                                                             const HitQuery q, long long group0, long long id0, double spread, double cull_spread,
                                                             void* __restrict__ out) {
    __shared__ __align__(16) double s_e[MSDF_EDGE_DOUBLES * HIT_CHUNK];
    __shared__ double s_red[5][HIT_BLOCK / 64];
    __shared__ int s_e0[HIT_BLOCK], s_e1[HIT_BLOCK], s_info[HIT_BLOCK];
    const int lane = threadIdx.x;
    double pa, pb;
    long long id;
    const bool live = hit_point_or_nan(q, group0 + blockIdx.x, lane, pa, pb, id);
    const bool fin = pa == pa;
    const HitBox box = hit_point_box(pa, pb, lane, s_red);
    double best[4] = {spread, spread, spread, spread};   // (a skipped group counts as +spread, and no group can give more)
    MsdfState state;
    msdf_begin(state);
    bool touched = false;   // (block-uniform: the group at hand has had an edge)
    hit_table_rounds(
        off, n_paths, lane, s_e0, s_e1,
        [&](int p, int e0, int e1) {
            s_info[lane] = path_info[p];
            return !(e1 > e0 && sdf_out_of_reach(gext + 4 * path_group[p], box, cull_spread));
        },
        [&](int, int j, int e0, int e1) {
            const int info = __builtin_amdgcn_readfirstlane(s_info[j]);
            if (e1 > e0) {
                touched = true;
                hit_chunk_walk<MSDF_EDGE_DOUBLES>(
                    edges, e0, e1, lane, s_e, [](double a0, double b0, double a1, double b1, double* pe) { msdf_edge_prepare(a0, b0, a1, b1, pe); },
                    [&](const double2* s) {
                        const double2 ab = s[0], xy = s[1], ia = s[2], br = s[3];
                        msdf_edge(state, info & 7, ab.x, ab.y, xy.x, xy.y, ia.x, ia.y, br.x, br.y, pa, pb);
                    });
            }
            if ((info & MSDF_PATH_LAST) && touched) {
                double v[4];
                msdf_finish(state, (info & MSDF_PATH_EVENODD) ? 1 : 0, (info & MSDF_PATH_NEGATIVE) ? -1 : 1, spread, fin, v);
                msdf_union(best, v);
                msdf_begin(state);
                touched = false;
            }
        });
    if (live) {
        const size_t at = 4 * (size_t)(id - id0);
        if constexpr (OUT == SDF_F64) {
            double2* dst = (double2*)((double*)out + at);
            dst[0] = make_double2(best[0], best[1]); dst[1] = make_double2(best[2], best[3]);
        } else if constexpr (OUT == SDF_F32) {
            *(float4*)((float*)out + at) = make_float4(sdf_encode_f32(best[0], spread), sdf_encode_f32(best[1], spread),
                                                       sdf_encode_f32(best[2], spread), sdf_encode_f32(best[3], spread));
        } else {
            *(uchar4*)((uint8_t*)out + at) = make_uchar4(sdf_encode_u8(best[0], spread), sdf_encode_u8(best[1], spread),
                                                         sdf_encode_u8(best[2], spread), sdf_encode_u8(best[3], spread));
        }
    }
}

// Plan only: exclusive prefix sums of the per-segment edge counts (seg_off[n] = their total).  One workgroup, a chunk of
// 1024 segments per step with the running total carried along: a plan-time pass over a few thousand to a few million ints.
__global__ __launch_bounds__(1024) void k_seg_scan(const int* __restrict__ seg_cnt, int n, int* __restrict__ seg_off) {
    // (eight consecutive counts per lane: a chunk is 8192 segments, a few barrier rounds for a drawing of tens of thousands --
    //  one count per lane was 23 rounds and 17.6 us for the bench scene's 22 703)
    constexpr int PER = 8;
    __shared__ int s_w[16];
    __shared__ int s_run;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) s_run = 0;
    __syncthreads();
    for (int c0 = 0; c0 < n; c0 += 1024 * PER) {
        const int i0 = c0 + tid * PER;
        int v[PER], mine = 0;
        if (i0 + PER <= n) {   // (the arrays are allocated in 256-byte blocks and i0 is a multiple of eight: two aligned 16-byte loads)
            const int4 a = ((const int4*)(seg_cnt + i0))[0], c = ((const int4*)(seg_cnt + i0))[1];
            v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = c.x; v[5] = c.y; v[6] = c.z; v[7] = c.w;
        } else {
#pragma unroll
            for (int k = 0; k < PER; ++k) v[k] = i0 + k < n ? seg_cnt[i0 + k] : 0;
        }
#pragma unroll
        for (int k = 0; k < PER; ++k) mine += v[k];
        int wtot;
        const int excl = wave_excl_scan(mine, lane, wtot);
        if (lane == 0) s_w[wave] = wtot;
        __syncthreads();
        const int run0 = s_run;
        int before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < 16; ++w) { before += w < wave ? s_w[w] : 0; all += s_w[w]; }
        int at = run0 + before + excl;
        int o[PER];
#pragma unroll
        for (int k = 0; k < PER; ++k) { o[k] = at; at += v[k]; }
        if (i0 + PER <= n) {
            ((int4*)(seg_off + i0))[0] = make_int4(o[0], o[1], o[2], o[3]);
            ((int4*)(seg_off + i0))[1] = make_int4(o[4], o[5], o[6], o[7]);
        } else {
#pragma unroll
            for (int k = 0; k < PER; ++k)
                if (i0 + k < n) seg_off[i0 + k] = o[k];
        }
        __syncthreads();
        if (tid == 0) s_run = run0 + all;
        __syncthreads();
    }
    if (tid == 0) seg_off[n] = s_run;
}

// Per-path binning record, written by k_path_bbox: the bands the (viewport-clipped) bbox covers and the path's
// first (path, band) pair.  One 16-byte load for the kernels that map an edge / a band to its pair.
struct PathBin {
    int b0, nb;   // first band, number of bands (0: empty path)
    int pb_off;   // pair index of (path, b0); pair of band b = pb_off + b - b0
    int cell_off; // first cell of the path: cell of (band b, column tile t) = cell_off + (b - b0) * nct + (t - ct0), with
                  // ct0 / nct the column tiles the bbox spans (path_ctiles)
};
// column tiles [ct0, ct0 + nct) that the layer columns [c0, c0 + cols) of a viewport starting at column vc0 span
__host__ __device__ __forceinline__ void path_ctiles(int c0, int cols, int vc0, int& ct0, int& nct) {
    span_ctiles(c0, cols, vc0, TC, ct0, nct);
}
static_assert(sizeof(PathBin) == 16, "PathBin is one dwordx4");

// One work item of k_path_build: the cells of path p in the bands [band0, band0 + nb) x its column tiles [k0, k0 + nk)
// (k relative to the path's first column tile).  A slab's counters and per-row sums live in LDS, so it holds at most
// PB_CELLS cells: a path of up to PB_CELLS column tiles is cut into runs of bands, a wider one band by band into runs of
// column tiles.
constexpr int PB_THREADS = 256;
constexpr int PB_CELLS = 80;
constexpr int PB_BANDS = 16;   // bands per slab at most: one TR-lane group of the workgroup scans each
static_assert(PB_BANDS * TR <= PB_THREADS && PB_BANDS <= PB_CELLS, "k_path_build: one lane group per band of the slab");
// It carries everything the workgroup needs of its path (bbox, bins, edge range): one load, then the edges -- looked up by
// the workgroup itself they were three dependent round trips in front of the first edge.
struct Slab {
    int p, band0, nb, k0;
    int nk, e_begin, e_end, pb_off;
    int r0, c0, rows, cols;       // the path's layer (clipped bbox)
    int b0, cell_off, pad[2];     // ... its first band, its first cell
};
static_assert(sizeof(Slab) == 64, "Slab is four dwordx4");
// how a path of nb bands x nct column tiles is cut: bands per slab, column-tile runs per band row
__host__ __device__ __forceinline__ void slab_shape(int nb, int nct, int& bands_per, int& col_runs) {
    if (nct <= PB_CELLS) {
        bands_per = PB_CELLS / nct < PB_BANDS ? PB_CELLS / nct : PB_BANDS;
        col_runs = 1;
    } else {
        bands_per = 1;
        col_runs = (nct + PB_CELLS - 1) / PB_CELLS;
    }
    (void)nb;
}

// bbox = {r0, c0, rows, cols}; viewport = same or has_vp = 0
// `stats`: fold the batch statistics (non-empty paths, path-pixels, union bbox) into BatchDev: only the plan reads them, and
// their six atomics per wave on shared addresses are most of this kernel's time when a render repeats the geometry
__global__ __launch_bounds__(64) void k_path_bbox(const unsigned long long* __restrict__ pkeys, int n_paths, int has_vp,
                                                  int vr0, int vc0, int vrows, int vcols, int* __restrict__ bbox,
                                                  PathBin* __restrict__ bins, BatchDev* __restrict__ bd, int stats,
                                                  const int* __restrict__ plist, Slab* __restrict__ slabs, int slab_cap, Owner own,
                                                  const int* __restrict__ path_seg0, const int* __restrict__ seg_off, int edge_cap,
                                                  const int* __restrict__ slab_at) {
    // (multi-GPU: thread i takes the i-th path of this rank's list, n_paths = its length; the others keep the empty bbox
    //  and bins the plan gave them)
    const int pi = blockIdx.x * blockDim.x + threadIdx.x, lane = threadIdx.x & 63;
    const int p = plist ? (pi < n_paths ? plist[pi] : 0x7fffffff) : pi;
    if (plist) n_paths = pi < n_paths ? 0x7fffffff : 0;  // (p < n_paths below = "this thread has a path")
    // (the path's edge range, for its slabs: asked for here, with the keys -- two dependent loads that used to follow the wave's
    //  reservations)
    int e_begin = 0, e_end = 0;
    if (slabs && p < n_paths) {
        e_begin = seg_off[path_seg0[p]]; e_end = seg_off[path_seg0[p + 1]];
    }
    // A planned render (`slab_at` given) makes no reservation: the path's pair and cell places are the ones the plan's own pass
    // left in `bins` -- same geometry, same bbox, same counts (a bbox that differs is an error) --, its slabs' places the plan's
    // heaviest-first order.  Asked for here, with the keys.
    const bool reuse = slab_at != nullptr;
    PathBin old_bin;
    old_bin.b0 = old_bin.nb = old_bin.pb_off = old_bin.cell_off = 0;
    int4 old_bb = make_int4(0, 0, 0, 0);
    if (reuse && p < n_paths) { old_bin = bins[p]; old_bb = ((const int4*)bbox)[p]; }
    int out[4] = {0, 0, 0, 0};
    int pb0 = 0, pnb = 0, pnct = 0;
    int st_n = 0;
    unsigned long long st_px = 0;
    unsigned st_minr = 0, st_minc = 0, st_maxr = 0, st_maxc = 0;
    PathBox pb = path_box(0ull, 0ull, 0ull, 0ull, has_vp, vr0, vc0, vrows, vcols, TR, TC);
    if (p < n_paths) {
        const unsigned long long* k = pkeys + 4 * (size_t)p;
        pb = path_box(k[0], k[1], k[2], k[3], has_vp, vr0, vc0, vrows, vcols, TR, TC);   // (svgr_core.h: the rule)
        if (pb.refused) atomicOr(&bd->err, 16);
        out[0] = pb.r0; out[1] = pb.c0; out[2] = pb.rows; out[3] = pb.cols;
        pb0 = pb.b0; pnb = pb.nb; pnct = pb.nct;
        if (pb.rows > 0 && pb.cols > 0) {
            st_n = 1;
            st_px = (unsigned long long)((long long)pb.rows * pb.cols);
            st_minr = (unsigned)(UNION_BIAS - pb.r0);
            st_minc = (unsigned)(UNION_BIAS - pb.c0);
            st_maxr = (unsigned)(UNION_BIAS + (pb.r0 + pb.rows));
            st_maxc = (unsigned)(UNION_BIAS + (pb.c0 + pb.cols));
        }
    }
    // A planned render whose geometry is not the plan's (a bbox or band count that differs: every setter voids the plan, so this is
    // a guard, not a path): the flag fails the render, and the path KEEPS THE PLAN'S bbox and places -- its slabs, pairs and cells
    // stay inside what the plan reserved, whatever the later kernels make of its edges (they clip to the layer they are given).
    if (reuse && p < n_paths && !path_box_is(pb, old_bb.x, old_bb.y, old_bb.z, old_bb.w, old_bin.nb)) {
        atomicOr(&bd->err, 32);
        out[0] = old_bb.x; out[1] = old_bb.y; out[2] = old_bb.z; out[3] = old_bb.w;
        pb0 = old_bin.b0; pnb = old_bin.nb; pnct = 0;
        if (pnb > 0 && out[2] > 0 && out[3] > 0) {
            int ct0_;
            path_ctiles(out[1], out[3], vc0, ct0_, pnct);
        } else {
            pnb = 0;
        }
        st_n = 0;
    }
    // (a path of 2^24 x 2^24 pixels has 2^38 cells: such a batch overflows the cursor and is refused, err bit 5)
    const long long want_cells = has_vp ? (long long)pnb * pnct : 0ll;  // (no viewport yet: the pass only finds the union)
    if (want_cells > (1ll << 28)) atomicOr(&bd->err, 32);
    // the path's slabs (band runs without a band of this rank are left out)
    int bands_per = 1, col_runs = 1, n_slabs = 0;
    if (has_vp && pnb > 0 && want_cells <= (1ll << 28)) {
        slab_shape(pnb, pnct, bands_per, col_runs);
        for (int bb = 0; bb < pnb; bb += bands_per) {
            const int be = bb + bands_per < pnb ? bb + bands_per : pnb;
            if (owns_any(own, pb0 + bb, pb0 + be - 1)) n_slabs += col_runs;
        }
    }
    // the wave's reservations of pair, cell and slab slots: three returning atomics issued TOGETHER (one round trip, not three
    // in a row: this kernel is one wave per 64 paths and nothing but latency)
    int off, cell_off, slab0;
    {
        const int n_cells_ = want_cells > (1ll << 28) ? 0 : (int)want_cells;
        int t_pb, t_cell, t_slab;
        const int e_pb = wave_excl_scan(pnb, lane, t_pb), e_cell = wave_excl_scan(n_cells_, lane, t_cell),
                  e_slab = wave_excl_scan(n_slabs, lane, t_slab);
        if (!reuse) {
            int b_pb = 0, b_cell = 0, b_slab = 0;
            if (lane == 0) {
                if (t_pb > 0) b_pb = atomicAdd(&bd->pb_cursor, t_pb);
                if (t_cell > 0) b_cell = atomicAdd(&bd->cell_cursor, t_cell);
                if (t_slab > 0) b_slab = atomicAdd(&bd->slab_cursor, t_slab);
            }
            off = __shfl(b_pb, 0) + e_pb;
            cell_off = __shfl(b_cell, 0) + e_cell;
            slab0 = __shfl(b_slab, 0) + e_slab;
        } else {
            // (svgr_batch::slab_at: workgroups are dispatched in slab order, and a launch that ends on its longest slabs ends late)
            off = old_bin.pb_off;
            cell_off = old_bin.cell_off;
            slab0 = p < n_paths ? slab_at[p] : 0;
            if (pi == 0) bd->slab_cursor = slab_cap;  // (k_path_build's grid: the plan's count)
        }
    }
    if (stats)
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {  // statistics: fold the wave, then one set of atomics
        st_n += __shfl_xor(st_n, d);
        st_px += __shfl_xor(st_px, d);
        unsigned a = __shfl_xor(st_minr, d), b = __shfl_xor(st_minc, d), c = __shfl_xor(st_maxr, d), e = __shfl_xor(st_maxc, d);
        st_minr = a > st_minr ? a : st_minr; st_minc = b > st_minc ? b : st_minc;
        st_maxr = c > st_maxr ? c : st_maxr; st_maxc = e > st_maxc ? e : st_maxc;
    }
    if (stats && lane == 0 && st_n > 0) {
        atomicAdd(&bd->n_nonempty, st_n);
        atomicAdd(&bd->path_pixels, st_px);
        atomicMax(&bd->umin_r, st_minr);
        atomicMax(&bd->umin_c, st_minc);
        atomicMax(&bd->umax_r, st_maxr);
        atomicMax(&bd->umax_c, st_maxc);
    }
    // One GPU (every band owned): the wave's slabs are dealt to its lanes one each -- slab i belongs to the lane whose run of slabs
    // it falls into -- instead of every lane writing its own path's one after the other (a large path is dozens of slabs: the
    // tiger @ 2048 spent 10 us here for 182 paths).
    const bool coop = slabs != nullptr && own.world <= 1;
    if (coop) {
        const bool fits = n_slabs > 0 && slab0 + n_slabs <= slab_cap;
        int t_sl;
        const int e_sl = wave_excl_scan(fits ? n_slabs : 0, lane, t_sl);
        const int eb = e_begin < edge_cap ? e_begin : edge_cap, ee = e_end < edge_cap ? e_end : edge_cap;
        for (int base = 0; base < t_sl; base += 64) {
            const int i = base + lane;
            int owner = 0;   // the last lane whose first slab is <= i (a lane without slabs shares its first slab with its successor)
#pragma unroll
            for (int step = 32; step >= 1; step >>= 1) {
                const int cand = owner + step;
                const int first = __shfl(e_sl, cand & 63);
                if (cand < 64 && first <= i) owner = cand;
            }
            const int o_first = __shfl(e_sl, owner), o_slab0 = __shfl(slab0, owner), o_p = __shfl(p, owner);
            const int o_pb0 = __shfl(pb0, owner), o_pnb = __shfl(pnb, owner), o_pnct = __shfl(pnct, owner);
            const int o_bper = __shfl(bands_per, owner), o_cruns = __shfl(col_runs, owner);
            const int o_eb = __shfl(eb, owner), o_ee = __shfl(ee, owner), o_off = __shfl(off, owner), o_cell = __shfl(cell_off, owner);
            const int o_r0 = __shfl(out[0], owner), o_c0 = __shfl(out[1], owner), o_rows = __shfl(out[2], owner), o_cols = __shfl(out[3], owner);
            if (i < t_sl) {
                const int j = i - o_first;
                const int br = o_cruns == 1 ? j : j / o_cruns, c = o_cruns == 1 ? 0 : j - br * o_cruns;
                const int bb = br * o_bper, be = bb + o_bper < o_pnb ? bb + o_bper : o_pnb;
                Slab sl;
                sl.p = o_p; sl.band0 = o_pb0 + bb; sl.nb = be - bb;
                sl.k0 = c * PB_CELLS; sl.nk = o_pnct - sl.k0 < PB_CELLS ? o_pnct - sl.k0 : PB_CELLS;
                sl.e_begin = o_eb; sl.e_end = o_ee; sl.pb_off = o_off;
                sl.r0 = o_r0; sl.c0 = o_c0; sl.rows = o_rows; sl.cols = o_cols;
                sl.b0 = o_pb0; sl.cell_off = o_cell;
                sl.pad[0] = sl.pad[1] = 0;
                slabs[o_slab0 + j] = sl;
            }
        }
    }
    if (slabs && n_slabs > 0 && !(coop && slab0 + n_slabs <= slab_cap)) {
        if (slab0 + n_slabs > slab_cap) {
            // (the launch covers the capacity: what this path would have filled of it must not be followed)
            atomicOr(&bd->err, 4);
            for (int at = slab0; at < slab_cap; ++at) {
                Slab sl;
                memset(&sl, 0, sizeof sl);
                slabs[at] = sl;
            }
        } else {
            int at = slab0;
            // the path's edges (k_flatten); a pass whose edge array was too small (flagged there) must not be read beyond it
            e_begin = e_begin < edge_cap ? e_begin : edge_cap;
            e_end = e_end < edge_cap ? e_end : edge_cap;
            for (int bb = 0; bb < pnb; bb += bands_per) {
                const int be = bb + bands_per < pnb ? bb + bands_per : pnb;
                if (!owns_any(own, pb0 + bb, pb0 + be - 1)) continue;
                for (int c = 0; c < col_runs; ++c) {
                    Slab sl;
                    sl.p = p; sl.band0 = pb0 + bb; sl.nb = be - bb;
                    sl.k0 = c * PB_CELLS; sl.nk = pnct - sl.k0 < PB_CELLS ? pnct - sl.k0 : PB_CELLS;
                    sl.e_begin = e_begin; sl.e_end = e_end; sl.pb_off = off;
                    sl.r0 = out[0]; sl.c0 = out[1]; sl.rows = out[2]; sl.cols = out[3];
                    sl.b0 = pb0; sl.cell_off = cell_off;
                    sl.pad[0] = sl.pad[1] = 0;
                    slabs[at++] = sl;
                }
            }
        }
    }
    if (p < n_paths) {
        ((int4*)bbox)[p] = make_int4(out[0], out[1], out[2], out[3]);
        PathBin pbin;
        pbin.b0 = pb0; pbin.nb = pnb; pbin.pb_off = off; pbin.cell_off = cell_off;
        bins[p] = pbin;
    }
}

// rows of an edge inside band `band` (layer-local [ya, yb))
__device__ __forceinline__ void band_rows(const EdgeSetup& es, int band, int vr0, int r0, int& ya, int& yb) {
    const int b0row = band * TR + vr0 - r0;
    ya = es.y_begin > b0row ? es.y_begin : b0row;
    yb = es.y_end < b0row + TR ? es.y_end : b0row + TR;
}

// One band-list entry: a (path, band) pair.  k_pair_scan reads it whole; k_tile_lists only the first 16 bytes.
struct TileEntry {
    int c0, cols;     // layer columns
    int cell0;        // cell of (pair, first column tile of the path): the cell of column tile t is cell0 + t - ct0
    int p;            // path id
    int r0, rows;     // layer rows
    int pad[2];
};
static_assert(sizeof(TileEntry) == 32, "TileEntry is 32 bytes");

// One workgroup per owned band, after k_path_bbox: the ascending (= paint order) list of the paths whose bbox reaches the
// band (TileEntry), and the band's first tile-list slot (one slot per cell of a listed pair: k_tile_lists fills them).
// A pair's place in its band's list is the bit that stands for it in the tiles' entry bitmasks.
constexpr int BE_BLOCK = 1024;
constexpr int BE_KEEP = 4;   // 64-path groups per wave whose bins stay in registers between the two passes
__global__ __launch_bounds__(BE_BLOCK) void k_band_entries(const PathBin* __restrict__ bins, int n_paths,
                                                              const int* __restrict__ plist,  // multi-GPU: the n_paths paths of this rank, ascending (else nullptr: all)
                                                              const int* __restrict__ bbox,
                                                              int* __restrict__ band_start, int* __restrict__ band_count,
                                                              int* __restrict__ band_item0,
                                                              TileEntry* __restrict__ entries, int* __restrict__ pair_idx,
                                                              int entry_cap, int item_cap, int vc0,
                                                              BatchDev* __restrict__ bd, Owner own, int reuse,
                                                              unsigned long long* __restrict__ clear_mask, int mask_span) {
    constexpr int NWV = BE_BLOCK / 64;
    __shared__ int s_n[NWV], s_c[NWV];
    __shared__ int s_ent0, s_ok;
    const int band = owned_band_at(own, blockIdx.x), tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    // (a first pass over fresh memory: the band's entry bitmasks cleared here, in front of k_path_build, instead of by a memset launch)
    if (clear_mask)
        for (int i = tid; i < mask_span; i += BE_BLOCK) clear_mask[(size_t)band * mask_span + i] = 0ull;
    // `reuse` (a planned render): the band's places in the entry and item arrays are the ones the plan's own pass left in
    // band_start / band_item0 -- same geometry, same counts.  Asked for here, with the bins; the 256 bands' returning atomics on
    // two cursors were a quarter of this kernel (a hot address serves ~90 of them per microsecond).
    int pre_e0 = 0, pre_i0 = 0, pre_tn = -1;
    if (reuse && tid == 0) { pre_e0 = band_start[band]; pre_tn = band_count[band]; pre_i0 = band_item0[band]; }
    // Wave w owns the consecutive paths [w * chunk, (w + 1) * chunk), as `groups` groups of 64: lane l of group g has
    // path w * chunk + g * 64 + l, so every load is coalesced and list order = (wave, group, lane).
    const int groups = (n_paths + BE_BLOCK - 1) / BE_BLOCK, chunk = groups * 64;
    const int p_wave = wave * chunk;
    auto path_at = [&](int idx) { return plist ? plist[idx < n_paths ? idx : 0] : idx; };  // (n_paths = length of the list, if any)
    auto ctiles_of = [&](const int4 bb) { int ct0, nct; path_ctiles(bb.y, bb.w, vc0, ct0, nct); return nct; };
    bool kmem[BE_KEEP];
    PathBin kb[BE_KEEP];
    int4 kbb[BE_KEEP];
    int my_n = 0, my_c = 0;  // this lane's entries / cells, over all its groups
    {
        // the first BE_KEEP groups with every load in flight together
#pragma unroll
        for (int g = 0; g < BE_KEEP; ++g) {
            const int p = p_wave + g * 64 + lane;
            const int pa = g < groups && p < n_paths ? path_at(p) : 0;
            kb[g] = bins[pa];
            kbb[g] = ((const int4*)bbox)[pa];
        }
#pragma unroll
        for (int g = 0; g < BE_KEEP; ++g) {
            const int p = p_wave + g * 64 + lane;
            kmem[g] = g < groups && p < n_paths && kb[g].nb > 0 && band >= kb[g].b0 && band < kb[g].b0 + kb[g].nb;
            if (kmem[g]) { ++my_n; my_c += ctiles_of(kbb[g]); }
        }
    }
    // (more than BE_KEEP * 1024 paths: the rest four groups at a time, again with the loads in flight together)
    auto load4 = [&](int g0, PathBin* tb, int4* tbb, bool* mem) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int p = p_wave + (g0 + j) * 64 + lane;
            const int pa = g0 + j < groups && p < n_paths ? path_at(p) : 0;
            tb[j] = bins[pa];
            tbb[j] = ((const int4*)bbox)[pa];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int p = p_wave + (g0 + j) * 64 + lane;
            mem[j] = g0 + j < groups && p < n_paths && tb[j].nb > 0 && band >= tb[j].b0 && band < tb[j].b0 + tb[j].nb;
        }
    };
    for (int g0 = BE_KEEP; g0 < groups; g0 += 4) {
        PathBin tb[4];
        int4 tbb[4];
        bool mem[4];
        load4(g0, tb, tbb, mem);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (mem[j]) { ++my_n; my_c += ctiles_of(tbb[j]); }
    }
    int wn = my_n, wc = my_c;  // wave totals
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { wn += __shfl_xor(wn, d); wc += __shfl_xor(wc, d); }
    if (lane == 0) { s_n[wave] = wn; s_c[wave] = wc; }
    __syncthreads();
    if (wave == 0) {  // exclusive scan of the wave totals by one wave, then the band's reservations
        const int a = lane < NWV ? s_n[lane] : 0, cc = lane < NWV ? s_c[lane] : 0;
        int tn, tcc;
        const int ea = wave_excl_scan(a, lane, tn);
        (void)wave_excl_scan(cc, lane, tcc);
        if (lane < NWV) s_n[lane] = ea;
        if (lane == 0) {
            int e0, i0, ok = 1;
            if (reuse) {
                e0 = pre_e0; i0 = pre_i0;
                if (pre_tn != tn) { atomicOr(&bd->err, 4); ok = 0; tn = 0; }  // (not the plan's count: its places do not hold)
            } else {
                e0 = tn ? atomicAdd(&bd->entry_cursor, tn) : 0;
                i0 = tcc ? atomicAdd(&bd->item_cursor, tcc) : 0;
            }
            if (ok && e0 + tn > entry_cap) { atomicOr(&bd->err, 4); ok = 0; tn = 0; }
            if (ok && (long long)i0 + tcc > (long long)item_cap) { atomicOr(&bd->err, 64); ok = 0; tn = 0; }
            if (tn && !reuse) atomicMax(&bd->max_band_entries, tn);
            s_ent0 = e0; s_ok = ok;
            band_start[band] = e0;
            band_count[band] = tn;
            band_item0[band] = i0;
        }
    }
    __syncthreads();
    if (!s_ok) return;
    int ent = s_ent0 + s_n[wave];  // running base of the wave, advanced group by group
    auto place = [&](bool m) {  // all lanes of the wave, one group: this lane's entry
        int tn;
        const int my_ent = ent + wave_excl_scan(m ? 1 : 0, lane, tn);
        ent += tn;
        return my_ent;
    };
    auto store = [&](int p, int my_ent, const int4 bb, const PathBin pbin) {
        TileEntry e;
        e.p = p; e.c0 = bb.y; e.cols = bb.w; e.r0 = bb.x; e.rows = bb.z;
        e.pad[0] = e.pad[1] = 0;
        int ct0, nct;
        path_ctiles(bb.y, bb.w, vc0, ct0, nct);
        e.cell0 = pbin.cell_off + (band - pbin.b0) * nct;
        entries[my_ent] = e;
        pair_idx[pbin.pb_off + band - pbin.b0] = my_ent - s_ent0;  // the pair's place in its band's list
    };
#pragma unroll
    for (int g = 0; g < BE_KEEP; ++g) {
        if (g >= groups) break;
        const int me = place(kmem[g]);
        if (kmem[g]) store(path_at(p_wave + g * 64 + lane), me, kbb[g], kb[g]);
    }
    for (int g0 = BE_KEEP; g0 < groups; g0 += 4) {
        PathBin tb[4];
        int4 tbb[4];
        bool mem[4];
        load4(g0, tb, tbb, mem);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            int me = 0;
            if (g0 + j < groups) me = place(mem[j]);  // (whole groups only: every lane of the wave scans)
            if (mem[j]) store(path_at(p_wave + (g0 + j) * 64 + lane), me, tbb[j], tb[j]);
        }
    }
}

// Sum of the pieces of one edge-row record (apply_record's list: x0i, x0i+1, the middle run, x0i+n-1, x0i+n) whose
// column -- clamped to 0 from the left like S:2262 -- lies in [ca, cb).  The middle run is counted, not walked.
__device__ __forceinline__ double record_sum_range(int x0i, int n, const double* v, int ca, int cb) {
    auto in = [&](int xi) { const int c = xi > 0 ? xi : 0; return c >= ca && c < cb; };
    double sum = 0.0;
    if (in(x0i)) sum = v[0];
    if (in(x0i + 1)) sum = sum + v[1];
    if (n >= 3) {
        // xi in [x0i + 2, x0i + n - 2]; negative xi sit in column 0
        const int lo = ca > 0 ? (x0i + 2 > ca ? x0i + 2 : ca) : x0i + 2;
        const int hi = x0i + n - 2 < cb - 1 ? x0i + n - 2 : cb - 1;
        if (hi >= lo) sum = sum + (double)(hi - lo + 1) * v[2];
        if (in(x0i + n - 1)) sum = sum + v[3];
    }
    if (n >= 2 && in(x0i + n)) sum = sum + v[4];
    return sum;
}

// The same pieces as the ADDS a tile makes for them: `single(c, v)` for a piece at layer column c, `run(c, len, v)` for
// len consecutive columns with the same value.  [ca, cb) are the layer columns of the cell (0 <= ca, cb <= layer width:
// what lies right of the layer is dropped, S:2260); pieces left of the layer fold into column 0 (S:2262), the part of the
// middle run that does as ONE add of neg * v[2].  Used twice by k_pair_cells with the same arguments: to count, then to write.
template <class Single, class Run>
__device__ __forceinline__ void record_adds(int x0i, int n, const double* v, int ca, int cb, Single&& single, Run&& run) {
    auto one = [&](int xi, double val) {
        const int c = xi > 0 ? xi : 0;
        if (c >= ca && c < cb) single(c, val);
    };
    one(x0i, v[0]);
    one(x0i + 1, v[1]);
    if (n >= 3) {
        const int xa = x0i + 2, xb = x0i + n - 2;  // the middle run, inclusive
        if (xa < 0 && ca == 0) {
            const int neg = (xb < -1 ? xb : -1) - xa + 1;
            if (neg > 0) single(0, (double)neg * v[2]);
        }
        int lo = xa > 0 ? xa : 0;
        lo = lo > ca ? lo : ca;
        const int hi = xb < cb - 1 ? xb : cb - 1;
        if (hi >= lo) run(lo, hi - lo + 1, v[2]);
        one(x0i + n - 1, v[3]);
    }
    if (n >= 2) one(x0i + n, v[4]);
}

// is the coverage of a constant running sum visible (S:984-990) ?
__device__ __forceinline__ bool carry_visible(double c, int rule) {
    return (rule ? fill_evenodd_raw(c) : fabs(c)) >= kZeroCut;
}

// offset of tile column `tcol` (>= 0) inside a padded delta row: every chunk of PX columns is followed by
// CHUNK_STRIDE - PX pad doubles, i.e. (tcol / PX) * CHUNK_STRIDE + tcol % PX without the multiply
__device__ __forceinline__ int lds_col(int tcol) {
    static_assert((PX & (PX - 1)) == 0, "PX is a power of two");
    return tcol + (int)((unsigned)tcol / PX) * (CHUNK_STRIDE - PX);
}
__device__ __forceinline__ int lds_index(int trow, int tcol) {
    return __mul24(trow, ROW_STRIDE) + lds_col(tcol);
}
// A run of equal adds is cut at the borders of the PX-column chunks of a tile row: how many pieces `len` columns from tile column
// `tcol` make.  (The tile kernel's lanes walk a run one column at a time while the rest of the wave waits: a shallow edge's
// run of 60 columns held its wave for 60 rounds.  Cut to a chunk a run is at most PX columns, its pieces go to different
// lanes -- an item's add list rarely fills the workgroup -- and a piece never steps over the padding behind a chunk.)
__device__ __forceinline__ int run_pieces(int tcol, int len) {
    return ((tcol + len - 1) / PX) - (tcol / PX) + 1;
}
// TileAdd::where of `len` adds starting at (tile row, tile column)
__device__ __forceinline__ unsigned add_where(int trow, int tcol, int len) {
    return (unsigned)(lds_index(trow, tcol) * 8) | ((unsigned)(len - 1) << 16) | ((unsigned)(tcol & (PX - 1)) << 22);
}

// ---------------------------------------------------------------------------------------------
// edges of a path -> the cells of the path: classes, carry-ins, headers, add lists.
// One workgroup per SLAB of a path's cells (k_path_bbox cuts them: at most PB_CELLS cells, PB_BANDS bands).  The edges of a
// path are one contiguous range of the edge array (k_flatten), so the workgroup walks exactly the geometry that can reach its
// cells, and everything it accumulates -- per cell the number of adds, per cell and tile row the sum of the pieces, which tile
// rows have a piece at all -- lives in LDS.
//
// A cell's add list is [the pieces of every edge row that reaches the cell][one carry-in add per tile row that has a piece
// anywhere LEFT of the cell, at the layer's first column in the tile][the layer-edge sentinels: NaN behind the layer's last
// column, see k_tile_render].  Every one of the three counts follows from the geometry's integers alone (which columns an edge
// row's pieces fall into), not from a rounded sum: the list of a cell has the same length and the same place in every pass
// over unchanged geometry, whatever order the LDS atomics ran in.  (Round 4 asked `carry != 0.0`: a sum that cancels in one
// order and leaves 1e-17 in another made the lists' sizes wobble, and their places had to be reserved again in every render.)
//
// PLANNED = false (the plan's passes, and renders of a batch whose plan left no add places):
//   pass A   per edge row of the slab (S:2244-2303) and column tile its pieces fall into: how many adds they make there, and
//            their sum (ds_add into the cell's counter and the cell's sum of that tile row)
//   walk     TR lanes per band of the slab walk its cells left to right with the running sum = the carry-in of every tile
//            row (np.cumsum entering the tile, S:983): class of every cell, size of its add list; ONE reservation of add slots
//            per slab (a global atomic in the path's shard)
//   write    headers, carry-in adds, sentinels, entry-bitmask bits; per cell {first add, pieces} into `cell_plan`
//   pass B   the rows again: the pieces as adds (`adds` == nullptr, the plan's measuring run: no pass B, nothing written to
//            the lists)
// PLANNED = true (every render of a planned batch): the cells' places are the ones the plan's own full pass left in
// `cell_plan` -- same geometry, same counts.  A row's pieces are computed ONCE: pass A adds the counts and sums AND stores the
// adds at `first add + ds_add_rtn(cell counter)`; the walk only produces carry-ins, classes and headers and CHECKS every
// cell's count against the plan's (a mismatch is the sticky error bit 32, as in k_path_bbox; an add that would land beyond
// the cell's planned pieces is not written).  No pass B, no global atomic.
//
// The rows are dealt to the lanes as RUNS of consecutive (edge, row) tasks, not edge by edge (a lane per edge runs as long as
// the longest edge of its wave: a synthetic blob has mean 3 rows, longest 49; real drawings hundreds next to two) and not row
// by row either (a lane that starts in the middle of an edge replays the reference's x recurrence, S:2244-2248, from the
// edge's first row: per task that was a tenth of the kernel): a lane reads its first task's edge from `s_start` (written by the
// staged edge whose rows hold that task), replays to its row once, and from there on takes ONE row_step per task,
// moving to the next staged edge when the edge's rows end.  Staged edges are compacted -- only those with a row inside the
// slab are kept -- so "the next edge" is the next slot.
// ---------------------------------------------------------------------------------------------
struct EdgeLds {
    double p0y, p1y, dxdy, x;  // as EdgeSetup; x = column at which the edge enters row ya
};
// x after the `n` rows y, y + 1, ... of the reference's recurrence (S:2244-2248), none of them the edge's last row: the column at
// which the edge enters row y + n.  Only the first of them can be a partial row (the edge's first row: ylo = p0y); in every
// later one dy = (y + 1) - y = 1.0 exactly, dxdy * 1.0 is dxdy, and row_step's `x + dxdy * dy` is `x + dxdy` bit for bit -- one
// addition per replayed row instead of the whole step.
__device__ __forceinline__ double replay_rows(double x, int y, int n, double p0y, double p1y, double dxdy) {
    if (n <= 0) return x;
    RowState st;
    st.x_next = x; st.x = x; st.d = 0.0;
    row_step(st, y, p0y, p1y, dxdy, 1.0);
    double xn = st.x_next;
    for (int k = 1; k < n; ++k) xn = xn + dxdy;
    return xn;
}
static_assert(sizeof(EdgeLds) == 32, "EdgeLds is two 16-byte LDS reads (its first row and direction ride in an int array beside it)");
constexpr int PB_BATCH = 256;            // edges staged together
constexpr int PB_EPL = (PB_BATCH + PB_THREADS - 1) / PB_THREADS;   // edges per lane and batch
static_assert(PB_BATCH % 64 == 0 && PB_BATCH / 16 <= 32, "two-level search: at most 32 coarse entries, read four at a time");
static_assert(PB_BANDS * TR * PB_BATCH < (1 << 20) && PB_BATCH < (1 << 11), "stage() scans row counts and live flags in one packed word");
constexpr int PB_WAVES = 6;
// The barriers of k_path_build order LDS traffic only -- nothing one wave writes to global memory is read by another inside the
// kernel --, so they wait for the wave's LDS operations and not, as __syncthreads() does, for its global stores as well: behind
// pass A those are the add lists on their way out, and a wave that waits for their acknowledgement stands still for a microsecond.
__device__ __forceinline__ void pb_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
// MODE 0: the exact two-pass form (PLANNED = false above).  MODE 1: a planned render (PLANNED = true above).
// MODE 2 (BOUNDED, round 6): ONE pass over the edge rows WITHOUT a plan -- the pass of a re-plan or of a first plan, which used to be
// MODE 0.  While a batch of edges is staged every edge adds, to each cell it can reach, an UPPER BOUND of the adds it can leave there
// (rows in the band x the most pieces one of its rows can put into one tile); a cell's place is the prefix sum of the bounds (plus
// room for its carry-ins and sentinels), the slab reserves that much in ONE atomic, and from there on the pass is MODE 1's: pieces
// stored as they are computed, the walk writes the cells (and `cell_plan`: the planned renders that follow take these places).  The
// lists keep the slack between them (memory, not traffic: only what is written is read).  A bound that did not hold is caught like
// a plan that does not fit: the pieces are not stored, error bit 32, the staged plan (MODE 0, exact) takes over.
// LEAN (with MODE 1): the placed pass of a replay that keeps its slab table behind the lean flatten (run_geometry), on one GPU, not
// deterministic, without groups or gradients.  What such a pass is given for its options -- one rank, `det` and `stats` 0, no keys
// to guard, no group or gradient table, no stamps -- is known when the kernel is compiled: no owns_band test, no guard block, no
// option lives in a register through the row loop.  Everything that keeps a wrong plan harmless is the full form's.
// The lean form also WRITES only what a replay can change.  A cell with pieces is class 2 by the geometry's integers, and of such a
// cell it stores the pieces and the carry-in adds (their values move with the order of the LDS atomics) but neither the header (80
// bytes that repeat from pass to pass under one set of paints), nor the sentinels (`{where, NaN}` at places that are counts), nor the
// two mask bits (k_tile_lists is told so -- `kept` == 2 -- and expects the saved class >= 1 row without the saved class-2 row).  The
// count check, the `add0 < 0` refusal and the `cell_cap` / `mask_ok` tests stay in front of all of it; class-1 cells are written as
// ever.  The host launches it only where the last pass that wrote `cell_hdr` and `adds` was a placed pass of this plan over every
// band, without groups or gradients, into the same blocks, with the paints that stand now (PlanState::cells), and where
// k_tile_lists keeps its lists.
template <int MODE, bool LEAN = false>
__global__ __launch_bounds__(PB_THREADS, PB_WAVES) void k_path_build(const Slab* __restrict__ slabs, const double* __restrict__ edges,
                                                           const int* __restrict__ pair_idx, const double* __restrict__ path_paint,
                                                           const uint8_t* __restrict__ path_rule, const int* __restrict__ path_group,
                                                           const int* __restrict__ path_grad, int vr0, int vc0, int n_ct, int mask_words,
                                                           unsigned long long* __restrict__ tile_mask, CellHdr* __restrict__ cell_hdr,
                                                           int cell_cap, const AddShards ash, TileAdd* __restrict__ adds,
                                                           int2* __restrict__ cell_plan, BatchDev* __restrict__ bd, Owner own, int stats, int det,
                                                           unsigned long long* __restrict__ dbg,
                                                           const unsigned long long* __restrict__ guard_keys, const int* __restrict__ guard_bbox,
                                                           const PathBin* __restrict__ guard_bins, int n_paths, int vrows, int vcols) {
#ifdef SVGR_DBG_PB_STAMP
#define PB_STAMP(i) do { if (threadIdx.x == 0 && dbg && blockIdx.x < 8192) dbg[8 * blockIdx.x + (i)] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define PB_STAMP(i) do { } while (0)
#endif
    constexpr bool PLANNED = MODE != 0;     // the cells' places are known BEFORE the rows' pieces are computed: one pass, the walk writes the cells
    constexpr bool BOUNDED = MODE == 2;     // ... known from bounds this workgroup makes itself, not from a plan
    static_assert(!LEAN || MODE == 1, "the lean form is a placed pass");
    if constexpr (LEAN) {   // (the values run_geometry would pass: constants from here on)
        own.world = 1; det = 0; stats = 0;
        path_group = nullptr; path_grad = nullptr; dbg = nullptr; guard_keys = nullptr;
    }
    PB_STAMP(0);
    __shared__ __attribute__((aligned(16))) double s_sum[PB_CELLS * TR];
    __shared__ double s_left[TR];
    __shared__ int s_cnt[PB_CELLS], s_pos[PB_CELLS], s_plan_n[PB_CELLS];
    __shared__ unsigned s_rowb[PB_CELLS + 1];                       // per cell: tile rows with a piece ([PB_CELLS]: left of the slab)
    __shared__ __attribute__((aligned(16))) EdgeLds s_edge[PB_BATCH];
    __shared__ int s_eya[PB_BATCH];              // per staged edge: ya | (dir < 0) << 31
    __shared__ __attribute__((aligned(16))) int s_pref[PB_BATCH + 4];
    __shared__ unsigned short s_start[PB_THREADS];   // per lane: the staged edge that holds the first task of its run
    __shared__ int s_wtot[PB_EPL][PB_THREADS / 64];
    __shared__ __attribute__((aligned(8))) int2 s_info[PB_CELLS];   // per cell: adds in front of it in its band, class
    __shared__ unsigned s_rowm[PB_CELLS];                           // ... rows with a carry-in add | rows with a sentinel << 16
    __shared__ int s_ptot[PB_BANDS], s_pidx[PB_BANDS], s_base, s_ok;
    __shared__ int s_rl;                                            // (LEAN) the path's rule byte, parked like the pairs' places
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // (the LDS tables are cleared whole, not just the slab's part of them: that needs nothing of the slab, so it runs while the
    //  slab record is on its way)
    for (int i = tid; i < PB_CELLS * TR / 2; i += PB_THREADS) ((double2*)s_sum)[i] = make_double2(0.0, 0.0);
    for (int i = tid; i < PB_CELLS; i += PB_THREADS) {
        s_cnt[i] = 0; s_pos[i] = (int)0x80000000; s_plan_n[i] = 0; s_rowb[i] = 0u;
        if (!LEAN) s_info[i] = make_int2(0, 0);   // (a planned pass never reads it)
    }
    if (tid < TR) s_left[tid] = 0.0;
    if (tid == 0) s_rowb[PB_CELLS] = 0u;
    if (LEAN && tid < PB_BANDS) s_pidx[tid] = 0;
    if (LEAN && tid == 0) s_rl = 0;
    // (both scalar loads asked for together: the slab first, the test of the cursor behind it -- the grid never exceeds the list)
    const Slab sl = slabs[blockIdx.x];
    // `guard_keys` given (MODE 1 only): a replay that KEEPS the slab table, bboxes and bins the previous render of the same plan left
    // -- k_path_bbox did not run, `bd->slab_cursor` is not written: the grid is the table.  What k_path_bbox checked of such a render
    // (the paths' keys still give the plan's bboxes: error bit 32 otherwise, the plan's places kept) is checked below, between pass A
    // and the walk, every path once -- with or without slabs of its own --: a lane per path, by the first wave of one workgroup per
    // 64 paths (as many waves as k_path_bbox was; a check per workgroup was 5 % of this kernel's vector instructions).
    // (the lean form is launched on a kept table only, behind the lean flatten, which leaves no key to check)
    const bool guarding = MODE == 1 && guard_keys != nullptr;
    const int n_slabs_now = LEAN || guarding ? (int)gridDim.x : bd->slab_cursor;
    if ((int)blockIdx.x >= n_slabs_now) return;  // (the grid covers the plan's slab capacity)
    // (a slot of a path that did not fit the slab list: flagged by k_path_bbox -- when the table was written, if it is a kept one: the
    //  error word is sticky)
    if (sl.nb <= 0 || sl.nk <= 0) return;
    PB_STAMP(7);
    const int p = sl.p;
    const int r0 = sl.r0, c0 = sl.c0, rows = sl.rows, cols = sl.cols;
    int ct0, nct;
    path_ctiles(c0, cols, vc0, ct0, nct);
    const int x_first = vc0 + ct0 * TC - c0;  // layer column at which the path's first column tile starts (<= 0)
    const int e_begin = sl.e_begin, e_end = sl.e_end;
    const int sr0 = vr0 + sl.band0 * TR - r0, sr1 = sr0 + sl.nb * TR;  // layer rows of the slab
    const int n_cell = sl.nb * sl.nk;
    const double o_r = (double)r0, o_c = (double)c0;  // `lines - [min_x, min_y]` (S:979)
    // (what the later phases need of the path -- scalar loads: asked for here, not behind a barrier each)
    // (a byte load lands in a vector register: in the lean form it does not live through the row loop either)
    int rl = path_rule[p], rule = rl & 1;
    const int group = path_group ? path_group[p] : -1;
    const int grad1 = path_grad ? path_grad[p] + 1 : 0;  // gradient index + 1 (0: solid colour)
    const double4 paint = ((const double4*)path_paint)[p];
    // global index of the slab's cell i (band-major inside the slab)
    auto cell_of = [&](int g, int k) { return sl.cell_off + (sl.band0 + g - sl.b0) * nct + sl.k0 + k; };
    // PLANNED: the cells' places {first add, pieces}, asked for here -- in front of the edges, so they have landed when the
    // edges have -- and put into LDS by the first stage()
    int s_per = 0;   // tasks per lane of the staged batch (stage -> for_rows)
    int2 my_plan = make_int2((int)0x80000000, 0);
    bool plan_pending = false;
    // (the place of the (path, band) pair of this lane's band in its band's list -- what the walk's lane 0 of every band sets
    //  the entry-bitmask bits with: asked for here, a global load that has long landed when the walk starts)
    int my_pidx = 0;
    if ((tid & (TR - 1)) == 0 && tid / TR < sl.nb && owns_band(own, sl.band0 + tid / TR)) my_pidx = pair_idx[sl.pb_off + sl.band0 + tid / TR - sl.b0];
    if (PLANNED && !BOUNDED) {
        if (tid < n_cell) {
            const int g = tid / sl.nk, k = tid - g * sl.nk;
            const int cell = cell_of(g, k);
            if (cell < cell_cap) my_plan = cell_plan[cell];
        }
        plan_pending = true;
    }

    // a batch of edges (slot = tid + j * PB_THREADS): set up, rows inside the slab counted; the edges that have any are kept,
    // in order, with the prefix sums of their row counts -> number of (edge, row) tasks of the batch
    auto stage = [&](int eb, bool bounds = false) -> int {
        int cnt[PB_EPL], eya[PB_EPL];
        EdgeLds el[PB_EPL];
#pragma unroll
        for (int j = 0; j < PB_EPL; ++j) {
            const int e = eb + tid + j * PB_THREADS;
            cnt[j] = 0;
            el[j].p0y = el[j].p1y = el[j].dxdy = el[j].x = 0.0; eya[j] = 0;
            if (e < e_end && tid + j * PB_THREADS < PB_BATCH) {
                const double4 ed = ((const double4*)edges)[e];
                const double ar = ed.x - o_r, ac = ed.y - o_c, br = ed.z - o_r, bc = ed.w - o_c;
                const EdgeSetup es = edge_setup(ar, ac, br, bc, rows);
                // an edge whose every column is beyond the layer never stores anything (S:2260, S:2274)
                const double cmin = ac < bc ? ac : bc;
                if (es.valid && !(cmin >= (double)cols + 2.0)) {
                    const int ya = es.y_begin > sr0 ? es.y_begin : sr0, yb = es.y_end < sr1 ? es.y_end : sr1;
                    if (ya < yb) {
                        cnt[j] = yb - ya;
                        // carry x from the edge's first row to the slab's, exactly as the walk would (S:2244-2248)
                        el[j].p0y = es.p0y; el[j].p1y = es.p1y; el[j].dxdy = es.dxdy; el[j].x = replay_rows(es.x, es.y_begin, ya - es.y_begin, es.p0y, es.p1y, es.dxdy);
                        eya[j] = ya | (es.dir < 0.0 ? (int)0x80000000 : 0);  // (ya >= 0)
                    }
                }
            }
        }
#ifdef SVGR_DBG_PB_STAMP
        if (PLANNED && eb == e_begin) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); PB_STAMP(5); }
#endif
        // one scan for both prefix sums: rows in bits 0-19, kept edges in bits 20-
        int excl[PB_EPL], wtot[PB_EPL];
#pragma unroll
        for (int j = 0; j < PB_EPL; ++j) excl[j] = wave_excl_scan(cnt[j] | ((cnt[j] > 0 ? 1 : 0) << 20), lane, wtot[j]);
        pb_barrier();  // (the previous batch's tasks are done with s_edge / s_pref)
        if (PLANNED && plan_pending) {
            if (tid < PB_CELLS) { s_pos[tid] = my_plan.x; s_plan_n[tid] = my_plan.y; }
            // (the lean form has no register to carry the pairs' places and the rule byte through the row loop: they wait in LDS like the places)
            if (LEAN && (tid & (TR - 1)) == 0) s_pidx[tid / TR] = my_pidx;
            if (LEAN && tid == 0) s_rl = rl;
            plan_pending = false;
        }
        if (BOUNDED && bounds) {
            // Every kept edge adds, to each cell it can reach, an upper bound of the adds it can leave there: `band_room` (svgr_core.h) of
            // where it enters and leaves the band -- in closed form: the recurrence's sum of dy is yhi - ylo.  The TILES: the columns it
            // can touch, one more on the right for the carry piece, clamped like row_tiles clamps a row's; an edge that reaches two
            // tiles of a band gives each the whole amount.
#pragma unroll
            for (int j = 0; j < PB_EPL; ++j) {
                if (cnt[j] <= 0) continue;
                const int ya = eya[j] & 0x7fffffff, yb = ya + cnt[j];
                const double dx = el[j].dxdy;
                const double ylo = (double)ya > el[j].p0y ? (double)ya : el[j].p0y;   // where the edge's first traced row in the slab starts
                for (int y0 = ya; y0 < yb;) {
                    const int vrow = r0 + y0 - vr0, band = vrow / TR;
                    int y1 = y0 + TR - (vrow & (TR - 1));
                    y1 = y1 < yb ? y1 : yb;
                    if (owns_band(own, band)) {
                        const double ta = ((double)y0 > el[j].p0y ? (double)y0 : el[j].p0y) - ylo;
                        const double tb = ((double)y1 < el[j].p1y ? (double)y1 : el[j].p1y) - ylo;
                        int lo, hi;
                        const int room = band_room(el[j].x + dx * ta, el[j].x + dx * tb, y1 - y0, cols, PX, lo, hi);
                        if (lo < cols) {   // (rows wholly beyond the layer store nothing, S:2260)
                            const int cf = lo > 0 ? lo : 0;
                            int cl = hi + 1 > 0 ? hi + 1 : 0;
                            cl = cl < cols - 1 ? cl : cols - 1;
                            int kf = (cf - x_first) / TC, kl = (cl - x_first) / TC;
                            kf = kf > sl.k0 ? kf : sl.k0;
                            kl = kl < sl.k0 + sl.nk - 1 ? kl : sl.k0 + sl.nk - 1;
                            for (int k = kf; k <= kl; ++k)
                                __hip_atomic_fetch_add(&s_plan_n[(band - sl.band0) * sl.nk + (k - sl.k0)], room, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        }
                    }
                    y0 = y1;
                }
            }
        }
#pragma unroll
        for (int j = 0; j < PB_EPL; ++j)
            if (lane == 0) s_wtot[j][wave] = wtot[j];
        pb_barrier();
        int all = 0;
        int pre[PB_EPL];
#pragma unroll
        for (int j = 0; j < PB_EPL; ++j) {
            int before = all;
#pragma unroll
            for (int w = 0; w < PB_THREADS / 64; ++w) { before += w < wave ? s_wtot[j][w] : 0; all += s_wtot[j][w]; }
            pre[j] = before + excl[j];
        }
        const int n_live = all >> 20, total = all & 0xfffff;
        // the tasks are dealt as runs of `per` (for_rows): the run of lane k starts at task k * per -- the edge that holds that task
        // says so itself (`s_start[k]`: a lane reads where it starts instead of searching the prefix sums: 90 vector instructions
        // and two dependent rounds of LDS reads per wave)
        const int nl = det ? 64 : PB_THREADS;
        const int per = (total + nl - 1) / nl;
        s_per = per;
        const float inv_per = per > 0 ? 1.0f / (float)per : 0.f;
#pragma unroll
        for (int j = 0; j < PB_EPL; ++j) {
            if (cnt[j] > 0) {
                const int cs = pre[j] >> 20, tp = pre[j] & 0xfffff;
                s_edge[cs] = el[j];
                s_eya[cs] = eya[j];
                s_pref[cs] = tp;
                if (cs == n_live - 1) s_pref[n_live] = 0x7fffffff;   // (behind the last kept edge: larger than any task number)
                // k0 = ceil(tp / per): a float estimate (tp < 2^20, exact in float), put right by two compares
                int k0 = (int)((float)tp * inv_per);
                k0 += k0 * per < tp ? 1 : 0;
                k0 -= (k0 - 1) * per >= tp ? 1 : 0;
                for (int k = k0; k * per < tp + cnt[j]; ++k) s_start[k] = (unsigned short)cs;
            }
        }
        pb_barrier();
        return total;
    };
    // the row of a task: its pieces (S:2250-2303) and where they fall
    struct RowAt {
        int x0i, n;
        double v[5];
        int where;   // bl | trow << 8 | live << 16
    };
    auto row_at = [&](double x, double x_next, double d, int y) -> RowAt {
        RowAt ra;
        const RowPieces rp = row_record(x, x_next, d);
        ra.x0i = rp.x0i; ra.n = rp.n;
        ra.v[0] = rp.v[0]; ra.v[1] = rp.v[1]; ra.v[2] = rp.v[2]; ra.v[3] = rp.v[3]; ra.v[4] = rp.v[4];
        if ((unsigned)ra.n > SPAN_MAX) { atomicOr(&bd->err, 16); ra.n = (int)SPAN_MAX; }
        const int vrow = r0 + y - vr0, band = vrow / TR;
        const bool live = owns_band(own, band) && rp.x0i < cols;  // (another rank's band; a row wholly beyond the layer, S:2260)
        ra.where = (band - sl.band0) | ((vrow & (TR - 1)) << 8) | ((int)live << 16);
        return ra;
    };
    // The `total` tasks of the staged batch, every lane a run of consecutive ones: body(RowAt).
    // (SVGR_RENDER_DETERMINISTIC: the first wave alone takes the rows -- every sum and every list is then filled in the same
    //  order from render to render, and in the same order by the plan's passes and by the planned renders)
    auto for_rows = [&](int total, auto&& body) {
        const int nl = det ? 64 : PB_THREADS;
        const int per = s_per;
        int t = tid * per;
        const int t1 = t + per < total ? t + per : total;
        if (tid >= nl || t >= t1) return;
        const int slot0 = s_start[tid];
        int slot = slot0;
        const int dy = t - s_pref[slot0];
        EdgeLds el = s_edge[slot];
        int ya_dir = s_eya[slot];
        int y = ya_dir & 0x7fffffff;
        double dir = ya_dir < 0 ? -1.0 : 1.0;
        int t_next = s_pref[slot + 1];   // first task of the next kept edge
        RowState st;
        st.x_next = replay_rows(el.x, y, dy, el.p0y, el.p1y, el.dxdy);
        st.x = st.x_next; st.d = 0.0;
        y += dy;
        for (; t < t1; ++t, ++y) {
            if (t == t_next) {
                ++slot;
                el = s_edge[slot];
                ya_dir = s_eya[slot];
                y = ya_dir & 0x7fffffff;
                dir = ya_dir < 0 ? -1.0 : 1.0;
                t_next = s_pref[slot + 1];
                st.x_next = el.x;
            }
            row_step(st, y, el.p0y, el.p1y, el.dxdy, dir);
            body(row_at(st.x, st.x_next, st.d, y));
        }
    };
    // the slab's column tiles [kf, kl] (relative to the path's first) the pieces of a row fall into
    auto row_tiles = [&](const RowAt& ra, int& kf, int& kl) {
        const int xl = ra.x0i + (ra.n >= 2 ? ra.n : 1);  // column of the last piece
        const int cf = ra.x0i > 0 ? ra.x0i : 0;
        int cl = xl > 0 ? xl : 0;
        cl = cl < cols - 1 ? cl : cols - 1;
        kf = (cf - x_first) / TC;
        kl = (cl - x_first) / TC;
        kl = kl < sl.k0 + sl.nk - 1 ? kl : sl.k0 + sl.nk - 1;
    };
    // layer columns [ca, cb) of the path's column tile k
    auto tile_cols = [&](int k, int& ca, int& cb) {
        ca = k * TC + x_first;
        cb = ca + TC;
        ca = ca > 0 ? ca : 0;
        cb = cb < cols ? cb : cols;
    };
    // the pieces of a row that fall into the cell of column tile k, as adds behind `dst`
    auto store_pieces = [&](const RowAt& ra, int trow, int ca, int cb, int cell_c0, TileAdd* dst) {
        record_adds(ra.x0i, ra.n, ra.v, ca, cb,
                    [&](int c, double val) { store_add(dst++, add_where(trow, c - cell_c0, 1), val); },
                    [&](int c, int len, double val) {
                        int tc = c - cell_c0;
                        while (len > 0) {  // (one piece per chunk of PX columns)
                            const int n = len < PX - (tc & (PX - 1)) ? len : PX - (tc & (PX - 1));
                            store_add(dst++, add_where(trow, tc, n), val);
                            tc += n; len -= n;
                        }
                    });
    };
    // One row, per cell its pieces fall into: the number of adds they make there, their sum, the row's bit.
    // STORE (a planned render): the adds themselves too, at the cell's planned place + what the counter held.
    auto count_row = [&](const RowAt& ra, auto store) {
        constexpr bool STORE = decltype(store)::value;
        if (!((ra.where >> 16) & 1)) return;
        const int bl = ra.where & 0xff, trow = (ra.where >> 8) & 0xff;
        int kf, kl;
        row_tiles(ra, kf, kl);
        if (sl.k0 > 0 && kf < sl.k0) {
            // (a slab that is not the first of its band row: what lies left of it is only summed)
            int ca, cb;
            tile_cols(sl.k0, ca, cb);
            const double part = record_sum_range(ra.x0i, ra.n, ra.v, 0, ca);
            __hip_atomic_fetch_add(&s_left[trow], part, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            __hip_atomic_fetch_or(&s_rowb[PB_CELLS], 1u << trow, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            kf = sl.k0;
        }
        for (int k = kf; k <= kl; ++k) {
            int ca, cb;
            tile_cols(k, ca, cb);
            int ne = 0;
            double part = 0.0;
            const int cell_c0 = k * TC + x_first;  // layer column of the tile's column 0
            record_adds(ra.x0i, ra.n, ra.v, ca, cb, [&](int, double val) { ++ne; part = part + val; },
                        [&](int c, int len, double val) { ne += run_pieces(c - cell_c0, len); part = part + (double)len * val; });
            if (ne == 0) continue;
            const int ci = bl * sl.nk + (k - sl.k0);
            const int pos = __hip_atomic_fetch_add(&s_cnt[ci], ne, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            __hip_atomic_fetch_add(&s_sum[ci * TR + trow], part, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            __hip_atomic_fetch_or(&s_rowb[ci], 1u << trow, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (STORE) {
                const int first = s_pos[ci];
                // (more pieces than the plan counted here, or a cell the plan has no place for: the walk flags the cell)
                if (first < 0 || pos + ne > s_plan_n[ci]) continue;
                store_pieces(ra, trow, ca, cb, cell_c0, adds + ((size_t)first + pos));
            }
        }
    };
    // pass B of one row (PLANNED = false): the pieces as adds, behind what their cells' lists hold already
    auto emit_row = [&](const RowAt& ra) {
        if (!((ra.where >> 16) & 1)) return;
        const int bl = ra.where & 0xff, trow = (ra.where >> 8) & 0xff;
        int kf, kl;
        row_tiles(ra, kf, kl);
        kf = kf > sl.k0 ? kf : sl.k0;
        for (int k = kf; k <= kl; ++k) {
            int ca, cb;
            tile_cols(k, ca, cb);
            int ne = 0;
            const int cell_c0 = k * TC + x_first;  // layer column of the tile's column 0
            record_adds(ra.x0i, ra.n, ra.v, ca, cb, [&](int, double) { ++ne; },
                        [&](int c, int len, double) { ne += run_pieces(c - cell_c0, len); });
            if (ne == 0) continue;
            const int ci = bl * sl.nk + (k - sl.k0);
            const int pos = __hip_atomic_fetch_add(&s_pos[ci], ne, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (pos < 0) continue;  // (the cell was refused by the walk: flagged there)
            store_pieces(ra, trow, ca, cb, cell_c0, adds + pos);
        }
    };

    // ---- pass A ----
    const bool one_batch = e_end - e_begin <= PB_BATCH;
    int total = 0, n_rows = 0;
    if (BOUNDED) {
        // the bounds of every staged batch, then the cells' places from them (one reservation for the slab), then the rows' pass
        for (int eb = e_begin; eb < e_end; eb += PB_BATCH) {
            total = stage(eb, true);
            n_rows += total;
        }
        PB_STAMP(1);
        static_assert(PB_CELLS <= 128, "the cells' places: a prefix sum by the first two waves");
        int room = 0, excl = 0;
        if (tid < 128) {
            const int bnd = tid < n_cell ? s_plan_n[tid] : 0;
            // (+ its carry-in adds: one per row of the layer in the band at most; + its sentinels: likewise, only in the column tile the
            //  layer ends in)
            const int gg = tid < n_cell ? tid / sl.nk : 0, kk = tid < n_cell ? tid - gg * sl.nk : 0;
            const bool ends_here = cols - ((sl.k0 + kk) * TC + x_first) < TC;
            const int b_lo = vr0 + (sl.band0 + gg) * TR - r0;                       // the band's first row in layer rows
            const int rin = (b_lo + TR < rows ? b_lo + TR : rows) - (b_lo > 0 ? b_lo : 0);   // rows of the layer in the band
            room = bnd > 0 ? bnd + rin + (ends_here ? rin : 0) : 0;
            int wt;
            excl = wave_excl_scan(room, lane, wt);
            if (lane == 0) s_ptot[wave] = wt;
        }
        pb_barrier();
        if (tid == 0) {
            const int all = s_ptot[0] + s_ptot[1];
            const int sh = p % ash.n;
            int at = 0;
            if (all > 0) at = atomicAdd(&bd->shard[sh].add_cursor, all);
            int ok = 1;
            if ((long long)at + all > (long long)ash.cap[sh]) { atomicOr(&bd->err, 64); ok = 0; }
            s_base = ash.base[sh] + at;
            s_ok = ok;
        }
        pb_barrier();
        if (tid < n_cell) s_pos[tid] = room > 0 && s_ok ? s_base + (wave ? s_ptot[0] : 0) + excl : (int)0x80000000;
        pb_barrier();
        if (one_batch) {
            for_rows(total, [&](const RowAt& ra) { count_row(ra, std::true_type{}); });   // (the batch is still staged)
        } else {
            for (int eb = e_begin; eb < e_end; eb += PB_BATCH) {
                const int tot = stage(eb);
                for_rows(tot, [&](const RowAt& ra) { count_row(ra, std::true_type{}); });
            }
        }
    } else if constexpr (LEAN) {
        // (the first batch apart from the loop over the others: what only its stage() parks in LDS -- the places, the pairs' places, the
        //  rule byte -- is in no register while the later batches run, and most slabs have one batch)
        if (e_begin < e_end) {
            total = stage(e_begin);
            for_rows(total, [&](const RowAt& ra) { count_row(ra, std::true_type{}); });
            for (int eb = e_begin + PB_BATCH; eb < e_end; eb += PB_BATCH) {
                total = stage(eb);
                for_rows(total, [&](const RowAt& ra) { count_row(ra, std::true_type{}); });
            }
        }
    } else
    for (int eb = e_begin; eb < e_end; eb += PB_BATCH) {
        total = stage(eb);
        PB_STAMP(1);
        n_rows += total;
        if (PLANNED) for_rows(total, [&](const RowAt& ra) { count_row(ra, std::true_type{}); });
        else for_rows(total, [&](const RowAt& ra) { count_row(ra, std::false_type{}); });
    }
    if (stats && tid == 0 && n_rows > 0) atomicAdd(&bd->bseg_cursor, n_rows);  // (plan only: edge rows of the batch)
    if (guarding && __builtin_amdgcn_readfirstlane(wave) == 0) {
        // (the workgroups from the middle of the work list on: neither the heaviest slabs, dispatched first, nor the launch's tail;
        //  the stride only matters to a batch of more than 64 paths per slab)
        const int grid = (int)gridDim.x, g0 = ((int)blockIdx.x + grid - grid / 2) % grid;
        for (int g = g0; g * 64 < n_paths; g += grid) {
            const int q = g * 64 + lane;
            if (q >= n_paths) continue;
            const unsigned long long* k = guard_keys + 4 * (size_t)q;
            const int4 bb = ((const int4*)guard_bbox)[q];
            const PathBox pb = path_box(k[0], k[1], k[2], k[3], 1, vr0, vc0, vrows, vcols, TR, TC);
            if (pb.refused) atomicOr(&bd->err, 16);
            if (!path_box_is(pb, bb.x, bb.y, bb.z, bb.w, guard_bins[q].nb)) atomicOr(&bd->err, 32);
        }
    }
    pb_barrier();
    PB_STAMP(2);
    if constexpr (LEAN) { rl = s_rl; rule = rl & 1; }
    // ---- walk ----
    // what one lane (tile row row_l) writes of a cell of class 1 or 2: its carry-in (class 1: into the header; class 2: an add at
    // the layer's first column in the tile, if any row piece lies left of the cell), its sentinel (behind the layer's last
    // column), and -- lane 0 of the cell -- the header and the entry-bitmask bits
    auto write_cell = [&](int g, int k, int cls, double cin, unsigned cm, unsigned sm, int own_n, int n_list, int add0, int row_l, int idx,
                          bool slab_ok) -> bool {
        const int band = sl.band0 + g;
        const int cell = cell_of(g, k);
        const bool mask_ok = (unsigned)(idx >> 6) < (unsigned)mask_words;  // (the plan sized the masks from the longest band list)
        if (!(cell < cell_cap && slab_ok && mask_ok) || (PLANNED && cls == 2 && add0 < 0)) {
            if (row_l == 0) atomicOr(&bd->err, 32);
            return false;
        }
        CellHdr* hd = cell_hdr + cell;
        if (cls == 1) hd->carry[row_l] = cin;   // (a class-2 cell's carry-ins are adds of its list: the tile kernel does not load this part of its header)
        const int cell_c0 = (sl.k0 + k) * TC + x_first;       // layer column of the tile's column 0
        const unsigned below = (1u << row_l) - 1u;
        const int n_carry = __popc(cm);
        if (((cm >> row_l) & 1u) && adds) {
            // at the layer's first column in the tile
            store_add(adds + ((size_t)add0 + own_n + __popc(cm & below)), add_where(row_l, cell_c0 < 0 ? -cell_c0 : 0, 1), cin);
        }
        // (the lean form stores none: where it stands and what it holds follows from the geometry's integers, and the full pass of this
        //  plan that the host's record asks for -- PlanState::cells -- has put it there)
        if (!LEAN && ((sm >> row_l) & 1u) && adds) {
            // behind the layer's last column
            store_add(adds + ((size_t)add0 + own_n + n_carry + __popc(sm & below)), add_where(row_l, cols - cell_c0, 1), __builtin_nan(""));
        }
        if (row_l == 0) {
            // the tiles' entry bitmasks: per (band, column tile) two rows of mask_words words, bit i = entry i of the band's
            // list has a cell of class >= 1 (row 0) / class 2 (row 1) here.  Classes 0 simply stay unset.
            unsigned long long* const mw = tile_mask + ((size_t)band * n_ct + ct0 + sl.k0 + k) * 2 * mask_words + (idx >> 6);
            const unsigned long long mbit = 1ull << (idx & 63);
            // (the lean form sets neither bit of a class-2 cell: the cell is class 2 by the plan's count alone, and k_tile_lists, which the
            //  host then asks to keep its lists, takes both bits from the words it saved -- `kept` == 2 there)
            if (LEAN && cls == 2) return true;
            atomicOr(mw, mbit);
            if (cls == 2) atomicOr(mw + mask_words, mbit);
            // (a class-2 cell's header -- paint, layer box, rule, its list's place and length, path, group -- is the same 80 bytes in every
            //  pass of one plan with one set of paints: the lean form has left above, and what the full pass wrote stands)
            hd->paint[0] = paint.x; hd->paint[1] = paint.y; hd->paint[2] = paint.z; hd->paint[3] = paint.w;
            hd->r0 = r0; hd->c0 = c0; hd->rows = rows; hd->cols = cols;
            hd->bits = rule | (((rl >> 1) & 3) << 1) | (cls << 3) | (grad1 << 5);
            hd->n_add = n_list; hd->add0 = add0; hd->p = p;
            hd->group = group;
        }
        return true;
    };
    {
        // TR lanes per band of the slab (lane = tile row) go through the band's cells left to right with the row's running sum
        // = the carry-in; per cell: class, adds, and which rows have a carry-in / a sentinel (as bit masks of the band's TR lanes).
        // PLANNED: the cell's place is known, so the lanes write the cell at once.  Else the row's running sum replaces the
        // cell's sum in s_sum and the cell's description goes to LDS: the write phase needs the slab's reservation first.
        static_assert(TR <= 16, "k_path_build packs two TR-bit row masks into one word");
        constexpr unsigned long long GMASK = (1ull << TR) - 1ull;
        const int g = tid / TR, row_l = tid & (TR - 1);
        const int shift = lane & ~(TR - 1);          // first lane of this band's group in the wave
        const int band = sl.band0 + g;
        const bool active = g < sl.nb && owns_band(own, band);
        const int row_abs = vr0 + band * TR + row_l;
        const bool row_in_layer = row_abs >= r0 && row_abs < r0 + rows;  // (the sentinel is set on rows of the layer only)
        int cursor = 0;                                    // adds of the column tiles walked so far
        bool mismatch = false;
        if (__ballot(active) != 0ull) {  // (a wave none of whose bands exists has nothing to walk)
            const int idx = LEAN ? s_pidx[g] : my_pidx;        // the pair's place in its band's list
            if (!PLANNED && active && row_l == 0) s_pidx[g] = idx;
            double run = sl.k0 > 0 ? s_left[row_l] : 0.0;      // the row's running sum left of the column tile
            unsigned had = sl.k0 > 0 ? s_rowb[PB_CELLS] : 0u;  // tile rows with a piece left of the column tile
            const unsigned sent_rows = (unsigned)((__ballot(active && row_in_layer) >> shift) & GMASK);
            for (int k = 0; k < sl.nk; ++k) {
                const int ci = g * sl.nk + k;
                const int own_n = active ? s_cnt[ci] : 0;
                const double sq = active ? s_sum[ci * TR + row_l] : 0.0;
                const unsigned rb = active ? s_rowb[ci] : 0u;
                const double cin = run;
                const bool vis = active && carry_visible(cin, rule);
                const unsigned long long vm = (__ballot(vis) >> shift) & GMASK;
                const int cls = own_n > 0 ? 2 : (vm != 0ull ? 1 : 0);
                // class 2: the cell's add list = [pieces][a carry-in for every row with a piece left of the cell][sentinels]
                const int t_end = cols - ((sl.k0 + k) * TC + x_first);     // tile column one past the layer's last column
                const unsigned cm = cls == 2 ? had & (unsigned)GMASK : 0u;
                const unsigned sm = cls == 2 && t_end < TC ? sent_rows : 0u;
                const int n_add = cls == 2 ? __popc(cm) + __popc(sm) + own_n : 0;
                if (active) {
                    if (PLANNED) {
                        if (row_l == 0 && (BOUNDED ? own_n > s_plan_n[ci] : own_n != s_plan_n[ci])) mismatch = true;   // (more pieces than the bound / not the plan's count)
                        if (BOUNDED && row_l == 0) {   // (what the planned renders that follow take their places from)
                            const int cell = cell_of(g, k);
                            if (cell < cell_cap) cell_plan[cell] = make_int2(cls == 2 ? s_pos[ci] : (int)0x80000000, cls == 2 ? own_n : 0);
                        }
                        if (cls != 0) write_cell(g, k, cls, cin, cm, sm, own_n, n_add, s_pos[ci], row_l, idx, true);
                    } else {
                        s_sum[ci * TR + row_l] = cin;
                        if (row_l == 0) {
                            s_cnt[ci] = n_add;                                   // (the cell's whole list now)
                            s_info[ci] = make_int2(cursor, cls);
                            s_rowm[ci] = cm | (sm << 16);
                        }
                    }
                }
                cursor += n_add;
                run = run + sq;
                had |= rb;
            }
        }
        if (PLANNED) {
            if (mismatch) atomicOr(&bd->err, 32);  // (not the plan's geometry: its places do not hold -- as in k_path_bbox)
        } else {
            // the slab's reservation of add slots: ONE atomic, in the path's shard
            if (row_l == 0 && g < PB_BANDS) s_ptot[g] = active ? cursor : 0;
            pb_barrier();
            if (tid < 64) {  // the bands' offsets: an exclusive scan over <= PB_BANDS totals by the first wave
                static_assert(PB_BANDS <= 64, "one lane per band of the slab");
                const int c = tid < sl.nb ? s_ptot[tid] : 0;
                int all;
                const int ex = wave_excl_scan(c, tid, all);
                if (tid < sl.nb) s_ptot[tid] = ex;
                if (tid == 0) {
                    const int sh = p % ash.n;  // (by path, not by slab: the slabs' order changes from pass to pass, the plan's shard sizes must hold)
                    int at = 0;
                    if (all > 0) at = atomicAdd(&bd->shard[sh].add_cursor, all);
                    int ok = 1;
                    if (adds && (long long)at + all > (long long)ash.cap[sh]) { atomicOr(&bd->err, 64); ok = 0; }
                    s_base = ash.base[sh] + at;
                    s_ok = ok;
                }
            }
            pb_barrier();
        }
    }
    PB_STAMP(3);
    if (!PLANNED) {
        // write: one lane per (cell, tile row); no lane idles through a band that does not exist.  Per cell {first add, pieces}
        // into `cell_plan`: what the renders of this plan take their places from.
        const bool slab_ok = s_ok != 0;
        for (int i = tid; i < n_cell * TR; i += PB_THREADS) {
            const int ci = i / TR, row_l = i & (TR - 1);
            const int2 info = s_info[ci];
            const unsigned rowm = s_rowm[ci];
            const int cls = info.y & 3, g = ci / sl.nk, k = ci - g * sl.nk;   // (a cell of another rank's band was never walked: its s_info is empty)
            if (!owns_band(own, sl.band0 + g)) continue;
            const int cell = cell_of(g, k);
            const int n_list = s_cnt[ci];
            const unsigned cm = rowm & 0xffffu, sm = rowm >> 16;
            const int own_n = n_list - __popc(cm) - __popc(sm);                    // (class 2: its pieces)
            const int add0 = s_base + s_ptot[g] + info.x;
            if (row_l == 0 && cell < cell_cap) cell_plan[cell] = make_int2(cls == 2 && slab_ok ? add0 : (int)0x80000000, cls == 2 ? own_n : 0);
            if (cls == 0) continue;
            const bool ok = write_cell(g, k, cls, s_sum[i], cm, sm, own_n, n_list, add0, row_l, s_pidx[g], slab_ok);
            if (ok && row_l == 0 && cls == 2 && adds) s_pos[ci] = add0;  // the pieces come first (pass B); a refused cell keeps "no place"
        }
    }
    PB_STAMP(4);
    if (PLANNED || !adds) {
#ifndef SVGR_DBG_PB_STAMP
        PB_STAMP(5);
#endif
        if (threadIdx.x == 0 && dbg && blockIdx.x < 8192) dbg[8 * blockIdx.x + 6] = (unsigned long long)n_rows;
        return;
    }
    pb_barrier();

    // ---- pass B ----  (PLANNED = false only)
    if (one_batch) {
        for_rows(total, emit_row);  // (the batch is still staged)
    } else {
        for (int eb = e_begin; eb < e_end; eb += PB_BATCH) {
            const int tot = stage(eb);
            for_rows(tot, emit_row);
        }
    }
    PB_STAMP(5);
    if (threadIdx.x == 0 && dbg && blockIdx.x < 8192) dbg[8 * blockIdx.x + 6] = (unsigned long long)n_rows;
}

// After k_path_build, one workgroup per owned band: the tiles' entry bitmasks become their item lists -- the cell ids of
// the set bits, in bit = list = paint order (class in the top bits) -- and the band's tiles are sorted by weight (number
// of items, cells with records counting twice), heaviest first.  The launch order of the tile kernel interleaves the
// bands' sorted lists (rank-major), which is a global heaviest-first order when the bands are alike: the long tiles
// start first and the launch ends on short ones.  The bitmasks are cleared for the next render.
// One lane per ITEM: an item's tile by binary search in the chunk's prefix sums, its bit by a select over the tile's words.
struct TileSlot {
    int band, ct;        // the tile: ordinal of its band among the owned bands, column tile
    int item0, n_items;  // its item list
};
// What workgroup w of a whole-canvas launch of the tile kernel asks for first: its PAGE -- the tile it takes (a TileSlot, in
// the page's last 16 bytes) and a copy of the first PAGE_ITEMS items of that tile's list, PAGE_STRIDE x 16 bytes that ONE load
// instruction fetches (a lane each).  Tile and items used to be two dependent round trips in front of the first header.
constexpr int PAGE_ITEMS = 24, PAGE_STRIDE = PAGE_ITEMS + 1;
static_assert(PAGE_STRIDE + 1 <= 64, "a page is one load per lane (and one more lane for the last word of the tile's entry)");
constexpr int TL_BLOCK = 1024;
__device__ __forceinline__ int select_bit(unsigned long long m, int r) {  // position of the r-th (0-based) set bit of m
    unsigned x = (unsigned)m;
    int pos = 0;
    int c = __popc(x);
    if (r >= c) { r -= c; pos = 32; x = (unsigned)(m >> 32); }
#pragma unroll
    for (int w = 16; w >= 1; w >>= 1) {
        const unsigned lo = x & ((1u << w) - 1u);
        c = __popc(lo);
        if (r >= c) { r -= c; pos += w; x >>= w; } else { x = lo; }
    }
    return pos;
}
__global__ __launch_bounds__(TL_BLOCK) void k_tile_lists(const int* __restrict__ band_start, const int* __restrict__ band_item0,
                                                         const TileEntry* __restrict__ entries, unsigned long long* __restrict__ tile_mask,
                                                         int mask_words, int n_ct, int vc0, Owner own, int n_owned,
                                                         int2* __restrict__ tile_info, uint4* __restrict__ pages,
                                                         uint4* __restrict__ items, const CellHdr* __restrict__ cell_hdr, int item_cap, int cell_cap,
                                                         BatchDev* __restrict__ bd, const PathBin* __restrict__ bins, const int* __restrict__ bbox,
                                                         unsigned long long* __restrict__ tile_mask_kept, int kept) {
    constexpr int NWV = TL_BLOCK / 64;
    __shared__ int s_base[TL_BLOCK + 1], s_rank[TL_BLOCK];
    __shared__ int s_hist[64], s_cur[64], s_wtot[NWV];
    __shared__ int s_run;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int band = owned_band_at(own, blockIdx.x);
    const int W = mask_words;
    unsigned long long* const mband = tile_mask + (size_t)band * n_ct * 2 * W;
    // `tile_mask_kept` (a placed replay that keeps its lists): the band's mask words as they stood when the lists now in place were
    // made -- the full path below saves them just before it clears them.  `kept`: those lists ARE in place (the host's record,
    // PlanState::lists).  Everything else an item is made of -- cell id, add place, add count -- is the plan's, checked by
    // k_path_build<1> (error bit 32), so a band whose words repeat would rewrite, item by item, what stands there: one round of
    // loads, both arrays asked for together, the words cleared, done.  A band with any other word is listed again as if entered here.
    unsigned long long* const kband = tile_mask_kept ? tile_mask_kept + (size_t)band * n_ct * 2 * W : nullptr;
    if (kept) {
        __shared__ int s_wdiff[NWV];
        auto any_differs = [&](bool d) {   // (one barrier: a flag per wave, every lane ORs the sixteen)
            const bool wd = __ballot(d) != 0ull;
            if (lane == 0) s_wdiff[wave] = wd ? 1 : 0;
            __syncthreads();
            int a = 0;
#pragma unroll
            for (int w = 0; w < NWV; ++w) a |= s_wdiff[w];
            return a != 0;
        };
        // `kept` == 2: the path build was the lean form, which sets no bit of a class-2 cell -- those cells are class 2 by the plan's
        // counts, in every replay.  The words to expect are then the saved class >= 1 row without the saved class-2 row, and an empty
        // class-2 row; a band that differs gets its full words back (row 0 | saved row 1, saved row 1) and is listed as ever.
        const bool implied = kept == 2;
        unsigned long long diff = 0ull;
        if (W == 1 && n_ct <= TL_BLOCK) {
            ulonglong2 m = make_ulonglong2(0ull, 0ull), k = m;
            if (tid < n_ct) { m = ((const ulonglong2*)mband)[tid]; k = ((const ulonglong2*)kband)[tid]; }
            diff = implied ? (m.x ^ (k.x & ~k.y)) | m.y : (m.x ^ k.x) | (m.y ^ k.y);
            if (!any_differs(diff != 0ull)) {
                if ((m.x | m.y) != 0ull) ((ulonglong2*)mband)[tid] = make_ulonglong2(0ull, 0ull);
                return;
            }
        } else {
            for (int ct = tid; ct < n_ct; ct += TL_BLOCK) {
                const unsigned long long* mw = mband + (size_t)ct * 2 * W;
                const unsigned long long* kw = kband + (size_t)ct * 2 * W;
                if (implied) for (int w = 0; w < W; ++w) diff |= (mw[w] ^ (kw[w] & ~kw[W + w])) | mw[W + w];
                else for (int w = 0; w < 2 * W; ++w) diff |= mw[w] ^ kw[w];
            }
            if (!any_differs(diff != 0ull)) {
                for (int ct = tid; ct < n_ct; ct += TL_BLOCK) {
                    unsigned long long* mw = mband + (size_t)ct * 2 * W;
                    for (int w = 0; w < 2 * W; ++w) mw[w] = 0ull;
                }
                return;
            }
        }
        if (implied) {   // (the band is listed again: from its full words)
            for (int ct = tid; ct < n_ct; ct += TL_BLOCK) {
                unsigned long long* mw = mband + (size_t)ct * 2 * W;
                const unsigned long long* kw = kband + (size_t)ct * 2 * W;
                for (int w = 0; w < W; ++w) { const unsigned long long c2 = kw[W + w]; mw[w] |= c2; mw[W + w] = c2; }
            }
            __threadfence_block();
            __syncthreads();
        }
    }
    const int ent0 = band_start[band], item_band0 = band_item0[band];
    auto count_tile = [&](int ct, int& n, int& n2) {
        n = 0; n2 = 0;
        const unsigned long long* mw = mband + (size_t)ct * 2 * W;
        for (int w = 0; w < W; ++w) { n += __popcll(mw[w]); n2 += __popcll(mw[W + w]); }
    };
    auto weight_of = [&](int n, int n2) { const int w = n + n2; return w < 63 ? w : 63; };
    if (tid < 64) s_hist[tid] = 0;
    if (tid == 0) s_run = 0;
    __syncthreads();
    // pass 1: histogram of the tile weights  (a band of up to TL_BLOCK tiles -- every canvas up to 65 536 columns -- keeps its
    // tiles' counts in registers for pass 2: reading the mask words twice was a memory round trip of a 9-us latency chain)
    const bool one_chunk = n_ct <= TL_BLOCK;
    int n_keep = 0, n2_keep = 0;
    for (int c0 = 0; c0 < n_ct; c0 += TL_BLOCK) {
        const int ct = c0 + tid;
        if (ct < n_ct) {
            int n, n2;
            count_tile(ct, n, n2);
            n_keep = n; n2_keep = n2;
            atomicAdd(&s_hist[weight_of(n, n2)], 1);
        }
    }
    __syncthreads();
    if (tid < 64) {  // first rank of every weight, heaviest first
        int before = 0;
        for (int w = 63; w > tid; --w) before += s_hist[w];
        s_cur[tid] = before;
    }
    __syncthreads();
    // pass 2: per chunk of TL_BLOCK tiles: prefix sums -> the tiles' list slots and ranks, then the items
    for (int c0 = 0; c0 < n_ct; c0 += TL_BLOCK) {
        const int ct = c0 + tid;
        int n = 0, n2 = 0;
        if (one_chunk) { n = n_keep; n2 = n2_keep; }
        else if (ct < n_ct) count_tile(ct, n, n2);
        int wtot;
        const int excl = wave_excl_scan(n, lane, wtot);
        if (lane == 0) s_wtot[wave] = wtot;
        __syncthreads();
        if (wave == 0) {
            const int t = lane < NWV ? s_wtot[lane] : 0;
            int tt;
            const int ex = wave_excl_scan(t, lane, tt);
            if (lane < NWV) s_wtot[lane] = ex;
            if (lane == 0) s_base[TL_BLOCK] = tt;  // items of this chunk
        }
        __syncthreads();
        const int run0 = s_run;  // items of the band's earlier chunks
        const int base = s_wtot[wave] + excl;
        s_base[tid] = base;
        if (ct < n_ct) {
            const int item0 = item_band0 + run0 + base;
            const bool fits = (long long)item0 + n <= (long long)item_cap;
            if (!fits) atomicOr(&bd->err, 64);
            tile_info[(size_t)band * n_ct + ct] = make_int2(item0, fits ? n : 0);
            const int rank = atomicAdd(&s_cur[weight_of(n, n2)], 1);
            s_rank[tid] = rank;
            // (band: its ordinal among the owned ones)
            pages[((size_t)rank * n_owned + blockIdx.x) * PAGE_STRIDE + PAGE_ITEMS] = make_uint4(blockIdx.x, (unsigned)ct, (unsigned)item0, (unsigned)(fits ? n : 0));
        }
        __syncthreads();
        const int total = s_base[TL_BLOCK];
        const int n_here = n_ct - c0 < TL_BLOCK ? n_ct - c0 : TL_BLOCK;
        for (int i = tid; i < total; i += TL_BLOCK) {
            int lo = 0, hi = n_here;  // the last tile whose first item is <= i
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (s_base[mid] <= i) lo = mid; else hi = mid;
            }
            int r = i - s_base[lo];
            const int r_tile = r;
            const int tct = c0 + lo;
            const unsigned long long* mw = mband + (size_t)tct * 2 * W;
            int w = 0;
            unsigned long long m = mw[0];
            for (;;) {
                const int c = __popcll(m);
                if (r < c || w + 1 >= W) break;
                r -= c;
                m = mw[++w];
            }
            const int bit = select_bit(m, r);
            int cell;
            if (bins) {
                // A planned render (round 5): the band's list -- which path stands at which place -- is the plan's, and k_band_entries
                // is not launched: it found the same lists again in every render (256 workgroups that each read every path's bins,
                // 7 us of latency).  What an entry says about its path is read from THIS render's bbox and bins instead.
                const int ep = entries[ent0 + w * 64 + bit].p;
                const PathBin pbin = bins[ep];
                const int4 bb = ((const int4*)bbox)[ep];
                int ct0_, nct_;
                path_ctiles(bb.y, bb.w, vc0, ct0_, nct_);
                cell = pbin.cell_off + (band - pbin.b0) * nct_ + (tct - ct0_);
            } else {
                const int4 eh = *(const int4*)(entries + ent0 + w * 64 + bit);  // {c0, cols, cell0, p}
                cell = eh.z + tct - (eh.x - vc0) / TC;
            }
            const unsigned cls = ((mw[W + w] >> bit) & 1ull) ? 2u : 1u;
            cell = cell >= 0 && cell < cell_cap ? cell : 0;
            const long long at = (long long)item_band0 + run0 + i;
            // (the item carries its add list: the tile kernel can then ask for an item's header and its adds at the same time)
            const int4 hd = cls == 2u ? *(const int4*)((const char*)(cell_hdr + cell) + 48) : make_int4(0, 0, 0, 0);  // {bits, n_add, add0, p}
            const uint4 it = make_uint4((unsigned)cell | (cls << 30), (unsigned)hd.z, (unsigned)hd.y, 0u);
            if (at < (long long)item_cap) items[at] = it;
            if (r_tile < PAGE_ITEMS) pages[((size_t)s_rank[lo] * n_owned + blockIdx.x) * PAGE_STRIDE + r_tile] = it;
        }
        __syncthreads();
        if (tid == 0) s_run = run0 + total;
        if (ct < n_ct) {  // this tile has listed everything: its words are cleared for the next render's atomicOr
            unsigned long long* mw = mband + (size_t)ct * 2 * W;
            if (kband) {  // (what these lists were made from: the next replay compares against it)
                unsigned long long* kw = kband + (size_t)ct * 2 * W;
                for (int w = 0; w < 2 * W; ++w) kw[w] = mw[w];
            }
            for (int w = 0; w < 2 * W; ++w) mw[w] = 0ull;
        }
        __syncthreads();
    }
}

// --------------------------------------------------------------------------------------
// gradients (S:1021-1047, 1544-1695): image = gradient(pixel centre) * mask
// --------------------------------------------------------------------------------------
constexpr int GRAD_MAX_STOPS = 32;   // stops carried inside the kernel argument; longer lists travel in a device buffer
struct GradDev {
    int kind, spread, has_gt, n_stops;
    int excl_enabled, pad0, pad1, pad2;
    double user_m6[6], gt_m6[6];
    double p0[2], vec[2], vv;
    double center[2], radius;
    double fcenter[2], fradius, cd[2], rd, a, frad_rd, frad2, excl_thresh;
    double stop_off[GRAD_MAX_STOPS];
    double stop_rgba[GRAD_MAX_STOPS][4];
    const double* ext_stops;  // n_stops > GRAD_MAX_STOPS: {offsets[n], rgba[n][4]} in device memory (the reference has no cap, S:1671-1683)
};

// position of pixel (i, j) of the layer in gradient space: grad_pixels (S:1653-1658), user transform
// (S:1023-1027) and the gradient's own transform (S:1559 / S:1603), both in numpy's fma form
__device__ __forceinline__ void grad_point(const GradDev& g, const double* __restrict__ pts, int i, int j, int r0, int c0, int cols,
                                           double& x, double& y) {
    if (pts) {  // Grad*.fill on a caller's coordinate array (S:1553, S:1577): the points as given -- the reference maps them by
                // nothing but the gradient's own transform, and even an identity matrix makes NaN of an infinite coordinate (inf * 0)
        const size_t idx = (size_t)i * cols + j;
        x = pts[2 * idx];
        y = pts[2 * idx + 1];
    } else {
        const double px = (double)i + ((double)r0 + 0.5);
        const double py = (double)j + ((double)c0 + 0.5);
        xform_point(g.user_m6, px, py, x, y);
    }
    if (g.has_gt) {
        double tx, ty;
        xform_point(g.gt_m6, x, y, tx, ty);
        x = tx;
        y = ty;
    }
}

// focal radial: b, c, det of S:1619-1626
__device__ __forceinline__ double grad_focal_det(const GradDev& g, double x, double y, double& b) {
    double pd0 = x - g.fcenter[0], pd1 = y - g.fcenter[1];
    b = (pd0 * g.cd[0] + pd1 * g.cd[1]) + g.frad_rd;
    double c = (pd0 * pd0 + pd1 * pd1) - g.frad2;
    return b * b - g.a * c;
}

// Colour of the gradient at the user-space point (x, y): offset (S:1561-1562 / S:1606-1607 / S:1619-1644), spread
// (S:1661-1668), piecewise-linear stops (grad_interpolate, S:1671-1683).  `use_mask`: the focal form found a negative
// determinant somewhere in the fill's layer and therefore masks (S:1627-1648).  Shared by the per-node kernel
// (k_gradient_fill) and by the tile kernel's gradient entries, so that both routes give the same bits.
__device__ __forceinline__ void grad_colour_user(const GradDev& g, double x, double y, bool use_mask, double* col) {
    double offset;
    bool masked = false;  // overlay[~mask] = 0 (S:1648)
    if (g.kind == 1) {  // linear, S:1561-1562: ((p - p0) @ vec) / (vec . vec), `@` with a 1-D rhs = fma(d0, v0, d1*v1)
        double d0 = x - g.p0[0], d1 = y - g.p0[1];
        offset = fma(d0, g.vec[0], d1 * g.vec[1]) / g.vv;
    } else if (g.kind == 2) {  // radial, S:1606-1607
        double o0 = (x - g.center[0]) / g.radius, o1 = (y - g.center[1]) / g.radius;
        offset = sqrt(o0 * o0 + o1 * o1);
    } else {  // two-circle (focal) radial, S:1619-1644
        double b;
        double det = grad_focal_det(g, x, y, b);
        if (use_mask && !(det >= 0.0)) {
            masked = true;
            offset = 0.0;
        } else {
            double t0 = sqrt(det);
            double t1 = (b + t0) / g.a, t2 = (b - t0) / g.a;
            offset = t1 > t2 ? t1 : (t2 > t1 ? t2 : (t1 != t1 ? t1 : t2));  // np.maximum (NaN propagates)
            if (use_mask && g.excl_enabled && !(offset > g.excl_thresh)) masked = true;  // negative r(t), S:1642-1644
        }
    }
    if (g.spread == 1) {  // repeat: np.modf(offset)[0], which is +-0 at +-inf (inf - trunc(inf) would be NaN: no stop at all)
        offset = isinf(offset) ? copysign(0.0, offset) : offset - trunc(offset);
    } else if (g.spread == 2) {  // reflect
        double a1 = offset + 1.0;
        offset = fabs((a1 - 2.0 * floor(a1 * 0.5)) - 1.0);
    }
    col[0] = col[1] = col[2] = col[3] = 0.0;
    const int n = g.n_stops;
    // grad_interpolate (S:1671-1683).  Two instantiations: the stops inside the description (a kernel argument for the
    // per-node kernel: scalar loads into SGPRs) and the long lists in device memory.  One pointer chosen at run time
    // would turn BOTH into vector loads with a wait per stop -- the per-node kernel ran at 0.4 of the streaming rate that way.
    auto interpolate = [&](auto off_at, auto rgba_at) {
        if (offset <= off_at(0)) {
            for (int k = 0; k < 4; ++k) col[k] = rgba_at(0, k);
        }
        if (offset > off_at(n - 1)) {
            for (int k = 0; k < 4; ++k) col[k] = rgba_at(n - 1, k);
        }
        for (int s = 0; s + 1 < n; ++s) {
            double o0 = off_at(s), o1 = off_at(s + 1);
            if (offset > o0 && offset <= o1) {
                double ratio = (offset - o0) / (o1 - o0);
                for (int k = 0; k < 4; ++k) col[k] = col[k] + ((1 - ratio) * rgba_at(s, k) + ratio * rgba_at(s + 1, k));
            }
        }
    };
    if (g.ext_stops) {
        const double* const eo = g.ext_stops;
        const double* const ec = g.ext_stops + n;
        interpolate([&](int s) { return eo[s]; }, [&](int s, int k) { return ec[4 * s + k]; });
    } else {
        interpolate([&](int s) { return g.stop_off[s]; }, [&](int s, int k) { return g.stop_rgba[s][k]; });
    }
    if (masked) col[0] = col[1] = col[2] = col[3] = 0.0;
}
// ... at the centre of the presentation-space pixel (row, col): grad_pixels (S:1653-1658) + the user transform (S:1023-1027)
// + the gradient's own transform, both in numpy's fma form
__device__ __forceinline__ void grad_colour_pixel(const GradDev& g, int row, int col_, bool use_mask, double* col) {
    double x, y;
    xform_point(g.user_m6, (double)row + 0.5, (double)col_ + 0.5, x, y);
    if (g.has_gt) {
        double tx, ty;
        xform_point(g.gt_m6, x, y, tx, ty);
        x = tx;
        y = ty;
    }
    grad_colour_user(g, x, y, use_mask, col);
}

// ======================================================================================
// tile kernel
// ======================================================================================
// nontemporal (streaming) store of 16 bytes: for data this launch writes once and does not read again, in whole lines
typedef float f32x4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void nt_store16(float4* p, const float4 v) {
    f32x4_t nv = {v.x, v.y, v.z, v.w};
    __builtin_nontemporal_store(nv, (f32x4_t*)p);
}
// evenodd fold |((s + 1) mod 2) - 1| (S:986-988) WITHOUT its outer |.|, in three instructions: (s + 1) / 2 by one fma (halving
// is exact, so the single rounding is the one of s + 1), its fractional part, and 2 f - 1 (2 f is exact).  Differs from
// a - 2 floor(a / 2) only where a = s + 1 is a negative number below half an ulp of 2 (v_fract clamps below 1): one ulp.
__device__ __forceinline__ double evenodd_fract_signed(double s) {
    return __builtin_fma(__builtin_amdgcn_fract(__builtin_fma(s, 0.5, 0.5)), 2.0, -1.0);
}
template <int N>
__device__ __forceinline__ double dpp_row_shr(double v) {  // lane i <- lane i-N inside a 16-lane row, else +0.0
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_update_dpp(0, lo, 0x110 + N, 0xf, 0xf, true);  // bound_ctrl: lanes without a source read 0
    hi = __builtin_amdgcn_update_dpp(0, hi, 0x110 + N, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}

// the lane's pixels, one macro call each (asm blocks with named operands cannot be written in a loop over a constexpr index)
static_assert(PX == 8, "the blend statements name a lane's eight pixels (16 px per lane / one wave per tile was built and measured slower: DESIGN section 4)");
#define SVGR_ACC_PX(F) F(0) F(1) F(2) F(3) F(4) F(5) F(6) F(7)
#define SVGR_ACC_PX2(F) F(0) F(2) F(4) F(6)

struct TileArgs {
    const uint4* pages;             // whole-canvas launches: per workgroup, in launch order (k_tile_lists: heaviest first), its page
    const int2* tile_info;          // per (band, column tile): {first item, items} -- what a window launch looks its tiles up in
    const uint4* items;             // the tiles' item lists, in paint order: {cell id | class << 30, first add, adds, 0}
    const CellHdr* cell_hdr;        // per cell of class 1 or 2: paint, layer, fill rule, add list, carry-in of every tile row
    const TileAdd* adds;            // add lists of the class-2 cells
    int n_ct;                       // column tiles of the viewport
    int n_bands;                    // bands of the launch (all owned bands, or those of the render window)
    int use_order;                  // 1: workgroup w takes order[w]; 0: the tiles of the window in raster order
    int ct0, win_ct, band0;         // render window in tiles: column tiles [ct0, ct0 + win_ct), bands from band0 (0, n_ct, 0: all)
    int win_r, win_c;               // ... its first row / column inside its first tile (0 .. TR-1 / TC-1)
    int win_rows, win_cols;         // ... its size = the extent of `out` (canvas outputs)
    const int* group_clip_src;      // per isolated group: path id of the clip source that clips it as a whole, or -1
    const double* group_opacity;    // ... and the opacity it is faded with when it closes (1: none)
    const GradDev* grads;           // gradient paints of the batch (CellHdr::bits carries the entry's index + 1)
    const int* grad_flags;          // per gradient: some pixel of the fill's layer has det < 0 (k_grad_detneg, focal form)
    void* out;
    void* trash;                 // 1 KiB nobody reads: where the lanes of a float32 row store that lie outside the output write
    unsigned* tile_ctr;          // persistent launch: 8 counters (one per XCD's workgroups, 128 bytes apart) that deal the tiles behind
    unsigned* tile_ctr_clear;    // the first two passes; the OTHER set of eight, zeroed by this launch for the next one
    int vr0, vc0, vrows, vcols;  // viewport
    Owner own;                   // owned bands
    int out_cols;                // row pitch of `out` in pixels
    int clip01;
    int det;                     // SVGR_RENDER_DETERMINISTIC: the first wave alone scatters, in list order
    const long long* layer_off;  // mask / fill outputs of several paths: per path the offset (in pixels) of its layer in `out`
    unsigned* arena;             // the batch's counter arena: zeroed here (all but its first word, the sticky error flags) for
    unsigned arena_words;        // the NEXT render, which then needs no memset launch in front of its flatten (0: leave it)
    unsigned long long* dbg;                // diagnostic builds only
};

// svgr_batch_render_windows: ALL the windows of a render in ONE launch.  Every window is a rectangle of tiles with an output buffer
// of its own; workgroup w of the launch draws tile w - tile0 of the window whose range [tile0, next tile0) it falls into.  The table
// rides in the kernel argument (no upload, nothing to keep alive): the workgroup finds its window by a binary search of scalar
// loads and takes the window's fields in the place of the launch's own (TileArgs::out, ct0 ... out_cols).
struct WinRec {
    void* out;
    int tile0;                      // first workgroup of the window
    int ct0, win_ct, band0, n_bands;
    int win_r, win_c;
    int win_rows, win_cols;
    int pad;
};
static_assert(sizeof(WinRec) == 48, "WinRec is 48 bytes");
constexpr int MAX_WINS = 64;        // windows per launch (the kernel argument segment holds 4 KiB)
struct WinTable {
    int n;                          // 0: the launch is one window, described by TileArgs itself
    int pad[3];
    WinRec w[MAX_WINS];
};

// OUT: 0 = canvas f32, 1 = canvas f64, 2 = mask f64 (single path), 3 = fill f64 (single path)
// CLIP: the batch contains SVGR_PATH_CLIP_SOURCE / SVGR_PATH_CLIPPED paths (one more LDS tile: its own instantiation,
// so that batches without clips keep their occupancy)
// GROUPS (implies CLIP): the batch contains isolated groups (SVGR_PATH_GROUP_MEMBER): a second register tile accumulates
// the group, which is clipped / faded as a whole when it closes (Scene.render CLIP / OPACITY over a GROUP, S:674-715)
// GRAD (implies GROUPS): the batch contains gradient-painted paths (svgr_batch_set_gradients): their colour is evaluated per
// visible pixel in the composite (Path.fill's gradient branch, S:1021-1047) instead of being a constant of the path
//
// The item loop is a software pipeline over the tile's items (cells, in paint order), all of it plain loads into
// registers -- nothing is staged through LDS but the deltas themselves:
//   item k+3   its header (80 bytes of CellHdr, one dword per lane of ONE load instruction) is requested
//   item k+2   its add list (one 16-byte TileAdd per lane) and, class 1, its carry-ins are requested
//   item k+1   its adds go into delta tile (k+1) & 1 (`ds_add_f64`, fire and forget)
//   item k     delta tile k & 1 is read back to zero, scanned along the rows, and composited
// with ONE barrier per item: behind it every wave's adds of item k have landed and the scan of item k-1 has returned
// its delta tile to zero.  The adds of the next item are in flight in the LDS while this wave's lanes run the composite.
// The float32 production variant keeps its pipeline's load targets in FIXED registers, v[FIX0 .. 127], which the compiler never
// allocates (the kernel is compiled for FIX0 VGPRs; the asm statements' clobber lists bring the count back to 128): a register
// with a load in flight cannot be copied, spilled or recoloured by a compiler that does not have it.  The persistent tile loop
// needs that: with several statements defining one target variable the allocator joins them with copies -- of registers
// whose load has not landed.  (The other variants take one tile per workgroup and keep the targets as ordinary variables.)
#define SVGR_FIX0 116
#define SVGR_FR(k) SVGR_FR_##k
#define SVGR_FR_0 "v116"
#define SVGR_FR_1 "v117"
#define SVGR_FR_2 "v118"
#define SVGR_FR_3 "v119"
#define SVGR_FR_4 "v120"
#define SVGR_FR_5 "v121"
#define SVGR_FR_6 "v122"
#define SVGR_FR_7 "v123"
#define SVGR_FR_8 "v124"
#define SVGR_FR_9 "v125"
#define SVGR_FR_10 "v126"
#define SVGR_FR_11 "v127"
#define SVGR_FP_45 "v[120:121]"
#define SVGR_FP_67 "v[122:123]"
#define SVGR_FP_89 "v[124:125]"
#define SVGR_FP_1011 "v[126:127]"
// The launch's arguments read AGAIN from the kernel-argument segment: scalar loads that hit the scalar cache, in the place of two
// dozen SGPRs held across the item loops (the persistent loop ran out of them).  The pointer passes through an empty asm so that
// the loads stay where they are written; it keeps its address space (constant): through a generic pointer they would be
// VECTOR loads, their results "divergent", and every branch on them an EXEC-masked one.
typedef const TileArgs __attribute__((address_space(4))) * KArgsPtr;
__device__ __forceinline__ void reload_tile_args(TileArgs& A) {
    KArgsPtr ka = (KArgsPtr)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(ka));
    A.pages = ka->pages; A.tile_info = ka->tile_info; A.items = ka->items;
    A.n_ct = ka->n_ct; A.n_bands = ka->n_bands; A.use_order = ka->use_order; A.ct0 = ka->ct0; A.win_ct = ka->win_ct; A.band0 = ka->band0;
    A.win_r = ka->win_r; A.win_c = ka->win_c; A.win_rows = ka->win_rows; A.win_cols = ka->win_cols;
    A.out = ka->out; A.trash = ka->trash;
    A.vr0 = ka->vr0; A.vc0 = ka->vc0; A.vrows = ka->vrows; A.vcols = ka->vcols;
    A.own.rank = ka->own.rank; A.own.world = ka->own.world; A.own.strip = ka->own.strip;
    A.out_cols = ka->out_cols; A.clip01 = ka->clip01;
}
// ... and, in a launch of several windows (k_tile_render_windows), the window's fields in the place of the launch's
typedef const WinTable __attribute__((address_space(4))) * KWinsPtr;
constexpr int WINTABLE_KERNARG_OFFSET = (int)((sizeof(TileArgs) + 7) & ~(size_t)7);   // the second kernel argument
__device__ __forceinline__ void patch_window_args(TileArgs& A, int win) {
    KWinsPtr wt = (KWinsPtr)((const char __attribute__((address_space(4)))*)__builtin_amdgcn_kernarg_segment_ptr() + WINTABLE_KERNARG_OFFSET);
    asm volatile("" : "+s"(wt));
    A.out = wt->w[win].out;
    A.ct0 = wt->w[win].ct0; A.win_ct = wt->w[win].win_ct; A.band0 = wt->w[win].band0; A.n_bands = wt->w[win].n_bands;
    A.win_r = wt->w[win].win_r; A.win_c = wt->w[win].win_c; A.win_rows = wt->w[win].win_rows; A.win_cols = wt->w[win].win_cols;
    A.out_cols = wt->w[win].win_cols;
    A.use_order = 0;
}
template <int OUT, bool CLIP, bool GROUPS, bool GRAD, bool WINS = false>
__device__ __forceinline__ void tile_body(const TileArgs& a, const int win = 0, const unsigned wg0 = 0u) {   // (WINS: window `win` of the launch's table, its first workgroup wg0; `a` = the launch's arguments with the window's fields)
    static_assert(!GROUPS || (CLIP && OUT <= 1), "groups live in the canvas variants with the clip tile");
    constexpr bool FIXED = OUT == 0 && !CLIP;   // the production variant: fixed load targets, persistent tile loop
    static_assert(!GRAD || GROUPS, "gradient entries live in the variant with the large register budget");
    constexpr int OFF_CLIP = 2 * DELTA_BYTES;                                // canvas modes: coverage tile of a clip path
    constexpr int LDS_BYTES = OFF_CLIP + (CLIP ? DELTA_BYTES : 0);
    __shared__ __attribute__((aligned(16))) unsigned char s_mem[LDS_BYTES];
    int clip_tag = -1;  // path whose coverage the clip tile holds (canvas modes)

    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int trow = tid / CH, chunk = tid % CH;
    const int lane_ = lane, trow_ = trow, chunk_ = chunk;
    // ---- which tiles ----
    // A whole-canvas launch is PERSISTENT: the host launches as many workgroups as the chip holds at once and each walks the
    // launch order (k_tile_lists' heaviest-first list of pages) in passes of gridDim.x tiles -- forwards in even passes,
    // backwards in odd ones, so the workgroup that drew the heaviest tile of one pass draws the lightest of the next.  What a
    // (The first two passes are dealt by position; behind them a workgroup draws its next tile from a counter -- one of eight, by
    //  blockIdx % 8, over the tiles of that residue: the launch order is heaviest first, so whoever is free takes the heaviest
    //  tile left.  Dealt by position throughout -- forwards and backwards in turn -- the workgroups' lifetimes spread by a third.)
    // workgroup that lives for ONE tile cannot overlap is a third of its slot's time: the page's round trip, the first
    // headers' and adds' round trip, and the acknowledgement of its stores (a wave ends only when they have come back).
    // Here the next tile's page arrives in the place of the add list of "the item behind the last one" -- a load the pipeline
    // makes anyway and used to point at a dummy --, and a finished tile's canvas is stored BEHIND the next tile's first
    // loads: both are on their way while the composite runs.  (Window launches take one tile per workgroup.)
    int by = 0, bx = 0, item0 = 0, n_items = 0, band = 0;
    int tile_r0 = 0, tile_c0 = 0, tile_c1 = 0;  // absolute row / column of the tile's first pixel, one past its last column
    const unsigned n_tiles_ = (unsigned)a.win_ct * (unsigned)a.n_bands;
    unsigned pass_ = 0u, tile_ = blockIdx.x - wg0;
    unsigned long long page01 = 0ull, page23 = 0ull;  // lane j < PAGE_ITEMS: item j of the tile's list {x, y}, {z, w}; lane PAGE_ITEMS: which tile
    if (a.use_order) {
        const uint4* const pp = a.pages + (size_t)tile_ * PAGE_STRIDE + (lane < PAGE_STRIDE ? lane : PAGE_ITEMS);
        unsigned long long t01, t23;
        asm volatile("global_load_dwordx2 %0, %2, off\n\tglobal_load_dwordx2 %1, %2, off offset:8\n\ts_waitcnt vmcnt(0)"
                     : "=&v"(t01), "=&v"(t23) : "v"(pp) : "memory");
        page01 = t01; page23 = t23;
    }

    double acc[PX][4];
#pragma unroll
    for (int i = 0; i < PX; ++i) acc[i][0] = acc[i][1] = acc[i][2] = acc[i][3] = 0.0;
#ifdef SVGR_DBG_TIMELINE
    const unsigned long long tl_start_ = __builtin_amdgcn_s_memrealtime();
    // sums over the workgroup's tiles: [0] from the end of a tile's items (the launch's start) to the wait for the next tile's
    // first loads, [1] that wait, [2] the item rounds; tl_mark_: the last stamp
    unsigned long long tl_ph_[6] = {0, 0, 0, 0, 0, 0};   // ([3..5]: parts of [0]: registers -> LDS, next tile's loads issued, stores)
    unsigned long long tl_mark_ = tl_start_, tl_sub_ = tl_start_;
#define TL_PHASE(i) do { const unsigned long long now_ = __builtin_amdgcn_s_memrealtime(); tl_ph_[i] += now_ - tl_mark_; tl_mark_ = now_; } while (0)
#else
#define TL_PHASE(i) do { } while (0)
#endif
    // Isolated groups: while one is open its members composite into `gacc`; when an item of another group (or of none)
    // arrives, or the tile's list ends, the group is closed: multiplied by the coverage of its clip path (the clip tile, if
    // that path reached this tile: else the intersection is empty here, S:403-404), by its opacity, and composited OVER
    // the canvas tile -- per pixel the reference's sequence: group layer, `Layer.compose([mask, image], IN)` /
    // `Layer.opacity`, then the parent's OVER (S:674-715).
    double gacc[GROUPS ? PX : 1][4];
    int open_g = -1;
    double* const my0 = (double*)s_mem + trow * ROW_STRIDE + chunk * CHUNK_STRIDE;  // this lane's 8 deltas in delta tile 0
    auto close_group = [&]() {
        if (GROUPS) {
            const int cs = a.group_clip_src[open_g];
            const double al = a.group_opacity[open_g];
            const double* const myclip = my0 + OFF_CLIP / 8;
            const bool have_clip = cs < 0 || clip_tag == cs;
#pragma unroll
            for (int i = 0; i < (GROUPS ? PX : 1); ++i) {
                double s0 = gacc[i][0], s1 = gacc[i][1], s2 = gacc[i][2], s3 = gacc[i][3];
                if (cs >= 0) {
                    const double c = have_clip ? myclip[i] : 0.0;
                    s0 = s0 * c; s1 = s1 * c; s2 = s2 * c; s3 = s3 * c;
                }
                if (al != 1.0) { s0 = s0 * al; s1 = s1 * al; s2 = s2 * al; s3 = s3 * al; }
                over_px(acc[i], s0, s1, s2, s3);
            }
            open_g = -1;
        }
    };

    // (once per workgroup, across the waves: the barrier behind it keeps it off the first transposed tile; between tiles a wave
    //  re-zeroes what its own transposed rows covered)
    for (int i = tid; i < 2 * TR * ROW_STRIDE; i += NT) ((double*)s_mem)[i] = 0.0;
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    if (a.arena_words) {  // nothing in this kernel reads the arena; the geometry kernels that did are finished
        for (unsigned i = 1u + blockIdx.x * NT + tid; i < a.arena_words; i += gridDim.x * NT) a.arena[i] = 0u;
    }

    // ---- the pipeline's loads ----
    // Issued from inline asm and waited for by hand with counted vmcnt: left to the compiler, every load sits in a branch
    // ("is there such an item") and each use waits vmcnt(0) -- three exposed round trips per item.  All of them are
    // unconditional (past the end of the list they read a valid dummy address and the result is discarded), so the queue
    // of outstanding loads is the same in every iteration: [header k+2, adds k+1] at the top of iteration k.
    // A register with a load in flight must not be touched until its wait, and the compiler -- which does not know these
    // are loads -- is free to copy or spill a variable wherever it likes (it did: with the wait written as a read-modify-write
    // of the target it put a v_mov of the target ABOVE the s_waitcnt).  So a load's target variable has exactly two
    // appearances: output of the load statement, input of the statement that waits and moves the landed value into an
    // ordinary variable.  With registers to spare (no spill, no live-range split) the compiler has no reason to touch it in
    // between; profiles/lint_inflight.py checks the generated loop for any other mention of those registers.
    // (Landing the loads in AGPRs instead would hide them from the compiler altogether, but a kernel that mentions AGPRs
    //  gets half its register budget as AGPRs -- 64 VGPRs for a 64-register canvas tile.)
    const void* tail_ptr_ = nullptr;  // this lane's entry of the next tile's page while the tile's last round runs, else a dummy in `trash`
    unsigned cells_v = 0u;  // lane j: item j of the round (cell id | class << 30)
    unsigned add0_v = 0u, nadd_v = 0u;  // ... its add list: first add, adds
    int n_round = 0;        // items of the round
    const int hdr_lane = lane < HDR_LOAD_DWORDS ? lane : HDR_LOAD_DWORDS - 1;
    // header of item j of the round: dword `lane` of its CellHdr (lanes 20 .. 51 hold the 16 carry-ins)
    // (past the end of the round: a dummy in `trash` -- every tile makes these loads, also one whose batch has no cell at all)
    auto hdr_ptr = [&](int j) -> const int* {
        if (j >= n_round) return (const int*)a.trash + hdr_lane;
        const unsigned cw = (unsigned)__builtin_amdgcn_readlane((int)cells_v, j & 63);
        // (class 2: the lanes behind the 20 scalar dwords ask for dword 19 again -- the 128 bytes of carry-ins, which for this class
        //  are in the add list, are neither written nor fetched)
        const int hl = (cw >> 30) == 2u ? (hdr_lane < HDR_DWORDS ? hdr_lane : HDR_DWORDS - 1) : hdr_lane;
        return (const int*)(a.cell_hdr + (cw & 0x3fffffffu)) + hl;
    };
    auto hdr_cls = [&](int h) { return (__builtin_amdgcn_readlane(h, 12) >> 3) & 3; };
    // class 2: this lane's first add of the item (its later ones, for lists longer than the workgroup, are loaded by the
    // scatter); else the list's first entry: any valid address
    // (from the item, not from its header: the adds of an item are asked for together with -- not behind -- its header)
    auto add_ptr = [&](int j) -> const void* {
        // (behind the round's items: the 16 bytes this lane would throw away are its entry of the NEXT tile's page while the tile's
        //  last round runs -- what the loop holds when it ends is the add "of item n + 1" --, a dummy in `trash` otherwise)
        if (j >= n_round) return tail_ptr_;
        const unsigned cw = (unsigned)__builtin_amdgcn_readlane((int)cells_v, j & 63);
        const int n_add = __builtin_amdgcn_readlane((int)nadd_v, j & 63);
        const int add0 = __builtin_amdgcn_readlane((int)add0_v, j & 63);
        const void* p = tail_ptr_;
        if ((cw >> 30) == 2u && n_add > 0) p = a.adds + (size_t)add0 + (tid < n_add ? tid : n_add - 1);
        return p;
    };
    // (class 1) the carry-in of this lane's tile row: dwords 20 + 2 row, 21 + 2 row of the header, fetched across the lanes
    auto carry_of = [&](int h, int trow) -> double {
        const int at = (HDR_DWORDS + 2 * trow) * 4;
        const int lo = __builtin_amdgcn_ds_bpermute(at, h), hi = __builtin_amdgcn_ds_bpermute(at + 4, h);
        return __hiloint2double(hi, lo);
    };
    // (names and clobber lists of the fixed targets; the pairs are even-aligned)
#define hq0_R SVGR_FR(0)
#define hq0_C SVGR_FR(0)
#define hq1_R SVGR_FR(1)
#define hq1_C SVGR_FR(1)
#define hq_R SVGR_FR(2)
#define hq_C SVGR_FR(2)
#define ctr_R SVGR_FR(3)
#define SVGR_WMOV "v_mov_b64"
    typedef unsigned long long addw_t;
#define wq0_R SVGR_FP_45
#define wq0_C SVGR_FR(4), SVGR_FR(5)
#define wq_R SVGR_FP_89
#define wq_C SVGR_FR(8), SVGR_FR(9)
#define vq0_R SVGR_FP_67
#define vq0_C SVGR_FR(6), SVGR_FR(7)
#define vq_R SVGR_FP_1011
#define vq_C SVGR_FR(10), SVGR_FR(11)
    static_assert(SVGR_FIX0 == 512 / WAVES_PER_EU - 12, "the register names above: the top twelve of the budget");
#define SVGR_ADD_NT ""
#define SVGR_HDR_LOAD(tgt, ptr)                                                                                        \
    do {                                                                                                               \
        if constexpr (FIXED) asm volatile("global_load_dword " tgt##_R ", %0, off" : : "v"(ptr) : "memory", tgt##_C);   \
        else asm volatile("global_load_dword %0, %1, off" : "=v"(tgt) : "v"(ptr) : "memory");                           \
    } while (0)
#define SVGR_ADD_LOAD(tw, tv, ptr)                                                                                     \
    do {                                                                                                               \
        if constexpr (FIXED)                                                                                           \
            asm volatile("global_load_dwordx2 " tw##_R ", %0, off" SVGR_ADD_NT "\n\tglobal_load_dwordx2 " tv##_R ", %0, off offset:8" SVGR_ADD_NT \
                         : : "v"(ptr) : "memory", tw##_C, tv##_C);                                                     \
        else                                                                                                           \
            asm volatile("global_load_dwordx2 %0, %2, off" SVGR_ADD_NT "\n\tglobal_load_dwordx2 %1, %2, off offset:8" SVGR_ADD_NT \
                         : "=&v"(tw), "=&v"(tv) : "v"(ptr) : "memory");                                                 \
    } while (0)
    // the wait at a round's start: ALL its first loads (the two headers and the add the first items need; header 2 and add 1, which
    // the loop starts with) -- n = what may stay in flight behind them: the previous tile's stores, or nothing
#define SVGR_STR_(x) #x
#define SVGR_STR(x) SVGR_STR_(x)
#define SVGR_N_STORES 8
#define SVGR_ROUND_TAKE(n, d0, d1, dw0, dv0, d2, dw1, dv1)                                                             \
    do {                                                                                                               \
        if constexpr (FIXED)                                                                                           \
            asm volatile("s_waitcnt vmcnt(" SVGR_STR(n) ")\n\tv_mov_b32 %0, " hq0_R "\n\tv_mov_b32 %1, " hq1_R "\n\t" SVGR_WMOV " %2, " wq0_R "\n\tv_mov_b64 %3, " vq0_R \
                         "\n\tv_mov_b32 %4, " hq_R "\n\t" SVGR_WMOV " %5, " wq_R "\n\tv_mov_b64 %6, " vq_R                 \
                         : "=&v"(d0), "=&v"(d1), "=&v"(dw0), "=&v"(dv0), "=&v"(d2), "=&v"(dw1), "=&v"(dv1) : : "memory"); \
        else                                                                                                           \
            asm volatile("s_waitcnt vmcnt(" SVGR_STR(n) ")\n\tv_mov_b32 %0, %7\n\tv_mov_b32 %1, %8\n\t" SVGR_WMOV " %2, %9\n\tv_mov_b64 %3, %10" \
                         "\n\tv_mov_b32 %4, %11\n\t" SVGR_WMOV " %5, %12\n\tv_mov_b64 %6, %13"                            \
                         : "=&v"(d0), "=&v"(d1), "=&v"(dw0), "=&v"(dv0), "=&v"(d2), "=&v"(dw1), "=&v"(dv1)              \
                         : "v"(hq0), "v"(hq1), "v"(wq0), "v"(vq0), "v"(hq), "v"(wq), "v"(vq) : "memory");                \
    } while (0)
    // the wait at an iteration's end: the header asked for at its start (three items ahead) and the add asked for in front of its
    // composite (two ahead) -- everything this wave has in flight, so nothing is counted
#define SVGR_ITER_TAKE(d2, dw1, dv1)                                                                                   \
    do {                                                                                                               \
        if constexpr (FIXED)                                                                                           \
            asm volatile("s_waitcnt vmcnt(0)\n\tv_mov_b32 %0, " hq_R "\n\t" SVGR_WMOV " %1, " wq_R "\n\tv_mov_b64 %2, " vq_R  \
                         : "=&v"(d2), "=&v"(dw1), "=&v"(dv1) : : "memory");                                             \
        else                                                                                                           \
            asm volatile("s_waitcnt vmcnt(0)\n\tv_mov_b32 %0, %3\n\t" SVGR_WMOV " %1, %4\n\tv_mov_b64 %2, %5"             \
                         : "=&v"(d2), "=&v"(dw1), "=&v"(dv1) : "v"(hq), "v"(wq), "v"(vq) : "memory");                    \
    } while (0)
    // the adds of an item into delta tile `buf`
    auto scatter = [&](int h, addw_t first_w, double first_v, int buf) {
        if (hdr_cls(h) != 2) return;
        if (a.det && wave != 0) return;
        int n_add = __builtin_amdgcn_readlane(h, 13);
        const int add0 = __builtin_amdgcn_readlane(h, 14);
        unsigned char* const base = s_mem + buf * DELTA_BYTES;
        const int i_step = a.det ? 64 : NT;
        auto one = [&](unsigned w, double v) {
            unsigned off = w & 0xffffu;
            __hip_atomic_fetch_add((double*)(base + off), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            // a run: the same value into the next `more` columns -- at most PX - 1, all inside the chunk (k_path_build cuts runs there)
            for (int more = (int)((w >> 16) & 63u); more > 0; --more) {
                off += 8u;
                __hip_atomic_fetch_add((double*)(base + off), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        };
        // The lane's first add is the one the pipeline brought.  Lists longer than the workgroup (rare) load the rest here, issued
        // and waited for by hand: a load the COMPILER sees makes it put `s_waitcnt vmcnt(0)` in front of every scatter's first
        // add -- also of the lists that load nothing --, and that waits for the header requested a moment ago: one exposed
        // memory round trip per item, the pipeline's depth gone.
        if (tid < n_add) one((unsigned)first_w, first_v);
        for (int i = tid + i_step; i < n_add; i += i_step) {
            addw_t w2;
            double v2;
            const TileAdd* const q = a.adds + (size_t)add0 + i;
            asm volatile("global_load_dwordx2 %0, %2, off\n\tglobal_load_dwordx2 %1, %2, off offset:8\n\ts_waitcnt vmcnt(0)"
                         : "=&v"(w2), "=&v"(v2) : "v"(q) : "memory");
            one((unsigned)w2, v2);
        }
    };

    // ---- scan + fill rule + paint + source-over of the item whose deltas are in delta tile `buf` ----
    const int wrow0 = __builtin_amdgcn_readfirstlane(wave) * (64 / CH);  // a wave owns 64 / CH tile rows
    const int wrow0_ = wrow0;
    // the scan's three lane masks as whole scalar pairs, opaque to the compiler: as constants it keeps one half of each and builds
    // the pair again in front of every use (their halves are equal)
    unsigned long long sm1_, sm2_, sm4_;
    {
        constexpr unsigned long long rep = 0x0101010101010101ull;   // one byte per tile row of CH = 8 lanes
        sm1_ = rep * 0xfeull; sm2_ = rep * 0xfcull; sm4_ = rep * 0xf0ull;
        asm volatile("" : "+s"(sm1_), "+s"(sm2_), "+s"(sm4_));
    }
    // (the uniform part of an item's header comes out of the vector load `h` by v_readlane; a scalar load issued an item ahead was
    //  built twice and measured equal: DESIGN section 4)
    auto process = [&](int h, int buf) {
        (void)lane;   // (kept in the closure: without it the header loads' lane clamp compiles to v_min_u32 for v_min_i32 --
                      //  the same values, but no longer the instructions that were measured)
        auto hw = [&](int j) { return __builtin_amdgcn_readlane(h, j); };
        const int bits = hw(12);
        const int cls = (bits >> 3) & 3;
        if (cls == 0) return;
        const int rule = bits & 1, pflags = (bits >> 1) & 3;
        const double p0 = __hiloint2double(hw(1), hw(0));
        const double p1 = __hiloint2double(hw(3), hw(2));
        const double p2 = __hiloint2double(hw(5), hw(4));
        const double p3 = __hiloint2double(hw(7), hw(6));
        const int r0 = hw(8), c0 = hw(9);
        const int rows = hw(10), cols = hw(11);
        const int pid = hw(15);
        const int row_shift = r0 - tile_r0;  // layer row y  -> tile row  y + row_shift
        const int col_shift = c0 - tile_c0;  // layer col x  -> tile col  x + col_shift
        const int lo_c = col_shift < 0 ? -col_shift : 0;             // first layer column inside the tile
        const int hi_c = cols < tile_c1 - c0 ? cols : tile_c1 - c0;  // one past the last
        const int item_g = GROUPS ? __builtin_amdgcn_readlane(h, 16) : -1;  // CellHdr::group
        const int grad_id = GRAD ? (bits >> 5) - 1 : -1;
        const bool grad_mask = GRAD && grad_id >= 0 && a.grads[grad_id].kind == 3 && a.grad_flags[grad_id] != 0;
        if (GROUPS && open_g >= 0 && item_g != open_g) close_group();
        if (GROUPS && item_g >= 0 && open_g < 0) {
            open_g = item_g;
#pragma unroll
            for (int i = 0; i < (GROUPS ? PX : 1); ++i) gacc[i][0] = gacc[i][1] = gacc[i][2] = gacc[i][3] = 0.0;
        }
        const bool is_clip_src = CLIP && (pflags & 1);   // coverage only: becomes the clip of the next path
        const bool is_clipped = CLIP && (pflags & 2);    // multiplied by the coverage of the previous path
        if (is_clip_src) clip_tag = pid;
        // a clipped path whose clip did not reach this tile is invisible here (empty intersection, S:403-404),
        // but its delta rows still have to be read back to zero
        const bool clip_missing = is_clipped && clip_tag != pid - 1;
        // skip the phase when the layer has no row among this wave's (its delta rows are untouched: nothing to read, zero
        // or composite).  A clip source always runs: its coverage tile must be rewritten whole.
        if (!(is_clip_src || (wrow0 + (64 / CH) > row_shift && wrow0 < row_shift + rows))) return;

        double* const my = my0 + buf * (DELTA_BYTES / 8);
        double t[PX];  // the winding number of the lane's pixels (np.cumsum along the row, S:983)
        int c1fast = 0;  // (production variant) class-1 item inside the layer's columns: t[0..4] = 1 - src_a, src
        if (cls == 1) {
            // No record reaches the tile: a row's running sum is its carry-in from the layer's first column in the tile
            // to its last (np.cumsum of zeros).  No delta tile, no prefix sum.
            const double cin1 = carry_of(h, trow);
            int lo_i = lo_c + col_shift - chunk * PX, hi_i = hi_c + col_shift - chunk * PX;
            lo_i = lo_i < 0 ? 0 : lo_i;
            hi_i = hi_i > PX ? PX : hi_i;
            // (a composite loop of its own for this class -- four fmas per pixel instead of eight -- costs 40 VGPRs: the register
            //  allocator does not keep the canvas tile in place across two unrolled loops that both rewrite it)
            if (lo_c + col_shift <= 0 && hi_c + col_shift >= TC) {
                // (the tile lies inside the layer's columns -- the usual case, a tile in the middle of a shape: no pixel tests)
                if (OUT == 0 && !CLIP && PX >= 5) {
                    // The coverage is one value for all of the lane's pixels: src = mask * paint (S:1019) and 1 - src_a once per
                    // lane, then dst = fma(dst, 1 - src_a, src) (S:286) -- four fmas per pixel instead of eight, no comparison.
                    // A row below the cut gets src = 0 and 1 - src_a = 1: dst stays as it is, bit for bit.
                    // The five per-lane values ride in t[0..4] into the pixels' blocks below, which branch on `c1fast` INSIDE
                    // their asm statement: a second C++ loop over the canvas tile makes the register allocator copy the
                    // tile at the join (168 VGPRs and spills), one statement with two bodies does not.
                    const double w = rule ? evenodd_fract_signed(cin1) : cin1;
                    double mval;
                    asm("v_min_f64 %0, |%1|, 1.0" : "=v"(mval) : "v"(w));
                    mval = fabs(w) >= kZeroCut ? mval : 0.0;
                    t[1] = mval * p0; t[2] = mval * p1; t[3] = mval * p2; t[4] = mval * p3;
                    t[0] = 1.0 - t[4];
#pragma unroll
                    for (int i = 5; i < PX; ++i) t[i] = 0.0;
                    c1fast = 1;
                } else {
#pragma unroll
                for (int i = 0; i < PX; ++i) t[i] = cin1;
                }
            } else {
#pragma unroll
                for (int i = 0; i < PX; ++i) t[i] = i >= lo_i && i < hi_i ? cin1 : 0.0;
            }
        } else {
#pragma unroll
            for (int i = 0; i < PX; ++i) t[i] = my[i];
#pragma unroll
            for (int i = 0; i < PX; ++i) my[i] = 0.0;
            double tot = t[0];
#pragma unroll
            for (int i = 1; i < PX; ++i) tot += t[i];
            double inc = tot;  // inclusive scan of the CH chunk totals of this tile row
            // a 16-lane DPP row holds two tile rows: a shift must not carry a value across their border.  The shifted value is
            // added under an EXEC mask (a scalar move on either side of the add) instead of being selected to zero first (two
            // VOP3 v_cndmask per step: a fifth of the scan's vector instructions).  The DPP moves themselves run with every lane
            // enabled: a disabled lane would read as zero on the source side as well.
            double v;
            const unsigned long long exec_all = __builtin_amdgcn_read_exec();   // (all ones: every branch above is wave-uniform)
            const unsigned long long m1 = sm1_, m2 = sm2_, m4 = sm4_;   // (whole scalar pairs made once: see their definition)
#define SVGR_MASKED_ADD(acc_, v_, m_) asm volatile("s_mov_b64 exec, %2\n\tv_add_f64 %0, %0, %1\n\ts_mov_b64 exec, %3" : "+v"(acc_) : "v"(v_), "s"(m_), "s"(exec_all))
            v = dpp_row_shr<1>(inc); SVGR_MASKED_ADD(inc, v, m1);
            v = dpp_row_shr<2>(inc); SVGR_MASKED_ADD(inc, v, m2);
            v = dpp_row_shr<4>(inc); SVGR_MASKED_ADD(inc, v, m4);
            v = dpp_row_shr<1>(inc);  // exclusive: everything left of this chunk (lanes that start a tile row: nothing)
            SVGR_MASKED_ADD(t[0], v, m1);
#pragma unroll
            for (int i = 1; i < PX; ++i) t[i] += t[i - 1];
        }

        if (OUT <= 1) {
            // Canvas: no bounds tests.  Left of / above / below the layer the delta tile is zero and so
            // is the running sum; right of the layer it is NaN (the add list's sentinel) or outside the viewport.
            double* const myclip = my0 + OFF_CLIP / 8;  // same cell of the clip tile
            if (OUT == 0 && !CLIP) {
                // The production variant (float32 canvas, no clip entries), one fused pixel loop per fill rule.
                // Composite for a float32 store: dst += m * (paint - dst * paint_a), two fmas per channel written
                // in place (the same value as src + dst * (1 - src_a) up to double rounding; the double outputs keep
                // the reference's operation order).
                // (the paint's alpha is an operand of every first fma, twice of the fourth: in a VGPR once per item -- left to the
                //  compiler it is moved there from its scalar pair again in every pixel's block)
                double p3v;
                asm("v_mov_b64 %0, %1" : "=v"(p3v) : "s"(p3));
                auto blend = [&](int i, double mval) {
                    double t0, t1, t2, t3;
                    // (the paint's colour channels ride as scalar operands -- one constant-bus read per instruction --, its alpha in a VGPR)
                    asm("v_fma_f64 %0, -%1, %2, %3" : "=v"(t0) : "v"(acc[i][0]), "v"(p3v), "s"(p0));
                    asm("v_fma_f64 %0, -%1, %2, %3" : "=v"(t1) : "v"(acc[i][1]), "v"(p3v), "s"(p1));
                    asm("v_fma_f64 %0, -%1, %2, %3" : "=v"(t2) : "v"(acc[i][2]), "v"(p3v), "s"(p2));
                    asm("v_fma_f64 %0, -%1, %2, %3" : "=v"(t3) : "v"(acc[i][3]), "v"(p3v), "v"(p3v));
                    asm("v_fma_f64 %0, %1, %2, %0" : "+v"(acc[i][0]) : "v"(mval), "v"(t0));
                    asm("v_fma_f64 %0, %1, %2, %0" : "+v"(acc[i][1]) : "v"(mval), "v"(t1));
                    asm("v_fma_f64 %0, %1, %2, %0" : "+v"(acc[i][2]) : "v"(mval), "v"(t2));
                    asm("v_fma_f64 %0, %1, %2, %0" : "+v"(acc[i][3]) : "v"(mval), "v"(t3));
                };
                // the winding per pixel is in t[]: the running sum itself for nonzero (its |.| rides as an operand modifier
                // below), folded for evenodd (already in [0, 1])
                if (rule && !c1fast) {
#pragma unroll
                    for (int i = 0; i < PX; ++i) t[i] = evenodd_fract_signed(t[i]);
                }
                // Then coverage = min(|t|, 1) where |t| >= 1e-6 (S:984-990): the comparison comes first because
                // v_min_f64 turns the NaN of the layer-edge sentinel into 1.0.  Pixels below the cut are skipped
                // under the exec mask: a tenth of the pixel slots of a wave have no visible lane at all.
                // ... as ONE block per pixel: v_cmpx narrows EXEC to the visible lanes, the block runs, a scalar move widens it
                // again -- no saveexec / branch / restore triple per pixel (three quarters of the kernel's scalar instructions),
                // no hole in the vector stream.  (EXEC is all ones here: every branch above is wave-uniform.)
                const double cut = kZeroCut;
                const unsigned long long exec_all = __builtin_amdgcn_read_exec();
#define SVGR_BLEND_PX(i)                                                                                               \
    if constexpr (i < PX) {                                                                                            \
        double t0, t1, t2, t3, mval;                                                                                   \
        unsigned long long vis_;                                                                                       \
        asm volatile(                                                                                                  \
            SVGR_BLEND_C1_HEAD                                                                                         \
            "v_cmpx_ge_f64_e64 %[vis], |%[t]|, %[cut]\n\t"                                                             \
            "v_min_f64 %[m], |%[t]|, 1.0\n\t"                                                                          \
            "v_fma_f64 %[t0], -%[a0], %[pa], %[p0]\n\t"                                                                \
            "v_fma_f64 %[t1], -%[a1], %[pa], %[p1]\n\t"                                                                \
            "v_fma_f64 %[t2], -%[a2], %[pa], %[p2]\n\t"                                                                \
            "v_fma_f64 %[t3], -%[a3], %[pa], %[pa]\n\t"                                                                \
            "v_fma_f64 %[a0], %[m], %[t0], %[a0]\n\t"                                                                  \
            "v_fma_f64 %[a1], %[m], %[t1], %[a1]\n\t"                                                                  \
            "v_fma_f64 %[a2], %[m], %[t2], %[a2]\n\t"                                                                  \
            "v_fma_f64 %[a3], %[m], %[t3], %[a3]\n\t"                                                                  \
            "s_mov_b64 exec, %[all]\n"                                                                                 \
            SVGR_BLEND_C1_TAIL                                                                                         \
            : [a0] "+v"(acc[i < PX ? i : 0][0]), [a1] "+v"(acc[i < PX ? i : 0][1]), [a2] "+v"(acc[i < PX ? i : 0][2]),   \
              [a3] "+v"(acc[i < PX ? i : 0][3]), [t0] "=&v"(t0), [t1] "=&v"(t1), [t2] "=&v"(t2), [t3] "=&v"(t3),          \
              [m] "=&v"(mval), [vis] "=&s"(vis_)                                                                        \
            : [t] "v"(t[i < PX ? i : 0]), [pa] "v"(p3v), [p0] "s"(p0), [p1] "s"(p1), [p2] "s"(p2), [cut] "s"(cut),        \
              [all] "s"(exec_all), [fast] "s"(__builtin_amdgcn_readfirstlane(c1fast)), [k] "v"(t[0]), [s0] "v"(t[1 % PX]), [s1] "v"(t[2 % PX]), [s2] "v"(t[3 % PX]),           \
              [s3] "v"(t[4 % PX])                                                                                       \
            : "scc");                                                                                                  \
    }
                // (the class-1 body sits out of line, behind the kernel's code: `.subsection 1` of the kernel's own section --
                //  the general body runs without a taken branch)
#define SVGR_BLEND_C1_HEAD "s_cmp_lg_u32 %[fast], 0\n\ts_cbranch_scc1 .Lc1f_%=\n\t"
#define SVGR_BLEND_C1_TAIL                                                                                             \
    ".Lc1b_%=:\n\t.subsection 1\n.Lc1f_%=:\n\t"                                                                        \
    "v_fma_f64 %[a0], %[a0], %[k], %[s0]\n\tv_fma_f64 %[a1], %[a1], %[k], %[s1]\n\t"                                    \
    "v_fma_f64 %[a2], %[a2], %[k], %[s2]\n\tv_fma_f64 %[a3], %[a3], %[k], %[s3]\n\t"                                    \
    "s_branch .Lc1b_%=\n\t.subsection 0"
                // two pixels per statement: one class-1 test (and, out of line, one way back) for both
#define SVGR_BLEND_ONE(a0, a1, a2, a3, t)                                                                              \
            "v_cmpx_ge_f64_e64 %[vis], |%[" #t "]|, %[cut]\n\t"                                                         \
            "v_min_f64 %[m], |%[" #t "]|, 1.0\n\t"                                                                      \
            "v_fma_f64 %[t0], -%[" #a0 "], %[pa], %[p0]\n\t"                                                            \
            "v_fma_f64 %[t1], -%[" #a1 "], %[pa], %[p1]\n\t"                                                            \
            "v_fma_f64 %[t2], -%[" #a2 "], %[pa], %[p2]\n\t"                                                            \
            "v_fma_f64 %[t3], -%[" #a3 "], %[pa], %[pa]\n\t"                                                            \
            "v_fma_f64 %[" #a0 "], %[m], %[t0], %[" #a0 "]\n\t"                                                          \
            "v_fma_f64 %[" #a1 "], %[m], %[t1], %[" #a1 "]\n\t"                                                          \
            "v_fma_f64 %[" #a2 "], %[m], %[t2], %[" #a2 "]\n\t"                                                          \
            "v_fma_f64 %[" #a3 "], %[m], %[t3], %[" #a3 "]\n\t"                                                          \
            "s_mov_b64 exec, %[all]\n\t"
#define SVGR_BLEND_FAST(a0, a1, a2, a3)                                                                                \
    "v_fma_f64 %[" #a0 "], %[" #a0 "], %[k], %[s0]\n\tv_fma_f64 %[" #a1 "], %[" #a1 "], %[k], %[s1]\n\t"                \
    "v_fma_f64 %[" #a2 "], %[" #a2 "], %[k], %[s2]\n\tv_fma_f64 %[" #a3 "], %[" #a3 "], %[k], %[s3]\n\t"
#define SVGR_BLEND_2PX(i)                                                                                              \
    {                                                                                                                  \
        double t0, t1, t2, t3, mval;                                                                                   \
        unsigned long long vis_;                                                                                       \
        asm volatile(                                                                                                  \
            "s_cmp_lg_u32 %[fast], 0\n\ts_cbranch_scc1 .Lc1f_%=\n\t"                                                  \
            SVGR_BLEND_ONE(a0, a1, a2, a3, ta)                                                                         \
            SVGR_BLEND_ONE(b0, b1, b2, b3, tb)                                                                         \
            ".Lc1b_%=:\n\t.subsection 1\n.Lc1f_%=:\n\t"                                                              \
            SVGR_BLEND_FAST(a0, a1, a2, a3)                                                                            \
            SVGR_BLEND_FAST(b0, b1, b2, b3)                                                                            \
            "s_branch .Lc1b_%=\n\t.subsection 0"                                                                      \
            : [a0] "+v"(acc[i][0]), [a1] "+v"(acc[i][1]), [a2] "+v"(acc[i][2]), [a3] "+v"(acc[i][3]),                    \
              [b0] "+v"(acc[i + 1][0]), [b1] "+v"(acc[i + 1][1]), [b2] "+v"(acc[i + 1][2]), [b3] "+v"(acc[i + 1][3]),    \
              [t0] "=&v"(t0), [t1] "=&v"(t1), [t2] "=&v"(t2), [t3] "=&v"(t3), [m] "=&v"(mval), [vis] "=&s"(vis_)        \
            : [ta] "v"(t[i]), [tb] "v"(t[i + 1]), [pa] "v"(p3v), [p0] "s"(p0), [p1] "s"(p1), [p2] "s"(p2), [cut] "s"(cut), \
              [all] "s"(exec_all), [fast] "s"(__builtin_amdgcn_readfirstlane(c1fast)), [k] "v"(t[0]), [s0] "v"(t[1]),   \
              [s1] "v"(t[2]), [s2] "v"(t[3]), [s3] "v"(t[4])                                                            \
            : "scc");                                                                                                  \
    }
                static_assert(PX == 8 || PX == 16, "statements of two pixels");
                SVGR_ACC_PX2(SVGR_BLEND_2PX)
#undef SVGR_BLEND_2PX
#undef SVGR_BLEND_ONE
#undef SVGR_BLEND_FAST
#undef SVGR_BLEND_PX
#undef SVGR_BLEND_C1_HEAD
#undef SVGR_BLEND_C1_TAIL
                (void)blend;
            } else {
                bool vis[PX];  // the 1e-6 cut (S:990), as lane masks
                if (rule) {
#pragma unroll
                    for (int i = 0; i < PX; ++i) { t[i] = fill_evenodd_raw(t[i]); vis[i] = t[i] >= kZeroCut; }
                } else {
#pragma unroll
                    for (int i = 0; i < PX; ++i) { t[i] = fill_nonzero_raw(t[i]); vis[i] = t[i] >= kZeroCut; }
                }
                // then one loop for the three kinds of path (three unrolled copies cost 60 VGPRs and an occupancy step):
                //   plain      dst = src OVER dst,  src = mask * paint
                //   clip src   Path.mask of a clip path (S:707): keep its coverage (after the 1e-6 cut) for the next path
                //   clipped    CLIP: (mask * paint) * clip_alpha on the intersection (S:712, S:290), then OVER
#pragma unroll
                for (int i = 0; i < PX; ++i) {
                    const double mval = t[i];
                    if (is_clip_src) {
                        myclip[i] = vis[i] ? mval : 0.0;
                    } else if (vis[i]) {
                        double s0, s1, s2, s3;
                        if (GRAD && grad_id >= 0) {
                            // gradient paint: colour at the pixel centre, times the coverage (canvas_compose(IN, mask, image),
                            // S:1044-1047), times the entry's opacity multiplier (Layer.opacity over the leaf, S:174)
                            double gc[4];
                            grad_colour_pixel(a.grads[grad_id], tile_r0 + trow, tile_c0 + chunk * PX + i, grad_mask, gc);
                            s0 = (gc[0] * mval) * p0; s1 = (gc[1] * mval) * p1; s2 = (gc[2] * mval) * p2; s3 = (gc[3] * mval) * p3;
                        } else {
                            s0 = mval * p0; s1 = mval * p1; s2 = mval * p2; s3 = mval * p3;
                        }
                        if (is_clipped) {
                            const double c = clip_missing ? 0.0 : myclip[i];
                            if (c == 0.0) continue;
                            s0 = s0 * c; s1 = s1 * c; s2 = s2 * c; s3 = s3 * c;
                        }
                        if (GROUPS && item_g >= 0) {
                            over_px(gacc[GROUPS ? i : 0], s0, s1, s2, s3);  // a member of the open group
                        } else if (OUT == 0) {
                            // over_px_fma with the fma written in place (v_fma_f64 acc, acc, k, s): left to the
                            // compiler it becomes v_fmac into the source register plus a v_mov back, 4 moves per pixel
                            const double k1 = 1 - s3;
                            asm("v_fma_f64 %0, %0, %1, %2" : "+v"(acc[i][0]) : "v"(k1), "v"(s0));
                            asm("v_fma_f64 %0, %0, %1, %2" : "+v"(acc[i][1]) : "v"(k1), "v"(s1));
                            asm("v_fma_f64 %0, %0, %1, %2" : "+v"(acc[i][2]) : "v"(k1), "v"(s2));
                            asm("v_fma_f64 %0, %0, %1, %2" : "+v"(acc[i][3]) : "v"(k1), "v"(s3));
                        } else {
                            over_px(acc[i], s0, s1, s2, s3);
                        }
                    }
                }
            }
        } else {
            const int lcols = cols;
            const long long loff = a.layer_off ? a.layer_off[pid] : 0ll;  // where this path's layer starts in `out`
            const int y_layer = trow - row_shift;
            const bool row_ok = y_layer >= 0 && y_layer < rows;
            const int x_layer0 = chunk * PX - col_shift;
#pragma unroll
            for (int i = 0; i < PX; ++i) {
                const int x_layer = x_layer0 + i;
                if (row_ok && x_layer >= lo_c && x_layer < hi_c) {
                    double mval = fill_rule(t[i], rule);
                    if (OUT == 2) {
                        ((double*)a.out)[(size_t)loff + (size_t)y_layer * lcols + x_layer] = mval;
                    } else {
                        double* o = (double*)a.out + 4 * ((size_t)loff + (size_t)y_layer * lcols + x_layer);
                        o[0] = mval * p0; o[1] = mval * p1; o[2] = mval * p2; o[3] = mval * p3;
                    }
                }
            }
        }
    };

    // ---- a finished tile goes out: clip, float32, transposed rows, stores (canvas outputs) ----
    // Returns with its stores in flight.  The float32 variant issues EXACTLY 64 / CH store instructions per wave, every lane
    // enabled (a lane outside the output writes its 16 bytes to `trash`): the counted waits of the next tile's first
    // loads step over them by number.
    auto store_tile_a = [&](const TileArgs& a, int by_, int bx_, int band_) {
        if (OUT > 1) return;
        // (the lane's coordinates pass through an empty asm: what is derived from them below is recomputed per tile instead
        //  of living in registers -- or in scratch -- across the item loops)
        int lane = lane_, trow = trow_, chunk = chunk_, wrow0 = wrow0_;
        asm volatile("" : "+v"(lane), "+v"(trow), "+v"(chunk), "+s"(wrow0));
        // (and the launch's arguments were read again from the kernel-argument segment: reload_tile_args)
        if (a.clip01 && OUT != 0) {
            // clip(0, 1) (S:326) as max / min: two instructions per channel (written as comparisons the compiler turns every
            // channel into two exec-masked branches).  A canvas value is never a NaN (the sentinel's never passes the
            // coverage test), so the NaN rule of v_max does not matter.
#pragma unroll
            for (int i = 0; i < PX; ++i)
#pragma unroll
                for (int q = 0; q < 4; ++q) asm("v_max_f64 %0, %0, 0\n\tv_min_f64 %0, %0, 1.0" : "+v"(acc[i][q]));
        }
        if (OUT == 0) {
            // float32: through an LDS transpose, so that one store instruction covers a whole 1-KiB tile row instead of
            // 64 separate 16-byte pieces 128 bytes apart.  A wave transposes its own rows: no workgroup barrier (the
            // delta tiles are free: the last barrier of the item loop is behind every scan).  Slot = 16 bytes; a lane's 8
            // pixels take 9 slots, so that the 8 lanes a ds_write_b128 serves together fall on different banks.
            constexpr int T_ROW = CH * (PX + 1);  // slots per transposed tile row
            static_assert(TR * T_ROW * 16 <= 2 * DELTA_BYTES, "the transposed tile fits the two delta tiles");
            float4* const tp = (float4*)s_mem;
            if (a.clip01) {
                // clip(0, 1) (S:326) rides on the conversion as its clamp modifier: rounding to float32 is monotone and 0 and 1
                // are float32 values, so clamp(round(x)) == round(clamp(x)) -- and 128 double max / min per wave and tile
                // (as much vector work as one and a half items) are gone
#pragma unroll
                for (int i = 0; i < PX; ++i) {
                    float f0, f1, f2, f3;
                    asm("v_cvt_f32_f64_e64 %0, %1 clamp" : "=v"(f0) : "v"(acc[i][0]));
                    asm("v_cvt_f32_f64_e64 %0, %1 clamp" : "=v"(f1) : "v"(acc[i][1]));
                    asm("v_cvt_f32_f64_e64 %0, %1 clamp" : "=v"(f2) : "v"(acc[i][2]));
                    asm("v_cvt_f32_f64_e64 %0, %1 clamp" : "=v"(f3) : "v"(acc[i][3]));
                    tp[trow * T_ROW + chunk * (PX + 1) + i] = make_float4(f0, f1, f2, f3);
                }
            } else {
#pragma unroll
                for (int i = 0; i < PX; ++i)
                    tp[trow * T_ROW + chunk * (PX + 1) + i] = make_float4((float)acc[i][0], (float)acc[i][1], (float)acc[i][2], (float)acc[i][3]);
            }
        } else {
            const int row = band_ * TR + trow;              // viewport-local row
            const int out_row = by_ * TR + trow - a.win_r;  // row of the output buffer (the window's / the owned bands packed)
            if (row < a.vrows && out_row >= 0 && out_row < a.win_rows) {
                const int col0 = (bx_ - a.ct0) * TC + chunk * PX - a.win_c;  // column of the output buffer
#pragma unroll
                for (int i = 0; i < PX; ++i) {
                    if (col0 + i >= 0 && col0 + i < a.win_cols) {
                        size_t o = (size_t)out_row * a.out_cols + col0 + i;
                        // (plain stores: a lane's pixels are 32 bytes each, 256 bytes from the next lane's -- nontemporal, such pieces
                        //  reach the memory one by one: material-design's tile kernel 0.22 -> 1.75 ms; the L2 merges them)
                        ((double4*)a.out)[o] = make_double4(acc[i][0], acc[i][1], acc[i][2], acc[i][3]);
                    }
                }
            }
        }
    };
    auto store_tile_b = [&](const TileArgs& a, int by_, int bx_, int band_) {
        if (OUT != 0) return;
        int lane = lane_, wrow0 = wrow0_;
        asm volatile("" : "+v"(lane), "+s"(wrow0));
        {
            constexpr int T_ROW = CH * (PX + 1);  // slots per transposed tile row
            float4* const tp = (float4*)s_mem;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            const int col = (bx_ - a.ct0) * TC + lane - a.win_c;  // column of the output buffer this lane stores
            const int orow0 = by_ * TR + wrow0 - a.win_r, vrow0 = band_ * TR + wrow0;   // the wave's first row: of the output / of the viewport
            const int col0 = (bx_ - a.ct0) * TC - a.win_c;
            // (the s_nop behind a store: a store of more than 8 bytes reads its data registers a moment AFTER it issues -- a VALU write
            //  to them in the next cycle lands in the stored value.  The compiler pads its own stores; it does not know these are.)
            // The canvas is written once and not read again by this launch: a NONTEMPORAL store (plain stores pushed the add
            // lists out of the caches the kernel reads them from: 162 -> 132 us).  Issued by hand: the count is what matters.
#define SVGR_ROW_STORE(dst, v) asm volatile("global_store_dwordx4 %0, %1, off nt\n\ts_nop 1" : : "v"(dst), "v"(v) : "memory")
            if (vrow0 + 64 / CH <= a.vrows && orow0 >= 0 && orow0 + 64 / CH <= a.win_rows && col0 >= 0 && col0 + TC <= a.win_cols) {
                // (the wave's rows lie inside the output -- every tile of a canvas whose size is a multiple of the tile's: no tests)
                float4* dst = (float4*)a.out + ((size_t)orow0 * a.out_cols + col);
                // (all the rows out of the LDS first, then the stores: a store statement is a memory barrier to the compiler, and a read
                //  behind each one exposed the LDS latency eight times per tile)
                float4 v4[64 / CH];
#pragma unroll
                for (int r = 0; r < 64 / CH; ++r) v4[r] = tp[(wrow0 + r) * T_ROW + lane + lane / PX];
#pragma unroll
                for (int r = 0; r < 64 / CH; ++r) {
                    const f32x4_t v = {v4[r].x, v4[r].y, v4[r].z, v4[r].w};
                    SVGR_ROW_STORE(dst, v);
                    dst += a.out_cols;
                }
            } else {
                const bool col_ok = col >= 0 && col < a.win_cols;
                float4* const trash = (float4*)a.trash + lane;
#pragma unroll
                for (int r = 0; r < 64 / CH; ++r) {
                    const int tr_ = wrow0 + r;
                    const int vrow = band_ * TR + tr_, orow = by_ * TR + tr_ - a.win_r;
                    const bool ok = vrow < a.vrows && orow >= 0 && orow < a.win_rows && col_ok;
                    const float4 v4 = tp[tr_ * T_ROW + lane + lane / PX];
                    const f32x4_t v = {v4.x, v4.y, v4.z, v4.w};
                    float4* const dst = ok ? (float4*)a.out + ((size_t)orow * a.out_cols + col) : trash;
                    SVGR_ROW_STORE(dst, v);
                }
            }
#undef SVGR_ROW_STORE
            // the wave's transposed rows back to zero: they are delta tiles again (its own LDS operations stay in order; the
            // barrier in front of the next scatter is between this and the other wave's adds)
            {
                constexpr int W_SLOTS = (64 / CH) * T_ROW;  // 16-byte slots of one wave's transposed rows
                float z0 = 0.f;
                asm volatile("" : "+v"(z0));   // (a zero made here: hoisted out of the tile loop it was spilled and reloaded -- behind a vmcnt(0))
                const float4 z = make_float4(z0, z0, z0, z0);
                static_assert(W_SLOTS % 64 == 0, "whole store instructions");
#pragma unroll
                for (int j = 0; j < W_SLOTS / 64; ++j) tp[wrow0 * T_ROW + j * 64 + lane] = z;
            }
        }
    };
    constexpr int N_STORES = 64 / CH;  // store instructions of store_tile<float32> per wave

    // ---- the tiles of this workgroup ----
    int hq0, hq1, hq;                  // load targets: the first two headers of a round, the header in flight in the loop
    addw_t wq0, wq;                    // load targets: the first add of the round's first item / the add in flight ({where, 0})
    double vq0, vq;                    // ... and their values
    (void)hq0; (void)hq1; (void)hq; (void)wq0; (void)wq; (void)vq0; (void)vq;
    unsigned next_tile_ = 0u;
    bool have_next_ = false;
#ifdef SVGR_DBG_TIMELINE
    unsigned long long tl_items_ = 0;
#endif
    // a round's items sit one per lane; its first loads: everything the first two items need, and the loop's standing queue
    // [header 2, add 1], asked for in ONE go (the items carry their add lists, so no load waits for another).  All of them are
    // unconditional: past the end of the list they read a valid dummy address (or the next tile's page: add_ptr).
    auto issue_round = [&](const uint4* pages_, int r0) {
        tail_ptr_ = a.trash;
        if (have_next_ && r0 + n_round >= n_items) {
            int ln = lane_;
            asm volatile("" : "+v"(ln));
            tail_ptr_ = pages_ + (size_t)next_tile_ * PAGE_STRIDE + (ln < PAGE_STRIDE ? ln : PAGE_ITEMS);
        }
        const int* q0 = hdr_ptr(0);
        const int* q1 = hdr_ptr(1);
        const int* q2 = hdr_ptr(2);
        const void* a0 = add_ptr(0);
        const void* a1 = add_ptr(1);
        SVGR_HDR_LOAD(hq0, q0);
        SVGR_HDR_LOAD(hq1, q1);
        SVGR_ADD_LOAD(wq0, vq0, a0);
        SVGR_HDR_LOAD(hq, q2);
        SVGR_ADD_LOAD(wq, vq, a1);
    };
    // the tile `tile_` (its page in page01 / page23): which one, its first round, and that round's loads on their way
    auto begin_tile = [&](const TileArgs& a) {
        int lane = lane_;
        asm volatile("" : "+v"(lane));
        if (a.use_order) {
            by = __builtin_amdgcn_readlane((int)(unsigned)page01, PAGE_ITEMS);  // (ordinal among the owned bands)
            bx = __builtin_amdgcn_readlane((int)(unsigned)(page01 >> 32), PAGE_ITEMS);
            item0 = __builtin_amdgcn_readlane((int)(unsigned)page23, PAGE_ITEMS);
            n_items = __builtin_amdgcn_readlane((int)(unsigned)(page23 >> 32), PAGE_ITEMS);
        } else {
            // (the launch covers the column tiles [ct0, ct0 + win_ct) of the bands [band0, band0 + n_bands): the render window)
            by = __builtin_amdgcn_readfirstlane((int)(tile_ / (unsigned)a.win_ct));
            bx = (int)tile_ - by * a.win_ct + a.ct0;
            const int2 ti = a.tile_info[(size_t)owned_band_at(a.own, by + a.band0) * a.n_ct + bx];
            item0 = __builtin_amdgcn_readfirstlane(ti.x);
            n_items = __builtin_amdgcn_readfirstlane(ti.y);
        }
        band = owned_band_at(a.own, by + a.band0);
        tile_r0 = a.vr0 + band * TR;
        tile_c0 = a.vc0 + bx * TC;
        tile_c1 = tile_c0 + TC;
        clip_tag = -1;
#ifdef SVGR_DBG_TIMELINE
        tl_items_ += (unsigned long long)n_items;
#endif
        // the first round (a whole-canvas launch has the first PAGE_ITEMS items in hand already: its first round is those)
        const int round_cap = a.use_order ? PAGE_ITEMS : 64;
        n_round = n_items < round_cap ? n_items : round_cap;
        if (a.use_order) {
            cells_v = lane < n_round ? (unsigned)page01 : 0u; add0_v = (unsigned)(page01 >> 32); nadd_v = (unsigned)page23;
        } else {
            const uint4 it = lane < n_round ? a.items[(size_t)item0 + lane] : make_uint4(0u, 0u, 0u, 0u);
            cells_v = it.x; add0_v = it.y; nadd_v = it.z;
        }
        // (the fixed-target variant asks for the round's first loads here -- ahead of the previous tile's stores; the others, whose
        //  targets are variables, have ONE statement per target: the one at the top of a round)
        if constexpr (FIXED) issue_round(a.pages, 0);
    };
    // the tile behind the next one: wave 0 asks a counter for it when a tile begins (a returning atomic of ONE lane, its target the
    // fixed register v119, issued in front of the tile's first loads: it has landed when they have), leaves it in an LDS word
    // the tile kernel uses for nothing else (padding of the last delta row) behind the tile's first barrier; both waves read
    // it when the tile ends
    constexpr int MAILBOX = 2 * DELTA_BYTES - 16;
    // (read and written as LDS: through a generic volatile pointer it was a FLAT access with system scope and a wait for every counter)
    typedef volatile __attribute__((address_space(3))) unsigned lds_vu32_t;
    const bool dealt = FIXED && a.use_order && gridDim.x < n_tiles_;   // (a persistent launch)
    const int wave_s = __builtin_amdgcn_readfirstlane(wave);
    bool asked = false;   // a fetch is in flight into v119 (wave 0)
    auto ask_tile = [&]() {
        if constexpr (FIXED) {
            asked = true;
            if (wave_s == 0) {
                unsigned* const ctr = a.tile_ctr + 32 * (blockIdx.x & 7u);
                const unsigned one = 1u;
                unsigned long long keep_;
                asm volatile("s_mov_b64 %[keep], exec\n\ts_mov_b64 exec, 1\n\tglobal_atomic_add " ctr_R ", %[p], %[one], off sc0\n\ts_mov_b64 exec, %[keep]"
                             : [keep] "=&s"(keep_) : [p] "v"(ctr), [one] "v"(one) : "memory", ctr_R);
            }
        }
    };
    if (dealt) {
        if (blockIdx.x == 0 && tid < 8) a.tile_ctr_clear[32 * tid] = 0u;
        next_tile_ = gridDim.x + blockIdx.x;
        have_next_ = next_tile_ < n_tiles_;
        if (have_next_) ask_tile();
    }
    {
        TileArgs a0;
        reload_tile_args(a0);
        if constexpr (WINS) patch_window_args(a0, win);
        begin_tile(a0);
    }
    bool pend = false;   // N_STORES store instructions (the previous tile's canvas) were issued behind the round's first loads
    for (;;) {
#pragma unroll
        for (int i = 0; i < PX; ++i) acc[i][0] = acc[i][1] = acc[i][2] = acc[i][3] = 0.0;
        int h_p, h_s, h_a;            // the landed headers of items k, k+1, k+2
        addw_t w_s;                   // the landed add of the round's first item
        double v_s;
        addw_t w_n;                   // the landed add of item k+1 -- when the tile's last round ends: the next tile's page {x, y}
        double v_n;                   // ... {z, w}
        // ---- the item loop: rounds of up to 64 items ----
        bool preissued = FIXED;   // the tile's first round: begin_tile has issued its loads
        int r0_ = 0;
        do {
            if (!preissued) {
                if (r0_ > 0) {   // (the first round's items: begin_tile)
                    n_round = n_items - r0_ < 64 ? n_items - r0_ : 64;
                    const uint4 it = lane < n_round ? a.items[(size_t)item0 + r0_ + lane] : make_uint4(0u, 0u, 0u, 0u);
                    cells_v = it.x; add0_v = it.y; nadd_v = it.z;
                }
                issue_round(a.pages, r0_);
            }
            const int n = n_round;
            static_assert(N_STORES == SVGR_N_STORES || OUT != 0, "the wait below steps over the previous tile's store instructions");
            if (r0_ == 0) TL_PHASE(0);
            if (preissued && pend) SVGR_ROUND_TAKE(SVGR_N_STORES, h_p, h_s, w_s, v_s, h_a, w_n, v_n);
            else SVGR_ROUND_TAKE(0, h_p, h_s, w_s, v_s, h_a, w_n, v_n);
            if (r0_ == 0) TL_PHASE(1);
            h_p = 0 < n ? h_p : 0;
            h_s = 1 < n ? h_s : 0;
            h_a = 2 < n ? h_a : 0;
            // (first tile: the zero-fill of the delta tiles; later: the previous round's last scans / the re-zeroed transposed rows)
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
            if constexpr (FIXED) {
                if (asked && r0_ == 0) {
                    asked = false;
                    if (wave_s == 0) {
                        unsigned q;
                        asm volatile("v_mov_b32 %0, " ctr_R : "=v"(q) : : "memory");   // (landed: older than the loads the wait above covered)
                        const unsigned t2 = 2u * gridDim.x + 8u * (unsigned)__builtin_amdgcn_readfirstlane((int)q) + (blockIdx.x & 7u);
                        if (tid == 0) *(lds_vu32_t*)(s_mem + MAILBOX) = t2;
                    }
                }
            }
            scatter(h_p, w_s, v_s, 0);
            for (int k = 0; k < n; ++k) {
                // in hand: the headers of items k, k+1, k+2 and the add of item k+1; the adds of item k are on their way into
                // delta tile k & 1
                {
                    const int* q = hdr_ptr(k + 3);
                    SVGR_HDR_LOAD(hq, q);
                }
                // behind this barrier: every wave's adds of item k have landed; everybody's scan of item k-1 has zeroed its tile
                asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
                scatter(h_s, w_n, v_n, (k + 1) & 1);
                {
                    const void* ap = add_ptr(k + 2);
                    SVGR_ADD_LOAD(wq, vq, ap);
                }
                process(h_p, k & 1);
                h_p = h_s; h_s = h_a;
                SVGR_ITER_TAKE(h_a, w_n, v_n);
                h_a = k + 3 < n ? h_a : 0;
            }
            // (nothing is in flight: the last iteration's wait)
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
            preissued = false;
            r0_ += n;
        } while (r0_ < n_items);
        TL_PHASE(2);
        if (GROUPS && open_g >= 0) close_group();
        // ---- on to the next tile: this tile leaves the registers (float32: into LDS), the next tile's first loads go out, and
        // behind them the stores ----
        const int s_by = by, s_bx = bx, s_band = band;
        const bool go = have_next_;
        TileArgs sw;   // (the launch's arguments, read again: reload_tile_args)
        reload_tile_args(sw);
        if constexpr (WINS) patch_window_args(sw, win);
        store_tile_a(sw, s_by, s_bx, s_band);
#ifdef SVGR_DBG_TIMELINE
        { const unsigned long long n_ = __builtin_amdgcn_s_memrealtime(); tl_ph_[3] += n_ - tl_mark_; tl_sub_ = n_; }
#endif
        if (go) {
            page01 = w_n;
            page23 = (unsigned long long)__double_as_longlong(v_n);
            tile_ = (unsigned)__builtin_amdgcn_readfirstlane((int)next_tile_);   // (scalars, said so: the compiler kept them in VGPRs -- and spilled them)
            pass_ = (unsigned)__builtin_amdgcn_readfirstlane((int)(pass_ + 1u));
            next_tile_ = (unsigned)__builtin_amdgcn_readfirstlane((int)*(lds_vu32_t*)(s_mem + MAILBOX));
            have_next_ = next_tile_ < n_tiles_;
            if (have_next_) ask_tile();
            begin_tile(sw);
        }
#ifdef SVGR_DBG_TIMELINE
        { const unsigned long long n_ = __builtin_amdgcn_s_memrealtime(); tl_ph_[4] += n_ - tl_sub_; tl_sub_ = n_; }
#endif
        store_tile_b(sw, s_by, s_bx, s_band);
#ifdef SVGR_DBG_TIMELINE
        { const unsigned long long n_ = __builtin_amdgcn_s_memrealtime(); tl_ph_[5] += n_ - tl_sub_; }
#endif
        if (!go) break;
        pend = OUT == 0;   // (the other outputs stored in front of the loads: their waits cover the stores anyway)
    }

#ifdef SVGR_DBG_TIMELINE
    // per workgroup {start, end, items, XCC | hardware id} on the 100 MHz clock (profiles/timeline.py)
    if (tid == 0 && a.dbg) {
        const unsigned wg_ = blockIdx.x;
        if (wg_ < (1u << 16)) {
            unsigned hwid_, xcc_;
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid_));
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc_));
            unsigned long long* t_ = a.dbg + 8 + 4 * (size_t)wg_;
            t_[0] = tl_start_; t_[1] = __builtin_amdgcn_s_memrealtime(); t_[2] = tl_items_;
            t_[3] = ((unsigned long long)xcc_ << 32) | hwid_;
            unsigned long long* p_ = a.dbg + 8 + 4 * (size_t)(1u << 16) + 4 * (size_t)wg_;
            p_[0] = tl_ph_[0]; p_[1] = tl_ph_[1]; p_[2] = tl_ph_[2]; p_[3] = (unsigned long long)(pass_ + 1u);
            // (the parts of the switch: a third table)
            unsigned long long* q_ = a.dbg + 8 + 8 * (size_t)(1u << 16) + 4 * (size_t)wg_;
            q_[0] = tl_ph_[3]; q_[1] = tl_ph_[4]; q_[2] = tl_ph_[5]; q_[3] = 0ull;
        }
    }
#endif
}

template <int OUT, bool CLIP = false, bool GROUPS = false, bool GRAD = false>
__global__ __launch_bounds__(NT, GROUPS ? 2 : (CLIP ? WAVES_PER_EU - 1 : WAVES_PER_EU)) void k_tile_render(const TileArgs a) {
    tile_body<OUT, CLIP, GROUPS, GRAD>(a);
}
template <>
__global__ __launch_bounds__(NT, WAVES_PER_EU) __attribute__((amdgpu_num_vgpr(SVGR_FIX0 / 2))) void k_tile_render<0, false, false, false>(const TileArgs a) {
    tile_body<0, false, false, false>(a);
}
// the canvas variants drawing several windows (WinTable): the variants a document's runs use -- every one but the production kernel,
// whose launch is persistent and whole-canvas
template <int OUT, bool CLIP = false, bool GROUPS = false, bool GRAD = false>
__global__ __launch_bounds__(NT, GROUPS ? 2 : (CLIP ? WAVES_PER_EU - 1 : WAVES_PER_EU)) void k_tile_render_windows(const TileArgs a, const WinTable wt) {
    static_assert(OUT <= 1, "windows exist in the canvas outputs");
    int w = 0;
#pragma unroll
    for (int step = MAX_WINS / 2; step >= 1; step >>= 1) {   // the last window whose first workgroup is <= this one
        const int c = w + step;
        if (c < wt.n && (unsigned)wt.w[c].tile0 <= blockIdx.x) w = c;
    }
    TileArgs A = a;
    patch_window_args(A, w);
    tile_body<OUT, CLIP, GROUPS, GRAD, true>(A, w, (unsigned)wt.w[w].tile0);
}

// ======================================================================================
// layer kernels (double images in HBM)
// ======================================================================================
// A layer is `ch` (1 or 4) doubles per pixel, row-major over a Box (svgr_box.h).  layer_px is THE read of "the
// pixel of that other layer under device pixel (R, C)": v = its four values, a single channel broadcast to all four; false, and v
// left as it is, where the layer does not reach.  An RGBA pixel goes as two 16-byte loads: a layer begins a pool block, aligned far
// beyond that, and its pixels are 32 bytes apart.  load_px is its second half, the pixel at a known index.
__device__ __forceinline__ void load_px(const double* p, int ch, size_t at, double* v) {
    if (ch == 4) {
        const double2* q = reinterpret_cast<const double2*>(p) + 2 * at;
        const double2 lo = q[0], hi = q[1];
        v[0] = lo.x; v[1] = lo.y; v[2] = hi.x; v[3] = hi.y;
    } else {
        v[0] = v[1] = v[2] = v[3] = p[at];
    }
}
__device__ __forceinline__ bool layer_px(const double* p, int ch, const Box& b, int R, int C, double* v) {
    size_t at;
    if (!box_find(b, R, C, at)) return false;
    load_px(p, ch, at, v);
    return true;
}
// channel c of an RGBA pixel held in registers (feDisplacementMap's channel selectors)
__device__ __forceinline__ double dm_channel(const double4& v, int c) { return c == 0 ? v.x : (c == 1 ? v.y : (c == 2 ? v.z : v.w)); }

// one lane per SOURCE pixel: it goes over (or, `first`, into) the destination pixel under it, where there is one
__global__ void k_layer_over(double* __restrict__ dst, Box db, const double* __restrict__ src, Box sb, int ch, int first) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x, at;
    if (i >= box_px(sb)) return;
    int R, C;
    box_cell(sb, i, R, C);
    if (!box_find(db, R, C, at)) return;
    double* d = dst + 4 * at;
    double s[4];
    load_px(src, ch, i, s);   // (the lane's own pixel)
    if (first) {
        d[0] = s[0]; d[1] = s[1]; d[2] = s[2]; d[3] = s[3];
    } else {
        over_px(d, s[0], s[1], s[2], s[3]);
    }
}

// canvas_compose modes other than OVER / IN (S:287-297) on the full union canvas (canvas_merge_union(full=True),
// S:348-361): out = blend(out, src zero-extended to the canvas), every pixel of the canvas.
//   mode 1 OUT: src * (1 - dst_a)      3 ATOP: src * dst_a + dst * (1 - src_a)      4 XOR: src * (1 - dst_a) + dst * (1 - src_a)
//   mode 5 arithmetic (feComposite k1..k4): clip(k1 * src * dst + k2 * src + k3 * dst + k4, 0, 1)
__global__ void k_layer_blend(double* __restrict__ out, Box ob, const double* __restrict__ src, Box sb, int ch, int mode, double k1,
                              double k2, double k3, double k4) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= box_px(ob)) return;
    int R, C;
    box_cell(ob, i, R, C);
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    layer_px(src, ch, sb, R, C, s);
    double* d = out + 4 * i;
    const double da = d[3], sa = s[3];
    for (int q = 0; q < 4; ++q) {
        const double dv = d[q], sv = s[q];
        double o;
        if (mode == 1) o = sv * (1 - da);
        else if (mode == 3) o = sv * da + dv * (1 - sa);
        else if (mode == 4) o = sv * (1 - da) + dv * (1 - sa);
        else {
            o = k1 * sv * dv + k2 * sv + k3 * dv + k4;
            o = o < 0.0 ? 0.0 : (o > 1.0 ? 1.0 : o);
        }
        d[q] = o;
    }
}

// Layer.color_matrix (S:95-104): image = clip(image @ M[:, :4].T + M[:, 4], 0, 1) on straight-alpha linear RGBA.
// m20 = the 4 x 5 matrix row-major.  np.matmul accumulates k = 0..3 with fused multiply-adds (dgemm).
__global__ void k_layer_color_matrix(double* __restrict__ img, size_t n_px, const double* __restrict__ m20) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_px) return;
    double* p = img + 4 * i;
    const double x0 = p[0], x1 = p[1], x2 = p[2], x3 = p[3];
    for (int q = 0; q < 4; ++q) {
        const double* m = m20 + 5 * q;
        double o = fma(x3, m[3], fma(x2, m[2], fma(x1, m[1], x0 * m[0]))) + m[4];
        p[q] = o < 0.0 ? 0.0 : (o > 1.0 ? 1.0 : o);
    }
}

// Layer.morphology (S:120-127) = min / max pooling with stride 1, no padding (pooling, S:419-468): out is
// (rows - ky + 1, cols - kx + 1, 4), out[R, C] = reduce over src[R .. R+ky-1, C .. C+kx-1].  NaNs are skipped (nanmax).
__global__ void k_layer_morphology(double* __restrict__ out, const double* __restrict__ src, int rows, int cols, int ky, int kx,
                                   int is_max) {
    const int orows = rows - ky + 1, ocols = cols - kx + 1;
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)orows * ocols) return;
    const int R = (int)(i / ocols), C = (int)(i % ocols);
    double a0 = __builtin_nan(""), a1 = a0, a2 = a0, a3 = a0;  // NaN = nothing seen yet (and NaN inputs are skipped: nanmax)
    auto take = [&](double acc, double v) -> double {
        if (v != v) return acc;
        if (acc != acc) return v;
        return is_max ? (v > acc ? v : acc) : (v < acc ? v : acc);
    };
    for (int dy = 0; dy < ky; ++dy) {
        const double4* row = (const double4*)src + ((size_t)(R + dy) * cols + C);
        for (int dx = 0; dx < kx; ++dx) {
            const double4 v = row[dx];
            a0 = take(a0, v.x); a1 = take(a1, v.y); a2 = take(a2, v.z); a3 = take(a3, v.w);
        }
    }
    double acc[4] = {a0, a1, a2, a3};
    double* o = out + 4 * i;
    o[0] = acc[0]; o[1] = acc[1]; o[2] = acc[2]; o[3] = acc[3];
}

// ---- filter primitives the reference does not implement (feTurbulence, feComponentTransfer, feConvolveMatrix,
//      feDisplacementMap; DESIGN.md "Filter primitives beyond the reference") ----

// feTurbulence over the layer `ob`: device pixel (R, C) is the device point (R + 0.5, C + 0.5), taken to user space
// by inv (plain products and sums, left to right) and evaluated by svgr::turb_point.  The lattice (35 KB) is staged in LDS
// once per workgroup and the workgroup strides over many pixels; one double4 store per pixel.
struct TurbLaunch {
    double inv[6];
    svgr::TurbParams p;
    Box ob;
};
__global__ __launch_bounds__(256) void k_layer_turbulence(double* __restrict__ out, const int* __restrict__ sel_g,
                                                          const double* __restrict__ grad_g, TurbLaunch a) {
    __shared__ double grad[svgr::kTurbLattice * 8];
    __shared__ int sel[svgr::kTurbLattice];
    for (int q = threadIdx.x; q < svgr::kTurbLattice * 8; q += blockDim.x) grad[q] = grad_g[q];
    for (int q = threadIdx.x; q < svgr::kTurbLattice; q += blockDim.x) sel[q] = sel_g[q];
    __syncthreads();
    const size_t n = box_px(a.ob);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        int R, C;
        box_cell(a.ob, i, R, C);
        const double d0 = (double)R + 0.5, d1 = (double)C + 0.5;
        const double px = a.inv[0] * d0 + a.inv[1] * d1 + a.inv[2];
        const double py = a.inv[3] * d0 + a.inv[4] * d1 + a.inv[5];
        double c[4];
        svgr::turb_point(sel, grad, a.p, px, py, c);
        reinterpret_cast<double4*>(out)[i] = make_double4(c[0], c[1], c[2], c[3]);
    }
}

// feComponentTransfer in place on straight-alpha RGBA: channel k through svgr::transfer_fn.  blob (staged in LDS) =
// 4 x 5 parameters {slope, intercept, amplitude, exponent, offset}, then the four tables back to back.
struct XferLaunch {
    int type0, type1, type2, type3;
    int n0, n1, n2, n3;
    int off0, off1, off2, off3;
    int n_blob;
};
__global__ __launch_bounds__(256) void k_layer_component_transfer(double* __restrict__ img, size_t n_px, const double* __restrict__ blob_g,
                                                                  XferLaunch a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double* blob = (double*)smem;
    for (int q = threadIdx.x; q < a.n_blob; q += blockDim.x) blob[q] = blob_g[q];
    __syncthreads();
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_px; i += (size_t)gridDim.x * blockDim.x) {
        double4 v = reinterpret_cast<const double4*>(img)[i];
        v.x = svgr::transfer_fn(v.x, a.type0, blob + 0, blob + a.off0, a.n0);
        v.y = svgr::transfer_fn(v.y, a.type1, blob + 5, blob + a.off1, a.n1);
        v.z = svgr::transfer_fn(v.z, a.type2, blob + 10, blob + a.off2, a.n2);
        v.w = svgr::transfer_fn(v.w, a.type3, blob + 15, blob + a.off3, a.n3);
        reinterpret_cast<double4*>(img)[i] = v;
    }
}

// feConvolveMatrix: a T x T workgroup computes a T x T output tile from a (T + oy - 1) x (T + ox - 1) input tile in LDS
// (edge mode applied as it is loaded) and the weights in LDS.  out[R, C] = sum over I (rows, outer), J (cols, inner) of
// src[R - ty + I, C - tx + J] * K[oy - 1 - I][ox - 1 - J], then / divisor + bias.  preserve = 0: all four channels of a
// premultiplied source, alpha clamped to [0, 1] and colour to [0, alpha]; 1: the colours of a straight source clamped to
// [0, 1], alpha copied (svgr::convolve_finish: a NaN sum ends as 0).
struct CmLaunch {
    int rows, cols, ox, oy, tx, ty, edge, preserve, tiles_x;
    double divisor, bias;
};
__global__ __launch_bounds__(256) void k_layer_convolve_matrix(double* __restrict__ out, const double* __restrict__ src,
                                                               const double* __restrict__ w_g, CmLaunch a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int T = blockDim.x;
    const int hr = T + a.oy - 1, hc = T + a.ox - 1;
    double4* tile = (double4*)smem;
    double* w = (double*)(smem + (size_t)hr * hc * sizeof(double4));
    const int tid = threadIdx.y * T + threadIdx.x, nt = T * T;
    for (int q = tid; q < a.ox * a.oy; q += nt) w[q] = w_g[q];
    const int tile_r = (int)blockIdx.x / a.tiles_x, tile_c = (int)blockIdx.x % a.tiles_x;
    const int r0 = tile_r * T - a.ty, c0 = tile_c * T - a.tx;
    const double4* s4 = (const double4*)src;
    for (int q = tid; q < hr * hc; q += nt) {
        int r = r0 + q / hc, c = c0 + q % hc;
        bool inside = true;
        if (a.edge == 0) {          // duplicate
            r = r < 0 ? 0 : (r >= a.rows ? a.rows - 1 : r);
            c = c < 0 ? 0 : (c >= a.cols ? a.cols - 1 : c);
        } else if (a.edge == 1) {   // wrap
            r = ((r % a.rows) + a.rows) % a.rows;
            c = ((c % a.cols) + a.cols) % a.cols;
        } else {                    // none
            inside = r >= 0 && r < a.rows && c >= 0 && c < a.cols;
        }
        tile[q] = inside ? s4[(size_t)r * a.cols + c] : make_double4(0.0, 0.0, 0.0, 0.0);
    }
    __syncthreads();
    const int R = tile_r * T + (int)threadIdx.y, C = tile_c * T + (int)threadIdx.x;
    if (R >= a.rows || C >= a.cols) return;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    for (int I = 0; I < a.oy; ++I) {
        const double4* row = tile + (size_t)(threadIdx.y + I) * hc + threadIdx.x;
        const double* wr = w + (size_t)(a.oy - 1 - I) * a.ox + (a.ox - 1);
        for (int J = 0; J < a.ox; ++J) {
            const double4 v = row[J];
            const double k = wr[-J];
            s0 = s0 + v.x * k;
            s1 = s1 + v.y * k;
            s2 = s2 + v.z * k;
            s3 = s3 + v.w * k;
        }
    }
    double s[4] = {s0, s1, s2, s3};
    svgr::convolve_finish(s, a.divisor, a.bias, a.preserve, a.preserve ? s4[(size_t)R * a.cols + C].w : 0.0);
    reinterpret_cast<double4*>(out)[(size_t)R * a.cols + C] = make_double4(s[0], s[1], s[2], s[3]);
}

// feDisplacementMap: out has the map's box `ob`.  d_user = scale * (map[XC] - 0.5, map[YC] - 0.5) of the straight-alpha map,
// d_dev = L d_user, and the output at device pixel (R, C) is the premultiplied pixel of the source (over `sb`) containing the
// device point (R + 0.5 + d_dev0, C + 0.5 + d_dev1); transparent outside the source.  That point is found in doubles, so the
// kernel keeps a read of its own.
struct DmLaunch {
    Box ob, sb;
    int xc, yc;
    double l00, l01, l10, l11, scale;
};
__global__ __launch_bounds__(256) void k_layer_displacement_map(double* __restrict__ out, const double* __restrict__ map,
                                                                const double* __restrict__ src, DmLaunch a) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= box_px(a.ob)) return;
    int R, C;
    box_cell(a.ob, i, R, C);
    const double4 m = reinterpret_cast<const double4*>(map)[i];
    const double du0 = a.scale * (dm_channel(m, a.xc) - 0.5), du1 = a.scale * (dm_channel(m, a.yc) - 0.5);
    const double dd0 = a.l00 * du0 + a.l01 * du1, dd1 = a.l10 * du0 + a.l11 * du1;
    const double p0 = (double)R + 0.5 + dd0, p1 = (double)C + 0.5 + dd1;
    const double r = floor(p0) - a.sb.r0, c = floor(p1) - a.sb.c0;   // (compared as doubles: a far displacement overflows no int)
    double4 v = make_double4(0.0, 0.0, 0.0, 0.0);
    if (r >= 0.0 && r < (double)a.sb.rows && c >= 0.0 && c < (double)a.sb.cols)
        v = reinterpret_cast<const double4*>(src)[(size_t)r * a.sb.cols + (size_t)c];
    reinterpret_cast<double4*>(out)[i] = v;
}

// feDiffuseLighting / feSpecularLighting over the region `ob`: a 16 x 16 workgroup stages the alpha of its
// tile and a one-pixel halo (18 x 18 doubles, 2.6 KB) in LDS -- zero outside the source and outside the region, so no input
// pixel outside the region is read -- then each lane picks its Sobel case from its place in the region and shades through
// svgr::light_pixel.  One double4 store per pixel; every region pixel is written.
constexpr int kLightTile = 16;
struct LightLaunch {
    svgr::LightParams p;
    Box ob, sb;
    int tiles_x;
};
__global__ __launch_bounds__(256) void k_layer_lighting(double* __restrict__ out, const double* __restrict__ src, LightLaunch a) {
    constexpr int T = kLightTile, H = kLightTile + 2;
    __shared__ double alpha[H * H];
    const int tile_r = (int)blockIdx.x / a.tiles_x, tile_c = (int)blockIdx.x % a.tiles_x;
    const int tid = threadIdx.y * T + threadIdx.x;
    const int r0 = tile_r * T - 1, c0 = tile_c * T - 1;   // (region coordinates of the halo's first pixel)
    for (int q = tid; q < H * H; q += T * T) {
        const int r = r0 + q / H, c = c0 + q % H;
        size_t at;
        double v = 0.0;   // (alpha alone: a load of its own)
        if (r >= 0 && r < a.ob.rows && c >= 0 && c < a.ob.cols && box_find(a.sb, a.ob.r0 + r, a.ob.c0 + c, at)) v = src[at * 4 + 3];
        alpha[q] = v;
    }
    __syncthreads();
    const int R = tile_r * T + (int)threadIdx.y, C = tile_c * T + (int)threadIdx.x;   // (region coordinates)
    if (R >= a.ob.rows || C >= a.ob.cols) return;
    double nb[9];
    for (int k = 0; k < 3; ++k)
        for (int j = 0; j < 3; ++j) nb[3 * k + j] = alpha[((int)threadIdx.y + k) * H + (int)threadIdx.x + j];
    double px[4];
    svgr::light_pixel(a.p, nb, R == 0, R == a.ob.rows - 1, C == 0, C == a.ob.cols - 1, (double)(a.ob.r0 + R) + 0.5, (double)(a.ob.c0 + C) + 0.5, px);
    reinterpret_cast<double4*>(out)[(size_t)R * a.ob.cols + C] = make_double4(px[0], px[1], px[2], px[3]);
}

// mix-blend-mode (svgr::mix_blend_px): every pixel of the window `win` (a box inside out's) gets the
// backdrop (zero outside its box), blended with the source where the source covers it.  Out of place the window is out's whole
// box; in place (out is the backdrop) it is the source's box, and what lies outside it is left as it is.  A 1-channel layer is
// alpha broadcast to all four.  Mode is a template parameter: each instantiation folds its mode's branches away.  One lane per
// pixel, 16-byte loads and stores (two double2 per RGBA pixel).  out and backdrop may be one buffer: each lane reads its
// pixel before it writes it.
struct MixBlendLaunch {
    Box ob, bb, sb, win;   // out, backdrop, source, window
    int bch, sch;
};
template <int MODE>
__global__ __launch_bounds__(256) void k_layer_mix_blend(double* out, const double* backdrop, const double* __restrict__ src,
                                                         MixBlendLaunch a) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= box_px(a.win)) return;
    int R, C;
    box_cell(a.win, i, R, C);
    double d[4] = {0.0, 0.0, 0.0, 0.0}, s[4];
    layer_px(backdrop, a.bch, a.bb, R, C, d);
    if (layer_px(src, a.sch, a.sb, R, C, s)) svgr::mix_blend_px(MODE, d, s);
    double2* o = reinterpret_cast<double2*>(out) + 2 * ((size_t)(R - a.ob.r0) * a.ob.cols + (C - a.ob.c0));   // (the window lies inside out's box)
    o[0] = make_double2(d[0], d[1]);
    o[1] = make_double2(d[2], d[3]);
}
template <int... M>
static decltype(&k_layer_mix_blend<0>) mix_blend_kernel(int mode, std::integer_sequence<int, M...>) {
    decltype(&k_layer_mix_blend<0>) k = nullptr;
    ((k = mode == M ? &k_layer_mix_blend<M> : k), ...);
    return k;
}

// feTile (svgr::tile_wrap / tile_next / tile_source): the output box `ob` filled with repeats of the tile box
// `tb` of the source layer over `sb`, transparent where the tile reaches beyond the layer.  A pure
// copy: every output pixel is written once, nothing is cleared in front.  One lane moves one 16-byte half of an RGBA-f64 pixel
// (a wave's accesses are 1 KiB contiguous in the output, and in the source up to the tile's seam) down kTileRows output rows:
// the column's modulo once per lane, the rows' once per workgroup (uniform: scalar) and a wrapping increment from row to row;
// all loads of a lane are issued before its first store.
constexpr int kTileRows = 8;
struct TileLaunch {
    Box ob, tb, sb;
    int chunks;   // workgroups per output row: ceil(2 * cols / 256)
};
__global__ __launch_bounds__(256) void k_layer_tile(double2* __restrict__ out, const double2* __restrict__ src, TileLaunch a) {
    const int chunk = (int)(blockIdx.x % (unsigned)a.chunks), R0 = (int)(blockIdx.x / (unsigned)a.chunks) * kTileRows;
    const int h = chunk * 256 + (int)threadIdx.x;   // (half pixel h of the row: pixel h / 2, doubles 2 (h % 2) ..)
    if (h >= 2 * a.ob.cols) return;
    const int sc = svgr::tile_source(svgr::tile_wrap(a.ob.c0 - a.tb.c0 + (h >> 1), a.tb.cols), a.tb.c0, a.sb.c0, a.sb.cols);
    int tr = svgr::tile_wrap(a.ob.r0 - a.tb.r0 + R0, a.tb.rows);
    double2 v[kTileRows];
    SVGR_UNROLL
    for (int k = 0; k < kTileRows; ++k) {
        const int sr = svgr::tile_source(tr, a.tb.r0, a.sb.r0, a.sb.rows);
        v[k] = make_double2(0.0, 0.0);
        if (R0 + k < a.ob.rows && sr >= 0 && sc >= 0) v[k] = src[((size_t)sr * a.sb.cols + sc) * 2 + (h & 1)];
        tr = svgr::tile_next(tr, a.tb.rows);
    }
    SVGR_UNROLL
    for (int k = 0; k < kTileRows; ++k)
        if (R0 + k < a.ob.rows) out[(size_t)(R0 + k) * a.ob.cols * 2 + h] = v[k];
}

// luminance mask (S:735): out(1 channel) = (rgb @ [0.2125, 0.7154, 0.072]) * alpha of a straight-alpha layer
__global__ void k_layer_luminance(double* __restrict__ out, const double* __restrict__ src, size_t n_px) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_px) return;
    const double* p = src + 4 * i;
    const double lum = fma(p[2], 0.072, fma(p[1], 0.7154, p[0] * 0.2125));
    out[i] = lum * p[3];
}

__global__ void k_layer_crop4(double* __restrict__ out, Box ob, const double* __restrict__ src, Box sb, int ch) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= box_px(ob)) return;
    int R, C;
    box_cell(ob, i, R, C);
    double v[4] = {0, 0, 0, 0};
    layer_px(src, ch, sb, R, C, v);
    double* o = out + 4 * i;
    o[0] = v[0]; o[1] = v[1]; o[2] = v[2]; o[3] = v[3];
}

__global__ void k_layer_in(double* __restrict__ out, Box ob, const double* __restrict__ src, Box sb, int ch) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= box_px(ob)) return;
    // The one two-layer kernel that keeps a read of its own: with box_find and layer_px its 1-channel row of
    // profiles/bench_layer_ops.py came out 2.4 % slower, with this form it is where it was (profiles/layer_boxes/README.md).
    // Box-relative row and column, the differences taken unsigned so that they wrap where an int would overflow: a wrapped
    // difference is negative or beyond 2^30, outside either way (svgr_box.h, box_find).
    const int R = (int)(i / ob.cols), C = (int)(i % ob.cols);
    const int r = (int)((unsigned)R + (unsigned)ob.r0 - (unsigned)sb.r0), c = (int)((unsigned)C + (unsigned)ob.c0 - (unsigned)sb.c0);
    if (r < 0 || r >= sb.rows || c < 0 || c >= sb.cols) return;
    double* o = out + 4 * i;
    const double* s = src + (size_t)ch * ((size_t)r * sb.cols + c);
    double da = o[3];
    o[0] = s[0] * da;
    o[1] = (ch == 4 ? s[1] : s[0]) * da;
    o[2] = (ch == 4 ? s[2] : s[0]) * da;
    o[3] = (ch == 4 ? s[3] : s[0]) * da;
}

// (dst may be src: in place)
__global__ void k_layer_scale(double* dst, const double* src, size_t n, double f) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = src[i] * f;
}

// ndarray.clip(0, 1) of canvas_merge_at (S:326): np.clip = min(max(v, 0), 1), NaN stays NaN
__global__ void k_layer_clip01(double* __restrict__ img, size_t n) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double v = img[i];
    if (v < 0.0) img[i] = 0.0;
    else if (v > 1.0) img[i] = 1.0;
}

// Layer.background (S:166-169): the image OVER a constant colour, canvas_compose(OVER, colour, image) = image + colour * (1 - a)
__global__ void k_layer_background(double* __restrict__ img, size_t n_px, double c0, double c1, double c2, double c3) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_px) return;
    double4 v = *reinterpret_cast<double4*>(img + 4 * i);
    const double k = 1.0 - v.w;
    v.x = v.x + c0 * k; v.y = v.y + c1 * k; v.z = v.z + c2 * k; v.w = v.w + c3 * k;
    *reinterpret_cast<double4*>(img + 4 * i) = v;
}

// Layer.convert on one RGBA pixel (S:129-164): the ops of svgr_layer_convert, in their order
__device__ __forceinline__ void convert_px(double* v, unsigned ops) {
    if (ops & 1u) {  // premultiplied -> straight, S:471-477 (divide where alpha > 1e-4, then clip all 4)
        double al = v[3];
        for (int c = 0; c < 4; ++c) {
            double x = v[c];
            if (c < 3 && al > 0.0001) x = x / al;
            v[c] = x < 0 ? 0 : (x > 1 ? 1 : x);
        }
    }
    if (ops & 2u)  // sRGB -> linear, S:496-503
        for (int c = 0; c < 3; ++c) v[c] = v[c] <= 0.04045 ? v[c] / 12.92 : pow((v[c] + 0.055) / 1.055, 2.4);
    if (ops & 4u)  // linear -> sRGB, S:486-493
        for (int c = 0; c < 3; ++c) v[c] = v[c] <= 0.0031308 ? v[c] * 12.92 : 1.055 * pow(v[c], 1.0 / 2.4) - 0.055;
    if (ops & 8u)  // straight -> premultiplied, S:480-483
        for (int c = 0; c < 3; ++c) v[c] = v[c] * v[3];
}

// `scale`: Layer.opacity behind the conversion (S:171-175: `convert(pre_alpha=True)`, then image * opacity) in the same pass
template <bool SCALE>
__global__ void k_layer_convert(double* dst, const double* src, size_t n_px, unsigned ops, double f) {   // (dst may be src)
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_px) return;
    double* px = dst + 4 * i;
    const double* sp = src + 4 * i;
    double v[4] = {sp[0], sp[1], sp[2], sp[3]};
    convert_px(v, ops);
    if (SCALE) { v[0] = v[0] * f; v[1] = v[1] * f; v[2] = v[2] * f; v[3] = v[3] * f; }
    px[0] = v[0]; px[1] = v[1]; px[2] = v[2]; px[3] = v[3];
}

// Layer.compose(layers, OVER) in ONE launch (canvas_merge_union, S:366-379 + S:286): every pixel of the union canvas walks the layers
// in their order -- the first is copied where it covers the pixel (S:374-375), the others go OVER what is there (zero outside every
// earlier layer) --, each source converted on the way in (`ops`: the Layer.convert a caller would have run as a pass of its own).
// `accumulate`: the canvas holds the result of an earlier launch over the layers before these (more layers than one table holds).
// Layer.compose(layers, IN) (canvas_merge_intersect, S:382-416 + S:290) is the same walk with another step: the output is the
// intersection of the layers' boxes; the first layer is cropped to it, every other one multiplied by the alpha of what is there --
// out = src * out_alpha, in the layers' order.  A source that does not reach the pixel is skipped (IN: the first stays zero,
// svgr_layer_crop4; the others leave it untouched, svgr_layer_in).
constexpr int OVER_SRCS = 24;
struct OverSrc {
    const double* p;
    Box b;
    int ch;
    unsigned ops;
};
struct OverTable {
    int n, accumulate;
    OverSrc s[OVER_SRCS];
};
template <bool IN>
__global__ __launch_bounds__(256) void k_layer_compose(double* __restrict__ out, Box ob, const OverTable t) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= box_px(ob)) return;
    int R, C;
    box_cell(ob, i, R, C);
    double d[4] = {0.0, 0.0, 0.0, 0.0};
    if (t.accumulate) { const double4 v = ((const double4*)out)[i]; d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w; }
    for (int k = 0; k < t.n; ++k) {
        double v[4];
        if (!layer_px(t.s[k].p, t.s[k].ch, t.s[k].b, R, C, v)) continue;
        if (t.s[k].ch == 4) convert_px(v, t.s[k].ops);
        if (k == 0 && !t.accumulate) { d[0] = v[0]; d[1] = v[1]; d[2] = v[2]; d[3] = v[3]; }
        else if (IN) { const double da = d[3]; d[0] = v[0] * da; d[1] = v[1] * da; d[2] = v[2] * da; d[3] = v[3] * da; }
        else over_px(d, v[0], v[1], v[2], v[3]);
    }
    ((double4*)out)[i] = make_double4(d[0], d[1], d[2], d[3]);
}

__global__ void k_to_f32(float* __restrict__ dst, const double* __restrict__ src, size_t n, int clip01) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double v = src[i];
    if (clip01) v = v < 0 ? 0 : (v > 1 ? 1 : v);
    dst[i] = (float)v;
}

// output stage (canvas_to_png, S:262): np.round(canvas * 255.0).astype(np.uint8), four channels per thread.
// np.round is round-half-to-even = rint in the default rounding mode; values outside [0, 255] (not produced by
// Layer.convert(pre_alpha=False), which clips to [0, 1]) saturate here instead of wrapping.
__global__ void k_to_rgba8(uchar4* __restrict__ dst, const double4* __restrict__ src, size_t n_px) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_px) return;
    const double4 v = src[i];
    auto q = [](double x) -> unsigned char {
        double r = rint(x * 255.0);
        r = r < 0.0 ? 0.0 : (r > 255.0 ? 255.0 : r);
        return (unsigned char)(int)r;  // (NaN -> 0)
    };
    dst[i] = make_uchar4(q(v.x), q(v.y), q(v.z), q(v.w));
}

// does any pixel of the layer have det < 0 ?  (the reference only builds its exclusion mask then, S:1627)
// (two-dimensional launches: block x = 256 columns, block y strides over the rows -- the row / column of a pixel without the
//  64-bit division that a flat index needs per thread)
__global__ __launch_bounds__(256) void k_gradient_detneg(const GradDev g, const double* __restrict__ pts, Box box, int* __restrict__ flag) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= box.cols) return;
    bool neg = false;
    for (int i = blockIdx.y; i < box.rows && !neg; i += gridDim.y) {
        double x, y, b;
        grad_point(g, pts, i, j, box.r0, box.c0, box.cols, x, y);
        neg = grad_focal_det(g, x, y, b) < 0.0;
    }
    if (neg) atomicOr(flag, 1);
}

// Batched form for the gradient entries of a batch: block row y = gradient y; only the focal form (kind 3) has a
// determinant.  The fill's layer = the clipped bbox of its path (device array), like the mask layer of the per-node route.
__global__ __launch_bounds__(256) void k_grad_detneg(const GradDev* __restrict__ grads, const int* __restrict__ grad_path,
                                                    const int* __restrict__ bbox, int* __restrict__ flags) {
    const int gi = blockIdx.y;
    const GradDev& g = grads[gi];
    if (g.kind != 3) return;
    const int4 bb = ((const int4*)bbox)[grad_path[gi]];
    const long long n = (long long)bb.z * bb.w;
    bool neg = false;
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < n && !neg; idx += (long long)gridDim.x * 256) {
        double x, y, b;
        grad_point(g, nullptr, (int)(idx / bb.w), (int)(idx % bb.w), bb.x, bb.y, bb.w, x, y);
        neg = grad_focal_det(g, x, y, b) < 0.0;
    }
    if (__ballot(neg) != 0ull && (threadIdx.x & 63) == 0) atomicOr(&flags[gi], 1);
}

// The parameter block travels as a kernel argument (1.6 KB of kernarg, read with scalar loads): no device copy of it, and
// for linear / plain radial gradients nothing the host would have to wait for.
__global__ __launch_bounds__(256) void k_gradient_fill(const GradDev g, const double* __restrict__ pts, const double* __restrict__ mask,
                                                      Box box, const int* __restrict__ detneg_flag, double* __restrict__ out) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= box.cols) return;
    const bool use_mask = g.kind == 3 && *detneg_flag != 0;
    for (int i = blockIdx.y; i < box.rows; i += gridDim.y) {
        const size_t idx = (size_t)i * box.cols + j;
        double x, y;
        grad_point(g, pts, i, j, box.r0, box.c0, box.cols, x, y);
        double col[4];
        grad_colour_user(g, x, y, use_mask, col);
        const double m = mask ? mask[idx] : 1.0;  // canvas_compose(COMPOSE_IN, mask, image) = image * mask (S:1046, S:290)
        double4 o = make_double4(col[0] * m, col[1] * m, col[2] * m, col[3] * m);
        *reinterpret_cast<double4*>(out + 4 * idx) = o;
    }
}

// --------------------------------------------------------------------------------------
// Path.fill, pattern branch (S:1066-1094): per pixel, the tile offset of the repeated pattern and tile * mask
// --------------------------------------------------------------------------------------
// np.remainder for doubles: C fmod, moved into the divisor's sign range
__device__ __forceinline__ double np_remainder(double a, double b) {
    double m = fmod(a, b);
    if (b == 0.0) return m;
    if (m != 0.0) {
        if ((b < 0.0) != (m < 0.0)) m += b;
    } else {
        m = copysign(0.0, b);
    }
    return m;
}

// One thread per pixel of the mask.  The pixel centre goes to pattern space (inv), is reduced modulo the cell, comes
// back (fwd, no translation) and is truncated like ndarray.astype(int); minus the integer corner minimum that is the
// offset into the (pw, ph) pattern canvas the reference allocates.  That canvas is zero except for the tile merged OVER
// it and clipped to [0, 1] (canvas_merge_at, S:304-327), so it is never built: the tile is read in place.  Negative
// offsets wrap like numpy's; an offset past the canvas (numpy: IndexError) raises the flag.
__global__ void k_pattern_fill(const svgr_pattern pt, const double* __restrict__ tile, const double* __restrict__ mask, Box box,
                               int* __restrict__ oob, double* __restrict__ out) {
    size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= box_px(box)) return;
    const int i = (int)(idx / box.cols), j = (int)(idx % box.cols);
    const double px = (double)i + ((double)box.r0 + 0.5), py = (double)j + ((double)box.c0 + 0.5);
    double ux, uy, tx, ty;
    xform_point(pt.inv_m6, px, py, ux, uy);
    const double rx = np_remainder(ux - pt.cell[0], pt.cell[2]), ry = np_remainder(uy - pt.cell[1], pt.cell[3]);
    xform_point(pt.fwd_m6, rx, ry, tx, ty);
    long long ox = (long long)tx - pt.min_xy[0], oy = (long long)ty - pt.min_xy[1];
    if (ox < 0) ox += pt.pat_shape[0];
    if (oy < 0) oy += pt.pat_shape[1];
    double4 v = make_double4(0.0, 0.0, 0.0, 0.0);
    if (ox < 0 || oy < 0 || ox >= pt.pat_shape[0] || oy >= pt.pat_shape[1] || tx != tx || ty != ty) {
        atomicOr(oob, 1);
    } else {
        const long long lx = ox - pt.tile_bbox[0], ly = oy - pt.tile_bbox[1];
        if (lx >= 0 && ly >= 0 && lx < pt.tile_bbox[2] && ly < pt.tile_bbox[3]) {
            v = *reinterpret_cast<const double4*>(tile + 4 * ((size_t)lx * (size_t)pt.tile_bbox[3] + (size_t)ly));
            v.x = fmin(fmax(v.x, 0.0), 1.0); v.y = fmin(fmax(v.y, 0.0), 1.0);
            v.z = fmin(fmax(v.z, 0.0), 1.0); v.w = fmin(fmax(v.w, 0.0), 1.0);
        }
    }
    const double m = mask[idx];  // canvas_compose(COMPOSE_IN, mask, pattern) = pattern * mask (S:1090, S:290)
    *reinterpret_cast<double4*>(out + 4 * idx) = make_double4(v.x * m, v.y * m, v.z * m, v.w * m);
}

// --------------------------------------------------------------------------------------
// SVG <image> (beyond the reference): the mip chain of an uploaded raster and its per-pixel sampling
// --------------------------------------------------------------------------------------
// level 0: byte / 255, sRGB -> linear (convert_px's formula) if asked, premultiplied, rounded to float32.  The colour of a
// byte takes one of 256 values: each workgroup puts them in LDS once (a pow per entry instead of three per texel) and strides
// over the texels.  256-lane blocks only.
__global__ void __launch_bounds__(256) k_image_prepare(const uchar4* __restrict__ src, size_t n, int linear_rgb,
                                                       float4* __restrict__ dst) {
    __shared__ double lut[256];
    {
        const double t = threadIdx.x / 255.0;
        double v[4] = {t, t, t, 1.0};
        convert_px(v, linear_rgb ? 2u : 0u);
        lut[threadIdx.x] = v[0];
    }
    __syncthreads();
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const uchar4 b = src[i];
        const double a = b.w / 255.0;
        dst[i] = make_float4((float)(lut[b.x] * a), (float)(lut[b.y] * a), (float)(lut[b.z] * a), (float)a);
    }
}

// level k + 1 from level k: the mean of the 2 x 2 parents (the last row / column reused on odd sizes), summed in double
__global__ void k_image_downsample(const float4* __restrict__ src, int h, int w, float4* __restrict__ dst, int dh, int dw) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)dh * dw) return;
    const int r = (int)(i / dw), c = (int)(i % dw);
    const int r0 = 2 * r, c0 = 2 * c, r1 = min(r0 + 1, h - 1), c1 = min(c0 + 1, w - 1);
    const float4 a = src[(size_t)r0 * w + c0], b = src[(size_t)r0 * w + c1];
    const float4 d = src[(size_t)r1 * w + c0], e = src[(size_t)r1 * w + c1];
    dst[i] = make_float4((float)((((double)a.x + b.x) + ((double)d.x + e.x)) * 0.25),
                         (float)((((double)a.y + b.y) + ((double)d.y + e.y)) * 0.25),
                         (float)((((double)a.z + b.z) + ((double)d.z + e.z)) * 0.25),
                         (float)((((double)a.w + b.w) + ((double)d.w + e.w)) * 0.25));
}

// --------------------------------------------------------------------------------------
// JPEG pixel stage (read_jpeg): coefficients -> sample planes -> RGBA.  The arithmetic is svgr_core.h's integer code,
// so the planes and the pixels equal the host build's bit for bit.
// --------------------------------------------------------------------------------------
// The coefficient layout of a frame (include/svgr.h): per component its first block, blocks per row and rows of blocks, and
// where its plane of samples starts (one byte per sample, 8 * bw bytes per row).  False if the frame makes no sense.
struct JpegLayout {
    int64_t base[3], bw[3], bh[3], plane[3];
    int64_t blocks, plane_bytes;
    int cw[3], ch[3], hs[3], vs[3];   // the component's own size in samples; full-resolution pixels per sample
};
static bool jpeg_layout(const svgr_jpeg_frame& f, JpegLayout& L) {
    if ((f.n_comp != 1 && f.n_comp != 3) || f.width < 1 || f.height < 1 || f.width > 65535 || f.height > 65535) return false;
    int hmax = 1, vmax = 1;
    for (int i = 0; i < f.n_comp; ++i) {
        if (f.h[i] < 1 || f.h[i] > 2 || f.v[i] < 1 || f.v[i] > 2) return false;
        hmax = std::max(hmax, (int)f.h[i]);
        vmax = std::max(vmax, (int)f.v[i]);
    }
    if (f.n_comp == 1 && (hmax != 1 || vmax != 1)) return false;
    if (f.n_comp == 1 ? f.colour != SVGR_JPEG_GREY : (f.colour != SVGR_JPEG_YCBCR && f.colour != SVGR_JPEG_RGB)) return false;
    const int64_t mcus_x = (f.width + 8 * hmax - 1) / (8 * hmax), mcus_y = (f.height + 8 * vmax - 1) / (8 * vmax);
    L.blocks = 0;
    for (int i = 0; i < 3; ++i) {
        const int k = i < f.n_comp ? i : 0;   // (a grey frame's unused slots repeat its one component)
        L.hs[i] = hmax / f.h[k];
        L.vs[i] = vmax / f.v[k];
        L.cw[i] = (f.width + L.hs[i] - 1) / L.hs[i];
        L.ch[i] = (f.height + L.vs[i] - 1) / L.vs[i];
        L.bw[i] = mcus_x * f.h[k];
        L.bh[i] = mcus_y * f.v[k];
        if (i < f.n_comp) {
            L.base[i] = L.blocks;
            L.blocks += L.bw[i] * L.bh[i];
        } else {
            L.base[i] = L.base[0];
        }
        L.plane[i] = L.base[i] * 64;
    }
    L.plane_bytes = L.blocks * 64;
    return true;
}

// Dequantise + inverse DCT + level shift + clamp.  Eight lanes per block, 32 blocks per workgroup: lane (block, k) loads row k
// of the block's coefficients and of its quantisation table as 16 bytes each (a wave reads 1 KiB of consecutive
// coefficients), the products go to LDS; lane (block, u) then runs the column pass of column u, lane (block, y) the row pass
// of row y and stores its eight samples as one 8-byte word.  Rows of 72 words keep the four blocks of a half-wave on
// different LDS banks in the column pass.
constexpr int JPEG_WG_BLOCKS = 32, JPEG_LDS_ROW = 72;
struct JpegIdctArgs {
    const int16_t* coef;
    const uint16_t* quant;   // [component][64]
    uint8_t* planes;
    long long end[3];        // one past each component's last block (the components follow each other)
    long long bw[3], plane[3];
};
__global__ void __launch_bounds__(256) k_jpeg_idct(JpegIdctArgs a) {
    __shared__ __attribute__((aligned(16))) int32_t d[JPEG_WG_BLOCKS * JPEG_LDS_ROW];
    __shared__ __attribute__((aligned(16))) int64_t t[JPEG_WG_BLOCKS * JPEG_LDS_ROW];
    const int blk = threadIdx.x >> 3, k = threadIdx.x & 7;
    const long long b = (long long)blockIdx.x * JPEG_WG_BLOCKS + blk;
    const bool live = b < a.end[2];
    const int ci = b < a.end[0] ? 0 : (b < a.end[1] ? 1 : 2);
    if (live) {
        union { uint4 v; int16_t s[8]; } c;
        union { uint4 v; uint16_t s[8]; } q;
        c.v = *reinterpret_cast<const uint4*>(a.coef + b * 64 + 8 * k);
        q.v = *reinterpret_cast<const uint4*>(a.quant + 64 * ci + 8 * k);
        int32_t* row = d + blk * JPEG_LDS_ROW + 8 * k;
#pragma unroll
        for (int j = 0; j < 8; ++j) row[j] = jpeg_dequant(c.s[j], q.s[j]);
    }
    __syncthreads();
    if (live) {   // column k: t[y][k] = sum_v T[y][v] d[v][k]
        int64_t col[8];
        jpeg_idct_pass(d + blk * JPEG_LDS_ROW + k, 8, col);
#pragma unroll
        for (int y = 0; y < 8; ++y) t[blk * JPEG_LDS_ROW + 8 * y + k] = col[y];
    }
    __syncthreads();
    if (live) {   // row k: s[k][x] = sum_u T[x][u] t[k][u]
        int64_t acc[8];
        jpeg_idct_pass(t + blk * JPEG_LDS_ROW + 8 * k, 1, acc);
        union { uint2 v; uint8_t s[8]; } o;
#pragma unroll
        for (int x = 0; x < 8; ++x) o.s[x] = jpeg_sample(acc[x]);
        const long long first = ci == 0 ? 0 : a.end[ci - 1], lb = b - first;
        const long long by = lb / a.bw[ci], bx = lb - by * a.bw[ci];
        *reinterpret_cast<uint2*>(a.planes + a.plane[ci] + (by * 8 + k) * (a.bw[ci] * 8) + bx * 8) = o.v;
    }
}

// Upsampling + colour + alpha: one pixel per lane, a 64 x 4 tile per workgroup, so that a wave writes 256 consecutive bytes
struct JpegColourArgs {
    JpegPlane c[3];
    int width, height, colour;
};
__global__ void __launch_bounds__(256) k_jpeg_colour(JpegColourArgs a, uint32_t* __restrict__ out) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= a.width || y >= a.height) return;
    const int s0 = jpeg_upsampled16(a.c[0], x, y);
    int s1 = s0, s2 = s0;
    if (a.colour != kJpegGrey) {
        s1 = jpeg_upsampled16(a.c[1], x, y);
        s2 = jpeg_upsampled16(a.c[2], x, y);
    }
    out[(size_t)y * a.width + x] = jpeg_rgba(a.colour, s0, s1, s2);
}

// --------------------------------------------------------------------------------------
// JPEG encode stage (write_jpeg): RGBA -> sample planes -> quantised coefficients, svgr_core.h's integer code again.
// --------------------------------------------------------------------------------------
// Colour + chroma downsampling: one lane per H x V group of pixels (the luma sampling factors; chroma has 1 x 1), so the lane
// that read a chroma sample's sources makes it.  A 64 x 4 tile of groups per workgroup: a wave reads 256 (H = 1) or 512
// consecutive bytes per pixel row and writes 64 consecutive bytes per chroma plane.  The planes are padded to whole MCUs:
// the grid covers the padding, whose groups read the image's last column / row (clamped indices).
struct JpegPlanesArgs {
    const uint32_t* rgba;
    uint8_t *y, *cb, *cr;
    int width, height;
    int gw, gh;   // groups per row and rows of groups = the chroma planes' size
    int n_comp;   // 1: Y alone
};
template <int H, int V>
__global__ void __launch_bounds__(256) k_jpeg_planes(JpegPlanesArgs a) {
    const int gx = blockIdx.x * 64 + (threadIdx.x & 63), gy = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (gx >= a.gw || gy >= a.gh) return;
    uint32_t px[H * V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
        const uint32_t* row = a.rgba + (size_t)min(gy * V + j, a.height - 1) * a.width;
        if (H == 2) {
            const int x0 = gx * 2;
            if ((a.width & 1) == 0 && x0 + 1 < a.width) {   // (an even width keeps every pair 8-byte aligned)
                const uint2 p = *reinterpret_cast<const uint2*>(row + x0);
                px[j * H] = p.x;
                px[j * H + H - 1] = p.y;
            } else {
                px[j * H] = row[min(x0, a.width - 1)];
                px[j * H + H - 1] = row[min(x0 + 1, a.width - 1)];
            }
        } else {
            px[j * H] = row[min(gx, a.width - 1)];
        }
    }
    uint8_t y[H * V];
    int cb, cr;
    jpeg_group<H, V>(px, y, &cb, &cr);
    const size_t yw = (size_t)a.gw * H;
#pragma unroll
    for (int j = 0; j < V; ++j) {
        uint8_t* o = a.y + ((size_t)gy * V + j) * yw + (size_t)gx * H;
        if (H == 2) *reinterpret_cast<uchar2*>(o) = make_uchar2(y[j * H], y[j * H + H - 1]);
        else *o = y[j * H];
    }
    if (a.n_comp == 3) {
        a.cb[(size_t)gy * a.gw + gx] = (uint8_t)cb;
        a.cr[(size_t)gy * a.gw + gx] = (uint8_t)cr;
    }
}

// Level shift + forward DCT + quantiser: k_jpeg_idct's counterpart, eight lanes per block, 32 blocks per workgroup.  Lane
// (block, k) loads row k of the block's samples as one 8-byte word, runs the row pass and leaves r[k][0..7] in LDS (int32, rows
// of JPEG_LDS_ROW words as above).  Lane (block, v) then runs the pass down the columns for output row v -- all eight columns at
// once: F[v][u] = sum_y T[y][v] r[y][u], r read as 16-byte words (the eight lanes of a block read the same words: a broadcast;
// the blocks of a lane group are 72 words = 8 banks apart) -- quantises and stores its eight int16 as one 16-byte word: a wave
// writes 1 KiB of consecutive coefficients.  T[.][v] depends on the lane, so the table sits in LDS, transposed.
struct JpegFdctArgs {
    const uint8_t* planes;
    const uint16_t* quant;   // [component][64]
    int16_t* coef;
    long long end[3];        // one past each component's last block (the components follow each other)
    long long bw[3], plane[3];
};
__global__ void __launch_bounds__(256) k_jpeg_fdct(JpegFdctArgs a) {
    __shared__ __attribute__((aligned(16))) int32_t r[JPEG_WG_BLOCKS * JPEG_LDS_ROW];
    __shared__ __attribute__((aligned(16))) int32_t tt[64];   // [v][y] = 2^15 T[y][v]
    const int blk = threadIdx.x >> 3, k = threadIdx.x & 7;
    const long long b = (long long)blockIdx.x * JPEG_WG_BLOCKS + blk;
    const bool live = b < a.end[2];
    const int ci = b < a.end[0] ? 0 : (b < a.end[1] ? 1 : 2);
    if (threadIdx.x < 64) tt[threadIdx.x] = kJpegIdct[8 * (threadIdx.x & 7) + (threadIdx.x >> 3)];
    if (live) {
        const long long first = ci == 0 ? 0 : a.end[ci - 1], lb = b - first;
        const long long by = lb / a.bw[ci], bx = lb - by * a.bw[ci];
        union { uint2 v; uint8_t s[8]; } in;
        in.v = *reinterpret_cast<const uint2*>(a.planes + a.plane[ci] + (by * 8 + k) * (a.bw[ci] * 8) + bx * 8);
        int32_t s[8], row[8];
#pragma unroll
        for (int x = 0; x < 8; ++x) s[x] = (int32_t)in.s[x] - 128;
        jpeg_fdct_pass(s, 1, row);
        int4* o = reinterpret_cast<int4*>(r + blk * JPEG_LDS_ROW + 8 * k);
        o[0] = make_int4(row[0], row[1], row[2], row[3]);
        o[1] = make_int4(row[4], row[5], row[6], row[7]);
    }
    __syncthreads();
    if (live) {
        const int4 t0 = *reinterpret_cast<const int4*>(tt + 8 * k), t1 = *reinterpret_cast<const int4*>(tt + 8 * k + 4);
        const int32_t t[8] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w};
        int64_t acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int y = 0; y < 8; ++y) {
            const int4* p = reinterpret_cast<const int4*>(r + blk * JPEG_LDS_ROW + 8 * y);
            const int4 lo = p[0], hi = p[1];
            const int32_t v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
            for (int u = 0; u < 8; ++u) acc[u] += (int64_t)t[y] * (int64_t)v[u];
        }
        union { uint4 v; uint16_t s[8]; } q;
        union { uint4 v; int16_t s[8]; } o;
        q.v = *reinterpret_cast<const uint4*>(a.quant + 64 * ci + 8 * k);
#pragma unroll
        for (int u = 0; u < 8; ++u) o.s[u] = jpeg_coefficient(acc[u], q.s[u], k == 0 && u == 0);
        *reinterpret_cast<uint4*>(a.coef + b * 64 + 8 * k) = o.v;
    }
}

struct ImageLevel {
    const float4* tex;
    int h, w;
    double scale;  // 2^-k
};

// bilinear at image-space (u, v) of one level: texel centres at + 0.5, clamp to edge.  The corner is clamped in double
// before it becomes an index (svgr::image_corner), so a NaN or huge coordinate lands on the edge, never outside the level.
// Interpolation in the form a + f (b - a): a uniform image gives back its texel exactly.
__device__ __forceinline__ double lerp_d(double a, double b, double f) { return a + f * (b - a); }
__device__ __forceinline__ double4 image_bilinear(const ImageLevel& L, double u, double v) {
    const double x = u * L.scale - 0.5, y = v * L.scale - 0.5;
    const ImageCorner k = image_corner(x, y, L.w, L.h);
    const int c0 = k.c0, c1 = k.c1, r0 = k.r0, r1 = k.r1;
    const double fx = k.fx, fy = k.fy;
    const float4 t00 = L.tex[(size_t)r0 * L.w + c0], t01 = L.tex[(size_t)r0 * L.w + c1];
    const float4 t10 = L.tex[(size_t)r1 * L.w + c0], t11 = L.tex[(size_t)r1 * L.w + c1];
    return make_double4(lerp_d(lerp_d(t00.x, t01.x, fx), lerp_d(t10.x, t11.x, fx), fy),
                        lerp_d(lerp_d(t00.y, t01.y, fx), lerp_d(t10.y, t11.y, fx), fy),
                        lerp_d(lerp_d(t00.z, t01.z, fx), lerp_d(t10.z, t11.z, fx), fy),
                        lerp_d(lerp_d(t00.w, t01.w, fx), lerp_d(t10.w, t11.w, fx), fy));
}

// One lane per output pixel; a 256-lane block covers a 32-column x 8-row tile (a wave: 32 x 2), so that under rotation or
// minification a wave's gathers stay on neighbouring texels.  Row tiles past the grid's height are strided over.  `blend`
// (frac(lod)) > 0: trilinear between `lo` and `hi`; else `lo` alone.  Nearest: the level-0 texel (floor v, floor u).
constexpr int IMG_TW = 32, IMG_TH = 8;
template <bool SMOOTH>
__global__ void __launch_bounds__(256) k_image_fill(const svgr_image im, ImageLevel lo, ImageLevel hi, double blend,
                                                    const double* __restrict__ mask, Box box, double* __restrict__ out) {
    const int j = blockIdx.x * IMG_TW + (threadIdx.x % IMG_TW);
    for (int ti = blockIdx.y; ti * IMG_TH < box.rows; ti += gridDim.y) {
        const int i = ti * IMG_TH + (int)(threadIdx.x / IMG_TW);
        if (i >= box.rows || j >= box.cols) continue;
        const size_t idx = (size_t)i * box.cols + j;
        double u, v;
        xform_point(im.inv_m6, (double)i + ((double)box.r0 + 0.5), (double)j + ((double)box.c0 + 0.5), u, v);
        double4 s;
        if (SMOOTH) {
            s = image_bilinear(lo, u, v);
            if (blend > 0.0) {
                const double4 t = image_bilinear(hi, u, v);
                s = make_double4(lerp_d(s.x, t.x, blend), lerp_d(s.y, t.y, blend), lerp_d(s.z, t.z, blend), lerp_d(s.w, t.w, blend));
            }
        } else {
            double xf, yf;
            image_nearest(u, v, lo.w, lo.h, xf, yf);
            const float4 t = lo.tex[(size_t)(int)yf * lo.w + (int)xf];
            s = make_double4(t.x, t.y, t.z, t.w);
        }
        const double m = mask[idx];  // image * coverage, as every paint of Path.fill
        *reinterpret_cast<double4*>(out + 4 * idx) = make_double4(s.x * m, s.y * m, s.z * m, s.w * m);
    }
}

// --------------------------------------------------------------------------------------
// full 2-D convolution of a (rows, cols, 4) image with a (kw, kh) kernel (Layer.convolve, S:106-118)
// --------------------------------------------------------------------------------------
template <typename KernPtr>
__device__ __forceinline__ void convolve_direct(double* __restrict__ out, const double* __restrict__ src, int rows, int cols,
                                                KernPtr kern, int kw, int kh) {
    const int orows = rows + kw - 1, ocols = cols + kh - 1;
    size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)orows * ocols) return;
    const int R = (int)(idx / ocols), C = (int)(idx % ocols);
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    const int i_lo = R - rows + 1 > 0 ? R - rows + 1 : 0, i_hi = R < kw - 1 ? R : kw - 1;
    const int j_lo = C - cols + 1 > 0 ? C - cols + 1 : 0, j_hi = C < kh - 1 ? C : kh - 1;
    for (int i = i_lo; i <= i_hi; ++i) {
        const double* srow = src + 4 * ((size_t)(R - i) * cols);
        const auto krow = kern + (size_t)i * kh;
        for (int j = j_lo; j <= j_hi; ++j) {
            const double w = krow[j];
            const double* px = srow + 4 * (C - j);
            acc[0] = fma(px[0], w, acc[0]);
            acc[1] = fma(px[1], w, acc[1]);
            acc[2] = fma(px[2], w, acc[2]);
            acc[3] = fma(px[3], w, acc[3]);
        }
    }
    double* o = out + 4 * idx;
    o[0] = acc[0]; o[1] = acc[1]; o[2] = acc[2]; o[3] = acc[3];
}
__global__ void k_layer_convolve(double* __restrict__ out, const double* __restrict__ src, int rows, int cols,
                                 const double* __restrict__ kern, int kw, int kh) {
    convolve_direct(out, src, rows, cols, kern, kw, kh);
}

// One axis of a separable kernel (full convolution along rows or along columns): out = sum_k w[k] * src[.. - k ..].
// AXIS 0: src (rows, cols, 4) -> out (rows + n - 1, cols, 4); AXIS 1: src (rows, cols, 4) -> out (rows, cols + n - 1, 4).
template <int AXIS>
__global__ void k_layer_convolve_1d(double* __restrict__ out, const double* __restrict__ src, int rows, int cols,
                                    const double* __restrict__ w, int n) {
    const int orows = AXIS == 0 ? rows + n - 1 : rows, ocols = AXIS == 1 ? cols + n - 1 : cols;
    size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)orows * ocols) return;
    const int R = (int)(idx / ocols), C = (int)(idx % ocols);
    const int pos = AXIS == 0 ? R : C, len = AXIS == 0 ? rows : cols;
    const int k_lo = pos - len + 1 > 0 ? pos - len + 1 : 0, k_hi = pos < n - 1 ? pos : n - 1;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int k = k_lo; k <= k_hi; ++k) {
        const double wk = w[k];
        const double* px = AXIS == 0 ? src + 4 * ((size_t)(R - k) * cols + C) : src + 4 * ((size_t)R * cols + (C - k));
        acc[0] = fma(px[0], wk, acc[0]);
        acc[1] = fma(px[1], wk, acc[1]);
        acc[2] = fma(px[2], wk, acc[2]);
        acc[3] = fma(px[3], wk, acc[3]);
    }
    double* o = out + 4 * idx;
    o[0] = acc[0]; o[1] = acc[1]; o[2] = acc[2]; o[3] = acc[3];
}

// The same two passes for kernels of up to CONV_TAPS taps per axis (every blur of the configs: 73 at most), blocked so that
// a source pixel is fetched once per block instead of once per tap, with the weights in the kernel argument (no device
// copy of them, nothing for the host to wait for).  Taps are accumulated in ascending k like the plain kernels above.
constexpr int CONV_TAPS = 160;
struct ConvW {
    int n, pad;
    double w[CONV_TAPS];
};
// the direct stencil with a small kernel's weights in the kernel argument (nothing uploaded, nothing for the host to wait for)
__global__ void k_layer_convolve_small(double* __restrict__ out, const double* __restrict__ src, int rows, int cols, const ConvW cw, int kw, int kh) {
    convolve_direct(out, src, rows, cols, (const double*)cw.w, kw, kh);
}
// along a row (AXIS 1): one workgroup = 256 consecutive output columns of one row, the source span staged in LDS -- converted as it
// is staged (`ops`: the Layer.convert the filter runs on its source, S:1803, folded into this pass: a pixel is converted once per
// workgroup that needs it, (256 + n - 1) / 256 times)
__global__ __launch_bounds__(256) void k_convolve_cols(double* __restrict__ out, const double* __restrict__ src, int rows, int cols,
                                                       const ConvW cw, unsigned ops) {
    __shared__ double4 s_px[256 + CONV_TAPS - 1];
    const int n = cw.n, ocols = cols + n - 1;
    const int R = blockIdx.y, C0 = blockIdx.x * 256, tid = threadIdx.x;
    const double4* srow = (const double4*)src + (size_t)R * cols;
    for (int i = tid; i < 256 + n - 1; i += 256) {
        const int c = C0 - (n - 1) + i;  // source column held at s_px[i]
        double4 q = make_double4(0.0, 0.0, 0.0, 0.0);
        if (c >= 0 && c < cols) {
            q = srow[c];
            if (ops) {
                double v[4] = {q.x, q.y, q.z, q.w};
                convert_px(v, ops);
                q = make_double4(v[0], v[1], v[2], v[3]);
            }
        }
        s_px[i] = q;
    }
    __syncthreads();
    const int C = C0 + tid;
    if (C >= ocols) return;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    for (int k = 0; k < n; ++k) {  // out[C] = sum_k w[k] * src[C - k]; (a tap outside the source adds fma(0, w, a) = a)
        const double wk = cw.w[k];
        const double4 px = s_px[tid + (n - 1) - k];
        a0 = fma(px.x, wk, a0); a1 = fma(px.y, wk, a1); a2 = fma(px.z, wk, a2); a3 = fma(px.w, wk, a3);
    }
    ((double4*)out)[(size_t)R * ocols + C] = make_double4(a0, a1, a2, a3);
}
// along a column (AXIS 0): one thread = CONV_RB consecutive output rows of one column; every source pixel of the
// column span is loaded once (coalesced across the threads of a row) and feeds the outputs it reaches.  The loop over the
// source rows is a chain of loads, one per row, in a launch of a few hundred waves: CONV_U of them are asked for together
// (round 5), and the weights are read from an LDS copy padded with CONV_RB zeros on either
// side, so that a tap outside the kernel is a multiplication by zero instead of a branch.
constexpr int CONV_RB = 12;   // (25-tap blur of a 2048x2048 layer: 8 -> 0.180 ms, 12 -> 0.171, 16 -> 0.176, 24 -> 0.203)
constexpr int CONV_U = 6;
__global__ __launch_bounds__(64) void k_convolve_rows(double* __restrict__ out, const double* __restrict__ src, int rows, int cols,
                                                      const ConvW cw) {
    __shared__ double s_w[CONV_TAPS + 2 * CONV_RB + CONV_U];   // (+ CONV_U: the rows asked for beyond the span's first are multiplied too)
    const int n = cw.n, orows = rows + n - 1;
    for (int i = threadIdx.x; i < n + 2 * CONV_RB + CONV_U; i += 64) s_w[i] = i >= CONV_RB && i < CONV_RB + n ? cw.w[i - CONV_RB] : 0.0;
    __syncthreads();
    const int C = blockIdx.x * 64 + threadIdx.x, R0 = blockIdx.y * CONV_RB;
    if (C >= cols) return;
    double acc[CONV_RB][4];
#pragma unroll
    for (int r = 0; r < CONV_RB; ++r) acc[r][0] = acc[r][1] = acc[r][2] = acc[r][3] = 0.0;
    // out[R] = sum_k w[k] * src[R - k]: walking the source rows downwards visits every output's taps in ascending k
    int j_hi = R0 + CONV_RB - 1, j_lo = R0 - (n - 1);
    j_hi = j_hi < rows - 1 ? j_hi : rows - 1;
    j_lo = j_lo > 0 ? j_lo : 0;
    for (int j = j_hi; j >= j_lo; j -= CONV_U) {
        double4 px[CONV_U];
#pragma unroll
        for (int u = 0; u < CONV_U; ++u)
            px[u] = j - u >= j_lo ? ((const double4*)src)[(size_t)(j - u) * cols + C] : make_double4(0.0, 0.0, 0.0, 0.0);
#pragma unroll
        for (int u = 0; u < CONV_U; ++u) {
            // output row R0 + r takes tap k = R0 + r - (j - u) of this source row: s_w[CONV_RB + k] (zero outside 0 .. n - 1)
            const double* const wr = s_w + (CONV_RB + R0 - (j - u));   // (>= s_w + 1; wr[CONV_RB - 1] inside the padded array)
#pragma unroll
            for (int r = 0; r < CONV_RB; ++r) {
                const double wk = wr[r];
                acc[r][0] = fma(px[u].x, wk, acc[r][0]); acc[r][1] = fma(px[u].y, wk, acc[r][1]);
                acc[r][2] = fma(px[u].z, wk, acc[r][2]); acc[r][3] = fma(px[u].w, wk, acc[r][3]);
            }
        }
    }
#pragma unroll
    for (int r = 0; r < CONV_RB; ++r)
        if (R0 + r < orows) ((double4*)out)[(size_t)(R0 + r) * cols + C] = make_double4(acc[r][0], acc[r][1], acc[r][2], acc[r][3]);
}

// ======================================================================================
// batch object
// ======================================================================================
#include "svgr_plan_state.h"   // (host only: the plan-standing flags, the results kept on the device and their transitions)

struct TimedEvents {
    hipEvent_t e0, e1, e2;  // start, before tile kernel, after tile kernel
};

struct svgr_batch {
    svgr_ctx* ctx = nullptr;
    int64_t n_segs = 0, n_paths = 0;
    int vp[4] = {0, 0, 0, 0};
    bool has_vp = false;       // as given by the caller
    double thr = 0.16000000000000003;
    Owner own{0, 1, 1};
    PlanState plan;               // does a plan stand, with which slab order, and which of its passes' results are kept on the device (svgr_plan_state.h)
    bool sized = false;           // a plan has succeeded with the viewport `sized_vp`: the buffers' capacities are a re-plan's guesses
    int sized_vp[4] = {0, 0, 0, 0};
    // SVGR_SAFE_PATH (a test hook, read when a plan is made): the renders take NO place from the plan -- slab places, band-list
    // places, the kept band lists, the lanes' edge places, the cells' add places all come from the device's cursors and a second
    // pass again, as in the staged plan's own passes -- and the round-6 shortcuts of a frame with new geometry are off as well: the
    // one-traversal flatten, k_path_build<2>, svgr_batch_draw's single wait (it plans, then renders).  Each of them was an A/B switch of its own while it was new; they have been
    // bit-identical since (tests/test_gpu_fullsize.py::test_planned_slab_places_do_not_change_the_picture compares the two ends).
    bool safe_path = false;
    void read_switches() {
        safe_path = getenv("SVGR_SAFE_PATH") != nullptr;
        add_places = !safe_path;   // (every planner ends in a full pass: it left every cell's add places)
    }
    bool has_clips = false;    // any SVGR_PATH_CLIP_SOURCE / SVGR_PATH_CLIPPED path
    int64_t n_groups = 0;      // isolated groups (svgr_batch_set_groups)
    DevArr<int> path_group, group_clip_src;
    DevArr<double> group_opacity;
    DevArr<char> groups_dev;   // ... one block holding the three (views), filled by ONE upload
    std::vector<uint8_t> host_rule;  // the paths' rule / flag bytes (checked against the groups)
    int64_t n_grads = 0;       // gradient-painted paths (svgr_batch_set_gradients)
    std::vector<int32_t> host_path_grad;   // ... which path has which (as last set)
    DevArr<GradDev> grads;
    DevArr<int> path_grad, grad_path, grad_flags;
    DevArr<char> grads_dev;    // grads / path_grad / grad_path as views of one block, filled by ONE upload
    bool has_focal = false;
    // inputs
    DevArr<double> segs, path_m6, path_paint;
    DevArr<uint8_t> seg_kind, path_rule;
    DevArr<int> seg_path;
    DevArr<unsigned char> in_dev;  // the one block the six input arrays above are views of
    std::vector<char> in_host;     // its host image, when the context's page-locked staging could not take it: source of the upload, alive as long as the batch
    size_t o_m6 = 0;               // ... where the transforms start in it (svgr_batch_set_transforms)
    // Uploads never make the host wait for the STREAM (a document's walk enqueues one batch after the other and must stay
    // ahead of the device): what an asynchronous copy reads is a host copy kept by the batch, an event marks the last
    // upload enqueued, and only svgr_batch_destroy -- or the next upload into the same array -- waits, for that event alone.
    std::vector<std::vector<char>> host_keep;
    hipEvent_t up_ev = nullptr;
    bool up_pending = false;
    const void* keep(const void* src, size_t n) {
        host_keep.emplace_back((const char*)src, (const char*)src + n);
        return host_keep.back().data();
    }
    hipError_t note_upload(hipStream_t st) {
        if (!up_ev)
            if (hipError_t e = hipEventCreateWithFlags(&up_ev, hipEventDisableTiming); e != hipSuccess) return e;
        up_pending = true;
        return hipEventRecord(up_ev, st);
    }
    void wait_uploads() {
        if (up_pending && up_ev) (void)hipEventSynchronize(up_ev);
        up_pending = false;
        host_keep.clear();
    }
    // zeroed once per render: [BatchDev | per-path min/max keys | per-path row reach (multi-GPU)]
    DevArr<unsigned char> arena;
    size_t arena_bytes = 0, arena_laid = 0, off_pkeys = 0, off_prow = 0, off_scan = 0;
    // work arrays fully rewritten by every render
    DevArr<int> edge_path, bbox, band_start, band_count;
    DevArr<PathBin> bins;
    DevArr<TileEntry> entries;
    DevArr<double> edges;
    DevArr<CellHdr> cell_hdr;               // per (path, band, column tile) cell: header (classes 1 and 2)
    DevArr<unsigned char> work_block;       // a first plan's work arrays in ONE block (two dozen hipMallocs were half of a cold render): the arrays below are then views of it
    DevArr<int2> cell_plan;                 // ... and where its add list lives: {first add, pieces}, left by the plan's full pass (k_path_build)
    bool add_places = false;                // `cell_plan` holds the places of the current plan: the renders take them (k_path_build<1>)
    // a pass that ended with an error flag may have left any of the self-cleaning buffers dirty
    void invalidate_work() { masks_zeroed = false; arena_zeroed = false; plan.pass_failed(); }
    DevArr<TileAdd> adds;                   // the cells' add lists (k_path_build: a slab reserves its cells' lists in one piece)
    DevArr<uint4> items;                    // the tiles' item lists: {cell id | class << 30, first add, adds, 0} (k_tile_lists)
    DevArr<int2> tile_info;                 // per (band, column tile): {first item, items}
    DevArr<uint4> pages;                    // per owned tile, in launch order (heaviest first): its page (k_tile_lists)
    DevArr<int> band_item0;                 // per band: its first item slot
    AddShards add_shards{};                 // where each shard's add slots live (the slabs of path p reserve in shard p % n)
    int64_t n_adds = 0;                     // add slots in all the shards
    bool count_adds_only = false;           // the plan's measuring run: k_path_build sizes the add lists, writes none
    bool adds_roomy = false;                // the add lists were sized by a guess with room for k_path_build<2>'s bounds (not measured exactly by the staged plan)
    bool fl_scan = false;                   // this pass flattens in ONE traversal (k_flatten<.., SCAN>): a re-plan's single pass
    bool late_scan = false;                 // the counting pass leaves k_seg_scan to its caller (two_pass_issue: behind the census's read-back)
    bool census_bbox = false;               // the two-pass plan's first pass: the counting flatten is followed by k_path_bbox (pairs, cells, slabs counted)
    bool deterministic = false;             // this pass runs for a SVGR_RENDER_DETERMINISTIC render
    // lay the add shards back to back: `need[k]` slots each plus slack (the sizes repeat from render to render except for
    // carry-ins that are exactly zero in one summation order and not in another)
    int size_adds(const int* need, int n_shards) {
        if (int rc = layout_adds(need, n_shards)) return rc;
        return adds.ensure((size_t)std::max<int64_t>(n_adds, 1));
    }
    int layout_adds(const int* need, int n_shards) {
        long long at = 0;
        add_shards.n = n_shards;
        for (int k = 0; k < NSH; ++k) {
            const long long cap = k < n_shards ? (long long)need[k] + need[k] / 8 + 256 : 0;
            add_shards.base[k] = (int)std::min<long long>(at, 0x7fffffff);
            add_shards.cap[k] = (int)std::min<long long>(cap, 0x7fffffff);
            at += cap;
        }
        if (at > 0x7fffffffll) return fail(SVGR_E_OVERFLOW, "%lld add slots: beyond the 32-bit add index (split the batch)", at);
        n_adds = at;
        return 0;
    }
    DevArr<int> pair_idx;                   // per (path, band) pair: its place in its band's list (k_band_entries)
    DevArr<Slab> slabs;                     // work items of k_path_build (k_path_bbox)
    DevArr<int> slab_at;                    // per path: its first slab, heaviest paths first (staged plan; renders only)
    unsigned long long stale_word = 0ull;   // SVGR_DBG_STALE_BAND: source of the one-word upload (alive until the stream has taken it)
    std::vector<int> slab_at_host;
    int64_t n_slabs = 0;                    // ... the plan's count = the launch's grid
    DevArr<int> seg_cnt, seg_off;           // per segment: edges it flattens into (the plan's counting pass), their prefix sums
    int fl_sub = FL_SUB;                    // log2 of the lanes k_flatten cuts a segment over (5, or 6 when the launch does not fill the chip: run_geometry)
    DevArr<int> lane_off;                   // per (segment, lane of its 2^fl_sub): the lane's first edge inside the segment's slots (same pass)
    DevArr<int> path_seg0;                  // per path its first segment (view of the input blob)
    DevArr<int> seg_list;                   // multi-GPU: the segments this rank flattens (k_seg_select, at plan time)
    int64_t n_seg_list = -1;                // (-1: no list, every segment)
    DevArr<int> path_list;                  // ... and the paths they belong to, ascending: what k_path_bbox / k_band_entries walk
    int64_t n_path_list = 0;
    DevArr<unsigned long long> tile_mask;   // per (band, column tile): 2 x mask_words words over the band's list (k_path_build)
    DevArr<unsigned long long> tile_mask_kept;   // same layout: the words the lists in place were made from (k_tile_lists, placed replays)
    int mask_words = 1;
    bool masks_zeroed = false;              // the last tile kernel left the masks cleared
    DevArr<long long> layer_off;            // SVGR_OUT_MASKS_F64: per path the start of its mask in the output
    std::vector<long long> host_layer_off;
    // plan results (n_edges = edge slots the edge kernels cover = sum of the shard capacities; n_edges_live = filled ones)
    bool geometry_fresh = false;  // the buffers hold the geometry of the current inputs (set by plan, consumed by render)
    bool geometry_current = false;  // ... and still do: no input has changed since the last geometry pass (SVGR_RENDER_SAME_GEOMETRY)
    bool arena_zeroed = false;    // the last tile kernel left the counter arena zeroed (all but the error word)
    int64_t n_edges_live = 0;
    int64_t n_edges = 0, n_pb = 0, n_bsegs = 0, n_cells = 0, n_entries = 0;
    int n_bands = 0;
    BatchDev host_bd{};
    EdgeShards shards{};       // plan result: where each flatten shard's edges live
    std::vector<int> host_bbox;
    bool host_bbox_stale = false;   // svgr_batch_draw's re-plan left the bboxes on the device: fetched when somebody asks (ensure_host_bbox)
    bool defer_bbox = false;        // ... this pass's read-back is the scalars alone
    std::vector<TimedEvents> events;
    std::vector<hipEvent_t> event_pool;
    // Hit testing (svgr_batch_winding / svgr_batch_pick): every flattened edge of the batch grouped by path, the paths' places in
    // that block and their extents {min a, min b, max a, max b}.  Made by the first query, kept until the transforms change; in
    // arrays of its own, so a plan the batch has is not touched.
    DevArr<double> hit_edges, hit_ext;
    DevArr<int> hit_off;
    bool hit_ready = false;

    int n_ctiles() const { return (vp[3] + TC - 1) / TC; }
    // the arrays k_tile_lists fills, for the planned band / tile / cell counts
    int size_tile_lists(int owned_bands) {
        const size_t nt = (size_t)std::max(n_bands, 1) * (size_t)std::max(n_ctiles(), 1);
        if (int rc = tile_info.ensure(nt)) return rc;
        if (int rc = pages.ensure((size_t)std::max(owned_bands, 1) * (size_t)std::max(n_ctiles(), 1) * PAGE_STRIDE)) return rc;
        if (int rc = band_item0.ensure((size_t)n_bands + 1)) return rc;
        return items.ensure((size_t)std::max<int64_t>(n_cells, 1));
    }
    size_t mask_bytes() const { return sizeof(unsigned long long) * 2 * (size_t)mask_words * (size_t)n_bands * (size_t)n_ctiles(); }
    // size the tiles' entry bitmasks for band lists of up to `longest` entries
    int size_masks(int64_t longest) {
        mask_words = (int)std::max<int64_t>((longest + 63) / 64, 1);
        masks_zeroed = false;
        plan.masks_resized();
        if (int rc = tile_mask_kept.ensure(mask_bytes() / sizeof(unsigned long long) + 1)) return rc;
        return tile_mask.ensure(mask_bytes() / sizeof(unsigned long long) + 1);
    }
    // Two sets of device scalars at the head of the arena: the passes and the renders count into the first (its first word is the
    // sticky error word), the two-pass plan's CENSUS into the second -- so the pass behind the census finds the first set still
    // zero and needs no memset launch in between (4-5 us each: a cold frame had four).
    bool census_set = false;
    BatchDev* bd() const { return (BatchDev*)arena.p + (census_set ? 1 : 0); }
    unsigned long long* pkeys() const { return (unsigned long long*)(arena.p + off_pkeys); }
    unsigned* prow() const { return (unsigned*)(arena.p + off_prow); }
    unsigned long long* scan_state() const { return (unsigned long long*)(arena.p + off_scan); }   // k_flatten<.., SCAN>: one word per workgroup

    int layout_arena() {
        off_pkeys = 2 * sizeof(BatchDev);
        off_prow = off_pkeys + sizeof(unsigned long long) * 4 * (size_t)n_paths;
        off_scan = (off_prow + sizeof(unsigned) * 2 * (size_t)n_paths + 7) & ~(size_t)7;
        arena_bytes = off_scan + sizeof(unsigned long long) * (((size_t)n_segs << 6) / FL_BLOCK + 2);   // (workgroups of the widest cut: 64 lanes per segment)
        arena_bytes = (arena_bytes + 255) & ~(size_t)255;
        const unsigned char* const before = arena.p;
        const size_t bytes_before = arena_laid;
        const int rc = arena.ensure(arena_bytes);
        if (arena.p != before || bytes_before != arena_bytes) arena_zeroed = false;  // (new size or new memory; else what the last tile kernel left stands)
        arena_laid = arena_bytes;
        return rc;
    }

    // (the device arrays free themselves)
    ~svgr_batch() {
        for (auto& t : events) { (void)hipEventDestroy(t.e0); (void)hipEventDestroy(t.e1); (void)hipEventDestroy(t.e2); }
        for (auto e : event_pool) (void)hipEventDestroy(e);
        if (up_ev) (void)hipEventDestroy(up_ev);
    }
};

// The work arrays of the last LARGE batch destroyed on a context, kept for the next batch made for the same viewport: a caller that
// draws frame after frame from new batches (the reference's model: every call starts from the geometry, S:948-957) then plans its
// frame like a re-plan -- ONE pass on the inherited CAPACITIES, flagged and planned in two passes when they do not hold -- instead of
// a census, a host wait and a sizing step.  Nothing of the old batch's geometry or results is read: every array is rewritten by the
// pass before anything reads it (the entry bitmasks are cleared again), and the counter arena is the new batch's own.
struct WorkSpare {
    int vp[4] = {0, 0, 0, 0};
    int64_t n_segs = 0, n_paths = 0;
    int mask_words = 1;
    AddShards add_shards{};
    int64_t n_adds = 0;
    bool adds_roomy = false;
    DevArr<int> edge_path, band_start, band_count, pair_idx, slab_at, seg_cnt, seg_off, lane_off, band_item0;
    DevArr<TileEntry> entries;
    DevArr<double> edges;
    DevArr<CellHdr> cell_hdr;
    DevArr<unsigned char> work_block;
    DevArr<int2> cell_plan, tile_info;
    DevArr<TileAdd> adds;
    DevArr<uint4> items, pages;
    DevArr<Slab> slabs;
    DevArr<unsigned long long> tile_mask, tile_mask_kept;
};
#define SVGR_SPARE_ARRAYS(X) X(edge_path) X(band_start) X(band_count) X(pair_idx) X(slab_at) X(seg_cnt) X(seg_off) X(lane_off) X(band_item0) \
    X(entries) X(edges) X(cell_hdr) X(work_block) X(cell_plan) X(tile_info) X(adds) X(items) X(pages) X(slabs) X(tile_mask) X(tile_mask_kept)
// a destroyed batch leaves its work arrays to its context (large planned batches with a viewport on one GPU only)
static void spare_stash(svgr_batch* b) {
    svgr_ctx* c = b->ctx;
    if (!b->sized || !b->has_vp || b->own.world > 1 || b->n_segs <= 4096 || !b->edges.p || !b->cell_plan.p || getenv("SVGR_NO_SPARE")) return;
    if (!c->spare) c->spare = new (std::nothrow) WorkSpare();
    if (!c->spare) return;
    WorkSpare& w = *c->spare;
    for (int k = 0; k < 4; ++k) w.vp[k] = b->sized_vp[k];
    w.n_segs = b->n_segs; w.n_paths = b->n_paths; w.mask_words = b->mask_words; w.add_shards = b->add_shards; w.n_adds = b->n_adds; w.adds_roomy = b->adds_roomy;
#define X(a) w.a = std::move(b->a);   // (the spare's old arrays are freed by the move)
    SVGR_SPARE_ARRAYS(X)
#undef X
}
// ... and a new, never planned batch of about the same size for the same viewport takes them over.  true: taken
static bool spare_adopt(svgr_batch* b) {
    svgr_ctx* c = b->ctx;
    WorkSpare* w = c->spare;
    if (!w || !w->edges.p || b->sized || !b->has_vp || b->own.world > 1 || b->n_segs <= 4096) return false;
    for (int k = 0; k < 4; ++k) if (w->vp[k] != b->vp[k]) return false;
    if (b->n_segs * 2 < w->n_segs || b->n_segs > w->n_segs + w->n_segs / 2 || b->n_paths * 2 < w->n_paths || b->n_paths > w->n_paths + w->n_paths / 2) return false;
    // (the capacities that are per path / per segment have to hold outright; the others are the pass's guesses)
    if (w->slab_at.cap && w->slab_at.cap < (size_t)b->n_paths) return false;
#define X(a) b->a = std::move(w->a);
    SVGR_SPARE_ARRAYS(X)
#undef X
    b->mask_words = w->mask_words; b->add_shards = w->add_shards; b->n_adds = w->n_adds; b->adds_roomy = w->adds_roomy;
    b->n_bands = (b->vp[2] + TR - 1) / TR;
    b->masks_zeroed = false;   // (whatever the last render of the old batch left: cleared again)
    b->plan.arrays_inherited();
    b->sized = true;
    for (int k = 0; k < 4; ++k) b->sized_vp[k] = b->vp[k];
    return true;
}

static inline dim3 grid1(size_t n, int block = 256) { return dim3((unsigned)((n + block - 1) / block)); }
static inline int cap_i32(size_t n) { return (int)std::min<size_t>(n, 0x7fffffff); }

// Geometry stages.  `upto`: 0 = flatten (count only) + bbox, 1 = flatten (count only: per-segment edge counts and their prefix
// sums), 2 = flatten + emit + bbox, 3 = + band lists, 4 = everything.  `use_vp` = clip bboxes to b->vp and bin relative to it.
// log2 of the lanes k_flatten cuts a segment over: 5, or 6 when a launch over `n_items` segments would not fill the chip
static int choose_fl_sub(const svgr_batch* b, int n_items) {
    const size_t waves32 = ((size_t)std::max(n_items, 1) << 5) / 64, slots = (size_t)b->ctx->n_cu * 4 * 6;   // (six waves per SIMD)
    return waves32 * 2 <= slots ? 6 : 5;
}
static int run_geometry(svgr_batch* b, int upto, bool use_vp) {
    hipStream_t st = b->ctx->stream;
    const int ns = (int)b->n_segs, np = (int)b->n_paths;
    if (!b->arena_zeroed) HIPCHK(hipMemsetAsync(b->arena.p, 0, b->arena_bytes, st));
    b->arena_zeroed = false;  // (the kernels below count into it)
    if (upto < 4) b->plan.lists.drop();   // (a pass that stops short of the tile lists leaves other geometry under them)
    if (upto < 4) b->plan.cells.drop();   // (... and under the cells)
    // multi-GPU with a viewport: the plan listed the segments of the paths whose rows can reach this rank's bands
    // (build_seg_list); a pass without such a list finds the reach itself and lets the flatten skip foreign paths
    const bool listed = use_vp && b->own.world > 1 && b->n_seg_list >= 0;
    const int n_items = listed ? (int)b->n_seg_list : ns;
    // (how many lanes a segment is cut over: decided when the counting pass runs -- the per-lane places follow it -- and kept for
    //  the passes that use its places)
    if (upto == 1) b->fl_sub = choose_fl_sub(b, n_items);
    const int fl_sub = b->fl_sub;
    const dim3 fgrid = grid1((size_t)std::max(n_items, 1) << fl_sub, FL_BLOCK);
    const int* seg_list = listed ? (const int*)b->seg_list.p : (const int*)nullptr;
    const int* plist = listed ? (const int*)b->path_list.p : (const int*)nullptr;
    const int np_walk = listed ? (int)b->n_path_list : np;  // paths k_path_bbox / k_band_entries walk
    const unsigned* prow = nullptr;
    if (use_vp && b->own.world > 1 && ns > 0 && !listed) {
        SVGR_LAUNCH(k_path_rows, grid1((size_t)ns), dim3(256), 0, st, (const double*)b->segs.p, (const uint8_t*)b->seg_kind.p,
                           (const int*)b->seg_path.p, (const double*)b->path_m6.p, ns, b->prow());
        prow = b->prow();
    }
    const int n_bands_vp = use_vp ? (b->vp[2] + TR - 1) / TR : 0;
    if (upto <= 1) {
        if (upto == 1) {  // (segments the pass skips keep a count of zero)
            if (int rc = b->seg_cnt.ensure((size_t)ns + 1)) return rc;
            if (int rc = b->seg_off.ensure((size_t)ns + 2)) return rc;
            if (int rc = b->lane_off.ensure(((size_t)ns << fl_sub) + 1)) return rc;
            if (listed || prow) HIPCHK(hipMemsetAsync(b->seg_cnt.p, 0, sizeof(int) * ((size_t)ns + 1), st));   // (else every segment writes its count)
        }
        if (ns > 0) {
            auto launch_cnt = [&](auto kern) {
                SVGR_LAUNCH(kern, fgrid, dim3(FL_BLOCK), 0, st, (const double*)b->segs.p,
                                   (const uint8_t*)b->seg_kind.p, (const int*)b->seg_path.p, (const double*)b->path_m6.p, ns,
                                   b->thr, (double*)nullptr, (int*)nullptr, b->shards, b->pkeys(), b->bd(), b->own, b->vp[0],
                                   n_bands_vp, prow, seg_list, n_items, upto == 1 ? b->seg_cnt.p : (int*)nullptr, (const int*)nullptr,
                                   use_vp ? b->vp[3] : 0 /* a counting pass: the viewport's width (bounds the columns it adds up) */,
                                   upto == 1 ? b->lane_off.p : (int*)nullptr, (int*)nullptr, (unsigned long long*)nullptr);
            };
            if (getenv("SVGR_DBG_PLAN")) fprintf(stderr, "[geometry] k_flatten<count, %d> full\n", fl_sub);   // (diagnostic, as below)
            if (fl_sub == 6) launch_cnt(k_flatten<false, false, 6>); else launch_cnt(k_flatten<false, false, 5>);
        }
        // (the prefix sums are pass 2's input, not the census's: a census whose read-back waits for an event has them enqueued BEHIND the
        //  read-back -- they run while the host sizes the buffers -- `late_scan`)
        if (upto == 1 && !b->late_scan)
            SVGR_LAUNCH(k_seg_scan, dim3(1), dim3(1024), 0, st, (const int*)b->seg_cnt.p, ns, b->seg_off.p);
        if (upto == 0 || (upto == 1 && b->census_bbox)) {  // bboxes only (no edges stored): the union when there is no viewport; the two-pass plan's census
            b->plan.slabs.drop(); b->plan.lists.drop();
            SVGR_LAUNCH(k_path_bbox, grid1((size_t)std::max(np_walk, 1), 64), dim3(64), 0, st, (const unsigned long long*)b->pkeys(),
                               np_walk, use_vp ? 1 : 0, b->vp[0], b->vp[1], b->vp[2], b->vp[3], b->bbox.p, b->bins.p, b->bd(), 1, plist,
                               (Slab*)nullptr, 0, b->own, (const int*)nullptr, (const int*)nullptr, 0, (const int*)nullptr);
        }
        return 0;
    }
    // (a planned render under the plan's places keeps the plan's band lists: k_tile_lists reads the paths' bboxes and bins itself)
    const bool keep_lists = upto >= 4 && b->plan.planned() && b->plan.slab_at_valid() && use_vp && !b->safe_path;
    // (a planned render takes every cell's add places from the plan's own full pass: one pass over the edge rows, no reservation)
    // (the places are per cell: they hold as long as the paths keep the plan's cell places, i.e. under the plan's slab order)
    const bool placed = b->plan.planned() && b->add_places && b->plan.slab_at_valid() && !b->count_adds_only && b->cell_plan.p != nullptr;
    // A replay of a plan whose slab table the previous render left (PlanState::slabs): k_path_bbox would write, record by
    // record, what is there -- same keys, same `slab_at`, same `bins` -- so it is not launched; k_path_build<1> checks the keys
    // against the kept bboxes instead (error bit 32, as the kernel's own comparison).  One GPU, every path: a rank's list keeps
    // its launch, and so does every pass that is not the placed render.
    const int edge_cap = cap_i32(std::min(b->edge_path.cap, b->edges.cap / 4));
    // (from `edges` on: what the flatten of that pass stored by -- a replay that keeps the table launches k_flatten<.., LEAN>, which takes the places on trust)
    const PlanPrint slabs_now = plan_print(b->slabs.p, b->bbox.p, b->bins.p, b->slab_at.p, b->n_slabs, b->n_paths, b->vp[0], b->vp[1], b->vp[2], b->vp[3],
                                           b->edges.p, b->seg_off.p, b->lane_off.p, b->n_segs, edge_cap, fl_sub, b->thr);
    const bool slabs_for_plan = keep_lists && b->own.world <= 1 && !listed && ns > 0 && b->n_slabs > 0 && b->n_slabs <= (int64_t)cap_i32(b->slabs.cap);
    const bool keep_slabs = b->plan.slabs.holds(slabs_for_plan && placed, slabs_now);
    // ... and the flatten of such a replay is the lean form (k_flatten<.., LEAN>): it stores the edges at the lanes' places and leaves
    // the keys zero, so k_path_build<1> is given no path to check (below).  What the flatten reads and where it stores -- the
    // transforms, the viewport, the bands, `seg_off`, `lane_off`, the edge array -- is what the full pass that made the table had:
    // whatever changes one of them drops PlanState::slabs or is part of `slabs_now`.
    bool lean_fl = false;
    if (ns > 0) {
        // (the counting pass that made `seg_off` left every lane's place inside its segment's slots beside it)
        const bool lane_places = !b->safe_path;
        // (`edge_path` says which path an edge belongs to -- svgr_batch_get_edges is its only reader -- and under a standing plan's lane
        //  places the pass that made the plan has written it, slot by slot, with what this one would store: a placed replay does not)
        const bool keep_edge_path = b->plan.planned() && lane_places && b->lane_off.p && b->lane_off.cap >= ((size_t)ns << fl_sub) && !b->fl_scan;
        auto launch_fl = [&](auto kern, int* places) {
            SVGR_LAUNCH(kern, fgrid, dim3(FL_BLOCK), 0, st, (const double*)b->segs.p,
                               (const uint8_t*)b->seg_kind.p, (const int*)b->seg_path.p, (const double*)b->path_m6.p, ns, b->thr,
                               b->edges.p, keep_edge_path ? (int*)nullptr : b->edge_path.p, b->shards, b->pkeys(), b->bd(), b->own, b->vp[0],
                               n_bands_vp, prow, seg_list, n_items, (int*)nullptr, (const int*)b->seg_off.p,
                               edge_cap, places, (int*)nullptr, (unsigned long long*)nullptr);
        };
        const bool placed_fl = lane_places && b->lane_off.p && b->lane_off.cap >= ((size_t)ns << fl_sub);
        lean_fl = keep_slabs && placed_fl && !b->fl_scan && keep_edge_path;
        if (getenv("SVGR_DBG_PLAN"))   // (diagnostic: which form of the flatten this pass launches)
            fprintf(stderr, "[geometry] k_flatten<%s, %d> %s\n", b->fl_scan ? "scan" : placed_fl ? "placed" : "offsets", fl_sub, lean_fl ? "lean" : "full");
        if (lean_fl) {
            if (fl_sub == 6) launch_fl(k_flatten<true, true, 6, false, true>, b->lane_off.p); else launch_fl(k_flatten<true, true, 5, false, true>, b->lane_off.p);
        } else if (b->fl_scan) {
            // ONE traversal: count, look back, store; leaves seg_cnt / seg_off / lane_off for the renders (needs: one GPU, no list)
            auto launch_scan = [&](auto kern) {
                SVGR_LAUNCH(kern, fgrid, dim3(FL_BLOCK), 0, st, (const double*)b->segs.p,
                                   (const uint8_t*)b->seg_kind.p, (const int*)b->seg_path.p, (const double*)b->path_m6.p, ns, b->thr,
                                   b->edges.p, b->edge_path.p, b->shards, b->pkeys(), b->bd(), b->own, b->vp[0],
                                   n_bands_vp, prow, seg_list, n_items, b->seg_cnt.p, (const int*)nullptr,
                                   cap_i32(std::min(b->edge_path.cap, b->edges.cap / 4)), b->lane_off.p, b->seg_off.p, b->scan_state());
            };
            if (fl_sub == 6) launch_scan(k_flatten<true, false, 6, true>); else launch_scan(k_flatten<true, false, 5, true>);
        } else if (fl_sub == 6) {
            if (placed_fl) launch_fl(k_flatten<true, true, 6>, b->lane_off.p); else launch_fl(k_flatten<true, false, 6>, (int*)nullptr);
        } else {
            if (placed_fl) launch_fl(k_flatten<true, true, 5>, b->lane_off.p); else launch_fl(k_flatten<true, false, 5>, (int*)nullptr);
        }
    }
    if (!keep_slabs) {
        SVGR_LAUNCH(k_path_bbox, grid1((size_t)std::max(np_walk, 1), 64), dim3(64), 0, st, (const unsigned long long*)b->pkeys(), np_walk,
                           use_vp ? 1 : 0, b->vp[0], b->vp[1], b->vp[2], b->vp[3], b->bbox.p, b->bins.p, b->bd(), b->plan.planned() ? 0 : 1, plist,
                           upto >= 3 ? b->slabs.p : (Slab*)nullptr, (int)std::min<int64_t>(cap_i32(b->slabs.cap), b->n_slabs) /* = k_path_build's grid */, b->own,
                           (const int*)b->path_seg0.p, (const int*)b->seg_off.p, edge_cap,
                           upto >= 4 && b->plan.planned() && b->plan.slab_at_valid() ? (const int*)b->slab_at.p : (const int*)nullptr);
        b->plan.slab_table_written(slabs_for_plan, slabs_now);   // (written at the plan's places, or in some other form)
    }
    if (upto == 2) return 0;
    // per owned band: its list of (path, band) pairs in paint order, and its first tile-list slot
    const int owned = count_owned_bands(b->own, b->n_bands);
    // (upto >= 4 on one GPU: the kernel also clears the tiles' entry bitmasks of its band when they are not clear yet)
    const bool clear_in_be = owned > 0 && !keep_lists && upto >= 4 && !b->masks_zeroed && b->tile_mask.p && b->own.world <= 1;
    if (!keep_lists) b->plan.lists.drop();   // (the bands are listed again: the tile lists in place follow the old band lists)
    if (owned > 0 && !keep_lists)
        SVGR_LAUNCH(k_band_entries, dim3(owned), dim3(BE_BLOCK), 0, st, (const PathBin*)b->bins.p, np_walk, plist,
                           (const int*)b->bbox.p, b->band_start.p, b->band_count.p, b->band_item0.p, b->entries.p,
                           b->pair_idx.p, cap_i32(std::min(b->entries.cap, b->pair_idx.cap)),
                           upto >= 4 ? cap_i32(b->items.cap) : 0x7fffffff, b->vp[1], b->bd(), b->own,
                           upto >= 4 && b->plan.planned() && use_vp && !b->safe_path ? 1 : 0,
                           clear_in_be ? b->tile_mask.p : (unsigned long long*)nullptr, b->n_ctiles() * 2 * b->mask_words);
    if (clear_in_be) b->masks_zeroed = true;
    if (upto == 3) return 0;
    // (the tiles read their mask words whether or not any pair exists: a batch without entries still needs them clear --
    //  a block from the cache is not zero)
    if (!b->masks_zeroed && b->tile_mask.p) {
        HIPCHK(hipMemsetAsync(b->tile_mask.p, 0, b->mask_bytes(), st));
        b->masks_zeroed = true;
    }
    // per slab of a path's cells: carry-ins, classes, headers, add lists
    unsigned long long* pb_dbg = nullptr;
#ifdef SVGR_DBG_PB_STAMP
    {
        static unsigned long long* buf = nullptr;
        if (!buf) { (void)hipMalloc((void**)&buf, 8 * 8 * 8192); (void)hipMemset(buf, 0, 8 * 8 * 8192); }
        pb_dbg = buf;
    }
#endif
    // A placed replay that keeps its band lists and writes or keeps the plan's slab table lists every band from the plan's places and
    // its own mask words alone: its full k_tile_lists saves the words (`tile_mask_kept`), and the replay behind it -- slab table kept,
    // the same arrays (`lists_now`) -- asks the kernel to list only the bands whose words differ from the saved ones.
    const size_t mask_n = b->mask_bytes() / sizeof(unsigned long long);
    const bool lists_for_plan = slabs_for_plan && placed && owned > 0 && b->n_ctiles() > 0 && b->tile_mask.p && b->tile_mask_kept.p &&
                                b->tile_mask.cap >= mask_n && b->tile_mask_kept.cap >= mask_n;
    const PlanPrint lists_now = plan_print(b->items.p, b->pages.p, b->tile_info.p, b->entries.p, b->bins.p, b->bbox.p, b->cell_hdr.p, b->cell_plan.p,
                                           b->tile_mask.p, b->tile_mask_kept.p, b->items.cap, b->pages.cap, b->tile_info.cap, b->entries.cap,
                                           b->bins.cap, b->bbox.cap, b->cell_hdr.cap, b->cell_plan.cap, b->tile_mask.cap, b->tile_mask_kept.cap,
                                           b->n_ctiles(), b->mask_words, owned, b->vp[0], b->vp[1], b->vp[2], b->vp[3]);
    const bool lists_kept = b->plan.lists.holds(lists_for_plan && keep_slabs, lists_now);
    bool bits_implied = false;   // the path build set no class-2 cell's mask bits (its lean form): k_tile_lists takes them from the saved words
    if (b->n_slabs <= 0) b->plan.cells.drop();
    if (b->n_slabs > 0) {
        b->masks_zeroed = false;  // (bits are set below; k_tile_lists clears them again)
        auto launch_pb = [&](auto kern) {
            SVGR_LAUNCH(kern, dim3((unsigned)b->n_slabs), dim3(PB_THREADS), 0, st, (const Slab*)b->slabs.p, (const double*)b->edges.p,
                               (const int*)b->pair_idx.p, (const double*)b->path_paint.p, (const uint8_t*)b->path_rule.p,
                               b->n_groups > 0 ? (const int*)b->path_group.p : (const int*)nullptr,
                               b->n_grads > 0 ? (const int*)b->path_grad.p : (const int*)nullptr, b->vp[0], b->vp[1], b->n_ctiles(), b->mask_words,
                               b->tile_mask.p, b->cell_hdr.p, cap_i32(std::min(b->cell_hdr.cap, b->cell_plan.cap)), b->add_shards,
                               b->count_adds_only ? (TileAdd*)nullptr : b->adds.p, b->cell_plan.p, b->bd(), b->own, b->plan.planned() ? 0 : 1,
                               b->deterministic ? 1 : 0, pb_dbg, keep_slabs ? (const unsigned long long*)b->pkeys() : (const unsigned long long*)nullptr,
                               (const int*)b->bbox.p, (const PathBin*)b->bins.p,
                               lean_fl ? 0 /* (no keys behind the lean flatten: the guard's loop over the paths makes no trip) */ : np, b->vp[2], b->vp[3]);
        };
        // (an unplanned pass over add lists sized with room to spare: ONE pass on the workgroup's own bounds, MODE 2)
        const bool bounded = !placed && !b->count_adds_only && b->adds.p && b->adds_roomy && !b->safe_path && !getenv("SVGR_SAFE_PATH");
        // The placed pass of a kept replay behind the lean flatten has nothing to guard; on one GPU, not deterministic, without groups or
        // gradients and with the plan standing (no statistics) every option of the kernel has the value k_path_build<1, LEAN> is compiled for.
        // The lean form writes neither the class-2 cells' headers nor the sentinels of their lists: it runs where the last pass that wrote
        // the cells left them as this one would (PlanState::cells).  In a run of kept replays that is the pass that wrote the slab
        // table; after svgr_batch_set_paints one full pass comes first.
        const PlanPrint cells_now = plan_print(b->adds.p, b->cell_hdr.p, b->cell_plan.p, b->tile_mask_kept.p, b->path_paint.p, b->path_rule.p,
                                               b->adds.cap, b->cell_hdr.cap, b->cell_plan.cap, b->tile_mask_kept.cap, b->add_shards);
        const bool cells_pass = placed && b->own.world <= 1 && b->n_groups == 0 && b->n_grads == 0 && b->plan.planned() && !b->count_adds_only &&
                                b->adds.p != nullptr;   // (deterministic or not: the same headers and sentinels at the same places)
        const bool cells_kept = b->plan.cells.holds(cells_pass, cells_now);
        bool lean_pb = placed && keep_slabs && lean_fl && b->own.world <= 1 && !b->deterministic && b->n_groups == 0 && b->n_grads == 0 &&
                       b->plan.planned() && !b->count_adds_only && b->adds.p != nullptr && cells_kept &&
                       lists_kept /* (it sets no class-2 cell's mask bits: the saved words have them) */;
        b->plan.cells.wrote(cells_pass, cells_now);
#ifdef SVGR_DBG_PB_STAMP
        lean_pb = false;   // (the stamps are the full form's)
#endif
        if (getenv("SVGR_DBG_PLAN")) {   // (diagnostic: which instantiation this pass launches, and whether it found the slab table in place)
            fprintf(stderr, "[geometry] path build form %s\n", lean_pb ? "lean" : "full");
            fprintf(stderr, "[geometry] cells %s\n", cells_kept ? "current" : "stale");   // (what stands in `cell_hdr` / `adds` is what this pass would write, or not)
            fprintf(stderr, "[geometry] k_path_build<%d>%s, %lld slabs, tile lists %s, slab table %s\n", placed ? 1 : bounded ? 2 : 0,
                    b->count_adds_only ? " measuring" : "", (long long)b->n_slabs,
                    lists_kept ? "kept" : "rebuilt" /* (what k_tile_lists is asked for: a band whose words differ is listed again on the device) */,
                    keep_slabs ? "kept" : "written");
        }
        bits_implied = lean_pb;
        if (lean_pb) launch_pb(k_path_build<1, true>); else if (placed) launch_pb(k_path_build<1>); else if (bounded) launch_pb(k_path_build<2>); else launch_pb(k_path_build<0>);
#ifdef SVGR_DBG_PB_STAMP
        if (pb_dbg && b->plan.planned() && !b->count_adds_only) {
            static int n_dump = 0;
            if (++n_dump == 20) {  // one render, well into the run
                HIPCHK(hipStreamSynchronize(st));
                const size_t n = (size_t)std::min<int64_t>(b->n_slabs, 8192);
                std::vector<unsigned long long> h(8 * n);
                HIPCHK(hipMemcpy(h.data(), pb_dbg, sizeof(unsigned long long) * h.size(), hipMemcpyDeviceToHost));
                double ph[5] = {0, 0, 0, 0, 0}, rows_ = 0;
                unsigned long long lo = ~0ull, hi = 0;
                for (size_t i = 0; i < n; ++i) {
                    for (int q = 0; q < 5; ++q) ph[q] += (double)(h[8 * i + q + 1] - h[8 * i + q]);
                    rows_ += (double)h[8 * i + 6];
                    lo = std::min(lo, h[8 * i]); hi = std::max(hi, h[8 * i + 3]);
                }
                double s_rec = 0, s_edges = 0;
                for (size_t i = 0; i < n; ++i) { s_rec += (double)(h[8 * i + 7] - h[8 * i]); s_edges += (double)(h[8 * i + 5] - h[8 * i + 7]); }
                fprintf(stderr, "[pb stamp] %zu slabs, mean us: stage %.2f (slab record %.2f, edges landed +%.2f)  passA %.2f  walk %.2f | rows/slab %.0f | span %.1f us\n", n,
                        ph[0] / n / 100, s_rec / n / 100, s_edges / n / 100, ph[1] / n / 100, ph[2] / n / 100, rows_ / n, (double)(hi - lo) / 100);
                if (const char* f = getenv("SVGR_DBG_PB_DUMP")) { if (FILE* fp = fopen(f, "wb")) { fwrite(h.data(), 8, h.size(), fp); fclose(fp); } }
            }
        }
#endif
    }
    // per owned band: the tiles' item lists and the launch order of the tile kernel; clears the bitmasks again
    if (owned > 0 && b->n_ctiles() > 0) {
        if (lists_kept)
            if (const char* sb = getenv("SVGR_DBG_STALE_BAND")) {   // (tests: one saved word of band `sb` made wrong -- that band, and no other, is listed again)
                const int band = atoi(sb);
                if (band >= 0 && band < b->n_bands) {
                    unsigned long long* const w0 = b->tile_mask_kept.p + (size_t)band * b->n_ctiles() * 2 * b->mask_words;
                    HIPCHK(hipMemcpyAsync(&b->stale_word, w0, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
                    HIPCHK(hipStreamSynchronize(st));
                    b->stale_word ^= 1ull;
                    HIPCHK(hipMemcpyAsync(w0, &b->stale_word, sizeof(unsigned long long), hipMemcpyHostToDevice, st));
                }
            }
        SVGR_LAUNCH(k_tile_lists, dim3(owned), dim3(TL_BLOCK), 0, st, (const int*)b->band_start.p, (const int*)b->band_item0.p,
                           (const TileEntry*)b->entries.p, b->tile_mask.p, b->mask_words, b->n_ctiles(), b->vp[1], b->own, owned,
                           b->tile_info.p, b->pages.p, b->items.p, (const CellHdr*)b->cell_hdr.p, cap_i32(b->items.cap), cap_i32(b->cell_hdr.cap), b->bd(),
                           keep_lists ? (const PathBin*)b->bins.p : (const PathBin*)nullptr, (const int*)b->bbox.p,
                           lists_for_plan ? b->tile_mask_kept.p : (unsigned long long*)nullptr, lists_kept ? (bits_implied ? 2 : 1) : 0);
        b->masks_zeroed = true;
    }
    b->plan.lists.wrote(lists_for_plan, lists_now);
    return 0;
}

// `capacity_bits`: when given, capacity overflows (bits 2|4|8) are returned there instead of failing
// Read the device-side error flags (and, while planning, all the counters: `whole`).  After renders only the error
// word is meaningful -- the tile kernel has zeroed the rest of the arena for the next render -- and it is sticky until
// it has been read here.  `capacity_bits`: when given, capacity overflows (bits 2|4|8) are returned there instead of failing.
// `with_bboxes`: fetch the per-path bboxes in the same round trip (one synchronisation instead of two)
// the sticky error word of a geometry pass -> status (capacity overflows are reported apart when the caller can recover)
static int eval_dev_err(int e, int* capacity_bits) {
    if (capacity_bits) { *capacity_bits = e & (2 | 4 | 8 | 32 | 64); e &= ~(2 | 4 | 8 | 32 | 64); }
    if (e & 1) return fail(SVGR_E_OVERFLOW, "flatten depth cap (%d) hit: non-finite or absurd control points", kMaxFlattenDepth);
    if (e & 16) return fail(SVGR_E_INVALID, "path extent beyond +-1e9 pixels or non-finite");
    if (e & (2 | 4 | 8 | 32 | 64)) return fail(SVGR_E_OVERFLOW, "work buffer capacity exceeded (err bits %d): call svgr_batch_plan again", e);
    return 0;
}
// enqueue the read-back of a pass's scalars (and bboxes) into the batch's host copies; valid after the stream has drained
// (`staging`: page-locked memory of sizeof(BatchDev) + 16 bytes per path -- a copy into pageable memory blocks the host until
//  it is done, which is what svgr_batch_plan_many is there to avoid; take_readback moves it into the host copies afterwards)
static int issue_readback(svgr_batch* b, bool with_bboxes, void* staging = nullptr) {
    void* bd_dst = staging ? staging : (void*)&b->host_bd;
    HIPCHK(hipMemcpyAsync(bd_dst, b->bd(), sizeof(BatchDev), hipMemcpyDeviceToHost, b->ctx->stream));
    if (with_bboxes && !(b->defer_bbox && staging)) {
        b->host_bbox.resize(4 * (size_t)b->n_paths);
        b->host_bbox_stale = false;
        void* bb_dst = staging ? (void*)((char*)staging + sizeof(BatchDev)) : (void*)b->host_bbox.data();
        HIPCHK(hipMemcpyAsync(bb_dst, b->bbox.p, sizeof(int) * 4 * (size_t)b->n_paths, hipMemcpyDeviceToHost, b->ctx->stream));
    }
    return 0;
}
static void take_readback(svgr_batch* b, const void* staging) {
    memcpy(&b->host_bd, staging, sizeof(BatchDev));
    if (b->defer_bbox) { b->host_bbox_stale = true; return; }
    memcpy(b->host_bbox.data(), (const char*)staging + sizeof(BatchDev), sizeof(int) * 4 * (size_t)b->n_paths);
    b->host_bbox_stale = false;
}
// the per-path bboxes on the host (a re-plan through svgr_batch_draw leaves them on the device until somebody needs them: the copy
// is a launch between the geometry pass and the tile kernel otherwise)
static int ensure_host_bbox(svgr_batch* b) {
    if (!b->host_bbox_stale) return 0;
    b->host_bbox.resize(4 * (size_t)b->n_paths);
    HIPCHK(hipMemcpyAsync(b->host_bbox.data(), b->bbox.p, sizeof(int) * 4 * (size_t)b->n_paths, hipMemcpyDeviceToHost, b->ctx->stream));
    HIPCHK(hipStreamSynchronize(b->ctx->stream));
    b->host_bbox_stale = false;
    return 0;
}
static int check_dev_err(svgr_batch* b, int* capacity_bits = nullptr, bool whole = true, bool with_bboxes = false) {
    int e = 0;
    if (whole) {
        if (int rc = issue_readback(b, with_bboxes)) return rc;
        HIPCHK(hipStreamSynchronize(b->ctx->stream));
        e = b->host_bd.err;
        if (e) b->invalidate_work();
    } else {
        HIPCHK(hipMemcpyAsync(&e, b->bd(), sizeof(int), hipMemcpyDeviceToHost, b->ctx->stream));
        HIPCHK(hipStreamSynchronize(b->ctx->stream));
        if (e) {
            HIPCHK(hipMemsetAsync(b->bd(), 0, sizeof(int), b->ctx->stream));
            b->invalidate_work();
        }
    }
    HIPCHK(hipGetLastError());
    return eval_dev_err(e, capacity_bits);
}

// No C++ exception crosses the ABI (std::vector / std::map growth on the host can throw): the entry points that allocate
// host memory run their body through this guard.
template <class F>
static int abi_guard(const char* what, F&& body) {
    try {
        return body();
    } catch (const std::bad_alloc&) {
        return fail(SVGR_E_NOMEM, "%s: out of host memory", what);
    } catch (...) {
        return fail(SVGR_E_INVALID, "%s: unexpected C++ exception", what);
    }
}

// the scalar part of a gradient description (everything but the stops)
static void fill_grad_dev(GradDev& h, const svgr_gradient* g) {
    memset(&h, 0, sizeof h);
    h.kind = g->kind; h.spread = g->spread; h.has_gt = g->has_gt; h.n_stops = g->n_stops; h.excl_enabled = g->excl_enabled;
    memcpy(h.user_m6, g->user_m6, sizeof h.user_m6);
    memcpy(h.gt_m6, g->gt_m6, sizeof h.gt_m6);
    h.p0[0] = g->p0[0]; h.p0[1] = g->p0[1]; h.vec[0] = g->vec[0]; h.vec[1] = g->vec[1]; h.vv = g->vv;
    h.center[0] = g->center[0]; h.center[1] = g->center[1]; h.radius = g->radius;
    h.fcenter[0] = g->fcenter[0]; h.fcenter[1] = g->fcenter[1]; h.fradius = g->fradius;
    h.cd[0] = g->cd[0]; h.cd[1] = g->cd[1]; h.rd = g->rd; h.a = g->a; h.frad_rd = g->frad_rd; h.frad2 = g->frad2;
    h.excl_thresh = g->excl_thresh;
}
static int check_gradient(const svgr_gradient* g) {
    if (g->kind < 1 || g->kind > 3 || g->spread < 0 || g->spread > 2) return fail(SVGR_E_INVALID, "invalid gradient kind / spread method");
    if (g->n_stops < 1 || g->n_stops > (1 << 20) || !g->stop_off || !g->stop_rgba)
        return fail(SVGR_E_INVALID, "gradient needs at least one stop");
    return 0;
}

// The production variant: a float32 canvas without gradients, groups or clips -- the tile kernel with fixed load registers and the
// persistent tile loop (k_tile_render<0, false>).
static bool production_variant(const svgr_batch* b, int out_kind) {
    return out_kind == SVGR_OUT_CANVAS_F32 && b->n_grads == 0 && b->n_groups == 0 && !b->has_clips;
}
// The tile kernel's variant for a render, chosen here for both kernel families: `launch(TileVariant<OUT, CLIP, GROUPS, GRAD>{})`.
template <int OUT_, bool CLIP_ = false, bool GROUPS_ = false, bool GRAD_ = false>
struct TileVariant {
    static constexpr int OUT = OUT_;
    static constexpr bool CLIP = CLIP_, GROUPS = GROUPS_, GRAD = GRAD_;
};
template <int OUT, class F>
static void with_canvas_variant(const svgr_batch* b, F& launch) {
    if (b->n_grads > 0) launch(TileVariant<OUT, true, true, true>{});
    else if (b->n_groups > 0) launch(TileVariant<OUT, true, true>{});
    else if (b->has_clips) launch(TileVariant<OUT, true>{});
    else launch(TileVariant<OUT, false>{});
}
template <class F>
static void with_tile_variant(const svgr_batch* b, int out_kind, F&& launch) {
    switch (out_kind) {
        case 0: with_canvas_variant<0>(b, launch); break;
        case 1: with_canvas_variant<1>(b, launch); break;
        case 2: launch(TileVariant<2>{}); break;
        default: launch(TileVariant<3>{}); break;
    }
}

// ---- the layer entries' common parts
// (a bbox argument becomes a Box through svgr::box_of, svgr_box.h: the range checks and the narrowing, once)
// the over / blend / crop4 / in entries: an RGBA layer over the box `ob` and a source of `ch` (1 or 4) values per pixel over `sb`
static int check_layer_pair(const char* entry, const svgr_ctx* ctx, const svgr_buf* out, const int64_t* ob, Box& o, const svgr_buf* src,
                            const int64_t* sb, Box& s, int ch) {
    if (!ctx || !out || !src || !box_of(ob, o) || !box_of(sb, s) || (ch != 1 && ch != 4)) return fail(SVGR_E_INVALID, "%s: bad arguments", entry);
    if (out->bytes < box_px(o) * 32 || src->bytes < box_px(s) * 8 * ch) return fail(SVGR_E_INVALID, "%s: buffer too small", entry);
    return 0;
}

// the end of an entry with one plain launch: on the context's stream, checked, no wait
template <class... Param, class... Arg>
static int launch_tail(svgr_ctx* ctx, void (*kernel)(Param...), dim3 grid, dim3 block, unsigned lds, Arg... args) {
    HIPCHK(enter_ctx(ctx));
    SVGR_LAUNCH(kernel, grid, block, lds, ctx->stream, args...);
    HIPCHK(hipGetLastError());
    return 0;
}

// The end of an entry that hands the device host arrays of its caller: the pieces go back to back into one pool block on the
// context's stream, `launch(block)` enqueues the work, and ONE wait lets the copies finish reading the caller's memory before
// the call returns.  The caller has entered the context.
struct HostSpan { const void* p; size_t bytes; };
template <class Launch>
static int upload_launch_wait(svgr_ctx* ctx, const char* entry, std::initializer_list<HostSpan> host, Launch&& launch) {
    size_t bytes = 0;
    for (const HostSpan& h : host) bytes += h.bytes;
    PoolBlock dev;
    hipError_t e = dev.alloc(bytes);
    size_t at = 0;
    for (const HostSpan& h : host) {
        if (e == hipSuccess) e = hipMemcpyAsync(dev.as<char>() + at, h.p, h.bytes, hipMemcpyHostToDevice, ctx->stream);
        at += h.bytes;
    }
    if (e == hipSuccess) {
        launch(dev.p);
        e = hipGetLastError();
        const hipError_t w = hipStreamSynchronize(ctx->stream);
        if (e == hipSuccess) e = w;
    }
    if (e != hipSuccess) return fail(SVGR_E_HIP, "%s: %s", entry, hipGetErrorString(e));
    return 0;
}

// Separable?  blur_kernel (S:1903-1944) is a product of two 1-D Gaussians whenever the transform is axis aligned
// (scale, translate, x/y swap): K = u v^T / S with u, v the row / column sums and S the total, to a few ulp.  Then two
// 1-D passes do the work of the kw x kh stencil (146 taps instead of 5329 for the largest blur of icons.svg).  A
// rotated or skewed blur is not rank 1 and takes the direct 2-D kernel.  (The reference lets scipy pick an FFT here,
// which carries ~1e-16 absolute noise itself; both device forms sum in double and stay below that.)
// (row / column sums in extended precision: summed in plain doubles their own rounding -- not the kernel's rank --
// decided the test below for some sizes, and a separable blur then took the 625-tap stencil)
// (the analysis of a kernel is kept: a document's blurs come back with every render, and the row / column sums of a
//  73 x 73 kernel are 5 000 long-double additions and as many comparisons -- 26 us of host time per call)
struct Analysed { std::vector<double> k, u, v; double total; bool separable; };
static std::shared_ptr<const Analysed> analyse_kernel(const double* kernel, int64_t kw, int64_t kh) {
    static std::mutex an_mu;
    static std::unordered_map<unsigned long long, std::shared_ptr<const Analysed>> an_cache;
    // (in front of the hash: the caller's array itself -- a document's blur kernels are kept by the caller and come back at the
    //  same address; hashing a 73 x 73 kernel was 5 us of the call's 9)
    struct ByPtr { const double* p = nullptr; int64_t kw = 0, kh = 0; std::shared_ptr<const Analysed> an; };
    static ByPtr by_ptr[64];
    ByPtr& slot = by_ptr[((uintptr_t)kernel >> 4) & 63];
    std::shared_ptr<const Analysed> an;
    {
        std::lock_guard<std::mutex> lk(an_mu);
        if (slot.p == kernel && slot.kw == kw && slot.kh == kh && slot.an && memcmp(slot.an->k.data(), kernel, sizeof(double) * (size_t)kw * kh) == 0)
            an = slot.an;
    }
    unsigned long long hkey = 1469598103934665603ull ^ (unsigned long long)kw * 1099511628211ull ^ ((unsigned long long)kh << 32);
    if (!an) {
        const unsigned long long* w64 = (const unsigned long long*)kernel;   // (doubles: 8 bytes each)
        for (int64_t i = 0; i < kw * kh; ++i) hkey = (hkey ^ w64[i]) * 1099511628211ull;
        std::lock_guard<std::mutex> lk(an_mu);
        auto it = an_cache.find(hkey);
        if (it != an_cache.end() && it->second->u.size() == (size_t)kw && it->second->v.size() == (size_t)kh &&
            memcmp(it->second->k.data(), kernel, sizeof(double) * (size_t)kw * kh) == 0) {
            an = it->second;
            slot.p = kernel; slot.kw = kw; slot.kh = kh; slot.an = an;
        }
    }
    if (!an) {
        auto fresh = std::make_shared<Analysed>();
        std::vector<long double> ul((size_t)kw, 0.0L), vl((size_t)kh, 0.0L);
        long double total_l = 0.0L;
        double kmax = 0.0;
        for (int64_t i = 0; i < kw; ++i)
            for (int64_t j = 0; j < kh; ++j) {
                const double k = kernel[i * kh + j];
                ul[(size_t)i] += k; vl[(size_t)j] += k; total_l += k;
                kmax = std::fabs(k) > kmax ? std::fabs(k) : kmax;
            }
        fresh->u.resize((size_t)kw); fresh->v.resize((size_t)kh);
        for (int64_t i = 0; i < kw; ++i) fresh->u[(size_t)i] = (double)ul[(size_t)i];
        for (int64_t j = 0; j < kh; ++j) fresh->v[(size_t)j] = (double)vl[(size_t)j];
        fresh->total = (double)total_l;
        bool sep = kw > 1 && kh > 1 && std::isfinite(fresh->total) && fresh->total != 0.0;
        for (int64_t i = 0; i < kw && sep; ++i)
            for (int64_t j = 0; j < kh; ++j)
                if (!(std::fabs(kernel[i * kh + j] - fresh->u[(size_t)i] * fresh->v[(size_t)j] / fresh->total) <= 8 * 2.220446049250313e-16 * kmax)) { sep = false; break; }
        fresh->separable = sep;
        fresh->k.assign(kernel, kernel + kw * kh);
        std::lock_guard<std::mutex> lk(an_mu);
        if (an_cache.size() > 256) an_cache.clear();
        an_cache[hkey] = fresh;
        an = fresh;
        slot.p = kernel; slot.kw = kw; slot.kh = kh; slot.an = an;
    }
    return an;
}
// ======================================================================================
// C ABI
// ======================================================================================
extern "C" {

int svgr_abi_version(void) { return SVGR_ABI_VERSION; }

// 64-bit hash of host buffers (see svgr.h): eight bytes at a time through a multiply-xorshift mixer, the tail and every
// buffer's length folded in.  Not cryptographic: it tells "edited in place" from "untouched".
int svgr_hash_buffers(const void* const* ptrs, const int64_t* nbytes, int64_t n, uint64_t* out) {
    if (n < 0 || !out || (n > 0 && (!ptrs || !nbytes))) return fail(SVGR_E_INVALID, "bad arguments");
    auto mix = [](uint64_t h, uint64_t v) {
        h ^= v * 0x9e3779b97f4a7c15ull;
        h = (h ^ (h >> 29)) * 0xbf58476d1ce4e5b9ull;
        return h ^ (h >> 32);
    };
    uint64_t h = 0x243f6a8885a308d3ull;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t len = nbytes[i];
        if (len < 0 || (len > 0 && !ptrs[i])) return fail(SVGR_E_INVALID, "buffer %lld: bad pointer or size", (long long)i);
        const unsigned char* p = (const unsigned char*)ptrs[i];
        // four independent lanes: the multiplies of one word do not wait for the previous word's
        uint64_t a = h, b = h ^ 0x13198a2e03707344ull, c = h ^ 0xa4093822299f31d0ull, d = h ^ 0x082efa98ec4e6c89ull;
        int64_t k = 0;
        for (; k + 32 <= len; k += 32) {
            uint64_t w[4];
            memcpy(w, p + k, 32);
            a = mix(a, w[0]); b = mix(b, w[1]); c = mix(c, w[2]); d = mix(d, w[3]);
        }
        for (; k + 8 <= len; k += 8) {
            uint64_t w;
            memcpy(&w, p + k, 8);
            a = mix(a, w);
        }
        uint64_t tail = 0;
        if (k < len) memcpy(&tail, p + k, (size_t)(len - k));
        h = mix(mix(mix(mix(mix(a, b), c), d), tail), (uint64_t)len);
    }
    *out = h;
    return 0;
}
int svgr_tile_rows(void) { return TR; }
int svgr_tile_cols(void) { return TC; }
const char* svgr_last_error(void) { return g_err.c_str(); }

int svgr_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// the context's page-locked upload staging, free to be written (the previous copy out of it has finished), at least `bytes` large;
// nullptr when `bytes` is beyond what is worth pinning or the allocation fails: the caller then uploads from its own host copy
static void* upload_stage(svgr_ctx* c, size_t bytes) {
    constexpr size_t kMaxStage = 64u << 20;
    if (bytes > kMaxStage) return nullptr;
    if (c->up_busy && c->up_ev) { (void)hipEventSynchronize(c->up_ev); c->up_busy = false; }
    if (c->up_stage_bytes < bytes) {
        if (c->up_stage) (void)hipHostFree(c->up_stage);
        c->up_stage = nullptr;
        c->up_stage_bytes = 0;
        const size_t want = std::min(std::max<size_t>(bytes + bytes / 2, 4u << 20), kMaxStage);
        if (hipHostMalloc(&c->up_stage, want, hipHostMallocDefault) != hipSuccess) { c->up_stage = nullptr; (void)hipGetLastError(); return nullptr; }
        c->up_stage_bytes = want;
    }
    if (!c->up_ev && hipEventCreateWithFlags(&c->up_ev, hipEventDisableTiming) != hipSuccess) { c->up_ev = nullptr; return nullptr; }
    return c->up_stage;
}
static hipError_t upload_staged(svgr_ctx* c, void* dst, size_t bytes) {   // (`bytes` of the staging -> dst, on the context's stream)
    hipError_t e = hipMemcpyAsync(dst, c->up_stage, bytes, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipEventRecord(c->up_ev, c->stream);
    c->up_busy = true;
    return e;
}

int svgr_init(int device_id, svgr_ctx** out) {
    if (!out) return fail(SVGR_E_INVALID, "svgr_init: out is NULL");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) return fail(SVGR_E_NODEVICE, "no HIP device visible (%s)", hipGetErrorString(e));
    if (device_id < 0 || device_id >= n) return fail(SVGR_E_INVALID, "device %d out of range (0..%d)", device_id, n - 1);
    HIPCHK(hipSetDevice(device_id));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device_id));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(SVGR_E_NODEVICE, "device %d is %s; this library is built for gfx950 only", device_id, prop.gcnArchName);
    svgr_ctx* c = new (std::nothrow) svgr_ctx();
    if (!c) return fail(SVGR_E_NOMEM, "out of host memory");
    c->device = device_id;
    static std::atomic<int> next_id{1};
    c->id = next_id.fetch_add(1);
    g_pool.open(c->id);
    tl_ctx_id = c->id;
    snprintf(c->name, sizeof c->name, "%s (%s, %d CUs)", prop.name[0] ? prop.name : "AMD Instinct", prop.gcnArchName, prop.multiProcessorCount);
    hipError_t se = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (se != hipSuccess) { delete c; return fail(SVGR_E_HIP, "hipStreamCreate: %s", hipGetErrorString(se)); }
    c->own_stream = true;
    c->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    if (hipMalloc(&c->trash, 1024) != hipSuccess || hipMalloc((void**)&c->tile_ctr, 2 * 8 * 128) != hipSuccess ||
        hipMemset(c->tile_ctr, 0, 2 * 8 * 128) != hipSuccess) {
        (void)hipStreamDestroy(c->stream);
        delete c;
        return fail(SVGR_E_NOMEM, "out of device memory");
    }
    // page-locked staging for the read-backs of svgr_batch_draw / svgr_batch_plan_many (grown on demand: a first frame should not pay for it)
    if (hipHostMalloc(&c->pinned, 1u << 20, hipHostMallocDefault) == hipSuccess) c->pinned_bytes = 1u << 20;
    else c->pinned = nullptr;
    if (hipEventCreateWithFlags(&c->pin_ev, hipEventDisableTiming) != hipSuccess) c->pin_ev = nullptr;
    (void)upload_stage(c, 1);   // (the upload staging at its smallest size, 4 MiB: likewise)
    *out = c;
    return 0;
}

int svgr_shutdown(svgr_ctx* ctx) {
    if (!ctx) return 0;
    (void)enter_ctx(ctx);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    if (ctx->own_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
    for (int k = 0; k < svgr_ctx::N_SIDE; ++k) {
        if (ctx->side[k]) { (void)hipStreamSynchronize(ctx->side[k]); (void)hipStreamDestroy(ctx->side[k]); }
        if (ctx->side_ev[k]) (void)hipEventDestroy(ctx->side_ev[k]);
    }
    if (ctx->fork_ev) (void)hipEventDestroy(ctx->fork_ev);
    for (auto e : ctx->xs_ev) if (e) (void)hipEventDestroy(e);
    for (auto e : ctx->meas_ev) if (e) (void)hipEventDestroy(e);
    if (ctx->pin_ev) (void)hipEventDestroy(ctx->pin_ev);
    delete ctx->spare;
    if (ctx->pinned) (void)hipHostFree(ctx->pinned);
    if (ctx->up_busy && ctx->up_ev) (void)hipEventSynchronize(ctx->up_ev);
    if (ctx->up_stage) (void)hipHostFree(ctx->up_stage);
    if (ctx->up_ev) (void)hipEventDestroy(ctx->up_ev);
    if (ctx->trash) (void)hipFree(ctx->trash);
    if (ctx->tile_ctr) (void)hipFree(ctx->tile_ctr);
    g_pool.close(ctx->id);  // (its cached blocks; what it still has out is freed on return)
    delete ctx;
    return 0;
}

int svgr_set_stream(svgr_ctx* ctx, void* hip_stream) {
    if (!ctx) return fail(SVGR_E_INVALID, "ctx is NULL");
    HIPCHK(enter_ctx(ctx));
    // The block cache hands a freed block to the next caller on the strength of stream order alone, so the outgoing
    // stream -- owned or the caller's -- must have drained before work is enqueued on another one.
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (ctx->own_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
    ctx->stream = (hipStream_t)hip_stream;
    ctx->own_stream = false;
    return 0;
}

int svgr_sync(svgr_ctx* ctx) {
    if (!ctx) return fail(SVGR_E_INVALID, "ctx is NULL");
    HIPCHK(enter_ctx(ctx));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    HIPCHK(hipGetLastError());
    return 0;
}

// ---- measurement helpers (bench.py): device time of a stretch of the context's stream, launches made ------------------------------
__global__ void k_spin(unsigned long long ticks) {   // s_memrealtime counts at 100 MHz
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    while (__builtin_amdgcn_s_memrealtime() - t0 < ticks) __builtin_amdgcn_s_sleep(32);
}
int svgr_measure_launches(uint64_t* out) {
    if (!out) return fail(SVGR_E_INVALID, "out is NULL");
    *out = g_n_launches.load(std::memory_order_relaxed);
    return 0;
}
int svgr_measure_begin(svgr_ctx* ctx, double hold_ms) {
    if (!ctx || !(hold_ms >= 0.0) || hold_ms > 200.0) return fail(SVGR_E_INVALID, "bad arguments");
    HIPCHK(enter_ctx(ctx));
    if (!ctx->meas_ev[0]) { HIPCHK(hipEventCreate(&ctx->meas_ev[0])); HIPCHK(hipEventCreate(&ctx->meas_ev[1])); }
    // (the stream is held busy for `hold_ms` so that everything the caller enqueues next queues up behind it and then runs back to back:
    //  the time between the two events is DEVICE time, whatever the host took to issue it -- as long as it took less than the hold)
    if (hold_ms > 0.0) SVGR_LAUNCH(k_spin, dim3(1), dim3(1), 0, ctx->stream, (unsigned long long)(hold_ms * 1e5));
    HIPCHK(hipEventRecord(ctx->meas_ev[0], ctx->stream));
    return 0;
}
int svgr_measure_end(svgr_ctx* ctx, double* ms) {
    if (!ctx || !ms || !ctx->meas_ev[0]) return fail(SVGR_E_INVALID, "bad arguments");
    HIPCHK(enter_ctx(ctx));
    HIPCHK(hipEventRecord(ctx->meas_ev[1], ctx->stream));
    HIPCHK(hipEventSynchronize(ctx->meas_ev[1]));
    float f = 0.f;
    HIPCHK(hipEventElapsedTime(&f, ctx->meas_ev[0], ctx->meas_ev[1]));
    *ms = (double)f;
    return 0;
}

int svgr_device_name(svgr_ctx* ctx, char* out, size_t cap) {
    if (!ctx || !out || cap == 0) return fail(SVGR_E_INVALID, "bad arguments");
    snprintf(out, cap, "%s", ctx->name);
    return 0;
}

int svgr_buf_alloc(svgr_ctx* ctx, size_t bytes, svgr_buf** out) {
    if (!ctx || !out) return fail(SVGR_E_INVALID, "bad arguments");
    *out = nullptr;
    svgr_buf* b = new (std::nothrow) svgr_buf();
    if (!b) return fail(SVGR_E_NOMEM, "out of host memory");
    HIPCHK(enter_ctx(ctx));
    hipError_t e = g_pool.alloc(&b->ptr, bytes ? bytes : 16, ctx->device);
    if (e != hipSuccess) { delete b; return fail(SVGR_E_NOMEM, "hipMalloc(%zu): %s", bytes, hipGetErrorString(e)); }
    b->bytes = bytes;
    b->owned = true;
    *out = b;
    return 0;
}

int svgr_buf_wrap(svgr_ctx* ctx, void* device_ptr, size_t bytes, svgr_buf** out) {
    if (!ctx || !out || !device_ptr) return fail(SVGR_E_INVALID, "bad arguments");
    svgr_buf* b = new (std::nothrow) svgr_buf();
    if (!b) return fail(SVGR_E_NOMEM, "out of host memory");
    b->ptr = device_ptr;
    b->bytes = bytes;
    b->owned = false;
    *out = b;
    return 0;
}

int svgr_buf_free(svgr_ctx* ctx, svgr_buf* buf) {
    if (!buf) return 0;
    (void)ctx;
    if (buf->owned && buf->ptr) g_pool.release(buf->ptr);  // stream order protects the next user of the block
    delete buf;
    return 0;
}

void* svgr_buf_ptr(const svgr_buf* buf) { return buf ? buf->ptr : nullptr; }
size_t svgr_buf_bytes(const svgr_buf* buf) { return buf ? buf->bytes : 0; }

int svgr_buf_zero(svgr_ctx* ctx, svgr_buf* buf) {
    if (!ctx || !buf) return fail(SVGR_E_INVALID, "bad arguments");
    HIPCHK(enter_ctx(ctx));
    HIPCHK(hipMemsetAsync(buf->ptr, 0, buf->bytes, ctx->stream));
    return 0;
}

int svgr_buf_copy(svgr_ctx* ctx, svgr_buf* dst, const svgr_buf* src, size_t bytes) {
    if (!ctx || !dst || !src) return fail(SVGR_E_INVALID, "bad arguments");
    if (bytes > dst->bytes || bytes > src->bytes) return fail(SVGR_E_INVALID, "copy of %zu bytes overruns a buffer", bytes);
    if (bytes == 0) return 0;
    HIPCHK(enter_ctx(ctx));
    HIPCHK(hipMemcpyAsync(dst->ptr, src->ptr, bytes, hipMemcpyDeviceToDevice, ctx->stream));
    return 0;
}

int svgr_upload(svgr_ctx* ctx, svgr_buf* dst, size_t dst_off, const void* host, size_t bytes) {
    if (!ctx || !dst || (!host && bytes)) return fail(SVGR_E_INVALID, "bad arguments");
    if (dst_off + bytes > dst->bytes) return fail(SVGR_E_INVALID, "upload of %zu bytes at %zu overruns a %zu byte buffer", bytes, dst_off, dst->bytes);
    if (bytes == 0) return 0;
    HIPCHK(enter_ctx(ctx));
    HIPCHK(hipMemcpyAsync((char*)dst->ptr + dst_off, host, bytes, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));  // host buffer is caller-owned and may be reused at once
    return 0;
}

int svgr_download(svgr_ctx* ctx, const svgr_buf* src, size_t src_off, void* host, size_t bytes) {
    if (!ctx || !src || (!host && bytes)) return fail(SVGR_E_INVALID, "bad arguments");
    if (src_off + bytes > src->bytes) return fail(SVGR_E_INVALID, "download of %zu bytes at %zu overruns a %zu byte buffer", bytes, src_off, src->bytes);
    if (bytes == 0) return 0;
    HIPCHK(enter_ctx(ctx));
    HIPCHK(hipMemcpyAsync(host, (const char*)src->ptr + src_off, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    HIPCHK(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------
// batch
// ---------------------------------------------------------------------------------------------
static int batch_create_impl(svgr_ctx* ctx, const svgr_batch_desc* d, svgr_batch** out);
int svgr_batch_create(svgr_ctx* ctx, const svgr_batch_desc* d, svgr_batch** out) {
    return abi_guard("svgr_batch_create", [&]() { return batch_create_impl(ctx, d, out); });
}

static int batch_create_impl(svgr_ctx* ctx, const svgr_batch_desc* d, svgr_batch** out) {
    if (!ctx || !d || !out) return fail(SVGR_E_INVALID, "bad arguments");
    *out = nullptr;
    if (d->n_paths <= 0 || d->n_segs < 0) return fail(SVGR_E_INVALID, "batch needs at least one path");
    if (d->n_segs > 0x3fffffff || d->n_paths > 0x3fffffff) return fail(SVGR_E_INVALID, "batch too large");
    if (!d->path_seg_off || !d->path_m6 || !d->path_rule || !d->path_paint || (d->n_segs && (!d->segs || !d->seg_kind)))
        return fail(SVGR_E_INVALID, "NULL array in batch description");
    for (int64_t p = 0; p < d->n_paths; ++p) {
        if (d->path_seg_off[p] > d->path_seg_off[p + 1]) return fail(SVGR_E_INVALID, "path_seg_off not monotone at %lld", (long long)p);
        if (d->path_rule[p] > 7) return fail(SVGR_E_INVALID, "Invalid fill rule: %d", (int)d->path_rule[p]);  // S:989
        if ((d->path_rule[p] & SVGR_PATH_CLIPPED) && (p == 0 || !(d->path_rule[p - 1] & SVGR_PATH_CLIP_SOURCE)))
            return fail(SVGR_E_INVALID, "path %lld is marked clipped but path %lld is not a clip source", (long long)p, (long long)p - 1);
    }
    if (d->path_seg_off[0] != 0 || d->path_seg_off[d->n_paths] != d->n_segs) return fail(SVGR_E_INVALID, "path_seg_off does not span segs");
    if (!(d->flatness > 0.0) || !std::isfinite(d->flatness)) return fail(SVGR_E_INVALID, "flatness must be positive");
    if (d->viewport[2] > 0 && (d->viewport[3] <= 0 || d->viewport[2] > (1 << 24) || d->viewport[3] > (1 << 24) ||
                               std::llabs(d->viewport[0]) > (1 << 28) || std::llabs(d->viewport[1]) > (1 << 28)))
        return fail(SVGR_E_INVALID, "viewport out of range");

    HIPCHK(enter_ctx(ctx));
    svgr_batch* b = new (std::nothrow) svgr_batch();
    if (!b) return fail(SVGR_E_NOMEM, "out of host memory");
    b->ctx = ctx;
    b->n_segs = d->n_segs;
    b->n_paths = d->n_paths;
    b->has_vp = d->viewport[2] > 0;
    for (int i = 0; i < 4; ++i) b->vp[i] = b->has_vp ? (int)d->viewport[i] : 0;
    b->thr = (d->flatness * d->flatness) * 16.0;  // S:2093
    for (int64_t p = 0; p < d->n_paths; ++p) b->has_clips = b->has_clips || (d->path_rule[p] & (SVGR_PATH_CLIP_SOURCE | SVGR_PATH_CLIPPED));
    b->host_rule.assign(d->path_rule, d->path_rule + d->n_paths);
    const size_t ns = (size_t)d->n_segs, np = (size_t)d->n_paths;
    int rc = 0;
    // The inputs travel as ONE host blob -> ONE device block (six small pageable copies cost more than the data): the blob
    // is a member of the batch, so the copy needs no host wait; the device arrays are views into the block.
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t o_segs = 0, o_m6 = al(o_segs + ns * 64), o_paint = al(o_m6 + np * 48), o_spath = al(o_paint + np * 32),
                 o_kind = al(o_spath + ns * 4), o_rule = al(o_kind + ns), o_seg0 = al(o_rule + np), total = al(o_seg0 + (np + 1) * 4);
    // (packed into the context's page-locked staging when there is one; else into a host image the batch keeps)
    char* hb = (char*)upload_stage(ctx, total);
    const bool staged = hb != nullptr;
    if (!staged) { b->in_host.resize(total); hb = b->in_host.data(); }
    b->o_m6 = o_m6;
    memcpy(hb + o_segs, d->segs, ns * 64);
    memcpy(hb + o_m6, d->path_m6, np * 48);
    memcpy(hb + o_paint, d->path_paint, np * 32);
    {
        int* sp = (int*)(hb + o_spath);
        for (size_t p = 0; p < np; ++p)
            for (int64_t s = d->path_seg_off[p]; s < d->path_seg_off[p + 1]; ++s) sp[(size_t)s] = (int)p;
    }
    memcpy(hb + o_kind, d->seg_kind, ns);
    memcpy(hb + o_rule, d->path_rule, np);
    {
        int* s0 = (int*)(hb + o_seg0);
        for (size_t p = 0; p <= np; ++p) s0[p] = (int)d->path_seg_off[p];
    }
    {
        // non-finite input is refused here (one pass without early exits over the copy just made; the slow loops only name what it found)
        auto nonfin = [](uint64_t x) -> uint64_t { return ((x >> 52) & 0x7ffu) == 0x7ffu; };
        const uint64_t* u = (const uint64_t*)(hb + o_segs);   // (the copy just made: in the cache)
        uint64_t bad = 0, bad_kind = 0;
        for (int64_t s = 0; s < d->n_segs; ++s) {
            const uint64_t lo = nonfin(u[8 * s]) | nonfin(u[8 * s + 1]) | nonfin(u[8 * s + 2]) | nonfin(u[8 * s + 3]);
            const uint64_t hi = nonfin(u[8 * s + 4]) | nonfin(u[8 * s + 5]) | nonfin(u[8 * s + 6]) | nonfin(u[8 * s + 7]);
            bad |= lo | (hi & (uint64_t)(d->seg_kind[s] == SVGR_SEG_CUBIC));
            bad_kind |= (uint64_t)(d->seg_kind[s] > 1);
        }
        if (bad | bad_kind)
            for (int64_t s = 0; s < d->n_segs; ++s) {
                if (d->seg_kind[s] > 1) { delete b; return fail(SVGR_E_INVALID, "unsupported path type: `%d`", (int)d->seg_kind[s]); }  // S:945
                int npts = d->seg_kind[s] == SVGR_SEG_CUBIC ? 8 : 4;
                for (int k = 0; k < npts; ++k)
                    if (!std::isfinite(d->segs[8 * s + k])) { delete b; return fail(SVGR_E_INVALID, "non-finite coordinate in segment %lld", (long long)s); }
            }
        const uint64_t* um = (const uint64_t*)(hb + o_m6);
        uint64_t bad_m = 0;
        for (int64_t i = 0; i < 6 * d->n_paths; ++i) bad_m |= nonfin(um[i]);
        if (bad_m) { delete b; return fail(SVGR_E_INVALID, "non-finite transform"); }
    }
    rc = b->in_dev.ensure(total);
    if (!rc) {
        hipError_t e;
        if (staged) e = upload_staged(ctx, b->in_dev.p, total);
        else {
            e = hipMemcpyAsync(b->in_dev.p, hb, total, hipMemcpyHostToDevice, ctx->stream);
            if (e == hipSuccess) e = b->note_upload(ctx->stream);
        }
        if (e != hipSuccess) rc = fail(SVGR_E_HIP, "upload: %s", hipGetErrorString(e));
    }
    if (!rc) {
        b->segs.point_at(b->in_dev.p, o_segs, ns * 8 ? ns * 8 : 1);
        b->path_m6.point_at(b->in_dev.p, o_m6, np * 6);
        b->path_paint.point_at(b->in_dev.p, o_paint, np * 4);
        b->seg_path.point_at(b->in_dev.p, o_spath, ns ? ns : 1);
        b->seg_kind.point_at(b->in_dev.p, o_kind, ns ? ns : 1);
        b->path_rule.point_at(b->in_dev.p, o_rule, np);
        b->path_seg0.point_at(b->in_dev.p, o_seg0, np + 1);
    }
    rc = rc ? rc : b->bbox.ensure(4 * np);
    rc = rc ? rc : b->bins.ensure(np + 1);
    rc = rc ? rc : b->layout_arena();
    if (rc) { delete b; return rc; }
    *out = b;
    return 0;
}

int svgr_batch_destroy(svgr_batch* b) {
    if (!b) return 0;
    (void)enter_ctx(b->ctx);
    // (kernels still in flight only touch device blocks, and those go back to this context's cache, whose next user is behind
    //  them on the same stream; what must not go away under a running copy is the batch's HOST memory)
    b->wait_uploads();
    spare_stash(b);
    delete b;
    return 0;
}

int svgr_batch_set_paints(svgr_batch* b, const double* path_paint) {
    if (!b || !path_paint) return fail(SVGR_E_INVALID, "bad arguments");
    HIPCHK(enter_ctx(b->ctx));
    b->wait_uploads();  // (a repeated call: the previous copy of the array may still be the source of a running upload)
    HIPCHK(hipMemcpyAsync(b->path_paint.p, b->keep(path_paint, sizeof(double) * 4 * (size_t)b->n_paths), sizeof(double) * 4 * b->n_paths,
                          hipMemcpyHostToDevice, b->ctx->stream));
    HIPCHK(b->note_upload(b->ctx->stream));
    b->geometry_fresh = false; b->geometry_current = false;  // the cell headers carry the paint
    b->plan.paints_changed();
    return 0;
}

int svgr_batch_set_transforms(svgr_batch* b, const double* path_m6) {
    if (!b || !path_m6) return fail(SVGR_E_INVALID, "bad arguments");
    for (int64_t i = 0; i < 6 * b->n_paths; ++i)
        if (!std::isfinite(path_m6[i])) return fail(SVGR_E_INVALID, "non-finite transform");
    HIPCHK(enter_ctx(b->ctx));
    const size_t mbytes = sizeof(double) * 6 * (size_t)b->n_paths;
    if (void* hs = upload_stage(b->ctx, mbytes)) {
        memcpy(hs, path_m6, mbytes);
        HIPCHK(upload_staged(b->ctx, b->path_m6.p, mbytes));
    } else {
        b->wait_uploads();
        HIPCHK(hipMemcpyAsync(b->path_m6.p, b->keep(path_m6, mbytes), mbytes, hipMemcpyHostToDevice, b->ctx->stream));
        HIPCHK(b->note_upload(b->ctx->stream));
    }
    b->plan.geometry_changed();
    b->hit_ready = false;
    return 0;
}

int svgr_batch_set_bands(svgr_batch* b, int rank, int world, int strip_bands) {
    if (!b || world <= 0 || rank < 0 || rank >= world || strip_bands <= 0) return fail(SVGR_E_INVALID, "bad band selection");
    b->own = Owner{rank, world, strip_bands};
    b->plan.geometry_changed();  // the edge / record capacities are per rank
    b->sized = false;
    b->n_seg_list = -1;  // ... and so is the list of segments to flatten
    return 0;
}

// Isolated groups (Scene.render CLIP / OPACITY over a GROUP of solid fills, S:674-715) inside one batch: the members of a
// group are consecutive paths; when the group closes it is multiplied by the coverage of its clip source (the path right
// in front of its first member) and / or by its opacity, and composited OVER the canvas as a whole.
int svgr_batch_set_groups(svgr_batch* b, const int32_t* path_group, int64_t n_groups, const int32_t* group_clip_src,
                          const double* group_opacity) {
    return abi_guard("svgr_batch_set_groups", [&]() -> int {
        if (!b) return fail(SVGR_E_INVALID, "batch is NULL");
        if (n_groups == 0) { b->n_groups = 0; b->geometry_fresh = false; b->geometry_current = false; return 0; }
        if (n_groups < 0 || n_groups > b->n_paths || !path_group || !group_clip_src || !group_opacity)
            return fail(SVGR_E_INVALID, "svgr_batch_set_groups: bad arguments");
        std::vector<int64_t> first((size_t)n_groups, -1), last((size_t)n_groups, -1);
        for (int64_t p = 0; p < b->n_paths; ++p) {
            const int g = path_group[p];
            if (g < -1 || g >= n_groups) return fail(SVGR_E_INVALID, "path %lld: group %d out of range", (long long)p, g);
            if (g < 0) continue;
            if (b->host_rule[(size_t)p] & (SVGR_PATH_CLIP_SOURCE | SVGR_PATH_CLIPPED))
                return fail(SVGR_E_INVALID, "path %lld: a group member cannot be a clip source or a clipped path itself", (long long)p);
            if (first[(size_t)g] < 0) first[(size_t)g] = p;
            else if (last[(size_t)g] != p - 1) return fail(SVGR_E_INVALID, "group %d: members must be consecutive paths", g);
            last[(size_t)g] = p;
        }
        for (int64_t g = 0; g < n_groups; ++g) {
            if (first[(size_t)g] < 0) return fail(SVGR_E_INVALID, "group %lld has no member", (long long)g);
            const int cs = group_clip_src[g];
            if (cs != -1 && (cs != first[(size_t)g] - 1 || !(b->host_rule[(size_t)cs] & SVGR_PATH_CLIP_SOURCE)))
                return fail(SVGR_E_INVALID, "group %lld: its clip source must be the path right in front of its first member", (long long)g);
            if (!std::isfinite(group_opacity[g])) return fail(SVGR_E_INVALID, "group %lld: opacity is not finite", (long long)g);
        }
        HIPCHK(enter_ctx(b->ctx));
        {
            // one host blob -> one device block (three small pageable copies cost more than the data); the arrays are the
            // caller's: the upload reads the copy the batch keeps
            auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
            const size_t np = (size_t)b->n_paths, ng = (size_t)n_groups;
            const size_t o_pg = 0, o_cs = al(o_pg + np * 4), o_op = al(o_cs + ng * 4), total = al(o_op + ng * 8);
            std::vector<char> blob(total, 0);
            memcpy(blob.data() + o_pg, path_group, np * 4);
            memcpy(blob.data() + o_cs, group_clip_src, ng * 4);
            memcpy(blob.data() + o_op, group_opacity, ng * 8);
            b->path_group.release(); b->group_clip_src.release(); b->group_opacity.release();
            if (int rc = b->groups_dev.ensure(total)) return rc;
            b->path_group.point_at(b->groups_dev.p, o_pg, np);
            b->group_clip_src.point_at(b->groups_dev.p, o_cs, ng);
            b->group_opacity.point_at(b->groups_dev.p, o_op, ng);
            hipStream_t st = b->ctx->stream;
            HIPCHK(hipMemcpyAsync(b->groups_dev.p, b->keep(blob.data(), total), total, hipMemcpyHostToDevice, st));
            HIPCHK(b->note_upload(st));
        }
        b->n_groups = n_groups;
        b->geometry_fresh = false; b->geometry_current = false;  // the cell headers carry the group ids
        return 0;
    });
}

// Gradient paints inside a batch (Path.fill's gradient branch, S:1021-1047, for userSpaceOnUse gradients of up to 32 stops):
// path_grad[p] = index into `grads` or -1 (solid colour).  A gradient entry's colour is evaluated per visible pixel by the
// tile kernel -- image = gradient(pixel centre) * coverage -- and multiplied by the entry's path_paint (1 everywhere, or
// the opacity of an OPACITY node directly above the leaf).  grads[i].user_m6 maps pixel centres to the gradient's user
// space exactly as for svgr_gradient_fill.
int svgr_batch_set_gradients(svgr_batch* b, const int32_t* path_grad, int64_t n_grads, const svgr_gradient* grads) {
    return abi_guard("svgr_batch_set_gradients", [&]() -> int {
        if (!b) return fail(SVGR_E_INVALID, "batch is NULL");
        if (n_grads == 0) { b->n_grads = 0; b->host_path_grad.clear(); b->geometry_fresh = false; b->geometry_current = false; return 0; }
        if (n_grads < 0 || n_grads > b->n_paths || !path_grad || !grads) return fail(SVGR_E_INVALID, "svgr_batch_set_gradients: bad arguments");
        std::vector<GradDev> host((size_t)n_grads);
        std::vector<int> owner((size_t)n_grads, -1);
        bool focal = false;
        for (int64_t i = 0; i < n_grads; ++i) {
            if (int rc = check_gradient(&grads[i])) return rc;
            if (grads[i].n_stops > GRAD_MAX_STOPS)
                return fail(SVGR_E_INVALID, "gradient %lld has %d stops: more than %d go through svgr_gradient_fill", (long long)i, grads[i].n_stops, GRAD_MAX_STOPS);
            fill_grad_dev(host[(size_t)i], &grads[i]);
            for (int k = 0; k < grads[i].n_stops; ++k) {
                host[(size_t)i].stop_off[k] = grads[i].stop_off[k];
                for (int c = 0; c < 4; ++c) host[(size_t)i].stop_rgba[k][c] = grads[i].stop_rgba[4 * k + c];
            }
            focal = focal || grads[i].kind == 3;
        }
        for (int64_t p = 0; p < b->n_paths; ++p) {
            const int gi = path_grad[p];
            if (gi < -1 || gi >= n_grads) return fail(SVGR_E_INVALID, "path %lld: gradient %d out of range", (long long)p, gi);
            if (gi < 0) continue;
            if (b->host_rule[(size_t)p] & SVGR_PATH_CLIP_SOURCE) return fail(SVGR_E_INVALID, "path %lld: a clip source has no paint", (long long)p);
            if (owner[(size_t)gi] >= 0) return fail(SVGR_E_INVALID, "gradient %d is used by two paths (one description per fill: its transform is the fill's)", gi);
            owner[(size_t)gi] = (int)p;
        }
        for (int64_t i = 0; i < n_grads; ++i)
            if (owner[(size_t)i] < 0) return fail(SVGR_E_INVALID, "gradient %lld is not used by any path", (long long)i);
        HIPCHK(enter_ctx(b->ctx));
        {
            // one host blob -> one device block, as for the groups
            auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
            const size_t np = (size_t)b->n_paths, ng = (size_t)n_grads;
            const size_t o_g = 0, o_pg = al(o_g + ng * sizeof(GradDev)), o_gp = al(o_pg + np * 4), total = al(o_gp + ng * 4);
            std::vector<char> blob(total, 0);
            memcpy(blob.data() + o_g, host.data(), ng * sizeof(GradDev));
            memcpy(blob.data() + o_pg, path_grad, np * 4);
            memcpy(blob.data() + o_gp, owner.data(), ng * 4);
            b->grads.release(); b->path_grad.release(); b->grad_path.release();
            if (int rc = b->grads_dev.ensure(total)) return rc;
            b->grads.point_at(b->grads_dev.p, o_g, ng);
            b->path_grad.point_at(b->grads_dev.p, o_pg, np);
            b->grad_path.point_at(b->grads_dev.p, o_gp, ng);
            if (int rc = b->grad_flags.ensure(ng)) return rc;
            hipStream_t st = b->ctx->stream;
            HIPCHK(hipMemcpyAsync(b->grads_dev.p, b->keep(blob.data(), total), total, hipMemcpyHostToDevice, st));
            HIPCHK(b->note_upload(st));
        }
        // (the cell headers carry the gradient indices: a new assignment of gradients to paths needs the geometry pass again; new
        //  descriptions for the same assignment -- the frames of objectBoundingBox paints, known once the plan has flattened their
        //  paths -- do not, nor do they touch what the plan's pass left in the buffers)
        const bool same_map = b->n_grads == n_grads && b->host_path_grad.size() == (size_t)b->n_paths &&
                              memcmp(b->host_path_grad.data(), path_grad, sizeof(int32_t) * (size_t)b->n_paths) == 0 && b->has_focal == focal;
        b->host_path_grad.assign(path_grad, path_grad + b->n_paths);
        b->n_grads = n_grads;
        b->has_focal = focal;
        if (!same_map) { b->geometry_fresh = false; b->geometry_current = false; }
        return 0;
    });
}

// Small batches (Path.mask / Path.fill of one path, a handful of glyphs): instead of the staged plan with a read-back
// per stage, size every buffer from bounds known on the host -- (path, band) pairs <= paths x bands exactly, edges and
// records by a generous guess -- run the whole geometry ONCE and read the counters back once.  If a guess was too
// small the kernels flag it and the staged plan takes over.  Returns 1 when it planned, 0 to fall back, < 0 on error.
// Two halves, so that svgr_batch_plan_many can put the passes of many batches behind ONE wait: spec_issue enqueues the pass
// and its read-back (1 issued, 0 not eligible), spec_finish reads the verdict once the stream has drained.
// `again`: the batch has been planned before with this viewport (svgr_batch_set_transforms / set_paints voided that plan): the
// capacities are what its buffers hold -- the last plan's exact counts plus the eighth every allocation adds --, whatever the
// batch's size.  A drawing that moved a little fits them; one that does not is flagged and takes the staged plan, like any
// other wrong guess.  (A re-plan is then two geometry passes behind ONE read-back instead of five passes and five: VERDICT r3 #3.)
static int spec_issue(svgr_batch* b, void* staging = nullptr, bool again = false) {
    const int np = (int)b->n_paths;
    const int64_t ns = b->n_segs;
    if (!b->has_vp || ns <= 0 || np <= 0 || b->own.world > 1) return 0;
    if (again) {
        if (!b->sized) (void)spare_adopt(b);   // (a new batch: the work arrays of the context's last large batch, if they fit its shape)
        if (!b->sized || b->sized_vp[0] != b->vp[0] || b->sized_vp[1] != b->vp[1] || b->sized_vp[2] != b->vp[2] || b->sized_vp[3] != b->vp[3]) return 0;
        b->n_edges = (int64_t)(b->edges.cap / 4);
        for (int k = 0; k < NSH; ++k) {
            b->shards.base[k] = k == 0 ? 0 : (int)b->n_edges;
            b->shards.cap[k] = k == 0 ? (int)b->n_edges : 0;
        }
        b->n_pb = (int64_t)std::min(b->entries.cap, b->pair_idx.cap);
        b->n_entries = b->n_pb;
        if (b->cell_plan.cap == 0) return 0;
        b->n_cells = (int64_t)std::min(std::min(b->cell_hdr.cap, b->cell_plan.cap) - 1, b->items.cap);
        b->n_slabs = (int64_t)b->slabs.cap;
        if (b->n_edges <= 0 || b->n_pb <= 0 || b->n_cells <= 0 || b->n_slabs <= 0 || b->edge_path.cap < (size_t)b->n_edges) return 0;
        int rc = b->layout_arena();
        if (rc) return rc;
        // ONE flatten traversal (k_flatten<.., SCAN>: count, look-back, store) when the last plan left arrays for its by-products;
        // else the counting pass + prefix sums in front of the storing one
        b->fl_sub = choose_fl_sub(b, (int)ns);   // (as the counting pass would choose it: the lanes' places follow it)
        const bool scan = !b->safe_path && getenv("SVGR_SAFE_PATH") == nullptr && b->seg_cnt.cap >= (size_t)ns + 1 &&
                          b->seg_off.cap >= (size_t)ns + 2 && b->lane_off.cap >= ((size_t)ns << b->fl_sub) + 1;
        if (!scan && (rc = run_geometry(b, 1, true))) return rc;
        b->fl_scan = scan;
        rc = run_geometry(b, 4, true);
        b->fl_scan = false;
        if (rc) return rc;
        if ((rc = issue_readback(b, true, staging))) return rc;
        return 1;
    }
    if (ns > 4096) return 0;
    const int n_bands = (b->vp[2] + TR - 1) / TR;
    if ((int64_t)np * n_bands > (1 << 20) || n_bands <= 0) return 0;
    const int n_ct = (b->vp[3] + TC - 1) / TC + 1;  // (+1: a layer need not start on a tile border)
    // Two size models.  Up to 256 segments (Path.mask / Path.fill of one path, a handful of glyphs): bounds that cannot be
    // exceeded except by absurd input.  Up to 4096 segments (the runs of a document's per-node route): guesses a few times
    // the typical need -- a wrong one costs the staged plan, never a wrong picture.
    const bool small = ns <= 256;
    // (tests: SVGR_SPEC_SHRINK="e,c,s,a" divides the guesses for edges, cells, slabs and add slots, so that each overflow path
    //  can be driven on purpose: the kernels must flag it and the staged plan must take over)
    long long shrink[4] = {1, 1, 1, 1};
    if (const char* sk = getenv("SVGR_SPEC_SHRINK")) sscanf(sk, "%lld,%lld,%lld,%lld", &shrink[0], &shrink[1], &shrink[2], &shrink[3]);
    for (auto& v : shrink) v = v < 1 ? 1 : v;
    const int64_t edge_guess = std::max<int64_t>((small ? 1024 * ns : 128 * ns + 8192) / shrink[0], 1);
    b->n_edges = edge_guess;
    for (int k = 0; k < NSH; ++k) {  // (the renders' edge array is one dense block: see k_flatten)
        b->shards.base[k] = k == 0 ? 0 : (int)b->n_edges;
        b->shards.cap[k] = k == 0 ? (int)b->n_edges : 0;
    }
    b->n_bands = n_bands;
    b->n_pb = (int64_t)np * n_bands;
    b->n_cells = std::min<int64_t>(b->n_pb * n_ct, std::max<int64_t>(262144, small ? 0 : 4 * b->n_pb));  // (overflow is flagged)
    b->n_cells = std::max<int64_t>(b->n_cells / shrink[1], 1);
    b->n_entries = b->n_pb;
    // slabs: at most one per (path, band) and run of PB_CELLS column tiles; typically one or two per path
    b->n_slabs = std::min<int64_t>(b->n_pb * ((n_ct + PB_CELLS - 1) / PB_CELLS), 64 * (int64_t)np + 1024);
    b->n_slabs = std::max<int64_t>(b->n_slabs / shrink[2], 1);
    const int64_t row_guess = small ? 16 * edge_guess + b->n_pb : 256 * ns + 4096;  // edge rows
    int rc = b->layout_arena();
    rc = rc ? rc : b->edges.ensure((size_t)b->n_edges * 4);
    rc = rc ? rc : b->edge_path.ensure((size_t)b->n_edges);
    rc = rc ? rc : b->band_start.ensure((size_t)n_bands + 1);
    rc = rc ? rc : b->band_count.ensure((size_t)n_bands + 1);
    rc = rc ? rc : b->entries.ensure((size_t)b->n_pb);
    rc = rc ? rc : b->pair_idx.ensure((size_t)b->n_pb);
    rc = rc ? rc : b->slabs.ensure((size_t)b->n_slabs);
    rc = rc ? rc : b->cell_hdr.ensure((size_t)b->n_cells + 1);
    rc = rc ? rc : b->cell_plan.ensure((size_t)b->n_cells + 1);
    rc = rc ? rc : b->size_tile_lists(n_bands);
    if (!rc) {
        // add slots: a guess like the others -- a few adds per edge row.  Few slabs: one shard (a batch of one slab would put
        // everything into its shard); more: four
        const int n_sh = small ? 1 : 4;
        int need[NSH];
        for (int k = 0; k < NSH; ++k) need[k] = (int)(std::min<int64_t>(4 * row_guess / (small ? 1 : 2) + 2048, 1 << 26) / shrink[3]);
        rc = b->size_adds(need, n_sh);
        b->adds_roomy = true;
    }
    rc = rc ? rc : b->size_masks(np);
    if (rc) return rc;
    // the per-segment edge counts and their prefix sums, then the whole geometry: both passes behind one read-back
    if ((rc = run_geometry(b, 1, true))) return rc;
    if ((rc = run_geometry(b, 4, true))) return rc;
    if ((rc = issue_readback(b, true, staging))) return rc;
    return 1;
}
// 1 planned, 0 a guess was too small (the staged plan takes over), < 0 error
static int spec_finish(svgr_batch* b) {
    int cap_bits = 0;
    if (b->host_bd.err) b->invalidate_work();
    if (getenv("SVGR_DBG_PLAN")) {   // (diagnostic: what the single pass was given and what it used)
        long long e = 0, a = 0;
        for (int k = 0; k < NSH; ++k) { e += b->host_bd.shard[k].cursor; a += b->host_bd.shard[k].add_cursor; }
        fprintf(stderr, "[plan] single pass: err %d | edges %lld of %lld, pairs %d of %lld, cells %d of %lld, slabs %d of %lld, adds %lld of %lld (shard 0: %d of %d), entries %d, longest band list %d (mask words %d)\n",
                b->host_bd.err, e, (long long)b->n_edges, b->host_bd.pb_cursor, (long long)b->n_pb, b->host_bd.cell_cursor, (long long)b->n_cells,
                b->host_bd.slab_cursor, (long long)b->n_slabs, a, (long long)b->n_adds, b->host_bd.shard[0].add_cursor, b->add_shards.cap[0],
                b->host_bd.entry_cursor, b->host_bd.max_band_entries, b->mask_words);
    }
    if (int rc = eval_dev_err(b->host_bd.err, &cap_bits)) return rc;
    if (cap_bits) return 0;
    b->n_entries = b->host_bd.entry_cursor;
    b->n_pb = b->host_bd.pb_cursor;    // (the pass ran on capacities: the statistics report what it found)
    b->n_slabs = b->host_bd.slab_cursor;
    b->n_edges_live = 0;
    for (int k = 0; k < NSH; ++k) b->n_edges_live += b->host_bd.shard[k].cursor;
    b->n_bsegs = b->host_bd.bseg_cursor;
    b->plan.plan_made();
    b->sized = true;
    for (int k = 0; k < 4; ++k) b->sized_vp[k] = b->vp[k];
    b->read_switches();
    b->geometry_fresh = true; b->geometry_current = true;
    return 1;
}
static int plan_slab_order(svgr_batch* b);
static int plan_speculative(svgr_batch* b) {
    // (first choice: the sizes of the batch's own last plan; then the size models for small batches)
    for (int again = 1; again >= 0; --again) {
        const int is = spec_issue(b, nullptr, again != 0);
        if (is < 0) return is;
        if (is == 0) continue;
        HIPCHK(hipStreamSynchronize(b->ctx->stream));
        HIPCHK(hipGetLastError());
        const int fin = spec_finish(b);
        if (fin > 0 && b->n_segs > 4096) {
            if (int rc = plan_slab_order(b)) return rc;   // (large batches: k_path_build's work list heaviest first)
        }
        if (fin != 0) return fin;
        b->plan.pass_withdrawn();
    }
    return 0;
}

// k_path_rows + k_seg_select + one read-back: b->seg_list / b->n_seg_list
static int build_seg_list(svgr_batch* b) {
    hipStream_t st = b->ctx->stream;
    const int ns = (int)b->n_segs;
    if (int rc = b->seg_list.ensure((size_t)ns)) return rc;
    HIPCHK(hipMemsetAsync(b->arena.p, 0, b->arena_bytes, st));
    b->arena_zeroed = false;
    SVGR_LAUNCH(k_path_rows, grid1((size_t)ns), dim3(256), 0, st, (const double*)b->segs.p, (const uint8_t*)b->seg_kind.p,
                       (const int*)b->seg_path.p, (const double*)b->path_m6.p, ns, b->prow());
    SVGR_LAUNCH(k_seg_select, grid1((size_t)ns), dim3(256), 0, st, (const int*)b->seg_path.p, ns, (const unsigned*)b->prow(), b->own,
                       b->vp[0], (b->vp[2] + TR - 1) / TR, b->seg_list.p, &b->bd()->edge_spare);
    int n = 0;
    std::vector<unsigned> reach(2 * (size_t)b->n_paths);
    HIPCHK(hipMemcpyAsync(&n, &b->bd()->edge_spare, sizeof n, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(reach.data(), b->prow(), sizeof(unsigned) * reach.size(), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipGetLastError());
    b->n_seg_list = n;
    // the same test per path, in path = paint order (the band lists keep that order)
    const int n_bands = (b->vp[2] + TR - 1) / TR, vr0 = b->vp[0];
    std::vector<int> mine;
    for (int64_t p = 0; p < b->n_paths; ++p) {
        if (reach[2 * (size_t)p] == 0u) continue;  // (no segment)
        const int lo = UNION_BIAS - (int)reach[2 * (size_t)p], hi = (int)reach[2 * (size_t)p + 1] - UNION_BIAS;
        int ba = (lo - 2 - vr0) / TR, bb = (hi + 2 - vr0) / TR;
        ba = lo - 2 - vr0 < 0 ? 0 : ba;
        bb = bb > n_bands - 1 ? n_bands - 1 : bb;
        if (ba <= bb && owns_any(b->own, ba, bb)) mine.push_back((int)p);
    }
    b->n_path_list = (int64_t)mine.size();
    if (int rc = b->path_list.ensure(mine.size() + 1)) return rc;
    if (!mine.empty()) HIPCHK(hipMemcpyAsync(b->path_list.p, mine.data(), sizeof(int) * mine.size(), hipMemcpyHostToDevice, st));
    // the paths that are not on the list keep an empty bbox and no bands for good
    HIPCHK(hipMemsetAsync(b->bbox.p, 0, sizeof(int) * 4 * (size_t)b->n_paths, st));
    HIPCHK(hipMemsetAsync(b->bins.p, 0, sizeof(PathBin) * (size_t)b->n_paths, st));
    HIPCHK(hipStreamSynchronize(st));  // (`mine` is a host vector of this call)
    return 0;
}

static int batch_plan_impl(svgr_batch* b, bool skip_speculative = false);
int svgr_batch_plan(svgr_batch* b) {
    return abi_guard("svgr_batch_plan", [&]() { return batch_plan_impl(b); });
}

// page-locked staging of at least `bytes` for this context's read-backs (the stream is drained before a smaller one is replaced)
static int ensure_pinned(svgr_ctx* c, size_t bytes) {
    if (c->pinned_bytes >= bytes) return 0;
    HIPCHK(hipStreamSynchronize(c->stream));
    if (c->pinned) (void)hipHostFree(c->pinned);
    c->pinned = nullptr;
    c->pinned_bytes = 0;
    const size_t want = std::max<size_t>(bytes + bytes / 2, 1u << 20);
    HIPCHK(hipHostMalloc(&c->pinned, want, hipHostMallocDefault));
    c->pinned_bytes = want;
    return 0;
}

// The plans of many batches behind one wait: a document's per-node route plans dozens of small batches (one per run of
// fills between two filter nodes), and each plan alone is a device round trip of ~0.15 ms of which the kernels are a
// fraction.  Every batch that qualifies for the single-pass plan has its pass enqueued first; then one wait per stream;
// the others, and those whose guesses were too small, are planned one by one as svgr_batch_plan would.
int svgr_batch_plan_many(svgr_batch** batches, int64_t n) {
    return abi_guard("svgr_batch_plan_many", [&]() {
        if (n < 0 || (n > 0 && !batches)) return fail(SVGR_E_INVALID, "bad arguments");
        for (int64_t i = 0; i < n; ++i)
            if (!batches[i]) return fail(SVGR_E_INVALID, "batch %lld is NULL", (long long)i);
        const bool no_spec = getenv("SVGR_NO_SPECULATIVE_PLAN") != nullptr;
        std::vector<char> issued((size_t)n, 0);
        // page-locked staging for every batch's read-back, carved from its context's slab
        std::vector<size_t> stage_off((size_t)n, 0);
        std::map<svgr_ctx*, size_t> stage_need;
        for (int64_t i = 0; i < n; ++i) {
            size_t& need = stage_need[batches[i]->ctx];
            stage_off[(size_t)i] = need;
            need += (sizeof(BatchDev) + 16 * (size_t)batches[i]->n_paths + 255) & ~(size_t)255;
        }
        for (auto& kv : stage_need) {
            HIPCHK(enter_ctx(kv.first));
            if (int rc = ensure_pinned(kv.first, kv.second)) return rc;
        }
        for (int64_t i = 0; i < n; ++i) {
            svgr_batch* b = batches[i];
            HIPCHK(enter_ctx(b->ctx));
            b->plan.plan_begins();
            b->geometry_fresh = false; b->geometry_current = false;
            const int is = no_spec ? 0 : spec_issue(b, (char*)b->ctx->pinned + stage_off[(size_t)i]);
            if (is < 0) return is;
            issued[(size_t)i] = (char)is;
        }
        for (int64_t i = 0; i < n; ++i)
            if (issued[(size_t)i]) {
                HIPCHK(enter_ctx(batches[i]->ctx));
                HIPCHK(hipStreamSynchronize(batches[i]->ctx->stream));  // (a no-op for the later batches of the same stream)
                HIPCHK(hipGetLastError());
                take_readback(batches[i], (const char*)batches[i]->ctx->pinned + stage_off[(size_t)i]);
            }
        for (int64_t i = 0; i < n; ++i) {
            svgr_batch* b = batches[i];
            int done = 0;
            if (issued[(size_t)i]) {
                done = spec_finish(b);
                if (done < 0) return done;
                if (done > 0 && b->n_segs > 4096)
                    if (int rc = plan_slab_order(b)) return rc;
            }
            if (!done)  // (not eligible, or a guess was too small: the staged plan directly -- the speculative pass would fail the same way)
                if (int rc = batch_plan_impl(b, issued[(size_t)i] != 0)) return rc;
        }
        return 0;
    });
}

// Where every path's slabs go in the renders that follow: the paths sorted by the work one of their slabs is (edge rows ~ the
// rows + columns of the part of the bbox it covers), heaviest first.  k_path_bbox's own count of a path's slabs is the same
// integer arithmetic on the same bbox (slab_shape, owns_any), so the places tile the list exactly; the geometry cannot change
// under a plan (set_transforms / set_bands invalidate it).
static int plan_slab_order(svgr_batch* b) {
    b->plan.slab_order_begins();
    if (getenv("SVGR_SAFE_PATH")) return 0;  // (tests: the renders then take their slab places from the cursor, in arrival order)
    const size_t np = (size_t)b->n_paths;
    if (int rc = ensure_host_bbox(b)) return rc;
    if (np == 0 || b->host_bbox.size() < 4 * np || b->n_slabs <= 0 || b->vp[2] <= 0) return 0;
    std::vector<int> n_sl(np, 0), order;
    std::vector<float> w(np, 0.f);
    order.reserve(np);
    long long total = 0;
    for (size_t p = 0; p < np; ++p) {
        const int r0 = b->host_bbox[4 * p], c0 = b->host_bbox[4 * p + 1], rows = b->host_bbox[4 * p + 2], cols = b->host_bbox[4 * p + 3];
        if (rows <= 0 || cols <= 0) continue;
        const int pb0 = (r0 - b->vp[0]) / TR, pnb = (r0 + rows - 1 - b->vp[0]) / TR - pb0 + 1;
        int ct0, pnct;
        path_ctiles(c0, cols, b->vp[1], ct0, pnct);
        if ((long long)pnb * pnct > (1ll << 28)) continue;
        int bands_per, col_runs, n = 0;
        slab_shape(pnb, pnct, bands_per, col_runs);
        for (int bb = 0; bb < pnb; bb += bands_per) {
            const int be = bb + bands_per < pnb ? bb + bands_per : pnb;
            if (owns_any(b->own, pb0 + bb, pb0 + be - 1)) n += col_runs;
        }
        if (n == 0) continue;
        n_sl[p] = n;
        w[p] = (float)std::min(rows, bands_per * TR) + (float)cols / (float)col_runs;
        order.push_back((int)p);
        total += n;
    }
    if (total != b->n_slabs) return 0;  // (not the count the device found: leave the order to the cursor)
    // heaviest first, paint order among equals: a counting sort over the weights in whole pixels (a comparison sort of a few
    // thousand paths was 0.15 ms of a 0.5 ms plan)
    b->slab_at_host.assign(np, 0);
    {
        constexpr int KEYS = 1 << 16;
        std::vector<int> first((size_t)KEYS + 1, 0);
        auto key_of = [&](int p) { const float v = w[(size_t)p]; return KEYS - 1 - (v < (float)(KEYS - 1) ? (int)v : KEYS - 1); };   // (descending)
        for (int p : order) first[(size_t)key_of(p) + 1] += n_sl[(size_t)p];
        for (int k = 0; k < KEYS; ++k) first[(size_t)k + 1] += first[(size_t)k];
        for (int p : order) { const int k = key_of(p); b->slab_at_host[(size_t)p] = first[(size_t)k]; first[(size_t)k] += n_sl[(size_t)p]; }
    }
    if (int rc = b->slab_at.ensure(np)) return rc;
    // (no wait: the renders are behind the copy in the stream; its source is a member, svgr_batch_destroy waits for uploads)
    b->wait_uploads();
    HIPCHK(hipMemcpyAsync(b->slab_at.p, b->slab_at_host.data(), sizeof(int) * np, hipMemcpyHostToDevice, b->ctx->stream));
    HIPCHK(b->note_upload(b->ctx->stream));
    b->plan.slab_order_made();
    return 0;
}

// The FIRST plan of a batch in two passes behind two read-backs (the staged plan below: five and five).
//   pass 1  the counting flatten (per-segment edge counts -> their prefix sums = where every segment's edges go; the rows and
//           columns the kept pieces cross) and k_path_bbox on its min / max keys: the bboxes, and with them -- the kernel's own
//           reservations -- the exact numbers of (path, band) pairs, cells and slabs
//   host    every buffer sized exactly, but the add lists: a guess from the rows / columns crossed and the cells
//   pass 2  the whole geometry (k_path_build<2>: one pass on its own bounds; it leaves every cell's add places): validated by its own error word
// An add-list guess that was too small is flagged by the kernels and the staged plan (which MEASURES the lists) takes over.
// 1 planned, 0 fall back, < 0 error.
static double now_ms() {
    timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec * 1e3 + (double)ts.tv_nsec * 1e-6;
}
// (`staging`: page-locked memory for pass 2's read-back -- svgr_batch_draw puts the tile kernel behind the pass and waits once;
//  two_pass_finish then reads what arrived)
static int two_pass_finish(svgr_batch* b, const void* staging);
static int two_pass_issue(svgr_batch* b, void* staging) {
    const double t_0 = now_ms();
    if (!b->has_vp || b->own.world > 1 || b->n_segs <= 0 || b->vp[2] <= 0 || b->vp[3] <= 0) return 0;
    if (getenv("SVGR_NO_TWO_PASS_PLAN")) return 0;   // (tests: the staged plan stays exercised)
    if (int rc = b->layout_arena()) return rc;
    b->n_seg_list = -1;
    b->census_bbox = true;
    b->census_set = true;      // (counts into the second set of scalars: the first stays zero for pass 2)
    b->late_scan = staging != nullptr && b->ctx->pin_ev != nullptr;
    int rc = run_geometry(b, 1, true);
    b->census_bbox = false;
    const bool late = b->late_scan;
    b->late_scan = false;
    if (!rc && staging) {   // (page-locked: the copy does not block, the wait below is the only one)
        rc = issue_readback(b, true, staging);
        if (!rc) {
            hipError_t e;
            if (late) {
                // the host waits for the read-back alone; the prefix sums pass 2 needs run meanwhile
                e = hipEventRecord(b->ctx->pin_ev, b->ctx->stream);
                SVGR_LAUNCH(k_seg_scan, dim3(1), dim3(1024), 0, b->ctx->stream, (const int*)b->seg_cnt.p, (int)b->n_segs, b->seg_off.p);
                if (e == hipSuccess) e = hipEventSynchronize(b->ctx->pin_ev);
            } else e = hipStreamSynchronize(b->ctx->stream);
            if (e != hipSuccess) rc = fail(SVGR_E_HIP, "census: %s", hipGetErrorString(e));
        }
        if (!rc) {
            take_readback(b, staging);
            if (b->host_bd.err) b->invalidate_work();
            rc = eval_dev_err(b->host_bd.err, nullptr);
        }
    } else if (!rc) rc = check_dev_err(b, nullptr, true, true);
    b->census_set = false;
    b->arena_zeroed = rc == 0;   // (the first set and the look-back state are untouched; the min / max keys hold what pass 2 finds again)
    if (rc) return rc;
    const double t_1 = now_ms();
    const double t_2 = now_ms();
    long long n_edges = 0, rows_x = 0, cols_x = 0;
    for (int k = 0; k < NSH; ++k) {
        n_edges += b->host_bd.shard[k].cursor;
        rows_x += b->host_bd.shard[k].rows_crossed;
        cols_x += b->host_bd.shard[k].cols_crossed;
    }
    if (n_edges > 0x7fffffff / 4) return fail(SVGR_E_OVERFLOW, "%lld edges: beyond the 32-bit edge index", n_edges);
    b->n_edges = n_edges;
    for (int k = 0; k < NSH; ++k) {  // (the renders' edge array is one dense block: see k_flatten)
        b->shards.base[k] = k == 0 ? 0 : (int)b->n_edges;
        b->shards.cap[k] = k == 0 ? (int)b->n_edges : 0;
    }
    b->n_bands = (b->vp[2] + TR - 1) / TR;
    b->n_pb = b->host_bd.pb_cursor;
    b->n_cells = b->host_bd.cell_cursor;
    b->n_slabs = b->host_bd.slab_cursor;
    b->n_entries = b->n_pb;
    // the longest band list (sizes the tiles' entry bitmasks): the bands every clipped bbox reaches
    std::vector<int> diff((size_t)b->n_bands + 1, 0);
    for (size_t p = 0; p < (size_t)b->n_paths; ++p) {
        const int r0 = b->host_bbox[4 * p], rows = b->host_bbox[4 * p + 2], cols = b->host_bbox[4 * p + 3];
        if (rows <= 0 || cols <= 0) continue;
        const int b0 = (r0 - b->vp[0]) / TR, b1 = (r0 + rows - 1 - b->vp[0]) / TR;
        if (b0 < 0 || b1 >= b->n_bands) return 0;
        diff[(size_t)b0] += 1;
        diff[(size_t)b1 + 1] -= 1;
    }
    int longest = 0, run = 0;
    for (int k = 0; k < b->n_bands; ++k) { run += diff[(size_t)k]; longest = std::max(longest, run); }
    {
        // add slots.  An edge row makes two adds (the pixel it lies in and the carry into the next) plus one per column border it
        // crosses (fewer for long shallow spans: one per PX columns): pieces <= 2 x edge rows + columns crossed.  A cell with pieces
        // adds up to TR carry-ins and TR sentinels: 9 per cell of the bbox on the bench scene, 12 budgeted.  (synth4096: 7.61 M adds;
        // rows 2.17 M, columns 1.4 M, cells 0.21 M -> 8.3 M, x 1.15 per shard, x 1.125 by layout_adds: 10.7 M slots -- round 5 asked
        // for 12.9 M; fresh device memory is cleared before its first use and a cold frame pays ~3.4 us per megabyte it asks for)
        double guess = 1.1 * (2.0 * (double)rows_x + (double)cols_x) + 14.0 * (double)b->n_cells + 65536.0;   // (k_path_build<2> reserves by BOUNDS: a tenth more than the pieces, TR (+ TR) per cell that can have any)
        if (const char* sk = getenv("SVGR_TWO_PASS_SHRINK")) guess /= std::max(atof(sk), 1.0);   // (tests: a guess that is too small on purpose)
        if (guess > (double)(1ll << 29)) return 0;
        int need[NSH];
        for (int k = 0; k < NSH; ++k) need[k] = (int)(guess * 1.15 / NSH) + 8192;
        if ((rc = b->layout_adds(need, NSH))) return rc;
        b->adds_roomy = true;
    }
    b->mask_words = (int)std::max<int64_t>(((int64_t)std::max(longest, 1) + 63) / 64, 1);
    b->masks_zeroed = false;
    b->plan.masks_resized();
    {
        // every work array of the batch out of ONE device block (each with the eighth of slack an allocation of its own would
        // have: a re-plan of a drawing that moved a little fits the same arrays, spec_issue(again))
        const size_t n_e = (size_t)std::max<int64_t>(b->n_edges, 1), n_c = (size_t)std::max<int64_t>(b->n_cells, 1);
        const size_t n_pairs = (size_t)std::max<int64_t>(b->n_pb, 1), n_bd = (size_t)b->n_bands + 1;
        const size_t n_tiles = (size_t)std::max(b->n_bands, 1) * (size_t)std::max(b->n_ctiles(), 1);
        const size_t owned = (size_t)std::max(count_owned_bands(b->own, b->n_bands), 1);
        auto layout = [&](Carver& c) {
            c.take(b->edges, n_e * 4);
            c.take(b->edge_path, n_e);
            c.take(b->band_start, n_bd);
            c.take(b->band_count, n_bd);
            c.take(b->band_item0, n_bd);
            c.take(b->cell_hdr, n_c + 1);
            c.take(b->cell_plan, n_c + 1);
            c.take(b->slabs, (size_t)std::max<int64_t>(b->n_slabs, 1));
            c.take(b->entries, n_pairs);
            c.take(b->pair_idx, n_pairs);
            c.take(b->tile_mask, b->mask_bytes() / sizeof(unsigned long long) + 1);
            c.take(b->tile_mask_kept, b->mask_bytes() / sizeof(unsigned long long) + 1);
            c.take(b->tile_info, n_tiles);
            c.take(b->pages, owned * (size_t)std::max(b->n_ctiles(), 1) * PAGE_STRIDE);
            c.take(b->items, n_c);
            c.take(b->adds, (size_t)std::max<int64_t>(b->n_adds, 1));
        };
        Carver sizing;
        layout(sizing);
        // (the arrays may be views of an earlier block of this batch: let go of them before the block)
        b->edges.release(); b->edge_path.release(); b->band_start.release(); b->band_count.release(); b->band_item0.release();
        b->cell_hdr.release(); b->cell_plan.release(); b->slabs.release(); b->entries.release(); b->pair_idx.release();
        b->tile_mask.release(); b->tile_mask_kept.release(); b->tile_info.release(); b->pages.release(); b->items.release(); b->adds.release();
        b->work_block.release();
        if ((rc = b->work_block.ensure(sizing.at))) return rc;
        Carver carve;
        carve.base = b->work_block.p;
        layout(carve);
    }
    const double t_3 = now_ms();
    if ((rc = run_geometry(b, 4, true))) return rc;
    // (pass 2 finds the bboxes the census found: with a staging, only its scalars come back -- a 64 KB copy in front of the tile
    //  kernel costs a frame ~20 us)
    if ((rc = issue_readback(b, staging == nullptr, staging))) return rc;
    if (getenv("SVGR_DBG_PLAN"))
        fprintf(stderr, "[plan] two passes, ms: pass 1 issued %.3f, drained %.3f, buffers sized %.3f, pass 2 issued %.3f | edges %lld, rows crossed %lld, columns %lld, pairs %lld, cells %lld, slabs %lld, add slots %lld, longest band list %d\n",
                t_1 - t_0, t_2 - t_1, t_3 - t_2, now_ms() - t_3, n_edges, rows_x, cols_x, (long long)b->n_pb, (long long)b->n_cells, (long long)b->n_slabs, (long long)b->n_adds, longest);
    return 1;
}
// pass 2 has drained: validate it.  1 planned, 0 fall back (a guess was too small), < 0 error
static int two_pass_finish(svgr_batch* b, const void* staging) {
    if (staging) memcpy(&b->host_bd, staging, sizeof(BatchDev));   // (the bboxes on the host are the census's: the same geometry)
    HIPCHK(hipGetLastError());
    if (b->host_bd.err) b->invalidate_work();
    int cap_bits = 0;
    if (int rc = eval_dev_err(b->host_bd.err, &cap_bits)) return rc;
    if (getenv("SVGR_DBG_PLAN")) {
        long long a = 0;
        for (int k = 0; k < NSH; ++k) a += b->host_bd.shard[k].add_cursor;
        fprintf(stderr, "[plan] two passes: capacity bits %d | adds %lld of %lld\n", cap_bits, a, (long long)b->n_adds);
    }
    if (cap_bits) return 0;
    b->n_entries = b->host_bd.entry_cursor;
    b->n_edges_live = b->n_edges;
    b->n_bsegs = b->host_bd.bseg_cursor;
    b->plan.plan_made();
    b->sized = true;
    for (int k = 0; k < 4; ++k) b->sized_vp[k] = b->vp[k];
    b->read_switches();
    b->geometry_fresh = true; b->geometry_current = true;
    return 1;
}

static int plan_two_pass(svgr_batch* b) {
    const int is = two_pass_issue(b, nullptr);
    if (is <= 0) return is;
    HIPCHK(hipStreamSynchronize(b->ctx->stream));
    const int fin = two_pass_finish(b, nullptr);
    if (fin <= 0) return fin;
    if (int rc = plan_slab_order(b)) return rc;
    return 1;
}

static int batch_plan_impl(svgr_batch* b, bool skip_speculative) {
    if (!b) return fail(SVGR_E_INVALID, "batch is NULL");
    HIPCHK(enter_ctx(b->ctx));
    b->defer_bbox = false;
    b->plan.plan_begins();
    b->geometry_fresh = false; b->geometry_current = false;
    {
        const bool no_spec = getenv("SVGR_NO_SPECULATIVE_PLAN") != nullptr;  // (tests exercise both planners)
        const int sp = no_spec || skip_speculative ? 0 : plan_speculative(b);
        if (sp < 0) return sp;
        if (sp > 0) return 0;
    }
    {
        const int tp = plan_two_pass(b);
        if (tp < 0) return tp;
        if (tp > 0) return 0;
        b->plan.plan_begins();
        b->geometry_fresh = false; b->geometry_current = false;
    }
    if (int rc = b->layout_arena()) return rc;
    // 1. Without a viewport (S:968 `viewport is None`) the union of the unclipped bboxes becomes the canvas.
    if (!b->has_vp) {
        if (int rc = run_geometry(b, 0, false)) return rc;
        if (int rc = check_dev_err(b)) return rc;
        if (b->host_bd.n_nonempty > 0) {
            long long r0 = (long long)UNION_BIAS - (long long)b->host_bd.umin_r, c0 = (long long)UNION_BIAS - (long long)b->host_bd.umin_c;
            long long ur = (long long)b->host_bd.umax_r - UNION_BIAS - r0, uc = (long long)b->host_bd.umax_c - UNION_BIAS - c0;
            if (ur * uc > (1ll << 31) || ur > (1 << 24) || uc > (1 << 24))
                return fail(SVGR_E_INVALID, "unclipped extent of %lldx%lld pixels is too large; pass a viewport", ur, uc);
            b->vp[0] = (int)r0; b->vp[1] = (int)c0; b->vp[2] = (int)ur; b->vp[3] = (int)uc;
        } else {
            b->vp[0] = b->vp[1] = 0; b->vp[2] = b->vp[3] = 0;
        }
    }
    // 1b. multi-GPU: the segments this rank has to flatten at all (a plan product: the renders launch over the list)
    b->n_seg_list = -1;
    if (b->own.world > 1 && b->n_segs > 0 && b->vp[2] > 0) {
        if (int rc = build_seg_list(b)) return rc;
    }
    // 2. count the edges this rank keeps: per segment, and their prefix sums = where every segment's edges go
    if (int rc = run_geometry(b, 1, true)) return rc;
    if (int rc = check_dev_err(b)) return rc;
    b->n_edges = 0;
    for (int k = 0; k < NSH; ++k) b->n_edges += b->host_bd.shard[k].cursor;
    if (b->n_edges > 0x7fffffff / 4) return fail(SVGR_E_OVERFLOW, "%lld edges: beyond the 32-bit edge index", (long long)b->n_edges);
    for (int k = 0; k < NSH; ++k) {  // (the renders' edge array is one dense block: see k_flatten)
        b->shards.base[k] = k == 0 ? 0 : (int)b->n_edges;
        b->shards.cap[k] = k == 0 ? (int)b->n_edges : 0;
    }
    if (int rc = b->edges.ensure((size_t)std::max<int64_t>(b->n_edges, 1) * 4)) return rc;
    if (int rc = b->edge_path.ensure((size_t)std::max<int64_t>(b->n_edges, 1))) return rc;
    b->n_bands = (b->vp[2] + TR - 1) / TR;
    if (int rc = b->band_start.ensure((size_t)b->n_bands + 1)) return rc;
    if (int rc = b->band_count.ensure((size_t)b->n_bands + 1)) return rc;
    if (int rc = b->band_item0.ensure((size_t)b->n_bands + 1)) return rc;
    if (int rc = run_geometry(b, 2, true)) return rc;
    if (int rc = check_dev_err(b)) return rc;
    b->n_pb = b->host_bd.pb_cursor;
    b->n_cells = b->host_bd.cell_cursor;
    b->n_slabs = b->host_bd.slab_cursor;
    if (int rc = b->cell_hdr.ensure((size_t)std::max<int64_t>(b->n_cells, 1) + 1)) return rc;
    if (int rc = b->cell_plan.ensure((size_t)std::max<int64_t>(b->n_cells, 1) + 1)) return rc;
    if (int rc = b->slabs.ensure((size_t)std::max<int64_t>(b->n_slabs, 1))) return rc;
    // 3. the band lists
    if (int rc = b->entries.ensure((size_t)std::max<int64_t>(b->n_pb, 1))) return rc;
    if (int rc = b->pair_idx.ensure((size_t)std::max<int64_t>(b->n_pb, 1))) return rc;
    if (int rc = run_geometry(b, 3, true)) return rc;
    if (int rc = check_dev_err(b)) return rc;
    b->n_entries = b->host_bd.entry_cursor;
    if (int rc = b->size_masks(b->host_bd.max_band_entries)) return rc;
    if (int rc = b->size_tile_lists(count_owned_bands(b->own, b->n_bands))) return rc;
    // 3b. the whole geometry once with k_path_build only SIZING the add lists: what every shard of add slots has to hold
    {
        b->count_adds_only = true;
        b->add_shards.n = NSH;
        int rc = run_geometry(b, 4, true);
        b->count_adds_only = false;
        if (rc) return rc;
        if ((rc = check_dev_err(b))) return rc;
        int need[NSH];
        for (int k = 0; k < NSH; ++k) need[k] = b->host_bd.shard[k].add_cursor;
        if ((rc = b->size_adds(need, NSH))) return rc;
        b->adds_roomy = false;   // (measured: the lists are dense, k_path_build<0> from here on)
    }
    // 4. full geometry once, to validate the capacities and fetch the bboxes
    if (int rc = run_geometry(b, 4, true)) return rc;

    if (int rc = check_dev_err(b, nullptr, true, true)) return rc;
    b->n_edges_live = b->n_edges;
    b->n_bsegs = b->host_bd.bseg_cursor;
    if (int rc = plan_slab_order(b)) return rc;
    b->plan.plan_made();
    b->sized = true;
    for (int k = 0; k < 4; ++k) b->sized_vp[k] = b->vp[k];
    b->read_switches();
    b->geometry_fresh = true; b->geometry_current = true;
    return 0;
}

int svgr_batch_get_stats(const svgr_batch* b, svgr_batch_stats* out) {
    if (!b || !out) return fail(SVGR_E_INVALID, "bad arguments");
    if (!b->plan.planned()) return fail(SVGR_E_STATE, "svgr_batch_plan has not run");
    out->n_edges = b->n_edges_live;
    out->path_pixels = (int64_t)b->host_bd.path_pixels;
    out->n_band_segs = b->n_bsegs;  // (edge rows)
    out->n_path_bands = b->n_pb;
    out->n_nonempty = b->host_bd.n_nonempty;
    if (b->host_bd.n_nonempty > 0) {
        long long r0 = (long long)UNION_BIAS - (long long)b->host_bd.umin_r, c0 = (long long)UNION_BIAS - (long long)b->host_bd.umin_c;
        out->bbox_union[0] = r0;
        out->bbox_union[1] = c0;
        out->bbox_union[2] = (long long)b->host_bd.umax_r - UNION_BIAS - r0;
        out->bbox_union[3] = (long long)b->host_bd.umax_c - UNION_BIAS - c0;
    } else {
        out->bbox_union[0] = out->bbox_union[1] = out->bbox_union[2] = out->bbox_union[3] = 0;
    }
    out->tile_rows = TR;
    out->tile_cols = TC;
    return 0;
}

int svgr_batch_get_bboxes(const svgr_batch* b, int32_t* out) {
    if (!b || !out) return fail(SVGR_E_INVALID, "bad arguments");
    if (!b->plan.planned()) return fail(SVGR_E_STATE, "svgr_batch_plan has not run");
    if (b->host_bbox_stale) {
        HIPCHK(enter_ctx(b->ctx));
        if (int rc = ensure_host_bbox(const_cast<svgr_batch*>(b))) return rc;
    }
    memcpy(out, b->host_bbox.data(), sizeof(int32_t) * 4 * (size_t)b->n_paths);
    return 0;
}

// The extent of every path's flattened points, unclipped and unrounded: {min row, min col, max row, max col} in device space --
// what ConvexHull(lines).bbox (S:993, S:2010-2020) comes to under a transform that keeps the axes apart, and with it the frame of
// an objectBoundingBox paint (S:1023-1027) without the hull.  The minima / maxima are those k_flatten folds for k_path_bbox (every
// point of every segment, whatever the viewport: min / max keys in the counter arena), so they are the plan's own pass's: asked for
// between svgr_batch_plan and the first render.  A path without edges reports {+inf, +inf, -inf, -inf}.
int svgr_batch_get_extents(svgr_batch* b, double* out) {
    return abi_guard("svgr_batch_get_extents", [&]() -> int {
        if (!b || !out) return fail(SVGR_E_INVALID, "bad arguments");
        if (!b->plan.planned() || !b->geometry_fresh)
            return fail(SVGR_E_STATE, "the extents are read from the plan's own geometry pass: call between svgr_batch_plan and the first render");
        const size_t np = (size_t)b->n_paths;
        if (np == 0) return 0;
        HIPCHK(enter_ctx(b->ctx));
        std::vector<unsigned long long> k(4 * np);
        HIPCHK(hipMemcpyAsync(k.data(), b->pkeys(), sizeof(unsigned long long) * 4 * np, hipMemcpyDeviceToHost, b->ctx->stream));
        HIPCHK(hipStreamSynchronize(b->ctx->stream));
        for (size_t p = 0; p < np; ++p) {
            double* o = out + 4 * p;
            if (k[4 * p] == 0ull) { o[0] = o[1] = INFINITY; o[2] = o[3] = -INFINITY; continue; }
            o[0] = key_f64(~k[4 * p]); o[1] = key_f64(~k[4 * p + 1]); o[2] = key_f64(k[4 * p + 2]); o[3] = key_f64(k[4 * p + 3]);
        }
        return 0;
    });
}

int svgr_batch_get_edges(const svgr_batch* b, double* edges, int32_t* edge_path, int64_t cap) {
    if (!b || !edges) return fail(SVGR_E_INVALID, "bad arguments");
    if (!b->plan.planned()) return fail(SVGR_E_STATE, "svgr_batch_plan has not run");
    if (cap < b->n_edges_live) return fail(SVGR_E_INVALID, "edge buffer holds %lld, need %lld", (long long)cap, (long long)b->n_edges_live);
    if (b->n_edges_live == 0) return 0;
    HIPCHK(enter_ctx(b->ctx));
    HIPCHK(hipStreamSynchronize(b->ctx->stream));
    // (one dense block in (path, segment, curve) order: see k_flatten)
    HIPCHK(hipMemcpy(edges, b->edges.p, sizeof(double) * 4 * (size_t)b->n_edges_live, hipMemcpyDeviceToHost));
    if (edge_path) HIPCHK(hipMemcpy(edge_path, b->edge_path.p, sizeof(int) * (size_t)b->n_edges_live, hipMemcpyDeviceToHost));
    return 0;
}

// Every flattened edge of every path, whatever the viewport: ConvexHull(lines) of Path.mask (S:993) is built from all
// of them, and objectBoundingBox clips / gradients / patterns take their frame from that hull -- a shape that hangs out of
// the viewport keeps its full bounding box.  (The render keeps only edges that can reach the viewport's rows.)
// Two flatten passes without row culling into scratch shards: count, then emit.  The batch's own plan stays valid; its
// counter arena is left dirty, so the next render starts from a fresh geometry pass.
static int batch_all_edges_impl(svgr_batch* b, double* edges, int32_t* edge_path, int64_t cap, int64_t* n_out);
int svgr_batch_all_edges(svgr_batch* b, double* edges, int32_t* edge_path, int64_t cap, int64_t* n_out) {
    return abi_guard("svgr_batch_all_edges", [&]() { return batch_all_edges_impl(b, edges, edge_path, cap, n_out); });
}

static int batch_all_edges_impl(svgr_batch* b, double* edges, int32_t* edge_path, int64_t cap, int64_t* n_out) {
    if (!b || !n_out) return fail(SVGR_E_INVALID, "bad arguments");
    HIPCHK(enter_ctx(b->ctx));
    hipStream_t st = b->ctx->stream;
    const int ns = (int)b->n_segs;
    *n_out = 0;
    if (ns <= 0) return 0;
    if (b->arena_bytes == 0)
        if (int rc = b->layout_arena()) return rc;
    const dim3 fgrid = grid1((size_t)ns << FL_SUB, FL_BLOCK);
    const Owner whole{0, 1, 1};
    b->geometry_fresh = false; b->geometry_current = false;
    b->arena_zeroed = false;
    HIPCHK(hipMemsetAsync(b->arena.p, 0, b->arena_bytes, st));
    SVGR_LAUNCH(k_flatten<false>, fgrid, dim3(FL_BLOCK), 0, st, (const double*)b->segs.p, (const uint8_t*)b->seg_kind.p,
                       (const int*)b->seg_path.p, (const double*)b->path_m6.p, ns, b->thr, (double*)nullptr, (int*)nullptr, b->shards,
                       b->pkeys(), b->bd(), whole, 0, 0, (const unsigned*)nullptr, (const int*)nullptr, 0, (int*)nullptr, (const int*)nullptr, 0, (int*)nullptr, (int*)nullptr, (unsigned long long*)nullptr);
    BatchDev counts;
    HIPCHK(hipMemcpyAsync(&counts, b->bd(), sizeof counts, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (counts.err & 1) return fail(SVGR_E_OVERFLOW, "flatten depth cap (%d) hit: non-finite or absurd control points", kMaxFlattenDepth);
    EdgeShards sh{};
    int64_t total = 0;
    for (int k = 0; k < NSH; ++k) {
        sh.base[k] = (int)total;
        sh.cap[k] = counts.shard[k].cursor;
        total += counts.shard[k].cursor;
    }
    *n_out = total;
    if (!edges || total == 0) return 0;  // (a size query)
    if (cap < total) return fail(SVGR_E_INVALID, "edge buffer holds %lld, need %lld", (long long)cap, (long long)total);
    if (total > 0x7fffffff / 4) return fail(SVGR_E_OVERFLOW, "%lld edges: beyond the 32-bit edge index", (long long)total);
    PoolBlock d_edges, d_path;
    HIPCHK(d_edges.alloc(sizeof(double) * 4 * (size_t)total));
    HIPCHK(d_path.alloc(sizeof(int) * (size_t)total));
    hipError_t e = hipMemsetAsync(b->arena.p, 0, b->arena_bytes, st);
    if (e == hipSuccess) {
        SVGR_LAUNCH(k_flatten<true>, fgrid, dim3(FL_BLOCK), 0, st, (const double*)b->segs.p, (const uint8_t*)b->seg_kind.p,
                           (const int*)b->seg_path.p, (const double*)b->path_m6.p, ns, b->thr, d_edges.as<double>(), d_path.as<int>(), sh, b->pkeys(), b->bd(),
                           whole, 0, 0, (const unsigned*)nullptr, (const int*)nullptr, 0, (int*)nullptr, (const int*)nullptr, 0, (int*)nullptr, (int*)nullptr, (unsigned long long*)nullptr);
        e = hipMemcpyAsync(edges, d_edges.p, sizeof(double) * 4 * (size_t)total, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && edge_path) e = hipMemcpyAsync(edge_path, d_path.p, sizeof(int) * (size_t)total, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e == hipSuccess) e = hipGetLastError();
    }
    if (e != hipSuccess) return fail(SVGR_E_HIP, "svgr_batch_all_edges: %s", hipGetErrorString(e));
    return 0;
}

int64_t svgr_batch_owned_rows(const svgr_batch* b) {
    if (!b || !b->plan.planned()) return -1;
    if (b->own.world <= 1) return b->vp[2];
    return (int64_t)count_owned_bands(b->own, b->n_bands) * TR;
}

static int get_event(svgr_batch* b, hipEvent_t* e) {
    if (!b->event_pool.empty()) { *e = b->event_pool.back(); b->event_pool.pop_back(); return 0; }
    HIPCHK(hipEventCreate(e));
    return 0;
}

// phase 0: geometry (unless it is current) and the tile launch; 1: the geometry part alone; 2: the tile launch alone, on `tile_st`
static int batch_render_impl(svgr_batch* b, svgr_buf* out, int out_kind, unsigned flags, const int32_t* window, int phase = 0,
                             hipStream_t tile_st = nullptr, WinTable* wt = nullptr);
int svgr_batch_render(svgr_batch* b, svgr_buf* out, int out_kind, unsigned flags) {
    return abi_guard("svgr_batch_render", [&]() { return batch_render_impl(b, out, out_kind, flags, nullptr); });
}
int svgr_batch_render_window(svgr_batch* b, svgr_buf* out, int out_kind, unsigned flags, const int32_t* window) {
    return abi_guard("svgr_batch_render_window", [&]() {
        if (!window) return fail(SVGR_E_INVALID, "window is NULL");
        return batch_render_impl(b, out, out_kind, flags, window);
    });
}

int svgr_batch_render_windows(svgr_batch* b, int64_t n, svgr_buf* const* outs, int out_kind, unsigned flags, const int32_t* windows) {
    return abi_guard("svgr_batch_render_windows", [&]() {
        if (!b || n < 0 || (n > 0 && (!outs || !windows))) return fail(SVGR_E_INVALID, "bad arguments");
        if (n == 0) return 0;
        for (int64_t i = 0; i < n; ++i)
            if (!outs[i]) return fail(SVGR_E_INVALID, "output %lld is NULL", (long long)i);
        if (flags & (SVGR_RENDER_TIMED | SVGR_RENDER_DETERMINISTIC)) return fail(SVGR_E_INVALID, "timed / deterministic renders draw one window at a time");
        svgr_ctx* c = b->ctx;
        HIPCHK(enter_ctx(c));
        // Every variant but the production kernel (whose launch is whole-canvas and persistent) draws the windows in ONE launch per
        // MAX_WINS of them: a window is a few dozen workgroups that live as long as its deepest tile, and a document's runs are dozens
        // of windows (icons.svg: 30 launches, 1.6 ms one after the other).  The production kernel, and a rank of a sharded canvas,
        // take a launch per window on eight streams.
        if (!production_variant(b, out_kind) && (out_kind == SVGR_OUT_CANVAS_F32 || out_kind == SVGR_OUT_CANVAS_F64) && b->own.world <= 1) {
            if (int rc = batch_render_impl(b, outs[0], out_kind, flags, windows, 1)) return rc;
            WinTable local;   // (3 KiB on the stack, copied into the launch's argument)
            for (int64_t at = 0; at < n; at += MAX_WINS) {
                local.n = 0; local.pad[0] = local.pad[1] = local.pad[2] = 0;
                const int64_t end = std::min<int64_t>(n, at + MAX_WINS);
                for (int64_t i = at; i < end; ++i)
                    if (int rc = batch_render_impl(b, outs[i], out_kind, flags, windows + 4 * i, 3, nullptr, &local)) return rc;
                for (int k = local.n; k < MAX_WINS; ++k) memset(&local.w[k], 0, sizeof(WinRec));
                if (int rc = batch_render_impl(b, outs[at], out_kind, flags, windows + 4 * at, 4, nullptr, &local)) return rc;
            }
            return 0;
        }
        if (!c->side_ready) {
            for (int k = 0; k < svgr_ctx::N_SIDE; ++k) {
                if (!c->side[k]) HIPCHK(hipStreamCreateWithFlags(&c->side[k], hipStreamNonBlocking));
                if (!c->side_ev[k]) HIPCHK(hipEventCreateWithFlags(&c->side_ev[k], hipEventDisableTiming));
            }
            if (!c->fork_ev) HIPCHK(hipEventCreateWithFlags(&c->fork_ev, hipEventDisableTiming));
            c->side_ready = true;
        }
        // the geometry kernels (unless the caller vouches for the previous pass) and the gradients' flags, on the context's stream
        if (int rc = batch_render_impl(b, outs[0], out_kind, flags, windows, 1)) return rc;
        const int used = (int)std::min<int64_t>(n, svgr_ctx::N_SIDE);
        HIPCHK(hipEventRecord(c->fork_ev, c->stream));
        for (int k = 0; k < used; ++k) HIPCHK(hipStreamWaitEvent(c->side[k], c->fork_ev, 0));
        // (everything the context's stream did before -- also the last use of a recycled output block -- is in front of the windows)
        int rc = 0;
        for (int64_t i = 0; i < n && rc == 0; ++i)
            rc = batch_render_impl(b, outs[i], out_kind, flags, windows + 4 * i, 2, c->side[i % svgr_ctx::N_SIDE]);
        // ... and the windows in front of everything it does next, whether all of them were launched or not
        for (int k = 0; k < used; ++k) {
            HIPCHK(hipEventRecord(c->side_ev[k], c->side[k]));
            HIPCHK(hipStreamWaitEvent(c->stream, c->side_ev[k], 0));
        }
        return rc;
    });
}

static int batch_render_impl(svgr_batch* b, svgr_buf* out, int out_kind, unsigned flags, const int32_t* window, int phase, hipStream_t tile_st, WinTable* wt) {
    if (!b || !out) return fail(SVGR_E_INVALID, "bad arguments");
    if (!b->plan.planned()) return fail(SVGR_E_STATE, "svgr_batch_plan must run before svgr_batch_render");
    if (out_kind < 0 || out_kind > 5) return fail(SVGR_E_INVALID, "unknown output kind %d", out_kind);
    if (b->plan.slab_order_pending() && !b->geometry_fresh) {   // (a replay of a plan svgr_batch_draw made: its places now, once)
        b->plan.slab_order_taken_up();
        if (int rc = plan_slab_order(b)) return rc;
        b->plan.slab_order_made_late();
    }
    const bool layers = out_kind == SVGR_OUT_MASKS_F64 || out_kind == SVGR_OUT_FILLS_F64;  // one mask / fill layer per path, back to back
    if (layers) out_kind = out_kind == SVGR_OUT_MASKS_F64 ? SVGR_OUT_MASK_F64 : SVGR_OUT_FILL_F64;
    const bool single = out_kind >= 2;
    if (single && !layers && b->n_paths != 1) return fail(SVGR_E_INVALID, "mask/fill outputs need a single-path batch");
    if (single && (b->n_groups > 0 || b->n_grads > 0)) return fail(SVGR_E_INVALID, "isolated groups and gradient paints exist in the canvas outputs only");
    if (layers && b->own.world > 1) return fail(SVGR_E_INVALID, "per-path mask output is not sharded");
    // render window (canvas outputs): viewport-local rectangle {row0, col0, rows, cols} that `out` covers
    int win[4] = {0, 0, b->vp[2], b->vp[3]};
    if (window) {
        if (single) return fail(SVGR_E_INVALID, "a render window applies to the canvas outputs");
        if (b->own.world > 1) return fail(SVGR_E_INVALID, "a render window and band sharding exclude each other");
        win[0] = window[0] - b->vp[0]; win[1] = window[1] - b->vp[1]; win[2] = window[2]; win[3] = window[3];
        if (win[2] <= 0 || win[3] <= 0 || win[0] < 0 || win[1] < 0 || (long long)win[0] + win[2] > b->vp[2] ||
            (long long)win[1] + win[3] > b->vp[3])
            return fail(SVGR_E_INVALID, "render window (%d, %d, %d, %d) is empty or not inside the viewport (%d, %d, %d, %d)", window[0],
                        window[1], window[2], window[3], b->vp[0], b->vp[1], b->vp[2], b->vp[3]);
    }
    HIPCHK(enter_ctx(b->ctx));
    hipStream_t st = b->ctx->stream;
    if (single && b->host_bbox_stale)
        if (int rc = ensure_host_bbox(b)) return rc;

    const int owned_bands = count_owned_bands(b->own, b->n_bands);
    const int n_ctiles = (b->vp[3] + TC - 1) / TC;
    size_t need;
    if (layers) {
        // layer p starts at the sum of the areas (rows x cols of the clipped bbox, 0 when empty) of the paths before it
        b->wait_uploads();  // (the previous render's copy of this table may still be running)
        b->host_layer_off.resize((size_t)b->n_paths);
        long long at = 0;
        for (int64_t p = 0; p < b->n_paths; ++p) {
            b->host_layer_off[(size_t)p] = at;
            const long long r = b->host_bbox[4 * (size_t)p + 2], c = b->host_bbox[4 * (size_t)p + 3];
            if (r > 0 && c > 0) at += r * c;
        }
        need = (size_t)at * sizeof(double) * (out_kind == SVGR_OUT_FILL_F64 ? 4 : 1);
        if (int rc = b->layer_off.ensure((size_t)b->n_paths)) return rc;
        HIPCHK(hipMemcpyAsync(b->layer_off.p, b->host_layer_off.data(), sizeof(long long) * (size_t)b->n_paths, hipMemcpyHostToDevice, st));
        HIPCHK(b->note_upload(st));  // (the source is a member: svgr_batch_destroy waits for it)
    } else if (single) {
        need = (size_t)std::max(b->host_bbox[2], 0) * std::max(b->host_bbox[3], 0) * sizeof(double) * (out_kind == 3 ? 4 : 1);
    } else {
        const bool all = b->own.world <= 1;
        size_t rows = all ? (size_t)win[2] : (size_t)owned_bands * TR;
        need = rows * (size_t)win[3] * 4 * (out_kind == 0 ? sizeof(float) : sizeof(double));
    }
    if (out->bytes < need) return fail(SVGR_E_INVALID, "output buffer has %zu bytes, needs %zu", out->bytes, need);

    const bool timed = (flags & SVGR_RENDER_TIMED) != 0;
    TimedEvents ev{};
    if (timed) {
        if (int rc = get_event(b, &ev.e0)) return rc;
        if (int rc = get_event(b, &ev.e1)) return rc;
        if (int rc = get_event(b, &ev.e2)) return rc;
        HIPCHK(hipEventRecord(ev.e0, st));
    }
    // geometry, identical to the last plan step but without read-backs (capacities are exact for
    // unchanged input; the kernels flag an overflow otherwise and svgr_batch_timings / the next
    // plan reports it)
    // (the first render after a plan finds the plan's own full geometry pass in the buffers: same inputs, same result)
    const bool det = (flags & SVGR_RENDER_DETERMINISTIC) != 0;
    // (SVGR_RENDER_SAME_GEOMETRY: another window of the canvas the previous render of this batch drew a window of -- the tile
    //  kernel only reads what the geometry kernels left, so the pass is not repeated; ignored when an input has changed since)
    // (phases of svgr_batch_render_windows -- 1: geometry only; 2: this window's tiles on `tile_st`; 3: this window into the table `wt`,
    //  nothing launched; 4: the table's windows in one launch)
    if (phase >= 2 && !b->geometry_current) return fail(SVGR_E_STATE, "a tile launch without its geometry pass");
    if (phase >= 3 && (!wt || !window)) return fail(SVGR_E_INVALID, "a window table is needed");
    const bool same = phase >= 2 || ((flags & SVGR_RENDER_SAME_GEOMETRY) != 0 && b->geometry_current && window != nullptr && !timed && !det);
    if (!(b->geometry_fresh && !timed && !det) && !same) {
        b->deterministic = det;
        b->geometry_current = false;
        const int rc = run_geometry(b, 4, true);
        b->deterministic = false;
        if (rc) return rc;
        b->geometry_current = true;
    }
    b->geometry_fresh = false;
    if (single && need) HIPCHK(hipMemsetAsync(out->ptr, 0, need, st));
    if (timed) HIPCHK(hipEventRecord(ev.e1, st));

    if (owned_bands > 0 && n_ctiles > 0) {
        TileArgs a;
        a.pages = b->pages.p; a.tile_info = b->tile_info.p; a.items = b->items.p; a.out = out->ptr;
        a.trash = b->ctx->trash;
        a.cell_hdr = b->cell_hdr.p; a.adds = b->adds.p;
        a.n_ct = b->n_ctiles();
        a.group_clip_src = b->group_clip_src.p; a.group_opacity = b->group_opacity.p;
        a.grads = b->grads.p; a.grad_flags = b->grad_flags.p;
        if (b->n_grads > 0 && b->has_focal && !same) {   // (another window of the same picture: the flags are the previous render's)
            // focal radial gradients mask their `det < 0` pixels only if the fill's layer has any (S:1627): one flag per fill
            HIPCHK(hipMemsetAsync(b->grad_flags.p, 0, sizeof(int) * (size_t)b->n_grads, st));
            SVGR_LAUNCH(k_grad_detneg, dim3(64, (unsigned)b->n_grads), dim3(256), 0, st, (const GradDev*)b->grads.p,
                               (const int*)b->grad_path.p, (const int*)b->bbox.p, b->grad_flags.p);
        }
        if (phase == 1) return 0;   // (the geometry kernels and the gradients' flags are on the stream: the windows follow)
        a.vr0 = b->vp[0]; a.vc0 = b->vp[1]; a.vrows = b->vp[2]; a.vcols = b->vp[3];
        a.own = b->own;
        a.out_cols = win[3];
        a.clip01 = (flags & SVGR_RENDER_CLIP01) ? 1 : 0;
        a.det = det ? 1 : 0;
        a.layer_off = layers ? b->layer_off.p : nullptr;
        a.arena = (unsigned*)b->arena.p;
        a.arena_words = (unsigned)(b->arena_bytes / 4);
        a.dbg = nullptr;
#ifdef SVGR_DBG_TIMELINE
        {
            // the PREVIOUS render's per-workgroup timeline goes to the file $SVGR_DBG_TIMELINE (raw u64 quadruples)
            static unsigned long long* tl_buf = nullptr;
            const size_t tl_bytes = 64 + 96 * (size_t)(1u << 16);
            HIPCHK(hipStreamSynchronize(st));
            if (!tl_buf) { (void)hipMalloc((void**)&tl_buf, tl_bytes); (void)hipMemset(tl_buf, 0, tl_bytes); }
            else if (getenv("SVGR_DBG_TIMELINE")) {
                std::vector<unsigned long long> tl(tl_bytes / 8);
                (void)hipMemcpy(tl.data(), tl_buf, tl_bytes, hipMemcpyDeviceToHost);
                if (FILE* f = fopen(getenv("SVGR_DBG_TIMELINE"), "wb")) { fwrite(tl.data(), 1, tl_bytes, f); fclose(f); }
            }
            a.dbg = tl_buf;
        }
#endif
        // the tiles the window touches (everything without one)
        a.ct0 = win[1] / TC;
        a.win_ct = (win[1] + win[3] - 1) / TC - a.ct0 + 1;
        a.band0 = window ? win[0] / TR : 0;
        a.n_bands = window ? (win[0] + win[2] - 1) / TR - a.band0 + 1 : owned_bands;
        a.win_r = win[0] - a.band0 * TR;
        a.win_c = win[1] - a.ct0 * TC;
        a.win_rows = b->own.world <= 1 ? win[2] : owned_bands * TR;
        a.win_cols = win[3];
        // the whole canvas: the tiles in k_tile_lists' order (heaviest first); a window: its tiles in raster order
        a.use_order = a.win_ct == n_ctiles && a.n_bands == owned_bands ? 1 : 0;
        // A whole-canvas launch is persistent: as many workgroups as the chip holds at once walk the tiles (k_tile_render);
        // how many a CU holds is the variant's register / LDS budget.
        const unsigned n_tiles = (unsigned)a.win_ct * (unsigned)a.n_bands;
        if (phase == 3) {
            if (wt->n >= MAX_WINS) return fail(SVGR_E_INVALID, "window table full");
            const long long first = wt->n ? (long long)wt->w[wt->n - 1].tile0 + (long long)wt->w[wt->n - 1].win_ct * wt->w[wt->n - 1].n_bands : 0ll;
            if (first + (long long)n_tiles > 0x7fffffffll) return fail(SVGR_E_OVERFLOW, "too many tiles in one launch");
            WinRec& r = wt->w[wt->n++];
            r.out = out->ptr; r.tile0 = (int)first;
            r.ct0 = a.ct0; r.win_ct = a.win_ct; r.band0 = a.band0; r.n_bands = a.n_bands;
            r.win_r = a.win_r; r.win_c = a.win_c; r.win_rows = a.win_rows; r.win_cols = a.win_cols; r.pad = 0;
            return 0;
        }
        constexpr int wgs_per_cu = std::min((WAVES_PER_EU * 4) / NW, (160 * 1024) / (2 * DELTA_BYTES));   // (registers, LDS)
        const bool production = production_variant(b, out_kind);   // (the variant with the tile loop)
        unsigned n_wgs = n_tiles;
        // (windows launched side by side on streams of their own take a workgroup per tile: the persistent launch's two sets of tile
        //  counters alternate per launch, which is only sound for launches that follow each other on ONE stream)
        if (a.use_order && production && tile_st == nullptr) n_wgs = std::min(n_tiles, (unsigned)wgs_per_cu * (unsigned)b->ctx->n_cu);
        a.tile_ctr = a.tile_ctr_clear = b->ctx->tile_ctr;
        if (n_wgs < n_tiles) {   // (a persistent launch: this set of counters, and the other one zeroed for the next such launch)
            a.tile_ctr = b->ctx->tile_ctr + 256 * b->ctx->tile_ctr_set;
            b->ctx->tile_ctr_set ^= 1;
            a.tile_ctr_clear = b->ctx->tile_ctr + 256 * b->ctx->tile_ctr_set;
        }
        dim3 grid(n_wgs);
        hipStream_t lst = tile_st ? tile_st : st;   // (svgr_batch_render_windows: a stream per window)
        if (phase == 4) {
            // every window of the table in this one launch: a workgroup per tile, the windows' tiles one window after the other
            if (wt->n <= 0 || production || out_kind > 1) return fail(SVGR_E_INVALID, "no window table for this launch");
            const WinRec& last = wt->w[wt->n - 1];
            const dim3 wgrid((unsigned)last.tile0 + (unsigned)last.win_ct * (unsigned)last.n_bands);
            a.use_order = 0;
            with_tile_variant(b, out_kind, [&](auto v) {
                using V = decltype(v);
                if constexpr (V::OUT <= 1 && (V::OUT == 1 || V::CLIP))   // (not the production variant: turned away above)
                    SVGR_LAUNCH((k_tile_render_windows<V::OUT, V::CLIP, V::GROUPS, V::GRAD>), wgrid, dim3(NT), 0, lst, a, *wt);
            });
            b->arena_zeroed = true;
            HIPCHK(hipGetLastError());
            return 0;
        }
        with_tile_variant(b, out_kind, [&](auto v) {
            using V = decltype(v);
            SVGR_LAUNCH((k_tile_render<V::OUT, V::CLIP, V::GROUPS, V::GRAD>), grid, dim3(NT), 0, lst, a);
        });
        b->arena_zeroed = true;  // (done by that kernel, see TileArgs::arena)
    }
    if (timed) {
        HIPCHK(hipEventRecord(ev.e2, st));
        b->events.push_back(ev);
    }
    HIPCHK(hipGetLastError());
    return 0;
}

// Plan (when the batch has no valid plan) AND render, behind ONE wait: what a caller pays for a frame with new geometry -- the
// reference's only mode (every Path.mask flattens and rasterises from scratch, S:948-957).  svgr_batch_plan + svgr_batch_render
// wait for the plan's last pass, sort the slabs on the host, and only then launch the tile kernel; here the tile kernel is
// enqueued right behind the plan's full geometry pass (it reads nothing but what that pass leaves, and a pass whose capacities did
// not hold has written nothing outside them), the pass's scalars and bboxes come back through page-locked memory, and the
// call waits once, at its end, to validate them.  A batch planned before (svgr_batch_set_transforms) takes the single pass with
// ONE flatten traversal (k_flatten<.., SCAN>), a new one the two-pass plan (census, then everything).  When a guess did not hold
// the staged plan and an ordinary render follow.  The slab order of the plan is made by the first render that replays it.
// On return the picture is in `out` (the stream has drained) and the batch is planned.
static int batch_draw_impl(svgr_batch* b, svgr_buf* out, int out_kind, unsigned flags) {
    if (!b || !out) return fail(SVGR_E_INVALID, "bad arguments");
    HIPCHK(enter_ctx(b->ctx));
    hipStream_t st = b->ctx->stream;
    b->defer_bbox = false;
    if (!b->plan.planned()) {
        const bool canvas = out_kind == SVGR_OUT_CANVAS_F32 || out_kind == SVGR_OUT_CANVAS_F64;
        const bool fast = canvas && b->has_vp && b->own.world <= 1 && b->n_segs > 0 && !(flags & (SVGR_RENDER_TIMED | SVGR_RENDER_DETERMINISTIC)) &&
                          getenv("SVGR_NO_SPECULATIVE_PLAN") == nullptr && getenv("SVGR_SAFE_PATH") == nullptr;
        int issued = 0;   // 1: the re-plan's single pass, 2: the two-pass plan's second pass
        if (fast) {
            const size_t stage_bytes = sizeof(BatchDev) + 16 * (size_t)b->n_paths + 256;
            if (int rc = ensure_pinned(b->ctx, stage_bytes)) return rc;
            b->plan.plan_begins();
            b->geometry_fresh = false; b->geometry_current = false;
            b->defer_bbox = true;                                       // (the bboxes stay on the device until somebody asks: ensure_host_bbox)
            int is = spec_issue(b, b->ctx->pinned, true);                 // (the buffers of the batch's last plan as the guesses)
            b->defer_bbox = is > 0;
            if (is == 0) is = spec_issue(b, b->ctx->pinned, false);      // (a small batch: size models)
            if (is < 0) return is;
            if (is > 0) issued = 1;
            else {
                is = two_pass_issue(b, b->ctx->pinned);
                if (is < 0) return is;
                if (is > 0) issued = 2;
            }
        }
        if (issued) {
            // the tile kernel right behind the pass: the batch counts as planned with that pass's geometry until the pass is validated
            b->plan.plan_made(); b->geometry_fresh = true; b->geometry_current = true;
            int rc = batch_render_impl(b, out, out_kind, flags, nullptr);
            b->plan.pass_withdrawn(); b->geometry_fresh = false; b->geometry_current = false;
            hipError_t e = hipStreamSynchronize(st);
            if (rc) return rc;
            HIPCHK(e);
            int fin;
            if (issued == 1) { take_readback(b, b->ctx->pinned); HIPCHK(hipGetLastError()); fin = spec_finish(b); }
            else fin = two_pass_finish(b, b->ctx->pinned);
            b->defer_bbox = false;
            if (fin < 0) return fin;
            if (fin > 0) {
                b->geometry_fresh = false;          // (consumed by the tile kernel above)
                b->plan.slab_order_left_to_replay(b->n_segs > 4096);  // (large batches: k_path_build's work list heaviest first, as svgr_batch_plan leaves it)
                return 0;
            }
            b->plan.plan_begins();
        }
        if (int rc = batch_plan_impl(b, issued == 1)) return rc;
    }
    if (int rc = batch_render_impl(b, out, out_kind, flags, nullptr)) return rc;
    HIPCHK(hipStreamSynchronize(st));
    return check_dev_err(b, nullptr, false);
}
int svgr_batch_draw(svgr_batch* b, svgr_buf* out, int out_kind, unsigned flags) {
    return abi_guard("svgr_batch_draw", [&]() { return batch_draw_impl(b, out, out_kind, flags); });
}

int svgr_batch_timings(svgr_batch* b, int* n_renders, double* ms_total, double* ms_geometry, double* ms_tile) {
    if (!b) return fail(SVGR_E_INVALID, "batch is NULL");
    HIPCHK(enter_ctx(b->ctx));
    HIPCHK(hipStreamSynchronize(b->ctx->stream));
    double tg = 0, tt = 0;
    for (auto& e : b->events) {
        float g = 0, t = 0;
        HIPCHK(hipEventElapsedTime(&g, e.e0, e.e1));
        HIPCHK(hipEventElapsedTime(&t, e.e1, e.e2));
        tg += g;
        tt += t;
        b->event_pool.push_back(e.e0);
        b->event_pool.push_back(e.e1);
        b->event_pool.push_back(e.e2);
    }
    if (n_renders) *n_renders = (int)b->events.size();
    if (ms_total) *ms_total = tg + tt;
    if (ms_geometry) *ms_geometry = tg;
    if (ms_tile) *ms_tile = tt;
    b->events.clear();
    if (int rc = check_dev_err(b, nullptr, false)) return rc;
    return 0;
}

// ---------------------------------------------------------------------------------------------
// layer ops
// ---------------------------------------------------------------------------------------------
int svgr_layer_over(svgr_ctx* ctx, svgr_buf* dst, const int64_t* db, const svgr_buf* src, const int64_t* sb, int ch, int first) {
    Box d, s;
    if (int rc = check_layer_pair("svgr_layer_over", ctx, dst, db, d, src, sb, s, ch)) return rc;
    const size_t n = box_px(s);
    if (n == 0) return 0;
    return launch_tail(ctx, k_layer_over, grid1(n), dim3(256), 0, (double*)dst->ptr, d, (const double*)src->ptr, s, ch, first);
}

int svgr_layer_blend(svgr_ctx* ctx, svgr_buf* out, const int64_t* ob, const svgr_buf* src, const int64_t* sb, int ch, int mode,
                     const double* k4) {
    if (!(mode == 1 || mode == 3 || mode == 4 || mode == 5) || (mode == 5 && !k4)) return fail(SVGR_E_INVALID, "invalid compose mode: %d", mode);
    Box o, s;
    if (int rc = check_layer_pair("svgr_layer_blend", ctx, out, ob, o, src, sb, s, ch)) return rc;
    const size_t n = box_px(o);
    if (n == 0) return 0;
    return launch_tail(ctx, k_layer_blend, grid1(n), dim3(256), 0, (double*)out->ptr, o, (const double*)src->ptr, s, ch, mode,
                       mode == 5 ? k4[0] : 0.0, mode == 5 ? k4[1] : 0.0, mode == 5 ? k4[2] : 0.0, mode == 5 ? k4[3] : 0.0);
}

int svgr_layer_color_matrix(svgr_ctx* ctx, svgr_buf* img, int64_t n_px, const double* m20) {
    if (!ctx || !img || !m20 || n_px < 0 || img->bytes < (size_t)n_px * 32) return fail(SVGR_E_INVALID, "svgr_layer_color_matrix: bad arguments");
    if (n_px == 0) return 0;
    HIPCHK(enter_ctx(ctx));
    return upload_launch_wait(ctx, "svgr_layer_color_matrix", {{m20, sizeof(double) * 20}}, [&](void* dm) {
        SVGR_LAUNCH(k_layer_color_matrix, grid1((size_t)n_px), dim3(256), 0, ctx->stream, (double*)img->ptr, (size_t)n_px, (const double*)dm);
    });
}

int svgr_layer_morphology(svgr_ctx* ctx, svgr_buf* out, const svgr_buf* src, int64_t rows, int64_t cols, int64_t ky, int64_t kx, int is_max) {
    if (!ctx || !out || !src || rows <= 0 || cols <= 0 || ky <= 0 || kx <= 0 || ky > rows || kx > cols || rows > (1 << 24) || cols > (1 << 24))
        return fail(SVGR_E_INVALID, "svgr_layer_morphology: bad arguments (the window must fit the layer)");
    const size_t n = (size_t)(rows - ky + 1) * (size_t)(cols - kx + 1);
    if (src->bytes < (size_t)rows * cols * 32 || out->bytes < n * 32) return fail(SVGR_E_INVALID, "svgr_layer_morphology: buffer too small");
    return launch_tail(ctx, k_layer_morphology, grid1(n), dim3(256), 0, (double*)out->ptr, (const double*)src->ptr, (int)rows, (int)cols,
                       (int)ky, (int)kx, is_max);
}

static_assert(svgr::kTurbMaxOctaves == SVGR_TURBULENCE_MAX_OCTAVES, "one octave limit");
// The floating-point parameters of the filter primitives below come from documents: every one must be finite, or the entry
// returns SVGR_E_INVALID before any launch (DESIGN.md "Filter primitives at the edges of their values").
static inline bool all_finite(const double* v, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(v[i])) return false;
    return true;
}
static inline unsigned stride_blocks(size_t n) { return (unsigned)std::max<size_t>(1, std::min<size_t>((n + 255) / 256, 1024)); }

int svgr_layer_turbulence(svgr_ctx* ctx, svgr_buf* out, const int64_t* bbox, const double* inv_m6, double base_fx, double base_fy,
                          const double* tile, int64_t seed, int octaves, int fractal, int stitch) {
    TurbLaunch a;
    if (!ctx || !out || !inv_m6 || !tile || !box_of(bbox, a.ob) || octaves < 0 || octaves > svgr::kTurbMaxOctaves || !(base_fx >= 0.0) ||
        !(base_fy >= 0.0) || (fractal != 0 && fractal != 1) || (stitch != 0 && stitch != 1))
        return fail(SVGR_E_INVALID, "svgr_layer_turbulence: bad arguments (octaves 0..%d, base frequencies >= 0)", svgr::kTurbMaxOctaves);
    const size_t n = box_px(a.ob);
    if (out->bytes < n * 32) return fail(SVGR_E_INVALID, "svgr_layer_turbulence: buffer too small");
    if (!all_finite(inv_m6, 6)) return fail(SVGR_E_INVALID, "svgr_layer_turbulence: the inverse transform is not finite");
    if (!svgr::turb_params_valid(base_fx, base_fy, tile, octaves, stitch))
        return fail(SVGR_E_INVALID, "svgr_layer_turbulence: base frequencies and stitch tile must be finite, the tile of positive width and "
                                    "height, and the stitch state of the last octave within 2^53");
    if (n == 0) return 0;
    return abi_guard("svgr_layer_turbulence", [&]() -> int {
        std::vector<char> host(sizeof(double) * svgr::kTurbLattice * 8 + sizeof(int) * svgr::kTurbLattice);
        double* grad = (double*)host.data();
        int* sel = (int*)(grad + svgr::kTurbLattice * 8);
        svgr::turb_init(seed, sel, grad);
        memcpy(a.inv, inv_m6, sizeof a.inv);
        a.p = svgr::turb_params(base_fx, base_fy, tile, octaves, fractal, stitch);
        HIPCHK(enter_ctx(ctx));
        return upload_launch_wait(ctx, "svgr_layer_turbulence", {{host.data(), host.size()}}, [&](void* dev) {
            SVGR_LAUNCH(k_layer_turbulence, dim3(stride_blocks(n)), dim3(256), 0, ctx->stream, (double*)out->ptr,
                        (const int*)((const double*)dev + svgr::kTurbLattice * 8), (const double*)dev, a);
        });
    });
}

int svgr_layer_component_transfer(svgr_ctx* ctx, svgr_buf* img, int64_t n_px, const int* types, const double* params,
                                  const int64_t* n_values, const double* values) {
    if (!ctx || !img || !types || !params || !n_values || n_px < 0 || img->bytes < (size_t)n_px * 32)
        return fail(SVGR_E_INVALID, "svgr_layer_component_transfer: bad arguments");
    int64_t total = 0;
    for (int k = 0; k < 4; ++k) {
        if (types[k] < svgr::kXferIdentity || types[k] > svgr::kXferGamma || n_values[k] < 0)
            return fail(SVGR_E_INVALID, "svgr_layer_component_transfer: channel %d: bad type %d or table length", k, types[k]);
        total += n_values[k];
    }
    if (total > SVGR_TRANSFER_MAX_VALUES)
        return fail(SVGR_E_INVALID, "svgr_layer_component_transfer: %lld table values (at most %d)", (long long)total, SVGR_TRANSFER_MAX_VALUES);
    if (total > 0 && !values) return fail(SVGR_E_INVALID, "svgr_layer_component_transfer: values is NULL");
    if (!all_finite(params, 20) || !all_finite(values, (size_t)total))
        return fail(SVGR_E_INVALID, "svgr_layer_component_transfer: parameters and table values must be finite");
    if (n_px == 0) return 0;
    return abi_guard("svgr_layer_component_transfer", [&]() -> int {
        std::vector<double> blob(20 + (size_t)total);
        memcpy(blob.data(), params, sizeof(double) * 20);
        if (total) memcpy(blob.data() + 20, values, sizeof(double) * (size_t)total);
        XferLaunch a;
        int off[4], cnt[4];
        int64_t at = 20;
        for (int k = 0; k < 4; ++k) { off[k] = (int)at; cnt[k] = (int)n_values[k]; at += n_values[k]; }
        a.type0 = types[0]; a.type1 = types[1]; a.type2 = types[2]; a.type3 = types[3];
        a.n0 = cnt[0]; a.n1 = cnt[1]; a.n2 = cnt[2]; a.n3 = cnt[3];
        a.off0 = off[0]; a.off1 = off[1]; a.off2 = off[2]; a.off3 = off[3];
        a.n_blob = (int)blob.size();
        HIPCHK(enter_ctx(ctx));
        return upload_launch_wait(ctx, "svgr_layer_component_transfer", {{blob.data(), sizeof(double) * blob.size()}}, [&](void* dev) {
            SVGR_LAUNCH(k_layer_component_transfer, dim3(stride_blocks((size_t)n_px)), dim3(256), (unsigned)(sizeof(double) * blob.size()),
                        ctx->stream, (double*)img->ptr, (size_t)n_px, (const double*)dev, a);
        });
    });
}

int svgr_layer_convolve_matrix(svgr_ctx* ctx, svgr_buf* out, const svgr_buf* src, int64_t rows, int64_t cols, const double* kernel,
                               int64_t order_x, int64_t order_y, int64_t target_x, int64_t target_y, double divisor, double bias,
                               int edge_mode, int preserve_alpha) {
    if (!ctx || !out || !src || !kernel || rows <= 0 || cols <= 0 || rows > (1 << 24) || cols > (1 << 24) || order_x < 1 || order_y < 1 ||
        order_x > SVGR_CONVOLVE_MATRIX_MAX_ORDER || order_y > SVGR_CONVOLVE_MATRIX_MAX_ORDER || target_x < 0 || target_x >= order_x ||
        target_y < 0 || target_y >= order_y || divisor == 0.0 || edge_mode < 0 || edge_mode > 2 || (preserve_alpha != 0 && preserve_alpha != 1))
        return fail(SVGR_E_INVALID, "svgr_layer_convolve_matrix: bad arguments (order 1..%d, target inside the kernel, divisor != 0, "
                                    "edge mode 0..2)", SVGR_CONVOLVE_MATRIX_MAX_ORDER);
    const size_t n = (size_t)rows * (size_t)cols;
    if (!all_finite(kernel, (size_t)(order_x * order_y)) || !std::isfinite(divisor) || !std::isfinite(bias))
        return fail(SVGR_E_INVALID, "svgr_layer_convolve_matrix: kernel, divisor and bias must be finite");
    if (src->bytes < n * 32 || out->bytes < n * 32) return fail(SVGR_E_INVALID, "svgr_layer_convolve_matrix: buffer too small");
    if (out->ptr == src->ptr) return fail(SVGR_E_INVALID, "svgr_layer_convolve_matrix: out must not be src");
    // 16 x 16 tiles while the input tile and the weights fit in 64 KiB of LDS, 8 x 8 beyond (order 32: 56 KiB)
    auto lds = [&](int T) { return (size_t)(T + order_y - 1) * (size_t)(T + order_x - 1) * 32 + (size_t)order_x * order_y * 8; };
    const int T = lds(16) <= (64u << 10) ? 16 : 8;
    CmLaunch a;
    a.rows = (int)rows; a.cols = (int)cols; a.ox = (int)order_x; a.oy = (int)order_y; a.tx = (int)target_x; a.ty = (int)target_y;
    a.edge = edge_mode; a.preserve = preserve_alpha; a.divisor = divisor; a.bias = bias;
    a.tiles_x = (int)((cols + T - 1) / T);
    const size_t tiles = (size_t)a.tiles_x * (size_t)((rows + T - 1) / T);
    HIPCHK(enter_ctx(ctx));
    return upload_launch_wait(ctx, "svgr_layer_convolve_matrix", {{kernel, sizeof(double) * (size_t)(order_x * order_y)}}, [&](void* dev) {
        SVGR_LAUNCH(k_layer_convolve_matrix, dim3((unsigned)tiles), dim3(T, T), (unsigned)lds(T), ctx->stream, (double*)out->ptr,
                    (const double*)src->ptr, (const double*)dev, a);
    });
}

int svgr_layer_displacement_map(svgr_ctx* ctx, svgr_buf* out, const int64_t* out_bbox, const svgr_buf* map, const svgr_buf* src,
                                const int64_t* src_bbox, const double* lin4, double scale, int x_channel, int y_channel) {
    DmLaunch a;
    if (!ctx || !out || !map || !src || !lin4 || !box_of(out_bbox, a.ob) || !box_of(src_bbox, a.sb) || x_channel < 0 || x_channel > 3 ||
        y_channel < 0 || y_channel > 3)
        return fail(SVGR_E_INVALID, "svgr_layer_displacement_map: bad arguments (channels 0..3)");
    const size_t n = box_px(a.ob);
    if (out->bytes < n * 32 || map->bytes < n * 32 || src->bytes < box_px(a.sb) * 32)
        return fail(SVGR_E_INVALID, "svgr_layer_displacement_map: buffer too small");
    if (out->ptr == src->ptr || out->ptr == map->ptr) return fail(SVGR_E_INVALID, "svgr_layer_displacement_map: out must not be an input");
    if (n == 0) return 0;
    a.xc = x_channel; a.yc = y_channel;
    a.l00 = lin4[0]; a.l01 = lin4[1]; a.l10 = lin4[2]; a.l11 = lin4[3]; a.scale = scale;
    return launch_tail(ctx, k_layer_displacement_map, grid1(n), dim3(256), 0, (double*)out->ptr, (const double*)map->ptr,
                       (const double*)src->ptr, a);
}

int svgr_layer_lighting(svgr_ctx* ctx, svgr_buf* out, const int64_t* out_bbox, const svgr_buf* src, const int64_t* src_bbox,
                        int light_kind, const double* light_params, const double* color3, double surface_scale, double constant,
                        double specular_exponent, int specular) {
    LightLaunch a;
    if (!ctx || !out || !src || !light_params || !color3 || !box_of(out_bbox, a.ob) || !box_of(src_bbox, a.sb) || light_kind < svgr::kLightDistant ||
        light_kind > svgr::kLightSpot || (specular != 0 && specular != 1))
        return fail(SVGR_E_INVALID, "svgr_layer_lighting: bad arguments (light kind 0..2, specular 0 or 1)");
    if (!all_finite(light_params, 8) || !all_finite(color3, 3) || !std::isfinite(surface_scale) || !std::isfinite(constant) ||
        !std::isfinite(specular_exponent))
        return fail(SVGR_E_INVALID, "svgr_layer_lighting: light parameters, colour, surface scale, constant and exponent must be finite");
    const size_t n = box_px(a.ob);
    a.tiles_x = (a.ob.cols + kLightTile - 1) / kLightTile;
    const size_t tiles = (size_t)a.tiles_x * (size_t)((a.ob.rows + kLightTile - 1) / kLightTile);
    if (tiles > 0x7fffffff) return fail(SVGR_E_INVALID, "svgr_layer_lighting: region too large");
    if (out->bytes < n * 32 || src->bytes < box_px(a.sb) * 32)
        return fail(SVGR_E_INVALID, "svgr_layer_lighting: buffer too small");
    if (out->ptr == src->ptr) return fail(SVGR_E_INVALID, "svgr_layer_lighting: out must not be src");
    if (n == 0) return 0;
    memcpy(a.p.l, light_params, sizeof a.p.l);
    memcpy(a.p.color, color3, sizeof a.p.color);
    a.p.surface_scale = surface_scale; a.p.constant = constant; a.p.specular_exponent = specular_exponent;
    a.p.kind = light_kind; a.p.specular = specular;
    return launch_tail(ctx, k_layer_lighting, dim3((unsigned)tiles), dim3(kLightTile, kLightTile), 0, (double*)out->ptr,
                       (const double*)src->ptr, a);
}

int svgr_layer_tile(svgr_ctx* ctx, svgr_buf* out, const int64_t* out_bbox, const svgr_buf* src, const int64_t* src_bbox,
                    const int64_t* tile_bbox) {
    TileLaunch a;
    if (!ctx || !out || !src || !box_of(out_bbox, a.ob) || !box_of(src_bbox, a.sb) || !box_of(tile_bbox, a.tb))
        return fail(SVGR_E_INVALID, "svgr_layer_tile: bad arguments");
    if (box_px(a.ob) == 0 || box_px(a.tb) == 0)
        return fail(SVGR_E_INVALID, "svgr_layer_tile: empty tile or output");
    // (the kernel's index arithmetic is 32-bit: an output coordinate relative to the tile's origin, and the half pixels of a row)
    for (int k = 0; k < 2; ++k)
        if (std::llabs(out_bbox[k] - tile_bbox[k]) + out_bbox[2 + k] + kTileRows >= (1ll << 31)) return fail(SVGR_E_INVALID, "svgr_layer_tile: output too far from the tile");
    const size_t chunks = ((size_t)a.ob.cols * 2 + 255) / 256;
    const size_t groups = chunks * (size_t)((a.ob.rows + kTileRows - 1) / kTileRows);
    if (a.ob.cols >= (1 << 29) || groups > 0x7fffffff) return fail(SVGR_E_INVALID, "svgr_layer_tile: output too large");
    if (out->bytes < box_px(a.ob) * 32 || src->bytes < box_px(a.sb) * 32)
        return fail(SVGR_E_INVALID, "svgr_layer_tile: buffer too small");
    if (out->ptr == src->ptr) return fail(SVGR_E_INVALID, "svgr_layer_tile: out must not be src");
    a.chunks = (int)chunks;
    return launch_tail(ctx, k_layer_tile, dim3((unsigned)groups), dim3(256), 0, (double2*)out->ptr, (const double2*)src->ptr, a);
}

int svgr_layer_mix_blend(svgr_ctx* ctx, svgr_buf* out, const int64_t* ob, const svgr_buf* backdrop, const int64_t* bb, int bch,
                         const svgr_buf* src, const int64_t* sb, int sch, int mode) {
    if (mode < svgr::kBlendNormal || mode >= svgr::kBlendModes) return fail(SVGR_E_INVALID, "svgr_layer_mix_blend: unknown mode %d", mode);
    MixBlendLaunch a;
    if (int rc = check_layer_pair("svgr_layer_mix_blend", ctx, out, ob, a.ob, src, sb, a.sb, sch)) return rc;
    if (int rc = check_layer_pair("svgr_layer_mix_blend", ctx, out, ob, a.ob, backdrop, bb, a.bb, bch)) return rc;
    if (src->ptr == out->ptr) return fail(SVGR_E_INVALID, "svgr_layer_mix_blend: out must not be the source");
    const bool in_place = backdrop->ptr == out->ptr;
    if (in_place && (bch != 4 || bb[0] != ob[0] || bb[1] != ob[1] || bb[2] != ob[2] || bb[3] != ob[3]))
        return fail(SVGR_E_INVALID, "svgr_layer_mix_blend: in place, the backdrop is out (4 channels, the same box)");
    a.bch = bch; a.sch = sch;
    // (in place only the pixels under the source change: the window is the source's box, clipped to out's)
    a.win = in_place ? box_meet(a.ob, a.sb) : a.ob;
    if (box_px(a.win) == 0) return 0;
    return launch_tail(ctx, mix_blend_kernel(mode, std::make_integer_sequence<int, svgr::kBlendModes>{}), grid1(box_px(a.win)), dim3(256), 0,
                       (double*)out->ptr, (const double*)backdrop->ptr, (const double*)src->ptr, a);
}

int svgr_layer_luminance(svgr_ctx* ctx, svgr_buf* out, const svgr_buf* src, int64_t n_px) {
    if (!ctx || !out || !src || n_px < 0 || out->bytes < (size_t)n_px * 8 || src->bytes < (size_t)n_px * 32) return fail(SVGR_E_INVALID, "svgr_layer_luminance: bad arguments");
    if (n_px == 0) return 0;
    return launch_tail(ctx, k_layer_luminance, grid1((size_t)n_px), dim3(256), 0, (double*)out->ptr, (const double*)src->ptr, (size_t)n_px);
}

int svgr_layer_crop4(svgr_ctx* ctx, svgr_buf* out, const int64_t* ob, const svgr_buf* src, const int64_t* sb, int ch) {
    Box o, s;
    if (int rc = check_layer_pair("svgr_layer_crop4", ctx, out, ob, o, src, sb, s, ch)) return rc;
    const size_t n = box_px(o);
    if (n == 0) return 0;
    return launch_tail(ctx, k_layer_crop4, grid1(n), dim3(256), 0, (double*)out->ptr, o, (const double*)src->ptr, s, ch);
}

int svgr_layer_in(svgr_ctx* ctx, svgr_buf* out, const int64_t* ob, const svgr_buf* src, const int64_t* sb, int ch) {
    Box o, s;
    if (int rc = check_layer_pair("svgr_layer_in", ctx, out, ob, o, src, sb, s, ch)) return rc;
    const size_t n = box_px(o);
    if (n == 0) return 0;
    return launch_tail(ctx, k_layer_in, grid1(n), dim3(256), 0, (double*)out->ptr, o, (const double*)src->ptr, s, ch);
}

int svgr_layer_scale_to(svgr_ctx* ctx, svgr_buf* dst, const svgr_buf* src, int64_t n, double f) {
    if (!ctx || !dst || !src || n < 0 || dst->bytes < (size_t)n * 8 || src->bytes < (size_t)n * 8)
        return fail(SVGR_E_INVALID, "svgr_layer_scale: bad arguments");
    if (n == 0) return 0;
    return launch_tail(ctx, k_layer_scale, grid1((size_t)n), dim3(256), 0, (double*)dst->ptr, (const double*)src->ptr, (size_t)n, f);
}
int svgr_layer_scale(svgr_ctx* ctx, svgr_buf* img, int64_t n, double f) { return svgr_layer_scale_to(ctx, img, img, n, f); }

int svgr_layer_clip01(svgr_ctx* ctx, svgr_buf* img, int64_t n) {
    if (!ctx || !img || n < 0 || img->bytes < (size_t)n * 8) return fail(SVGR_E_INVALID, "svgr_layer_clip01: bad arguments");
    if (n == 0) return 0;
    return launch_tail(ctx, k_layer_clip01, grid1((size_t)n), dim3(256), 0, (double*)img->ptr, (size_t)n);
}

int svgr_layer_background(svgr_ctx* ctx, svgr_buf* img, int64_t n_px, const double* rgba) {
    if (!ctx || !img || !rgba || n_px < 0 || img->bytes < (size_t)n_px * 32) return fail(SVGR_E_INVALID, "svgr_layer_background: bad arguments");
    if (n_px == 0) return 0;
    return launch_tail(ctx, k_layer_background, grid1((size_t)n_px), dim3(256), 0, (double*)img->ptr, (size_t)n_px, rgba[0],
                       rgba[1], rgba[2], rgba[3]);
}

int svgr_layer_convert_to(svgr_ctx* ctx, svgr_buf* dst, const svgr_buf* src, int64_t n_px, unsigned ops) {
    if (!ctx || !dst || !src || n_px < 0 || dst->bytes < (size_t)n_px * 32 || src->bytes < (size_t)n_px * 32 || (ops & ~15u))
        return fail(SVGR_E_INVALID, "svgr_layer_convert: bad arguments");
    if (n_px == 0 || (ops == 0 && dst->ptr == src->ptr)) return 0;
    return launch_tail(ctx, k_layer_convert<false>, grid1((size_t)n_px), dim3(256), 0, (double*)dst->ptr, (const double*)src->ptr, (size_t)n_px, ops, 1.0);
}
int svgr_layer_convert(svgr_ctx* ctx, svgr_buf* img, int64_t n_px, unsigned ops) { return svgr_layer_convert_to(ctx, img, img, n_px, ops); }

int svgr_layer_convert_scale_to(svgr_ctx* ctx, svgr_buf* dst, const svgr_buf* src, int64_t n_px, unsigned ops, double factor) {
    if (!ctx || !dst || !src || n_px < 0 || dst->bytes < (size_t)n_px * 32 || src->bytes < (size_t)n_px * 32 || (ops & ~15u))
        return fail(SVGR_E_INVALID, "svgr_layer_convert_scale_to: bad arguments");
    if (n_px == 0) return 0;
    return launch_tail(ctx, k_layer_convert<true>, grid1((size_t)n_px), dim3(256), 0, (double*)dst->ptr, (const double*)src->ptr, (size_t)n_px, ops, factor);
}

static int layer_compose_many(svgr_ctx* ctx, svgr_buf* out, const int64_t* ob, int64_t n, svgr_buf* const* srcs, const int64_t* sbs,
                              const int32_t* chs, const uint32_t* ops, bool in_mode);
int svgr_layer_compose_over(svgr_ctx* ctx, svgr_buf* out, const int64_t* ob, int64_t n, svgr_buf* const* srcs, const int64_t* sbs,
                            const int32_t* chs, const uint32_t* ops) {
    return layer_compose_many(ctx, out, ob, n, srcs, sbs, chs, ops, false);
}
int svgr_layer_compose_in(svgr_ctx* ctx, svgr_buf* out, const int64_t* ob, int64_t n, svgr_buf* const* srcs, const int64_t* sbs,
                          const int32_t* chs, const uint32_t* ops) {
    return layer_compose_many(ctx, out, ob, n, srcs, sbs, chs, ops, true);
}
static int layer_compose_many(svgr_ctx* ctx, svgr_buf* out, const int64_t* ob, int64_t n, svgr_buf* const* srcs, const int64_t* sbs,
                              const int32_t* chs, const uint32_t* ops, bool in_mode) {
    Box o;
    if (!ctx || !out || !box_of(ob, o) || n <= 0 || !srcs || !sbs || !chs) return fail(SVGR_E_INVALID, "svgr_layer_compose_over / _in: bad arguments");
    const size_t n_out = box_px(o);
    if (out->bytes < n_out * 32) return fail(SVGR_E_INVALID, "svgr_layer_compose_over: output buffer too small");
    return abi_guard("svgr_layer_compose_over / _in", [&]() -> int {
        // every source is checked, and its box narrowed, as it goes into its table: OVER_SRCS to a launch
        std::vector<OverTable> tables((size_t)((n + OVER_SRCS - 1) / OVER_SRCS));
        memset(tables.data(), 0, tables.size() * sizeof(OverTable));
        for (int64_t i = 0; i < n; ++i) {
            OverTable& t = tables[(size_t)(i / OVER_SRCS)];
            OverSrc& s = t.s[t.n++];
            if (!srcs[i] || !box_of(sbs + 4 * i, s.b) || (chs[i] != 1 && chs[i] != 4) || (ops && ((ops[i] & ~15u) || (ops[i] && chs[i] != 4))))
                return fail(SVGR_E_INVALID, "svgr_layer_compose_over: bad source %lld", (long long)i);
            if (srcs[i]->bytes < box_px(s.b) * 8 * chs[i]) return fail(SVGR_E_INVALID, "svgr_layer_compose_over: source %lld too small", (long long)i);
            if (srcs[i]->ptr == out->ptr) return fail(SVGR_E_INVALID, "svgr_layer_compose_over: the output is one of the sources");
            s.p = (const double*)srcs[i]->ptr;
            s.ch = chs[i]; s.ops = ops ? ops[i] : 0u;
            t.accumulate = i >= OVER_SRCS ? 1 : 0;
        }
        if (n_out == 0) return 0;
        HIPCHK(enter_ctx(ctx));
        const auto kernel = in_mode ? k_layer_compose<true> : k_layer_compose<false>;
        for (const OverTable& t : tables) SVGR_LAUNCH(kernel, grid1(n_out), dim3(256), 0, ctx->stream, (double*)out->ptr, o, t);
        HIPCHK(hipGetLastError());
        return 0;
    });
}

int svgr_layer_to_f32(svgr_ctx* ctx, svgr_buf* dst, const svgr_buf* src, int64_t n, int clip01) {
    if (!ctx || !dst || !src || n < 0 || dst->bytes < (size_t)n * 4 || src->bytes < (size_t)n * 8) return fail(SVGR_E_INVALID, "svgr_layer_to_f32: bad arguments");
    if (n == 0) return 0;
    return launch_tail(ctx, k_to_f32, grid1((size_t)n), dim3(256), 0, (float*)dst->ptr, (const double*)src->ptr, (size_t)n, clip01);
}

int svgr_layer_to_rgba8(svgr_ctx* ctx, svgr_buf* dst, const svgr_buf* src, int64_t n_px) {
    if (!ctx || !dst || !src || n_px < 0 || dst->bytes < (size_t)n_px * 4 || src->bytes < (size_t)n_px * 32) return fail(SVGR_E_INVALID, "svgr_layer_to_rgba8: bad arguments");
    if (n_px == 0) return 0;
    return launch_tail(ctx, k_to_rgba8, grid1((size_t)n_px), dim3(256), 0, (uchar4*)dst->ptr, (const double4*)src->ptr, (size_t)n_px);
}

// the gradient over the pixel grid of `box` times `mask` (pts == nullptr), or at the n = rows * cols points of `pts`
static int gradient_run(svgr_ctx* ctx, const svgr_gradient* g, const double* pts, const svgr_buf* mask, const Box& box, svgr_buf* out) {
    if (int rc = check_gradient(g)) return rc;
    const size_t n = box_px(box);
    if ((mask && mask->bytes < n * 8) || out->bytes < n * 32) return fail(SVGR_E_INVALID, "svgr_gradient_fill: buffer too small");
    if (n == 0) return 0;
    const double* mptr = mask ? (const double*)mask->ptr : nullptr;
    GradDev h;
    fill_grad_dev(h, g);
    HIPCHK(enter_ctx(ctx));
    hipError_t e = hipSuccess;
    const dim3 ggrid((unsigned)(((long long)box.cols + 255) / 256), (unsigned)std::min<long long>(box.rows, 32768));
    PoolBlock ext;  // long stop lists: one device block {offsets, colours}
    if (g->n_stops <= GRAD_MAX_STOPS) {
        for (int i = 0; i < g->n_stops; ++i) {
            h.stop_off[i] = g->stop_off[i];
            for (int k = 0; k < 4; ++k) h.stop_rgba[i][k] = g->stop_rgba[4 * i + k];
        }
    } else {
        const size_t ns = (size_t)g->n_stops;
        HIPCHK(ext.alloc(sizeof(double) * 5 * ns, ctx->device));
        e = hipMemcpyAsync(ext.p, g->stop_off, sizeof(double) * ns, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(ext.as<double>() + ns, g->stop_rgba, sizeof(double) * 4 * ns, hipMemcpyHostToDevice, ctx->stream);
        if (e != hipSuccess) return fail(SVGR_E_HIP, "svgr_gradient_fill: %s", hipGetErrorString(e));
        h.ext_stops = ext.as<double>();
    }
    if (g->kind == 3) {
        // the two-circle gradient needs a device flag (any det < 0 ?) between its two kernels: a word from the block cache
        PoolBlock flag;
        HIPCHK(flag.alloc(16));
        e = hipMemsetAsync(flag.p, 0, 16, ctx->stream);
        if (e == hipSuccess) {
            SVGR_LAUNCH(k_gradient_detneg, ggrid, dim3(256), 0, ctx->stream, h, pts, box, flag.as<int>());
            SVGR_LAUNCH(k_gradient_fill, ggrid, dim3(256), 0, ctx->stream, h, pts, mptr, box, (const int*)flag.p, (double*)out->ptr);
            e = hipGetLastError();
        }
    } else {
        SVGR_LAUNCH(k_gradient_fill, ggrid, dim3(256), 0, ctx->stream, h, pts, mptr, box, (const int*)nullptr, (double*)out->ptr);
        e = hipGetLastError();
    }
    // (the stops are the caller's host arrays: the copies above must have been consumed before returning)
    if (ext.p && e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return fail(SVGR_E_HIP, "svgr_gradient_fill: %s", hipGetErrorString(e));
    return 0;
}

int svgr_gradient_fill(svgr_ctx* ctx, const svgr_gradient* g, const svgr_buf* mask, const int64_t* bbox, svgr_buf* out) {
    Box box;
    if (!ctx || !g || !mask || !out || !box_of(bbox, box)) return fail(SVGR_E_INVALID, "svgr_gradient_fill: bad arguments");
    return gradient_run(ctx, g, nullptr, mask, box, out);
}

int svgr_gradient_eval(svgr_ctx* ctx, const svgr_gradient* g, const svgr_buf* points, int64_t n_points, svgr_buf* out) {
    if (!ctx || !g || !points || !out || n_points < 0 || n_points > ((int64_t)1 << 31) - 1 || points->bytes < (size_t)n_points * 16)
        return fail(SVGR_E_INVALID, "svgr_gradient_eval: bad arguments");
    const Box as_row{0, 0, 1, (int)n_points};   // (one row of up to 2^31 - 1 points: wider than box_of admits, and no layer)
    return gradient_run(ctx, g, (const double*)points->ptr, nullptr, as_row, out);
}

int svgr_pattern_fill(svgr_ctx* ctx, const svgr_pattern* pt, const svgr_buf* tile, const svgr_buf* mask, const int64_t* bbox,
                      svgr_buf* out) {
    Box box;
    if (!ctx || !pt || !tile || !mask || !out || !box_of(bbox, box)) return fail(SVGR_E_INVALID, "svgr_pattern_fill: bad arguments");
    if (!(pt->cell[2] == pt->cell[2]) || !(pt->cell[3] == pt->cell[3]) || pt->pat_shape[0] <= 0 || pt->pat_shape[1] <= 0 ||
        pt->tile_bbox[2] < 0 || pt->tile_bbox[3] < 0 || pt->tile_bbox[2] > (1 << 24) || pt->tile_bbox[3] > (1 << 24))
        return fail(SVGR_E_INVALID, "svgr_pattern_fill: bad pattern geometry");
    const size_t n = box_px(box);
    if (mask->bytes < n * 8 || out->bytes < n * 32 || tile->bytes < (size_t)pt->tile_bbox[2] * (size_t)pt->tile_bbox[3] * 32)
        return fail(SVGR_E_INVALID, "svgr_pattern_fill: buffer too small");
    if (n == 0) return 0;
    HIPCHK(enter_ctx(ctx));
    PoolBlock flag;
    HIPCHK(flag.alloc(16));
    int oob = 0;
    hipError_t e = hipMemsetAsync(flag.p, 0, 16, ctx->stream);
    if (e == hipSuccess) {
        SVGR_LAUNCH(k_pattern_fill, grid1(n), dim3(256), 0, ctx->stream, *pt, (const double*)tile->ptr, (const double*)mask->ptr,
                           box, flag.as<int>(), (double*)out->ptr);
        e = hipMemcpyAsync(&oob, flag.p, sizeof oob, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e == hipSuccess) e = hipGetLastError();
    }
    if (e != hipSuccess) return fail(SVGR_E_HIP, "svgr_pattern_fill: %s", hipGetErrorString(e));
    if (oob) return fail(SVGR_E_INVALID, "svgr_pattern_fill: a tile offset falls outside the pattern canvas");
    return 0;
}

// the mip chain of an (h, w) image: level k's size and its first texel in the one buffer that holds them all
static int64_t image_level(int64_t h, int64_t w, int64_t k, int64_t* lh, int64_t* lw) {
    int64_t off = 0;
    for (int64_t i = 0; i < k; ++i) {
        off += h * w;
        h = (h + 1) / 2;
        w = (w + 1) / 2;
    }
    *lh = h;
    *lw = w;
    return off;
}
static int64_t image_n_levels(int64_t h, int64_t w) {
    int64_t n = 1;
    for (; h > 1 || w > 1; ++n) { h = (h + 1) / 2; w = (w + 1) / 2; }
    return n;
}
static bool image_size_ok(int64_t h, int64_t w) { return h > 0 && w > 0 && h <= (1 << 16) && w <= (1 << 16) && h * w <= ((int64_t)1 << 30); }

int svgr_image_upload(svgr_ctx* ctx, const uint8_t* rgba, int64_t h, int64_t w, int linear_rgb, svgr_buf* levels) {
    if (!ctx || !rgba || !levels || !image_size_ok(h, w)) return fail(SVGR_E_INVALID, "svgr_image_upload: bad arguments");
    const int64_t nl = image_n_levels(h, w);
    int64_t lh, lw;
    const int64_t total = image_level(h, w, nl, &lh, &lw);
    if (levels->bytes < (size_t)total * 16) return fail(SVGR_E_INVALID, "svgr_image_upload: buffer too small");
    HIPCHK(enter_ctx(ctx));
    const size_t n0 = (size_t)h * w;
    PoolBlock staging;
    HIPCHK(staging.alloc(n0 * 4, ctx->device));
    float4* tex = (float4*)levels->ptr;
    hipError_t e = hipMemcpyAsync(staging.p, rgba, n0 * 4, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) {
        const dim3 pgrid((unsigned)std::min<size_t>((n0 + 255) / 256, 2048));
        SVGR_LAUNCH(k_image_prepare, pgrid, dim3(256), 0, ctx->stream, (const uchar4*)staging.p, n0, linear_rgb ? 1 : 0, tex);
        int64_t ph = h, pw = w, off = 0;
        for (int64_t k = 1; k < nl; ++k) {
            const int64_t dh = (ph + 1) / 2, dw = (pw + 1) / 2;
            SVGR_LAUNCH(k_image_downsample, grid1((size_t)(dh * dw)), dim3(256), 0, ctx->stream, (const float4*)(tex + off), (int)ph,
                        (int)pw, tex + off + ph * pw, (int)dh, (int)dw);
            off += ph * pw;
            ph = dh;
            pw = dw;
        }
        e = hipGetLastError();
        // (the caller's array must have been read before the call returns)
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    }
    if (e != hipSuccess) return fail(SVGR_E_HIP, "svgr_image_upload: %s", hipGetErrorString(e));
    return 0;
}

int svgr_image_fill(svgr_ctx* ctx, const svgr_image* im, const svgr_buf* levels, const svgr_buf* mask, const int64_t* bbox,
                    svgr_buf* out) {
    Box box;
    if (!ctx || !im || !levels || !mask || !out || !box_of(bbox, box) || !image_size_ok(im->height, im->width))
        return fail(SVGR_E_INVALID, "svgr_image_fill: bad arguments");
    const int64_t nl = image_n_levels(im->height, im->width);
    if (!(im->lod >= 0.0 && im->lod <= (double)(nl - 1)) || (im->smooth != 0 && im->smooth != 1))
        return fail(SVGR_E_INVALID, "svgr_image_fill: bad level of detail or mode");
    int64_t th, tw;
    const size_t n = box_px(box);
    if (mask->bytes < n * 8 || out->bytes < n * 32 || levels->bytes < (size_t)image_level(im->height, im->width, nl, &th, &tw) * 16)
        return fail(SVGR_E_INVALID, "svgr_image_fill: buffer too small");
    if (n == 0) return 0;
    // the two levels the fill reads (the level of detail is constant over an affine map): floor(lod) and the one above
    const int64_t k = im->smooth ? (int64_t)std::floor(im->lod) : 0;
    const double blend = im->smooth ? im->lod - (double)k : 0.0;
    const int64_t k1 = std::min<int64_t>(k + 1, nl - 1);
    int64_t h0, w0, h1, w1;
    const int64_t o0 = image_level(im->height, im->width, k, &h0, &w0), o1 = image_level(im->height, im->width, k1, &h1, &w1);
    const float4* tex = (const float4*)levels->ptr;
    const ImageLevel lo{tex + o0, (int)h0, (int)w0, std::ldexp(1.0, -(int)k)}, hi{tex + o1, (int)h1, (int)w1, std::ldexp(1.0, -(int)k1)};
    const dim3 grid((unsigned)((box.cols + IMG_TW - 1) / IMG_TW), (unsigned)std::min<int64_t>((box.rows + IMG_TH - 1) / IMG_TH, 32768));
    return launch_tail(ctx, im->smooth ? k_image_fill<true> : k_image_fill<false>, grid, dim3(256), 0, *im, lo, hi, blend,
                       (const double*)mask->ptr, box, (double*)out->ptr);
}

int svgr_jpeg_decode(svgr_ctx* ctx, const svgr_jpeg_frame* frame, const int16_t* coef, int64_t n_coef, const uint16_t* quant,
                     svgr_buf* out) {
    JpegLayout L;
    if (!ctx || !frame || !coef || !quant || !out || !jpeg_layout(*frame, L) || !image_size_ok(frame->height, frame->width))
        return fail(SVGR_E_INVALID, "svgr_jpeg_decode: bad arguments");
    if (n_coef != L.blocks * 64) return fail(SVGR_E_INVALID, "svgr_jpeg_decode: %lld coefficients for a frame of %lld", (long long)n_coef, (long long)L.blocks * 64);
    if (out->bytes < (size_t)frame->width * frame->height * 4) return fail(SVGR_E_INVALID, "svgr_jpeg_decode: buffer too small");
    static_assert(kJpegGrey == SVGR_JPEG_GREY && kJpegYCbCr == SVGR_JPEG_YCBCR && kJpegRGB == SVGR_JPEG_RGB, "colour models");
    HIPCHK(enter_ctx(ctx));
    PoolBlock planes;
    HIPCHK(planes.alloc((size_t)L.plane_bytes, ctx->device));
    const size_t coef_bytes = (size_t)n_coef * 2;   // (a multiple of 128: the tables behind it stay 16-byte aligned)
    return upload_launch_wait(ctx, "svgr_jpeg_decode", {{coef, coef_bytes}, {quant, (size_t)frame->n_comp * 128}}, [&](void* dev) {
        JpegIdctArgs ia;
        ia.coef = (const int16_t*)dev;
        ia.quant = (const uint16_t*)((const char*)dev + coef_bytes);
        ia.planes = planes.as<uint8_t>();
        JpegColourArgs ca;
        for (int i = 0; i < 3; ++i) {
            const int k = i < frame->n_comp ? i : frame->n_comp - 1;
            ia.end[i] = L.base[k] + L.bw[k] * L.bh[k];
            ia.bw[i] = L.bw[i];
            ia.plane[i] = L.plane[i];
            ca.c[i] = JpegPlane{planes.as<uint8_t>() + L.plane[i], L.bw[i] * 8, L.cw[i], L.ch[i], L.hs[i], L.vs[i]};
        }
        ca.width = frame->width; ca.height = frame->height; ca.colour = frame->colour;
        SVGR_LAUNCH(k_jpeg_idct, dim3((unsigned)((L.blocks + JPEG_WG_BLOCKS - 1) / JPEG_WG_BLOCKS)), dim3(256), 0, ctx->stream, ia);
        SVGR_LAUNCH(k_jpeg_colour, dim3((unsigned)((frame->width + 63) / 64), (unsigned)((frame->height + 3) / 4)), dim3(256), 0,
                    ctx->stream, ca, (uint32_t*)out->ptr);
    });
}

int svgr_jpeg_encode(svgr_ctx* ctx, const svgr_jpeg_frame* frame, const svgr_buf* src_rgba8, const uint16_t* quant, int16_t* coef_out,
                     int64_t n_coef) {
    JpegLayout L;
    if (!ctx || !frame || !src_rgba8 || !quant || !coef_out || !jpeg_layout(*frame, L) || !image_size_ok(frame->height, frame->width))
        return fail(SVGR_E_INVALID, "svgr_jpeg_encode: bad arguments");
    if (frame->colour != (frame->n_comp == 1 ? SVGR_JPEG_GREY : SVGR_JPEG_YCBCR))
        return fail(SVGR_E_INVALID, "svgr_jpeg_encode: a frame is written as YCbCr (three components) or grey (one)");
    if (frame->n_comp == 3 && (frame->h[1] != 1 || frame->v[1] != 1 || frame->h[2] != 1 || frame->v[2] != 1))
        return fail(SVGR_E_INVALID, "svgr_jpeg_encode: the chroma components take sampling factors 1 x 1");
    if (n_coef != L.blocks * 64) return fail(SVGR_E_INVALID, "svgr_jpeg_encode: room for %lld coefficients, the frame has %lld", (long long)n_coef, (long long)L.blocks * 64);
    if (src_rgba8->bytes < (size_t)frame->width * frame->height * 4) return fail(SVGR_E_INVALID, "svgr_jpeg_encode: buffer too small");
    for (int i = 0; i < frame->n_comp * 64; ++i)
        if (quant[i] < 1 || quant[i] > 255) return fail(SVGR_E_INVALID, "svgr_jpeg_encode: quantisation table entry %d of component %d is %d (1 .. 255)", i & 63, i >> 6, (int)quant[i]);
    HIPCHK(enter_ctx(ctx));
    PoolBlock planes, coef;
    HIPCHK(planes.alloc((size_t)L.plane_bytes, ctx->device));
    HIPCHK(coef.alloc((size_t)n_coef * 2, ctx->device));
    return upload_launch_wait(ctx, "svgr_jpeg_encode", {{quant, (size_t)frame->n_comp * 128}}, [&](void* dev) {
        const int H = frame->h[0], V = frame->v[0];   // (1 x 1 for a grey frame)
        JpegPlanesArgs pa;
        pa.rgba = (const uint32_t*)src_rgba8->ptr;
        pa.y = planes.as<uint8_t>() + L.plane[0];
        pa.cb = planes.as<uint8_t>() + L.plane[1];
        pa.cr = planes.as<uint8_t>() + L.plane[2];
        pa.width = frame->width; pa.height = frame->height; pa.n_comp = frame->n_comp;
        pa.gw = (int)(L.bw[0] * 8 / H); pa.gh = (int)(L.bh[0] * 8 / V);
        JpegFdctArgs fa;
        fa.planes = planes.as<uint8_t>();
        fa.quant = (const uint16_t*)dev;
        fa.coef = coef.as<int16_t>();
        for (int i = 0; i < 3; ++i) {
            const int k = i < frame->n_comp ? i : frame->n_comp - 1;
            fa.end[i] = L.base[k] + L.bw[k] * L.bh[k];
            fa.bw[i] = L.bw[i];
            fa.plane[i] = L.plane[i];
        }
        const dim3 pgrid((unsigned)((pa.gw + 63) / 64), (unsigned)((pa.gh + 3) / 4));
        if (H == 2 && V == 2) SVGR_LAUNCH((k_jpeg_planes<2, 2>), pgrid, dim3(256), 0, ctx->stream, pa);
        else if (H == 2) SVGR_LAUNCH((k_jpeg_planes<2, 1>), pgrid, dim3(256), 0, ctx->stream, pa);
        else if (V == 2) SVGR_LAUNCH((k_jpeg_planes<1, 2>), pgrid, dim3(256), 0, ctx->stream, pa);
        else SVGR_LAUNCH((k_jpeg_planes<1, 1>), pgrid, dim3(256), 0, ctx->stream, pa);
        SVGR_LAUNCH(k_jpeg_fdct, dim3((unsigned)((L.blocks + JPEG_WG_BLOCKS - 1) / JPEG_WG_BLOCKS)), dim3(256), 0, ctx->stream, fa);
        // (the one wait of upload_launch_wait covers this copy too)
        (void)hipMemcpyAsync(coef_out, coef.p, (size_t)n_coef * 2, hipMemcpyDeviceToHost, ctx->stream);
    });
}

static int layer_convolve_impl(svgr_ctx* ctx, svgr_buf* out, const svgr_buf* src, int64_t rows, int64_t cols, const double* kernel,
                               int64_t kw, int64_t kh, unsigned src_ops);
int svgr_layer_convolve(svgr_ctx* ctx, svgr_buf* out, const svgr_buf* src, int64_t rows, int64_t cols, const double* kernel,
                        int64_t kw, int64_t kh) {
    // (the separability test builds host vectors: std::bad_alloc must not cross the ABI)
    return abi_guard("svgr_layer_convolve", [&]() { return layer_convolve_impl(ctx, out, src, rows, cols, kernel, kw, kh, 0u); });
}
int svgr_layer_convolve_ops(svgr_ctx* ctx, svgr_buf* out, const svgr_buf* src, int64_t rows, int64_t cols, const double* kernel,
                            int64_t kw, int64_t kh, unsigned src_ops) {
    if (src_ops & ~15u) return fail(SVGR_E_INVALID, "svgr_layer_convolve_ops: unknown conversion ops");
    return abi_guard("svgr_layer_convolve_ops", [&]() { return layer_convolve_impl(ctx, out, src, rows, cols, kernel, kw, kh, src_ops); });
}

static int layer_convolve_impl(svgr_ctx* ctx, svgr_buf* out, const svgr_buf* src, int64_t rows, int64_t cols, const double* kernel,
                               int64_t kw, int64_t kh, unsigned src_ops) {
    if (!ctx || !out || !src || !kernel || rows <= 0 || cols <= 0 || kw <= 0 || kh <= 0 || rows > (1 << 24) || cols > (1 << 24) ||
        kw > 4096 || kh > 4096)
        return fail(SVGR_E_INVALID, "svgr_layer_convolve: bad arguments");
    const size_t n_out = (size_t)(rows + kw - 1) * (size_t)(cols + kh - 1);
    if (src->bytes < (size_t)rows * cols * 32 || out->bytes < n_out * 32) return fail(SVGR_E_INVALID, "svgr_layer_convolve: buffer too small");
    HIPCHK(enter_ctx(ctx));
    const std::shared_ptr<const Analysed> an = analyse_kernel(kernel, kw, kh);
    const double total = an->total;
    const bool separable = an->separable && getenv("SVGR_BLUR_DIRECT") == nullptr;
    static const bool dbg_conv = getenv("SVGR_DBG_CONV") != nullptr;
    const bool blocked = separable && kw <= CONV_TAPS && kh <= CONV_TAPS && rows <= 65535;  // (the row index rides in gridDim.y)
    if (dbg_conv) fprintf(stderr, "[convolve] %lld x %lld layer, %lld x %lld kernel, ops %u: %s\n", (long long)rows, (long long)cols, (long long)kw,
                          (long long)kh, src_ops, blocked ? "two blocked passes" : separable ? "two plain passes" : "direct");
    // (the passes that do not convert as they read: the source converted first, into a block of its own)
    PoolBlock conv_src;
    const double* src_px = (const double*)src->ptr;
    if (src_ops && !blocked) {
        HIPCHK(conv_src.alloc((size_t)rows * cols * 32, ctx->device));
        SVGR_LAUNCH(k_layer_convert<false>, grid1((size_t)rows * cols), dim3(256), 0, ctx->stream, conv_src.as<double>(), src_px, (size_t)rows * cols, src_ops, 1.0);
        src_px = conv_src.as<double>();
    }
    if (blocked) {
        // along the rows first (the pass that stages its source in LDS converts it there), then down the columns; K = (u / S) v^T
        ConvW cu{}, cv{};
        cu.n = (int)kw; cv.n = (int)kh;
        for (int64_t i = 0; i < kw; ++i) cu.w[i] = an->u[(size_t)i] / total;
        for (int64_t j = 0; j < kh; ++j) cv.w[j] = an->v[(size_t)j];
        const int64_t ocols = cols + kh - 1;
        const size_t n_tmp = (size_t)rows * (size_t)ocols;
        PoolBlock tmp;
        HIPCHK(tmp.alloc(n_tmp * 32, ctx->device));
        SVGR_LAUNCH(k_convolve_cols, dim3((unsigned)((ocols + 255) / 256), (unsigned)rows), dim3(256), 0, ctx->stream, tmp.as<double>(), src_px,
                           (int)rows, (int)cols, cv, src_ops);
        SVGR_LAUNCH(k_convolve_rows, dim3((unsigned)((ocols + 63) / 64), (unsigned)((rows + kw - 1 + CONV_RB - 1) / CONV_RB)), dim3(64), 0,
                           ctx->stream, (double*)out->ptr, (const double*)tmp.p, (int)rows, (int)ocols, cu);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return fail(SVGR_E_HIP, "svgr_layer_convolve: %s", hipGetErrorString(e));
        return 0;
    }
    if (separable) {
        std::vector<double> u(an->u);
        for (auto& x : u) x /= total;  // K = (u / S) v^T
        const size_t n_tmp = (size_t)(rows + kw - 1) * (size_t)cols;
        PoolBlock tmp;
        HIPCHK(tmp.alloc(n_tmp * 32));
        return upload_launch_wait(ctx, "svgr_layer_convolve", {{u.data(), sizeof(double) * (size_t)kw}, {an->v.data(), sizeof(double) * (size_t)kh}},
                                  [&](void* dw) {
            SVGR_LAUNCH(k_layer_convolve_1d<0>, grid1(n_tmp), dim3(256), 0, ctx->stream, tmp.as<double>(), src_px, (int)rows,
                               (int)cols, (const double*)dw, (int)kw);
            SVGR_LAUNCH(k_layer_convolve_1d<1>, grid1(n_out), dim3(256), 0, ctx->stream, (double*)out->ptr, (const double*)tmp.p,
                               (int)(rows + kw - 1), (int)cols, (const double*)dw + kw, (int)kh);
        });
    }
    if (kw * kh <= CONV_TAPS) {
        ConvW ck{};
        ck.n = (int)(kw * kh);
        for (int64_t i = 0; i < kw * kh; ++i) ck.w[i] = kernel[i];
        SVGR_LAUNCH(k_layer_convolve_small, grid1(n_out), dim3(256), 0, ctx->stream, (double*)out->ptr, src_px, (int)rows, (int)cols, ck,
                           (int)kw, (int)kh);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return fail(SVGR_E_HIP, "svgr_layer_convolve: %s", hipGetErrorString(e));
        return 0;
    }
    return upload_launch_wait(ctx, "svgr_layer_convolve", {{kernel, sizeof(double) * (size_t)kw * kh}}, [&](void* dk) {
        SVGR_LAUNCH(k_layer_convolve, grid1(n_out), dim3(256), 0, ctx->stream, (double*)out->ptr, src_px,
                           (int)rows, (int)cols, (const double*)dk, (int)kw, (int)kh);
    });
}

}  // extern "C"

// ======================================================================================
// Path.dash: stroke-dasharray / stroke-dashoffset in front of the host stroker (svgr_path_dash).
// The per-lane arithmetic is svgr_dash.h; DESIGN.md "Dashed strokes" has the definitions.
//
//   k_dash_measure   32 lanes per segment (two segments per wave): lane i integrates sub-interval i of a cubic, a 32-lane
//                    inclusive scan gives the segment's cumulative table and its length; a line costs one lane
//   k_scan_*         two-level scans, DASH_S items per workgroup: the segment lengths restart at every subpath (a segmented
//                    scan), the piece / dash counts run over the whole path.  Their association depends on the launch
//                    geometry alone, never on the order in which waves run
//   k_dash_pattern   one workgroup: the path's total length (pathLength scales the pattern by it) and the pattern's tables
//   k_dash_count     per segment, closed form: the pieces it emits and the output subpaths it starts
//   k_dash_wrap      per subpath: where its pieces and dashes begin, and, for a closed subpath whose trailing and leading
//                    dash are one, how many pieces the leading dash has (they are placed behind the trailing ones)
//   k_dash_emit      32 lanes per segment stride over its pieces: invert both ends, split, store at the piece's place
//   k_dash_close     per output subpath: its terminating line and its size
// Every place is a prefix sum; no atomic takes part.  All geometry is f64.
// ======================================================================================
#include "svgr_dash.h"
#include "svgr_stroke_out.h"

constexpr int DASH_S = 1024;      // segments one workgroup scans (256 threads x 4): the test shapes sit at its multiples
constexpr int DASH_SEGS_WG = 8;   // segments per workgroup of the 32-lanes-per-segment kernels
// The pieces one segment may have.  Its 32 lanes stride over them, so this bounds the time of one half-wave: 2^15 rounds of two
// inversions.  (The path's total is bounded by the 32-bit counts of the result alone.)
constexpr long long DASH_SEG_PIECES_MAX = 1ll << 20;
constexpr double DASH_COORD_MAX = 1e150;   // beyond it dx * dx leaves the doubles and a length would be infinite

struct DashFV { double v; int f; int pad; };        // segmented sum: f = a subpath begins at or in front of this item
struct DashCnt { long long p, d; };                 // pieces, output subpaths
struct DashFVOp {
    __device__ static DashFV zero() { return DashFV{0.0, 0, 0}; }
    __device__ static DashFV add(const DashFV& a, const DashFV& b) { return DashFV{b.f ? b.v : a.v + b.v, a.f | b.f, 0}; }
};
struct DashCntOp {
    __device__ static DashCnt zero() { return DashCnt{0, 0}; }
    __device__ static DashCnt add(const DashCnt& a, const DashCnt& b) { return DashCnt{a.p + b.p, a.d + b.d}; }
};
struct DashSub { long long A, n, nl, dbase, nd; int mode, pad; };   // k_dash_wrap's row of a subpath
struct DashTot { DashCnt c; int too_many, pad; };                   // what the host reads back after the counting kernels

// inclusive scan of DASH_S items per workgroup, in place; tot[b] = the workgroup's sum
template <class T, class Op>
__global__ __launch_bounds__(256) void k_scan_block(T* __restrict__ a, T* __restrict__ tot, int n) {
    __shared__ T sh[256];
    const int t = threadIdx.x, base = blockIdx.x * DASH_S + t * 4;
    T v[4];
    T acc = Op::zero();
    for (int i = 0; i < 4; ++i) {
        v[i] = base + i < n ? a[base + i] : Op::zero();
        acc = Op::add(acc, v[i]);
        v[i] = acc;
    }
    sh[t] = acc;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
        T x = sh[t];
        if (t >= d) x = Op::add(sh[t - d], x);
        __syncthreads();
        sh[t] = x;
        __syncthreads();
    }
    const T pre = t ? sh[t - 1] : Op::zero();
    for (int i = 0; i < 4; ++i)
        if (base + i < n) a[base + i] = Op::add(pre, v[i]);
    if (t == 255) tot[blockIdx.x] = sh[255];
}
// one workgroup: tot[b] <- sum of the workgroups in front of b
template <class T, class Op>
__global__ __launch_bounds__(256) void k_scan_tops(T* __restrict__ tot, int nb) {
    __shared__ T sh[256];
    const int t = threadIdx.x;
    T carry = Op::zero();
    for (int base = 0; base < nb; base += 256) {
        const T mine = base + t < nb ? tot[base + t] : Op::zero();
        sh[t] = mine;
        __syncthreads();
        for (int d = 1; d < 256; d <<= 1) {
            T x = sh[t];
            if (t >= d) x = Op::add(sh[t - d], x);
            __syncthreads();
            sh[t] = x;
            __syncthreads();
        }
        const T excl = Op::add(carry, t ? sh[t - 1] : Op::zero());
        if (base + t < nb) tot[base + t] = excl;
        carry = Op::add(carry, sh[255]);
        __syncthreads();
    }
}
template <class T, class Op>
__global__ __launch_bounds__(256) void k_scan_apply(T* __restrict__ a, const T* __restrict__ tot, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int b = i / DASH_S;
    if (i < n && b > 0) a[i] = Op::add(tot[b], a[i]);
}

__global__ __launch_bounds__(256) void k_dash_measure(const int* __restrict__ types, const double* __restrict__ params,
                                                      const int* __restrict__ seg_sub, const int* __restrict__ sub_off, int n,
                                                      double* __restrict__ tab, double* __restrict__ len, DashFV* __restrict__ cum) {
    const int l = threadIdx.x & 31, seg = blockIdx.x * DASH_SEGS_WG + (threadIdx.x >> 5);
    if (seg >= n) return;   // (uniform over the 32 lanes of a segment)
    const int type = types[seg];
    const double* c = params + (size_t)seg * 8;
    double total = 0.0;
    if (type == SVGR_PATH_CUBIC) {
        double x = dash_sub_length(c, l);
        for (int d = 1; d < 32; d <<= 1) {
            const double y = __shfl_up(x, d, 32);
            if (l >= d) x += y;
        }
        tab[(size_t)seg * DASH_SUB + l] = x;
        total = __shfl(x, 31, 32);
    } else if (type != SVGR_PATH_UNCLOSED) {
        total = dash_line_length(c);
    }
    if (l == 0) {
        len[seg] = total;
        cum[seg] = DashFV{total, seg == sub_off[seg_sub[seg]] ? 1 : 0, 0};
    }
}

// one workgroup: the sum of the subpaths' lengths (strided partial sums, then a tree: a fixed association), the pattern from it
__global__ __launch_bounds__(256) void k_dash_pattern(const DashFV* __restrict__ cum, const int* __restrict__ sub_off, int n_sub,
                                                      const double* __restrict__ raw, int n_raw, double offset, double path_length,
                                                      DashPat* __restrict__ pat) {
    __shared__ double sh[256];
    const int t = threadIdx.x;
    double acc = 0.0;
    if (path_length > 0.0)
        for (int s = t; s < n_sub; s += 256) acc += cum[sub_off[s + 1] - 1].v;
    sh[t] = acc;
    __syncthreads();
    for (int d = 128; d >= 1; d >>= 1) {
        if (t < d) sh[t] += sh[t + d];
        __syncthreads();
    }
    if (t == 0) {
        double scale = 1.0;
        if (path_length > 0.0) scale = sh[0] / path_length;
        if (!(scale > 0.0) || !(scale < 1.7e308)) scale = 1.0;   // (a path without length has no pieces either way)
        DashPat p;
        dash_build_pattern(raw, n_raw, offset, scale, p);
        if (!(p.P > 0.0) || !(p.P < 1.7e308)) p.N = 0;           // (a scaled period that left the doubles: nothing is drawn)
        *pat = p;
    }
}

struct DashSegIn { int type, first, last, mode; double len, s0, s1; };
__device__ __forceinline__ DashSegIn dash_seg_in(const DashPat& pat, const int* types, const int* seg_sub, const int* sub_off,
                                                 const double* len, const DashFV* cum, int i) {
    DashSegIn s;
    const int sp = seg_sub[i];
    s.first = sub_off[sp];
    s.last = sub_off[sp + 1] - 1;
    s.type = types[i];
    s.len = len[i];
    s.s1 = cum[i].v;
    s.s0 = i == s.first ? 0.0 : cum[i - 1].v;
    s.mode = dash_sub_mode(pat, cum[s.last].v, types[s.last] == SVGR_PATH_CLOSED);
    return s;
}

__global__ __launch_bounds__(256) void k_dash_count(const DashPat* __restrict__ patp, const int* __restrict__ types,
                                                    const int* __restrict__ seg_sub, const int* __restrict__ sub_off,
                                                    const double* __restrict__ len, const DashFV* __restrict__ cum, int n,
                                                    DashCnt* __restrict__ cnt, DashTot* __restrict__ tot) {
    __shared__ DashPat pat;
    for (int w = threadIdx.x; w < (int)(sizeof(DashPat) / 4); w += 256) ((int*)&pat)[w] = ((const int*)patp)[w];
    __syncthreads();
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const DashSegIn s = dash_seg_in(pat, types, seg_sub, sub_off, len, cum, i);
    DashSeg g;
    dash_seg_pieces(pat, s.type, s.len, s.s0, s.s1, s.mode, g);
    cnt[i] = DashCnt{g.cnt, g.cnt - g.cont};
    if (g.cnt > DASH_SEG_PIECES_MAX) tot->too_many = 1;   // (the host zeroed it; every writer stores the same value)
}

// (cnt: the inclusive scan of k_dash_count's rows; tot[0] = the path's totals, read back by the host)
__global__ __launch_bounds__(256) void k_dash_wrap(const DashPat* __restrict__ patp, const int* __restrict__ types,
                                                   const int* __restrict__ sub_off, const DashFV* __restrict__ cum,
                                                   const DashCnt* __restrict__ cnt, int n, int n_sub, DashSub* __restrict__ sub,
                                                   DashTot* __restrict__ tot) {
    const int sp = blockIdx.x * 256 + threadIdx.x;
    if (sp == 0) tot->c = n ? cnt[n - 1] : DashCnt{0, 0};
    if (sp >= n_sub) return;
    const DashPat& pat = *patp;
    const int first = sub_off[sp], last = sub_off[sp + 1] - 1;
    DashSub r;
    r.A = first ? cnt[first - 1].p : 0;
    r.dbase = first ? cnt[first - 1].d : 0;
    r.n = cnt[last].p - r.A;
    r.nd = cnt[last].d - r.dbase;
    r.mode = dash_sub_mode(pat, cum[last].v, types[last] == SVGR_PATH_CLOSED);
    r.nl = 0;
    r.pad = 0;
    if (r.mode == DASH_MERGED) {
        // the last segment that begins inside the leading dash's interval: the pieces up to its first one are the leading dash
        long long k0, k;
        int j0, j;
        double rr;
        dash_idx_ge(pat, pat.phase, k0, j0, rr);
        int lo = first, hi = last;   // (the first segment begins at 0: inside)
        while (lo < hi) {            // at most 31 halvings of an int range
            const int mid = lo + (hi - lo + 1) / 2;
            dash_idx_ge(pat, cum[mid - 1].v + pat.phase, k, j, rr);
            if (k < k0 || (k == k0 && j <= j0)) lo = mid; else hi = mid - 1;
        }
        const long long before = lo ? cnt[lo - 1].p : 0, own = cnt[lo].p - before;
        r.nl = before + (own > 0 ? 1 : 0) - r.A;
    }
    sub[sp] = r;
}

__global__ __launch_bounds__(256) void k_dash_emit(const DashPat* __restrict__ patp, const int* __restrict__ types,
                                                   const double* __restrict__ params, const int* __restrict__ seg_sub,
                                                   const int* __restrict__ sub_off, const double* __restrict__ tab,
                                                   const double* __restrict__ len, const DashFV* __restrict__ cum,
                                                   const DashCnt* __restrict__ cnt, const DashSub* __restrict__ sub, int n,
                                                   long long n_out, long long n_dash, int* __restrict__ out_types,
                                                   double* __restrict__ out_params, int* __restrict__ dstart, int* __restrict__ dkind,
                                                   int* __restrict__ bad) {
    __shared__ DashPat pat;
    for (int w = threadIdx.x; w < (int)(sizeof(DashPat) / 4); w += 256) ((int*)&pat)[w] = ((const int*)patp)[w];
    __syncthreads();
    const int l = threadIdx.x & 31, i = blockIdx.x * DASH_SEGS_WG + (threadIdx.x >> 5);
    if (i >= n) return;
    const DashSegIn s = dash_seg_in(pat, types, seg_sub, sub_off, len, cum, i);
    DashSeg g;
    dash_seg_pieces(pat, s.type, s.len, s.s0, s.s1, s.mode, g);
    if (g.cnt == 0) return;
    const DashSub sb = sub[seg_sub[i]];
    const long long poff = i ? cnt[i - 1].p : 0, doff = i ? cnt[i - 1].d : 0;
    long long k0 = 0;
    int j0 = 0;
    if (s.mode == DASH_MERGED) {
        double rr;
        dash_idx_ge(pat, pat.phase, k0, j0, rr);
    }
    const double* c = params + (size_t)i * 8;
    const double* tb = tab + (size_t)i * DASH_SUB;
    const double own_len = s.type == SVGR_PATH_CUBIC ? tb[DASH_SUB - 1] : s.len;
    for (long long q = l; q < g.cnt; q += 32) {
        long long k;
        int j;
        double o[8];
        const int ot = dash_piece(pat, g, s.type, c, tb, own_len, s.mode, q, k, j, o);
        long long place = poff + q, d = doff + q - (g.cont ? 1 : 0);
        if (s.mode == DASH_MERGED) {
            long long local = place - sb.A - sb.nl;
            if (local < 0) local += sb.n;
            place = sb.A + local;
            if (k == k0 && j == j0) d = sb.dbase + sb.nd - 1;   // the leading dash: part of the subpath's last one
        }
        const long long at = place + d;
        if (d < 0 || d >= n_dash || at < 0 || at >= n_out) {   // no place outside the arrays, whatever the tables say:
            *bad = 1;                                          // the host reports it
            continue;
        }
        if (q > 0 || !g.cont) {
            dstart[d] = (int)place;
            dkind[d] = s.mode == DASH_WHOLE ? SVGR_PATH_CLOSED : SVGR_PATH_UNCLOSED;
        }
        out_types[at] = ot;
        double* dst = out_params + (size_t)at * 8;
        for (int e = 0; e < 8; ++e) dst[e] = o[e];
    }
}

__global__ __launch_bounds__(256) void k_dash_close(const int* __restrict__ dstart, const int* __restrict__ dkind, long long n_pieces,
                                                    long long n_dash, int* __restrict__ out_types, double* __restrict__ out_params,
                                                    int* __restrict__ out_sizes, int* __restrict__ bad) {
    const long long d = (long long)blockIdx.x * 256 + threadIdx.x;
    if (d >= n_dash) return;
    const long long first = dstart[d] + d, end = (d + 1 < n_dash ? (long long)dstart[d + 1] : n_pieces) + d;
    if (first < 0 || end <= first || end >= n_pieces + n_dash) { out_sizes[d] = 0; *bad = 1; return; }
    const double* a = out_params + (size_t)first * 8;
    const double* b = out_params + (size_t)(end - 1) * 8;
    const int be = out_types[end - 1] == SVGR_PATH_CUBIC ? 6 : 2;
    double* o = out_params + (size_t)end * 8;
    o[0] = b[be]; o[1] = b[be + 1]; o[2] = a[0]; o[3] = a[1];
    o[4] = o[5] = o[6] = o[7] = 0.0;
    out_types[end] = dkind[d];
    out_sizes[d] = (int)(end - first + 1);
}

template <class T, class Op>
static void dash_scan(hipStream_t st, T* a, T* tot, int n) {
    const int nb = (n + DASH_S - 1) / DASH_S;
    SVGR_LAUNCH((k_scan_block<T, Op>), dim3((unsigned)nb), dim3(256), 0, st, a, tot, n);
    if (nb > 1) {
        SVGR_LAUNCH((k_scan_tops<T, Op>), dim3(1), dim3(256), 0, st, tot, nb);
        SVGR_LAUNCH((k_scan_apply<T, Op>), grid1((size_t)n), dim3(256), 0, st, a, (const T*)tot, n);
    }
}

// ---- what the passes over a path (dash, markers, text on a path) share: the check and the upload of the path
// the segment count of `n_subpaths` subpaths; the segment arrays may be null while there is no segment
static int path_count(const char* what, const int32_t* seg_types, const double* seg_params, const int32_t* subpath_sizes, int64_t n_subpaths,
                      int64_t& n) {
    n = 0;
    for (int64_t s = 0; s < n_subpaths; ++s) {
        if (subpath_sizes[s] < 0) return fail(SVGR_E_INVALID, "%s: negative subpath size", what);
        n += subpath_sizes[s];
        if (n > INT32_MAX / 2) return fail(SVGR_E_OVERFLOW, "%s: more than 2^30 segments", what);
    }
    if (n > 0 && (!seg_types || !seg_params)) return fail(SVGR_E_INVALID, "%s: bad arguments", what);
    return 0;
}
// types and coordinates of n segments in the stroker's array form
static int textpath_check_segments(const char* what, const int32_t* types, const double* params, int64_t n) {
    for (int64_t i = 0; i < n; ++i) {
        const int t = types[i];
        if (t != SVGR_PATH_LINE && t != SVGR_PATH_CUBIC && t != SVGR_PATH_CLOSED && t != SVGR_PATH_UNCLOSED)
            return fail(SVGR_E_INVALID, "%s: segment %lld has type %d (quadratics and arcs are converted by the caller)", what, (long long)i, t);
        const int np = t == SVGR_PATH_CUBIC ? 8 : 4;
        for (int e = 0; e < np; ++e)
            if (!(std::fabs(params[8 * i + e]) <= DASH_COORD_MAX))
                return fail(SVGR_E_INVALID, "%s: segment %lld has a coordinate that is not finite or beyond 1e150", what, (long long)i);
    }
    return 0;
}
// The head of the three uploads: coordinates, types, the subpath of every segment, the subpaths' first segments (empty
// subpaths are skipped).  The path has passed path_count.
struct PathSections {
    Section<double> params;
    Section<int32_t> types, seg_sub, sub_off;
    int n, n_sub;
};
static PathSections path_put(HostBlob& blob, const int32_t* seg_types, const double* seg_params, const int32_t* subpath_sizes, int64_t n_subpaths,
                             int64_t n) {
    std::vector<int32_t> sub_off{0};
    for (int64_t s = 0; s < n_subpaths; ++s)
        if (subpath_sizes[s] > 0) sub_off.push_back(sub_off.back() + subpath_sizes[s]);
    PathSections p;
    p.n = (int)n;
    p.n_sub = (int)sub_off.size() - 1;
    p.params = blob.put(seg_params, (size_t)n * 8);
    p.types = blob.put(seg_types, (size_t)n);
    int32_t* seg_sub;
    p.seg_sub = blob.reserve((size_t)n, seg_sub);
    for (int s = 0; seg_sub && s < p.n_sub; ++s)   // (null in HostBlob::build's sizing pass)
        for (int i = sub_off[(size_t)s]; i < sub_off[(size_t)s + 1]; ++i) seg_sub[i] = s;
    p.sub_off = blob.put(sub_off.data(), sub_off.size());
    return p;
}
// params and types of a result that is a path, from the downloaded block
static void stroke_out_take(svgr_stroke_out& res, const char* back, Section<double> params, Section<int32_t> types) {
    res.params.assign(params.on(back), params.on(back) + params.n);
    res.types.assign(types.on(back), types.on(back) + types.n);
}

static int path_dash_impl(svgr_ctx* ctx, const int32_t* seg_types, const double* seg_params, const int32_t* subpath_sizes,
                          int64_t n_subpaths, const double* dashes, int64_t n_dashes, double offset, double path_length,
                          svgr_stroke_out** out) {
    if (!out || n_subpaths < 0 || n_dashes < 0 || (n_subpaths > 0 && (!seg_types || !seg_params || !subpath_sizes)) || (n_dashes > 0 && !dashes))
        return fail(SVGR_E_INVALID, "svgr_path_dash: bad arguments");
    if (!std::isfinite(offset)) return fail(SVGR_E_INVALID, "svgr_path_dash: the offset is not finite");
    int64_t n = 0;
    if (int rc = path_count("svgr_path_dash", seg_types, seg_params, subpath_sizes, n_subpaths, n)) return rc;
    if (int rc = textpath_check_segments("svgr_path_dash", seg_types, seg_params, n)) return rc;
    std::unique_ptr<svgr_stroke_out> res(new svgr_stroke_out());
    // a pattern that asks for a solid stroke: the input comes back as it is
    bool solid = n_dashes < 1;
    double sum = 0.0;
    int gaps = 0;
    for (int64_t j = 0; j < n_dashes && !solid; ++j) {
        if (!std::isfinite(dashes[j]) || dashes[j] < 0.0) solid = true;
        else sum += dashes[j];
    }
    if (!solid) {
        const int64_t m = (n_dashes & 1) ? 2 * n_dashes : n_dashes;
        for (int64_t j = 0; j < m; ++j) gaps += (j & 1) && dashes[j % n_dashes] > 0.0;
        if (!(sum > 0.0) || !std::isfinite(sum) || gaps == 0) solid = true;
        else if (m > DASH_MAX) return fail(SVGR_E_INVALID, "svgr_path_dash: %lld dash entries (at most %d, counting an odd list twice)", (long long)m, DASH_MAX);
    }
    if (solid || n == 0) {
        res->types.assign(seg_types, seg_types + n);
        res->params.assign(seg_params, seg_params + 8 * n);
        for (int64_t s = 0; s < n_subpaths; ++s) res->sizes.push_back(subpath_sizes[s]);
        *out = res.release();
        return 0;
    }
    if (!ctx) return fail(SVGR_E_INVALID, "svgr_path_dash: no context");
    // ---- one upload: the path, the dash list
    PassFrame f(ctx);
    hipStream_t st = f.st;
    PathSections path;
    Section<double> raw;
    f.blob.build([&](HostBlob& b) {
        path = path_put(b, seg_types, seg_params, subpath_sizes, n_subpaths, n);
        raw = b.put(dashes, (size_t)n_dashes);
    });
    const int n_sub = path.n_sub, ni = path.n, nd_raw = (int)n_dashes;
    if (int rc = f.upload()) return rc;
    if (int rc = ensure_pinned(ctx, sizeof(DashTot))) return rc;
    const int nb = (ni + DASH_S - 1) / DASH_S;
    double *tab = f.scratch<double>((size_t)n * DASH_SUB), *len = f.scratch<double>((size_t)n);
    DashFV *cum = f.scratch<DashFV>((size_t)n), *tops_fv = f.scratch<DashFV>((size_t)nb);
    DashCnt *cnt = f.scratch<DashCnt>((size_t)n), *tops_cnt = f.scratch<DashCnt>((size_t)nb);
    DashSub* sub = f.scratch<DashSub>((size_t)n_sub);
    DashPat* pat = f.scratch<DashPat>(1);
    DashTot* tot = f.scratch<DashTot>(1);
    if (f.err) return f.err;
    HIPCHK(hipMemsetAsync(tot, 0, sizeof(DashTot), st));
    const double* d_params = path.params.on(f.in.p);
    const int* d_types = path.types.on(f.in.p);
    const int* d_seg_sub = path.seg_sub.on(f.in.p);
    const int* d_sub_off = path.sub_off.on(f.in.p);
    const dim3 seg_grid((unsigned)((ni + DASH_SEGS_WG - 1) / DASH_SEGS_WG));
    SVGR_LAUNCH(k_dash_measure, seg_grid, dim3(256), 0, st, d_types, d_params, d_seg_sub, d_sub_off, ni, tab, len, cum);
    dash_scan<DashFV, DashFVOp>(st, cum, tops_fv, ni);
    SVGR_LAUNCH(k_dash_pattern, dim3(1), dim3(256), 0, st, cum, d_sub_off, n_sub, raw.on(f.in.p), nd_raw, offset, path_length, pat);
    SVGR_LAUNCH(k_dash_count, grid1((size_t)ni), dim3(256), 0, st, pat, d_types, d_seg_sub, d_sub_off, len, cum, ni, cnt, tot);
    dash_scan<DashCnt, DashCntOp>(st, cnt, tops_cnt, ni);
    SVGR_LAUNCH(k_dash_wrap, grid1((size_t)n_sub), dim3(256), 0, st, pat, d_types, d_sub_off, cum, cnt, ni, n_sub, sub, tot);
    HIPCHK(hipGetLastError());
    // ---- the counts come back through the context's page-locked staging
    HIPCHK(hipMemcpyAsync(ctx->pinned, tot, sizeof(DashTot), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    DashTot counted;
    memcpy(&counted, ctx->pinned, sizeof counted);
    const DashCnt total = counted.c;
    if (counted.too_many)
        return fail(SVGR_E_OVERFLOW, "svgr_path_dash: a segment with more than %lld pieces", DASH_SEG_PIECES_MAX);
    if (total.p < 0 || total.d < 0 || total.p + total.d > INT32_MAX)
        return fail(SVGR_E_OVERFLOW, "svgr_path_dash: %lld pieces in %lld dashes do not fit the 32-bit counts of the result", total.p, total.d);
    if (total.p == 0 || total.d == 0) {   // nothing is drawn
        *out = res.release();
        return 0;
    }
    // ---- the second phase: now that its size is known, the result (the placing kernels' error flag travels with it)
    const size_t n_out = (size_t)(total.p + total.d), n_dash = (size_t)total.d;
    Layout lay;
    const Section<double> o_params = lay.take<double>(n_out * 8);
    const Section<int32_t> o_types = lay.take<int32_t>(n_out), o_sizes = lay.take<int32_t>(n_dash);
    if (int rc = f.result(lay)) return rc;
    int *dstart = f.scratch<int>(n_dash), *dkind = f.scratch<int>(n_dash);
    if (f.err) return f.err;
    double* d_out_params = o_params.on(f.out.p);
    int* d_out_types = o_types.on(f.out.p);
    int* d_bad = f.bad.on(f.out.p);
    SVGR_LAUNCH(k_dash_emit, seg_grid, dim3(256), 0, st, pat, d_types, d_params, d_seg_sub, d_sub_off, tab, len, cum, cnt, sub, ni,
                (long long)n_out, (long long)n_dash, d_out_types, d_out_params, dstart, dkind, d_bad);
    SVGR_LAUNCH(k_dash_close, grid1(n_dash), dim3(256), 0, st, dstart, dkind, total.p, total.d, d_out_types, d_out_params, o_sizes.on(f.out.p),
                d_bad);
    if (int rc = f.finish("svgr_path_dash", "the counting and the placing kernels disagree about a place")) return rc;
    stroke_out_take(*res, f.back.data(), o_params, o_types);
    res->sizes.assign(o_sizes.on(f.back.data()), o_sizes.on(f.back.data()) + n_dash);
    *out = res.release();
    return 0;
}

extern "C" {
int svgr_dash_scan_segments(void) { return DASH_S; }
int svgr_path_dash(svgr_ctx* ctx, const int32_t* seg_types, const double* seg_params, const int32_t* subpath_sizes, int64_t n_subpaths,
                   const double* dashes, int64_t n_dashes, double offset, double path_length, svgr_stroke_out** out) {
    return abi_guard("svgr_path_dash", [&]() {
        return path_dash_impl(ctx, seg_types, seg_params, subpath_sizes, n_subpaths, dashes, n_dashes, offset, path_length, out);
    });
}
}  // extern "C"

// ======================================================================================
// Path.vertices: the vertices of a path with their directions, for marker-start / -mid / -end (svgr_path_markers).
// The per-lane arithmetic is svgr_marker.h; DESIGN.md "Markers" has the definitions.
//
//   k_marker_classify   one lane per segment: its 64-byte record in two loads, its two unit directions, its flags, its row of counts
//   k_scan_*            the dasher's two-level sum scan (DASH_S segments per workgroup) over (segments with a direction, vertices):
//                       a segment's place in the compacted table and every vertex's slot
//   k_marker_table      one lane per segment: a segment with a direction enters the compacted table at its count
//   k_marker_emit       one lane per segment: the vertices it owns (the first of its subpath, its end point); a degenerate segment
//                       finds its neighbours' directions through the table, backwards and forwards, within its subpath
// Every slot is a prefix sum; no atomic takes part.  All geometry is f64.
// ======================================================================================
#include "svgr_marker.h"

constexpr int MARKER_B = 256;   // segments (= lanes) per workgroup of the classify / table / emit kernels
// The tile kernel's cold paths live in subsection 1 of .text, behind every kernel of this file, and its branches to them reach
// 2^15 instructions: what is added to .text behind the tile kernel lengthens them.  These kernels go into a section of their own.
#define MARKER_KERNEL __global__ __launch_bounds__(MARKER_B) __attribute__((section(".text.svgr_marker")))

struct svgr_marker_out {
    std::vector<double> xyuv;    // 4 per vertex: x, y, ux, uy
    std::vector<int32_t> kind;   // MARKER_START / _MID / _END
};
struct MarkerCntOp {
    __device__ static MarkerCnt zero() { return MarkerCnt{0, 0}; }
    __device__ static MarkerCnt add(const MarkerCnt& a, const MarkerCnt& b) { return MarkerCnt{a.nd + b.nd, a.v + b.v}; }
};

MARKER_KERNEL void k_marker_classify(const int* __restrict__ types, const double* __restrict__ params,
                                                              const int* __restrict__ seg_sub, const int* __restrict__ sub_off,
                                                              const int* __restrict__ seg_vertex, int n, int* __restrict__ flags,
                                                              MarkerDirs* __restrict__ dirs, MarkerCnt* __restrict__ cnt) {
    const int i = blockIdx.x * MARKER_B + threadIdx.x;
    if (i >= n) return;
    const double4* rec = reinterpret_cast<const double4*>(params) + (size_t)i * 2;
    const double4 lo = rec[0], hi = rec[1];
    const double c[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    MarkerDirs d{0.0, 0.0, 0.0, 0.0};
    MarkerCnt row;
    flags[i] = marker_classify(types, seg_sub, sub_off, seg_vertex, i, c, d, row);
    marker_store2(&dirs[i].sx, d.sx, d.sy);
    marker_store2(&dirs[i].ex, d.ex, d.ey);
    cnt[i] = row;
}

// (cnt: the inclusive scan of k_marker_classify's rows)
MARKER_KERNEL void k_marker_table(const int* __restrict__ flags, const MarkerCnt* __restrict__ cnt, int n,
                                                           int* __restrict__ tab, int* __restrict__ bad) {
    const int i = blockIdx.x * MARKER_B + threadIdx.x;
    if (i >= n || !(flags[i] & MARKER_F_DIR)) return;
    const long long k = cnt[i].nd - 1;
    if (k < 0 || k >= n) { *bad = 1; return; }   // (the host zeroed it; every writer stores the same value)
    tab[k] = i;
}

MARKER_KERNEL void k_marker_emit(MarkerView v, long long n_vert, double* __restrict__ xyuv, int* __restrict__ kind,
                                                          int* __restrict__ bad) {
    const int i = blockIdx.x * MARKER_B + threadIdx.x;
    if (i >= v.n) return;
    if (!marker_emit(v, i, n_vert, xyuv, kind)) *bad = 1;
}

static int path_markers_impl(svgr_ctx* ctx, const int32_t* seg_types, const double* seg_params, const int32_t* seg_vertex,
                             const int32_t* subpath_sizes, int64_t n_subpaths, svgr_marker_out** out) {
    if (!out || n_subpaths < 0 || (n_subpaths > 0 && !subpath_sizes))
        return fail(SVGR_E_INVALID, "svgr_path_markers: bad arguments");
    int64_t n = 0;
    if (int rc = path_count("svgr_path_markers", seg_types, seg_params, subpath_sizes, n_subpaths, n)) return rc;
    if (int rc = textpath_check_segments("svgr_path_markers", seg_types, seg_params, n)) return rc;
    // the vertex count is a matter of types and flags alone: known before anything is launched
    int64_t n_vert = 0;
    for (int64_t s = 0, at = 0; s < n_subpaths; at += subpath_sizes[s], ++s) {
        if (subpath_sizes[s] == 0) continue;
        const int64_t end = at + subpath_sizes[s] - (seg_types[at + subpath_sizes[s] - 1] == SVGR_PATH_UNCLOSED ? 1 : 0);
        if (end == at) continue;
        n_vert += 1;
        if (!seg_vertex) n_vert += end - at;
        else for (int64_t i = at; i < end; ++i) n_vert += seg_vertex[i] != 0;
    }
    if (n_vert > INT32_MAX) return fail(SVGR_E_OVERFLOW, "svgr_path_markers: %lld vertices do not fit a 32-bit count", (long long)n_vert);
    std::unique_ptr<svgr_marker_out> res(new svgr_marker_out());
    if (n == 0 || n_vert == 0) {
        *out = res.release();
        return 0;
    }
    if (!ctx) return fail(SVGR_E_INVALID, "svgr_path_markers: no context");
    // ---- one upload: the path, the vertex flags
    PassFrame f(ctx);
    hipStream_t st = f.st;
    PathSections path;
    Section<int32_t> vertex;
    f.blob.build([&](HostBlob& b) {
        path = path_put(b, seg_types, seg_params, subpath_sizes, n_subpaths, n);
        if (seg_vertex) vertex = b.put(seg_vertex, (size_t)n);
    });
    const int ni = path.n, nb = (ni + DASH_S - 1) / DASH_S;
    Layout lay;
    const Section<double> o_xyuv = lay.take<double>((size_t)n_vert * 4);
    const Section<int32_t> o_kind = lay.take<int32_t>((size_t)n_vert);
    if (int rc = f.begin(lay)) return rc;
    int *flags = f.scratch<int>((size_t)n), *tab = f.scratch<int>((size_t)n);
    MarkerDirs* dirs = f.scratch<MarkerDirs>((size_t)n);
    MarkerCnt *cnt = f.scratch<MarkerCnt>((size_t)n), *tops = f.scratch<MarkerCnt>((size_t)nb);
    if (f.err) return f.err;
    const double* d_params = path.params.on(f.in.p);
    const int* d_types = path.types.on(f.in.p);
    const int* d_seg_sub = path.seg_sub.on(f.in.p);
    const int* d_sub_off = path.sub_off.on(f.in.p);
    const int* d_vertex = seg_vertex ? vertex.on(f.in.p) : nullptr;
    int* d_bad = f.bad.on(f.out.p);
    const dim3 grid = grid1((size_t)ni, MARKER_B);
    SVGR_LAUNCH(k_marker_classify, grid, dim3(MARKER_B), 0, st, d_types, d_params, d_seg_sub, d_sub_off, d_vertex, ni, flags, dirs, cnt);
    dash_scan<MarkerCnt, MarkerCntOp>(st, cnt, tops, ni);
    SVGR_LAUNCH(k_marker_table, grid, dim3(MARKER_B), 0, st, flags, cnt, ni, tab, d_bad);
    const MarkerView view{d_types, d_params, d_seg_sub, d_sub_off, flags, dirs, cnt, tab, ni};
    SVGR_LAUNCH(k_marker_emit, grid, dim3(MARKER_B), 0, st, view, (long long)n_vert, o_xyuv.on(f.out.p), o_kind.on(f.out.p), d_bad);
    if (int rc = f.finish("svgr_path_markers", "the counting and the placing kernels disagree about a place")) return rc;
    res->xyuv.assign(o_xyuv.on(f.back.data()), o_xyuv.on(f.back.data()) + o_xyuv.n);
    res->kind.assign(o_kind.on(f.back.data()), o_kind.on(f.back.data()) + o_kind.n);
    *out = res.release();
    return 0;
}

extern "C" {
int svgr_marker_block_segments(void) { return MARKER_B; }
int svgr_path_markers(svgr_ctx* ctx, const int32_t* seg_types, const double* seg_params, const int32_t* seg_vertex,
                      const int32_t* subpath_sizes, int64_t n_subpaths, svgr_marker_out** out) {
    return abi_guard("svgr_path_markers", [&]() {
        return path_markers_impl(ctx, seg_types, seg_params, seg_vertex, subpath_sizes, n_subpaths, out);
    });
}
int svgr_marker_out_counts(const svgr_marker_out* m, int64_t* n_vertices) {
    if (!m) return SVGR_E_INVALID;
    if (n_vertices) *n_vertices = (int64_t)m->kind.size();
    return SVGR_OK;
}
int svgr_marker_out_copy(const svgr_marker_out* m, double* xyuv, int32_t* kind) {
    if (!m) return SVGR_E_INVALID;
    if (xyuv && !m->xyuv.empty()) memcpy(xyuv, m->xyuv.data(), sizeof(double) * m->xyuv.size());
    if (kind && !m->kind.empty()) memcpy(kind, m->kind.data(), sizeof(int32_t) * m->kind.size());
    return SVGR_OK;
}
void svgr_marker_out_free(svgr_marker_out* m) { delete m; }
}  // extern "C"

// ======================================================================================
// Text on a path: the frame of a path at an arc length (svgr_path_sample) and glyph outlines placed in such frames
// (svgr_path_place_glyphs).  The per-lane arithmetic is svgr_textpath.h; DESIGN.md "Text on a path" has the definitions.
//
//   k_dash_measure      the dasher's: per-segment lengths and the cubics' tables
//   k_scan_*            the dasher's two-level sum scan (DASH_S segments per workgroup) over the lengths of the whole path -- no
//                       restart at a subpath: inc[i], the length up to and with segment i
//   k_textpath_locate   one lane per query: binary search in inc, then the frame (x, y, ux, uy) and the inside flag
//   k_textpath_emit     one lane per output segment: its instance by binary search in the host-built prefix sums of the instances'
//                       segment counts, the instance's frame, its 64-byte atlas record in two loads, 8 transformed doubles
// Every slot is known to the host before the launch; no atomic takes part.  All geometry is f64.
// ======================================================================================
#include "svgr_textpath.h"

constexpr int TEXTPATH_B = 256;   // queries / output segments (= lanes) per workgroup
// (a section of its own, like the marker kernels': the tile kernel's branches to its cold paths keep their reach)
#define TEXTPATH_KERNEL __global__ __launch_bounds__(TEXTPATH_B) __attribute__((section(".text.svgr_textpath")))

struct TextLenOp {
    __device__ static double zero() { return 0.0; }
    __device__ static double add(const double& a, const double& b) { return a + b; }
};

TEXTPATH_KERNEL void k_textpath_locate(TextPathView v, const double* __restrict__ s, int nq, double* __restrict__ xyuv,
                                       int* __restrict__ inside) {
    const int q = blockIdx.x * TEXTPATH_B + threadIdx.x;
    if (q >= nq) return;
    TextFrame f;
    inside[q] = textpath_locate(v, s[q], f);
    marker_store2(xyuv + (size_t)q * 4, f.x, f.y);
    marker_store2(xyuv + (size_t)q * 4 + 2, f.ux, f.uy);
}

TEXTPATH_KERNEL void k_textpath_emit(TextEmitView v, int n_out, double* __restrict__ out, int* __restrict__ bad) {
    const int j = blockIdx.x * TEXTPATH_B + threadIdx.x;
    if (j >= n_out) return;
    if (!textpath_emit(v, j, out + (size_t)j * 8)) *bad = 1;   // (the host zeroed it; every writer stores the same value)
}

struct TextPlaceIn {   // the glyph side of svgr_path_place_glyphs
    const int32_t* atlas_types;
    const double* atlas_params;
    const int32_t* glyph_seg_off;
    int64_t n_glyphs;
    const int32_t* inst_glyph;
    const double *inst_half, *inst_dy;
};

// Both entries: the frames of `nq` arc lengths `s`; with `pl`, the queries are the instances' anchors and their outlines follow.
static int textpath_impl(const char* what, svgr_ctx* ctx, const int32_t* seg_types, const double* seg_params, const int32_t* subpath_sizes,
                         int64_t n_subpaths, const double* s, int64_t nq, const TextPlaceIn* pl, double* xyuv_out, int32_t* flag_out,
                         double* params_out, double* total_length_out) {
    if (n_subpaths < 0 || nq < 0 || (n_subpaths > 0 && !subpath_sizes) || (nq > 0 && (!s || !flag_out || (!pl && !xyuv_out))))
        return fail(SVGR_E_INVALID, "%s: bad arguments", what);
    int64_t n = 0;
    if (int rc = path_count(what, seg_types, seg_params, subpath_sizes, n_subpaths, n)) return rc;
    if (nq > INT32_MAX / 2) return fail(SVGR_E_OVERFLOW, "%s: %lld queries do not fit a 32-bit count", what, (long long)nq);
    if (int rc = textpath_check_segments(what, seg_types, seg_params, n)) return rc;
    for (int64_t q = 0; q < nq; ++q)
        if (!std::isfinite(s[q])) return fail(SVGR_E_INVALID, "%s: arc length %lld is not finite", what, (long long)q);
    // ---- the glyph side: every output slot is a matter of the segment counts alone, known before anything is launched
    std::vector<int32_t> inst_off;
    int64_t n_out = 0, n_atlas = 0;
    if (pl) {
        if (pl->n_glyphs < 0 || pl->n_glyphs > INT32_MAX / 2 || !pl->glyph_seg_off || (nq > 0 && (!pl->inst_glyph || !pl->inst_half || !pl->inst_dy)))
            return fail(SVGR_E_INVALID, "%s: bad arguments", what);
        if (pl->glyph_seg_off[0] != 0) return fail(SVGR_E_INVALID, "%s: the glyph offsets do not begin at 0", what);
        for (int64_t g = 0; g < pl->n_glyphs; ++g)
            if (pl->glyph_seg_off[g + 1] < pl->glyph_seg_off[g]) return fail(SVGR_E_INVALID, "%s: the glyph offsets decrease at glyph %lld", what, (long long)g);
        n_atlas = pl->glyph_seg_off[pl->n_glyphs];
        if (n_atlas > 0 && (!pl->atlas_types || !pl->atlas_params)) return fail(SVGR_E_INVALID, "%s: bad arguments", what);
        if (int rc = textpath_check_segments(what, pl->atlas_types, pl->atlas_params, n_atlas)) return rc;
        inst_off.assign((size_t)nq + 1, 0);
        for (int64_t k = 0; k < nq; ++k) {
            const int64_t g = pl->inst_glyph[k];
            if (g < 0 || g >= pl->n_glyphs) return fail(SVGR_E_INVALID, "%s: instance %lld names glyph %lld of %lld", what, (long long)k, (long long)g, (long long)pl->n_glyphs);
            if (!std::isfinite(pl->inst_half[k]) || !std::isfinite(pl->inst_dy[k]))
                return fail(SVGR_E_INVALID, "%s: instance %lld has an advance or a shift that is not finite", what, (long long)k);
            n_out += pl->glyph_seg_off[g + 1] - pl->glyph_seg_off[g];
            if (n_out > INT32_MAX / 2) return fail(SVGR_E_OVERFLOW, "%s: the placed outlines do not fit a 32-bit count of segments", what);
            inst_off[(size_t)k + 1] = (int32_t)n_out;
        }
        if (n_out > 0 && !params_out) return fail(SVGR_E_INVALID, "%s: bad arguments", what);
    }
    if (total_length_out) *total_length_out = 0.0;
    if (nq > 0) {
        memset(flag_out, 0, (size_t)nq * 4);
        if (xyuv_out) memset(xyuv_out, 0, (size_t)nq * 32);
    }
    if (n_out > 0) memset(params_out, 0, (size_t)n_out * 64);
    if (n == 0) return 0;   // a path without segments: L = 0, nothing is inside, nothing is launched
    if (!ctx) return fail(SVGR_E_INVALID, "%s: no context", what);
    // ---- one upload: the path, the queries, and the glyph side (atlas, offsets, instances)
    PassFrame f(ctx);
    hipStream_t st = f.st;
    PathSections path;
    Section<double> q_s, atlas, half, dy;
    Section<int32_t> atypes, goff, iglyph, ioff;
    f.blob.build([&](HostBlob& b) {
        path = path_put(b, seg_types, seg_params, subpath_sizes, n_subpaths, n);
        q_s = b.put(s, (size_t)nq);
        if (!pl) return;
        atlas = b.put(pl->atlas_params, (size_t)n_atlas * 8), atypes = b.put(pl->atlas_types, (size_t)n_atlas);
        goff = b.put(pl->glyph_seg_off, (size_t)pl->n_glyphs + 1), iglyph = b.put(pl->inst_glyph, (size_t)nq);
        ioff = b.put(inst_off.data(), inst_off.size()), half = b.put(pl->inst_half, (size_t)nq), dy = b.put(pl->inst_dy, (size_t)nq);
    });
    const int ni = path.n, nqi = (int)nq, n_outi = (int)n_out, nb = (ni + DASH_S - 1) / DASH_S;
    // the result block: placed outlines, frames, flags, the total length
    Layout lay;
    const Section<double> o_params = lay.take<double>((size_t)n_out * 8), o_frames = lay.take<double>((size_t)nq * 4);
    const Section<int32_t> o_flag = lay.take<int32_t>((size_t)nq);
    const Section<double> o_len = lay.take<double>(1);
    if (int rc = f.begin(lay)) return rc;
    double *tab = f.scratch<double>((size_t)n * DASH_SUB), *len = f.scratch<double>((size_t)n), *inc = f.scratch<double>((size_t)n);
    double* tops = f.scratch<double>((size_t)nb);
    DashFV* cum = f.scratch<DashFV>((size_t)n);
    if (f.err) return f.err;
    const void* d_in = f.in.p;
    const double* d_params = path.params.on(d_in);
    const int* d_types = path.types.on(d_in);
    double* d_frames = o_frames.on(f.out.p);
    int* d_flag = o_flag.on(f.out.p);
    const dim3 seg_grid((unsigned)((ni + DASH_SEGS_WG - 1) / DASH_SEGS_WG));
    SVGR_LAUNCH(k_dash_measure, seg_grid, dim3(256), 0, st, d_types, d_params, path.seg_sub.on(d_in), path.sub_off.on(d_in), ni, tab, len, cum);
    HIPCHK(hipMemcpyAsync(inc, len, (size_t)n * 8, hipMemcpyDeviceToDevice, st));
    dash_scan<double, TextLenOp>(st, inc, tops, ni);
    HIPCHK(hipMemcpyAsync(o_len.on(f.out.p), inc + (ni - 1), 8, hipMemcpyDeviceToDevice, st));
    if (nqi > 0) {
        const TextPathView view{d_types, d_params, len, tab, inc, ni};
        SVGR_LAUNCH(k_textpath_locate, grid1((size_t)nqi, TEXTPATH_B), dim3(TEXTPATH_B), 0, st, view, q_s.on(d_in), nqi, d_frames, d_flag);
    }
    if (n_outi > 0) {
        const TextEmitView ev{atypes.on(d_in), atlas.on(d_in), goff.on(d_in), iglyph.on(d_in), ioff.on(d_in), half.on(d_in), dy.on(d_in),
                              d_frames,        d_flag,         nqi,           (int)n_atlas};
        SVGR_LAUNCH(k_textpath_emit, grid1((size_t)n_outi, TEXTPATH_B), dim3(TEXTPATH_B), 0, st, ev, n_outi, o_params.on(f.out.p), f.bad.on(f.out.p));
    }
    if (int rc = f.finish(what, "a lane met a slot outside the result")) return rc;
    const char* back = f.back.data();
    if (total_length_out) *total_length_out = *o_len.on(back);
    if (n_out > 0) memcpy(params_out, o_params.on(back), (size_t)n_out * 64);
    if (nq > 0) {
        if (xyuv_out) memcpy(xyuv_out, o_frames.on(back), (size_t)nq * 32);
        memcpy(flag_out, o_flag.on(back), (size_t)nq * 4);
    }
    return 0;
}

extern "C" {
int svgr_textpath_block(void) { return TEXTPATH_B; }
int svgr_path_sample(svgr_ctx* ctx, const int32_t* seg_types, const double* seg_params, const int32_t* subpath_sizes, int64_t n_subpaths,
                     const double* s, int64_t n, double* xyuv_out, int32_t* inside_out, double* total_length_out) {
    return abi_guard("svgr_path_sample", [&]() {
        return textpath_impl("svgr_path_sample", ctx, seg_types, seg_params, subpath_sizes, n_subpaths, s, n, nullptr, xyuv_out, inside_out,
                             nullptr, total_length_out);
    });
}
int svgr_path_place_glyphs(svgr_ctx* ctx, const int32_t* seg_types, const double* seg_params, const int32_t* subpath_sizes, int64_t n_subpaths,
                           const int32_t* atlas_types, const double* atlas_params, const int32_t* glyph_seg_off, int64_t n_glyphs,
                           const int32_t* inst_glyph, const double* inst_s_mid, const double* inst_half, const double* inst_dy, int64_t n_inst,
                           double* params_out, int32_t* visible_out, double* total_length_out) {
    return abi_guard("svgr_path_place_glyphs", [&]() {
        const TextPlaceIn pl{atlas_types, atlas_params, glyph_seg_off, n_glyphs, inst_glyph, inst_half, inst_dy};
        return textpath_impl("svgr_path_place_glyphs", ctx, seg_types, seg_params, subpath_sizes, n_subpaths, inst_s_mid, n_inst, &pl, nullptr,
                             visible_out, params_out, total_length_out);
    });
}
}  // extern "C"

// ======================================================================================
// TrueType outlines: the contours of simple glyphs (`glyf`) as the lines and cubics of a path (svgr_glyf_outline).  The
// per-lane arithmetic and the host's validation walk are svgr_glyf.h; DESIGN.md "TrueType fonts" has the definitions.
//
//   k_glyf_emit   one lane per (part, atlas point) pair: its part by binary search in the host-built prefix sums of the parts'
//                 point counts, its contour by binary search in the contour offsets, three int16 points and their flags, at most
//                 one segment (type + 8 doubles) and, for a contour's last point, the closing line
//   k_gvar_delta  (svgr_glyf_outline_var, svgr_gvar_deltas; svgr_gvar.h, DESIGN.md "Variable fonts") one lane per atlas point: its
//                 contour and glyph by binary search, then per tuple of the glyph three binary searches in the tuple's sorted point
//                 indices and the stored or interpolated delta; one pair of doubles per point, which k_glyf_emit then adds to the
//                 int16 point it reads
// Every slot is a glyph constant the host made while it checked the input; stores are disjoint and no atomic takes part (the
// `bad` flag is a plain store of the same value by every writer).  No LDS.  All geometry is f64.
// ======================================================================================
#include "svgr_glyf.h"
#include "svgr_gvar.h"

constexpr int GLYF_B = 256;   // (part, point) pairs (= lanes) per workgroup
// (a section of its own, like the marker kernels': the tile kernel's branches to its cold paths keep their reach)
#define GLYF_KERNEL __global__ __launch_bounds__(GLYF_B) __attribute__((section(".text.svgr_glyf")))

GLYF_KERNEL void k_glyf_emit(GlyfView v, int n_lanes, int* __restrict__ types, double* __restrict__ params, int* __restrict__ bad) {
    const int j = blockIdx.x * GLYF_B + threadIdx.x;
    if (j >= n_lanes) return;
    if (!glyf_emit(v, j, types, params)) *bad = 1;   // (the host zeroed it; every writer stores the same value)
}

// The tuples of a variable font's instance, as svgr_glyf_outline_var and svgr_gvar_deltas take them (svgr_gvar.h).
struct GvarIn {
    const int32_t* glyph_tuple_off;
    const double* tuple_scalar;
    int64_t n_tuples;
    const int32_t* tuple_pt_off;
    const int32_t* tp_index;
    const int16_t* tp_dxy;
    int64_t n_entries;
};

// Where the tuple arrays lie in an upload, and the delta pass's view of it.
struct GvarSections {
    Section<int32_t> toff, poff, index;
    Section<double> scalar;
    Section<int16_t> dxy;
    GvarView view(const void* d_in, const int16_t* pt_xy, const int* contour_off, const int* glyph_contour_off, int nc, int ng, int npt) const {
        return GvarView{pt_xy, contour_off, glyph_contour_off, toff.on(d_in), scalar.on(d_in), poff.on(d_in), index.on(d_in), dxy.on(d_in),
                        nc,    ng,          npt,               (int)scalar.n};
    }
};
static GvarSections gvar_put(HostBlob& blob, const GvarIn& g, int64_t n_glyphs) {
    GvarSections v;
    v.toff = blob.put(g.glyph_tuple_off, (size_t)n_glyphs + 1);
    v.scalar = blob.put(g.tuple_scalar, (size_t)g.n_tuples);
    v.poff = blob.put(g.tuple_pt_off, (size_t)g.n_tuples + 1);
    v.index = blob.put(g.tp_index, (size_t)g.n_entries);
    v.dxy = blob.put(g.tp_dxy, (size_t)g.n_entries * 2);
    return v;
}

constexpr int GVAR_B = 256;   // atlas points (= lanes) per workgroup

// One lane per atlas point: its delta at the instance, summed over its glyph's tuples (gvar_delta), stored as one pair.
__global__ __launch_bounds__(GVAR_B) __attribute__((section(".text.svgr_glyf")))
void k_gvar_delta(GvarView v, double* __restrict__ pt_dxy, int* __restrict__ bad) {
    const int a = blockIdx.x * GVAR_B + threadIdx.x;
    if (a >= v.n_points) return;
    double dx, dy;
    if (!gvar_delta(v, a, dx, dy)) *bad = 1;   // (the host zeroed it; every writer stores the same value)
    marker_store2(pt_dxy + 2 * (size_t)a, dx, dy);
}

// svgr_glyf_outline (gv null) and svgr_glyf_outline_var: with tuples, k_gvar_delta runs in front of k_glyf_emit on the same
// stream and the deltas stay on the device.
static int glyf_outline_impl(const char* name, svgr_ctx* ctx, const int16_t* pt_xy, const uint8_t* pt_on, int64_t n_points,
                             const int32_t* contour_off, int64_t n_contours, const int32_t* glyph_contour_off, int64_t n_glyphs,
                             const int32_t* part_glyph, const double* part_m, const double* part_pen, const double* part_sx,
                             const double* part_sy, int64_t n_parts, const GvarIn* gv, svgr_stroke_out** out) {
    if (!out || (n_points > 0 && !pt_xy)) return fail(SVGR_E_INVALID, "%s: bad arguments", name);
    GlyfTables t;
    if (int rc = glyf_tables(pt_on, n_points, contour_off, n_contours, glyph_contour_off, n_glyphs, part_glyph, part_m, part_pen, part_sx,
                             part_sy, n_parts, t))
        return fail(rc, "%s: %s", name, t.why);
    if (gv) {
        const char* why = "";
        if (int rc = gvar_tables(n_points, contour_off, n_contours, glyph_contour_off, n_glyphs, gv->glyph_tuple_off, gv->tuple_scalar,
                                 gv->n_tuples, gv->tuple_pt_off, gv->tp_index, gv->tp_dxy, gv->n_entries, why))
            return fail(rc, "%s: %s", name, why);
        if (gv->n_tuples == 0) gv = nullptr;   // (no tuple: the default instance, svgr_glyf_outline's own launch)
    }
    std::unique_ptr<svgr_stroke_out> res(new svgr_stroke_out());
    const int n_lanes = t.part_lane_off[(size_t)n_parts], n_out = t.part_seg_off[(size_t)n_parts];
    if (n_lanes == 0 || n_out == 0) {   // no part, parts of empty glyphs, or contours of a single point only
        *out = res.release();
        return 0;
    }
    if (!ctx) return fail(SVGR_E_INVALID, "%s: no context", name);
    // ---- one upload: the atlas with its slot table, the parts with their prefix sums, the tuples
    const int np = (int)n_parts, npt = (int)n_points, nc = (int)n_contours, ng = (int)n_glyphs;
    PassFrame f(ctx);
    Section<int16_t> xy;
    Section<uint8_t> on;
    Section<int32_t> slot, coff, goff, pglyph, plane, pseg;
    Section<double> m, pen, sx, sy;
    GvarSections gs;
    f.blob.build([&](HostBlob& b) {
        xy = b.put(pt_xy, (size_t)npt * 2), on = b.put(pt_on, (size_t)npt), slot = b.put(t.pt_slot.data(), (size_t)npt);
        coff = b.put(contour_off, (size_t)nc + 1), goff = b.put(glyph_contour_off, (size_t)ng + 1), pglyph = b.put(part_glyph, (size_t)np);
        plane = b.put(t.part_lane_off.data(), (size_t)np + 1), pseg = b.put(t.part_seg_off.data(), (size_t)np + 1);
        m = b.put(part_m, (size_t)np * 6), pen = b.put(part_pen, (size_t)np), sx = b.put(part_sx, (size_t)np), sy = b.put(part_sy, (size_t)np);
        if (gv) gs = gvar_put(b, *gv, n_glyphs);
    });
    // the result block: params, types; behind what is downloaded, the deltas (they stay on the device)
    Layout lay;
    const Section<double> o_params = lay.take<double>((size_t)n_out * 8);
    const Section<int32_t> o_types = lay.take<int32_t>((size_t)n_out);
    if (int rc = f.begin(lay, gv ? pad64((size_t)npt * 16) : 0)) return rc;
    const void* d_in = f.in.p;
    int* d_bad = f.bad.on(f.out.p);
    double* d_dxy = gv ? f.behind<double>() : nullptr;
    if (gv) {
        SVGR_LAUNCH(k_gvar_delta, grid1((size_t)npt, GVAR_B), dim3(GVAR_B), 0, f.st, gs.view(d_in, xy.on(d_in), coff.on(d_in), goff.on(d_in), nc, ng, npt),
                    d_dxy, d_bad);
        HIPCHK(hipGetLastError());
    }
    const GlyfView view{xy.on(d_in),  on.on(d_in), slot.on(d_in), coff.on(d_in), goff.on(d_in), pglyph.on(d_in), plane.on(d_in), pseg.on(d_in),
                        m.on(d_in),   pen.on(d_in), sx.on(d_in),  sy.on(d_in),   nc,            np,              npt,            n_out,
                        d_dxy};
    SVGR_LAUNCH(k_glyf_emit, grid1((size_t)n_lanes, GLYF_B), dim3(GLYF_B), 0, f.st, view, n_lanes, o_types.on(f.out.p), o_params.on(f.out.p), d_bad);
    if (int rc = f.finish(name, "a lane met a slot outside the result")) return rc;
    stroke_out_take(*res, f.back.data(), o_params, o_types);
    res->sizes = std::move(t.sizes);
    *out = res.release();
    return 0;
}

// svgr_gvar_deltas: the deltas alone.
static int gvar_deltas_impl(svgr_ctx* ctx, const int16_t* pt_xy, int64_t n_points, const int32_t* contour_off, int64_t n_contours,
                            const int32_t* glyph_contour_off, int64_t n_glyphs, const GvarIn& gv, double* pt_dxy_out) {
    if ((n_points > 0 && (!pt_xy || !pt_dxy_out))) return fail(SVGR_E_INVALID, "svgr_gvar_deltas: bad arguments");
    const char* why = "";
    if (int rc = gvar_tables(n_points, contour_off, n_contours, glyph_contour_off, n_glyphs, gv.glyph_tuple_off, gv.tuple_scalar, gv.n_tuples,
                             gv.tuple_pt_off, gv.tp_index, gv.tp_dxy, gv.n_entries, why))
        return fail(rc, "svgr_gvar_deltas: %s", why);
    if (n_points == 0) return 0;
    if (gv.n_tuples == 0) {   // the default instance: zeros, nothing is launched
        for (int64_t k = 0; k < 2 * n_points; ++k) pt_dxy_out[k] = 0.0;
        return 0;
    }
    if (!ctx) return fail(SVGR_E_INVALID, "svgr_gvar_deltas: no context");
    const int npt = (int)n_points, nc = (int)n_contours, ng = (int)n_glyphs;
    PassFrame f(ctx);
    Section<int16_t> xy;
    Section<int32_t> coff, goff;
    GvarSections gs;
    f.blob.build([&](HostBlob& b) {
        xy = b.put(pt_xy, (size_t)npt * 2), coff = b.put(contour_off, (size_t)nc + 1), goff = b.put(glyph_contour_off, (size_t)ng + 1);
        gs = gvar_put(b, gv, n_glyphs);
    });
    Layout lay;
    const Section<double> o_dxy = lay.take<double>((size_t)npt * 2);
    if (int rc = f.begin(lay)) return rc;
    const void* d_in = f.in.p;
    SVGR_LAUNCH(k_gvar_delta, grid1((size_t)npt, GVAR_B), dim3(GVAR_B), 0, f.st, gs.view(d_in, xy.on(d_in), coff.on(d_in), goff.on(d_in), nc, ng, npt),
                o_dxy.on(f.out.p), f.bad.on(f.out.p));
    if (int rc = f.finish("svgr_gvar_deltas", "a lane met a point outside its tables")) return rc;
    memcpy(pt_dxy_out, o_dxy.on(f.back.data()), (size_t)npt * 16);
    return 0;
}

extern "C" {
int svgr_glyf_block(void) { return GLYF_B; }
int svgr_gvar_block(void) { return GVAR_B; }
int svgr_glyf_outline(svgr_ctx* ctx, const int16_t* pt_xy, const uint8_t* pt_on, int64_t n_points, const int32_t* contour_off,
                      int64_t n_contours, const int32_t* glyph_contour_off, int64_t n_glyphs, const int32_t* part_glyph, const double* part_m,
                      const double* part_pen, const double* part_sx, const double* part_sy, int64_t n_parts, svgr_stroke_out** out) {
    return abi_guard("svgr_glyf_outline", [&]() {
        return glyf_outline_impl("svgr_glyf_outline", ctx, pt_xy, pt_on, n_points, contour_off, n_contours, glyph_contour_off, n_glyphs,
                                 part_glyph, part_m, part_pen, part_sx, part_sy, n_parts, nullptr, out);
    });
}
int svgr_glyf_outline_var(svgr_ctx* ctx, const int16_t* pt_xy, const uint8_t* pt_on, int64_t n_points, const int32_t* contour_off,
                          int64_t n_contours, const int32_t* glyph_contour_off, int64_t n_glyphs, const int32_t* part_glyph,
                          const double* part_m, const double* part_pen, const double* part_sx, const double* part_sy, int64_t n_parts,
                          const int32_t* glyph_tuple_off, const double* tuple_scalar, int64_t n_tuples, const int32_t* tuple_pt_off,
                          const int32_t* tp_index, const int16_t* tp_dxy, int64_t n_entries, svgr_stroke_out** out) {
    return abi_guard("svgr_glyf_outline_var", [&]() {
        const GvarIn gv{glyph_tuple_off, tuple_scalar, n_tuples, tuple_pt_off, tp_index, tp_dxy, n_entries};
        return glyf_outline_impl("svgr_glyf_outline_var", ctx, pt_xy, pt_on, n_points, contour_off, n_contours, glyph_contour_off, n_glyphs,
                                 part_glyph, part_m, part_pen, part_sx, part_sy, n_parts, &gv, out);
    });
}
int svgr_gvar_deltas(svgr_ctx* ctx, const int16_t* pt_xy, int64_t n_points, const int32_t* contour_off, int64_t n_contours,
                     const int32_t* glyph_contour_off, int64_t n_glyphs, const int32_t* glyph_tuple_off, const double* tuple_scalar,
                     int64_t n_tuples, const int32_t* tuple_pt_off, const int32_t* tp_index, const int16_t* tp_dxy, int64_t n_entries,
                     double* pt_dxy_out) {
    return abi_guard("svgr_gvar_deltas", [&]() {
        const GvarIn gv{glyph_tuple_off, tuple_scalar, n_tuples, tuple_pt_off, tp_index, tp_dxy, n_entries};
        return gvar_deltas_impl(ctx, pt_xy, n_points, contour_off, n_contours, glyph_contour_off, n_glyphs, gv, pt_dxy_out);
    });
}
}  // extern "C"

// ======================================================================================
// OpenType / CFF outlines: the contours of Type 2 charstrings as the lines and cubics of a path (svgr_cff_outline).  The
// per-lane arithmetic and the host's validation walk are svgr_cff.h; DESIGN.md 7m has the definitions.
//
//   k_cff_emit   one lane per OUTPUT segment: its part by binary search in the host-built prefix sums of the parts' segment
//                counts, its atlas segment, the 2 or 4 double points that segment reads, one type and one row of 8 doubles --
//                a wave's stores are one contiguous run
// Which points emit is a glyph constant the host made while it checked the input; stores are disjoint and no atomic takes part
// (the `bad` flag is a plain store of the same value by every writer).  No LDS.  All geometry is f64.
// ======================================================================================
#include "svgr_cff.h"

constexpr int CFF_B = 256;   // output segments (= lanes) per workgroup
#define CFF_KERNEL __global__ __launch_bounds__(CFF_B) __attribute__((section(".text.svgr_cff")))

CFF_KERNEL void k_cff_emit(CffView v, int* __restrict__ types, double* __restrict__ params, int* __restrict__ bad) {
    const int j = blockIdx.x * CFF_B + threadIdx.x;
    if (j >= v.n_out) return;
    if (!cff_emit(v, j, types, params)) *bad = 1;   // (the host zeroed it; every writer stores the same value)
}

static int cff_outline_impl(svgr_ctx* ctx, const double* pt_xy, const uint8_t* pt_kind, int64_t n_points, const int32_t* contour_off,
                            int64_t n_contours, const int32_t* glyph_contour_off, int64_t n_glyphs, const int32_t* part_glyph,
                            const double* part_m, const double* part_pen, const double* part_sx, const double* part_sy, int64_t n_parts,
                            svgr_stroke_out** out) {
    if (!out) return fail(SVGR_E_INVALID, "svgr_cff_outline: bad arguments");
    CffTables t;
    if (int rc = cff_tables(pt_xy, pt_kind, n_points, contour_off, n_contours, glyph_contour_off, n_glyphs, part_glyph, part_m, part_pen,
                            part_sx, part_sy, n_parts, t))
        return fail(rc, "svgr_cff_outline: %s", t.why);
    std::unique_ptr<svgr_stroke_out> res(new svgr_stroke_out());
    const int n_out = t.part_seg_off[(size_t)n_parts];
    if (n_out == 0) {   // no part, parts of empty glyphs, or contours of a lone MOVE only
        *out = res.release();
        return 0;
    }
    if (!ctx) return fail(SVGR_E_INVALID, "svgr_cff_outline: no context");
    // ---- one upload: the atlas with its segment tables, the parts with their prefix sums
    const int np = (int)n_parts, npt = (int)n_points, nc = (int)n_contours, ng = (int)n_glyphs, ns = (int)t.seg_ref.size();
    PassFrame f(ctx);
    Section<double> xy, m, pen, sx, sy;
    Section<uint8_t> kind;
    Section<int32_t> ref, gseg, coff, pglyph, pseg;
    f.blob.build([&](HostBlob& b) {
        xy = b.put(pt_xy, (size_t)npt * 2), kind = b.put(pt_kind, (size_t)npt), ref = b.put(t.seg_ref.data(), (size_t)ns);
        gseg = b.put(t.glyph_seg_off.data(), (size_t)ng + 1), coff = b.put(contour_off, (size_t)nc + 1), pglyph = b.put(part_glyph, (size_t)np);
        pseg = b.put(t.part_seg_off.data(), (size_t)np + 1), m = b.put(part_m, (size_t)np * 6), pen = b.put(part_pen, (size_t)np);
        sx = b.put(part_sx, (size_t)np), sy = b.put(part_sy, (size_t)np);
    });
    // the result block: params, types
    Layout lay;
    const Section<double> o_params = lay.take<double>((size_t)n_out * 8);
    const Section<int32_t> o_types = lay.take<int32_t>((size_t)n_out);
    if (int rc = f.begin(lay)) return rc;
    const void* d_in = f.in.p;
    const CffView view{xy.on(d_in), kind.on(d_in), ref.on(d_in), gseg.on(d_in), coff.on(d_in), pglyph.on(d_in), pseg.on(d_in), m.on(d_in),
                       pen.on(d_in), sx.on(d_in),  sy.on(d_in),  nc,            np,            npt,             ns,            n_out};
    SVGR_LAUNCH(k_cff_emit, grid1((size_t)n_out, CFF_B), dim3(CFF_B), 0, f.st, view, o_types.on(f.out.p), o_params.on(f.out.p), f.bad.on(f.out.p));
    if (int rc = f.finish("svgr_cff_outline", "a lane met an index outside its tables")) return rc;
    stroke_out_take(*res, f.back.data(), o_params, o_types);
    res->sizes = std::move(t.sizes);
    *out = res.release();
    return 0;
}

extern "C" {
int svgr_cff_block(void) { return CFF_B; }
int svgr_cff_outline(svgr_ctx* ctx, const double* pt_xy, const uint8_t* pt_kind, int64_t n_points, const int32_t* contour_off,
                     int64_t n_contours, const int32_t* glyph_contour_off, int64_t n_glyphs, const int32_t* part_glyph, const double* part_m,
                     const double* part_pen, const double* part_sx, const double* part_sy, int64_t n_parts, svgr_stroke_out** out) {
    return abi_guard("svgr_cff_outline", [&]() {
        return cff_outline_impl(ctx, pt_xy, pt_kind, n_points, contour_off, n_contours, glyph_contour_off, n_glyphs, part_glyph, part_m,
                                part_pen, part_sx, part_sy, n_parts, out);
    });
}
}  // extern "C"

// ======================================================================================
// PNG output on the device: scanline filters and deflate (svgr_png_filter, svgr_deflate).  The per-lane arithmetic, the token
// rule and the host's code builder are svgr_png.h / svgr_deflate.h; DESIGN.md 7n has the definitions.
//
//   k_png_filter      one workgroup per row, a lane per pixel (striding): for the adaptive choice the row's five sums first (per
//                     wave in registers, then five LDS adds per wave), then the filtered bytes of the chosen type
//   k_deflate_tokens  one workgroup per chunk.  The hash table lives in LDS and takes positions with an atomic MAX: first the 32 KiB
//                     in front of the chunk, then the chunk sub-window by sub-window, each sub-window reading its candidates
//                     before it enters itself.  Every position's best match, then the greedy parse without a walk over the chunk:
//                     each lane resolves, backwards, where a parse entering its segment at any position leaves it; one lane hops
//                     from segment to segment (as many steps as there are segments); each lane then walks its own segment from its
//                     entry, counts, and -- after a scan of the counts -- stores its tokens.  Histogram in LDS, then one global
//                     add per used symbol; the chunk's Adler pair
//   k_deflate_emit    one workgroup per chunk: a lane sums the bit lengths of its run of tokens, a scan gives each run its bit
//                     offset, the bits are OR-ed into the slot in LDS (ds_or: lanes share words), the slot is stored with dwords
//   k_scan_*          the dasher's two-level scan over the chunks' byte counts
//   k_deflate_gather  one workgroup per chunk: its bytes to their place in the one stream
// Integer sums, maxima and ORs only: the result does not depend on the order in which lanes or workgroups run.
// ======================================================================================
#include "svgr_png.h"
#include "svgr_deflate.h"

constexpr int PNG_B = 256;                        // lanes per workgroup of k_png_filter (= per row) and k_deflate_gather
constexpr int DEFL_B = 512;                       // lanes per workgroup of the two deflate kernels
constexpr int DEFL_SEG = DEFLATE_CH / DEFL_B;     // positions per lane of the parse
static_assert(DEFL_SEG == 32 && DEFL_B >= DEFLATE_SUB && DEFL_B >= DEFLATE_NSYM, "the LDS paddings below assume 32 positions per lane");
#define PNG_KERNEL(B) __global__ __launch_bounds__(B) __attribute__((section(".text.svgr_png")))
// a lane walks 32 consecutive entries: one word (two halfwords) of padding per segment keeps the lanes on different banks
#define DEFL_BI(p) ((p) + ((p) >> 5))
#define DEFL_EI(p) ((p) + (((p) >> 5) << 1))

PNG_KERNEL(PNG_B) void k_png_filter(const uint32_t* __restrict__ src, int cols, int mode, uint8_t* __restrict__ out) {
    __shared__ uint32_t sums[PNG_FILTER_TYPES];
    const int64_t row = blockIdx.x;
    int type = mode;
    if (mode == PNG_FILTER_ADAPTIVE) {   // (uniform over the launch)
        if (threadIdx.x < PNG_FILTER_TYPES) sums[threadIdx.x] = 0;
        __syncthreads();
        uint32_t s[PNG_FILTER_TYPES] = {0, 0, 0, 0, 0};
        for (int x = threadIdx.x; x < cols; x += PNG_B) {
            uint32_t px, a, b, c;
            png_neighbours(src, row, cols, x, px, a, b, c);
#pragma unroll
            for (int t = 0; t < PNG_FILTER_TYPES; ++t) s[t] += png_cost_px(png_filter_px(t, px, a, b, c));
        }
#pragma unroll
        for (int t = 0; t < PNG_FILTER_TYPES; ++t) {
            for (int d = 32; d; d >>= 1) s[t] += __shfl_down(s[t], d, 64);
            if ((threadIdx.x & 63) == 0) atomicAdd(&sums[t], s[t]);
        }
        __syncthreads();
        type = png_pick(sums);
    }
    uint8_t* o = out + (size_t)row * (1 + 4 * (size_t)cols);
    if (threadIdx.x == 0) o[0] = (uint8_t)type;
    for (int x = threadIdx.x; x < cols; x += PNG_B) {
        uint32_t px, a, b, c;
        png_neighbours(src, row, cols, x, px, a, b, c);
        png_store_px(o, x, png_filter_px(type, px, a, b, c));
    }
}

// inclusive sum scan over the workgroup's DEFL_B values, in sh
__device__ __forceinline__ void defl_scan(uint32_t* sh, uint32_t v) {
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int d = 1; d < DEFL_B; d <<= 1) {
        uint32_t x = sh[t];
        if (t >= d) x += sh[t - d];
        __syncthreads();
        sh[t] = x;
        __syncthreads();
    }
}

struct DeflTokArgs {
    const uint8_t* src;
    long long n;
    uint32_t* tok;               // DEFLATE_CH per chunk
    int* n_tok;
    uint32_t* adler;             // 2 per chunk
    unsigned long long* hist;    // DEFLATE_NSYM, zeroed by the host
};
PNG_KERNEL(DEFL_B) void k_deflate_tokens(DeflTokArgs a) {
    __shared__ uint32_t table[1 << DEFLATE_HASH_BITS];
    __shared__ uint32_t best[DEFLATE_CH + DEFLATE_CH / 32];   // first the hash candidates, then the positions' tokens
    __shared__ uint16_t exitp[DEFLATE_CH + DEFLATE_CH / 16];
    __shared__ uint32_t hist[DEFL_B];
    __shared__ uint32_t scan[DEFL_B];
    __shared__ uint16_t entry[DEFL_B];
    __shared__ unsigned long long ad[2];
    const int t = threadIdx.x;
    const long long start = (long long)blockIdx.x * DEFLATE_CH, base = start - DEFLATE_WINDOW;
    const long long end = a.n < start + DEFLATE_CH ? a.n : start + DEFLATE_CH;
    const int len = (int)(end - start);   // (0 for the one chunk of an empty input)
    for (int i = t; i < (1 << DEFLATE_HASH_BITS); i += DEFL_B) table[i] = 0;
    hist[t] = 0;
    entry[t] = 0xFFFF;
    if (t < 2) ad[t] = 0;
    __syncthreads();
    // ---- the window in front of the chunk (an entry is position - base + 1; 0: none)
    for (long long q = (base > 0 ? base : 0) + t; q < start; q += DEFL_B)
        if (deflate_hashed(q, a.n)) atomicMax(&table[deflate_hash3(a.src + q)], (uint32_t)(q - base + 1));
    __syncthreads();
    // ---- the chunk, sub-window by sub-window: read the candidates, then enter the sub-window
    for (int w = 0; w < len; w += DEFLATE_SUB) {
        const int i = w + t;
        const bool in = t < DEFLATE_SUB && i < len, hashed = in && start + i + 2 < end;
        uint32_t h = 0, cand = 0;
        if (hashed) {
            h = deflate_hash3(a.src + start + i);
            cand = table[h];
        }
        if (in) best[DEFL_BI(i)] = cand;
        __syncthreads();
        if (hashed) atomicMax(&table[h], (uint32_t)(start + i - base + 1));
        __syncthreads();
    }
    // ---- every position's token, and the Adler sums on the way
    unsigned long long A = 0, B = 0;
    for (int i = t; i < len; i += DEFL_B) {
        const uint32_t cand = best[DEFL_BI(i)];
        best[DEFL_BI(i)] = deflate_best(a.src, start + i, end, cand ? base + cand - 1 : -1);
        const uint32_t b = a.src[start + i];
        A += b;
        B += (unsigned long long)(len - i) * b;
    }
    __syncthreads();
    // ---- the parse: where a parse that enters my segment at i leaves it
    const int s0 = t * DEFL_SEG, s1 = s0 + DEFL_SEG < len ? s0 + DEFL_SEG : len;
    for (int i = s1 - 1; i >= s0; --i) {
        const int nx = i + deflate_tok_hop(best[DEFL_BI(i)]);
        exitp[DEFL_EI(i)] = nx >= s1 ? (uint16_t)nx : exitp[DEFL_EI(nx)];
    }
    __syncthreads();
    if (t == 0)
        for (int e = 0; e < len; e = exitp[DEFL_EI(e)]) entry[e / DEFL_SEG] = (uint16_t)e;
    __syncthreads();
    const int e0 = entry[t];
    uint32_t cnt = 0;
    if (e0 != 0xFFFF)
        for (int p = e0; p < s1; p += deflate_tok_hop(best[DEFL_BI(p)])) ++cnt;
    defl_scan(scan, cnt);
    if (e0 != 0xFFFF) {
        uint32_t* o = a.tok + (size_t)blockIdx.x * DEFLATE_CH + (scan[t] - cnt);
        for (int p = e0; p < s1;) {
            const uint32_t tok = best[DEFL_BI(p)];
            *o++ = tok;
            int ls, ds;
            deflate_token_syms(tok, ls, ds);
            atomicAdd(&hist[ls], 1u);
            if (ds >= 0) atomicAdd(&hist[DEFLATE_NLIT + ds], 1u);
            p += deflate_tok_hop(tok);
        }
    }
    for (int d = 32; d; d >>= 1) {
        A += __shfl_down(A, d, 64);
        B += __shfl_down(B, d, 64);
    }
    if ((t & 63) == 0) {
        atomicAdd(&ad[0], A);
        atomicAdd(&ad[1], B);
    }
    __syncthreads();
    if (t < DEFLATE_NSYM) {
        const uint32_t h = hist[t] + (t == DEFLATE_EOB ? 1u : 0u);
        if (h) atomicAdd(&a.hist[t], (unsigned long long)h);
    }
    if (t == 0) {
        a.n_tok[blockIdx.x] = (int)scan[DEFL_B - 1];
        a.adler[2 * (size_t)blockIdx.x] = (uint32_t)(ad[0] % ADLER_MOD);
        a.adler[2 * (size_t)blockIdx.x + 1] = (uint32_t)(ad[1] % ADLER_MOD);
    }
}

struct DeflEmitArgs {
    const uint32_t* tok;
    const int* n_tok;
    const DeflateCodes* codes;
    uint8_t* slots;              // DEFLATE_SLOT per chunk
    long long* cnt;              // the chunk's bytes
    long long* incl;             // the same again: scanned in place afterwards
    int n_chunks;
};
PNG_KERNEL(DEFL_B) void k_deflate_emit(DeflEmitArgs a) {
    __shared__ uint32_t words[DEFLATE_SLOT / 4];
    __shared__ DeflateCodes c;
    __shared__ uint32_t scan[DEFL_B];
    __shared__ uint32_t n_bytes;
    const int t = threadIdx.x;
    const bool last = (int)blockIdx.x == a.n_chunks - 1;
    for (int i = t; i < (int)(sizeof(DeflateCodes) / 4); i += DEFL_B) ((uint32_t*)&c)[i] = ((const uint32_t*)a.codes)[i];
    for (int i = t; i < DEFLATE_SLOT / 4; i += DEFL_B) words[i] = 0;
    __syncthreads();
    const uint32_t* tok = a.tok + (size_t)blockIdx.x * DEFLATE_CH;
    const int n = a.n_tok[blockIdx.x], per = (n + DEFL_B - 1) / DEFL_B;
    const int i0 = t * per < n ? t * per : n, i1 = i0 + per < n ? i0 + per : n;
    uint32_t bits = 0;
    uint64_t v;
    for (int i = i0; i < i1; ++i) bits += (uint32_t)deflate_token_bits(c.lcode, c.llen, c.dcode, c.dlen, tok[i], v);
    defl_scan(scan, bits);
    if (t < (int)((c.hdr_bits + 31) / 32)) atomicOr(&words[t], c.hdr[t] | (t == 0 && last ? 1u : 0u));   // (BFINAL is the first bit)
    uint32_t pos = c.hdr_bits + scan[t] - bits;
    for (int i = i0; i < i1; ++i) {
        const int nb = deflate_token_bits(c.lcode, c.llen, c.dcode, c.dlen, tok[i], v);
        deflate_put(words, pos, v);
        pos += (uint32_t)nb;
    }
    if (t == 0) n_bytes = deflate_chunk_tail(words, c.hdr_bits + scan[DEFL_B - 1], c.lcode[DEFLATE_EOB], c.llen[DEFLATE_EOB], last);
    __syncthreads();
    uint32_t* o = (uint32_t*)(a.slots + (size_t)blockIdx.x * DEFLATE_SLOT);
    for (int i = t; i < (int)((n_bytes + 3) / 4); i += DEFL_B) o[i] = words[i];
    if (t == 0) a.cnt[blockIdx.x] = a.incl[blockIdx.x] = n_bytes;
}

struct DeflSumOp {
    __device__ static long long zero() { return 0; }
    __device__ static long long add(const long long& a, const long long& b) { return a + b; }
};
PNG_KERNEL(PNG_B) void k_deflate_gather(const uint8_t* __restrict__ slots, const long long* __restrict__ cnt,
                                        const long long* __restrict__ incl, uint8_t* __restrict__ out) {
    const long long n = cnt[blockIdx.x];
    const uint8_t* s = slots + (size_t)blockIdx.x * DEFLATE_SLOT;
    uint8_t* o = out + (incl[blockIdx.x] - n);
    for (long long i = threadIdx.x; i < n; i += PNG_B) o[i] = s[i];
}

constexpr int64_t DEFLATE_MAX_BYTES = (int64_t)5 << 30;   // (the filtered stream of the largest image: 2^30 pixels and their rows' type bytes)

static int deflate_impl(svgr_ctx* ctx, const svgr_buf* src, int64_t n_bytes, int huffman, uint8_t* out, int64_t out_cap, int64_t* n_out) {
    if (!ctx || !src || !n_out || n_bytes < 0 || out_cap < 0 || (!out && out_cap) || (n_bytes && !src->ptr))
        return fail(SVGR_E_INVALID, "svgr_deflate: bad arguments");
    if (huffman != SVGR_DEFLATE_FIXED && huffman != SVGR_DEFLATE_DYNAMIC) return fail(SVGR_E_INVALID, "svgr_deflate: unknown Huffman mode %d", huffman);
    if (n_bytes > DEFLATE_MAX_BYTES) return fail(SVGR_E_INVALID, "svgr_deflate: %lld bytes are more than %lld", (long long)n_bytes, (long long)DEFLATE_MAX_BYTES);
    if (src->bytes < (size_t)n_bytes) return fail(SVGR_E_INVALID, "svgr_deflate: buffer too small");
    static_assert(SVGR_DEFLATE_FIXED == DEFLATE_FIXED && SVGR_DEFLATE_DYNAMIC == DEFLATE_DYNAMIC, "Huffman modes");
    const int nc = n_bytes ? (int)((n_bytes + DEFLATE_CH - 1) / DEFLATE_CH) : 1;
    const int nb = (nc + DASH_S - 1) / DASH_S;
    // one block of small arrays: histogram, codes, per chunk the token count, the Adler pair, the byte count twice, the scan's tops
    Layout lay;
    const Section<unsigned long long> s_hist = lay.take<unsigned long long>(DEFLATE_NSYM);
    const Section<DeflateCodes> s_codes = lay.take<DeflateCodes>(1);
    const Section<int> s_ntok = lay.take<int>((size_t)nc);
    const Section<uint32_t> s_adler = lay.take<uint32_t>((size_t)nc * 2);
    const Section<long long> s_cnt = lay.take<long long>((size_t)nc), s_incl = lay.take<long long>((size_t)nc), s_tops = lay.take<long long>((size_t)nb);
    unsigned long long counts[DEFLATE_NSYM] = {0};
    DeflateCodes codes;
    std::vector<uint32_t> adler((size_t)nc * 2);
    long long total = 0;
    PassFrame f(ctx);   // (no upload and no result block: its scratch blocks and its drain)
    HIPCHK(enter_ctx(ctx));
    hipStream_t st = f.st;
    char* d = f.scratch<char>(lay.bytes());
    uint32_t* toks = f.scratch<uint32_t>((size_t)nc * DEFLATE_CH);
    uint8_t* slots = f.scratch<uint8_t>((size_t)nc * DEFLATE_SLOT);
    if (f.err) return f.err;
    unsigned long long* d_hist = s_hist.on(d);
    long long *d_cnt = s_cnt.on(d), *d_incl = s_incl.on(d);
    HIPCHK(hipMemsetAsync(d_hist, 0, DEFLATE_NSYM * 8, st));
    const DeflTokArgs ta{(const uint8_t*)src->ptr, (long long)n_bytes, toks, s_ntok.on(d), s_adler.on(d), d_hist};
    SVGR_LAUNCH(k_deflate_tokens, dim3((unsigned)nc), dim3(DEFL_B), 0, st, ta);
    HIPCHK(hipGetLastError());
    if (huffman == DEFLATE_DYNAMIC) {   // the one round trip: 316 counts down, the tables and the header up
        HIPCHK(hipMemcpyAsync(counts, d_hist, sizeof counts, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "counts");
    deflate_build_codes((const uint64_t*)counts, huffman, codes);
    HIPCHK(hipMemcpyAsync(s_codes.on(d), &codes, sizeof codes, hipMemcpyHostToDevice, st));
    const DeflEmitArgs ea{toks, s_ntok.on(d), s_codes.on(d), slots, d_cnt, d_incl, nc};
    SVGR_LAUNCH(k_deflate_emit, dim3((unsigned)nc), dim3(DEFL_B), 0, st, ea);
    dash_scan<long long, DeflSumOp>(st, d_incl, s_tops.on(d), nc);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(&total, d_incl + (nc - 1), 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(adler.data(), s_adler.on(d), (size_t)nc * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (total <= 0 || total > (long long)nc * DEFLATE_SLOT) return fail(SVGR_E_STATE, "svgr_deflate: the chunks' byte counts do not add up");
    *n_out = 2 + total + 4;
    if (*n_out > out_cap) return SVGR_DEFLATE_NO_ROOM;
    // ---- only the compressed bytes cross: the chunks' bytes to one run, then one download
    uint8_t* packed = f.scratch<uint8_t>((size_t)total);
    if (f.err) return f.err;
    SVGR_LAUNCH(k_deflate_gather, dim3((unsigned)nc), dim3(PNG_B), 0, st, slots, d_cnt, d_incl, packed);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out + 2, packed, (size_t)total, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    out[0] = 0x78;   // CMF: deflate, 32 KiB window; FLG: fastest, FCHECK
    out[1] = 0x01;
    uint32_t s1 = 1, s2 = 0;
    for (int k = 0; k < nc; ++k) {
        const long long len = std::min<long long>(DEFLATE_CH, (long long)n_bytes - (long long)k * DEFLATE_CH);
        adler_combine(s1, s2, adler[2 * (size_t)k], adler[2 * (size_t)k + 1], len);
    }
    const uint32_t ad = (s2 << 16) | s1;
    uint8_t* tail = out + 2 + total;
    tail[0] = (uint8_t)(ad >> 24); tail[1] = (uint8_t)(ad >> 16); tail[2] = (uint8_t)(ad >> 8); tail[3] = (uint8_t)ad;
    return 0;
}

extern "C" {
int svgr_deflate_chunk(void) { return DEFLATE_CH; }
int svgr_png_filter(svgr_ctx* ctx, const svgr_buf* src_rgba8, int64_t rows, int64_t cols, int filter, svgr_buf* out_filtered) {
    if (!ctx || !src_rgba8 || !out_filtered || !image_size_ok(rows, cols)) return fail(SVGR_E_INVALID, "svgr_png_filter: bad arguments");
    if (filter < 0 || filter > SVGR_PNG_FILTER_ADAPTIVE) return fail(SVGR_E_INVALID, "svgr_png_filter: unknown filter %d", filter);
    static_assert(SVGR_PNG_FILTER_ADAPTIVE == PNG_FILTER_ADAPTIVE, "filter numbers");
    if (src_rgba8->bytes < (size_t)rows * cols * 4 || out_filtered->bytes < (size_t)rows * (1 + 4 * (size_t)cols))
        return fail(SVGR_E_INVALID, "svgr_png_filter: buffer too small");
    if (src_rgba8->ptr == out_filtered->ptr) return fail(SVGR_E_INVALID, "svgr_png_filter: the output must not be the source");
    return launch_tail(ctx, k_png_filter, dim3((unsigned)rows), dim3(PNG_B), 0, (const uint32_t*)src_rgba8->ptr, (int)cols, filter,
                       (uint8_t*)out_filtered->ptr);
}
int svgr_deflate(svgr_ctx* ctx, const svgr_buf* src, int64_t n_bytes, int huffman, uint8_t* out, int64_t out_cap, int64_t* n_out) {
    return abi_guard("svgr_deflate", [&]() { return deflate_impl(ctx, src, n_bytes, huffman, out, out_cap, n_out); });
}
}  // extern "C"

// --------------------------------------------------------------------------------------
// PNG sample formats (svgr_png_samples, svgr_png_filter_bytes): grey, grey + alpha, RGB and RGBA at 8 or 16 bits.  The arithmetic
// is the second part of svgr_png.h; DESIGN.md 7v has the definitions.
//
//   k_png_samples       a lane per pixel: one 32-byte load (a double4; 8 bytes of a mask, 4 of a byte pixel), the pixel's 1 to 8
//                       sample bytes put together in registers, and the widest stores their place allows: a dword pair at bpp
//                       8, a dword at 4, a short at 2; at 6 a dword and a short, at 3 a short and a byte, in the order the
//                       pixel's parity asks for; a byte at 1
//   k_png_filter_bytes  one workgroup per row, PNGF_SPAN bytes of the row per pass, a lane four consecutive bytes of them at a time.
//                       A row of a 1-, 2-, 3- or 6-byte format begins anywhere, so a pass first brings the ALIGNED dwords that
//                       cover its span and the 8 bytes in front of it (the furthest a left neighbour lies back) into LDS, the
//                       current row's and the row's above, lane t the words t, t + 256, ...  A lane then reads four consecutive words of each,
//                       shifts them into the three dwords that begin 8 bytes in front of its own four bytes (the row's
//                       misalignment is the same for every lane), and has x, a, b, c of its bytes in registers, a dword each:
//                       the operands of png_filter_px, whose bytes are filtered on their own whatever the pixel size.  The adaptive
//                       choice sums as k_png_filter does: per lane, a wave shuffle, one LDS add per wave and type
// --------------------------------------------------------------------------------------
constexpr int PNGF_LANE_WORDS = 8;                            // dwords of a span per lane
constexpr int PNGF_SPAN = 4 * PNGF_LANE_WORDS * PNG_B;        // bytes of a row per pass of k_png_filter_bytes
constexpr int PNGF_BACK = 8;                                  // bytes in front of a span that its first bytes' neighbours may lie in (the largest bpp)
constexpr int PNGF_WORDS = (PNGF_BACK + PNGF_SPAN) / 4 + 1;   // aligned dwords that cover them at any misalignment

template <int KIND>
PNG_KERNEL(PNG_B) void k_png_samples(const void* __restrict__ src, long long n_px, int color, int depth, uint8_t* __restrict__ dst) {
    const long long i = (long long)blockIdx.x * PNG_B + threadIdx.x;
    if (i >= n_px) return;
    uint64_t s;
    if (KIND == PNG_SRC_RGBA_F64) {
        const double4 v = ((const double4*)src)[i];
        s = png_samples_px(v.x, v.y, v.z, v.w, color, depth);
    } else if (KIND == PNG_SRC_MASK_F64) {
        s = png_samples_px(((const double*)src)[i], depth);
    } else {
        s = png_samples_px(((const uint32_t*)src)[i], color, depth);
    }
    const uint32_t lo = (uint32_t)s, hi = (uint32_t)(s >> 32);
    const int bpp = png_bpp(color, depth);   // (uniform over the launch)
    uint8_t* o = dst + i * bpp;
    if (bpp == 8) {
        *(uint2*)o = make_uint2(lo, hi);
    } else if (bpp == 4) {
        *(uint32_t*)o = lo;
    } else if (bpp == 2) {
        *(uint16_t*)o = (uint16_t)lo;
    } else if (bpp == 1) {
        *o = (uint8_t)lo;
    } else if (bpp == 6) {   // (6 i is a multiple of 4 at an even pixel, of 2 at an odd one)
        if (i & 1) {
            *(uint16_t*)o = (uint16_t)lo;
            *(uint32_t*)(o + 2) = (lo >> 16) | (hi << 16);
        } else {
            *(uint32_t*)o = lo;
            *(uint16_t*)(o + 4) = (uint16_t)hi;
        }
    } else {                 // bpp 3: 3 i is even at an even pixel
        if (i & 1) {
            *o = (uint8_t)lo;
            *(uint16_t*)(o + 1) = (uint16_t)(lo >> 8);
        } else {
            *(uint16_t*)o = (uint16_t)lo;
            o[2] = (uint8_t)(lo >> 16);
        }
    }
}

// Aligned dword d of an image of `total` bytes; zero in front of it and behind it, the last bytes one by one where the image does
// not end on a dword.
__device__ __forceinline__ uint32_t pngf_load_word(const uint8_t* __restrict__ src, long long d, long long total) {
    const long long o = d * 4;
    if (d < 0 || o >= total) return 0u;
    if (o + 4 <= total) return *(const uint32_t*)(src + o);
    uint32_t w = 0;
    for (int k = 0; k < 3; ++k)
        if (o + k < total) w |= (uint32_t)src[o + k] << (8 * k);
    return w;
}

// The aligned dwords that cover `bytes` image bytes from byte `first` on (which may lie in front of the image) into LDS, zeros
// behind them up to PNGF_WORDS; lane t has the words t, t + 256, ... (its loads are independent and go out together).  Returns
// where in the first dword that byte is.
__device__ __forceinline__ int pngf_stage(uint32_t* lds, const uint8_t* __restrict__ src, long long first, int bytes, long long total) {
    const int m = (int)(first & 3), t = threadIdx.x;
    const long long d0 = (first - m) / 4;
    const int n_words = (m + bytes + 3) >> 2;
    uint32_t w[PNGF_LANE_WORDS];
#pragma unroll
    for (int j = 0; j < PNGF_LANE_WORDS; ++j) w[j] = t + j * PNG_B < n_words ? pngf_load_word(src, d0 + t + j * PNG_B, total) : 0u;
#pragma unroll
    for (int j = 0; j < PNGF_LANE_WORDS; ++j) lds[t + j * PNG_B] = w[j];
    constexpr int DONE = PNGF_LANE_WORDS * PNG_B;
    if (t < PNGF_WORDS - DONE) lds[DONE + t] = DONE + t < n_words ? pngf_load_word(src, d0 + DONE + t, total) : 0u;
    return m;
}

// The three dwords that begin PNGF_BACK bytes in front of lane t's four bytes, out of the staged words.
__device__ __forceinline__ void pngf_window(const uint32_t* lds, int t, int m, uint32_t* w) {
    const uint32_t q0 = lds[t], q1 = lds[t + 1], q2 = lds[t + 2], q3 = lds[t + 3];
    const int sh = 8 * m;
    w[0] = (uint32_t)((((uint64_t)q1 << 32) | q0) >> sh);
    w[1] = (uint32_t)((((uint64_t)q2 << 32) | q1) >> sh);
    w[2] = (uint32_t)((((uint64_t)q3 << 32) | q2) >> sh);
}
// The dword at byte `off` (a constant, at most 8) of such a window.
__device__ __forceinline__ uint32_t pngf_dword(const uint32_t* w, int off) {
    const int i = off >> 2, sh = 8 * (off & 3);
    return sh ? (w[i] >> sh) | (w[i + 1] << (32 - sh)) : w[i];
}

// Four filtered bytes to their place in the stream, which begins anywhere: the widest stores `o`'s alignment allows.
__device__ __forceinline__ void pngf_store(uint8_t* o, uint32_t f, int n) {
    const int al = (int)((uintptr_t)o & 3);
    if (n == 4 && al == 0) {
        *(uint32_t*)o = f;
    } else if (n == 4 && al == 2) {
        *(uint16_t*)o = (uint16_t)f;
        *(uint16_t*)(o + 2) = (uint16_t)(f >> 16);
    } else if (n == 4) {
        o[0] = (uint8_t)f;
        *(uint16_t*)(o + 1) = (uint16_t)(f >> 8);
        o[3] = (uint8_t)(f >> 24);
    } else {
        for (int k = 0; k < n; ++k) o[k] = (uint8_t)(f >> (8 * k));
    }
}

template <int BPP>
PNG_KERNEL(PNG_B) void k_png_filter_bytes(const uint8_t* __restrict__ src, long long total, int row_bytes, int mode, uint8_t* __restrict__ out) {
    __shared__ uint32_t cur[PNGF_WORDS], abv[PNGF_WORDS];   // (the last lane's last window ends with the last word)
    __shared__ uint32_t sums[PNG_FILTER_TYPES];
    const int row = blockIdx.x, t = threadIdx.x;
    const long long g0 = (long long)row * row_bytes;
    int type = mode;
    if (mode == PNG_FILTER_ADAPTIVE && t < PNG_FILTER_TYPES) sums[t] = 0;
    uint32_t s[PNG_FILTER_TYPES] = {0, 0, 0, 0, 0};
    uint8_t* const o_row = out + (size_t)row * (1 + (size_t)row_bytes);
    // pass 0 sums (adaptive only), pass 1 writes
    for (int pass = mode == PNG_FILTER_ADAPTIVE ? 0 : 1; pass < 2; ++pass) {
        for (int s0 = 0; s0 < row_bytes; s0 += PNGF_SPAN) {
            __syncthreads();   // (the words of the span before have been read)
            const int need = PNGF_BACK + (row_bytes - s0 < PNGF_SPAN ? row_bytes - s0 : PNGF_SPAN);
            const int m = pngf_stage(cur, src, g0 + s0 - PNGF_BACK, need, total);
            const int ma = row ? pngf_stage(abv, src, g0 - row_bytes + s0 - PNGF_BACK, need, total) : 0;
            __syncthreads();
            for (int j = 0; j < PNGF_LANE_WORDS; ++j) {   // (lane t: the span's dwords t, t + 256, ...)
                const int q = t + j * PNG_B, i0 = s0 + 4 * q;
                if (i0 >= row_bytes) break;
                uint32_t wc[3], wa[3] = {0u, 0u, 0u};
                pngf_window(cur, q, m, wc);
                if (row) pngf_window(abv, q, ma, wa);
                const int n = row_bytes - i0 < 4 ? row_bytes - i0 : 4;
                // its four bytes x, their left neighbours a, and b, c above them, a dword each: png_filter_px's operands
                const uint32_t x = wc[2], b = wa[2];
                uint32_t a = pngf_dword(wc, PNGF_BACK - BPP), c = pngf_dword(wa, PNGF_BACK - BPP);
                if (i0 < BPP) {   // (the row's first pixel: nothing to its left)
                    uint32_t keep = 0;
                    for (int k = 0; k < 4; ++k)
                        if (i0 + k >= BPP) keep |= 255u << (8 * k);
                    a &= keep;
                    c &= keep;
                }
                const uint32_t inside = n == 4 ? 0xFFFFFFFFu : (1u << (8 * n)) - 1u;   // (a filtered byte of 0 adds nothing to a sum)
                if (pass == 0) {
#pragma unroll
                    for (int ty = 0; ty < PNG_FILTER_TYPES; ++ty) s[ty] += png_cost_px(png_filter_px(ty, x, a, b, c) & inside);
                } else {
                    pngf_store(o_row + 1 + i0, png_filter_px(type, x, a, b, c), n);
                }
            }
        }
        if (pass == 0) {
#pragma unroll
            for (int ty = 0; ty < PNG_FILTER_TYPES; ++ty) {
                for (int d = 32; d; d >>= 1) s[ty] += __shfl_down(s[ty], d, 64);
                if ((t & 63) == 0) atomicAdd(&sums[ty], s[ty]);
            }
            __syncthreads();
            type = png_pick(sums);
        }
    }
    if (t == 0) o_row[0] = (uint8_t)type;
}

template <int BPP>
static int png_filter_bytes_launch(svgr_ctx* ctx, const svgr_buf* src, int64_t rows, int64_t row_bytes, int filter, svgr_buf* out) {
    return launch_tail(ctx, k_png_filter_bytes<BPP>, dim3((unsigned)rows), dim3(PNG_B), 0, (const uint8_t*)src->ptr, (long long)(rows * row_bytes),
                       (int)row_bytes, filter, (uint8_t*)out->ptr);
}

extern "C" {
int svgr_png_filter_span(void) { return PNGF_SPAN; }
int svgr_png_samples(svgr_ctx* ctx, const svgr_buf* src, int src_kind, int64_t rows, int64_t cols, int color, int depth, svgr_buf* dst) {
    if (!ctx || !src || !dst || !image_size_ok(rows, cols)) return fail(SVGR_E_INVALID, "svgr_png_samples: bad arguments");
    static_assert(SVGR_PNG_SRC_RGBA_F64 == PNG_SRC_RGBA_F64 && SVGR_PNG_SRC_MASK_F64 == PNG_SRC_MASK_F64 && SVGR_PNG_SRC_RGBA_U8 == PNG_SRC_RGBA_U8, "source kinds");
    static_assert(SVGR_PNG_COLOR_GREY == PNG_COLOR_GREY && SVGR_PNG_COLOR_RGB == PNG_COLOR_RGB && SVGR_PNG_COLOR_GREY_ALPHA == PNG_COLOR_GREY_ALPHA &&
                  SVGR_PNG_COLOR_RGBA == PNG_COLOR_RGBA, "colour types");
    const int bpp = png_bpp(color, depth);
    if (!bpp) return fail(SVGR_E_INVALID, "svgr_png_samples: unknown colour type %d or depth %d", color, depth);
    if (src_kind < SVGR_PNG_SRC_RGBA_F64 || src_kind > SVGR_PNG_SRC_RGBA_U8) return fail(SVGR_E_INVALID, "svgr_png_samples: unknown source kind %d", src_kind);
    if (src_kind == SVGR_PNG_SRC_MASK_F64 && color != SVGR_PNG_COLOR_GREY) return fail(SVGR_E_INVALID, "svgr_png_samples: a mask is written as grey only");
    const size_t n = (size_t)rows * cols, src_px = src_kind == SVGR_PNG_SRC_RGBA_F64 ? 32 : src_kind == SVGR_PNG_SRC_MASK_F64 ? 8 : 4;
    if (src->bytes < n * src_px || dst->bytes < n * (size_t)bpp) return fail(SVGR_E_INVALID, "svgr_png_samples: buffer too small");
    if (src->ptr == dst->ptr) return fail(SVGR_E_INVALID, "svgr_png_samples: the output must not be the source");
    if ((uintptr_t)src->ptr % src_px || (uintptr_t)dst->ptr % 8) return fail(SVGR_E_INVALID, "svgr_png_samples: a buffer is not aligned to its elements");
    const dim3 grid((unsigned)((n + PNG_B - 1) / PNG_B));
    uint8_t* o = (uint8_t*)dst->ptr;
    if (src_kind == SVGR_PNG_SRC_RGBA_F64) return launch_tail(ctx, k_png_samples<PNG_SRC_RGBA_F64>, grid, dim3(PNG_B), 0, (const void*)src->ptr, (long long)n, color, depth, o);
    if (src_kind == SVGR_PNG_SRC_MASK_F64) return launch_tail(ctx, k_png_samples<PNG_SRC_MASK_F64>, grid, dim3(PNG_B), 0, (const void*)src->ptr, (long long)n, color, depth, o);
    return launch_tail(ctx, k_png_samples<PNG_SRC_RGBA_U8>, grid, dim3(PNG_B), 0, (const void*)src->ptr, (long long)n, color, depth, o);
}
int svgr_png_filter_bytes(svgr_ctx* ctx, const svgr_buf* src, int64_t rows, int64_t row_bytes, int bpp, int filter, svgr_buf* out_filtered) {
    if (!ctx || !src || !out_filtered) return fail(SVGR_E_INVALID, "svgr_png_filter_bytes: bad arguments");
    if (!png_bpp_ok(bpp)) return fail(SVGR_E_INVALID, "svgr_png_filter_bytes: %d bytes per pixel is none of 1, 2, 3, 4, 6, 8", bpp);
    if (row_bytes <= 0 || row_bytes % bpp) return fail(SVGR_E_INVALID, "svgr_png_filter_bytes: a row of %lld bytes is no whole number of %d-byte pixels", (long long)row_bytes, bpp);
    if (!image_size_ok(rows, row_bytes / bpp)) return fail(SVGR_E_INVALID, "svgr_png_filter_bytes: bad arguments");
    if (filter < 0 || filter > SVGR_PNG_FILTER_ADAPTIVE) return fail(SVGR_E_INVALID, "svgr_png_filter_bytes: unknown filter %d", filter);
    if (src->bytes < (size_t)rows * row_bytes || out_filtered->bytes < (size_t)rows * (1 + (size_t)row_bytes))
        return fail(SVGR_E_INVALID, "svgr_png_filter_bytes: buffer too small");
    if (src->ptr == out_filtered->ptr) return fail(SVGR_E_INVALID, "svgr_png_filter_bytes: the output must not be the source");
    if ((uintptr_t)src->ptr % 4 || (uintptr_t)out_filtered->ptr % 4) return fail(SVGR_E_INVALID, "svgr_png_filter_bytes: a buffer is not aligned to a dword");
    switch (bpp) {
        case 1: return png_filter_bytes_launch<1>(ctx, src, rows, row_bytes, filter, out_filtered);
        case 2: return png_filter_bytes_launch<2>(ctx, src, rows, row_bytes, filter, out_filtered);
        case 3: return png_filter_bytes_launch<3>(ctx, src, rows, row_bytes, filter, out_filtered);
        case 4: return png_filter_bytes_launch<4>(ctx, src, rows, row_bytes, filter, out_filtered);
        case 6: return png_filter_bytes_launch<6>(ctx, src, rows, row_bytes, filter, out_filtered);
        default: return png_filter_bytes_launch<8>(ctx, src, rows, row_bytes, filter, out_filtered);
    }
}
}  // extern "C"

// ======================================================================================
// tensor output: svgr_layer_to_tensor / svgr_tensor_to_layer (csrc/svgr_tensor.h has the per-pixel arithmetic, DESIGN.md 7p the
// rest), and the two stream-ordering entries
// ======================================================================================
#include "svgr_tensor.h"

// k_tensor_pack is a transposition from 32-byte (or 16-byte) pixels to narrow planes, through LDS: a workgroup takes TENSOR_BLOCK
// consecutive pixels of ONE row (rows are strided: nothing runs across a row's end).
//   phase 1  lane t takes the pixels t, t + 256, ...: consecutive lanes read consecutive pixels (a double4 apiece: whole cache
//            lines per instruction), run them through tensor_px / tensor_encode, and put the ELEMENTS -- 1, 2 or 4 bytes --
//            into LDS, a row per plane.  What is transposed is the narrow result, not the doubles
//   phase 2  the LDS rows go out in 16-byte units, a unit per lane: TENSOR_RUN pixels of a 2-byte plane.  An element sits in
//            LDS at its GLOBAL element address modulo a unit, so a unit is aligned in LDS exactly when it is in memory, wherever
//            the row begins: the stores of a row's interior are all dwordx4.  For that a workgroup's share of a plane's row
//            does not end at its pixels' ends but at the unit boundary at or below them (it reaches back TENSOR_MARGIN elements
//            at most into the pixels of the workgroup before, which it converts again: 16 of 2048); only the first
//            workgroup's head and the last one's tail, the row's own ragged ends, are stored element by element
// An interleaved destination is one plane of cols * channels elements per row.
constexpr int TENSOR_LANES = 256, TENSOR_RUN = 8, TENSOR_BLOCK = TENSOR_LANES * TENSOR_RUN, TENSOR_MARGIN = 16;
struct TensorLaunch {
    TensorOp op;
    int src_kind, n_ch;
    int planes, per_px;        // planar: n_ch planes of 1 element per pixel; interleaved: 1 plane of n_ch
    Box sb;                    // the source layer's box
    long long rows, cols;
    long long stride_p, stride_h, offset;   // elements
};
static_assert(SVGR_TENSOR_SRC_RGBA_F64 == TENSOR_SRC_RGBA_F64 && SVGR_TENSOR_SRC_RGBA_F32 == TENSOR_SRC_RGBA_F32 &&
              SVGR_TENSOR_SRC_MASK_F64 == TENSOR_SRC_MASK_F64 && SVGR_TENSOR_F32 == TENSOR_F32 && SVGR_TENSOR_F16 == TENSOR_F16 &&
              SVGR_TENSOR_BF16 == TENSOR_BF16 && SVGR_TENSOR_U8 == TENSOR_U8 && SVGR_TENSOR_RGBA == TENSOR_RGBA &&
              SVGR_TENSOR_RGB == TENSOR_RGB && SVGR_TENSOR_ALPHA == TENSOR_ALPHA && SVGR_TENSOR_LUMA == TENSOR_LUMA, "tensor enums");

template <class T>   // the element: uint32_t (F32), uint16_t (F16, BF16), uint8_t (U8)
__global__ __launch_bounds__(TENSOR_LANES) void k_tensor_pack(T* __restrict__ dst, const void* __restrict__ src, const TensorLaunch a) {
    constexpr long long E = 16 / sizeof(T);                     // elements of a unit
    constexpr int PLANE = 4 * (TENSOR_BLOCK + 2 * TENSOR_MARGIN);   // elements of LDS: four planes of a block and its margins (planar RGBA)
    __shared__ __align__(16) T lds[PLANE];                          // (interleaved RGBA: one plane of 4 * TENSOR_BLOCK + 2 * TENSOR_MARGIN)
    const int tid = threadIdx.x, Q = a.per_px, plane_lds = Q * TENSOR_BLOCK + 2 * TENSOR_MARGIN;
    const long long C0 = (long long)blockIdx.x * TENSOR_BLOCK, C1 = C0 + TENSOR_BLOCK < a.cols ? C0 + TENSOR_BLOCK : a.cols;
    const long long J0 = C0 * Q, J1 = C1 * Q;                          // this workgroup's pixels as elements of a plane's row
    const long long jlo = J0 > TENSOR_MARGIN ? J0 - TENSOR_MARGIN : 0;  // the first element it may have to provide
    const long long clo = jlo / Q;
    const long long abs0 = (long long)((uintptr_t)dst / sizeof(T));     // the tensor's first element as an absolute element address
    for (long long row = blockIdx.y; row < a.rows; row += gridDim.y) {
        // plane p's row begins at absolute element gb[p]; the element j of it sits in LDS at gb[p] + j - lb[p], lb a unit boundary
        long long gb[4], lb[4];
        SVGR_UNROLL
        for (int p = 0; p < 4; ++p) {
            gb[p] = abs0 + a.offset + (long long)p * a.stride_p + row * a.stride_h;
            lb[p] = (gb[p] + jlo) & ~(E - 1);
        }
        // ---- phase 1
        const int n_px = (int)(C1 - clo);
        for (int i = tid; i < n_px; i += TENSOR_LANES) {
            const long long col = clo + i;
            double px[4], y[4];
            tensor_load_px(src, a.src_kind, row, col, a.sb.r0, a.sb.c0, a.sb.rows, a.sb.cols, px);
            const int n = tensor_px(a.op, px[0], px[1], px[2], px[3], y);
            SVGR_UNROLL
            for (int k = 0; k < 4; ++k) {
                if (k >= n) break;
                const T v = (T)tensor_encode(a.op.dtype, y[k]);
                if (Q == 1) lds[k * plane_lds + (int)(gb[k] + col - lb[k])] = v;
                else if (col * Q + k >= jlo) lds[(int)(gb[0] + col * Q + k - lb[0])] = v;
            }
        }
        __syncthreads();
        // ---- phase 2
        for (int p = 0; p < a.planes; ++p) {
            const long long g = p == 0 ? gb[0] : p == 1 ? gb[1] : p == 2 ? gb[2] : gb[3], l = p == 0 ? lb[0] : p == 1 ? lb[1] : p == 2 ? lb[2] : lb[3];
            // this workgroup's share [js, je) of the plane's row: from unit boundary to unit boundary, the row's own ends as they are
            const long long js = C0 == 0 ? 0 : J0 - ((g + J0) & (E - 1)), je = C1 == a.cols ? J1 : J1 - ((g + J1) & (E - 1));
            const int is = (int)(g + js - l), ie = (int)(g + je - l);   // the same in LDS positions
            const T* lp = lds + p * plane_lds;
            T* gp = (T*)(uintptr_t)(l * (long long)sizeof(T));          // LDS position i is the element gp[i]
            for (int u = is / (int)E + tid; u * (int)E < ie; u += TENSOR_LANES) {
                const int i0 = u * (int)E;
                if (i0 >= is && i0 + (int)E <= ie) {
                    *(uint4*)(gp + i0) = *(const uint4*)(lp + i0);
                } else {
                    for (int i = i0 > is ? i0 : is; i < i0 + (int)E && i < ie; ++i) gp[i] = lp[i];
                }
            }
        }
        __syncthreads();   // (the next row writes the same LDS)
    }
}

// the inverse: a lane per pixel (consecutive lanes read consecutive elements of a plane, or consecutive pixels of an interleaved row)
template <class T>
__global__ __launch_bounds__(256) void k_tensor_unpack(double* __restrict__ dst, const T* __restrict__ src, const TensorLaunch a, long long stride_c,
                                                       long long stride_w) {
    const long long col = (long long)blockIdx.x * 256 + threadIdx.x;
    if (col >= a.cols) return;
    for (long long row = blockIdx.y; row < a.rows; row += gridDim.y) {
        double v[4], px[4];
        SVGR_UNROLL
        for (int k = 0; k < 4; ++k)
            if (k < a.n_ch) v[k] = tensor_decode(a.op.dtype, (uint32_t)src[a.offset + k * stride_c + row * a.stride_h + col * stride_w]);
        const int n = tensor_unpack_px(a.op.channels, v, px);
        double* o = dst + (row * a.cols + col) * n;
        if (n == 4) *(double4*)o = make_double4(px[0], px[1], px[2], px[3]);
        else o[0] = px[0];
    }
}

// Everything of a description that can be wrong, and the launch's numbers from it.  `tensor_bytes`: of the buffer on the tensor's
// side, `tensor_ptr` its address.  *empty: nothing to do.
static int tensor_check(const char* entry, const svgr_tensor_desc* d, TensorLaunch& a, long long& stride_c, long long& stride_w, bool& empty) {
    if (!d) return fail(SVGR_E_INVALID, "%s: desc is NULL", entry);
    if (d->source < 0 || d->source >= TENSOR_SRC_KINDS) return fail(SVGR_E_INVALID, "%s: unknown source kind %d", entry, (int)d->source);
    if (d->dtype < 0 || d->dtype >= TENSOR_DTYPES) return fail(SVGR_E_INVALID, "%s: unknown dtype %d", entry, (int)d->dtype);
    if (d->channels < 0 || d->channels >= TENSOR_CHANNEL_KINDS) return fail(SVGR_E_INVALID, "%s: unknown channel selection %d", entry, (int)d->channels);
    if (d->has_bg != 0 && d->has_bg != 1) return fail(SVGR_E_INVALID, "%s: has_bg is 0 or 1", entry);
    constexpr int64_t kMaxSide = 1ll << 30, kMaxStride = 1ll << 40;
    if (d->rows < 0 || d->cols < 0 || d->rows >= kMaxSide || d->cols >= kMaxSide) return fail(SVGR_E_INVALID, "%s: rows and cols are 0 .. 2^30 - 1", entry);
    if (d->stride_c < 0 || d->stride_h < 0 || d->stride_w < 0 || d->offset < 0 || d->stride_c > kMaxStride || d->stride_h > kMaxStride ||
        d->stride_w > kMaxStride || d->offset > (1ll << 50))
        return fail(SVGR_E_INVALID, "%s: a stride or the offset is negative (or beyond 2^40)", entry);
    const int n_ch = tensor_n_channels(d->channels);
    const bool planar = d->stride_w == 1, interleaved = !planar && d->stride_c == 1 && d->stride_w == n_ch;
    if (!planar && !interleaved)
        return fail(SVGR_E_INVALID, "%s: strides (%lld, %lld, %lld) are neither planar (stride_w 1) nor interleaved (stride_c 1, stride_w %d)", entry,
                    (long long)d->stride_c, (long long)d->stride_h, (long long)d->stride_w, n_ch);
    const int per_px = planar ? 1 : n_ch;
    if (d->stride_h < d->cols * per_px) return fail(SVGR_E_INVALID, "%s: stride_h %lld is below the row's %lld elements", entry, (long long)d->stride_h, (long long)(d->cols * per_px));
    for (int k = 0; k < 4; ++k)
        if (!std::isfinite(d->scale[k]) || !std::isfinite(d->bias[k]) || (k < 3 && !std::isfinite(d->bg[k])))
            return fail(SVGR_E_INVALID, "%s: scale, bias and bg must be finite", entry);
    memset(&a, 0, sizeof a);
    a.op.dtype = d->dtype; a.op.channels = d->channels; a.op.has_bg = d->has_bg;
    for (int k = 0; k < 4; ++k) {
        a.op.scale[k] = d->scale[k]; a.op.bias[k] = d->bias[k];
        if (k < n_ch && (d->scale[k] != 1.0 || d->bias[k] != 0.0)) a.op.affine = 1;
        if (k < 3) a.op.bg[k] = d->bg[k];
    }
    a.src_kind = d->source; a.n_ch = n_ch;
    a.planes = planar ? n_ch : 1; a.per_px = per_px;
    a.rows = d->rows; a.cols = d->cols;
    a.stride_p = planar ? d->stride_c : 0; a.stride_h = d->stride_h; a.offset = d->offset;
    stride_c = d->stride_c; stride_w = d->stride_w;
    empty = d->rows == 0 || d->cols == 0;
    return 0;
}
// the tensor's side of either entry: the buffer holds the largest element the description reaches, and its address is an element's
static int tensor_bounds(const char* entry, const svgr_tensor_desc* d, const TensorLaunch& a, const svgr_buf* t) {
    const unsigned es = (unsigned)tensor_elem_bytes(d->dtype);
    const unsigned __int128 last = (unsigned __int128)d->offset + (unsigned __int128)(a.planes - 1) * (unsigned __int128)a.stride_p +
                                   (unsigned __int128)(d->rows - 1) * (unsigned __int128)d->stride_h + (unsigned __int128)(d->cols * a.per_px - 1);
    if ((last + 1) * es > (unsigned __int128)t->bytes)
        return fail(SVGR_E_INVALID, "%s: the largest element index %llu reaches past the tensor's %zu bytes (%u per element)", entry,
                    (unsigned long long)last, t->bytes, es);
    if ((uintptr_t)t->ptr % es) return fail(SVGR_E_INVALID, "%s: the tensor's address is no multiple of its element size", entry);
    return 0;
}

extern "C" {
int svgr_tensor_block(void) { return TENSOR_BLOCK; }
int svgr_tensor_run(void) { return TENSOR_RUN; }

int svgr_layer_to_tensor(svgr_ctx* ctx, const svgr_tensor_desc* desc, const svgr_buf* src, const int64_t* src_bbox, svgr_buf* dst) {
    static const char* entry = "svgr_layer_to_tensor";
    TensorLaunch a;
    long long sc, sw;
    bool empty;
    if (int rc = tensor_check(entry, desc, a, sc, sw, empty)) return rc;
    if (empty) return 0;
    if (!src || !dst || !box_of(src_bbox, a.sb)) return fail(SVGR_E_INVALID, "%s: bad arguments", entry);
    if (int rc = tensor_bounds(entry, desc, a, dst)) return rc;
    const size_t px_bytes = desc->source == TENSOR_SRC_RGBA_F64 ? 32 : desc->source == TENSOR_SRC_RGBA_F32 ? 16 : 8;
    if (src->bytes < box_px(a.sb) * px_bytes) return fail(SVGR_E_INVALID, "%s: the source buffer is too small for its box", entry);
    if (!ctx) return fail(SVGR_E_INVALID, "%s: ctx is NULL", entry);
    const dim3 grid((unsigned)((a.cols + TENSOR_BLOCK - 1) / TENSOR_BLOCK), (unsigned)std::min<long long>(a.rows, 65535));
    switch (tensor_elem_bytes(desc->dtype)) {
        case 4: return launch_tail(ctx, k_tensor_pack<uint32_t>, grid, dim3(TENSOR_LANES), 0, (uint32_t*)dst->ptr, (const void*)src->ptr, a);
        case 2: return launch_tail(ctx, k_tensor_pack<uint16_t>, grid, dim3(TENSOR_LANES), 0, (uint16_t*)dst->ptr, (const void*)src->ptr, a);
        default: return launch_tail(ctx, k_tensor_pack<uint8_t>, grid, dim3(TENSOR_LANES), 0, (uint8_t*)dst->ptr, (const void*)src->ptr, a);
    }
}

int svgr_tensor_to_layer(svgr_ctx* ctx, const svgr_tensor_desc* desc, const svgr_buf* src, svgr_buf* dst_f64) {
    static const char* entry = "svgr_tensor_to_layer";
    TensorLaunch a;
    long long sc, sw;
    bool empty;
    if (int rc = tensor_check(entry, desc, a, sc, sw, empty)) return rc;
    if (empty) return 0;
    if (!src || !dst_f64) return fail(SVGR_E_INVALID, "%s: bad arguments", entry);
    if (int rc = tensor_bounds(entry, desc, a, src)) return rc;
    const size_t out_ch = desc->channels == TENSOR_RGBA || desc->channels == TENSOR_RGB ? 4 : 1;
    if (dst_f64->bytes < (size_t)desc->rows * (size_t)desc->cols * out_ch * 8) return fail(SVGR_E_INVALID, "%s: the layer buffer is too small", entry);
    if (!ctx) return fail(SVGR_E_INVALID, "%s: ctx is NULL", entry);
    const dim3 grid((unsigned)((a.cols + 255) / 256), (unsigned)std::min<long long>(a.rows, 65535));
    switch (tensor_elem_bytes(desc->dtype)) {
        case 4: return launch_tail(ctx, k_tensor_unpack<uint32_t>, grid, dim3(256), 0, (double*)dst_f64->ptr, (const uint32_t*)src->ptr, a, sc, sw);
        case 2: return launch_tail(ctx, k_tensor_unpack<uint16_t>, grid, dim3(256), 0, (double*)dst_f64->ptr, (const uint16_t*)src->ptr, a, sc, sw);
        default: return launch_tail(ctx, k_tensor_unpack<uint8_t>, grid, dim3(256), 0, (double*)dst_f64->ptr, (const uint8_t*)src->ptr, a, sc, sw);
    }
}

// Both through an event of the context's own: recorded on the stream that is waited for, waited for on the other.  (An event
// recorded again while an earlier wait on it is still pending is fine: a wait holds the record it was enqueued behind.)
static int stream_order(svgr_ctx* ctx, int which, hipStream_t first, hipStream_t then) {
    HIPCHK(enter_ctx(ctx));
    if (!ctx->xs_ev[which]) HIPCHK(hipEventCreateWithFlags(&ctx->xs_ev[which], hipEventDisableTiming));
    HIPCHK(hipEventRecord(ctx->xs_ev[which], first));
    HIPCHK(hipStreamWaitEvent(then, ctx->xs_ev[which], 0));
    return 0;
}
int svgr_stream_wait_for(svgr_ctx* ctx, void* other) {
    if (!ctx) return fail(SVGR_E_INVALID, "ctx is NULL");
    if ((hipStream_t)other == ctx->stream) return 0;
    return stream_order(ctx, 0, (hipStream_t)other, ctx->stream);
}
int svgr_stream_signal_to(svgr_ctx* ctx, void* other) {
    if (!ctx) return fail(SVGR_E_INVALID, "ctx is NULL");
    if ((hipStream_t)other == ctx->stream) return 0;
    return stream_order(ctx, 1, ctx->stream, (hipStream_t)other);
}
}  // extern "C"

// ======================================================================================
// Hit testing: winding numbers of points against the batch's paths, and the topmost path under each point
// (svgr_batch_winding, svgr_batch_pick; the arithmetic and its contract: svgr_hit.h)
// ======================================================================================
// The batch's full edge set, grouped by path, on the device (b->hit_*): a counting and an emitting flatten without row culling,
// as svgr_batch_all_edges runs them, but with a counter arena of their own -- the batch's arena, plan and geometry stay as they are.
static int hit_prepare(svgr_batch* b) {
    if (b->hit_ready) return 0;
    hipStream_t st = b->ctx->stream;
    const int ns = (int)b->n_segs, np = (int)b->n_paths;
    if (int rc = b->hit_off.ensure((size_t)np + 1)) return rc;
    if (int rc = b->hit_ext.ensure(4 * (size_t)np)) return rc;
    std::vector<int> off((size_t)np + 1, 0);
    int64_t total = 0;
    PoolBlock d_edges, d_path, scratch, d_cnt;
    if (ns > 0) {
        if (b->arena_bytes == 0)
            if (int rc = b->layout_arena()) return rc;
        HIPCHK(scratch.alloc(b->arena_bytes));
        BatchDev* bd = scratch.as<BatchDev>();
        unsigned long long* pkeys = (unsigned long long*)(scratch.as<unsigned char>() + b->off_pkeys);
        const dim3 fgrid = grid1((size_t)ns << FL_SUB, FL_BLOCK);
        const Owner whole{0, 1, 1};
        HIPCHK(hipMemsetAsync(scratch.p, 0, b->arena_bytes, st));
        SVGR_LAUNCH(k_flatten<false>, fgrid, dim3(FL_BLOCK), 0, st, (const double*)b->segs.p, (const uint8_t*)b->seg_kind.p,
                           (const int*)b->seg_path.p, (const double*)b->path_m6.p, ns, b->thr, (double*)nullptr, (int*)nullptr, b->shards,
                           pkeys, bd, whole, 0, 0, (const unsigned*)nullptr, (const int*)nullptr, 0, (int*)nullptr, (const int*)nullptr, 0, (int*)nullptr, (int*)nullptr, (unsigned long long*)nullptr);
        BatchDev counts;
        HIPCHK(hipMemcpyAsync(&counts, bd, sizeof counts, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (counts.err & 1) return fail(SVGR_E_OVERFLOW, "flatten depth cap (%d) hit: non-finite or absurd control points", kMaxFlattenDepth);
        EdgeShards sh{};
        for (int k = 0; k < NSH; ++k) {
            sh.base[k] = (int)std::min<int64_t>(total, 0x7fffffff);
            sh.cap[k] = counts.shard[k].cursor;
            total += counts.shard[k].cursor;
        }
        if (total > 0x7fffffff / 4) return fail(SVGR_E_OVERFLOW, "%lld edges: beyond the 32-bit edge index", (long long)total);
        if (total > 0) {
            HIPCHK(d_edges.alloc(sizeof(double) * 4 * (size_t)total));
            HIPCHK(d_path.alloc(sizeof(int) * (size_t)total));
            HIPCHK(d_cnt.alloc(sizeof(int) * 2 * ((size_t)np + 1)));
            HIPCHK(hipMemsetAsync(scratch.p, 0, b->arena_bytes, st));
            HIPCHK(hipMemsetAsync(d_path.p, 0xff, sizeof(int) * (size_t)total, st));   // (a slot the flatten should leave empty is no path's)
            HIPCHK(hipMemsetAsync(d_cnt.p, 0, sizeof(int) * 2 * ((size_t)np + 1), st));
            SVGR_LAUNCH(k_flatten<true>, fgrid, dim3(FL_BLOCK), 0, st, (const double*)b->segs.p, (const uint8_t*)b->seg_kind.p,
                               (const int*)b->seg_path.p, (const double*)b->path_m6.p, ns, b->thr, d_edges.as<double>(), d_path.as<int>(), sh, pkeys, bd,
                               whole, 0, 0, (const unsigned*)nullptr, (const int*)nullptr, 0, (int*)nullptr, (const int*)nullptr, 0, (int*)nullptr, (int*)nullptr, (unsigned long long*)nullptr);
            SVGR_LAUNCH(k_hit_count, grid1((size_t)total), dim3(256), 0, st, d_path.as<int>(), (long long)total, np, d_cnt.as<int>());
            std::vector<int> cnt((size_t)np);
            HIPCHK(hipMemcpyAsync(cnt.data(), d_cnt.p, sizeof(int) * (size_t)np, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            for (int p = 0; p < np; ++p) off[(size_t)p + 1] = off[(size_t)p] + cnt[(size_t)p];
        }
    }
    const int64_t kept = off[(size_t)np];
    if (int rc = b->hit_edges.ensure(4 * (size_t)std::max<int64_t>(kept, 1))) return rc;
    HIPCHK(hipMemcpyAsync(b->hit_off.p, off.data(), sizeof(int) * ((size_t)np + 1), hipMemcpyHostToDevice, st));
    if (kept > 0)
        SVGR_LAUNCH(k_hit_place, grid1((size_t)total), dim3(256), 0, st, d_edges.as<double>(), d_path.as<int>(), (long long)total, np,
                    (const int*)b->hit_off.p, d_cnt.as<int>() + np + 1, b->hit_edges.p);
    SVGR_LAUNCH(k_hit_extent, dim3((unsigned)np), dim3(64), 0, st, (const double*)b->hit_edges.p, (const int*)b->hit_off.p, np, b->hit_ext.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));   // (`off` is the source of an upload)
    b->hit_ready = true;
    return 0;
}

// the points of a query: `points` (n x 2 doubles of the caller's) or the grid {row0, col0, rows, cols}; checked, nothing uploaded yet
static int hit_query(const char* entry, const double* points, const int64_t* grid, int64_t n_points, HitQuery& q, long long& n_groups) {
    memset(&q, 0, sizeof q);
    if ((points != nullptr) == (grid != nullptr)) return fail(SVGR_E_INVALID, "%s: give the points or the grid, one of them", entry);
    if (grid) {
        if (grid[2] < 0 || grid[3] < 0 || grid[2] >= (1ll << 30) || grid[3] >= (1ll << 30) || grid[2] * grid[3] != n_points)
            return fail(SVGR_E_INVALID, "%s: the grid's rows x cols are not n_points", entry);
        if (grid[0] < -(1ll << 50) || grid[0] > (1ll << 50) || grid[1] < -(1ll << 50) || grid[1] > (1ll << 50))
            return fail(SVGR_E_INVALID, "%s: the grid's origin is beyond 2^50", entry);
        q.row0 = grid[0]; q.col0 = grid[1]; q.rows = grid[2]; q.cols = grid[3];
        q.tiles_x = std::max<long long>((q.cols + HIT_TILE - 1) / HIT_TILE, 1);
        n_groups = q.tiles_x * ((q.rows + HIT_TILE - 1) / HIT_TILE);
    } else {
        q.n = n_points;
        n_groups = (n_points + HIT_BLOCK - 1) / HIT_BLOCK;
    }
    if (n_groups > 0x7fffffffll) return fail(SVGR_E_OVERFLOW, "%s: %lld points are more than one launch takes", entry, (long long)n_points);
    return 0;
}
static int hit_upload_points(svgr_batch* b, const double* points, int64_t n_points, PoolBlock& dev, HitQuery& q) {
    if (!points || n_points == 0) return 0;
    HIPCHK(dev.alloc(sizeof(double) * 2 * (size_t)n_points));
    HIPCHK(hipMemcpyAsync(dev.p, points, sizeof(double) * 2 * (size_t)n_points, hipMemcpyHostToDevice, b->ctx->stream));
    q.pts = dev.as<double>();
    return 0;
}

// ---- what the two distance entries (svgr_batch_distance, svgr_batch_msdf) share
// the checks of the flags, the encoding (into `enc`) and the spread, in the order the entries report them
static int distance_encoding(const char* entry, int flags, int known_flags, double spread, int& enc) {
    if (flags & ~known_flags) return fail(SVGR_E_INVALID, "%s: unknown flags 0x%x", entry, (unsigned)flags);
    enc = flags & SVGR_SDF_ENCODING_MASK;
    if (enc >= SDF_ENCODINGS) return fail(SVGR_E_INVALID, "%s: unknown encoding %d", entry, enc);
    if (!(spread > 0.0)) return fail(SVGR_E_INVALID, "%s: the spread is +inf or a finite value > 0, not %g", entry, spread);
    if (enc != SDF_F64 && !(spread < INFINITY)) return fail(SVGR_E_INVALID, "%s: the float32 and uint8 encodings need a finite spread", entry);
    return 0;
}
static_assert(SVGR_MSDF_ENCODING_MASK == SVGR_SDF_ENCODING_MASK && SVGR_MSDF_F64 == SDF_F64 && SVGR_MSDF_F32 == SDF_F32 && SVGR_MSDF_U8 == SDF_U8,
              "the two entries name the same encodings");
// the encoding as a compile-time value: `launch(std::integral_constant<int, SDF_*>{})`
template <class F>
static void with_sdf_encoding(int enc, F&& launch) {
    if (enc == SDF_F64) launch(std::integral_constant<int, SDF_F64>{});
    else if (enc == SDF_F32) launch(std::integral_constant<int, SDF_F32>{});
    else launch(std::integral_constant<int, SDF_U8>{});
}
// what a query without paths answers, on the host: +spread in every one of `n` elements of the caller's
static int distance_fill_spread(void* out, int64_t n, int enc, double spread) {
    for (int64_t i = 0; i < n; ++i) {
        if (enc == SDF_F64) ((double*)out)[i] = spread;
        else if (enc == SDF_F32) ((float*)out)[i] = sdf_encode_f32(spread, spread);
        else ((uint8_t*)out)[i] = sdf_encode_u8(spread, spread);
    }
    return 0;
}
// the spread the kernels cull with (sdf_out_of_reach): none for an infinite spread and for one below 2^-100
static double distance_cull_spread(double spread) { return (spread < INFINITY && spread >= 0x1p-100) ? spread : (double)INFINITY; }
// The points go through in passes of whole workgroups -- of whole rows of tiles for a grid, so that a pass is a contiguous run
// of the caller's row-major order -- as many at a time as the scratch holds: `launch(first workgroup, workgroups, first point)`
// enqueues a pass that writes `point_bytes` per point into `d_out` (the entry's own block, allocated here), and the run is
// copied out behind it.  Returns behind the wait for the last copy.
template <class Launch>
static int distance_passes(svgr_batch* b, const HitQuery& q, bool grid, long long n_wgs, int64_t n_points, size_t point_bytes, size_t scratch_bytes,
                           PoolBlock& d_out, void* out, Launch&& launch) {
    hipStream_t st = b->ctx->stream;
    // a pass unit: a workgroup's points, or a row of tiles of a grid
    const long long unit_groups = grid ? q.tiles_x : 1, unit_points = grid ? HIT_TILE * q.cols : HIT_BLOCK;
    const long long n_units = n_wgs / unit_groups;
    const size_t budget = scratch_bytes ? scratch_bytes : (size_t)256 << 20;
    const long long per_pass = std::min<long long>(n_units, std::max<long long>((long long)(budget / (point_bytes * (size_t)unit_points)), 1));
    const long long pass_points = std::min<long long>(n_points, per_pass * unit_points);
    HIPCHK(d_out.alloc(point_bytes * (size_t)pass_points));
    for (long long u0 = 0; u0 < n_units; u0 += per_pass) {
        const long long nu = std::min<long long>(per_pass, n_units - u0);
        const long long i0 = u0 * unit_points, i1 = std::min<long long>(n_points, (u0 + nu) * unit_points);
        launch(u0 * unit_groups, nu * unit_groups, i0);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync((unsigned char*)out + point_bytes * (size_t)i0, d_out.p, point_bytes * (size_t)(i1 - i0), hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    return 0;
}

extern "C" {
int svgr_hit_block(void) { return HIT_BLOCK; }
int svgr_hit_chunk(void) { return HIT_CHUNK; }

int svgr_batch_winding(svgr_batch* b, const double* points, const int64_t* grid, int64_t n_points, int32_t* winding_out) {
    static const char* entry = "svgr_batch_winding";
    return abi_guard(entry, [&]() -> int {
        if (!b || n_points < 0) return fail(SVGR_E_INVALID, "%s: bad arguments", entry);
        PoolBlock d_pts, d_out;
        HitQuery q;
        long long n_groups = 0;
        if (int rc = hit_query(entry, points, grid, n_points, q, n_groups)) return rc;
        const int64_t np = b->n_paths;
        if (np == 0 || n_points == 0) return 0;
        if (n_points > 0x7fffffffll / np) return fail(SVGR_E_OVERFLOW, "%s: %lld points x %lld paths leave 31 bits", entry, (long long)n_points, (long long)np);
        if (!winding_out) return fail(SVGR_E_INVALID, "%s: winding_out is NULL", entry);
        HIPCHK(enter_ctx(b->ctx));
        hipStream_t st = b->ctx->stream;
        if (int rc = hit_prepare(b)) return rc;
        if (int rc = hit_upload_points(b, points, n_points, d_pts, q)) return rc;
        const size_t bytes = sizeof(int32_t) * (size_t)n_points * (size_t)np;
        HIPCHK(d_out.alloc(bytes));
        SVGR_LAUNCH(k_hit_winding<false>, dim3((unsigned)n_groups), dim3(HIT_BLOCK), 0, st, (const double*)b->hit_edges.p, (const int*)b->hit_off.p,
                    (const double*)b->hit_ext.p, (const uint8_t*)b->path_rule.p, (int)np, q, 0ll, d_out.as<int>(), (uint32_t*)nullptr, 0);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(winding_out, d_out.p, bytes, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        return 0;
    });
}

int svgr_batch_pick(svgr_batch* b, const double* points, const int64_t* grid, int64_t n_points, const uint8_t* pickable, const int32_t* clip_off,
                    const int32_t* clip_group, const int32_t* group_off, const int32_t* group_src, int64_t n_clip_groups, size_t scratch_bytes,
                    int32_t* top_out, uint32_t* bits_out) {
    static const char* entry = "svgr_batch_pick";
    return abi_guard(entry, [&]() -> int {
        if (!b || n_points < 0 || n_clip_groups < 0 || n_clip_groups > 0x7fffffffll) return fail(SVGR_E_INVALID, "%s: bad arguments", entry);
        PoolBlock d_pts, d_top, d_bits;
        HitQuery q;
        long long n_groups = 0;
        if (int rc = hit_query(entry, points, grid, n_points, q, n_groups)) return rc;
        const int64_t np = b->n_paths;
        if (n_points > 0 && !top_out) return fail(SVGR_E_INVALID, "%s: top_out is NULL", entry);
        if (np == 0) {
            for (int64_t i = 0; i < n_points; ++i) top_out[i] = -1;
            return 0;
        }
        if (!pickable || !clip_off) return fail(SVGR_E_INVALID, "%s: pickable or clip_off is NULL", entry);
        if (n_clip_groups > 0 && (!group_off || (group_off[n_clip_groups] > 0 && !group_src))) return fail(SVGR_E_INVALID, "%s: the clip groups' tables are NULL", entry);
        if (clip_off[np] > 0 && !clip_group) return fail(SVGR_E_INVALID, "%s: clip_group is NULL", entry);
        if (clip_off[np] > 0 && n_clip_groups == 0) return fail(SVGR_E_INVALID, "%s: clip groups are used and none is given", entry);
        if (const long long bad = hit_check_tables(np, clip_off, clip_group, group_off, group_src, n_clip_groups))
            return fail(SVGR_E_INVALID, "%s: the clip tables of path %lld: offsets must ascend from 0, a group must exist, and every clip source must lie in front of the path that uses it",
                        entry, bad - 1);
        if (n_points == 0) return 0;
        const int words = (int)((np + 31) / 32);
        if ((size_t)n_points > SIZE_MAX / 8 / (size_t)words) return fail(SVGR_E_OVERFLOW, "%s: the bit matrix leaves the address space", entry);
        HIPCHK(enter_ctx(b->ctx));
        hipStream_t st = b->ctx->stream;
        if (int rc = hit_prepare(b)) return rc;
        if (int rc = hit_upload_points(b, points, n_points, d_pts, q)) return rc;
        // the tables in one upload: the four int arrays, then the pickable bytes.  (`staged` is declared in front of the frame:
        // the frame's drain waits for the copies into it on every way out)
        std::vector<uint32_t> staged;   // a grid's rows come back in tile order: put in row-major order behind the wait
        PassFrame f(b->ctx);
        const int32_t zero = 0;
        const Section<int32_t> s_co = f.blob.put(clip_off, (size_t)np + 1), s_cg = f.blob.put(clip_group, (size_t)clip_off[np]);
        const Section<int32_t> s_go = n_clip_groups > 0 ? f.blob.put(group_off, (size_t)n_clip_groups + 1) : f.blob.put(&zero, 1);
        const Section<int32_t> s_gs = f.blob.put(group_src, n_clip_groups > 0 ? (size_t)group_off[n_clip_groups] : 0);
        const Section<uint8_t> s_pick = f.blob.put(pickable, (size_t)np);
        if (int rc = f.upload()) return rc;
        const void* d_tab = f.in.p;
        const int32_t *t_co = s_co.on(d_tab), *t_cg = s_cg.on(d_tab), *t_go = s_go.on(d_tab), *t_gs = s_gs.on(d_tab);
        const uint8_t* t_pick = s_pick.on(d_tab);
        // the point-by-path bit matrix: as many workgroups' rows at a time as the scratch holds
        const size_t group_bytes = sizeof(uint32_t) * (size_t)words * HIT_BLOCK;
        const size_t budget = scratch_bytes ? scratch_bytes : (size_t)256 << 20;
        const long long per_pass = std::min<long long>(n_groups, std::max<long long>((long long)(budget / group_bytes), 1));
        HIPCHK(d_bits.alloc(group_bytes * (size_t)per_pass));
        HIPCHK(d_top.alloc(sizeof(int32_t) * (size_t)n_points));
        if (bits_out && grid) staged.resize((size_t)n_groups * HIT_BLOCK * (size_t)words);
        for (long long g0 = 0; g0 < n_groups; g0 += per_pass) {
            const long long ng = std::min<long long>(per_pass, n_groups - g0);
            SVGR_LAUNCH(k_hit_winding<true>, dim3((unsigned)ng), dim3(HIT_BLOCK), 0, st, (const double*)b->hit_edges.p, (const int*)b->hit_off.p,
                        (const double*)b->hit_ext.p, (const uint8_t*)b->path_rule.p, (int)np, q, g0, (int*)nullptr, d_bits.as<uint32_t>(), words);
            SVGR_LAUNCH(k_hit_resolve, dim3((unsigned)ng), dim3(HIT_BLOCK), 0, st, d_bits.as<uint32_t>(), words, (int)np, q, g0, t_pick, t_co,
                        t_cg, t_go, t_gs, d_top.as<int32_t>());
            HIPCHK(hipGetLastError());
            if (bits_out && grid) {
                HIPCHK(hipMemcpyAsync(staged.data() + (size_t)g0 * HIT_BLOCK * (size_t)words, d_bits.p, group_bytes * (size_t)ng, hipMemcpyDeviceToHost, st));
            } else if (bits_out) {
                const long long i0 = g0 * HIT_BLOCK, i1 = std::min<long long>(n_points, (g0 + ng) * HIT_BLOCK);
                HIPCHK(hipMemcpyAsync(bits_out + (size_t)i0 * (size_t)words, d_bits.p, sizeof(uint32_t) * (size_t)words * (size_t)(i1 - i0), hipMemcpyDeviceToHost, st));
            }
        }
        HIPCHK(hipMemcpyAsync(top_out, d_top.p, sizeof(int32_t) * (size_t)n_points, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (bits_out && grid)
            for (long long g = 0; g < n_groups; ++g)
                for (int lane = 0; lane < HIT_BLOCK; ++lane) {
                    const long long r = (g / q.tiles_x) * HIT_TILE + lane / HIT_TILE, c = (g % q.tiles_x) * HIT_TILE + lane % HIT_TILE;
                    if (r >= q.rows || c >= q.cols) continue;
                    memcpy(bits_out + (size_t)(r * q.cols + c) * (size_t)words, staged.data() + ((size_t)g * HIT_BLOCK + (size_t)lane) * (size_t)words,
                           sizeof(uint32_t) * (size_t)words);
                }
        return 0;
    });
}

// Signed distance fields (the arithmetic and its contract: svgr_sdf.h).
int svgr_batch_distance(svgr_batch* b, const double* points, const int64_t* grid, int64_t n_points, double spread, int flags, size_t scratch_bytes,
                        void* out) {
    static const char* entry = "svgr_batch_distance";
    return abi_guard(entry, [&]() -> int {
        if (!b || n_points < 0) return fail(SVGR_E_INVALID, "%s: bad arguments", entry);
        int enc = 0;
        if (int rc = distance_encoding(entry, flags, SVGR_SDF_ENCODING_MASK | SVGR_SDF_UNION | SVGR_SDF_UNSIGNED, spread, enc)) return rc;
        PoolBlock d_pts, d_out;
        HitQuery q;
        long long n_wgs = 0;
        if (int rc = hit_query(entry, points, grid, n_points, q, n_wgs)) return rc;
        const int64_t np = b->n_paths;
        const bool uni = (flags & SVGR_SDF_UNION) != 0;
        if (n_points == 0 || (np == 0 && !uni)) return 0;
        if (!uni && n_points > 0x7fffffffll / np) return fail(SVGR_E_OVERFLOW, "%s: %lld points x %lld paths leave 31 bits", entry, (long long)n_points, (long long)np);
        if (!out) return fail(SVGR_E_INVALID, "%s: out is NULL", entry);
        if (np == 0) return distance_fill_spread(out, n_points, enc, spread);   // a union over no paths
        HIPCHK(enter_ctx(b->ctx));
        hipStream_t st = b->ctx->stream;
        if (int rc = hit_prepare(b)) return rc;
        if (int rc = hit_upload_points(b, points, n_points, d_pts, q)) return rc;
        const double cull_spread = distance_cull_spread(spread);
        const int is_signed = (flags & SVGR_SDF_UNSIGNED) ? 0 : 1;
        const size_t point_bytes = (size_t)sdf_elem_bytes(enc) * (uni ? 1 : (size_t)np);
        return distance_passes(b, q, grid != nullptr, n_wgs, n_points, point_bytes, scratch_bytes, d_out, out, [&](long long wg0, long long wgs, long long i0) {
            with_sdf_encoding(enc, [&](auto e) {
                auto launch = [&](auto kernel) {
                    SVGR_LAUNCH(kernel, dim3((unsigned)wgs), dim3(HIT_BLOCK), 0, st, (const double*)b->hit_edges.p, (const int*)b->hit_off.p,
                                (const double*)b->hit_ext.p, (const uint8_t*)b->path_rule.p, (int)np, q, wg0, i0, spread, cull_spread, is_signed, d_out.p);
                };
                if (uni) launch(k_sdf_distance<decltype(e)::value, true>);
                else launch(k_sdf_distance<decltype(e)::value, false>);
            });
        });
    });
}

// Multi-channel distance fields (the arithmetic and its contract: svgr_msdf.h): four values to a point, and the
// groups' tables in one upload.
int svgr_batch_msdf(svgr_batch* b, const double* points, const int64_t* grid, int64_t n_points, double spread, int flags, const uint8_t* colour,
                    const int32_t* group_off, const int8_t* orient, int64_t n_groups, size_t scratch_bytes, void* out) {
    static const char* entry = "svgr_batch_msdf";
    return abi_guard(entry, [&]() -> int {
        if (!b || n_points < 0 || n_groups < 0 || n_groups > 0x7fffffffll) return fail(SVGR_E_INVALID, "%s: bad arguments", entry);
        int enc = 0;
        if (int rc = distance_encoding(entry, flags, SVGR_MSDF_ENCODING_MASK, spread, enc)) return rc;
        PoolBlock d_pts, d_out;
        HitQuery q;
        long long n_wgs = 0;
        if (int rc = hit_query(entry, points, grid, n_points, q, n_wgs)) return rc;
        const int64_t np = b->n_paths;
        if (!colour || (n_groups > 0 && (!group_off || !orient))) return fail(SVGR_E_INVALID, "%s: colour, group_off or orient is NULL", entry);
        for (int64_t p = 0; p < np; ++p)
            if (colour[p] < 1 || colour[p] > 7) return fail(SVGR_E_INVALID, "%s: the colour of path %lld is a mask 1 .. 7, not %d", entry, (long long)p, (int)colour[p]);
        if (n_groups > 0 && group_off[0] != 0) return fail(SVGR_E_INVALID, "%s: group_off begins at 0", entry);
        for (int64_t g = 0; g < n_groups; ++g)
            if (group_off[g + 1] < group_off[g] || group_off[g + 1] > np)
                return fail(SVGR_E_INVALID, "%s: group_off ascends and ends within the batch's %lld paths (group %lld)", entry, (long long)np, (long long)g);
        for (int64_t g = 0; g < n_groups; ++g) {
            if (orient[g] != 1 && orient[g] != -1) return fail(SVGR_E_INVALID, "%s: the orient of group %lld is +1 or -1, not %d", entry, (long long)g, (int)orient[g]);
            for (int32_t p = group_off[g] + 1; p < group_off[g + 1]; ++p)
                if ((b->host_rule[(size_t)p] & 1) != (b->host_rule[(size_t)group_off[g]] & 1))
                    return fail(SVGR_E_INVALID, "%s: the paths of group %lld differ in fill rule", entry, (long long)g);
        }
        if (n_points == 0) return 0;
        if (!out) return fail(SVGR_E_INVALID, "%s: out is NULL", entry);
        const int used = n_groups > 0 ? group_off[n_groups] : 0;   // the paths the groups cover: 0 .. used
        if (used == 0) return distance_fill_spread(out, 4 * n_points, enc, spread);   // no group, or none with a path
        // per path of the groups: its colour and its group's marks, and its group
        std::vector<uint8_t> info((size_t)used);
        std::vector<int32_t> owner((size_t)used);
        for (int64_t g = 0; g < n_groups; ++g)
            for (int32_t p = group_off[g]; p < group_off[g + 1]; ++p) {
                info[(size_t)p] = (uint8_t)(colour[p] | (p == group_off[g + 1] - 1 ? MSDF_PATH_LAST : 0) | (orient[g] < 0 ? MSDF_PATH_NEGATIVE : 0) |
                                            ((b->host_rule[(size_t)p] & 1) ? MSDF_PATH_EVENODD : 0));
                owner[(size_t)p] = (int32_t)g;
            }
        HIPCHK(enter_ctx(b->ctx));
        hipStream_t st = b->ctx->stream;
        if (int rc = hit_prepare(b)) return rc;
        if (int rc = hit_upload_points(b, points, n_points, d_pts, q)) return rc;
        PassFrame f(b->ctx);
        const Section<int32_t> s_go = f.blob.put(group_off, (size_t)n_groups + 1), s_own = f.blob.put(owner.data(), owner.size());
        const Section<uint8_t> s_info = f.blob.put(info.data(), info.size());
        if (int rc = f.upload()) return rc;
        double* gext = f.scratch<double>(4 * (size_t)n_groups);
        if (f.err) return f.err;
        SVGR_LAUNCH(k_msdf_group_extent, grid1((size_t)n_groups), dim3(256), 0, st, (const double*)b->hit_ext.p, (const int32_t*)s_go.on(f.in.p), (int)n_groups, gext);
        const double cull_spread = distance_cull_spread(spread);
        return distance_passes(b, q, grid != nullptr, n_wgs, n_points, 4 * (size_t)sdf_elem_bytes(enc), scratch_bytes, d_out, out,
                               [&](long long wg0, long long wgs, long long i0) {
                                   with_sdf_encoding(enc, [&](auto e) {
                                       SVGR_LAUNCH((k_msdf_distance<decltype(e)::value>), dim3((unsigned)wgs), dim3(HIT_BLOCK), 0, st, (const double*)b->hit_edges.p,
                                                   (const int*)b->hit_off.p, (const double*)gext, (const uint8_t*)s_info.on(f.in.p),
                                                   (const int32_t*)s_own.on(f.in.p), used, q, wg0, i0, spread, cull_spread, d_out.p);
                                   });
                               });
    });
}
}  // extern "C"

// ======================================================================================
// Indexed PNG output: the colour quantiser's device stages (svgr_quant_distinct, svgr_quant_bins, svgr_quant_index).  The
// per-lane arithmetic is svgr_quant.h; DESIGN.md 7t has the definitions and the palette builder, which runs on the host over
// the bins.  A lane takes QUANT_RUN consecutive pixels, a workgroup QUANT_BLOCK: flat art repeats its pixels, and a lane that
// meets the pixel it has just had does no work for it.
//
//   k_quant_distinct  an open-addressed set of QUANT_SLOTS words in memory: a lane reads the slot (most pixels find their colour
//                     there), and only an empty one is claimed with a compare-and-swap, which also counts.  A slot changes once,
//                     from empty to a colour, so a stale read costs a swap that fails and nothing else.  Lanes stop once the
//                     count is past max_colors; the set itself is the result, and no order of arrival changes a set
//   k_quant_bins      per lane the run's pixels of one bin summed in registers; a wave whose lanes all end in the same bin adds
//                     them up with shuffles and one lane sends the five adds -- to a small table of bins in LDS, which the
//                     workgroup, striding over many blocks, sends to memory once at its end: the few bins of flat art would
//                     otherwise take every wave's adds at the same five addresses.  Integer adds only
//   k_quant_flag / k_scan_* / k_quant_compact   the dasher's two-level scan over "bin is not empty": the bins in key order
//   k_quant_index     the palette's coordinates in LDS (every lane reads the same entry at the same time: a broadcast), per
//                     pixel the nearest entry, the run's indices packed to `depth` bytes and stored
// ======================================================================================
#include "svgr_quant.h"

constexpr int QUANT_LANES = 256, QUANT_BLOCK = QUANT_LANES * QUANT_RUN;
// (a section of its own, like the marker kernels': the tile kernel's branches to its cold paths keep their reach)
#define QUANT_KERNEL __global__ __launch_bounds__(QUANT_LANES) __attribute__((section(".text.svgr_quant")))
struct QuantSet { uint32_t slot[QUANT_SLOTS]; uint32_t count, full; };
struct QuantSumOp {
    __device__ static int zero() { return 0; }
    __device__ static int add(const int& a, const int& b) { return a + b; }
};

// the lane's run: pixels i0 .. i0 + n - 1 (i0 is a multiple of QUANT_RUN; 0 <= n <= QUANT_RUN)
__device__ __forceinline__ int quant_load_run(const uint32_t* __restrict__ src, long long n_px, long long i0, uint32_t* px) {
    const long long left = n_px - i0;
    const int n = left >= QUANT_RUN ? QUANT_RUN : left > 0 ? (int)left : 0;
    if (n == QUANT_RUN && ((uintptr_t)src & 15) == 0) {
        const uint4 lo = *(const uint4*)(src + i0), hi = *(const uint4*)(src + i0 + 4);
        px[0] = lo.x; px[1] = lo.y; px[2] = lo.z; px[3] = lo.w; px[4] = hi.x; px[5] = hi.y; px[6] = hi.z; px[7] = hi.w;
    } else {
        SVGR_UNROLL
        for (int k = 0; k < QUANT_RUN; ++k) px[k] = k < n ? src[i0 + k] : 0u;
    }
    return n;
}

QUANT_KERNEL void k_quant_distinct(const uint32_t* __restrict__ src, long long n_px, uint32_t max_colors, QuantSet* set) {
    const long long i0 = ((long long)blockIdx.x * QUANT_LANES + threadIdx.x) * QUANT_RUN;
    uint32_t px[QUANT_RUN];
    const int n = quant_load_run(src, n_px, i0, px);
    uint32_t prev = QUANT_EMPTY;
    for (int k = 0; k < n; ++k) {
        const uint32_t c = quant_canon(px[k]);
        if (c == prev) continue;
        prev = c;
        if (__hip_atomic_load(&set->count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > max_colors) return;
        uint32_t s = quant_slot(c), probes = 0;
        for (; probes < QUANT_SLOTS; ++probes, s = (s + 1) & (QUANT_SLOTS - 1)) {
            uint32_t cur = set->slot[s];
            if (cur == QUANT_EMPTY) {
                cur = atomicCAS(&set->slot[s], QUANT_EMPTY, c);
                if (cur == QUANT_EMPTY) {
                    atomicAdd(&set->count, 1u);
                    break;
                }
            }
            if (cur == c) break;
        }
        if (probes == QUANT_SLOTS) atomicOr(&set->full, 1u);   // (every slot holds another colour: more than max_colors of them)
    }
}

// At most QUANT_GROUPS workgroups stride over the image's blocks; each keeps QUANT_CACHE bins in LDS (claimed by compare-and-swap,
// QUANT_PROBES slots tried) and sends them to memory once, at its end; a bin that finds no slot goes to memory directly.
constexpr int QUANT_GROUPS = 1024, QUANT_CACHE = QUANT_LANES, QUANT_PROBES = 4;
QUANT_KERNEL void k_quant_bins(const uint32_t* __restrict__ src, long long n_px, long long n_blocks, QuantBin* __restrict__ hist) {
    __shared__ uint32_t ckey[QUANT_CACHE];
    __shared__ unsigned long long csum[QUANT_CACHE][5];
    ckey[threadIdx.x] = 0xFFFFFFFFu;
    SVGR_UNROLL
    for (int j = 0; j < 5; ++j) csum[threadIdx.x][j] = 0;
    __syncthreads();
    uint32_t key, cnt, s[4];   // (a run's sums: 8 * 65025 at the most)
    auto flush = [&]() {
        if (!cnt) return;
        uint32_t slot = (key * 2654435761u) >> 24;
        static_assert(QUANT_CACHE == 256, "the slot is the hash's top eight bits");
        for (int p = 0; p < QUANT_PROBES; ++p, slot = (slot + 1) & (QUANT_CACHE - 1)) {
            const uint32_t old = atomicCAS(&ckey[slot], 0xFFFFFFFFu, key);
            if (old == 0xFFFFFFFFu || old == key) {
                atomicAdd(&csum[slot][0], (unsigned long long)cnt);
                SVGR_UNROLL
                for (int j = 0; j < 4; ++j) atomicAdd(&csum[slot][1 + j], (unsigned long long)s[j]);
                return;
            }
        }
        unsigned long long* b = (unsigned long long*)&hist[key];
        atomicAdd(b, (unsigned long long)cnt);
        SVGR_UNROLL
        for (int j = 0; j < 4; ++j) atomicAdd(b + 1 + j, (unsigned long long)s[j]);
    };
    for (long long blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const long long i0 = (blk * QUANT_LANES + threadIdx.x) * QUANT_RUN;
        uint32_t px[QUANT_RUN];
        const int n = quant_load_run(src, n_px, i0, px);
        key = 0xFFFFFFFFu;
        cnt = s[0] = s[1] = s[2] = s[3] = 0;
        for (int k = 0; k < n; ++k) {
            const uint32_t c = quant_canon(px[k]), kk = quant_bin_key(c);
            if (kk != key) {
                flush();
                key = kk;
                cnt = s[0] = s[1] = s[2] = s[3] = 0;
            }
            uint32_t x[4];
            quant_x(c, x);
            ++cnt;
            SVGR_UNROLL
            for (int j = 0; j < 4; ++j) s[j] += x[j];
        }
        // what is left: one bin for the whole wave (a wave's sums: 512 * 65025 at the most), or each lane for itself
        if (__all(key == (uint32_t)__builtin_amdgcn_readfirstlane((int)key))) {
            for (int d = 32; d; d >>= 1) {
                cnt += __shfl_down(cnt, d, 64);
                SVGR_UNROLL
                for (int j = 0; j < 4; ++j) s[j] += __shfl_down(s[j], d, 64);
            }
            if ((threadIdx.x & 63) == 0) flush();
        } else {
            flush();
        }
    }
    __syncthreads();
    const uint32_t mine = ckey[threadIdx.x];
    if (mine != 0xFFFFFFFFu) {
        unsigned long long* b = (unsigned long long*)&hist[mine];
        SVGR_UNROLL
        for (int j = 0; j < 5; ++j)
            if (csum[threadIdx.x][j]) atomicAdd(b + j, csum[threadIdx.x][j]);
    }
}

QUANT_KERNEL void k_quant_flag(const QuantBin* __restrict__ hist, int* __restrict__ flag) {
    const uint32_t i = blockIdx.x * QUANT_LANES + threadIdx.x;
    if (i < QUANT_BINS) flag[i] = hist[i].n != 0;
}
QUANT_KERNEL void k_quant_compact(const QuantBin* __restrict__ hist, const int* __restrict__ incl, int n_out, uint32_t* __restrict__ keys,
                                  QuantBin* __restrict__ out) {
    const uint32_t i = blockIdx.x * QUANT_LANES + threadIdx.x;
    if (i >= QUANT_BINS) return;
    const QuantBin b = hist[i];
    if (!b.n) return;
    const int pos = incl[i] - 1;
    if (pos < 0 || pos >= n_out) return;
    keys[pos] = i;
    out[pos] = b;
}

QUANT_KERNEL void k_quant_index(const uint32_t* __restrict__ src, int rows, int cols, const uint32_t* __restrict__ pal, int n_pal, int depth,
                                uint8_t* __restrict__ stream, uint8_t* __restrict__ indices) {
    __shared__ uint32_t pal_x[4 * QUANT_MAX_COLORS];
    if ((int)threadIdx.x < n_pal) quant_x(quant_canon(pal[threadIdx.x]), pal_x + 4 * threadIdx.x);
    __syncthreads();
    const long long c0 = ((long long)blockIdx.x * QUANT_LANES + threadIdx.x) * QUANT_RUN;
    if (c0 >= cols) return;
    const int n = cols - c0 >= QUANT_RUN ? QUANT_RUN : (int)(cols - c0);
    const long long rb = quant_row_bytes(cols, depth);
    for (long long row = blockIdx.y; row < rows; row += gridDim.y) {
        const uint32_t* p = src + row * cols + c0;
        uint8_t idx[QUANT_RUN], bytes[QUANT_RUN];
        uint32_t prev = 0;
        SVGR_UNROLL
        for (int k = 0; k < QUANT_RUN; ++k) {
            idx[k] = 0;
            if (k < n) {
                const uint32_t c = quant_canon(p[k]);
                if (k && c == prev) {
                    idx[k] = idx[k - 1];
                } else {
                    uint32_t x[4];
                    quant_x(c, x);
                    idx[k] = (uint8_t)quant_nearest(pal_x, n_pal, x);
                }
                prev = c;
            }
        }
        if (indices) {
            SVGR_UNROLL
            for (int k = 0; k < QUANT_RUN; ++k)
                if (k < n) indices[row * cols + c0 + k] = idx[k];
        }
        if (stream) {
            uint8_t* o = stream + row * rb;
            if (c0 == 0) o[0] = 0;
            quant_pack_run(idx, n, depth, bytes);
            const int nb = (n * depth + 7) / 8;
            o += 1 + c0 * depth / 8;
            SVGR_UNROLL
            for (int j = 0; j < QUANT_RUN; ++j)
                if (j < nb) o[j] = bytes[j];
        }
    }
}

// Widths: a bin's count is at most 2^30 and a sum at most 2^30 * 65025 < 2^46 at the largest image image_size_ok lets in (2^30
// pixels, 2^16 a side): the 64-bit fields cannot overflow.
static int quant_check(const char* entry, svgr_ctx* ctx, const svgr_buf* src, int64_t rows, int64_t cols) {
    if (!ctx || !src) return fail(SVGR_E_INVALID, "%s: bad arguments", entry);
    if (!image_size_ok(rows, cols)) return fail(SVGR_E_INVALID, "%s: %lld x %lld is empty or beyond 2^16 a side, 2^30 pixels", entry, (long long)rows, (long long)cols);
    if (src->bytes < (size_t)rows * cols * 4) return fail(SVGR_E_INVALID, "%s: buffer too small", entry);
    return 0;
}

static int quant_distinct_impl(svgr_ctx* ctx, const svgr_buf* src, int64_t rows, int64_t cols, int max_colors, uint32_t* colors, int64_t* n_colors, int* overflow) {
    static const char* entry = "svgr_quant_distinct";
    if (int rc = quant_check(entry, ctx, src, rows, cols)) return rc;
    if (!colors || !n_colors || !overflow) return fail(SVGR_E_INVALID, "%s: bad arguments", entry);
    if (max_colors < 1 || max_colors > QUANT_MAX_COLORS) return fail(SVGR_E_INVALID, "%s: max_colors is 1 .. %d, not %d", entry, QUANT_MAX_COLORS, max_colors);
    std::vector<QuantSet> host(1);
    PassFrame f(ctx);
    HIPCHK(enter_ctx(ctx));
    QuantSet* set = f.scratch<QuantSet>(1);
    if (f.err) return f.err;
    HIPCHK(hipMemsetD32Async((hipDeviceptr_t)set->slot, (int)QUANT_EMPTY, QUANT_SLOTS, f.st));
    HIPCHK(hipMemsetAsync(&set->count, 0, 8, f.st));
    const long long n_px = (long long)rows * cols;
    SVGR_LAUNCH(k_quant_distinct, grid1((size_t)n_px, QUANT_BLOCK), dim3(QUANT_LANES), 0, f.st, (const uint32_t*)src->ptr, n_px, (uint32_t)max_colors, set);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(host.data(), set, sizeof(QuantSet), hipMemcpyDeviceToHost, f.st));
    HIPCHK(hipStreamSynchronize(f.st));
    const QuantSet& h = host[0];
    *n_colors = 0;
    *overflow = h.full || h.count > (uint32_t)max_colors;
    if (*overflow) return 0;
    int64_t n = 0;
    for (uint32_t s = 0; s < QUANT_SLOTS; ++s)
        if (h.slot[s] != QUANT_EMPTY) {
            if (n == max_colors) return fail(SVGR_E_STATE, "%s: the set holds more colours than it counted", entry);
            colors[n++] = h.slot[s];
        }
    if (n != (int64_t)h.count) return fail(SVGR_E_STATE, "%s: the set holds %lld colours and counted %u", entry, (long long)n, h.count);
    std::sort(colors, colors + n);
    *n_colors = n;
    return 0;
}

static int quant_bins_impl(svgr_ctx* ctx, const svgr_buf* src, int64_t rows, int64_t cols, uint32_t* keys, uint64_t* bins, int64_t cap, int64_t* n_bins) {
    static const char* entry = "svgr_quant_bins";
    if (int rc = quant_check(entry, ctx, src, rows, cols)) return rc;
    if (!n_bins || cap < 0 || (cap && (!keys || !bins))) return fail(SVGR_E_INVALID, "%s: bad arguments", entry);
    static_assert(sizeof(QuantBin) == 40, "five 64-bit fields");
    int total = 0;
    PassFrame f(ctx);
    HIPCHK(enter_ctx(ctx));
    hipStream_t st = f.st;
    QuantBin* hist = f.scratch<QuantBin>(QUANT_BINS);
    int* flag = f.scratch<int>(QUANT_BINS);
    int* tops = f.scratch<int>(QUANT_BINS / DASH_S);
    if (f.err) return f.err;
    HIPCHK(hipMemsetAsync(hist, 0, (size_t)QUANT_BINS * sizeof(QuantBin), st));
    const long long n_px = (long long)rows * cols;
    const long long n_blocks = (n_px + QUANT_BLOCK - 1) / QUANT_BLOCK;
    SVGR_LAUNCH(k_quant_bins, dim3((unsigned)std::min<long long>(n_blocks, QUANT_GROUPS)), dim3(QUANT_LANES), 0, st, (const uint32_t*)src->ptr, n_px, n_blocks, hist);
    SVGR_LAUNCH(k_quant_flag, grid1(QUANT_BINS, QUANT_LANES), dim3(QUANT_LANES), 0, st, (const QuantBin*)hist, flag);
    dash_scan<int, QuantSumOp>(st, flag, tops, (int)QUANT_BINS);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(&total, flag + (QUANT_BINS - 1), sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (total <= 0 || (long long)total > n_px) return fail(SVGR_E_STATE, "%s: %d bins for %lld pixels", entry, total, n_px);
    *n_bins = total;
    if (total > cap) return fail(SVGR_E_INVALID, "%s: %d bins need more room than %lld", entry, total, (long long)cap);
    uint32_t* d_keys = f.scratch<uint32_t>((size_t)total);
    QuantBin* d_bins = f.scratch<QuantBin>((size_t)total);
    if (f.err) return f.err;
    SVGR_LAUNCH(k_quant_compact, grid1(QUANT_BINS, QUANT_LANES), dim3(QUANT_LANES), 0, st, (const QuantBin*)hist, (const int*)flag, total, d_keys, d_bins);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(keys, d_keys, (size_t)total * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(bins, d_bins, (size_t)total * sizeof(QuantBin), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return 0;
}

extern "C" {
int svgr_quant_block(void) { return QUANT_BLOCK; }
int svgr_quant_groups(void) { return QUANT_GROUPS; }
int svgr_quant_distinct(svgr_ctx* ctx, const svgr_buf* src_rgba8, int64_t rows, int64_t cols, int max_colors, uint32_t* colors, int64_t* n_colors,
                        int* overflow) {
    return abi_guard("svgr_quant_distinct", [&]() { return quant_distinct_impl(ctx, src_rgba8, rows, cols, max_colors, colors, n_colors, overflow); });
}
int svgr_quant_bins(svgr_ctx* ctx, const svgr_buf* src_rgba8, int64_t rows, int64_t cols, uint32_t* keys, uint64_t* bins, int64_t cap, int64_t* n_bins) {
    return abi_guard("svgr_quant_bins", [&]() { return quant_bins_impl(ctx, src_rgba8, rows, cols, keys, bins, cap, n_bins); });
}
int svgr_quant_index(svgr_ctx* ctx, const svgr_buf* src_rgba8, int64_t rows, int64_t cols, const svgr_buf* palette, int n_palette, svgr_buf* out_stream,
                     svgr_buf* out_indices) {
    static const char* entry = "svgr_quant_index";
    if (int rc = quant_check(entry, ctx, src_rgba8, rows, cols)) return rc;
    if (!palette || (!out_stream && !out_indices)) return fail(SVGR_E_INVALID, "%s: bad arguments", entry);
    if (n_palette < 1 || n_palette > QUANT_MAX_COLORS) return fail(SVGR_E_INVALID, "%s: a palette has 1 .. %d entries, not %d", entry, QUANT_MAX_COLORS, n_palette);
    const int depth = quant_depth(n_palette);
    if (palette->bytes < (size_t)n_palette * 4 || (out_stream && out_stream->bytes < (size_t)rows * (size_t)quant_row_bytes(cols, depth)) ||
        (out_indices && out_indices->bytes < (size_t)rows * cols))
        return fail(SVGR_E_INVALID, "%s: buffer too small", entry);
    if ((out_stream && out_stream->ptr == src_rgba8->ptr) || (out_indices && out_indices->ptr == src_rgba8->ptr))
        return fail(SVGR_E_INVALID, "%s: an output must not be the source", entry);
    const dim3 grid((unsigned)((cols + QUANT_BLOCK - 1) / QUANT_BLOCK), (unsigned)std::min<int64_t>(rows, 65535));
    return launch_tail(ctx, k_quant_index, grid, dim3(QUANT_LANES), 0, (const uint32_t*)src_rgba8->ptr, (int)rows, (int)cols, (const uint32_t*)palette->ptr,
                       n_palette, depth, out_stream ? (uint8_t*)out_stream->ptr : (uint8_t*)nullptr, out_indices ? (uint8_t*)out_indices->ptr : (uint8_t*)nullptr);
}
}  // extern "C"

// ======================================================================================
// Dithering for indexed PNG output (svgr_quant_dither): svgr_dither.h has the arithmetic, DESIGN.md 7u the definitions.
//
//   k_quant_dither_ordered   k_quant_index with the Bayer offset added to the pixel's coordinates: a map over the pixels.  The
//                            target, not the pixel, decides whether a lane may reuse its previous pixel's entry
//   k_quant_dither_diffuse   Floyd-Steinberg is sequential as written: (r, c) needs (r, c-1), (r-1, c-1), (r-1, c), (r-1, c+1), so
//                            the pixels with equal c + 2 r are independent.  A tile is a strip of DITHER_S rows, skewed two
//                            columns to the left per row into a parallelogram DITHER_W wide: at step j every row works on its j-th
//                            pixel, and what it needs from the row above was made at the steps j-1, j-2 and j-3.  One workgroup
//                            takes one tile, DITHER_L lanes a pixel: each lane searches its slice of the palette (read from LDS
//                            once and held in registers: it is the same for every pixel of the tile), and a
//                            butterfly of shuffles takes the minimum of (D << 8 | index) -- D < 2^36, so the one 64-bit compare
//                            orders by D and then by index, the sequential loop's tie rule.  The errors of the tile's rows live
//                            in LDS.  A tile needs its left neighbour and, for its first row, the two tiles above it and above to
//                            the right (DITHER_W > 2 (DITHER_S - 1) keeps it to those): tiles with equal block + 2 strip share a
//                            launch, the launches follow each other on the stream, and no workgroup ever waits for another.  What
//                            crosses a tile's edge goes through memory: the errors of a strip's last row (one buffer per strip
//                            parity, the pixel at c+1 included) and the last three errors of every row of a tile
// ======================================================================================
#include "svgr_dither.h"

QUANT_KERNEL void k_quant_dither_ordered(const uint32_t* __restrict__ src, int rows, int cols, const uint32_t* __restrict__ pal, int n_pal, int depth,
                                         uint32_t amp, uint8_t* __restrict__ stream, uint8_t* __restrict__ indices) {
    __shared__ uint32_t pal_x[4 * QUANT_MAX_COLORS];
    if ((int)threadIdx.x < n_pal) quant_x(quant_canon(pal[threadIdx.x]), pal_x + 4 * threadIdx.x);
    __syncthreads();
    const long long c0 = ((long long)blockIdx.x * QUANT_LANES + threadIdx.x) * QUANT_RUN;
    if (c0 >= cols) return;
    const int n = cols - c0 >= QUANT_RUN ? QUANT_RUN : (int)(cols - c0);
    const long long rb = quant_row_bytes(cols, depth);
    for (long long row = blockIdx.y; row < rows; row += gridDim.y) {
        const uint32_t* p = src + row * cols + c0;
        uint8_t idx[QUANT_RUN], bytes[QUANT_RUN];
        uint32_t prev[4] = {0, 0, 0, 0};
        SVGR_UNROLL
        for (int k = 0; k < QUANT_RUN; ++k) {
            idx[k] = 0;
            if (k < n) {
                const uint32_t c = quant_canon(p[k]);
                uint32_t x[4], t[4];
                quant_x(c, x);
                dither_ordered_target(x, c >> 24, amp, row, c0 + k, t);
                if (k && t[0] == prev[0] && t[1] == prev[1] && t[2] == prev[2] && t[3] == prev[3]) idx[k] = idx[k - 1];
                else idx[k] = (uint8_t)quant_nearest(pal_x, n_pal, t);
                SVGR_UNROLL
                for (int j = 0; j < 4; ++j) prev[j] = t[j];
            }
        }
        if (indices) {
            SVGR_UNROLL
            for (int k = 0; k < QUANT_RUN; ++k)
                if (k < n) indices[row * cols + c0 + k] = idx[k];
        }
        if (stream) {
            uint8_t* o = stream + row * rb;
            if (c0 == 0) o[0] = 0;
            quant_pack_run(idx, n, depth, bytes);
            const int nb = (n * depth + 7) / 8;
            o += 1 + c0 * depth / 8;
            SVGR_UNROLL
            for (int j = 0; j < QUANT_RUN; ++j)
                if (j < nb) o[j] = bytes[j];
        }
    }
}

constexpr int DITHER_S = 16, DITHER_W = 32, DITHER_L = QUANT_LANES / DITHER_S, DITHER_EDGE = 3;
static_assert(DITHER_W > 2 * (DITHER_S - 1), "a tile's first row reaches no further than the tile above to the right");
static_assert(DITHER_L <= 64 && 64 % DITHER_L == 0 && (DITHER_L & (DITHER_L - 1)) == 0, "a pixel's lanes are one aligned group of a wave");
static_assert(DITHER_S * DITHER_W == 2 * QUANT_LANES, "the load and store phases give a lane two pixels");

// The nearest entry to the target (t0, t1, t2, t3) over the group's DITHER_L lanes; every lane of the group gets the result.  A lane
// searches the same entries for every pixel of the tile -- l, l + DITHER_L, ... (l: its place in the group) -- and holds them in
// registers: `mine`, the first n_mine of which exist in some lane.  quant_dist, a coordinate at a time on the entry's four words.
constexpr int DITHER_SLICE = QUANT_MAX_COLORS / DITHER_L;
__device__ __forceinline__ int dither_group_nearest(const uint4 (&mine)[DITHER_SLICE], int n_mine, int n_pal, uint32_t t0, uint32_t t1, uint32_t t2, uint32_t t3, int l) {
    unsigned long long best = ~0ull;
    SVGR_UNROLL
    for (int q = 0; q < DITHER_SLICE; ++q) {
        if (q < n_mine) {   // (the same in every lane)
            const uint4 y = mine[q];
            const uint32_t d0 = t0 > y.x ? t0 - y.x : y.x - t0, d1 = t1 > y.y ? t1 - y.y : y.y - t1, d2 = t2 > y.z ? t2 - y.z : y.z - t2,
                           d3 = t3 > y.w ? t3 - y.w : y.w - t3;   // (each <= 65025: its square fits 32 bits)
            const unsigned long long d = (unsigned long long)(d0 * d0) + (unsigned long long)(d1 * d1) + (unsigned long long)(d2 * d2) + (unsigned long long)(d3 * d3);
            const unsigned long long key = l + q * DITHER_L < n_pal ? d << 8 | (unsigned)(l + q * DITHER_L) : ~0ull;
            best = key < best ? key : best;
        }
    }
    SVGR_UNROLL
    for (int m = DITHER_L / 2; m; m >>= 1) {
        const unsigned long long other = __shfl_xor(best, m, DITHER_L);
        best = other < best ? other : best;
    }
    return (int)(best & 255u);
}

// The tiles (strip, block) with block + 2 strip == front, strip = strip0 + blockIdx.x.  row_err: 2 * cols errors, the last row of a
// strip at [(strip & 1) * cols + c]; col_err: per image row DITHER_EDGE errors, those of the row's last pixels in the tile that
// has just been through it.
QUANT_KERNEL void k_quant_dither_diffuse(const uint32_t* __restrict__ src, int rows, int cols, const uint32_t* __restrict__ pal, int n_pal, int depth,
                                         int front, int strip0, int4* __restrict__ row_err, int4* __restrict__ col_err, uint8_t* __restrict__ stream,
                                         uint8_t* __restrict__ indices) {
    __shared__ uint4 pal_x[QUANT_MAX_COLORS];
    __shared__ int4 err[DITHER_S + 1][DITHER_W + DITHER_EDGE];   // [1 + row][EDGE + step]; row -1 is the strip above
    __shared__ uint32_t px_s[DITHER_S][DITHER_W];
    __shared__ uint8_t idx_s[DITHER_S][DITHER_W];
    const int tid = (int)threadIdx.x, strip = strip0 + (int)blockIdx.x, block = front - 2 * strip;
    const int row0 = strip * DITHER_S, col0 = block * DITHER_W;   // the tile's row i begins at the column col0 - 2 i
    if (tid < n_pal) {
        uint32_t y[4];
        quant_x(quant_canon(pal[tid]), y);
        pal_x[tid] = make_uint4(y[0], y[1], y[2], y[3]);
    }
    SVGR_UNROLL
    for (int p = tid; p < DITHER_S * DITHER_W; p += QUANT_LANES) {
        const int i = p / DITHER_W, j = p % DITHER_W, r = row0 + i, c = col0 - 2 * i + j;
        px_s[i][j] = (r < rows && c >= 0 && c < cols) ? quant_canon(src[(long long)r * cols + c]) : 0u;   // (outside: no error, no store)
    }
    if (tid < DITHER_W + DITHER_EDGE) {   // the row above: step j' of it is the column col0 + j' + 2
        const int c = col0 - 1 + tid;
        int4 e = make_int4(0, 0, 0, 0);
        if (strip > 0 && c >= 0 && c < cols) e = row_err[(long long)((strip - 1) & 1) * cols + c];
        err[0][tid] = e;
    }
    if (tid < DITHER_S * DITHER_EDGE) {
        const int i = tid / DITHER_EDGE, q = tid % DITHER_EDGE;
        int4 e = make_int4(0, 0, 0, 0);
        if (block > 0) e = col_err[(long long)(row0 + i) * DITHER_EDGE + q];
        err[1 + i][q] = e;
    }
    __syncthreads();
    const int i = tid / DITHER_L, l = tid % DITHER_L;
    uint4 mine[DITHER_SLICE];
    const int n_mine = (n_pal + DITHER_L - 1) / DITHER_L;
    SVGR_UNROLL
    for (int q = 0; q < DITHER_SLICE; ++q) mine[q] = pal_x[l + q * DITHER_L];   // (beyond n_pal: read, never used)
    const int clear = dither_group_nearest(mine, n_mine, n_pal, 0u, 0u, 0u, 0u, l);
    for (int j = 0; j < DITHER_W; ++j) {
        const uint32_t px = px_s[i][j];
        // errors: of this row's last pixel; of the row above at the columns c + 1, c, c - 1, which it had at the steps j - 1, j - 2, j - 3
        const int4 left = err[1 + i][DITHER_EDGE + j - 1], u1 = err[i][DITHER_EDGE + j - 1], u2 = err[i][DITHER_EDGE + j - 2], u3 = err[i][DITHER_EDGE + j - 3];
        const int32_t acc[4] = {7 * left.x + 3 * u1.x + 5 * u2.x + u3.x, 7 * left.y + 3 * u1.y + 5 * u2.y + u3.y,
                                7 * left.z + 3 * u1.z + 5 * u2.z + u3.z, 7 * left.w + 3 * u1.w + 5 * u2.w + u3.w};
        uint32_t x[4], t[4];
        quant_x(px, x);
        dither_diffusion_target(x, acc, t);
        const int k = dither_group_nearest(mine, n_mine, n_pal, t[0], t[1], t[2], t[3], l);   // (every lane takes part, whatever its pixel: the shuffles stay whole)
        if (l == 0) {
            const uint4 y = pal_x[k];
            err[1 + i][DITHER_EDGE + j] = px ? make_int4((int)t[0] - (int)y.x, (int)t[1] - (int)y.y, (int)t[2] - (int)y.z, (int)t[3] - (int)y.w) : make_int4(0, 0, 0, 0);
            idx_s[i][j] = (uint8_t)(px ? k : clear);
        }
        __syncthreads();   // (step j + 1 reads what step j wrote, and writes where nobody reads before the next barrier)
    }
    // what the tiles to the right and below need
    if (tid < DITHER_S * DITHER_EDGE) {
        const int ii = tid / DITHER_EDGE, q = tid % DITHER_EDGE;
        col_err[(long long)(row0 + ii) * DITHER_EDGE + q] = err[1 + ii][DITHER_W + q];   // (it has a strip's rows for every strip)
    }
    if (tid < DITHER_W) {
        const int c = col0 - 2 * (DITHER_S - 1) + tid;
        if (c >= 0 && c < cols) row_err[(long long)(strip & 1) * cols + c] = err[DITHER_S][DITHER_EDGE + tid];
    }
    if (indices) {
        SVGR_UNROLL
        for (int p = tid; p < DITHER_S * DITHER_W; p += QUANT_LANES) {
            const int ii = p / DITHER_W, j = p % DITHER_W, r = row0 + ii, c = col0 - 2 * ii + j;
            if (r < rows && c >= 0 && c < cols) indices[(long long)r * cols + c] = idx_s[ii][j];
        }
    }
    if (stream && row0 + i < rows) {
        // the row's bytes that hold a pixel of this tile; a byte shared with the tile to the left or right (another launch, earlier
        // or later on the stream) gets this tile's bits added: the stream was cleared before the first launch
        const int first = col0 - 2 * i, c_lo = first > 0 ? first : 0, c_hi = first + DITHER_W - 1 < cols - 1 ? first + DITHER_W - 1 : cols - 1;
        const int per = 8 / depth;
        uint8_t* o = stream + (long long)(row0 + i) * quant_row_bytes(cols, depth) + 1;
        if (c_lo <= c_hi)
            for (int q = c_lo / per + l; q <= c_hi / per; q += DITHER_L) {
                uint32_t v = 0;
                for (int k = 0; k < per; ++k) {
                    const int c = q * per + k;
                    if (c >= c_lo && c <= c_hi) v |= (uint32_t)idx_s[i][c - first] << (8 - depth * (k + 1));
                }
                o[q] = depth == 8 ? (uint8_t)v : (uint8_t)(o[q] | v);
            }
    }
}

static int quant_dither_impl(svgr_ctx* ctx, const svgr_buf* src, int64_t rows, int64_t cols, const svgr_buf* palette, int n_palette, int mode, int amp,
                             svgr_buf* out_stream, svgr_buf* out_indices) {
    static const char* entry = "svgr_quant_dither";
    if (int rc = quant_check(entry, ctx, src, rows, cols)) return rc;
    if (!palette || (!out_stream && !out_indices)) return fail(SVGR_E_INVALID, "%s: bad arguments", entry);
    if (mode != DITHER_ORDERED && mode != DITHER_DIFFUSION) return fail(SVGR_E_INVALID, "%s: mode is 1 (ordered) or 2 (diffusion), not %d", entry, mode);
    if (amp < 0 || amp > DITHER_X_MAX) return fail(SVGR_E_INVALID, "%s: the amplitude is 0 .. %d, not %d", entry, (int)DITHER_X_MAX, amp);
    if (n_palette < 1 || n_palette > QUANT_MAX_COLORS) return fail(SVGR_E_INVALID, "%s: a palette has 1 .. %d entries, not %d", entry, QUANT_MAX_COLORS, n_palette);
    const int depth = quant_depth(n_palette);
    const size_t stream_bytes = (size_t)rows * (size_t)quant_row_bytes(cols, depth);
    if (palette->bytes < (size_t)n_palette * 4 || (out_stream && out_stream->bytes < stream_bytes) || (out_indices && out_indices->bytes < (size_t)rows * cols))
        return fail(SVGR_E_INVALID, "%s: buffer too small", entry);
    if ((out_stream && out_stream->ptr == src->ptr) || (out_indices && out_indices->ptr == src->ptr))
        return fail(SVGR_E_INVALID, "%s: an output must not be the source", entry);
    uint8_t* stream = out_stream ? (uint8_t*)out_stream->ptr : (uint8_t*)nullptr;
    uint8_t* indices = out_indices ? (uint8_t*)out_indices->ptr : (uint8_t*)nullptr;
    if (mode == DITHER_ORDERED) {
        const dim3 grid((unsigned)((cols + QUANT_BLOCK - 1) / QUANT_BLOCK), (unsigned)std::min<int64_t>(rows, 65535));
        return launch_tail(ctx, k_quant_dither_ordered, grid, dim3(QUANT_LANES), 0, (const uint32_t*)src->ptr, (int)rows, (int)cols, (const uint32_t*)palette->ptr,
                           n_palette, depth, (uint32_t)amp, stream, indices);
    }
    // the blocks cover the last row of a strip, which begins 2 (DITHER_S - 1) columns to the left of the first
    const int strips = (int)((rows + DITHER_S - 1) / DITHER_S), blocks = (int)((cols + 2 * (DITHER_S - 1) + DITHER_W - 1) / DITHER_W);
    PassFrame f(ctx);
    HIPCHK(enter_ctx(ctx));
    int4* row_err = f.scratch<int4>(2 * (size_t)cols);
    int4* col_err = f.scratch<int4>((size_t)strips * DITHER_S * DITHER_EDGE);
    if (f.err) return f.err;
    if (stream) HIPCHK(hipMemsetAsync(stream, 0, stream_bytes, f.st));
    for (int front = 0; front <= blocks - 1 + 2 * (strips - 1); ++front) {
        const int lo = front - (blocks - 1) > 0 ? (front - (blocks - 1) + 1) / 2 : 0, hi = std::min(strips - 1, front / 2);
        if (lo > hi) continue;
        SVGR_LAUNCH(k_quant_dither_diffuse, dim3((unsigned)(hi - lo + 1)), dim3(QUANT_LANES), 0, f.st, (const uint32_t*)src->ptr, (int)rows, (int)cols,
                    (const uint32_t*)palette->ptr, n_palette, depth, front, lo, row_err, col_err, stream, indices);
    }
    HIPCHK(hipGetLastError());
    return 0;   // (the frame waits for the stream before its scratch goes)
}

extern "C" {
int svgr_dither_tile_rows(void) { return DITHER_S; }
int svgr_dither_tile_cols(void) { return DITHER_W; }
int svgr_quant_dither(svgr_ctx* ctx, const svgr_buf* src_rgba8, int64_t rows, int64_t cols, const svgr_buf* palette, int n_palette, int mode, int amp,
                      svgr_buf* out_stream, svgr_buf* out_indices) {
    return abi_guard("svgr_quant_dither", [&]() { return quant_dither_impl(ctx, src_rgba8, rows, cols, palette, n_palette, mode, amp, out_stream, out_indices); });
}
}  // extern "C"

// ======================================================================================
// differentiable coverage: svgr_cover_forward / svgr_cover_backward (csrc/svgr_cover.h has the per-lane arithmetic, DESIGN.md 7w
// the derivation).  New kernels beside the renderer's: k_flatten, k_path_build and k_tile_render are not involved.
//   forward   k_cover_accumulate  a lane per segment: flattens in registers and adds every row piece of every edge into the path's
//                                 double plane with one global atomic add each (the ATOMIC form: a plane may be any size, so it
//                                 cannot be staged in LDS, and a segment leaves a handful of pieces per row it crosses)
//             k_cover_resolve     a wave per (path, row): the running sum of the row, COVER_SCAN columns per step, -> cover, slope
//   backward  k_cover_vjp         a lane per segment: flattens again with the same code (the same edges to the bit), walks each edge
//                                 over W = grad_out * slope and writes its own 8 + 6 doubles; no atomics, no edge list
//             k_cover_vjp_m6      a lane per path: the 6 partials of its segments summed in segment order
// No host read-back between the launches; nothing waits.
// ======================================================================================
#include "svgr_cover.h"

constexpr int COVER_BLOCK = 64;                 // segments per workgroup of the two segment kernels: a lane each, one wave
constexpr int COVER_RUN = 4;                    // consecutive columns a lane of the row scan takes per step
constexpr int COVER_SCAN = 64 * COVER_RUN;      // columns per step of the row scan

struct CoverGeom {
    const double* segs;
    const uint8_t* kind;
    const int* seg_off;
    const double* m6;
    int n_segs, n_paths, rows, cols;
    double or0, oc0, thr;
};

// the path whose range [off[p], off[p + 1]) holds `seg` (empty paths in front of it are passed over); -1: none
__device__ __forceinline__ int cover_path_of(const int* __restrict__ off, int n_paths, int seg) {
    int lo = 0, hi = n_paths;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= seg) lo = mid; else hi = mid;
    }
    return off[lo] <= seg && seg < off[lo + 1] ? lo : -1;
}

__global__ __launch_bounds__(COVER_BLOCK) void k_cover_accumulate(const CoverGeom g, double* __restrict__ acc, unsigned* __restrict__ status) {
    const int seg = blockIdx.x * COVER_BLOCK + threadIdx.x;
    if (seg >= g.n_segs) return;
    const int p = cover_path_of(g.seg_off, g.n_paths, seg);
    if (p < 0) return;
    double pts[8];
    for (int i = 0; i < 8; ++i) pts[i] = g.segs[8 * (size_t)seg + i];
    const int rows = g.rows, cols = g.cols;
    double* plane = acc + (size_t)p * (size_t)rows * (size_t)cols;
    const int st = cover_seg_accumulate(pts, g.kind[seg] != SVGR_SEG_LINE, g.m6 + 6 * (size_t)p, g.or0, g.oc0, rows, cols, g.thr,
                                        [&](int r, int c, double v) {
                                            if ((unsigned)r < (unsigned)rows && (unsigned)c < (unsigned)cols)
                                                unsafeAtomicAdd(plane + (size_t)r * (size_t)cols + (size_t)c, v);
                                        });
    if (st) atomicOr(status, (unsigned)st);
}

// (acc and cover are the same memory for double planes: a lane reads its own columns of a step before it writes them)
template <class T>
__global__ __launch_bounds__(64) void k_cover_resolve(const double* acc, const uint8_t* __restrict__ rule, int rows, int cols, T* cover,
                                                      int8_t* __restrict__ slope) {
    const size_t pr = blockIdx.x;   // path * rows + row
    const int evenodd = rule[pr / (size_t)rows] & 1;
    const double* a = acc + pr * (size_t)cols;
    T* o = cover + pr * (size_t)cols;
    int8_t* s = slope + pr * (size_t)cols;
    const int lane = threadIdx.x;
    double carry = 0.0;
    for (int c0 = 0; c0 < cols; c0 += COVER_SCAN) {
        const int c = c0 + lane * COVER_RUN;
        double v[COVER_RUN];
        SVGR_UNROLL
        for (int k = 0; k < COVER_RUN; ++k) v[k] = c + k < cols ? a[c + k] : 0.0;
        SVGR_UNROLL
        for (int k = 1; k < COVER_RUN; ++k) v[k] = v[k - 1] + v[k];
        double inc = v[COVER_RUN - 1];
        for (int d = 1; d < 64; d <<= 1) {
            const double up = __shfl_up(inc, d);
            if (lane >= d) inc = up + inc;
        }
        double before = __shfl_up(inc, 1);
        before = lane == 0 ? carry : carry + before;
        SVGR_UNROLL
        for (int k = 0; k < COVER_RUN; ++k) {
            if (c + k < cols) {
                const double A = before + v[k];
                o[c + k] = (T)fill_rule(A, evenodd);
                s[c + k] = (int8_t)cover_slope(A, evenodd);
            }
        }
        carry = carry + __shfl(inc, 63);
    }
}

template <class T>
__global__ __launch_bounds__(COVER_BLOCK) void k_cover_vjp(const CoverGeom g, const int8_t* __restrict__ slope, const T* __restrict__ grad_out,
                                                           double* __restrict__ grad_segs, double* __restrict__ part,
                                                           unsigned* __restrict__ status) {
    const int seg = blockIdx.x * COVER_BLOCK + threadIdx.x;
    if (seg >= g.n_segs) return;
    const int p = cover_path_of(g.seg_off, g.n_paths, seg);
    double gs[8], gm[6];
    for (int i = 0; i < 8; ++i) gs[i] = 0.0;
    for (int i = 0; i < 6; ++i) gm[i] = 0.0;
    if (p >= 0) {
        double pts[8];
        for (int i = 0; i < 8; ++i) pts[i] = g.segs[8 * (size_t)seg + i];
        const int rows = g.rows, cols = g.cols;
        const size_t base = (size_t)p * (size_t)rows * (size_t)cols;
        const int st = cover_seg_vjp(pts, g.kind[seg] != SVGR_SEG_LINE, g.m6 + 6 * (size_t)p, g.or0, g.oc0, rows, cols, g.thr,
                                     [&](int r, int c) {
                                         if ((unsigned)r >= (unsigned)rows || (unsigned)c >= (unsigned)cols) return 0.0;
                                         const size_t i = base + (size_t)r * (size_t)cols + (size_t)c;
                                         const int sl = slope[i];
                                         return sl ? cover_weight((double)grad_out[i], sl) : 0.0;
                                     }, gs, gm);
        if (st) atomicOr(status, (unsigned)st);
    }
    for (int i = 0; i < 8; ++i) grad_segs[8 * (size_t)seg + i] = gs[i];
    for (int i = 0; i < 6; ++i) part[6 * (size_t)seg + i] = gm[i];
}

__global__ __launch_bounds__(64) void k_cover_vjp_m6(const double* __restrict__ part, const int* __restrict__ seg_off, int n_segs, int n_paths,
                                                     double* __restrict__ grad_m6) {
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= n_paths) return;
    int s0 = seg_off[p], s1 = seg_off[p + 1];
    s0 = s0 < 0 ? 0 : s0;
    s1 = s1 > n_segs ? n_segs : s1;
    double m[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int s = s0; s < s1; ++s)
        for (int k = 0; k < 6; ++k) m[k] = m[k] + part[6 * (size_t)s + k];
    for (int k = 0; k < 6; ++k) grad_m6[6 * (size_t)p + k] = m[k];
}

// Everything of a description and its input buffers that can be wrong, and the kernels' numbers from it.
static int cover_check(const char* entry, const svgr_ctx* ctx, const svgr_cover_desc* d, const svgr_buf* segs, const svgr_buf* kind,
                       const svgr_buf* off, const svgr_buf* m6, const svgr_buf* status, CoverGeom& g, size_t& n_px) {
    if (!ctx) return fail(SVGR_E_INVALID, "%s: ctx is NULL", entry);
    if (!d) return fail(SVGR_E_INVALID, "%s: desc is NULL", entry);
    constexpr int64_t kMax = (1ll << 31) - 1;
    if (d->n_segs < 0 || d->n_segs > kMax - COVER_BLOCK || d->n_paths <= 0 || d->n_paths > kMax - 64)
        return fail(SVGR_E_INVALID, "%s: n_segs %lld is negative or n_paths %lld is not positive (or beyond 2^31)", entry, (long long)d->n_segs, (long long)d->n_paths);
    const int64_t row0 = d->viewport[0], col0 = d->viewport[1], rows = d->viewport[2], cols = d->viewport[3];
    if (rows <= 0 || cols <= 0) return fail(SVGR_E_INVALID, "%s: a viewport of %lld x %lld", entry, (long long)rows, (long long)cols);
    if (row0 < -(1ll << 30) || row0 > (1ll << 30) || col0 < -(1ll << 30) || col0 > (1ll << 30))
        return fail(SVGR_E_INVALID, "%s: the viewport's origin is beyond +-2^30", entry);
    if (d->plane < 0 || d->plane >= COVER_PLANES || d->reserved != 0) return fail(SVGR_E_INVALID, "%s: unknown plane type %d", entry, (int)d->plane);
    if (!(d->flatness > 0.0) || !std::isfinite(d->flatness)) return fail(SVGR_E_INVALID, "%s: flatness must be positive and finite", entry);
    if (rows > kMax || cols > kMax || (unsigned __int128)d->n_paths * (unsigned __int128)rows * (unsigned __int128)cols > (unsigned __int128)kMax)
        return fail(SVGR_E_OVERFLOW, "%s: %lld planes of %lld x %lld pixels are beyond 2^31 - 1 pixels", entry, (long long)d->n_paths, (long long)rows, (long long)cols);
    if (!off || !m6 || !status || (d->n_segs > 0 && (!segs || !kind))) return fail(SVGR_E_INVALID, "%s: a buffer is NULL", entry);
    if ((d->n_segs > 0 && (segs->bytes < (size_t)d->n_segs * 64 || kind->bytes < (size_t)d->n_segs)) || off->bytes < ((size_t)d->n_paths + 1) * 4 ||
        m6->bytes < (size_t)d->n_paths * 48 || status->bytes < 4)
        return fail(SVGR_E_INVALID, "%s: an input buffer is too small for the description", entry);
    n_px = (size_t)d->n_paths * (size_t)rows * (size_t)cols;
    g.segs = d->n_segs > 0 ? (const double*)segs->ptr : nullptr;
    g.kind = d->n_segs > 0 ? (const uint8_t*)kind->ptr : nullptr;
    g.seg_off = (const int*)off->ptr;
    g.m6 = (const double*)m6->ptr;
    g.n_segs = (int)d->n_segs; g.n_paths = (int)d->n_paths; g.rows = (int)rows; g.cols = (int)cols;
    g.or0 = (double)row0; g.oc0 = (double)col0;
    g.thr = (d->flatness * d->flatness) * 16.0;   // (svgr_batch_create's)
    return 0;
}

static int cover_forward_impl(svgr_ctx* ctx, const svgr_cover_desc* d, const svgr_buf* segs, const svgr_buf* kind, const svgr_buf* off,
                              const svgr_buf* m6, const svgr_buf* rule, svgr_buf* cover, svgr_buf* slope, svgr_buf* status) {
    static const char* entry = "svgr_cover_forward";
    CoverGeom g;
    size_t n_px;
    if (int rc = cover_check(entry, ctx, d, segs, kind, off, m6, status, g, n_px)) return rc;
    if (!rule || !cover || !slope) return fail(SVGR_E_INVALID, "%s: a buffer is NULL", entry);
    const size_t eb = (size_t)cover_plane_bytes(d->plane);
    if (rule->bytes < (size_t)g.n_paths || cover->bytes < n_px * eb || slope->bytes < n_px)
        return fail(SVGR_E_INVALID, "%s: rule, cover or slope is too small for the description", entry);
    HIPCHK(enter_ctx(ctx));
    hipStream_t st = ctx->stream;
    if (g.n_segs == 0) {
        HIPCHK(hipMemsetAsync(cover->ptr, 0, n_px * eb, st));
        HIPCHK(hipMemsetAsync(slope->ptr, 0, n_px, st));
        return 0;
    }
    PoolBlock scratch;   // (float planes: the double accumulation plane; goes back at scope end by the pool's stream-order rule)
    double* acc = (double*)cover->ptr;
    if (d->plane == COVER_F32) {
        HIPCHK(scratch.alloc(n_px * 8, ctx->device));
        acc = scratch.as<double>();
    }
    HIPCHK(hipMemsetAsync(acc, 0, n_px * 8, st));
    SVGR_LAUNCH(k_cover_accumulate, grid1((size_t)g.n_segs, COVER_BLOCK), dim3(COVER_BLOCK), 0, st, g, acc, (unsigned*)status->ptr);
    const dim3 rgrid((unsigned)((size_t)g.n_paths * (size_t)g.rows));
    if (d->plane == COVER_F32)
        SVGR_LAUNCH(k_cover_resolve<float>, rgrid, dim3(64), 0, st, (const double*)acc, (const uint8_t*)rule->ptr, g.rows, g.cols, (float*)cover->ptr, (int8_t*)slope->ptr);
    else
        SVGR_LAUNCH(k_cover_resolve<double>, rgrid, dim3(64), 0, st, (const double*)acc, (const uint8_t*)rule->ptr, g.rows, g.cols, (double*)cover->ptr, (int8_t*)slope->ptr);
    HIPCHK(hipGetLastError());
    return 0;
}

static int cover_backward_impl(svgr_ctx* ctx, const svgr_cover_desc* d, const svgr_buf* segs, const svgr_buf* kind, const svgr_buf* off,
                               const svgr_buf* m6, const svgr_buf* slope, const svgr_buf* grad_out, svgr_buf* grad_segs, svgr_buf* grad_m6,
                               svgr_buf* status) {
    static const char* entry = "svgr_cover_backward";
    CoverGeom g;
    size_t n_px;
    if (int rc = cover_check(entry, ctx, d, segs, kind, off, m6, status, g, n_px)) return rc;
    if (!slope || !grad_out || !grad_m6 || (g.n_segs > 0 && !grad_segs)) return fail(SVGR_E_INVALID, "%s: a buffer is NULL", entry);
    const size_t eb = (size_t)cover_plane_bytes(d->plane);
    if (slope->bytes < n_px || grad_out->bytes < n_px * eb || grad_m6->bytes < (size_t)g.n_paths * 48 ||
        (g.n_segs > 0 && grad_segs->bytes < (size_t)g.n_segs * 64))
        return fail(SVGR_E_INVALID, "%s: slope, grad_out, grad_segs or grad_m6 is too small for the description", entry);
    HIPCHK(enter_ctx(ctx));
    hipStream_t st = ctx->stream;
    if (g.n_segs == 0) {
        HIPCHK(hipMemsetAsync(grad_m6->ptr, 0, (size_t)g.n_paths * 48, st));
        return 0;
    }
    PoolBlock part;   // the segments' 6 partials of their path's transform
    HIPCHK(part.alloc((size_t)g.n_segs * 48, ctx->device));
    const dim3 sgrid = grid1((size_t)g.n_segs, COVER_BLOCK);
    if (d->plane == COVER_F32)
        SVGR_LAUNCH(k_cover_vjp<float>, sgrid, dim3(COVER_BLOCK), 0, st, g, (const int8_t*)slope->ptr, (const float*)grad_out->ptr, (double*)grad_segs->ptr,
                    part.as<double>(), (unsigned*)status->ptr);
    else
        SVGR_LAUNCH(k_cover_vjp<double>, sgrid, dim3(COVER_BLOCK), 0, st, g, (const int8_t*)slope->ptr, (const double*)grad_out->ptr, (double*)grad_segs->ptr,
                    part.as<double>(), (unsigned*)status->ptr);
    SVGR_LAUNCH(k_cover_vjp_m6, grid1((size_t)g.n_paths, 64), dim3(64), 0, st, (const double*)part.p, g.seg_off, g.n_segs, g.n_paths, (double*)grad_m6->ptr);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" {
int svgr_cover_block(void) { return COVER_BLOCK; }
int svgr_cover_scan(void) { return COVER_SCAN; }

int svgr_cover_forward(svgr_ctx* ctx, const svgr_cover_desc* desc, const svgr_buf* segs, const svgr_buf* seg_kind, const svgr_buf* path_seg_off,
                       const svgr_buf* path_m6, const svgr_buf* path_rule, svgr_buf* cover, svgr_buf* slope, svgr_buf* status) {
    return abi_guard("svgr_cover_forward", [&]() { return cover_forward_impl(ctx, desc, segs, seg_kind, path_seg_off, path_m6, path_rule, cover, slope, status); });
}

int svgr_cover_backward(svgr_ctx* ctx, const svgr_cover_desc* desc, const svgr_buf* segs, const svgr_buf* seg_kind, const svgr_buf* path_seg_off,
                        const svgr_buf* path_m6, const svgr_buf* slope, const svgr_buf* grad_out, svgr_buf* grad_segs, svgr_buf* grad_m6,
                        svgr_buf* status) {
    return abi_guard("svgr_cover_backward", [&]() { return cover_backward_impl(ctx, desc, segs, seg_kind, path_seg_off, path_m6, slope, grad_out, grad_segs, grad_m6, status); });
}
}  // extern "C"

// ======================================================================================
// differentiable compositing: one compositor in four tiers, an entry pair each (DESIGN.md 7x has the scheme and the derivations)
//   solid    svgr_compose_forward / _backward           solid fills source-over in paint order (csrc/svgr_compose.h)
//   painted  svgr_compose_painted_forward / _backward   a fill is solid or a linear / radial gradient (csrc/svgr_gradpaint.h)
//   grouped  svgr_compose_grouped_forward / _backward   a PROGRAM of FILL / BEGIN / END items: isolated groups with an opacity, a
//                                                       clip mask, both or neither (csrc/svgr_group.h)
//   masked   svgr_compose_masked_forward / _backward    the program's HOLD and END_MASK: luminance-masked groups (csrc/svgr_mask.h)
// A tier computes what the one below computes, bit for bit, on input that does not use what it adds.  That holds because the
// pieces below are written once and every tier's kernels are built from them:
//   compose_px_load / _store    the four channels of a pixel as one vector
//   wave_sum                    the fixed 32-to-1 shuffle tree
//   ComposeIn                   the wave-uniform read-only inputs, built inside each kernel from its own restrict parameters
//                               (uniform addresses of restrict pointers: scalar loads)
//   compose_fill / compose_fill_through / compose_fill_vjp
//                               a FILL in the forward, in walk 1 (T_p into the plane's slot) and in walk 2 (d / d m_p over T_p, the
//                               4 or 14 dense terms and 5 per stop reduced over the wave into given LDS rows; nothing where no
//                               lane of the wave is covered)
//   compose_clip_mask / compose_clip_vjp    a clip's planes composed to one mask, and their gradient
//   compose_sums_clear / compose_sums_flush the waves' LDS rows: added in wave order, at barriers, into the workgroup's own row of
//                               partials; no atomics
//   program_need, program_forward_px        the LDS slots of an item; one pixel of a program's forward
// Kernels: a pair per tier, so that each keeps its own footprint.  k_compose_over / k_compose_vjp (solid: a leaner 4-slot layout,
// COMPOSE_CHUNK paths between two flushes), k_compose_over_painted / k_compose_vjp_painted (a flat list of paths, the stops' rows
// after all dense rows of a run), k_compose_over_program<T, MASKS> / k_compose_vjp_program<T, MASKS> (an item table, an item's
// stop rows after its own dense row; MASKS is the compile-time tier: the grouped instantiation holds none of the masked one's
// LDS, ops or walk 0).  k_compose_paint_sum (solid) and k_compose_param_sum (the others) add the workgroups' partials in
// workgroup order.  The host tables go up as kernel ARGUMENTS (k_painted_topology, k_group_program): no copy from memory the
// caller may free on return.  No host read-back between the launches; nothing waits.  The renderer's kernels and the coverage
// kernels are not involved.
// ======================================================================================
#include "svgr_compose.h"
#include "svgr_gradpaint.h"
#include "svgr_group.h"
#include "svgr_mask.h"

constexpr int COMPOSE_BLOCK = 256;                  // pixels per workgroup step: a lane each, four waves
constexpr int COMPOSE_WAVES = COMPOSE_BLOCK / 64;
constexpr int COMPOSE_GROUPS = 512;                 // the workgroup cap of the backward kernels: two per CU
constexpr int COMPOSE_CHUNK = COMPOSE_BLOCK / 4;    // solid: paths whose sums sit in LDS between two flushes, a lane per (path, channel)
constexpr int PAINTED_TOPO = 384;     // paths per k_painted_topology launch: 3 ints each, within the 4 KiB of kernel arguments
constexpr int PAINTED_SLOTS = 1024;   // parameters of one run of paths or items in LDS, per wave (a path has at most 14 + 5 * 32 = 174)
constexpr int GROUPED_INTS = 960;     // ints per k_group_program launch: within the 4 KiB of kernel arguments
static_assert(GRADPAINT_DENSE + GRADPAINT_STOP * GRADPAINT_MAX_STOPS <= PAINTED_SLOTS, "a path's parameters fit one run");
static_assert(GRADPAINT_MAX_STOPS == GRAD_MAX_STOPS, "one cap");

struct ComposeBg { double c[4]; };
struct PaintedView { long long row0, col0; unsigned cols; };
template <class T> struct ComposePx;
template <> struct ComposePx<float> { using type = float4; };
template <> struct ComposePx<double> { using type = double4; };

template <class T>
__device__ __forceinline__ void compose_px_load(const T* image, size_t i, double* c) {
    const typename ComposePx<T>::type v = reinterpret_cast<const typename ComposePx<T>::type*>(image)[i];
    c[0] = (double)v.x; c[1] = (double)v.y; c[2] = (double)v.z; c[3] = (double)v.w;
}

template <class T>
__device__ __forceinline__ void compose_px_store(T* image, size_t i, const double* c) {
    typename ComposePx<T>::type v;
    v.x = (T)c[0]; v.y = (T)c[1]; v.z = (T)c[2]; v.w = (T)c[3];
    reinterpret_cast<typename ComposePx<T>::type*>(image)[i] = v;
}

__device__ __forceinline__ double wave_sum(double v) {
    for (int d = 32; d > 0; d >>= 1) v = v + __shfl_down(v, d);
    return v;
}

// ---- solid ----
template <class T>
__global__ __launch_bounds__(COMPOSE_BLOCK) void k_compose_over(const T* __restrict__ cover, const double* __restrict__ paints, const ComposeBg bg,
                                                                int n_paths, size_t n_px, T* __restrict__ image) {
    const size_t i = (size_t)blockIdx.x * COMPOSE_BLOCK + threadIdx.x;
    if (i >= n_px) return;
    double C[4] = {bg.c[0], bg.c[1], bg.c[2], bg.c[3]};
#pragma unroll 4
    for (int p = 0; p < n_paths; ++p) compose_step(C, (double)cover[(size_t)p * n_px + i], paints + 4 * (size_t)p);
    compose_px_store(image, i, C);
}

// a lane per pixel, at most COMPOSE_GROUPS workgroups striding over the pixels.  Walk 1 goes from the top path down and leaves T_p
// in the pixel's grad_cover slot; walk 2 goes from the bottom up, carries the canvas as the forward does, writes d / d m_p over
// T_p and reduces the four paint terms of every path.
// (through and grad_cover are the same memory for double planes: a lane reads its own T_p before it writes d / d m_p there)
template <class T>
__global__ __launch_bounds__(COMPOSE_BLOCK) void k_compose_vjp(const T* __restrict__ cover, const double* __restrict__ paints, const ComposeBg bg,
                                                               int n_paths, size_t n_px, const T* __restrict__ grad_image, double* through,
                                                               T* grad_cover, double* __restrict__ part) {
    __shared__ double sums[COMPOSE_WAVES][COMPOSE_CHUNK][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int fq = threadIdx.x >> 2, fk = threadIdx.x & 3;   // the (path of the chunk, channel) this lane flushes
    double* mine = part + (size_t)blockIdx.x * (size_t)n_paths * 4;
    SVGR_UNROLL
    for (int w = 0; w < COMPOSE_WAVES; ++w) sums[w][fq][fk] = 0.0;
    __syncthreads();
    for (size_t base = (size_t)blockIdx.x * COMPOSE_BLOCK; base < n_px; base += (size_t)gridDim.x * COMPOSE_BLOCK) {
        const size_t i = base + threadIdx.x;
        const bool live = i < n_px;
        double gi[4] = {0.0, 0.0, 0.0, 0.0};
        if (live) {
            double above = 1.0;   // T_p: what the paths above p let through
            for (int p = n_paths - 1; p >= 0; --p) {
                const size_t at = (size_t)p * n_px + i;
                through[at] = above;
                above = above * compose_through((double)cover[at], paints[4 * (size_t)p + 3]);
            }
            compose_px_load(grad_image, i, gi);
        }
        double C[4] = {bg.c[0], bg.c[1], bg.c[2], bg.c[3]};
        for (int p0 = 0; p0 < n_paths; p0 += COMPOSE_CHUNK) {
            const int p1 = p0 + COMPOSE_CHUNK < n_paths ? p0 + COMPOSE_CHUNK : n_paths;
            for (int p = p0; p < p1; ++p) {
                const double* paint = paints + 4 * (size_t)p;
                double m = 0.0, t[4] = {0.0, 0.0, 0.0, 0.0};
                if (live) {
                    const size_t at = (size_t)p * n_px + i;
                    m = (double)cover[at];
                    const double dm = compose_vjp_step(C, through[at], gi, m, paint, t);
                    grad_cover[at] = (T)dm;
                    compose_step(C, m, paint);
                }
                if (__ballot(m != 0.0) == 0ull) continue;   // (the same in every lane of the wave; a lane past the end has m == 0)
                SVGR_UNROLL
                for (int k = 0; k < 4; ++k) t[k] = wave_sum(t[k]);
                if (lane == 0) {
                    double* s = sums[wave][p - p0];
                    s[0] = s[0] + t[0]; s[1] = s[1] + t[1]; s[2] = s[2] + t[2]; s[3] = s[3] + t[3];
                }
            }
            __syncthreads();
            if (p0 + fq < p1) {
                double s = sums[0][fq][fk];
                SVGR_UNROLL
                for (int w = 1; w < COMPOSE_WAVES; ++w) s = s + sums[w][fq][fk];
                double* o = mine + 4 * (size_t)(p0 + fq) + fk;
                *o = *o + s;
            }
            SVGR_UNROLL
            for (int w = 0; w < COMPOSE_WAVES; ++w) sums[w][fq][fk] = 0.0;
            __syncthreads();
        }
    }
}

// a lane per (path, channel): the workgroups' partials added in workgroup order
__global__ __launch_bounds__(64) void k_compose_paint_sum(const double* __restrict__ part, int n_groups, size_t n4, double* __restrict__ grad_paints) {
    const size_t j = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (j >= n4) return;
    double s = 0.0;
    for (int g = 0; g < n_groups; ++g) s = s + part[(size_t)g * n4 + j];
    grad_paints[j] = s;
}

// ---- what the painted and the program kernels share ----
// The wave-uniform read-only inputs.  A kernel builds this from its own restrict parameters; it is never a kernel argument.
// The painted tier has no program: items, clip_off, clip_planes and opacity are null there.
template <class T>
struct ComposeIn {
    const T* cover;
    const double* paints;
    const int4* desc;          // {kind, spread, first stop, end stop} per path
    const double *m6s, *geoms, *pos, *rgba;
    const int4* items;         // {0, p, 0, 0}, {1 | 2, g, opacity slot or -1, clip or -1}, and svgr_mask.h's
    const int *clip_off, *clip_planes;
    const double* opacity;
    PaintedView vw;
    size_t n_px;
};

struct ComposeAt { size_t i; unsigned row, colj; };   // a lane's pixel

__device__ __forceinline__ ComposeAt compose_at(const PaintedView vw, size_t i, bool live) {   // (n_px < 2^31)
    ComposeAt px;
    px.i = i;
    px.row = live ? (unsigned)i / vw.cols : 0u;
    px.colj = live ? (unsigned)i - px.row * vw.cols : 0u;
    return px;
}

// the colour of gradient path p, d its description, at the pixel
template <class T>
__device__ __forceinline__ void compose_fill_colour(const ComposeIn<T>& in, int p, const int4 d, const ComposeAt px, double* col, GradPaintPx& e) {
    gradpaint_colour(d.x, d.y, in.m6s + 6 * (size_t)p, in.geoms + 4 * (size_t)p, d.w - d.z, in.pos + d.z, in.rgba + 4 * (size_t)d.z, px.row, px.colj,
                     in.vw.row0, in.vw.col0, col, e);
}

// forward: path p over the canvas X
template <class T>
__device__ __forceinline__ void compose_fill(const ComposeIn<T>& in, int p, const ComposeAt px, double* X) {
    const int4 d = in.desc[p];
    const double m = (double)in.cover[(size_t)p * in.n_px + px.i];
    if (d.x == 0) {
        compose_step(X, m, in.paints + 4 * (size_t)p);
    } else {
        double col[4];
        GradPaintPx e;
        compose_fill_colour(in, p, d, px, col, e);
        gradpaint_step(X, m, col, in.paints + 4 * (size_t)p);
    }
}

// walk 1: parks `above` (T_p) in the plane's slot and returns what path p lets through
template <class T>
__device__ __forceinline__ double compose_fill_through(const ComposeIn<T>& in, int p, const ComposeAt px, double above, double* through) {
    const int4 d = in.desc[p];
    const size_t at = (size_t)p * in.n_px + px.i;
    const double m = (double)in.cover[at];
    double u;
    if (d.x == 0) {
        u = compose_through(m, in.paints[4 * (size_t)p + 3]);
    } else {
        double col[4];
        GradPaintPx e;
        compose_fill_colour(in, p, d, px, col, e);
        u = gradpaint_through(m, col, in.paints + 4 * (size_t)p);
    }
    through[at] = above;
    return u;
}

// walk 2: d / d m_p over T_p, path p over the canvas X, and the path's terms summed over the wave into rowd (4 for a solid
// path, GRADPAINT_DENSE for a gradient) and rows (GRADPAINT_STOP per stop, only the stops some lane of the wave used).  B is
// the adjoint of X.  Nothing is added where no lane of the wave is covered.
template <class T>
__device__ __forceinline__ void compose_fill_vjp(const ComposeIn<T>& in, int p, const int4 d, bool live, const ComposeAt px, const double* through,
                                                 T* grad_cover, double* X, const double* B, int lane, double* rowd, double* rows) {
    const double* paint = in.paints + 4 * (size_t)p;
    double m = 0.0, dense[GRADPAINT_DENSE], lo[GRADPAINT_STOP], hi[GRADPAINT_STOP];
    SVGR_UNROLL
    for (int k = 0; k < GRADPAINT_DENSE; ++k) dense[k] = 0.0;
    SVGR_UNROLL
    for (int k = 0; k < GRADPAINT_STOP; ++k) lo[k] = hi[k] = 0.0;
    int used_lo = -1, used_hi = -1;
    if (live) {
        const size_t at = (size_t)p * in.n_px + px.i;
        m = (double)in.cover[at];
        if (d.x == 0) {
            const double dm = compose_vjp_step(X, through[at], B, m, paint, dense);
            grad_cover[at] = (T)dm;
            compose_step(X, m, paint);
        } else {
            double col[4], P[4], t[4];
            GradPaintPx e;
            compose_fill_colour(in, p, d, px, col, e);
            gradpaint_effective(col, paint, P);
            const double dm = compose_vjp_step(X, through[at], B, m, P, t);
            grad_cover[at] = (T)dm;
            gradpaint_vjp(d.x, in.geoms + 4 * (size_t)p, in.pos + d.z, in.rgba + 4 * (size_t)d.z, col, paint, e, t, dense, lo, hi);
            gradpaint_step(X, m, col, paint);
            used_lo = e.lo;
            used_hi = e.hi;
        }
    }
    if (__ballot(m != 0.0) == 0ull) return;   // (the same in every lane of the wave; a lane past the end has m == 0)
    if (d.x == 0) {
        SVGR_UNROLL
        for (int k = 0; k < 4; ++k) dense[k] = wave_sum(dense[k]);
        if (lane == 0) {
            SVGR_UNROLL
            for (int k = 0; k < 4; ++k) rowd[k] = rowd[k] + dense[k];
        }
        return;
    }
    SVGR_UNROLL
    for (int k = 0; k < GRADPAINT_DENSE; ++k) dense[k] = wave_sum(dense[k]);
    if (lane == 0) {
        SVGR_UNROLL
        for (int k = 0; k < GRADPAINT_DENSE; ++k) rowd[k] = rowd[k] + dense[k];
    }
    const int ns = d.w - d.z;
    for (int s = 0; s < ns; ++s) {
        const bool at_lo = used_lo == s, at_hi = used_hi == s;
        if (__ballot(m != 0.0 && (at_lo || at_hi)) == 0ull) continue;
        double v[GRADPAINT_STOP];
        SVGR_UNROLL
        for (int k = 0; k < GRADPAINT_STOP; ++k) v[k] = wave_sum(at_lo ? lo[k] : (at_hi ? hi[k] : 0.0));
        if (lane == 0) {
            SVGR_UNROLL
            for (int k = 0; k < GRADPAINT_STOP; ++k) rows[GRADPAINT_STOP * s + k] = rows[GRADPAINT_STOP * s + k] + v[k];
        }
    }
}

// the mask of clip `clip`: its planes composed OVER in one channel; 1 without a clip
template <class T>
__device__ __forceinline__ double compose_clip_mask(const ComposeIn<T>& in, int clip, size_t i) {
    if (clip < 0) return 1.0;
    const int a0 = in.clip_off[clip], a1 = in.clip_off[clip + 1];
    double k = 0.0;
    for (int a = a0; a < a1; ++a) k = group_mask_step(k, (double)in.cover[(size_t)in.clip_planes[a] * in.n_px + i], a == a0);
    return k;
}

// walk 2 at the closer of a clipped group: d / d m of every clip plane from dk = d / d k, the planes' suffix products parked in
// their own slots as T_p is.  Returns the mask.
template <class T>
__device__ __forceinline__ double compose_clip_vjp(const ComposeIn<T>& in, int clip, size_t i, double dk, double* through, T* grad_cover) {
    if (clip < 0) return 1.0;
    const int a0 = in.clip_off[clip], a1 = in.clip_off[clip + 1];
    double suffix = 1.0;
    for (int a = a1 - 1; a >= a0; --a) {
        const size_t at = (size_t)in.clip_planes[a] * in.n_px + i;
        through[at] = suffix;
        suffix = suffix * (1.0 - (double)in.cover[at]);
    }
    double k = 0.0;
    for (int a = a0; a < a1; ++a) {
        const size_t at = (size_t)in.clip_planes[a] * in.n_px + i;
        const double dm = group_clip_vjp(dk, a == a0, k, through[at]);
        grad_cover[at] = (T)dm;
        k = group_mask_step(k, (double)in.cover[at], a == a0);
    }
    return k;
}

// the waves' LDS rows of parameter sums, PAINTED_SLOTS each
__device__ __forceinline__ void compose_sums_clear(double (*sums)[PAINTED_SLOTS]) {
    for (int j = threadIdx.x; j < PAINTED_SLOTS; j += COMPOSE_BLOCK) {
        SVGR_UNROLL
        for (int w = 0; w < COMPOSE_WAVES; ++w) sums[w][j] = 0.0;
    }
}

// (between two barriers) slots slot .. slot + need - 1, added in wave order and cleared: the first `split` of them go to
// mine[first_at ..], the others to mine[rest_at ..]
__device__ __forceinline__ void compose_sums_flush(double (*sums)[PAINTED_SLOTS], int slot, int need, int split, double* mine, size_t first_at,
                                                   size_t rest_at) {
    for (int j = threadIdx.x; j < need; j += COMPOSE_BLOCK) {
        double s = sums[0][slot + j];
        SVGR_UNROLL
        for (int w = 1; w < COMPOSE_WAVES; ++w) s = s + sums[w][slot + j];
        double* o = mine + (j < split ? first_at + (size_t)j : rest_at + (size_t)(j - split));
        *o = *o + s;
        SVGR_UNROLL
        for (int w = 0; w < COMPOSE_WAVES; ++w) sums[w][slot + j] = 0.0;
    }
}

// a lane per parameter: the workgroups' partials added in workgroup order, stored to the array the parameter belongs to.  The
// parameters are 14 per path, then 5 per stop, then (from n_stop_end on; the painted tier has none) one per opacity.
__global__ __launch_bounds__(64) void k_compose_param_sum(const double* __restrict__ part, int n_groups, size_t n_dense, size_t n_stop_end, size_t n_params,
                                                          double* __restrict__ g_paints, double* __restrict__ g_m6, double* __restrict__ g_geom,
                                                          double* __restrict__ g_pos, double* __restrict__ g_rgba, double* __restrict__ g_opacity) {
    const size_t j = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (j >= n_params) return;
    double s = 0.0;
    for (int g = 0; g < n_groups; ++g) s = s + part[(size_t)g * n_params + j];
    if (j < n_dense) {
        const size_t p = j / GRADPAINT_DENSE;
        const int k = (int)(j - p * GRADPAINT_DENSE);
        if (k < 4) g_paints[4 * p + k] = s;
        else if (k < 10) g_m6[6 * p + (k - 4)] = s;
        else g_geom[4 * p + (k - 10)] = s;
    } else if (j < n_stop_end) {
        const size_t q = (j - n_dense) / GRADPAINT_STOP;
        const int k = (int)((j - n_dense) - q * GRADPAINT_STOP);
        if (k == 0) g_pos[q] = s;
        else g_rgba[4 * q + (k - 1)] = s;
    } else {
        g_opacity[j - n_stop_end] = s;
    }
}

// ---- painted: a flat list of paths ----
struct PaintedTopo {
    int first, n;
    int kind_spread[PAINTED_TOPO];     // kind | spread << 8
    int stop_off[PAINTED_TOPO + 1];
};

__global__ __launch_bounds__(64) void k_painted_topology(const PaintedTopo t, int4* __restrict__ desc) {
    const int q = (int)(blockIdx.x * 64 + threadIdx.x);
    if (q >= t.n) return;
    desc[t.first + q] = make_int4(t.kind_spread[q] & 255, t.kind_spread[q] >> 8, t.stop_off[q], t.stop_off[q + 1]);
}

template <class T>
__global__ __launch_bounds__(COMPOSE_BLOCK) void k_compose_over_painted(const T* __restrict__ cover, const double* __restrict__ paints,
                                                                        const int4* __restrict__ desc, const double* __restrict__ m6s,
                                                                        const double* __restrict__ geoms, const double* __restrict__ pos,
                                                                        const double* __restrict__ rgba, const ComposeBg bg, const PaintedView vw,
                                                                        int n_paths, size_t n_px, T* __restrict__ image) {
    const ComposeIn<T> in = {cover, paints, desc, m6s, geoms, pos, rgba, nullptr, nullptr, nullptr, nullptr, vw, n_px};
    const size_t i = (size_t)blockIdx.x * COMPOSE_BLOCK + threadIdx.x;
    if (i >= n_px) return;
    const ComposeAt px = compose_at(vw, i, true);
    double C[4] = {bg.c[0], bg.c[1], bg.c[2], bg.c[3]};
    for (int p = 0; p < n_paths; ++p) compose_fill(in, p, px, C);
    compose_px_store(image, i, C);
}

// The two walks of k_compose_vjp.  The waves' sums sit in LDS for a run of paths whose parameters fit PAINTED_SLOTS: the paths'
// dense rows first, then their stops' rows (both contiguous in the partials: n_params = 14 n_paths + 5 n_stops).
// (through and grad_cover are the same memory for double planes, as in k_compose_vjp)
template <class T>
__global__ __launch_bounds__(COMPOSE_BLOCK) void k_compose_vjp_painted(const T* __restrict__ cover, const double* __restrict__ paints,
                                                                       const int4* __restrict__ desc, const double* __restrict__ m6s,
                                                                       const double* __restrict__ geoms, const double* __restrict__ pos,
                                                                       const double* __restrict__ rgba, const ComposeBg bg, const PaintedView vw,
                                                                       int n_paths, int n_stops, size_t n_px, const T* __restrict__ grad_image,
                                                                       double* through, T* grad_cover, double* __restrict__ part) {
    __shared__ double sums[COMPOSE_WAVES][PAINTED_SLOTS];
    const ComposeIn<T> in = {cover, paints, desc, m6s, geoms, pos, rgba, nullptr, nullptr, nullptr, nullptr, vw, n_px};
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t n_dense = (size_t)GRADPAINT_DENSE * (size_t)n_paths;
    double* mine = part + (size_t)blockIdx.x * (n_dense + (size_t)GRADPAINT_STOP * (size_t)n_stops);
    compose_sums_clear(sums);
    __syncthreads();
    for (size_t base = (size_t)blockIdx.x * COMPOSE_BLOCK; base < n_px; base += (size_t)gridDim.x * COMPOSE_BLOCK) {
        const size_t i = base + threadIdx.x;
        const bool live = i < n_px;
        const ComposeAt px = compose_at(vw, i, live);
        double gi[4] = {0.0, 0.0, 0.0, 0.0};
        if (live) {
            double above = 1.0;   // T_p: what the paths above p let through
            for (int p = n_paths - 1; p >= 0; --p) above = above * compose_fill_through(in, p, px, above, through);
            compose_px_load(grad_image, i, gi);
        }
        double C[4] = {bg.c[0], bg.c[1], bg.c[2], bg.c[3]};
        int p0 = 0;
        while (p0 < n_paths) {
            // the run of paths p0 .. p1 - 1 whose parameters fit the LDS rows
            const int s_first = desc[p0].z;
            int p1 = p0, used = 0;
            while (p1 < n_paths) {
                const int4 d = desc[p1];
                const int need = GRADPAINT_DENSE + GRADPAINT_STOP * (d.w - d.z);
                if (used + need > PAINTED_SLOTS) break;
                used += need;
                ++p1;
            }
            const int nd = GRADPAINT_DENSE * (p1 - p0);
            for (int p = p0; p < p1; ++p) {
                const int4 d = desc[p];
                compose_fill_vjp(in, p, d, live, px, through, grad_cover, C, gi, lane, &sums[wave][GRADPAINT_DENSE * (p - p0)],
                                 &sums[wave][nd + GRADPAINT_STOP * (d.z - s_first)]);
            }
            __syncthreads();
            compose_sums_flush(sums, 0, used, nd, mine, (size_t)GRADPAINT_DENSE * (size_t)p0, n_dense + (size_t)GRADPAINT_STOP * (size_t)s_first);
            __syncthreads();
            p0 = p1;
        }
    }
}

// ---- grouped and masked: a program of items; MASKS is the tier ----
// The canvas of the open level is in registers; the levels below it sit in LDS, a column per lane, indexed by the wave-uniform
// level: no private array, no scratch.  The masked tier adds the held group H = (G o) k_clip of the pair open on a level, in LDS
// too, and the mask canvas M of every pair parked in four planes of the call's scratch, as T_end is parked per group: walk 1
// needs k_mask and walk 2 d k / d M before either arrives at the mask group.
struct GroupSlice {
    int first, n;
    int v[GROUPED_INTS];
};

__global__ __launch_bounds__(64) void k_group_program(const GroupSlice t, int* __restrict__ table) {
    const int q = (int)(blockIdx.x * 64 + threadIdx.x);
    if (q >= t.n) return;
    table[t.first + q] = t.v[q];
}

struct GroupedProgram {
    const int4* items;        // in the kernels' form (svgr_group.h, svgr_mask.h)
    const int* clip_off;
    const int* clip_planes;
    int n_items;
};

template <bool MASKS>
__device__ __forceinline__ int program_op(int x) {
    if constexpr (MASKS) return mask_op(x);
    else return x;
}

// the LDS slots an item's parameters take in a run: a FILL's 14 dense terms and 5 per stop, the opacity of an END or a HOLD
template <bool MASKS>
__device__ __forceinline__ int program_need(const int4 it, const int4* __restrict__ desc) {
    const int op = program_op<MASKS>(it.x);
    if (op == GROUP_FILL) {
        const int4 d = desc[it.y];
        return GRADPAINT_DENSE + GRADPAINT_STOP * (d.w - d.z);
    }
    return (op == GROUP_END || (MASKS && op == MASK_HOLD)) && it.z >= 0 ? 1 : 0;
}

// level `level` of a lane's column: the canvas X goes below and a transparent one opens / X comes back.  Walk 2 keeps the
// canvas' adjoint B in the column's rows 4 .. 7.
template <int BELOW>
__device__ __forceinline__ void program_push(double (*below)[BELOW][COMPOSE_BLOCK], int level, double* X) {
    SVGR_UNROLL
    for (int c = 0; c < 4; ++c) {
        below[level][c][threadIdx.x] = X[c];
        X[c] = 0.0;
    }
}

template <int BELOW>
__device__ __forceinline__ void program_pop(double (*below)[BELOW][COMPOSE_BLOCK], int level, double* X) {
    SVGR_UNROLL
    for (int c = 0; c < 4; ++c) X[c] = below[level][c][threadIdx.x];
}

__device__ __forceinline__ void program_push_adjoint(double (*below)[8][COMPOSE_BLOCK], int level, double* X, const double* B) {
    program_push(below, level, X);
    SVGR_UNROLL
    for (int c = 0; c < 4; ++c) below[level][4 + c][threadIdx.x] = B[c];
}

__device__ __forceinline__ void program_pop_adjoint(double (*below)[8][COMPOSE_BLOCK], int level, double* X, double* B) {
    program_pop(below, level, X);
    SVGR_UNROLL
    for (int c = 0; c < 4; ++c) B[c] = below[level][4 + c][threadIdx.x];
}

// M of a pair from its four planes
__device__ __forceinline__ void masked_parked(const double* park, int pair, size_t n_px, size_t i, double* M) {
    const size_t at = (size_t)pair * 4 * n_px + i;
    SVGR_UNROLL
    for (int c = 0; c < 4; ++c) M[c] = park[at + (size_t)c * n_px];
}

// one pixel of the forward over items[0 .. n_run): X is the root canvas on entry and on return.  below has BELOW rows per level
// (the canvas in the first four).  Masked tier only: held, and park, which if not null gets M of every pair (walk 0).
template <class T, bool MASKS, int BELOW>
__device__ __forceinline__ void program_forward_px(const ComposeIn<T>& in, int n_run, const ComposeAt px, double (*below)[BELOW][COMPOSE_BLOCK],
                                                   double (*held)[4][COMPOSE_BLOCK], double* park, double* X) {
    int level = 0;
    for (int q = 0; q < n_run; ++q) {
        const int4 it = in.items[q];
        const int op = program_op<MASKS>(it.x);
        // (how the op chains of this template read: a `MASKS && ...` arm is dead in the grouped instantiation; a `!MASKS || ...` arm
        // is the grouped tier's catch-all, its last op; what follows it, under `if constexpr (MASKS)`, exists in the masked one only)
        if (op == GROUP_FILL) {
            compose_fill(in, it.y, px, X);
        } else if (op == GROUP_BEGIN || (MASKS && (op == MASK_BEGIN_HELD || op == MASK_BEGIN_MASK))) {
            program_push(below, level, X);
            ++level;
        } else if (!MASKS || op == GROUP_END) {   // (grouped: whatever is left is an END)
            --level;
            const double o = it.z < 0 ? 1.0 : in.opacity[it.z];
            const double k = compose_clip_mask(in, it.w, px.i);
            const double G[4] = {X[0], X[1], X[2], X[3]};
            program_pop(below, level, X);
            group_step(X, G, o, k);
        } else if constexpr (MASKS) {
            --level;
            if (op == MASK_HOLD) {
                const double o = it.z < 0 ? 1.0 : in.opacity[it.z];
                const double k = compose_clip_mask(in, it.w, px.i);
                double H[4];
                mask_hold(X, o, k, H);
                SVGR_UNROLL
                for (int c = 0; c < 4; ++c) held[level][c][threadIdx.x] = H[c];
                program_pop(below, level, X);
            } else {   // MASK_END
                const double M[4] = {X[0], X[1], X[2], X[3]};
                if (park) {
                    const size_t at = (size_t)mask_pair(it.x) * 4 * in.n_px + px.i;
                    SVGR_UNROLL
                    for (int c = 0; c < 4; ++c) park[at + (size_t)c * in.n_px] = M[c];
                }
                double H[4];
                program_pop(below, level, X);
                SVGR_UNROLL
                for (int c = 0; c < 4; ++c) H[c] = held[level][c][threadIdx.x];
                mask_step(X, H, mask_value(M));
            }
        }
    }
}

template <class T, bool MASKS>
__global__ __launch_bounds__(COMPOSE_BLOCK) void k_compose_over_program(const T* __restrict__ cover, const double* __restrict__ paints,
                                                                        const int4* __restrict__ desc, const double* __restrict__ m6s,
                                                                        const double* __restrict__ geoms, const double* __restrict__ pos,
                                                                        const double* __restrict__ rgba, const int4* __restrict__ items,
                                                                        const int* __restrict__ clip_off, const int* __restrict__ clip_planes,
                                                                        const double* __restrict__ opacity, const ComposeBg bg, const PaintedView vw,
                                                                        int n_items, size_t n_px, T* __restrict__ image) {
    __shared__ double below[GROUP_DEPTH][4][COMPOSE_BLOCK];   // the canvases under the open level, a column per lane
    double (*held)[4][COMPOSE_BLOCK] = nullptr;
    if constexpr (MASKS) {
        __shared__ double held_lds[GROUP_DEPTH][4][COMPOSE_BLOCK];   // the held group of the pair open on a level
        held = held_lds;
    }
    const ComposeIn<T> in = {cover, paints, desc, m6s, geoms, pos, rgba, items, clip_off, clip_planes, opacity, vw, n_px};
    const size_t i = (size_t)blockIdx.x * COMPOSE_BLOCK + threadIdx.x;
    if (i >= n_px) return;   // (no barrier below: a lane reads its own column only)
    double X[4] = {bg.c[0], bg.c[1], bg.c[2], bg.c[3]};
    program_forward_px<T, MASKS, 4>(in, n_items, compose_at(vw, i, true), below, held, nullptr, X);
    compose_px_store(image, i, X);
}

// The two walks of svgr_group.h and svgr_mask.h.  Walk 1 needs no stack (T_end is a plane per group in memory).  Walk 2 keeps
// canvas and base adjoint of the open level in registers and those below in LDS.  Parameter sums as in k_compose_vjp_painted, for a
// run of ITEMS whose parameters fit PAINTED_SLOTS, each item's slots after the one before; an opacity is one more slot after
// the stops: n_params = 14 n_paths + 5 n_stops + n_opacities.  Masked tier: walk 0 is the forward over the first n_walk0 items
// (to the last END_MASK) and parks M of every pair; a program without pairs skips it and takes the grouped steps: the same bits.
// The grouped tier passes n_walk0 = 0 and no park.
// (through and grad_cover are the same memory for double planes, as in k_compose_vjp)
template <class T, bool MASKS>
__global__ __launch_bounds__(COMPOSE_BLOCK) void k_compose_vjp_program(const T* __restrict__ cover, const double* __restrict__ paints,
                                                                       const int4* __restrict__ desc, const double* __restrict__ m6s,
                                                                       const double* __restrict__ geoms, const double* __restrict__ pos,
                                                                       const double* __restrict__ rgba, const int4* __restrict__ items,
                                                                       const int* __restrict__ clip_off, const int* __restrict__ clip_planes,
                                                                       const double* __restrict__ opacity, const ComposeBg bg, const PaintedView vw,
                                                                       int n_items, int n_walk0, int n_paths, int n_stops, int n_opacities, size_t n_px,
                                                                       const T* __restrict__ grad_image, double* through, T* grad_cover,
                                                                       double* __restrict__ t_end, double* park, double* __restrict__ part) {
    __shared__ double sums[COMPOSE_WAVES][PAINTED_SLOTS];
    __shared__ double below[GROUP_DEPTH][8][COMPOSE_BLOCK];   // canvas and base adjoint of the levels under the open one, a column per lane
    double (*held)[4][COMPOSE_BLOCK] = nullptr;
    if constexpr (MASKS) {
        __shared__ double held_lds[GROUP_DEPTH][4][COMPOSE_BLOCK];   // the held group of the pair open on a level
        held = held_lds;
    }
    const ComposeIn<T> in = {cover, paints, desc, m6s, geoms, pos, rgba, items, clip_off, clip_planes, opacity, vw, n_px};
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t n_dense = (size_t)GRADPAINT_DENSE * (size_t)n_paths;
    const size_t n_stop_end = n_dense + (size_t)GRADPAINT_STOP * (size_t)n_stops;
    double* mine = part + (size_t)blockIdx.x * (n_stop_end + (size_t)n_opacities);
    compose_sums_clear(sums);
    __syncthreads();
    for (size_t base = (size_t)blockIdx.x * COMPOSE_BLOCK; base < n_px; base += (size_t)gridDim.x * COMPOSE_BLOCK) {
        const size_t i = base + threadIdx.x;
        const bool live = i < n_px;
        const ComposeAt px = compose_at(vw, i, live);
        double B[4] = {0.0, 0.0, 0.0, 0.0};
        if (live) {
            if constexpr (MASKS) {
                if (n_walk0 > 0) {   // walk 0: the lane reads back below only what it parks here itself
                    double X0[4] = {bg.c[0], bg.c[1], bg.c[2], bg.c[3]};
                    program_forward_px<T, true, 8>(in, n_walk0, px, below, held, park, X0);
                }
            }
            double above = 1.0;
            for (int q = n_items - 1; q >= 0; --q) {
                const int4 it = items[q];
                const int op = program_op<MASKS>(it.x);
                if (op == GROUP_FILL) {
                    above = above * compose_fill_through(in, it.y, px, above, through);
                } else if (op == GROUP_END) {
                    t_end[(size_t)it.y * n_px + i] = above;
                    above = 1.0;
                } else if (MASKS && op == MASK_END) {
                    t_end[(size_t)it.z * n_px + i] = above;   // (of the pair's target)
                    above = 1.0;
                } else if (MASKS && op == MASK_HOLD) {
                    above = 1.0;
                } else if (!MASKS || op == GROUP_BEGIN) {   // (grouped: whatever is left is a BEGIN; the MASKS arms above are dead there)
                    const double o = it.z < 0 ? 1.0 : opacity[it.z];
                    const double k = compose_clip_mask(in, it.w, i);
                    const double u = group_through(above, o, k);
                    above = t_end[(size_t)it.y * n_px + i] * u;
                } else if constexpr (MASKS) {
                    if (op == MASK_BEGIN_HELD) {
                        const double o = it.z < 0 ? 1.0 : opacity[it.z];
                        const double k = compose_clip_mask(in, it.w, i);
                        double M[4];
                        masked_parked(park, mask_pair(it.x), n_px, i, M);
                        const double u = mask_through(above, o, k, mask_value(M));
                        above = t_end[(size_t)it.y * n_px + i] * u;
                    }   // (the BEGIN of a mask group: nothing carries over)
                }
            }
            compose_px_load(grad_image, i, B);
        }
        double X[4] = {bg.c[0], bg.c[1], bg.c[2], bg.c[3]};
        [[maybe_unused]] double qok = 0.0;   // masked tier: from a HOLD to the BEGIN after it
        int level = 0;
        int q0 = 0;
        while (q0 < n_items) {
            // the run of items q0 .. q1 - 1 whose parameters fit the LDS rows
            int q1 = q0, used = 0;
            while (q1 < n_items) {
                const int need = program_need<MASKS>(items[q1], desc);
                if (used + need > PAINTED_SLOTS) break;
                used += need;
                ++q1;
            }
            int slot = 0;
            for (int q = q0; q < q1; ++q) {
                const int4 it = items[q];
                const int op = program_op<MASKS>(it.x);
                double* rowd = &sums[wave][slot];
                slot += program_need<MASKS>(it, desc);
                // (grouped: FILL, BEGIN and END, the first three arms with their `MASKS &&` parts dead; the last arm is masked only)
                if (op == GROUP_FILL) {
                    compose_fill_vjp(in, it.y, desc[it.y], live, px, through, grad_cover, X, B, lane, rowd, rowd + GRADPAINT_DENSE);
                } else if (op == GROUP_BEGIN || (MASKS && op == MASK_BEGIN_HELD)) {
                    if (live) {
                        const double o = it.z < 0 ? 1.0 : opacity[it.z];
                        const double k = compose_clip_mask(in, it.w, i);
                        double adj[4];
                        group_adjoint(X, t_end[(size_t)it.y * n_px + i], B, adj);
                        program_push_adjoint(below, level, X, B);
                        if (!MASKS || op == GROUP_BEGIN) {   // (grouped: always)
                            group_base(adj, o, k, B);
                        } else if constexpr (MASKS) {
                            double M[4];
                            masked_parked(park, mask_pair(it.x), n_px, i, M);
                            mask_base(adj, o, k, mask_value(M), B);
                        }
                    }
                    ++level;
                } else if (op == GROUP_END || (MASKS && op == MASK_HOLD)) {
                    --level;
                    const bool hold = MASKS && op == MASK_HOLD;
                    double term = 0.0;
                    if (live) {
                        const double o = it.z < 0 ? 1.0 : opacity[it.z];
                        const double G[4] = {X[0], X[1], X[2], X[3]};
                        program_pop_adjoint(below, level, X, B);
                        double adj[4];
                        group_adjoint(X, t_end[(size_t)it.y * n_px + i], B, adj);
                        const double qd = compose_dot(adj, G);
                        double km = 1.0;
                        if constexpr (MASKS) {
                            if (hold) {
                                double M[4];
                                masked_parked(park, mask_pair(it.x), n_px, i, M);
                                km = mask_value(M);
                            }
                        }
                        const double k = compose_clip_vjp(in, it.w, i, hold ? mask_clip_term(qd, o, km) : qd * o, through, grad_cover);
                        if (!hold) {
                            term = qd * k;
                            group_step(X, G, o, k);
                        } else if constexpr (MASKS) {
                            term = mask_opacity_term(qd, k, km);
                            qok = mask_held_dot(qd, o, k);
                            double H[4];
                            mask_hold(G, o, k, H);
                            SVGR_UNROLL
                            for (int c = 0; c < 4; ++c) held[level][c][threadIdx.x] = H[c];
                        }
                    }
                    if (it.z >= 0) {
                        term = wave_sum(term);
                        if (lane == 0) rowd[0] = rowd[0] + term;
                    }
                } else if constexpr (MASKS) {
                    if (op == MASK_BEGIN_MASK) {
                        if (live) {
                            double M[4];
                            masked_parked(park, mask_pair(it.x), n_px, i, M);
                            program_push_adjoint(below, level, X, B);
                            mask_base_of_mask(qok, M, B);
                        }
                        ++level;
                    } else {   // MASK_END
                        --level;
                        if (live) {
                            double M[4], H[4];
                            masked_parked(park, mask_pair(it.x), n_px, i, M);
                            program_pop_adjoint(below, level, X, B);
                            SVGR_UNROLL
                            for (int c = 0; c < 4; ++c) H[c] = held[level][c][threadIdx.x];
                            mask_step(X, H, mask_value(M));
                        }
                    }
                }
            }
            __syncthreads();
            slot = 0;
            for (int q = q0; q < q1; ++q) {
                const int4 it = items[q];
                const int need = program_need<MASKS>(it, desc);
                if (need == 0) continue;
                // a FILL's dense terms and its stops' terms, or the opacity of an END or a HOLD
                if (program_op<MASKS>(it.x) == GROUP_FILL)
                    compose_sums_flush(sums, slot, need, GRADPAINT_DENSE, mine, (size_t)GRADPAINT_DENSE * (size_t)it.y,
                                       n_dense + (size_t)GRADPAINT_STOP * (size_t)desc[it.y].z);
                else
                    compose_sums_flush(sums, slot, need, GRADPAINT_DENSE, mine, n_stop_end + (size_t)it.z, 0);
                slot += need;
            }
            __syncthreads();
            q0 = q1;
        }
    }
}

// ---- host: one checked description, one forward and one backward path ----
enum ComposeTier { TIER_SOLID, TIER_PAINTED, TIER_GROUPED, TIER_MASKED };

// The device buffers of a call: the inputs, the forward's output, the backward's.  A tier leaves what it does not take NULL, and
// nothing looks at it.
struct ComposeBufs {
    const svgr_buf *cover, *paints, *m6, *geom, *stop_pos, *stop_rgba, *opacity;
    svgr_buf* image;
    const svgr_buf* grad_image;
    svgr_buf *grad_cover, *grad_paints, *grad_m6, *grad_geom, *grad_stop_pos, *grad_stop_rgba, *grad_opacity;
};

// A checked description and the kernels' numbers from it: every tier fills what it has.
struct ComposeShape {
    int n_paths, plane;
    size_t n_px, n_all, elem;   // pixels of one plane, of all planes, bytes of a plane element
    ComposeBg bg;
    int n_stops = 0;            // painted and above: the stops, the view, the caller's topology tables
    PaintedView vw;
    const int32_t *kind, *spread, *path_stop_off;
    int n_items = 0, n_groups = 0, n_opacities = 0, n_clips = 0;   // grouped and above
    std::vector<int> table;     // items in the kernels' form, clip_off, clip_planes
    int n_pairs = 0, n_walk0 = 0;   // masked: the pairs; the items walk 0 runs: to the last END_MASK
};

static bool compose_aligned(const svgr_buf* b) { return ((uintptr_t)b->ptr & 15) == 0; }
static bool painted_has(const svgr_buf* b, size_t bytes) { return b && b->bytes >= bytes && (b->ptr || bytes == 0); }
static const double* painted_ptr(const svgr_buf* b) { return b ? (const double*)b->ptr : nullptr; }

// Everything of a description, its host tables and its input buffers that can be wrong, in the order solid, painted, program.
// The description's type says which of these it has; tier tells a masked program from a grouped one.
template <class Desc>
static int compose_check(ComposeTier tier, const char* entry, const svgr_ctx* ctx, const Desc* d, const ComposeBufs& b, ComposeShape& s) {
    constexpr bool kPainted = !std::is_same_v<Desc, svgr_compose_desc>, kProgram = std::is_same_v<Desc, svgr_grouped_desc>;
    if (kPainted && !d) return fail(SVGR_E_INVALID, "%s: desc is NULL", entry);   // (the solid entries name a NULL ctx first)
    if (!ctx) return fail(SVGR_E_INVALID, "%s: ctx is NULL", entry);
    if (!d) return fail(SVGR_E_INVALID, "%s: desc is NULL", entry);
    constexpr int64_t kMax = (1ll << 31) - 1;
    if (d->n_paths <= 0 || d->rows <= 0 || d->cols <= 0)
        return fail(SVGR_E_INVALID, "%s: %lld planes of %lld x %lld pixels", entry, (long long)d->n_paths, (long long)d->rows, (long long)d->cols);
    if (d->plane < 0 || d->plane >= COVER_PLANES) return fail(SVGR_E_INVALID, "%s: unknown plane type %d", entry, (int)d->plane);
    if (d->has_bg != 0 && d->has_bg != 1) return fail(SVGR_E_INVALID, "%s: has_bg is 0 or 1, not %d", entry, (int)d->has_bg);
    if (d->n_paths > kMax || d->rows > kMax || d->cols > kMax ||
        (unsigned __int128)d->n_paths * (unsigned __int128)d->rows * (unsigned __int128)d->cols > (unsigned __int128)kMax)
        return fail(SVGR_E_OVERFLOW, "%s: %lld planes of %lld x %lld pixels are beyond 2^31 - 1 pixels", entry, (long long)d->n_paths, (long long)d->rows, (long long)d->cols);
    if (!b.cover || !b.paints) return fail(SVGR_E_INVALID, "%s: a buffer is NULL", entry);
    const int64_t n = d->n_paths;
    s.n_paths = (int)n;
    s.plane = (int)d->plane;
    s.n_px = (size_t)d->rows * (size_t)d->cols;
    s.n_all = s.n_px * (size_t)n;
    s.elem = (size_t)cover_plane_bytes(d->plane);
    if (b.cover->bytes < s.n_all * s.elem || b.paints->bytes < (size_t)n * 32)
        return fail(SVGR_E_INVALID, "%s: cover or paints is too small for the description", entry);
    for (int k = 0; k < 4; ++k) s.bg.c[k] = d->has_bg ? d->bg[k] : 0.0;
    if constexpr (kPainted) {
        if (!d->kind || !d->spread || !d->path_stop_off) return fail(SVGR_E_INVALID, "%s: a topology table is NULL", entry);
        if (d->n_stops < 0 || d->n_stops > n * GRADPAINT_MAX_STOPS) return fail(SVGR_E_INVALID, "%s: %lld stops for %lld paths", entry, (long long)d->n_stops, (long long)n);
        if (d->path_stop_off[0] != 0 || (int64_t)d->path_stop_off[n] != d->n_stops)
            return fail(SVGR_E_INVALID, "%s: path_stop_off goes from %d to %d, not from 0 to %lld", entry, (int)d->path_stop_off[0], (int)d->path_stop_off[n], (long long)d->n_stops);
        for (int64_t p = 0; p < n; ++p) {
            const int32_t kind = d->kind[p], spread = d->spread[p];
            const int64_t ns = (int64_t)d->path_stop_off[p + 1] - (int64_t)d->path_stop_off[p];
            if (kind < 0 || kind > 2) return fail(SVGR_E_INVALID, "%s: path %lld has the unknown kind %d (0 solid, 1 linear, 2 radial)", entry, (long long)p, (int)kind);
            if (spread < 0 || spread > 2) return fail(SVGR_E_INVALID, "%s: path %lld has the unknown spread %d", entry, (long long)p, (int)spread);
            if (ns < 0) return fail(SVGR_E_INVALID, "%s: path_stop_off decreases at path %lld", entry, (long long)p);
            if (kind == 0 && ns != 0) return fail(SVGR_E_INVALID, "%s: the solid path %lld has %lld stops", entry, (long long)p, (long long)ns);
            if (kind != 0 && (ns < 1 || ns > GRADPAINT_MAX_STOPS))
                return fail(SVGR_E_INVALID, "%s: the gradient path %lld has %lld stops: 1 to %d", entry, (long long)p, (long long)ns, GRADPAINT_MAX_STOPS);
        }
        const size_t np = (size_t)n, nst = (size_t)d->n_stops;
        if (!painted_has(b.m6, np * 48) || !painted_has(b.geom, np * 32) || !b.m6->ptr || !b.geom->ptr)
            return fail(SVGR_E_INVALID, "%s: paint_m6 or paint_geom is missing or too small for the description", entry);
        if (nst && (!painted_has(b.stop_pos, nst * 8) || !painted_has(b.stop_rgba, nst * 32)))
            return fail(SVGR_E_INVALID, "%s: stop_pos or stop_rgba is missing or too small for the description", entry);
        s.n_stops = (int)d->n_stops;
        s.vw.row0 = (long long)d->row0;
        s.vw.col0 = (long long)d->col0;
        s.vw.cols = (unsigned)d->cols;
        s.kind = d->kind;
        s.spread = d->spread;
        s.path_stop_off = d->path_stop_off;
    }
    if constexpr (kProgram) {
        if (d->n_groups < 0 || d->n_groups > kMax || d->n_items < 0 || d->n_items > kMax || d->n_opacities < 0 || d->n_clip_planes < 0)
            return fail(SVGR_E_INVALID, "%s: %lld items, %lld groups, %lld opacities, %lld clip planes", entry, (long long)d->n_items, (long long)d->n_groups,
                        (long long)d->n_opacities, (long long)d->n_clip_planes);
        if (d->n_groups > d->n_items) return fail(SVGR_E_INVALID, "%s: %lld groups in %lld items", entry, (long long)d->n_groups, (long long)d->n_items);
        if (d->n_items > GROUP_MAX_ITEMS) return fail(SVGR_E_OVERFLOW, "%s: %lld items are beyond %d", entry, (long long)d->n_items, GROUP_MAX_ITEMS);
        std::vector<int> seen((size_t)d->n_paths + (size_t)d->n_groups + (size_t)std::min(d->n_opacities, d->n_groups) + 1);
        s.table.assign(4 * (size_t)d->n_items, 0);
        long long at = -1;
        int last_mask = -1;
        const char* what = tier == TIER_MASKED
                               ? mask_program_check(d->items, d->n_items, d->n_paths, d->n_groups, d->n_clip_planes, d->n_opacities, d->clip_off, d->clip_planes,
                                                    seen.data(), s.table.data(), &s.n_clips, &s.n_pairs, &last_mask, &at)
                               : group_program_check(d->items, d->n_items, d->n_paths, d->n_groups, d->n_clip_planes, d->n_opacities, d->clip_off, d->clip_planes,
                                                     seen.data(), s.table.data(), &s.n_clips, &at);
        if (what) return fail(SVGR_E_INVALID, "%s: the program is wrong: %s (at %lld)", entry, what, at);
        // (T_end is a plane per group; this bounds walk 0's planes too: a pair is two groups and parks four planes)
        if ((unsigned __int128)d->n_groups * (unsigned __int128)s.n_px > (unsigned __int128)kMax)
            return fail(SVGR_E_OVERFLOW, "%s: %lld groups of %zu pixels are beyond 2^31 - 1 pixels", entry, (long long)d->n_groups, s.n_px);
        if (d->n_opacities && (!painted_has(b.opacity, (size_t)d->n_opacities * 8) || !b.opacity->ptr))
            return fail(SVGR_E_INVALID, "%s: opacity is missing or too small for the description", entry);
        s.n_items = (int)d->n_items;
        s.n_groups = (int)d->n_groups;
        s.n_opacities = (int)d->n_opacities;
        s.n_walk0 = last_mask + 1;
        if (s.n_clips) {
            s.table.insert(s.table.end(), d->clip_off, d->clip_off + s.n_clips + 1);
            s.table.insert(s.table.end(), d->clip_planes, d->clip_planes + d->n_clip_planes);
        }
    }
    return 0;
}

// the forward's output
static int compose_image_check(const char* entry, const ComposeShape& s, const svgr_buf* image) {
    if (!image) return fail(SVGR_E_INVALID, "%s: a buffer is NULL", entry);
    if (image->bytes < s.n_px * 4 * s.elem || !compose_aligned(image))
        return fail(SVGR_E_INVALID, "%s: image is too small for the description or not aligned to 16 bytes", entry);
    return 0;
}

// the backward's gradient image and outputs.  (The program tiers also refuse an output without memory, and say so.)
static int compose_grads_check(ComposeTier tier, const char* entry, const ComposeShape& s, const ComposeBufs& b) {
    const bool painted = tier != TIER_SOLID, program = tier == TIER_GROUPED || tier == TIER_MASKED;
    if (!b.grad_image || !b.grad_cover || !b.grad_paints || (painted && (!b.grad_m6 || !b.grad_geom)))
        return fail(SVGR_E_INVALID, "%s: a buffer is NULL", entry);
    if (b.grad_image->bytes < s.n_px * 4 * s.elem || !compose_aligned(b.grad_image))
        return fail(SVGR_E_INVALID, "%s: grad_image is too small for the description or not aligned to 16 bytes", entry);
    const size_t np = (size_t)s.n_paths, nst = (size_t)s.n_stops, nop = (size_t)s.n_opacities;
    bool bad = b.grad_cover->bytes < s.n_all * s.elem || b.grad_paints->bytes < np * 32;
    if (!painted) return bad ? fail(SVGR_E_INVALID, "%s: grad_cover or grad_paints is too small for the description", entry) : 0;
    bad = bad || b.grad_m6->bytes < np * 48 || b.grad_geom->bytes < np * 32;
    if (program) bad = bad || !b.grad_cover->ptr || !b.grad_paints->ptr || !b.grad_m6->ptr || !b.grad_geom->ptr;
    if (bad)
        return fail(SVGR_E_INVALID, "%s: grad_cover, grad_paints, grad_m6 or grad_geom is %stoo small for the description", entry, program ? "missing or " : "");
    if (nst && (!painted_has(b.grad_stop_pos, nst * 8) || !painted_has(b.grad_stop_rgba, nst * 32)))
        return fail(SVGR_E_INVALID, "%s: grad_stop_pos or grad_stop_rgba is missing or too small for the description", entry);
    if (nop && (!painted_has(b.grad_opacity, nop * 8) || !b.grad_opacity->ptr))
        return fail(SVGR_E_INVALID, "%s: grad_opacity is missing or too small for the description", entry);
    return 0;
}

// the workgroups of a backward kernel: they stride over the pixels
static int compose_groups(const ComposeShape& s) {
    const size_t steps = (s.n_px + COMPOSE_BLOCK - 1) / COMPOSE_BLOCK;
    return (int)(steps < (size_t)COMPOSE_GROUPS ? steps : (size_t)COMPOSE_GROUPS);
}

// the plane type of a call as a type: f(T()) with T float or double
template <class F>
static void compose_by_plane(int plane, F&& f) {
    if (plane == COVER_F32) f(float());
    else f(double());
}

// the topology tables into the device block, by kernel arguments
static void painted_topology(const ComposeShape& s, int4* desc, hipStream_t st) {
    PaintedTopo t;
    for (int first = 0; first < s.n_paths; first += PAINTED_TOPO) {
        t.first = first;
        t.n = std::min(PAINTED_TOPO, s.n_paths - first);
        for (int q = 0; q < t.n; ++q) {
            t.kind_spread[q] = (int)s.kind[first + q] | ((int)s.spread[first + q] << 8);
            t.stop_off[q] = (int)s.path_stop_off[first + q];
        }
        t.stop_off[t.n] = (int)s.path_stop_off[first + t.n];
        for (int q = t.n; q < PAINTED_TOPO; ++q) { t.kind_spread[q] = 0; t.stop_off[q + 1] = 0; }
        SVGR_LAUNCH(k_painted_topology, grid1((size_t)t.n, 64), dim3(64), 0, st, t, desc);
    }
}

// the program's table into the device block, by kernel arguments
static GroupedProgram grouped_program(const ComposeShape& s, int* table, hipStream_t st) {
    GroupSlice t;
    const int n = (int)s.table.size();
    for (int first = 0; first < n; first += GROUPED_INTS) {
        t.first = first;
        t.n = std::min(GROUPED_INTS, n - first);
        for (int q = 0; q < GROUPED_INTS; ++q) t.v[q] = q < t.n ? s.table[(size_t)first + q] : 0;
        SVGR_LAUNCH(k_group_program, grid1((size_t)t.n, 64), dim3(64), 0, st, t, table);
    }
    GroupedProgram g;
    g.items = (const int4*)table;
    g.clip_off = table + 4 * (size_t)s.n_items;
    g.clip_planes = g.clip_off + (s.n_clips ? s.n_clips + 1 : 0);
    g.n_items = s.n_items;
    return g;
}

static int compose_forward_impl(svgr_ctx* ctx, const svgr_compose_desc* d, const ComposeBufs& b) {
    static const char* entry = "svgr_compose_forward";
    ComposeShape s;
    if (int rc = compose_check(TIER_SOLID, entry, ctx, d, b, s)) return rc;
    if (int rc = compose_image_check(entry, s, b.image)) return rc;
    HIPCHK(enter_ctx(ctx));
    hipStream_t st = ctx->stream;
    compose_by_plane(s.plane, [&](auto zero) {
        using T = decltype(zero);
        SVGR_LAUNCH(k_compose_over<T>, grid1(s.n_px, COMPOSE_BLOCK), dim3(COMPOSE_BLOCK), 0, st, (const T*)b.cover->ptr, (const double*)b.paints->ptr, s.bg,
                    s.n_paths, s.n_px, (T*)b.image->ptr);
    });
    HIPCHK(hipGetLastError());
    return 0;
}

static int compose_backward_impl(svgr_ctx* ctx, const svgr_compose_desc* d, const ComposeBufs& b) {
    static const char* entry = "svgr_compose_backward";
    ComposeShape s;
    if (int rc = compose_check(TIER_SOLID, entry, ctx, d, b, s)) return rc;
    if (int rc = compose_grads_check(TIER_SOLID, entry, s, b)) return rc;
    HIPCHK(enter_ctx(ctx));
    hipStream_t st = ctx->stream;
    const int groups = compose_groups(s);
    const size_t n4 = (size_t)s.n_paths * 4;
    // (the blocks go back at scope end by the pool's stream-order rule)
    PoolBlock part, through;   // the workgroups' partial paint sums; float planes: the double T_p plane of walk 1
    HIPCHK(part.alloc((size_t)groups * n4 * 8, ctx->device));
    HIPCHK(hipMemsetAsync(part.p, 0, (size_t)groups * n4 * 8, st));
    if (s.plane == COVER_F32) HIPCHK(through.alloc(s.n_all * 8, ctx->device));
    compose_by_plane(s.plane, [&](auto zero) {
        using T = decltype(zero);
        SVGR_LAUNCH(k_compose_vjp<T>, dim3((unsigned)groups), dim3(COMPOSE_BLOCK), 0, st, (const T*)b.cover->ptr, (const double*)b.paints->ptr, s.bg, s.n_paths,
                    s.n_px, (const T*)b.grad_image->ptr, through.p ? through.as<double>() : (double*)b.grad_cover->ptr, (T*)b.grad_cover->ptr, part.as<double>());
    });
    SVGR_LAUNCH(k_compose_paint_sum, grid1(n4, 64), dim3(64), 0, st, (const double*)part.p, groups, n4, (double*)b.grad_paints->ptr);
    HIPCHK(hipGetLastError());
    return 0;
}

// the painted, grouped and masked forward: output check, blocks, table uploads, the tier's kernel
template <class Desc>
static int compose_tier_forward(ComposeTier tier, const char* entry, svgr_ctx* ctx, const Desc* d, const ComposeBufs& b) {
    ComposeShape s;
    if (int rc = compose_check(tier, entry, ctx, d, b, s)) return rc;
    if (int rc = compose_image_check(entry, s, b.image)) return rc;
    const bool program = tier != TIER_PAINTED;
    HIPCHK(enter_ctx(ctx));
    hipStream_t st = ctx->stream;
    PoolBlock topo, table;   // the paths' descriptions; the program (go back at scope end by the pool's stream-order rule)
    HIPCHK(topo.alloc((size_t)s.n_paths * sizeof(int4), ctx->device));
    if (program) HIPCHK(table.alloc(s.table.size() * sizeof(int), ctx->device));
    painted_topology(s, topo.as<int4>(), st);
    const GroupedProgram g = program ? grouped_program(s, table.as<int>(), st) : GroupedProgram();
    const dim3 grid = grid1(s.n_px, COMPOSE_BLOCK);
    compose_by_plane(s.plane, [&](auto zero) {
        using T = decltype(zero);
        const T* cover = (const T*)b.cover->ptr;
        const double* paints = (const double*)b.paints->ptr;
        T* image = (T*)b.image->ptr;
        if (!program) {
            SVGR_LAUNCH(k_compose_over_painted<T>, grid, dim3(COMPOSE_BLOCK), 0, st, cover, paints, topo.as<int4>(), painted_ptr(b.m6), painted_ptr(b.geom),
                        painted_ptr(b.stop_pos), painted_ptr(b.stop_rgba), s.bg, s.vw, s.n_paths, s.n_px, image);
        } else {
            const auto kernel = tier == TIER_MASKED ? k_compose_over_program<T, true> : k_compose_over_program<T, false>;
            SVGR_LAUNCH(kernel, grid, dim3(COMPOSE_BLOCK), 0, st, cover, paints, topo.as<int4>(), painted_ptr(b.m6), painted_ptr(b.geom),
                        painted_ptr(b.stop_pos), painted_ptr(b.stop_rgba), g.items, g.clip_off, g.clip_planes, painted_ptr(b.opacity), s.bg, s.vw, g.n_items,
                        s.n_px, image);
        }
    });
    HIPCHK(hipGetLastError());
    return 0;
}

// the painted, grouped and masked backward: output checks, blocks, memset, table uploads, the tier's kernel, the sum kernel
template <class Desc>
static int compose_tier_backward(ComposeTier tier, const char* entry, svgr_ctx* ctx, const Desc* d, const ComposeBufs& b) {
    ComposeShape s;
    if (int rc = compose_check(tier, entry, ctx, d, b, s)) return rc;
    if (int rc = compose_grads_check(tier, entry, s, b)) return rc;
    const bool program = tier != TIER_PAINTED;
    HIPCHK(enter_ctx(ctx));
    hipStream_t st = ctx->stream;
    const int groups = compose_groups(s);
    const size_t np = (size_t)s.n_paths, nst = (size_t)s.n_stops, nop = (size_t)s.n_opacities;
    const size_t n_dense = np * GRADPAINT_DENSE, n_stop_end = n_dense + nst * GRADPAINT_STOP, n_params = n_stop_end + nop;
    // (the blocks go back at scope end by the pool's stream-order rule)
    // the paths' descriptions; the program; the workgroups' partial sums; float planes: the double T_p plane of walk 1; T_end per
    // group; masked: M per pair, four planes
    PoolBlock topo, table, part, through, t_end, park;
    HIPCHK(topo.alloc(np * sizeof(int4), ctx->device));
    if (program) HIPCHK(table.alloc(s.table.size() * sizeof(int), ctx->device));
    HIPCHK(part.alloc((size_t)groups * n_params * 8, ctx->device));
    if (s.plane == COVER_F32) HIPCHK(through.alloc(s.n_all * 8, ctx->device));
    if (program) HIPCHK(t_end.alloc(std::max<size_t>(1, (size_t)s.n_groups) * s.n_px * 8, ctx->device));
    if (tier == TIER_MASKED) HIPCHK(park.alloc(std::max<size_t>(1, (size_t)s.n_pairs) * 4 * s.n_px * 8, ctx->device));
    HIPCHK(hipMemsetAsync(part.p, 0, (size_t)groups * n_params * 8, st));
    painted_topology(s, topo.as<int4>(), st);
    const GroupedProgram g = program ? grouped_program(s, table.as<int>(), st) : GroupedProgram();
    compose_by_plane(s.plane, [&](auto zero) {
        using T = decltype(zero);
        const T* cover = (const T*)b.cover->ptr;
        const double* paints = (const double*)b.paints->ptr;
        const T* grad_image = (const T*)b.grad_image->ptr;
        T* grad_cover = (T*)b.grad_cover->ptr;
        double* thr = through.p ? through.as<double>() : (double*)b.grad_cover->ptr;
        if (!program) {
            SVGR_LAUNCH(k_compose_vjp_painted<T>, dim3((unsigned)groups), dim3(COMPOSE_BLOCK), 0, st, cover, paints, topo.as<int4>(), painted_ptr(b.m6),
                        painted_ptr(b.geom), painted_ptr(b.stop_pos), painted_ptr(b.stop_rgba), s.bg, s.vw, s.n_paths, s.n_stops, s.n_px, grad_image, thr,
                        grad_cover, part.as<double>());
        } else {
            const auto kernel = tier == TIER_MASKED ? k_compose_vjp_program<T, true> : k_compose_vjp_program<T, false>;
            SVGR_LAUNCH(kernel, dim3((unsigned)groups), dim3(COMPOSE_BLOCK), 0, st, cover, paints, topo.as<int4>(), painted_ptr(b.m6), painted_ptr(b.geom),
                        painted_ptr(b.stop_pos), painted_ptr(b.stop_rgba), g.items, g.clip_off, g.clip_planes, painted_ptr(b.opacity), s.bg, s.vw, g.n_items,
                        s.n_walk0, s.n_paths, s.n_stops, s.n_opacities, s.n_px, grad_image, thr, grad_cover, t_end.as<double>(), park.as<double>(),
                        part.as<double>());
        }
    });
    SVGR_LAUNCH(k_compose_param_sum, grid1(n_params, 64), dim3(64), 0, st, (const double*)part.p, groups, n_dense, n_stop_end, n_params,
                (double*)b.grad_paints->ptr, (double*)b.grad_m6->ptr, (double*)b.grad_geom->ptr, nst ? (double*)b.grad_stop_pos->ptr : nullptr,
                nst ? (double*)b.grad_stop_rgba->ptr : nullptr, nop ? (double*)b.grad_opacity->ptr : nullptr);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" {
int svgr_compose_block(void) { return COMPOSE_BLOCK; }
int svgr_compose_groups(void) { return COMPOSE_GROUPS; }
int svgr_group_depth(void) { return GROUP_DEPTH; }

int svgr_compose_forward(svgr_ctx* ctx, const svgr_compose_desc* desc, const svgr_buf* cover, const svgr_buf* paints, svgr_buf* image) {
    return abi_guard("svgr_compose_forward", [&]() {
        ComposeBufs b = {};
        b.cover = cover, b.paints = paints, b.image = image;
        return compose_forward_impl(ctx, desc, b);
    });
}

int svgr_compose_backward(svgr_ctx* ctx, const svgr_compose_desc* desc, const svgr_buf* cover, const svgr_buf* paints, const svgr_buf* grad_image,
                          svgr_buf* grad_cover, svgr_buf* grad_paints) {
    return abi_guard("svgr_compose_backward", [&]() {
        ComposeBufs b = {};
        b.cover = cover, b.paints = paints, b.grad_image = grad_image, b.grad_cover = grad_cover, b.grad_paints = grad_paints;
        return compose_backward_impl(ctx, desc, b);
    });
}

int svgr_compose_painted_forward(svgr_ctx* ctx, const svgr_painted_desc* desc, const svgr_buf* cover, const svgr_buf* paints, const svgr_buf* paint_m6,
                                 const svgr_buf* paint_geom, const svgr_buf* stop_pos, const svgr_buf* stop_rgba, svgr_buf* image) {
    static const char* entry = "svgr_compose_painted_forward";
    return abi_guard(entry, [&]() {
        return compose_tier_forward(TIER_PAINTED, entry, ctx, desc, ComposeBufs{cover, paints, paint_m6, paint_geom, stop_pos, stop_rgba, nullptr, image});
    });
}

int svgr_compose_painted_backward(svgr_ctx* ctx, const svgr_painted_desc* desc, const svgr_buf* cover, const svgr_buf* paints, const svgr_buf* paint_m6,
                                  const svgr_buf* paint_geom, const svgr_buf* stop_pos, const svgr_buf* stop_rgba, const svgr_buf* grad_image,
                                  svgr_buf* grad_cover, svgr_buf* grad_paints, svgr_buf* grad_m6, svgr_buf* grad_geom, svgr_buf* grad_stop_pos,
                                  svgr_buf* grad_stop_rgba) {
    static const char* entry = "svgr_compose_painted_backward";
    return abi_guard(entry, [&]() {
        return compose_tier_backward(TIER_PAINTED, entry, ctx, desc,
                                     ComposeBufs{cover, paints, paint_m6, paint_geom, stop_pos, stop_rgba, nullptr, nullptr, grad_image, grad_cover, grad_paints,
                                                 grad_m6, grad_geom, grad_stop_pos, grad_stop_rgba, nullptr});
    });
}

int svgr_compose_grouped_forward(svgr_ctx* ctx, const svgr_grouped_desc* desc, const svgr_buf* cover, const svgr_buf* paints, const svgr_buf* paint_m6,
                                 const svgr_buf* paint_geom, const svgr_buf* stop_pos, const svgr_buf* stop_rgba, const svgr_buf* opacity, svgr_buf* image) {
    static const char* entry = "svgr_compose_grouped_forward";
    return abi_guard(entry, [&]() {
        return compose_tier_forward(TIER_GROUPED, entry, ctx, desc, ComposeBufs{cover, paints, paint_m6, paint_geom, stop_pos, stop_rgba, opacity, image});
    });
}

int svgr_compose_grouped_backward(svgr_ctx* ctx, const svgr_grouped_desc* desc, const svgr_buf* cover, const svgr_buf* paints, const svgr_buf* paint_m6,
                                  const svgr_buf* paint_geom, const svgr_buf* stop_pos, const svgr_buf* stop_rgba, const svgr_buf* opacity,
                                  const svgr_buf* grad_image, svgr_buf* grad_cover, svgr_buf* grad_paints, svgr_buf* grad_m6, svgr_buf* grad_geom,
                                  svgr_buf* grad_stop_pos, svgr_buf* grad_stop_rgba, svgr_buf* grad_opacity) {
    static const char* entry = "svgr_compose_grouped_backward";
    return abi_guard(entry, [&]() {
        return compose_tier_backward(TIER_GROUPED, entry, ctx, desc,
                                     ComposeBufs{cover, paints, paint_m6, paint_geom, stop_pos, stop_rgba, opacity, nullptr, grad_image, grad_cover, grad_paints,
                                                 grad_m6, grad_geom, grad_stop_pos, grad_stop_rgba, grad_opacity});
    });
}

int svgr_compose_masked_forward(svgr_ctx* ctx, const svgr_grouped_desc* desc, const svgr_buf* cover, const svgr_buf* paints, const svgr_buf* paint_m6,
                                const svgr_buf* paint_geom, const svgr_buf* stop_pos, const svgr_buf* stop_rgba, const svgr_buf* opacity, svgr_buf* image) {
    static const char* entry = "svgr_compose_masked_forward";
    return abi_guard(entry, [&]() {
        return compose_tier_forward(TIER_MASKED, entry, ctx, desc, ComposeBufs{cover, paints, paint_m6, paint_geom, stop_pos, stop_rgba, opacity, image});
    });
}

int svgr_compose_masked_backward(svgr_ctx* ctx, const svgr_grouped_desc* desc, const svgr_buf* cover, const svgr_buf* paints, const svgr_buf* paint_m6,
                                 const svgr_buf* paint_geom, const svgr_buf* stop_pos, const svgr_buf* stop_rgba, const svgr_buf* opacity,
                                 const svgr_buf* grad_image, svgr_buf* grad_cover, svgr_buf* grad_paints, svgr_buf* grad_m6, svgr_buf* grad_geom,
                                 svgr_buf* grad_stop_pos, svgr_buf* grad_stop_rgba, svgr_buf* grad_opacity) {
    static const char* entry = "svgr_compose_masked_backward";
    return abi_guard(entry, [&]() {
        return compose_tier_backward(TIER_MASKED, entry, ctx, desc,
                                     ComposeBufs{cover, paints, paint_m6, paint_geom, stop_pos, stop_rgba, opacity, nullptr, grad_image, grad_cover, grad_paints,
                                                 grad_m6, grad_geom, grad_stop_pos, grad_stop_rgba, grad_opacity});
    });
}
}  // extern "C"
