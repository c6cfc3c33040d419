// svgr_plan_state.h -- what a batch knows about its standing plan and about the results earlier passes left on the device.
//
// Host only: no HIP type, no device code; a pointer is here for its bits alone.  svgr_batch (svgr_hip.hip) holds one PlanState, and
// tests/plan_state_harness.cpp drives the same code on the CPU.  Every member is private: a change of state is one of the named
// transitions below, each with the reason for what it clears, and the three kept results are written by run_geometry alone,
// through `wrote` / `drop` / `slab_table_written`.
#pragma once

#include <array>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <type_traits>

namespace svgr {

// What a result on the device was made FROM -- the arrays (pointer and capacity), the counts, the viewport, the threshold's bit
// pattern -- as 64-bit words in the order its pass lists them; words not used stay zero.  Only ever compared: a replay that finds
// another fingerprint than the one recorded makes the result again.
constexpr size_t kPrintWords = 28;
using PlanPrint = std::array<uint64_t, kPrintWords>;

template <class T> constexpr size_t print_words() { return (sizeof(T) + 7) / 8; }
// every argument goes in by its bytes, padded to whole words (a pointer, a size, a double: one word; AddShards: its 33 ints)
template <class... A> PlanPrint plan_print(const A&... a) {
    static_assert((print_words<A>() + ... + 0) <= kPrintWords, "the fingerprint has no room for these");
    static_assert((std::is_trivially_copyable<A>::value && ...), "a fingerprint is made of plain values");
    PlanPrint f{};
    size_t at = 0;
    ((memcpy(&f[at], &a, sizeof(A)), at += print_words<A>()), ...);
    return f;
}

// A result kept on the device: whether it stands, and the fingerprint of the pass that wrote it.
class Kept {
    bool current_ = false;
    PlanPrint made_{};

public:
    // may this pass skip the work?  `eligible`: it is a pass of the kind that can; `now`: what it would make the result from
    bool holds(bool eligible, const PlanPrint& now) const { return eligible && current_ && made_ == now; }
    // a pass has written the result (`valid`: in the form a later replay may keep)
    void wrote(bool valid, const PlanPrint& now) { current_ = valid; made_ = now; }
    void drop() { current_ = false; }
};

class PlanState {
    bool planned_ = false;              // a plan stands: svgr_batch_render may run
    bool slab_at_valid_ = false;        // `slab_at` holds the standing plan's slab order (heaviest paths first)
    bool slab_order_pending_ = false;   // svgr_batch_draw planned the batch and left the slab order to the first render that replays the plan
    // The slab order was made by the render that is running, not by the plan (svgr_batch_draw leaves it to the first replay): that
    // render's pass writes the table but does not mark it kept -- the replay behind it runs k_path_bbox once more and marks it.  Nothing
    // in the arrays asks for this; the suite pins five launches for that replay (tests/test_gpu_draw.py), and a batch planned by a
    // draw pays one launch of 6 us once.  A batch planned by svgr_batch_plan has its order from the plan and is not held back.
    bool slab_order_late_ = false;

    // (every transition that takes the plan away: see plan_begins for why the cells go with it)
    void forget_plan() {
        planned_ = false; slab_at_valid_ = false; slab_order_pending_ = false;
        slabs.drop(); lists.drop(); cells.drop();
    }

public:
    // slabs: a geometry pass has run k_path_bbox under the standing plan's `slab_at` order: `slabs`, `bbox` and `bins` hold the plan's
    //   places, and a replay under the same plan keeps them instead of launching the kernel again (its flatten is the lean form, which
    //   writes no keys -- behind a full flatten k_path_build<1> checks the paths' keys against them).  Dropped wherever the plan or its
    //   slab order is, and by every pass that writes the three arrays in another form.
    // lists: the same for what k_tile_lists leaves (`items`, `pages`, `tile_info`): a placed replay that keeps its slab table would
    //   list, band by band, what the previous one listed unless a band's mask words differ -- and the kernel compares them against
    //   `tile_mask_kept`, the words its last full run saved.  Recorded by a full run that saved them; dropped wherever the plan or the
    //   slab table is, by every pass that stops short of the lists, lists the bands again (k_band_entries) or builds the cells by
    //   another k_path_build than <1>.  Passes that only read the lists (windows, the other outputs) leave it alone.
    // cells: and for what k_path_build<1, LEAN> no longer writes -- the headers of the class-2 cells and the layer-edge sentinels of
    //   their add lists, the same bytes at the same places in every placed pass of one plan with one set of paints and rules --: the
    //   last pass that wrote `cell_hdr` and `adds` was a placed pass (full or lean) over every band, with add lists, without groups or
    //   gradients, into the blocks the fingerprint records, and nothing has changed a header field since.  Where this does not hold
    //   the placed pass is the full form, once.  Case by case:
    //     a measuring pass (`adds` == nullptr), every unplanned pass (<0>, <2>)   void it: they reserve other places / write no list
    //                                                                             (run_geometry records `wrote(false, ..)`)
    //     a pass of one rank of several                                           voids it: the other ranks' cells are not written
    //     a pass with groups or gradients                                         voids it: the header's `group` and `bits` differ
    //     a pass without slabs, or one that stops short of the path build         voids it (run_geometry: `drop`)
    //     a pass that ends in an error                                            voids it (pass_failed)
    //     a deterministic render                                                  valid: the full form, same plan, same bytes
    //     a window render, an OUT_CANVAS_F64 render                               valid: the geometry pass in front of them is an
    //                                                                             ordinary placed pass, the tile kernels only read
    //     svgr_batch_set_paints                                                   voids it (paints_changed); `path_rule` is written
    //                                                                             when the batch is made and never again; groups and
    //                                                                             gradients void it by the passes that run under them
    //     new transforms, bands, viewport, a re-plan, inherited arrays            void it (geometry_changed, plan_begins,
    //                                                                             arrays_inherited); a new batch starts with it clear
    Kept slabs, lists, cells;

    bool planned() const { return planned_; }
    bool slab_at_valid() const { return slab_at_valid_; }
    bool slab_order_pending() const { return slab_order_pending_; }
    bool slab_order_late() const { return slab_order_late_; }   // (for the host test: the product only reads it in slab_table_written)

    // New transforms (svgr_batch_set_transforms) or another share of the bands (svgr_batch_set_bands: the edge and record capacities
    // are per rank): the plan was made for other geometry, and everything made under it goes.
    void geometry_changed() { forget_plan(); }
    // A planner starts (svgr_batch_plan, svgr_batch_plan_many, svgr_batch_draw's pass; also where one planner gives up and the next
    // takes over): whatever plan stood is gone until this one succeeds.  svgr_batch_draw's single pass calls this with no plan
    // standing (it runs under `if (!planned())`), where clearing `planned_` changes nothing.
    // The cells are dropped with the plan although no pass has touched them yet.  That cannot change a decision: `cells.holds` is
    // asked only by a placed pass, a placed pass needs planned(), and plan_made() is only ever called behind a run_geometry(b, 4)
    // that ran to its end with planned() false (spec_issue, two_pass_issue, the staged plan's step 4) -- an unplanned pass, which
    // records the cells as not kept (`wrote(false, ..)`, or `drop` where there is no slab).  So by the time the next placed pass
    // asks, the cells are void whether this transition dropped them or not.
    void plan_begins() { forget_plan(); }
    // A planner's pass has been validated (or, in svgr_batch_draw, is taken on trust for the tile kernel right behind it).
    void plan_made() { planned_ = true; }
    // A pass that was taken for a plan is not one (yet): the single pass whose guesses were too small, and svgr_batch_draw's pass
    // between its tile kernel and its validation.  The pass was unplanned, so it left no slab order and no pending one -- plan_begins
    // cleared both and nothing has set them since: they are left alone.  The slab table and the tile lists it wrote are in the
    // unplanned form: not kept.  (The cells: that pass recorded them as not kept itself.)
    void pass_withdrawn() { planned_ = false; slabs.drop(); lists.drop(); }
    // plan_slab_order starts: the places in `slab_at` are about to change, and the table and the lists written at the old places
    // with them.  The order is the plan's again, not a running render's (slab_order_made_late follows where it is).
    void slab_order_begins() { slab_at_valid_ = false; slab_order_late_ = false; slabs.drop(); lists.drop(); }
    // ... and has uploaded an order (it returns before this where it leaves the order to the device's cursor).
    void slab_order_made() { slab_at_valid_ = true; }
    // svgr_batch_draw has planned a batch: large ones get their slab order from the first render that replays the plan.
    void slab_order_left_to_replay(bool large) { slab_order_pending_ = large; }
    // That render takes the order up (before it runs plan_slab_order: an error there does not leave it pending) ...
    void slab_order_taken_up() { slab_order_pending_ = false; }
    // ... and has made it: its own pass does not mark the table kept (slab_order_late_ above).
    void slab_order_made_late() { slab_order_late_ = true; }
    // A new batch has taken over the work arrays of a destroyed one (spare_adopt): another drawing's slab order, table and lists.
    // `slab_order_late_` is not touched: no render of this batch can be running.  The cells are another drawing's too and go as
    // well; adoption happens only inside a planner's single pass, with planned() false, so plan_begins' argument holds here.
    void arrays_inherited() { slab_at_valid_ = false; slabs.drop(); lists.drop(); cells.drop(); }
    // The tiles' entry bitmasks have another width (size_masks, the two-pass plan's sizing): the saved words no longer line up.
    void masks_resized() { lists.drop(); }
    // svgr_batch_set_paints: the cell headers carry the paint, and the lean path build leaves the class-2 cells' headers as they
    // are -- one full placed pass first.  The geometry is the same: plan, slab table and lists stand.
    void paints_changed() { cells.drop(); }
    // A pass ended with an error flag: it may have stopped anywhere, so nothing it was to write is kept.  The plan itself stands
    // (its caller decides); svgr_batch::invalidate_work clears the self-cleaning buffers' flags beside this.
    void pass_failed() { slabs.drop(); lists.drop(); cells.drop(); }
    // run_geometry has launched k_path_bbox: the table is kept when it was written at the standing plan's places (`for_plan`) by a
    // pass that did not make the slab order itself.
    void slab_table_written(bool for_plan, const PlanPrint& now) {
        slabs.wrote(for_plan && !slab_order_late_, now);
        slab_order_late_ = false;
    }
};

}  // namespace svgr
