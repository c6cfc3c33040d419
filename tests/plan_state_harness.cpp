// Host build of svgrasterize.py_amd/csrc/svgr_plan_state.h alone: the plan-standing flags of a batch, the three results kept on the
// device (slab table, tile lists, cells) and the named transitions between them, driven as run_geometry drives them.  For CPU-side
// unit tests only (tests/test_plan_state_host.py).  NOT a CPU fallback of the product: the package never loads it.
#include "../svgrasterize.py_amd/csrc/svgr_plan_state.h"

using namespace svgr;

namespace {
PlanState st;
PlanPrint last[3];   // what the harness recorded last for slabs, lists, cells

PlanPrint print_of(const uint64_t* w) {
    PlanPrint f{};
    for (size_t k = 0; k < kPrintWords; ++k) f[k] = w[k];
    return f;
}
Kept& kept(int which) { return which == 0 ? st.slabs : which == 1 ? st.lists : st.cells; }
}  // namespace

extern "C" {

int ps_print_words() { return (int)kPrintWords; }
void ps_reset() { st = PlanState(); for (auto& f : last) f = PlanPrint{}; }

// the transitions, in the order tests/test_plan_state_host.py names them; -1: no such transition
int ps_apply(int k) {
    switch (k) {
    case 0: st.geometry_changed(); break;
    case 1: st.plan_begins(); break;
    case 2: st.plan_made(); break;
    case 3: st.pass_withdrawn(); break;
    case 4: st.slab_order_begins(); break;
    case 5: st.slab_order_made(); break;
    case 6: st.slab_order_left_to_replay(true); break;
    case 7: st.slab_order_left_to_replay(false); break;
    case 8: st.slab_order_taken_up(); break;
    case 9: st.slab_order_made_late(); break;
    case 10: st.arrays_inherited(); break;
    case 11: st.masks_resized(); break;
    case 12: st.paints_changed(); break;
    case 13: st.pass_failed(); break;
    default: return -1;
    }
    return 0;
}

// a pass records a result as run_geometry does: which = 0 the slab table (k_path_bbox ran), 1 the tile lists, 2 the cells
void ps_wrote(int which, int valid, const uint64_t* words) {
    last[which] = print_of(words);
    if (which == 0) st.slab_table_written(valid != 0, last[0]); else kept(which).wrote(valid != 0, last[which]);
}
void ps_drop(int which) { kept(which).drop(); }
int ps_holds(int which, int eligible, const uint64_t* words) { return kept(which).holds(eligible != 0, print_of(words)) ? 1 : 0; }

// bit 0 planned, 1 slab_at_valid, 2 slab_order_pending, 3 slab_order_late, 4 / 5 / 6: slabs / lists / cells hold for what was recorded last
int ps_flags() {
    return (st.planned() ? 1 : 0) | (st.slab_at_valid() ? 2 : 0) | (st.slab_order_pending() ? 4 : 0) | (st.slab_order_late() ? 8 : 0) |
           (st.slabs.holds(true, last[0]) ? 16 : 0) | (st.lists.holds(true, last[1]) ? 32 : 0) | (st.cells.holds(true, last[2]) ? 64 : 0);
}

// plan_print's packing: two pointers, a size, two ints, a double and a 33-int block (AddShards' shape) -> the words
void ps_print_of(const void* p0, const void* p1, size_t n, int a, int b, double thr, const int* block33, uint64_t* out) {
    struct Block { int v[33]; } blk;
    memcpy(&blk, block33, sizeof blk);
    const PlanPrint f = plan_print(p0, p1, n, a, b, thr, blk);
    for (size_t k = 0; k < kPrintWords; ++k) out[k] = f[k];
}

}  // extern "C"
