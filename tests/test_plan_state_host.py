"""The batch's plan state (svgrasterize.py_amd/csrc/svgr_plan_state.h) on the CPU: the flags that say whether a plan stands, the three
results a replay may keep on the device (slab table, tile lists, cells) and the named transitions, through tests/plan_state_harness.cpp,
which includes that header alone and drives it as run_geometry does.

What a transition clears is stated here once more, on purpose: a transition that starts to clear more, or less, fails here first."""
import ctypes
import struct

import numpy as np
import pytest

from tests.util import host_build

P, V, Q, L, S, T, C = 1, 2, 4, 8, 16, 32, 64   # planned, slab_at_valid, slab_order_pending, slab_order_late; slabs, lists, cells held
ALL = P | V | Q | L | S | T | C
SLABS, LISTS, CELLS = 0, 1, 2
# name -> (number in the harness, clears, sets)
TRANSITIONS = {
    "geometry_changed": (0, P | V | Q | S | T | C, 0),
    "plan_begins": (1, P | V | Q | S | T | C, 0),
    "plan_made": (2, 0, P),
    "pass_withdrawn": (3, P | S | T, 0),
    "slab_order_begins": (4, V | L | S | T, 0),
    "slab_order_made": (5, 0, V),
    "slab_order_left_to_replay(large)": (6, 0, Q),
    "slab_order_left_to_replay(small)": (7, Q, 0),
    "slab_order_taken_up": (8, Q, 0),
    "slab_order_made_late": (9, 0, L),
    "arrays_inherited": (10, V | S | T | C, 0),
    "masks_resized": (11, T, 0),
    "paints_changed": (12, C, 0),
    "pass_failed": (13, S | T | C, 0),
}


@pytest.fixture(scope="module")
def lib():
    so = host_build("plan_state_harness")
    so.ps_holds.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    so.ps_wrote.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    so.ps_print_of.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_double,
                               ctypes.c_void_p, ctypes.c_void_p]
    return so


def _words(lib, seed):
    return np.random.default_rng(seed).integers(1, 2 ** 63, lib.ps_print_words(), dtype=np.uint64)


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


PRINTS = {SLABS: 11, LISTS: 12, CELLS: 13}   # seeds of the three fingerprints a placed pass records here


def _placed_pass(lib, which=(SLABS, LISTS, CELLS)):
    """a placed pass under the plan: writes (and may keep) each of `which`"""
    for w in which:
        lib.ps_wrote(w, 1, _ptr(_words(lib, PRINTS[w])))


def _holds(lib, which, eligible=True):
    return bool(lib.ps_holds(which, int(eligible), _ptr(_words(lib, PRINTS[which]))))


def _all_set(lib):
    lib.ps_reset()
    for name in ("plan_made", "slab_order_made", "slab_order_left_to_replay(large)"):
        assert lib.ps_apply(TRANSITIONS[name][0]) == 0
    _placed_pass(lib)
    lib.ps_apply(TRANSITIONS["slab_order_made_late"][0])
    assert lib.ps_flags() == ALL


def test_the_table_names_every_transition(lib):
    assert sorted(n for n, _c, _s in TRANSITIONS.values()) == list(range(len(TRANSITIONS)))
    assert lib.ps_apply(len(TRANSITIONS)) == -1
    lib.ps_reset()
    assert lib.ps_flags() == 0   # (a new batch: nothing stands, nothing is kept)


@pytest.mark.parametrize("name", sorted(TRANSITIONS))
def test_a_transition_clears_exactly_its_flags(lib, name):
    k, clears, sets = TRANSITIONS[name]
    _all_set(lib)
    assert lib.ps_apply(k) == 0
    assert lib.ps_flags() == (ALL & ~clears) | sets, (name, "from the all-set state", bin(lib.ps_flags()))
    lib.ps_reset()
    assert lib.ps_apply(k) == 0
    assert lib.ps_flags() == sets, (name, "from the all-clear state", bin(lib.ps_flags()))


def test_holds_needs_an_eligible_pass(lib):
    _all_set(lib)
    for which in (SLABS, LISTS, CELLS):
        assert _holds(lib, which) and not _holds(lib, which, eligible=False)
    lib.ps_reset()
    for which in (SLABS, LISTS, CELLS):
        assert not _holds(lib, which) and not _holds(lib, which, eligible=False)


@pytest.mark.parametrize("which", (SLABS, LISTS, CELLS))
def test_a_fingerprint_differs_in_any_single_word(lib, which):
    _all_set(lib)
    made = _words(lib, PRINTS[which])
    assert lib.ps_holds(which, 1, _ptr(made)) == 1
    for at in range(len(made)):
        for flip in (1, 1 << 31, 1 << 63):
            now = made.copy()
            now[at] ^= np.uint64(flip)
            assert lib.ps_holds(which, 1, _ptr(now)) == 0, (at, flip)
    assert lib.ps_holds(which, 1, _ptr(made)) == 1   # (asking changes nothing)


def test_plan_print_packs_every_value_into_words_of_its_own(lib):
    n_words = lib.ps_print_words()
    block = np.arange(100, 133, dtype=np.int32)

    def words(p0=0x1000, p1=0x2000, n=7, a=-1, b=3, thr=0.16, blk=block):
        out = np.full(n_words, 0xdead, dtype=np.uint64)
        lib.ps_print_of(p0, p1, n, a, b, thr, _ptr(np.ascontiguousarray(blk)), _ptr(out))
        return out

    base = words()
    want = [0x1000, 0x2000, 7, 0xffffffff, 3, struct.unpack("<Q", struct.pack("<d", 0.16))[0]]
    want += [int(block[2 * k]) | (int(block[2 * k + 1]) << 32) for k in range(16)] + [int(block[32])]
    assert [int(v) for v in base] == want + [0] * (n_words - len(want))
    # one value changed: exactly its word differs (the bit pattern of the threshold: -0.0 is not 0.0)
    for kw, at in ((dict(p0=0x1008), 0), (dict(p1=0), 1), (dict(n=1 << 40), 2), (dict(a=0), 3), (dict(b=-3), 4), (dict(thr=0.16000000000000003), 5)):
        assert list(np.flatnonzero(words(**kw) != base)) == [at], kw
    assert list(np.flatnonzero(words(thr=-0.0) != words(thr=0.0))) == [5]
    for k in range(33):
        blk = block.copy()
        blk[k] += 1
        assert list(np.flatnonzero(words(blk=blk) != base)) == [6 + k // 2], k


def test_after_a_pass_that_ended_with_an_error_flag_nothing_is_kept(lib):
    _all_set(lib)
    lib.ps_apply(TRANSITIONS["pass_failed"][0])
    assert [_holds(lib, w) for w in (SLABS, LISTS, CELLS)] == [False] * 3
    assert lib.ps_flags() & P   # (the plan itself stands: its caller decides)


def test_a_render_that_made_the_slab_order_itself_does_not_keep_its_table(lib):
    lib.ps_reset()
    for name in ("plan_made", "slab_order_left_to_replay(large)", "slab_order_taken_up", "slab_order_begins", "slab_order_made", "slab_order_made_late"):
        lib.ps_apply(TRANSITIONS[name][0])
    assert lib.ps_flags() == P | V | L
    _placed_pass(lib, (SLABS,))
    assert not _holds(lib, SLABS) and lib.ps_flags() == P | V   # (written, not kept; the order is the plan's from here on)
    _placed_pass(lib, (SLABS,))
    assert _holds(lib, SLABS)


# ------------------------------------------------------------------------------- the cells: every row of the header's table
def _lean_ready(lib):
    """plan, slab order, one full placed pass: the next placed pass may be the lean form"""
    lib.ps_reset()
    for name in ("plan_begins", "plan_made", "slab_order_begins", "slab_order_made"):
        lib.ps_apply(TRANSITIONS[name][0])
    _placed_pass(lib)
    assert lib.ps_flags() == P | V | S | T | C


def test_cells_a_pass_that_is_not_a_whole_placed_pass_voids_them(lib):
    # a measuring pass, an unplanned pass (<0>, <2>), one rank of several, groups or gradients: run_geometry records `wrote(false, ..)`
    _lean_ready(lib)
    lib.ps_wrote(CELLS, 0, _ptr(_words(lib, PRINTS[CELLS])))
    assert not _holds(lib, CELLS)
    # a pass without slabs, or one that stops short of the path build: `drop`
    _lean_ready(lib)
    lib.ps_drop(CELLS)
    assert not _holds(lib, CELLS)
    # a pass that ends in an error
    _lean_ready(lib)
    lib.ps_apply(TRANSITIONS["pass_failed"][0])
    assert not _holds(lib, CELLS)


def test_cells_placed_passes_of_any_output_leave_them_valid(lib):
    # a deterministic render (the full form), the pass in front of a window or a float64 canvas: placed passes into the same blocks
    _lean_ready(lib)
    for _nth in range(3):
        _placed_pass(lib)
        assert _holds(lib, CELLS) and _holds(lib, SLABS) and _holds(lib, LISTS)
    # ... into other blocks, or with another paint array: the pass that finds them writes everything, the one behind it keeps
    other = _words(lib, 99)
    assert lib.ps_holds(CELLS, 1, _ptr(other)) == 0
    lib.ps_wrote(CELLS, 1, _ptr(other))
    assert lib.ps_holds(CELLS, 1, _ptr(other)) == 1 and not _holds(lib, CELLS)


def test_cells_new_paints_ask_for_one_full_pass_and_nothing_else(lib):
    _lean_ready(lib)
    lib.ps_apply(TRANSITIONS["paints_changed"][0])
    assert not _holds(lib, CELLS) and _holds(lib, SLABS) and _holds(lib, LISTS) and lib.ps_flags() & P
    _placed_pass(lib, (CELLS,))
    assert _holds(lib, CELLS)


@pytest.mark.parametrize("name", ("geometry_changed", "plan_begins", "arrays_inherited"))
def test_cells_new_geometry_a_new_plan_and_inherited_arrays_void_them(lib, name):
    _lean_ready(lib)
    lib.ps_apply(TRANSITIONS[name][0])
    assert not _holds(lib, CELLS)
    # ... and stay void through the planner's unplanned pass until a placed pass has written them
    lib.ps_wrote(CELLS, 0, _ptr(_words(lib, PRINTS[CELLS])))
    lib.ps_apply(TRANSITIONS["plan_made"][0])
    assert not _holds(lib, CELLS)
    _placed_pass(lib, (CELLS,))
    assert _holds(lib, CELLS)


def test_cells_a_new_batch_starts_without_them(lib):
    lib.ps_reset()
    assert not _holds(lib, CELLS)
    assert lib.ps_holds(CELLS, 1, _ptr(np.zeros(lib.ps_print_words(), dtype=np.uint64))) == 0   # (not even for the empty fingerprint)
