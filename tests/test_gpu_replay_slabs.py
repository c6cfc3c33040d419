"""A replay of a planned batch keeps the slab table, bboxes and bins the previous render of the same plan left: k_path_bbox is not
launched again (four launches instead of five), k_path_build<1> checks the paths' keys against the kept records.  Here: the launch
counts, and that nothing which voids the plan -- new transforms, a change of the owned bands, a new plan -- or passes between two
replays -- a window render -- ever lets a render read a table that is not its own: every picture against a FRESH batch of the same
inputs, bit for bit (deterministic renders: the order of the adds is fixed)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZE, N = 1024, 1200


@pytest.fixture(scope="module")
def S():
    import svgrasterize_amd as S

    S.Context.get()
    return S


@pytest.fixture(scope="module")
def sc():
    from svgrasterize_amd import synth

    scene = synth.make_scene(SIZE, N)
    assert len(scene["seg_kind"]) > 4096   # (a plan orders the slabs of a batch of more than 4096 segments: only such a batch keeps its lists)
    return scene


def _new(S, sc, m6=None):
    from svgrasterize_amd import _abi

    return _abi.Batch(S.Context.get(), sc["segs"], sc["seg_kind"], sc["path_seg_off"], sc["path_m6"] if m6 is None else m6,
                      sc["path_rule"], sc["path_paint"], viewport=list(sc["viewport"]))


def _moved(sc, d_rows, d_cols):
    m6 = np.array(sc["path_m6"], dtype=np.float64, copy=True).reshape(-1, 6)
    m6[:, 2] += d_rows
    m6[:, 5] += d_cols
    return m6


def _flags():
    from svgrasterize_amd import _abi

    return _abi.RENDER_CLIP01 | _abi.RENDER_DETERMINISTIC


def _canvas(out):
    return out.download((SIZE, SIZE, 4), np.float32)


def _render(b, out):
    from svgrasterize_amd import _abi

    b.render(out, _abi.OUT_CANVAS_F32, _flags())
    return _canvas(out)


def _fresh(S, sc, m6=None):
    """the picture of a new batch of the same inputs: plan + one deterministic render"""
    ctx = S.Context.get()
    b = _new(S, sc, m6)
    out = ctx.alloc(SIZE * SIZE * 16)
    b.plan()
    want = _render(b, out)
    b.destroy()
    out.free()
    assert want.any()
    return want


def _replayed(S, sc, out, n=3):
    """a planned batch that has been replayed `n` times: the last of them kept the slab table"""
    b = _new(S, sc)
    b.plan()
    for _ in range(n):
        got = _render(b, out)
    return b, got


def test_a_replay_is_four_launches(S, sc):
    """plan, the render that finds the plan's own pass, the first replay (it writes the slabs at the plan's heaviest-first places:
    five launches at most), then every further replay: flatten, path build, tile lists, tile kernel."""
    from svgrasterize_amd import _abi

    ctx = S.Context.get()
    out = ctx.alloc(SIZE * SIZE * 16)
    b = _new(S, sc)
    b.plan()
    for k in range(2):
        n0 = ctx.launches()
        b.render(out, _abi.OUT_CANVAS_F32, _abi.RENDER_CLIP01)
        assert ctx.launches() - n0 <= 5, k
    first = _canvas(out)
    for k in range(3):
        n0 = ctx.launches()
        b.render(out, _abi.OUT_CANVAS_F32, _abi.RENDER_CLIP01)
        assert ctx.launches() - n0 == 4, k
    ctx.sync()
    err = np.abs(_canvas(out).astype(np.float64) - first.astype(np.float64)).max()
    print(f"replay with the kept table against the first replay: max abs difference {err:.3e}")
    assert err <= 2.0 ** -23    # (float32 canvas in [0, 1]: one ulp at 1.0 -- the adds' order is free without the deterministic flag)
    # the other outputs go through the same pass
    n0 = ctx.launches()
    b.render(out, _abi.OUT_CANVAS_F32, _flags())
    assert ctx.launches() - n0 == 4
    b.destroy()
    out.free()


def test_new_transforms_void_the_kept_table(S, sc):
    """set_transforms, draw, render, render: each picture is the fresh batch's for the moved transforms."""
    from svgrasterize_amd import _abi

    ctx = S.Context.get()
    out = ctx.alloc(SIZE * SIZE * 16)
    b, got = _replayed(S, sc, out)
    assert np.array_equal(got, _fresh(S, sc))
    m6 = _moved(sc, 3.375, -2.0625)
    want = _fresh(S, sc, m6)
    b.set_transforms(m6)
    b.draw(out, _abi.OUT_CANVAS_F32, _flags())
    assert np.array_equal(_canvas(out), want), "draw after set_transforms"
    for k in range(3):
        assert np.array_equal(_render(b, out), want), f"replay {k} after set_transforms + draw"
    b.destroy()
    out.free()


def test_a_stale_table_is_never_read(S, sc):
    """plan, replay twice, then a shift of several tiles and a draw: the paths' slabs, bboxes and bins are all elsewhere."""
    from svgrasterize_amd import _abi

    ctx = S.Context.get()
    out = ctx.alloc(SIZE * SIZE * 16)
    b, _ = _replayed(S, sc, out, n=3)
    m6 = _moved(sc, 5.0 * _abi.tile_rows() + 0.5, -3.0 * _abi.tile_cols() - 0.25)
    want = _fresh(S, sc, m6)
    assert not np.array_equal(want, _fresh(S, sc))
    b.set_transforms(m6)
    b.draw(out, _abi.OUT_CANVAS_F32, _flags())
    assert np.array_equal(_canvas(out), want), "draw after a shift of several tiles"
    for k in range(2):
        assert np.array_equal(_render(b, out), want), f"replay {k} after the shift"
    # ... and back, through plan() instead of draw()
    b.set_transforms(sc["path_m6"])
    b.plan()
    want0 = _fresh(S, sc)
    for k in range(3):
        assert np.array_equal(_render(b, out), want0), f"replay {k} after moving back"
    b.destroy()
    out.free()


def test_set_bands_voids_the_kept_table(S, sc):
    """set_bands on one rank (world = 1: the ABI shards by interleaved strips, a rank of one owns every band): the plan is void, the
    new plan's first replay writes the table again."""
    ctx = S.Context.get()
    out = ctx.alloc(SIZE * SIZE * 16)
    b, _ = _replayed(S, sc, out)
    want = _fresh(S, sc)
    b.set_bands(0, 1, 3)
    b.plan()
    n_launch = []
    for k in range(4):
        n0 = ctx.launches()
        assert np.array_equal(_render(b, out), want), f"replay {k} after set_bands"
        n_launch.append(ctx.launches() - n0)
    assert n_launch[0] <= 5 and n_launch[1:] == [4, 4, 4], n_launch   # (a deterministic render does not take the plan's own pass)
    b.destroy()
    out.free()


def test_a_window_render_between_two_replays(S, sc):
    """a window of the canvas between whole renders: the window is the whole picture's part, and the renders behind it are whole."""
    from svgrasterize_amd import _abi

    ctx = S.Context.get()
    out = ctx.alloc(SIZE * SIZE * 16)
    b, got = _replayed(S, sc, out)
    want = _fresh(S, sc)
    assert np.array_equal(got, want)
    win = (3 * _abi.tile_rows(), 2 * _abi.tile_cols(), 20 * _abi.tile_rows(), 7 * _abi.tile_cols())
    wout = ctx.alloc(win[2] * win[3] * 16)
    b.render(wout, _abi.OUT_CANVAS_F32, _flags(), window=win)
    part = wout.download((win[2], win[3], 4), np.float32)
    assert np.array_equal(part, want[win[0]:win[0] + win[2], win[1]:win[1] + win[3]])
    for k in range(2):
        assert np.array_equal(_render(b, out), want), f"replay {k} after a window render"
    b.destroy()
    out.free()
    wout.free()


def test_a_drawn_batch_keeps_the_table_one_replay_later(S, sc):
    """svgr_batch_draw leaves the slab order to the first replay; that replay writes the table, the next one runs k_path_bbox once
    more (five launches: what tests/test_gpu_draw.py pins for it), and from then on a replay is four launches.  Same picture
    throughout."""
    from svgrasterize_amd import _abi

    ctx = S.Context.get()
    out = ctx.alloc(SIZE * SIZE * 16)
    b = _new(S, sc)
    b.draw(out, _abi.OUT_CANVAS_F32, _abi.RENDER_CLIP01)
    n_launch = []
    for _ in range(5):
        n0 = ctx.launches()
        b.render(out, _abi.OUT_CANVAS_F32, _abi.RENDER_CLIP01)
        n_launch.append(ctx.launches() - n0)
    assert n_launch[0] <= 5 and n_launch[1] == 5 and n_launch[2:] == [4, 4, 4], n_launch
    assert np.array_equal(_render(b, out), _fresh(S, sc))
    b.destroy()
    out.free()
