"""CPU: the lookahead contract.  The numpy model of it
(tests/lookahead_model.py) against its own stated properties; the library's
host-side entry points (thor_lookahead_blocks, thor_lookahead_scenecut) against
Python; the exported symbols; and every argument error, none of which needs a
device."""
import ctypes as C

import numpy as np
import pytest

import lookahead_model as M
from thor_amd import lib as L


def _random(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def _shifted(cur, dy, dx):
    """The frame whose lowres plane holds cur's lowres pixel (y, x) at (y + dy, x + dx) (even sizes; wraps)."""
    assert cur.shape[0] % 2 == 0 and cur.shape[1] % 2 == 0
    return np.roll(cur, (2 * dy, 2 * dx), axis=(0, 1))


def _inside(w, h):
    """Mask (bh, bw) of the blocks whose whole search window lies inside the lowres plane."""
    bw, bh = M.blocks(w, h)
    ys, xs = 8 * np.arange(bh)[:, None], 8 * np.arange(bw)[None, :]
    return (ys >= M.RANGE) & (ys + 8 + M.RANGE <= h >> 1) & (xs >= M.RANGE) & (xs + 8 + M.RANGE <= w >> 1)


def test_lowres_and_block_grid():
    p = _random(19, 37, 1)
    l = M.lowres(p)
    assert l.shape == (18, 9)
    q = p.copy()
    q[:, 18] = 0  # the last odd column is not read
    q[36, :] = 0  # nor the last odd row
    assert (M.lowres(q) == l).all()
    y, x = 5, 3
    assert l[y, x] == (int(p[10, 6]) + int(p[10, 7]) + int(p[11, 6]) + int(p[11, 7]) + 2) >> 2
    assert M.blocks(16, 16) == (1, 1) and M.blocks(50, 38) == (3, 2) and M.blocks(3840, 2160) == (240, 135)
    assert (M.HADAMARD @ M.HADAMARD.T == 8 * np.eye(8)).all() and (M.HADAMARD[:, 0] == 1).all()
    assert M.HADAMARD[1].tolist() == [1, -1] * 4  # Sylvester order


def test_identical_frames():
    for w, h in ((16, 16), (50, 38), (144, 80)):
        cur = _random(w, h, w + h)
        rec, sums = M.frame(cur, cur.copy())
        assert (rec["sad"] == 0).all() and (rec["inter"] == 0).all()
        assert (rec["mvx"] == 0).all() and (rec["mvy"] == 0).all()
        assert sums[1] == 0 and sums[2] == 0 and sums[3] == 0 and sums[0] == int(rec["intra"].sum()) > 0


def test_flat_frames():
    w, h = 80, 48
    flat = np.full((h, w), 128, np.uint8)
    rec, sums = M.frame(flat, flat.copy())
    assert sums == [0, 0, 0, 0]
    for name in rec.dtype.names:
        assert (rec[name] == 0).all(), name
    # any other level: only the first block, whose DC predictor is the constant 128, has an intra cost
    other = np.full((h, w), 50, np.uint8)
    rec, sums = M.frame(other, np.full((h, w), 50, np.uint8))
    assert (rec["mvx"] == 0).all() and (rec["mvy"] == 0).all() and (rec["sad"] == 0).all() and (rec["inter"] == 0).all()
    want = np.zeros_like(rec["intra"])
    want[0, 0] = (64 * 78 + 2) >> 2
    assert (rec["intra"] == want).all()


@pytest.mark.parametrize("dy,dx", [(8, 8), (8, -8), (-8, 8), (-8, -8), (0, 5), (-3, 0)])
def test_shifted_reference_recovers_the_vector(dy, dx):
    w, h = 144, 112
    cur = _random(w, h, 3)
    rec, _ = M.frame(cur, _shifted(cur, dy, dx))
    ins = _inside(w, h)
    assert ins.sum() >= 8
    assert (rec["mvx"][ins] == dx).all() and (rec["mvy"][ins] == dy).all()
    assert (rec["sad"][ins] == 0).all() and (rec["inter"][ins] == 0).all()


def test_black_against_white():
    w, h = 48, 32
    rec, sums = M.frame(np.zeros((h, w), np.uint8), np.full((h, w), 255, np.uint8))
    assert (rec["sad"] == 16320).all() and (rec["inter"] == 4080).all()
    assert (rec["mvx"] == 0).all() and (rec["mvy"] == 0).all()  # every candidate ties: the shortest vector
    # black: first block against 128, every other block has a neighbour that predicts it exactly
    assert rec["intra"][0, 0] == (64 * 128 + 2) >> 2 and int(rec["intra"].sum()) == 2048
    assert sums == [2048, 4080 * 6, 2048, 6]


def _stripes(w, h, phase=0):
    """Vertical stripes of period 4 lowres pixels (8 source pixels), moved right by `phase` lowres pixels."""
    x = (np.arange(w) // 2 - phase) % 4
    return np.tile(np.array([10, 90, 170, 250], np.uint8)[x][None, :], (h, 1))


def test_tie_break_shortest_vector_then_raster_order():
    w, h = 144, 112
    ins = _inside(w, h)
    cur = _stripes(w, h)
    # identical: every (dy, dx) with dx = 0 mod 4 has SAD 0; the shortest is (0, 0)
    rec, _ = M.frame(cur, cur.copy())
    assert (rec["sad"] == 0).all() and (rec["mvx"] == 0).all() and (rec["mvy"] == 0).all()
    # moved by 2: SAD 0 at dx in {-6, -2, 2, 6}, any dy; the shortest are (0, -2) and (0, 2), and -2 is first in raster order
    rec, _ = M.frame(cur, _stripes(w, h, 2))
    assert (rec["sad"][ins] == 0).all() and (rec["mvy"][ins] == 0).all() and (rec["mvx"][ins] == -2).all()
    # moved by 1: SAD 0 at dx in {-7, -3, 1, 5}: the shortest alone decides
    rec, _ = M.frame(cur, _stripes(w, h, 1))
    assert (rec["sad"][ins] == 0).all() and (rec["mvy"][ins] == 0).all() and (rec["mvx"][ins] == 1).all()


def test_costs_fit_uint16():
    w, h = 80, 64
    rng = np.random.default_rng(5)
    a = _random(w, h, 6)
    binary = (rng.integers(0, 2, (h, w)) * 255).astype(np.uint8)
    binary2 = (rng.integers(0, 2, (h, w)) * 255).astype(np.uint8)
    checker = ((np.arange(h)[:, None] // 2 + np.arange(w)[None, :] // 2) % 2 * 255).astype(np.uint8)
    for name, (x, y) in {"random": (a, _random(w, h, 7)), "binary": (binary, binary2), "inverted": (a, 255 - a),
                         "binary_inverted": (binary, 255 - binary), "checker": (checker, 255 - checker)}.items():
        rec, sums = M.frame(x, y)
        assert int(rec["intra"].max()) <= 32640 and int(rec["inter"].max()) <= 32640, name
        assert int(rec["sad"].max()) <= 16320, name
        assert sums[2] <= min(sums[0], sums[1]) and 0 <= sums[3] <= rec.size, name
    # a flat or checkerboard difference of 255 is one coefficient of 64 * 255
    d = np.where((np.arange(8)[:, None] + np.arange(8)[None, :]) % 2 == 0, 255, -255)
    assert int(M.satd(d)) == 4080 and int(np.abs(M.HADAMARD @ d @ M.HADAMARD.T).sum()) == 16320
    worst = np.where(M.HADAMARD > 0, 255, -255)  # Parseval: sum |.| <= 8 * sqrt(64 * 255^2 * 64) = 130 560
    assert int(np.abs(M.HADAMARD @ worst @ M.HADAMARD.T).sum()) <= 130560


def test_intra_only_pair():
    cur = _random(50, 38, 9)
    rec, sums = M.frame(cur, None)
    assert (rec["inter"] == rec["intra"]).all() and (rec["sad"] == M.NO_SAD).all()
    assert (rec["mvx"] == 0).all() and (rec["mvy"] == 0).all()
    assert sums[0] == sums[1] == sums[2] and sums[3] == 0
    assert (rec["intra"] == M.frame(cur, cur)[0]["intra"]).all()


def test_synthetic_scene_cut():
    """352 x 288, seed 1 for t = 0..2, seed 2 for t = 3..5 (measured: 0.589-0.610 inside a scene, 0.970 at the
    seed change, 324 of 396 blocks intra there)."""
    from thor_amd import synth

    w, h = 352, 288
    frames = [synth.synth_frame(w, h, t, 1 if t < 3 else 2)[0] for t in range(6)]
    res = M.sequence(frames)
    ratio = [s[2] / s[0] for _, s in res]
    assert ratio[0] == 1.0
    for k in (1, 2, 4, 5):
        assert ratio[k] < 0.70, (k, ratio[k])
    assert ratio[3] > 0.90, ratio[3]
    assert res[3][1][3] > 396 // 2
    for percent in (70, 80, 90):
        assert [k for k, (_, s) in enumerate(res) if M.scenecut(s, percent)] == [0, 3]
    lib = L.load()
    for percent in (70, 90):
        got = [lib.thor_lookahead_scenecut((C.c_uint64 * 4)(*s), percent) for _, s in res]
        assert got == [1, 0, 0, 1, 0, 0]


def test_host_entry_points_against_python():
    lib = L.load()
    bw, bh = C.c_int(-1), C.c_int(-1)
    for w, h in ((16, 16), (17, 31), (48, 32), (50, 38), (272, 80), (352, 288), (3840, 2160), (16384, 16384)):
        n = lib.thor_lookahead_blocks(w, h, C.byref(bw), C.byref(bh))
        assert (bw.value, bh.value) == M.blocks(w, h) and n == bw.value * bh.value, (w, h)
        assert lib.thor_lookahead_blocks(w, h, None, None) == n
    for w, h in ((15, 16), (16, 15), (16385, 16), (16, 16386), (0, 0), (-16, 16)):
        assert lib.thor_lookahead_blocks(w, h, C.byref(bw), C.byref(bh)) == L.THOR_ERR_ARG, (w, h)
    rng = np.random.default_rng(3)
    cases = [[0, 0, 0, 0], [100, 50, 70, 3], [100, 50, 69, 3], [1, 1, 1, 0], [10, 0, 0, 0],
             [32640 << 20, 32640 << 20, 32640 << 20, 1 << 20]]
    cases += [[int(a), int(b), int(min(a, b) * f), 0] for a, b, f in zip(rng.integers(1, 1 << 34, 50),
                                                                            rng.integers(1, 1 << 34, 50), rng.random(50))]
    for s in cases:
        arr = (C.c_uint64 * 4)(*s)
        for percent in (1, 50, 69, 70, 71, 90, 100):
            assert lib.thor_lookahead_scenecut(arr, percent) == int(M.scenecut(s, percent)), (s, percent)
        for percent in (0, -1, 101, 1000):
            assert lib.thor_lookahead_scenecut(arr, percent) == L.THOR_ERR_ARG
    assert lib.thor_lookahead_scenecut(None, 50) == L.THOR_ERR_ARG


def test_python_scene_cuts():
    from thor_amd import lookahead

    sums = np.array([[100, 100, 100, 0], [100, 50, 50, 1], [100, 120, 95, 9], [0, 0, 0, 0]], np.uint64)
    assert lookahead.scene_cuts(sums, 90) == [0, 2]
    assert lookahead.scene_cuts(sums, 50) == [0, 1, 2]
    assert lookahead.scene_cuts(sums, 96) == [0]
    with pytest.raises(ValueError):
        lookahead.scene_cuts(sums, 0)
    assert lookahead.block_grid(50, 38) == (3, 2)
    with pytest.raises(ValueError):
        lookahead.block_grid(8, 8)
    assert lookahead.BLOCK == M.BLOCK and lookahead.BLOCK.itemsize == 8


def test_symbols_and_argument_errors():
    lib = L.load()
    for name in ("thor_lookahead_blocks", "thor_lookahead_i420", "thor_lookahead_scenecut", "thor_d2h_stream"):
        assert name in L.BATCHED_SYMBOLS and getattr(lib, name).argtypes is not None, name
    # every argument error is found before any device call (no GPU needed): the pointers are never followed
    one = (L.ThorYuvPlanes * 1)(L.ThorYuvPlanes(16, None, None, 16, 8))
    sums, recs = C.c_void_p(64), C.c_void_p(128)
    E = L.THOR_ERR_ARG
    f = lib.thor_lookahead_i420
    assert f(None, one, 1, 16, 16, recs, sums, None) == E
    assert f(one, one, 1, 16, 16, recs, None, None) == E
    assert f(one, one, 0, 16, 16, recs, sums, None) == E
    assert f(one, one, -1, 16, 16, recs, sums, None) == E
    assert f(one, one, 65536, 16, 16, recs, sums, None) == E
    assert f(one, one, 1, 15, 16, recs, sums, None) == E
    assert f(one, one, 1, 16, 15, recs, sums, None) == E
    assert f(one, one, 1, 16385, 16, recs, sums, None) == E
    assert f(one, one, 1, 16, 16385, recs, sums, None) == E
    assert f(one, one, 1, 16, 16, C.c_void_p(130), sums, None) == E  # records are 8-byte aligned
    assert f(one, one, 1, 16, 16, recs, C.c_void_p(68), None) == E
    null_y = (L.ThorYuvPlanes * 1)(L.ThorYuvPlanes(None, 32, 48, 16, 8))
    assert f(null_y, one, 1, 16, 16, recs, sums, None) == E
    narrow = (L.ThorYuvPlanes * 1)(L.ThorYuvPlanes(16, None, None, 15, 8))
    assert f(narrow, one, 1, 16, 16, recs, sums, None) == E
    assert f(one, narrow, 1, 16, 16, recs, sums, None) == E
    two = (L.ThorYuvPlanes * 2)(L.ThorYuvPlanes(16, None, None, 16, 8), L.ThorYuvPlanes(None, None, None, 16, 8))
    assert f(two, two, 2, 16, 16, recs, sums, None) == E  # the second cur has no luma
    assert lib.thor_d2h_stream(None, sums, 8, None) == E
    assert lib.thor_d2h_stream(sums, None, 8, None) == E
    assert lib.thor_d2h_stream(sums, sums, 0, None) == E
