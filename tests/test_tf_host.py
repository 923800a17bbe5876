"""CPU: the temporal-filter contract.  The numpy model of it
(tests/tf_model.py) against its own stated properties; the library's host-side
entry points (thor_tf_check, thor_tf_mult, thor_tf_blocks) against Python; the
exported symbols; and every argument error, none of which needs a device.  (The
kernels divide with the plain integer `/`: there is no reciprocal to check.)"""
import ctypes as C
import math

import numpy as np
import pytest

import tf_model as M
from thor_amd import lib as L


def _random_frame(w, h, seed):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h // 2, w // 2), dtype=np.uint8),
            rng.integers(0, 256, (h // 2, w // 2), dtype=np.uint8))


def _smooth(w, h, seed):
    """A smooth luma plane (a random field through a 3x3 box, stretched to full contrast): smooth enough for the
    half-resolution stage to land next to an odd or half-pel displacement, textured enough for one least SAD."""
    rng = np.random.default_rng(seed)
    p = rng.integers(0, 256, (h + 32, w + 32)).astype(np.float64)
    p = sum(np.roll(p, k, 0) for k in (-1, 0, 1)) / 3
    p = sum(np.roll(p, k, 1) for k in (-1, 0, 1)) / 3
    p = (p - p.min()) / (p.max() - p.min()) * 255
    return np.rint(p[16:-16, 16:-16]).astype(np.uint8)


def _inside(w, h, reach=16 + M.IR + 2):
    """Mask (bh8, bw8) of the 8x8 blocks whose combined search window (start +-16, refinement +-2, the half-pel
    neighbours) lies inside the plane."""
    bw8, bh8 = M.blocks(w, h)
    ys, xs = 8 * np.arange(bh8)[:, None], 8 * np.arange(bw8)[None, :]
    return (ys >= reach) & (ys + 8 + reach <= h) & (xs >= reach) & (xs + 8 + reach <= w)


def test_lut_and_mult():
    for k in range(63):
        assert M.LUT[k] == math.floor(256 * math.exp(-k / 16) + 0.5), k
    assert M.LUT[63] == 0 and M.LUT[0] == 256
    assert M.mult(1) == 1 << 20 and M.mult(8) == 16384 and M.mult(3) == 116508 and M.mult(64) == 256
    # the product fits 32 bits, the numerator and the denominator their stated bounds
    assert 2047 * max(M.mult(s) for s in range(1, 65)) < 1 << 32
    assert 256 * 255 + 4 * 256 * 255 == 326400 and 256 + 4 * 256 == 1280


def test_identical_references_leave_the_target_unchanged():
    for w, h in ((16, 16), (24, 40), (48, 32)):
        T = _random_frame(w, h, w + h)
        out, recs = M.frame(T, [tuple(p.copy() for p in T)] * 3, (8, 3))
        for c in range(3):
            assert (out[c] == T[c]).all()
        assert (recs["e"] == 0).all() and (recs["mvx"] == 0).all() and (recs["mvy"] == 0).all()


def test_inverted_top_bit_references_leave_the_target_unchanged():
    """With every |d| >= 64, m = (d d + e) >> 1 passes 2047 and k = min(63, (2047 * mult) >> 16): 63, weight 0,
    for every strength up to 22.  From 23 on the clamp of m keeps k below 63 and the least weight above 0 (sec. 7g
    says so): the property is one of the strengths up to 22, the defaults among them.  A target with samples in
    [32, 96) has |d| in (64, 192) wherever the vectors point; a full-range random one is checked at the defaults."""
    assert all((2047 * M.mult(s)) >> 16 >= 63 for s in range(1, 23))
    assert (2047 * M.mult(23)) >> 16 == 61 and (2047 * M.mult(64)) >> 16 == 7
    for w, h in ((16, 16), (24, 40), (48, 32)):
        T = tuple(32 + (p >> 2) for p in _random_frame(w, h, 3 * w + h))
        X = tuple(p ^ 0x80 for p in T)
        for strength in ((1, 1), (8, 3), (22, 22)):
            out, _ = M.frame(T, [X, X, X, X], strength)
            for c in range(3):
                assert (out[c] == T[c]).all(), (w, h, strength, c)
        T = _random_frame(w, h, 3 * w + h)
        out, _ = M.frame(T, [tuple(p ^ 0x80 for p in T)] * 2, (8, 3))
        assert all((out[c] == T[c]).all() for c in range(3)), (w, h)


def test_absent_references():
    w, h = 24, 40
    T, R = _random_frame(w, h, 1), _random_frame(w, h, 2)
    out, recs = M.frame(T, [None, None], (8, 3))
    assert all((out[c] == T[c]).all() for c in range(3)) and not recs.view(np.uint32).any()
    a, ra = M.frame(T, [R, None, R], (8, 3))
    b, rb = M.frame(T, [R, R], (8, 3))
    assert all((a[c] == b[c]).all() for c in range(3))
    assert (ra[0] == rb[0]).all() and (ra[2] == rb[1]).all() and not ra[1].view(np.uint32).any()


@pytest.mark.parametrize("dy,dx", [(16, 16), (16, -16), (-16, 16), (-16, -16), (0, 5), (-3, 0), (7, -12), (15, -15)])
def test_whole_pixel_shift_recovers_the_vector(dy, dx):
    """The reference holds the target's pixel (y, x) at (y + dy, x + dx).  The displacements are those the
    half-resolution stage can see (+-8 of its pixels): the corners of its reach on white noise (an even shift is a
    whole shift there), odd ones on smooth content, where it lands next to them and the refinement does the rest.
    (A displacement of 17 or 18 is inside the combined window, but the coarse stage has no candidate there and
    finds the neighbouring one only on very smooth content: test_gpu_tf.py drives those corners for coverage.)"""
    w, h = 144, 112
    T = np.random.default_rng(3).integers(0, 256, (h, w), dtype=np.uint8) if dy % 2 == 0 and dx % 2 == 0 else _smooth(w, h, 3)
    rec = M.motion(T, np.roll(T, (dy, dx), axis=(0, 1)))
    ins = _inside(w, h)
    assert ins.sum() >= 8
    assert (rec["mvx"][ins] == 2 * dx).all() and (rec["mvy"][ins] == 2 * dy).all() and (rec["e"][ins] == 0).all()


@pytest.mark.parametrize("mvy,mvx", [(0, 1), (1, 0), (1, 1), (-5, 3), (7, -9), (-1, -1)])
def test_half_pel_prediction_of_a_smooth_image_recovers_the_vector(mvy, mvx):
    """The target is the contract's own half-pel prediction of a smooth reference."""
    w, h = 144, 112
    R = _smooth(w, h, 7)
    y0, x0 = M._grid(w, h, 8)
    T = M._untile(M.predict(R, y0, x0, 8, np.full(len(y0), mvy), np.full(len(y0), mvx)), w, h, 8).astype(np.uint8)
    rec = M.motion(T, R)
    ins = _inside(w, h)
    assert (rec["mvx"][ins] == mvx).all() and (rec["mvy"][ins] == mvy).all() and (rec["e"][ins] == 0).all()


def test_tie_break_prefers_the_zero_vector_on_a_flat_block():
    w, h = 48, 32
    flat = np.full((h, w), 77, np.uint8)
    rec = M.motion(flat, np.full((h, w), 80, np.uint8))
    assert (rec["mvx"] == 0).all() and (rec["mvy"] == 0).all() and (rec["e"] == 9).all()


def test_predict_cases_and_clamp():
    R = np.arange(64, dtype=np.uint8).reshape(8, 8) * 3
    a = M.predict(R, [2], [3], 2, [0], [0])[0]
    assert (a == R[2:4, 3:5]).all()
    assert (M.predict(R, [2], [3], 2, [0], [1])[0] == (R[2:4, 3:5].astype(int) + R[2:4, 4:6] + 1) >> 1).all()
    assert (M.predict(R, [2], [3], 2, [1], [0])[0] == (R[2:4, 3:5].astype(int) + R[3:5, 3:5] + 1) >> 1).all()
    assert (M.predict(R, [2], [3], 2, [1], [1])[0] ==
            (R[2:4, 3:5].astype(int) + R[2:4, 4:6] + R[3:5, 3:5] + R[3:5, 4:6] + 2) >> 2).all()
    # -1 in half pels: the integer part is -1 (floor), the fraction 1
    assert (M.predict(R, [2], [3], 2, [-1], [0])[0] == (R[1:3, 3:5].astype(int) + R[2:4, 3:5] + 1) >> 1).all()
    assert (M.predict(R, [0], [0], 2, [-8], [-8])[0] == R[0, 0]).all()  # clamped
    assert (M.predict(R, [6], [6], 2, [9], [9])[0] == R[7, 7]).all()


def test_quality_on_the_synthetic_clip():
    """352 x 288, seed 1, t = 2 from t = 0, 1, 3, 4, strengths (8, 3), against the noise-free frame (measured with
    this model: luma 0.261, U 0.674, V 0.674 of the unfiltered SSE; luma 0.670 with all vectors zero, so found /
    zero = 0.39).  The bounds are those figures with a quarter added."""
    from thor_amd import synth

    w, h, t0 = 352, 288, 2
    fr = [synth.synth_frame(w, h, t) for t in range(5)]
    clean = (synth._plane(w, h, t0, 1, 1, synth._LUMA_OCT, 0, 3, 128),
             synth._plane(w // 2, h // 2, t0, 1001, 2, synth._CHROMA_OCT, 0, 1, 120),
             synth._plane(w // 2, h // 2, t0, 2001, 2, synth._CHROMA_OCT, 0, 1, 136))
    T, refs = fr[t0], [fr[t] for t in (0, 1, 3, 4)]

    def sse(planes):
        return [int(((planes[c].astype(np.int64) - clean[c]) ** 2).sum()) for c in range(3)]

    base = sse(T)
    found = sse(M.frame(T, refs, (8, 3))[0])
    zero = sse(M.frame(T, refs, (8, 3), zero=True)[0])
    print("unfiltered", base, "filtered", found, "zero vectors", zero)
    assert found[0] < 0.33 * base[0] and found[1] < 0.85 * base[1] and found[2] < 0.85 * base[2]
    assert found[0] < 0.5 * zero[0]


def test_host_entry_points_against_python():
    lib = L.load()
    for s in range(1, 65):
        assert lib.thor_tf_mult(s) == M.mult(s), s
    for s in (0, -1, 65, 1000):
        assert lib.thor_tf_mult(s) == L.THOR_ERR_ARG
    bw, bh = C.c_int(-1), C.c_int(-1)
    for w, h in ((16, 16), (24, 40), (48, 32), (352, 288), (3840, 2160), (16384, 16384), (16384, 16), (16, 16384)):
        assert lib.thor_tf_blocks(w, h, C.byref(bw), C.byref(bh)) == (w >> 3) * (h >> 3)
        assert (bw.value, bh.value) == M.blocks(w, h)
        assert lib.thor_tf_blocks(w, h, None, None) == (w >> 3) * (h >> 3)
    for w, h in ((8, 16), (16, 8), (17, 16), (16, 20), (16392, 16), (16, 16392), (0, 0), (-16, 16)):
        assert lib.thor_tf_blocks(w, h, C.byref(bw), C.byref(bh)) == L.THOR_ERR_ARG, (w, h)
    for w in (0, 8, 12, 16, 20, 24, 352, 16384, 16392):
        for h in (8, 16, 36, 40, 16384, 16400):
            for nrefs in (0, 1, 2, 4, 5):
                assert (lib.thor_tf_check(w, h, nrefs) == 0) == M.check(w, h, nrefs), (w, h, nrefs)


def test_python_wrappers_without_a_device():
    from thor_amd import tfilter

    assert tfilter.RECORD == M.RECORD and tfilter.RECORD.itemsize == 4
    assert tfilter.mult(8) == 16384 and tfilter.block_grid(24, 40) == (3, 5)
    assert tfilter.size_ok(24, 40, 4) and not tfilter.size_ok(24, 40, 5) and not tfilter.size_ok(20, 40)
    with pytest.raises(ValueError):
        tfilter.mult(0)
    with pytest.raises(ValueError):
        tfilter.block_grid(20, 16)
    with pytest.raises(ValueError):
        tfilter.TemporalFilter(20, 16)
    with pytest.raises(ValueError):
        tfilter.TemporalFilter(16, 16, 0)
    with pytest.raises(ValueError):
        tfilter.filter_sequence(4096, 8192, 3, 16, 16, radius=3)
    assert tfilter.sequence_refs(0, 6, 2) == [None, None, 1, 2] and tfilter.sequence_refs(5, 6, 1) == [4, None]
    assert tfilter.sequence_refs(3, 6, 2) == [1, 2, 4, 5]


class _FakeTf(C.Structure):
    """The head of the library's context, enough for the argument checks (which never reach the device)."""
    _fields_ = [("w", C.c_int), ("h", C.c_int), ("max_targets", C.c_int), ("device", C.c_int),
                ("la", C.c_void_p), ("sums", C.c_void_p), ("recs", C.c_void_p)]


def test_symbols_and_argument_errors():
    lib = L.load()
    for name in ("thor_tf_check", "thor_tf_mult", "thor_tf_blocks", "thor_tf_create", "thor_tf_destroy", "thor_tf_i420"):
        assert name in L.BATCHED_SYMBOLS and getattr(lib, name).argtypes is not None, name
    assert not lib.thor_tf_create(20, 16, 1, 0) and not lib.thor_tf_create(16, 16, 0, 0)
    assert not lib.thor_tf_create(16, 16, L.THOR_TF_MAX_TARGETS + 1, 0)
    lib.thor_tf_destroy(None)
    # every argument error is found before any device call (no GPU needed): the pointers are never followed
    ctx = _FakeTf(16, 16, 2, 0, None, None, None)
    t = C.addressof(ctx)
    PL = L.ThorYuvPlanes
    cur = (PL * 2)(PL(0x1000, 0x1100, 0x1140, 16, 8), PL(0x2000, 0x2100, 0x2140, 16, 8))
    ref = (PL * 4)(PL(0x3000, 0x3100, 0x3140, 16, 8), PL(None, None, None, 0, 0), PL(0x4000, 0x4100, 0x4140, 16, 8),
                   PL(0x5000, 0x5100, 0x5140, 16, 8))
    dst = (PL * 2)(PL(0x6000, 0x6100, 0x6140, 16, 8), PL(0x7000, 0x7100, 0x7140, 16, 8))
    mv = C.c_void_p(0x8000)
    E = L.THOR_ERR_ARG
    f = lib.thor_tf_i420
    assert f(None, cur, ref, dst, 2, 2, 8, 3, mv, None) == E
    assert f(t, None, ref, dst, 2, 2, 8, 3, mv, None) == E
    assert f(t, cur, None, dst, 2, 2, 8, 3, mv, None) == E
    assert f(t, cur, ref, None, 2, 2, 8, 3, mv, None) == E
    for n in (0, -1, 3):  # the context takes two targets
        assert f(t, cur, ref, dst, n, 1, 8, 3, mv, None) == E
    for nrefs in (0, -1, 5):
        assert f(t, cur, ref, dst, 1, nrefs, 8, 3, mv, None) == E
    for s in (0, -3, 65):
        assert f(t, cur, ref, dst, 2, 2, s, 3, mv, None) == E
        assert f(t, cur, ref, dst, 2, 2, 8, s, mv, None) == E
    assert f(t, cur, ref, dst, 2, 2, 8, 3, C.c_void_p(0x8002), None) == E  # records are 4-byte aligned

    def with_(arr, i, **kw):
        out = type(arr)(*[PL(p.y, p.u, p.v, p.stride_y, p.stride_c) for p in arr])
        for k, v in kw.items():
            setattr(out[i], k, v)
        return out

    for name in ("y", "u", "v"):
        assert f(t, with_(cur, 1, **{name: None}), ref, dst, 2, 2, 8, 3, mv, None) == E
        assert f(t, cur, ref, with_(dst, 0, **{name: None}), 2, 2, 8, 3, mv, None) == E
    for name in ("u", "v"):  # a present reference has all three planes
        assert f(t, cur, with_(ref, 2, **{name: None}), dst, 2, 2, 8, 3, mv, None) == E
    for name, v in (("stride_y", 15), ("stride_c", 7)):
        assert f(t, with_(cur, 0, **{name: v}), ref, dst, 2, 2, 8, 3, mv, None) == E
        assert f(t, cur, with_(ref, 3, **{name: v}), dst, 2, 2, 8, 3, mv, None) == E
        assert f(t, cur, ref, with_(dst, 1, **{name: v}), 2, 2, 8, 3, mv, None) == E
    # not in place: a dst plane equal to its cur plane or to one of its references' planes
    for name in ("y", "u", "v"):
        assert f(t, cur, ref, with_(dst, 0, **{name: getattr(cur[0], name)}), 2, 2, 8, 3, mv, None) == E
        assert f(t, cur, ref, with_(dst, 1, **{name: getattr(ref[2], name)}), 2, 2, 8, 3, mv, None) == E
        assert f(t, cur, ref, with_(dst, 1, **{name: getattr(ref[3], name)}), 2, 2, 8, 3, mv, None) == E
