"""CPU: the SSIM contract.  The numpy model of it
(tests/ssim_model.py) against its own stated properties and against an
independent float64 SSIM per window; the library's host-side entry points
(thor_ssim_windows, thor_ssim, thor_ssim_db) against Python; the exported
symbols; and every argument error, none of which needs a device."""
import ctypes as C
import math

import numpy as np
import pytest

import ssim_model as M
from thor_amd import lib as L


def _contents(w, h, seed=7):
    """name -> (a, b), the kinds of content the contract's bounds were stated for."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (h, w), dtype=np.uint8)
    b = rng.integers(0, 256, (h, w), dtype=np.uint8)
    noisy = np.clip(a.astype(np.int16) + rng.integers(-3, 4, (h, w)), 0, 255).astype(np.uint8)
    binary = (rng.integers(0, 2, (h, w)) * 255).astype(np.uint8)
    binary2 = (rng.integers(0, 2, (h, w)) * 255).astype(np.uint8)
    return {"random": (a, b), "noise": (a, noisy), "identical": (a, a.copy()), "inverted": (a, 255 - a),
            "binary": (binary, binary2), "binary_inverted": (binary, 255 - binary),
            "constant": (np.zeros((h, w), np.uint8), np.full((h, w), 255, np.uint8))}


def test_identical_planes_give_one_per_window():
    for w, h in ((8, 8), (18, 22), (72, 40)):
        a = _contents(w, h)["identical"][0]
        q = M.window_q(a, a)
        assert q.shape == ((h >> 2) - 1, (w >> 2) - 1) and (q == M.ONE).all()
        assert M.plane_sum(a, a) == M.windows(w, h) * 2 ** 30
        assert M.ssim(M.plane_sum(a, a), w, h) == 1.0 and M.ssim_db(1.0) == math.inf


def test_inverted_planes_give_a_negative_sum():
    a, b = _contents(72, 40)["inverted"]
    assert M.plane_sum(a, b) < 0
    assert (M.window_q(a, b) >= -M.ONE).all()


def test_constant_0_against_255_is_1677_per_window():
    a, b = _contents(24, 16)["constant"]
    q = M.window_q(a, b)
    # A1 = 416, B1 = (64 * 255)^2 + 416, A2 = B2 = 235963: 416 / 266 342 816 * 2^30 = 1677.07...
    assert (q == 1677).all() and M.plane_sum(a, b) == 1677 * M.windows(24, 16)


@pytest.mark.parametrize("w,h", [(16, 16), (72, 40), (264, 36)])
def test_terms_fit_in_int32(w, h):
    lim = 2 ** 31
    for name, (a, b) in _contents(w, h).items():
        A1, A2, B1, B2, vars_ = M.window_terms(a, b)
        assert (vars_ >= 0).all(), name
        for t in (A1, A2, B1, B2):
            assert (np.abs(t) < lim).all(), name
        assert np.abs(A1).max() <= 532685216 and B1.max() <= 532685216, name
        assert np.abs(A2).max() <= 532920763 and B2.max() <= 532920763, name
        assert (np.abs(M.window_q(a, b)) <= M.ONE).all(), name
    # the first pair's bound is reached by every pixel 255 in both frames; the second pair's is 64 * max(ss) + C2,
    # above anything content can give (half the pixels 255 in both frames: 2 * 66 585 600 + C2)
    full = np.full((8, 8), 255, np.uint8)
    A1, A2, B1, B2, _ = M.window_terms(full, full)
    assert A1.max() == B1.max() == 532685216
    half = np.zeros((8, 8), np.uint8)
    half[:, ::2] = 255
    _, A2, _, B2, _ = M.window_terms(half, half)
    assert A2.max() == B2.max() == 2 * 66585600 + M.C2 <= 532920763


def _float_ssim(a, b):
    """SSIM of every window from its 64 pixels in float64: means, (population) variances and covariance
    taken from the pixels themselves, no block sums.  The constants are the contract's on the scale of
    one pixel: C1 / 64^2 and C2 / 64^2."""
    h, w = a.shape
    c1, c2 = M.C1 / 4096.0, M.C2 / 4096.0
    out = np.empty(((h >> 2) - 1, (w >> 2) - 1))
    for j in range(out.shape[0]):
        for i in range(out.shape[1]):
            x = a[4 * j:4 * j + 8, 4 * i:4 * i + 8].astype(np.float64).ravel()
            y = b[4 * j:4 * j + 8, 4 * i:4 * i + 8].astype(np.float64).ravel()
            mx, my = x.mean(), y.mean()
            vx, vy = ((x - mx) ** 2).mean(), ((y - my) ** 2).mean()
            cov = ((x - mx) * (y - my)).mean()
            out[j, i] = (2 * mx * my + c1) * (2 * cov + c2) / ((mx * mx + my * my + c1) * (vx + vy + c2))
    return out


def test_model_agrees_with_a_float_restatement():
    """Within 2^-30 per window.  Derived, not measured: rint contributes at most 2^-31, and the model's three
    correctly rounded double operations on exact integers, like the restatement's few dozen on values of
    magnitude <= 1 after the divide, contribute far less than the other 2^-31."""
    for name, (a, b) in _contents(42, 30, seed=11).items():
        got = M.window_q(a, b) / float(M.ONE)
        err = np.abs(got - _float_ssim(a, b)).max()
        assert err <= 2.0 ** -30, (name, err)


SIZES = [(7, 7), (7, 64), (8, 8), (8, 7), (11, 11), (12, 12), (12, 11), (16, 16), (18, 22), (3840, 2160), (8192, 8192)]


def test_host_finish_against_python():
    lib = L.load()
    assert L.THOR_SSIM_ONE == M.ONE
    for w, h in SIZES:
        n = M.windows(w, h)
        assert lib.thor_ssim_windows(w, h) == n, (w, h)
        assert n == (0 if min(w, h) < 8 else ((w >> 2) - 1) * ((h >> 2) - 1))
        if not n:
            assert math.isnan(lib.thor_ssim(5, w, h))
            continue
        for total in (n * M.ONE, 0, -n * M.ONE // 3, n * M.ONE - 1, 1677 * n, 123456789):
            assert lib.thor_ssim(total, w, h) == M.ssim(total, w, h), (w, h, total)
        assert lib.thor_ssim(n * M.ONE, w, h) == 1.0
    assert lib.thor_ssim_windows(8, 8) == 1 and lib.thor_ssim_windows(16, 16) == 9
    assert lib.thor_ssim_windows(8192, 8192) == 2047 * 2047
    for s in (1.0, 0.0, 0.5, 0.987654321, -0.25, 1 - 2.0 ** -30):
        assert lib.thor_ssim_db(s) == M.ssim_db(s), s
    assert lib.thor_ssim_db(1.0) == math.inf and lib.thor_ssim_db(0.0) == 0.0 and lib.thor_ssim_db(0.9) == pytest.approx(10.0)


def test_symbols_and_argument_errors():
    lib = L.load()
    names = ("thor_ssim_windows", "thor_ssim_i420", "thor_ssim", "thor_ssim_db", "thor_dec_frame_ssim",
             "thor_enc_recon_ssim")
    for name in names:
        assert name in L.BATCHED_SYMBOLS and getattr(lib, name).argtypes is not None, name
    assert lib.thor_ssim.restype is C.c_double and lib.thor_ssim_db.restype is C.c_double
    # every argument error is found before any device call (no GPU needed): the pointers are never followed
    one = (L.ThorYuvPlanes * 1)(L.ThorYuvPlanes(16, 32, 48, 16, 8))
    sums = C.c_void_p(64)
    E = L.THOR_ERR_ARG
    assert lib.thor_ssim_i420(None, one, 1, 16, 16, sums, None) == E
    assert lib.thor_ssim_i420(one, None, 1, 16, 16, sums, None) == E
    assert lib.thor_ssim_i420(one, one, 1, 16, 16, None, None) == E
    assert lib.thor_ssim_i420(one, one, 0, 16, 16, sums, None) == E
    assert lib.thor_ssim_i420(one, one, -1, 16, 16, sums, None) == E
    assert lib.thor_ssim_i420(one, one, 65536, 16, 16, sums, None) == E
    assert lib.thor_ssim_i420(one, one, 1, 15, 16, sums, None) == E
    assert lib.thor_ssim_i420(one, one, 1, 16, 15, sums, None) == E
    for hole in range(3):  # a plane set with a null plane
        p = [16, 32, 48]
        p[hole] = None
        bad = (L.ThorYuvPlanes * 1)(L.ThorYuvPlanes(p[0], p[1], p[2], 16, 8))
        assert lib.thor_ssim_i420(bad, one, 1, 16, 16, sums, None) == E
        assert lib.thor_ssim_i420(one, bad, 1, 16, 16, sums, None) == E
    assert lib.thor_dec_frame_ssim(None, 0, one, sums) == E
    assert lib.thor_dec_frame_ssim(None, 0, None, None) == E
    assert lib.thor_enc_recon_ssim(None, one, sums) == E
    assert lib.thor_enc_recon_ssim(None, None, None) == E
