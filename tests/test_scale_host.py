"""The frame scaler's host side without a GPU: thor_scale_taps against the
Python model of the contract (tests/scale_model.py), the properties of the
tables and of the model, and argument rejection before any device call."""
import ctypes as C

import numpy as np
import pytest

import scale_model as M
from thor_amd import lib as L

FILTERS = [L.THOR_SCALE_BILINEAR, L.THOR_SCALE_BICUBIC]
SMALL = [(S, D) for S in range(1, 25) for D in range(1, 25) if S <= 8 * D]
LADDER = [(3840, 1920), (3840, 1280), (3840, 640), (2160, 360), (1920, 3840), (8192, 1024), (1024, 8192), (1080, 1088)]


def host_taps(S, D, f):
    lib = L.load()
    n = C.c_int(0)
    assert lib.thor_scale_taps(S, D, f, None, None, C.byref(n)) == 0
    first = np.zeros(D, np.int32)
    coef = np.full((D, n.value), 0x5a5a, np.int16)
    n2 = C.c_int(0)
    assert lib.thor_scale_taps(S, D, f, first.ctypes.data_as(C.POINTER(C.c_int32)),
                               coef.ctypes.data_as(C.POINTER(C.c_int16)), C.byref(n2)) == 0
    assert n2.value == n.value
    return first, coef, n.value


def check_table(S, D, f):
    first, coef, n = host_taps(S, D, f)
    mf, mc, mn = M.taps(S, D, f)
    assert n == mn, (S, D, f)
    assert np.array_equal(first, mf), (S, D, f)
    assert np.array_equal(coef, mc), (S, D, f)
    R = 1 if f == L.THOR_SCALE_BILINEAR else 2
    c = coef.astype(np.int64)
    assert (c.sum(axis=1) == 16384).all(), (S, D, f)
    assert int(np.abs(c).sum(axis=1).max()) <= 21299, (S, D, f)
    assert n <= 2 * R * max(1, -(-S // D)) + 1 <= L.THOR_SCALE_MAX_TAPS, (S, D, f)
    assert (np.diff(first) >= 0).all(), (S, D, f)
    if S == D:  # a single tap: the identity
        assert ((c != 0).sum(axis=1) == 1).all()
        assert (c[np.arange(D), np.arange(D) - first] == 16384).all()


@pytest.mark.parametrize("f", FILTERS)
def test_small_tables_equal_the_model(f):
    for S, D in SMALL:
        check_table(S, D, f)


@pytest.mark.parametrize("f", FILTERS)
@pytest.mark.parametrize("S,D", LADDER)
def test_ladder_tables_equal_the_model(S, D, f):
    check_table(S, D, f)


def test_bilinear_two_to_one_taps():
    """2:1 triangle: four taps 1/8, 3/8, 3/8, 1/8 of 16384, symmetric around the output's centre."""
    first, coef, n = host_taps(16, 8, L.THOR_SCALE_BILINEAR)
    assert n == 4
    for d in range(8):
        assert first[d] == 2 * d - 1
        assert coef[d].tolist() == [2048, 6144, 6144, 2048]
    assert sorted(M.taps(16, 8, M.BILINEAR)[1][3].tolist()) == [2048, 2048, 6144, 6144]


@pytest.mark.parametrize("f", FILTERS)
def test_model_keeps_constant_planes(f):
    """All 256 values, shrinking on one axis and enlarging on the other: no drift through the two roundings."""
    for sw, sh, dw, dh in ((12, 6, 5, 14), (6, 16, 16, 2)):
        for v in range(256):
            out = M.scale_plane(np.full((sh, sw), v, np.uint8), dw, dh, f)
            assert out.shape == (dh, dw) and (out == v).all(), (sw, sh, dw, dh, v)


def test_model_identity():
    rng = np.random.default_rng(3)
    a = rng.integers(0, 256, (10, 14), dtype=np.uint8)
    for f in FILTERS:
        assert np.array_equal(M.scale_plane(a, 14, 10, f), a)


def test_size_and_filter_rejection():
    lib = L.load()
    ok = lib.thor_scale_check
    assert ok(3840, 2160, 640, 360, 1) == 0 and ok(2, 2, 8192, 8192, 0) == 0 and ok(16, 16, 2, 2, 1) == 0
    for bad in ((3, 2, 2, 2), (2, 5, 2, 2), (2, 2, 7, 2), (2, 2, 2, 9),  # odd
                (0, 2, 2, 2), (2, 0, 2, 2), (2, 2, 0, 2), (2, 2, 2, 0), (-2, 2, 2, 2), (1, 2, 2, 2),  # below 2
                (8194, 2, 8192, 2), (2, 8194, 2, 8192), (2, 2, 8194, 2), (2, 2, 2, 8194),  # above 8192
                (18, 2, 2, 2), (2, 18, 2, 2), (8192, 8192, 1022, 8192)):  # ratio above 8
        for f in FILTERS:
            assert ok(*bad, f) == L.THOR_ERR_ARG, bad
    for f in (-1, 2, 7):
        assert ok(16, 16, 8, 8, f) == L.THOR_ERR_ARG
    n = C.c_int(0)
    assert lib.thor_scale_taps(16, 8, 2, None, None, C.byref(n)) == L.THOR_ERR_ARG
    assert lib.thor_scale_taps(17, 2, 0, None, None, C.byref(n)) == L.THOR_ERR_ARG
    assert lib.thor_scale_taps(0, 2, 0, None, None, C.byref(n)) == L.THOR_ERR_ARG
    assert lib.thor_scale_taps(8, 8193, 0, None, None, C.byref(n)) == L.THOR_ERR_ARG
    assert lib.thor_scale_taps(8, 8, 0, None, None, None) == L.THOR_ERR_ARG
    # a scaler of refused sizes is refused by the size check, whatever the device
    assert not lib.thor_scaler_create(18, 2, 2, 2, 0, 0)
    assert L.create_error("thor_scaler_create").code == L.THOR_ERR_ARG
    assert not lib.thor_scaler_create(16, 16, 8, 8, 5, 0)
    assert L.create_error("thor_scaler_create").code == L.THOR_ERR_ARG


def test_scale_call_rejection_without_a_scaler():
    """thor_scale_i420 / thor_dec_frame_scaled return THOR_ERR_ARG before any device call: no scaler, no
    descriptors, n out of range.  (Strides and NULL planes against a live scaler: tests/test_gpu_scale.py.)"""
    lib = L.load()
    one = (L.ThorYuvPlanes * 1)(L.ThorYuvPlanes(256, 512, 768, 16, 8))
    assert lib.thor_scale_i420(None, one, one, 1, None) == L.THOR_ERR_ARG
    assert lib.thor_scale_i420(None, None, None, 1, None) == L.THOR_ERR_ARG
    for n in (0, -1, 65536):
        assert lib.thor_scale_i420(None, one, one, n, None) == L.THOR_ERR_ARG
    assert lib.thor_dec_frame_scaled(None, 0, None, one) == L.THOR_ERR_ARG


def test_python_surface_rejects_before_the_library():
    from thor_amd import scale

    assert scale.FILTERS == {"bilinear": 0, "bicubic": 1}
    with pytest.raises(ValueError):
        scale.Scaler(18, 2, 2, 2)
    with pytest.raises(ValueError):
        scale.Scaler(16, 16, 8, 8, filter="lanczos")
    assert scale.scaled_size_ok(3840, 2160, 1280, 720) and not scale.scaled_size_ok(3840, 2160, 1281, 720)
