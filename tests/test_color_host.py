"""Colour conversion, host side (no device): the coefficient tables the library
exports, the integer contract's properties over all 2^24 colours (the numpy
model, tests/color_model.py), the float rule, and every argument rejection of
thor_i420_to_rgb / thor_rgb_to_i420, which happens before any device call."""
import ctypes as C

import numpy as np
import pytest

import color_model as M
from thor_amd import lib as L

FWD = {
    (0, 0): [4207, 8260, 1604, -2428, -4768, 7196, 7196, -6026, -1170],
    (0, 1): [4899, 9617, 1868, -2765, -5427, 8192, 8192, -6860, -1332],
    (1, 0): [2991, 10064, 1016, -1649, -5547, 7196, 7196, -6536, -660],
    (1, 1): [3483, 11718, 1183, -1877, -6315, 8192, 8192, -7441, -751],
}
INV = {
    (0, 0): [19077, 0, 26149, 19077, -6419, -13320, 19077, 33050, 0],
    (0, 1): [16384, 0, 22970, 16384, -5638, -11700, 16384, 29032, 0],
    (1, 0): [19077, 0, 29372, 19077, -3494, -8731, 19077, 34610, 0],
    (1, 1): [16384, 0, 25802, 16384, -3069, -7670, 16384, 30402, 0],
}
PAIRS = [(0, 0), (0, 1), (1, 0), (1, 1)]


@pytest.mark.parametrize("matrix,full", PAIRS)
def test_coefficient_tables(matrix, full):
    lib = L.load()
    f, i = (C.c_int32 * 9)(), (C.c_int32 * 9)()
    assert lib.thor_csc_coeffs(matrix, full, f, i) == 0
    assert list(f) == FWD[(matrix, full)] and list(i) == INV[(matrix, full)]
    assert sum(f[0:3]) == (16384 if full else 14071)
    assert sum(f[3:6]) == 0 and sum(f[6:9]) == 0
    # either output may be left out
    assert lib.thor_csc_coeffs(matrix, full, None, i) == 0 and lib.thor_csc_coeffs(matrix, full, f, None) == 0
    # the model and the Python wrapper hold the same tables
    assert np.array(M.FWD[(matrix, full)]).reshape(-1).tolist() == list(f)
    assert np.array(M.INV[(matrix, full)]).reshape(-1).tolist() == list(i)
    from thor_amd import color

    fw, iv = color.coeffs(matrix, bool(full))
    assert sum(fw, []) == list(f) and sum(iv, []) == list(i)


def test_coefficients_reject_bad_enums():
    lib = L.load()
    f, i = (C.c_int32 * 9)(), (C.c_int32 * 9)()
    for m, r in ((2, 0), (-1, 0), (0, 2), (0, -1)):
        assert lib.thor_csc_coeffs(m, r, f, i) == L.THOR_ERR_ARG


@pytest.mark.parametrize("matrix,full", PAIRS)
def test_model_over_all_colours(matrix, full):
    """Grey gives Cb = Cr = 128, black / white hit the range ends, and RGB ->
    YCbCr -> RGB (flat 2x2 blocks, nearest chroma) is within 2 (limited) / 1
    (full range) in every channel, for every one of the 2^24 colours."""
    g = np.arange(256)
    cb, cr = M.chroma(4 * g, 4 * g, 4 * g, matrix, full)
    assert (cb == 128).all() and (cr == 128).all()
    y = M.luma(g, g, g, matrix, full)
    assert (y[0], y[255]) == ((0, 255) if full else (16, 235))
    bound = 1 if full else 2
    gg, bb = np.meshgrid(g, g, indexing="ij")
    gg, bb = gg.reshape(-1), bb.reshape(-1)
    worst = 0
    for r0 in range(0, 256, 16):
        r = np.repeat(np.arange(r0, r0 + 16), gg.size)
        gq, bq = np.tile(gg, 16), np.tile(bb, 16)
        yv = M.luma(r, gq, bq, matrix, full)
        cb, cr = M.chroma(4 * r, 4 * gq, 4 * bq, matrix, full)
        back = M.yuv_to_rgb16(yv, 16 * cb, 16 * cr, matrix, full)
        worst = max(worst, int(np.abs(back - np.stack([r, gq, bq], axis=-1)).max()))
    assert worst <= bound, worst


def test_float_rule():
    q = np.arange(256)
    f = M.byte_to_float(q)
    assert f.dtype == np.float32 and f[255] == np.float32(1.0) and f[0] == 0
    assert np.array_equal(M.float_to_byte(f), q)
    sp = np.array([np.nan, np.inf, -np.inf, -0.0, -0.25, 1.25, 0.5 / 255, 1.5 / 255, 2.5 / 255, 1e-45], np.float32)
    assert M.float_to_byte(sp).tolist() == [0, 255, 0, 0, 0, 255, 0, 2, 2, 0]


def _args(W=16, H=8, fmt=L.THOR_RGB8_PACKED):
    row = {L.THOR_RGB8_PACKED: 3 * W, L.THOR_RGB8_PLANAR: W, L.THOR_RGBF32_PLANAR: 4 * W}[fmt]
    yuv = L.ThorYuvPlanes(0x1000, 0x2000, 0x3000, W, W // 2)  # dummy non-null pointers: never dereferenced
    img = L.ThorImage(0x4000, fmt, row, row * H)
    return yuv, img, L.ThorCsc(1, 0, 1)


def _both(lib, yuv, img, n, W, H, csc):
    y = C.byref(yuv) if yuv is not None else None
    i = C.byref(img) if img is not None else None
    c = C.byref(csc) if csc is not None else None
    return lib.thor_i420_to_rgb(y, i, n, W, H, c, None), lib.thor_rgb_to_i420(i, y, n, W, H, c, None)


def test_argument_rejection_without_a_device():
    lib = L.load()
    E = (L.THOR_ERR_ARG, L.THOR_ERR_ARG)
    yuv, img, csc = _args()
    # null descriptor arrays / csc
    assert _both(lib, None, img, 1, 16, 8, csc) == E
    assert _both(lib, yuv, None, 1, 16, 8, csc) == E
    assert _both(lib, yuv, img, 1, 16, 8, None) == E
    # batch size
    for n in (0, -1, 65536):
        assert _both(lib, yuv, img, n, 16, 8, csc) == E
    # odd or empty sizes
    for W, H in ((15, 8), (16, 7), (0, 8), (16, 0), (1, 2), (2, 1), (-16, 8)):
        assert _both(lib, yuv, img, 1, W, H, csc) == E
    # enums
    for m, r in ((2, 0), (-1, 0), (0, 2), (0, -1)):
        assert _both(lib, yuv, img, 1, 16, 8, L.ThorCsc(m, r, 0)) == E
    for up in (2, -1):
        assert lib.thor_i420_to_rgb(C.byref(yuv), C.byref(img), 1, 16, 8, C.byref(L.ThorCsc(0, 0, up)), None) == \
            L.THOR_ERR_ARG
    for fmt in (3, -1):
        assert _both(lib, yuv, L.ThorImage(0x4000, fmt, 4096, 65536), 1, 16, 8, csc) == E
    # null planes / data
    for k in ("y", "u", "v"):
        y2, _, _ = _args()
        setattr(y2, k, None)
        assert _both(lib, y2, img, 1, 16, 8, csc) == E
    assert _both(lib, yuv, L.ThorImage(None, 0, 48, 0), 1, 16, 8, csc) == E
    # strides below a row
    assert _both(lib, L.ThorYuvPlanes(0x1000, 0x2000, 0x3000, 15, 8), img, 1, 16, 8, csc) == E
    assert _both(lib, L.ThorYuvPlanes(0x1000, 0x2000, 0x3000, 16, 7), img, 1, 16, 8, csc) == E
    for fmt in (L.THOR_RGB8_PACKED, L.THOR_RGB8_PLANAR, L.THOR_RGBF32_PLANAR):
        _, im, _ = _args(fmt=fmt)
        im.stride -= 1 if fmt != L.THOR_RGBF32_PLANAR else 4
        assert _both(lib, yuv, im, 1, 16, 8, csc) == E
    # float: strides and pointers that are no multiple of 4
    for field, delta in (("stride", 2), ("plane_stride", 2), ("data", 2), ("data", 1)):
        _, im, _ = _args(fmt=L.THOR_RGBF32_PLANAR)
        setattr(im, field, getattr(im, field) + delta)
        assert _both(lib, yuv, im, 1, 16, 8, csc) == E
    # all images of a call share the format; every descriptor is checked, not only the first
    imgs = (L.ThorImage * 2)(_args()[1], _args(fmt=L.THOR_RGB8_PLANAR)[1])
    yuvs = (L.ThorYuvPlanes * 2)(yuv, yuv)
    assert lib.thor_i420_to_rgb(yuvs, imgs, 2, 16, 8, C.byref(csc), None) == L.THOR_ERR_ARG
    assert lib.thor_rgb_to_i420(imgs, yuvs, 2, 16, 8, C.byref(csc), None) == L.THOR_ERR_ARG
    yuvs[1].u = None
    imgs[1] = imgs[0]
    assert lib.thor_i420_to_rgb(yuvs, imgs, 2, 16, 8, C.byref(csc), None) == L.THOR_ERR_ARG
    # decoder entry points: null context
    assert lib.thor_dec_frame_planes(None, 0, C.byref(yuv)) == L.THOR_ERR_ARG
    assert lib.thor_dec_frame_rgb(None, 0, C.byref(img), C.byref(csc)) == L.THOR_ERR_ARG


def test_python_surface_imports_without_torch_at_module_level():
    """thor_amd.color imports torch inside its functions only."""
    import ast
    import os

    import thor_amd.color as color

    tree = ast.parse(open(os.path.splitext(color.__file__)[0] + ".py").read())
    top = [n for n in tree.body if isinstance(n, (ast.Import, ast.ImportFrom))]
    names = {a.name.split(".")[0] for n in top if isinstance(n, ast.Import) for a in n.names}
    names |= {(n.module or "").split(".")[0] for n in top if isinstance(n, ast.ImportFrom)}
    assert "torch" not in names
    assert color.csc("bt601", True, "nearest").matrix == 0
    with pytest.raises(ValueError):
        color.csc("bt2020")
