"""The colour-conversion contract restated in plain numpy,
int64 / float32: the yardstick of tests/test_color_host.py and
tests/test_gpu_color.py.  Not a test.  Written from the contract, not from
thor_amd/csrc/color.hip.

Coefficients are 14-bit fixed point, row-major 3x3.  Forward rows give Y, Cb,
Cr from (R, G, B); inverse rows give R, G, B from (Y - yo, Cb - 128, Cr - 128);
yo = 16 for limited range, 0 for full range."""
import numpy as np

# (matrix, full_range) -> table; matrix 0 = BT.601, 1 = BT.709
FWD = {
    (0, 0): [[4207, 8260, 1604], [-2428, -4768, 7196], [7196, -6026, -1170]],
    (0, 1): [[4899, 9617, 1868], [-2765, -5427, 8192], [8192, -6860, -1332]],
    (1, 0): [[2991, 10064, 1016], [-1649, -5547, 7196], [7196, -6536, -660]],
    (1, 1): [[3483, 11718, 1183], [-1877, -6315, 8192], [8192, -7441, -751]],
}
INV = {
    (0, 0): [[19077, 0, 26149], [19077, -6419, -13320], [19077, 33050, 0]],
    (0, 1): [[16384, 0, 22970], [16384, -5638, -11700], [16384, 29032, 0]],
    (1, 0): [[19077, 0, 29372], [19077, -3494, -8731], [19077, 34610, 0]],
    (1, 1): [[16384, 0, 25802], [16384, -3069, -7670], [16384, 30402, 0]],
}
MATRICES = {"bt601": 0, "bt709": 1}
UNORM = np.float32(float.fromhex("0x1.010102p-8"))  # the float32 nearest 1/255


def _clamp(v):
    return np.clip(v, 0, 255)


def float_to_byte(v):
    """q = clamp(rint(v * 255.0f)): one float32 multiply, half to even, NaN -> 0."""
    with np.errstate(invalid="ignore", over="ignore"):
        x = np.rint(np.asarray(v, np.float32) * np.float32(255.0))
        x = np.where(np.isnan(x), np.float32(0), x)
        return np.clip(x, np.float32(0), np.float32(255)).astype(np.int64)


def byte_to_float(q):
    """(float)q * 0x1.010102p-8f: one float32 multiply."""
    return np.asarray(q).astype(np.float32) * UNORM


def luma(r, g, b, matrix, full_range):
    F = FWD[(matrix, full_range)]
    yo = 0 if full_range else 16
    r, g, b = (np.asarray(a, np.int64) for a in (r, g, b))
    return _clamp((F[0][0] * r + F[0][1] * g + F[0][2] * b + (yo << 14) + (1 << 13)) >> 14)


def chroma(rs, gs, bs, matrix, full_range):
    """(Cb, Cr) of 2x2 blocks from the sums of their four pixels' channels."""
    F = FWD[(matrix, full_range)]
    rs, gs, bs = (np.asarray(a, np.int64) for a in (rs, gs, bs))
    return tuple(_clamp((F[k][0] * rs + F[k][1] * gs + F[k][2] * bs + (128 << 16) + (1 << 15)) >> 16) for k in (1, 2))


def rgb_to_i420(rgb, matrix=1, full_range=0):
    """rgb: (H, W, 3) bytes (any integer dtype) or float32 -> (Y, U, V) uint8 planes."""
    rgb = np.asarray(rgb)
    q = float_to_byte(rgb) if rgb.dtype.kind == "f" else rgb.astype(np.int64)
    r, g, b = q[..., 0], q[..., 1], q[..., 2]
    y = luma(r, g, b, matrix, full_range)

    def box(p):
        return p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2]

    cb, cr = chroma(box(r), box(g), box(b), matrix, full_range)
    return y.astype(np.uint8), cb.astype(np.uint8), cr.astype(np.uint8)


def _chroma16(c, H, W, bilinear):
    c = np.asarray(c, np.int64)
    cyi = np.arange(H) >> 1
    cxi = np.arange(W) >> 1
    if not bilinear:
        return 16 * c[cyi][:, cxi]
    CH, CW = H // 2, W // 2
    nyi = np.clip(np.where(np.arange(H) % 2 == 0, cyi - 1, cyi + 1), 0, CH - 1)
    nxi = np.clip(np.where(np.arange(W) % 2 == 0, cxi - 1, cxi + 1), 0, CW - 1)
    return 9 * c[cyi][:, cxi] + 3 * c[cyi][:, nxi] + 3 * c[nyi][:, cxi] + c[nyi][:, nxi]


def yuv_to_rgb16(y, cb16, cr16, matrix, full_range):
    """out_k = clamp((Ik0 16 (Y - yo) + Ik1 (Cb16 - 2048) + Ik2 (Cr16 - 2048) + 2^17) >> 18), stacked last."""
    I = INV[(matrix, full_range)]
    yo = 0 if full_range else 16
    yp = 16 * (np.asarray(y, np.int64) - yo)
    up = np.asarray(cb16, np.int64) - 2048
    vp = np.asarray(cr16, np.int64) - 2048
    return np.stack([_clamp((I[k][0] * yp + I[k][1] * up + I[k][2] * vp + (1 << 17)) >> 18) for k in range(3)], axis=-1)


def i420_to_rgb(y, u, v, matrix=1, full_range=0, bilinear=True, as_float=False):
    """(H, W, 3): uint8, or float32 in [0, 1] with as_float."""
    H, W = np.asarray(y).shape
    out = yuv_to_rgb16(y, _chroma16(u, H, W, bilinear), _chroma16(v, H, W, bilinear), matrix, full_range)
    return byte_to_float(out) if as_float else out.astype(np.uint8)


def split_i420(buf, W, H):
    """Contiguous I420 bytes -> (Y, U, V) views."""
    buf = np.asarray(buf, np.uint8).reshape(-1)
    y = buf[:W * H].reshape(H, W)
    u = buf[W * H:W * H + (W // 2) * (H // 2)].reshape(H // 2, W // 2)
    v = buf[W * H + (W // 2) * (H // 2):W * H * 3 // 2].reshape(H // 2, W // 2)
    return y, u, v


def join_i420(y, u, v):
    return np.concatenate([np.asarray(p, np.uint8).reshape(-1) for p in (y, u, v)])
