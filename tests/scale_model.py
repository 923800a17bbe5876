"""The frame scaler's contract in Python ints and numpy: the
specification the host tables (thor_scale_taps) and the kernel (scale.hip) are
tested against.  Not a test."""
import functools

import numpy as np

BILINEAR, BICUBIC = 0, 1
MAX_TAPS = 33
UNIT = 16384


def weight(u, M, f):
    """Exact numerator of the filter at distance u / M (u >= 0, inside the support)."""
    if f == BILINEAR:
        return M - u
    if u < M:
        return 3 * u ** 3 - 5 * M * u ** 2 + 2 * M ** 3
    return -u ** 3 + 5 * M * u ** 2 - 8 * M * M * u + 4 * M ** 3


@functools.lru_cache(maxsize=None)
def taps(S, D, f):
    """(first, coef, ntaps): first[d] = the first source sample of output d (not
    clamped), coef an int64 array (D, ntaps) whose rows sum to 16384, zero-padded."""
    R = 1 if f == BILINEAR else 2
    M = 2 * max(S, D)
    first, rows = [], []
    for d in range(D):
        c2 = (2 * d + 1) * S - D
        s0 = (c2 - R * M) // (2 * D) + 1
        s1 = -((-(c2 + R * M)) // (2 * D)) - 1
        P = [weight(abs(2 * D * s - c2), M, f) for s in range(s0, s1 + 1)]
        T = sum(P)
        c = [(2 * p * UNIT + T) // (2 * T) for p in P]
        c[P.index(max(P))] += UNIT - sum(c)
        first.append(s0)
        rows.append(c)
    n = max(len(r) for r in rows)
    coef = np.zeros((D, n), np.int64)
    for d, r in enumerate(rows):
        coef[d, :len(r)] = r
    return np.array(first, np.int64), coef, n


def _gather(S, D, f):
    first, coef, n = taps(S, D, f)
    idx = np.clip(first[:, None] + np.arange(n)[None, :], 0, S - 1)
    return idx, coef


def scale_plane(a, dw, dh, f):
    """a: (sh, sw) uint8 -> (dh, dw) uint8: horizontal pass into 6 fractional bits, then vertical."""
    a = np.asarray(a).astype(np.int64)
    sh, sw = a.shape
    ix, cx = _gather(sw, dw, f)
    h = ((a[:, ix] * cx[None]).sum(axis=2) + 128) >> 8  # (sh, dw)
    assert np.abs(h).max() <= 32767
    iy, cy = _gather(sh, dh, f)
    v = (h[iy] * cy[:, :, None]).sum(axis=1)  # (dh, dw)
    assert np.abs(v).max() < 2 ** 31
    return np.clip((v + (1 << 19)) >> 20, 0, 255).astype(np.uint8)


def scale_i420(y, u, v, dw, dh, f):
    """Three planes: Y to (dh, dw), U and V to the halved sizes, same formulas."""
    return [scale_plane(y, dw, dh, f), scale_plane(u, dw // 2, dh // 2, f), scale_plane(v, dw // 2, dh // 2, f)]


def scale_frames(frames, sw, sh, dw, dh, f):
    """(n, sw*sh*3/2) uint8 contiguous I420 frames -> (n, dw*dh*3/2)."""
    frames = np.asarray(frames, np.uint8).reshape(-1, sw * sh * 3 // 2)
    out = np.empty((frames.shape[0], dw * dh * 3 // 2), np.uint8)
    for i, fr in enumerate(frames):
        y = fr[:sw * sh].reshape(sh, sw)
        u = fr[sw * sh:sw * sh * 5 // 4].reshape(sh // 2, sw // 2)
        v = fr[sw * sh * 5 // 4:].reshape(sh // 2, sw // 2)
        out[i] = np.concatenate([p.reshape(-1) for p in scale_i420(y, u, v, dw, dh, f)])
    return out
