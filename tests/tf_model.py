"""The temporal-filter contract of DESIGN.md sec. 7g in numpy: the oracle of
k_tf_luma / k_tf_chroma (thor_amd/csrc/tf.hip).  Integers only; the coarse
stage is lookahead_model's, and nothing here shares code with the library.

A target frame and up to four references of the same size (8-bit I420, both
sizes multiples of 8).  Per reference and 8x8 luma block a half-pel vector
(lookahead start, +-2 integer refinement, +-1 half-pel refinement) and the
block's error; per pixel of every plane a weighted mean of the target and the
motion-compensated references, the weight falling with the pixel's and the
block's squared error."""
import numpy as np

import lookahead_model as LA

IR = 2  # the integer refinement is [-IR, IR]^2 around the start
LUT = [256, 240, 226, 212, 199, 187, 176, 165, 155, 146, 137, 129, 121, 114, 107, 100, 94, 88, 83, 78, 73, 69, 65, 61,
       57, 54, 50, 47, 44, 42, 39, 37, 35, 33, 31, 29, 27, 25, 24, 22, 21, 20, 19, 17, 16, 15, 14, 14, 13, 12, 11, 11,
       10, 9, 9, 8, 8, 7, 7, 6, 6, 6, 5, 0]
assert len(LUT) == 64
RECORD = np.dtype([("mvx", "i1"), ("mvy", "i1"), ("e", "<u2")])
assert RECORD.itemsize == 4


def mult(s: int) -> int:
    assert 1 <= s <= 64
    return ((16 << 16) + (s * s >> 1)) // (s * s)


def blocks(w: int, h: int):
    """(bw8, bh8): the 8x8 luma blocks of a w x h frame."""
    return w >> 3, h >> 3


def check(w: int, h: int, nrefs: int) -> bool:
    return w % 8 == 0 and h % 8 == 0 and 16 <= w <= 16384 and 16 <= h <= 16384 and 1 <= nrefs <= 4


def predict(ref: np.ndarray, y0, x0, n: int, mvy, mvx) -> np.ndarray:
    """(B, n, n) int64: the n x n blocks at (y0[b], x0[b]) predicted from `ref` at the half-pel vectors
    (mvy[b], mvx[b]); coordinates clamped to the plane."""
    H, W = ref.shape
    y0, x0, mvy, mvx = (np.asarray(v, np.int64).reshape(-1) for v in (y0, x0, mvy, mvx))
    r = np.arange(n)
    ya = np.clip((y0 + (mvy >> 1))[:, None] + r, 0, H - 1)
    yb = np.clip((y0 + (mvy >> 1))[:, None] + r + 1, 0, H - 1)
    xa = np.clip((x0 + (mvx >> 1))[:, None] + r, 0, W - 1)
    xb = np.clip((x0 + (mvx >> 1))[:, None] + r + 1, 0, W - 1)
    R = ref.astype(np.int64)
    a, b = R[ya[:, :, None], xa[:, None, :]], R[ya[:, :, None], xb[:, None, :]]
    c, d = R[yb[:, :, None], xa[:, None, :]], R[yb[:, :, None], xb[:, None, :]]
    fy, fx = (mvy & 1).astype(bool)[:, None, None], (mvx & 1).astype(bool)[:, None, None]
    return np.where(fx & fy, (a + b + c + d + 2) >> 2, np.where(fx, (a + b + 1) >> 1, np.where(fy, (a + c + 1) >> 1, a)))


def _grid(w: int, h: int, n: int):
    """y0, x0 (flat, raster order) of the n x n blocks of a w x h plane."""
    ys, xs = np.meshgrid(np.arange(h // n) * n, np.arange(w // n) * n, indexing="ij")
    return ys.reshape(-1), xs.reshape(-1)


def _tiles(p: np.ndarray, n: int) -> np.ndarray:
    h, w = p.shape
    return p.astype(np.int64).reshape(h // n, n, w // n, n).transpose(0, 2, 1, 3).reshape(-1, n, n)


def start_vectors(T: np.ndarray, R: np.ndarray):
    """(sy, sx) flat over the 8x8 blocks, in source pixels: twice the lookahead's vector of the 16x16 block, (0, 0)
    outside the lookahead's grid."""
    h, w = T.shape
    rec, _ = LA.frame(T, R)
    lbh, lbw = rec.shape
    bw8, bh8 = blocks(w, h)
    by, bx = np.meshgrid(np.arange(bh8) >> 1, np.arange(bw8) >> 1, indexing="ij")
    ins = (by < lbh) & (bx < lbw)
    byc, bxc = np.minimum(by, lbh - 1), np.minimum(bx, lbw - 1)
    sy = np.where(ins, 2 * rec["mvy"].astype(np.int64)[byc, bxc], 0)
    sx = np.where(ins, 2 * rec["mvx"].astype(np.int64)[byc, bxc], 0)
    return sy.reshape(-1), sx.reshape(-1)


def motion(T: np.ndarray, R: np.ndarray, zero: bool = False):
    """Records (bh8, bw8) of luma target T against luma reference R.  zero: every vector forced to (0, 0)."""
    h, w = T.shape
    bw8, bh8 = blocks(w, h)
    y0, x0 = _grid(w, h, 8)
    cur = _tiles(T, 8)
    rec = np.zeros((bh8, bw8), RECORD)
    if zero:
        mvy = mvx = np.zeros(len(y0), np.int64)
    else:
        sy, sx = start_vectors(T, R)
        best = np.full(len(y0), 1 << 62, np.int64)
        for dy in range(-IR, IR + 1):
            for dx in range(-IR, IR + 1):
                sad = np.abs(cur - predict(R, y0, x0, 8, 2 * (sy + dy), 2 * (sx + dx))).sum(axis=(1, 2))
                assert sad.max() < (1 << 14)
                best = np.minimum(best, (sad << 10) | ((abs(dx) + abs(dy)) << 5) | ((dy + IR) * 5 + dx + IR))
        idx = best & 31
        iy, ix = sy + idx // 5 - IR, sx + idx % 5 - IR
        best = np.full(len(y0), 1 << 62, np.int64)
        for hy in (-1, 0, 1):
            for hx in (-1, 0, 1):
                sad = np.abs(cur - predict(R, y0, x0, 8, 2 * iy + hy, 2 * ix + hx)).sum(axis=(1, 2))
                best = np.minimum(best, (sad << 6) | ((abs(hx) + abs(hy)) << 4) | ((hy + 1) * 3 + hx + 1))
        idx = best & 15
        mvy, mvx = 2 * iy + idx // 3 - 1, 2 * ix + idx % 3 - 1
        assert np.abs(mvy).max() <= 37 and np.abs(mvx).max() <= 37
    d = cur - predict(R, y0, x0, 8, mvy, mvx)
    rec["mvy"], rec["mvx"] = mvy.reshape(bh8, bw8), mvx.reshape(bh8, bw8)
    rec["e"] = ((d * d).sum(axis=(1, 2)) >> 6).reshape(bh8, bw8)
    return rec


def _untile(b: np.ndarray, w: int, h: int, n: int) -> np.ndarray:
    return b.reshape(h // n, w // n, n, n).transpose(0, 2, 1, 3).reshape(h, w)


def blend(Tp: np.ndarray, Rps, recs, strength: int, chroma: bool) -> np.ndarray:
    """One plane: Tp the target's, Rps the references' (None: absent), recs their luma records."""
    h, w = Tp.shape
    n = 4 if chroma else 8
    y0, x0 = _grid(w, h, n)
    T = Tp.astype(np.int64)
    num, den = 256 * T, np.full((h, w), 256, np.int64)
    lut, mu = np.array(LUT, np.int64), mult(strength)
    for Rp, rec in zip(Rps, recs):
        if Rp is None:
            continue
        mvy, mvx = rec["mvy"].astype(np.int64).reshape(-1), rec["mvx"].astype(np.int64).reshape(-1)
        if chroma:
            mvy, mvx = mvy >> 1, mvx >> 1
        pb = predict(Rp, y0, x0, n, mvy, mvx)
        P = _untile(pb, w, h, n)
        d = T - P
        e = (_tiles(d, n) ** 2).sum(axis=(1, 2)) >> (4 if chroma else 6)
        if not chroma:
            assert (e == rec["e"].reshape(-1)).all()
        m = (d * d + _untile(np.repeat(e, n * n).reshape(-1, n, n), w, h, n)) >> 1
        wgt = lut[np.minimum(63, (np.minimum(m, 2047) * mu) >> 16)]
        num += wgt * P
        den += wgt
    assert num.max() <= 326400 and den.max() <= 1280
    return ((num + (den >> 1)) // den).astype(np.uint8)


def frame(T, refs, strength=(8, 3), zero: bool = False):
    """(out, records): T and refs are (y, u, v) plane triples (a reference may be None: absent); out the filtered
    triple, records a RECORD array (len(refs), bh8, bw8), zero for an absent reference."""
    h, w = T[0].shape
    assert check(w, h, len(refs))
    bw8, bh8 = blocks(w, h)
    recs = np.zeros((len(refs), bh8, bw8), RECORD)
    for r, R in enumerate(refs):
        if R is not None:
            recs[r] = motion(T[0], R[0], zero)
    out = tuple(blend(T[c], [None if R is None else R[c] for R in refs], recs, strength[1 if c else 0], c > 0)
                for c in range(3))
    return out, recs


def split(frame_bytes: np.ndarray, w: int, h: int):
    """(y, u, v) views of one contiguous I420 frame."""
    f = np.asarray(frame_bytes, np.uint8).reshape(-1)
    y, c = w * h, (w // 2) * (h // 2)
    return f[:y].reshape(h, w), f[y:y + c].reshape(h // 2, w // 2), f[y + c:y + 2 * c].reshape(h // 2, w // 2)


def join(planes) -> np.ndarray:
    return np.concatenate([p.reshape(-1) for p in planes]).astype(np.uint8)


def sequence(frames, w: int, h: int, radius: int = 2, strength=(8, 3)):
    """Frame k of `frames` (n, w*h*3/2) filtered from the unfiltered frames k - radius .. k + radius that exist
    (nearest last is not implied: the order is k - radius, .., k - 1, k + 1, .., k + radius)."""
    n = len(frames)
    out = np.empty((n, w * h * 3 // 2), np.uint8)
    for k in range(n):
        refs = [split(frames[j], w, h) if 0 <= j < n else None
                for j in list(range(k - radius, k)) + list(range(k + 1, k + radius + 1))]
        out[k] = join(frame(split(frames[k], w, h), refs, strength)[0])
    return out
