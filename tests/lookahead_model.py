"""The lookahead contract of DESIGN.md sec. 7f in numpy: the oracle of k_lookahead
(thor_amd/csrc/lookahead.hip).  Integers only; nothing here shares code with the
library.

Only luma is read.  A w x h plane has a (w >> 1) x (h >> 1) lowres plane (2x2
box, one rounding; the last odd column and row are not read), and that has
bw x bh = (lw >> 3) x (lh >> 3) blocks of 8x8 lowres pixels.  Per block: the
least SATD over the intra predictors available (DC, V, H from the source's own
lowres neighbours), and the SATD at the winner of an integer full search of
+-8 lowres pixels on the reference's lowres plane (coordinates clamped)."""
import numpy as np

RANGE = 8                      # the search is [-RANGE, RANGE]^2
NCAND = (2 * RANGE + 1) ** 2   # 289
NO_SAD = 0xFFFF                # `sad` of an intra-only pair
BLOCK = np.dtype([("intra", "<u2"), ("inter", "<u2"), ("sad", "<u2"), ("mvx", "i1"), ("mvy", "i1")])
assert BLOCK.itemsize == 8

_H2 = np.array([[1, 1], [1, -1]], np.int64)
HADAMARD = np.kron(np.kron(_H2, _H2), _H2)  # 8x8, Sylvester order


def blocks(w: int, h: int):
    """(bw, bh)."""
    return (w >> 1) >> 3, (h >> 1) >> 3


def lowres(p: np.ndarray) -> np.ndarray:
    h, w = p.shape
    lh, lw = h >> 1, w >> 1
    q = p[:2 * lh, :2 * lw].astype(np.int64)
    return ((q[0::2, 0::2] + q[0::2, 1::2] + q[1::2, 0::2] + q[1::2, 1::2] + 2) >> 2).astype(np.int64)


def satd(d: np.ndarray) -> np.ndarray:
    """(sum |H d H^T| + 2) >> 2 over the last two axes (8, 8) of an integer array."""
    t = HADAMARD @ d.astype(np.int64) @ HADAMARD.T
    return (np.abs(t).sum(axis=(-1, -2)) + 2) >> 2


def _tiles(l: np.ndarray, bw: int, bh: int) -> np.ndarray:
    """(bh, bw, 8, 8): the blocks of the first 8 bh rows and 8 bw columns of `l`."""
    return l[:8 * bh, :8 * bw].reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3)


def intra_costs(lc: np.ndarray, bw: int, bh: int) -> np.ndarray:
    """(bh, bw) int64: min SATD over DC, V (not in the first block row), H (not in the first block column)."""
    cur = _tiles(lc, bw, bh)
    out = np.empty((bh, bw), np.int64)
    for by in range(bh):
        for bx in range(bw):
            c = cur[by, bx]
            top = lc[8 * by - 1, 8 * bx:8 * bx + 8] if by else None
            left = lc[8 * by:8 * by + 8, 8 * bx - 1] if bx else None
            if top is not None and left is not None:
                dc = (int(top.sum()) + int(left.sum()) + 8) >> 4
            elif top is not None:
                dc = (int(top.sum()) + 4) >> 3
            elif left is not None:
                dc = (int(left.sum()) + 4) >> 3
            else:
                dc = 128
            best = int(satd(c - dc))
            if top is not None:
                best = min(best, int(satd(c - top[None, :])))
            if left is not None:
                best = min(best, int(satd(c - left[:, None])))
            out[by, bx] = best
    return out


def search(lc: np.ndarray, lr: np.ndarray, bw: int, bh: int):
    """(key, pred): the least key of every block, (bh, bw) int64, and the reference block at its vector,
    (bh, bw, 8, 8).  key = sad << 14 | (|dx| + |dy|) << 9 | ((dy + 8) * 17 + (dx + 8))."""
    lh, lw = lr.shape
    cur = _tiles(lc, bw, bh)
    ys, xs = np.arange(8 * bh), np.arange(8 * bw)
    best = np.full((bh, bw), 1 << 62, np.int64)
    pred = np.zeros((bh, bw, 8, 8), np.int64)
    for dy in range(-RANGE, RANGE + 1):
        rows = lr[np.clip(ys + dy, 0, lh - 1)]
        for dx in range(-RANGE, RANGE + 1):
            cand = _tiles(rows[:, np.clip(xs + dx, 0, lw - 1)], bw, bh)
            sad = np.abs(cur - cand).sum(axis=(2, 3))
            key = (sad << 14) | ((abs(dx) + abs(dy)) << 9) | ((dy + RANGE) * 17 + (dx + RANGE))
            win = key < best
            best = np.where(win, key, best)
            pred = np.where(win[:, :, None, None], cand, pred)
    return best, pred


def frame(cur: np.ndarray, ref):
    """(records, sums) of one luma pair: records a BLOCK array (bh, bw), sums four Python ints
    [sum intra, sum inter, sum min(intra, inter), blocks with intra < inter].  ref None: intra-only."""
    h, w = cur.shape
    bw, bh = blocks(w, h)
    lc = lowres(cur)
    rec = np.zeros((bh, bw), BLOCK)
    intra = intra_costs(lc, bw, bh)
    if ref is None:
        inter, sad = intra.copy(), np.full((bh, bw), NO_SAD, np.int64)
        mvx = mvy = np.zeros((bh, bw), np.int64)
    else:
        assert ref.shape == (h, w)
        key, pred = search(lc, lowres(ref), bw, bh)
        inter = satd(_tiles(lc, bw, bh) - pred)
        sad, idx = key >> 14, key & 511
        mvy, mvx = idx // 17 - RANGE, idx % 17 - RANGE
    assert intra.max(initial=0) <= 32640 and inter.max(initial=0) <= 32640
    rec["intra"], rec["inter"], rec["sad"], rec["mvx"], rec["mvy"] = intra, inter, sad, mvx, mvy
    sums = [int(intra.sum()), int(inter.sum()), int(np.minimum(intra, inter).sum()), int((intra < inter).sum())]
    return rec, sums


def scenecut(sums, percent: int) -> bool:
    return sums[0] > 0 and 100 * sums[2] >= percent * sums[0]


def sequence(frames):
    """[(records, sums)] of luma frames in display order: frame k against frame k - 1, frame 0 intra-only."""
    return [frame(f, frames[k - 1] if k else None) for k, f in enumerate(frames)]
