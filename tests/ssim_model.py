"""The SSIM contract of DESIGN.md sec. 7e in numpy: the oracle of k_ssim_i420
(thor_amd/csrc/ssim.hip).  int64 sums, float64 for the two multiplies and the
divide, np.rint; nothing here shares code with the library.

A plane of w x h pixels has bw x bh = (w >> 2) x (h >> 2) 4x4 blocks (the last
w & 3 columns and h & 3 rows are not read) and (bw - 1) x (bh - 1) windows of
2x2 blocks."""
import numpy as np

C1, C2 = 416, 235963
ONE = 1 << 30


def windows(w: int, h: int) -> int:
    return ((w >> 2) - 1) * ((h >> 2) - 1) if w >= 8 and h >= 8 else 0


def window_sums(a: np.ndarray, b: np.ndarray):
    """(s1, s2, ss, s12) of every window, int64 arrays (bh - 1, bw - 1)."""
    h, w = a.shape
    assert b.shape == (h, w) and w >= 8 and h >= 8
    bw, bh = w >> 2, h >> 2
    a = a[:4 * bh, :4 * bw].astype(np.int64)
    b = b[:4 * bh, :4 * bw].astype(np.int64)

    def blocks(x):
        return x.reshape(bh, 4, bw, 4).sum(axis=(1, 3))

    def wins(x):
        return x[:-1, :-1] + x[:-1, 1:] + x[1:, :-1] + x[1:, 1:]

    return wins(blocks(a)), wins(blocks(b)), wins(blocks(a * a + b * b)), wins(blocks(a * b))


def window_terms(a: np.ndarray, b: np.ndarray):
    """(A1, A2, B1, B2, vars) of every window, int64."""
    s1, s2, ss, s12 = window_sums(a, b)
    vars_ = 64 * ss - s1 * s1 - s2 * s2
    covar = 64 * s12 - s1 * s2
    return 2 * s1 * s2 + C1, 2 * covar + C2, s1 * s1 + s2 * s2 + C1, vars_ + C2, vars_


def window_q(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """q = rint(A1 * A2 / (B1 * B2) * 2^30) of every window, int64."""
    A1, A2, B1, B2, _ = window_terms(a, b)
    f = np.float64
    return np.rint((A1.astype(f) * A2.astype(f)) / (B1.astype(f) * B2.astype(f)) * f(ONE)).astype(np.int64)


def plane_sum(a: np.ndarray, b: np.ndarray) -> int:
    return int(window_q(a, b).sum())


def frame_sums(fa, fb):
    """[Y, U, V] sums of two frames given as (y, u, v) plane triples."""
    return [plane_sum(x, y) for x, y in zip(fa, fb)]


def ssim(total: int, w: int, h: int) -> float:
    return total / (float(ONE) * windows(w, h))


def ssim_db(s: float) -> float:
    return float("inf") if s == 1 else float(-10 * np.log10(1 - s))
