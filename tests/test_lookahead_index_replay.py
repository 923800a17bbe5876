"""CPU: a replay of k_lookahead's index arithmetic (thor_amd/csrc/lookahead.hip)
with bounds checks.  The tile constants are read from the kernel's #defines; the
index expressions are restated here next to the lines they mirror, so a change
of the kernel's layout that this file does not follow fails on the constants or
has to be made here too.  Checked: every LDS word of the fill written once and
inside the array, every source byte of the fill inside the plane, every LDS
read of the two search passes and of the cost stage inside the image, and the
289 candidates covered exactly once."""
import os
import re

import numpy as np
import pytest

SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "thor_amd", "csrc", "lookahead.hip")


def _defines():
    env = {}
    for name, expr in re.findall(r"^#define (LA_[A-Z_]+) ([^/\n]+?)\s*(?://.*)?$", open(SRC).read(), re.M):
        env[name] = eval(expr, {}, env)  # (the defines are integer expressions of earlier defines)
    return env


D = _defines()
TBW, TBH, R, SIDE = D["LA_TBW"], D["LA_TBH"], D["LA_RANGE"], D["LA_SIDE"]
CUR_COLS, CUR_ROWS, CUR_STRIDE = D["LA_CUR_COLS"], D["LA_CUR_ROWS"], D["LA_CUR_STRIDE"]
REF_COLS, REF_ROWS, REF_STRIDE = D["LA_REF_COLS"], D["LA_REF_ROWS"], D["LA_REF_STRIDE"]
CUR_BYTES, REF_BYTES = D["LA_CUR_BYTES"], D["LA_REF_BYTES"]
LDS_WORDS = (CUR_BYTES + REF_BYTES) // 4  # (the four words of workgroup sums follow)


def test_constants():
    assert (TBW, TBH, R, SIDE, D["LA_NCAND"], D["LA_INL"]) == (8, 4, 8, 17, 289, 8)
    assert (CUR_STRIDE, CUR_ROWS, REF_STRIDE, REF_ROWS) == (72, 33, 80, 48)
    assert CUR_BYTES % 4 == 0 and REF_BYTES % 4 == 0 and CUR_BYTES + REF_BYTES + 16 == 6248


def _fill(rows, cols4, stride4, x_off, y_off, x0, y0, words):
    """(x, y) of the first lowres pixel of every group of the fill loop; its LDS word is written once, in range."""
    g = np.arange(rows * cols4)
    ry = g // cols4
    gx = g - ry * cols4
    idx = ry * stride4 + gx
    assert idx.min() >= 0 and idx.max() < words and len(np.unique(idx)) == len(idx)
    return x0 + x_off + 4 * gx, y0 + y_off + ry


def _source_in_plane(x, y, lw, lh, w, h):
    """la_lowres4: rows 2 yc, 2 yc + 1; bytes 2 x .. 2 x + 7 of a group inside the plane, else clamped pixels."""
    yc = np.clip(y, 0, lh - 1)
    fast = (x >= 0) & (x + 3 < lw)
    lo = np.where(fast, 2 * x, 2 * np.clip(x, 0, lw - 1))
    hi = np.where(fast, 2 * x + 7, 2 * np.clip(x + 3, 0, lw - 1) + 1)
    assert lo.min() >= 0 and hi.max() < w and (2 * yc).min() >= 0 and (2 * yc + 1).max() < h


@pytest.mark.parametrize("w,h", [(16, 16), (17, 19), (32, 32), (48, 32), (50, 38), (128, 64), (272, 80), (144, 144),
                                 (352, 288), (3840, 2160), (16384, 16), (16, 16384)])
def test_fill_stays_inside_the_plane_and_the_image(w, h):
    lw, lh = w >> 1, h >> 1
    bw, bh = lw >> 3, lh >> 3
    for ty in range((bh + TBH - 1) // TBH):
        for tx in range((bw + TBW - 1) // TBW):
            x0, y0 = tx * 8 * TBW, ty * 8 * TBH
            x, y = _fill(CUR_ROWS, CUR_COLS // 4, CUR_STRIDE // 4, -4, -1, x0, y0, CUR_BYTES // 4)
            _source_in_plane(x, y, lw, lh, w, h)
            x, y = _fill(REF_ROWS, REF_COLS // 4, REF_STRIDE // 4, -R, -R, x0, y0, REF_BYTES // 4)
            _source_in_plane(x, y, lw, lh, w, h)


def _first_pass(lane):
    return lane & 15, (lane >> 4) * 4  # dx, dy0: the lane takes dy0 .. dy0 + 3


def _second_pass(lane):
    q = min(lane, 2 * SIDE - 2)
    return (2 * R, q) if q < SIDE else (q - SIDE, 2 * R)  # dy, dx


def test_candidates_covered_once():
    first = [(dy0 + j) * SIDE + dx for dx, dy0 in map(_first_pass, range(64)) for j in range(4)]
    second = {dy * SIDE + dx for dy, dx in map(_second_pass, range(64))}
    assert len(first) == len(set(first)) == 256 and len(second) == 33 and not set(first) & second
    assert set(first) | second == set(range(SIDE * SIDE))


def test_lds_reads_stay_inside_the_image():
    for b in range(TBW * TBH):
        by, bx = divmod(b, TBW)
        cbase = (8 * by + 1) * CUR_STRIDE + 8 * bx + 4
        assert cbase % 4 == 0
        words = [((cbase + r * CUR_STRIDE) >> 2) + k for r in range(8) for k in (0, 1)]  # c0 / c1
        assert min(words) >= 0 and max(words) < CUR_BYTES // 4
        for lane in range(64):
            dx, dy0 = _first_pass(lane)
            rbase = (8 * by + dy0) * REF_STRIDE + 8 * bx + dx
            ws = [(rbase >> 2) + t * (REF_STRIDE // 4) + k for t in range(11) for k in (0, 1, 2)]
            assert min(ws) >= 0 and max(ws) < REF_BYTES // 4
            dy, dx = _second_pass(lane)
            rbase = (8 * by + dy) * REF_STRIDE + 8 * bx + dx
            ws = [(rbase >> 2) + r * (REF_STRIDE // 4) + k for r in range(8) for k in (0, 1, 2)]
            assert min(ws) >= 0 and max(ws) < REF_BYTES // 4
            # the cost stage: the DC sum's byte, the lane's own dword, the predictor's two dwords
            ea = cbase - CUR_STRIDE + lane if lane < 8 else cbase + ((lane - 8) & 7) * CUR_STRIDE - 1
            assert 0 <= ea < CUR_BYTES
            hf, rr, rj = lane & 1, (lane >> 1) & 7, lane >> 4
            own = cbase + rr * CUR_STRIDE + 4 * hf
            assert own % 4 == 0 and own + 4 <= CUR_BYTES
            for wdy in range(SIDE):
                for wdx in range(SIDE):
                    pa = own
                    if rj == 0:
                        pa = CUR_BYTES + (8 * by + wdy + rr) * REF_STRIDE + 8 * bx + wdx + 4 * hf
                    if rj == 2:
                        pa = cbase - CUR_STRIDE + 4 * hf
                    if rj == 3:
                        pa = cbase + rr * CUR_STRIDE - 1
                    assert pa >= 0 and (pa >> 2) + 1 < LDS_WORDS
