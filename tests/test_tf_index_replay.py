"""CPU: a replay of the index arithmetic of k_tf_luma and k_tf_chroma
(thor_amd/csrc/tf.hip) with bounds checks.  The tile constants are read from the
kernel's #defines; the index expressions are restated here next to the lines
they mirror, so a change of the kernel's layout that this file does not follow
fails on the constants or has to be made here too.  Checked: every LDS word of
the window fill written once and inside the array, every source byte of the
fills inside the plane, every LDS read of the two search stages and of the
blend inside the window's filled rows and columns, the candidates covered
exactly once, every output byte and record written exactly once and inside the
frame, and the chroma kernel's reads and writes inside its planes."""
import os
import re

import numpy as np
import pytest

SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "thor_amd", "csrc", "tf.hip")


def _defines():
    env = {}
    for name, expr in re.findall(r"^#define (TF_[A-Z_]+) ([^/\n]+?)\s*(?://.*)?$", open(SRC).read(), re.M):
        env[name] = eval(expr, {}, env)  # (the defines are integer expressions of earlier defines)
    return env


D = _defines()
BLK, WAVES, IR, MARGIN = D["TF_BLK"], D["TF_WAVES"], D["TF_IR"], D["TF_MARGIN"]
ROWS, COLS, STRIDE, WORDS = D["TF_WIN_ROWS"], D["TF_WIN_COLS"], D["TF_WIN_STRIDE"], D["TF_WIN_WORDS"]
CUR_WORDS, WAVE_WORDS, INL = D["TF_CUR_WORDS"], D["TF_WAVE_WORDS"], D["TF_INL"]
CBX, CBY = D["TF_CBX"], D["TF_CBY"]
SIDE = 2 * IR + 1
SIZES = [(16, 16), (24, 40), (48, 32), (136, 40), (352, 288), (16384, 16), (16, 16384)]


def test_constants():
    assert (BLK, WAVES, IR, MARGIN, INL) == (16, 4, 2, 3, 4)
    assert (D["TF_TILE_W"], D["TF_TILE_H"]) == (64, 16)
    assert (ROWS, COLS, STRIDE, WORDS, CUR_WORDS, WAVE_WORDS) == (22, 22, 24, 132, 64, 196)
    assert (CBX, CBY) == (64, 4) and CBX * CBY == 256 and D["TF_LUT_WORDS"] == 64
    assert (WAVES * WAVE_WORDS + D["TF_LUT_WORDS"]) * 4 == 3392  # the workgroup's LDS


def _load4_in_plane(x, y, w, h):
    """ld4_clamped (frame_ops.h): row clamped; bytes x .. x + 3 of a group inside the plane, else clamped pixels."""
    yc = np.clip(y, 0, h - 1)
    fast = (x >= 0) & (x + 3 < w)
    lo = np.where(fast, x, np.clip(x, 0, w - 1))
    hi = np.where(fast, x + 3, np.clip(x + 3, 0, w - 1))
    assert lo.min() >= 0 and hi.max() < w and yc.min() >= 0 and yc.max() < h


def _edge_blocks(nx, ny):
    """All blocks of a small grid; of a large one the first two and last two of every row and column."""
    xs = range(nx) if nx <= 24 else [0, 1, nx // 2, nx - 2, nx - 1]
    ys = range(ny) if ny <= 24 else [0, 1, ny // 2, ny - 2, ny - 1]
    return [(X, Y) for Y in ys for X in xs]


@pytest.mark.parametrize("w,h", SIZES)
def test_fills_stay_inside_the_plane_and_the_window(w, h):
    gx_tiles, gy_tiles = (w + BLK * WAVES - 1) // (BLK * WAVES), (h + BLK - 1) // BLK
    g = np.concatenate([np.arange(lane, WORDS, 64) for lane in range(64)])  # for (g = lane; g < WORDS; g += 64)
    assert len(g) == WORDS and len(np.unique(g)) == WORDS and g.min() == 0 and g.max() == WORDS - 1
    ry = g // (STRIDE // 4)
    gx = g - ry * (STRIDE // 4)
    assert ry.max() == ROWS - 1 and gx.max() == STRIDE // 4 - 1
    lane = np.arange(64)
    for X, Y in _edge_blocks(gx_tiles * WAVES, gy_tiles):
        x0, y0 = BLK * X, BLK * Y
        if not x0 < w:  # live
            continue
        assert y0 < h
        # the target's block: curw[lane]
        px, py = x0 + 4 * (lane & 3), y0 + (lane >> 2)
        ok = (px < w) & (py < h)
        assert (px[ok] + 3 < w).all() and ok.any()
        for sy in (-16, 0, 16):
            for sx in (-16, 0, 16):
                _load4_in_plane(x0 + sx - MARGIN + 4 * gx, y0 + sy - MARGIN + ry, w, h)


def _row9(row, col):
    """tf_row9: the three words, inside the window and the row; the nine bytes inside the filled columns."""
    a = row * STRIDE + col
    assert 0 <= row < ROWS and 0 <= col and col + 8 < COLS
    assert 0 <= (a >> 2) and (a >> 2) + 2 < WORDS and (col >> 2) + 2 < STRIDE // 4 and (a & 3) == (col & 3)


def _row5(row, col):
    a = row * STRIDE + col
    assert 0 <= row < ROWS and 0 <= col and col + 4 < COLS
    assert 0 <= (a >> 2) and (a >> 2) + 1 < WORDS and (col >> 2) + 1 < STRIDE // 4


def _integer_candidate(l16, p):
    k = min(l16 + 16 * p, SIDE * SIDE - 1)
    dy = k // SIDE - IR
    return k, dy, k - (dy + IR) * SIDE - IR


def test_candidates_covered_once():
    ks = [_integer_candidate(l16, p) for p in range(2) for l16 in range(16)]
    assert {k for k, _, _ in ks} == set(range(SIDE * SIDE))
    assert sorted({(dy, dx) for _, dy, dx in ks}) == [(dy, dx) for dy in range(-IR, IR + 1) for dx in range(-IR, IR + 1)]
    for k, dy, dx in ks:
        assert k == (dy + IR) * SIDE + dx + IR
    hs = []
    for l16 in range(16):
        k = min(l16, 8)
        hy = k // 3 - 1
        hs.append((k, hy, k - (hy + 1) * 3 - 1))
    assert sorted({(hy, hx) for _, hy, hx in hs}) == [(hy, hx) for hy in (-1, 0, 1) for hx in (-1, 0, 1)]
    for k, hy, hx in hs:
        assert k == (hy + 1) * 3 + hx + 1


def test_lds_reads_stay_inside_the_window():
    for lane in range(64):
        sub, l16 = lane >> 4, lane & 15
        sbx, sby = sub & 1, sub >> 1
        rr, hf = l16 >> 1, l16 & 1
        # the target's block: c0 / c1 and the lane's own dword
        for r in range(8):
            i = (8 * sby + r) * (BLK // 4) + 2 * sbx
            assert 0 <= i and i + 1 < CUR_WORDS
        assert 0 <= (8 * sby + rr) * (BLK // 4) + 2 * sbx + hf < CUR_WORDS
        brow, bcol = 8 * sby + MARGIN, 8 * sbx + MARGIN
        for p in range(2):
            _, dy, dx = _integer_candidate(l16, p)
            for j in range(8):
                _row9(brow + dy + j, bcol + dx)
        for oy in range(-IR, IR + 1):
            for ox in range(-IR, IR + 1):
                k = min(l16, 8)
                hy = k // 3 - 1
                hx = k - (hy + 1) * 3 - 1
                row, col = brow + oy + (hy >> 1), bcol + ox + (hx >> 1)
                for j in range(9):
                    _row9(row + j, col)
                for hy in (-1, 0, 1):
                    for hx in (-1, 0, 1):
                        row, col = brow + oy + (hy >> 1) + rr, bcol + ox + (hx >> 1) + 4 * hf
                        _row5(row, col)
                        _row5(row + 1, col)


def test_window_coordinates_are_the_contract_positions():
    """Window (row, col) holds the reference pixel (y0 + sy - MARGIN + row, x0 + sx - MARGIN + col): the
    prediction's integer position of a sub-block's pixel (rr, 4 hf) at the vector 2 (s + o) + h."""
    y0, sy = 32, -6
    for sby in (0, 1):
        for oy in range(-IR, IR + 1):
            for hy in (-1, 0, 1):
                for rr in range(8):
                    mvy = 2 * (sy + oy) + hy
                    want = y0 + 8 * sby + rr + (mvy >> 1)
                    row = 8 * sby + MARGIN + oy + (hy >> 1) + rr
                    assert y0 + sy - MARGIN + row == want and (mvy & 1) == (hy & 1)


@pytest.mark.parametrize("w,h", SIZES)
def test_outputs_and_records_written_once_inside_the_frame(w, h):
    bw8, bh8 = w >> 3, h >> 3
    gx_tiles, gy_tiles = (w + BLK * WAVES - 1) // (BLK * WAVES), (h + BLK - 1) // BLK
    assert gx_tiles * WAVES * BLK >= w and gy_tiles * BLK >= h
    lane = np.arange(64)
    sub, l16 = lane >> 4, lane & 15
    sbx, sby, rr, hf = sub & 1, sub >> 1, l16 >> 1, l16 & 1
    small = w * h <= 352 * 288
    seen = np.zeros((h, w), np.int32) if small else None
    recs = np.zeros((bh8, bw8), np.int32) if small else None
    for X, Y in ([(X, Y) for Y in range(gy_tiles) for X in range(gx_tiles * WAVES)] if small else
                 _edge_blocks(gx_tiles * WAVES, gy_tiles)):
        x0, y0 = BLK * X, BLK * Y
        live = x0 < w
        sub_live = live & (x0 + 8 * sbx < w) & (y0 + 8 * sby < h)
        y, x = y0 + 8 * sby + rr, x0 + 8 * sbx + 4 * hf
        assert (y[sub_live] < h).all() and (x[sub_live] + 3 < w).all()
        ry, rx = 2 * Y + sby, 2 * X + sbx
        head = sub_live & (l16 == 0)
        assert (ry[head] < bh8).all() and (rx[head] < bw8).all()
        if small:
            for i in np.nonzero(sub_live)[0]:
                seen[y[i], x[i]:x[i] + 4] += 1
            for i in np.nonzero(head)[0]:
                recs[ry[i], rx[i]] += 1
    if small:
        assert (seen == 1).all() and (recs == 1).all()


@pytest.mark.parametrize("w,h", SIZES)
def test_chroma_reads_and_writes_stay_inside_the_planes(w, h):
    bw8, bh8, cw, ch = w >> 3, h >> 3, w >> 1, h >> 1
    gx, gy = (bw8 + CBX - 1) // CBX, (bh8 + CBY - 1) // CBY
    tid = np.arange(256)
    seen = np.zeros((bh8, bw8), np.int32)
    for Yb in (range(gy) if gy <= 80 else [0, 1, gy - 2, gy - 1]):
        for Xb in range(gx):
            bx, by = Xb * CBX + (tid & (CBX - 1)), Yb * CBY + tid // CBX
            ok = (bx < bw8) & (by < bh8)
            bx, by = bx[ok], by[ok]
            seen[by, bx] += 1
            assert (4 * bx + 3 < cw).all() and (4 * by + 3 < ch).all()  # the target's and the output's 4x4 block
            for mv in (-37, -36, -3, -2, -1, 0, 1, 2, 3, 36, 37):  # the luma vector; the chroma one is mv >> 1
                c = mv >> 1
                ix, iy = 4 * bx + (c >> 1), 4 * by + (c >> 1)
                inside = (ix >= 0) & (ix + 4 < cw)
                lo = np.where(inside, ix, np.clip(ix, 0, cw - 1))
                hi = np.where(inside, ix + 4, np.clip(ix + 4, 0, cw - 1))
                assert lo.min() >= 0 and hi.max() < cw
                for j in range(5):
                    r = np.clip(iy + j, 0, ch - 1)
                    assert r.min() >= 0 and r.max() < ch
    if gy <= 80:
        assert (seen == 1).all()
