"""GPU: lookahead costs measured on the device (k_lookahead,
thor_amd/csrc/lookahead.hip) against the numpy model of the contract
(tests/lookahead_model.py).  Records and sums must equal the
model's exactly.

- the primitive (thor_lookahead_i420), thirteen pairs per size in one call (so
  every call splits into two launches): random, random plus noise, identical, the
  six shifted references (every corner of the search window, (0, 5) and
  (-3, 0): each corner takes another path through the kernel's two search
  passes), the striped tie pattern, 0 against 255, and an intra-only pair in the
  middle.  Sizes: 16x16 (one block, no neighbour, the whole search
  through the clamp), 48x32, 50x38 (lowres area beyond the last block), and the
  edges of the kernel's tile of 8 x 4 blocks (128 x 64 source pixels): 272x80
  (three tiles across, two down), 144x144 (two across, three down), 352x288.
  Planes tight, and at odd byte offsets with odd strides inside noise-filled
  guards; both outputs inside guards that must come back untouched
- 17 pairs of 32x32 in one call (three launches), with and without records
- scaler -> lookahead -> lookahead chained on one non-default stream
- GpuEncoder.input_costs() against the model, and the coded bytes with and
  without the call"""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLD = os.path.join(ROOT, "tests", "golden")

import lookahead_model as M  # noqa: E402
from dev_frames import _luma, _side_context, dev  # noqa: E402, F401

pytestmark = pytest.mark.gpu

LA_INL = 8   # pairs per launch (thor_amd/csrc/lookahead.hip)
GUARD = 64   # bytes either side of an output
FILL = 0xA5


def _enqueue(dev, cur, ref, w, h, blocks=True, stream=None):
    """thor_lookahead_i420 with both outputs inside guards; _collect reads them once the stream is done."""
    L, lib = dev.L, dev.lib
    n = len(cur)
    bw, bh = M.blocks(w, h)
    none = L.ThorYuvPlanes(None, None, None, 0, 0)
    refs = (L.ThorYuvPlanes * n)(*[none if r is None else r for r in ref])
    nb, ns = n * bw * bh * 8, n * 32
    d_recs = dev.put(np.full(nb + 2 * GUARD, FILL, np.uint8))
    d_sums = dev.put(np.full(ns + 2 * GUARD, FILL, np.uint8))
    L.check(lib.thor_lookahead_i420((L.ThorYuvPlanes * n)(*cur), refs, n, w, h, d_recs + GUARD if blocks else None,
                                    d_sums + GUARD, stream), "thor_lookahead_i420")
    return d_recs, d_sums, nb, ns, (n, bh, bw), blocks


def _collect(dev, job):
    """(records or None, sums) of an _enqueue, the guards checked."""
    d_recs, d_sums, nb, ns, shape, blocks = job
    raw_r, raw_s = dev.get(d_recs, nb + 2 * GUARD), dev.get(d_sums, ns + 2 * GUARD)
    for raw, size in ((raw_r, nb), (raw_s, ns)):
        assert (raw[:GUARD] == FILL).all() and (raw[GUARD + size:] == FILL).all(), "an output's guard was written"
    sums = raw_s[GUARD:GUARD + ns].view(np.uint64).reshape(shape[0], 4)
    if not blocks:
        assert (raw_r == FILL).all()
        return None, sums
    return raw_r[GUARD:GUARD + nb].view(M.BLOCK).reshape(shape), sums


def _run(dev, cur, ref, w, h, blocks=True):
    """On the null stream, which the read-back follows."""
    return _collect(dev, _enqueue(dev, cur, ref, w, h, blocks))


def _stripes(w, h, phase=0):
    x = (np.arange(w) // 2 - phase) % 4
    return np.tile(np.array([10, 90, 170, 250], np.uint8)[x][None, :], (h, 1))


SHIFTS = {"shift_8_m8": (8, -8), "shift_0_5": (0, 5), "shift_m3_0": (-3, 0), "shift_8_8": (8, 8), "shift_m8_8": (-8, 8),
          "shift_m8_m8": (-8, -8)}  # (dy, dx) in lowres pixels
CONTENT = ["random", "noise", "identical", "shift_8_m8", "shift_0_5", "intra_only", "shift_m3_0", "stripes", "black_white",
           "random2", "shift_8_8", "shift_m8_8", "shift_m8_m8"]


def _content(w, h):
    """[(cur, ref or None)] in CONTENT's order."""
    rng = np.random.default_rng(w * 31 + h)
    a = rng.integers(0, 256, (h, w), dtype=np.uint8)
    b = rng.integers(0, 256, (h, w), dtype=np.uint8)
    # (smooth content, so that costs are not all alike and the search has a gradient)
    s = ((a.astype(np.uint16) + np.roll(a, 1, 1) + np.roll(a, 1, 0) + np.roll(a, (1, 1), (0, 1))) // 4).astype(np.uint8)
    noisy = np.clip(s.astype(np.int16) + rng.integers(-3, 4, s.shape), 0, 255).astype(np.uint8)

    def shifted(p, dy, dx):  # lowres (y, x) of p lands at (y + dy, x + dx); w, h even
        return np.roll(p, (2 * dy, 2 * dx), axis=(0, 1))

    return [(a, b), (s, noisy), (a, a.copy()), (s, shifted(s, 8, -8)), (a, shifted(a, 0, 5)), (b, None),
            (s, shifted(s, -3, 0)), (_stripes(w, h), _stripes(w, h, 2)), (np.zeros((h, w), np.uint8), np.full((h, w), 255, np.uint8)),
            (b, s), (a, shifted(a, 8, 8)), (s, shifted(s, -8, 8)), (b, shifted(b, -8, -8))]


_MODEL = {}


def _want(w, h):
    """The model's (records, sums) of _content(w, h), computed once per size."""
    if (w, h) not in _MODEL:
        _MODEL[(w, h)] = [M.frame(c, r) for c, r in _content(w, h)]
    return _MODEL[(w, h)]


SIZES = [(16, 16), (48, 32), (50, 38), (272, 80), (144, 144), (352, 288)]


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("layout", ["tight", "odd_offsets"])
def test_lookahead_primitive_against_model(dev, w, h, layout):
    """tight: stride = width, planes at an allocation's start; odd_offsets: cur 1 byte and ref 3 bytes past it,
    strides width + 3 and width + 5.  All thirteen kinds of content in one call of two launches."""
    assert w % 2 == 0 and h % 2 == 0 and len(CONTENT) > LA_INL
    (cs, co), (rs, ro) = {"tight": ((w, 0), (w, 0)), "odd_offsets": ((w + 3, 1), (w + 5, 3))}[layout]
    pairs = _content(w, h)
    cur = [_luma(dev, c, cs, co) for c, _ in pairs]
    ref = [None if r is None else _luma(dev, r, rs, ro) for _, r in pairs]
    recs, sums = _run(dev, cur, ref, w, h)
    for name, got_r, got_s, (want_r, want_s) in zip(CONTENT, recs, sums.tolist(), _want(w, h)):
        for field in M.BLOCK.names:
            assert (got_r[field] == want_r[field]).all(), (w, h, layout, name, field, got_r[field], want_r[field])
        assert got_s == want_s, (w, h, layout, name, got_s, want_s)
    k = CONTENT.index("identical")
    assert (recs[k]["sad"] == 0).all() and (recs[k]["inter"] == 0).all() and sums[k, 1] == 0
    k = CONTENT.index("black_white")
    assert (recs[k]["sad"] == 16320).all() and (recs[k]["inter"] == 4080).all() and (recs[k]["mvx"] == 0).all()
    k = CONTENT.index("intra_only")
    assert (recs[k]["sad"] == M.NO_SAD).all() and (recs[k]["inter"] == recs[k]["intra"]).all()
    # every shifted reference: the device finds that vector, with SAD 0, in every block whose whole search
    # window lies inside the lowres plane (the sizes from 272 x 80 on have such blocks)
    bw, bh = M.blocks(w, h)
    ys, xs = 8 * np.arange(bh)[:, None], 8 * np.arange(bw)[None, :]
    ins = (ys >= M.RANGE) & (ys + 8 + M.RANGE <= h >> 1) & (xs >= M.RANGE) & (xs + 8 + M.RANGE <= w >> 1)
    assert ins.any() == (w >= 144 and h >= 80)
    for name, (dy, dx) in SHIFTS.items():
        r = recs[CONTENT.index(name)]
        assert (r["mvy"][ins] == dy).all() and (r["mvx"][ins] == dx).all() and (r["sad"][ins] == 0).all(), (w, h, name)


def test_lookahead_synthetic_scene_cut(dev):
    """352 x 288 synth frames, seed 1 for t = 0..2 and seed 2 for t = 3..5, through sequence_costs: the model's
    sums, and the cut at the seed change for every percent from 70 to 90."""
    from thor_amd import lookahead, synth

    w, h = 352, 288
    frames = [np.concatenate([p.ravel() for p in synth.synth_frame(w, h, t, 1 if t < 3 else 2)]) for t in range(6)]
    want = M.sequence([f[:w * h].reshape(h, w) for f in frames])
    sums, recs = lookahead.sequence_costs(dev.put(np.stack(frames)), 6, w, h, blocks=True)
    assert sums.dtype == np.uint64 and sums.shape == (6, 4) and recs.shape == (6, 18, 22)
    assert sums.tolist() == [s for _, s in want]
    for k in range(6):
        assert (recs[k] == want[k][0]).all(), k
    for percent in (70, 80, 90):
        assert lookahead.scene_cuts(sums, percent) == [0, 3]


@pytest.mark.parametrize("blocks", [True, False])
def test_lookahead_batch_splits_into_launches(dev, blocks):
    """17 different pairs of 32 x 32 (three launches), the fourth and the last intra-only: each pair's own
    records and sums, in order; without records the sums alone, and nothing written through the NULL."""
    n, (w, h) = 2 * LA_INL + 1, (32, 32)
    rng = np.random.default_rng(17)
    fa = [rng.integers(0, 256, (h, w), dtype=np.uint8) for _ in range(n)]
    fb = [None if i in (3, n - 1) else np.roll(np.clip(fa[i].astype(np.int16) + (i - 8) * 2, 0, 255).astype(np.uint8), 2 * (i % 5 - 2), 1)
          for i in range(n)]
    want = [M.frame(c, r) for c, r in zip(fa, fb)]
    assert len({tuple(s) for _, s in want}) == n
    cur = [_luma(dev, c, w, 0) for c in fa]
    ref = [None if r is None else _luma(dev, r, w + 5, 3) for r in fb]
    recs, sums = _run(dev, cur, ref, w, h, blocks=blocks)
    assert sums.tolist() == [s for _, s in want]
    if blocks:
        for i in range(n):
            assert (recs[i] == want[i][0]).all(), i


def test_lookahead_behind_the_scaler_on_one_stream(dev):
    """Three 96 x 64 frames scaled to 48 x 32 by the device scaler, then two lookahead calls (frames 1, 2 against
    0, 1; then frame 0 intra-only), all on one non-default stream: equal to the model on the scaled bytes."""
    from thor_amd.scale import Scaler, i420_planes

    w, h, w2, h2, n = 96, 64, 48, 32, 3
    fs, fs2 = w * h * 3 // 2, w2 * h2 * 3 // 2
    rng = np.random.default_rng(77)
    base = rng.integers(0, 256, (h + 8, w + 8), dtype=np.uint8)
    base = ((base.astype(np.uint16) + np.roll(base, 1, 1) + np.roll(base, 1, 0) + np.roll(base, (1, 1), (0, 1))) // 4).astype(np.uint8)
    src = np.stack([np.concatenate([base[2 * t:2 * t + h, 4 * t:4 * t + w].ravel(), np.full(fs - w * h, 128, np.uint8)])
                    for t in range(n)])
    d_src, d_small = dev.put(src), dev.put(np.zeros(n * fs2, np.uint8))
    ctx = _side_context()
    down = Scaler(w, h, w2, h2)
    try:
        st = ctx.stream()
        assert st
        down.run_frames(d_src, d_small, n, st)
        small = [i420_planes(d_small + k * fs2, w2, h2) for k in range(n)]
        j1 = _enqueue(dev, small[1:], small[:-1], w2, h2, stream=st)
        j0 = _enqueue(dev, small[:1], [None], w2, h2, stream=st)
        ctx.sync()
        (r1, s1), (r0, s0) = _collect(dev, j1), _collect(dev, j0)
        back = dev.get(d_small, n * fs2).reshape(n, fs2)
    finally:
        down.close()
        ctx.close()
    luma = [back[k, :w2 * h2].reshape(h2, w2) for k in range(n)]
    assert (luma[0] != luma[1]).any()
    want = M.sequence(luma)
    assert s0.tolist() == [want[0][1]] and (r0[0] == want[0][0]).all()
    assert s1.tolist() == [want[1][1], want[2][1]] and (r1[0] == want[1][0]).all() and (r1[1] == want[2][0]).all()
    assert want[1][1][1] < want[1][1][0]  # the pan is found: inter below intra


def test_encoder_input_costs(dev):
    """Six 128 x 64 frames uploaded to an encoder: input_costs() equals the model (frame k against k - 1, frame 0
    intra-only), before the first frame and between frames, and the coded bytes equal those of a run without
    the call."""
    from thor_amd import synth
    from thor_amd.encoder import GpuEncoder, params_for

    with open(os.path.join(GOLD, "quality.json")) as f:
        m = json.load(f)["ldb_nofilt"]
    w, h, nin, ncode = 128, 64, 6, 3
    seq = synth.synth_frames(w, h, nin, 7, workers=1)
    want = M.sequence([f[:w * h].reshape(h, w) for f in seq.reshape(nin, -1)])

    def run(measure):
        enc = GpuEncoder(params_for(m["config"], w, h, ncode, m["extra"]))
        chunks = []
        try:
            enc.upload_sequence(seq)
            if measure:
                sums, recs = enc.input_costs(blocks=True)
                assert sums.shape == (nin, 4) and recs.shape == (nin, 4, 8)
                assert sums.tolist() == [s for _, s in want]
                for k in range(nin):
                    assert (recs[k] == want[k][0]).all(), k
            chunks.append(bytes(enc.encode_next()))
            if measure:
                assert enc.input_costs().tolist() == [s for _, s in want]
            chunks += [bytes(enc.encode_next()) for _ in range(ncode - 1)]
        finally:
            enc.close()
        return chunks

    with_call, without = run(True), run(False)
    assert with_call == without and all(len(c) > 4 for c in without)
