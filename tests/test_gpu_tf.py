"""GPU: the temporal filter on the device (k_tf_luma / k_tf_chroma,
thor_amd/csrc/tf.hip) against the numpy model of the contract
(tests/tf_model.py).  Output planes and records must equal
the model's exactly.

- the primitive (thor_tf_i420), five targets of four references per size in one
  call (TF_INL = 4 targets per launch, so every call splits into two launches):
  random / smooth plus noise / identical / ^ 0x80; whole-pixel shifts to the four
  corners of the combined window (start +-16, refinement +-2); half-pel shifts
  in x, y and both with an absent reference in the middle; all references
  absent; and a mix with an absent reference.  Sizes: 16x16 (one lookahead
  block, everything through the clamp), 24x40 (8x8 blocks outside the
  lookahead's grid in both directions), 48x32, 136x40 (the luma kernel's tile is
  64 x 16 pixels, the chroma kernel's 64 x 4 blocks of 8x8 luma pixels: two
  luma tiles and a partial one in each direction), 352x288.  Planes tight, and
  at byte offsets 1 and 3 with odd strides inside noise-filled guards; outputs
  and records inside guards that must come back untouched
- a call without records; nrefs 1 and 2; strengths (1, 1) and (64, 64)
- filter_sequence over six 128x64 synth frames at radius 1 and 2
- scaler -> filter chained on one non-default stream
- GpuEncoder.filter_input() against an encoder given the model's frames, and
  the golden bytes of an encoder that never calls it"""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLD = os.path.join(ROOT, "tests", "golden")

import tf_model as M  # noqa: E402
from dev_frames import _frame_in, _side_context, dev  # noqa: E402, F401

pytestmark = pytest.mark.gpu

TF_INL = 4   # targets per launch (thor_amd/csrc/tf.hip)
GUARD = 64   # bytes either side of an output
FILL = 0xA5


class _Out:
    """An output frame whose three planes lie inside FILL bytes: GUARD either side, and the row padding."""

    def __init__(self, dev, w, h, pad, off):
        self.dev, self.shapes, self.off = dev, [(h, w), (h // 2, w // 2), (h // 2, w // 2)], off
        self.strides = [w + pad, w // 2 + pad, w // 2 + pad]
        self.sizes = [GUARD + off + hh * s + GUARD for (hh, _), s in zip(self.shapes, self.strides)]
        self.ptrs = [dev.put(np.full(n, FILL, np.uint8)) for n in self.sizes]
        p = [q + GUARD + off for q in self.ptrs]
        self.planes = dev.L.ThorYuvPlanes(p[0], p[1], p[2], self.strides[0], self.strides[1])

    def collect(self):
        out = []
        for q, n, (hh, ww), s in zip(self.ptrs, self.sizes, self.shapes, self.strides):
            raw = self.dev.get(q, n)
            body = raw[GUARD + self.off:GUARD + self.off + hh * s].reshape(hh, s)
            out.append(body[:, :ww].copy())
            body[:, :ww] = FILL
            assert (raw == FILL).all(), "bytes around an output plane were written"
        return tuple(out)


def _run(dev, tf, targets, refs, w, h, strength=(8, 3), records=True, in_pad=0, in_off=(0, 0), out_pad=0, out_off=0,
         stream=None):
    """thor_tf_i420 of host frames: (filtered triples, records or None), every guard checked."""
    L, lib = dev.L, dev.lib
    n, nrefs = len(targets), len(refs[0])
    cur = [_frame_in(dev, t, in_pad, in_off[0]) for t in targets]
    none = L.ThorYuvPlanes(None, None, None, 0, 0)
    rf = [none if r is None else _frame_in(dev, r, in_pad + (2 if in_pad else 0), in_off[1]) for rs in refs for r in rs]
    outs = [_Out(dev, w, h, out_pad, out_off) for _ in range(n)]
    nb = n * nrefs * (w >> 3) * (h >> 3) * 4
    d_recs = dev.put(np.full(nb + 2 * GUARD, FILL, np.uint8))
    L.check(lib.thor_tf_i420(tf.h_, (L.ThorYuvPlanes * n)(*cur), (L.ThorYuvPlanes * len(rf))(*rf),
                             (L.ThorYuvPlanes * n)(*[o.planes for o in outs]), n, nrefs, strength[0], strength[1],
                             d_recs + GUARD if records else None, stream), "thor_tf_i420")
    got = [o.collect() for o in outs]  # (the null stream: the read-back follows the kernels)
    raw = dev.get(d_recs, nb + 2 * GUARD)
    if not records:
        assert (raw == FILL).all()
        return got, None
    assert (raw[:GUARD] == FILL).all() and (raw[GUARD + nb:] == FILL).all(), "the records' guard was written"
    return got, raw[GUARD:GUARD + nb].view(M.RECORD).reshape(n, nrefs, h >> 3, w >> 3)


def _chroma_of(y, seed):
    """Chroma planes that follow the luma (its 2x2 mean, offset), so that the luma vectors mean something there."""
    h, w = y.shape
    c = (y.astype(np.uint16).reshape(h // 2, 2, w // 2, 2).sum(axis=(1, 3)) // 4).astype(np.int16)
    rng = np.random.default_rng(seed)
    return (np.clip(c // 2 + 60 + rng.integers(-1, 2, c.shape), 0, 255).astype(np.uint8),
            np.clip(200 - c // 2 + rng.integers(-1, 2, c.shape), 0, 255).astype(np.uint8))


def _frame_of(y, seed):
    return (y,) + _chroma_of(y, seed)


def _roll(f, dy, dx):
    """The frame that holds f's luma pixel (y, x) at (y + dy, x + dx) (dy, dx even; wraps)."""
    return (np.roll(f[0], (dy, dx), (0, 1)), np.roll(f[1], (dy // 2, dx // 2), (0, 1)), np.roll(f[2], (dy // 2, dx // 2), (0, 1)))


def _half_pel(f, mvy, mvx):
    """f predicted at a constant half-pel luma vector, every plane by the contract's own rule."""
    out = []
    for c, p in enumerate(f):
        n = 4 if c else 8
        hh, ww = p.shape
        y0, x0 = M._grid(ww, hh, n)
        vy, vx = (mvy >> 1, mvx >> 1) if c else (mvy, mvx)
        out.append(M._untile(M.predict(p, y0, x0, n, np.full(len(y0), vy), np.full(len(y0), vx)), ww, hh, n).astype(np.uint8))
    return tuple(out)


def _content(w, h):
    """(targets, refs): five targets of four references."""
    rng = np.random.default_rng(w * 31 + h)
    a = rng.integers(0, 256, (h, w), dtype=np.uint8)
    b = rng.integers(0, 256, (h, w), dtype=np.uint8)
    s = a.astype(np.uint16)
    for _ in range(2):  # smooth content, so that the searches have a gradient
        s = (s + np.roll(s, 1, 1) + np.roll(s, 1, 0) + np.roll(s, (1, 1), (0, 1)) + 2) // 4
    s = s.astype(np.uint8)
    noisy = [np.clip(s.astype(np.int16) + rng.integers(-4, 5, s.shape), 0, 255).astype(np.uint8)]
    A, B, S = _frame_of(a, 1), tuple(rng.integers(0, 256, p.shape, dtype=np.uint8) for p in _frame_of(b, 2)), _frame_of(s, 3)
    N0 = _frame_of(noisy[0], 4)
    AN = _frame_of(np.clip(a.astype(np.int16) + rng.integers(-6, 7, a.shape), 0, 255).astype(np.uint8), 5)
    # very smooth (a 9x9 box twice, full contrast): the half-resolution stage, which has no candidate at 9 of its
    # pixels, then lands at 8 in most blocks, and the refinement's corner +-2 gives the window's corner +-18
    v = b.astype(np.float64)
    for _ in range(2):
        v = sum(np.roll(v, k, 0) for k in range(-4, 5)) / 9
        v = sum(np.roll(v, k, 1) for k in range(-4, 5)) / 9
    V = _frame_of(np.rint((v - v.min()) / (v.max() - v.min()) * 255).astype(np.uint8), 6)
    targets = [S, V, S, A, A]
    refs = [[B, N0, tuple(p.copy() for p in S), tuple(p ^ 0x80 for p in S)],
            [_roll(V, 18, 18), _roll(V, 18, -18), _roll(V, -18, 18), _roll(V, -18, -18)],
            [_half_pel(S, 0, 1), _half_pel(S, 1, 0), None, _half_pel(S, -3, 5)],
            [None, None, None, None],
            [B, _roll(AN, -2, 6), None, _roll(A, 4, -10)]]
    return targets, refs


_MODEL = {}


def _want(w, h, strength=(8, 3)):
    """The model's [(out, records)] of _content(w, h), computed once per size and strength."""
    key = (w, h, strength)
    if key not in _MODEL:
        targets, refs = _content(w, h)
        _MODEL[key] = [M.frame(t, r, strength) for t, r in zip(targets, refs)]
    return _MODEL[key]


def _compare(got, recs, want, tag):
    for i, (g, (wo, wr)) in enumerate(zip(got, want)):
        if recs is not None:
            for field in M.RECORD.names:
                assert (recs[i][field] == wr[field]).all(), (tag, i, field, np.argwhere(recs[i][field] != wr[field])[:4])
        for c in range(3):
            assert (g[c] == wo[c]).all(), (tag, i, c, np.argwhere(g[c] != wo[c])[:4])


SIZES = [(16, 16), (24, 40), (48, 32), (136, 40), (352, 288)]


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("layout", ["tight", "odd_offsets"])
def test_tf_primitive_against_model(dev, w, h, layout):
    """tight: stride = width, planes at an allocation's start; odd_offsets: the targets 1 byte and the references
    3 bytes past it, strides width + 3 and width + 5 (chroma alike), outputs at offset 1 with stride + 1."""
    from thor_amd.tfilter import TemporalFilter

    targets, refs = _content(w, h)
    assert len(targets) > TF_INL
    kw = {"tight": {}, "odd_offsets": dict(in_pad=3, in_off=(1, 3), out_pad=1, out_off=1)}[layout]
    tf = TemporalFilter(w, h, len(targets))
    try:
        got, recs = _run(dev, tf, targets, refs, w, h, **kw)
    finally:
        tf.close()
    want = _want(w, h)
    _compare(got, recs, want, (w, h, layout))
    # identical and ^ 0x80 weigh nothing or change nothing; all references absent: the target itself, zero records
    for c in range(3):
        assert (got[3][c] == targets[3][c]).all()
    assert not recs[3].view(np.uint32).any() and not recs[2][2].view(np.uint32).any() and not recs[4][2].view(np.uint32).any()
    assert (recs[0][2]["e"] == 0).all() and (recs[0][2]["mvx"] == 0).all() and (recs[0][2]["mvy"] == 0).all()
    # the corners of the combined window (start +-16, refinement +-2) are taken, with no error, at the large size
    if (w, h) == (352, 288):
        for r, (dy, dx) in enumerate([(18, 18), (18, -18), (-18, 18), (-18, -18)]):
            m = recs[1][r]
            hit = (m["mvy"] == 2 * dy) & (m["mvx"] == 2 * dx) & (m["e"] == 0)
            assert hit.sum() >= 100, (dy, dx, int(hit.sum()))


@pytest.mark.parametrize("strength", [(1, 1), (64, 64)])
def test_tf_strengths(dev, strength):
    from thor_amd.tfilter import TemporalFilter

    w, h = 48, 32
    targets, refs = _content(w, h)
    tf = TemporalFilter(w, h, len(targets))
    try:
        got, recs = _run(dev, tf, targets, refs, w, h, strength=strength)
    finally:
        tf.close()
    _compare(got, recs, _want(w, h, strength), strength)
    assert any((_want(w, h, strength)[0][0][c] != _want(w, h)[0][0][c]).any() for c in range(3))


@pytest.mark.parametrize("nrefs", [1, 2])
def test_tf_fewer_references_and_no_records(dev, nrefs):
    """nrefs 1 and 2 (24 x 40, odd offsets), without records: nothing is written where they would have gone, and
    the context's own records serve the chroma kernel."""
    from thor_amd.tfilter import TemporalFilter

    w, h = 24, 40
    targets, refs = _content(w, h)
    targets, refs = targets[:3], [r[:nrefs] for r in refs[:3]]
    want = [M.frame(t, r, (8, 3)) for t, r in zip(targets, refs)]
    tf = TemporalFilter(w, h, 4)
    try:
        got, recs = _run(dev, tf, targets, refs, w, h, in_pad=3, in_off=(1, 3), out_pad=1, out_off=3)
        _compare(got, recs, want, nrefs)
        got, recs = _run(dev, tf, targets, refs, w, h, records=False)
        assert recs is None
        _compare(got, None, want, nrefs)
    finally:
        tf.close()


def _synth_sequence(w, h, n, seed):
    from thor_amd import synth

    return np.ascontiguousarray(synth.synth_frames(w, h, n, seed, workers=1), dtype=np.uint8).reshape(n, -1)


@pytest.mark.parametrize("radius", [1, 2])
def test_filter_sequence_against_model(dev, radius):
    """Six 128 x 64 synth frames: frame k from the unfiltered frames k - radius .. k + radius that exist."""
    from thor_amd import tfilter

    w, h, n = 128, 64, 6
    seq = _synth_sequence(w, h, n, 7)
    want = M.sequence(seq, w, h, radius)
    d_src, d_dst = dev.put(seq), dev.put(np.zeros_like(seq))
    tfilter.filter_sequence(d_src, d_dst, n, w, h, radius)
    got = dev.get(d_dst, seq.size).reshape(n, -1)
    for k in range(n):
        assert (got[k] == want[k]).all(), (radius, k)
    assert (dev.get(d_src, seq.size).reshape(n, -1) == seq).all()
    assert (want != seq).any()


def test_tf_behind_the_scaler_on_one_stream(dev):
    """Four 96 x 64 frames scaled to 48 x 32 by the device scaler, then filtered at radius 1, both on one
    non-default stream: equal to the model on the scaled bytes."""
    from thor_amd import tfilter
    from thor_amd.scale import Scaler

    w, h, w2, h2, n = 96, 64, 48, 32, 4
    fs2 = w2 * h2 * 3 // 2
    src = _synth_sequence(w, h, n, 11)
    d_src, d_small, d_out = dev.put(src), dev.put(np.zeros(n * fs2, np.uint8)), dev.put(np.zeros(n * fs2, np.uint8))
    ctx = _side_context()
    down = Scaler(w, h, w2, h2)
    tf = tfilter.TemporalFilter(w2, h2, n)
    try:
        st = ctx.stream()
        assert st
        down.run_frames(d_src, d_small, n, st)
        tfilter.filter_sequence(d_small, d_out, n, w2, h2, 1, stream=st, tf=tf)
        ctx.sync()
        small = dev.get(d_small, n * fs2).reshape(n, fs2)
        got = dev.get(d_out, n * fs2).reshape(n, fs2)
    finally:
        tf.close()
        down.close()
        ctx.close()
    assert (small[0] != small[1]).any()
    want = M.sequence(small, w2, h2, 1)
    assert (got == want).all() and (want != small).any()


def test_encoder_filter_input(dev):
    """Six 128 x 64 frames uploaded to an encoder, filter_input(): the coded bytes equal those of an encoder given
    the model's filtered frames through upload_sequence, and differ from the unfiltered run's."""
    from thor_amd.encoder import GpuEncoder, params_for

    with open(os.path.join(GOLD, "quality.json")) as f:
        m = json.load(f)["ldb_nofilt"]
    w, h, nin, ncode = 128, 64, 6, 3
    seq = _synth_sequence(w, h, nin, 7)
    model = M.sequence(seq, w, h, 2)

    def run(frames, filt):
        enc = GpuEncoder(params_for(m["config"], w, h, ncode, m["extra"]))
        try:
            enc.upload_sequence(frames)
            if filt:
                enc.filter_input()
                assert enc.own_seq and enc.nin == nin
            return [bytes(enc.encode_next()) for _ in range(ncode)]
        finally:
            enc.close()

    on_device, from_model, plain = run(seq, True), run(model, False), run(seq, False)
    assert on_device == from_model and all(len(c) > 4 for c in on_device)
    assert on_device != plain


def test_encoder_without_the_filter_codes_the_golden_bytes():
    """An encoder that never calls filter_input() (the library with the filter in it): the golden .bit."""
    from thor_amd import synth
    from thor_amd.encoder import GpuEncoder, params_for

    with open(os.path.join(GOLD, "streams.json")) as f:
        meta = json.load(f)["cif_low"]
    n, w, h = 3, meta["width"], meta["height"]
    enc = GpuEncoder(params_for(meta["config"], w, h, n, meta["extra"]))
    try:
        enc.upload_sequence(synth.synth_frames(w, h, n, meta["seed"], workers=1))
        bits = enc.encode_all()
    finally:
        enc.close()
    with open(os.path.join(GOLD, "cif_low.bit"), "rb") as f:
        assert len(bits) > 100 and f.read().startswith(bits)
