"""GPU: SSIM measured on the device (k_ssim_i420, thor_amd/csrc/ssim.hip) against
the numpy model of the contract (tests/ssim_model.py).  The
device sums must equal the model's exactly.

- the primitive (thor_ssim_i420), six kinds of content per size in one call:
  the sizes the contract names (one chroma window, both remainders, wider than
  one wave, many bands) and the three sizes one block under, at and over each
  edge of the kernel:
    a tile owns 252 window columns (w = 1012 at the edge: 1008, 1012, 1016; for
    chroma 2016, 2024, 2032);
    a tile whose 64 lanes all lie inside the plane takes the branch-free path
    from 256 blocks on (w = 1020, 1024, 1028; for chroma 2040, 2048, 2056);
    a band owns 16 window rows (h = 68 at the edge: 64, 68, 72; for chroma 128,
    136, 144);
  planes 16-byte aligned with padded strides, and one byte off alignment with
  odd strides inside noise-filled guards; a batch one larger than a launch's
  pair cap; a non-null stream; pixels the contract does not read; the sign
- the decoder (thor_dec_frame_ssim) and the encoder (thor_enc_recon_ssim)
  against the model on the frames they read back, their argument errors, and
  the coded bytes with and without the call
- scaler -> scaler -> SSIM chained on one stream"""
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

import ssim_model as M  # noqa: E402
from dev_frames import _dims, _frame, _random_planes, _side_context, dev  # noqa: E402, F401

pytestmark = pytest.mark.gpu

SSIM_INL = 8  # pairs per launch (thor_amd/csrc/ssim.hip)


CONTENT = ["random", "noise", "identical", "inverted", "constant", "step"]


def _content(w, h):
    """[(a, b)] in CONTENT's order: frames as plane triples."""
    rng = np.random.default_rng(w * 31 + h)
    a = _random_planes(w, h, w * 1000 + h)
    noisy = [np.clip(p.astype(np.int16) + rng.integers(-2, 3, p.shape), 0, 255).astype(np.uint8) for p in a]
    zero = [np.zeros_like(p) for p in a]
    step_a, step_b = [], []
    for p in a:  # a vertical step (left dark, right bright), a pixel further right in b
        x = np.arange(p.shape[1])[None, :].repeat(p.shape[0], 0)
        step_a.append(np.where(x < p.shape[1] // 2, 16, 235).astype(np.uint8))
        step_b.append(np.where(x < p.shape[1] // 2 + 1, 16, 235).astype(np.uint8))
    return [(a, _random_planes(w, h, w * 2000 + h)), (a, noisy), (a, [p.copy() for p in a]), (a, [255 - p for p in a]),
            (zero, [np.full_like(p, 255) for p in a]), (step_a, step_b)]


_MODEL = {}


def _want(w, h):
    """The model's sums of _content(w, h), computed once per size."""
    if (w, h) not in _MODEL:
        _MODEL[(w, h)] = [M.frame_sums(a, b) for a, b in _content(w, h)]
    return _MODEL[(w, h)]


NAMED = [(16, 16), (24, 16), (16, 24), (18, 22), (40, 24), (72, 40), (264, 36), (1048, 20), (16, 300)]
EDGES = [(1008, 20), (1012, 20), (1016, 20), (2016, 16), (2024, 16), (2032, 16),  # tile
         (1020, 16), (1024, 16), (1028, 16), (2040, 16), (2048, 16), (2056, 16),  # branch-free path
         (24, 64), (24, 68), (24, 72), (24, 128), (24, 136), (24, 144)]           # band


@pytest.mark.parametrize("w,h", NAMED + EDGES)
@pytest.mark.parametrize("layout", ["padded16", "off_by_one"])
def test_ssim_primitive_against_model(dev, w, h, layout):
    """padded16: planes 16-byte aligned, strides rounded up to 16 and one 16 more (16-byte loads); off_by_one:
    every plane one byte past alignment with odd strides (the dword path).  All six kinds of content in one call."""
    from thor_amd.encoder import ssim_i420

    cw = w // 2
    sy, sc, off = {"padded16": ((w + 15) // 16 * 16 + 16, (cw + 15) // 16 * 16 + 16, 0),
                   "off_by_one": (w + 3, cw + 5, 1)}[layout]
    pairs = _content(w, h)
    pa = [_frame(dev, a, sy, sc, off) for a, _ in pairs]
    pb = [_frame(dev, b, sy + (0 if layout == "padded16" else 2), sc, off) for _, b in pairs]
    got = ssim_i420(pa, pb, w, h)
    want = _want(w, h)
    assert got.dtype == np.int64 and got.shape == (len(CONTENT), 3)
    for name, g, x in zip(CONTENT, got.tolist(), want):
        assert g == x, (w, h, layout, name, g, x)
    nw = [M.windows(pw, ph) for pw, ph in _dims(w, h)]
    assert got[CONTENT.index("identical")].tolist() == [n * M.ONE for n in nw]
    assert got[CONTENT.index("constant")].tolist() == [n * 1677 for n in nw]


def test_ssim_signed_accumulation(dev):
    """Inverted content at 72 x 40: the sums are negative and equal the model's."""
    from thor_amd.encoder import ssim_from_sums, ssim_i420

    w, h = 72, 40
    a, b = _content(w, h)[CONTENT.index("inverted")]
    got = ssim_i420([_frame(dev, a, w, w // 2, 0)], [_frame(dev, b, w, w // 2, 0)], w, h)[0].tolist()
    assert got == M.frame_sums(a, b) and all(s < 0 for s in got), got
    y, u, v, al = ssim_from_sums(got, w, h)
    assert [y, u, v] == [M.ssim(s, pw, ph) for s, (pw, ph) in zip(got, _dims(w, h))] and al == (4 * y + u + v) / 6
    assert -1 <= y < 0


def test_ssim_ignores_the_remainder_pixels(dev):
    """18 x 22: luma columns 16, 17 and rows 20, 21 and chroma column 8 and rows 8..10 are outside every block.
    Two pairs that differ only there give equal sums."""
    from thor_amd.encoder import ssim_i420

    w, h = 18, 22
    a, b = _random_planes(w, h, 5), _random_planes(w, h, 6)
    a2, b2 = [p.copy() for p in a], [p.copy() for p in b]
    rng = np.random.default_rng(9)
    for p in a2 + b2:
        ph, pw = p.shape
        p[:, pw & ~3:] = rng.integers(0, 256, (ph, pw & 3), dtype=np.uint8)
        p[ph & ~3:, :] = rng.integers(0, 256, (ph & 3, pw), dtype=np.uint8)
    assert any((x != y).any() for x, y in zip(a + b, a2 + b2))
    got = ssim_i420([_frame(dev, a, w + 3, w // 2 + 5, 1), _frame(dev, a2, w + 3, w // 2 + 5, 1)],
                    [_frame(dev, b, w, w // 2, 0), _frame(dev, b2, w, w // 2, 0)], w, h).tolist()
    assert got[0] == got[1] == M.frame_sums(a, b)


@pytest.mark.parametrize("stream", ["null", "own"])
def test_ssim_batch_past_one_launch(dev, stream):
    """SSIM_INL + 1 pairs, every pair different: each pair's own sums, in order, on the null stream and on a
    stream of its own (a decoder context's)."""
    from thor_amd.encoder import ssim_i420

    n, (w, h) = SSIM_INL + 1, (40, 24)
    fa = [_random_planes(w, h, 10 * i + 1) for i in range(n)]
    fb = [[np.clip(p.astype(np.int16) + (i - 4) * 3, 0, 255).astype(np.uint8) for p in fa[i]] for i in range(n)]
    want = [M.frame_sums(x, y) for x, y in zip(fa, fb)]
    assert len({tuple(s) for s in want}) == n
    pa, pb = [_frame(dev, x, w, w // 2, 0) for x in fa], [_frame(dev, y, w + 3, w // 2 + 5, 1) for y in fb]
    if stream == "null":
        got = ssim_i420(pa, pb, w, h)
    else:
        ctx = _side_context()
        try:
            assert ctx.stream()
            got = ssim_i420(pa, pb, w, h, stream=ctx.stream(), wait=ctx.sync)
        finally:
            ctx.close()
    assert got.tolist() == want


def test_decoder_frame_ssim(dev, streams):
    """Two frames of cif_low.bit: GpuDecoder.ssim against an uploaded source equals the model on read()'s bytes;
    a frame number the ring does not hold gives THOR_ERR_REF."""
    from thor_amd import lib as L
    from thor_amd import synth
    from thor_amd.bitstream import parse_stream
    from thor_amd.decoder import GpuDecoder
    from thor_amd.encoder import yuv_planes

    meta = streams["cif_low"]
    w, h = meta["width"], meta["height"]
    with open(os.path.join(GOLD, "cif_low.bit"), "rb") as f:
        seq, frames = parse_stream(f.read())
    frames = frames[:2]
    src = synth.synth_frames(w, h, len(frames), meta["seed"], workers=1).reshape(len(frames), -1)
    dec = GpuDecoder(seq)
    try:
        for fr in frames:
            dec.decode(dec.upload(fr))
            o = src[fr.frame_num]
            planes = (o[:w * h].reshape(h, w), o[w * h:w * h * 5 // 4].reshape(h // 2, w // 2),
                      o[w * h * 5 // 4:].reshape(h // 2, w // 2))
            got = dec.ssim(fr.frame_num, yuv_planes(dev.put(o), w, h))
            want = M.frame_sums(planes, dec.read(fr.frame_num))
            assert list(got) == want and 0 < want[0] < M.windows(w, h) * M.ONE, (fr.frame_num, got, want)
        out = dev.put(np.zeros(3, np.int64))
        p = yuv_planes(dev.put(src[0]), w, h)
        assert dec.lib.thor_dec_frame_ssim(dec.h, 99, C.byref(p), out) == L.THOR_ERR_REF
        assert dec.lib.thor_dec_frame_ssim(dec.h, frames[-1].frame_num, C.byref(p), out) == L.THOR_OK
        dec.sync()
    finally:
        dec.close()


def test_encoder_recon_ssim(dev):
    """Two frames of the 40 x 24 matrix case: recon_ssim against the input equals the model on
    thor_enc_read_recon's bytes, the coded bytes equal those of a run without the call, and the call is an
    argument error before the first frame and between thor_enc_frames_begin and _end."""
    from thor_amd import lib as L
    from thor_amd import synth
    from thor_amd.encoder import GpuEncoder, encode_batch_begin, encode_batch_end, params_for, yuv_planes

    with open(os.path.join(GOLD, "quality.json")) as f:
        m = json.load(f)["low_40x24"]
    w, h = m["width"], m["height"]
    assert (w, h) == (40, 24)
    seq = synth.synth_frames(w, h, m["skip"] + m["frames"], m["seed"], workers=1)
    src = seq.reshape(-1, w * h * 3 // 2)

    def run(measure):
        enc = GpuEncoder(params_for(m["config"], w, h, m["frames"], m["extra"]))
        chunks = []
        try:
            enc.upload_sequence(seq)
            out = dev.put(np.zeros(3, np.int64))
            p0 = yuv_planes(dev.put(src[0]), w, h)
            if measure:
                assert enc.lib.thor_enc_recon_ssim(enc.h, C.byref(p0), out) == L.THOR_ERR_ARG  # no frame has ended
            for _ in range(2):
                o = src[enc.lib.thor_enc_next_input(enc.h)]
                chunks.append(bytes(enc.encode_next()))
                if not measure:
                    continue
                got = enc.recon_ssim(yuv_planes(dev.put(o), w, h))
                rec = [np.empty((ph, pw), np.uint8) for pw, ph in _dims(w, h)]
                L.check(enc.lib.thor_enc_read_recon(enc.h, *[r.ctypes.data for r in rec]), "thor_enc_read_recon")
                planes = (o[:w * h].reshape(h, w), o[w * h:w * h * 5 // 4].reshape(h // 2, w // 2),
                          o[w * h * 5 // 4:].reshape(h // 2, w // 2))
                want = M.frame_sums(planes, rec)
                assert list(got) == want and want[0] > 0, (got, want)
            if measure:
                encode_batch_begin([enc])
                rc = enc.lib.thor_enc_recon_ssim(enc.h, C.byref(p0), out)
                chunks.append(bytes(encode_batch_end([enc])[0]))
                assert rc == L.THOR_ERR_ARG  # a batch was in flight
                assert enc.lib.thor_enc_recon_ssim(enc.h, C.byref(p0), out) == L.THOR_OK
                L.check(enc.lib.thor_enc_read_recon(enc.h, None, None, None), "thor_enc_read_recon")  # (waits)
            else:
                chunks.append(bytes(enc.encode_next()))
        finally:
            enc.close()
        return chunks

    assert m["frames"] >= 3
    with_call, without = run(True), run(False)
    assert with_call == without and all(len(c) > 4 for c in without)


def test_ladder_composition(dev):
    """A 64 x 48 source scaled down to 32 x 24 and back up with the device scaler, then thor_ssim_i420 against
    the source, all on one stream: the sums equal the model on the same bytes read back."""
    from thor_amd.encoder import ssim_i420
    from thor_amd.scale import Scaler, i420_planes

    w, h, w2, h2 = 64, 48, 32, 24
    fs = w * h * 3 // 2
    src = np.concatenate([p.ravel() for p in _random_planes(w, h, 77)])
    # (smooth the noise a little so the round trip is not pure decorrelation)
    src = ((src.astype(np.uint16) + np.roll(src, 1) + np.roll(src, 2) + np.roll(src, 3)) // 4).astype(np.uint8)
    d_src, d_small, d_back = dev.put(src), dev.put(np.zeros(w2 * h2 * 3 // 2, np.uint8)), dev.put(np.zeros(fs, np.uint8))
    ctx = _side_context()
    down, up = Scaler(w, h, w2, h2), Scaler(w2, h2, w, h)
    try:
        st = ctx.stream()
        assert st
        down.run_frames(d_src, d_small, 1, st)
        up.run_frames(d_small, d_back, 1, st)
        got = ssim_i420([i420_planes(d_src, w, h)], [i420_planes(d_back, w, h)], w, h, stream=st, wait=ctx.sync)[0].tolist()
        back = dev.get(d_back, fs)
    finally:
        down.close()
        up.close()
        ctx.close()

    def planes(x):
        return (x[:w * h].reshape(h, w), x[w * h:w * h * 5 // 4].reshape(h // 2, w // 2),
                x[w * h * 5 // 4:].reshape(h // 2, w // 2))

    want = M.frame_sums(planes(src), planes(back))
    assert got == want and (back != src).any() and want[0] < M.windows(w, h) * M.ONE, (got, want)
