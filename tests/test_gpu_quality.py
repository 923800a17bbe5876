"""GPU: frame quality measured on the device (k_sse_i420, thor_amd/csrc/quality.hip)
against numpy and against the reference's own numbers, tests/golden/quality.json
(tools/make_quality_goldens.py: per coded frame the exact Y / U / V sums of
squared errors between the input frame and the reference encoder's
reconstruction, and the PSNR strings the reference printed).

- the primitive (thor_sse_i420) against numpy in uint64: sizes below one pass,
  not a multiple of 16, several bands and blocks; padded and odd strides; planes
  one byte off 16-byte alignment; several pairs per call; totals past 2^32; the
  wrap case of the three-dot form
- the encoder frame by frame (thor_enc_frame), in pipelined batches
  (thor_enc_frames_begin / _end, two in flight) and in the sequence launch
  (thor_enc_seq_*): every frame's sums equal the reference's, its PSNR prints
  as the reference printed it, and the coded bytes do not change
- the decoder (thor_dec_frame_sse) against numpy on the frames it reads back"""
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

from dev_frames import _frame, _random_planes, dev  # noqa: E402, F401

pytestmark = pytest.mark.gpu

with open(os.path.join(GOLD, "quality.json")) as _f:
    TABLE = json.load(_f)
CASES = sorted(c for c in TABLE if c != "low_40x24_b")
FMT = ("%10.4f", "%8.4f", "%8.4f")  # enc/mainenc.c:536-540


def _interp_ref(meta):
    from thor_amd import configs

    fl = configs.flags(meta["config"], meta["width"], meta["height"], meta["frames"], meta["extra"])
    return int(dict(zip(fl[0::2], fl[1::2])).get("-interp_ref", "0"))


# the sequence launch refuses contexts with interpolated references (thor_enc_frames codes them)
NO_INTERP = [c for c in CASES if not _interp_ref(TABLE[c])]


def test_cases():
    assert len(CASES) == 8 and sorted(set(CASES) - set(NO_INTERP)) == ["hdb16_n9"]


@pytest.fixture(autouse=True)
def _bounded_waits():
    """A wedged launch (per frame or sequence) gives up after 20 s (reported as
    a device error) instead of the 5-minute default."""
    from thor_amd import lib as L

    lib = L.load()
    lib.thor_enc_debug_stall(-1, 20000)
    yield
    lib.thor_enc_debug_stall(-1, 0)


# ---- the primitive ---------------------------------------------------------------------------------------------
def _np_sse(a, b):
    return [int(((x.astype(np.int64) - y.astype(np.int64)) ** 2).sum()) for x, y in zip(a, b)]


SIZES = [(8, 8), (40, 24), (136, 72), (1920, 8)]


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("layout", ["tight", "padded16", "odd_stride", "off_by_one"])
def test_sse_primitive_against_numpy(dev, w, h, layout):
    """tight: stride = width (16-byte loads where the width allows them: 1920 x 8); padded16: strides rounded up
    to 16 and one 16 more (16-byte loads with a short last pass per row: 8, 40, 136 wide); odd_stride: width + 3
    and width / 2 + 5 (rows at every alignment: the dword path); off_by_one: 16-byte strides, every plane one
    byte past alignment (the dword path at a fixed misalignment)."""
    from thor_amd.encoder import sse_i420

    a, b = _random_planes(w, h, 1000 + w), _random_planes(w, h, 2000 + h)
    cw = w // 2
    sy, sc, off = {"tight": (w, cw, 0), "padded16": ((w + 15) // 16 * 16 + 16, (cw + 15) // 16 * 16 + 16, 0),
                   "odd_stride": (w + 3, cw + 5, 0),
                   "off_by_one": ((w + 15) // 16 * 16, (cw + 15) // 16 * 16, 1)}[layout]
    # (the two frames of a pair have their own strides: b keeps the tight one unless the layout is about alignment)
    pa = _frame(dev, a, sy, sc, off)
    pb = _frame(dev, b, sy, sc, off) if layout in ("padded16", "off_by_one") else _frame(dev, b, w, cw, 0)
    got = sse_i420([pa], [pb], w, h)
    assert got.dtype == np.uint64 and got.tolist() == [_np_sse(a, b)], (w, h, layout)


def test_sse_primitive_pairs_do_not_leak(dev):
    """n = 3 pairs of distinct content in one call, and 11 pairs (more than one launch's worth of kernel
    arguments): every pair's own sums, in order."""
    from thor_amd.encoder import sse_i420

    for n, (w, h) in ((3, (136, 72)), (11, (40, 24))):
        fa = [_random_planes(w, h, 10 * i + 1) for i in range(n)]
        fb = [_random_planes(w, h, 10 * i + 2) for i in range(n)]
        want = [_np_sse(x, y) for x, y in zip(fa, fb)]
        assert len({tuple(s) for s in want}) == n
        got = sse_i420([_frame(dev, x, w, w // 2, 0) for x in fa], [_frame(dev, y, w, w // 2, 0) for y in fb], w, h)
        assert got.tolist() == want, n


def test_sse_primitive_totals_past_32_bits_and_the_wrap_case(dev):
    """1024 x 1024 of all 0 against all 255: the luma total, 2^20 * 255^2, is above 2^32, and every 32-bit
    partial kept past 66 051 pixels would overflow.  All 255 against all 255: the three dot products of the
    inner loop each wrap, their combination must be exactly 0."""
    from thor_amd.encoder import sse_i420

    w = h = 1024
    zero = [np.zeros((ph, pw), np.uint8) for pw, ph in ((w, h), (w // 2, h // 2), (w // 2, h // 2))]
    full = [np.full_like(p, 255) for p in zero]
    pz, pf, pf2 = _frame(dev, zero, w, w // 2, 0), _frame(dev, full, w, w // 2, 0), _frame(dev, full, w, w // 2, 0)
    got = sse_i420([pz, pf, pf], [pf, pf2, pz], w, h).tolist()
    big = [w * h * 65025, w * h // 4 * 65025, w * h // 4 * 65025]
    assert big[0] > 2 ** 32
    assert got == [big, [0, 0, 0], big]


# ---- the encoder ------------------------------------------------------------------------------------------------
def _chunks(b):
    out, o = [], 0
    while o < len(b):
        n = int.from_bytes(b[o:o + 4], "big")
        out.append(b[o:o + 4 + n])
        o += 4 + n
    return out


def _golden_chunks(name):
    """The reference's chunks of a matrix case (None for the cases only quality.json has)."""
    if not TABLE[name]["matrix"]:
        return None
    with open(os.path.join(GOLD, "matrix_%s.bit" % name), "rb") as f:
        return _chunks(f.read())


_INPUT = {}


def _input(name):
    """The case's input sequence (the -skip frames leading), generated once per session."""
    from thor_amd import synth

    if name not in _INPUT:
        m = TABLE[name]
        _INPUT[name] = synth.synth_frames(m["width"], m["height"], m["skip"] + m["frames"], m["seed"], workers=1)
    return _INPUT[name]


def _encoder(name, measure=True):
    from thor_amd.encoder import GpuEncoder, params_for

    m = TABLE[name]
    enc = GpuEncoder(params_for(m["config"], m["width"], m["height"], m["frames"], m["extra"]))
    try:
        enc.upload_sequence(_input(name))
        if measure:
            enc.measure_quality()
    except Exception:
        enc.close()
        raise
    return enc


def _check_frame(name, i, sse, psnr):
    f = TABLE[name]["coded"][i]
    assert list(sse) == f["sse"], (name, i, f["type"], list(sse), f["sse"])
    assert [(fmt % v).strip() for fmt, v in zip(FMT, psnr)] == f["psnr"], (name, i, psnr, f["psnr"])


@pytest.mark.parametrize("name", CASES)
def test_encoder_frames_match_reference(name):
    """Frame by frame through thor_enc_frame: the sums, the printed PSNR, and -- with measurement on -- the
    reference's bytes."""
    meta, want = TABLE[name], _golden_chunks(name)
    enc = _encoder(name)
    try:
        assert enc.num_frames() == meta["frames"]
        for i, f in enumerate(meta["coded"]):
            assert enc.lib.thor_enc_next_input(enc.h) == f["input"], (name, i)
            got = enc.encode_next()
            _check_frame(name, i, enc.sse(), enc.psnr())
            if want is not None:
                assert bytes(got) == want[i], (name, i, len(got), len(want[i]))
    finally:
        enc.close()


def test_encoder_measurement_is_off_by_default():
    from thor_amd import lib as L

    enc = _encoder("low_8x8", measure=False)
    try:
        out = (C.c_uint64 * 3)()
        enc.encode_next()
        assert enc.lib.thor_enc_frame_sse(enc.h, out) == L.THOR_ERR_ARG  # off
        enc.measure_quality()
        assert enc.lib.thor_enc_frame_sse(enc.h, out) == L.THOR_ERR_ARG  # on, no frame ended with it on
        enc.encode_next()
        _check_frame("low_8x8", 1, enc.sse(), enc.psnr())
        enc.measure_quality(False)
        assert enc.lib.thor_enc_frame_sse(enc.h, out) == L.THOR_ERR_ARG
        enc.measure_quality()
        enc.reset()  # the sums go with the chunk
        assert enc.lib.thor_enc_frame_sse(enc.h, out) == L.THOR_ERR_ARG
        enc.encode_next()
        _check_frame("low_8x8", 0, enc.sse(), enc.psnr())
    finally:
        enc.close()


def test_encoder_batches_in_flight():
    """low_40x24 and the same size with another seed in one begin / end pipeline, two batches in flight: each
    context reports its own frame's sums, in order, and the bytes stay the reference's."""
    from thor_amd import lib as L
    from thor_amd.encoder import encode_batch_begin, encode_batch_end

    names = ["low_40x24", "low_40x24_b"]
    want = _golden_chunks("low_40x24")
    encs = [_encoder(n) for n in names]
    try:
        n = TABLE[names[0]]["frames"]
        assert n == TABLE[names[1]]["frames"] >= 3
        encode_batch_begin(encs)
        assert encs[0].lib.thor_enc_measure_sse(encs[0].h, 0) == L.THOR_ERR_ARG  # not with a batch in flight
        for i in range(n):
            if i + 1 < n:
                encode_batch_begin(encs)  # frame i + 1 enqueued before frame i is collected
            got = encode_batch_end(encs)
            for k, name in enumerate(names):
                _check_frame(name, i, encs[k].sse(), encs[k].psnr())
            assert bytes(got[0]) == want[i], i
    finally:
        for e in encs:
            e.close()


def test_encoder_batch_with_one_context_measuring():
    from thor_amd import lib as L
    from thor_amd.encoder import encode_batch

    names = ["low_40x24_b", "low_40x24"]
    want = _golden_chunks("low_40x24")
    encs = [_encoder(names[0], measure=False), _encoder(names[1])]
    try:
        out = (C.c_uint64 * 3)()
        for i in range(TABLE[names[1]]["frames"]):
            got = encode_batch(encs)
            assert encs[0].lib.thor_enc_frame_sse(encs[0].h, out) == L.THOR_ERR_ARG
            _check_frame(names[1], i, encs[1].sse(), encs[1].psnr())
            assert bytes(got[1]) == want[i], i
    finally:
        for e in encs:
            e.close()


def test_encoder_input_with_a_padded_stride(dev):
    """The input uploaded with orig_stride 64 > width 40 (chroma stride 32): the launch reads orig[i] with
    orig_stride[i], as the RD loop does."""
    from thor_amd import lib as L

    name = "low_40x24"
    meta, want = TABLE[name], _golden_chunks(name)
    w, h, s = meta["width"], meta["height"], 64
    src = _input(name).reshape(-1, w * h * 3 // 2)
    enc = _encoder(name)
    try:
        for i, f in enumerate(meta["coded"]):
            fr = src[f["input"]]
            y, u, v = fr[:w * h].reshape(h, w), fr[w * h:w * h * 5 // 4].reshape(h // 2, w // 2), fr[w * h * 5 // 4:].reshape(
                h // 2, w // 2)
            buf = np.full(s * h + (s // 2) * (h // 2) * 2, 0x5a, np.uint8)
            buf[:s * h].reshape(h, s)[:, :w] = y
            buf[s * h:s * h + (s // 2) * (h // 2)].reshape(h // 2, s // 2)[:, :w // 2] = u
            buf[s * h + (s // 2) * (h // 2):].reshape(h // 2, s // 2)[:, :w // 2] = v
            L.check(enc.lib.thor_enc_frame(enc.h, dev.put(buf), s), "thor_enc_frame")
            _check_frame(name, i, enc.sse(), enc.psnr())
            assert enc.chunk() == want[i], i
    finally:
        enc.close()


@pytest.mark.parametrize("name", NO_INTERP)
def test_sequence_launch_matches_reference(name):
    """Two copies per sequence launch: every frame's sums, accumulated inside the launch row by row, equal the
    reference's -- the frames whose reconstructions the launch overwrites included -- and the bytes do not change."""
    from thor_amd.encoder import SeqLaunch, psnr_i420

    meta, want = TABLE[name], _golden_chunks(name)
    encs = []
    try:
        for _ in range(2):
            encs.append(_encoder(name))
        s = SeqLaunch(encs)
        s.end()
        assert s.nf == meta["frames"]
        for i in range(2):
            for f in range(s.nf):
                sse = s.sse(i, f)
                _check_frame(name, f, sse, psnr_i420(sse, meta["width"], meta["height"]))
                if want is not None:
                    assert s.chunk(i, f) == want[f], (name, i, f)
            _check_frame(name, s.nf - 1, encs[i].sse(), encs[i].psnr())  # the last frame is the context's own too
    finally:
        for e in encs:
            e.close()


def test_sequence_launch_with_one_context_measuring():
    from thor_amd import lib as L
    from thor_amd.encoder import SeqLaunch, psnr_i420

    name = "ldb_skip3_hq3"
    want = _golden_chunks(name)
    encs = []
    try:
        encs = [_encoder(name, measure=False), _encoder(name)]
        s = SeqLaunch(encs)
        assert encs[1].lib.thor_enc_measure_sse(encs[1].h, 0) == L.THOR_ERR_ARG  # not with a launch in flight
        s.end()
        out = (C.c_uint64 * 3)()
        for f in range(s.nf):
            assert s.lib.thor_enc_seq_sse(encs[0].h, 0, f, out) == L.THOR_ERR_ARG
            _check_frame(name, f, s.sse(1, f), psnr_i420(s.sse(1, f), TABLE[name]["width"], TABLE[name]["height"]))
            assert s.chunk(0, f) == s.chunk(1, f) == want[f]
        assert s.lib.thor_enc_seq_sse(encs[0].h, 2, 0, out) == L.THOR_ERR_ARG
    finally:
        for e in encs:
            e.close()


# ---- the decoder -------------------------------------------------------------------------------------------------
def test_decoder_frame_sse(dev, streams):
    """cif_low.bit decoded from the bitstream: GpuDecoder.sse of each frame against a device-resident synthetic
    source equals numpy on read() of the same frame; a frame the ring has evicted gives THOR_ERR_REF."""
    from thor_amd import lib as L
    from thor_amd import synth
    from thor_amd.bitstream import parse_stream
    from thor_amd.decoder import GpuDecoder, ring_slots
    from thor_amd.encoder import yuv_planes

    meta = streams["cif_low"]
    w, h = meta["width"], meta["height"]
    with open(os.path.join(GOLD, "cif_low.bit"), "rb") as f:
        seq, frames = parse_stream(f.read())
    frames = frames[:6]
    src = synth.synth_frames(w, h, len(frames), meta["seed"], workers=1).reshape(len(frames), -1)
    slots = ring_slots(frames)
    assert slots < len(frames)  # so the first frame leaves the ring
    dec = GpuDecoder(seq, slots=slots)
    try:
        for fr in frames:
            dec.decode(dec.upload(fr))
            fn = fr.frame_num
            o = src[fn]
            planes = (o[:w * h].reshape(h, w), o[w * h:w * h * 5 // 4].reshape(h // 2, w // 2),
                      o[w * h * 5 // 4:].reshape(h // 2, w // 2))
            got = dec.sse(fn, yuv_planes(dev.put(o), w, h))
            want = _np_sse(planes, dec.read(fn))
            assert list(got) == want and want[0] > 0, (fn, got, want)
        out = dev.put(np.zeros(3, np.uint64))
        p = yuv_planes(dev.put(src[0]), w, h)
        assert dec.lib.thor_dec_frame_sse(dec.h, frames[0].frame_num, C.byref(p), out) == L.THOR_ERR_REF
        assert dec.lib.thor_dec_frame_sse(dec.h, frames[-1].frame_num, C.byref(p), out) == L.THOR_OK
        dec.sync()
    finally:
        dec.close()
