"""Frame scaling on the device against the Python model of the contract
(tests/scale_model.py), bit for bit: both filters, shrinking and enlarging,
aligned and unaligned frames with guarded padding, clamping content, batches,
streams, argument rejection against a live scaler, and the decoder's and the
encoder's scaled surfaces.  No torch in this process: device buffers go through
thor_dev_alloc / thor_h2d / thor_d2h."""
import ctypes as C

import numpy as np
import pytest

import scale_model as M
from conftest import trace_path
from thor_amd import lib as L

pytestmark = pytest.mark.gpu

# (sw, sh, dw, dh): a source shorter than the taps enlarged 8x; 8:1 with 33 taps below one tile; the identity;
# down on one axis and up on the other; a ragged source over several tiles and row bands; a non-integer ratio
# with a ragged last tile; 2:1; 1:2
PAIRS = [(2, 2, 16, 16), (16, 16, 2, 2), (8, 8, 8, 8), (40, 24, 24, 40), (130, 66, 352, 288), (352, 288, 130, 66),
         (352, 288, 176, 144), (136, 72, 272, 144)]
FILTERS = [L.THOR_SCALE_BILINEAR, L.THOR_SCALE_BICUBIC]
GUARD = 0xA5
LEAD = 32  # guard bytes in front of and behind every plane


class DevBuf:
    def __init__(self, a):
        a = np.ascontiguousarray(a)
        self.lib, self.shape, self.dtype, self.nbytes = L.load(), a.shape, a.dtype, a.nbytes
        self.ptr = self.lib.thor_dev_alloc(max(a.nbytes, 16))
        assert self.ptr
        assert self.lib.thor_h2d(self.ptr, a.ctypes.data, a.nbytes) == 0

    def numpy(self):
        out = np.empty(self.shape, self.dtype)
        assert self.lib.thor_d2h(out.ctypes.data, self.ptr, self.nbytes) == 0  # (waits for the null stream)
        return out

    def __del__(self):
        if self.ptr:
            self.lib.thor_dev_free(self.ptr)
            self.ptr = None


class Yuv:
    """An I420 frame in three guarded device buffers.  ragged: odd luma stride,
    padded chroma stride, planes 1 byte off 16-byte alignment; pad: more row
    padding on top (batches: another stride per image)."""

    def __init__(self, W, H, ragged, planes=None, pad=0):
        self.W, self.H = W, H
        self.sy = W + (5 if ragged else 0) + pad
        self.sc = W // 2 + (3 if ragged else 0) + pad
        self.off = LEAD + (1 if ragged else 0)
        self.dims = ((W, H, self.sy), (W // 2, H // 2, self.sc), (W // 2, H // 2, self.sc))
        self.host = []
        for k, (w, h, s) in enumerate(self.dims):
            b = np.full(self.off + s * h + LEAD, GUARD, np.uint8)
            if planes is not None:
                b[self.off:self.off + s * h].reshape(h, s)[:, :w] = planes[k]
            self.host.append(b)
        self.dev = [DevBuf(b) for b in self.host]

    def desc(self):
        assert all(d.ptr % 16 == 0 for d in self.dev)
        p = [d.ptr + self.off for d in self.dev]
        return L.ThorYuvPlanes(p[0], p[1], p[2], self.sy, self.sc)

    def expect(self, planes):
        """The host buffers as they must look after `planes` was written: guards intact."""
        out = []
        for k, (w, h, s) in enumerate(self.dims):
            b = self.host[k].copy()
            b[self.off:self.off + s * h].reshape(h, s)[:, :w] = planes[k]
            out.append(b)
        return out

    def back(self):
        return [d.numpy() for d in self.dev]


class Scaler:
    def __init__(self, sw, sh, dw, dh, f):
        self.lib = L.load()
        self.h = self.lib.thor_scaler_create(sw, sh, dw, dh, f, 0)
        assert self.h, L.create_error("thor_scaler_create")

    def run(self, srcs, dsts, stream=None):
        n = len(srcs)
        return self.lib.thor_scale_i420(self.h, (L.ThorYuvPlanes * n)(*[s.desc() for s in srcs]),
                                        (L.ThorYuvPlanes * n)(*[d.desc() for d in dsts]), n, stream)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.lib.thor_scaler_destroy(self.h)
        self.h = None


def _same(got, want, what):
    for k, (g, w) in enumerate(zip(got, want)):
        if not np.array_equal(g, w):
            bad = np.flatnonzero(g != w)
            raise AssertionError("%s, plane %d: %d bytes differ, first at %s (got %s, want %s)"
                                 % (what, k, bad.size, bad[:6].tolist(), g[bad[:6]].tolist(), w[bad[:6]].tolist()))


def _contents(sw, sh):
    """Seeded random bytes; a 0 / 255 checkerboard and a 0 / 255 step edge (the cubic's overshoot clamps at both ends)."""
    rng = np.random.default_rng(1000 * sw + sh)
    dims = ((sh, sw), (sh // 2, sw // 2), (sh // 2, sw // 2))
    yield "random", [rng.integers(0, 256, d, dtype=np.uint8) for d in dims]
    yield "checkerboard", [(((np.arange(h)[:, None] + np.arange(w)[None, :]) & 1) * 255).astype(np.uint8) for h, w in dims]
    yield "step", [np.repeat((np.arange(w)[None, :] >= max(w // 2, 1)) * 255, h, axis=0).astype(np.uint8) for h, w in dims]


@pytest.mark.parametrize("f", FILTERS)
@pytest.mark.parametrize("pair", PAIRS)
def test_scaled_frames_match_the_model(pair, f):
    """The whole destination buffers are compared, so row padding and the bytes
    around every plane keep their guard pattern."""
    sw, sh, dw, dh = pair
    with Scaler(sw, sh, dw, dh, f) as sc:
        for name, planes in _contents(sw, sh):
            want = M.scale_i420(*planes, dw, dh, f)
            for ragged in (False, True):
                src, dst = Yuv(sw, sh, ragged, planes), Yuv(dw, dh, ragged)
                assert sc.run([src], [dst]) == 0
                _same(dst.back(), dst.expect(want), "%s %s filter %d ragged %d" % (pair, name, f, ragged))
                _same(src.back(), src.host, "source of %s" % (pair,))


@pytest.mark.parametrize("n", [3, L.THOR_SCALE_LAUNCH_IMAGES + 1])
def test_batches(n):
    """n = 3: unrelated allocations, another stride per image; launch cap + 1: the batch splits across launches."""
    sw, sh, dw, dh = 40, 24, 24, 40
    rng = np.random.default_rng(n)
    planes = [[rng.integers(0, 256, d, dtype=np.uint8) for d in ((sh, sw), (sh // 2, sw // 2), (sh // 2, sw // 2))]
              for _ in range(n)]
    for f in FILTERS:
        with Scaler(sw, sh, dw, dh, f) as sc:
            srcs = [Yuv(sw, sh, bool(i % 2), planes[i], pad=3 * (i % 3)) for i in range(n)]
            dsts = [Yuv(dw, dh, bool((i // 2) % 2), pad=2 * (i % 4)) for i in range(n)]
            assert sc.run(srcs, dsts) == 0
            for i in range(n):
                _same(dsts[i].back(), dsts[i].expect(M.scale_i420(*planes[i], dw, dh, f)), "image %d of %d" % (i, n))


def test_second_stream_and_second_call():
    """The same call twice, and once on a non-null stream (a decoder context's own), gives the same bytes."""
    from thor_amd.decoder import GpuDecoder
    from thor_amd.trace import load_trace

    sw, sh, dw, dh = 130, 66, 352, 288
    planes = next(_contents(sw, sh))[1]
    want = M.scale_i420(*planes, dw, dh, L.THOR_SCALE_BICUBIC)
    ctx = GpuDecoder(load_trace(trace_path("cif_low"))[0])
    try:
        side = ctx.stream()
        assert side
        with Scaler(sw, sh, dw, dh, L.THOR_SCALE_BICUBIC) as sc:
            src = Yuv(sw, sh, True, planes)
            a, b, c = (Yuv(dw, dh, True) for _ in range(3))
            assert sc.run([src], [a]) == 0 and sc.run([src], [b]) == 0
            _same(a.back(), a.expect(want), "first call")
            _same(b.back(), a.expect(want), "second call")
            assert sc.run([src], [c], side) == 0
            ctx.sync()
            _same(c.back(), c.expect(want), "second stream")
    finally:
        ctx.close()


def test_rejection_with_a_live_scaler():
    """NULL planes, strides below a row and n out of range are refused before any launch: the guards and
    the destination stay as they were."""
    lib = L.load()
    sw, sh, dw, dh = 40, 24, 24, 40
    with Scaler(sw, sh, dw, dh, L.THOR_SCALE_BILINEAR) as sc:
        src, dst = Yuv(sw, sh, False, next(_contents(sw, sh))[1]), Yuv(dw, dh, False)
        good_s, good_d = src.desc(), dst.desc()

        def call(s, d, n=1):
            return lib.thor_scale_i420(sc.h, (L.ThorYuvPlanes * 1)(s), (L.ThorYuvPlanes * 1)(d), n, None)

        def edit(desc, **kw):
            v = {k: getattr(desc, k) for k in ("y", "u", "v", "stride_y", "stride_c")}
            v.update(kw)
            return L.ThorYuvPlanes(v["y"], v["u"], v["v"], v["stride_y"], v["stride_c"])

        for k in ("y", "u", "v"):
            assert call(edit(good_s, **{k: None}), good_d) == L.THOR_ERR_ARG
            assert call(good_s, edit(good_d, **{k: None})) == L.THOR_ERR_ARG
        assert call(edit(good_s, stride_y=sw - 1), good_d) == L.THOR_ERR_ARG
        assert call(edit(good_s, stride_c=sw // 2 - 1), good_d) == L.THOR_ERR_ARG
        assert call(good_s, edit(good_d, stride_y=dw - 1)) == L.THOR_ERR_ARG
        assert call(good_s, edit(good_d, stride_c=dw // 2 - 1)) == L.THOR_ERR_ARG
        for n in (0, -3, 65536):
            assert call(good_s, good_d, n) == L.THOR_ERR_ARG
        assert lib.thor_scale_i420(sc.h, None, (L.ThorYuvPlanes * 1)(good_d), 1, None) == L.THOR_ERR_ARG
        assert lib.thor_scale_i420(sc.h, (L.ThorYuvPlanes * 1)(good_s), None, 1, None) == L.THOR_ERR_ARG
        _same(dst.back(), dst.host, "destination after refused calls")
    assert not lib.thor_scaler_create(sw, sh, dw, dh, 0, 4096)  # no such device
    assert L.create_error("thor_scaler_create").code == L.THOR_ERR_ARG


def test_decoder_scaled_frames():
    """thor_dec_frame_scaled / GpuDecoder.read_scaled of a resident frame equal the model applied to
    GpuDecoder.read's planes; THOR_ERR_REF for a frame that is not resident, THOR_ERR_ARG for a scaler of
    another source size."""
    from thor_amd.decoder import GpuDecoder
    from thor_amd.trace import load_trace

    seq, frames = load_trace(trace_path("cif_low"))
    W, H = seq.width, seq.height
    dw, dh = 176, 144
    dec = GpuDecoder(seq)
    try:
        with Scaler(W, H, dw, dh, L.THOR_SCALE_BICUBIC) as sc, Scaler(W + 2, H, dw, dh, L.THOR_SCALE_BICUBIC) as other:
            for fr in frames[:2]:
                dec.decode(dec.upload(fr))
                y, u, v = dec.read(fr.frame_num)
                want = M.scale_i420(y, u, v, dw, dh, L.THOR_SCALE_BICUBIC)
                dst = Yuv(dw, dh, True)
                d = dst.desc()
                assert dec.lib.thor_dec_frame_scaled(dec.h, fr.frame_num, sc.h, C.byref(d)) == 0
                dec.sync()
                _same(dst.back(), dst.expect(want), "thor_dec_frame_scaled frame %d" % fr.frame_num)
                assert dec.read_scaled(fr.frame_num, dw, dh) == b"".join(p.tobytes() for p in want)
                small = M.scale_i420(y, u, v, 88, 72, L.THOR_SCALE_BILINEAR)
                assert dec.read_scaled(fr.frame_num, 88, 72, "bilinear") == b"".join(p.tobytes() for p in small)
            assert len(dec._scalers) == 2
            never = max(fr.frame_num for fr in frames) + 100
            dst = Yuv(dw, dh, False)
            d = dst.desc()
            assert dec.lib.thor_dec_frame_scaled(dec.h, never, sc.h, C.byref(d)) == L.THOR_ERR_REF
            assert dec.lib.thor_dec_frame_scaled(dec.h, frames[0].frame_num, other.h, C.byref(d)) == L.THOR_ERR_ARG
            with pytest.raises(RuntimeError, match="status -4"):
                dec.read_scaled(never, dw, dh)
            dec.sync()
            _same(dst.back(), dst.host, "destination after refused calls")
    finally:
        dec.close()
    assert dec._scalers == {}


def test_encoder_scaled_input():
    """A 272x144 clip through set_input_scaled into a 136x72 encoder gives, byte for byte, the .bit the
    same encoder produces from the model-scaled frames through upload_sequence, and the same per-frame SSE
    against its input."""
    from thor_amd import synth
    from thor_amd.encoder import GpuEncoder, params_for

    lib = L.load()
    lib.thor_enc_debug_stall(-1, 20000)  # a wedged launch gives up after 20 s instead of 5 minutes
    sw, sh, W, H, n = 272, 144, 136, 72, 3
    cfg = "config_LDB_low_complexity.txt"
    clip = synth.synth_frames(sw, sh, n, 5, workers=1)
    want_in = M.scale_frames(clip, sw, sh, W, H, M.BICUBIC)
    src = DevBuf(clip)
    a, b = GpuEncoder(params_for(cfg, W, H, n)), GpuEncoder(params_for(cfg, W, H, n))
    try:
        a.measure_quality()
        b.measure_quality()
        a.set_input_scaled(src.ptr, n, sw, sh, filter="bicubic")
        b.upload_sequence(want_in)
        for k in range(n):
            assert a.encode_next() == b.encode_next(), k
            assert a.sse() == b.sse(), k
        got_in = np.empty(want_in.shape, np.uint8)
        assert lib.thor_d2h(got_in.ctypes.data, a.seq_dev, got_in.nbytes) == 0
        assert np.array_equal(got_in, want_in)
        with pytest.raises(ValueError):
            a.set_input_scaled(src.ptr, n, 2048, sh)  # more than 8:1
    finally:
        lib.thor_enc_debug_stall(-1, 0)
        a.close()
        b.close()


def test_torch_surface_in_a_child_process():
    """thor_amd.scale.scale_i420 with torch tensors and streams (tests/scale_torch_case.py).  In a child
    process: torch's HIP runtime has to come up before the library's, and in this process the library's is
    already up."""
    import os
    import subprocess
    import sys

    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-u", os.path.join(here, "scale_torch_case.py")], capture_output=True, text=True,
                       timeout=240, cwd=os.path.dirname(here))
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert r.stdout.strip().splitlines()[-1] == "ok: scale_i420", r.stdout[-1000:]
