"""Colour conversion on the device against the numpy model of the contract
(tests/color_model.py), bit for bit: both directions, every format, matrix,
range and chroma mode, aligned and unaligned images with guarded padding,
batches, streams, the decoder's and encoder's RGB surfaces and torch interop."""
import ctypes as C
import hashlib
import itertools

import numpy as np
import pytest

import color_model as M
from conftest import trace_path
from thor_amd import lib as L

pytestmark = pytest.mark.gpu

# below one lane strip, one strip, a ragged last strip, more than one wave per row, several row bands
SIZES = [(2, 2), (4, 2), (6, 4), (8, 8), (40, 24), (130, 66), (352, 288)]
FORMATS = [L.THOR_RGB8_PACKED, L.THOR_RGB8_PLANAR, L.THOR_RGBF32_PLANAR]
PAIRS = [(0, 0), (0, 1), (1, 0), (1, 1)]
GUARD = 0xA5
LEAD = 32  # guard bytes in front of every buffer


class DevBuf:
    """A device buffer through the library's own helpers (thor_dev_alloc / thor_h2d / thor_d2h):
    no torch in this process -- torch's HIP runtime finds no GPU once the library's is up."""

    def __init__(self, a):
        a = np.ascontiguousarray(a)
        self.lib, self.shape, self.dtype, self.nbytes = L.load(), a.shape, a.dtype, a.nbytes
        self.ptr = self.lib.thor_dev_alloc(max(a.nbytes, 16))
        assert self.ptr
        assert self.lib.thor_h2d(self.ptr, a.ctypes.data, a.nbytes) == 0

    def data_ptr(self):
        return self.ptr

    def cpu(self):
        return self

    def numpy(self):
        out = np.empty(self.shape, self.dtype)
        assert self.lib.thor_d2h(out.ctypes.data, self.ptr, self.nbytes) == 0  # (waits for the null stream)
        return out

    def __del__(self):
        if self.ptr:
            self.lib.thor_dev_free(self.ptr)
            self.ptr = None


def _up(a):
    return DevBuf(a)


class Yuv:
    """Host image of an I420 frame in three guarded buffers: padded strides (odd
    for luma) and planes 1 byte off 16-byte alignment when `ragged`."""

    def __init__(self, W, H, ragged, planes=None, fill=None):
        self.W, self.H = W, H
        self.sy = W + (5 if ragged else 0)
        self.sc = W // 2 + (3 if ragged else 0)
        self.off = LEAD + (1 if ragged else 0)
        self.host = []
        for k, (w, h, s) in enumerate(((W, H, self.sy), (W // 2, H // 2, self.sc), (W // 2, H // 2, self.sc))):
            b = np.full(self.off + s * h + LEAD, GUARD if fill is None else fill, np.uint8)
            if planes is not None:
                b[self.off:self.off + s * h].reshape(h, s)[:, :w] = planes[k]
            self.host.append(b)
        self.dev = [_up(b) for b in self.host]

    def desc(self):
        p = [d.data_ptr() + self.off for d in self.dev]
        assert all(d.data_ptr() % 16 == 0 for d in self.dev)
        return L.ThorYuvPlanes(p[0], p[1], p[2], self.sy, self.sc)

    def expect(self, planes):
        """The host buffers as they must look after `planes` was written: guards intact."""
        out = []
        for k, (w, h, s) in enumerate(((self.W, self.H, self.sy), (self.W // 2, self.H // 2, self.sc),
                                       (self.W // 2, self.H // 2, self.sc))):
            b = self.host[k].copy()
            b[self.off:self.off + s * h].reshape(h, s)[:, :w] = planes[k]
            out.append(b)
        return out

    def back(self):
        return [d.cpu().numpy() for d in self.dev]


class Rgb:
    """Host image of an RGB image in a guarded buffer: padded row and plane
    strides and a pointer 1 byte (float: 4 bytes) off 16-byte alignment when
    `ragged`."""

    def __init__(self, W, H, fmt, ragged, pixels=None):
        self.W, self.H, self.fmt = W, H, fmt
        self.esz = 4 if fmt == L.THOR_RGBF32_PLANAR else 1
        self.row = 3 * W if fmt == L.THOR_RGB8_PACKED else W * self.esz
        self.rs = self.row + (8 if ragged else 0)
        self.ps = self.rs * H + (12 if ragged else 0)
        self.off = LEAD + ((4 if fmt == L.THOR_RGBF32_PLANAR else 1) if ragged else 0)
        body = self.rs * H if fmt == L.THOR_RGB8_PACKED else 3 * self.ps
        self.host = np.full(self.off + body + LEAD, GUARD, np.uint8)
        if pixels is not None:
            self.host = self.expect(pixels)
        self.dev = _up(self.host)

    def desc(self):
        assert self.dev.data_ptr() % 16 == 0
        return L.ThorImage(self.dev.data_ptr() + self.off, self.fmt, self.rs, self.ps)

    def expect(self, pixels):
        """pixels: (H, W, 3) uint8, or float32 for the float format."""
        b = self.host.copy()
        H, W = self.H, self.W
        if self.fmt == L.THOR_RGB8_PACKED:
            b[self.off:self.off + self.rs * H].reshape(H, self.rs)[:, :3 * W] = pixels.reshape(H, 3 * W)
        else:
            for k in range(3):
                o = self.off + k * self.ps
                b[o:o + self.rs * H].reshape(H, self.rs)[:, :self.row] = \
                    np.ascontiguousarray(pixels[..., k]).view(np.uint8).reshape(H, self.row)
        return b

    def back(self):
        return self.dev.cpu().numpy()


def _to_rgb(yuvs, rgbs, W, H, csc, stream=None):
    n = len(yuvs)
    rc = L.load().thor_i420_to_rgb((L.ThorYuvPlanes * n)(*[y.desc() for y in yuvs]),
                                   (L.ThorImage * n)(*[r.desc() for r in rgbs]), n, W, H, C.byref(csc), stream)
    assert rc == 0, rc


def _from_rgb(rgbs, yuvs, W, H, csc, stream=None):
    n = len(yuvs)
    rc = L.load().thor_rgb_to_i420((L.ThorImage * n)(*[r.desc() for r in rgbs]),
                                   (L.ThorYuvPlanes * n)(*[y.desc() for y in yuvs]), n, W, H, C.byref(csc), stream)
    assert rc == 0, rc


def _planes(rng, W, H):
    return [rng.integers(0, 256, s, dtype=np.uint8) for s in ((H, W), (H // 2, W // 2), (H // 2, W // 2))]


def _pixels(rng, W, H, fmt):
    if fmt != L.THOR_RGBF32_PLANAR:
        return rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    px = rng.uniform(-0.25, 1.25, (H, W, 3)).astype(np.float32)
    sp = np.array([-0.0, 1.0, np.nan, np.inf, -np.inf, 1e-45, -1e-40, 1e-39, 0.5 / 255, 1.5 / 255, 2.5 / 255, 0.0],
                  np.float32)
    flat = px.reshape(-1)
    flat[:min(sp.size, flat.size)] = sp[:flat.size]
    return px


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
        raise AssertionError("%s: %d bytes differ, first at %s" % (what, bad.size, bad[:8].tolist()))


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("size", SIZES)
def test_to_rgb_matches_model(size, fmt):
    """Random planes over 0..255 (out-of-range Y and chroma exercise the
    clamps); the whole destination buffer is compared, so row padding, the bytes
    between planes and the bytes around the image keep their guard pattern."""
    W, H = size
    rng = np.random.default_rng(1000 * W + H)
    planes = _planes(rng, W, H)
    for ragged in (False, True):
        src = Yuv(W, H, ragged, planes)
        for (m, fr), bil in itertools.product(PAIRS, (0, 1)):
            dst = Rgb(W, H, fmt, ragged)
            _to_rgb([src], [dst], W, H, L.ThorCsc(m, fr, bil))
            want = M.i420_to_rgb(*planes, m, fr, bool(bil), as_float=fmt == L.THOR_RGBF32_PLANAR)
            _same(dst.back(), dst.expect(want), "to rgb %s fmt %d m %d fr %d bil %d ragged %d" % (size, fmt, m, fr, bil, ragged))


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("size", SIZES)
def test_from_rgb_matches_model(size, fmt):
    """Float input from [-0.25, 1.25] plus -0.0, 1.0, NaN, +-inf, denormals and
    rounding ties; guard bytes in the I420 row padding must survive."""
    W, H = size
    rng = np.random.default_rng(2000 * W + H)
    px = _pixels(rng, W, H, fmt)
    for ragged in (False, True):
        src = Rgb(W, H, fmt, ragged, px)
        for m, fr in PAIRS:
            dst = Yuv(W, H, ragged)
            _from_rgb([src], [dst], W, H, L.ThorCsc(m, fr, 0))
            want = dst.expect(M.rgb_to_i420(px, m, fr))
            for k, (g, w) in enumerate(zip(dst.back(), want)):
                _same(g, w, "from rgb %s fmt %d m %d fr %d ragged %d plane %d" % (size, fmt, m, fr, ragged, k))


@pytest.mark.parametrize("n", [3, 40])
def test_batches_equal_single_images(n):
    """n = 3: three unrelated allocations and strides in one call; n = 40: more
    than one launch carries (THOR_CSC_LAUNCH_IMAGES = 16).  Every image equals
    its n = 1 result and the model."""
    assert n == 3 or n > 2 * L.THOR_CSC_LAUNCH_IMAGES
    W, H = 40, 24
    rng = np.random.default_rng(n)
    csc = L.ThorCsc(1, 0, 1)
    planes = [_planes(rng, W, H) for _ in range(n)]
    for fmt in FORMATS:
        srcs = [Yuv(W, H, bool(i % 2), planes[i]) for i in range(n)]
        dsts = [Rgb(W, H, fmt, bool((i // 2) % 2)) for i in range(n)]
        _to_rgb(srcs, dsts, W, H, csc)
        backs = [Yuv(W, H, bool((i // 3) % 2)) for i in range(n)]
        _from_rgb(dsts, backs, W, H, csc)
        for i in range(n):
            one = Rgb(W, H, fmt, bool((i // 2) % 2))
            _to_rgb([srcs[i]], [one], W, H, csc)
            got = dsts[i].back()
            _same(got, one.back(), "image %d of %d, fmt %d" % (i, n, fmt))
            want = M.i420_to_rgb(*planes[i], 1, 0, True, as_float=fmt == L.THOR_RGBF32_PLANAR)
            _same(got, dsts[i].expect(want), "image %d vs model" % i)
            b1 = Yuv(W, H, bool((i // 3) % 2))
            _from_rgb([dsts[i]], [b1], W, H, csc)
            for g, w, e in zip(backs[i].back(), b1.back(), b1.expect(M.rgb_to_i420(want, 1, 0))):
                _same(g, w, "back image %d of %d" % (i, n))
                _same(g, e, "back image %d vs model" % i)


def test_determinism_across_calls_and_streams():
    """The same call twice, and once on a second stream (a decoder context's own), gives the same bytes."""
    from thor_amd.decoder import GpuDecoder
    from thor_amd.trace import load_trace

    W, H = 130, 66
    rng = np.random.default_rng(7)
    planes = _planes(rng, W, H)
    src = Yuv(W, H, True, planes)
    ctx = GpuDecoder(load_trace(trace_path("cif_low"))[0])
    try:
        side = ctx.stream()
        assert side
        for fmt in FORMATS:
            csc = L.ThorCsc(0, 0, 1)
            a, b, c = (Rgb(W, H, fmt, True) for _ in range(3))
            _to_rgb([src], [a], W, H, csc)
            _to_rgb([src], [b], W, H, csc)
            ra, rb = a.back(), b.back()  # (the copies wait for the null stream)
            _to_rgb([src], [c], W, H, csc, side)
            ctx.sync()
            _same(ra, rb, "second call")
            _same(ra, c.back(), "second stream")
            ya, yb = Yuv(W, H, True), Yuv(W, H, True)
            _from_rgb([a], [ya], W, H, csc)
            wa = ya.back()
            _from_rgb([a], [yb], W, H, csc, side)
            ctx.sync()
            for g, w in zip(wa, yb.back()):
                _same(g, w, "from rgb, second stream")
    finally:
        ctx.close()


@pytest.mark.parametrize("matrix,full", PAIRS)
def test_round_trip_on_the_device(matrix, full):
    """Random RGB, flat in every 2x2 block -> I420 -> RGB (nearest chroma) stays
    within 2 (limited range) / 1 (full range): the bounds of the contract over
    all colours (tests/test_color_host.py)."""
    W, H = 130, 66
    rng = np.random.default_rng(11)
    px = np.repeat(np.repeat(rng.integers(0, 256, (H // 2, W // 2, 3), dtype=np.uint8), 2, axis=0), 2, axis=1)
    src = Rgb(W, H, L.THOR_RGB8_PACKED, False, px)
    mid = Yuv(W, H, False)
    dst = Rgb(W, H, L.THOR_RGB8_PACKED, False)
    csc = L.ThorCsc(matrix, full, 0)
    _from_rgb([src], [mid], W, H, csc)
    _to_rgb([mid], [dst], W, H, csc)
    got = dst.back()[dst.off:dst.off + 3 * W * H].reshape(H, W, 3).astype(np.int64)
    assert int(np.abs(got - px).max()) <= (1 if full else 2)


def test_decoder_planes(streams):
    """thor_dec_frame_planes: the device planes read back with thor_d2h are the
    frame thor_dec_read_frame returns; a frame never decoded is THOR_ERR_REF;
    the decoded frames are still the reference decoder's."""
    from thor_amd.decoder import GpuDecoder
    from thor_amd.trace import load_trace

    meta = streams["cif_low"]
    seq, frames = load_trace(trace_path("cif_low"))
    W, H = seq.width, seq.height
    dec = GpuDecoder(seq)
    try:
        for fr in frames[:3]:
            dec.decode(dec.upload(fr))
            y, u, v = dec.read(fr.frame_num)
            p = dec.planes(fr.frame_num)
            assert p.stride_y >= W and p.stride_c >= W // 2
            dec.sync()
            for ptr, stride, want in ((p.y, p.stride_y, y), (p.u, p.stride_c, u), (p.v, p.stride_c, v)):
                h, w = want.shape
                buf = np.empty(stride * (h - 1) + w, np.uint8)
                assert dec.lib.thor_d2h(buf.ctypes.data, ptr, buf.nbytes) == 0
                _same(np.lib.stride_tricks.as_strided(buf, (h, w), (stride, 1)), want, "planes")
            # the same kernel on the context's stream into a library buffer: thor_dec_frame_rgb
            for bil in (0, 1):
                dst = Rgb(W, H, L.THOR_RGB8_PACKED, True)
                img, csc = dst.desc(), L.ThorCsc(0, 0, bil)
                assert dec.lib.thor_dec_frame_rgb(dec.h, fr.frame_num, C.byref(img), C.byref(csc)) == 0
                dec.sync()
                _same(dst.back(), dst.expect(M.i420_to_rgb(y, u, v, 0, 0, bool(bil))), "thor_dec_frame_rgb %d" % bil)
            assert hashlib.md5(dec.read_i420(fr.frame_num)).hexdigest() == \
                meta["stage_md5"][fr.decode_order]["final"], fr.decode_order
        never = max(fr.frame_num for fr in frames) + 100
        with pytest.raises(RuntimeError, match="status -4"):
            dec.planes(never)
        dst = Rgb(W, H, L.THOR_RGB8_PACKED, False)
        img, csc = dst.desc(), L.ThorCsc(0, 0, 0)
        assert dec.lib.thor_dec_frame_rgb(dec.h, never, C.byref(img), C.byref(csc)) == L.THOR_ERR_REF
    finally:
        dec.close()


def test_torch_surfaces_in_a_child_process():
    """GpuDecoder.read_rgb, GpuEncoder.set_input_rgb and thor_amd.color with torch
    tensors and streams (tests/color_torch_case.py).  In a child process: torch's
    HIP runtime has to come up before the library's, and in this process the
    library's is already up."""
    import os
    import subprocess
    import sys

    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-u", os.path.join(here, "color_torch_case.py")], capture_output=True, text=True,
                       timeout=240, cwd=os.path.dirname(here))
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert r.stdout.strip().splitlines()[-1] == "ok: decoder, encoder, interop", r.stdout[-1000:]
