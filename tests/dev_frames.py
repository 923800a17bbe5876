"""What the GPU tests of the frame utilities (test_gpu_quality, _ssim, _lookahead,
_tf) share: host arrays in device memory for the life of a test, planes and
frames laid out with noise around the pixels, random frames, and a decoder
context for its stream.  A plain module: a test file imports what it uses, the
`dev` fixture included (`from dev_frames import dev  # noqa: F401`).

The seeds of the noise are part of the tests' inputs: each layout helper keeps
the seed its test file used, so every test sees the bytes it always saw."""
import os

import numpy as np
import pytest

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


class _Dev:
    """Host arrays in device memory for the life of a test."""

    def __init__(self):
        from thor_amd import lib as L

        self.L, self.lib, self.ptrs = L, L.load(), []

    def put(self, arr):
        a = np.ascontiguousarray(arr)
        p = self.lib.thor_dev_alloc(max(a.nbytes, 16))
        assert p
        self.ptrs.append(p)
        self.L.check(self.lib.thor_h2d(p, a.ctypes.data, a.nbytes), "thor_h2d")
        return p

    def get(self, p, nbytes):
        out = np.empty(nbytes, np.uint8)
        self.L.check(self.lib.thor_d2h(out.ctypes.data, p, nbytes), "thor_d2h")
        return out

    def free(self):
        for p in self.ptrs:
            self.lib.thor_dev_free(p)
        self.ptrs = []


@pytest.fixture()
def dev():
    d = _Dev()
    yield d
    d.free()


def _plane_noise(dev, plane, stride, off, rng):
    """A plane (2-D uint8) laid out with `stride`, its first pixel `off` bytes past an allocation's start (a
    256-byte boundary); the bytes around the pixels are `rng`'s noise, so a kernel that reads past a row is
    caught.  The device address of the first pixel."""
    h, w = plane.shape
    assert stride >= w
    buf = rng.integers(0, 256, off + h * stride + 16, dtype=np.uint8)
    buf[off:off + h * stride].reshape(h, stride)[:, :w] = plane
    return dev.put(buf) + off


def _frame(dev, planes, sy, sc, off):
    """ThorYuvPlanes of the three planes with strides sy / sc and offset `off`, one stream of noise for the frame."""
    rng = np.random.default_rng(sy * 7 + sc * 3 + off)
    ptrs = [_plane_noise(dev, p, s, off, rng) for p, s in zip(planes, (sy, sc, sc))]
    return dev.L.ThorYuvPlanes(ptrs[0], ptrs[1], ptrs[2], sy, sc)


def _luma(dev, plane, stride, off):
    """ThorYuvPlanes of a luma plane alone (the lookahead reads no chroma)."""
    return dev.L.ThorYuvPlanes(_plane_noise(dev, plane, stride, off, np.random.default_rng(stride * 7 + off)), None, None,
                               stride, 0)


def _plane_in(dev, plane, stride, off):
    """One plane, its noise seeded by its own layout."""
    return _plane_noise(dev, plane, stride, off, np.random.default_rng(stride * 7 + off + plane.shape[0]))


def _frame_in(dev, planes, pad, off):
    """ThorYuvPlanes of a (y, u, v) triple: strides width + pad (chroma: its own width + pad), offset `off`."""
    y, u, v = planes
    sy, sc = y.shape[1] + pad, u.shape[1] + pad
    return dev.L.ThorYuvPlanes(_plane_in(dev, y, sy, off), _plane_in(dev, u, sc, off), _plane_in(dev, v, sc, off), sy, sc)


def _dims(w, h):
    return ((w, h), (w // 2, h // 2), (w // 2, h // 2))


def _random_planes(w, h, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (ph, pw), dtype=np.uint8) for pw, ph in _dims(w, h)]


def _side_context():
    """A decoder context, for its stream (no torch in this process: torch's HIP runtime has to come up before
    the library's)."""
    from thor_amd.bitstream import parse_stream
    from thor_amd.decoder import GpuDecoder

    with open(os.path.join(GOLD, "cif_low.bit"), "rb") as f:
        return GpuDecoder(parse_stream(f.read())[0])
