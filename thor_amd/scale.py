"""Frame scaling on the device: bit-exact I420 resize (thor_scaler_create /
thor_scale_i420, thor_amd/csrc/scale.hip).  The arithmetic is specified in
integers: a scaled frame is a function of the source
bytes, the same on every run.  Calls are enqueued, nothing waits.  torch is
imported inside scale_i420 only, so `import thor_amd` works without it.
No fallback: a missing library or device is an error."""
from __future__ import annotations

from . import lib as L

FILTERS = {"bilinear": L.THOR_SCALE_BILINEAR, "bicubic": L.THOR_SCALE_BICUBIC}


def filter_id(filter) -> int:
    f = FILTERS.get(filter, filter) if isinstance(filter, str) else filter
    if f not in (L.THOR_SCALE_BILINEAR, L.THOR_SCALE_BICUBIC):
        raise ValueError("filter: 'bilinear' or 'bicubic', not %r" % (filter,))
    return int(f)


def scaled_size_ok(sw: int, sh: int, dw: int, dh: int, filter="bicubic") -> bool:
    """thor_scale_check: all sizes even, 2 .. 8192, shrinking by at most 8 per axis (host only)."""
    return L.load().thor_scale_check(sw, sh, dw, dh, filter_id(filter)) == 0


def i420_planes(ptr: int, width: int, height: int) -> L.ThorYuvPlanes:
    """thor_yuv_planes_t of one contiguous I420 frame at DEVICE address `ptr`."""
    u = ptr + width * height
    return L.ThorYuvPlanes(ptr, u, u + (width // 2) * (height // 2), width, width // 2)


class Scaler:
    """One size pair and filter: the tap tables are built and uploaded here, once;
    run() only launches."""

    def __init__(self, sw: int, sh: int, dw: int, dh: int, filter="bicubic", device: int = 0):
        self.lib = L.load()
        self.filter = filter_id(filter)
        if self.lib.thor_scale_check(sw, sh, dw, dh, self.filter) != 0:
            raise ValueError("cannot scale %dx%d to %dx%d: sizes even, 2 .. %d, shrinking by at most 8"
                             % (sw, sh, dw, dh, L.THOR_SCALE_MAX_SIZE))
        self.sw, self.sh, self.dw, self.dh, self.device = sw, sh, dw, dh, device
        self.h = self.lib.thor_scaler_create(sw, sh, dw, dh, self.filter, device)
        if not self.h:
            raise L.create_error("thor_scaler_create")

    def run(self, src_planes, dst_planes, n: int, stream=0):
        """src_planes / dst_planes: ctypes arrays of n ThorYuvPlanes (DEVICE
        pointers, own strides); enqueued on `stream` (a HIP stream handle, 0 =
        the null stream)."""
        L.check(self.lib.thor_scale_i420(self.h, src_planes, dst_planes, n, stream or None), "thor_scale_i420")

    def run_frames(self, src_ptr: int, dst_ptr: int, n: int, stream=0):
        """n contiguous I420 frames at DEVICE address src_ptr -> n contiguous frames at dst_ptr."""
        fs, fd = self.sw * self.sh * 3 // 2, self.dw * self.dh * 3 // 2
        src = (L.ThorYuvPlanes * n)(*[i420_planes(src_ptr + i * fs, self.sw, self.sh) for i in range(n)])
        dst = (L.ThorYuvPlanes * n)(*[i420_planes(dst_ptr + i * fd, self.dw, self.dh) for i in range(n)])
        self.run(src, dst, n, stream)

    def close(self):
        if self.h:
            self.lib.thor_scaler_destroy(self.h)
            self.h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


def scale_i420(frames, sw: int, sh: int, dw: int, dh: int, filter="bicubic", scaler: Scaler = None):
    """frames: uint8 CUDA tensor (n, sh*3/2, sw) or (n, sw*sh*3/2) of contiguous
    I420 frames -> uint8 tensor (n, dh*3/2, dw), allocated by torch and scaled on
    torch's current stream.  `scaler`: a Scaler of these sizes to reuse (one is
    made and freed otherwise: a table build and upload per call)."""
    import torch

    fs = sw * sh * 3 // 2
    if not frames.is_cuda or frames.dtype != torch.uint8 or frames.dim() < 2:
        raise ValueError("frames: a uint8 CUDA tensor (n, H*3/2, W) or (n, W*H*3/2)")
    n = frames.shape[0]
    if n < 1 or frames.numel() != n * fs:
        raise ValueError("frames of shape %s are not %d I420 frames of %dx%d" % (tuple(frames.shape), n, sw, sh))
    frames = frames.contiguous()
    dev = frames.device.index if frames.device.index is not None else torch.cuda.current_device()
    own = scaler is None
    if own:
        scaler = Scaler(sw, sh, dw, dh, filter, dev)
    elif (scaler.sw, scaler.sh, scaler.dw, scaler.dh, scaler.device) != (sw, sh, dw, dh, dev):
        raise ValueError("the scaler is not one of %dx%d -> %dx%d on device %d" % (sw, sh, dw, dh, dev))
    try:
        out = torch.empty((n, dh * 3 // 2, dw), dtype=torch.uint8, device=frames.device)
        with torch.cuda.device(frames.device):
            cur = torch.cuda.current_stream()
            scaler.run_frames(frames.data_ptr(), out.data_ptr(), n, cur.cuda_stream)
            frames.record_stream(cur)  # (a contiguous copy made here is released at once)
    finally:
        if own:
            cur_sync = torch.cuda.current_stream(frames.device)
            cur_sync.synchronize()  # the tables must outlive the launch
            scaler.close()
    return out
