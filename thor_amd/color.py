"""Colour conversion on the device for torch users: I420 frames <-> RGB tensors
in HBM (thor_i420_to_rgb / thor_rgb_to_i420, thor_amd/csrc/color.hip).  The
arithmetic is specified in integers: the same bytes on
every run.  Everything is enqueued on torch's current stream, nothing waits.
torch is imported inside the functions, so `import thor_amd` works without it.
No fallback: a missing library or device is an error."""
from __future__ import annotations

import ctypes as C

from . import lib as L

MATRICES = {"bt601": 0, "bt709": 1}
CHROMA = {"nearest": 0, "bilinear": 1}


def csc(matrix="bt709", full_range=False, chroma="bilinear") -> L.ThorCsc:
    """thor_csc_t from names (or the header's integers)."""
    m = MATRICES.get(matrix, matrix) if isinstance(matrix, str) else matrix
    c = CHROMA.get(chroma, chroma) if isinstance(chroma, str) else chroma
    if m not in (0, 1):
        raise ValueError("matrix: 'bt601' or 'bt709', not %r" % (matrix,))
    if c not in (0, 1):
        raise ValueError("chroma: 'nearest' or 'bilinear', not %r" % (chroma,))
    return L.ThorCsc(int(m), 1 if full_range else 0, int(c))


def coeffs(matrix="bt709", full_range=False):
    """(forward, inverse) 3x3 tables as nested lists (thor_csc_coeffs; host only)."""
    lib = L.load()
    c = csc(matrix, full_range)
    f, i = (C.c_int32 * 9)(), (C.c_int32 * 9)()
    L.check(lib.thor_csc_coeffs(c.matrix, c.full_range, f, i), "thor_csc_coeffs")
    return [list(f[3 * r:3 * r + 3]) for r in range(3)], [list(i[3 * r:3 * r + 3]) for r in range(3)]


def i420_planes(ptr: int, width: int, height: int) -> L.ThorYuvPlanes:
    """thor_yuv_planes_t of one contiguous I420 frame at DEVICE address `ptr`."""
    u = ptr + width * height
    return L.ThorYuvPlanes(ptr, u, u + (width // 2) * (height // 2), width, width // 2)


def _check_size(width: int, height: int):
    if width < 2 or height < 2 or width % 2 or height % 2:
        raise ValueError("width and height must be even and >= 2, not %dx%d" % (width, height))


def rgb_images(rgb, layout=None):
    """(ThorImage array, n, width, height, keep-alive tensor) of an (n, ...) RGB
    tensor: uint8 (n, H, W, 3) "hwc", uint8 (n, 3, H, W) "chw" or float32
    (n, 3, H, W).  The tensor's strides are honoured when its innermost
    dimension is dense (a crop of a larger tensor converts in place); any other
    view is made contiguous first."""
    import torch

    if not rgb.is_cuda or rgb.dim() != 4:
        raise ValueError("an (n, ...) CUDA tensor of RGB images is required")
    if rgb.dtype not in (torch.uint8, torch.float32):
        raise ValueError("RGB tensors are uint8 or float32, not %s" % rgb.dtype)
    if layout is None:
        hwc, chw = rgb.shape[3] == 3, rgb.shape[1] == 3
        if rgb.dtype == torch.float32 or (chw and not hwc):
            layout = "chw"
        elif hwc and not chw:
            layout = "hwc"
        else:
            raise ValueError("shape %s fits both layouts: pass layout='hwc' or 'chw'" % (tuple(rgb.shape),))
    if layout not in ("hwc", "chw") or (rgb.dtype == torch.float32 and layout != "chw"):
        raise ValueError("layout 'hwc' or 'chw'; float32 goes with 'chw' only")
    if rgb.shape[3 if layout == "hwc" else 1] != 3:
        raise ValueError("shape %s is not %s RGB" % (tuple(rgb.shape), layout))
    n = rgb.shape[0]
    esz = rgb.element_size()
    if layout == "hwc":
        H, W = rgb.shape[1], rgb.shape[2]
        if rgb.stride(3) != 1 or rgb.stride(2) != 3:
            rgb = rgb.contiguous()
        fmt, stride, plane = L.THOR_RGB8_PACKED, rgb.stride(1), 0
    else:
        H, W = rgb.shape[2], rgb.shape[3]
        if rgb.stride(3) != 1:
            rgb = rgb.contiguous()
        fmt = L.THOR_RGBF32_PLANAR if rgb.dtype == torch.float32 else L.THOR_RGB8_PLANAR
        stride, plane = rgb.stride(2) * esz, rgb.stride(1) * esz
    _check_size(W, H)
    base, step = rgb.data_ptr(), rgb.stride(0) * esz
    imgs = (L.ThorImage * n)(*[L.ThorImage(base + i * step, fmt, stride, plane) for i in range(n)])
    return imgs, n, W, H, rgb


def i420_to_rgb(frames, width: int, height: int, *, matrix="bt709", full_range=False, chroma="bilinear",
                layout="chw", dtype=None):
    """frames: uint8 CUDA tensor (n, H*3/2, W) or (n, W*H*3/2) of contiguous
    I420 -> RGB tensor (n, H, W, 3) ("hwc") or (n, 3, H, W) ("chw"), uint8
    (default) or float32 in [0, 1] ("chw" only), allocated by torch and converted
    on torch's current stream."""
    import torch

    lib = L.load()
    dtype = torch.uint8 if dtype is None else dtype
    _check_size(width, height)
    fsize = width * height * 3 // 2
    if not frames.is_cuda or frames.dtype != torch.uint8 or frames.dim() < 2:
        raise ValueError("frames: a uint8 CUDA tensor (n, H*3/2, W) or (n, W*H*3/2)")
    n = frames.shape[0]
    if n < 1 or frames.numel() != n * fsize:
        raise ValueError("frames of shape %s are not %d I420 frames of %dx%d" % (tuple(frames.shape), n, width, height))
    frames = frames.contiguous()
    if layout not in ("hwc", "chw") or dtype not in (torch.uint8, torch.float32) or \
            (dtype == torch.float32 and layout != "chw"):
        raise ValueError("layout 'hwc' or 'chw'; dtype uint8 or float32 (float32 with 'chw' only)")
    shape = (n, height, width, 3) if layout == "hwc" else (n, 3, height, width)
    out = torch.empty(shape, dtype=dtype, device=frames.device)
    imgs = rgb_images(out, layout)[0]
    base = frames.data_ptr()
    src = (L.ThorYuvPlanes * n)(*[i420_planes(base + i * fsize, width, height) for i in range(n)])
    c = csc(matrix, full_range, chroma)
    with torch.cuda.device(frames.device):
        st = torch.cuda.current_stream().cuda_stream
        L.check(lib.thor_i420_to_rgb(src, imgs, n, width, height, C.byref(c), st), "thor_i420_to_rgb")
    return out


def rgb_to_i420(rgb, *, matrix="bt709", full_range=False, layout=None, out=None):
    """rgb: CUDA tensor uint8 (n, H, W, 3), uint8 (n, 3, H, W) or float32
    (n, 3, H, W) (`layout` settles a shape that fits both) -> uint8 tensor
    (n, H*3/2, W) of contiguous I420 frames (`out`: write into this contiguous
    uint8 tensor of n * W*H*3/2 bytes instead), on torch's current stream."""
    import torch

    lib = L.load()
    imgs, n, W, H, keep = rgb_images(rgb, layout)
    fsize = W * H * 3 // 2
    if out is None:
        out = torch.empty((n, H * 3 // 2, W), dtype=torch.uint8, device=rgb.device)
    elif not out.is_cuda or out.dtype != torch.uint8 or not out.is_contiguous() or out.numel() != n * fsize:
        raise ValueError("out: a contiguous uint8 CUDA tensor of %d bytes" % (n * fsize))
    base = out.data_ptr()
    dst = (L.ThorYuvPlanes * n)(*[i420_planes(base + i * fsize, W, H) for i in range(n)])
    c = csc(matrix, full_range)
    with torch.cuda.device(rgb.device):
        cur = torch.cuda.current_stream()
        L.check(lib.thor_rgb_to_i420(imgs, dst, n, W, H, C.byref(c), cur.cuda_stream), "thor_rgb_to_i420")
        keep.record_stream(cur)  # (a contiguous copy made here is released at once)
    return out
