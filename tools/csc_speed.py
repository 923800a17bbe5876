#!/usr/bin/env python3
"""Throughput of the colour-conversion kernels (thor_amd.color) on the device,
next to two baselines measured in the same process:

  torch  the same conversion written with torch elementwise ops in float (what a
         user without these kernels writes; not bit-defined), and
  copy   a device-to-device copy_ that moves the same total number of bytes (the
         streaming ceiling of the box for this amount of traffic).

Every figure is GB/s of the bytes the contract moves: 1.5 bytes per pixel of
I420 plus 3 (uint8) or 12 (float32) bytes per pixel of RGB.  Timing: device
events around `--launches` back-to-back calls on warm buffers, `--reps`
repetitions; median, minimum and maximum are reported.  No GPU, no numbers.

    python tools/csc_speed.py --out profiles/csc_speed.json
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from speed_common import rates, timed, write_result  # noqa: E402


def torch_to_rgb(torch, frames, W, H, bilinear, as_float, hwc):
    """BT.709 limited range with torch ops: float temporaries, rounding left to torch."""
    n = frames.shape[0]
    flat = frames.reshape(n, -1)
    y = flat[:, :W * H].reshape(n, 1, H, W).float()
    u = flat[:, W * H:W * H * 5 // 4].reshape(n, 1, H // 2, W // 2).float()
    v = flat[:, W * H * 5 // 4:].reshape(n, 1, H // 2, W // 2).float()
    if bilinear:
        u = torch.nn.functional.interpolate(u, scale_factor=2, mode="bilinear", align_corners=False)
        v = torch.nn.functional.interpolate(v, scale_factor=2, mode="bilinear", align_corners=False)
    else:
        u = u.repeat_interleave(2, 2).repeat_interleave(2, 3)
        v = v.repeat_interleave(2, 2).repeat_interleave(2, 3)
    y = (y - 16) * (255 / 219)
    u, v = u - 128, v - 128
    rgb = torch.cat([y + 1.7927 * v, y - 0.2132 * u - 0.5329 * v, y + 2.1124 * u], 1)
    if as_float:
        return (rgb * (1 / 255)).clamp_(0, 1)
    rgb = rgb.round_().clamp_(0, 255).to(torch.uint8)
    return rgb.permute(0, 2, 3, 1).contiguous() if hwc else rgb


def torch_from_rgb(torch, rgb, W, H, hwc):
    n = rgb.shape[0]
    x = rgb.permute(0, 3, 1, 2).float() if hwc else rgb.float()
    if rgb.dtype == torch.float32:
        x = (x * 255).round_().clamp_(0, 255)
    r, g, b = x[:, 0:1], x[:, 1:2], x[:, 2:3]
    y = 16 + 0.1826 * r + 0.6142 * g + 0.0620 * b
    cb = 128 - 0.1006 * r - 0.3386 * g + 0.4392 * b
    cr = 128 + 0.4392 * r - 0.3989 * g - 0.0403 * b
    cb, cr = torch.nn.functional.avg_pool2d(cb, 2), torch.nn.functional.avg_pool2d(cr, 2)
    parts = [p.round_().clamp_(0, 255).to(torch.uint8).reshape(n, -1) for p in (y, cb, cr)]
    return torch.cat(parts, 1)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("-n", type=int, default=64, help="frames per call")
    ap.add_argument("--torch-n", type=int, default=8, help="frames per call of the torch baseline (float temporaries)")
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    import ctypes as C

    import torch

    from thor_amd import color
    from thor_amd import lib as L

    lib = L.load()
    if not torch.cuda.is_available():
        raise SystemExit("csc_speed: no GPU visible; nothing is measured without one")
    W, H, n, tn = a.width, a.height, a.n, a.torch_n
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(1)
    frames = torch.randint(0, 256, (n, H * 3 // 2, W), dtype=torch.uint8, device=dev, generator=gen)
    px = W * H
    res = {"width": W, "height": H, "n": n, "torch_n": tn, "launches": a.launches, "reps": a.reps,
           "device": torch.cuda.get_device_name(0), "cases": []}

    def copy_rate(nbytes):
        src = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        return rates(2 * src.numel(), timed(torch, lambda: dst.copy_(src), a.launches, a.reps))

    cases = [("to_rgb", "hwc", torch.uint8), ("to_rgb", "chw", torch.uint8), ("to_rgb", "chw", torch.float32),
             ("from_rgb", "hwc", torch.uint8), ("from_rgb", "chw", torch.uint8), ("from_rgb", "chw", torch.float32)]
    for direction, layout, dtype in cases:
        esz = 4 if dtype == torch.float32 else 1
        per_frame = px * 3 // 2 + 3 * px * esz
        shape = (n, H, W, 3) if layout == "hwc" else (n, 3, H, W)
        rgb = torch.empty(shape, dtype=dtype, device=dev)
        # warm, meaningful RGB content for the from-RGB direction
        rgb.copy_(color.i420_to_rgb(frames, W, H, layout=layout, dtype=dtype))
        cp = copy_rate(n * per_frame)
        for chroma in (("nearest", "bilinear") if direction == "to_rgb" else (None,)):
            if direction == "to_rgb":
                imgs = color.rgb_images(rgb, layout)[0]
                src = (L.ThorYuvPlanes * n)(*[color.i420_planes(frames.data_ptr() + i * px * 3 // 2, W, H)
                                              for i in range(n)])
                c = color.csc("bt709", False, chroma)
                st = torch.cuda.current_stream().cuda_stream

                def ours():
                    L.check(lib.thor_i420_to_rgb(src, imgs, n, W, H, C.byref(c), st), "thor_i420_to_rgb")

                def theirs():
                    torch_to_rgb(torch, frames[:tn], W, H, chroma == "bilinear", dtype == torch.float32,
                                 layout == "hwc")
            else:
                out = torch.empty((n, H * 3 // 2, W), dtype=torch.uint8, device=dev)

                imgs = color.rgb_images(rgb, layout)[0]
                dst = (L.ThorYuvPlanes * n)(*[color.i420_planes(out.data_ptr() + i * px * 3 // 2, W, H)
                                              for i in range(n)])
                c = color.csc("bt709", False)
                st = torch.cuda.current_stream().cuda_stream

                def ours():
                    L.check(lib.thor_rgb_to_i420(imgs, dst, n, W, H, C.byref(c), st), "thor_rgb_to_i420")

                def theirs():
                    torch_from_rgb(torch, rgb[:tn], W, H, layout == "hwc")
            k = rates(n * per_frame, timed(torch, ours, a.launches, a.reps))
            t = rates(tn * per_frame, timed(torch, theirs, max(a.launches // 5, 1), max(a.reps // 2, 3), warmup=1))
            case = {"direction": direction, "layout": layout, "dtype": str(dtype).replace("torch.", ""),
                    "chroma": chroma, "bytes_per_call": n * per_frame, "kernel": k, "torch": t, "copy": cp,
                    "vs_torch": k["gbps_median"] / t["gbps_median"], "vs_copy": k["gbps_median"] / cp["gbps_median"]}
            res["cases"].append(case)
            print("%-8s %s %-7s %-8s  kernel %7.1f GB/s (%.1f..%.1f)  torch %6.1f (%.1f..%.1f)  copy %7.1f (%.1f..%.1f)"
                  "  x%.1f torch, %.2f of copy" % (direction, layout, case["dtype"], chroma or "-", k["gbps_median"],
                                                  k["gbps_min"], k["gbps_max"], t["gbps_median"], t["gbps_min"],
                                                  t["gbps_max"], cp["gbps_median"], cp["gbps_min"], cp["gbps_max"],
                                                  case["vs_torch"], case["vs_copy"]), flush=True)
        del rgb
        torch.cuda.empty_cache()
    write_result(res, a.out)


if __name__ == "__main__":
    main()
