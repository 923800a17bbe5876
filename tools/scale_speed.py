#!/usr/bin/env python3
"""Throughput of the frame scaler (thor_amd.scale, k_scale_i420) on the device,
next to two baselines measured in the same process:

  torch  F.interpolate(..., antialias=True) in float on the three planes, rounded
         back to bytes (what a user without the kernel writes; not bit-defined,
         a speed reference only), and
  copy   a device-to-device copy_ that moves the same total number of bytes
         (source read plus destination written).

Every figure is GB/s of the bytes the contract moves: 1.5 bytes per source pixel
read plus 1.5 bytes per destination pixel written.  Timing: device events around
`--launches` back-to-back calls on warm buffers, `--reps` repetitions; median,
minimum and maximum are reported.  Outside the timed region the first and the
last frame of every result are compared with the Python model of the contract
(tests/scale_model.py).  No GPU, no numbers.

    python tools/scale_speed.py --out profiles/scale_speed.json
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from speed_common import rates, timed, write_result  # noqa: E402


def torch_scale(torch, frames, sw, sh, dw, dh, mode):
    n = frames.shape[0]
    flat = frames.reshape(n, -1)
    out = []
    for off, w, h, ow, oh in ((0, sw, sh, dw, dh), (sw * sh, sw // 2, sh // 2, dw // 2, dh // 2),
                              (sw * sh * 5 // 4, sw // 2, sh // 2, dw // 2, dh // 2)):
        p = flat[:, off:off + w * h].reshape(n, 1, h, w).float()
        q = torch.nn.functional.interpolate(p, size=(oh, ow), mode=mode, antialias=True, align_corners=False)
        out.append(q.round_().clamp_(0, 255).to(torch.uint8).reshape(n, -1))
    return torch.cat(out, 1)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--sizes", default="1920x1080,1280x720,640x360")
    ap.add_argument("-n", type=int, default=64, help="frames per call")
    ap.add_argument("--torch-n", type=int, default=8, help="frames per call of the torch baseline (float temporaries)")
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-check", action="store_true", help="skip the comparison with the model")
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    import numpy as np
    import torch

    import scale_model as M
    from thor_amd import scale

    if not torch.cuda.is_available():
        raise SystemExit("scale_speed: no GPU visible; nothing is measured without one")
    sw, sh, n, tn = a.width, a.height, a.n, a.torch_n
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(1)
    frames = torch.randint(0, 256, (n, sh * 3 // 2, sw), dtype=torch.uint8, device=dev, generator=gen)
    fs = sw * sh * 3 // 2
    res = {"width": sw, "height": sh, "n": n, "torch_n": tn, "launches": a.launches, "reps": a.reps,
           "device": torch.cuda.get_device_name(0), "cases": []}
    st = torch.cuda.current_stream().cuda_stream
    for size in a.sizes.split(","):
        dw, dh = (int(v) for v in size.split("x"))
        fd = dw * dh * 3 // 2
        nbytes = n * (fs + fd)
        csrc = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
        cdst = torch.empty_like(csrc)
        cp = rates(2 * csrc.numel(), timed(torch, lambda: cdst.copy_(csrc), a.launches, a.reps))
        del csrc, cdst
        out = torch.empty((n, dh * 3 // 2, dw), dtype=torch.uint8, device=dev)
        for name in ("bilinear", "bicubic"):
            sc = scale.Scaler(sw, sh, dw, dh, name, 0)
            try:
                out.zero_()
                k = rates(nbytes, timed(torch, lambda: sc.run_frames(frames.data_ptr(), out.data_ptr(), n, st),
                                        a.launches, a.reps))
                torch.cuda.synchronize()
            finally:
                sc.close()
            checked = []
            if not a.no_check:
                for i in sorted({0, n - 1}):
                    want = M.scale_frames(frames[i].cpu().numpy().reshape(1, -1), sw, sh, dw, dh, scale.FILTERS[name])
                    if not np.array_equal(out[i].cpu().numpy().reshape(-1), want[0]):
                        raise SystemExit("scale_speed: frame %d of %s %dx%d differs from the model" % (i, name, dw, dh))
                    checked.append(i)
            t = rates(tn * (fs + fd), timed(torch, lambda: torch_scale(torch, frames[:tn], sw, sh, dw, dh, name),
                                            max(a.launches // 5, 1), max(a.reps // 2, 3), warmup=1))
            case = {"dst": [dw, dh], "filter": name, "bytes_per_call": nbytes, "kernel": k, "torch": t, "copy": cp,
                    "frames_checked": checked, "vs_torch": k["gbps_median"] / t["gbps_median"],
                    "vs_copy": k["gbps_median"] / cp["gbps_median"]}
            res["cases"].append(case)
            print("%dx%d -> %4dx%-4d %-8s  kernel %7.1f GB/s (%.1f..%.1f)  torch %6.1f (%.1f..%.1f)  copy %7.1f (%.1f..%.1f)"
                  "  x%.1f torch, %.2f of copy" % (sw, sh, dw, dh, name, k["gbps_median"], k["gbps_min"], k["gbps_max"],
                                                  t["gbps_median"], t["gbps_min"], t["gbps_max"], cp["gbps_median"],
                                                  cp["gbps_min"], cp["gbps_max"], case["vs_torch"], case["vs_copy"]),
                  flush=True)
            torch.cuda.empty_cache()
        del out
    write_result(res, a.out)


if __name__ == "__main__":
    main()
