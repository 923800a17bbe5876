#!/usr/bin/env python3
"""Throughput of the SSIM kernel (thor_ssim_i420, thor_amd/csrc/ssim.hip) on the
device, next to two baselines on the same buffers in the same process:

  sse   thor_sse_i420 of the same frame pairs (the streaming reduction that
        reads the same bytes and pays no fp64 tail), and
  copy  a device-to-device copy_ of one of the two frame sets (reads n frames,
        writes n frames: the same total number of bytes).

Every figure is GB/s of the bytes the contract reads: two I420 frames, 3 bytes
per pixel pair.  Timing: device events around `--launches` back-to-back calls on
warm buffers, `--reps` repetitions; median, minimum and maximum are reported.
No GPU, no numbers.

The measurement runs in one child process (one session, one set of buffers);
each of its three steps has its own time limit (`--step-seconds`, an alarm that
ends the child), and the parent gives up on the child after their sum.

    python tools/ssim_speed.py --out profiles/ssim_speed.json
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from speed_common import run_worker, timed_step, write_result  # noqa: E402

STEPS = ("ssim", "sse", "copy")


def worker(a):
    import torch

    from thor_amd import lib as L
    from thor_amd.scale import i420_planes

    lib = L.load()
    if not torch.cuda.is_available():
        raise SystemExit("ssim_speed: no GPU visible; nothing is measured without one")
    W, H, n = a.width, a.height, a.n
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(1)
    fs = W * H * 3 // 2
    fa = torch.randint(0, 256, (n, fs), dtype=torch.uint8, device=dev, generator=gen)
    noise = torch.randint(-3, 4, (n, fs), dtype=torch.int16, device=dev, generator=gen)
    fb = (fa.to(torch.int16) + noise).clamp_(0, 255).to(torch.uint8)  # a coded frame's kind of difference
    del noise
    dst = torch.empty_like(fa)
    pa = (L.ThorYuvPlanes * n)(*[i420_planes(fa.data_ptr() + i * fs, W, H) for i in range(n)])
    pb = (L.ThorYuvPlanes * n)(*[i420_planes(fb.data_ptr() + i * fs, W, H) for i in range(n)])
    sums = torch.zeros(3 * n, dtype=torch.int64, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    nbytes = 2 * n * fs

    def ssim():
        L.check(lib.thor_ssim_i420(pa, pb, n, W, H, sums.data_ptr(), st), "thor_ssim_i420")

    def sse():
        L.check(lib.thor_sse_i420(pa, pb, n, W, H, sums.data_ptr(), st), "thor_sse_i420")

    def copy():
        dst.copy_(fa)

    res = {"width": W, "height": H, "n": n, "launches": a.launches, "reps": a.reps, "bytes_per_call": nbytes,
           "device": torch.cuda.get_device_name(0)}
    for name, fn in zip(STEPS, (ssim, sse, copy)):
        res[name] = timed_step(torch, fn, nbytes, a)
        print("%-5s %8.1f GB/s (%.1f..%.1f)  %.3f ms per call" % (
            name, res[name]["gbps_median"], res[name]["gbps_min"], res[name]["gbps_max"], res[name]["ms_median"]),
            flush=True)
    ssim()
    torch.cuda.synchronize()
    y = sums[0::3].sum().item() / float(n * L.THOR_SSIM_ONE * lib.thor_ssim_windows(W, H))
    res["mean_ssim_y"] = y  # (that the kernel measured something: noise of +-3 on random content)
    res["ssim_vs_sse"] = res["ssim"]["gbps_median"] / res["sse"]["gbps_median"]
    res["ssim_vs_copy"] = res["ssim"]["gbps_median"] / res["copy"]["gbps_median"]
    print("ssim: %.2f of sse, %.2f of copy" % (res["ssim_vs_sse"], res["ssim_vs_copy"]), flush=True)
    write_result(res, a.out)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("-n", type=int, default=64, help="frame pairs per call")
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--step-seconds", type=int, default=60, help="time limit of each of the three GPU steps")
    ap.add_argument("--out", default="")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    # set-up (torch import, 2.4 GB of frames) + the three steps
    limit = 180 + len(STEPS) * a.step_seconds
    run_worker("ssim_speed", __file__, a.step_seconds, limit)


if __name__ == "__main__":
    main()
