#!/usr/bin/env python3
"""Throughput of the lookahead kernel (thor_lookahead_i420,
thor_amd/csrc/lookahead.hip) on the device, next to two baselines on the same
buffers in the same process:

  ssim  thor_ssim_i420 of the same frame pairs (a streaming reduction over all
        three planes of both frames: 1.5x the bytes the lookahead reads), and
  copy  a device-to-device copy_ of n luma planes' worth of bytes (reads n,
        writes n: the same total as the two luma planes per pair read here).

The lookahead's GB/s are the bytes its contract reads: the luma of two frames,
2 bytes per pixel pair; ssim's are its own (3 bytes per pixel pair).  Timing:
device events around `--launches` back-to-back calls on warm buffers, `--reps`
repetitions; median, minimum and maximum are reported.  Outside the timed
region the first and the last pair of both lookahead results (records and sums;
the sums of the call without records) are compared with the numpy model
(tests/lookahead_model.py).  No GPU, no numbers.

The measurement runs in one child process (one session, one set of buffers);
each of its steps has its own time limit (`--step-seconds`, an alarm that ends
the child), and the parent gives up on the child after their sum.

    python tools/lookahead_speed.py --out profiles/lookahead_speed.json
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from speed_common import run_worker, timed_step, write_result  # noqa: E402

STEPS = ("lookahead", "lookahead_sums_only", "ssim", "copy")


def worker(a):
    import numpy as np
    import torch

    import lookahead_model as M
    from thor_amd import lib as L
    from thor_amd.scale import i420_planes

    lib = L.load()
    if not torch.cuda.is_available():
        raise SystemExit("lookahead_speed: no GPU visible; nothing is measured without one")
    W, H, n = a.width, a.height, a.n
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(1)
    fs = W * H * 3 // 2
    # a coded sequence's kind of pair: smooth content, the reference moved by a few pixels, plus noise
    fa = torch.randint(0, 256, (n, fs), dtype=torch.uint8, device=dev, generator=gen)
    y = fa[:, :W * H].view(n, H, W).to(torch.int16)
    y = ((y + y.roll(1, 2) + y.roll(1, 1) + y.roll((1, 1), (1, 2))) >> 2).to(torch.uint8)
    fa[:, :W * H] = y.view(n, -1)
    del y
    noise = torch.randint(-3, 4, (n, fs), dtype=torch.int16, device=dev, generator=gen)
    fb = (fa.to(torch.int16) + noise).clamp_(0, 255).to(torch.uint8)
    fb[:, :W * H] = fb[:, :W * H].view(n, H, W).roll((4, -6), (1, 2)).reshape(n, -1)  # lowres (2, -3)
    del noise
    luma = fa[:, :W * H].clone()
    dst = torch.empty_like(luma)
    pa = (L.ThorYuvPlanes * n)(*[i420_planes(fa.data_ptr() + i * fs, W, H) for i in range(n)])
    pb = (L.ThorYuvPlanes * n)(*[i420_planes(fb.data_ptr() + i * fs, W, H) for i in range(n)])
    bw, bh = M.blocks(W, H)
    recs = torch.zeros((n, bh, bw, 8), dtype=torch.uint8, device=dev)
    sums = torch.zeros((n, 4), dtype=torch.int64, device=dev)
    ssim_sums = torch.zeros(3 * n, dtype=torch.int64, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    la_bytes, ssim_bytes = 2 * n * W * H, 2 * n * fs

    def lookahead():
        L.check(lib.thor_lookahead_i420(pa, pb, n, W, H, recs.data_ptr(), sums.data_ptr(), st), "thor_lookahead_i420")

    def lookahead_sums_only():
        L.check(lib.thor_lookahead_i420(pa, pb, n, W, H, None, sums.data_ptr(), st), "thor_lookahead_i420")

    def ssim():
        L.check(lib.thor_ssim_i420(pa, pb, n, W, H, ssim_sums.data_ptr(), st), "thor_ssim_i420")

    def copy():
        dst.copy_(luma)

    res = {"width": W, "height": H, "n": n, "launches": a.launches, "reps": a.reps, "bytes_per_call": la_bytes,
           "ssim_bytes_per_call": ssim_bytes, "blocks_per_frame": bw * bh, "device": torch.cuda.get_device_name(0)}
    for name, fn, nbytes in zip(STEPS, (lookahead, lookahead_sums_only, ssim, copy), (la_bytes, la_bytes, ssim_bytes, la_bytes)):
        res[name] = timed_step(torch, fn, nbytes, a, ms_range=True)
        print("%-20s %8.1f GB/s (%.1f..%.1f)  %.3f ms per call (%.3f..%.3f)" % (
            name, res[name]["gbps_median"], res[name]["gbps_min"], res[name]["gbps_max"], res[name]["ms_median"],
            res[name]["ms_min"], res[name]["ms_max"]), flush=True)
    res["us_per_pair"] = res["lookahead"]["ms_median"] * 1e3 / n
    res["time_vs_copy"] = res["lookahead"]["ms_median"] / res["copy"]["ms_median"]
    res["time_vs_ssim"] = res["lookahead"]["ms_median"] / res["ssim"]["ms_median"]
    res["rate_vs_copy"] = res["lookahead"]["gbps_median"] / res["copy"]["gbps_median"]
    res["rate_vs_ssim"] = res["lookahead"]["gbps_median"] / res["ssim"]["gbps_median"]
    print("lookahead: %.1f us per pair; %.1fx the time of the copy, %.1fx the time of ssim" % (
        res["us_per_pair"], res["time_vs_copy"], res["time_vs_ssim"]), flush=True)

    # outside the timed region: the first and the last pair of both results (with records, and the sums alone
    # into a buffer of their own) against the model
    sums_only = torch.full((n, 4), -1, dtype=torch.int64, device=dev)
    lookahead()
    L.check(lib.thor_lookahead_i420(pa, pb, n, W, H, None, sums_only.data_ptr(), st), "thor_lookahead_i420")
    torch.cuda.synchronize()
    got_r = recs.cpu().numpy().view(M.BLOCK).reshape(n, bh, bw)
    got_s = sums.cpu().numpy().astype(np.uint64)
    got_o = sums_only.cpu().numpy().astype(np.uint64)
    ha, hb = fa.cpu().numpy(), fb.cpu().numpy()
    for i in sorted({0, n - 1}):
        want_r, want_s = M.frame(ha[i, :W * H].reshape(H, W), hb[i, :W * H].reshape(H, W))
        if not (got_r[i] == want_r).all() or got_s[i].tolist() != want_s:
            raise SystemExit("lookahead_speed: pair %d differs from the model" % i)
        if got_o[i].tolist() != want_s:
            raise SystemExit("lookahead_speed: pair %d of the call without records differs from the model" % i)
    if (got_o != got_s).any():
        raise SystemExit("lookahead_speed: the sums with and without records differ")
    res["checked_pairs"] = sorted({0, n - 1})
    res["ratio_min_over_intra"] = float(got_s[:, 2].sum()) / float(got_s[:, 0].sum())
    print("pairs %s of both results equal the model; sum min / sum intra = %.3f" % (res["checked_pairs"], res["ratio_min_over_intra"]),
          flush=True)
    write_result(res, a.out)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("-n", type=int, default=64, help="frame pairs per call")
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--step-seconds", type=int, default=60, help="time limit of each GPU step")
    ap.add_argument("--out", default="")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    # set-up (torch import, 1.6 GB of frames), the steps, the model on two 4K pairs
    limit = 300 + len(STEPS) * a.step_seconds
    run_worker("lookahead_speed", __file__, a.step_seconds, limit)


if __name__ == "__main__":
    main()
