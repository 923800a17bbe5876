#!/usr/bin/env python3
"""Throughput of the temporal filter (thor_tf_i420, thor_amd/csrc/tf.hip) on the
device, next to two baselines on the same buffers in the same process:

  lookahead  thor_lookahead_i420 alone on the same (target, reference) pairs
             (the filter's coarse stage: 4 pairs per target at radius 2), and
  copy       a device-to-device copy_ of the bytes the filter's contract reads
             and writes: per target one frame and 2 * radius reference frames
             read and one frame written (the copy reads half of that and
             writes half).

`-n` targets of one clip of n + 2 * radius frames (smooth content panning by
(1, -2) pixels a frame, noise of +-3): target k is frame k + radius, filtered from
its 2 * radius neighbours, all present.  Timing: device events around
`--launches` back-to-back calls on warm buffers, `--reps` repetitions; median,
minimum and maximum are reported.  Outside the timed region the first
`--check` targets (output frame and records) are compared with the numpy model
(tests/tf_model.py; about a minute and a half per 4K target).  No GPU, no
numbers.

The measurement runs in one child process (one session, one set of buffers);
each of its steps has its own time limit (`--step-seconds`, an alarm that ends
the child), and the parent gives up on the child after their sum.

    python tools/tf_speed.py --out profiles/tf_speed.json
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from speed_common import run_worker, timed_step, write_result  # noqa: E402

STEPS = ("filter", "filter_no_records", "lookahead", "copy")


def worker(a):
    import numpy as np
    import torch

    import tf_model as M
    from thor_amd import lib as L
    from thor_amd import tfilter
    from thor_amd.scale import i420_planes

    lib = L.load()
    if not torch.cuda.is_available():
        raise SystemExit("tf_speed: no GPU visible; nothing is measured without one")
    W, H, n, R = a.width, a.height, a.n, a.radius
    nf, nrefs = n + 2 * R, 2 * R
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(1)
    fs = W * H * 3 // 2
    # one smooth frame, panned by (1, -2) pixels a frame (chroma by half that, rounded down), noise of +-3 per frame
    base = torch.randint(0, 256, (fs,), dtype=torch.uint8, device=dev, generator=gen)
    planes = [(0, H, W), (W * H, H // 2, W // 2), (W * H + (W // 2) * (H // 2), H // 2, W // 2)]
    for off, ph, pw in planes:
        p = base[off:off + ph * pw].view(ph, pw).to(torch.int16)
        for _ in range(2):
            p = (p + p.roll(1, 1) + p.roll(1, 0) + p.roll((1, 1), (0, 1)) + 2) >> 2
        base[off:off + ph * pw] = p.to(torch.uint8).view(-1)
    src = torch.empty((nf, fs), dtype=torch.uint8, device=dev)
    for k in range(nf):
        for c, (off, ph, pw) in enumerate(planes):
            p = base[off:off + ph * pw].view(ph, pw).roll((k >> (c > 0), -2 * k >> (c > 0)), (0, 1)).to(torch.int16)
            p = (p + torch.randint(-3, 4, (ph, pw), dtype=torch.int16, device=dev, generator=gen)).clamp_(0, 255)
            src[k, off:off + ph * pw] = p.to(torch.uint8).view(-1)
    dst = torch.zeros((n, fs), dtype=torch.uint8, device=dev)
    frames = [i420_planes(src.data_ptr() + k * fs, W, H) for k in range(nf)]
    cur = [frames[k + R] for k in range(n)]
    refs = [[frames[k + R + d] for d in list(range(-R, 0)) + list(range(1, R + 1))] for k in range(n)]
    out = [i420_planes(dst.data_ptr() + k * fs, W, H) for k in range(n)]
    c_cur, c_out = (L.ThorYuvPlanes * n)(*cur), (L.ThorYuvPlanes * n)(*out)
    c_refs = (L.ThorYuvPlanes * (n * nrefs))(*[r for rs in refs for r in rs])
    la_cur = (L.ThorYuvPlanes * (n * nrefs))(*[cur[k] for k in range(n) for _ in range(nrefs)])
    bw8, bh8 = tfilter.block_grid(W, H)
    recs = torch.zeros((n, nrefs, bh8, bw8, 4), dtype=torch.uint8, device=dev)
    la_sums = torch.zeros((n * nrefs, 4), dtype=torch.int64, device=dev)
    la_recs = torch.zeros((n * nrefs, (H >> 4) * (W >> 4), 8), dtype=torch.uint8, device=dev)
    copy_src = torch.empty((n * (nrefs + 2) // 2, fs), dtype=torch.uint8, device=dev)
    copy_dst = torch.empty_like(copy_src)
    st = torch.cuda.current_stream().cuda_stream
    tf = tfilter.TemporalFilter(W, H, n)
    sy, sc = a.strength
    tf_bytes = n * (nrefs + 2) * fs

    def filt():
        L.check(lib.thor_tf_i420(tf.h_, c_cur, c_refs, c_out, n, nrefs, sy, sc, recs.data_ptr(), st), "thor_tf_i420")

    def filt_no_records():
        L.check(lib.thor_tf_i420(tf.h_, c_cur, c_refs, c_out, n, nrefs, sy, sc, None, st), "thor_tf_i420")

    def lookahead():
        L.check(lib.thor_lookahead_i420(la_cur, c_refs, n * nrefs, W, H, la_recs.data_ptr(), la_sums.data_ptr(), st),
                "thor_lookahead_i420")

    def copy():
        copy_dst.copy_(copy_src)

    res = {"width": W, "height": H, "n": n, "radius": R, "strength": [sy, sc], "launches": a.launches, "reps": a.reps,
           "bytes_per_call": tf_bytes, "lookahead_bytes_per_call": 2 * n * nrefs * W * H,
           "device": torch.cuda.get_device_name(0)}
    for name, fn, nbytes in zip(STEPS, (filt, filt_no_records, lookahead, copy),
                                (tf_bytes, tf_bytes, 2 * n * nrefs * W * H, tf_bytes)):
        res[name] = timed_step(torch, fn, nbytes, a, ms_range=True)
        print("%-20s %8.1f GB/s (%.1f..%.1f)  %.3f ms per call (%.3f..%.3f)" % (
            name, res[name]["gbps_median"], res[name]["gbps_min"], res[name]["gbps_max"], res[name]["ms_median"],
            res[name]["ms_min"], res[name]["ms_max"]), flush=True)
    res["ms_per_frame"] = res["filter"]["ms_median"] / n
    res["lookahead_share"] = res["lookahead"]["ms_median"] / res["filter"]["ms_median"]
    res["time_vs_copy"] = res["filter"]["ms_median"] / res["copy"]["ms_median"]
    print("filter: %.3f ms per frame at radius %d; the lookahead alone is %.2f of it; %.1fx the time of the copy" % (
        res["ms_per_frame"], R, res["lookahead_share"], res["time_vs_copy"]), flush=True)

    # outside the timed region: the first targets of the call with records against the model, and the call
    # without records against the call with them
    filt()
    torch.cuda.synchronize()
    got, got_r = dst.cpu().numpy(), recs.cpu().numpy().view(M.RECORD).reshape(n, nrefs, bh8, bw8)
    dst.zero_()
    filt_no_records()
    torch.cuda.synchronize()
    if (dst.cpu().numpy() != got).any():
        raise SystemExit("tf_speed: the outputs with and without records differ")
    host = src.cpu().numpy()
    for k in range(min(a.check, n)):
        T = M.split(host[k + R], W, H)
        rf = [M.split(host[k + R + d], W, H) for d in list(range(-R, 0)) + list(range(1, R + 1))]
        want, want_r = M.frame(T, rf, (sy, sc))
        if (M.join(want) != got[k]).any() or (want_r != got_r[k]).any():
            raise SystemExit("tf_speed: target %d differs from the model" % k)
    res["checked_targets"] = list(range(min(a.check, n)))
    res["pixels_changed"] = float((got != host[R:R + n]).mean())
    print("targets %s equal the model; %.3f of the bytes changed" % (res["checked_targets"], res["pixels_changed"]), flush=True)
    tf.close()
    write_result(res, a.out)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("-n", type=int, default=16, help="targets per call")
    ap.add_argument("--radius", type=int, default=2, choices=(1, 2))
    ap.add_argument("--strength", type=int, nargs=2, default=(8, 3))
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--check", type=int, default=1, help="targets compared with the model")
    ap.add_argument("--step-seconds", type=int, default=60, help="time limit of each GPU step")
    ap.add_argument("--out", default="")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    # set-up (torch import, the frames), the steps, the model on the checked targets
    limit = 300 + len(STEPS) * a.step_seconds + 240 * a.check
    run_worker("tf_speed", __file__, a.step_seconds, limit)


if __name__ == "__main__":
    main()
