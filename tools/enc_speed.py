#!/usr/bin/env python3
"""Device encoder timing probe: code a golden clip with B concurrent contexts
(thor_enc_frames batches), check every stream's bits against the reference
.bit, report per-frame wall times.  --extra appends encoder flags to the
clip's (one string, e.g. --extra="-rdoq 1"); the bits are then checked, outside the timed
region as always, against --bit-md5 (rdoq.json's speed_4k for k4_low with
-rdoq 1: tools/make_rdoq_goldens.py) or, with no md5 given, not at all.
--quality turns the on-device frame quality measurement on for every context
(thor_enc_measure_sse: one more launch per batch) and prints the
last frame's PSNR of the first stream."""
import argparse
import hashlib
import json
import os
import shlex
import sys
import time


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from thor_amd import synth  # noqa: E402
from thor_amd.encoder import GpuEncoder, encode_batch, params_for  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--name", default="k4_low")
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--frames", type=int, default=0)
    ap.add_argument("--limit", type=int, default=0,
                    help="code only the first LIMIT coded frames of the plan (the GOP as for --frames)")
    ap.add_argument("--extra", default="", help="encoder flags appended to the clip's own, as one string")
    ap.add_argument("--bit-md5", default="", help="md5 of the whole reference .bit for the clip with --extra")
    ap.add_argument("--quality", action="store_true", help="measure every coded frame's SSE on the device")
    a = ap.parse_args()
    a.extra = shlex.split(a.extra)
    meta = json.load(open(os.path.join(ROOT, "tests", "golden", "streams.json")))[a.name]
    n = a.frames or meta["frames"]
    w, h = meta["width"], meta["height"]
    frames = synth.synth_frames(w, h, n, meta["seed"], workers=8)  # before any GPU call (fork)
    want = open(os.path.join(ROOT, "tests", "golden", a.name + ".bit"), "rb").read()
    res = {}
    for B in a.batch:
        encs = [GpuEncoder(params_for(meta["config"], w, h, n, list(meta["extra"]) + a.extra)) for _ in range(B)]
        for e in encs:
            e.upload_sequence(frames)
            if a.quality:
                e.measure_quality()
        out = [b""] * B
        t_frames = []
        for i in range(a.limit or n):
            t0 = time.perf_counter()
            ch = encode_batch(encs)
            t_frames.append(time.perf_counter() - t0)
            print("  frame %d: %.1f ms" % (i, 1e3 * t_frames[-1]), flush=True)  # progress (long speed-0 frames)
            for k in range(B):
                out[k] += ch[k]
        if a.extra:  # another stream than the golden .bit: the md5 of the whole of it, or nothing to compare with
            ok = all(hashlib.md5(o).hexdigest() == a.bit_md5 for o in out) if (
                a.bit_md5 and n == meta["frames"] and not a.limit) else None
        else:
            ok = all(o == want[:len(o)] for o in out) and len(out[0]) == len(want) if (
                n == meta["frames"] and not a.limit) else all(want.startswith(o) for o in out)
        tot = sum(t_frames)
        res[B] = dict(ok=ok, total_s=tot, frame_ms=[round(1000 * t, 2) for t in t_frames],
                      mpx_s=B * w * h * (a.limit or n) / tot / 1e6)
        if a.quality:
            res[B]["last_psnr"] = [round(v, 4) for v in encs[0].psnr()]
        print(a.name, "batch", B, json.dumps(res[B]), flush=True)
        for e in encs:
            e.close()


if __name__ == "__main__":
    main()
