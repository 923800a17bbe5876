#!/usr/bin/env python3
"""Goldens of the on-device frame quality measurement (TEST INFRASTRUCTURE):
tests/golden/quality.json.

Runs ONLY in the build container.  Per case the seeded thor_amd/synth.py clip
(skip + frames input frames) is coded by the reference encoder built by the
oracle/ recipe (oracle/_ref/Thorenc, parameters from thor_amd/configs.py + the
case's extra flags) with -rf.  Recorded per coded frame, in coding order:

  sse   the three exact sums of squared errors (Y, U, V), computed here with
        numpy from the input frame the encoder's log names and that frame's
        reconstruction in the -rf file (display order)
  psnr  the three PSNR strings exactly as the reference printed them
        (enc/mainenc.c:536-540: %10.4f %8.4f %8.4f, stripped)

The generator checks itself: formatting -10 * log10(sse / (65025.0 * h * w))
(snr_yuv, common/snr.c:60-61) must give exactly the printed strings, frame by
frame, or it fails -- so the sums are the reference's own, and a frame paired
with the wrong reconstruction cannot pass.

Cases: seven of tests/golden/matrix.json (config, size, frames, seed and extra
flags as given there; the .bit must equal matrix_<case>.bit), ldb_nofilt
(neither loop filter runs) and low_40x24_b (low_40x24 with another seed: the
second stream of the batch test).

  python tools/make_quality_goldens.py

Writes only tests/golden/quality.json (reference OUTPUT data: numbers and
printed strings); a second run rewrites an identical file."""
from __future__ import annotations

import json
import math
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from thor_amd import configs, synth  # noqa: E402

REF = os.environ.get("THOR_REF", "/root/reference")
OREF = os.path.join(ROOT, "oracle", "_ref")
GOLD = os.path.join(ROOT, "tests", "golden")
LDB = "config_LDB_low_complexity.txt"
# what each matrix case is here for
MATRIX = {
    "low_8x8": "one partial SB, 4x4 chroma",
    "low_40x24": "no full SB, width not a multiple of 16",
    "ldb_skip3_hq3": "input index != frame number",
    "hdb4_nodyadic_noint": "coding order != display order, B frames, no interpolated reference",
    "hdb16_n9": "interpolated references enabled: per-frame path only",
    "wrap_i": "frame QP wrapped to 51",
    "low_qp51": "qp 51",
}
# case -> (config, width, height, frames, seed, extra flags, why)
NEW = {
    "ldb_nofilt": (LDB, 136, 72, 3, 60, "-qp 24 -deblocking 0 -clpf 0", "neither filter stage runs"),
    "low_40x24_b": (LDB, 40, 24, 4, 61, "-qp 20", "low_40x24 with another seed (second stream of a batch)"),
}
# "frame  T  qp  bits  psnr-y  psnr-u  psnr-v  <references> |" (enc/mainenc.c:535-558)
LOG_LINE = re.compile(r"^\s*(\d+) ([IPB])\s+(\d+)\s+(\d+)\s+(\S+)\s+(\S+)\s+(\S+) .*? \| ")


def planes(frame: np.ndarray, w: int, h: int):
    y = frame[:w * h].reshape(h, w)
    c = (w // 2) * (h // 2)
    return y, frame[w * h:w * h + c].reshape(h // 2, w // 2), frame[w * h + c:w * h + 2 * c].reshape(h // 2, w // 2)


def psnr_strings(sse, w, h):
    out = []
    for s, (pw, ph), fmt in zip(sse, ((w, h), (w >> 1, h >> 1), (w >> 1, h >> 1)), ("%10.4f", "%8.4f", "%8.4f")):
        v = -10 * math.log10(s / (65025.0 * ph * pw)) if s else math.inf
        out.append((fmt % v).strip())
    return out


def run(name, config, w, h, n, seed, extra, why, work, want_bit=None):
    skip = int(extra[extra.index("-skip") + 1]) if "-skip" in extra else 0
    src = synth.synth_frames(w, h, skip + n, seed, workers=1).reshape(skip + n, -1)
    yuv, bit, rec = (os.path.join(work, name + e) for e in (".yuv", ".bit", ".rec"))
    src.tofile(yuv)
    cmd = [os.path.join(OREF, "Thorenc"), "-if", yuv, "-of", bit, "-rf", rec, "-stat", os.path.join(work, "stat.txt")]
    r = subprocess.run(cmd + configs.flags(config, w, h, n, extra), check=True, stdout=subprocess.PIPE,
                       stderr=subprocess.DEVNULL, text=True)
    if want_bit is not None:
        assert open(bit, "rb").read() == want_bit, (name, "not the stream of matrix_%s.bit" % name)
    recs = np.fromfile(rec, np.uint8).reshape(n, -1)  # display order: frame_num = input index - skip
    frames = []
    for line in r.stdout.splitlines():
        m = LOG_LINE.match(line)
        if not m:
            continue
        inp = int(m.group(1))
        sse = [int(((a.astype(np.int64) - b.astype(np.int64)) ** 2).sum())
               for a, b in zip(planes(src[inp], w, h), planes(recs[inp - skip], w, h))]
        printed = [m.group(5), m.group(6), m.group(7)]
        assert psnr_strings(sse, w, h) == printed, (name, inp, sse, psnr_strings(sse, w, h), printed)
        frames.append({"input": inp, "frame_num": inp - skip, "type": m.group(2), "sse": sse, "psnr": printed})
    assert len(frames) == n, (name, len(frames))
    print("%-22s %s" % (name, " ".join("%s%s" % (f["type"], f["psnr"][0]) for f in frames)), flush=True)
    return {"config": config, "width": w, "height": h, "frames": n, "seed": seed, "extra": extra, "skip": skip,
            "why": why, "matrix": want_bit is not None, "coded": frames}


def main():
    if not os.path.isdir(os.path.join(REF, "common")):
        sys.exit("reference sources not found at %s: goldens can only be generated in the build container" % REF)
    subprocess.run(["make", "-s", "-j8", "-C", os.path.join(ROOT, "oracle"), "ref"], check=True)
    matrix = json.load(open(os.path.join(GOLD, "matrix.json")))
    table = {}
    with tempfile.TemporaryDirectory() as work:
        for name, why in MATRIX.items():
            m = matrix[name]
            want = open(os.path.join(GOLD, "matrix_%s.bit" % name), "rb").read()
            table[name] = run(name, m["config"], m["width"], m["height"], m["frames"], m["seed"], list(m["extra"]), why,
                              work, want)
            assert [f["input"] for f in table[name]["coded"]] == [f["input"] for f in m["plan"]], name
        for name, (config, w, h, n, seed, extra, why) in NEW.items():
            table[name] = run(name, config, w, h, n, seed, extra.split(), why, work)
    json.dump(table, open(os.path.join(GOLD, "quality.json"), "w"), indent=1, sort_keys=True)
    print("wrote quality.json (%d cases)" % len(table))


if __name__ == "__main__":
    main()
