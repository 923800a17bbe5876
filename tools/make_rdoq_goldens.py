#!/usr/bin/env python3
"""Goldens for full RDOQ (-rdoq 1; quantize's tail, enc/encode_block.c:179-472)
(TEST INFRASTRUCTURE): tests/golden/rdoq_q.npz, rdoq.json, rdoq_<case>.bit,
rdoq_rd.npz.  Runs ONLY in the build container; writes reference OUTPUT data
only (coefficients, levels, bitstreams, md5s, costs).

rdoq_q.npz -- the reference quantize(..., rdoq = 1), called through
oracle/_ref/libthor_ref.so on coefficients from the reference transform of
seeded residuals (within +-255).  Per size 4, 8, 16, 32, 64: 80 TUs,

  q<size>_coef   (80, q, q) int16   input coefficients (the q x q corner quantize reads, q = min(size, 16))
  q<size>_meta   (80, 4) int32      qp, type (bit1 intra, bit0 chroma), cbp with rdoq 1, cbp with rdoq 0
  q<size>_lev1   (80, q, q) int16   levels with rdoq 1
  q<size>_lev0   (80, q, q) int16   levels with rdoq 0

chosen from >= 600 candidates per size by what the reference does with them:
per size >= 20 TUs whose rdoq-1 levels differ from rdoq 0; over the file >= 10
with cbp 1 -> 0 and >= 3 chroma TUs that end as a single level at scan
position 0 that rdoq 0 did not produce (the "single DC" candidate, :443-459).

rdoq.json / rdoq_<case>.bit / rdoq_rd.npz -- whole-encoder cases, as
tools/make_leaf8_goldens.py: seeded thor_amd/synth.py clips of 136 x 72 and
72 x 136 pixels coded by oracle/_ref/thorenc_rd (the plain Thorenc writes the
same bytes) with -rdoq 1, each superblock's top-level RD costs recorded.  The
same run with -rdoq 0 tells which frames RDOQ changed ("differs" per frame):
every case has two at least, but low_w_qp8, which has none (dense levels: the
guard against RDOQ acting where it should not).  "speed_4k": the md5 of the
reference's -rdoq 1 .bit of the 4K LDB-low clip (streams.json k4_low), what
tools/enc_speed.py --extra="-rdoq 1" --bit-md5 .. checks.

  python tools/make_rdoq_goldens.py [--no-4k]
"""
from __future__ import annotations

import ctypes as C
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from make_kernel_goldens import LIB, aligned, ptr  # noqa: E402
from thor_amd import configs, synth  # noqa: E402

REF = os.environ.get("THOR_REF", "/root/reference")
OREF = os.path.join(ROOT, "oracle", "_ref")
GOLD = os.path.join(ROOT, "tests", "golden")
LOW, MED, HE = "config_LDB_low_complexity.txt", "config_LDB_medium_complexity.txt", "config_LDB_high_efficiency.txt"
HDB, HDBHE = "config_HDB16_low_complexity.txt", "config_HDB16_high_efficiency.txt"
# case -> (config, width, height, seed, extra flags, frames)
CASES = {
    "low_w_qp20": (LOW, 136, 72, 21, ["-qp", "20", "-rdoq", "1"], 3),
    "low_h_qp14": (LOW, 72, 136, 22, ["-qp", "14", "-rdoq", "1"], 3),
    "low_h_qp26": (LOW, 72, 136, 22, ["-qp", "26", "-rdoq", "1"], 3),
    "med_w_qp20": (MED, 136, 72, 31, ["-qp", "20", "-rdoq", "1"], 3),
    "hdb_w_qp20": (HDB, 136, 72, 26, ["-qp", "20", "-rdoq", "1"], 3),
    "he_h_qp20": (HE, 72, 136, 32, ["-qp", "20", "-rdoq", "1"], 3),
    "hdbhe_w": (HDBHE, 136, 72, 33, ["-num_reorder_pics", "3", "-rdoq", "1"], 5),
    "low_w_qp8": (LOW, 136, 72, 34, ["-qp", "8", "-rdoq", "1"], 3),
}
PER_SIZE, MIN_CAND, MIN_CHANGED, MIN_FLIP, MIN_DC = 80, 600, 20, 10, 3


def quant_goldens():
    L = C.CDLL(LIB)
    C.c_int.in_dll(L, "use_simd").value = 1
    P, I = C.c_void_p, C.c_int
    L.transform.argtypes = [P, P, I, I]
    L.quantize.argtypes = [P, P, I, I, I, I]
    L.quantize.restype = I
    rng = np.random.default_rng(20261020)
    out, flips, dcs = {}, 0, 0
    for size in (4, 8, 16, 32, 64):
        q = min(size, 16)
        cand = []  # (kind, coef, qp, type, cbp1, cbp0, lev1, lev0); kind 3 single DC, 2 cbp flip, 1 changed, 0 same
        n = {0: 0, 1: 0, 2: 0, 3: 0}
        while len(cand) < MIN_CAND or n[1] + n[2] + n[3] < MIN_CHANGED + 10 or n[2] < 4:
            if len(cand) >= 20 * MIN_CAND:
                sys.exit("size %d: the draw does not reach the counts %r" % (size, n))
            qp, typ = int(rng.integers(16, 45)), int(rng.integers(0, 4))
            amp = int(rng.integers(2, 7 + int(2 ** (qp / 6))))
            res = rng.integers(-amp, amp + 1, (size, size))
            if len(cand) & 1:
                res = res + np.cumsum(rng.integers(-3, 4, (size, size)), axis=1)
            block, coeff = aligned((64, 64), np.int16), aligned((64, 64), np.int16)
            block.reshape(-1)[:size * size] = np.clip(res, -255, 255).reshape(-1)
            L.transform(ptr(block), ptr(coeff), size, int(rng.integers(0, 2)) if size >= 32 else 0)
            c = coeff.reshape(-1)[:size * size].reshape(size, size)
            lev = []
            for rdoq in (1, 0):
                cq = aligned((64, 64), np.int16)
                cbp = L.quantize(ptr(coeff), ptr(cq), qp, size, typ, rdoq)
                lev.append((cbp, cq.reshape(-1)[:size * size].reshape(size, size)[:q, :q].copy()))
            (cbp1, l1), (cbp0, l0) = lev
            kind = 0
            if not np.array_equal(l1, l0):
                only_dc = np.count_nonzero(l1) == 1 and l1[0, 0] != 0
                kind = 3 if (typ & 1) and only_dc and np.count_nonzero(l0) != 1 else (2 if cbp0 and not cbp1 else 1)
            n[kind] += 1
            cand.append((kind, c[:q, :q].copy(), qp, typ, cbp1, cbp0, l1, l0))
        # single-DC cases and cbp flips (8 each at most), changed ones and further flips up to 40 in all, the rest
        # unchanged; in candidate order
        take = [i for i, t in enumerate(cand) if t[0] == 3][:8]
        take += [i for i, t in enumerate(cand) if t[0] == 2][:8]
        take += [i for i, t in enumerate(cand) if t[0] == 1][:40 - len(take)]
        take += [i for i, t in enumerate(cand) if t[0] == 2][8:8 + 40 - len(take)]  # (4 x 4: few but flips)
        take += [i for i, t in enumerate(cand) if t[0] == 0][:PER_SIZE - len(take)]
        sel = [cand[i] for i in sorted(take)]
        assert len(sel) == PER_SIZE and sum(t[0] > 0 for t in sel) >= MIN_CHANGED, (size, n)
        flips += sum(t[0] == 2 for t in sel)
        dcs += sum(t[0] == 3 for t in sel)
        out["q%d_coef" % size] = np.stack([t[1] for t in sel]).astype(np.int16)
        out["q%d_meta" % size] = np.array([t[2:6] for t in sel], np.int32)
        out["q%d_lev1" % size] = np.stack([t[6] for t in sel]).astype(np.int16)
        out["q%d_lev0" % size] = np.stack([t[7] for t in sel]).astype(np.int16)
        print("size %2d: %d candidates (same, changed, cbp 1->0, single DC) = %r" % (size, len(cand), tuple(n.values())),
              flush=True)
    assert flips >= MIN_FLIP and dcs >= MIN_DC, (flips, dcs)
    np.savez_compressed(os.path.join(GOLD, "rdoq_q.npz"), **out)
    print("rdoq_q.npz: %d cbp 1->0, %d chroma single DC" % (flips, dcs))


def frames_of(b):
    out, o = [], 0
    while o < len(b):
        n = int.from_bytes(b[o:o + 4], "big")
        out.append(b[o:o + 4 + n])
        o += 4 + n
    return out


def run(name, work):
    config, w, h, seed, extra, nfr = CASES[name]
    yuv = os.path.join(work, name + ".yuv")
    synth.synth_frames(w, h, nfr, seed, workers=1).tofile(yuv)
    bit, log = os.path.join(work, name + ".bit"), os.path.join(work, name + ".rd")
    cmd = [os.path.join(OREF, "thorenc_rd"), "-cf", os.path.join(REF, config), "-if", yuv, "-of", bit,
           "-rf", os.path.join(work, name + ".rec"), "-stat", os.path.join(work, "stat.txt"), "-width", str(w),
           "-height", str(h), "-n", str(nfr)] + extra
    quiet = dict(check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    subprocess.run(cmd, env=dict(os.environ, THOR_RD_LOG=log), **quiet)
    data = open(bit, "rb").read()
    # the plain reference encoder writes the same bytes (the wrap only records) ...
    bit2 = os.path.join(work, name + "_plain.bit")
    cmd[0], cmd[cmd.index("-of") + 1] = os.path.join(OREF, "Thorenc"), bit2
    subprocess.run(cmd, **quiet)
    assert open(bit2, "rb").read() == data, name
    # ... and, with -rdoq 0, tells which frames RDOQ changed
    cmd[cmd.index("-rdoq") + 1] = "0"
    subprocess.run(cmd, **quiet)
    f1, f0 = frames_of(data), frames_of(open(bit2, "rb").read())
    assert len(f1) == len(f0) == nfr, name
    differs = [int(a != b) for a, b in zip(f1, f0)]
    assert sum(differs) == 0 if name == "low_w_qp8" else sum(differs) >= 2, (name, differs)
    dec = os.path.join(work, name + ".dec")
    subprocess.run([os.path.join(OREF, "Thordec"), bit, dec], **quiet)
    r = np.fromfile(log, dtype="<i4")
    r = r[:len(r) // 6 * 6].reshape(-1, 6).astype(np.int32)
    open(os.path.join(GOLD, "rdoq_%s.bit" % name), "wb").write(data)
    meta = {"config": config, "width": w, "height": h, "seed": seed, "extra": extra, "frames": nfr,
            "bit_bytes": len(data), "bit_md5": hashlib.md5(data).hexdigest(), "differs": differs,
            "dec_md5": hashlib.md5(open(dec, "rb").read()).hexdigest(),
            "synth_md5": hashlib.md5(open(yuv, "rb").read()).hexdigest()}
    print(name, meta["bit_bytes"], "bytes,", len(r), "RD records, frames changed by RDOQ:", differs, flush=True)
    return meta, r


def speed_4k(work):
    """The reference's -rdoq 1 .bit of streams.json's k4_low clip, md5 only."""
    m = json.load(open(os.path.join(GOLD, "streams.json")))["k4_low"]
    w, h, n = m["width"], m["height"], m["frames"]
    extra = list(m["extra"]) + ["-rdoq", "1"]
    yuv, bit = os.path.join(work, "k4.yuv"), os.path.join(work, "k4.bit")
    synth.synth_frames(w, h, n, m["seed"], workers=8).tofile(yuv)
    subprocess.run([os.path.join(OREF, "Thorenc"), "-cf", os.path.join(REF, m["config"]), "-if", yuv, "-of", bit,
                    "-rf", os.path.join(work, "k4.rec"), "-stat", os.path.join(work, "k4.stat")]
                   + configs.flags(m["config"], w, h, n, extra), check=True, stdout=subprocess.DEVNULL,
                   stderr=subprocess.DEVNULL)
    b = open(bit, "rb").read()
    assert hashlib.md5(b).hexdigest() != m["bit_md5"]
    return {"name": "k4_low", "extra": ["-rdoq", "1"], "frames": n, "bit_bytes": len(b),
            "bit_md5": hashlib.md5(b).hexdigest()}


def main():
    if not os.path.isdir(os.path.join(REF, "common")):
        sys.exit("reference sources not found at %s: goldens can only be generated in the build container" % REF)
    subprocess.run(["make", "-s", "-j8", "-C", os.path.join(ROOT, "oracle"), "ref"], check=True)
    quant_goldens()
    table, rd = {}, {}
    path = os.path.join(GOLD, "rdoq.json")
    with tempfile.TemporaryDirectory() as work:
        for name in CASES:
            table[name], rd[name] = run(name, work)
        if "--no-4k" in sys.argv[1:]:  # keep the recorded one
            table["speed_4k"] = json.load(open(path))["speed_4k"]
        else:
            table["speed_4k"] = speed_4k(work)
    json.dump(table, open(path, "w"), indent=1, sort_keys=True)
    np.savez_compressed(os.path.join(GOLD, "rdoq_rd.npz"), **rd)
    print("wrote rdoq_q.npz, rdoq.json, rdoq_rd.npz and %d .bit files" % len(CASES))


if __name__ == "__main__":
    main()
