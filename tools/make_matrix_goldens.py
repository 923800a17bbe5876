#!/usr/bin/env python3
"""Goldens of the small-clip parity matrix (TEST INFRASTRUCTURE):
tests/golden/matrix.json, matrix_<case>.bit, matrix_rd.npz.

Runs ONLY in the build container.  The committed stream goldens use six
configurations and change only -qp, -interp_ref and -rdoq; this matrix is the
rest of what the frame loop (TeGop::plan_frame / plan_all, thor_amd/csrc/enc_gop.h)
and the sequence header can ask of the device code, on clips of two or six
superblocks (136 x 72, 72 x 136) or less than one (40 x 24, 8 x 8):
-intra_period (I frames mid-stream, references dropped for random access),
sub-GOPs of 2 / 4 / 8 / 16, -dyadic_coding 0, a tail that reverts to PPP coding,
-skip, 1 / 3 / 4 references with an HQperiod, -f 30, the HDB16 medium config,
-deblocking 0, -clpf 0, -use_block_contexts 0, -enable_bipred 0, -max_delta_qp
2 / 3 with -delta_qp_step 2, frames without a full superblock, the QP range's
ends and a frame QP that computes below 0 (the reference keeps it in a uint8_t,
enc/mainenc.h:122, so it wraps and is clipped to 51).

Per case the seeded thor_amd/synth.py clip (skip + frames input frames) is
coded by the reference encoder built by the oracle/ recipe with
-Wl,--wrap=process_block (oracle/_ref/thorenc_rd: the config file + extra
flags; records every superblock's top-level RD costs); the plain Thorenc, given
the flags of thor_amd/configs.py + extra and no config file, must write the
same bytes.  thordec_trace (THOR_TRACE_DUMP) gives each frame's three stage
md5s, the plain Thordec must write the same output, and that equals the
encoder's reconstruction.  The per-frame plan (input frame, type, qp, number of
references, interpolated reference) is read from the encoder's stdout log.

The non-vacuity conditions (each case reaches what it is there for) are
asserted here on the reference's own plan and output, and again by the tests
from matrix.json: see check().

  python tools/make_matrix_goldens.py [--only case ...]

Writes only the files named above (reference OUTPUT data: bitstreams, md5s,
costs, plans); a second run rewrites identical files."""
from __future__ import annotations

import argparse
import hashlib
import io
import json
import os
import re
import subprocess
import sys
import tempfile
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from thor_amd import configs, synth  # noqa: E402

REF = os.environ.get("THOR_REF", "/root/reference")
OREF = os.path.join(ROOT, "oracle", "_ref")
GOLD = os.path.join(ROOT, "tests", "golden")
LDB, MED, HE = ("config_LDB_low_complexity.txt", "config_LDB_medium_complexity.txt",
                "config_LDB_high_efficiency.txt")
HDB, HDBM, HDBHE = ("config_HDB16_low_complexity.txt", "config_HDB16_medium_complexity.txt",
                    "config_HDB16_high_efficiency.txt")
# case -> (config, width, height, frames, seed, extra flags)
CASES = {
    "hdb16_tail20": (HDB, 72, 136, 20, 31, "-qp 24"),
    "hdb16_n9": (HDB, 136, 72, 9, 32, ""),
    "hdbm_20": (HDBM, 136, 72, 20, 33, "-qp 24"),
    "hdbm_ra8": (HDBM, 72, 136, 20, 34, "-qp 24 -num_reorder_pics 7 -intra_period 8"),
    # (the two speed-0 clips with I frames mid-stream are cut to the fewest frames that still put a P frame
    # behind the second I frame: at 10 and 7 frames the device encoder took 24 s and 15 s to code them)
    "hdbhe_ra4": (HDBHE, 136, 72, 6, 35, "-qp 24 -num_reorder_pics 3 -intra_period 4"),
    "hdb2": (HDB, 72, 136, 8, 36, "-num_reorder_pics 1"),
    "hdb8_nodyadic": (HDB, 72, 136, 18, 37, "-qp 24 -num_reorder_pics 7 -dyadic_coding 0"),
    "hdb4_nodyadic_noint": (HDB, 72, 136, 11, 38, "-num_reorder_pics 3 -dyadic_coding 0 -interp_ref 0 -max_num_ref 4"),
    "hdb16_f30": (HDB, 72, 136, 17, 39, "-f 30"),
    "ldb_ip4": (LDB, 72, 136, 10, 40, "-intra_period 4"),
    "he_ip3_dqp2": (HE, 72, 136, 5, 41, "-qp 24 -intra_period 3 -max_delta_qp 2"),
    "he_dqp3_step2": (HE, 136, 72, 3, 42, "-qp 24 -max_delta_qp 3 -delta_qp_step 2"),
    "ldb_skip3_hq3": (LDB, 136, 72, 7, 43, "-qp 24 -skip 3 -HQperiod 3 -dqpP 1"),
    "ldb_ref3": (LDB, 72, 136, 8, 44, "-max_num_ref 3 -HQperiod 3"),
    "med_nobipred_ref4": (MED, 136, 72, 6, 45, "-qp 24 -enable_bipred 0 -max_num_ref 4 -HQperiod 4"),
    "ldb_ref1": (LDB, 72, 136, 4, 46, "-max_num_ref 1"),
    # the four 136 x 72 high-efficiency clips below share a seed: the same input, coded with the
    # sequence header's filter / context switches apart (run() also codes it with the filter left on: FILTER_OFF)
    "he_noctx_nofilt": (HE, 136, 72, 4, 47, "-qp 24 -use_block_contexts 0 -deblocking 0 -clpf 0"),
    "he_nodeblock": (HE, 136, 72, 4, 47, "-qp 24 -deblocking 0"),
    "he_noclpf": (HE, 136, 72, 4, 47, "-qp 24 -clpf 0"),
    "low_40x24": (LDB, 40, 24, 4, 48, "-qp 20"),
    "low_8x8": (LDB, 8, 8, 3, 49, "-qp 20"),
    "low_qp2": (LDB, 136, 72, 3, 50, "-qp 2"),
    "low_qp51": (LDB, 136, 72, 3, 51, "-qp 51 -dqpI 2"),
    "wrap_i": (LDB, 136, 72, 2, 52, "-qp 0"),
    "wrap_p": (LDB, 136, 72, 4, 53, "-qp 1 -dqpI 0 -mqpP 1.0 -dqpP -3 -HQperiod 2"),
    "wrap_b": (HDB, 136, 72, 6, 54, "-qp 1 -dqpI 0 -num_reorder_pics 3 -dqpB0 -2 -dqpB1 -2"),
}
TAIL = ("hdb16_tail20", "hdb16_n9")
FILTER_OFF = {"he_noclpf": "-clpf", "he_nodeblock": "-deblocking"}
# "frame  T  qp  bits  psnr-y  psnr-u  psnr-v  <reference list> | <their frame numbers>" (enc/mainenc.c:535-558)
LOG_LINE = re.compile(r"^\s*(\d+) ([IPB])\s+(\d+)\s+(\d+)\s+\S+\s+\S+\s+\S+ (.*?) \| ")


def md5(b: bytes) -> str:
    return hashlib.md5(b).hexdigest()


def flag(extra, name, default=None):
    return extra[extra.index(name) + 1] if name in extra else default


def chunks(b: bytes):
    out, o = [], 0
    while o < len(b):
        n = int.from_bytes(b[o:o + 4], "big")
        out.append(b[o + 4:o + 4 + n])
        o += 4 + n
    return out


def read_plan(log: str, skip: int):
    """One entry per coded frame, coding order: the input frame's index (the
    -skip frames counted), the frame number the header carries, type, qp, the
    number of references and whether the first is interpolated."""
    plan = []
    for line in log.splitlines():
        m = LOG_LINE.match(line)
        if not m:
            continue
        refs = re.findall(r"I\(-?\d+,-?\d+\)|-?\d+", m.group(5))
        plan.append({"input": int(m.group(1)), "frame_num": int(m.group(1)) - skip, "type": m.group(2),
                     "qp": int(m.group(3)), "num_ref": len(refs), "interp": int(bool(refs) and refs[0][0] == "I")})
    return plan


def encode(binary, config, yuv, bit, rec, work, w, h, n, extra, by_flags, rd_log=None):
    """The reference encoder on `yuv`: parameters from the config file + extra,
    or (by_flags) from thor_amd/configs.py + extra alone.  Returns its stdout."""
    io_flags = ["-if", yuv, "-of", bit, "-rf", rec, "-stat", os.path.join(work, "stat.txt")]
    if by_flags:
        cmd = [os.path.join(OREF, binary)] + io_flags + configs.flags(config, w, h, n, extra)
    else:
        cmd = [os.path.join(OREF, binary), "-cf", os.path.join(REF, config)] + io_flags + [
            "-width", str(w), "-height", str(h), "-n", str(n)] + extra
    env = dict(os.environ)
    if rd_log:
        env["THOR_RD_LOG"] = rd_log
    r = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, env=env, text=True)
    return r.stdout


def final_qps(rd, extra, config):
    """(frame_num, qp) of every superblock's final encode, from the RD records:
    per SB the delta-QP trials, then the final encode with the chosen qp."""
    mdq = int(flag(extra, "-max_delta_qp", configs.CONFIGS[config].get("-max_delta_qp", "0")))
    step = int(flag(extra, "-delta_qp_step", "1"))
    per = (2 * mdq) // step + 2 if mdq else 1
    assert len(rd) % per == 0
    return rd[per - 1::per][:, [0, 4]]


def dropped_refs(plan, max_ref):
    """P / B frames after the second I frame left with fewer references than
    max_num_ref gives a frame at that place of the coding order (min(frames
    coded, max_num_ref), one more when an interpolated reference joins two,
    enc/mainenc.c:289, :316): the loop that removes references across an I frame."""
    second_i = [i for i, f in enumerate(plan) if f["type"] == "I"][1]
    out = []
    for i, f in enumerate(plan):
        full = min(i, max_ref)
        if f["interp"] and full == 2:
            full = 3
        if i > second_i and f["type"] != "I" and f["num_ref"] < full:
            out.append(i)
    return out


def wrapped_runs(qps):
    """Runs of frames at qp 51 (coding order) whose neighbours on both sides
    (where the clip has one) are at qp <= 1: a frame QP that wrapped below 0,
    not one that is high anyway.  (wrap_b's three B frames form one run.)"""
    runs, i = [], 0
    while i < len(qps):
        j = i
        while j < len(qps) and qps[j] == 51:
            j += 1
        if j > i:
            near = [qps[k] for k in (i - 1, j) if 0 <= k < len(qps)]
            if near and all(q <= 1 for q in near):
                runs.append((i, j))
            i = j
        else:
            i += 1
    return runs


def save_npz(path, arrays):
    """np.savez_compressed with fixed member timestamps (a second run writes the same file)."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            b = io.BytesIO()
            np.lib.format.write_array(b, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(k + ".npy", (1980, 1, 1, 0, 0, 0)), b.getvalue(), zipfile.ZIP_DEFLATED)


def check(name, meta, rd, payloads):
    """The non-vacuity conditions, on the reference's own plan and output (the
    tests assert the same from matrix.json: tests/test_oracle_matrix.py)."""
    plan, extra, config = meta["plan"], meta["extra"], meta["config"]
    types = [f["type"] for f in plan]
    assert len(plan) == meta["frames"] == len(payloads) and types[0] == "I", name
    cfg = dict(configs.CONFIGS[config])
    max_ref = int(flag(extra, "-max_num_ref", cfg["-max_num_ref"]))
    interp_ref = int(flag(extra, "-interp_ref", cfg.get("-interp_ref", "0")))
    if "-intra_period" in extra:
        assert types.count("I") >= 2, name
        assert dropped_refs(plan, max_ref), (name, "no reference dropped for random access")
    if name in TAIL:
        sub_gop = int(flag(extra, "-num_reorder_pics", cfg["-num_reorder_pics"])) + 1
        whole = (meta["frames"] - 1) // sub_gop * sub_gop
        assert any(f["type"] == "P" and f["frame_num"] > whole for f in plan), (name, "no P frame in the tail")
    if interp_ref:
        assert min(meta["width"], meta["height"]) >= 32, name
        # (hdb16_n9: 9 frames never fill the 16-frame sub-GOP, so the reference codes I + 8 P and
        # interpolates nothing: the one -interp_ref 1 case without a B frame)
        assert any(f["interp"] for f in plan) or (name == "hdb16_n9" and "B" not in types), name
    else:
        assert not any(f["interp"] for f in plan), name
    if name == "hdb16_f30":
        assert sum(f["interp"] for f in plan) < meta["interp_frames_f60"], name
    if name.startswith("wrap_"):
        assert wrapped_runs([f["qp"] for f in plan]), (name, [f["qp"] for f in plan])
    if name in FILTER_OFF:
        assert meta["filter_on_bit_md5"] != meta["bit_md5"], name
    if "-max_delta_qp" in extra:
        fq = {f["frame_num"]: f["qp"] for f in plan}
        assert any(int(q) != fq[int(fn)] for fn, q in final_qps(rd, extra, config)), (name, "every SB at the frame qp")
    for f, pl in zip(plan, payloads):
        assert f["type"] == "I" or f["qp"] == 51 or len(pl) >= 8, (name, f, len(pl))


def run(name, work):
    config, w, h, n, seed, extra = CASES[name]
    extra = extra.split()
    skip = int(flag(extra, "-skip", "0"))
    yuv = os.path.join(work, name + ".yuv")
    with open(yuv, "wb") as f:
        for t in range(skip + n):
            for p in synth.synth_frame(w, h, t, seed):
                f.write(p.tobytes())
    bit, rec, rdl = (os.path.join(work, name + e) for e in (".bit", ".rec", ".rd"))
    log = encode("thorenc_rd", config, yuv, bit, rec, work, w, h, n, extra, by_flags=False, rd_log=rdl)
    data = open(bit, "rb").read()
    # the plain encoder, its parameters from thor_amd/configs.py: the same bytes, the same log
    bit2 = os.path.join(work, name + "_plain.bit")
    log2 = encode("Thorenc", config, yuv, bit2, rec + "2", work, w, h, n, extra, by_flags=True)
    assert open(bit2, "rb").read() == data, (name, "thor_amd/configs.py and the config file disagree")
    plan = read_plan(log, skip)
    assert plan == read_plan(log2, skip), name
    dump = os.path.join(work, name + "_dump")
    os.makedirs(dump)
    dec = os.path.join(work, name + ".dec")
    subprocess.run([os.path.join(OREF, "thordec_trace"), bit, dec], check=True, stdout=subprocess.DEVNULL,
                   stderr=subprocess.DEVNULL, env=dict(os.environ, THOR_TRACE_DUMP=dump))
    subprocess.run([os.path.join(OREF, "Thordec"), bit, dec + ".plain"], check=True, stdout=subprocess.DEVNULL,
                   stderr=subprocess.DEVNULL)
    dd = open(dec, "rb").read()
    assert dd == open(dec + ".plain", "rb").read(), (name, "trace hooks changed the decoder output")
    assert dd == open(rec, "rb").read(), (name, "encoder reconstruction != decoder output")
    stages = []
    deblocking = int(flag(extra, "-deblocking", "1"))
    for k in range(len(plan)):
        fr = {}
        for st in ("pre_deblock", "post_deblock", "final"):
            path = os.path.join(dump, "f%03d_%s.yuv" % (k, st))
            if st == "pre_deblock" and not deblocking:  # the hook sits on deblock_frame_y, which is never
                assert not os.path.exists(path)         # called: the frame goes unchanged to the next stage
                path = os.path.join(dump, "f%03d_post_deblock.yuv" % k)
            fr[st] = md5(open(path, "rb").read())
        stages.append(fr)
    assert not os.path.exists(os.path.join(dump, "f%03d_final.yuv" % len(plan))), name
    r = np.fromfile(rdl, dtype="<i4")
    r = r[:len(r) // 6 * 6].reshape(-1, 6).astype(np.int32)
    meta = {"config": config, "width": w, "height": h, "seed": seed, "extra": extra, "frames": n, "skip": skip,
            "bit_bytes": len(data), "bit_md5": md5(data), "dec_md5": md5(dd),
            "synth_md5": md5(open(yuv, "rb").read()), "stage_md5": stages, "plan": plan}
    if name == "hdb16_f30":  # the same clip at the config's 60 fps: one interpolation depth more
        x = extra[:extra.index("-f")] + extra[extra.index("-f") + 2:]
        meta["interp_frames_f60"] = sum(f["interp"] for f in read_plan(
            encode("Thorenc", config, yuv, bit2, rec + "2", work, w, h, n, x, by_flags=True), skip))
    if name in FILTER_OFF:  # the same clip with the filter left on
        i = extra.index(FILTER_OFF[name])
        encode("Thorenc", config, yuv, bit2, rec + "2", work, w, h, n, extra[:i] + extra[i + 2:], by_flags=True)
        meta["filter_on_bit_md5"] = md5(open(bit2, "rb").read())
    check(name, meta, r, chunks(data))
    assert len(data) < 40 * 1024, (name, len(data))
    open(os.path.join(GOLD, "matrix_%s.bit" % name), "wb").write(data)
    print("%-20s %6d bytes  %s" % (name, len(data), " ".join("%s%d" % (f["type"], f["qp"]) for f in plan)), flush=True)
    return meta, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", nargs="*")
    a = ap.parse_args()
    if not os.path.isdir(os.path.join(REF, "common")):
        sys.exit("reference sources not found at %s: goldens can only be generated in the build container" % REF)
    subprocess.run(["make", "-s", "-j8", "-C", os.path.join(ROOT, "oracle"), "ref"], check=True)
    jpath, zpath = os.path.join(GOLD, "matrix.json"), os.path.join(GOLD, "matrix_rd.npz")
    table, rd = {}, {}
    if a.only and os.path.exists(jpath):
        table = json.load(open(jpath))
        rd = dict(np.load(zpath))
    with tempfile.TemporaryDirectory() as work:
        for name in CASES:
            if not a.only or name in a.only:
                table[name], rd[name] = run(name, work)
    json.dump(table, open(jpath, "w"), indent=1, sort_keys=True)
    save_npz(zpath, rd)
    print("wrote matrix.json, matrix_rd.npz and %d .bit files" % len(table))


if __name__ == "__main__":
    main()
