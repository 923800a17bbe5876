"""CPU: the host parser (thor_parse_frame) and the CPU oracle decoder on every
stream of the small-clip parity matrix, tests/golden/matrix*
(tools/make_matrix_goldens.py): I frames mid-stream, sub-GOPs of 2 / 4 / 8 / 16
with and without dyadic coding, interpolated references at 72 x 136 / 136 x 72,
1 - 4 references, -deblocking 0 / -clpf 0 / -use_block_contexts 0 in the
sequence header, frames without a full superblock (40 x 24, 8 x 8: no CLPF
flags), qp 0 and 51.  Per frame the parsed header equals the plan the reference
encoder logged, the oracle's reconstruction equals the reference decoder's at
each of the three stages, and the display-order output equals its .yuv.

Also here: the matrix is what it claims to be.  The conditions the generator
asserted on the reference's plan and output (check() there: every
-intra_period case drops a reference across an I frame, the tails revert to P
frames, the wrap_* cases have a frame at qp 51 between frames at qp <= 1, ...)
are asserted again from the committed files."""
import hashlib
import importlib.util
import json
import os

import numpy as np
import pytest

from oracle import OracleDecoder
from thor_amd.bitstream import parse_stream, split_chunks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")

with open(os.path.join(GOLD, "matrix.json")) as _f:
    TABLE = json.load(_f)
CASES = sorted(TABLE)


def _md5(b):
    return hashlib.md5(b).hexdigest()


def _bit(name):
    with open(os.path.join(GOLD, "matrix_%s.bit" % name), "rb") as f:
        return f.read()


def _generator():
    spec = importlib.util.spec_from_file_location("make_matrix_goldens",
                                                  os.path.join(ROOT, "tools", "make_matrix_goldens.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


GEN = _generator()


def test_matrix_holds_every_case():
    assert sorted(GEN.CASES) == CASES and len(CASES) == 26


@pytest.mark.parametrize("name", CASES)
def test_matrix_case_is_not_vacuous(name):
    meta, data = TABLE[name], _bit(name)
    config, w, h, n, seed, extra = GEN.CASES[name]
    assert (meta["config"], meta["width"], meta["height"], meta["frames"], meta["seed"], meta["extra"]) == (
        config, w, h, n, seed, extra.split())
    assert _md5(data) == meta["bit_md5"] and len(data) < 40 * 1024
    rd = np.load(os.path.join(GOLD, "matrix_rd.npz"))[name]
    nsb = ((w + 63) // 64) * ((h + 63) // 64)
    assert len(rd) > 0 and len(rd) % (nsb * n) == 0
    GEN.check(name, meta, rd, split_chunks(data))


@pytest.mark.parametrize("name", CASES)
def test_parser_and_oracle_match_reference(name):
    meta = TABLE[name]
    seq, frames = parse_stream(_bit(name))
    assert (seq.width, seq.height) == (meta["width"], meta["height"])
    plan = meta["plan"]
    assert len(frames) == len(plan) == meta["frames"]
    dyadic = "-dyadic_coding" not in meta["extra"]
    nflags = (meta["width"] >> 6) * (meta["height"] >> 6)
    dec = OracleDecoder(seq)
    out = {}
    for fr, pl in zip(frames, plan):
        k = fr.decode_order
        assert (fr.frame_num, fr.qp, fr.num_ref) == (pl["frame_num"], pl["qp"], pl["num_ref"]), (name, k)
        # (the header says intra or inter: a B frame is an inter frame with a later reference)
        assert (fr.frame_type == 0) == (pl["type"] == "I"), (name, k)
        # the log names an interpolated reference, not its ratio: 2 (the midpoint) in a dyadic sub-GOP
        assert (fr.interp_ratio > 0) == bool(pl["interp"]), (name, k)
        if pl["interp"] and dyadic:
            assert (fr.interp_ratio, fr.interp_pos) == (2, 1), (name, k)
        if not fr.clpf_on or nflags == 0:
            assert fr.clpf_flags.size == 0, (name, k)
        for stage, key in ((0, "pre_deblock"), (1, "post_deblock")):
            cur = dec.decode(fr, stage)
            assert _md5(cur.i420()) == meta["stage_md5"][k][key], (name, k, key)
        cur = dec.decode(fr, 2)
        assert _md5(cur.i420()) == meta["stage_md5"][k]["final"], (name, k)
        out[fr.frame_num] = cur.i420()
        dec.push_reference(cur)
    assert _md5(b"".join(out[k] for k in sorted(out))) == meta["dec_md5"]
