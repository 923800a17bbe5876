"""CPU: the host build of the device encoder's frame loop and RD source
(tools/enc_host, one lane: TeGop::plan_frame / plan_all of
thor_amd/csrc/enc_gop.h, the RD loop of enc_rd.h) against the reference encoder
on the small-clip parity matrix, tests/golden/matrix* (tools/make_matrix_goldens.py):
-intra_period, sub-GOPs of 2 / 4 / 8 / 16, -dyadic_coding 0, the tail that
reverts to PPP coding, -skip, 1 / 3 / 4 references with an HQperiod, -f 30, the
HDB16 medium config, -deblocking 0, -clpf 0, -use_block_contexts 0,
-enable_bipred 0, -max_delta_qp 2 / 3 with -delta_qp_step 2, frames without a
full superblock, and a frame QP that computes below 0 (wrap_*: the reference
keeps it in a uint8_t, so it wraps and is clipped to 51, not to 0).  The .bit
must equal the reference Thorenc's byte for byte; for three cases the
per-superblock RD costs must equal its process_block returns, call by call.
The GPU build of the same source is checked in tests/test_gpu_encoder_matrix.py."""
import json
import os
import subprocess

import numpy as np
import pytest

from thor_amd import configs, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tools", "enc_host")
GOLD = os.path.join(ROOT, "tests", "golden")

with open(os.path.join(GOLD, "matrix.json")) as _f:
    TABLE = json.load(_f)
CASES = sorted(TABLE)


@pytest.fixture(scope="module")
def enc_host():
    r = subprocess.run(["make", "-s", "-C", HOST, "enc_host"], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("host compiler unavailable: " + r.stderr[-200:])
    return os.path.join(HOST, "enc_host")


@pytest.fixture(scope="module")
def coded(enc_host, tmp_path_factory):
    """coded(name) -> (the host lane's .bit, its RD cost records) of a case; each case is coded once."""
    done = {}

    def run(name):
        if name not in done:
            meta, work = TABLE[name], tmp_path_factory.mktemp(name)
            w, h, n = meta["width"], meta["height"], meta["frames"]
            yuv, out, rd = work / "in.yuv", work / "out.bit", work / "costs.bin"
            # the -skip frames lead the file
            synth.synth_frames(w, h, meta["skip"] + n, meta["seed"], workers=1).tofile(yuv)
            subprocess.run([enc_host, "-if", str(yuv), "-of", str(out), "-rdlog", str(rd)] +
                           configs.flags(meta["config"], w, h, n, meta["extra"]), check=True,
                           stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
            done[name] = (out.read_bytes(), np.fromfile(rd, dtype="<i4").reshape(-1, 6))
            yuv.unlink()
        return done[name]

    return run


def _chunks(b):
    out, o = [], 0
    while o < len(b):
        n = int.from_bytes(b[o:o + 4], "big")
        out.append(b[o:o + 4 + n])
        o += 4 + n
    return out


def test_matrix_has_every_case():
    assert len(CASES) == 26 and sum(c.startswith("wrap_") for c in CASES) == 3


@pytest.mark.parametrize("name", CASES)
def test_host_build_matches_reference(coded, name):
    meta = TABLE[name]
    want = open(os.path.join(GOLD, "matrix_%s.bit" % name), "rb").read()
    assert len(want) == meta["bit_bytes"]
    got = coded(name)[0]
    if got != want:
        g, w = _chunks(got), _chunks(want)
        bad = [i for i in range(min(len(g), len(w))) if g[i] != w[i]]
        assert False, (name, "frames", len(g), "of", len(w), "first differing frame (coding order)",
                       bad[:1], "sizes", [len(c) for c in g], [len(c) for c in w])


@pytest.mark.parametrize("name", ["he_dqp3_step2", "he_ip3_dqp2", "hdbm_ra8"])
def test_host_build_rd_costs_match_reference(coded, name):
    """Every superblock's top-level RD costs (each delta-QP trial with its own
    qp, then the final encode) == the reference encoder's (matrix_rd.npz)."""
    got = coded(name)[1]
    want = np.load(os.path.join(GOLD, "matrix_rd.npz"))[name]
    assert len(got) == len(want) and len(got) > 0
    assert (got[:, :4] == want[:, :4]).all()
    trial = got[:, 4] >= 0  # (the host lane's final-encode records carry -1, the reference's the chosen qp)
    assert (got[trial, 4] == want[trial, 4]).all()
    bad = np.nonzero(got[:, 5] != want[:, 5])[0]
    assert bad.size == 0, ("first differing call", want[bad[0]].tolist(), int(got[bad[0], 5]))
