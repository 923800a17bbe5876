"""The device encoder with full RDOQ (-rdoq 1: te_rdoq, thor_amd/csrc/enc_pix.h,
called by every quantize of the RD loop) against the reference encoder:
tests/golden/rdoq*. (tools/make_rdoq_goldens.py) -- clips of 136 x 72 and
72 x 136 pixels (one full superblock, a partial SB column / row 8 px wide):
LDB low complexity at -qp 20, 14, 26 and 8, LDB medium complexity, HDB16 low
complexity, LDB and HDB16 high efficiency (tb split, delta-QP trials -- each
trial's RDOQ lambda follows its own qp --, speed 0).  Per case: every frame's
bytes and every superblock's RD costs equal the reference's; the first frame's
reconstruction equals the oracle decoder's of the bytes written.  At -qp 8
the reference's -rdoq 0 run writes the same bytes (RDOQ must not act); in every
other case at least two frames differ from it.  I-frame 8x8 CUs keep the
generic path under rdoq (the register-resident leaf path quantises with rdoq 0)."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLD = os.path.join(ROOT, "tests", "golden")

pytestmark = pytest.mark.gpu

CASES = ["low_w_qp20", "low_h_qp14", "low_h_qp26", "med_w_qp20", "hdb_w_qp20", "he_h_qp20", "hdbhe_w", "low_w_qp8"]


def _table():
    with open(os.path.join(GOLD, "rdoq.json")) as f:
        return json.load(f)


def _frames(b):
    out, o = [], 0
    while o < len(b):
        n = int.from_bytes(b[o:o + 4], "big")
        out.append(b[o:o + 4 + n])
        o += 4 + n
    return out


@pytest.mark.parametrize("name", CASES)
def test_rdoq_matches_reference(name):
    from oracle import OracleDecoder
    from thor_amd import synth
    from thor_amd.bitstream import parse_stream
    from thor_amd.encoder import GpuEncoder, params_for

    meta = _table()[name]
    w, h, n = meta["width"], meta["height"], meta["frames"]
    assert sum(meta["differs"]) == 0 if name == "low_w_qp8" else sum(meta["differs"]) >= 2
    params = params_for(meta["config"], w, h, n, meta["extra"])
    assert params.rdoq == 1
    enc = GpuEncoder(params)
    try:
        enc.upload_sequence(synth.synth_frames(w, h, n, meta["seed"], workers=1))
        enc.record_sb_costs()
        enc.lib.thor_enc_leaf8_count(0)  # (clears)
        chunks, costs, recon = [], [], None
        for i in range(enc.num_frames()):
            chunks.append(enc.encode_next())
            costs.append(enc.sb_costs().reshape(-1).copy())
            if i == 0:
                y, u, v = np.empty(w * h, np.uint8), np.empty(w * h // 4, np.uint8), np.empty(w * h // 4, np.uint8)
                assert enc.lib.thor_enc_read_recon(enc.h, y.ctypes.data, u.ctypes.data, v.ctypes.data) == 0
                recon = np.concatenate([y, u, v])
        leaf8 = int(enc.lib.thor_enc_leaf8_count(0))
    finally:
        enc.close()
    want = _frames(open(os.path.join(GOLD, "rdoq_%s.bit" % name), "rb").read())
    assert len(want) == n == len(chunks)
    rd = np.load(os.path.join(GOLD, "rdoq_rd.npz"))[name]
    order = []  # frame numbers in coding order
    for f in rd[:, 0]:
        if not order or order[-1] != f:
            order.append(int(f))
    for i, got in enumerate(chunks):
        assert bytes(got) == want[i], (name, i, len(got), len(want[i]))
        r = rd[rd[:, 0] == order[i]]
        assert costs[i].size == len(r), (name, i, costs[i].size, len(r))
        bad = np.nonzero(costs[i] != r[:, 5])[0]
        assert bad.size == 0, (name, i, "first differing call (frame, size, y, x, qp, ref cost), device cost",
                               r[bad[0]].tolist(), int(costs[i][bad[0]]), "of", bad.size)
    # the first frame's reconstruction == the oracle decoder's of the bytes it wrote
    seq, frames = parse_stream(bytes(chunks[0]))
    (fr, cur), = list(OracleDecoder(seq).run(frames))
    assert cur.i420() == recon.tobytes(), name
    assert leaf8 == 0, name


def test_check_params_accepts_rdoq_0_and_1_only():
    from thor_amd import lib as L
    from thor_amd.encoder import params_for

    lib = L.load()
    meta = _table()["low_w_qp20"]
    p = params_for(meta["config"], meta["width"], meta["height"], meta["frames"], meta["extra"])
    assert p.rdoq == 1 and lib.thor_enc_check_params(C.byref(p)) == 0
    p.rdoq = 0
    assert lib.thor_enc_check_params(C.byref(p)) == 0
    for bad in (2, -1):
        p.rdoq = bad
        assert lib.thor_enc_check_params(C.byref(p)) == L.THOR_ERR_ARG
