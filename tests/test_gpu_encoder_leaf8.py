"""The I-frame 8x8 leaf path of the device encoder (te_leaf8_intra,
thor_amd/csrc/enc_rd.h) against the reference encoder: tests/golden/leaf8*.
(tools/make_leaf8_goldens.py) -- two-frame clips (I, then P) of 136 x 72 and
72 x 136 pixels (one full superblock, a partial SB column / row 8 px wide),
LDB low complexity at the config's qp, -qp 8 and -qp 48, and HDB16 low
complexity.  Per case: every frame's bytes and every superblock's RD costs
equal the reference's; the I frame's reconstruction equals the oracle decoder's
of the bytes written; the path is taken for every 8x8 CU of the I frame and for
none of the P frame.  The same holds with THOR_ENC_LEAF8=0 (a fresh child
process: the switch is read once), where no CU takes the path."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLD = os.path.join(ROOT, "tests", "golden")

pytestmark = pytest.mark.gpu

CASES = ["ldb_w", "ldb_h", "ldb_w_qp8", "ldb_h_qp8", "ldb_w_qp48", "hdb_w"]


def _table():
    with open(os.path.join(GOLD, "leaf8.json")) as f:
        return json.load(f)


def _frames(b):
    out, o = [], 0
    while o < len(b):
        n = int.from_bytes(b[o:o + 4], "big")
        out.append(b[o:o + 4 + n])
        o += 4 + n
    return out


def _code(name, meta):
    """Both frames of case `name` through the device encoder: per frame the
    chunk, the per-SB costs and the count of CUs that took the leaf path; the
    I frame's reconstruction (I420)."""
    from thor_amd import synth
    from thor_amd.encoder import GpuEncoder, params_for

    w, h, n = meta["width"], meta["height"], meta["frames"]
    enc = GpuEncoder(params_for(meta["config"], w, h, n, meta["extra"]))
    try:
        enc.upload_sequence(synth.synth_frames(w, h, n, meta["seed"], workers=1))
        enc.record_sb_costs()
        enc.lib.thor_enc_leaf8_count(0)  # (clears)
        chunks, costs, taken, recon = [], [], [], None
        for i in range(enc.num_frames()):
            chunks.append(enc.encode_next())
            costs.append(enc.sb_costs().reshape(-1).copy())
            taken.append(int(enc.lib.thor_enc_leaf8_count(0)))
            if i == 0:
                y, u, v = np.empty(w * h, np.uint8), np.empty(w * h // 4, np.uint8), np.empty(w * h // 4, np.uint8)
                assert enc.lib.thor_enc_read_recon(enc.h, y.ctypes.data, u.ctypes.data, v.ctypes.data) == 0
                recon = np.concatenate([y, u, v])
    finally:
        enc.close()
    return chunks, costs, taken, recon


def _check(name, meta, chunks, costs, taken, recon, leaf_on):
    from oracle import OracleDecoder
    from thor_amd.bitstream import parse_stream

    want = _frames(open(os.path.join(GOLD, "leaf8_%s.bit" % name), "rb").read())
    assert len(want) == meta["frames"] == len(chunks)
    rd = np.load(os.path.join(GOLD, "leaf8_rd.npz"))[name]
    order = []
    for f in rd[:, 0]:
        if not order or order[-1] != f:
            order.append(int(f))
    for i, got in enumerate(chunks):
        assert bytes(got) == want[i], (name, i, len(got), len(want[i]))
        w = rd[rd[:, 0] == order[i]]
        assert costs[i].size == len(w), (name, i, costs[i].size, len(w))
        bad = np.nonzero(costs[i] != w[:, 5])[0]
        assert bad.size == 0, (name, i, "first differing SB (frame, size, y, x, qp, ref cost), device cost",
                               w[bad[0]].tolist(), int(costs[i][bad[0]]), "of", bad.size)
    # the I frame's reconstruction == the oracle decoder's of the bytes it wrote
    seq, frames = parse_stream(bytes(chunks[0]))
    (fr, cur), = list(OracleDecoder(seq).run(frames))
    assert cur.i420() == recon.tobytes(), name
    # the path: every 8x8 CU of the I frame (all lie inside: the sizes are multiples of 8), none of the P frame
    n8 = (meta["width"] // 8) * (meta["height"] // 8)
    assert taken == [n8 if leaf_on else 0, 0], (name, taken, n8)


@pytest.mark.parametrize("name", CASES)
def test_leaf8_matches_reference(name):
    meta = _table()[name]
    _check(name, meta, *_code(name, meta), leaf_on=True)


@pytest.fixture(scope="module")
def switched_off(tmp_path_factory):
    """Every case coded with THOR_ENC_LEAF8=0 in one fresh child process."""
    out = str(tmp_path_factory.mktemp("leaf8") / "off.npz")
    env = dict(os.environ, THOR_ENC_LEAF8="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], capture_output=True, text=True, timeout=100,
                       env=env, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    return np.load(out)


@pytest.mark.parametrize("name", CASES)
def test_leaf8_switched_off_keeps_generic_path(name, switched_off):
    z, meta = switched_off, _table()[name]
    n = meta["frames"]
    chunks = [z["%s_chunk%d" % (name, i)].tobytes() for i in range(n)]
    costs = [z["%s_cost%d" % (name, i)] for i in range(n)]
    _check(name, meta, chunks, costs, z[name + "_taken"].tolist(), z[name + "_recon"], leaf_on=False)


if __name__ == "__main__":  # the child of `switched_off`: code every case, save what _check reads
    table, res = _table(), {}
    for name in CASES:
        chunks, costs, taken, recon = _code(name, table[name])
        for i in range(len(chunks)):
            res["%s_chunk%d" % (name, i)] = np.frombuffer(chunks[i], np.uint8)
            res["%s_cost%d" % (name, i)] = costs[i]
        res[name + "_taken"] = np.array(taken, np.int64)
        res[name + "_recon"] = recon
    np.savez(sys.argv[1], **res)
