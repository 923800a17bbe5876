"""The fused SKIP-candidate pass of the device encoder (te_skip_fused,
thor_amd/csrc/enc_rd.h: early-skip check, prediction, SSD and syntax of a
uni-pred SKIP candidate from one set of registers) against the reference
encoder: tests/golden/esfuse* (tools/make_esfuse_goldens.py) -- three-frame
clips (I, P, P) of 264 x 136 and 136 x 264 pixels (4 x 2 full superblocks, a
partial SB column / row 8 px wide), LDB low complexity at the config's qp,
-qp 48 (nearly every CU a 64 x 64 early skip), -qp 8 (failed checks, so
mode_decision's SKIP candidates) and -encoder_speed 1, and HDB16 low complexity
(bi-pred candidates and future references keep the generic path).  Per case:
every frame's bytes and every superblock's RD costs equal the reference's; the
last frame's reconstruction equals the oracle decoder's of the bytes written;
no candidate takes the path in the I frame, and some do in each P frame of the
config-qp and -qp 48 cases.  The same holds with THOR_ENC_ESFUSE=0 (a fresh
child process: the switch is read once), where no candidate takes the path.

The pass falls back to the generic path when the vector clipped for the 32 x 32
sub-blocks differs from the one clipped for the 64 x 64 CU, which takes a vector
reaching more than 80 px outside the frame: frames this small cannot provoke
it.  The comparison of the two clipped vectors guards it, and the fallback is
the switched-off path this test runs."""
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

CASES = ["ldb_w", "ldb_h", "ldb_w_qp48", "ldb_w_qp8", "ldb_w_speed1", "hdb_w"]
MUST_TAKE = ("ldb_w", "ldb_h", "ldb_w_qp48")  # the path is taken in each P frame


def _table():
    with open(os.path.join(GOLD, "esfuse.json")) as f:
        return json.load(f)


def _frames(b):
    out, o = [], 0
    while o < len(b):
        n = int.from_bytes(b[o:o + 4], "big")
        out.append(b[o:o + 4 + n])
        o += 4 + n
    return out


def _code(name, meta):
    """Every frame of case `name` through the device encoder: per frame the
    chunk, the per-SB costs and the count of candidates that took the fused
    pass; the last frame's reconstruction (I420)."""
    from thor_amd import synth
    from thor_amd.encoder import GpuEncoder, params_for

    w, h, n = meta["width"], meta["height"], meta["frames"]
    enc = GpuEncoder(params_for(meta["config"], w, h, n, meta["extra"]))
    try:
        enc.upload_sequence(synth.synth_frames(w, h, n, meta["seed"], workers=1))
        enc.record_sb_costs()
        enc.lib.thor_enc_esfuse_count(0)  # (clears)
        chunks, costs, taken = [], [], []
        for i in range(enc.num_frames()):
            chunks.append(enc.encode_next())
            costs.append(enc.sb_costs().reshape(-1).copy())
            taken.append(int(enc.lib.thor_enc_esfuse_count(0)))
        y, u, v = np.empty(w * h, np.uint8), np.empty(w * h // 4, np.uint8), np.empty(w * h // 4, np.uint8)
        assert enc.lib.thor_enc_read_recon(enc.h, y.ctypes.data, u.ctypes.data, v.ctypes.data) == 0
        recon = np.concatenate([y, u, v])
    finally:
        enc.close()
    return chunks, costs, taken, recon


def _check(name, meta, chunks, costs, taken, recon, fuse_on):
    from oracle import OracleDecoder
    from thor_amd.bitstream import parse_stream

    want = _frames(open(os.path.join(GOLD, "esfuse_%s.bit" % name), "rb").read())
    assert len(want) == meta["frames"] == len(chunks)
    rd = np.load(os.path.join(GOLD, "esfuse_rd.npz"))[name]
    order = []
    for f in rd[:, 0]:
        if not order or order[-1] != f:
            order.append(int(f))
    print(name, "fused on" if fuse_on else "fused off", "candidates per frame:", taken)
    for i, got in enumerate(chunks):
        assert bytes(got) == want[i], (name, i, len(got), len(want[i]))
        w = rd[rd[:, 0] == order[i]]
        assert costs[i].size == len(w), (name, i, costs[i].size, len(w))
        bad = np.nonzero(costs[i] != w[:, 5])[0]
        assert bad.size == 0, (name, i, "first differing SB (frame, size, y, x, qp, ref cost), device cost",
                               w[bad[0]].tolist(), int(costs[i][bad[0]]), "of", bad.size)
    # the last frame's reconstruction == the oracle decoder's of the bytes written
    seq, frames = parse_stream(b"".join(bytes(c) for c in chunks))
    last = None
    for _, cur in OracleDecoder(seq).run(frames):
        last = cur.i420()
    assert last == recon.tobytes(), name
    # the path: never in the I frame; with the switch off, nowhere
    assert taken[0] == 0, (name, taken)
    if not fuse_on:
        assert taken == [0] * len(taken), (name, taken)
    elif name in MUST_TAKE:
        assert all(t > 0 for t in taken[1:]), (name, taken)


@pytest.mark.parametrize("name", CASES)
def test_esfuse_matches_reference(name):
    meta = _table()[name]
    _check(name, meta, *_code(name, meta), fuse_on=True)


@pytest.fixture(scope="module")
def switched_off(tmp_path_factory):
    """Every case coded with THOR_ENC_ESFUSE=0 in one fresh child process."""
    out = str(tmp_path_factory.mktemp("esfuse") / "off.npz")
    env = dict(os.environ, THOR_ENC_ESFUSE="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], capture_output=True, text=True, timeout=100,
                       env=env, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    return np.load(out)


@pytest.mark.parametrize("name", CASES)
def test_esfuse_switched_off_keeps_generic_path(name, switched_off):
    z, meta = switched_off, _table()[name]
    n = meta["frames"]
    chunks = [z["%s_chunk%d" % (name, i)].tobytes() for i in range(n)]
    costs = [z["%s_cost%d" % (name, i)] for i in range(n)]
    _check(name, meta, chunks, costs, z[name + "_taken"].tolist(), z[name + "_recon"], fuse_on=False)


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
