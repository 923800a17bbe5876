"""GPU: the device encoder on the small-clip parity matrix, tests/golden/matrix*
(tools/make_matrix_goldens.py): what the frame loop (TeGop::plan_frame /
plan_all, thor_amd/csrc/enc_gop.h) and the sequence header can ask of
k_enc_rows, the device loop filters, padding, the reference ring, bit packing
and k_enc_seq beyond the six configurations of the stream goldens --
-intra_period (the ring across a mid-stream I frame), sub-GOPs of 2 / 4 / 8 /
16 with and without dyadic coding, the tail that reverts to PPP coding, -skip,
1 / 3 / 4 references, -f 30, the HDB16 medium config, -deblocking 0 and -clpf 0
(the stage skip and the CLPF bits in packing), -use_block_contexts 0,
-enable_bipred 0, -max_delta_qp 2 / 3 with -delta_qp_step 2, frames without a
full superblock (40 x 24, 8 x 8), qp 0 and 51, and a frame QP that computes
below 0 (wrap_*: coded at 51 as the reference's uint8_t frame QP makes it).

Per case, frame by frame (thor_enc_frame): every chunk equals the reference
Thorenc's, every frame's reconstruction (thor_enc_read_recon) equals the
reference decoder's final frame of that coding-order position, and every
superblock's top-level RD costs equal the reference's process_block returns.
The cases without interpolated references also go through the sequence launch
(thor_enc_seq_begin), two copies per launch, byte-equal.  The CPU build of the
same source is checked in tests/test_enc_host_matrix.py."""
import hashlib
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

with open(os.path.join(GOLD, "matrix.json")) as _f:
    TABLE = json.load(_f)
CASES = sorted(TABLE)


def _interp_ref(meta):
    from thor_amd import configs

    fl = configs.flags(meta["config"], meta["width"], meta["height"], meta["frames"], meta["extra"])
    return int(dict(zip(fl[0::2], fl[1::2])).get("-interp_ref", "0"))


# the sequence launch refuses contexts with interpolated references (thor_enc_frames codes them)
NO_INTERP = [c for c in CASES if not _interp_ref(TABLE[c])]


def _chunks(b):
    out, o = [], 0
    while o < len(b):
        n = int.from_bytes(b[o:o + 4], "big")
        out.append(b[o:o + 4 + n])
        o += 4 + n
    return out


def _golden(name):
    with open(os.path.join(GOLD, "matrix_%s.bit" % name), "rb") as f:
        return _chunks(f.read())


def _encoder(meta):
    from thor_amd import synth
    from thor_amd.encoder import GpuEncoder, params_for

    w, h, n = meta["width"], meta["height"], meta["frames"]
    enc = GpuEncoder(params_for(meta["config"], w, h, n, meta["extra"]))
    try:  # the input sequence leads with the -skip frames (thor_enc_next_input counts them)
        enc.upload_sequence(synth.synth_frames(w, h, meta["skip"] + n, meta["seed"], workers=1))
    except Exception:
        enc.close()
        raise
    return enc


@pytest.fixture(autouse=True)
def _bounded_waits():
    """A wedged launch (per frame or sequence) gives up after 20 s (reported as
    a device error) instead of the 5-minute default."""
    from thor_amd import lib as L

    lib = L.load()
    lib.thor_enc_debug_stall(-1, 20000)
    yield
    lib.thor_enc_debug_stall(-1, 0)


def test_matrix_cases():
    assert len(CASES) == 26 and len(NO_INTERP) == 17, (len(CASES), NO_INTERP)


@pytest.mark.parametrize("name", CASES)
def test_frames_match_reference(name):
    meta = TABLE[name]
    w, h = meta["width"], meta["height"]
    want = _golden(name)
    rd = np.load(os.path.join(GOLD, "matrix_rd.npz"))[name]
    enc = _encoder(meta)
    try:
        assert enc.num_frames() == meta["frames"] == len(want)
        enc.record_sb_costs()
        y, u, v = np.empty(w * h, np.uint8), np.empty(w * h // 4, np.uint8), np.empty(w * h // 4, np.uint8)
        for i, pl in enumerate(meta["plan"]):
            assert enc.lib.thor_enc_next_input(enc.h) == pl["input"], (name, i)
            got = enc.encode_next()
            assert bytes(got) == want[i], (name, i, pl, len(got), len(want[i]))
            assert enc.lib.thor_enc_read_recon(enc.h, y.ctypes.data, u.ctypes.data, v.ctypes.data) == 0
            assert hashlib.md5(np.concatenate([y, u, v]).tobytes()).hexdigest() == meta["stage_md5"][i]["final"], (
                name, i, pl)
            costs = enc.sb_costs().reshape(-1)
            ref = rd[rd[:, 0] == pl["frame_num"]]
            assert costs.size == len(ref) > 0, (name, i, costs.size, len(ref))
            bad = np.nonzero(costs != ref[:, 5])[0]
            assert bad.size == 0, (name, i, "first differing call (frame, size, y, x, qp, ref cost), device cost",
                                   ref[bad[0]].tolist(), int(costs[bad[0]]), "of", bad.size)
        assert enc.lib.thor_enc_next_input(enc.h) == -1
    finally:
        enc.close()


@pytest.mark.parametrize("name", NO_INTERP)
def test_sequence_launch_matches_reference(name):
    from thor_amd.encoder import SeqLaunch

    meta = TABLE[name]
    want = _golden(name)
    encs = []
    try:
        for _ in range(2):
            encs.append(_encoder(meta))
        s = SeqLaunch(encs)
        st = s.end()
        assert st["tasks"] > 0 and s.nf == meta["frames"]
        assert (s.ready() >= 0).all()
        for i in range(2):
            for f in range(s.nf):
                got = s.chunk(i, f)
                assert got == want[f], (name, i, f, meta["plan"][f], len(got), len(want[f]))
            assert encs[i].chunk() == want[-1]
    finally:
        for e in encs:
            e.close()
