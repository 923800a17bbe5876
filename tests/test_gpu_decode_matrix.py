"""GPU: the host parser and the batched GPU decoder (thor_dec_frames: k_recon,
intra, the loop filters, the interpolated reference) on every stream of the
small-clip parity matrix, tests/golden/matrix* (tools/make_matrix_goldens.py).
The decoder had only met 352 x 288, 360 x 288, 1080p and 4K: these are 136 x 72
and 72 x 136 (one full superblock, partial ones 8 px wide or high), 40 x 24 and
8 x 8 (no full superblock, so no CLPF flags), with I frames mid-stream, every
sub-GOP shape, interpolated references at these sizes, 1 - 4 references,
-deblocking 0 / -clpf 0 in the sequence header, qp 0 and 51.  Per frame the
three stages (pre-deblock, post-deblock, final: thor_dec_set_stop_stage) equal
the reference decoder's, and the display-order output equals its .yuv.  The
four 136 x 72 high-efficiency streams, whose sequence headers differ in
deblocking, CLPF and block contexts, are also decoded together
(decode_batch): a per-launch flag that should be per context would show.  The
CPU oracle on the same streams: tests/test_oracle_matrix.py."""
import hashlib
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLD = os.path.join(ROOT, "tests", "golden")

pytestmark = pytest.mark.gpu

with open(os.path.join(GOLD, "matrix.json")) as _f:
    TABLE = json.load(_f)
CASES = sorted(TABLE)
STAGES = ((0, "pre_deblock"), (1, "post_deblock"), (2, "final"))


def _md5(b):
    return hashlib.md5(b).hexdigest()


def _parsed(name):
    from thor_amd.bitstream import parse_stream

    with open(os.path.join(GOLD, "matrix_%s.bit" % name), "rb") as f:
        return parse_stream(f.read())


@pytest.mark.parametrize("name", CASES)
def test_gpu_stages_match_reference(name):
    from thor_amd.decoder import GpuDecoder

    meta = TABLE[name]
    seq, frames = _parsed(name)
    assert (seq.width, seq.height, len(frames)) == (meta["width"], meta["height"], meta["frames"])
    dec = GpuDecoder(seq)
    try:
        out = {}
        for fr in frames:
            d = dec.upload(fr)
            for stage, key in STAGES:  # the last pass (stage 2) leaves the finished reference in the ring
                dec.set_stop_stage(stage)
                dec.decode(d)
                dec.sync()
                got = dec.read_i420(fr.frame_num)
                assert _md5(got) == meta["stage_md5"][fr.decode_order][key], (name, fr.decode_order, key,
                                                                               meta["plan"][fr.decode_order])
            out[fr.frame_num] = got
        assert _md5(b"".join(out[k] for k in sorted(out))) == meta["dec_md5"]
    finally:
        dec.close()


def test_batched_contexts_with_different_sequence_flags():
    from thor_amd.decoder import GpuDecoder, decode_batch

    names = ["he_dqp3_step2", "he_noctx_nofilt", "he_nodeblock", "he_noclpf"]
    assert all((TABLE[n]["width"], TABLE[n]["height"]) == (136, 72) for n in names)
    decs, devs, frs = [], [], []
    try:
        for nm in names:
            seq, frames = _parsed(nm)
            d = GpuDecoder(seq)
            decs.append(d)
            frs.append(frames)
            devs.append([d.upload(fr) for fr in frames])
        assert sorted((d.seq.deblocking, d.seq.clpf) for d in decs) == [(0, 0), (0, 1), (1, 0), (1, 1)]
        for i in range(max(len(f) for f in frs)):
            live = [k for k in range(len(names)) if i < len(frs[k])]
            decode_batch([decs[k] for k in live], [devs[k][i] for k in live])
            for k in live:
                fr = frs[k][i]
                got = decs[k].read_i420(fr.frame_num)
                assert _md5(got) == TABLE[names[k]]["stage_md5"][fr.decode_order]["final"], (names[k], i)
    finally:
        for d in decs:
            d.close()
