"""GPU: a plain `bench.py` run (no --full) on the smallest workload -- 2 streams
of one clip, one timed step -- prints the headline line only, and
--dump-outputs writes the last timed step's outputs as float .npy files."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

FULL_ONLY = ("roofline", "rows", "cpu_baseline", "encoder_tu_chain", "config3_encoder", "config5_encoder")


def test_plain_run_prints_the_headline_and_dumps_outputs(tmp_path):
    d = tmp_path / "dump"
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "1", "--warmup", "1",
                        "--streams", "2", "--clips", "1", "--dump-outputs", str(d)],
                       capture_output=True, text=True, timeout=110, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["steps"] == 1 and out["full"] is False and out["bit_exact"] is True
    assert out["unit"] == "Mpixels/s" and out["higher_is_better"] is True and out["dtype"] == "u8/i16"
    assert not [k for k in FULL_ONLY if k in out] and "serial_t_enc_ms" not in out["config"]
    assert r.stderr.count("timed step:") == 1
    cfg = out["config"]
    px = 2 * cfg["width"] * cfg["height"] * cfg["frames"]
    assert out["ms_per_step"] > 0
    assert abs(out["value"] - px / out["ms_per_step"] / 1e3) <= 0.01 + 1e-4 * out["value"]  # rounding of both

    arrs = {f[:-4]: np.load(str(d / f)) for f in sorted(os.listdir(str(d)))}
    assert sorted(arrs) == ["bitstream_digest", "bitstream_head", "decoded_digest", "decoded_sample",
                            "decoded_streams"]
    assert all(a.dtype in (np.float32, np.float64) for a in arrs.values())
    assert sum(a.nbytes for a in arrs.values()) <= 64 << 20
    dig = arrs["bitstream_digest"]
    assert dig.shape == (2, 2) and dig[0, 0] > 0 and (dig[0] == dig[1]).all()  # both streams code the same clip
    assert arrs["decoded_streams"].tolist() == [0.0, 1.0]
    assert arrs["decoded_digest"].shape == (2, cfg["frames"])
    assert (arrs["decoded_digest"][0] == arrs["decoded_digest"][1]).all()
    s = arrs["decoded_sample"]
    assert s.shape[:2] == (2, cfg["frames"]) and s.min() >= 0 and s.max() <= 255 and s.std() > 0
    head = arrs["bitstream_head"]
    assert head.shape[0] == 1 and np.count_nonzero(head[0, :int(min(dig[0, 0], head.shape[1]))]) > 0
