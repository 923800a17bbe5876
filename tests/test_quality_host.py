"""CPU: the frame quality measurement's host parts against the reference's own
numbers, tests/golden/quality.json (tools/make_quality_goldens.py: per coded
frame the exact Y / U / V sums of squared errors between the input frame and
the reference encoder's reconstruction, and the three PSNR strings exactly as
the reference printed them).

- thor_psnr (libthor_amd.so; snr_yuv's arithmetic, common/snr.c:60-61) on every
  golden sum formats to the reference's printed string; a sum of 0 gives inf.
- tools/enc_host -sselog -- the CPU build of the encoder source, which
  reconstructs every frame anyway -- writes the golden sums frame by frame.
The device measurement itself is checked in tests/test_gpu_quality.py."""
import ctypes as C
import json
import math
import os
import subprocess

import numpy as np
import pytest

from thor_amd import configs, synth
from thor_amd import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tools", "enc_host")
GOLD = os.path.join(ROOT, "tests", "golden")

with open(os.path.join(GOLD, "quality.json")) as _f:
    TABLE = json.load(_f)
FMT = ("%10.4f", "%8.4f", "%8.4f")  # enc/mainenc.c:536-540


def test_quality_goldens_cover_the_cases():
    assert sorted(TABLE) == sorted(["low_8x8", "low_40x24", "ldb_skip3_hq3", "hdb4_nodyadic_noint", "hdb16_n9", "wrap_i",
                                    "low_qp51", "ldb_nofilt", "low_40x24_b"])
    for name, meta in TABLE.items():
        assert len(meta["coded"]) == meta["frames"] > 0, name
        assert all(len(f["sse"]) == 3 and len(f["psnr"]) == 3 for f in meta["coded"]), name
    # what the cases are there for, on the reference's own plan
    assert TABLE["low_8x8"]["width"] == 8 and TABLE["low_40x24"]["width"] % 16 != 0
    assert any(f["input"] != f["frame_num"] for f in TABLE["ldb_skip3_hq3"]["coded"])
    order = [f["input"] for f in TABLE["hdb4_nodyadic_noint"]["coded"]]
    assert order != sorted(order) and any(f["type"] == "B" for f in TABLE["hdb4_nodyadic_noint"]["coded"])
    x = TABLE["ldb_nofilt"]["extra"]
    assert x[x.index("-deblocking") + 1] == "0" and x[x.index("-clpf") + 1] == "0"
    assert TABLE["low_40x24_b"]["seed"] != TABLE["low_40x24"]["seed"]


def test_thor_psnr_formats_as_the_reference_printed():
    lib = L.load()
    n = 0
    for name, meta in TABLE.items():
        w, h = meta["width"], meta["height"]
        dims = ((w, h), (w >> 1, h >> 1), (w >> 1, h >> 1))
        for f in meta["coded"]:
            for s, (pw, ph), fmt, want in zip(f["sse"], dims, FMT, f["psnr"]):
                got = lib.thor_psnr(s, pw, ph)
                assert (fmt % got).strip() == want, (name, f["input"], s, got, want)
                n += 1
    assert n >= 3 * 40
    # a perfect plane: log10(0) = -inf, printed as the C library prints it
    v = lib.thor_psnr(0, 136, 72)
    assert math.isinf(v) and v > 0 and ("%10.4f" % v).strip() == "inf"
    # 64-bit sums: every pixel of a 4K plane off by 255
    big = 3840 * 2160 * 255 * 255
    assert big > 2 ** 32 and lib.thor_psnr(big, 3840, 2160) == 0.0


@pytest.fixture(scope="module")
def enc_host():
    r = subprocess.run(["make", "-s", "-C", HOST, "enc_host"], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("host compiler unavailable: " + r.stderr[-200:])
    return os.path.join(HOST, "enc_host")


@pytest.mark.parametrize("name", ["low_8x8", "low_40x24", "ldb_skip3_hq3", "ldb_nofilt"])
def test_enc_host_sselog_matches_reference(enc_host, tmp_path, name):
    meta = TABLE[name]
    w, h, n = meta["width"], meta["height"], meta["frames"]
    yuv, out, log = tmp_path / "in.yuv", tmp_path / "out.bit", tmp_path / "sse.bin"
    synth.synth_frames(w, h, meta["skip"] + n, meta["seed"], workers=1).tofile(yuv)  # the -skip frames lead the file
    subprocess.run([enc_host, "-if", str(yuv), "-of", str(out), "-sselog", str(log)] +
                   configs.flags(meta["config"], w, h, n, meta["extra"]), check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    got = np.fromfile(log, dtype="<u8").reshape(-1, 3)
    want = np.array([f["sse"] for f in meta["coded"]], np.uint64)
    assert got.shape == want.shape == (n, 3)
    assert (got == want).all(), (name, got.tolist(), want.tolist())
    if meta["matrix"]:  # the same run still writes the reference's bits
        assert out.read_bytes() == open(os.path.join(GOLD, "matrix_%s.bit" % name), "rb").read()


def test_prototypes_cover_the_new_symbols():
    lib = L.load()
    for name in ("thor_sse_i420", "thor_psnr", "thor_dec_frame_sse", "thor_enc_measure_sse", "thor_enc_frame_sse",
                 "thor_enc_seq_sse"):
        assert name in L.BATCHED_SYMBOLS and getattr(lib, name).argtypes is not None, name
    assert lib.thor_psnr.restype is C.c_double
    # NULL contexts are argument errors, not crashes (no GPU needed)
    out = (C.c_uint64 * 3)()
    assert lib.thor_enc_frame_sse(None, out) == L.THOR_ERR_ARG
    assert lib.thor_enc_seq_sse(None, 0, 0, out) == L.THOR_ERR_ARG
    assert lib.thor_dec_frame_sse(None, 0, None, None) == L.THOR_ERR_ARG
    assert lib.thor_sse_i420(None, None, 1, 8, 8, None, None) == L.THOR_ERR_ARG
