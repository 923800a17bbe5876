"""The L2 quantize (include/thor_l2.h) with rdoq = 1 -- one wave running
te_quant_t and te_rdoq (thor_amd/csrc/enc_pix.h) on one TU -- against the
reference's quantize(..., rdoq = 1): tests/golden/rdoq_q.npz
(tools/make_rdoq_goldens.py), 80 TUs per size 4, 8, 16, 32, 64 picked by what
the reference does with them (per size >= 20 whose levels full RDOQ changes;
cbp 1 -> 0; the chroma "single DC" outcome; the rest left alone).  Levels
inside q x q and cbp equal the reference's, elements outside q x q keep a
sentinel, and the same inputs with rdoq = 0 still give the rdoq-0 levels."""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")

SENTINEL = 12345


def _lib():
    from thor_amd import lib as L

    lib = L.load()
    lib.quantize.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
    lib.quantize.restype = C.c_int
    return lib


def test_goldens_cover_what_full_rdoq_does():
    """(the data, not the device) what tools/make_rdoq_goldens.py selected for."""
    z = np.load(os.path.join(GOLD, "rdoq_q.npz"))
    flips = dcs = 0
    for size in (4, 8, 16, 32, 64):
        meta, l1, l0 = z["q%d_meta" % size], z["q%d_lev1" % size], z["q%d_lev0" % size]
        assert len(meta) == 80
        assert sum(not np.array_equal(a, b) for a, b in zip(l1, l0)) >= 20
        flips += int(((meta[:, 3] != 0) & (meta[:, 2] == 0)).sum())
        dcs += sum(bool(m[1] & 1) and np.count_nonzero(a) == 1 and a[0, 0] != 0 and np.count_nonzero(b) != 1
                   for m, a, b in zip(meta, l1, l0))
    assert flips >= 10 and dcs >= 3


@pytest.mark.gpu
@pytest.mark.parametrize("size", [4, 8, 16, 32, 64])
def test_gpu_quantize_full_rdoq_vs_reference(size):
    lib = _lib()
    z = np.load(os.path.join(GOLD, "rdoq_q.npz"))
    q = min(size, 16)
    for k, (coef, (qp, typ, cbp1, cbp0)) in enumerate(zip(z["q%d_coef" % size], z["q%d_meta" % size])):
        c = np.zeros((size, size), np.int16)
        c[:q, :q] = coef
        for rdoq, cbp, want in ((1, cbp1, z["q%d_lev1" % size][k]), (0, cbp0, z["q%d_lev0" % size][k])):
            got = np.full((size, size), SENTINEL, np.int16)
            r = lib.quantize(c.ctypes.data, got.ctypes.data, int(qp), size, int(typ), rdoq)
            assert r == int(cbp), (size, k, int(qp), int(typ), rdoq)
            assert np.array_equal(got[:q, :q], want), (size, k, int(qp), int(typ), rdoq)
            outside = np.ones((size, size), bool)
            outside[:q, :q] = False
            assert (got[outside] == SENTINEL).all(), (size, k, rdoq)  # outside q x q untouched
