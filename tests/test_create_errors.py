"""Create failures say why (thor_last_create_error): unsupported parameters are
THOR_ERR_ARG, exhausted HBM is THOR_ERR_NOMEM with the size of the allocation
that failed (a 320-stream run died on a bare
"thor_dec_create failed")."""
import ctypes as C

import pytest

from thor_amd import lib as L


def _dec_create(width, height, slots=34, device=0):
    lib = L.load()
    cs = L.ThorSeq(width, height, 0, 1, 1, 0, 0)
    return lib.thor_dec_create(C.byref(cs), device, slots)


def test_bad_size_is_arg_error_with_reason():
    """Rejected before any HIP call, so it runs without a GPU."""
    assert not _dec_create(1922, 1080)  # not a multiple of 8 (enc/strings.c:437)
    err = L.create_error("thor_dec_create")
    assert err.code == L.THOR_ERR_ARG
    assert "multiples of 8" in err.reason
    lib = L.load()
    assert not lib.thor_ti_create(0, 64, 0)
    assert L.create_error("thor_ti_create").code == L.THOR_ERR_ARG


@pytest.mark.gpu
def test_ring_over_descriptor_range_is_arg_error():
    """A ring k_recon's 32-bit buffer offsets cannot address."""
    assert not _dec_create(16384, 16384, slots=34)
    err = L.create_error("thor_dec_create")
    assert err.code == L.THOR_ERR_ARG and "2 GiB" in err.reason and err.bytes > 2 ** 31


@pytest.mark.gpu
def test_exhausted_hbm_is_nomem_with_bytes():
    """Take every byte of HBM the library's HIP runtime will hand out (8 GiB,
    then 256 MiB chunks), then ask for a 4K decoder (a 34-slot ring is 483 MB):
    THOR_ERR_NOMEM naming the ring and its size; once the memory is released
    the same create succeeds.  (No torch here: torch's own HIP runtime must not
    be initialised after the library's in this process.)"""
    from thor_amd.decoder import GpuDecoder
    from thor_amd.trace import SeqParams

    lib = L.load()
    held = []
    try:
        for chunk in (8 << 30, 256 << 20):
            while len(held) < 4096:
                p = lib.thor_dev_alloc(chunk)
                if not p:
                    break
                held.append(p)
        seq = SeqParams(3840, 2160, 0, 1, 4, 0, 0, 1, 1, 1, 0)
        with pytest.raises(L.CreateError) as ei:
            GpuDecoder(seq, device=0, slots=34)
        assert ei.value.code == L.THOR_ERR_NOMEM, str(ei.value)
        assert "reference ring" in ei.value.reason
        assert ei.value.bytes >= 34 * 3840 * 2160 * 3 // 2
    finally:
        for p in held:
            lib.thor_dev_free(p)
    d = GpuDecoder(seq, device=0, slots=34)
    d.close()
    assert L.create_error("thor_dec_create").code == L.THOR_OK


def _matrix():
    import json
    import os

    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "matrix.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("name", ["wrap_i", "wrap_p", "wrap_b"])
def test_frame_qp_below_zero_is_accepted(name):
    """Parameters whose frame QP computes below 0 (tests/golden/matrix.json,
    wrap_*) are the reference's to code -- at qp 51, its uint8_t frame QP
    wrapping (enc/mainenc.h:122, enc/mainenc.c:287) -- so thor_enc_check_params
    takes them.  No HIP call: runs without a GPU."""
    from thor_amd.encoder import params_for

    meta = _matrix()[name]
    p = params_for(meta["config"], meta["width"], meta["height"], meta["frames"], meta["extra"])
    assert 51 in [f["qp"] for f in meta["plan"]] and p.qp <= 1
    assert L.load().thor_enc_check_params(C.byref(p)) == 0


def test_interpolation_below_32_pixels_is_refused():
    """With min(width, height) < 32 the reference's interpolate_frames computes
    max_levels <= 0 and never writes the interpolated frame
    (common/temporal_interp.c:977-1033): the oracle and thor_ti_create refuse
    such a size instead of inventing one.  Runs without a GPU."""
    from oracle.py import PaddedFrame, interpolate_frames, load

    assert load().or_ti_levels(24, 200) < 1 <= load().or_ti_levels(32, 200)
    with pytest.raises(RuntimeError, match="or_interpolate_frames failed"):
        interpolate_frames(PaddedFrame(24, 200), PaddedFrame(24, 200), 2, 1)
    interpolate_frames(PaddedFrame(32, 200), PaddedFrame(32, 200), 2, 1)  # the smallest size it takes
    lib = L.load()
    assert not lib.thor_ti_create(24, 200, 0)
    err = L.create_error("thor_ti_create")
    assert err.code == L.THOR_ERR_ARG and "24x200" in err.reason


@pytest.mark.gpu
def test_encoder_and_decoder_with_interpolation_below_32_pixels_are_arg_errors():
    """thor_enc_create and thor_dec_create with interp_ref 1 at 24 x 200: NULL,
    THOR_ERR_ARG, and the reason names the size (the create's first cause, not
    a bare "HIP call failed")."""
    from thor_amd.encoder import params_for

    lib = L.load()
    p = params_for("config_HDB16_low_complexity.txt", 24, 200, 5)
    assert p.interp_ref == 1 and lib.thor_enc_check_params(C.byref(p)) == 0
    assert not lib.thor_enc_create(C.byref(p), 0)
    err = L.create_error("thor_enc_create")
    assert err.code == L.THOR_ERR_ARG and "24x200" in err.reason, str(err)
    cs = L.ThorSeq(24, 200, 1, 1, 1, 0, 1)
    assert cs.interp_ref == 1
    assert not lib.thor_dec_create(C.byref(cs), 0, 34)
    err = L.create_error("thor_dec_create")
    assert err.code == L.THOR_ERR_ARG and "24x200" in err.reason, str(err)
    # the same contexts without interpolated references are created
    p.interp_ref = 0
    e = lib.thor_enc_create(C.byref(p), 0)
    assert e
    lib.thor_enc_destroy(e)
    cs.interp_ref = 0
    d = lib.thor_dec_create(C.byref(cs), 0, 34)
    assert d
    lib.thor_dec_destroy(d)
