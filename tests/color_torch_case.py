"""Child process of tests/test_gpu_color.py::test_torch_surfaces_in_a_child_process:
the torch-facing colour surfaces (GpuDecoder.read_rgb, GpuEncoder.set_input_rgb,
thor_amd.color) against the numpy model.  torch initialises the GPU first, then
the library.  Not collected by pytest; prints "ok: ..." as its last line."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import color_model as M  # noqa: E402
from conftest import trace_path  # noqa: E402
from thor_amd import lib as L  # noqa: E402


def _torch():
    import torch

    return torch


def _up(a):
    return _torch().from_numpy(np.ascontiguousarray(a)).cuda()


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
        raise AssertionError("%s: %d bytes differ, first at %s" % (what, bad.size, bad[:8].tolist()))


def _decoded(nframes=3):
    from thor_amd.decoder import GpuDecoder
    from thor_amd.trace import load_trace

    seq, frames = load_trace(trace_path("cif_low"))
    dec = GpuDecoder(seq)
    frames = frames[:nframes]
    for fr in frames:
        dec.decode(dec.upload(fr))
    return seq, frames, dec


def case_decoder():
    torch = _torch()
    seq, frames, dec = _decoded()
    W, H = seq.width, seq.height
    try:
        for fr in frames:
            y, u, v = dec.read(fr.frame_num)
            for chroma in ("nearest", "bilinear"):
                got = dec.read_rgb(fr.frame_num, matrix="bt601", chroma=chroma, layout="hwc")
                assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (H, W, 3)
                _same(got.cpu().numpy(), M.i420_to_rgb(y, u, v, 0, 0, chroma == "bilinear"), "read_rgb %s" % chroma)
            f = dec.read_rgb(fr.frame_num, full_range=True, dtype=torch.float32)
            assert f.dtype == torch.float32 and tuple(f.shape) == (3, H, W)
            _same(f.cpu().numpy(), M.i420_to_rgb(y, u, v, 1, 1, True, as_float=True).transpose(2, 0, 1), "float chw")
        never = max(fr.frame_num for fr in frames) + 100
        try:
            dec.read_rgb(never)
        except RuntimeError as e:
            assert "status -4" in str(e), e
        else:
            raise AssertionError("read_rgb of a frame never decoded did not raise")
    finally:
        dec.close()


def case_encoder():
    """set_input_rgb + encode_all == upload_sequence(model(rgb)) + encode_all,
    byte for byte; the stream decodes and read_rgb has the input's shape."""
    from thor_amd import synth
    from thor_amd.bitstream import parse_stream
    from thor_amd.decoder import GpuDecoder
    from thor_amd.encoder import GpuEncoder, params_for

    lib = L.load()
    lib.thor_enc_debug_stall(-1, 20000)  # a wedged launch gives up after 20 s instead of 5 minutes
    W, H, n = 64, 64, 3
    cfg = "config_LDB_low_complexity.txt"
    clip = synth.synth_frames(W, H, n, 5, workers=1)
    rgb = np.stack([M.i420_to_rgb(*M.split_i420(f, W, H), 1, 0, True) for f in clip])  # (n, H, W, 3)
    want_in = np.stack([M.join_i420(*M.rgb_to_i420(im, 1, 0)) for im in rgb])
    a = GpuEncoder(params_for(cfg, W, H, n))
    b = GpuEncoder(params_for(cfg, W, H, n))
    dec = None
    try:
        a.set_input_rgb(_up(rgb))
        got_in = np.empty(want_in.shape, np.uint8)
        assert lib.thor_d2h(got_in.ctypes.data, a.seq_dev, got_in.nbytes) == 0
        _same(got_in, want_in, "converted input sequence")
        bits = a.encode_all()
        b.upload_sequence(want_in)
        assert bits == b.encode_all()
        # the same from planar float input of the same bytes
        a.reset()
        a.set_input_rgb(_up(M.byte_to_float(rgb).transpose(0, 3, 1, 2)))
        assert a.encode_all() == bits
        seq, frames = parse_stream(bits)
        assert len(frames) == n
        dec = GpuDecoder(seq)
        for fr in frames:
            dec.decode(dec.upload(fr))
            out = dec.read_rgb(fr.frame_num, layout="hwc")
            assert tuple(out.shape) == rgb.shape[1:]
    finally:
        lib.thor_enc_debug_stall(-1, 0)
        a.close()
        b.close()
        if dec is not None:
            dec.close()


def case_interop():
    """Input produced and output consumed by torch ops on a non-default stream,
    no explicit synchronisation in between; documented shapes and dtypes; a crop
    of a larger tensor converts through its strides."""
    torch = _torch()
    from thor_amd import color

    W, H, n = 40, 24, 3
    rng = np.random.default_rng(3)
    frames = rng.integers(0, 256, (n, H * 3 // 2, W), dtype=np.uint8)
    host = _up(frames)
    big = rng.integers(0, 256, (n, H + 10, W + 14, 3), dtype=np.uint8)
    big_dev = _up(big)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        x = host ^ 0x5A  # produced on `side`
        hwc = color.i420_to_rgb(x, W, H, matrix="bt601", full_range=True, chroma="nearest", layout="hwc")
        chw = color.i420_to_rgb(x.reshape(n, -1), W, H)
        flt = color.i420_to_rgb(x, W, H, dtype=torch.float32)
        s_hwc, s_chw, s_flt = (t.to(torch.float64).sum() for t in (hwc, chw, flt))  # consumed on `side`
        crop = big_dev[:, 4:4 + H, 6:6 + W, :]
        assert not crop.is_contiguous()
        back = color.rgb_to_i420(crop + 0, matrix="bt601")  # a fresh tensor made on `side`
        back_view = color.rgb_to_i420(crop, matrix="bt601")
        back_chw = color.rgb_to_i420(crop.permute(0, 3, 1, 2), matrix="bt601", layout="chw")  # innermost not dense
        back_f = color.rgb_to_i420(flt, full_range=True)
        total = back.to(torch.int64).sum() + back_view.to(torch.int64).sum()
    side.synchronize()
    assert hwc.is_cuda and hwc.dtype == torch.uint8 and tuple(hwc.shape) == (n, H, W, 3)
    assert chw.dtype == torch.uint8 and tuple(chw.shape) == (n, 3, H, W)
    assert flt.dtype == torch.float32 and tuple(flt.shape) == (n, 3, H, W)
    assert tuple(back.shape) == (n, H * 3 // 2, W) and back.dtype == torch.uint8
    xs = frames ^ 0x5A
    w_hwc = np.stack([M.i420_to_rgb(*M.split_i420(f, W, H), 0, 1, False) for f in xs])
    w_chw = np.stack([M.i420_to_rgb(*M.split_i420(f, W, H), 1, 0, True) for f in xs])
    _same(hwc.cpu().numpy(), w_hwc, "hwc")
    _same(chw.cpu().numpy(), w_chw.transpose(0, 3, 1, 2), "chw")
    _same(flt.cpu().numpy(), M.byte_to_float(w_chw).transpose(0, 3, 1, 2), "float")
    assert int(s_hwc.item()) == int(w_hwc.astype(np.int64).sum()) and int(s_chw.item()) == int(w_chw.astype(np.int64).sum())
    assert abs(float(s_flt.item()) - float(M.byte_to_float(w_chw).astype(np.float64).sum())) < 1e-6 * w_chw.size
    cw = big[:, 4:4 + H, 6:6 + W, :]
    w_back = np.stack([M.join_i420(*M.rgb_to_i420(im, 0, 0)) for im in cw]).reshape(n, H * 3 // 2, W)
    _same(back.cpu().numpy(), w_back, "rgb_to_i420 of a fresh tensor")
    _same(back_view.cpu().numpy(), w_back, "rgb_to_i420 through a crop's strides")
    _same(back_chw.cpu().numpy(), w_back, "rgb_to_i420 of a permuted view")
    assert int(total.item()) == 2 * int(w_back.astype(np.int64).sum())
    w_back_f = np.stack([M.join_i420(*M.rgb_to_i420(im, 1, 1)) for im in w_chw]).reshape(n, H * 3 // 2, W)
    _same(back_f.cpu().numpy(), w_back_f, "rgb_to_i420 of the float tensor")


if __name__ == "__main__":
    _torch().zeros(1).cuda()  # torch's runtime first
    case_decoder()
    case_encoder()
    case_interop()
    print("ok: decoder, encoder, interop")
