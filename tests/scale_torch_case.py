"""Child process of tests/test_gpu_scale.py::test_torch_surface_in_a_child_process:
thor_amd.scale.scale_i420 with torch tensors and streams against the Python
model.  torch initialises the GPU first, then the library.  Not collected by
pytest; prints "ok: ..." as its last line."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import scale_model as M  # noqa: E402


def main():
    import torch

    from thor_amd import scale

    sw, sh, dw, dh, n = 40, 24, 24, 40, 3
    rng = np.random.default_rng(5)
    frames = rng.integers(0, 256, (n, sh * 3 // 2, sw), dtype=np.uint8)
    dev = torch.from_numpy(frames).cuda()
    for name, f in scale.FILTERS.items():
        want = M.scale_frames(frames.reshape(n, -1), sw, sh, dw, dh, f)
        out = scale.scale_i420(dev, sw, sh, dw, dh, filter=name)
        assert out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == (n, dh * 3 // 2, dw)
        assert np.array_equal(out.cpu().numpy().reshape(n, -1), want), name
        # produced and consumed by torch ops on a side stream, a kept scaler, no explicit synchronisation
        sc = scale.Scaler(sw, sh, dw, dh, name, 0)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        try:
            with torch.cuda.stream(side):
                src = dev.flatten(1) ^ 0x55
                got = scale.scale_i420(src, sw, sh, dw, dh, filter=name, scaler=sc)
                total = got.to(torch.int64).sum()
            side.synchronize()
            want2 = M.scale_frames(frames.reshape(n, -1) ^ 0x55, sw, sh, dw, dh, f)
            assert np.array_equal(got.cpu().numpy().reshape(n, -1), want2), name
            assert int(total.item()) == int(want2.astype(np.int64).sum())
        finally:
            sc.close()
    for bad in (dev.float(), dev.cpu(), dev[:, :-1]):
        try:
            scale.scale_i420(bad, sw, sh, dw, dh)
        except ValueError:
            pass
        else:
            raise AssertionError("scale_i420 accepted a wrong tensor")
    print("ok: scale_i420")


if __name__ == "__main__":
    main()
