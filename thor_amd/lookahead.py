"""Frame analysis on the device: lookahead costs and scene cuts
(thor_lookahead_i420, thor_amd/csrc/lookahead.hip).  Per 16x16 source block a
cheap intra and inter cost on a half-resolution copy of the luma, and four sums
per frame.  The arithmetic is specified in integers: the
result is a function of the source bytes, the same on every run.  No fallback:
a missing library or device is an error."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import lib as L

# thor_la_block_t; vectors in lowres pixels (the source displacement is twice that)
BLOCK = np.dtype([("intra", "<u2"), ("inter", "<u2"), ("sad", "<u2"), ("mvx", "i1"), ("mvy", "i1")])
# the columns of a frame's sums
SUM_INTRA, SUM_INTER, SUM_MIN, NUM_INTRA = range(4)


def block_grid(w: int, h: int):
    """(bw, bh) of a w x h frame (thor_lookahead_blocks)."""
    bw, bh = C.c_int(0), C.c_int(0)
    if L.load().thor_lookahead_blocks(w, h, C.byref(bw), C.byref(bh)) < 0:
        raise ValueError("lookahead: 16 <= width, height <= 16384, not %dx%d" % (w, h))
    return bw.value, bh.value


def frame_costs(cur, ref, w: int, h: int, blocks: bool = False, stream=None):
    """thor_lookahead_i420 of the plane-set pairs (cur[i], ref[i]) (ThorYuvPlanes of
    DEVICE pointers; only luma is read; ref[i] None, or ref None: intra-only):
    uint64 array (n, 4) of sum intra, sum inter, sum min(intra, inter) and the
    number of blocks with intra < inter; with `blocks` also the records, a BLOCK
    array (n, bh, bw).  Enqueued on `stream` (a hipStream_t as an int; default the
    null stream); the results are read back behind it on the same stream."""
    lib = L.load()
    n = len(cur)
    if n == 0 or (ref is not None and len(ref) != n):
        raise ValueError("frame_costs: two non-empty lists of the same length")
    bw, bh = block_grid(w, h)
    none = L.ThorYuvPlanes(None, None, None, 0, 0)
    refs = (L.ThorYuvPlanes * n)(*[none if r is None else r for r in (ref if ref is not None else [None] * n)])
    sums = np.empty((n, 4), np.uint64)
    recs = np.empty((n, bh, bw), BLOCK) if blocks else None
    d_sums = lib.thor_dev_alloc(sums.nbytes)
    d_recs = lib.thor_dev_alloc(max(recs.nbytes, 8)) if blocks else None
    try:
        if not d_sums or (blocks and not d_recs):
            raise MemoryError("thor_dev_alloc")
        L.check(lib.thor_lookahead_i420((L.ThorYuvPlanes * n)(*cur), refs, n, w, h, d_recs, d_sums, stream or None),
                "thor_lookahead_i420")
        if blocks and recs.nbytes:
            L.check(lib.thor_d2h_stream(recs.ctypes.data, d_recs, recs.nbytes, stream or None), "thor_d2h_stream")
        L.check(lib.thor_d2h_stream(sums.ctypes.data, d_sums, sums.nbytes, stream or None), "thor_d2h_stream")
    finally:
        if d_recs:
            lib.thor_dev_free(d_recs)
        if d_sums:
            lib.thor_dev_free(d_sums)
    return (sums, recs) if blocks else sums


def sequence_costs(ptr: int, nframes: int, w: int, h: int, blocks: bool = False, stream=None):
    """frame_costs of `nframes` contiguous I420 frames at DEVICE address `ptr`
    (frame k at ptr + k * w*h*3/2): frame k against frame k - 1 in display order,
    frame 0 intra-only."""
    from .scale import i420_planes

    fs = w * h * 3 // 2
    cur = [i420_planes(ptr + k * fs, w, h) for k in range(nframes)]
    return frame_costs(cur, [None] + cur[:-1], w, h, blocks, stream)


def scene_cuts(sums, percent: int):
    """Indices of the frames of `sums` (n, 4) that thor_lookahead_scenecut calls a
    cut at `percent` (1..100): sum intra > 0 and 100 * sum min >= percent * sum intra."""
    lib = L.load()
    out = []
    for k, row in enumerate(np.asarray(sums, np.uint64).reshape(-1, 4)):
        rc = lib.thor_lookahead_scenecut((C.c_uint64 * 4)(*[int(v) for v in row]), int(percent))
        if rc < 0:
            raise ValueError("scene_cuts: percent is 1..100, not %r" % (percent,))
        if rc:
            out.append(k)
    return out
