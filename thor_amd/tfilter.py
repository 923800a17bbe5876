"""Temporal denoise on the device: a motion-compensated pre-filter of I420
source frames (thor_tf_create / thor_tf_i420, thor_amd/csrc/tf.hip).  The
arithmetic is specified in integers: a filtered frame is a
function of the source bytes, the same on every run.  Calls are enqueued,
nothing waits unless records are read back.  No fallback: a missing library or
device is an error."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import lib as L

# thor_tf_record_t; vectors in half-pel units of the luma plane
RECORD = np.dtype([("mvx", "i1"), ("mvy", "i1"), ("e", "<u2")])


def size_ok(w: int, h: int, nrefs: int = 1) -> bool:
    """thor_tf_check (host only)."""
    return L.load().thor_tf_check(w, h, nrefs) == 0


def mult(strength: int) -> int:
    """thor_tf_mult (host only)."""
    m = L.load().thor_tf_mult(strength)
    if m < 0:
        raise ValueError("strength: 1 .. 64, not %r" % (strength,))
    return m


def block_grid(w: int, h: int):
    """(bw8, bh8) of a w x h frame (thor_tf_blocks)."""
    bw, bh = C.c_int(0), C.c_int(0)
    if L.load().thor_tf_blocks(w, h, C.byref(bw), C.byref(bh)) < 0:
        raise ValueError("temporal filter: width, height multiples of 8 in 16 .. 16384, not %dx%d" % (w, h))
    return bw.value, bh.value


class TemporalFilter:
    """One frame size: the workspace (lookahead records and sums of the coarse
    stage, motion records) is allocated here, once; run() only launches.  Two
    run() calls of one filter must not overlap on different streams."""

    def __init__(self, w: int, h: int, max_targets: int = 1, device: int = 0):
        self.lib = L.load()
        if self.lib.thor_tf_check(w, h, 1) != 0:
            raise ValueError("temporal filter: width, height multiples of 8 in 16 .. 16384, not %dx%d" % (w, h))
        if not 1 <= max_targets <= L.THOR_TF_MAX_TARGETS:
            raise ValueError("max_targets: 1 .. %d, not %r" % (L.THOR_TF_MAX_TARGETS, max_targets))
        self.w, self.h, self.max_targets, self.device = w, h, max_targets, device
        self.h_ = self.lib.thor_tf_create(w, h, max_targets, device)
        if not self.h_:
            raise L.create_error("thor_tf_create")

    def run(self, cur, refs, dst, strength=(8, 3), records: bool = False, stream=None):
        """cur / dst: lists of n ThorYuvPlanes (DEVICE pointers, own strides); refs:
        a list of n lists of the same length 1 .. 4, an entry None for an absent
        reference.  Enqueued on `stream` (a hipStream_t as an int; default the null
        stream).  With `records` the motion records are read back behind the call
        on the same stream: a RECORD array (n, nrefs, bh8, bw8)."""
        n = len(cur)
        if n == 0 or len(dst) != n or len(refs) != n:
            raise ValueError("run: three non-empty lists of the same length")
        nrefs = len(refs[0])
        if any(len(r) != nrefs for r in refs):
            raise ValueError("run: every target takes the same number of references")
        none = L.ThorYuvPlanes(None, None, None, 0, 0)
        flat = [none if r is None else r for rs in refs for r in rs]
        sy, sc = strength
        bw8, bh8 = self.w >> 3, self.h >> 3
        recs = np.empty((n, nrefs, bh8, bw8), RECORD) if records else None
        d_recs = self.lib.thor_dev_alloc(max(recs.nbytes, 4)) if records else None
        if records and not d_recs:
            raise MemoryError("thor_dev_alloc")
        try:
            rc = self.lib.thor_tf_i420(self.h_, (L.ThorYuvPlanes * n)(*cur), (L.ThorYuvPlanes * max(len(flat), 1))(*flat),
                                       (L.ThorYuvPlanes * n)(*dst), n, nrefs, int(sy), int(sc), d_recs, stream or None)
            if rc == L.THOR_ERR_ARG:
                raise ValueError("thor_tf_i420: bad arguments (1 .. %d targets, 1 .. 4 references, strengths 1 .. 64, "
                                 "non-NULL planes, strides of at least a row, dst apart from cur and refs)" % self.max_targets)
            L.check(rc, "thor_tf_i420")
            if records and recs.nbytes:
                L.check(self.lib.thor_d2h_stream(recs.ctypes.data, d_recs, recs.nbytes, stream or None), "thor_d2h_stream")
        finally:
            if d_recs:
                self.lib.thor_dev_free(d_recs)
        return recs

    def close(self):
        if self.h_:
            self.lib.thor_tf_destroy(self.h_)
            self.h_ = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


def sequence_refs(k: int, nframes: int, radius: int):
    """The frames frame k is filtered from: k - radius .. k - 1, k + 1 .. k + radius; None where there is none."""
    return [j if 0 <= j < nframes else None for j in list(range(k - radius, k)) + list(range(k + 1, k + radius + 1))]


def filter_sequence(src_ptr: int, dst_ptr: int, nframes: int, w: int, h: int, radius: int = 2, strength=(8, 3),
                    stream=None, tf: TemporalFilter = None, device: int = 0):
    """`nframes` contiguous I420 frames at DEVICE address src_ptr (frame k at
    src_ptr + k * w*h*3/2) -> the same number at dst_ptr (another buffer).  Frame
    k is filtered from the UNFILTERED frames k - radius .. k + radius that exist
    (radius 1 or 2; the ends have fewer references): the filter is not
    recursive, so all frames are independent and go in one call.  `tf`: a
    TemporalFilter of this size with max_targets >= nframes to reuse; otherwise
    one is made here and freed after `stream` has been waited for."""
    from .scale import i420_planes

    if radius not in (1, 2):
        raise ValueError("radius: 1 or 2, not %r" % (radius,))
    if nframes < 1:
        raise ValueError("filter_sequence: no frames")
    fs = w * h * 3 // 2
    src = [i420_planes(src_ptr + k * fs, w, h) for k in range(nframes)]
    dst = [i420_planes(dst_ptr + k * fs, w, h) for k in range(nframes)]
    refs = [[None if j is None else src[j] for j in sequence_refs(k, nframes, radius)] for k in range(nframes)]
    own = tf is None
    if own:
        tf = TemporalFilter(w, h, nframes, device)
    elif (tf.w, tf.h) != (w, h) or tf.max_targets < nframes:
        raise ValueError("the filter is not one of %dx%d for %d targets" % (w, h, nframes))
    try:
        tf.run(src, refs, dst, strength, False, stream)
        if own:
            # the workspace must outlive the launches: wait for the stream (a one-byte read behind it)
            one = np.empty(1, np.uint8)
            L.check(tf.lib.thor_d2h_stream(one.ctypes.data, dst_ptr, 1, stream or None), "thor_d2h_stream")
    finally:
        if own:
            tf.close()
