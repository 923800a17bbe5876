// Single translation unit for libthor_amd.so (no relocatable device code).
#include "recon.hip"
#include "resid.hip"
#include "txq.hip"
#include "inter.hip"
#include "intra.hip"
#include "loopfilter.hip"
#include "pyramid.hip"
#include "interp.hip"
#include "tme.hip"
#include "capi.hip"
// The six frame utilities: each includes frame_ops.h for what they share.  They follow capi.hip (the
// decoder context, find_slot_host and HIPCHK of their thor_dec_frame_* entry points).  Among themselves
// and towards the encoder any order compiles: a file that calls another's function declares it (tf.hip:
// la_enqueue of lookahead.hip; enc.hip: sse_enqueue, ssim_enqueue; enc_seq.hip: sse_wave_band of
// quality.hip), and scale.hip reaches color.hip's thor_dec_frame_planes through the public header.
#include "quality.hip"
#include "color.hip"
#include "scale.hip"
#include "ssim.hip"
#include "lookahead.hip"
#include "tf.hip"
#include "enc.hip"
#include "enc_seq.hip"
#include "parse.hip"
#include "simd_surface.hip"
#include "l2_surface.hip"
