// The common ground of the frame utilities that work on I420 planes in HBM:
// quality.hip (SSE / PSNR), ssim.hip, lookahead.hip, tf.hip, color.hip and
// scale.hip, and of what enc.hip / enc_seq.hip use of them.  Global-memory access
// types, the 16-lane-row and wave reductions, the edge-clamped four-pixel load,
// the plane-pair descriptors and the host side every entry point repeats:
// argument checks, a decoder or encoder slot as a plane set, the zeroing of the
// sums and the launch loop over descriptors that travel in the kernel arguments.
// A new frame utility starts from this header and includes it explicitly.
//
// Only helpers: no kernel lives here, and the *Args structs that kernels take by
// value stay with their kernels.
#pragma once
#include "common.h"

// ---- global memory -------------------------------------------------------------------------------------------
// The planes are in global memory: accesses through pointers of that address space are global_load_* /
// global_store_* (the generic pointers of a plane set would make them flat_*, which wait on both memory
// counters and cannot take the unaligned dword form).  The global forms take any alignment -- also in their
// 8- and 16-byte forms, so one instruction per row segment serves aligned and unaligned images alike (the
// memory pipeline splits what straddles).
typedef __attribute__((address_space(1))) uint8_t *gptr;
typedef const __attribute__((address_space(1))) uint8_t *gcptr;
typedef __attribute__((address_space(1))) float *gptrf;
typedef const __attribute__((address_space(1))) float *gcptrf;
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));  // (native vectors: loads through an address-space pointer)
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(1))) u32x4 *gcptr16;  // an aligned 16-byte load
typedef uint32_t __attribute__((aligned(1))) u32u;
typedef u32x2 __attribute__((aligned(1))) u32x2u;
typedef f32x4 __attribute__((aligned(4))) f32x4u;  // (float images are 4-byte aligned: include/thor_amd.h)

__device__ __forceinline__ uint32_t g_ld4(gcptr p) { return *(const __attribute__((address_space(1))) u32u *)p; }
__device__ __forceinline__ void g_st4(gptr p, uint32_t v) { *(__attribute__((address_space(1))) u32u *)p = v; }
__device__ __forceinline__ u32x2 g_ld8(gcptr p) { return *(const __attribute__((address_space(1))) u32x2u *)p; }
__device__ __forceinline__ void g_st8(gptr p, u32x2 v) { *(__attribute__((address_space(1))) u32x2u *)p = v; }
__device__ __forceinline__ f32x4 g_ld16f(gcptrf p) { return *(const __attribute__((address_space(1))) f32x4u *)p; }
__device__ __forceinline__ void g_st16f(gptrf p, f32x4 v) { *(__attribute__((address_space(1))) f32x4u *)p = v; }
// four unaligned dwords: what a 16-byte load takes where pointer or stride are not 16-byte aligned
__device__ __forceinline__ u32x4 g_ld4x4(gcptr p) { return u32x4{g_ld4(p), g_ld4(p + 4), g_ld4(p + 8), g_ld4(p + 12)}; }

// Four pixels (x .. x + 3, row y; both clamped to the plane) of plane p, packed in a dword: one (unaligned) dword
// load inside the plane, pixel by pixel across its edge.  Nothing is read outside the plane.
__device__ __forceinline__ uint32_t ld4_clamped(gcptr p, int stride, int x, int y, int w, int h) {
  const gcptr r = p + (long long)min(max(y, 0), h - 1) * stride;
  if (x >= 0 && x + 3 < w) return g_ld4(r + x);
  uint32_t out = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) out |= (uint32_t)r[min(max(x + k, 0), w - 1)] << (8 * k);
  return out;
}

// ---- rows and waves ------------------------------------------------------------------------------------------
// A DPP move inside the 16-lane rows (all lanes active: every lane has a source).
template <int CTRL>
__device__ __forceinline__ uint32_t dpp_mov(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, CTRL, 0xF, 0xF, false);
}
// The value of lane ^ (1 << BIT) of the same row, BIT 0..3.  ^1 and ^2 are quad permutations, ^8 a rotation by
// half a row; ^4 is row_half_mirror (^7) followed by a reversal of every quad (^3).
template <int BIT>
__device__ __forceinline__ uint32_t row_xor(uint32_t v) {
  if (BIT == 0) return dpp_mov<0xB1>(v);                 // quad_perm [1,0,3,2]
  if (BIT == 1) return dpp_mov<0x4E>(v);                 // quad_perm [2,3,0,1]
  if (BIT == 2) return dpp_mov<0x1B>(dpp_mov<0x141>(v));  // quad_perm [3,2,1,0] of row_half_mirror
  return dpp_mov<0x128>(v);                              // row_ror:8
}
// The operations of the reductions below, as accumulations in place (a op= b).
struct OpSum {
  __device__ __forceinline__ void operator()(uint32_t &a, uint32_t b) const { a += b; }
};
struct OpMin {
  __device__ __forceinline__ void operator()(uint32_t &a, uint32_t b) const { a = min(a, b); }
};
// Every lane: `v` reduced over its 16-lane row (all lanes active).
template <class Op>
__device__ __forceinline__ uint32_t row_reduce(uint32_t v, Op op) {
  op(v, dpp_mov<0xB1>(v));   // quad_perm [1,0,3,2]
  op(v, dpp_mov<0x4E>(v));   // quad_perm [2,3,0,1]
  op(v, dpp_mov<0x141>(v));  // row_half_mirror
  op(v, dpp_mov<0x140>(v));  // row_mirror
  return v;
}
// `v` reduced over the wave, uniform (all 64 lanes active, wave-uniform call site): DPP inside each 16-lane row,
// the four rows through readlane, folded pairwise (enc_core.h's te_sum).
template <class Op>
__device__ __forceinline__ uint32_t wave_reduce(uint32_t v, Op op) {
  v = row_reduce(v, op);
  uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)v, 0);
  op(lo, (uint32_t)__builtin_amdgcn_readlane((int)v, 16));
  uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)v, 32);
  op(hi, (uint32_t)__builtin_amdgcn_readlane((int)v, 48));
  op(lo, hi);
  return lo;
}
// Wave sum of a 64-bit value (all 64 lanes active, wave-uniform call site).
__device__ __forceinline__ long long wave_sum64(long long v) {
#pragma unroll
  for (int m = 32; m; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// ---- plane pairs ---------------------------------------------------------------------------------------------
// Two I420 frames to compare (k_sse_i420, k_ssim_i420; 64 bytes in the kernel arguments).
struct SsePair {
  const uint8_t *a[3], *b[3];  // Y, U, V interior (0, 0)
  int as[2], bs[2];            // luma / chroma stride
};
// The luma of a frame and of its reference (k_lookahead; 24 bytes in the kernel arguments).
struct LaPair {
  const uint8_t *cur, *ref;  // luma interior (0, 0); ref nullptr: an intra-only pair
  int cs, rs;                // strides
};
// The lookahead's half-resolution plane (lw x lh) and its 8x8 blocks (bw x bh) of a W x H frame.
static inline void la_dims(int W, int H, int &lw, int &lh, int &bw, int &bh) {
  lw = W >> 1, lh = H >> 1;
  bw = lw >> 3, bh = lh >> 3;
}

// ---- host side -----------------------------------------------------------------------------------------------
static inline bool planes_present(const thor_yuv_planes_t &p) { return p.y && p.u && p.v; }
// Three planes, every stride at least a row of a W-pixel-wide frame.
static inline bool planes_ok(const thor_yuv_planes_t &p, int W) {
  return planes_present(p) && p.stride_y >= W && p.stride_c >= (W >> 1);
}
// (the strides are the caller's to check: thor_sse_i420 and thor_ssim_i420 take them as they come)
static inline bool sse_fill_pair(SsePair &P, const thor_yuv_planes_t &a, const thor_yuv_planes_t &b) {
  if (!planes_present(a) || !planes_present(b)) return false;
  P.a[0] = a.y, P.a[1] = a.u, P.a[2] = a.v;
  P.b[0] = b.y, P.b[1] = b.u, P.b[2] = b.v;
  P.as[0] = a.stride_y, P.as[1] = a.stride_c;
  P.bs[0] = b.stride_y, P.bs[1] = b.stride_c;
  return true;
}
// The luma of `cur` against the luma of `ref`; ref nullptr or without a luma plane: an intra-only pair.
static inline void la_fill_pair(LaPair &P, const thor_yuv_planes_t &cur, const thor_yuv_planes_t *ref) {
  P.cur = cur.y, P.cs = cur.stride_y;
  P.ref = nullptr, P.rs = 0;
  if (ref && ref->y) P.ref = ref->y, P.rs = ref->stride_y;
}

// Slot `slot` of a decoder's or an encoder's reference ring as a plane set (thor_dec, thor_enc: the same members).
template <class Ctx>
static inline thor_yuv_planes_t slot_planes(const Ctx *c, int slot) {
  uint8_t *base = c->slots + (long long)slot * c->slot_bytes;
  return thor_yuv_planes_t{base + c->offy, base + c->offu, base + c->offv, c->sy, c->sc};
}

// Zero `count` 64-bit sums on `st`: THOR_OK or THOR_ERR_HIP.
static inline int zero_sums(unsigned long long *sums, size_t count, hipStream_t st) {
  if (hipMemsetAsync(sums, 0, count * sizeof(unsigned long long), st) == hipSuccess) return THOR_OK;
  (void)hipGetLastError();
  return THOR_ERR_HIP;
}
// n descriptors, at most `inl` per launch: launch(i0, m) enqueues descriptors [i0, i0 + m).  THOR_OK, or
// THOR_ERR_HIP if a launch was refused.
template <class Launch>
static inline int launch_batches(int n, int inl, Launch launch) {
  for (int i0 = 0; i0 < n; i0 += inl) launch(i0, n - i0 < inl ? n - i0 : inl);
  return hipGetLastError() == hipSuccess ? THOR_OK : THOR_ERR_HIP;
}
