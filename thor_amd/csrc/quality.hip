// Frame quality measured on the device: the sum of squared errors of I420
// frame pairs (include/thor_amd.h: thor_sse_i420, thor_psnr, thor_dec_frame_sse;
// the encoder's use of it is in enc.hip / enc_seq.hip).  What the reference
// computes on the host per coded frame (snr_yuv, common/snr.c:32-89, called at
// enc/mainenc.c:522-531), here a bandwidth-bound reduction over frames that
// already live in HBM: two reads of each frame, three 64-bit sums out.
//
// The sums are exact integers, so the order of summation does not matter:
// every wave adds its band's sum to the pair's 64-bit totals with one integer
// atomic per plane.
// The decoder context, find_slot_host and HIPCHK are capi.hip's.
#include <math.h>

#include "frame_ops.h"

#define SSE_BAND 8  // luma rows (and the 4 chroma rows under them) per wave
#define SSE_INL 8   // frame pairs that travel in the kernel arguments (64 bytes each)
// One wave sums at most SSE_SPILL lane passes of 16 pixels in 32 bits before it
// spills to 64: 64 lanes x 64 passes x 16 = 65 536 pixels <= floor(2^32 / 255^2) = 66 051,
// the most a 32-bit sum of squared byte differences is guaranteed to hold.
#define SSE_SPILL 64
static_assert(64LL * SSE_SPILL * 16 * 255 * 255 < (1LL << 32), "a wave's 32-bit partial must hold its pixels");

struct SseArgs {
  const SsePair *dev;  // the pairs in device memory, or nullptr: inl[]
  unsigned long long *sse;  // [3 * pairs], zero before the launch
  int W, H;
  SsePair inl[SSE_INL];
};
static_assert(sizeof(SseArgs) <= 1024, "the pairs travel in the kernarg segment");

// Wave sum of a 32-bit value (all 64 lanes active, wave-uniform call site).  frame_ops.h's wave_reduce but for
// its last step: that one folds the four rows pairwise, and the compiler schedules the pairwise sum differently
// from the chain this kernel has always had, so the chain stays.
__device__ __forceinline__ uint32_t sse_wave_sum(uint32_t v) {
  v = row_reduce(v, OpSum());
  return (uint32_t)__builtin_amdgcn_readlane((int)v, 0) + (uint32_t)__builtin_amdgcn_readlane((int)v, 16) +
         (uint32_t)__builtin_amdgcn_readlane((int)v, 32) + (uint32_t)__builtin_amdgcn_readlane((int)v, 48);
}

// Sum of (a - b)^2 over rows [r0, r1) of a w-pixel-wide plane, by one wave
// (every lane calls it with the same arguments; the result is uniform).
// A lane pass takes 16 pixels of one row: the passes of the band are numbered
// row-major (nc = ceil(w / 16) per row) and dealt to the lanes round-robin, so
// narrow planes keep every lane busy.  16-byte loads when both pointers and
// both strides are 16-byte aligned, else four (unaligned) dword loads; a row's
// last pass (w % 16 pixels) takes dwords, then single bytes.
// Four pixels cost three packed dot products: sum (a - b)^2 = sum a^2 + sum b^2 - 2 sum ab.
// The three 32-bit sums may wrap; their combination is the true partial modulo
// 2^32, and the true partial fits: it is spilled to the 64-bit total after
// SSE_SPILL passes per lane (65 536 pixels per wave, the limit is 66 051).
__device__ __forceinline__ unsigned long long sse_wave_rows(const uint8_t *a_, int as, const uint8_t *b_, int bs, int w,
                                                            int r0, int r1) {
  const gcptr a = (gcptr)a_, b = (gcptr)b_;
  const int lane = threadIdx.x & 63;
  const int nc = (w + 15) >> 4, total = (r1 - r0) * nc;
  if (total <= 0) return 0;
  const bool wide = (((uintptr_t)a | (uintptr_t)b | (uintptr_t)(unsigned)as | (uintptr_t)(unsigned)bs) & 15) == 0;
  const int dq = 64 / nc, dr = 64 - dq * nc;  // a step of 64 passes = dq rows + dr passes
  int row = lane / nc, c = lane - row * nc;
  unsigned long long tot = 0;
  uint32_t s = 0, ab = 0;
  int held = 0;
  for (int g0 = 0; g0 < total; g0 += 64) {
    if (g0 + lane < total) {
      const int x = c << 4, n = min(16, w - x);
      const gcptr pa = a + (long long)(r0 + row) * as + x, pb = b + (long long)(r0 + row) * bs + x;
      if (n == 16) {
        u32x4 u, v;
        if (wide) {
          u = *(gcptr16)pa;
          v = *(gcptr16)pb;
        } else {
          u = g_ld4x4(pa);
          v = g_ld4x4(pb);
        }
        s = __builtin_amdgcn_udot4(u.x, u.x, s, false);
        s = __builtin_amdgcn_udot4(v.x, v.x, s, false);
        ab = __builtin_amdgcn_udot4(u.x, v.x, ab, false);
        s = __builtin_amdgcn_udot4(u.y, u.y, s, false);
        s = __builtin_amdgcn_udot4(v.y, v.y, s, false);
        ab = __builtin_amdgcn_udot4(u.y, v.y, ab, false);
        s = __builtin_amdgcn_udot4(u.z, u.z, s, false);
        s = __builtin_amdgcn_udot4(v.z, v.z, s, false);
        ab = __builtin_amdgcn_udot4(u.z, v.z, ab, false);
        s = __builtin_amdgcn_udot4(u.w, u.w, s, false);
        s = __builtin_amdgcn_udot4(v.w, v.w, s, false);
        ab = __builtin_amdgcn_udot4(u.w, v.w, ab, false);
      } else {
        int j = 0;
        for (; j + 4 <= n; j += 4) {
          const uint32_t u = g_ld4(pa + j), v = g_ld4(pb + j);
          s = __builtin_amdgcn_udot4(u, u, s, false);
          s = __builtin_amdgcn_udot4(v, v, s, false);
          ab = __builtin_amdgcn_udot4(u, v, ab, false);
        }
        for (; j < n; j++) {
          const int d = (int)pa[j] - (int)pb[j];
          s += (uint32_t)(d * d);
        }
      }
    }
    row += dq;
    c += dr;
    if (c >= nc) c -= nc, row++;
    if (++held == SSE_SPILL) {  // the spill to 64 bits (uniform: every lane has made `held` passes at most)
      tot += sse_wave_sum(s - 2u * ab);
      s = ab = 0;
      held = 0;
    }
  }
  if (held) tot += sse_wave_sum(s - 2u * ab);
  return tot;
}

// The three sums of luma rows [r0, r1) and the chroma rows under them, added to sse[0..2] (one wave).
__device__ __forceinline__ void sse_wave_band(const SsePair &P, int W, int H, int r0, int r1, unsigned long long *sse) {
  const int lane = threadIdx.x & 63;
  const int c0 = r0 >> 1, c1 = min(r1 >> 1, H >> 1);
  const unsigned long long y = sse_wave_rows(P.a[0], P.as[0], P.b[0], P.bs[0], W, r0, r1);
  const unsigned long long u = sse_wave_rows(P.a[1], P.as[1], P.b[1], P.bs[1], W >> 1, c0, c1);
  const unsigned long long v = sse_wave_rows(P.a[2], P.as[1], P.b[2], P.bs[1], W >> 1, c0, c1);
  if (lane == 0) {
    if (y) atomicAdd(&sse[0], y);
    if (u) atomicAdd(&sse[1], u);
    if (v) atomicAdd(&sse[2], v);
  }
}

// grid (ceil(H / (4 * SSE_BAND)), pairs), 256 threads: wave w of block x takes luma rows
// [(4 x + w) SSE_BAND, + SSE_BAND) of pair blockIdx.y.  Bandwidth bound: ~40 VGPRs, no LDS,
// so every CU holds its full complement of waves to cover the loads.
__global__ __launch_bounds__(256) void k_sse_i420(const SseArgs A) {
  const int i = blockIdx.y;
  // (the inline pairs are read in place in the kernarg segment: a dynamic index into the by-value
  // argument would copy it to scratch)
  const SsePair *pp = A.dev ? A.dev + i : ((const SseArgs *)__builtin_amdgcn_kernarg_segment_ptr())->inl + i;
  const int r0 = (blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6)) * SSE_BAND;  // (uniform: SGPRs)
  if (r0 >= A.H) return;
  const SsePair P = *pp;
  sse_wave_band(P, A.W, A.H, r0, min(r0 + SSE_BAND, A.H), A.sse + 3 * (size_t)i);
}

// Zero the sums and launch k_sse_i420 for n pairs on `st`: the pairs in device memory (`dev`, one
// launch) or on the host (`host`, SSE_INL per launch through the kernel arguments).
static int sse_enqueue(const SsePair *dev, const SsePair *host, int n, int W, int H, unsigned long long *sse,
                       hipStream_t st) {
  if (zero_sums(sse, (size_t)n * 3, st) != THOR_OK) return THOR_ERR_HIP;
  const unsigned gx = (unsigned)((H + 4 * SSE_BAND - 1) / (4 * SSE_BAND));
  SseArgs A;
  memset(&A, 0, sizeof(A));
  A.W = W;
  A.H = H;
  A.dev = dev;
  return launch_batches(n, dev ? n : SSE_INL, [&](int i0, int m) {
    if (!dev) memcpy(A.inl, host + i0, (size_t)m * sizeof(SsePair));
    A.sse = sse + 3 * (size_t)i0;
    k_sse_i420<<<dim3(gx, (unsigned)m), 256, 0, st>>>(A);
  });
}

extern "C" {

int thor_sse_i420(const thor_yuv_planes_t *a, const thor_yuv_planes_t *b, int n, int width, int height, uint64_t *sse,
                  void *stream) {
  if (!a || !b || !sse || n <= 0 || n > 65535 || width < 2 || height < 2) return THOR_ERR_ARG;
  std::vector<SsePair> pairs((size_t)n);
  for (int i = 0; i < n; i++)
    if (!sse_fill_pair(pairs[i], a[i], b[i])) return THOR_ERR_ARG;
  return sse_enqueue(nullptr, pairs.data(), n, width, height, (unsigned long long *)sse, (hipStream_t)stream);
}

// snr_yuv's arithmetic (common/snr.c:60-61): plse = sumsqr / (65025.0 * ydim * xdim) with the
// dimensions unsigned, psnr = -10 * log10(plse); a sum of 0 gives +inf there too.
double thor_psnr(uint64_t sse, int width, int height) {
  const double plse = (double)sse / (65025.0 * (unsigned)height * (unsigned)width);
  return -10 * log10(plse);
}

int thor_dec_frame_sse(thor_dec_t *d, int frame_num, const thor_yuv_planes_t *orig, uint64_t *sse_dev) {
  if (!d || !orig || !sse_dev) return THOR_ERR_ARG;
  const int s = find_slot_host(d, frame_num);
  if (s < 0) return THOR_ERR_REF;
  SsePair P;
  if (!sse_fill_pair(P, *orig, slot_planes(d, s))) return THOR_ERR_ARG;
  HIPCHK(hipSetDevice(d->device));
  return sse_enqueue(nullptr, &P, 1, d->seq.width, d->seq.height, (unsigned long long *)sse_dev, d->stream);
}

}  // extern "C"
