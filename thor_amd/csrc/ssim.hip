// Frame quality measured on the device: SSIM of I420 frame pairs in the x264 /
// ffmpeg layout (include/thor_amd.h: thor_ssim_i420, thor_ssim, thor_dec_frame_ssim;
// the encoder's thor_enc_recon_ssim is in enc.hip).  The contract is DESIGN.md
// sec. 7e: 4x4 block sums, 8x8 windows on a 4-pixel grid, every window's value
// quantised to an integer q = rint(ssim * 2^30), three 64-bit sums of q out.
// The reference has no SSIM: the integer contract is the specification, and
// tests/ssim_model.py restates it in numpy.
//
// The sums are exact integers, so the order of summation does not matter:
// every wave adds its windows' sum to the pair's 64-bit plane total with one
// integer atomic (two's complement: q is negative where the covariance is).
// The decoder context, find_slot_host and HIPCHK are capi.hip's.
#include <math.h>

#include "frame_ops.h"

#define SSIM_BAND 16   // window rows per wave: SSIM_BAND + 1 block rows are read
#define SSIM_LANES 63  // lanes of a wave that own windows: four each; lane 63 only lends lane 62 its first block
#define SSIM_TILE (4 * SSIM_LANES)  // window columns per wave: 252 (tiles start on multiples of 1008 pixels)
#define SSIM_INL 8     // frame pairs that travel in the kernel arguments (64 bytes each)
#define SSIM_C1 416    // ffmpeg's integers for 8-bit samples and 64-pixel windows
#define SSIM_C2 235963

struct SsimArgs {
  unsigned long long *sums;  // [3 * pairs], zero before the launch
  int W, H;
  SsePair inl[SSIM_INL];
};
static_assert(sizeof(SsimArgs) <= 1024, "the pairs travel in the kernarg segment");

// Tiles and bands of a plane of bw x bh blocks: (bw - 1) x (bh - 1) windows.
static __host__ __device__ inline int ssim_tiles(int bw) { return (bw - 1 + SSIM_TILE - 1) / SSIM_TILE; }
static __host__ __device__ inline int ssim_bands(int bh) { return (bh - 1 + SSIM_BAND - 1) / SSIM_BAND; }

// The sums of one block row's four 4x4 blocks of this lane: s12[k] = sum a b, ss[k] = sum a^2 + sum b^2,
// p[k] = sum a | sum b << 16 (each <= 4080: the two stay apart through the window's four blocks, <= 16 320).
// pa / pb: the lane's first pixel of the block row; nb: how many of its four blocks lie inside the plane
// (FULL: four in every lane; wide: 16-byte loads).  Nothing is read outside those nb blocks.
template <bool FULL>
__device__ __forceinline__ void ssim_block_row(gcptr pa, int as, gcptr pb, int bs, int nb, bool wide, uint32_t p[4],
                                               uint32_t ss[4], uint32_t s12[4]) {
  uint32_t s1[4] = {0, 0, 0, 0}, s2[4] = {0, 0, 0, 0};
#pragma unroll
  for (int k = 0; k < 4; k++) ss[k] = s12[k] = 0;
#pragma unroll
  for (int y = 0; y < 4; y++) {
    const gcptr ra = pa + (long long)y * as, rb = pb + (long long)y * bs;
    u32x4 u = {0, 0, 0, 0}, v = {0, 0, 0, 0};
    if (FULL || nb == 4) {
      if (wide) {
        u = *(gcptr16)ra;
        v = *(gcptr16)rb;
      } else {
        u = g_ld4x4(ra);
        v = g_ld4x4(rb);
      }
    } else {
      if (nb > 0) u.x = g_ld4(ra), v.x = g_ld4(rb);
      if (nb > 1) u.y = g_ld4(ra + 4), v.y = g_ld4(rb + 4);
      if (nb > 2) u.z = g_ld4(ra + 8), v.z = g_ld4(rb + 8);
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
      s1[k] = __builtin_amdgcn_udot4(u[k], 0x01010101u, s1[k], false);
      s2[k] = __builtin_amdgcn_udot4(v[k], 0x01010101u, s2[k], false);
      ss[k] = __builtin_amdgcn_udot4(u[k], u[k], ss[k], false);
      ss[k] = __builtin_amdgcn_udot4(v[k], v[k], ss[k], false);
      s12[k] = __builtin_amdgcn_udot4(u[k], v[k], s12[k], false);
    }
  }
#pragma unroll
  for (int k = 0; k < 4; k++) p[k] = s1[k] | (s2[k] << 16);
}

// One window's q = rint(ssim * 2^30) from its four sums.  Every integer fits in
// 32 bits (|A1|, |B1| <= 532 685 216; |A2|, |B2| <= 532 920 763) and is exact in a double; two
// multiplies, one true divide, the exact scale and rint: no add, so nothing can be contracted.
__device__ __forceinline__ int ssim_q(uint32_t s1, uint32_t s2, uint32_t ss, uint32_t s12) {
  const int m11 = (int)(s1 * s1), m22 = (int)(s2 * s2), m12 = (int)(s1 * s2);
  const int vars = (int)(64u * ss) - m11 - m22, covar = (int)(64u * s12) - m12;
  const int A1 = 2 * m12 + SSIM_C1, B1 = m11 + m22 + SSIM_C1;
  const int A2 = 2 * covar + SSIM_C2, B2 = vars + SSIM_C2;
  const double q = ((double)A1 * (double)A2) / ((double)B1 * (double)B2) * 1073741824.0;
  return (int)__builtin_rint(q);
}

// The sum of q over the windows one wave owns: window rows [0, nrows - 1) of the nrows block rows
// that start at pa / pb (the lane's first pixel), window columns k < nwin of the lane's four.
// The wave marches down the block rows keeping the previous row's sums in registers; a window is
// two block rows x two blocks, the fifth block of a lane's four windows is its neighbour's first.
template <bool FULL>
__device__ __forceinline__ long long ssim_wave_tile(gcptr pa, int as, gcptr pb, int bs, int nb, int nwin, bool wide,
                                                    int nrows) {
  const int next = (((int)(threadIdx.x & 63) + 1) & 63) << 2;  // ds_bpermute address of the lane to the right
  uint32_t pp[4], pss[4], ps12[4];
  ssim_block_row<FULL>(pa, as, pb, bs, nb, wide, pp, pss, ps12);
  long long tot = 0;
  for (int r = 1; r < nrows; r++) {
    pa += 4LL * as;
    pb += 4LL * bs;
    uint32_t cp[4], css[4], cs12[4];
    ssim_block_row<FULL>(pa, as, pb, bs, nb, wide, cp, css, cs12);
    uint32_t vp[5], vss[5], vs12[5];  // the two block rows added: columns 0..3 this lane's, 4 the neighbour's
#pragma unroll
    for (int k = 0; k < 4; k++) {
      vp[k] = pp[k] + cp[k], vss[k] = pss[k] + css[k], vs12[k] = ps12[k] + cs12[k];
      pp[k] = cp[k], pss[k] = css[k], ps12[k] = cs12[k];
    }
    // (all 64 lanes are active here: the partial loads above have reconverged)
    vp[4] = (uint32_t)__builtin_amdgcn_ds_bpermute(next, (int)vp[0]);
    vss[4] = (uint32_t)__builtin_amdgcn_ds_bpermute(next, (int)vss[0]);
    vs12[4] = (uint32_t)__builtin_amdgcn_ds_bpermute(next, (int)vs12[0]);
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const uint32_t p = vp[k] + vp[k + 1];
      const int q = ssim_q(p & 0xffffu, p >> 16, vss[k] + vss[k + 1], vs12[k] + vs12[k + 1]);
      tot += k < nwin ? q : 0;
    }
  }
  return tot;
}

// grid (ceil(units / 4), pairs), 256 threads: a wave takes one unit of pair blockIdx.y.  The units of a
// frame are the (band, tile) cells of its planes, Y then U then V, tiles of one band adjacent: a tile is
// SSIM_TILE window columns (64 lanes x 16 pixels read, the last four blocks only for their first), a band
// SSIM_BAND window rows (one more block row read).  Neighbouring tiles and bands share one block column /
// row, so every window has exactly one owner.
__global__ __launch_bounds__(256) void k_ssim_i420(const SsimArgs A) {
  // (the inline pairs are read in place in the kernarg segment: a dynamic index into the by-value
  // argument would copy it to scratch)
  const SsePair *pp = ((const SsimArgs *)__builtin_amdgcn_kernarg_segment_ptr())->inl + blockIdx.y;
  int u = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // (uniform: SGPRs)
  const int cw = A.W >> 1, ch = A.H >> 1;
  const int nY = ssim_tiles(A.W >> 2) * ssim_bands(A.H >> 2), nC = ssim_tiles(cw >> 2) * ssim_bands(ch >> 2);
  int pl = 0;
  if (u >= nY) {
    u -= nY;
    pl = 1;
    if (u >= nC) u -= nC, pl = 2;
    if (u >= nC) return;
  }
  const int bw = (pl ? cw : A.W) >> 2, bh = (pl ? ch : A.H) >> 2;
  const int nt = ssim_tiles(bw), band = u / nt, tile = u - band * nt;
  const int as = pp->as[pl ? 1 : 0], bs = pp->bs[pl ? 1 : 0];
  const uint8_t *a_ = pp->a[pl], *b_ = pp->b[pl];
  const bool wide = (((uintptr_t)a_ | (uintptr_t)b_ | (uintptr_t)(unsigned)as | (uintptr_t)(unsigned)bs) & 15) == 0;
  const int lane = threadIdx.x & 63;
  const int r0 = band * SSIM_BAND, nrows = min(SSIM_BAND, bh - 1 - r0) + 1;  // block rows [r0, r0 + nrows) <= bh
  const int bx0 = tile * SSIM_TILE + 4 * lane;                                // the lane's first block
  const int nb = min(max(bw - bx0, 0), 4);                                    // its blocks inside the plane
  const int nwin = lane < SSIM_LANES ? min(max(bw - 1 - bx0, 0), 4) : 0;      // the windows it owns
  const gcptr pa = (gcptr)a_ + 4LL * r0 * as + 4 * bx0, pb = (gcptr)b_ + 4LL * r0 * bs + 4 * bx0;
  long long tot;
  if (tile * SSIM_TILE + 256 <= bw)  // (uniform) every lane's four blocks are inside the plane
    tot = ssim_wave_tile<true>(pa, as, pb, bs, 4, nwin, wide, nrows);
  else
    tot = ssim_wave_tile<false>(pa, as, pb, bs, nb, nwin, wide, nrows);
  tot = wave_sum64(tot);  // (all 64 lanes active: the tile's partial loads have reconverged)
  if (lane == 0 && tot) atomicAdd(A.sums + 3 * (size_t)blockIdx.y + pl, (unsigned long long)tot);
}

// Zero the sums and launch k_ssim_i420 for n pairs on `st`, SSIM_INL per launch through the kernel arguments.
static int ssim_enqueue(const SsePair *host, int n, int W, int H, unsigned long long *sums, hipStream_t st) {
  if (zero_sums(sums, (size_t)n * 3, st) != THOR_OK) return THOR_ERR_HIP;
  const int units = ssim_tiles(W >> 2) * ssim_bands(H >> 2) + 2 * ssim_tiles(W >> 3) * ssim_bands(H >> 3);
  SsimArgs A;
  memset(&A, 0, sizeof(A));
  A.W = W;
  A.H = H;
  return launch_batches(n, SSIM_INL, [&](int i0, int m) {
    memcpy(A.inl, host + i0, (size_t)m * sizeof(SsePair));
    A.sums = sums + 3 * (size_t)i0;
    k_ssim_i420<<<dim3((unsigned)((units + 3) / 4), (unsigned)m), 256, 0, st>>>(A);
  });
}

extern "C" {

int thor_ssim_windows(int width, int height) {
  if (width < 8 || height < 8) return 0;
  return ((width >> 2) - 1) * ((height >> 2) - 1);
}

int thor_ssim_i420(const thor_yuv_planes_t *a, const thor_yuv_planes_t *b, int n, int width, int height, int64_t *sums,
                   void *stream) {
  if (!a || !b || !sums || n <= 0 || n > 65535 || width < 16 || height < 16) return THOR_ERR_ARG;
  std::vector<SsePair> pairs((size_t)n);
  for (int i = 0; i < n; i++)
    if (!sse_fill_pair(pairs[i], a[i], b[i])) return THOR_ERR_ARG;
  return ssim_enqueue(pairs.data(), n, width, height, (unsigned long long *)sums, (hipStream_t)stream);
}

double thor_ssim(int64_t sum, int width, int height) {
  const int n = thor_ssim_windows(width, height);
  return n ? (double)sum / (1073741824.0 * n) : NAN;  // (a plane without a window has no SSIM)
}

double thor_ssim_db(double ssim) { return -10 * log10(1 - ssim); }

int thor_dec_frame_ssim(thor_dec_t *d, int frame_num, const thor_yuv_planes_t *orig, int64_t *sums_dev) {
  if (!d || !orig || !sums_dev || d->seq.width < 16 || d->seq.height < 16) return THOR_ERR_ARG;
  const int s = find_slot_host(d, frame_num);
  if (s < 0) return THOR_ERR_REF;
  SsePair P;
  if (!sse_fill_pair(P, *orig, slot_planes(d, s))) return THOR_ERR_ARG;
  HIPCHK(hipSetDevice(d->device));
  return ssim_enqueue(&P, 1, d->seq.width, d->seq.height, (unsigned long long *)sums_dev, d->stream);
}

}  // extern "C"
