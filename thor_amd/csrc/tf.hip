// Temporal denoise on the device: a motion-compensated pre-filter of I420 source
// frames (include/thor_amd.h: thor_tf_create, thor_tf_i420).  The contract is
// per reference and 8x8 luma block a half-pel vector (the
// lookahead's vector of the 16x16 block as the start, +-2 integer pixels, then
// +-1 half pel, bilinear), and per pixel of every plane a weighted mean of the
// target and the motion-compensated references, the weight falling with the
// pixel's and the block's squared error.  The reference has no such filter: the
// integer contract is the specification, and tests/tf_model.py restates it in
// numpy.
//
// Every value is an exact integer and the search winners are unsigned minima of
// distinct keys, so nothing depends on the order of reduction.  The per-pixel
// division is the plain integer `/`.
// The coarse stage is the lookahead's: la_enqueue (lookahead.hip) runs before the two kernels here.
#include "frame_ops.h"

static int la_enqueue(const LaPair *host, int n, int W, int H, thor_la_block_t *blocks, unsigned long long *sums,
                      hipStream_t st);  // lookahead.hip

#define TF_BLK 16    // a wave's luma block: four 8x8 sub-blocks that share the lookahead's start vector
#define TF_WAVES 4   // waves of a workgroup, side by side: a tile of 64 x 16 luma pixels
#define TF_TILE_W (TF_BLK * TF_WAVES)
#define TF_TILE_H TF_BLK
#define TF_IR 2      // the integer refinement is [-TF_IR, TF_IR]^2
#define TF_MARGIN (TF_IR + 1)  // the half-pel step below the integer winner reads one pixel more
// The reference's window of a wave in LDS: pixels -TF_MARGIN .. TF_BLK + TF_MARGIN - 1 around the block at the
// start vector (the half-pel neighbour of the last candidate is the last of them), coordinates clamped to the plane.
#define TF_WIN_ROWS (TF_BLK + 2 * TF_MARGIN)  // 22
#define TF_WIN_COLS (TF_BLK + 2 * TF_MARGIN)  // 22
#define TF_WIN_STRIDE 24                      // bytes: whole dwords
#define TF_WIN_WORDS (TF_WIN_ROWS * TF_WIN_STRIDE >> 2)
#define TF_CUR_WORDS (TF_BLK * TF_BLK >> 2)   // the target's block
#define TF_WAVE_WORDS (TF_WIN_WORDS + TF_CUR_WORDS)
#define TF_LUT_WORDS 64
#define TF_INL 4     // targets that travel in the kernel arguments (192 bytes each)
#define TF_CBX 64    // k_tf_chroma: 4x4 chroma blocks per workgroup row (a lane each)
#define TF_CBY 4     // and rows of them
static_assert(TF_WIN_STRIDE % 4 == 0 && TF_WIN_STRIDE >= TF_WIN_COLS, "rows are whole dwords");
static_assert(((TF_WIN_COLS - 9) / 4 + 3) * 4 <= TF_WIN_STRIDE,"nine bytes from the last candidate's column: three dwords inside the row");
static_assert(255 * 64 < (1 << 14) && 2 * TF_IR < (1 << 5) && (2 * TF_IR + 1) * (2 * TF_IR + 1) <= (1 << 5), "the key's three fields");
static_assert(THOR_TF_MAX_REFS == 4, "TfTarget");

__device__ static const uint16_t tf_lut_dev[TF_LUT_WORDS] = {
    256, 240, 226, 212, 199, 187, 176, 165, 155, 146, 137, 129, 121, 114, 107, 100, 94, 88, 83, 78, 73, 69,
    65,  61,  57,  54,  50,  47,  44,  42,  39,  37,  35,  33,  31,  29,  27,  25,  24, 22, 21, 20, 19, 17,
    16,  15,  14,  14,  13,  12,  11,  11,  10,  9,   9,   8,   8,   7,   7,   6,   6,  6,  5,  0};

struct TfTarget {
  const uint8_t *cur[3];
  uint8_t *dst[3];
  const uint8_t *ref[THOR_TF_MAX_REFS][3];  // ref[r][0] nullptr: absent
  int cs[2], ds[2], rs[THOR_TF_MAX_REFS][2];  // strides: luma, chroma
};
struct TfArgs {
  uint32_t *recs;    // [targets][nrefs][bh8][bw8] records (always there: the chroma kernel reads them)
  const uint2 *la;   // [targets][nrefs][lbh][lbw] lookahead records
  int w, h, bw8, bh8, lbw, lbh, nrefs;
  uint32_t mult_y, mult_c;
  TfTarget inl[TF_INL];
};
static_assert(sizeof(TfTarget) == 192 && sizeof(TfArgs) <= 1024, "the targets travel in the kernarg segment");

// (a + b + c + d + 2) >> 2 of four packed bytes.  With b = a, c = a, d = a it is a; with c = a, d = b it is
// (a + b + 1) >> 1: the contract's four prediction cases are this one form with the taps chosen by the fractions.
__device__ __forceinline__ uint32_t tf_avg4(uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
  const uint32_t M = 0x00ff00ffu;
  const uint32_t e = (a & M) + (b & M) + (c & M) + (d & M) + 0x00020002u;
  const uint32_t o = ((a >> 8) & M) + ((b >> 8) & M) + ((c >> 8) & M) + ((d >> 8) & M) + 0x00020002u;
  return ((e >> 2) & M) | (((o >> 2) & M) << 8);
}

// Bytes col .. col + 8 of row `row` of a window: lo the first four, hi the next four, the ninth in ex's low byte.
__device__ __forceinline__ void tf_row9(const uint32_t *win, int row, int col, uint32_t &lo, uint32_t &hi, uint32_t &ex) {
  const int a = row * TF_WIN_STRIDE + col;
  const uint32_t *p = win + (a >> 2);
  const uint32_t sh = (uint32_t)a & 3u;
  const uint32_t w0 = p[0], w1 = p[1], w2 = p[2];
  lo = __builtin_amdgcn_alignbyte(w1, w0, sh);
  hi = __builtin_amdgcn_alignbyte(w2, w1, sh);
  ex = w2 >> (8 * sh);
}
// Bytes col .. col + 4: lo the first four, the fifth in ex's low byte.
__device__ __forceinline__ void tf_row5(const uint32_t *win, int row, int col, uint32_t &lo, uint32_t &ex) {
  const int a = row * TF_WIN_STRIDE + col;
  const uint32_t *p = win + (a >> 2);
  const uint32_t sh = (uint32_t)a & 3u;
  const uint32_t w0 = p[0], w1 = p[1];
  lo = __builtin_amdgcn_alignbyte(w1, w0, sh);
  ex = w1 >> (8 * sh);
}

// Four output bytes at p: one dword where it is aligned, bytes elsewhere.
__device__ __forceinline__ void tf_store4(uint8_t *p, uint32_t v) {
  if (((uintptr_t)p & 3) == 0) {
    *(uint32_t *)p = v;
  } else {
#pragma unroll
    for (int k = 0; k < 4; k++) p[k] = (uint8_t)(v >> (8 * k));
  }
}

// The weight of one reference pixel: d its difference, e its block's mean squared error.
__device__ __forceinline__ uint32_t tf_weight(const uint32_t *lut, int d, uint32_t e, uint32_t mult) {
  const uint32_t m = ((uint32_t)(d * d) + e) >> 1;
  return lut[min(63u, (min(m, 2047u) * mult) >> 16)];
}

// grid (ceil(w / TF_TILE_W), ceil(h / TF_TILE_H), targets), 256 threads: wave `wv` of a workgroup owns the 16x16
// luma block TF_WAVES * blockIdx.x + wv of block row blockIdx.y of target blockIdx.z, 16 lanes per 8x8 sub-block.
// Per reference: the window at the lookahead's vector into the wave's LDS, the 25 integer candidates (two per
// lane), the 9 half-pel candidates (one per lane), then the blend of the lane's four pixels (row l16 >> 1, columns
// 4 (l16 & 1) .. + 3 of the sub-block).  Numerator and denominator stay in registers over the references.
__global__ __launch_bounds__(256) void k_tf_luma(const TfArgs A) {
  __shared__ uint32_t lds[TF_WAVES * TF_WAVE_WORDS + TF_LUT_WORDS];
  // (the inline targets are read in place in the kernarg segment: a dynamic index into the by-value
  // argument would copy it to scratch)
  const TfTarget *tg = ((const TfArgs *)__builtin_amdgcn_kernarg_segment_ptr())->inl + blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  uint32_t *const win = lds + wave * TF_WAVE_WORDS, *const curw = win + TF_WIN_WORDS;
  uint32_t *const lut = lds + TF_WAVES * TF_WAVE_WORDS;
  const int X = blockIdx.x * TF_WAVES + wave, Y = blockIdx.y;
  const int x0 = TF_BLK * X, y0 = TF_BLK * Y;
  const bool live = x0 < A.w;  // (uniform in the wave; y0 < h in every workgroup)
  const int sub = lane >> 4, l16 = lane & 15, sbx = sub & 1, sby = sub >> 1;
  const bool sub_live = live && x0 + 8 * sbx < A.w && y0 + 8 * sby < A.h;
  const int rr = l16 >> 1, hf = l16 & 1;  // the lane's pixels in the blend: row rr, columns 4 hf .. 4 hf + 3 of its sub-block
  const int cs = tg->cs[0], ds = tg->ds[0];

  if (tid < TF_LUT_WORDS) lut[tid] = tf_lut_dev[tid];
  if (live) {
    const int px = x0 + 4 * (lane & 3), py = y0 + (lane >> 2);
    curw[lane] = px < A.w && py < A.h ? g_ld4((gcptr)tg->cur[0] + (long long)py * cs + px) : 0u;
  }
  __syncthreads();
  uint32_t c0[8], c1[8];
#pragma unroll
  for (int r = 0; r < 8; r++) {
    c0[r] = curw[(8 * sby + r) * (TF_BLK / 4) + 2 * sbx];
    c1[r] = curw[(8 * sby + r) * (TF_BLK / 4) + 2 * sbx + 1];
  }
  const uint32_t tw = curw[(8 * sby + rr) * (TF_BLK / 4) + 2 * sbx + hf];
  uint32_t num[4], den[4];
#pragma unroll
  for (int k = 0; k < 4; k++) num[k] = 256u * ((tw >> (8 * k)) & 0xffu), den[k] = 256u;

  const size_t rec_target = (size_t)blockIdx.z * A.nrefs;
  for (int r = 0; r < A.nrefs; r++) {
    const gcptr ref = (gcptr)tg->ref[r][0];
    const int rs = tg->rs[r][0];
    uint32_t *const rec = A.recs + ((rec_target + r) * A.bh8 + (2 * Y + sby)) * A.bw8 + 2 * X + sbx;
    if (!ref) {  // (uniform in the workgroup) an absent reference: zero records, no weight
      if (sub_live && l16 == 0) *rec = 0u;
      continue;
    }
    int sx = 0, sy = 0;  // the start: twice the lookahead's vector, in source pixels (uniform in the wave)
    if (X < A.lbw && Y < A.lbh) {
      const uint32_t v = A.la[((rec_target + r) * A.lbh + Y) * A.lbw + X].y;
      sx = 2 * (int)(int8_t)(v >> 16), sy = 2 * (int)(int8_t)(v >> 24);
    }
    __syncthreads();  // the window's readers of the reference before are done
    if (live)
      for (int g = lane; g < TF_WIN_WORDS; g += 64) {
        const int ry = g / (TF_WIN_STRIDE / 4), gx = g - ry * (TF_WIN_STRIDE / 4);
        win[g] = ld4_clamped(ref, rs, x0 + sx - TF_MARGIN + 4 * gx, y0 + sy - TF_MARGIN + ry, A.w, A.h);
      }
    __syncthreads();
    if (!live) continue;  // (uniform in the wave; nothing below has a barrier)

    // integer refinement: candidate k = (dy + 2) * 5 + dx + 2, lane l16 takes k = l16 and k = l16 + 16 (the lanes
    // past 24 repeat 24)
    const int brow = 8 * sby + TF_MARGIN, bcol = 8 * sbx + TF_MARGIN;  // the sub-block at the start vector
    uint32_t best = 0xffffffffu;
#pragma unroll
    for (int pass = 0; pass < 2; pass++) {
      const int k = min(l16 + 16 * pass, (2 * TF_IR + 1) * (2 * TF_IR + 1) - 1);
      const int dy = k / (2 * TF_IR + 1) - TF_IR, dx = k - (dy + TF_IR) * (2 * TF_IR + 1) - TF_IR;
      uint32_t sad = 0;
#pragma unroll
      for (int j = 0; j < 8; j++) {
        uint32_t lo, hi, ex;
        tf_row9(win, brow + dy + j, bcol + dx, lo, hi, ex);
        sad = __builtin_amdgcn_sad_u8(lo, c0[j], sad);
        sad = __builtin_amdgcn_sad_u8(hi, c1[j], sad);
      }
      best = min(best, (sad << 10) | ((uint32_t)(abs(dx) + abs(dy)) << 5) | (uint32_t)k);
    }
    best = row_reduce(best, OpMin());  // (all 64 lanes active here and below: `live` is uniform in the wave)
    const int wk = (int)(best & 31u), oy = wk / (2 * TF_IR + 1) - TF_IR, ox = wk - (oy + TF_IR) * (2 * TF_IR + 1) - TF_IR;

    // half-pel refinement: candidate k = (hy + 1) * 3 + hx + 1 (the lanes past 8 repeat 8).  The half-pel vector
    // 2 o + h has the integer part o + (h >> 1) and the fraction h & 1.
    {
      const int k = min(l16, 8);
      const int hy = k / 3 - 1, hx = k - (hy + 1) * 3 - 1;
      const bool fx = hx & 1, fy = hy & 1;
      const int row = brow + oy + (hy >> 1), col = bcol + ox + (hx >> 1);
      uint32_t alo, ahi, aex, sad = 0;
      tf_row9(win, row, col, alo, ahi, aex);
#pragma unroll
      for (int j = 0; j < 8; j++) {
        uint32_t nlo, nhi, nex;
        tf_row9(win, row + j + 1, col, nlo, nhi, nex);
        const uint32_t blo = fx ? __builtin_amdgcn_alignbyte(ahi, alo, 1) : alo;
        const uint32_t bhi = fx ? __builtin_amdgcn_alignbyte(aex, ahi, 1) : ahi;
        const uint32_t clo = fy ? nlo : alo, chi = fy ? nhi : ahi;
        const uint32_t dlo = fy ? (fx ? __builtin_amdgcn_alignbyte(nhi, nlo, 1) : nlo) : blo;
        const uint32_t dhi = fy ? (fx ? __builtin_amdgcn_alignbyte(nex, nhi, 1) : nhi) : bhi;
        sad = __builtin_amdgcn_sad_u8(tf_avg4(alo, blo, clo, dlo), c0[j], sad);
        sad = __builtin_amdgcn_sad_u8(tf_avg4(ahi, bhi, chi, dhi), c1[j], sad);
        alo = nlo, ahi = nhi, aex = nex;
      }
      best = row_reduce((sad << 6) | ((uint32_t)(abs(hx) + abs(hy)) << 4) | (uint32_t)k, OpMin());
    }
    const int hk = (int)(best & 15u), hy = hk / 3 - 1, hx = hk - (hy + 1) * 3 - 1;
    const int mvx = 2 * (sx + ox) + hx, mvy = 2 * (sy + oy) + hy;

    // the blend: the lane's four pixels of the prediction at the winner
    const bool fx = hx & 1, fy = hy & 1;
    const int row = brow + oy + (hy >> 1) + rr, col = bcol + ox + (hx >> 1) + 4 * hf;
    uint32_t a, ae, n, ne;
    tf_row5(win, row, col, a, ae);
    tf_row5(win, row + 1, col, n, ne);
    const uint32_t b = fx ? __builtin_amdgcn_alignbyte(ae, a, 1) : a;
    const uint32_t c = fy ? n : a;
    const uint32_t d = fy ? (fx ? __builtin_amdgcn_alignbyte(ne, n, 1) : n) : b;
    const uint32_t pw = tf_avg4(a, b, c, d);
    int df[4];
    uint32_t ssd = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      df[k] = (int)((tw >> (8 * k)) & 0xffu) - (int)((pw >> (8 * k)) & 0xffu);
      ssd += (uint32_t)(df[k] * df[k]);
    }
    const uint32_t e = row_reduce(ssd, OpSum()) >> 6;  // (<= 65 025)
    if (sub_live && l16 == 0) *rec = ((uint32_t)mvx & 0xffu) | (((uint32_t)mvy & 0xffu) << 8) | (e << 16);
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const uint32_t wgt = tf_weight(lut, df[k], e, A.mult_y);
      num[k] += wgt * ((pw >> (8 * k)) & 0xffu);
      den[k] += wgt;
    }
  }
  if (sub_live) {
    uint32_t out = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) out |= ((num[k] + (den[k] >> 1)) / den[k]) << (8 * k);
    tf_store4(tg->dst[0] + (long long)(y0 + 8 * sby + rr) * ds + x0 + 8 * sbx + 4 * hf, out);
  }
}

// grid (ceil(bw8 / TF_CBX), ceil(bh8 / TF_CBY), 2 * targets), 256 threads: a lane owns the 4x4 block (bx, by) of
// the U (blockIdx.z even) or V plane of target blockIdx.z >> 1, under the 8x8 luma block whose records it reads.
// No LDS: the 5x5 reference pixels of a block come straight from the plane (a dword and a byte per row), and a
// lane's sixteen numerators and denominators stay in registers over the references.
__global__ __launch_bounds__(256) void k_tf_chroma(const TfArgs A) {
  __shared__ uint32_t lut[TF_LUT_WORDS];
  const int z = blockIdx.z >> 1, pl = 1 + (blockIdx.z & 1);
  const TfTarget *tg = ((const TfArgs *)__builtin_amdgcn_kernarg_segment_ptr())->inl + z;
  const int tid = threadIdx.x;
  if (tid < TF_LUT_WORDS) lut[tid] = tf_lut_dev[tid];
  __syncthreads();
  const int bx = blockIdx.x * TF_CBX + (tid & (TF_CBX - 1)), by = blockIdx.y * TF_CBY + tid / TF_CBX;
  if (bx >= A.bw8 || by >= A.bh8) return;
  const int cw = A.w >> 1, ch = A.h >> 1;
  const int cs = tg->cs[1], ds = tg->ds[1];
  const gcptr cur = (gcptr)tg->cur[pl] + (long long)(4 * by) * cs + 4 * bx;
  uint32_t tw[4], num[16], den[16];
#pragma unroll
  for (int j = 0; j < 4; j++) {
    tw[j] = g_ld4(cur + (long long)j * cs);
#pragma unroll
    for (int k = 0; k < 4; k++) num[4 * j + k] = 256u * ((tw[j] >> (8 * k)) & 0xffu), den[4 * j + k] = 256u;
  }
  for (int r = 0; r < A.nrefs; r++) {
    const gcptr ref = (gcptr)tg->ref[r][pl];
    if (!tg->ref[r][0]) continue;
    const int rs = tg->rs[r][1];
    const uint32_t rec = A.recs[(((size_t)z * A.nrefs + r) * A.bh8 + by) * A.bw8 + bx];
    const int mvx = (int)(int8_t)(rec & 0xffu) >> 1, mvy = (int)(int8_t)((rec >> 8) & 0xffu) >> 1;
    const bool fx = mvx & 1, fy = mvy & 1;
    const int ix = 4 * bx + (mvx >> 1), iy = 4 * by + (mvy >> 1);
    const bool inside = ix >= 0 && ix + 4 < cw;
    uint32_t pw[4], a = 0, b = 0;
#pragma unroll
    for (int j = 0; j < 5; j++) {
      const gcptr row = ref + (long long)min(max(iy + j, 0), ch - 1) * rs;
      uint32_t lo, ex;
      if (inside) {
        lo = g_ld4(row + ix), ex = row[ix + 4];
      } else {
        lo = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) lo |= (uint32_t)row[min(max(ix + k, 0), cw - 1)] << (8 * k);
        ex = row[min(max(ix + 4, 0), cw - 1)];
      }
      const uint32_t nb = fx ? __builtin_amdgcn_alignbyte(ex, lo, 1) : lo;
      if (j > 0) pw[j - 1] = tf_avg4(a, b, fy ? lo : a, fy ? nb : b);
      a = lo, b = nb;
    }
    int df[16];
    uint32_t ssd = 0;
#pragma unroll
    for (int j = 0; j < 4; j++)
#pragma unroll
      for (int k = 0; k < 4; k++) {
        df[4 * j + k] = (int)((tw[j] >> (8 * k)) & 0xffu) - (int)((pw[j] >> (8 * k)) & 0xffu);
        ssd += (uint32_t)(df[4 * j + k] * df[4 * j + k]);
      }
    const uint32_t e = ssd >> 4;
#pragma unroll
    for (int j = 0; j < 4; j++)
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const uint32_t wgt = tf_weight(lut, df[4 * j + k], e, A.mult_c);
        num[4 * j + k] += wgt * ((pw[j] >> (8 * k)) & 0xffu);
        den[4 * j + k] += wgt;
      }
  }
  uint8_t *const dst = tg->dst[pl] + (long long)(4 * by) * ds + 4 * bx;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    uint32_t out = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) out |= ((num[4 * j + k] + (den[4 * j + k] >> 1)) / den[4 * j + k]) << (8 * k);
    tf_store4(dst + (long long)j * ds, out);
  }
}

struct thor_tf {
  int w, h, max_targets, device;  // (tests/test_tf_host.py mirrors this head to reach the argument checks without a device)
  thor_la_block_t *la;        // [max_targets * 4 * lbw * lbh] lookahead records
  unsigned long long *sums;   // [max_targets * 4 * 4] its sums
  uint32_t *recs;             // [max_targets * 4 * bw8 * bh8] records of a call without mv_dev
};

static inline uint32_t tf_mult_of(int s) { return (uint32_t)(((16 << 16) + ((s * s) >> 1)) / (s * s)); }

extern "C" {

int thor_tf_check(int width, int height, int nrefs) {
  if (width < 16 || height < 16 || width > 16384 || height > 16384 || (width & 7) || (height & 7)) return THOR_ERR_ARG;
  if (nrefs < 1 || nrefs > THOR_TF_MAX_REFS) return THOR_ERR_ARG;
  return THOR_OK;
}

int thor_tf_mult(int strength) {
  if (strength < 1 || strength > 64) return THOR_ERR_ARG;
  return (int)tf_mult_of(strength);
}

int thor_tf_blocks(int width, int height, int *bw8, int *bh8) {
  if (thor_tf_check(width, height, 1) != THOR_OK) return THOR_ERR_ARG;
  if (bw8) *bw8 = width >> 3;
  if (bh8) *bh8 = height >> 3;
  return (width >> 3) * (height >> 3);
}

void thor_tf_destroy(thor_tf_t *t) {
  if (!t) return;
  (void)hipSetDevice(t->device);
  if (t->la) (void)hipFree(t->la);
  if (t->sums) (void)hipFree(t->sums);
  if (t->recs) (void)hipFree(t->recs);
  delete t;
}

thor_tf_t *thor_tf_create(int width, int height, int max_targets, int device) {
  create_begin();
  if (thor_tf_check(width, height, 1) != THOR_OK || max_targets < 1 || max_targets > THOR_TF_MAX_TARGETS) {
    create_fail(THOR_ERR_ARG, 0, "thor_tf_create: unsupported size %dx%d or %d targets", width, height, max_targets);
    return nullptr;
  }
  if (hipSetDevice(device) != hipSuccess) {
    (void)hipGetLastError();
    create_fail(THOR_ERR_ARG, 0, "thor_tf_create: no HIP device %d", device);
    return nullptr;
  }
  thor_tf *t = new thor_tf();
  t->w = width, t->h = height, t->max_targets = max_targets, t->device = device;
  int lw, lh, lbw, lbh;
  la_dims(width, height, lw, lh, lbw, lbh);
  const size_t pairs = (size_t)max_targets * THOR_TF_MAX_REFS;
  bool ok = dev_alloc(&t->la, pairs * lbw * lbh * sizeof(thor_la_block_t), "thor_tf_create: lookahead records");
  ok = ok && dev_alloc(&t->sums, pairs * 4 * sizeof(unsigned long long), "thor_tf_create: lookahead sums");
  ok = ok && dev_alloc(&t->recs, pairs * (width >> 3) * (height >> 3) * sizeof(uint32_t), "thor_tf_create: records");
  if (!ok) {
    thor_tf_destroy(t);
    return nullptr;
  }
  return t;
}

int thor_tf_i420(thor_tf_t *t, const thor_yuv_planes_t *cur, const thor_yuv_planes_t *refs, const thor_yuv_planes_t *dst,
                 int n, int nrefs, int strength_y, int strength_c, thor_tf_record_t *mv_dev, void *stream) {
  if (!t || !cur || !refs || !dst || n < 1 || n > t->max_targets || nrefs < 1 || nrefs > THOR_TF_MAX_REFS)
    return THOR_ERR_ARG;
  if (strength_y < 1 || strength_y > 64 || strength_c < 1 || strength_c > 64 || ((uintptr_t)mv_dev & 3)) return THOR_ERR_ARG;
  const int W = t->w, H = t->h;
  std::vector<TfTarget> tg((size_t)n);
  std::vector<LaPair> pairs((size_t)n * nrefs);
  for (int i = 0; i < n; i++) {
    const thor_yuv_planes_t &c = cur[i], &d = dst[i];
    if (!planes_ok(c, W) || !planes_ok(d, W)) return THOR_ERR_ARG;
    if (d.y == c.y || d.u == c.u || d.v == c.v) return THOR_ERR_ARG;  // not in place
    TfTarget &g = tg[i];
    memset(&g, 0, sizeof(g));
    g.cur[0] = c.y, g.cur[1] = c.u, g.cur[2] = c.v;
    g.dst[0] = d.y, g.dst[1] = d.u, g.dst[2] = d.v;
    g.cs[0] = c.stride_y, g.cs[1] = c.stride_c, g.ds[0] = d.stride_y, g.ds[1] = d.stride_c;
    for (int r = 0; r < nrefs; r++) {
      const thor_yuv_planes_t &f = refs[(size_t)i * nrefs + r];
      LaPair &p = pairs[(size_t)i * nrefs + r];
      la_fill_pair(p, c, &f);
      if (!f.y) continue;  // absent
      if (!planes_ok(f, W)) return THOR_ERR_ARG;
      if (d.y == f.y || d.u == f.u || d.v == f.v) return THOR_ERR_ARG;
      g.ref[r][0] = f.y, g.ref[r][1] = f.u, g.ref[r][2] = f.v;
      g.rs[r][0] = f.stride_y, g.rs[r][1] = f.stride_c;
    }
  }
  HIPCHK(hipSetDevice(t->device));
  const hipStream_t st = (hipStream_t)stream;
  // the coarse stage: the lookahead of every (target, reference) pair, its records in the context
  const int rc = la_enqueue(pairs.data(), n * nrefs, W, H, t->la, t->sums, st);
  if (rc != THOR_OK) return rc;
  TfArgs A;
  memset(&A, 0, sizeof(A));
  int lw, lh;
  la_dims(W, H, lw, lh, A.lbw, A.lbh);
  A.w = W, A.h = H, A.bw8 = W >> 3, A.bh8 = H >> 3, A.nrefs = nrefs;
  A.mult_y = tf_mult_of(strength_y), A.mult_c = tf_mult_of(strength_c);
  uint32_t *const recs = mv_dev ? (uint32_t *)mv_dev : t->recs;
  const dim3 gl((unsigned)((W + TF_TILE_W - 1) / TF_TILE_W), (unsigned)((H + TF_TILE_H - 1) / TF_TILE_H), 1);
  const dim3 gc((unsigned)((A.bw8 + TF_CBX - 1) / TF_CBX), (unsigned)((A.bh8 + TF_CBY - 1) / TF_CBY), 1);
  return launch_batches(n, TF_INL, [&](int i0, int m) {
    memcpy(A.inl, tg.data() + i0, (size_t)m * sizeof(TfTarget));
    A.recs = recs + (size_t)i0 * nrefs * A.bw8 * A.bh8;
    A.la = (const uint2 *)t->la + (size_t)i0 * nrefs * A.lbw * A.lbh;
    k_tf_luma<<<dim3(gl.x, gl.y, (unsigned)m), 256, 0, st>>>(A);
    k_tf_chroma<<<dim3(gc.x, gc.y, (unsigned)(2 * m)), 256, 0, st>>>(A);
  });
}

}  // extern "C"
