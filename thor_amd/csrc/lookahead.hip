// Frame analysis on the device: lookahead costs of I420 frame pairs
// (include/thor_amd.h: thor_lookahead_i420, thor_lookahead_blocks,
// thor_lookahead_scenecut).  The contract is DESIGN.md sec. 7f: a half-resolution
// (2x2 box) copy of the luma of both frames, 8x8 lowres blocks, per block the
// least SATD over the intra predictors built from the source's own lowres
// neighbours and the SATD at the winner of an integer full search of +-8 lowres
// pixels on the reference's lowres plane; one 8-byte record per block and four
// 64-bit sums per frame.  The reference has no lookahead: the integer contract
// is the specification, and tests/lookahead_model.py restates it in numpy.
//
// Every value is an exact integer and the search winner is an unsigned minimum
// of distinct keys, so neither depends on the order of reduction.
#include "frame_ops.h"

#define LA_TBW 8    // blocks per tile row: 64 lowres pixels
#define LA_TBH 4    // block rows per tile: 32 lowres pixels
#define LA_RANGE 8  // the search is [-LA_RANGE, LA_RANGE]^2 lowres pixels
#define LA_SIDE (2 * LA_RANGE + 1)
#define LA_NCAND (LA_SIDE * LA_SIDE)  // 289
#define LA_INL 8    // frame pairs that travel in the kernel arguments (24 bytes each)
// The tile's lowres pixels in LDS.  cur: one row above and four columns (one dword; only the last is a
// neighbour) to the left of the tile; ref: LA_RANGE pixels all round, coordinates clamped to the plane.
#define LA_CUR_COLS (8 * LA_TBW + 4)
#define LA_CUR_ROWS (8 * LA_TBH + 1)
#define LA_CUR_STRIDE (LA_CUR_COLS + 4)  // 72 bytes
#define LA_REF_COLS (8 * LA_TBW + 2 * LA_RANGE)
#define LA_REF_ROWS (8 * LA_TBH + 2 * LA_RANGE)
#define LA_REF_STRIDE LA_REF_COLS        // 80 bytes
#define LA_CUR_BYTES (LA_CUR_ROWS * LA_CUR_STRIDE)
#define LA_REF_BYTES (LA_REF_ROWS * LA_REF_STRIDE + 16)  // (the realigning read of a row's last 8 bytes takes one dword more)
static_assert(LA_CUR_STRIDE % 4 == 0 && LA_REF_STRIDE % 4 == 0 && LA_CUR_BYTES % 4 == 0, "rows are whole dwords");
static_assert(255 * 64 < (1 << 14) && 2 * LA_RANGE < (1 << 5) && LA_NCAND <= (1 << 9), "the key's three fields");

struct LaArgs {
  uint2 *blocks;             // [pairs * bw * bh] records, or nullptr
  unsigned long long *sums;  // [4 * pairs], zero before the launch
  int lw, lh, bw, bh;
  LaPair inl[LA_INL];
};
static_assert(sizeof(LaArgs) <= 1024, "the pairs travel in the kernarg segment");

// Four lowres pixels (x .. x + 3, row y; both clamped to the plane) of the source plane p, packed in a dword.
// A group inside the plane takes four dword loads (two source rows x 8 bytes, any alignment); a group across
// the plane's edge goes pixel by pixel.  Nothing is read outside source rows [0, 2 lh) and columns [0, 2 lw).
__device__ __forceinline__ uint32_t la_lowres4(gcptr p, int stride, int x, int y, int lw, int lh) {
  const int yc = min(max(y, 0), lh - 1);
  const gcptr r0 = p + (long long)(2 * yc) * stride, r1 = r0 + stride;
  if (x >= 0 && x + 3 < lw) {
    uint32_t t[2];
#pragma unroll
    for (int k = 0; k < 2; k++) {
      const uint32_t a = g_ld4(r0 + 2 * x + 4 * k), b = g_ld4(r1 + 2 * x + 4 * k);
      // two pixels at once in 16-bit fields: each sum <= 4 * 255 + 2
      const uint32_t s =
          (a & 0x00ff00ffu) + ((a >> 8) & 0x00ff00ffu) + (b & 0x00ff00ffu) + ((b >> 8) & 0x00ff00ffu) + 0x00020002u;
      const uint32_t q = (s >> 2) & 0x00ff00ffu;
      t[k] = (q & 0xffu) | ((q >> 8) & 0xff00u);
    }
    return t[0] | (t[1] << 16);
  }
  uint32_t out = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int xc = 2 * min(max(x + k, 0), lw - 1);
    const uint32_t v = ((uint32_t)r0[xc] + r0[xc + 1] + r1[xc] + r1[xc + 1] + 2u) >> 2;
    out |= v << (8 * k);
  }
  return out;
}

typedef short la_s2 __attribute__((ext_vector_type(2)));
// One butterfly of two packed 16-bit values across lane bit BIT: the lane with the bit clear gets the sum, the
// other the difference (sg: the lane's packed +1 or -1 for this bit).
template <int BIT>
__device__ __forceinline__ la_s2 la_butterfly(la_s2 v, la_s2 sg) {
  const la_s2 p = __builtin_bit_cast(la_s2, row_xor<BIT>(__builtin_bit_cast(uint32_t, v)));
  return p + v * sg;
}

// grid (ceil(bw / LA_TBW), ceil(bh / LA_TBH), pairs), 256 threads: a workgroup owns a tile of LA_TBW x LA_TBH
// blocks of pair blockIdx.z.  It builds the lowres of the tile of both frames in LDS straight from the source,
// then every wave takes blocks wave, wave + 4, ... of the tile's 32: the search with four candidates per lane
// (16 dx x 16 dy) and one more for the last row and column, then the four residual blocks' Hadamard transforms
// side by side: 16 lanes per residual, four pixels per lane.
__global__ __launch_bounds__(256) void k_lookahead(const LaArgs A) {
  __shared__ uint32_t lds[(LA_CUR_BYTES + LA_REF_BYTES) / 4 + 4];
  uint32_t *const curw = lds, *const refw = lds + LA_CUR_BYTES / 4, *const wsum = refw + LA_REF_BYTES / 4;
  const uint8_t *const curb = (const uint8_t *)curw;
  // (the inline pairs are read in place in the kernarg segment: a dynamic index into the by-value
  // argument would copy it to scratch)
  const LaPair *pp = ((const LaArgs *)__builtin_amdgcn_kernarg_segment_ptr())->inl + blockIdx.z;
  const gcptr cur = (gcptr)pp->cur, ref = (gcptr)pp->ref;
  const int cs = pp->cs, rs = pp->rs;
  const bool inter_pair = pp->ref != nullptr;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int x0 = blockIdx.x * (8 * LA_TBW), y0 = blockIdx.y * (8 * LA_TBH);  // the tile's first lowres pixel

  if (tid < 4) wsum[tid] = 0;
  for (int g = tid; g < LA_CUR_ROWS * (LA_CUR_COLS / 4); g += 256) {
    const int ry = g / (LA_CUR_COLS / 4), gx = g - ry * (LA_CUR_COLS / 4);
    curw[ry * (LA_CUR_STRIDE / 4) + gx] = la_lowres4(cur, cs, x0 - 4 + 4 * gx, y0 - 1 + ry, A.lw, A.lh);
  }
  if (inter_pair)
    for (int g = tid; g < LA_REF_ROWS * (LA_REF_COLS / 4); g += 256) {
      const int ry = g / (LA_REF_COLS / 4), gx = g - ry * (LA_REF_COLS / 4);
      refw[ry * (LA_REF_STRIDE / 4) + gx] = la_lowres4(ref, rs, x0 - LA_RANGE + 4 * gx, y0 - LA_RANGE + ry, A.lw, A.lh);
    }
  __syncthreads();

  uint32_t t_intra = 0, t_inter = 0, t_min = 0, t_cnt = 0;  // (uniform)
  // the lane's place in the cost stage: residual rj, row rr of the block, pixels 4 hf .. 4 hf + 3; and its
  // packed sign for the butterfly across each of its four low lane bits
  const int hf = lane & 1, rr = (lane >> 1) & 7, rj = lane >> 4;
  const la_s2 sg0 = (lane & 1) ? la_s2{-1, -1} : la_s2{1, 1}, sg1 = (lane & 2) ? la_s2{-1, -1} : la_s2{1, 1},
              sg2 = (lane & 4) ? la_s2{-1, -1} : la_s2{1, 1}, sg3 = (lane & 8) ? la_s2{-1, -1} : la_s2{1, 1};
  for (int b = wave; b < LA_TBW * LA_TBH; b += 4) {
    const int by = b / LA_TBW, bx = b - by * LA_TBW;
    const int gbx = blockIdx.x * LA_TBW + bx, gby = blockIdx.y * LA_TBH + by;
    if (gbx >= A.bw || gby >= A.bh) continue;  // (uniform)
    // the block in the cur image: row 8 by + 1 (row 0 is the neighbour row), byte column 8 bx + 4
    const int cbase = (8 * by + 1) * LA_CUR_STRIDE + 8 * bx + 4;
    uint32_t best = 0xffffffffu;
    if (inter_pair) {
      uint32_t c0[8], c1[8];
#pragma unroll
      for (int r = 0; r < 8; r++) {
        c0[r] = curw[(cbase + r * LA_CUR_STRIDE) >> 2];
        c1[r] = curw[((cbase + r * LA_CUR_STRIDE) >> 2) + 1];
      }
      // 256 candidates in one pass: lane 16 g + dx takes (dy, dx) for dy = 4 g .. 4 g + 3, so that the eleven
      // rows of the reference those four share are read and realigned once
      {
        const int dx = lane & 15, dy0 = (lane >> 4) * 4;
        const int rbase = (8 * by + dy0) * LA_REF_STRIDE + 8 * bx + dx;
        const uint32_t sh = (uint32_t)rbase & 3u;
        const uint32_t *rw = refw + (rbase >> 2);
        uint32_t sad[4] = {0, 0, 0, 0};
#pragma unroll
        for (int t = 0; t < 11; t++) {
          const uint32_t w0 = rw[t * (LA_REF_STRIDE / 4)], w1 = rw[t * (LA_REF_STRIDE / 4) + 1],
                         w2 = rw[t * (LA_REF_STRIDE / 4) + 2];
          const uint32_t lo = __builtin_amdgcn_alignbyte(w1, w0, sh), hi = __builtin_amdgcn_alignbyte(w2, w1, sh);
#pragma unroll
          for (int j = 0; j < 4; j++)
            if (t - j >= 0 && t - j < 8) {
              sad[j] = __builtin_amdgcn_sad_u8(lo, c0[t - j], sad[j]);
              sad[j] = __builtin_amdgcn_sad_u8(hi, c1[t - j], sad[j]);
            }
        }
        const uint32_t lx = (uint32_t)abs(dx - LA_RANGE);
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const int dy = dy0 + j;
          best = min(best, (sad[j] << 14) | ((lx + (uint32_t)abs(dy - LA_RANGE)) << 9) | (uint32_t)(dy * LA_SIDE + dx));
        }
      }
      // the other 33: the last row (dy = 16: lanes 0 .. 16) and the last column (dx = 16: lanes 17 .. 32), a
      // candidate per lane; the spare lanes repeat lane 32's
      {
        const int q = min(lane, 2 * LA_SIDE - 2);
        const int dy = q < LA_SIDE ? 2 * LA_RANGE : q - LA_SIDE, dx = q < LA_SIDE ? q : 2 * LA_RANGE;
        const int rbase = (8 * by + dy) * LA_REF_STRIDE + 8 * bx + dx;
        const uint32_t sh = (uint32_t)rbase & 3u;
        const uint32_t *rw = refw + (rbase >> 2);
        uint32_t sad = 0;
#pragma unroll
        for (int r = 0; r < 8; r++) {
          const uint32_t w0 = rw[r * (LA_REF_STRIDE / 4)], w1 = rw[r * (LA_REF_STRIDE / 4) + 1],
                         w2 = rw[r * (LA_REF_STRIDE / 4) + 2];
          sad = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(w1, w0, sh), c0[r], sad);
          sad = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(w2, w1, sh), c1[r], sad);
        }
        const uint32_t len = (uint32_t)(abs(dx - LA_RANGE) + abs(dy - LA_RANGE));
        best = min(best, (sad << 14) | (len << 9) | (uint32_t)(dy * LA_SIDE + dx));
      }
      best = wave_reduce(best, OpMin());  // (all 64 lanes active: the branch is uniform)
    }
    const int wk = (int)(best & 511u), wdy = inter_pair ? wk / LA_SIDE : LA_RANGE;
    const int wdx = inter_pair ? wk - wdy * LA_SIDE : LA_RANGE;

    // DC: the sum of the row above (lanes 0..7) and of the column to the left (lanes 8..15), where they exist
    const bool has_top = gby > 0, has_left = gbx > 0;  // (uniform)
    const int ea = lane < 8 ? cbase - LA_CUR_STRIDE + lane : cbase + ((lane - 8) & 7) * LA_CUR_STRIDE - 1;
    const uint32_t ev = (lane < 8 ? has_top : lane < 16 && has_left) ? (uint32_t)curb[ea] : 0u;
    const uint32_t edge = (uint32_t)__builtin_amdgcn_readlane((int)row_reduce(ev, OpSum()), 0);
    const uint32_t dc = has_top && has_left ? (edge + 8) >> 4 : has_top || has_left ? (edge + 4) >> 3 : 128u;
    // The four residuals, one per 16-lane row (rj: 0 the search winner, 1 DC, 2 V, 3 H); a lane takes four
    // pixels of a row of the block (row rr, columns 4 hf ..) and the same four of its row's predictor: two dwords
    // realigned from byte address pa of the LDS image -- the winner's pixels, the row above (aligned), or the
    // dword that ends in the left neighbour (its byte 3, then replicated).
    const int own = cbase + rr * LA_CUR_STRIDE + 4 * hf;
    const uint32_t cw = curw[own >> 2];
    int pa = own;
    if (rj == 0 && inter_pair) pa = LA_CUR_BYTES + (8 * by + wdy + rr) * LA_REF_STRIDE + 8 * bx + wdx + 4 * hf;
    if (rj == 2) pa = cbase - LA_CUR_STRIDE + 4 * hf;
    if (rj == 3) pa = cbase + rr * LA_CUR_STRIDE - 1;
    uint32_t pred = __builtin_amdgcn_alignbyte(lds[(pa >> 2) + 1], lds[pa >> 2], (uint32_t)pa & 3u);
    if (rj == 3) pred = (pred & 0xffu) * 0x01010101u;
    if (rj == 1) pred = dc * 0x01010101u;
    // differences of pixels 0, 2 and of pixels 1, 3 as packed 16-bit pairs, then the transform: two butterflies
    // inside the lane (pixel bits 0 and 1), four across the lanes of the row (hf, then the three row bits).
    // Every intermediate is at most 64 * 255 in magnitude.
    const la_s2 e = __builtin_bit_cast(la_s2, cw & 0x00ff00ffu) - __builtin_bit_cast(la_s2, pred & 0x00ff00ffu);
    const la_s2 o = __builtin_bit_cast(la_s2, (cw >> 8) & 0x00ff00ffu) - __builtin_bit_cast(la_s2, (pred >> 8) & 0x00ff00ffu);
    const la_s2 s1 = e + o, d1 = e - o;
    la_s2 ta = la_s2{(short)(s1.x + s1.y), (short)(s1.x - s1.y)}, tb = la_s2{(short)(d1.x + d1.y), (short)(d1.x - d1.y)};
    ta = la_butterfly<0>(ta, sg0), tb = la_butterfly<0>(tb, sg0);
    ta = la_butterfly<1>(ta, sg1), tb = la_butterfly<1>(tb, sg1);
    ta = la_butterfly<2>(ta, sg2), tb = la_butterfly<2>(tb, sg2);
    ta = la_butterfly<3>(ta, sg3), tb = la_butterfly<3>(tb, sg3);
    // (a lane's four magnitudes sum to at most 4 * 16 320, a row's to at most 130 560)
    const uint32_t mag =
        (uint32_t)abs((int)ta.x) + (uint32_t)abs((int)ta.y) + (uint32_t)abs((int)tb.x) + (uint32_t)abs((int)tb.y);
    const uint32_t rowsum = row_reduce(mag, OpSum());
    const uint32_t s_dc = ((uint32_t)__builtin_amdgcn_readlane((int)rowsum, 16) + 2) >> 2;
    const uint32_t s_v = has_top ? ((uint32_t)__builtin_amdgcn_readlane((int)rowsum, 32) + 2) >> 2 : 0xffffffffu;
    const uint32_t s_h = has_left ? ((uint32_t)__builtin_amdgcn_readlane((int)rowsum, 48) + 2) >> 2 : 0xffffffffu;
    const uint32_t intra = min(s_dc, min(s_v, s_h));
    const uint32_t inter = inter_pair ? ((uint32_t)__builtin_amdgcn_readlane((int)rowsum, 0) + 2) >> 2 : intra;
    const uint32_t sad = inter_pair ? best >> 14 : 0xffffu;
    t_intra += intra;
    t_inter += inter;
    t_min += min(intra, inter);
    t_cnt += intra < inter ? 1u : 0u;
    if (A.blocks && lane == 0) {
      const uint32_t mvx = (uint32_t)(wdx - LA_RANGE) & 0xffu, mvy = (uint32_t)(wdy - LA_RANGE) & 0xffu;
      A.blocks[((size_t)blockIdx.z * A.bh + gby) * A.bw + gbx] =
          make_uint2(intra | (inter << 16), sad | (mvx << 16) | (mvy << 24));
    }
  }
  if (lane == 0) {
    atomicAdd(&wsum[0], t_intra);  // (<= 32 blocks x 32 640 per workgroup)
    atomicAdd(&wsum[1], t_inter);
    atomicAdd(&wsum[2], t_min);
    atomicAdd(&wsum[3], t_cnt);
  }
  __syncthreads();
  if (tid < 4 && wsum[tid]) atomicAdd(A.sums + 4 * (size_t)blockIdx.z + tid, (unsigned long long)wsum[tid]);
}

// Zero the sums and launch k_lookahead for n pairs on `st`, LA_INL per launch through the kernel arguments.
static int la_enqueue(const LaPair *host, int n, int W, int H, thor_la_block_t *blocks, unsigned long long *sums,
                      hipStream_t st) {
  if (zero_sums(sums, (size_t)n * 4, st) != THOR_OK) return THOR_ERR_HIP;
  LaArgs A;
  memset(&A, 0, sizeof(A));
  la_dims(W, H, A.lw, A.lh, A.bw, A.bh);
  const dim3 grid((unsigned)((A.bw + LA_TBW - 1) / LA_TBW), (unsigned)((A.bh + LA_TBH - 1) / LA_TBH), 1);
  return launch_batches(n, LA_INL, [&](int i0, int m) {
    memcpy(A.inl, host + i0, (size_t)m * sizeof(LaPair));
    A.sums = sums + 4 * (size_t)i0;
    A.blocks = blocks ? (uint2 *)blocks + (size_t)i0 * A.bw * A.bh : nullptr;
    k_lookahead<<<dim3(grid.x, grid.y, (unsigned)m), 256, 0, st>>>(A);
  });
}

extern "C" {

int thor_lookahead_blocks(int width, int height, int *bw, int *bh) {
  if (width < 16 || height < 16 || width > 16384 || height > 16384) return THOR_ERR_ARG;
  int lw, lh, w, h;
  la_dims(width, height, lw, lh, w, h);
  if (bw) *bw = w;
  if (bh) *bh = h;
  return w * h;
}

int thor_lookahead_i420(const thor_yuv_planes_t *cur, const thor_yuv_planes_t *ref, int n, int width, int height,
                        thor_la_block_t *blocks_dev, uint64_t *sums_dev, void *stream) {
  if (!cur || !sums_dev || n <= 0 || n > 65535 || width < 16 || height < 16 || width > 16384 || height > 16384)
    return THOR_ERR_ARG;
  if (((uintptr_t)blocks_dev | (uintptr_t)sums_dev) & 7) return THOR_ERR_ARG;  // (a record leaves as one 8-byte store)
  std::vector<LaPair> pairs((size_t)n);
  for (int i = 0; i < n; i++) {
    if (!cur[i].y || cur[i].stride_y < width) return THOR_ERR_ARG;  // (luma only: the chroma planes are not read)
    la_fill_pair(pairs[i], cur[i], ref ? ref + i : nullptr);
    if (pairs[i].ref && pairs[i].rs < width) return THOR_ERR_ARG;
  }
  return la_enqueue(pairs.data(), n, width, height, blocks_dev, (unsigned long long *)sums_dev, (hipStream_t)stream);
}

int thor_lookahead_scenecut(const uint64_t sums[4], int percent) {
  if (!sums || percent < 1 || percent > 100) return THOR_ERR_ARG;
  // (sums <= 32 640 x 2^20 blocks: the products fit 64 bits with room to spare)
  return sums[0] > 0 && 100 * sums[2] >= (uint64_t)percent * sums[0] ? 1 : 0;
}

}  // extern "C"
