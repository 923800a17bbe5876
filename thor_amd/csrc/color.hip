// Colour conversion on the device: planar I420 <-> RGB images in HBM
// (include/thor_amd.h: thor_csc_coeffs, thor_i420_to_rgb, thor_rgb_to_i420,
// thor_dec_frame_planes, thor_dec_frame_rgb).  The reference has no colour
// conversion; the arithmetic is this project's contract, in
// integers, so a stream decoded to RGB is the same bytes on every run and every
// launch shape, as its I420 already is.
//
// Two streaming kernels, one per direction; format and chroma mode are
// template parameters, the frame is grid dimension z.  A lane owns a strip two
// rows high and 8 pixels wide, so both rows share one chroma fetch; a wave
// reads and writes contiguous row segments (64 strips = 512 pixels).
// The decoder context, find_slot_host and HIPCHK are capi.hip's.
#include "frame_ops.h"

#define CSC_INL THOR_CSC_LAUNCH_IMAGES  // images that travel in the kernel arguments (56 bytes each)

struct CscImg {
  uint8_t *y, *u, *v;  // I420 interior (0, 0)
  uint8_t *rgb;        // R of pixel (0, 0)
  long long ps;        // bytes between RGB planes
  int sy, sc, rs;      // luma / chroma / RGB row stride (bytes)
  int rsv;
};
struct CscArgs {
  int W, H;
  // to RGB:   k[3 c + {0, 1, 2}] = 16 I[c][0], I[c][1], I[c][2]; k[9 + c] = the row's constant
  // from RGB: k[0..8] = F; k[9] = Y constant, k[10] = chroma constant
  int k[12];
  CscImg inl[CSC_INL];
};
static_assert(sizeof(CscImg) == 56, "image descriptor layout");
static_assert(sizeof(CscArgs) <= 1024, "the images travel in the kernarg segment");

// (14-bit fixed point; the Y row sums to round(ys * 2^14), the chroma rows to 0: include/thor_amd.h)
static const int32_t CSC_FWD[4][9] = {
    {4207, 8260, 1604, -2428, -4768, 7196, 7196, -6026, -1170},   // BT.601 limited
    {4899, 9617, 1868, -2765, -5427, 8192, 8192, -6860, -1332},   // BT.601 full
    {2991, 10064, 1016, -1649, -5547, 7196, 7196, -6536, -660},   // BT.709 limited
    {3483, 11718, 1183, -1877, -6315, 8192, 8192, -7441, -751}};  // BT.709 full
static const int32_t CSC_INV[4][9] = {{19077, 0, 26149, 19077, -6419, -13320, 19077, 33050, 0},
                                      {16384, 0, 22970, 16384, -5638, -11700, 16384, 29032, 0},
                                      {19077, 0, 29372, 19077, -3494, -8731, 19077, 34610, 0},
                                      {16384, 0, 25802, 16384, -3069, -7670, 16384, 30402, 0}};

// Every global address (frame_ops.h) is a uniform row base plus the lane's unsigned offset (SGPR base + 32-bit
// VGPR offset).
__device__ __forceinline__ int csc_byte(uint32_t v, int k) { return (int)((v >> (8 * k)) & 255u); }
// clamp to [0, 255].  The empty asm hides the result's origin from the instruction selector: it would
// otherwise fuse shift, clamp and the packing of two such bytes into v_ashr_pk_u8_i32 and or the other two
// bytes of the dword on top of it, and on the MI355X the dwords packed that way came out with bytes 2 and 3
// wrong (the instruction's upper result half is not the zero the selector takes it for).
__device__ __forceinline__ int csc_clamp8(int v) {
  v = min(max(v, 0), 255);
#if defined(__HIP_DEVICE_COMPILE__)
  asm("" : "+v"(v));
#endif
  return v;
}
__device__ __forceinline__ uint32_t csc_pack4(int a, int b, int c, int d) {
  return (uint32_t)a | ((uint32_t)b << 8) | ((uint32_t)c << 16) | ((uint32_t)d << 24);
}
// byte -> float in [0, 1]: one multiply by the float32 nearest 1/255 (255 -> exactly 1.0f)
__device__ __forceinline__ float csc_unorm(int q) { return (float)q * 0x1.010102p-8f; }
// float -> byte: clamp(rint(v * 255)), half to even, NaN -> 0 (fmaxf returns the other operand)
__device__ __forceinline__ int csc_quant(float v) { return (int)fminf(fmaxf(rintf(v * 255.0f), 0.0f), 255.0f); }

// to RGB: out_c = clamp((I[c][0] 16 (Y - yo) + I[c][1] (Cb16 - 2048) + I[c][2] (Cr16 - 2048) + 2^17) >> 18); the
// offsets are folded into the row's constant k[9 + c], and every product fits 24 x 24 bits.
__device__ __forceinline__ int csc_rgb(const int *k, int c, int y, int u16, int v16) {
  return csc_clamp8((__mul24(k[3 * c], y) + __mul24(k[3 * c + 1], u16) + __mul24(k[3 * c + 2], v16) + k[9 + c]) >> 18);
}
// from RGB: Y = clamp((F00 r + F01 g + F02 b + (yo << 14) + 2^13) >> 14); Cb / Cr from a 2x2 block's channel
// sums, clamp((F1. / F2. (Rs, Gs, Bs) + (128 << 16) + 2^15) >> 16): a box filter with one rounding.
__device__ __forceinline__ int csc_luma(const int *k, int r, int g, int b) {
  return csc_clamp8((__mul24(k[0], r) + __mul24(k[1], g) + __mul24(k[2], b) + k[9]) >> 14);
}
__device__ __forceinline__ int csc_chroma(const int *k, int row, int rs, int gs, int bs) {
  return csc_clamp8((__mul24(k[3 * row], rs) + __mul24(k[3 * row + 1], gs) + __mul24(k[3 * row + 2], bs) + k[10]) >> 16);
}

// One pixel of an RGB image (frames narrower than a strip take this path, a lane per 2x2 block).
template <int FMT>
__device__ __forceinline__ void csc_put_px(const CscImg &P, int x, int y, const int px[3]) {
  const gptr row = (gptr)P.rgb + (long long)y * P.rs;
  for (int c = 0; c < 3; c++) {
    if (FMT == THOR_RGB8_PACKED) row[(unsigned)(3 * x + c)] = (uint8_t)px[c];
    else if (FMT == THOR_RGB8_PLANAR) (row + c * P.ps)[(unsigned)x] = (uint8_t)px[c];
    else ((gptrf)(row + c * P.ps))[(unsigned)x] = csc_unorm(px[c]);
  }
}
template <int FMT>
__device__ __forceinline__ void csc_get_px(const CscImg &P, int x, int y, int px[3]) {
  const gcptr row = (gcptr)P.rgb + (long long)y * P.rs;
  for (int c = 0; c < 3; c++) {
    if (FMT == THOR_RGB8_PACKED) px[c] = row[(unsigned)(3 * x + c)];
    else if (FMT == THOR_RGB8_PLANAR) px[c] = (row + c * P.ps)[(unsigned)x];
    else px[c] = csc_quant(((gcptrf)(row + c * P.ps))[(unsigned)x]);
  }
}

// One chroma row's six samples around a strip: c[0] = left neighbour, c[1..4] = the strip's (one dword),
// c[5] = right neighbour, the neighbours clamped to [0, CW - 1]: a second and third load that hit the
// cache lines the adjacent lanes fetch.
template <int BILIN>
__device__ __forceinline__ void csc_chroma_row(gcptr row, int cx0, int CW, int c[6]) {
  const uint32_t d = g_ld4(row + (unsigned)cx0);
#pragma unroll
  for (int j = 0; j < 4; j++) c[1 + j] = csc_byte(d, j);
  if (BILIN) {
    c[0] = row[(unsigned)max(cx0 - 1, 0)];
    c[5] = row[(unsigned)min(cx0 + 4, CW - 1)];
  }
}
// Horizontal half of the bilinear tap for the strip's 8 pixels: 3 * own sample + the neighbour towards the pixel.
__device__ __forceinline__ void csc_chroma_h(const int c[6], int h[8]) {
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const int k = 1 + (i >> 1);
    h[i] = 3 * c[k] + c[(i & 1) ? k + 1 : k - 1];
  }
}

// grid (ceil(W / 512), ceil(H / 8), images), 256 threads: wave w of block (x, y) takes luma rows
// 2 (4 y + w), + 1 and strips [64 x, 64 x + 64) of image z.  A row's last strip starts at W - 8: when W is
// no multiple of 8 it overlaps its neighbour, and both lanes write the same bytes there.  No LDS, no scratch.
template <int FMT, int BILIN>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_csc_to_rgb(const CscArgs A) {
  // (the images are read in place in the kernarg segment: a dynamic index into the by-value
  // argument would copy it to scratch)
  const CscImg P = ((const CscArgs *)__builtin_amdgcn_kernarg_segment_ptr())->inl[blockIdx.z];
  const int W = A.W, CW = W >> 1, CH = A.H >> 1;
  const int cy = blockIdx.y * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // (uniform: SGPRs)
  const int strip = blockIdx.x * 64 + (threadIdx.x & 63);
  if (cy >= CH) return;
  const gcptr Y = (gcptr)P.y + (long long)(2 * cy) * P.sy;
  const gcptr U = (gcptr)P.u + (long long)cy * P.sc, V = (gcptr)P.v + (long long)cy * P.sc;
  if (W < 8) {  // (uniform) narrower than a strip: a lane per 2x2 block, sample by sample
    const int bx = strip;
    if (bx >= CW) return;
    for (int r = 0; r < 2; r++)
      for (int dx = 0; dx < 2; dx++) {
        int u16 = 16 * U[(unsigned)bx], v16 = 16 * V[(unsigned)bx];
        if (BILIN) {
          const int nx = dx ? min(bx + 1, CW - 1) : max(bx - 1, 0), ny = r ? min(cy + 1, CH - 1) : max(cy - 1, 0);
          const gcptr Un = (gcptr)P.u + (long long)ny * P.sc, Vn = (gcptr)P.v + (long long)ny * P.sc;
          u16 = 9 * U[(unsigned)bx] + 3 * U[(unsigned)nx] + 3 * Un[(unsigned)bx] + Un[(unsigned)nx];
          v16 = 9 * V[(unsigned)bx] + 3 * V[(unsigned)nx] + 3 * Vn[(unsigned)bx] + Vn[(unsigned)nx];
        }
        const int yv = (Y + (long long)r * P.sy)[(unsigned)(2 * bx + dx)];
        const int px[3] = {csc_rgb(A.k, 0, yv, u16, v16), csc_rgb(A.k, 1, yv, u16, v16), csc_rgb(A.k, 2, yv, u16, v16)};
        csc_put_px<FMT>(P, 2 * bx + dx, 2 * cy + r, px);
      }
    return;
  }
  if (strip * 8 >= W) return;
  const int x0 = min(strip * 8, W - 8), cx0 = x0 >> 1;

  const u32x2 yr[2] = {g_ld8(Y + (unsigned)x0), g_ld8(Y + P.sy + (unsigned)x0)};
  // chroma: the strip's row, and for bilinear the rows above and below it (clamped at the frame edge)
  int cu[6], cv[6];
  csc_chroma_row<BILIN>(U, cx0, CW, cu);
  csc_chroma_row<BILIN>(V, cx0, CW, cv);
#pragma unroll
  for (int r = 0; r < 2; r++) {
    int u16[8], v16[8];
    if (BILIN) {
      const int ny = r ? min(cy + 1, CH - 1) : max(cy - 1, 0);
      int nu[6], nv[6], h[8], g[8];
      csc_chroma_row<1>((gcptr)P.u + (long long)ny * P.sc, cx0, CW, nu);
      csc_chroma_h(cu, h);
      csc_chroma_h(nu, g);
#pragma unroll
      for (int i = 0; i < 8; i++) u16[i] = 3 * h[i] + g[i];
      csc_chroma_row<1>((gcptr)P.v + (long long)ny * P.sc, cx0, CW, nv);
      csc_chroma_h(cv, h);
      csc_chroma_h(nv, g);
#pragma unroll
      for (int i = 0; i < 8; i++) v16[i] = 3 * h[i] + g[i];
    } else {
#pragma unroll
      for (int i = 0; i < 8; i++) u16[i] = 16 * cu[1 + (i >> 1)], v16[i] = 16 * cv[1 + (i >> 1)];
    }
    int yv[8];
#pragma unroll
    for (int i = 0; i < 8; i++) yv[i] = csc_byte(i < 4 ? yr[r].x : yr[r].y, i & 3);
    const gptr row = (gptr)P.rgb + (long long)(2 * cy + r) * P.rs;
    if (FMT == THOR_RGB8_PACKED) {  // 24 contiguous bytes: a wave writes 1 536 contiguous bytes per row
      int px[3][8];
#pragma unroll
      for (int i = 0; i < 8; i++)
#pragma unroll
        for (int c = 0; c < 3; c++) px[c][i] = csc_rgb(A.k, c, yv[i], u16[i], v16[i]);
      uint32_t d[6];
#pragma unroll
      for (int j = 0; j < 6; j++) {
        int b[4];
#pragma unroll
        for (int t = 0; t < 4; t++) b[t] = px[(4 * j + t) % 3][(4 * j + t) / 3];
        d[j] = csc_pack4(b[0], b[1], b[2], b[3]);
      }
      const gptr o = row + (unsigned)(x0 * 3);
      g_st8(o, u32x2{d[0], d[1]});
      g_st8(o + 8, u32x2{d[2], d[3]});
      g_st8(o + 16, u32x2{d[4], d[5]});
    } else if (FMT == THOR_RGB8_PLANAR) {
#pragma unroll
      for (int c = 0; c < 3; c++) {  // a plane at a time
        int px[8];
#pragma unroll
        for (int i = 0; i < 8; i++) px[i] = csc_rgb(A.k, c, yv[i], u16[i], v16[i]);
        g_st8(row + c * P.ps + (unsigned)x0,
                u32x2{csc_pack4(px[0], px[1], px[2], px[3]), csc_pack4(px[4], px[5], px[6], px[7])});
      }
    } else {
#pragma unroll
      for (int c = 0; c < 3; c++) {
        int px[8];
#pragma unroll
        for (int i = 0; i < 8; i++) px[i] = csc_rgb(A.k, c, yv[i], u16[i], v16[i]);
        const gptrf o = (gptrf)(row + c * P.ps) + (unsigned)x0;
        g_st16f(o, f32x4{csc_unorm(px[0]), csc_unorm(px[1]), csc_unorm(px[2]), csc_unorm(px[3])});
        g_st16f(o + 4, f32x4{csc_unorm(px[4]), csc_unorm(px[5]), csc_unorm(px[6]), csc_unorm(px[7])});
      }
    }
  }
}

// Same grid and strips.  A lane reads its strip's 2 x 8 RGB pixels, writes 2 x 8 luma bytes and 4 + 4 chroma bytes.
template <int FMT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_csc_from_rgb(const CscArgs A) {
  const CscImg P = ((const CscArgs *)__builtin_amdgcn_kernarg_segment_ptr())->inl[blockIdx.z];
  const int W = A.W, CW = W >> 1, CH = A.H >> 1;
  const int cy = blockIdx.y * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int strip = blockIdx.x * 64 + (threadIdx.x & 63);
  if (cy >= CH) return;
  const gptr U = (gptr)P.u + (long long)cy * P.sc, V = (gptr)P.v + (long long)cy * P.sc;
  if (W < 8) {  // (uniform) a lane per 2x2 block
    const int bx = strip;
    if (bx >= CW) return;
    int sum[3] = {0, 0, 0};
    for (int r = 0; r < 2; r++)
      for (int dx = 0; dx < 2; dx++) {
        int px[3];
        csc_get_px<FMT>(P, 2 * bx + dx, 2 * cy + r, px);
        ((gptr)P.y + (long long)(2 * cy + r) * P.sy)[(unsigned)(2 * bx + dx)] = (uint8_t)csc_luma(A.k, px[0], px[1], px[2]);
        for (int c = 0; c < 3; c++) sum[c] += px[c];
      }
    U[(unsigned)bx] = (uint8_t)csc_chroma(A.k, 1, sum[0], sum[1], sum[2]);
    V[(unsigned)bx] = (uint8_t)csc_chroma(A.k, 2, sum[0], sum[1], sum[2]);
    return;
  }
  if (strip * 8 >= W) return;
  const int x0 = min(strip * 8, W - 8), cx0 = x0 >> 1;

  int sum[3][4];  // per 2x2 block: the four pixels' R, G, B sums
#pragma unroll
  for (int r = 0; r < 2; r++) {
    int px[3][8];
    const gcptr row = (gcptr)P.rgb + (long long)(2 * cy + r) * P.rs;
    if (FMT == THOR_RGB8_PACKED) {
      const gcptr s = row + (unsigned)(x0 * 3);
      const u32x2 a = g_ld8(s), b = g_ld8(s + 8), c = g_ld8(s + 16);
      const uint32_t d[6] = {a.x, a.y, b.x, b.y, c.x, c.y};
#pragma unroll
      for (int j = 0; j < 24; j++) px[j % 3][j / 3] = csc_byte(d[j >> 2], j & 3);
    } else if (FMT == THOR_RGB8_PLANAR) {
#pragma unroll
      for (int c = 0; c < 3; c++) {
        const u32x2 d = g_ld8(row + c * P.ps + (unsigned)x0);
#pragma unroll
        for (int i = 0; i < 8; i++) px[c][i] = csc_byte(i < 4 ? d.x : d.y, i & 3);
      }
    } else {
#pragma unroll
      for (int c = 0; c < 3; c++) {
        const gcptrf s = (gcptrf)(row + c * P.ps) + (unsigned)x0;
        const f32x4 a = g_ld16f(s), b = g_ld16f(s + 4);
        px[c][0] = csc_quant(a.x), px[c][1] = csc_quant(a.y), px[c][2] = csc_quant(a.z), px[c][3] = csc_quant(a.w);
        px[c][4] = csc_quant(b.x), px[c][5] = csc_quant(b.y), px[c][6] = csc_quant(b.z), px[c][7] = csc_quant(b.w);
      }
    }
    int yv[8];
#pragma unroll
    for (int i = 0; i < 8; i++) yv[i] = csc_luma(A.k, px[0][i], px[1][i], px[2][i]);
    g_st8((gptr)P.y + (long long)(2 * cy + r) * P.sy + (unsigned)x0,
            u32x2{csc_pack4(yv[0], yv[1], yv[2], yv[3]), csc_pack4(yv[4], yv[5], yv[6], yv[7])});
#pragma unroll
    for (int c = 0; c < 3; c++)
#pragma unroll
      for (int j = 0; j < 4; j++) sum[c][j] = (r ? sum[c][j] : 0) + px[c][2 * j] + px[c][2 * j + 1];
  }
  int cb[4], cr[4];
#pragma unroll
  for (int j = 0; j < 4; j++) {
    cb[j] = csc_chroma(A.k, 1, sum[0][j], sum[1][j], sum[2][j]);
    cr[j] = csc_chroma(A.k, 2, sum[0][j], sum[1][j], sum[2][j]);
  }
  g_st4(U + (unsigned)cx0, csc_pack4(cb[0], cb[1], cb[2], cb[3]));
  g_st4(V + (unsigned)cx0, csc_pack4(cr[0], cr[1], cr[2], cr[3]));
}

// Everything that can be refused without a device: THOR_OK or THOR_ERR_ARG.
static int csc_check(const thor_yuv_planes_t *yuv, const thor_image_t *img, int n, int W, int H, const thor_csc_t *csc,
                     bool to_rgb) {
  if (!yuv || !img || !csc || n <= 0 || n > 65535) return THOR_ERR_ARG;
  if (W < 2 || H < 2 || (W & 1) || (H & 1) || W > (1 << 24) || H > (1 << 19)) return THOR_ERR_ARG;  // (grid limits)
  if (csc->matrix < 0 || csc->matrix > 1 || csc->full_range < 0 || csc->full_range > 1) return THOR_ERR_ARG;
  if (to_rgb && (csc->chroma_up < 0 || csc->chroma_up > 1)) return THOR_ERR_ARG;
  const int fmt = img[0].format;
  if (fmt != THOR_RGB8_PACKED && fmt != THOR_RGB8_PLANAR && fmt != THOR_RGBF32_PLANAR) return THOR_ERR_ARG;
  const long long row = fmt == THOR_RGB8_PACKED ? 3LL * W : fmt == THOR_RGB8_PLANAR ? (long long)W : 4LL * W;
  for (int i = 0; i < n; i++) {
    if (!planes_ok(yuv[i], W) || !img[i].data || img[i].format != fmt || img[i].stride < row) return THOR_ERR_ARG;
    if (fmt == THOR_RGBF32_PLANAR &&
        (((uintptr_t)img[i].data | (uintptr_t)(unsigned)img[i].stride | (uintptr_t)img[i].plane_stride) & 3))
      return THOR_ERR_ARG;
  }
  return THOR_OK;
}

template <int FMT>
static void csc_launch_to(int bilin, dim3 g, hipStream_t st, const CscArgs &A) {
  if (bilin)
    k_csc_to_rgb<FMT, 1><<<g, 256, 0, st>>>(A);
  else
    k_csc_to_rgb<FMT, 0><<<g, 256, 0, st>>>(A);
}

// Launch the conversion of n checked images on `st`, CSC_INL per launch through the kernel arguments.
static int csc_enqueue(const thor_yuv_planes_t *yuv, const thor_image_t *img, int n, int W, int H, const thor_csc_t *csc,
                       bool to_rgb, hipStream_t st) {
  CscArgs A;
  memset(&A, 0, sizeof(A));
  A.W = W;
  A.H = H;
  const int t = csc->matrix * 2 + csc->full_range, yo = csc->full_range ? 0 : 16;
  if (to_rgb) {
    const int32_t *I = CSC_INV[t];
    for (int c = 0; c < 3; c++) {
      A.k[3 * c] = 16 * I[3 * c];
      A.k[3 * c + 1] = I[3 * c + 1];
      A.k[3 * c + 2] = I[3 * c + 2];
      A.k[9 + c] = (1 << 17) - 16 * yo * I[3 * c] - 2048 * (I[3 * c + 1] + I[3 * c + 2]);
    }
  } else {
    for (int j = 0; j < 9; j++) A.k[j] = CSC_FWD[t][j];
    A.k[9] = (yo << 14) + (1 << 13);
    A.k[10] = (128 << 16) + (1 << 15);
  }
  const int fmt = img[0].format;
  const unsigned gx = (unsigned)((W + 511) / 512), gy = (unsigned)(((H >> 1) + 3) / 4);
  return launch_batches(n, CSC_INL, [&](int i0, int m) {
    for (int i = 0; i < m; i++) {
      const thor_yuv_planes_t &y = yuv[i0 + i];
      const thor_image_t &r = img[i0 + i];
      A.inl[i] = CscImg{y.y, y.u, y.v, (uint8_t *)r.data, fmt == THOR_RGB8_PACKED ? 0 : (long long)r.plane_stride,
                        y.stride_y, y.stride_c, r.stride, 0};
    }
    const dim3 g(gx, gy, (unsigned)m);
    if (to_rgb) {
      if (fmt == THOR_RGB8_PACKED) csc_launch_to<THOR_RGB8_PACKED>(csc->chroma_up, g, st, A);
      else if (fmt == THOR_RGB8_PLANAR) csc_launch_to<THOR_RGB8_PLANAR>(csc->chroma_up, g, st, A);
      else csc_launch_to<THOR_RGBF32_PLANAR>(csc->chroma_up, g, st, A);
    } else {
      if (fmt == THOR_RGB8_PACKED) k_csc_from_rgb<THOR_RGB8_PACKED><<<g, 256, 0, st>>>(A);
      else if (fmt == THOR_RGB8_PLANAR) k_csc_from_rgb<THOR_RGB8_PLANAR><<<g, 256, 0, st>>>(A);
      else k_csc_from_rgb<THOR_RGBF32_PLANAR><<<g, 256, 0, st>>>(A);
    }
  });
}

extern "C" {

int thor_csc_coeffs(int matrix, int full_range, int32_t fwd[9], int32_t inv[9]) {
  if (matrix < 0 || matrix > 1 || full_range < 0 || full_range > 1) return THOR_ERR_ARG;
  const int t = matrix * 2 + full_range;
  if (fwd) memcpy(fwd, CSC_FWD[t], sizeof(CSC_FWD[t]));
  if (inv) memcpy(inv, CSC_INV[t], sizeof(CSC_INV[t]));
  return THOR_OK;
}

int thor_i420_to_rgb(const thor_yuv_planes_t *src, const thor_image_t *dst, int n, int width, int height,
                     const thor_csc_t *csc, void *stream) {
  const int rc = csc_check(src, dst, n, width, height, csc, true);
  if (rc != THOR_OK) return rc;
  return csc_enqueue(src, dst, n, width, height, csc, true, (hipStream_t)stream);
}

int thor_rgb_to_i420(const thor_image_t *src, const thor_yuv_planes_t *dst, int n, int width, int height,
                     const thor_csc_t *csc, void *stream) {
  const int rc = csc_check(dst, src, n, width, height, csc, false);
  if (rc != THOR_OK) return rc;
  return csc_enqueue(dst, src, n, width, height, csc, false, (hipStream_t)stream);
}

int thor_dec_frame_planes(thor_dec_t *d, int frame_num, thor_yuv_planes_t *out) {
  if (!d || !out) return THOR_ERR_ARG;
  const int s = find_slot_host(d, frame_num);
  if (s < 0) return THOR_ERR_REF;
  *out = slot_planes(d, s);
  return THOR_OK;
}

int thor_dec_frame_rgb(thor_dec_t *d, int frame_num, const thor_image_t *dst, const thor_csc_t *csc) {
  if (!d || !dst || !csc) return THOR_ERR_ARG;
  thor_yuv_planes_t rec;
  const int rc = thor_dec_frame_planes(d, frame_num, &rec);
  if (rc != THOR_OK) return rc;
  if (csc_check(&rec, dst, 1, d->seq.width, d->seq.height, csc, true) != THOR_OK) return THOR_ERR_ARG;
  HIPCHK(hipSetDevice(d->device));
  return csc_enqueue(&rec, dst, 1, d->seq.width, d->seq.height, csc, true, d->stream);
}

}  // extern "C"
