// Frame scaling on the device: planar I420 frames in HBM resized by an integer
// contract (include/thor_amd.h: thor_scaler_create, thor_scale_i420,
// thor_dec_frame_scaled).  The reference has no scaler; the
// contract is this project's, so a rung of an encode ladder is a function of
// the source bytes: the same bytes on every run and every launch shape.
//
// One kernel, one launch per batch: grid z = image x plane.  A 256-lane
// workgroup owns a tile of 64 x 16 output samples: it copies the source window
// the tile needs into LDS in chunks of rows (dword loads, all in flight at
// once), filters each chunk horizontally into an LDS intermediate (int16, 6
// fractional bits, two rows per word), then runs the vertical pass from there;
// both passes are v_dot2_i32_i16 on pairs of taps.
// The decoder context and HIPCHK are capi.hip's; thor_dec_frame_scaled takes the slot from color.hip's
// thor_dec_frame_planes.
#include "frame_ops.h"
#include "scale_host.h"

#define SCALE_INL THOR_SCALE_LAUNCH_IMAGES  // images that travel in the kernel arguments (64 bytes each)
#define SCALE_RAW_BYTES 8192                // LDS for a chunk of the source window
#define SCALE_TPB 4                         // adjacent tiles a workgroup takes, one after the other

// One plane class (0: luma, 1: chroma) -- sizes, table pointers (DEVICE) and the workgroup's LDS layout.
struct ScalePlane {
  const int32_t *hstart;   // per tile column x 64: first source sample of the output column
  const uint32_t *hc;      // horizontal coefficient pairs, (tile, pair, column)
  const int32_t *vpair0;   // per output row: first LDS row pair of its taps
  const int32_t *vy0;      // per tile row: first source row, row count
  const uint32_t *vc;      // vertical coefficient pairs, (row, pair)
  int dw, dh;
  int ntH, npH, npV;       // horizontal taps and pairs, vertical pairs
  int hp;                  // LDS row pairs of the intermediate
  int ndw, cr;             // the source window in LDS: words per row, rows per chunk
  unsigned mndw;           // recon_recip(ndw)
  int tx, ty;              // tiles
  int rsv;
};
struct ScaleImg {
  const uint8_t *s[3];
  uint8_t *d[3];
  int ssy, ssc, dsy, dsc;
};
struct ScaleArgs {
  ScalePlane pl[2];
  ScaleImg img[SCALE_INL];
};
static_assert(sizeof(ScaleImg) == 64 && sizeof(ScalePlane) == 88, "descriptor layout");
static_assert(sizeof(ScaleArgs) <= 2048, "the images travel in the kernarg segment");

struct thor_scaler {
  int sw, sh, dw, dh, filter, device;
  void *tab;  // every table, one allocation
  ScalePlane pl[2];
  size_t lds;
};

typedef short scl_s2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ int scl_dot2(uint32_t a, uint32_t b, int c) {
  return __builtin_amdgcn_sdot2(__builtin_bit_cast(scl_s2, a), __builtin_bit_cast(scl_s2, b), c, false);
}
// clamp((v + 2^19) >> 20) of an accumulator that already holds the rounding term.  The empty asm keeps the
// selector from fusing shift, clamp and pack into v_ashr_pk_u8_i32 (color.hip).
__device__ __forceinline__ uint32_t scl_byte(int acc) {
  int v = min(max(acc >> 20, 0), 255);
#if defined(__HIP_DEVICE_COMPILE__)
  asm("" : "+v"(v));
#endif
  return (uint32_t)v;
}

__device__ __forceinline__ int scl_mis(gcptr p) { return (int)((unsigned long long)p & 3u); }

// What a lane holds of the next chunk while the current one is filtered: its dwords of the source window,
// and with a tile's first chunk its words of the tile's horizontal table.
#define SCALE_NPRE (SCALE_RAW_BYTES / 4 / 256)
#define SCALE_NPREH ((THOR_SCALE_MAX_TAPS + 1) / 2 * 64 / 256 + 1)
struct ScalePre {
  uint32_t raw[SCALE_NPRE], hc[SCALE_NPREH];
  int myoff, xs0, span;
};

// Issue the loads of chunk c (rows [c cr, c cr + rows)) of tile column t; nothing waits here.
__device__ __forceinline__ void scl_fetch(const ScalePlane &P, gcptr plane, int sstride, int y0, int nrows, int t, int c,
                                          int tid, ScalePre &R) {
  // the tile's source span [xs0, xs0 + span) lies inside the row (start[] is clamped on the host), span + 3 <= 4 ndw
  R.xs0 = P.hstart[t * 64];
  R.span = P.hstart[t * 64 + 63] + P.ntH - R.xs0;  // (uniform)
  R.myoff = P.hstart[t * 64 + (tid & 63)] - R.xs0;
  const int ndw = P.ndw, rows = min(P.cr, nrows - c * P.cr), total = rows * ndw;
  const gcptr win = plane + (long long)(y0 + c * P.cr) * sstride + R.xs0;
  // Aligned dwords only: a row is fetched from its span's address rounded down to 4 (scl_mis bytes earlier),
  // so the up to 3 bytes read before and after the span share a dword with a sample of the span.
#pragma unroll
  for (int k = 0; k < SCALE_NPRE; k++) {
    if (256 * k >= total) break;  // (uniform)
    const int idx = 256 * k + tid;
    const int rr = recon_div((unsigned)idx, P.mndw), b = 4 * (idx - rr * ndw);
    const gcptr p = win + (long long)rr * sstride;
    const int mis = scl_mis(p);
    uint32_t v = 0;
    if (idx < total && b < R.span + mis) v = *(const __attribute__((address_space(1))) uint32_t *)(p - mis + b);
    R.raw[k] = v;
  }
  if (c == 0) {
    const uint32_t *hc = P.hc + (size_t)t * P.npH * 64;
#pragma unroll
    for (int k = 0; k < SCALE_NPREH; k++) {
      if (256 * k >= P.npH * 64) break;
      R.hc[k] = 256 * k + tid < P.npH * 64 ? hc[256 * k + tid] : 0u;
    }
  }
}

// grid (ceil(luma tile columns / SCALE_TPB), luma tile rows, 3 x images), 256 threads, dynamic LDS (thor_scaler::lds):
//   [hp x 64] intermediate row pairs | [npH x 64] horizontal pairs | [16 x npV] vertical pairs | [16] pair0 |
//   [cr x ndw + 1] a chunk of the source window.
// A workgroup takes SCALE_TPB adjacent tiles of one tile row, chunk by chunk; the next chunk's loads are in
// flight while the current one is filtered.  Chroma planes use the lower left part of the grid; their other
// workgroups leave at once.
__global__ __launch_bounds__(256) void k_scale_i420(const ScaleArgs A) {
  extern __shared__ uint32_t scl_lds[];
  // (read in place in the kernarg segment: a dynamic index into the by-value argument would copy it to scratch)
  const ScaleArgs *K = (const ScaleArgs *)__builtin_amdgcn_kernarg_segment_ptr();
  const int im = blockIdx.z / 3, pc = blockIdx.z - 3 * im;
  const ScalePlane &P = K->pl[pc ? 1 : 0];
  const int t0 = blockIdx.x * SCALE_TPB, by = blockIdx.y;
  if (t0 >= P.tx || by >= P.ty) return;
  const ScaleImg &I = K->img[im];
  const int sstride = pc ? I.ssc : I.ssy, dstride = pc ? I.dsc : I.dsy;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int npH = P.npH, npV = P.npV, ndw = P.ndw;

  uint32_t *hbuf = scl_lds;
  uint32_t *hcoef = hbuf + P.hp * 64;
  uint32_t *vcoef = hcoef + npH * 64;
  int *vp0 = (int *)(vcoef + SCALE_TILE_H * npV);
  uint32_t *raw = (uint32_t *)(vp0 + SCALE_TILE_H);

  const int y0 = P.vy0[2 * by], nrows = P.vy0[2 * by + 1];
  const int nch = (nrows + P.cr - 1) / P.cr, nwork = min(SCALE_TPB, P.tx - t0) * nch;
  const gcptr plane = (gcptr)I.s[pc];
  ScalePre R;
  scl_fetch(P, plane, sstride, y0, nrows, t0, 0, tid, R);
  // the tile row's vertical table (made visible by the loop's first barrier)
  const int e0 = by * SCALE_TILE_H, ne = min(SCALE_TILE_H, P.dh - e0);
  for (int i = tid; i < SCALE_TILE_H * npV; i += 256) vcoef[i] = i < ne * npV ? P.vc[(size_t)e0 * npV + i] : 0u;
  if (tid < SCALE_TILE_H) vp0[tid] = tid < ne ? P.vpair0[e0 + tid] : 0;

  int t = t0, c = 0, myoff = 0, xs0 = 0;
  for (int w = 0; w < nwork; w++) {
    // the fetched chunk goes to LDS (raw and hcoef are free: the barrier below the horizontal pass)
    const int rows = min(P.cr, nrows - c * P.cr), total = rows * ndw;
#pragma unroll
    for (int k = 0; k < SCALE_NPRE; k++) {
      if (256 * k >= total) break;
      if (256 * k + tid < total) raw[256 * k + tid] = R.raw[k];
    }
    if (c == 0) {
#pragma unroll
      for (int k = 0; k < SCALE_NPREH; k++) {
        if (256 * k >= npH * 64) break;
        if (256 * k + tid < npH * 64) hcoef[256 * k + tid] = R.hc[k];
      }
      myoff = R.myoff, xs0 = R.xs0;
    }
    __syncthreads();
    const int tc = t, cc = c;
    if (++c == nch) c = 0, t++;
    if (w + 1 < nwork) scl_fetch(P, plane, sstride, y0, nrows, t, c, tid, R);
    // horizontal: wave w filters the chunk's rows w, w + 4, ..., a lane per output column
    for (int rr = wave; rr < rows; rr += 4) {
      const int r = cc * P.cr + rr;
      const uint8_t *sb = (const uint8_t *)(raw + rr * ndw) + scl_mis(plane + (long long)(y0 + r) * sstride + xs0) + myoff;
      int acc = 128;
      for (int p = 0; p < npH; p++)
        acc = scl_dot2((uint32_t)sb[2 * p] | ((uint32_t)sb[2 * p + 1] << 16), hcoef[p * 64 + lane], acc);
      ((int16_t *)hbuf)[((r >> 1) * 64 + lane) * 2 + (r & 1)] = (int16_t)(acc >> 8);
    }
    __syncthreads();
    if (cc != nch - 1) continue;
    // vertical: lane = (row of the tile, 4 adjacent columns).  (The next chunk's horizontal pass writes hbuf
    // only after the next barrier, which every lane reaches after this.)
    const int er = tid >> 4, cg = tid & 15, e = e0 + er, d0 = tc * 64 + 4 * cg;
    if (e >= P.dh || d0 >= P.dw) continue;
    const uint4 *hp4 = (const uint4 *)(hbuf + vp0[er] * 64 + 4 * cg);
    const uint32_t *vcr = vcoef + er * npV;
    int a0 = 1 << 19, a1 = 1 << 19, a2 = 1 << 19, a3 = 1 << 19;
    for (int p = 0; p < npV; p++) {
      const uint32_t cf = vcr[p];
      const uint4 v = hp4[p * 16];
      a0 = scl_dot2(v.x, cf, a0);
      a1 = scl_dot2(v.y, cf, a1);
      a2 = scl_dot2(v.z, cf, a2);
      a3 = scl_dot2(v.w, cf, a3);
    }
    const uint32_t b0 = scl_byte(a0), b1 = scl_byte(a1), b2 = scl_byte(a2), b3 = scl_byte(a3);
    const gptr out = (gptr)I.d[pc] + (long long)e * dstride + (unsigned)d0;
    if (d0 + 3 < P.dw) {
      g_st4(out, b0 | (b1 << 8) | (b2 << 16) | (b3 << 24));
    } else {  // the row's ragged end: sample by sample, nothing past dw
      out[0] = (uint8_t)b0;
      if (d0 + 1 < P.dw) out[1] = (uint8_t)b1;
      if (d0 + 2 < P.dw) out[2] = (uint8_t)b2;
    }
  }
}

// Everything that can be refused without a device: THOR_OK or THOR_ERR_ARG.
static int scale_check_images(const thor_scaler *s, const thor_yuv_planes_t *src, const thor_yuv_planes_t *dst, int n) {
  if (!s || !src || !dst || n <= 0 || n > 65535) return THOR_ERR_ARG;
  for (int i = 0; i < n; i++)
    if (!planes_ok(src[i], s->sw) || !planes_ok(dst[i], s->dw)) return THOR_ERR_ARG;
  return THOR_OK;
}

// Launch the scaling of n checked images on `st`, SCALE_INL per launch through the kernel arguments.
static int scale_enqueue(const thor_scaler *s, const thor_yuv_planes_t *src, const thor_yuv_planes_t *dst, int n,
                         hipStream_t st) {
  ScaleArgs A;
  memset(&A, 0, sizeof(A));
  A.pl[0] = s->pl[0];
  A.pl[1] = s->pl[1];
  return launch_batches(n, SCALE_INL, [&](int i0, int m) {
    for (int i = 0; i < m; i++) {
      const thor_yuv_planes_t &a = src[i0 + i], &b = dst[i0 + i];
      A.img[i] = ScaleImg{{a.y, a.u, a.v}, {b.y, b.u, b.v}, a.stride_y, a.stride_c, b.stride_y, b.stride_c};
    }
    k_scale_i420<<<dim3((unsigned)((s->pl[0].tx + SCALE_TPB - 1) / SCALE_TPB), (unsigned)s->pl[0].ty, (unsigned)(3 * m)), 256, s->lds, st>>>(A);
  });
}

extern "C" {

thor_scaler_t *thor_scaler_create(int sw, int sh, int dw, int dh, int filter, int device) {
  create_begin();
  if (thor_scale_check(sw, sh, dw, dh, filter) != THOR_OK) {
    create_fail(THOR_ERR_ARG, 0, "thor_scaler_create: unsupported sizes %dx%d -> %dx%d or filter %d", sw, sh, dw, dh,
                filter);
    return nullptr;
  }
  // the four axis tables: (luma, chroma) x (horizontal, vertical)
  ScaleHTab ht[2];
  ScaleVTab vt[2];
  size_t lds = 0, words = 0, off[2][5];
  for (int c = 0; c < 2; c++) {
    ScaleAxis ah, av;
    if (scale_axis_build(sw >> c, dw >> c, filter, &ah) != THOR_OK ||
        scale_axis_build(sh >> c, dh >> c, filter, &av) != THOR_OK) {
      create_fail(THOR_ERR_ARG, 0, "thor_scaler_create: no tap table for %dx%d -> %dx%d", sw, sh, dw, dh);
      return nullptr;
    }
    scale_htab_build(ah, &ht[c]);
    scale_vtab_build(av, &vt[c]);
    const size_t sizes[5] = {ht[c].start.size(), ht[c].c.size(), vt[c].pair0.size(), vt[c].y0.size(), vt[c].c.size()};
    for (int k = 0; k < 5; k++) {
      off[c][k] = words;
      words += (sizes[k] + 3) & ~(size_t)3;
    }
  }
  if (hipSetDevice(device) != hipSuccess) {
    (void)hipGetLastError();
    create_fail(THOR_ERR_ARG, 0, "thor_scaler_create: no HIP device %d", device);
    return nullptr;
  }
  thor_scaler *s = new thor_scaler();
  s->sw = sw, s->sh = sh, s->dw = dw, s->dh = dh, s->filter = filter, s->device = device;
  std::vector<uint32_t> host(words, 0u);
  if (!dev_alloc((uint32_t **)&s->tab, words * 4, "thor_scaler_create: tap tables")) {
    delete s;
    return nullptr;
  }
  const uint32_t *base = (const uint32_t *)s->tab;
  for (int c = 0; c < 2; c++) {
    memcpy(&host[off[c][0]], ht[c].start.data(), ht[c].start.size() * 4);
    memcpy(&host[off[c][1]], ht[c].c.data(), ht[c].c.size() * 4);
    memcpy(&host[off[c][2]], vt[c].pair0.data(), vt[c].pair0.size() * 4);
    memcpy(&host[off[c][3]], vt[c].y0.data(), vt[c].y0.size() * 4);
    memcpy(&host[off[c][4]], vt[c].c.data(), vt[c].c.size() * 4);
    ScalePlane &P = s->pl[c];
    P.hstart = (const int32_t *)(base + off[c][0]);
    P.hc = base + off[c][1];
    P.vpair0 = (const int32_t *)(base + off[c][2]);
    P.vy0 = (const int32_t *)(base + off[c][3]);
    P.vc = base + off[c][4];
    P.dw = dw >> c, P.dh = dh >> c;
    P.ntH = ht[c].nt;
    P.npH = ht[c].np, P.npV = vt[c].np;
    P.hp = (vt[c].rows + 2) / 2;
    P.ndw = (ht[c].span + 3 + 3) / 4;  // (+ 3: a row is fetched from an aligned address)
    P.mndw = recon_recip((unsigned)P.ndw);
    // chunks of at most SCALE_RAW_BYTES, at least 4 rows (one per wave)
    P.cr = SCALE_RAW_BYTES / (4 * P.ndw) > 4 ? SCALE_RAW_BYTES / (4 * P.ndw) : 4;
    if (P.cr > vt[c].rows) P.cr = vt[c].rows;
    P.tx = ht[c].tiles, P.ty = (P.dh + SCALE_TILE_H - 1) / SCALE_TILE_H;
    const size_t w = (size_t)P.hp * 64 + (size_t)P.npH * 64 + (size_t)SCALE_TILE_H * P.npV + SCALE_TILE_H +
                     (size_t)P.cr * P.ndw + 1;  // + 1: an odd tap count's last pair reads one byte past the row (times 0)
    if (w * 4 > lds) lds = w * 4;
  }
  s->lds = lds;
  if (lds > 64 * 1024) {  // (8:1 cubic needs 34 KB)
    create_fail(THOR_ERR_ARG, 0, "thor_scaler_create: the tile needs %zu bytes of LDS", lds);
    thor_scaler_destroy(s);
    return nullptr;
  }
  if (hipMemcpy(s->tab, host.data(), words * 4, hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipGetLastError();
    create_fail(THOR_ERR_HIP, 0, "thor_scaler_create: table upload failed");
    thor_scaler_destroy(s);
    return nullptr;
  }
  return s;
}

void thor_scaler_destroy(thor_scaler_t *s) {
  if (!s) return;
  (void)hipSetDevice(s->device);
  if (s->tab) (void)hipFree(s->tab);
  delete s;
}

int thor_scale_i420(thor_scaler_t *s, const thor_yuv_planes_t *src, const thor_yuv_planes_t *dst, int n, void *stream) {
  const int rc = scale_check_images(s, src, dst, n);
  if (rc != THOR_OK) return rc;
  HIPCHK(hipSetDevice(s->device));
  return scale_enqueue(s, src, dst, n, (hipStream_t)stream);
}

int thor_dec_frame_scaled(thor_dec_t *d, int frame_num, thor_scaler_t *s, const thor_yuv_planes_t *dst) {
  if (!d || !s || !dst) return THOR_ERR_ARG;
  if (s->sw != d->seq.width || s->sh != d->seq.height || s->device != d->device) return THOR_ERR_ARG;
  thor_yuv_planes_t rec;
  const int rc = thor_dec_frame_planes(d, frame_num, &rec);
  if (rc != THOR_OK) return rc;
  if (scale_check_images(s, &rec, dst, 1) != THOR_OK) return THOR_ERR_ARG;
  HIPCHK(hipSetDevice(d->device));
  return scale_enqueue(s, &rec, dst, 1, d->stream);
}

}  // extern "C"
