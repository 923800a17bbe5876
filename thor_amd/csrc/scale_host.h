// Host side of the frame scaler (thor_scale_taps / thor_scale_check,
// include/thor_amd.h; the contract is DESIGN.md sec. 7d): the per-axis tap
// tables in exact integers, and the form the kernel reads them in (edge clamp
// folded into the coefficients, packed in pairs for v_dot2_i32_i16).  Plain
// C++, no HIP types, usable without a device.  Included once, by scale.hip.
#pragma once
#include <stdint.h>

#include <vector>

#include "../../include/thor_amd.h"

#define SCALE_UNIT 16384
#define SCALE_TILE_W 64  // output columns / rows of a workgroup's tile (scale.hip)
#define SCALE_TILE_H 16

static inline long long scale_floordiv(long long a, long long b) {  // b > 0; towards -inf
  return a >= 0 ? a / b : -((-a + b - 1) / b);
}
static inline int scale_axis_ok(int S, int D) {
  return S >= 1 && D >= 1 && S <= THOR_SCALE_MAX_SIZE && D <= THOR_SCALE_MAX_SIZE && S <= 8LL * D;
}
// numerator of the filter at distance u / M, 0 <= u < R M
static inline long long scale_weight(long long u, long long M, int filter) {
  if (filter == THOR_SCALE_BILINEAR) return M - u;
  if (u < M) return 3 * u * u * u - 5 * M * u * u + 2 * M * M * M;
  return -u * u * u + 5 * M * u * u - 8 * M * M * u + 4 * M * M * M;
}
// The taps of output d: s0 and the count are returned, c[0 .. count) filled (count <= THOR_SCALE_MAX_TAPS).
static inline int scale_row(int S, int D, int filter, int d, int32_t *s0_out, int16_t *c) {
  const long long R = filter == THOR_SCALE_BILINEAR ? 1 : 2, M = 2LL * (S > D ? S : D);
  const long long c2 = (2LL * d + 1) * S - D;
  const long long s0 = scale_floordiv(c2 - R * M, 2LL * D) + 1, s1 = -scale_floordiv(-(c2 + R * M), 2LL * D) - 1;
  const int n = (int)(s1 - s0 + 1);
  *s0_out = (int32_t)s0;
  if (n < 1 || n > THOR_SCALE_MAX_TAPS) return -1;
  long long P[THOR_SCALE_MAX_TAPS], T = 0;
  int best = 0;
  for (int k = 0; k < n; k++) {
    const long long t = 2LL * D * (s0 + k) - c2;
    P[k] = scale_weight(t < 0 ? -t : t, M, filter);
    T += P[k];
    if (P[k] > P[best]) best = k;
  }
  long long sum = 0, q[THOR_SCALE_MAX_TAPS];
  for (int k = 0; k < n; k++) {
    q[k] = scale_floordiv(2 * P[k] * SCALE_UNIT + T, 2 * T);
    sum += q[k];
  }
  q[best] += SCALE_UNIT - sum;
  for (int k = 0; k < n; k++) c[k] = (int16_t)q[k];
  return n;
}

int thor_scale_taps(int S, int D, int filter, int32_t *first, int16_t *coef, int *ntaps) {
  if (!ntaps || !scale_axis_ok(S, D) || (filter != THOR_SCALE_BILINEAR && filter != THOR_SCALE_BICUBIC))
    return THOR_ERR_ARG;
  int16_t c[THOR_SCALE_MAX_TAPS];
  int32_t s0;
  int nt = 0;
  for (int d = 0; d < D; d++) {
    const int n = scale_row(S, D, filter, d, &s0, c);
    if (n < 0) return THOR_ERR_ARG;
    if (n > nt) nt = n;
  }
  *ntaps = nt;
  if (!first || !coef) return THOR_OK;
  for (int d = 0; d < D; d++) {
    const int n = scale_row(S, D, filter, d, &first[d], c);
    for (int k = 0; k < nt; k++) coef[(size_t)d * nt + k] = k < n ? c[k] : 0;
  }
  return THOR_OK;
}

int thor_scale_check(int sw, int sh, int dw, int dh, int filter) {
  if (filter != THOR_SCALE_BILINEAR && filter != THOR_SCALE_BICUBIC) return THOR_ERR_ARG;
  const int v[4] = {sw, sh, dw, dh};
  for (int i = 0; i < 4; i++)
    if (v[i] < 2 || (v[i] & 1) || v[i] > THOR_SCALE_MAX_SIZE) return THOR_ERR_ARG;
  if (sw > 8LL * dw || sh > 8LL * dh) return THOR_ERR_ARG;
  return THOR_OK;
}

// One axis as the kernel reads it.  The edge clamp is folded in: the coefficients of taps outside
// [0, S - 1] are added to the edge sample's (the same integer), so a row is nt = min(ntaps, S)
// coefficients for the in-range samples start[d] .. start[d] + nt - 1, start non-decreasing.
struct ScaleAxis {
  int S, D, nt;
  std::vector<int32_t> start;
  std::vector<int16_t> c;  // D x nt
};
static inline int scale_axis_build(int S, int D, int filter, ScaleAxis *a) {
  int ntaps = 0;
  if (thor_scale_taps(S, D, filter, nullptr, nullptr, &ntaps) != THOR_OK) return THOR_ERR_ARG;
  std::vector<int32_t> first((size_t)D);
  std::vector<int16_t> coef((size_t)D * ntaps);
  thor_scale_taps(S, D, filter, first.data(), coef.data(), &ntaps);
  const int nt = ntaps < S ? ntaps : S;
  a->S = S, a->D = D, a->nt = nt;
  a->start.assign((size_t)D, 0);
  a->c.assign((size_t)D * nt, 0);
  for (int d = 0; d < D; d++) {
    int st = first[d] < 0 ? 0 : first[d];
    if (st > S - nt) st = S - nt;
    a->start[d] = st;
    for (int k = 0; k < ntaps; k++) {
      int s = first[d] + k;
      s = s < 0 ? 0 : (s > S - 1 ? S - 1 : s);
      const int j = s - st;
      if (j < 0 || j >= nt) {
        if (coef[(size_t)d * ntaps + k]) return THOR_ERR_ARG;  // (cannot happen: see DESIGN.md sec. 7d)
        continue;
      }
      a->c[(size_t)d * nt + j] = (int16_t)(a->c[(size_t)d * nt + j] + coef[(size_t)d * ntaps + k]);
    }
  }
  return THOR_OK;
}

// The horizontal table, per tile of SCALE_TILE_W output columns: word (tile * np + p) * 64 + col holds
// coefficients 2p (low half) and 2p + 1 of column 64 tile + col; columns past D - 1 repeat start[D - 1] with
// zero coefficients.  span = the longest source span of a tile (bytes), np = ceil(nt / 2).
struct ScaleHTab {
  int nt, np, span, tiles;
  std::vector<int32_t> start;  // tiles x 64
  std::vector<uint32_t> c;
};
static inline void scale_htab_build(const ScaleAxis &a, ScaleHTab *t) {
  const int tiles = (a.D + SCALE_TILE_W - 1) / SCALE_TILE_W, np = (a.nt + 1) / 2;
  t->nt = a.nt, t->np = np, t->tiles = tiles, t->span = 0;
  t->start.assign((size_t)tiles * SCALE_TILE_W, 0);
  t->c.assign((size_t)tiles * np * SCALE_TILE_W, 0);
  for (int tl = 0; tl < tiles; tl++) {
    for (int col = 0; col < SCALE_TILE_W; col++) {
      const int d = tl * SCALE_TILE_W + col, dd = d < a.D ? d : a.D - 1;
      t->start[(size_t)tl * SCALE_TILE_W + col] = a.start[dd];
      if (d >= a.D) continue;
      for (int k = 0; k < a.nt; k++)
        t->c[((size_t)tl * np + (k >> 1)) * SCALE_TILE_W + col] |= (uint32_t)(uint16_t)a.c[(size_t)d * a.nt + k]
                                                                    << (16 * (k & 1));
    }
    const int dl = (tl + 1) * SCALE_TILE_W - 1 < a.D ? (tl + 1) * SCALE_TILE_W - 1 : a.D - 1;
    const int span = a.start[dl] + a.nt - a.start[tl * SCALE_TILE_W];
    if (span > t->span) t->span = span;
  }
}

// The vertical table.  A tile of SCALE_TILE_H output rows keeps its source rows y0 = start[first row of the
// tile] .. in LDS as pairs (rows y0 + 2q, y0 + 2q + 1 in one word); row e's taps begin at off = start[e] - y0,
// so its coefficients are stored from pair off >> 1 on, shifted by one when off is odd: np = ceil((nt + 1) / 2)
// words at c[e * np], the first pair in pair0[e].  rows = the most source rows a tile needs.
struct ScaleVTab {
  int np, rows;
  std::vector<int32_t> pair0;  // D
  std::vector<int32_t> y0;     // per tile: first source row, then the row count: 2 x tiles
  std::vector<uint32_t> c;
};
static inline void scale_vtab_build(const ScaleAxis &a, ScaleVTab *t) {
  const int tiles = (a.D + SCALE_TILE_H - 1) / SCALE_TILE_H, np = (a.nt + 2) / 2;
  t->np = np, t->rows = 0;
  t->pair0.assign((size_t)a.D, 0);
  t->y0.assign((size_t)2 * tiles, 0);
  t->c.assign((size_t)a.D * np, 0);
  for (int tl = 0; tl < tiles; tl++) {
    const int e0 = tl * SCALE_TILE_H, e1 = e0 + SCALE_TILE_H - 1 < a.D ? e0 + SCALE_TILE_H - 1 : a.D - 1;
    const int y0 = a.start[e0], rows = a.start[e1] + a.nt - y0;
    t->y0[2 * tl] = y0, t->y0[2 * tl + 1] = rows;
    if (rows > t->rows) t->rows = rows;
    for (int e = e0; e <= e1; e++) {
      const int off = a.start[e] - y0;
      t->pair0[e] = off >> 1;
      for (int k = 0; k < a.nt; k++) {
        const int j = k + (off & 1);
        t->c[(size_t)e * np + (j >> 1)] |= (uint32_t)(uint16_t)a.c[(size_t)e * a.nt + k] << (16 * (j & 1));
      }
    }
  }
}
