// Building blocks shared by the weight-gradient kernels (conv_wgrad*.hip and the weight-gradient half of conv_stem.hip): the bias
// pseudo-tap operand and the geometry / row walk / slab order of the two split-K kernels.  (Packed taps, their predicates and
// tile_origin are in ctseg_dev.h: the forward kernels use them too.)
#pragma once
#include "ctseg_dev.h"

namespace ctseg {

// ---- the tap predicates of ctseg_dev.h on a weight-gradient descriptor -----------------------------------------------------------
static inline bool taps_within_unit_cube(const ctseg_wgrad_desc* d) { return taps_within(d->taps, d->ntaps, -1, 1); }
static inline bool taps_canonical_27(const ctseg_wgrad_desc* d) { return taps_canonical_27(d->taps, 1); }

// Gathered operand of the all-ones pseudo tap: 1.0 on channel row 0 for every voxel, so that row 0 of its product is the column sum
// of the other operand (the bias gradient).
__device__ __forceinline__ bf16x8 bias_ones_frag(int r16) {
  typedef __attribute__((ext_vector_type(8))) short s16x8;
  const short o = (r16 == 0) ? (short)0x3f80 : (short)0;
  return __builtin_bit_cast(bf16x8, s16x8{o, o, o, o, o, o, o, o});
}

// ---- split-K kernels (conv_wgrad_kernel, conv_wgrad_ring_kernel) -----------------------------------------------------------------
struct RadixStep { int sx, sy, sz; };      // a step of `rows` rows of the (Xr, Yr, Zr) row grid, z fastest, without carries
static inline RadixStep radix_step(int rows, int Zr, int Yr) { return {rows / Zr / Yr, (rows / Zr) % Yr, rows % Zr}; }

// What both kernels take by value (their argument structs derive from it)
struct WgradGeom {
  const char* in;
  const char* dy;
  float* ws;
  int N, Xi, Yi, Zi, Xr, Yr, Zr;
  int Cg, Cn, g_ld, d_ld, sin, ntaps;
  int rows, splits, rows_per_split;
  int kpad_w, cn_pad, d_valid;
  RadixStep step;                          // of the rows a thread's staging slot advances by: 32 (a stage) or 512 (a row-table chunk)
  int taps[CTSEG_MAX_TAPS];
};

// Everything but `step`, which the launcher sets with radix_step.  rows_per_split: checked by the entry point (32-row aligned, its
// row bytes within 32-bit offsets)
static inline void wgrad_geom_fill(WgradGeom& a, const ctseg_wgrad_desc* d, int rows_per_split) {
  a.in = (const char*)d->in; a.dy = (const char*)d->dy; a.ws = d->ws;
  a.N = d->N; a.Xi = d->Xi; a.Yi = d->Yi; a.Zi = d->Zi; a.Xr = d->Xr; a.Yr = d->Yr; a.Zr = d->Zr;
  a.Cg = d->Cg; a.Cn = d->Cn; a.g_ld = d->g_ld; a.d_ld = d->d_ld; a.sin = d->sin; a.ntaps = d->ntaps;
  a.rows = d->Xr * d->Yr * d->Zr; a.splits = d->splits; a.rows_per_split = rows_per_split;
  a.kpad_w = d->kpad_w; a.cn_pad = d->cn_pad;
  const int EPC = d->dtype == CTSEG_F32 ? 4 : 8, dv = ((d->Cn + EPC - 1) / EPC) * EPC;
  a.d_valid = dv < d->d_ld ? dv : d->d_ld;
  for (int i = 0; i < CTSEG_MAX_TAPS; ++i) a.taps[i] = i < d->ntaps ? d->taps[i] : 0;
}

// Workgroups go to the 8 XCDs round-robin by linear id.  With a (tile, slab) grid the tiles of one slab (the same rows of `in` and
// `dy`) land on different XCDs and each XCD's L2 fetches its own copy.  Flat grid: ids L, L + 8, L + 16, ... inside a group of
// 8 * tiles are the tiles of ONE slab -> same XCD, dispatched together, one fetch.  The launchers use it when this holds:
static inline bool slab_grid_is_flat(int zs, int tiles) { return zs % 8 == 0 && tiles > 1; }
struct SlabTile { int tile, zslab; };
__device__ __forceinline__ SlabTile slab_xcd_decode(int L, int tiles) {
  const int G = 8 * tiles, g = L / G, r = L - g * G;
  return {r >> 3, g * 8 + (r & 7)};
}

// A staging slot's voxel row as SCALED coordinates (x sin, y sin, z sin) of the gathered operand plus its 32-bit byte offset inside
// the sample; advance() moves all four by a uniform step of rows: constants plus two carry corrections, no multiplies or divisions.
struct RowStepK { int zrs, yrs, sin, sxs, sys, szs, o_step, o_cz, o_cy; };
__device__ __forceinline__ RowStepK row_step_k(const WgradGeom& P, int gl) {      // gl: bytes of a gathered voxel row
  const int szs = P.step.sz * P.sin, sys = P.step.sy * P.sin, sxs = P.step.sx * P.sin;
  return {P.Zr * P.sin, P.Yr * P.sin, P.sin, sxs, sys, szs, (szs + (sys + sxs * P.Yi) * P.Zi) * gl,
          P.sin * gl * (P.Zi - P.Zr), P.sin * gl * P.Zi * (P.Yi - P.Yr)};        // o_cz / o_cy: what a z carry / a y carry adds
}
struct RowWalk {
  int x, y, z, off;
  __device__ __forceinline__ void advance(const RowStepK& K) {
    z += K.szs;
    const bool carry_z = z >= K.zrs;
    z -= carry_z ? K.zrs : 0;
    y += K.sys + (carry_z ? K.sin : 0);
    const bool carry_y = y >= K.yrs;
    y -= carry_y ? K.yrs : 0;
    x += K.sxs + (carry_y ? K.sin : 0);
    off += K.o_step + (carry_z ? K.o_cz : 0) + (carry_y ? K.o_cy : 0);
  }
};

}  // namespace ctseg
