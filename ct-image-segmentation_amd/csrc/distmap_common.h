// What the distance-map kernels of the 2-D planes (distmap2d.hip) and of the volumes (distmap3d.hip) share: the modes, the sentinels,
// the check of the sides, the outward lower-envelope search with its three cell policies (uint16 rows, int32 squared cells, float32
// cells under voxel sizes) and the exact integer / correctly rounded roots of the value pass.
#pragma once
#include "ctseg_dev.h"

namespace ctseg {

enum { DM_REFERENCE = 0, DM_SIGNED = 1 };
constexpr int DM_MAX_SIDE = 1024;        // 3 * 1023^2 fits int32 (and float's 24 bits); a distance along one axis fits uint16 below the sentinel
constexpr uint32_t DM_NONE = 0xffffu;
constexpr int DM_INF = 0x7fffffff;
constexpr uint32_t DM_W_NONE = 0x7f800000u;   // +inf, the "none" of the float32 cells

// `count` volumes (or samples) with sides in 1..DM_MAX_SIDE
static inline int check_sides(const char* who, int count, int X, int Y, int Z) {
  CTSEG_REQUIRE(count >= 1 && X >= 1 && Y >= 1 && Z >= 1, "%s: count, X, Y, Z >= 1 (got %d of %d x %d x %d)", who, count, X, Y, Z);
  CTSEG_REQUIRE(X <= DM_MAX_SIDE && Y <= DM_MAX_SIDE && Z <= DM_MAX_SIDE, "%s: sides up to %d (got %d x %d x %d)", who, DM_MAX_SIDE, X,
                Y, Z);
  return 0;
}

// One float32 rounding each.  Device code is compiled with contraction on, and the toolchain's __fmul_rn / __fadd_rn are a plain
// `*` and `+` that may still fuse once inlined; the pragma takes the contraction flag off these two operations themselves, and a
// product or a sum without it is never made part of an FMA.
__device__ __forceinline__ float mul_rn(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}
__device__ __forceinline__ float add_rn(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}

// The outward lower-envelope search: min over t' of step(|t - t'|) + value(f[t']) on one LDS line of n cells, `stride` words apart,
// for the voxel at t.  It starts from the voxel's own cell and walks d = 1, 2, ... until the step alone reaches the best value or
// both neighbours have left the line.  A cell policy M says what a cell holds:
//   value(word)   what the cell contributes: 0 where its class differs from the voxel's, the stored number where it is equal, M's
//                 "none" where that says so
//   own(word)     value() of the voxel's own cell, whose class is equal by definition: the stored number, without the test
//   step(d)       the cost of offset d
//   add(s, v)     the candidate; "none" stays "none", and adding a non-negative value is monotone, which is what lets
//                 step(d) >= best end the search
template <class M>
__device__ __forceinline__ typename M::T envelope_min(const M& m, const typename M::Word* f, int t, int n, int stride) {
  typename M::T best = m.own(f[t * stride]);
  for (int d = 1; d < n; ++d) {
    const typename M::T dd = m.step(d);
    if (dd >= best) break;
    const int tl = t - d, tr = t + d;
    if (tl < 0 && tr >= n) break;
    if (tl >= 0) { const typename M::T c = m.add(dd, m.value(f[tl * stride])); best = c < best ? c : best; }
    if (tr < n) { const typename M::T c = m.add(dd, m.value(f[tr * stride])); best = c < best ? c : best; }
  }
  return best;
}

// DM_INF is the largest int: a candidate that stays "none" never replaces the best value
__device__ __forceinline__ int add_sat(int s, int v) { return v == DM_INF ? DM_INF : s + v; }

// The uint16 rows of the 2-D pass: the distance along the column to the class searched for (DM_NONE: none), squared on the fly.
struct CellsU16 {
  using Word = uint16_t;
  using T = int;
  __device__ __forceinline__ int value(uint32_t v) const { return v == DM_NONE ? DM_INF : (int)(v * v); }
  __device__ __forceinline__ int own(uint32_t v) const { return value(v); }
  __device__ __forceinline__ int step(int d) const { return d * d; }
  __device__ __forceinline__ int add(int s, int v) const { return add_sat(s, v); }
};

// The cells of the volumes, for a voxel of class `mine` (bit 31) looking for the other class.  An LDS word is class << 31 | f, f the
// int32 squared distance from that voxel to the other class found so far (DM_INF: none): a voxel of the other class itself counts 0.
struct CellsSq {
  using Word = uint32_t;
  using T = int;
  uint32_t mine;
  __device__ __forceinline__ int value(uint32_t v) const { return ((v ^ mine) >> 31) ? 0 : own(v); }
  __device__ __forceinline__ int own(uint32_t v) const { return (int)(v & 0x7fffffffu); }
  __device__ __forceinline__ int step(int d) const { return d * d; }
  __device__ __forceinline__ int add(int s, int v) const { return add_sat(s, v); }
};

// The same cells under a squared voxel size w, in float32: a word is class << 31 | the bits of f >= 0, the squared physical distance
// found so far (DM_W_NONE: none).  The candidate at offset d is fl(fl(w * d^2) + f), each a single rounding, and +inf stays +inf.
struct CellsW {
  using Word = uint32_t;
  using T = float;
  uint32_t mine;
  float w;
  __device__ __forceinline__ float value(uint32_t v) const { return ((v ^ mine) >> 31) ? 0.f : own(v); }
  __device__ __forceinline__ float own(uint32_t v) const { return __uint_as_float(v & 0x7fffffffu); }
  __device__ __forceinline__ float step(int d) const { return mul_rn(w, (float)(d * d)); }   // d^2 < 2^24: exact
  __device__ __forceinline__ float add(float s, float v) const { return add_rn(s, v); }
};

// floor(sqrt(v)) for 0 <= v < 2^24: the float root is only a first guess
__device__ __forceinline__ int isqrt(int v) {
  int r = (int)__fsqrt_rn((float)v);
  while (r * r > v) --r;
  while ((r + 1) * (r + 1) <= v) ++r;
  return r;
}

// sqrt(v) in float32, correctly rounded; a perfect square gives its integer root
__device__ __forceinline__ float root_f32(int v) {
  const int r = isqrt(v);
  return r * r == v ? (float)r : __fsqrt_rn((float)v);
}

}  // namespace ctseg
