// What the distance-map kernels of the 2-D planes (distmap2d.hip) and of the volumes (distmap3d.hip) share: the modes, the sentinels,
// the outward lower-envelope searches (integer, and float32 under voxel sizes) and the exact integer / correctly rounded roots of
// the value pass.
#pragma once
#include "ctseg_dev.h"

namespace ctseg {

enum { DM_REFERENCE = 0, DM_SIGNED = 1 };
constexpr int DM_MAX_SIDE = 1024;        // 3 * 1023^2 fits int32 (and float's 24 bits); a distance along one axis fits uint16 below the sentinel
constexpr uint32_t DM_NONE = 0xffffu;
constexpr int DM_INF = 0x7fffffff;

// min over x' of (x - x')^2 + g[x']^2 on one LDS row; DM_INF when no column of the row holds a value
__device__ __forceinline__ int row_min(const uint16_t* g, int x, int W) {
  int best = DM_INF;
  const uint32_t g0 = g[x];
  if (g0 != DM_NONE) best = (int)(g0 * g0);
  for (int d = 1; d < W; ++d) {
    const int dd = d * d;
    if (dd >= best) break;
    const int xl = x - d, xr = x + d;
    if (xl < 0 && xr >= W) break;
    if (xl >= 0) {
      const uint32_t v = g[xl];
      if (v != DM_NONE) { const int c = dd + (int)(v * v); best = c < best ? c : best; }
    }
    if (xr < W) {
      const uint32_t v = g[xr];
      if (v != DM_NONE) { const int c = dd + (int)(v * v); best = c < best ? c : best; }
    }
  }
  return best;
}

// The same search on values that are squared already, for a voxel of class `mine` (bit 31) looking for the other class.  An LDS word
// is class << 31 | f, f the squared distance from that voxel to the other class found so far (DM_INF: none): a voxel of the other
// class itself counts 0.  t and n are in elements of the line, `stride` is the line's step in words.
__device__ __forceinline__ int line_min_sq(const uint32_t* f, int t, int n, int stride, uint32_t mine) {
  int best = (int)(f[t * stride] & 0x7fffffffu);               // its own word is of its own class
  for (int d = 1; d < n; ++d) {
    const int dd = d * d;
    if (dd >= best) break;
    const int tl = t - d, tr = t + d;
    if (tl < 0 && tr >= n) break;
    if (tl >= 0) {
      const uint32_t v = f[tl * stride];
      const int fv = ((v ^ mine) >> 31) ? 0 : (int)(v & 0x7fffffffu);
      if (fv != DM_INF) { const int c = dd + fv; best = c < best ? c : best; }
    }
    if (tr < n) {
      const uint32_t v = f[tr * stride];
      const int fv = ((v ^ mine) >> 31) ? 0 : (int)(v & 0x7fffffffu);
      if (fv != DM_INF) { const int c = dd + fv; best = c < best ? c : best; }
    }
  }
  return best;
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

// The weighted form of line_min_sq, on float32: a word is class << 31 | the bits of f >= 0, the squared physical distance found so
// far (DM_W_NONE, +inf: none).  Non-negative floats order like their bit patterns, so the layout is that of the integer search.
// The candidate at offset d is fl(fl(w * d^2) + f), each a single rounding (mul_rn, add_rn); adding a non-negative term is monotone
// in float arithmetic, so fl(w * d^2) >= best ends the search as d^2 >= best does there.
constexpr uint32_t DM_W_NONE = 0x7f800000u;
__device__ __forceinline__ float line_min_w(const uint32_t* f, int t, int n, int stride, uint32_t mine, float w) {
  float best = __uint_as_float(f[t * stride] & 0x7fffffffu);    // its own word is of its own class
  for (int d = 1; d < n; ++d) {
    const float dd = mul_rn(w, (float)(d * d));                  // d^2 < 2^24: exact
    if (dd >= best) break;
    const int tl = t - d, tr = t + d;
    if (tl < 0 && tr >= n) break;
    if (tl >= 0) {
      const uint32_t v = f[tl * stride];
      const float c = add_rn(dd, ((v ^ mine) >> 31) ? 0.f : __uint_as_float(v & 0x7fffffffu));   // (+inf stays +inf)
      best = c < best ? c : best;
    }
    if (tr < n) {
      const uint32_t v = f[tr * stride];
      const float c = add_rn(dd, ((v ^ mine) >> 31) ? 0.f : __uint_as_float(v & 0x7fffffffu));
      best = c < best ? c : best;
    }
  }
  return best;
}

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
