// What the distance-map kernels of the 2-D planes (distmap2d.hip) and of the volumes (distmap3d.hip) share: the modes, the sentinels,
// the outward lower-envelope searches and the exact integer / correctly rounded roots of the value pass.
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
