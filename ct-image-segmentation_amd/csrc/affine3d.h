// The affine view of the 3-D resample passes, shared by the augmentation tile (resample3d_tile.h) and the test-time-augmentation
// merge (tta3d.hip): a 3 x 4 matrix in the kernel's arguments sends a voxel of the grid a kernel writes to the point it samples;
// a mask / class permutation travels beside it, 4 bits per entry.  The host half checks both, the device half evaluates the matrix
// and has the cores of the nearest and trilinear rules.  Every float operation is one float32 rounding: nothing may be contracted
// into an FMA, here or in an including file.
#pragma once
#pragma clang fp contract(off)
#include <cmath>

#include "ctseg_dev.h"

namespace ctseg {

struct Affine3d {
  float a[12];                       // row-major 3 x 4, rows and columns ordered d, h, w (read with constant indices only)
};

// finite entries, and coordinates that stay far inside float32 over the whole grid of `extent` voxels per axis (`what` names that
// grid in the message): no inf - inf in the kernel
inline int affine3d_check(const char* who, const float* matrix, const int extent[3], const char* what, Affine3d& m) {
  for (int a = 0; a < 3; ++a) {
    double reach = 0.0;
    for (int j = 0; j < 4; ++j) {
      const float v = matrix[a * 4 + j];
      CTSEG_REQUIRE(std::isfinite(v), "%s: matrix entry [%d][%d] is not finite", who, a, j);
      reach += fabs((double)v) * (j < 3 ? (double)(extent[j] - 1) : 1.0);
      m.a[a * 4 + j] = v;
    }
    CTSEG_REQUIRE(reach < 1e30, "%s: matrix row %d sends the %s beyond 1e30", who, a, what);
  }
  return 0;
}

// src[0..n) (`name` in the message; a null pointer is the identity) is a permutation of 0..n-1, n <= 16 -> 4 bits per entry
inline int pack_permutation(const char* who, const char* name, const int32_t* src, int n, unsigned long long& packed, bool& identity) {
  packed = 0, identity = true;
  unsigned seen = 0;
  for (int k = 0; k < n; ++k) {
    const int s = src ? src[k] : k;
    CTSEG_REQUIRE(s >= 0 && s < n && !((seen >> s) & 1u), "%s: %s is not a permutation of 0..%d (entry %d = %d)", who, name, n - 1, k, s);
    seen |= 1u << s;
    packed |= (unsigned long long)s << (4 * k);
    identity = identity && s == k;
  }
  return 0;
}

// the point that voxel (fd, fh, fw) samples
__device__ __forceinline__ void affine3d_point(const Affine3d& m, float fd, float fh, float fw, float& qd, float& qh, float& qw) {
  qd = ((m.a[0] * fd + m.a[1] * fh) + m.a[2] * fw) + m.a[3];
  qh = ((m.a[4] * fd + m.a[5] * fh) + m.a[6] * fw) + m.a[7];
  qw = ((m.a[8] * fd + m.a[9] * fh) + m.a[10] * fw) + m.a[11];
}

// a whole float g -> index, clamped into [-1, n] before the conversion so that no float outside the int range is converted
__device__ __forceinline__ int affine3d_index(float g, int n) { return (int)fminf(fmaxf(g, -1.f), (float)n); }
// the nearest rule: the whole coordinate nearest to q, and its index in [-1, n]
__device__ __forceinline__ float affine3d_whole(float q) { return floorf(q + 0.5f); }
__device__ __forceinline__ int affine3d_nearest(float q, int n) { return affine3d_index(affine3d_whole(q), n); }
// the base b = floorf(q) of the two trilinear corners, clamped into [-2, n]: b + 1 stays a small whole number on the outside it belongs to
__device__ __forceinline__ float affine3d_corner(float b, int n) { return fminf(fmaxf(b, -2.f), (float)n); }

__device__ __forceinline__ float affine3d_lerp(float x, float y, float t) { return x + t * (y - x); }

}  // namespace ctseg
