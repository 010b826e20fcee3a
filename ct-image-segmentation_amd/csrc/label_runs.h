// Label maps as runs of 16 voxels along Z, the innermost axis: what the passes over uint8 [B][X][Y][Z] maps share (surface_distance.hip,
// components.hip).  A lane owns one run; with Z a multiple of 16 a run is one 16-byte load, otherwise the same body moves bytes and
// the last run of a line is short.
#pragma once
#include "ctseg_dev.h"

namespace ctseg {

constexpr int SD_RUN = 16;               // voxels of a lane's run along Z, and bytes of the wide loads and stores
constexpr int SD_MAX_CLASSES = 16;
enum { SD_AXIS_X = 1, SD_AXIS_Y = 2, SD_AXIS_Z = 4 };

// byte i of a run held as four words; i is a constant after unrolling, so the run stays in registers
__device__ __forceinline__ uint32_t run_byte(const u32x4& w, int i) { return (w[i >> 2] >> ((i & 3) * 8)) & 255u; }

// n <= 16 bytes at p as four words; WIDE: n == 16 and p is 16-byte aligned
template <bool WIDE> __device__ __forceinline__ u32x4 load_run(const uint8_t* p, int n) {
  if constexpr (WIDE) {
    return *reinterpret_cast<const u32x4*>(p);
  } else {
    u32x4 w = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < SD_RUN; ++i)
      if (i < n) w[i >> 2] |= (uint32_t)p[i] << ((i & 3) * 8);
    return w;
  }
}

// the limits of one launch over label maps [B][X][Y][Z] with C classes, shared by the entries of components.hip and fill_holes.hip
static inline int check_components_dims(const char* who, int32_t B, int32_t X, int32_t Y, int32_t Z, int32_t C) {
  CTSEG_REQUIRE(B >= 1 && X >= 1 && Y >= 1 && Z >= 1, "%s: B, X, Y, Z >= 1 (got %d samples of %d x %d x %d)", who, B, X, Y, Z);
  CTSEG_REQUIRE(X <= 1024 && Y <= 1024 && Z <= 1024, "%s: sides up to 1024 (got %d x %d x %d)", who, X, Y, Z);
  CTSEG_REQUIRE((int64_t)B * X * Y * Z < ((int64_t)1 << 31) && B <= 65535,
                "%s: %d samples of %d x %d x %d are too many for one launch (fewer than 2^31 voxels, at most 65535 samples)", who, B, X,
                Y, Z);
  CTSEG_REQUIRE(C >= 2 && C <= SD_MAX_CLASSES, "%s: 2 <= C <= %d classes (got %d)", who, SD_MAX_CLASSES, C);
  return 0;
}

}  // namespace ctseg
