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

}  // namespace ctseg
