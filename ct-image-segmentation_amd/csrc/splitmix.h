// The stateless noise of the augmentation kernels (warp2d.hip: displacement fields, deform3d.hip: control lattice): one splitmix64
// mix of seed + (counter + 1) * golden.  Each user builds its own counter and takes the top 53 bits as a uniform in [0, 1).
#pragma once
#include <cstdint>

namespace ctseg {

constexpr uint64_t SPLITMIX_GOLDEN = 0x9E3779B97F4A7C15ull;

__host__ __device__ __forceinline__ uint64_t splitmix64_mix(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// u = (z >> 11) * 2^-53 of the mixed counter
__host__ __device__ __forceinline__ double splitmix64_unit(uint64_t seed, uint64_t counter) {
  return (double)(splitmix64_mix(seed + (counter + 1ull) * SPLITMIX_GOLDEN) >> 11) * 0x1.0p-53;
}

}  // namespace ctseg
