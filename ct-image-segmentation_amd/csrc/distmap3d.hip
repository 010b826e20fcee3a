// Distance maps of the 3-D pipeline on gfx950: capstone/data/utils.py:10-26 (compute_distance_map, rank-agnostic in the reference)
// for P volumes [X][Y][Z] of mask bytes, Z innermost: the (K, H, W, D) storage of ctseg_resize3d_to_hwd.
// The exact Euclidean distance transform in its separable form, in integers throughout, three launches:
//   sweep   along X.  One lane per line (y, z) walks down and then up; neighbouring lanes hold neighbouring (y, z), which are
//           contiguous in memory, so every load and store of both sweeps is coalesced.  (A sweep along Z would stride by a line
//           per lane.)
//   lines   lower envelope along Z, the contiguous axis: a workgroup stages a run of whole Z lines in LDS, squared.
//   slabs   lower envelope along Y and the map value: a workgroup stages the slab Y x ztile of one x, so its global loads and
//           stores stay contiguous along Z, and searches along Y with the slab's row length as the step.
// A voxel is foreground or background, and its squared distance to its own class is 0.  So every pass keeps ONE number per voxel,
// the distance to the OTHER class, beside the class bit; every voxel runs one search per pass, not two; and the workspace is
//   sweep: uint16  class << 15 | distance along X (DM3_NONE: the line has no voxel of the other class)
//   lines: uint32  class << 31 | squared distance within the voxel's (X, Z) plane (DM_INF: the plane has none)
// A search sees "class differs: 0, class equal: the stored number".  "None" survives a pass exactly when the whole line holds
// none, so after the last pass it means that the volume has no voxel of the other class: -1 in that d2 output and a map of 0,
// decided per voxel, with no flag shared between lanes.
// The value pass is that of distmap2d.hip: REFERENCE gives table[k] of the byte the reference stores, SIGNED the float map.
// The line and slab kernels are written once over a metric, and the search once over its cells (envelope_min, distmap_common.h).
// ctseg_distmap3d_batch runs them with MetricSq, as described above.  ctseg_distmap3d_weighted runs them with MetricW, the same
// transform under per-volume voxel sizes: squared physical distances in float32, the class bit in the float's sign bit, +inf for
// "none", and no value pass.
#include "distmap_common.h"

namespace ctseg {

constexpr uint32_t DM3_NONE = 0x7fffu;   // of the sweep's 15-bit distance (a side is at most DM_MAX_SIDE = 1024)
constexpr int DM3_LINE_WORDS = 4096;     // LDS words of the line pass: 16 KiB, whole Z lines back to back (at least one: Z <= 1024)
constexpr int DM3_SLAB_WORDS = 8192;     // LDS words of the slab pass: 32 KiB = Y x ztile, ztile a power of two in 8..64 (Y <= 1024)
constexpr int DM3_ZTILE_MIN = 8, DM3_ZTILE_MAX = 64;

// Lane: line (y, z) of volume p; `plane` = Y * Z voxels.
__global__ __launch_bounds__(256) void distmap3d_sweep_kernel(const uint8_t* __restrict__ masks, int64_t lines, int X, int64_t plane,
                                                              uint16_t* __restrict__ ws) {
  const int64_t line = (int64_t)blockIdx.x * 256 + threadIdx.x;     // the lines of all volumes, back to back
  if (line >= lines) return;
  const int64_t p = line / plane, yz = line - p * plane;
  const int64_t base = p * X * plane + yz;
  const uint8_t* m = masks + base;
  uint16_t* g = ws + base;
  int last_fg = -1, last_bg = -1;        // x of the nearest one below, -1: none yet
#pragma unroll 8
  for (int x = 0; x < X; ++x) {
    const bool fg = m[(int64_t)x * plane] != 0;
    if (fg) last_fg = x; else last_bg = x;
    const int other = fg ? last_bg : last_fg;
    const uint32_t d = other < 0 ? DM3_NONE : (uint32_t)(x - other);
    g[(int64_t)x * plane] = (uint16_t)((fg ? 0x8000u : 0u) | d);
  }
  int next_fg = -1, next_bg = -1;
#pragma unroll 8
  for (int x = X - 1; x >= 0; --x) {
    const uint32_t v = g[(int64_t)x * plane];
    const bool fg = (v & 0x8000u) != 0;
    if (fg) next_fg = x; else next_bg = x;
    const int other = fg ? next_bg : next_fg;
    const uint32_t u = other < 0 ? DM3_NONE : (uint32_t)(other - x);
    const uint32_t d = v & 0x7fffu;
    g[(int64_t)x * plane] = (uint16_t)((v & 0x8000u) | (u < d ? u : d));    // the sentinel is the largest value
  }
}

// ---- the two metrics ---------------------------------------------------------------------------------------------------------
// A metric names its cells (distmap_common.h), turns the sweep's squared distance along X into the first of them and writes what the
// last pass found.  MetricSq: squared voxel distances in int32, and the value pass.  MetricW: squared physical distances in float32
// under w[p] = {wx, wy, wz}, the squared voxel sizes of volume p, on the device.  The line pass turns dx into fl(wx * dx^2) and
// searches along Z with wz, the slab pass searches along Y with wy: fl(fl(wy dy^2) + fl(fl(wz dz^2) + fl(wx dx^2))) minimised over
// the candidates, because every pass applies a monotone map to the minimum of the pass before.  It has no value pass.
struct MetricSq {
  static constexpr bool WEIGHTED = false;
  static constexpr uint32_t NONE = (uint32_t)DM_INF;
  using D2 = int32_t;
  static __device__ __forceinline__ CellsSq cells(uint32_t mine, float) { return {mine}; }
  static __device__ __forceinline__ uint32_t first_cell(uint32_t dd, float) { return dd; }
  static __device__ __forceinline__ void store(int64_t at, bool inside, int d2, int mode, const float* __restrict__ table,
                                               float* __restrict__ map, int32_t* __restrict__ d2_fg, int32_t* __restrict__ d2_bg) {
    const bool none = d2 == DM_INF;                            // the volume has no voxel of the other class
    if (d2_fg) d2_fg[at] = inside ? 0 : (none ? -1 : d2);
    if (d2_bg) d2_bg[at] = inside ? (none ? -1 : d2) : 0;
    float val = 0.f;
    if (!none) {
      if (mode == DM_REFERENCE) {
        const int k = inside ? (1 - isqrt(d2)) & 255 : isqrt(d2) & 255;
        val = table[k];
      } else {
        val = inside ? __fdiv_rn(-(root_f32(d2) - 1.f), 255.f) : __fdiv_rn(root_f32(d2), 255.f);
      }
    }
    map[at] = val;
  }
};

struct MetricW {
  static constexpr bool WEIGHTED = true;
  static constexpr uint32_t NONE = DM_W_NONE;
  using D2 = float;
  static __device__ __forceinline__ CellsW cells(uint32_t mine, float w) { return {mine, w}; }
  static __device__ __forceinline__ uint32_t first_cell(uint32_t dd, float wx) { return __float_as_uint(mul_rn(wx, (float)dd)); }
  static __device__ __forceinline__ void store(int64_t at, bool inside, float d2, int, const float*, float*,   // (no value pass)
                                               float* __restrict__ d2_fg, float* __restrict__ d2_bg) {
    const float val = __float_as_uint(d2) == DM_W_NONE ? -1.f : d2;   // +inf: the volume has no voxel of the other class
    if (d2_fg) d2_fg[at] = inside ? 0.f : val;
    if (d2_bg) d2_bg[at] = inside ? val : 0.f;
  }
};

// Workgroup b: the Z lines [b * L, b * L + L) of all volumes, L * Z <= DM3_LINE_WORDS voxels that are contiguous in memory.  Under
// MetricW the lines may belong to two or more volumes, so each line looks its volume up, XY = X * Y; MetricSq has no such lookup.
template <class M>
__global__ __launch_bounds__(256) void distmap3d_lines_kernel(const uint16_t* __restrict__ g, int64_t voxels, int Z, int L, int XY,
                                                              const float* __restrict__ w, uint32_t* __restrict__ f) {
  __shared__ uint32_t s[DM3_LINE_WORDS];
  const int64_t line0 = (int64_t)blockIdx.x * L, e0 = line0 * Z;
  const int n = voxels - e0 < (int64_t)L * Z ? (int)(voxels - e0) : L * Z;   // whole lines: voxels is a multiple of Z
  const int tid = threadIdx.x;
  int64_t p0 = 0;
  int rem0 = 0;
  if constexpr (M::WEIGHTED) { p0 = line0 / XY; rem0 = (int)(line0 - p0 * XY); }
  const auto weight = [&](int r, int axis) -> float {          // of the volume of the workgroup's line r
    if constexpr (M::WEIGHTED) return w[(p0 + (rem0 + r) / XY) * 3 + axis];
    else return 0.f;
  };
  for (int i = tid; i < n; i += 256) {
    const float wx = weight(i / Z, 0);
    const uint32_t v = g[e0 + i], d = v & 0x7fffu;
    s[i] = ((v & 0x8000u) << 16) | (d == DM3_NONE ? M::NONE : M::first_cell(d * d, wx));
  }
  __syncthreads();
  for (int i = tid; i < n; i += 256) {
    const int r = i / Z, z = i - r * Z;
    const uint32_t mine = s[i] & 0x80000000u;
    f[e0 + i] = mine | __builtin_bit_cast(uint32_t, envelope_min(M::cells(mine, weight(r, 2)), s + r * Z, z, Z, 1));
  }
}

// Workgroup (b, t): row b = p * X + x of Y lines, columns [t * ZT, t * ZT + ZT) of Z; ZT = 1 << zshift, Y * ZT <= DM3_SLAB_WORDS.
// The row belongs to volume b / X.
template <class M>
__global__ __launch_bounds__(256) void distmap3d_slabs_kernel(const uint32_t* __restrict__ f, int X, int Y, int Z, int zshift, int ztiles,
                                                              const float* __restrict__ w, int mode, const float* __restrict__ table,
                                                              float* __restrict__ map, typename M::D2* __restrict__ d2_fg,
                                                              typename M::D2* __restrict__ d2_bg) {
  __shared__ uint32_t s[DM3_SLAB_WORDS];
  const int ZT = 1 << zshift;
  const int64_t b = blockIdx.x / ztiles;
  const int z0 = (int)(blockIdx.x - b * ztiles) << zshift;
  const int zn = Z - z0 < ZT ? Z - z0 : ZT;
  const int64_t base = b * Y * Z + z0;
  float wy = 0.f;
  if constexpr (M::WEIGHTED) wy = w[(b / X) * 3 + 1];
  const int n = Y << zshift;
  const int tid = threadIdx.x;
  for (int i = tid; i < n; i += 256) {
    const int y = i >> zshift, zc = i & (ZT - 1);
    if (zc < zn) s[i] = f[base + (int64_t)y * Z + zc];
  }
  __syncthreads();
  for (int i = tid; i < n; i += 256) {
    const int y = i >> zshift, zc = i & (ZT - 1);
    if (zc >= zn) continue;
    const uint32_t mine = s[i] & 0x80000000u;
    const auto d2 = envelope_min(M::cells(mine, wy), s + zc, y, Y, ZT);   // to the other class
    M::store(base + (int64_t)y * Z + zc, mine != 0, d2, mode, table, map, d2_fg, d2_bg);
  }
}

// the launch geometry both transforms share: Z lines per workgroup of the line pass, the slab tile, the three grids
struct Dm3Grid { int L, zshift, ztiles; int64_t sweep_blocks, line_blocks, slab_blocks; };
static inline Dm3Grid dm3_grid(int P, int X, int Y, int Z) {
  Dm3Grid g;
  g.L = DM3_LINE_WORDS / Z;                                    // >= 4
  g.zshift = 3;                                                // the widest slab tile that fits and that Z can fill
  while ((2 << g.zshift) <= DM3_ZTILE_MAX && ((int64_t)Y << (g.zshift + 1)) <= DM3_SLAB_WORDS && (1 << g.zshift) < Z) ++g.zshift;
  g.ztiles = (Z + (1 << g.zshift) - 1) >> g.zshift;
  g.sweep_blocks = ((int64_t)P * Y * Z + 255) / 256;
  g.line_blocks = ((int64_t)P * X * Y + g.L - 1) / g.L;
  g.slab_blocks = (int64_t)P * X * g.ztiles;
  return g;
}

// What the two entry points share: the checks that do not depend on the metric, and the three launches.
template <class M>
static int distmap3d_impl(const char* who, const uint8_t* masks, int P, int X, int Y, int Z, const float* w, void* workspace,
                          int64_t workspace_bytes, int mode, const float* table, float* map, typename M::D2* d2_fg,
                          typename M::D2* d2_bg, void* stream) {
  if (check_sides(who, P, X, Y, Z)) return -1;
  const int64_t plane = (int64_t)Y * Z, voxels = (int64_t)P * X * plane;
  CTSEG_REQUIRE(workspace_bytes >= 6 * voxels, "%s: the workspace holds %lld bytes, %lld are needed", who, (long long)workspace_bytes,
                (long long)(6 * voxels));
  CTSEG_REQUIRE(((uintptr_t)workspace % 4) == 0 && ((uintptr_t)w % 4) == 0 && ((uintptr_t)table % 4) == 0 && ((uintptr_t)map % 4) == 0 &&
                    ((uintptr_t)d2_fg % 4) == 0 && ((uintptr_t)d2_bg % 4) == 0,
                "%s: unaligned pointer", who);
  const Dm3Grid gr = dm3_grid(P, X, Y, Z);
  CTSEG_REQUIRE(gr.sweep_blocks <= 0x7fffffff && gr.line_blocks <= 0x7fffffff && gr.slab_blocks <= 0x7fffffff,
                "%s: %d volumes are too many for one launch", who, P);
  uint32_t* f = (uint32_t*)workspace;                          // [voxels] uint32, then [voxels] uint16
  uint16_t* g = (uint16_t*)(f + voxels);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(distmap3d_sweep_kernel, dim3((unsigned)gr.sweep_blocks), dim3(256), 0, st, masks, (int64_t)P * plane, X, plane, g);
  CTSEG_LAUNCH_CHECK_PASS(who, "sweep");
  hipLaunchKernelGGL(distmap3d_lines_kernel<M>, dim3((unsigned)gr.line_blocks), dim3(256), 0, st, (const uint16_t*)g, voxels, Z, gr.L,
                     X * Y, w, f);
  CTSEG_LAUNCH_CHECK_PASS(who, "lines");
  hipLaunchKernelGGL(distmap3d_slabs_kernel<M>, dim3((unsigned)gr.slab_blocks), dim3(256), 0, st, (const uint32_t*)f, X, Y, Z, gr.zshift,
                     gr.ztiles, w, mode, table, map, d2_fg, d2_bg);
  CTSEG_LAUNCH_CHECK_PASS(who, "slabs");
  return 0;
}

}  // namespace ctseg

using namespace ctseg;

extern "C" int ctseg_distmap3d_batch(const uint8_t* masks, int32_t P, int32_t X, int32_t Y, int32_t Z, int32_t mode, const float* table,
                                     void* workspace, int64_t workspace_bytes, float* out, int32_t* d2_fg, int32_t* d2_bg,
                                     void* stream) {
  CTSEG_REQUIRE(masks && table && workspace && out, "distmap3d_batch: null pointer (masks, table, workspace and out are required)");
  CTSEG_REQUIRE(mode == DM_REFERENCE || mode == DM_SIGNED, "distmap3d_batch: mode %d", mode);
  return distmap3d_impl<MetricSq>("distmap3d_batch", masks, P, X, Y, Z, nullptr, workspace, workspace_bytes, mode, table, out, d2_fg,
                                  d2_bg, stream);
}

extern "C" int ctseg_distmap3d_weighted(const uint8_t* masks, int32_t P, int32_t X, int32_t Y, int32_t Z, const float* w, void* workspace,
                                        int64_t workspace_bytes, float* d2_fg, float* d2_bg, void* stream) {
  CTSEG_REQUIRE(masks && w && workspace && (d2_fg || d2_bg),
                "distmap3d_weighted: null pointer (masks, w, workspace and one of d2_fg, d2_bg are required)");
  return distmap3d_impl<MetricW>("distmap3d_weighted", masks, P, X, Y, Z, w, workspace, workspace_bytes, 0, nullptr, nullptr, d2_fg,
                                 d2_bg, stream);   // (no mode, table or map: no value pass)
}
