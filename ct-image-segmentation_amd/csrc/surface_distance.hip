// Surface metrics on gfx950: the percentile Hausdorff distance and the average surface distance between two label maps, in integers
// up to the last square root.  Three stages; the middle one is ctseg_distmap3d_batch, unchanged:
//   edges   ctseg_surface_edges: the surface voxels of every class of `pred` and of `target`, as P = 2 * B * (C - 1) mask volumes
//           [side][b][c][X][Y][Z] that the distance transform takes as they are, and their counts.  A voxel is on the surface of its
//           own class exactly when one of its neighbours along an active axis is missing or holds another label: one flag per voxel,
//           whatever the class.  A lane owns a run of 16 voxels along Z: its Z neighbours are in the run and its two border bytes,
//           its X and Y neighbours in four runs a line or a plane away.  With Z a multiple of 16 every run is one 16-byte load and
//           every class one 16-byte store; otherwise the same body moves bytes and the last run of a line is short.
//   select  ctseg_surface_select: row r = (side, b, c) pairs its own surface mask with d2_fg of the OTHER side's surface, the squared
//           distance of every voxel to that surface.  Exact order statistics by a two-level radix select over the 22-bit values
//           (3 * 1023^2 < 2^22): histogram d2 >> 11, locate the coarse buckets of the two ranks, histogram d2 & 2047 inside them,
//           pick.  Histograms are integer atomics (LDS, then one flush per workgroup): order independent.  The float64 sum of the
//           roots goes through per-workgroup partials in fixed slots, added in slot order.  The ranks lo = floor((n - 1) * q / 100)
//           and hi = min(lo + 1, n - 1) are computed on the device from the counts of the edge pass: no host synchronisation.
//           ctseg_surface_select_f32 is the same select on the float32 squared distances of ctseg_distmap3d_weighted (physical
//           units), three levels over the 31-bit patterns of the non-negative floats.
#include "distmap_common.h"
#include "label_runs.h"

namespace ctseg {

constexpr int SD_BINS = 2048;            // of either radix level: 11 + 11 bits
constexpr int SD_SHIFT = 11;
constexpr int SD_MAX_SLOTS = 64;         // workgroups (and float64 partials) per row of the select
constexpr int SD_CHUNK = 256 * SD_RUN;   // voxels one workgroup of the select takes per step

// Grid (ceil(lines * runs / 256), B, 2): side 0 = pred, 1 = target.  Lane: run k of line (x, y) of sample b.
template <bool WIDE>
__global__ __launch_bounds__(256) void surface_edges_kernel(const uint8_t* __restrict__ pred, const uint8_t* __restrict__ target, int B,
                                                            int X, int Y, int Z, int C, int axes, int runs, uint8_t* __restrict__ edges,
                                                            int32_t* __restrict__ counts) {
  __shared__ uint32_t s_cnt[SD_MAX_CLASSES];
  const int tid = threadIdx.x, b = blockIdx.y, side = blockIdx.z;
  if (tid < SD_MAX_CLASSES) s_cnt[tid] = 0u;
  __syncthreads();
  const int64_t plane = (int64_t)Y * Z, S = (int64_t)X * plane;
  const int64_t g = (int64_t)blockIdx.x * 256 + tid;
  const int64_t line = g / runs;
  if (line < (int64_t)X * Y) {
    const int z0 = (int)(g - line * runs) * SD_RUN;
    const int x = (int)(line / Y), y = (int)(line - (int64_t)x * Y);
    const int n = Z - z0 < SD_RUN ? Z - z0 : SD_RUN;
    const int64_t at = line * Z + z0;                               // of the run's first voxel in its volume
    const uint8_t* L = (side ? target : pred) + (int64_t)b * S + at;
    const u32x4 c = load_run<WIDE>(L, n);
    uint32_t edge = 0u;                                             // bit i: voxel i has a missing or different neighbour
    if (axes & SD_AXIS_Z) {
      const bool has_l = z0 > 0, has_r = z0 + n < Z;
      const uint32_t lb = has_l ? L[-1] : 0u, rb = has_r ? L[n] : 0u;
#pragma unroll
      for (int i = 0; i < SD_RUN; ++i) {
        const uint32_t v = run_byte(c, i);
        const bool l_same = i == 0 ? (has_l && lb == v) : run_byte(c, i > 0 ? i - 1 : 0) == v;
        const bool r_in = i + 1 < n;
        const bool r_same = r_in ? run_byte(c, i + 1 < SD_RUN ? i + 1 : i) == v : (has_r && rb == v);
        if (!(l_same && r_same)) edge |= 1u << i;
      }
    }
    if (axes & SD_AXIS_Y) {
      if (y == 0 || y == Y - 1) edge = 0xffffu;
      if (y > 0) {
        const u32x4 o = load_run<WIDE>(L - Z, n);
#pragma unroll
        for (int i = 0; i < SD_RUN; ++i) if (run_byte(o, i) != run_byte(c, i)) edge |= 1u << i;
      }
      if (y < Y - 1) {
        const u32x4 o = load_run<WIDE>(L + Z, n);
#pragma unroll
        for (int i = 0; i < SD_RUN; ++i) if (run_byte(o, i) != run_byte(c, i)) edge |= 1u << i;
      }
    }
    if (axes & SD_AXIS_X) {
      if (x == 0 || x == X - 1) edge = 0xffffu;
      if (x > 0) {
        const u32x4 o = load_run<WIDE>(L - plane, n);
#pragma unroll
        for (int i = 0; i < SD_RUN; ++i) if (run_byte(o, i) != run_byte(c, i)) edge |= 1u << i;
      }
      if (x < X - 1) {
        const u32x4 o = load_run<WIDE>(L + plane, n);
#pragma unroll
        for (int i = 0; i < SD_RUN; ++i) if (run_byte(o, i) != run_byte(c, i)) edge |= 1u << i;
      }
    }
    // the label where the voxel is on a surface, 0 elsewhere and past the end of a short run; a label >= C is in no class
    u32x4 el = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < SD_RUN; ++i) {
      const uint32_t v = run_byte(c, i);
      if (i < n && ((edge >> i) & 1u) && v >= 1u && v < (uint32_t)C) {
        el[i >> 2] |= v << ((i & 3) * 8);
        atomicAdd(&s_cnt[v], 1u);
      }
    }
    uint8_t* out = edges + ((int64_t)(side * B + b) * (C - 1)) * S + at;
    for (int k = 1; k < C; ++k, out += S) {
      u32x4 m;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        uint32_t w = 0u;
#pragma unroll
        for (int t = 0; t < 4; ++t) w |= (((el[j] >> (t * 8)) & 255u) == (uint32_t)k ? 1u : 0u) << (t * 8);
        m[j] = w;
      }
      if constexpr (WIDE) {
        *reinterpret_cast<u32x4*>(out) = m;
      } else {
#pragma unroll
        for (int i = 0; i < SD_RUN; ++i)
          if (i < n) out[i] = (uint8_t)run_byte(m, i);
      }
    }
  }
  __syncthreads();
  if (tid >= 1 && tid < C && s_cnt[tid]) atomicAdd(&counts[(int64_t)(side * B + b) * (C - 1) + tid - 1], (int32_t)s_cnt[tid]);
}

// ---- the select -------------------------------------------------------------------------------------------------------------
// Row r of 2 * half rows: its partner is the same (b, c) on the other side.  A row has values when both surfaces have voxels.
__device__ __forceinline__ int sd_partner(int r, int half) { return r < half ? r + half : r - half; }

struct SdRanks { int64_t lo, hi; double gamma; };
__device__ __forceinline__ SdRanks sd_ranks(int32_t n, double q) {
  const double r = (double)(n - 1) * (q / 100.0);
  int64_t lo = (int64_t)floor(r);
  lo = lo < 0 ? 0 : (lo > n - 1 ? n - 1 : lo);
  return {lo, lo + 1 < n ? lo + 1 : (int64_t)n - 1, r - (double)lo};
}

// f(d2) for every surface voxel of the row in [v0, v1) (v0 a multiple of SD_CHUNK): `mask` and `d2` point at the row's volume and
// at the partner's squared distances.  WIDE: S is a multiple of 16, so 16 mask bytes are one load, and most of them are all zero.
template <bool WIDE, class F>
__device__ __forceinline__ void sd_for_each(const uint8_t* __restrict__ mask, const int32_t* __restrict__ d2, int64_t v0, int64_t v1,
                                            F&& f) {
  for (int64_t v = v0 + (int64_t)threadIdx.x * SD_RUN; v < v1; v += SD_CHUNK) {
    const int n = v1 - v < SD_RUN ? (int)(v1 - v) : SD_RUN;
    const u32x4 m = load_run<WIDE>(mask + v, n);
    if ((m[0] | m[1] | m[2] | m[3]) == 0u) continue;
#pragma unroll
    for (int i = 0; i < SD_RUN; ++i)
      if (run_byte(m, i)) {                                          // (bytes past a short run are zero)
        const int d = d2[v + i];
        if (d >= 0) f(d);
      }
  }
}

// The coarse (or fine) bucket that holds rank k of a 2048-bin histogram `h`, and the number of values below the bucket: 256 lanes,
// 8 bins each, the sums of the lanes before it read from LDS.  Every lane returns the same pair.  k < the histogram's total.
__device__ __forceinline__ void sd_locate(const uint32_t* __restrict__ h, int64_t k0, int64_t k1, uint32_t* s_sum, int64_t* s_found,
                                          int& b0, int64_t& below0, int& b1, int64_t& below1) {
  const int tid = threadIdx.x;
  uint32_t mine[8];
  uint32_t tot = 0u;
#pragma unroll
  for (int j = 0; j < 8; ++j) { mine[j] = h[tid * 8 + j]; tot += mine[j]; }
  __syncthreads();                                                   // (s_sum and s_found may still be read from an earlier call)
  s_sum[tid] = tot;
  __syncthreads();
  int64_t before = 0;
  for (int t = 0; t < tid; ++t) before += s_sum[t];
#pragma unroll
  for (int w = 0; w < 2; ++w) {
    const int64_t k = w ? k1 : k0;
    if (k >= before && k < before + tot) {
      int64_t acc = before;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if (k >= acc && k < acc + mine[j]) { s_found[2 * w] = tid * 8 + j; s_found[2 * w + 1] = acc; }
        acc += mine[j];
      }
    }
  }
  __syncthreads();
  b0 = (int)s_found[0]; below0 = s_found[1];
  b1 = (int)s_found[2]; below1 = s_found[3];
}

__global__ __launch_bounds__(256) void surface_zero_kernel(uint32_t* __restrict__ p, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) p[i] = 0u;
}

// Grid (slots, rows).  Workgroup (w, r): voxels [w * per, w * per + per) of row r.
template <bool WIDE>
__global__ __launch_bounds__(256) void surface_coarse_kernel(const uint8_t* __restrict__ edges, const int32_t* __restrict__ d2,
                                                             const int32_t* __restrict__ counts, int half, int64_t S, int64_t per,
                                                             uint32_t* __restrict__ coarse, int32_t* __restrict__ vmax,
                                                             double* __restrict__ part) {
  __shared__ uint32_t s_h[SD_BINS];
  __shared__ double s_red[4];
  __shared__ int s_max;
  const int r = blockIdx.y, o = sd_partner(r, half), tid = threadIdx.x;
  if (counts[r] <= 0 || counts[o] <= 0) return;                      // (the whole workgroup)
  for (int i = tid; i < SD_BINS; i += 256) s_h[i] = 0u;
  if (tid == 0) s_max = 0;
  __syncthreads();
  const int64_t v0 = (int64_t)blockIdx.x * per, v1 = v0 + per < S ? v0 + per : S;
  double sum = 0.0;
  int mx = 0;
  sd_for_each<WIDE>(edges + (int64_t)r * S, d2 + (int64_t)o * S, v0, v1, [&](int d) {
    const int bin = d >> SD_SHIFT;
    atomicAdd(&s_h[bin < SD_BINS ? bin : SD_BINS - 1], 1u);
    mx = d > mx ? d : mx;
    sum += sqrt((double)d);
  });
  sum = wave_sum(sum);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { const int t = __shfl_xor(mx, off, 64); mx = t > mx ? t : mx; }
  if ((tid & 63) == 0) { s_red[tid >> 6] = sum; atomicMax(&s_max, mx); }
  __syncthreads();
  for (int i = tid; i < SD_BINS; i += 256)
    if (s_h[i]) atomicAdd(&coarse[(int64_t)r * SD_BINS + i], s_h[i]);
  if (tid == 0) {
    part[(int64_t)r * gridDim.x + blockIdx.x] = (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
    if (s_max) atomicMax(&vmax[r], s_max);
  }
}

template <bool WIDE>
__global__ __launch_bounds__(256) void surface_fine_kernel(const uint8_t* __restrict__ edges, const int32_t* __restrict__ d2,
                                                           const int32_t* __restrict__ counts, int half, int64_t S, int64_t per, double q,
                                                           const uint32_t* __restrict__ coarse, uint32_t* __restrict__ fine) {
  __shared__ uint32_t s_h[2 * SD_BINS];                             // of the bucket of lo, then of hi
  __shared__ uint32_t s_sum[256];
  __shared__ int64_t s_found[4];
  const int r = blockIdx.y, o = sd_partner(r, half), tid = threadIdx.x;
  const int32_t n = counts[r];
  if (n <= 0 || counts[o] <= 0) return;
  const SdRanks k = sd_ranks(n, q);
  for (int i = tid; i < 2 * SD_BINS; i += 256) s_h[i] = 0u;
  if (tid < 4) s_found[tid] = 0;
  int b0, b1;
  int64_t below0, below1;
  sd_locate(coarse + (int64_t)r * SD_BINS, k.lo, k.hi, s_sum, s_found, b0, below0, b1, below1);
  const int64_t v0 = (int64_t)blockIdx.x * per, v1 = v0 + per < S ? v0 + per : S;
  sd_for_each<WIDE>(edges + (int64_t)r * S, d2 + (int64_t)o * S, v0, v1, [&](int d) {
    const int bin = d >> SD_SHIFT, c = bin < SD_BINS ? bin : SD_BINS - 1;
    if (c == b0) atomicAdd(&s_h[d & (SD_BINS - 1)], 1u);
    if (c == b1) atomicAdd(&s_h[SD_BINS + (d & (SD_BINS - 1))], 1u);
  });
  __syncthreads();
  for (int i = tid; i < 2 * SD_BINS; i += 256)
    if (s_h[i]) atomicAdd(&fine[(int64_t)r * 2 * SD_BINS + i], s_h[i]);
}

// Grid (rows).  stats[r] = {d2[lo], d2[hi], max, 1} and fstats[r] = {sum of the roots, gamma}; {0, 0, 0, 0} and {0, 0} on a row
// without values.
__global__ __launch_bounds__(256) void surface_pick_kernel(const int32_t* __restrict__ counts, int half, int slots, double q,
                                                           const uint32_t* __restrict__ coarse, const uint32_t* __restrict__ fine,
                                                           const int32_t* __restrict__ vmax, const double* __restrict__ part,
                                                           int32_t* __restrict__ stats, double* __restrict__ fstats) {
  __shared__ uint32_t s_sum[256];
  __shared__ int64_t s_found[4];
  const int r = blockIdx.x, o = sd_partner(r, half), tid = threadIdx.x;
  const int32_t n = counts[r];
  if (n <= 0 || counts[o] <= 0) {
    if (tid < 4) stats[r * 4 + tid] = 0;
    if (tid < 2) fstats[r * 2 + tid] = 0.0;
    return;
  }
  const SdRanks k = sd_ranks(n, q);
  if (tid < 4) s_found[tid] = 0;
  int b0, b1, f0, f1, unused_b;
  int64_t below0, below1, unused;
  sd_locate(coarse + (int64_t)r * SD_BINS, k.lo, k.hi, s_sum, s_found, b0, below0, b1, below1);
  const uint32_t* fr = fine + (int64_t)r * 2 * SD_BINS;
  sd_locate(fr, k.lo - below0, k.lo - below0, s_sum, s_found, f0, unused, unused_b, unused);
  sd_locate(fr + SD_BINS, k.hi - below1, k.hi - below1, s_sum, s_found, f1, unused, unused_b, unused);
  if (tid == 0) {
    double sum = 0.0;
    for (int w = 0; w < slots; ++w) sum += part[(int64_t)r * slots + w];       // slot order: the same bits every run
    stats[r * 4 + 0] = (b0 << SD_SHIFT) | f0;
    stats[r * 4 + 1] = (b1 << SD_SHIFT) | f1;
    stats[r * 4 + 2] = vmax[r];
    stats[r * 4 + 3] = 1;
    fstats[r * 2 + 0] = sum;
    fstats[r * 2 + 1] = k.gamma;
  }
}

// ---- the select on float32 keys ----------------------------------------------------------------------------------------------
// The values are the non-negative float32 squared distances of ctseg_distmap3d_weighted (-1.0f: none, skipped by its sign like the
// integer -1).  Their 31-bit patterns order like the values, so the select runs on the patterns, in three levels of 11 + 11 + 9
// bits: `top` = bits >> 20, `mid` = (bits >> 9) & 2047 inside the top buckets of the two ranks, `low` = bits & 511 inside their
// mid buckets.  Every histogram has SD_BINS slots (the low ones use 512 of them), so sd_locate serves all three.
constexpr int SDF_TOP_SHIFT = 20, SDF_MID_SHIFT = 9, SDF_LOW_MASK = 511;

template <bool WIDE>
__global__ __launch_bounds__(256) void surface_top_f32_kernel(const uint8_t* __restrict__ edges, const int32_t* __restrict__ d2,
                                                              const int32_t* __restrict__ counts, int half, int64_t S, int64_t per,
                                                              uint32_t* __restrict__ top, int32_t* __restrict__ vmax,
                                                              double* __restrict__ part) {
  __shared__ uint32_t s_h[SD_BINS];
  __shared__ double s_red[4];
  __shared__ int s_max;
  const int r = blockIdx.y, o = sd_partner(r, half), tid = threadIdx.x;
  if (counts[r] <= 0 || counts[o] <= 0) return;                      // (the whole workgroup)
  for (int i = tid; i < SD_BINS; i += 256) s_h[i] = 0u;
  if (tid == 0) s_max = 0;
  __syncthreads();
  const int64_t v0 = (int64_t)blockIdx.x * per, v1 = v0 + per < S ? v0 + per : S;
  double sum = 0.0;
  int mx = 0;
  sd_for_each<WIDE>(edges + (int64_t)r * S, d2 + (int64_t)o * S, v0, v1, [&](int d) {   // d: the bits of a float >= 0
    atomicAdd(&s_h[d >> SDF_TOP_SHIFT], 1u);
    mx = d > mx ? d : mx;
    sum += sqrt((double)__int_as_float(d));
  });
  sum = wave_sum(sum);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { const int t = __shfl_xor(mx, off, 64); mx = t > mx ? t : mx; }
  if ((tid & 63) == 0) { s_red[tid >> 6] = sum; atomicMax(&s_max, mx); }
  __syncthreads();
  for (int i = tid; i < SD_BINS; i += 256)
    if (s_h[i]) atomicAdd(&top[(int64_t)r * SD_BINS + i], s_h[i]);
  if (tid == 0) {
    part[(int64_t)r * gridDim.x + blockIdx.x] = (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
    if (s_max) atomicMax(&vmax[r], s_max);
  }
}

// LEVEL 1: the mid histograms inside the top buckets of lo and hi; LEVEL 2: the low histograms inside their mid buckets.
// `lower` is [rows][2][SD_BINS] of the level being written, `mid` the finished mid histograms (LEVEL 2 only).
template <bool WIDE, int LEVEL>
__global__ __launch_bounds__(256) void surface_lower_f32_kernel(const uint8_t* __restrict__ edges, const int32_t* __restrict__ d2,
                                                                const int32_t* __restrict__ counts, int half, int64_t S, int64_t per,
                                                                double q, const uint32_t* __restrict__ top,
                                                                const uint32_t* __restrict__ mid, uint32_t* __restrict__ lower) {
  __shared__ uint32_t s_h[2 * SD_BINS];                             // of the bucket of lo, then of hi
  __shared__ uint32_t s_sum[256];
  __shared__ int64_t s_found[4];
  const int r = blockIdx.y, o = sd_partner(r, half), tid = threadIdx.x;
  const int32_t n = counts[r];
  if (n <= 0 || counts[o] <= 0) return;
  const SdRanks k = sd_ranks(n, q);
  for (int i = tid; i < 2 * SD_BINS; i += 256) s_h[i] = 0u;
  if (tid < 4) s_found[tid] = 0;
  int t0, t1, unused_b;
  int64_t below0, below1, unused;
  sd_locate(top + (int64_t)r * SD_BINS, k.lo, k.hi, s_sum, s_found, t0, below0, t1, below1);
  int p0 = t0, p1 = t1, shift = SDF_TOP_SHIFT, mask = SD_BINS - 1;   // the prefixes to match above `shift`, the bin below it
  if constexpr (LEVEL == 2) {
    const uint32_t* mr = mid + (int64_t)r * 2 * SD_BINS;
    int m0, m1;
    sd_locate(mr, k.lo - below0, k.lo - below0, s_sum, s_found, m0, unused, unused_b, unused);
    sd_locate(mr + SD_BINS, k.hi - below1, k.hi - below1, s_sum, s_found, m1, unused, unused_b, unused);
    p0 = (t0 << (SDF_TOP_SHIFT - SDF_MID_SHIFT)) | m0;
    p1 = (t1 << (SDF_TOP_SHIFT - SDF_MID_SHIFT)) | m1;
    shift = SDF_MID_SHIFT;
  }
  const int low_shift = LEVEL == 1 ? SDF_MID_SHIFT : 0;
  if constexpr (LEVEL == 2) mask = SDF_LOW_MASK;
  const int64_t v0 = (int64_t)blockIdx.x * per, v1 = v0 + per < S ? v0 + per : S;
  sd_for_each<WIDE>(edges + (int64_t)r * S, d2 + (int64_t)o * S, v0, v1, [&](int d) {
    const int p = d >> shift, bin = (d >> low_shift) & mask;
    if (p == p0) atomicAdd(&s_h[bin], 1u);
    if (p == p1) atomicAdd(&s_h[SD_BINS + bin], 1u);
  });
  __syncthreads();
  for (int i = tid; i < 2 * SD_BINS; i += 256)
    if (s_h[i]) atomicAdd(&lower[(int64_t)r * 2 * SD_BINS + i], s_h[i]);
}

// Grid (rows).  stats[r] = {bits of d2[lo], bits of d2[hi], bits of the maximum, 1}, fstats[r] as surface_pick_kernel.
__global__ __launch_bounds__(256) void surface_pick_f32_kernel(const int32_t* __restrict__ counts, int half, int slots, double q,
                                                               const uint32_t* __restrict__ top, const uint32_t* __restrict__ mid,
                                                               const uint32_t* __restrict__ low, const int32_t* __restrict__ vmax,
                                                               const double* __restrict__ part, int32_t* __restrict__ stats,
                                                               double* __restrict__ fstats) {
  __shared__ uint32_t s_sum[256];
  __shared__ int64_t s_found[4];
  const int r = blockIdx.x, o = sd_partner(r, half), tid = threadIdx.x;
  const int32_t n = counts[r];
  if (n <= 0 || counts[o] <= 0) {
    if (tid < 4) stats[r * 4 + tid] = 0;
    if (tid < 2) fstats[r * 2 + tid] = 0.0;
    return;
  }
  const SdRanks k = sd_ranks(n, q);
  if (tid < 4) s_found[tid] = 0;
  int t0, t1, m0, m1, l0, l1, unused_b;
  int64_t below0, below1, mbelow0, mbelow1, unused;
  sd_locate(top + (int64_t)r * SD_BINS, k.lo, k.hi, s_sum, s_found, t0, below0, t1, below1);
  const uint32_t* mr = mid + (int64_t)r * 2 * SD_BINS;
  const uint32_t* lr = low + (int64_t)r * 2 * SD_BINS;
  sd_locate(mr, k.lo - below0, k.lo - below0, s_sum, s_found, m0, mbelow0, unused_b, unused);
  sd_locate(mr + SD_BINS, k.hi - below1, k.hi - below1, s_sum, s_found, m1, mbelow1, unused_b, unused);
  sd_locate(lr, k.lo - below0 - mbelow0, k.lo - below0 - mbelow0, s_sum, s_found, l0, unused, unused_b, unused);
  sd_locate(lr + SD_BINS, k.hi - below1 - mbelow1, k.hi - below1 - mbelow1, s_sum, s_found, l1, unused, unused_b, unused);
  if (tid == 0) {
    double sum = 0.0;
    for (int w = 0; w < slots; ++w) sum += part[(int64_t)r * slots + w];       // slot order: the same bits every run
    stats[r * 4 + 0] = (t0 << SDF_TOP_SHIFT) | (m0 << SDF_MID_SHIFT) | l0;
    stats[r * 4 + 1] = (t1 << SDF_TOP_SHIFT) | (m1 << SDF_MID_SHIFT) | l1;
    stats[r * 4 + 2] = vmax[r];
    stats[r * 4 + 3] = 1;
    fstats[r * 2 + 0] = sum;
    fstats[r * 2 + 1] = k.gamma;
  }
}

// voxels per workgroup of the select (a multiple of SD_CHUNK) and the workgroups per row that follow from it, <= SD_MAX_SLOTS
static inline int64_t sd_per_slot(int64_t S) {
  const int64_t per = (S + SD_MAX_SLOTS - 1) / SD_MAX_SLOTS;
  return (per + SD_CHUNK - 1) / SD_CHUNK * SD_CHUNK;
}

// per row: SD_MAX_SLOTS float64 partials, the coarse and the two fine histograms, the maximum (+ pad)
static_assert(CTSEG_SURFACE_SELECT_ROW_BYTES == SD_MAX_SLOTS * 8 + 3 * SD_BINS * 4 + 8, "the header's workspace size");
// float32 keys: the top histogram and two each of the mid and low ones
static_assert(CTSEG_SURFACE_SELECT_F32_ROW_BYTES == SD_MAX_SLOTS * 8 + 5 * SD_BINS * 4 + 8, "the header's workspace size");

}  // namespace ctseg

using namespace ctseg;

static int check_surface_dims(const char* who, int32_t B, int32_t X, int32_t Y, int32_t Z, int32_t C) {
  CTSEG_REQUIRE(B >= 1 && X >= 1 && Y >= 1 && Z >= 1, "%s: B, X, Y, Z >= 1 (got %d samples of %d x %d x %d)", who, B, X, Y, Z);
  CTSEG_REQUIRE(X <= DM_MAX_SIDE && Y <= DM_MAX_SIDE && Z <= DM_MAX_SIDE, "%s: sides up to %d (got %d x %d x %d)", who, DM_MAX_SIDE, X,
                Y, Z);
  CTSEG_REQUIRE(C >= 2 && C <= SD_MAX_CLASSES, "%s: 2 <= C <= %d classes (got %d)", who, SD_MAX_CLASSES, C);
  CTSEG_REQUIRE((int64_t)2 * B * (C - 1) <= 65535, "%s: %d samples of %d classes are too many for one launch", who, B, C);
  return 0;
}

extern "C" int ctseg_surface_edges(const uint8_t* pred, const uint8_t* target, int32_t B, int32_t X, int32_t Y, int32_t Z, int32_t C,
                                   int32_t axes, uint8_t* edges, int32_t* counts, void* stream) {
  CTSEG_REQUIRE(pred && target && edges && counts, "surface_edges: null pointer (pred, target, edges and counts are required)");
  if (check_surface_dims("surface_edges", B, X, Y, Z, C)) return -1;
  CTSEG_REQUIRE(axes >= 1 && axes <= 7, "surface_edges: axes is a mask of X = 1, Y = 2, Z = 4 (got %d)", axes);
  CTSEG_REQUIRE(((uintptr_t)counts % 4) == 0, "surface_edges: unaligned pointer (counts)");
  const bool wide = Z % SD_RUN == 0;
  CTSEG_REQUIRE(!wide || (((uintptr_t)pred % 16) == 0 && ((uintptr_t)target % 16) == 0 && ((uintptr_t)edges % 16) == 0),
                "surface_edges: unaligned pointer (16 bytes for pred, target and edges when Z is a multiple of 16)");
  const int runs = (Z + SD_RUN - 1) / SD_RUN;
  const int64_t blocks = ((int64_t)X * Y * runs + 255) / 256;
  CTSEG_REQUIRE(blocks <= 0x7fffffff, "surface_edges: the volume is too large for one launch");
  const dim3 grid((unsigned)blocks, (unsigned)B, 2);
  hipStream_t st = (hipStream_t)stream;
  if (wide)
    hipLaunchKernelGGL(surface_edges_kernel<true>, grid, dim3(256), 0, st, pred, target, B, X, Y, Z, C, axes, runs, edges, counts);
  else
    hipLaunchKernelGGL(surface_edges_kernel<false>, grid, dim3(256), 0, st, pred, target, B, X, Y, Z, C, axes, runs, edges, counts);
  CTSEG_LAUNCH_CHECK("surface_edges");
  return 0;
}

extern "C" int ctseg_surface_select(const uint8_t* edges, const int32_t* d2, const int32_t* counts, int32_t B, int32_t X, int32_t Y,
                                    int32_t Z, int32_t C, double q, void* workspace, int64_t workspace_bytes, int32_t* stats,
                                    double* fstats, void* stream) {
  CTSEG_REQUIRE(edges && d2 && counts && workspace && stats && fstats,
                "surface_select: null pointer (edges, d2, counts, workspace, stats and fstats are required)");
  if (check_surface_dims("surface_select", B, X, Y, Z, C)) return -1;
  CTSEG_REQUIRE(q >= 0.0 && q <= 100.0, "surface_select: a percentile in [0, 100] (got %g)", q);
  const int64_t S = (int64_t)X * Y * Z, per = sd_per_slot(S);
  const int rows = 2 * B * (C - 1), slots = (int)((S + per - 1) / per);
  const int64_t need = (int64_t)rows * CTSEG_SURFACE_SELECT_ROW_BYTES;
  CTSEG_REQUIRE(workspace_bytes >= need, "surface_select: the workspace holds %lld bytes, %lld are needed", (long long)workspace_bytes,
                (long long)need);
  const bool wide = S % SD_RUN == 0;
  CTSEG_REQUIRE(((uintptr_t)workspace % 8) == 0 && ((uintptr_t)fstats % 8) == 0 && ((uintptr_t)stats % 4) == 0 &&
                    ((uintptr_t)counts % 4) == 0 && ((uintptr_t)d2 % 4) == 0 && (!wide || ((uintptr_t)edges % 16) == 0),
                "surface_select: unaligned pointer");
  double* part = (double*)workspace;                                 // [rows][slots <= 64], then the integer tables
  uint32_t* coarse = (uint32_t*)(part + (int64_t)rows * SD_MAX_SLOTS);   // [rows][2048]
  uint32_t* fine = coarse + (int64_t)rows * SD_BINS;                 // [rows][2][2048]
  int32_t* vmax = (int32_t*)(fine + (int64_t)rows * 2 * SD_BINS);    // [rows]
  const int64_t words = (int64_t)rows * (3 * SD_BINS + 1);
  const int half = B * (C - 1);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(surface_zero_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, st, coarse, words);
  CTSEG_LAUNCH_CHECK("surface_select (zero)");
  const dim3 grid((unsigned)slots, (unsigned)rows);
  if (wide) {
    hipLaunchKernelGGL(surface_coarse_kernel<true>, grid, dim3(256), 0, st, edges, d2, counts, half, S, per, coarse, vmax, part);
    CTSEG_LAUNCH_CHECK("surface_select (coarse)");
    hipLaunchKernelGGL(surface_fine_kernel<true>, grid, dim3(256), 0, st, edges, d2, counts, half, S, per, q,
                       (const uint32_t*)coarse, fine);
  } else {
    hipLaunchKernelGGL(surface_coarse_kernel<false>, grid, dim3(256), 0, st, edges, d2, counts, half, S, per, coarse, vmax, part);
    CTSEG_LAUNCH_CHECK("surface_select (coarse)");
    hipLaunchKernelGGL(surface_fine_kernel<false>, grid, dim3(256), 0, st, edges, d2, counts, half, S, per, q,
                       (const uint32_t*)coarse, fine);
  }
  CTSEG_LAUNCH_CHECK("surface_select (fine)");
  hipLaunchKernelGGL(surface_pick_kernel, dim3((unsigned)rows), dim3(256), 0, st, counts, half, slots, q, (const uint32_t*)coarse,
                     (const uint32_t*)fine, (const int32_t*)vmax, (const double*)part, stats, fstats);
  CTSEG_LAUNCH_CHECK("surface_select (pick)");
  return 0;
}

extern "C" int ctseg_surface_select_f32(const uint8_t* edges, const float* d2, const int32_t* counts, int32_t B, int32_t X, int32_t Y,
                                        int32_t Z, int32_t C, double q, void* workspace, int64_t workspace_bytes, int32_t* stats,
                                        double* fstats, void* stream) {
  CTSEG_REQUIRE(edges && d2 && counts && workspace && stats && fstats,
                "surface_select_f32: null pointer (edges, d2, counts, workspace, stats and fstats are required)");
  if (check_surface_dims("surface_select_f32", B, X, Y, Z, C)) return -1;
  CTSEG_REQUIRE(q >= 0.0 && q <= 100.0, "surface_select_f32: a percentile in [0, 100] (got %g)", q);
  const int64_t S = (int64_t)X * Y * Z, per = sd_per_slot(S);
  const int rows = 2 * B * (C - 1), slots = (int)((S + per - 1) / per);
  const int64_t need = (int64_t)rows * CTSEG_SURFACE_SELECT_F32_ROW_BYTES;
  CTSEG_REQUIRE(workspace_bytes >= need, "surface_select_f32: the workspace holds %lld bytes, %lld are needed",
                (long long)workspace_bytes, (long long)need);
  const bool wide = S % SD_RUN == 0;
  CTSEG_REQUIRE(((uintptr_t)workspace % 8) == 0 && ((uintptr_t)fstats % 8) == 0 && ((uintptr_t)stats % 4) == 0 &&
                    ((uintptr_t)counts % 4) == 0 && ((uintptr_t)d2 % 4) == 0 && (!wide || ((uintptr_t)edges % 16) == 0),
                "surface_select_f32: unaligned pointer");
  double* part = (double*)workspace;                                 // [rows][slots <= 64], then the integer tables
  uint32_t* top = (uint32_t*)(part + (int64_t)rows * SD_MAX_SLOTS);  // [rows][2048]
  uint32_t* mid = top + (int64_t)rows * SD_BINS;                     // [rows][2][2048]
  uint32_t* low = mid + (int64_t)rows * 2 * SD_BINS;                 // [rows][2][2048], 512 of each in use
  int32_t* vmax = (int32_t*)(low + (int64_t)rows * 2 * SD_BINS);     // [rows]
  const int64_t words = (int64_t)rows * (5 * SD_BINS + 1);
  const int half = B * (C - 1);
  const int32_t* bits = (const int32_t*)d2;                          // a float >= 0 orders like its bits; -1.0f is negative either way
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(surface_zero_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, st, top, words);
  CTSEG_LAUNCH_CHECK("surface_select_f32 (zero)");
  const dim3 grid((unsigned)slots, (unsigned)rows);
  if (wide) {
    hipLaunchKernelGGL(surface_top_f32_kernel<true>, grid, dim3(256), 0, st, edges, bits, counts, half, S, per, top, vmax, part);
    CTSEG_LAUNCH_CHECK("surface_select_f32 (top)");
    hipLaunchKernelGGL((surface_lower_f32_kernel<true, 1>), grid, dim3(256), 0, st, edges, bits, counts, half, S, per, q,
                       (const uint32_t*)top, (const uint32_t*)mid, mid);
    CTSEG_LAUNCH_CHECK("surface_select_f32 (mid)");
    hipLaunchKernelGGL((surface_lower_f32_kernel<true, 2>), grid, dim3(256), 0, st, edges, bits, counts, half, S, per, q,
                       (const uint32_t*)top, (const uint32_t*)mid, low);
  } else {
    hipLaunchKernelGGL(surface_top_f32_kernel<false>, grid, dim3(256), 0, st, edges, bits, counts, half, S, per, top, vmax, part);
    CTSEG_LAUNCH_CHECK("surface_select_f32 (top)");
    hipLaunchKernelGGL((surface_lower_f32_kernel<false, 1>), grid, dim3(256), 0, st, edges, bits, counts, half, S, per, q,
                       (const uint32_t*)top, (const uint32_t*)mid, mid);
    CTSEG_LAUNCH_CHECK("surface_select_f32 (mid)");
    hipLaunchKernelGGL((surface_lower_f32_kernel<false, 2>), grid, dim3(256), 0, st, edges, bits, counts, half, S, per, q,
                       (const uint32_t*)top, (const uint32_t*)mid, low);
  }
  CTSEG_LAUNCH_CHECK("surface_select_f32 (low)");
  hipLaunchKernelGGL(surface_pick_f32_kernel, dim3((unsigned)rows), dim3(256), 0, st, counts, half, slots, q, (const uint32_t*)top,
                     (const uint32_t*)mid, (const uint32_t*)low, (const int32_t*)vmax, (const double*)part, stats, fstats);
  CTSEG_LAUNCH_CHECK("surface_select_f32 (pick)");
  return 0;
}
