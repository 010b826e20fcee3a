// Surface metrics on gfx950: the percentile Hausdorff distance and the average surface distance between two label maps, in integers
// up to the last square root.  Three stages; the middle one is ctseg_distmap3d_batch, unchanged:
//   edges   ctseg_surface_edges: the surface voxels of every class of `pred` and of `target`, as P = 2 * B * (C - 1) mask volumes
//           [side][b][c][X][Y][Z] that the distance transform takes as they are, and their counts.  A voxel is on the surface of its
//           own class exactly when one of its neighbours along an active axis is missing or holds another label: one flag per voxel,
//           whatever the class.  A lane owns a run of 16 voxels along Z: its Z neighbours are in the run and its two border bytes,
//           its X and Y neighbours in four runs a line or a plane away.  With Z a multiple of 16 every run is one 16-byte load and
//           every class one 16-byte store; otherwise the same body moves bytes and the last run of a line is short.
//   select  ctseg_surface_select: row r = (side, b, c) pairs its own surface mask with d2_fg of the OTHER side's surface, the squared
//           distance of every voxel to that surface.  Exact order statistics by a radix select, written once over a key layout
//           (KeysI32, KeysF32 below): histogram the keys' first digit, locate the bins of the two ranks, histogram the next digit
//           inside them, and so on down the levels; pick.  The 22-bit integer values (3 * 1023^2 < 2^22) take two levels of 11 bits.
//           Histograms are integer atomics (LDS, then one flush per workgroup): order independent.  The float64 sum of the
//           roots goes through per-workgroup partials in fixed slots, added in slot order.  The ranks lo = floor((n - 1) * q / 100)
//           and hi = min(lo + 1, n - 1) are computed on the device from the counts of the edge pass: no host synchronisation.
//           ctseg_surface_select_f32 is the same select on the float32 squared distances of ctseg_distmap3d_weighted (physical
//           units), three levels over the 31-bit patterns of the non-negative floats.
#include <type_traits>

#include "distmap_common.h"
#include "label_runs.h"

namespace ctseg {

constexpr int SD_BINS = 2048;            // slots of every histogram of the select: a digit has 11 bits at the most
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
    const auto differs = [&](const uint8_t* other) {                // bit i: voxel i of the neighbouring run at `other` holds another label
      const u32x4 o = load_run<WIDE>(other, n);
      uint32_t m = 0u;
#pragma unroll
      for (int i = 0; i < SD_RUN; ++i) if (run_byte(o, i) != run_byte(c, i)) m |= 1u << i;
      return m;
    };
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
      if (y > 0) edge |= differs(L - Z);
      if (y < Y - 1) edge |= differs(L + Z);
    }
    if (axes & SD_AXIS_X) {
      if (x == 0 || x == X - 1) edge = 0xffffu;
      if (x > 0) edge |= differs(L - plane);
      if (x < X - 1) edge |= differs(L + plane);
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

// A key layout: the non-negative int32 keys split into LEVELS radix digits, digit l = (key >> SHIFT[l]) & MASK[l], every digit with its
// histogram of SD_BINS slots; top(key) is digit 0, and root(key) the distance that the float64 sum takes.
struct KeysI32 {             // squared voxel distances: 22 bits (3 * 1023^2 < 2^22) as 11 + 11
  static constexpr int LEVELS = 2;
  static constexpr int SHIFT[LEVELS] = {11, 0}, MASK[LEVELS] = {2047, 2047};
  // a value past the documented 22 bits counts in the last bin instead of past the table
  static __device__ __forceinline__ int top(int d) { return d >> 11 < SD_BINS ? d >> 11 : SD_BINS - 1; }
  static __device__ __forceinline__ double root(int d) { return sqrt((double)d); }
};
// The non-negative float32 squared distances of ctseg_distmap3d_weighted (-1.0f: none, skipped by its sign like the integer -1).
// Their 31-bit patterns order like the values, so the select runs on the patterns, as 11 + 11 + 9 bits (the last histograms use 512
// of their slots).
struct KeysF32 {
  static constexpr int LEVELS = 3;
  static constexpr int SHIFT[LEVELS] = {20, 9, 0}, MASK[LEVELS] = {2047, 2047, 511};
  static __device__ __forceinline__ int top(int d) { return d >> 20; }
  static __device__ __forceinline__ double root(int d) { return sqrt((double)__int_as_float(d)); }
};

// the digits 0 .. LEVEL of a key: what the prefixes of sd_walk are compared with
template <class KEYS, int LEVEL> __device__ __forceinline__ int sd_prefix(int d) {
  if constexpr (LEVEL == 0) return KEYS::top(d);
  else return d >> KEYS::SHIFT[LEVEL];
}

// The histograms of a select over `rows` rows, after one another: level 0 as [rows][SD_BINS], then every level l >= 1 as
// [rows][2][SD_BINS], inside the prefix of lo and inside that of hi.
__device__ __host__ __forceinline__ int64_t sd_level_at(int rows, int level) {
  return level == 0 ? 0 : (int64_t)rows * (2 * level - 1) * SD_BINS;
}

// The bins of a 2048-bin histogram `h` that hold the ranks k0 and k1, and the number of values below each bin: 256 lanes, 8 bins
// each, the sums of the lanes before it read from LDS.  Every lane returns the same.  k0, k1 < the histogram's total.
struct SdFound { int bin[2]; int64_t below[2]; };
__device__ __forceinline__ SdFound sd_locate(const uint32_t* __restrict__ h, int64_t k0, int64_t k1, uint32_t* s_sum, int64_t* s_found) {
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
  return {{(int)s_found[0], (int)s_found[2]}, {s_found[1], s_found[3]}};
}

// The levels 0 .. UPTO - 1 of row r, walked for both ranks: the prefix of the key found so far (its digits 0 .. UPTO - 1) and the
// rank that remains inside that prefix.  After all LEVELS the prefix is the key.
struct SdWalk { int prefix[2]; int64_t rank[2]; };
template <class KEYS, int UPTO>
__device__ __forceinline__ SdWalk sd_walk(const uint32_t* __restrict__ hist, int rows, int r, const SdRanks& k, uint32_t* s_sum,
                                          int64_t* s_found) {
  const SdFound top = sd_locate(hist + (int64_t)r * SD_BINS, k.lo, k.hi, s_sum, s_found);
  SdWalk w = {{top.bin[0], top.bin[1]}, {k.lo - top.below[0], k.hi - top.below[1]}};
#pragma unroll
  for (int l = 1; l < UPTO; ++l) {
    const uint32_t* t = hist + sd_level_at(rows, l) + (int64_t)r * 2 * SD_BINS;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const SdFound in = sd_locate(t + j * SD_BINS, w.rank[j], w.rank[j], s_sum, s_found);
      w.prefix[j] = (w.prefix[j] << (KEYS::SHIFT[l - 1] - KEYS::SHIFT[l])) | in.bin[0];
      w.rank[j] -= in.below[0];
    }
  }
  return w;
}

__global__ __launch_bounds__(256) void surface_zero_kernel(uint32_t* __restrict__ p, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) p[i] = 0u;
}

// Grid (slots, rows).  Workgroup (w, r): voxels [w * per, w * per + per) of row r.  The level-0 histogram, the maximum and the
// float64 partial in its fixed slot.
template <bool WIDE, class KEYS>
__global__ __launch_bounds__(256) void surface_level0_kernel(const uint8_t* __restrict__ edges, const int32_t* __restrict__ d2,
                                                             const int32_t* __restrict__ counts, int half, int64_t S, int64_t per,
                                                             uint32_t* __restrict__ hist, int32_t* __restrict__ vmax,
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
    atomicAdd(&s_h[KEYS::top(d)], 1u);
    mx = d > mx ? d : mx;
    sum += KEYS::root(d);
  });
  sum = wave_sum(sum);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { const int t = __shfl_xor(mx, off, 64); mx = t > mx ? t : mx; }
  if ((tid & 63) == 0) { s_red[tid >> 6] = sum; atomicMax(&s_max, mx); }
  __syncthreads();
  for (int i = tid; i < SD_BINS; i += 256)
    if (s_h[i]) atomicAdd(&hist[(int64_t)r * SD_BINS + i], s_h[i]);
  if (tid == 0) {
    part[(int64_t)r * gridDim.x + blockIdx.x] = (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
    if (s_max) atomicMax(&vmax[r], s_max);
  }
}

// The same grid.  The two histograms of digit LEVEL >= 1 inside the prefixes of lo and hi, which the finished levels below LEVEL
// of `hist` give; `lower` is level LEVEL of the same tables.  The ranks lo = floor((n - 1) q / 100), hi = min(lo + 1, n - 1) come
// from the counts of the edge pass.
template <bool WIDE, class KEYS, int LEVEL>
__global__ __launch_bounds__(256) void surface_lower_kernel(const uint8_t* __restrict__ edges, const int32_t* __restrict__ d2,
                                                            const int32_t* __restrict__ counts, int half, int64_t S, int64_t per,
                                                            double q, const uint32_t* __restrict__ hist,
                                                            uint32_t* __restrict__ lower) {
  __shared__ uint32_t s_h[2 * SD_BINS];                             // inside the prefix of lo, then of hi
  __shared__ uint32_t s_sum[256];
  __shared__ int64_t s_found[4];
  const int r = blockIdx.y, o = sd_partner(r, half), tid = threadIdx.x;
  const int32_t n = counts[r];
  if (n <= 0 || counts[o] <= 0) return;
  for (int i = tid; i < 2 * SD_BINS; i += 256) s_h[i] = 0u;
  if (tid < 4) s_found[tid] = 0;
  const SdWalk w = sd_walk<KEYS, LEVEL>(hist, gridDim.y, r, sd_ranks(n, q), s_sum, s_found);
  const int64_t v0 = (int64_t)blockIdx.x * per, v1 = v0 + per < S ? v0 + per : S;
  sd_for_each<WIDE>(edges + (int64_t)r * S, d2 + (int64_t)o * S, v0, v1, [&](int d) {
    const int p = sd_prefix<KEYS, LEVEL - 1>(d), bin = (d >> KEYS::SHIFT[LEVEL]) & KEYS::MASK[LEVEL];
    if (p == w.prefix[0]) atomicAdd(&s_h[bin], 1u);
    if (p == w.prefix[1]) atomicAdd(&s_h[SD_BINS + bin], 1u);
  });
  __syncthreads();
  for (int i = tid; i < 2 * SD_BINS; i += 256)
    if (s_h[i]) atomicAdd(&lower[(int64_t)r * 2 * SD_BINS + i], s_h[i]);
}

// Grid (rows).  stats[r] = {key[lo], key[hi], the largest key, 1} and fstats[r] = {sum of the roots, gamma}; {0, 0, 0, 0} and {0, 0}
// on a row without values.  (KeysF32: the keys are the bits of the floats.)
template <class KEYS>
__global__ __launch_bounds__(256) void surface_pick_kernel(const int32_t* __restrict__ counts, int half, int slots, double q,
                                                           const uint32_t* __restrict__ hist, const int32_t* __restrict__ vmax,
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
  const SdWalk w = sd_walk<KEYS, KEYS::LEVELS>(hist, gridDim.x, r, k, s_sum, s_found);
  if (tid == 0) {
    double sum = 0.0;
    for (int s = 0; s < slots; ++s) sum += part[(int64_t)r * slots + s];       // slot order: the same bits every run
    stats[r * 4 + 0] = w.prefix[0];
    stats[r * 4 + 1] = w.prefix[1];
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

// per row: SD_MAX_SLOTS float64 partials, the histograms (one of level 0, two of every level after it), the maximum (+ pad)
template <class KEYS> constexpr int64_t SD_ROW_BYTES = SD_MAX_SLOTS * 8 + (2 * KEYS::LEVELS - 1) * SD_BINS * 4 + 8;
static_assert(CTSEG_SURFACE_SELECT_ROW_BYTES == SD_ROW_BYTES<KeysI32>, "the header's workspace size");
static_assert(CTSEG_SURFACE_SELECT_F32_ROW_BYTES == SD_ROW_BYTES<KeysF32>, "the header's workspace size");

// f(std::true_type{}) or f(std::false_type{}): the one place where WIDE becomes a template argument
template <class F> static inline int with_wide(bool wide, F&& f) { return wide ? f(std::true_type{}) : f(std::false_type{}); }

static int check_surface_dims(const char* who, int32_t B, int32_t X, int32_t Y, int32_t Z, int32_t C) {
  if (check_sides(who, B, X, Y, Z)) return -1;
  CTSEG_REQUIRE(C >= 2 && C <= SD_MAX_CLASSES, "%s: 2 <= C <= %d classes (got %d)", who, SD_MAX_CLASSES, C);
  CTSEG_REQUIRE((int64_t)2 * B * (C - 1) <= 65535, "%s: %d samples of %d classes are too many for one launch", who, B, C);
  return 0;
}

// `keys`: the int32 squared distances, or the bits of the float32 ones (a float >= 0 orders like its bits; -1.0f is negative either way)
template <class KEYS>
static int surface_select_impl(const char* who, const uint8_t* edges, const int32_t* keys, const int32_t* counts, int32_t B, int32_t X,
                               int32_t Y, int32_t Z, int32_t C, double q, void* workspace, int64_t workspace_bytes, int32_t* stats,
                               double* fstats, void* stream) {
  CTSEG_REQUIRE(edges && keys && counts && workspace && stats && fstats,
                "%s: null pointer (edges, d2, counts, workspace, stats and fstats are required)", who);
  if (check_surface_dims(who, B, X, Y, Z, C)) return -1;
  CTSEG_REQUIRE(q >= 0.0 && q <= 100.0, "%s: a percentile in [0, 100] (got %g)", who, q);
  const int64_t S = (int64_t)X * Y * Z, per = sd_per_slot(S);
  const int rows = 2 * B * (C - 1), slots = (int)((S + per - 1) / per);
  const int64_t need = (int64_t)rows * SD_ROW_BYTES<KEYS>;
  CTSEG_REQUIRE(workspace_bytes >= need, "%s: the workspace holds %lld bytes, %lld are needed", who, (long long)workspace_bytes,
                (long long)need);
  const bool wide = S % SD_RUN == 0;
  CTSEG_REQUIRE(((uintptr_t)workspace % 8) == 0 && ((uintptr_t)fstats % 8) == 0 && ((uintptr_t)stats % 4) == 0 &&
                    ((uintptr_t)counts % 4) == 0 && ((uintptr_t)keys % 4) == 0 && (!wide || ((uintptr_t)edges % 16) == 0),
                "%s: unaligned pointer", who);
  double* part = (double*)workspace;                                 // [rows][slots <= 64], then the integer tables
  uint32_t* hist = (uint32_t*)(part + (int64_t)rows * SD_MAX_SLOTS);   // see sd_level_at
  int32_t* vmax = (int32_t*)(hist + sd_level_at(rows, KEYS::LEVELS));  // [rows]
  const int64_t words = sd_level_at(rows, KEYS::LEVELS) + rows;
  const int half = B * (C - 1);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(surface_zero_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, st, hist, words);
  CTSEG_LAUNCH_CHECK_PASS(who, "zero");
  const dim3 grid((unsigned)slots, (unsigned)rows);
  const int rc = with_wide(wide, [&](auto wide_t) {
    constexpr bool WIDE = decltype(wide_t)::value;
    hipLaunchKernelGGL((surface_level0_kernel<WIDE, KEYS>), grid, dim3(256), 0, st, edges, keys, counts, half, S, per, hist, vmax, part);
    CTSEG_LAUNCH_CHECK_PASS(who, "level 0");
    const auto lower = [&](auto level) {                             // no launch for a level that the layout does not have
      constexpr int LEVEL = decltype(level)::value;
      if constexpr (LEVEL < KEYS::LEVELS) {
        hipLaunchKernelGGL((surface_lower_kernel<WIDE, KEYS, LEVEL>), grid, dim3(256), 0, st, edges, keys, counts, half, S, per, q,
                           (const uint32_t*)hist, hist + sd_level_at(rows, LEVEL));
        CTSEG_LAUNCH_CHECK_PASS(who, "lower level");
      }
      return 0;
    };
    static_assert(KEYS::LEVELS <= 3, "one call of `lower` per level");
    return lower(std::integral_constant<int, 1>{}) || lower(std::integral_constant<int, 2>{}) ? -2 : 0;
  });
  if (rc) return rc;
  hipLaunchKernelGGL(surface_pick_kernel<KEYS>, dim3((unsigned)rows), dim3(256), 0, st, counts, half, slots, q, (const uint32_t*)hist,
                     (const int32_t*)vmax, (const double*)part, stats, fstats);
  CTSEG_LAUNCH_CHECK_PASS(who, "pick");
  return 0;
}

}  // namespace ctseg

using namespace ctseg;

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
  with_wide(wide, [&](auto wide_t) {
    hipLaunchKernelGGL(surface_edges_kernel<decltype(wide_t)::value>, grid, dim3(256), 0, st, pred, target, B, X, Y, Z, C, axes, runs,
                       edges, counts);
    return 0;
  });
  CTSEG_LAUNCH_CHECK("surface_edges");
  return 0;
}

extern "C" int ctseg_surface_select(const uint8_t* edges, const int32_t* d2, const int32_t* counts, int32_t B, int32_t X, int32_t Y,
                                    int32_t Z, int32_t C, double q, void* workspace, int64_t workspace_bytes, int32_t* stats,
                                    double* fstats, void* stream) {
  return surface_select_impl<KeysI32>("surface_select", edges, d2, counts, B, X, Y, Z, C, q, workspace, workspace_bytes, stats, fstats,
                                      stream);
}

extern "C" int ctseg_surface_select_f32(const uint8_t* edges, const float* d2, const int32_t* counts, int32_t B, int32_t X, int32_t Y,
                                        int32_t Z, int32_t C, double q, void* workspace, int64_t workspace_bytes, int32_t* stats,
                                        double* fstats, void* stream) {
  return surface_select_impl<KeysF32>("surface_select_f32", edges, (const int32_t*)d2, counts, B, X, Y, Z, C, q, workspace,
                                      workspace_bytes, stats, fstats, stream);
}
