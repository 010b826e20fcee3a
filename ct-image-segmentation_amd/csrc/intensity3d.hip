// Intensity stage of the 3-D input pipeline: Gaussian blur, additive Gaussian noise and a gamma curve on one fp32 volume
// [Ho][Wo][Do] (Do contiguous), in this fixed order: blur, then noise, then gamma.  Any of the three may be absent.  The rules are
// restated in include/ctseg_hip.h (ctseg_intensity3d); tests/test_intensity3d.py holds the kernels to a numpy restatement of them.
//
// Blur    separable, one pass per axis with a radius > 0, in the order d (contiguous), w, h; each pass stores float32.  Per axis the
//         host hands over r <= 12 and the taps w_0..w_r.  Border = edge replication (indices clamped to [0, n - 1]; r may exceed n).
//           acc = w_0 * v[i];   for k = 1..r:  acc = acc + w_k * (v[i-k] + v[i+k])
//         Every operation is ONE float32 rounding: a rounded add of the pair, a rounded multiply, a rounded add into acc
//         and never a fused multiply-add, so that a float32 restatement gives the same bits.  The expressions are plain * and +
//         under this file's `fp contract(off)`: HIP's __fmul_rn / __fadd_rn are themselves plain operators compiled under the
//         header's contraction mode, and the compiler fuses them.
// Noise   v = v + std * n,  n = sqrtf(-2 * logf(u1)) * cosf(6.2831855f * u2) in float32 (each product and the sum rounded once),
//         u1 = ((z >> 40) + 1) * 2^-24 in (0, 1],  u2 = ((z >> 16) & 0xFFFFFF) * 2^-24 in [0, 1),
//         z = splitmix64_mix(seed + (i + 1) * SPLITMIX_GOLDEN),  i = the voxel's linear index in storage.  Stateless.
// Gamma   t = min(max((v - lo) * inv, 0), 1),  v = lo + (hi - lo) * powf(t, g);  inv = (float)(1 / ((double)hi - lo)) and hi - lo
//         (float32) are formed on the host.  Values outside [lo, hi], such as those the noise pushed out, are CLAMPED by this step.
//
// A workgroup owns whole lines of the axis it blurs and keeps them in LDS: the d pass a contiguous run of whole rows (<= 2048
// voxels), the w and h passes all n positions of 32 (n <= 512) or 16 adjacent columns (n * TI * 4 <= 64 KiB).  Nothing outside its
// own lines is read, so a pass moves 8 bytes per voxel, reads no halo, and may run IN PLACE: the first pass reads the input and
// writes the output, every later one works on the output, and no scratch volume exists.  The point stage (noise, gamma) sits in the
// store of the last blur pass; it is a launch of its own only when no axis is blurred.
#pragma clang fp contract(off)
#include <cmath>

#include "ctseg_dev.h"
#include "splitmix.h"

namespace ctseg {

constexpr int INTENSITY_MAX_R = 12;
constexpr int D_CHUNK = 2048;           // voxels of whole rows a workgroup of the d pass holds
constexpr int MAX_SIDE = 1024;

struct BlurTaps {
  int r;
  float w[INTENSITY_MAX_R + 1];
};

struct PointArgs {
  int noise, gamma;
  float std;
  uint64_t seed;
  float lo, span, inv, g;
};

__device__ __forceinline__ float point_value(float v, uint64_t i, const PointArgs& p) {
  if (p.noise) {
    const uint64_t z = splitmix64_mix(p.seed + (i + 1ull) * SPLITMIX_GOLDEN);
    const float u1 = (float)((uint32_t)(z >> 40) + 1u) * 0x1.0p-24f;        // exact: integers of at most 2^24
    const float u2 = (float)((uint32_t)(z >> 16) & 0xFFFFFFu) * 0x1.0p-24f;
    const float n = sqrtf(-2.f * logf(u1)) * cosf(6.2831855f * u2);
    v = v + p.std * n;
  }
  if (p.gamma) {
    const float t = fminf(fmaxf((v - p.lo) * p.inv, 0.f), 1.f);
    v = p.lo + p.span * powf(t, p.g);
  }
  return v;
}

// one output of a pass: line[] holds the axis' n values `stride` floats apart, a = the position
__device__ __forceinline__ float blur_at(const float* line, int stride, int a, int n, const BlurTaps& t) {
  float acc = t.w[0] * line[a * stride];
  for (int k = 1; k <= t.r; ++k) {
    const int lo = max(a - k, 0), hi = min(a + k, n - 1);
    acc = acc + t.w[k] * (line[lo * stride] + line[hi * stride]);
  }
  return acc;
}

// d pass: the volume as `rows` contiguous rows of Z; a workgroup holds `per` whole rows (per * Z <= D_CHUNK)
template <bool POINT>
__global__ __launch_bounds__(256) void blur3d_d_kernel(const float* in, float* out, int64_t rows, int Z, int per, const BlurTaps t,
                                                       const PointArgs p) {
  __shared__ float s[D_CHUNK];
  const int64_t row0 = (int64_t)blockIdx.x * per;
  const int count = (int)min((int64_t)per, rows - row0) * Z;
  const int64_t base = row0 * Z;
  for (int e = threadIdx.x; e < count; e += 256) s[e] = in[base + e];
  __syncthreads();
  for (int e = threadIdx.x; e < count; e += 256) {
    const int z = e % Z;
    const float v = blur_at(s + (e - z), 1, z, Z, t);
    out[base + e] = POINT ? point_value(v, (uint64_t)(base + e), p) : v;
  }
}

// w and h passes: the volume as [outer][n][inner]; a workgroup holds all n positions of TI adjacent inner columns
template <int TI, bool POINT>
__global__ __launch_bounds__(256) void blur3d_line_kernel(const float* in, float* out, int n, int64_t inner, int tiles, const BlurTaps t,
                                                          const PointArgs p) {
  extern __shared__ __attribute__((aligned(16))) float line[];
  const int64_t o = blockIdx.x / tiles;
  const int64_t col = (int64_t)(blockIdx.x % tiles) * TI + threadIdx.x % TI;
  const int c = threadIdx.x % TI, a0 = threadIdx.x / TI;
  const bool live = col < inner;
  const int64_t base = o * n * inner + col;
  for (int a = a0; a < n; a += 256 / TI) line[a * TI + c] = live ? in[base + a * inner] : 0.f;
  __syncthreads();
  if (!live) return;
  for (int a = a0; a < n; a += 256 / TI) {
    const float v = blur_at(line + c, TI, a, n, t);
    const int64_t i = base + a * inner;
    out[i] = POINT ? point_value(v, (uint64_t)i, p) : v;
  }
}

__global__ __launch_bounds__(256) void intensity3d_point_kernel(const float* in, float* out, int64_t N, const PointArgs p) {
  const int64_t i0 = (int64_t)blockIdx.x * 1024 + threadIdx.x;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int64_t i = i0 + 256 * j;
    if (i < N) out[i] = point_value(in[i], (uint64_t)i, p);
  }
}

// what a call launches: the axes with a radius, and whether a point stage exists.  -1: an argument the entry refuses
static int intensity3d_plan(const char* who, const int32_t* radius, float noise_std, int32_t has_range, float gamma, bool& point) {
  CTSEG_REQUIRE(radius, "%s: radius is a null pointer", who);
  int passes = 0;
  for (int a = 0; a < 3; ++a) {
    CTSEG_REQUIRE(radius[a] >= 0 && radius[a] <= INTENSITY_MAX_R, "%s: radius[%d] = %d is outside [0, %d] (0 < sigma <= 4)", who, a,
                  radius[a], INTENSITY_MAX_R);
    passes += radius[a] > 0;
  }
  CTSEG_REQUIRE(std::isfinite(noise_std) && noise_std >= 0.f, "%s: noise_std is negative or not finite", who);
  CTSEG_REQUIRE(has_range == 0 || has_range == 1, "%s: has_range is 0 or 1", who);
  if (has_range) CTSEG_REQUIRE(gamma >= 0.25f && gamma <= 4.f, "%s: gamma %g is outside [0.25, 4]", who, (double)gamma);
  else CTSEG_REQUIRE(gamma == 1.f, "%s: gamma %g without a value range", who, (double)gamma);
  point = noise_std > 0.f || has_range;
  return passes + (passes == 0 && point);
}

}  // namespace ctseg

using namespace ctseg;

extern "C" int ctseg_intensity3d_launches(const int32_t* radius, float noise_std, int32_t has_range, float gamma) {
  bool point;
  return intensity3d_plan("intensity3d_launches", radius, noise_std, has_range, gamma, point);
}

extern "C" int ctseg_intensity3d(const float* image, float* image_out, int32_t Do, int32_t Ho, int32_t Wo, const int32_t* radius,
                                 const float* taps, float noise_std, int64_t noise_seed, int32_t has_range, float lo, float hi,
                                 float gamma, void* stream) {
  const char* who = "intensity3d";
  CTSEG_REQUIRE(image && image_out, "%s: null pointer", who);
  CTSEG_REQUIRE(Do >= 1 && Ho >= 1 && Wo >= 1 && Do <= MAX_SIDE && Ho <= MAX_SIDE && Wo <= MAX_SIDE,
                "%s: bad geometry %d x %d x %d (sides in [1, %d])", who, Do, Ho, Wo, MAX_SIDE);
  bool point;
  const int launches = intensity3d_plan(who, radius, noise_std, has_range, gamma, point);
  if (launches < 0) return launches;
  BlurTaps bt[3];
  for (int a = 0; a < 3; ++a) {
    bt[a].r = radius[a];
    if (radius[a] == 0) continue;
    CTSEG_REQUIRE(taps, "%s: taps is a null pointer", who);
    double sum = 0.0;
    for (int k = 0; k <= radius[a]; ++k) {
      const float w = taps[a * (INTENSITY_MAX_R + 1) + k];
      CTSEG_REQUIRE(std::isfinite(w) && w >= 0.f, "%s: taps[%d][%d] is negative or not finite", who, a, k);
      bt[a].w[k] = w;
      sum += k ? 2.0 * w : w;
    }
    CTSEG_REQUIRE(std::fabs(sum - 1.0) <= (radius[a] + 2) * 0x1.0p-24, "%s: taps[%d] sum to %.9g, not 1 (w_0 + 2 sum w_k)", who, a, sum);
  }
  PointArgs p = {};
  if (has_range) {
    CTSEG_REQUIRE(std::isfinite(lo) && std::isfinite(hi) && lo < hi && std::isfinite(hi - lo), "%s: value range (%g, %g) is empty or not finite",
                  who, (double)lo, (double)hi);
    p.gamma = 1, p.lo = lo, p.span = hi - lo, p.inv = (float)(1.0 / ((double)hi - (double)lo)), p.g = gamma;
    CTSEG_REQUIRE(std::isfinite(p.inv), "%s: value range (%g, %g) is too narrow", who, (double)lo, (double)hi);
  }
  p.noise = noise_std > 0.f, p.std = noise_std, p.seed = (uint64_t)noise_seed;

  hipStream_t st = (hipStream_t)stream;
  const int64_t N = (int64_t)Do * Ho * Wo;              // at most 2^30
  if (launches == 0) {                                   // nothing to do: no launch; a separate output gets the input's bits
    if (image_out != image) {
      const hipError_t e = hipMemcpyAsync(image_out, image, (size_t)N * 4, hipMemcpyDeviceToDevice, st);
      CTSEG_REQUIRE(e == hipSuccess, "%s: %s", who, hipGetErrorString(e));
    }
    return 0;
  }
  const PointArgs none = {};
  const float* src = image;                              // the first launch reads the input, every later one works on the output
  int left = launches;
  bool blurred = false;
  auto last = [&] { return --left == 0 && point; };
  if (bt[0].r) {                                         // d: storage axis Z
    const int64_t rows = (int64_t)Ho * Wo;
    const int per = D_CHUNK / Do;                        // >= 2
    const dim3 grid((unsigned)((rows + per - 1) / per));
    if (last()) hipLaunchKernelGGL(blur3d_d_kernel<true>, grid, dim3(256), 0, st, src, image_out, rows, Do, per, bt[0], p);
    else hipLaunchKernelGGL(blur3d_d_kernel<false>, grid, dim3(256), 0, st, src, image_out, rows, Do, per, bt[0], none);
    CTSEG_LAUNCH_CHECK("intensity3d (d pass)");
    src = image_out, blurred = true;
  }
  // w: storage axis Y, [Ho][Wo][Do];  h: storage axis X, [1][Ho][Wo * Do]
  const struct { int axis, outer, n; int64_t inner; } strided[2] = {{2, Ho, Wo, Do}, {1, 1, Ho, (int64_t)Wo * Do}};
  for (const auto& s : strided) {
    if (!bt[s.axis].r) continue;
    const bool pt = last();
    const int ti = s.n <= 512 ? 32 : 16;
    const int tiles = (int)((s.inner + ti - 1) / ti);
    const dim3 grid((unsigned)(s.outer * tiles));        // at most 1024 * 32 or 2^20 / 16
    const size_t lds = (size_t)s.n * ti * 4;             // at most 64 KiB
    const PointArgs& pa = pt ? p : none;
    if (ti == 32) {
      if (pt) hipLaunchKernelGGL((blur3d_line_kernel<32, true>), grid, dim3(256), lds, st, src, image_out, s.n, s.inner, tiles, bt[s.axis], pa);
      else hipLaunchKernelGGL((blur3d_line_kernel<32, false>), grid, dim3(256), lds, st, src, image_out, s.n, s.inner, tiles, bt[s.axis], pa);
    } else {
      if (pt) hipLaunchKernelGGL((blur3d_line_kernel<16, true>), grid, dim3(256), lds, st, src, image_out, s.n, s.inner, tiles, bt[s.axis], pa);
      else hipLaunchKernelGGL((blur3d_line_kernel<16, false>), grid, dim3(256), lds, st, src, image_out, s.n, s.inner, tiles, bt[s.axis], pa);
    }
    CTSEG_LAUNCH_CHECK(s.axis == 2 ? "intensity3d (w pass)" : "intensity3d (h pass)");
    src = image_out, blurred = true;
  }
  if (!blurred) {                                        // no axis is blurred: the point stage is the launch
    hipLaunchKernelGGL(intensity3d_point_kernel, dim3((unsigned)((N + 1023) / 1024)), dim3(256), 0, st, src, image_out, N, p);
    CTSEG_LAUNCH_CHECK("intensity3d (point stage)");
  }
  return 0;
}
