// BatchNorm{2,3}d(affine=True, track_running_stats=True) + PReLU forward/backward for channels-last activations (gfx950).
// MONAI's Convolution block with norm=Norm.BATCH = conv -> BatchNorm -> PReLU.  The training-mode statistics are the conv
// epilogue's per-(sample, tile) (sum, sumsq) partials -- the same ones InstanceNorm uses (norm_act.hip) -- summed over the
// samples as well as the tiles.  Every sum is combined in fp64 in a fixed order (no float atomics): results are deterministic.
//
// Passes (one launch each):
//   training forward : batchnorm_finalize (mean/rstd, scale/shift table, running statistics, num_batches_tracked)
//                      -> scale_shift_prelu_fwd
//   eval forward     : batchnorm_eval_table (scale/shift from the running statistics) -> scale_shift_prelu_fwd
//   training backward: bn_prelu_bwd_reduce -> bn_prelu_bwd_finalize (d gamma, d beta) -> bn_prelu_bwd_apply (dy, d alpha)
#include "norm_common.h"

namespace ctseg {

// partials: R = N * P rows of [2][ld] fp32 (sample-major, so the rows of all samples are contiguous).  One block per 8 channels
// (col16_stats); threads t < 8 then own one channel each: statistics, tables and the running-statistics update.
template <int RL>
__global__ __launch_bounds__(16 * RL) void bn_finalize_kernel(const float* __restrict__ part, int R, int ld, int col0, int C,
                                                             double count, double eps, double momentum,
                                                             const float* __restrict__ gamma, const float* __restrict__ beta,
                                                             float* __restrict__ running_mean, float* __restrict__ running_var,
                                                             int64_t* __restrict__ nbt, float* __restrict__ mean_rstd,
                                                             float* __restrict__ scale_shift) {
  const int c0 = blockIdx.x * 8, t = threadIdx.x;
  col16_stats<RL>(part, R, ld, col0, C, count, c0, t, [&](int k, double mean, double var) NORM_FN {
    const int ch = c0 + k;
    const double rstd = 1.0 / sqrt(var + eps);
    const double sc = (double)gamma[ch] * rstd;
    mean_rstd[2 * ch] = (float)mean;
    mean_rstd[2 * ch + 1] = (float)rstd;
    scale_shift[2 * ch] = (float)sc;
    scale_shift[2 * ch + 1] = (float)((double)beta[ch] - mean * sc);
    const double unbiased = count > 1.0 ? var * count / (count - 1.0) : var;
    running_mean[ch] = (float)((1.0 - momentum) * (double)running_mean[ch] + momentum * mean);
    running_var[ch] = (float)((1.0 - momentum) * (double)running_var[ch] + momentum * unbiased);
  });
  if (blockIdx.x == 0 && t == 0) nbt[0] = nbt[0] + 1;
}

__global__ __launch_bounds__(256) void bn_eval_table_kernel(const float* __restrict__ running_mean, const float* __restrict__ running_var,
                                                            const float* __restrict__ gamma, const float* __restrict__ beta, int C,
                                                            double eps, float* __restrict__ scale_shift) {
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    const double sc = (double)gamma[c] / sqrt((double)running_var[c] + eps);
    scale_shift[2 * c] = (float)sc;
    scale_shift[2 * c + 1] = (float)((double)beta[c] - (double)running_mean[c] * sc);
  }
}

// out = prelu(y * scale_c + shift_c, alpha) [+ res]: instnorm_prelu_fwd_kernel's access pattern with one table for every sample
template <typename T, int EPC>
__global__ __launch_bounds__(256) void scale_shift_prelu_fwd_kernel(const char* __restrict__ y, int y_ld,
                                                                     const float* __restrict__ scale_shift,
                                                                     const float* __restrict__ alpha, const char* __restrict__ res,
                                                                     int res_ld, char* __restrict__ out, int out_ld, int64_t S,
                                                                     int C, int Cv) {
  constexpr int SZ = TT<T>::SZ;
  extern __shared__ float s_ss[];   // tab_row<2, EPC>: (scale, shift) of each channel
  const int n = blockIdx.y;
  for (int i = threadIdx.x; i < 2 * C; i += blockDim.x) tab_row<2, EPC>(s_ss, i >> 1)[i & 1] = scale_shift[i];
  __syncthreads();
  const float al = alpha[0];
  const int64_t stride = (int64_t)gridDim.x * blockDim.x, i0 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  chunk_sweep_fwd(i0, stride, S, Cv, [&](int64_t v, int cv) {
    const float* tab = tab_chunk<2, EPC>(s_ss, cv);
    const int64_t vox = (int64_t)n * S + v;
    float x[EPC], r[EPC];
    load_ep<T, EPC>(y + (vox * y_ld + cv * EPC) * SZ, x);
    if (res != nullptr) load_ep<T, EPC>(res + (vox * res_ld + cv * EPC) * SZ, r);
#pragma unroll
    for (int e = 0; e < EPC; ++e) {
      const int c = cv * EPC + e;
      float o = 0.f;
      if (c < C) {
        o = x[e] * tab[2 * e] + tab[2 * e + 1];
        o = o > 0.f ? o : al * o;
        if (res != nullptr) o += r[e];
      }
      x[e] = o;
    }
    store_ep<T, EPC>(out + (vox * out_ld + cv * EPC) * SZ, x);
  });
}

// backward pass 1, per block (p, n): rows [p*rows_per, ...) of sample n -> partials[n][p][3][ld] =
// (sum dz, sum dz * xhat, sum over z <= 0 of g * z) with z = gamma * xhat + beta, dz = g * prelu'(z)
template <typename T, int EPC>
__global__ __launch_bounds__(256) void bn_prelu_bwd_reduce_kernel(const char* __restrict__ g, int g_ld, const char* __restrict__ y,
                                                                   int y_ld, const float* __restrict__ mean_rstd,
                                                                   const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                   const float* __restrict__ alpha, float* __restrict__ partials,
                                                                   int P, int ld, int64_t S, int C, int Cv) {
  extern __shared__ float s_tab[];       // tab_row<4, EPC>: mean, rstd, gamma, beta of each channel, then the reduction scratch
  const int n = blockIdx.y;
  for (int i = threadIdx.x; i < C; i += blockDim.x) {
    float* t = tab_row<4, EPC>(s_tab, i);
    t[0] = mean_rstd[2 * i];
    t[1] = mean_rstd[2 * i + 1];
    t[2] = gamma[i];
    t[3] = beta[i];
  }
  __syncthreads();
  const float al = alpha[0];
  bwd_reduce_rows<T, EPC>(g, g_ld, y, y_ld, partials, tab_chunk<4, EPC>(s_tab, Cv), P, ld, S, C, Cv, blockIdx.x, n, threadIdx.x,
                          [&](int cv, int e, float gv, float yv, float& a1, float& a2, float& a3) NORM_FN {
    const float* tab = tab_chunk<4, EPC>(s_tab, cv);
    const float xh = (yv - tab[4 * e]) * tab[4 * e + 1];
    const float z = tab[4 * e + 2] * xh + tab[4 * e + 3];
    const float dz = gv * (z > 0.f ? 1.f : al);
    a1 += dz;
    a2 += dz * xh;
    a3 += z > 0.f ? 0.f : gv * z;
  });
}

// backward pass 2, one block per channel: the R = N * P partial rows in a fixed tree -> d beta, d gamma (straight into the flat
// gradient buffer), sums[c] = (d beta / M, d gamma / M) for the apply pass, da_part[c] = the channel's slope-gradient term
__global__ __launch_bounds__(256) void bn_prelu_bwd_finalize_kernel(const float* __restrict__ partials, int R, int ld, double M,
                                                                    float* __restrict__ sums, float* __restrict__ dgamma,
                                                                    float* __restrict__ dbeta, double* __restrict__ da_part) {
  __shared__ double s_acc[3][4];
  const int c = blockIdx.x;
  block_sum3(R, ld, threadIdx.x, s_acc, [&](int row) NORM_FN { return partials + (int64_t)row * 3 * ld + c; },
             [&](double db, double dg, double da) NORM_FN {
    sums[2 * c] = (float)(db / M);
    sums[2 * c + 1] = (float)(dg / M);
    dbeta[c] = (float)db;
    dgamma[c] = (float)dg;
    da_part[c] = da;
  });
}

// backward pass 3: dy = gamma * rstd * (dz - d beta / M - xhat * d gamma / M) [+ g copied to g_copy]; block (0, 0) also writes
// dalpha = fixed-order sum of da_part[0 .. n_da).  Walks backwards (last sample, last voxel first) like the InstanceNorm apply
// pass: the reduce pass streamed (g, y) front to back, so the tail of both is still in L2 / Infinity Cache.
template <typename T, int EPC>
__global__ __launch_bounds__(256) void bn_prelu_bwd_apply_kernel(const char* __restrict__ g, int g_ld, const char* __restrict__ y,
                                                                  int y_ld, const float* __restrict__ mean_rstd,
                                                                  const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                  const float* __restrict__ alpha, const float* __restrict__ sums,
                                                                  char* __restrict__ dy, int dy_ld, char* __restrict__ g_copy,
                                                                  int g_copy_ld, int64_t S, int C, int Cv,
                                                                  const double* __restrict__ da_part, int n_da,
                                                                  float* __restrict__ dalpha) {
  constexpr int SZ = TT<T>::SZ;
  extern __shared__ float s_tab[];   // tab_row<6, EPC>: mean, rstd, gamma, beta, s1, s2 of each channel
  if (da_part != nullptr && blockIdx.x == 0 && blockIdx.y == 0) slope_grad_sum(da_part, n_da, dalpha, threadIdx.x);
  const int n = gridDim.y - 1 - blockIdx.y;
  for (int i = threadIdx.x; i < C; i += blockDim.x) {
    float* t = tab_row<6, EPC>(s_tab, i);
    t[0] = mean_rstd[2 * i];
    t[1] = mean_rstd[2 * i + 1];
    t[2] = gamma[i];
    t[3] = beta[i];
    t[4] = sums[2 * i];
    t[5] = sums[2 * i + 1];
  }
  __syncthreads();
  const float al = alpha[0];
  const int64_t stride = (int64_t)gridDim.x * blockDim.x, ir0 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  chunk_sweep_bwd(ir0, stride, S * Cv, Cv, [&](int64_t v, int cv) {
    const float* tab = tab_chunk<6, EPC>(s_tab, cv);
    const int64_t vox = (int64_t)n * S + v;
    float gv[EPC], yv[EPC], o[EPC];
    load_ep<T, EPC>(g + (vox * g_ld + cv * EPC) * SZ, gv);
    load_ep<T, EPC>(y + (vox * y_ld + cv * EPC) * SZ, yv);
#pragma unroll
    for (int e = 0; e < EPC; ++e) {
      float r = 0.f;
      if (cv * EPC + e < C) {
        const float* k = tab + 6 * e;
        const float xh = (yv[e] - k[0]) * k[1];
        const float z = k[2] * xh + k[3];
        const float dz = gv[e] * (z > 0.f ? 1.f : al);
        r = k[2] * k[1] * (dz - k[4] - xh * k[5]);
      }
      o[e] = r;
    }
    store_dy_chunk<T, EPC>(dy, dy_ld, vox, cv, Cv, o);
    if (g_copy != nullptr) store_ep<T, EPC>(g_copy + (vox * g_copy_ld + cv * EPC) * SZ, gv);
  });
}

}  // namespace ctseg

using namespace ctseg;

extern "C" int ctseg_batchnorm_finalize(const float* partials, int32_t N, int32_t P, int32_t ld, int32_t col0, int32_t C,
                                        double count, double eps, double momentum, const float* gamma, const float* beta,
                                        float* running_mean, float* running_var, int64_t* num_batches_tracked, float* mean_rstd,
                                        float* scale_shift, void* stream) {
  CTSEG_REQUIRE(partials && gamma && beta && running_mean && running_var && num_batches_tracked && mean_rstd && scale_shift &&
                N > 0 && P > 0 && C > 0 && col0 >= 0 && col0 + C <= ld && count > 0.0 && momentum >= 0.0 && momentum <= 1.0,
                "batchnorm_finalize: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  const int R = N * P;
  if (R <= 1024)
    hipLaunchKernelGGL(bn_finalize_kernel<16>, dim3((C + 7) / 8), dim3(256), 0, st, partials, R, ld, col0, C, count, eps, momentum,
                       gamma, beta, running_mean, running_var, (int64_t*)num_batches_tracked, mean_rstd, scale_shift);
  else
    hipLaunchKernelGGL(bn_finalize_kernel<64>, dim3((C + 7) / 8), dim3(1024), 0, st, partials, R, ld, col0, C, count, eps, momentum,
                       gamma, beta, running_mean, running_var, (int64_t*)num_batches_tracked, mean_rstd, scale_shift);
  CTSEG_LAUNCH_CHECK("batchnorm_finalize");
  return 0;
}

extern "C" int ctseg_batchnorm_eval_table(const float* running_mean, const float* running_var, const float* gamma, const float* beta,
                                          int32_t C, double eps, float* scale_shift, void* stream) {
  CTSEG_REQUIRE(running_mean && running_var && gamma && beta && scale_shift && C > 0, "batchnorm_eval_table: bad arguments");
  hipLaunchKernelGGL(bn_eval_table_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, running_mean, running_var, gamma, beta, C, eps,
                     scale_shift);
  CTSEG_LAUNCH_CHECK("batchnorm_eval_table");
  return 0;
}

extern "C" int ctseg_scale_shift_prelu_fwd(int32_t dtype, const void* y, int32_t y_ld, const float* scale_shift, const float* alpha,
                                           const void* res, int32_t res_ld, void* out, int32_t out_ld, int32_t N, int64_t S,
                                           int32_t C, void* stream) {
  CTSEG_REQUIRE(y && out && scale_shift && alpha && N > 0 && S > 0 && C > 0, "scale_shift_prelu_fwd: bad arguments");
  CHECK_CL(dtype, C, true, true, y_ld, out_ld, res ? res_ld : y_ld);
  dim3 grid(ew_blocks_for(S * Cv, Cv), N);
  const size_t sh = Cv * (2 * EPC_ + 1) * sizeof(float);
  hipStream_t st = (hipStream_t)stream;
  dispatch_chunk<true>(dtype, EPC_, [&](auto t, auto ep) {
    hipLaunchKernelGGL((scale_shift_prelu_fwd_kernel<decltype(t), ep>), grid, dim3(256), sh, st, (const char*)y, y_ld, scale_shift,
                       alpha, (const char*)res, res_ld, (char*)out, out_ld, S, C, Cv);
  });
  CTSEG_LAUNCH_CHECK("scale_shift_prelu_fwd");
  return 0;
}

extern "C" int ctseg_batchnorm_prelu_bwd_reduce(int32_t dtype, const void* g, int32_t g_ld, const void* y, int32_t y_ld,
                                                const float* mean_rstd, const float* gamma, const float* beta, const float* alpha,
                                                float* partials, int32_t P, int32_t ld, int32_t N, int64_t S, int32_t C, void* stream) {
  CTSEG_REQUIRE(g && y && mean_rstd && gamma && beta && alpha && partials && P > 0 && N > 0 && S > 0 && C > 0 && C <= ld,
                "batchnorm_prelu_bwd_reduce: bad arguments");
  CHECK_CL(dtype, C, true, false, g_ld, y_ld);
  CTSEG_REQUIRE(Cv <= 256, "batchnorm_prelu_bwd_reduce: too many channels");
  const bool pow2 = (Cv & (Cv - 1)) == 0 && Cv <= 64;
  const size_t sh = (Cv * (4 * EPC_ + 1) + (pow2 ? 4 * Cv * 3 * EPC_ : 256 * 3 * EPC_)) * sizeof(float);
  hipStream_t st = (hipStream_t)stream;
  dispatch_chunk<false>(dtype, EPC_, [&](auto t, auto ep) {
    hipLaunchKernelGGL((bn_prelu_bwd_reduce_kernel<decltype(t), ep>), dim3(P, N), dim3(256), sh, st, (const char*)g, g_ld, (const char*)y,
                       y_ld, mean_rstd, gamma, beta, alpha, partials, P, ld, S, C, Cv);
  });
  CTSEG_LAUNCH_CHECK("batchnorm_prelu_bwd_reduce");
  return 0;
}

extern "C" int ctseg_batchnorm_prelu_bwd_finalize(const float* partials, int32_t N, int32_t P, int32_t ld, int32_t C, double count,
                                                  float* sums, float* dgamma, float* dbeta, double* da_part, void* stream) {
  CTSEG_REQUIRE(partials && sums && dgamma && dbeta && da_part && N > 0 && P > 0 && C > 0 && C <= ld && count > 0.0,
                "batchnorm_prelu_bwd_finalize: bad arguments");
  hipLaunchKernelGGL(bn_prelu_bwd_finalize_kernel, dim3(C), dim3(256), 0, (hipStream_t)stream, partials, N * P, ld, count, sums,
                     dgamma, dbeta, da_part);
  CTSEG_LAUNCH_CHECK("batchnorm_prelu_bwd_finalize");
  return 0;
}

extern "C" int ctseg_batchnorm_prelu_bwd_apply(int32_t dtype, const void* g, int32_t g_ld, const void* y, int32_t y_ld,
                                               const float* mean_rstd, const float* gamma, const float* beta, const float* alpha,
                                               const float* sums, void* dy, int32_t dy_ld, void* g_copy, int32_t g_copy_ld, int32_t N,
                                               int64_t S, int32_t C, const double* da_part, int32_t n_da, float* dalpha, void* stream) {
  CTSEG_REQUIRE(g && y && mean_rstd && gamma && beta && alpha && sums && dy && N > 0 && S > 0 && C > 0,
                "batchnorm_prelu_bwd_apply: bad arguments");
  CTSEG_REQUIRE(da_part == nullptr || (dalpha != nullptr && n_da > 0), "batchnorm_prelu_bwd_apply: slope-gradient arguments");
  CHECK_CL(dtype, C, true, false, g_ld, y_ld, dy_ld, g_copy ? g_copy_ld : dy_ld);
  dim3 grid(ew_blocks_for(S * Cv, Cv), N);
  const size_t sh = Cv * (6 * EPC_ + 1) * sizeof(float);
  hipStream_t st = (hipStream_t)stream;
  dispatch_chunk<false>(dtype, EPC_, [&](auto t, auto ep) {
    hipLaunchKernelGGL((bn_prelu_bwd_apply_kernel<decltype(t), ep>), grid, dim3(256), sh, st, (const char*)g, g_ld, (const char*)y, y_ld,
                       mean_rstd, gamma, beta, alpha, sums, (char*)dy, dy_ld, (char*)g_copy, g_copy_ld, S, C, Cv, da_part, n_da, dalpha);
  });
  CTSEG_LAUNCH_CHECK("batchnorm_prelu_bwd_apply");
  return 0;
}
