// Boundary loss (capstone/models/losses.py:127-157, BoundaryLossWrapper) on gfx950: the third user of loss_common.h.
//   ctseg_boundary_stats : sum_v softmax(x)[c + 1][v] * D[c][v] per (sample, side, foreground class) -> per-workgroup fp64 partials
//   ctseg_boundary_grad  : d/d(logits) of  sum_{b, s, c} bw[b][s][c] * sum_v p[b][c + 1][v] * D_s[b][c][v],  stored or added to a
//                          gradient row that another loss pass wrote
// The logits are the fp32 channels-last rows the other loss passes read; the distance maps are fp32 planes [B][C - 1][S] (no
// background plane), so neighbouring lanes read neighbouring voxels of a plane.  The loss is linear in D: the mixup step's second
// side (the maps of sample perm[b], capstone/training/mixup_trainer.py:70-75) costs one more plane read per class and no second
// softmax.  Both are HBM-bound streaming passes, one voxel per lane, with seg_loss_kernel's thread -> voxel assignment.  A perm
// entry outside [0, B) is clamped: the index lives on the device and no launch may read out of bounds for it.
#include "loss_common.h"

namespace ctseg {

__device__ __forceinline__ int partner_sample(int i, int B) { return i < 0 ? 0 : (i >= B ? B - 1 : i); }

// one rounding of the sum, never contracted with the product behind b: the accumulated row is the stored row plus the value the
// storing variant writes, bit for bit
__device__ __forceinline__ float add_rn(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}

// pr[CP] = softmax of one voxel's logits row, zeros from C on: the expressions of seg_loss_kernel
template <int CP> __device__ __forceinline__ void softmax_row(const float* row, int nld4, int C, float* pr) {
  float x[CP];
  load_logits_row<CP>(row, nld4, x);
  float m = x[0];
#pragma unroll
  for (int c = 1; c < CP; ++c) if (c < C) m = fmaxf(m, x[c]);
  float ssum = 0.f;
#pragma unroll
  for (int c = 0; c < CP; ++c) { pr[c] = (c < C) ? expf(x[c] - m) : 0.f; if (c < C) ssum += pr[c]; }
#pragma unroll
  for (int c = 0; c < CP; ++c) pr[c] = (c < C) ? pr[c] / ssum : 0.f;
}

// Block (p, b) covers voxels [p*vp, (p+1)*vp) of sample b.  part [B][P][NS][C - 1]: the workgroup's sums, the four waves added in
// fixed order; no floating-point atomics, so two runs give the same bits.
template <int CP, int NS>
__global__ __launch_bounds__(256) void boundary_stats_kernel(const float* __restrict__ logits, int ld, const float* __restrict__ maps,
                                                             const int* __restrict__ perm, int B, int64_t S, int C,
                                                             double* __restrict__ part, int P) {
  __shared__ double s_part[4][NS][CMAX];
  const int p = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t vp = (S + P - 1) / P;
  const int64_t v0 = p * vp, v1 = (v0 + vp < S) ? v0 + vp : S;
  const int nld4 = ld / 4;
  const int64_t plane = (int64_t)(C - 1) * S;
  const float* dm[NS];
  dm[0] = maps + (int64_t)b * plane;
  if constexpr (NS > 1) dm[1] = maps + (int64_t)partner_sample(perm[b], B) * plane;

  float acc[NS][CP];                         // acc[s][c]: class c, entry 0 unused (the background has no plane)
#pragma unroll
  for (int s = 0; s < NS; ++s)
#pragma unroll
    for (int c = 0; c < CP; ++c) acc[s][c] = 0.f;

  for (int64_t v = v0 + tid; v < v1; v += 256) {
    float pr[CP];
    softmax_row<CP>(logits + ((int64_t)b * S + v) * ld, nld4, C, pr);
#pragma unroll
    for (int c = 1; c < CP; ++c) {
      if (c < C) {
#pragma unroll
        for (int s = 0; s < NS; ++s) acc[s][c] += pr[c] * dm[s][(int64_t)(c - 1) * S + v];
      }
    }
  }

  // wave shuffle reduction (fp64) -> LDS -> one partial record per workgroup
#pragma unroll
  for (int s = 0; s < NS; ++s) {
#pragma unroll
    for (int c = 1; c < CP; ++c) {
      const double w = wave_sum((double)acc[s][c]);
      if (lane == 0) s_part[wave][s][c] = w;
    }
  }
  __syncthreads();
  const int R = NS * (C - 1);
  if (tid < R) {
    const int s = NS > 1 ? tid / (C - 1) : 0, c = 1 + tid - s * (C - 1);
    part[((int64_t)b * P + p) * R + tid] = s_part[0][s][c] + s_part[1][s][c] + s_part[2][s][c] + s_part[3][s][c];
  }
}

// bw [B][NS][C - 1] = weight of (sample, side, class) in the differentiated scalar, 1 / S and the upstream gradient folded in by the
// caller.  g_0 = 0, g_c = sum_s bw[b][s][c - 1] * D_s[c - 1][v]; d_k = p_k (g_k - sum_j g_j p_j) for every k, the background included.
// ACC = false: the row is stored, zeros in its pad columns.  ACC = true: the row is read, d added in fp32 and stored once; the pad
// columns get back the values read.
template <typename GT, int CP, int NS, bool ACC>
__global__ __launch_bounds__(256) void boundary_grad_kernel(const float* __restrict__ logits, int ld, const float* __restrict__ maps,
                                                            const int* __restrict__ perm, int B, int64_t S, int C,
                                                            const float* __restrict__ bw, int P, char* __restrict__ dlogits, int g_ld) {
  __shared__ float s_bw[NS][CMAX];           // s_bw[s][c]: class c, 0 for the background and from C on
  const int p = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  if (tid < NS * CMAX) {
    const int s = NS > 1 ? tid / CMAX : 0, c = tid - s * CMAX;
    s_bw[s][c] = (c >= 1 && c < C) ? bw[((int64_t)b * NS + s) * (C - 1) + c - 1] : 0.f;
  }
  __syncthreads();
  const int64_t vp = (S + P - 1) / P;
  const int64_t v0 = p * vp, v1 = (v0 + vp < S) ? v0 + vp : S;
  const int nld4 = ld / 4;
  const int64_t plane = (int64_t)(C - 1) * S;
  const float* dm[NS];
  dm[0] = maps + (int64_t)b * plane;
  if constexpr (NS > 1) dm[1] = maps + (int64_t)partner_sample(perm[b], B) * plane;

  for (int64_t v = v0 + tid; v < v1; v += 256) {
    const int64_t vox = (int64_t)b * S + v;
    float pr[CP];
    softmax_row<CP>(logits + vox * ld, nld4, C, pr);
    float gk[CP], dot = 0.f;
    gk[0] = 0.f;
#pragma unroll
    for (int c = 1; c < CP; ++c) {
      float g = 0.f;
      if (c < C) {
        const float w0 = s_bw[0][c], d0 = dm[0][(int64_t)(c - 1) * S + v];
        g = w0 * d0;
        if constexpr (NS > 1) {
          // the two sides may cancel: the first product's rounding error (exact, by an FMA) is added back, so that g is good to a
          // few ulp of g itself and not of its larger term
          const float lo = __builtin_fmaf(w0, d0, -g);
          g = __builtin_fmaf(s_bw[1][c], dm[1][(int64_t)(c - 1) * S + v], g) + lo;
        }
      }
      gk[c] = g;
      dot += g * pr[c];
    }
    float d[CMAX];
#pragma unroll
    for (int c = 0; c < CMAX; ++c) d[c] = 0.f;
#pragma unroll
    for (int c = 0; c < CP; ++c) d[c] = pr[c] * (gk[c] - dot);      // pr is 0 from C on
    char* gp = dlogits + vox * g_ld * TT<GT>::SZ;
    if constexpr (ACC) {
      float old[CMAX];
      load_grad_row<GT, CP>(gp, g_ld, old);
#pragma unroll
      for (int c = 0; c < CMAX; ++c) d[c] = (c < C) ? add_rn(old[c], d[c]) : old[c];
    }
    store_grad_row<GT, CP>(gp, g_ld, d);
  }
}

}  // namespace ctseg

using namespace ctseg;

// the arguments both entry points share: check_loss_args's rules for the logits rows, fp32 planes for the maps
static int check_boundary_args(const char* name, const float* logits, int ld, const float* maps, int B, int64_t S, int C, int P) {
  CTSEG_REQUIRE(logits && maps && B > 0 && B <= 65535 && S > 0 && C >= 2 && C <= CMAX, "%s: bad arguments (C <= 16)", name);
  CTSEG_REQUIRE(ld % 4 == 0 && ld >= C && ld <= CMAX && ((uintptr_t)logits % 16) == 0, "%s: logits stride %d", name, ld);
  CTSEG_REQUIRE(((uintptr_t)maps % 4) == 0, "%s: unaligned fp32 maps", name);
  CTSEG_REQUIRE(P > 0, "%s: P = %d", name, P);
  return 0;
}

extern "C" int ctseg_boundary_stats(const float* logits, int32_t ld, const float* maps, const int32_t* perm, int32_t B, int64_t S,
                                    int32_t C, double* part, int32_t P, void* stream) {
  if (check_boundary_args("boundary_stats", logits, ld, maps, B, S, C, P)) return -1;
  CTSEG_REQUIRE(part, "boundary_stats: stats buffers");
  dispatch_cp(C, ld, [&](auto cp) {
    if (perm)
      hipLaunchKernelGGL((boundary_stats_kernel<cp, 2>), dim3(P, B), dim3(256), 0, (hipStream_t)stream, logits, ld, maps, perm, B, S, C,
                         part, P);
    else
      hipLaunchKernelGGL((boundary_stats_kernel<cp, 1>), dim3(P, B), dim3(256), 0, (hipStream_t)stream, logits, ld, maps, perm, B, S, C,
                         part, P);
  });
  CTSEG_LAUNCH_CHECK("boundary_stats");
  return 0;
}

extern "C" int ctseg_boundary_grad(const float* logits, int32_t ld, const float* maps, const int32_t* perm, int32_t B, int64_t S,
                                   int32_t C, const float* bw, int32_t P, void* dlogits, int32_t g_ld, int32_t gdtype,
                                   int32_t accumulate, void* stream) {
  if (check_boundary_args("boundary_grad", logits, ld, maps, B, S, C, P)) return -1;
  CTSEG_REQUIRE(bw && dlogits && (gdtype == CTSEG_F32 || gdtype == CTSEG_BF16), "boundary_grad: grad buffers");
  // bf16 gradients: 16-byte chunked rows, or 12 wide (8-byte pieces) for the <= 12 class case
  CTSEG_REQUIRE(g_ld % 4 == 0 && (gdtype == CTSEG_F32 || g_ld % 8 == 0 || g_ld == 12) && g_ld >= C && g_ld <= CMAX &&
                    ((uintptr_t)dlogits % 16) == 0,
                "boundary_grad: dlogits stride %d", g_ld);
  auto launch = [&](auto gt, auto ns, auto acc) {
    dispatch_cp(C, ld, [&](auto cp) {
      hipLaunchKernelGGL((boundary_grad_kernel<decltype(gt), cp, ns, acc>), dim3(P, B), dim3(256), 0, (hipStream_t)stream, logits, ld, maps,
                         perm, B, S, C, bw, P, (char*)dlogits, g_ld);
    });
  };
  auto with_ns = [&](auto gt, auto acc) {
    if (perm) launch(gt, std::integral_constant<int, 2>(), acc);
    else launch(gt, std::integral_constant<int, 1>(), acc);
  };
  auto with_acc = [&](auto gt) {
    if (accumulate) with_ns(gt, std::true_type());
    else with_ns(gt, std::false_type());
  };
  if (gdtype == CTSEG_BF16) with_acc(BF16());
  else with_acc(float());
  CTSEG_LAUNCH_CHECK("boundary_grad");
  return 0;
}
