// Mixup training (capstone/training/utils.py:23-56, capstone/training/mixup_trainer.py:52-92) on gfx950:
//   ctseg_mixup_images  : mixup_tensors(images, images[index], lambda) — bit-equal to the torch expression
//   ctseg_seg_loss_pair : the soft path of ctseg_seg_loss (loss_metric.hip) against TWO targets of one prediction, labels[b] and
//                         labels[perm[b]]: the reference calls its loss wrapper twice and sums lambda * a + (1 - lambda) * b.  One
//                         softmax per voxel feeds both sides' sums; the gradient pass writes d_A + d_B once.
// Both are HBM-bound streaming passes, one voxel (or one 16-byte piece) per lane.  A perm entry outside [0, B) is clamped: the
// index lives on the device and no launch may read out of bounds for it.
#include "loss_common.h"

namespace ctseg {

typedef float f32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));   // a 16-byte access at a 4-byte aligned address

__device__ __forceinline__ int clamp_sample(int i, int B) { return i < 0 ? 0 : (i >= B ? B - 1 : i); }

// two roundings of the products, one of the sum, never contracted into an FMA: what torch computes for l0 * x + l1 * y.
// (HIP's __fmul_rn / __fadd_rn are plain operators that -ffp-contract=fast still fuses; the pragma takes the permission away.)
__device__ __forceinline__ float mix2(float l0, float a, float l1, float b) {
#pragma clang fp contract(off)
  const float pa = l0 * a;
  const float pb = l1 * b;
  return pa + pb;
}

// Row b = head (< 4 scalars up to the first 16-byte boundary of x[b] / out[b], which share their alignment), 16-byte pieces, tail
// (< 4 scalars).  The partner row x[perm[b]] starts at another offset when n % 4 != 0: its pieces are 4-byte aligned accesses.
__global__ __launch_bounds__(256) void mixup_images_kernel(const float* __restrict__ x, const int* __restrict__ perm, int B, int64_t n,
                                                           float l0, float l1, float* __restrict__ out) {
  const int b = blockIdx.y;
  const float* xa = x + (int64_t)b * n;
  const float* xb = x + (int64_t)clamp_sample(perm[b], B) * n;
  float* o = out + (int64_t)b * n;
  int64_t head = (int64_t)((16u - (unsigned)((uintptr_t)xa & 15u)) & 15u) / 4;
  if ((((uintptr_t)xa ^ (uintptr_t)o) & 15u) != 0) head = n;       // out and x disagree in alignment: all scalar
  if (head > n) head = n;
  const int64_t nvec = (n - head) / 4;
  const int64_t gtid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, gstride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t j = gtid; j < nvec; j += gstride) {
    const int64_t i = head + 4 * j;
    const f32x4 a = *reinterpret_cast<const f32x4*>(xa + i);
    const f32x4_a4 p = *reinterpret_cast<const f32x4_a4*>(xb + i);
    f32x4 r;
#pragma unroll
    for (int q = 0; q < 4; ++q) r[q] = mix2(l0, a[q], l1, p[q]);
    *reinterpret_cast<f32x4*>(o + i) = r;
  }
  const int64_t tail0 = head + 4 * nvec;
  for (int64_t i = gtid; i < head + (n - tail0); i += gstride) {
    const int64_t e = i < head ? i : tail0 + (i - head);
    o[e] = mix2(l0, xa[e], l1, xb[e]);
  }
}

// The per-voxel functions of seg_loss_kernel<GT, true, CP> (loss_common.h; softmax and the soft gradient: the same text, see
// there), its thread -> voxel assignment and its summation order: the counts of each side equal a single-target run's exactly
// and its sums agree to the last bits.
// GRAD = false: statistics.  part [B][P][2][R] (R = 2 + 3C, each side laid out as seg_loss_kernel's record), cnt [B][2][3][C].
// GRAD = true : dlogits = d_A + d_B, each term seg_loss_kernel's formula with its own coef row [b][side] and class weights [side].
template <typename GT, int CP, bool GRAD>
__global__ __launch_bounds__(256) void seg_loss_pair_kernel(const float* __restrict__ logits, int ld, const uint8_t* __restrict__ labels,
                                                            const int* __restrict__ perm, int B, int64_t S, int C,
                                                            const float* __restrict__ class_weight, double* __restrict__ part, int P,
                                                            unsigned long long* __restrict__ cnt, const float* __restrict__ coef,
                                                            char* __restrict__ dlogits, int g_ld) {
  __shared__ float s_coef[2][1 + 3 * CMAX];
  __shared__ float s_cw[2][CMAX];
  __shared__ double s_part[GRAD ? 1 : 4][2][LOSS_RM];
  __shared__ unsigned int s_cnt[2][3 * CMAX];
  const int p = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  init_tables<2>(tid, C, class_weight, &s_cw[0][0], &s_coef[0][0], &s_cnt[0][0]);
  __syncthreads();
  if (GRAD && tid < 2 * (1 + 3 * C)) {
    const int s = tid / (1 + 3 * C);
    fill_coef_row(s_coef[s], coef + ((int64_t)b * 2 + s) * (1 + 3 * C), tid % (1 + 3 * C), C);
  }
  __syncthreads();
  const int64_t vp = (S + P - 1) / P;
  const int64_t v0 = p * vp, v1 = (v0 + vp < S) ? v0 + vp : S;
  const int nld4 = ld / 4;
  const uint8_t* lab_a = labels + (int64_t)b * S;
  const uint8_t* lab_b = labels + (int64_t)clamp_sample(perm[b], B) * S;

  float a_ce[2] = {0.f, 0.f}, a_w[2] = {0.f, 0.f};
  float a_p[CP], a_py[2][CP], a_fo[2][CP];
  unsigned int c_pr[CP], c_in[2][CP], c_tr[2][CP];
#pragma unroll
  for (int c = 0; c < CP; ++c) {
    a_p[c] = 0.f; c_pr[c] = 0u;
#pragma unroll
    for (int s = 0; s < 2; ++s) { a_py[s][c] = a_fo[s][c] = 0.f; c_in[s][c] = c_tr[s][c] = 0u; }
  }

  for (int64_t v = v0 + tid; v < v1; v += 256) {
    const int64_t vox = (int64_t)b * S + v;
    float x[CP];
    load_logits_row<CP>(logits + vox * ld, nld4, x);
    const int tt[2] = {(int)lab_a[v], (int)lab_b[v]};
    // spelled out here and in seg_loss_kernel (loss_metric.hip), the same text: as an inlined helper it changed both kernels' VGPR counts
    float m = x[0];
#pragma unroll
    for (int c = 1; c < CP; ++c) if (c < C) m = fmaxf(m, x[c]);
    float e[CP], ssum = 0.f;
#pragma unroll
    for (int c = 0; c < CP; ++c) { e[c] = (c < C) ? expf(x[c] - m) : 0.f; if (c < C) ssum += e[c]; }
    // softmax THEN argmax, first maximal index (capstone/training/utils.py:19-20)
    float pr[CP], best = -1.f;
    int pred = 0;
#pragma unroll
    for (int c = 0; c < CP; ++c) {
      pr[c] = (c < C) ? e[c] / ssum : 0.f;
      if (c < C && pr[c] > best) { best = pr[c]; pred = c; }
    }
    // cross-entropy as log(sum) + (m - x_t), log p_t as (x_t - m) - log(sum): m + log(sum) would be rounded at the magnitude of m
    // before the subtraction cancels it (confident voxels, a shifted head bias)
    const float ls = logf(ssum);
    if constexpr (!GRAD) {
#pragma unroll
      for (int c = 0; c < CP; ++c) {
        if (c < C) { a_p[c] += pr[c]; if (c == pred) c_pr[c] += 1u; }
      }
    }
    float d[CMAX];
#pragma unroll
    for (int c = 0; c < CMAX; ++c) d[c] = 0.f;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int t = tt[s];
      float xt, pt;
      target_terms<CP>(x, pr, t, xt, pt);
      const float logpt = (xt - m) - ls;
      const float w = s_cw[s][t < CMAX ? t : 0];
      const float om = 1.f - pt;
      if constexpr (!GRAD) {
        a_ce[s] += w * (ls + (m - xt));
        a_w[s] += w;
        const float fo = -om * om * logpt;
#pragma unroll
        for (int c = 0; c < CP; ++c) {
          if (c < C && c == t) {
            a_py[s][c] += pr[c]; a_fo[s][c] += fo; c_tr[s][c] += 1u;
            if (c == pred) c_in[s][c] += 1u;
          }
        }
      } else {
        const float ce_scale = s_coef[s][0] * w;
        // soft-Dice: dL/dp_c = a_c*[c==t] + b_c ; through softmax: p_k (g_k - sum_j g_j p_j).  Spelled out here and in
        // seg_loss_kernel, the same expressions: as an inlined helper it changed both kernels' VGPR counts
        float gk[CP], dot = 0.f;
#pragma unroll
        for (int c = 0; c < CP; ++c) {
          gk[c] = (c < C) ? (s_coef[s][1 + CMAX + c] + (c == t ? s_coef[s][1 + c] : 0.f)) : 0.f;
          dot += gk[c] * pr[c];
        }
        const float ft = s_coef[s][1 + 2 * CMAX + (t < CMAX ? t : 0)];
        const float fterm = ft * (2.f * om * pt * logpt - om * om);
#pragma unroll
        for (int c = 0; c < CP; ++c) {
          const float ind = (c == t) ? 1.f : 0.f;
          const float ds = (c < C) ? (ce_scale * (pr[c] - ind) + pr[c] * (gk[c] - dot) + fterm * (ind - pr[c])) : 0.f;
          d[c] = s == 0 ? ds : d[c] + ds;
        }
      }
    }
    if constexpr (GRAD) store_grad_row<GT, CP>(dlogits + vox * g_ld * TT<GT>::SZ, g_ld, d);
  }

  if constexpr (!GRAD) {
    // wave shuffle reduction (fp64) -> LDS -> one partial record per workgroup and side; sum p goes to both sides
    {
      const double sa = wave_sum((double)a_ce[0]), sb = wave_sum((double)a_ce[1]);
      const double wa = wave_sum((double)a_w[0]), wb = wave_sum((double)a_w[1]);
      if (lane == 0) { s_part[wave][0][0] = sa; s_part[wave][1][0] = sb; s_part[wave][0][1] = wa; s_part[wave][1][1] = wb; }
    }
#pragma unroll
    for (int c = 0; c < CMAX; ++c) {
      const double sp = c < CP ? wave_sum((double)a_p[c < CP ? c : 0]) : 0.0;
      if (lane == 0) s_part[wave][0][2 + c] = s_part[wave][1][2 + c] = sp;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const double spy = c < CP ? wave_sum((double)a_py[s][c < CP ? c : 0]) : 0.0;
        const double sfo = c < CP ? wave_sum((double)a_fo[s][c < CP ? c : 0]) : 0.0;
        if (lane == 0) { s_part[wave][s][2 + CMAX + c] = spy; s_part[wave][s][2 + 2 * CMAX + c] = sfo; }
      }
    }
#pragma unroll
    for (int c = 0; c < CP; ++c) {
      const unsigned int bq = wave_count(c_pr[c]), a0 = wave_count(c_in[0][c]), a1 = wave_count(c_in[1][c]),
                         t0 = wave_count(c_tr[0][c]), t1 = wave_count(c_tr[1][c]);
      if (lane == 0 && c < C) {
        if (a0) atomicAdd(&s_cnt[0][c], a0);
        if (a1) atomicAdd(&s_cnt[1][c], a1);
        if (bq) { atomicAdd(&s_cnt[0][CMAX + c], bq); atomicAdd(&s_cnt[1][CMAX + c], bq); }   // one predicted class per voxel
        if (t0) atomicAdd(&s_cnt[0][2 * CMAX + c], t0);
        if (t1) atomicAdd(&s_cnt[1][2 * CMAX + c], t1);
      }
    }
    __syncthreads();
    flush_records<2>(tid, b, p, P, C, &s_part[0][0][0], &s_cnt[0][0], part, cnt);
  }
}

}  // namespace ctseg

using namespace ctseg;

extern "C" int ctseg_mixup_images(const float* x, const int32_t* perm, int32_t B, int64_t n, double lambda, float* out, void* stream) {
  CTSEG_REQUIRE(x && perm && out && B > 0 && n > 0, "mixup_images: bad arguments");
  CTSEG_REQUIRE(((uintptr_t)x % 4) == 0 && ((uintptr_t)out % 4) == 0, "mixup_images: unaligned fp32 pointer");
  CTSEG_REQUIRE(out + (int64_t)B * n <= x || x + (int64_t)B * n <= out, "mixup_images: out must not alias x");
  int64_t blocks = ((n + 3) / 4 + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  // the two factors as torch forms them from the Python float: (float)lambda and (float)(1 - lambda), the difference in double
  hipLaunchKernelGGL(mixup_images_kernel, dim3((unsigned)blocks, B), dim3(256), 0, (hipStream_t)stream, x, perm, B, n, (float)lambda,
                     (float)(1.0 - lambda), out);
  CTSEG_LAUNCH_CHECK("mixup_images");
  return 0;
}

extern "C" int ctseg_seg_loss_pair(const float* logits, int32_t ld, const uint8_t* labels, const int32_t* perm, int32_t B, int64_t S,
                                   int32_t C, const float* class_weight, int32_t do_grad, double* part, int32_t P, int64_t* cnt,
                                   const float* coef, void* dlogits, int32_t g_ld, int32_t gdtype, void* stream) {
  CTSEG_REQUIRE(perm, "seg_loss_pair: bad arguments (C <= 16)");
  if (check_loss_args("seg_loss_pair", logits, ld, labels, B, S, C, P, !do_grad, part, cnt, do_grad, coef, dlogits, g_ld, gdtype)) return -1;
  auto launch = [&](auto gt, auto grad) {
    dispatch_cp(C, ld, [&](auto cp) {
      hipLaunchKernelGGL((seg_loss_pair_kernel<decltype(gt), cp, grad>), dim3(P, B), dim3(256), 0, (hipStream_t)stream, logits, ld, labels,
                         perm, B, S, C, class_weight, part, P, (unsigned long long*)cnt, coef, (char*)dlogits, g_ld);
    });
  };
  if (!do_grad) launch(float(), std::false_type());
  else if (gdtype == CTSEG_BF16) launch(BF16(), std::true_type());
  else launch(float(), std::true_type());
  CTSEG_LAUNCH_CHECK("seg_loss_pair");
  return 0;
}
