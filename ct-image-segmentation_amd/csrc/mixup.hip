// Mixup training (capstone/training/utils.py:23-56, capstone/training/mixup_trainer.py:52-92) on gfx950:
//   ctseg_mixup_images  : mixup_tensors(images, images[index], lambda) — bit-equal to the torch expression
//   ctseg_seg_loss_pair : the soft path of ctseg_seg_loss (loss_metric.hip) against TWO targets of one prediction, labels[b] and
//                         labels[perm[b]]: the reference calls its loss wrapper twice and sums lambda * a + (1 - lambda) * b.  One
//                         softmax per voxel feeds both sides' sums; the gradient pass writes d_A + d_B once.
// Both are HBM-bound streaming passes, one voxel (or one 16-byte piece) per lane.  A perm entry outside [0, B) is clamped: the
// index lives on the device and no launch may read out of bounds for it.
#include "ctseg_dev.h"

namespace ctseg {

constexpr int CMAX = 16;

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

// Per-voxel arithmetic, thread -> voxel assignment and summation order are those of seg_loss_kernel<GT, true, CP>: the counts
// of each side equal a single-target run's exactly and its sums agree to the last bits.
// GRAD = false: statistics.  part [B][P][2][R] (R = 2 + 3C, each side laid out as seg_loss_kernel's record), cnt [B][2][3][C].
// GRAD = true : dlogits = d_A + d_B, each term seg_loss_kernel's formula with its own coef row [b][side] and class weights [side].
template <typename GT, int CP, bool GRAD>
__global__ __launch_bounds__(256) void seg_loss_pair_kernel(const float* __restrict__ logits, int ld, const uint8_t* __restrict__ labels,
                                                            const int* __restrict__ perm, int B, int64_t S, int C,
                                                            const float* __restrict__ class_weight, double* __restrict__ part, int P,
                                                            unsigned long long* __restrict__ cnt, const float* __restrict__ coef,
                                                            char* __restrict__ dlogits, int g_ld) {
  constexpr int GSZ = TT<GT>::SZ, GEPC = TT<GT>::EPC;
  constexpr int RM = 2 + 3 * CMAX;
  __shared__ float s_coef[2][1 + 3 * CMAX];
  __shared__ float s_cw[2][CMAX];
  __shared__ double s_part[GRAD ? 1 : 4][2][RM];
  __shared__ unsigned int s_cnt[2][3 * CMAX];
  const int p = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid < 2 * CMAX) {
    const int s = tid / CMAX, c = tid % CMAX;
    s_cw[s][c] = (class_weight != nullptr && c < C) ? class_weight[s * C + c] : 1.f;
  }
  if (tid < 2 * (1 + 3 * CMAX)) (&s_coef[0][0])[tid] = 0.f;
  if (tid < 2 * 3 * CMAX) (&s_cnt[0][0])[tid] = 0u;
  __syncthreads();
  if (GRAD && tid < 2 * (1 + 3 * C)) {
    // coef[b][side] = (ce_scale, a[C], b[C], f[C]) -> padded to CMAX per table
    const int s = tid / (1 + 3 * C), i = tid % (1 + 3 * C);
    const float v = coef[((int64_t)b * 2 + s) * (1 + 3 * C) + i];
    if (i == 0) s_coef[s][0] = v;
    else { const int t = (i - 1) / C, c = (i - 1) % C; s_coef[s][1 + t * CMAX + c] = v; }
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
    const f32x4* lp = reinterpret_cast<const f32x4*>(logits + vox * ld);
#pragma unroll
    for (int q = 0; q < CP / 4; ++q) {
      f32x4 t = {0.f, 0.f, 0.f, 0.f};
      if (q < nld4) t = lp[q];
      x[4 * q] = t[0]; x[4 * q + 1] = t[1]; x[4 * q + 2] = t[2]; x[4 * q + 3] = t[3];
    }
    const int tt[2] = {(int)lab_a[v], (int)lab_b[v]};
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
    const float lse = m + logf(ssum);
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
      float xt = 0.f, pt = 0.f;
#pragma unroll
      for (int c = 0; c < CP; ++c) if (c == t) { xt = x[c]; pt = pr[c]; }
      const float logpt = xt - lse;
      const float w = s_cw[s][t < CMAX ? t : 0];
      const float om = 1.f - pt;
      if constexpr (!GRAD) {
        a_ce[s] += w * (lse - xt);
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
        // soft-Dice: dL/dp_c = a_c*[c==t] + b_c ; through softmax: p_k (g_k - sum_j g_j p_j)
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
    if constexpr (GRAD) {
      char* gp = dlogits + vox * g_ld * GSZ;
      if (GSZ == 2 && (g_ld & 7) != 0) {
        // bf16 rows 12 wide (24 bytes, 8-byte aligned): 8-byte pieces
        if constexpr (GSZ == 2) {
#pragma unroll
          for (int u = 0; u < CP / 4; ++u)
            if (u * 4 < g_ld) store_ep<GT, 4>(gp + u * 8, d + u * 4);
        }
      } else {
#pragma unroll
        for (int q = 0; q < CMAX / GEPC; ++q)
          if (q * GEPC < g_ld) store_chunk<GT>(gp + q * 16, d + q * GEPC);
      }
    }
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
      unsigned int bq = c_pr[c], a0 = c_in[0][c], a1 = c_in[1][c], t0 = c_tr[0][c], t1 = c_tr[1][c];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        bq += __shfl_xor(bq, o, 64);
        a0 += __shfl_xor(a0, o, 64); a1 += __shfl_xor(a1, o, 64);
        t0 += __shfl_xor(t0, o, 64); t1 += __shfl_xor(t1, o, 64);
      }
      if (lane == 0 && c < C) {
        if (a0) atomicAdd(&s_cnt[0][c], a0);
        if (a1) atomicAdd(&s_cnt[1][c], a1);
        if (bq) { atomicAdd(&s_cnt[0][CMAX + c], bq); atomicAdd(&s_cnt[1][CMAX + c], bq); }
        if (t0) atomicAdd(&s_cnt[0][2 * CMAX + c], t0);
        if (t1) atomicAdd(&s_cnt[1][2 * CMAX + c], t1);
      }
    }
    __syncthreads();
    const int R = 2 + 3 * C;
    if (tid < 2 * R) {
      const int s = tid / R, i = tid % R;
      int src = i;
      if (i >= 2) { const int t = (i - 2) / C, c = (i - 2) % C; src = 2 + t * CMAX + c; }
      const double sum = s_part[0][s][src] + s_part[1][s][src] + s_part[2][s][src] + s_part[3][s][src];
      part[(((int64_t)b * P + p) * 2 + s) * R + i] = sum;
    }
    if (tid < 2 * 3 * C) {
      const int s = tid / (3 * C), t = (tid % (3 * C)) / C, c = tid % C;
      const unsigned int v = s_cnt[s][t * CMAX + c];
      if (v) atomicAdd(&cnt[(((int64_t)b * 2 + s) * 3 + t) * C + c], (unsigned long long)v);
    }
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
  CTSEG_REQUIRE(logits && labels && perm && B > 0 && S > 0 && C >= 2 && C <= CMAX, "seg_loss_pair: bad arguments (C <= 16)");
  CTSEG_REQUIRE(ld % 4 == 0 && ld >= C && ld <= CMAX && ((uintptr_t)logits % 16) == 0, "seg_loss_pair: logits stride %d", ld);
  CTSEG_REQUIRE(P > 0 && (do_grad || (part && cnt)), "seg_loss_pair: stats buffers");
  if (do_grad) {
    CTSEG_REQUIRE(coef && dlogits && (gdtype == CTSEG_F32 || gdtype == CTSEG_BF16), "seg_loss_pair: grad buffers");
    // the row widths of ctseg_seg_loss: 16-byte chunked rows, or bf16 12 wide (8-byte pieces) for the <= 12 class case
    CTSEG_REQUIRE(g_ld % 4 == 0 && (gdtype == CTSEG_F32 || g_ld % 8 == 0 || g_ld == 12) && g_ld >= C && g_ld <= CMAX &&
                      ((uintptr_t)dlogits % 16) == 0,
                  "seg_loss_pair: dlogits stride %d", g_ld);
  }
  hipStream_t st = (hipStream_t)stream;
#define CTSEG_PAIR_LAUNCH2(GT, CP, GRAD)                                                                                           \
  hipLaunchKernelGGL((seg_loss_pair_kernel<GT, CP, GRAD>), dim3(P, B), dim3(256), 0, st, logits, ld, labels, perm, B, S, C, class_weight, \
                     part, P, (unsigned long long*)cnt, coef, (char*)dlogits, g_ld)
#define CTSEG_PAIR_LAUNCH(GT, GRAD)                                       \
  do {                                                                    \
    if (C <= 12 && ld <= 12) CTSEG_PAIR_LAUNCH2(GT, 12, GRAD);            \
    else CTSEG_PAIR_LAUNCH2(GT, 16, GRAD);                                \
  } while (0)
  if (!do_grad) CTSEG_PAIR_LAUNCH(float, false);
  else if (gdtype == CTSEG_BF16) CTSEG_PAIR_LAUNCH(BF16, true);
  else CTSEG_PAIR_LAUNCH(float, true);
#undef CTSEG_PAIR_LAUNCH2
#undef CTSEG_PAIR_LAUNCH
  CTSEG_LAUNCH_CHECK("seg_loss_pair");
  return 0;
}
