// Loss / metric kernels for the reference's 3-D training step (gfx950, HBM-bound, one voxel per lane):
//   ctseg_squash_masks  : _squash_masks_3D (capstone/volumetric/utils.py:4-7)
//   ctseg_seg_loss      : F.cross_entropy [+ class weights] (capstone/models/losses.py:45-68), softmax -> argmax
//                         (capstone/training/utils.py:19-20), the integer counts behind compute_meandice
//                         (capstone/models/temp.py:173-214), soft-Dice / focal sums (monai DiceLoss, FocalLoss as
//                         configured at capstone/volumetric/losses.py:72-77,107) and d(loss)/d(logits).
// The reference materialises softmax, two 1 GB one-hots and their product; here one pass reads the logits
// once, keeps everything in registers and reduces with wave shuffles -> per-workgroup fp64 partials
// (summed later in fixed order: deterministic) and exact int64 counts.  The per-voxel pieces of that pass live in
// loss_common.h, which the two-target pass of mixup.hip shares.
#include "loss_common.h"

namespace ctseg {

// PRESENT: also present[b][k] |= any(masks[b][k] == 1), from the same read (weighted_mixup's structure indicator, capstone/training/
// utils.py:27: per RAW mask — a structure wholly covered by a higher-numbered one is absent from the squashed labels' histogram)
template <bool PRESENT>
__global__ __launch_bounds__(256) void squash_masks_kernel(const uint8_t* __restrict__ masks, int K, int64_t S,
                                                           uint8_t* __restrict__ labels, int64_t* __restrict__ labels_i64,
                                                           unsigned long long* __restrict__ hist, int* __restrict__ present) {
  __shared__ unsigned int s_h[32];
  __shared__ unsigned int s_pres;
  const int b = blockIdx.y;
  if (threadIdx.x < 32) s_h[threadIdx.x] = 0;
  if (PRESENT && threadIdx.x == 0) s_pres = 0u;
  unsigned int pres = 0u;                      // bit k: this thread saw masks[b][k] == 1
  __syncthreads();
  const uint8_t* mb = masks + (int64_t)b * K * S;
  int bg = 0;
  const bool vec = (S % 16 == 0) && (((uintptr_t)masks % 16) == 0) && (((uintptr_t)labels % 16) == 0);
  const int64_t nchunk = (S + 15) / 16;
  for (int64_t ch = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; ch < nchunk; ch += (int64_t)gridDim.x * blockDim.x) {
    const int64_t v0 = ch * 16;
    int lab[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) lab[i] = 0;
    if (vec) {
      for (int k = 0; k < K; ++k) {
        const u32x4 m = *reinterpret_cast<const u32x4*>(mb + (int64_t)k * S + v0);
        if constexpr (PRESENT) {
          unsigned int hit = 0u;               // a zero byte of (word ^ 0x01010101) is a mask byte equal to 1
#pragma unroll
          for (int w = 0; w < 4; ++w) { const uint32_t z = m[w] ^ 0x01010101u; hit |= (z - 0x01010101u) & ~z & 0x80808080u; }
          if (hit) pres |= 1u << k;
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int val = (int)((m[i >> 2] >> (8 * (i & 3))) & 0xffu) * (k + 1);
          lab[i] = val > lab[i] ? val : lab[i];
        }
      }
      u32x4 o;
#pragma unroll
      for (int w = 0; w < 4; ++w)
        o[w] = (uint32_t)(lab[4 * w] & 0xff) | ((uint32_t)(lab[4 * w + 1] & 0xff) << 8) | ((uint32_t)(lab[4 * w + 2] & 0xff) << 16) |
               ((uint32_t)(lab[4 * w + 3] & 0xff) << 24);
      *reinterpret_cast<u32x4*>(labels + (int64_t)b * S + v0) = o;
    } else {
      for (int i = 0; i < 16; ++i) {
        if (v0 + i >= S) break;
        int l = 0;
        for (int k = 0; k < K; ++k) {
          const int mv = (int)mb[(int64_t)k * S + v0 + i];
          if (PRESENT && mv == 1) pres |= 1u << k;
          const int val = mv * (k + 1);
          l = val > l ? val : l;
        }
        lab[i] = l;
        labels[(int64_t)b * S + v0 + i] = (uint8_t)l;
      }
    }
    // histogram: background is ~99 % of a CT volume, and 64 lanes adding to ONE LDS word serialise — count it per thread
    int nbg = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      if (v0 + i < S) {
        if (labels_i64 != nullptr) labels_i64[(int64_t)b * S + v0 + i] = lab[i];
        if (lab[i] == 0) ++nbg;
        else if (lab[i] <= K) atomicAdd(&s_h[lab[i]], 1u);
      }
    }
    bg += nbg;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) bg += __shfl_xor(bg, o, 64);
  if ((threadIdx.x & 63) == 0 && bg) atomicAdd(&s_h[0], (unsigned)bg);
  __syncthreads();
  if (threadIdx.x <= K && hist != nullptr && s_h[threadIdx.x] != 0)
    atomicAdd(&hist[(int64_t)b * (K + 1) + threadIdx.x], (unsigned long long)s_h[threadIdx.x]);
  if constexpr (PRESENT) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) pres |= __shfl_xor(pres, o, 64);
    if ((threadIdx.x & 63) == 0 && pres) atomicOr(&s_pres, pres);
    __syncthreads();
    if (threadIdx.x < K && ((s_pres >> threadIdx.x) & 1u)) atomicOr(&present[(int64_t)b * K + threadIdx.x], 1);
  }
}

// One pass over fp32 channels-last logits.  Block (p, b) covers voxels [p*vp, (p+1)*vp) of sample b.
// SOFT = false: cross-entropy-only fast path (the reference's 3-D default): no soft-Dice / focal sums, CE-only gradient
// CP = extent of the per-class register arrays (12 when C <= 12 — the reference's 10 classes — else 16): fewer live registers,
// more waves per SIMD for this latency-bound streaming pass
template <typename GT, bool SOFT, int CP>
__global__ __launch_bounds__(256) void seg_loss_kernel(const float* __restrict__ logits, int ld, const uint8_t* __restrict__ labels,
                                                       int64_t S, int C, const float* __restrict__ class_weight, int do_stats,
                                                       double* __restrict__ part, int P, unsigned long long* __restrict__ cnt,
                                                       int do_grad, const float* __restrict__ coef, char* __restrict__ dlogits,
                                                       int g_ld, uint8_t* __restrict__ pred_out) {
  __shared__ float s_coef[1 + 3 * CMAX];
  __shared__ float s_cw[CMAX];
  __shared__ double s_part[4][LOSS_RM];
  __shared__ unsigned int s_cnt[3 * CMAX];
  const int p = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  init_tables<1>(tid, C, class_weight, s_cw, s_coef, s_cnt);
  __syncthreads();
  if (do_grad && tid < 1 + 3 * C) fill_coef_row(s_coef, coef + (int64_t)b * (1 + 3 * C), tid, C);
  __syncthreads();
  const int64_t vp = (S + P - 1) / P;
  const int64_t v0 = p * vp, v1 = (v0 + vp < S) ? v0 + vp : S;
  const int nld4 = ld / 4;

  float a_ce = 0.f, a_w = 0.f;
  float a_p[CP], a_py[CP], a_fo[CP];
  unsigned int c_in[CP], c_pr[CP], c_tr[CP];
#pragma unroll
  for (int c = 0; c < CP; ++c) { a_p[c] = a_py[c] = a_fo[c] = 0.f; c_in[c] = c_pr[c] = c_tr[c] = 0u; }

  for (int64_t v = v0 + tid; v < v1; v += 256) {
    const int64_t vox = (int64_t)b * S + v;
    float x[CP];
    load_logits_row<CP>(logits + vox * ld, nld4, x);
    const int t = (int)labels[vox];
    // spelled out here and in seg_loss_pair_kernel (mixup.hip), the same text: as an inlined helper it changed both kernels' VGPR counts
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
    float xt, pt;
    target_terms<CP>(x, pr, t, xt, pt);
    const float logpt = (xt - m) - ls;
    const float w = s_cw[t < CMAX ? t : 0];
    if (pred_out != nullptr) pred_out[vox] = (uint8_t)pred;
    if (do_stats) {
      a_ce += w * (ls + (m - xt));
      a_w += w;
      const float om = 1.f - pt;
      const float fo = -om * om * logpt;
#pragma unroll
      for (int c = 0; c < CP; ++c) {
        if (c < C) {
          if (SOFT) a_p[c] += pr[c];
          if (c == t) { if (SOFT) { a_py[c] += pr[c]; a_fo[c] += fo; } c_tr[c] += 1u; }
          if (c == pred) { c_pr[c] += 1u; if (c == t) c_in[c] += 1u; }
        }
      }
    }
    if (do_grad) {
      const float ce_scale = s_coef[0] * w;
      float d[CMAX];
#pragma unroll
      for (int c = CP; c < CMAX; ++c) d[c] = 0.f;
      if constexpr (SOFT) {
        // soft-Dice: dL/dp_c = a_c*[c==t] + b_c ; through softmax: p_k (g_k - sum_j g_j p_j).  Spelled out here and in
        // seg_loss_pair_kernel, the same expressions: as an inlined helper it changed both kernels' VGPR counts
        float gk[CP], dot = 0.f;
#pragma unroll
        for (int c = 0; c < CP; ++c) {
          gk[c] = (c < C) ? (s_coef[1 + CMAX + c] + (c == t ? s_coef[1 + c] : 0.f)) : 0.f;
          dot += gk[c] * pr[c];
        }
        const float ft = s_coef[1 + 2 * CMAX + (t < CMAX ? t : 0)];
        const float om = 1.f - pt;
        const float fterm = ft * (2.f * om * pt * logpt - om * om);
#pragma unroll
        for (int c = 0; c < CP; ++c) {
          const float ind = (c == t) ? 1.f : 0.f;
          d[c] = (c < C) ? (ce_scale * (pr[c] - ind) + pr[c] * (gk[c] - dot) + fterm * (ind - pr[c])) : 0.f;
        }
      } else {
#pragma unroll
        for (int c = 0; c < CP; ++c) d[c] = (c < C) ? ce_scale * (pr[c] - ((c == t) ? 1.f : 0.f)) : 0.f;
      }
      store_grad_row<GT, CP>(dlogits + vox * g_ld * TT<GT>::SZ, g_ld, d);
    }
  }

  if (do_stats) {
    // wave shuffle reduction (fp64) -> LDS -> one partial record per workgroup
    double rec[LOSS_RM];
    rec[0] = a_ce; rec[1] = a_w;
#pragma unroll
    for (int c = 0; c < CMAX; ++c) {
      rec[2 + c] = c < CP ? a_p[c < CP ? c : 0] : 0.f;
      rec[2 + CMAX + c] = c < CP ? a_py[c < CP ? c : 0] : 0.f;
      rec[2 + 2 * CMAX + c] = c < CP ? a_fo[c < CP ? c : 0] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < LOSS_RM; ++i) {
      double s = 0.0;
      if (SOFT || i < 2) s = wave_sum(rec[i]);
      if (lane == 0) s_part[wave][i] = s;
    }
#pragma unroll
    for (int c = 0; c < CP; ++c) {
      const unsigned int a = wave_count(c_in[c]), bq = wave_count(c_pr[c]), cq = wave_count(c_tr[c]);
      if (lane == 0 && c < C) {
        if (a) atomicAdd(&s_cnt[c], a);
        if (bq) atomicAdd(&s_cnt[CMAX + c], bq);
        if (cq) atomicAdd(&s_cnt[2 * CMAX + c], cq);
      }
    }
    __syncthreads();
    flush_records<1>(tid, b, p, P, C, &s_part[0][0], s_cnt, part, cnt);
  }
}

// Dice counts from two label maps (DiceMetricWrapper called on already-squashed predictions)
__global__ __launch_bounds__(256) void dice_counts_kernel(const uint8_t* __restrict__ pred, const uint8_t* __restrict__ truth,
                                                          int64_t S, int C, unsigned long long* __restrict__ cnt) {
  __shared__ unsigned int s_cnt[3 * CMAX];
  const int b = blockIdx.y;
  if (threadIdx.x < 3 * CMAX) s_cnt[threadIdx.x] = 0u;
  __syncthreads();
  for (int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; v < S; v += (int64_t)gridDim.x * blockDim.x) {
    const int p = pred[(int64_t)b * S + v], t = truth[(int64_t)b * S + v];
    if (p < C) atomicAdd(&s_cnt[CMAX + p], 1u);
    if (t < C) atomicAdd(&s_cnt[2 * CMAX + t], 1u);
    if (p == t && p < C) atomicAdd(&s_cnt[p], 1u);
  }
  __syncthreads();
  if (threadIdx.x < 3 * C) {
    const int k = threadIdx.x / C, c = threadIdx.x % C;
    const unsigned int v = s_cnt[k * CMAX + c];
    if (v) atomicAdd(&cnt[((int64_t)b * 3 + k) * C + c], (unsigned long long)v);
  }
}

// part [B][P][R] -> out [B][R]; one block per (record entry r, b): 256 strided sub-sums over P, combined in fixed order
__global__ __launch_bounds__(256) void reduce_partials_f64_kernel(const double* __restrict__ part, int P, int R,
                                                                  double* __restrict__ out) {
  __shared__ double s[256];
  const int r = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
  double a = 0.0;
  for (int p = t; p < P; p += 256) a += part[((int64_t)b * P + p) * R + r];
  s[t] = a;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {          // fixed pairing => deterministic
    if (t < w) s[t] += s[t + w];
    __syncthreads();
  }
  if (t == 0) out[(int64_t)b * R + r] = s[0];
}

// The scalar bookkeeping of a cross-entropy training step in ONE launch instead of ~20 scalar-sized torch kernels:
// out[0] = sum_b red[b][0] / sum_b red[b][1] (mean cross-entropy), out[2 + k] = Dice of foreground class k+1 averaged over the
// samples whose ground truth holds it ("mean_batch" with NaN for an empty truth, capstone/models/metrics.py:15-31), 0 when
// no sample does; out[1] = their mean over the C-1 foreground classes.  fp32 arithmetic in the order of the torch expressions.
__global__ __launch_bounds__(64) void loss_dice_summary_kernel(const double* __restrict__ red, int B, int R,
                                                                 const long long* __restrict__ cnt, int C, float* __restrict__ out) {
  __shared__ float s_pc[CMAX];
  const int t = threadIdx.x;
  if (t < C - 1) {
    const int c = t + 1;
    float sum = 0.f, n_ok = 0.f;
    for (int b = 0; b < B; ++b) {
      const float inter = (float)cnt[((int64_t)b * 3 + 0) * C + c], pred = (float)cnt[((int64_t)b * 3 + 1) * C + c],
                  truth = (float)cnt[((int64_t)b * 3 + 2) * C + c];
      if (truth > 0.f) { sum += 2.0f * inter / (truth + pred); n_ok += 1.f; }
    }
    const float pc = n_ok > 0.f ? sum / n_ok : 0.f;
    s_pc[t] = pc;
    out[2 + t] = pc;
  }
  __syncthreads();
  if (t == 0) {
    double a = 0.0, w = 0.0;
    for (int b = 0; b < B; ++b) { a += red[(int64_t)b * R]; w += red[(int64_t)b * R + 1]; }
    out[0] = (float)(a / w);
    float m = 0.f;
    for (int k = 0; k < C - 1; ++k) m += s_pc[k];
    out[1] = m / (float)(C - 1);
  }
}

}  // namespace ctseg

using namespace ctseg;

extern "C" int ctseg_loss_dice_summary(const double* red, int32_t B, int32_t R, const int64_t* cnt, int32_t C, float* out,
                                       void* stream) {
  CTSEG_REQUIRE(red && cnt && out && B > 0 && R >= 2 && C >= 2 && C <= CMAX, "loss_dice_summary: bad arguments");
  hipLaunchKernelGGL(loss_dice_summary_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, red, B, R, (const long long*)cnt, C, out);
  CTSEG_LAUNCH_CHECK("loss_dice_summary");
  return 0;
}

static int squash_masks_launch(const uint8_t* masks, int32_t B, int32_t K, int64_t S, uint8_t* labels, int64_t* labels_i64,
                               int64_t* hist, int32_t* present, void* stream) {
  const int64_t nchunk = (S + 15) / 16;
  int64_t blocks = (nchunk + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  if (present)
    hipLaunchKernelGGL(squash_masks_kernel<true>, dim3((unsigned)blocks, B), dim3(256), 0, (hipStream_t)stream, masks, K, S, labels,
                       labels_i64, (unsigned long long*)hist, present);
  else
    hipLaunchKernelGGL(squash_masks_kernel<false>, dim3((unsigned)blocks, B), dim3(256), 0, (hipStream_t)stream, masks, K, S, labels,
                       labels_i64, (unsigned long long*)hist, (int*)nullptr);
  return 0;
}

extern "C" int ctseg_squash_masks(const uint8_t* masks, int32_t B, int32_t K, int64_t S, uint8_t* labels, int64_t* labels_i64,
                                  int64_t* hist, void* stream) {
  CTSEG_REQUIRE(masks && labels && B > 0 && K > 0 && K < 32 && S > 0, "squash_masks: bad arguments");
  squash_masks_launch(masks, B, K, S, labels, labels_i64, hist, nullptr, stream);
  CTSEG_LAUNCH_CHECK("squash_masks");
  return 0;
}

extern "C" int ctseg_squash_masks_present(const uint8_t* masks, int32_t B, int32_t K, int64_t S, uint8_t* labels, int64_t* labels_i64,
                                          int64_t* hist, int32_t* present, void* stream) {
  CTSEG_REQUIRE(masks && labels && present && B > 0 && K > 0 && K < 32 && S > 0, "squash_masks_present: bad arguments");
  squash_masks_launch(masks, B, K, S, labels, labels_i64, hist, present, stream);
  CTSEG_LAUNCH_CHECK("squash_masks_present");
  return 0;
}

extern "C" int ctseg_seg_loss(const float* logits, int32_t ld, const uint8_t* labels, int32_t B, int64_t S, int32_t C,
                              const float* class_weight, int32_t do_stats, double* part, int32_t P, int64_t* cnt,
                              int32_t do_grad, const float* coef, void* dlogits, int32_t g_ld, int32_t gdtype, uint8_t* pred_out,
                              void* stream) {
  if (check_loss_args("seg_loss", logits, ld, labels, B, S, C, P, do_stats != 0, part, cnt, do_grad, coef, dlogits, g_ld, gdtype)) return -1;
  const bool lite = (do_stats == 2 || do_stats == 0) && (do_grad == 2 || do_grad == 0);   // cross-entropy only
  const bool gbf = do_grad && gdtype == CTSEG_BF16;
  auto launch = [&](auto gt, auto soft) {
    dispatch_cp(C, ld, [&](auto cp) {
      hipLaunchKernelGGL((seg_loss_kernel<decltype(gt), soft, cp>), dim3(P, B), dim3(256), 0, (hipStream_t)stream, logits, ld, labels, S, C,
                         class_weight, do_stats, part, P, (unsigned long long*)cnt, do_grad, coef, (char*)dlogits, g_ld, pred_out);
    });
  };
  if (gbf) { if (lite) launch(BF16(), std::false_type()); else launch(BF16(), std::true_type()); }
  else { if (lite) launch(float(), std::false_type()); else launch(float(), std::true_type()); }
  CTSEG_LAUNCH_CHECK("seg_loss");
  return 0;
}

extern "C" int ctseg_reduce_partials_f64(const double* part, int32_t B, int32_t P, int32_t R, double* out, void* stream) {
  CTSEG_REQUIRE(part && out && B > 0 && P > 0 && R > 0 && R <= 64, "reduce_partials_f64: bad arguments");
  hipLaunchKernelGGL(reduce_partials_f64_kernel, dim3(R, B), dim3(256), 0, (hipStream_t)stream, part, P, R, out);
  CTSEG_LAUNCH_CHECK("reduce_partials_f64");
  return 0;
}

extern "C" int ctseg_dice_counts(const uint8_t* pred, const uint8_t* truth, int32_t B, int64_t S, int32_t C, int64_t* cnt,
                                 void* stream) {
  CTSEG_REQUIRE(pred && truth && cnt && B > 0 && S > 0 && C >= 2 && C <= CMAX, "dice_counts: bad arguments");
  int64_t blocks = (S + 256 * 16 - 1) / (256 * 16);
  if (blocks > 1024) blocks = 1024;
  hipLaunchKernelGGL(dice_counts_kernel, dim3((unsigned)blocks, B), dim3(256), 0, (hipStream_t)stream, pred, truth, S, C,
                     (unsigned long long*)cnt);
  CTSEG_LAUNCH_CHECK("dice_counts");
  return 0;
}
