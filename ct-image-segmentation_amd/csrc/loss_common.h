// Shared pieces of the loss passes over fp32 channels-last logits: seg_loss_kernel (loss_metric.hip, one target) and
// seg_loss_pair_kernel (mixup.hip, two targets of one prediction).  The padded LDS tables, the logits row load, the target's terms,
// the gradient row store, the counts' wave sum and the record / count flush exist here once, plus the host-side argument checks and
// the CP dispatch of both entry points.  Two pieces stay spelled out in both kernels, softmax -> argmax and one side's soft
// gradient: as inlined helpers they changed the kernels' register counts (see the comments there).  (The fused cross-entropy
// epilogue of conv_halo_x.hip is a different formulation on purpose and shares nothing with this.)  The Boundary loss passes
// (boundary_loss.hip) are a third user: the logits row load, the gradient row store and its counterpart load_grad_row, the CP dispatch.
#pragma once
#include <type_traits>

#include "ctseg_dev.h"

namespace ctseg {

constexpr int CMAX = 16;              // most classes; every per-class LDS table is padded to it
constexpr int LOSS_RM = 2 + 3 * CMAX; // a padded partial record: (ce, weight, p[CMAX], p_target[CMAX], focal[CMAX])

// Entry i of a row (LEAD scalars, then tables of C) -> its place in the row with the tables padded to CMAX: coefficient rows
// (ce_scale, a[C], b[C], f[C]) have LEAD = 1, partial records LEAD = 2.
template <int LEAD> __device__ __forceinline__ int padded_index(int i, int C) {
  return i < LEAD ? i : LEAD + (i - LEAD) / C * CMAX + (i - LEAD) % C;
}

// Before the first barrier: class weights of NS sides (class_weight [NS][C], or 1) -> s_cw [NS][CMAX]; s_coef [NS][1 + 3 CMAX] and
// s_cnt [NS][3 CMAX] zeroed.
template <int NS>
__device__ __forceinline__ void init_tables(int tid, int C, const float* class_weight, float* s_cw, float* s_coef,
                                            unsigned int* s_cnt) {
  if (tid < NS * CMAX) {
    const int s = NS > 1 ? tid / CMAX : 0, c = tid - s * CMAX;
    s_cw[tid] = (class_weight != nullptr && c < C) ? class_weight[s * C + c] : 1.f;
  }
  if (tid < NS * (1 + 3 * CMAX)) s_coef[tid] = 0.f;
  if (tid < NS * 3 * CMAX) s_cnt[tid] = 0u;
}

// Between the barriers: thread i < 1 + 3 C copies entry i of one coefficient row (ce_scale, a[C], b[C], f[C]) to its padded LDS row
__device__ __forceinline__ void fill_coef_row(float* s_row, const float* row, int i, int C) {
  s_row[padded_index<1>(i, C)] = row[i];
}

// x[CP] = one voxel's logits row of nld4 16-byte pieces, zeros beyond
template <int CP> __device__ __forceinline__ void load_logits_row(const float* row, int nld4, float* x) {
  const f32x4* lp = reinterpret_cast<const f32x4*>(row);
#pragma unroll
  for (int q = 0; q < CP / 4; ++q) {
    f32x4 t = {0.f, 0.f, 0.f, 0.f};
    if (q < nld4) t = lp[q];
    x[4 * q] = t[0]; x[4 * q + 1] = t[1]; x[4 * q + 2] = t[2]; x[4 * q + 3] = t[3];
  }
}

// logit and probability of the label t (0 for a label outside the row)
template <int CP> __device__ __forceinline__ void target_terms(const float* x, const float* pr, int t, float& xt, float& pt) {
  xt = 0.f; pt = 0.f;
#pragma unroll
  for (int c = 0; c < CP; ++c) {
    // selects of values already read: as a chain of `if (c == t)` this helper compiles to a switch over t before it is inlined
    const float xc = x[c], pc = pr[c];
    xt = c == t ? xc : xt; pt = c == t ? pc : pt;
  }
}

// d[CMAX] (zeros from CP on) -> one gradient row of g_ld elements at gp
template <typename GT, int CP> __device__ __forceinline__ void store_grad_row(char* gp, int g_ld, const float* d) {
  constexpr int GSZ = TT<GT>::SZ, GEPC = TT<GT>::EPC;
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

// store_grad_row's counterpart: one gradient row of g_ld elements at gp -> o[CMAX], zeros beyond the row (a pass that adds to a
// row another pass wrote, boundary_loss.hip)
template <typename GT, int CP> __device__ __forceinline__ void load_grad_row(const char* gp, int g_ld, float* o) {
  constexpr int GSZ = TT<GT>::SZ, GEPC = TT<GT>::EPC;
  if (GSZ == 2 && (g_ld & 7) != 0) {
    if constexpr (GSZ == 2) {
#pragma unroll
      for (int u = 0; u < CMAX / 4; ++u) {
        float t[4] = {0.f, 0.f, 0.f, 0.f};
        if (u < CP / 4 && u * 4 < g_ld) load_ep<GT, 4>(gp + u * 8, t);
#pragma unroll
        for (int i = 0; i < 4; ++i) o[u * 4 + i] = t[i];
      }
    }
  } else {
#pragma unroll
    for (int q = 0; q < CMAX / GEPC; ++q) {
      float t[GEPC];
#pragma unroll
      for (int i = 0; i < GEPC; ++i) t[i] = 0.f;
      if (q * GEPC < g_ld) load_chunk<GT>(gp + q * 16, t);
#pragma unroll
      for (int i = 0; i < GEPC; ++i) o[q * GEPC + i] = t[i];
    }
  }
}

// integer wave sum of one per-thread counter.  The kernels take all of a class's sums first and add to LDS afterwards: the
// butterflies of one class then share a basic block and overlap
__device__ __forceinline__ unsigned int wave_count(unsigned int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// After the barrier behind the wave reductions: the workgroup's NS partial records, s_part [4 waves][NS][LOSS_RM] summed over the
// waves in fixed order, -> part [B][P][NS][R = 2 + 3 C], and its counts s_cnt [NS][3][CMAX] -> cnt [B][NS][3][C]
template <int NS>
__device__ __forceinline__ void flush_records(int tid, int b, int p, int P, int C, const double* s_part, const unsigned int* s_cnt,
                                              double* part, unsigned long long* cnt) {
  const int R = 2 + 3 * C;
  if (tid < NS * R) {
    const int s = NS > 1 ? tid / R : 0;
    const double* sp = s_part + s * LOSS_RM + padded_index<2>(tid - s * R, C);
    constexpr int W = NS * LOSS_RM;
    part[((int64_t)b * P + p) * (NS * R) + tid] = sp[0] + sp[W] + sp[2 * W] + sp[3 * W];
  }
  if (tid < NS * 3 * C) {
    const unsigned int v = s_cnt[tid / C * CMAX + tid % C];
    if (v) atomicAdd(&cnt[(int64_t)b * (NS * 3 * C) + tid], (unsigned long long)v);
  }
}

// ---- host side ----------------------------------------------------------------------------------

// The arguments ctseg_seg_loss and ctseg_seg_loss_pair share; `name` is the entry point's, `need_stats` whether this launch
// writes part / cnt
static int check_loss_args(const char* name, const float* logits, int ld, const uint8_t* labels, int B, int64_t S, int C, int P,
                           bool need_stats, const double* part, const int64_t* cnt, int do_grad, const float* coef,
                           const void* dlogits, int g_ld, int gdtype) {
  CTSEG_REQUIRE(logits && labels && B > 0 && S > 0 && C >= 2 && C <= CMAX, "%s: bad arguments (C <= 16)", name);
  CTSEG_REQUIRE(ld % 4 == 0 && ld >= C && ld <= CMAX && ((uintptr_t)logits % 16) == 0, "%s: logits stride %d", name, ld);
  CTSEG_REQUIRE(P > 0 && (!need_stats || (part && cnt)), "%s: stats buffers", name);
  if (do_grad) {
    CTSEG_REQUIRE(coef && dlogits && (gdtype == CTSEG_F32 || gdtype == CTSEG_BF16), "%s: grad buffers", name);
    // bf16 gradients: 16-byte chunked rows, or 12 wide (8-byte pieces) for the <= 12 class case
    CTSEG_REQUIRE(g_ld % 4 == 0 && (gdtype == CTSEG_F32 || g_ld % 8 == 0 || g_ld == 12) && g_ld >= C && g_ld <= CMAX &&
                      ((uintptr_t)dlogits % 16) == 0,
                  "%s: dlogits stride %d", name, g_ld);
  }
  return 0;
}

// f(std::integral_constant<int, CP>()): CP = extent of the kernels' per-class register arrays, 12 when C <= 12 and the rows are 12
// wide (the reference's 10 classes), else 16
template <class F> static inline void dispatch_cp(int C, int ld, F f) {
  if (C <= 12 && ld <= 12) f(std::integral_constant<int, 12>());
  else f(std::integral_constant<int, 16>());
}

}  // namespace ctseg
