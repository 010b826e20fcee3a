// Shared skeleton of the InstanceNorm (norm_act.hip) and BatchNorm (batch_norm_act.hip) + PReLU passes over channels-last
// activations: the padded per-chunk constant table, the channel-chunk grid-stride sweeps, the three-sum backward row reduction, the
// whole-row dy store, the fp64 summation trees, and the host-side channel-chunk validation, grid and dtype dispatch.  Each piece
// takes the per-element arithmetic as a callable and does not know which norm calls it.  The kernels compute a sweep's start and
// stride from the built-in registers and hand them in: a sweep that read blockDim.x itself made every caller load the workgroup
// size from the dispatch packet.
#pragma once
#include <type_traits>

#include "ctseg_dev.h"

// Marks the per-element lambdas handed to the skeleton below: inlined before the kernel is optimised, as if written in place
#define NORM_FN __attribute__((always_inline))

namespace ctseg {

// Per-chunk constant table in LDS: the K constants of the EPC channels of chunk cv at cv * (K * EPC + 1).  Consecutive lanes read
// consecutive chunks, and without the pad word their addresses are K * EPC floats apart -- a 32-way bank conflict on every read at
// C = 256 (the 25 MB bottom-level backward pass took 91 us, the 151 MB level-1 pass 47).  tab_chunk(s, Cv) is the first word past
// the table.
template <int K, int EPC> __device__ __forceinline__ float* tab_chunk(float* s, int cv) { return s + cv * (K * EPC + 1); }
// tab_row(s, c)[k] = constant k of channel c
template <int K, int EPC> __device__ __forceinline__ float* tab_row(float* s, int c) { return tab_chunk<K, EPC>(s, c / EPC) + (c % EPC) * K; }

// Grid-stride sweep of body(v, cv) over S rows of Cv channel chunks from item i0 = blockIdx.x * blockDim.x + threadIdx.x.  A
// thread keeps its channel chunk when the grid stride is a multiple of Cv (the launcher arranges it, ew_blocks_for): no 64-bit
// division per element, and the per-channel constants stay in registers.
template <class Body>
__device__ __forceinline__ void chunk_sweep_fwd(int64_t i0, int64_t stride, int64_t S, int Cv, Body body) {
  if (stride % Cv == 0) {
    int64_t v = i0 / Cv;
    const int cv = (int)(i0 - v * Cv);
    const int64_t vstep = stride / Cv;
    for (; v < S; v += vstep) body(v, cv);
  } else {
    const int64_t total = S * Cv;
    for (int64_t i = i0; i < total; i += stride) {
      const int64_t v = i / Cv;
      body(v, (int)(i - v * Cv));
    }
  }
}

// The same sweep BACKWARDS over total = S * Cv items (last row first).  The backward reduce pass that precedes an apply pass
// streamed (g, y) front to back: walking back re-reads the most recently read part of both while it still sits in L2 / Infinity
// Cache.
template <class Body>
__device__ __forceinline__ void chunk_sweep_bwd(int64_t i0, int64_t stride, int64_t total, int Cv, Body body) {
  if (stride % Cv == 0) {
    if (i0 < total) {
      const int64_t i = total - 1 - i0;
      int64_t v = i / Cv;
      const int cv = (int)(i - v * Cv);
      const int64_t vstep = stride / Cv;
      for (; v >= 0; v -= vstep) body(v, cv);
    }
  } else {
    for (int64_t ir = i0; ir < total; ir += stride) {
      const int64_t i = total - 1 - ir;
      const int64_t v = i / Cv;
      body(v, (int)(i - v * Cv));
    }
  }
}

// Backward pass 1 of a 256-thread block (p, n): rows [p * rows_per, ...) of sample n -> partials[n][p][3][ld], the three per-channel
// sums that term(cv, e, g, y, a1, a2, a3) accumulates for channel cv * EPC + e < C.  s_red: the cross-thread reduction scratch --
// 4 waves x Cv x 3 x EPC floats when Cv is a power of two <= 64 (wave butterflies first), else one slot per thread (256 x 3 x EPC).
// The footprint matters: this pass shares the CUs with the weight-gradient kernels of the side stream, and at 24 KB per block few
// of its blocks found room beside them.
template <typename T, int EPC, class Term>
__device__ __forceinline__ void bwd_reduce_rows(const char* __restrict__ g, int g_ld, const char* __restrict__ y, int y_ld,
                                                float* __restrict__ partials, float* s_red, int P, int ld, int64_t S, int C, int Cv,
                                                int p, int n, unsigned tid, Term term) {
  constexpr int SZ = TT<T>::SZ;
  const bool pow2 = (Cv & (Cv - 1)) == 0 && Cv <= 64;
  const int64_t rows_per = (S + P - 1) / P;
  const int64_t v0 = p * rows_per, v1 = (v0 + rows_per < S) ? v0 + rows_per : S;
  const int nrow_thr = 256 / Cv;  // threads along rows
  const int cv = tid % Cv, rsub = tid / Cv;
  float a1[EPC], a2[EPC], a3[EPC];
#pragma unroll
  for (int e = 0; e < EPC; ++e) a1[e] = a2[e] = a3[e] = 0.f;
  if (rsub < nrow_thr) {
    for (int64_t v = v0 + rsub; v < v1; v += nrow_thr) {
      const int64_t vox = (int64_t)n * S + v;
      float gv[EPC], yv[EPC];
      load_ep<T, EPC>(g + (vox * g_ld + cv * EPC) * SZ, gv);
      load_ep<T, EPC>(y + (vox * y_ld + cv * EPC) * SZ, yv);
#pragma unroll
      for (int e = 0; e < EPC; ++e)
        if (cv * EPC + e < C) term(cv, e, gv[e], yv[e], a1[e], a2[e], a3[e]);
    }
  }
  if (pow2) {
    // lanes l, l + Cv, l + 2 Cv ... of a wave hold the same channel chunk (64 % Cv == 0): xor butterfly, then 4 waves via LDS
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int e = 0; e < EPC; ++e)
      for (int o = 32; o >= Cv; o >>= 1) {
        a1[e] += __shfl_xor(a1[e], o, 64);
        a2[e] += __shfl_xor(a2[e], o, 64);
        a3[e] += __shfl_xor(a3[e], o, 64);
      }
    if (lane < Cv) {
#pragma unroll
      for (int e = 0; e < EPC; ++e) {
        s_red[((wave * Cv + lane) * 3 + 0) * EPC + e] = a1[e];
        s_red[((wave * Cv + lane) * 3 + 1) * EPC + e] = a2[e];
        s_red[((wave * Cv + lane) * 3 + 2) * EPC + e] = a3[e];
      }
    }
    __syncthreads();
    for (int i = tid; i < 3 * C; i += blockDim.x) {
      const int which = i / C, c = i - which * C;
      const int ccv = c / EPC, e = c - ccv * EPC;
      float s = 0.f;
#pragma unroll
      for (int w = 0; w < 4; ++w) s += s_red[((w * Cv + ccv) * 3 + which) * EPC + e];
      partials[(((int64_t)n * P + p) * 3 + which) * ld + c] = s;
    }
    return;
  }
#pragma unroll
  for (int e = 0; e < EPC; ++e) {
    s_red[(tid * 3 + 0) * EPC + e] = a1[e];
    s_red[(tid * 3 + 1) * EPC + e] = a2[e];
    s_red[(tid * 3 + 2) * EPC + e] = a3[e];
  }
  __syncthreads();
  for (int i = tid; i < 3 * C; i += blockDim.x) {
    const int which = i / C, c = i - which * C;
    const int ccv = c / EPC, e = c - ccv * EPC;
    float s = 0.f;
    for (int r = 0; r < nrow_thr; ++r) s += s_red[((r * Cv + ccv) * 3 + which) * EPC + e];
    partials[(((int64_t)n * P + p) * 3 + which) * ld + c] = s;
  }
}

// Store one chunk of dy.  8-byte chunks into rows one chunk wider than the channels (12-wide inputs, 16-wide dy): the last chunk and
// the padding go out as ONE 16-byte store, so every 32-byte row is written whole (no partial sectors at the memory side).
template <typename T, int EPC>
__device__ __forceinline__ void store_dy_chunk(char* __restrict__ dy, int dy_ld, int64_t vox, int cv, int Cv, const float* o) {
  constexpr int SZ = TT<T>::SZ;
  if constexpr (EPC * SZ == 8) {
    if (cv == Cv - 1 && dy_ld == (Cv + 1) * EPC) {
      float o2[2 * EPC];
#pragma unroll
      for (int e = 0; e < EPC; ++e) { o2[e] = o[e]; o2[EPC + e] = 0.f; }
      store_ep<T, 2 * EPC>(dy + (vox * dy_ld + cv * EPC) * SZ, o2);
      return;
    }
  }
  store_ep<T, EPC>(dy + (vox * dy_ld + cv * EPC) * SZ, o);
}

// PReLU slope gradient = fixed-order sum of the backward finalize pass's per-channel terms, taken by one 256-thread block of the
// apply launch on the side (no launch of its own, no atomics -- a same-address counter in the finalize cost ~40 ns per block,
// 20 us at C = 256)
__device__ __forceinline__ void slope_grad_sum(const double* __restrict__ da_part, int n_da, float* __restrict__ dalpha, unsigned tid) {
  __shared__ double s_da[4];
  double a = 0.0;
  for (int k = tid; k < n_da; k += 256) a += da_part[k];
  a = wave_sum(a);
  if ((tid & 63) == 0) s_da[tid >> 6] = a;
  __syncthreads();
  if (tid == 0) dalpha[0] = (float)(((s_da[0] + s_da[1]) + s_da[2]) + s_da[3]);
}

// Backward pass 2: three column sums over R partial rows (row(r) -> the row's first sum; the others follow ld and 2 ld further) in a
// fixed tree of a 256-thread block -- strided fp64 sub-sums, wave butterflies, then the four wave sums in order; a few bytes of LDS,
// so the block fits on a CU whatever else runs there.  Thread 0 gets fin(r1, r2, r3).
template <class Row, class Fin>
__device__ __forceinline__ void block_sum3(int R, int ld, int t, double (&s_acc)[3][4], Row row, Fin fin) {
  double s1 = 0.0, s2 = 0.0, s3 = 0.0;
  for (int r = t; r < R; r += 256) {
    const float* q = row(r);
    s1 += (double)q[0];
    s2 += (double)q[ld];
    s3 += (double)q[2 * ld];
  }
  s1 = wave_sum(s1); s2 = wave_sum(s2); s3 = wave_sum(s3);
  if ((t & 63) == 0) { s_acc[0][t >> 6] = s1; s_acc[1][t >> 6] = s2; s_acc[2][t >> 6] = s3; }
  __syncthreads();
  if (t == 0)
    fin(((s_acc[0][0] + s_acc[0][1]) + s_acc[0][2]) + s_acc[0][3], ((s_acc[1][0] + s_acc[1][1]) + s_acc[1][2]) + s_acc[1][3],
        ((s_acc[2][0] + s_acc[2][1]) + s_acc[2][2]) + s_acc[2][3]);
}

// Statistics of 8 channels c0 .. c0 + 7 from R rows of [2][ld] (sum, sumsq) partials: 16 columns (8 sums, 8 sums of squares) x RL
// row lanes of a 16 * RL-thread block; lane r adds rows r, r + RL, ... in fp64, the RL sub-sums combine in lane order: fixed order,
// no atomics.  Thread k < 8 with c0 + k < C then gets fin(k, mean, var) (var clamped at 0).
template <int RL, class Fin>
__device__ __forceinline__ void col16_stats(const float* __restrict__ part, int R, int ld, int col0, int C, double count, int c0, int t,
                                            Fin fin) {
  __shared__ double s_sub[RL][17];
  const int col = t & 15, r = t >> 4;                 // col < 8: sum of channel c0 + col; col >= 8: sum of squares of channel c0 + col - 8
  const int c = c0 + (col & 7);
  double s = 0.0;
  if (c < C) {
    const float* p = part + (col >> 3) * ld + col0 + c;
#pragma unroll 4
    for (int row = r; row < R; row += RL) s += (double)p[(int64_t)row * 2 * ld];
  }
  s_sub[r][col] = s;
  __syncthreads();
  if (t < 8 && c0 + t < C) {
    double sm = 0.0, q = 0.0;
#pragma unroll
    for (int k = 0; k < RL; ++k) { sm += s_sub[k][t]; q += s_sub[k][8 + t]; }
    const double mean = sm / count;
    double var = q / count - mean * mean;
    if (var < 0.0) var = 0.0;
    fin(t, mean, var);
  }
}

// ---- host side ----------------------------------------------------------------------------------

// Grid of a sweep over `total` chunk items: about one item per thread, at most min(4096, cap) blocks of 256, rounded down to a
// multiple of Cv's odd part so that the stride (blocks * 256) is a multiple of Cv and a thread keeps one channel chunk (256 supplies
// the twos).  A grid too small for that keeps its size (the sweep then divides per element), or becomes 0 when `exact`.
static inline int ew_blocks_for(int64_t total, int Cv, bool exact = false, int cap = 4096) {
  const int64_t b64 = (total + 255) / 256;
  int b = (int)(b64 > 4096 ? 4096 : (b64 < 1 ? 1 : b64)), step = Cv;
  if (b > cap) b = cap;
  while (step % 2 == 0) step /= 2;
  if (exact || b >= step) b = b / step * step;
  return b;
}

// f(T(), std::integral_constant<int, EPC>()) for the storage type and chunk width a launch validated: (float, 4), (BF16, 8 or 4), and
// (F16, 8 or 4) only where F16_OK (the forward passes; no backward kernel exists for F16)
template <bool F16_OK, class F> static inline void dispatch_chunk(int dtype, int EPC_, F f) {
  using E4 = std::integral_constant<int, 4>;
  using E8 = std::integral_constant<int, 8>;
  if (dtype == CTSEG_F32) f(float(), E4());
  else if (F16_OK && dtype == CTSEG_F16) {
    if constexpr (F16_OK) { if (EPC_ == 8) f(F16(), E8()); else f(F16(), E4()); }
  }
  else if (EPC_ == 8) f(BF16(), E8());
  else f(BF16(), E4());
}

}  // namespace ctseg

// Channel-chunk validation of a launch: defines EPC_ (elements per chunk the launch works in) and Cv (chunks per row).  16-byte
// chunks, or 8-byte ones for 16-bit storage when HALF_CHUNKS and some tensor's channel stride is a multiple of 4 but not of 8
// (10 classes stored 12 wide); every stride must then be a multiple of EPC_.  F16_OK: CTSEG_F16 storage is accepted (forward only).
#define CHECK_CL(dtype, C, HALF_CHUNKS, F16_OK, ...)                                                                  \
  CTSEG_REQUIRE(dtype == CTSEG_F32 || dtype == CTSEG_BF16 || (F16_OK && dtype == CTSEG_F16),                           \
                "bad dtype %d (CTSEG_F16 is accepted by the forward pass only)", dtype);                              \
  int EPC_ = dtype == CTSEG_F32 ? 4 : 8;                                                                              \
  {                                                                                                                   \
    const int lds_[] = {__VA_ARGS__};                                                                                 \
    if (HALF_CHUNKS && ctseg::is16(dtype))                                                                            \
      for (int ld_ : lds_) if (ld_ % 8 != 0) EPC_ = 4;                                                                \
  }                                                                                                                   \
  const int Cv = (C + EPC_ - 1) / EPC_;                                                                               \
  {                                                                                                                   \
    const int lds_[] = {__VA_ARGS__};                                                                                 \
    for (int ld_ : lds_) CTSEG_REQUIRE(ld_ % EPC_ == 0 && ld_ >= Cv * EPC_, "channel stride %d not chunked for C=%d", ld_, C); \
  }
