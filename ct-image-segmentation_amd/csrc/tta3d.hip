// Test-time augmentation of the 3-D U-Net: one view's channels-last logits are resampled onto a target grid (the model's (h, w, d)
// grid or the raw scan's (d, h, w) grid), turned into logits or probabilities, permuted by the view's class map and added into an
// accumulator; a second pass turns the accumulator into labels (and probabilities, and a histogram).  The rules are in
// include/ctseg_hip.h (ctseg_tta_accumulate, ctseg_tta_finish).
// One thread owns one target voxel: it gathers up to eight view rows of ld floats as 16-byte loads and reads, updates and writes its
// own accumulator row as 16-byte accesses; there are no atomics.  One workgroup is one target h and a 16 x 16 tile of (w, d).  The
// view's contiguous axis is d and a (d, h, w) target's is w, so the tile is square: whichever of the two the lanes run along, a
// wave touches runs of 16 consecutive rows (16 * 4 * ld bytes) on both sides, and the other 15 rows of a fetched line are used by
// the same workgroup.  The lanes' fast axis is the accumulator's contiguous one (d for layout 0, w for layout 1).
// Every float operation is one float32 rounding: nothing may be contracted into an FMA.
#pragma clang fp contract(off)
#include "affine3d.h"

namespace ctseg {

constexpr int TTA_T = 16, TTA_CMAX = 16;

struct TtaArgs {
  int C, D, H, W, Dt, Ht, Wt, layout, mode, ld, acc_ld, permute;
  Affine3d m;                        // target voxel -> the point of the view it samples
  float weight;
  unsigned long long src;            // 4 bits per accumulator column: the view channel it takes
};

// nearest index of one axis; inside = it lies in [0, n)
__device__ __forceinline__ int tta_near(float q, int n, bool& inside) {
  const int r = affine3d_nearest(q, n);
  inside = r >= 0 && r < n;
  return r;
}

// corner b + c of one axis, clamped to the volume
__device__ __forceinline__ int tta_corner(float b, int c, int n) {
  const int r = (int)affine3d_corner(b, n) + c;
  return r < 0 ? 0 : (r > n - 1 ? n - 1 : r);
}

// N4 16-byte chunks of one view row
template <int N4> __device__ __forceinline__ void tta_row(const float* __restrict__ logits, int vox, int ld, float* z) {
  const char* p = reinterpret_cast<const char*>(logits + (int64_t)vox * ld);
#pragma unroll
  for (int j = 0; j < N4; ++j) load_chunk<float>(p + 16 * j, z + 4 * j);
}

// v[0..C) <- z[0..C) (mode 0) or its softmax (mode 1); entries at and beyond C are left alone
template <int N4> __device__ __forceinline__ void tta_value(float* z, int C, int mode) {
  if (mode == 0) return;
  float m = z[0];
#pragma unroll
  for (int c = 1; c < 4 * N4; ++c)
    if (c < C) m = fmaxf(m, z[c]);
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < 4 * N4; ++c)
    if (c < C) {
      z[c] = expf(z[c] - m);
      s = c == 0 ? z[0] : s + z[c];
    }
#pragma unroll
  for (int c = 0; c < 4 * N4; ++c)
    if (c < C) z[c] = z[c] / s;
}

template <int N4, int INTERP>
__global__ __launch_bounds__(256) void tta_accumulate_kernel(const float* __restrict__ logits, const TtaArgs p, float* __restrict__ acc) {
  __shared__ float s_v[TTA_CMAX][256];      // a thread's own column: the class permutation indexes it at run time
  const int t = threadIdx.x;
  const int C = p.C, D = p.D, H = p.H, W = p.W, Dt = p.Dt, Wt = p.Wt;
  const int ndt = (Dt + TTA_T - 1) / TTA_T;
  const int fast = t & (TTA_T - 1), slow = t >> 4;
  const int td = (blockIdx.x % ndt) * TTA_T + (p.layout == 0 ? fast : slow);
  const int tw = (blockIdx.x / ndt) * TTA_T + (p.layout == 0 ? slow : fast);
  const int th = blockIdx.y;
  if (td >= Dt || tw >= Wt) return;
  float qd, qh, qw;
  affine3d_point(p.m, (float)td, (float)th, (float)tw, qd, qh, qw);
  bool okd, okh, okw;
  const int rd = tta_near(qd, D, okd), rh = tta_near(qh, H, okh), rw = tta_near(qw, W, okw);
  if (!(okd && okh && okw)) return;         // not covered by this view: the row is not touched
  float z[4 * N4];
  if (INTERP == 0) {
    tta_row<N4>(logits, (rh * W + rw) * D + rd, p.ld, z);             // < 2^31: the entry checks D * H * W
  } else {
    const float bd = floorf(qd), bh = floorf(qh), bw = floorf(qw);
    const float gd = qd - bd, gh = qh - bh, gw = qw - bw;
    int id[2], ih[2], iw[2];
    for (int c = 0; c < 2; ++c) {
      id[c] = tta_corner(bd, c, D);
      ih[c] = tta_corner(bh, c, H) * W;
      iw[c] = tta_corner(bw, c, W);
    }
    float cd[2][4 * N4];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      float ch[2][4 * N4];
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        float x[4 * N4], y[4 * N4];
        tta_row<N4>(logits, (ih[b] + iw[0]) * D + id[a], p.ld, x);
        tta_row<N4>(logits, (ih[b] + iw[1]) * D + id[a], p.ld, y);
#pragma unroll
        for (int c = 0; c < 4 * N4; ++c) ch[b][c] = affine3d_lerp(x[c], y[c], gw);
      }
#pragma unroll
      for (int c = 0; c < 4 * N4; ++c) cd[a][c] = affine3d_lerp(ch[0][c], ch[1][c], gh);
    }
#pragma unroll
    for (int c = 0; c < 4 * N4; ++c) z[c] = affine3d_lerp(cd[0][c], cd[1][c], gd);
  }
  tta_value<N4>(z, C, p.mode);
  if (p.permute) {
#pragma unroll
    for (int c = 0; c < 4 * N4; ++c)
      if (c < C) s_v[c][t] = z[c];
#pragma unroll
    for (int k = 0; k < 4 * N4; ++k)
      if (k < C) z[k] = s_v[(int)((p.src >> (4 * k)) & 15ull)][t];
  }
  const int row = p.layout == 0 ? (th * Wt + tw) * Dt + td : (td * p.Ht + th) * Wt + tw;      // < 2^31: the entry checks Dt * Ht * Wt
  char* out = reinterpret_cast<char*>(acc + (int64_t)row * p.acc_ld);
  // columns 0..C: ceil((C + 1) / 4) chunks, which is N4 or N4 + 1; what lies beyond column C is written back as it was read
#pragma unroll
  for (int j = 0; j <= N4; ++j) {
    if (4 * j > C) break;
    float v[4];
    load_chunk<float>(out + 16 * j, v);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int k = 4 * j + i;
      if (k < C) {
        if (j < N4) v[i] = v[i] + p.weight * z[k < 4 * N4 ? k : 0];
      } else if (k == C) {
        v[i] = v[i] + p.weight;
      }
    }
    store_chunk<float>(out + 16 * j, v);
  }
}

__global__ __launch_bounds__(256) void tta_finish_kernel(const float* __restrict__ acc, int acc_ld, int C, int64_t St, int mode,
                                                         uint8_t* __restrict__ labels, float* __restrict__ probs,
                                                         unsigned long long* __restrict__ hist) {
  __shared__ unsigned int s_h[TTA_CMAX];
  const int t = threadIdx.x;
  if (t < TTA_CMAX) s_h[t] = 0;
  __syncthreads();
  // a workgroup walks the rows with stride gridDim.x * 256, so that its counts reach the global histogram once: one workgroup
  // per 256 rows sent 10 same-address atomics each and ran 4 x slower on the model grid
  for (int64_t row = (int64_t)blockIdx.x * 256 + t; row < St; row += (int64_t)gridDim.x * 256) {
    const char* in = reinterpret_cast<const char*>(acc + row * acc_ld);
    float v[TTA_CMAX + 4];
#pragma unroll
    for (int j = 0; j <= TTA_CMAX / 4; ++j)
      if (4 * j <= C) load_chunk<float>(in + 16 * j, v + 4 * j);
    float wsum = 0.f;
#pragma unroll
    for (int k = 1; k <= TTA_CMAX; ++k)
      if (k == C) wsum = v[k];
    int lab = 0;
    float best = v[0];
#pragma unroll
    for (int k = 1; k < TTA_CMAX; ++k)
      if (k < C && v[k] > best) best = v[k], lab = k;
    if (wsum == 0.f) lab = 0;
    labels[row] = (uint8_t)lab;
    if (hist) atomicAdd(&s_h[lab], 1u);
    if (probs) {
      float* pr = probs + row * C;
      if (wsum == 0.f) {
#pragma unroll
        for (int k = 0; k < TTA_CMAX; ++k)
          if (k < C) pr[k] = 0.f;
      } else {
#pragma unroll
        for (int k = 0; k < TTA_CMAX; ++k)
          if (k < C) v[k] = v[k] / wsum;
        if (mode == 0) tta_value<TTA_CMAX / 4>(v, C, 1);
#pragma unroll
        for (int k = 0; k < TTA_CMAX; ++k)
          if (k < C) pr[k] = v[k];
      }
    }
  }
  __syncthreads();
  if (hist && t < C && s_h[t]) atomicAdd(&hist[t], (unsigned long long)s_h[t]);
}

}  // namespace ctseg

using namespace ctseg;

extern "C" int ctseg_tta_accumulate(const float* logits, int32_t ld, int32_t C, int32_t D, int32_t H, int32_t W, const float* matrix,
                                    const int32_t* chan_src, float weight, int32_t mode, int32_t interp, int32_t Dt, int32_t Ht,
                                    int32_t Wt, int32_t layout, float* acc, int32_t acc_ld, void* stream) {
  CTSEG_REQUIRE(logits && acc && matrix, "tta_accumulate: logits, matrix or acc is a null pointer");
  CTSEG_REQUIRE(D > 0 && H > 0 && W > 0 && Dt > 0 && Ht > 0 && Wt > 0, "tta_accumulate: bad geometry");
  CTSEG_REQUIRE((int64_t)D * H * W < (1ll << 31) && (int64_t)Dt * Ht * Wt < (1ll << 31), "tta_accumulate: a volume of 2^31 voxels or more");
  CTSEG_REQUIRE(Ht <= 65535, "tta_accumulate: a target of more than 65535 rows along h");
  CTSEG_REQUIRE(C >= 1 && C <= TTA_CMAX, "tta_accumulate: C = %d is outside 1..16", C);
  CTSEG_REQUIRE(ld % 4 == 0 && C <= ld, "tta_accumulate: ld = %d needs ld %% 4 == 0 and ld >= C = %d", ld, C);
  CTSEG_REQUIRE(acc_ld % 4 == 0 && acc_ld >= C + 1, "tta_accumulate: acc_ld = %d needs acc_ld %% 4 == 0 and acc_ld >= C + 1 = %d", acc_ld, C + 1);
  CTSEG_REQUIRE((uintptr_t)logits % 16 == 0 && (uintptr_t)acc % 16 == 0, "tta_accumulate: unaligned logits or acc (16 bytes)");
  CTSEG_REQUIRE(mode == 0 || mode == 1, "tta_accumulate: mode %d is neither 0 (logits) nor 1 (probabilities)", mode);
  CTSEG_REQUIRE(interp == 0 || interp == 1, "tta_accumulate: interp %d is neither 0 (nearest) nor 1 (trilinear)", interp);
  CTSEG_REQUIRE(layout == 0 || layout == 1, "tta_accumulate: layout %d is neither 0 (h, w, d) nor 1 (d, h, w)", layout);
  CTSEG_REQUIRE(std::isfinite(weight) && weight > 0.f, "tta_accumulate: weight is not a finite positive number");
  TtaArgs p;
  const int tgt[3] = {Dt, Ht, Wt};
  if (int rc = affine3d_check("tta_accumulate", matrix, tgt, "target grid", p.m)) return rc;
  bool identity;
  if (int rc = pack_permutation("tta_accumulate", "chan_src", chan_src, C, p.src, identity)) return rc;
  p.permute = !identity;
  p.C = C, p.D = D, p.H = H, p.W = W, p.Dt = Dt, p.Ht = Ht, p.Wt = Wt, p.layout = layout, p.mode = mode, p.ld = ld, p.acc_ld = acc_ld;
  p.weight = weight;
  dim3 grid(((Dt + TTA_T - 1) / TTA_T) * ((Wt + TTA_T - 1) / TTA_T), Ht);
  hipStream_t st = (hipStream_t)stream;
#define CTSEG_TTA_LAUNCH(N4)                                                                                          \
  do {                                                                                                                \
    if (interp) hipLaunchKernelGGL((tta_accumulate_kernel<N4, 1>), grid, dim3(256), 0, st, logits, p, acc);           \
    else hipLaunchKernelGGL((tta_accumulate_kernel<N4, 0>), grid, dim3(256), 0, st, logits, p, acc);                  \
  } while (0)
  switch ((C + 3) / 4) {
    case 1: CTSEG_TTA_LAUNCH(1); break;
    case 2: CTSEG_TTA_LAUNCH(2); break;
    case 3: CTSEG_TTA_LAUNCH(3); break;
    default: CTSEG_TTA_LAUNCH(4); break;
  }
#undef CTSEG_TTA_LAUNCH
  CTSEG_LAUNCH_CHECK("tta_accumulate");
  return 0;
}

extern "C" int ctseg_tta_finish(const float* acc, int32_t acc_ld, int32_t C, int64_t St, int32_t mode, uint8_t* labels, float* probs,
                                int64_t* hist, void* stream) {
  CTSEG_REQUIRE(acc && labels, "tta_finish: acc or labels is a null pointer");
  CTSEG_REQUIRE(C >= 1 && C <= TTA_CMAX, "tta_finish: C = %d is outside 1..16", C);
  CTSEG_REQUIRE(St > 0 && St < (1ll << 31), "tta_finish: St = %lld is outside 1..2^31-1", (long long)St);
  CTSEG_REQUIRE(acc_ld % 4 == 0 && acc_ld >= C + 1, "tta_finish: acc_ld = %d needs acc_ld %% 4 == 0 and acc_ld >= C + 1 = %d", acc_ld, C + 1);
  CTSEG_REQUIRE((uintptr_t)acc % 16 == 0 && (!probs || (uintptr_t)probs % 4 == 0) && (!hist || (uintptr_t)hist % 8 == 0),
                "tta_finish: unaligned acc (16 bytes), probs (4) or hist (8)");
  CTSEG_REQUIRE(mode == 0 || mode == 1, "tta_finish: mode %d is neither 0 (logits) nor 1 (probabilities)", mode);
  const int64_t wgs = (St + 255) / 256;
  hipLaunchKernelGGL(tta_finish_kernel, dim3((unsigned)(wgs < 8 * CTSEG_NUM_CU ? wgs : 8 * CTSEG_NUM_CU)), dim3(256), 0,
                     (hipStream_t)stream, acc, acc_ld, C, St, mode, labels, probs, (unsigned long long*)hist);
  CTSEG_LAUNCH_CHECK("tta_finish");
  return 0;
}
