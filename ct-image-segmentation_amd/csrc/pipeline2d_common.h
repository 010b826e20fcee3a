// What the 2-D input pipeline kernels share (pipeline2d.hip: crop / resize in one pass; warp2d.hip: the warping presets in two
// passes over an intermediate): the per-sample table row, the window and normalize arithmetic, the rot90 / flip index walk, and the
// mask side (plane stores, label map, hist, present).  The arithmetic is the reference's, operation by operation, so a file that
// includes this sets `#pragma clang fp contract(off)` first.
#pragma once
#include "ctseg_dev.h"

namespace ctseg {

constexpr int P2_KMAX = 15, P2_CMAX = 4, P2_COLS = 8;
// table row of one sample (int64 each): image_off (elements into the image store), mask_off (bytes into the mask store; planes
// [K][H][W]), H, W, y0, x0, k, flip
enum { P2_IMG, P2_MSK, P2_H, P2_W, P2_Y0, P2_X0, P2_ROT, P2_FLIP };

struct Pipe2dWin {
  double lo[P2_CMAX], hi[P2_CMAX], den[P2_CMAX];      // den = hi - lo + 1e-8, formed in double as Python forms it
  float mean[P2_CMAX], denom[P2_CMAX];
  int C, shift, normalize;
};

// the host arrays of an entry point -> Pipe2dWin (C = 0: no image)
static inline int fill_windows(Pipe2dWin& w, const char* who, int C, const int32_t* win_lo, const int32_t* win_hi, int shift, const float* mean,
                               const float* denom) {
  w = Pipe2dWin{};
  w.C = C;
  w.shift = shift != 0;
  w.normalize = mean != nullptr;
  for (int c = 0; c < C; ++c) {
    CTSEG_REQUIRE(win_hi[c] > win_lo[c], "%s: window %d is empty", who, c);
    w.lo[c] = (double)win_lo[c];
    w.hi[c] = (double)win_hi[c];
    w.den[c] = (double)(win_hi[c] - win_lo[c]) + 1e-8;
    if (mean) { w.mean[c] = mean[c]; w.denom[c] = denom[c]; }
  }
  return 0;
}

template <typename T> struct Vec4;                     // 4 consecutive elements at the alignment of ONE element
template <> struct Vec4<uint8_t> { typedef uint8_t type __attribute__((ext_vector_type(4), aligned(1))); };
template <> struct Vec4<short> { typedef short type __attribute__((ext_vector_type(4), aligned(2))); };
template <> struct Vec4<float> { typedef float type __attribute__((ext_vector_type(4), aligned(4))); };

// v[q] = p[q * step], q < n.  step = +-1 with all four wanted: one vector load (from p - 3 and reversed for -1)
template <typename T> __device__ __forceinline__ void load4(const T* p, int64_t step, int n, T* v) {
  using V = typename Vec4<T>::type;
  if (n == 4 && step == 1) {
    const V t = *reinterpret_cast<const V*>(p);
    v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
  } else if (n == 4 && step == -1) {
    const V t = *reinterpret_cast<const V*>(p - 3);
    v[0] = t[3]; v[1] = t[2]; v[2] = t[1]; v[3] = t[0];
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = q < n ? p[q * step] : T(0);
  }
}

// apply_window (transforms_2d.py:97-107) as numpy evaluates it: a float32 array stays float32 (bounds and divisor cast to float32),
// an integer array goes through float64.  The caller holds the result as float64 (WindowedChannels writes into a float64 array).
template <typename TI> __device__ __forceinline__ double window_value(TI raw, const Pipe2dWin& w, int c) {
  if constexpr (sizeof(TI) == 4) {
    float v = fminf(fmaxf((float)raw, (float)w.lo[c]), (float)w.hi[c]);
    if (w.shift) v = (v - (float)w.lo[c]) / (float)w.den[c];
    return (double)v;
  } else {
    double v = fmin(fmax((double)raw, w.lo[c]), w.hi[c]);
    if (w.shift) v = (v - w.lo[c]) / w.den[c];
    return v;
  }
}

// A.Normalize: astype(float32), -= mean, *= reciprocal(std): two fp32 roundings
__device__ __forceinline__ float normalize_value(double v, const Pipe2dWin& w, int c) {
  float f = (float)v;
  if (w.normalize) {
    f = f - w.mean[c];
    f = f * w.denom[c];
  }
  return f;
}

// np.rot90(Cr, k)[i][j'] of the Hc x Wc crop Cr is Cr[i][j'], Cr[j'][Wc-1-i], Cr[Hc-1-i][Wc-1-j'], Cr[Hc-1-j'][i] for k = 0..3:
// crop row = cy0 + yi*i + yj*j', crop column = cx0 + xi*i + xj*j'
struct RotWalk { int64_t cy0, yi, yj, cx0, xi, xj; };
__device__ __forceinline__ RotWalk rot_walk(int64_t rot, int64_t Hc, int64_t Wc) {
  if (rot == 0) return RotWalk{0, 1, 0, 0, 0, 1};
  if (rot == 1) return RotWalk{0, 0, 1, Wc - 1, -1, 0};
  if (rot == 2) return RotWalk{Hc - 1, -1, 0, Wc - 1, 0, -1};
  return RotWalk{Hc - 1, 0, -1, 0, 1, 0};
}

// 4 window values of channel c -> normalized floats at o: one 16-byte store, or the first n element by element
__device__ __forceinline__ void store_image4(float* o, const double* val, const Pipe2dWin& win, int c, int n, bool vec) {
  f32x4 r;
#pragma unroll
  for (int q = 0; q < 4; ++q) r[q] = normalize_value(val[q], win, c);
  if (vec) {
    *reinterpret_cast<f32x4*>(o) = r;
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q) if (q < n) o[q] = r[q];
  }
}

// 4 bytes at o: one 4-byte store, or the first n byte by byte
__device__ __forceinline__ void store_bytes4(uint8_t* o, uint32_t b0, uint32_t b1, uint32_t b2, uint32_t b3, int n, bool vec) {
  if (vec) {
    *reinterpret_cast<uint32_t*>(o) = (b0 & 0xff) | ((b1 & 0xff) << 8) | ((b2 & 0xff) << 16) | ((b3 & 0xff) << 24);
  } else {
    const uint32_t b[4] = {b0, b1, b2, b3};
#pragma unroll
    for (int q = 0; q < 4; ++q) if (q < n) o[q] = (uint8_t)b[q];
  }
}

// the mask side of one sample in one workgroup: plane k of 4 pixels -> present bit and label (highest set class wins); labels ->
// hist counts; then one atomic per workgroup and class (squash_masks_kernel's pattern)
struct MaskTally {
  unsigned int pres = 0u;
  int bg = 0;
  __device__ __forceinline__ void plane(const uint8_t* m, int n, int k, int* lab) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (q < n) {
        if (m[q] == 1) pres |= 1u << k;
        const int val = (int)m[q] * (k + 1);
        lab[q] = val > lab[q] ? val : lab[q];
      }
    }
  }
  // background is nearly all of a CT slice, and 64 lanes adding to ONE LDS word serialise: count it per thread
  __device__ __forceinline__ void count(const int* lab, int n, int K, unsigned int* s_h) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (q < n) {
        if (lab[q] == 0) ++bg;
        else if (lab[q] <= K) atomicAdd(&s_h[lab[q]], 1u);
      }
    }
  }
  // wave reduction, then LDS, then global; s_h[P2_KMAX + 1] and s_pres were zeroed before the walk (a barrier in between)
  __device__ __forceinline__ void flush(unsigned int* s_h, unsigned int* s_pres, int K, int tid, unsigned long long* hist_row, int* present_row) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { bg += __shfl_xor(bg, o, 64); pres |= __shfl_xor(pres, o, 64); }
    if ((tid & 63) == 0) {
      if (bg) atomicAdd(&s_h[0], (unsigned)bg);
      if (pres) atomicOr(s_pres, pres);
    }
    __syncthreads();
    if (hist_row != nullptr && tid <= K && s_h[tid] != 0u) atomicAdd(&hist_row[tid], (unsigned long long)s_h[tid]);
    if (present_row != nullptr && tid < K && ((*s_pres >> tid) & 1u)) atomicOr(&present_row[tid], 1);
  }
};

}  // namespace ctseg
