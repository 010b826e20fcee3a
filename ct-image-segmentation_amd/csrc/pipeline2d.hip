// 2-D input pipeline on gfx950: the albumentations presets of capstone/transforms/predefined.py that are per-pixel and index
// arithmetic (windowed_degree_1, windowed_degree_2 and every "test" side), a whole batch in one launch:
//   WindowedChannels / SoftTissueWindowing (capstone/transforms/transforms_2d.py:97-107)
//   -> A.RandomCrop + A.RandomRotate90 + A.HorizontalFlip  (CROP)   or   A.Resize  (RESIZE)
//   -> A.Normalize(max_pixel_value=1.0) -> ToTensorV2, and optionally _squash_masks + weighted_mixup's structure indicator.
// A memory-bound streaming pass.  One lane owns 4 consecutive OUTPUT pixels of a row: the image leaves as one 16-byte store per
// window, each mask plane and the label map as one 4-byte store; rotation and flip are on the gather side, where a crop row that
// runs along +x or -x is still one (element-aligned) vector load per plane.  Every raw pixel is read once for all windows, every
// mask byte once for masks, labels, hist and present.
// The arithmetic is the reference's, operation by operation (float64 where numpy holds float64), so nothing here may be contracted:
#pragma clang fp contract(off)
#include "ctseg_dev.h"

namespace ctseg {

constexpr int P2_KMAX = 15, P2_CMAX = 4, P2_COLS = 8;
enum { P2_CROP = 0, P2_RESIZE = 1 };
// table row of one sample (int64 each): image_off (elements into the image store), mask_off (bytes into the mask store; planes
// [K][H][W]), H, W, y0, x0, k, flip
enum { P2_IMG, P2_MSK, P2_H, P2_W, P2_Y0, P2_X0, P2_ROT, P2_FLIP };

struct Pipe2dWin {
  double lo[P2_CMAX], hi[P2_CMAX], den[P2_CMAX];      // den = hi - lo + 1e-8, formed in double as Python forms it
  float mean[P2_CMAX], denom[P2_CMAX];
  int C, shift, normalize;
};

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

// bilinear source of one axis (half-pixel centres): first tap s and the float32 weight of tap s + 1
__device__ __forceinline__ void lin_src(int d, double scale, int in, int& s, float& wt) {
  const float f = (float)(((double)d + 0.5) * scale - 0.5);
  s = (int)floorf(f);
  wt = f - (float)s;
  if (s < 0) { s = 0; wt = 0.f; }
  if (s >= in - 1) { s = in - 1; wt = 0.f; }
}
__device__ __forceinline__ int near_src(int d, double scale, int in) {
  const int s = (int)floor((double)d * scale);
  return s < in - 1 ? s : in - 1;
}
__device__ __forceinline__ double lerp2(double a, double b, float wt) {
  const float w0 = 1.f - wt;                            // float32, as `1 - w` of a float32 w
  return a * (double)w0 + b * (double)wt;
}

// Block (x, b) walks the 4-pixel groups of sample b with stride gridDim.x * 256.
template <typename TI, int MODE>
__global__ __launch_bounds__(256) void pipeline2d_kernel(const TI* __restrict__ image_store, int64_t image_elems,
                                                         const uint8_t* __restrict__ mask_store, int64_t mask_bytes,
                                                         const int64_t* __restrict__ table, int K, int Ho, int Wo, Pipe2dWin win,
                                                         float* __restrict__ image_out, uint8_t* __restrict__ masks_out,
                                                         uint8_t* __restrict__ labels_out, unsigned long long* __restrict__ hist,
                                                         int* __restrict__ present) {
  __shared__ unsigned int s_h[P2_KMAX + 1];
  __shared__ unsigned int s_pres;
  const int b = blockIdx.y, tid = threadIdx.x;
  const int64_t* row = table + (int64_t)b * P2_COLS;
  const int64_t img_off = row[P2_IMG], msk_off = row[P2_MSK], H64 = row[P2_H], W64 = row[P2_W];
  const int64_t y0 = row[P2_Y0], x0 = row[P2_X0], rot = row[P2_ROT], flip = row[P2_FLIP];
  // The table lives on the device: no launch may read outside its stores for it.  A row the host-side checks would have refused
  // leaves its sample untouched.
  bool ok = H64 > 0 && W64 > 0 && H64 < (1 << 24) && W64 < (1 << 24);
  if (ok && image_store) ok = img_off >= 0 && img_off + H64 * W64 <= image_elems;
  if (ok && mask_store) ok = msk_off >= 0 && msk_off + (int64_t)K * H64 * W64 <= mask_bytes;
  if (ok && MODE == P2_CROP) {
    const int64_t Hc = (rot & 1) ? Wo : Ho, Wc = (rot & 1) ? Ho : Wo;
    ok = rot >= 0 && rot <= 3 && y0 >= 0 && x0 >= 0 && y0 + Hc <= H64 && x0 + Wc <= W64;
  }
  if (!ok) return;
  const int H = (int)H64, W = (int)W64;
  const int64_t plane = H64 * W64;
  if (tid <= P2_KMAX) s_h[tid] = 0u;
  if (tid == 0) s_pres = 0u;
  __syncthreads();

  // CROP: source element of output (i, j) = base + i * si + j * sj.  With j' = flip ? Wo - 1 - j : j, np.rot90(Cr, k)[i][j'] is
  // Cr[i][j'], Cr[j'][Wc-1-i], Cr[Hc-1-i][Wc-1-j'], Cr[Hc-1-j'][i] for k = 0..3 (Cr the Hc x Wc crop at (y0, x0))
  int64_t base = 0, si = 0, sj = 0;
  if (MODE == P2_CROP) {
    const int64_t Hc = (rot & 1) ? Wo : Ho, Wc = (rot & 1) ? Ho : Wo;
    int64_t cy0, cx0, yi, yj, xi, xj;                  // crop row = cy0 + yi*i + yj*j', crop column = cx0 + xi*i + xj*j'
    if (rot == 0) { cy0 = 0; yi = 1; yj = 0; cx0 = 0; xi = 0; xj = 1; }
    else if (rot == 1) { cy0 = 0; yi = 0; yj = 1; cx0 = Wc - 1; xi = -1; xj = 0; }
    else if (rot == 2) { cy0 = Hc - 1; yi = -1; yj = 0; cx0 = Wc - 1; xi = 0; xj = -1; }
    else { cy0 = Hc - 1; yi = 0; yj = -1; cx0 = 0; xi = 1; xj = 0; }
    base = (y0 + cy0) * W64 + (x0 + cx0);
    si = yi * W64 + xi;
    sj = yj * W64 + xj;
    if (flip) { base += (int64_t)(Wo - 1) * sj; sj = -sj; }
  }
  const double scy = (double)H / (double)Ho, scx = (double)W / (double)Wo;      // RESIZE: In / Out per axis
  const TI* img = image_store ? image_store + img_off : nullptr;
  const uint8_t* msk = mask_store ? mask_store + msk_off : nullptr;
  const bool img_vec = (Wo % 4 == 0) && (((uintptr_t)image_out % 16) == 0);
  const bool msk_vec = (Wo % 4 == 0) && (((uintptr_t)masks_out % 4) == 0) && (((uintptr_t)labels_out % 4) == 0);
  const bool want_lab = labels_out != nullptr || hist != nullptr;
  const int gpr = (Wo + 3) / 4;                          // groups per output row
  const int64_t ngroups = (int64_t)Ho * gpr, So = (int64_t)Ho * Wo;
  unsigned int pres = 0u;
  int bg = 0;

  for (int64_t g = blockIdx.x * (int64_t)blockDim.x + tid; g < ngroups; g += (int64_t)gridDim.x * blockDim.x) {
    const int oy = (int)(g / gpr), ox0 = (int)(g % gpr) * 4;
    const int n = Wo - ox0 < 4 ? Wo - ox0 : 4;
    const int64_t src0 = base + oy * si + ox0 * sj;      // CROP
    const int64_t dst = (int64_t)oy * Wo + ox0;

    if (img != nullptr && image_out != nullptr) {
      double val[P2_CMAX][4];
      if (MODE == P2_CROP) {
        TI raw[4];
        load4<TI>(img + src0, sj, n, raw);
#pragma unroll
        for (int c = 0; c < P2_CMAX; ++c)
#pragma unroll
          for (int q = 0; q < 4; ++q) val[c][q] = c < win.C ? window_value<TI>(raw[q], win, c) : 0.0;
      } else {
        int sy; float wy;
        lin_src(oy, scy, H, sy, wy);
        const TI* r0 = img + (int64_t)sy * W;
        const TI* r1 = img + (int64_t)(sy + 1 < H ? sy + 1 : H - 1) * W;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          int sx; float wx;
          lin_src(q < n ? ox0 + q : ox0, scx, W, sx, wx);
          const int sx1 = sx + 1 < W ? sx + 1 : W - 1;
          const TI t00 = r0[sx], t01 = r0[sx1], t10 = r1[sx], t11 = r1[sx1];
#pragma unroll
          for (int c = 0; c < P2_CMAX; ++c) {
            if (c < win.C) {
              // horizontal pass on both rows, then the vertical one
              const double h0 = lerp2(window_value<TI>(t00, win, c), window_value<TI>(t01, win, c), wx);
              const double h1 = lerp2(window_value<TI>(t10, win, c), window_value<TI>(t11, win, c), wx);
              val[c][q] = lerp2(h0, h1, wy);
            } else {
              val[c][q] = 0.0;
            }
          }
        }
      }
#pragma unroll
      for (int c = 0; c < P2_CMAX; ++c) {
        if (c < win.C) {
          float* o = image_out + ((int64_t)b * win.C + c) * So + dst;
          f32x4 r;
#pragma unroll
          for (int q = 0; q < 4; ++q) r[q] = normalize_value(val[c][q], win, c);
          if (img_vec) {
            *reinterpret_cast<f32x4*>(o) = r;
          } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) if (q < n) o[q] = r[q];
          }
        }
      }
    }

    if (msk != nullptr) {
      int64_t m0 = src0, ms = sj;
      int sxm[4] = {0, 0, 0, 0};
      if (MODE == P2_RESIZE) {
        m0 = (int64_t)near_src(oy, scy, H) * W;
        ms = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) sxm[q] = near_src(q < n ? ox0 + q : ox0, scx, W);
      }
      int lab[4] = {0, 0, 0, 0};
      for (int k = 0; k < K; ++k) {
        const uint8_t* p = msk + (int64_t)k * plane + m0;
        uint8_t m[4];
        if (MODE == P2_CROP) {
          load4<uint8_t>(p, ms, n, m);
        } else {
#pragma unroll
          for (int q = 0; q < 4; ++q) m[q] = p[sxm[q]];
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          if (q < n) {
            if (m[q] == 1) pres |= 1u << k;
            const int val = (int)m[q] * (k + 1);
            lab[q] = val > lab[q] ? val : lab[q];
          }
        }
        if (masks_out != nullptr) {
          uint8_t* o = masks_out + ((int64_t)b * K + k) * So + dst;
          if (msk_vec) {
            *reinterpret_cast<uint32_t*>(o) = (uint32_t)m[0] | ((uint32_t)m[1] << 8) | ((uint32_t)m[2] << 16) | ((uint32_t)m[3] << 24);
          } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) if (q < n) o[q] = m[q];
          }
        }
      }
      if (want_lab) {
        if (labels_out != nullptr) {
          uint8_t* o = labels_out + (int64_t)b * So + dst;
          if (msk_vec) {
            *reinterpret_cast<uint32_t*>(o) = (uint32_t)(lab[0] & 0xff) | ((uint32_t)(lab[1] & 0xff) << 8) |
                                              ((uint32_t)(lab[2] & 0xff) << 16) | ((uint32_t)(lab[3] & 0xff) << 24);
          } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) if (q < n) o[q] = (uint8_t)lab[q];
          }
        }
        // background is nearly all of a CT slice, and 64 lanes adding to ONE LDS word serialise: count it per thread
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          if (q < n) {
            if (lab[q] == 0) ++bg;
            else if (lab[q] <= K) atomicAdd(&s_h[lab[q]], 1u);
          }
        }
      }
    }
  }

  // wave reduction, then one atomic per workgroup and class (squash_masks_kernel's pattern)
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { bg += __shfl_xor(bg, o, 64); pres |= __shfl_xor(pres, o, 64); }
  if ((tid & 63) == 0) {
    if (bg) atomicAdd(&s_h[0], (unsigned)bg);
    if (pres) atomicOr(&s_pres, pres);
  }
  __syncthreads();
  if (hist != nullptr && tid <= K && s_h[tid] != 0u) atomicAdd(&hist[(int64_t)b * (K + 1) + tid], (unsigned long long)s_h[tid]);
  if (present != nullptr && tid < K && ((s_pres >> tid) & 1u)) atomicOr(&present[(int64_t)b * K + tid], 1);
}

// the host's copy of the table, row by row: what the kernel would skip is an error here
static int check_table(const int64_t* t, int B, int K, int mode, int Ho, int Wo, bool has_image, int64_t image_elems, bool has_masks,
                       int64_t mask_bytes) {
  for (int b = 0; b < B; ++b) {
    const int64_t* r = t + (int64_t)b * P2_COLS;
    const int64_t H = r[P2_H], W = r[P2_W], k = r[P2_ROT];
    CTSEG_REQUIRE(H > 0 && W > 0 && H < (1 << 24) && W < (1 << 24), "pipeline2d_batch: sample %d: bad slice size", b);
    CTSEG_REQUIRE(!has_image || (r[P2_IMG] >= 0 && r[P2_IMG] + H * W <= image_elems), "pipeline2d_batch: sample %d: image outside its store", b);
    CTSEG_REQUIRE(!has_masks || (r[P2_MSK] >= 0 && r[P2_MSK] + (int64_t)K * H * W <= mask_bytes),
                  "pipeline2d_batch: sample %d: masks outside their store", b);
    if (mode != P2_CROP) continue;
    CTSEG_REQUIRE(k >= 0 && k <= 3 && (r[P2_FLIP] == 0 || r[P2_FLIP] == 1), "pipeline2d_batch: sample %d: k in 0..3, flip in 0/1", b);
    CTSEG_REQUIRE(!(k & 1) || Ho == Wo, "pipeline2d_batch: sample %d: rot90 by an odd k needs a square output (%d x %d)", b, Ho, Wo);
    CTSEG_REQUIRE(r[P2_Y0] >= 0 && r[P2_X0] >= 0 && r[P2_Y0] + Ho <= H && r[P2_X0] + Wo <= W,
                  "pipeline2d_batch: sample %d: crop (%lld, %lld) + %d x %d leaves the %lld x %lld slice", b, (long long)r[P2_Y0],
                  (long long)r[P2_X0], Ho, Wo, (long long)H, (long long)W);
  }
  return 0;
}

}  // namespace ctseg

using namespace ctseg;

extern "C" int ctseg_pipeline2d_batch(const void* image_store, int32_t image_dtype, int64_t image_elems, const uint8_t* mask_store,
                                      int64_t mask_bytes, const int64_t* table, const int64_t* table_host, int32_t B, int32_t K,
                                      int32_t mode, int32_t Ho, int32_t Wo, int32_t C, const int32_t* win_lo, const int32_t* win_hi,
                                      int32_t shift, const float* mean, const float* denom, float* image_out, uint8_t* masks_out,
                                      uint8_t* labels_out, int64_t* hist, int32_t* present, void* stream) {
  CTSEG_REQUIRE(table && table_host && B > 0 && B <= 65535 && Ho > 0 && Wo > 0 && (image_store || mask_store),
                "pipeline2d_batch: bad arguments");
  CTSEG_REQUIRE(mode == P2_CROP || mode == P2_RESIZE, "pipeline2d_batch: mode %d", mode);
  CTSEG_REQUIRE(!image_store || (image_out && C >= 1 && C <= P2_CMAX && win_lo && win_hi && image_elems > 0),
                "pipeline2d_batch: an image needs image_out and 1..%d windows", P2_CMAX);
  CTSEG_REQUIRE(!image_store || image_dtype == CTSEG_F32 || image_dtype == CTSEG_I16 || image_dtype == CTSEG_U8,
                "pipeline2d_batch: image dtype %d", image_dtype);
  CTSEG_REQUIRE((mean == nullptr) == (denom == nullptr), "pipeline2d_batch: mean and denom come together");
  CTSEG_REQUIRE(!mask_store || (K > 0 && K <= P2_KMAX && mask_bytes > 0 && (masks_out || labels_out || present)),
                "pipeline2d_batch: masks need K <= %d and an output", P2_KMAX);
  CTSEG_REQUIRE(mask_store || !(masks_out || labels_out || hist || present), "pipeline2d_batch: mask outputs without masks");
  CTSEG_REQUIRE(!hist || labels_out, "pipeline2d_batch: hist needs labels_out");
  CTSEG_REQUIRE(((uintptr_t)image_out % 4) == 0 && ((uintptr_t)image_store % (image_dtype == CTSEG_F32 ? 4 : image_dtype == CTSEG_I16 ? 2 : 1)) == 0,
                "pipeline2d_batch: unaligned image pointer");
  if (check_table(table_host, B, K, mode, Ho, Wo, image_store != nullptr, image_elems, mask_store != nullptr, mask_bytes)) return -1;
  Pipe2dWin w = {};
  w.C = image_store ? C : 0;
  w.shift = shift != 0;
  w.normalize = mean != nullptr;
  for (int c = 0; c < w.C; ++c) {
    CTSEG_REQUIRE(win_hi[c] > win_lo[c], "pipeline2d_batch: window %d is empty", c);
    w.lo[c] = (double)win_lo[c];
    w.hi[c] = (double)win_hi[c];
    w.den[c] = (double)(win_hi[c] - win_lo[c]) + 1e-8;
    if (mean) { w.mean[c] = mean[c]; w.denom[c] = denom[c]; }
  }
  const int64_t ngroups = (int64_t)Ho * ((Wo + 3) / 4);
  int64_t blocks = (ngroups + 255) / 256;
  if (blocks > 64) blocks = 64;
  const dim3 grid((unsigned)blocks, B);
  hipStream_t st = (hipStream_t)stream;
#define CTSEG_P2_LAUNCH(TI, MODE)                                                                                                   \
  hipLaunchKernelGGL((pipeline2d_kernel<TI, MODE>), grid, dim3(256), 0, st, (const TI*)image_store, image_elems, mask_store, mask_bytes, \
                     table, K, Ho, Wo, w, image_out, masks_out, labels_out, (unsigned long long*)hist, present)
  if (mode == P2_CROP) {
    if (image_dtype == CTSEG_I16) CTSEG_P2_LAUNCH(short, P2_CROP);
    else if (image_dtype == CTSEG_U8) CTSEG_P2_LAUNCH(uint8_t, P2_CROP);
    else CTSEG_P2_LAUNCH(float, P2_CROP);
  } else {
    if (image_dtype == CTSEG_I16) CTSEG_P2_LAUNCH(short, P2_RESIZE);
    else if (image_dtype == CTSEG_U8) CTSEG_P2_LAUNCH(uint8_t, P2_RESIZE);
    else CTSEG_P2_LAUNCH(float, P2_RESIZE);
  }
#undef CTSEG_P2_LAUNCH
  CTSEG_LAUNCH_CHECK("pipeline2d_batch");
  return 0;
}
