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
#include "pipeline2d_common.h"

namespace ctseg {

enum { P2_CROP = 0, P2_RESIZE = 1 };

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
    const RotWalk r = rot_walk(rot, Hc, Wc);
    base = (y0 + r.cy0) * W64 + (x0 + r.cx0);
    si = r.yi * W64 + r.xi;
    sj = r.yj * W64 + r.xj;
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
  MaskTally tally;

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
          store_image4(image_out + ((int64_t)b * win.C + c) * So + dst, val[c], win, c, n, img_vec);
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
        tally.plane(m, n, k, lab);
        if (masks_out != nullptr) store_bytes4(masks_out + ((int64_t)b * K + k) * So + dst, m[0], m[1], m[2], m[3], n, msk_vec);
      }
      if (want_lab) {
        if (labels_out != nullptr) store_bytes4(labels_out + (int64_t)b * So + dst, lab[0], lab[1], lab[2], lab[3], n, msk_vec);
        tally.count(lab, n, K, s_h);
      }
    }
  }

  tally.flush(s_h, &s_pres, K, tid, hist ? hist + (int64_t)b * (K + 1) : nullptr, present ? present + (int64_t)b * K : nullptr);
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
  CTSEG_REQUIRE(!image_store || is_raw_dtype(image_dtype), "pipeline2d_batch: image dtype %d", image_dtype);
  CTSEG_REQUIRE((mean == nullptr) == (denom == nullptr), "pipeline2d_batch: mean and denom come together");
  CTSEG_REQUIRE(!mask_store || (K > 0 && K <= P2_KMAX && mask_bytes > 0 && (masks_out || labels_out || present)),
                "pipeline2d_batch: masks need K <= %d and an output", P2_KMAX);
  CTSEG_REQUIRE(mask_store || !(masks_out || labels_out || hist || present), "pipeline2d_batch: mask outputs without masks");
  CTSEG_REQUIRE(!hist || labels_out, "pipeline2d_batch: hist needs labels_out");
  CTSEG_REQUIRE(((uintptr_t)image_out % 4) == 0 && ((uintptr_t)image_store % (image_dtype == CTSEG_F32 ? 4 : image_dtype == CTSEG_I16 ? 2 : 1)) == 0,
                "pipeline2d_batch: unaligned image pointer");
  if (check_table(table_host, B, K, mode, Ho, Wo, image_store != nullptr, image_elems, mask_store != nullptr, mask_bytes)) return -1;
  Pipe2dWin w;
  if (fill_windows(w, "pipeline2d_batch", image_store ? C : 0, win_lo, win_hi, shift, mean, denom)) return -1;
  const int64_t ngroups = (int64_t)Ho * ((Wo + 3) / 4);
  int64_t blocks = (ngroups + 255) / 256;
  if (blocks > 64) blocks = 64;
  const dim3 grid((unsigned)blocks, B);
  // (a call without an image may carry any dtype code: one that names no pixel type takes the float kernel)
  with_raw_dtype(is_raw_dtype(image_dtype) ? image_dtype : CTSEG_F32, [&](auto ti) {
    using TI = decltype(ti);
    auto launch = [&](auto md) {
      hipLaunchKernelGGL((pipeline2d_kernel<TI, decltype(md)::value>), grid, dim3(256), 0, (hipStream_t)stream, (const TI*)image_store,
                         image_elems, mask_store, mask_bytes, table, K, Ho, Wo, w, image_out, masks_out, labels_out,
                         (unsigned long long*)hist, present);
    };
    if (mode == P2_CROP) launch(std::integral_constant<int, P2_CROP>{});
    else launch(std::integral_constant<int, P2_RESIZE>{});
  });
  CTSEG_LAUNCH_CHECK("pipeline2d_batch");
  return 0;
}
