// The warping presets of capstone/transforms/predefined.py (degree_0, windowed_degree_3, windowed_degree_4 "train") on gfx950:
//   window -> A.RandomCrop -> A.ElasticTransform and/or A.GridDistortion -> [A.RandomRotate90 + A.HorizontalFlip] -> A.Normalize
// Three launches per batch:
//   fields   per ELASTIC sample the two displacement fields np.float32(gaussian_filter(2 * u - 1, sigma) * alpha): u from a counter
//            hash, the blur separable in float64 over lines staged in LDS (scipy's "reflect" border, axis 0 then axis 1)
//   pass 1   crop + window (+ the elastic transform's cv2.warpAffine, border on the CROP) -> float64 planes and mask bytes
//   pass 2   cv2.remap of that intermediate through the field / the grid tables / nothing, rot90 + flip on the output index side,
//            normalize, mask planes or label map, hist, present (pipeline2d_common.h: the code pipeline2d.hip runs)
// OpenCV's fixed-point rules are restated here as the tests' numpy restatement states them; nothing may be contracted:
#pragma clang fp contract(off)
#include "pipeline2d_common.h"
#include "splitmix.h"

namespace ctseg {

// the table row of pipeline2d.hip, then: kind, seed, the INVERSE affine matrix M00 M01 M02 M10 M11 M12 (float64 bit patterns),
// offsets of the sample's float32 xx (Wo values) and yy (Ho values) tables, slot of its fields (ELASTIC: 0 .. n_slots - 1, rising)
enum { P2W_KIND = P2_COLS, P2W_SEED, P2W_M, P2W_XX = P2W_M + 6, P2W_YY, P2W_SLOT, P2W_COLS };
enum { W2_NONE = 0, W2_ELASTIC = 1, W2_GRID = 2 };
enum { W2_FIELDS = 1, W2_PASS1 = 2, W2_PASS2 = 4 };
constexpr int W2_LINE_MAX = 256;          // Ho, Wo of a warped batch: a line of doubles and its reflected margins stay in LDS
constexpr int W2_LDS_DOUBLES = 6144;      // 48 KiB: lines of n + 2 * radius doubles
constexpr int W2_FIELD_THREADS = 1024;

struct Warp2dDims {
  int K, Ho, Wo, n_slots, has_image, has_masks;
  int64_t image_elems, mask_bytes, xx_elems, yy_elems;
};

// what both the host's validation and every kernel ask of a row
__host__ __device__ inline bool warp_row_ok(const int64_t* r, const Warp2dDims& d) {
  const int64_t H = r[P2_H], W = r[P2_W], k = r[P2_ROT], kind = r[P2W_KIND];
  if (!(H > 0 && W > 0 && H < (1 << 24) && W < (1 << 24))) return false;
  if (d.has_image && !(r[P2_IMG] >= 0 && r[P2_IMG] + H * W <= d.image_elems)) return false;
  if (d.has_masks && !(r[P2_MSK] >= 0 && r[P2_MSK] + (int64_t)d.K * H * W <= d.mask_bytes)) return false;
  if (!(k >= 0 && k <= 3 && (r[P2_FLIP] == 0 || r[P2_FLIP] == 1)) || ((k & 1) && d.Ho != d.Wo)) return false;
  if (!(r[P2_Y0] >= 0 && r[P2_X0] >= 0 && r[P2_Y0] + d.Ho <= H && r[P2_X0] + d.Wo <= W)) return false;
  if (kind == W2_ELASTIC) return r[P2W_SLOT] >= 0 && r[P2W_SLOT] < d.n_slots;
  if (kind == W2_GRID) return r[P2W_XX] >= 0 && r[P2W_XX] + d.Wo <= d.xx_elems && r[P2W_YY] >= 0 && r[P2W_YY] + d.Ho <= d.yy_elems;
  return kind == W2_NONE;
}

// scipy.ndimage "reflect" (d c b a | a b c d) and cv2.BORDER_REFLECT_101 (d c b | a b c d), any distance outside
__device__ __forceinline__ int reflect_sym(int p, int n) {
  const int m = 2 * n;
  p %= m;
  if (p < 0) p += m;
  return p < n ? p : m - 1 - p;
}
__device__ __forceinline__ int reflect_101(int p, int n) {
  if (n == 1) return 0;
  const int m = 2 * n - 2;
  p %= m;
  if (p < 0) p += m;
  return p < n ? p : m - p;
}

// noise of field f at (i, j): one splitmix64 mix of seed + (counter + 1) * golden, counter = f << 40 | i << 20 | j; the top 53 bits
__device__ __forceinline__ double field_noise(uint64_t seed, int f, int i, int j) {
  const double u = splitmix64_unit(seed, ((uint64_t)f << 40) | ((uint64_t)i << 20) | (uint64_t)j);
  return 2.0 * u - 1.0;
}

// Block (f, b): field f of sample b, both blur passes.  A line (a column, then a row) is staged with its reflected margins, so the
// tap loop reads LDS at fixed offsets; the weights are wave-uniform loads.  Axis 0 leaves float64 in `tmp`, which the same
// workgroup reads back after a barrier.
__global__ __launch_bounds__(W2_FIELD_THREADS) void warp2d_fields_kernel(const int64_t* __restrict__ table, Warp2dDims d,
                                                                         const double* __restrict__ gw, int radius, double alpha,
                                                                         double* __restrict__ tmp, float* __restrict__ fields) {
  __shared__ double ext[W2_LDS_DOUBLES];
  const int b = blockIdx.y, f = blockIdx.x, tid = threadIdx.x;
  const int64_t* row = table + (int64_t)b * P2W_COLS;
  if (!warp_row_ok(row, d) || row[P2W_KIND] != W2_ELASTIC) return;
  const uint64_t seed = (uint64_t)row[P2W_SEED];
  const int Ho = d.Ho, Wo = d.Wo;
  const int64_t S = (int64_t)Ho * Wo;
  double* T = tmp + (row[P2W_SLOT] * 2 + f) * S;
  float* F = fields + (row[P2W_SLOT] * 2 + f) * S;

  for (int phase = 0; phase < 2; ++phase) {
    const int n = phase == 0 ? Ho : Wo, nlines = phase == 0 ? Wo : Ho, E = n + 2 * radius;
    int lpi = W2_LDS_DOUBLES / E;                         // lines per round
    if (lpi > W2_FIELD_THREADS / n) lpi = W2_FIELD_THREADS / n;
    const int q = tid / n, l = tid - q * n;
    for (int line0 = 0; line0 < nlines; line0 += lpi) {
      const int nl = nlines - line0 < lpi ? nlines - line0 : lpi;
      for (int e = tid; e < nl * E; e += W2_FIELD_THREADS) {
        const int lq = e / E, src = reflect_sym(e - lq * E - radius, n), line = line0 + lq;
        ext[e] = phase == 0 ? field_noise(seed, f, src, line) : T[(int64_t)line * Wo + src];
      }
      __syncthreads();
      if (q < nl) {
        const double* c = ext + q * E + radius + l;
        double acc = c[0] * gw[0];
        for (int k = 1; k <= radius; ++k) acc = acc + (c[-k] + c[k]) * gw[k];
        const int line = line0 + q;
        if (phase == 0) T[(int64_t)l * Wo + line] = acc;
        else F[(int64_t)line * Wo + l] = (float)(acc * alpha);
      }
      __syncthreads();
    }
    __threadfence_block();
    __syncthreads();
  }
}

__device__ __forceinline__ int64_t sat_lrint(double v) {                       // saturate_cast<int>: round half to even, clamped
  return (int64_t)__double2ll_rn(fmin(fmax(v, -2147483648.0), 2147483647.0));
}
// the four float32 weights of a bilinear tap pair, each product rounded to float32
__device__ __forceinline__ void bilinear_weights(float fx, float fy, float* w) {
  const float gx = 1.f - fx, gy = 1.f - fy;
  w[0] = gx * gy; w[1] = fx * gy; w[2] = gx * fy; w[3] = fx * fy;
}
__device__ __forceinline__ double bilinear_value(double s00, double s01, double s10, double s11, const float* w) {
  return s00 * (double)w[0] + s01 * (double)w[1] + s10 * (double)w[2] + s11 * (double)w[3];
}

// Pass 1.  Block (x, b) walks the 4-pixel groups of the crop of sample b.  inter: float64 [B][C][Ho][Wo], then u8 [B][K][Ho][Wo].
template <typename TI>
__global__ __launch_bounds__(256) void warp2d_pass1_kernel(const TI* __restrict__ image_store, const uint8_t* __restrict__ mask_store,
                                                           const int64_t* __restrict__ table, Warp2dDims d, Pipe2dWin win,
                                                           double* __restrict__ inter_img, uint8_t* __restrict__ inter_msk) {
  const int b = blockIdx.y, tid = threadIdx.x;
  const int64_t* row = table + (int64_t)b * P2W_COLS;
  if (!warp_row_ok(row, d)) return;
  const int K = d.K, Ho = d.Ho, Wo = d.Wo;
  const int64_t W64 = row[P2_W], plane = row[P2_H] * W64, So = (int64_t)Ho * Wo;
  const int64_t base = row[P2_Y0] * W64 + row[P2_X0];
  const TI* img = image_store ? image_store + row[P2_IMG] : nullptr;
  const uint8_t* msk = mask_store ? mask_store + row[P2_MSK] : nullptr;
  const bool elastic = row[P2W_KIND] == W2_ELASTIC;
  double M[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) M[i] = __longlong_as_double(row[P2W_M + i]);
  const bool vec = (Wo % 4 == 0) && (((uintptr_t)inter_msk % 4) == 0);
  const int gpr = (Wo + 3) / 4;
  const int64_t ngroups = (int64_t)Ho * gpr;

  for (int64_t g = blockIdx.x * (int64_t)blockDim.x + tid; g < ngroups; g += (int64_t)gridDim.x * blockDim.x) {
    const int oy = (int)(g / gpr), ox0 = (int)(g % gpr) * 4;
    const int n = Wo - ox0 < 4 ? Wo - ox0 : 4;
    const int64_t dst = (int64_t)oy * Wo + ox0;
    if (!elastic) {
      const int64_t src0 = base + oy * W64 + ox0;
      if (img != nullptr) {
        TI raw[4];
        load4<TI>(img + src0, 1, n, raw);
#pragma unroll
        for (int c = 0; c < P2_CMAX; ++c) {
          if (c < win.C) {
            double* o = inter_img + ((int64_t)b * win.C + c) * So + dst;
#pragma unroll
            for (int q = 0; q < 4; ++q) if (q < n) o[q] = window_value<TI>(raw[q], win, c);
          }
        }
      }
      if (msk != nullptr) {
        for (int k = 0; k < K; ++k) {
          uint8_t m[4];
          load4<uint8_t>(msk + (int64_t)k * plane + src0, 1, n, m);
          store_bytes4(inter_msk + ((int64_t)b * K + k) * So + dst, m[0], m[1], m[2], m[3], n, vec);
        }
      }
      continue;
    }
    // cv2.warpAffine of the crop: AB_BITS = 10, INTER_BITS = 5; bilinear taps and the nearest mask tap per pixel
    const int64_t X0 = sat_lrint((M[1] * (double)oy + M[2]) * 1024.0), Y0 = sat_lrint((M[4] * (double)oy + M[5]) * 1024.0);
    int64_t near[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int x = q < n ? ox0 + q : ox0;
      const int64_t ax = sat_lrint(M[0] * (double)x * 1024.0), ay = sat_lrint(M[3] * (double)x * 1024.0);
      const int64_t X = (X0 + 16 + ax) >> 5, Y = (Y0 + 16 + ay) >> 5;
      const int cx = reflect_101((int)((X0 + 512 + ax) >> 10), Wo), cy = reflect_101((int)((Y0 + 512 + ay) >> 10), Ho);
      near[q] = base + cy * W64 + cx;
      if (img != nullptr) {
        const int sx = (int)(X >> 5), sy = (int)(Y >> 5);
        float w[4];
        bilinear_weights((float)(X & 31) / 32.f, (float)(Y & 31) / 32.f, w);
        const int64_t c0 = reflect_101(sx, Wo), c1 = reflect_101(sx + 1, Wo);
        const int64_t r0 = base + reflect_101(sy, Ho) * W64, r1 = base + reflect_101(sy + 1, Ho) * W64;
        const TI t00 = img[r0 + c0], t01 = img[r0 + c1], t10 = img[r1 + c0], t11 = img[r1 + c1];
#pragma unroll
        for (int c = 0; c < P2_CMAX; ++c) {
          if (c < win.C && q < n)
            inter_img[((int64_t)b * win.C + c) * So + dst + q] = bilinear_value(window_value<TI>(t00, win, c), window_value<TI>(t01, win, c),
                                                                                window_value<TI>(t10, win, c), window_value<TI>(t11, win, c), w);
        }
      }
    }
    if (msk != nullptr) {
      for (int k = 0; k < K; ++k) {
        const uint8_t* p = msk + (int64_t)k * plane;
        store_bytes4(inter_msk + ((int64_t)b * K + k) * So + dst, p[near[0]], p[near[1]], p[near[2]], p[near[3]], n, vec);
      }
    }
  }
}

// Pass 2.  Block (x, b) walks the 4-pixel groups of the OUTPUT of sample b; (r, c) is the pixel of the warped crop that rot90 and
// flip put there.
__global__ __launch_bounds__(256) void warp2d_pass2_kernel(const double* __restrict__ inter_img, const uint8_t* __restrict__ inter_msk,
                                                           const int64_t* __restrict__ table, Warp2dDims d, Pipe2dWin win,
                                                           const float* __restrict__ fields, const float* __restrict__ xx,
                                                           const float* __restrict__ yy, float* __restrict__ image_out,
                                                           uint8_t* __restrict__ masks_out, uint8_t* __restrict__ labels_out,
                                                           unsigned long long* __restrict__ hist, int* __restrict__ present) {
  __shared__ unsigned int s_h[P2_KMAX + 1];
  __shared__ unsigned int s_pres;
  const int b = blockIdx.y, tid = threadIdx.x;
  const int64_t* row = table + (int64_t)b * P2W_COLS;
  if (!warp_row_ok(row, d)) return;
  if (tid <= P2_KMAX) s_h[tid] = 0u;
  if (tid == 0) s_pres = 0u;
  __syncthreads();
  const int K = d.K, Ho = d.Ho, Wo = d.Wo;
  const int64_t So = (int64_t)Ho * Wo, kind = row[P2W_KIND], flip = row[P2_FLIP];
  const RotWalk rw = rot_walk(row[P2_ROT], Ho, Wo);      // an odd k has Ho == Wo
  const float* fx_tab = kind == W2_ELASTIC ? fields + row[P2W_SLOT] * 2 * So : xx + row[P2W_XX];
  const float* fy_tab = kind == W2_ELASTIC ? fields + (row[P2W_SLOT] * 2 + 1) * So : yy + row[P2W_YY];
  const bool img_vec = (Wo % 4 == 0) && (((uintptr_t)image_out % 16) == 0);
  const bool msk_vec = (Wo % 4 == 0) && (((uintptr_t)masks_out % 4) == 0) && (((uintptr_t)labels_out % 4) == 0);
  const bool want_lab = labels_out != nullptr || hist != nullptr;
  const int gpr = (Wo + 3) / 4;
  const int64_t ngroups = (int64_t)Ho * gpr;
  MaskTally tally;

  for (int64_t g = blockIdx.x * (int64_t)blockDim.x + tid; g < ngroups; g += (int64_t)gridDim.x * blockDim.x) {
    const int oy = (int)(g / gpr), ox0 = (int)(g % gpr) * 4;
    const int n = Wo - ox0 < 4 ? Wo - ox0 : 4;
    const int64_t dst = (int64_t)oy * Wo + ox0;
    int64_t t00[4], t01[4], t10[4], t11[4], near[4];     // element offsets inside one Ho x Wo plane
    float w[4][4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int j = q < n ? ox0 + q : ox0, jp = flip ? Wo - 1 - j : j;
      const int r = (int)(rw.cy0 + rw.yi * oy + rw.yj * jp), c = (int)(rw.cx0 + rw.xi * oy + rw.xj * jp);
      if (kind == W2_NONE) {
        near[q] = t00[q] = (int64_t)r * Wo + c;
        continue;
      }
      float map_x, map_y;
      if (kind == W2_ELASTIC) {
        map_x = (float)((double)c + (double)fx_tab[(int64_t)r * Wo + c]);
        map_y = (float)((double)r + (double)fy_tab[(int64_t)r * Wo + c]);
      } else {
        map_x = fx_tab[c];
        map_y = fy_tab[r];
      }
      // cv2.remap: INTER_BITS = 5 fixed point of the float32 map, round half to even
      const int sx = __float2int_rn(map_x * 32.f), sy = __float2int_rn(map_y * 32.f);
      const int ix = sx >> 5, iy = sy >> 5;
      bilinear_weights((float)(sx & 31) / 32.f, (float)(sy & 31) / 32.f, w[q]);
      const int64_t c0 = reflect_101(ix, Wo), c1 = reflect_101(ix + 1, Wo);
      const int64_t r0 = (int64_t)reflect_101(iy, Ho) * Wo, r1 = (int64_t)reflect_101(iy + 1, Ho) * Wo;
      t00[q] = r0 + c0; t01[q] = r0 + c1; t10[q] = r1 + c0; t11[q] = r1 + c1;
      near[q] = (int64_t)reflect_101(__float2int_rn(map_y), Ho) * Wo + reflect_101(__float2int_rn(map_x), Wo);
    }

    if (inter_img != nullptr && image_out != nullptr) {
#pragma unroll
      for (int c = 0; c < P2_CMAX; ++c) {
        if (c < win.C) {
          const double* p = inter_img + ((int64_t)b * win.C + c) * So;
          double val[4];
#pragma unroll
          for (int q = 0; q < 4; ++q)
            val[q] = kind == W2_NONE ? p[t00[q]] : bilinear_value(p[t00[q]], p[t01[q]], p[t10[q]], p[t11[q]], w[q]);
          store_image4(image_out + ((int64_t)b * win.C + c) * So + dst, val, win, c, n, img_vec);
        }
      }
    }

    if (inter_msk != nullptr) {
      int lab[4] = {0, 0, 0, 0};
      for (int k = 0; k < K; ++k) {
        const uint8_t* p = inter_msk + ((int64_t)b * K + k) * So;
        const uint8_t m[4] = {p[near[0]], p[near[1]], p[near[2]], p[near[3]]};
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

// the host's copy of the table, row by row: what the kernels would skip is an error here
static int check_warp_table(const int64_t* t, int B, const Warp2dDims& d) {
  int64_t last_slot = -1;
  for (int b = 0; b < B; ++b) {
    const int64_t* r = t + (int64_t)b * P2W_COLS;
    const int64_t H = r[P2_H], W = r[P2_W], k = r[P2_ROT], kind = r[P2W_KIND];
    CTSEG_REQUIRE(H > 0 && W > 0 && H < (1 << 24) && W < (1 << 24), "pipeline2d_warp_batch: sample %d: bad slice size", b);
    CTSEG_REQUIRE(!d.has_image || (r[P2_IMG] >= 0 && r[P2_IMG] + H * W <= d.image_elems),
                  "pipeline2d_warp_batch: sample %d: image outside its store", b);
    CTSEG_REQUIRE(!d.has_masks || (r[P2_MSK] >= 0 && r[P2_MSK] + (int64_t)d.K * H * W <= d.mask_bytes),
                  "pipeline2d_warp_batch: sample %d: masks outside their store", b);
    CTSEG_REQUIRE(k >= 0 && k <= 3 && (r[P2_FLIP] == 0 || r[P2_FLIP] == 1), "pipeline2d_warp_batch: sample %d: k in 0..3, flip in 0/1", b);
    CTSEG_REQUIRE(!(k & 1) || d.Ho == d.Wo, "pipeline2d_warp_batch: sample %d: rot90 by an odd k needs a square output (%d x %d)", b,
                  d.Ho, d.Wo);
    CTSEG_REQUIRE(r[P2_Y0] >= 0 && r[P2_X0] >= 0 && r[P2_Y0] + d.Ho <= H && r[P2_X0] + d.Wo <= W,
                  "pipeline2d_warp_batch: sample %d: crop (%lld, %lld) + %d x %d leaves the %lld x %lld slice", b, (long long)r[P2_Y0],
                  (long long)r[P2_X0], d.Ho, d.Wo, (long long)H, (long long)W);
    CTSEG_REQUIRE(kind == W2_NONE || kind == W2_ELASTIC || kind == W2_GRID, "pipeline2d_warp_batch: sample %d: kind %lld", b, (long long)kind);
    if (kind == W2_ELASTIC) {
      CTSEG_REQUIRE(r[P2W_SLOT] > last_slot && r[P2W_SLOT] < d.n_slots,
                    "pipeline2d_warp_batch: sample %d: field slot %lld (slots rise from 0 below %d)", b, (long long)r[P2W_SLOT], d.n_slots);
      last_slot = r[P2W_SLOT];
    } else if (kind == W2_GRID) {
      CTSEG_REQUIRE(r[P2W_XX] >= 0 && r[P2W_XX] + d.Wo <= d.xx_elems && r[P2W_YY] >= 0 && r[P2W_YY] + d.Ho <= d.yy_elems,
                    "pipeline2d_warp_batch: sample %d: grid tables outside their buffers", b);
    }
    if (!warp_row_ok(r, d)) { set_error("pipeline2d_warp_batch: sample %d: refused row", b); return -1; }
  }
  return 0;
}

}  // namespace ctseg

using namespace ctseg;

extern "C" int ctseg_pipeline2d_warp_batch(const void* image_store, int32_t image_dtype, int64_t image_elems, const uint8_t* mask_store,
                                           int64_t mask_bytes, const int64_t* table, const int64_t* table_host, int32_t B, int32_t K,
                                           int32_t Ho, int32_t Wo, int32_t C, const int32_t* win_lo, const int32_t* win_hi, int32_t shift,
                                           const float* mean, const float* denom, const double* gauss_w, int32_t radius, double alpha,
                                           const float* xx, int64_t xx_elems, const float* yy, int64_t yy_elems, float* fields,
                                           double* field_tmp, int32_t n_slots, void* inter, int64_t inter_bytes, float* image_out,
                                           uint8_t* masks_out, uint8_t* labels_out, int64_t* hist, int32_t* present, int32_t launches,
                                           void* stream) {
  const char* who = "pipeline2d_warp_batch";
  CTSEG_REQUIRE(table && table_host && B > 0 && B <= 65535 && (image_store || mask_store), "%s: bad arguments", who);
  CTSEG_REQUIRE(Ho > 0 && Wo > 0 && Ho <= W2_LINE_MAX && Wo <= W2_LINE_MAX, "%s: output %d x %d (1..%d per axis)", who, Ho, Wo, W2_LINE_MAX);
  CTSEG_REQUIRE(launches > 0 && launches <= (W2_FIELDS | W2_PASS1 | W2_PASS2), "%s: launches %d", who, launches);
  CTSEG_REQUIRE(!image_store || (image_out && C >= 1 && C <= P2_CMAX && win_lo && win_hi && image_elems > 0),
                "%s: an image needs image_out and 1..%d windows", who, P2_CMAX);
  CTSEG_REQUIRE(!image_store || is_raw_dtype(image_dtype), "%s: image dtype %d", who, image_dtype);
  CTSEG_REQUIRE((mean == nullptr) == (denom == nullptr), "%s: mean and denom come together", who);
  CTSEG_REQUIRE(!mask_store || (K > 0 && K <= P2_KMAX && mask_bytes > 0 && (masks_out || labels_out || present)),
                "%s: masks need K <= %d and an output", who, P2_KMAX);
  CTSEG_REQUIRE(mask_store || !(masks_out || labels_out || hist || present), "%s: mask outputs without masks", who);
  CTSEG_REQUIRE(!hist || labels_out, "%s: hist needs labels_out", who);
  CTSEG_REQUIRE(((uintptr_t)image_out % 4) == 0 && ((uintptr_t)image_store % (image_dtype == CTSEG_F32 ? 4 : image_dtype == CTSEG_I16 ? 2 : 1)) == 0,
                "%s: unaligned image pointer", who);
  CTSEG_REQUIRE(n_slots >= 0 && xx_elems >= 0 && yy_elems >= 0 && (xx || xx_elems == 0) && (yy || yy_elems == 0), "%s: bad table buffers", who);
  if (n_slots > 0) {
    CTSEG_REQUIRE(radius >= 0, "%s: radius %d", who, radius);
    CTSEG_REQUIRE(gauss_w && fields && field_tmp, "%s: elastic samples need the weights, the fields and their float64 scratch", who);
    CTSEG_REQUIRE((Ho > Wo ? Ho : Wo) + 2 * (int64_t)radius <= W2_LDS_DOUBLES, "%s: radius %d: a line and its margins exceed %d doubles", who,
                  radius, W2_LDS_DOUBLES);
    CTSEG_REQUIRE(((uintptr_t)gauss_w % 8) == 0 && ((uintptr_t)field_tmp % 8) == 0 && ((uintptr_t)fields % 4) == 0, "%s: unaligned field buffers", who);
  }
  const int64_t So = (int64_t)Ho * Wo;
  const int Ci = image_store ? C : 0, Ki = mask_store ? K : 0;
  CTSEG_REQUIRE(inter && ((uintptr_t)inter % 8) == 0 && inter_bytes >= (int64_t)B * (Ci * 8 + Ki) * So,
                "%s: the intermediate needs B * (C * 8 + K) * Ho * Wo = %lld bytes, 8-byte aligned", who, (long long)((int64_t)B * (Ci * 8 + Ki) * So));
  Warp2dDims d;
  d.K = K; d.Ho = Ho; d.Wo = Wo; d.n_slots = n_slots; d.has_image = image_store != nullptr; d.has_masks = mask_store != nullptr;
  d.image_elems = image_elems; d.mask_bytes = mask_bytes; d.xx_elems = xx_elems; d.yy_elems = yy_elems;
  if (check_warp_table(table_host, B, d)) return -1;
  Pipe2dWin w;
  if (fill_windows(w, who, Ci, win_lo, win_hi, shift, mean, denom)) return -1;
  double* inter_img = (double*)inter;
  uint8_t* inter_msk = mask_store ? (uint8_t*)inter + (int64_t)B * Ci * 8 * So : nullptr;
  const int64_t ngroups = (int64_t)Ho * ((Wo + 3) / 4);
  int64_t blocks = (ngroups + 255) / 256;
  if (blocks > 64) blocks = 64;
  const dim3 grid((unsigned)blocks, B);
  hipStream_t st = (hipStream_t)stream;
  if ((launches & W2_FIELDS) && n_slots > 0)
    hipLaunchKernelGGL(warp2d_fields_kernel, dim3(2, B), dim3(W2_FIELD_THREADS), 0, st, table, d, gauss_w, radius, alpha, field_tmp, fields);
  if (launches & W2_PASS1)      // (a call without an image may carry any dtype code: one that names no pixel type takes the float kernel)
    with_raw_dtype(is_raw_dtype(image_dtype) ? image_dtype : CTSEG_F32, [&](auto ti) {
      using TI = decltype(ti);
      hipLaunchKernelGGL((warp2d_pass1_kernel<TI>), grid, dim3(256), 0, st, (const TI*)image_store, mask_store, table, d, w, inter_img,
                         inter_msk);
    });
  if (launches & W2_PASS2)
    hipLaunchKernelGGL(warp2d_pass2_kernel, grid, dim3(256), 0, st, image_store ? inter_img : nullptr, inter_msk, table, d, w, fields, xx, yy,
                       image_out, masks_out, labels_out, (unsigned long long*)hist, present);
  CTSEG_LAUNCH_CHECK(who);
  return 0;
}
