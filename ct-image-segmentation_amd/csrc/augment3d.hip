// 3-D augmentation in the input pipeline's one pass per instance: the nearest Resize3D + (D,H,W)->(H,W,D) + window + squash of
// resize3d_hwd_kernel (loss_metric.hip), with the output voxel sent through a 3 x 4 affine matrix first, the mask channels through
// a permutation, and the windowed value through gain / bias.  The rules are in include/ctseg_hip.h (ctseg_augment3d_to_hwd).
// The same tile as the resize: one workgroup = one h, a 64-wide w tile and a 32-deep d tile.  Phase 1 has lanes along output w
// (with the small rotations of an augmentation neighbouring lanes read neighbouring source w, the source's contiguous axis),
// phase 2 has lanes along d, the output's contiguous axis; the transposition goes through LDS, rows padded to an odd dword count.
// Every float operation is one float32 rounding: nothing may be contracted into an FMA.
#pragma clang fp contract(off)
#include <cmath>

#include "ctseg_dev.h"

namespace ctseg {

constexpr int AG_TW = 64, AG_TD = 32, AG_KMAX = 15;

// everything a lane needs besides pointers, in the kernel's arguments (scalar registers): no table in memory
struct Aug3dArgs {
  int K, D, H, W, Do, Ho, Wo, border, window, apply_gain;
  float sD, sH, sW;                  // (float)in / out per axis, the resize's scales
  float a[12];                       // row-major 3 x 4, rows and columns ordered d, h, w (read with constant indices only)
  float cval, win_lo, win_hi, gain, bias;
  unsigned long long perm;           // 4 bits per output channel: its input channel
};

// the resize's nearest rule
__device__ __forceinline__ int ag_rz(int dst, float scale, int in) {
  const int s = (int)floorf((float)dst * scale);
  return s < in - 1 ? s : in - 1;
}

// one axis of the virtual resized volume: grid coordinate g (a whole float), clamped into [-1, out] before the conversion so that
// no float outside the int range is converted; -> source index, and whether g was inside [0, out)
__device__ __forceinline__ int ag_axis(float g, int out, int in, float scale, int border, bool& ok) {
  int r = (int)fminf(fmaxf(g, -1.f), (float)out);
  ok = r >= 0 && r < out;
  if (border) {
    r = r < 0 ? 0 : (r > out - 1 ? out - 1 : r);
    ok = true;
  }
  return ag_rz(ok ? r : 0, scale, in);
}

__device__ __forceinline__ float ag_lerp(float x, float y, float t) { return x + t * (y - x); }

template <typename TI, int INTERP>
__global__ __launch_bounds__(256) void augment3d_hwd_kernel(const TI* __restrict__ image, const uint8_t* __restrict__ masks, const Aug3dArgs p,
                                                            float* __restrict__ image_out, uint8_t* __restrict__ masks_out,
                                                            uint8_t* __restrict__ labels_out, unsigned long long* __restrict__ hist) {
  __shared__ float s_img[AG_TD][AG_TW + 1];
  __shared__ uint8_t s_lab[AG_TD][AG_TW + 4];
  __shared__ unsigned short s_bits[AG_TD][AG_TW + 2];      // bit k = output mask k at this voxel (masks_out only)
  __shared__ unsigned int s_h[AG_KMAX + 1];
  const int t = threadIdx.x;
  const int K = p.K, D = p.D, H = p.H, W = p.W, Do = p.Do, Ho = p.Ho, Wo = p.Wo;
  const int ndt = (Do + AG_TD - 1) / AG_TD;
  const int d0 = (blockIdx.x % ndt) * AG_TD, w0 = (blockIdx.x / ndt) * AG_TW, h = blockIdx.y;
  if (t <= AG_KMAX) s_h[t] = 0;
  __syncthreads();
  {
    const int ww = t & 63, w = w0 + ww;
    const float fh = (float)h, fw = (float)w;
    const int HW = H * W;
    for (int r = 0; r < AG_TD / 4; ++r) {
      const int dd = r * 4 + (t >> 6), d = d0 + dd;
      if (w >= Wo || d >= Do) continue;
      const float fd = (float)d;
      const float qd = ((p.a[0] * fd + p.a[1] * fh) + p.a[2] * fw) + p.a[3];
      const float qh = ((p.a[4] * fd + p.a[5] * fh) + p.a[6] * fw) + p.a[7];
      const float qw = ((p.a[8] * fd + p.a[9] * fh) + p.a[10] * fw) + p.a[11];
      bool okd, okh, okw;
      const int nd = ag_axis(floorf(qd + 0.5f), Do, D, p.sD, p.border, okd);
      const int nh = ag_axis(floorf(qh + 0.5f), Ho, H, p.sH, p.border, okh);
      const int nw = ag_axis(floorf(qw + 0.5f), Wo, W, p.sW, p.border, okw);
      const bool inside = okd && okh && okw;
      const int src = (nd * H + nh) * W + nw;               // < 2^31: the entry checks D * H * W
      if (image) {
        float v;
        if (INTERP == 0) {
          v = inside ? (float)image[(unsigned)src] : p.cval;
        } else {
          const float bd = floorf(qd), bh = floorf(qh), bw = floorf(qw);
          const float td = qd - bd, th = qh - bh, tw = qw - bw;
          bool od[2], oh[2], ow[2];
          int id[2], ih[2], iw[2];
          for (int c = 0; c < 2; ++c) {
            // b is clamped to [-2, out] first, so that b + 1 stays a small whole number on the outside it belongs to
            id[c] = ag_axis(fminf(fmaxf(bd, -2.f), (float)Do) + (float)c, Do, D, p.sD, p.border, od[c]) * HW;
            ih[c] = ag_axis(fminf(fmaxf(bh, -2.f), (float)Ho) + (float)c, Ho, H, p.sH, p.border, oh[c]) * W;
            iw[c] = ag_axis(fminf(fmaxf(bw, -2.f), (float)Wo) + (float)c, Wo, W, p.sW, p.border, ow[c]);
          }
          float cd[2];
          for (int a = 0; a < 2; ++a) {
            float ch[2];
            for (int b = 0; b < 2; ++b) {
              const int base = id[a] + ih[b];
              const bool ok = od[a] && oh[b];
              const float x = ok && ow[0] ? (float)image[(unsigned)(base + iw[0])] : p.cval;
              const float y = ok && ow[1] ? (float)image[(unsigned)(base + iw[1])] : p.cval;
              ch[b] = ag_lerp(x, y, tw);
            }
            cd[a] = ag_lerp(ch[0], ch[1], th);
          }
          v = ag_lerp(cd[0], cd[1], td);
        }
        if (p.window) {
          v = fminf(fmaxf(v, p.win_lo), p.win_hi);
          if (p.window == 2) v = (v - p.win_lo) / (float)((double)p.win_hi - (double)p.win_lo + 1e-8);   // as the resize kernel
        }
        if (p.apply_gain) v = v * p.gain + p.bias;
        s_img[dd][ww] = v;
      }
      if (masks) {
        int lab = 0;
        unsigned bits = 0;
        if (inside) {
          for (int k = 0; k < K; ++k) {
            const int ch = (int)((p.perm >> (4 * k)) & 15ull);        // wave-uniform: the channel's base stays scalar
            const int m = (masks + (int64_t)ch * D * HW)[(unsigned)src];
            bits |= (m ? 1u : 0u) << k;
            const int val = m * (k + 1);
            lab = val > lab ? val : lab;
          }
        }
        s_lab[dd][ww] = (uint8_t)lab;
        s_bits[dd][ww] = (unsigned short)bits;
        if (hist) atomicAdd(&s_h[lab & AG_KMAX], 1u);
      }
    }
  }
  __syncthreads();
  {
    const int dd = t & 31, d = d0 + dd;
    const int64_t plane = (int64_t)Ho * Wo * Do;
    for (int r = 0; r < AG_TW / 8; ++r) {
      const int ww = r * 8 + (t >> 5), w = w0 + ww;
      if (w >= Wo || d >= Do) continue;
      const int dst = (h * Wo + w) * Do + d;                  // < 2^31: the entry checks Do * Ho * Wo
      if (image) image_out[dst] = s_img[dd][ww];
      if (masks) {
        if (labels_out) labels_out[dst] = s_lab[dd][ww];
        if (masks_out) {
          const unsigned bits = s_bits[dd][ww];
          for (int k = 0; k < K; ++k) masks_out[k * plane + dst] = (uint8_t)((bits >> k) & 1u);
        }
      }
    }
  }
  __syncthreads();
  if (hist && t <= K && s_h[t]) atomicAdd(&hist[t], (unsigned long long)s_h[t]);
}

}  // namespace ctseg

using namespace ctseg;

extern "C" int ctseg_augment3d_to_hwd(const void* image, int32_t image_dtype, const uint8_t* masks, int32_t K, int32_t D, int32_t H,
                                      int32_t W, int32_t Do, int32_t Ho, int32_t Wo, const float* matrix, int32_t interp, int32_t border,
                                      float cval, const int32_t* mask_src, int32_t window, float win_lo, float win_hi, float gain,
                                      float bias, float* image_out, uint8_t* masks_out, uint8_t* labels_out, int64_t* hist,
                                      void* stream) {
  CTSEG_REQUIRE(D > 0 && H > 0 && W > 0 && Do > 0 && Ho > 0 && Wo > 0 && (image || masks), "augment3d_to_hwd: bad geometry");
  CTSEG_REQUIRE((int64_t)D * H * W < (1ll << 31) && (int64_t)Do * Ho * Wo < (1ll << 31), "augment3d_to_hwd: a volume of 2^31 voxels or more");
  CTSEG_REQUIRE(!image || image_out, "augment3d_to_hwd: image without image_out");
  CTSEG_REQUIRE(!masks || (K > 0 && K <= AG_KMAX && (masks_out || labels_out)), "augment3d_to_hwd: masks need K <= 15 and an output");
  CTSEG_REQUIRE(!hist || labels_out, "augment3d_to_hwd: hist needs labels_out");
  CTSEG_REQUIRE(window >= 0 && window <= 2 && (!window || win_hi > win_lo), "augment3d_to_hwd: bad window");
  CTSEG_REQUIRE(image_dtype == CTSEG_F32 || image_dtype == CTSEG_I16 || image_dtype == CTSEG_U8, "augment3d_to_hwd: image dtype %d", image_dtype);
  CTSEG_REQUIRE(interp == 0 || interp == 1, "augment3d_to_hwd: interp %d is neither 0 (nearest) nor 1 (trilinear)", interp);
  CTSEG_REQUIRE(border == 0 || border == 1, "augment3d_to_hwd: border %d is neither 0 (constant) nor 1 (edge)", border);
  CTSEG_REQUIRE(matrix, "augment3d_to_hwd: matrix is a null pointer");
  Aug3dArgs p;
  const int out[3] = {Do, Ho, Wo};
  for (int a = 0; a < 3; ++a) {
    // finite entries, and coordinates that stay far inside float32 over the whole output grid: no inf - inf in the kernel
    double reach = 0.0;
    for (int j = 0; j < 4; ++j) {
      const float v = matrix[a * 4 + j];
      CTSEG_REQUIRE(std::isfinite(v), "augment3d_to_hwd: matrix entry [%d][%d] is not finite", a, j);
      reach += fabs((double)v) * (j < 3 ? (double)(out[j] - 1) : 1.0);
      p.a[a * 4 + j] = v;
    }
    CTSEG_REQUIRE(reach < 1e30, "augment3d_to_hwd: matrix row %d sends the output grid beyond 1e30", a);
  }
  CTSEG_REQUIRE(std::isfinite(cval), "augment3d_to_hwd: cval is not finite");
  CTSEG_REQUIRE(std::isfinite(gain) && std::isfinite(bias), "augment3d_to_hwd: gain / bias is not finite");
  p.perm = 0;
  unsigned seen = 0;
  for (int k = 0; k < (masks ? K : 0); ++k) {
    const int s = mask_src ? mask_src[k] : k;
    CTSEG_REQUIRE(s >= 0 && s < K && !((seen >> s) & 1u), "augment3d_to_hwd: mask_src is not a permutation of 0..%d (entry %d = %d)", K - 1, k, s);
    seen |= 1u << s;
    p.perm |= (unsigned long long)s << (4 * k);
  }
  p.K = masks ? K : 0, p.D = D, p.H = H, p.W = W, p.Do = Do, p.Ho = Ho, p.Wo = Wo, p.border = border, p.window = window;
  p.apply_gain = !(gain == 1.f && bias == 0.f);
  p.sD = (float)D / (float)Do, p.sH = (float)H / (float)Ho, p.sW = (float)W / (float)Wo;
  p.cval = cval, p.win_lo = win_lo, p.win_hi = win_hi, p.gain = gain, p.bias = bias;
  dim3 grid(((Do + AG_TD - 1) / AG_TD) * ((Wo + AG_TW - 1) / AG_TW), Ho);
  hipStream_t st = (hipStream_t)stream;
#define CTSEG_AG_LAUNCH(TI)                                                                                                          \
  do {                                                                                                                               \
    if (interp)                                                                                                                      \
      hipLaunchKernelGGL((augment3d_hwd_kernel<TI, 1>), grid, dim3(256), 0, st, (const TI*)image, masks, p, image_out, masks_out, \
                         labels_out, (unsigned long long*)hist);                                                                     \
    else                                                                                                                             \
      hipLaunchKernelGGL((augment3d_hwd_kernel<TI, 0>), grid, dim3(256), 0, st, (const TI*)image, masks, p, image_out, masks_out, \
                         labels_out, (unsigned long long*)hist);                                                                     \
  } while (0)
  if (image_dtype == CTSEG_F32) CTSEG_AG_LAUNCH(float);
  else if (image_dtype == CTSEG_I16) CTSEG_AG_LAUNCH(short);
  else CTSEG_AG_LAUNCH(uint8_t);
#undef CTSEG_AG_LAUNCH
  CTSEG_LAUNCH_CHECK("augment3d_to_hwd");
  return 0;
}
