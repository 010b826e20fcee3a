// The tile of the 3-D augmentation pass, shared by augment3d.hip (affine only) and deform3d.hip (affine + B-spline lattice): the
// arguments, the entry's validation and the two-phase workgroup body.  One workgroup = one h, a 64-wide w tile and a 32-deep d tile.
// Phase 1 has lanes along output w (with the small rotations of an augmentation neighbouring lanes read neighbouring source w, the
// source's contiguous axis), phase 2 has lanes along d, the output's contiguous axis; the transposition goes through LDS, rows padded
// to an odd dword count.  Every float operation is one float32 rounding: nothing may be contracted into an FMA.
#pragma once
#pragma clang fp contract(off)
#include <cmath>

#include "ctseg_dev.h"

namespace ctseg {

constexpr int AG_TW = 64, AG_TD = 32, AG_KMAX = 15;
// the h-collapsed lattice slab of a tile: cells are at least 4 voxels, so 32 voxels along d touch at most 9 cells (12 rows of
// control points) and 64 along w at most 17 (20 rows)
constexpr int DF_RD = 12, DF_RW = 20;

// everything a lane needs besides pointers, in the kernel's arguments (scalar registers): no table in memory
struct Aug3dArgs {
  int K, D, H, W, Do, Ho, Wo, border, window, apply_gain;
  float sD, sH, sW;                  // (float)in / out per axis, the resize's scales
  float a[12];                       // row-major 3 x 4, rows and columns ordered d, h, w (read with constant indices only)
  float cval, win_lo, win_hi, gain, bias;
  unsigned long long perm;           // 4 bits per output channel: its input channel
};

// the control lattice [3][Gd+3][Gh+3][Gw+3] of the deformed pass
struct Deform3dArgs {
  int Gd, Gh, Gw;
  float gd, gh, gw;                  // (float)G / (float)out per axis: output voxel -> lattice coordinate
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

// one axis of the lattice: output index o -> cell i = min((int)floorf(u), G - 1), u = (float)o * g, and the four cubic B-spline
// weights of t = u - (float)i
__device__ __forceinline__ int df_axis(int o, float g, int G, float B[4]) {
  const float u = (float)o * g;
  int i = (int)floorf(u);
  i = i < G - 1 ? i : G - 1;
  const float t = u - (float)i, s = 1.f - t;
  B[0] = ((s * s) * s) / 6.f;
  B[1] = ((((3.f * t - 6.f) * t) * t) + 4.f) / 6.f;
  B[2] = (((((-3.f * t + 3.f) * t) + 3.f) * t) + 1.f) / 6.f;
  B[3] = ((t * t) * t) / 6.f;
  return i;
}
// the cell alone
__device__ __forceinline__ int df_cell(int o, float g, int G) {
  const int i = (int)floorf((float)o * g);
  return i < G - 1 ? i : G - 1;
}

// DEFORM: `lattice` and `dg` are read, and the sampling coordinate gains the lattice's displacement; otherwise neither is touched
template <typename TI, int INTERP, bool DEFORM>
__device__ __forceinline__ void augment3d_tile(const TI* __restrict__ image, const uint8_t* __restrict__ masks, const Aug3dArgs p,
                                               float* __restrict__ image_out, uint8_t* __restrict__ masks_out,
                                               uint8_t* __restrict__ labels_out, unsigned long long* __restrict__ hist,
                                               const float* __restrict__ lattice, const Deform3dArgs dg) {
  __shared__ float s_img[AG_TD][AG_TW + 1];
  __shared__ uint8_t s_lab[AG_TD][AG_TW + 4];
  __shared__ unsigned short s_bits[AG_TD][AG_TW + 2];      // bit k = output mask k at this voxel (masks_out only)
  __shared__ unsigned int s_h[AG_KMAX + 1];
  // P[c][row_d][row_w] = sum_e Bh[e] * L[c][rd0 + row_d][ih + e][rw0 + row_w]: a workgroup has one h.  A wave of phase 1 has one
  // row_d and its 64 lanes at most 17 consecutive row_w: every read is a broadcast over distinct banks
  __shared__ float s_slab[DEFORM ? 3 : 1][DEFORM ? DF_RD : 1][DEFORM ? DF_RW : 1];
  const int t = threadIdx.x;
  const int K = p.K, D = p.D, H = p.H, W = p.W, Do = p.Do, Ho = p.Ho, Wo = p.Wo;
  const int ndt = (Do + AG_TD - 1) / AG_TD;
  const int d0 = (blockIdx.x % ndt) * AG_TD, w0 = (blockIdx.x / ndt) * AG_TW, h = blockIdx.y;
  if (t <= AG_KMAX) s_h[t] = 0;
  int rd0 = 0, rw0 = 0;
  if constexpr (DEFORM) {
    float Bh[4];
    const int ih = df_axis(h, dg.gh, dg.Gh, Bh);
    rd0 = df_cell(d0, dg.gd, dg.Gd), rw0 = df_cell(w0, dg.gw, dg.Gw);
    const int d1 = d0 + AG_TD - 1 < Do - 1 ? d0 + AG_TD - 1 : Do - 1, w1 = w0 + AG_TW - 1 < Wo - 1 ? w0 + AG_TW - 1 : Wo - 1;
    int nrd = df_cell(d1, dg.gd, dg.Gd) - rd0 + 4, nrw = df_cell(w1, dg.gw, dg.Gw) - rw0 + 4;
    nrd = nrd < DF_RD ? nrd : DF_RD, nrw = nrw < DF_RW ? nrw : DF_RW;       // (the entry's 4 * G <= out keeps them below anyway)
    const int Lh = dg.Gh + 3, Lw = dg.Gw + 3;
    const int64_t comp = (int64_t)(dg.Gd + 3) * Lh * Lw;
    for (int e = t; e < 3 * nrd * nrw; e += 256) {
      const int c = e / (nrd * nrw), rem = e - c * (nrd * nrw), rd = rem / nrw, rw = rem - rd * nrw;
      const float* L = lattice + c * comp + ((int64_t)(rd0 + rd) * Lh + ih) * Lw + (rw0 + rw);
      s_slab[c][rd][rw] = ((Bh[0] * L[0] + Bh[1] * L[Lw]) + Bh[2] * L[2 * Lw]) + Bh[3] * L[3 * Lw];
    }
  }
  __syncthreads();
  {
    const int ww = t & 63, w = w0 + ww;
    const float fh = (float)h, fw = (float)w;
    const int HW = H * W;
    float Bw[4];
    int jw = 0;
    if constexpr (DEFORM) {
      jw = df_axis(w, dg.gw, dg.Gw, Bw) - rw0;
      jw = jw < 0 ? 0 : (jw > DF_RW - 4 ? DF_RW - 4 : jw);                  // (lanes past Wo: they store nothing, and read inside)
    }
    for (int r = 0; r < AG_TD / 4; ++r) {
      const int dd = r * 4 + (t >> 6), d = d0 + dd;
      if (w >= Wo || d >= Do) continue;
      const float fd = (float)d;
      float qd = ((p.a[0] * fd + p.a[1] * fh) + p.a[2] * fw) + p.a[3];
      float qh = ((p.a[4] * fd + p.a[5] * fh) + p.a[6] * fw) + p.a[7];
      float qw = ((p.a[8] * fd + p.a[9] * fh) + p.a[10] * fw) + p.a[11];
      if constexpr (DEFORM) {
        float Bd[4];
        int jd = df_axis(d, dg.gd, dg.Gd, Bd) - rd0;
        jd = jd < 0 ? 0 : (jd > DF_RD - 4 ? DF_RD - 4 : jd);
        float s[3];
        for (int c = 0; c < 3; ++c) {
          float along_d[4];
          for (int a = 0; a < 4; ++a) {
            const float* P = &s_slab[c][jd + a][jw];
            along_d[a] = ((Bw[0] * P[0] + Bw[1] * P[1]) + Bw[2] * P[2]) + Bw[3] * P[3];
          }
          s[c] = ((Bd[0] * along_d[0] + Bd[1] * along_d[1]) + Bd[2] * along_d[2]) + Bd[3] * along_d[3];
        }
        qd = qd + s[0], qh = qh + s[1], qw = qw + s[2];
      }
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

// What ctseg_augment3d_to_hwd asks of its arguments, and the kernel's argument block and grid; `who` names the entry in messages
inline int augment3d_prepare(const char* who, const void* image, int32_t image_dtype, const uint8_t* masks, int32_t K, int32_t D,
                             int32_t H, int32_t W, int32_t Do, int32_t Ho, int32_t Wo, const float* matrix, int32_t interp,
                             int32_t border, float cval, const int32_t* mask_src, int32_t window, float win_lo, float win_hi, float gain,
                             float bias, const float* image_out, const uint8_t* masks_out, const uint8_t* labels_out,
                             const int64_t* hist, Aug3dArgs& p, dim3& grid) {
  CTSEG_REQUIRE(D > 0 && H > 0 && W > 0 && Do > 0 && Ho > 0 && Wo > 0 && (image || masks), "%s: bad geometry", who);
  CTSEG_REQUIRE((int64_t)D * H * W < (1ll << 31) && (int64_t)Do * Ho * Wo < (1ll << 31), "%s: a volume of 2^31 voxels or more", who);
  CTSEG_REQUIRE(!image || image_out, "%s: image without image_out", who);
  CTSEG_REQUIRE(!masks || (K > 0 && K <= AG_KMAX && (masks_out || labels_out)), "%s: masks need K <= 15 and an output", who);
  CTSEG_REQUIRE(!hist || labels_out, "%s: hist needs labels_out", who);
  CTSEG_REQUIRE(window >= 0 && window <= 2 && (!window || win_hi > win_lo), "%s: bad window", who);
  CTSEG_REQUIRE(image_dtype == CTSEG_F32 || image_dtype == CTSEG_I16 || image_dtype == CTSEG_U8, "%s: image dtype %d", who, image_dtype);
  CTSEG_REQUIRE(interp == 0 || interp == 1, "%s: interp %d is neither 0 (nearest) nor 1 (trilinear)", who, interp);
  CTSEG_REQUIRE(border == 0 || border == 1, "%s: border %d is neither 0 (constant) nor 1 (edge)", who, border);
  CTSEG_REQUIRE(matrix, "%s: matrix is a null pointer", who);
  const int out[3] = {Do, Ho, Wo};
  for (int a = 0; a < 3; ++a) {
    // finite entries, and coordinates that stay far inside float32 over the whole output grid: no inf - inf in the kernel
    double reach = 0.0;
    for (int j = 0; j < 4; ++j) {
      const float v = matrix[a * 4 + j];
      CTSEG_REQUIRE(std::isfinite(v), "%s: matrix entry [%d][%d] is not finite", who, a, j);
      reach += fabs((double)v) * (j < 3 ? (double)(out[j] - 1) : 1.0);
      p.a[a * 4 + j] = v;
    }
    CTSEG_REQUIRE(reach < 1e30, "%s: matrix row %d sends the output grid beyond 1e30", who, a);
  }
  CTSEG_REQUIRE(std::isfinite(cval), "%s: cval is not finite", who);
  CTSEG_REQUIRE(std::isfinite(gain) && std::isfinite(bias), "%s: gain / bias is not finite", who);
  p.perm = 0;
  unsigned seen = 0;
  for (int k = 0; k < (masks ? K : 0); ++k) {
    const int s = mask_src ? mask_src[k] : k;
    CTSEG_REQUIRE(s >= 0 && s < K && !((seen >> s) & 1u), "%s: mask_src is not a permutation of 0..%d (entry %d = %d)", who, K - 1, k, s);
    seen |= 1u << s;
    p.perm |= (unsigned long long)s << (4 * k);
  }
  p.K = masks ? K : 0, p.D = D, p.H = H, p.W = W, p.Do = Do, p.Ho = Ho, p.Wo = Wo, p.border = border, p.window = window;
  p.apply_gain = !(gain == 1.f && bias == 0.f);
  p.sD = (float)D / (float)Do, p.sH = (float)H / (float)Ho, p.sW = (float)W / (float)Wo;
  p.cval = cval, p.win_lo = win_lo, p.win_hi = win_hi, p.gain = gain, p.bias = bias;
  grid = dim3(((Do + AG_TD - 1) / AG_TD) * ((Wo + AG_TW - 1) / AG_TW), Ho);
  return 0;
}

}  // namespace ctseg
