// The tile of the 3-D resample passes of the input pipeline, shared by resize3d.hip (nearest resize), augment3d.hip (affine),
// deform3d.hip (affine + B-spline lattice) and patch3d.hip (affine on the source grid, about a device-side centre): the arguments,
// the entries' shared validation and the two-phase workgroup body.  One workgroup = one h, a 64-wide w tile and a 32-deep d tile.  Phase 1 has lanes along output w (the resize, and the small rotations
// of an augmentation, make neighbouring lanes read neighbouring source w, the source's contiguous axis), phase 2 has lanes along d,
// the output's contiguous axis; the transposition goes through LDS, rows padded to an odd dword count.  Where the source voxel
// comes from is a compile-time choice (Coord); from the fetched value on the passes are one text.
// Every float operation is one float32 rounding: nothing may be contracted into an FMA.
#pragma once
#pragma clang fp contract(off)
#include <cmath>
#include <type_traits>

#include "affine3d.h"

namespace ctseg {

constexpr int RS_TW = 64, RS_TD = 32, RS_KMAX = 15;
// the h-collapsed lattice slab of a tile: cells are at least 4 voxels, so 32 voxels along d touch at most 9 cells (12 rows of
// control points) and 64 along w at most 17 (20 rows)
constexpr int DF_RD = 12, DF_RW = 20;

// The coordinate source of a pass:
//   RESIZE   the separable nearest index of the output voxel itself, 64-bit offsets: no limit on the volumes
//   AFFINE   the output voxel goes through a 3 x 4 matrix first; 32-bit per-lane offsets (the entry checks 2^31 voxels)
//   LATTICE  AFFINE, and the sampling coordinate gains the displacement of a control lattice
//   PATCH    AFFINE with the matrix addressing the SOURCE grid itself (D x H x W, every scale 1): the output dims only tile the
//            pass and lay out its stores (patch3d.hip, whose kernel moves the translation column by a centre it reads)
enum class Coord { RESIZE, AFFINE, LATTICE, PATCH };

// everything a lane needs besides pointers, in the kernel's arguments (scalar registers): no table in memory
struct Resize3dArgs {
  int K, D, H, W, Do, Ho, Wo, window;
  float sD, sH, sW;                  // (float)in / out per axis, the resize's scales
  float win_lo, win_hi;
};
struct Aug3dArgs : Resize3dArgs {
  int border, apply_gain;
  Affine3d m;                        // output voxel -> the point it samples, on the grid the matrix addresses: the virtual resized
                                     // volume (Do x Ho x Wo), or the source grid itself for Coord::PATCH
  float cval, gain, bias;
  unsigned long long perm;           // 4 bits per output channel: its input channel
};

// the control lattice [3][Gd+3][Gh+3][Gw+3] of the deformed pass
struct Deform3dArgs {
  int Gd, Gh, Gw;
  float gd, gh, gw;                  // (float)G / (float)out per axis: output voxel -> lattice coordinate
};

// the resize's nearest rule, torch's: src = min((int)floorf(dst * ((float)in / out)), in - 1)
__device__ __forceinline__ int nearest_src(int dst, float scale, int in) {
  const int s = (int)floorf((float)dst * scale);
  return s < in - 1 ? s : in - 1;
}

// one axis of the virtual resized volume: grid coordinate g (a whole float) -> source index, and whether g was inside [0, out).
// (The conversion stays in here: handed the index instead, the kernels keep the ok flags in vector registers, 1-2 more each.)
__device__ __forceinline__ int ag_axis(float g, int out, int in, float scale, int border, bool& ok) {
  int r = affine3d_index(g, out);
  ok = r >= 0 && r < out;
  if (border) {
    r = r < 0 ? 0 : (r > out - 1 ? out - 1 : r);
    ok = true;
  }
  return nearest_src(ok ? r : 0, scale, in);
}

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

// Args = Resize3dArgs for RESIZE (INTERP is not read), Aug3dArgs otherwise; `lattice` and `dg` are touched by LATTICE alone
template <Coord SRC, typename TI, int INTERP, class Args>
__device__ __forceinline__ void resample3d_tile(const TI* __restrict__ image, const uint8_t* __restrict__ masks, const Args p,
                                                float* __restrict__ image_out, uint8_t* __restrict__ masks_out,
                                                uint8_t* __restrict__ labels_out, unsigned long long* __restrict__ hist,
                                                const float* __restrict__ lattice, const Deform3dArgs dg) {
  constexpr bool RESIZE = SRC == Coord::RESIZE, DEFORM = SRC == Coord::LATTICE, PATCH = SRC == Coord::PATCH;
  static_assert(std::is_same<Args, std::conditional_t<RESIZE, Resize3dArgs, Aug3dArgs>>::value, "the argument block of the source");
  using Off = std::conditional_t<RESIZE, int64_t, int>;          // an offset into a volume
  using SrcOff = std::conditional_t<RESIZE, int64_t, unsigned>;   // the source voxel's, zero-extended where it is 32-bit
  __shared__ float s_img[RS_TD][RS_TW + 1];
  __shared__ uint8_t s_lab[RS_TD][RS_TW + 4];
  __shared__ unsigned short s_bits[RS_TD][RS_TW + 2];      // bit k = output mask k at this voxel (masks_out only)
  __shared__ unsigned int s_h[RS_KMAX + 1];
  // P[c][row_d][row_w] = sum_e Bh[e] * L[c][rd0 + row_d][ih + e][rw0 + row_w]: a workgroup has one h.  A wave of phase 1 has one
  // row_d and its 64 lanes at most 17 consecutive row_w: every read is a broadcast over distinct banks
  __shared__ float s_slab[DEFORM ? 3 : 1][DEFORM ? DF_RD : 1][DEFORM ? DF_RW : 1];
  const int t = threadIdx.x;
  const int K = p.K, D = p.D, H = p.H, W = p.W, Do = p.Do, Ho = p.Ho, Wo = p.Wo;
  const int Vd = PATCH ? D : Do, Vh = PATCH ? H : Ho, Vw = PATCH ? W : Wo;      // the grid the matrix addresses
  const int ndt = (Do + RS_TD - 1) / RS_TD;
  const int d0 = (blockIdx.x % ndt) * RS_TD, w0 = (blockIdx.x / ndt) * RS_TW, h = blockIdx.y;
  if (t <= RS_KMAX) s_h[t] = 0;
  int rd0 = 0, rw0 = 0;
  if constexpr (DEFORM) {
    float Bh[4];
    const int ih = df_axis(h, dg.gh, dg.Gh, Bh);
    rd0 = df_cell(d0, dg.gd, dg.Gd), rw0 = df_cell(w0, dg.gw, dg.Gw);
    const int d1 = d0 + RS_TD - 1 < Do - 1 ? d0 + RS_TD - 1 : Do - 1, w1 = w0 + RS_TW - 1 < Wo - 1 ? w0 + RS_TW - 1 : Wo - 1;
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
    const Off HW = (Off)H * W;
    int sh = 0, sw = 0;                                     // RESIZE: the source h of the workgroup and the source w of the lane
    if constexpr (RESIZE) sh = nearest_src(h, p.sH, H), sw = nearest_src(w < Wo ? w : Wo - 1, p.sW, W);
    const float fh = (float)h, fw = (float)w;
    float Bw[4];
    int jw = 0;
    if constexpr (DEFORM) {
      jw = df_axis(w, dg.gw, dg.Gw, Bw) - rw0;
      jw = jw < 0 ? 0 : (jw > DF_RW - 4 ? DF_RW - 4 : jw);                  // (lanes past Wo: they store nothing, and read inside)
    }
    for (int r = 0; r < RS_TD / 4; ++r) {
      const int dd = r * 4 + (t >> 6), d = d0 + dd;
      if (w >= Wo || d >= Do) continue;
      SrcOff src;
      bool okd = true, okh = true, okw = true;              // RESIZE: every output voxel has its source voxel
      float qd = 0.f, qh = 0.f, qw = 0.f;                   // the sampling point (not RESIZE)
      if constexpr (RESIZE) {
        src = ((int64_t)nearest_src(d, p.sD, D) * H + sh) * W + sw;
      } else {
        affine3d_point(p.m, (float)d, fh, fw, qd, qh, qw);
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
        const int nd = ag_axis(affine3d_whole(qd), Vd, D, p.sD, p.border, okd);
        const int nh = ag_axis(affine3d_whole(qh), Vh, H, p.sH, p.border, okh);
        const int nw = ag_axis(affine3d_whole(qw), Vw, W, p.sW, p.border, okw);
        src = (unsigned)((nd * H + nh) * W + nw);             // < 2^31: the entry checks D * H * W
      }
      const bool inside = okd && okh && okw;
      if (image) {
        float v;
        if constexpr (RESIZE) {
          v = (float)image[src];
        } else if constexpr (INTERP == 0) {
          v = inside ? (float)image[src] : p.cval;
        } else {
          const float bd = floorf(qd), bh = floorf(qh), bw = floorf(qw);
          const float td = qd - bd, th = qh - bh, tw = qw - bw;
          bool od[2], oh[2], ow[2];
          int id[2], ih[2], iw[2];
          for (int c = 0; c < 2; ++c) {
            id[c] = ag_axis(affine3d_corner(bd, Vd) + (float)c, Vd, D, p.sD, p.border, od[c]) * HW;
            ih[c] = ag_axis(affine3d_corner(bh, Vh) + (float)c, Vh, H, p.sH, p.border, oh[c]) * W;
            iw[c] = ag_axis(affine3d_corner(bw, Vw) + (float)c, Vw, W, p.sW, p.border, ow[c]);
          }
          float cd[2];
          for (int a = 0; a < 2; ++a) {
            float ch[2];
            for (int b = 0; b < 2; ++b) {
              const int base = id[a] + ih[b];
              const bool ok = od[a] && oh[b];
              const float x = ok && ow[0] ? (float)image[(unsigned)(base + iw[0])] : p.cval;
              const float y = ok && ow[1] ? (float)image[(unsigned)(base + iw[1])] : p.cval;
              ch[b] = affine3d_lerp(x, y, tw);
            }
            cd[a] = affine3d_lerp(ch[0], ch[1], th);
          }
          v = affine3d_lerp(cd[0], cd[1], td);
        }
        if (p.window) {
          v = fminf(fmaxf(v, p.win_lo), p.win_hi);
          if (p.window == 2) v = (v - p.win_lo) / (float)((double)p.win_hi - (double)p.win_lo + 1e-8);   // numpy float32 arithmetic of apply_window
        }
        if constexpr (!RESIZE)
          if (p.apply_gain) v = v * p.gain + p.bias;
        s_img[dd][ww] = v;
      }
      if (masks) {
        int lab = 0;
        unsigned bits = 0;
        if (inside) {
          for (int k = 0; k < K; ++k) {
            int ch = k;
            if constexpr (!RESIZE) ch = (int)((p.perm >> (4 * k)) & 15ull);   // wave-uniform: the channel's base stays scalar
            const int m = (masks + (int64_t)ch * D * HW)[src];
            bits |= (m ? 1u : 0u) << k;
            const int val = m * (k + 1);
            lab = val > lab ? val : lab;
          }
        }
        s_lab[dd][ww] = (uint8_t)lab;
        s_bits[dd][ww] = (unsigned short)bits;
        if (hist) atomicAdd(&s_h[lab & RS_KMAX], 1u);
      }
    }
  }
  __syncthreads();
  {
    const int dd = t & 31, d = d0 + dd;
    const int64_t plane = (int64_t)Ho * Wo * Do;
    for (int r = 0; r < RS_TW / 8; ++r) {
      const int ww = r * 8 + (t >> 5), w = w0 + ww;
      if (w >= Wo || d >= Do) continue;
      const Off dst = ((Off)h * Wo + w) * Do + d;       // AFFINE, LATTICE: < 2^31, the entry checks Do * Ho * Wo
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

// What the three entries ask of the arguments they share, and the kernels' geometry block and grid; `who` names the entry in
// messages.  offsets32: the kernel's per-lane offsets are 32-bit
inline int resample3d_prepare(const char* who, bool offsets32, const void* image, int32_t image_dtype, const uint8_t* masks, int32_t K,
                              int32_t D, int32_t H, int32_t W, int32_t Do, int32_t Ho, int32_t Wo, int32_t window, float win_lo,
                              float win_hi, const float* image_out, const uint8_t* masks_out, const uint8_t* labels_out,
                              const int64_t* hist, Resize3dArgs& p, dim3& grid) {
  CTSEG_REQUIRE(D > 0 && H > 0 && W > 0 && Do > 0 && Ho > 0 && Wo > 0 && (image || masks), "%s: bad geometry", who);
  CTSEG_REQUIRE(!offsets32 || ((int64_t)D * H * W < (1ll << 31) && (int64_t)Do * Ho * Wo < (1ll << 31)),
                "%s: a volume of 2^31 voxels or more", who);
  CTSEG_REQUIRE(!image || image_out, "%s: image without image_out", who);
  CTSEG_REQUIRE(!masks || (K > 0 && K <= RS_KMAX && (masks_out || labels_out)), "%s: masks need K <= 15 and an output", who);
  CTSEG_REQUIRE(!hist || labels_out, "%s: hist needs labels_out", who);
  CTSEG_REQUIRE(window >= 0 && window <= 2 && (!window || win_hi > win_lo), "%s: bad window", who);
  CTSEG_REQUIRE(is_raw_dtype(image_dtype), "%s: image dtype %d", who, image_dtype);
  p.K = masks ? K : 0, p.D = D, p.H = H, p.W = W, p.Do = Do, p.Ho = Ho, p.Wo = Wo, p.window = window;
  p.sD = (float)D / (float)Do, p.sH = (float)H / (float)Ho, p.sW = (float)W / (float)Wo;
  p.win_lo = win_lo, p.win_hi = win_hi;
  grid = dim3(((Do + RS_TD - 1) / RS_TD) * ((Wo + RS_TW - 1) / RS_TW), Ho);
  return 0;
}

// What ctseg_augment3d_to_hwd asks of its arguments beyond that, and the rest of the argument block
inline int augment3d_prepare(const char* who, const void* image, int32_t image_dtype, const uint8_t* masks, int32_t K, int32_t D,
                             int32_t H, int32_t W, int32_t Do, int32_t Ho, int32_t Wo, const float* matrix, int32_t interp,
                             int32_t border, float cval, const int32_t* mask_src, int32_t window, float win_lo, float win_hi, float gain,
                             float bias, const float* image_out, const uint8_t* masks_out, const uint8_t* labels_out,
                             const int64_t* hist, Aug3dArgs& p, dim3& grid) {
  if (int rc = resample3d_prepare(who, true, image, image_dtype, masks, K, D, H, W, Do, Ho, Wo, window, win_lo, win_hi, image_out,
                                  masks_out, labels_out, hist, p, grid))
    return rc;
  CTSEG_REQUIRE(interp == 0 || interp == 1, "%s: interp %d is neither 0 (nearest) nor 1 (trilinear)", who, interp);
  CTSEG_REQUIRE(border == 0 || border == 1, "%s: border %d is neither 0 (constant) nor 1 (edge)", who, border);
  CTSEG_REQUIRE(matrix, "%s: matrix is a null pointer", who);
  const int out[3] = {Do, Ho, Wo};
  if (int rc = affine3d_check(who, matrix, out, "output grid", p.m)) return rc;
  CTSEG_REQUIRE(std::isfinite(cval), "%s: cval is not finite", who);
  CTSEG_REQUIRE(std::isfinite(gain) && std::isfinite(bias), "%s: gain / bias is not finite", who);
  bool identity;                     // (not asked for: the tile decodes the word either way)
  if (int rc = pack_permutation(who, "mask_src", mask_src, p.K, p.perm, identity)) return rc;
  p.border = border, p.apply_gain = !(gain == 1.f && bias == 0.f);
  p.cval = cval, p.gain = gain, p.bias = bias;
  return 0;
}

// image_dtype and interp, both checked -> f(the pixel type's tag, std::integral_constant<int, interp>): one kernel per pair
template <class F> static inline void with_pixel_and_interp(int image_dtype, int interp, F&& f) {
  with_raw_dtype(image_dtype, [&](auto ti) {
    if (interp) f(ti, std::integral_constant<int, 1>{});
    else f(ti, std::integral_constant<int, 0>{});
  });
}

}  // namespace ctseg
