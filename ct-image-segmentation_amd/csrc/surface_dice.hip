// Surface Dice at tolerance (normalised surface Dice) on gfx950: per sample and class, how many voxels of the prediction's surface
// have a voxel of the truth's surface within the tolerance, and the mirror image.  One launch, no workspace, no transform: the
// search is bounded by the tolerance, so a workgroup answers it for a tile of the volume from LDS.
//   stage    both label maps of the tile with a halo of radius + 1 voxels (the extra voxel is for the surface rule), one byte per
//            voxel: the label in the low nibble (C <= 16), 0 for a label >= C and outside the volume, which both differ from every
//            class.  Rows along Z start at a multiple of 4, so with Z a multiple of 4 a lane moves a word.
//   codes    in place, a word (4 voxels along Z) per lane: the high nibble of a byte becomes the label where the voxel is on the
//            surface of its class (a neighbour along an active axis holds another low nibble), 0 elsewhere.  Lanes read the words
//            around theirs while those are being rewritten: only low nibbles are read and only high nibbles change.
//   compact  the interior voxels with a code, of both maps, into a list: surface voxels are a few percent of a tile, so lanes take
//            list entries, not raster voxels.  Their numbers per side and class are the surface sizes.
//   search   a lane looks for its voxel's code in the other map, first within one voxel and then over the whole box, every axis from
//            offset 0 outwards.  The acceptance rule is the loop bound: a partial sum past the limit ends that axis' walk (adding a
//            non-negative term and rounding never lowers a sum), so each class walks its own box inside the launch's.
// Counts leave by integer atomics (LDS, then one add per workgroup, side and class): the same bits every run.
#include <type_traits>

#include "distmap_common.h"
#include "label_runs.h"

namespace ctseg {

constexpr int NSD_MAX_RADIUS = CTSEG_SURFACE_DICE_MAX_RADIUS;
constexpr int NSD_LDS_BYTES = 60 * 1024;   // of the dynamic part: with the static tables the workgroup stays under 64 KiB
constexpr uint32_t NSD_LOW = 0x0f0f0f0fu;

// interior t, halo h (hz a multiple of 4), LDS extents n = t + 2 h (nz a multiple of 4), the launch's radii r
struct NsdTile { int tx, ty, tz, hx, hy, hz, nx, ny, nz, rx, ry, rz; };

// The acceptance rule without a spacing: dx^2 + dy^2 + dz^2 <= T2 in integers.
struct NsdVoxels {
  using T = int;
  int lim;
  __device__ __forceinline__ NsdVoxels(uint32_t bits, const float*) : lim((int)bits) {}
  __device__ __forceinline__ int term(int, int d) const { return d * d; }
  __device__ __forceinline__ int add(int a, int b) const { return a + b; }
};
// With squared voxel sizes w: fl(fl(w1 d1^2) + fl(fl(w2 d2^2) + fl(w0 d0^2))) <= t2, the expression of ctseg_distmap3d_weighted.
struct NsdSpacing {
  using T = float;
  float lim, w[3];
  __device__ __forceinline__ NsdSpacing(uint32_t bits, const float* sw) : lim(__uint_as_float(bits)), w{sw[0], sw[1], sw[2]} {}
  __device__ __forceinline__ float term(int a, int d) const { return mul_rn(w[a], (float)(d * d)); }   // d^2 <= 64: exact
  __device__ __forceinline__ float add(float a, float b) const { return add_rn(a, b); }
};

template <class R> struct NsdTag { using type = R; };

// offsets of an axis in the order 0, -1, 1, -2, 2, ...: |d| never decreases
__device__ __forceinline__ int nsd_zigzag(int j) { return (j & 1) ? -((j + 1) >> 1) : (j >> 1); }

// Is code c at an accepted offset from byte p of `other`, inside the box (r0, r1, r2)?  sx, sy: bytes per X and Y step.
template <class RULE>
__device__ __forceinline__ bool nsd_walk(const RULE& rule, const uint8_t* other, int p, int sx, int sy, uint32_t c, int r0, int r1, int r2) {
  for (int j0 = 0; j0 <= 2 * r0; ++j0) {
    const int d0 = nsd_zigzag(j0);
    const typename RULE::T a = rule.term(0, d0);
    if (a > rule.lim) break;
    for (int j2 = 0; j2 <= 2 * r2; ++j2) {
      const int d2 = nsd_zigzag(j2);
      const typename RULE::T b = rule.add(rule.term(2, d2), a);
      if (b > rule.lim) break;
      for (int j1 = 0; j1 <= 2 * r1; ++j1) {
        const int d1 = nsd_zigzag(j1);
        if (rule.add(rule.term(1, d1), b) > rule.lim) break;
        if ((uint32_t)(other[p + d0 * sx + d1 * sy + d2] >> 4) == c) return true;
      }
    }
  }
  return false;
}

// Grid (tiles of a sample, B).  WORDS: Z is a multiple of 4 and both maps are 4-byte aligned.
template <class RULE, bool WORDS>
__global__ __launch_bounds__(256) void surface_dice_kernel(const uint8_t* __restrict__ pred, const uint8_t* __restrict__ target, int B,
                                                           int X, int Y, int Z, int C, int axes, NsdTile g, int tyn, int tzn,
                                                           const uint32_t* __restrict__ limit, const float* __restrict__ w2,
                                                           int32_t* __restrict__ counts, int32_t* __restrict__ within) {
  extern __shared__ __attribute__((aligned(16))) uint8_t nsd_lds[];
  __shared__ uint32_t s_cnt[2][SD_MAX_CLASSES], s_in[2][SD_MAX_CLASSES], s_lim[SD_MAX_CLASSES], s_n;
  __shared__ float s_w[3];
  const int tid = threadIdx.x, b = blockIdx.y, K = C - 1;
  int r = blockIdx.x;
  const int z0 = (r % tzn) * g.tz; r /= tzn;
  const int y0 = (r % tyn) * g.ty, x0 = (r / tyn) * g.tx;
  const int nzw = g.nz >> 2, vol_w = g.nx * g.ny * nzw;             // words of a row and of a map
  uint32_t* words = reinterpret_cast<uint32_t*>(nsd_lds);           // [2][nx][ny][nzw]
  uint16_t* list = reinterpret_cast<uint16_t*>(nsd_lds + 8 * (size_t)vol_w);
  if (tid < 2 * SD_MAX_CLASSES) { s_cnt[tid >> 4][tid & 15] = 0u; s_in[tid >> 4][tid & 15] = 0u; }
  if (tid >= 1 && tid < C) s_lim[tid] = limit[b * K + tid - 1];
  if (tid < 3) s_w[tid] = w2 ? w2[b * 3 + tid] : 1.f;
  if (tid == 0) s_n = 0u;

  // ---- stage
  const int64_t S = (int64_t)X * Y * Z;
  for (int w = tid; w < 2 * vol_w; w += 256) {
    const int side = w >= vol_w, ww = w - side * vol_w;
    const int row = ww / nzw, kw = ww - row * nzw;
    const int i = row / g.ny, j = row - i * g.ny;
    const int x = x0 - g.hx + i, y = y0 - g.hy + j, z = z0 - g.hz + 4 * kw;
    uint32_t v = 0u;
    if (x >= 0 && x < X && y >= 0 && y < Y && z > -4 && z < Z) {
      const uint8_t* src = (side ? target : pred) + (int64_t)b * S + ((int64_t)x * Y + y) * Z;
      if constexpr (WORDS) {
        if (z >= 0) v = *reinterpret_cast<const uint32_t*>(src + z);
      } else {
#pragma unroll
        for (int t = 0; t < 4; ++t)
          if (z + t >= 0 && z + t < Z) v |= (uint32_t)src[z + t] << (8 * t);
      }
    }
    uint32_t m = 0u;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const uint32_t l = (v >> (8 * t)) & 255u;
      if (l < (uint32_t)C) m |= l << (8 * t);
    }
    words[w] = m;
  }
  __syncthreads();

  // ---- codes (the outermost layer along an active axis has no neighbours staged and is never looked at)
  const int step_x = g.ny * nzw, step_y = nzw;
  for (int w = tid; w < 2 * vol_w; w += 256) {
    const int side = w >= vol_w, ww = w - side * vol_w;
    const int row = ww / nzw, kw = ww - row * nzw;
    const int i = row / g.ny, j = row - i * g.ny;
    if ((axes & SD_AXIS_X) && (i == 0 || i == g.nx - 1)) continue;
    if ((axes & SD_AXIS_Y) && (j == 0 || j == g.ny - 1)) continue;
    const uint32_t own = words[w] & NSD_LOW;
    if (own == 0u) continue;
    uint32_t d = 0u;
    if (axes & SD_AXIS_X) d |= (own ^ words[w - step_x]) | (own ^ words[w + step_x]);
    if (axes & SD_AXIS_Y) d |= (own ^ words[w - step_y]) | (own ^ words[w + step_y]);
    if (axes & SD_AXIS_Z) {
      const uint32_t prev = kw > 0 ? words[w - 1] : 0u, next = kw < nzw - 1 ? words[w + 1] : 0u;
      d |= (own ^ ((own << 8) | ((prev >> 24) & 15u))) | (own ^ ((own >> 8) | ((next & 15u) << 24)));
    }
    d &= NSD_LOW;
    const uint32_t differs = ((d | (d >> 1) | (d >> 2) | (d >> 3)) & 0x01010101u) * 15u;   // 0x0f in the bytes with a differing neighbour
    words[w] = own | ((own & differs) << 4);
  }
  __syncthreads();

  // ---- compact
  const int tzw = g.tz >> 2, tile_w = g.tx * g.ty * tzw;
  for (int q = tid; q < 2 * tile_w; q += 256) {
    const int side = q >= tile_w, qq = q - side * tile_w;
    const int line = qq / tzw, kw = qq - line * tzw;
    const int ix = line / g.ty, iy = line - ix * g.ty;
    const uint32_t code = (words[side * vol_w + ((ix + g.hx) * g.ny + iy + g.hy) * nzw + (g.hz >> 2) + kw] >> 4) & NSD_LOW;
    if (code == 0u) continue;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const uint32_t c = (code >> (8 * t)) & 15u;
      if (c) {
        list[atomicAdd(&s_n, 1u)] = (uint16_t)((side << 15) | (line * g.tz + 4 * kw + t));
        atomicAdd(&s_cnt[side][c], 1u);
      }
    }
  }
  __syncthreads();

  // ---- search
  const int n = (int)s_n, sy = g.nz, sx = g.ny * g.nz, vol = 4 * vol_w;
  for (int e = tid; e < n; e += 256) {
    const int side = list[e] >> 15, at = list[e] & 0x7fff;
    const int line = at / g.tz, iz = at - line * g.tz;
    const int ix = line / g.ty, iy = line - ix * g.ty;
    const int p = (ix + g.hx) * sx + (iy + g.hy) * sy + g.hz + iz;
    const uint32_t c = nsd_lds[side * vol + p] >> 4;
    const uint8_t* other = nsd_lds + (1 - side) * vol;
    const RULE rule(s_lim[c], s_w);
    const int nx1 = g.rx < 1 ? g.rx : 1, ny1 = g.ry < 1 ? g.ry : 1, nz1 = g.rz < 1 ? g.rz : 1;
    if (nsd_walk(rule, other, p, sx, sy, c, nx1, ny1, nz1) || nsd_walk(rule, other, p, sx, sy, c, g.rx, g.ry, g.rz))
      atomicAdd(&s_in[side][c], 1u);
  }
  __syncthreads();
  if (tid < 2 * SD_MAX_CLASSES) {
    const int side = tid >> 4, c = tid & 15;
    if (c >= 1 && c < C) {
      const int64_t at = (int64_t)(side * B + b) * K + c - 1;
      if (s_cnt[side][c]) atomicAdd(&counts[at], (int32_t)s_cnt[side][c]);
      if (s_in[side][c]) atomicAdd(&within[at], (int32_t)s_in[side][c]);
    }
  }
}

// dynamic LDS of a tile: both staged maps and the list of its interior surface voxels (two bytes each, both sides)
static inline int64_t nsd_tile_bytes(const NsdTile& g) { return 2 * (int64_t)g.nx * g.ny * g.nz + 4 * (int64_t)g.tx * g.ty * g.tz; }

// The largest tile whose staging fits: the halo is the launch's radius per axis, plus the neighbour of the surface rule along an
// active axis, and along Z rounded up to whole words.
static NsdTile nsd_tile(int X, int Y, int Z, int axes, const int rmax[3]) {
  static const int cand[][3] = {{8, 8, 64}, {8, 8, 32}, {4, 8, 32}, {4, 4, 32}, {4, 4, 16}};
  NsdTile g = {};
  g.rx = rmax[0]; g.ry = rmax[1]; g.rz = rmax[2];
  g.hx = rmax[0] + ((axes & SD_AXIS_X) ? 1 : 0);
  g.hy = rmax[1] + ((axes & SD_AXIS_Y) ? 1 : 0);
  g.hz = (rmax[2] + ((axes & SD_AXIS_Z) ? 1 : 0) + 3) / 4 * 4;
  for (const auto& t : cand) {
    g.tx = X < t[0] ? X : t[0];
    g.ty = Y < t[1] ? Y : t[1];
    g.tz = (Z + 3) / 4 * 4 < t[2] ? (Z + 3) / 4 * 4 : t[2];
    g.nx = g.tx + 2 * g.hx; g.ny = g.ty + 2 * g.hy; g.nz = g.tz + 2 * g.hz;
    if (nsd_tile_bytes(g) <= NSD_LDS_BYTES) break;
  }
  return g;
}

}  // namespace ctseg

using namespace ctseg;

extern "C" int ctseg_surface_dice(const uint8_t* pred, const uint8_t* target, int32_t B, int32_t X, int32_t Y, int32_t Z, int32_t C,
                                  int32_t axes, const int32_t* radius, const void* limit, const float* w2, int32_t* counts,
                                  int32_t* within, void* stream) {
  CTSEG_REQUIRE(pred && target && radius && limit && counts && within,
                "surface_dice: null pointer (pred, target, radius, limit, counts and within are required)");
  if (check_sides("surface_dice", B, X, Y, Z)) return -1;
  CTSEG_REQUIRE(C >= 2 && C <= SD_MAX_CLASSES, "surface_dice: 2 <= C <= %d classes (got %d)", SD_MAX_CLASSES, C);
  CTSEG_REQUIRE(B <= 65535, "surface_dice: %d samples are too many for one launch", B);
  CTSEG_REQUIRE(axes >= 1 && axes <= 7, "surface_dice: axes is a mask of X = 1, Y = 2, Z = 4 (got %d)", axes);
  CTSEG_REQUIRE(((uintptr_t)limit % 4) == 0 && ((uintptr_t)w2 % 4) == 0 && ((uintptr_t)counts % 4) == 0 &&
                    ((uintptr_t)within % 4) == 0 && ((uintptr_t)radius % 4) == 0,
                "surface_dice: unaligned pointer (radius, limit, w2, counts, within)");
  int rmax[3] = {0, 0, 0};
  for (int64_t i = 0; i < (int64_t)B * (C - 1) * 3; ++i) {
    CTSEG_REQUIRE(radius[i] >= 0 && radius[i] <= NSD_MAX_RADIUS, "surface_dice: radius %d of sample %d, class %d, axis %d is not in 0..%d",
                  radius[i], (int)(i / (3 * (C - 1))), (int)(i / 3 % (C - 1)) + 1, (int)(i % 3), NSD_MAX_RADIUS);
    rmax[i % 3] = radius[i] > rmax[i % 3] ? radius[i] : rmax[i % 3];
  }
  const NsdTile g = nsd_tile(X, Y, Z, axes, rmax);
  CTSEG_REQUIRE(nsd_tile_bytes(g) <= NSD_LDS_BYTES, "surface_dice: no tile fits the LDS (radii %d, %d, %d)", rmax[0], rmax[1], rmax[2]);
  const int txn = (X + g.tx - 1) / g.tx, tyn = (Y + g.ty - 1) / g.ty, tzn = (Z + g.tz - 1) / g.tz;
  const dim3 grid((unsigned)(txn * tyn * tzn), (unsigned)B);
  const bool words = Z % 4 == 0 && ((uintptr_t)pred % 4) == 0 && ((uintptr_t)target % 4) == 0;
  hipStream_t st = (hipStream_t)stream;
  const auto launch = [&](auto rule, auto words_t) {
    using RULE = typename decltype(rule)::type;
    hipLaunchKernelGGL((surface_dice_kernel<RULE, decltype(words_t)::value>), grid, dim3(256), (size_t)nsd_tile_bytes(g), st, pred, target, B,
                       X, Y, Z, C, axes, g, tyn, tzn, (const uint32_t*)limit, w2, counts, within);
  };
  const auto by_words = [&](auto rule) { words ? launch(rule, std::true_type{}) : launch(rule, std::false_type{}); };
  if (w2) by_words(NsdTag<NsdSpacing>{});
  else by_words(NsdTag<NsdVoxels>{});
  CTSEG_LAUNCH_CHECK("surface_dice");
  return 0;
}
