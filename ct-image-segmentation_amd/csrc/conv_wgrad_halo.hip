// LDS-halo weight-gradient kernel (bf16) for 3x3x3 stride-1 layers with few channels (gfx950).
//
//   R[tap*Cg + a][b] = sum_voxels x[voxel + d(tap)][a] * dy[voxel][b],   R[27*Cg][b] = sum_voxels dy[voxel][b]
//
// The generic split-K kernel re-gathers x once per 128 K-rows (27x through L2 for a 3x3x3 layer).  Here a persistent
// workgroup stages the 6x10x10 halo of x and the 4x8x8 tile of dy ONCE per tile (double-buffered), and the four waves
// split the 27 taps (+ one all-ones pseudo tap = bias gradient): wave w owns taps w, w+4, ... and keeps their
// [Cg x Cn] fp32 accumulators in registers across ALL of the workgroup's tiles; dy fragments are read once per
// 32-voxel k-step and reused for the wave's 7 taps.  Both MFMA operands contract over voxels, the slow axis of the
// channels-last tensors: ds_read_b64_tr_b16 transposes 4 voxels x 16 channels per 16-lane group; the LDS images are
// planes of 16 channels (32 B per voxel) and a k-step is 4 z-rows of 8 voxels, so each 32-lane half reads 8
// contiguous 32-byte rows (256 B): bank-conflict free.  One fp32 slab per workgroup -> ctseg_conv_wgrad_reduce.
#include "conv_common.h"
#include "wgrad_common.h"

#ifndef WH_ABL
#define WH_ABL 0     // timing-only ablation of the two head kernels (tools/ablate_wgrad_head*.sh; results are garbage): 1 = no MFMAs, 2 = no LDS operand reads, 4 = no global loads, 8 = no LDS staging stores
#endif

namespace ctseg {

struct WgradHaloArgs {
  const char* in;
  const char* dy;
  float* ws;
  int N, X, Y, Z, Cg, g_ld, d_ld;
  int kpad_w, cn_pad;
  int tiles, txn, tyn, tzn;   // tiles per sample and per axis
  int delta[28];              // halo voxel delta of each tap (in 32-byte rows), entry 27 unused
  // InstanceNorm + PReLU of the gathered operand on load (ctseg_wgrad_desc::in_mean_rstd): conv_wgrad_head2_kernel only
  const float* in_mr;
  const float* in_alpha;
  int in_C;
};

constexpr int WH_NRM_MAXN = 16;

constexpr int WH_HV = 600, WH_TV = 256;

// NW waves split the 27 taps (+ the all-ones pseudo tap): 4 waves x 7 taps, or 8 waves x 3-4 taps.  With 64-byte operands the 7-tap
// accumulators (112 registers) left one wave per SIMD (302 registers): 8 waves with <= 4 taps each fit two per SIMD.
template <int VB, int DBY, int NW>
__global__ __launch_bounds__(64 * NW) void conv_wgrad_halo_kernel(const WgradHaloArgs P, int total_tiles) {
  constexpr int NTH = 64 * NW, TPW = (28 + NW - 1) / NW, TFULL = 27 / NW;    // taps per wave; taps every wave owns (the last may not exist)
  constexpr int PA = VB / 32, PB = DBY / 32;
  // plane pitches padded by 64 B: with two planes the 8 lanes of a 16-byte staging store hold 2 voxels x 2 planes, and pitches
  // that are multiples of the 256-byte bank period (19 200 / 8 192 B) put both planes of a voxel on the same banks
  constexpr int XPL = WH_HV * 32 + (PA > 1 ? 64 : 0), DPL = WH_TV * 32 + (PB > 1 ? 64 : 0);
  constexpr int XBYTES = PA * XPL, DBYTES = PB * DPL, BUF = XBYTES + DBYTES;
  constexpr int XCH = WH_HV * (VB / 16), DCH = WH_TV * (DBY / 16);
  constexpr int JX = (XCH + NTH - 1) / NTH, JD = (DCH + NTH - 1) / NTH;

  // ONE staging buffer: the next tile's operands wait in registers (gload) while this tile is consumed and are written after
  // the barrier that ends it.  Half the LDS of a double buffer -> twice the workgroups per CU, whose phases interleave.
  __shared__ __attribute__((aligned(16))) char smem[BUF];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform: tap selection stays on the scalar unit
  const int r16 = lane & 15, q4 = lane >> 4;
  const int tq = r16 >> 2, tp = r16 & 3;

  // per-thread constants of the staging slots (only a scalar tile base changes from tile to tile)
  const int YZ = P.Y * P.Z;
  int gx_byte[JX], gx_hxyz[JX], gx_lds[JX], gd_byte[JD], gd_xyz[JD], gd_lds[JD];
#pragma unroll
  for (int j = 0; j < JX; ++j) {
    const int idx = tid + j * NTH;
    const int c = idx % (VB / 16), hv = idx / (VB / 16);
    const int hx = hv / 100, rem = hv - hx * 100, hy = rem / 10, hz = rem - hy * 10;
    gx_byte[j] = (((hx - 1) * YZ + (hy - 1) * P.Z + (hz - 1)) * P.g_ld + c * 8) * 2;
    gx_hxyz[j] = (idx < XCH) ? (hx | (hy << 8) | (hz << 16)) : 0x7f7f7f;
    gx_lds[j] = (c >> 1) * XPL + hv * 32 + (c & 1) * 16;
  }
#pragma unroll
  for (int j = 0; j < JD; ++j) {
    const int idx = tid + j * NTH;
    const int c = idx % (DBY / 16), tv = idx / (DBY / 16);
    const int tx = tv >> 6, ty = (tv >> 3) & 7, tz = tv & 7;
    gd_byte[j] = ((tx * YZ + ty * P.Z + tz) * P.d_ld + c * 8) * 2;
    gd_xyz[j] = (idx < DCH) ? (tx | (ty << 8) | (tz << 16)) : 0x7f7f7f;
    gd_lds[j] = (c >> 1) * DPL + tv * 32 + (c & 1) * 16;
  }
  u32x4 rx[JX], rd[JD];
  // 12-wide bf16 rows (24 bytes): chunk 1 is channels 8..11 + zero fill (32-byte planes only)
  const bool x12 = VB == 32 && (P.g_ld & 7) != 0, d12 = DBY == 32 && (P.d_ld & 7) != 0;
  auto load_row_chunk = [](const char* p, bool w12, bool second) -> u32x4 {
    if (!w12) return *reinterpret_cast<const u32x4*>(p);
    return load_row12_chunk(p, second);
  };
  auto gload = [&](int t) {
    const auto [n, x0, y0, z0] = tile_origin<4, 8, 8>(t, P.tiles, P.tyn, P.tzn);
    const int64_t vb = (((int64_t)n * P.X + x0) * P.Y + y0) * P.Z + z0;
    const char* xb = P.in + vb * P.g_ld * 2;
    const char* db = P.dy + vb * P.d_ld * 2;
#pragma unroll
    for (int j = 0; j < JX; ++j) {
      const int xi = x0 - 1 + (gx_hxyz[j] & 0xff), yi = y0 - 1 + ((gx_hxyz[j] >> 8) & 0xff), zi = z0 - 1 + (gx_hxyz[j] >> 16);
      u32x4 v = {0u, 0u, 0u, 0u};
      if ((unsigned)xi < (unsigned)P.X && (unsigned)yi < (unsigned)P.Y && (unsigned)zi < (unsigned)P.Z)
        v = load_row_chunk(xb + gx_byte[j], x12, (gx_lds[j] & 16) != 0);
      rx[j] = v;
    }
#pragma unroll
    for (int j = 0; j < JD; ++j) {
      const int xi = x0 + (gd_xyz[j] & 0xff), yi = y0 + ((gd_xyz[j] >> 8) & 0xff), zi = z0 + (gd_xyz[j] >> 16);
      u32x4 v = {0u, 0u, 0u, 0u};
      if (xi < P.X && yi < P.Y && zi < P.Z) v = load_row_chunk(db + gd_byte[j], d12, (gd_lds[j] & 16) != 0);
      rd[j] = v;
    }
  };
  auto sstore = [&](int) {
    char* xs = smem;
    char* ds = xs + XBYTES;
#pragma unroll
    for (int j = 0; j < JX; ++j)
      if (JX * NTH == XCH || tid + j * NTH < XCH) *reinterpret_cast<u32x4*>(xs + gx_lds[j]) = rx[j];
#pragma unroll
    for (int j = 0; j < JD; ++j)
      if (JD * NTH == DCH || tid + j * NTH < DCH) *reinterpret_cast<u32x4*>(ds + gd_lds[j]) = rd[j];
  };

  f32x4 acc[TPW][PA][PB];
#pragma unroll
  for (int t = 0; t < TPW; ++t)
#pragma unroll
    for (int a = 0; a < PA; ++a)
#pragma unroll
      for (int b = 0; b < PB; ++b) acc[t][a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

  // this lane's voxel inside a k-step for the two transposed reads: y-row 2r + (q4>>1), z = 4*(q4&1) + tq
  const int lz = 4 * (q4 & 1) + tq, ly = q4 >> 1;
  const bf16x8 ones = bias_ones_frag(r16);

  const auto [first, tstride, tlast] = xcd_tile_seq([] { return blockIdx.x; }, gridDim.x, total_tiles);
  int t = first;
  if (t < tlast) {
    gload(t);
    sstore(0);
  }
  __syncthreads();
  for (; t < tlast; t += tstride) {
    const int tn = t + tstride;
    if (tn < tlast) gload(tn);
    const char* xs = smem;
    const char* ds = xs + XBYTES;
#pragma unroll 2
    for (int s = 0; s < 8; ++s) {
      const int x = s >> 1, yb = 4 * (s & 1);
      // dy fragments of this k-step (shared by the wave's 7 taps)
      bf16x8 df[PB];
#pragma unroll
      for (int b = 0; b < PB; ++b)
        df[b] = tr16_frag(ds + b * DPL + (((x * 8) + (yb + ly)) * 8 + lz) * 32 + tp * 8, 2 * 8 * 32);
      const int hbase = (((x + 1) * 10) + (yb + ly + 1)) * 10 + (lz + 1);
      // taps wave, wave+4, ..., wave+20 always exist: fetch all their operands first, then issue the MFMAs back to back
      // (branch-free, so the LDS latency of one tap hides behind the others); tap wave+24 may be the pseudo tap 27
      bf16x8 af[TFULL][PA];
#pragma unroll
      for (int ti = 0; ti < TFULL; ++ti) {
        const int h = hbase + P.delta[wave + NW * ti];
#pragma unroll
        for (int a = 0; a < PA; ++a) af[ti][a] = tr16_frag(xs + a * XPL + h * 32 + tp * 8, 2 * 10 * 32);
      }
#pragma unroll
      for (int ti = 0; ti < TFULL; ++ti)
#pragma unroll
        for (int a = 0; a < PA; ++a)
#pragma unroll
          for (int b = 0; b < PB; ++b)
            acc[ti][a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[ti][a], df[b], acc[ti][a][b], 0, 0, 0);
      if constexpr (TPW > TFULL) {
        const int tap = wave + NW * TFULL;      // wave-uniform: a real tap, the pseudo tap 27, or nothing
        if (tap < 27) {
          const int h = hbase + P.delta[tap];
#pragma unroll
          for (int a = 0; a < PA; ++a) {
            const bf16x8 a6 = tr16_frag(xs + a * XPL + h * 32 + tp * 8, 2 * 10 * 32);
#pragma unroll
            for (int b = 0; b < PB; ++b) acc[TFULL][a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a6, df[b], acc[TFULL][a][b], 0, 0, 0);
          }
        } else if (tap == 27) {  // pseudo tap 27: x == 1 on channel row 0 -> row 0 of the tile accumulates sum(dy) (bias gradient)
#pragma unroll
          for (int b = 0; b < PB; ++b)
            acc[TFULL][0][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, df[b], acc[TFULL][0][b], 0, 0, 0);
        }
      }
    }
    __syncthreads();
    if (tn < tlast) sstore(0);
    __syncthreads();
  }

  // ---- one slab per workgroup: lane holds column c16 = dy channel, rows 4*q4 + e = x channel ------------------------
  float* slab = P.ws + (int64_t)blockIdx.x * P.kpad_w * P.cn_pad;
#pragma unroll
  for (int ti = 0; ti < TPW; ++ti) {
    const int tap = wave + NW * ti;
    if (tap > 27) continue;
#pragma unroll
    for (int a = 0; a < PA; ++a) {
      if (tap == 27 && a > 0) continue;
#pragma unroll
      for (int b = 0; b < PB; ++b)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int row = tap * P.Cg + a * 16 + 4 * q4 + e;
          if (row < P.kpad_w) slab[(int64_t)row * P.cn_pad + b * 16 + r16] = acc[ti][a][b][e];
        }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The 16 -> <= 16 channel layer at full resolution (the logits convolution of the head: 25 M voxels, 1.2 GB of operands, 348 GFLOP of
// padded MFMA work) is HBM-latency bound in the kernel above.  The two head kernels below share one staging scheme (HeadStage): rows
// move in 8-byte pieces with raw buffer loads — 12-wide (24-byte) and 16-wide rows alike, a voxel outside the volume is an
// out-of-range offset selected by one v_and / v_cmp / v_cndmask — with no per-load branches, ONE register set of loads in flight per
// workgroup and 128 registers per lane: the phases of a workgroup (loads -> multiplies -> barrier -> LDS stores -> barrier) do not
// overlap inside it; they overlap with those of the other workgroups on its CU.
__device__ __forceinline__ bf16x8 wh_frag(const char* p0, int hi_off) {
  if constexpr ((WH_ABL & 2) != 0) {      // (timing only)
    typedef __attribute__((ext_vector_type(8))) short s16x8;
    const short v0 = (short)(uintptr_t)p0;
    return __builtin_bit_cast(bf16x8, s16x8{v0, v0, v0, v0, v0, v0, v0, v0});
  }
  return tr16_frag(p0, hi_off);
}

template <int NPX, int NPD, int NTH>      // 8-byte pieces per x / dy voxel row: 3 (12 wide) or 4 (16 wide); threads
struct HeadStage {
  static constexpr int XBYTES = WH_HV * 32, DBYTES = WH_TV * 32, BUF = XBYTES + DBYTES;
  static constexpr int XN = WH_HV * NPX, DN = WH_TV * NPD, JX = (XN + NTH - 1) / NTH, JD = (DN + NTH - 1) / NTH;
  // per-thread constants of the staging slots: byte offset from the halo / tile origin, one-hot (x, y, z) position inside the halo /
  // tile (bit 31: no such piece), byte offset in LDS.  Piece j of a thread holds channel quad (tid + j * NTH) % NPX.
  int xo[JX], xl[JX], dof[JD], dl[JD];
  uint32_t xh[JX], dh[JD];
  int bias_bytes;                           // the halo origin lies one voxel per axis before the tile's
  __device__ __forceinline__ HeadStage(const WgradHaloArgs& P, int tid) {
    const int YZ = P.Y * P.Z;
#pragma unroll
    for (int j = 0; j < JX; ++j) {
      const int idx = tid + j * NTH, hv = idx / NPX, part = idx - hv * NPX;
      const int hx = hv / 100, rem = hv - hx * 100, hy = rem / 10, hz = rem - hy * 10;
      xo[j] = (hx * YZ + hy * P.Z + hz) * P.g_ld * 2 + part * 8;
      xh[j] = idx < XN ? ((1u << hx) | (1u << (6 + hy)) | (1u << (16 + hz))) : 0x80000000u;
      xl[j] = hv * 32 + part * 8;
    }
#pragma unroll
    for (int j = 0; j < JD; ++j) {
      const int idx = tid + j * NTH, tv = idx / NPD, part = idx - tv * NPD;
      const int tx = tv >> 6, ty = (tv >> 3) & 7, tz = tv & 7;
      dof[j] = (tx * YZ + ty * P.Z + tz) * P.d_ld * 2 + part * 8;
      dh[j] = idx < DN ? ((1u << tx) | (1u << (4 + ty)) | (1u << (12 + tz))) : 0x80000000u;
      dl[j] = XBYTES + tv * 32 + part * 8;
    }
    bias_bytes = (YZ + P.Z + 1) * P.g_ld * 2;
  }
  static __device__ __forceinline__ uint32_t range_mask(int lo, int hi, int nbits) {      // bits lo .. hi, clamped to [0, nbits)
    lo = lo < 0 ? 0 : lo;
    hi = hi > nbits - 1 ? nbits - 1 : hi;
    return hi < lo ? 0u : ((2u << hi) - (1u << lo));
  }
  // one-hot positions (as in xh / dh) of the tile at `o` that lie OUTSIDE the volume
  static __device__ __forceinline__ uint32_t x_outside(const WgradHaloArgs& P, const TileOrigin& o) {
    return ~(range_mask(1 - o.x0, P.X - o.x0, 6) | (range_mask(1 - o.y0, P.Y - o.y0, 10) << 6) | (range_mask(1 - o.z0, P.Z - o.z0, 10) << 16));
  }
  static __device__ __forceinline__ uint32_t d_outside(const WgradHaloArgs& P, const TileOrigin& o) {
    return ~(range_mask(0, P.X - o.x0 - 1, 4) | (range_mask(0, P.Y - o.y0 - 1, 8) << 4) | (range_mask(0, P.Z - o.z0 - 1, 8) << 12));
  }
  __device__ __forceinline__ void gload(const WgradHaloArgs& P, int t, int x_sample_bytes, int d_sample_bytes, u32x2 (&rx)[JX], u32x2 (&rd)[JD]) const {
    const TileOrigin o = tile_origin<4, 8, 8>(t, P.tiles, P.tyn, P.tzn);
    const uint32_t xm = x_outside(P, o), dm = d_outside(P, o);
    const __amdgpu_buffer_rsrc_t xr = buffer_rsrc(P.in + (int64_t)o.n * x_sample_bytes - bias_bytes, x_sample_bytes + bias_bytes);
    const __amdgpu_buffer_rsrc_t dr = buffer_rsrc(P.dy + (int64_t)o.n * d_sample_bytes, d_sample_bytes);
    const int xs = ((o.x0 * P.Y + o.y0) * P.Z + o.z0) * P.g_ld * 2, dsf = ((o.x0 * P.Y + o.y0) * P.Z + o.z0) * P.d_ld * 2;
#pragma unroll
    for (int j = 0; j < JX; ++j)
      rx[j] = (WH_ABL & 4) ? u32x2{(uint32_t)xs, 0u} : __builtin_amdgcn_raw_buffer_load_b64(xr, (xh[j] & xm) == 0u ? xo[j] : (int)0x80000000, xs, 0);
#pragma unroll
    for (int j = 0; j < JD; ++j)
      rd[j] = (WH_ABL & 4) ? u32x2{(uint32_t)dsf, 0u} : __builtin_amdgcn_raw_buffer_load_b64(dr, (dh[j] & dm) == 0u ? dof[j] : (int)0x80000000, dsf, 0);
  }
  // rows narrower than 32 bytes: the pad bytes of every slot are zero for the whole launch
  static __device__ __forceinline__ void zero_pads(char* smem, int tid) {
    if (NPX < 4) for (int i = tid; i < WH_HV; i += NTH) *reinterpret_cast<u32x2*>(smem + i * 32 + 24) = u32x2{0u, 0u};
    if (NPD < 4) for (int i = tid; i < WH_TV; i += NTH) *reinterpret_cast<u32x2*>(smem + XBYTES + i * 32 + 24) = u32x2{0u, 0u};
  }
  // (WH_ABL & 8, timing only: a store that never happens but keeps its operands alive)
  __device__ __forceinline__ void store_x(char* smem, int tid, const u32x2 (&rx)[JX]) const {
#pragma unroll
    for (int j = 0; j < JX; ++j)
      if ((JX * NTH == XN || tid + j * NTH < XN) && (!(WH_ABL & 8) || rx[j][0] == 0x12345u)) *reinterpret_cast<u32x2*>(smem + xl[j]) = rx[j];
  }
  __device__ __forceinline__ void store_d(char* smem, int tid, const u32x2 (&rd)[JD]) const {
#pragma unroll
    for (int j = 0; j < JD; ++j)
      if ((JD * NTH == DN || tid + j * NTH < DN) && (!(WH_ABL & 8) || rd[j][0] == 0x54321u)) *reinterpret_cast<u32x2*>(smem + dl[j]) = rd[j];
  }
};

// The tile loop of both head kernels: the loads of the next tile wait in registers while this one multiplies and are written to the
// single LDS buffer behind the barrier that ends it.  The callables come by reference: copies of the closures changed the head kernel's
// register allocation (24 -> 44 bytes of scratch per lane).
template <class Load, class Compute, class Store>
__device__ __forceinline__ void head_tile_loop(const TileSeq seq, const Load& load, const Compute& compute, const Store& store) {
  int t = seq.first;
  const int tstride = seq.stride, tlast = seq.last;
  if (t < tlast) {
    load(t);
    store(t);
  }
  __syncthreads();
  for (; t < tlast; t += tstride) {
    if (t + tstride < tlast) load(t + tstride);
    compute();
    __syncthreads();
    if (t + tstride < tlast) store(t + tstride);
    __syncthreads();
  }
}

// Four waves split the 27 taps + the pseudo tap as conv_wgrad_halo_kernel<32, 32, 4> does (its multiplies); FOUR workgroups per CU.
// Serves taps in any order.
template <int NPX, int NPD>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) void conv_wgrad_head_kernel(const WgradHaloArgs P, int total_tiles, int x_sample_bytes, int d_sample_bytes) {
  using ST = HeadStage<NPX, NPD, 256>;
  __shared__ __attribute__((aligned(16))) char smem[ST::BUF];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r16 = lane & 15, q4 = lane >> 4;
  const int tq = r16 >> 2, tp = r16 & 3;
  const ST stg(P, tid);

  f32x4 acc[7];
#pragma unroll
  for (int t = 0; t < 7; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int lz = 4 * (q4 & 1) + tq, ly = q4 >> 1;
  const bf16x8 ones = bias_ones_frag(r16);
  auto compute = [&]() {
    const char* xs = smem;
    const char* ds = xs + ST::XBYTES;
#pragma unroll 2
    for (int s = 0; s < 8; ++s) {
      const int x = s >> 1, yb = 4 * (s & 1);
      const bf16x8 df = wh_frag(ds + (((x * 8) + (yb + ly)) * 8 + lz) * 32 + tp * 8, 2 * 8 * 32);
      const int hbase = (((x + 1) * 10) + (yb + ly + 1)) * 10 + (lz + 1);
      bf16x8 af[6];
#pragma unroll
      for (int ti = 0; ti < 6; ++ti) af[ti] = wh_frag(xs + (hbase + P.delta[wave + 4 * ti]) * 32 + tp * 8, 2 * 10 * 32);
#pragma unroll
      for (int ti = 0; ti < 6; ++ti) {
        if constexpr ((WH_ABL & 1) != 0) acc[ti][0] += __builtin_bit_cast(f32x4, af[ti])[0] * __builtin_bit_cast(f32x4, df)[1];
        else acc[ti] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[ti], df, acc[ti], 0, 0, 0);
      }
      const int tap = wave + 24;
      if (tap < 27) {
        acc[6] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh_frag(xs + (hbase + P.delta[tap]) * 32 + tp * 8, 2 * 10 * 32), df, acc[6], 0, 0, 0);
      } else {   // pseudo tap 27: row 0 accumulates sum(dy) (bias gradient)
        acc[6] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, df, acc[6], 0, 0, 0);
      }
    }
  };

  const TileSeq seq = xcd_tile_seq([] { return blockIdx.x; }, gridDim.x, total_tiles);
  ST::zero_pads(smem, tid);
  u32x2 rx[ST::JX], rd[ST::JD];
  head_tile_loop(
      seq, [&](int t) { stg.gload(P, t, x_sample_bytes, d_sample_bytes, rx, rd); }, compute,
      [&](int) {
        stg.store_x(smem, tid, rx);
        stg.store_d(smem, tid, rd);
      });

  float* slab = P.ws + (int64_t)blockIdx.x * P.kpad_w * P.cn_pad;
#pragma unroll
  for (int ti = 0; ti < 7; ++ti) {
    const int tap = wave + 4 * ti;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int row = tap * P.Cg + 4 * q4 + e;
      if (row < P.kpad_w) slab[(int64_t)row * P.cn_pad + r16] = acc[ti][e];
    }
  }
}

// x-column reuse for the transposed operand reads (round 2): a k-step is 32 voxels of ONE x plane (4 y rows x 8 z), so the x^T
// fragment of output plane p for tap (dx,dy,dz) IS the fragment of halo plane p+1+dx for tap (0,dy,dz).  Eight waves = two k halves
// (y rows 0-3 / 4-7 of every plane) x four groups of (dy,dz) combos {0,1,2} {3,4} {5,6} {7,8 + the all-ones pseudo tap}: per combo a
// wave reads the six halo-plane fragments of its half once (12 ds_read_b64_tr_b16) and feeds 12 MFMAs (3 dx x 4 planes) against the
// four dy fragments of its half — 280 transposed reads per tile instead of 512.  The two k halves accumulate into two slabs.
template <int NPX, int NPD>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(4, 4))) void conv_wgrad_head2_kernel(const WgradHaloArgs P, int total_tiles, int x_sample_bytes, int d_sample_bytes) {
  using ST = HeadStage<NPX, NPD, 512>;
  constexpr int JX = ST::JX, XN = ST::XN;
  __shared__ __attribute__((aligned(16))) char smem[ST::BUF + WH_NRM_MAXN * 128];
  float* const sPar = reinterpret_cast<float*>(smem + ST::BUF);     // per sample: 4 channel quads x (mean x 4, rstd x 4)
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r16 = lane & 15, q4 = lane >> 4;
  const int tq = r16 >> 2, tp = r16 & 3;
  const ST stg(P, tid);
  u32x2 rx[JX], rd[ST::JD];

  // operand normalisation on load (the arithmetic of instnorm_prelu_fwd_kernel, rounded to bf16 as that pass rounds): x pieces only;
  // halo voxels outside the volume and channels >= in_C stay 0.
  const bool nrm = P.in_mr != nullptr;
  const float nrm_al = nrm ? P.in_alpha[0] : 1.f;
  if (nrm)
    for (int i = tid; i < P.N * 32; i += 512) {
      const int n = i >> 5, k = i & 31, c = (k >> 3) * 4 + (k & 3);
      sPar[i] = c < P.in_C ? P.in_mr[((int64_t)n * P.in_C + c) * 2 + ((k >> 2) & 1)] : 0.f;
    }
  auto sstore = [&](int t) {
    if (!nrm) {
      stg.store_x(smem, tid, rx);
    } else {
      const TileOrigin o = tile_origin<4, 8, 8>(t, P.tiles, P.tyn, P.tzn);
      const uint32_t xm = ST::x_outside(P, o);
      const float* par = sPar + o.n * 32;
#pragma unroll
      for (int j = 0; j < JX; ++j) {
        const int part = (tid + j * 512) % NPX;
        const f32x4 mean = *reinterpret_cast<const f32x4*>(par + part * 8), rstd = *reinterpret_cast<const f32x4*>(par + part * 8 + 4);
        float v[4] = {h2f<BF16>(rx[j][0] & 0xffffu), h2f<BF16>(rx[j][0] >> 16), h2f<BF16>(rx[j][1] & 0xffffu), h2f<BF16>(rx[j][1] >> 16)};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float a = (v[e] - mean[e]) * rstd[e];
          v[e] = a > 0.f ? a : nrm_al * a;
        }
        const u32x2 w = (stg.xh[j] & xm) == 0u ? u32x2{pack2<BF16>(v[0], v[1]), pack2<BF16>(v[2], v[3])} : u32x2{0u, 0u};
        if (JX * 512 == XN || tid + j * 512 < XN) *reinterpret_cast<u32x2*>(smem + stg.xl[j]) = w;
      }
    }
    stg.store_d(smem, tid, rd);
  };
  const int kh = wave >> 2, cg = wave & 3;               // k half, combo group
  // first (dy,dz) combo of the group, how many.  Waves w and w + 4 (the two k halves of one combo group) share a SIMD: with the same
  // partition {3,2,2,2} in both halves that SIMD ran 72 of the tile's 224 MFMAs (and 3 + 3 of the 18 operand-read groups) against 48 /
  // 48 / 56 on the others and every barrier waited for it.  Round 4: the second half takes {2,3,2,2}: 60 / 60 / 48 / 56.
  const int c0 = kh == 0 ? (cg == 0 ? 0 : 2 * cg + 1) : (cg == 0 ? 0 : cg == 1 ? 2 : 2 * cg + 1);
  const int nco = kh == 0 ? (cg == 0 ? 3 : 2) : (cg == 1 ? 3 : 2);
  f32x4 acc[3][3], acc_ps = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ci = 0; ci < 3; ++ci)
#pragma unroll
    for (int dxi = 0; dxi < 3; ++dxi) acc[ci][dxi] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int lz = 4 * (q4 & 1) + tq, ly = q4 >> 1;
  const bf16x8 ones = bias_ones_frag(r16);
  auto compute = [&]() {
    const char* xs = smem;
    const char* ds = xs + ST::XBYTES;
    const int yb = 4 * kh;
    bf16x8 df[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) df[p] = wh_frag(ds + (((p * 8) + (yb + ly)) * 8 + lz) * 32 + tp * 8, 2 * 8 * 32);
    const int hb0 = (yb + ly + 1) * 10 + (lz + 1);          // halo voxel of this lane in plane 0, before the (dy,dz) shift
#pragma unroll
    for (int ci = 0; ci < 3; ++ci) {
      if (ci < nco) {                                        // wave-uniform
        const int dyz = P.delta[9 + c0 + ci];                // taps 9..17 are the dx = 0 group: delta = dy * 10 + dz
        bf16x8 xf[6];
#pragma unroll
        for (int q = 0; q < 6; ++q) xf[q] = wh_frag(xs + (q * 100 + hb0 + dyz) * 32 + tp * 8, 2 * 10 * 32);
#pragma unroll
        for (int dxi = 0; dxi < 3; ++dxi)
#pragma unroll
          for (int p = 0; p < 4; ++p) {
            if constexpr ((WH_ABL & 1) != 0) { acc[ci][dxi][0] += __builtin_bit_cast(f32x4, xf[p + dxi])[0] * __builtin_bit_cast(f32x4, df[p])[1]; continue; }   // (timing only)
            acc[ci][dxi] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xf[p + dxi], df[p], acc[ci][dxi], 0, 0, 0);
          }
      }
    }
    if (cg == 3) {       // pseudo tap 27: row 0 accumulates sum(dy) (bias gradient)
#pragma unroll
      for (int p = 0; p < 4; ++p) acc_ps = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, df[p], acc_ps, 0, 0, 0);
    }
  };

  const TileSeq seq = xcd_tile_seq([] { return blockIdx.x; }, gridDim.x, total_tiles);
  ST::zero_pads(smem, tid);
  __syncthreads();          // the operand-normalisation table is written
  head_tile_loop(seq, [&](int t) { stg.gload(P, t, x_sample_bytes, d_sample_bytes, rx, rd); }, compute, sstore);

  float* slab = P.ws + ((int64_t)blockIdx.x * 2 + kh) * P.kpad_w * P.cn_pad;       // one slab per k half
#pragma unroll
  for (int ci = 0; ci < 3; ++ci) {
    if (ci >= nco) continue;
#pragma unroll
    for (int dxi = 0; dxi < 3; ++dxi) {
      const int tap = dxi * 9 + c0 + ci;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int row = tap * P.Cg + 4 * q4 + e;
        if (row < P.kpad_w) slab[(int64_t)row * P.cn_pad + r16] = acc[ci][dxi][e];
      }
    }
  }
  if (cg == 3) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int row = 27 * P.Cg + 4 * q4 + e;
      if (row < P.kpad_w) slab[(int64_t)row * P.cn_pad + r16] = acc_ps[e];
    }
  }
}

// (Round 4, measured and not kept — source under tools/experiments/: the same pass with LDS-DMA staging in 12-byte pieces into a ring of
// three buffers, requests two tiles ahead, an explicit s_waitcnt vmcnt(4) and ONE barrier per tile, 96 registers: parity-green, and
// 0.68 ms against 0.51 alone, +0.2 ms/step.  With two pieces per 24-byte voxel a tile is 27 DMA instructions of 768 useful bytes, and a
// DMA instruction costs its wave 60-185 issue cycles; the register-staged loop pays 6 cheap loads and 6 ds_write_b64 per lane instead.)
bool wgrad_halo_eligible(const ctseg_wgrad_desc* d) {
  if (d->dtype != CTSEG_BF16 || d->ntaps != 27 || d->sin != 1) return false;
  const int vb = d->Cg * 2, db = ((d->Cn + 15) / 16) * 32;
  if (!(vb == 32 || vb == 64) || !(db == 32 || db == 64)) return false;
  if (d->Xr != d->Xi || d->Yr != d->Yi || d->Zr != d->Zi || d->Zr < 4) return false;
  // rows 16-byte chunked, or 12 wide (24 bytes) on a 32-byte-plane operand
  const bool x_ok = d->g_ld % 8 == 0 || (vb == 32 && d->g_ld == 12), d_ok = d->d_ld % 8 == 0 || (db == 32 && d->d_ld == 12);
  if (!x_ok || !d_ok || d->d_ld < d->Cn || ((uintptr_t)d->in % 16) || ((uintptr_t)d->dy % 16)) return false;
  if (d->d_ld % 8 == 0 && d->d_ld < db / 2) return false;
  if (d->cn_pad < db / 2) return false;
  if ((int64_t)d->Xi * d->Yi * d->Zi * (d->g_ld > d->d_ld ? d->g_ld : d->d_ld) * 2 >= (1ll << 31)) return false;  // 32-bit per-sample byte offsets
  return taps_within_unit_cube(d);
}

// Which kernel of this file serves an eligible descriptor, and its instantiation: the one place that decides it.  The launcher
// dispatches on it; the grid / slab sizing, ctseg_wgrad_in_norm_ok and ctseg_wgrad_pass_name report it.
enum class WhKernel { HALO, HEAD, HEAD2 };      // conv_wgrad_halo_kernel<a, b, .> (plane bytes), conv_wgrad_head_kernel / head2<a, b> (8-byte pieces per row)
struct WgradHaloVariant { WhKernel k; int a, b; };
static WgradHaloVariant wgrad_halo_variant(const ctseg_wgrad_desc* d) {
  const int vb = d->Cg * 2, db = ((d->Cn + 15) / 16) * 32;
  if (!(vb == 32 && db == 32 && (d->g_ld == 12 || d->g_ld == 16) && (d->d_ld == 12 || d->d_ld == 16))) return {WhKernel::HALO, vb, db};
  // the x-column reuse indexes taps as dx * 9 + (dy, dz): canonical order only
  return {taps_canonical_27(d) ? WhKernel::HEAD2 : WhKernel::HEAD, d->g_ld / 4, d->d_ld / 4};
}

static int wgrad_halo_grid(const ctseg_wgrad_desc* d) {
  const int tiles = ((d->Xr + 3) / 4) * ((d->Yr + 7) / 8) * ((d->Zr + 7) / 8) * d->N;
  const WgradHaloVariant v = wgrad_halo_variant(d);
  // more workgroups per CU than this measured no faster with the single staging buffer (0.245 / 0.250 / 0.255 ms at 1 / 2 / 3
  // per CU for the 32->32 layer); the smaller LDS footprint is kept for what it leaves to the main stream's kernels
  int per_cu = (v.a + v.b <= 64) ? 2 : 1;
  if (v.k != WhKernel::HALO)
    per_cu = v.k == WhKernel::HEAD2 ? 1 : 4;      // 27 KB of LDS, 128 registers: four 4-wave or two 8-wave workgroups per CU would fit.
  // ONE 8-wave workgroup per CU for the head kernel: alone it is slower that way (0.43 -> 0.50 ms), inside the step — it runs on the
  // side stream beside the main stream's HBM-bound head passes — faster: 9.94 / 9.90 -> 9.86 / 9.82 ms/step (same box, round 2)
  if (const char* e = getenv("CTSEG_WH_PER_CU")) per_cu = atoi(e);
  return persistent_grid(CTSEG_NUM_CU * per_cu, tiles);
}

static bool wgrad_head2(const ctseg_wgrad_desc* d) { return wgrad_halo_variant(d).k == WhKernel::HEAD2; }

bool wgrad_halo_in_norm_ok(const ctseg_wgrad_desc* d) { return wgrad_halo_eligible(d) && wgrad_head2(d) && d->N <= WH_NRM_MAXN && d->in_norm_C <= 12; }

int wgrad_halo_slabs(const ctseg_wgrad_desc* d) { return wgrad_head2(d) ? 2 * wgrad_halo_grid(d) : wgrad_halo_grid(d); }

// name of the kernel launch_wgrad_halo runs (ctseg_wgrad_pass_name); a variant outside the table has no kernel: NULL
const char* wgrad_halo_name(const ctseg_wgrad_desc* d) {
  static const struct { WhKernel k; int a, b; const char* name; } NAMES[] = {
      {WhKernel::HEAD2, 3, 3, "x-column head 12/12"}, {WhKernel::HEAD2, 3, 4, "x-column head 12/16"},
      {WhKernel::HEAD2, 4, 3, "x-column head 16/12"}, {WhKernel::HEAD2, 4, 4, "x-column head 16/16"},
      {WhKernel::HEAD, 3, 3, "head 12/12"},           {WhKernel::HEAD, 3, 4, "head 12/16"},
      {WhKernel::HEAD, 4, 3, "head 16/12"},           {WhKernel::HEAD, 4, 4, "head 16/16"},
      {WhKernel::HALO, 32, 32, "halo 32x32"},         {WhKernel::HALO, 32, 64, "halo 32x64"},
      {WhKernel::HALO, 64, 32, "halo 64x32"},         {WhKernel::HALO, 64, 64, "halo 64x64"}};
  const WgradHaloVariant v = wgrad_halo_variant(d);
  for (const auto& e : NAMES)
    if (e.k == v.k && e.a == v.a && e.b == v.b) return e.name;
  return nullptr;
}

void launch_wgrad_halo(const ctseg_wgrad_desc* d, hipStream_t st) {
  WgradHaloArgs a;
  a.in = (const char*)d->in; a.dy = (const char*)d->dy; a.ws = d->ws;
  a.N = d->N; a.X = d->Xr; a.Y = d->Yr; a.Z = d->Zr; a.Cg = d->Cg; a.g_ld = d->g_ld; a.d_ld = d->d_ld;
  a.kpad_w = d->kpad_w; a.cn_pad = d->cn_pad;
  a.in_mr = d->in_mean_rstd; a.in_alpha = d->in_alpha; a.in_C = d->in_norm_C;
  a.txn = (d->Xr + 3) / 4; a.tyn = (d->Yr + 7) / 8; a.tzn = (d->Zr + 7) / 8;
  a.tiles = a.txn * a.tyn * a.tzn;
  for (int j = 0; j < 28; ++j) {
    int v = 0;
    if (j < 27) {
      const int tp = d->taps[j];
      v = (tap_dx(tp) * 10 + tap_dy(tp)) * 10 + tap_dz(tp);
    }
    a.delta[j] = v;
  }
  const int total = a.tiles * d->N, grid = wgrad_halo_grid(d);
  const WgradHaloVariant v = wgrad_halo_variant(d);
  if (v.k != WhKernel::HALO) {
    const int xsb = (int)((int64_t)d->Xi * d->Yi * d->Zi * d->g_ld * 2), dsb = (int)((int64_t)d->Xi * d->Yi * d->Zi * d->d_ld * 2);
    const bool v2 = v.k == WhKernel::HEAD2;
#define WH_GO(NX, ND)                                                                                                       \
  do {                                                                                                                      \
    if (v2) hipLaunchKernelGGL((conv_wgrad_head2_kernel<NX, ND>), dim3(grid), dim3(512), 0, st, a, total, xsb, dsb);    \
    else hipLaunchKernelGGL((conv_wgrad_head_kernel<NX, ND>), dim3(grid), dim3(256), 0, st, a, total, xsb, dsb);             \
  } while (0)
    if (v.a == 3) { if (v.b == 3) WH_GO(3, 3); else WH_GO(3, 4); }
    else { if (v.b == 3) WH_GO(4, 3); else WH_GO(4, 4); }
#undef WH_GO
  } else if (v.a == 32 && v.b == 32) hipLaunchKernelGGL((conv_wgrad_halo_kernel<32, 32, 4>), dim3(grid), dim3(256), 0, st, a, total);
  else if (v.a == 32) hipLaunchKernelGGL((conv_wgrad_halo_kernel<32, 64, 4>), dim3(grid), dim3(256), 0, st, a, total);
  else if (v.b == 32) hipLaunchKernelGGL((conv_wgrad_halo_kernel<64, 32, 4>), dim3(grid), dim3(256), 0, st, a, total);
  else hipLaunchKernelGGL((conv_wgrad_halo_kernel<64, 64, 8>), dim3(grid), dim3(512), 0, st, a, total);
}

}  // namespace ctseg
