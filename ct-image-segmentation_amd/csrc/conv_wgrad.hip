// Weight-gradient pass for gfx950: R[slot*Cg + a][b] = sum_rows in[row*sin + d(slot)][a] * dy[row][b]
// (autograd's Conv3d / ConvTranspose3d weight + bias backward in the reference's training step,
// capstone/volumetric/base_trainer.py:80-82 -> loss.backward()).
//
// The contraction runs over voxels (rows), which is the SLOW axis of both channels-last operands, so
// the MFMA fragments need a transpose: bf16 uses ds_read_b64_tr_b16 (hardware transposed LDS read,
// 4 voxels x 16 channels per 16-lane group); fp32 feeds v_mfma_f32_16x16x4_f32 one element per lane,
// which needs none.  A workgroup owns 128 K-rows x BNW columns and a contiguous row range of one
// sample (split-K); partial tiles go to fp32 slabs that ctseg_conv_wgrad_reduce sums in fixed order
// (deterministic) straight into the torch weight layout.  K index ntaps*Cg is a virtual all-ones
// gathered channel, so its row of R is the bias gradient.
#include "wgrad_common.h"

namespace ctseg {

struct WgradKArgs : WgradGeom {   // step: 32 rows
  int kblocks, cblocks;   // > 0: flat grid, workgroup -> (K block, column block, slab) by slab_xcd_decode
  int addr64;             // 1: a sample of the gathered operand is >= 2 GiB (or CTSEG_WGRAD_ADDR64): 64-bit address chain per chunk
};

// GLDS (bf16, 16-byte-chunked gather, >= 64 columns): operands go global -> LDS directly (global_load_lds, no VGPR staging,
// no ds_write pass).  The LDS image is then lane-linear (no row padding), so the bank spread the padding gave the transposed
// reads comes from an XOR of the 32-byte column slot with the row instead, applied on the SOURCE side (which chunk a lane
// fetches) and in the read address: 256-byte rows: slot ^ (row & 7); 128-byte rows: slot ^ ((row >> 1) & 3).
__device__ __attribute__((aligned(16))) unsigned short g_wg_zero16[8] = {0, 0, 0, 0, 0, 0, 0, 0};
__device__ __attribute__((aligned(16))) unsigned short g_wg_one16[8] = {0x3f80, 0, 0, 0, 0, 0, 0, 0};   // bf16 1.0 on channel 0

template <typename T, int BNW, bool SMALLC> struct WgradCfg {
  static constexpr int SZ = TT<T>::SZ;
  static constexpr bool GLDS = SZ == 2 && !SMALLC && BNW >= 64;
  static constexpr int PA = GLDS ? 256 : 128 * SZ + (SZ == 2 ? 32 : 64);
  static constexpr int PD = GLDS ? BNW * 2 : BNW * SZ + ((SZ == 2) ? (BNW == 16 ? 64 : 32) : 64);
  static constexpr int STAGE = 32 * (PA + PD);
};

template <typename T, int BNW, int WK, int WC, bool SMALLC>
__global__ __launch_bounds__(256) void conv_wgrad_kernel(const WgradKArgs P) {
  constexpr int SZ = TT<T>::SZ, EPC = TT<T>::EPC;
  using CF = WgradCfg<T, BNW, SMALLC>;
  constexpr int PA = CF::PA, PD = CF::PD;
  constexpr bool GLDS = CF::GLDS;
  constexpr int KT = 128 / WK / 16, CT = BNW / WC / 16;
  constexpr int ACPR = 128 / EPC;            // 16-byte chunks per gathered row (16 bf16 / 32 fp32)
  constexpr int AJ = 32 * ACPR / 256;        // gathered chunks per thread per stage (2 / 4)
  constexpr int ARS = 256 / ACPR;            // row stride between a thread's chunks (16 / 8)
  constexpr int DCPR = BNW / EPC;            // chunks per dy row
  constexpr int DJ = (32 * DCPR + 255) / 256;
  static_assert(WK * WC == 4 && KT >= 1 && CT >= 1, "4 waves");

  __shared__ __attribute__((aligned(16))) char smem[2 * CF::STAGE];
  __shared__ int sTap[32];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid < 32) sTap[tid] = tid < P.ntaps ? P.taps[tid] : 0;
  __syncthreads();
  const int wk = wave / WC, wc = wave % WC;
  const int r16 = lane & 15, q4 = lane >> 4;
  int kblock, cblock, zslab;
  if (P.kblocks > 0) {
    const SlabTile st = slab_xcd_decode(blockIdx.x, P.kblocks * P.cblocks);
    zslab = st.zslab;
    kblock = st.tile % P.kblocks;
    cblock = st.tile / P.kblocks;
  } else {
    kblock = blockIdx.x; cblock = blockIdx.y; zslab = blockIdx.z;
  }
  const int col0 = cblock * BNW;
  const int n = zslab / P.splits, sp = zslab % P.splits;
  const int mstart = sp * P.rows_per_split;
  int mend = mstart + P.rows_per_split;
  if (mend > P.rows) mend = P.rows;
  const int nst = (mend > mstart) ? (mend - mstart + 31) / 32 : 0;

  // ---- fixed K position of this thread's gathered chunks -----------------------------------------
  const int arow0 = tid / ACPR;
  // GLDS: the thread's LDS position is (row, tid % 16); it holds logical chunk ((slot32 ^ (row & 7)) << 1) | low
  const int acc_c = GLDS ? (((((tid % ACPR) >> 1) ^ (arow0 & 7)) << 1) | (tid & 1)) : tid % ACPR;
  const int kpos = kblock * 128 + acc_c * EPC;
  const int ktot = P.ntaps * P.Cg;
  const int slot = kpos / P.Cg, ci = kpos - slot * P.Cg;
  const bool kvalid = kpos < ktot, kones = kpos == ktot;
  int dx = 0, dy_ = 0, dz = 0;
  if (kvalid) {
    const int tp = sTap[slot & 31];
    dx = tap_dx(tp); dy_ = tap_dy(tp); dz = tap_dz(tp);
  }
  int cx[AJ], cy[AJ], cz[AJ];
#pragma unroll
  for (int j = 0; j < AJ; ++j) {
    int m = mstart + arow0 + j * ARS;
    cz[j] = m % P.Zr; int t = m / P.Zr;
    cy[j] = t % P.Yr; cx[j] = t / P.Yr;
  }
  const int64_t nbase = (int64_t)n * P.Xi;
  const char* dbase = P.dy + ((int64_t)n * P.rows * P.d_ld + col0) * SZ;

  u32x4 ra[AJ], rd[DJ];
  u32x4 ones = {0u, 0u, 0u, 0u};
  ones[0] = (SZ == 4) ? 0x3f800000u : 0x3f80u;
  auto gload = [&](int s) {
    const int mb = mstart + s * 32;
#pragma unroll
    for (int j = 0; j < AJ; ++j) {
      const int m = mb + arow0 + j * ARS;
      u32x4 v = {0u, 0u, 0u, 0u};
      if constexpr (SMALLC) {
        // gathered channel count is not a multiple of the 16-byte chunk (the Cin = 1 stem): element-wise gather
        if (m < mend) {
          uint32_t el[EPC];
#pragma unroll
          for (int t = 0; t < EPC; ++t) {
            const int kp = kpos + t;
            uint32_t val = 0u;
            if (kp < ktot) {
              const int sl = kp / P.Cg, c = kp - sl * P.Cg;
              const int tp = sTap[sl & 31];
              const int xi = cx[j] * P.sin + tap_dx(tp), yi = cy[j] * P.sin + tap_dy(tp), zi = cz[j] * P.sin + tap_dz(tp);
              if ((unsigned)xi < (unsigned)P.Xi && (unsigned)yi < (unsigned)P.Yi && (unsigned)zi < (unsigned)P.Zi) {
                const int64_t vox = ((nbase + xi) * P.Yi + yi) * P.Zi + zi;
                const char* p = P.in + (vox * P.g_ld + c) * SZ;
                if constexpr (SZ == 4) val = *reinterpret_cast<const uint32_t*>(p);
                else val = *reinterpret_cast<const unsigned short*>(p);
              }
            } else if (kp == ktot) {
              val = (SZ == 4) ? 0x3f800000u : 0x3f80u;
            }
            el[t] = val;
          }
          if constexpr (SZ == 4) { v[0] = el[0]; v[1] = el[1]; v[2] = el[2]; v[3] = el[3]; }
          else {
#pragma unroll
            for (int t = 0; t < 4; ++t) v[t] = el[2 * t] | (el[2 * t + 1] << 16);
          }
        }
      } else if (m < mend) {
        if (kvalid) {
          const int xi = cx[j] * P.sin + dx, yi = cy[j] * P.sin + dy_, zi = cz[j] * P.sin + dz;
          if ((unsigned)xi < (unsigned)P.Xi && (unsigned)yi < (unsigned)P.Yi && (unsigned)zi < (unsigned)P.Zi) {
            const int64_t vox = ((nbase + xi) * P.Yi + yi) * P.Zi + zi;
            v = *reinterpret_cast<const u32x4*>(P.in + (vox * P.g_ld + ci) * SZ);
          }
        } else if (kones) {
          v = ones;
        }
      }
      ra[j] = v;
      // advance this chunk's row by 32 (mixed radix z,y,x)
      cz[j] += P.step.sz; if (cz[j] >= P.Zr) { cz[j] -= P.Zr; ++cy[j]; }
      cy[j] += P.step.sy; if (cy[j] >= P.Yr) { cy[j] -= P.Yr; ++cx[j]; }
      cx[j] += P.step.sx;
    }
#pragma unroll
    for (int j = 0; j < DJ; ++j) {
      const int idx = tid + j * 256;
      u32x4 v = {0u, 0u, 0u, 0u};
      if (idx < 32 * DCPR) {
        const int r = idx / DCPR, dc = idx - r * DCPR;
        const int m = mb + r;
        if (m < mend && col0 + dc * EPC < P.d_valid)
          v = *reinterpret_cast<const u32x4*>(dbase + ((int64_t)m * P.d_ld + dc * EPC) * SZ);
      }
      rd[j] = v;
    }
  };
  typedef const __attribute__((address_space(1))) void* gptr_t;
  typedef __attribute__((address_space(3))) void* lptr_t;
  // GLDS: dy chunk this thread's LDS position holds (source-side swizzle, see WgradCfg)
  const int d_row0 = tid / DCPR, d_pos = tid % DCPR;
  const int d_c32 = (BNW == 128) ? ((d_pos >> 1) ^ (d_row0 & 7)) : ((d_pos >> 1) ^ ((d_row0 >> 1) & 3));
  const int d_chunk = (d_c32 << 1) | (d_pos & 1);
  // GLDS addressing without multiplies (the 64-bit voxel -> byte chain of gload() above is ~12 quarter-rate multiplies per chunk and
  // stage; with two chunks and 16 MFMAs per stage the address code, not the matrix pipe, bounded the kernel at ~30 % MFMA):
  // a chunk walks its rows with a RowWalk, 32 rows per stage.  Samples >= 2 GiB keep the 64-bit chain (P.addr64).
  const int gl = P.g_ld * SZ;
  const char* inb = P.in + (int64_t)n * P.Xi * P.Yi * P.Zi * gl;
  const RowStepK K = row_step_k(P, gl);
  RowWalk aw[AJ];             // (off: of THIS chunk, its tap and channel included)
  if constexpr (GLDS) {
#pragma unroll
    for (int j = 0; j < AJ; ++j) {
      aw[j] = RowWalk{cx[j] * P.sin, cy[j] * P.sin, cz[j] * P.sin, 0};
      aw[j].off = (((aw[j].x + dx) * P.Yi + aw[j].y + dy_) * P.Zi + aw[j].z + dz) * gl + ci * SZ;
    }
  }
  const bool dcol_ok = col0 + d_chunk * EPC < P.d_valid;
  int doff = (d_row0 * P.d_ld + d_chunk * EPC) * SZ;                     // byte offset of this thread's first dy chunk in the stage
  const char* dstage = dbase + (int64_t)mstart * P.d_ld * SZ;              // (uniform) first row of the split
  const int d_step = 32 * P.d_ld * SZ, d_jstep = (256 / DCPR) * P.d_ld * SZ;
  auto gload_lds = [&](int s, int buf) {
    const int mb = mstart + s * 32;
    char* a = smem + buf * CF::STAGE + wave * 1024;
    char* d = smem + buf * CF::STAGE + 32 * PA + wave * 1024;
#pragma unroll
    for (int j = 0; j < AJ; ++j) {
      const int m = mb + arow0 + j * ARS;
      const char* src = reinterpret_cast<const char*>(g_wg_zero16);
      const int xi = aw[j].x + dx, yi = aw[j].y + dy_, zi = aw[j].z + dz;
      const bool inside = (unsigned)xi < (unsigned)P.Xi && (unsigned)yi < (unsigned)P.Yi && (unsigned)zi < (unsigned)P.Zi;
      if (m < mend) {
        if (kvalid) {
          if (inside) src = P.addr64 ? P.in + ((((nbase + xi) * P.Yi + yi) * P.Zi + zi) * P.g_ld + ci) * SZ : inb + (uint32_t)aw[j].off;
        } else if (kones) {
          src = reinterpret_cast<const char*>(g_wg_one16);
        }
      }
      aw[j].advance(K);
      __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(a + j * (ARS * PA)), 16, 0, 0);
    }
#pragma unroll
    for (int j = 0; j < DJ; ++j) {
      const int m = mb + d_row0 + j * (256 / DCPR);
      const char* src = (m < mend && dcol_ok) ? dstage + (uint32_t)(doff + j * d_jstep) : reinterpret_cast<const char*>(g_wg_zero16);
      __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(d + j * 4096), 16, 0, 0);
    }
    doff += d_step;
  };
  // The same stage through range-checked buffer loads (every K block but the one holding the all-ones bias row, samples < 2 GiB):
  // a voxel outside the volume, a row past the split or a column past d_valid is an out-of-range offset (the hardware delivers
  // zeros) -- no zero page, no 64-bit pointer arithmetic, one select per chunk.
  const bool use_buf = GLDS && !P.addr64 && !(kblock * 128 <= ktot && ktot < kblock * 128 + 128);
  const i32x4 rsA = make_rsrc(inb, (uint32_t)((int64_t)P.Xi * P.Yi * P.Zi * gl));
  const i32x4 rsD = make_rsrc(dstage, (uint32_t)((int64_t)(mend > mstart ? mend - mstart : 0) * P.d_ld * SZ));
  int doffb = dcol_ok ? doff : (int)0x80000000;          // (stays out of range: rows * row bytes < 2^31)
  auto gload_lds_buf = [&](int s, int buf) {
    const int mb = mstart + s * 32;
    char* a = smem + buf * CF::STAGE + wave * 1024;
    char* d = smem + buf * CF::STAGE + 32 * PA + wave * 1024;
#pragma unroll
    for (int j = 0; j < AJ; ++j) {
      const int m = mb + arow0 + j * ARS;
      const bool ok = m < mend && kvalid && (unsigned)(aw[j].x + dx) < (unsigned)P.Xi && (unsigned)(aw[j].y + dy_) < (unsigned)P.Yi &&
                      (unsigned)(aw[j].z + dz) < (unsigned)P.Zi;
      const int vo = ok ? aw[j].off : (int)0x80000000;
      aw[j].advance(K);
      raw_buffer_load_lds(rsA, (lds_u32_ptr)(a + j * (ARS * PA)), 16, vo, 0, 0, 0);
    }
#pragma unroll
    for (int j = 0; j < DJ; ++j) raw_buffer_load_lds(rsD, (lds_u32_ptr)(d + j * 4096), 16, doffb + j * d_jstep, 0, 0, 0);
    doffb += d_step;
  };
  auto sstore = [&](int buf) {
    char* a = smem + buf * CF::STAGE;
    char* d = a + 32 * PA;
#pragma unroll
    for (int j = 0; j < AJ; ++j) *reinterpret_cast<u32x4*>(a + (arow0 + j * ARS) * PA + acc_c * 16) = ra[j];
#pragma unroll
    for (int j = 0; j < DJ; ++j) {
      const int idx = tid + j * 256;
      if (idx < 32 * DCPR) {
        const int r = idx / DCPR, dc = idx - r * DCPR;
        *reinterpret_cast<u32x4*>(d + r * PD + dc * 16) = rd[j];
      }
    }
  };

  f32x4 acc[KT][CT];
#pragma unroll
  for (int i = 0; i < KT; ++i)
#pragma unroll
    for (int j = 0; j < CT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  if (nst > 0) {
    if constexpr (GLDS) { if (use_buf) gload_lds_buf(0, 0); else gload_lds(0, 0); }
    else { gload(0); sstore(0); }
  }
  __syncthreads();
  for (int s = 0; s < nst; ++s) {
    const int buf = s & 1;
    if (s + 1 < nst) {
      if constexpr (GLDS) { if (use_buf) gload_lds_buf(s + 1, buf ^ 1); else gload_lds(s + 1, buf ^ 1); }   // streams into the other buffer while this one feeds the MFMAs
      else gload(s + 1);
    }
    const char* a = smem + buf * CF::STAGE;
    const char* d = a + 32 * PA;
    if constexpr (SZ == 2) {
      // transposed reads: lane supplies row (4*q4 + (r16>>2)) [+16], columns 4*(r16&3).. of its 16-column block
      const int mrow = 4 * q4 + (r16 >> 2), pc = (r16 & 3) * 4;
      bf16x8 af[KT], df[CT];
#pragma unroll
      for (int i = 0; i < KT; ++i) {
        const char* p = GLDS ? a + mrow * PA + ((((wk * KT + i) ^ (mrow & 7)) << 5) + (pc << 1))
                             : a + mrow * PA + (((wk * KT + i) * 16 + pc) << 1);
        af[i] = tr16_frag(p, 16 * PA);
      }
#pragma unroll
      for (int j = 0; j < CT; ++j) {
        const char* p = GLDS ? d + mrow * PD + ((((wc * CT + j) ^ (BNW == 128 ? (mrow & 7) : ((mrow >> 1) & 3))) << 5) + (pc << 1))
                             : d + mrow * PD + (((wc * CT + j) * 16 + pc) << 1);
        df[j] = tr16_frag(p, 16 * PD);
      }
#pragma unroll
      for (int i = 0; i < KT; ++i)
#pragma unroll
        for (int j = 0; j < CT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], df[j], acc[i][j], 0, 0, 0);
    } else {
#pragma unroll
      for (int st = 0; st < 8; ++st) {
        const int m = 4 * st + q4;
        float af[KT], df[CT];
#pragma unroll
        for (int i = 0; i < KT; ++i) af[i] = *reinterpret_cast<const float*>(a + m * PA + (((wk * KT + i) * 16 + r16) << 2));
#pragma unroll
        for (int j = 0; j < CT; ++j) df[j] = *reinterpret_cast<const float*>(d + m * PD + (((wc * CT + j) * 16 + r16) << 2));
#pragma unroll
        for (int i = 0; i < KT; ++i)
#pragma unroll
          for (int j = 0; j < CT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i], df[j], acc[i][j], 0, 0, 0);
      }
    }
    if constexpr (!GLDS) { if (s + 1 < nst) sstore(buf ^ 1); }
    __syncthreads();
  }

  float* slab = P.ws + ((int64_t)zslab * P.kpad_w + kblock * 128) * P.cn_pad + col0;
#pragma unroll
  for (int i = 0; i < KT; ++i)
#pragma unroll
    for (int j = 0; j < CT; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int row = (wk * KT + i) * 16 + 4 * q4 + e, col = (wc * CT + j) * 16 + r16;
        slab[(int64_t)row * P.cn_pad + col] = acc[i][j][e];
      }
}

template <int NSUB>
__global__ __launch_bounds__(32 * NSUB) void wgrad_reduce_kernel(const float* __restrict__ ws, int nslabs, int kpad_w, int cn_pad, int A, int AS, int T,
                                    int col0, int nb, float* __restrict__ dw, float* __restrict__ db) {
  // block = 32 (k,b) elements x NSUB strided sub-sums over the slabs, combined in fixed order (deterministic);
  // consecutive threads walk b (contiguous in the slab).  NSUB = 32 for the many-slab / few-element case (the stem: 1024
  // slabs x 896 elements ran 28 blocks of 128 serial loads each)
  __shared__ float s_part[NSUB][32];
  const int64_t total = (int64_t)(T * AS + 1) * nb;
  const int64_t slab = (int64_t)kpad_w * cn_pad;
  const int el = threadIdx.x & 31, sub = threadIdx.x >> 5;
  for (int64_t base = (int64_t)blockIdx.x * 32; base < total; base += (int64_t)gridDim.x * 32) {
    const int64_t i = base + el;
    int k = 0, b = 0;
    float s = 0.f;
    if (i < total) {
      k = (int)(i / nb);
      b = (int)(i - (int64_t)k * nb);
      const float* p = ws + (int64_t)k * cn_pad + col0 + b;
      for (int q = sub; q < nslabs; q += NSUB) s += p[q * slab];
    }
    s_part[sub][el] = s;
    __syncthreads();
    if (sub == 0 && i < total) {
      float t8 = 0.f;
#pragma unroll
      for (int q = 0; q < NSUB; ++q) t8 += s_part[q][el];
      if (k == T * AS) {
        if (db != nullptr) db[b] = t8;
      } else {
        const int t = k / AS, a = k - t * AS;
        if (a < A) dw[((int64_t)b * A + a) * T + t] = t8;
      }
    }
    __syncthreads();
  }
}

// Vectorised reduce: 8 lanes x float4 cover up to 128 contiguous bytes of a slab row, 32 strided sub-sums per block (256 threads),
// combined in fixed order; ceil(rows * ceil(nb / 4) / 8) blocks.  (The scalar kernel above moves 128 B per half wave with 8
// sub-sums: 1 - 1.5 TB/s on the 30 - 67 MB of slabs of a persistent LDS-halo weight-gradient kernel, 12 + 6 launches per step of
// the reference's network.)  col0 a multiple of 4; columns nb .. roundup(nb, 4) are pad columns of the slab (read, not written).
// <= 32 registers (modest unrolling): a block then fits beside the persistent one-workgroup-per-CU halo kernels of the main stream
// (2 x 240 of a SIMD's 512 registers, <= 154 KB of LDS) instead of waiting for them to end; same summation order.
// One body for the single call (LW a template argument) and the batched one (LW read from the job).
__device__ __forceinline__ void reduce4_core(f32x4* s_part, int LW, int block, const float* __restrict__ ws, int nslabs, int kpad_w, int cn_pad,
                                             int A, int AS, int T, int col0, int nb, float* __restrict__ dw, float* __restrict__ db) {
  const int NSUB = 256 / LW;        // s_part[sub * LW + el]
  const int nb4 = (nb + 3) >> 2, total4 = (T * AS + 1) * nb4;
  const int64_t slab = (int64_t)kpad_w * cn_pad;
  const int el = threadIdx.x % LW, sub = threadIdx.x / LW;
  const int i4 = block * LW + el;
  const int k = i4 / nb4, b0 = (i4 - k * nb4) * 4;
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  if (i4 < total4) {
    const float* p = ws + (int64_t)k * cn_pad + col0 + b0;
#pragma unroll 2
    for (int q = sub; q < nslabs; q += NSUB) s += *reinterpret_cast<const f32x4*>(p + q * slab);
  }
  s_part[sub * LW + el] = s;
  __syncthreads();
  if (sub == 0 && i4 < total4) {
    f32x4 t = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int q = 0; q < NSUB; ++q) t += s_part[q * LW + el];
    if (k == T * AS) {
      if (db != nullptr)
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (b0 + e < nb) db[b0 + e] = t[e];
    } else {
      const int tt = k / AS, a = k - tt * AS;
      if (a < A)
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (b0 + e < nb) dw[((int64_t)(b0 + e) * A + a) * T + tt] = t[e];
    }
  }
}

template <int LW, int NSUB>      // LW lanes x float4 along a slab row, NSUB strided sub-sums: (8, 32) for many slabs, (32, 8) for few
__global__ __launch_bounds__(256) __attribute__((amdgpu_num_vgpr(32))) void wgrad_reduce4_kernel(const float* __restrict__ ws, int nslabs, int kpad_w, int cn_pad, int A, int AS, int T,
                                                            int col0, int nb, float* __restrict__ dw, float* __restrict__ db) {
  static_assert(LW * NSUB == 256, "256 threads");
  __shared__ f32x4 s_part[256];
  reduce4_core(s_part, LW, blockIdx.x, ws, nslabs, kpad_w, cn_pad, A, AS, T, col0, nb, dw, db);
}

// wgrad_reduce4_kernel for a table of passes: block -> job by a scan of the (few) block0 entries, then reduce4_core with
// LW = job.lanes (8 or 32): the same strided sub-sums, the same combine order.
__global__ __launch_bounds__(256) __attribute__((amdgpu_num_vgpr(32))) void wgrad_reduce_batch_kernel(const ctseg_reduce_job* __restrict__ jobs, int n_jobs) {
  __shared__ f32x4 s_part[256];
  int j = 0;
  while (j + 1 < n_jobs && (int)blockIdx.x >= jobs[j + 1].block0) ++j;       // (uniform: scalar loads)
  const ctseg_reduce_job J = jobs[j];
  reduce4_core(s_part, J.lanes, (int)blockIdx.x - J.block0, J.ws, J.nslabs, J.kpad_w, J.cn_pad, J.A, J.Astride, J.T, J.col0, J.nb, J.dw, J.db);
}

bool wgrad_up_eligible(const ctseg_wgrad_desc* d);
int wgrad_up_slabs(const ctseg_wgrad_desc* d);
void launch_wgrad_up(const ctseg_wgrad_desc* d, hipStream_t st);
const char* wgrad_up_name(const ctseg_wgrad_desc* d);
bool wgrad_stem_eligible(const ctseg_wgrad_desc* d);
bool wgrad_stem_dyn_ok(const ctseg_wgrad_desc* d);
int wgrad_stem_slabs(const ctseg_wgrad_desc* d);
void launch_wgrad_stem(const ctseg_wgrad_desc* d, hipStream_t st);
const char* wgrad_stem_name(const ctseg_wgrad_desc* d);
bool wgrad_halo_eligible(const ctseg_wgrad_desc* d);
int wgrad_halo_slabs(const ctseg_wgrad_desc* d);
bool wgrad_halo_in_norm_ok(const ctseg_wgrad_desc* d);
void launch_wgrad_halo(const ctseg_wgrad_desc* d, hipStream_t st);
const char* wgrad_halo_name(const ctseg_wgrad_desc* d);
bool wgrad_ring_eligible(const ctseg_wgrad_desc* d);
int wgrad_ring_wgs_per_slab(const ctseg_wgrad_desc* d, int32_t* stage_bytes);
void launch_wgrad_ring(const ctseg_wgrad_desc* d, int rows_per_split, hipStream_t st);
const char* wgrad_ring_name(const ctseg_wgrad_desc* d);

enum class WgradPass { HALO, UP, STEM, RING, GENERIC };

// the gathered operand is not in whole 16-byte chunks: the generic kernel stages it element-wise (its SMALLC instantiation)
static bool wgrad_small_operand(const ctseg_wgrad_desc* d) {
  const int EPC = d->dtype == CTSEG_F32 ? 4 : 8;
  return (d->Cg % EPC) != 0 || (d->g_ld % EPC) != 0 || ((uintptr_t)d->in % 16) != 0;
}

// The one place that orders the weight-gradient passes: the first eligible family runs.  CTSEG_NO_WGRAD_UP and CTSEG_WGRAD_RING=0
// (test / A/B switches, read per call: tests flip them inside one process) skip UP and RING.
static WgradPass select_wgrad_pass(const ctseg_wgrad_desc* d) {
  if (wgrad_halo_eligible(d)) return WgradPass::HALO;
  if (getenv("CTSEG_NO_WGRAD_UP") == nullptr && wgrad_up_eligible(d)) return WgradPass::UP;
  if (wgrad_stem_eligible(d)) return WgradPass::STEM;
  const char* ring = getenv("CTSEG_WGRAD_RING");
  if (!(ring != nullptr && atoi(ring) == 0) && !wgrad_small_operand(d) && wgrad_ring_eligible(d)) return WgradPass::RING;
  return WgradPass::GENERIC;
}

// dY formed on load (ctseg_wgrad_desc::dyn_*): the stem pass of a first layer only
static bool wgrad_dy_norm_ok(const ctseg_wgrad_desc* d, WgradPass p) {
  return d->dyn_col0 > 0 && d->in_mean_rstd == nullptr && p == WgradPass::STEM && wgrad_stem_dyn_ok(d);
}

// The instantiation conv_wgrad_kernel<T, bnw, ., ., smallc> of the generic family: the one place that decides it (the entry point
// dispatches on it, ctseg_conv_wgrad_wgs_per_slab sizes by it, ctseg_wgrad_pass_name reports it)
struct WgradGenericTile { int bnw; bool smallc; };
static WgradGenericTile wgrad_generic_tile(const ctseg_wgrad_desc* d) { return {ctseg_wgrad_tile_cols(d->Cn), wgrad_small_operand(d)}; }

// 12-wide bf16 rows of a 16-channel gathered operand: the LDS-halo and stride-2 transposed kernels only
static bool wgrad_rows12_ok(const ctseg_wgrad_desc* d, WgradPass p) {
  return p == WgradPass::HALO || p == WgradPass::UP || d->dtype != CTSEG_BF16 || d->g_ld != 12 || d->Cg != 16;
}

// What the entry point refuses apart from null operands and slab sizes, as the message it reports; NULL: nothing.  Shared with
// ctseg_wgrad_pass_name, which names only what the launch would run.  _early: before a pass can be selected.
static const char* wgrad_refusal_early(const ctseg_wgrad_desc* d) {
  if (d->dtype != CTSEG_F32 && d->dtype != CTSEG_BF16) return "conv_wgrad: bad dtype";
  if (!(d->ntaps >= 1 && d->ntaps <= CTSEG_MAX_TAPS && d->splits >= 1)) return "conv_wgrad: ntaps/splits";
  return nullptr;
}
static const char* wgrad_refusal(const ctseg_wgrad_desc* d, WgradPass pass) {
  const int EPC = d->dtype == CTSEG_F32 ? 4 : 8;
  const bool halo = pass == WgradPass::HALO;     // (also moves 12-wide bf16 rows: ctseg_wgrad_narrow_ok)
  if (d->dyn_g != nullptr) {
    if (!(wgrad_dy_norm_ok(d, pass) && d->dyn_y && d->dyn_mean_rstd && d->dyn_alpha && d->dyn_sums &&
          ((uintptr_t)d->dyn_g % 16) == 0 && ((uintptr_t)d->dyn_y % 16) == 0))
      return "conv_wgrad: dyn_* (dY formed on load) is not implemented for this pass (ask ctseg_wgrad_dy_norm_ok)";
  } else if (d->dyn_col0 != 0) {
    return "conv_wgrad: dyn_col0 without dyn_g";
  }
  if (d->in_mean_rstd != nullptr && !(halo && wgrad_halo_in_norm_ok(d) && d->in_alpha != nullptr))
    return "conv_wgrad: in_mean_rstd (normalise the operand on load) is not implemented for this pass (ask ctseg_wgrad_in_norm_ok)";
  if (!((d->d_ld % EPC == 0 || halo) && ((uintptr_t)d->dy % 16) == 0)) return "conv_wgrad: dy must be 16-byte chunked";
  if (!wgrad_rows12_ok(d, pass)) return "conv_wgrad: 12-wide rows need an LDS-halo kernel";
  return nullptr;
}

template <typename T, bool SMALLC> static void launch_wgrad(WgradKArgs& a, int bnw, hipStream_t st) {
  const int kb = a.kpad_w / 128, cb = a.cn_pad / bnw, zs = a.N * a.splits;
  dim3 grid((unsigned)kb, (unsigned)cb, (unsigned)zs);
  a.kblocks = a.cblocks = 0;
  a.addr64 = ((int64_t)a.Xi * a.Yi * a.Zi * a.g_ld * (int64_t)sizeof(T) >= ((int64_t)1 << 31) - 4096 || getenv("CTSEG_WGRAD_ADDR64") != nullptr) ? 1 : 0;
  if (slab_grid_is_flat(zs, kb * cb)) {
    a.kblocks = kb; a.cblocks = cb;
    grid = dim3((unsigned)(kb * cb * zs), 1u, 1u);
  }
  if (bnw == 16) hipLaunchKernelGGL((conv_wgrad_kernel<T, 16, 4, 1, SMALLC>), grid, dim3(256), 0, st, a);
  else if (bnw == 32) hipLaunchKernelGGL((conv_wgrad_kernel<T, 32, 2, 2, SMALLC>), grid, dim3(256), 0, st, a);
  else if (bnw == 64) hipLaunchKernelGGL((conv_wgrad_kernel<T, 64, 2, 2, SMALLC>), grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL((conv_wgrad_kernel<T, 128, 2, 2, SMALLC>), grid, dim3(256), 0, st, a);
}

}  // namespace ctseg

using namespace ctseg;

extern "C" int ctseg_wgrad_tile_cols(int32_t Cn) { return Cn <= 16 ? 16 : Cn <= 32 ? 32 : Cn <= 64 ? 64 : 128; }

// number of fp32 slabs [kpad_w][cn_pad] a ctseg_conv_wgrad call with this descriptor writes into `ws`
extern "C" int ctseg_conv_wgrad_slabs(const ctseg_wgrad_desc* d) {
  if (!desc_ok(d)) return -1;
  switch (select_wgrad_pass(d)) {
    case WgradPass::HALO: return wgrad_halo_slabs(d);
    case WgradPass::UP: return wgrad_up_slabs(d);
    case WgradPass::STEM: return wgrad_stem_slabs(d);
    default: return d->N * d->splits;
  }
}

extern "C" int ctseg_conv_wgrad_wgs_per_slab(const ctseg_wgrad_desc* d, int32_t* per_cu, int32_t* stage_bytes) {
  if (per_cu) *per_cu = 0;
  if (stage_bytes) *stage_bytes = 0;
  if (!desc_ok(d)) return -1;
  switch (select_wgrad_pass(d)) {
    case WgradPass::RING:
      if (per_cu) *per_cu = 1;
      return wgrad_ring_wgs_per_slab(d, stage_bytes);
    case WgradPass::GENERIC: {
      const int bnw = wgrad_generic_tile(d).bnw;
      if (per_cu) *per_cu = 4;
      if (stage_bytes) *stage_bytes = 32 * (128 + bnw) * (d->dtype == CTSEG_F32 ? 4 : 2);
      return (d->kpad_w / 128) * (d->cn_pad / bnw);
    }
    default: return 0;
  }
}

extern "C" int ctseg_wgrad_in_norm_ok(const ctseg_wgrad_desc* d) { return (desc_ok(d) && d->dtype == CTSEG_BF16 && wgrad_halo_in_norm_ok(d)) ? 1 : 0; }

extern "C" int ctseg_wgrad_dy_norm_ok(const ctseg_wgrad_desc* d) {
  if (!desc_ok(d) || d->dyn_col0 <= 0 || d->in_mean_rstd != nullptr) return 0;
  return wgrad_dy_norm_ok(d, select_wgrad_pass(d)) ? 1 : 0;
}

extern "C" int ctseg_wgrad_narrow_ok(const ctseg_wgrad_desc* d) {
  if (!desc_ok(d)) return 0;
  const WgradPass p = select_wgrad_pass(d);
  // the stride-2 transposed-conv kernel takes a 12-wide gathered operand
  return (p == WgradPass::HALO || (p == WgradPass::UP && d->d_ld != 12)) ? 1 : 0;
}

// The kernel a launch of this descriptor runs, by the helper its launcher dispatches on (wgrad_halo_variant, wgrad_up_width,
// wgrad_stem_variant, wring_kind, wgrad_generic_tile), for tests that must know a shape still lands on the kernel they were
// written for.  NULL: rejected, or refused by the checks the launch shares with it (wgrad_refusal_early, wgrad_refusal).
extern "C" const char* ctseg_wgrad_pass_name(const ctseg_wgrad_desc* d) {
  if (!desc_ok(d) || wgrad_refusal_early(d) != nullptr) return nullptr;
  if (d->N <= 0 || d->Cg <= 0 || d->Cn <= 0 || d->Xr <= 0 || d->Yr <= 0 || d->Zr <= 0) return nullptr;
  const WgradPass p = select_wgrad_pass(d);
  if (wgrad_refusal(d, p) != nullptr) return nullptr;
  switch (p) {
    case WgradPass::HALO: return wgrad_halo_name(d);
    case WgradPass::UP: return wgrad_up_name(d);
    case WgradPass::STEM: return wgrad_stem_name(d);
    case WgradPass::RING: return wgrad_ring_name(d);
    case WgradPass::GENERIC: break;
  }
  static const struct { int bnw; bool smallc; const char* name; } NAMES[] = {
      {16, false, "generic 16"},  {32, false, "generic 32"},  {64, false, "generic 64"},  {128, false, "generic 128"},
      {16, true, "generic 16 element-wise"}, {32, true, "generic 32 element-wise"}, {64, true, "generic 64 element-wise"},
      {128, true, "generic 128 element-wise"}};
  const WgradGenericTile t = wgrad_generic_tile(d);
  for (const auto& e : NAMES)
    if (e.bnw == t.bnw && e.smallc == t.smallc) return e.name;
  return nullptr;
}

extern "C" int ctseg_conv_wgrad(const ctseg_wgrad_desc* d, void* stream) {
  CTSEG_REQUIRE_DESC(d, "conv_wgrad");
  CTSEG_REQUIRE(d->in && d->dy && d->ws, "conv_wgrad: null pointer");
  const char* why = wgrad_refusal_early(d);
  CTSEG_REQUIRE(why == nullptr, "%s", why);
  const int SZ = d->dtype == CTSEG_F32 ? 4 : 2;
  const WgradPass pass = select_wgrad_pass(d);
  why = wgrad_refusal(d, pass);
  CTSEG_REQUIRE(why == nullptr, "%s", why);
  const WgradGenericTile gt = wgrad_generic_tile(d);
  const int bnw = gt.bnw;
  const int ktot = d->ntaps * d->Cg;
  hipStream_t st = (hipStream_t)stream;
  switch (pass) {
    case WgradPass::HALO:
      CTSEG_REQUIRE(d->kpad_w >= ktot + 16 && d->cn_pad >= ((d->Cn + 15) / 16) * 16, "conv_wgrad: slab too small for the halo kernel");
      launch_wgrad_halo(d, st);
      CTSEG_LAUNCH_CHECK("conv_wgrad_halo");
      return 0;
    case WgradPass::UP:
      launch_wgrad_up(d, st);
      CTSEG_LAUNCH_CHECK("conv_wgrad_up");
      return 0;
    case WgradPass::STEM:
      launch_wgrad_stem(d, st);
      CTSEG_LAUNCH_CHECK("conv_wgrad_stem");
      return 0;
    default: break;
  }
  // the ring and generic kernels: `splits` row ranges per sample, 32-row aligned, addressed with 32-bit offsets
  CTSEG_REQUIRE(d->kpad_w % 128 == 0 && d->kpad_w >= ktot + 1, "conv_wgrad: kpad_w %d (K=%d)", d->kpad_w, ktot);
  CTSEG_REQUIRE(d->cn_pad % bnw == 0 && d->cn_pad >= d->Cn, "conv_wgrad: cn_pad %d", d->cn_pad);
  const int64_t rows64 = (int64_t)d->Xr * d->Yr * d->Zr;
  CTSEG_REQUIRE(rows64 < (1ll << 31) - 4096, "conv_wgrad: row grid too large");
  int rps = (int)((rows64 + d->splits - 1) / d->splits);
  rps = ((rps + 31) / 32) * 32;
  CTSEG_REQUIRE((int64_t)(rps + 64) * d->d_ld * SZ < ((int64_t)1 << 31), "conv_wgrad: rows per split * row bytes exceed 32-bit offsets (raise splits)");
  if (pass == WgradPass::RING) {
    launch_wgrad_ring(d, rps, st);
    CTSEG_LAUNCH_CHECK("conv_wgrad_ring");
    return 0;
  }
  WgradKArgs a;
  wgrad_geom_fill(a, d, rps);
  a.step = radix_step(32, d->Zr, d->Yr);
  if (d->dtype == CTSEG_F32) { if (gt.smallc) launch_wgrad<float, true>(a, bnw, st); else launch_wgrad<float, false>(a, bnw, st); }
  else { if (gt.smallc) launch_wgrad<BF16, true>(a, bnw, st); else launch_wgrad<BF16, false>(a, bnw, st); }
  CTSEG_LAUNCH_CHECK("conv_wgrad");
  return 0;
}

extern "C" int ctseg_conv_wgrad_reduce(const float* ws, int32_t nslabs, int32_t kpad_w, int32_t cn_pad, int32_t A, int32_t AS,
                                       int32_t T, int32_t col0, int32_t nb, float* dw, float* db, void* stream) {
  CTSEG_REQUIRE(ws && dw && nslabs >= 1 && A <= AS && T * AS + 1 <= kpad_w && col0 + nb <= cn_pad, "wgrad_reduce: bad arguments");
  const int64_t total = (int64_t)(T * AS + 1) * nb;
  if (ctseg_conv_wgrad_reduce_batch_ok(ws, cn_pad, col0, nb)) {
    const int total4 = (T * AS + 1) * ((nb + 3) / 4);
    if (nslabs >= 64)
      hipLaunchKernelGGL((wgrad_reduce4_kernel<8, 32>), dim3((unsigned)((total4 + 7) / 8)), dim3(256), 0, (hipStream_t)stream, ws, nslabs, kpad_w,
                         cn_pad, A, AS, T, col0, nb, dw, db);
    else
      hipLaunchKernelGGL((wgrad_reduce4_kernel<32, 8>), dim3((unsigned)((total4 + 31) / 32)), dim3(256), 0, (hipStream_t)stream, ws, nslabs, kpad_w,
                         cn_pad, A, AS, T, col0, nb, dw, db);
    CTSEG_LAUNCH_CHECK("wgrad_reduce4");
    return 0;
  }
  int blocks = (int)((total + 31) / 32);
  if (blocks > 8192) blocks = 8192;
  if (nslabs >= 256 && blocks <= 1024)
    hipLaunchKernelGGL(wgrad_reduce_kernel<32>, dim3(blocks), dim3(1024), 0, (hipStream_t)stream, ws, nslabs, kpad_w, cn_pad, A, AS, T,
                       col0, nb, dw, db);
  else
    hipLaunchKernelGGL(wgrad_reduce_kernel<8>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, ws, nslabs, kpad_w, cn_pad, A, AS, T,
                       col0, nb, dw, db);
  CTSEG_LAUNCH_CHECK("wgrad_reduce");
  return 0;
}

extern "C" int ctseg_conv_wgrad_reduce_batch_ok(const float* ws, int32_t cn_pad, int32_t col0, int32_t nb) {
  return ((col0 & 3) == 0 && (cn_pad & 3) == 0 && col0 + ((nb + 3) & ~3) <= cn_pad && ((uintptr_t)ws & 15) == 0) ? 1 : 0;
}

extern "C" int ctseg_conv_wgrad_reduce_batch(const ctseg_reduce_job* jobs, int32_t n_jobs, int32_t total_blocks, void* stream) {
  CTSEG_REQUIRE(jobs && n_jobs >= 1 && total_blocks >= 1, "wgrad_reduce_batch: bad arguments");
  hipLaunchKernelGGL(wgrad_reduce_batch_kernel, dim3((unsigned)total_blocks), dim3(256), 0, (hipStream_t)stream, jobs, n_jobs);
  CTSEG_LAUNCH_CHECK("wgrad_reduce_batch");
  return 0;
}
