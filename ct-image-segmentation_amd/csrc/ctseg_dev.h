// Device-side helpers shared by the gfx950 kernels (wave = 64 lanes, MFMA 16x16 family).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>

#include "ctseg_hip.h"

#include <stdlib.h>

namespace ctseg {

// The one target: MI355X (gfx950) = 256 CUs in 8 XCDs, 160 KiB of LDS and 4 SIMDs x 512 VGPRs per CU.  Persistent kernels launch
// CTSEG_NUM_CU * k workgroups (k = workgroups that fit a CU) and walk tiles with stride gridDim.x; XCD-aware orders assume 8 XCDs.
constexpr int CTSEG_NUM_CU = 256;
constexpr int CTSEG_NUM_XCD = 8;

// Grid size of a persistent launch: min(wanted, tiles), optionally capped by the TEST-ONLY environment knob CTSEG_MAX_WG=n so that
// small test shapes make every workgroup walk several tiles (the inter-tile paths — prefetch of tile t+1, store of tile t-1, ring-slot
// rotation across an epilogue, statistics flush at a sample change — are otherwise reached only at 512x512x48).  Every sizing query
// (partial-slot / slab counts) goes through the same function as its launch, so the knob must not change between recording a plan
// and running it.  Unset in production.
static inline int persistent_grid(int wanted, int tiles) {
  int g = wanted < tiles ? wanted : tiles;
  if (const char* e = getenv("CTSEG_MAX_WG")) {
    const int cap = atoi(e);
    if (cap >= 1 && cap < g) g = cap;
  }
  return g < 1 ? 1 : g;
}

typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;
typedef __attribute__((ext_vector_type(2))) uint32_t u32x2;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(4))) int32_t i32x4;
typedef s16x4 __attribute__((address_space(3)))* lds_s16x4;     // LDS operand of __builtin_amdgcn_ds_read_tr16_b64_v4i16
typedef uint32_t __attribute__((address_space(3)))* lds_u32_ptr;

// Word 3 of every buffer descriptor here: DATA_FORMAT = 32 (bits 18:15 = 4), untyped dword access, no swizzle, no index stride
constexpr uint32_t BUF_RSRC_CONFIG = 0x00020000u;

// Descriptor of [base, base + bytes) for the __builtin_amdgcn_raw_buffer_* loads and stores: an offset past the range loads zeros
// and drops a store.  base and bytes must be wave-uniform.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buffer_rsrc(const void* base, int bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, bytes, BUF_RSRC_CONFIG);
}

// buffer_load_dword* ... lds (direct-to-LDS DMA): per-lane 32-bit byte offset into a range-checked buffer; an offset past the range
// delivers zeros (the padding voxels of a tap), so a staging loop needs no branch and no zero page.  Its descriptor is the i32x4
// of make_rsrc, its four words read from the first lane so that the compiler holds them in SGPRs.
__device__ void raw_buffer_load_lds(i32x4 rsrc, lds_u32_ptr lds, int size, int voffset, int soffset, int offset,
                                    int aux) __asm("llvm.amdgcn.raw.buffer.load.lds");
__device__ __forceinline__ i32x4 make_rsrc(const void* p, uint32_t bytes) {
  struct __attribute__((packed)) { const void* ptr; uint32_t range; uint32_t config; } r{p, bytes, BUF_RSRC_CONFIG};
  i32x4 v = __builtin_bit_cast(i32x4, r);
  v[0] = __builtin_amdgcn_readfirstlane(v[0]);
  v[1] = __builtin_amdgcn_readfirstlane(v[1]);
  v[2] = __builtin_amdgcn_readfirstlane(v[2]);
  v[3] = __builtin_amdgcn_readfirstlane(v[3]);
  return v;
}

struct BF16 {};  // storage tag: 16-bit brain float kept as raw ushort
struct F16 {};   // storage tag: IEEE half kept as raw ushort (forward / inference passes only)

template <typename T> struct TT;
// H = the 16-bit storage kind whose conversions a kernel body names in branches that are dead for fp32 storage;
// E = what a pointer to such storage points at (both 16-bit kinds travel as raw uint16_t)
template <> struct TT<float> { static constexpr int SZ = 4, EPC = 4, DT = CTSEG_F32; using H = BF16; using E = float; };
template <> struct TT<BF16> { static constexpr int SZ = 2, EPC = 8, DT = CTSEG_BF16; using H = BF16; using E = uint16_t; };
template <> struct TT<F16> { static constexpr int SZ = 2, EPC = 8, DT = CTSEG_F16; using H = F16; using E = uint16_t; };
template <typename T> using elem_t = typename TT<T>::E;

__device__ __forceinline__ float bf2f(uint32_t u16) { return __uint_as_float(u16 << 16); }
__device__ __forceinline__ uint32_t f2bf(float x) {
  __bf16 b = (__bf16)x;  // v_cvt_pk_bf16_f32: RNE, NaN stays NaN
  return (uint32_t)__builtin_bit_cast(unsigned short, b);
}
__device__ __forceinline__ uint32_t pack2bf(float lo, float hi) { return f2bf(lo) | (f2bf(hi) << 16); }

// 16-bit storage kind H (BF16 / F16): element <-> float.  Half stores saturate at +-65504 instead of overflowing to inf (a
// convolution output ahead of its InstanceNorm may be large; its statistics are taken from the fp32 accumulators anyway).
template <typename H> __device__ __forceinline__ float h2f(uint32_t u16);
template <> __device__ __forceinline__ float h2f<BF16>(uint32_t u16) { return bf2f(u16); }
template <> __device__ __forceinline__ float h2f<F16>(uint32_t u16) {
  return (float)__builtin_bit_cast(_Float16, (unsigned short)u16);
}
template <typename H> __device__ __forceinline__ uint32_t f2h(float x);
template <> __device__ __forceinline__ uint32_t f2h<BF16>(float x) { return f2bf(x); }
template <> __device__ __forceinline__ uint32_t f2h<F16>(float x) {
  // RNE.  The clamp is IEEE-754 minimum / maximum (v_minimum3_f32, v_maximum3_f32), which hand a NaN on: NaN stays NaN.  (v_med3_f32
  // drops a NaN operand: it stored a NaN as -65504, a signalling one as +65504.  A select around it spills in conv_halo_sw_kernel.)
  const _Float16 h = (_Float16)__builtin_elementwise_maximum(__builtin_elementwise_minimum(x, 65504.f), -65504.f);
  return (uint32_t)__builtin_bit_cast(unsigned short, h);
}
template <typename H> __device__ __forceinline__ uint32_t pack2(float lo, float hi) { return f2h<H>(lo) | (f2h<H>(hi) << 16); }

// One element of storage kind T (float / BF16 / F16) <-> float: the identity for fp32, h2f / f2h of the kind otherwise
template <typename T> __device__ __forceinline__ float to_float(elem_t<T> e) {
  if constexpr (TT<T>::SZ == 4) return e;
  else return h2f<typename TT<T>::H>(e);
}
template <typename T> __device__ __forceinline__ elem_t<T> from_float(float x) {
  if constexpr (TT<T>::SZ == 4) return x;
  else return (elem_t<T>)f2h<typename TT<T>::H>(x);
}

// Load / store EPC<T> consecutive elements (one 16-byte chunk) as floats.
template <typename T> __device__ __forceinline__ void load_chunk(const char* p, float* v);
template <> __device__ __forceinline__ void load_chunk<float>(const char* p, float* v) {
  f32x4 t = *reinterpret_cast<const f32x4*>(p);
  v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
}
template <> __device__ __forceinline__ void load_chunk<BF16>(const char* p, float* v) {
  u32x4 t = *reinterpret_cast<const u32x4*>(p);
#pragma unroll
  for (int i = 0; i < 4; ++i) { v[2 * i] = bf2f(t[i] & 0xffffu); v[2 * i + 1] = bf2f(t[i] >> 16); }
}
template <> __device__ __forceinline__ void load_chunk<F16>(const char* p, float* v) {
  u32x4 t = *reinterpret_cast<const u32x4*>(p);
#pragma unroll
  for (int i = 0; i < 4; ++i) { v[2 * i] = h2f<F16>(t[i] & 0xffffu); v[2 * i + 1] = h2f<F16>(t[i] >> 16); }
}
template <typename T> __device__ __forceinline__ void store_chunk(char* p, const float* v);
template <> __device__ __forceinline__ void store_chunk<float>(char* p, const float* v) {
  f32x4 t = {v[0], v[1], v[2], v[3]};
  *reinterpret_cast<f32x4*>(p) = t;
}
template <> __device__ __forceinline__ void store_chunk<BF16>(char* p, const float* v) {
  u32x4 t;
#pragma unroll
  for (int i = 0; i < 4; ++i) t[i] = pack2bf(v[2 * i], v[2 * i + 1]);
  *reinterpret_cast<u32x4*>(p) = t;
}

template <> __device__ __forceinline__ void store_chunk<F16>(char* p, const float* v) {
  u32x4 t;
#pragma unroll
  for (int i = 0; i < 4; ++i) t[i] = pack2<F16>(v[2 * i], v[2 * i + 1]);
  *reinterpret_cast<u32x4*>(p) = t;
}

// EP consecutive elements as floats: EP = EPC<T> (one 16-byte chunk) or, for bf16 rows whose stride is an odd multiple of
// 4 elements (10 classes stored 12 wide: 24-byte rows), EP = 4 (an 8-byte chunk; rows are then only 8-byte aligned)
template <typename T, int EP> __device__ __forceinline__ void load_ep(const char* p, float* v) {
  if constexpr (EP == TT<T>::EPC) {
    load_chunk<T>(p, v);
  } else {
    static_assert(EP == 4 && TT<T>::SZ == 2, "half chunks exist for 16-bit storage only");
    using H = typename TT<T>::H;
    const u32x2 t = *reinterpret_cast<const u32x2*>(p);
    v[0] = h2f<H>(t[0] & 0xffffu); v[1] = h2f<H>(t[0] >> 16); v[2] = h2f<H>(t[1] & 0xffffu); v[3] = h2f<H>(t[1] >> 16);
  }
}
template <typename T, int EP> __device__ __forceinline__ void store_ep(char* p, const float* v) {
  if constexpr (EP == TT<T>::EPC) {
    store_chunk<T>(p, v);
  } else {
    static_assert(EP == 4 && TT<T>::SZ == 2, "half chunks exist for 16-bit storage only");
    using H = typename TT<T>::H;
    *reinterpret_cast<u32x2*>(p) = u32x2{pack2<H>(v[0], v[1]), pack2<H>(v[2], v[3])};
  }
}

// 16-byte chunk `second` (0 / 1) of a 12-wide bf16 row (24 bytes, 8-byte aligned) as 8-byte pieces: chunk 0 is two of
// them, chunk 1 is channels 8..11 + zero fill.  (One 16-byte load from the 8-byte aligned address measured 1.4x slower on
// the whole pass: the memory pipeline splits it.)
__device__ __forceinline__ u32x4 load_row12_chunk(const char* p, bool second) {
  const u32x2 lo = *reinterpret_cast<const u32x2*>(p);
  u32x2 hi = {0u, 0u};
  if (!second) hi = *reinterpret_cast<const u32x2*>(p + 8);
  return u32x4{lo[0], lo[1], hi[0], hi[1]};
}

// One bf16 MFMA operand whose contraction index is the SLOW axis of the LDS image (voxels of a channels-last tile): two transposed
// reads (ds_read_b64_tr_b16: 4 rows x 16 columns per 16-lane group) at p0 and p0 + hi_off, the second 16 rows further on.
__device__ __forceinline__ bf16x8 tr16_frag(const char* p0, int hi_off) {
  typedef __attribute__((ext_vector_type(8))) short s16x8;
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4)(p0));
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4)(p0 + hi_off));
  const s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8, v);
}

// ---- packed taps: signed bytes (dx, dy, dz) in bits 0-7, 8-15, 16-23 -------------------------------------------------------------
__host__ __device__ __forceinline__ int tap_dx(int tp) { return (int)(int8_t)(tp & 0xff); }
__host__ __device__ __forceinline__ int tap_dy(int tp) { return (int)(int8_t)((tp >> 8) & 0xff); }
__host__ __device__ __forceinline__ int tap_dz(int tp) { return (int)(int8_t)((tp >> 16) & 0xff); }

// every offset of every tap lies in [lo, hi]
static inline bool taps_within(const int* taps, int ntaps, int lo, int hi) {
  for (int j = 0; j < ntaps; ++j) {
    const int d[3] = {tap_dx(taps[j]), tap_dy(taps[j]), tap_dz(taps[j])};
    for (int v : d)
      if (v < lo || v > hi) return false;
  }
  return true;
}

// the first 27 taps are the 3x3x3 set in torch order, tap j = sign * (j / 9 - 1, (j / 3) % 3 - 1, j % 3 - 1): sign = 1 the forward
// order, -1 the negated order of an input gradient
static inline bool taps_canonical_27(const int* taps, int sign) {
  for (int j = 0; j < 27; ++j)
    if (tap_dx(taps[j]) != sign * (j / 9 - 1) || tap_dy(taps[j]) != sign * ((j / 3) % 3 - 1) || tap_dz(taps[j]) != sign * (j % 3 - 1)) return false;
  return true;
}

// ---- persistent tile kernels -----------------------------------------------------------------------------------------------------
// Tile id -> sample and first voxel of a TX x TY x TZ tile; tiles per sample `tiles`, of which tyn / tzn along y / z (z fastest).
struct TileOrigin { int n, x0, y0, z0; };
template <int TX, int TY, int TZ> __device__ __forceinline__ TileOrigin tile_origin(int t, int tiles, int tyn, int tzn) {
  const int n = t / tiles;
  int r = t - n * tiles;
  const int tz = r % tzn; r /= tzn;
  const int ty = r % tyn, tx = r / tyn;
  return {n, tx * TX, ty * TY, tz * TZ};
}

// n consecutive elements, fp32 or 16-bit kind H by a runtime flag -> floats (n = 4 or 8; pointer aligned to n*size)
template <typename H = BF16> __device__ __forceinline__ void load_n_as_float(const char* p, bool is_f32, int n, float* v) {
  if (is_f32) {
    for (int i = 0; i < n; i += 4) load_chunk<float>(p + 4 * i, v + i);
  } else if (n == 8) {
    load_chunk<H>(p, v);
  } else {
    u32x2 t = *reinterpret_cast<const u32x2*>(p);
    v[0] = h2f<H>(t[0] & 0xffffu); v[1] = h2f<H>(t[0] >> 16); v[2] = h2f<H>(t[1] & 0xffffu); v[3] = h2f<H>(t[1] >> 16);
  }
}

// One element of the InstanceNorm + PReLU backward (what instnorm_prelu_bwd_apply_kernel stores): shared by the apply pass and by
// the passes that form it on load, so that both round the same way
__device__ __forceinline__ float inorm_prelu_bwd_value(float g, float y, float mean, float rstd, float s1, float s2, float al) {
  const float xh = (y - mean) * rstd;
  const float dxh = g * (xh > 0.f ? 1.f : al);
  return rstd * (dxh - s1 - xh * s2);
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ---- host-side error plumbing -------------------------------------------------------------------
void set_error(const char* fmt, ...);
#define CTSEG_REQUIRE(cond, ...)            \
  do {                                      \
    if (!(cond)) {                          \
      ctseg::set_error(__VA_ARGS__);        \
      return -1;                            \
    }                                       \
  } while (0)
#define CTSEG_LAUNCH_CHECK(name)                                         \
  do {                                                                   \
    hipError_t e_ = hipGetLastError();                                   \
    if (e_ != hipSuccess) {                                              \
      ctseg::set_error("%s: %s", name, hipGetErrorString(e_));          \
      return -2;                                                         \
    }                                                                    \
  } while (0)
// the same for an entry point whose name is a run-time string: "<who> (<pass>): <error>"
#define CTSEG_LAUNCH_CHECK_PASS(who, pass)                                        \
  do {                                                                            \
    hipError_t e_ = hipGetLastError();                                            \
    if (e_ != hipSuccess) {                                                       \
      ctseg::set_error("%s (%s): %s", who, pass, hipGetErrorString(e_));          \
      return -2;                                                                  \
    }                                                                             \
  } while (0)

// ABI 2: a descriptor names the size of the struct its caller was compiled against; anything else is a caller built against
// another header (round 2 grew both structs under version 1: the library would read past the end of the old, shorter struct)
template <class D> static inline bool desc_ok(const D* d) { return d != nullptr && d->struct_size == (int32_t)sizeof(D); }
#define CTSEG_REQUIRE_DESC(d, name)                                                                                         \
  CTSEG_REQUIRE(ctseg::desc_ok(d), "%s: descriptor struct_size %d != %d (caller compiled against another ctseg_hip.h; ABI %d)", \
                name, (d) ? (d)->struct_size : -1, (int)sizeof(*(d)), CTSEG_ABI_VERSION)

static inline bool is16(int dtype) { return dtype == CTSEG_BF16 || dtype == CTSEG_F16; }   // 16-bit storage kinds

// Run-time storage kind -> its tag: calls f(float{}), f(BF16{}) or f(F16{}) and returns true.  A code that is none of the three,
// or a kind outside ACCEPT (a mask of 1 << CTSEG_*; no call is instantiated for it), calls nothing and returns false: the entry
// point refuses it.
constexpr unsigned ANY_STORAGE = 1u << CTSEG_F32 | 1u << CTSEG_BF16 | 1u << CTSEG_F16;
template <unsigned ACCEPT = ANY_STORAGE, class F> static inline bool with_dtype(int dtype, F&& f) {
  if constexpr ((ACCEPT >> CTSEG_F32) & 1) if (dtype == CTSEG_F32) return f(float{}), true;
  if constexpr ((ACCEPT >> CTSEG_BF16) & 1) if (dtype == CTSEG_BF16) return f(BF16{}), true;
  if constexpr ((ACCEPT >> CTSEG_F16) & 1) if (dtype == CTSEG_F16) return f(F16{}), true;
  return false;
}

// The raw-image dtypes of the input pipelines (CTSEG_F32 / CTSEG_I16 / CTSEG_U8), and their element types in the same style:
// calls f(float{}), f(short{}) or f(uint8_t{}) and returns true; any other code calls nothing and returns false
static inline bool is_raw_dtype(int dtype) { return dtype == CTSEG_F32 || dtype == CTSEG_I16 || dtype == CTSEG_U8; }
template <class F> static inline bool with_raw_dtype(int dtype, F&& f) {
  if (dtype == CTSEG_F32) return f(float{}), true;
  if (dtype == CTSEG_I16) return f(short{}), true;
  if (dtype == CTSEG_U8) return f(uint8_t{}), true;
  return false;
}

static inline int ilog_ceil_div(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

}  // namespace ctseg
