// Foreground-biased patch sampling for 3-D training: the centre pick (ctseg_patch_centres: a count pass and a select pass, integer
// arithmetic only) and the crop pass (ctseg_patch3d_to_hwd: the affine pass of augment3d.hip on the source grid itself, its
// translation column moved by a centre that only the device knows).  The rules are in include/ctseg_hip.h.
//
// Count pass: the masks [K][N] (N = D * H * W) are cut into blocks of PC_BLOCK voxels per class; one workgroup counts the set bytes
// of one (class, block) with 16-byte loads at 16-byte aligned ADDRESSES (N need not be a multiple of 16, so a class need not start
// on one: the chunks at both ends of a block are masked down to the block's bytes, and a chunk that is not wholly inside the
// mask array is read byte by byte) and stores the int32 count at workspace[class * nb + block].  Select pass: one workgroup per
// patch sums every class's block counts in a fixed order (the K totals; workgroup 0 stores them behind the counts), picks the
// class and the rank, finds the block by a prefix scan over that class's counts and the voxel by per-lane byte counts of the block's
// chunks and a second scan.  No word is read that the count pass did not write, nothing is accumulated with atomics, and the order
// of every sum is fixed: the workspace may arrive poisoned and two runs give the same bits.
#pragma clang fp contract(off)
#include "resample3d_tile.h"

namespace ctseg {

constexpr int PC_THREADS = 256, PC_BLOCK = 16384, PC_KMAX = 15, PC_PMAX = 16, PC_TOTALS = 16;
constexpr int PC_CHUNKS = PC_BLOCK / 16 + 1;                              // aligned 16-byte chunks an unaligned block can touch
constexpr int PC_PER = (PC_CHUNKS + PC_THREADS - 1) / PC_THREADS;         // ... per thread: 5

struct PatchCentreArgs {
  int K, D, H, W, P, class_mask, has_patch, nb;
  int patch[3];
  unsigned draws[PC_PMAX][3];
};

static inline int64_t pc_blocks(int64_t N) { return (N + PC_BLOCK - 1) / PC_BLOCK; }

// bit 7 of every byte of w that is not zero
__device__ __forceinline__ unsigned pc_flags(unsigned w) { return (((w & 0x7f7f7f7fu) + 0x7f7f7f7fu) | w) & 0x80808080u; }
__device__ __forceinline__ int pc_count(u32x4 v) {
  return __popc(pc_flags(v[0])) + __popc(pc_flags(v[1])) + __popc(pc_flags(v[2])) + __popc(pc_flags(v[3]));
}
__device__ __forceinline__ unsigned pc_low_bytes(long long n) { return n >= 4 ? 0xffffffffu : (n <= 0 ? 0u : (1u << (8 * (int)n)) - 1u); }

// The 16 bytes at the 16-byte aligned address a with every byte outside [lo, hi) zeroed, for a chunk that is not wholly inside
// [lo, hi).  [buf0, buf1) is the mask array, which contains [lo, hi): a chunk that reaches outside it is read byte by byte.
__device__ __forceinline__ u32x4 pc_load16(const uint8_t* masks, uintptr_t a) {                // (from the kernel's pointer: a global load)
  return *reinterpret_cast<const u32x4*>(masks + (int64_t)(a - (uintptr_t)masks));
}
__device__ __forceinline__ u32x4 pc_edge_chunk(const uint8_t* masks, uintptr_t a, uintptr_t lo, uintptr_t hi, uintptr_t buf0,
                                               uintptr_t buf1) {
  u32x4 v = {0u, 0u, 0u, 0u};
  if (a + 16 <= lo || a >= hi) return v;
  if (a >= buf0 && a + 16 <= buf1) {
    v = pc_load16(masks, a);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const long long s = (long long)(a + 4 * i);
      v[i] &= pc_low_bytes((long long)hi - s) & ~pc_low_bytes((long long)lo - s);
    }
  } else {
#pragma unroll
    for (int b = 0; b < 16; ++b) {
      const uintptr_t at = a + b;
      if (at >= lo && at < hi) v[b >> 2] |= (unsigned)masks[(int64_t)(at - buf0)] << (8 * (b & 3));
    }
  }
  return v;
}
__device__ __forceinline__ u32x4 pc_chunk(const uint8_t* masks, uintptr_t a, uintptr_t lo, uintptr_t hi, uintptr_t buf0, uintptr_t buf1) {
  if (a >= lo && a + 16 <= hi) return pc_load16(masks, a);
  return pc_edge_chunk(masks, a, lo, hi, buf0, buf1);
}

// the bytes of block j of class k: [lo, hi)
__device__ __forceinline__ void pc_block_range(uintptr_t buf0, int64_t N, int k, int j, uintptr_t& lo, uintptr_t& hi) {
  const int64_t v0 = (int64_t)j * PC_BLOCK, v1 = v0 + PC_BLOCK < N ? v0 + PC_BLOCK : N;
  lo = buf0 + (uintptr_t)(k * N + v0), hi = buf0 + (uintptr_t)(k * N + v1);
}

__device__ __forceinline__ int pc_wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// exclusive prefix of v over the workgroup's 256 threads in thread order; s_wave: 4 words of LDS
__device__ __forceinline__ int pc_exclusive_scan(int v, int* s_wave) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int x = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int n = __shfl_up(x, o, 64);
    if (lane >= o) x += n;
  }
  __syncthreads();                                        // (the previous use of s_wave has been read)
  if (lane == 63) s_wave[wave] = x;
  __syncthreads();
  int base = 0;
  for (int w = 0; w < wave; ++w) base += s_wave[w];
  return base + x - v;
}

__global__ __launch_bounds__(PC_THREADS) void patch_count_kernel(const uint8_t* __restrict__ masks, int64_t N, int K, int nb,
                                                                 int* __restrict__ counts) {
  __shared__ int s_part[PC_THREADS / 64];
  const int t = threadIdx.x, j = blockIdx.x, k = blockIdx.y;
  const uintptr_t buf0 = (uintptr_t)masks, buf1 = buf0 + (uintptr_t)(K * N);
  uintptr_t lo, hi;
  pc_block_range(buf0, N, k, j, lo, hi);
  const uintptr_t first = lo & ~(uintptr_t)15;
  u32x4 v[PC_PER];
  // the chunks wholly inside the block first, all loads in flight; consecutive lanes read consecutive chunks
#pragma unroll
  for (int i = 0; i < PC_PER; ++i) {
    const uintptr_t a = first + 16 * (uintptr_t)(t + PC_THREADS * i);
    v[i] = u32x4{0u, 0u, 0u, 0u};
    if (a >= lo && a + 16 <= hi) v[i] = pc_load16(masks, a);
  }
#pragma unroll
  for (int i = 0; i < PC_PER; ++i) {
    const uintptr_t a = first + 16 * (uintptr_t)(t + PC_THREADS * i);
    if (a < hi && !(a >= lo && a + 16 <= hi)) v[i] = pc_edge_chunk(masks, a, lo, hi, buf0, buf1);
  }
  int n = 0;
#pragma unroll
  for (int i = 0; i < PC_PER; ++i) n += pc_count(v[i]);
  n = pc_wave_sum(n);
  if ((t & 63) == 0) s_part[t >> 6] = n;
  __syncthreads();
  if (t == 0) counts[k * nb + j] = (s_part[0] + s_part[1]) + (s_part[2] + s_part[3]);
}

__global__ __launch_bounds__(PC_THREADS) void patch_select_kernel(const uint8_t* __restrict__ masks, const PatchCentreArgs p,
                                                                  int* __restrict__ counts, int* __restrict__ centres) {
  __shared__ int s_part[PC_KMAX][PC_THREADS / 64];
  __shared__ int s_wave[PC_THREADS / 64];
  __shared__ int s_found[2];                               // the block and the rank inside it; then the voxel
  const int t = threadIdx.x, pi = blockIdx.x;
  const int K = p.K, nb = p.nb;
  const int64_t N = (int64_t)p.D * p.H * p.W;
  for (int k = 0; k < K; ++k) {
    int n = 0;
    for (int i = t; i < nb; i += PC_THREADS) n += counts[k * nb + i];
    n = pc_wave_sum(n);
    if ((t & 63) == 0) s_part[k][t >> 6] = n;
  }
  if (t < 2) s_found[t] = 0;
  __syncthreads();
  // the class: the (a * m >> 32)-th of the eligible ones
  const unsigned fg = p.draws[pi][0], da = p.draws[pi][1], db = p.draws[pi][2];
  int m = 0;
  for (int k = 0; k < K; ++k) {
    const int n = (s_part[k][0] + s_part[k][1]) + (s_part[k][2] + s_part[k][3]);
    if (pi == 0 && t == 0) counts[K * nb + k] = n;
    m += ((p.class_mask >> k) & 1) && n > 0;
  }
  int cls = -1, ncls = 0;
  if (fg != 0u && m > 0) {
    const int pick = (int)(((unsigned long long)da * (unsigned)m) >> 32);
    int seen = 0;
    for (int k = 0; k < K; ++k) {
      const int n = (s_part[k][0] + s_part[k][1]) + (s_part[k][2] + s_part[k][3]);
      if (((p.class_mask >> k) & 1) && n > 0) {
        if (seen == pick) cls = k, ncls = n;
        ++seen;
      }
    }
  }
  int64_t vox;
  if (cls < 0) {
    vox = (int64_t)(((unsigned long long)db * (unsigned long long)N) >> 32);
  } else {
    const int r = (int)(((unsigned long long)db * (unsigned)ncls) >> 32);
    // the block: thread t owns blocks [t * per, (t + 1) * per)
    const int per = (nb + PC_THREADS - 1) / PC_THREADS;
    const int b0 = t * per < nb ? t * per : nb, b1 = b0 + per < nb ? b0 + per : nb;
    const int* row = counts + cls * nb;
    int mine = 0;
    for (int i = b0; i < b1; ++i) mine += row[i];
    int before = pc_exclusive_scan(mine, s_wave);
    if (before <= r && r < before + mine) {
      for (int i = b0; i < b1; ++i) {
        const int c = row[i];
        if (r < before + c) {
          s_found[0] = i, s_found[1] = r - before;
          break;
        }
        before += c;
      }
    }
    __syncthreads();
    const int blk = s_found[0], rank = s_found[1];
    // the voxel: thread t owns chunks [t * PC_PER, (t + 1) * PC_PER) of the block
    const uintptr_t buf0 = (uintptr_t)masks, buf1 = buf0 + (uintptr_t)(K * N);
    uintptr_t lo, hi;
    pc_block_range(buf0, N, cls, blk, lo, hi);
    const uintptr_t first = (lo & ~(uintptr_t)15) + 16 * (uintptr_t)(t * PC_PER);
    int inside = 0;
#pragma unroll
    for (int i = 0; i < PC_PER; ++i) {
      const uintptr_t a = first + 16 * (uintptr_t)i;
      if (a < hi) inside += pc_count(pc_chunk(masks, a, lo, hi, buf0, buf1));
    }
    int skip = rank - pc_exclusive_scan(inside, s_wave);   // set bytes of this thread's chunks to pass over
    if (skip >= 0 && skip < inside) {
      for (int i = 0; i < PC_PER; ++i) {
        const uintptr_t a = first + 16 * (uintptr_t)i;
        if (a >= hi) break;
        const u32x4 v = pc_chunk(masks, a, lo, hi, buf0, buf1);
        const unsigned w[4] = {v[0], v[1], v[2], v[3]};
        for (int b = 0; b < 16; ++b) {
          if ((w[b >> 2] >> (8 * (b & 3))) & 0xffu) {
            if (skip == 0) s_found[0] = (int)((int64_t)(a + b - buf0) - cls * N);
            --skip;
          }
        }
      }
    }
    __syncthreads();
    vox = s_found[0];
  }
  if (t == 0) {
    const int HW = p.H * p.W;
    int c[3] = {(int)(vox / HW), (int)((vox % HW) / p.W), (int)(vox % p.W)};
    const int dim[3] = {p.D, p.H, p.W};
    if (p.has_patch) {
      for (int a = 0; a < 3; ++a) {
        const int pa = p.patch[a], lo_c = pa / 2, hi_c = dim[a] - (pa - pa / 2);
        c[a] = dim[a] < pa ? dim[a] / 2 : (c[a] < lo_c ? lo_c : (c[a] > hi_c ? hi_c : c[a]));
      }
    }
    centres[4 * pi + 0] = c[0], centres[4 * pi + 1] = c[1], centres[4 * pi + 2] = c[2], centres[4 * pi + 3] = cls;
  }
}

// the crop: the affine tile on the source grid, the translation column moved by the centre (one float32 add per axis)
template <typename TI, int INTERP>
__global__ __launch_bounds__(256) void patch3d_hwd_kernel(const TI* __restrict__ image, const uint8_t* __restrict__ masks, const Aug3dArgs p,
                                                          const int32_t* __restrict__ centre, float* __restrict__ image_out,
                                                          uint8_t* __restrict__ masks_out, uint8_t* __restrict__ labels_out,
                                                          unsigned long long* __restrict__ hist) {
  Aug3dArgs q = p;
  q.m.a[3] = p.m.a[3] + (float)centre[0];
  q.m.a[7] = p.m.a[7] + (float)centre[1];
  q.m.a[11] = p.m.a[11] + (float)centre[2];
  resample3d_tile<Coord::PATCH, TI, INTERP>(image, masks, q, image_out, masks_out, labels_out, hist, nullptr, Deform3dArgs{});
}

static int patch_centres_geometry(const char* who, int32_t K, int32_t D, int32_t H, int32_t W, int64_t& N, int64_t& nb) {
  CTSEG_REQUIRE(K >= 1 && K <= PC_KMAX, "%s: K = %d masks, 1 to %d are taken", who, K, PC_KMAX);
  CTSEG_REQUIRE(D > 0 && H > 0 && W > 0, "%s: bad geometry", who);
  N = (int64_t)D * H * W;
  CTSEG_REQUIRE(N < (1ll << 31), "%s: a volume of 2^31 voxels or more", who);
  nb = pc_blocks(N);
  return 0;
}

}  // namespace ctseg

using namespace ctseg;

extern "C" int64_t ctseg_patch_centres_workspace(int32_t K, int32_t D, int32_t H, int32_t W) {
  int64_t N, nb;
  if (patch_centres_geometry("patch_centres_workspace", K, D, H, W, N, nb)) return -1;
  return 4 * (K * nb + PC_TOTALS);
}

extern "C" int ctseg_patch_centres(const uint8_t* masks, int32_t K, int32_t D, int32_t H, int32_t W, const uint32_t* draws, int32_t P,
                                   int32_t class_mask, const int32_t* patch, void* workspace, int64_t workspace_bytes,
                                   int32_t* centres, void* stream) {
  const char* who = "patch_centres";
  CTSEG_REQUIRE(masks && draws && workspace && centres, "%s: null pointer", who);
  CTSEG_REQUIRE(P >= 1 && P <= PC_PMAX, "%s: P = %d patches, 1 to %d are taken", who, P, PC_PMAX);
  int64_t N, nb;
  if (int rc = patch_centres_geometry(who, K, D, H, W, N, nb)) return rc;
  CTSEG_REQUIRE(workspace_bytes >= 4 * (K * nb + PC_TOTALS), "%s: workspace of %lld bytes, %lld are needed", who,
                (long long)workspace_bytes, (long long)(4 * (K * nb + PC_TOTALS)));
  CTSEG_REQUIRE(((uintptr_t)workspace & 3) == 0 && ((uintptr_t)centres & 3) == 0, "%s: workspace / centres not 4-byte aligned", who);
  PatchCentreArgs p;
  p.K = K, p.D = D, p.H = H, p.W = W, p.P = P, p.class_mask = class_mask, p.has_patch = patch != nullptr, p.nb = (int)nb;
  for (int a = 0; a < 3; ++a) {
    p.patch[a] = patch ? patch[a] : 1;
    CTSEG_REQUIRE(p.patch[a] >= 1, "%s: patch side %d along axis %d", who, p.patch[a], a);
  }
  for (int i = 0; i < PC_PMAX; ++i)
    for (int c = 0; c < 3; ++c) p.draws[i][c] = i < P ? draws[i * 3 + c] : 0u;
  hipLaunchKernelGGL(patch_count_kernel, dim3((unsigned)nb, (unsigned)K), dim3(PC_THREADS), 0, (hipStream_t)stream, masks, N, K, (int)nb,
                     (int*)workspace);
  CTSEG_LAUNCH_CHECK("patch_centres (count)");
  hipLaunchKernelGGL(patch_select_kernel, dim3((unsigned)P), dim3(PC_THREADS), 0, (hipStream_t)stream, masks, p, (int*)workspace, centres);
  CTSEG_LAUNCH_CHECK("patch_centres (select)");
  return 0;
}

extern "C" int ctseg_patch3d_to_hwd(const void* image, int32_t image_dtype, const uint8_t* masks, int32_t K, int32_t D, int32_t H,
                                    int32_t W, int32_t Pd, int32_t Ph, int32_t Pw, const float* matrix, const int32_t* centre,
                                    int32_t interp, int32_t border, float cval, const int32_t* mask_src, int32_t window, float win_lo,
                                    float win_hi, float gain, float bias, float* image_out, uint8_t* masks_out, uint8_t* labels_out,
                                    int64_t* hist, void* stream) {
  Aug3dArgs p;
  dim3 grid;
  if (int rc = augment3d_prepare("patch3d_to_hwd", image, image_dtype, masks, K, D, H, W, Pd, Ph, Pw, matrix, interp, border, cval,
                                 mask_src, window, win_lo, win_hi, gain, bias, image_out, masks_out, labels_out, hist, p, grid))
    return rc;
  CTSEG_REQUIRE(centre, "patch3d_to_hwd: centre is a null pointer");
  p.sD = p.sH = p.sW = 1.f;                                // the matrix addresses the source grid itself: no virtual resized volume
  with_pixel_and_interp(image_dtype, interp, [&](auto ti, auto ic) {
    using TI = decltype(ti);
    hipLaunchKernelGGL((patch3d_hwd_kernel<TI, decltype(ic)::value>), grid, dim3(256), 0, (hipStream_t)stream, (const TI*)image, masks, p,
                       centre, image_out, masks_out, labels_out, (unsigned long long*)hist);
  });
  CTSEG_LAUNCH_CHECK("patch3d_to_hwd");
  return 0;
}
