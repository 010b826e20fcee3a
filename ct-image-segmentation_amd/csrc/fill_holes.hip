// Enclosed holes of a label map filled on gfx950 (what MONAI ships as FillHoles): integers only.
// A hole is a connected component of label 0 that does not reach its sample's boundary and whose neighbours off the background all
// carry ONE class c in 1..C-1; its voxels become c.  The components are those of ctseg_components_label (components.hip) on the
// background map, so the union-find, its termination and its uniqueness are that file's; this one adds three streaming passes.
//   ctseg_fill_holes
//     map      map = (label == 0), the per-voxel border word = 0, the table = 0: every word that a later pass reads or adds to.
//     label    ctseg_components_label(map, C = 2): ids = the component's representative, sizes = its voxel count there.
//     border   one workgroup per tile of 8 x 16 x 32 voxels, the tile's labels in LDS with a halo of one voxel read from the
//              neighbouring tiles (0 outside the sample: no neighbour).  A background voxel gathers bit 0 when it lies on the
//              sample's boundary along an active axis, bit c for every neighbouring class c, bit 16 for a neighbour >= C, and ORs
//              them into word[its representative].
//     rewrite  a lane rewrites a run of 16 labels: a voxel of label 0 whose representative's word is one bit of class_mask (so no
//              bit 0, no bit 16, no second class) and whose component passes max_size takes that class; everything else is copied.
//              table[b][c-1] = {holes filled (counted at representatives), voxels filled}: integer atomic adds, pre-reduced in LDS.
//
// The atomic traffic of the border pass.  Almost all of the background is ONE component, the outside, so its word is the
// destination of nearly every contribution.  Three reductions come before a global atomic: a voxel without a bit (inside the
// background, away from every class and from the boundary: most of them) contributes nothing, and a run of 16 whose 3 x 3 x 18
// neighbourhood holds no label and which touches no boundary is dismissed after 54 LDS words; a lane ORs the consecutive voxels of
// one representative in registers; a tile ORs by representative in an LDS table of 256 slots (a representative whose slot is taken
// goes to memory directly).  What is left is one atomic OR per tile and component, and that one is skipped when a relaxed load
// shows the bits already set: OR only ever sets bits, so a stale value can only cause a redundant OR, never a missing one.
// Integer OR and integer adds commute: two runs give the same bits.  No workgroup waits for another.
#include "label_runs.h"

namespace ctseg {

constexpr int FH_TX = 8, FH_TY = 16, FH_TZ = 32;                 // the tile: that of the labelling pass
constexpr int FH_RUNS = FH_TZ / SD_RUN;
constexpr int FH_ROW = FH_TZ + 8;                                // bytes of an LDS line: voxel z at byte z + 4, z = -1 and TZ around
constexpr int FH_LINES = (FH_TX + 2) * (FH_TY + 2);
constexpr int FH_LAB_WORDS = FH_LINES * FH_ROW / 4;
constexpr int FH_SLOTS = 256;                                    // of the tile's OR table: one per lane for the flush
constexpr uint32_t FH_BOUNDARY = 1u, FH_OTHER = 1u << 16;
static_assert(FH_TX * FH_TY * FH_RUNS == 256 && FH_TZ % SD_RUN == 0 && FH_ROW % 4 == 0 && FH_SLOTS == 256, "one run per lane");
static_assert(SD_MAX_CLASSES <= 16, "bit 16 is the first past the classes");

// offset k of the 27: (k / 9 - 1, k / 3 % 3 - 1, k % 3 - 1)
__host__ __device__ __forceinline__ void fh_offset(int k, int& dx, int& dy, int& dz) {
  dx = k / 9 - 1;
  dy = (k / 3) % 3 - 1;
  dz = k % 3 - 1;
}

// bit k: offset k is a neighbour step: along active axes only, and along 1..connectivity of them
static inline uint32_t fh_offset_mask(int connectivity, int axes) {
  uint32_t m = 0u;
  for (int k = 0; k < 27; ++k) {
    int dx, dy, dz;
    fh_offset(k, dx, dy, dz);
    const int steps = (dx != 0) + (dy != 0) + (dz != 0);
    const bool active = (!dx || (axes & SD_AXIS_X)) && (!dy || (axes & SD_AXIS_Y)) && (!dz || (axes & SD_AXIS_Z));
    if (steps >= 1 && steps <= connectivity && active) m |= 1u << k;
  }
  return m;
}

// Grid (ceil(ceil(N / 16) / 256)).  Lane: 16 consecutive voxels of the launch, and a stride of the table.  WIDE: 16-byte accesses.
template <bool WIDE>
__global__ __launch_bounds__(256) void fill_holes_map_kernel(const uint8_t* __restrict__ labels, int64_t N, uint8_t* __restrict__ map,
                                                             uint32_t* __restrict__ word, int32_t* __restrict__ table,
                                                             int table_words) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  for (int64_t i = g; i < table_words; i += (int64_t)gridDim.x * 256) table[i] = 0;
  const int64_t v0 = g * SD_RUN;
  if (v0 >= N) return;
  const int n = N - v0 < SD_RUN ? (int)(N - v0) : SD_RUN;
  const u32x4 c = load_run<WIDE>(labels + v0, n);
  u32x4 m;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    uint32_t w = 0u;
#pragma unroll
    for (int t = 0; t < 4; ++t)
      if (((c[j] >> (t * 8)) & 255u) == 0u) w |= 1u << (t * 8);
    m[j] = w;
  }
  if constexpr (WIDE) {
    *reinterpret_cast<u32x4*>(map + v0) = m;
#pragma unroll
    for (int j = 0; j < 4; ++j) reinterpret_cast<u32x4*>(word + v0)[j] = u32x4{0u, 0u, 0u, 0u};
  } else {
#pragma unroll
    for (int i = 0; i < SD_RUN; ++i)
      if (i < n) {
        map[v0 + i] = (uint8_t)run_byte(m, i);
        word[v0 + i] = 0u;
      }
  }
}

// bits only ever get set during the border pass: when a load shows them all, the OR would change nothing
__device__ __forceinline__ void fh_global_or(uint32_t* p, uint32_t bits) {
  if ((__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bits) != bits)
    __hip_atomic_fetch_or(p, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Grid (tiles of a sample, B).  Lane: run (tid % 2) of tile line tid / 2, as in the labelling pass.
template <bool WIDE>
__global__ __launch_bounds__(256) void fill_holes_border_kernel(const uint8_t* __restrict__ labels, const int32_t* __restrict__ ids,
                                                                int X, int Y, int Z, int C, uint32_t offsets, int axes, int tyn,
                                                                int tzn, uint32_t* __restrict__ word) {
  __shared__ uint32_t s_lab_w[FH_LAB_WORDS];
  __shared__ int s_key[FH_SLOTS];
  __shared__ uint32_t s_bits[FH_SLOTS];
  uint8_t* s_lab = reinterpret_cast<uint8_t*>(s_lab_w);
  const int tid = threadIdx.x;
  const TileOrigin o = tile_origin<FH_TX, FH_TY, FH_TZ>((int)blockIdx.x, (int)gridDim.x, tyn, tzn);
  for (int i = tid; i < FH_LAB_WORDS; i += 256) s_lab_w[i] = 0u;
  s_key[tid] = -1;
  s_bits[tid] = 0u;
  __syncthreads();
  const int S = X * Y * Z;
  const uint8_t* L = labels + (int64_t)blockIdx.y * S;
  const int line = tid / FH_RUNS, lx = line / FH_TY, ly = line % FH_TY, lz0 = (tid % FH_RUNS) * SD_RUN;
  const int x = o.x0 + lx, y = o.y0 + ly, z0 = o.z0 + lz0;
  const int n = (x < X && y < Y && z0 < Z) ? (Z - z0 < SD_RUN ? Z - z0 : SD_RUN) : 0;    // voxels of the run inside the volume
  const int at = (x * Y + y) * Z + z0;                                                     // (read only where n > 0)
  uint8_t* row = s_lab + ((lx + 1) * (FH_TY + 2) + ly + 1) * FH_ROW + 4 + lz0;
  if (n > 0) {
    const u32x4 c = load_run<WIDE>(L + at, n);
#pragma unroll
    for (int j = 0; j < 4; ++j) reinterpret_cast<uint32_t*>(row)[j] = c[j];
  }
  // the halo: one voxel around the tile, where that lies inside the sample (elsewhere the 0 stays: no label, no bit)
  for (int i = tid; i < FH_LINES * (FH_TZ + 2); i += 256) {
    const int hl = i / (FH_TZ + 2), hz = i % (FH_TZ + 2) - 1;
    const int hx = hl / (FH_TY + 2) - 1, hy = hl % (FH_TY + 2) - 1;
    if ((unsigned)hx < (unsigned)FH_TX && (unsigned)hy < (unsigned)FH_TY && (unsigned)hz < (unsigned)FH_TZ) continue;
    const int gx = o.x0 + hx, gy = o.y0 + hy, gz = o.z0 + hz;
    if ((unsigned)gx < (unsigned)X && (unsigned)gy < (unsigned)Y && (unsigned)gz < (unsigned)Z)
      s_lab[hl * FH_ROW + 4 + hz] = L[(gx * Y + gy) * Z + gz];
  }
  __syncthreads();
  if (n > 0) {
    // the 3 x 3 lines around the run, bytes z0 - 1 .. z0 + 16 and a few more: no label there, no class bit for any voxel of the run
    uint32_t around = 0u;
#pragma unroll
    for (int d = 0; d < 9; ++d) {
      const uint32_t* w = s_lab_w + ((lx + d / 3) * (FH_TY + 2) + ly + d % 3) * (FH_ROW / 4) + lz0 / 4;
#pragma unroll
      for (int j = 0; j < 6; ++j) around |= w[j];
    }
    const bool xy_edge = ((axes & SD_AXIS_X) && (x == 0 || x == X - 1)) || ((axes & SD_AXIS_Y) && (y == 0 || y == Y - 1));
    const bool z_active = (axes & SD_AXIS_Z) != 0;
    if (around != 0u || xy_edge || (z_active && (z0 == 0 || z0 + n == Z))) {
      int cur = -1;
      uint32_t acc = 0u;
      for (int i = 0; i <= n; ++i) {
        uint32_t bits = 0u;
        int r = -1;
        if (i < n && row[i] == 0u) {
          if (xy_edge || (z_active && (z0 + i == 0 || z0 + i == Z - 1))) bits = FH_BOUNDARY;
          if (around != 0u) {
            for (int k = 0; k < 27; ++k) {
              if (!((offsets >> k) & 1u)) continue;
              int dx, dy, dz;
              fh_offset(k, dx, dy, dz);
              const uint32_t v = row[(dx * (FH_TY + 2) + dy) * FH_ROW + i + dz];
              if (v != 0u) bits |= v < (uint32_t)C ? 1u << v : FH_OTHER;
            }
          }
          if (bits != 0u) r = ids[(int64_t)blockIdx.y * S + at + i];
          if ((uint32_t)r >= (uint32_t)S) bits = 0u;                  // (the ids of the labelling pass always are inside)
        }
        if (acc != 0u && (i == n || (bits != 0u && r != cur))) {      // the lane's OR of one representative goes to the tile's table
          const uint32_t slot = ((uint32_t)cur * 2654435761u) >> 24;
          const int prev = atomicCAS(&s_key[slot], -1, cur);
          if (prev == -1 || prev == cur)
            atomicOr(&s_bits[slot], acc);
          else
            fh_global_or(word + (int64_t)blockIdx.y * S + cur, acc);
          acc = 0u;
        }
        if (bits != 0u) {
          cur = r;
          acc |= bits;
        }
      }
    }
  }
  __syncthreads();
  if (s_key[tid] >= 0 && s_bits[tid] != 0u) fh_global_or(word + (int64_t)blockIdx.y * S + s_key[tid], s_bits[tid]);
}

// Grid (ceil(ceil(S / 16) / 256), B).  Lane: 16 consecutive voxels of the sample.  WIDE: S is a multiple of 16.
template <bool WIDE>
__global__ __launch_bounds__(256) void fill_holes_rewrite_kernel(const uint8_t* __restrict__ labels, const int32_t* __restrict__ ids,
                                                                 const int32_t* __restrict__ sizes, const uint32_t* __restrict__ word,
                                                                 int S, int C, uint32_t class_mask, int max_size,
                                                                 uint8_t* __restrict__ out, int32_t* __restrict__ table) {
  __shared__ int s_holes[SD_MAX_CLASSES];
  __shared__ int s_voxels[SD_MAX_CLASSES];
  const int tid = threadIdx.x, b = blockIdx.y;
  if (tid < SD_MAX_CLASSES) {
    s_holes[tid] = 0;
    s_voxels[tid] = 0;
  }
  __syncthreads();
  const int64_t v0 = ((int64_t)blockIdx.x * 256 + tid) * SD_RUN;
  if (v0 < S) {
    const int n = S - v0 < SD_RUN ? (int)(S - v0) : SD_RUN;
    const int64_t base = (int64_t)b * S, at = base + v0;
    const u32x4 c = load_run<WIDE>(labels + at, n);
    u32x4 o = c;
    int cur = -1, filled = 0;
    uint32_t fill = 0u;                                              // the class that the voxels of representative `cur` take, 0: none
#pragma unroll
    for (int i = 0; i < SD_RUN; ++i) {
      if (i < n && run_byte(c, i) == 0u) {
        const int r = ids[at + i];
        if (r != cur) {
          if (filled) atomicAdd(&s_voxels[fill], filled);
          cur = r;
          filled = 0;
          fill = 0u;
          if ((uint32_t)r < (uint32_t)S) {                           // (the ids of the labelling pass always are)
            const uint32_t w = word[base + r];
            // one bit, and that one a class of the mask: no boundary (bit 0), no label past the classes (bit 16), no second class
            if (w != 0u && (w & (w - 1u)) == 0u && (w & class_mask) == w && (max_size == 0 || sizes[base + r] <= max_size))
              fill = (uint32_t)__builtin_ctz(w);
          }
        }
        if (fill) {
          o[i >> 2] |= fill << ((i & 3) * 8);
          ++filled;
          if ((int64_t)r == v0 + i) atomicAdd(&s_holes[fill], 1);
        }
      }
    }
    if (filled) atomicAdd(&s_voxels[fill], filled);
    if constexpr (WIDE) {
      *reinterpret_cast<u32x4*>(out + at) = o;
    } else {
#pragma unroll
      for (int i = 0; i < SD_RUN; ++i)
        if (i < n) out[at + i] = (uint8_t)run_byte(o, i);
    }
  }
  __syncthreads();
  if (tid >= 1 && tid < C) {
    int32_t* t = table + ((int64_t)b * (C - 1) + tid - 1) * 2;
    if (s_holes[tid]) atomicAdd(t, s_holes[tid]);
    if (s_voxels[tid]) atomicAdd(t + 1, s_voxels[tid]);
  }
}

}  // namespace ctseg

using namespace ctseg;

extern "C" int64_t ctseg_fill_holes_workspace_bytes(int32_t B, int32_t X, int32_t Y, int32_t Z, int32_t C) {
  if (check_components_dims("fill_holes_workspace_bytes", B, X, Y, Z, C)) return -1;
  return (int64_t)CTSEG_FILL_HOLES_BYTES_PER_VOXEL * B * X * Y * Z;
}

extern "C" int ctseg_fill_holes(const uint8_t* labels, int32_t B, int32_t X, int32_t Y, int32_t Z, int32_t C, int32_t connectivity,
                                int32_t axes, int32_t class_mask, int32_t max_size, void* workspace, int64_t workspace_bytes,
                                uint8_t* out, int32_t* table, void* stream) {
  CTSEG_REQUIRE(labels && workspace && out && table, "fill_holes: null pointer (labels, workspace, out and table are required)");
  if (check_components_dims("fill_holes", B, X, Y, Z, C)) return -1;
  CTSEG_REQUIRE(connectivity >= 1 && connectivity <= 3, "fill_holes: connectivity is 1, 2 or 3 (got %d)", connectivity);
  CTSEG_REQUIRE(axes >= 1 && axes <= 7, "fill_holes: axes is a mask of X = 1, Y = 2, Z = 4 (got %d)", axes);
  CTSEG_REQUIRE(class_mask >= 0 && (class_mask & ~(((1 << C) - 1) & ~1)) == 0,
                "fill_holes: class_mask has bits of the classes 1..%d only (got 0x%x)", C - 1, class_mask);
  CTSEG_REQUIRE(max_size >= 0, "fill_holes: max_size >= 0 (got %d)", max_size);
  const int64_t N = (int64_t)B * X * Y * Z;
  const int64_t need = CTSEG_FILL_HOLES_BYTES_PER_VOXEL * N;
  CTSEG_REQUIRE(workspace_bytes >= need, "fill_holes: the workspace holds %lld bytes, %lld are needed", (long long)workspace_bytes,
                (long long)need);
  const int S = X * Y * Z;
  const bool wide = S % SD_RUN == 0;
  CTSEG_REQUIRE(((uintptr_t)workspace % 16) == 0 && ((uintptr_t)table % 4) == 0 &&
                    (!wide || (((uintptr_t)labels % 16) == 0 && ((uintptr_t)out % 16) == 0)),
                "fill_holes: unaligned pointer (16 bytes for the workspace, 4 for the table, 16 for labels and out when X * Y * Z is "
                "a multiple of 16)");
  // ids, sizes, word: 4 N bytes each, then the map.  With Z a multiple of 16 so is N, and every part starts on 16 bytes.
  int32_t* ids = (int32_t*)workspace;
  int32_t* sizes = ids + N;
  uint32_t* word = (uint32_t*)(sizes + N);
  uint8_t* map = (uint8_t*)(word + N);
  hipStream_t st = (hipStream_t)stream;
  const int table_words = B * (C - 1) * 2;
  const dim3 all((unsigned)(((N + SD_RUN - 1) / SD_RUN + 255) / 256));
  if (wide)
    hipLaunchKernelGGL(fill_holes_map_kernel<true>, all, dim3(256), 0, st, labels, N, map, word, table, table_words);
  else
    hipLaunchKernelGGL(fill_holes_map_kernel<false>, all, dim3(256), 0, st, labels, N, map, word, table, table_words);
  CTSEG_LAUNCH_CHECK("fill_holes (map)");
  const int rc = ctseg_components_label(map, B, X, Y, Z, 2, connectivity, axes, ids, sizes, stream);
  if (rc != 0) return rc;
  const uint32_t offsets = fh_offset_mask(connectivity, axes);
  const int txn = ilog_ceil_div(X, FH_TX), tyn = ilog_ceil_div(Y, FH_TY), tzn = ilog_ceil_div(Z, FH_TZ);
  const dim3 tiles((unsigned)(txn * tyn * tzn), (unsigned)B);
  if (Z % SD_RUN == 0)
    hipLaunchKernelGGL(fill_holes_border_kernel<true>, tiles, dim3(256), 0, st, labels, ids, X, Y, Z, C, offsets, axes, tyn, tzn, word);
  else
    hipLaunchKernelGGL(fill_holes_border_kernel<false>, tiles, dim3(256), 0, st, labels, ids, X, Y, Z, C, offsets, axes, tyn, tzn, word);
  CTSEG_LAUNCH_CHECK("fill_holes (border)");
  const int64_t runs = ((int64_t)S + SD_RUN - 1) / SD_RUN;
  const dim3 grid((unsigned)((runs + 255) / 256), (unsigned)B);
  if (wide)
    hipLaunchKernelGGL(fill_holes_rewrite_kernel<true>, grid, dim3(256), 0, st, labels, ids, sizes, word, S, C, (uint32_t)class_mask,
                       max_size, out, table);
  else
    hipLaunchKernelGGL(fill_holes_rewrite_kernel<false>, grid, dim3(256), 0, st, labels, ids, sizes, word, S, C, (uint32_t)class_mask,
                       max_size, out, table);
  CTSEG_LAUNCH_CHECK("fill_holes (rewrite)");
  return 0;
}
