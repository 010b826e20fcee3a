// Connected components of a label map on gfx950, and the keep-largest / minimum-size clean-up on top of them: integers only.
// A component is a maximal set of voxels of ONE label in 1..C-1 joined by neighbour steps inside its sample; its representative is
// the smallest linear index (x * Y + y) * Z + z among its voxels.  Label equivalence by union-find on parent links that only ever
// decrease, in separate launches in stream order; no workgroup waits for another.
//   ctseg_components_label
//     local    one workgroup per tile of 8 x 16 x 32 voxels.  The tile's labels go to LDS once (a lane loads a run of 16 along Z)
//              inside a border of zeros, so all 13 backward neighbours of a voxel are LDS bytes and a neighbour outside the tile
//              never matches.  Unions on an LDS parent array, a flatten, the voxel count of every local tree (a lane adds up the
//              equal roots of its run first, then one LDS atomic add per change of root).  Writes ids = the local root as an index
//              of the sample (-1 off the classes) and sizes = the local count at a local root, 0 elsewhere: every word of both.
//     merge    voxels on a tile face look at their backward neighbours in OTHER tiles and unite across the face on `ids` itself,
//              the global parent array, with device-scope atomic minima.
//     flatten  ids[v] = root of v; a local root that is no longer a root moves its count to its root (one integer atomic add per
//              tile and component) and zeroes its own.
//   ctseg_components_keep
//     zero, scan (per sample and class: the number of representatives and one 64-bit atomic maximum of size << 32 | ~representative,
//     both pre-reduced in LDS), apply (a lane rewrites a run of 16 labels), table.
//
// Why every find / union loop ends, and why the result does not depend on the schedule.  par[v] <= v holds from the start (par[v] =
// v) and for ever: the only writes are atomic minima with a smaller index and the flatten's store of a root found by walking down.
// A find therefore walks strictly decreasing indices and ends at a v with par[v] == v after at most v steps, whatever it reads on
// the way: every value a link ever held is an ancestor of its voxel in the same component, so a value that is out of date only
// lengthens the walk.  A union that fails to link (its atomic minimum returns old != a: another lane linked a first) goes on with
// old < a in place of a, so its larger end strictly decreases; it ends at the latest with both ends at the component's minimum.
// No loop waits for a value that another lane has yet to write.  When all unions are done every tree's root is the one voxel whose
// link was never lowered, the minimum index of its component, whatever the order of the unions; the counts are integer sums and the
// winner an integer maximum.  Two runs give the same bits.
#include "label_runs.h"

namespace ctseg {

constexpr int CC_TX = 8, CC_TY = 16, CC_TZ = 32;                 // the tile: powers of two
constexpr int CC_TILE = CC_TX * CC_TY * CC_TZ;                   // 4096 voxels, 16 per lane
constexpr int CC_RUNS = CC_TZ / SD_RUN;                          // runs of a tile line
constexpr int CC_ROW = CC_TZ + 8;                                // bytes of an LDS line: voxel z at byte z + 4, zeros around
constexpr int CC_LAB_WORDS = (CC_TX + 2) * (CC_TY + 2) * CC_ROW / 4;
constexpr int CC_OFFSETS = 13;                                   // of the 26 neighbours, those before a voxel in raster order
static_assert(CC_TX * CC_TY * CC_RUNS == 256 && CC_TZ % SD_RUN == 0 && CC_ROW % 4 == 0, "one run per lane");
static_assert(CTSEG_COMPONENTS_KEEP_ROW_BYTES == 16, "the header's workspace size");

struct CcRow { unsigned long long key; int32_t count, removed; };   // of the keep's workspace, per sample and class 1..C-1
static_assert(sizeof(CcRow) == CTSEG_COMPONENTS_KEEP_ROW_BYTES, "the header's workspace size");

// backward offset k: (-1, *, *) for k < 9, (0, -1, *) for k < 12, (0, 0, -1)
__host__ __device__ __forceinline__ void cc_offset(int k, int& dx, int& dy, int& dz) {
  dx = k < 9 ? -1 : 0;
  dy = k < 9 ? k / 3 - 1 : (k < 12 ? -1 : 0);
  dz = k < 9 ? k % 3 - 1 : (k < 12 ? k - 10 : -1);
}

// bit k: offset k moves along active axes only, and along at most `connectivity` of them
static inline uint32_t cc_offset_mask(int connectivity, int axes) {
  uint32_t m = 0u;
  for (int k = 0; k < CC_OFFSETS; ++k) {
    int dx, dy, dz;
    cc_offset(k, dx, dy, dz);
    const bool active = (!dx || (axes & SD_AXIS_X)) && (!dy || (axes & SD_AXIS_Y)) && (!dz || (axes & SD_AXIS_Z));
    if (active && (dx != 0) + (dy != 0) + (dz != 0) <= connectivity) m |= 1u << k;
  }
  return m;
}

// SCOPE: __HIP_MEMORY_SCOPE_WORKGROUP on the LDS array, __HIP_MEMORY_SCOPE_AGENT on the global one.  (Termination: the head comment.)
template <int SCOPE> __device__ __forceinline__ int cc_find(const int* par, int v) {
  for (;;) {
    const int p = __hip_atomic_load(par + v, __ATOMIC_RELAXED, SCOPE);
    if (p == v) return v;
    v = p;
  }
}
template <int SCOPE> __device__ __forceinline__ void cc_union(int* par, int a, int b) {
  for (;;) {
    a = cc_find<SCOPE>(par, a);
    b = cc_find<SCOPE>(par, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }                  // the larger root goes under the smaller
    const int old = __hip_atomic_fetch_min(par + a, b, __ATOMIC_RELAXED, SCOPE);
    if (old == a) return;                                          // a was still a root: linked
    a = old;                                                       // a hangs under old < a since: unite that with b
  }
}

template <bool WIDE> __device__ __forceinline__ void store_run_i32(int32_t* p, const int (&v)[SD_RUN], int n) {
  if constexpr (WIDE) {
#pragma unroll
    for (int j = 0; j < 4; ++j) reinterpret_cast<i32x4*>(p)[j] = i32x4{v[4 * j], v[4 * j + 1], v[4 * j + 2], v[4 * j + 3]};
  } else {
#pragma unroll
    for (int i = 0; i < SD_RUN; ++i)
      if (i < n) p[i] = v[i];
  }
}

// Grid (tiles of a sample, B).  Lane: run (tid % 2) of tile line tid / 2.
template <bool WIDE>
__global__ __launch_bounds__(256) void components_local_kernel(const uint8_t* __restrict__ labels, int X, int Y, int Z, int C,
                                                               uint32_t offsets, int tyn, int tzn, int32_t* __restrict__ ids,
                                                               int32_t* __restrict__ sizes) {
  __shared__ uint32_t s_lab_w[CC_LAB_WORDS];
  __shared__ __attribute__((aligned(16))) int s_par[CC_TILE];                  // (16-byte stores of a run's links)
  __shared__ int s_cnt[CC_TILE];
  uint8_t* s_lab = reinterpret_cast<uint8_t*>(s_lab_w);
  const int tid = threadIdx.x;
  const TileOrigin o = tile_origin<CC_TX, CC_TY, CC_TZ>((int)blockIdx.x, (int)gridDim.x, tyn, tzn);
  for (int i = tid; i < CC_LAB_WORDS; i += 256) s_lab_w[i] = 0u;
  for (int i = tid; i < CC_TILE; i += 256) s_cnt[i] = 0;
  __syncthreads();
  const int line = tid / CC_RUNS, lx = line / CC_TY, ly = line % CC_TY, lz0 = (tid % CC_RUNS) * SD_RUN;
  const int x = o.x0 + lx, y = o.y0 + ly, z0 = o.z0 + lz0;
  const int n = (x < X && y < Y && z0 < Z) ? (Z - z0 < SD_RUN ? Z - z0 : SD_RUN) : 0;    // voxels of the run inside the volume
  const int64_t S = (int64_t)X * Y * Z;
  const int64_t at = (int64_t)blockIdx.y * S + ((int64_t)x * Y + y) * Z + z0;              // (read only where n > 0)
  const int li = line * CC_TZ + lz0;                                                       // the run's first voxel in the tile
  uint8_t* row = s_lab + ((lx + 1) * (CC_TY + 2) + ly + 1) * CC_ROW + 4 + lz0;
  u32x4 c = {0u, 0u, 0u, 0u};
  if (n > 0) {
    c = load_run<WIDE>(labels + at, n);
#pragma unroll
    for (int j = 0; j < 4; ++j) {                                    // a label >= C is in no component: 0 from here on
      uint32_t w = 0u;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const uint32_t v = (c[j] >> (t * 8)) & 255u;
        if (v < (uint32_t)C) w |= v << (t * 8);
      }
      c[j] = w;
      reinterpret_cast<uint32_t*>(row)[j] = w;
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) reinterpret_cast<i32x4*>(s_par + li)[j] = i32x4{li + 4 * j, li + 4 * j + 1, li + 4 * j + 2, li + 4 * j + 3};
  __syncthreads();
  const bool any = (c[0] | c[1] | c[2] | c[3]) != 0u;
  if (any) {
    for (int i = 0; i < SD_RUN; ++i) {
      const uint32_t v = row[i];
      if (v == 0u) continue;
      for (int k = 0; k < CC_OFFSETS; ++k) {
        if (!((offsets >> k) & 1u)) continue;
        int dx, dy, dz;
        cc_offset(k, dx, dy, dz);
        if (row[(dx * (CC_TY + 2) + dy) * CC_ROW + i + dz] == v)     // (a border byte is 0)
          cc_union<__HIP_MEMORY_SCOPE_WORKGROUP>(s_par, li + i, li + i + (dx * CC_TY + dy) * CC_TZ + dz);
      }
    }
  }
  __syncthreads();
  if (any) {
    for (int i = 0; i < SD_RUN; ++i)
      if (row[i])
        __hip_atomic_store(s_par + li + i, cc_find<__HIP_MEMORY_SCOPE_WORKGROUP>(s_par, li + i), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  __syncthreads();
  int word[SD_RUN];
  int cur = -1, cnt = 0;
#pragma unroll
  for (int i = 0; i < SD_RUN; ++i) {
    const int r = s_par[li + i];
    const bool in = run_byte(c, i) != 0u;
    const int rx = r / (CC_TY * CC_TZ), ry = (r / CC_TZ) % CC_TY, rz = r % CC_TZ;
    word[i] = in ? ((o.x0 + rx) * Y + o.y0 + ry) * Z + o.z0 + rz : -1;
    if (in) {
      if (r != cur) {
        if (cnt) atomicAdd(&s_cnt[cur], cnt);
        cur = r;
        cnt = 0;
      }
      ++cnt;
    }
  }
  if (cnt) atomicAdd(&s_cnt[cur], cnt);
  if (n > 0) store_run_i32<WIDE>(ids + at, word, n);
  __syncthreads();
#pragma unroll
  for (int i = 0; i < SD_RUN; ++i) word[i] = (run_byte(c, i) != 0u && s_par[li + i] == li + i) ? s_cnt[li + i] : 0;
  if (n > 0) store_run_i32<WIDE>(sizes + at, word, n);
}

// Grid (ceil(lines * runs / 256), B).  Lane: run k of line (x, y), as in the edge pass of the surface metrics.
template <bool WIDE>
__global__ __launch_bounds__(256) void components_merge_kernel(const uint8_t* __restrict__ labels, int X, int Y, int Z, int C,
                                                               uint32_t offsets, int runs, int32_t* __restrict__ ids) {
  const int64_t S = (int64_t)X * Y * Z;
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t line = g / runs;
  if (line >= (int64_t)X * Y) return;
  const int z0 = (int)(g - line * runs) * SD_RUN;
  const int x = (int)(line / Y), y = (int)(line - (int64_t)x * Y);
  const int n = Z - z0 < SD_RUN ? Z - z0 : SD_RUN;
  const int at = (int)(line * Z + z0);
  const uint8_t* L = labels + (int64_t)blockIdx.y * S;
  int32_t* par = ids + (int64_t)blockIdx.y * S;
  const u32x4 c = load_run<WIDE>(L + at, n);
  if ((c[0] | c[1] | c[2] | c[3]) == 0u) return;
  const int xt = x % CC_TX, yt = y % CC_TY;
  const bool xy_face = xt == 0 || xt == CC_TX - 1 || yt == 0 || yt == CC_TY - 1;
  for (int i = 0; i < n; ++i) {
    const uint32_t v = L[at + i];
    if (v == 0u || v >= (uint32_t)C) continue;
    const int z = z0 + i, zt = z % CC_TZ;
    if (!xy_face && zt != 0 && zt != CC_TZ - 1) continue;            // inside its tile: the local pass saw all its neighbours
    for (int k = 0; k < CC_OFFSETS; ++k) {
      if (!((offsets >> k) & 1u)) continue;
      int dx, dy, dz;
      cc_offset(k, dx, dy, dz);
      const int nx = x + dx, ny = y + dy, nz = z + dz;
      if (nx < 0 || ny < 0 || ny >= Y || nz < 0 || nz >= Z) continue;                       // (dx <= 0: nx < X)
      if (nx / CC_TX == x / CC_TX && ny / CC_TY == y / CC_TY && nz / CC_TZ == z / CC_TZ) continue;
      const int nat = (nx * Y + ny) * Z + nz;
      if (L[nat] == v) cc_union<__HIP_MEMORY_SCOPE_AGENT>(par, at + i, nat);
    }
  }
}

// Grid (ceil(S / 256), B).  Lane: one voxel.
__global__ __launch_bounds__(256) void components_flatten_kernel(int32_t* __restrict__ ids, int32_t* __restrict__ sizes, int S) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= S) return;
  int32_t* par = ids + (int64_t)blockIdx.y * S;
  int32_t* sz = sizes + (int64_t)blockIdx.y * S;
  const int p = __hip_atomic_load(par + v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (p < 0) return;
  const int r = cc_find<__HIP_MEMORY_SCOPE_AGENT>(par, p);
  if (r != p) __hip_atomic_store(par + v, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  // a count sits at a local root; only roots receive one, and v is none when r != v, so nobody adds to sz[v]
  const int n = sz[v];
  if (n > 0 && r != (int)v) {
    atomicAdd(sz + r, n);
    sz[v] = 0;
  }
}

__global__ __launch_bounds__(256) void components_zero_kernel(uint32_t* __restrict__ p, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) p[i] = 0u;
}

// Grid (ceil(S / CC_TILE), B): 16 voxels per lane, so that the classes' two global atomics come once per 4096 voxels (one per 256
// voxels made this launch the slowest of the seven on a map with thousands of small components).  A voxel with a count is a
// representative.
__global__ __launch_bounds__(256) void components_scan_kernel(const uint8_t* __restrict__ labels, const int32_t* __restrict__ sizes,
                                                              int S, int C, CcRow* __restrict__ rows) {
  __shared__ unsigned long long s_key[SD_MAX_CLASSES];
  __shared__ int s_n[SD_MAX_CLASSES];
  const int tid = threadIdx.x, b = blockIdx.y;
  if (tid < SD_MAX_CLASSES) { s_key[tid] = 0ull; s_n[tid] = 0; }
  __syncthreads();
  for (int j = 0; j < CC_TILE / 256; ++j) {
    const int64_t v = ((int64_t)blockIdx.x * (CC_TILE / 256) + j) * 256 + tid;
    if (v >= S) break;
    const int n = sizes[(int64_t)b * S + v];
    if (n > 0) {
      const uint32_t c = labels[(int64_t)b * S + v];
      if (c >= 1u && c < (uint32_t)C) {
        atomicAdd(&s_n[c], 1);
        atomicMax(&s_key[c], (unsigned long long)(uint32_t)n << 32 | (uint32_t)~(uint32_t)v);
      }
    }
  }
  __syncthreads();
  if (tid >= 1 && tid < C && s_n[tid]) {
    CcRow* r = rows + (int64_t)b * (C - 1) + tid - 1;
    atomicAdd(&r->count, s_n[tid]);
    atomicMax(&r->key, s_key[tid]);
  }
}

// Grid (ceil(ceil(S / 16) / 256), B).  Lane: 16 consecutive voxels of the sample.  WIDE: S is a multiple of 16.
template <bool WIDE>
__global__ __launch_bounds__(256) void components_apply_kernel(const uint8_t* __restrict__ labels, const int32_t* __restrict__ ids,
                                                               const int32_t* __restrict__ sizes, int S, int C, uint32_t class_mask,
                                                               int keep_largest, int min_size, CcRow* __restrict__ rows,
                                                               uint8_t* __restrict__ out) {
  __shared__ unsigned long long s_key[SD_MAX_CLASSES];
  __shared__ int s_gone[SD_MAX_CLASSES];
  const int tid = threadIdx.x, b = blockIdx.y;
  if (tid < SD_MAX_CLASSES) {
    s_key[tid] = (tid >= 1 && tid < C) ? rows[(int64_t)b * (C - 1) + tid - 1].key : 0ull;
    s_gone[tid] = 0;
  }
  __syncthreads();
  const int64_t v0 = ((int64_t)blockIdx.x * 256 + tid) * SD_RUN;
  if (v0 < S) {
    const int n = S - v0 < SD_RUN ? (int)(S - v0) : SD_RUN;
    const int64_t at = (int64_t)b * S + v0;
    const u32x4 c = load_run<WIDE>(labels + at, n);
    u32x4 o = c;
    if ((c[0] | c[1] | c[2] | c[3]) != 0u) {
#pragma unroll
      for (int i = 0; i < SD_RUN; ++i) {
        const uint32_t v = run_byte(c, i);
        if (i < n && v >= 1u && v < (uint32_t)C && ((class_mask >> v) & 1u)) {
          const int r = ids[at + i];
          bool keep = (uint32_t)r < (uint32_t)S;                     // (ids the label pass wrote always are)
          if (keep) {
            if (keep_largest) {
              const unsigned long long key = s_key[v];
              keep = (uint32_t)r == ~(uint32_t)key && (int)(key >> 32) >= min_size;
            } else if (min_size > 1) {
              keep = sizes[(int64_t)b * S + r] >= min_size;
            }
          }
          if (!keep) {
            o[i >> 2] &= ~(255u << ((i & 3) * 8));
            atomicAdd(&s_gone[v], 1);
          }
        }
      }
    }
    if constexpr (WIDE) {
      *reinterpret_cast<u32x4*>(out + at) = o;
    } else {
#pragma unroll
      for (int i = 0; i < SD_RUN; ++i)
        if (i < n) out[at + i] = (uint8_t)run_byte(o, i);
    }
  }
  __syncthreads();
  if (tid >= 1 && tid < C && s_gone[tid]) atomicAdd(&rows[(int64_t)b * (C - 1) + tid - 1].removed, s_gone[tid]);
}

// table[r] = {components, size of the largest, its representative (-1: none), voxels set to 0}
__global__ __launch_bounds__(256) void components_table_kernel(const CcRow* __restrict__ rows, int n, int32_t* __restrict__ table) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  const CcRow row = rows[r];
  table[r * 4 + 0] = row.count;
  table[r * 4 + 1] = (int32_t)(row.key >> 32);
  table[r * 4 + 2] = row.count > 0 ? (int32_t)~(uint32_t)row.key : -1;
  table[r * 4 + 3] = row.removed;
}

}  // namespace ctseg

using namespace ctseg;

extern "C" int ctseg_components_label(const uint8_t* labels, int32_t B, int32_t X, int32_t Y, int32_t Z, int32_t C,
                                      int32_t connectivity, int32_t axes, int32_t* ids, int32_t* sizes, void* stream) {
  CTSEG_REQUIRE(labels && ids && sizes, "components_label: null pointer (labels, ids and sizes are required)");
  if (check_components_dims("components_label", B, X, Y, Z, C)) return -1;
  CTSEG_REQUIRE(connectivity >= 1 && connectivity <= 3, "components_label: connectivity is 1, 2 or 3 (got %d)", connectivity);
  CTSEG_REQUIRE(axes >= 1 && axes <= 7, "components_label: axes is a mask of X = 1, Y = 2, Z = 4 (got %d)", axes);
  CTSEG_REQUIRE(((uintptr_t)ids % 4) == 0 && ((uintptr_t)sizes % 4) == 0, "components_label: unaligned pointer (ids, sizes)");
  const bool wide = Z % SD_RUN == 0;
  CTSEG_REQUIRE(!wide || (((uintptr_t)labels % 16) == 0 && ((uintptr_t)ids % 16) == 0 && ((uintptr_t)sizes % 16) == 0),
                "components_label: unaligned pointer (16 bytes for labels, ids and sizes when Z is a multiple of 16)");
  const uint32_t offsets = cc_offset_mask(connectivity, axes);
  const int txn = ilog_ceil_div(X, CC_TX), tyn = ilog_ceil_div(Y, CC_TY), tzn = ilog_ceil_div(Z, CC_TZ);
  const int runs = (Z + SD_RUN - 1) / SD_RUN;
  const int S = X * Y * Z;
  const dim3 tiles((unsigned)(txn * tyn * tzn), (unsigned)B), lanes((unsigned)(((int64_t)X * Y * runs + 255) / 256), (unsigned)B);
  hipStream_t st = (hipStream_t)stream;
  if (wide) {
    hipLaunchKernelGGL(components_local_kernel<true>, tiles, dim3(256), 0, st, labels, X, Y, Z, C, offsets, tyn, tzn, ids, sizes);
    CTSEG_LAUNCH_CHECK("components_label (local)");
    hipLaunchKernelGGL(components_merge_kernel<true>, lanes, dim3(256), 0, st, labels, X, Y, Z, C, offsets, runs, ids);
  } else {
    hipLaunchKernelGGL(components_local_kernel<false>, tiles, dim3(256), 0, st, labels, X, Y, Z, C, offsets, tyn, tzn, ids, sizes);
    CTSEG_LAUNCH_CHECK("components_label (local)");
    hipLaunchKernelGGL(components_merge_kernel<false>, lanes, dim3(256), 0, st, labels, X, Y, Z, C, offsets, runs, ids);
  }
  CTSEG_LAUNCH_CHECK("components_label (merge)");
  hipLaunchKernelGGL(components_flatten_kernel, dim3((unsigned)((S + 255) / 256), (unsigned)B), dim3(256), 0, st, ids, sizes, S);
  CTSEG_LAUNCH_CHECK("components_label (flatten)");
  return 0;
}

extern "C" int ctseg_components_keep(const uint8_t* labels, const int32_t* ids, const int32_t* sizes, int32_t B, int32_t X, int32_t Y,
                                     int32_t Z, int32_t C, int32_t class_mask, int32_t keep_largest, int32_t min_size,
                                     void* workspace, int64_t workspace_bytes, uint8_t* out, int32_t* table, void* stream) {
  CTSEG_REQUIRE(labels && ids && sizes && workspace && out && table,
                "components_keep: null pointer (labels, ids, sizes, workspace, out and table are required)");
  if (check_components_dims("components_keep", B, X, Y, Z, C)) return -1;
  CTSEG_REQUIRE(keep_largest == 0 || keep_largest == 1, "components_keep: keep_largest is 0 or 1 (got %d)", keep_largest);
  CTSEG_REQUIRE(min_size >= 0, "components_keep: min_size >= 0 (got %d)", min_size);
  CTSEG_REQUIRE(class_mask >= 0 && (class_mask & ~(((1 << C) - 1) & ~1)) == 0,
                "components_keep: class_mask has bits of the classes 1..%d only (got 0x%x)", C - 1, class_mask);
  const int rows = B * (C - 1);
  const int64_t need = (int64_t)rows * CTSEG_COMPONENTS_KEEP_ROW_BYTES;
  CTSEG_REQUIRE(workspace_bytes >= need, "components_keep: the workspace holds %lld bytes, %lld are needed", (long long)workspace_bytes,
                (long long)need);
  const int S = X * Y * Z;
  const bool wide = S % SD_RUN == 0;
  CTSEG_REQUIRE(((uintptr_t)workspace % 8) == 0 && ((uintptr_t)ids % 4) == 0 && ((uintptr_t)sizes % 4) == 0 &&
                    ((uintptr_t)table % 4) == 0 && (!wide || (((uintptr_t)labels % 16) == 0 && ((uintptr_t)out % 16) == 0)),
                "components_keep: unaligned pointer (8 bytes for the workspace, 16 for labels and out when X * Y * Z is a multiple "
                "of 16)");
  CcRow* ws = (CcRow*)workspace;
  hipStream_t st = (hipStream_t)stream;
  const int64_t words = need / 4;
  hipLaunchKernelGGL(components_zero_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, st, (uint32_t*)workspace, words);
  CTSEG_LAUNCH_CHECK("components_keep (zero)");
  hipLaunchKernelGGL(components_scan_kernel, dim3((unsigned)((S + CC_TILE - 1) / CC_TILE), (unsigned)B), dim3(256), 0, st, labels, sizes, S, C, ws);
  CTSEG_LAUNCH_CHECK("components_keep (scan)");
  const int64_t runs = ((int64_t)S + SD_RUN - 1) / SD_RUN;
  const dim3 grid((unsigned)((runs + 255) / 256), (unsigned)B);
  if (wide)
    hipLaunchKernelGGL(components_apply_kernel<true>, grid, dim3(256), 0, st, labels, ids, sizes, S, C, (uint32_t)class_mask,
                       keep_largest, min_size, ws, out);
  else
    hipLaunchKernelGGL(components_apply_kernel<false>, grid, dim3(256), 0, st, labels, ids, sizes, S, C, (uint32_t)class_mask,
                       keep_largest, min_size, ws, out);
  CTSEG_LAUNCH_CHECK("components_keep (apply)");
  hipLaunchKernelGGL(components_table_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, (const CcRow*)ws, rows, table);
  CTSEG_LAUNCH_CHECK("components_keep (table)");
  return 0;
}
