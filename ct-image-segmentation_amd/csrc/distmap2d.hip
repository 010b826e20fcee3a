// Distance maps of the 2-D pipeline on gfx950: capstone/data/utils.py:10-26 (compute_distance_map) for a whole batch of planes.
// The exact Euclidean distance transform in its separable form, in integers throughout, two launches:
//   columns  one lane per column of a plane sweeps down and then up: the vertical distance to the nearest foreground and to the
//            nearest background pixel of that column, two uint16 per pixel in the workspace (0xffff: the column has none)
//   rows     one workgroup per DM_ROWS rows of a plane, the two uint16 rows in LDS; one lane per output pixel takes
//            d2 = min over x' of (x - x')^2 + g[x']^2 for both transforms, searching outward from x until (x - x')^2 reaches the best
//            value so far, then forms the map value.
// A row in which every column holds the sentinel belongs to a plane without such a pixel (a column covers the plane's full height):
// its search is skipped and its squared distance is "none" (-1 in the d2 outputs).
// REFERENCE mode is the reference's own arithmetic: its result array is uint8, so what it stores is the byte
//   k = isqrt(d2_fg) & 255 outside, (1 - isqrt(d2_bg)) & 255 inside, 0 on a plane without foreground
// and the map is k / 255.0, here table[k] with the host's float32(k / 255.0).  SIGNED is the evidently intended float map.  A plane
// without any background pixel has no defined reference value (scipy's output there is an artefact): it is all zero in both modes.
#include "distmap_common.h"

namespace ctseg {

constexpr int DM_ROWS = 4;               // rows of a plane per workgroup of the row pass: 4 * 1024 * 4 B = 16 KiB of LDS at the most

// Lane (plane p, column x); the workspace holds fg | bg << 16 per pixel.  Both sweeps are coalesced across x.
__global__ __launch_bounds__(256) void distmap2d_columns_kernel(const uint8_t* __restrict__ masks, int P, int H, int W,
                                                                uint32_t* __restrict__ ws) {
  const int64_t col = (int64_t)blockIdx.x * 256 + threadIdx.x;      // columns of all planes, back to back
  if (col >= (int64_t)P * W) return;
  const int64_t p = col / W, x = col - p * W;
  const int64_t base = p * H * W + x;
  const uint8_t* m = masks + base;
  uint32_t* g = ws + base;
  int last_fg = -1, last_bg = -1;        // row of the nearest one above, -1: none yet
#pragma unroll 8
  for (int y = 0; y < H; ++y) {
    if (m[(int64_t)y * W] != 0) last_fg = y; else last_bg = y;
    const uint32_t dfg = last_fg < 0 ? DM_NONE : (uint32_t)(y - last_fg);
    const uint32_t dbg = last_bg < 0 ? DM_NONE : (uint32_t)(y - last_bg);
    g[(int64_t)y * W] = dfg | (dbg << 16);
  }
  int next_fg = -1, next_bg = -1;
#pragma unroll 8
  for (int y = H - 1; y >= 0; --y) {
    const uint32_t v = g[(int64_t)y * W];
    uint32_t dfg = v & 0xffffu, dbg = v >> 16;
    if (dfg == 0u) next_fg = y; else next_bg = y;              // a pixel is foreground exactly when its own distance is 0
    const uint32_t ufg = next_fg < 0 ? DM_NONE : (uint32_t)(next_fg - y);
    const uint32_t ubg = next_bg < 0 ? DM_NONE : (uint32_t)(next_bg - y);
    dfg = ufg < dfg ? ufg : dfg;                               // the sentinel is the largest value: min keeps "none" only for both
    dbg = ubg < dbg ? ubg : dbg;
    g[(int64_t)y * W] = dfg | (dbg << 16);
  }
}

// Workgroup b: rows [r0, r0 + DM_ROWS) of plane p.
__global__ __launch_bounds__(256) void distmap2d_rows_kernel(const uint32_t* __restrict__ ws, int P, int H, int W, int mode,
                                                             const float* __restrict__ table, float* __restrict__ out,
                                                             int* __restrict__ d2_fg, int* __restrict__ d2_bg) {
  __shared__ uint16_t s_fg[DM_ROWS][DM_MAX_SIDE];
  __shared__ uint16_t s_bg[DM_ROWS][DM_MAX_SIDE];
  __shared__ int s_any_fg, s_any_bg;
  const int groups = (H + DM_ROWS - 1) / DM_ROWS;
  const int p = blockIdx.x / groups, r0 = (blockIdx.x % groups) * DM_ROWS;
  if (p >= P) return;
  const int rows = H - r0 < DM_ROWS ? H - r0 : DM_ROWS;
  const int n = rows * W;                                      // the rows of one group are contiguous
  const int64_t base = ((int64_t)p * H + r0) * W;
  const int tid = threadIdx.x;
  if (tid == 0) { s_any_fg = 0; s_any_bg = 0; }
  __syncthreads();
  bool any_fg = false, any_bg = false;
  for (int i = tid; i < n; i += blockDim.x) {
    const uint32_t v = ws[base + i];
    const int r = i / W, x = i - r * W;
    s_fg[r][x] = (uint16_t)(v & 0xffffu);
    s_bg[r][x] = (uint16_t)(v >> 16);
    any_fg |= (v & 0xffffu) != DM_NONE;
    any_bg |= (v >> 16) != DM_NONE;
  }
  if (any_fg) s_any_fg = 1;                                    // (every writer stores the same value)
  if (any_bg) s_any_bg = 1;
  __syncthreads();
  const bool has_fg = s_any_fg != 0, has_bg = s_any_bg != 0;   // of the whole plane, see the head of this file
  for (int i = tid; i < n; i += blockDim.x) {
    const int r = i / W, x = i - r * W;
    const int dfg = has_fg ? envelope_min(CellsU16{}, s_fg[r], x, W, 1) : DM_INF;
    const int dbg = has_bg ? envelope_min(CellsU16{}, s_bg[r], x, W, 1) : DM_INF;
    if (d2_fg) d2_fg[base + i] = has_fg ? dfg : -1;
    if (d2_bg) d2_bg[base + i] = has_bg ? dbg : -1;
    float val = 0.f;
    if (has_fg && has_bg) {
      const bool inside = s_fg[r][x] == 0;
      if (mode == DM_REFERENCE) {
        const int k = inside ? (1 - isqrt(dbg)) & 255 : isqrt(dfg) & 255;
        val = table[k];
      } else {
        val = inside ? __fdiv_rn(-(root_f32(dbg) - 1.f), 255.f) : __fdiv_rn(root_f32(dfg), 255.f);
      }
    }
    out[base + i] = val;
  }
}

}  // namespace ctseg

using namespace ctseg;

extern "C" int ctseg_distmap2d_batch(const uint8_t* masks, int32_t P, int32_t H, int32_t W, int32_t mode, const float* table,
                                     void* workspace, int64_t workspace_bytes, float* out, int32_t* d2_fg, int32_t* d2_bg,
                                     void* stream) {
  CTSEG_REQUIRE(masks && table && workspace && out, "distmap2d_batch: null pointer (masks, table, workspace and out are required)");
  CTSEG_REQUIRE(P >= 1 && H >= 1 && W >= 1, "distmap2d_batch: P, H, W >= 1 (got %d planes of %d x %d)", P, H, W);
  CTSEG_REQUIRE(H <= DM_MAX_SIDE && W <= DM_MAX_SIDE, "distmap2d_batch: sides up to %d (got %d x %d)", DM_MAX_SIDE, H, W);
  CTSEG_REQUIRE(mode == DM_REFERENCE || mode == DM_SIGNED, "distmap2d_batch: mode %d", mode);
  const int64_t pixels = (int64_t)P * H * W;
  CTSEG_REQUIRE(workspace_bytes >= 4 * pixels, "distmap2d_batch: the workspace holds %lld bytes, %lld are needed",
                (long long)workspace_bytes, (long long)(4 * pixels));
  CTSEG_REQUIRE(((uintptr_t)workspace % 4) == 0 && ((uintptr_t)out % 4) == 0 && ((uintptr_t)table % 4) == 0 &&
                    ((uintptr_t)d2_fg % 4) == 0 && ((uintptr_t)d2_bg % 4) == 0,
                "distmap2d_batch: unaligned pointer");
  const int64_t col_blocks = ((int64_t)P * W + 255) / 256, row_blocks = (int64_t)P * ((H + DM_ROWS - 1) / DM_ROWS);
  CTSEG_REQUIRE(col_blocks <= 0x7fffffff && row_blocks <= 0x7fffffff, "distmap2d_batch: %d planes are too many for one launch", P);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(distmap2d_columns_kernel, dim3((unsigned)col_blocks), dim3(256), 0, st, masks, P, H, W, (uint32_t*)workspace);
  CTSEG_LAUNCH_CHECK("distmap2d_batch (columns)");
  hipLaunchKernelGGL(distmap2d_rows_kernel, dim3((unsigned)row_blocks), dim3(256), 0, st, (const uint32_t*)workspace, P, H, W, mode,
                     table, out, d2_fg, d2_bg);
  CTSEG_LAUNCH_CHECK("distmap2d_batch (rows)");
  return 0;
}
