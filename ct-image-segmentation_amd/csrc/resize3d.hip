// 3-D input pipeline in one pass per instance: nearest Resize3D + (D,H,W)->(H,W,D) + optional window + optional
// squash.  The rules are in include/ctseg_hip.h (ctseg_resize3d_to_hwd).  The tile (one h, 64 along w, 32 along d; two phases
// through LDS) and the entry's validation are in resample3d_tile.h, which augment3d.hip and deform3d.hip share; this is its
// separable instantiation: no matrix, 64-bit offsets.  (The affine kernel under an identity matrix gives the same bits, slower:
// DESIGN.md §6.)
#pragma clang fp contract(off)
#include "resample3d_tile.h"

namespace ctseg {

template <typename TI>
__global__ __launch_bounds__(256) void resize3d_hwd_kernel(const TI* __restrict__ image, const uint8_t* __restrict__ masks, const Resize3dArgs p,
                                                           float* __restrict__ image_out, uint8_t* __restrict__ masks_out,
                                                           uint8_t* __restrict__ labels_out, unsigned long long* __restrict__ hist) {
  resample3d_tile<Coord::RESIZE, TI, 0>(image, masks, p, image_out, masks_out, labels_out, hist, nullptr, Deform3dArgs{});
}

}  // namespace ctseg

using namespace ctseg;

extern "C" int ctseg_resize3d_to_hwd(const void* image, int32_t image_dtype, const uint8_t* masks, int32_t K, int32_t D, int32_t H,
                                     int32_t W, int32_t Do, int32_t Ho, int32_t Wo, int32_t window, float win_lo, float win_hi,
                                     float* image_out, uint8_t* masks_out, uint8_t* labels_out, int64_t* hist, void* stream) {
  Resize3dArgs p;
  dim3 grid;
  if (int rc = resample3d_prepare("resize3d_to_hwd", false, image, image_dtype, masks, K, D, H, W, Do, Ho, Wo, window, win_lo, win_hi,
                                  image_out, masks_out, labels_out, hist, p, grid))
    return rc;
  with_raw_dtype(image_dtype, [&](auto ti) {
    using TI = decltype(ti);
    hipLaunchKernelGGL(resize3d_hwd_kernel<TI>, grid, dim3(256), 0, (hipStream_t)stream, (const TI*)image, masks, p, image_out, masks_out,
                       labels_out, (unsigned long long*)hist);
  });
  CTSEG_LAUNCH_CHECK("resize3d_to_hwd");
  return 0;
}
