// 3-D augmentation in the input pipeline's one pass per instance: the nearest Resize3D + (D,H,W)->(H,W,D) + window + squash of
// ctseg_resize3d_to_hwd (resize3d.hip), with the output voxel sent through a 3 x 4 affine matrix first, the mask channels through
// a permutation, and the windowed value through gain / bias.  The rules are in include/ctseg_hip.h (ctseg_augment3d_to_hwd).
// The tile (one h, 64 along w, 32 along d; two phases through LDS) and the entry's validation are in resample3d_tile.h, which
// resize3d.hip and deform3d.hip share.  Every float operation is one float32 rounding: nothing may be contracted into an FMA.
#pragma clang fp contract(off)
#include "resample3d_tile.h"

namespace ctseg {

template <typename TI, int INTERP>
__global__ __launch_bounds__(256) void augment3d_hwd_kernel(const TI* __restrict__ image, const uint8_t* __restrict__ masks, const Aug3dArgs p,
                                                            float* __restrict__ image_out, uint8_t* __restrict__ masks_out,
                                                            uint8_t* __restrict__ labels_out, unsigned long long* __restrict__ hist) {
  resample3d_tile<Coord::AFFINE, TI, INTERP>(image, masks, p, image_out, masks_out, labels_out, hist, nullptr, Deform3dArgs{});
}

}  // namespace ctseg

using namespace ctseg;

extern "C" int ctseg_augment3d_to_hwd(const void* image, int32_t image_dtype, const uint8_t* masks, int32_t K, int32_t D, int32_t H,
                                      int32_t W, int32_t Do, int32_t Ho, int32_t Wo, const float* matrix, int32_t interp, int32_t border,
                                      float cval, const int32_t* mask_src, int32_t window, float win_lo, float win_hi, float gain,
                                      float bias, float* image_out, uint8_t* masks_out, uint8_t* labels_out, int64_t* hist,
                                      void* stream) {
  Aug3dArgs p;
  dim3 grid;
  if (int rc = augment3d_prepare("augment3d_to_hwd", image, image_dtype, masks, K, D, H, W, Do, Ho, Wo, matrix, interp, border, cval,
                                 mask_src, window, win_lo, win_hi, gain, bias, image_out, masks_out, labels_out, hist, p, grid))
    return rc;
  with_pixel_and_interp(image_dtype, interp, [&](auto ti, auto ic) {
    using TI = decltype(ti);
    hipLaunchKernelGGL((augment3d_hwd_kernel<TI, decltype(ic)::value>), grid, dim3(256), 0, (hipStream_t)stream, (const TI*)image, masks, p,
                       image_out, masks_out, labels_out, (unsigned long long*)hist);
  });
  CTSEG_LAUNCH_CHECK("augment3d_to_hwd");
  return 0;
}
