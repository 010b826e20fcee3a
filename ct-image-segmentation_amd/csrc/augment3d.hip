// 3-D augmentation in the input pipeline's one pass per instance: the nearest Resize3D + (D,H,W)->(H,W,D) + window + squash of
// resize3d_hwd_kernel (loss_metric.hip), with the output voxel sent through a 3 x 4 affine matrix first, the mask channels through
// a permutation, and the windowed value through gain / bias.  The rules are in include/ctseg_hip.h (ctseg_augment3d_to_hwd).
// The tile (one h, 64 along w, 32 along d; two phases through LDS) and the entry's validation are in augment3d_tile.h, which
// deform3d.hip shares.  Every float operation is one float32 rounding: nothing may be contracted into an FMA.
#pragma clang fp contract(off)
#include "augment3d_tile.h"

namespace ctseg {

template <typename TI, int INTERP>
__global__ __launch_bounds__(256) void augment3d_hwd_kernel(const TI* __restrict__ image, const uint8_t* __restrict__ masks, const Aug3dArgs p,
                                                            float* __restrict__ image_out, uint8_t* __restrict__ masks_out,
                                                            uint8_t* __restrict__ labels_out, unsigned long long* __restrict__ hist) {
  augment3d_tile<TI, INTERP, false>(image, masks, p, image_out, masks_out, labels_out, hist, nullptr, Deform3dArgs{});
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
  hipStream_t st = (hipStream_t)stream;
#define CTSEG_AG_LAUNCH(TI)                                                                                                          \
  do {                                                                                                                               \
    if (interp)                                                                                                                      \
      hipLaunchKernelGGL((augment3d_hwd_kernel<TI, 1>), grid, dim3(256), 0, st, (const TI*)image, masks, p, image_out, masks_out, \
                         labels_out, (unsigned long long*)hist);                                                                     \
    else                                                                                                                             \
      hipLaunchKernelGGL((augment3d_hwd_kernel<TI, 0>), grid, dim3(256), 0, st, (const TI*)image, masks, p, image_out, masks_out, \
                         labels_out, (unsigned long long*)hist);                                                                     \
  } while (0)
  if (image_dtype == CTSEG_F32) CTSEG_AG_LAUNCH(float);
  else if (image_dtype == CTSEG_I16) CTSEG_AG_LAUNCH(short);
  else CTSEG_AG_LAUNCH(uint8_t);
#undef CTSEG_AG_LAUNCH
  CTSEG_LAUNCH_CHECK("augment3d_to_hwd");
  return 0;
}
