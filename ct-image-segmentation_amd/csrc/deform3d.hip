// Free-form deformation in the 3-D augmentation pass: a cubic B-spline over a coarse control lattice (Rueckert-style) is added to the
// sampling coordinate of ctseg_augment3d_to_hwd; from that coordinate on the pass is unchanged (resample3d_tile.h).  The rules are in
// include/ctseg_hip.h (ctseg_deform3d_lattice, ctseg_augment3d_deform_to_hwd).
//   lattice  one thread per control point: a counter hash of the seed (splitmix.h), scaled by the axis' magnitude.  No upload.
//   pass     the workgroup (one h) collapses the lattice's h axis once into an LDS slab of at most 12 x 20 rows per component; a
//            voxel then takes 16 taps per component from it, along w inside and along d outside: the rule's summation order.
// Every float operation is one float32 rounding: nothing may be contracted into an FMA.
#pragma clang fp contract(off)
#include "resample3d_tile.h"
#include "splitmix.h"

namespace ctseg {

struct LatticeArgs {
  int n[3];                          // Gd + 3, Gh + 3, Gw + 3
  float magnitude[3];
};

__global__ __launch_bounds__(256) void deform3d_lattice_kernel(uint64_t seed, const LatticeArgs a, float* __restrict__ lattice) {
  const int64_t per = (int64_t)a.n[0] * a.n[1] * a.n[2];
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= 3 * per) return;
  const int c = (int)(e / per);
  const int64_t rem = e - c * per;
  const int k = (int)(rem % a.n[2]), j = (int)((rem / a.n[2]) % a.n[1]), i = (int)(rem / ((int64_t)a.n[2] * a.n[1]));
  const double u = splitmix64_unit(seed, ((uint64_t)c << 60) | ((uint64_t)i << 40) | ((uint64_t)j << 20) | (uint64_t)k);
  const float m = c == 0 ? a.magnitude[0] : (c == 1 ? a.magnitude[1] : a.magnitude[2]);
  lattice[e] = (float)((2.0 * u - 1.0) * (double)m);
}

template <typename TI, int INTERP>
__global__ __launch_bounds__(256) void augment3d_deform_hwd_kernel(const TI* __restrict__ image, const uint8_t* __restrict__ masks,
                                                                   const Aug3dArgs p, const float* __restrict__ lattice,
                                                                   const Deform3dArgs dg, float* __restrict__ image_out,
                                                                   uint8_t* __restrict__ masks_out, uint8_t* __restrict__ labels_out,
                                                                   unsigned long long* __restrict__ hist) {
  resample3d_tile<Coord::LATTICE, TI, INTERP>(image, masks, p, image_out, masks_out, labels_out, hist, lattice, dg);
}

}  // namespace ctseg

using namespace ctseg;

extern "C" int ctseg_deform3d_lattice(int64_t seed, const int32_t* cells, const float* magnitude, float* lattice, int64_t lattice_elems,
                                      void* stream) {
  CTSEG_REQUIRE(cells && magnitude && lattice, "deform3d_lattice: null pointer");
  LatticeArgs a;
  int64_t elems = 3;
  for (int c = 0; c < 3; ++c) {
    CTSEG_REQUIRE(cells[c] >= 1 && (int64_t)cells[c] + 3 <= (1ll << 20), "deform3d_lattice: cells[%d] = %d is outside [1, 2^20 - 3]", c, cells[c]);
    CTSEG_REQUIRE(std::isfinite(magnitude[c]) && magnitude[c] >= 0.f, "deform3d_lattice: magnitude[%d] is negative or not finite", c);
    a.n[c] = cells[c] + 3, a.magnitude[c] = magnitude[c];
    elems *= a.n[c];               // at most 3 * 2^60
  }
  CTSEG_REQUIRE(lattice_elems == elems, "deform3d_lattice: lattice_elems %lld != 3 * prod(cells + 3) = %lld", (long long)lattice_elems, (long long)elems);
  CTSEG_REQUIRE((elems + 255) / 256 < (1ll << 31), "deform3d_lattice: the lattice is too large");
  hipLaunchKernelGGL(deform3d_lattice_kernel, dim3((unsigned)((elems + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (uint64_t)seed, a, lattice);
  CTSEG_LAUNCH_CHECK("deform3d_lattice");
  return 0;
}

extern "C" int ctseg_augment3d_deform_to_hwd(const void* image, int32_t image_dtype, const uint8_t* masks, int32_t K, int32_t D, int32_t H,
                                             int32_t W, int32_t Do, int32_t Ho, int32_t Wo, const float* matrix, int32_t interp,
                                             int32_t border, float cval, const int32_t* mask_src, int32_t window, float win_lo,
                                             float win_hi, float gain, float bias, float* image_out, uint8_t* masks_out,
                                             uint8_t* labels_out, int64_t* hist, const float* lattice, const int32_t* cells,
                                             void* stream) {
  Aug3dArgs p;
  dim3 grid;
  if (int rc = augment3d_prepare("augment3d_deform_to_hwd", image, image_dtype, masks, K, D, H, W, Do, Ho, Wo, matrix, interp, border,
                                 cval, mask_src, window, win_lo, win_hi, gain, bias, image_out, masks_out, labels_out, hist, p, grid))
    return rc;
  CTSEG_REQUIRE(lattice && cells, "augment3d_deform_to_hwd: lattice or cells is a null pointer");
  const int out[3] = {Do, Ho, Wo};
  // the slab holds the lattice rows of a 32 x 64 (d, w) tile: cells of at least 4 voxels along the tiled axes.  A workgroup has one h
  for (int a = 0; a < 3; ++a)
    CTSEG_REQUIRE(cells[a] >= 1 && (a == 1 ? 1 : 4) * (int64_t)cells[a] <= out[a],
                  "augment3d_deform_to_hwd: cells[%d] = %d: a cell has at least %d of the %d output voxels", a, cells[a], a == 1 ? 1 : 4, out[a]);
  Deform3dArgs dg;
  dg.Gd = cells[0], dg.Gh = cells[1], dg.Gw = cells[2];
  dg.gd = (float)cells[0] / (float)Do, dg.gh = (float)cells[1] / (float)Ho, dg.gw = (float)cells[2] / (float)Wo;
  with_pixel_and_interp(image_dtype, interp, [&](auto ti, auto ic) {
    using TI = decltype(ti);
    hipLaunchKernelGGL((augment3d_deform_hwd_kernel<TI, decltype(ic)::value>), grid, dim3(256), 0, (hipStream_t)stream, (const TI*)image,
                       masks, p, lattice, dg, image_out, masks_out, labels_out, (unsigned long long*)hist);
  });
  CTSEG_LAUNCH_CHECK("augment3d_deform_to_hwd");
  return 0;
}
