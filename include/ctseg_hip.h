/*
 * ctseg_hip.h — C ABI of libctseg_hip.so: the MI355X (gfx950) kernels behind the reference's
 * 3-D U-Net training step.  Plain pointers and sizes only; no torch types.  Every pointer is a
 * DEVICE pointer unless a parameter says "host".  `stream` is a hipStream_t passed as void*.
 *
 * The reference (MrinalJain17/CT-image-segmentation) has no FFI of its own: its hot path is Python
 * calling torch/MONAI ops.  Each entry point below therefore names the reference call site (or the
 * torch/MONAI op that call site executes) it replaces; INTEGRATION.md shows the ctypes binding.
 *
 * Layout convention: activations are channels-last, [N][X][Y][Z][ld] with `ld` >= C elements per
 * voxel (X,Y,Z are the reference's (H,W,D) after ToTensorV3, capstone/volumetric/transforms.py:40;
 * 2-D tensors use Z = 1).  dtype: CTSEG_F32, CTSEG_BF16 or (forward passes) CTSEG_F16 storage, fp32 accumulation always.
 *
 * Return value: 0 on success, negative on a rejected argument or a HIP launch error
 * (ctseg_last_error() gives the text).  Nothing here allocates, frees or synchronises.
 */
#ifndef CTSEG_HIP_H
#define CTSEG_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI history.  1: round 1.  2: both descriptor structs start with `struct_size` (= sizeof of the struct the CALLER was compiled
 * against); every entry point that takes a descriptor rejects a size it does not know, so a caller built against an older header
 * can never make the library read past the end of its struct (round 2 appended fields to both structs under version 1).
 * 3: ctseg_conv_desc ends with the bst_* fields (backward InstanceNorm statistics taken in the epilogue of the pass that writes
 * the gradient); ctseg_conv_bwd_stats_slots(). */
#define CTSEG_ABI_VERSION 3
#define CTSEG_F32 0
#define CTSEG_BF16 1
#define CTSEG_I16 2 /* raw-input dtypes of ctseg_resize3d_to_hwd only */
#define CTSEG_U8 3
#define CTSEG_F16 4 /* IEEE half storage, fp32 accumulation: the FORWARD (inference) passes only — ctseg_conv_igemm,
                       ctseg_instnorm_prelu_fwd, ctseg_gather_cast, ctseg_nc_to_cl / cl_to_nc, ctseg_window_gather*;
                       the backward passes and the loss gradient reject it (train in CTSEG_BF16 or CTSEG_F32) */
#define CTSEG_MAX_TAPS 27
#define CTSEG_MAX_CLASSES 8

int ctseg_abi_version(void);
const char* ctseg_last_error(void);

/* One output-parity class of an implicit-GEMM convolution pass.  A plain convolution has one class;
 * a stride-2 transposed convolution (and the input-gradient of a stride-2 convolution) has 8. */
typedef struct ctseg_conv_class {
  int32_t ntaps;                 /* K = ntaps * Cg                                            */
  int32_t kpad;                  /* padded K of this class's weight rows (multiple of 128 B)    */
  int64_t w_off;                 /* element offset of this class's [rows][kpad] weight block    */
  int32_t ox, oy, oz;            /* written voxel = row * sout + (ox,oy,oz)                     */
  int32_t taps[CTSEG_MAX_TAPS];  /* packed offsets (dx&255)|(dy&255)<<8|(dz&255)<<16, int8 each */
} ctseg_conv_class;

/* Implicit-GEMM pass: out[row-voxel][n] = bias[n] + add[..][n] + sum_{tap,c} in[row*sin+d(tap)][c] * W[n][tap*Cg+c]
 * Replaces nn.Conv3d / nn.ConvTranspose3d forward and input-gradient inside monai UNet
 * (reference capstone/models/__init__.py:3, built at capstone/volumetric/base_trainer.py:65-72). */
typedef struct ctseg_conv_desc {
  int32_t struct_size;   /* sizeof(ctseg_conv_desc) of the caller's header: checked by every entry point (ABI 2)  */
  int32_t reserved0;     /* 0                                                                                     */
  const void* in;        /* gathered tensor [N][Xi][Yi][Zi][g_ld]                                */
  const void* w;         /* packed weights (ctseg_pack_weights), rows padded to a multiple of 128 */
  const float* bias;     /* [Cn] or NULL                                                         */
  void* out;             /* written tensor [N][Xo][Yo][Zo][o_ld]                                  */
  const void* add;       /* optional addend with out's voxel indexing, [..][add_ld]; may == out    */
  float* stats;          /* optional per-tile (sum, sumsq) partials [N][stats_tiles][2][stats_ld]  */
  int32_t dtype;         /* CTSEG_F32 / CTSEG_BF16: storage of in, w (and out/add unless *_f32)    */
  int32_t N, Xi, Yi, Zi; /* gathered tensor dims                                                  */
  int32_t Xr, Yr, Zr;    /* row grid per sample                                                   */
  int32_t Xo, Yo, Zo;    /* written tensor dims                                                   */
  int32_t Cg, Cn;        /* gathered channels per tap, GEMM columns                               */
  int32_t Cn_store;      /* channels actually stored per voxel (>= Cn, pad columns are zeros)      */
  int32_t g_ld, o_ld, add_ld;
  int32_t sin, sout;
  int32_t out_f32, add_f32;
  int32_t stats_ld, stats_tiles, stats_tile0; /* partial layout; this call fills tiles [tile0, tile0+tiles*nclass) */
  int32_t nclass;
  ctseg_conv_class cls[CTSEG_MAX_CLASSES];
  /* Optional split output (where ctseg_conv_split_ok() == 1): GEMM columns >= out2_col0 are written to `out2` (same voxel
   * indexing, channel stride o2_ld, column c at channel c - out2_col0) instead of `out` — two DENSE tensors instead of
   * two interleaved channel slices of one (the fused [residual | unit0] convolution of a down ResidualUnit, the
   * [skip | sub] gradient of a SkipConnection's torch.cat).  out2 == NULL: feature off. */
  void* out2;
  int32_t out2_col0, o2_ld;
  /* Optional InstanceNorm + PReLU applied to the GATHERED operand on its way into the pass (where ctseg_conv_in_norm_ok() == 1):
   * the pass multiplies prelu((in - mean[n][c]) * rstd[n][c]) instead of in, so the normalised activation of the producing layer
   * (reference: monai Convolution's ADN "NDA" = InstanceNorm3d -> Dropout(0) -> PReLU behind capstone/models/unet.py) is never
   * written to memory; an identity-residual addend (add == in) is the transformed value as well.
   * in_mean_rstd: fp32 [N][in_norm_C][2] (mean, 1/sqrt(var + eps)) as ctseg_instnorm_finalize writes it, in_alpha: the PReLU slope
   * (one value).  NULL: feature off. */
  const float* in_mean_rstd;
  const float* in_alpha;
  int32_t in_norm_C;
  /* Optional backward statistics of the InstanceNorm + PReLU whose OUTPUT GRADIENT this pass writes (where
   * ctseg_conv_bwd_stats_slots() > 0).  The written tensor is g = dL/d prelu(xhat), xhat = (y - mean) * rstd with y the forward
   * convolution output that norm normalised (autograd of monai Convolution's ADN, reached through loss.backward() at reference
   * capstone/volumetric/base_trainer.py:80-82).  Its backward needs, per (sample, channel), sum dxhat, sum dxhat * xhat
   * (dxhat = g * prelu'(xhat)) and sum g * min(xhat, 0) (the slope gradient) — what ctseg_instnorm_prelu_bwd_reduce computes in a
   * pass of its own over (g, y).  With bst_partials set, the epilogue of THIS pass reads the matching y tile and accumulates the
   * three sums of the values it stores (after the addend, rounded to the storage type), one partial row per workgroup (or tile)
   * and sample: bst_partials[n][p][3][bst_ld], p < bst_P — exactly ctseg_instnorm_prelu_bwd_finalize's input, so the reduce
   * pass and its second read of g disappear.  Columns [bst_col0, bst_col0 + bst_C) of the pass carry channels 0..bst_C-1 of the
   * norm (bst_col0 != 0: the norm sits behind the second half of a split output, bst_col0 == out2_col0).  bst_y is indexed like
   * the written tensor (same voxels), channel stride bst_y_ld, storage dtype of the pass.  The caller zero-fills bst_partials
   * once: a workgroup only writes the rows of samples it worked on.  bst_partials == NULL: feature off. */
  const void* bst_y;
  const float* bst_mean_rstd;  /* [N][bst_C][2] as ctseg_instnorm_finalize writes it */
  const float* bst_alpha;      /* the PReLU slope (one value)                        */
  float* bst_partials;
  int32_t bst_y_ld, bst_C, bst_col0, bst_P, bst_ld;
  int32_t reserved1;
} ctseg_conv_desc;

/* Rows of the row grid / output columns one workgroup tile covers for a pass with Cn columns. */
int ctseg_conv_tile_rows(int32_t Cn);
int ctseg_conv_tile_cols(int32_t Cn);
/* InstanceNorm partial tiles per sample (summed over classes) that a pass with this geometry fills: size `stats` with it */
int ctseg_conv_num_tiles(const ctseg_conv_desc* d);
/* 1 if a pass with this geometry can take out2 / out2_col0 / o2_ld (out2_col0 must be set; pointers are ignored) */
int ctseg_conv_split_ok(const ctseg_conv_desc* d);
/* Narrow rows.  A bf16 tensor of 9..12 channels (the reference's 10 classes) may be stored 12 elements wide (24-byte rows)
 * instead of 16: the tensors either side of the logits convolution are the largest the network moves, and a quarter of
 * their bytes is padding.  g_ld == 12 with Cg == 16 (channels 12..15 read as zero), o_ld == 12 with Cn_store == 12 and
 * add_ld == 12 are accepted where this returns 1: the resident-weight 3x3x3 LDS-halo pass (any of the three) and the
 * stride-2 transposed "up" pass (output / addend only).  The InstanceNorm, loss and layout entry points take such rows as
 * they are.  The host mirror asks before it lays a tensor out this way and falls back to 16-wide rows otherwise. */
int ctseg_conv_narrow_ok(const ctseg_conv_desc* d);
/* 1 if a pass with this geometry can take in_mean_rstd / in_alpha / in_norm_C (pointers are ignored): the x-column LDS-halo pass
 * over 12-wide 16-bit rows (whose operand is staged through registers), at most 16 samples and 12 normalised channels */
int ctseg_conv_in_norm_ok(const ctseg_conv_desc* d);
/* Partial rows per sample (bst_P) the pass with this geometry fills when bst_partials is set; 0: the pass cannot take the bst_*
 * fields (run ctseg_instnorm_prelu_bwd_reduce instead).  bst_y_ld, bst_C, bst_col0 must be set; pointers other than in / out /
 * out2 / add (which select the kernel) are ignored. */
int ctseg_conv_bwd_stats_slots(const ctseg_conv_desc* d);
/* Name of the kernel family the launch of this descriptor would run, in the order the library tries them: "x-column halo", "halo",
 * "up", "stem", "streamed-weight halo", "stride-2 halo", "stride-2 register-weight", "many-channel 8-class", or "generic" followed
 * by its tile ("generic 256x16", "generic 256x32", "generic 128x64", "generic 128x128", "generic 192x256", "generic ring 192x128",
 * "generic ring 192x256").  Host-only like the sizing queries above (pointers select the kernel by their alignment and by being set,
 * nothing is dereferenced); a static string, NULL for a descriptor the queries reject.  For tests and tools: a shape that an
 * eligibility change moved to another kernel is seen by name instead of silently testing something else. */
const char* ctseg_conv_pass_name(const ctseg_conv_desc* d);
int ctseg_conv_igemm(const ctseg_conv_desc* d, void* stream);

/* Weight gradient: R[tap*Cg+a][b] = sum_rows in[row*sin+d(tap)][a] * dy[row][b]; row K=ntaps*Cg of R is
 * sum_rows dy[row][b] (the bias gradient).  Written as `splits` fp32 slabs [N*splits][kpad_w][cn_pad]
 * into `ws`, then ctseg_conv_wgrad_reduce sums them in fixed order (deterministic) into torch layout.
 * `ws` need not be initialised: of each of the ctseg_conv_wgrad_slabs() slabs the pass writes every element the reduce reads
 * (rows [0, ntaps*Cg] x columns [0, roundup(Cn, 4)), pad channels, the bias row, an empty last split and the slabs of a capped
 * persistent grid included), so a recorded plan may replay over its own stale slabs (tests/test_gpu_wgrad.py poisons them).
 * Replaces autograd's conv weight/bias backward for the same modules as above. */
typedef struct ctseg_wgrad_desc {
  int32_t struct_size;   /* sizeof(ctseg_wgrad_desc) of the caller's header (ABI 2) */
  int32_t reserved0;
  const void* in;        /* gathered tensor [N][Xi][Yi][Zi][g_ld]  */
  const void* dy;        /* [N][rows][d_ld], rows = Xr*Yr*Zr        */
  float* ws;             /* slabs                                    */
  int32_t dtype;
  int32_t N, Xi, Yi, Zi, Xr, Yr, Zr;
  int32_t Cg, Cn, g_ld, d_ld, sin;
  int32_t ntaps;
  int32_t taps[CTSEG_MAX_TAPS];
  int32_t splits;        /* row ranges per sample                    */
  int32_t kpad_w, cn_pad; /* slab dims: kpad_w = roundup(ntaps*Cg+1,128), cn_pad = roundup(Cn, tile cols) */
  /* optional InstanceNorm + PReLU of the gathered operand, as ctseg_conv_desc's (where ctseg_wgrad_in_norm_ok() == 1) */
  const float* in_mean_rstd;
  const float* in_alpha;
  int32_t in_norm_C;
  /* dY formed on load (ABI 3, where ctseg_wgrad_dy_norm_ok() == 1; dyn_g == NULL: off).  Columns [dyn_col0, Cn) of dY are not read
   * from `dy` (which then holds columns [0, dyn_col0) only, d_ld >= dyn_col0) but computed from the gradient dyn_g behind the
   * InstanceNorm + PReLU of those columns and its forward input dyn_y — element for element what
   * ctseg_instnorm_prelu_bwd_apply(dyn_g, dyn_y, dyn_mean_rstd, dyn_alpha, dyn_sums) would have stored, bf16 rounding included.
   * For the FIRST layer of a network (no input gradient wanted) this removes the last norm-backward pass of the step and the copy
   * of the residual gradient into a fused [d_res | d_y0] operand
   * (reference: the first ResidualUnit of the MONAI UNet built at capstone/volumetric/base_trainer.py:65-72). */
  int32_t dyn_col0;
  const void* dyn_g;           /* [N][rows][dyn_g_ld], channel c <-> column dyn_col0 + c */
  const void* dyn_y;           /* [N][rows][dyn_y_ld] */
  int32_t dyn_g_ld, dyn_y_ld;
  const float* dyn_mean_rstd;  /* [N][Cn - dyn_col0][2] */
  const float* dyn_alpha;
  const float* dyn_sums;       /* [N][Cn - dyn_col0][2]: ctseg_instnorm_prelu_bwd_finalize's output */
} ctseg_wgrad_desc;

int ctseg_wgrad_tile_cols(int32_t Cn);
/* slabs this descriptor makes ctseg_conv_wgrad write (N*splits, or one per persistent workgroup of the LDS-halo
 * kernel that few-channel 3x3x3 stride-1 bf16 layers take): size `ws` and call the reduce with it. `ws`/`dy`/`in` may be NULL here */
int ctseg_conv_wgrad_slabs(const ctseg_wgrad_desc* d);
/* Workgroups ONE slab (one sample x one row range) of this pass takes, how many of them a CU holds at a time (`per_cu`) and the
 * operand bytes one workgroup stages per 32 rows (`stage_bytes`; either may be NULL), for the caller that picks `splits`: a
 * split-K pass costs (rounds of 256 * per_cu workgroups) x (32-row stages per workgroup) x (time of a stage: its staging
 * traffic at ~24 B/clk/CU) plus the fp32 slabs it writes and the reduce reads back.  0: the pass is a persistent
 * LDS-halo kernel that sizes its own grid (splits is ignored).  `splits`, `ws`, `in`, `dy` need not be set.  (The 512-thread ring
 * kernel of the many-channel bf16 layers holds ONE 256 x 256 / 256 x 128 / 512 x 64 tile per CU; the generic kernel four
 * 128 x 128 ones.) */
int ctseg_conv_wgrad_wgs_per_slab(const ctseg_wgrad_desc* d, int32_t* per_cu, int32_t* stage_bytes);
/* 1 when this weight-gradient pass may read 12-wide bf16 rows (g_ld == 12 with Cg == 16 and / or d_ld == 12): the LDS-halo kernel */
int ctseg_wgrad_narrow_ok(const ctseg_wgrad_desc* d);
/* 1 when this weight-gradient pass can normalise its gathered operand on the fly (the 16 -> <= 16 channel LDS-halo kernel) */
int ctseg_wgrad_in_norm_ok(const ctseg_wgrad_desc* d);
/* 1 when this weight-gradient pass can form the upper columns of dY on load (dyn_*): the single-channel stride-2 first layer */
int ctseg_wgrad_dy_norm_ok(const ctseg_wgrad_desc* d);
/* Name of the kernel the launch of this descriptor would run, precise to the instantiation: "x-column head GW/DW" and "head GW/DW"
 * (16 -> <= 16 channels; GW / DW = row widths 12 or 16 of `in` / `dy`; "head" when the taps are not in canonical order),
 * "halo 32x32" / "halo 32x64" / "halo 64x32" / "halo 64x64" (bytes per voxel of the gathered / dY LDS planes), "up 12" / "up 16",
 * "stem 16" .. "stem 64", "stem 32 dyn" / "stem 64 dyn", "ring 256x256" / "ring 256x128" / "ring 512x64", or "generic 16" ..
 * "generic 128" (column tile) with " element-wise" appended when the gathered operand is staged element by element.  Host-only like
 * the sizing queries (pointers select the kernel by their alignment and by being set, nothing is dereferenced); a static string,
 * NULL for a descriptor the queries reject and for dyn_g / in_mean_rstd on a pass that refuses them.  CTSEG_NO_WGRAD_UP and
 * CTSEG_WGRAD_RING=0 are honoured as the launch honours them. */
const char* ctseg_wgrad_pass_name(const ctseg_wgrad_desc* d);
int ctseg_conv_wgrad(const ctseg_wgrad_desc* d, void* stream);
/* dw[(b*A + a)*T + t] = sum_s ws[s][t*Astride + a][col0 + b]  for a < A, b < nb;
 * db[b] = sum_s ws[s][T*Astride][col0+b] (db may be NULL).  Astride = the pass's (padded) Cg. */
int ctseg_conv_wgrad_reduce(const float* ws, int32_t nslabs, int32_t kpad_w, int32_t cn_pad, int32_t A, int32_t Astride,
                            int32_t T, int32_t col0, int32_t nb, float* dw, float* db, void* stream);
/* The same reduction for SEVERAL weight-gradient passes in ONE launch: `jobs` is a device array of the arguments above (one entry
 * per ctseg_conv_wgrad_reduce call it replaces), results bit-identical to the per-pass calls (same partition of the slabs, same
 * fixed-order combine).  Replaces the 18 slab reduces of a training step (autograd's per-parameter gradient accumulation,
 * capstone/volumetric/base_trainer.py:80-82 -> loss.backward()) by one launch per gradient chunk: on the weight-gradient stream
 * every small launch between two GEMMs waits for the tail of the one before it.  block0 / lanes are filled by the caller:
 * lanes = 8 when nslabs >= 64 else 32 (float4 lanes along a slab row); blocks = ceil((T * Astride + 1) * ceil(nb / 4) / lanes);
 * block0 = running sum of the blocks of the jobs before it; total_blocks = the sum over all jobs.  Every job needs col0 % 4 == 0,
 * cn_pad % 4 == 0, col0 + roundup(nb, 4) <= cn_pad and a 16-byte aligned ws (ctseg_conv_wgrad_reduce_batch_ok). */
typedef struct ctseg_reduce_job {
  const float* ws;
  float* dw;
  float* db;                     /* may be NULL */
  int32_t nslabs, kpad_w, cn_pad, A, Astride, T, col0, nb;
  int32_t block0, lanes;
} ctseg_reduce_job;
int ctseg_conv_wgrad_reduce_batch_ok(const float* ws, int32_t cn_pad, int32_t col0, int32_t nb);
int ctseg_conv_wgrad_reduce_batch(const ctseg_reduce_job* jobs, int32_t n_jobs, int32_t total_blocks, void* stream);

/* dst[i] = (dtype) src[idx[i]], i < n.  With a host-built index this turns the flat fp32 parameter buffer
 * (torch Conv/ConvTranspose weight layouts) into every K-contiguous packed operand of the passes above in
 * ONE launch per optimizer step; pad entries point at a zero element of src. */
int ctseg_gather_cast(const float* src, const int32_t* idx, void* dst, int32_t dtype, int64_t n, void* stream);

/* The same re-layout, structured (ABI 3): one [rows][kpad] block of a packed operand is described instead of indexed element by
 * element.  Packed element (row n, K slot j * gs + g) of a block is the weight src[part.o + (n - part.n_lo) * part.SN +
 * (g - part.g_lo) * part.SG + tap[j]] of the part whose row / gathered-channel ranges hold (n, g), zero when no part does or
 * j >= ntaps.  A workgroup takes one row: it reads the row's source region in T-element runs (contiguous when SG == T) into LDS
 * and writes the K-contiguous row from there -- 25 MB written for ~40 MB read, where the index-driven gather reads 450 MB (every
 * gathered element sits in another cache line: consecutive K slots are T elements apart in torch's [out][in][taps] layout).
 * `rows` lists (block, row) pairs (device int32[2 * n_rows]); rows it does not list are never written (padding rows stay at the
 * zeros the caller initialised them with).  Device arrays; dtype = storage of dst (CTSEG_F32 / BF16 / F16). */
#define CTSEG_PACK_LDS_FLOATS 12288 /* sum over a block's parts of (g_hi - g_lo) * T must not exceed this (48 KB of LDS) */
typedef struct ctseg_pack_part {
  int64_t o;                     /* element offset of the weight tensor in src                          */
  int32_t n_lo, n_hi, g_lo, g_hi; /* rows / gathered channels this tensor supplies                       */
  int32_t SN, SG;                /* source strides (elements) of the row and of the gathered channel     */
} ctseg_pack_part;
typedef struct ctseg_pack_block {
  int64_t dst_off;               /* element offset of the block in dst                                   */
  int32_t kpad, gs, ntaps, T;    /* row pitch, gathered-channel stride, K slots in use = ntaps * gs, taps of the source weight */
  int32_t nparts, reserved;
  ctseg_pack_part part[2];
  int32_t tap[CTSEG_MAX_TAPS];   /* source tap id of K-slot group j                                      */
  int32_t reserved2;
} ctseg_pack_block;
int ctseg_pack_weights(const float* src, const ctseg_pack_block* blocks, int32_t n_blocks, const int32_t* rows, int32_t n_rows,
                       void* dst, int32_t dtype, void* stream);

/* InstanceNorm3d(affine=False, eps) + PReLU(1 scalar), as MONAI's Convolution block applies them
 * (SURVEY.md §3.2).  Statistics come from the conv pass's partials. */
/* partials [N][P][2][ld] fp32 -> mean_rstd [N][C][2] fp32 (biased variance, fp64 combine, fixed order) */
int ctseg_instnorm_finalize(const float* partials, int32_t N, int32_t P, int32_t ld, int32_t col0, int32_t C, double count,
                            double eps, double* scratch /* [N][64][2][ld] + N doubles; the tail zero-initialised once (completion counters) */,
                            float* mean_rstd, void* stream);
/* out = prelu((y-mean)*rstd, alpha) [+ res] ;  S = voxels per sample; mean_rstd NULL => identity norm/act skipped */
int ctseg_instnorm_prelu_fwd(int32_t dtype, const void* y, int32_t y_ld, const float* mean_rstd, const float* alpha,
                             const void* res, int32_t res_ld, void* out, int32_t out_ld, int32_t N, int64_t S, int32_t C,
                             void* stream);
/* backward, pass 1: partials [N][P][3][ld]: (sum dxhat, sum dxhat*xhat, sum g*xhat*[xhat<=0]) */
int ctseg_instnorm_prelu_bwd_reduce(int32_t dtype, const void* g, int32_t g_ld, const void* y, int32_t y_ld,
                                    const float* mean_rstd, const float* alpha, float* partials, int32_t P, int32_t ld,
                                    int32_t N, int64_t S, int32_t C, void* stream);
/* partials -> sums [N][C][2] (already divided by S) and dalpha (scalar, overwritten); scratch: N*C + 1 doubles, the last
 * one a zero-initialised completion counter (the block that finishes last sums the N*C slope terms in fixed order and
 * resets it: no extra launch).  dalpha == NULL: only the per-(n,c) slope terms are left in scratch (N*C doubles suffice)
 * and ctseg_instnorm_prelu_dalpha can sum them later. */
int ctseg_instnorm_prelu_bwd_finalize(const float* partials, int32_t N, int32_t P, int32_t ld, int32_t C, double S,
                                      double* scratch, float* sums, float* dalpha, void* stream);
int ctseg_instnorm_prelu_dalpha(const double* scratch, int32_t NC, float* dalpha, void* stream);
/* backward, pass 2: dy = rstd*(dxhat - s1 - xhat*s2); optionally also copies g to g_copy (fused residual hand-off).
 * da_part != NULL: one workgroup of the launch also writes dalpha = fixed-order sum of da_part[0 .. n_da) (the per-(n,c) slope
 * terms ctseg_instnorm_prelu_bwd_finalize left in its scratch) -- the PReLU slope gradient without a launch of its own. */
int ctseg_instnorm_prelu_bwd_apply(int32_t dtype, const void* g, int32_t g_ld, const void* y, int32_t y_ld,
                                   const float* mean_rstd, const float* alpha, const float* sums, void* dy, int32_t dy_ld,
                                   void* g_copy, int32_t g_copy_ld, int32_t N, int64_t S, int32_t C, const double* da_part,
                                   int32_t n_da, float* dalpha, void* stream);
/* Same pass, plus the column sums of dy over all N*S voxels -> colsum_out[C] (fp32): the bias gradient of the ConvTranspose3d
 * whose output this norm consumed (autograd: dOut.sum over voxels), without a second trip over dy.  colsum_partials: scratch of
 * P_cap rows x roundup(C, chunk) floats (P_cap >= N; a few thousand rows keep the whole chip busy); fixed-order sums. */
int ctseg_instnorm_prelu_bwd_apply_colsum(int32_t dtype, const void* g, int32_t g_ld, const void* y, int32_t y_ld,
                                          const float* mean_rstd, const float* alpha, const float* sums, void* dy, int32_t dy_ld,
                                          void* g_copy, int32_t g_copy_ld, int32_t N, int64_t S, int32_t C, float* colsum_partials,
                                          int32_t P_cap, float* colsum_out, const double* da_part, int32_t n_da, float* dalpha,
                                          void* stream);

/* out[c] = sum over rows of x[row][c] (bias gradient of nn.ConvTranspose3d); partials [P][roundup(C,chunk)] fp32 scratch */
int ctseg_colsum(int32_t dtype, const void* x, int32_t ld, int64_t rows, int32_t C, float* partials, int32_t P, float* out,
                 void* stream);

/* BatchNorm{2,3}d(affine=True, track_running_stats=True, eps, momentum) + PReLU(1 scalar), MONAI's Convolution block with
 * norm=Norm.BATCH.  Per-channel tables are the same for every sample: mean_rstd [C][2], scale_shift [C][2], sums [C][2].
 * Training forward: partials [N][P][2][ld] as for ctseg_instnorm_finalize, summed over samples AND rows (count = N*S) in fp64,
 * fixed order.  Writes mean_rstd (biased variance), scale_shift = (gamma*rstd, beta - mean*gamma*rstd), updates
 * running_mean / running_var in place ((1-m)*r + m*x, unbiased variance var*count/(count-1)) and adds 1 to *num_batches_tracked. */
int ctseg_batchnorm_finalize(const float* partials, int32_t N, int32_t P, int32_t ld, int32_t col0, int32_t C, double count,
                             double eps, double momentum, const float* gamma, const float* beta, float* running_mean,
                             float* running_var, int64_t* num_batches_tracked, float* mean_rstd, float* scale_shift, void* stream);
/* Eval forward: scale_shift = (gamma/sqrt(running_var+eps), beta - running_mean*gamma/sqrt(running_var+eps)). */
int ctseg_batchnorm_eval_table(const float* running_mean, const float* running_var, const float* gamma, const float* beta,
                               int32_t C, double eps, float* scale_shift, void* stream);
/* out = prelu(y*scale_c + shift_c, alpha) [+ res]; strides and dtypes as ctseg_instnorm_prelu_fwd (CTSEG_F16 accepted). */
int ctseg_scale_shift_prelu_fwd(int32_t dtype, const void* y, int32_t y_ld, const float* scale_shift, const float* alpha,
                                const void* res, int32_t res_ld, void* out, int32_t out_ld, int32_t N, int64_t S, int32_t C,
                                void* stream);
/* Training backward with z = gamma*xhat + beta, dz = g*prelu'(z).  Pass 1: partials [N][P][3][ld] =
 * (sum dz, sum dz*xhat, sum over z<=0 of g*z) per (sample, row range). */
int ctseg_batchnorm_prelu_bwd_reduce(int32_t dtype, const void* g, int32_t g_ld, const void* y, int32_t y_ld,
                                     const float* mean_rstd, const float* gamma, const float* beta, const float* alpha,
                                     float* partials, int32_t P, int32_t ld, int32_t N, int64_t S, int32_t C, void* stream);
/* Pass 2: dbeta[c] = sum dz, dgamma[c] = sum dz*xhat (overwritten), sums[c] = (dbeta/count, dgamma/count), da_part[c] = the
 * channel's slope-gradient term (C doubles). */
int ctseg_batchnorm_prelu_bwd_finalize(const float* partials, int32_t N, int32_t P, int32_t ld, int32_t C, double count,
                                       float* sums, float* dgamma, float* dbeta, double* da_part, void* stream);
/* Pass 3: dy = gamma*rstd*(dz - s1 - xhat*s2) [g copied to g_copy]; da_part != NULL: dalpha = fixed-order sum of da_part[0..n_da). */
int ctseg_batchnorm_prelu_bwd_apply(int32_t dtype, const void* g, int32_t g_ld, const void* y, int32_t y_ld,
                                    const float* mean_rstd, const float* gamma, const float* beta, const float* alpha,
                                    const float* sums, void* dy, int32_t dy_ld, void* g_copy, int32_t g_copy_ld, int32_t N,
                                    int64_t S, int32_t C, const double* da_part, int32_t n_da, float* dalpha, void* stream);

/* _squash_masks_3D (capstone/volumetric/utils.py:4-7): masks u8 [B][K][S] -> labels u8 [B][S]
 * (+ optional int64 copy) and per-sample class histogram hist[B][K+1] (int64, must be zeroed by the caller). */
int ctseg_squash_masks(const uint8_t* masks, int32_t B, int32_t K, int64_t S, uint8_t* labels, int64_t* labels_i64,
                       int64_t* hist, void* stream);
/* The same squash (same labels, int64 copy and histogram) plus, from the same read of the masks, present[B][K] (int32, zeroed by
 * the caller) = any(masks[b][k] == 1): the structure indicator of weighted_mixup (capstone/training/utils.py:27), taken per RAW
 * mask — a structure wholly covered by a higher-numbered one is missing from the squashed labels' histogram. */
int ctseg_squash_masks_present(const uint8_t* masks, int32_t B, int32_t K, int64_t S, uint8_t* labels, int64_t* labels_i64,
                               int64_t* hist, int32_t* present, void* stream);
/* mixup_tensors(x, x[perm], lambda) (capstone/training/utils.py:40,55-56) on fp32 rows [B][n]:
 *   out[b] = (float)lambda * x[b] + (float)(1 - lambda) * x[perm[b]]
 * with 1 - lambda formed in double and both products and the sum rounded separately (no FMA): bit-equal to the torch expression.
 * perm: int32 [B] on the device, entries outside [0, B) are clamped; out must not overlap x. */
int ctseg_mixup_images(const float* x, const int32_t* perm, int32_t B, int64_t n, double lambda, float* out, void* stream);

/* Fused loss / metric pass over channels-last fp32 logits [B][S][ld], C classes (C <= 16).
 * Replaces F.cross_entropy (capstone/models/losses.py:53,68), softmax->argmax (capstone/training/utils.py:19-20),
 * the one-hot + compute_meandice counts (capstone/models/temp.py:173-214) and the soft-Dice / focal sums of
 * monai DiceLoss / FocalLoss.  do_stats: per-workgroup partials part[B][P][2+3C] doubles
 *   (sum w*nll, sum w, then per class sum p, sum p*y, sum focal) and integer counts cnt[B][3][C]
 *   (|pred==c & true==c|, |pred==c|, |true==c|; int64, zeroed by the caller).
 * do_stats / do_grad = 2 select the cross-entropy-only fast path (soft sums left 0, gradient = ce term only).
 * do_grad: dlogits = coef-weighted gradient, coef[B][1+3C] fp32 = (ce_scale, a[C], b[C], f[C]):
 *   ce_scale*w[t]*(p-onehot) + softmax-jacobian of (a_c*y_c + b_c) + focal term f_t.  dlogits dtype = gdtype. */
int ctseg_seg_loss(const float* logits, int32_t ld, const uint8_t* labels, int32_t B, int64_t S, int32_t C,
                   const float* class_weight, int32_t do_stats, double* part, int32_t P, int64_t* cnt, int32_t do_grad,
                   const float* coef, void* dlogits, int32_t g_ld, int32_t gdtype, uint8_t* pred_out, void* stream);
/* ctseg_seg_loss's soft path against TWO targets of one prediction: side A of sample b is labels[b], side B is
 * labels[perm[b]] (perm int32 [B] on the device, clamped to [0, B); no gathered label map exists).  The mixup step
 * (capstone/training/mixup_trainer.py:63-81) calls its loss wrapper once per target; here the softmax is taken once per voxel.
 * do_grad = 0: part[B][P][2][2+3C] (each side laid out as ctseg_seg_loss's record: ctseg_reduce_partials_f64 with R = 2*(2+3C)
 *   reduces both) and cnt[B][2][3][C] (zeroed by the caller); sum p and |pred==c| are computed once and written to both sides.
 * do_grad = 1: dlogits = d_A + d_B, each term ctseg_seg_loss's gradient with coef[B][2][1+3C]; lambda is folded into coef by
 *   the caller.  class_weight: [2][C] (one row per side) or NULL.  Same dlogits row widths as ctseg_seg_loss. */
int ctseg_seg_loss_pair(const float* logits, int32_t ld, const uint8_t* labels, const int32_t* perm, int32_t B, int64_t S,
                        int32_t C, const float* class_weight, int32_t do_grad, double* part, int32_t P, int64_t* cnt,
                        const float* coef, void* dlogits, int32_t g_ld, int32_t gdtype, void* stream);
/* Boundary loss (capstone/models/losses.py:127-157): passes of their own over the same fp32 channels-last logits (the row rules of
 * ctseg_seg_loss) and the fp32 distance maps [B][C-1][S] (planar, contiguous, no background plane; any S).  perm: NULL, or int32 [B]
 * on the device (clamped to [0, B)): NS = 2 sides, side 1 of sample b reads the maps of sample perm[b] (the mixup step).
 * ctseg_boundary_stats: part[B][P][NS][C-1] doubles = per-workgroup sums over voxels of softmax(x)[c+1] * D_s[c]; the voxel ranges
 *   are ctseg_seg_loss's for the same P; ctseg_reduce_partials_f64 with R = NS*(C-1) finishes.  No atomics: deterministic.
 * ctseg_boundary_grad: bw[B][NS][C-1] fp32 = weight of (sample, side, class) in the differentiated scalar (1/S and the upstream
 *   gradient folded in by the caller); g_c = sum_s bw[b][s][c-1] * D_s[c-1], g_0 = 0, d_k = p_k (g_k - sum_j g_j p_j).
 *   accumulate = 0: dlogits rows = d, zeros in the pad columns.  accumulate = 1: rows += d (one fp32 add, one store), pad columns
 *   unchanged.  dlogits / g_ld / gdtype as in ctseg_seg_loss. */
int ctseg_boundary_stats(const float* logits, int32_t ld, const float* maps, const int32_t* perm, int32_t B, int64_t S, int32_t C,
                         double* part, int32_t P, void* stream);
int ctseg_boundary_grad(const float* logits, int32_t ld, const float* maps, const int32_t* perm, int32_t B, int64_t S, int32_t C,
                        const float* bw, int32_t P, void* dlogits, int32_t g_ld, int32_t gdtype, int32_t accumulate, void* stream);
/* The logits convolution of the U-Net's head with the cross-entropy of the training step fused into its epilogue: the fp32 logits
 * (1.2 GB per step at 2 x 512 x 512 x 48) are never written or re-read.  Replaces, for the native training step, the pair
 *   ctseg_conv_igemm(d) [monai UNet model.2.1.conv.unit0 + identity residual]  +  ctseg_seg_loss(do_stats = do_grad = 2)
 *   [F.cross_entropy, capstone/models/losses.py:45-68; softmax -> argmax + Dice counts, training/utils.py:19-20, models/metrics.py:15-21]
 * with the same per-voxel arithmetic: dlogits and cnt are bit-identical to the two-call path, the loss sums differ in summation
 * order only.  d: the recorded descriptor of that convolution (d->out is not written).  labels [N][S] u8; class_weight [C] or NULL;
 * coef[n * coef_stride] = d(loss)/d(weighted NLL sum of sample n); dlogits [N][S][g_ld] in d->dtype; part [N][P][R] doubles, this
 * launch writes slots 0 .. ctseg_conv_logits_ce_slots()-1 of every sample (entries 0 = weighted NLL sum, 1 = weight sum, rest 0);
 * cnt [N][3][C] += counts (zeroed by the caller).  ctseg_conv_logits_ce_slots: 0 when the pass is not eligible (the caller then
 * keeps the two-call path), else the number of partial slots per sample the launch fills. */
int ctseg_conv_logits_ce_slots(const ctseg_conv_desc* d, int32_t C);
int ctseg_conv_logits_ce(const ctseg_conv_desc* d, const uint8_t* labels, int32_t C, const float* class_weight, const float* coef,
                         int32_t coef_stride, void* dlogits, int32_t g_ld, double* part, int32_t P, int32_t R, int64_t* cnt,
                         void* stream);
/* cnt[B][3][C] += (|pred==c & true==c|, |pred==c|, |true==c|) from two u8 label maps [B][S]
 * (DiceMetricWrapper on squashed predictions, capstone/models/metrics.py:15-31); cnt zeroed by the caller. */
int ctseg_dice_counts(const uint8_t* pred, const uint8_t* truth, int32_t B, int64_t S, int32_t C, int64_t* cnt, void* stream);
/* part [B][P][R] doubles -> out [B][R] doubles, fixed order */
int ctseg_reduce_partials_f64(const double* part, int32_t B, int32_t P, int32_t R, double* out, void* stream);
/* One launch for the scalars a cross-entropy training step logs (capstone/volumetric/base_trainer.py:80-82, 98-110 ->
 * capstone/models/losses.py:45-68 and metrics.py:15-31): out[0] = sum_b red[b][0] / sum_b red[b][1] with red = the reduced
 * ctseg_seg_loss records (entry 0 = weighted NLL sum, 1 = weight sum); out[2 + k] = Dice of class k+1 averaged over the
 * samples whose truth holds it (0 if none), from cnt[B][3][C]; out[1] = mean of those C-1 values.  out: 1 + C floats. */
int ctseg_loss_dice_summary(const double* red, int32_t B, int32_t R, const int64_t* cnt, int32_t C, float* out, void* stream);

/* torch.optim.Adam step (capstone/volumetric/base_trainer.py:113-114) on flat fp32 buffers.  lr / betas / eps are doubles (ABI 3),
 * as the Python floats torch receives: 1 - beta2 is formed in double and THEN rounded (0.001f; 1.f - 0.999f is 1.3e-5 off). */
int ctseg_adam_step(float* p, const float* g, float* m, float* v, int64_t n, double lr, double beta1, double beta2, double eps,
                    int32_t step, float grad_scale, void* stream);

/* x[0..n) *= host_scale * (dev_scale ? *dev_scale : 1), in place; a launch whose factor is exactly 1 touches no memory.
 * Two users: the upstream gradient autograd hands ``loss.backward()`` (capstone/volumetric/base_trainer.py:80-82 returns the
 * loss; Lightning / AMP may scale it) applied to the d loss / d logits the fused loss pass wrote for an upstream gradient of 1,
 * and the 1 / world of the data-parallel gradient MEAN applied to the all-reduced flat gradient on the drop-in path.
 * dtype: CTSEG_F32 or CTSEG_BF16. */
int ctseg_scale_inplace(void* x, int32_t dtype, int64_t n, const float* dev_scale, float host_scale, void* stream);

/* Layout / dtype plumbing. */
int ctseg_cast(const void* src, int32_t src_dtype, void* dst, int32_t dst_dtype, int64_t n, void* stream);
/* fp32 [N][C][S] (torch NC*) -> dtype [N][S][ld] channels-last (pad channels zeroed) and back (fp32 out) */
int ctseg_nc_to_cl(const float* src, void* dst, int32_t dtype, int32_t N, int32_t C, int64_t S, int32_t ld, void* stream);
int ctseg_cl_to_nc(const void* src, int32_t dtype, float* dst, int32_t N, int32_t C, int64_t S, int32_t ld, void* stream);

/* 3-D input pipeline on the device: one pass per instance replaces
 *   Resize3D.apply / apply_to_mask   capstone/volumetric/transforms.py:14-22  (F.interpolate, mode "nearest":
 *                                    src = min((int)floorf(dst * ((float)in / out)), in - 1) per axis)
 *   ToTensorV3.apply / apply_to_mask capstone/volumetric/transforms.py:39-43  ((C,D,H,W) -> (C,H,W,D))
 *   optionally _squash_masks_3D      capstone/volumetric/utils.py:4-7         (labels_out, + per-class voxel counts in hist[K+1],
 *                                    which the caller zeroes) and the HU window of capstone/transforms/transforms_2d.py:97-107
 *                                    (window 0: none, 1: clip to [lo,hi], 2: clip and map to [0,1]; the 3-D reference path has none).
 * image [D][H][W] of image_dtype (CTSEG_F32 / CTSEG_I16 / CTSEG_U8) -> image_out fp32 [Ho][Wo][Do];
 * masks [K][D][H][W] u8 -> masks_out [K][Ho][Wo][Do] and/or labels_out [Ho][Wo][Do].  image or masks may be NULL. */
int ctseg_resize3d_to_hwd(const void* image, int32_t image_dtype, const uint8_t* masks, int32_t K, int32_t D, int32_t H, int32_t W,
                          int32_t Do, int32_t Ho, int32_t Wo, int32_t window, float win_lo, float win_hi, float* image_out,
                          uint8_t* masks_out, uint8_t* labels_out, int64_t* hist, void* stream);

/* 3-D augmentation in that same pass: an affine resample, a permutation of the mask channels and an intensity gain / bias.  Inputs,
 * outputs, dtypes (CTSEG_F32 / CTSEG_I16 / CTSEG_U8), layouts and the K <= 15 limit are those of ctseg_resize3d_to_hwd; each
 * volume (D * H * W, Do * Ho * Wo) has fewer than 2^31 voxels.  matrix (12 floats, row-major 3 x 4; rows and columns ordered
 * d, h, w) and mask_src (K ints, or NULL for the identity) are HOST arrays copied into the kernel's arguments: no device upload, no
 * synchronisation.  Rejected: a matrix entry that is not finite (or a row that sends the output grid beyond 1e30), a mask_src that
 * is no permutation of 0..K-1, interp or border out of range, a cval, gain or bias that is not finite.
 * Every float operation is one float32 rounding; nothing is contracted into an FMA.
 *   - The augmentation acts on the VIRTUAL RESIZED VOLUME V of size Do x Ho x Wo: V[r] = src[rz(r_d), rz(r_h), rz(r_w)], rz the
 *     nearest rule above, min((int)floorf(r * ((float)in / out)), in - 1).  V is never stored.
 *   - For output voxel o = (od, oh, ow), taken as floats, the sampling coordinate is
 *     q_a = ((A[a][0]*od + A[a][1]*oh) + A[a][2]*ow) + A[a][3], evaluated in that order.
 *   - Nearest (interp 0): r_a = (int)floorf(q_a + 0.5f).  border 0 (constant): any r_a outside [0, out_a) gives cval for the image
 *     and 0 for the masks.  border 1 (edge): r_a is clamped to the volume.
 *   - Trilinear (interp 1), image only: b_a = floorf(q_a), f_a = q_a - b_a.  The eight corners V[b + {0,1}^3] are fetched by the
 *     same in/out rule: a corner outside gives cval, or the clamped voxel with border 1.  They are combined as
 *     lerp(x, y, t) = x + t * (y - x), along w first, then h, then d.
 *   - Image value: sample, then the window (the arithmetic of ctseg_resize3d_to_hwd, unchanged), then v * gain + bias; that last
 *     step is skipped altogether when gain == 1 && bias == 0.
 *   - Masks are always nearest: output channel k is the nearest sample of input channel mask_src[k].  labels = max_k(m_k * (k + 1))
 *     and hist (which the caller zeroes) are taken over the OUTPUT channels, as in the resize kernel.
 * The identity matrix reproduces ctseg_resize3d_to_hwd bit for bit with either interp (all weights are exactly 0 and
 * x + 0 * (y - x) = x); integer flip and quarter-turn matrices reproduce the flipped / turned resize. */
int ctseg_augment3d_to_hwd(const void* image, int32_t image_dtype, const uint8_t* masks, int32_t K, int32_t D, int32_t H, int32_t W,
                           int32_t Do, int32_t Ho, int32_t Wo, const float* matrix /* host */, int32_t interp, int32_t border,
                           float cval, const int32_t* mask_src /* host */, int32_t window, float win_lo, float win_hi, float gain,
                           float bias, float* image_out, uint8_t* masks_out, uint8_t* labels_out, int64_t* hist, void* stream);

/* Free-form deformation of that pass: a cubic B-spline over a coarse control lattice (Rueckert et al. 1999) is added to the
 * sampling coordinate.  The lattice is made on the device from a seed: no upload, no synchronisation.  Every float operation below
 * is one float32 rounding (double where it says so); nothing is contracted into an FMA.
 *
 * ctseg_deform3d_lattice fills lattice, DEVICE fp32 [3][Gd+3][Gh+3][Gw+3] (component c = 0: d, 1: h, 2: w displacement, in output
 * voxels), for cells = (Gd, Gh, Gw) and magnitude[3], both HOST arrays:
 *   lattice[c][i][j][k] = (float)((2 u - 1) * (double)magnitude[c]), u = (z >> 11) * 2^-53 in double, z the splitmix64 mix
 *   (z ^= z >> 30, z *= 0xBF58476D1CE4E5B9, z ^= z >> 27, z *= 0x94D049BB133111EB, z ^= z >> 31) of
 *   seed + (((c << 60) | (i << 40) | (j << 20) | k) + 1) * 0x9E3779B97F4A7C15, all in uint64.
 * Rejected: G_a < 1, G_a + 3 > 2^20, a magnitude that is negative or not finite, lattice_elems != 3 * prod(G_a + 3). */
int ctseg_deform3d_lattice(int64_t seed, const int32_t* cells /* host, 3 */, const float* magnitude /* host, 3 */, float* lattice,
                           int64_t lattice_elems, void* stream);

/* ctseg_augment3d_to_hwd with that lattice (DEVICE) over cells = (Gd, Gh, Gw) (HOST) cells of the OUTPUT grid.  Inputs, outputs,
 * limits and rules are those of ctseg_augment3d_to_hwd; rejected in addition: lattice or cells NULL, G_a < 1, 4 * G_a > out_a
 * along d and w (a cell is at least 4 output voxels along the axes the kernel tiles, which bounds the lattice rows a tile touches),
 * G_h > out_h.
 *   - Per axis a of output voxel o = (od, oh, ow): g_a = (float)G_a / (float)out_a (formed on the host), u_a = (float)o_a * g_a,
 *     i_a = min((int)floorf(u_a), G_a - 1), t_a = u_a - (float)i_a and, with s = 1 - t, the weights
 *       B0 = ((s*s)*s) / 6,  B1 = ((((3*t - 6)*t)*t) + 4) / 6,  B2 = (((((-3*t + 3)*t) + 3)*t) + 1) / 6,  B3 = ((t*t)*t) / 6.
 *   - Displacement, component c:
 *       s_c = sum_{a=0..3} Bd[a] * ( sum_{b=0..3} Bw[b] * ( sum_{e=0..3} Bh[e] * lattice[c][id+a][ih+e][iw+b] ) ),
 *     each sum starting from its first product and adding left to right.  h is innermost: a workgroup of the kernel has one h and
 *     collapses that axis once for all its voxels.
 *   - Sampling coordinate: q_a = (((A[a][0]*od + A[a][1]*oh) + A[a][2]*ow) + A[a][3]) + s_a.  From q on everything is
 *     ctseg_augment3d_to_hwd: nearest and trilinear rules, border, window, gain / bias, masks, labels, hist.
 * An all-zero lattice reproduces ctseg_augment3d_to_hwd bit for bit (q + 0 = q). */
int ctseg_augment3d_deform_to_hwd(const void* image, int32_t image_dtype, const uint8_t* masks, int32_t K, int32_t D, int32_t H,
                                  int32_t W, int32_t Do, int32_t Ho, int32_t Wo, const float* matrix /* host */, int32_t interp,
                                  int32_t border, float cval, const int32_t* mask_src /* host */, int32_t window, float win_lo,
                                  float win_hi, float gain, float bias, float* image_out, uint8_t* masks_out, uint8_t* labels_out,
                                  int64_t* hist, const float* lattice, const int32_t* cells /* host, 3 */, void* stream);

/* Intensity stage of that pipeline: Gaussian blur, additive Gaussian noise and a gamma curve on the fp32 image [Ho][Wo][Do] that the
 * passes above write, applied in this fixed order: blur, then noise, then gamma; any of the three may be absent.  image and image_out
 * may be the same buffer (every pass can run in place: a workgroup reads nothing but the lines it owns) and there is no scratch
 * volume; otherwise image is left untouched.  Sides are in [1, 1024].  radius (3 ints) and taps (3 rows of 13 floats, row a holding
 * w_0..w_radius[a]; may be NULL when every radius is 0) are HOST arrays ordered d, h, w and copied into the kernels' arguments: no
 * device upload, no synchronisation.  Every float operation below is one float32 rounding; nothing is contracted into an FMA.
 *   - Blur: separable, one pass per axis with radius[a] > 0, in the order d (the contiguous axis), w, h; each pass stores float32.
 *     The caller forms r = ceil(3 sigma) and w_k = exp(-k^2 / (2 sigma^2)), k = 0..r, normalised so that w_0 + 2 sum_{k>=1} w_k = 1,
 *     in float64 and rounds once; 0 < sigma <= 4, so r <= 12; radius 0 skips the axis with no launch.  Border: edge replication,
 *     indices clamped to [0, n - 1]; r may exceed n.  Along an axis with values v[]:
 *         acc = w_0 * v[i];    for k = 1..r:  acc = acc + w_k * (v[max(i-k, 0)] + v[min(i+k, n-1)])
 *     where the pair's sum, its product with w_k and the sum into acc are three separate roundings (a rounded multiply and a
 *     rounded add, NOT a fused multiply-add).
 *   - Noise (noise_std > 0): v = v + noise_std * n(seed, i), i = (h * Wo + w) * Do + d, the voxel's linear index in storage:
 *         z = splitmix64 mix (see ctseg_deform3d_lattice) of noise_seed + (i + 1) * 0x9E3779B97F4A7C15, in uint64,
 *         u1 = ((z >> 40) + 1) * 2^-24 in (0, 1],   u2 = ((z >> 16) & 0xFFFFFF) * 2^-24 in [0, 1)   (both exact in float32),
 *         n = sqrtf(-2 * logf(u1)) * cosf(6.2831855f * u2).
 *     Stateless: the seed and the index fix the field, whatever the volume's shape.  It is added after the blur.
 *   - Gamma (has_range = 1, over the value range (lo, hi)): t = min(max((v - lo) * inv, 0), 1), v = lo + (hi - lo) * powf(t, gamma),
 *     with inv = (float)(1 / ((double)hi - (double)lo)) and the float32 hi - lo formed on the host; gamma in [0.25, 4].  Values
 *     outside the range, such as those the noise pushed out, are CLAMPED by this step (gamma = 1 is a clamp to the range).
 *   - Launches (ctseg_intensity3d_launches returns their number for the same arguments, or a negative value where the entry
 *     refuses them; it touches no device): one per blurred axis, the point stage (noise, gamma) folded into the store of the last
 *     of them; one launch for a point stage alone; none when there is nothing to do (image_out, if another buffer, then gets the
 *     input's bits by an asynchronous copy).
 * Rejected before any launch: a null image or image_out (or taps, with a radius > 0); a side outside [1, 1024]; a radius outside
 * [0, 12]; a tap that is negative or not finite, or taps whose w_0 + 2 sum w_k differs from 1 by more than (r + 2) * 2^-24; a
 * noise_std that is negative or not finite; has_range other than 0 / 1; gamma outside [0.25, 4], or other than 1 without a range;
 * a range that is not finite or has lo >= hi. */
int ctseg_intensity3d(const float* image, float* image_out, int32_t Do, int32_t Ho, int32_t Wo, const int32_t* radius /* host, 3 */,
                      const float* taps /* host, 3 x 13 */, float noise_std, int64_t noise_seed, int32_t has_range, float lo, float hi,
                      float gamma, void* stream);
int ctseg_intensity3d_launches(const int32_t* radius /* host, 3 */, float noise_std, int32_t has_range, float gamma);

/* Foreground-biased patch sampling for training at native resolution (MONAI's RandCropByPosNegLabel, nnU-Net's foreground
 * oversampling): ctseg_patch_centres picks P patch centres on the device, most of them on a voxel of a structure drawn with equal
 * chance per class, and ctseg_patch3d_to_hwd crops (or resamples) a patch around a centre that only the device knows.
 *
 * ctseg_patch_centres.  masks is the raw [K][D][H][W] u8 block (DEVICE); a voxel is set where its byte is nonzero; structures may
 * overlap.  Limits: 1 <= K <= 15, 1 <= P <= 16, D * H * W < 2^31.  draws (HOST, P x 3 uint32: fg, a, b per patch) and patch (HOST,
 * 3 ints ordered d, h, w, or NULL) are copied into the kernel's arguments: no upload, no synchronisation.  Everything is integer
 * arithmetic; there is no float operation and no host round trip.
 *   - n_k is the number of set voxels of mask k.
 *   - The eligible classes are those with bit k set in class_mask and n_k > 0, in ascending k; m is their number.
 *   - If fg != 0 and m > 0: class = eligible[(uint64)a * m >> 32], rank r = (uint64)b * n_class >> 32, and the centre is the r-th
 *     set voxel of that mask in raster (d, h, w) order (r = 0 is the first).
 *   - Otherwise class = -1 and the centre is voxel (uint64)b * (D * H * W) >> 32 of the volume, in raster order.
 *   - Clamp, applied when patch is given: along each axis a with dim_a >= patch_a, c_a is clamped into
 *     [patch_a / 2, dim_a - (patch_a - patch_a / 2)] (integer division); along an axis with dim_a < patch_a, c_a = dim_a / 2.
 *     A patch that starts at c_a - patch_a / 2 then lies inside the volume wherever the volume is large enough.
 *   - centres (DEVICE, P x 4 int32): centres[p] = (d, h, w, class).
 * Two launches.  The count pass reads every mask byte once with 16-byte loads and writes one int32 count per (class, block of 16384
 * voxels) to the workspace; the select pass, one workgroup per patch, sums each class's counts in a fixed order (the K totals,
 * which it also stores behind the counts: workspace word K * nb + k, nb = ceil(D * H * W / 16384)), finds the block by a prefix
 * scan over the class's counts and the voxel inside it by per-lane byte counts and a second scan.  Every workspace word that is
 * read has been written by the count pass of the same call, so the workspace may arrive with any content, and nothing is summed
 * by atomics: two runs give the same bits.
 * ctseg_patch_centres_workspace returns the bytes needed, 4 * (K * ceil(D * H * W / 16384) + 16), or a negative value where the
 * entry refuses the geometry; it touches no device.
 * Rejected before any launch: a null masks, draws, workspace or centres; P outside [1, 16]; K outside [1, 15]; a side < 1;
 * D * H * W >= 2^31; workspace_bytes below the query's answer; a patch side < 1. */
int ctseg_patch_centres(const uint8_t* masks, int32_t K, int32_t D, int32_t H, int32_t W, const uint32_t* draws /* host, P x 3 */,
                        int32_t P, int32_t class_mask, const int32_t* patch /* host, 3 (d,h,w), or NULL */, void* workspace,
                        int64_t workspace_bytes, int32_t* centres /* device, P x 4 */, void* stream);
int64_t ctseg_patch_centres_workspace(int32_t K, int32_t D, int32_t H, int32_t W);

/* The crop pass: ctseg_augment3d_to_hwd on a patch of Pd x Ph x Pw output voxels, about a centre read from the device.  Dtypes,
 * layouts (image_out fp32 [Ph][Pw][Pd], masks_out [K][Ph][Pw][Pd], labels_out [Ph][Pw][Pd]), nearest / trilinear, constant / edge
 * border, window, gain / bias, label map, hist and mask_src are those of ctseg_augment3d_to_hwd, and so is what is rejected (with
 * a null centre in addition).  Two things differ:
 *   - The grid the matrix addresses is the SOURCE grid itself, D x H x W: there is no virtual resized volume, rz is the identity,
 *     and "outside" means outside [0, dim_a).
 *   - The kernel reads centre (DEVICE, 3 int32: d, h, w; row p of ctseg_patch_centres' table) and forms
 *     t'_a = A[a][3] + (float)c_a, one float32 add per axis; the sampling coordinate of output voxel o is then
 *     q_a = ((A[a][0]*od + A[a][1]*oh) + A[a][2]*ow) + t'_a.
 * This entry IS the affine pass with that translated matrix.  With A = the identity and A[a][3] = -(P_a / 2) every q is a whole
 * number and the patch is the exact crop src[c - P/2 + o] (cval / 0 / the edge voxel where that leaves the volume), with either
 * interp.  One launch per patch; the host never waits for the centre. */
int ctseg_patch3d_to_hwd(const void* image, int32_t image_dtype, const uint8_t* masks, int32_t K, int32_t D, int32_t H, int32_t W,
                         int32_t Pd, int32_t Ph, int32_t Pw, const float* matrix /* host */, const int32_t* centre /* DEVICE, 3 */,
                         int32_t interp, int32_t border, float cval, const int32_t* mask_src /* host */, int32_t window,
                         float win_lo, float win_hi, float gain, float bias, float* image_out, uint8_t* masks_out,
                         uint8_t* labels_out, int64_t* hist, void* stream);

/* Test-time augmentation of the 3-D network: the prediction of one VIEW (the network's logits for an augmented copy of the scan)
 * is resampled onto a TARGET grid and added into an accumulator there; ctseg_tta_finish turns the accumulator into labels.
 * Inputs and layout:
 *   - logits is the view's fp32 channels-last block [H][W][D][ld], the storage the network returns for one sample; channels
 *     0..C-1 are read.  ld % 4 == 0, 1 <= C <= 16, C <= ld.
 *   - The target grid is Dt x Ht x Wt.  layout 0 stores target rows in (h, w, d) order, the model's grid: row (th * Wt + tw) * Dt
 *     + td.  layout 1 stores them in (d, h, w) order, the raw scan's grid: row (td * Ht + th) * Wt + tw.
 *   - acc is [St][acc_ld] fp32, St = Dt * Ht * Wt, acc_ld % 4 == 0, acc_ld >= C + 1.  The caller zeroes it before the first view.
 *   - logits and acc are 16-byte aligned; every volume (D * H * W, Dt * Ht * Wt) has fewer than 2^31 voxels.
 *   - matrix (12 floats, row-major 3 x 4; rows and columns ordered d, h, w, as for ctseg_augment3d_to_hwd) and chan_src (C ints,
 *     or NULL for the identity) are HOST arrays copied into the kernel's arguments: no device upload, no synchronisation.
 * Every float operation is one float32 rounding; nothing is contracted into an FMA.
 *   - Sampling coordinate: the matrix maps a TARGET voxel t = (td, th, tw), taken as floats, to the point of the VIEW's grid that
 *     it samples: q_a = ((M[a][0]*td + M[a][1]*th) + M[a][2]*tw) + M[a][3], evaluated in that order.
 *   - Coverage: r_a = (int)floorf(q_a + 0.5f), the float clamped into [-1, n_a] before the conversion.  If any r_a lies outside
 *     [0, n_a) the view contributes nothing to this voxel and its accumulator row is not touched.
 *   - Sample, per channel: interp 0 takes z_c = logits[r][c].  interp 1 (trilinear) uses b_a = floorf(q_a), f_a = q_a - b_a; the
 *     corners b + {0,1}^3 are clamped to the volume and combined as lerp(x, y, t) = x + t * (y - x), along w first, then h, then d.
 *   - Value: mode 0 (mean of logits) v_c = z_c.  mode 1 (mean of probabilities) m = max_c z_c, e_c = expf(z_c - m), s = the sum
 *     of e_c in channel order, v_c = e_c / s.
 *   - Accumulate: acc[t][k] += weight * v[chan_src[k]] for k < C, and acc[t][C] += weight: column C is the voxel's weight sum.
 *     Columns beyond C keep their bits.  One thread owns a voxel's row and there are no atomics: views added in the same order
 *     give the same bits.
 * Rejected before any launch: a null pointer; a matrix entry that is not finite, or a row that sends the target grid beyond 1e30;
 * a weight that is not finite or is <= 0; a chan_src that is no permutation of 0..C-1; mode, interp or layout out of range; ld or
 * acc_ld breaking the conditions above; an unaligned logits or acc. */
int ctseg_tta_accumulate(const float* logits, int32_t ld, int32_t C, int32_t D, int32_t H, int32_t W, const float* matrix /* host, 12 */,
                         const int32_t* chan_src /* host, C, or NULL */, float weight, int32_t mode, int32_t interp, int32_t Dt,
                         int32_t Ht, int32_t Wt, int32_t layout, float* acc, int32_t acc_ld, void* stream);
/* The accumulator of ctseg_tta_accumulate (same acc_ld, C, mode; St rows, 0 < St < 2^31) -> an answer:
 *   - labels[t] is the first maximal k of acc[t][0..C), the tie rule of _squash_predictions (capstone/training/utils.py); a voxel
 *     that no view covered (acc[t][C] == 0) gets label 0.
 *   - probs [St][C], or NULL: acc[t][k] / acc[t][C] in mode 1; in mode 0 the softmax, by the formula above, of acc[t][k] / acc[t][C].
 *     An uncovered voxel gets an all-zero row.
 *   - hist (C counters, which the caller zeroes), or NULL: hist[k] counts the labels. */
int ctseg_tta_finish(const float* acc, int32_t acc_ld, int32_t C, int64_t St, int32_t mode, uint8_t* labels,
                     float* probs /* [St][C] or NULL */, int64_t* hist /* C, caller zeroes, or NULL */, void* stream);

/* 2-D input pipeline on the device, a whole batch in one launch: the presets of capstone/transforms/predefined.py that are
 * per-pixel and index arithmetic (windowed_degree_1, windowed_degree_2, every "test" side):
 *   window     apply_window (capstone/transforms/transforms_2d.py:97-107) per window c: lo = win_lo[c], hi = win_hi[c] (HOST
 *              arrays of C <= 4 ints), clip(v, lo, hi) and with shift (clipped - lo) / (hi - lo + 1e-8); integer input is
 *              evaluated in float64, fp32 input in fp32 (numpy's result for a float32 array); the value is then held as float64
 *   geometry   mode 0 CROP:   Cr = x[y0:y0+Ho, x0:x0+Wo], R = np.rot90(Cr, k), out = R[:, ::-1] if flip else R, the same
 *                             indices for image and masks (k odd needs Ho == Wo)
 *              mode 1 RESIZE: image bilinear with half-pixel centres on the windowed float64 values, per axis
 *                             f = (float)((d + 0.5) * (In / Out) - 0.5), s = floor(f), w = f - s in float32, s < 0 -> (0, 0),
 *                             s >= In - 1 -> (In - 1, 0), a * (1 - w) + b * w in float64 with 1 - w formed in float32,
 *                             horizontal pass first; masks nearest, s = min(floor(d * (In / Out)), In - 1) in float64
 *                             (y0, x0, k, flip are not read)
 *   normalize  (float)v, then - mean[c], then * denom[c] (HOST arrays of C floats, denom = 1 / std formed by the caller): two
 *              fp32 roundings; mean == denom == NULL: the cast alone
 * Nothing is contracted into an FMA.  image_store holds the raw slices (image_dtype CTSEG_I16 / CTSEG_U8 / CTSEG_F32,
 * image_elems elements), mask_store their masks as u8 planes [K][H][W] (mask_bytes bytes; K <= 15).  table (DEVICE) and
 * table_host (its HOST copy, which is validated before the launch) are int64 [B][8] rows
 *   image_off (elements into image_store), mask_off (bytes into mask_store), H, W, y0, x0, k, flip
 * so slices of different sizes share one launch.  Outputs, each optional: image_out fp32 [B][C][Ho][Wo], masks_out u8
 * [B][K][Ho][Wo] (the raw bytes), labels_out u8 [B][Ho][Wo] (highest set class wins: ctseg_squash_masks' rule), hist int64
 * [B][K+1] (needs labels_out) and present int32 [B][K] = any(output mask == 1) per RAW mask (ctseg_squash_masks_present's
 * meaning); hist and present are zeroed by the caller.  image_store or mask_store may be NULL. */
int ctseg_pipeline2d_batch(const void* image_store, int32_t image_dtype, int64_t image_elems, const uint8_t* mask_store,
                           int64_t mask_bytes, const int64_t* table, const int64_t* table_host, int32_t B, int32_t K, int32_t mode,
                           int32_t Ho, int32_t Wo, int32_t C, const int32_t* win_lo, const int32_t* win_hi, int32_t shift,
                           const float* mean, const float* denom, float* image_out, uint8_t* masks_out, uint8_t* labels_out,
                           int64_t* hist, int32_t* present, void* stream);

/* The warping presets (degree_0, windowed_degree_3, windowed_degree_4 "train") on the device, three launches per batch:
 * window -> A.RandomCrop -> A.ElasticTransform or A.GridDistortion -> rot90 / flip -> normalize, with ctseg_pipeline2d_batch's
 * window, normalize and mask-side arithmetic and its outputs.  table / table_host are int64 [B][19] rows: the 8 columns of
 * ctseg_pipeline2d_batch (the crop is always Ho x Wo at (y0, x0); k and flip turn the WARPED crop), then
 *   kind (0 NONE, 1 ELASTIC, 2 GRID), seed, the INVERSE 2x3 affine matrix M00 M01 M02 M10 M11 M12 as float64 bit patterns,
 *   xx_off, yy_off (elements into xx / yy: Wo and Ho float32 map values of a GRID sample), slot (ELASTIC: index of the sample's
 *   fields, rising from 0 below n_slots)
 *   fields  per ELASTIC sample and field f (0: dx, 1: dy): noise(i, j) = 2 u - 1, u = (z >> 11) * 2^-53 with z the splitmix64 mix
 *           of seed + ((f << 40 | i << 20 | j) + 1) * 0x9E3779B97F4A7C15; separable blur in float64, axis 0 then axis 1, border
 *           "reflect" (d c b a | a b c d, any distance), out[l] = in[l] w[0] + sum_{k=1..radius} (in[l-k] + in[l+k]) w[k] in that
 *           order; fields[slot][f] = (float)(blur * alpha).  gauss_w: DEVICE float64 [radius + 1], normalised by the caller.
 *           field_tmp: float64 [n_slots][2][Ho][Wo], fields: float32 of the same shape.
 *   pass 1  inter = float64 [B][C][Ho][Wo] windowed crop, then u8 [B][K][Ho][Wo] mask bytes.  ELASTIC: cv2.warpAffine of the crop,
 *           border REFLECT_101 on the crop: X = (lrint((M01 y + M02) 1024) + 16 + lrint(M00 x 1024)) >> 5 (Y from M10, M11, M12;
 *           lrint saturates to int32), sx = X >> 5, fx = (X & 31) / 32; masks nearest with + 512 and >> 10.
 *   pass 2  cv2.remap of inter, border REFLECT_101: ELASTIC map_x = (float)(c + dx[r][c]), map_y = (float)(r + dy[r][c]); GRID
 *           map_x = xx[c], map_y = yy[r]; NONE a copy.  Bilinear: sx = lrint(map_x * 32) in float32 (half to even), ix = sx >> 5,
 *           fx = (sx & 31) / 32; nearest: lrint(map_x).  Both bilinear steps: float32 weights (1-fx)(1-fy), fx(1-fy), (1-fx)fy,
 *           fx fy, v = s00 w0 + s01 w1 + s10 w2 + s11 w3 in float64, left to right.
 * Ho, Wo <= 256 and max(Ho, Wo) + 2 radius <= 6144.  launches: bit 0 fields, bit 1 pass 1, bit 2 pass 2 (7: all of them).  The
 * host table is validated before any launch; the kernels repeat the range checks and leave a refused sample untouched. */
int ctseg_pipeline2d_warp_batch(const void* image_store, int32_t image_dtype, int64_t image_elems, const uint8_t* mask_store,
                                int64_t mask_bytes, const int64_t* table, const int64_t* table_host, int32_t B, int32_t K, int32_t Ho,
                                int32_t Wo, int32_t C, const int32_t* win_lo, const int32_t* win_hi, int32_t shift, const float* mean,
                                const float* denom, const double* gauss_w, int32_t radius, double alpha, const float* xx,
                                int64_t xx_elems, const float* yy, int64_t yy_elems, float* fields, double* field_tmp, int32_t n_slots,
                                void* inter, int64_t inter_bytes, float* image_out, uint8_t* masks_out, uint8_t* labels_out,
                                int64_t* hist, int32_t* present, int32_t launches, void* stream);

/* Distance maps of the 2-D pipeline (capstone/data/utils.py:10-26, compute_distance_map) for P planes of H x W mask bytes
 * (contiguous, nonzero = foreground) in two launches: the exact Euclidean distance transform, separable and in integers.
 *   d2_fg / d2_bg  int32 [P][H][W], each optional: the squared distance to the nearest foreground / background pixel of the
 *                  plane, -1 where the plane has none
 *   out            fp32 [P][H][W].  mode 0 (REFERENCE): the reference keeps its result in a uint8 array, so its map is
 *                  k / 255.0 of the byte k = isqrt(d2_fg) & 255 outside a structure and (1 - isqrt(d2_bg)) & 255 inside; here
 *                  out = table[k], table = 256 fp32 on the device that the caller fills with float32(k / 255.0).  mode 1
 *                  (SIGNED): sqrt(d2_fg) / 255 outside, -(sqrt(d2_bg) - 1) / 255 inside, each step rounded to fp32.
 *                  A plane without foreground is all zero, as in the reference; so is a plane without background, for which
 *                  the reference has no defined value.
 *   workspace      >= 4 * P * H * W bytes on the device, 4-byte aligned; its contents are not kept between calls
 * H, W <= 1024.  Every argument is validated on the host before the first launch. */
int ctseg_distmap2d_batch(const uint8_t* masks, int32_t P, int32_t H, int32_t W, int32_t mode, const float* table,
                          void* workspace, int64_t workspace_bytes, float* out, int32_t* d2_fg, int32_t* d2_bg, void* stream);

/* The same maps for P volumes of X x Y x Z mask bytes, Z innermost (the (K, H, W, D) storage ctseg_resize3d_to_hwd writes), in
 * three launches: a sweep along X, a lower-envelope pass along Z and one along Y that also forms the value.  The distances are the
 * exact 3-D squared Euclidean distances; masks, mode, table, out, d2_fg and d2_bg are as above, per volume.  No atomics: two runs
 * give the same bits.
 *   workspace      >= 6 * P * X * Y * Z bytes on the device (4 per voxel for the line pass's result, then 2 per voxel for the
 *                  sweep's), 4-byte aligned; its contents are not kept between calls
 * X, Y, Z <= 1024 (3 * 1023^2 fits int32 and float's 24 bits; the LDS tiles cover lines of 1024 on Y and Z, and X is only
 * swept).  Every argument is validated on the host before the first launch. */
int ctseg_distmap3d_batch(const uint8_t* masks, int32_t P, int32_t X, int32_t Y, int32_t Z, int32_t mode, const float* table,
                          void* workspace, int64_t workspace_bytes, float* out, int32_t* d2_fg, int32_t* d2_bg, void* stream);

/* Surface metrics between two label maps: the percentile Hausdorff distance and the average surface distance, per sample and
 * class 1..C-1, in voxels of the labels' grid.  Three calls in stream order, no host synchronisation between them:
 *   ctseg_surface_edges -> ctseg_distmap3d_batch(masks = edges, P = 2*B*(C-1), d2_fg = d2, d2_bg = NULL) -> ctseg_surface_select.
 * ctseg_surface_edges: pred, target uint8 [B][X][Y][Z] -> edges uint8 [2][B][C-1][X][Y][Z] (side 0 = pred, 1 = target; every byte
 *   written, 0 or 1) and counts[2][B][C-1] += the surface voxels of each volume (zeroed by the caller; integer atomics).  A voxel of
 *   label c is on the surface of class c when a neighbour at +-1 along an active axis is outside the volume or holds another
 *   label; `axes` is the mask of active axes, X = 1 | Y = 2 | Z = 4 (planes: [B][H][W][1] with axes = 3).  A label >= C is in no
 *   class and differs from every neighbour's.  With Z a multiple of 16, pred, target and edges are 16-byte aligned.
 * ctseg_surface_select: row r = (side, b, c) takes the values d2[partner row][v] at the voxels v with edges[r][v] != 0, the
 *   squared distances from this side's surface to the other's (d2: the d2_fg output of the transform of `edges`).  With n =
 *   counts[r], r_q = (n - 1) * (q / 100) in float64, lo = floor(r_q), hi = min(lo + 1, n - 1):
 *     stats[r]  = {d2 of rank lo, d2 of rank hi, the largest d2, 1}   (ranks in ascending order, from 0; exact integers)
 *     fstats[r] = {sum over v of sqrt(d2) in float64, r_q - lo}
 *   and all zeros on a row where counts[r] or its partner's is 0: the flag stats[r][3] says whether the row has values.  The sum
 *   is added from per-workgroup partials in a fixed order and the histograms are integer atomics: two runs give the same bits.
 *   workspace >= 2*B*(C-1) * CTSEG_SURFACE_SELECT_ROW_BYTES bytes, 8-byte aligned; the call zeroes what it needs of it.
 * Both: B >= 1, sides in 1..1024, 2 <= C <= 16, 2*B*(C-1) <= 65535; validated on the host before the first launch. */
#define CTSEG_SURFACE_SELECT_ROW_BYTES 25096
int ctseg_surface_edges(const uint8_t* pred, const uint8_t* target, int32_t B, int32_t X, int32_t Y, int32_t Z, int32_t C,
                        int32_t axes, uint8_t* edges, int32_t* counts, void* stream);
int ctseg_surface_select(const uint8_t* edges, const int32_t* d2, const int32_t* counts, int32_t B, int32_t X, int32_t Y, int32_t Z,
                         int32_t C, double q, void* workspace, int64_t workspace_bytes, int32_t* stats, double* fstats,
                         void* stream);

/* The same metrics in physical units: a weighted transform and a select on float32 keys.  Three calls in stream order:
 *   ctseg_surface_edges -> ctseg_distmap3d_weighted(masks = edges, P = 2*B*(C-1), d2_fg = d2, d2_bg = NULL) -> ctseg_surface_select_f32.
 * ctseg_distmap3d_weighted: masks as ctseg_distmap3d_batch takes them; w[P][3] float32 on the device, the SQUARED voxel sizes of
 *   every volume along X, Y, Z (finite and positive: the table is on the device, so the caller answers for its values).
 *   d2_fg / d2_bg float32 [P][X][Y][Z], either may be NULL, not both: the squared physical distance to the nearest foreground /
 *   background voxel, 0 at a voxel of that class, -1.0f everywhere when the volume has none.  For voxel v the value is the
 *   minimum over the voxels u of the class, (dx, dy, dz) = |u - v|, of
 *     fl(fl(wy * dy^2) + fl(fl(wz * dz^2) + fl(wx * dx^2)))
 *   every fl() one float32 rounding to nearest, the integer squares exact: the result is defined bit for bit.  No value map is
 *   written.  workspace >= 6 * P * X * Y * Z bytes, 4-byte aligned, as for ctseg_distmap3d_batch; sides up to 1024.
 * ctseg_surface_select_f32: ctseg_surface_select on those float32 squared distances.  Rows, ranks, fstats and determinism are the
 *   same; the order statistics are taken over the bit patterns of the non-negative floats (three radix levels, 11 + 11 + 9 bits);
 *     stats[r] = {bits of d2 of rank lo, bits of d2 of rank hi, bits of the largest d2, 1}   (float32 bit patterns in int32 words)
 *   workspace >= 2*B*(C-1) * CTSEG_SURFACE_SELECT_F32_ROW_BYTES bytes, 8-byte aligned.
 * Both validate every argument on the host before the first launch. */
#define CTSEG_SURFACE_SELECT_F32_ROW_BYTES 41480
int ctseg_distmap3d_weighted(const uint8_t* masks, int32_t P, int32_t X, int32_t Y, int32_t Z, const float* w, void* workspace,
                             int64_t workspace_bytes, float* d2_fg, float* d2_bg, void* stream);
int ctseg_surface_select_f32(const uint8_t* edges, const float* d2, const int32_t* counts, int32_t B, int32_t X, int32_t Y, int32_t Z,
                             int32_t C, double q, void* workspace, int64_t workspace_bytes, int32_t* stats, double* fstats,
                             void* stream);

/* Surface Dice at tolerance (normalised surface Dice): one launch, no workspace.  pred, target uint8 [B][X][Y][Z] and `axes` as for
 * ctseg_surface_edges, whose surface rule this is.  For side 0 = pred -> target and 1 = target -> pred, sample b and class c = 1..C-1:
 *     counts[side][b][c-1] += the voxels on the surface of c in that side's map
 *     within[side][b][c-1] += those of them with a voxel u on the surface of c in the OTHER map at an accepted offset (d0, d1, d2)
 * (both int32, zeroed by the caller; integer atomics: the same bits every run).  An offset is accepted
 *   without w2: when d0^2 + d1^2 + d2^2 <= limit[b][c-1], limit int32 [B][C-1] on the device;
 *   with w2:    when fl(fl(w1 * d1^2) + fl(fl(w2 * d2^2) + fl(w0 * d0^2))) <= limit[b][c-1], limit float32 [B][C-1] and w2 float32
 *               [B][3] on the device, the squared voxel sizes of the sample along X, Y, Z; every fl() one float32 rounding, the
 *               expression of ctseg_distmap3d_weighted.
 * radius int32 [B][C-1][3] ON THE HOST: per sample, class and axis a bound of |d_a| over the accepted offsets, each in
 *   0..CTSEG_SURFACE_DICE_MAX_RADIUS.  Their maxima per axis size the search box and the halo of the launch: an accepted offset
 *   outside them is not found.  The table is read before the call returns.
 * B in 1..65535, sides in 1..1024, 2 <= C <= 16; validated on the host before the launch. */
#define CTSEG_SURFACE_DICE_MAX_RADIUS 8
int ctseg_surface_dice(const uint8_t* pred, const uint8_t* target, int32_t B, int32_t X, int32_t Y, int32_t Z, int32_t C,
                       int32_t axes, const int32_t* radius, const void* limit, const float* w2, int32_t* counts, int32_t* within,
                       void* stream);

/* Connected components of a label map, and the keep-largest / minimum-size clean-up of a prediction on top of them (what MONAI
 * ships as KeepLargestConnectedComponent).  Two calls in stream order, no host synchronisation between them:
 *   ctseg_components_label -> ctseg_components_keep(labels, ids, sizes as the first call left them).
 * A component is a maximal set of voxels of ONE label in 1..C-1 joined by neighbour steps inside its sample: different classes never
 * join, samples never join, and the end of a Z row (or of a Y plane) is no neighbour of the start of the next.  Label 0 and labels
 * >= C are in no component.  Neighbours differ by +-1 along at most `connectivity` (1, 2, 3) of the active axes: 6 / 18 / 26 of them
 * in a volume; `axes` is the mask of active axes, X = 1 | Y = 2 | Z = 4, as in ctseg_surface_edges (planes: [B][H][W][1] with
 * axes = 3, where connectivity 1 / 2 is 4 / 8 neighbours); a connectivity above the number of active axes means all of them.
 * ctseg_components_label: labels uint8 [B][X][Y][Z] -> both int32 [B][X][Y][Z], every word written:
 *     ids[v]    the smallest index (x * Y + y) * Z + z WITHIN THE SAMPLE over the voxels of v's component, its representative;
 *               -1 where the voxel is in no component
 *     sizes[v]  the component's voxel count at its representative (ids[v] == v), 0 everywhere else
 *   Three launches: tiles of 8 x 16 x 32 voxels labelled in LDS, unions across the tile faces on `ids` (atomic minima), a flatten
 *   that also adds the tiles' counts up (integer atomic adds).  Parent links only ever decrease, so every loop ends and no
 *   workgroup waits for another; the representative is the minimum whatever the order of the unions and integer sums commute: the
 *   output is unique, and two runs give the same bits.  With Z a multiple of 16, labels, ids and sizes are 16-byte aligned.
 * ctseg_components_keep: out uint8 [B][X][Y][Z], every byte written.  A voxel of a class c whose bit is set in class_mask (bits
 *   1..C-1 only) keeps its label when (keep_largest == 0 or its component is the largest of class c in its sample) and its
 *   component has at least min_size voxels; otherwise it becomes 0.  Among equally large components the one with the smallest
 *   representative wins: the one whose first voxel comes first in raster order.  Label 0, labels >= C and the other classes are
 *   copied.  table int32 [B][C-1][4], for every class 1..C-1, processed or not:
 *     {number of components, size of the largest, its representative (-1: the class is absent), voxels set to 0}
 *   Four launches; the winner is one 64-bit atomic maximum of size << 32 | ~representative per class, counts are integer atomic
 *   adds: the same bits every run.  workspace >= B * (C-1) * CTSEG_COMPONENTS_KEEP_ROW_BYTES bytes, 8-byte aligned; the call zeroes
 *   it.  With X * Y * Z a multiple of 16, labels and out are 16-byte aligned.
 * Both: B >= 1 (at most 65535), sides in 1..1024, B * X * Y * Z < 2^31, 2 <= C <= 16; every argument is validated on the host
 * before the first launch.  Device memory: 10 bytes per voxel (labels 1 + ids 4 + sizes 4 + out 1) and 16 per sample and class. */
#define CTSEG_COMPONENTS_KEEP_ROW_BYTES 16
int ctseg_components_label(const uint8_t* labels, int32_t B, int32_t X, int32_t Y, int32_t Z, int32_t C, int32_t connectivity,
                           int32_t axes, int32_t* ids, int32_t* sizes, void* stream);
int ctseg_components_keep(const uint8_t* labels, const int32_t* ids, const int32_t* sizes, int32_t B, int32_t X, int32_t Y, int32_t Z,
                          int32_t C, int32_t class_mask, int32_t keep_largest, int32_t min_size, void* workspace,
                          int64_t workspace_bytes, uint8_t* out, int32_t* table, void* stream);

/* Enclosed holes of a label map filled (what MONAI ships as FillHoles): one call, six launches in stream order, no host
 * synchronisation.  labels, out uint8 [B][X][Y][Z]; neighbours, `connectivity`, `axes` and the limits as for ctseg_components_label.
 *   A background component is a maximal set of voxels of label exactly 0 joined by neighbour steps inside its sample.  It touches
 *   the boundary when one of its voxels has coordinate 0 or side - 1 along an ACTIVE axis.  Its border set holds the labels of all
 *   neighbours of its voxels that are not 0, every label >= C counting as one foreign label.  The component is a hole of class c when
 *   it does not touch the boundary, its border set is exactly {c} with 1 <= c < C, bit c of class_mask (bits 1..C-1 only) is set
 *   and max_size == 0 or the component has at most max_size voxels.  The voxels of a hole become c in `out`; every other voxel,
 *   labels >= C included, is copied: every byte of `out` is written.  One pass: a component bordered by two classes stays.
 *   table int32 [B][C-1][2], every word written: {holes filled, voxels filled} of every class.
 *   Launches: the background map (which also clears the border words and the table), the three of ctseg_components_label on that
 *   map, the border pass (integer atomic OR at the component's representative, reduced per lane and per tile of 8 x 16 x 32 first),
 *   the rewrite (integer atomic adds into the table).  OR and integer sums commute: the same bits every run.
 *   workspace: ctseg_fill_holes_workspace_bytes(B, X, Y, Z, C) bytes = CTSEG_FILL_HOLES_BYTES_PER_VOXEL per voxel (ids 4 + sizes 4 +
 *   border word 4 + map 1), 16-byte aligned, any content on entry; the query returns -1 for dimensions that the call refuses.
 *   With X * Y * Z a multiple of 16, labels and out are 16-byte aligned.  Every argument is validated on the host before the first
 *   launch. */
#define CTSEG_FILL_HOLES_BYTES_PER_VOXEL 13
int ctseg_fill_holes(const uint8_t* labels, int32_t B, int32_t X, int32_t Y, int32_t Z, int32_t C, int32_t connectivity, int32_t axes,
                     int32_t class_mask, int32_t max_size, void* workspace, int64_t workspace_bytes, uint8_t* out, int32_t* table,
                     void* stream);
int64_t ctseg_fill_holes_workspace_bytes(int32_t B, int32_t X, int32_t Y, int32_t Z, int32_t C);

/* Sliding-window inference (BASELINE.json configs[4]).  The reference has no inferer (grep: 0 hits); the
 * semantics are those of MONAI 0.3 `monai.inferers.sliding_window_inference`, the companion of the `monai.networks.nets.UNet`
 * the reference builds at capstone/volumetric/base_trainer.py:65-72.
 *  gather: vol fp32 [Cin][X][Y][Z] -> dst dtype [rx][ry][rz][ld] = the window at (x0,y0,z0); voxels outside the volume = cval
 *          (MONAI pads volumes smaller than the ROI; starts may be negative), pad channels = 0.
 *  blend : out[x0+x][y0+y][z0+z][c] += importance[x][y][z] * inv_count[dst voxel] * logits[x][y][z][c] for voxels inside
 *          the volume (inv_count == NULL: factor 1 — used to accumulate the weight sum itself); one window per launch, so
 *          overlapping windows accumulate in stream order (deterministic). */
int ctseg_window_gather(const float* vol, int32_t Cin, int32_t X, int32_t Y, int32_t Z, int32_t x0, int32_t y0, int32_t z0,
                        int32_t rx, int32_t ry, int32_t rz, float cval, void* dst, int32_t dtype, int32_t ld, void* stream);
/* The same for nw windows in one launch: starts[nw][3] (device) = window origins, dst = [nw][rx*ry*rz][ld]. */
int ctseg_window_gather_batch(const float* vol, int32_t Cin, int32_t X, int32_t Y, int32_t Z, const int32_t* starts, int32_t nw,
                              int32_t rx, int32_t ry, int32_t rz, float cval, void* dst, int32_t dtype, int32_t ld, void* stream);
int ctseg_window_blend(const float* logits, int32_t ld, int32_t C, int32_t rx, int32_t ry, int32_t rz, int32_t x0, int32_t y0,
                       int32_t z0, const float* importance, const float* inv_count, float* out, int32_t X, int32_t Y, int32_t Z,
                       int32_t out_ld, void* stream);
/* The same accumulation for ALL nw windows of one forward batch in one launch (logits [nw][rx*ry*rz][ld], starts[nw][3] =
 * window origins in output coordinates, on the device): per output voxel the covering windows are added in index order, i.e.
 * exactly the sums of nw ctseg_window_blend calls in that order.  Rows are 16-byte vectors: ld == out_ld, a multiple of 4, <= 16.
 * bbox (HOST pointer, 6 ints: origin x,y,z and extents, inside the volume; NULL = whole volume) bounds the voxels swept: it must
 * contain every window of the batch clipped to the volume. */
int ctseg_window_blend_batch(const float* logits, int32_t ld, int32_t C, int32_t rx, int32_t ry, int32_t rz, const int32_t* starts,
                             int32_t nw, const float* importance, const float* inv_count, float* out, int32_t X, int32_t Y,
                             int32_t Z, int32_t out_ld, const int32_t* bbox, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CTSEG_HIP_H */
