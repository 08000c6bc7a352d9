/* libeffdet_hip.so - C ABI of the MI355X (gfx950) EfficientDet inference + OOD-scoring hot path (and of the
 * pretrain step's loss / backward / optimizer operators).
 *
 * The reference (DavidPetrus/ood_object_detection, a fork of rwightman/efficientdet-pytorch 0.2.3) is
 * pure Python with no FFI layer: its "operator API" for this path is a handful of Python callables and
 * the PyTorch ops under them.  Each entry point below names the reference call site (file:line under
 * the reference tree) whose arithmetic it replaces; INTEGRATION.md shows the ctypes binding a
 * maintainer of the reference would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless it is an array-of-parameters argument documented as
 *     host memory ("host:" below); buffers are caller-owned; nothing is allocated internally;
 *   - `stream` is a hipStream_t; all work is enqueued on it; no call synchronises (graph-capturable);
 *   - activations are NHWC, channels a multiple of 8; `dtype` 0 = float32 (parity mode),
 *     1 = bfloat16 (throughput mode, fp32 accumulate); weights of the MFMA GEMMs use the same dtype,
 *     every per-channel vector (scale/shift/bias/depthwise taps/SE weights) is float32; the effdet_train_* and
 *     effdet_eval_* entry points are float32 only (channels a multiple of 4);
 *   - `dtype` 2 = EFFDET_BF16X2, the "accurate" mode (accepted by effdet_stem_dw_fused[_u8], effdet_mbconv_expand_dw[_gated],
 *     effdet_pw_gemm_bn_act / _group, effdet_sepconv_fused, effdet_maxpool_same and the *_parts / *_tiles queries): every
 *     activation and GEMM weight is the unevaluated sum of two bfloat16 numbers, x ~ hi + lo with hi = bf16(x),
 *     lo = bf16(x - hi) (16 significand bits), and a multiply is three bf16 MFMAs (hi*hi + hi*lo + lo*hi, fp32 accumulate) -
 *     float32-grade results (north_star's 1e-3 against the reference's float32 CPU path) without the 16x slower fp32 MFMA.
 *     Layout: 8 consecutive channels (or 8 consecutive K of a weight row) are 32 bytes, [8 x bf16 hi][8 x bf16 lo]; a tensor
 *     therefore has the shape, pitch and byte size of its float32 counterpart.  Pointers 16-byte aligned, channel counts
 *     multiples of 8.  The kernel that PRODUCES a value splits it; ood_object_detection_amd/pairfmt.py packs weights.  The
 *     reference computes this path in float32 (effdet/anchors.py:136, efficientdet.py:895-933): dtype 0 and dtype 2 both
 *     stand for it, at different speeds;
 *   - return value: 0 on success, -22 (EINVAL) for a rejected argument, -5 (EIO) if the launch failed or if a kernel
 *     of an EARLIER call flagged a failure on the device (effdet_device_error);
 *   - thread-safe per stream; the only global mutable state is the device-side failure word.
 */
#ifndef EFFDET_HIP_H
#define EFFDET_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define EFFDET_F32 0
#define EFFDET_BF16 1
#define EFFDET_BF16X2 2          /* two-term bfloat16 values ("accurate" mode), see Conventions */
/* Padding convention of strided convolutions / pools (timm `padding=`, effdet config.pad_type; reference call sites
 * effdet/efficientdet.py:46,66,70,165): default TF-"SAME" (the tf_ model family); OR this flag into the `dtype` argument of an
 * inference entry point that pads (effdet_stem_*, effdet_mbconv_expand_dw[_gated], effdet_dwconv_bn_act, effdet_maxpool_same,
 * effdet_sepconv_fused) - or into the first selector argument of a training entry point that pads (`k` of effdet_train_dwconv_*,
 * `op` of effdet_train_spatial, `method` of effdet_train_fpn_combine / _wgrad, `idx` of effdet_train_fpn_input_bwd, `B` of
 * effdet_train_im2col_stem) - for pad_type='' (efficientdet_d0 / d1 on efficientnet_b0 / b1: static symmetric padding
 * ((s-1)+(k-1))/2).  Output sizes are the same; the window of a stride-2 layer on an even map starts one pixel earlier. */
#define EFFDET_PAD_SYMMETRIC (1 << 24)

/* ABI version of this header (bumped on any signature change). */
int effdet_abi_version(void);
/* Text of the HIP error behind the calling thread's most recent -5 return. */
const char* effdet_last_error(void);
/* Device-side failure word: kernels OR a bit into it when they detect a failure they cannot return (bit 0: a wave of the
 * wide MBConv kernel ran out of spins waiting for its workgroup's X-ring hand-off - its output tile is invalid).  The word is
 * host-coherent memory: no copy, no synchronisation.  While it is non-zero every launching entry point returns -5.
 * Returns the word; clear != 0 resets it.  (The reference has no counterpart: PyTorch raises from the failing op itself.) */
int effdet_device_error(int clear);

/* ---- backbone (timm EfficientNet; timm call sites effdet/efficientdet.py:17-18,837) ---------------- */

/* conv_stem 3x3/s2 TF-SAME + bn1 + SiLU.  X: NCHW [B,3,H,W] (in_dtype), Wt: [27][Cout] tap-major
 * (ky,kx,ci), Y: NHWC [B,ceil(H/2),ceil(W/2),Cout] (out_dtype). */
int effdet_stem_conv(void* stream, int in_dtype, int out_dtype, const void* X, const float* Wt,
                     const float* scale, const float* shift, void* Y, int B, int H, int W, int Cout);

/* Fused conv_stem + bn1 + SiLU -> blocks.0.0 depthwise 3x3/s1 + BN + SiLU (+ SE pool partials); the stem
 * output stays in LDS.  Wk: [C][32] im2col weights (dtype), k = (ky*3+kx)*3+ci zero-padded from 27 to 32;
 * taps [9][C] fp32; Y NHWC [B,ceil(H/2),ceil(W/2),C]; pool_partial [B][effdet_stem_dw_parts(dtype,H,W,C)][C]
 * or NULL: the launch writes exactly that many rows per image (the count depends on the form the dtype and
 * sizes select) - size AND sum the buffer by effdet_stem_dw_parts.  The same rule holds for
 * effdet_mbconv_expand_dw[_gated]: its pool_partial has effdet_mbconv[_gated]_tiles_per_image(dtype, ...) rows
 * per image.  C <= 64. */
int effdet_stem_dw_fused(void* stream, int in_dtype, int dtype, const void* X, const void* Wk,
                         const float* s1, const float* t1, const float* taps, const float* s2, const float* t2,
                         void* Y, float* pool_partial, int B, int H, int W, int C);
int effdet_stem_dw_parts(int dtype, int H, int W, int C);      /* pool partial rows per image of the kernel that will run (bf16: rolling-window form) */
/* Alignment of X: the rolling-window form (bf16 and two-term bf16 with C = 32, an even W and ceil(W/2) >= 16, ceil(H/2) >= 8)
 * loads two adjacent pixels of a plane with one instruction and returns EFFDET_EINVAL, before any launch, unless X is aligned to
 * that load: 4 bytes for float32 and bfloat16 images, 2 bytes for uint8 images.  The tile form takes any element-aligned X.
 * Host-only: the form and geometry an effdet_stem_dw_fused[_u8] call (in_dtype 0 | 1 | 2 = uint8) would run, from the functions
 * the launch itself uses (stem_dw_plan / pick_stem_roll); contract of effdet_pw_gemm_plan_describe (negative where the launch
 * refuses; the pad flag in dtype selects pad_t / pad_l and is otherwise stripped).  Slots:
 *    0  form: 0 = 16 x 16 tiles (stem_dw.hip), 1 = rolling window (stem_roll.hip);  1  pool partial rows per image (= effdet_stem_dw_parts)
 *    2  pad_t;  3  pad_l;  4  Ho;  5  Wo;  6  tiles along x | strips;  7  tiles along y | bands;  8  tile width | strip width in
 *    output columns;  9  tile height | rows per band;  10  workgroups per image (rolling form; 0 for tiles);  11  dynamic LDS bytes
 *    12  tile form: the geometric part of the two-pixel patch load (bf16 image into bf16, even W, even pad_l; the launch also
 *        wants X 4-byte aligned); 0 in the rolling form */
#define EFFDET_STEM_DW_PLAN_INTS 13
int effdet_stem_dw_plan_describe(int dtype, int in_dtype, int H, int W, int C, int* out, int n);

/* Input normalisation of the reference's PrefetchLoader (effdet/data/loader.py:114-128):
 * y = (float(x) - mean[c]) / std[c], x uint8 NCHW [B,C,hw], mean/std = 255 * the dataset constants
 * (host arrays of C <= 4 floats), y in out_dtype.  The *_u8 stem entry points apply the same arithmetic
 * (result rounded to the model dtype, exactly what feeding the normalised tensor would give) while loading
 * the input patch, so a uint8 batch needs no separate pass. */
/* ResizePad (effdet/data/transforms.py:75-107): Pillow's 8-bit BILINEAR resize of an HWC uint8 image [h][w][3] to
 * sw x sh, pasted top-left on an S x S canvas of fill_rgb (host array of 3 ints), written planar [3][S][S].  bounds_*
 * [out][2] = (first source index, count) and coef_* [out][ksize] are Pillow's integer coefficient tables (22 fractional
 * bits; device pointers, built by the caller as Pillow's precompute_coeffs / normalize_coeffs_8bpc do); workspace:
 * h*sw*3 bytes.  Bit-identical to Image.resize(.., BILINEAR) + paste. */
int effdet_resize_pad_u8(void* stream, const unsigned char* src, int h, int w, unsigned char* dst, int S, int sw, int sh,
                         const int* bounds_x, const int* coef_x, int ksize_x,
                         const int* bounds_y, const int* coef_y, int ksize_y,
                         const int* fill_rgb, unsigned char* workspace);
int effdet_normalize_u8(void* stream, int out_dtype, const unsigned char* X, const float* mean, const float* stdv,
                        void* Y, int B, int C, long long hw);

/* The image transforms of effdet/data/transforms.py for a whole ragged batch in one launch: ResizePad (:75-107),
 * RandomFlip + RandomResizePad (:170-276) and ProjResizePad's pixel path (:143-148).  Per image, in this order: mirror the stored
 * frame (flip_h / flip_v), take the crop rectangle (cx0, cy0, cw, ch) of the mirrored frame, resample it to sw x sh with
 * Pillow's 8-bit filter (0 = BILINEAR, 1 = BICUBIC; bounds clamp to the crop, as img.crop(..).resize(..) does), take the
 * window that starts at (ox, oy) of the resampled image and paste its min(S, sw - ox) x min(S, sh - oy) pixels top-left on
 * an S x S canvas of the fill colour.  src: uint8 HWC [h][w][3], pitch 3 * w, ANY byte alignment (the aligned 32-bit words
 * that cover a row are loaded).  Output: planar uint8 [B][3][S][S], image pitch dst_image_stride bytes (<= 0: 3 * S * S).
 * The coefficient tables are computed on the device in fp64 exactly as Pillow's precompute_coeffs / normalize_coeffs_8bpc
 * do; results are bit-identical to PIL and do not depend on the batch an image travels in.  No workspace.
 * desc: device array of B descriptors; desc_host: the same B descriptors in host memory (read during the call only: argument
 * checks and the LDS size of the launch).  fill_rgb: host array of 3 ints.  Limits: cw <= 64 * sw and ch <= 64 * sh (a 64 : 1
 * reduction per axis), sizes up to 2^20, B <= 65535, S <= 16384; beyond them -22. */
typedef struct EffdetResampleDesc {
    const unsigned char* src;
    int h, w;
    int flip_h, flip_v;
    int cx0, cy0, cw, ch;
    int filter;
    int sw, sh;
    int ox, oy;
    int reserved;
} EffdetResampleDesc;                /* 64 bytes */
int effdet_resample_batch_u8(void* stream, const EffdetResampleDesc* desc, const EffdetResampleDesc* desc_host, int B,
                             unsigned char* dst, long long dst_image_stride, int S, const int* fill_rgb);

/* The box arithmetic of the same transforms (transforms.py:96-103, 150-158, 216-227, 250-260) in float32, one rounding per
 * reference operation: flip (x' = img_w - x with the two x columns swapped; y likewise), subtract (pre_y, pre_x), multiply by
 * scale, subtract (post_y, post_x), clip to [0, clip_h] x [0, clip_w], keep the rows with ymin < ymax and xmin < xmax.
 * boxes [B][Mmax][4] yxyx, classes [B][Mmax] int64, padding rows = class -1 with a zero box (what effdet_label_anchors reads);
 * Mmax <= 512.  out_boxes / out_classes: the kept rows in their original order, then padding rows; counts [B] int32;
 * valid [B][Mmax] bytes (0 / 1) aligned with the INPUT rows (anno['valid_indices']).  Outputs must not alias inputs. */
typedef struct EffdetBoxParams {
    float img_w, img_h;
    int flip_h, flip_v;
    float pre_y, pre_x, scale, post_y, post_x, clip_h, clip_w;
    int reserved;
} EffdetBoxParams;                   /* 48 bytes */
int effdet_transform_boxes(void* stream, const float* boxes, const long long* classes, const EffdetBoxParams* params,
                           int B, int Mmax, float* out_boxes, long long* out_classes, int* counts, unsigned char* valid);
int effdet_stem_conv_u8(void* stream, int out_dtype, const unsigned char* X, const float* mean, const float* stdv,
                        const float* Wt, const float* scale, const float* shift, void* Y, int B, int H, int W, int Cout);
int effdet_stem_dw_fused_u8(void* stream, int dtype, const unsigned char* X, const float* mean, const float* stdv,
                            const void* Wk, const float* s1, const float* t1, const float* taps, const float* s2, const float* t2,
                            void* Y, float* pool_partial, int B, int H, int W, int C);

/* 1x1 conv as GEMM with folded BN / bias, optional SiLU (act=1) or ReLU (act=2), optional SE gate on A
 * (gate [B,K] fp32, rows_per_image = H*W), optional residual [M,N].  A: [M,K], W: [N,K].
 * Output row m goes to C + (m / rows_per_image) * c_image_stride + (m % rows_per_image) * ldc
 * (pass 0 for rows_per_image / c_image_stride / ldc to get a plain [M,N] matrix).
 * Replaces conv_pw / conv_pwl + BatchNorm2d (+Swish) of timm's MBConv blocks and the BiFPN lateral
 * ConvBnAct2d (effdet/efficientdet.py:42-57, :155-158). */
int effdet_pw_gemm_bn_act(void* stream, int dtype, const void* A, long long M, int K, const void* W, int N,
                          const float* scale, const float* shift, int act, const void* residual,
                          const float* gate, int rows_per_image,
                          void* C, long long c_image_stride, long long ldc);
/* n <= 8 independent GEMMs of this form (no gate, no residual, dense [M][N] outputs) in ONE launch; every N must select the
 * same output-channel tile (N <= 96).  The BiFPN's lateral 1x1 convs of the backbone features (ResampleFeatureMap.conv,
 * effdet/efficientdet.py:155-158): six small problems that each fill a fraction of the chip. */
int effdet_pw_gemm_group(void* stream, int dtype, int n, const void* const* A, const long long* M, const int* K,
                         const void* const* W, const int* N, const float* const* scale, const float* const* shift,
                         int act, void* const* C);
/* Host-only: the kernel instantiation and geometry an effdet_pw_gemm_bn_act call of this shape runs - answered by the launcher's
 * own dispatch, which describes its choice instead of launching.  gated / has_residual: the pointer is present; `aligned` != 0:
 * A, W, C and the residual are 32-byte aligned (with N, ldc and c_image_stride this decides vec_ok; two-term calls are refused
 * without it); rows_per_image, ldc, c_image_stride: 0 for the defaults, as in the launch.  group != 0: the call is a group launch
 * of this one problem (no gate, no residual, a dense output, BN <= 96).  Contract of effdet_sepconv_plan_describe: fills
 * min(n, EFFDET_PW_GEMM_PLAN_INTS) ints of `out` and returns that count, or EFFDET_EINVAL (out == NULL, n <= 0, or anything the
 * launch refuses from the shape); a pad flag in dtype is ignored.  Slots:
 *    0  BN: output channels per workgroup as instantiated;  1  PT: 16-pixel tiles per wave;  2  NTH: threads per workgroup
 *    3  GATED;  4  tiles_per_image (128-pixel tiles);  5  n_tiles (output-channel tiles);  6  workgroups of the launch
 *    7  small: the launch has fewer than 512 workgroups (PT 1, NTH 512 unless BN is 128)
 *    8  vec_ok: residual loads and output stores are 8-channel vectors
 *    9  K-chunks;  10  pipeline stages (nst);  11  LDS bytes, static + dynamic;  12  K values per K-chunk
 * effdet_pw_gemm_group_plan_describe: the same for an effdet_pw_gemm_group call of n_problems problems; slots 4, 5, 8, 9, 10
 * are those of problem `which`, slot 6 counts the whole launch. */
#define EFFDET_PW_GEMM_PLAN_INTS 13
int effdet_pw_gemm_plan_describe(int dtype, long long M, int K, int N, int rows_per_image, int gated, int has_residual,
                                 long long ldc, long long c_image_stride, int aligned, int group, int* out, int n);
int effdet_pw_gemm_group_plan_describe(int dtype, int n_problems, const long long* M, const int* K, const int* N, int aligned,
                                       int which, int* out, int n);

/* depthwise k x k (k = 3|5, stride 1|2, TF-SAME) + folded BN + SiLU.  Wt: [k*k][C] fp32.
 * If pool_partial != NULL it receives [B][effdet_dwconv_blocks_per_image(Ho,Wo,C)][C] partial sums of
 * the output for the squeeze-excite average. */
int effdet_dwconv_bn_act(void* stream, int dtype, const void* X, void* Y, const float* Wt,
                         const float* scale, const float* shift, int act, float* pool_partial,
                         int B, int H, int W, int C, int k, int stride);
int effdet_dwconv_blocks_per_image(int Ho, int Wo, int C);
/* Host-only: the geometry an effdet_dwconv_bn_act call on an H x W x C map runs (pooled != 0: with pool_partial), from the
 * function the launch itself uses; contract of effdet_pw_gemm_plan_describe (the pad flag in dtype selects pad_t / pad_l and is
 * otherwise stripped).  Slots:
 *    0  KS;  1  nz: channel slices (grid.z);  2  CG: 8-channel groups per workgroup;  3  PT: pixels in flight per workgroup
 *    4  threads per workgroup;  5  pixels per workgroup;  6  workgroups per image and slice (= effdet_dwconv_blocks_per_image)
 *    7  pad_t;  8  pad_l;  9  LDS bytes */
#define EFFDET_DWCONV_PLAN_INTS 10
int effdet_dwconv_plan_describe(int dtype, int H, int W, int C, int k, int stride, int pooled, int* out, int n);

/* Fused front half of an inverted-residual block: expand 1x1 (MFMA) + BN + SiLU -> depthwise k x k
 * (TF-SAME, stride 1|2) + BN + SiLU; the expanded activation never leaves LDS.  W1: [mid][Cin] (dtype),
 * taps: [k*k][mid] fp32.  pool_partial (optional): [B][effdet_mbconv_tiles_per_image(...)][mid] partial
 * sums for the SE average.  Early stages run as spatial tiles, late stages (wide inputs, small maps) as
 * (row band x 64-channel slice) workgroups; the choice is internal.  Replaces conv_pw/bn1/act1/conv_dw/bn2/act2 of timm's InvertedResidual. */
int effdet_mbconv_expand_dw(void* stream, int dtype, const void* X, void* Y, const void* W1,
                            const float* s1, const float* t1, const float* taps,
                            const float* s2, const float* t2, float* pool_partial,
                            int B, int H, int W, int Cin, int mid, int k, int stride);
int effdet_mbconv_tiles_per_image(int dtype, int H, int W, int Cin, int mid, int k, int stride);
/* The same with X multiplied by a per-image channel gate [B][Cin] (rounded to dtype) while it is loaded.  Lets a
 * squeeze-excited, residual-free block hand its depthwise output straight to the next block: its project conv +
 * BN (both linear) are folded into W1 / t1 by the caller, so the narrow tensor in between is never written.
 * Always the spatial-tile geometry: size pool_partial with effdet_mbconv_gated_tiles_per_image. */
int effdet_mbconv_expand_dw_gated(void* stream, int dtype, const void* X, const float* in_gate, void* Y, const void* W1,
                                  const float* s1, const float* t1, const float* taps,
                                  const float* s2, const float* t2, float* pool_partial,
                                  int B, int H, int W, int Cin, int mid, int k, int stride);
int effdet_mbconv_gated_tiles_per_image(int dtype, int H, int W, int Cin, int mid, int k, int stride);
/* Host-only plan query (launches nothing): which fused form and which geometry effdet_mbconv_expand_dw (gated == 0) or
 * effdet_mbconv_expand_dw_gated (gated != 0) runs for this block - answered by the launcher's own planning function.
 * EFFDET_PAD_SYMMETRIC in dtype is ignored (no geometry depends on the padding convention).  Fills min(n,
 * EFFDET_MBCONV_PLAN_INTS) ints of `out` and returns that count, or EFFDET_EINVAL (out == NULL, n <= 0, or Cin / mid not a
 * positive multiple of 8, which the launch refuses before it plans; the two tiles_per_image queries do not make that check and
 * answer for the geometry alone).  Slots, unused ones 0:
 *    0  form: 0 none (the caller runs expand GEMM + depthwise), 1 rolling window, 2 shared-X rolling window ("wide"),
 *             3 band x channel slice ("deep"), 4 spatial tiles ("front")
 *    1  parts: pool-partial rows per image (= effdet_mbconv[_gated]_tiles_per_image; 0 for form 0)
 *    2  nkc: 32-channel K chunks of Cin                         (roll, wide)
 *    3  MT: 16-pixel input tiles per strip row                  (roll, wide)
 *    4  NO: 16-pixel output tiles per strip row                 (roll, wide)
 *    5  NJ: channel tiles per wave (roll) / NPL: 16-byte X pieces a lane stages per row (wide)
 *    6  TWo: strip width in output pixels                       (roll, wide)
 *    7  nstrips                                                 (roll, wide)
 *    8  band_rows: output rows per band                         (roll, wide, deep)
 *    9  nbands                                                  (roll, wide, deep)
 *   10  waves per workgroup                                     (roll, wide)
 *   11  dynamic LDS bytes of a workgroup                        (every form)
 *   12  nchunks: 64-channel slices of mid                       (deep)
 *   13  TH, 14 TW: output tile; 15 tiles_x, 16 tiles_y          (front) */
#define EFFDET_MBCONV_PLAN_INTS 17
int effdet_mbconv_plan_describe(int dtype, int H, int W, int Cin, int mid, int k, int stride, int gated, int* out, int n);

/* SqueezeExcite gate: mean -> fc(C->R)+SiLU -> fc(R->C) -> sigmoid.  W1: [R][C] (conv_reduce weight),
 * W2t: [R][C] (conv_expand weight TRANSPOSED, so that consecutive threads read consecutive channels). */
int effdet_se_gate(void* stream, const float* partial, int nblk, int hw, const float* W1, const float* b1,
                   const float* W2t, const float* b2, float* gate, int B, int C, int R);

/* ---- BiFPN + heads (effdet/efficientdet.py:140-469) ---------------------------------------------- */

/* create_pool2d('max', 3, 2, 'same') (effdet/efficientdet.py:165-166): P6, P7.  image strides in
 * elements (0 = dense). */
int effdet_maxpool_same(void* stream, int dtype, const void* X, long long x_image_stride,
                        void* Y, long long y_image_stride, int B, int H, int W, int C);

/* Fused FpnCombine -> Swish -> SeparableConv2d -> BN for one BiFPN node (nlevels = 1,
 * effdet/efficientdet.py:224-245, :281-292), or one HeadNet layer over all pyramid levels
 * (nlevels <= 5, effdet/efficientdet.py:438-452) with the per-anchor OOD energy / max-logit epilogue
 * when ood_classes > 0.  All array arguments are host: memory.
 *   level_hw[l] = {H,W};  per (level, input): pointer, image stride (elements), {H,W}, mode
 *   (0 same size, 1 nearest x2 upsample, 2 max-pool 3x3/s2 SAME);
 *   fuse_mode 0: single input, 1: sum_i (x_i*w_i)/den ('fastattn'), 2: sum_i x_i*w_i ('attn','sum');
 *   dw_w [9][F] fp32; pw_w [N][F] (dtype); scale/shift [rows][N] fp32 indexed by affine_row[l]
 *   (scale may be NULL); out_ptr[l] + b*out_image_stride[l] + (y*W+x)*N.
 *   dtype 3 (= 1 | 2): bfloat16 inputs / weights, float32 OUTPUTS written straight from the accumulators (out pointers and
 *   strides then address float32 elements) - used for the box regressions, which decode reads as float32 (anchors.py:136).
 *   dtype 6 (= 2 | 4): two-term bf16 inputs / weights, plain float32 OUTPUTS (the accurate mode's class logits and box
 *   regressions: what _post_process and decode read). */
int effdet_sepconv_fused(void* stream, int dtype, int B, int nlevels, const int* level_hw, int n_in,
                         const void* const* in_ptr, const long long* in_image_stride, const int* in_hw,
                         const int* in_mode, int fuse_mode, const float* fuse_w, float fuse_den, int pre_act,
                         const float* dw_w, const void* pw_w, const float* scale, const float* shift,
                         const int* affine_row, int post_act, int F, int N,
                         void* const* out_ptr, const long long* out_image_stride,
                         int ood_classes, int num_anchors, float* ood_energy, float* ood_maxlogit,
                         long long ood_image_stride, const long long* ood_level_off);
/* Host-only plan query (launches nothing): which instantiation of the kernel template and which geometry a call of
 * effdet_sepconv_fused with this dtype (EFFDET_PAD_SYMMETRIC is ignored: no form depends on the padding convention), these
 * levels, n_in, F, N, ood_classes / num_anchors, scale present or NULL and post_act runs - answered by the launcher's own
 * dispatch, which describes its choice instead of launching.  `aligned` != 0: every output pointer is 16-byte aligned and every
 * output image stride a whole number of dwords (together with the row lengths this decides vec_ok; two-term calls are refused
 * without it).  Contract of effdet_mbconv_plan_describe: fills min(n, EFFDET_SEPCONV_PLAN_INTS) ints of `out` and returns that
 * count, or EFFDET_EINVAL (out == NULL, n <= 0, or anything the launch refuses from the shape: dtype, level count and sizes,
 * n_in, F not a positive multiple of 8, N, num_anchors * ood_classes != N, a tile that does not fit 160 KiB of LDS).  Slots:
 *    0  element kind: 0 float32, 1 bf16, 2 two-term bf16
 *    1  TH, 2 TW: pixel tile;  3 threads per workgroup
 *    4  FT: compile-time channel count (0: the generic-width kernel)
 *    5  BN: output channels per chunk (96: class chunk, 64)
 *    6  OOD: per-anchor chunks with the energy / max-logit epilogue
 *    7  BST: the branch-free class predict
 *    8  NIN: inputs the instantiation holds registers for (1 or 3)
 *    9  META: the MetaHead form (0 from this query: it describes effdet_sepconv_fused)
 *   10  subs: sub-chunks per anchor (1 without OOD)
 *   11  nchunks: channel chunks a workgroup walks
 *   12  tiles_total: workgroups per image
 *   13  dynamic LDS bytes of a workgroup
 *   14  the depthwise taps are prefetched into registers (9 F <= 1536 with 512 threads, <= 1280 with 256)
 *   15  the next W chunk is prefetched into registers
 *   16  float32 outputs from a 16-bit compute kind (dtype 3 / 6)
 *   17  vec_ok: 8-channel output pieces leave as vectors */
#define EFFDET_SEPCONV_PLAN_INTS 18
int effdet_sepconv_plan_describe(int dtype, int nlevels, const int* level_hw, int n_in, int F, int N, int ood_classes,
                                 int num_anchors, int has_scale, int post_act, int aligned, int* out, int n);

/* MetaHead (effdet/efficientdet.py:569-695): the fork's functional class head - SeparableConv layers shared by the
 * levels, each followed by F.batch_norm(training=True) (statistics of the current batch, per level) and Swish.
 * effdet_sepconv_meta runs one layer for all levels: the previous layer's batch-norm arrives folded into
 * in_scale / in_shift [rows][F] (row in_affine_row[level]; NULL for the first layer) applied before the SiLU (pre_act),
 * the conv output q + bias is written raw and, per tile and channel, three floats go to stat_partial
 * [B][effdet_sepconv_tiles][3][N] (NULL: not needed): a pivot (the tile's first pixel), the sum of q - pivot and the sum of
 * (q - pivot)^2 over the tile's pixels inside the map.  dw_out (optional, per level [B, H*W, F]) receives the
 * depthwise output (`x_pred`, what ret_activs returns).  effdet_bn_batch_stats (same dtype and level_hw as the launch that
 * wrote the table: the tile counts follow from them) merges the tiles by Chan's update in double and turns them into the next
 * layer's scale / shift [nlevels][N]: scale = w / sqrt(var_biased + eps), shift = b - mean * scale with
 * weight / bias [rows][N] (row param_row[level]).
 * Widths: F a multiple of 8 whose tile fits 160 KiB of LDS - up to 288 (float32 needs 162 432 bytes there); F >= 384 returns
 * the invalid-argument code from effdet_sepconv_meta in both dtypes, before anything is launched. */
int effdet_sepconv_meta(void* stream, int dtype, int B, int nlevels, const int* level_hw,
                        const void* const* in_ptr, const long long* in_image_stride,
                        const float* in_scale, const float* in_shift, const int* in_affine_row, int pre_act,
                        const float* dw_w, const void* pw_w, const float* bias, int F, int N,
                        void* const* out_ptr, const long long* out_image_stride,
                        float* stat_partial, void* const* dw_out, const long long* dw_out_image_stride);
int effdet_sepconv_tiles(int dtype, int nlevels, const int* level_hw, int* level_tile_begin);
int effdet_bn_batch_stats(void* stream, int dtype, const float* partial, int B, int nlevels, const int* level_hw, int N,
                          const float* weight, const float* bias, const int* param_row, float eps,
                          float* out_scale, float* out_shift);

/* ---- post-processing ------------------------------------------------------------------------------ */

/* _post_process (effdet/bench.py:12-56).  cls_all [B, n_anchors, C], box_all [B, n_anchors, 4] (dtype);
 * outputs out_cls [B,k], out_box [B,k,4] (dtype), out_indices / out_classes [B,k] int64.
 * Descending by logit, ties by lower flat index.  k <= 16384.
 * anchor_max: optional [B, n_anchors] fp32 maximum logit of every anchor (the class head's OOD max-logit
 * output); lets the select skip the anchors that cannot reach the top k.  NULL: computed internally. */
long long effdet_topk_workspace_bytes(int B, long long n_anchors);
int effdet_topk_select(void* stream, int dtype, const void* cls_all, const float* anchor_max, int B, long long n_anchors, int C,
                       const void* box_all, int k, void* out_cls, void* out_box,
                       long long* out_indices, long long* out_classes, void* workspace, long long workspace_bytes);

/* generate_detections, first half (effdet/anchors.py:132-144): decode, clip (when img_scale and img_size
 * are given), sigmoid, keep score > 0.01 (order kept).  Outputs are [B,k(,4)] with count[b] valid rows.
 * dtype 0: logits and box regressions float32; 1: both bfloat16; 3 (= 1 | 2): bfloat16 logits, float32 box regressions
 * (what a bfloat16 model's box head writes, see effdet_sepconv_fused). */
int effdet_decode_threshold(void* stream, int dtype, const void* cls_topk, const void* box_topk,
                            const float* anchors, const long long* indices, const long long* classes,
                            const float* img_scale, const float* img_size, int B, int k,
                            float* boxes, float* scores, int* classes_out, int* src, int* count, float* maxcoord);
/* The same with the box regressions taken from the box head's full output box_all [B, n_anchors, 4] through `indices`
 * (effdet_topk_select may then be called with box_all = NULL and run concurrently with the box head). */
int effdet_decode_threshold_gather(void* stream, int dtype, const void* cls_topk, const void* box_all, long long n_anchors,
                                   const float* anchors, const long long* indices, const long long* classes,
                                   const float* img_scale, const float* img_size, int B, int k,
                                   float* boxes, float* scores, int* classes_out, int* src, int* count, float* maxcoord);

/* generate_detections, second half (effdet/anchors.py:145-166).  det [B,max_det,6] zero padded rows
 * x1,y1,x2,y2,score,class+1; det_count [B]; keep_src [B,max_det] = position in the top-k list or -1.
 * Hard: torchvision batched_nms semantics (anchors.py:150).  Soft: effdet/soft_nms.py:42-169. */
int effdet_nms_hard(void* stream, const float* boxes, const float* scores, const int* classes, const int* src,
                    const int* count, const float* maxcoord, int B, int k, double iou_threshold, int max_det,
                    const float* img_scale, float* det, int* det_count, int* keep_src);

/* effdet_decode_threshold[_gather] followed by effdet_nms_hard in ONE launch (the hard-NMS path of generate_detections,
 * effdet/anchors.py:132-166): n_anchors > 0 reads the box regressions from the head's [B, n_anchors, 4] output through `indices`
 * (0: `box` is the gathered [B, k, 4] tensor); img_scale_clip / img_size as in effdet_decode_threshold (clipping, both or neither),
 * img_scale_out as effdet_nms_hard's img_scale (output scaling).  The compacted intermediate arrays are still written. */
int effdet_detections_hard(void* stream, int dtype, const void* cls_topk, const void* box, long long n_anchors,
                           const float* anchors, const long long* indices, const long long* classes,
                           const float* img_scale_clip, const float* img_size, int B, int k,
                           float* boxes, float* scores, int* classes_out, int* src, int* count, float* maxcoord,
                           double iou_threshold, int max_det, const float* img_scale_out,
                           float* det, int* det_count, int* keep_src);

int effdet_nms_soft(void* stream, const float* boxes, const float* scores, const int* classes, const int* src,
                    const int* count, const float* maxcoord, int B, int k, int method_gaussian, float sigma,
                    float iou_threshold, float score_threshold, int max_det,
                    const float* img_scale, float* det, int* det_count, int* keep_src);

/* The same soft-NMS for any k (the stand-alone soft_nms / batched_soft_nms API of effdet/soft_nms.py:42-169 has no size
 * limit and returns every pick): working scores in `score_scratch` [B,k] floats, max_det <= k. effdet_nms_soft itself
 * keeps the candidates in registers (k <= 8192, max_det <= k). */
int effdet_nms_soft_large(void* stream, const float* boxes, const float* scores, const int* classes, const int* src,
                          const int* count, const float* maxcoord, int B, int k, int method_gaussian, float sigma,
                          float iou_threshold, float score_threshold, int max_det,
                          const float* img_scale, float* det, int* det_count, int* keep_src, float* score_scratch);

/* OOD scores of the kept detections: energy/maxlogit [B,n_anchors] -> [B,max_det] (0 where padded); out_anchor
 * (optional) receives the anchor index each kept detection came from (-1 where padded). */
int effdet_gather_ood(void* stream, const int* keep_src, const long long* indices, const float* energy,
                      const float* maxlogit, long long n_anchors, int B, int k, int max_det,
                      float* out_energy, float* out_maxlogit, long long* out_anchor);

/* ---- training-side operators -------------------------------------------------- */

/* loss_fn (effdet/loss.py:224-298): alpha-weighted BCE-with-logits on one-hot targets (gamma unused, as in the
 * fork), label smoothing, `target != -2` mask, Huber box loss on targets != 0, normaliser sum(num_positives)+1.
 * cls [B,N,C], box [B,N,4] (dtype), cls_t [B,N] int64 (class index, -1 background, -2 ignore), box_t [B,N,4] fp32.
 * out3 = {total, class_loss, box_loss}; grad_cls / grad_box (dtype, optional) = d total / d head outputs. */
long long effdet_detection_loss_workspace_floats(int B, long long N, int C);
int effdet_detection_loss(void* stream, int dtype, const void* cls, const void* box, const long long* cls_t,
                          const float* box_t, const float* num_positives, int B, long long N, int C,
                          float alpha, float delta, float box_loss_weight, float label_smoothing,
                          float* out3, void* grad_cls, void* grad_box, float* workspace, long long workspace_floats);

/* AnchorLabeler.batch_label_anchors (effdet/anchors.py:384-438): IoU (region_similarity_calculator.py:24-73),
 * ArgMaxMatcher thresholds (t, t) with force_match_for_each_row (argmax_matcher.py:116-146), class target =
 * label - 1 (background -1), FasterRcnnBoxCoder.encode (box_coder.py:81-110).  gt_boxes [B,Mmax,4] yxyx,
 * gt_cls [B,Mmax] int64 (rows with class <= -1 are padding / filtered), anchors [N,4] yxyx.
 * Outputs cls_t [B,N] int64, box_t [B,N,4], num_positives [B], match [B,N] int64 (optional; index into the
 * valid rows, -1 unmatched).  Mmax <= 512. */
long long effdet_label_anchors_workspace_bytes(int B, int Mmax, long long N);
int effdet_label_anchors(void* stream, const float* anchors, const float* gt_boxes, const long long* gt_cls,
                         int B, int Mmax, long long N, float match_threshold, long long* cls_t, float* box_t,
                         float* num_positives, long long* match, void* workspace, long long workspace_bytes);

/* The same assignment for the reference's filter_valid=False (effdet/data/loader.py:84): every row takes part whatever
 * its class, so a row of class c <= -1 is matched like any other (a zero box is forced onto anchor 0) and gives class
 * target c - 1, i.e. -2 for the usual -1, which effdet_detection_loss ignores.  Only rows of class EFFDET_LABEL_PAD are
 * the caller's own padding and invisible; `match` indexes the rows that are not.  Same workspace as above. */
#define EFFDET_LABEL_PAD (-0x7fffffffffffffffLL - 1)
int effdet_label_anchors_rows(void* stream, const float* anchors, const float* gt_boxes, const long long* gt_cls,
                              int B, int Mmax, long long N, float match_threshold, long long* cls_t, float* box_t,
                              float* num_positives, long long* match, void* workspace, long long workspace_bytes);

/* The `task_cls` branch of AnchorLabeler.batch_label_anchors (effdet/anchors.py:396-403), run before effdet_label_anchors
 * on the same padded tensors: per image, every row whose IoU (same arithmetic as above; boxlist1 = the rows of class
 * task_cls) with some row of class task_cls is > iou_threshold (the reference: 0.9) gets class task_cls, in place.
 * The decision reads the classes as they were on entry.  Padding rows (class -1, zero box) have IoU 0 and never change;
 * an image without a row of class task_cls is left alone.  task_cls >= 0, 0 < Mmax <= 512.  One launch for the batch. */
int effdet_relabel_task_cls(void* stream, const float* gt_boxes, long long* gt_cls, int B, int Mmax,
                            long long task_cls, float iou_threshold);

/* ProjectionNet.weighted_median (effdet/efficientdet.py:748-760): per column of embds [n][d] (n <= 1024), the value at
 * which the cumulative confidence (in ascending value order) first reaches half of sum(confs); conf_sum[0] = that sum. */
int effdet_weighted_median(void* stream, const float* embds, const float* confs, int n, int d, float* med, float* conf_sum);

/* ---- network backward of the pretrain step (pretrain.py:226-236 `qry_loss.backward()`) ------------
 * float32, NHWC.  Generic operators the host sequences into forward-with-saved-activations and backward
 * (ood_object_detection_amd/train_engine.py).  "Row maps": row m of a matrix lives at
 * base + (m / rpi) * img_stride + (m % rpi) * ld  (pass rpi = img_stride = 0 for a dense matrix; ld = 0 -> #columns):
 * lets the class / box predict layers read and write the packed [B, N, C] head outputs per pyramid level.
 * Every reduction is two-stage in a fixed order (bitwise reproducible gradients); workspaces are caller-owned. */

/* C[M,N] (+)= A[M,K] W[N,K]^T + bias[N] (bias may be NULL).  1x1-conv forward (replaces the nn.Conv2d(1x1) calls of
 * timm's blocks and effdet/efficientdet.py:42-83 in training), and its input gradient dX = dY W when W is passed
 * transposed.  C2 (optional, addressed like C) receives silu(C): the pre-activation and the activation in one pass. */
int effdet_train_gemm_nt(void* stream, const float* A, long long a_rpi, long long a_img_stride, long long a_ld,
                         const float* W, const float* bias, float* C, long long c_rpi, long long c_img_stride,
                         long long c_ld, long long M, int K, int N, int accumulate, float* C2);
/* dY[M,N]^T [X[M,K] | 1] in one pass: out = the 1x1-conv weight gradient as a dense [N][K] matrix followed by the N sums
 * sum_m dY[m,n] (bias / BN shift gradient); out holds N*K + N floats (autograd of conv2d 1x1). */
long long effdet_train_gemm_tn_workspace_floats(long long M, int N, int K);
int effdet_train_gemm_tn(void* stream, const float* dY, long long y_rpi, long long y_img_stride, long long y_ld,
                         const float* X, long long x_rpi, long long x_img_stride, long long x_ld,
                         long long M, int N, int K, float* out, float* workspace, long long workspace_floats);
/* out[g][l] (+)= sum_s in[g][s][l], s ascending. */
int effdet_train_reduce_mid(void* stream, const float* in, int G, int S, long long L, float* out, int accumulate);
/* depthwise k x k (k = 3|5, stride 1|2, TF-SAME) backward: dX [B,H,W,C] from dY [B,Ho,Wo,C] and taps [k*k][C];
 * out [(k*k+1)][C] = tap gradients (rows 0..k*k-1) and sum of dY (last row); cmajor != 0: the tap gradients in the
 * parameter's layout [C][k*k], followed by the C sums. */
int effdet_train_dwconv_bwd_dx(void* stream, const float* dY, const float* taps, float* dX,
                               int B, int H, int W, int C, int k, int stride);
long long effdet_train_dwconv_bwd_dw_workspace_floats(int B, int H, int W, int C, int k, int stride);
int effdet_train_dwconv_bwd_dw(void* stream, const float* dY, const float* X, float* out,
                               int B, int H, int W, int C, int k, int stride, float* workspace, long long workspace_floats, int cmajor);
/* Element-wise family over n floats (n, C multiples of 4; channel = i % C, image = i / (hw*C)):
 *  0 silu(a)   1 b*silu'(a)   2 a+b   3 a*v0[c]+v1[c] (v1 optional)   4 a*v0[img,c]   5 a*v0[img,c]+v1[img,c]*s0
 *  6 v0[c]*(a - v1[c] - (b - v2[c])*v3[c])  (batch-statistics BN backward)
 *  7 (a*s0)/s3 + (b*s1)/s3 [+ (c*s2)/s3]  (FpnCombine 'fastattn', effdet/efficientdet.py:240-242)   8 a*s0
 *  9 a*s0 + b*s1 [+ c*s2]   10 a*b   11 a*b*silu''(c)  (double backward of SiLU: the MetaHead's second-order MAML terms)
 * sdev (optional): device float[4] that replaces s0..s3 at run time, so that a captured hipGraph of the training step
 * sees the current BiFPN edge weights.  out2 (optional): silu(out), written in the same pass. */
int effdet_train_ew(void* stream, int op, float* out, const float* a, const float* b, const float* c,
                    const float* v0, const float* v1, const float* v2, const float* v3,
                    float s0, float s1, float s2, float s3, long long n, int C, long long hw, const float* sdev, float* out2);
/* Per-channel reductions over the rows of dense [G][R][C] tensors -> out [G][C]:
 * mode 0 sum a; 1 sum a*b; 2 sum (a - v[c])^2; 3 sum a*(b - v[c]); 4: modes 0 and 3 in one pass, out [G][2][C];
 * every result is multiplied by alpha (1/M gives means). */
long long effdet_train_col_reduce_workspace_floats(int G, long long R, int C);
int effdet_train_col_reduce(void* stream, int mode, const float* a, const float* b, const float* v,
                            int G, long long R, int C, float* out, float* workspace, long long workspace_floats, float alpha);
/* op 0: nearest x2 upsample in [B,H,W,C] -> out [B,2H,2W,C];  op 1: its backward, in = d out [B,2H,2W,C] -> [B,H,W,C];
 * op 2: 3x3/s2 TF-SAME max-pool backward, in = pool input [B,H,W,C], aux = dY [B,ceil(H/2),ceil(W/2),C] -> dX
 * (gradient goes to the first maximum of a window in row-major order, as torch's max_pool2d does). */
int effdet_train_spatial(void* stream, int op, const float* in, const float* aux, float* out, int B, int H, int W, int C);
/* conv_stem patches: X NCHW [B,3,H,W] fp32 -> col [B*ceil(H/2)*ceil(W/2)][32], k = (ky*3+kx)*3+ci, columns 27..31 zero. */
int effdet_train_im2col_stem(void* stream, const float* X, float* col, int B, int H, int W);
/* SqueezeExcite backward: pool_sum / gate / dgate [B,C], W1 [R][C], W2t [R][C] (as effdet_se_gate) -> ds [B,C]
 * (gradient w.r.t. the pooled mean) and per-image parameter gradients pgrad [B][R*C + R + R*C + C] =
 * {d conv_reduce.weight, d conv_reduce.bias, d conv_expand.weight^T, d conv_expand.bias}. */
int effdet_train_se_bwd(void* stream, const float* pool_sum, int hw, const float* gate, const float* dgate,
                        const float* W1, const float* b1, const float* W2t, float* ds, float* pgrad, int B, int C, int R);

/* Parameter-sized helpers of conv + BatchNorm on running statistics (one launch each instead of a dozen tensor ops):
 * fold: scale = gamma / sqrt(var + eps), shift = beta - mean * scale, rstd; Wf [N][K] = W * scale[n], WfT [K][N] = Wf^T,
 * WT [K][N] = W^T (each matrix optional).  grads: from dWext = effdet_train_gemm_tn's output ([N][K] then N sums; or the
 * depthwise [(K+1)][N] layout when transposed != 0): dW [N][K] = scale * dWraw, d gamma = rstd * (sum_k W * dWraw - mean * dsum),
 * d beta = dsum.  Each is one record of the stage tables below handed to the same device code by value (nothing is uploaded). */
int effdet_train_fold_bn(void* stream, const float* W, int N, int K, const float* gamma, const float* beta,
                         const float* mean, const float* var, float eps,
                         float* Wf, float* WfT, float* WT, float* scale, float* shift, float* rstd);
int effdet_train_convbn_grads(void* stream, const float* dWext, int N, int K, int transposed, const float* W,
                              const float* scale, const float* rstd, const float* mean,
                              float* dW, float* dgamma, float* dbeta);

/* nn.BatchNorm2d bookkeeping of the layers that are not folded (BiFPN / heads), one launch each.  finalize: from the batch
 * (train != 0: running stats updated with `momentum`, running_var with var * unbias, num_batches_tracked += 1) or running
 * (train == 0; pass them as mean / var) statistics -> rstd, scale = gamma * rstd, shift = beta - mean * scale.
 * bwd_prep: s1 = sum(dy), s2c = sum(dy (c - mean)) -> d gamma, d beta and the two vectors v1 = s1/M, v3 = rstd^2 s2c/M that
 * op 6 of effdet_train_ew needs. */
int effdet_train_bn_finalize(void* stream, const float* mean, const float* var, const float* gamma, const float* beta,
                             float* running_mean, float* running_var, long long* num_batches_tracked, int C, int train,
                             float momentum, float unbias, float eps, float* scale, float* shift, float* rstd);
int effdet_train_bn_bwd_prep(void* stream, const float* s1, const float* s2c, const float* rstd, int C, float inv_m,
                             float* dgamma, float* dbeta, float* v1, float* v3);
/* The two halves above fused with the column reductions in front of them (one launch less per BatchNorm and direction):
 * bn_var_finalize = effdet_train_col_reduce mode 2 over a [R][C] with the batch mean, then finalize in training mode;
 * bn_bwd_sums     = effdet_train_col_reduce mode 4 (sum dy, sum dy (c - mean)), then bwd_prep -> out [4][C] = d gamma, d beta, v1, v3.
 * workspace: effdet_train_col_reduce_workspace_floats(1, R, C) floats. */
int effdet_train_bn_var_finalize(void* stream, const float* a, const float* mean, long long R, int C, const float* gamma,
                                 const float* beta, float* running_mean, float* running_var, long long* num_batches_tracked,
                                 float momentum, float unbias, float eps, float* scale, float* shift, float* rstd,
                                 float* workspace, long long workspace_floats);
int effdet_train_bn_bwd_sums(void* stream, const float* dy, const float* c, const float* mean, const float* rstd,
                             long long R, int C, float* out, float* workspace, long long workspace_floats);

/* Stage tables: the records of effdet_train_fold_bn / plain transposes / effdet_train_fpn_weights and of
 * effdet_train_convbn_grads for all convs of a stage in one launch; a record computes bit for bit what the single call does
 * (one device body, csrc/train_param.h).  `table` = n records in DEVICE memory:
 *   prep  { int kind, rows, cols; float eps; const float *src, *gamma, *beta, *mean, *var; float *dst0, *dst1, *dst2, *scale,
 *           *shift, *rstd; }   kind 0: dst0 [cols][rows] = src [rows][cols] transposed; kind 1: fold_bn with W = src [N = rows][K = cols],
 *           dst0 = Wf, dst1 = WfT, dst2 = WT (each optional); kind 2: effdet_train_fpn_weights with src = edge_weights [rows],
 *           cols = 1, method = (int) eps, dst0 = {w0, w1, w2, den}
 *   grads { const float *dWext, *W, *scale, *rstd, *mean; float *dW, *dgamma, *dbeta; int N, K, transposed, pad; } */
int effdet_train_prep_table(void* stream, const void* table, int n, long long max_elems);
int effdet_train_grads_table(void* stream, const void* table, int n, int max_n);

/* ---- fused forms of one MBConv block of the backbone (timm InvertedResidual / DepthwiseSeparableConv, BN in eval mode) --------
 * train_dwconv_fwd:     conv_dw + folded BN: Z = pre-activation (kept for the backward), A = silu(Z) (optional) and the SE pool partial
 *                       rows of A ([B][effdet_train_dwconv_fwd_parts(H,W,C,k,stride)][C], optional) in one pass
 * train_se_gate:        effdet_se_gate that also writes the pooled sums [B][C] effdet_train_se_bwd reads
 * train_gemm_nt_fused:  C = (A * a_scale[row / a_scale_rows]) W^T + bias + R, C2 = silu(C): the SE gate [B][K] applied while A
 *                       is loaded, the shortcut R [M][N] added in the epilogue (a_scale, bias, R, C2 optional; dense rows)
 * train_gemm_tn_scaled: out = dY^T [X * x_scale[row / x_scale_rows] | 1] (weight gradient of the gated project conv)
 * train_dwconv_bwd_dx_silu: effdet_train_dwconv_bwd_dx followed by * silu'(Z) in the same pass
 * (effdet_train_ew op 12: (a * v0[img][c] + v1[img][c] * s0) * silu'(c) - SE gate backward and SiLU backward in one pass) */
int effdet_train_dwconv_fwd_parts(int H, int W, int C, int k, int stride);
int effdet_train_dwconv_fwd(void* stream, const float* X, float* Z, float* A, const float* Wt, const float* scale,
                            const float* shift, float* pool_partial, int B, int H, int W, int C, int k, int stride);
int effdet_train_se_gate(void* stream, const float* partial, int nblk, int hw, const float* W1, const float* b1,
                         const float* W2t, const float* b2, float* gate, float* pool_sum, int B, int C, int R);
int effdet_train_gemm_nt_fused(void* stream, const float* A, const float* a_scale, long long a_scale_rows, const float* W,
                               const float* bias, const float* R, float* C, float* C2, long long M, int K, int N);
int effdet_train_gemm_tn_scaled(void* stream, const float* dY, const float* X, const float* x_scale, long long x_scale_rows,
                                long long M, int N, int K, float* out, float* workspace, long long workspace_floats);
int effdet_train_dwconv_bwd_dx_silu(void* stream, const float* dY, const float* taps, const float* Z, float* dX,
                                    int B, int H, int W, int C, int k, int stride);

/* ---- ProjectionNet training (effdet/efficientdet.py:762: bias-free Linear + ReLU chain), dense float32 rows ------------------
 * gemm_nt_relu: C[M,N] = relu(A[M,K] W[N,K]^T)               hidden-layer forward (the pre-activation is not kept)
 * gemm_nt_mask: C[M,N] = (A[M,K] W[N,K]^T) * [mask[M,N] > 0]   input gradient of a Linear fed by a ReLU, W passed transposed and
 *               mask = that ReLU's output: the ReLU backward (0 where the pre-activation is exactly 0) in the GEMM's epilogue
 * relu_mask:    out[i] = g[i] * [y[i] > 0] over n floats       the same mask on its own (double backward of gemm_nt_mask)
 * The weight gradient is effdet_train_gemm_tn (its extra column of sums is not needed). */
int effdet_train_gemm_nt_relu(void* stream, const float* A, const float* W, float* C, long long M, int K, int N);
int effdet_train_gemm_nt_mask(void* stream, const float* A, const float* W, const float* mask, float* C, long long M, int K, int N);
int effdet_train_relu_mask(void* stream, const float* g, const float* y, float* out, long long n);

/* ---- host-only plan queries of the training GEMMs and depthwise entries (launch nothing) ------------------------------------------
 * What the launchers of effdet_train_gemm_nt* / _gemm_tn* / _dwconv_* decide from the shape, the row maps and the pointer
 * alignment, answered by the launchers' own decision code.  Contract of effdet_mbconv_plan_describe: fills min(n, *_PLAN_INTS) ints
 * of `out` and returns that count, or EFFDET_EINVAL (out == NULL, n <= 0, or arguments the entry points refuse).
 * A row-map side is (levels, rpi, img_stride, ld): levels == 0 -> the (rpi, img_stride, ld) map of effdet_train_gemm_nt (zeros:
 * dense rows); levels != 0 -> the level-packed map of the *_levels entries with img_stride = pk_img_stride, ld = pk_ld.
 * `align`: address mod 16 (0, 4, 8 or 12) of each pointer; entries of absent operands are ignored.
 * gemm_nt: operands = EFFDET_NT_HAS_* bits; epi 0 none / 1 relu / 2 mask (needs HAS_MASK); align[8] = A, W, C, bias, R, C2,
 *          a_scale, mask.  Slots: 0 VEC, 1 KS, 2 FAST, 3 EPI (template arguments of the kernel), 4 floats per store (4 / 2 / 1 -> 0),
 *          5 workgroups, 6 kchunk: the k range of one wave of the split-K form (0 when KS == 1)
 * gemm_tn: x_scale_rows > 0 -> effdet_train_gemm_tn_scaled (dense rows); align[3] = dY, X, x_scale.  Slots: 0 body (0 gemm_tn_kernel,
 *          1 the pipelined _v, 2 the 128-column _w), 1 VY (width of the dY loads), 2 VX (plain body; 1 for the others), 3 DENSE,
 *          4 SCALED, 5 S (slices over M), 6 rows_per_slice, 7 empty trailing slices, 8-10 grid x, y, z
 * dwconv:  which 0 effdet_train_dwconv_fwd / 1 _bwd_dx[_silu] / 2 _bwd_dw; k may carry EFFDET_PAD_SYMMETRIC.  Slots (those of the
 *          other entries 0): 0 Ho, 1 Wo, 2 pad_t, 3 pad_l, 4 channel groups of 64; forward: 5 blocks_per_image (= _fwd_parts),
 *          6 strips_x; d input: 7 kernel (1 the 4-pixel stride-1 form, 0 general), 8 workgroups; d taps: 9 seg, 10 segments per
 *          row, 11 segs_per_chunk, 12 chunks (workspace = chunks * (k * k + 1) * C floats) */
#define EFFDET_NT_HAS_BIAS 1
#define EFFDET_NT_HAS_R 2
#define EFFDET_NT_HAS_C2 4
#define EFFDET_NT_HAS_A_SCALE 8
#define EFFDET_NT_ACCUMULATE 16
#define EFFDET_NT_HAS_MASK 32
#define EFFDET_TRAIN_GEMM_NT_PLAN_INTS 7
#define EFFDET_TRAIN_GEMM_TN_PLAN_INTS 11
#define EFFDET_TRAIN_DWCONV_PLAN_INTS 13
int effdet_train_gemm_nt_plan_describe(long long M, int K, int N, int a_levels, long long a_rpi, long long a_img_stride,
                                       long long a_ld, int c_levels, long long c_rpi, long long c_img_stride, long long c_ld,
                                       int operands, long long a_scale_rows, int epi, const int* align, int* out, int n);
int effdet_train_gemm_tn_plan_describe(long long M, int N, int K, int y_levels, long long y_rpi, long long y_img_stride,
                                       long long y_ld, int x_levels, long long x_rpi, long long x_img_stride, long long x_ld,
                                       long long x_scale_rows, const int* align, int* out, int n);
int effdet_train_dwconv_plan_describe(int which, int H, int W, int C, int k, int stride, int B, int* out, int n);

/* ---- the head towers over the whole pyramid in one launch per layer (effdet/efficientdet.py:438-452: conv weights shared by
 * the levels, BatchNorm per level).  "Packed pyramid" = float32 [sum_l B*Hs[l]*Ws[l]][C], level-major: the NHWC tensors of the L
 * levels (L <= 8) one behind the other.  A 1x1 conv over it is ONE GEMM: effdet_train_gemm_nt_levels / _tn_levels are
 * effdet_train_gemm_nt / _tn over those rows, where the side flagged `*_packed` is instead the image-major head tensor of
 * effdet/loss.py's packing, [B][sum_l Hs[l]*Ws[l]][pk_ld] with pk_img_stride floats per image (a_packed and c_packed exclude each
 * other; C2 needs a dense C).  Reductions are two-stage in a fixed order (bitwise reproducible); `workspace`:
 * effdet_train_levels_workspace_floats floats.
 *   levels_dw          depthwise 3x3 / s1 / TF-SAME, taps [9][C]; flip != 0: taps mirrored = gradient w.r.t. the input
 *   levels_dw_bwd_dw   out [9][C] (cmajor != 0: [C][9], the parameter's layout) = gradient of the (shared) taps, summed over all levels
 *   levels_col_reduce  out [L][C] (mode 0: sum a; mode 2: sum (a - v[l][c] * vscale[l])^2) or [L][2][C] (mode 4: sum a',
 *                      sum a' (b - v[l][c]), a' = a * silu'(pre) when pre is given - the SiLU backward of the layer above)
 *   levels_bn_finalize nn.BatchNorm2d bookkeeping of the L layers (pointer tables of their parameters / buffers; train[l] != 0:
 *                      batch statistics mean = sum * inv_m, var = sq * inv_m, running stats updated; else running statistics)
 *                      -> mean, scale = gamma * rstd, shift = beta - mean * scale, rstd, all [L][C]
 *   levels_bn_bwd_prep sums [L][2][C] of mode 4 -> d gamma, d beta, v1, v3 ([L][C]; per level and channel the arithmetic of
 *                      effdet_train_bn_bwd_prep, as levels_bn_finalize shares effdet_train_bn_finalize's: csrc/train_param.h)
 *   levels_ew          op 3: out = a * v0[l][c] + v1[l][c] (out2 = silu(out) when given); op 6: BatchNorm backward
 *                      v0 (a' - v1 - (b - v2) v3) for levels with train[l] != 0, a' v0 otherwise; a' as in mode 4 */
int effdet_train_gemm_nt_levels(void* stream, const float* A, int a_packed, const float* W, const float* bias, float* C,
                                int c_packed, int B, int L, const int* Hs, const int* Ws, long long pk_img_stride,
                                long long pk_ld, int K, int N, float* C2);
int effdet_train_gemm_tn_levels(void* stream, const float* dY, int y_packed, const float* X, int B, int L, const int* Hs,
                                const int* Ws, long long pk_img_stride, long long pk_ld, int N, int K, float* out,
                                float* workspace, long long workspace_floats);
long long effdet_train_levels_workspace_floats(int B, int L, const int* Hs, const int* Ws, int C);
int effdet_train_levels_dw(void* stream, const float* X, const float* taps, float* Y, int B, int L, const int* Hs,
                           const int* Ws, int C, int flip);
int effdet_train_levels_dw_bwd_dw(void* stream, const float* dY, const float* X, float* out, int B, int L,
                                  const int* Hs, const int* Ws, int C, float* workspace, long long workspace_floats,
                                  int cmajor);
int effdet_train_levels_col_reduce(void* stream, int mode, const float* a, const float* b, const float* v,
                                   const float* pre, const float* vscale, int B, int L, const int* Hs, const int* Ws, int C,
                                   float* out, float* workspace, long long workspace_floats);
int effdet_train_levels_bn_finalize(void* stream, const float* sum, const float* sq, int L, int C, const void* const* gamma,
                                    const void* const* beta, void* const* running_mean, void* const* running_var,
                                    void* const* num_batches_tracked, const int* train, const float* inv_m,
                                    const float* unbias, const float* momentum, const float* eps,
                                    float* mean, float* scale, float* shift, float* rstd);
int effdet_train_levels_bn_bwd_prep(void* stream, const float* sums, const float* rstd, const float* inv_m, int L, int C,
                                    float* dgamma, float* dbeta, float* v1, float* v3);
int effdet_train_levels_ew(void* stream, int op, float* out, float* out2, const float* a, const float* b, const float* pre,
                           const float* v0, const float* v1, const float* v2, const float* v3, const int* train,
                           int B, int L, const int* Hs, const int* Ws, int C);

/* ---- one BiFPN node's FpnCombine without materialising the resampled inputs (effdet/efficientdet.py:180-245).  The n (2 or 3)
 * source tensors are float32 NHWC [B][hs[i]][ws[i]][C]; each is the node's size (identity), half of it (nearest x2 upsample) or
 * about twice it (3x3 / s2 TF-SAME max-pool) - told from the shapes.  method: 0 'fastattn', 1 'attn', 2 'sum'.
 *   fpn_weights   edge_weights -> wdev = {w0, w1, w2, den}: relu and den = sum + 1e-4 | softmax, den 1 | ones, den 1
 *   fpn_combine   fused = sum_i (R_i(x_i) * w_i) / den ('fastattn' arithmetic; else sum_i R_i(x_i) * w_i), act = silu(fused)
 *   fpn_wgrad     dots [n][C] = sum over pixels of dfused * R_i(x_i), dfused = dact * silu'(fused); grad [n] = d edge_weights
 *                 (workspace: effdet_train_fpn_dots_workspace_floats floats; method 2: dots only)
 *   fpn_input_bwd out = (w_idx / den) * R_idx^T(dfused) + acc (acc optional): gradient of source tensor idx, [B][h][w][C] */
int effdet_train_fpn_weights(void* stream, const float* edge_weights, int n, int method, float* wdev);
int effdet_train_fpn_combine(void* stream, int n, const void* const* srcs, const int* hs, const int* ws, int method,
                             const float* wdev, float* fused, float* act, int B, int H, int W, int C);
long long effdet_train_fpn_dots_workspace_floats(int B, int H, int W, int C);
int effdet_train_fpn_wgrad(void* stream, int n, const void* const* srcs, const int* hs, const int* ws, int method,
                           const float* wdev, const float* edge_weights, const float* dact, const float* fused,
                           float* dots, float* grad, int B, int H, int W, int C, float* workspace, long long workspace_floats);
int effdet_train_fpn_input_bwd(void* stream, int idx, const float* src, int h, int w, const float* wdev, const float* dact,
                               const float* fused, const float* acc, float* out, int B, int H, int W, int C);

/* ---- optimizer half of the pretrain step (pretrain.py:272-276) ------------------------------------ */

/* torch.nn.utils.clip_grad_norm_(params, max_norm) + torch.optim.Adam.step() on flat float32 buffers.
 * effdet_sqnorm: out[0] (+)= sum(g^2) (two-stage, fixed order; workspace of effdet_sqnorm_workspace_floats floats).
 * effdet_adam_clip_step: g' = g * min(1, max_norm / (sqrt(*sqnorm) + 1e-6)) (sqnorm NULL: no clipping), then Adam
 * in torch's operation order with bias corrections for `step` (1-based). */
long long effdet_sqnorm_workspace_floats(void);
int effdet_sqnorm(void* stream, const float* g, long long n, float* workspace, float* out, int accumulate);
int effdet_adam_clip_step(void* stream, float* p, const float* g, float* m, float* v, long long n,
                          float lr, float beta1, float beta2, float eps, int step, float max_norm, const float* sqnorm);
/* The same with the two bias corrections read from device memory (bc_dev[0] = 1 - beta1^step, bc_dev[1] = sqrt(1 - beta2^step)):
 * the launch can sit in a captured hipGraph while the host refreshes bc_dev before every replay. */
int effdet_adam_clip_step_dev(void* stream, float* p, const float* g, float* m, float* v, long long n,
                              float lr, float beta1, float beta2, float eps, const float* bc_dev, float max_norm, const float* sqnorm);

/* ---- grouped optimizer (group_optim.hip): clip_grad_norm_ per clip domain + torch.optim.Adam / SGD with parameter groups ------
 * Flat float32 buffers of n_floats values (a multiple of 16) for parameters, gradients and state (Adam: state1 = exp_avg,
 * state2 = exp_avg_sq; SGD: state1 = momentum buffer, state2 ignored).  A parameter tensor is a segment: start and padded length
 * multiples of 16 floats, padding zero.  Device tables (int32), built by optim.plan_layout:
 *   pieces     [n_pieces][4]      {offset, length (both in 16-byte units, length <= effdet_group_piece_floats() / 4), segment, 0};
 *                                 a piece lies inside one segment; the first n_norm_pieces pieces are those of the clip domains,
 *                                 domain after domain
 *   seg_group  [n_segments]       group of the segment, -1: in no group (it only contributes to its domain's norm)
 *   dom_ranges [n_domains + 1][4] {first piece, end piece, first segment, end segment} per domain; last row: segments in no domain
 *   dyn        what may change between steps: n_groups rows of 16 words {double lr, beta1, beta2; float weight_decay, eps,
 *              float(1 - beta1), float(beta2), float(1 - beta2), momentum; int nesterov; 3 unused}, then float max_norm[n_domains],
 *              then int present[n_segments]
 * and device state: step [n_segments] int32 (Adam: updates so far; SGD: 1 once the momentum buffer exists), advanced by the
 * kernels; seg_const [n_segments][4] 32-bit words (workspace: three floats and an integer flag word per segment, 16-byte aligned),
 * partial [max(1, n_norm_pieces)], norms [max(1, n_domains)] floats (workspace / output).
 * Per domain: norms[d] = sqrt(sum g^2) over its present segments, coef = min(1, max_norm / (norm + 1e-6)), applied to the gradient
 * value inside the update (the gradient buffer is not modified).  A segment that is not present, or in no group, keeps every byte
 * of its parameters, state and step count.  kind 0: Adam, 1: SGD (momentum, optional Nesterov, dampening 0); both with coupled
 * weight decay, in the operation order of torch's single-tensor paths.  Three launches, fixed-order sums, no atomics, nothing
 * read back: capturable.  effdet_group_norms: the norms alone (needs n_domains > 0). */
long long effdet_group_piece_floats(void);
int effdet_group_norms(void* stream, const float* grad, long long n_floats, const int* pieces, int n_pieces, int n_norm_pieces,
                       const int* seg_group, int n_segments, const int* dom_ranges, int n_domains, const int* dyn, int n_groups,
                       float* partial, float* norms);
int effdet_group_step(void* stream, int kind, float* param, const float* grad, float* state1, float* state2, long long n_floats,
                      const int* pieces, int n_pieces, int n_norm_pieces, const int* seg_group, int n_segments,
                      const int* dom_ranges, int n_domains, const int* dyn, int n_groups, int* step, float* seg_const,
                      float* partial, float* norms);

/* ---- detection evaluation (the effdet/evaluation package, driven by pretrain.py:246-252) ----------------------- */

/* Per-image greedy matching (per_image_evaluation.py:377-405) + CorLoc (:143-176).  det [B,max_det,6] rows
 * x1,y1,x2,y2,score,class (1-based) in descending score order, det_count [B]; gt_boxes [B,M,4] yxyx, gt_cls [B,M]
 * 1-based (<= 0: padding).  tp [B,max_det]: 1 true positive, 0 false positive, -1 dropped (padding row, box with
 * ymax <= ymin or xmax <= xmin, class out of range).  gt_count / gt_imgs / correct_imgs [num_classes] int32 are
 * accumulated (+=): ground-truth instances, images containing the class, images whose top-scoring detection of the
 * class is correctly localised. */
int effdet_eval_match(void* stream, const float* det, const int* det_count, const float* gt_boxes, const long long* gt_cls,
                      int B, int max_det, int M, int num_classes, float iou_threshold,
                      int* tp, int* gt_count, int* gt_imgs, int* correct_imgs);
/* VOC all-points average precision per class (metrics.py:4-90) over n accumulated detections: scores [n], classes [n]
 * 0-based, tp [n] as above; ap [num_classes] float64, NaN for classes without ground truth.  n <= 65536. */
long long effdet_eval_ap_workspace_bytes(int n);
int effdet_eval_ap(void* stream, const float* scores, const int* classes, const int* tp, int n, int num_classes,
                   const int* gt_count, double* ap, void* workspace, long long workspace_bytes);

/* ---- dataset-scale detection evaluation (csrc/eval_scale.hip): sorted AP at up to 16 IoU thresholds, `difficult` flags ------ */

/* effdet_eval_match for `num_thresholds` (1..16) ascending IoU thresholds (a HOST array) and optional `difficult` flags
 * gt_difficult [B,M] bytes (NULL: none).  A detection's candidate is the ground-truth box of its class with the largest IoU
 * (first on ties, difficult boxes included); at threshold t with IoU >= thresholds[t]: candidate difficult -> the detection is
 * ignored at t; candidate free at t -> true positive, the box is taken at t; otherwise false positive.  flags [B,max_det]:
 * bit t = true positive at t, bit 16 + t = ignored at t, bit 31 = dropped (padding row, degenerate box, class outside
 * 1..num_classes, NaN score; with 16 thresholds bit 31 is also `ignored at all of them`, which drops the row just the same).
 * kept (NULL, or [2 B] for effdet_eval_append): slots of image b without bit 31, then its NaN
 * scores.  gt_count [C] (boxes that are not difficult), gt_imgs [C] (images with the class, difficult or not) and
 * correct_imgs [T][C] (CorLoc, difficult boxes count as ground truth) are accumulated (+=).  B * max_det <= 2^24. */
int effdet_eval_match_multi(void* stream, const float* det, const int* det_count, const float* gt_boxes, const long long* gt_cls,
                            const unsigned char* gt_difficult, int B, int max_det, int M, int num_classes,
                            const float* thresholds, int num_thresholds, unsigned int* flags, int* kept,
                            int* gt_count, int* gt_imgs, int* correct_imgs);
/* Appends (score, 0-based class, flag word) of every slot without bit 31 to the `capacity`-sized buffers (<= 2^24) at the device
 * cursor, in (image, slot) order; -0.0 is stored as +0.0.  state: 4 unsigned words on the device, zeroed by the caller to reset:
 * {cursor, entries lost beyond the capacity, NaN scores, 0}.  Two launches; the host reads nothing back. */
int effdet_eval_append(void* stream, const float* det, const unsigned int* flags, const int* kept, int B, int max_det,
                       float* scores, int* classes, unsigned int* out_flags, long long capacity, unsigned int* state);
/* entries one workgroup handles per radix pass */
int effdet_eval_scale_sort_tile(void);
/* pure host queries: workspace size; byte offset in the workspace of the sorted 64-bit keys (which = 0: class << 32 | ~k(score),
 * k = the order-preserving map of the float32 bits) and of their flag words (which = 1) after effdet_eval_ap_sorted; size of the
 * result block */
long long effdet_eval_ap_sorted_workspace_bytes(long long capacity, int num_classes);
long long effdet_eval_ap_sorted_offset(long long capacity, int num_classes, int which);
long long effdet_eval_ap_sorted_result_bytes(int num_thresholds, int num_classes);
/* VOC all-points AP per (threshold, class) over the first n entries (n < 0: min(state[0], capacity), read on the device) without
 * n x n work: a stable radix sort by (class, score descending; equal scores in arrival order), then per class and threshold
 * rank = running count of the entries not ignored, precision = cumulative TP / rank (float64), envelope = maximum over the later
 * entries, AP = sum over the true positives of (recall step) * envelope in a fixed order.  Entries with bit 31, a class outside
 * 0..num_classes-1 or a NaN score take no part.  result: 8-byte words {n, lost, NaN scores, T, C, 0, 0, 0}, AP [T][C] float64
 * (NaN without ground truth, 0 with ground truth and no detection), then int64 gt_count [C], gt_imgs [C], correct_imgs [T][C].
 * num_classes <= 65535.  Capturable; bit-identical from run to run. */
int effdet_eval_ap_sorted(void* stream, const float* scores, const int* classes, const unsigned int* flags, long long capacity,
                          long long n, const unsigned int* state, int num_thresholds, int num_classes, const int* gt_count,
                          const int* gt_imgs, const int* correct_imgs, void* workspace, long long workspace_bytes, void* result);

/* ---- open-set detection evaluation (csrc/eval_scale.hip): unknown recall, A-OSE, wilderness impact ----------------------------
 * `num_classes` counts the unknown class here: the known classes are 1 .. num_classes - 1, the unknown class is U = num_classes,
 * in the ground truth and in the detections; matching is effdet_eval_match_multi with these num_classes. */

/* After effdet_eval_match_multi: open [B,max_det], bit t = the row is kept (no bit 31 in `flags`), its class is known and the
 * largest IoU (the float32 expression of the matching, inter / (area_d + area_g - inter)) between its box and the image's
 * ground-truth boxes of class U, difficult or not, is >= thresholds[t]; 0 for every other row.  One workgroup per image, the
 * unknown boxes staged in static LDS 256 ground-truth rows at a time: any M > 0. */
int effdet_eval_open_words(void* stream, const float* det, const unsigned int* flags, const float* gt_boxes, const long long* gt_cls,
                           int B, int max_det, int M, int num_classes, const float* thresholds, int num_thresholds,
                           unsigned int* open);
/* effdet_eval_append that also appends the open words to out_open at the same positions (one cursor, one count of lost entries
 * and of NaN scores). */
int effdet_eval_append_open(void* stream, const float* det, const unsigned int* flags, const unsigned int* open, const int* kept,
                            int B, int max_det, float* scores, int* classes, unsigned int* out_flags, unsigned int* out_open,
                            long long capacity, unsigned int* state);
/* pure host queries, as for effdet_eval_ap_sorted; which = 2: the sorted open words */
long long effdet_eval_open_sorted_workspace_bytes(long long capacity, int num_classes);
long long effdet_eval_open_sorted_offset(long long capacity, int num_classes, int which);
long long effdet_eval_open_sorted_result_bytes(int num_thresholds, int num_classes);
/* effdet_eval_ap_sorted (the same sort kernels with the open word as a second payload, the same AP kernel: the same bits) over
 * num_classes classes, then one workgroup per (class, threshold) for the open-set counts.  result: the block of
 * effdet_eval_ap_sorted, followed by seven int64 matrices [T][num_classes] over a class's kept entries in sorted order (positions
 * from 0, ctp_p = true positives at positions <= p): n_det (not ignored), tp, open_total (open bit set, ignored or not), and, where
 * the class has ground truth and an entry (otherwise 0, 0, -1, 0, 0): k_star = the cumulative count among those reachable
 * whose recall k / gt_count is nearest recall_level in float64 (ties: the smaller), pos = the first position with ctp = k_star,
 * rank_at / open_at = entries not ignored / with the open bit at positions <= pos.  0 < recall_level <= 1.  Capturable;
 * bit-identical from run to run. */
int effdet_eval_open_sorted(void* stream, const float* scores, const int* classes, const unsigned int* flags,
                            const unsigned int* open, long long capacity, long long n, const unsigned int* state, int num_thresholds,
                            int num_classes, const int* gt_count, const int* gt_imgs, const int* correct_imgs, double recall_level,
                            void* workspace, long long workspace_bytes, void* result);
/* det_out [B,max_det,6] = det_in with the class (column 5) of row (b, j) set to num_known + 1 where j < count[b], the class is in
 * 1..num_known and !(score[b * pitch + j * stride] >= tau) (a NaN score becomes unknown); every other row is copied.  tau is read
 * from tau_device on the device when that is not NULL.  det_out may be det_in.  One launch. */
int effdet_relabel_unknown(void* stream, const float* det_in, const int* count, const float* score, long long pitch,
                           long long stride, int B, int max_det, int num_known, float tau, const float* tau_device, float* det_out);

/* ---- COCO-protocol detection evaluation (csrc/coco_eval.hip): COCOeval 'bbox' with crowd regions, area ranges, AP / AR --------- */

/* COCOeval.evaluateImg for every image, at `num_thresholds` (1..15) ascending IoU thresholds and `num_areas` (1..4) area ranges
 * [lo, hi] (area_ranges [num_areas][2], inclusive), both HOST arrays.  det / det_count / gt_boxes / gt_cls as effdet_eval_match;
 * gt_crowd [B,M] bytes (NULL: none), gt_area [B,M] float32 (NULL: the float32 box area).  A slot is dropped when it lies beyond
 * the count, its box is degenerate, its class is outside 1..num_classes, its score is NaN or < min_score, or its 0-based rank
 * among the kept slots of its class in the image is >= max_rank (the largest max_dets).  Per (t, a) a detection takes, among the
 * boxes of its class, the one not ignored at a (crowd, or area outside the range) and not taken at (t, a) with the largest IoU
 * >= thresholds[t], the last on equal IoU; if there is none, the ignored box by the same rule (a crowd box, IoU = intersection /
 * detection area, can be matched any number of times).  flags [B,max_det,num_areas]: bit t = true positive, bit 16 + t = ignored
 * (matched to an ignored box, or unmatched with its own box area outside the range), bit 31 = dropped; rank [B,max_det] (-1:
 * dropped); kept (NULL, or [2 B] for effdet_coco_append): kept slots of image b, then its NaN scores; npig [C][num_areas] += the
 * boxes of class c not ignored at a.  40 M + 4 num_classes bytes of LDS <= 64 KiB; B * max_det <= 2^24. */
int effdet_coco_match(void* stream, const float* det, const int* det_count, const float* gt_boxes, const long long* gt_cls,
                      const unsigned char* gt_crowd, const float* gt_area, int B, int max_det, int M, int num_classes,
                      const float* thresholds, int num_thresholds, const float* area_ranges, int num_areas, int max_rank,
                      float min_score, unsigned int* flags, int* rank, int* kept, int* npig);
/* effdet_eval_append for the kept slots of effdet_coco_match: (score, 0-based class, num_areas flag words, rank) to scores, classes,
 * words [capacity][num_areas] and ranks at the device cursor; `state` as there. */
int effdet_coco_append(void* stream, const float* det, const unsigned int* flags, const int* rank, const int* kept, int B, int max_det,
                       int num_areas, float* scores, int* classes, unsigned int* words, int* ranks, long long capacity,
                       unsigned int* state);
/* pure host queries: workspace size; byte offset in the workspace, after effdet_coco_sorted, of the sorted 64-bit keys (which = 0,
 * as effdet_eval_ap_sorted_offset), the entries' indices (1), their flag words [n][num_areas] (2) and ranks (3); size of the result */
long long effdet_coco_sorted_workspace_bytes(long long capacity, int num_classes, int num_areas);
long long effdet_coco_sorted_offset(long long capacity, int num_classes, int num_areas, int which);
long long effdet_coco_sorted_result_bytes(int num_thresholds, int num_classes, int num_areas, int num_max_dets);
/* COCOeval.accumulate over the first n entries (n < 0: min(state[0], capacity), read on the device): the stable radix sort by
 * (class, score descending), then per (t, c, a, m) over the entries with rank < max_dets[m] not ignored at (t, a): rc = tp / npig,
 * pr = tp / ((fp + tp) + 2^-52) in float64, made non-increasing from the right; q[r] = pr at the first entry with rc >= rec_thr[r]
 * (0: none); AP = (q[0] + q[1] + ...) / num_rec, AR = the last rc (0 without entries), both NaN where npig = 0.  max_dets: 1..4
 * ascending ints (HOST); rec_thr: 1..256 ASCENDING float64 on the DEVICE (not checked: another order gives unspecified q, never
 * an access out of bounds).  result: 8-byte words {n, lost, NaN scores, T, C, A, Mx, R}, AP [T][C][A][Mx] float64, AR the same,
 * then int64 npig [C][A].  precision (NULL, or [T][R][C][A][Mx] float64 on the device): q itself, NaN where npig = 0.
 * Capturable; bit-identical from run to run. */
int effdet_coco_sorted(void* stream, const float* scores, const int* classes, const unsigned int* words, const int* ranks,
                       long long capacity, long long n, const unsigned int* state, int num_thresholds, int num_classes, int num_areas,
                       const int* max_dets, int num_max_dets, const double* rec_thr, int num_rec, const int* npig, void* workspace,
                       long long workspace_bytes, void* result, double* precision);

/* ---- LVIS federated detection evaluation (csrc/lvis_eval.hip): per-image category sets, one cap over all categories ------------- */

/* pure host query: the LDS bytes of one effdet_lvis_match workgroup, 40 M + 12 ceil(num_classes / 32) + 8 max_det + 16;
 * -22 for max_det outside 1..2048, M < 1 or num_classes outside 1..65535.  The launch needs it <= 64 KiB. */
long long effdet_lvis_match_lds_bytes(int max_det, int M, int num_classes);
/* LVISEval.evaluate_img for every image: effdet_coco_match without crowd regions, with the det rows IN ANY ORDER and per image
 * neg_cls [B,Kn] / nel_cls [B,Ke] int64 1-based category lists (<= 0 or > num_classes: padding): the categories checked absent and
 * the categories not exhaustively annotated.  neg_cls NULL: every category is judged in every image; nel_cls NULL: no category is
 * not-exhaustive; a non-NULL list may have length 0 (the empty set).  A slot is valid when it lies below the count, its box is not
 * degenerate, its class is in 1..num_classes and its score is neither NaN nor < min_score.  Its image rank r is the number of valid
 * slots of the image with a larger score, or an equal score and a lower index; it is dropped when r >= max_rank (LVIS's cap over
 * ALL categories), and then when its class is neither the class of a box of the image nor in neg_cls.  The kept slots are matched
 * in ascending r by effdet_coco_match's rule; an unmatched detection is ignored at (t, a) when its own box area is outside the
 * range or its class is in nel_cls, else a false positive.  flags / rank (the image rank; -1: dropped) / kept / npig as
 * effdet_coco_match, so effdet_coco_append and effdet_coco_sorted take them as they are.  max_det <= 2048; B * max_det <= 2^24. */
int effdet_lvis_match(void* stream, const float* det, const int* det_count, const float* gt_boxes, const long long* gt_cls,
                      const float* gt_area, int B, int max_det, int M, int num_classes, const float* thresholds, int num_thresholds,
                      const float* area_ranges, int num_areas, int max_rank, float min_score, const long long* neg_cls, int Kn,
                      const long long* nel_cls, int Ke, unsigned int* flags, int* rank, int* kept, int* npig);

/* ---- OpenImages detection evaluation (csrc/openimages_eval.hip): group-of boxes, weighted AP, verified labels, pooled mAP ---------- */

/* pure host query: the LDS bytes of one effdet_openimages_match workgroup,
 * 4 (num_classes + ceil(num_classes / 32) + (3 + num_thresholds) M + 24); -22 for M < 1, num_classes outside 1..65535 or
 * num_thresholds outside 1..15.  The launch needs it <= 64 KiB. */
long long effdet_openimages_match_lds_bytes(int M, int num_classes, int num_thresholds);
/* The matching of effdet_eval_match_multi with group-of boxes, for 1..15 ASCENDING thresholds (HOST array).  gt_group_of [B,M]
 * (NULL: none) marks group-of boxes, gt_difficult [B,M] (NULL: none) difficult ones; labeled_cls [B,K] int64 1-based verified
 * image-level labels (<= 0 or > num_classes: padding; NULL: every class is evaluatable in every image; K may be 0): with a list, a
 * detection whose class is neither the class of a box of its image nor in the list is dropped (bit 31).  Stage 1: the candidate is
 * the box of the class that is NOT group-of with the largest IoU (first on ties); IoU >= thr and difficult: ignored; IoU >= thr and
 * not taken: true positive.  Stage 2: a detection that is neither at thr takes the group-of box of its class with the largest
 * intersection over the detection's own area (first on ties); IoA >= thr: absorbed (bit 16 + t) and the box remembers the largest
 * absorbed score.  flags [B,max_det]: bit t true positive, bit 16 + t ignored or absorbed, bit 31 dropped.  vscore / vflags
 * [B,M,num_thresholds]: slot (j, t) is the virtual entry of group-of box j at threshold t when emit_virtual != 0 and the
 * remembered score is > 0 - vscore = that score, vflags = bit t | the ignore bits of every other threshold | bit 15 - else
 * vscore = 0 and vflags = bit 31.  kept [2 B]: kept detection slots + virtual entries of image b, then its NaN scores.  Integer
 * atomics add to n_plain [C] (boxes neither difficult nor group-of), n_group [C] (group-of, not difficult), gt_imgs [C] and
 * correct_imgs [T][C] (the top-scoring detection of the class reaches thr by IoU with ANY box of the class).  A box that is both
 * difficult and group-of absorbs like a group-of box and is counted in neither.  B * max_det and B * M * num_thresholds <= 2^24. */
int effdet_openimages_match(void* stream, const float* det, const int* det_count, const float* gt_boxes, const long long* gt_cls,
                            const unsigned char* gt_difficult, const unsigned char* gt_group_of, const long long* labeled_cls, int K,
                            int B, int max_det, int M, int num_classes, const float* thresholds, int num_thresholds, int emit_virtual,
                            unsigned int* flags, float* vscore, unsigned int* vflags, int* kept, int* n_plain, int* n_group,
                            int* gt_imgs, int* correct_imgs);
/* effdet_eval_append for that match: per image its kept detection slots in slot order, then its virtual entries in (box,
 * threshold) order (class = the box's), at the device cursor state[0]; state as effdet_eval_append.  Virtual entries count
 * against the capacity. */
int effdet_openimages_append(void* stream, const float* det, const unsigned int* flags, const long long* gt_cls, const float* vscore,
                             const unsigned int* vflags, const int* kept, int B, int max_det, int M, int num_thresholds, float* scores,
                             int* classes, unsigned int* out_flags, long long capacity, unsigned int* state);
/* workspace bytes of effdet_openimages_sorted (pooled != 0: with the buffers of the second sort); -22 for a bad argument */
long long effdet_openimages_sorted_workspace_bytes(long long capacity, int num_classes, int pooled);
/* byte offset in the workspace of the sorted keys (which = 0) and flag words (1) of the class sort, and of the keys (2) and flag
 * words (3) of the pooled sort; keys are (class << 32) | order-preserving score key, the pooled class being 0 (takes part) or 1 */
long long effdet_openimages_sorted_offset(long long capacity, int num_classes, int which);
/* bytes of the result block: 8-byte words {n, lost, NaN scores, T, C, pooled, 0, 0}, AP [T][C] float64, pooled AP [T] float64,
 * then int64 n_plain [C], n_group [C], gt_imgs [C], correct [T][C] */
long long effdet_openimages_sorted_result_bytes(int num_thresholds, int num_classes);
/* The stable radix sort by (class, score descending) and the weighted VOC all-points AP per (threshold, class) over the first n
 * entries (n < 0: min(state[0], capacity), read on the device): num_gt = n_plain + w n_group (w = group_of_weight, finite, >= 0);
 * over the entries not ignored at thr, with a plain and g group true positives (bit 15) at or before an entry, ctp = a + w g,
 * precision = ctp / (ctp + (rank - a - g)), AP = the sum over the true positives of (ctp / num_gt - ctp_before / num_gt) * the
 * envelope of precision; NaN where num_gt = 0.  pooled != 0: the sorted entries are sorted once more by score alone, entries of
 * classes without instances behind the rest, equal scores in (class, arrival) order, and the same AP runs over that one segment
 * with num_gt = the sum over the classes with instances; else the pooled AP is NaN.  Capturable; bit-identical from run to run. */
int effdet_openimages_sorted(void* stream, const float* scores, const int* classes, const unsigned int* flags, long long capacity,
                             long long n, const unsigned int* state, int num_thresholds, int num_classes, double group_of_weight,
                             int pooled, const int* n_plain, const int* n_group, const int* gt_imgs, const int* correct_imgs,
                             void* workspace, long long workspace_bytes, void* result);

/* ---- detection calibration (csrc/calibration_eval.hip): reliability tables, D-ECE / LaECE terms, Platt / temperature fit ---------- */

/* effdet_eval_match_multi (the same flag words, gt_count, gt_imgs and correct_imgs, bit for bit) that also writes iou [B,max_det]:
 * the float32 IoU of the slot's box with its candidate, the box of its class with the largest IoU (lowest index on ties), 0 where
 * the class has no box or the slot is dropped.  kept [2 B] (required): the slots of image b that are not dropped and have
 * score >= score_threshold (not NaN), then its NaN scores.  (num_classes + 3 M + 8) ints of LDS <= 64 KiB. */
int effdet_calibration_match(void* stream, const float* det, const int* det_count, const float* gt_boxes, const long long* gt_cls,
                             const unsigned char* gt_difficult, int B, int max_det, int M, int num_classes, const float* thresholds,
                             int num_thresholds, float score_threshold, unsigned int* flags, float* iou, int* kept, int* gt_count,
                             int* gt_imgs, int* correct_imgs);
/* effdet_eval_append for that match and the same score_threshold: (score, 0-based class, flag word, IoU) of the kept slots to
 * scores, classes, out_flags and out_iou at the device cursor; `state` as there. */
int effdet_calibration_append(void* stream, const float* det, const unsigned int* flags, const float* iou, const int* kept, int B,
                              int max_det, float score_threshold, float* scores, int* classes, unsigned int* out_flags,
                              float* out_iou, long long capacity, unsigned int* state);
/* pure host queries: workspace bytes of effdet_calibration_table; byte offset in it of the sorted keys (which = 0), flag words (1)
 * and IoU (2) of the class sort and of the same three of the pooled sort (3, 4, 5); bytes of the result block, -22 unless
 * 1 <= num_thresholds <= 16, 1 <= num_classes <= 65535, 1 <= bins <= 64 and num_thresholds (num_classes + 1) bins <= 2^20 */
long long effdet_calibration_workspace_bytes(long long capacity, int num_classes);
long long effdet_calibration_sorted_offset(long long capacity, int num_classes, int which);
long long effdet_calibration_result_bytes(int num_thresholds, int num_classes, int bins);
/* The stable radix sort by (class, score descending, arrival) of the first n entries (n < 0: min(state[0], capacity), read on the
 * device) with flag word and IoU as payload, the same sort again by score alone (scope `pooled`), then per (threshold t, scope s
 * = class 0 .. C-1 or pooled = C, scheme, bin k) over the bin's entries not ignored at t: n, tp, sum_p, sum_iou (over the true
 * positives).  Scheme 0 (width): k = min(bins - 1, max(0, (int)(p * (float)bins))); scheme 1 (mass): the sorted positions
 * [floor(k m / bins), floor((k + 1) m / bins)) of the scope's m entries.  result: 8-byte words {n, lost, NaN scores, T, C, bins, 0,
 * 0}; n, tp (int64), sum_p, sum_iou (float64) [T][C+1][2][bins] each; brier, nll (float64), out_of_range, entries (int64)
 * [T][C+1] each; int64 gt_count [C], gt_imgs [C], correct [T][C].  Every float64 sum is taken in an order that depends on the
 * sorted positions alone (calibration_eval.hip's header).  Capturable; bit-identical from run to run. */
int effdet_calibration_table(void* stream, const float* scores, const int* classes, const unsigned int* flags, const float* iou,
                             long long capacity, long long n, const unsigned int* state, int num_thresholds, int num_classes, int bins,
                             const int* gt_count, const int* gt_imgs, const int* correct_imgs, void* workspace,
                             long long workspace_bytes, void* result);
/* bytes of the partial sums of effdet_calibration_fit_step: 64 per 2048 entries of the capacity */
long long effdet_calibration_fit_workspace_bytes(long long capacity);
/* One iteration (two launches) of the damped Newton fit of p' = sigmoid(a logit(p~) + b) over the appended, unsorted entries that
 * are not ignored at threshold_index, target tp (soft_target = 0) or tp ? IoU : 0; temperature != 0 keeps b = 0.  fit_state: 16
 * float64 on the device {a, b, NLL, trial a, trial b, step scale, direction a, b, first NLL, evaluations, halvings, converged,
 * frozen, has an accepted point, entries used, 0}, started as {1, 0, 0, 1, 0, 1, 0 ...}.  A frozen state (converged, or given
 * up) makes the launches exit at once.  Nothing is read back; capturable. */
int effdet_calibration_fit_step(void* stream, const float* scores, const unsigned int* flags, const float* iou, long long capacity,
                                const unsigned int* state, int threshold_index, int soft_target, int temperature, double* fit_state,
                                void* workspace, long long workspace_bytes);
/* det_out [B,max_det,6] = det_in with the score (column 4) of row (b, j), j < count[b], replaced by
 * float32(sigmoid(a logit(p~) + b)) in float64, (a, b) = fit_state[0], fit_state[1] read on the device, p~ = the score clamped
 * to [2^-24, 1 - 2^-24]; a NaN score stays NaN.  det_out may be det_in.  One launch. */
int effdet_calibration_apply(void* stream, const float* det_in, const int* count, const double* fit_state, int B, int max_det,
                             float* det_out);

/* ---- OOD evaluation helpers -------------------------------------------- */

/* The fork's novelty score (infer.py:425-427, 465-471, 607-616), reported beside energy / max-logit:
 * embds [n,d] fp32 = ProjectionNet outputs (normalised inside, F.normalize p=2), confs [n] = anchor confidences (logits),
 * proto_idx [m] int64 = rows of embds that form the cluster (`max_idxs` of the episode code).
 * soft_thresh = sigmoid(dot_mult * (conf + dot_add)); sim = mean_j (use_max = 0) or max_j (use_max = 1) of the cosine
 * similarity to the prototypes; score = soft_thresh * sim.  m * d <= 16384.
 * A proto_idx entry outside [0, n) is never dereferenced: every row of `score` and `sim` then comes back NaN (checked on
 * the device, no host synchronisation; `soft_thresh` stays valid). */
int effdet_novelty_score(void* stream, const float* embds, const float* confs, const long long* proto_idx, int n, int d, int m,
                         float dot_mult, float dot_add, int use_max, float* score, float* soft_thresh, float* sim);

/* Image-level OOD score out[b] = max_a(-energy[b, a]) over the per-anchor energies [B, N]. */
int effdet_ood_image_score(void* stream, const float* energy, int B, long long N, float* out);
/* AUROC of in-distribution scores `pos` against OOD scores `neg` by exact pair counting:
 * counts[0] = #{(i,j): pos_i > neg_j}, counts[1] = #{pos_i == neg_j};  AUROC = (counts[0] + counts[1]/2) / (n_pos*n_neg). */
int effdet_auroc_counts(void* stream, const float* pos, const float* neg, int n_pos, int n_neg, unsigned long long* counts);

/* ---- detection-level OOD evaluation (csrc/ood_eval.hip): AUROC, AUPR in / out, FPR at a TPR level ----
 * Two multisets of float32 scores, pos (in-distribution, the positive class) and neg (OOD); higher = more in-distribution.
 * Each side is a flat device buffer of `capacity` floats (<= 2^27) filled from a device cursor; `state` is 4 unsigned words
 * on the device, zeroed by the caller to reset: {pos cursor, pos flags, neg cursor, neg flags}, side flags 1 = a NaN was
 * appended, 2 = the capacity overflowed (the surplus was dropped).  No call below synchronises with the host or allocates, so
 * all of them can be captured in a graph; the workspace (size from the query, pure host code like the tile query) is shared
 * by all three and must not be used by anything else between the sort and the metrics call. */
long long effdet_ood_eval_workspace_bytes(long long capacity_pos, long long capacity_neg);
/* keys one workgroup handles per radix pass */
int effdet_ood_eval_sort_tile(void);
/* byte offset in the workspace of the sorted float32 scores of side 0 (pos) / 1 (neg) after the sort call (pure host code) */
long long effdet_ood_eval_sorted_offset(long long capacity_pos, long long capacity_neg, int side);
/* Appends the kept entries of the [B, K] matrix scores[b * pitch + j * stride] to `buffer` in (b, j) order: entry (b, j) is
 * kept when j < count[b] (count NULL: all K; int32, or int64 when count_is_int64) and, with det_score != NULL, when
 * det_score[b * det_pitch + j * det_stride] >= min_score.  negate: the value is stored negated (energy -> score).  -0.0 is
 * stored as +0.0.  side_state = state + 2 * side.  B * K <= 2^27.  Three launches: counts, bases, writes. */
int effdet_ood_eval_append(void* stream, const float* scores, long long pitch, long long stride, int B, int K,
                           const void* count, int count_is_int64, const float* det_score, long long det_pitch,
                           long long det_stride, float min_score, int negate, float* buffer, long long capacity,
                           unsigned int* side_state, void* workspace, long long workspace_bytes);
/* Sorts both sides (keys only, 4 radix passes of histogram / scan / scatter launches); the buffers are left as they are. */
int effdet_ood_eval_sort(void* stream, const float* pos, long long capacity_pos, const float* neg, long long capacity_neg,
                         const unsigned int* state, void* workspace, long long workspace_bytes);
/* After the sort: result = 12 words of 8 bytes {P, N, pairs_gt, pairs_eq, tp, fp, flags, k} as uint64, {aupr_in, aupr_out}
 * as float64, the float32 threshold in the low half of word 10, 0.  flags = pos side flags | neg side flags << 2 | 16 (pos
 * empty) | 32 (neg empty).  The threshold is the k-th largest positive, k the smallest integer with k / P >= level (float64
 * division); tp / fp count the positives / negatives >= it.  0 < level <= 1.  Two launches; bit-identical from run to run. */
int effdet_ood_eval_metrics(void* stream, long long capacity_pos, long long capacity_neg, const unsigned int* state,
                            void* workspace, long long workspace_bytes, double level, void* result);

/* ---- feature-space OOD scores (csrc/feature_ood.hip): Mahalanobis distance with a tied covariance, and its relative form ----
 * Rows are features of the BiFPN pyramid, read through a level table of num_levels (<= 8) host arrays: level l holds
 * level_cells[l] cells; the F channels (float32 or bfloat16, dtype = EFFDET_F32 / EFFDET_BF16; channel stride 1, anything else
 * is refused) of cell p of image b start at level_bases[l] + b * level_batch_strides[l] + p * level_cell_strides[l] (elements).
 * P = sum of the cell counts, B * P <= 2^31.  Row (b, j), j < K, is anchor anchor_index[b * K + j] (int64; NULL: anchor j) and
 * sits on cell anchor / A; it counts when j < count[b] (NULL: all K; int32, or int64 when count_is_int64) and the anchor lies in
 * [0, A * P).  F is one of 64, 88, 112, 160, 224, 288; 1 <= C <= 1024; B * K <= 2^27.  Bad arguments return -22 before any
 * launch.  No call synchronises with the host or allocates; results are bit-identical from run to run. */
/* bytes of the fit workspace for `rows` = B * K rows of width F (pure host code; -22 for a bad argument) */
long long effdet_feature_ood_workspace_bytes(long long rows, int F);
/* Adds the valid rows to the running statistics n_c [C] int64, s_c [C][F] float64 (sum of the rows of a class) and S [F][F]
 * float64 (sum of f f^T over all valid rows).  The class of row (b, j) is classes[b * class_pitch + j * class_stride] -
 * class_offset (class_dtype 0: int32, 1: int64, 2: float32, truncated); a row whose class lies outside [0, C) is skipped.
 * Six launches: valid-row counts, bases, compaction in (b, j) order, S partials over 16 fixed row chunks, their sum in chunk
 * order added to S, one workgroup per class for s_c / n_c.  No floating-point atomics. */
int effdet_feature_ood_fit(void* stream, int dtype, int num_levels, const void* const* level_bases, const long long* level_cells,
                           const long long* level_batch_strides, const long long* level_cell_strides,
                           const long long* level_channel_strides, int F, int C, int A, int B, long long K,
                           const long long* anchor_index, const void* classes, int class_dtype, long long class_pitch,
                           long long class_stride, long long class_offset, const void* count, int count_is_int64,
                           long long* n_c, double* s_c, double* S, void* workspace, long long workspace_bytes);
/* Scores every row in float32: xc = f - mu0, z = W xc, z0 = W0 xc, d_c = |z|^2 - 2 z.M_c + m2_c,
 * mahalanobis = -min_c d_c, relative = -(min_c d_c - |z0|^2), nearest = argmin_c d_c (ties to the lower class).  With
 * Fp = F rounded up to 16 and Cp = C rounded up to 32: W, W0 [Fp][Fp] and M [Cp][Fp] row-major and mu0 [Fp], zero in the padding;
 * m2 [Cp], +inf for the padding and for classes without rows.  Outputs [B][K]: float32, float32, int32; a row that does not
 * count holds 0, 0, -1.  The products run on the float32-input MFMA.  One launch. */
int effdet_feature_ood_score(void* stream, int dtype, int num_levels, const void* const* level_bases, const long long* level_cells,
                             const long long* level_batch_strides, const long long* level_cell_strides,
                             const long long* level_channel_strides, int F, int C, int A, int B, long long K,
                             const long long* anchor_index, const void* count, int count_is_int64, const float* W,
                             const float* W0, const float* M, const float* m2, const float* mu0, float* mahalanobis,
                             float* relative, int* nearest);

/* ---- nearest-neighbour feature OOD score (csrc/feature_knn.hip): a bank of pyramid rows and the k-th nearest of them ----------
 * Rows are addressed as above (level table, anchor_index, count, A).  The bank is bank [capacity][Fp] float32 (Fp = F rounded up
 * to 16, zero in the padding), norms [capacity] float32 (|r|^2 of the stored values), bank_classes [capacity] int32 and counters
 * [3] int64 = {size, seen, lost}, all zero after a clear.  |x|^2 is summed in one fixed order everywhere: 16 partial sums over
 * k mod 16 (k ascending), then the tree (p[j] + p[j + 8]), (.. + 4), (.. + 2), (.. + 1).  1 <= k <= 32, capacity <= 2^24,
 * B * K <= 2^27, 0 <= splits <= 64.  Bad arguments return -22 before any launch.  No call synchronises with the host or
 * allocates; no floating-point atomics; results are bit-identical from run to run. */
/* bytes of the workspace for `rows` = B * K rows: of append when k = 0, of score with k and `splits` (0: the most the library may
 * choose for these rows) otherwise (pure host code; -22 for a bad argument) */
long long effdet_feature_knn_workspace_bytes(long long rows, int F, int k, int splits);
/* Adds valid rows to the bank in (b, j) order.  A row is valid when j < count[b], its class (as in effdet_feature_ood_fit; C = 0:
 * no classes, `classes` may be NULL and -1 is stored) lies in [0, C) and its anchor in [0, A * P).  The valid row with global
 * ordinal g - counted in `seen` since the counters were cleared, across calls - is kept when g % sample_every == 0; kept rows
 * beyond `capacity` are dropped and counted in `lost`.  normalize != 0 stores r * (1 / sqrt(max(|r|^2, 1e-24))).  Four
 * launches: valid-row counts, bases and the counter update in one workgroup, the bank row of every entry, the rows. */
int effdet_feature_knn_append(void* stream, int dtype, int num_levels, const void* const* level_bases, const long long* level_cells,
                              const long long* level_batch_strides, const long long* level_cell_strides,
                              const long long* level_channel_strides, int F, int C, int A, int B, long long K,
                              const long long* anchor_index, const void* classes, int class_dtype, long long class_pitch,
                              long long class_stride, long long class_offset, const void* count, int count_is_int64,
                              int normalize, long long sample_every, long long capacity, float* bank, float* norms,
                              int* bank_classes, long long* counters, void* workspace, long long workspace_bytes);
/* For every row q (normalised like the bank rows when normalize != 0) and the bank rows r_i, i < M (1 <= M <= 2^24):
 * d2_i = max((|q|^2 + |r_i|^2) - 2 q.r_i, 0) in float32, q.r_i on the float32-input MFMA.  knn [B][K] float32 = minus the
 * min(k, M)-th smallest d2; knn_index [B][K] int32 = the lexicographic minimum of (d2, i); knn_class its class; a row that does
 * not count holds 0, -1, -1.  The bank is walked in `splits` parts (0: chosen by the library); the outputs are bit-identical
 * for every split count.  Two launches. */
int effdet_feature_knn_score(void* stream, int dtype, int num_levels, const void* const* level_bases, const long long* level_cells,
                             const long long* level_batch_strides, const long long* level_cell_strides,
                             const long long* level_channel_strides, int F, int A, int B, long long K,
                             const long long* anchor_index, const void* count, int count_is_int64, int normalize, int k,
                             int splits, long long M, const float* bank, const float* norms, const int* bank_classes,
                             float* knn, int* knn_index, int* knn_class, void* workspace, long long workspace_bytes);

/* ---- subspace OOD scores (csrc/feature_subspace.hip): residual norm, partial Mahalanobis distance and ViM ----------------------
 * Rows are addressed as above (level table, anchor_index, count, A).  With Fp = F rounded up to 16 and Rp = the number of
 * residual directions rounded up to 16 (16 <= Rp <= Fp): Rt [Rp][Fp] row-major holds the directions as rows, inv_lambda [Rp] their
 * weights and mu0 [Fp] the origin, all float32 and zero in the padding.  Per row, in float32: xc = f - mu0, y = Rt xc on the
 * float32-input MFMA, r = sqrt(sum_i y_i^2), pm = sum_i inv_lambda_i * y_i^2 (each sum in one fixed order that depends on Rp
 * alone), t = logit_score[b * ls_pitch + j * ls_stride] (elements), negated when negate != 0.  B * K <= 2^27.  Bad arguments
 * return -22 before any launch.  No call synchronises with the host or allocates; no floating-point atomics; results are
 * bit-identical from run to run and do not depend on how the rows are grouped into calls. */
/* residual [B][K] = -r, partial [B][K] = -pm and, when vim is not NULL (logit_score must then be given), vim [B][K] =
 * t - alpha * r (the product rounded, then the difference); a row that does not count holds 0 in each.  One launch. */
int effdet_feature_subspace_score(void* stream, int dtype, int num_levels, const void* const* level_bases, const long long* level_cells,
                                  const long long* level_batch_strides, const long long* level_cell_strides,
                                  const long long* level_channel_strides, int F, int A, int B, long long K,
                                  const long long* anchor_index, const void* count, int count_is_int64, const float* Rt,
                                  const float* inv_lambda, const float* mu0, int Rp, const float* logit_score, long long ls_pitch,
                                  long long ls_stride, int negate, float alpha, float* residual, float* partial, float* vim);
/* Adds, over the rows that count: their number to counters[0] (int64), sum t to sums[0] and sum r to sums[1] (float64), r being
 * bit-equal to the score's.  A workgroup adds its rows in (b, j) order to one partial in the workspace; one workgroup then adds
 * the partials in workgroup order.  Two launches. */
int effdet_feature_subspace_calibrate(void* stream, int dtype, int num_levels, const void* const* level_bases,
                                      const long long* level_cells, const long long* level_batch_strides,
                                      const long long* level_cell_strides, const long long* level_channel_strides, int F, int A, int B,
                                      long long K, const long long* anchor_index, const void* count, int count_is_int64,
                                      const float* Rt, const float* mu0, int Rp, const float* logit_score, long long ls_pitch,
                                      long long ls_stride, int negate, long long* counters, double* sums, void* workspace,
                                      long long workspace_bytes);
/* bytes of the calibrate workspace for `rows` = B * K rows (pure host code; -22 for a bad argument) */
long long effdet_feature_subspace_workspace_bytes(long long rows);

/* ---- logit-space OOD scores (csrc/logit_ood.hip): MSP, entropy, GEN, JointEnergy, KL matching, standardized max logit ----------
 * Rows are the C class logits (float32 or bfloat16, dtype = EFFDET_F32 / EFFDET_BF16, class stride 1) of anchor n of image b at
 * logits + b * image_stride + n * anchor_stride (elements, both >= 0), n < N <= 2^31.  Row (b, j), j < K, is anchor
 * anchor_index[b * K + j] (int64; NULL: anchor j); it counts when j < count[b] (NULL: all K; int32, or int64 when count_is_int64)
 * and the anchor lies in [0, N).  1 <= C <= 1024, B * K <= 2^27, temperature > 0.  Bad arguments return -22 before any launch.
 * No call synchronises with the host or allocates; no floating-point atomics; results are bit-identical from run to run and a
 * row's scores do not depend on how the rows are grouped into calls. */
/* Per row in float32, with u = z / temperature, m = max u, k* the lowest argmax, e_k = exp(u_k - m), s = sum e, lse = m + log s,
 * l_k = u_k - lse, p_k = exp(l_k):  msp = exp(m - lse);  neg_entropy = sum p_k l_k;  gen = -sum over the top_m largest u_k (equal
 * values: the lower k first; top_m >= C: all) of exp(gamma * (l_k + q_k)), q_k = log1p(-p_k) for k != k* and
 * log(sum_{k != k*} e_k) - log s for k*;  joint_energy = sum max(z_k, 0) + log1p(exp(-|z_k|));  predicted_class = k* (int64).
 * With Cp = C rounded up to 16 and the fitted parameters log_d [Cp][Cp] (row c: log of template c; zero in the padding and in
 * classes without rows), kl_inf [Cp] (0, or +inf for the padding and for classes without rows), mu [C], inv_sigma [C] - all
 * NULL or all given, together with their three outputs:  kl_c = (neg_entropy - sum_k p_k log_d[c][k]) + kl_inf[c] with p and
 * neg_entropy taken at temperature 1, the product on the float32-input MFMA;  kl_matching = -min_c kl_c;  kl_class = argmin
 * (ties to the lower class);  standardized = (max z - mu[k*]) * inv_sigma[k*].  Outputs [B][K]; a row that does not count holds
 * 0 in the float outputs and -1 in the class outputs.  One launch. */
int effdet_logit_ood_score(void* stream, int dtype, const void* logits, long long image_stride, long long anchor_stride, int C, int B,
                           long long N, long long K, const long long* anchor_index, const void* count, int count_is_int64,
                           float temperature, float gamma, int top_m, const float* log_d, const float* kl_inf, const float* mu,
                           const float* inv_sigma, float* msp, float* neg_entropy, float* gen, float* joint_energy,
                           long long* predicted_class, float* kl_matching, long long* kl_class, float* standardized);
/* Adds the rows that count (and, when use_min != 0, whose max z >= min_max_logit) to the running statistics of their predicted
 * class c: n_c [C] int64, P_c [C][C] float64 (sum of p at temperature 1), a_c [C] and b_c [C] float64 (sum of max z and of its
 * square).  The valid rows are compacted in (b, j) order; workgroup (c, s) adds the rows of class c of chunk s of that list in list
 * order to a float64 partial, the chunks are added in chunk order and then to the statistics: the order depends on the number of
 * valid rows and C alone.  Six launches. */
int effdet_logit_ood_fit(void* stream, int dtype, const void* logits, long long image_stride, long long anchor_stride, int C, int B,
                         long long N, long long K, const long long* anchor_index, const void* count, int count_is_int64,
                         float temperature, int use_min, float min_max_logit, long long* n_c, double* P_c, double* a_c, double* b_c,
                         void* workspace, long long workspace_bytes);
/* bytes of the fit workspace for `rows` = B * K rows of C classes (pure host code; -22 for a bad argument) */
long long effdet_logit_ood_workspace_bytes(long long rows, int C);

/* ---- activation-shaping OOD scores (csrc/act_shaping.hip): ReAct, ASH-P / ASH-B / ASH-S, SCALE, GradNorm -------------------------
 * The class tower - the input of class_net.predict.conv_dw - is addressed by a level table as above (float32 or bfloat16, channel
 * stride 1, F in {64, 88, 112, 160, 224, 288}) with level_heights / level_widths (host int arrays; height * width = the level's
 * cells, a cell is y * width + x).  taps [9][F] float32 (k = 3 ky + kx).  With Cp = C rounded up to 16 and Fp = F rounded up to 16
 * the pointwise weight W [A * C][F] comes packed per anchor slot a: w_rows [A][F][Cp] (w_rows[a][j][c] = W[a C + c][j]) for the
 * entries form, w_tiles [A][Cp][Fp] for the cells form, bias [A][Cp] for both; zero in the padding of the weights, -inf in that of
 * the bias.  1 <= C <= 1024, A >= 1, B * K <= 2^27.
 * Penultimate row of a cell in float32 (bfloat16 widened exactly), every product and every sum rounded once:
 *   d_j = t_0j x_0j, then d_j = d_j + t_kj x_kj for k = 1 .. 8, x_k the tower value at (y + ky - 1, x + kx - 1), 0 outside the map.
 * Shaping d -> x', method 0 none: x' = d;  1 react: x'_j = min(d_j, react_c[0]) (device memory);  with the kept set = the k largest
 * d_j by value (1 <= k <= F; equal values: the lower j first), s1 = sum_j max(d_j, 0), s2 = the same over the kept set and
 * f = exp(s1 / s2) (1 where s2 == 0):  2 ash_p: kept d_j, others 0;  3 ash_b: kept s1 / k, others 0;  4 ash_s: kept d_j f, others 0;
 * 5 scale: d_j f for every j.  s1, s2: a lane's channels t, t + 64, .. ascending, then the lanes by the xor tree 32 .. 1.
 * Logits of anchor slot a: z_c = bias[a][c] + sum_j W[a C + c][j] x'_j, u = z / temperature (> 0):
 *   energy = -(temperature * logsumexp(u)),  max_logit = max z,  predicted_class = the lowest argmax (int64),
 *   gradnorm (NULL: not wanted) = (sum_c |p_c - 1 / C|) * (sum_j |d_j|), p the softmax at temperature 1 of the logits of the
 *   unshaped row d.  A row with a non-finite d_j scores NaN in the float outputs and -1 in the class output.
 * A row's scores are not bit-equal between the entries and the cells form.  Bad arguments return -22 before any launch.  No call
 * synchronises with the host or allocates; no floating-point atomics; results are bit-identical from run to run and a row's
 * (a cell's) scores do not depend on how rows (cells) are grouped into workgroups or calls. */
/* bytes of the fit workspace for `rows` = B * K rows (pure host code; -22 for a bad argument) */
long long effdet_act_shaping_workspace_bytes(long long rows, int F);
/* Entries form.  Row (b, j) is the cell anchor / A and the slot anchor % A of anchor = anchor_index[b * K + j] (NULL: j); it counts
 * when j < count[b] (NULL: all) and the anchor lies in [0, A * P).  Outputs [B][K]; a row that does not count holds 0 in the float
 * outputs and -1 in the class output.  rows (NULL: not wanted) [B][K][F] float32 receives x' (NaN for a non-finite row, 0 for a
 * row that does not count).  One wave per row, sum_j a float64 fma chain with j ascending, rounded to float32 once.  One launch. */
int effdet_act_shaping_score(void* stream, int dtype, int num_levels, const void* const* level_bases, const long long* level_cells,
                             const long long* level_batch_strides, const long long* level_cell_strides,
                             const long long* level_channel_strides, const int* level_heights, const int* level_widths, int F, int C,
                             int A, int B, long long K, const long long* anchor_index, const void* count, int count_is_int64,
                             const float* taps, const float* w_rows, const float* bias, int method, int k, const float* react_c,
                             float temperature, float* energy, float* max_logit, long long* predicted_class, float* gradnorm,
                             float* rows);
/* Cells form: every anchor of every cell, outputs [B][A * P] at index cell * A + a (the head's anchor order).  The shaped row is
 * formed once per cell; the [16 cells x Fp] by [Fp x Cp] products run on the float32-input MFMA (K-chunk c of 16 into accumulator
 * c mod 4, then (a0 + a1) + (a2 + a3)), the log-sum-exp is kept online in
 * registers over the class tiles ascending and combined over the 16 lanes of a row by the xor tree 1 .. 8.  One launch. */
int effdet_act_shaping_score_cells(void* stream, int dtype, int num_levels, const void* const* level_bases, const long long* level_cells,
                                   const long long* level_batch_strides, const long long* level_cell_strides,
                                   const long long* level_channel_strides, const int* level_heights, const int* level_widths, int F,
                                   int C, int A, int B, const float* taps, const float* w_tiles, const float* bias, int method, int k,
                                   const float* react_c, float temperature, float* energy, float* max_logit,
                                   long long* predicted_class, float* gradnorm);
/* Fit statistics over the rows that count (selected as in the entries form) and whose d is finite: their number onto n [1] int64,
 * sum d onto sum_d [F] float64 - the rows compacted in (b, j) order; workgroup s of 256 adds chunk s of that list (wave w the rows
 * w, w + 4, .. in list order, then the waves in order), one workgroup adds the chunks in chunk order: the order follows from the
 * number of such rows alone - and every d_j onto hist [65536] int64 at the upper 16 bits of its order-preserving key (bits ^ 2^31
 * for a cleared sign bit, ~bits otherwise; integer atomics).  Six launches. */
int effdet_act_shaping_fit(void* stream, int dtype, int num_levels, const void* const* level_bases, const long long* level_cells,
                           const long long* level_batch_strides, const long long* level_cell_strides,
                           const long long* level_channel_strides, const int* level_heights, const int* level_widths, int F, int A,
                           int B, long long K, const long long* anchor_index, const void* count, int count_is_int64, const float* taps,
                           long long* n, double* sum_d, long long* hist, void* workspace, long long workspace_bytes);

/* ---- energy-margin OOD training losses (csrc/energy_reg.hip): energy-bounded hinge and logistic uncertainty loss, with gradients --
 * Rows are the C class logits (float32 or bfloat16, dtype = EFFDET_F32 / EFFDET_BF16) of a contiguous [B][N][C] tensor, role [B][N]
 * int8: 1 = in-distribution, 0 = outlier, anything else = the row does not count and is not read.  1 <= C <= 1024, B * N <= 2^27.
 * energy_kind 0 (logsumexp): mz = max z, m = mz / temperature, s = sum_k exp(z_k / temperature - m), E = -(temperature * (m + log s));
 * energy_kind 1 (joint, temperature must be 1): E = -sum_k (max(z_k, 0) + log1p(exp(-|z_k|))).  With use_min != 0 an outlier row
 * counts only when mz >= min_max_logit (a row that holds a NaN does not pass).
 * form 0 (hinge): l_in = max(0, E - margin_in)^2, l_out = max(0, margin_out - E)^2;  form 1 (logistic, phi = (w, b) on the device):
 * sv = w * (-E) + b, l_in = softplus(-sv), l_out = softplus(sv).  E, its derivative and grad_logits are float32 in that order; the
 * terms of the sums over rows are evaluated in float64 - the hinge's l from the float32 max(0, .), the logistic l and dl/dsv from
 * the float32 m and s of the log-sum-exp (E once more as -(temperature * (m + log s)) in float64) or from the float32 joint energy -
 * and added in float64 in an order that follows from B * N alone (no floating-point atomics).
 *   loss [1] float32 = c_in * sum_in l + c_out * sum_out l,  c_side = weight_side / max(n_side, 1);
 *   stats [8] float64 = n_in, n_out, mean l in / out, mean E in / out, rows with a positive hinge in / out (0 for form 1);
 *   energy [B][N] float32 or NULL: E, 0 where the row does not count;
 *   grad_logits [B][N][C] in the logits' dtype or NULL: d loss / d z, zero in every row that does not count;
 *   grad_phi [2] float32: d loss / d (w, b) (0 for form 0).
 * Bad arguments return -22 before any launch.  No call synchronises with the host or allocates; three launches, four with
 * grad_logits; results are bit-identical from run to run. */
int effdet_energy_reg(void* stream, int dtype, const void* logits, const signed char* role, int B, long long N, int C, int form,
                      int energy_kind, float temperature, float margin_in, float margin_out, float weight_in, float weight_out,
                      int use_min, float min_max_logit, const float* phi, float* loss, double* stats, float* energy,
                      void* grad_logits, float* grad_phi, void* workspace, long long workspace_bytes);
/* bytes of the workspace for `rows` = B * N rows (pure host code; -22 for a bad argument) */
long long effdet_energy_reg_workspace_bytes(long long rows);

/* ---- von Mises-Fisher hyperspherical OOD head (csrc/vmf.hip; SIREN, Du et al. 2022) ------------------------------------------------
 * U [B][P][d] float32 (contiguous) is the embedding of every pyramid cell, 2 <= d <= 256; prototypes [C][d] float32 and valid [C]
 * int32 are the unit class means and whether a class has received a row; 1 <= C <= 1024.  A dense label map [B][K = A * P]
 * (classes_dtype 0 int32, 1 int64, 2 float32; element (b, j) at b * pitch + j * stride) names the class of anchor j, which sits on
 * cell j / A; an entry counts when its label less class_offset lies in [0, C) and its cell's row holds finite values only.
 *   n = max(sqrt(sum u_k^2), 1e-12), r = u / n        (float32; lane t of 64 adds elements t, t + 64, .. then the xor tree 32 .. 1)
 * effdet_vmf_partition: theta [C] float32 -> kappa = float32(exp(clamp(theta, log 2^-7, log 2^13))) [C] float32, logZ [C] float32
 *   and float64, logZ = (d / 2 - 1) log kappa - (d / 2) log(2 pi) - log I_{d/2-1}(kappa), ratio [C] float64 = I_{d/2} / I_{d/2-1}
 *   at kappa, clamped [C] int32 = 1 where theta lies outside the clamp (or is a NaN).  Float64 on the device, a thread per class.
 * effdet_vmf_update: per class c, its counted rows in (b, j) order, at most rows_per_class of them (0: all):
 *   v = alpha * mu_c + (1 - alpha) * r, mu_c = v / max(|v|, 1e-12); valid[c] = 1 once a row arrived.  0 <= alpha <= 1.
 * effdet_vmf_loss: over the entries that count and whose class is valid, l_c = logZ_c + kappa_c (mu_c . r) over the valid classes,
 *   loss [1] float32 = (1 / max(m, 1)) sum_i (logsumexp_c l_ic - l_iy), dU [B][P][d] float32 = d loss / d U (zero in every other cell;
 *   the counted anchors of a cell added in ascending order), dtheta [C] float32 = d loss / d theta (0 where clamped),
 *   stats [8] float64 = m, rows skipped as non-finite, valid classes, mean mu_y . r, mean kappa, max kappa, the loss in float64, 0.
 *   The prototypes are constants.  Sums over rows are float64 in an order that follows from B * K alone.
 * effdet_vmf_score: entry (b, j) of a [B][K] call is the cell anchor_index[b][j] / A (NULL: j / A) and counts when j < count[b]
 *   (NULL: all) and the anchor lies in [0, A * P); gathered != 0: U is [B][K][d], the row of entry (b, j) is row j.  vmf = max_c l_c,
 *   vmf_class (int64) the lowest class that attains it, vmf_cosine = max_c mu_c . r; 0, -1, 0 for an entry that does not count or
 *   without a valid class; NaN, -1, NaN for a non-finite row.  rows [B][K][d] or NULL: r (zeros where the entry does not count).
 * effdet_vmf_gather: out [B * K][F] float32 = the tower rows (level table as in effdet_feature_ood_*; float32 or bfloat16 widened
 *   exactly; F a BiFPN width) of the selected anchors, zeros where the entry does not count.
 * The workspace (effdet_vmf_workspace_bytes(B * K, C, d)) is scratch.  Bad arguments return -22 before any launch; no call
 * synchronises with the host or allocates; no floating-point atomics; results are bit-identical from run to run. */
long long effdet_vmf_workspace_bytes(long long rows, int C, int d);
int effdet_vmf_partition(void* stream, const float* theta, int C, int d, float* kappa, float* logz, double* logz64, double* ratio,
                         int* clamped);
int effdet_vmf_update(void* stream, const float* U, int B, long long P, int A, int d, const void* classes, int classes_dtype,
                      long long classes_pitch, long long classes_stride, long long class_offset, int C, float alpha,
                      long long rows_per_class, float* prototypes, int* valid, void* workspace, long long workspace_bytes);
int effdet_vmf_loss(void* stream, const float* U, int B, long long P, int A, int d, const void* classes, int classes_dtype,
                    long long classes_pitch, long long classes_stride, long long class_offset, int C, const float* prototypes,
                    const int* valid, const float* kappa, const float* logz, const double* ratio, const int* clamped, float* loss,
                    double* stats, float* dU, float* dtheta, void* workspace, long long workspace_bytes);
int effdet_vmf_score(void* stream, const float* U, int B, long long P, int A, int d, long long K, const long long* anchor_index,
                     const void* count, int count_is_int64, int gathered, int C, const float* prototypes, const int* valid,
                     const float* kappa, const float* logz, float* vmf, long long* vmf_class, float* vmf_cosine, float* rows,
                     void* workspace, long long workspace_bytes);
int effdet_vmf_gather(void* stream, int dtype, int num_levels, const void* const* bases, const long long* cells,
                      const long long* batch_strides, const long long* cell_strides, const long long* channel_strides, int F, int A,
                      int B, long long K, const long long* anchor_index, const void* count, int count_is_int64, float* out);

/* ---- virtual outlier synthesis (csrc/outlier_synth.hip): sample the class-conditional Gaussians, keep the least likely ------------
 * For each of the n classes c = class_ids[ci] (device int32 [n]; NULL: c = ci) draw S candidates x = mu_c + L eps, eps ~ N(0, I_F),
 * and keep the k with the largest |eps|^2, which is the Mahalanobis distance of x: the least likely ones.  eps comes from
 * Philox4x32-10 with the counter (j, c | q << 16, t_lo, t_hi) and the key (seed_lo, seed_hi) for candidate j, feature block q
 * (features 4 q .. 4 q + 3) and the draw number t = draw[0] (device int64); a word x gives u1 = (float(x >> 8) + 1) * 2^-24 or
 * u2 = float(x >> 8) * 2^-24, words (0, 1) and (2, 3) are one Box-Muller pair each: sqrtf(-2 logf(u1)) * cosf / sinf(fl(2 pi) * u2),
 * float32.  r2 = sum_d eps_d^2 with d ascending, the product and the sum rounded separately.  mu [C][F], U [F][F] = L transposed
 * (row-major, upper triangular: cov = U^T U), log_const [1] = -sum log L_dd - F / 2 * log(2 pi), valid [C] int8: device memory, read
 * when the kernels run, so a fit copied into them in place is seen by the next replay of a captured call.
 *   rows [n][k][F] float32: x_d = mu_c[d] + sum_{d' <= d} U[d'][d] * eps_d' (d' ascending from 0, float32 multiplies and adds);
 *                           zeros where valid[c] == 0 or c lies outside [0, C)
 *   index [n][k] int32: the candidates kept, r2 descending, equal r2 by j ascending;  r2 [n][k] float32
 *   log_density [n][k] float32 = -(r2 * 0.5) + log_const[0];  roles [n * k] int8: 0, or -1 where the rows are zeros
 * advance != 0: a last one-thread launch sets draw[0] = t + 1.  Limits: F a multiple of 4 in [4, 512], 1 <= C <= 1024,
 * 1 <= n <= 1024, 1 <= S <= 2^20, n * S <= 2^26, 1 <= k <= S, n * k <= 2^20; -22 otherwise, for a NULL pointer (class_ids
 * excepted) or a workspace smaller than the query's.  No floating-point atomics, no host synchronisation, no allocation; results
 * are bit-identical from run to run and for every grouping of the classes into calls (with the same draw[0]). */
int effdet_outlier_synth(void* stream, int F, int C, int n, const int* class_ids, long long S, int k, unsigned long long seed,
                         long long* draw, int advance, const float* mu, const float* U, const float* log_const,
                         const signed char* valid, float* rows, int* index, float* r2, float* log_density, signed char* roles,
                         void* workspace, long long workspace_bytes);
/* bytes of the workspace for n classes of S candidates: 20 bytes a candidate plus the sort's counts (pure host code; -22 for a bad
 * argument) */
long long effdet_outlier_synth_workspace_bytes(int n, long long S);

/* ---- few-shot episode stage (infer.py:362-447 projection phase, :566-654 meta phase), float32 ------- */

/* Confident anchors per (image, level): confs[l] -> image b's `counts[l]` confidences in (y, x, a) order at
 * confs[l] + b * image_strides[l] (elements).  outs[l] [B][keeps[l]] int32 receives the indices of the keeps[l] largest,
 * ascending; equal confidences at the cut go to the lower index; keeps[l] == counts[l] keeps all.  The pointer / size
 * arrays are host arrays of num_levels (<= 8) entries.  One launch, one workgroup per (image, level). */
int effdet_episode_select(void* stream, int B, int num_levels, const void* const* confs, const long long* image_strides,
                          const int* counts, const int* keeps, void* const* outs);

/* ProjectionNet feed rows of the selected anchors: feed [B][R][Kp], R = sum keeps[l], row =
 * [F embedding | anch_enc[a] (8) | lev_enc[first_level + l] (6) | cell enc (28) | zeros], and conf_out [B][R].
 * activs[l]: [B][W][W][F] memory, image stride activ_strides[l]; confs[l]: [B][W][W][A], image stride conf_strides[l];
 * sels[l]: [B][keeps[l]] int32 as written by the select above (an index outside the level is clamped into it).
 * Square maps of widths[l] <= cell_rows cells; the cell encoding is the reference's expression (infer.py:370-371). */
int effdet_episode_feed(void* stream, int B, int num_levels, const void* const* activs, const long long* activ_strides,
                        const void* const* confs, const long long* conf_strides, const void* const* sels, const int* keeps,
                        const int* widths, const float* anch_enc, const float* lev_enc, int lev_rows, const float* cell_enc,
                        int cell_rows, int first_level, int A, int F, int Kp, float* feed, float* conf_out);

/* Clustering of the n = m * p projected rows embds [n][d] of m images (p consecutive rows each) without any n x n matrix:
 * soft_thresh = sigmoid(dot_mult * (conf + dot_add)) (dots != NULL: a device pointer to {dot_mult, dot_add}, read instead
 * of the two arguments); proto0 / avg_init0: first per-image prototypes and their init-cluster means - 1/m;
 * valid = avg_init0 > mean(avg_init0) (use_thresh == 0) or > valid_threshold; proto / avg_init: second pick;
 * target_clust [m]; sim / nearest [n]: max and argmax (use_max) or mean (nearest = -1) cosine similarity to the second
 * prototypes; target = soft_thresh * target_clust[nearest] * sim (use_max) or soft_thresh * sim.  An empty valid set
 * gives NaN target_clust, as the reference; n_valid[0] reports it.  m <= 64, d <= 512, m * d <= 16384, n % m == 0.
 * The workspace size (floats) comes from the query below (-1: unsupported shape). */
long long effdet_episode_cluster_workspace_floats(int n, int d, int m);
int effdet_episode_cluster(void* stream, const float* embds, const float* confs, int n, int d, int m, float dot_mult,
                           float dot_add, const float* dots, int use_thresh, float valid_threshold, int use_max,
                           float* workspace, long long workspace_floats, float* soft_thresh, long long* proto0,
                           float* avg_init0, unsigned char* valid, int* n_valid, long long* proto, float* avg_init,
                           float* target_clust, float* sim, long long* nearest, float* target);

/* The projection phase's losses (infer.py:448-498) on the decisions of the cluster call above, forward and backward, without
 * any n x n matrix.  embds [n][d], confs [n], labs [n] int64 (-2 / -1 / class ids); the task class is cls_id, or
 * cls_id_dev[0] when cls_id_dev (a device pointer) is not NULL; dot_mult / dot_add / dots as for the cluster call.
 * proto0 / valid / proto [m] and nearest [n] (NULL allowed when use_max == 0) are the cluster call's results or the caller's
 * own decisions: proto0 / proto are clamped into [0, n) and nearest into [0, m) before use, so a bad index gives a wrong
 * number, never an out-of-range access.  loss_mode 0 'separate', 1 'same', 2 'no_conf' (read when use_max != 0 only).
 * Forward: losses [3] = clust_loss, embds_loss (both cosine_loss means, hinge at 0) and obj_loss (BCE-with-logits sum on
 * dot_mult (conf + dot_add) against labs > -1); inner_target [n]; stats [6] = task mean, task min, other-object mean,
 * other-object max, no-object mean, no-object max of inner_target (both entries of an empty group are NaN); counts [3]
 * the three group sizes.  An empty valid set gives NaN target_clust and so NaN clust_loss, as the reference does.
 * Backward: grad_losses [3] device floats, the upstream gradients of the three losses; d_embds [n][d], d_confs [n],
 * d_dots [2] = d dot_mult, d dot_add are overwritten.  It must be given the workspace the forward call with the same
 * arguments left behind (its first part holds inv, s, sim, target_clust, cmean and the prototypes).  The sum over the
 * rows into the prototype rows runs over a fixed split of the rows and an ordered second stage, without atomics: two
 * calls give the same bits.  n >= m, m <= 64, d <= 512, m * d <= 16384; the workspace is O(n + 32 m d) floats, its size
 * comes from the query (-1: unsupported shape). */
long long effdet_episode_proj_loss_workspace_floats(int n, int d, int m);
int effdet_episode_proj_loss(void* stream, const float* embds, const float* confs, const long long* labs, int n, int d, int m,
                             long long cls_id, const long long* cls_id_dev, float dot_mult, float dot_add, const float* dots,
                             const long long* proto0, const unsigned char* valid, const long long* proto,
                             const long long* nearest, int use_max, int loss_mode, float margin, float* workspace,
                             long long workspace_floats, float* losses, float* inner_target, float* stats, int* counts);
int effdet_episode_proj_loss_backward(void* stream, const float* embds, const float* confs, const long long* labs, int n, int d,
                                      int m, long long cls_id, const long long* cls_id_dev, float dot_mult, float dot_add,
                                      const float* dots, const long long* proto0, const unsigned char* valid,
                                      const long long* proto, const long long* nearest, int use_max, int loss_mode,
                                      float margin, const float* grad_losses, float* workspace, long long workspace_floats,
                                      float* d_embds, float* d_confs, float* d_dots);

/* The meta phase's support loss (infer.py:645-658), loss = mean_i BCE-with-logits(logits_i, t_i) with the target
 * t_i = s_i target_clust[nearest_i] sim_i ('max', use_max != 0) or s_i sim_i ('avg') of the cluster call, on the decisions
 * proto0 / valid / proto / nearest (clamped as for effdet_episode_proj_loss), differentiable twice.  float32; logits [n] may
 * be the same memory as confs.  Forward: loss [1], target [n]; the first O(n + m d) floats of the workspace keep inv, s, sim,
 * target_clust, cmean and the prototypes for the two later calls, which must be given the same arguments and workspace.
 * Backward: grad_loss [1] a device float, the upstream gradient g; d_embds [n][d], d_confs [n], d_logits [n], d_dots [2] are
 * overwritten.  thresh_grad == 0 holds s constant (FLAGS.inner_thresh_train off): d_confs and d_dots are then zero.
 * Backward2: the backward of that backward.  v_embds [n][d], v_confs [n], v_logits [n], v_mult [1], v_add [1] are the
 * cotangents on d_embds, d_confs, d_logits, d_dots[0], d_dots[1]; any of them may be NULL (zero).  d_grad [1] receives the
 * gradient with respect to g, h_embds / h_confs / h_logits / h_dots the ones with respect to the forward's inputs (g times a
 * Hessian-vector product).  Third order is not provided.  No atomics, every sum in a fixed order: two calls give the same
 * bits.  The forward and the backward compute in float32, backward2 in float64 from the float32 inputs with one rounding on
 * the way out; it uses the workspace's scratch as doubles, so the workspace must be 8-byte aligned (EINVAL otherwise).
 * n >= m, m <= 64, d <= 512, m * d <= 16384; the workspace is at most 11.5 n + 75 m d + 4 d + 400 floats (3 n + m d kept, the
 * rest scratch of a pass; -1 from the query: unsupported). */
long long effdet_episode_supp_loss_workspace_floats(int n, int d, int m);
int effdet_episode_supp_loss(void* stream, const float* embds, const float* confs, const float* logits, int n, int d, int m,
                             float dot_mult, float dot_add, const float* dots, const long long* proto0,
                             const unsigned char* valid, const long long* proto, const long long* nearest, int use_max,
                             float* workspace, long long workspace_floats, float* loss, float* target);
int effdet_episode_supp_loss_backward(void* stream, const float* embds, const float* confs, const float* logits, int n, int d,
                                      int m, float dot_mult, float dot_add, const float* dots, const long long* proto0,
                                      const unsigned char* valid, const long long* proto, const long long* nearest,
                                      int use_max, int thresh_grad, const float* grad_loss, float* workspace,
                                      long long workspace_floats, float* d_embds, float* d_confs, float* d_logits,
                                      float* d_dots);
int effdet_episode_supp_loss_backward2(void* stream, const float* embds, const float* confs, const float* logits, int n, int d,
                                       int m, float dot_mult, float dot_add, const float* dots, const long long* proto0,
                                       const unsigned char* valid, const long long* proto, const long long* nearest,
                                       int use_max, int thresh_grad, const float* grad_loss, const float* v_embds,
                                       const float* v_confs, const float* v_logits, const float* v_mult, const float* v_add,
                                       float* workspace, long long workspace_floats, float* d_grad, float* h_embds,
                                       float* h_confs, float* h_logits, float* h_dots);

/* The meta phase's inner update (infer.py:660-678) for a list of n_tensors float32 tensors in one launch:
 *     out[t][i] = p[t][i] - (lr[lr_index[t]] * g[t][i]),   i < count[t],
 * the product and the difference rounded separately, as torch's `par - par_lr * inner_grad`.  p, g, out, count, lr_index are
 * HOST arrays of n_tensors entries (device pointers to contiguous memory in the first three); lr_ptr / lr_val are host arrays
 * of n_lr entries: step size k is read on the device from lr_ptr[k] at the time the kernel runs, or is lr_val[k] when
 * lr_ptr[k] is NULL.  Everything travels by value in the kernel arguments, so the launch captures into a graph and a step
 * size changed in place is seen by the next replay.  Any 4-byte aligned pointers; 16-byte accesses are used for a tensor
 * only when its three pointers allow them.  The output tensors must not overlap the inputs or each other.
 * Limits: 1 <= n_tensors <= effdet_inner_update_max_tensors() (32), 1 <= n_lr <= effdet_inner_update_max_step_sizes() (16),
 * 1 <= count[t] <= 2^30, 0 <= lr_index[t] < n_lr; EINVAL otherwise or for a NULL pointer (lr_ptr[k] excepted).  Longer lists
 * are split by the caller.
 * Backward, for the cotangents grad_out[t] of out[t]:
 *     dg[t][i] = -(lr[lr_index[t]] * grad_out[t][i])            (dg[t] == NULL: not wanted),
 *     dlr[k]   = -sum_{t: lr_index[t] == k} sum_i grad_out[t][i] * g[t][i]     (dlr == NULL: not wanted, no reduction runs);
 * the gradient with respect to p[t] is grad_out[t] itself.  dlr [n_lr] floats are overwritten; a step size no tensor uses
 * gets 0.  The sum is taken in float64 from the float32 inputs: per workgroup, then per step size in one ordered pass, and is
 * rounded to float32 once; no atomics, two calls give the same bits.  At most two launches.  The workspace (8-byte aligned,
 * size from the query below, -1: arguments outside the limits) holds the float64 totals [max_step_sizes] followed by the
 * per-workgroup partials.  accumulate != 0 starts from the totals an earlier call left in the same workspace instead of from
 * zero and writes dlr for both together - how a caller chains the pieces of a list longer than max_tensors with the same
 * lr_ptr / lr_val table and still rounds once. */
int effdet_inner_update_max_tensors(void);
int effdet_inner_update_max_step_sizes(void);
long long effdet_inner_update_workspace_doubles(int n_tensors, const long long* count);
int effdet_inner_update(void* stream, int n_tensors, const void* const* p, const void* const* g, void* const* out,
                        const long long* count, const int* lr_index, int n_lr, const void* const* lr_ptr,
                        const float* lr_val);
int effdet_inner_update_backward(void* stream, int n_tensors, const void* const* grad_out, const void* const* g,
                                 void* const* dg, const long long* count, const int* lr_index, int n_lr,
                                 const void* const* lr_ptr, const float* lr_val, double* workspace,
                                 long long workspace_doubles, int accumulate, float* dlr);

#ifdef __cplusplus
}
#endif
#endif /* EFFDET_HIP_H */
