/*
 * tmr.h -- C ABI of libtmr.so, the MI355X-native TMR hot path.
 *
 * Every entry point replaces one reference operation on the path named by
 * BASELINE.json north_star (file:line into mFinn27/Template-Matching-and-
 * Regression-MapReduce @ 2026-01-16).  The reference
 * is pure Python over ATen/torchvision, so the "FFI" a maintainer binds is
 * Python ctypes (INTEGRATION.md shows the stub); no torch types cross this
 * boundary.
 *
 * Conventions
 *  - All tensor pointers are DEVICE pointers owned by the caller; the library
 *    never allocates or frees device memory.  fp32, NCHW, contiguous.
 *  - Every call is asynchronous on `stream` (a hipStream_t, passed as void*;
 *    NULL = the null stream) and returns 0 or a negative TMR_E* code; nothing
 *    throws across the ABI.  tmr_strerror() names the code.
 *  - No global mutable state (beyond an idempotent per-(device, kernel) cache of
 *    the LDS-size attribute): calls are reentrant across streams/devices.
 *  - "units" are (image, exemplar) matching units, described by a device
 *    array of tmr_unit_t built on the host (the reference sizes templates on
 *    the host too: template_matching.py:56-73 runs Python math on 0-d
 *    tensors).
 */
#ifndef TMR_H_
#define TMR_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TMR_ABI_VERSION 3  /* 2: per-unit out_absmax, per-sample activation scales;
                            * 3: one correlation entry point (tmr_xcorr_args_t), one
                            * sizing query (tmr_size), one split conv entry point,
                            * no subset launches (tmr_unit_t.out_unit removed) */

enum {
    TMR_OK = 0,
    TMR_E_INVALID = -1,    /* bad argument / shape */
    TMR_E_HIP = -2,        /* a HIP runtime error (launch failure) */
    TMR_E_UNSUPPORTED = -3 /* configuration not built into this library */
};

enum { TMR_TEMPLATE_ROI_ALIGN = 0, TMR_TEMPLATE_PROTOTYPE = 1 };

/* One (image, exemplar) matching unit.  Built by the host from the exemplar
 * box exactly as models/template_matching.py:43-76 does. */
typedef struct tmr_unit {
    int32_t image;         /* index into the feature batch                        */
    int32_t type;          /* TMR_TEMPLATE_*                                      */
    int32_t ht, wt;        /* template size (odd; 1x1 for prototype)              */
    float roi[4];          /* roi_align box in feature px (x1,y1,x2,y2), :61-63   */
    int32_t pbox[4];       /* prototype snapped box (x1,y1,x2,y2), :49-50         */
    int64_t tmpl_offset;   /* float offset of this unit's [C,ht,wt] template      */
    int32_t row_offset;    /* sum of na(ht) * nb(wt) over the units before this    */
                           /* one: the MFMA correlation's template windows per    */
                           /* channel (tmr_template_split defines na, nb)         */
    int32_t pad_;
} tmr_unit_t;

/* Per-unit peak-finder parameters (utils/TM_utils.py:236-278). */
typedef struct tmr_peak_param {
    float thr;             /* fl32(cls_ths), compared p >= thr (:254)             */
    float scale_w, scale_h;/* decode scale: clamped exemplar w,h or 1 (:239-243)  */
    int32_t mask;          /* 9-bit 3x3 kernel, bit (dy+1)*3+(dx+1) (:363-377)    */
    int32_t mode;          /* 0 box regression, 1 ablation_c, 2 no regression      */
    int32_t pad_;
} tmr_peak_param_t;

int tmr_version(void);
const char *tmr_strerror(int rc);

/* ---- sizes of the caller-provided buffers ---------------------------------
 * tmr_size(kind, d0..d5) returns the size of a buffer the caller allocates
 * (bytes, or floats where noted), or -1 for invalid dimensions; unused
 * dimensions are 0.
 *   TMR_SIZE_TEMPLATE_SPLIT (U, C, total_rows)          bytes, tmr_template_split: C *
 *                                                       total_rows * 2 fragments of 1024 B,
 *                                                       then 4 * U * C bytes of exponents
 *                                                       (total_rows = sum of na * nb windows)
 *   TMR_SIZE_HEADS_PARTIALS (N, U, H, W)                floats, tmr_split_conv heads
 *   TMR_SIZE_XPACK          (S, C, H, W, ks, prec)      bytes, tmr_split_xpack (H, W at
 *                                                       the output resolution)
 *   TMR_SIZE_WPACK          (N, C0, C1, ks, prec)       bytes, tmr_split_wpack
 *   TMR_SIZE_ACC            (U, N, H, W)                floats, TMR_SPLIT_TILED_OUT slabs
 *   TMR_SIZE_NMS_WORK       (total_cand, sum_nb, max_cand, G)  bytes, tmr_nms
 *   TMR_SIZE_STATS_WORK     (B)                         bytes, tmr_feature_stats
 *   TMR_SIZE_GT_WORK        (G_total, NI, H, W, U)      bytes, tmr_gt_loss */
enum {
    TMR_SIZE_TEMPLATE_SPLIT = 1,
    TMR_SIZE_HEADS_PARTIALS = 2,
    TMR_SIZE_XPACK = 3,
    TMR_SIZE_WPACK = 4,
    TMR_SIZE_ACC = 5,
    TMR_SIZE_NMS_WORK = 6,
    TMR_SIZE_STATS_WORK = 7,
    TMR_SIZE_GT_WORK = 8
};
int64_t tmr_size(int kind, int64_t d0, int64_t d1, int64_t d2, int64_t d3, int64_t d4, int64_t d5);

/* ---- (a2+a13) bilinear x2 upsample ---------------------------------------
 * f[0] = F.interpolate(feat, scale_factor=2, mode='bilinear',
 * align_corners=False) alone (matching_net.py:50-51, the API output :81):
 * feat [BC][Hin][Win] -> out [BC][2 Hin][2 Win], bit-exact with ATen's CPU
 * kernel's fma nesting. */
int tmr_upsample2x(const float *feat, int BC, int Hin, int Win, float *out, void *stream);

/* ---- (a6+a7+a8) exemplar templates --------------------------------------
 * torchvision.ops.roi_align(f, [roi], (ht,wt), aligned=True) per unit
 * (models/template_matching.py:75) or the prototype AdaptiveAvgPool2d(1)
 * (:52).  f [B,C,H,W]; templates written at units[u].tmpl_offset as [C,ht,wt]. */
int tmr_templates(const float *f, int B, int C, int H, int W, const tmr_unit_t *units, int U,
                  int max_ht, int max_wt, float *templates, void *stream);

/* ---- (a9+a4) depthwise cross-correlation + pad + scale -------------------
 * out[u] = pad(conv2d(f[img(u)], T_u, groups=C) / fl32(ht*wt)) * scale
 * (models/template_matching.py:23-41, :97), one launch over all units:
 *  f [B,C,H,W] (the projected features fp); templates from tmr_templates;
 *  units [U] sorted by image, img_units (device int32[B+1]) each image's unit
 *  range (an image's feature band is staged once for all of its exemplars);
 *  scale: device scalar (matcher.scale).
 *  squeeze != 0: out is [U,1,H,W] = pad(sum_c ...) * scale (:34-35) and `work`
 *  holds U*C*H*W floats; otherwise out is [U,C,H,W] and work may be NULL.
 *  relu_out (nullable) receives relu(out) (matching_net.py:79).
 *  out_absmax (nullable, device float[U], zeroed by the caller): raised to
 *  max |out[u]| per unit (the split decoder's per-unit activation scale
 *  source, TMR_SPLIT_XMAX_PER_UNIT), with no extra pass over out.
 *  algo: TMR_XCORR_VALU (fp32 LDS-blocked wavefront kernels), TMR_XCORR_MFMA
 *  (2-D window Toeplitz implicit GEMM on v_mfma_f32_16x16x32_{f16,bf16}:
 *  W % 64 == 0, W <= 256, templates <= 31x31, the staged band fits,
 *  tmpl_split given; TMR_E_UNSUPPORTED
 *  otherwise) or TMR_XCORR_AUTO (MFMA when it fits, tmpl_split is given and
 *  min_k -- the smallest template side of the launch -- reaches the
 *  crossover; VALU otherwise).
 *  tmpl_split / total_rows: tmr_template_split of the same templates and prec.
 *  prec (TMR_PREC_*, below): the MFMA operands -- TMR_PREC_F16X3 the fp32
 *  path's 3-term split (1e-5 contract); TMR_PREC_BF16 / TMR_PREC_F16 one
 *  16-bit term with fp32 accumulation (config C's bf16 contract, 1e-2).  The
 *  VALU kernels are fp32 whatever prec says.
 *  out_bf16 = 1: out is bf16 [U][C][H][W], each element the round-to-nearest-
 *  even bf16 of the fp32 value (the bf16 contract's detect path, whose decoder
 *  records are those bf16 values); needs algo TMR_XCORR_MFMA, prec
 *  TMR_PREC_BF16, squeeze 0 and relu_out NULL. */
#define TMR_XCORR_AUTO 0
#define TMR_XCORR_VALU 1
#define TMR_XCORR_MFMA 2
typedef struct tmr_xcorr_args {
    const float *f;
    const float *templates;
    const tmr_unit_t *units;
    const int32_t *img_units;
    const float *scale;
    void *out;
    float *relu_out;
    float *work;
    float *out_absmax;
    const void *tmpl_split;
    int64_t total_rows;
    int32_t B, C, H, W;
    int32_t U, max_ht, max_wt;
    int32_t squeeze;
    int32_t algo, min_k, prec, out_bf16;
} tmr_xcorr_args_t;
int tmr_xcorr(const tmr_xcorr_args_t *args, void *stream);
/* Which kernel tmr_xcorr(args) would launch, from the host: the same
 * validation and dispatch rule (tmr_xcorr itself decides through it), nothing
 * launched, no device pointer dereferenced (the pointer fields are only
 * compared with NULL).  Returns what tmr_xcorr returns before its first
 * launch: TMR_OK with *plan filled, else TMR_E_INVALID / TMR_E_UNSUPPORTED
 * with *plan zeroed.
 *  kernel: TMR_XCORR_KERNEL_VALU the generic fp32 kernel (W % 4 != 0 or a
 *   template wider than 31), _ROWS15 / _ROWS31 the row-tiled fp32 kernel's
 *   width specialisations (max_wt <= 15 / <= 31), _MFMA the window kernel;
 *  band_rows: output rows per block -- MFMA: 64 where the band, its halo and
 *   the 3 over-rows fit the staging registers ((67 + 2 (max_ht / 2)) * W <=
 *   16384 floats) and the band's LDS planes leave two blocks per CU (<= 78 KB),
 *   else 32; VALU: 32, fewer where the staged rows would pass 150 KB of LDS
 *   (TMR_E_UNSUPPORTED below one row);
 *  col_groups: W / 64 accumulator groups per row quad (MFMA), else 0;
 *  out16: the bf16-plane instantiation (args->out_bf16). */
#define TMR_XCORR_KERNEL_VALU 0
#define TMR_XCORR_KERNEL_ROWS15 1
#define TMR_XCORR_KERNEL_ROWS31 2
#define TMR_XCORR_KERNEL_MFMA 3
typedef struct tmr_xcorr_plan {
    int32_t kernel, band_rows, col_groups, out16;
} tmr_xcorr_plan_t;
int tmr_xcorr_plan(const tmr_xcorr_args_t *args, tmr_xcorr_plan_t *plan);
/* Operand prep of the MFMA correlation: per (unit u, channel c) template
 * T [h = ht][w = wt] = templates[units[u].tmpl_offset + c*h*w ...], x = t * 2^-e
 * (one fp32 product, exact short of fp32 underflow) with 2^-e = the scale of
 * the scale source max |T| (tmr_split_xpack's rule below: 2^-e = 2^clamp(14 -
 * e', -63, 63) with max |T| < 2^e', so max |x| < 2^14; e = 0 for an all-zero,
 * non-finite or > 3e38 maximum; NaN taps are ignored by the maximum), written
 * as the kernel's MFMA A fragments over 2-D windows of 4 template rows x 8
 * template columns:
 *   na = ceil((h + 1) / 4) window rows, nb = ceil((w + 7 + s) / 8) window
 *   columns, s = (-(w / 2)) mod 8 (w / 2 the integer quotient; 0 <= s < 8);
 *   a fragment is 1024 B = 64 lanes x 8 16-bit elements, lane l at byte 16 l;
 *   with m = l & 15 and g = l >> 4, element q = 0..7 of lane l of window
 *   (a, b) holds T[4a + g - (m >> 3)][8b + q - (m & 7) - s], and 0 where that
 *   index lies outside [0, h) x [0, w);
 *   term k (0 hi, 1 lo) of window (a, b) of (u, c) is fragment number
 *   (C * row_offset(u) + c * na * nb) * 2 + (b * na + a) * 2 + k
 *   (column-major over the windows: the order the kernel walks them);
 *   then the exponents e, int32[U][C], at byte C * total_rows * 2 * 1024.
 * row_offset(u) = sum over the units before u of na * nb, and total_rows =
 * that sum over all units (tmr_unit_t.row_offset, set by the host; the units
 * may come in any order of sizes).  Size: tmr_size(TMR_SIZE_TEMPLATE_SPLIT, U,
 * C, total_rows).
 * The terms, by prec:
 *   TMR_PREC_F16X3: hi = fp16(x rounded to TH_BITS significant bits), lo =
 *     fp16(x - hi) (the difference in fp32).  TH_BITS is the one constant of
 *     that name in csrc/xcorr.hip (11 as of ABI 3); "rounded
 *     to K significant bits" is round-to-nearest-even on the fp32 bit pattern,
 *     clearing its low 24 - K bits (inf / NaN unchanged), and K >= 11 means
 *     the plain hi = fp16(x);
 *   TMR_PREC_F16: hi = fp16(x); TMR_PREC_BF16: hi = bf16(x) (e is still
 *     written and x still scaled by 2^-e).
 *   All conversions round to nearest even.  The one-term precisions write the
 *   hi fragments only: the contents of their lo (k = 1) slots are unspecified. */
int tmr_template_split(const float *templates, const tmr_unit_t *units, int U, int C,
                       int64_t total_rows, int prec, void *out, void *stream);

/* ---- (a10+a11+a12) conv stack: head partials ------------------------------
 * tmr_split_conv with headw (below) never stores the decoder activations:
 * each 128-channel tile t of the fused decoder_b || decoder_o GEMM writes
 *   partials[t][j][u][h][w] = sum_{n in tile t} act(conv)[n] * headw[n][j], j < 5
 * (headw [ceil(N/128)*128][5] fp32, zero padded; j 0-3 = ltrbs_head,
 * 4 = objectness_head, regression_head.py:31,50), and tmr_heads_reduce() sums
 * the tiles and adds the head biases.  Size: TMR_SIZE_HEADS_PARTIALS floats. */
/* o [U,1,H,W] = head_bias[4] + sum_t partials[t][4];  b [U,4,H,W] (nullable) =
 * head_bias[j] + sum_t partials[t][j], t over ceil(N/tile_n) channel tiles
 * (tile_n = 128, the split kernel's tile; 64 is accepted too).  With b NULL
 * only the objectness partials (j = 4) are read.  Each sum is fp32, over the
 * tiles t = 0, 1, .. in order starting from +0, and the bias is added last.
 * partials is [tile][5][U][H][W].  Over a tile window of a
 * launch (TMR_SPLIT_TILE_WINDOW): partials + first * 5*U*H*W, N = 128 * count. */
int tmr_heads_reduce(const float *partials, int N, int tile_n, int U, int H, int W,
                     const float *head_bias, float *o, float *b, void *stream);

/* ---- (a11) the decoder conv: split-precision 16-bit MFMA -------------------
 * Direct implicit-GEMM kxk conv (ks 1/3/5/7, pad ks/2) over the virtual
 * channel concat x_u = cat([src0[unit_image[u]] (C0 ch), src1[u] (C1 ch)])
 * (matching_net.py:64) with bias and optional LeakyReLU(0.01)
 * (regression_head.py:7-8) on v_mfma_f32_16x16x32_{f16,bf16}; unit_image
 * (device int32[U]) may be NULL (identity).  Operands are pre-packed 16-bit
 * records:
 *   TMR_PREC_F16X3: x*s = xh + xl, w*s' = wh + wl (fp16, power-of-two scales
 *                   from the tensors' max |.|), x.w = (wh xh + wl xh + wh xl)
 *                   / (s s') with fp32 accumulation: the fp32 path's 1e-5
 *                   normwise contract (config B);
 *   TMR_PREC_BF16:  one bf16 term, fp32 accumulation (config C, 1e-2 contract);
 *   TMR_PREC_F16:   one scaled fp16 term.
 * Scale sources and scales.  A scale source is a float m >= 0, normally a
 * max |.|; its scale is split_scale(m) = 2^clamp(14 - e, -63, 63) with e the
 * integer with 2^(e-1) <= m < 2^e (so m * scale < 2^14; the clamp keeps the
 * product of an activation and a weight scale a normal fp32 number).  A
 * source that is 0, negative, NaN, infinite or above 3e38 gives scale 1.
 * TMR_PREC_BF16 uses no scales (scale 1; the scale pointers may be NULL).
 * tmr_absmax_rows: out[s] = max |x[s][0..n)| for x [S][n] (or max(out[s], ...)
 * when accumulate; S < 65536; n = 0 gives 0, or leaves out[s] when accumulate;
 * any alignment of x), the scale sources for the packs and the conv (F16X3 /
 * F16; NULL allowed for BF16).  tmr_pixel_absmax (below) likewise per pixel.
 * Both ignore NaN elements (a row or pixel of NaNs alone gives 0), return
 * +inf when an element is +-inf, and +0 for -0.0; with accumulate, out[s]
 * must hold a non-negative float (it is compared as an unsigned bit pattern).
 * tmr_scale_merge: out_img[b] = max(0, img_max[b] (nullable: absent),
 * unit_max[u] over the units with unit_image[u] == b), out_unit[u] =
 * out_img[unit_image[u]] (out_img nullable: only out_unit is written) -- one
 * scale per image for a launch whose tiles read an image's src0 records and
 * its units' src1 records together.  unit_image may be in any order and any
 * U; an image without units receives max(0, img_max[b]), i.e. 0 when img_max
 * is NULL; out_unit[u] of a unit whose image lies outside [0, B) is not written.
 * tmr_split_xpack: x [S][C][H][W] fp32 -> planar 16-B pieces
 *   [S][NC = ceil(C/32) chunks][halves][4 pieces q][Hp][Wp][8 x 16 bit]
 * (halves 2 for F16X3: hi then lo; 1 otherwise), Hp = ceil(H/16)*16 + ks - 1,
 * Wp = ceil(W/32)*32 + ks - 1 (whole 16x32 tiles plus the ks halo; size
 * TMR_SIZE_XPACK = S * NC * halves * Hp * Wp * 64 bytes).  Element j of piece
 * q of chunk c at padded (yp, xp) is channel 32c + 8q + j of pixel (yp - ks/2,
 * xp - ks/2); channels >= C and pixels outside the image are zero in every
 * term.  With v = x * scale (one fp32 product): F16X3 hi = fp16(v), lo =
 * fp16(v - hi) (the difference in fp32); F16 fp16(v); BF16 bf16(x); all
 * round to nearest even.  In every record and fragment of this header the
 * sign of the zero terms of a -0.0 input is unspecified: they may be stored
 * as +0 or as -0 (the compiler may fuse the scaling and the conversion into
 * one multiply-add with a +0 addend, for some elements of a piece and not
 * for others); a zero operand adds the same to every non-zero sum either
 * way.  Every other term, negative values that round to -0 included, is as
 * stated.  `up` bit TMR_XPACK_UPSAMPLE: the records are
 * of up2x(x) (tmr_upsample2x's values bit for bit; H, W are x's; the records',
 * and those in the formulas above, are 2H, 2W); bit TMR_XPACK_ONES: a
 * constant-1 channel is appended as channel C (C + 1 channels in the formulas
 * above; see tmr_split_fold_proj): 1 inside the image, 0 in the padding, so
 * its hi element is fp16(1 * scale) (lo 0).  The caller keeps that finite: the
 * scale source must be >= 0.25 (scale <= 2^15; a smaller source gives
 * scale >= 2^16 and an infinite fp16), e.g. max(max |x|, 1), the maximum
 * over the appended channel too; a source of 2^38 or more (scale <= 2^-25)
 * rounds the channel to 0.
 * xmax_per_sample = 0: one scale source *xmax for
 * every sample; 1: xmax[s] for sample s (float[S]); 2: xmax[s][y][x] per
 * (output-resolution) pixel, for TMR_SPLIT_XMAX_PER_PIXEL 1x1 convs.
 * Per-sample scales make a unit's arithmetic independent of the other units
 * of the batch: its hi/lo parts never go subnormal because another sample is
 * 2^20 larger (a power-of-two rescale is exact otherwise, so results equal
 * the single-unit run's bit for bit).
 * tmr_split_wpack: w [N][C0+C1][ks][ks] -> planar 16-B pieces
 *   [tap = ky*ks + kx][chunk][plane][Npad = ceil(N/128)*128][8 x 16 bit];
 * the conv's src0 (per image, C0 channels, packed by xpack with S = images)
 * and src1 (per unit, C1) may both be present, and each is padded to whole
 * 32-channel chunks by itself: chunks 0 .. NC0-1 (NC0 = ceil(C0/32)) are
 * src0's, element j of piece q of chunk c being input channel 32c + 8q + j
 * (zero from C0 on); chunks NC0 .. NC0+NC1-1 (NC1 = ceil(C1/32)) are src1's,
 * input channel C0 + 32(c - NC0) + 8q + j (zero from C0 + C1 on).  Planes:
 * 4 hi pieces q = 0..3, then for F16X3 4 lo pieces (8 planes; 4 otherwise).
 * Rows n >= N are zero.  Size TMR_SIZE_WPACK = ks*ks * (NC0+NC1) * Npad *
 * (128 | 64) bytes.  With v = w * split_scale(*wmax) (one fp32 product):
 * F16X3 wh = fp16(v rounded to WH_BITS significant bits), wl = fp16(v - wh)
 * (the difference in fp32) -- WH_BITS is the one constant of that name in
 * csrc/conv_split.hip (8 as of ABI 3), "rounded to K
 * significant bits" as under tmr_template_split; F16 fp16(v); BF16 bf16(w).
 * The activations' hi part is always the plain fp16(v).
 * Head partials use 128-channel tiles (tmr_heads_reduce tile_n = 128). */
#define TMR_PREC_F16X3 0
#define TMR_PREC_BF16 1
#define TMR_PREC_F16 2
int tmr_absmax_rows(const float *x, int S, int64_t n, int accumulate, float *out, void *stream);
int tmr_scale_merge(const float *img_max, const float *unit_max, const int32_t *unit_image, int B, int U,
                    float *out_img, float *out_unit, void *stream);
#define TMR_XPACK_UPSAMPLE 1
#define TMR_XPACK_ONES 2
int tmr_split_xpack(const float *x, int S, int C, int H, int W, int up, int ks, int prec,
                    const float *xmax, int xmax_per_sample, void *out, void *stream);
/* tmr_split_xpack16: the TMR_PREC_BF16 records of a bf16 x [S][C][H][W]
 * (tmr_xcorr's bf16 f_TM; W % 8 == 0) in tmr_split_xpack's planar layout,
 * size and padding: bit-identical to tmr_split_xpack of the fp32 values
 * those bf16 elements round. */
int tmr_split_xpack16(const void *x, int S, int C, int H, int W, int ks, int prec, void *out,
                      void *stream);
/* tmr_split_fold_proj: with tmr_split_xpack's TMR_XPACK_UPSAMPLE | ONES
 * records of the SAM features it feeds the decoder's fp half without
 * materialising fp: conv(input_proj(x))
 * = conv'([x; 1]), W'[n][c] = sum_k Wd[n][k] P[k][c], W'[n][Cin] = sum_k
 * Wd[n][k] b[k] per tap (matching_net.py:27-30,56,63-69), each sum accumulated
 * in fp64 over k = 0 .. Cp-1 ascending from 0 and rounded once to fp32;
 * out [N][Cin+1][ks][ks] from wd [N][Cw][ks][ks] (first Cp channels = fp),
 * proj_w [Cp][Cin], proj_b [Cp]. */
int tmr_split_fold_proj(const float *wd, int N, int Cw, int Cp, int ks, const float *proj_w,
                        const float *proj_b, int Cin, float *out, void *stream);
int tmr_split_wpack(const float *w, int N, int C0, int C1, int ks, int prec, const float *wmax,
                    void *out, void *stream);
/* tmr_split_conv: headw NULL -- `out` [U][N][H][W] receives act(conv + bias);
 * headw given -- `out` receives the head partials (above, TMR_SIZE_HEADS_PARTIALS
 * floats) and the activations are never stored.
 * flags: TMR_SPLIT_TILED_OUT (headw NULL only): `out` receives the raw conv
 * result (no bias / activation) in the kernel's tiled accumulator layout,
 * TMR_SIZE_ACC(U, N, H, W) floats; TMR_SPLIT_TILED_INIT: `acc_init` is
 * in that layout (indexed by unit_image), e.g. the per-image fp half. */
#define TMR_SPLIT_TILED_OUT 1
#define TMR_SPLIT_TILED_INIT 2
#define TMR_SPLIT_INIT_BCAST 4  /* acc_init is ONE slab shared by every unit
                                 * (e.g. the folded projection bias plane) */
/* the tiled `out` (TMR_SPLIT_OUT_BF16) / tiled `acc_init` (TMR_SPLIT_INIT_BF16)
 * hold bf16 values (round to nearest even) in the first half of the same
 * allocation: one-term precisions only (the per-image fp half under the bf16
 * contract; halves the heads launch's initial-value read) */
#define TMR_SPLIT_OUT_BF16 8
#define TMR_SPLIT_INIT_BF16 16
/* xmax is float[U], one activation scale source per unit u (the output slab;
 * the image index for a per-image store): both record sets a tile reads must
 * have been packed with that unit's value (tmr_split_xpack xmax_per_sample,
 * tmr_scale_merge when src0 is per image) */
#define TMR_SPLIT_XMAX_PER_UNIT 32
/* 1x1 plain stores (no acc_init, no tiled out): xmax is float[U][H][W], one
 * scale source per output pixel -- the max over that pixel's input channels
 * (tmr_pixel_absmax), the records packed with tmr_split_xpack(_up)
 * xmax_per_sample = 2 -- so every pixel is fp32-grade relative to its own
 * magnitude (the projection: templates cut from a quiet region of an image
 * are renormalised by the correlation, template_matching.py:75,31) */
#define TMR_SPLIT_XMAX_PER_PIXEL 64
/* flags bits 8..15: E, the units per image (unit u of image u / E; U % E ==
 * 0) -- the launch then runs an image's E units' blocks of one output tile
 * back to back (image-major order; 0 or 1: unit-major).  Results are the
 * same either way; only the order, and so the cache reuse, changes. */
#define TMR_SPLIT_UNITS_PER_IMAGE_SHIFT 8
/* flags bits 16..23 / 24..30: a window (first tile, tile count) of the
 * ceil(N/128) 128-channel tiles: the launch computes only those tiles, from
 * the same packs, acc_init slabs and out / partials layout as the full launch
 * (N, bias, headw stay the full problem's), so what it writes is bit-identical
 * to the full launch's; count 0 (with first 0) = every tile.  Head partials
 * are [tile][5][U][H][W], so tmr_heads_reduce over a window takes partials +
 * first * 5 * U * H * W and N = 128 * count (b = NULL where the window holds
 * no regression channels).  A head's partial from a tile where its head
 * weights are zero is 0 * act = +-0 (act finite): leaving such tiles out
 * changes at most the sign of an exactly zero sum, and never a sum the
 * reduce starts from +0. */
#define TMR_SPLIT_TILE_FIRST_SHIFT 16
#define TMR_SPLIT_TILE_COUNT_SHIFT 24
#define TMR_SPLIT_TILE_WINDOW(first, count) \
    (((first) << TMR_SPLIT_TILE_FIRST_SHIFT) | ((count) << TMR_SPLIT_TILE_COUNT_SHIFT))
/* out[s][p] = max_c |x[s][c][p]| for x [S][C][HW], any C >= 1 (NaN, inf and
 * -0.0 as tmr_absmax_rows: see "Scale sources and scales" above) */
int tmr_pixel_absmax(const float *x, int S, int C, int64_t HW, float *out, void *stream);
int tmr_split_conv(const void *xp0, int C0, const int32_t *unit_image, const void *xp1, int C1, int U,
                   int H, int W, int ks, int prec, const void *wpack, const float *wmax, const float *xmax,
                   const float *bias, int N, int leaky, const float *headw, const float *acc_init,
                   float *out, int flags, void *stream);

/* tmr_split_conv_points: the heads launch at a list of points.  For every
 * candidate listed by `tiles` it computes what tmr_split_conv (headw given,
 * the same operands and flags) followed by tmr_heads_reduce writes into
 * b [U][4][H][W] at that candidate's pixel -- bit for bit: the same chain of
 * MFMAs per accumulator element, head arithmetic and tile-order sum -- and
 * writes those four values there; every other element of b is left untouched.
 * tiles (device int32[ntiles][3]): (unit, first candidate, count), count in
 * 1..TMR_POINTS_TILE, a tile within one unit, the list in any order (the
 * launch may process tiles in pairs, entries 2i and 2i+1 in one workgroup,
 * whatever their units; no value depends on the pairing); candidate i of unit u has its
 * pixel index y*W + x in ((const int32_t *)box)[4 * (u*H*W + i)], where
 * tmr_peaks_decode with TMR_PEAKS_FIND_ONLY leaves it.  acc_init is NULL or
 * tiled (TMR_SPLIT_TILED_INIT, optionally _INIT_BCAST / _INIT_BF16); the
 * flags' tile window selects the channel tiles summed into b (at most 8, e.g.
 * decoder_b's of decoder_b || decoder_o).  ks must be 3; other kernel sizes
 * and wider windows return TMR_E_UNSUPPORTED (run the dense window instead). */
#define TMR_POINTS_TILE 64
int tmr_split_conv_points(const void *xp0, int C0, const int32_t *unit_image, const void *xp1, int C1, int U,
                          int H, int W, int ks, int prec, const void *wpack, const float *wmax, const float *xmax,
                          const float *bias, int N, int leaky, const float *headw, const float *head_bias,
                          const float *acc_init, const float *box, const int32_t *tiles, int ntiles, float *b,
                          int flags, void *stream);

/* (tmr_points_chain.h, an extension outside this ABI: the per-image store launch and this launch at the
 * points as one chain, without the slab between them) */

/* ---- (a16) custom_shape_3x3_maxpool2d -----------------------------------
 * utils/TM_utils.py:337-361 on device fp32 planes x [planes][H][W]: out[e] =
 * the max over the 3x3 neighbourhood taps selected by mask9 (bit 3*r + c is
 * kernel[r][c]; zero padding as F.unfold), taps in row-major order, a NaN
 * propagates and ties keep the earlier tap.  mask9 == 0 (an empty selection,
 * which torch.max rejects) or bits above 8 return TMR_E_INVALID. */
int tmr_maxpool3x3(const float *x, int64_t planes, int H, int W, int mask9, float *out, void *stream);

/* ---- (a14-a16) peak finder + box decode ------------------------------------
 * Get_pred_boxes per unit (utils/TM_utils.py:245-282): p = sigmoid(o) (or o
 * itself when input_is_prob), masked 3x3 local max with zero padding,
 * p >= thr, row-major compaction (no cap), decode.  Outputs per unit u at
 * stride cap = H*W: logits[(u*cap+i)*2] = (p, 0) (TM_utils.py:260-261),
 * box[(u*cap+i)*4] (normalised xyxy), ref[(u*cap+i)*2], counts[u]; a unit
 * with no peak (counts[u] = 0) gets the reference's dummy row at its row 0
 * (logits (0,0), box (0,0,1e-14,1e-14), ref (0,0); TM_utils.py:288-291).
 * prob [U,H,W] receives the probability map (required).  With
 * TMR_PEAKS_PROB_SCRATCH or-ed into input_is_prob it is scratch only: a
 * pixel whose logit lies well below its unit's threshold holds -1 there (its
 * sigmoid is skipped); the candidates are the same.
 * exp_table (device, nullable): the reference-exp table (tmr_amd/exp_table.py:
 * 128-B header, uint32 offsets[65537], sorted uint16 low halves).  The decode's
 * exp (TM_utils.py:272) is the correctly rounded value except at the table's
 * inputs, where it is the other neighbour, as the reference's torch.exp (MKL
 * vsExp) rounds; NULL = correctly rounded everywhere. */
#define TMR_PEAKS_PROB_SCRATCH 2  /* input_is_prob flag: prob is scratch (see above) */
/* Two-phase use (input_is_prob flags; value 4 is not a flag and is refused).
 * TMR_PEAKS_FIND_ONLY: probability map + finder only (reg may be NULL):
 * logits, ref and counts as above, and box row i of unit u holds candidate
 * i's pixel index y*W + x as an int32 in its first element instead of a box
 * (the dummy row of an empty unit is written as above).
 * TMR_PEAKS_DECODE_ONLY: the decode alone over the rows a FIND_ONLY call left
 * (o, prob, logits unused but required non-NULL): box rows become boxes. */
#define TMR_PEAKS_FIND_ONLY 8
#define TMR_PEAKS_DECODE_ONLY 16
int tmr_peaks_decode(const float *o, int input_is_prob, const float *reg, int U, int H, int W,
                     const tmr_peak_param_t *params, float *prob, float *logits, float *box,
                     float *ref, int32_t *counts, const void *exp_table, void *stream);

/* ---- (§8 GT_map + SetCriterion_TM) evaluation losses ------------------------
 * What the reference's trainer.py:75-153 computes on every validation / test
 * step when ground truth is present: GT_map.Get_pred_gts (utils/TM_utils.py:
 * 94-222) and SetCriterion_TM (criterion/criterions_TM.py) for ONE level of
 * U (image, exemplar) units over NI images with their GT boxes.  No gradient
 * is produced: training and backward are out of scope.
 *
 * Per GT box g = (x1,y1,x2,y2) of an image (fp32, every op separately rounded,
 * divisions correctly rounded): cx = (x2+x1)/2, cy = (y2+y1)/2, ws = x2-x1,
 * hs = y2-y1, ratio = -hs/ws (inf / NaN for ws = 0: both tests below are then
 * false by IEEE comparison, as in the reference), bias_p = fl32((1-pt)/(1+pt))
 * * hs and bias_n likewise from nt (the quotient in double on the host, rounded
 * once), area = (x2-x1)*(y2-y1).
 * Per pixel i = y*W + x: cxs = fl32(x)/fl32(W), cys = fl32(y)/fl32(H),
 * rx = |cxs-cx|, ry = |cys-cy|, inpos = (ratio*rx + bias_p) >= ry, inneg =
 * (ratio*rx + bias_n) < ry (mul and add not fused).  center_g = the lowest-index
 * pixel minimising fl32(rx+ry).  pt == 1.0: inpos := is_center; nt == 1.0:
 * inneg := !is_center.  pos_g = inpos | is_center on the last level, inpos
 * otherwise.  Per image and pixel: any_pos, all_pos, any_notneg = any_g(!inneg),
 * and target = the first g minimising (pos_g ? area : 1e8f) (0 when no pos_g).
 * Per unit: nib = pad_y <= y < H-pad_y && pad_x <= x < W-pad_x (the exemplar's
 * boundary rectangle, TM_utils.py:36-54); positive = nib & any_pos; ignore =
 * nib & !all_pos & any_notneg; negative = !(positive | ignore); gt_map = 1.0
 * positive, 0.5 ignore only, 0.0 negative.  So the box loop runs once per
 * IMAGE; a unit only applies its rectangle.
 * Prediction row of a positive pixel (TM_utils.py:183-193): xy = (cxs,cys) +
 * reg[0:2] * (sw,sh) ((1,1) for mode 1), wh = exp(reg[2:4]) * (scale_w,
 * scale_h), zero regressions for mode 2, the exp as tmr_peaks_decode's
 * (exp_table); its GT row is (cx, cy, ws, hs) of box target.  A unit with no
 * positive pixel contributes the row [0,0,1e-14,1e-14] as both.
 * Element losses (fp64 evaluation of the fp32 samples / rows): ce = BCE with
 * logits (positives: target 1, negatives: target 0, ignore pixels excluded),
 * with focal: at * (1-exp(-ce))^2 * ce, at = 0.25 positives / 0.75 negatives;
 * giou = torchvision generalized_box_iou_loss(eps = 1e-13) on the cxcywh ->
 * xyxy rows: intersection only where both extents are > 0, iou = I/(U+eps),
 * 1 - iou + (Ac-U)/(Ac+eps).  Sums are fp64 in a fixed order (a unit's pixels
 * in TMR_GT_SLICES slices, then the slices in order): a repeat run, or the
 * unit inside another batch, gives the same bits.
 *
 * phase (a bit set; the steps run in this order):
 *  TMR_GT_ASSIGN  box records, per-image classes, then per unit gt_map
 *                 [U,1,H,W], target [U,H,W] (int32, box index local to the
 *                 image; 0 where not positive) and counts [U][2] = positive,
 *                 negative pixels.  With TMR_GT_LOSS in the same call, also
 *                 sums [U][2] (fp64) = {sum ce, sum giou} straight from o /
 *                 reg, no gather; a unit with no positive pixel has sum giou =
 *                 the dummy pair's loss and counts 1 row towards num_positive
 *                 (the caller's max(counts[u][0], 1)).
 *  TMR_GT_LOSS    only together with TMR_GT_ASSIGN (above).
 *  TMR_GT_GATHER  from gt_map / target / counts of an earlier ASSIGN (same
 *                 arguments): unit u's samples at obj_out + samp_off[u]:
 *                 o at its positive pixels (row-major), then at its negative
 *                 pixels; label_out the same layout of 1 / 0; rows_pred /
 *                 rows_gt [.,4] at row row_off[u]: one per positive pixel, or
 *                 the dummy row.  samp_off / row_off (device int64[U]) are the
 *                 host's prefix sums of counts (one read-back, as the
 *                 reference's boolean indexing syncs).
 *  TMR_GT_ROWS    alone: the same element losses over gathered lists:
 *                 obj_out / label_out [n_samples], rows_pred / rows_gt
 *                 [n_rows,4] -> sums[0..1] = {sum ce, sum giou}.
 * ASSIGN / GATHER need boxes (device float[G_total][4], finite), box_off
 * (device int32[NI+1], image m's boxes box_off[m] .. box_off[m+1]-1), units
 * (device tmr_gt_unit_t[U]) and min_boxes = the smallest per-image box count
 * as the host counted it: 0 (an image without GT, where the reference's
 * torch.min raises) is refused.  Each image needs fewer than 2^29 boxes and
 * H*W must fit int32.  work: TMR_SIZE_GT_WORK(G_total, NI, H, W, U) bytes
 * (TMR_GT_ROWS: any G_total, NI, H, W, U >= 1). */
typedef struct tmr_gt_unit {
    int32_t image;           /* index into box_off: the image whose boxes apply     */
    int32_t pad_x, pad_y;    /* boundary pads (TM_utils.py:36-48), >= 0             */
    int32_t mode;            /* as tmr_peak_param_t.mode                            */
    float scale_w, scale_h;  /* clamped exemplar w,h or 1 (TM_utils.py:128-135)     */
    int32_t pad_[2];
} tmr_gt_unit_t;
#define TMR_GT_ASSIGN 1
#define TMR_GT_LOSS 2
#define TMR_GT_GATHER 4
#define TMR_GT_ROWS 8
#define TMR_GT_SLICES 16
typedef struct tmr_gt_loss_args {
    const float *o;            /* [U,1,H,W] objectness logits (LOSS, GATHER)          */
    const float *reg;          /* [U,4,H,W] regressions; NULL only if every mode is 2 */
    const float *boxes;
    const int32_t *box_off;
    const tmr_gt_unit_t *units;
    const void *exp_table;     /* nullable, as tmr_peaks_decode                       */
    void *work;
    float *gt_map;
    int32_t *target;
    int32_t *counts;
    double *sums;
    const int64_t *samp_off;
    const int64_t *row_off;
    float *obj_out;
    float *label_out;
    float *rows_pred;
    float *rows_gt;
    double positive_threshold, negative_threshold;
    int64_t n_samples, n_rows; /* TMR_GT_ROWS                                         */
    int32_t U, NI, H, W;
    int32_t G_total, min_boxes;
    int32_t last_level, focal;
    int32_t phase, pad_;
} tmr_gt_loss_args_t;
int tmr_gt_loss(const tmr_gt_loss_args_t *args, void *stream);

/* ---- (a17-a19) per-image greedy NMS over the exemplar-ordered union --------
 * torchvision.ops.nms (utils/TM_utils.py:317-323) on, per image g, the
 * concatenation (in unit order seg_units[g] .. seg_units[g+1]-1) of each
 * unit's candidates, or of the dummy row [0,0,1e-14,1e-14]/score 0 when the
 * unit has none (TM_utils.py:288-291).  Unit u's counts[u] candidates start
 * at row unit_off[u] (device int64[U]) of logits [.,2] / box [.,4] /
 * ref [.,2]; the score is logits[.,0] (:319).  seg_units (device int32[G+1]),
 * cand_off (device int64[G+1], the offsets of those unions) and nb_off
 * (device int64[G+1], prefix sums of ceil(n_g/64)) are computed on the
 * host from the candidate counts (one sync, as the reference's torch.where);
 * sum_nb = nb_off[G], max_cand = max n_g.
 * Outputs are written per image at cand_off[g]: keep-ordered logits [n,2] =
 * (score, 0), boxes [n,4], refs [n,2], optionally the keep indices (int64,
 * local to the image's union, = torchvision's return value) and kept[g].
 * `work` holds TMR_SIZE_NMS_WORK(total_cand, sum_nb, max_cand, G) bytes:
 * linear in the candidates, at most ~640 B per candidate (the suppressor
 * lists take 512 B of it: 128 entries per row, sized per 64-row block), so
 * the worst case -- every pixel of 16 units at 192^2 a candidate of one
 * image, 589,824 rows -- needs ~0.38 GB.  An image of more than 655,360
 * candidates is refused with TMR_E_INVALID (the greedy wave's LDS holds the
 * kept bitmap), never truncated. */
int tmr_nms(const float *logits, const float *box, const float *ref, const int32_t *counts,
            const int64_t *unit_off, const int32_t *seg_units, const int64_t *cand_off,
            const int64_t *nb_off,
            int G, int64_t total_cand, int64_t max_cand, int64_t sum_nb, double iou_threshold,
            float *out_logits, float *out_boxes, float *out_refs, int64_t *out_keep,
            int32_t *kept, void *work, void *stream);
/* tmr_nms for images of at most TMR_NMS_SMALL candidates, sized on the
 * DEVICE from counts (no host sync before it, so it can follow the peak
 * finder inside one captured forward): image g's kept rows are written at
 * row g * TMR_NMS_SMALL of out_logits [G*TMR_NMS_SMALL,2] / out_boxes [.,4] /
 * out_refs [.,2] (+ out_keep, nullable), kept[g] = their count -- the same
 * rows and order tmr_nms produces -- or kept[g] = -1 when the image's union
 * exceeds TMR_NMS_SMALL rows (then nothing is written for it: run tmr_nms).
 * One workgroup per image, no work memory. */
#define TMR_NMS_SMALL 256
int tmr_nms_small(const float *logits, const float *box, const float *ref, const int32_t *counts,
                  const int64_t *unit_off, const int32_t *seg_units, int G, double iou_threshold,
                  float *out_logits, float *out_boxes, float *out_refs, int64_t *out_keep,
                  int32_t *kept, void *stream);

/* ---- (§8f f1) streaming mapper statistics ---------------------------------
 * Per image b of x [B][n] fp32 (the backbone feature the mapper computes,
 * mapper.py:94), out[b] = {mean, std, max, sparsity} (fp64), as
 * mapper.py:97-101 computes them with numpy: mean = np.mean(f) and
 * std = np.std(f) (population) each correctly rounded to fp32 from an fp64
 * evaluation (numpy's float32 pairwise sums differ by a few fp32 ulps),
 * max = np.max(f) exactly, sparsity = np.mean(f <= 0) = count / n exactly.
 * Deterministic (fixed reduction order).  `work` holds
 * TMR_SIZE_STATS_WORK(B) bytes. */
int tmr_feature_stats(const float *x, int B, int64_t n, void *work, double *out, void *stream);

/* ---- the decode's reference-exp table, compact form ------------------------
 * Host-only (no device pointers, no stream).  The table of fp32 inputs where
 * the reference's torch.exp (utils/TM_utils.py:272, MKL vsExp on the golden
 * host) is not the correctly rounded exp (tmr_amd/exp_table.py) is committed
 * as a range-coded candidate bitmap (csrc/exp_codec.cpp).
 * tmr_exp_table_encode: `exc` = the n recorded fp32 bit patterns, sorted
 * (positive x first); out = NULL returns the blob size; else writes it and
 * returns its size (< 0: TMR_E_INVALID, or TMR_E_UNSUPPORTED when an input
 * lies outside the codec's candidate set).
 * tmr_exp_table_decode: out = NULL returns the recorded count; else writes
 * the sorted bit patterns and returns the count (< 0 on a malformed blob). */
int64_t tmr_exp_table_encode(const uint32_t *exc, int64_t n, uint8_t *out, int64_t cap);
int64_t tmr_exp_table_decode(const uint8_t *blob, int64_t nbytes, uint32_t *out, int64_t cap);

#ifdef __cplusplus
}
#endif
#endif /* TMR_H_ */
