/* tmr_maskhead.h -- the third optional extension of libtmr.so: the mask head of
 * the SAM mask decoder (reference utils/segment_anything/modeling/
 * mask_decoder.py:149-156 with the argmax selection of :101-103), fused.
 *
 * Not part of the core ABI of tmr.h (TMR_ABI_VERSION is unchanged by it).  The
 * two-way transformer, the token-side MLPs and the prompt encoder stay the
 * caller's modules; this is what follows the transformer: output_upscaling
 * (ConvTranspose2d 256->64 k2 s2, LayerNorm2d, GELU, ConvTranspose2d 64->32
 * k2 s2, GELU) and the product with ONE hypernetwork row per prompt.  Neither
 * the [N,64,2h,2w] nor the [N,32,4h,4w] tensor is ever written to memory.
 *
 * THE RULE.  For prompt n and embedding pixel p = y * w + x:
 *   src[n][p][0..255]   the transformer's second output, token-major, as
 *                       TwoWayTransformer returns it
 *   hyper[n][0..31]     the selected hypernetwork MLP's output
 *   W1[256][64][2][2], b1[64]   output_upscaling.0, ConvTranspose2d layout
 *                               [in][out][ky][kx]
 *   g[64], beta[64], eps        output_upscaling.1 (LayerNorm2d)
 *   W2[64][32][2][2], b2[32]    output_upscaling.3
 *
 *   u[k][l][o] = b1[o] + sum_c src[n][p][c] * W1[c][o][k][l]      k,l in {0,1}, o < 64
 *   mu = mean_o u[k][l][.];  s = mean_o (u - mu)^2
 *   a[k][l][o] = gelu(g[o] * (u[k][l][o] - mu) / sqrt(s + eps) + beta[o])
 *                                       gelu(x) = x/2 * (1 + erf(x / sqrt 2))
 *   t[k][l][m][j][q] = gelu(b2[q] + sum_o a[k][l][o] * W2[o][q][m][j])   m,j in {0,1}, q < 32
 *   mask[n][4y + 2k + m][4x + 2l + j] = sum_q hyper[n][q] * t[k][l][m][j][q]
 *
 * Precision: the fp32 contract (normwise <= 1e-5 against the rule in float64).
 * Both products run on v_mfma_f32_16x16x32_f16 as three fp16 terms
 * (hi.hi + lo.hi + hi.lo, fp32 accumulation) with power-of-two scales: one per
 * src row, one per (pixel, k, l) row of a, one per weight tensor.  erf is
 * evaluated in fp32 to 1e-7 absolute.
 *
 * Non-finite values: any non-finite value in a src row makes that pixel's 16
 * mask values NaN; a NaN in hyper[n] makes mask n NaN; every other pixel and
 * mask keeps the contract.
 *
 * PACKED WEIGHTS (tmr_mask_head_prep -> wpack, TMR_MASK_HEAD_WPACK_BYTES, 16-B
 * aligned).  Nine 32-KiB chunks of 1-KiB MFMA A fragments (64 lanes x 8 fp16;
 * lane = 16 * grp + row, element e) and a 64-B tail:
 *   chunks 0..7 (W1, K step ks = channels 32ks .. 32ks+31): fragment
 *     (T * 2 + half), T < 16, half 0 = hi, 1 = lo;  row R = 16T + row =
 *     64 * (2k + l) + o, channel c = 32ks + 8grp + e:  W1[c][o][k][l] * s1
 *   chunk 8 (W2): fragment ((T * 2 + st) * 2 + half), T < 8, st < 2;  row
 *     R = 16T + row = 32 * (2m + j) + q, o = 16 * (2st + (e >> 2)) + 4grp + (e & 3)
 *     (the order in which stage 1's accumulator registers hold o):
 *     W2[o][q][m][j] * s2
 *   tail: float 1 / s1, 1 / s2; s = the power of two with max|W| s < 2^14;
 *     hi = fp16(W s), lo = fp16(W s - hi).
 *
 * Limits: C == 256 (else TMR_E_UNSUPPORTED); 1 <= h <= 16384, 1 <= w <= 1024
 * (4h, 4w within tmr_mask_boxes' limits), 0 <= N, N * h * w < 2^31, eps >= 0; src,
 * wpack and masks 16-B aligned; otherwise TMR_E_INVALID.  Null buffers with
 * N > 0: TMR_E_INVALID.  N = 0 is a no-op.  Everything is enqueued on
 * `stream`; nothing synchronises with the host.
 */
#ifndef TMR_MASKHEAD_H_
#define TMR_MASKHEAD_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TMR_MASK_HEAD_WPACK_BYTES (9 * 32768 + 64)

#define TMR_MASK_HEAD_VARIANT_MFMA128 0 /* 4 waves x 32 embedding pixels, weights staged per K step */

typedef struct tmr_mask_head_args {
    const float *src;    /* [N][h*w][C] */
    const float *hyper;  /* [N][C/8] */
    const float *w1;     /* prep only: [C][C/4][2][2] */
    const float *w2;     /* prep only: [C/4][C/8][2][2] */
    void *wpack;         /* TMR_MASK_HEAD_WPACK_BYTES: written by prep, read by tmr_mask_head */
    const float *b1;     /* [C/4] */
    const float *g;      /* [C/4] */
    const float *beta;   /* [C/4] */
    const float *b2;     /* [C/8] */
    float *masks;        /* out [N][4h][4w] */
    int64_t N;
    int32_t h, w;        /* embedding size */
    int32_t C;           /* transformer_dim: 256 */
    float eps;
} tmr_mask_head_args_t;

typedef struct tmr_mask_head_plan {
    int32_t variant;       /* TMR_MASK_HEAD_VARIANT_* */
    int32_t tile_pixels;   /* embedding pixels per block */
    int32_t threads;
    int32_t lds_bytes;
    int32_t tiles;         /* blocks per prompt: ceil(h * w / tile_pixels) */
    int32_t blocks;        /* N * tiles */
} tmr_mask_head_plan_t;

/* stream: a hipStream_t.  Return TMR_OK or a TMR_E_* code of tmr.h. */

/* Packs w1 / w2 into wpack (two small launches; once per weight version).
 * Reads w1, w2, wpack and C of args. */
int tmr_mask_head_prep(const tmr_mask_head_args_t *args, void *stream);

/* One launch: masks = the rule above.  w1 / w2 are not read. */
int tmr_mask_head(const tmr_mask_head_args_t *args, void *stream);

/* The launch geometry tmr_mask_head(args) would use, from the host: the same
 * validation (tmr_mask_head itself decides through it), nothing launched, no
 * buffer dereferenced.  Returns what tmr_mask_head returns before its launch;
 * on TMR_OK (N = 0 included, whatever the pointers) the plan is filled in,
 * otherwise it is zero. */
int tmr_mask_head_plan(const tmr_mask_head_args_t *args, tmr_mask_head_plan_t *plan);

#ifdef __cplusplus
}
#endif
#endif /* TMR_MASKHEAD_H_ */
