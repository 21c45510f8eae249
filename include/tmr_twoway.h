/* tmr_twoway.h -- the fourth optional extension of libtmr.so: the image side of
 * the SAM mask decoder's two-way transformer (reference utils/segment_anything/
 * modeling/transformer.py:62-240), as two kernels that see no projection
 * weights.
 *
 * Not part of the core ABI of tmr.h (TMR_ABI_VERSION is unchanged by it).
 * Self-attention, the MLP, the token-side norms and every projection stay the
 * caller's (token-sized) torch ops; both cross-attentions are folded so that
 * the image side needs only per-prompt [64][256] operands:
 *
 *   tokens -> image:  qf[n][8h+t][:] = (q_proj(q)[n][t][head h] . Wk_h) / sqrt(d)
 *                     out_h = ctx[n][8h+t][:] . Wv_h^T + bv_h      (k_proj's bias
 *                     is constant over the pixels and cancels in the softmax)
 *   image -> tokens:  A[n][8h+t][:] = k_proj(q)[n][t][head h] . Wq_h / sqrt(d)
 *                     c[n][8h+t]    = k_proj(q)[n][t][head h] . bq_h / sqrt(d)
 *                     B[n][8h+t][:] = Wo[:, head h] . v_proj(q)[n][t][head h]
 *
 * OPERAND LAYOUT.  C = 256 channels, H = 8 heads, T tokens per prompt,
 * 1 <= T <= 8.  A per-prompt operand is [N][64][256] fp32 (c: [N][64]) with
 * row j = 8 h + t.  Rows with t >= T are ABSENT: they are never read and take
 * no part in a softmax.  One head's tokens are then 8 consecutive accumulator
 * rows of a 16x16 MFMA tile.
 *
 * tmr_twoway_pool -- attention pooling of the raw keys.  n' = n, or 0 when
 * Nk = 1 (layer 0's keys are shared by every prompt):
 *   s[n][j][p]   = sum_c qf[n][j][c] * (keys[n'][p][c] + pe[p][c])
 *   a[n][j][.]   = softmax over the P pixels of s[n][j][.]
 *   ctx[n][j][c] = sum_p a[n][j][p] * keys[n'][p][c]
 * Absent rows of ctx are written as 0.  P is split into chunks of
 * TMR_TWOWAY_POOL_CHUNK pixels, one block per (prompt, chunk), each an online
 * softmax (running max and sum per row) whose partial goes to `work`
 * (TMR_TWOWAY_POOL_WORK_BYTES(N, P), 16-B aligned); a second small launch
 * combines the partials in chunk order.  No atomics; the chunking depends on P
 * alone, so prompt n's result has the same bits alone and in a batch.
 *
 * tmr_twoway_update -- cross attention image -> tokens + residual + LayerNorm,
 * one launch.  Per prompt n and pixel p, x = keys_in[n'][p][:]:
 *   s[j]  = c[n][j] + sum_c A[n][j][c] * (x[c] + pe[p][c])
 *   a[8h+t] = softmax over the T present tokens of head h
 *   y[c]  = bo[c] + sum_j a[j] * B[n][j][c]
 *   z     = x + y;  mu = mean_c z;  var = mean_c (z - mu)^2   (biased)
 *   keys_out[n][p][c] = g[c] * (z[c] - mu) / sqrt(var + eps) + beta[c]
 * keys_out may be keys_in when Nk = N: a row is read and written by the same
 * wave, read first.
 *
 * Precision: the fp32 contract (normwise <= 1e-5 against the rule in float64).
 * All four products run on v_mfma_f32_16x16x4_f32, whose result is bit for bit
 * an fp32 fmaf chain in K order; exp is the library's expf.
 *
 * Non-finite values follow the rule's own IEEE arithmetic:
 *   pool: a NaN in keys[n'] or pe makes every present row of ctx[n] NaN; a NaN
 *     in qf[n][j] makes row j NaN (the running max is taken with fmaxf, which
 *     drops NaNs: they reach the result through the exponentials and the
 *     sums, in every chunk, first to last).  An infinity makes NaN whatever the
 *     rule makes NaN.  A prompt whose inputs are all finite keeps the contract
 *     whatever other prompts hold (with Nk = 1 the shared keys reach everyone).
 *   update: a non-finite value in a pixel's x or pe row makes that output row
 *     NaN and no other; a NaN in a present row of A, c or B of prompt n makes
 *     every row of prompt n NaN and no other prompt's.
 *
 * Limits: C == 256, H == 8, T <= 8 (else TMR_E_UNSUPPORTED); T >= 1, N >= 0,
 * 1 <= P <= 2^24, N * P < 2^31 (pool: also 64 N < 2^31), Nk in {1, N}, eps >= 0, keys_out != keys_in
 * unless Nk == N; with N > 0 every buffer non-null and 16-B aligned; otherwise
 * TMR_E_INVALID.  N = 0 is a no-op.  Everything is enqueued on `stream`;
 * nothing synchronises with the host.
 */
#ifndef TMR_TWOWAY_H_
#define TMR_TWOWAY_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TMR_TWOWAY_ROWS 64          /* 8 heads x 8 token slots */
#define TMR_TWOWAY_POOL_CHUNK 512   /* pixels per pooling block */
/* per (prompt, chunk): a [64][256] partial context and 64 (max, sum) pairs */
#define TMR_TWOWAY_POOL_CHUNKS(P) (((int64_t)(P) + TMR_TWOWAY_POOL_CHUNK - 1) / TMR_TWOWAY_POOL_CHUNK)
#define TMR_TWOWAY_POOL_WORK_BYTES(N, P) \
    ((int64_t)(N) * TMR_TWOWAY_POOL_CHUNKS(P) * TMR_TWOWAY_ROWS * (256 + 2) * 4)

#define TMR_TWOWAY_VARIANT_F32MFMA 0 /* exact fp32-input MFMA (v_mfma_f32_16x16x4_f32) */

typedef struct tmr_twoway_pool_args {
    const float *keys;  /* [Nk][P][C] */
    const float *pe;    /* [P][C] */
    const float *qf;    /* [N][64][C] */
    float *ctx;         /* out [N][64][C] */
    void *work;         /* TMR_TWOWAY_POOL_WORK_BYTES(N, P) */
    int64_t N, Nk, P;
    int32_t C, H, T;
    int32_t pad_;
} tmr_twoway_pool_args_t;

typedef struct tmr_twoway_update_args {
    const float *keys_in;  /* [Nk][P][C] */
    const float *pe;       /* [P][C] */
    const float *A;        /* [N][64][C] */
    const float *c;        /* [N][64] */
    const float *B;        /* [N][64][C] */
    const float *bo;       /* [C] */
    const float *g;        /* [C] */
    const float *beta;     /* [C] */
    float *keys_out;       /* [N][P][C] */
    int64_t N, Nk, P;
    int32_t C, H, T;
    float eps;
} tmr_twoway_update_args_t;

typedef struct tmr_twoway_plan {
    int32_t variant;       /* TMR_TWOWAY_VARIANT_* */
    int32_t tile_pixels;   /* pixels per inner step of a block */
    int32_t chunk_pixels;  /* pixels per block */
    int32_t chunks;        /* blocks per prompt: ceil(P / chunk_pixels) */
    int32_t threads;
    int32_t lds_bytes;
    int32_t blocks;        /* N * chunks (pool: of the first launch; the second has 64 N blocks of 64) */
    int32_t pad_;
} tmr_twoway_plan_t;

/* stream: a hipStream_t.  Return TMR_OK or a TMR_E_* code of tmr.h. */

/* Two launches: the chunk partials, then their combination into ctx. */
int tmr_twoway_pool(const tmr_twoway_pool_args_t *args, void *stream);

/* One launch: keys_out = the update rule above. */
int tmr_twoway_update(const tmr_twoway_update_args_t *args, void *stream);

/* The launch geometry the two calls would use, from the host: the same
 * validation (the launches decide through these), nothing launched, no buffer
 * dereferenced.  They return what the launch returns before launching; on
 * TMR_OK (N = 0 included, whatever the pointers) the plan is filled in,
 * otherwise it is zero. */
int tmr_twoway_pool_plan(const tmr_twoway_pool_args_t *args, tmr_twoway_plan_t *plan);
int tmr_twoway_update_plan(const tmr_twoway_update_args_t *args, tmr_twoway_plan_t *plan);

#ifdef __cplusplus
}
#endif
#endif /* TMR_TWOWAY_H_ */
