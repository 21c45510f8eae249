/* tmr_tokens.h -- the fifth optional extension of libtmr.so: the token side of
 * the SAM mask decoder (reference utils/segment_anything/modeling/
 * transformer.py:62-240 and mask_decoder.py:145-159), as three kernels that
 * replace the token-sized torch ops tmr_twoway.h leaves to its caller: self
 * attention, the MLP, the token-side norms, every projection and folding of the
 * two-way transformer, and the decoder's IoU and hypernetwork MLPs.
 *
 * Not part of the core ABI of tmr.h (TMR_ABI_VERSION is unchanged by it).
 *
 * WEIGHTS are raw pointers to the caller's live parameters: a linear layer's
 * weight is [out][in] row-major fp32, its bias [out]; a LayerNorm's g and b are
 * [C].  Nothing is packed, cached or version-tracked.
 *
 * LAYOUT.  C = 256 channels, H = 8 heads, T tokens per prompt, 1 <= T <= 8.
 * Tokens are [N][T][C] fp32.  Per-prompt operands keep the layout of
 * tmr_twoway.h: [N][64][C] (c: [N][64]) with row j = 8 h + t; the kernels here
 * WRITE rows with t >= T as 0.
 *
 * Below x = x[n], p = p[n] (the prompt's positional encoding: the point
 * embedding), I an attention's internal dimension, d = I / 8, and Att(q, k, v)
 * the stock Attention.forward: per head h, softmax over the T tokens of
 * q_proj(q)_h . k_proj(k)_h^T / sqrt(d), times v_proj(v)_h; heads concatenated;
 * out_proj.  norm is LayerNorm over C with the biased variance.
 *
 * tmr_tokens_front -- optional self-attention and norm1, then the queries of a
 * tokens -> image attention `cross`, folded:
 *   has_self_attn, skip_pe:   x1 = norm1(Att(x, x, x))          (no residual)
 *   has_self_attn, !skip_pe:  q = x + p;  x1 = norm1(x + Att(q, q, x))
 *   !has_self_attn:           x1 = x      (norm1 and self_attn are not read)
 *   qh = q_proj(x1 + p) / sqrt(d)
 *   qf[n][8h+t][c] = sum_e qh[t][h d + e] * Wk[h d + e][c]       (cross.k.w)
 * Outputs: x1 [N][T][C] (may be x itself), qf [N][64][C].  Of `cross` only q
 * (w, b) and k.w are read.
 *
 * tmr_tokens_back -- from the pooled context ctx [N][64][C] of that attention
 * (t2i) to the operands of the next image -> tokens attention (i2t):
 *   v[t][h d + e] = sum_c ctx[n][8h+t][c] * Wv[h d + e][c] + bv[h d + e]
 *   u = x1 + out_proj(v);  x2 = norm(u)
 *   has_mlp:  x3 = norm3(x2 + lin2(relu(lin1(x2))))
 *             kt = k_proj(x3 + p) / sqrt(d);  vt = v_proj(x3)           (i2t)
 *             A[n][8h+t][c] = sum_e kt[t][h d + e] * Wq[h d + e][c]
 *             c[n][8h+t]    = sum_e kt[t][h d + e] * bq[h d + e]
 *             B[n][8h+t][c] = sum_e Wo[c][h d + e] * vt[t][h d + e]
 *             outputs: x_out = x3, A, c, B
 *   !has_mlp: output x_out = x2 only (the final attention with norm_final_attn;
 *             lin1, lin2, norm3, i2t, A, c, B are not read or written)
 * Of t2i only v (w, b) and o (w, b) are read; of i2t k (w, b), v (w, b), q
 * (w, b) and o.w.  x_out may be x1 itself.
 *
 * tmr_tokens_tail -- the decoder's token-sized tail on hs [N][T][C], T >= 1 + M:
 *   iou_pred[n][:]     = MLP_iou(hs[n][0])         [N][M]
 *   hyper_all[n][i][:] = MLP_i(hs[n][1 + i])       [N][M][32],  i < M
 * Each MLP is Linear, ReLU, Linear, ReLU, Linear (no sigmoid).  The kernel
 * selects nothing: argmax and the gathers stay the caller's, so no discrete
 * decision depends on this kernel's rounding.
 *
 * Arithmetic: fp32 throughout.  Every matrix product runs on
 * v_mfma_f32_16x16x4_f32 (bit for bit an fp32 fmaf chain), 16 token rows per
 * tile: two prompts x 8 slots (front, back), 16 prompts of one MLP (tail).  A
 * tile's columns are independent and the order of every sum depends on the
 * shapes alone, so prompt n's results have the same bits alone and in a batch,
 * whatever its position.  exp is the library's expf.  ReLU is x < 0 ? 0 : x: a
 * NaN stays a NaN, as torch.relu has it.
 *
 * Non-finite values follow the rule's own IEEE arithmetic and stay with their
 * prompt: a non-finite value in prompt n's x, p or ctx reaches only prompt n's
 * outputs (a NaN in one token reaches every token of the prompt through the
 * self-attention, and one token's rows otherwise).
 *
 * Limits: C == 256, H == 8, T <= 8 (tail: M <= 8, any T), every attention with
 * in = out = C and I in {128, 256}, mlp_dim a multiple of 64 and <= 8192, the
 * tail's MLPs C -> hid -> hid -> out with hid a multiple of 32 and <= 256 and
 * out = M (IoU) or 32 (hypernetworks); else TMR_E_UNSUPPORTED.  T >= 1 (tail:
 * M >= 1, T >= 1 + M), 0 <= N <= 2^24, eps >= 0; with N > 0 every buffer and
 * every parameter that is read non-null and 16-B aligned; otherwise
 * TMR_E_INVALID.  N = 0 is a no-op.  One launch each, enqueued on `stream`;
 * nothing is allocated and nothing synchronises with the host.
 */
#ifndef TMR_TOKENS_H_
#define TMR_TOKENS_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TMR_TOKENS_MAX_MASKS 8      /* M <= 8 */
#define TMR_TOKENS_HYPER_OUT 32     /* a hypernetwork MLP's outputs */
#define TMR_TOKENS_MLP_CHUNK 512    /* hidden activations of the MLP kept in LDS at a time */

#define TMR_TOKENS_VARIANT_F32MFMA 0 /* exact fp32-input MFMA (v_mfma_f32_16x16x4_f32) */

typedef struct tmr_tok_linear {
    const float *w;  /* [out][in] */
    const float *b;  /* [out] */
    int32_t in, out;
} tmr_tok_linear_t;

typedef struct tmr_tok_attn {
    tmr_tok_linear_t q, k, v, o;
} tmr_tok_attn_t;

typedef struct tmr_tok_norm {
    const float *g;  /* [C] */
    const float *b;  /* [C] */
    float eps;
    int32_t pad_;
} tmr_tok_norm_t;

typedef struct tmr_tok_mlp3 {
    tmr_tok_linear_t l[3];
} tmr_tok_mlp3_t;

typedef struct tmr_tokens_front_args {
    const float *x;   /* [N][T][C] */
    const float *p;   /* [N][T][C] */
    float *x1;        /* out [N][T][C] */
    float *qf;        /* out [N][64][C] */
    tmr_tok_attn_t self_attn;
    tmr_tok_norm_t norm1;
    tmr_tok_attn_t cross;
    int64_t N;
    int32_t C, H, T;
    int32_t has_self_attn, skip_pe;
    int32_t pad_;
} tmr_tokens_front_args_t;

typedef struct tmr_tokens_back_args {
    const float *x1;   /* [N][T][C] */
    const float *p;    /* [N][T][C] */
    const float *ctx;  /* [N][64][C] */
    float *x_out;      /* out [N][T][C] */
    float *A;          /* out [N][64][C] */
    float *c;          /* out [N][64] */
    float *B;          /* out [N][64][C] */
    tmr_tok_attn_t t2i;
    tmr_tok_norm_t norm;
    tmr_tok_linear_t lin1, lin2;
    tmr_tok_norm_t norm3;
    tmr_tok_attn_t i2t;
    int64_t N;
    int32_t C, H, T;
    int32_t has_mlp;
} tmr_tokens_back_args_t;

typedef struct tmr_tokens_tail_args {
    const float *hs;   /* [N][T][C] */
    float *iou_pred;   /* out [N][M] */
    float *hyper_all;  /* out [N][M][32] */
    tmr_tok_mlp3_t iou;
    tmr_tok_mlp3_t hyper[TMR_TOKENS_MAX_MASKS];  /* the first M are read */
    int64_t N;
    int32_t C, T, M;
    int32_t pad_;
} tmr_tokens_tail_args_t;

typedef struct tmr_tokens_plan {
    int32_t variant;            /* TMR_TOKENS_VARIANT_* */
    int32_t threads;
    int32_t lds_bytes;
    int32_t blocks;
    int32_t prompts_per_block;  /* front, back: 2; tail: 16 (per MLP) */
    int32_t pad_;
} tmr_tokens_plan_t;

/* stream: a hipStream_t.  Return TMR_OK or a TMR_E_* code of tmr.h. */
int tmr_tokens_front(const tmr_tokens_front_args_t *args, void *stream);
int tmr_tokens_back(const tmr_tokens_back_args_t *args, void *stream);
int tmr_tokens_tail(const tmr_tokens_tail_args_t *args, void *stream);

/* The launch geometry the three calls would use, from the host: the same
 * validation (the launches decide through these), nothing launched, no buffer
 * dereferenced.  They return what the launch returns before launching; on
 * TMR_OK (N = 0 included, whatever the pointers) the plan is filled in,
 * otherwise it is zero. */
int tmr_tokens_front_plan(const tmr_tokens_front_args_t *args, tmr_tokens_plan_t *plan);
int tmr_tokens_back_plan(const tmr_tokens_back_args_t *args, tmr_tokens_plan_t *plan);
int tmr_tokens_tail_plan(const tmr_tokens_tail_args_t *args, tmr_tokens_plan_t *plan);

#ifdef __cplusplus
}
#endif
#endif /* TMR_TOKENS_H_ */
