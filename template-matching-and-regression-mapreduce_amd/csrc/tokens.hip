// The token side of the SAM mask decoder (include/tmr_tokens.h; reference
// utils/segment_anything/modeling/transformer.py:62-240, mask_decoder.py:145-159),
// gfx950.
//
// Everything here is a handful of [16 rows] x [out][in] products on live
// nn.Linear weights.  Every product runs on v_mfma_f32_16x16x4_f32 with the
// roles of twoway.hip: lane (grp = lane >> 4, col = lane & 15) gives
// A[row col][k grp] and B[k grp][column col] and holds D[row 4 grp + r][column
// col] in register r.  Here the MFMA rows are 16 OUTPUT CHANNELS and the MFMA
// columns the 16 TOKEN ROWS of a block: a lane reads its weight row
// W[o0 + col][.] and its token row X[col][.] as one float4 per four K steps
// (step e takes channel 16 kk + 4 grp + e on both sides) and ends with four
// consecutive output channels of one token row.  A column of D depends on its
// own column of B alone, so a token row never sees another row's values: that
// is the batch independence and the containment of non-finite values the
// header promises.  Two accumulators (even and odd kk) hide the MFMA's
// dependent latency; the order of the sum depends on K alone.
//
// front, back: block = two prompts x 8 token slots (row 8 pp + t), 16 waves, the
// 16 x 256 activations in LDS (row stride 260 floats); a wave takes every 16th
// tile of 16 output channels.  Absent rows (t >= T, or a prompt past N) are
// zero-filled on load, carry finite junk through the stages and are never
// stored, except as the zeros the layout asks for.  back keeps the MLP's hidden
// activations in LDS in chunks of TMR_TOKENS_MLP_CHUNK; a wave's lin2 tile
// stays in its registers across the chunks.
// tail: block = (16 prompts, one of the 1 + M MLPs).
#include "tmr_common.h"

#include <math.h>

#include "../../include/tmr_tokens.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int C = 256;             // embedding_dim
constexpr int C4 = C / 4;
constexpr int HEADS = 8;
constexpr int SLOTS = 8;           // token slots per head
constexpr int ROWS = 16;           // token rows per block
constexpr int NT = 1024;           // threads per block: 16 waves, four per SIMD
constexpr int NW = NT / 64;
constexpr int LD = 260;            // LDS row stride, floats (as twoway.hip)
constexpr int CHUNK = TMR_TOKENS_MLP_CHUNK;
constexpr int LDH = CHUNK + 4;
constexpr int BUF = ROWS * LD;     // one [16][256] activation buffer, floats
constexpr int FRONT_LDS = 7 * BUF * 4;
constexpr int BACK_LDS = (5 * BUF + ROWS * LDH) * 4;
constexpr int TAIL_LDS = 3 * BUF * 4;
constexpr int64_t N_MAX = 1ll << 24;
static_assert(FRONT_LDS <= 160 * 1024 && BACK_LDS <= 160 * 1024, "LDS per CU");
constexpr int TPW = C / 16 / NW;    // lin2 tiles of 16 output channels per wave
static_assert(TPW * NW * 16 == C, "the waves share lin2's tiles evenly");

__device__ __forceinline__ f32x4 mma(float a, float b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ float el(const float4 &v, int e) { return e == 0 ? v.x : e == 1 ? v.y : e == 2 ? v.z : v.w; }

__device__ __forceinline__ float4 ld4(const float *p) { return *reinterpret_cast<const float4 *>(p); }

__device__ __forceinline__ float relu(float v) { return v < 0.0f ? 0.0f : v; }  // a NaN stays a NaN

// One tile: D[o0 + 4 grp + r][row col] = sum_{k < K} W[o0 + col][k] * X[row col][k], K % 16 == 0.
// w = the lane's weight row + 4 grp, x = the lane's token row + 4 grp.  No load is predicated: a lane
// whose channel or token row does not exist is pointed at one that does, and its row or column of D
// (which depends on nothing else, and nothing else on it) is dropped by the caller.
__device__ __forceinline__ f32x4 tile(const float *w, const float *x, int K) {
    f32x4 a0 = {0.0f, 0.0f, 0.0f, 0.0f}, a1 = a0;
    const int nk = K >> 4;
#pragma unroll 4
    for (int i = 0; i < (nk >> 1); ++i) {
        const int kk = 2 * i;
        const float4 w0 = ld4(w + 16 * kk), w1 = ld4(w + 16 * kk + 16);
        const float4 x0 = ld4(x + 16 * kk), x1 = ld4(x + 16 * kk + 16);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            a0 = mma(el(w0, e), el(x0, e), a0);
            a1 = mma(el(w1, e), el(x1, e), a1);
        }
    }
    if (nk & 1) {
        const int kk = nk - 1;
        const float4 w0 = ld4(w + 16 * kk), x0 = ld4(x + 16 * kk);
#pragma unroll
        for (int e = 0; e < 4; ++e) a0 = mma(el(w0, e), el(x0, e), a0);
    }
    return a0 + a1;
}

// The same tile on a weight read across its rows: D[o0 + 4 grp + r][row col] =
// sum_{k < K} Wt[k][o0 + col] * X[row col][k], K in {16, 32}.  wt = Wt + grp * ldw + o0 + col,
// x = the lane's token row + grp; K step s takes k = 4 s + grp.
__device__ __forceinline__ f32x4 tile_t(const float *wt, int ldw, const float *x, int K) {
    f32x4 a0 = {0.0f, 0.0f, 0.0f, 0.0f}, a1 = a0;
    for (int s = 0; s < (K >> 2); s += 2) {
        a0 = mma(wt[(int64_t)(4 * s) * ldw], x[4 * s], a0);
        a1 = mma(wt[(int64_t)(4 * s + 4) * ldw], x[4 * s + 4], a1);
    }
    return a0 + a1;
}

// Y = X . W^T over the block's 16 rows: wave wv takes the tiles o0 = 16 (wv + NW i) < out and hands
// epi(o, row, v) the four channels o .. o + 3 of token row `row` (channels >= out hold junk).
template <class Epi>
__device__ __forceinline__ void linear16(const float *X, int ldx, const float *W, int ldw, int K, int out, Epi epi) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, col = lane & 15, grp = lane >> 4;
    for (int o0 = 16 * wv; o0 < out; o0 += 16 * NW) {
        const bool wok = o0 + col < out;
        const f32x4 v = tile(W + (int64_t)(wok ? o0 + col : 0) * ldw + 4 * grp, X + col * ldx + 4 * grp, K);
        epi(o0 + 4 * grp, col, v);
    }
}

__device__ __forceinline__ float4 bias4(const float *b, int o) { return *reinterpret_cast<const float4 *>(b + o); }

__device__ __forceinline__ void st4(float *p, float a, float b, float c, float d) {
    *reinterpret_cast<float4 *>(p) = make_float4(a, b, c, d);
}

__device__ __forceinline__ float wave_sum(float s) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m);
    return s;
}

// LayerNorm of the 16 rows of Z (in place allowed): one wave per row, a lane has 4 channels
__device__ __forceinline__ void norm16(const float *Z, float *Y, const tmr_tok_norm_t &nm) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const float4 g = bias4(nm.g, 4 * lane), b = bias4(nm.b, 4 * lane);
    for (int r = wv; r < ROWS; r += NW) {
        const float4 z = *reinterpret_cast<const float4 *>(Z + r * LD + 4 * lane);
        const float mu = wave_sum((z.x + z.y) + (z.z + z.w)) * (1.0f / C);
        const float dx = z.x - mu, dy = z.y - mu, dz = z.z - mu, dw = z.w - mu;
        const float var = wave_sum((dx * dx + dy * dy) + (dz * dz + dw * dw)) * (1.0f / C);
        const float sd = sqrtf(var + nm.eps);
        st4(Y + r * LD + 4 * lane, g.x * (dx / sd) + b.x, g.y * (dy / sd) + b.y, g.z * (dz / sd) + b.z,
            g.w * (dw / sd) + b.w);
    }
}

// the block's 16 token rows of a [N][T][C] tensor into LDS, absent rows as zeros
__device__ __forceinline__ void load_rows(const float *src, float *dst, int64_t n0, int64_t N, int T) {
    for (int idx = threadIdx.x; idx < ROWS * C4; idx += NT) {
        const int r = idx >> 6, c4 = idx & 63, t = r & 7;
        const int64_t n = n0 + (r >> 3);
        const bool ok = n < N && t < T;
        const float4 v = ld4(src + ((ok ? n * T + t : 0) * C4 + c4) * 4);
        *reinterpret_cast<float4 *>(dst + r * LD + 4 * c4) = ok ? v : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
}

// the present rows of an LDS buffer to a [N][T][C] tensor; with P also Q = S + P (every row)
__device__ __forceinline__ void store_rows(const float *S, float *dst, const float *P, float *Q, int64_t n0, int64_t N,
                                           int T) {
    for (int idx = threadIdx.x; idx < ROWS * C4; idx += NT) {
        const int r = idx >> 6, c4 = idx & 63, t = r & 7;
        const int64_t n = n0 + (r >> 3);
        const float4 v = *reinterpret_cast<const float4 *>(S + r * LD + 4 * c4);
        if (n < N && t < T) *reinterpret_cast<float4 *>(dst + ((n * T + t) * C4 + c4) * 4) = v;
        if (P) {
            const float4 p = *reinterpret_cast<const float4 *>(P + r * LD + 4 * c4);
            st4(Q + r * LD + 4 * c4, v.x + p.x, v.y + p.y, v.z + p.z, v.w + p.w);
        }
    }
}

// out[n][8 h + t][o0 ..] over all (head, 16-channel tile) items: `item(h, o0)` gives the lane's tile;
// rows t >= T are written as 0, prompts past N not at all
template <class Item>
__device__ __forceinline__ void fold_rows(float *out, int64_t n0, int64_t N, int T, Item item) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, col = lane & 15, grp = lane >> 4;
    const int64_t n = n0 + (col >> 3);
    const int t = col & 7;
    for (int it = wv; it < HEADS * (C / 16); it += NW) {
        const int h = it >> 4, o0 = (it & 15) * 16;
        f32x4 v = item(h, o0);
        if (t >= T) v = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        if (n < N) st4(out + ((n * 64 + 8 * h + t) * C + o0 + 4 * grp), v[0], v[1], v[2], v[3]);
    }
}

// ---------------------------------------------------------------- front
__global__ __launch_bounds__(NT) void tokens_front_kernel(tmr_tokens_front_args_t a) {
    extern __shared__ float4 lds4[];
    float *XS = reinterpret_cast<float *>(lds4);  // x
    float *PS = XS + BUF;                         // p
    float *QS = PS + BUF;                         // x or x + p; later x1 + p
    float *Qb = QS + BUF;                         // q_proj; then the heads' outputs
    float *Kb = Qb + BUF;                         // k_proj; later qh
    float *Vb = Kb + BUF;                         // v_proj
    float *U = Vb + BUF;                          // x1

    const int tid = threadIdx.x, lane = tid & 63, col = lane & 15, grp = lane >> 4;
    const int64_t n0 = 2 * (int64_t)blockIdx.x;
    const int T = a.T;

    load_rows(a.x, XS, n0, a.N, T);
    load_rows(a.p, PS, n0, a.N, T);
    __syncthreads();
    const float *X1 = XS;
    if (a.has_self_attn) {
        const tmr_tok_attn_t &sa = a.self_attn;
        const int I = sa.q.out, d = I / HEADS;
        const float *qin = XS;
        if (!a.skip_pe) {
            store_rows(XS, nullptr, PS, QS, 0, 0, 0);  // QS = x + p
            __syncthreads();
            qin = QS;
        }
        auto plain = [&](float *Y, const float *b) {
            return [=](int o, int row, f32x4 v) {
                const float4 bb = bias4(b, o);
                st4(Y + row * LD + o, v[0] + bb.x, v[1] + bb.y, v[2] + bb.z, v[3] + bb.w);
            };
        };
        linear16(qin, LD, sa.q.w, C, C, I, plain(Qb, sa.q.b));
        linear16(qin, LD, sa.k.w, C, C, I, plain(Kb, sa.k.b));
        linear16(XS, LD, sa.v.w, C, C, I, plain(Vb, sa.v.b));
        __syncthreads();
        if (tid < ROWS * HEADS) {  // one (row, head): T scores, their softmax, d outputs (over the head's q)
            const int r = tid >> 3, h = tid & 7, r0 = r & 8;
            float *q = Qb + r * LD + h * d;
            const float scale = sqrtf((float)d);
            float s[SLOTS], m = -INFINITY;
#pragma unroll
            for (int t = 0; t < SLOTS; ++t) {
                s[t] = 0.0f;
                if (t < T) {
                    const float *k = Kb + (r0 + t) * LD + h * d;
                    float acc = 0.0f;
                    for (int e = 0; e < d; ++e) acc = fmaf(q[e], k[e], acc);
                    s[t] = acc / scale;
                    m = fmaxf(m, s[t]);
                }
            }
            float sum = 0.0f;
#pragma unroll
            for (int t = 0; t < SLOTS; ++t)
                if (t < T) {
                    s[t] = expf(s[t] - m);
                    sum += s[t];
                }
#pragma unroll
            for (int t = 0; t < SLOTS; ++t) s[t] = s[t] / sum;
            for (int e = 0; e < d; ++e) {
                float acc = 0.0f;
#pragma unroll
                for (int t = 0; t < SLOTS; ++t)
                    if (t < T) acc = fmaf(s[t], Vb[(r0 + t) * LD + h * d + e], acc);
                q[e] = acc;
            }
        }
        __syncthreads();
        const bool residual = !a.skip_pe;
        linear16(Qb, LD, sa.o.w, I, I, C, [=](int o, int row, f32x4 v) {
            const float4 bb = bias4(sa.o.b, o);
            float4 x = *reinterpret_cast<const float4 *>(XS + row * LD + o);
            if (!residual) x = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            st4(U + row * LD + o, x.x + (v[0] + bb.x), x.y + (v[1] + bb.y), x.z + (v[2] + bb.z), x.w + (v[3] + bb.w));
        });
        __syncthreads();
        norm16(U, U, a.norm1);
        __syncthreads();
        X1 = U;
    }
    store_rows(X1, a.x1, PS, QS, n0, a.N, T);  // x1 out; QS = x1 + p
    __syncthreads();
    const int d = a.cross.q.out / HEADS;
    {
        const float scale = sqrtf((float)d);
        const float *b = a.cross.q.b;
        linear16(QS, LD, a.cross.q.w, C, C, a.cross.q.out, [=](int o, int row, f32x4 v) {
            const float4 bb = bias4(b, o);
            st4(Kb + row * LD + o, (v[0] + bb.x) / scale, (v[1] + bb.y) / scale, (v[2] + bb.z) / scale,
                (v[3] + bb.w) / scale);
        });
    }
    __syncthreads();
    const float *Wk = a.cross.k.w;
    fold_rows(a.qf, n0, a.N, T, [=](int h, int o0) {
        return tile_t(Wk + (int64_t)(h * d + grp) * C + o0 + col, C, Kb + col * LD + h * d + grp, d);
    });
}

// ---------------------------------------------------------------- back
__global__ __launch_bounds__(NT) void tokens_back_kernel(tmr_tokens_back_args_t a) {
    extern __shared__ float4 lds4[];
    float *XS = reinterpret_cast<float *>(lds4);  // x1; later x3 + p
    float *PS = XS + BUF;                         // p
    float *VS = PS + BUF;                         // the attention's values; later kt
    float *Z = VS + BUF;                          // u, x2; later vt
    float *Y = Z + BUF;                           // x3
    float *HB = Y + BUF;                          // [16][LDH]: a chunk of the MLP's hidden activations

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, col = lane & 15, grp = lane >> 4;
    const int64_t n0 = 2 * (int64_t)blockIdx.x;
    const int T = a.T;

    load_rows(a.x1, XS, n0, a.N, T);
    load_rows(a.p, PS, n0, a.N, T);
    {   // v = ctx_h . Wv_h^T + bv_h: the lane's token row of head h's tile is ctx[n][8 h + t][.], read once
        const int I = a.t2i.v.out, d = I / HEADS;
        const int64_t n = n0 + (col >> 3);
        const int t = col & 7;
        const bool xok = n < a.N && t < T;
        for (int o0 = 16 * wv; o0 < I; o0 += 16 * NW) {
            const int h = o0 / d;
            const f32x4 v = tile(a.t2i.v.w + (int64_t)(o0 + col) * C + 4 * grp,
                                 a.ctx + ((xok ? n * 64 + 8 * h + t : 0) * C + 4 * grp), C);
            const int o = o0 + 4 * grp;
            const float4 bb = bias4(a.t2i.v.b, o);
            st4(VS + col * LD + o, v[0] + bb.x, v[1] + bb.y, v[2] + bb.z, v[3] + bb.w);
        }
    }
    __syncthreads();
    {
        const float *b = a.t2i.o.b;
        linear16(VS, LD, a.t2i.o.w, a.t2i.o.in, a.t2i.o.in, C, [=](int o, int row, f32x4 v) {
            const float4 bb = bias4(b, o);
            const float4 x = *reinterpret_cast<const float4 *>(XS + row * LD + o);
            st4(Z + row * LD + o, x.x + (v[0] + bb.x), x.y + (v[1] + bb.y), x.z + (v[2] + bb.z), x.w + (v[3] + bb.w));
        });
    }
    __syncthreads();
    norm16(Z, Z, a.norm);  // x2
    __syncthreads();
    if (!a.has_mlp) {
        store_rows(Z, a.x_out, nullptr, nullptr, n0, a.N, T);
        return;
    }
    {   // x3 = norm3(x2 + lin2(relu(lin1(x2)))), the hidden activations a chunk at a time
        const int Dm = a.lin1.out;
        f32x4 y[TPW];
#pragma unroll
        for (int i = 0; i < TPW; ++i) y[i] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        for (int c0 = 0; c0 < Dm; c0 += CHUNK) {
            const int cw = min(CHUNK, Dm - c0);
            const float *b1 = a.lin1.b + c0;
            linear16(Z, LD, a.lin1.w + (int64_t)c0 * C, C, C, cw, [=](int o, int row, f32x4 v) {
                const float4 bb = bias4(b1, o);
                st4(HB + row * LDH + o, relu(v[0] + bb.x), relu(v[1] + bb.y), relu(v[2] + bb.z), relu(v[3] + bb.w));
            });
            __syncthreads();
#pragma unroll
            for (int i = 0; i < TPW; ++i) {
                const int o0 = 16 * (wv + NW * i);
                y[i] += tile(a.lin2.w + (int64_t)(o0 + col) * Dm + c0 + 4 * grp, HB + col * LDH + 4 * grp, cw);
            }
            __syncthreads();
        }
#pragma unroll
        for (int i = 0; i < TPW; ++i) {
            const int o = 16 * (wv + NW * i) + 4 * grp;
            const float4 bb = bias4(a.lin2.b, o);
            const float4 x = *reinterpret_cast<const float4 *>(Z + col * LD + o);
            st4(Y + col * LD + o, x.x + (y[i][0] + bb.x), x.y + (y[i][1] + bb.y), x.z + (y[i][2] + bb.z),
                x.w + (y[i][3] + bb.w));
        }
    }
    __syncthreads();
    norm16(Y, Y, a.norm3);  // x3
    __syncthreads();
    store_rows(Y, a.x_out, PS, XS, n0, a.N, T);  // x3 out; XS = x3 + p
    __syncthreads();
    const int I = a.i2t.k.out, d = I / HEADS;
    {
        const float scale = sqrtf((float)d);
        const float *bk = a.i2t.k.b, *bv = a.i2t.v.b;
        linear16(XS, LD, a.i2t.k.w, C, C, I, [=](int o, int row, f32x4 v) {
            const float4 bb = bias4(bk, o);
            st4(VS + row * LD + o, (v[0] + bb.x) / scale, (v[1] + bb.y) / scale, (v[2] + bb.z) / scale,
                (v[3] + bb.w) / scale);
        });
        linear16(Y, LD, a.i2t.v.w, C, C, I, [=](int o, int row, f32x4 v) {
            const float4 bb = bias4(bv, o);
            st4(Z + row * LD + o, v[0] + bb.x, v[1] + bb.y, v[2] + bb.z, v[3] + bb.w);
        });
    }
    __syncthreads();
    const float *Wq = a.i2t.q.w, *Wo = a.i2t.o.w;
    fold_rows(a.A, n0, a.N, T, [=](int h, int o0) {
        return tile_t(Wq + (int64_t)(h * d + grp) * C + o0 + col, C, VS + col * LD + h * d + grp, d);
    });
    fold_rows(a.B, n0, a.N, T, [=](int h, int o0) {
        return tile(Wo + (int64_t)(o0 + col) * I + h * d + 4 * grp, Z + col * LD + h * d + 4 * grp, d);
    });
    if (tid < ROWS * HEADS) {
        const int r = tid >> 3, h = tid & 7, t = r & 7;
        const int64_t n = n0 + (r >> 3);
        float acc = 0.0f;
        for (int e = 0; e < d; ++e) acc = fmaf(VS[r * LD + h * d + e], a.i2t.q.b[h * d + e], acc);
        if (n < a.N) a.c[n * 64 + 8 * h + t] = t < T ? acc : 0.0f;
    }
}

// ---------------------------------------------------------------- tail
__global__ __launch_bounds__(NT) void tokens_tail_kernel(tmr_tokens_tail_args_t a) {
    extern __shared__ float4 lds4[];
    float *X = reinterpret_cast<float *>(lds4);
    float *H1 = X + BUF;
    float *H2 = H1 + BUF;

    const int which = blockIdx.y;  // 0: the IoU head on token 0; 1 + i: hypernetwork i on token 1 + i
    const tmr_tok_mlp3_t &mlp = which == 0 ? a.iou : a.hyper[which - 1];
    const int64_t n0 = (int64_t)ROWS * blockIdx.x;
    for (int idx = threadIdx.x; idx < ROWS * C4; idx += NT) {
        const int r = idx >> 6, c4 = idx & 63;
        const int64_t n = n0 + r;
        const bool ok = n < a.N;
        const float4 v = ld4(a.hs + ((ok ? n * a.T + which : 0) * C4 + c4) * 4);
        *reinterpret_cast<float4 *>(X + r * LD + 4 * c4) = ok ? v : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    __syncthreads();
    auto hidden = [](float *Yb, const float *b) {
        return [=](int o, int row, f32x4 v) {
            const float4 bb = bias4(b, o);
            st4(Yb + row * LD + o, relu(v[0] + bb.x), relu(v[1] + bb.y), relu(v[2] + bb.z), relu(v[3] + bb.w));
        };
    };
    linear16(X, LD, mlp.l[0].w, C, C, mlp.l[0].out, hidden(H1, mlp.l[0].b));
    __syncthreads();
    linear16(H1, LD, mlp.l[1].w, mlp.l[1].in, mlp.l[1].in, mlp.l[1].out, hidden(H2, mlp.l[1].b));
    __syncthreads();
    const int out = mlp.l[2].out;
    const float *b = mlp.l[2].b;
    float *dst = which == 0 ? a.iou_pred : a.hyper_all + (int64_t)(which - 1) * TMR_TOKENS_HYPER_OUT;
    const int64_t stride = which == 0 ? a.M : (int64_t)a.M * TMR_TOKENS_HYPER_OUT;
    const int64_t N = a.N;
    linear16(H2, LD, mlp.l[2].w, mlp.l[2].in, mlp.l[2].in, out, [=](int o, int row, f32x4 v) {
        const int64_t n = n0 + row;
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (n < N && o + r < out) dst[n * stride + o + r] = v[r] + b[o + r];
    });
}

// ---------------------------------------------------------------- host
bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
bool buf_ok(const void *p) { return p && aligned16(p); }
bool lin_ok(const tmr_tok_linear_t &l) { return buf_ok(l.w) && buf_ok(l.b); }
bool norm_ok(const tmr_tok_norm_t &n) { return buf_ok(n.g) && buf_ok(n.b); }

bool attn_supported(const tmr_tok_attn_t &t) {
    const int I = t.q.out;
    return (I == 128 || I == 256) && t.q.in == C && t.k.in == C && t.v.in == C && t.o.out == C && t.k.out == I
           && t.v.out == I && t.o.in == I;
}

int check_dims(int64_t N, int c, int h, int t) {
    if (c != C || h != HEADS || t > SLOTS) return TMR_E_UNSUPPORTED;
    TMR_REQUIRE(t >= 1 && N >= 0 && N <= N_MAX);
    return TMR_OK;
}

void fill_plan(tmr_tokens_plan_t *plan, int lds, int64_t blocks, int per_block) {
    plan->variant = TMR_TOKENS_VARIANT_F32MFMA;
    plan->threads = NT;
    plan->lds_bytes = lds;
    plan->blocks = (int32_t)blocks;
    plan->prompts_per_block = per_block;
}

}  // namespace

// The one statement of each call's validation and launch rule (host only: no
// buffer is dereferenced).  *launch stays false for the N = 0 no-op.
static int front_plan(const tmr_tokens_front_args_t *args, tmr_tokens_plan_t *plan, bool *launch) {
    *launch = false;
    *plan = tmr_tokens_plan_t{};
    TMR_REQUIRE(args);
    const tmr_tokens_front_args_t &a = *args;
    if (!attn_supported(a.cross) || (a.has_self_attn && !attn_supported(a.self_attn))) return TMR_E_UNSUPPORTED;
    const int rc = check_dims(a.N, a.C, a.H, a.T);
    if (rc != TMR_OK) return rc;
    if (a.has_self_attn) TMR_REQUIRE(a.norm1.eps >= 0.0f);  // (a NaN eps fails)
    if (a.N > 0) {
        TMR_REQUIRE(buf_ok(a.x) && buf_ok(a.p) && buf_ok(a.x1) && buf_ok(a.qf));
        TMR_REQUIRE(lin_ok(a.cross.q) && buf_ok(a.cross.k.w));
        if (a.has_self_attn)
            TMR_REQUIRE(lin_ok(a.self_attn.q) && lin_ok(a.self_attn.k) && lin_ok(a.self_attn.v) && lin_ok(a.self_attn.o)
                        && norm_ok(a.norm1));
    }
    fill_plan(plan, FRONT_LDS, tmr_cdiv(a.N, 2), 2);
    *launch = a.N > 0;
    return TMR_OK;
}

static int back_plan(const tmr_tokens_back_args_t *args, tmr_tokens_plan_t *plan, bool *launch) {
    *launch = false;
    *plan = tmr_tokens_plan_t{};
    TMR_REQUIRE(args);
    const tmr_tokens_back_args_t &a = *args;
    if (!attn_supported(a.t2i)) return TMR_E_UNSUPPORTED;
    if (a.has_mlp) {
        const int Dm = a.lin1.out;
        if (!attn_supported(a.i2t) || a.lin1.in != C || a.lin2.out != C || a.lin2.in != Dm || Dm < 64 || Dm % 64
            || Dm > 8192)
            return TMR_E_UNSUPPORTED;
    }
    const int rc = check_dims(a.N, a.C, a.H, a.T);
    if (rc != TMR_OK) return rc;
    TMR_REQUIRE(a.norm.eps >= 0.0f && (!a.has_mlp || a.norm3.eps >= 0.0f));
    if (a.N > 0) {
        TMR_REQUIRE(buf_ok(a.x1) && buf_ok(a.p) && buf_ok(a.ctx) && buf_ok(a.x_out));
        TMR_REQUIRE(lin_ok(a.t2i.v) && lin_ok(a.t2i.o) && norm_ok(a.norm));
        if (a.has_mlp) {
            TMR_REQUIRE(buf_ok(a.A) && buf_ok(a.c) && buf_ok(a.B));
            TMR_REQUIRE(lin_ok(a.lin1) && lin_ok(a.lin2) && norm_ok(a.norm3));
            TMR_REQUIRE(lin_ok(a.i2t.k) && lin_ok(a.i2t.v) && lin_ok(a.i2t.q) && buf_ok(a.i2t.o.w));
        }
    }
    fill_plan(plan, BACK_LDS, tmr_cdiv(a.N, 2), 2);
    *launch = a.N > 0;
    return TMR_OK;
}

static int tail_plan(const tmr_tokens_tail_args_t *args, tmr_tokens_plan_t *plan, bool *launch) {
    *launch = false;
    *plan = tmr_tokens_plan_t{};
    TMR_REQUIRE(args);
    const tmr_tokens_tail_args_t &a = *args;
    if (a.C != C || a.M > TMR_TOKENS_MAX_MASKS) return TMR_E_UNSUPPORTED;
    TMR_REQUIRE(a.M >= 1 && a.T >= 1 + a.M && a.N >= 0 && a.N <= N_MAX);
    for (int i = 0; i <= a.M; ++i) {
        const tmr_tok_mlp3_t &m = i == 0 ? a.iou : a.hyper[i - 1];
        const int h0 = m.l[0].out, h1 = m.l[1].out;
        if (m.l[0].in != C || m.l[1].in != h0 || m.l[2].in != h1 || h0 < 32 || h0 % 32 || h0 > C || h1 < 32 || h1 % 32
            || h1 > C || m.l[2].out != (i == 0 ? a.M : TMR_TOKENS_HYPER_OUT))
            return TMR_E_UNSUPPORTED;
    }
    if (a.N > 0) {
        TMR_REQUIRE(buf_ok(a.hs) && buf_ok(a.iou_pred) && buf_ok(a.hyper_all));
        for (int i = 0; i <= a.M; ++i) {
            const tmr_tok_mlp3_t &m = i == 0 ? a.iou : a.hyper[i - 1];
            TMR_REQUIRE(lin_ok(m.l[0]) && lin_ok(m.l[1]) && lin_ok(m.l[2]));
        }
    }
    fill_plan(plan, TAIL_LDS, tmr_cdiv(a.N, ROWS) * (1 + a.M), ROWS);
    *launch = a.N > 0;
    return TMR_OK;
}

extern "C" int tmr_tokens_front_plan(const tmr_tokens_front_args_t *args, tmr_tokens_plan_t *plan) {
    TMR_REQUIRE(plan);
    bool launch;
    return front_plan(args, plan, &launch);
}

extern "C" int tmr_tokens_back_plan(const tmr_tokens_back_args_t *args, tmr_tokens_plan_t *plan) {
    TMR_REQUIRE(plan);
    bool launch;
    return back_plan(args, plan, &launch);
}

extern "C" int tmr_tokens_tail_plan(const tmr_tokens_tail_args_t *args, tmr_tokens_plan_t *plan) {
    TMR_REQUIRE(plan);
    bool launch;
    return tail_plan(args, plan, &launch);
}

extern "C" int tmr_tokens_front(const tmr_tokens_front_args_t *args, void *stream) {
    tmr_tokens_plan_t plan;
    bool launch;
    const int rc = front_plan(args, &plan, &launch);
    if (rc != TMR_OK || !launch) return rc;
    if (tmr_set_max_lds(reinterpret_cast<const void *>(tokens_front_kernel), FRONT_LDS) != hipSuccess) return TMR_E_HIP;
    hipLaunchKernelGGL(tokens_front_kernel, dim3((unsigned)plan.blocks), dim3(NT), FRONT_LDS, tmr_stream(stream), *args);
    TMR_CHECK_LAUNCH();
    return TMR_OK;
}

extern "C" int tmr_tokens_back(const tmr_tokens_back_args_t *args, void *stream) {
    tmr_tokens_plan_t plan;
    bool launch;
    const int rc = back_plan(args, &plan, &launch);
    if (rc != TMR_OK || !launch) return rc;
    if (tmr_set_max_lds(reinterpret_cast<const void *>(tokens_back_kernel), BACK_LDS) != hipSuccess) return TMR_E_HIP;
    hipLaunchKernelGGL(tokens_back_kernel, dim3((unsigned)plan.blocks), dim3(NT), BACK_LDS, tmr_stream(stream), *args);
    TMR_CHECK_LAUNCH();
    return TMR_OK;
}

extern "C" int tmr_tokens_tail(const tmr_tokens_tail_args_t *args, void *stream) {
    tmr_tokens_plan_t plan;
    bool launch;
    const int rc = tail_plan(args, &plan, &launch);
    if (rc != TMR_OK || !launch) return rc;
    const tmr_tokens_tail_args_t &a = *args;
    if (tmr_set_max_lds(reinterpret_cast<const void *>(tokens_tail_kernel), TAIL_LDS) != hipSuccess) return TMR_E_HIP;
    hipLaunchKernelGGL(tokens_tail_kernel, dim3((unsigned)tmr_cdiv(a.N, ROWS), (unsigned)(1 + a.M)), dim3(NT), TAIL_LDS,
                       tmr_stream(stream), a);
    TMR_CHECK_LAUNCH();
    return TMR_OK;
}
