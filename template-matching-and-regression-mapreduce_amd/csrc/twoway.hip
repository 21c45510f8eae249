// The image side of the SAM mask decoder's two-way transformer
// (include/tmr_twoway.h; reference utils/segment_anything/modeling/
// transformer.py:62-240), gfx950.
//
// Both cross-attentions are folded on the token side, so the
// kernels here see the raw keys, the positional encoding and per-prompt
// [64][256] operands (row 8 h + t) only.  Every product runs on
// v_mfma_f32_16x16x4_f32: lane (grp = lane >> 4, col = lane & 15) gives
// A[row col][k grp] and B[k grp][column col] and holds D[row 4 grp + r][column
// col] in register r.  The K order of a product is free as long as A and B
// agree on it, which is used twice in each kernel:
//   - an operand row read from memory as one float4 serves four K steps
//     (step e takes channel 16 kk + 4 grp + e);
//   - the first product's accumulator is the second product's B operand as it
//     stands (K step r takes the row 4 grp + r the lane already holds): the
//     softmax weights never move between lanes or through LDS.
//
// tmr_twoway_pool, block = (prompt, chunk of 512 pixels), 4 waves, wave w =
// rows 16 w .. 16 w + 15 (two heads).  Per tile of 32 pixels the block stages
// keys and keys + pe in LDS (row stride 260 floats: conflict-free for both read
// patterns); a wave computes S^T [32 pixels x 16 rows] (pixels = MFMA rows, so
// the two pixel tiles are independent accumulators), the online-softmax update
// per row (= per lane column: the rescale is a per-lane scalar), and
// ctx^T [256 x 16] += keys^T . P^T.  The wave's 16 rows of qf stay in 64
// registers.  Partials (ctx, max, sum) go to `work`; twoway_pool_combine_kernel
// merges the chunks in chunk order.
//
// tmr_twoway_update, block = (prompt, 256 pixels), 8 waves x 16 pixels x 2
// steps (two waves per SIMD; a first version with 4 waves x 4 steps was slower,
// DESIGN.md 4.11).  A[n] and B[n] stay resident in LDS (2 x 65 KiB) for the
// block's life; a lane loads its own pixel's x and pe as float4 straight from
// memory (they are the B operand of the first product AND the residual of the
// epilogue, same registers); the second step's loads are issued before the
// first step's products (the two steps are unrolled, so the last one
// prefetches nothing).  S [64 rows x 16 pixels] has a head's 8 tokens in two
// lanes' registers (one xor-16 step); Y^T [256 x 16 pixels] += B^T . a has the
// pixel on the lane, so the LayerNorm is 64 registers + xor 16, xor 32.
#include "tmr_common.h"

#include <math.h>

#include "../../include/tmr_twoway.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int C = 256;             // embedding_dim
constexpr int C4 = C / 4;
constexpr int HEADS = 8;
constexpr int ROWS = TMR_TWOWAY_ROWS;
constexpr int NT = 256;            // threads per block
constexpr int LDW = 260;           // LDS row stride, floats (1040 B: 16-B aligned, 4 banks off per row)
constexpr int P_TILE = 32;         // pool: pixels per step
constexpr int P_CHUNK = TMR_TWOWAY_POOL_CHUNK;
constexpr int POOL_LDS = 2 * P_TILE * LDW * 4;
constexpr int UNT = 512;           // update: threads per block
constexpr int U_STEP = UNT / 4;    // update: pixels per step (8 waves x 16)
constexpr int U_TILE = 256;        // update: pixels per block
constexpr int UPD_LDS = (2 * ROWS * LDW + 3 * C) * 4;
constexpr int64_t P_MAX = 1ll << 24;
static_assert(P_CHUNK % P_TILE == 0 && U_TILE % U_STEP == 0, "tiles divide chunks");
static_assert(UPD_LDS <= 160 * 1024 && 2 * POOL_LDS <= 160 * 1024, "LDS per CU");

__device__ __forceinline__ f32x4 mma(float a, float b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ float el(const float4 &v, int e) { return e == 0 ? v.x : e == 1 ? v.y : e == 2 ? v.z : v.w; }

// ---------------------------------------------------------------- pool
struct PoolArgs {
    const float4 *keys, *pe, *qf;
    float4 *wctx;   // [N][chunks][64][64] float4
    float2 *wml;    // [N][chunks][64] (max, sum)
    int64_t P;
    int chunks, T, shared;
};

__global__ __launch_bounds__(NT, 2) void twoway_pool_kernel(PoolArgs a) {
    extern __shared__ float4 lds4[];
    float *xs = reinterpret_cast<float *>(lds4);  // [P_TILE][LDW] keys
    float *xp = xs + P_TILE * LDW;                // [P_TILE][LDW] keys + pe

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int col = lane & 15, grp = lane >> 4;
    const int64_t n = blockIdx.x / a.chunks;
    const int ch = blockIdx.x % a.chunks;
    const int64_t p0 = (int64_t)ch * P_CHUNK;
    const int64_t p1 = min(a.P, p0 + P_CHUNK);
    const float4 *keys = a.keys + (a.shared ? 0 : n * a.P * C4);

    // the wave's 16 rows of qf: lane (grp, col) holds row 16 wv + col, channels 16 kk + 4 grp + e
    const int j = 16 * wv + col;
    const bool present = (j & 7) < a.T;
    float4 q[16];
    {
        const float4 *qrow = a.qf + (n * ROWS + j) * C4 + grp;
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) q[kk] = present ? qrow[4 * kk] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }

    f32x4 acc[16];  // ctx^T: channel 16 ct + 4 grp + r, row j
#pragma unroll
    for (int ct = 0; ct < 16; ++ct) acc[ct] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    float M = -INFINITY, L = 0.0f;

    for (int64_t tb = p0; tb < p1; tb += P_TILE) {
        __syncthreads();  // the previous tile's reads
#pragma unroll
        for (int i = 0; i < P_TILE * C4 / NT; ++i) {
            const int idx = i * NT + tid, r = idx >> 6, c4 = idx & 63;
            const int64_t p = tb + r;
            float4 x = make_float4(0.0f, 0.0f, 0.0f, 0.0f), e = x;
            if (p < p1) {
                x = keys[p * C4 + c4];
                e = a.pe[p * C4 + c4];
            }
            *reinterpret_cast<float4 *>(xs + r * LDW + 4 * c4) = x;
            *reinterpret_cast<float4 *>(xp + r * LDW + 4 * c4) = make_float4(x.x + e.x, x.y + e.y, x.z + e.z, x.w + e.w);
        }
        __syncthreads();

        // S^T: pixel tb + 16 pt + 4 grp + r (rows), row j (column)
        f32x4 s[2] = {f32x4{0.0f, 0.0f, 0.0f, 0.0f}, f32x4{0.0f, 0.0f, 0.0f, 0.0f}};
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) {
            float4 av[2];
#pragma unroll
            for (int pt = 0; pt < 2; ++pt)
                av[pt] = *reinterpret_cast<const float4 *>(xp + (16 * pt + col) * LDW + 16 * kk + 4 * grp);
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int pt = 0; pt < 2; ++pt) s[pt] = mma(el(av[pt], e), el(q[kk], e), s[pt]);
        }

        // the online softmax of row j over this tile's pixels
        float mt = -INFINITY;
#pragma unroll
        for (int pt = 0; pt < 2; ++pt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (tb + 16 * pt + 4 * grp + r >= p1) s[pt][r] = -INFINITY;
                mt = fmaxf(mt, s[pt][r]);
            }
        mt = fmaxf(mt, __shfl_xor(mt, 16));
        mt = fmaxf(mt, __shfl_xor(mt, 32));
        const float Mn = fmaxf(M, mt);
        const float sc = expf(M - Mn);
        float ls = 0.0f;
#pragma unroll
        for (int pt = 0; pt < 2; ++pt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                s[pt][r] = expf(s[pt][r] - Mn);  // a NaN score stays a NaN here and in both sums
                ls += s[pt][r];
            }
        ls += __shfl_xor(ls, 16);
        ls += __shfl_xor(ls, 32);
        L = L * sc + ls;
        M = Mn;
#pragma unroll
        for (int ct = 0; ct < 16; ++ct) acc[ct] *= sc;

        // ctx^T += keys^T . P^T: K step (pt, r) is pixel 16 pt + 4 grp + r
#pragma unroll
        for (int pt = 0; pt < 2; ++pt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float *xr = xs + (16 * pt + 4 * grp + r) * LDW + col;
#pragma unroll
                for (int ct = 0; ct < 16; ++ct) acc[ct] = mma(xr[16 * ct], s[pt][r], acc[ct]);
            }
    }

    const int64_t slot = (n * a.chunks + ch) * ROWS + j;
#pragma unroll
    for (int ct = 0; ct < 16; ++ct)
        a.wctx[slot * C4 + 4 * ct + grp] = make_float4(acc[ct][0], acc[ct][1], acc[ct][2], acc[ct][3]);
    if (grp == 0) a.wml[slot] = make_float2(M, L);
}

// one block of 64 threads per (prompt, row); thread = 4 channels; chunks in order
__global__ __launch_bounds__(64) void twoway_pool_combine_kernel(const float4 *__restrict__ wctx,
                                                                 const float2 *__restrict__ wml,
                                                                 float4 *__restrict__ ctx, int chunks, int T) {
    const int j = blockIdx.x & (ROWS - 1);
    const int64_t n = blockIdx.x >> 6;
    const int c4 = threadIdx.x;
    float4 *out = ctx + (n * ROWS + j) * C4 + c4;
    if ((j & 7) >= T) {
        *out = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        return;
    }
    float M = -INFINITY;
    for (int k = 0; k < chunks; ++k) M = fmaxf(M, wml[(n * chunks + k) * ROWS + j].x);
    float4 sum = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float L = 0.0f;
    for (int k = 0; k < chunks; ++k) {
        const int64_t slot = (n * chunks + k) * ROWS + j;
        const float2 ml = wml[slot];
        const float w = expf(ml.x - M);
        const float4 v = wctx[slot * C4 + c4];
        L += w * ml.y;
        sum.x += w * v.x;
        sum.y += w * v.y;
        sum.z += w * v.z;
        sum.w += w * v.w;
    }
    *out = make_float4(sum.x / L, sum.y / L, sum.z / L, sum.w / L);
}

// ---------------------------------------------------------------- update
struct UpdArgs {
    const float4 *x, *pe, *A, *B, *bo, *g, *beta;
    const float *c;
    float4 *out;
    int64_t P;
    int tiles, T, shared;
    float eps;
};

__global__ __launch_bounds__(UNT) void twoway_update_kernel(UpdArgs a) {
    extern __shared__ float4 lds4[];
    float *As = reinterpret_cast<float *>(lds4);  // [64][LDW]
    float *Bs = As + ROWS * LDW;                  // [64][LDW]
    float *vs = Bs + ROWS * LDW;                  // bo, g, beta

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int col = lane & 15, grp = lane >> 4;
    const int64_t n = blockIdx.x / a.tiles;
    const int tl = blockIdx.x % a.tiles;

    // A[n], B[n] -> LDS; absent rows are not read
#pragma unroll 4
    for (int i = 0; i < ROWS * C4 / UNT; ++i) {
        const int idx = i * UNT + tid, r = idx >> 6, c4 = idx & 63;
        float4 va = make_float4(0.0f, 0.0f, 0.0f, 0.0f), vb = va;
        if ((r & 7) < a.T) {
            va = a.A[(n * ROWS + r) * C4 + c4];
            vb = a.B[(n * ROWS + r) * C4 + c4];
        }
        *reinterpret_cast<float4 *>(As + r * LDW + 4 * c4) = va;
        *reinterpret_cast<float4 *>(Bs + r * LDW + 4 * c4) = vb;
    }
    if (tid < 3 * C4) {
        const float4 *src = tid < C4 ? a.bo : tid < 2 * C4 ? a.g : a.beta;
        reinterpret_cast<float4 *>(vs)[tid] = src[tid & (C4 - 1)];
    }

    // row j = 16 jt + 4 grp + r: token t = 4 (grp & 1) + r of head 2 jt + (grp >> 1)
    float cj[4][4];
    bool pr[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        pr[r] = 4 * (grp & 1) + r < a.T;
#pragma unroll
        for (int jt = 0; jt < 4; ++jt) cj[jt][r] = pr[r] ? a.c[n * ROWS + 16 * jt + 4 * grp + r] : 0.0f;
    }
    __syncthreads();

    const float4 *xin = a.x + (a.shared ? 0 : n * a.P * C4);
    float4 *xout = a.out + n * a.P * C4;
    const int64_t pblock = (int64_t)tl * U_TILE + wv * 16;

    // lane (grp, col): pixel pbase + col, channels 16 kk + 4 grp + e
    float4 xc[16], ec[16];
    {
        const int64_t p = min(pblock + col, a.P - 1);
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) {
            xc[kk] = xin[p * C4 + 4 * kk + grp];
            ec[kk] = a.pe[p * C4 + 4 * kk + grp];
        }
    }

#pragma unroll
    for (int it = 0; it < U_TILE / U_STEP; ++it) {
        const int64_t pbase = pblock + (int64_t)it * U_STEP;
        if (pbase >= a.P) break;  // wave-uniform; no barrier below
        float4 xn[16], en[16];
        // the loop is unrolled, so the last step's prefetch does not exist; a next step past P (no
        // branch here: one would pin all 32 loads at the top and spill) reads the one row P - 1
        if (it + 1 < U_TILE / U_STEP) {
            const int64_t p = min(pbase + U_STEP + col, a.P - 1);
#pragma unroll
            for (int kk = 0; kk < 16; ++kk) {
                xn[kk] = xin[p * C4 + 4 * kk + grp];
                en[kk] = a.pe[p * C4 + 4 * kk + grp];
            }
        }

        // S: row 16 jt + 4 grp + r, pixel col
        f32x4 s[4];
#pragma unroll
        for (int jt = 0; jt < 4; ++jt) s[jt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) {
            const float4 b = make_float4(xc[kk].x + ec[kk].x, xc[kk].y + ec[kk].y, xc[kk].z + ec[kk].z,
                                         xc[kk].w + ec[kk].w);
            float4 av[4];
#pragma unroll
            for (int jt = 0; jt < 4; ++jt)
                av[jt] = *reinterpret_cast<const float4 *>(As + (16 * jt + col) * LDW + 16 * kk + 4 * grp);
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int jt = 0; jt < 4; ++jt) s[jt] = mma(el(av[jt], e), el(b, e), s[jt]);
        }

        // softmax over each head's present tokens: 4 registers x lanes (grp, grp ^ 1)
#pragma unroll
        for (int jt = 0; jt < 4; ++jt) {
            float m = -INFINITY;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                s[jt][r] = pr[r] ? cj[jt][r] + s[jt][r] : -INFINITY;
                m = fmaxf(m, s[jt][r]);
            }
            m = fmaxf(m, __shfl_xor(m, 16));
            float sum = 0.0f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                s[jt][r] = expf(s[jt][r] - m);
                sum += s[jt][r];
            }
            sum += __shfl_xor(sum, 16);
            const float inv = 1.0f / sum;
#pragma unroll
            for (int r = 0; r < 4; ++r) s[jt][r] *= inv;
        }

        // Y^T: channel 16 ct + 4 grp + r, pixel col; K step (jt, r) is row 16 jt + 4 grp + r
        f32x4 y[16];
#pragma unroll
        for (int ct = 0; ct < 16; ++ct) {
            const float4 b = *reinterpret_cast<const float4 *>(vs + 16 * ct + 4 * grp);
            y[ct] = f32x4{b.x, b.y, b.z, b.w};
        }
#pragma unroll
        for (int jt = 0; jt < 4; ++jt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float *br = Bs + (16 * jt + 4 * grp + r) * LDW + col;
#pragma unroll
                for (int ct = 0; ct < 16; ++ct) y[ct] = mma(br[16 * ct], s[jt][r], y[ct]);
            }

        // z = x + y, LayerNorm over the 256 channels of the lane's pixel
        float sum = 0.0f;
#pragma unroll
        for (int ct = 0; ct < 16; ++ct) {
            y[ct][0] += xc[ct].x;
            y[ct][1] += xc[ct].y;
            y[ct][2] += xc[ct].z;
            y[ct][3] += xc[ct].w;
            sum += (y[ct][0] + y[ct][1]) + (y[ct][2] + y[ct][3]);
        }
        sum += __shfl_xor(sum, 16);
        sum += __shfl_xor(sum, 32);
        const float mu = sum * (1.0f / C);
        float sq = 0.0f;
#pragma unroll
        for (int ct = 0; ct < 16; ++ct)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                y[ct][r] -= mu;
                sq += y[ct][r] * y[ct][r];
            }
        sq += __shfl_xor(sq, 16);
        sq += __shfl_xor(sq, 32);
        const float rstd = 1.0f / sqrtf(sq * (1.0f / C) + a.eps);
        if (pbase + col < a.P) {
            float4 *dst = xout + (pbase + col) * C4 + grp;
#pragma unroll
            for (int ct = 0; ct < 16; ++ct) {
                const float4 gg = *reinterpret_cast<const float4 *>(vs + C + 16 * ct + 4 * grp);
                const float4 bb = *reinterpret_cast<const float4 *>(vs + 2 * C + 16 * ct + 4 * grp);
                dst[4 * ct] = make_float4(gg.x * (y[ct][0] * rstd) + bb.x, gg.y * (y[ct][1] * rstd) + bb.y,
                                          gg.z * (y[ct][2] * rstd) + bb.z, gg.w * (y[ct][3] * rstd) + bb.w);
            }
        }
        if (it + 1 < U_TILE / U_STEP) {
#pragma unroll
            for (int kk = 0; kk < 16; ++kk) {
                xc[kk] = xn[kk];
                ec[kk] = en[kk];
            }
        }
    }
}

bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// what both calls share: C, H, T, N, Nk, P
int check_dims(int64_t N, int64_t Nk, int64_t P, int c, int h, int t) {
    if (c != C || h != HEADS || t > 8) return TMR_E_UNSUPPORTED;
    TMR_REQUIRE(t >= 1 && N >= 0 && P >= 1 && P <= P_MAX);
    TMR_REQUIRE(N * P < (1ll << 31));
    TMR_REQUIRE(Nk == 1 || Nk == N);
    return TMR_OK;
}

}  // namespace

// The one statement of each call's validation and launch rule (host only: no
// buffer is dereferenced).  *launch stays false for the N = 0 no-op.
static int pool_plan(const tmr_twoway_pool_args_t *args, tmr_twoway_plan_t *plan, bool *launch) {
    *launch = false;
    *plan = tmr_twoway_plan_t{};
    TMR_REQUIRE(args);
    const tmr_twoway_pool_args_t &a = *args;
    const int rc = check_dims(a.N, a.Nk, a.P, a.C, a.H, a.T);
    if (rc != TMR_OK) return rc;
    if (a.N > 0) {
        TMR_REQUIRE(a.keys && a.pe && a.qf && a.ctx && a.work);
        TMR_REQUIRE(aligned16(a.keys) && aligned16(a.pe) && aligned16(a.qf) && aligned16(a.ctx) && aligned16(a.work));
    }
    const int64_t chunks = TMR_TWOWAY_POOL_CHUNKS(a.P);
    TMR_REQUIRE(a.N * chunks < (1ll << 31));
    TMR_REQUIRE(a.N * ROWS < (1ll << 31));  // the combine launch's grid
    plan->variant = TMR_TWOWAY_VARIANT_F32MFMA;
    plan->tile_pixels = P_TILE;
    plan->chunk_pixels = P_CHUNK;
    plan->chunks = (int32_t)chunks;
    plan->threads = NT;
    plan->lds_bytes = POOL_LDS;
    plan->blocks = (int32_t)(a.N * chunks);
    *launch = a.N > 0;
    return TMR_OK;
}

static int update_plan(const tmr_twoway_update_args_t *args, tmr_twoway_plan_t *plan, bool *launch) {
    *launch = false;
    *plan = tmr_twoway_plan_t{};
    TMR_REQUIRE(args);
    const tmr_twoway_update_args_t &a = *args;
    const int rc = check_dims(a.N, a.Nk, a.P, a.C, a.H, a.T);
    if (rc != TMR_OK) return rc;
    TMR_REQUIRE(a.eps >= 0.0f);  // (a NaN eps fails)
    if (a.N > 0) {
        TMR_REQUIRE(a.keys_in && a.pe && a.A && a.c && a.B && a.bo && a.g && a.beta && a.keys_out);
        TMR_REQUIRE(aligned16(a.keys_in) && aligned16(a.pe) && aligned16(a.A) && aligned16(a.B) && aligned16(a.bo)
                    && aligned16(a.g) && aligned16(a.beta) && aligned16(a.keys_out));
        TMR_REQUIRE(a.keys_out != a.keys_in || a.Nk == a.N);
    }
    const int64_t chunks = tmr_cdiv(a.P, U_TILE);
    TMR_REQUIRE(a.N * chunks < (1ll << 31));
    plan->variant = TMR_TWOWAY_VARIANT_F32MFMA;
    plan->tile_pixels = U_STEP;
    plan->chunk_pixels = U_TILE;
    plan->chunks = (int32_t)chunks;
    plan->threads = UNT;
    plan->lds_bytes = UPD_LDS;
    plan->blocks = (int32_t)(a.N * chunks);
    *launch = a.N > 0;
    return TMR_OK;
}

extern "C" int tmr_twoway_pool_plan(const tmr_twoway_pool_args_t *args, tmr_twoway_plan_t *plan) {
    TMR_REQUIRE(plan);
    bool launch;
    return pool_plan(args, plan, &launch);
}

extern "C" int tmr_twoway_update_plan(const tmr_twoway_update_args_t *args, tmr_twoway_plan_t *plan) {
    TMR_REQUIRE(plan);
    bool launch;
    return update_plan(args, plan, &launch);
}

extern "C" int tmr_twoway_pool(const tmr_twoway_pool_args_t *args, void *stream) {
    tmr_twoway_plan_t plan;
    bool launch;
    const int rc = pool_plan(args, &plan, &launch);
    if (rc != TMR_OK || !launch) return rc;
    const tmr_twoway_pool_args_t &a = *args;
    PoolArgs k;
    k.keys = reinterpret_cast<const float4 *>(a.keys);
    k.pe = reinterpret_cast<const float4 *>(a.pe);
    k.qf = reinterpret_cast<const float4 *>(a.qf);
    k.wctx = static_cast<float4 *>(a.work);
    k.wml = reinterpret_cast<float2 *>(k.wctx + a.N * plan.chunks * ROWS * C4);
    k.P = a.P;
    k.chunks = plan.chunks;
    k.T = a.T;
    k.shared = (a.Nk == 1 && a.N != 1) ? 1 : 0;
    hipStream_t s = tmr_stream(stream);
    if (tmr_set_max_lds(reinterpret_cast<const void *>(twoway_pool_kernel), POOL_LDS) != hipSuccess) return TMR_E_HIP;
    hipLaunchKernelGGL(twoway_pool_kernel, dim3((unsigned)plan.blocks), dim3(NT), POOL_LDS, s, k);
    TMR_CHECK_LAUNCH();
    hipLaunchKernelGGL(twoway_pool_combine_kernel, dim3((unsigned)(a.N * ROWS)), dim3(64), 0, s, k.wctx, k.wml,
                       reinterpret_cast<float4 *>(a.ctx), plan.chunks, a.T);
    TMR_CHECK_LAUNCH();
    return TMR_OK;
}

extern "C" int tmr_twoway_update(const tmr_twoway_update_args_t *args, void *stream) {
    tmr_twoway_plan_t plan;
    bool launch;
    const int rc = update_plan(args, &plan, &launch);
    if (rc != TMR_OK || !launch) return rc;
    const tmr_twoway_update_args_t &a = *args;
    UpdArgs k;
    k.x = reinterpret_cast<const float4 *>(a.keys_in);
    k.pe = reinterpret_cast<const float4 *>(a.pe);
    k.A = reinterpret_cast<const float4 *>(a.A);
    k.B = reinterpret_cast<const float4 *>(a.B);
    k.bo = reinterpret_cast<const float4 *>(a.bo);
    k.g = reinterpret_cast<const float4 *>(a.g);
    k.beta = reinterpret_cast<const float4 *>(a.beta);
    k.c = a.c;
    k.out = reinterpret_cast<float4 *>(a.keys_out);
    k.P = a.P;
    k.tiles = plan.chunks;
    k.T = a.T;
    k.shared = (a.Nk == 1 && a.N != 1) ? 1 : 0;
    k.eps = a.eps;
    if (tmr_set_max_lds(reinterpret_cast<const void *>(twoway_update_kernel), UPD_LDS) != hipSuccess) return TMR_E_HIP;
    hipLaunchKernelGGL(twoway_update_kernel, dim3((unsigned)plan.blocks), dim3(UNT), UPD_LDS, tmr_stream(stream), k);
    TMR_CHECK_LAUNCH();
    return TMR_OK;
}
