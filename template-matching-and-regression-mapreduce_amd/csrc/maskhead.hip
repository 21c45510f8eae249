// The fused mask head of the SAM mask decoder (include/tmr_maskhead.h;
// reference utils/segment_anything/modeling/mask_decoder.py:101-103, 149-156),
// gfx950.
//
// Both transposed convolutions have kernel = stride = 2: an embedding pixel
// produces its own 4x4 block of the low-resolution mask through two small
// GEMMs, and nothing overlaps.  One kernel reads src once and writes the
// [N][4h][4w] masks once; the [N,64,2h,2w] and [N,32,4h,4w] tensors of the
// stock module never exist.
//
// GEMM orientation: the WEIGHTS are the MFMA A operand (rows = output
// columns of the layer), the pixels are the 16 columns of the B operand.  The
// accumulator of v_mfma_f32_16x16x32_f16 then has its pixel on the lane
// (lane & 15) and its output channels in (lane >> 4, register), so
//   - the LayerNorm over the 64 channels of a (k, l) group is a sum over 16
//     registers and two cross-lane steps (xor 16, xor 32);
//   - stage 2 sums over stage 1's ROW index, so the activated accumulator is
//     stage 2's B operand as it stands, no lane movement and no LDS: the K
//     order this implies (o = 16 (2 st + (e >> 2)) + 4 grp + (e & 3)) is the
//     order tmr_mask_head_prep packs W2's K in;
//   - the dot with hyper[n] is again registers + xor 16, xor 32.
//
// Block: 4 waves, one prompt, 128 consecutive embedding pixels (wave: 32 = two
// B column tiles, so every weight fragment read from LDS feeds two pixel
// tiles).  A wave holds its 32 src rows in registers (128 fp32), takes each
// row's power-of-two scale from them and splits hi / lo per K step.  The packed
// weights stream through a double-buffered 32-KiB LDS stage, one chunk per K
// step (global -> registers -> LDS, one barrier per step); W2's chunk rides
// the same pipeline as "step 8".  Stage 1: 16 row tiles x 8 K steps x 3 terms
// x 2 pixel tiles; stage 2 per (k, l): 8 row tiles x 2 K steps x 3 x 2.
//
// 3-term split: x.w ~= (wh xh + wl xh + wh xl) / (s_x s_w), as conv_split.hip.
#include "tmr_common.h"

#include "../../include/tmr_maskhead.h"

namespace {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int NT = 256;            // threads per block
constexpr int TILE = 128;          // embedding pixels per block
constexpr int C = 256;             // transformer_dim
constexpr int KS = C / 32;         // K steps of stage 1
constexpr int CHUNK = 32768;       // bytes of one packed chunk
constexpr int CHUNK_V = CHUNK / 16;  // uint4 per chunk
constexpr int NCHUNK = KS + 1;     // + W2
constexpr int LDS_BYTES = 2 * CHUNK;
constexpr int H_MAX = 16384, W_MAX = 1024;  // 4h, 4w within tmr_mask_boxes' limits
static_assert(TMR_MASK_HEAD_WPACK_BYTES == NCHUNK * CHUNK + 64, "header out of sync");

// power of two s with v * s < 2^14 (conv_split.hip split_scale)
__device__ __forceinline__ float pow2_scale(float v) {
    if (!(v > 0.0f && v <= 3.0e38f)) return 1.0f;
    int e;
    frexpf(v, &e);  // v < 2^e
    return ldexpf(1.0f, min(max(14 - e, -63), 63));
}

// erf without a branch: 1 - exp(-t q(t)), t = min(|x|, 4) (erfc(4) = 1.5e-8 is below fp32's
// spacing at 1), q the degree-10 least-squares fit on Chebyshev nodes of -ln(erfc(t)) / t over
// [0, 4].  Absolute error of the fp32 evaluation <= 1e-7 against float64 erf on [0, 6] (2 000 001
// points), beside the exp's own rounding; the library erff is a two-branch routine of ~30
// instructions, which made every GELU a basic block of its own.  gelu(x) = x/2 (1 + erf(x / sqrt 2))
// then holds to ~2e-7 |x|.  A NaN x passes through the product below.
__device__ __forceinline__ float erf_nb(float x) {
    const float t = fminf(fabsf(x), 4.0f);
    float q = -9.946280954409303e-08f;
    q = fmaf(q, t, 2.5187375740642892e-06f);
    q = fmaf(q, t, -2.8390299121383578e-05f);
    q = fmaf(q, t, 0.00018635796732269228f);
    q = fmaf(q, t, -0.0007667069439776242f);
    q = fmaf(q, t, 0.0018134170677512884f);
    q = fmaf(q, t, -0.0002471829648129642f);
    q = fmaf(q, t, -0.019128648564219475f);
    q = fmaf(q, t, 0.10277583450078964f);
    q = fmaf(q, t, 0.6366192102432251f);
    q = fmaf(q, t, 1.128379225730896f);
    return copysignf(1.0f - __expf(-(t * q)), x);
}

__device__ __forceinline__ float gelu(float x) { return 0.5f * x * (1.0f + erf_nb(x * 0.70710678118654752440f)); }

__device__ __forceinline__ f32x4 mma(h8 a, h8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ float group_sum(float v) {  // over the 4 lane groups of a column
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 32);
    return v;
}
__device__ __forceinline__ float group_max(float v) {
    v = fmaxf(v, __shfl_xor(v, 16));
    v = fmaxf(v, __shfl_xor(v, 32));
    return v;
}

// ---------------------------------------------------------------- prep
// tail[0] = 1 / s1, tail[1] = 1 / s2, tail[2] = s1, tail[3] = s2
__global__ __launch_bounds__(1024) void mask_head_wmax_kernel(const float *__restrict__ w1,
                                                              const float *__restrict__ w2,
                                                              float *__restrict__ tail) {
    __shared__ float red[2][16];
    float m1 = 0.0f, m2 = 0.0f;
    for (int i = threadIdx.x; i < C * (C / 4) * 4; i += 1024) m1 = fmaxf(m1, fabsf(w1[i]));
    for (int i = threadIdx.x; i < (C / 4) * (C / 8) * 4; i += 1024) m2 = fmaxf(m2, fabsf(w2[i]));
    for (int o = 32; o > 0; o >>= 1) {
        m1 = fmaxf(m1, __shfl_xor(m1, o));
        m2 = fmaxf(m2, __shfl_xor(m2, o));
    }
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = m1;
        red[1][threadIdx.x >> 6] = m2;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < 16; ++i) {
            m1 = fmaxf(m1, red[0][i]);
            m2 = fmaxf(m2, red[1][i]);
        }
        const float s1 = pow2_scale(m1), s2 = pow2_scale(m2);
        tail[0] = 1.0f / s1;
        tail[1] = 1.0f / s2;
        tail[2] = s1;
        tail[3] = s2;
        for (int i = 4; i < 16; ++i) tail[i] = 0.0f;
    }
}

// one thread per (fragment pair, lane): the hi and the lo 16-B pieces
__global__ __launch_bounds__(NT) void mask_head_pack_kernel(const float *__restrict__ w1,
                                                            const float *__restrict__ w2,
                                                            char *__restrict__ wpack) {
    const int t = blockIdx.x * NT + threadIdx.x;  // < NCHUNK * 16 * 64
    if (t >= NCHUNK * 16 * 64) return;
    const float *tail = reinterpret_cast<const float *>(wpack + (size_t)NCHUNK * CHUNK);
    const int lane = t & 63, fp = (t >> 6) & 15, ch = t >> 10;
    const int row = lane & 15, grp = lane >> 4;
    float v[8];
    float s;
    if (ch < KS) {  // W1[c][o][k][l], fragment pair fp = row tile T
        s = tail[2];
        const int R = 16 * fp + row, kl = R >> 6, o = R & 63;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int c = 32 * ch + 8 * grp + e;
            v[e] = w1[((size_t)c * 64 + o) * 4 + kl];
        }
    } else {  // W2[o][q][m][j], fragment pair fp = T * 2 + st
        s = tail[3];
        const int T = fp >> 1, st = fp & 1;
        const int R = 16 * T + row, mj = R >> 5, q = R & 31;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int o = 16 * (2 * st + (e >> 2)) + 4 * grp + (e & 3);
            v[e] = w2[((size_t)o * 32 + q) * 4 + mj];
        }
    }
    h8 hi, lo;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float xs = v[e] * s;
        const _Float16 hh = (_Float16)xs;
        hi[e] = hh;
        lo[e] = (_Float16)(xs - (float)hh);
    }
    h8 *dst = reinterpret_cast<h8 *>(wpack + (size_t)ch * CHUNK + (size_t)fp * 2048);
    dst[lane] = hi;
    dst[64 + lane] = lo;
}

// ---------------------------------------------------------------- the head
struct MArgs {
    const float *src, *hyper, *b1, *g, *beta, *b2;
    const uint4 *wpack;
    float *masks;
    int h, w, hw, tiles;
    float eps;
};

__device__ __forceinline__ void split8(const float (&x)[8], h8 &hi, h8 &lo) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const _Float16 hh = (_Float16)x[e];
        hi[e] = hh;
        lo[e] = (_Float16)(x[e] - (float)hh);
    }
}

__global__ __launch_bounds__(NT) void mask_head_kernel(MArgs a) {
    __shared__ uint4 wbuf[2][CHUNK_V];

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int col = lane & 15, grp = lane >> 4;
    const int64_t n = blockIdx.x / a.tiles;
    const int tile = blockIdx.x % a.tiles;
    const int pbase = tile * TILE + wv * 32;

    // the wave's 32 src rows: lane (grp, col) holds channels 32 ks + 8 grp + e of
    // pixel pbase + 16 pt + col (rows past the plane repeat its last pixel)
    float xs[2][KS][8];
#pragma unroll
    for (int pt = 0; pt < 2; ++pt) {
        const int p = min(pbase + 16 * pt + col, a.hw - 1);
        const float4 *row = reinterpret_cast<const float4 *>(a.src + (n * a.hw + p) * C) + 2 * grp;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const float4 lo4 = row[8 * ks], hi4 = row[8 * ks + 1];
            xs[pt][ks][0] = lo4.x; xs[pt][ks][1] = lo4.y; xs[pt][ks][2] = lo4.z; xs[pt][ks][3] = lo4.w;
            xs[pt][ks][4] = hi4.x; xs[pt][ks][5] = hi4.y; xs[pt][ks][6] = hi4.z; xs[pt][ks][7] = hi4.w;
        }
    }
    // chunk 0 -> LDS
    uint4 stage[CHUNK_V / NT];
#pragma unroll
    for (int i = 0; i < CHUNK_V / NT; ++i) stage[i] = a.wpack[i * NT + tid];
#pragma unroll
    for (int i = 0; i < CHUNK_V / NT; ++i) wbuf[0][i * NT + tid] = stage[i];

    const float *tail = reinterpret_cast<const float *>(a.wpack + (size_t)NCHUNK * CHUNK_V);
    const float inv_s1 = tail[0], inv_s2 = tail[1];

    // one power-of-two scale per src row (a NaN is skipped by fmaxf and stays a
    // NaN in the operand; an infinity gives scale 1 and a NaN lo part)
    float inv1[2];
#pragma unroll
    for (int pt = 0; pt < 2; ++pt) {
        float m = 0.0f;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
#pragma unroll
            for (int e = 0; e < 8; ++e) m = fmaxf(m, fabsf(xs[pt][ks][e]));
        const float s = pow2_scale(group_max(m));
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
#pragma unroll
            for (int e = 0; e < 8; ++e) xs[pt][ks][e] *= s;
        inv1[pt] = (1.0f / s) * inv_s1;
    }
    __syncthreads();

    // ------------------------------------------------------------ stage 1
    f32x4 acc[2][16];
#pragma unroll
    for (int pt = 0; pt < 2; ++pt)
#pragma unroll
        for (int T = 0; T < 16; ++T) acc[pt][T] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        const uint4 *nxt = a.wpack + (size_t)(ks + 1) * CHUNK_V;  // ks + 1 = KS: W2's chunk
#pragma unroll
        for (int i = 0; i < CHUNK_V / NT; ++i) stage[i] = nxt[i * NT + tid];
        h8 bh[2], bl[2];
#pragma unroll
        for (int pt = 0; pt < 2; ++pt) split8(xs[pt][ks], bh[pt], bl[pt]);
        const h8 *wf = reinterpret_cast<const h8 *>(wbuf[ks & 1]) + lane;
#pragma unroll
        for (int T = 0; T < 16; ++T) {
            const h8 ah = wf[(2 * T) * 64], al = wf[(2 * T + 1) * 64];
#pragma unroll
            for (int pt = 0; pt < 2; ++pt) {
                acc[pt][T] = mma(ah, bh[pt], acc[pt][T]);
                acc[pt][T] = mma(al, bh[pt], acc[pt][T]);
                acc[pt][T] = mma(ah, bl[pt], acc[pt][T]);
            }
        }
#pragma unroll
        for (int i = 0; i < CHUNK_V / NT; ++i) wbuf[(ks + 1) & 1][i * NT + tid] = stage[i];
        __syncthreads();
    }

    // ------------------------------------------ epilogue 1, stage 2, epilogue 2
    // lane (grp, col), row tile t, register r: channel o = 16 t + 4 grp + r
    float hy[2][4], bq[2][4];
#pragma unroll
    for (int hf = 0; hf < 2; ++hf)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int q = 16 * hf + 4 * grp + r;
            hy[hf][r] = a.hyper[n * 32 + q];
            bq[hf][r] = a.b2[q];
        }
    const h8 *w2f = reinterpret_cast<const h8 *>(wbuf[KS & 1]) + lane;
    float outv[2][4] = {};  // [pt][2l + j] of the lane group's mask row

#pragma unroll
    for (int kl = 0; kl < 4; ++kl) {
        h8 ah2[2][2], al2[2][2];  // [pt][st]
        float inv2[2];
#pragma unroll
        for (int pt = 0; pt < 2; ++pt) {
            float u[4][4];
            float sum = 0.0f;
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    u[t][r] = acc[pt][kl * 4 + t][r] * inv1[pt] + a.b1[16 * t + 4 * grp + r];
                    sum += u[t][r];
                }
            const float mu = group_sum(sum) * (1.0f / 64.0f);
            float sq = 0.0f;
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    u[t][r] -= mu;
                    sq += u[t][r] * u[t][r];
                }
            const float rstd = 1.0f / sqrtf(group_sum(sq) * (1.0f / 64.0f) + a.eps);
            float m = 0.0f;
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int o = 16 * t + 4 * grp + r;
                    u[t][r] = gelu(a.g[o] * (u[t][r] * rstd) + a.beta[o]);
                    m = fmaxf(m, fabsf(u[t][r]));
                }
            const float s = pow2_scale(group_max(m));
            inv2[pt] = (1.0f / s) * inv_s2;
#pragma unroll
            for (int st = 0; st < 2; ++st) {
                float v[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = u[2 * st + (e >> 2)][e & 3] * s;
                split8(v, ah2[pt][st], al2[pt][st]);
            }
        }
        f32x4 acc2[2][8];
#pragma unroll
        for (int T = 0; T < 8; ++T) {
            acc2[0][T] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            acc2[1][T] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int st = 0; st < 2; ++st) {
                const h8 wh = w2f[((T * 2 + st) * 2) * 64], wl = w2f[((T * 2 + st) * 2 + 1) * 64];
#pragma unroll
                for (int pt = 0; pt < 2; ++pt) {
                    acc2[pt][T] = mma(wh, ah2[pt][st], acc2[pt][T]);
                    acc2[pt][T] = mma(wl, ah2[pt][st], acc2[pt][T]);
                    acc2[pt][T] = mma(wh, al2[pt][st], acc2[pt][T]);
                }
            }
        }
        // row tile T = 2 (2m + j) + hf, register r: q = 16 hf + 4 grp + r.  Lane group grp keeps
        // mask row 4y + grp of its pixel (k = grp >> 1, m = grp & 1): columns 2l + j
#pragma unroll
        for (int pt = 0; pt < 2; ++pt) {
            float d[4];
#pragma unroll
            for (int mj = 0; mj < 4; ++mj) {
                float part = 0.0f;
#pragma unroll
                for (int hf = 0; hf < 2; ++hf)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        part += hy[hf][r] * gelu(acc2[pt][2 * mj + hf][r] * inv2[pt] + bq[hf][r]);
                d[mj] = group_sum(part);
            }
            const float j0 = (grp & 1) ? d[2] : d[0], j1 = (grp & 1) ? d[3] : d[1];
            const bool mine = (grp >> 1) == (kl >> 1);
            outv[pt][2 * (kl & 1)] = mine ? j0 : outv[pt][2 * (kl & 1)];
            outv[pt][2 * (kl & 1) + 1] = mine ? j1 : outv[pt][2 * (kl & 1) + 1];
        }
    }

    // 16 consecutive pixels of an embedding row give 256 contiguous bytes per mask row
#pragma unroll
    for (int pt = 0; pt < 2; ++pt) {
        const int p = pbase + 16 * pt + col;
        const int y = p / a.w, x = p - y * a.w;
        if (p < a.hw) {
            float *dst = a.masks + ((n * 4 * a.h + 4 * y + grp) * (int64_t)(4 * a.w) + 4 * x);
            *reinterpret_cast<float4 *>(dst) = make_float4(outv[pt][0], outv[pt][1], outv[pt][2], outv[pt][3]);
        }
    }
}

bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

// The one statement of tmr_mask_head's validation and launch rule (host only:
// no buffer is dereferenced).  *launch stays false for the N = 0 no-op.
static int mask_head_plan(const tmr_mask_head_args_t *args, tmr_mask_head_plan_t *plan, bool *launch) {
    *launch = false;
    *plan = tmr_mask_head_plan_t{};
    TMR_REQUIRE(args);
    const tmr_mask_head_args_t &a = *args;
    if (a.C != C) return TMR_E_UNSUPPORTED;
    TMR_REQUIRE(a.N >= 0);
    TMR_REQUIRE(a.h >= 1 && a.h <= H_MAX && a.w >= 1 && a.w <= W_MAX);
    const int64_t hw = (int64_t)a.h * a.w;
    const int64_t tiles = tmr_cdiv(hw, TILE);
    TMR_REQUIRE(a.N * hw < (1ll << 31));
    TMR_REQUIRE(a.eps >= 0.0f);  // (a NaN eps fails)
    if (a.N > 0) {
        TMR_REQUIRE(a.src && a.hyper && a.wpack && a.b1 && a.g && a.beta && a.b2 && a.masks);
        TMR_REQUIRE(aligned16(a.src) && aligned16(a.wpack) && aligned16(a.masks));
    }
    plan->variant = TMR_MASK_HEAD_VARIANT_MFMA128;
    plan->tile_pixels = TILE;
    plan->threads = NT;
    plan->lds_bytes = LDS_BYTES;
    plan->tiles = (int32_t)tiles;
    plan->blocks = (int32_t)(a.N * tiles);
    *launch = a.N > 0;
    return TMR_OK;
}

extern "C" int tmr_mask_head_plan(const tmr_mask_head_args_t *args, tmr_mask_head_plan_t *plan) {
    TMR_REQUIRE(plan);
    bool launch;
    return mask_head_plan(args, plan, &launch);
}

extern "C" int tmr_mask_head_prep(const tmr_mask_head_args_t *args, void *stream) {
    TMR_REQUIRE(args);
    if (args->C != C) return TMR_E_UNSUPPORTED;
    TMR_REQUIRE(args->w1 && args->w2 && args->wpack && aligned16(args->wpack));
    hipStream_t s = tmr_stream(stream);
    char *wp = static_cast<char *>(args->wpack);
    hipLaunchKernelGGL(mask_head_wmax_kernel, dim3(1), dim3(1024), 0, s, args->w1, args->w2,
                       reinterpret_cast<float *>(wp + (size_t)NCHUNK * CHUNK));
    TMR_CHECK_LAUNCH();
    hipLaunchKernelGGL(mask_head_pack_kernel, dim3(NCHUNK * 16 * 64 / NT), dim3(NT), 0, s, args->w1, args->w2, wp);
    TMR_CHECK_LAUNCH();
    return TMR_OK;
}

extern "C" int tmr_mask_head(const tmr_mask_head_args_t *args, void *stream) {
    tmr_mask_head_plan_t plan;
    bool launch;
    const int rc = mask_head_plan(args, &plan, &launch);
    if (rc != TMR_OK || !launch) return rc;
    const tmr_mask_head_args_t &a = *args;
    MArgs m;
    m.src = a.src; m.hyper = a.hyper; m.b1 = a.b1; m.g = a.g; m.beta = a.beta; m.b2 = a.b2;
    m.wpack = static_cast<const uint4 *>(a.wpack);
    m.masks = a.masks;
    m.h = a.h; m.w = a.w; m.hw = a.h * a.w; m.tiles = plan.tiles;
    m.eps = a.eps;
    hipLaunchKernelGGL(mask_head_kernel, dim3((unsigned)plan.blocks), dim3(NT), 0, tmr_stream(stream), m);
    TMR_CHECK_LAUNCH();
    return TMR_OK;
}
