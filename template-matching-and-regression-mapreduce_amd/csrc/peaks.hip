// Peak finder + box decode (gfx950): Get_pred_boxes for one level
// (utils/TM_utils.py:245-282) with adaptive_kernel_generater's 3x3 mask
// (:363-377) and custom_shape_3x3_maxpool2d (:337-361, zero padding).
//
//   peaks_kernel: one workgroup per unit, one pass: p = sigmoid(o)
//   (near-correctly rounded; or p = o) staged in LDS by row chunks, flags
//   p >= thr && p == masked 3x3 max, wave ballots + mbcnt + a workgroup scan
//   give each candidate its row-major slot (torch.where order, no cap), and
//   the candidate is decoded in place: ref = (x/W, y/H); xy = ref + r[:2]*s;
//   wh = exp(r[2:])*(bw,bh); box = (xy - wh/2, xy + wh/2).
// exp: the reference's torch.exp (ATen CPU -> MKL VML vsExp, high accuracy)
// restated as the correctly rounded value except at the inputs recorded in
// the reference-exp table (tmr_amd/exp_table.py), where MKL rounds to the
// other neighbour; without a table, correctly rounded.
// Built with -ffp-contract=off so every op is separately rounded as in the
// reference's elementwise torch ops.
#include "tmr_common.h"

namespace {

constexpr int EXP_HEADER = 128;  // tmr_amd/exp_table.py

struct ExpTable {
    const uint32_t *off;  // [65537] by the input's upper 16 bits
    const uint16_t *lo;   // sorted lower 16 bits of the recorded inputs
};

__device__ __forceinline__ float expf_ref(float x, ExpTable t) {
    const double e = exp((double)x);
    float y = (float)e;
    if (!t.off) return y;
    const uint32_t b = __float_as_uint(x);
    const uint32_t hb = b >> 16, key = b & 0xffffu;
    uint32_t s = t.off[hb], n = t.off[hb + 1];
    const uint32_t end = n;
    while (s < n) {  // lower bound of key in lo[s, end)
        const uint32_t m = (s + n) >> 1;
        if (t.lo[m] < key) s = m + 1; else n = m;
    }
    if (s < end && t.lo[s] == key)  // MKL rounded to the exact value's other side
        y = e > (double)y ? nextafterf(y, __builtin_inff()) : nextafterf(y, -__builtin_inff());
    return y;
}

// custom_shape_3x3_maxpool2d (TM_utils.py:337-361): per element, the max of
// the masked 3x3 neighbourhood (F.unfold's zero padding), taps in row-major
// order; a NaN propagates (torch.max) and a tie keeps the earlier tap.
__global__ void maxpool3x3_kernel(const float *__restrict__ x, int64_t n, int H, int W, int mask,
                                  float *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t hw = (int64_t)H * W;
    const int64_t pl = i / hw;
    const int r = (int)(i - pl * hw), y = r / W, xx = r % W;
    const float *p = x + pl * hw;
    float mx = 0.0f;
    bool first = true;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            if (!((mask >> ((dy + 1) * 3 + dx + 1)) & 1)) continue;
            const int yy = y + dy, xc = xx + dx;
            const float q = (yy < 0 || yy >= H || xc < 0 || xc >= W) ? 0.0f : p[yy * W + xc];
            if (first || q > mx || (q != q && mx == mx)) { mx = q; first = false; }
        }
    out[i] = mx;
}

// The probability map, chip-wide (one thread per 4 pixels): p = sigmoid(o)
// (near-correctly rounded), or o itself when the input is already p.  With
// TMR_PEAKS_PROB_SCRATCH the caller does not want the map: a logit whose
// sigmoid cannot round to thr or above is written as -1 without its sigmoid
// -- it can neither be a candidate nor beat one (its p < thr <= the
// candidate's p) -- and NaN stays NaN.  (Computing the sigmoid inside the
// one-workgroup-per-unit finder left a single unit's map to one CU: 25 us
// at config A.)
__global__ __launch_bounds__(256) void prob_kernel(const float *__restrict__ o, int is_prob, int scratch, int64_t n,
                                                   int64_t HW, const tmr_peak_param_t *__restrict__ params,
                                                   float *__restrict__ prob) {
    const int64_t i0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    int64_t ulast = -1;
    float olo = -INFINITY;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int64_t i = i0 + k;
        if (i >= n) break;
        const float x = o[i];
        float v = x;
        if (!is_prob) {
            const int64_t u = i / HW;
            if (scratch && u != ulast) {
                ulast = u;
                const float thr = params[u].thr;
                olo = -INFINITY;
                if (thr > 0.0f) {
                    // p = (float)sigmoid(x) reaches thr only when the exact sigmoid is at least
                    // the midpoint between thr and the float below it; a logit under that
                    // midpoint's logit (less a margin far above the double sigmoid's error and
                    // olo's own fp32 rounding) cannot round up to thr, even for thr near 1
                    const float tq = fminf(thr, 1.0f);
                    const double mid = 0.5 * ((double)tq + (double)nextafterf(tq, 0.0f));
                    const double lg = log(mid / (1.0 - mid));
                    olo = (float)(lg - 1e-5 * (1.0 + fabs(lg)));
                }
            }
            v = x < olo ? -1.0f : tmr_sigmoid_cr(x);
        }
        prob[i] = v;
    }
}

// One workgroup per unit, one pass (north_star kernel 4, "wavefront-ballot"):
// the unit's probability map is walked in chunks of R whole rows; each chunk
// and its two halo rows (zero outside the image: F.unfold's padding) are
// staged in LDS.  Every wave takes 64 consecutive row-major pixels per step
// and keeps the step's is_peak ballot in LDS; after ONE barrier every lane
// finds its slot from the ballots of the steps and waves before it (+ mbcnt),
// so the candidates leave in row-major (torch.where) order, three barriers
// per chunk (round 5's first ballot kernel synchronised twice per 512-pixel
// step: 72 barriers per 128x128 unit).
constexpr int PNT = 1024;               // threads per unit block (16 waves: one unit per CU at most)
constexpr int PNW = PNT / 64;           // waves
constexpr int PCHUNK = 16384;           // staged pixels per chunk (whole rows): a 128 x 128 map in one
constexpr int PSTEPS = PCHUNK / PNT;    // PNT-pixel steps per chunk at most (W <= PCHUNK / 2)

__host__ __device__ inline int peak_rows(int W) { return W >= PCHUNK ? 1 : PCHUNK / W; }

__device__ __forceinline__ void decode_one(const float *__restrict__ reg, int HW, const tmr_peak_param_t &pp,
                                           int u, int i, const float *__restrict__ ref, float *__restrict__ box,
                                           ExpTable et);

__global__ __launch_bounds__(PNT) void peaks_kernel(const float *__restrict__ pm, int H, int W,
                                                    const tmr_peak_param_t *__restrict__ params,
                                                    float *__restrict__ logits, float *__restrict__ box,
                                                    float *__restrict__ ref, int32_t *__restrict__ counts,
                                                    const float *__restrict__ reg, int fuse_decode, ExpTable et) {
    extern __shared__ float sp[];  // [R + 2][W] probabilities, row 0 = image row r0 - 1
    __shared__ uint64_t bal[PSTEPS][PNW];
    const int u = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const tmr_peak_param_t pp = params[u];
    const int HW = H * W, R = peak_rows(W);
    // e / W by one multiply: exact while e < (R + 2) W <= 2 * PCHUNK (far below 2^22)
    const float rW = 1.0f / (float)W;
    const float *pmu = pm + (size_t)u * HW;
    const size_t cap = (size_t)HW;
    const uint64_t lt = (1ull << lane) - 1ull;  // lanes below this one
    int base = 0;  // candidates so far (block-uniform)
    for (int r0 = 0; r0 < H; r0 += R) {
        const int rn = min(R, H - r0), np = rn * W, ns = (np + PNT - 1) / PNT;
#pragma unroll 4
        for (int e = tid; e < (rn + 2) * W; e += PNT) {
            const int lr = (int)(((float)e + 0.5f) * rW), c = e - lr * W, y = r0 - 1 + lr;
            sp[e] = (y >= 0 && y < H) ? pmu[(size_t)y * W + c] : 0.0f;
        }
        __syncthreads();  // (1) the chunk is staged
        uint32_t fb = 0;  // bit s: this lane's pixel of step s is a candidate
        for (int st = 0; st < ns; ++st) {
            const int i = st * PNT + tid;  // pixel of the chunk
            bool f = false;
            if (i < np) {
                const int ly = (int)(((float)i + 0.5f) * rW) + 1, x = i - (ly - 1) * W;
                const float v = sp[ly * W + x];
                if (v >= pp.thr) {  // masked 3x3 max (TM_utils.py:337-361): first tap, then strict >;
                    float mx = 0.0f;  // a NaN tap sticks (torch.max, :359), so `pooled == p` (:253) fails
                    bool first = true;
#pragma unroll
                    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                        for (int dx = -1; dx <= 1; ++dx) {
                            if (!((pp.mask >> ((dy + 1) * 3 + dx + 1)) & 1)) continue;
                            const int xx = x + dx;
                            const float q = (xx < 0 || xx >= W) ? 0.0f : sp[(ly + dy) * W + xx];
                            if (first || q > mx || q != q) { mx = q; first = false; }
                        }
                    f = mx == v;
                }
            }
            const uint64_t bw = __ballot(f);
            if (lane == 0) bal[st][wave] = bw;
            fb |= (uint32_t)f << st;
        }
        __syncthreads();  // (2) every step's ballots are in
        int before = 0, tot = 0;  // candidates of the chunk before this wave's step st
        for (int st = 0; st < ns; ++st) {
            int cw = 0;
#pragma unroll
            for (int k = 0; k < PNW; ++k) {
                const int c = __popcll(bal[st][k]);
                cw += k < wave ? c : 0;
                tot += c;
            }
            if ((fb >> st) & 1u) {  // the slot's pixel index rides in the box row until decode_kernel
                const int i = st * PNT + tid, ly = (int)(((float)i + 0.5f) * rW) + 1, x = i - (ly - 1) * W;
                const int y = r0 + ly - 1;
                const size_t k = (size_t)u * cap + base + before + cw + __popcll(bal[st][wave] & lt);
                *reinterpret_cast<float2 *>(logits + 2 * k) = float2{sp[ly * W + x], 0.0f};
                reinterpret_cast<int *>(box)[4 * k] = y * W + x;
                *reinterpret_cast<float2 *>(ref + 2 * k) = float2{(float)x / (float)W, (float)y / (float)H};
            }
            before = tot;
        }
        base += tot;
        __syncthreads();  // (3) sp and the ballots free again
    }
    if (fuse_decode) {  // the block's own candidates (written above; visible after the barrier)
        for (int i = tid; i < base; i += PNT) decode_one(reg, HW, pp, u, i, ref, box, et);
    }
    if (tid == 0) {
        counts[u] = base;
        if (base == 0) {  // the empty unit's dummy row (TM_utils.py:288-291) at row 0
            *reinterpret_cast<float2 *>(logits + (size_t)u * cap * 2) = float2{0.0f, 0.0f};
            *reinterpret_cast<float4 *>(box + (size_t)u * cap * 4) = float4{0.0f, 0.0f, 1e-14f, 1e-14f};
            *reinterpret_cast<float2 *>(ref + (size_t)u * cap * 2) = float2{0.0f, 0.0f};
        }
    }
}

// The box decode of candidate i of unit u (TM_utils.py:264-278): the slot's
// pixel index rides in the box row until here.
__device__ __forceinline__ void decode_one(const float *__restrict__ reg, int HW, const tmr_peak_param_t &pp,
                                           int u, int i, const float *__restrict__ ref, float *__restrict__ box,
                                           ExpTable et) {
    const float *r = reg ? reg + (size_t)u * 4 * HW : nullptr;
    const float sx = pp.mode == 1 ? 1.0f : pp.scale_w, sy = pp.mode == 1 ? 1.0f : pp.scale_h;
    const size_t k = (size_t)u * HW + i;
    const int pi = reinterpret_cast<const int *>(box)[4 * k];
    const float2 rf = *reinterpret_cast<const float2 *>(ref + 2 * k);
    float r0v = 0.0f, r1 = 0.0f, r2 = 0.0f, r3 = 0.0f;
    if (pp.mode != 2 && r) {
        r0v = r[pi]; r1 = r[HW + pi]; r2 = r[2 * HW + pi]; r3 = r[3 * HW + pi];
    }
    const float cx = rf.x + r0v * sx, cy = rf.y + r1 * sy;
    const float w = expf_ref(r2, et) * pp.scale_w, h = expf_ref(r3, et) * pp.scale_h;
    const float hw2 = w / 2.0f, hh2 = h / 2.0f;
    *reinterpret_cast<float4 *>(box + 4 * k) = float4{cx - hw2, cy - hh2, cx + hw2, cy + hh2};
}

// Every candidate's decode, chip-wide: one thread per candidate, so the
// reference-exp table's binary search (a chain of dependent loads) overlaps
// across thousands of threads instead of serialising the finder's steps.
// (Launches of a few units decode inside peaks_kernel instead: one launch
// less, config A.)
__global__ __launch_bounds__(256) void decode_kernel(const float *__restrict__ reg, int H, int W,
                                                     const tmr_peak_param_t *__restrict__ params,
                                                     const int32_t *__restrict__ counts, const float *__restrict__ ref,
                                                     float *__restrict__ box, ExpTable et) {
    const int u = blockIdx.x;
    const int n = counts[u];
    const tmr_peak_param_t pp = params[u];
    for (int i = blockIdx.y * 256 + threadIdx.x; i < n; i += gridDim.y * 256)
        decode_one(reg, H * W, pp, u, i, ref, box, et);
}

constexpr int kFuseDecodeUnits = 8;

}  // namespace

extern "C" int tmr_maxpool3x3(const float *x, int64_t planes, int H, int W, int mask9, float *out,
                              void *stream) {
    if (planes < 0 || H < 0 || W < 0 || (mask9 & 0x1ff) == 0 || (mask9 & ~0x1ff) != 0) return TMR_E_INVALID;
    const int64_t n = planes * H * W;
    if (n == 0) return TMR_OK;
    if (!x || !out) return TMR_E_INVALID;
    hipLaunchKernelGGL(maxpool3x3_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       x, n, H, W, mask9, out);
    TMR_CHECK_LAUNCH();
    return TMR_OK;
}

extern "C" int tmr_peaks_decode(const float *o, int input_is_prob, const float *reg, int U, int H,
                                int W, const tmr_peak_param_t *params, float *prob, float *logits,
                                float *box, float *ref, int32_t *counts, const void *exp_table,
                                void *stream) {
    TMR_REQUIRE(o && params && prob && logits && box && ref && counts && U > 0 && H > 0 && W > 0);
    TMR_REQUIRE((input_is_prob & ~(1 | TMR_PEAKS_PROB_SCRATCH | TMR_PEAKS_FIND_ONLY | TMR_PEAKS_DECODE_ONLY)) == 0);
    const bool find_only = input_is_prob & TMR_PEAKS_FIND_ONLY, decode_only = input_is_prob & TMR_PEAKS_DECODE_ONLY;
    TMR_REQUIRE(!(find_only && decode_only));
    const int is_prob = input_is_prob & 1, scratch = (input_is_prob & TMR_PEAKS_PROB_SCRATCH) != 0;
    hipStream_t s = tmr_stream(stream);
    ExpTable et = {nullptr, nullptr};
    if (exp_table) {
        const char *base = reinterpret_cast<const char *>(exp_table);
        et.off = reinterpret_cast<const uint32_t *>(base + EXP_HEADER);
        et.lo = reinterpret_cast<const uint16_t *>(base + EXP_HEADER + 4 * 65537);
    }
    const int ny = (int)std::min<int64_t>(tmr_cdiv((int64_t)H * W, 256), 32);
    if (decode_only) {  // the rows of an earlier TMR_PEAKS_FIND_ONLY call
        hipLaunchKernelGGL(decode_kernel, dim3(U, ny), dim3(256), 0, s, reg, H, W, params, counts, ref, box, et);
        TMR_CHECK_LAUNCH();
        return TMR_OK;
    }
    TMR_REQUIRE(W <= PCHUNK / 2);  // (R + 2) W floats of LDS <= 3 * 8192 * 4 B
    const size_t lds = (size_t)(peak_rows(W) + 2) * W * sizeof(float);
    if (lds > 64 * 1024 && tmr_set_max_lds((const void *)peaks_kernel, lds) != hipSuccess) return TMR_E_HIP;
    const float *pm = o;
    if (!(is_prob && scratch)) {  // the map (or its scratch form) into prob
        const int64_t n = (int64_t)U * H * W;
        TMR_REQUIRE(tmr_cdiv(n, 1024) < (1LL << 31));
        hipLaunchKernelGGL(prob_kernel, dim3((unsigned)tmr_cdiv(n, 1024)), dim3(256), 0, s, o, is_prob, scratch, n,
                           (int64_t)H * W, params, prob);
        TMR_CHECK_LAUNCH();
        pm = prob;
    }
    // a few units: decode inside the finder (one launch less); many: chip-wide
    const int fuse = U <= kFuseDecodeUnits && !find_only;
    hipLaunchKernelGGL(peaks_kernel, dim3(U), dim3(PNT), lds, s, pm, H, W, params, logits, box, ref, counts, reg,
                       fuse, et);
    TMR_CHECK_LAUNCH();
    if (!fuse && !find_only) {
        hipLaunchKernelGGL(decode_kernel, dim3(U, ny), dim3(256), 0, s, reg, H, W, params, counts, ref, box, et);
        TMR_CHECK_LAUNCH();
    }
    return TMR_OK;
}

// ---------------------------------------------------------------------------
// Evaluation losses (tmr_gt_loss, include/tmr.h): GT_map.Get_pred_gts
// (utils/TM_utils.py:94-222) and SetCriterion_TM (criterion/criterions_TM.py)
// for one level.  The [H*W, G] matrices of the reference are never built:
//   gt_box_kernel:    one wave per GT box: its 32-B record (cx, cy, ratio,
//                     bias_p, bias_n, area, centre pixel).
//   gt_image_kernel:  one thread per pixel per IMAGE; the image's records are
//                     staged through LDS in chunks of GT_CHUNK (any G); one
//                     packed word per pixel: target | any_pos | all_pos |
//                     any_notneg.
//   gt_unit_kernel:   grid (TMR_GT_SLICES, U): the unit's boundary rectangle
//                     over its image's words -> gt_map, target; with the loss
//                     fused, the BCE / focal and GIoU terms straight from o and
//                     reg; fp64 partials {positives, negatives, sum ce, sum
//                     giou} per slice, summed in a fixed order.
//   gt_final_kernel:  the slices in order -> counts, sums (+ the dummy pair).
//   gt_gather_kernel: one workgroup per unit, row-major ballot compaction.
//   gt_rows_kernel:   the element losses over gathered lists.
namespace {

constexpr int GT_NT = 256;       // threads per block
constexpr int GT_CHUNK = 256;    // box records staged per LDS chunk (8 KB)
constexpr int GT_SL = TMR_GT_SLICES;
constexpr uint32_t GT_ANY_POS = 1u << 29, GT_ALL_POS = 1u << 30, GT_ANY_NOTNEG = 1u << 31;
constexpr uint32_t GT_TARGET = GT_ANY_POS - 1u;

struct GtBox {  // 32 B
    float cx, cy, ratio, bias_p, bias_n, area;
    int32_t center, pad_;
};

__global__ __launch_bounds__(64) void gt_box_kernel(const float *__restrict__ boxes, int G, int H, int W,
                                                    float coef_p, float coef_n, int need_center,
                                                    GtBox *__restrict__ rec) {
    const int g = blockIdx.x, lane = threadIdx.x;
    if (g >= G) return;
    const float4 b = *reinterpret_cast<const float4 *>(boxes + 4 * (size_t)g);
    const float cx = (b.z + b.x) / 2.0f, cy = (b.w + b.y) / 2.0f;
    const float ws = b.z - b.x, hs = b.w - b.y;
    int best = 0;
    if (need_center) {
        // argmin over the pixels of d = fl32(rx[x] + ry[y]), lowest index on ties, in O(H + W):
        // rounding is monotone, so min_x fl32(rx[x] + c) = fl32(min rx + c) for any c, the
        // minimum is dmin = fl32(min rx + min ry), a row y holds a minimiser iff
        // fl32(min rx + ry[y]) == dmin, and the lowest index is the first such row's first
        // column with fl32(rx[x] + ry[y]) == dmin (the boxes are finite: no NaN)
        const float fW = (float)W, fH = (float)H;
        float mrx = INFINITY, mry = INFINITY;
        for (int x = lane; x < W; x += 64) mrx = fminf(mrx, fabsf((float)x / fW - cx));
        for (int y = lane; y < H; y += 64) mry = fminf(mry, fabsf((float)y / fH - cy));
        for (int o = 32; o > 0; o >>= 1) {
            mrx = fminf(mrx, __shfl_xor(mrx, o));
            mry = fminf(mry, __shfl_xor(mry, o));
        }
        const float dmin = mrx + mry;
        int ys = 0x7fffffff, xs = 0x7fffffff;
        for (int y = lane; y < H; y += 64)
            if (mrx + fabsf((float)y / fH - cy) == dmin) ys = min(ys, y);
        for (int o = 32; o > 0; o >>= 1) ys = min(ys, __shfl_xor(ys, o));
        if (ys == 0x7fffffff) ys = 0;
        const float rys = fabsf((float)ys / fH - cy);
        for (int x = lane; x < W; x += 64)
            if (fabsf((float)x / fW - cx) + rys == dmin) xs = min(xs, x);
        for (int o = 32; o > 0; o >>= 1) xs = min(xs, __shfl_xor(xs, o));
        if (xs == 0x7fffffff) xs = 0;
        best = ys * W + xs;
    }
    if (lane == 0) {
        GtBox r;
        r.cx = cx; r.cy = cy;
        r.ratio = -hs / ws;
        r.bias_p = coef_p * hs;
        r.bias_n = coef_n * hs;
        r.area = (b.z - b.x) * (b.w - b.y);
        r.center = best; r.pad_ = 0;
        rec[g] = r;
    }
}

__global__ __launch_bounds__(GT_NT) void gt_image_kernel(const GtBox *__restrict__ rec,
                                                         const int32_t *__restrict__ box_off, int G_total,
                                                         int H, int W, int pos_is_center, int neg_is_center, int last_level,
                                                         uint32_t *__restrict__ cls) {
    __shared__ GtBox sb[GT_CHUNK];
    const int m = blockIdx.y, HW = H * W;
    const int i = blockIdx.x * GT_NT + threadIdx.x;
    const int g0 = box_off[m];
    int G = box_off[m + 1] - g0;
    if (g0 < 0 || G < 0 || G > G_total - g0) G = 0;  // a range outside the records: nothing is read
    const int y = i / W, x = i - y * W;
    const float cxs = (float)x / (float)W, cys = (float)y / (float)H;
    bool any_pos = false, all_pos = true, any_notneg = false;
    float best_a = 0.0f;
    int best = 0;
    for (int c0 = 0; c0 < G; c0 += GT_CHUNK) {
        const int n = min(GT_CHUNK, G - c0);
        __syncthreads();  // the previous chunk is consumed
        for (int k = threadIdx.x; k < n; k += GT_NT) sb[k] = rec[g0 + c0 + k];
        __syncthreads();
        if (i < HW) {
            for (int k = 0; k < n; ++k) {
                const GtBox r = sb[k];
                const float rx = fabsf(cxs - r.cx), ry = fabsf(cys - r.cy);
                const float t = r.ratio * rx;
                const bool isc = i == r.center;
                bool inpos = (t + r.bias_p) >= ry, inneg = (t + r.bias_n) < ry;
                if (pos_is_center) inpos = isc;
                if (neg_is_center) inneg = !isc;
                const bool pos = inpos || (last_level && isc);
                any_pos |= pos;
                all_pos &= pos;
                any_notneg |= !inneg;
                // torch.min over (pos ? area : 1e8): the first minimum
                const float a = pos ? r.area : 100000000.0f;
                if ((c0 | k) == 0 || a < best_a) { best_a = a; best = c0 + k; }
            }
        }
    }
    if (i < HW)
        cls[(size_t)m * HW + i] = (uint32_t)best | (any_pos ? GT_ANY_POS : 0u) | (all_pos ? GT_ALL_POS : 0u) |
                                  (any_notneg ? GT_ANY_NOTNEG : 0u);
}

// binary_cross_entropy_with_logits(x, t), optionally WeightedFocalLoss(alpha .25, gamma 2)
__device__ __forceinline__ double gt_ce(float xf, float tf, int focal) {
    const double x = (double)xf, t = (double)tf;
    const double ce = fmax(x, 0.0) - x * t + log1p(exp(-fabs(x)));
    if (!focal) return ce;
    const double at = ((long long)tf == 1) ? 0.25 : 0.75;  // alpha.gather(targets.long())
    const double q = 1.0 - exp(-ce);
    return at * q * q * ce;
}

// gIoU_loss of one cxcywh pair (criterions_TM.py:7-13, torchvision
// generalized_box_iou_loss, eps 1e-13), evaluated in fp64
__device__ __forceinline__ double gt_giou(float4 p, float4 g) {
    const double eps = 1e-13;
    const double x1 = (double)p.x - (double)p.z / 2, y1 = (double)p.y - (double)p.w / 2;
    const double x2 = (double)p.x + (double)p.z / 2, y2 = (double)p.y + (double)p.w / 2;
    const double x1g = (double)g.x - (double)g.z / 2, y1g = (double)g.y - (double)g.w / 2;
    const double x2g = (double)g.x + (double)g.z / 2, y2g = (double)g.y + (double)g.w / 2;
    const double xk1 = fmax(x1, x1g), yk1 = fmax(y1, y1g), xk2 = fmin(x2, x2g), yk2 = fmin(y2, y2g);
    double inter = 0.0;
    if (yk2 > yk1 && xk2 > xk1) inter = (xk2 - xk1) * (yk2 - yk1);
    const double uni = (x2 - x1) * (y2 - y1) + (x2g - x1g) * (y2g - y1g) - inter;
    const double iou = inter / (uni + eps);
    const double xc1 = fmin(x1, x1g), yc1 = fmin(y1, y1g), xc2 = fmax(x2, x2g), yc2 = fmax(y2, y2g);
    const double ac = (xc2 - xc1) * (yc2 - yc1);
    return 1.0 - iou + (ac - uni) / (ac + eps);
}

// The prediction row (cx, cy, w, h) of pixel pi of unit u (TM_utils.py:183-189),
// the arithmetic of decode_one.
__device__ __forceinline__ float4 gt_pred_row(const float *__restrict__ reg, int HW, int W, int H,
                                              const tmr_gt_unit_t &un, int u, int pi, ExpTable et) {
    const int y = pi / W, x = pi - y * W;
    const float rx = (float)x / (float)W, ry = (float)y / (float)H;
    const float sx = un.mode == 1 ? 1.0f : un.scale_w, sy = un.mode == 1 ? 1.0f : un.scale_h;
    float r0 = 0.0f, r1 = 0.0f, r2 = 0.0f, r3 = 0.0f;
    if (un.mode != 2 && reg) {
        const float *r = reg + (size_t)u * 4 * HW;
        r0 = r[pi]; r1 = r[HW + pi]; r2 = r[2 * (size_t)HW + pi]; r3 = r[3 * (size_t)HW + pi];
    }
    return float4{rx + r0 * sx, ry + r1 * sy, expf_ref(r2, et) * un.scale_w, expf_ref(r3, et) * un.scale_h};
}

__device__ __forceinline__ float4 gt_row_of_box(const float *__restrict__ boxes, int g) {
    const float4 b = *reinterpret_cast<const float4 *>(boxes + 4 * (size_t)g);
    return float4{(b.z + b.x) / 2.0f, (b.w + b.y) / 2.0f, b.z - b.x, b.w - b.y};
}

// block sum of 4 fp64 values in a fixed order: xor butterfly inside each wave,
// then the waves in order; the result is valid on thread 0
__device__ __forceinline__ void gt_block_sum(double (&v)[4], double (*ws)[4]) {
    for (int o = 32; o > 0; o >>= 1)
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] += __shfl_xor(v[k], o);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int k = 0; k < 4; ++k) ws[w][k] = v[k];
    __syncthreads();
    if (threadIdx.x == 0)
        for (int i = 1; i < GT_NT / 64; ++i)
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] += ws[i][k];
}

__global__ __launch_bounds__(GT_NT) void gt_unit_kernel(const uint32_t *__restrict__ cls,
                                                        const tmr_gt_unit_t *__restrict__ units,
                                                        const int32_t *__restrict__ box_off,
                                                        const float *__restrict__ boxes, const float *__restrict__ o,
                                                        const float *__restrict__ reg, int NI, int H, int W,
                                                        int with_loss, int focal, ExpTable et, float *__restrict__ gt_map,
                                                        int32_t *__restrict__ target, double *__restrict__ part) {
    __shared__ double ws[GT_NT / 64][4];
    const int s = blockIdx.x, u = blockIdx.y, HW = H * W;
    const tmr_gt_unit_t un = units[u];
    if ((unsigned)un.image >= (unsigned)NI) return;  // block-uniform: an image outside the batch writes nothing
    const uint32_t *c = cls + (size_t)un.image * HW;
    const int g0 = box_off[un.image];
    const int per = (HW + GT_SL - 1) / GT_SL;
    const int beg = min(s * per, HW), end = min(beg + per, HW);
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = beg + (int)threadIdx.x; i < end; i += GT_NT) {
        const int y = i / W, x = i - y * W;
        const uint32_t w = c[i];
        const bool nib = y >= un.pad_y && y < H - un.pad_y && x >= un.pad_x && x < W - un.pad_x;
        const bool positive = nib && (w & GT_ANY_POS);
        const bool ignore = nib && !(w & GT_ALL_POS) && (w & GT_ANY_NOTNEG);
        const bool negative = !(positive || ignore);
        const int tg = positive ? (int)(w & GT_TARGET) : 0;
        const size_t k = (size_t)u * HW + i;
        gt_map[k] = positive ? 1.0f : (negative ? 0.0f : 0.5f);
        target[k] = tg;
        v[0] += positive ? 1.0 : 0.0;
        v[1] += negative ? 1.0 : 0.0;
        if (with_loss) {
            if (positive) {
                v[2] += gt_ce(o[k], 1.0f, focal);
                v[3] += gt_giou(gt_pred_row(reg, HW, W, H, un, u, i, et), gt_row_of_box(boxes, g0 + tg));
            } else if (negative) {
                v[2] += gt_ce(o[k], 0.0f, focal);
            }
        }
    }
    gt_block_sum(v, ws);
    if (threadIdx.x == 0) {
        double *p = part + ((size_t)u * GT_SL + s) * 4;
        p[0] = v[0]; p[1] = v[1]; p[2] = v[2]; p[3] = v[3];
    }
}

// rows == 0: per unit, the slices in order -> counts [U][2], sums [U][2] (a
// unit without a positive pixel: the dummy pair's GIoU loss); rows == 1: the
// list form, sums[0..1] only.
__global__ void gt_final_kernel(const double *__restrict__ part, int U, int with_loss, int rows,
                                int32_t *__restrict__ counts, double *__restrict__ sums) {
    const int u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= U) return;
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    for (int s = 0; s < GT_SL; ++s)
        for (int k = 0; k < 4; ++k) v[k] += part[((size_t)u * GT_SL + s) * 4 + k];
    if (!rows) {
        counts[2 * u] = (int32_t)v[0];
        counts[2 * u + 1] = (int32_t)v[1];
        if (v[0] == 0.0) {
            const float4 d = float4{0.0f, 0.0f, 1e-14f, 1e-14f};
            v[3] = gt_giou(d, d);
        }
    }
    if (with_loss) { sums[2 * u] = v[2]; sums[2 * u + 1] = v[3]; }
}

// One workgroup per unit: positives, then negatives, each in row-major order.
__global__ __launch_bounds__(GT_NT) void gt_gather_kernel(const float *__restrict__ gt_map,
                                                          const int32_t *__restrict__ target,
                                                          const int32_t *__restrict__ counts,
                                                          const tmr_gt_unit_t *__restrict__ units,
                                                          const int32_t *__restrict__ box_off,
                                                          const float *__restrict__ boxes, const float *__restrict__ o,
                                                          const float *__restrict__ reg, int NI, int H, int W,
                                                          ExpTable et, const int64_t *__restrict__ samp_off,
                                                          const int64_t *__restrict__ row_off,
                                                          float *__restrict__ obj_out, float *__restrict__ label_out,
                                                          float *__restrict__ rows_pred, float *__restrict__ rows_gt) {
    __shared__ int wc[GT_NT / 64][2];
    const int u = blockIdx.x, HW = H * W, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const tmr_gt_unit_t un = units[u];
    if ((unsigned)un.image >= (unsigned)NI) return;  // block-uniform
    const int g0 = box_off[un.image], gi = box_off[un.image + 1] - g0;
    const int npos = counts[2 * u];
    const int64_t so = samp_off[u], ro = row_off[u];
    const uint64_t lt = (1ull << lane) - 1ull;
    int bp = 0, bn = 0;  // positives / negatives before this chunk (block-uniform)
    for (int c0 = 0; c0 < HW; c0 += GT_NT) {
        const int i = c0 + tid;
        float m = 0.5f;
        if (i < HW) m = gt_map[(size_t)u * HW + i];
        const bool p = m == 1.0f, n = m == 0.0f;
        const uint64_t pb = __ballot(p), nb = __ballot(n);
        if (lane == 0) { wc[wave][0] = __popcll(pb); wc[wave][1] = __popcll(nb); }
        __syncthreads();
        int pp = 0, pn = 0, tp = 0, tn = 0;
#pragma unroll
        for (int k = 0; k < GT_NT / 64; ++k) {
            pp += k < wave ? wc[k][0] : 0;
            pn += k < wave ? wc[k][1] : 0;
            tp += wc[k][0];
            tn += wc[k][1];
        }
        if (p) {
            const int k = bp + pp + __popcll(pb & lt);
            obj_out[so + k] = o[(size_t)u * HW + i];
            label_out[so + k] = 1.0f;
            const float4 pr = gt_pred_row(reg, HW, W, H, un, u, i, et);
            const float4 gr = gt_row_of_box(boxes, g0 + min(max(target[(size_t)u * HW + i], 0), gi - 1));
            float *dp = rows_pred + 4 * (ro + k), *dg = rows_gt + 4 * (ro + k);
            dp[0] = pr.x; dp[1] = pr.y; dp[2] = pr.z; dp[3] = pr.w;
            dg[0] = gr.x; dg[1] = gr.y; dg[2] = gr.z; dg[3] = gr.w;
        } else if (n) {
            const int k = npos + bn + pn + __popcll(nb & lt);
            obj_out[so + k] = o[(size_t)u * HW + i];
            label_out[so + k] = 0.0f;
        }
        bp += tp;
        bn += tn;
        __syncthreads();  // wc free again
    }
    if (tid == 0 && npos == 0) {  // the dummy pair (TM_utils.py:201-203)
        float *dp = rows_pred + 4 * ro, *dg = rows_gt + 4 * ro;
        dp[0] = dg[0] = 0.0f; dp[1] = dg[1] = 0.0f; dp[2] = dg[2] = 1e-14f; dp[3] = dg[3] = 1e-14f;
    }
}

// The element losses over gathered lists: slice s of GT_SL of both lists.
__global__ __launch_bounds__(GT_NT) void gt_rows_kernel(const float *__restrict__ obj, const float *__restrict__ label,
                                                        int64_t ns, const float *__restrict__ rp,
                                                        const float *__restrict__ rg, int64_t nr, int focal,
                                                        double *__restrict__ part) {
    __shared__ double ws[GT_NT / 64][4];
    const int s = blockIdx.x;
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    {
        const int64_t per = (ns + GT_SL - 1) / GT_SL;
        const int64_t beg = min((int64_t)s * per, ns), end = min(beg + per, ns);
        for (int64_t i = beg + threadIdx.x; i < end; i += GT_NT) v[2] += gt_ce(obj[i], label[i], focal);
    }
    {
        const int64_t per = (nr + GT_SL - 1) / GT_SL;
        const int64_t beg = min((int64_t)s * per, nr), end = min(beg + per, nr);
        for (int64_t i = beg + threadIdx.x; i < end; i += GT_NT)
            v[3] += gt_giou(float4{rp[4 * i], rp[4 * i + 1], rp[4 * i + 2], rp[4 * i + 3]},
                            float4{rg[4 * i], rg[4 * i + 1], rg[4 * i + 2], rg[4 * i + 3]});
    }
    gt_block_sum(v, ws);
    if (threadIdx.x == 0) {
        double *p = part + (size_t)s * 4;
        p[0] = 0.0; p[1] = 0.0; p[2] = v[2]; p[3] = v[3];
    }
}

inline int64_t gt_align(int64_t v) { return (v + 255) / 256 * 256; }

}  // namespace

// work = [box records | per-image class words | slice partials]
TMR_INTERNAL int64_t tmr_gt_work_bytes(int64_t G, int64_t NI, int64_t H, int64_t W, int64_t U);
int64_t tmr_gt_work_bytes(int64_t G, int64_t NI, int64_t H, int64_t W, int64_t U) {
    if (G < 1 || NI < 1 || H < 1 || W < 1 || U < 1 || H * W > INT32_MAX) return -1;
    if (G > INT32_MAX || NI > 65535 || U > 65535) return -1;
    return gt_align(G * (int64_t)sizeof(GtBox)) + gt_align(NI * H * W * 4) + gt_align(U * GT_SL * 4 * 8);
}

extern "C" int tmr_gt_loss(const tmr_gt_loss_args_t *a, void *stream) {
    TMR_REQUIRE(a != nullptr);
    const int ph = a->phase;
    TMR_REQUIRE(ph != 0 && (ph & ~(TMR_GT_ASSIGN | TMR_GT_LOSS | TMR_GT_GATHER | TMR_GT_ROWS)) == 0);
    TMR_REQUIRE(!(ph & TMR_GT_ROWS) || ph == TMR_GT_ROWS);
    TMR_REQUIRE(!(ph & TMR_GT_LOSS) || (ph & TMR_GT_ASSIGN));
    TMR_REQUIRE(a->work != nullptr);
    hipStream_t s = tmr_stream(stream);
    ExpTable et = {nullptr, nullptr};
    if (a->exp_table) {
        const char *base = reinterpret_cast<const char *>(a->exp_table);
        et.off = reinterpret_cast<const uint32_t *>(base + EXP_HEADER);
        et.lo = reinterpret_cast<const uint16_t *>(base + EXP_HEADER + 4 * 65537);
    }
    if (ph == TMR_GT_ROWS) {
        TMR_REQUIRE(a->n_samples >= 0 && a->n_rows >= 0 && a->sums);
        TMR_REQUIRE((a->n_samples == 0 || (a->obj_out && a->label_out)) &&
                    (a->n_rows == 0 || (a->rows_pred && a->rows_gt)));
        double *part = static_cast<double *>(a->work);  // TMR_SIZE_GT_WORK(>=1, ...) holds GT_SL * 4 doubles
        hipLaunchKernelGGL(gt_rows_kernel, dim3(GT_SL), dim3(GT_NT), 0, s, a->obj_out, a->label_out, a->n_samples,
                           a->rows_pred, a->rows_gt, a->n_rows, a->focal, part);
        TMR_CHECK_LAUNCH();
        hipLaunchKernelGGL(gt_final_kernel, dim3(1), dim3(64), 0, s, part, 1, 1, 1, (int32_t *)nullptr, a->sums);
        TMR_CHECK_LAUNCH();
        return TMR_OK;
    }
    TMR_REQUIRE(a->U > 0 && a->U <= 65535 && a->NI > 0 && a->NI <= 65535 && a->H > 0 && a->W > 0);
    TMR_REQUIRE((int64_t)a->H * a->W <= INT32_MAX);
    TMR_REQUIRE(a->G_total > 0 && a->min_boxes > 0 && a->min_boxes < (1 << 29));
    TMR_REQUIRE(a->boxes && a->box_off && a->units && a->gt_map && a->target && a->counts);
    TMR_REQUIRE(!(ph & TMR_GT_LOSS) || (a->o && a->sums));
    TMR_REQUIRE(!(ph & TMR_GT_GATHER) || (a->o && a->samp_off && a->row_off && a->obj_out && a->label_out &&
                                          a->rows_pred && a->rows_gt));
    const int H = a->H, W = a->W, HW = H * W;
    char *wk = static_cast<char *>(a->work);
    GtBox *rec = reinterpret_cast<GtBox *>(wk);
    uint32_t *cls = reinterpret_cast<uint32_t *>(wk + gt_align((int64_t)a->G_total * sizeof(GtBox)));
    double *part = reinterpret_cast<double *>(reinterpret_cast<char *>(cls) + gt_align((int64_t)a->NI * HW * 4));
    if (ph & TMR_GT_ASSIGN) {
        const double pt = a->positive_threshold, nt = a->negative_threshold;
        TMR_REQUIRE(pt == pt && nt == nt);
        const float coef_p = (float)((1.0 - pt) / (1.0 + pt)), coef_n = (float)((1.0 - nt) / (1.0 + nt));
        const int pc = pt == 1.0, nc = nt == 1.0, last = a->last_level != 0;
        const int with_loss = (ph & TMR_GT_LOSS) != 0;
        hipLaunchKernelGGL(gt_box_kernel, dim3(a->G_total), dim3(64), 0, s, a->boxes, a->G_total, H, W, coef_p,
                           coef_n, pc | nc | last, rec);
        TMR_CHECK_LAUNCH();
        hipLaunchKernelGGL(gt_image_kernel, dim3((unsigned)tmr_cdiv(HW, GT_NT), a->NI), dim3(GT_NT), 0, s, rec,
                           a->box_off, a->G_total, H, W, pc, nc, last, cls);
        TMR_CHECK_LAUNCH();
        hipLaunchKernelGGL(gt_unit_kernel, dim3(GT_SL, a->U), dim3(GT_NT), 0, s, cls, a->units, a->box_off,
                           a->boxes, a->o, a->reg, a->NI, H, W, with_loss, a->focal, et, a->gt_map, a->target, part);
        TMR_CHECK_LAUNCH();
        hipLaunchKernelGGL(gt_final_kernel, dim3((unsigned)tmr_cdiv(a->U, 64)), dim3(64), 0, s, part, a->U,
                           with_loss, 0, a->counts, a->sums);
        TMR_CHECK_LAUNCH();
    }
    if (ph & TMR_GT_GATHER) {
        hipLaunchKernelGGL(gt_gather_kernel, dim3(a->U), dim3(GT_NT), 0, s, a->gt_map, a->target, a->counts,
                           a->units, a->box_off, a->boxes, a->o, a->reg, a->NI, H, W, et, a->samp_off, a->row_off,
                           a->obj_out, a->label_out, a->rows_pred, a->rows_gt);
        TMR_CHECK_LAUNCH();
    }
    return TMR_OK;
}
