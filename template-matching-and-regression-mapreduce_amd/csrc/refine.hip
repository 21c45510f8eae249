// Mask -> box step of the SAM box refiner (include/tmr_refine.h; reference
// utils/box_refine.py:158-176, 232-246), gfx950.
//
// The reference upsamples [N,1,h,w] mask logits to [N,1,H,W], thresholds them
// and takes min / max of torch.where per mask in a Python loop (one sync per
// mask).  Here the upsampled plane never exists:
//
//   1. mask_boxes_init_kernel: work[n] = (INT_MAX, INT_MAX, -1, -1).
//   2. mask_boxes_kernel: one block per (mask, band of TB output rows).  The
//      low-resolution rows the band touches are staged in LDS once; a thread
//      owns output columns X = tid, tid + NT, ... and walks the band's rows,
//      keeping the x-interpolated pair (top, bot) of its current cell in
//      registers: it is recomputed only when the cell row changes, and a cell
//      whose four corners all compare <= 0 is skipped (exact: the weights are
//      >= 0; a NaN corner fails the comparison and is evaluated); a band
//      whose staged rows hold no such value ends after the staging.  The
//      rows' own parameters are wave-uniform and live in scalar registers
//      (the row loop is unrolled over the TB_MAX rows of a band).  min / max
//      are reduced in the wave, across the block's waves in LDS, and across
//      blocks with four integer atomics per block that saw a positive pixel.
//   3. mask_boxes_epilogue_kernel: one thread per mask: the reference's
//      division, centre / extent / scaler arithmetic and score product, fp32,
//      in its order.
//
// Integer min / max are order-independent, so the result is deterministic.
// Built with -ffp-contract=off: every fp32 operation of the rule is rounded
// on its own.
#include "tmr_common.h"

#include <limits.h>

#include "../../include/tmr_refine.h"

namespace {

constexpr int NT = 256;
constexpr int TB_MAX = 16;         // output rows per band, at most
constexpr int LDS_FLOATS = 8192;   // staged low-resolution rows (32 KiB)
constexpr int DIM_MAX = 65536;
constexpr int W_LOW_MAX = LDS_FLOATS / 2;  // two rows must fit

// Low-resolution rows a band of tb output rows can touch, at most:
// y0(Y) = trunc(fl(sy * Y)) with fl() within 2^-24 relative, so over tb rows
// y0 grows by at most floor(sy * (tb - 1) + 2^-23 * h) + 1 <= floor(sy * (tb - 1) + 0.25) + 1
// (h <= 65536), and y1 adds one more row.
int band_rows(int tb, int h, int H) {
    if (tb == 1) return 2;
    const double sy = H > 1 ? (double)(h - 1) / (double)(H - 1) : 0.0;
    return (int)(sy * (double)(tb - 1) + 0.25) + 3;
}

__global__ __launch_bounds__(NT) void mask_boxes_init_kernel(int4 *__restrict__ acc, int64_t N) {
    const int64_t n = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (n < N) acc[n] = make_int4(INT_MAX, INT_MAX, -1, -1);
}

__device__ __forceinline__ void src_coord(float s, int D, int lim, int &i0, int &i1, float &l, float &hgh) {
    const float r = s * (float)D;
    int a = (int)r;
    a = a < lim - 1 ? a : lim - 1;  // never taken within the documented limits (memory safety only)
    i0 = a;
    i1 = a + ((a < lim - 1) ? 1 : 0);
    l = r - (float)a;
    hgh = 1.0f - l;
}

__global__ __launch_bounds__(NT) void mask_boxes_kernel(const float *__restrict__ masks, int h, int w, int H,
                                                        int W, float sy, float sx, int tb, int nbands,
                                                        int cap_rows, int *__restrict__ acc) {
    __shared__ float band[LDS_FLOATS];
    __shared__ int row_r0[TB_MAX], row_r1[TB_MAX];
    __shared__ float row_ly[TB_MAX], row_hy[TB_MAX];
    __shared__ int red[NT / 64][4];

    const int tid = threadIdx.x;
    const int64_t n = blockIdx.x / nbands;
    const int bi = blockIdx.x % nbands;
    const int Yb = bi * tb;
    const int Ye = min(Yb + tb, H);
    const int rows_out = Ye - Yb;

    // the band's low-resolution rows [r_lo, r_lo + nrows)
    int r_lo, r_hi, t0, t1;
    float tl, th;
    src_coord(sy, Yb, h, r_lo, t1, tl, th);
    src_coord(sy, Ye - 1, h, t0, r_hi, tl, th);
    int nrows = r_hi - r_lo + 1;
    nrows = nrows < cap_rows ? nrows : cap_rows;  // band_rows() bounds it; clamped for memory safety

    const float *src = masks + (size_t)n * h * w + (size_t)r_lo * w;
    const int nstage = nrows * w;
    int any_live = 0;
    for (int i = tid; i < nstage; i += NT) {
        const float v = src[i];
        band[i] = v;
        any_live |= !(v <= 0.0f);
    }
    if (tid < TB_MAX) {  // (entries past the band's last row repeat it; they are never evaluated)
        int y0, y1;
        float ly, hy;
        src_coord(sy, Yb + min(tid, rows_out - 1), h, y0, y1, ly, hy);
        row_r0[tid] = min(y0 - r_lo, nrows - 1);
        row_r1[tid] = min(y1 - r_lo, nrows - 1);
        row_ly[tid] = ly;
        row_hy[tid] = hy;
    }
    // no staged value compares > 0 (or is NaN): every cell of the band is skipped
    if (!__syncthreads_or(any_live)) return;

    // the rows' parameters are the same for every lane: ly and the "a new cell
    // row starts here" bits are held in scalar registers, hy in vector ones
    float lys[TB_MAX], hys[TB_MAX];
    unsigned newrow = 1u;
#pragma unroll
    for (int j = 0; j < TB_MAX; ++j) {
        lys[j] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(row_ly[j])));
        hys[j] = row_hy[j];
        if (j > 0 && row_r0[j] != row_r0[j - 1]) newrow |= 1u << j;
    }
    newrow = (unsigned)__builtin_amdgcn_readfirstlane((int)newrow);

    int mnx = INT_MAX, mny = INT_MAX, mxx = -1, mxy = -1;
    for (int X = tid; X < W; X += NT) {
        int x0, x1;
        float lx, hx;
        src_coord(sx, X, w, x0, x1, lx, hx);
        bool live = false, hit = false;
        float top = 0.0f, bot = 0.0f;
#pragma unroll
        for (int j = 0; j < TB_MAX; ++j) {
            if (j < rows_out) {
                if (newrow & (1u << j)) {  // a new cell row: its x-interpolated pair
                    const int o0 = row_r0[j] * w, o1 = row_r1[j] * w;
                    const float a = band[o0 + x0], b = band[o0 + x1];
                    const float c = band[o1 + x0], d = band[o1 + x1];
                    live = !(a <= 0.0f && b <= 0.0f && c <= 0.0f && d <= 0.0f);
                    top = hx * a + lx * b;
                    bot = hx * c + lx * d;
                }
                if (live) {
                    const float v = hys[j] * top + lys[j] * bot;
                    if (v > 0.0f) {
                        mny = min(mny, Yb + j);
                        mxy = max(mxy, Yb + j);
                        hit = true;
                    }
                }
            }
        }
        if (hit) {
            mnx = min(mnx, X);
            mxx = max(mxx, X);
        }
    }

    for (int o = 32; o > 0; o >>= 1) {
        mnx = min(mnx, __shfl_xor(mnx, o));
        mny = min(mny, __shfl_xor(mny, o));
        mxx = max(mxx, __shfl_xor(mxx, o));
        mxy = max(mxy, __shfl_xor(mxy, o));
    }
    const int wv = tid >> 6;
    if ((tid & 63) == 0) {
        red[wv][0] = mnx; red[wv][1] = mny; red[wv][2] = mxx; red[wv][3] = mxy;
    }
    __syncthreads();
    if (tid == 0) {
        for (int i = 1; i < NT / 64; ++i) {
            mnx = min(mnx, red[i][0]); mny = min(mny, red[i][1]);
            mxx = max(mxx, red[i][2]); mxy = max(mxy, red[i][3]);
        }
        if (mxx >= 0) {
            int *p = acc + n * 4;
            atomicMin(p + 0, mnx);
            atomicMin(p + 1, mny);
            atomicMax(p + 2, mxx);
            atomicMax(p + 3, mxy);
        }
    }
}

__global__ __launch_bounds__(NT) void mask_boxes_epilogue_kernel(const int4 *__restrict__ acc,
                                                                 const float *__restrict__ logits,
                                                                 const float *__restrict__ iou,
                                                                 const float *__restrict__ scaler, int64_t N,
                                                                 int H, int W, int mode,
                                                                 float *__restrict__ boxes,
                                                                 float *__restrict__ refs,
                                                                 float *__restrict__ logits_out) {
    const int64_t n = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (n >= N) return;
    int4 q = acc[n];
    if (q.z < 0) q = make_int4(0, 0, 0, 0);  // no positive pixel: the reference's zeros row
    const float fw = (float)W, fh = (float)H;
    float b0 = (float)q.x / fw, b1 = (float)q.y / fh, b2 = (float)q.z / fw, b3 = (float)q.w / fh;
    if (mode == TMR_REFINE_SCALED) {
        const float cx = (b0 + b2) / 2.0f, cy = (b1 + b3) / 2.0f;
        const float l = (cx - b0) * scaler[0], t = (cy - b1) * scaler[1];
        const float r = (b2 - cx) * scaler[2], b = (b3 - cy) * scaler[3];
        b0 = cx - l; b1 = cy - t; b2 = cx + r; b3 = cy + b;
    }
    boxes[n * 4 + 0] = b0; boxes[n * 4 + 1] = b1; boxes[n * 4 + 2] = b2; boxes[n * 4 + 3] = b3;
    refs[n * 2 + 0] = (b0 + b2) / 2.0f;
    refs[n * 2 + 1] = (b1 + b3) / 2.0f;
    logits_out[n * 2 + 0] = iou[n] * logits[n * 2 + 0];
    logits_out[n * 2 + 1] = 0.0f * logits[n * 2 + 1];
}

}  // namespace

// The one statement of tmr_mask_boxes' validation and band rule (host only:
// no buffer is dereferenced).  *launch stays false for the N = 0 no-op.
static int mask_boxes_plan(const tmr_mask_boxes_args_t *args, int *tb_out, int *cap_rows_out, int *nbands_out,
                           bool *launch) {
    *launch = false;
    TMR_REQUIRE(args);
    const tmr_mask_boxes_args_t &a = *args;
    TMR_REQUIRE(a.N >= 0);
    TMR_REQUIRE(a.h >= 1 && a.h <= DIM_MAX && a.w >= 1 && a.w <= W_LOW_MAX);
    TMR_REQUIRE(a.H >= 1 && a.H <= DIM_MAX && a.W >= 1 && a.W <= DIM_MAX);
    TMR_REQUIRE(a.mode == TMR_REFINE_FORWARD || a.mode == TMR_REFINE_SCALED);
    // the tallest band whose low-resolution rows fit the LDS stage
    int tb = TB_MAX;
    while (tb > 1 && (int64_t)band_rows(tb, a.h, a.H) * a.w > LDS_FLOATS) --tb;
    *tb_out = tb;
    *cap_rows_out = LDS_FLOATS / a.w;  // >= 2
    *nbands_out = (int)tmr_cdiv(a.H, tb);
    if (a.N == 0) return TMR_OK;
    TMR_REQUIRE(a.masks && a.logits && a.iou && a.boxes && a.refs && a.logits_out && a.work);
    TMR_REQUIRE(a.mode == TMR_REFINE_FORWARD || a.scaler);
    TMR_REQUIRE((reinterpret_cast<uintptr_t>(a.work) & 15) == 0);
    TMR_REQUIRE(a.N * *nbands_out < (1ll << 31));
    *launch = true;
    return TMR_OK;
}

extern "C" int tmr_mask_boxes_plan(const tmr_mask_boxes_args_t *args, int32_t *band_rows_out, int32_t *cap_rows,
                                   int32_t *nbands) {
    TMR_REQUIRE(band_rows_out && cap_rows && nbands);
    int tb = 0, cap = 0, nb = 0;
    bool launch;
    const int rc = mask_boxes_plan(args, &tb, &cap, &nb, &launch);
    *band_rows_out = rc == TMR_OK ? tb : 0;
    *cap_rows = rc == TMR_OK ? cap : 0;
    *nbands = rc == TMR_OK ? nb : 0;
    return rc;
}

extern "C" int tmr_mask_boxes(const tmr_mask_boxes_args_t *args, void *stream) {
    int tb = 0, cap_rows = 0, nbands = 0;
    bool launch;
    const int rc = mask_boxes_plan(args, &tb, &cap_rows, &nbands, &launch);
    if (rc != TMR_OK || !launch) return rc;
    const tmr_mask_boxes_args_t &a = *args;
    const unsigned nblk = (unsigned)tmr_cdiv(a.N, NT);
    const float sy = a.H > 1 ? (float)(a.h - 1) / (float)(a.H - 1) : 0.0f;
    const float sx = a.W > 1 ? (float)(a.w - 1) / (float)(a.W - 1) : 0.0f;

    hipStream_t s = tmr_stream(stream);
    int4 *acc = static_cast<int4 *>(a.work);
    hipLaunchKernelGGL(mask_boxes_init_kernel, dim3(nblk), dim3(NT), 0, s, acc, a.N);
    TMR_CHECK_LAUNCH();
    hipLaunchKernelGGL(mask_boxes_kernel, dim3((unsigned)(a.N * nbands)), dim3(NT), 0, s, a.masks, a.h, a.w, a.H,
                       a.W, sy, sx, tb, nbands, cap_rows, reinterpret_cast<int *>(acc));
    TMR_CHECK_LAUNCH();
    hipLaunchKernelGGL(mask_boxes_epilogue_kernel, dim3(nblk), dim3(NT), 0, s, acc, a.logits, a.iou, a.scaler,
                       a.N, a.H, a.W, a.mode, a.boxes, a.refs, a.logits_out);
    TMR_CHECK_LAUNCH();
    return TMR_OK;
}
