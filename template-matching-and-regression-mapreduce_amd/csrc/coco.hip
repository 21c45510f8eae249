// COCO AP matching (include/tmr_coco.h; pycocotools COCOeval.evaluateImg for
// iouType 'bbox', as eval_log.CocoEvalMaxDets._evaluate_img restates it), gfx950.
//
// One block per (image, area range).  The dependency is serial over the
// image's detections and parallel over its ground truths and the T thresholds;
// the [D][G] IoU matrix never exists.
//
//   producer (all threads, detection d + 1): thread i owns the ground truths
//     g = i, i + NT, ...; it computes o(d + 1, g) once and, where o reaches the
//     smallest threshold, appends (g, o) to a candidate list in LDS.  The IoU
//     does not depend on what is matched, so this runs one detection AHEAD of
//     the scan, into the other of two lists: one barrier per detection.
//   scan (lane t < T of wave 0, detection d): lane t owns threshold t.  It walks
//     detection d's list (a few entries: the ground truths that overlap d by
//     half or more), keeps the best (non-ignored first, IoU, index) candidate
//     that is still free at t, and commits the match.  Bit t of a ground
//     truth's matched bits (LDS) and row t of the outputs are touched by lane t
//     alone, so the scan needs no further synchronisation.
//   A detection with more than LIST_CAP candidates (hundreds of duplicate
//     ground truths) is rescanned by the T lanes over all ground truths, serially.
//
// LDS variant (G <= cap): boxes and state words staged once per block.
// Global variant (G > cap): boxes, areas and crowd flags are read from global
// memory (inputs only); the matched bits stay in LDS, 16 per ground truth.
// No output element is written by two threads and none is read back: what the
// threads exchange (lists, matched bits) is in LDS, ordered by __syncthreads.
//
// The order in which candidates enter the list is arbitrary; the choice is a
// total order over (group, IoU, index), so the result is deterministic.
// Built with -ffp-contract=off: every fp64 operation of the rule is rounded on
// its own.
#include "tmr_common.h"

#include "../../include/tmr_coco.h"

namespace {

constexpr int LIST_CAP = 512;
constexpr int TILE_CAP = 4096;
constexpr int NT_SMALL = 256, NT_LARGE = 1024;
constexpr int NT_SWITCH = 1024;  // max_g above this: NT_LARGE threads
constexpr int LDS_FIXED = 2 * LIST_CAP * 8 + 2 * LIST_CAP * 4 + 16;
constexpr int LDS_PER_GT = 36;
constexpr unsigned ST_IGN = 1u << 16, ST_CROWD = 1u << 17;  // bits 0..15: matched at t

static_assert(LDS_FIXED + LDS_PER_GT * TILE_CAP <= 160 * 1024, "LDS");
static_assert(TMR_COCO_T_MAX <= 16, "state word");
static_assert(16 * TILE_CAP >= TMR_COCO_G_MAX, "the global variant's matched bits fit the box stage");

struct Params {
    const int64_t *det_off;
    const double *det_box, *det_area;
    const int64_t *gt_off;
    const double *gt_box, *gt_area;
    const uint8_t *gt_crowd;
    const double *area_rng, *iou_thr;
    int32_t *dt_match;
    uint8_t *dt_ignore, *gt_ignore;
    int32_t *gt_match;
    int64_t sum_d, sum_g;
    int A, T, max_d, max_g, cap;
};

struct Det {
    double x, y, x2, y2, a;
};

__device__ __forceinline__ Det load_det(const double *b) {
    Det d;
    const double w = b[2], h = b[3];
    d.x = b[0];
    d.y = b[1];
    d.x2 = d.x + w;
    d.y2 = d.y + h;
    d.a = w * h;
    return d;
}

__device__ __forceinline__ double box_iou(const Det &d, double gx, double gy, double gw, double gh, bool crowd) {
    const double gx2 = gx + gw, gy2 = gy + gh;
    const double w = (d.x2 < gx2 ? d.x2 : gx2) - (d.x > gx ? d.x : gx);
    const double h = (d.y2 < gy2 ? d.y2 : gy2) - (d.y > gy ? d.y : gy);
    if (!(w > 0.0 && h > 0.0)) return 0.0;
    const double inter = w * h;
    const double u = crowd ? d.a : (d.a + gw * gh) - inter;
    return inter / u;
}

// One block's view of its image.
template <bool RES>
struct Image {
    // LDS (RES)
    const double *sx, *sy, *sw, *sh;
    unsigned *state;
    // global (!RES)
    const double *gbox;
    const uint8_t *gcrowd;
    const double *garea;

    __device__ __forceinline__ double iou(const Det &d, int g) const {
        if (RES) return box_iou(d, sx[g], sy[g], sw[g], sh[g], (state[g] & ST_CROWD) != 0);
        const double *b = gbox + 4 * (size_t)g;
        return box_iou(d, b[0], b[1], b[2], b[3], gcrowd[g] != 0);
    }
};

template <bool RES>
__device__ void match_image(const Params &p, unsigned char *smem, int a, int64_t d0, int D, int64_t g0, int G) {
    const int cap = p.cap;
    double *list_o = reinterpret_cast<double *>(smem);
    double *sx = list_o + 2 * LIST_CAP, *sy = sx + cap, *sw = sy + cap, *sh = sw + cap;
    int *list_g = reinterpret_cast<int *>(sh + cap);
    unsigned *state = reinterpret_cast<unsigned *>(list_g + 2 * LIST_CAP);
    int *cnt = reinterpret_cast<int *>(state + cap);

    const int tid = threadIdx.x, NT = blockDim.x, T = p.T;
    const double lo = p.area_rng[2 * a], hi = p.area_rng[2 * a + 1];
    const double thr_cap = 1.0 - 1e-10;
    double thr_min = thr_cap;
    for (int t = 0; t < T; ++t) {
        const double v = p.iou_thr[t];
        thr_min = v < thr_min ? v : thr_min;
    }

    uint8_t *gign = p.gt_ignore + (size_t)a * p.sum_g + g0;
    const size_t row0 = (size_t)a * T;  // (a, t) rows of the [A][T][.] outputs
    for (int g = tid; g < G; g += NT) {
        const bool crowd = p.gt_crowd[g0 + g] != 0;
        const double ar = p.gt_area[g0 + g];
        const bool ign = crowd || ar < lo || ar > hi;
        gign[g] = ign ? 1 : 0;
        if (RES) {
            const double *b = p.gt_box + 4 * (size_t)(g0 + g);
            sx[g] = b[0];
            sy[g] = b[1];
            sw[g] = b[2];
            sh[g] = b[3];
            state[g] = (ign ? ST_IGN : 0u) | (crowd ? ST_CROWD : 0u);
        }
    }
    // global variant: 16 matched bits per ground truth, two ground truths per word, in the (unused)
    // box stage: 32 * cap bytes hold 2 bytes for each of 16 * cap >= G_MAX ground truths
    unsigned *mbits = reinterpret_cast<unsigned *>(sx);
    if (!RES)
        for (int i = tid; i < (G + 1) / 2; i += NT) mbits[i] = 0u;
    if (tid < 2) cnt[tid] = 0;
    __syncthreads();

    if (G == 0) {  // nothing to match: every detection is ignored iff its area is out of range
        for (int t = 0; t < T; ++t) {
            int32_t *dm = p.dt_match + (row0 + t) * p.sum_d + d0;
            uint8_t *di = p.dt_ignore + (row0 + t) * p.sum_d + d0;
            for (int d = tid; d < D; d += NT) {
                const double ar = p.det_area[d0 + d];
                dm[d] = 0;
                di[d] = (ar < lo || ar > hi) ? 1 : 0;
            }
        }
        return;
    }

    Image<RES> im;
    im.sx = sx; im.sy = sy; im.sw = sw; im.sh = sh;
    im.state = state;
    im.gbox = p.gt_box + 4 * (size_t)g0;
    im.gcrowd = p.gt_crowd + g0;
    im.garea = p.gt_area + g0;

    auto produce = [&](int d) {
        const Det dd = load_det(p.det_box + 4 * (size_t)(d0 + d));
        const int b = d & 1;
        for (int g = tid; g < G; g += NT) {
            const double o = im.iou(dd, g);
            if (o >= thr_min) {
                const int s = atomicAdd(&cnt[b], 1);
                if (s < LIST_CAP) {
                    list_g[b * LIST_CAP + s] = g;
                    list_o[b * LIST_CAP + s] = o;
                }
            }
        }
    };

    // lane t's threshold and output rows
    const int t = tid;
    double thr = 0.0;
    int32_t *gm = nullptr, *dm = nullptr;
    uint8_t *di = nullptr;
    if (t < T) {
        const double v = p.iou_thr[t];
        thr = v < thr_cap ? v : thr_cap;
        gm = p.gt_match + (row0 + t) * p.sum_g + g0;
        dm = p.dt_match + (row0 + t) * p.sum_d + d0;
        di = p.dt_ignore + (row0 + t) * p.sum_d + d0;
    }

    if (D > 0) produce(0);
    __syncthreads();
    for (int d = 0; d < D; ++d) {
        if (d + 1 < D) produce(d + 1);
        if (t < T) {
            const int b = d & 1;
            const int n = cnt[b];  // (read by every scanning lane before lane 0 clears it below)
            int best_g = -1;
            unsigned best_ign = 0;
            double best_o = 0.0;
            auto consider = [&](int g, double o) {
                if (!(o >= thr)) return;
                unsigned ign;
                bool crowd, matched;
                if (RES) {
                    const unsigned st = state[g];
                    ign = (st & ST_IGN) ? 1u : 0u;
                    crowd = (st & ST_CROWD) != 0;
                    matched = (st >> t) & 1u;
                } else {
                    const double ar = im.garea[g];  // (from the inputs, as the staging computed it)
                    crowd = im.gcrowd[g] != 0;
                    ign = (crowd || ar < lo || ar > hi) ? 1u : 0u;
                    matched = (mbits[g >> 1] >> ((g & 1) * 16 + t)) & 1u;
                }
                if (matched && !crowd) return;
                const bool better = best_g < 0 || ign < best_ign ||
                                    (ign == best_ign && (o > best_o || (o == best_o && g > best_g)));
                if (better) {
                    best_g = g;
                    best_ign = ign;
                    best_o = o;
                }
            };
            if (n <= LIST_CAP) {
                for (int i = 0; i < n; ++i) consider(list_g[b * LIST_CAP + i], list_o[b * LIST_CAP + i]);
            } else {  // the list overflowed: every ground truth, serially
                const Det dd = load_det(p.det_box + 4 * (size_t)(d0 + d));
                for (int g = 0; g < G; ++g) consider(g, im.iou(dd, g));
            }
            if (best_g >= 0) {
                dm[d] = best_g + 1;
                di[d] = (uint8_t)best_ign;
                gm[best_g] = d + 1;
                if (RES)
                    atomicOr(&state[best_g], 1u << t);
                else
                    atomicOr(&mbits[best_g >> 1], 1u << ((best_g & 1) * 16 + t));
            } else {
                const double ar = p.det_area[d0 + d];
                dm[d] = 0;
                di[d] = (ar < lo || ar > hi) ? 1 : 0;
            }
            if (t == 0) cnt[b] = 0;  // free for detection d + 2, produced after the barrier
        }
        __syncthreads();
    }
    // the gt_match entries no detection claimed.  Every element of every output is written exactly
    // once, by one thread (a crowd's entry again by the same lane): all that threads exchange goes
    // through LDS, which is what __syncthreads orders
    for (int tt = 0; tt < T; ++tt) {
        int32_t *row = p.gt_match + (row0 + tt) * p.sum_g + g0;
        for (int g = tid; g < G; g += NT) {
            const unsigned m = RES ? state[g] >> tt : mbits[g >> 1] >> ((g & 1) * 16 + tt);
            if (!(m & 1u)) row[g] = 0;
        }
    }
}

__global__ __launch_bounds__(NT_LARGE) void coco_match_kernel(Params p) {
    extern __shared__ __align__(16) unsigned char coco_smem[];
    const int img = blockIdx.x / p.A, a = blockIdx.x % p.A;
    const int64_t d0 = p.det_off[img], d1 = p.det_off[img + 1];
    const int64_t g0 = p.gt_off[img], g1 = p.gt_off[img + 1];
    // offsets that contradict the descriptor: skip the image (memory safety only)
    if (d0 < 0 || d1 < d0 || d1 > p.sum_d || d1 - d0 > p.max_d) return;
    if (g0 < 0 || g1 < g0 || g1 > p.sum_g || g1 - g0 > p.max_g) return;
    const int D = (int)(d1 - d0), G = (int)(g1 - g0);
    if (G <= p.cap)
        match_image<true>(p, coco_smem, a, d0, D, g0, G);
    else
        match_image<false>(p, coco_smem, a, d0, D, g0, G);
}

}  // namespace

// The one statement of tmr_coco_match's validation and geometry (host only: no
// buffer is dereferenced).  *launch stays false for the I = 0 no-op.
static int coco_plan(const tmr_coco_match_args_t *args, tmr_coco_match_plan_t *plan, bool *launch) {
    *launch = false;
    TMR_REQUIRE(args);
    const tmr_coco_match_args_t &a = *args;
    TMR_REQUIRE(a.I >= 0 && a.A >= 1 && a.T >= 1 && a.T <= TMR_COCO_T_MAX);
    TMR_REQUIRE(a.sum_d >= 0 && a.sum_g >= 0);
    TMR_REQUIRE(a.max_d >= 0 && a.max_d <= TMR_COCO_D_MAX);
    TMR_REQUIRE(a.max_g >= 0 && a.max_g <= TMR_COCO_G_MAX);
    TMR_REQUIRE((int64_t)a.I * a.A < (1ll << 31));
    TMR_REQUIRE(a.max_d <= a.sum_d && a.max_g <= a.sum_g);
    TMR_REQUIRE(a.sum_d <= (int64_t)a.I * a.max_d && a.sum_g <= (int64_t)a.I * a.max_g);
    const int cap = a.max_g < TILE_CAP ? a.max_g : TILE_CAP;
    plan->variant = a.max_g <= TILE_CAP ? TMR_COCO_VARIANT_LDS : TMR_COCO_VARIANT_GLOBAL;
    plan->tile_cap = TILE_CAP;
    plan->list_cap = LIST_CAP;
    plan->threads = a.max_g <= NT_SWITCH ? NT_SMALL : NT_LARGE;
    plan->lds_bytes = LDS_FIXED + LDS_PER_GT * cap;
    plan->blocks = a.I * a.A;
    if (a.I == 0) return TMR_OK;
    TMR_REQUIRE(a.det_off && a.gt_off && a.area_rng && a.iou_thr);
    TMR_REQUIRE(a.sum_d == 0 || (a.det_box && a.det_area && a.dt_match && a.dt_ignore));
    TMR_REQUIRE(a.sum_g == 0 || (a.gt_box && a.gt_area && a.gt_crowd && a.gt_ignore && a.gt_match));
    *launch = true;
    return TMR_OK;
}

extern "C" int tmr_coco_match_plan(const tmr_coco_match_args_t *args, tmr_coco_match_plan_t *plan) {
    TMR_REQUIRE(plan);
    tmr_coco_match_plan_t q = {};
    bool launch;
    const int rc = coco_plan(args, &q, &launch);
    if (rc != TMR_OK) q = tmr_coco_match_plan_t{};
    *plan = q;
    return rc;
}

extern "C" int tmr_coco_match(const tmr_coco_match_args_t *args, void *stream) {
    tmr_coco_match_plan_t q = {};
    bool launch;
    const int rc = coco_plan(args, &q, &launch);
    if (rc != TMR_OK || !launch) return rc;
    const tmr_coco_match_args_t &a = *args;
    Params p;
    p.det_off = a.det_off; p.det_box = a.det_box; p.det_area = a.det_area;
    p.gt_off = a.gt_off; p.gt_box = a.gt_box; p.gt_area = a.gt_area; p.gt_crowd = a.gt_crowd;
    p.area_rng = a.area_rng; p.iou_thr = a.iou_thr;
    p.dt_match = a.dt_match; p.dt_ignore = a.dt_ignore; p.gt_ignore = a.gt_ignore; p.gt_match = a.gt_match;
    p.sum_d = a.sum_d; p.sum_g = a.sum_g;
    p.A = a.A; p.T = a.T; p.max_d = a.max_d; p.max_g = a.max_g;
    p.cap = a.max_g < TILE_CAP ? a.max_g : TILE_CAP;
    if (q.lds_bytes > 64 * 1024 &&
        tmr_set_max_lds((const void *)coco_match_kernel, (size_t)q.lds_bytes) != hipSuccess)
        return TMR_E_HIP;
    hipLaunchKernelGGL(coco_match_kernel, dim3((unsigned)q.blocks), dim3((unsigned)q.threads),
                       (size_t)q.lds_bytes, tmr_stream(stream), p);
    TMR_CHECK_LAUNCH();
    return TMR_OK;
}
