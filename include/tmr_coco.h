/* tmr_coco.h -- the optional evaluation extension of libtmr.so for COCO AP: the
 * per-image detection / ground-truth matching of pycocotools' COCOeval.evaluateImg
 * (iouType 'bbox'; reference utils/log_utils.py:137-205 through COCOeval), for
 * every image, area range and IoU threshold in one call.
 *
 * Not part of the core ABI of tmr.h (TMR_ABI_VERSION is unchanged by it): one
 * entry point and its host-side plan query, exported by the same libtmr.so, as
 * tmr_refine.h.  Accumulation (precision / recall tables) stays the caller's.
 *
 * LAYOUT.  Images i = 0..I-1 own the detections det_off[i] .. det_off[i+1]-1 and
 * the ground truths gt_off[i] .. gt_off[i+1]-1 (CSR; det_off[0] = gt_off[0] = 0,
 * det_off[I] = sum_d, gt_off[I] = sum_g).  Boxes are (x, y, w, h) in fp64.  The
 * detections of an image are ALREADY in descending score order (stable) and cut
 * to the largest maxDets; the kernel never sees a score.  Indices below ("d",
 * "g") are positions inside the image, in the order given.
 *
 * THE RULE.  Every operation is one IEEE fp64 operation rounded on its own (no
 * fused multiply-add); a < b ? a : b is written min(a, b).
 *   IoU o(d, g), with (dx, dy, dw, dh) = det_box[d], (gx, gy, gw, gh) = gt_box[g]:
 *     w = min(dx + dw, gx + gw) - max(dx, gx)
 *     h = min(dy + dh, gy + gh) - max(dy, gy)
 *     if (w > 0 && h > 0):
 *        inter = w * h;  da = dw * dh;  ga = gw * gh
 *        u = gt_crowd[g] ? da : (da + ga) - inter
 *        o = inter / u
 *     else o = 0
 *   (det_area / gt_area take no part in the IoU: they only decide ignoring.)
 *   Area range a = (lo, hi) = area_rng[a]:
 *     gt_ignore[a][g] = gt_crowd[g] || gt_area[g] < lo || gt_area[g] > hi
 *   Threshold t: thr = min(iou_thr[t], 1 - 1e-10).  iou_thr is used as given.
 *   For each (a, t) on its own, the detections d = 0, 1, ... IN ORDER:
 *     candidates: the g with o(d, g) >= thr that are unmatched at (a, t) or crowd;
 *     among the candidates with gt_ignore[a][g] == 0 take the largest o, of equal
 *     o the LARGEST g; only when no such candidate exists, the same choice among
 *     the candidates with gt_ignore[a][g] == 1;
 *     a match m:  dt_match[a][t][d] = m + 1,  gt_match[a][t][m] = d + 1 (a crowd
 *       ground truth keeps the last detection matched to it),
 *       dt_ignore[a][t][d] = gt_ignore[a][m], and m is matched at (a, t);
 *     no match:   dt_match[a][t][d] = 0,
 *       dt_ignore[a][t][d] = det_area[d] < lo || det_area[d] > hi.
 *   gt_match entries of unmatched ground truths are 0.
 * This is eval_log.bbox_iou and CocoEvalMaxDets._evaluate_img (pycocotools scans
 * the ground truths sorted by gt_ignore, stably, and keeps the last one reaching
 * the running best IoU: the same choice).
 *
 * Limits: 0 <= I, 1 <= A, 1 <= T <= 16, I * A < 2^31, detections per image
 * <= 4096 and ground truths per image <= 65536 (max_d / max_g, the per-image
 * maxima, which the caller computes from its host-side offsets); otherwise
 * TMR_E_INVALID: nothing is ever truncated.  I = 0 is a no-op.  Everything is
 * enqueued on `stream`; nothing synchronises with the host.  Every element of
 * the four outputs is written.  An image whose counts contradict max_d / max_g
 * or sum_d / sum_g is skipped by the kernel (memory safety only).
 */
#ifndef TMR_COCO_H_
#define TMR_COCO_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TMR_COCO_T_MAX 16
#define TMR_COCO_D_MAX 4096
#define TMR_COCO_G_MAX 65536

/* tmr_coco_match_plan_t.variant */
#define TMR_COCO_VARIANT_LDS 0    /* the image's ground truths stay in LDS for the whole scan */
#define TMR_COCO_VARIANT_GLOBAL 1 /* more ground truths than the tile: read from global memory */

typedef struct tmr_coco_match_args {
    const int64_t *det_off;   /* [I+1] */
    const double *det_box;    /* [sum_d][4] */
    const double *det_area;   /* [sum_d] */
    const int64_t *gt_off;    /* [I+1] */
    const double *gt_box;     /* [sum_g][4] */
    const double *gt_area;    /* [sum_g] */
    const uint8_t *gt_crowd;  /* [sum_g] */
    const double *area_rng;   /* [A][2] device */
    const double *iou_thr;    /* [T] device */
    int32_t *dt_match;        /* out [A][T][sum_d] */
    uint8_t *dt_ignore;       /* out [A][T][sum_d] */
    uint8_t *gt_ignore;       /* out [A][sum_g] */
    int32_t *gt_match;        /* out [A][T][sum_g] */
    int64_t sum_d, sum_g;     /* det_off[I], gt_off[I] */
    int32_t I, A, T;
    int32_t max_d, max_g;     /* max over images of the per-image counts */
    int32_t pad_;
} tmr_coco_match_args_t;

typedef struct tmr_coco_match_plan {
    int32_t variant;    /* TMR_COCO_VARIANT_*: what serves the image with max_g ground truths */
    int32_t tile_cap;   /* ground truths one LDS tile holds: images up to it take the LDS variant */
    int32_t list_cap;   /* candidates per detection the LDS list holds before the serial rescan */
    int32_t threads;    /* threads per block */
    int32_t lds_bytes;  /* dynamic LDS per block */
    int32_t blocks;     /* I * A: one block per (image, area range) */
} tmr_coco_match_plan_t;

/* stream: a hipStream_t.  Returns TMR_OK or a TMR_E_* code of tmr.h. */
int tmr_coco_match(const tmr_coco_match_args_t *args, void *stream);

/* The launch tmr_coco_match(args) would make, from the host: the same
 * validation (tmr_coco_match itself decides through it), nothing launched, no
 * buffer dereferenced.  Returns what tmr_coco_match returns before its launch;
 * on TMR_OK (I = 0 included, whatever the pointers):
 *  tile_cap = 4096, list_cap = 512;
 *  variant = max_g <= tile_cap ? LDS : GLOBAL (each block picks by its own
 *   image's count: a launch may mix both);
 *  threads = max_g <= 1024 ? 256 : 1024;
 *  lds_bytes = 12304 + 36 * min(max_g, tile_cap): both candidate lists and the
 *   staged boxes and state words of the largest image the LDS variant serves;
 *  blocks = I * A.
 * Otherwise the plan is zeroed. */
int tmr_coco_match_plan(const tmr_coco_match_args_t *args, tmr_coco_match_plan_t *plan);

#ifdef __cplusplus
}
#endif
#endif /* TMR_COCO_H_ */
