/* tmr_refine.h -- the optional evaluation extension of libtmr.so: the mask-to-box
 * step of the SAM box refiner (reference utils/box_refine.py:158-176, 232-246).
 *
 * Not part of the core ABI of tmr.h (TMR_ABI_VERSION is unchanged by it): one
 * entry point and its host-side plan query, exported by the same libtmr.so, for callers that run the
 * reference's --refine_box evaluation.  The mask decoder and the prompt
 * encoder stay the caller's modules; this is what follows them.
 *
 * tmr_mask_boxes: N low-resolution mask logit planes float[N][h][w] -> per
 * mask the tight integer box of the pixels that are positive after the
 * reference's F.interpolate(masks, (H, W), mode="bilinear", align_corners=True),
 * then the reference's box / reference-point / score arithmetic.  The
 * [N][H][W] plane is never written anywhere.
 *
 * INTERPOLATION RULE.  Every operation below is an fp32 operation rounded on
 * its own (no fused multiply-add):
 *     sy = (H > 1) ? (float)(h - 1) / (float)(H - 1) : 0.0f     (sx likewise from w, W)
 *   output pixel (Y, X):
 *     yr = sy * (float)Y;  y0 = (int)yr;  y1 = y0 + (y0 < h - 1);
 *     ly = yr - (float)y0;  hy = 1.0f - ly                       (x0, x1, lx, hx likewise)
 *     a = m[y0][x0], b = m[y0][x1], c = m[y1][x0], d = m[y1][x1]
 *     v = hy * (hx * a + lx * b) + ly * (hx * c + lx * d)
 *   the pixel belongs to the mask iff v > 0 (a NaN v does not).
 * ibox = (min X, min Y, max X, max Y) over the mask's pixels; a mask without a
 * positive pixel gives (0, 0, 0, 0), as the reference's torch.zeros row.
 * The kernel skips a low-resolution cell when its four corners all compare
 * <= 0: the weights are non-negative, so no pixel of that cell can be positive
 * and the skip is exact; a NaN corner fails the comparison and the cell is
 * evaluated literally.
 *
 * EPILOGUE, fp32, in the reference's order of operations:
 *   TMR_REFINE_FORWARD (box_refine.py:244-246, 253):
 *     box = (float)ibox / (W, H, W, H)
 *     ref = ((box0 + box2) / 2, (box1 + box3) / 2)
 *     logits_out = (iou * logits[.][0], 0 * logits[.][1])
 *   TMR_REFINE_SCALED (forward_refine, box_refine.py:170-176, 183): box as
 *     above, then
 *     cx = (box0 + box2) / 2, cy = (box1 + box3) / 2
 *     ltrb = (cx - box0, cy - box1, box2 - cx, box3 - cy) * scaler[0..3]
 *     box = (cx - l, cy - t, cx + r, cy + b);  ref from the new box as above
 *     logits_out as above.  IEEE semantics carry through (an infinite scaler
 *     times a zero extent is NaN, as in the reference).
 *
 * Limits: 1 <= h, H, W <= 65536, 1 <= w <= 4096, 0 <= N and
 * N * ceil(H / band rows) < 2^31; otherwise TMR_E_INVALID.  N = 0 is a no-op.
 * Everything is enqueued on `stream`; nothing synchronises with the host.
 * `work` is TMR_MASK_BOXES_WORK_BYTES(N) bytes of device scratch (16-B
 * aligned), uninitialised on entry.  Outputs are fully written for every n.
 */
#ifndef TMR_REFINE_H_
#define TMR_REFINE_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TMR_REFINE_FORWARD 0
#define TMR_REFINE_SCALED 1

/* bytes of tmr_mask_boxes_args_t.work: one int32[4] box accumulator per mask */
#define TMR_MASK_BOXES_WORK_BYTES(N) ((int64_t)16 * (int64_t)(N))

typedef struct tmr_mask_boxes_args {
    const float *masks;   /* [N][h][w] low-resolution mask logits */
    const float *logits;  /* [N][2] candidate score rows */
    const float *iou;     /* [N] the decoder's IoU predictions */
    const float *scaler;  /* [4] device; TMR_REFINE_SCALED only (else may be NULL) */
    float *boxes;         /* out [N][4] */
    float *refs;          /* out [N][2] */
    float *logits_out;    /* out [N][2] */
    void *work;           /* TMR_MASK_BOXES_WORK_BYTES(N) */
    int64_t N;
    int32_t h, w;         /* mask size */
    int32_t H, W;         /* target (image) size */
    int32_t mode;         /* TMR_REFINE_FORWARD | TMR_REFINE_SCALED */
    int32_t pad_;
} tmr_mask_boxes_args_t;

/* stream: a hipStream_t.  Returns TMR_OK or a TMR_E_* code of tmr.h. */
int tmr_mask_boxes(const tmr_mask_boxes_args_t *args, void *stream);

/* The launch geometry tmr_mask_boxes(args) would use, from the host: the same
 * validation and band rule (tmr_mask_boxes itself decides through it), nothing
 * launched, no buffer dereferenced.  Returns what tmr_mask_boxes returns
 * before its first launch; on TMR_OK (N = 0 included, whatever the pointers):
 *  band_rows: output rows per block -- 16, lowered until the low-resolution
 *   rows such a band can touch, rows(tb) = (tb == 1) ? 2 :
 *   (int)((double)(h - 1) / (H - 1) * (tb - 1) + 0.25) + 3, times w fit the
 *   8192 staged floats;
 *  cap_rows: 8192 / w, the most rows a band stages (>= 2);
 *  nbands: ceil(H / band_rows), blocks per mask.
 * Otherwise the three are zero. */
int tmr_mask_boxes_plan(const tmr_mask_boxes_args_t *args, int32_t *band_rows, int32_t *cap_rows,
                        int32_t *nbands);

#ifdef __cplusplus
}
#endif
#endif /* TMR_REFINE_H_ */
