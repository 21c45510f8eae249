/* tmr_points_chain.h -- an optional extension of libtmr.so: decoder_b's whole
 * chain at the detected candidates only.
 *
 * Not part of the core ABI of tmr.h (TMR_ABI_VERSION is unchanged by it); the
 * operands are tmr.h's: the packed records and weights of tmr_split_xpack /
 * tmr_split_wpack, the tiled accumulator layout (TMR_SIZE_ACC), the flags'
 * tile window and the tile list of tmr_split_conv_points. */
#ifndef TMR_POINTS_CHAIN_H
#define TMR_POINTS_CHAIN_H

#include "tmr.h"

#ifdef __cplusplus
extern "C" {
#endif

/* tmr_split_conv_points_chain: the shared route's per-image store launch AND
 * its heads launch at a list of points, without the acc0 slab between them.
 * For every candidate listed by `tiles` (as tmr_split_conv_points) it computes
 * what these three calls write into b at that candidate's pixel, bit for bit:
 *   tmr_split_conv(xp0, C0, NULL, NULL, 0, B, .., wpack_fp, wmax_fp, xmax0,
 *                  zero bias, N, 0, NULL, bias_plane, acc0, TMR_SPLIT_TILED_OUT |
 *                  TMR_SPLIT_XMAX_PER_UNIT | TMR_SPLIT_TILED_INIT | _INIT_BCAST)
 *   tmr_split_conv(NULL, 0, unit_image, xp1, C1, U, .., wpack, wmax, xmax1, bias,
 *                  N, leaky, headw, acc0, partials, TMR_SPLIT_TILED_INIT |
 *                  TMR_SPLIT_XMAX_PER_UNIT | window)
 *   tmr_heads_reduce over the window
 * One workgroup runs, per accumulator element, acc = bias_plane * s_x0 s_w0,
 * phase 0 (the image's records xp0 of unit_image[u], wpack_fp, the per-image
 * scale xmax0[unit_image[u]]), then acc * (1 / s_x0 s_w0) and * s_x1 s_w1 as
 * two separately rounded fp32 multiplies (the slab's store and reload, also
 * where one of them under- or overflows), phase 1 (the unit's records xp1,
 * wpack, xmax1[u]) and the heads.  The slab is neither read nor written.
 * xmax0 is float[images], xmax1 float[U]; bias_plane is NULL or ONE tiled fp32
 * slab (TMR_SIZE_ACC(1, N, H, W)); both weight packs hold the same N.  flags:
 * the tile window only (at most 8 tiles).  TMR_PREC_F16X3 and ks = 3; anything
 * else returns TMR_E_UNSUPPORTED (run the store launch's window and
 * tmr_split_conv_points instead). */
int tmr_split_conv_points_chain(const void *xp0, int C0, const float *xmax0, const void *wpack_fp,
                                const float *wmax_fp, const float *bias_plane, const int32_t *unit_image,
                                const void *xp1, int C1, const float *xmax1, const void *wpack, const float *wmax,
                                int U, int H, int W, int ks, int prec, const float *bias, int N, int leaky,
                                const float *headw, const float *head_bias, const float *box,
                                const int32_t *tiles, int ntiles, float *b, int flags, void *stream);

#ifdef __cplusplus
}
#endif

#endif
