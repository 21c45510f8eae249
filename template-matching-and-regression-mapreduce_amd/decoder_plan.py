"""The one-layer decoder's route: which launches run with which flag words
(DecoderPlan, pure host arithmetic), and the heads launch's operands
(HeadsLaunch): the full launch, the points route's objectness-only launch and
decoder_b's dense fallback are tile windows of it."""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

from ._lib import (SPLIT_INIT_BCAST, SPLIT_INIT_BF16, SPLIT_OUT_BF16, SPLIT_TILED_INIT, SPLIT_TILED_OUT,
                   SPLIT_UNITS_PER_IMAGE_SHIFT, SPLIT_XMAX_PER_UNIT, call, ptr, split_tile_window, stream)

# the heads launch's image-major block order (an image's units innermost) for
# up to this many units per image: config B (3 per image) 106.6 -> 106.0 ms,
# config E (16 per image) 166.6 -> 168.5 ms.  A/B knob
# TMR_HEADS_IMAGE_MAJOR_MAX (the flags field holds <= 255)
HEADS_IMAGE_MAJOR_MAX = min(255, int(os.environ.get("TMR_HEADS_IMAGE_MAJOR_MAX", "4")))

# where the heads launch's activation scales come from
SCALES_OWN = "own"        # the fp half is its own launch with per-image scales; f_TM per unit
SCALES_MERGED = "merged"  # one launch reads both sources of a tile with ONE scale per image
SCALES_FTM = "ftm"        # no fusion: f_TM per unit only


def units_per_image(unit_image, B: int) -> int:
    """E when the units are E per image in image order (the heads launch
    then runs image-major, TMR_SPLIT_UNITS_PER_IMAGE_SHIFT), else 1."""
    U = len(unit_image)
    E = U // max(B, 1)
    if E <= 1 or E > HEADS_IMAGE_MAJOR_MAX or E * B != U:
        return 1
    ui = np.asarray(unit_image)
    return E if np.array_equal(ui, np.repeat(np.arange(B), E)) else 1


@dataclass(frozen=True)
class DecoderPlan:
    fold: bool      # the fp half runs on [up2x(f)] with weights folded through input_proj (+ bias plane)
    share: bool     # the fp half is computed once per image (acc0) and the heads launch starts from it
    acc16: bool     # acc0 is a bf16 slab
    unscaled: bool  # bf16 records and kernels carry no activation scale
    scales: str     # SCALES_*
    fp_flags: int   # the fp-half launch (share only)
    init_flags: int  # the heads launch's initial-value and scale bits
    epi: int        # its image-major bits
    skip_tiles: int  # box_later: decoder_b's leading 128-channel tiles, left to the regression launches
    # box_later, shared + folded, fp32: the fp-half launch leaves decoder_b's tiles out as well; after the finder
    # they are computed at the candidates (tmr_split_conv_points_chain) or by a late store launch (fp_window)
    fp_late: bool = False

    def window(self, ntiles: int) -> Tuple[int, int]:
        """(first, count) of the heads launch's channel tiles; (0, 0) = all."""
        return (self.skip_tiles, ntiles - self.skip_tiles) if self.skip_tiles else (0, 0)

    def heads_flags(self, first: int = 0, count: int = 0) -> int:
        return self.init_flags | self.epi | split_tile_window(first, count)

    def points_flags(self) -> int:
        return self.init_flags | split_tile_window(0, self.skip_tiles)

    def fp_window(self, ntiles: int, late: bool = False) -> Tuple[int, int]:
        """(first, count) of the fp-half launch's channel tiles: every tile, or (fp_late) decoder_o's before the
        finder and decoder_b's in the late launch."""
        if not self.fp_late:
            return (0, 0)
        return (0, self.skip_tiles) if late else (self.skip_tiles, ntiles - self.skip_tiles)

    def fp_store_flags(self, ntiles: int, late: bool = False) -> int:
        return self.fp_flags | split_tile_window(*self.fp_window(ntiles, late))


def decoder_plan(cfg, fold_proj: bool, share_fp_half: bool, reuse_image_work: bool, have_feats: bool, U: int,
                 B: int, unit_image, box_later: bool = False, nbt: int = 0, fp_late: bool = False) -> DecoderPlan:
    """The route of decode() over U units of B images.  box_later: only the
    tiles after decoder_b's nbt run in the heads launch.  fp_late (asked for
    by the engine above its floor): the fp-half launch leaves them out too,
    where the chained points launch can stand in for it (shared, folded,
    3-term fp16)."""
    fold = bool(cfg.fusion and fold_proj and have_feats)
    # share the fp half across an image's exemplars when that removes work
    # (U >= 2B), or when the module API keeps it for the image's next calls
    # (one forward per exemplar on the SAME features, demo.py:111, trainer.py:96)
    share = bool(share_fp_half and cfg.fusion and (U >= 2 * B or (reuse_image_work and fold)))
    bf16 = cfg.precision == "bf16"
    # the bf16 contract keeps acc0 and the bias plane in bf16: half the
    # initial-value read, a chip-wide burst before the first MFMA (10.49 -> 10.07
    # ms per 48 units).  Not under "f16" (1e-3 contract: b 1.8e-3 with a bf16 acc0)
    acc16 = share and bf16
    # activation scales are PER SAMPLE (per unit for f_TM and the heads launch, per
    # image for the fp half): a unit's precision never depends on the other units'
    xpu = 0 if bf16 else SPLIT_XMAX_PER_UNIT
    plane = (SPLIT_TILED_INIT | SPLIT_INIT_BCAST | (SPLIT_INIT_BF16 if bf16 else 0)) if fold else 0
    if share:
        fp_flags = SPLIT_TILED_OUT | (SPLIT_OUT_BF16 if acc16 else 0) | xpu | plane
        init = SPLIT_TILED_INIT | (SPLIT_INIT_BF16 if acc16 else 0)
    else:
        fp_flags, init = 0, plane
    return DecoderPlan(fold, share, acc16, bf16, SCALES_OWN if share else SCALES_MERGED if cfg.fusion else SCALES_FTM,
                       fp_flags, init | xpu, units_per_image(unit_image, B) << SPLIT_UNITS_PER_IMAGE_SHIFT,
                       nbt if box_later else 0,
                       bool(fp_late and box_later and nbt > 0 and share and fold and cfg.precision == "fp32"))


def fp_late_bound_macs(B: int, H: int, W: int, nbt: int, C0: int, ks: int) -> int:
    """The most fp_late can save: the MACs of decoder_b's tiles of the fp-half launch."""
    return B * H * W * 128 * nbt * C0 * ks * ks


@dataclass
class HeadsLaunch:
    """Everything the heads launch and the regression launches after it read
    (the tensors stay alive as long as this object does)."""
    xp0: Optional[torch.Tensor]  # the image half's records (None: shared fp half, or no fusion)
    C0: int
    ui: torch.Tensor
    xp1: torch.Tensor
    C1: int
    U: int
    H: int
    W: int
    ks: int
    pc: int
    wp: tuple  # (packed weights, max |w|)
    xmax1: Optional[torch.Tensor]
    bias: torch.Tensor
    N: int
    hw: torch.Tensor
    hb: torch.Tensor
    a0: Optional[torch.Tensor]  # initial values: acc0, or the unshared folded half's bias plane
    part: torch.Tensor
    plan: DecoderPlan
    b: Optional[torch.Tensor] = None  # box_later: the regression map still to fill
    fp: Optional["FpHalf"] = None     # plan.fp_late: the fp-half launch's operands

    def _conv_args(self):
        return (ptr(self.xp0) if self.C0 else None, self.C0, ptr(self.ui), ptr(self.xp1), self.C1, self.U, self.H,
                self.W, self.ks, self.pc, ptr(self.wp[0]), ptr(self.wp[1]), ptr(self.xmax1), ptr(self.bias), self.N,
                1, ptr(self.hw))

    def run(self, first: int = 0, count: int = 0) -> None:
        """tmr_split_conv + heads epilogue over a window of channel tiles."""
        call("tmr_split_conv", *self._conv_args(), ptr(self.a0), ptr(self.part),
             self.plan.heads_flags(first, count), stream())

    def run_points(self, box: torch.Tensor, tiles: torch.Tensor, ntiles: int) -> None:
        """decoder_b + ltrbs_head at the candidates of `tiles` only."""
        call("tmr_split_conv_points", *self._conv_args(), ptr(self.hb), ptr(self.a0), ptr(box), ptr(tiles), ntiles,
             ptr(self.b), self.plan.points_flags(), stream())

    def run_points_chain(self, box: torch.Tensor, tiles: torch.Tensor, ntiles: int) -> None:
        """The fp half's decoder_b tiles, decoder_b's f_TM half and ltrbs_head at the candidates, in one chain."""
        f = self.fp
        call("tmr_split_conv_points_chain", ptr(f.xp0), f.C0, ptr(f.xmax0), ptr(f.wp[0]), ptr(f.wp[1]),
             ptr(f.bplane), ptr(self.ui), ptr(self.xp1), self.C1, ptr(self.xmax1), ptr(self.wp[0]), ptr(self.wp[1]),
             self.U, self.H, self.W, self.ks, self.pc, ptr(self.bias), self.N, 1, ptr(self.hw), ptr(self.hb), ptr(box),
             ptr(tiles), ntiles, ptr(self.b), split_tile_window(0, self.plan.skip_tiles), stream())


@dataclass
class FpHalf:
    """The shared fp-half (store) launch: per image, into the acc0 slab the heads launch starts from."""
    xp0: torch.Tensor
    C0: int
    B: int
    H: int
    W: int
    ks: int
    pc: int
    wp: tuple  # (packed folded weights, max |w|)
    xmax0: Optional[torch.Tensor]
    zero_b: torch.Tensor
    N: int
    bplane: Optional[torch.Tensor]
    acc0: torch.Tensor

    def run(self, flags: int) -> None:
        call("tmr_split_conv", ptr(self.xp0), self.C0, None, None, 0, self.B, self.H, self.W, self.ks, self.pc,
             ptr(self.wp[0]), ptr(self.wp[1]), ptr(self.xmax0), ptr(self.zero_b), self.N, 0, None, ptr(self.bplane),
             ptr(self.acc0), flags, stream())
