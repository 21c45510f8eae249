"""Batched native pipeline of the TMR hot path.

``TMREngine`` runs, for a batch of B images x E exemplars (U = B*E matching
units), everything after the frozen backbone on libtmr.so:

  input_proj (+ upsample x2)     tmr_split_conv + tmr_upsample2x   matching_net.py:50-56
  exemplar templates             tmr_templates       template_matching.py:55-76
  depthwise xcorr + pad + scale  tmr_xcorr           template_matching.py:23-41,97
  decoders + heads (fused)       tmr_split_conv (heads) + tmr_heads_reduce
                                                     regression_head.py, matching_net.py:63-75
  peaks + decode                 tmr_peaks_decode    TM_utils.py:224-305
  NMS over the exemplar union    tmr_nms             TM_utils.py:307-323, demo.py:106-130

The projection is computed once per image and shared by its E units; the
reference recomputes it per exemplar (demo.py:111, trainer.py:96-97), with
bit-identical results, so sharing it changes no output.

Weights are the reference's state_dict tensors (SURVEY.md §8b keys); packed
MFMA layouts are derived caches, rebuilt when a parameter changes.
"""
from __future__ import annotations

import contextlib
import weakref
from dataclasses import dataclass
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import exp_table, graphs, host
from ._lib import (PEAKS_DECODE_ONLY, PEAKS_FIND_ONLY, PEAKS_PROB_SCRATCH, POINTS_TILE, PREC_CODES, SPLIT_OUT_BF16,
                   SPLIT_TILED_OUT, SPLIT_XMAX_PER_PIXEL, UNIT_DTYPE, XCORR_ALGOS, TMRError, call, ptr, require_gpu,
                   size, stream, xcorr)
from .decoder_plan import SCALES_FTM, SCALES_MERGED, FpHalf, HeadsLaunch, decoder_plan, fp_late_bound_macs
from .graphs import _clone_outputs, _GraphBook, _h2d, _units_to_device
from .operands import absmax  # noqa: F401 -- unused here; tests written before operands.py import it from engine
from .operands import (absmax_rows, conv2d_split, fold_proj, pack_split_up, pack_split_w, pack_split_x, pixel_absmax,
                       prec_code, scale_merge)
from .xcorr_cost import mfma_fits, xcorr_choice

NHEAD = 5
NMS_SMALL = 256  # TMR_NMS_SMALL (include/tmr.h)


@dataclass
class PathConfig:
    """The matching_net flags on the path (matching_net.py:13-39)."""
    emb_dim: int = 512
    fusion: bool = True
    squeeze: bool = False
    box_reg: bool = True
    template_type: str = "roi_align"
    feature_upsample: bool = True
    decoder_num_layer: int = 1
    decoder_kernel_size: int = 3
    no_matcher: bool = False
    # decoder-conv and MFMA-correlation arithmetic: "fp32" (3-term fp16 split
    # on 16-bit MFMA, the fp32 1e-5 contract), "bf16" (config C: one bf16
    # term, 1e-2 contract) or "f16" (one scaled fp16 term)
    precision: str = "fp32"

    @classmethod
    def from_args(cls, args) -> "PathConfig":
        return cls(emb_dim=args.emb_dim, fusion=bool(args.fusion), squeeze=bool(args.squeeze),
                   box_reg=not args.ablation_no_box_regression, template_type=args.template_type,
                   feature_upsample=bool(args.feature_upsample),
                   decoder_num_layer=args.decoder_num_layer,
                   decoder_kernel_size=args.decoder_kernel_size, no_matcher=bool(args.no_matcher),
                   precision=getattr(args, "precision", "fp32"))


@contextlib.contextmanager
def _timed(events: Optional[list]):
    """When `events` is a list (bench.py), append (start, end) HIP events
    recorded on the launch stream around the body."""
    if events is None:
        yield
        return
    ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    ev[0].record()
    yield
    ev[1].record()
    events.append(ev)


def _version_key(ts: Sequence[torch.Tensor]):
    return tuple((t.data_ptr(), t._version, tuple(t.shape)) for t in ts)


class _PackCache:
    """Derived weight layouts keyed on the parameters' storage and version AND
    on the tensor objects themselves (weak references): a rebuilt tensor that
    reuses a freed address at _version 0 never hits a stale entry."""

    def __init__(self):
        self._d: Dict[str, Tuple[tuple, tuple, object]] = {}

    def get(self, name: str, tensors: Sequence[torch.Tensor], build):
        key = _version_key(tensors)
        hit = self._d.get(name)
        if hit is not None and hit[0] == key and all(r() is t for r, t in zip(hit[1], tensors)):
            return hit[2]
        val = build()
        self._d[name] = (key, tuple(weakref.ref(t) for t in tensors), val)
        return val


@dataclass
class _ImageMemo:
    """What reuse_image_work keeps of the last feature tensor: its projection
    and, once decode() has run, the decoder's per-image fp half."""
    feats: "weakref.ref"
    version: int
    data_ptr: int
    pkey: tuple    # TMREngine._proj_key(): what the projection's values depend on
    params: tuple  # weak references to the input_proj parameters
    fp: Optional[torch.Tensor]
    split: object = None  # the packed decoder halves acc0 was computed with
    size: Optional[tuple] = None
    acc0: Optional[torch.Tensor] = None

    def is_for(self, feats: torch.Tensor) -> bool:
        return self.feats() is feats and self.version == feats._version and self.data_ptr == feats.data_ptr()


class TMREngine:
    """Native forward + post-processing over (image, exemplar) units."""

    def __init__(self, params: Dict[str, torch.Tensor], cfg: PathConfig):
        self.P = params
        self.cfg = cfg
        self._cache = _PackCache()
        # when lists (bench.py), the heads launch and the correlation kernel
        # append (start, end) events recorded around them (_timed)
        self.decoder_events = self.xcorr_events = None
        self.xcorr_split_events = []  # (start, end) of each timed launch's tmr_template_split
        self.last_xcorr_flops = self.last_xcorr_bytes = self.last_xcorr_dram_bytes = 0.0
        # conv(cat[fp, f_TM]) = conv_fp(fp) + conv_tm(f_TM): compute conv_fp once
        # per image when several exemplars share it (fp32, changes only the
        # summation order; same 1e-5 contract)
        self.share_fp_half = True
        # every conv runs on the split 16-bit-MFMA implicit GEMM
        # (conv_split.hip) in cfg.precision
        prec_code(cfg.precision)
        # split kernel + fusion: run the decoder's fp half on [up2x(f); 1]
        # with weights folded through input_proj (Cin+1 = 257 instead of 512
        # input channels; same linear map, fp32-level rounding differences)
        self.fold_proj = True
        self._absmax_memo: Dict[tuple, tuple] = {}
        # correlation kernel: "auto" (the crossover rule, xcorr_cost.py), "valu"
        # or "mfma" (csrc/xcorr.hip)
        self.xcorr_algo = "auto"
        self.last_xcorr_algo = None
        self.last_nms_small = False  # detect: the kept rows came from the in-forward small NMS
        # bf16 contract, detect path: the one-term MFMA correlation writes
        # f_TM as bf16 (the decoder's bf16 records are bf16(f_TM) either way)
        self.out_bf16 = True
        self.last_xcorr_out16 = False
        # keep an image's projection and decoder fp half for the next call on
        # the same feature tensor (the module API's per-exemplar calls)
        self.reuse_image_work = False
        self._memo: Optional[_ImageMemo] = None
        self._graphs = _GraphBook(self.GRAPH_CACHE)
        self._pnames = None
        self.last_graph = self.last_graph_error = self.last_decoder_algo = None
        self.last_decoder_flops = self.last_shared_flops = 0.0
        # detect()'s regression route of the last call ("points" / "dense";
        # None: the fused dense launch), its candidates and the points
        # launch's direct conv FLOPs (whole tiles of POINTS_TILE points)
        self.last_box_route = None
        self.last_points = 0
        self.last_points_flops = 0.0
        self._box_ctx: Optional[HeadsLaunch] = None  # decode(box_later=True)'s heads launch
        self._fp_late_lost: Dict[tuple, bool] = {}  # box_fp_at_points "auto": shapes whose last call lost the cost rule
        if cfg.decoder_kernel_size not in (1, 3, 5, 7):
            raise TMRError("decoder_kernel_size must be 1, 3, 5 or 7")

    # ------------------------------------------------------------ weights
    def _dec_layers(self, pre: str):
        return [(self.P[f"{pre}.layer.{2 * l}.weight"], self.P[f"{pre}.layer.{2 * l}.bias"])
                for l in range(self.cfg.decoder_num_layer)]

    def _fused_decoders(self, split_c0: int = 0, fold: bool = False):
        """Layer-0 weights of decoder_b and decoder_o concatenated along N, with
        the 1x1 heads as a [Npad,5] epilogue matrix (only for 1-layer decoders).
        split_c0 > 0 additionally packs the input-channel halves [:c0] / [c0:]
        (conv(cat[fp, f_TM]) = conv_fp(fp) + conv_tm(f_TM)).  fold (split
        kernel, fusion) replaces the fp half by its fold through input_proj:
        conv_fp(proj(x)) = conv'([x; 1]) (tmr_split_fold_proj), Cin+1 channels."""
        cfg = self.cfg
        layers = [self._dec_layers(pre)[0] for pre in (["decoder_b"] if cfg.box_reg else []) + ["decoder_o"]]
        ow, ob = self.P["objectness_head.head.0.weight"], self.P["objectness_head.head.0.bias"]
        heads = [ow, ob]
        if cfg.box_reg:
            lw, lb = self.P["ltrbs_head.head.0.weight"], self.P["ltrbs_head.head.0.bias"]
            heads += [lw, lb]
        tensors = [t for wb in layers for t in wb] + heads
        if fold:
            pw_, pb_ = self.P["input_proj.0.weight"], self.P["input_proj.0.bias"]
            tensors += [pw_, pb_]

        def build():
            W = torch.cat([w.detach().float() for w, _ in layers], 0).contiguous()
            Bv = torch.cat([b.detach().float() for _, b in layers], 0).contiguous()
            N = W.shape[0]
            npad = ((N + 127) // 128) * 128
            hw = torch.zeros((npad, NHEAD), device=W.device, dtype=torch.float32)
            hb = torch.zeros(NHEAD, device=W.device, dtype=torch.float32)
            n0 = 0
            if cfg.box_reg:
                nb = layers[0][0].shape[0]
                hw[:nb, 0:4] = lw.detach().float().reshape(4, nb).t()
                hb[0:4] = lb.detach().float()
                n0 = nb
            no = layers[-1][0].shape[0]
            hw[n0:n0 + no, 4] = ow.detach().float().reshape(no)
            hb[4] = ob.detach().float().reshape(())
            c0_full = split_c0 or (cfg.emb_dim if cfg.fusion else 0)
            W0, W1, wbias = W[:, :c0_full], W[:, c0_full:], None  # the image half, the f_TM half
            if fold:
                # fp half folded through input_proj: [N, Cin+1, k, k]; the
                # constant-1 channel's conv is a fixed plane per map size
                # (_bias_plane), so the GEMM runs on the Cin channels only
                Wf = fold_proj(W, c0_full, pw_, pb_)
                W0, wbias = Wf[:, :-1], Wf[:, -1:].contiguous()
            c0 = W0.shape[1]
            full = split = None
            if split_c0:
                split = (pack_split_w(W0, c0, cfg.precision), pack_split_w(W1, 0, cfg.precision),
                         torch.zeros(N, device=W.device, dtype=torch.float32))
            else:
                full = pack_split_w(torch.cat([W0, W1], 1), c0, cfg.precision)
            return full, Bv, N, W.shape[1], hw.contiguous(), hb.contiguous(), split, wbias

        return self._cache.get(f"fused_dec{split_c0}_{cfg.precision}_{int(fold)}", tensors, build)

    def _bias_plane(self, wbias: torch.Tensor, H: int, W: int) -> torch.Tensor:
        """conv'(1) of the folded projection bias (wbias [N,1,k,k]): the
        constant-1 input channel of [up2x(f); 1], zero in the conv padding
        like fp's, as one slab in the split kernel's tiled accumulator
        layout (acc_init with TMR_SPLIT_INIT_BCAST).  Cached per weights
        version and map size."""
        N, _, ks, _ = wbias.shape
        prec = self.cfg.precision

        def build():
            dev = wbias.device
            ones = torch.ones((1, 1, H, W), device=dev, dtype=torch.float32)
            one = torch.ones(1, device=dev, dtype=torch.float32)
            xp = pack_split_x(ones, ks, prec, one)
            wp, wmax = pack_split_w(wbias, 1, prec)
            plane = torch.empty(size("acc", 1, N, H, W), device=dev, dtype=torch.float32)
            zero = torch.zeros(N, device=dev, dtype=torch.float32)
            call("tmr_split_conv", ptr(xp), 1, None, None, 0, 1, H, W, ks, prec_code(prec),
                 ptr(wp), ptr(wmax), ptr(one), ptr(zero), N, 0, None, None, ptr(plane),
                 SPLIT_TILED_OUT | (SPLIT_OUT_BF16 if prec == "bf16" else 0), stream())
            return plane

        # a bf16 slab under the bf16 contract (decoder_plan reads it with
        # INIT_BF16): its broadcast read is the fp-half store's initial-value
        # burst, 9% of that launch in fp32
        return self._cache.get(f"bias_plane_{H}x{W}_{prec}", [wbias], build)

    def _conv(self, name: str, x: torch.Tensor, w: torch.Tensor, b: torch.Tensor, leaky: bool):
        """One nn.Conv2d (+ LeakyReLU) of the general-depth stack on the
        split decoder kernel."""
        prec = self.cfg.precision
        wp = self._cache.get(f"{name}_split_{prec}", [w], lambda: pack_split_w(w, w.shape[1], prec))
        return conv2d_split(x, w, b, leaky, prec, wp)

    # ------------------------------------------------------------ forward
    def _feat_absmax(self, feats: torch.Tensor) -> torch.Tensor:
        """max |feats[b]| per image as a device [B] tensor (memoised per
        tensor): the per-image scale source of the up2x(f) records (bilinear
        weights are convex, so max |up2x(f)| <= max |f|).  None under the
        bf16 contract: bf16 records and kernels are unscaled."""
        if self.cfg.precision == "bf16":
            return None
        return self._memo_absmax(feats, "feat", lambda: absmax_rows(feats))

    def _memo_absmax(self, t: torch.Tensor, tag: str, compute):
        """Device max scalars memoised per tensor OBJECT and version (a freed
        tensor's address reused by another never hits)."""
        key = (t.data_ptr(), tag)
        hit = self._absmax_memo.get(key)
        if hit is not None and hit[0]() is t and hit[1] == t._version:
            return hit[2]
        val = compute()
        self._absmax_memo[key] = (weakref.ref(t), t._version, val)
        return val

    def project(self, feats: torch.Tensor, want_f0: bool = False):
        """fp = input_proj(up2x(feats)) [B,emb,H,W] (+ f0 = up2x(feats))."""
        require_gpu(feats, "features")
        feats = feats.float().contiguous()
        B, Cin, Hin, Win = feats.shape
        self._absmax_memo = {}
        up = self.cfg.feature_upsample
        H, W = (2 * Hin, 2 * Win) if up else (Hin, Win)
        # 1x1 conv on the split kernel from records of up2x(f) packed
        # straight from the SAM features; f[0] (the module API output,
        # matching_net.py:81) by the upsample kernel alone.  The fp32-grade
        # 3-term split except under the bf16 contract, where fp feeds only
        # one-term bf16 arithmetic downstream (the correlation and the
        # decoders' f_TM half; the fp half is folded from the features):
        # one bf16 term here too (forward error measured within 1e-2)
        pprec = "bf16" if self.cfg.precision == "bf16" else "fp32"
        pcode = prec_code(pprec)
        pw, pb = self.P["input_proj.0.weight"], self.P["input_proj.0.bias"]
        N, Cw = pw.shape[0], pw.shape[1]
        if Cw != Cin:
            raise TMRError(f"input_proj expects {Cw} channels, got {Cin}")
        wp, wmax = self._cache.get(f"proj_split_{pprec}", [pw], lambda: pack_split_w(pw, Cin, pprec))
        # one activation scale per feature PIXEL (the max over its channels):
        # the templates are cut from fp and renormalised per (unit, channel)
        # by the correlation, so a quiet region of an image must keep its
        # own fp32-grade precision (tests/test_gpu_precision.py (b))
        xmax = None if pprec == "bf16" else pixel_absmax(feats)
        if xmax is not None and self.cfg.precision != "bf16":
            # max |f| per image (the fp half's record scale, _feat_absmax) is
            # the max of these per-pixel maxima: no second read of the features
            self._memo_absmax(feats, "feat", lambda: absmax_rows(xmax))
        # the 1x1 projection commutes with the bilinear x2 (both linear;
        # the interpolation weights of each output sum to 1, so the bias
        # passes through): project at the features' size, then upsample
        # the projection -- a quarter of the MFMA work
        # (input_proj(up2x(f)) and up2x(input_proj(f)) differ in fp32
        # rounding only)
        xp = pack_split_up(feats, False, 1, pprec, xmax, ones=False)
        fq = torch.empty((B, N, Hin, Win), device=feats.device, dtype=torch.float32)
        call("tmr_split_conv", ptr(xp), Cin, None, None, 0, B, Hin, Win, 1, pcode, ptr(wp),
             ptr(wmax), ptr(xmax), ptr(pb.detach().float().contiguous()), N, 0, None, None, ptr(fq),
             SPLIT_XMAX_PER_PIXEL if xmax is not None else 0, stream())
        if up:
            fp = torch.empty((B, N, H, W), device=feats.device, dtype=torch.float32)
            call("tmr_upsample2x", ptr(fq), B * N, Hin, Win, ptr(fp), stream())
        else:
            fp = fq
        return fp, (self._f0(feats) if want_f0 else None)

    def _f0(self, feats: torch.Tensor) -> torch.Tensor:
        """f[0] = up2x(feats), the module API output (matching_net.py:81): a
        fresh tensor per call, like the reference's."""
        if not self.cfg.feature_upsample:
            return feats
        B, Cin, Hin, Win = feats.shape
        f0 = torch.empty((B, Cin, 2 * Hin, 2 * Win), device=feats.device, dtype=torch.float32)
        call("tmr_upsample2x", ptr(feats.float().contiguous()), B * Cin, Hin, Win, ptr(f0), stream())
        return f0

    def match(self, fp: torch.Tensor, unit_image: Sequence[int], unit_boxes: np.ndarray,
              want_relu: bool = False, allow_bf16: bool = False):
        """TemplateMatching.forward over units -> f_TM [U,C|1,H,W] (+ relu).
        allow_bf16: the caller only packs f_TM into bf16 decoder records (the
        bf16 contract's detect path), so the one-term bf16 MFMA kernel may
        write it as bf16 (tmr_xcorr out_bf16; the records are bit-identical)."""
        B, C, H, W = fp.shape
        U = len(unit_image)
        cfg = self.cfg
        units, tfl, mh, mw = host.build_units(unit_boxes, unit_image, H, W, C, cfg.template_type)
        dev = fp.device
        units_d = _units_to_device(units, dev, tag="units")
        img_units = host.image_ranges(unit_image, B)  # units are sorted by image
        img_units_d = _h2d(np.asarray(img_units), dev, tag="img_units")
        tmpl = torch.empty(max(tfl, 1), device=dev, dtype=torch.float32)
        call("tmr_templates", ptr(fp), B, C, H, W, ptr(units_d), U, mh, mw, ptr(tmpl), stream())
        Co = 1 if cfg.squeeze else C
        work = torch.empty((U, C, H, W), device=dev, dtype=torch.float32) if cfg.squeeze else None
        scale = self.P["matcher.scale"].detach().float().contiguous()
        # max |f_TM| per unit fused in the kernel (the decoder's per-unit
        # activation scale source)
        slots = torch.zeros(U, device=dev, dtype=torch.float32)
        min_k = int(min(units["ht"].min(), units["wt"].min()))
        # MFMA operand precision: the fp32 path's 3-term split, or one bf16 /
        # fp16 term under the bf16 contract (config C); the VALU kernels are fp32
        pc = prec_code(cfg.precision)
        choice = self.xcorr_algo
        if choice == "auto":  # measured per-k cost model (xcorr_cost.py)
            choice = xcorr_choice(units["ht"], units["wt"], U / max(1, len(set(unit_image))),
                                  mfma_fits(W, mh, mw), one_term=pc != PREC_CODES["fp32"])
        self.last_xcorr_algo = choice
        algo = XCORR_ALGOS[choice]
        out16 = (allow_bf16 and self.out_bf16 and pc == PREC_CODES["bf16"] and algo == XCORR_ALGOS["mfma"]
                 and not cfg.squeeze and not want_relu and W % 8 == 0)
        self.last_xcorr_out16 = out16
        out = torch.empty((U, Co, H, W), device=dev, dtype=torch.bfloat16 if out16 else torch.float32)
        relu = torch.empty_like(out) if want_relu else None
        tsplit, rows = None, 0
        if algo != XCORR_ALGOS["valu"] and tfl > 0:
            # the MFMA correlation's template operands (per (unit, channel) scale)
            rows = host.tsplit_rows(units)
            tsplit = torch.empty(size("template_split", U, C, rows), device=dev, dtype=torch.uint8)
            # (bench.py times the correlation kernel alone and, separately, its template split)
            with _timed(self.xcorr_split_events if self.xcorr_events is not None else None):
                call("tmr_template_split", ptr(tmpl), ptr(units_d), U, C, rows, pc, ptr(tsplit), stream())
        with _timed(self.xcorr_events):
            xcorr(f=ptr(fp), templates=ptr(tmpl), units=ptr(units_d), img_units=ptr(img_units_d), scale=ptr(scale),
                  out=ptr(out), relu_out=ptr(relu), work=ptr(work), out_absmax=ptr(slots), tmpl_split=ptr(tsplit),
                  total_rows=rows, B=B, C=C, H=H, W=W, U=U, max_ht=mh, max_wt=mw, squeeze=int(cfg.squeeze),
                  algo=algo, min_k=min_k, prec=pc, out_bf16=int(out16), stream=stream())
        # SURVEY.md 8d algorithmic work of the launch: per unit 2*C*(H-h+1)(W-w+1)*h*w
        # FLOPs, read + write C*H*W fp32
        ht, wt = units["ht"].astype(np.float64), units["wt"].astype(np.float64)
        self.last_xcorr_flops = float(np.sum(2.0 * C * (H - ht + 1) * (W - wt + 1) * ht * wt))
        self.last_xcorr_bytes = 2.0 * 4 * C * H * W * U
        # the minimum DRAM traffic of this launch: the kernels stage each
        # image's fp plane once for all its units (read once per IMAGE), and
        # write one f_TM plane per unit
        # (fp32 reads; the f_TM write is bf16, 2 B, under out16)
        nimg = len(set(int(i) for i in unit_image))
        self.last_xcorr_dram_bytes = float(C * H * W) * (4.0 * nimg + (2.0 if out16 else 4.0) * U)
        self._memo_absmax(out, "ftm", lambda: slots)
        return out, relu

    def decode(self, fp: torch.Tensor, f_tm: torch.Tensor, unit_image: Sequence[int],
               feats: Optional[torch.Tensor] = None, box_later: bool = False):
        """Decoders + heads over cat([fp[img(u)], f_TM[u]]) -> o [U,1,H,W], b [U,4,H,W]|None.
        feats (the SAM features fp was projected from) enables the folded fp half.
        box_later (box_at_peaks_ok() holds): only decoder_o's channel tiles
        run; b comes back unwritten and box_at_points() / box_dense() fill it
        from the heads launch kept in self._box_ctx."""
        cfg = self.cfg
        ui = _h2d(np.asarray(unit_image, np.int32), f_tm.device, tag="unit_image")
        if cfg.decoder_num_layer != 1:
            return self._decode_stack(fp, f_tm, ui)
        U, C1, H, W = f_tm.shape
        B, dev = fp.shape[0], f_tm.device
        ks, prec, pc = cfg.decoder_kernel_size, cfg.precision, prec_code(cfg.precision)
        # ---- plan: which launches, with which flags
        nbt = self._box_tiles() if box_later else 0
        p = decoder_plan(cfg, self.fold_proj, self.share_fp_half, self.reuse_image_work, feats is not None, U, B,
                         unit_image, box_later, nbt, box_later and feats is not None and
                         self._fp_at_points_wanted(B, H, W, nbt, feats.shape[1], ks, U))
        Cfp = fp.shape[1] if cfg.fusion else 0
        wp, bias, N, Cw, hw, hb, split, wbias = self._fused_decoders(Cfp if p.share else 0, p.fold)
        if Cw != Cfp + C1:
            raise TMRError(f"decoders expect {Cw} input channels, got {Cfp + C1}")
        # ---- operands: scale sources and records of the image half (fp, or
        # up2x(f) + the bias plane when folded) and of f_TM
        C0 = feats.shape[1] if p.fold else Cfp
        bplane = self._bias_plane(wbias, H, W) if p.fold else None
        xmax1 = None if p.unscaled else self._memo_absmax(f_tm, "ftm", lambda: absmax_rows(f_tm))
        xp0 = xmax0 = acc0 = None
        if p.scales != SCALES_FTM:
            # max |up2x(f)| <= max |f| (bilinear weights are convex)
            xmax0 = None if p.unscaled else self._feat_absmax(feats) if p.fold else absmax_rows(fp)
            if p.scales == SCALES_MERGED and not p.unscaled:  # per image, max(image half, its units' f_TM)
                xmax0, xmax1 = scale_merge(xmax0, xmax1, ui, B)
            if p.share and p.fold:
                acc0 = self._acc0_lookup(feats, split, H, W)  # the image's cached fp half
            if acc0 is None:
                xp0 = pack_split_up(feats, cfg.feature_upsample, ks, prec, xmax0, ones=False) if p.fold else \
                    pack_split_x(fp, ks, prec, xmax0)
        xp1 = pack_split_x(f_tm, ks, prec, xmax1)
        # ---- launches: the fp half once per image, then the heads launch
        fph, ntiles = None, (N + 127) // 128
        if p.share:
            wp_fp, wp, zero_b = split
            if acc0 is None:  # acc0 in the kernel's tiled accumulator layout (private)
                acc0 = torch.empty(size("acc", B, N, H, W), device=dev, dtype=torch.float32)
                fph = FpHalf(xp0, C0, B, H, W, ks, pc, wp_fp, xmax0, zero_b, N, bplane, acc0)
                # (fp_late: decoder_o's tiles only; decoder_b's part of acc0 stays unwritten until a late store)
                fph.run(p.fp_store_flags(ntiles))
                if p.fold and self.reuse_image_work:
                    self._acc0_store(feats, split, H, W, acc0)
        part = torch.empty(size("heads_partials", N, U, H, W), device=dev, dtype=torch.float32)
        heads = HeadsLaunch(xp0=None if p.share else xp0, C0=0 if p.share else C0, ui=ui, xp1=xp1, C1=C1, U=U, H=H, W=W,
                            ks=ks, pc=pc, wp=wp, xmax1=xmax1, bias=bias, N=N, hw=hw, hb=hb,
                            a0=acc0 if p.share else bplane, part=part, plan=p, fp=fph if p.fp_late else None)
        first, count = p.window(ntiles)
        with _timed(self.decoder_events):
            heads.run(first, count)
        # direct conv FLOPs of the timed launch's channel tiles (the kernel
        # executes 3 16-bit MFMA terms per product under the fp32 contract)
        n_run = 128 * count if box_later else N
        self.last_decoder_flops = 2.0 * H * W * n_run * (heads.C0 + C1) * ks ** 2 * U
        # (the channels the fp-half launch ran: fp_late leaves decoder_b's to _detect_box_at_peaks)
        n_fp = N - 128 * nbt if p.fp_late else N
        self.last_shared_flops = 2.0 * H * W * n_fp * C0 * ks ** 2 * B if p.share else 0.0
        self.last_decoder_algo = "split"
        # o and b as contiguous views of ONE buffer (a graph replay then
        # copies both out with one copy, _clone_outputs)
        ob = torch.empty(U * (5 if cfg.box_reg else 1) * H * W, device=dev, dtype=torch.float32)
        o = ob[:U * H * W].view(U, 1, H, W)
        b = ob[U * H * W:].view(U, 4, H, W) if cfg.box_reg else None
        # (a window's partials sit where the full launch writes them)
        call("tmr_heads_reduce", ptr(part[first * NHEAD * U * H * W:]), n_run, 128, U, H, W, ptr(hb), ptr(o),
             None if box_later else ptr(b), stream())
        if box_later:
            heads.b = b
            self._box_ctx = heads
        return o, b

    def _decode_stack(self, fp, f_tm, ui):
        """General depth: per-decoder conv stack, heads as 1x1 convs."""
        cfg = self.cfg
        x0 = torch.cat([fp.index_select(0, ui.long()), f_tm], 1) if cfg.fusion else f_tm
        res = {}
        for pre in (["decoder_b"] if cfg.box_reg else []) + ["decoder_o"]:
            x = x0
            for l, (w, bb) in enumerate(self._dec_layers(pre)):
                x = self._conv(f"{pre}.{l}", x, w, bb, True)
            res[pre] = x
        ow, ob = self.P["objectness_head.head.0.weight"], self.P["objectness_head.head.0.bias"]
        o = self._conv("obj", res["decoder_o"], ow, ob, False)
        b = None
        if cfg.box_reg:
            lw, lb = self.P["ltrbs_head.head.0.weight"], self.P["ltrbs_head.head.0.bias"]
            b = self._conv("ltrbs", res["decoder_b"], lw, lb, False)
        return o, b

    # ---- the regression map only where detect() reads it --------------------
    # detect() returns kept boxes, and the decode reads b at the candidates
    # alone (csrc/peaks.hip decode_one): a few percent of the pixels.  On its
    # eager route (no speculative small NMS: more than GRAPH_MAX_UNITS units,
    # or graphs off) detect() therefore runs decoder_o's tiles densely, finds
    # the peaks, reads the counts back (the sync it always had) and computes
    # decoder_b + ltrbs_head at the candidates (tmr_split_conv_points), bit
    # for bit the dense values.  "auto" falls back to decoder_b's dense tiles
    # when the candidates exceed BOX_POINTS_CROSSOVER of the pixels.
    box_at_peaks = "auto"  # "auto" | "always" | "never"
    # (dense decoder_b tiles' time per pixel) / (points launch's time per point), measured on one
    # box at configs B-E (profiles/points_kloop/crossover.json, profiles/points_crossover.py): 3-term fp16
    # 0.57-0.66, one term 0.48 (bf16; f16 has no bench config and keeps bf16's)
    BOX_POINTS_CROSSOVER = {"fp32": 0.57, "bf16": 0.47, "f16": 0.47}

    # ---- decoder_b's fp half only where the candidates are ---------------------
    # On the route above with a shared, folded fp half (fp32 contract) the
    # fp-half launch still computed decoder_b's tiles at every pixel of every
    # image for the points launch to read a few percent of.  Above a floor it
    # now runs decoder_o's tiles alone, and after the counts read-back the
    # regression takes one of three routes: the chained points launch
    # (tmr_split_conv_points_chain: both halves at the candidates, no acc0
    # slab; "points_chain"), or decoder_b's store tiles now -- what the early
    # launch would have cost -- followed by the points launch ("points") or
    # the dense tiles ("dense").  Values are bit-identical on every route.
    box_fp_at_points = "auto"  # "auto" | "always" (no floor, no cost rule: tests) | "never"
    # the cost rule's constants, measured on one box at configs B, D with two exemplars and E (profiles/points_chain/
    # crossover.json, profiles/points_crossover.py --chain): ns the chain adds to the points launch per candidate
    # (11.1-12.7), ns of decoder_b's store tiles per image pixel (9.2-9.3).  Config E (16 units per image: 0.86
    # candidates per image pixel) takes the late store, B (0.17) and D2 (0.11) the chain
    FP_CHAIN_NS_PER_POINT = 12.0
    FP_STORE_NS_PER_PIXEL = 9.3
    # the floor: decoder_b's store tiles in MACs (decoder_plan.fp_late_bound_macs) below which the launches keep
    # today's order.  The same sweep over config B's shapes at 1..64 images: from 16 images on (6.18e11 MACs) the
    # chain route beat the parent's by more than 3x the spread, at 8 images (0.9 of 12.2 ms) by less
    FP_AT_POINTS_FLOOR_MACS = 6.1e11

    def _fp_at_points_wanted(self, B: int, H: int, W: int, nbt: int, C0: int, ks: int, U: int = 0) -> bool:
        """Whether the fp-half launch leaves decoder_b's tiles out.  "auto": above the floor, and not where the
        last call of this shape (images, units, map) ended on a late store: two store launches cost a little more
        than one (config E: +0.1..0.3 ms of 115), so a shape whose candidates keep losing the cost rule goes back
        to today's order until a call's count says the chain would have won (_fp_late_note)."""
        mode = self.box_fp_at_points
        if mode not in ("auto", "always", "never"):
            raise TMRError("box_fp_at_points must be 'auto', 'always' or 'never'")
        return mode == "always" or \
            (mode == "auto" and fp_late_bound_macs(B, H, W, nbt, C0, ks) >= self.FP_AT_POINTS_FLOOR_MACS and
             not self._fp_late_lost.get((B, U, H, W), False))

    def _fp_chain_wins(self, points: int, B: int, H: int, W: int) -> bool:
        """The cost rule: the chain's added time at the candidates against the store tiles' over the images."""
        return points * self.FP_CHAIN_NS_PER_POINT < B * H * W * self.FP_STORE_NS_PER_PIXEL

    def _fp_late_note(self, B: int, U: int, H: int, W: int, wins: bool) -> None:
        if len(self._fp_late_lost) >= 64:  # (shapes seen, bounded)
            self._fp_late_lost.clear()
        self._fp_late_lost[(B, U, H, W)] = not wins

    def _box_tiles(self) -> int:
        """decoder_b's 128-channel tiles at the front of decoder_b || decoder_o."""
        return int(self.P["decoder_b.layer.0.weight"].shape[0]) // 128

    def box_at_peaks_ok(self) -> bool:
        """The points route's preconditions: one fused decoder layer with box
        regression, kernel size 3 (other sizes stay on the dense launch),
        decoder_b in 1..8 whole channel tiles, no per-image memo."""
        cfg = self.cfg
        if self.box_at_peaks == "never" or cfg.decoder_num_layer != 1 or not cfg.box_reg or \
                cfg.decoder_kernel_size != 3 or self.reuse_image_work:
            return False
        if self.box_at_peaks not in ("auto", "always"):
            raise TMRError("box_at_peaks must be 'auto', 'always' or 'never'")
        nb = int(self.P["decoder_b.layer.0.weight"].shape[0])
        return nb % 128 == 0 and 1 <= nb // 128 <= 8

    def box_at_points(self, box: torch.Tensor, tiles: np.ndarray) -> None:
        """b at the candidates of `tiles` (host.point_tiles), from the last
        decode(box_later=True)'s heads launch."""
        if len(tiles):
            td = _h2d(np.ascontiguousarray(tiles, np.int32).reshape(-1), box.device)
            self._box_ctx.run_points(box, td, len(tiles))

    def box_chain_at_points(self, box: torch.Tensor, tiles: np.ndarray) -> None:
        """b at the candidates of `tiles` with decoder_b's fp half computed there too (plan.fp_late: acc0 holds
        decoder_o's tiles only)."""
        if len(tiles):
            td = _h2d(np.ascontiguousarray(tiles, np.int32).reshape(-1), box.device)
            self._box_ctx.run_points_chain(box, td, len(tiles))

    def box_late_store(self) -> None:
        """decoder_b's tiles of the fp-half launch, left out before the finder (plan.fp_late)."""
        h = self._box_ctx
        h.fp.run(h.plan.fp_store_flags((h.N + 127) // 128, late=True))

    def box_dense(self) -> None:
        """b everywhere: decoder_b's tiles of the dense heads launch."""
        h = self._box_ctx
        nbt = h.plan.skip_tiles
        h.run(0, nbt)
        scratch_o = torch.empty(h.U * h.H * h.W, device=h.b.device, dtype=torch.float32)
        call("tmr_heads_reduce", ptr(h.part), 128 * nbt, 128, h.U, h.H, h.W, ptr(h.hb), ptr(scratch_o), ptr(h.b),
             stream())

    def _detect_box_at_peaks(self, feats, unit_image, boxes, params):
        """detect()'s eager forward with the regression at the peaks:
        objectness tiles, finder, counts read-back, points launch (or the
        dense decoder_b tiles), decode.  Returns (logits, box, ref, counts,
        counts_host)."""
        r = self._forward_units_eager(feats, [int(i) for i in unit_image], boxes, box_later=True)
        o, b = r["o"], r["b"]
        U, _, H, W = o.shape
        logits, box, ref, counts, _ = self.peaks(o, None, params, want_prob=False, phase="find")
        counts_host = counts.cpu().numpy()  # torch.where-style sync (TM_utils.py:254)
        need = np.where(params["mode"] != 2, counts_host, 0)
        self.last_points = int(need.sum())
        dense = self.box_at_peaks == "auto" and \
            self.last_points > self.BOX_POINTS_CROSSOVER[self.cfg.precision] * U * H * W
        h = self._box_ctx
        nbt = h.plan.skip_tiles
        # fp_late: the chain where its added time at the candidates is under the store tiles' over the images
        nimg = feats.shape[0]
        wins = not dense and self._fp_chain_wins(self.last_points, nimg, H, W)
        if self.box_fp_at_points == "auto":
            self._fp_late_note(nimg, U, H, W, wins)
        chain = h.plan.fp_late and not dense and (self.box_fp_at_points == "always" or wins)
        self.last_box_route = "dense" if dense else "points_chain" if chain else "points"
        if h.plan.fp_late and not chain:  # decoder_b's store tiles after all, at the early launch's cost
            self.box_late_store()
            self.last_shared_flops += 2.0 * H * W * 128 * nbt * h.fp.C0 * h.ks ** 2 * h.fp.B
        if dense:
            self.box_dense()
            self.last_points_flops = 0.0
        else:
            tiles = host.point_tiles(need, POINTS_TILE)
            (self.box_chain_at_points if chain else self.box_at_points)(box, tiles)
            cin = (h.fp.C0 if chain else h.C0) + h.C1
            self.last_points_flops = 2.0 * 128 * nbt * cin * h.ks ** 2 * POINTS_TILE * len(tiles)
        self._box_ctx = None
        self.peaks(o, b, params, want_prob=False, phase="decode", found=(logits, box, ref, counts))
        return logits, box, ref, counts, counts_host

    # ---------------------------------------------------- per-image reuse
    def _proj_key(self):
        """(params, pkey): the memo follows input_proj's storage, version AND identity
        (as _PackCache), and the path options that change the projection's arithmetic."""
        params = (self.P["input_proj.0.weight"], self.P["input_proj.0.bias"])
        return params, (_version_key(params), self.cfg.precision, self.cfg.feature_upsample)

    def _bind_memo(self, feats: torch.Tensor, fp, split=None, size_=None, acc0=None):
        """Point the per-image memo at (fp, acc0) for `feats`."""
        params, pkey = self._proj_key()
        self._memo = _ImageMemo(weakref.ref(feats), feats._version, feats.data_ptr(), pkey,
                                tuple(weakref.ref(t) for t in params), fp, split, size_, acc0)

    def _fp_lookup(self, feats: torch.Tensor):
        m = self._memo
        params, pkey = self._proj_key()
        hit = m is not None and m.is_for(feats) and m.fp is not None and m.pkey == pkey and \
            all(r() is t for r, t in zip(m.params, params))
        return m.fp if hit else None

    def _acc0_lookup(self, feats, split, H, W):
        m = self._memo
        hit = self.reuse_image_work and m is not None and m.is_for(feats) and m.split is split and m.size == (H, W)
        return m.acc0 if hit else None

    def _acc0_store(self, feats, split, H, W, acc0):
        m = self._memo
        if m is not None and m.is_for(feats):
            m.split, m.size, m.acc0 = split, (H, W), acc0
        else:
            self._bind_memo(feats, None, split, (H, W), acc0)

    def _memo_hit(self, feats: torch.Tensor) -> Optional[_ImageMemo]:
        """The memo when an earlier call kept both fp and acc0 for this feature tensor."""
        return self._memo if self._fp_lookup(feats) is not None and self._memo.acc0 is not None else None

    def _forward_units_graphed(self, feats, unit_image, unit_boxes, want_aux):
        """The module API's per-exemplar forward (reuse_image_work) as a
        replayed HIP graph once its signature recurs.  Two graphs per shape:
        the image's first call (projection + fp half + correlation + heads;
        its fp / acc0 become the image's memo) and the later calls on the same
        features (correlation + heads off that memo).  Outputs are cloned: a
        caller may keep one exemplar's maps while the next replay runs."""
        if not (self.use_graphs and feats.is_cuda and len(unit_image) <= self.GRAPH_MAX_UNITS) or \
                self.decoder_events is not None or self.xcorr_events is not None or self.cfg.no_matcher or \
                self.cfg.decoder_num_layer != 1 or not (self.cfg.fusion and self.fold_proj):
            return None
        B, Cin, Hin, Win = feats.shape
        H, W = (2 * Hin, 2 * Win) if self.cfg.feature_upsample else (Hin, Win)
        C = int(self.P["input_proj.0.weight"].shape[0])
        boxes = np.asarray(unit_boxes, np.float32).reshape(-1, 4)
        units = host.build_units(boxes, unit_image, H, W, C, self.cfg.template_type)[0]
        hit = self._memo_hit(feats)
        base = self._graph_signature(feats, units, unit_image, False, False, module=True)
        if base is None:
            return None
        sig = base + (bool(want_aux), None if hit is None else (hit.fp.data_ptr(), hit.acc0.data_ptr()))
        g = self._graphs.get(sig)
        self.last_graph = "replay" if g is not None else "eager"
        if g is None:
            if not self._graphs.want_capture(sig):
                return None
            g = self._capture_module(feats, unit_image, boxes, want_aux, hit, self._detect_host_inputs(
                units, unit_image, B, np.zeros(0, np.uint8)))
            self._graphs.put(sig, g)
            if g is None:
                return None
            self.last_graph = "captured"
        host_in = self._detect_host_inputs(units, unit_image, B, np.zeros(0, np.uint8))
        out = g.replay(self, feats.float().contiguous(), host_in, reuse_feats=True)
        if hit is None:  # this image's memo: the first-call graph's fp / acc0
            m = g.memo
            self._bind_memo(feats, m.fp, m.split, m.size, m.acc0)
        return _clone_outputs(out)

    def _capture_module(self, feats, unit_image, boxes, want_aux, hit, host_in):
        saved = self._memo

        def run(static):
            if hit is not None:  # the capture reads the memo buffers
                self._bind_memo(static, hit.fp, hit.split, hit.size, hit.acc0)
            else:
                self._memo = None
            return self._forward_units_eager(static, unit_image, boxes, want_aux)

        try:
            g = graphs.capture(self, feats, host_in, run)
            if g is not None and hit is None:
                g.memo = self._memo
                if g.memo is None or g.memo.acc0 is None:  # (share_fp_half off): nothing for later calls to reuse
                    self.last_graph_error, g = "the image's first call kept no fp half: the signature stays eager", None
        finally:
            self._memo = saved
        return g

    def forward_units(self, feats: torch.Tensor, unit_image: Sequence[int], unit_boxes,
                      want_aux: bool = False):
        """One matching_net forward per unit (image unit_image[u], exemplar
        unit_boxes[u]).  Returns dict(o, b, f_tm_relu, f0, fp)."""
        unit_image = [int(i) for i in unit_image]
        if self.reuse_image_work and not graphs.capturing():
            r = self._forward_units_graphed(feats, unit_image, unit_boxes, want_aux)
            if r is not None:
                return r
        return self._forward_units_eager(feats, unit_image, unit_boxes, want_aux)

    def _forward_units_eager(self, feats: torch.Tensor, unit_image: Sequence[int], unit_boxes,
                             want_aux: bool = False, box_later: bool = False):
        fp = self._fp_lookup(feats) if self.reuse_image_work else None
        if fp is not None:
            f0 = self._f0(feats) if want_aux else None
        else:
            fp, f0 = self.project(feats, want_f0=want_aux)
            if self.reuse_image_work:
                m = self._memo  # (an acc0 kept for these features stays with them)
                self._bind_memo(feats, fp, *((m.split, m.size, m.acc0) if m is not None and m.is_for(feats) else ()))
        if self.cfg.no_matcher:
            ui = _h2d(np.asarray(unit_image, np.int64), fp.device, tag="unit_image64")
            f_tm = fp.index_select(0, ui).contiguous()
            relu = torch.relu(f_tm) if want_aux else None
        else:
            # a bf16 f_TM plane only where the decode packs it into bf16
            # records and nothing else reads it
            split1 = self.cfg.decoder_num_layer == 1
            f_tm, relu = self.match(fp, unit_image, np.asarray(unit_boxes, np.float32), want_aux,
                                    allow_bf16=split1 and not want_aux)
        o, b = self.decode(fp, f_tm, unit_image, feats, box_later=box_later)
        return dict(o=o, b=b, f_tm_relu=relu, f0=f0, fp=fp)

    # ------------------------------------------------------------ post
    # the decode's exp (TM_utils.py:272): "reference" = the reference's
    # torch.exp (MKL vsExp) through the recorded table (exp_table.py),
    # "cr" = correctly rounded
    exp_mode = "reference"

    @staticmethod
    def peaks(o: torch.Tensor, b: Optional[torch.Tensor], params: np.ndarray,
              input_is_prob: bool = False, want_prob: bool = True, phase: Optional[str] = None,
              found=None):
        """Peak finder + decode per unit -> (logits, box, ref, counts, prob)
        with per-unit stride H*W; prob is None unless want_prob (without it
        the kernel skips the sigmoid of pixels that cannot matter).
        phase "find": the finder alone (b unused; each box row holds its
        candidate's pixel index); phase "decode": the decode alone over
        found = the (logits, box, ref, counts) of a "find" call."""
        require_gpu(o, "objectness")
        o = o.float().contiguous()
        U = o.shape[0]
        H, W = o.shape[-2:]
        dev = o.device
        cap = H * W
        prm = _h2d(params.view(np.uint8), dev, tag="peak_params")
        bb = b.float().contiguous() if b is not None else None
        tab = exp_table.device_table(dev) if TMREngine.exp_mode == "reference" else None
        flags = int(input_is_prob) | (0 if want_prob else PEAKS_PROB_SCRATCH)
        if phase == "decode":  # (o stands in the prob argument; no prob comes back)
            (logits, box, ref, counts), prob, want_prob = found, o, False
            flags |= PEAKS_DECODE_ONLY
        else:
            prob = torch.empty((U, H, W), device=dev, dtype=torch.float32)  # (scratch unless want_prob)
            logits = torch.empty((U * cap, 2), device=dev, dtype=torch.float32)
            box = torch.empty((U * cap, 4), device=dev, dtype=torch.float32)
            ref = torch.empty((U * cap, 2), device=dev, dtype=torch.float32)
            counts = torch.empty(U, device=dev, dtype=torch.int32)
            if phase == "find":
                flags |= PEAKS_FIND_ONLY
        call("tmr_peaks_decode", ptr(o), flags, ptr(bb), U, H, W, ptr(prm), ptr(prob), ptr(logits), ptr(box),
             ptr(ref), ptr(counts), ptr(tab), stream())
        return logits, box, ref, counts, (prob if want_prob else None)

    @staticmethod
    def eval_loss(o, b, unit_image: Sequence[int], unit_boxes, gt_boxes, *, positive_threshold: float,
                  negative_threshold: float, focal: bool = False, ablation_no_box_regression: bool = False,
                  regression_scaling_imgsize: bool = False, regression_scaling_WH_only: bool = False,
                  groups: Optional[Sequence[int]] = None):
        """The evaluation losses of trainer.py:75-153 (GT_map.Get_pred_gts +
        SetCriterion_TM) fused on the GPU (tmr_gt_loss): no [H*W, G] matrix,
        no gather and no sync.  o / b: the objectness [U,1,H,W] and regression
        [U,4,H,W] maps of forward_units, or lists of them over levels (b may
        be None with ablation_no_box_regression); unit_image[u] indexes
        gt_boxes (a list of per-image [G,4] xyxy boxes, host arrays preferred);
        unit_boxes [U,4] are the exemplars.  `groups` [U] names the units that
        share one num_positive -- one group per model() call of the trainer:
        the whole batch in each_step (None), one exemplar in
        each_step_multi_exemplars.  Returns loss_ce / loss_giou (fp32, 0-d, or
        [groups] when groups is given; the mean over levels), gt_map (per
        level [U,1,H,W]) and the last level's per-unit sums [U,2] fp64
        {sum ce, sum giou}, counts [U,2] int32 {positive, negative pixels} and
        target [U,H,W].  Outputs carry no autograd graph: training and
        backward are out of scope."""
        from . import gt_loss as gl

        os_ = list(o) if isinstance(o, (list, tuple)) else [o]
        bs_ = list(b) if isinstance(b, (list, tuple)) else [b] * len(os_)
        boxes = np.asarray(unit_boxes, np.float32).reshape(-1, 4)
        gtb = gl.host_boxes(gt_boxes)
        ces, gis, maps = [], [], []
        for lv, (ol, bl) in enumerate(zip(os_, bs_)):
            H, W = ol.shape[-2:]
            units = host.gt_units(boxes, unit_image, H, W, not ablation_no_box_regression,
                                  regression_scaling_imgsize, regression_scaling_WH_only)
            st = gl.assign(ol, None if ablation_no_box_regression else bl, units, gtb, positive_threshold,
                           negative_threshold, lv == len(os_) - 1, focal, with_loss=True)
            ce, gi = gl.group_losses(st.sums, st.counts, groups)
            ces.append(ce); gis.append(gi); maps.append(st.gt_map)
        return dict(loss_ce=torch.stack(ces).mean(0), loss_giou=torch.stack(gis).mean(0),
                    gt_map=maps if isinstance(o, (list, tuple)) else maps[0],
                    sums=st.sums, counts=st.counts, target=st.target)

    @staticmethod
    def nms(logits, box, ref, counts: torch.Tensor, counts_host: np.ndarray,
            unit_off: torch.Tensor, seg_units: np.ndarray, iou_threshold: float,
            want_keep: bool = False):
        """Greedy NMS per image over its units' candidates (+ dummy rows).
        counts: the device counts, or None (staged from counts_host);
        unit_off: a device tensor or a host int64 array (staged).  The host
        arrays go to the device as ONE staged copy (this runs right after the
        counts sync, while the GPU idles).  Returns per-image lists of
        (logits, boxes, refs) device tensors (+ keep indices when want_keep)."""
        dev = logits.device
        G = len(seg_units) - 1
        cand_off, nb_off, max_cand = host.nms_offsets(counts_host, seg_units)
        T = int(cand_off[-1])
        sum_nb = int(nb_off[-1])
        work = torch.empty(max(size("nms_work", T, sum_nb, max_cand, G), 1), device=dev,
                           dtype=torch.uint8)
        parts = [np.asarray(seg_units, np.int32), np.asarray(cand_off, np.int64), np.asarray(nb_off, np.int64)]
        if counts is None:
            parts.append(np.asarray(counts_host, np.int32))
        host_off = not isinstance(unit_off, torch.Tensor)
        if host_off:
            parts.append(np.asarray(unit_off, np.int64))
        offs, o = [], 0
        for a in parts:  # 8-B aligned sections of one byte blob
            offs.append(o)
            o += (a.nbytes + 7) // 8 * 8
        blob = np.zeros(max(o, 8), np.uint8)
        for a, q in zip(parts, offs):
            blob[q:q + a.nbytes] = a.view(np.uint8)
        blob_d = _h2d(blob, dev)
        views = [blob_d[q:q + a.nbytes].view(torch.int32 if a.dtype == np.int32 else torch.int64)
                 for a, q in zip(parts, offs)]
        seg_d, coff_d, nboff_d = views[:3]
        rest = views[3:]
        if counts is None:
            counts = rest.pop(0)
        if host_off:
            unit_off = rest.pop(0)
        out_l = torch.empty((T, 2), device=dev, dtype=torch.float32)
        out_b = torch.empty((T, 4), device=dev, dtype=torch.float32)
        out_r = torch.empty((T, 2), device=dev, dtype=torch.float32)
        kept = torch.empty(G, device=dev, dtype=torch.int32)
        keep = torch.empty(T, device=dev, dtype=torch.int64) if want_keep else None
        call("tmr_nms", ptr(logits), ptr(box), ptr(ref), ptr(counts), ptr(unit_off), ptr(seg_d),
             ptr(coff_d), ptr(nboff_d), G, T, max_cand, sum_nb, float(iou_threshold), ptr(out_l), ptr(out_b),
             ptr(out_r), ptr(keep) if keep is not None else None, ptr(kept), ptr(work), stream())
        k = kept.cpu().numpy()  # variable-length result: one sync
        L, Bx, R, K = [], [], [], []
        for g in range(G):
            s, e = int(cand_off[g]), int(cand_off[g]) + int(k[g])
            L.append(out_l[s:e]); Bx.append(out_b[s:e]); R.append(out_r[s:e])
            if keep is not None:
                K.append(keep[s:e])
        return (L, Bx, R, K) if want_keep else (L, Bx, R)

    # detect's forward (projection ... peaks) as a replayed HIP graph when
    # the same launch signature recurs (the reference's per-image loop at one
    # image size and recurring template sizes): the host then issues ONE
    # launch instead of ~30, and the GPU no longer idles while Python prepares
    # them (config A: 0.38 of 2.95 ms per image).  A signature is captured the
    # second time it is seen; up to GRAPH_MAX_UNITS units (the graph's memory
    # pool holds every intermediate) and GRAPH_CACHE entries (graphs.py).
    use_graphs = True
    GRAPH_MAX_UNITS = 32
    GRAPH_CACHE = 8

    def _graph_signature(self, feats: torch.Tensor, units: np.ndarray, unit_image, ablation_b, ablation_c,
                         module: bool = False):
        if not (self.use_graphs and feats.is_cuda and len(unit_image) <= self.GRAPH_MAX_UNITS):
            return None
        if self.decoder_events is not None or self.xcorr_events is not None or \
                (self.reuse_image_work and not module):
            return None  # timed runs record events around single launches; detect has no image memo
        return (tuple(feats.shape), feats.dtype, str(feats.device), tuple(int(i) for i in unit_image),
                tuple(units["ht"].tolist()), tuple(units["wt"].tolist()), tuple(sorted(vars(self.cfg).items())),
                self.fold_proj, self.share_fp_half, self.xcorr_algo, self.out_bf16, TMREngine.exp_mode,
                bool(ablation_b), bool(ablation_c), self._param_key())

    def _param_key(self):
        """(name, storage, version) of every parameter, in name order (the
        sorted names cached while the dict keeps its key set)."""
        P = self.P
        names = self._pnames
        if names is None or names[1] is not P or len(names[0]) != len(P):
            names = self._pnames = (tuple(sorted(P)), P)
        try:
            return tuple((k, P[k].data_ptr(), P[k]._version) for k in names[0])
        except KeyError:  # a key replaced by another: re-sort
            self._pnames = None
            return self._param_key()

    @staticmethod
    def _detect_host_inputs(units, unit_image, B, params, nms=None) -> Dict[str, np.ndarray]:
        """The tagged host inputs of detect's forward, as _h2d stages them
        (nms: the speculative small NMS's (unit_off, seg, iou_threshold))."""
        d = {"units": units.view(np.uint8), "img_units": np.asarray(host.image_ranges(unit_image, B)),
             "unit_image": np.asarray(unit_image, np.int32), "unit_image64": np.asarray(unit_image, np.int64),
             "peak_params": params.view(np.uint8)}
        if nms is not None:
            d["nms_unit_off"], d["nms_seg"] = nms[:2]
        return d

    def _forward_peaks(self, feats, unit_image, boxes, params, nms=None):
        """forward + peak finder; with nms = (unit_off, seg, iou_threshold)
        also the device-sized small NMS (tmr_nms_small) and one int32 tensor
        [counts..., kept...] to read back with a single sync."""
        r = self.forward_units(feats, unit_image, boxes)
        logits, box, ref, counts, _ = self.peaks(r["o"], r["b"], params, want_prob=False)
        if nms is None:
            return logits, box, ref, counts
        unit_off, seg, iou = nms
        dev = logits.device
        G = len(seg) - 1
        uo = _h2d(unit_off, dev, tag="nms_unit_off")
        sg = _h2d(seg, dev, tag="nms_seg")
        out_l = torch.empty((G * NMS_SMALL, 2), device=dev, dtype=torch.float32)
        out_b = torch.empty((G * NMS_SMALL, 4), device=dev, dtype=torch.float32)
        out_r = torch.empty((G * NMS_SMALL, 2), device=dev, dtype=torch.float32)
        kept = torch.empty(G, device=dev, dtype=torch.int32)
        call("tmr_nms_small", ptr(logits), ptr(box), ptr(ref), ptr(counts), ptr(uo), ptr(sg), G, float(iou),
             ptr(out_l), ptr(out_b), ptr(out_r), None, ptr(kept), stream())
        return logits, box, ref, counts, torch.cat([counts, kept]), out_l, out_b, out_r

    def _detect_refined(self, feats, unit_image, boxes, params, shape, iou_threshold, refiner, image,
                        sam_features, refine_exemplars):
        """detect() with a box refiner: the eager route up to the candidates
        (no speculative NMS), the per-image lists in exemplar order (an empty
        unit contributes its dummy row, as Get_pred_boxes), the refiner, then
        the package's NMS."""
        from .tm_utils import NMS

        if image is None or sam_features is None:
            raise TMRError("detect(refiner=...) needs image and sam_features")
        B, E, cap = shape
        self.last_graph, self.last_nms_small = "eager", False
        if self.box_at_peaks_ok():
            logits, box, ref, _, counts_host = self._detect_box_at_peaks(feats, unit_image, boxes, params)
        else:
            self.last_box_route = None
            logits, box, ref, counts = self._forward_peaks(feats, unit_image, boxes, params)
            counts_host = counts.cpu().numpy()  # torch.where-style sync (TM_utils.py:254)
        rows = np.maximum(counts_host, 1)  # (row 0 of an empty unit holds the dummy row)
        L, Bx, R = [], [], []
        for i in range(B):
            us = range(i * E, (i + 1) * E)
            L.append(torch.cat([logits[u * cap:u * cap + int(rows[u])] for u in us]))
            Bx.append(torch.cat([box[u * cap:u * cap + int(rows[u])] for u in us]))
            R.append(torch.cat([ref[u * cap:u * cap + int(rows[u])] for u in us]))
        if refine_exemplars is not None:
            L, Bx, R = refiner.forward_refine(L, Bx, R, image, refine_exemplars, sam_features)
        else:
            L, Bx, R = refiner(L, Bx, R, image, sam_features)
        return NMS(L, Bx, R, iou_threshold)

    def detect(self, feats: torch.Tensor, exemplars, cls_ths: float, iou_threshold: float,
               ablation_b: bool = False, ablation_c: bool = False, refiner=None, image=None,
               sam_features=None, refine_exemplars=None):
        """The reference's multi-exemplar inference (demo.py:106-130,
        trainer.py:95-118) for a batch: per image, one forward per exemplar,
        Get_pred_boxes, concat in exemplar order, one NMS.

        exemplars: [B,E,4] normalised xyxy (array or tensor).
        refiner (a SAM_box_refiner): the --refine_box order of
        trainer.py:106-118: the candidates of every exemplar, concatenated
        per image, go through refiner.forward(.., image, sam_features) (or
        forward_refine with refine_exemplars) before the NMS; image [B,3,h,w]
        and sam_features (per image [C,he,we]) are the refiner's inputs.
        Returns per-image lists (logits [k,2], boxes [k,4], refs [k,2])."""
        ex = exemplars.detach().cpu().numpy() if isinstance(exemplars, torch.Tensor) else \
            np.asarray(exemplars)
        ex = ex.astype(np.float32)
        B, E = ex.shape[:2]
        unit_image = np.repeat(np.arange(B), E)
        boxes = ex.reshape(B * E, 4)
        require_gpu(feats, "features")
        Hin, Win = feats.shape[-2:]
        H, W = (2 * Hin, 2 * Win) if self.cfg.feature_upsample else (Hin, Win)
        params = host.peak_params(boxes, H, W, cls_ths, self.cfg.box_reg, ablation_b, ablation_c)
        C = int(self.P["input_proj.0.weight"].shape[0])
        U = B * E
        unit_off = np.arange(U, dtype=np.int64) * (H * W)
        seg = np.arange(0, U + 1, E, dtype=np.int64)
        if refiner is not None:
            return self._detect_refined(feats, unit_image, boxes, params, (B, E, H * W), iou_threshold, refiner,
                                        image, sam_features, refine_exemplars)
        if not (self.use_graphs and U <= self.GRAPH_MAX_UNITS):
            # the unspeculated eager route (no graph prep at all): the
            # regression only at the peaks where that applies
            self.last_graph, self.last_nms_small = "eager", False
            if self.box_at_peaks_ok():
                logits, box, ref, counts, counts_host = self._detect_box_at_peaks(feats, unit_image, boxes, params)
            else:
                self.last_box_route = None
                logits, box, ref, counts = self._forward_peaks(feats, unit_image, boxes, params)
                counts_host = counts.cpu().numpy()  # torch.where-style sync (TM_utils.py:254)
            return self.nms(logits, box, ref, counts, counts_host, unit_off, seg, iou_threshold)
        # small batches also run the device-sized small NMS in the same
        # forward (tmr_nms_small): one sync instead of two when every image's
        # union fits NMS_SMALL rows (else tmr_nms after the sync)
        spec = (unit_off, seg.astype(np.int32), iou_threshold)
        units = host.build_units(boxes, unit_image, H, W, C, self.cfg.template_type)[0] \
            if not self.cfg.no_matcher else np.zeros(0, UNIT_DTYPE)
        sig = self._graph_signature(feats, units, unit_image, ablation_b, ablation_c)
        if sig is not None:
            sig = sig + (float(iou_threshold),)  # a kernel argument of the captured NMS
        g = self._graphs.get(sig) if sig is not None else None
        self.last_graph = "replay" if g is not None else "eager"
        if g is None and sig is not None and self._graphs.want_capture(sig):
            g = graphs.capture(self, feats, self._detect_host_inputs(units, unit_image, B, params, spec),
                               lambda static: self._forward_peaks(static, unit_image, boxes, params, spec))
            self._graphs.put(sig, g)
            if g is not None:
                self.last_graph = "captured"
        if g is not None:
            out = g.replay(self, feats.float().contiguous(), self._detect_host_inputs(units, unit_image, B, params, spec))
        else:
            self.last_box_route = None
            out = self._forward_peaks(feats, unit_image, boxes, params, spec)
        logits, box, ref, counts = out[:4]
        ck = out[4].cpu().numpy()  # torch.where-style sync (TM_utils.py:254): counts + kept
        counts_host, kept = ck[:U], ck[U:]
        self.last_nms_small = bool((kept >= 0).all())
        if not self.last_nms_small:
            return self.nms(logits, box, ref, counts, counts_host, unit_off, seg, iou_threshold)
        # graph outputs are the graph's static buffers: copied out
        ol, ob, orf = (t.clone() for t in out[5:8]) if g is not None else out[5:8]
        s0 = [int(i) * NMS_SMALL for i in range(B)]
        return ([ol[a:a + int(k)] for a, k in zip(s0, kept)], [ob[a:a + int(k)] for a, k in zip(s0, kept)],
                [orf[a:a + int(k)] for a, k in zip(s0, kept)])
