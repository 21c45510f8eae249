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

import gc
import json
import os
import threading
import weakref
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import exp_table, host
from ._lib import (PEAKS_DECODE_ONLY, PEAKS_FIND_ONLY, PEAKS_PROB_SCRATCH, POINTS_TILE, PREC_CODES, SPLIT_INIT_BCAST, SPLIT_INIT_BF16, SPLIT_OUT_BF16,
                   SPLIT_TILED_INIT, SPLIT_TILED_OUT, SPLIT_UNITS_PER_IMAGE_SHIFT, SPLIT_XMAX_PER_PIXEL,
                   SPLIT_XMAX_PER_UNIT, SIZE_KINDS, XPACK_ONES, XPACK_UPSAMPLE,
                   UNIT_DTYPE, XCORR_ALGOS, TMRError, call, load, ptr,
                   require_gpu, size, split_tile_window, stream, xcorr)

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


# Correlation-kernel crossover (tmr_xcorr_args_t.algo).  Since round 3 the table is
# the committed rocprofv3 sweep (xcorr_cost.json, below): kernel-trace
# durations of both kernels per k in the two regimes, beside each point's
# counted HBM bytes and MFMA busy (profiles/xcorr_crossover.json; DESIGN.md
# 4.3), re-swept whenever xcorr.hip changes (its source digest is recorded and
# tests/test_abi_host.py fails on a stale one).  The constants here are the
# round-2 HIP-event tables it replaced (kbench_xcorr,
# profiles/archive/r02w_sweep{128,192}.jsonl), as ms per unit at the 512 x
# 128^2 map size, in two exemplar-count regimes: E = 3 (64 images x 3
# exemplars at 128^2; the image's band staging is shared by 3 units) and
# E = 16 (8 images x 16 exemplars at 192^2, times / 2.25 for the area).
# "auto" interpolates the regimes in log E, sums the per-unit costs of a
# launch (linear in k in between) and runs the cheaper kernel.  Round-6
# sweep (2-D window MFMA kernel): fp32 MFMA wins from k = 7 in both regimes;
# one bf16 term from k = 5 at E = 3 and at every k at E = 16.
XCORR_COST_K = (1, 3, 5, 7, 9, 11, 13, 15, 17, 19, 21, 23, 25, 27, 29, 31)
_T128 = {  # ms per 192 units (E = 3), r02w sweep (aligned A fragments)
    "valu": (1.720, 1.849, 2.498, 3.174, 4.051, 5.281, 6.538, 8.069, 10.139, 12.159, 14.558, 16.630, 20.469, 23.479, 26.392, 29.846),
    "mfma": (1.962, 2.577, 3.189, 3.755, 4.350, 4.796, 5.407, 5.987, 6.666, 10.969, 12.070, 13.200, 14.328, 15.542, 16.785, 17.876),
    # one bf16 term (tmr_xcorr prec, the bf16 contract), r02af sweep (A prefetch 4 rows)
    "mfma1": (1.875, 2.267, 2.280, 2.634, 2.972, 3.237, 3.465, 3.740, 4.002, 6.008, 6.330, 6.924, 7.386, 7.826, 8.118, 8.554),
}
_K192 = (3, 9, 15, 21, 31)
_T192 = {  # ms per 128 units (E = 16) at 192^2, r02w sweep
    "valu": (2.539, 6.081, 13.025, 22.462, 51.697),
    "mfma": (3.192, 5.520, 7.462, 15.101, 22.257),
    "mfma1": (2.919, 3.890, 4.632, 7.261, 9.791),
}
XCORR_COST = {
    a: (np.asarray(_T128[a]) / 192.0,
        np.interp(XCORR_COST_K, _K192, np.asarray(_T192[a]) / 128.0 / 2.25))
    for a in ("valu", "mfma", "mfma1")
}
XCORR_COST_SOURCE = "engine.py tables (HIP events, profiles/archive/r02w_*, r02af_*)"
# The committed rocprofv3 sweep (profiles/gpu_xcorr_sweep.sh ->
# profiles/xcorr_sweep_assemble.py -> xcorr_cost.json: kernel-trace launch
# durations of both kernels per k and regime, recorded beside their FETCH /
# WRITE bytes and MFMA-busy counters in profiles/xcorr_crossover.json)
# replaces the tables above when present.
_COST_JSON = os.path.join(os.path.dirname(os.path.abspath(__file__)), "xcorr_cost.json")


def _load_xcorr_cost(path: str = _COST_JSON):
    """The rocprof-swept per-k cost table (xcorr_cost.json).  Missing file:
    None (the built-in tables above apply).  A file that exists but does not
    parse raises: a silently moved crossover would change which
    kernel runs."""
    if not os.path.exists(path):
        return None
    try:
        with open(path) as fh:
            d = json.load(fh)
    except ValueError as err:
        raise TMRError(f"{path}: malformed correlation cost table ({err})") from err
    reg = d.get("regimes", {})

    def per_unit(name, algo, area):
        r = reg[name]
        ks, ms = zip(*sorted((int(k), float(v)) for k, v in r["ms"][algo] if v is not None))
        return np.interp(XCORR_COST_K, ks, np.asarray(ms) / (r["images"] * r["E"]) / area)

    try:
        table = {
            "valu": (per_unit("r128_e3_fp32", "valu", 1.0), per_unit("r192_e16_fp32", "valu", 2.25)),
            "mfma": (per_unit("r128_e3_fp32", "mfma", 1.0), per_unit("r192_e16_fp32", "mfma", 2.25)),
            "mfma1": (per_unit("r128_e3_bf16", "mfma", 1.0), per_unit("r192_e16_bf16", "mfma", 2.25)),
        }
    except (KeyError, ValueError, TypeError) as err:
        raise TMRError(f"{path}: correlation cost table lacks a regime or algorithm ({err!r})") from err
    return table, d.get("source", path)


_swept = _load_xcorr_cost()
if _swept is not None:
    XCORR_COST, XCORR_COST_SOURCE = _swept
# A mixed-size MFMA launch stages every band with the LARGEST template's halo
# rows (and that template's band height), and its band staging is shared by
# fewer units when an image has few of them.  Rounds 2-5 (row-Toeplitz
# kernel): 1.10-1.13x the per-k sum at the config-B 3..15 mix (profiles/
# archive/r02w_mixB.jsonl).  Round 6 (2-D window kernel, rolling band rows):
# 1.04x (3.764 ms mix vs 3.619 ms per-k mean, one run on one box,
# profiles/r06_xcorr_rolling).
# Empirical: 1 + MIX / units-per-image.
XCORR_MFMA_MIX = 0.12


def xcorr_choice(ht: np.ndarray, wt: np.ndarray, units_per_image: float, mfma_ok: bool,
                 one_term: bool = False) -> str:
    """The cheaper correlation kernel ("valu" or "mfma") for a launch over
    units of these template sizes (XCORR_COST model); one_term: the MFMA
    kernel runs one 16-bit term (bf16 contract) instead of the 3-term split."""
    if not mfma_ok:
        return "valu"
    k = np.maximum(np.asarray(ht), np.asarray(wt)).astype(np.float64)
    lam = float(np.clip(np.log(max(units_per_image, 1.0) / 3.0) / np.log(16.0 / 3.0), 0.0, 1.0))
    cost = {}
    for alg, table in (("valu", "valu"), ("mfma", "mfma1" if one_term else "mfma")):
        c3, c16 = XCORR_COST[table]
        per_k = (1.0 - lam) * c3 + lam * c16
        cost[alg] = float(np.interp(k, XCORR_COST_K, per_k).sum())
    if k.size and k.min() != k.max():
        cost["mfma"] *= 1.0 + XCORR_MFMA_MIX / max(units_per_image, 1.0)
    return min(cost, key=cost.get)


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


def absmax(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """max |x| as a 1-element device tensor (max(out, |x|) when out is given):
    tmr_absmax_rows over one row."""
    require_gpu(x, "absmax input")
    if x.dtype != torch.float32:
        raise TMRError(f"absmax of a {x.dtype} tensor (fp32 only)")
    x = x.contiguous()
    acc = out is not None
    if out is None:
        out = torch.empty(1, device=x.device, dtype=torch.float32)
    call("tmr_absmax_rows", ptr(x), 1, x.numel(), int(acc), ptr(out), stream())
    return out


def absmax_rows(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Per-sample max |x[s]| of x [S, ...] as an [S] device tensor (max(out, .)
    when out is given): the per-sample activation scale source of the split
    kernels (tmr_absmax_rows)."""
    require_gpu(x, "absmax input")
    if x.dtype != torch.float32:
        raise TMRError(f"absmax of a {x.dtype} tensor (fp32 only)")
    x = x.contiguous()
    S = x.shape[0]
    acc = out is not None
    if out is None:
        out = torch.empty(S, device=x.device, dtype=torch.float32)
    elif out.numel() != S:
        raise TMRError(f"absmax_rows: out holds {out.numel()} values for {S} samples")
    call("tmr_absmax_rows", ptr(x), S, x.numel() // max(S, 1), int(acc), ptr(out), stream())
    return out


def scale_merge(img_max: Optional[torch.Tensor], unit_max: torch.Tensor, unit_image: torch.Tensor, B: int):
    """(per-image, per-unit) scale sources of a launch whose tiles read an
    image's src0 records and its units' src1 records with ONE scale:
    img[b] = max(img_max[b], unit_max[u] for u of image b), unit[u] =
    img[unit_image[u]] (tmr_scale_merge)."""
    U = unit_max.numel()
    out_img = torch.empty(B, device=unit_max.device, dtype=torch.float32)
    out_unit = torch.empty(U, device=unit_max.device, dtype=torch.float32)
    call("tmr_scale_merge", ptr(img_max) if img_max is not None else None, ptr(unit_max), ptr(unit_image),
         B, U, ptr(out_img), ptr(out_unit), stream())
    return out_img, out_unit


def pixel_absmax(x: torch.Tensor) -> torch.Tensor:
    """max_c |x[s, c, y, x]| as [S, H, W] (tmr_pixel_absmax): the per-pixel
    scale source of a 1x1 conv (TMR_SPLIT_XMAX_PER_PIXEL)."""
    require_gpu(x, "absmax input")
    x = x.float().contiguous()
    S, C, H, W = x.shape
    out = torch.empty((S, H, W), device=x.device, dtype=torch.float32)
    call("tmr_pixel_absmax", ptr(x), S, C, H * W, ptr(out), stream())
    return out


def _per_sample(xmax: Optional[torch.Tensor], S: int) -> int:
    """The xmax_per_sample mode of the record packs: 0 for one shared scale
    source, 1 for one per sample ([S]), 2 for one per pixel ([S, H, W])."""
    if xmax is None or xmax.numel() == 1:
        return 0
    if xmax.dim() == 3:
        if xmax.shape[0] != S:
            raise TMRError(f"per-pixel scale sources for {xmax.shape[0]} samples, not {S}")
        return 2
    if xmax.numel() != S:
        raise TMRError(f"scale source holds {xmax.numel()} values for {S} samples")
    return 1


def prec_code(precision: str) -> int:
    if precision not in PREC_CODES:
        raise TMRError(f"precision must be one of {sorted(PREC_CODES)}, got {precision!r}")
    return PREC_CODES[precision]


def pack_split_w(w: torch.Tensor, c0: int, precision: str):
    """[N,C0+C1,ks,ks] fp32 -> (16-bit packed weights, max|w|) for the split
    conv kernel (include/tmr.h tmr_split_wpack)."""
    require_gpu(w, "conv weight")
    w = w.detach().float().contiguous()
    N, C, ks, ks2 = w.shape
    if ks != ks2:
        raise TMRError("square kernels only (regression_head.py:7)")
    pc = prec_code(precision)
    n = load().tmr_size(SIZE_KINDS["wpack"], N, c0, C - c0, ks, pc, 0)
    if n <= 0:
        raise TMRError(f"unsupported conv shape {tuple(w.shape)}")
    wmax = absmax(w)
    out = torch.empty(n, device=w.device, dtype=torch.uint8)
    call("tmr_split_wpack", ptr(w), N, c0, C - c0, ks, pc, ptr(wmax), ptr(out), stream())
    return out, wmax


def pack_split_x(x: torch.Tensor, ks: int, precision: str, xmax: torch.Tensor) -> torch.Tensor:
    """[S,C,H,W] fp32 -> zero-padded 16-bit records (tmr_split_xpack); a bf16
    x (the correlation's bf16 f_TM plane, tmr_xcorr out_bf16) under the bf16
    contract -> the same records (tmr_split_xpack16).  xmax: one scale source,
    or [S] (one per sample)."""
    require_gpu(x, "conv input")
    S, C, H, W = x.shape
    pc = prec_code(precision)
    n = load().tmr_size(SIZE_KINDS["xpack"], S, C, H, W, ks, pc, 0)
    if n <= 0:
        raise TMRError(f"unsupported conv input {tuple(x.shape)}")
    out = torch.empty(n, device=x.device, dtype=torch.uint8)
    if x.dtype == torch.bfloat16:
        x = x.contiguous()
        call("tmr_split_xpack16", ptr(x), S, C, H, W, ks, pc, ptr(out), stream())
        return out
    x = x.float().contiguous()
    call("tmr_split_xpack", ptr(x), S, C, H, W, 0, ks, pc, ptr(xmax), _per_sample(xmax, S), ptr(out), stream())
    return out


def fold_proj(w: torch.Tensor, cp: int, proj_w: torch.Tensor, proj_b: torch.Tensor) -> torch.Tensor:
    """Fold the first cp input channels of w [N,Cw,k,k] through the 1x1
    input_proj (proj_w [cp,Cin,1,1], proj_b [cp]) -> [N, Cin+1, k, k]
    (tmr_split_fold_proj; the last channel multiplies a constant-1 plane)."""
    require_gpu(w, "conv weight")
    w = w.detach().float().contiguous()
    N, Cw, k, _ = w.shape
    pw = proj_w.detach().float().reshape(cp, -1).contiguous()
    pb = proj_b.detach().float().contiguous()
    cin = pw.shape[1]
    out = torch.empty((N, cin + 1, k, k), device=w.device, dtype=torch.float32)
    call("tmr_split_fold_proj", ptr(w), N, Cw, cp, k, ptr(pw), ptr(pb), cin, ptr(out), stream())
    return out


def pack_split_up(f: torch.Tensor, upsample: bool, ks: int, precision: str,
                  xmax: torch.Tensor, ones: bool = True) -> torch.Tensor:
    """SAM features [S,Cin,h,w] -> records of [up2x(f) or f; 1] (tmr_split_xpack
    with TMR_XPACK_UPSAMPLE / TMR_XPACK_ONES; without the constant-1 channel
    when ones=False)."""
    require_gpu(f, "features")
    f = f.float().contiguous()
    S, Cin, Hin, Win = f.shape
    H, W = (2 * Hin, 2 * Win) if upsample else (Hin, Win)
    pc = prec_code(precision)
    n = load().tmr_size(SIZE_KINDS["xpack"], S, Cin + int(ones), H, W, ks, pc, 0)
    if n <= 0:
        raise TMRError(f"unsupported feature shape {tuple(f.shape)}")
    out = torch.empty(n, device=f.device, dtype=torch.uint8)
    up = (XPACK_UPSAMPLE if upsample else 0) | (XPACK_ONES if ones else 0)
    call("tmr_split_xpack", ptr(f), S, Cin, Hin, Win, up, ks, pc, ptr(xmax), _per_sample(xmax, S), ptr(out), stream())
    return out


def conv2d_split(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor, leaky: bool,
                 precision: str = "fp32", packed=None):
    """nn.Conv2d(padding=(k-1)//2) [+ LeakyReLU(0.01)] on the split 16-bit
    MFMA kernel (precision "fp32" keeps the 1e-5 contract).  One activation
    scale per SAMPLE (per PIXEL for a 1x1 conv, whose output columns are
    pixels): each sample's result is that of a batch of one."""
    require_gpu(x, "conv input")
    x = x.float().contiguous()
    U, C, H, W = x.shape
    N, Cw, ks, _ = w.shape
    if Cw != C:
        raise TMRError(f"conv expects {Cw} input channels, got {C}")
    wp, wmax = packed if packed is not None else pack_split_w(w, C, precision)
    pix = ks == 1
    xmax = pixel_absmax(x) if pix else absmax_rows(x)
    xp = pack_split_x(x, ks, precision, xmax)
    out = torch.empty((U, N, H, W), device=x.device, dtype=torch.float32)
    call("tmr_split_conv", ptr(xp), C, None, None, 0, U, H, W, ks, prec_code(precision),
         ptr(wp), ptr(wmax), ptr(xmax), ptr(b.detach().float().contiguous()), N, int(leaky), None, None,
         ptr(out), SPLIT_XMAX_PER_PIXEL if pix else SPLIT_XMAX_PER_UNIT, stream())
    return out


# graph capture of TMREngine.detect's forward (_DetectGraph): while set, every
# tagged host input staged by _h2d is a view of the capture's _HostBlob
_capture = threading.local()


class _HostBlob:
    """The tagged host inputs of a captured forward in ONE pinned buffer and
    ONE device buffer: the capture's first node copies the pinned bytes up,
    every tagged _h2d inside the capture is a view of the device buffer, and a
    replay only rewrites the pinned bytes -- one copy node per forward instead
    of one per input (each is a ~5 us blit on the GPU's timeline)."""

    def __init__(self, host_in: Dict[str, np.ndarray], device):
        self.offs: Dict[str, tuple] = {}
        o = 0
        for t, a in host_in.items():
            if a.nbytes:
                self.offs[t] = (o, a.nbytes)
                o += (a.nbytes + 15) // 16 * 16  # 16-B aligned sections
        self.pinned = torch.empty(max(o, 16), dtype=torch.uint8).pin_memory()
        self.dev = torch.empty(max(o, 16), dtype=torch.uint8, device=device)
        self.fill(host_in)

    def fill(self, host: Dict[str, np.ndarray]):
        pn = self.pinned.numpy()
        for t, a in host.items():
            if t in self.offs:
                o, n = self.offs[t]
                pn[o:o + n] = np.ascontiguousarray(a).reshape(-1).view(np.uint8)

    def upload(self):  # inside the capture, before anything reads the inputs
        self.dev.copy_(self.pinned, non_blocking=True)

    def view(self, tag: Optional[str], t: torch.Tensor) -> torch.Tensor:
        o, n = self.offs.get(tag, (0, -1)) if tag is not None else (0, -1)
        if n != t.numel() * t.element_size():
            raise TMRError(f"host input {tag!r} inside a graph capture has no pre-allocated slot")
        pn = self.pinned.numpy()
        pn[o:o + n] = t.numpy().reshape(-1).view(np.uint8)  # (the capture's own values)
        return self.dev[o:o + n].view(t.dtype).reshape(t.shape)


def _h2d(arr: np.ndarray, device, dtype=None, tag: Optional[str] = None) -> torch.Tensor:
    """A small host array on the device WITHOUT a stream sync: staged through
    torch's caching pinned-memory allocator and copied non_blocking (the
    allocator keeps the pinned block until the copy's stream event has
    completed).  A pageable `.to(device)` synchronises the stream, leaving the
    GPU idle while the host prepares the next launches.  Inside a graph
    capture a tagged input is a view of the capture's _HostBlob (the replay
    rewrites its pinned bytes)."""
    t = torch.from_numpy(np.ascontiguousarray(arr))
    if dtype is not None:
        t = t.to(dtype)
    device = torch.device(device)
    if device.type != "cuda":
        return t.to(device)
    blob = getattr(_capture, "blob", None)
    if blob is None:
        return t.pin_memory().to(device, non_blocking=True)
    return blob.view(tag, t)


def _units_to_device(units: np.ndarray, device, tag: Optional[str] = None) -> torch.Tensor:
    return _h2d(units.view(np.uint8), device, tag=tag)


def _clone_outputs(out: Dict[str, object], keep=("fp",)) -> Dict[str, object]:
    """Fresh copies of a replayed graph's static outputs (a caller may keep
    one call's maps while the next replay runs): tensors that are contiguous
    views of one storage (o and b) are copied out by ONE copy of the range
    they cover; names in `keep` are returned as they are."""
    res, groups = {}, {}
    for k, v in out.items():
        if isinstance(v, torch.Tensor) and k not in keep:
            groups.setdefault(v.untyped_storage().data_ptr(), []).append(k)
        else:
            res[k] = v
    for ks in groups.values():
        ts = [out[k] for k in ks]
        if len(ks) == 1 or not all(t.is_contiguous() for t in ts):
            res.update({k: out[k].clone() for k in ks})
            continue
        lo = min(t.storage_offset() for t in ts)
        hi = max(t.storage_offset() + t.numel() for t in ts)
        base = ts[0].as_strided((hi - lo,), (1,), lo).clone()
        for k, t in zip(ks, ts):
            res[k] = base.as_strided(t.shape, t.stride(), t.storage_offset() - lo)
    return res


class _GraphBook:
    """Which launch signatures have a captured graph, how often the others
    were seen, and which failed to capture.  A signature is
    captured on its second sighting; the seen-counts are an LRU bounded by
    `seen_cap` (mapper workloads with varied exemplar sizes make a new
    signature almost every batch), graphs an LRU of `cap`, and a signature
    whose capture failed stays eager (bounded too) instead of retrying the
    sync + clone + capture on every call.  Host-only: tested on CPU."""

    FAILED = object()

    def __init__(self, cap: int, seen_cap: int = 256):
        from collections import OrderedDict
        self.cap, self.seen_cap = cap, seen_cap
        self.graphs: "OrderedDict[tuple, object]" = OrderedDict()
        self.seen: "OrderedDict[tuple, int]" = OrderedDict()
        self.failed: "OrderedDict[tuple, None]" = OrderedDict()

    def get(self, sig):
        g = self.graphs.get(sig)
        if g is not None:
            self.graphs.move_to_end(sig)
        return g

    def want_capture(self, sig) -> bool:
        """Count a sighting of sig (no graph yet); True when it should be
        captured now (second sighting, never failed)."""
        if sig in self.failed:
            return False
        n = self.seen.pop(sig, 0) + 1
        self.seen[sig] = n
        while len(self.seen) > self.seen_cap:
            self.seen.popitem(last=False)
        return n >= 2

    def put(self, sig, g):
        self.seen.pop(sig, None)
        if g is None:
            self.failed[sig] = None
            while len(self.failed) > self.seen_cap:
                self.failed.popitem(last=False)
            return
        self.graphs[sig] = g
        while len(self.graphs) > self.cap:
            self.graphs.popitem(last=False)

    def clear(self):
        self.graphs.clear(); self.seen.clear(); self.failed.clear()


class _DetectGraph:
    """One captured detect forward (projection ... peaks) for a fixed launch
    signature: the inputs are a static feature buffer and the pinned host
    blob of its tagged host inputs; the outputs the forward's static
    buffers.  A replay refills both and launches the whole forward at once."""

    def __init__(self, graph, feats, blob, outputs, last):
        self.graph, self.feats, self.blob, self.outputs, self.last = graph, feats, blob, outputs, last
        self.done = None  # event after the last replay: its copy node reads the pinned blob
        self.src = None  # (tensor ref, version, data_ptr) of the features last copied into feats

    def replay(self, feats: torch.Tensor, host: Dict[str, np.ndarray], reuse_feats: bool = False):
        """reuse_feats (the module API's later exemplar calls on one image,
        where reusing the image is the intent): skip the feature copy when
        the same tensor object at the same version was copied last.  detect()
        always copies: writes through a raw pointer or a caller's
        own graph replay change a tensor without bumping its version."""
        # the blob is rewritten by the host at once: a previous replay still
        # queued (two calls with no sync between them) must have read it first
        if self.done is not None:
            self.done.synchronize()
        self.blob.fill(host)
        src = self.src
        if not reuse_feats or src is None or src[0]() is not feats or \
                src[1] != (feats._version, feats.data_ptr()):
            self.feats.copy_(feats)
            self.src = (weakref.ref(feats), (feats._version, feats.data_ptr()))
        self.graph.replay()
        if self.done is None:
            self.done = torch.cuda.Event()
        self.done.record()
        return self.outputs


# the heads launch's image-major block order (an image's units innermost) for
# up to this many units per image: config B (3 per image) 106.6 -> 106.0 ms
# (profiles/archive/r05/r05c), config E (16 per image) 166.6 -> 168.5 ms (profiles/archive/r05/r05t).
# A/B knob TMR_HEADS_IMAGE_MAJOR_MAX (the flags field holds <= 255)
HEADS_IMAGE_MAJOR_MAX = min(255, int(os.environ.get("TMR_HEADS_IMAGE_MAJOR_MAX", "4")))


class _no_gc:
    """Python's cyclic GC off for the length of a graph capture: a collection
    inside the capture can destroy an unreachable object that owns a HIP
    event or graph (an evicted replay's), and a destroy call during a global
    capture aborts the process (seen once in test_module_graph_replays_back_to_back,
    profiles/archive/r05/r05aa).  torch.cuda.graph collects on entry; this keeps it off
    until the capture has ended."""

    def __enter__(self):
        self.was = gc.isenabled()
        gc.collect()
        gc.disable()

    def __exit__(self, *exc):
        if self.was:
            gc.enable()
        return False


class TMREngine:
    """Native forward + post-processing over (image, exemplar) units."""

    def __init__(self, params: Dict[str, torch.Tensor], cfg: PathConfig):
        self.P = params
        self.cfg = cfg
        self._cache = _PackCache()
        # when a list, decode() appends (start, end) torch.cuda.Events recorded
        # on the launch stream around the fused decoder kernel (bench.py)
        self.decoder_events = None
        self.xcorr_events = None
        self.xcorr_split_events = []  # (start, end) of each timed launch's tmr_template_split
        self.last_xcorr_flops = 0.0
        self.last_xcorr_bytes = 0.0
        self.last_xcorr_dram_bytes = 0.0
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
        # correlation kernel: "auto" (the crossover rule, XCORR_COST), "valu" or
        # "mfma" (csrc/xcorr.hip).  (Round 5's per-unit split of a mixed launch
        # over two streams, its in-kernel A fragments and its bf16 record output
        # were measured, not kept and removed in round 6: DESIGN_HISTORY.md.)
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
        self._fp_memo = None
        self._acc0_memo = None
        self._graphs = _GraphBook(self.GRAPH_CACHE)
        self._pnames = None
        self.last_graph = None
        self.last_graph_error = None
        self.last_decoder_flops = 0.0
        self.last_shared_flops = 0.0
        self.last_decoder_algo = None
        # detect()'s regression route of the last call ("points" / "dense";
        # None: the fused dense launch), its candidates and the points
        # launch's direct conv FLOPs (whole tiles of POINTS_TILE points)
        self.last_box_route = None
        self.last_points = 0
        self.last_points_flops = 0.0
        self._box_ctx = None
        if cfg.decoder_kernel_size not in (1, 3, 5, 7):
            raise TMRError("decoder_kernel_size must be 1, 3, 5 or 7")

    # ------------------------------------------------------------ weights
    def _dec_layers(self, pre: str):
        out = []
        for l in range(self.cfg.decoder_num_layer):
            out.append((self.P[f"{pre}.layer.{2 * l}.weight"], self.P[f"{pre}.layer.{2 * l}.bias"]))
        return out

    def _fused_decoders(self, split_c0: int = 0, fold: bool = False):
        """Layer-0 weights of decoder_b and decoder_o concatenated along N, with
        the 1x1 heads as a [Npad,5] epilogue matrix (only for 1-layer decoders).
        split_c0 > 0 additionally packs the input-channel halves [:c0] / [c0:]
        (conv(cat[fp, f_TM]) = conv_fp(fp) + conv_tm(f_TM)).  fold (split
        kernel, fusion) replaces the fp half by its fold through input_proj:
        conv_fp(proj(x)) = conv'([x; 1]) (tmr_split_fold_proj), Cin+1 channels."""
        cfg = self.cfg
        layers = ([self._dec_layers("decoder_b")[0]] if cfg.box_reg else []) + \
            [self._dec_layers("decoder_o")[0]]
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
            c0_full = cfg.emb_dim if cfg.fusion else 0
            prec = cfg.precision
            pk = lambda w_, c0: pack_split_w(w_, c0, prec)  # noqa: E731
            split = None
            if fold:
                # fp half folded through input_proj: [N, Cin+1, k, k]; the
                # constant-1 channel's conv is a fixed plane per map size
                # (_bias_plane), so the GEMM runs on the Cin channels only
                Wf = fold_proj(W, c0_full, pw_, pb_)
                cf = Wf.shape[1] - 1
                wbias = Wf[:, cf:].contiguous()
                Wf = Wf[:, :cf].contiguous()
                if split_c0:
                    split = (pk(Wf, cf), pk(W[:, c0_full:].contiguous(), 0),
                             torch.zeros(N, device=W.device, dtype=torch.float32))
                    full = None
                else:
                    full = pk(torch.cat([Wf, W[:, c0_full:]], 1).contiguous(), cf)
                return full, Bv, N, W.shape[1], hw.contiguous(), hb.contiguous(), split, wbias
            if split_c0:
                split = (pk(W[:, :split_c0].contiguous(), split_c0), pk(W[:, split_c0:].contiguous(), 0),
                         torch.zeros(N, device=W.device, dtype=torch.float32))
            full = None if split_c0 else pk(W, c0_full)
            return full, Bv, N, W.shape[1], hw.contiguous(), hb.contiguous(), split, None

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
                 SPLIT_TILED_OUT | (SPLIT_OUT_BF16 if self._plane16() else 0), stream())
            return plane

        return self._cache.get(f"bias_plane_{H}x{W}_{prec}", [wbias], build)

    def _plane16(self) -> bool:
        """The bias plane slab is kept in bf16 under the bf16 contract (its
        broadcast read is the fp-half store's initial-value burst: 9% of that
        launch in fp32, r02am)."""
        return self.cfg.precision == "bf16"

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

    def _memo_absmax(self, t: torch.Tensor, tag: str, compute=None):
        """Device max scalars memoised per tensor OBJECT and version (a freed
        tensor's address reused by another never hits)."""
        key = (t.data_ptr(), tag)
        hit = self._absmax_memo.get(key)
        if hit is not None and hit[0]() is t and hit[1] == t._version:
            return hit[2]
        if compute is None:
            return None
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
        Hq, Wq = Hin, Win
        n = size("xpack", B, Cin, Hq, Wq, 1, pcode)
        xp = torch.empty(n, device=feats.device, dtype=torch.uint8)
        call("tmr_split_xpack", ptr(feats), B, Cin, Hin, Win, 0, 1, pcode,
             ptr(xmax), _per_sample(xmax, B), ptr(xp), stream())
        fq = torch.empty((B, N, Hq, Wq), device=feats.device, dtype=torch.float32)
        call("tmr_split_conv", ptr(xp), Cin, None, None, 0, B, Hq, Wq, 1, pcode, ptr(wp),
             ptr(wmax), ptr(xmax), ptr(pb.detach().float().contiguous()), N, 0, None, None, ptr(fq),
             SPLIT_XMAX_PER_PIXEL if xmax is not None else 0, stream())
        if up:
            fp = torch.empty((B, N, H, W), device=feats.device, dtype=torch.float32)
            call("tmr_upsample2x", ptr(fq), B * N, Hin, Win, ptr(fp), stream())
        else:
            fp = fq
        f0 = None
        if want_f0:
            if up:
                f0 = torch.empty((B, Cin, H, W), device=feats.device, dtype=torch.float32)
                call("tmr_upsample2x", ptr(feats), B * Cin, Hin, Win, ptr(f0), stream())
            else:
                f0 = feats
        return fp, f0

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
        ev = evs = None
        if self.xcorr_events is not None:  # bench.py: HIP events on the launch stream, around
            # the correlation kernel alone and, separately, its template split
            ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            evs = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        min_k = int(min(units["ht"].min(), units["wt"].min()))
        # MFMA operand precision: the fp32 path's 3-term split, or one bf16 /
        # fp16 term under the bf16 contract (config C); the VALU kernels are fp32
        pc = prec_code(cfg.precision)
        choice = self.xcorr_algo
        if choice == "auto":  # measured per-k cost model (XCORR_COST)
            # (xcorr.hip mfma_fits: a 32-row band, its halo and WIN_OVER = 3 rows staged in registers)
            fits = W % 64 == 0 and W <= 256 and mh <= 31 and mw <= 31 and (35 + mh // 2 * 2) * W <= 16384
            choice = xcorr_choice(units["ht"], units["wt"], U / max(1, len(set(unit_image))), fits,
                                  one_term=pc != PREC_CODES["fp32"])
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
            if evs is not None:
                evs[0].record()
            call("tmr_template_split", ptr(tmpl), ptr(units_d), U, C, rows, pc, ptr(tsplit), stream())
            if evs is not None:
                evs[1].record()
                self.xcorr_split_events.append(evs)
        if ev is not None:
            ev[0].record()
        xcorr(f=ptr(fp), templates=ptr(tmpl), units=ptr(units_d), img_units=ptr(img_units_d), scale=ptr(scale),
              out=ptr(out), relu_out=ptr(relu), work=ptr(work), out_absmax=ptr(slots), tmpl_split=ptr(tsplit),
              total_rows=rows, B=B, C=C, H=H, W=W, U=U, max_ht=mh, max_wt=mw, squeeze=int(cfg.squeeze),
              algo=algo, min_k=min_k, prec=pc, out_bf16=int(out16), stream=stream())
        if ev is not None:
            ev[1].record()
            self.xcorr_events.append(ev)
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
        from the launch's operands kept in self._box_ctx."""
        cfg = self.cfg
        U, C1, H, W = f_tm.shape
        dev = f_tm.device
        C0 = fp.shape[1] if cfg.fusion else 0
        ui = _h2d(np.asarray(unit_image, np.int32), dev, tag="unit_image")
        src0 = fp if cfg.fusion else None
        if cfg.decoder_num_layer == 1:
            B = fp.shape[0]
            # share the fp half of the decoder conv across an image's exemplars
            # when that removes work (U >= 2B): conv_fp once per image, then
            # the per-unit kernel starts from it and runs only the f_TM half
            fold0 = cfg.fusion and self.fold_proj and feats is not None
            # module API (reuse_image_work): the reference's callers run one
            # forward per exemplar on the SAME image features (demo.py:111,
            # trainer.py:96); the image's fp half is then computed once and
            # kept for the next calls (_acc0_memo)
            share = self.share_fp_half and cfg.fusion and (U >= 2 * B or (self.reuse_image_work and fold0))
            # the bf16 contract keeps the per-image fp half (acc0) in bf16:
            # half the heads launch's initial-value read (a chip-wide burst
            # before the first MFMA: 12% of the one-term kernel, r02ah;
            # measured 10.49 -> 10.07 ms per 48 units, r02ak).  Not under
            # "f16" (its 1e-3 contract: b 1.8e-3 with a bf16 acc0, r02ak).
            acc16 = share and cfg.precision == "bf16"
            ks = cfg.decoder_kernel_size
            fold = fold0
            wp, bias, N, Cw, hw, hb, split, wbias = self._fused_decoders(C0 if share else 0, fold)
            if Cw != C0 + C1:
                raise TMRError(f"decoders expect {Cw} input channels, got {C0 + C1}")
            bplane = None
            if fold:  # the fp half runs on up2x(f) (Cin channels) + the bias plane
                C0 = feats.shape[1]
                bplane = self._bias_plane(wbias, H, W)
            nparts = size("heads_partials", N, U, H, W)
            part = torch.empty(nparts, device=dev, dtype=torch.float32)
            acc0 = None
            C0k = C0
            pc = prec_code(cfg.precision)
            # Activation scales are PER SAMPLE (per unit for the f_TM records
            # and the heads launch, per image for the fp half), so a unit's
            # precision never depends on the other units' magnitudes
            # (TMR_SPLIT_XMAX_PER_UNIT); bf16 records are unscaled
            unscaled = cfg.precision == "bf16"
            tm_max = None if unscaled else self._memo_absmax(f_tm, "ftm", lambda: absmax_rows(f_tm))
            if fold:
                # records of up2x(f) (max |.| <= max |f|: bilinear weights are
                # convex), per image
                xmax0 = self._feat_absmax(feats)
                if share:
                    # the fp half is its own launch (tmr_split_conv, tiled out) with
                    # its own per-image scales
                    xmax1 = tm_max
                    acc0 = self._acc0_lookup(feats, split, H, W)
                    xp0 = None if acc0 is not None else \
                        pack_split_up(feats, cfg.feature_upsample, ks, cfg.precision, xmax0, ones=False)
                else:
                    # ONE launch reads both sources of a tile with ONE scale:
                    # per image, max(max|f|, max|f_TM| of its units)
                    xs0, xmax1 = (None, None) if unscaled else scale_merge(xmax0, tm_max, ui, B)
                    xp0 = pack_split_up(feats, cfg.feature_upsample, ks, cfg.precision, xs0, ones=False)
                xp1 = pack_split_x(f_tm, ks, cfg.precision, xmax1)
                C0k = C0
            else:
                if share:
                    xmax0 = None if unscaled else absmax_rows(fp)
                    xp0 = pack_split_x(fp, ks, cfg.precision, xmax0)
                    xmax1 = tm_max
                elif src0 is not None:
                    xs0, xmax1 = (None, None) if unscaled else scale_merge(absmax_rows(fp), tm_max, ui, B)
                    xp0 = pack_split_x(fp, ks, cfg.precision, xs0)
                else:
                    xp0, xmax1 = None, tm_max
                xp1 = pack_split_x(f_tm, ks, cfg.precision, xmax1)
            xpu = 0 if unscaled else SPLIT_XMAX_PER_UNIT
            if share:
                wp_fp, wp_tm, zero_b = split
                if acc0 is None:  # acc0 in the kernel's tiled accumulator layout (private)
                    acc0 = torch.empty(size("acc", B, N, H, W), device=dev, dtype=torch.float32)
                    fl = SPLIT_TILED_OUT | (SPLIT_OUT_BF16 if acc16 else 0) | xpu
                    if bplane is not None:
                        fl |= SPLIT_TILED_INIT | SPLIT_INIT_BCAST | (SPLIT_INIT_BF16 if self._plane16() else 0)
                    call("tmr_split_conv", ptr(xp0), C0, None, None, 0, B, H, W, ks, pc,
                         ptr(wp_fp[0]), ptr(wp_fp[1]), ptr(xmax0), ptr(zero_b), N, 0, None,
                         ptr(bplane) if bplane is not None else None, ptr(acc0), fl, stream())
                    if fold and self.reuse_image_work:
                        self._acc0_store(feats, split, H, W, acc0)
                # else: the image's cached fp half
                wp, src0, C0k = wp_tm, None, 0
            ev = None
            if self.decoder_events is not None:
                ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                ev[0].record()
            a0 = ptr(acc0) if acc0 is not None else None
            fl = (SPLIT_TILED_INIT | (SPLIT_INIT_BF16 if acc16 else 0)) if a0 is not None else 0
            if acc0 is None and bplane is not None:  # unshared folded fp half: its bias plane
                a0 = ptr(bplane)
                fl = SPLIT_TILED_INIT | SPLIT_INIT_BCAST | (SPLIT_INIT_BF16 if self._plane16() else 0)
            fl |= xpu
            epi = self._units_per_image(unit_image, B) << SPLIT_UNITS_PER_IMAGE_SHIFT
            # box_later: decoder_o's tiles only (the window's partials sit where
            # the full launch writes them)
            nbt = self._box_tiles() if box_later else 0
            nt_all = (N + 127) // 128
            win = split_tile_window(nbt, nt_all - nbt) if box_later else 0
            call("tmr_split_conv", ptr(xp0) if C0k else None, C0k, ptr(ui), ptr(xp1), C1,
                 U, H, W, ks, pc, ptr(wp[0]), ptr(wp[1]), ptr(xmax1), ptr(bias), N, 1, ptr(hw),
                 a0, ptr(part), fl | epi | win, stream())
            if ev is not None:
                ev[1].record()
                self.decoder_events.append(ev)
            # direct conv FLOPs of the timed launch's channel tiles (the kernel
            # executes 3 16-bit MFMA terms per product under the fp32 contract)
            n_run = 128 * (nt_all - nbt) if box_later else N
            self.last_decoder_flops = 2.0 * H * W * n_run * (C0k + C1) * ks ** 2 * U
            self.last_shared_flops = 2.0 * H * W * N * C0 * ks ** 2 * B if share else 0.0
            self.last_decoder_algo = "split"
            # o and b as contiguous views of ONE buffer (a graph replay then
            # copies both out with one copy, _clone_outputs)
            ob = torch.empty(U * (5 if cfg.box_reg else 1) * H * W, device=dev, dtype=torch.float32)
            o = ob[:U * H * W].view(U, 1, H, W)
            b = ob[U * H * W:].view(U, 4, H, W) if cfg.box_reg else None
            if box_later:
                call("tmr_heads_reduce", ptr(part[nbt * NHEAD * U * H * W:]), 128 * (nt_all - nbt), 128, U, H, W,
                     ptr(hb), ptr(o), None, stream())
                # everything the regression launches read (tensors kept alive here)
                self._box_ctx = dict(
                    args=(ptr(xp0) if C0k else None, C0k, ptr(ui), ptr(xp1), C1, U, H, W, ks, pc, ptr(wp[0]),
                          ptr(wp[1]), ptr(xmax1), ptr(bias), N, 1, ptr(hw)),
                    a0=a0, fl=fl, epi=epi, hb=hb, part=part, b=b, nbt=nbt, flops_per_point=2.0 * 128 * nbt *
                    (C0k + C1) * ks ** 2, keep=(xp0, ui, xp1, wp, xmax1, bias, hw, acc0, bplane))
                return o, b
            call("tmr_heads_reduce", ptr(part), N, 128, U, H, W, ptr(hb), ptr(o),
                 ptr(b) if b is not None else None, stream())
            return o, b
        # general depth: per-decoder conv stack, heads as 1x1 convs
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
    # box at configs B-E (profiles/r07points/crossover.json): 3-term fp16 0.40-0.43, one term 0.29
    BOX_POINTS_CROSSOVER = {"fp32": 0.40, "bf16": 0.28, "f16": 0.28}

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
        decode(box_later=True)'s operands."""
        c = self._box_ctx
        if len(tiles) == 0:
            return
        td = _h2d(np.ascontiguousarray(tiles, np.int32).reshape(-1), box.device)
        call("tmr_split_conv_points", *c["args"], ptr(c["hb"]), c["a0"], ptr(box), ptr(td), len(tiles),
             ptr(c["b"]), c["fl"] | split_tile_window(0, c["nbt"]), stream())

    def box_dense(self) -> None:
        """b everywhere: decoder_b's tiles of the dense heads launch."""
        c = self._box_ctx
        U, H, W = c["args"][5:8]
        N = c["args"][14]
        call("tmr_split_conv", *c["args"], c["a0"], ptr(c["part"]),
             c["fl"] | c["epi"] | split_tile_window(0, c["nbt"]), stream())
        scratch_o = torch.empty(U * H * W, device=c["b"].device, dtype=torch.float32)
        call("tmr_heads_reduce", ptr(c["part"]), 128 * c["nbt"], 128, U, H, W, ptr(c["hb"]), ptr(scratch_o),
             ptr(c["b"]), stream())

    def _detect_box_at_peaks(self, feats, unit_image, boxes, params):
        """detect()'s eager forward with the regression at the peaks:
        objectness tiles, finder, counts read-back, points launch (or the
        dense decoder_b tiles), decode.  Returns (logits, box, ref, counts,
        counts_host)."""
        r = self._forward_units_eager(feats, [int(i) for i in unit_image], boxes, box_later=True)
        o, b = r["o"], r["b"]
        U = o.shape[0]
        H, W = o.shape[-2:]
        logits, box, ref, counts, _ = self.peaks(o, None, params, want_prob=False, phase="find")
        counts_host = counts.cpu().numpy()  # torch.where-style sync (TM_utils.py:254)
        need = np.where(params["mode"] != 2, counts_host, 0)
        self.last_points = int(need.sum())
        dense = self.box_at_peaks == "auto" and \
            self.last_points > self.BOX_POINTS_CROSSOVER[self.cfg.precision] * U * H * W
        self.last_box_route = "dense" if dense else "points"
        if dense:
            self.box_dense()
            self.last_points_flops = 0.0
        else:
            tiles = host.point_tiles(need, POINTS_TILE)
            self.box_at_points(box, tiles)
            self.last_points_flops = self._box_ctx["flops_per_point"] * POINTS_TILE * len(tiles)
        self._box_ctx = None
        self.peaks(o, b, params, want_prob=False, phase="decode", found=(logits, box, ref, counts))
        return logits, box, ref, counts, counts_host

    @staticmethod
    def _units_per_image(unit_image, B: int) -> int:
        """E when the units are E per image in image order (the heads launch
        then runs image-major, TMR_SPLIT_UNITS_PER_IMAGE_SHIFT), else 1."""
        U = len(unit_image)
        E = U // max(B, 1)
        if E <= 1 or E > HEADS_IMAGE_MAJOR_MAX or E * B != U:
            return 1
        ui = np.asarray(unit_image)
        return E if np.array_equal(ui, np.repeat(np.arange(B), E)) else 1

    # ---------------------------------------------------- per-image reuse
    def _same_image(self, memo, feats: torch.Tensor) -> bool:
        return memo is not None and memo[0]() is feats and memo[1] == feats._version and \
            memo[2] == feats.data_ptr()

    def _acc0_lookup(self, feats, split, H, W):
        m = self._acc0_memo
        if self.reuse_image_work and self._same_image(m, feats) and m[3] is split and m[4] == (H, W):
            return m[5]
        return None

    def _acc0_store(self, feats, split, H, W, acc0):
        self._acc0_memo = (weakref.ref(feats), feats._version, feats.data_ptr(), split, (H, W), acc0)

    def _memo_hit(self, feats: torch.Tensor):
        """(fp, acc0) kept for this feature tensor by an earlier call, or None."""
        m, a = self._fp_memo, self._acc0_memo
        params = (self.P["input_proj.0.weight"], self.P["input_proj.0.bias"])
        pkey = (_version_key(params), self.cfg.precision, self.cfg.feature_upsample)
        if self._same_image(m, feats) and m[3] == pkey and all(r() is t for r, t in zip(m[5], params)) and \
                self._same_image(a, feats):
            return m[4], a[3:6]
        return None

    def _rebind_memos(self, feats: torch.Tensor, fp: torch.Tensor, acc0_memo: tuple):
        """Point the per-image memos at (fp, acc0) for `feats`; acc0_memo =
        (split, (H, W), acc0) as _acc0_store keeps them."""
        params = (self.P["input_proj.0.weight"], self.P["input_proj.0.bias"])
        pkey = (_version_key(params), self.cfg.precision, self.cfg.feature_upsample)
        self._fp_memo = (weakref.ref(feats), feats._version, feats.data_ptr(), pkey, fp,
                         tuple(weakref.ref(t) for t in params))
        self._acc0_memo = (weakref.ref(feats), feats._version, feats.data_ptr()) + tuple(acc0_memo)

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
        sig = base + (bool(want_aux), None if hit is None else (hit[0].data_ptr(), hit[1][2].data_ptr()))
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
        out = g.replay(feats.float().contiguous(), host_in, reuse_feats=True)
        for k, v in g.last.items():
            setattr(self, k, v)
        if hit is None:  # this image's memo: the first-call graph's fp / acc0
            self._rebind_memos(feats, g.fp, g.acc0)
        return _clone_outputs(out)

    def _capture_module(self, feats, unit_image, boxes, want_aux, hit, host_in):
        static = feats.detach().float().contiguous().clone()
        blob = _HostBlob(host_in, feats.device)
        saved = (self._fp_memo, self._acc0_memo)
        if hit is not None:
            self._rebind_memos(static, hit[0], hit[1])  # the capture reads the memo buffers
        else:
            self._fp_memo = self._acc0_memo = None
        torch.cuda.synchronize(feats.device)
        graph = torch.cuda.CUDAGraph()
        _capture.blob = blob
        try:
            with _no_gc(), torch.cuda.graph(graph):
                blob.upload()
                out = self._forward_units_eager(static, unit_image, boxes, want_aux)
            fp_acc0 = (self._fp_memo[4], self._acc0_memo[3:6]) if hit is None else (None, None)
        except Exception as err:  # noqa: BLE001 -- stay eager
            self.last_graph_error = f"{type(err).__name__}: {err}"
            self._fp_memo, self._acc0_memo = saved
            return None
        finally:
            _capture.blob = None
        self._fp_memo, self._acc0_memo = saved
        g = _DetectGraph(graph, static, blob, out,
                         {k: v for k, v in vars(self).items() if k.startswith("last_") and
                          not k.startswith("last_graph")})
        g.fp, g.acc0 = fp_acc0
        return g

    def forward_units(self, feats: torch.Tensor, unit_image: Sequence[int], unit_boxes,
                      want_aux: bool = False):
        """One matching_net forward per unit (image unit_image[u], exemplar
        unit_boxes[u]).  Returns dict(o, b, f_tm_relu, f0, fp)."""
        unit_image = [int(i) for i in unit_image]
        if self.reuse_image_work and getattr(_capture, "blob", None) is None:
            r = self._forward_units_graphed(feats, unit_image, unit_boxes, want_aux)
            if r is not None:
                return r
        return self._forward_units_eager(feats, unit_image, unit_boxes, want_aux)

    def _forward_units_eager(self, feats: torch.Tensor, unit_image: Sequence[int], unit_boxes,
                             want_aux: bool = False, box_later: bool = False):
        m = self._fp_memo
        # the projection memo follows the input_proj parameters' storage,
        # version AND identity (as _PackCache), and the path options that
        # change the projection's arithmetic
        params = (self.P["input_proj.0.weight"], self.P["input_proj.0.bias"])
        pkey = (_version_key(params), self.cfg.precision, self.cfg.feature_upsample)
        if self.reuse_image_work and self._same_image(m, feats) and m[3] == pkey and \
                all(r() is t for r, t in zip(m[5], params)):
            fp, f0 = m[4], None
            if want_aux:  # f[0]: a fresh tensor per call, like the reference's
                f0 = feats
                if self.cfg.feature_upsample:
                    B, Cin, Hin, Win = feats.shape
                    f0 = torch.empty((B, Cin, 2 * Hin, 2 * Win), device=feats.device, dtype=torch.float32)
                    call("tmr_upsample2x", ptr(feats.float().contiguous()), B * Cin, Hin, Win, ptr(f0),
                         stream())
        else:
            fp, f0 = self.project(feats, want_f0=want_aux)
            if self.reuse_image_work:
                self._fp_memo = (weakref.ref(feats), feats._version, feats.data_ptr(), pkey, fp,
                                 tuple(weakref.ref(t) for t in params))
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
        if phase == "decode":
            logits, box, ref, counts = found
            call("tmr_peaks_decode", ptr(o), flags | PEAKS_DECODE_ONLY, ptr(bb) if bb is not None else None,
                 U, H, W, ptr(prm), ptr(o), ptr(logits), ptr(box), ptr(ref), ptr(counts),
                 ptr(tab) if tab is not None else None, stream())
            return logits, box, ref, counts, None
        prob = torch.empty((U, H, W), device=dev, dtype=torch.float32)  # (scratch unless want_prob)
        logits = torch.empty((U * cap, 2), device=dev, dtype=torch.float32)
        box = torch.empty((U * cap, 4), device=dev, dtype=torch.float32)
        ref = torch.empty((U * cap, 2), device=dev, dtype=torch.float32)
        counts = torch.empty(U, device=dev, dtype=torch.int32)
        if phase == "find":
            flags |= PEAKS_FIND_ONLY
        call("tmr_peaks_decode", ptr(o), flags, ptr(bb) if bb is not None else None,
             U, H, W, ptr(prm), ptr(prob), ptr(logits), ptr(box), ptr(ref), ptr(counts),
             ptr(tab) if tab is not None else None, stream())
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
    # them (config A: 0.38 of 2.95 ms per image, profiles/archive/r04b/).  A signature
    # is captured the second time it is seen; up to GRAPH_MAX_UNITS units (the
    # graph's memory pool holds every intermediate) and GRAPH_CACHE entries.
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
                self.fold_proj,
                self.share_fp_half, self.xcorr_algo, self.out_bf16, TMREngine.exp_mode,
                bool(ablation_b), bool(ablation_c),
                self._param_key())

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
    def _detect_host_inputs(units, unit_image, B, params, nms_in=None) -> Dict[str, np.ndarray]:
        """The tagged host inputs of detect's forward, as _h2d stages them
        (nms_in: the speculative small NMS's (unit_off, seg) arrays)."""
        d = {"units": units.view(np.uint8), "img_units": np.asarray(host.image_ranges(unit_image, B)),
             "unit_image": np.asarray(unit_image, np.int32), "unit_image64": np.asarray(unit_image, np.int64),
             "peak_params": params.view(np.uint8)}
        if nms_in is not None:
            d["nms_unit_off"], d["nms_seg"] = nms_in
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

    def _capture_detect(self, feats, unit_image, boxes, params, host_in, nms=None):
        """Capture _forward_peaks on a static copy of feats (caches built by
        the eager call that preceded).  None if capture fails (eager then)."""
        static = feats.detach().float().contiguous().clone()
        blob = _HostBlob(host_in, feats.device)
        torch.cuda.synchronize(feats.device)
        graph = torch.cuda.CUDAGraph()
        _capture.blob = blob
        try:
            with _no_gc(), torch.cuda.graph(graph):
                blob.upload()
                out = self._forward_peaks(static, unit_image, boxes, params, nms)
        except Exception as err:  # noqa: BLE001 -- a launch this HIP runtime cannot capture: stay eager
            self.last_graph_error = f"{type(err).__name__}: {err}"
            return None
        finally:
            _capture.blob = None
        last = {k: v for k, v in vars(self).items() if k.startswith("last_") and not k.startswith("last_graph")}
        return _DetectGraph(graph, static, blob, out, last)

    def detect(self, feats: torch.Tensor, exemplars, cls_ths: float, iou_threshold: float,
               ablation_b: bool = False, ablation_c: bool = False):
        """The reference's multi-exemplar inference (demo.py:106-130,
        trainer.py:95-118) for a batch: per image, one forward per exemplar,
        Get_pred_boxes, concat in exemplar order, one NMS.

        exemplars: [B,E,4] normalised xyxy (array or tensor).
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
        sig = units = nms_in = None
        if self.use_graphs and len(unit_image) <= self.GRAPH_MAX_UNITS:  # else no graph prep at all
            units = host.build_units(boxes, unit_image, H, W, C, self.cfg.template_type)[0] \
                if not self.cfg.no_matcher else np.zeros(0, UNIT_DTYPE)
            sig = self._graph_signature(feats, units, unit_image, ablation_b, ablation_c)
            # small batches also run the device-sized small NMS in the same
            # forward (tmr_nms_small): one sync instead of two when every
            # image's union fits NMS_SMALL rows (else tmr_nms after the sync)
            nms_in = (unit_off, seg.astype(np.int32))
            if sig is not None:
                sig = sig + (float(iou_threshold),)  # a kernel argument of the captured NMS
        spec = (unit_off, seg.astype(np.int32), iou_threshold) if nms_in is not None else None
        g = self._graphs.get(sig) if sig is not None else None
        self.last_graph = "replay" if g is not None else "eager"
        if g is None and sig is not None and self._graphs.want_capture(sig):
            g = self._capture_detect(feats, unit_image, boxes, params, self._detect_host_inputs(
                units, unit_image, B, params, nms_in), spec)
            self._graphs.put(sig, g)
            if g is not None:
                self.last_graph = "captured"
        if g is not None:
            host_in = self._detect_host_inputs(units, unit_image, B, params, nms_in)
            out = g.replay(feats.float().contiguous(), host_in)
            for k, v in g.last.items():
                setattr(self, k, v)
        elif spec is None and self.box_at_peaks_ok():
            # the unspeculated eager route: the regression only at the peaks
            logits, box, ref, counts, counts_host = self._detect_box_at_peaks(feats, unit_image, boxes, params)
            self.last_nms_small = False
            return self.nms(logits, box, ref, counts, counts_host, unit_off, seg, iou_threshold)
        else:
            self.last_box_route = None
            out = self._forward_peaks(feats, unit_image, boxes, params, spec)
        logits, box, ref, counts = out[:4]
        if spec is not None:
            ck = out[4].cpu().numpy()  # torch.where-style sync (TM_utils.py:254): counts + kept
            counts_host, kept = ck[:U], ck[U:]
            self.last_nms_small = bool((kept >= 0).all())
            if self.last_nms_small:
                # graph outputs are the graph's static buffers: copied out
                ol, ob, orf = (t.clone() for t in out[5:8]) if g is not None else out[5:8]
                s0 = [int(i) * NMS_SMALL for i in range(B)]
                return ([ol[a:a + int(k)] for a, k in zip(s0, kept)], [ob[a:a + int(k)] for a, k in zip(s0, kept)],
                        [orf[a:a + int(k)] for a, k in zip(s0, kept)])
        else:
            counts_host = counts.cpu().numpy()  # torch.where-style sync (TM_utils.py:254)
            self.last_nms_small = False
        return self.nms(logits, box, ref, counts, counts_host, unit_off, seg, iou_threshold)
