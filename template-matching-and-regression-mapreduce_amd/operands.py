"""Operands of the split 16-bit-MFMA conv kernel (conv_split.hip): scale sources,
packed weights and records, the projection fold; one whole nn.Conv2d on it (conv2d_split)."""
from __future__ import annotations

from typing import Optional

import torch

from ._lib import (PREC_CODES, SIZE_KINDS, SPLIT_XMAX_PER_PIXEL, SPLIT_XMAX_PER_UNIT, XPACK_ONES, XPACK_UPSAMPLE,
                   TMRError, call, load, ptr, require_gpu, stream)


def absmax(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """max |x| as a 1-element device tensor (max(out, |x|) when out is given):
    tmr_absmax_rows over one row."""
    return _absmax(x, out, rows=False)


def absmax_rows(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Per-sample max |x[s]| of x [S, ...] as an [S] device tensor (max(out, .)
    when out is given): the per-sample activation scale source of the split
    kernels (tmr_absmax_rows)."""
    return _absmax(x, out, rows=True)


def _absmax(x: torch.Tensor, out: Optional[torch.Tensor], rows: bool) -> torch.Tensor:
    require_gpu(x, "absmax input")
    if x.dtype != torch.float32:
        raise TMRError(f"absmax of a {x.dtype} tensor (fp32 only)")
    x = x.contiguous()
    S = x.shape[0] if rows else 1
    acc = out is not None
    if out is None:
        out = torch.empty(S, device=x.device, dtype=torch.float32)
    elif rows and out.numel() != S:
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
        call("tmr_split_xpack16", ptr(x.contiguous()), S, C, H, W, ks, pc, ptr(out), stream())
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
