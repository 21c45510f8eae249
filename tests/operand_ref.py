"""TEST HELPER: plain numpy / torch restatements of the operand-prep entry
points of include/tmr.h -- the scale sources, the 16-bit activation and weight
records, the correlation's template fragments, the heads reduce and the
projection fold -- written from the header's text, not from the kernels.

Each function names the header passage it restates (include/tmr.h, by the
passage's first words; line numbers as of this file's writing).  All
arithmetic is fp32 with every operation separately rounded unless stated, all
16-bit conversions round to nearest even (numpy's float16, torch's bfloat16).
tests/test_operand_ref_host.py checks this file on the CPU;
tests/test_gpu_operands.py compares the kernels with it bit for bit.
"""
from __future__ import annotations

import numpy as np
import torch

f32 = np.float32

# TMR_PREC_* (tmr.h "#define TMR_PREC_F16X3")
F16X3, BF16, F16 = 0, 1, 2
PREC_NAMES = {F16X3: "fp32", BF16: "bf16", F16: "f16"}

# Significant bits of the hi part of the 3-term split: the
# weights' (tmr.h "F16X3 wh = fp16(v rounded to WH_BITS", :295; the constant
# of that name in csrc/conv_split.hip) and the templates' (tmr.h "The terms,
# by prec", :188; csrc/xcorr.hip).  A retune edits these two lines;
# test_operand_ref_host.py holds them to the sources.
WH_BITS = 8
TH_BITS = 11
XH_BITS = 11  # activations: always the plain fp16 hi (tmr.h :259, :299)


# ----------------------------------------------------------------- scales
def split_scale(m) -> np.ndarray:
    """tmr.h "Scale sources and scales" (:232): 2^clamp(14 - e, -63, 63) with
    2^(e-1) <= m < 2^e; 1 for m <= 0, NaN, inf or m > 3e38.  Elementwise, fp32."""
    m = np.asarray(m, f32)
    ok = (m > 0) & (m <= f32(3.0e38))  # false for NaN
    e = np.frexp(np.where(ok, m, f32(1)))[1]  # m = f 2^e, 0.5 <= f < 1
    s = np.exp2(np.clip(14 - e, -63, 63).astype(np.float64))
    return np.where(ok, s, 1.0).astype(f32)


def absmax(x, axis=None) -> np.ndarray:
    """The scale source of tmr_absmax_rows / tmr_pixel_absmax (tmr.h :238-244, :378):
    max |x| ignoring NaN, +inf for an infinity, +0 for an empty or all-zero
    (or all-NaN) input."""
    a = np.abs(np.asarray(x, f32))
    return np.fmax.reduce(a, axis=axis, initial=f32(0)).astype(f32)


def scale_merge(img_max, unit_max, unit_image, B):
    """tmr_scale_merge (tmr.h :245-251): (out_img [B], out_unit [U])."""
    unit_max, unit_image = np.asarray(unit_max, f32), np.asarray(unit_image)
    out_img = np.zeros(B, f32)
    for b in range(B):
        m = f32(0)
        if img_max is not None:
            m = np.fmax(m, f32(img_max[b]))
        for u in np.nonzero(unit_image == b)[0]:
            m = np.fmax(m, unit_max[u])
        out_img[b] = m
    return out_img, out_img[unit_image]


# --------------------------------------------------------- the hi/lo split
def round_sig_bits(x, bits: int) -> np.ndarray:
    """"Rounded to K significant bits" (tmr.h :191-194): round to nearest even
    on the fp32 bit pattern, clearing its low 24 - K bits; inf / NaN unchanged."""
    x = np.ascontiguousarray(x, f32)
    if bits >= 24:
        return x.copy()
    u = x.view(np.uint32).astype(np.uint64)
    drop = 24 - bits
    r = (u + ((1 << (drop - 1)) - 1) + ((u >> drop) & 1)) & ~np.uint64((1 << drop) - 1)
    r = np.where((u & 0x7f800000) == 0x7f800000, u, r)
    return r.astype(np.uint32).view(f32)


def _words16(v: np.ndarray, bf16: bool) -> np.ndarray:
    v = np.ascontiguousarray(v, f32)
    if bf16:
        return torch.from_numpy(v).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    with np.errstate(over="ignore"):
        return v.astype(np.float16).view(np.uint16)


def split_terms(v, prec: int, hi_bits: int):
    """The 16-bit terms of already scaled fp32 values v: (hi words, lo words or
    None) as uint16.  F16X3: hi = fp16(v rounded to hi_bits significant bits)
    (hi_bits >= 11: the plain fp16(v)), lo = fp16(v - hi), the difference in
    fp32; F16: fp16(v); BF16: bf16(v).  (tmr.h :188-198, :259-261, :294-299)
    The sign of the zero terms of a -0.0 input is unspecified there (:261-266);
    this restatement gives the IEEE one."""
    v = np.ascontiguousarray(v, f32)
    if prec == BF16:
        return _words16(v, True), None
    with np.errstate(over="ignore"):
        if prec == F16X3 and hi_bits < 11:
            h = round_sig_bits(v, hi_bits).astype(np.float16)
        else:
            h = v.astype(np.float16)
    if prec != F16X3:
        return h.view(np.uint16), None
    with np.errstate(invalid="ignore"):
        lo = (v - h.astype(f32)).astype(f32)
    return h.view(np.uint16), _words16(lo, False)


# ------------------------------------------------------ activation records
def xpack_dims(C, H, W, ks):
    """(NC, Hp, Wp) of tmr_split_xpack (tmr.h :252-257)."""
    return -(-C // 32), -(-H // 16) * 16 + ks - 1, -(-W // 32) * 32 + ks - 1


def xpack_bytes(S, C, H, W, ks, prec) -> int:
    NC, Hp, Wp = xpack_dims(C, H, W, ks)
    return S * NC * (2 if prec == F16X3 else 1) * Hp * Wp * 64


def xrecords_ref(x, ks, prec, xmax):
    """tmr_split_xpack's record layout restated in torch (tmr.h :252-261):
    [s][chunk][half][piece q][Hp][Wp][8 x 16-bit], hi = fl16(x s), lo =
    fl16(x s - hi) (F16X3), s = split_scale of the scale source(s), zero ring.
    x: torch [S,C,H,W] (any device); prec "fp32" / "bf16" / "f16"; xmax: one
    source, one per sample [S] or one per pixel [S,H,W].  Returns the int16
    words, flat, on x's device."""
    S, C, H, W = x.shape
    NCc, pad = (C + 31) // 32, ks // 2
    Hp, Wp = -(-H // 16) * 16 + ks - 1, -(-W // 32) * 32 + ks - 1
    xs = torch.zeros(S, NCc * 32, Hp, Wp, dtype=torch.float32, device=x.device)
    sc = 1.0
    if prec != "bf16":
        m = np.asarray(xmax, np.float32)
        sc = split_scale(m)
        sc = torch.from_numpy(sc.reshape((S, 1, H, W) if m.ndim == 3 else (-1, 1, 1, 1) if m.ndim else ()))
        sc = sc.to(x.device)
    xs[:, :C, pad:pad + H, pad:pad + W] = x * sc
    dt = torch.bfloat16 if prec == "bf16" else torch.float16
    hi = xs.to(dt)
    halves = [hi]
    if prec == "fp32":
        halves.append((xs - hi.float()).to(dt))
    # [S][NCc][32][Hp][Wp] -> [S][NCc][P=4][Hp][Wp][8]
    recs = [h.view(S, NCc, 4, 8, Hp, Wp).permute(0, 1, 2, 4, 5, 3) for h in halves]
    return torch.stack(recs, 2).contiguous().view(torch.int16).flatten()


# ---------------------------------------------------------- weight records
def wpack_bytes(N, C0, C1, ks, prec) -> int:
    """TMR_SIZE_WPACK (tmr.h :293-294)."""
    return ks * ks * (-(-C0 // 32) + -(-C1 // 32)) * (-(-N // 128) * 128) * (128 if prec == F16X3 else 64)


def wrecords_ref(w, C0, C1, prec: int, wmax) -> np.ndarray:
    """tmr_split_wpack (tmr.h :284-299): w [N][C0+C1][ks][ks] ->
    [tap][chunk: src0's then src1's][plane: 4 hi pieces, then 4 lo pieces]
    [Npad][8 x 16 bit] as flat uint16 words; zero rows / channels in the padding."""
    w = np.asarray(w, f32)
    N, C, ks, _ = w.shape
    assert C == C0 + C1
    T, NC0, NC1, Npad = ks * ks, -(-C0 // 32), -(-C1 // 32), -(-N // 128) * 128
    wt = w.reshape(N, C, T).transpose(2, 1, 0)  # [tap][channel][n]
    v = np.zeros((T, (NC0 + NC1) * 32, Npad), f32)
    v[:, :C0, :N] = wt[:, :C0]
    v[:, NC0 * 32:NC0 * 32 + C1, :N] = wt[:, C0:]
    if prec != BF16:
        v = (v * split_scale(f32(wmax))).astype(f32)
    hi, lo = split_terms(v, prec, WH_BITS)
    # [tap][chunk][piece q][element j][n] -> [tap][chunk][q][n][j]
    planes = [t.reshape(T, NC0 + NC1, 4, 8, Npad).transpose(0, 1, 2, 4, 3) for t in (hi, lo) if t is not None]
    return np.ascontiguousarray(np.concatenate(planes, 2)).reshape(-1)


# ------------------------------------------------------ template fragments
def window_geometry(h: int, w: int):
    """(na, nb, s) of tmr_template_split (tmr.h :174-175)."""
    s = (-(w // 2)) % 8
    return -(-(h + 1) // 4), -(-(w + 7 + s) // 8), s


def window_count(h: int, w: int) -> int:
    na, nb, _ = window_geometry(h, w)
    return na * nb


def template_split_bytes(U: int, C: int, total_rows: int) -> int:
    """TMR_SIZE_TEMPLATE_SPLIT (tmr.h :78-81)."""
    return C * total_rows * 2 * 1024 + 4 * U * C


def window_taps(h: int, w: int):
    """(i, j, valid), each [na][nb][64 lanes][8]: the template index every
    fragment element holds (tmr.h :176-179) and whether it lies inside."""
    na, nb, s = window_geometry(h, w)
    lane = np.arange(64)
    m, g = lane & 15, lane >> 4
    a = np.arange(na)[:, None, None, None]
    b = np.arange(nb)[None, :, None, None]
    q = np.arange(8)[None, None, None, :]
    i = 4 * a + (g - (m >> 3))[None, None, :, None] + 0 * b + 0 * q
    j = 8 * b + q - (m & 7)[None, None, :, None] - s + 0 * a
    return i, j, (i >= 0) & (i < h) & (j >= 0) & (j < w)


def template_split_ref(templates, row_offset, total_rows: int, prec: int):
    """tmr_template_split (tmr.h :166-198).  templates: per unit a [C][h][w]
    fp32 array; row_offset: per unit.  Returns (frags uint16 [C * total_rows *
    2][64][8], known bool [C * total_rows * 2], e int32 [U][C]); known is
    False for fragments no unit covers and for the lo slots of the one-term
    precisions, which the header leaves unspecified."""
    U, C = len(templates), templates[0].shape[0]
    frags = np.zeros((C * total_rows * 2, 64, 8), np.uint16)
    known = np.zeros(C * total_rows * 2, bool)
    exps = np.zeros((U, C), np.int32)
    for u, tm in enumerate(templates):
        tm = np.asarray(tm, f32)
        _, h, w = tm.shape
        na, nb, _ = window_geometry(h, w)
        i, j, valid = window_taps(h, w)
        ic, jc = np.clip(i, 0, h - 1), np.clip(j, 0, w - 1)
        fa = (np.arange(nb)[None, :] * na + np.arange(na)[:, None]) * 2  # (b * na + a) * 2
        for c in range(C):
            sc = split_scale(absmax(tm[c]))
            exps[u, c] = -(np.frexp(sc)[1] - 1)  # x = t 2^-e
            hi, lo = split_terms((tm[c] * sc).astype(f32), prec, TH_BITS)
            base = (C * int(row_offset[u]) + c * na * nb) * 2
            for k, t in enumerate((hi, lo)):
                if t is None:
                    continue
                assert not known[base + fa + k].any(), "overlapping units"
                frags[base + fa + k] = np.where(valid, t[ic, jc], np.uint16(0))
                known[base + fa + k] = True
    return frags, known, exps


# ------------------------------------------------------------ heads reduce
def heads_reduce_ref(partials, head_bias, with_b: bool = True):
    """tmr_heads_reduce (tmr.h :209-215): partials [tiles][5][U][H][W]; fp32
    sums over the tiles in order starting from +0, then the bias.  Returns
    (o [U,1,H,W], b [U,4,H,W] or None).  With with_b False only plane 4 is read."""
    p, hb = np.asarray(partials, f32), np.asarray(head_bias, f32)
    planes = range(5) if with_b else (4,)
    out = {}
    for j in planes:
        s = np.zeros(p.shape[2:], f32)
        for t in range(p.shape[0]):
            s = (s + p[t, j]).astype(f32)
        out[j] = (s + hb[j]).astype(f32)
    o = out[4][:, None]
    return o, (np.stack([out[j] for j in range(4)], 1) if with_b else None)


# -------------------------------------------------------------------- fold
def fold_proj_ref(wd, Cp: int, proj_w, proj_b) -> np.ndarray:
    """tmr_split_fold_proj (tmr.h :317-324): out [N][Cin+1][ks][ks]; every sum
    in fp64 over k ascending from 0, rounded once to fp32.  A float x float
    product is exact in a double, so a fused multiply-add gives the same bits."""
    wd = np.asarray(wd, np.float64)
    pw, pb = np.asarray(proj_w, np.float64), np.asarray(proj_b, np.float64)
    N, _, ks, _ = wd.shape
    Cin = pw.shape[1]
    acc = np.zeros((N, Cin + 1, ks, ks), np.float64)
    for k in range(Cp):
        acc[:, :Cin] += wd[:, k, None] * pw[k][None, :, None, None]
        acc[:, Cin] += wd[:, k] * pb[k]
    return acc.astype(f32)
