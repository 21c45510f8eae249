"""CPU-only: the operand-prep restatement (tests/operand_ref.py) checked
against the host's sizing arithmetic, the library's tmr_size and the
properties include/tmr.h states for the records and fragments."""
import os
import re

import numpy as np
import pytest
import torch

import operand_ref as orf
import tmr_amd
from tmr_amd import _lib, host

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(os.path.dirname(_lib.LIB_PATH), "csrc")
ODD = range(1, 32, 2)


def _size(kind, *d):
    return int(tmr_amd.load().tmr_size(_lib.SIZE_KINDS[kind], *(list(d) + [0] * (6 - len(d)))))


def test_hi_bit_constants_match_the_sources():
    """WH_BITS / TH_BITS of the restatement are the kernels' constants (a
    retune edits the source, operand_ref.py and DESIGN.md §4.2 together)."""
    for name, src, val in (("WH_BITS", "conv_split.hip", orf.WH_BITS), ("TH_BITS", "xcorr.hip", orf.TH_BITS)):
        txt = open(os.path.join(CSRC, src)).read()
        got = re.findall(r"constexpr int %s = (\d+);" % name, txt)
        assert got == [str(val)], (name, got)
    assert orf.PREC_NAMES == {v: k for k, v in _lib.PREC_CODES.items()}


def test_split_scale():
    """2^13 <= m * scale < 2^14 inside the clamp; 1 for 0, negative, NaN, inf
    and sources above 3e38; clamped to [2^-63, 2^63]."""
    rng = np.random.default_rng(0)
    m = np.exp2(rng.uniform(-48, 76, 4000)).astype(np.float32)
    m = np.concatenate([m, np.exp2(np.arange(-48, 77)).astype(np.float32),
                        np.nextafter(np.exp2(np.arange(-48, 77)).astype(np.float32), np.float32(0))])
    s = orf.split_scale(m)
    p = m.astype(np.float64) * s
    assert (p >= 2.0 ** 13).all() and (p < 2.0 ** 14).all()
    assert (np.frexp(s)[0] == 0.5).all()  # powers of two
    one = orf.split_scale(np.array([0.0, -0.0, -3.0, np.nan, np.inf, -np.inf, 3.1e38], np.float32))
    assert (one == 1.0).all()
    assert orf.split_scale(np.float32(3.0e38)) == np.float32(2.0 ** -63)
    assert orf.split_scale(np.float32(2.0 ** 100)) == np.float32(2.0 ** -63)
    assert orf.split_scale(np.float32(1e-45)) == np.float32(2.0 ** 63)
    assert orf.split_scale(np.float32(2.0 ** -50)) == np.float32(2.0 ** 63)
    # the TMR_XPACK_ONES bound of the header: sources >= 0.25 keep 1 * scale finite in fp16
    assert orf.split_scale(np.float32(0.25)) == np.float32(2.0 ** 15)
    assert np.isfinite(np.float16(orf.split_scale(np.float32(0.25))))
    with np.errstate(over="ignore"):
        assert np.isinf(np.float16(orf.split_scale(np.nextafter(np.float32(0.25), np.float32(0)))))
    assert np.float16(orf.split_scale(np.float32(2.0 ** 38))) == 0  # ... and below 2^38 keep it non-zero
    assert np.float16(orf.split_scale(np.nextafter(np.float32(2.0 ** 38), np.float32(0)))) == np.float16(2.0 ** -24)


def test_absmax_and_scale_merge_statement():
    x = np.array([[1.0, np.nan, -3.0, 2.0], [np.nan, np.nan, np.nan, np.nan], [-0.0, -0.0, 0.0, -0.0],
                  [1.0, -np.inf, np.nan, 5.0]], np.float32)
    got = orf.absmax(x, axis=1)
    assert got.view(np.uint32).tolist() == np.array([3.0, 0.0, 0.0, np.inf], np.float32).view(np.uint32).tolist()
    assert orf.absmax(np.zeros((3, 0), np.float32), axis=1).tolist() == [0, 0, 0]
    oi, ou = orf.scale_merge([0.5, 7.0, 1.0], [2.0, 9.0, 4.0], [2, 0, 2], 3)
    assert oi.tolist() == [9.0, 7.0, 4.0] and ou.tolist() == [4.0, 9.0, 4.0]
    oi, ou = orf.scale_merge(None, [2.0, 9.0, 4.0], [2, 0, 2], 3)
    assert oi.tolist() == [9.0, 0.0, 4.0] and ou.tolist() == [4.0, 9.0, 4.0]


def test_round_sig_bits():
    x = np.array([1.0, 1.00390625, 1.001953125, 1.005859375, -1.005859375, 255.5, 3.0e-40, np.inf], np.float32)
    # 8 bits: ulp 2^-7 at 1; ties to even
    exp = np.array([1.0, 1.0, 1.0, 1.0078125, -1.0078125, 256.0, 0, np.inf], np.float32)
    got = orf.round_sig_bits(x, 8)
    assert got[:6].tolist() == exp[:6].tolist() and np.isinf(got[7])
    assert (orf.round_sig_bits(x, 24).view(np.uint32) == x.view(np.uint32)).all()
    rng = np.random.default_rng(1)
    v = (rng.standard_normal(5000) * np.exp2(rng.integers(-20, 20, 5000))).astype(np.float32)
    for k in (6, 8, 11):
        r = orf.round_sig_bits(v, k)
        assert (np.abs(r.astype(np.float64) - v) <= 2.0 ** -k * np.abs(v)).all()
        assert ((r.view(np.uint32) & ((1 << (24 - k)) - 1)) == 0).all()


def test_window_counts_match_host_and_tmr_size():
    """For every odd h, w <= 31: na * nb of the header's formulas equals
    host.tsplit_windows (what the engine sizes buffers and offsets with), and
    TMR_SIZE_TEMPLATE_SPLIT is the header's byte formula."""
    total = 0
    for h in ODD:
        for w in ODD:
            n = orf.window_count(h, w)
            assert n == host.tsplit_windows(h, w), (h, w)
            assert n == int(host.tsplit_windows_vec(np.array([h]), np.array([w]))[0])
            i, j, valid = orf.window_taps(h, w)
            assert i.shape == j.shape == valid.shape == orf.window_geometry(h, w)[:2] + (64, 8)
            total += n
            for U, C in ((1, 1), (3, 5)):
                assert _size("template_split", U, C, n) == orf.template_split_bytes(U, C, n)
    assert _size("template_split", 256, 7, total) == orf.template_split_bytes(256, 7, total)


def test_every_tap_sits_where_the_formula_names():
    """For every odd h, w <= 31 and every one of the 16 (m >> 3, m & 7) patch
    positions of a lane: tap T[i][j] is element q = (j + (m&7) + s) % 8 of lane
    m + 16 g, g = (i + (m>>3)) % 4, of window (a, b) = ((i + (m>>3)) / 4,
    (j + (m&7) + s) / 8) -- the inverse of the header's lane formula -- and
    every other element is zero: each output position meets each tap once."""
    for h in ODD:
        for w in ODD:
            na, nb, s = orf.window_geometry(h, w)
            # distinct taps, exact in fp16 at any scale: 1 .. h*w <= 961 < 2^10
            T = (1 + np.arange(h * w, dtype=np.float32)).reshape(1, h, w)
            frags, known, exps = orf.template_split_ref([T], [0], na * nb, orf.F16X3)
            assert known.all() and frags.shape[0] == 2 * na * nb
            sc = 2.0 ** -float(exps[0, 0])
            assert 2.0 ** 13 <= h * w * sc < 2.0 ** 14
            hi = frags[0::2].view(np.float16).astype(np.float64) / sc  # [b * na + a][lane][q]
            assert not frags[1::2].any()  # exact values: no lo part
            i, j, m = np.meshgrid(np.arange(h), np.arange(w), np.arange(16), indexing="ij")
            r, cc = m >> 3, m & 7
            a, g = (i + r) // 4, (i + r) % 4
            b, q = (j + cc + s) // 8, (j + cc + s) % 8
            assert a.max() < na and b.max() < nb, (h, w)
            got = hi[b * na + a, m + 16 * g, q]
            assert np.array_equal(got, T[0][i, j]), (h, w)
            assert np.count_nonzero(hi) == 16 * h * w, (h, w)


def test_template_split_offsets_and_exponents():
    """Two units in either order: fragments land at C * row_offset(u) + c * na
    * nb; the exponent is 0 for an all-zero channel and scales max |T| into
    [2^13, 2^14) otherwise; the one-term precisions leave the lo slots unknown."""
    rng = np.random.default_rng(2)
    t0 = rng.standard_normal((2, 5, 9)).astype(np.float32)
    t1 = rng.standard_normal((2, 3, 3)).astype(np.float32) * np.float32(2.0 ** 20)
    t1[1] = 0
    n0, n1 = orf.window_count(5, 9), orf.window_count(3, 3)
    fa, ka, ea = orf.template_split_ref([t0, t1], [0, n0], n0 + n1, orf.F16X3)
    fb, kb, eb = orf.template_split_ref([t1, t0], [0, n1], n0 + n1, orf.F16X3)
    assert ka.all() and kb.all()
    assert np.array_equal(fa[:2 * 2 * n0], fb[2 * 2 * n1:]) and np.array_equal(fa[2 * 2 * n0:], fb[:2 * 2 * n1])
    assert np.array_equal(ea, eb[::-1]) and ea[1, 1] == 0
    for e, t in ((ea[0, 0], t0[0]), (ea[1, 0], t1[0])):
        assert 2.0 ** 13 <= np.abs(t).max() * 2.0 ** -float(e) < 2.0 ** 14
    assert not fa[2 * 2 * n0 + 2 * n1:].any()  # the zero channel: zero words in both terms
    for prec in (orf.F16, orf.BF16):
        f1, k1, e1 = orf.template_split_ref([t0, t1], [0, n0], n0 + n1, prec)
        assert k1[0::2].all() and not k1[1::2].any() and np.array_equal(e1, ea)
    f16 = orf.template_split_ref([t0, t1], [0, n0], n0 + n1, orf.F16)[0]
    assert np.array_equal(f16[0::2], fa[0::2]) == (orf.TH_BITS >= 11)


@pytest.mark.parametrize("prec", [orf.F16X3, orf.BF16, orf.F16])
def test_record_sizes_match_tmr_size(prec):
    rng = np.random.default_rng(3)
    for N, C0, C1, ks in ((8, 24, 0, 1), (136, 24, 40, 3), (130, 0, 33, 5), (16, 12, 0, 7)):
        w = rng.standard_normal((N, C0 + C1, ks, ks)).astype(np.float32)
        rec = orf.wrecords_ref(w, C0, C1, prec, np.abs(w).max())
        assert rec.dtype == np.uint16
        assert 2 * rec.size == _size("wpack", N, C0, C1, ks, prec) == orf.wpack_bytes(N, C0, C1, ks, prec)
    for S, C, H, W, ks in ((2, 32, 10, 18, 3), (1, 32, 16, 32, 1), (2, 41, 14, 12, 5), (3, 33, 8, 12, 7)):
        x = torch.from_numpy(rng.standard_normal((S, C, H, W)).astype(np.float32))
        rec = orf.xrecords_ref(x, ks, orf.PREC_NAMES[prec], float(x.abs().max()))
        assert rec.dtype == torch.int16
        assert 2 * rec.numel() == _size("xpack", S, C, H, W, ks, prec) == orf.xpack_bytes(S, C, H, W, ks, prec)


def test_wrecords_layout_and_padding():
    """Each weight sits at [tap][chunk][plane q][n][j] with channel 32 c + 8 q
    + j of its own source, src1's chunks after src0's; everything else is zero."""
    N, C0, C1, ks = 5, 33, 3, 3
    w = (1 + np.arange(N * (C0 + C1) * ks * ks, dtype=np.float32)).reshape(N, C0 + C1, ks, ks)  # < 2^11: exact
    assert w.max() < 2048
    rec = orf.wrecords_ref(w, C0, C1, orf.F16, w.max()).reshape(ks * ks, 3, 4, 128, 8)
    sc = float(orf.split_scale(w.max()))
    val = rec.view(np.float16).astype(np.float64) / sc
    seen = 0
    for n in range(N):
        for ch in range(C0 + C1):
            c, k = (ch // 32, ch % 32) if ch < C0 else (2 + (ch - C0) // 32, (ch - C0) % 32)
            for tap in range(ks * ks):
                assert val[tap, c, k // 8, n, k % 8] == w[n, ch, tap // ks, tap % ks]
                seen += 1
    assert np.count_nonzero(val) == seen
    # F16X3: hi planes 0..3 carry WH_BITS significant bits, lo planes 4..7 the rest
    rec3 = orf.wrecords_ref(w, C0, C1, orf.F16X3, w.max()).reshape(ks * ks, 3, 8, 128, 8).view(np.float16)
    hi, lo = rec3[:, :, :4].astype(np.float64), rec3[:, :, 4:].astype(np.float64)
    assert np.array_equal((hi + lo) / sc, val)
    assert np.array_equal(orf.round_sig_bits(hi.astype(np.float32), orf.WH_BITS), hi.astype(np.float32))
    if orf.WH_BITS < 11:
        assert np.count_nonzero(lo)


@pytest.mark.parametrize("K", sorted({orf.WH_BITS, orf.TH_BITS, orf.XH_BITS}))
def test_hi_lo_reconstruction_bound(K):
    """(hi + lo) / s reconstructs x to within 2^-(K+11) |x| + 2^-25 / s: the
    residual after a K-bit hi is at most 2^-K |x s|, fp16 keeps 11 bits of it,
    and 2^-25 is half the smallest fp16 subnormal."""
    rng = np.random.default_rng(4)
    for spread in (0, 10, 30):
        x = (rng.standard_normal(20000) * np.exp2(-rng.uniform(0, spread, 20000))).astype(np.float32)
        for mag in (3e-5, 1.0, 7e4):
            xm = (x * np.float32(mag)).astype(np.float32)
            s = orf.split_scale(orf.absmax(xm))
            hi, lo = orf.split_terms((xm * s).astype(np.float32), orf.F16X3, K)
            rec = (hi.view(np.float16).astype(np.float64) + lo.view(np.float16).astype(np.float64)) / float(s)
            bound = 2.0 ** -(K + 11) * np.abs(xm.astype(np.float64)) + 2.0 ** -25 / float(s)
            assert (np.abs(rec - xm) <= bound).all(), (K, spread, mag)
            assert np.isfinite(hi.view(np.float16)).all()


def test_heads_reduce_and_fold_statement():
    rng = np.random.default_rng(5)
    p = rng.standard_normal((3, 5, 2, 2, 3)).astype(np.float32)
    hb = rng.standard_normal(5).astype(np.float32)
    o, b = orf.heads_reduce_ref(p, hb)
    s = ((np.float32(0) + p[0]) + p[1]) + p[2]
    assert np.array_equal(o[:, 0], s[4] + hb[4]) and np.array_equal(b[:, 2], s[2] + hb[2])
    pn = p.copy()
    pn[:, :4] = np.nan
    o2, b2 = orf.heads_reduce_ref(pn, hb, with_b=False)
    assert b2 is None and np.array_equal(o2, o)
    # -0 partials: the sum starts from +0
    z = np.full((2, 5, 1, 1, 1), -0.0, np.float32)
    oz, _ = orf.heads_reduce_ref(z, np.zeros(5, np.float32))
    assert not np.signbit(oz).any()
    wd = rng.standard_normal((4, 6, 3, 3)).astype(np.float32)
    pw, pb = rng.standard_normal((5, 3)).astype(np.float32), rng.standard_normal(5).astype(np.float32)
    out = orf.fold_proj_ref(wd, 5, pw, pb)
    assert out.shape == (4, 4, 3, 3) and out.dtype == np.float32
    ref = np.einsum("nkyx,kc->ncyx", wd[:, :5].astype(np.float64), pw.astype(np.float64))
    refb = np.einsum("nkyx,k->nyx", wd[:, :5].astype(np.float64), pb.astype(np.float64))
    assert np.abs(out[:, :3] - ref).max() <= 1e-6 and np.abs(out[:, 3] - refb).max() <= 1e-6
