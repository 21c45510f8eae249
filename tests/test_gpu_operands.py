"""GPU: the operand-prep kernels of libtmr.so, each by itself, bit for bit
against the CPU restatement of include/tmr.h (tests/operand_ref.py).

Every comparison is exact (fp32 bit patterns or 16-bit words).  Every
reference, the scale sources handed to the pack references included, is
computed on the CPU with numpy; no GPU helper feeds a reference.  Every
output buffer is pre-filled with 0xA5 bytes or 1e30, so an element the kernel
does not write is seen.  Scale maxima are planted as negative values at the
positions a reduction can miss (first, last, the vector tail, block seams,
the last channel group, units past the first 256), with every other magnitude
at most half of the maximum."""
import numpy as np
import pytest
import torch

import operand_ref as orf
import oracle
from tmr_amd import _lib
from tmr_amd._lib import XPACK_ONES, XPACK_UPSAMPLE, call, ptr, size, stream

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
f32 = np.float32
PRECS = (orf.F16X3, orf.BF16, orf.F16)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def junk_f(*shape):
    return torch.full(shape, 1e30, device=DEV, dtype=torch.float32)


def junk_b(nbytes):
    return torch.full((int(nbytes),), 0xA5, device=DEV, dtype=torch.uint8)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def assert_bits(got, ref, what=""):
    got, ref = np.ascontiguousarray(got, f32), np.ascontiguousarray(ref, f32)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bad = np.nonzero(got.view(np.uint32).ravel() != ref.view(np.uint32).ravel())[0]
    assert bad.size == 0, f"{what}: {bad.size} of {ref.size} differ, first at {bad[0]}: " \
                          f"{got.ravel()[bad[0]]!r} != {ref.ravel()[bad[0]]!r}"


def assert_words(got, ref, what=""):
    got, ref = np.asarray(got).view(np.uint16).ravel(), np.asarray(ref).view(np.uint16).ravel()
    assert got.size == ref.size, (what, got.size, ref.size)
    bad = np.nonzero(got != ref)[0]
    assert bad.size == 0, f"{what}: {bad.size} of {ref.size} 16-bit words differ, first at {bad[0]}: " \
                          f"{got[bad[0]]:#06x} != {ref[bad[0]]:#06x}"


# ------------------------------------------------------------ tmr_absmax_rows
ABS_SHAPES = [(1, 1), (1, 7), (3, 1023), (5, 1024), (2, 8196), (1, 24584), (4, 65541), (700, 36), (65535, 3)]


def _positions(n, rng):
    cand = [0, n - 1, n - 4, 1023, 1024, int(rng.integers(n))]
    return sorted({p for p in cand if 0 <= p < n})


def _planted_rows(base, p):
    """base with row s's maximum -(1 + s % 13) planted at column p (an int or one per row)."""
    S = base.shape[0]
    x = base.copy()
    x[np.arange(S), p] = -(1.0 + np.arange(S) % 13).astype(f32)
    return x


def _absmax_rows(xd, S, n, accumulate=0, out=None):
    out = junk_f(S) if out is None else out
    call("tmr_absmax_rows", ptr(xd) if xd is not None else None, S, n, accumulate, ptr(out), stream())
    return host(out)


@pytest.mark.parametrize("S,n", ABS_SHAPES)
def test_absmax_rows_planted_maximum(S, n):
    """One block per row, several blocks per row on the float4 path (n % 4 ==
    0) and on the scalar path, S up to the grid limit: the planted negative
    maximum is found wherever it sits; out holds garbage before the call."""
    rng = np.random.default_rng(S * 100003 + n)
    base = rng.uniform(-0.5, 0.5, (S, n)).astype(f32)
    cases = _positions(n, rng) + [rng.integers(n, size=S)]
    for p in cases:
        x = _planted_rows(base, p)
        ref = orf.absmax(x, axis=1)
        assert np.array_equal(ref, (1.0 + np.arange(S) % 13).astype(f32))
        assert_bits(_absmax_rows(dev(x), S, n), ref, f"absmax_rows {S}x{n} max at {p}")


@pytest.mark.parametrize("S,n", [(5, 1024), (2, 8196), (1, 24584)])
def test_absmax_rows_unaligned_base(S, n):
    """n % 4 == 0 with the base pointer one float past a 16-B boundary: the
    scalar path; the element before the view holds a larger value."""
    rng = np.random.default_rng(n)
    base = rng.uniform(-0.5, 0.5, (S, n)).astype(f32)
    big = torch.full((S * n + 1,), -1e6, device=DEV, dtype=torch.float32)
    xd = big[1:].view(S, n)
    assert xd.data_ptr() % 16 == 4 and xd.is_contiguous()
    for p in _positions(n, rng):
        x = _planted_rows(base, p)
        xd.copy_(torch.from_numpy(x))
        assert_bits(_absmax_rows(xd, S, n), orf.absmax(x, axis=1), f"unaligned {S}x{n} max at {p}")


def test_absmax_rows_empty_and_accumulate():
    """n = 0: zeros (accumulate: out untouched).  accumulate = 1: max(out,
    row max) with out above the row maximum for some rows and below it for
    others; accumulate = 0 ignores what out held."""
    assert_bits(_absmax_rows(None, 3, 0), np.zeros(3, f32), "n = 0")
    keep = dev(np.array([0.0, 2.5, 7.0], f32))
    assert_bits(_absmax_rows(None, 3, 0, 1, keep), np.array([0.0, 2.5, 7.0], f32), "n = 0, accumulate")
    rng = np.random.default_rng(7)
    for n in (1028, 1030):  # the float4 path and the scalar path
        S = 6
        x = _planted_rows(rng.uniform(-0.5, 0.5, (S, n)).astype(f32), rng.integers(n, size=S))  # maxima 1 .. 6
        prev = np.array([0.25, 100.0, 2.5, 4.0, 5.5, 0.0], f32)
        ref = np.maximum(prev, orf.absmax(x, axis=1))
        assert (ref == prev).any() and (ref != prev).any()
        xd = dev(x)
        assert_bits(_absmax_rows(xd, S, n, 1, dev(prev)), ref, f"accumulate n={n}")
        assert_bits(_absmax_rows(xd, S, n, 0, dev(prev)), orf.absmax(x, axis=1), f"no accumulate n={n}")


@pytest.mark.parametrize("n", [1024, 1027])
def test_absmax_rows_special_values(n):
    """NaN elements are ignored, -inf gives +inf, a row of -0.0 gives +0."""
    rng = np.random.default_rng(n)
    x = rng.uniform(-0.5, 0.5, (4, n)).astype(f32)
    x[0, ::3] = np.nan
    x[0, n - 2] = -3.0
    x[1, n - 1] = -np.inf
    x[1, 5] = np.nan
    x[2] = -0.0
    x[3] = np.nan
    ref = orf.absmax(x, axis=1)
    assert_bits(ref, np.array([3.0, np.inf, 0.0, 0.0], f32))
    assert_bits(_absmax_rows(dev(x), 4, n), ref, f"special values n={n}")


# ----------------------------------------------------------- tmr_pixel_absmax
@pytest.mark.parametrize("S,C,HW", [(1, 1, 1), (2, 3, 5), (3, 9, 64), (2, 17, 65), (1, 8, 130), (5, 33, 63)])
def test_pixel_absmax_planted_maximum(S, C, HW):
    """C below 8 and not a multiple of 8 (the last channel group), 64-pixel
    blocks that straddle two samples; the negative maximum of every pixel at
    channel 0, at channel C - 1 and at a random channel per pixel."""
    rng = np.random.default_rng(S * 1009 + C * 101 + HW)
    base = rng.uniform(-0.5, 0.5, (S, C, HW)).astype(f32)
    peak = np.broadcast_to(-(1.0 + np.arange(HW) % 5).astype(f32), (S, 1, HW))
    for name, ch in (("first", np.zeros((S, 1, HW), np.int64)), ("last", np.full((S, 1, HW), C - 1)),
                     ("random", rng.integers(C, size=(S, 1, HW)))):
        x = base.copy()
        np.put_along_axis(x, ch, peak, axis=1)
        ref = orf.absmax(x, axis=1)
        assert np.array_equal(ref, -peak[:, 0])
        xd, out = dev(x), junk_f(S, HW)
        call("tmr_pixel_absmax", ptr(xd), S, C, HW, ptr(out), stream())
        assert_bits(host(out), ref, f"pixel_absmax {S}x{C}x{HW} max at the {name} channel")
    x = base.copy()
    x[:, C - 1, 0] = np.nan
    x[0, 0, HW - 1] = -np.inf
    xd, out = dev(x), junk_f(S, HW)
    call("tmr_pixel_absmax", ptr(xd), S, C, HW, ptr(out), stream())
    assert_bits(host(out), orf.absmax(x, axis=1), "pixel_absmax NaN / inf")


# ------------------------------------------------------------ tmr_scale_merge
def _merge_cases():
    rng = np.random.default_rng(9)
    ui = np.array([2, 0, 3, 0, 2, 2, 3, 0, 3], np.int32)  # unsorted; image 1 has no unit
    um = np.array([3.0, 0.5, 9.0, 4.0, 8.0, 1.0, 2.0, 0.25, 6.0], f32)
    im = np.array([0.5, 7.0, 100.0, 0.01], f32)
    yield "U9", 4, ui, um, im
    ui = rng.integers(0, 3, 600).astype(np.int32)
    um = rng.uniform(0.1, 1.0, 600).astype(f32)
    ui[[599, 300, 5]] = [0, 1, 2]  # each image's maximum: past 512, past 256, in the first 256
    um[[599, 300, 5]] = [5.0, 6.0, 7.0]
    yield "U600", 3, ui, um, np.array([9.0, 0.5, 0.0], f32)


@pytest.mark.parametrize("name,B,ui,um,im", list(_merge_cases()), ids=lambda v: v if isinstance(v, str) else None)
def test_scale_merge(name, B, ui, um, im):
    """Unsorted unit_image, an image without units, units past the block's
    first 256; img_max and out_img each NULL or given."""
    U = len(ui)
    imd, umd, uid = dev(im), dev(um), dev(ui)
    for with_img in (True, False):
        ref_img, ref_unit = orf.scale_merge(im if with_img else None, um, ui, B)
        for with_out in (True, False):
            out_img, out_unit = junk_f(B), junk_f(U)
            call("tmr_scale_merge", ptr(imd) if with_img else None, ptr(umd), ptr(uid), B, U,
                 ptr(out_img) if with_out else None, ptr(out_unit), stream())
            what = f"{name} img_max={with_img} out_img={with_out}"
            assert_bits(host(out_unit), ref_unit, what + " out_unit")
            assert_bits(host(out_img), ref_img if with_out else np.full(B, 1e30, f32), what + " out_img")


# -------------------------------------------------------- tmr_split_fold_proj
@pytest.mark.parametrize("N,Cw,Cp,Cin,ks", [(5, 7, 4, 3, 1), (5, 7, 4, 3, 3), (130, 24, 24, 33, 3)])
def test_fold_proj_bitexact(N, Cw, Cp, Cin, ks):
    """fp64 sums over k ascending, one rounding: exact against the restatement."""
    rng = np.random.default_rng(N + Cin)
    wd = rng.standard_normal((N, Cw, ks, ks)).astype(f32)
    pw = rng.standard_normal((Cp, Cin)).astype(f32)
    pb = rng.standard_normal(Cp).astype(f32)
    wdd, pwd, pbd, out = dev(wd), dev(pw), dev(pb), junk_f(N, Cin + 1, ks, ks)
    call("tmr_split_fold_proj", ptr(wdd), N, Cw, Cp, ks, ptr(pwd), ptr(pbd), Cin, ptr(out), stream())
    assert_bits(host(out), orf.fold_proj_ref(wd, Cp, pw, pb), "fold_proj")


# ------------------------------------------------------------ tmr_split_wpack
@pytest.mark.parametrize("N,C0,C1,ks", [(8, 24, 0, 1), (72, 40, 0, 3), (136, 24, 40, 3), (130, 0, 33, 5),
                                        (16, 12, 0, 7)])
def test_wpack_records_bitexact(N, C0, C1, ks):
    """Weight records of one or two sources, every precision, weights at
    3e-5, 1 and 7e4 and an all-zero tensor; wmax from numpy."""
    rng = np.random.default_rng(N * 7 + ks)
    w0 = rng.standard_normal((N, C0 + C1, ks, ks)).astype(f32)
    for mag in (3e-5, 1.0, 7e4, 0.0):
        # the all-zero tensor is +0 throughout: the sign of a -0.0 input's terms
        # is unspecified (test_pack_negative_zero_inputs)
        w = (w0 * f32(mag)).astype(f32) if mag else np.zeros_like(w0)
        wmax = orf.absmax(w)
        wd, md = dev(w), dev(np.array([wmax], f32))
        for prec in PRECS:
            n = size("wpack", N, C0, C1, ks, prec)
            assert n == orf.wpack_bytes(N, C0, C1, ks, prec)
            out = junk_b(n)
            call("tmr_split_wpack", ptr(wd), N, C0, C1, ks, prec, None if prec == orf.BF16 else ptr(md), ptr(out),
                 stream())
            assert_words(host(out), orf.wrecords_ref(w, C0, C1, prec, wmax),
                         f"wpack {orf.PREC_NAMES[prec]} x{mag}")


def _zero_sign_free(words):
    w = np.asarray(words).view(np.uint16).ravel().copy()
    w[w == 0x8000] = 0
    return w


def test_pack_negative_zero_inputs():
    """-0.0 inputs among ordinary ones: every non-zero term is exact and the
    -0.0 inputs' terms are zero; their sign alone is free (include/tmr.h:
    the compiler may fuse scale and conversion into a multiply-add with a +0
    addend for some elements of a piece)."""
    rng = np.random.default_rng(21)
    N, C0, ks = 9, 40, 3
    w = rng.standard_normal((N, C0, ks, ks)).astype(f32)
    w[rng.random(w.shape) < 0.3] = -0.0
    x = rng.standard_normal((2, 33, 7, 9)).astype(f32)
    x[rng.random(x.shape) < 0.3] = -0.0
    wmax, xmax = orf.absmax(w), orf.absmax(x)
    wd, xd, wm, xm = dev(w), dev(x), dev(np.array([wmax], f32)), dev(np.array([xmax], f32))
    for prec in PRECS:
        out = junk_b(size("wpack", N, C0, 0, ks, prec))
        call("tmr_split_wpack", ptr(wd), N, C0, 0, ks, prec, ptr(wm), ptr(out), stream())
        assert_words(_zero_sign_free(host(out)), _zero_sign_free(orf.wrecords_ref(w, C0, 0, prec, wmax)),
                     f"wpack -0.0 {orf.PREC_NAMES[prec]}")
        out = junk_b(size("xpack", 2, 33, 7, 9, ks, prec))
        call("tmr_split_xpack", ptr(xd), 2, 33, 7, 9, 0, ks, prec, ptr(xm), 0, ptr(out), stream())
        ref = orf.xrecords_ref(torch.from_numpy(x), ks, orf.PREC_NAMES[prec], float(xmax)).numpy()
        assert_words(_zero_sign_free(host(out)), _zero_sign_free(ref), f"xpack -0.0 {orf.PREC_NAMES[prec]}")


# ----------------------------------------- tmr_split_xpack: upsample and ones
@pytest.mark.parametrize("up", [XPACK_UPSAMPLE, XPACK_ONES, XPACK_UPSAMPLE | XPACK_ONES])
@pytest.mark.parametrize("S,Cin,Hin,Win,ks", [(2, 31, 5, 9, 3), (1, 32, 8, 16, 1), (2, 40, 7, 6, 5)])
def test_xpack_upsample_ones_bitexact(S, Cin, Hin, Win, ks, up):
    """Records of cat[up2x(f) or f, ones] (the bit-exact fma form of the
    oracle), padding ring included; the ones channel is zero in the ring.
    Scale sources from numpy; with the ones channel they respect the header's
    lower bound 0.25 -- the quiet second sample sits exactly on it, so its ones
    channel is 2^15."""
    rng = np.random.default_rng(S * 1000 + Cin * 10 + ks)
    f = rng.standard_normal((S, Cin, Hin, Win)).astype(f32)
    f *= np.array([1.0, 2.0 ** -12][:S], f32)[:, None, None, None]
    v = np.stack([oracle.upsample2x(x) for x in f]) if up & XPACK_UPSAMPLE else f
    per = orf.absmax(v.reshape(S, -1), axis=1)
    if up & XPACK_ONES:
        per = np.maximum(per, f32(0.25))
        assert S == 1 or per[1] == f32(0.25)
        v = np.concatenate([v, np.ones((S, 1) + v.shape[2:], f32)], 1)
    C, H, W = v.shape[1:]
    fd, vt = dev(f), torch.from_numpy(v)
    for mode, xmax in ((0, np.array([per.max()], f32)), (1, per)):
        xd = dev(xmax)
        for prec in PRECS:
            n = size("xpack", S, C, H, W, ks, prec)
            out = junk_b(n)
            call("tmr_split_xpack", ptr(fd), S, Cin, Hin, Win, up, ks, prec, ptr(xd), mode, ptr(out), stream())
            ref = orf.xrecords_ref(vt, ks, orf.PREC_NAMES[prec], xmax if mode else float(xmax[0]))
            assert_words(host(out), ref.numpy(), f"xpack up={up} {orf.PREC_NAMES[prec]} xmax_per_sample={mode}")
            if up & XPACK_ONES and prec != orf.BF16:  # finite, as the bound promises
                assert np.isfinite(ref.numpy().view(np.float16).astype(f32)).all()


# --------------------------------------------------------- tmr_template_split
TSPLIT_SIZES = [(1, 1), (3, 3), (5, 9), (7, 15), (15, 7), (17, 17), (13, 29), (31, 1), (1, 31), (31, 31)]


@pytest.mark.parametrize("order", ["listed", "shuffled"])
@pytest.mark.parametrize("prec", PRECS)
def test_template_split_fragments_and_exponents(prec, order):
    """Window fragments (hi; lo for the 3-term split) and exponents of ten
    units in two orders -- row_offset is then not monotone in template size --
    with channel magnitudes 2^-20, 1 and 2^20 and all-zero channels (exponent
    0).  The lo slots of the one-term precisions are unspecified and skipped."""
    C = 3
    sizes = list(TSPLIT_SIZES)
    if order == "shuffled":
        sizes = [sizes[i] for i in (9, 2, 7, 0, 5, 8, 1, 6, 3, 4)]
    rng = np.random.default_rng(12)
    U = len(sizes)
    units = np.zeros(U, _lib.UNIT_DTYPE)
    tmpls, off, rows = [], 0, 0
    for u, (h, w) in enumerate(sizes):
        t = rng.standard_normal((C, h, w)).astype(f32)
        for c in range(C):
            t[c] *= f32(2.0 ** (-20, 0, 20)[(u + c) % 3])
        if u % 3 == 1:
            t[1] = 0.0
        tmpls.append(t)
        units[u]["ht"], units[u]["wt"] = h, w
        units[u]["tmpl_offset"], units[u]["row_offset"] = off, rows
        off += C * h * w
        rows += orf.window_count(h, w)
    nbytes = size("template_split", U, C, rows)
    assert nbytes == orf.template_split_bytes(U, C, rows)
    out = junk_b(nbytes)
    td = dev(np.concatenate([t.ravel() for t in tmpls]))
    ud = dev(units.view(np.uint8))
    call("tmr_template_split", ptr(td), ptr(ud), U, C, rows, prec, ptr(out), stream())
    got = host(out)
    frags, known, exps = orf.template_split_ref(tmpls, units["row_offset"], rows, prec)
    nf = C * rows * 2
    assert known[0::2].all() and known[1::2].all() == (prec == orf.F16X3)
    assert (exps[1::3, 1] == 0).all() and len(set(exps.ravel().tolist())) > 3
    assert np.array_equal(got[nf * 1024:].view(np.int32).reshape(U, C), exps), "exponents"
    gf = got[:nf * 1024].view(np.uint16).reshape(nf, 64, 8)
    assert_words(gf[0::2], frags[0::2], f"hi fragments {orf.PREC_NAMES[prec]}")
    if prec == orf.F16X3:
        assert_words(gf[1::2], frags[1::2], "lo fragments")


# ----------------------------------------------------------- tmr_heads_reduce
def _partials(rng, NT, U, H, W):
    p = rng.standard_normal((NT, 5, U, H, W)).astype(f32)
    p[:, :, 0, 0, 0] = -0.0  # an exactly zero sum: +0 from the +0 start
    return p


@pytest.mark.parametrize("tile_n", [128, 64])
@pytest.mark.parametrize("U,H,W", [(1, 1, 1), (3, 5, 7), (2, 16, 33)])
def test_heads_reduce_bitexact(U, H, W, tile_n):
    """N = 200 in tiles of 128 (2 tiles) and 64 (4 tiles), a non-zero bias;
    with b, and with b = NULL over partials whose regression planes are NaN."""
    N = 200
    NT = -(-N // tile_n)
    rng = np.random.default_rng(U * 31 + W + tile_n)
    p, hb = _partials(rng, NT, U, H, W), rng.standard_normal(5).astype(f32)
    hb[0] = -0.0  # (+0 + -0 partials) + -0 = +0: a sum not started from +0 would give -0
    ro, rb = orf.heads_reduce_ref(p, hb)
    assert rb[0, 0, 0, 0] == 0 and not np.signbit(rb[0, 0, 0, 0])
    pd, hbd, o, b = dev(p), dev(hb), junk_f(U, 1, H, W), junk_f(U, 4, H, W)
    call("tmr_heads_reduce", ptr(pd), N, tile_n, U, H, W, ptr(hbd), ptr(o), ptr(b), stream())
    assert_bits(host(o), ro, "o")
    assert_bits(host(b), rb, "b")
    pn = p.copy()
    pn[:, :4] = np.nan
    pnd, o2 = dev(pn), junk_f(U, 1, H, W)
    call("tmr_heads_reduce", ptr(pnd), N, tile_n, U, H, W, ptr(hbd), ptr(o2), None, stream())
    assert_bits(host(o2), orf.heads_reduce_ref(pn, hb, with_b=False)[0], "o with b = NULL")
    assert_bits(host(o2), ro, "o with b = NULL equals o with b")


def test_heads_reduce_tile_window():
    """A tile window (first 1, count 2) of a 4-tile launch: partials + first *
    5*U*H*W and N = 128 * count; the tiles outside the window hold NaN."""
    U, H, W, first, count = 3, 5, 7, 1, 2
    rng = np.random.default_rng(3)
    p, hb = _partials(rng, 4, U, H, W), rng.standard_normal(5).astype(f32)
    p[0] = p[3] = np.nan
    pd = dev(p)
    win = pd[first:first + count]
    assert win.data_ptr() == pd.data_ptr() + 4 * first * 5 * U * H * W
    ro, rb = orf.heads_reduce_ref(p[first:first + count], hb)
    hbd, o, b = dev(hb), junk_f(U, 1, H, W), junk_f(U, 4, H, W)
    call("tmr_heads_reduce", ptr(win), 128 * count, 128, U, H, W, ptr(hbd), ptr(o), ptr(b), stream())
    assert_bits(host(o), ro, "o over a window")
    assert_bits(host(b), rb, "b over a window")


# ------------------------------------------------------------- tmr_upsample2x
def test_upsample2x_more_planes_than_one_launch():
    """65537 planes: the plane loop's second launch (grid z holds 65535)."""
    BC, Hin, Win = 65537, 2, 3
    f = np.random.default_rng(5).standard_normal((BC, Hin, Win)).astype(f32)
    fd, out = dev(f), junk_f(BC, 2 * Hin, 2 * Win)
    call("tmr_upsample2x", ptr(fd), BC, Hin, Win, ptr(out), stream())
    assert_bits(host(out), oracle.upsample2x(f), "upsample2x over 65537 planes")
