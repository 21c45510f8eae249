"""The regression heads at the peaks only: tmr_split_conv_points, the dense
launch's channel-tile window and the two-phase peak finder, each bit for bit
against the dense fused path; then TMREngine.detect with box_at_peaks
"always" / "never" / "auto".

Every comparison here is bit-equality (no tolerance): the points kernel
issues the dense kernel's chain of operations per output element.
"""
import numpy as np
import pytest
import torch

import tmr_amd
from tmr_amd import host, synth
from tmr_amd._lib import (PEAK_DTYPE, POINTS_TILE, PREC_CODES, SPLIT_INIT_BCAST, SPLIT_INIT_BF16,
                          SPLIT_OUT_BF16, SPLIT_TILED_INIT, SPLIT_TILED_OUT, SPLIT_XMAX_PER_UNIT, call, ptr,
                          size, split_tile_window, stream)

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
# 17 x 33: partial 16 x 32 tiles both ways; N = 256: decoder_b || decoder_o of
# one 128-channel tile each; C1 = 40: a partial 32-channel chunk
B, U, C0, C1, N, H, W = 2, 3, 24, 40, 256, 17, 33
HW = H * W
UI = np.array([1, 0, 1], np.int32)
SENTINEL = 12345.0


def cuda(x):
    return torch.as_tensor(x).to(DEV)


def bits_equal(a, b):
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.fixture(scope="module")
def data():
    g = torch.Generator().manual_seed(7)
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    hw = torch.zeros(N, 5)
    hw[:128, 0:4] = rn(128, 4)   # ltrbs_head over decoder_b's tile
    hw[128:, 4] = rn(128)        # objectness_head over decoder_o's tile
    d = dict(x0=rn(B, C0, H, W), x1=rn(U, C1, H, W), w=rn(N, C0 + C1, 3, 3) * 0.02, bias=rn(N) * 0.1,
             hw=hw, hb=rn(5), one=rn(1, 8, H, W), wone=rn(N, 8, 3, 3) * 0.02)
    d = {k: cuda(v) for k, v in d.items()}
    # candidate rows as the finder leaves them: unit 0 every pixel (8 whole tiles
    # + 49), in a shuffled order; unit 1 one point (the last pixel); unit 2 none
    perm = torch.randperm(HW, generator=g).numpy().astype(np.int32)
    box = np.zeros((U * HW, 4), np.int32)
    box[:HW, 0] = perm
    box[HW, 0] = HW - 1
    d["counts"] = np.array([HW, 1, 0])
    d["box"] = cuda(box).view(torch.float32)
    d["listed"] = [np.arange(HW), np.array([HW - 1]), np.zeros(0, np.int64)]
    return d


def _operands(d, prec, form, x1=None, ui=UI):
    """(args, acc_init, flags) of the heads launch.  form "tiled": the f_TM
    half over a per-image slab from a store launch of the fp half (bf16 slab
    under "bf16" when slab16); "bcast": both sources in one launch over a
    broadcast plane (the E = 1 path)."""
    from tmr_amd.operands import absmax, absmax_rows, pack_split_w, pack_split_x, scale_merge
    pc = PREC_CODES[prec]
    x1 = d["x1"] if x1 is None else x1
    nu = x1.shape[0]
    uid = cuda(np.asarray(ui, np.int32))
    scaled = prec != "bf16"
    tm_max = absmax_rows(x1) if scaled else None
    xpu = SPLIT_XMAX_PER_UNIT if scaled else 0
    zero = torch.zeros(N, device=DEV)
    keep = [uid, tm_max, zero]
    if form in ("tiled", "tiled16"):
        w0, w1 = d["w"][:, :C0].contiguous(), d["w"][:, C0:].contiguous()
        wp0, wm0 = pack_split_w(w0, C0, prec)
        wp1, wm1 = pack_split_w(w1, 0, prec)
        xm0 = absmax_rows(d["x0"]) if scaled else None
        xp0 = pack_split_x(d["x0"], 3, prec, xm0)
        slab = torch.empty(size("acc", B, N, H, W), device=DEV)
        s16 = form == "tiled16"
        call("tmr_split_conv", ptr(xp0), C0, None, None, 0, B, H, W, 3, pc, ptr(wp0), ptr(wm0), ptr(xm0),
             ptr(zero), N, 0, None, None, ptr(slab), SPLIT_TILED_OUT | xpu | (SPLIT_OUT_BF16 if s16 else 0), stream())
        xp1 = pack_split_x(x1, 3, prec, tm_max)
        args = (None, 0, ptr(uid), ptr(xp1), C1, nu, H, W, 3, pc, ptr(wp1), ptr(wm1), ptr(tm_max),
                ptr(d["bias"]), N, 1, ptr(d["hw"]))
        keep += [wp0, wp1, wm1, xp1, slab]
        return args, slab, SPLIT_TILED_INIT | xpu | (SPLIT_INIT_BF16 if s16 else 0), keep
    wp, wm = pack_split_w(d["w"], C0, prec)
    wpo, wmo = pack_split_w(d["wone"], 8, prec)
    om = absmax(d["one"]) if scaled else None
    plane = torch.empty(size("acc", 1, N, H, W), device=DEV)
    call("tmr_split_conv", ptr(pack_split_x(d["one"], 3, prec, om)), 8, None, None, 0, 1, H, W, 3, pc, ptr(wpo),
         ptr(wmo), ptr(om), ptr(zero), N, 0, None, None, ptr(plane), SPLIT_TILED_OUT, stream())
    xs0, xm1 = scale_merge(absmax_rows(d["x0"]), tm_max, uid, B) if scaled else (None, None)
    xp0, xp1 = pack_split_x(d["x0"], 3, prec, xs0), pack_split_x(x1, 3, prec, xm1)
    args = (ptr(xp0), C0, ptr(uid), ptr(xp1), C1, nu, H, W, 3, pc, ptr(wp), ptr(wm), ptr(xm1), ptr(d["bias"]), N, 1,
            ptr(d["hw"]))
    keep += [wp, wm, xp0, xp1, xm1, plane]
    return args, plane, SPLIT_TILED_INIT | SPLIT_INIT_BCAST | xpu, keep


def _dense(d, args, init, flags, window=0):
    nu = args[5]
    part = torch.full((size("heads_partials", N, nu, H, W),), float("nan"), device=DEV)
    call("tmr_split_conv", *args, ptr(init), ptr(part), flags | window, stream())
    return part


def _dense_ob(d, args, init, flags):
    nu = args[5]
    part = _dense(d, args, init, flags)
    o, b = torch.empty((nu, 1, H, W), device=DEV), torch.empty((nu, 4, H, W), device=DEV)
    call("tmr_heads_reduce", ptr(part), N, 128, nu, H, W, ptr(d["hb"]), ptr(o), ptr(b), stream())
    return o.cpu().numpy(), b.cpu().numpy()


def _points(d, args, init, flags, counts, box):
    nu = args[5]
    tiles = host.point_tiles(counts, POINTS_TILE)
    b = torch.full((nu, 4, H, W), SENTINEL, device=DEV)
    td = cuda(tiles.reshape(-1))
    call("tmr_split_conv_points", *args, ptr(d["hb"]), ptr(init), ptr(box), ptr(td), len(tiles), ptr(b),
         flags | split_tile_window(0, 1), stream())
    torch.cuda.synchronize()
    return b.cpu().numpy()


FORMS = [("fp32", "tiled"), ("bf16", "tiled"), ("bf16", "tiled16"), ("f16", "tiled"),
         ("fp32", "bcast"), ("bf16", "bcast"), ("f16", "bcast")]


@pytest.mark.parametrize("prec,form", FORMS)
def test_points_equal_dense_bits(data, prec, form):
    """b at every listed pixel is the dense launch + tmr_heads_reduce's, bit for
    bit; every other element of b is untouched."""
    d = data
    args, init, flags, _keep = _operands(d, prec, form)
    _, want = _dense_ob(d, args, init, flags)
    got = _points(d, args, init, flags, d["counts"], d["box"])
    assert np.isfinite(want).all()
    for u in range(U):
        listed = np.zeros(HW, bool)
        listed[d["listed"][u]] = True
        g, w_ = got[u].reshape(4, HW), want[u].reshape(4, HW)
        assert bits_equal(g[:, listed], w_[:, listed]), (prec, form, u)
        assert (g[:, ~listed] == SENTINEL).all(), (prec, form, u)


@pytest.mark.parametrize("prec", ["fp32", "bf16", "f16"])
def test_points_unit_scaled_alone_or_in_batch(data, prec):
    """Per-unit activation scales: unit 0 scaled by 2^20 gives the same bits
    in the batch as when it runs alone."""
    d = data
    x1 = d["x1"].clone()
    x1[0] *= 2.0 ** 20
    counts = np.array([HW, 0, 0])
    args, init, flags, _k = _operands(d, prec, "tiled", x1=x1)
    batch = _points(d, args, init, flags, counts, d["box"])
    # alone: image UI[0]'s slab must sit where unit_image points, so keep both images' slab
    args1, init1, flags1, _k1 = _operands(d, prec, "tiled", x1=x1[:1].contiguous(), ui=UI[:1])
    alone = _points(d, args1, init1, flags1, counts[:1], d["box"][:HW].contiguous())
    assert bits_equal(batch[0], alone[0])
    _, want = _dense_ob(d, args, init, flags)
    assert bits_equal(batch[0], want[0])


@pytest.mark.parametrize("prec,form", [("fp32", "tiled"), ("bf16", "tiled16"), ("f16", "bcast")])
def test_tile_window_objectness_equals_full_launch(data, prec, form):
    """A launch over the second channel tile only (decoder_o's) + the reduce
    over that tile gives the full launch's objectness bit for bit, and writes
    no other tile's partials; the first tile alone gives the full launch's b."""
    d = data
    args, init, flags, _keep = _operands(d, prec, form)
    o_full, b_full = _dense_ob(d, args, init, flags)
    tile = 5 * U * HW
    part = _dense(d, args, init, flags, split_tile_window(1, 1))
    assert torch.isnan(part[:tile]).all() and not torch.isnan(part[tile:2 * tile]).any()
    o = torch.empty((U, 1, H, W), device=DEV)
    call("tmr_heads_reduce", ptr(part[tile:]), 128, 128, U, H, W, ptr(d["hb"]), ptr(o), None, stream())
    assert bits_equal(o.cpu().numpy(), o_full)
    part = _dense(d, args, init, flags, split_tile_window(0, 1))
    assert torch.isnan(part[tile:2 * tile]).all()
    b = torch.empty((U, 4, H, W), device=DEV)
    call("tmr_heads_reduce", ptr(part), 128, 128, U, H, W, ptr(d["hb"]), ptr(o), ptr(b), stream())
    assert bits_equal(b.cpu().numpy(), b_full)
    with pytest.raises(tmr_amd.TMRError):  # a window past the last tile
        _dense(d, args, init, flags, split_tile_window(1, 2))


def test_points_refuses_what_it_does_not_build(data):
    d = data
    args, init, flags, _keep = _operands(d, "fp32", "tiled")
    td = cuda(host.point_tiles(d["counts"], POINTS_TILE).reshape(-1))
    b = torch.zeros((U, 4, H, W), device=DEV)
    with pytest.raises(tmr_amd.TMRError):  # plain-layout initial values
        call("tmr_split_conv_points", *args, ptr(d["hb"]), ptr(init), ptr(d["box"]), ptr(td), 1, ptr(b),
             flags & ~SPLIT_TILED_INIT, stream())
    a5 = args[:8] + (5,) + args[9:]
    with pytest.raises(tmr_amd.TMRError):  # kernel size 5 belongs to the dense launch
        call("tmr_split_conv_points", *a5, ptr(d["hb"]), ptr(init), ptr(d["box"]), ptr(td), 1, ptr(b), flags,
             stream())


def test_find_then_decode_equals_one_call():
    """TMR_PEAKS_FIND_ONLY + TMR_PEAKS_DECODE_ONLY = the one-call finder, bit
    for bit, on a random map with plateaus and a NaN; for few units (the
    fused-decode form) and many."""
    rng = np.random.default_rng(3)
    for nu in (3, 11):
        Hm, Wm = 23, 37
        o = rng.normal(size=(nu, 1, Hm, Wm)).astype(np.float32)
        o[:, :, 4:7, 5:9] = 1.5          # plateaus
        o[0, 0, 10, 10:14] = 2.0
        o[1, 0, 12, 20] = np.nan
        reg = (rng.normal(size=(nu, 4, Hm, Wm)) * 0.3).astype(np.float32)
        boxes = np.stack([synth.exemplar_box(50 + u, Hm, Wm, 3, 9) for u in range(nu)])
        params = host.peak_params(boxes, Hm, Wm, 0.5, True, False, False)
        params["thr"][nu - 1] = 2.0      # no candidate: the dummy row
        od, rd = cuda(o), cuda(reg)
        one = tmr_amd.TMREngine.peaks(od, rd, params, want_prob=False)
        found = tmr_amd.TMREngine.peaks(od, None, params, want_prob=False, phase="find")
        cnt = found[3].cpu().numpy()
        pix = found[1].view(torch.int32).cpu().numpy().reshape(nu, Hm * Wm, 4)[:, :, 0]
        prob = 1.0 / (1.0 + np.exp(-o[:, 0].astype(np.float64)))
        for u in range(nu - 1):  # the rows hold row-major pixel indices of candidates
            p = pix[u, :cnt[u]]
            assert (np.diff(p) > 0).all() and (prob[u].reshape(-1)[p] >= 0.5 - 1e-6).all()
        two = tmr_amd.TMREngine.peaks(od, rd, params, want_prob=False, phase="decode", found=found[:4])
        torch.cuda.synchronize()
        c1 = one[3].cpu().numpy()
        assert np.array_equal(c1, cnt) and cnt[nu - 1] == 0 and cnt[:nu - 1].min() > 0
        for a, b_, width in ((one[0], two[0], 2), (one[1], two[1], 4), (one[2], two[2], 2)):
            a, b_ = a.cpu().numpy().reshape(nu, Hm * Wm, width), b_.cpu().numpy().reshape(nu, Hm * Wm, width)
            for u in range(nu):
                n = max(int(c1[u]), 1)
                assert np.array_equal(a[u, :n].view(np.uint32), b_[u, :n].view(np.uint32)), (nu, u)


# ---------------------------------------------------------------- engine
@pytest.fixture(scope="module")
def model():
    P = synth.reference_state_dict(0)
    return {k: v.to(DEV) for k, v in P.items()}, cuda(synth.sam_features(1000, 2, 256, 16, 16))


def _detect(Pd, feats, ex, prec, route, thr):
    eng = tmr_amd.TMREngine(Pd, tmr_amd.PathConfig(precision=prec))
    eng.use_graphs = False
    eng.box_at_peaks = route
    out = eng.detect(feats, ex, cls_ths=thr, iou_threshold=0.5)
    torch.cuda.synchronize()
    return [[t.cpu().numpy() for t in lst] for lst in out], eng


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("E", [3, 1])
def test_detect_routes_agree(model, prec, E):
    """detect() with the regression at the peaks ("always"), fused and dense
    ("never") and "auto" returns the same L, Bx, R bit for bit: at a threshold
    that gives a few percent of the pixels, at one that leaves a unit without
    a candidate (its dummy row), and with a tiny exemplar at a low threshold,
    where every pixel is a candidate and "auto" takes the dense tiles."""
    Pd, feats = model
    ex, _ = synth.exemplar_set(2000, 2, E, 32, 32, 3, 9)
    tiny = ex.copy()
    tiny[..., 2:] = tiny[..., :2] + 1e-3  # a 1x1 adaptive mask: every pixel is its own maximum
    never0, e0 = _detect(Pd, feats, ex, prec, "never", 0.1)
    assert e0.last_box_route is None
    # a threshold between the units' best peaks: some unit keeps none
    eng = tmr_amd.TMREngine(Pd, tmr_amd.PathConfig(precision=prec))
    r = eng.forward_units(feats, np.repeat(np.arange(2), E), ex.reshape(-1, 4))
    top = torch.sigmoid(r["o"].double()).amax(dim=(1, 2, 3)).cpu().numpy()
    thr_gap = float(np.sort(top)[0] + np.sort(top)[1]) / 2 if len(top) > 1 else 0.5
    assert np.sort(top)[0] < thr_gap < np.sort(top)[1]
    for exs, thr, want_auto in ((ex, 0.1, "points"), (ex, thr_gap, "points"), (tiny, 1e-6, "dense")):
        never, _ = _detect(Pd, feats, exs, prec, "never", thr)
        for route in ("always", "auto"):
            got, e = _detect(Pd, feats, exs, prec, route, thr)
            assert e.last_box_route == ("points" if route == "always" else want_auto), (route, thr)
            if e.last_box_route == "points":
                assert e.last_points_flops >= e.last_points * 2.0 * 1024 * 512 * 9
            for a, b_ in zip(got, never):
                assert len(a) == len(b_) == 2
                for x, y in zip(a, b_):
                    assert bits_equal(x, y), (route, thr, E, prec)
        if want_auto == "dense":
            assert e.last_points > e.BOX_POINTS_CROSSOVER[prec] * 2 * E * 32 * 32
        if thr == thr_gap:  # the empty unit's dummy row went through the NMS
            assert sum(len(x) for x in never[0]) >= 1
