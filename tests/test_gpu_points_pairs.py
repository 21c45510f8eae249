"""tmr_split_conv_points where a block takes two host tiles and a window of
more than four channel tiles runs the K loop twice: windows of 1, 3, 4, 5 and 8
decoder_b tiles, tile pairs that cross units and images, and degenerate lists.

The expected values are always the dense tmr_split_conv over decoder_b's
window + tmr_heads_reduce at the listed pixels, compared bit for bit (no
tolerance: the points kernel issues the dense kernel's chain of operations per
output element); every unlisted element of b must still hold the sentinel.
The dense reference of an operand set is computed once and shared.

Every case runs the way tests/test_gpu_guarded.py runs its routes: unpatched,
with every allocation poisoned with zero bytes and with 0xFF bytes, the
outputs bit-identical across the three runs and no guard byte written.

Shapes: a 17 x 33 map (partial dense 16 x 32 tiles both ways), C0 = C1 = 64,
three images, four units (unit 3's f_TM scaled by 2^10: per-unit scales),
N = 128 (nb + 1): decoder_b's nb tiles || decoder_o's one.
"""
import numpy as np
import pytest
import torch

import guarded_alloc as ga
import test_gpu_guarded as TG
from test_gpu_points import SENTINEL, bits_equal
from tmr_amd._lib import (POINTS_TILE, PREC_CODES, SPLIT_INIT_BCAST, SPLIT_INIT_BF16, SPLIT_OUT_BF16,
                          SPLIT_TILED_INIT, SPLIT_TILED_OUT, SPLIT_XMAX_PER_UNIT, call, ptr, size,
                          split_tile_window, stream)
from tmr_amd import host

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
B, U, C0, C1, H, W = 3, 4, 64, 64, 17, 33
HW = H * W
UI = np.array([2, 0, 1, 0], np.int32)
# candidates per unit of the pair cases: 64 + 3, 1, none, 64 + 64 + 17
PAIR_COUNTS = np.array([POINTS_TILE + 3, 1, 0, 2 * POINTS_TILE + 17])

_INPUTS = {}  # nb -> host tensors
_WANT = {}    # (nb, prec, form) -> dense b [U][4][H][W]


def _inputs(nb):
    """Host tensors of the window of nb decoder_b tiles, and the candidate
    rows as the finder leaves them: unit 0 every pixel in a shuffled order (8
    whole tiles + 49), unit 1 the last pixel, unit 2 none, unit 3 145 pixels of
    another order."""
    if nb not in _INPUTS:
        N = 128 * (nb + 1)
        g = torch.Generator().manual_seed(100 + nb)
        rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
        hw = torch.zeros(N, 5)
        hw[:128 * nb, 0:4] = rn(128 * nb, 4)   # ltrbs_head over decoder_b's tiles
        hw[128 * nb:, 4] = rn(128)             # objectness_head over decoder_o's tile
        x1 = rn(U, C1, H, W)
        x1[3] *= 2.0 ** 10
        d = dict(N=N, x0=rn(B, C0, H, W), x1=x1, w=rn(N, C0 + C1, 3, 3) * 0.02, bias=rn(N) * 0.1, hw=hw, hb=rn(5),
                 one=rn(1, 8, H, W), wone=rn(N, 8, 3, 3) * 0.02)
        box = np.zeros((U * HW, 4), np.int32)
        box[:HW, 0] = torch.randperm(HW, generator=g).numpy()
        box[HW, 0] = HW - 1
        box[3 * HW:3 * HW + PAIR_COUNTS[3], 0] = torch.randperm(HW, generator=g).numpy()[:PAIR_COUNTS[3]]
        d["box"] = box
        _INPUTS[nb] = d
    return _INPUTS[nb]


def _operands(a, nb, prec, form):
    """tests/test_gpu_points.py's _operands at this file's shapes, the inputs
    placed through the allocator context `a`: (args, acc_init, flags, keep)."""
    from tmr_amd.operands import absmax, absmax_rows, pack_split_w, pack_split_x, scale_merge
    d = _inputs(nb)
    N, pc = d["N"], PREC_CODES[prec]
    t = {k: a.place(d[k]) for k in ("x0", "x1", "w", "bias", "hw", "hb", "one", "wone")}
    uid = a.place(UI)
    scaled = prec != "bf16"
    tm_max = absmax_rows(t["x1"]) if scaled else None
    xpu = SPLIT_XMAX_PER_UNIT if scaled else 0
    zero = torch.zeros(N, device=DEV)
    keep = [t, uid, tm_max, zero]
    if form in ("tiled", "tiled16"):
        w0, w1 = t["w"][:, :C0].contiguous(), t["w"][:, C0:].contiguous()
        wp0, wm0 = pack_split_w(w0, C0, prec)
        wp1, wm1 = pack_split_w(w1, 0, prec)
        xm0 = absmax_rows(t["x0"]) if scaled else None
        xp0 = pack_split_x(t["x0"], 3, prec, xm0)
        slab = torch.empty(size("acc", B, N, H, W), device=DEV)
        s16 = form == "tiled16"
        call("tmr_split_conv", ptr(xp0), C0, None, None, 0, B, H, W, 3, pc, ptr(wp0), ptr(wm0), ptr(xm0),
             ptr(zero), N, 0, None, None, ptr(slab), SPLIT_TILED_OUT | xpu | (SPLIT_OUT_BF16 if s16 else 0), stream())
        xp1 = pack_split_x(t["x1"], 3, prec, tm_max)
        args = (None, 0, ptr(uid), ptr(xp1), C1, U, H, W, 3, pc, ptr(wp1), ptr(wm1), ptr(tm_max),
                ptr(t["bias"]), N, 1, ptr(t["hw"]))
        keep += [wp0, wm0, xm0, xp0, wp1, wm1, xp1, slab]
        return args, slab, SPLIT_TILED_INIT | xpu | (SPLIT_INIT_BF16 if s16 else 0), keep
    assert form == "bcast"
    wp, wm = pack_split_w(t["w"], C0, prec)
    wpo, wmo = pack_split_w(t["wone"], 8, prec)
    om = absmax(t["one"]) if scaled else None
    plane = torch.empty(size("acc", 1, N, H, W), device=DEV)
    xpo = pack_split_x(t["one"], 3, prec, om)
    call("tmr_split_conv", ptr(xpo), 8, None, None, 0, 1, H, W, 3, pc, ptr(wpo), ptr(wmo), ptr(om), ptr(zero), N, 0,
         None, None, ptr(plane), SPLIT_TILED_OUT, stream())
    xs0, xm1 = scale_merge(absmax_rows(t["x0"]), tm_max, uid, B) if scaled else (None, None)
    xp0, xp1 = pack_split_x(t["x0"], 3, prec, xs0), pack_split_x(t["x1"], 3, prec, xm1)
    args = (ptr(xp0), C0, ptr(uid), ptr(xp1), C1, U, H, W, 3, pc, ptr(wp), ptr(wm), ptr(xm1), ptr(t["bias"]), N, 1,
            ptr(t["hw"]))
    keep += [wp, wm, wpo, wmo, om, xpo, xs0, xm1, xp0, xp1, plane]
    return args, plane, SPLIT_TILED_INIT | SPLIT_INIT_BCAST | xpu, keep


def _want(nb, prec, form):
    """The dense launch over decoder_b's window + tmr_heads_reduce: b of every
    pixel, computed once per operand set."""
    key = (nb, prec, form)
    if key not in _WANT:
        with ga.context(None, DEV) as a:
            args, init, flags, keep = _operands(a, nb, prec, form)
            N = _inputs(nb)["N"]
            part = torch.full((size("heads_partials", N, U, H, W),), float("nan"), device=DEV)
            call("tmr_split_conv", *args, ptr(init), ptr(part), flags | split_tile_window(0, nb), stream())
            o, b = torch.empty((U, 1, H, W), device=DEV), torch.empty((U, 4, H, W), device=DEV)
            call("tmr_heads_reduce", ptr(part), 128 * nb, 128, U, H, W, ptr(keep[0]["hb"]), ptr(o), ptr(b), stream())
            torch.cuda.synchronize()
            _WANT[key] = b.cpu().numpy()
            assert np.isfinite(_WANT[key]).all()
    return _WANT[key]


def _points(a, ops, nb, tiles):
    """b (sentinel-filled) after the points launch over the tile list."""
    args, init, flags, keep = ops
    tiles = np.ascontiguousarray(tiles, np.int32).reshape(-1, 3)
    b = torch.full((U, 4, H, W), SENTINEL, device=DEV)
    td = a.place(tiles.reshape(-1) if len(tiles) else np.zeros(3, np.int32))
    box = a.place(_inputs(nb)["box"]).view(torch.float32)
    call("tmr_split_conv_points", *args, ptr(keep[0]["hb"]), ptr(init), ptr(box), ptr(td), len(tiles), ptr(b),
         flags | split_tile_window(0, nb), stream())
    torch.cuda.synchronize()
    return b.cpu().numpy()


def _check(got, want, nb, tiles, what):
    """Listed pixels carry the dense bits, every other element the sentinel."""
    box = _inputs(nb)["box"][:, 0].reshape(U, HW)
    listed = np.zeros((U, HW), bool)
    for u, first, cnt in np.asarray(tiles, np.int64).reshape(-1, 3):
        listed[u, box[u, first:first + cnt]] = True
    for u in range(U):
        g, w_ = got[u].reshape(4, HW), want[u].reshape(4, HW)
        assert bits_equal(g[:, listed[u]], w_[:, listed[u]]), (what, u)
        assert (g[:, ~listed[u]] == SENTINEL).all(), (what, u)
    return int(listed.sum())


def _run(key, nb, prec, form, lists):
    """The points launch over every tile list of `lists` (name -> rows), under
    the guarded allocator's three runs; each against the dense reference."""
    want = _want(nb, prec, form)

    def flow(a):
        ops = _operands(a, nb, prec, form)
        return {name: _points(a, ops, nb, tiles) for name, tiles in lists.items()}

    def verify(out):
        for name, tiles in lists.items():
            _check(out[name], want, nb, tiles, (key, name))

    return TG._guarded_runs(f"points_pairs:{key}", ga.POISON_FF, flow, verify)


WINDOWS = [(1, "fp32", "tiled"), (3, "fp32", "tiled"), (4, "fp32", "tiled"), (5, "fp32", "tiled"),
           (8, "fp32", "tiled"), (5, "bf16", "tiled16"), (5, "f16", "bcast")]


@pytest.mark.parametrize("nb,prec,form", WINDOWS)
def test_window_of_tiles_equals_dense_bits(nb, prec, form):
    """One unit with every pixel listed: 8 whole tiles + 49, an odd tile count
    (the last block takes one tile); nb = 4 and 5 sit on either side of the
    second pass over K, nb = 8 is the full width."""
    tiles = host.point_tiles(np.array([HW, 0, 0, 0]), POINTS_TILE)
    assert len(tiles) == 9 and tiles[-1, 2] == 49
    _run(f"window{nb}-{prec}-{form}", nb, prec, form, {"all": tiles})


def _pair_lists():
    T = POINTS_TILE
    natural = host.point_tiles(PAIR_COUNTS, T)
    assert natural.tolist() == [[0, 0, T], [0, T, 3], [1, 0, 1], [3, 0, T], [3, T, T], [3, 2 * T, 17]]
    # unit 3's and unit 0's tiles apart from each other, unit 0's tail cut in two: an odd list
    apart = np.array([[3, T, T], [0, T, 2], [3, 0, T], [1, 0, 1], [0, 0, T], [3, 2 * T, 17], [0, T + 2, 1]], np.int32)
    return {"natural": natural, "reversed": natural[::-1].copy(), "apart": apart}


@pytest.mark.parametrize("prec,form", [("fp32", "tiled"), ("bf16", "tiled16"), ("f16", "bcast")])
def test_pairs_across_units_and_images(prec, form):
    """Blocks whose two tiles belong to different units, images and per-unit
    scales (natural order: (0, 0), (1, 3), (3, 3)); the same list reversed;
    one unit's tiles non-adjacent.  Each equals the dense values, so each
    equals the others."""
    lists = _pair_lists()
    out = _run(f"pairs-{prec}-{form}", 5, prec, form, lists)
    for name in ("reversed", "apart"):
        assert bits_equal(out[name], out["natural"]), name


def test_degenerate_lists():
    """One tile with one candidate; two one-candidate tiles of two units in
    one block; an empty list returns TMR_OK and writes nothing."""
    lists = {"one": np.array([[1, 0, 1]], np.int32), "two": np.array([[3, 0, 1], [1, 0, 1]], np.int32),
             "none": np.zeros((0, 3), np.int32)}
    out = _run("degenerate", 5, "fp32", "tiled", lists)
    assert (out["none"] == SENTINEL).all()
    assert int((out["one"] != SENTINEL).sum()) == 4 and int((out["two"] != SENTINEL).sum()) == 8
