"""tmr_split_conv_points_chain: the shared route's store launch, heads launch
and reduce at the candidates as ONE accumulator chain, without the acc0 slab.

Expected values: tmr_split_conv store (tiled out, from the broadcast bias
plane, window (0, nb)), tmr_split_conv heads over window (0, nb) starting from
that slab, tmr_heads_reduce -- at the listed pixels, compared bit for bit (no
tolerance: the chain kernel issues the same operations per output element,
with the slab's store and reload as two separately rounded multiplies); every
unlisted element of b must still hold the sentinel.  The chain call is given
no slab at all, so decoder_b's part of acc0 can be neither read nor written.

Operands: tests/test_gpu_points_pairs.py's set (a 17 x 33 map, three images,
four units whose tile pairs cross units and images, unit 3's f_TM scaled by
2^10) with C1 = 160 (the K loop runs on across chunks), C0 = 64 or 40 (a
padded last chunk) and image 1's features scaled by 2^-12: the mid-chain ratio
s_x1 s_w1 / s_x0 s_w0 is then not 1 and differs between the two halves of a
block.  Every case runs plain, zero-poisoned and 0xFF-poisoned
(tests/test_gpu_guarded.py): identical outputs, no guard byte written.
"""
import numpy as np
import pytest
import torch

import guarded_alloc as ga
import test_gpu_guarded as TG
from test_gpu_points import SENTINEL, bits_equal
from test_gpu_points_pairs import PAIR_COUNTS, UI
from tmr_amd._lib import (POINTS_TILE, PREC_CODES, SPLIT_INIT_BCAST, SPLIT_TILED_INIT, SPLIT_TILED_OUT,
                          SPLIT_XMAX_PER_UNIT, call, load, ptr, size, split_tile_window, stream)
from tmr_amd import host

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
B, U, C1, H, W = 3, 4, 160, 17, 33
HW = H * W

_INPUTS = {}  # (nb, C0) -> host tensors
_WANT = {}    # (nb, C0) -> b [U][4][H][W] of the three-launch route


def _inputs(nb, C0):
    if (nb, C0) not in _INPUTS:
        N = 128 * (nb + 1)
        g = torch.Generator().manual_seed(300 + 10 * nb + C0)
        rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
        hw = torch.zeros(N, 5)
        hw[:128 * nb, 0:4] = rn(128 * nb, 4)
        hw[128 * nb:, 4] = rn(128)
        x0, x1 = rn(B, C0, H, W), rn(U, C1, H, W)
        x0[1] *= 2.0 ** -12
        x1[3] *= 2.0 ** 10
        d = dict(N=N, x0=x0, x1=x1, w=rn(N, C0 + C1, 3, 3) * 0.02, bias=rn(N) * 0.1, hw=hw, hb=rn(5),
                 one=rn(1, 8, H, W), wone=rn(N, 8, 3, 3) * 0.02)
        box = np.zeros((U * HW, 4), np.int32)
        box[:HW, 0] = torch.randperm(HW, generator=g).numpy()
        box[HW, 0] = HW - 1
        box[3 * HW:3 * HW + PAIR_COUNTS[3], 0] = torch.randperm(HW, generator=g).numpy()[:PAIR_COUNTS[3]]
        d["box"] = box
        _INPUTS[(nb, C0)] = d
    return _INPUTS[(nb, C0)]


def _operands(a, nb, C0):
    """The packed operands of both launches and the bias plane, the inputs
    placed through the allocator context `a`."""
    from tmr_amd.operands import absmax, absmax_rows, pack_split_w, pack_split_x
    d = _inputs(nb, C0)
    N, pc = d["N"], PREC_CODES["fp32"]
    t = {k: a.place(d[k]) for k in ("x0", "x1", "w", "bias", "hw", "hb", "one", "wone")}
    o = dict(t=t, N=N, pc=pc, uid=a.place(UI), zero=torch.zeros(N, device=DEV))
    o["wp0"], o["wm0"] = pack_split_w(t["w"][:, :C0].contiguous(), C0, "fp32")
    o["wp1"], o["wm1"] = pack_split_w(t["w"][:, C0:].contiguous(), 0, "fp32")
    o["xm0"], o["xm1"] = absmax_rows(t["x0"]), absmax_rows(t["x1"])
    o["xp0"], o["xp1"] = pack_split_x(t["x0"], 3, "fp32", o["xm0"]), pack_split_x(t["x1"], 3, "fp32", o["xm1"])
    wpo, wmo = pack_split_w(t["wone"], 8, "fp32")
    om = absmax(t["one"])
    xpo = pack_split_x(t["one"], 3, "fp32", om)
    o["plane"] = torch.empty(size("acc", 1, N, H, W), device=DEV)
    call("tmr_split_conv", ptr(xpo), 8, None, None, 0, 1, H, W, 3, pc, ptr(wpo), ptr(wmo), ptr(om), ptr(o["zero"]), N,
         0, None, None, ptr(o["plane"]), SPLIT_TILED_OUT, stream())
    o["keep"] = (wpo, wmo, om, xpo)
    return o


def _want(nb, C0):
    """Store launch, heads launch and reduce over decoder_b's window: b of
    every pixel, computed once per operand set."""
    if (nb, C0) not in _WANT:
        with ga.context(None, DEV) as a:
            o = _operands(a, nb, C0)
            N, pc, t = o["N"], o["pc"], o["t"]
            win = split_tile_window(0, nb)
            slab = torch.full((size("acc", B, N, H, W),), float("nan"), device=DEV)
            call("tmr_split_conv", ptr(o["xp0"]), C0, None, None, 0, B, H, W, 3, pc, ptr(o["wp0"]), ptr(o["wm0"]),
                 ptr(o["xm0"]), ptr(o["zero"]), N, 0, None, ptr(o["plane"]), ptr(slab),
                 SPLIT_TILED_OUT | SPLIT_XMAX_PER_UNIT | SPLIT_TILED_INIT | SPLIT_INIT_BCAST | win, stream())
            part = torch.full((size("heads_partials", N, U, H, W),), float("nan"), device=DEV)
            call("tmr_split_conv", None, 0, ptr(o["uid"]), ptr(o["xp1"]), C1, U, H, W, 3, pc, ptr(o["wp1"]),
                 ptr(o["wm1"]), ptr(o["xm1"]), ptr(t["bias"]), N, 1, ptr(t["hw"]), ptr(slab), ptr(part),
                 SPLIT_TILED_INIT | SPLIT_XMAX_PER_UNIT | win, stream())
            ob, b = torch.empty((U, 1, H, W), device=DEV), torch.empty((U, 4, H, W), device=DEV)
            call("tmr_heads_reduce", ptr(part), 128 * nb, 128, U, H, W, ptr(t["hb"]), ptr(ob), ptr(b), stream())
            torch.cuda.synchronize()
            _WANT[(nb, C0)] = b.cpu().numpy()
            assert np.isfinite(_WANT[(nb, C0)]).all()
    return _WANT[(nb, C0)]


def _chain_args(o, C0, box, td, ntiles, b, nb, prec="fp32"):
    t = o["t"]
    return (ptr(o["xp0"]), C0, ptr(o["xm0"]), ptr(o["wp0"]), ptr(o["wm0"]), ptr(o["plane"]), ptr(o["uid"]),
            ptr(o["xp1"]), C1, ptr(o["xm1"]), ptr(o["wp1"]), ptr(o["wm1"]), U, H, W, 3, PREC_CODES[prec],
            ptr(t["bias"]), o["N"], 1, ptr(t["hw"]), ptr(t["hb"]), ptr(box), ptr(td), ntiles, ptr(b),
            split_tile_window(0, nb), stream())


def _chain(a, o, nb, C0, tiles):
    """b (sentinel-filled) after the chained launch over the tile list."""
    tiles = np.ascontiguousarray(tiles, np.int32).reshape(-1, 3)
    b = torch.full((U, 4, H, W), SENTINEL, device=DEV)
    td = a.place(tiles.reshape(-1) if len(tiles) else np.zeros(3, np.int32))
    box = a.place(_inputs(nb, C0)["box"]).view(torch.float32)
    call("tmr_split_conv_points_chain", *_chain_args(o, C0, box, td, len(tiles), b, nb))
    torch.cuda.synchronize()
    return b.cpu().numpy()


def _check(got, want, nb, C0, tiles, what):
    box = _inputs(nb, C0)["box"][:, 0].reshape(U, HW)
    listed = np.zeros((U, HW), bool)
    for u, first, cnt in np.asarray(tiles, np.int64).reshape(-1, 3):
        listed[u, box[u, first:first + cnt]] = True
    for u in range(U):
        g, w_ = got[u].reshape(4, HW), want[u].reshape(4, HW)
        assert bits_equal(g[:, listed[u]], w_[:, listed[u]]), (what, u)
        assert (g[:, ~listed[u]] == SENTINEL).all(), (what, u)


def _lists():
    T = POINTS_TILE
    every = host.point_tiles(np.array([HW, 0, 0, 0]), T)  # unit 0's every pixel: borders, 9 tiles (an odd count)
    assert len(every) == 9 and every[-1, 2] == HW - 8 * T
    return {"full": np.array([[0, 0, T]], np.int32), "one": np.array([[1, 0, 1]], np.int32), "unit0": every,
            "pairs": host.point_tiles(PAIR_COUNTS, T),  # blocks (0, 0), (1, 3), (3, 3): other units, images, scales
            "none": np.zeros((0, 3), np.int32)}


@pytest.mark.parametrize("C0", [64, 40])
@pytest.mark.parametrize("nb", [1, 5, 8])
def test_chain_equals_store_heads_reduce_bits(nb, C0):
    """nb = 5 and 8 run both phases in each of two passes; C0 = 40 pads phase
    0's last chunk."""
    want = _want(nb, C0)
    lists = _lists()

    def flow(a):
        o = _operands(a, nb, C0)
        return {name: _chain(a, o, nb, C0, tiles) for name, tiles in lists.items()}

    def verify(out):
        for name, tiles in lists.items():
            _check(out[name], want, nb, C0, tiles, (nb, C0, name))
        assert (out["none"] == SENTINEL).all()
        assert int((out["one"] != SENTINEL).sum()) == 4

    TG._guarded_runs(f"points_chain:{nb}-{C0}", ga.POISON_FF, flow, verify)


def test_scaled_image_hands_over_with_its_own_ratio():
    """Unit 2 reads image 1, the one scaled by 2^-12, and has no candidate in
    the shared rows: here it gets 70 of its own, paired in one block with a
    tile of unit 3 (image 0, f_TM scaled by 2^10), so the two halves of that
    block hand over between the phases with different powers of two."""
    nb, C0 = 5, 64
    assert UI[2] == 1 and UI[3] == 0
    d = _inputs(nb, C0)
    want = _want(nb, C0)
    with ga.context(None, DEV) as a:
        o = _operands(a, nb, C0)
        box = d["box"].copy()
        box[2 * HW:2 * HW + 70, 0] = np.arange(70) * 7 % HW
        tiles = np.array([[2, 0, 64], [3, 0, 64], [2, 64, 6]], np.int32)
        b = torch.full((U, 4, H, W), SENTINEL, device=DEV)
        call("tmr_split_conv_points_chain", *_chain_args(o, C0, a.place(box).view(torch.float32),
                                                         a.place(tiles.reshape(-1)), len(tiles), b, nb))
        torch.cuda.synchronize()
        got = b.cpu().numpy()
    for u, pix in ((2, box[2 * HW:2 * HW + 70, 0]), (3, box[3 * HW:3 * HW + 64, 0])):
        assert bits_equal(got[u].reshape(4, HW)[:, pix], want[u].reshape(4, HW)[:, pix]), u
    assert int((got != SENTINEL).sum()) == 4 * (70 + 64)


@pytest.mark.parametrize("prec", ["bf16", "f16"])
def test_other_precisions_are_unsupported(prec):
    """The chain is the 3-term fp16 engine's: a bf16 slab's rounding between
    the phases is not reproduced, so those engines stay on the slab route."""
    nb, C0 = 1, 64
    with ga.context(None, DEV) as a:
        o = _operands(a, nb, C0)
        b = torch.full((U, 4, H, W), SENTINEL, device=DEV)
        td = a.place(np.array([1, 0, 1], np.int32))
        box = a.place(_inputs(nb, C0)["box"]).view(torch.float32)
        rc = load().tmr_split_conv_points_chain(*_chain_args(o, C0, box, td, 1, b, nb, prec))
        torch.cuda.synchronize()
    assert rc == -3  # TMR_E_UNSUPPORTED
    assert (b.cpu().numpy() == SENTINEL).all()
