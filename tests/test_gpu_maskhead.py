"""GPU: the fused SAM mask head (tmr_mask_head, include/tmr_maskhead.h) and
FusedMaskDecoder against the reference's own MaskDecoder.forward
(tests/golden/maskhead.npz), the float64 restatement of the rule
(tests/maskhead_ref.py) and the stock torch head on the same device.

The contract is the project's fp32 one: normwise (max |got - ref| / max |ref|
over a call) <= 1e-5.  Where boxes are compared, they are compared exactly:
an error within d = 1e-4 * max|mask| leaves the positive set between {v > d}
and {v > -d}, whose boxes the fixture (and the seeded draws' filter) found
equal, and the box is monotone in the positive set."""
import numpy as np
import pytest
import torch

import guarded_alloc as ga
import maskhead_ref as R
import refine_ref
import tmr_amd
from tmr_amd import _lib

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
f32 = np.float32
TOL = 1e-5
TILE = 128  # the plan's pixels per block (asserted below)


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def upscaling(wt):
    return R.set_upscaling(R.Decoder().output_upscaling, wt).to(DEV)


@pytest.fixture(scope="module")
def wt():
    return R.weights(3)


@pytest.fixture(scope="module")
def packed(wt):
    return tmr_amd.mask_head_weights(upscaling(wt))


def run(packed, src, hyper, size, place=cuda):
    got = tmr_amd.mask_head(place(src), place(hyper), packed, size)
    assert got.dtype == torch.float32 and tuple(got.shape) == (src.shape[0], 1, 4 * size[0], 4 * size[1])
    return got


def check(packed, wt, src, hyper, size, tol=TOL):
    got = run(packed, src, hyper, size)[:, 0].cpu().numpy()
    ref = R.ref_of(wt, src, hyper, size)
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    err = R.normwise(got, ref)
    print(f"N = {src.shape[0]}, {size}: {err:.3e} normwise")
    assert err <= tol, (src.shape, size, err)
    return got, ref


def draw(seed, N, h, w, amp=2.0):
    rng = np.random.default_rng(seed)
    return (amp * rng.standard_normal((N, h * w, 256))).astype(f32), rng.standard_normal((N, 32)).astype(f32)


# ------------------------------------------------------------------ the fixture
def fixture_packed(g):
    return tmr_amd.mask_head_weights(upscaling(R.fixture_weights(g)))


def test_fixture_masks_and_boxes(golden):
    g = golden("maskhead")
    size, img = tuple(int(v) for v in g["emb_size"]), tuple(int(v) for v in g["image_size"])
    got = run(fixture_packed(g), g["src"], g["hyper"], size)
    m, ref = got.cpu().numpy(), g["masks"]
    err = R.normwise(m, ref)
    print(f"fixture: {err:.3e} normwise")
    assert err <= TOL
    for n in range(ref.shape[0]):  # within each mask's box margin
        assert np.abs(m[n] - ref[n]).max() <= 1e-4 * np.abs(ref[n]).max(), n
    lg = np.tile(np.array([[0.7, 0.3]], f32), (ref.shape[0], 1))
    _, boxes, _ = tmr_amd.mask_boxes(got, img, cuda(lg), cuda(g["iou"]))
    assert np.array_equal(boxes.cpu().numpy(), g["boxes"])  # all five, exactly


class Prompt:
    """A prompt encoder stand-in: zero embeddings of the fixture's sizes."""

    def __init__(self, emb, dim=256):
        self.emb, self.dim, self.calls = emb, dim, 0

    def to(self, device):
        return self

    def __call__(self, points, boxes, masks):
        assert points is None and masks is None
        self.calls += 1
        n = boxes.shape[0]
        return torch.zeros(n, 2, self.dim, device=DEV), torch.zeros(n, self.dim, *self.emb, device=DEV)

    def get_dense_pe(self):
        return torch.zeros(1, self.dim, *self.emb, device=DEV)


def fixture_module(g, place=cuda):
    dec = R.decoder_from_fixture(g, place(g["hs"]), place(g["src"])).to(DEV)
    return tmr_amd.FusedMaskDecoder(dec), dec


def test_module_on_fixture(golden):
    g = golden("maskhead")
    fused, dec = fixture_module(g)
    with torch.no_grad():
        masks, iou = fused(*(cuda(g["in_" + k]) for k in ("image_embeddings", "image_pe", "sparse_prompt_embeddings",
                                                          "dense_prompt_embeddings")), False)
        ids = torch.argmax(dec.iou_prediction_head(cuda(g["hs"])[:, 0]), 1)
    assert dec.transformer.calls == 1
    assert np.array_equal(ids.cpu().numpy(), g["ids"])
    assert tuple(iou.shape) == g["iou"].shape and np.abs(iou.cpu().numpy() - g["iou"]).max() <= 1e-5
    m = masks.cpu().numpy()
    assert m.shape == g["masks"].shape and R.normwise(m, g["masks"]) <= TOL
    for n in range(m.shape[0]):
        assert np.abs(m[n] - g["masks"][n]).max() <= 1e-4 * np.abs(g["masks"][n]).max(), n


def refiner_flow(g, place=cuda):
    size, img = tuple(int(v) for v in g["emb_size"]), tuple(int(v) for v in g["image_size"])
    fused, _ = fixture_module(g, place)
    enc = Prompt(size)
    refiner = tmr_amd.SAM_box_refiner(fused, lambda image_size, emb_size: enc)
    N = g["masks"].shape[0]
    lg = np.stack([np.linspace(0.2, 0.9, N), np.linspace(0.8, 0.1, N)], 1).astype(f32)
    bx = np.tile(np.array([[0.2, 0.2, 0.6, 0.6]], f32), (N, 1))
    with torch.no_grad():
        L, B, Rf = refiner([place(lg)], [place(bx)], [place(bx[:, :2])], torch.zeros(1, 3, *img, device=DEV),
                           torch.zeros(1, 256, *size, device=DEV))
    assert enc.calls == 1
    return lg, L[0], B[0], Rf[0]


def test_refiner_with_fused_decoder_returns_fixture_boxes(golden):
    g = golden("maskhead")
    lg, L, B, Rf = refiner_flow(g)
    assert np.array_equal(B.cpu().numpy(), g["boxes"])
    want = np.stack([g["iou"][:, 0] * lg[:, 0], f32(0) * lg[:, 1]], 1)
    assert np.abs(L.cpu().numpy() - want).max() <= 1e-5


def test_non_finite_record(golden):
    g = golden("maskhead")
    size = tuple(int(v) for v in g["emb_size"])
    got = run(fixture_packed(g), g["nf_src"], g["nf_hyper"], size).cpu().numpy()
    ref = g["nf_masks"]
    assert np.isnan(ref).sum() == 32 and np.array_equal(np.isnan(got), np.isnan(ref))
    assert R.normwise(got, ref) <= TOL
    hy = np.stack([g["nf_hyper"][0], g["nf_hyper"][0]])
    hy[1, 5] = np.nan  # a NaN in hyper[n]: mask n is NaN, mask 0 keeps the contract
    src = np.concatenate([g["nf_src"], g["src"][:1]])
    got = run(fixture_packed(g), src, hy, size).cpu().numpy()
    assert np.isnan(got[1]).all() and np.array_equal(np.isnan(got[0]), np.isnan(ref[0]))
    assert R.normwise(got[0], ref[0]) <= TOL


# ------------------------------------------------------------------ shapes against the float64 rule
def test_plan_tile():
    assert _lib.mask_head_plan(h=64, w=64)["tile_pixels"] == TILE


@pytest.mark.parametrize("N,h,w", [(1, 1, 1), (2, 5, 7), (2, 8, 16), (2, 3, 43), (2, 1, 127), (1, 3, 40), (1, 40, 3),
                                   (51, 2, 3), (2, 64, 64)])
def test_shapes_equal_restatement(packed, wt, N, h, w):
    if (h, w) in ((8, 16), (3, 43), (1, 127)):  # a full tile, one pixel more, one less
        assert h * w - TILE == {(8, 16): 0, (3, 43): 1, (1, 127): -1}[(h, w)]
    src, hy = draw(N * 1000 + h * w, N, h, w)
    check(packed, wt, src, hy, (h, w))


def test_variant_mfma128(packed, wt):
    """The one variant the plan reports, by name, on a launch it describes."""
    src, hy = draw(11, 3, 9, 17)
    fake = {k: 4096 for k in ("src", "hyper", "wpack", "b1", "g", "beta", "b2", "masks")}
    plan = _lib.mask_head_plan(h=9, w=17, N=3, **fake)
    assert plan == {"variant": "mfma128", "tile_pixels": 128, "threads": 256, "lds_bytes": 65536, "tiles": 2,
                    "blocks": 6}
    assert sorted(_lib.MASK_HEAD_VARIANTS.values()) == ["mfma128"]
    check(packed, wt, src, hy, (9, 17))


def test_row_scales(packed, wt):
    N, h, w = 3, 5, 9
    src, hy = draw(5, N, h, w)
    rng = np.random.default_rng(6)
    src *= np.ldexp(1.0, rng.integers(-12, 13, (N, h * w, 1))).astype(f32)  # row by row, 2^-12 .. 2^12
    src[0, 7] = 0.0  # an all-zero row
    # one huge channel: 2^23 times the largest other row, and small enough that the rule itself stays
    # finite in fp32 (the LayerNorm's sum of 64 squares of u ~ 0.06 * 3e10)
    src[1, 11, 100] = 3.0e10
    src[1, 12, 3] = -1.0e-20
    hy[2] = 0.0  # hyper = 0: a zero mask
    got, ref = check(packed, wt, src, hy, (h, w))
    assert not got[2].any() and not ref[2].any()
    for n in range(2):  # per mask as well: no mask hides behind a larger one
        assert R.normwise(got[n], ref[n]) <= TOL


# ------------------------------------------------------------------ boxes on seeded draws
def stable(ref32, size):
    """Per mask: whether the box of {v > +d} equals the box of {v > -d}, d = 1e-4 max|mask|, under
    tmr_mask_boxes' rule (tests/refine_ref.py) on the restatement's masks."""
    keep = []
    for m in ref32:
        d = 1e-4 * float(np.abs(m).max())
        v = refine_ref.upsample(m, size)
        keep.append(np.array_equal(refine_ref.int_boxes(m[None], size, lambda a, s: v - f32(d)),
                                   refine_ref.int_boxes(m[None], size, lambda a, s: v + f32(d))))
    return np.array(keep)


# seeds picked on the CPU: the restatement alone keeps 16 of 16 masks at both
@pytest.mark.parametrize("seed,h,w,img", [(21, 6, 8, (61, 93)), (22, 9, 5, (50, 37))])
def test_boxes_on_seeded_draws(packed, wt, seed, h, w, img):
    N = 16
    rng = np.random.default_rng(seed)
    src = R.windowed_src(rng, N, h, w)
    hy = rng.standard_normal((N, 32)).astype(f32)
    ref = R.ref_of(wt, src, hy, (h, w))
    ref32 = ref.astype(f32)
    keep = stable(ref32, img)
    print(f"seed {seed}: {int(keep.sum())} of {N} masks enter the box comparison")
    assert keep.sum() >= 0.75 * N
    got = run(packed, src, hy, (h, w))
    m = got[:, 0].cpu().numpy()
    assert R.normwise(m, ref) <= TOL
    for n in np.nonzero(keep)[0]:
        assert np.abs(m[n] - ref[n]).max() <= 1e-4 * np.abs(ref[n]).max(), n
    lg = np.tile(np.array([[0.5, 0.5]], f32), (N, 1))
    _, boxes, _ = tmr_amd.mask_boxes(got, img, cuda(lg), cuda(np.ones(N, f32)))
    want = refine_ref.mask_boxes(ref32, img, lg, np.ones(N, f32))[1]
    assert np.array_equal(boxes.cpu().numpy()[keep], want[keep])


# ------------------------------------------------------------------ the workload's shape
def test_workload_shape_equals_stock_torch():
    """N = 50 at 64x64 against the stock torch head on the same device:
    output_upscaling, the four MLPs, the matmul, the argmax selection."""
    N, h, w = 50, 64, 64
    torch.manual_seed(7)
    dec = R.Decoder()
    R.set_upscaling(dec.output_upscaling, R.weights(9))
    dec = dec.to(DEV).eval()
    gen = torch.Generator(device="cpu").manual_seed(8)
    hs = torch.randn(N, 7, 256, generator=gen).to(DEV)
    src = (2 * torch.randn(N, h * w, 256, generator=gen)).to(DEV)
    dec.transformer = R.Replay(hs, src)
    fused = tmr_amd.FusedMaskDecoder(dec)
    with torch.no_grad():
        want, want_iou, ids = dec.stock_head(hs, src, (h, w))
        emb = torch.zeros(1, 256, h, w, device=DEV)
        masks, iou = fused(emb, emb, torch.zeros(N, 2, 256, device=DEV), emb, False)
    assert len(set(ids.tolist())) >= 2
    assert tuple(masks.shape) == (N, 1, 4 * h, 4 * w) and torch.equal(iou, want_iou)
    err = float((masks - want).abs().max() / want.abs().max())
    print(f"N = 50, 64x64 against stock torch: {err:.3e} normwise")
    assert err <= TOL


# ------------------------------------------------------------------ the weights cache
def test_weights_cache_follows_in_place_edits(wt):
    up = upscaling(wt)
    W = tmr_amd.mask_head_weights(up)
    src, hy = draw(31, 2, 4, 5)
    a = run(W, src, hy, (4, 5))
    assert W.packs == 1
    b = run(W, src, hy, (4, 5))
    assert W.packs == 1 and torch.equal(a, b)  # no repack without an edit
    with torch.no_grad():
        up[0].weight.mul_(1.5)
    c = run(W, src, hy, (4, 5))
    assert W.packs == 2 and not torch.equal(a, c)
    wt2 = dict(wt, W1=up[0].weight.detach().cpu().numpy())
    assert R.normwise(c[:, 0].cpu().numpy(), R.ref_of(wt2, src, hy, (4, 5))) <= TOL
    with torch.no_grad():
        up[1].bias.add_(0.25)  # the LayerNorm2d bias is followed too
    d = run(W, src, hy, (4, 5))
    wt3 = dict(wt2, beta=up[1].bias.detach().cpu().numpy())
    assert W.packs == 3 and R.normwise(d[:, 0].cpu().numpy(), R.ref_of(wt3, src, hy, (4, 5))) <= TOL


# ------------------------------------------------------------------ guarded allocator
def _bits(a, b, path=""):
    if isinstance(a, dict):
        assert set(a) == set(b)
        for k in a:
            _bits(a[k], b[k], f"{path}.{k}")
    else:
        assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), path


def test_routes_under_guarded_allocator(golden, wt):
    """The mask_head route (ragged last tiles: 3x43 = one pixel past a tile,
    5x7) and the FusedMaskDecoder -> tmr_mask_boxes route: the same bits
    unpatched, zero- and 0xFF-poisoned, and no guard byte written."""
    g = golden("maskhead")

    def flow(a):
        place = lambda x: a.place(np.ascontiguousarray(x))  # noqa: E731
        out = {}
        W = tmr_amd.mask_head_weights(upscaling(wt))
        for key, (N, h, w) in (("ragged129", (2, 3, 43)), ("ragged35", (3, 5, 7))):
            src, hy = draw(40 + N, N, h, w)
            out[key] = run(W, src, hy, (h, w), place).cpu().numpy()
        _, L, B, Rf = refiner_flow(g, place)
        out.update(refiner_logits=L.cpu().numpy(), refiner_boxes=B.cpu().numpy(), refiner_refs=Rf.cpu().numpy())
        return out

    with ga.context(None, DEV) as a:
        plain = flow(a)
    assert np.array_equal(plain["refiner_boxes"], g["boxes"])
    for poison in (ga.POISON_ZERO, ga.POISON_FF):  # zero first
        with ga.GuardedAlloc(poison, DEV) as a:
            out = flow(a)
            assert len(a.records) > 0
            a.check()
        _bits(plain, out, f"poison {poison:#x}")
