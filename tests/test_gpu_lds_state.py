"""Every LDS-using entry point of libtmr.so on LDS that holds a known pattern
(tests/lds_state.py, tests/lds_state/): the on-chip counterpart of
tests/test_gpu_guarded.py.

A kernel that pads an MFMA tile with zero operands is right only where the
other operand was staged: 0 x (stale LDS bits) can be NaN.  Whether a run shows
such a read depends on what the previous kernel on that CU left behind, so
every case here runs four times: with no fill, then with the LDS of every CU
filled with 0x00000000, 0xFFFFFFFF (NaN / -1) and 0x7B7B7B7B (large, finite:
fmaxf-style reductions ignore a NaN) immediately before the entry point under
test, on its own stream.  The zero fill comes first: the other two can turn a
stale index into a wild address, so they follow a passed zero run.

(i)   The mechanism: a fill reaches every CU, and the next dispatch's LDS
      allocation holds it (the planted read).  Every other test depends on the
      second through the `mechanism` fixture: where it fails they report an
      error, not a pass.
(ii)  One entry point at a time (CASES), at the smallest shapes of the
      existing tests where padding exists: grids of a few blocks to a few
      hundred, so that (nearly) every block is the first on its CU.
      (a) each run makes the reference check of that entry point's existing
          test: the bodies are the existing tests' own (imported, not
          restated), so a wrong kernel fails here as it fails there;
      (b) every device tensor the body brings to the host, and every output it
          returns, is bit-identical across the four runs.  Where a body
          compares on the device, bit for bit, (a) in each run implies (b).
      Allocations of torch.empty / empty_like are zeroed during a run, so an
      unwritten output element holds the same bytes every time.
(iii) Whole routes inside filled(pattern): every stream-taking call of the
      route is preceded by a fill.  Eager (use_graphs = False): a fill inside
      a capture would become part of the graph.

NO_LDS lists the stream-taking entry points whose source file declares no
__shared__ storage; tests/test_lds_state_host.py requires every bound
stream-taking symbol to be in exactly one of CASES and NO_LDS.

Limits.  Registers cannot be filled, neither can LDS addresses outside a
kernel's allocation.  Only the first block a CU runs after the fill sees the
pattern.  Another tenant's kernel between fill and launch weakens a case: a
miss, never a false alarm.  Graph replay is not covered.  Of an entry point
that launches several kernels only the first is certain to start on filled
LDS; a later one finds the pattern wherever the earlier ones wrote no LDS, and
their leavings elsewhere.  These launch more than one: tmr_xcorr with squeeze
(correlation, squeeze), tmr_nms with an image above 256 rows (gather, sort,
bins, pairs, greedy, scan, emit), tmr_peaks_decode (probabilities, finder,
decode), tmr_gt_loss (boxes, images, units, final, gather / rows),
tmr_mask_boxes (init, bands, epilogue), tmr_mask_head_prep (maxima, pack),
tmr_twoway_pool (pool, combine), tmr_feature_stats (partials, final).  Every
other entry point is one kernel.  The routes of (iii) reach later kernels no
better.
"""
import numpy as np
import pytest
import torch

import guarded_alloc as ga
import lds_state as ls
import oracle
import test_gpu_coco as T_coco
import test_gpu_evalloss as T_eval
import test_gpu_guarded as T_guard
import test_gpu_maskhead as T_mh
import test_gpu_operands as T_ops
import test_gpu_parity as T_par
import test_gpu_points as T_pts
import test_gpu_points_chain as T_chain
import test_gpu_points_pairs as T_pairs
import test_gpu_random as T_rand
import test_gpu_refine as T_refine
import test_gpu_third_party_pins as T_pins
import test_gpu_tokens as T_tok
import test_gpu_twoway as T_tw
import test_stream as T_stream
import tmr_amd
import xcorr_cases
from test_gpu_guarded import _same_bits
from test_gpu_maskhead import packed, wt  # noqa: F401  (fixtures of the mask head's weights)
from test_gpu_points import data  # noqa: F401  (fixture of the points operands)
from tmr_amd import _lib
from tmr_amd import mapreduce as mr
from tmr_amd import synth

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
RUNS = (("plain", None), ("zero", ls.PATTERN_ZERO), ("ff", ls.PATTERN_FF), ("7b", ls.PATTERN_7B))
PLANTED_EXACT = 2016.0  # 1 + 2 + ... + 63


# ------------------------------------------------------------------ (i) mechanism
def _planted(pattern):
    torch.cuda.synchronize()
    out = ls.fill_then(pattern, ls.planted_read)
    return int((out == PLANTED_EXACT).sum()), int(np.isnan(out).sum()), out.size


def _check_planted():
    """The toy kernel that reads one LDS word it never staged, one block per
    entry: exact after the zero fill, NaN after 0xFFFFFFFF, exact again after
    0x7B7B7B7B (0 x finite).  Another tenant's kernel between fill and read can
    take the pattern off a CU, so the three reads may be made up to three
    times; every attempt is printed and the first complete one passes."""
    seen = []
    for attempt in range(3):
        got = [_planted(p) for p in (ls.PATTERN_ZERO, ls.PATTERN_FF, ls.PATTERN_7B)]
        seen.append(got)
        print(f"planted read, attempt {attempt}: (exact, NaN, blocks) after the zero fill {got[0]}, after 0xFFFFFFFF "
              f"{got[1]}, after 0x7B7B7B7B {got[2]}")
        n = got[0][2]
        assert got[0] == (n, 0, n) and got[2] == (n, 0, n), f"0 x a finite stale word changed an exact sum: {got}"
        assert got[1][0] + got[1][1] == n, got
        if got[1] == (0, n, n):
            return
    raise AssertionError(f"a fill of 0xFFFFFFFF does not reach the next dispatch's LDS on every CU: {seen}")


@pytest.fixture(scope="module")
def mechanism():
    _check_planted()


def test_fill_reaches_every_cu():
    """Fill, then probe with the same geometry: as many distinct CU keys as the
    device has CUs, and no word that differs from the pattern in any block.
    Up to three attempts (another tenant's kernel may run between the two),
    each printed; the first complete one passes."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    blocks = ls.FILL_MULTIPLE * cus
    stream = torch.cuda.current_stream().cuda_stream
    seen = []
    for attempt in range(3):
        for pattern in (ls.PATTERN_7B, ls.PATTERN_FF):
            torch.cuda.synchronize()
            ls.fill(pattern, stream, blocks)
            keys, bad = ls.probe(pattern, blocks)
            seen.append((len(set(keys.tolist())), int((bad != 0).sum()), int(bad.max())))
            print(f"attempt {attempt}, pattern {pattern:#010x}, {blocks} blocks ({ls.FILL_MULTIPLE} x {cus} CUs): "
                  f"{seen[-1][0]} distinct CU keys, {seen[-1][1]} blocks with differing words (max {seen[-1][2]})")
        if all(s == (cus, 0, 0) for s in seen[-2:]):
            break
    else:
        raise AssertionError(f"no complete fill-and-probe in three attempts: (keys, bad blocks, max bad) = {seen}, "
                             f"{cus} CUs")
    # a pattern nobody filled differs everywhere: the probe reads what is there
    keys, bad = ls.probe(0x12345678, blocks)
    assert int(bad.min()) == 163840 // 4


def test_planted_read_is_detected():
    _check_planted()


# ------------------------------------------------------------------ the four runs
class _HostCapture:
    """While active: records every device tensor brought to the host
    (Tensor.cpu / .to / .tolist / .item) as raw bytes, and zeroes what
    torch.empty / torch.empty_like allocate on the device."""

    def __enter__(self):
        self.seen, self.meta = [], []
        T = torch.Tensor
        self._real = {n: getattr(T, n) for n in ("cpu", "to", "tolist", "item")}
        self._alloc = {n: getattr(torch, n) for n in ("empty", "empty_like")}
        real, rec = self._real, self._record

        def cpu(t, *a, **k):
            r = real["cpu"](t, *a, **k)
            if t.is_cuda:
                rec(r)
            return r

        def to(t, *a, **k):
            r = real["to"](t, *a, **k)
            if t.is_cuda and not r.is_cuda:
                rec(r)
            return r

        def tolist(t):
            return real["tolist"](cpu(t) if t.is_cuda else t)

        def item(t):
            return real["item"](cpu(t) if t.is_cuda else t)

        def zeroing(fn):
            def alloc(*a, **k):
                t = fn(*a, **k)
                return t.zero_() if t.is_cuda else t
            return alloc

        T.cpu, T.to, T.tolist, T.item = cpu, to, tolist, item
        torch.empty, torch.empty_like = zeroing(self._alloc["empty"]), zeroing(self._alloc["empty_like"])
        return self

    def _record(self, r):
        r = r.detach()
        self.meta.append((tuple(r.shape), str(r.dtype)))
        self.seen.append(r.reshape(-1).contiguous().view(torch.uint8).numpy().copy())

    def __exit__(self, *exc):
        for n, f in self._real.items():
            setattr(torch.Tensor, n, f)
        for n, f in self._alloc.items():
            setattr(torch, n, f)
        return False


def _host(x):
    """Nested outputs with every tensor as a host array."""
    if isinstance(x, dict):
        return {k: _host(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_host(v) for v in x]
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu()
        return x.reshape(-1).contiguous().view(torch.uint8).numpy() if x.dtype == torch.bfloat16 else x.numpy()
    return x


def _one_run(what, body, entries, pattern):
    torch.cuda.synchronize()
    with _HostCapture() as cap, ls.filled(pattern, only=entries) as proxy:
        ret = body()
        torch.cuda.synchronize()
    if proxy is not None:
        assert proxy.calls, f"{what}: the body launched nothing under the fill"
        for e in entries or ():
            assert e in proxy.calls, f"{what}: {e} was not called (calls: {sorted(set(proxy.calls))})"
    return dict(meta=cap.meta, host=cap.seen, ret=_host(ret))


def _four_runs(what, body, entries=None):
    """body() four times (RUNS): its own assertions are (a); what it brings to
    the host and what it returns must be bit-identical across the runs (b).
    entries: the entry points that get a fill in front (None: every one);
    each must have been called in every filled run.  The first run also fills
    whatever the body caches (shared references, packed weights): where it
    brought other tensors to the host than the second, it is made once more,
    and that run is the unfilled one of the four."""
    kept = {}
    for name, pattern in RUNS:
        out = _one_run(what, body, entries, pattern)
        if name == "zero" and out["meta"] != kept["plain"]["meta"]:
            kept["plain"] = _one_run(what, body, entries, None)
        for other, ref in kept.items():
            assert out["meta"] == ref["meta"], \
                f"{what}: {name} vs {other}: the runs brought different tensors to the host"
            _same_bits({k: ref[k] for k in ("host", "ret")}, {k: out[k] for k in ("host", "ret")},
                       f"{what}: {name} vs {other}")
        kept[name] = out
    return kept


def _np(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else x


# ------------------------------------------------------------------ (ii) bodies that are not one existing test
def _mfma_variant(table, H, W, C, kmax):
    (variant,) = [c[4] for c in table if c[:4] == (H, W, C, kmax)]
    return variant


def _xcorr_mfma(H, W, C, kmax, prec):
    table = xcorr_cases.MFMA_3TERM if prec == "fp32" else xcorr_cases.MFMA_ONE_TERM
    return lambda fx: T_par._xcorr_mfma_case(H, W, C, kmax, prec, _mfma_variant(table, H, W, C, kmax))


POINT_LISTS = {  # a tile of 1 candidate, of 63, of 64; three tiles: a pair and a block with one tile missing
    "one": [[1, 0, 1]], "t63": [[0, 0, 63]], "t64": [[0, 64, 64]],
    "odd": [[3, 0, _lib.POINTS_TILE], [3, _lib.POINTS_TILE, _lib.POINTS_TILE], [3, 2 * _lib.POINTS_TILE, 17]],
}


def _points_lists(prec, form):
    """tmr_split_conv_points over POINT_LISTS at the smallest window of
    tests/test_gpu_points_pairs.py, against its dense reference, bit for bit."""
    def body(fx):
        nb = 1
        want = T_pairs._want(nb, prec, form)
        out = {}
        with ga.context(None, DEV) as a:
            ops = T_pairs._operands(a, nb, prec, form)
            for name, tiles in POINT_LISTS.items():
                out[name] = T_pairs._points(a, ops, nb, tiles)
                assert T_pairs._check(out[name], want, nb, tiles, (prec, form, name)) == sum(t[2] for t in tiles)
        return out
    return body


def _chain_lists(C0):
    """tmr_split_conv_points_chain over POINT_LISTS (tests/test_gpu_points_chain.py's
    operands and three-launch reference); C0 = 40 pads phase 0's last chunk."""
    def body(fx):
        nb = 1
        want = T_chain._want(nb, C0)
        out = {}
        with ga.context(None, DEV) as a:
            o = T_chain._operands(a, nb, C0)
            for name, tiles in POINT_LISTS.items():
                out[name] = T_chain._chain(a, o, nb, C0, tiles)
                T_chain._check(out[name], want, nb, C0, tiles, (C0, name))
        return out
    return body


NMS_SIZES = (1, 63, 64, 65, 257)


def _nms_small(fx):
    """tmr_nms_small over five images of one unit each, 1 / 63 / 64 / 65 / 257
    rows (the last above TMR_NMS_SMALL: kept = -1, nothing written), against
    oracle.nms, exact."""
    thr = 0.5
    rows = [T_guard._nms_rows(n) for n in NMS_SIZES]
    bx, lg, rf = (np.concatenate([r[i] for r in rows]) for i in range(3))
    counts = np.array(NMS_SIZES, np.int32)
    off = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64)
    G, S = len(NMS_SIZES), _lib.ptr
    d = [torch.from_numpy(x).to(DEV) for x in (lg, bx, rf, counts, off, np.arange(G + 1, dtype=np.int32))]
    out_l, out_b, out_r = (torch.full((G * 256, k), -7.0, device=DEV) for k in (2, 4, 2))
    kept = torch.full((G,), -7, device=DEV, dtype=torch.int32)
    _lib.call("tmr_nms_small", *(S(t) for t in d), G, thr, S(out_l), S(out_b), S(out_r), None, S(kept), _lib.stream())
    torch.cuda.synchronize()
    kept_h, L, Bx, R = kept.cpu().numpy(), out_l.cpu().numpy(), out_b.cpu().numpy(), out_r.cpu().numpy()
    for g, (b, l, r) in enumerate(rows):
        sl = slice(g * 256, (g + 1) * 256)
        if NMS_SIZES[g] > 256:
            assert kept_h[g] == -1 and (L[sl] == -7.0).all() and (Bx[sl] == -7.0).all() and (R[sl] == -7.0).all()
            continue
        k = oracle.nms(b, l[:, 0], thr)
        assert kept_h[g] == len(k), (g, kept_h[g], len(k))
        n = len(k)
        assert T_par.bits_equal(L[sl][:n], l[k]) and T_par.bits_equal(Bx[sl][:n], b[k]) and \
            T_par.bits_equal(R[sl][:n], r[k]), g
        assert (L[sl][n:] == -7.0).all() and (Bx[sl][n:] == -7.0).all()
    return dict(kept=kept_h, L=L, Bx=Bx, R=R)


def _feature_stats(shape):
    def body(fx):
        f = synth.sam_features(11, *shape)
        f[:, :, 0, 0] = 0.0
        got = mr.feature_stats(torch.from_numpy(f).to(DEV))
        T_stream.check_feature_stats(f, got)
        return _np(got)
    return body


def _mask_head_with_prep(N, h, w):
    """The weights are packed inside the run (tmr_mask_head_prep), then the head."""
    def body(fx):
        w_ = fx("wt")
        src, hy = T_mh.draw(N * 1000 + h * w, N, h, w)
        got, _ = T_mh.check(tmr_amd.mask_head_weights(T_mh.upscaling(w_)), w_, src, hy, (h, w))
        return got
    return body


def _t(fn, *args):
    """An existing test's body with its parameters."""
    return lambda fx: fn(*args)


def _tf(fn, fixtures, *args):
    """The same for a test that takes fixtures first."""
    return lambda fx: fn(*(fx(n) for n in fixtures), *args)


SPLIT_CONV = [(13, 200, 9, 70, 3, False), (40, 72, 17, 33, 3, True), (16, 16, 24, 24, 5, True),
              (24, 8, 20, 20, 1, False), (12, 12, 9, 9, 7, True)]  # rows of test_split_conv_vs_torch
MASK_HEAD = [(1, 1, 1), (2, 3, 43), (2, 1, 127)]
TWOWAY = [(N, pi, T, shared) for (N, T) in ((1, 7), (3, 5), (5, 8)) for pi in (0, 1) for shared in (False, True)]

# entry point -> {case id: body(fx)}; fx(name) gives a fixture.  The fill goes in front of every call of the
# entry point the body makes, and of no other.
CASES = {
    "tmr_xcorr": {
        **{f"mfma-{H}x{W}x{C}-k{k}-fp32": _xcorr_mfma(H, W, C, k, "fp32")
           for H, W, C, k in ((33, 64, 8, 15), (70, 192, 4, 11), (40, 256, 8, 29), (77, 256, 8, 9))},
        **{f"mfma-{H}x{W}x{C}-k{k}-{p}": _xcorr_mfma(H, W, C, k, p)  # bf16: the bf16 output plane as well
           for H, W, C, k in ((70, 192, 4, 19), (40, 256, 4, 29), (77, 256, 4, 9)) for p in ("bf16", "f16")},
        "valu-29x37": _t(T_par.test_xcorr_units_both_kernels_vs_oracle, 29, 37),
        "rows-33x64": _t(T_par.test_xcorr_units_both_kernels_vs_oracle, 33, 64),
        "rows31-9x1024-band19": _t(T_par.test_xcorr_valu_reduced_bands_vs_exact, 9, 1024, (27, 31), ("rows31", 19)),
    },
    "tmr_template_split": {f"prec{p}": _t(T_ops.test_template_split_fragments_and_exponents, p, "listed")
                           for p in T_ops.PRECS},
    "tmr_split_conv": {
        **{f"{C}-{N}-{H}x{W}-k{ks}-{p}": _t(T_par.test_split_conv_vs_torch, C, N, H, W, ks, leaky, p)
           for C, N, H, W, ks, leaky in SPLIT_CONV for p in ("fp32", "bf16", "f16")},
        "heads-two-sources": _t(T_par.test_split_conv_scales_and_two_sources, 1.0),
        "tiled-slab-bf16": _t(T_par.test_split_acc_slab_bf16),
    },
    "tmr_split_conv_points": {
        **{f"{p}-{f}": _tf(T_pts.test_points_equal_dense_bits, ("data",), p, f) for p, f in T_pts.FORMS},
        **{f"lists-{p}-{f}": _points_lists(p, f) for p, f in (("fp32", "tiled"), ("bf16", "tiled16"), ("f16", "bcast"))},
    },
    "tmr_split_conv_points_chain": {"lists-C0-64": _chain_lists(64), "lists-C0-40": _chain_lists(40)},
    "tmr_split_xpack": {f"{S}-{C}-{H}x{W}-k{ks}": _t(T_par.test_xpack_records_bitexact, S, C, H, W, ks)
                        for S, C, H, W, ks in ((3, 33, 8, 12, 1), (2, 40, 19, 37, 3), (2, 32, 9, 20, 5))},
    # the bf16 input form runs where W % 8 == 0 (test_xpack_records_bitexact)
    "tmr_split_xpack16": {"1-8-16x32-k1": _t(T_par.test_xpack_records_bitexact, 1, 8, 16, 32, 1)},
    "tmr_split_wpack": {"8-24-0-k1": _t(T_ops.test_wpack_records_bitexact, 8, 24, 0, 1),
                        "72-40-0-k3": _t(T_ops.test_wpack_records_bitexact, 72, 40, 0, 3)},
    "tmr_split_fold_proj": {"5-7-4-3-k1": _t(T_ops.test_fold_proj_bitexact, 5, 7, 4, 3, 1),
                            "5-7-4-3-k3": _t(T_ops.test_fold_proj_bitexact, 5, 7, 4, 3, 3)},
    "tmr_absmax_rows": {f"{S}x{n}": _t(T_ops.test_absmax_rows_planted_maximum, S, n)
                        for S, n in ((1, 1), (1, 7), (3, 1023), (5, 1024))},
    "tmr_pixel_absmax": {f"{S}-{C}-{HW}": _t(T_ops.test_pixel_absmax_planted_maximum, S, C, HW)
                         for S, C, HW in ((1, 1, 1), (2, 17, 65), (5, 33, 63))},
    "tmr_scale_merge": {c[0]: _t(T_ops.test_scale_merge, *c) for c in T_ops._merge_cases()},
    "tmr_heads_reduce": {f"{U}-{H}x{W}-t{t}": _t(T_ops.test_heads_reduce_bitexact, U, H, W, t)
                         for U, H, W in ((1, 1, 1), (3, 5, 7), (2, 16, 33)) for t in (128, 64)},
    "tmr_upsample2x": {"7x5": _t(T_par.test_upsample2x_tiled_and_projection_order, 7, 5),
                       "33x47": _t(T_par.test_upsample2x_tiled_and_projection_order, 33, 47)},
    "tmr_templates": {"golden-rois": _tf(T_par.test_roi_align_bitexact_vs_oracle, ("golden",)),
                      "mixed-units-C5": _t(T_pins.test_templates_mixed_units_one_launch, 5)},
    "tmr_peaks_decode": {"empty-unit": _t(T_par.test_get_pred_boxes_empty_units_dummy_row),
                         "find-then-decode": _t(T_pts.test_find_then_decode_equals_one_call),
                         "golden": _tf(T_par.test_get_pred_boxes_golden, ("golden",), "pred_boxes")},
    "tmr_maxpool3x3": {"x".join(map(str, s)): (lambda s: lambda fx: T_par.run_maxpool(s))(s)
                       for s in ((2, 3, 7, 9), (1, 1, 1, 1), (3, 1, 2, 5))},
    "tmr_nms": {f"n{n}": _t(T_par.test_nms_random_vs_oracle, n, 0.5) for n in NMS_SIZES},
    "tmr_nms_small": {"n1-63-64-65-257": _nms_small},
    "tmr_feature_stats": {"3-7-5x3": _feature_stats((3, 7, 5, 3)), "2-8-8x8": _feature_stats((2, 8, 8, 8))},
    "tmr_gt_loss": {"8x8-G1": lambda fx: T_eval.run_sweep(T_eval.SWEEP.index((8, 8, 1)), fused=True)},
    "tmr_mask_boxes": {"x".join(map(str, s)): _t(T_refine.test_mask_boxes_equals_restatement, s)
                       for s in ((5, 7, 1, 9), (12, 9, 7, 4), (1, 1, 6, 6))},
    "tmr_coco_match": {f"D{D}-G{G}": _t(T_coco.test_matching_shapes, D, G) for D, G in ((3, 65), (5, 0), (7, 257))},
    "tmr_mask_head": {f"{N}-{h}x{w}": _tf(T_mh.test_shapes_equal_restatement, ("packed", "wt"), N, h, w)
                      for N, h, w in MASK_HEAD},
    "tmr_mask_head_prep": {f"{N}-{h}x{w}": _mask_head_with_prep(N, h, w) for N, h, w in MASK_HEAD},
    "tmr_twoway_pool": {f"N{N}-P{pi}-T{T}-{'shared' if s else 'own'}": _t(T_tw.test_pool_equals_rule, N, pi, T, s)
                        for N, pi, T, s in TWOWAY},
    "tmr_twoway_update": {f"N{N}-P{pi}-T{T}-{'shared' if s else 'own'}": _t(T_tw.test_update_equals_rule, N, pi, T, s)
                          for N, pi, T, s in TWOWAY},
    "tmr_tokens_front": {f"N{N}-T{T}-{m}": _t(T_tok.test_front_equals_rule, N, T, m, 128)
                         for N, T, m in ((1, 7, "skip"), (5, 1, "pe"), (19, 7, "none"))},
    "tmr_tokens_back": {f"N{N}-T{T}-mlp{m}": _t(T_tok.test_back_equals_rule, N, T, m, 128)
                        for N, T, m in ((1, 7, 64), (5, 1, 0), (19, 7, 64))},
    # the tail needs T >= 1 + M = 5 tokens: (5, 5) stands where front and back run (5, 1)
    "tmr_tokens_tail": {f"N{N}-T{T}": _t(T_tok.test_tail_equals_rule, N, T, 32) for N, T in ((1, 7), (5, 5), (19, 7))},
}

# stream-taking entry point -> the source file of its kernels, which declares no __shared__ storage.  Every .hip
# file of the library declares some today, so every entry point has cases above.
NO_LDS = {}

ENTRY_CASES = [(e, c) for e, cases in CASES.items() for c in cases]


@pytest.mark.parametrize("entry,case", ENTRY_CASES, ids=[f"{e}-{c}" for e, c in ENTRY_CASES])
def test_entry_point(entry, case, mechanism, request):
    _four_runs(f"{entry} {case}", lambda: CASES[entry][case](request.getfixturevalue), entries=(entry,))


# ------------------------------------------------------------------ (iii) whole routes
def _detect(name):
    seed, setup, want, candidates = T_guard.DETECT[name]

    def body(fx):
        r = T_rand.run_config(seed, setup=setup)
        route = r["route"]
        assert route["graph"] == "eager", route
        for k, v in want.items():
            assert route[k] == v, (name, k, route)
        assert not candidates or route["points"] > 0, route
        return {k: r[k] for k in ("o", "b", "L", "Bx", "R")}
    return body


def _module(seed):
    def body(fx):
        r = T_rand._module_variant(seed, 1e-5, setup=T_guard._eager_module)
        assert r["graph"] in (None, "eager"), r["graph"]
        return {k: r[k] for k in ("o", "b", "f_tm", "f0")}
    return body


def _refiner(fx):
    with ga.context(None, DEV) as a:
        return T_refine._refine_flow(fx("golden")("refine"))(a)


ROUTES = {
    "detect-valu": _detect("23"),  # an 18 x 18 map: the generic VALU correlation
    "detect-mfma": _detect("10"),  # W = 64, E = 5, k <= 31: the MFMA correlation
    "detect-mfma-bf16-points": _detect("130"),  # the bf16 f_TM plane and the points launch
    "module-35": _module(35),  # squeeze, no upsample, 2 layers, k 5
    "eval-loss-8x8-G1": lambda fx: T_eval.run_sweep(T_eval.SWEEP.index((8, 8, 1)), fused=True),
    "maxpool": lambda fx: T_par.run_maxpool((2, 3, 7, 9)),
    "feature-stats": _feature_stats((3, 7, 5, 3)),
    "refiner": _refiner,
    "fused-decoder-transformer": _t(T_tw.test_fused_decoder_with_fused_transformer),
    "fused-decoder-tokens": _tf(T_tok.test_decoder_with_fused_tokens, ("golden",)),
}


@pytest.mark.parametrize("name", list(ROUTES))
def test_route(name, mechanism, request):
    _four_runs(f"route {name}", lambda: ROUTES[name](request.getfixturevalue))
