"""The guarded allocator (tests/guarded_alloc.py) proved on the CPU, through its
device override: overruns on either side are caught and named, a read of an
unwritten element shows between the two poisons, a clean function passes,
the patched functions come back, and the package allocates tensors only by
the spellings the tool patches."""
import glob
import os
import re

import numpy as np
import pytest
import torch

import guarded_alloc as ga
import tmr_amd

CPU = "cpu"
THIS = os.path.abspath(__file__)


def _guarded(poison):
    return ga.GuardedAlloc(poison, device=CPU)


def test_views_are_contiguous_aligned_and_exact():
    """Every patched spelling, for fp32, bf16, int64, uint8 and empty shapes:
    the requested dtype and shape, contiguous, 256-B aligned, the payload
    ending where the post-guard begins, values as asked."""
    with _guarded(ga.POISON_FF) as g:
        made = [torch.empty((3, 5), dtype=torch.float32, device=CPU), torch.empty(7, dtype=torch.bfloat16, device=CPU),
                torch.empty(2, 3, dtype=torch.int64, device=CPU), torch.empty(0, dtype=torch.float32, device=CPU),
                torch.empty((0, 4), dtype=torch.float32, device=CPU), torch.empty((), dtype=torch.float64, device=CPU),
                torch.empty(size=(13,), dtype=torch.uint8, device=CPU)]
        for t, (raw, nbytes, shape, dtype, site, byte) in zip(made, g.records):
            assert t.is_contiguous() and t.dtype == dtype and tuple(t.shape) == shape
            assert nbytes == t.numel() * t.element_size() and raw.numel() == 2 * ga.GUARD + nbytes
            assert t.storage_offset() * t.element_size() == ga.GUARD and ga.GUARD % 256 == 0
            assert t.numel() == 0 or t.data_ptr() == raw.data_ptr() + ga.GUARD
            assert site.startswith(THIS + ":") and byte == ga.GUARD_BYTE
            assert bool((raw[:ga.GUARD] == ga.GUARD_BYTE).all()) and bool((raw[ga.GUARD + nbytes:] == ga.GUARD_BYTE).all())
        assert torch.isnan(made[0]).all() and torch.isnan(made[1].float()).all() and bool((made[2] == -1).all())
        z = torch.zeros((2, 3), device=CPU)
        assert z.dtype == torch.float32 and bool((z == 0).all())
        assert bool((torch.zeros(4, dtype=torch.int32, device=CPU) == 0).all())
        assert bool((torch.ones(3, device=CPU) == 1).all())
        f = torch.full((2, 2), 2.5, device=CPU)
        assert f.dtype == torch.float32 and bool((f == 2.5).all())
        assert torch.full((3,), 7, device=CPU).dtype == torch.int64
        assert torch.full((1,), 1.5, dtype=torch.float64, device=CPU).dtype == torch.float64
        e = torch.empty_like(made[0])
        assert e.shape == made[0].shape and e.dtype == torch.float32 and torch.isnan(e).all()
        zl = torch.zeros_like(made[2])
        assert zl.dtype == torch.int64 and bool((zl == 0).all())
        n = len(g.records)
        assert n == len(made) + 8
        g.check()
    with _guarded(ga.POISON_ZERO) as g:
        assert bool((torch.empty(5, dtype=torch.float32, device=CPU) == 0).all())
        p = g.place(np.arange(6, dtype=np.float32).reshape(2, 3))
        assert p.tolist() == [[0, 1, 2], [3, 4, 5]] and g.records[-1][5] == ga.POISON_ZERO
        g.check()


def test_other_devices_pass_through():
    """A context guarding another device leaves CPU requests to torch."""
    with ga.GuardedAlloc(ga.POISON_FF, device="cuda:0") as g:
        t = torch.empty(4, dtype=torch.float32)
        u = torch.zeros((2, 2), device="cpu")
        v = torch.empty_like(u)
        assert not g.records and t.shape == (4,) and u.shape == v.shape == (2, 2)


def _overrun_kernel(delta):
    out = torch.empty(10, dtype=torch.float32, device=CPU)  # SITE
    out.fill_(1.0)
    # one element past the end (delta = 10) or before the start (delta = -1)
    out.as_strided((1,), (1,), out.storage_offset() + delta).fill_(3.0)
    return out


SITE_LINE = next(i + 1 for i, l in enumerate(open(THIS)) if l.rstrip().endswith("# SITE"))


@pytest.mark.parametrize("delta,first,last", [(10, 40, 43), (-1, -4, -1)])
def test_overrun_by_one_element_is_caught_and_named(delta, first, last):
    with _guarded(ga.POISON_ZERO) as g:
        torch.empty(3, dtype=torch.float32, device=CPU)  # an innocent neighbour
        _overrun_kernel(delta)
        with pytest.raises(ga.GuardDamage) as err:
            g.check()
    msg = str(err.value)
    assert "1 of 2 guarded buffers" in msg
    assert f"{THIS}:{SITE_LINE}" in msg, msg
    assert "(10,) torch.float32" in msg and f"offsets {first} .. {last}" in msg, msg


def test_placed_input_guards_are_checked_too():
    with _guarded(ga.POISON_FF) as g:
        x = g.place(torch.arange(4, dtype=torch.float32))
        assert torch.isnan(x.as_strided((1,), (1,), x.storage_offset() + 4)).all()  # a read past it: the poison
        g.check()
        x.as_strided((1,), (1,), x.storage_offset() + 4).fill_(0.0)
        with pytest.raises(ga.GuardDamage):
            g.check()


def _reads_unwritten(n):
    """Writes n - 1 of n elements, then sums all n."""
    buf = torch.empty(n, dtype=torch.float32, device=CPU)
    buf[:n - 1] = 1.0
    return float(buf.sum())


def _forgets_to_zero(n):
    """Accumulates into a buffer the caller should have zeroed: correct by
    accident under the zero poison."""
    acc = torch.empty(n, dtype=torch.float32, device=CPU)
    acc += 1.0
    return acc.clone()


def _clean(n):
    buf = torch.empty(n, dtype=torch.float32, device=CPU)
    buf[:] = torch.arange(n, dtype=torch.float32)
    acc = torch.zeros(n, dtype=torch.float32, device=CPU)
    acc += buf
    return acc.clone()


def test_poison_dependence_shows_and_a_clean_function_passes():
    res = {}
    for poison in (ga.POISON_ZERO, ga.POISON_FF):
        with _guarded(poison) as g:
            res[poison] = (_reads_unwritten(8), _forgets_to_zero(8), _clean(8))
            g.check()
    z, f = res[ga.POISON_ZERO], res[ga.POISON_FF]
    assert z[0] == 7.0 and np.isnan(f[0])
    assert bool((z[1] == 1).all()) and torch.isnan(f[1]).all()  # only the 0xFF run notices
    assert np.array_equal(z[2].numpy().view(np.uint32), f[2].numpy().view(np.uint32))
    assert np.array_equal(z[2].numpy(), _clean(8).numpy())


def test_patched_functions_are_restored():
    before = {n: getattr(torch, n) for n in ga.PATCHED}
    with _guarded(ga.POISON_FF):
        assert all(getattr(torch, n) is not before[n] for n in ga.PATCHED)
    assert all(getattr(torch, n) is before[n] for n in ga.PATCHED)
    with pytest.raises(ZeroDivisionError):
        with _guarded(ga.POISON_FF):
            1 / 0
    assert all(getattr(torch, n) is before[n] for n in ga.PATCHED)
    g = _guarded(ga.POISON_ZERO)
    with g:
        with pytest.raises(RuntimeError):
            g.__enter__()
    assert all(getattr(torch, n) is before[n] for n in ga.PATCHED)
    with pytest.raises(ValueError):
        ga.GuardedAlloc(0x5A)
    with ga.context(None, CPU) as u:
        assert torch.empty is before["empty"] and u.place(np.zeros(2)).shape == (2,)
        u.check()


# Every way the package could get tensor memory that the tool would not see.
FORBIDDEN = [
    (r"\.new_(empty|zeros|ones|full|tensor)\b", "Tensor.new_*"),
    (r"\bempty_(strided|permuted|quantized)\b", "torch.empty_strided and kin"),
    (r"\b(full|ones|rand|randn|randint)_like\b", "an unpatched *_like"),
    (r"\bfrom\s+torch\s+import\b(?!\s+nn\s*$)", "from torch import <allocator>"),
    (r"\bimport\s+torch\s+as\b", "torch under another name"),
    (r"(?<![\w.])(?!torch\.)[\w.]+\.(empty|empty_like|zeros|zeros_like|full|ones)\(.*\bdevice\s*=",
     "an allocator reached through another module name"),
    (r"\btorch\.(empty|empty_like|zeros|zeros_like|full|ones)\b(?!\s*\()", "an allocator bound to another name"),
    (r"getattr\(\s*torch\b", "getattr(torch, ...)"),
    (r"\btorch\.(cuda\.)?(Float|Half|BFloat16|Double|Int|Long|Byte|Short|Char|Bool)?Tensor\(", "a legacy constructor"),
]


def _violations(text):
    out = []
    for pat, what in FORBIDDEN:
        for m in re.finditer(pat, text, re.M):
            out.append((text.count("\n", 0, m.start()) + 1, what))
    return out


def test_tripwire_patterns_fire():
    """The tripwire itself: each forbidden spelling is seen, the package's own
    spellings are not."""
    for bad in ("y = x.new_empty(3)", "y = x.new_zeros((2, 2))", "t = torch.empty_strided((2,), (1,), device=d)",
                "from torch import empty", "from torch import nn, zeros", "import torch as th",
                "alloc = torch.empty\n", "f(torch.zeros, 3)", "y = torch.ones_like(x)", "t = torch.FloatTensor(3)",
                "t = th.empty(3, device=dev)", "e = getattr(torch, 'empty')", "t = torch.Tensor(4)"):
        assert _violations(bad), bad
    for ok in ("out = torch.empty((B, 4), dtype=torch.float64, device=x.device)", "from torch import nn",
               "relu = torch.empty_like(out) if want_relu else None", "blob = np.zeros(max(o, 8), np.uint8)",
               "xy = torch.zeros_like(centers)", "P['b'] = torch.full((1,), float(obj_bias))",
               "one = torch.ones(1, device=dev)", "pad = np.empty(3)"):
        assert not _violations(ok), ok


def test_package_allocates_only_by_the_patched_spellings():
    """If this fails, the package has a tensor allocation that a guarded run
    would not poison or guard: extend tests/guarded_alloc.py (PATCHED and the
    argument handling) to cover the new spelling, then allow it here."""
    pkg = os.path.dirname(os.path.abspath(tmr_amd.__file__))
    files = sorted(glob.glob(os.path.join(pkg, "**", "*.py"), recursive=True))
    assert len(files) >= 15
    found, uses = [], 0
    for path in files:
        text = open(path).read()
        uses += len(re.findall(r"\btorch\.(?:empty|empty_like|zeros|zeros_like|full|ones)\(", text))
        found += [f"{os.path.relpath(path, pkg)}:{line}: {what}" for line, what in _violations(text)]
    assert not found, ("tensor allocations the guarded allocator does not patch -- extend "
                       "tests/guarded_alloc.py:\n  " + "\n  ".join(found))
    assert uses >= 80  # the scan reads the real sources (engine.py alone has ~50 sites)
