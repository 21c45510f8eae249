"""A poisoning, guard-banded tensor allocator for the length of one test.

The package allocates its outputs, scratch buffers and workspaces with
torch.empty / empty_like / zeros / zeros_like / full / ones, at exactly the
sizes tmr_size returns.  Under torch's caching allocator such memory holds an
earlier test's values of the same kind, and an overrun of a few elements lands
in a neighbouring block and faults nothing.  While a GuardedAlloc context is
active each of those six functions, for a request on the guarded device, gives

    [ GUARD bytes of 0xA5 | payload | GUARD bytes of 0xA5 ]

as ONE uint8 buffer from the real torch.empty, and hands the caller the payload
as a contiguous view of the requested dtype and shape.  The payload of
empty / empty_like is filled with the run's poison byte; zeros / full / ones
hold what was asked for.  GUARD is 64 KiB, so the payload keeps the 256-B
alignment of the real allocation and ends exactly where the post-guard begins
(no rounding of nbytes).  Every buffer stays alive in the context until it
exits: a recycled block would make the guard check meaningless.

    with GuardedAlloc(POISON_FF) as ga:
        x = ga.place(host_array)        # a test's own input, guards = poison
        out = run_the_flow(x)
        ga.check()                      # every guard byte of every buffer

A flow is run under POISON_ZERO and under POISON_FF (NaN for fp32 / bf16 / fp16,
-1 for integers): a result that read memory nobody wrote differs between the
two, a missing zeroing by the caller passes the first and fails the second.
Requests for other devices pass through untouched.  Not a conftest, not a
plugin: tests import it.  Graph capture is out of scope (a poison fill inside a
capture would become part of the graph).
"""
import math
import os
import sys

import torch

GUARD = 64 * 1024
GUARD_BYTE = 0xA5
POISON_ZERO = 0x00
POISON_FF = 0xFF
PATCHED = ("empty", "empty_like", "zeros", "zeros_like", "full", "ones")

_THIS = os.path.abspath(__file__)
_KW = {"dtype", "device", "requires_grad", "memory_format"}


class GuardDamage(AssertionError):
    pass


def _shape(args, kwargs):
    if "size" in kwargs:
        args = (kwargs.pop("size"),)
    if len(args) == 1 and isinstance(args[0], (tuple, list, torch.Size)):
        args = tuple(args[0])
    return tuple(int(a) for a in args)


class GuardedAlloc:
    """See the module docstring.  device: the device whose requests are
    guarded (a CPU device here lets the tool be tested without a GPU)."""

    def __init__(self, poison, device="cuda:0"):
        if poison not in (POISON_ZERO, POISON_FF):
            raise ValueError("the poison byte is 0x00 or 0xFF")
        self.poison = poison
        self.device = torch.device(device)
        self.records = []  # (raw, nbytes, shape, dtype, site, guard byte)
        self._real = None

    # ------------------------------------------------------------ patching
    def __enter__(self):
        if self._real is not None:
            raise RuntimeError("GuardedAlloc is not re-entrant")
        self._real = {n: getattr(torch, n) for n in PATCHED}
        try:
            for n in PATCHED:
                setattr(torch, n, self._wrap(n))
        except BaseException:
            self._restore()
            raise
        return self

    def __exit__(self, *exc):
        self._restore()
        self.records = []
        return False

    def _restore(self):
        for n, f in (self._real or {}).items():
            setattr(torch, n, f)
        self._real = None

    def _ours(self, dev):
        """Whether a request for `dev` (None: torch's default) is guarded."""
        if dev is None:
            dev = torch.get_default_device() if hasattr(torch, "get_default_device") else "cpu"
        dev = torch.device(dev) if not isinstance(dev, int) else torch.device("cuda", dev)
        if dev.type != self.device.type:
            return None
        return dev if dev.index is not None or dev.type == "cpu" else self.device

    def _wrap(self, name):
        real = self._real[name]
        like = name.endswith("_like")

        def fn(*args, **kwargs):
            src = args[0] if like and args else kwargs.get("input")
            dev = kwargs.get("device", src.device if like and src is not None else None)
            dev = self._ours(dev)
            if dev is None or kwargs.get("out") is not None:
                return real(*args, **kwargs)
            kw = dict(kwargs)
            extra = set(kw) - _KW - {"size", "fill_value", "input"}
            if extra or kw.get("requires_grad") or \
                    kw.get("memory_format", torch.contiguous_format) not in (torch.contiguous_format,
                                                                             torch.preserve_format):
                raise NotImplementedError(f"guarded torch.{name}: unsupported arguments {sorted(kw)}; "
                                          "extend tests/guarded_alloc.py")
            value = None
            if like:
                if not src.is_contiguous():
                    raise NotImplementedError(f"guarded torch.{name} of a non-contiguous tensor")
                shape, dtype = tuple(src.shape), kw.get("dtype") or src.dtype
            else:
                rest = list(args)
                if name == "full":
                    value = kw.pop("fill_value") if "fill_value" in kw else rest.pop(1 if "size" not in kw else 0)
                shape = _shape(tuple(rest), kw)
                dtype = kw.get("dtype")
                if dtype is None:
                    dtype = torch.get_default_dtype()
                    if name == "full" and not isinstance(value, float):
                        dtype = torch.bool if isinstance(value, bool) else torch.int64
            if name.startswith("zeros"):
                value = 0
            elif name == "ones":
                value = 1
            return self._alloc(shape, dtype, dev, value, GUARD_BYTE, sys._getframe(1))

        fn.__name__ = f"guarded_{name}"
        return fn

    # ---------------------------------------------------------- allocation
    def _alloc(self, shape, dtype, dev, value, guard_byte, frame):
        while frame is not None and os.path.abspath(frame.f_code.co_filename) == _THIS:
            frame = frame.f_back
        site = f"{frame.f_code.co_filename}:{frame.f_lineno}" if frame is not None else "?"
        empty = self._real["empty"] if self._real is not None else torch.empty
        esize = empty(0, dtype=dtype).element_size()
        nbytes = math.prod(shape) * esize
        raw = empty(GUARD + nbytes + GUARD, dtype=torch.uint8, device=dev)
        raw[:GUARD].fill_(guard_byte)
        raw[GUARD + nbytes:].fill_(guard_byte)
        pay = raw[GUARD:GUARD + nbytes]
        if value is None:
            pay.fill_(self.poison)
        t = pay.view(dtype).view(shape)
        if value is not None:
            t.fill_(value)
        assert t.is_contiguous() and t.storage_offset() * esize == GUARD
        self.records.append((raw, nbytes, tuple(shape), dtype, site, guard_byte))
        return t

    def place(self, t, dtype=None):
        """A test's own input (tensor or array, any device) copied into a
        guarded buffer on the guarded device.  Its guards hold the POISON byte:
        an out-of-range read that reaches a result shows as a dependence on
        the poison (check() still verifies that nothing wrote them)."""
        t = torch.as_tensor(t)
        if dtype is not None:
            t = t.to(dtype)
        g = self._alloc(tuple(t.shape), t.dtype, self.device, None, self.poison, sys._getframe(1))
        g.copy_(t)
        return g

    # --------------------------------------------------------------- check
    def check(self):
        """Synchronise, then assert every guard byte of every buffer made in
        the context.  A failure names each damaged buffer's shape, dtype and
        allocation site and the first and last damaged byte offsets relative
        to the payload (negative: before it; >= its size: past its end)."""
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        flags = [raw.as_strided((2, GUARD), (GUARD + nbytes, 1)).ne(byte).any()
                 for raw, nbytes, _, _, _, byte in self.records]
        if not flags:
            return
        bad = torch.stack(flags).cpu().nonzero().flatten().tolist()
        if not bad:
            return
        lines = []
        for i in bad:
            raw, nbytes, shape, dtype, site, byte = self.records[i]
            pre = raw[:GUARD].ne(byte).nonzero().flatten().cpu() - GUARD
            post = raw[GUARD + nbytes:].ne(byte).nonzero().flatten().cpu() + nbytes
            off = torch.cat([pre, post])
            lines.append(f"  {tuple(shape)} {dtype} ({nbytes} B) allocated at {site}: {off.numel()} guard bytes "
                         f"damaged, payload-relative offsets {int(off.min())} .. {int(off.max())}")
        raise GuardDamage(f"{len(bad)} of {len(self.records)} guarded buffers were written outside their "
                          "payload:\n" + "\n".join(lines))


class Unguarded:
    """The same interface with torch's own allocator: the reference run."""

    poison = None

    def __init__(self, device="cuda:0"):
        self.device = torch.device(device)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False

    def place(self, t, dtype=None):
        t = torch.as_tensor(t)
        return (t if dtype is None else t.to(dtype)).to(self.device).contiguous()

    def check(self):
        pass


def context(poison, device="cuda:0"):
    """GuardedAlloc(poison), or the unguarded stand-in for poison None."""
    return Unguarded(device) if poison is None else GuardedAlloc(poison, device)
