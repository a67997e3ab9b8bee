"""Poisoned, guard-banded buffers for the kernel tests (imported like _fcn / _x39; no fixture, no conftest).

A kernel owns exactly the bytes of the tensors it is handed.  `guarded(t, fill)` copies an operand into the middle of a
fresh byte arena [guard | payload | guard] whose every byte is `fill`; `Guarded(fill)` makes every allocation of the
provider (its outputs and its workspaces, the latter at exactly the size the library reports) come out of such an arena.
`.check()` then proves that no guard byte moved, and running the same call under two different fills proves that no
output byte comes from memory the kernel was not given: an element that is never written keeps the fill, and an operand
read past its end computes with the fill, so either shows as a difference between the two results.

0xFF is NaN as bf16 and as fp32 (-1 / 255 as an integer), 0xA5 a small finite negative number in both."""
import sys
import types

import torch

GUARD_BYTES = 1 << 20
ALIGN = 256
FILLS = (0xFF, 0xA5)

_live = []                      # the active Guarded contexts, innermost last: guarded() records its arenas there


class _Arena:
    def __init__(self, raw, off, nbytes, fill, label):
        self.raw, self.off, self.nbytes, self.fill, self.label = raw, off, nbytes, fill, label

    def damage(self):
        """offset (relative to the payload's first byte) of the first guard byte that is no longer `fill`, or None"""
        for base, part in ((-self.off, self.raw[:self.off]), (self.nbytes, self.raw[self.off + self.nbytes:])):
            bad = (part != self.fill).nonzero()
            if bad.numel():
                return base + int(bad[0, 0])
        return None


def _extent(shape, strides):
    """elements between the first and one past the last element a dense or strided view touches"""
    if any(s == 0 for s in shape):
        return 0
    return 1 + sum((s - 1) * st for s, st in zip(shape, strides))


def _arena_view(shape, strides, dtype, device, fill, label, zero=False):
    """a [guard | payload | guard] arena filled with `fill` -> (arena, the payload as a view of that shape and strides)"""
    es = torch.empty((), dtype=dtype).element_size()
    nbytes = _extent(shape, strides) * es
    raw = torch.full((GUARD_BYTES + ALIGN + nbytes + GUARD_BYTES,), fill, dtype=torch.uint8, device=device)
    off = GUARD_BYTES + (-(raw.data_ptr() + GUARD_BYTES)) % ALIGN
    payload = raw[off:off + nbytes]
    if zero:
        payload.zero_()
    typed = payload.view(dtype)
    view = typed.as_strided(tuple(shape), tuple(strides), typed.storage_offset())
    assert view.data_ptr() % ALIGN == 0 or nbytes == 0
    return _Arena(raw, off, nbytes, fill, label), view


def guarded(t, fill):
    """`t` copied into a fresh arena on its device: same dtype, shape and strides (contiguous and channels_last survive),
    the payload exactly t's storage extent, on a 256-byte boundary, at least 1 MiB of `fill` on either side"""
    label = "operand %s %s" % (tuple(t.shape), t.dtype)
    arena, view = _arena_view(t.shape, t.stride(), t.dtype, t.device, fill, label)
    view.copy_(t)
    if _live:
        _live[-1]._record(arena)
    else:
        view._guard_arena = arena
    return view


class _TorchProxy(types.ModuleType):
    """`torch` as the patched module sees it: the allocation calls go to the Guarded context, everything else through"""

    def __init__(self, ctx):
        super().__init__("torch")
        self.__dict__["_ctx"] = ctx

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, *a, **kw):
        return self._ctx._alloc(torch.empty, a, kw, False)

    def zeros(self, *a, **kw):
        return self._ctx._alloc(torch.zeros, a, kw, True)

    def empty_like(self, t, **kw):
        kw.setdefault("device", t.device)
        return self._ctx._alloc(torch.empty_like, (t,), kw, False)

    def zeros_like(self, t, **kw):
        kw.setdefault("device", t.device)
        return self._ctx._alloc(torch.zeros_like, (t,), kw, True)


class Guarded:
    """Context manager: while active, torch.empty / empty_like / zeros / zeros_like called from the provider's module
    return views of fresh arenas filled with `fill` (zeros: the payload alone is zeroed), recorded in call order; the
    provider's scratch buffers are set aside, so every workspace is re-allocated inside guards at exactly the size the
    library asks for and holds `fill`.  On exit the scratch buffers come back and the guarded ones are retired the way
    an outgrown scratch buffer is (kept: a launch may still be using them)."""

    def __init__(self, fill, prov=None, module=None):
        self.fill = int(fill)
        if module is None:
            from torchseg_amd import kernels as module
            if prov is None:
                prov = module.provider()
        self.module, self.prov = module, prov
        self.arenas = []

    def _record(self, arena):
        arena.label = "#%d %s" % (len(self.arenas), arena.label)
        self.arenas.append(arena)

    def _alloc(self, fn, a, kw, zero):
        device = torch.device(kw.get("device") or "cpu")
        meta = fn(*[x.to("meta") if isinstance(x, torch.Tensor) else x for x in a], **dict(kw, device="meta"))
        label = "%s %s %s" % (fn.__name__, tuple(meta.shape), meta.dtype)
        arena, view = _arena_view(meta.shape, meta.stride(), meta.dtype, device, self.fill, label, zero)
        self._record(arena)
        return view

    def guarded(self, t):
        return guarded(t, self.fill)

    def adopt(self, *tensors):
        """record the arenas of operands made by guarded() before the context was entered"""
        for t in tensors:
            if t is not None and getattr(t, "_guard_arena", None) is not None:
                self._record(t._guard_arena)
                t._guard_arena = None

    def __enter__(self):
        self._torch = self.module.__dict__["torch"]
        self.module.__dict__["torch"] = _TorchProxy(self)
        if self.prov is not None:
            self._scratch = self.prov.__dict__.get("_scratch_bufs")
            self.prov.__dict__["_scratch_bufs"] = {}
        _live.append(self)
        return self

    def __exit__(self, *exc):
        _live.remove(self)
        self.module.__dict__["torch"] = self._torch
        if self.prov is not None:
            mine = self.prov.__dict__.pop("_scratch_bufs", {})
            self.prov.__dict__.setdefault("_scratch_retired", []).extend(mine.values())
            if self._scratch is not None:
                self.prov.__dict__["_scratch_bufs"] = self._scratch
        return False

    def check(self):
        """every guard byte of every recorded arena still equals the fill"""
        if any(a.raw.is_cuda for a in self.arenas):
            torch.cuda.synchronize()
        for a in self.arenas:
            at = a.damage()
            assert at is None, ("guard of allocation %s (payload %d bytes, fill 0x%02X) damaged at payload offset %d"
                                % (a.label, a.nbytes, a.fill, at))


def raw_bytes(t):
    """the bytes of every element of `t` in logical order, on the CPU: NaN payloads and -0 count"""
    if t is None:
        return None
    c = t.detach().contiguous().cpu()
    return c.reshape(-1).view(torch.uint8) if c.numel() else c.reshape(-1)


def flatten(out):
    """the tensors of a provider method's result (a tensor, a tuple with tensors, ints and Nones), in order"""
    items = out if isinstance(out, (tuple, list)) else (out,)
    return [o for o in items if isinstance(o, torch.Tensor)]


def assert_bit_identical(results, names):
    """results: one provider result per call; every tensor (and every plain value) of each equals the first call's"""
    first = results[0]
    for other, name in zip(results[1:], names[1:]):
        a = first if isinstance(first, (tuple, list)) else (first,)
        b = other if isinstance(other, (tuple, list)) else (other,)
        assert len(a) == len(b), (names[0], name)
        for i, (u, v) in enumerate(zip(a, b)):
            if isinstance(u, (tuple, list)):
                assert_bit_identical([u, v], [names[0], name])
            elif isinstance(u, torch.Tensor):
                assert u.shape == v.shape and u.dtype == v.dtype and u.stride() == v.stride(), (i, names[0], name)
                bu, bv = raw_bytes(u), raw_bytes(v)
                diff = (bu != bv).nonzero()
                assert diff.numel() == 0, ("output %d %s %s: %s and %s differ in %d bytes, first at byte %d"
                                           % (i, tuple(u.shape), u.dtype, names[0], name, diff.shape[0], int(diff[0, 0])))
            else:
                assert u == v, (i, u, v, names[0], name)


def three_calls(fn, operands, prov=None, module=None):
    """fn(*operands) on ordinary tensors, then inside arenas filled with 0xFF and with 0xA5 (operands a list of tensors /
    None / plain values, tuples of those allowed) -> [plain, guarded 0xFF, guarded 0xA5]; asserts that both guarded calls
    left their guards alone and that the three results are bit-identical"""
    def wrap(o, g):
        if isinstance(o, torch.Tensor):
            return g.guarded(o)
        if isinstance(o, (tuple, list)):
            return type(o)(wrap(v, g) for v in o)
        return o

    results = [fn(*operands)]
    names = ["plain"]
    for fill in FILLS:
        with Guarded(fill, prov=prov, module=module) as g:
            out = fn(*[wrap(o, g) for o in operands])
        g.check()
        results.append(out)
        names.append("guarded 0x%02X" % fill)
    assert_bit_identical(results, names)
    return results
