"""Memory-footprint guard for the kernels' buffers: where a kernel reads and writes, not what it computes.

Every buffer a kernel writes is allocated by the Python hosts with ``torch.empty`` / ``zeros`` / ``ones`` / ``full`` (or
their ``_like`` / ``new_*`` forms).  ``guarded(fill)`` replaces those factories for its duration.  A call made from the
package then gets one flat byte buffer ``[guard | payload | guard]`` and receives the payload as a view of the requested
shape and dtype, its first byte on a 256-byte boundary like a real allocation's:

* the guards hold a seeded random byte pattern; after the case ``check()`` synchronises once and compares them with
  ``torch.equal``.  A damaged guard is reported with the file and line of the allocation, the side, the first and last
  damaged byte offset (relative to the payload: negative = in front of it, >= 0 = bytes past its end) and the byte count;
* a ``torch.empty`` payload is filled with ``fill`` bytes: 0xFF (NaN in fp16 / bf16 / fp32 / fp64, -1 as an integer) or
  0x00.  ``zeros`` / ``ones`` / ``full`` payloads get the value they asked for.  A kernel that reads scratch before it
  writes it therefore computes from two different contents in the two runs of a case, and the results differ;
* ``guard_input(t)`` copies a test-made operand into a guarded allocation of the same strides (the gaps of a strided view
  hold ``fill`` too), so an out-of-bounds read meets poison, and keeps a snapshot: ``check()`` proves a ``const`` operand
  was not written;
* CPU allocations and calls from outside the package pass through untouched.  A device allocation made by the package
  with arguments the wrapper does not understand (``out=``, ``names=``, a sparse layout, ...) passes through as well but
  is COUNTED, and ``check()`` fails on a non-zero count: nothing is left unguarded silently.

Guard size, per side: at least 64 KiB and at least 256 rows of the tensor's own row pitch (last-dimension stride in bytes
times the last dimension's size).  The largest output tile in the library is the 256 x 288 GEMM tile, so a whole stray
row-block of any kernel lands inside a guard.  A tensor of fewer than two dimensions (the byte workspaces of the mesh
stages, count-sized index arrays) has no rows: its pitch is one element, i.e. the 64 KiB floor decides - 256 copies of a
multi-hundred-megabyte workspace on either side would not fit the card.

What this cannot see:

* a stray store farther from the payload than the guard, or one that lands in the interior of ANOTHER live tensor: the
  guards of that tensor stay intact.  Such a store surfaces only if it changes a result, through the comparison of the
  two fills and of the guarded with the unguarded run (``hold``);
* a stray store whose byte equals the pattern byte it overwrites (1 in 256 per byte);
* reads that stay inside the payload but belong to another row (a wrong-row read is an arithmetic error, and the
  contract tests own those);
* allocations that never pass through the intercepted factories (``torch.tensor(...).to(dev)``, ``.clone()``, the results
  of torch ops): they are torch's own, not kernel destinations of this library, except where a host passes one to a
  kernel as an output - the hosts do not.

The module is plain (no fixtures, no conftest hook) and device-agnostic: ``guarded(fill, any_device=True)`` guards CPU
tensors too, which is how tests/test_footprint_cpu.py proves the mechanism without a GPU.
"""
from __future__ import annotations

import math
import operator
import sys
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import torch

GUARD_MIN = 64 << 10     # bytes per side, at least
GUARD_ROWS = 256         # rows of the tensor's own pitch per side, at least (the 256 x 288 GEMM tile)
ALIGN = 256              # payload alignment (what the caching allocator gives at least)
PACKAGE = "topia_xl_amd"
FILLS = (0xFF, 0x00)

_OPS = ("empty", "zeros", "ones", "full")
_REAL = {}               # the real factories, captured once at import (guarded() is not re-entrant)
for _op in _OPS:
    _REAL[_op] = getattr(torch, _op)
    _REAL[_op + "_like"] = getattr(torch, _op + "_like")
    _REAL["new_" + _op] = getattr(torch.Tensor, "new_" + _op)

_active: Optional["Guard"] = None


class FootprintError(AssertionError):
    """check() found a damaged guard, a written const operand or an unguarded device allocation."""


class _NotUnderstood(Exception):
    pass


def _itemsize(dtype: torch.dtype) -> int:
    return torch._utils._element_size(dtype)


def _size_of(args: Sequence) -> Tuple[int, ...]:
    if len(args) == 1 and isinstance(args[0], (tuple, list, torch.Size)):
        args = args[0]
    try:
        return tuple(operator.index(a) for a in args)
    except TypeError:
        raise _NotUnderstood(f"size {args!r}") from None


def _device_of(dev) -> torch.device:
    if dev is None:
        dev = torch.get_default_device() if hasattr(torch, "get_default_device") else "cpu"
    dev = torch.device(dev)
    if dev.type == "cuda" and dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    return dev


def _parse(mode: str, op: str, args: tuple, kwargs: dict):
    """-> (shape, strides or None, dtype, device, value or None) of one factory call, or _NotUnderstood."""
    kw = dict(kwargs)
    if kw.pop("requires_grad", False) or kw.pop("pin_memory", False):
        raise _NotUnderstood("requires_grad / pin_memory")
    if kw.pop("layout", torch.strided) is not torch.strided:
        raise _NotUnderstood("layout")
    fmt = kw.pop("memory_format", None)
    args = list(args)
    like = None
    if mode == "factory":
        if "size" in kw:
            args.insert(0, kw.pop("size"))
    else:
        like = args.pop(0) if args else kw.pop("input", None)
        if not isinstance(like, torch.Tensor) or like.layout is not torch.strided:
            raise _NotUnderstood("source tensor")
        if mode == "new" and "size" in kw:
            args.insert(0, kw.pop("size"))
    value = None
    if op == "full":
        if "fill_value" in kw:
            value = kw.pop("fill_value")
        elif mode == "like" and len(args) == 1:
            value = args.pop()
        elif mode != "like" and len(args) == 2:
            value = args.pop()
        else:
            raise _NotUnderstood("fill value")
        if isinstance(value, torch.Tensor):
            value = value.item()
        if not isinstance(value, (bool, int, float)):
            raise _NotUnderstood("fill value type")
    elif op == "ones":
        value = 1
    elif op == "zeros":
        value = 0
    dtype = kw.pop("dtype", None)
    device = kw.pop("device", None)
    if kw:
        raise _NotUnderstood("arguments " + ", ".join(sorted(kw)))
    strides = None
    if mode == "like":
        if args:
            raise _NotUnderstood("positional arguments")
        shape = tuple(like.shape)
        if fmt not in (None, torch.preserve_format, torch.contiguous_format):
            raise _NotUnderstood("memory_format")
        if fmt is not torch.contiguous_format and not like.is_contiguous() and like.numel() \
                and torch._prims_common.is_non_overlapping_and_dense(like):
            strides = tuple(like.stride())          # a permuted dense source: the result keeps its strides
    else:
        if fmt not in (None, torch.contiguous_format):
            raise _NotUnderstood("memory_format")
        shape = _size_of(args)
    if any(s < 0 for s in shape):
        raise _NotUnderstood("negative size")
    if dtype is None:
        if like is not None:
            dtype = like.dtype
        elif op == "full" and isinstance(value, bool):
            dtype = torch.bool
        elif op == "full" and isinstance(value, int):
            dtype = torch.int64
        else:
            dtype = torch.get_default_dtype()
    if dtype.is_complex or not isinstance(dtype, torch.dtype):
        raise _NotUnderstood("dtype")
    device = _device_of(device) if device is not None or like is None else like.device
    return shape, strides, dtype, device, value


def _copy_view(dst: torch.Tensor, src: torch.Tensor) -> None:
    """dst.copy_(src) for two views of equal strides; a broadcast dimension (stride 0) is written once."""
    for d, (n, st) in enumerate(zip(src.shape, src.stride())):
        if st == 0 and n > 1:
            dst, src = dst.narrow(d, 0, 1), src.narrow(d, 0, 1)
    dst.copy_(src)


class _Record:
    __slots__ = ("site", "base", "lo", "hi", "want_l", "want_r", "snapshot", "const", "what")

    def payload(self) -> torch.Tensor:
        return self.base[self.lo:self.hi]


class InputHandle:
    """A test-made operand inside a guarded allocation: ``.t`` is the tensor to pass to the kernel."""

    def __init__(self, t: torch.Tensor, rec: Optional[_Record], name: str):
        self.t, self._rec, self.name = t, rec, name

    def changed_bytes(self) -> int:
        if self._rec is None:
            return 0
        return int((self._rec.payload() != self._rec.snapshot).sum())

    def assert_unchanged(self) -> None:
        n = self.changed_bytes()
        if n:
            raise FootprintError(f"const operand {self.name} ({self._rec.site}) was written: {n} bytes differ from the snapshot")


class Guard:
    def __init__(self, fill: int, packages: Sequence[str] = (PACKAGE,), any_device: bool = False, seed: int = 0x5EED,
                 active: bool = True):
        if fill not in FILLS:
            raise ValueError("fill must be 0xFF or 0x00")
        self.fill, self.packages, self.any_device, self.seed, self.active = fill, tuple(packages), any_device, seed, active
        self.records: List[_Record] = []
        self.bypassed: List[Tuple[str, str]] = []
        self._pools: Dict[torch.device, List[torch.Tensor]] = {}
        self._n = 0
        self._saved = []

    # ------------------------------------------------------------------ interception
    def _mine(self, frame) -> bool:
        name = frame.f_globals.get("__name__", "")
        return any(name == p or name.startswith(p + ".") for p in self.packages)

    def _wants(self, device: torch.device) -> bool:
        return device.type == "cuda" or (self.any_device and device.type == "cpu")

    def _wrap(self, mode: str, op: str, real: Callable) -> Callable:
        guard = self

        def factory(*args, **kwargs):
            frame = sys._getframe(1)
            if not guard._mine(frame):
                return real(*args, **kwargs)
            site = f"{frame.f_code.co_filename}:{frame.f_lineno}"
            try:
                shape, strides, dtype, device, value = _parse(mode, op, args, kwargs)
            except _NotUnderstood as e:
                out = real(*args, **kwargs)
                if isinstance(out, torch.Tensor) and guard._wants(out.device):
                    guard.bypassed.append((site, f"torch {mode} {op}: {e}"))
                return out
            if not guard._wants(device):
                return real(*args, **kwargs)
            return guard._alloc(shape, strides, dtype, device, value, site, op)
        factory.__name__ = real.__name__ if hasattr(real, "__name__") else op
        return factory

    def __enter__(self) -> "Guard":
        global _active
        if _active is not None:
            raise RuntimeError("guarded() is not re-entrant")
        _active = self
        if self.active:
            for op in _OPS:
                for mode, owner, name in (("factory", torch, op), ("like", torch, op + "_like"), ("new", torch.Tensor, "new_" + op)):
                    self._saved.append((owner, name, name in vars(owner), vars(owner).get(name)))
                    setattr(owner, name, self._wrap(mode, op, _REAL[name]))
        return self

    def _restore(self) -> None:
        global _active
        for owner, name, own, old in reversed(self._saved):
            if own:
                setattr(owner, name, old)
            else:
                delattr(owner, name)          # (an attribute inherited from the C base class: uncover it again)
        self._saved = []
        _active = None

    def __exit__(self, et, ev, tb) -> bool:
        self._restore()
        if et is None:
            self.check()
        return False

    # ------------------------------------------------------------------ allocation
    def _pattern(self, device: torch.device, n: int) -> torch.Tensor:
        pools = self._pools.setdefault(device, [])
        if not pools or pools[-1].numel() < n:
            gen = torch.Generator().manual_seed(self.seed + len(pools))
            size = max(16 << 20 if device.type == "cuda" else 1 << 20, 2 * n)
            pools.append(torch.randint(0, 256, (size,), dtype=torch.uint8, generator=gen).to(device))
        pool = pools[-1]
        self._n += 1
        off = (self._n * 7919) % (pool.numel() - n + 1)
        return pool[off:off + n]

    def prime(self, device) -> None:
        """Upload the guard pattern of `device` now (a blocking copy) instead of at the first allocation: tests/streamorder.py
        allocates behind a blocked stream, where the host must not wait."""
        self._pattern(_device_of(device), 1)

    def _alloc(self, shape, strides, dtype, device, value, site: str, what: str, span: Optional[int] = None) -> torch.Tensor:
        """`span`: elements of the payload when the view is strided (guard_input); default the product of `shape`."""
        item = _itemsize(dtype)
        numel = math.prod(shape) if span is None else span
        nbytes = numel * item
        last_stride = 1 if strides is None else strides[-1]
        pitch = shape[-1] * last_stride * item if len(shape) >= 2 else item
        g = -(-max(GUARD_MIN, GUARD_ROWS * pitch) // ALIGN) * ALIGN
        base = _REAL["empty"](g + nbytes + g + ALIGN, dtype=torch.uint8, device=device)
        rec = _Record()
        rec.site, rec.base, rec.what, rec.snapshot, rec.const = site, base, what, None, False
        rec.lo = g + (-(base.data_ptr() + g)) % ALIGN
        rec.hi = rec.lo + nbytes
        rec.want_l = self._pattern(device, rec.lo)
        rec.want_r = self._pattern(device, base.numel() - rec.hi)
        base[:rec.lo].copy_(rec.want_l)
        base[rec.hi:].copy_(rec.want_r)
        flat = base[rec.lo:rec.hi].view(dtype) if nbytes else _REAL["empty"](0, dtype=dtype, device=device)
        if value is None or span is not None:
            base[rec.lo:rec.hi].fill_(self.fill)
        else:
            flat.fill_(value)
        self.records.append(rec)
        if strides is not None:
            return flat.as_strided(shape, strides)
        return flat.view(shape)

    def _site(self, depth: int = 2) -> str:
        f = sys._getframe(depth)
        return f"{f.f_code.co_filename}:{f.f_lineno}"

    def empty(self, *size, dtype: torch.dtype, device) -> torch.Tensor:
        """A guarded, `fill`-poisoned destination made by the test itself (an `out=` argument, a workspace)."""
        shape = _size_of(size)
        if not self.active:
            return _REAL["empty"](shape, dtype=dtype, device=device)
        return self._alloc(shape, None, dtype, _device_of(device), None, self._site(), "empty")

    def guard_input(self, t: torch.Tensor, name: str = "", const: bool = True) -> InputHandle:
        """Copy `t` into a guarded allocation with the same strides.  const=False: a documented in-place operand (not
        compared with its snapshot by check(), still guarded on both sides)."""
        if any(s < 0 for s in t.stride()):
            raise ValueError("guard_input: negative strides")
        span = 1 + sum((n - 1) * s for n, s in zip(t.shape, t.stride())) if t.numel() else 0
        if not self.active or not self._wants(t.device):
            flat = _REAL["zeros"](span, dtype=t.dtype, device=t.device)
            c = flat.as_strided(tuple(t.shape), tuple(t.stride()))
            _copy_view(c, t)
            return InputHandle(c, None, name)
        site = self._site()
        c = self._alloc(tuple(t.shape), tuple(t.stride()), t.dtype, t.device, None, site, "input " + name, span=span)
        _copy_view(c, t)
        rec = self.records[-1]
        rec.snapshot, rec.const = rec.payload().clone(), const
        return InputHandle(c, rec, name or site)

    # ------------------------------------------------------------------ the verdict
    def damaged(self) -> List[str]:
        out = []
        for rec in self.records:
            for side, got, want, origin in (("front", rec.base[:rec.lo], rec.want_l, -rec.lo),
                                            ("back", rec.base[rec.hi:], rec.want_r, 0)):
                if torch.equal(got, want):
                    continue
                bad = (got != want).nonzero().flatten()
                out.append(f"{rec.what} allocated at {rec.site}: {side} guard damaged, {bad.numel()} bytes, "
                           f"offsets {int(bad[0]) + origin} .. {int(bad[-1]) + origin} relative to the payload's "
                           f"{'first byte' if side == 'front' else 'end'} (payload {rec.hi - rec.lo} bytes)")
        return out

    def written_inputs(self) -> List[str]:
        out = []
        for rec in self.records:
            if rec.const and rec.snapshot is not None and not torch.equal(rec.payload(), rec.snapshot):
                n = int((rec.payload() != rec.snapshot).sum())
                out.append(f"const operand '{rec.what}' ({rec.site}) was written: {n} bytes differ from the snapshot")
        return out

    def check(self) -> None:
        if torch.cuda.is_available() and any(r.base.is_cuda for r in self.records):
            torch.cuda.synchronize()
        problems = self.damaged() + self.written_inputs()
        problems += [f"unguarded device allocation at {site} ({why})" for site, why in self.bypassed]
        if problems:
            raise FootprintError(f"{len(problems)} footprint violation(s):\n  " + "\n  ".join(problems))


def guarded(fill: int, packages: Sequence[str] = (PACKAGE,), any_device: bool = False) -> Guard:
    """Context manager: intercept the allocations of `packages` for its duration; check() runs on a clean exit."""
    return Guard(fill, packages, any_device)


def unguarded() -> Guard:
    """The same interface with nothing intercepted: the plain call a guarded case is compared with."""
    return Guard(0x00, active=False)


def guard_input(t: torch.Tensor, name: str = "", const: bool = True) -> InputHandle:
    if _active is None:
        raise RuntimeError("guard_input outside guarded()")
    return _active.guard_input(t, name, const)


def check() -> None:
    if _active is None:
        raise RuntimeError("check outside guarded()")
    _active.check()


# ---------------------------------------------------------------------- bitwise comparison of results
def _flatten(x, prefix: str, out: dict) -> None:
    if isinstance(x, torch.Tensor):
        out[prefix or "result"] = x
    elif isinstance(x, dict):
        for k, v in x.items():
            _flatten(v, f"{prefix}.{k}" if prefix else str(k), out)
    elif isinstance(x, (tuple, list)):
        for i, v in enumerate(x):
            _flatten(v, f"{prefix}[{i}]", out)
    elif x is not None:
        out[prefix or "result"] = x


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Bit-identical (NaN payloads and signed zeros included), any strides."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.numel() == 0:
        return True
    a, b = a.contiguous().view(-1), b.contiguous().view(-1)
    return torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def differences(a, b) -> List[str]:
    fa, fb = {}, {}
    _flatten(a, "", fa)
    _flatten(b, "", fb)
    out = [f"{k}: present in one run only" for k in sorted(set(fa) ^ set(fb))]
    for k in fa.keys() & fb.keys():
        x, y = fa[k], fb[k]
        if isinstance(x, torch.Tensor) and isinstance(y, torch.Tensor):
            if not same_bits(x, y):
                if x.shape != y.shape or x.dtype != y.dtype:
                    out.append(f"{k}: {tuple(x.shape)} {x.dtype} vs {tuple(y.shape)} {y.dtype}")
                else:
                    n = int((x.contiguous().view(-1).view(torch.uint8) != y.contiguous().view(-1).view(torch.uint8)).sum())
                    out.append(f"{k}: {n} of {x.numel() * x.element_size()} bytes differ")
        elif x != y:
            out.append(f"{k}: {x!r} vs {y!r}")
    return sorted(out)


def hold(case: Callable[[Guard], object], packages: Sequence[str] = (PACKAGE,), any_device: bool = False):
    """Run `case(g)` under both fills and once unguarded.  Asserts (a) intact guards, (b) unchanged const inputs and a
    bypass count of 0 (check() on leaving each guarded run), (c) results bit-identical between the fills, (d) and to the
    unguarded call.  `case` returns its outputs and documented in-place operands (tensor, or nested tuple / list / dict;
    plain numbers such as counts are compared with ==).  Returns the unguarded result."""
    res = []
    for fill in FILLS:
        with Guard(fill, packages, any_device) as g:
            res.append(case(g))
    with unguarded() as g:
        plain = case(g)
    d = differences(res[0], res[1])
    if d:
        raise FootprintError("results depend on the contents of torch.empty scratch (fill 0xFF vs 0x00):\n  " + "\n  ".join(d))
    d = differences(res[0], plain)
    if d:
        raise FootprintError("guarded and unguarded results differ:\n  " + "\n  ".join(d))
    return plain
