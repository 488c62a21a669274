"""Stream-order probe for the entry points: WHERE a call enqueues its work and whether the host waits, not what it computes.

include/primx_hip.h, boundary rules: "Work is enqueued on `stream` and is asynchronous with respect to the host."  A launch
that goes to stream 0 by mistake, a memset or read-back on another stream than the launches around it, or a stray host
synchronisation is invisible to a test on the default stream with finished inputs.  `run()` makes each of them visible
deterministically, not as a race:

* the reference result is computed once on the default stream with nothing else in flight;
* the measured call runs under ``torch.cuda.stream(s)`` for a side stream `s` (non-blocking with respect to stream 0), while
  BOTH streams are blocked by a sleep kernel (``torch.cuda._sleep``, calibrated with events): a long one on stream 0, a short
  one on `s`;
* the operands are produced late: behind the blocker of `s` the clean values are copied into staging buffers that hold poison
  until then (0xFF bytes = NaN for floating types and uint8 masks; zero for integer tensors, which the kernels use as
  indices - a misordered launch must read a wrong value, never an address outside its buffers);
* the call runs inside ``footprint.guarded(0xFF)``: every ``torch.empty`` output and scratch buffer of the package holds NaN
  bytes, written on `s` as well, and a consumer on `s` clones every output and in-place operand right after the call.

Verdict, after ``s.synchronize()``:

(a) ORDER: the consumer's copies equal the reference bit for bit.  Work that went to any other stream either ran before the
    producer (and read poison) or still waits behind stream 0's blocker (and the consumer read poison output).
(b) CONCLUSIVE: the event recorded behind stream 0's blocker has not completed when the consumer has.  Otherwise the blocker was
    too short or something synchronised the device: the case is INCONCLUSIVE - it does not pass.
(c) ASYNCHRONY: for a call that documents no host synchronisation, the event recorded behind the blocker of `s` has not
    completed when the Python call returns: the host came back before its inputs existed.  A loop of many steps asserts that
    per step: ``probe.step()`` puts a fresh short blocker in front of the step and ``probe.returned()`` looks at it.

Blocker lengths come from measurements of the case itself (`Blocker`, `run`): the blocker of `s` from the host time of a warm-up
run of the same case on `s`, stream 0's from the wall time of that whole warm-up (blockers of `s` included) times a margin;
when (b) says it was too short the case is repeated ONCE with a longer one.  The warm-up uses other input values (stale memory
cannot hold the right answer) and leaves the caching allocator with every block the measured run asks for (no hipMalloc behind
the blockers).

The module is plain - no fixtures, no conftest hook - and `classify` / `Report` need no GPU (tests/test_streamorder_cpu.py).
"""
from __future__ import annotations

import re
import time
from typing import Callable, Dict, List, Optional, Sequence

import torch

from tests import footprint as fp

OK, ORDER, INCONCLUSIVE, SYNCHRONISED = "ok", "order violation", "inconclusive", "host synchronisation"
CAP_MS = 4000.0            # no blocker is longer than this: a case takes a few seconds at the most
MARGINS = (3.0, 10.0)      # stream 0's blocker = margin x the warm-up's wall time (+ FLOOR_MS); the second only after (b) failed
FLOOR_MS = 20.0
S_MIN_MS, S_MAX_MS = 10.0, 400.0


# ---------------------------------------------------------------------- the verdict (no GPU needed)
def classify(differences: Sequence[str], null_gate_done: bool, late_returns: Sequence[bool], must_sync: bool) -> str:
    """`differences`: footprint.differences(consumer copies, reference); `null_gate_done`: stream 0's gate event had completed
    when the consumer finished; `late_returns`: one flag per probed return (the call's, or each step's of a loop) - True when
    the gate of `s` had already completed, i.e. the host had waited for the stream; `must_sync`: the case documents a host
    synchronisation, so (c) is not asked.  A difference is a finding whatever else happened; without one an elapsed stream-0
    blocker proves nothing."""
    if differences:
        return ORDER
    if null_gate_done:
        return INCONCLUSIVE
    if not must_sync and any(late_returns):
        return SYNCHRONISED
    return OK


class Report:
    def __init__(self, name: str, differences: Sequence[str], null_gate_done: bool, late_returns: Sequence[bool], must_sync: bool,
                 s_ms: float = 0.0, null_ms: float = 0.0, host_ms: float = 0.0, attempts: int = 1):
        self.name, self.differences, self.null_gate_done = name, list(differences), bool(null_gate_done)
        self.late_returns, self.must_sync = [bool(x) for x in late_returns], bool(must_sync)
        self.s_ms, self.null_ms, self.host_ms, self.attempts = s_ms, null_ms, host_ms, attempts
        self.verdict = classify(self.differences, self.null_gate_done, self.late_returns, self.must_sync)

    def message(self) -> str:
        head = f"{self.name}: {self.verdict}"
        if self.verdict == ORDER:
            return (head + " - (a) the results behind the late producer differ from the default-stream reference: a launch, memset "
                    "or copy went to another stream than the one given\n  " + "\n  ".join(self.differences))
        if self.verdict == INCONCLUSIVE:
            return (head + f" - (b) stream 0's blocker ({self.null_ms:.0f} ms) had ended when the consumer finished: too short, or "
                    "something synchronised the whole device; this proves nothing and does not pass")
        if self.verdict == SYNCHRONISED:
            n = sum(self.late_returns)
            return (head + f" - (c) the host waited for the stream in {n} of {len(self.late_returns)} probed calls: the blocker of "
                    f"the side stream ({self.s_ms:.0f} ms) had ended at the return, and no synchronisation is documented")
        return head

    def line(self) -> str:
        """One line for the log: the blocker times that were needed."""
        return (f"streamorder {self.name}: {self.verdict}; blocker {self.s_ms:.0f} ms on the side stream, {self.null_ms:.0f} ms on "
                f"stream 0, host {self.host_ms:.1f} ms, {len(self.late_returns)} probed return(s), attempt {self.attempts}"
                + (", synchronising" if self.must_sync else ""))


def stream_prototypes(header_text: str) -> List[str]:
    """Names of every prototype of include/primx_hip.h with a `void* stream` parameter."""
    text = re.sub(r"/\*.*?\*/", "", header_text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    protos = re.findall(r"\b(primx_\w+)\s*\(([^;{}()]*)\)\s*;", text)
    return [name for name, args in protos if re.search(r"\bvoid\s*\*\s*stream\b", args)]


# ---------------------------------------------------------------------- blockers
class Blocker:
    """torch.cuda._sleep in milliseconds: two timed sleeps on the current stream give cycles per millisecond (made once per test
    module; plain compute - nothing waits on it forever)."""

    def __init__(self):
        if not hasattr(torch.cuda, "_sleep"):
            raise RuntimeError("torch.cuda._sleep is missing from this torch build")
        torch.cuda._sleep(1000)                                    # (loads the kernel)
        t = [self._time(c) for c in (2_000_000, 20_000_000)]
        self.cycles_per_ms = (20_000_000 - 2_000_000) / max(t[1] - t[0], 1e-3)

    @staticmethod
    def _time(cycles: int) -> float:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        torch.cuda._sleep(cycles)
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def sleep(self, ms: float) -> None:
        """Enqueue `ms` milliseconds of sleep on the current stream."""
        torch.cuda._sleep(max(int(min(ms, CAP_MS) * self.cycles_per_ms), 1))


class Probe:
    """Handed to a case's `call`: a loop brackets each step with `step()` / `returned()`; everything else ignores it.  On the
    reference and warm-up runs `returned()` records nothing that is judged."""

    def __init__(self, blocker: Optional[Blocker], ms: float):
        self.blocker, self.ms, self.late, self._gate = blocker, ms, [], None

    def step(self) -> None:
        """A fresh short blocker on the current stream in front of the next step."""
        if self.blocker is not None:
            self.blocker.sleep(self.ms)
            self._gate = torch.cuda.Event()
            self._gate.record()

    def returned(self) -> None:
        """The step's Python call has returned: had the host waited for its blocker?"""
        if self._gate is not None:
            self.late.append(self._gate.query())
            self._gate = None


# ---------------------------------------------------------------------- one case
def _poison(t: torch.Tensor) -> None:
    if t.dtype in (torch.int16, torch.int32, torch.int64):
        t.zero_()                                                  # index tensors: a wrong but addressable value
    else:
        t.view(torch.uint8).fill_(0xFF)


def _snapshot(x):
    if isinstance(x, torch.Tensor):
        return x.clone()
    if isinstance(x, dict):
        return {k: _snapshot(v) for k, v in x.items()}
    if isinstance(x, (tuple, list)):
        return [_snapshot(v) for v in x]
    return x


def _check_inputs(vals: Dict[str, torch.Tensor], other: Dict[str, torch.Tensor]) -> None:
    for k, v in vals.items():
        if not (isinstance(v, torch.Tensor) and v.is_cuda and v.is_contiguous() and v.dim() >= 1):
            raise ValueError(f"input {k}: `make` returns contiguous device tensors of at least one dimension (views are taken in `call`)")
        w = other.get(k)
        if w is None or w.shape != v.shape or w.dtype != v.dtype:
            raise ValueError(f"input {k}: the warm-up values make(1) must have the shape and dtype of make(0)")


def run(name: str, make: Callable[[int], Dict[str, torch.Tensor]], call: Callable, stream: "torch.cuda.Stream", blocker: Blocker,
        setup: Optional[Callable[[], object]] = None, must_sync: bool = False, null_ms: Optional[float] = None) -> Report:
    """`make(k)` -> dict of contiguous device tensors, other values for another k; `setup()` -> a context object made before the
    blockers (a FRESH module instance, whose lazy caches then fill behind them), or None; `call(ctx, inputs, probe)` -> outputs
    and documented in-place operands (tensor / nested tuple, list, dict; plain numbers compare with ==).  `null_ms`: overrides
    stream 0's blocker (the positive control of (b))."""
    dev = torch.device("cuda", torch.cuda.current_device())
    null = torch.cuda.default_stream()
    clean, other = make(0), make(1)
    _check_inputs(clean, other)
    torch.cuda.synchronize()

    # the reference: default stream, nothing else in flight
    ctx = setup() if setup is not None else None
    ins = {k: v.clone() for k, v in clean.items()}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ref = _snapshot(call(ctx, ins, Probe(None, 0.0)))
    host_ref = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    del ctx, ins

    with torch.cuda.stream(stream):
        stage = {k: torch.empty_like(v) for k, v in clean.items()}  # (allocated on `stream`, reused by both runs below)

    def attempt(values, s_ms: float, n_ms: Optional[float]):
        with torch.cuda.stream(stream):
            ctx = setup() if setup is not None else None
            for t in stage.values():
                _poison(t)
            guard = fp.Guard(0xFF)
            guard.prime(dev)                                        # the guard pattern is uploaded now, not behind the blockers
            torch.cuda.synchronize()
            null_gate, s_gate = torch.cuda.Event(), torch.cuda.Event()
            w0 = time.perf_counter()
            if n_ms is not None:
                with torch.cuda.stream(null):
                    blocker.sleep(n_ms)
                    null_gate.record()
            blocker.sleep(s_ms)
            s_gate.record()
            for k, t in stage.items():                              # the late producer
                t.copy_(values[k])
            probe = Probe(blocker, s_ms)
            with guard:
                h0 = time.perf_counter()
                out = call(ctx, stage, probe)
                late = s_gate.query()
                host = (time.perf_counter() - h0) * 1e3
                got = _snapshot(out)                                # the consumer
                stream.synchronize()
                null_done = null_gate.query() if n_ms is not None else False
                wall = (time.perf_counter() - w0) * 1e3
                # (leaving the guard synchronises the device for its own check: stream 0's blocker ends there)
            # (a case that probes its steps is judged by them: a loop may synchronise once before its first step)
            return got, null_done, (probe.late or [late]), host, wall

    s_ms = min(max(S_MIN_MS, 2.0 * host_ref), S_MAX_MS)
    _, _, _, host, wall = attempt(other, s_ms, None)               # warm-up: other values, no blocker on stream 0
    s_ms = min(max(S_MIN_MS, 3.0 * host), S_MAX_MS)
    rep = None
    for i, margin in enumerate(MARGINS if null_ms is None else (None,)):
        n_ms = null_ms if null_ms is not None else min(margin * (wall + s_ms) + FLOOR_MS, CAP_MS)
        got, null_done, late, host, _ = attempt(clean, s_ms, n_ms)
        rep = Report(name, fp.differences(got, ref), null_done, late, must_sync, s_ms, n_ms, host, i + 1)
        if rep.verdict != INCONCLUSIVE:
            break
    torch.cuda.synchronize()
    return rep


# ---------------------------------------------------------------------- two calls at once
def overlap(name: str, a: Callable[[], object], b: Callable[[], object], streams: Sequence["torch.cuda.Stream"], blocker: Blocker,
            hold_ms: float = 50.0) -> List[str]:
    """`a()` and `b()` (closures over finished inputs) serially on the default stream, then `a` on streams[0] and `b` on streams[1]
    at once: both streams wait for ONE event behind a blocker on stream 0, so `a` is enqueued in full and `b` begins while neither
    has started (put a host that synchronises second).
    -> the differences of each concurrent result to its serial one (empty: "no state between calls" holds under concurrency)."""
    null = torch.cuda.default_stream()
    refs = []
    for fn in (a, b):
        refs.append(_snapshot(fn()))
        torch.cuda.synchronize()
    for fn, s in zip((a, b), streams):                             # allocator warm-up on each stream
        with torch.cuda.stream(s):
            fn()
    torch.cuda.synchronize()
    go = torch.cuda.Event()
    with torch.cuda.stream(null):
        blocker.sleep(hold_ms)
        go.record()
    got, started_together = [], True
    for fn, s in zip((a, b), streams):
        s.wait_event(go)
        started_together = not go.query()                          # (asked before the second call: `b` may be a host that synchronises)
        with torch.cuda.stream(s):
            got.append(_snapshot(fn()))
    for s in streams:
        s.synchronize()
    torch.cuda.synchronize()
    out = [] if started_together else [f"{name}: the release event had fired before the second call began ({hold_ms:.0f} ms)"]
    for tag, g, r in zip("ab", got, refs):
        out += [f"{name} [{tag}] {d}" for d in fp.differences(g, r)]
    return out
