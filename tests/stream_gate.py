"""A gate for tests/test_stream_contract_gpu.py (a helper module, not a conftest): does a call run on the stream it was
given, and does it return before that stream has drained?

The gate is a delay kernel (torch.cuda._sleep; a chain of device-to-device copies where that does not delay) on a producer
stream S1, with the event `done` recorded behind it.  While it runs, nothing that is ordered behind S1 can have happened:

  Recording  placement.Plain that also keeps, in call order, a pristine device copy of what every to() uploaded and the
             arguments of every full().
  Gated      the same interface, built from the Recording of an earlier identical run.  The k-th to() returns a fresh
             buffer that holds poison at once (filled on a stream of its own that never waits for the gate); behind the
             gate, on S1, the recorded payload is copied into it, and the current stream waits for an event of S1.
             full() is filled the same way.  No host memory is touched, so nothing in the allocator waits for the device.
  watching   patches conceptattention_amd._lib.check for one run: ops and the tests pass every return code through it
             straight after the C call returns, so done.query() at that moment says whether the call came back while
             the gate was still running.

A launch that goes to another stream than the current one reads poison, or has its output overwritten by the late fill;
a call that waits for its stream sees done.query() == True.  Every assertion built on this fails when the gate is too
short, so its length is a convenience and no tolerance.

Gate length: 50 ms (GATE_MS); torch.cuda._sleep delays on an MI355X (2.4 million of its cycles per millisecond), the
copy chain is the fall-back.  That is about 4 s of gates for the 85 probes; the whole GPU file ran in 10 s there.  Host
enqueue time of a probed helper on its eager warm-up run, from its first allocator call to the return of its last entry
point (uploads from pageable memory included), measured there: 145 ms for the first call of the process (the library
and its code objects are loaded), 22 ms for the first launch of one GEMM kernel, at most 2.6 ms for every other probe and
0.1 to 0.3 ms for most.  The probe run comes after that warm-up, so it pays the last figure
(tests/test_stream_contract_gpu.py prints the figure of every probe with pytest -s)."""
from __future__ import annotations

import contextlib
import time

import torch

import placement

GATE_MS = 50.0
POISON_BYTE = 0xA5
NAN = float("nan")


def poison_kind(dtype, is_input: bool) -> str:
    """What a Gated buffer holds until the gate opens: "nan" for floating types, "index" for the int32 / int64 inputs
    (ids, row_idx: a valid index but a wrong one -- the payload rotated by one element -- so that a kernel that reads it
    too early stays inside its tables), "bytes" (0xA5) for every other integer type and for integer outputs."""
    if dtype.is_floating_point:
        return "nan"
    if is_input and dtype in (torch.int32, torch.int64):
        return "index"
    return "bytes"


class Recording(placement.Plain):
    """Ordinary allocations; `calls` keeps ("to", pristine device copy) / ("full", shape, fill, dtype) in call order."""

    def __init__(self, dev="cuda"):
        super().__init__(dev)
        self.calls = []
        self.t_first = None       # host time of the first allocator call

    def to(self, t, roles=None):
        self.t_first = self.t_first or time.perf_counter()
        d = super().to(t, roles)
        self.calls.append(("to", d.clone()))
        return d

    def full(self, shape, fill, dtype, roles=None):
        self.t_first = self.t_first or time.perf_counter()
        self.calls.append(("full", tuple(shape), fill, dtype))
        return super().full(shape, fill, dtype, roles)


class Gate:
    """The delay on S1 and the event behind it.  `poison` is the stream the poison fills run on."""

    _rate = None          # (kind, units per millisecond), calibrated once per process

    def __init__(self, ms: float = GATE_MS):
        self.ms = ms
        self.s1, self.poison = torch.cuda.Stream(), torch.cuda.Stream()
        self.done = torch.cuda.Event()
        self.started = False

    @classmethod
    def _delay(cls, kind, units):
        if kind == "sleep":
            torch.cuda._sleep(int(units))
        else:
            a, b = cls._copy_bufs
            for _ in range(int(units)):
                b.copy_(a)

    @classmethod
    def calibrate(cls):
        if cls._rate is not None:
            return cls._rate
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            for kind, units in (("sleep", 4_000_000), ("copies", 16)):
                if kind == "copies":
                    cls._copy_bufs = (torch.zeros(1 << 28, dtype=torch.uint8, device="cuda"),
                                      torch.empty(1 << 28, dtype=torch.uint8, device="cuda"))
                cls._delay(kind, units // 8)                      # loads the kernel
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                cls._delay(kind, units)
                e1.record()
                e1.synchronize()
                ms = e0.elapsed_time(e1)
                if ms > 0.2:                                      # the delay delays: use it
                    cls._rate = (kind, units / ms)
                    return cls._rate
        raise AssertionError("neither torch.cuda._sleep nor a chain of copies delays a stream on this device")

    def start(self):
        kind, rate = self.calibrate()
        assert not self.started
        self.started = True
        with torch.cuda.stream(self.s1):
            self._delay(kind, rate * self.ms)
            self.done.record()

    def running(self) -> bool:
        return not self.done.query()


class Gated:
    """placement.Plain's interface behind a Gate, from the Recording of an earlier identical run."""
    straddle = None

    def __init__(self, recording: Recording, gate: Gate = None, dev="cuda"):
        self.expected = list(recording.calls)
        self.gate, self.dev = gate, dev
        self.k = 0
        self.keep = []            # every buffer stays alive until release(): they are used on three streams

    def _next(self, kind, shape, dtype):
        assert self.k < len(self.expected), f"call {self.k}: the recorded run made only {len(self.expected)} calls"
        rec = self.expected[self.k]
        want_shape, want_dtype = (tuple(rec[1].shape), rec[1].dtype) if rec[0] == "to" else (rec[1], rec[3])
        assert (rec[0], want_shape, want_dtype) == (kind, tuple(shape), dtype), \
            f"call {self.k}: {kind} {tuple(shape)} {dtype}, the recorded run made {rec[0]} {want_shape} {want_dtype}"
        self.k += 1
        return rec

    def _behind_the_gate(self, shape, dtype, kind, late):
        g = self.gate
        if not g.started:
            g.start()
        with torch.cuda.stream(g.poison):          # allocated and poisoned on a stream the gate never holds up
            buf = torch.empty(shape, dtype=dtype, device=self.dev)
            if kind == "nan":
                buf.fill_(NAN)
            elif kind == "index":
                buf.copy_(torch.roll(late.reshape(-1), 1).reshape(shape))
            else:
                buf.view(torch.uint8).fill_(POISON_BYTE)
        g.s1.wait_stream(g.poison)
        with torch.cuda.stream(g.s1):              # behind the gate
            if isinstance(late, torch.Tensor):
                buf.copy_(late)
            else:
                buf.fill_(late)
            ev = torch.cuda.Event()
            ev.record()
        torch.cuda.current_stream().wait_event(ev)
        self.keep.append(buf)
        return buf

    def to(self, t, roles=None):
        rec = self._next("to", t.shape, t.dtype)
        return self._behind_the_gate(tuple(t.shape), t.dtype, poison_kind(t.dtype, True), rec[1])

    def full(self, shape, fill, dtype, roles=None):
        rec = self._next("full", shape, dtype)
        assert rec[2] == fill or (rec[2] != rec[2] and fill != fill), f"call {self.k - 1}: fill {fill}, recorded {rec[2]}"
        return self._behind_the_gate(tuple(shape), dtype, poison_kind(dtype, False), fill)

    def check_guards(self):
        pass

    def release(self):
        assert self.k == len(self.expected), f"{self.k} allocator calls, the recorded run made {len(self.expected)}"
        torch.cuda.synchronize()
        self.keep.clear()


@contextlib.contextmanager
def watching(gate: Gate = None):
    """Patch conceptattention_amd._lib.check for one run: yields the list of (name, gate still running, host time) per call
    (gate None: the name and the time only, for the warm-up run's enqueue time)."""
    from conceptattention_amd import _lib as L
    real, calls = L.check, []

    def check(rc, what=""):
        calls.append((what, gate is None or gate.running(), time.perf_counter()))
        return real(rc, what)
    L.check = check
    try:
        yield calls
    finally:
        L.check = real
