"""Helpers of tests/test_gpu_streams.py: the poison-and-delay run of one entry point on a side
stream, the calibrated delay kernel, and bit-exact comparison of device tensors.

The idea (include/pfb_api.h, "Streams"): torch's streams are non-blocking, so nothing orders
the default stream, or any third stream, against the side stream ``s`` a call is given.  With a
long delay kernel at the head of ``s``, every operation the call enqueues on ``s`` waits; one it
enqueues anywhere else runs at once, while the input still holds poison (NaN, 0xFF bytes), the
output a sentinel and the plan's carry the samples of an earlier run.  The result then differs
from the same call made on the idle default stream, which it must equal bit for bit.
"""
import time

SENTINEL = complex(7.0, -7.0)
MIN_DELAY_MS = 10.0    # the delay is at least this ...
DELAY_FACTOR = 10.0    # ... and this many times the reference call (host enqueue + device time)

_CAL = {}


def bits(t):
    """The bytes of ``t`` as a flat uint8 tensor (NaNs compare by their bits)."""
    import torch
    t = t.contiguous()
    if t.is_complex():
        t = torch.view_as_real(t)
    return t.reshape(-1).view(torch.uint8)


def same_bits(a, b):
    import torch
    return tuple(a.shape) == tuple(b.shape) and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def poison_(t):
    """NaN in every float component, 0xFF in every byte of an integer tensor."""
    import torch
    if t.is_complex() or t.is_floating_point():
        t.fill_(complex(float("nan"), float("nan")) if t.is_complex() else float("nan"))
    else:
        t.view(torch.uint8).fill_(255)
    return t


def sentinel_like(t):
    import torch
    if t.is_complex():
        return torch.full_like(t, SENTINEL)
    return torch.full_like(t, 85)


def scrambled(x):
    """``x``'s samples in reverse order: other data of the same shape, for a warm-up run."""
    return x.contiguous().reshape(-1).flip(0).reshape(x.shape).contiguous()


def _sleep_ms(torch, cycles):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    torch.cuda._sleep(int(cycles))
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def cycles_per_ms():
    """``torch.cuda._sleep`` cycles per millisecond, measured with events once per process: the
    slope between two delays (the launch overhead cancels), the longer at least 8 ms."""
    if "cpm" not in _CAL:
        import torch
        _sleep_ms(torch, 1000)  # loads the kernel
        c = 1 << 16
        while min(_sleep_ms(torch, c) for _ in range(2)) < 8.0:
            c *= 2
            assert c < (1 << 40), "torch.cuda._sleep does not delay"
        hi = min(_sleep_ms(torch, c) for _ in range(3))
        lo = min(_sleep_ms(torch, c // 4) for _ in range(3))
        _CAL["cpm"] = (c - c // 4) / (hi - lo)
    return _CAL["cpm"]


def delay_for(ref_ms):
    """(cycles, ms, text) of the delay in front of a call whose reference took ``ref_ms``."""
    cpm = cycles_per_ms()
    ms = max(MIN_DELAY_MS, DELAY_FACTOR * ref_ms)
    text = (f"delay {ms:.1f} ms = max({MIN_DELAY_MS:.0f}, {DELAY_FACTOR:.0f} x {ref_ms:.3f} ms reference), "
            f"{cpm:.0f} sleep cycles per ms")
    return int(ms * cpm), ms, text


class Delayed:
    """``with Delayed(ref_ms) as d:`` — a fresh side stream (or ``stream``, idle) with the delay
    kernel at its head, current inside the block.  ``d.assert_pending()`` is step 3: the delay
    has not finished, so nothing enqueued behind it on the stream has run."""

    def __init__(self, ref_ms, what="", stream=None):
        import torch
        self.torch = torch
        self.what = what
        self.cycles, self.ms, self.text = delay_for(ref_ms)
        self.stream = torch.cuda.Stream() if stream is None else stream
        self.event = torch.cuda.Event()
        self._ctx = None

    def __enter__(self):
        torch = self.torch
        self._ctx = torch.cuda.stream(self.stream)
        self._ctx.__enter__()
        torch.cuda._sleep(self.cycles)
        self.event.record(self.stream)
        return self

    def __exit__(self, *exc):
        return self._ctx.__exit__(*exc)

    def assert_pending(self):
        assert not self.event.query(), (
            f"{self.what}: the delay kernel had finished when the call returned to the host, so a "
            f"launch on another stream would not have run early; {self.text}")


class Gate:
    """Holds ``streams`` behind one delay kernel, which runs on a stream of the gate's own, until
    the host has enqueued everything it means to: the streams' work is then released at the same
    moment and overlaps on the device however slowly the host enqueued it.
    ``assert_pending()``, once everything is enqueued, is the proof that nothing ran before."""

    def __init__(self, ref_ms, streams, what=""):
        import torch
        self.what = what
        cycles, self.ms, self.text = delay_for(ref_ms)
        self.stream = torch.cuda.Stream()
        self.event = torch.cuda.Event()
        with torch.cuda.stream(self.stream):
            torch.cuda._sleep(cycles)
            self.event.record(self.stream)
        for s in streams:
            s.wait_event(self.event)

    def assert_pending(self):
        assert not self.event.query(), (
            f"{self.what}: the gate's delay had finished before every call was enqueued, so the "
            f"streams' work need not have overlapped; {self.text}")


def timed(fn):
    """(result, ms): ``fn()`` on the idle device, host enqueue and device time together."""
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = fn()
    torch.cuda.synchronize()
    return res, (time.perf_counter() - t0) * 1e3


def poison_delay(what, make, run, xs, takes_out=False, reset=None, buffered=None, check=None):
    """Steps 1-4 for one entry point.

    make() -> a fresh plan or stream object; run(obj, xs, outs) -> the list of tensors the
    call(s) wrote, given the list of input tensors ``xs`` (one per chunk) and, when
    ``takes_out``, the buffers to write into (else None); reset(obj): forget the carry;
    buffered(obj) -> the object's buffered count; check(obj): asserts about the object after
    its run (which host branch it took), made of the reference and of the side-stream object.
    Returns (reference outputs, the reference object): the default-stream results on the idle
    device, for an oracle check."""
    import torch
    # the object under test has run before, on other samples: its buffers exist (no allocation
    # or free, which waits for the device, in the run below) and hold a stale carry
    obj = make()
    warm = run(obj, [scrambled(x) for x in xs], None)
    torch.cuda.synchronize()
    if reset is not None:
        reset(obj)
    ref_obj = make()
    ref, ref_ms = timed(lambda: run(ref_obj, xs, None))
    ref = [r.clone() for r in ref]
    assert [tuple(r.shape) for r in ref] == [tuple(w.shape) for w in warm]
    assert sum(r.numel() for r in ref) > 0, f"{what}: the reference wrote nothing"
    del warm
    # 1. poisoned input, sentinel output
    inp = [poison_(torch.empty_like(x)) for x in xs]
    outs = [sentinel_like(r) for r in ref] if takes_out else None
    torch.cuda.synchronize()
    # 2. delay, fill, call, copy out — all on the side stream
    with Delayed(ref_ms, what) as d:
        for i, x in zip(inp, xs):
            i.copy_(x)
        got = run(obj, inp, outs)
        got = [g.clone() for g in got]
        # 3. (the clones are enqueued too: the host has done everything by now)
        d.assert_pending()
    # 4.
    d.stream.synchronize()
    torch.cuda.synchronize()
    assert len(got) == len(ref)
    for k, (g, r) in enumerate(zip(got, ref)):
        assert same_bits(g, r), (
            f"{what}: output {k} on the side stream differs from the default-stream call "
            f"(NaN: {bool(torch.isnan(torch.view_as_real(g) if g.is_complex() else g.float()).any())}); {d.text}")
    for k, (i, x) in enumerate(zip(inp, xs)):
        assert same_bits(i, x), f"{what}: input {k} changed"
    if buffered is not None:
        assert buffered(obj) == buffered(ref_obj), f"{what}: buffered count"
    if check is not None:
        check(ref_obj)
        check(obj)
    return ref, ref_obj
