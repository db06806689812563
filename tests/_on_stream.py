"""TEST INFRASTRUCTURE: arrays that arrive late on a stream.  What tests/_guarded.py does in space this does in time: a case
keeps a side stream busy for DELAY_MS, lets its inputs arrive on that stream behind the delay, makes the library call with
that stream and reads back on that stream.  Until the delay has drained an input holds the NaN of _guarded.PATTERN and an
output has not yet been filled with it, so any part of the library's work that is not ordered on the stream it was given (a
launch without its stream argument, a memset on the null stream, an FFT plan whose stream was never set) reads NaN or is
overwritten by the fill, and the comparison with the oracle fails.  tests/test_gpu_streams.py uses it and proves first,
on a stand-in that breaks the rule, that it can fail.  Nothing here touches a GPU on import.

DELAY_MS.  The delay must outlast the host-side enqueue of the warmed call under test.  Measured on the MI355X over the
asynchronous cases of tests/test_gpu_streams.py (from the enqueue of the delay, through the arrival of the late arrays, to the
return of the call; the figure of every case is in docs/measurement_log.md):

    largest host time     MEASURED_MAX_ENQUEUE_MS  (below)
    DELAY_MS              ten times that, rounded up to a whole millisecond

Make the arrays of a call before its delay is enqueued, and after a warm pass of the same case: an allocation that reaches
hipMalloc waits for the device, and with it for the delay (measured: 20 ms where 0.1 ms was expected).

It is no tolerance: every asynchronous case asserts `still_busy` after its call returns, so a delay that was too short for
the machine it runs on fails the case instead of passing it for the wrong reason."""
import time

import numpy as np

from _guarded import PATTERN

MEASURED_MAX_ENQUEUE_MS = 1.634   # "spdhg tv in a placed block, 4 rounds on two streams" (1.142 in another run); one call alone:
DELAY_MS = 17                     # 0.644 (pdtv_slabs)

_UINT = {4: np.uint32, 2: np.uint16, 1: np.uint8}
_cycles_per_ms = None             # set by calibrate(), once per module (a module-scoped fixture of the test file)
ENQUEUE_LOG = []                  # (label, delayed?, host milliseconds from the delay's enqueue to the first read-back request)
_busy_tensor = None               # the fallback of _busy_work, allocated once by calibrate()


def side_stream():
    """a stream of torch's pool: non-blocking, so the null stream does not implicitly wait for it nor it for the null stream"""
    import torch
    return torch.cuda.Stream()


_staging = None


def staging_stream():
    """the one stream every late array is staged from.  One stream, because torch's caching allocator keeps a pool per stream:
    the warm pass of a case leaves the blocks the delayed pass then takes, and no allocation reaches hipMalloc -- which waits
    for the device, the delay included -- while a delay is pending."""
    global _staging
    if _staging is None:
        _staging = side_stream()
    return _staging


def _busy_work(stream, amount):
    """keeps `stream` busy in proportion to `amount`: torch.cuda._sleep where it exists, else a chain of in-place
    element-wise operations on a large tensor"""
    import torch
    with torch.cuda.stream(stream):
        if hasattr(torch.cuda, "_sleep"):
            torch.cuda._sleep(int(amount))
        else:
            for _ in range(max(1, int(amount) // 1000000)):
                _busy_tensor.add_(1.0)


def calibrate():
    """the amount of _busy_work that one millisecond takes, measured once with HIP events on a stream of its own"""
    global _cycles_per_ms, _busy_tensor
    import torch
    if _busy_tensor is None and not hasattr(torch.cuda, "_sleep"):
        _busy_tensor = torch.zeros(1 << 26, device="cuda")      # here, not in delay(): an allocation waits for the device
        torch.cuda.synchronize()
    s = side_stream()
    amount = 20000000
    _busy_work(s, amount)           # warm
    s.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record(s)
    _busy_work(s, amount)
    t1.record(s)
    s.synchronize()
    ms = t0.elapsed_time(t1)
    assert ms > 0.05, ms
    _cycles_per_ms = amount / ms
    return _cycles_per_ms


def delay(stream, ms=None):
    """keeps `stream` busy for DELAY_MS (or `ms`)"""
    assert _cycles_per_ms is not None, "calibrate() first: a module-scoped fixture of the test file does"
    _busy_work(stream, _cycles_per_ms * (DELAY_MS if ms is None else ms))


def _torch_dtype(dt):
    import torch
    return getattr(torch, np.dtype(dt).name)


def _raw_on_device(image, staging):
    """the bytes of a host array on the device, complete before this returns; the host waits for `staging` alone"""
    import torch
    with torch.cuda.stream(staging):
        raw = torch.from_numpy(np.ascontiguousarray(image).reshape(-1).view(np.uint8).copy()).cuda()
    staging.synchronize()
    return raw


class Staged:
    """the two halves of `late` / `late_out`: everything that makes the host wait (allocation, the copies from pageable
    memory) happens at construction, on `staging`; `arrive(stream)` only enqueues on `stream` and never waits.  The tensor
    holds the pattern until its contents arrive: the given array, or for an output the fill value.  Every copy moves bytes,
    so the integer tables need no arithmetic of torch's."""

    def __init__(self, given, shape, dtype, fill, staging):
        import torch
        self.staging = staging or staging_stream()
        dt = np.dtype(dtype)
        shape = tuple(int(s) for s in shape)
        n = int(np.prod(shape, dtype=np.int64))
        if given is None:
            given = np.full(n, (np.nan if dt.kind == "f" else 0) if fill is None else fill, dt)
        self._pat = _raw_on_device(np.full(n, PATTERN[dt.itemsize], _UINT[dt.itemsize]), self.staging)
        self._raw = _raw_on_device(np.full(n, PATTERN[dt.itemsize], _UINT[dt.itemsize]), self.staging)
        self._src = _raw_on_device(np.asarray(given, dt), self.staging)
        self._event = torch.cuda.Event()
        self._event.record(self.staging)
        self.t = self._raw.view(_torch_dtype(dt)).view(shape)

    def poison(self, stream):
        """the pattern again, in stream order: a read-only input becomes late once more for the next call"""
        import torch
        with torch.cuda.stream(stream):
            self._raw.copy_(self._pat, non_blocking=True)

    def arrive(self, stream):
        import torch
        stream.wait_event(self._event)
        with torch.cuda.stream(stream):
            self._raw.copy_(self._src, non_blocking=True)
        return self.t


def late(host_array, stream, staging=None):
    """a device tensor that holds the pattern (NaN for float32) now and `host_array` once `stream` has reached the copy
    enqueued here -- behind whatever `stream` is busy with, a `delay` in particular.  The true data are staged on the device
    from `staging`, so the host never blocks on `stream`.  Returns (the tensor, what must stay alive until the read-back)."""
    a = np.ascontiguousarray(host_array)
    st = Staged(a, a.shape, a.dtype, None, staging)
    return st.arrive(stream), st


def late_out(shape, stream, dtype=np.float32, fill=None, staging=None):
    """an output tensor that is filled on `stream` -- NaN for float32, 0 for the integer types unless `fill` says otherwise,
    like _guarded.guarded --, behind whatever `stream` is busy with: a store that is not ordered on `stream` lands before the
    fill and is overwritten by it.  Until then the tensor holds the pattern.  Returns (the tensor, what must stay alive)."""
    st = Staged(None, tuple(int(s) for s in shape), dtype, fill, staging)
    return st.arrive(stream), st


def still_busy(stream):
    return not stream.query()


def read(t, stream):
    """synchronises `stream` only and copies to the host"""
    import torch
    dt = np.dtype(str(t.dtype).split(".")[1])
    with torch.cuda.stream(stream):
        h = t.detach().reshape(-1).view(torch.uint8).cpu()   # a copy to pageable memory waits for the current stream alone
    stream.synchronize()
    return h.numpy().view(dt).reshape(tuple(t.shape)).copy()


class _Late:
    """one array of a Late provider: `.view` and `.host()` as tests/_guarded.Guarded has them"""

    def __init__(self, owner, given, shape, dtype, fill):
        self._owner, self._given, self.dtype = owner, given, np.dtype(dtype)
        self._staged = Staged(given, shape, dtype, fill, owner.staging)      # kept alive with the provider
        self._t = None

    def _deliver(self):
        self._t = self._staged.arrive(self._owner.stream)

    @property
    def view(self):
        self._owner.arm()
        if self._t is None:           # behind the delay of the call that takes it first, not of an earlier one
            self._deliver()
        return self._t

    def host(self):
        if self._t is None:
            self.view
        return self._owner.read(self._t)

    def check(self, what="", read_only=False):
        if read_only:
            got = self.host()
            isz = self.dtype.itemsize
            assert np.array_equal(got.view(_UINT[isz]), self._given.view(_UINT[isz])), (what, "a read-only input was written")


class Late:
    """the arrays of one case on `stream`, with the interface of the `Arrays` of tests/test_gpu_guards.py (ro / rw / out /
    check), so that one case body runs guard-banded there and late here.  The first `.view` taken after a read-back -- the
    arguments of the next library call -- enqueues a delay on the stream.  An array arrives behind the delay of the call that
    first takes its `.view`, however early it was made; a read-only input that an earlier call of the body used is given the
    pattern again in front of every later delay and arrives behind it once more (tensors a body kept stay valid).  So every
    call of a body finds its inputs late and its fresh outputs unfilled, not the first call alone.  The first `.host()` after the call asserts, for a case whose entry
    points are documented as asynchronous, that the stream is still busy: the call did not synchronise it and the delay
    outlasted the enqueue.  With `delayed=False` nothing is delayed and nothing asserted: the warm-up pass."""

    def __init__(self, stream, delayed=True, asynchronous=True, label=""):
        self.stream, self.delayed, self.asynchronous, self.label = stream, delayed, asynchronous, label
        self.staging = staging_stream()
        self.arrays, self.read_only = [], []
        self.armed, self.t_armed, self.asserted = False, None, 0

    def __call__(self, shift=0):        # `Arrays(shift)` of a case body: alignment is the guard suite's subject
        return self

    def arm(self):
        if self.armed:
            return
        self.armed, self.t_armed = True, time.perf_counter()
        if self.delayed:
            import torch
            again = [a for a in self.read_only if a._t is not None]
            for a in again:
                a._staged.poison(self.stream)
            delay(self.stream)
            self.delay_done = torch.cuda.Event()
            self.delay_done.record(self.stream)
            for a in again:
                a._deliver()

    def _make(self, a_or_shape, dtype=np.float32, fill=None, **_):
        if isinstance(a_or_shape, np.ndarray):
            if dtype is np.float32 and a_or_shape.dtype.kind in "iu":
                dtype = a_or_shape.dtype
            given = np.ascontiguousarray(a_or_shape, dtype=dtype)
            arr = _Late(self, given, given.shape, dtype, None)
        else:
            shape = (int(a_or_shape),) if np.isscalar(a_or_shape) else tuple(int(s) for s in a_or_shape)
            arr = _Late(self, None, shape, dtype, fill)
        self.arrays.append(arr)
        return arr

    def ro(self, a, shift=None, **kw):
        arr = self._make(a, **kw)
        self.read_only.append(arr)
        return arr

    def rw(self, a, shift=None, **kw):
        return self._make(a, **kw)

    def out(self, shape, shift=None, **kw):
        return self._make(tuple(shape), **kw)

    def returned(self):
        """right after a library call has returned: the premise of the case and the entry point's asynchrony in one look"""
        if not self.armed:
            return
        ENQUEUE_LOG.append((self.label, self.delayed, (time.perf_counter() - self.t_armed) * 1e3))
        if self.delayed and self.asynchronous:
            # (the stream alone could be busy with the entry point's own last launch: the delay itself must be pending still)
            assert still_busy(self.stream) and not self.delay_done.query(), (
                self.label, "the delay drained before the call returned: the entry point synchronised its stream, or DELAY_MS "
                "is too short for this host")
            self.asserted += 1
        self.armed = False

    done = returned          # `Arrays.done` of tests/test_gpu_guards.py: a call that reports to the host has returned

    def read(self, t):
        self.returned()
        return read(t, self.stream)

    def close(self):
        """gives the arrays back to the allocator (after the stream has been synchronised): the next provider takes them"""
        for a in self.arrays:
            a._staged = a._t = None
        self.arrays, self.read_only = [], []

    def check(self, what=""):
        for k, a in enumerate(self.arrays):
            if a._t is not None and any(a is r for r in self.read_only):
                a.check((what, "array", k), read_only=True)
