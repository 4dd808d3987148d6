"""Timing skew for stream-schedule tests, on the launch hook of _lib.call.

Every launch of the package goes through `_lib._HOOK[0](name, args) -> closer | None` on the launch's own stream.  `skew(slow=...)`
installs a hook that puts a spin (`torch.cuda._sleep`) in front of every launch issued on one of the `slow` streams: everything on
those streams then finishes late, while the other streams run at their natural pace.  A consumer on another stream that lacks its
event wait reaches its launch while the producer still sits behind the spin; a tensor handed to a slow stream without being kept
alive is freed, and its block reused, long before the slow reader runs.  Neither shows at natural timing.

The hook counts launches and delayed launches per stream (the guard against a comparison that delayed nothing), can time every
launch between two events of its stream (`timed=True`: how the tests size the delay), chains to a hook that was already installed
and puts it back on exit, also when the body raises.

Streams are told apart by their handle (`stream.cuda_stream`), so the objects `torch.cuda.current_stream()` makes anew at every
call compare as the stream they name; a stand-in without that attribute stands for itself.  The module imports torch only where it
touches the GPU: the logic is tested without one (tests/test_stream_skew_cpu.py) through the `hook_cell`, `current_stream`, `sleep`
and `event` arguments."""
from contextlib import contextmanager

_CYCLES_PER_US = [None]


def stream_key(stream):
    return getattr(stream, "cuda_stream", stream)


def calibrate(sleep=None, event=None, synchronize=None, cycles=(2_000_000, 10_000_000)):
    """Spin cycles of `torch.cuda._sleep` per microsecond on this device, measured once per process: two spins of different length,
    each between two events on the current stream, and the slope between them (what a launch costs besides its spin cancels)."""
    if sleep is None and _CYCLES_PER_US[0] is not None:
        return _CYCLES_PER_US[0]
    own = sleep is None
    if own:
        import torch
        sleep, synchronize = torch.cuda._sleep, torch.cuda.synchronize
        event = lambda: torch.cuda.Event(enable_timing=True)
        sleep(cycles[0])                                       # (the first launch of the spin kernel loads it)
    times = []
    for n in cycles:
        synchronize()
        a, b = event(), event()
        a.record(); sleep(n); b.record()
        synchronize()
        times.append(a.elapsed_time(b) * 1000.0)               # ms -> us
    if not times[1] > times[0] > 0.0:
        raise RuntimeError(f"spin calibration: {cycles[0]} cycles took {times[0]} us, {cycles[1]} cycles {times[1]} us")
    rate = (cycles[1] - cycles[0]) / (times[1] - times[0])
    if own:
        _CYCLES_PER_US[0] = rate
    return rate


class Skew:
    """What `skew()` yields: the counters and, with timed=True, the launches' durations."""

    def __init__(self, slow, cycles, timed, current_stream, sleep, event):
        self.slow = {stream_key(s) for s in slow}
        self.cycles = int(cycles)
        self.launches, self.delayed = {}, {}                   # stream key -> count
        self._timed, self._spans = timed, []                   # (name, stream key, start event, end event)
        self._current, self._sleep, self._event = current_stream, sleep, event
        self._prev = None

    def _hook(self, name, args):
        key = stream_key(self._current())
        self.launches[key] = self.launches.get(key, 0) + 1
        if key in self.slow and self.cycles > 0:
            self._sleep(self.cycles)                           # on the current stream: the launch's own
            self.delayed[key] = self.delayed.get(key, 0) + 1
        inner = self._prev(name, args) if self._prev is not None else None
        if not self._timed:
            return inner
        a, b = self._event(), self._event()
        a.record()                                             # behind the spin: the span is the launch alone
        self._spans.append((name, key, a, b))

        def close():
            b.record()
            if inner is not None:
                inner()
        return close

    def launches_on(self, stream):
        return self.launches.get(stream_key(stream), 0)

    def delayed_on(self, stream):
        return self.delayed.get(stream_key(stream), 0)

    def durations_us(self, start=0):
        """[(name, microseconds)] of the timed launches from the start-th on; the caller has synchronised the device."""
        return [(name, a.elapsed_time(b) * 1000.0) for name, _, a, b in self._spans[start:]]

    @property
    def timed_launches(self):
        return len(self._spans)


@contextmanager
def skew(slow=(), delay_us=0.0, cycles_per_us=None, timed=False, hook_cell=None, current_stream=None, sleep=None, event=None):
    """slow: a stream or a collection of streams whose launches are delayed by delay_us each.  cycles_per_us: calibrate() by default.
    hook_cell: the one-element list that holds the hook (_lib._HOOK by default)."""
    if hasattr(slow, "cuda_stream") or not hasattr(slow, "__iter__"):
        slow = (slow,)
    slow = tuple(slow)
    if hook_cell is None or current_stream is None or sleep is None or (timed and event is None):
        import torch
        from _pkg import sub
        hook_cell = sub("_lib")._HOOK if hook_cell is None else hook_cell
        current_stream = current_stream or torch.cuda.current_stream
        sleep = sleep or torch.cuda._sleep
        event = event or (lambda: torch.cuda.Event(enable_timing=True))
    if delay_us < 0:
        raise ValueError("delay_us must not be negative")
    cycles = 0
    if slow and delay_us > 0:
        cycles = max(1, round(delay_us * (calibrate() if cycles_per_us is None else cycles_per_us)))
    s = Skew(slow, cycles, timed, current_stream, sleep, event)
    s._prev = hook_cell[0]
    hook_cell[0] = s._hook
    try:
        yield s
    finally:
        hook_cell[0] = s._prev
