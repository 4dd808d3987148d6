"""The timing-skew harness of tests/_streamskew.py without a GPU: stand-in streams, a stand-in spin and a stand-in hook cell."""
import pytest

from _streamskew import calibrate, skew, stream_key


class _Stream:
    """A stand-in for torch.cuda.Stream: a new object per current_stream() call names the same stream through its handle."""

    def __init__(self, handle):
        self.cuda_stream = handle


class _World:
    def __init__(self):
        self.cell = [None]
        self.current = 1
        self.sleeps = []                                       # (stream handle, cycles), in order
        self.log = []

    def current_stream(self):
        return _Stream(self.current)

    def sleep(self, cycles):
        self.sleeps.append((self.current, cycles))

    def launch(self, name, on):
        """What _lib.call does around a launch."""
        self.current = on
        hook = self.cell[0]
        done = hook(name, ()) if hook is not None else None
        self.log.append(("launch", name, on))
        if done is not None:
            done()

    def skew(self, **kw):
        return skew(hook_cell=self.cell, current_stream=self.current_stream, sleep=self.sleep, **kw)


def test_launches_are_counted_per_stream_and_only_slow_streams_are_delayed():
    w = _World()
    with w.skew(slow=_Stream(2), delay_us=100.0, cycles_per_us=1500.0) as s:
        for name, on in (("a", 1), ("b", 2), ("c", 2), ("d", 3), ("e", 1), ("f", 2)):
            w.launch(name, on)
    assert s.launches == {1: 2, 2: 3, 3: 1} and s.delayed == {2: 3}
    assert (s.launches_on(_Stream(1)), s.launches_on(_Stream(2)), s.launches_on(_Stream(4))) == (2, 3, 0)
    assert (s.delayed_on(_Stream(1)), s.delayed_on(_Stream(2))) == (0, 3)
    assert w.sleeps == [(2, 150000)] * 3                       # on the launch's own stream, delay_us * cycles_per_us each
    assert [e[1] for e in w.log] == list("abcdef")


def test_a_set_of_slow_streams_and_no_slow_stream():
    w = _World()
    with w.skew(slow={_Stream(1), _Stream(3)}, delay_us=2.0, cycles_per_us=10.0) as s:
        for on in (1, 2, 3, 3):
            w.launch("k", on)
    assert s.delayed == {1: 1, 3: 2} and w.sleeps == [(1, 20), (3, 20), (3, 20)]
    w = _World()
    with w.skew() as s:                                        # counting only
        w.launch("k", 1)
    assert s.launches == {1: 1} and s.delayed == {} and w.sleeps == []
    with pytest.raises(ValueError):
        with w.skew(slow=_Stream(1), delay_us=-1.0, cycles_per_us=1.0):
            pass
    assert w.cell[0] is None


def test_a_stand_in_without_a_handle_stands_for_itself():
    assert stream_key("main") == "main" and stream_key(_Stream(7)) == 7


def test_the_spin_goes_out_before_an_installed_hook_is_called_and_its_closer_still_runs():
    w = _World()
    seen = []

    def installed(name, args):
        seen.append(("open", name, len(w.sleeps)))
        return lambda: seen.append(("close", name))

    w.cell[0] = installed
    with w.skew(slow=_Stream(1), delay_us=1.0, cycles_per_us=1.0) as s:
        assert w.cell[0] is not installed
        w.launch("x", 1)
        w.launch("y", 2)
    assert w.cell[0] is installed                              # put back
    assert seen == [("open", "x", 1), ("close", "x"), ("open", "y", 1), ("close", "y")]
    assert s.launches == {1: 1, 2: 1}
    w.launch("z", 1)                                           # ... and no longer delayed or counted
    assert len(w.sleeps) == 1 and s.launches == {1: 1, 2: 1} and seen[-1] == ("close", "z")


def test_an_installed_hook_without_a_closer_and_nested_skews():
    w = _World()
    names = []
    w.cell[0] = lambda name, args: names.append(name)
    with w.skew(slow=_Stream(1), delay_us=1.0, cycles_per_us=4.0) as outer:
        with w.skew(slow=_Stream(2), delay_us=1.0, cycles_per_us=8.0) as inner:
            w.launch("p", 1)
            w.launch("q", 2)
        w.launch("r", 2)
    assert names == ["p", "q", "r"]
    assert inner.launches == {1: 1, 2: 1} and outer.launches == {1: 1, 2: 2}
    assert w.sleeps == [(1, 4), (2, 8)]


def test_the_previous_hook_is_restored_when_the_body_raises():
    w = _World()
    installed = lambda name, args: None
    w.cell[0] = installed
    with pytest.raises(KeyError):
        with w.skew(slow=_Stream(1), delay_us=1.0, cycles_per_us=1.0):
            w.launch("x", 1)
            raise KeyError("boom")
    assert w.cell[0] is installed
    w.cell[0] = None

    def failing_spin(cycles):
        raise RuntimeError("spin failed")
    with pytest.raises(RuntimeError):                          # the hook itself raises inside a launch
        with skew(slow=_Stream(1), delay_us=1.0, cycles_per_us=1.0, hook_cell=w.cell, current_stream=w.current_stream, sleep=failing_spin):
            w.launch("x", 1)
    assert w.cell[0] is None


class _Event:
    clock = [0.0]                                              # ms

    def record(self):
        self.t = _Event.clock[0]

    def elapsed_time(self, other):
        return other.t - self.t


def test_timed_launches_are_bracketed_behind_the_spin():
    w = _World()
    _Event.clock[0] = 0.0

    def sleep(cycles):
        _Event.clock[0] += 5.0                                 # the spin takes 5 ms: it must stay outside the span
    with skew(slow=_Stream(1), delay_us=1.0, cycles_per_us=1.0, timed=True, hook_cell=w.cell, current_stream=w.current_stream,
              sleep=sleep, event=_Event) as s:
        for name, ms in (("a", 0.25), ("b", 0.5)):
            w.current = 1
            done = w.cell[0](name, ())
            _Event.clock[0] += ms                              # the launch itself
            done()
    assert s.timed_launches == 2
    assert s.durations_us() == [("a", 250.0), ("b", 500.0)] and s.durations_us(start=1) == [("b", 500.0)]


def test_calibration_takes_the_slope_between_two_spins():
    _Event.clock[0] = 0.0
    overhead_ms, rate = 0.02, 1500.0                           # cycles per microsecond

    def sleep(cycles):
        _Event.clock[0] += overhead_ms + cycles / rate / 1000.0
    got = calibrate(sleep=sleep, event=_Event, synchronize=lambda: None, cycles=(1_000_000, 4_000_000))
    assert got == pytest.approx(rate, rel=1e-9)                # the per-launch overhead cancels
    with pytest.raises(RuntimeError):
        calibrate(sleep=lambda c: None, event=_Event, synchronize=lambda: None)
