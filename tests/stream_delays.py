"""Delay injection: every cross-stream dependency is tested by making one stream late at one point of the host's program.
Shared by tests/test_stream_delays_cpu.py (the host logic, a recorder in place of the sleep, no GPU) and
tests/test_gpu_stream_delays.py (the loops, the nets, the segmenters and the loader).  A plain module: nothing here is a
fixture or a pytest setting.

The method.  ``torch.cuda._sleep`` is a spin kernel on the current stream (engine._streams_overlap probes the queue mapping
with it).  Queued on stream S at point P of the host's program, it makes everything S does behind P late by a chosen time L;
every other stream runs ahead until it meets a wait that orders it behind S.  Where the wait is in place the results are the
same bits as without the delay.  Where it is missing the consumer reads what the buffer held before, or the writer overwrites
what the late reader still needs: stale but valid memory, and other bits.  One pair (point, delayed stream) therefore tests
every edge that leaves S behind P, in both directions, at the smallest shapes.  A delay is a stimulus, never a criterion:
nothing here asserts a time, apart from the spin itself being as long as asked for.

The length.  L = max(3 x t_cycle, 2 ms) per scenario, t_cycle the host's wall time between two device synchronisations of
one unit of the undelayed leg (an accumulation cycle of a loop, one submit..result of a segmenter, one window of the loader):
the host has issued everything of this unit and of the next while the stream sleeps.  A leg injects at most once per unit.

What it cannot see.  (a) An edge whose two ends sit on one hardware queue: the sleep holds both back (``sighted`` says so
before a scenario relies on a pair).  (b) A hazard between the host and a pinned buffer: the host is never delayed.

Points.  A point is a named place of the host's program, made by wrapping a callable: ``forward:before`` / ``forward:after``
(``net.forward``; "after" is the point in front of the loss and the backward pass), ``step:early`` / ``step:late`` /
``step:plain`` (``optimizer.step`` by its ``tag``), ``prepack`` (``net.prepack_weights``), ``join`` (``net.join_gradients``),
``bucket`` (``net.wait_grad_bucket``), ``compute`` (``seg._compute``), ``submit`` (``seg.submit``), ``launch``
(``loader._launch``).  ``train_online.class_balanced_cross_entropy_loss`` is never wrapped: run_pass tests that name by identity.
"""
import time

import torch

MIN_DELAY_MS = 2.0
CYCLE_FACTOR = 3.0

# the named points, and the callable each is made of: point -> (attribute, "before" | "after")
POINTS = {
    "forward:before": ("forward", "before"), "forward:after": ("forward", "after"),
    "step:early": ("step", "before"), "step:late": ("step", "before"), "step:plain": ("step", "before"),
    "prepack": ("prepack_weights", "before"), "join": ("join_gradients", "before"), "bucket": ("wait_grad_bucket", "before"),
    "compute": ("_compute", "before"), "submit": ("submit", "before"), "launch": ("_launch", "before"),
}
# the points whose call ends a unit of a training loop (an accumulation cycle ends with its last optimizer step)
LOOP_UNIT_ENDS = ("step:late", "step:plain")


def delay_length(t_cycle_ms):
    """L of a scenario whose undelayed unit took ``t_cycle_ms`` on the host."""
    return max(CYCLE_FACTOR * float(t_cycle_ms), MIN_DELAY_MS)


def _step_point(args, kwargs):
    tag = kwargs.get("tag")
    return "step:" + (tag if tag in ("early", "late") else "plain")


class Injector:
    """Wraps callables, counts the named points they make and calls ``action()`` at ONE chosen occurrence of ONE point per unit.

    ``wrap(obj, attr, before=, after=)`` registers a callable; ``before`` / ``after`` name the point in front of and behind the
    call - a string, or a function (args, kwargs) -> string (``optimizer.step`` is three points by its tag).  Nothing is
    patched before ``__enter__`` and every attribute is what it was after ``__exit__``, whatever happened inside: an attribute
    that lived in the instance's ``__dict__`` is put back, one that came from the class is deleted from the instance.

    Units.  An ``after`` name that ends in ``/end`` is no point: it says that the call of the point in front of the slash has
    RETURNED, and where that point is one of ``unit_ends`` the current unit closes there (a cycle ends behind its last
    optimizer step; a segmenter's unit behind ``submit``; the loader's behind ``_launch``).  ``counts`` is one dict per unit,
    point -> occurrences, in order.

    The occurrence.  With ``point`` set, unit u fires at occurrence ``(u + offset) % n`` of the point, n = what
    ``occurrences[u][point]`` (the ``counts`` of an undelayed, recording leg) says the unit holds: the occurrence rotates over
    the units, and legs with offsets 0, U, 2U ... (U units a leg) cover a point with more occurrences than the leg has units
    (``offsets``).  ``fired`` lists (unit, point, occurrence) of every call of ``action``.  ``point=None`` records only."""

    def __init__(self, action=None, point=None, occurrences=None, offset=0, unit_ends=LOOP_UNIT_ENDS):
        if point is not None and point not in POINTS:
            raise ValueError("unknown point %r" % (point,))
        if point is not None and (action is None or occurrences is None):
            raise ValueError("a firing injector needs an action and the occurrences of a recording leg")
        self.action, self.point, self.occurrences, self.offset = action, point, occurrences, int(offset)
        self.unit_ends = tuple(unit_ends)
        self._specs, self._undo = [], []
        self.counts, self.fired = [{}], []
        self._fired_this_unit = False

    # ------------------------------------------------------------------------------------------ registration
    def wrap(self, obj, attr, before=None, after=None):
        if not callable(getattr(obj, attr)):
            raise TypeError("%r.%s is not callable" % (obj, attr))
        self._specs.append((obj, attr, before, after))
        return self

    def wrap_training(self, net, optimizer):
        """The points of a training loop on ``net`` and ``optimizer`` (the attributes a module does not have are left out:
        the CPU stand-in of the data-parallel tests has no ``wait_grad_bucket`` and no ``prepack_weights``)."""
        self.wrap(net, "forward", before="forward:before", after="forward:after")
        self.wrap(optimizer, "step", before=_step_point, after=lambda a, k: _step_point(a, k) + "/end")
        for attr, name in (("prepack_weights", "prepack"), ("join_gradients", "join"), ("wait_grad_bucket", "bucket")):
            if callable(getattr(net, attr, None)):
                self.wrap(net, attr, before=name)
        return self

    # ------------------------------------------------------------------------------------------ the context
    def __enter__(self):
        try:
            for obj, attr, before, after in self._specs:
                own = attr in getattr(obj, "__dict__", {})
                old = obj.__dict__[attr] if own else None
                setattr(obj, attr, self._wrapper(getattr(obj, attr), before, after))
                self._undo.append((obj, attr, own, old))
        except BaseException:
            self._restore()
            raise
        return self

    def __exit__(self, *exc):
        self._restore()
        return False

    def _restore(self):
        while self._undo:
            obj, attr, own, old = self._undo.pop()
            if own:
                setattr(obj, attr, old)
            else:
                delattr(obj, attr)

    def _wrapper(self, real, before, after):
        def name_of(spec, args, kwargs):
            return spec(args, kwargs) if callable(spec) else spec

        def call(*args, **kwargs):
            if before is not None:
                self.hit(name_of(before, args, kwargs))
            out = real(*args, **kwargs)
            if after is not None:
                self.hit(name_of(after, args, kwargs))
            return out
        return call

    # ------------------------------------------------------------------------------------------ the points
    def hit(self, name):
        if name.endswith("/end"):  # the call of a point returned: only a unit's end is read from it
            if name[:-4] in self.unit_ends:
                self.next_unit()
            return
        unit = self.counts[-1]
        k = unit.get(name, 0)
        unit[name] = k + 1
        if name == self.point and not self._fired_this_unit:
            u = len(self.counts) - 1
            n = self.occurrences[u].get(name, 0) if u < len(self.occurrences) else 0
            if n and k == (u + self.offset) % n:
                self._fired_this_unit = True
                self.fired.append((u, name, k))
                self.action()

    def next_unit(self):
        self.counts.append({})
        self._fired_this_unit = False

    @property
    def units(self):
        """The closed units' counts (the open one is left out while it is empty)."""
        return self.counts if self.counts[-1] else self.counts[:-1]


def offsets(occurrences, point):
    """The rotation offsets a point needs so that every occurrence of it inside a unit is hit in some unit of some leg:
    0, U, 2U ... below the largest number of occurrences a unit holds (U = the units of a leg).  Empty where the point never
    occurs."""
    units = [u for u in occurrences if u.get(point)]   # (the units that hold the point at all)
    most = max((u[point] for u in units), default=0)
    if not most:
        return []
    return list(range(0, most, max(len(units), 1)))


def covered(occurrences, point, fired_of_legs):
    """Whether the legs' ``fired`` lists together hit every occurrence index of ``point`` that a unit holds."""
    most = max((u.get(point, 0) for u in occurrences), default=0)
    hit = {k for fired in fired_of_legs for (_, name, k) in fired if name == point}
    return hit >= set(range(most))


# ---------------------------------------------------------------------------------------------- the scenario tables
# (role of the delayed stream, point) of every leg; tests/test_gpu_stream_delays.py runs them, tests/test_stream_delays_cpu.py
# checks that every role and every point is listed.
LOOP_STREAMS = ("caller", "aux", "pass", "comm")
LOOP_POINTS = ("forward:before", "forward:after", "step:early", "step:late", "step:plain", "prepack", "join")
ONLINE_CONFIGS = {
    # name: (frame sizes of a cycle, avg_grad_every_n, LoopOptions fields)
    "one_pass": ([(40, 70)] * 5, 5, {"microbatch_group": 5}),
    "two_pairs": ([(40, 70), (32, 56), (40, 70), (32, 56)], 4, {}),
    "two_singles": ([(40, 70), (40, 70)], 2, {"microbatch_group": 1}),
    "cycle_over_two_windows": ([(40, 70), (32, 56), (40, 70), (32, 56)], 4, {"microbatch_group": 1, "group_window": 2}),
}
OFFLINE_GROUPS = (1, 5)
OFFLINE_POINTS = ("forward:before", "forward:after", "step:plain", "join")
DP_LEGS = tuple((role, point) for role in ("comm", "aux", "caller") for point in ("forward:after", "step:early"))
NET_LEGS = {"vgg_fwd_aux": ("caller", "aux"), "resnet_aux": ("caller", "aux")}   # delayed in front of the call
SEGMENTER_FORMS = ("plain", "net_size", "jpeg_second_copy", "clean_temporal", "roi", "refine", "device_frame", "objects_png")
SEGMENTER_LEGS = (("net", "compute"), ("up", "submit"), ("down", "compute"), ("up", "compute"))
SEGMENTER_DEPTHS = (1, 2, 3)
LOADER_LEGS = (("decode", "launch"), ("consumer", "launch"))

SCENARIOS = {
    "online": [(s, p) for s in LOOP_STREAMS for p in LOOP_POINTS],
    "offline": [(s, p) for s in LOOP_STREAMS for p in OFFLINE_POINTS],
    "data_parallel": list(DP_LEGS),
    "nets": [(s, "forward:before") for legs in NET_LEGS.values() for s in legs],
    "segmenters": list(SEGMENTER_LEGS),
    "loader": list(LOADER_LEGS),
    "mutation_training": [("caller", "step:late")],
    "mutation_segmenter": [("up", "submit")],
}
STREAM_ROLES = ("caller", "aux", "pass", "comm", "net", "up", "down", "decode", "consumer")


# ---------------------------------------------------------------------------------------------- the device side
class Calibration:
    """Cycles of ``torch.cuda._sleep`` per millisecond on ``device``, from two events around one spin (the best of three
    after a warm-up: the fastest clock seen, so that a length in cycles is never shorter than asked for)."""

    PROBE_CYCLES = 2_000_000

    def __init__(self, device):
        self.device = torch.device(device)
        self._lengths = {}
        self.measure(self.PROBE_CYCLES)
        ms = min(self.measure(self.PROBE_CYCLES) for _ in range(3))
        self.cycles_per_ms = self.PROBE_CYCLES / ms

    def measure(self, cycles, stream=None):
        """Milliseconds between two events around one spin of ``cycles`` on ``stream`` (default: the current one)."""
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(st):
            a.record()
            torch.cuda._sleep(int(cycles))
            b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def cycles_for(self, ms):
        """Cycles of a spin of AT LEAST ``ms``: chosen with a margin, measured once again, lengthened until the measurement
        is at least the length asked for (at most three times: a clock that keeps running away is a failure)."""
        key = round(float(ms), 3)
        if key not in self._lengths:
            cycles = int(1.25 * ms * self.cycles_per_ms) + 1
            for _ in range(4):
                got = self.measure(cycles)
                if got >= ms:
                    break
                cycles = int(cycles * 1.5 * ms / max(got, 1e-3)) + 1
            assert got >= ms, "a spin of %d cycles took %.3f ms, %.3f ms were asked for" % (cycles, got, ms)
            self._lengths[key] = (cycles, got)
        return self._lengths[key][0]

    def measured(self, ms):
        """What the spin chosen for ``ms`` measured when it was chosen."""
        self.cycles_for(ms)
        return self._lengths[round(float(ms), 3)][1]


_CALIBRATIONS = {}


def calibration(device):
    """The device's Calibration (made once per process and device)."""
    dev = torch.device(device)
    key = (dev.type, dev.index if dev.index is not None else torch.cuda.current_device())
    if key not in _CALIBRATIONS:
        _CALIBRATIONS[key] = Calibration(dev)
        print("stream_delays: calibration on %s: %.0f cycles per ms" % (dev, _CALIBRATIONS[key].cycles_per_ms))
    return _CALIBRATIONS[key]


def calibrate(device):
    """Cycles of the spin kernel per millisecond on ``device``."""
    return calibration(device).cycles_per_ms


def sleep_ms(stream, ms):
    """Queue a spin of at least ``ms`` on ``stream``."""
    cal = calibration(stream.device)
    cycles = cal.cycles_for(ms)
    with torch.cuda.stream(stream):
        torch.cuda._sleep(cycles)


SIGHT_MS = 2.0


def _sight(delayed, other, wait):
    dev = delayed.device
    x = torch.zeros(4096, device=dev)
    torch.cuda.synchronize(dev)
    sleep_ms(delayed, SIGHT_MS)
    with torch.cuda.stream(delayed):
        x.fill_(1)
    with torch.cuda.stream(other):
        if wait:
            other.wait_stream(delayed)
        y = x.clone()
    torch.cuda.synchronize(dev)
    return y.cpu()


def sighted(delayed, other):
    """Can a missing wait of ``other`` on ``delayed`` show?  ``delayed`` sleeps, then fills x with ones; ``other`` clones x
    with no wait.  Sighted iff the clone is all zeros: ``other`` ran ahead.  Two streams on one hardware queue are blind."""
    y = _sight(delayed, other, wait=False)
    return bool((y == 0).all())


def ordered(delayed, other):
    """The same pair with ``other.wait_stream(delayed)``: the clone must be all ones."""
    y = _sight(delayed, other, wait=True)
    return bool((y == 1).all())


def timed(fn, device, units):
    """(fn's value, host milliseconds per unit): ``fn`` between two device synchronisations."""
    torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize(device)
    return out, (time.perf_counter() - t0) * 1e3 / max(int(units), 1)
