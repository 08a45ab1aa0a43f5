"""Island tests: every operand of a raw C-ABI call sits alone between two margins the test owns, and the call runs three times
on different surroundings.  Shared by tests/test_islands_cpu.py (the detector on fake ops that misbehave on purpose, no GPU)
and tests/test_gpu_islands.py (the kernels of the VGG step).  A plain module: nothing here is a fixture or a pytest setting.

The island.  [front margin | operand | back margin], operand = an input, an output, an in-out tensor or the workspace.  All
islands of one call are carved out of ONE torch.uint8 allocation, so a stray access that stays within a margin stays inside
memory the test owns.  An operand starts at a multiple of 256 bytes (plus ``offset`` where a case asks for the least alignment
an entry point allows).  A map [N,H,W,C] gets margins of at least 17 rows plus one pixel of itself (the tallest tile is 16
rows and a halo row) and never less than 64 KiB, rounded up to 256; vectors, weights, loss outputs and workspaces get 64 KiB.
Every kind of operand takes an ``offset``, in-out operands and workspaces included.  A file of variable length (the PNG and
JPEG encoders) lives in an in-out slot: the pre-fill behind the file is part of the expected bits.

Three runs of every case, which differ only in what surrounds and pre-fills the operands:
  Z  margins of zero bytes; outputs and workspace pre-filled with 0x00.
  N  every margin holds the POSITIVE quiet NaN of the operand's element type (bf16 0x7FC0, fp32 0x7FC00000; byte and integer
     operands 0xFF); outputs and workspace pre-filled with 0xFF.  Positive, because relu_f (csrc/common.hpp) is a signed
     integer max on the float's bits: a NaN with the sign bit set becomes 0, so the 0xFF poison would be laundered by every
     ReLU epilogue.  NaN x 0 is NaN: a stray operand is seen even where it meets a zero weight or a zero-padded channel.
  B  margins of large finite values from a seeded generator, random sign, magnitude 2^(90+k), k in 0..7 (all of them bf16
     values; byte operands 0xA5); outputs and workspace pre-filled with seeded random bytes.  Catches a stray read where a NaN
     would be laundered (a sign flip in front of a ReLU, a comparison).

After each run: (a) every output equals the expected bits - which implies that the three runs agree, i.e. that no surrounding
value was read, that every output byte was written and none was read, and that nothing depends on what the workspace held
(in-out operands - accumulate, an addend aliased to the output - carry their pre-fill as DATA: it is an operand, the same in
all runs, and part of the reference); (b) every margin is byte for byte what it was; (c) every pure input is byte for byte
what it was; (d) the workspace island holds exactly the bytes the matching *_workspace_bytes reports, so a store past them is
a changed margin.  Where no expected bits are given for an output, run Z's bits are the expectation of runs N and B.

A failure says which operand, front or back, how many bytes changed and where the first one lies, as a distance from the
operand's first / last element in (rows, pixels, channels) or in elements; for outputs how many elements differ, the first
index, both values and whether the value is non-finite.  Only after a failure the helper repeats run N with the poison
around one input (and one side) at a time - every other margin and the pre-fills as in run Z, so that what still differs
came from that margin - and names the input whose surroundings were read.

The limit of the method.  A stray READ is seen only through its effect.  A load whose value is discarded - a lane that is
masked after the load, a prefetch nobody consumes - passes all three runs.  Stray stores are seen wherever they land inside
a margin."""
import torch

ALIGN = 256
FLAT_MARGIN = 64 * 1024
RUNS = ("Z", "N", "B")
_ESIZE = {torch.bfloat16: 2, torch.float32: 4, torch.uint8: 1, torch.int32: 4, torch.float64: 8}
_BITS = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
_NAN_BITS = {torch.bfloat16: 0x7FC0, torch.float32: 0x7FC00000}


def _ru(a, b):
    return (a + b - 1) // b * b


def margin_bytes(shape, dtype, is_map):
    """The margin rule (one side)."""
    if not is_map:
        return FLAT_MARGIN
    n, h, w, c = shape
    return _ru(max(FLAT_MARGIN, (17 * w * c + c) * _ESIZE[dtype]), ALIGN)


class Operand:
    """One operand of a call.  kind: "in" (pure input, ``data`` given), "out" (pre-filled per run), "inout" (``data`` is the
    pre-fill in every run and the operand is written), "ws" (bytes, pre-filled per run)."""

    def __init__(self, name, kind, shape, dtype, data=None, is_map=False, offset=0):
        assert kind in ("in", "out", "inout", "ws") and dtype in _ESIZE and offset % _ESIZE[dtype] == 0
        assert not is_map or len(shape) == 4
        self.name, self.kind, self.shape, self.dtype, self.is_map, self.offset = name, kind, tuple(shape), dtype, is_map, offset
        self.data = None if data is None else data.detach().cpu().contiguous()
        assert (self.data is None) == (kind in ("out", "ws"))
        assert self.data is None or (tuple(self.data.shape) == self.shape and self.data.dtype == dtype)
        self.numel = 1
        for s in self.shape:
            self.numel *= int(s)
        self.nbytes = self.numel * _ESIZE[dtype]
        self.margin = margin_bytes(self.shape, dtype, is_map)


def inp(name, data, is_map=None, offset=0):
    return Operand(name, "in", data.shape, data.dtype, data, data.dim() == 4 if is_map is None else is_map, offset)


def out(name, shape, dtype, is_map=None, offset=0):
    return Operand(name, "out", shape, dtype, None, len(shape) == 4 if is_map is None else is_map, offset)


def inout(name, data, is_map=None, offset=0):
    return Operand(name, "inout", data.shape, data.dtype, data, data.dim() == 4 if is_map is None else is_map, offset)


def workspace(name, nbytes, margin=None, offset=0):
    """margin: a larger margin than the flat one (an arena that holds maps); offset: the least alignment the entry accepts."""
    o = Operand(name, "ws", (int(nbytes),), torch.uint8, offset=offset)
    if margin is not None:
        assert margin % ALIGN == 0 and margin >= FLAT_MARGIN
        o.margin = margin
    return o


def _margin_fill(op, run, nbytes, gen):
    """``nbytes`` of margin content for one side of ``op`` in run ``run`` (uint8, cpu)."""
    if run == "Z":
        return torch.zeros(nbytes, dtype=torch.uint8)
    es = _ESIZE[op.dtype]
    if op.dtype not in _NAN_BITS:
        return torch.full((nbytes,), 0xFF if run == "N" else 0xA5, dtype=torch.uint8)
    assert nbytes % es == 0
    n = nbytes // es
    if run == "N":
        return torch.full((n,), _NAN_BITS[op.dtype], dtype=torch.int32).to(_BITS[es]).view(torch.uint8)
    sign = torch.randint(0, 2, (n,), generator=gen, dtype=torch.int32)
    expo = 127 + 90 + torch.randint(0, 8, (n,), generator=gen, dtype=torch.int32)
    if op.dtype == torch.bfloat16:
        bits = (expo << 7) - (sign << 15)  # as a signed 16-bit pattern: sign bit set = minus 2^15
        return bits.to(torch.int16).view(torch.uint8)
    bits = (expo << 23) + sign * (-2 ** 31)
    return bits.view(torch.uint8)


def _random_bytes(nbytes, gen):
    words = torch.randint(-2 ** 63, 2 ** 63 - 1, ((nbytes + 7) // 8,), generator=gen, dtype=torch.int64)
    return words.view(torch.uint8)[:nbytes]


class Islands:
    """The islands of one call in one run.  ``arena``: the one allocation; ``start[name]`` / ``end[name]``: byte range of the
    operand in it; ``lo[name]`` / ``hi[name]``: byte range of the whole island."""

    def __init__(self, operands, run, device, seed=0, poison=None):
        """poison: None = every margin as the run says; else a set of (operand name, "front" | "back"): only these margins
        get the run's content, every other margin and the pre-fill of outputs and workspace are run Z's (the attribution
        runs: whatever still differs from the expected bits came from that one margin)."""
        self.operands, self.run, self.device = list(operands), run, torch.device(device)
        assert len({o.name for o in self.operands}) == len(self.operands)
        self.lo, self.start, self.end, self.hi = {}, {}, {}, {}
        at = 0
        for o in self.operands:
            self.lo[o.name] = at
            self.start[o.name] = at + o.margin + o.offset
            self.end[o.name] = self.start[o.name] + o.nbytes
            at = _ru(self.end[o.name] + o.margin, ALIGN)
            self.hi[o.name] = at
        self.total = at
        gen = torch.Generator().manual_seed(1000003 * seed + 17)
        host = torch.empty(self.total + ALIGN, dtype=torch.uint8)
        raw = torch.empty(self.total + ALIGN, dtype=torch.uint8, device=self.device)
        self.base = (-raw.data_ptr()) % ALIGN
        self._raw = raw
        img = host[:self.total]
        for o in self.operands:
            lo, a, b, hi = self.lo[o.name], self.start[o.name], self.end[o.name], self.hi[o.name]
            for side, (p, q) in (("front", (lo, a)), ("back", (b, hi))):
                on = poison is None or (o.name, side) in poison
                img[p:q] = _margin_fill(o, run if on else "Z", q - p, gen)
            if o.data is not None:
                img[a:b] = o.data.reshape(-1).view(torch.uint8)
            elif poison is not None:
                img[a:b] = 0x00
            elif run == "B":
                img[a:b] = _random_bytes(b - a, gen)
            else:
                img[a:b] = 0x00 if run == "Z" else 0xFF
        self.arena = raw[self.base:self.base + self.total]
        self.arena.copy_(img)
        self.before = self.arena.clone()

    def op(self, name):
        return next(o for o in self.operands if o.name == name)

    def ptr(self, name):
        """Device (or host) address of the operand's first element; None for an unknown name is an error."""
        return self.arena.data_ptr() + self.start[name]

    def view(self, name):
        """The operand as a typed tensor view into the arena."""
        o = self.op(name)
        return self.arena[self.start[name]:self.end[name]].view(o.dtype).view(*o.shape)

    def nbytes(self, name):
        return self.op(name).nbytes


# ------------------------------------------------------------------------------------------ the failure report
def _where(o, delta_bytes, side):
    """Distance of a byte from the operand's first (front) or last (back) element, in the operand's own units."""
    es = _ESIZE[o.dtype]
    elems = (delta_bytes + es - 1) // es  # 1 = the element next to the operand
    if o.is_map:
        n, h, w, c = o.shape
        rows, rest = divmod(elems, w * c)
        px, ch = divmod(rest, c)
        return f"{elems} elements = ({rows} rows, {px} pixels, {ch} channels) {'in front of the first' if side == 'front' else 'behind the last'} element"
    return f"{elems} elements {'in front of the first' if side == 'front' else 'behind the last'} element"


def _changed(now, before):
    d = (now != before).nonzero()
    return int(d.numel()), (int(d[0]), int(d[-1])) if d.numel() else None


def _int_view(t):
    return t.contiguous().view(_BITS[t.element_size()])


def compare_output(o, got, want):
    """None, or one line: how many elements differ, the first index, both values, non-finite or not."""
    want = want.to(got.device)
    if tuple(want.shape) != tuple(got.shape) or want.dtype != got.dtype:
        return f"expected bits have shape/dtype {tuple(want.shape)} {want.dtype}, the operand {tuple(got.shape)} {got.dtype}"
    bad = _int_view(got) != _int_view(want)
    n_bad = int(bad.sum())
    if n_bad == 0:
        return None
    idx = tuple(int(i) for i in bad.nonzero()[0])
    g, w = got[idx], want[idx]
    finite = bool(torch.isfinite(g.float())) if g.dtype.is_floating_point else True
    return (f"{n_bad} / {bad.numel()} elements differ; first at {idx}: got {g.item()!r} (bits {int(_int_view(got)[idx]) & (2 ** (8 * got.element_size()) - 1):#x}), "
            f"expected {w.item()!r}; the value is {'finite' if finite else 'NON-FINITE'}")


def inspect(isl, expected):
    """The failures of one finished run: list of lines (empty = the run holds a, b, c and d).  expected: name -> tensor."""
    fails = []
    now, before = isl.arena, isl.before
    for o in isl.operands:
        lo, a, b, hi = isl.lo[o.name], isl.start[o.name], isl.end[o.name], isl.hi[o.name]
        if not torch.equal(now[lo:a], before[lo:a]):
            cnt, (first, last) = _changed(now[lo:a], before[lo:a])
            fails.append(f"margin of {o.name}, front: {cnt} bytes changed; nearest to the operand {_where(o, a - lo - last, 'front')}, "
                         f"first changed byte {_where(o, a - lo - first, 'front')}")
        if not torch.equal(now[b:hi], before[b:hi]):
            cnt, (first, last) = _changed(now[b:hi], before[b:hi])
            fails.append(f"margin of {o.name}, back: {cnt} bytes changed; first changed byte {_where(o, first + 1, 'back')}")
        if o.kind == "in" and not torch.equal(now[a:b], before[a:b]):
            cnt, (first, last) = _changed(now[a:b], before[a:b])
            fails.append(f"input {o.name} modified in place: {cnt} bytes changed; first at element {first // _ESIZE[o.dtype]}")
        if o.kind in ("out", "inout") and o.name in expected:
            msg = compare_output(o, isl.view(o.name), expected[o.name])
            if msg is not None:
                fails.append(f"output {o.name}: {msg}")
    return fails


class Result:
    """What ``run_case`` found: ``fails[run]`` = the lines of that run, ``read`` = the attribution lines, ``outputs[run]`` =
    name -> cpu tensor."""

    def __init__(self, tag):
        self.tag, self.fails, self.read, self.outputs = tag, {}, [], {}

    def ok(self, run=None):
        return not (self.fails[run] if run else any(self.fails.values()))

    def lines(self):
        out_ = [f"run {r}: {m}" for r in RUNS for m in self.fails.get(r, [])]
        return out_ + self.read

    def check(self):
        assert self.ok(), f"[{self.tag}] " + " || ".join(self.lines())


def _sync(device):
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize()


def run_case(tag, operands, call, expected=None, device="cuda:0", seed=0, attribute=True):
    """Run ``call(islands)`` three times (Z, N, B) on fresh islands of ``operands`` and inspect each run.  expected: name ->
    cpu tensor of the bits an output (or in-out operand) must hold; an output without an entry must hold run Z's bits in runs
    N and B.  Returns a Result; ``.check()`` asserts it."""
    res = Result(tag)
    expected = dict(expected or {})
    for run in RUNS:
        isl = Islands(operands, run, device, seed)
        call(isl)
        _sync(device)
        res.fails[run] = inspect(isl, expected)
        res.outputs[run] = {o.name: isl.view(o.name).cpu().clone() for o in operands if o.kind in ("out", "inout")}
        if run == "Z":
            for name, t in res.outputs["Z"].items():
                expected.setdefault(name, t)
        del isl
    if attribute and not res.ok():
        for o in operands:
            if o.kind != "in":
                continue
            for side in ("front", "back"):
                isl = Islands(operands, "N", device, seed, poison={(o.name, side)})
                call(isl)
                _sync(device)
                hit = [m for m in inspect(isl, expected) if m.startswith("output")]
                if hit:
                    res.read.append(f"poison around {o.name} alone ({side}) reaches the outputs: the surroundings of {o.name} "
                                    f"({side}) were read [{hit[0]}]")
                del isl
    return res


class Report:
    """Collects the failed forms of one case (as Report in tests/test_gpu_exact.py): every form runs, one assertion lists all."""

    def __init__(self, tag):
        self.tag, self.bad = tag, []

    def add(self, result):
        if not result.ok():
            self.bad.append(f"<{result.tag}> " + " || ".join(result.lines()))

    def done(self):
        assert not self.bad, f"[{self.tag}] " + " ## ".join(self.bad)
