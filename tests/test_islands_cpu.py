"""The detector must detect (no GPU): tests/islands.py on fake ops written in torch, on islands built with device="cpu".  A
correct fake 3x3 convolution passes all three runs; each planted fault is reported with the right operand and location; the
island geometry follows the margin rule."""
import pytest
import torch
import torch.nn.functional as F

import islands as I

H, W, C, CO = 5, 7, 8, 8
BF, F32 = torch.bfloat16, torch.float32


def _data():
    g = torch.Generator().manual_seed(77)
    x = torch.randint(-8, 9, (1, H, W, C), generator=g).float()
    w = torch.randint(-4, 5, (CO, C, 3, 3), generator=g).float()
    y = F.conv2d(x.permute(0, 3, 1, 2), w, None, padding=1).permute(0, 2, 3, 1).contiguous()
    assert float(y.abs().max()) < 2 ** 24
    return x.to(BF), w, y.to(BF)


X, WT, Y = _data()
WS_BYTES = H * W * CO * 4


def operands():
    return [I.inp("x", X), I.inp("w", WT), I.out("y", (1, H, W, CO), BF), I.workspace("ws", WS_BYTES)]


def relu_laundering(t):
    """relu_f of csrc/common.hpp: a signed-integer max on the float's bits.  A NaN with the sign bit set becomes 0."""
    return torch.clamp(t.contiguous().view(torch.int32), min=0).view(torch.float32)


def conv(isl, fault=None, arg=None):
    """The fake op: fp32 partial sums through the workspace, then the bf16 output.  ``fault`` plants one misbehaviour."""
    a = isl.arena
    x, w, y = isl.view("x"), isl.view("w"), isl.view("y")
    ws = a[isl.start["ws"]:isl.end["ws"]].view(F32).view(1, H, W, CO)
    stale = a[isl.start["ws"]:isl.start["ws"] + 16].float().sum()  # (what the workspace held, as byte values)
    ws.copy_(F.conv2d(x.float().permute(0, 3, 1, 2), w, None, padding=1).permute(0, 2, 3, 1))
    behind_x = a[isl.end["x"]:isl.end["x"] + 2 * 64].view(BF).float()  # (the first 64 elements behind x)
    if fault == "zero_weight_read":
        ws[0, H - 1, W - 1, CO - 1] += behind_x[0] * 0.0
    if fault == "laundered_read":  # -(stray) through the ReLU, added to a pixel; arg: which element behind x
        ws[0, H - 1, W - 1, CO - 1] += relu_laundering(-behind_x[arg:arg + 1])[0]
    if fault == "stale_workspace":
        ws[0, 0, 0, 0] += stale
    keep = y[0, 2, 3, 4].clone()
    y.copy_(ws.to(BF))
    if fault == "unwritten":
        y[0, 2, 3, 4] = keep
    if fault == "byte_in_front_of_y":
        a[isl.start["y"] - 1] += 1
    if fault == "element_behind_y":
        a[isl.end["y"]:isl.end["y"] + 2] += 1
    if fault == "far_stores":  # 1 row, 2 pixels and 3 channels behind y; exactly one row in front of x
        a[isl.end["y"] + 2 * (W * CO + 2 * CO + 3 - 1)] += 1
        a[isl.start["x"] - 2 * W * C] += 1
    if fault == "past_workspace":
        a[isl.end["ws"]:isl.end["ws"] + 4] += 1
    if fault == "input_in_place":
        x[0, 1, 2, 3] += 1


def run(fault=None, arg=None):
    return I.run_case(f"fake conv, {fault}", operands(), lambda isl: conv(isl, fault, arg), {"y": Y}, device="cpu", seed=5)


def test_correct_fake_conv_passes_all_three_runs():
    r = run()
    assert set(r.fails) == set(I.RUNS) and r.ok(), r.lines()
    for k in I.RUNS:
        assert torch.equal(r.outputs[k]["y"].view(torch.int16), Y.view(torch.int16))
    r.check()


def _all_runs_say(r, *words):
    for k in I.RUNS:
        assert any(all(w in line for w in words) for line in r.fails[k]), (k, words, r.fails[k])
    with pytest.raises(AssertionError):
        r.check()


def test_one_byte_stored_in_front_of_the_output():
    _all_runs_say(run("byte_in_front_of_y"), "margin of y, front", "1 bytes changed", "(0 rows, 0 pixels, 1 channels) in front of the first")


def test_one_element_stored_behind_the_output():
    _all_runs_say(run("element_behind_y"), "margin of y, back", "2 bytes changed", "(0 rows, 0 pixels, 1 channels) behind the last")


def test_distances_are_given_in_rows_pixels_and_channels():
    r = run("far_stores")
    _all_runs_say(r, "margin of y, back", "1 bytes changed", "(1 rows, 2 pixels, 3 channels) behind the last")
    _all_runs_say(r, "margin of x, front", "1 bytes changed", "(1 rows, 0 pixels, 0 channels) in front of the first")


def test_read_behind_an_input_times_a_zero_weight_fails_run_N_only():
    r = run("zero_weight_read")
    assert r.ok("Z") and r.ok("B") and not r.ok("N")
    assert any("output y" in m and "NON-FINITE" in m and f"first at (0, {H - 1}, {W - 1}, {CO - 1})" in m for m in r.fails["N"])
    assert len(r.read) == 1 and "surroundings of x (back) were read" in r.read[0], r.read
    with pytest.raises(AssertionError, match="surroundings of x"):
        r.check()


def test_laundered_read_behind_an_input_fails_run_B():
    """The stray value goes through a sign flip and the sign-laundering ReLU: the positive NaN of run N becomes a negative one
    and then 0, so run N passes (as a 0xFF poison would have passed anywhere).  The element is picked where run B planted a
    NEGATIVE value, so that run B sees 2^90 or more in the output."""
    isl = I.Islands(operands(), "B", "cpu", seed=5)
    behind = isl.arena[isl.end["x"]:isl.end["x"] + 2 * 64].view(BF).float()
    assert bool((behind.abs() >= 2.0 ** 90).all()) and bool((behind.abs() <= 2.0 ** 97).all())
    k = int((behind < 0).nonzero()[0])
    nan = I.Islands(operands(), "N", "cpu", seed=5)
    stray = nan.arena[nan.end["x"]:nan.end["x"] + 2].view(BF).float()
    assert float(relu_laundering(-stray)) == 0.0 and torch.isnan(relu_laundering(stray)).all()
    r = run("laundered_read", k)
    assert r.ok("Z") and r.ok("N") and not r.ok("B"), r.lines()
    assert any("output y" in m and f"first at (0, {H - 1}, {W - 1}, {CO - 1})" in m for m in r.fails["B"])


def test_one_output_element_left_unwritten():
    assert float(Y[0, 2, 3, 4]) != 0.0  # (so that run Z's zero pre-fill shows it too)
    _all_runs_say(run("unwritten"), "output y", "1 / %d elements differ" % Y.numel(), "first at (0, 2, 3, 4)")
    assert any("NON-FINITE" in m for m in run("unwritten").fails["N"])


def test_result_that_depends_on_the_previous_workspace_content():
    r = run("stale_workspace")
    assert r.ok("Z") and not r.ok("N") and not r.ok("B")
    for k in ("N", "B"):
        assert any("output y" in m and "first at (0, 0, 0, 0)" in m for m in r.fails[k])
    assert r.read == []  # no input's surroundings are to blame


def test_store_past_the_reported_workspace_size():
    _all_runs_say(run("past_workspace"), "margin of ws, back", "4 bytes changed", "1 elements behind the last")


def test_input_modified_in_place():
    _all_runs_say(run("input_in_place"), "input x modified in place", "1 bytes changed", f"first at element {(1 * W + 2) * C + 3}")


def test_one_case_reports_all_failed_forms_together():
    rep = I.Report("case")
    rep.add(run())
    rep.add(run("unwritten"))
    rep.add(run("past_workspace"))
    with pytest.raises(AssertionError) as e:
        rep.done()
    assert "unwritten" in str(e.value) and "past_workspace" in str(e.value) and "fake conv, None" not in str(e.value)


def test_island_geometry():
    big = I.inp("big", torch.zeros(2, 40, 300, 64, dtype=BF))
    f32map = I.out("side", (1, 30, 54, 16), F32)
    ops_ = operands() + [big, f32map, I.inp("void", torch.zeros(15, dtype=torch.uint8)),
                         I.inp("logits", torch.zeros(1, 1, 3, 5), is_map=False, offset=16)]
    assert (17 * 300 * 64 + 64) * 2 <= big.margin < (17 * 300 * 64 + 64) * 2 + 256 and big.margin % 256 == 0 and big.margin > I.FLAT_MARGIN
    assert I.margin_bytes((1, 61, 107, 64), BF, True) == I._ru((17 * 107 * 64 + 64) * 2, 256)
    assert f32map.margin == I.FLAT_MARGIN == 65536  # 17 rows of it are 58816 bytes: the floor holds
    for run_ in I.RUNS:
        isl = I.Islands(ops_, run_, "cpu", seed=3)
        base = isl.arena.data_ptr()
        assert base % 256 == 0 and isl.arena.dtype == torch.uint8 and isl.arena.numel() == isl.total
        prev = 0
        for o in ops_:
            lo, a, b, hi = isl.lo[o.name], isl.start[o.name], isl.end[o.name], isl.hi[o.name]
            assert lo == prev and a - lo >= o.margin and hi - b >= o.margin and b - a == o.nbytes and hi <= isl.total
            assert (base + a) % 256 == o.offset and isl.ptr(o.name) == base + a
            v = isl.view(o.name)  # one allocation: every operand is a view into the arena's storage
            assert v.untyped_storage().data_ptr() == isl.arena.untyped_storage().data_ptr()
            if o.data is not None:
                assert torch.equal(v.contiguous().view(torch.uint8).reshape(-1), o.data.view(torch.uint8).reshape(-1))
            else:
                raw = isl.arena[a:b]
                assert {"Z": bool((raw == 0).all()), "N": bool((raw == 255).all()), "B": len(raw.unique()) > 2}[run_]
            prev = hi
            for p, q in ((lo, a), (b, hi)):
                m = isl.arena[p:q]
                if run_ == "Z":
                    assert bool((m == 0).all())
                elif o.dtype == torch.uint8:
                    assert bool((m == (0xFF if run_ == "N" else 0xA5)).all())
                elif run_ == "N":
                    bits = m.view(torch.int16 if o.dtype == BF else torch.int32)
                    assert bool((bits == (0x7FC0 if o.dtype == BF else 0x7FC00000)).all())  # positive, quiet
                    assert bool(torch.isnan(m.view(o.dtype)).all()) and bool((bits > 0).all())
                else:
                    val = m.view(o.dtype).float()
                    assert bool((val.abs() >= 2.0 ** 90).all()) and bool((val.abs() <= 2.0 ** 97).all())
                    assert torch.equal(val.to(BF).float(), val) and 0.3 < float((val < 0).float().mean()) < 0.7
                    assert len(val.abs().unique()) == 8
        assert prev == isl.total
    a, b = I.Islands(ops_, "B", "cpu", seed=3), I.Islands(ops_, "B", "cpu", seed=3)
    assert torch.equal(a.arena, b.arena)  # seeded


def _file_operands(prefill):
    """A fake file encoder's operands (tests/test_gpu_io_islands.py): two slots of 40 bytes in an IN-OUT buffer that begins at
    an odd address, the lengths, a workspace at the 4 bytes such an entry asks for."""
    return [I.inp("bytes", torch.arange(24, dtype=torch.uint8).view(2, 12), offset=3), I.inout("out", prefill, offset=1),
            I.out("lengths", (2,), torch.int32, offset=4), I.workspace("ws", 32, offset=4)]


def _fake_encoder(isl, fault=None):
    """File n = the frame's 12 bytes behind a 2-byte mark, in slot n; the bytes behind a file stay as they were."""
    src, out, lengths = isl.view("bytes"), isl.view("out"), isl.view("lengths")
    isl.arena[isl.start["ws"]:isl.end["ws"]] = 7
    for n in range(2):
        out[40 * n:40 * n + 2] = 0x4D
        out[40 * n + 2:40 * n + 14] = src[n]
        lengths[n] = 14
    if fault == "ragged_tail":  # the last dword of a file copied whole: two bytes behind the file, inside its slot
        out[14:16] = 0
    if fault == "prefill_in_file":  # a file byte that depends on what the slot held
        out[40 + 5] ^= out[40 + 20]


def test_offsets_of_in_out_and_workspace_operands_and_a_store_behind_a_file():
    """An in-out operand and a workspace take an ``offset`` like inputs and outputs do.  A file of variable length lives in
    an in-out slot: its pre-fill is data, so a store behind the file but inside the slot - which no margin sees - is a
    differing output element, under either pre-fill."""
    g = torch.Generator().manual_seed(3)
    for k in range(2):
        prefill = torch.randint(0, 256, (80,), generator=g, dtype=torch.uint8)
        ops_ = _file_operands(prefill)
        for run_ in I.RUNS:
            isl = I.Islands(ops_, run_, "cpu", seed=k)
            for o in ops_:
                assert (isl.arena.data_ptr() + isl.start[o.name]) % 256 == o.offset == {"bytes": 3, "out": 1, "lengths": 4, "ws": 4}[o.name]
                assert isl.start[o.name] - isl.lo[o.name] >= o.margin and isl.hi[o.name] - isl.end[o.name] >= o.margin
            assert torch.equal(isl.view("out"), prefill)  # the same data in every run
        want = prefill.clone()
        for n in range(2):
            want[40 * n:40 * n + 2] = 0x4D
            want[40 * n + 2:40 * n + 14] = torch.arange(12 * n, 12 * n + 12, dtype=torch.uint8)
        expected = {"out": want, "lengths": torch.tensor([14, 14], dtype=torch.int32)}
        assert int(prefill[14]) != 0 and int(prefill[60]) != 0
        r = I.run_case("fake encoder", ops_, _fake_encoder, expected, device="cpu", seed=k)
        assert r.ok(), r.lines()
        _all_runs_say(I.run_case("ragged", ops_, lambda isl: _fake_encoder(isl, "ragged_tail"), expected, device="cpu", seed=k),
                      "output out", "first at (14,)")
        _all_runs_say(I.run_case("dep", ops_, lambda isl: _fake_encoder(isl, "prefill_in_file"), expected, device="cpu", seed=k),
                      "output out", "1 / 80 elements differ", "first at (45,)")


def test_loss_void_maps_leave_both_classes():
    """The loss cases of tests/test_gpu_islands.py: neither class is empty among the valid pixels of any frame, nor in the
    labels, and every frame has void pixels."""
    from test_gpu_islands import LOSS_SHAPES, loss_inputs
    for shape in LOSS_SHAPES:
        _, label, void = loss_inputs(shape)
        valid = (void == 0).reshape(shape[0], -1)
        pos = (label >= 0.5).reshape(shape[0], -1)
        assert bool((valid & pos).any(1).all()) and bool((valid & ~pos).any(1).all()) and bool((~valid).any(1).all())
        assert bool(pos.any(1).all()) and bool((~pos).any(1).all())
