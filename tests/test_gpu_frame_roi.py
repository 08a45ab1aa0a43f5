"""Following the object, on a real MI355X: ``ops.frame_prep_window``, ``ops.overlay_window`` and ``ops.window_next``
(csrc/stream.hip: k_frame_prep_window, k_overlay_window, k_window_reset + k_window_next) against the numpy statement of the
arithmetic (util/frame_roi.py) - exact equality for the prep, the boolean modes and the windows, everywhere but within 1e-9 of a
rounding boundary for the soft modes; the entries on islands; ``FrameSegmenter(roi=)`` end to end against ``frame_roi.track``."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fosvos_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import frame_roi_cases as C  # noqa: E402
import islands as I  # noqa: E402
from util import frame_overlay as F  # noqa: E402
from util import frame_roi as W  # noqa: E402
from util import mask_components as M  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def offset_view(t, elems=1):
    """The same values in a tensor whose base pointer lies `elems` elements behind an allocation's start."""
    buf = torch.empty(t.numel() + elems, dtype=t.dtype, device=t.device)
    view = buf[elems:].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() == buf.data_ptr() + elems * t.element_size()
    return view


def garbage(shape, dtype):
    if dtype == torch.uint8:
        return torch.full(shape, 0xA5, dtype=dtype, device=DEV)
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def on_device(case, windows, zeros=True):
    n, hf, wf, hn, wn = case
    f, x, w = C.frames(n, hf, wf), C.logits(n, hn, wn, zeros=zeros), C.windows_array(windows)
    return f, x, w, torch.from_numpy(f).to(DEV), torch.from_numpy(x).to(DEV), torch.from_numpy(w).to(DEV)


# ------------------------------------------------------------------------------------------ frame_prep_window
@pytest.mark.parametrize("case,windows", C.CASES, ids=C.IDS)
def test_frame_prep_window_is_prepare_frame_window(case, windows):
    from fosvos_hip import ops
    n, hf, wf, hn, wn = case
    f, _, w, fd, _, wd = on_device(case, windows)
    for mirror in (False, True):
        want = np.concatenate([W.prepare_frame_window(f[k], w[k], hn, wn, mirror) for k in range(n)])
        out = garbage((n, 3, hn, wn), torch.float32)
        assert ops.frame_prep_window(fd, wd, (hn, wn), mirror, out=out) is out
        got = out.cpu().numpy()
        assert got.tobytes() == want.tobytes(), (case, windows, mirror, int((got != want).sum()))
        again = ops.frame_prep_window(fd, wd, (hn, wn), mirror)
        assert again.shape == (n, 3, hn, wn) and torch.equal(again, out)
        # base pointers off every boundary: the frames by one byte, the image by one float, the windows by one int
        out2 = offset_view(garbage((n, 3, hn, wn), torch.float32))
        ops.frame_prep_window(offset_view(fd), offset_view(wd), (hn, wn), mirror, out=out2)
        assert out2.cpu().numpy().tobytes() == want.tobytes(), (case, windows, mirror, "offset")
        # what lies outside the windows is not part of the image
        poisoned = np.full_like(f, 0xA5)
        for k in range(n):
            y0, x0, hw, ww = W.sanitize(w[k], hf, wf, hn, wn)
            xs = wf - x0 - ww if mirror else x0
            poisoned[k, y0:y0 + hw, xs:xs + ww] = f[k, y0:y0 + hw, xs:xs + ww]
        got = ops.frame_prep_window(torch.from_numpy(poisoned).to(DEV), wd, (hn, wn), mirror).cpu().numpy()
        assert got.tobytes() == want.tobytes(), (case, windows, mirror, "poison outside the window")


@pytest.mark.parametrize("case", sorted({c for c, _ in C.CASES}), ids=lambda c: "%dx%dx%d_to_%dx%d" % c)
def test_whole_frame_windows_are_the_scaled_launches_on_the_device(case):
    from fosvos_hip import lib, ops
    n, hf, wf, hn, wn = case
    f, x, _, fd, xd, wd = on_device(case, [(0, 0, hf, wf)] * n)
    st = torch.cuda.current_stream().cuda_stream

    def scaled_prep(mirror):  # the C entry: the Python face never sends the frame's own size as the net's
        img = garbage((n, 3, hn, wn), torch.float32)
        assert lib().fosvos_frame_prep_scaled(fd.data_ptr(), n, hf, wf, hn, wn, int(mirror), ops._mean_bgr(), img.data_ptr(), 0,
                                              st) == 0
        return img

    def scaled_overlay(mirror, mode, out):
        assert lib().fosvos_overlay_scaled(fd.data_ptr(), xd.data_ptr(), n, hf, wf, hn, wn, int(mirror), mode, 1, 0.5,
                                           out.data_ptr(), 0, st) == 0
        return out

    for mirror in (False, True):
        assert torch.equal(ops.frame_prep_window(fd, wd, (hn, wn), mirror).view(torch.int32),
                           scaled_prep(mirror).view(torch.int32)), (case, mirror)
        for boolean in (True, False):
            for overlay in (True, False):
                mode = (0 if overlay else 2) + (0 if boolean else 1)
                want = scaled_overlay(mirror, mode, garbage((n, hf, wf, 3) if overlay else (n, hf, wf), torch.uint8))
                got = ops.overlay_window(fd, xd, wd, mirror, boolean, "g", 0.5, overlay)
                assert torch.equal(got, want), (case, mirror, boolean, overlay)


# ------------------------------------------------------------------------------------------ overlay_window, boolean
@pytest.mark.parametrize("case,windows", C.CASES, ids=C.IDS)
def test_boolean_overlay_window_is_exact(case, windows):
    from fosvos_hip import ops
    n, hf, wf, hn, wn = case
    f, x, w, fd, xd, wd = on_device(case, windows)
    fo, xo, wo = offset_view(fd), offset_view(xd), offset_view(wd)
    for mirror in (False, True):
        src = f[:, :, ::-1] if mirror else f
        for color in ("b", "r"):
            c = F.COLOR_CHANNEL[color]
            for alpha in C.ALPHAS:
                want = np.stack([W.overlay_window(f[k], x[k, 0], w[k], mirror, True, color, alpha) for k in range(n)])
                out = garbage((n, hf, wf, 3), torch.uint8)
                assert ops.overlay_window(fd, xd, wd, mirror, True, color, alpha, out=out) is out
                got = out.cpu().numpy()
                assert np.array_equal(got, want), (case, windows, mirror, color, alpha, int((got != want).sum()))
                others = [k for k in range(3) if k != c]
                assert np.array_equal(got[..., others], src[..., others])  # untouched channels: the (mirrored) input
        out = offset_view(garbage((n, hf, wf, 3), torch.uint8))
        ops.overlay_window(fo, xo, wo, mirror, True, "g", 0.5, out=out)
        want = np.stack([W.overlay_window(f[k], x[k, 0], w[k], mirror, True, "g", 0.5) for k in range(n)])
        assert np.array_equal(out.cpu().numpy(), want), (case, windows, mirror, "offset")
    # the mask bytes, at the frames' size (nothing to mirror: the windows and the logits are in output order)
    want = np.stack([W.mask_bytes_window(x[k, 0], w[k], hf, wf, True) for k in range(n)])
    for mirror in (False, True):
        out = garbage((n, hf, wf), torch.uint8)
        assert ops.overlay_window(fd, xd, wd, mirror, True, overlay=False, out=out) is out
        assert np.array_equal(out.cpu().numpy(), want), (case, windows, mirror)
    out = offset_view(garbage((n, hf, wf), torch.uint8))
    ops.overlay_window(fo, xo, wo, True, True, overlay=False, out=out)
    assert np.array_equal(out.cpu().numpy(), want)
    for k in range(n):  # nothing is object outside the window
        _, inside = W.logits_up_window(x[k, 0], w[k], hf, wf)
        assert (want[k][~inside] == 0).all()


# ------------------------------------------------------------------------------------------ overlay_window, soft
def test_soft_overlay_window_outside_the_rounding_band():
    """Every case in one test: the band's share is taken over all of them (on the host the reference alone has 0 band pixels
    of 952900 for these cases, far below BAND_SHARE)."""
    from fosvos_hip import ops
    n_band = n_all = 0

    def compare(got, want, band, what):
        nonlocal n_band, n_all
        diff = np.abs(got.astype(np.int32) - want.astype(np.int32))
        print(what, "band pixels", int(band.sum()), "differing", int((diff != 0).sum()))
        assert not (diff != 0)[~band].any(), (what, int((diff != 0)[~band].sum()))
        assert diff.max() <= 1, what
        n_band += int(band.sum())
        n_all += band.size

    for case, windows in C.CASES:
        n, hf, wf, hn, wn = case
        f, x, w, fd, xd, wd = on_device(case, windows, zeros=False)
        for mirror in (False, True):
            for color in ("b", "r"):
                c = F.COLOR_CHANNEL[color]
                for alpha in C.SOFT_ALPHAS:
                    want = np.stack([W.overlay_window(f[k], x[k, 0], w[k], mirror, False, color, alpha) for k in range(n)])
                    band = np.stack([C.soft_band_window(f[k], x[k, 0], w[k], mirror, True, color, alpha) for k in range(n)])
                    out = garbage((n, hf, wf, 3), torch.uint8)
                    got = ops.overlay_window(fd, xd, wd, mirror, False, color, alpha, out=out).cpu().numpy()
                    others = [k for k in range(3) if k != c]
                    assert np.array_equal(got[..., others], want[..., others])
                    compare(got[..., c], want[..., c], band, (case, windows, mirror, color, alpha))
            # alpha 0 adds an exact zero: no exclusion
            got = ops.overlay_window(fd, xd, wd, mirror, False, "r", 0.0).cpu().numpy()
            assert np.array_equal(got, f[:, :, ::-1] if mirror else f)
        want = np.stack([W.mask_bytes_window(x[k, 0], w[k], hf, wf, False) for k in range(n)])
        band = np.stack([C.soft_band_window(f[k], x[k, 0], w[k], False, False, "r", 1.0) for k in range(n)])
        out = offset_view(garbage((n, hf, wf), torch.uint8))
        got = ops.overlay_window(offset_view(fd), offset_view(xd), offset_view(wd), True, False, overlay=False, out=out).cpu().numpy()
        compare(got, want, band, (case, windows, "mask"))
        for k in range(n):  # exactly 0 outside the window, in the soft mask too
            _, inside = W.logits_up_window(x[k, 0], w[k], hf, wf)
            assert (got[k][~inside] == 0).all()
    print("band pixels", n_band, "of", n_all)
    assert n_band <= C.BAND_SHARE * n_all, (n_band, n_all)


# ------------------------------------------------------------------------------------------ window_next
def next_cases(hf, wf, hn, wn):
    """[(name, logits [Hn,Wn], window)]"""
    whole, some = (0, 0, hf, wf), (hf // 8, wf // 8, hn + (hf - hn) // 2, wn + (wf - wn) // 2)
    empty = np.full((hn, wn), -1.0, dtype=np.float32)
    out = [("empty", empty, some), ("all_nan", np.full((hn, wn), np.nan, dtype=np.float32), some)]
    x = empty.copy()
    x[hn // 3, wn // 2] = -0.0
    out.append(("minus_zero", x, some))
    x = empty.copy()
    x[hn // 3, wn // 2] = np.nan
    out.append(("one_nan", x, some))
    for name, (i, j) in (("corner_tl", (0, 0)), ("corner_tr", (0, wn - 1)), ("corner_bl", (hn - 1, 0)), ("corner_br", (hn - 1, wn - 1))):
        x = empty.copy()
        x[i, j] = 1.0
        out.append((name, x, whole))
        out.append((name + "_windowed", x, some))
    out.append(("large_box", C.blob(hn, wn, (1, hn - 2), (1, wn - 2)), whole))   # larger than every level but the last
    out.append(("blob", C.blob(hn, wn, (hn // 4, hn // 2), (wn // 3, wn // 2 + 1)), some))
    out.append(("blob_invalid_window", C.blob(hn, wn, (hn // 4, hn // 2), (wn // 3, wn // 2 + 1)), (C.INT32_MAX, C.INT32_MIN, 5, 5)))
    out.append(("noise", C.logits(1, hn, wn)[0, 0], some))
    return out


@pytest.mark.parametrize("hf,wf,hn,wn", [(96, 172, 24, 43), (200, 300, 70, 150), (33, 47, 33, 47), (40, 64, 1, 1)])
def test_window_next_is_next_window(hf, wf, hn, wn):
    from fosvos_hip import ops
    cases = next_cases(hf, wf, hn, wn)
    x = np.stack([c[1] for c in cases])[:, None]
    w = C.windows_array([c[2] for c in cases])
    xd, wd = torch.from_numpy(np.ascontiguousarray(x)).to(DEV), torch.from_numpy(w).to(DEV)
    for levels, margin, min_pad in ((8, 0.25, 16), (1, 0.25, 4), (64, 0.25, 4), (4, 0.0, 0), (8, 4.0, 2), (3, 0.0004, 1)):
        permille = int(round(1000 * margin))
        want = np.array([W.next_window(x[k, 0], w[k], hf, wf, levels, permille, min_pad) for k in range(len(cases))], dtype=np.int32)
        got = ops.window_next(xd, wd, (hf, wf), levels, margin, min_pad)
        assert got.dtype == torch.int32 and got.shape == (len(cases), 4)
        bad = [(cases[k][0], got[k].tolist(), want[k].tolist()) for k in range(len(cases)) if got[k].tolist() != want[k].tolist()]
        assert not bad, ((levels, margin, min_pad), bad)
        assert torch.equal(wd.cpu(), torch.from_numpy(w))  # the input windows are as they were
    # one frame at a time gives the same, and so does `out` aliasing `in`, off every boundary
    want = np.array([W.next_window(x[k, 0], w[k], hf, wf, 8, 250, 16) for k in range(len(cases))], dtype=np.int32)
    for k in (0, 2, len(cases) - 2):
        assert ops.window_next(xd[k:k + 1], wd[k:k + 1], (hf, wf)).tolist() == [want[k].tolist()]
    alias = offset_view(wd.clone())
    assert ops.window_next(offset_view(xd), alias, (hf, wf), out=alias) is alias
    assert alias.cpu().numpy().tolist() == want.tolist()


def test_window_next_three_frames_three_answers():
    from fosvos_hip import ops
    hf, wf, hn, wn = 96, 172, 24, 43
    x = np.stack([C.blob(hn, wn, (2, 5), (3, 9)), np.full((hn, wn), -1.0, dtype=np.float32), C.blob(hn, wn, (10, 20), (30, 40))])[:, None]
    w = C.windows_array([(0, 0, hf, wf), (5, 5, 60, 100), (20, 40, 60, 107)])
    want = [list(W.next_window(x[k, 0], w[k], hf, wf, 4, 250, 4)) for k in range(3)]
    assert len({tuple(r) for r in want}) == 3
    got = ops.window_next(torch.from_numpy(np.ascontiguousarray(x)).to(DEV), torch.from_numpy(w).to(DEV), (hf, wf), 4, 0.25, 4)
    assert got.tolist() == want


# ------------------------------------------------------------------------------------------ islands
def _st():
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize("windows", [[(3, 5, 21, 31), (9, 14, 17, 23)], [(0, 0, 33, 47), (17, 27, 16, 20)],
                                     [(C.INT32_MIN, C.INT32_MAX, C.INT32_MAX, C.INT32_MIN), (C.INT32_MAX, 0, 33, 47)],
                                     [(1, 1, C.INT32_MAX, C.INT32_MAX), (C.INT32_MIN, C.INT32_MIN, C.INT32_MIN, C.INT32_MIN)]],
                         ids=["valid", "edges", "int32_limits", "overflowing"])
def test_window_entries_on_islands(windows):
    """The three entries on operands between poisoned margins: nothing outside the operands is read or written, whatever the
    windows hold."""
    from fosvos_hip import lib, ops
    L = lib()
    n, hf, wf, hn, wn = 2, 33, 47, 16, 20
    f, x, w = C.frames(n, hf, wf), C.logits(n, hn, wn), C.windows_array(windows)
    ft, xt, wt = torch.from_numpy(f), torch.from_numpy(x), torch.from_numpy(w)
    rep = I.Report("windows " + str(windows))
    for mirror in (0, 1):
        want = np.concatenate([W.prepare_frame_window(f[k], w[k], hn, wn, bool(mirror)) for k in range(n)])
        ops_ = [I.inp("frames", ft), I.inp("windows", wt, is_map=False), I.out("image", (n, 3, hn, wn), torch.float32)]
        for off in (0, 4):
            ops_[2] = I.out("image", (n, 3, hn, wn), torch.float32, offset=off)

            def call(isl):
                assert L.fosvos_frame_prep_window(isl.ptr("frames"), isl.ptr("windows"), n, hf, wf, hn, wn, mirror,
                                                  ops._mean_bgr(), isl.ptr("image"), 0, _st()) == 0
            rep.add(I.run_case("prep mirror %d offset %d" % (mirror, off), ops_, call, {"image": torch.from_numpy(want)}, device=DEV))
        for mode in range(4):
            boolean, overlay = mode in (0, 2), mode < 2
            if overlay:
                want = np.stack([W.overlay_window(f[k], x[k, 0], w[k], bool(mirror), boolean, "g", 0.5) for k in range(n)])
            else:
                want = np.stack([W.mask_bytes_window(x[k, 0], w[k], hf, wf, boolean) for k in range(n)])
            shape = (n, hf, wf, 3) if overlay else (n, hf, wf)
            ops_ = [I.inp("frames", ft), I.inp("logits", xt), I.inp("windows", wt, is_map=False),
                    I.out("out", shape, torch.uint8, is_map=False, offset=1)]

            def call(isl):
                assert L.fosvos_overlay_window(isl.ptr("frames"), isl.ptr("logits"), isl.ptr("windows"), n, hf, wf, hn, wn, mirror,
                                               mode, 1, 0.5, isl.ptr("out"), 0, _st()) == 0
            # a soft byte may differ from the host's by one within the band: the three runs must agree with each other
            expected = {"out": torch.from_numpy(want)} if boolean else None
            rep.add(I.run_case("overlay mirror %d mode %d" % (mirror, mode), ops_, call, expected, device=DEV))
    need = int(L.fosvos_window_next_workspace_bytes(n))
    assert need == n * 5 * 4
    want = np.array([W.next_window(x[k, 0], w[k], hf, wf, 4, 250, 2) for k in range(n)], dtype=np.int32)
    ops_ = [I.inp("logits", xt), I.inp("windows", wt, is_map=False), I.out("next", (n, 4), torch.int32), I.workspace("workspace", need)]

    def call(isl):
        assert L.fosvos_window_next(isl.ptr("logits"), isl.ptr("windows"), n, hf, wf, hn, wn, 4, 250, 2, isl.ptr("next"),
                                    isl.ptr("workspace"), need, 0, _st()) == 0
    rep.add(I.run_case("window_next", ops_, call, {"next": torch.from_numpy(want)}, device=DEV))
    ops_ = [I.inp("logits", xt), I.inout("windows", wt, is_map=False), I.workspace("workspace", need)]

    def call(isl):
        assert L.fosvos_window_next(isl.ptr("logits"), isl.ptr("windows"), n, hf, wf, hn, wn, 4, 250, 2, isl.ptr("windows"),
                                    isl.ptr("workspace"), need, 0, _st()) == 0
    rep.add(I.run_case("window_next in place", ops_, call, {"windows": torch.from_numpy(want)}, device=DEV))
    rep.done()


# ------------------------------------------------------------------------------------------ arguments
def test_window_bad_arguments_raise_and_launch_nothing():
    from fosvos_hip import LaunchProfile, lib, ops
    n, hf, wf, hn, wn = 2, 33, 47, 16, 20
    size = (hn, wn)
    f = torch.from_numpy(C.frames(n, hf, wf)).to(DEV)
    x = torch.from_numpy(C.logits(n, hn, wn)).to(DEV)
    w = torch.from_numpy(C.windows_array([(3, 5, 21, 31), (0, 0, 33, 47)])).to(DEV)
    out = torch.full((n, hf, wf, 3), 7, dtype=torch.uint8, device=DEV)
    img = torch.full((n, 3, hn, wn), 7.0, device=DEV)
    nxt = torch.full((n, 4), 7, dtype=torch.int32, device=DEV)
    L = lib()
    st = _st()
    mean = ops._mean_bgr()
    ws = torch.empty(64, dtype=torch.uint8, device=DEV)
    with LaunchProfile(0) as prof:
        for bad in (lambda: ops.frame_prep_window(f, w, None), lambda: ops.frame_prep_window(f, w, (hf + 1, wn)),
                    lambda: ops.frame_prep_window(f, w, (hn, wf + 1)), lambda: ops.frame_prep_window(f, w, (0, wn)),
                    lambda: ops.frame_prep_window(f, w, (hn,)), lambda: ops.frame_prep_window(f, w, (16.0, 20)),
                    lambda: ops.frame_prep_window(f, w, (True, 20)),
                    lambda: ops.frame_prep_window(f, w[:1], size), lambda: ops.frame_prep_window(f, w.long(), size),
                    lambda: ops.frame_prep_window(f, w.reshape(-1), size), lambda: ops.frame_prep_window(f, w.t().contiguous().t(), size),
                    lambda: ops.frame_prep_window(f, w, size, out=img[:, :, :, :19]),
                    lambda: ops.frame_prep_window(f, w, size, out=img.double()), lambda: ops.frame_prep_window(f[:0], w[:0], size),
                    lambda: ops.overlay_window(f, x[:1], w), lambda: ops.overlay_window(f, x[:, 0], w),
                    lambda: ops.overlay_window(f, x.double(), w), lambda: ops.overlay_window(f, x, w[:1]),
                    lambda: ops.overlay_window(f, x, w.float()),
                    lambda: ops.overlay_window(f, torch.zeros((n, 1, hf + 1, wf), device=DEV), w),
                    lambda: ops.overlay_window(f, x, w, alpha=-0.5), lambda: ops.overlay_window(f, x, w, alpha=float("nan")),
                    lambda: ops.overlay_window(f, x, w, color="x"), lambda: ops.overlay_window(f, x, w, out=out[:, :, :, :2]),
                    lambda: ops.overlay_window(f, x, w, overlay=False, out=out),
                    lambda: ops.window_next(x, w, (hn - 1, wf)), lambda: ops.window_next(x, w, (hf, wn - 1)),
                    lambda: ops.window_next(x, w, (hf,)), lambda: ops.window_next(x, w, (hf, 47.0)), lambda: ops.window_next(x, w, (8193, wf)),
                    lambda: ops.window_next(x, w, (hf, wf), levels=0), lambda: ops.window_next(x, w, (hf, wf), levels=65),
                    lambda: ops.window_next(x, w, (hf, wf), levels=2.0), lambda: ops.window_next(x, w, (hf, wf), margin=-0.1),
                    lambda: ops.window_next(x, w, (hf, wf), margin=4.01), lambda: ops.window_next(x, w, (hf, wf), margin=float("nan")),
                    lambda: ops.window_next(x, w, (hf, wf), margin=float("inf")), lambda: ops.window_next(x, w, (hf, wf), margin="1"),
                    lambda: ops.window_next(x, w, (hf, wf), min_pad=-1), lambda: ops.window_next(x, w, (hf, wf), min_pad=4096),
                    lambda: ops.window_next(x, w, (hf, wf), min_pad=1.0), lambda: ops.window_next(x, w[:1], (hf, wf)),
                    lambda: ops.window_next(x[:, 0], w, (hf, wf)), lambda: ops.window_next(x.double(), w, (hf, wf)),
                    lambda: ops.window_next(x, w, (hf, wf), out=nxt[:1]), lambda: ops.window_next(x, w, (hf, wf), out=nxt.long())):
            with pytest.raises(ValueError):
                bad()
        for bad in (lambda: ops.frame_prep_window(f.cpu(), w, size), lambda: ops.frame_prep_window(f, w.cpu(), size),
                    lambda: ops.overlay_window(f, x.cpu(), w), lambda: ops.overlay_window(f, x, w.cpu()),
                    lambda: ops.overlay_window(f, x, w, out=out.cpu()), lambda: ops.window_next(x.cpu(), w, (hf, wf)),
                    lambda: ops.window_next(x, w.cpu(), (hf, wf)), lambda: ops.window_next(x, w, (hf, wf), out=nxt.cpu())):
            with pytest.raises(RuntimeError):
                bad()

        # straight through the C ABI: the library's error codes, never a fault
        def fp(fr=f.data_ptr(), wi=w.data_ptr(), n_=n, hf_=hf, wf_=wf, hn_=hn, wn_=wn, m=mean, im=img.data_ptr()):
            return L.fosvos_frame_prep_window(fr, wi, n_, hf_, wf_, hn_, wn_, 0, m, im, 0, st)

        def ov(fr=f.data_ptr(), lg=x.data_ptr(), wi=w.data_ptr(), n_=n, hf_=hf, wf_=wf, hn_=hn, wn_=wn, mode=0, ch=2, alpha=1.0,
               o=out.data_ptr()):
            return L.fosvos_overlay_window(fr, lg, wi, n_, hf_, wf_, hn_, wn_, 1, mode, ch, alpha, o, 0, st)

        def nx(lg=x.data_ptr(), wi=w.data_ptr(), n_=n, hf_=hf, wf_=wf, hn_=hn, wn_=wn, lv=8, pm=250, pad=16, o=nxt.data_ptr(),
               wp=ws.data_ptr(), wb=64):
            return L.fosvos_window_next(lg, wi, n_, hf_, wf_, hn_, wn_, lv, pm, pad, o, wp, wb, 0, st)

        assert fp(fr=None) == -2 and fp(wi=None) == -2 and fp(m=None) == -2 and fp(im=None) == -2
        assert fp(wi=w.data_ptr() + 2) == -2 and b"windows" in L.fosvos_last_error()
        assert fp(im=img.data_ptr() + 2) == -2
        assert fp(n_=0) == -1 and fp(hf_=0) == -1 and fp(wn_=-2) == -1 and fp(hn_=hf + 1) == -1 and fp(wf_=8193) == -1
        assert ov(ch=3) == -2 and ov(mode=4) == -2 and ov(mode=-1) == -2 and ov(alpha=-1.0) == -2 and ov(alpha=float("nan")) == -2
        assert ov(fr=None) == -2 and ov(lg=None) == -2 and ov(wi=None) == -2 and ov(o=None) == -2
        assert ov(wi=w.data_ptr() + 1) == -2 and ov(lg=x.data_ptr() + 2) == -2
        assert ov(n_=0) == -1 and ov(hn_=0) == -1 and ov(wn_=wf + 1) == -1 and ov(hf_=8193) == -1
        assert nx(lg=None) == -2 and nx(wi=None) == -2 and nx(o=None) == -2 and nx(wp=None) == -2
        assert nx(lv=0) == -2 and nx(lv=65) == -2 and nx(pm=-1) == -2 and nx(pm=4001) == -2 and nx(pad=-1) == -2 and nx(pad=4096) == -2
        assert nx(wb=n * 20 - 1) == -2 and b"workspace" in L.fosvos_last_error()
        assert nx(o=nxt.data_ptr() + 2) == -2 and nx(wp=ws.data_ptr() + 2) == -2 and nx(lg=x.data_ptr() + 2) == -2
        assert nx(n_=0) == -1 and nx(hn_=hf + 1) == -1 and nx(wn_=0) == -1 and nx(hf_=8193) == -1
        assert L.fosvos_window_next_workspace_bytes(0) == 0 and L.fosvos_window_next_workspace_bytes(-3) == 0
    assert not prof.records, prof.records
    torch.cuda.synchronize()
    assert (out == 7).all() and (img == 7.0).all() and (nxt == 7).all()  # none of the refused calls wrote anything
    with LaunchProfile(0) as prof:
        ops.frame_prep_window(f, w, size, True, out=img)
        ops.overlay_window(f, x, w, True, out=out)
        ops.window_next(x, w, (hf, wf), out=nxt)
        assert ov(fr=None, mode=2, o=out.data_ptr()) == 0  # the mask modes do not read the frames
        full = torch.empty((n, 3, hf, wf), device=DEV)
        assert fp(hn_=hf, wn_=wf, im=full.data_ptr()) == 0  # equal sizes are in range: a ladder of one size
        ops.frame_prep_window(f, w, (hf, wf))
    assert prof.records["k_frame_prep_window"]["launches"] == 3 and prof.records["k_overlay_window"]["launches"] == 2
    assert prof.records["k_window_reset"]["launches"] == 1 and prof.records["k_window_next"]["launches"] == 1
    assert set(prof.records) == {"k_frame_prep_window", "k_overlay_window", "k_window_reset", "k_window_next"}


# ------------------------------------------------------------------------------------------ FrameSegmenter
class RedThreshold(torch.nn.Module):
    """The stand-in net: the red channel of the prepared image less a constant, one float32 subtraction
    (frame_roi_cases.threshold_net_fn is the same in numpy)."""

    def __init__(self):
        super().__init__()
        self.offset = torch.nn.Parameter(torch.tensor(C.red_offset(), dtype=torch.float32), requires_grad=False)

    def forward(self, x):
        return [x[:, 2:3] - self.offset]


HF, WF, SIZE = 96, 172, (48, 86)


def clean_largest(x):
    return M.clean_logits(x, M.keep_components(M.logits_mask(x), largest=True))


def run_segmenter(frames, **kw):
    from fosvos_hip.options import RoiOptions
    from fosvos_hip.stream import FrameSegmenter
    net = RedThreshold().to(DEV).eval()
    seed = kw.pop("seed_mask", None)
    with FrameSegmenter(net, HF, WF, net_size=SIZE, roi=RoiOptions(levels=4, min_pad=4), **kw) as seg:
        if seed is not None:
            seg.seed_window(seed)
        outs = list(seg.segment(frames))
        return outs, seg.last_window()


def test_segmenter_with_roi_is_track():
    small = C.drifting_frames(12, HF, WF)                                  # settles on the net's own size, 1:1
    large = C.drifting_frames(12, HF, WF, top=25, left=50, h=30, w=50)     # settles on a level in between
    for frames, kw in ((small, dict()), (large, dict()), (large, dict(mirror=False, color="g", alpha=0.5)),
                       (small, dict(overlay=False))):
        want, used, last = W.track(frames, C.threshold_net_fn, SIZE[0], SIZE[1], mirror=kw.get("mirror", True),
                                   overlay_on=kw.get("overlay", True), color=kw.get("color", "r"), alpha=kw.get("alpha", 1.0),
                                   levels=4, margin_permille=250, min_pad=4)
        assert used[0] == (0, 0, HF, WF) and used[-1][2:] != (HF, WF) and len(set(used)) >= 4  # it zooms in and it moves
        assert (used[-1][2:] == SIZE) == (frames is small)
        one, last1 = run_segmenter(frames, depth=1, **kw)
        two, last2 = run_segmenter(frames, depth=2, **kw)
        assert len(one) == len(two) == 12
        for k in range(12):
            assert one[k].tobytes() == two[k].tobytes(), (kw, k)
            assert one[k].shape == want[k].shape and one[k].tobytes() == want[k].tobytes(), (kw, k, used[k])
        assert last1 == last2 == last, (kw, last1, last2, last)


def test_segmenter_with_roi_seeded_and_cleaned():
    from fosvos_hip.options import CleanOptions
    frames = C.drifting_frames(12, HF, WF, distractor=(70, 8, 9, 11))
    # the annotation of the first frame, in the frame's own coordinates; the reference sees the mirrored picture
    mask = np.zeros((HF, WF), dtype=np.uint8)
    mask[20:42, 30:64] = 1
    start = W.window_of_mask(mask[:, ::-1], SIZE[0], SIZE[1], 4, 250, 4)
    assert start[2:] != (HF, WF)
    want, used, last = W.track(frames, C.threshold_net_fn, SIZE[0], SIZE[1], mirror=True, levels=4, margin_permille=250, min_pad=4,
                               window=start, clean_fn=clean_largest)
    plain, used_plain, _ = W.track(frames, C.threshold_net_fn, SIZE[0], SIZE[1], mirror=True, levels=4, margin_permille=250,
                                   min_pad=4)
    assert used != used_plain  # the seed and the cleaning both matter here
    for depth in (1, 2):
        got, last_got = run_segmenter(frames, depth=depth, clean=CleanOptions(largest=True), seed_mask=mask)
        for k in range(12):
            assert got[k].tobytes() == want[k].tobytes(), (depth, k, used[k])
        assert last_got == last


def test_segmenter_with_roi_jpeg_is_the_same_picture():
    from fosvos_hip import ops
    frames = C.drifting_frames(5, HF, WF)
    want, _, _ = W.track(frames, C.threshold_net_fn, SIZE[0], SIZE[1], mirror=True, levels=4, margin_permille=250, min_pad=4)
    buf, lengths = ops.jpeg_encode(torch.from_numpy(np.ascontiguousarray(np.stack(want))).to(DEV), 90)
    files = [buf[k, :int(lengths[k])].cpu().numpy().tobytes() for k in range(5)]
    got, _ = run_segmenter(frames, depth=2, encode="jpeg", quality=90)
    assert [isinstance(g, bytes) for g in got] == [True] * 5 and got == files


def test_segmenter_refuses_what_roi_does_not_go_with():
    from fosvos_hip.options import CleanOptions, RoiOptions
    from fosvos_hip.stream import FrameSegmenter, ObjectSegmenter
    net = RedThreshold().to(DEV).eval()
    with pytest.raises(ValueError, match="net_size"):
        FrameSegmenter(net, HF, WF, roi=RoiOptions())
    with pytest.raises(ValueError, match="temporal_radius"):
        FrameSegmenter(net, HF, WF, net_size=SIZE, roi=RoiOptions(), clean=CleanOptions(temporal_radius=3))
    with pytest.raises(ValueError, match="RoiOptions"):
        FrameSegmenter(net, HF, WF, net_size=SIZE, roi=dict(levels=4))
    with pytest.raises(ValueError, match="not built"):
        ObjectSegmenter([net], HF, WF, net_size=SIZE, roi=RoiOptions())
    with FrameSegmenter(net, HF, WF, net_size=SIZE) as seg:  # no roi: nothing to seed, nothing to report
        assert seg.roi is None and seg._window is None
        with pytest.raises(RuntimeError):
            seg.seed_window(np.zeros((HF, WF), dtype=np.uint8))
        with pytest.raises(RuntimeError):
            seg.last_window()
    with FrameSegmenter(net, HF, WF, net_size=SIZE, roi=RoiOptions()) as seg:
        assert seg.last_window() == (0, 0, HF, WF)
        for bad in (np.zeros((HF, WF), dtype=np.float32), np.zeros(SIZE, dtype=np.uint8), np.zeros((HF, WF, 1), dtype=np.uint8)):
            with pytest.raises(ValueError):
                seg.seed_window(bad)
        seg.seed_window(np.zeros((HF, WF), dtype=bool))  # an empty annotation: the whole frame
        assert seg.last_window() == (0, 0, HF, WF)
    assert seg._window is None  # closed: the tensors are dropped
    with FrameSegmenter(net, HF, WF, net_size=(HF, WF), roi=RoiOptions()) as seg:  # the frame's own size: a ladder of one size
        frame = C.drifting_frames(1, HF, WF)[0]
        want, _, _ = W.track([frame], C.threshold_net_fn, HF, WF, mirror=True)
        assert seg.apply(frame).tobytes() == want[0].tobytes() and seg.last_window() == (0, 0, HF, WF)


def test_a_segmenter_without_roi_launches_what_it_launched():
    from fosvos_hip import LaunchProfile
    from fosvos_hip.options import CleanOptions, RoiOptions
    from fosvos_hip.stream import FrameSegmenter
    net = RedThreshold().to(DEV).eval()
    frames = C.drifting_frames(3, HF, WF)

    def launched(**kw):
        with FrameSegmenter(net, HF, WF, **kw) as seg:
            with LaunchProfile(0) as prof:
                outs = [seg.apply(f) for f in frames]
        return {k: v["launches"] for k, v in prof.records.items()}, outs

    names, _ = launched(net_size=SIZE)
    assert names == {"k_frame_prep_scaled": 3, "k_overlay_scaled": 3}
    names, _ = launched()
    assert names == {"k_frame_prep": 3, "k_overlay": 3}
    cleaned, _ = launched(net_size=SIZE, clean=CleanOptions(largest=True))
    assert cleaned["k_frame_prep_scaled"] == 3 and cleaned["k_overlay_scaled"] == 3
    assert not [k for k in cleaned if "window" in k]
    with_roi, _ = launched(net_size=SIZE, roi=RoiOptions())
    assert with_roi == {"k_frame_prep_window": 3, "k_window_reset": 3, "k_window_next": 3, "k_overlay_window": 3}
    both, _ = launched(net_size=SIZE, roi=RoiOptions(), clean=CleanOptions(largest=True))
    extra = {k: v for k, v in both.items() if k not in cleaned}
    assert extra == with_roi and {k: v for k, v in both.items() if k in cleaned and "scaled" not in k} == \
        {k: v for k, v in cleaned.items() if "scaled" not in k}
