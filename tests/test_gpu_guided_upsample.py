"""Edge-aware upsampling on a real MI355X: ``ops.guided_coefficients`` (csrc/guided.hip: k_guided_fit + k_guided_smooth) and
``ops.overlay_guided`` (csrc/stream.hip: k_overlay_guided) against the numpy statement of the arithmetic
(util/guided_upsample.py) - exact equality for the coefficient maps and the boolean modes, everywhere but within 1e-9 of a
rounding boundary for the soft modes; both entries on islands; ``FrameSegmenter(refine=)`` end to end against ``apply_guided``."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fosvos_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import frame_roi_cases as RC  # noqa: E402
import guided_cases as C  # noqa: E402
import islands as I  # noqa: E402
from util import frame_overlay as F  # noqa: E402
from util import frame_resample as R  # noqa: E402
from util import guided_upsample as G  # noqa: E402
from util import jpeg_layout  # noqa: E402
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


def host(a):
    return torch.from_numpy(np.array(a))   # a copy: the shared references are read-only


def dev(a):
    return host(a).to(DEV)


# ------------------------------------------------------------------------------------------ guided_coefficients
@pytest.mark.parametrize("eps", C.EPS)
@pytest.mark.parametrize("kind", C.KINDS)
@pytest.mark.parametrize("case", C.CASES, ids=C.IDS)
def test_coefficients_are_the_definition_bit_for_bit(case, kind, eps):
    from fosvos_hip import ops
    n, hf, wf, hn, wn, r = case
    _, im, x, want = C.reference(case, kind, eps)
    imd, xd = dev(im), dev(x)
    out = garbage((n, 2, hn, wn), torch.float64)
    assert ops.guided_coefficients(imd, xd, r, eps, C.CLIP, out=out) is out
    got = out.cpu().numpy()
    assert got.tobytes() == want.tobytes(), (case, kind, eps, int((got != want).sum()), float(np.nanmax(np.abs(got - want))))
    again = ops.guided_coefficients(imd, xd, r, eps, C.CLIP)
    assert again.dtype == torch.float64 and again.shape == (n, 2, hn, wn) and again.cpu().numpy().tobytes() == want.tobytes()
    # base pointers off by one element: the image and the logits by one float, the maps by one double
    out2 = offset_view(garbage((n, 2, hn, wn), torch.float64))
    ops.guided_coefficients(offset_view(imd), offset_view(xd), r, eps, C.CLIP, out=out2)
    assert out2.cpu().numpy().tobytes() == want.tobytes(), (case, kind, eps, "offset")
    if n > 1:   # frames do not see each other
        for k in range(n):
            one = ops.guided_coefficients(imd[k:k + 1].contiguous(), xd[k:k + 1].contiguous(), r, eps, C.CLIP)
            assert one.cpu().numpy().tobytes() == want[k:k + 1].tobytes(), (case, kind, eps, k)


def test_coefficients_launch_twice_and_take_the_options_defaults():
    from fosvos_hip import LaunchProfile, ops
    from fosvos_hip.options import RefineOptions
    case = C.CASES[1]
    n, hf, wf, hn, wn, _ = case
    f, x = C.frames(n, hf, wf), C.logits(n, hn, wn)
    im = C.images(f, hn, wn)
    o = RefineOptions()
    want = np.stack([G.coefficients(im[k], x[k, 0], o.radius, o.eps, o.clip) for k in range(n)])
    with LaunchProfile(0) as prof:
        got = ops.guided_coefficients(dev(im), dev(x))
    assert got.cpu().numpy().tobytes() == want.tobytes()
    assert {k: v["launches"] for k, v in prof.records.items()} == {"k_guided_fit": 1, "k_guided_smooth": 1}


# ------------------------------------------------------------------------------------------ overlay_guided, boolean
@pytest.mark.parametrize("kind", C.KINDS)
@pytest.mark.parametrize("case", C.CASES, ids=C.IDS)
def test_boolean_overlay_guided_is_exact(case, kind):
    from fosvos_hip import ops
    n, hf, wf, hn, wn, r = case
    for mirror in (False, True):
        f, _, _, coeff = C.reference(case, kind, 400.0, mirror)
        fd, cd = dev(f), dev(coeff)
        src = f[:, :, ::-1] if mirror else f
        for color, alpha in (("b", 0.5), ("r", 1.0), ("g", 0.0), ("g", 2.0)):
            c = F.COLOR_CHANNEL[color]
            want = np.stack([G.overlay_guided(f[k], coeff[k], mirror, True, color, alpha) for k in range(n)])
            out = garbage((n, hf, wf, 3), torch.uint8)
            assert ops.overlay_guided(fd, cd, mirror, True, color, alpha, out=out) is out
            got = out.cpu().numpy()
            assert np.array_equal(got, want), (case, kind, mirror, color, alpha, int((got != want).sum()))
            others = [k for k in range(3) if k != c]
            assert np.array_equal(got[..., others], src[..., others])  # untouched channels: the (mirrored) input
        want = np.stack([G.mask_bytes_guided(f[k], coeff[k], mirror, True) for k in range(n)])
        out = garbage((n, hf, wf), torch.uint8)
        assert ops.overlay_guided(fd, cd, mirror, True, overlay=False, out=out) is out
        assert np.array_equal(out.cpu().numpy(), want), (case, kind, mirror, "mask")
        assert set(np.unique(want).tolist()) <= {0, 255}
        # base pointers off by one element
        out = offset_view(garbage((n, hf, wf, 3), torch.uint8))
        ops.overlay_guided(offset_view(fd), offset_view(cd), mirror, True, "g", 0.5, out=out)
        want = np.stack([G.overlay_guided(f[k], coeff[k], mirror, True, "g", 0.5) for k in range(n)])
        assert np.array_equal(out.cpu().numpy(), want), (case, kind, mirror, "offset")
        out = offset_view(garbage((n, hf, wf), torch.uint8))
        ops.overlay_guided(offset_view(fd), offset_view(cd), mirror, True, overlay=False, out=out)
        assert np.array_equal(out.cpu().numpy(), np.stack([G.mask_bytes_guided(f[k], coeff[k], mirror, True) for k in range(n)]))


def test_the_mirrored_mask_is_the_mask_of_the_flipped_frame():
    from fosvos_hip import ops
    case = C.CASES[1]
    n, hf, wf, hn, wn, r = case
    f, _, _, coeff = C.reference(case, "random", 400.0, True)
    flipped = np.ascontiguousarray(f[:, :, ::-1])
    a = ops.overlay_guided(dev(f), dev(coeff), True, True, overlay=False)
    b = ops.overlay_guided(dev(flipped), dev(coeff), False, True, overlay=False)
    c = ops.overlay_guided(dev(f), dev(coeff), False, True, overlay=False)
    assert torch.equal(a, b) and not torch.equal(a, c)   # the frame is read, mirrored, in the mask modes too


# ------------------------------------------------------------------------------------------ overlay_guided, soft
def test_soft_overlay_guided_outside_the_rounding_band():
    """Every case in one test: the band's share is taken over all of them, as the scaled overlay's test does."""
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

    for case in C.CASES:
        n, hf, wf, hn, wn, r = case
        for mirror in (False, True):
            f, _, _, coeff = C.reference(case, "random", 400.0, mirror)
            fd, cd = dev(f), dev(coeff)
            for color in ("b", "r"):
                c = F.COLOR_CHANNEL[color]
                for alpha in C.SOFT_ALPHAS:
                    want = np.stack([G.overlay_guided(f[k], coeff[k], mirror, False, color, alpha) for k in range(n)])
                    band = np.stack([C.soft_band_guided(f[k], coeff[k], mirror, True, color, alpha) for k in range(n)])
                    out = garbage((n, hf, wf, 3), torch.uint8)
                    got = ops.overlay_guided(fd, cd, mirror, False, color, alpha, out=out).cpu().numpy()
                    others = [k for k in range(3) if k != c]
                    assert np.array_equal(got[..., others], want[..., others])
                    compare(got[..., c], want[..., c], band, (case, mirror, color, alpha))
            # alpha 0 adds an exact zero: no exclusion
            got = ops.overlay_guided(fd, cd, mirror, False, "r", 0.0).cpu().numpy()
            assert np.array_equal(got, f[:, :, ::-1] if mirror else f)
            want = np.stack([G.mask_bytes_guided(f[k], coeff[k], mirror, False) for k in range(n)])
            band = np.stack([C.soft_band_guided(f[k], coeff[k], mirror, False, "r", 1.0) for k in range(n)])
            out = offset_view(garbage((n, hf, wf), torch.uint8))
            got = ops.overlay_guided(offset_view(fd), offset_view(cd), mirror, False, overlay=False, out=out).cpu().numpy()
            compare(got, want, band, (case, mirror, "mask"))
    print("band pixels", n_band, "of", n_all)
    assert n_band <= C.BAND_SHARE * n_all, (n_band, n_all)


# ------------------------------------------------------------------------------------------ islands
def _st():
    return torch.cuda.current_stream().cuda_stream


def test_guided_entries_on_islands():
    """Both entries on operands between poisoned margins: nothing outside the operands is read or written, the workspace
    included, and nothing depends on what the workspace or the output held."""
    from fosvos_hip import lib, ops
    L = lib()
    case = C.CASES[1]
    n, hf, wf, hn, wn, r = case
    rep = I.Report("guided " + str(case))
    need = int(L.fosvos_guided_coefficients_workspace_bytes(n, hn, wn))
    assert need == n * 2 * hn * wn * 8
    for kind, eps in (("random", 400.0), ("step", 1e-3)):
        f, im, x, coeff = C.reference(case, kind, eps)
        for off in (0, 8):
            ops_ = [I.inp("image", host(im)), I.inp("logits", host(x)),
                    I.out("coeff", (n, 2, hn, wn), torch.float64, offset=off), I.workspace("workspace", need)]

            def call(isl):
                assert L.fosvos_guided_coefficients(isl.ptr("image"), isl.ptr("logits"), n, hn, wn, r, eps, C.CLIP, isl.ptr("coeff"),
                                                    isl.ptr("workspace"), need, 0, _st()) == 0
            rep.add(I.run_case("coefficients %s offset %d" % (kind, off), ops_, call, {"coeff": host(coeff)}, device=DEV))
    for mirror in (0, 1):
        f, _, _, coeff = C.reference(case, "random", 400.0, bool(mirror))
        for mode in range(4):
            boolean, overlay = mode in (0, 2), mode < 2
            if overlay:
                want = np.stack([G.overlay_guided(f[k], coeff[k], bool(mirror), boolean, "g", 0.5) for k in range(n)])
            else:
                want = np.stack([G.mask_bytes_guided(f[k], coeff[k], bool(mirror), boolean) for k in range(n)])
            shape = (n, hf, wf, 3) if overlay else (n, hf, wf)
            ops_ = [I.inp("frames", host(f)), I.inp("coeff", host(coeff)),
                    I.out("out", shape, torch.uint8, is_map=False, offset=1)]

            def call(isl):
                assert L.fosvos_overlay_guided(isl.ptr("frames"), isl.ptr("coeff"), n, hf, wf, hn, wn, mirror, mode, 1, 0.5,
                                               ops._mean_bgr(), isl.ptr("out"), 0, _st()) == 0
            # a soft byte may differ from the host's by one within the band: the three runs must agree with each other
            expected = {"out": host(want)} if boolean else None
            rep.add(I.run_case("overlay mirror %d mode %d" % (mirror, mode), ops_, call, expected, device=DEV))
    rep.done()


# ------------------------------------------------------------------------------------------ arguments
def test_guided_bad_arguments_raise_and_launch_nothing():
    from fosvos_hip import LaunchProfile, lib, ops
    n, hf, wf, hn, wn = 2, 33, 47, 16, 20
    f = dev(C.frames(n, hf, wf))
    im = dev(C.images(C.frames(n, hf, wf), hn, wn))
    x = dev(C.logits(n, hn, wn))
    co = torch.full((n, 2, hn, wn), 7.0, dtype=torch.float64, device=DEV)
    out = torch.full((n, hf, wf, 3), 7, dtype=torch.uint8, device=DEV)
    L, st, mean = lib(), _st(), ops._mean_bgr()
    ws = torch.empty(n * 2 * hn * wn * 8, dtype=torch.uint8, device=DEV)
    with LaunchProfile(0) as prof:
        for bad in (lambda: ops.guided_coefficients(im, x, radius=0), lambda: ops.guided_coefficients(im, x, radius=9),
                    lambda: ops.guided_coefficients(im, x, radius=2.0), lambda: ops.guided_coefficients(im, x, radius=True),
                    lambda: ops.guided_coefficients(im, x, eps=1e-4), lambda: ops.guided_coefficients(im, x, eps=2e9),
                    lambda: ops.guided_coefficients(im, x, eps=float("nan")), lambda: ops.guided_coefficients(im, x, eps="1"),
                    lambda: ops.guided_coefficients(im, x, clip=0.0), lambda: ops.guided_coefficients(im, x, clip=2e4),
                    lambda: ops.guided_coefficients(im, x, clip=float("inf")),
                    lambda: ops.guided_coefficients(im[:, :2], x), lambda: ops.guided_coefficients(im.double(), x),
                    lambda: ops.guided_coefficients(im, x[:1]), lambda: ops.guided_coefficients(im, x[:, 0]),
                    lambda: ops.guided_coefficients(im, x.double()), lambda: ops.guided_coefficients(im[:0], x[:0]),
                    lambda: ops.guided_coefficients(im, x, out=co.float()), lambda: ops.guided_coefficients(im, x, out=co[:1]),
                    lambda: ops.guided_coefficients(im.permute(0, 1, 3, 2), x),
                    lambda: ops.overlay_guided(f, co[:1]), lambda: ops.overlay_guided(f, co[:, :1]), lambda: ops.overlay_guided(f, co.float()),
                    lambda: ops.overlay_guided(f, torch.zeros((n, 2, hf + 1, wf), dtype=torch.float64, device=DEV)),
                    lambda: ops.overlay_guided(f, torch.zeros((n, 2, hf, wf + 1), dtype=torch.float64, device=DEV)),
                    lambda: ops.overlay_guided(f, co, alpha=-0.5), lambda: ops.overlay_guided(f, co, alpha=float("nan")),
                    lambda: ops.overlay_guided(f, co, color="x"), lambda: ops.overlay_guided(f, co, out=out[:, :, :, :2]),
                    lambda: ops.overlay_guided(f, co, overlay=False, out=out), lambda: ops.overlay_guided(f[..., :2], co)):
            with pytest.raises(ValueError):
                bad()
        for bad in (lambda: ops.guided_coefficients(im.cpu(), x), lambda: ops.guided_coefficients(im, x.cpu()),
                    lambda: ops.guided_coefficients(im, x, out=co.cpu()), lambda: ops.overlay_guided(f.cpu(), co),
                    lambda: ops.overlay_guided(f, co.cpu()), lambda: ops.overlay_guided(f, co, out=out.cpu())):
            with pytest.raises(RuntimeError):
                bad()

        # straight through the C ABI: the library's error codes, never a fault
        def gc(i=im.data_ptr(), lg=x.data_ptr(), n_=n, hn_=hn, wn_=wn, r=4, eps=400.0, clip=6.0, o=co.data_ptr(), wp=ws.data_ptr(),
               wb=ws.numel()):
            return L.fosvos_guided_coefficients(i, lg, n_, hn_, wn_, r, eps, clip, o, wp, wb, 0, st)

        def ov(fr=f.data_ptr(), c=co.data_ptr(), n_=n, hf_=hf, wf_=wf, hn_=hn, wn_=wn, mode=0, ch=2, alpha=1.0, m=mean, o=out.data_ptr()):
            return L.fosvos_overlay_guided(fr, c, n_, hf_, wf_, hn_, wn_, 1, mode, ch, alpha, m, o, 0, st)

        assert gc(i=None) == -2 and gc(lg=None) == -2 and gc(o=None) == -2 and gc(wp=None) == -2
        assert gc(r=0) == -2 and gc(r=9) == -2 and gc(eps=9e-4) == -2 and gc(eps=float("nan")) == -2 and gc(eps=1.1e9) == -2
        assert gc(clip=0.0) == -2 and gc(clip=float("nan")) == -2 and gc(clip=1.1e4) == -2
        assert gc(i=im.data_ptr() + 2) == -2 and gc(lg=x.data_ptr() + 1) == -2
        assert gc(o=co.data_ptr() + 4) == -2 and gc(wp=ws.data_ptr() + 4) == -2
        assert gc(wb=ws.numel() - 1) == -2 and b"workspace" in L.fosvos_last_error()
        assert gc(n_=0) == -1 and gc(hn_=0) == -1 and gc(wn_=-1) == -1 and gc(hn_=8193) == -1
        assert ov(fr=None) == -2 and ov(c=None) == -2 and ov(m=None) == -2 and ov(o=None) == -2
        assert ov(fr=None, mode=2) == -2   # the mask modes read the frames too
        assert ov(mode=4) == -2 and ov(mode=-1) == -2 and ov(ch=3) == -2 and ov(alpha=-1.0) == -2 and ov(alpha=float("nan")) == -2
        assert ov(c=co.data_ptr() + 4) == -2
        assert ov(n_=0) == -1 and ov(hn_=0) == -1 and ov(hn_=hf + 1) == -1 and ov(wn_=wf + 1) == -1 and ov(hf_=8193) == -1
        assert L.fosvos_guided_coefficients_workspace_bytes(0, 4, 4) == 0 and L.fosvos_guided_coefficients_workspace_bytes(1, 8193, 4) == 0
    assert not prof.records, prof.records
    torch.cuda.synchronize()
    assert (out == 7).all() and (co == 7.0).all()   # none of the refused calls wrote anything
    with LaunchProfile(0) as prof:
        ops.guided_coefficients(im, x, out=co)
        ops.overlay_guided(f, co, True, out=out)
    assert {k: v["launches"] for k, v in prof.records.items()} == {"k_guided_fit": 1, "k_guided_smooth": 1, "k_overlay_guided": 1}


# ------------------------------------------------------------------------------------------ FrameSegmenter
class RedThreshold(torch.nn.Module):
    """The stand-in net: the red channel of the prepared image less a constant, one float32 subtraction."""

    def __init__(self):
        super().__init__()
        self.offset = torch.nn.Parameter(torch.tensor(RC.red_offset(), dtype=torch.float32), requires_grad=False)

    def forward(self, x):
        return [x[:, 2:3] - self.offset]


HF, WF, SIZE = 96, 172, (48, 86)   # the sizes of the window test's end-to-end case


def clean_largest(x):
    return M.clean_logits(x, M.keep_components(M.logits_mask(x), largest=True))


def definition(net, frame, size, mirror, refine, clean_fn=None, **paint):
    """``apply_guided`` fed the device's own prep and logits of this frame."""
    from fosvos_hip import ops
    with torch.no_grad():
        image = ops.frame_prep(dev(frame[None]), mirror, net_size=size)
        logits = net(image)[-1].contiguous().cpu().numpy()[0, 0]
    if clean_fn is not None:
        logits = clean_fn(logits)
    return G.apply_guided(frame, image.cpu().numpy(), logits, mirror, radius=refine.radius, eps=refine.eps, clip=refine.clip, **paint)


@pytest.mark.parametrize("size", [SIZE, None], ids=["scaled", "unscaled"])
def test_segmenter_with_refine_is_apply_guided(size):
    from fosvos_hip.options import CleanOptions, RefineOptions
    from fosvos_hip.stream import FrameSegmenter
    net = RedThreshold().to(DEV).eval()
    frames = RC.drifting_frames(4, HF, WF, distractor=(70, 8, 9, 11))
    for refine, kw, clean in ((RefineOptions(), dict(), False), (RefineOptions(radius=2, eps=50.0, clip=3.0), dict(mirror=False, color="g", alpha=0.5), False),
                              (RefineOptions(), dict(overlay=False), False), (RefineOptions(), dict(), True),
                              (RefineOptions(), dict(overlay=False, mirror=False), True)):
        paint = dict(overlay_on=kw.get("overlay", True), color=kw.get("color", "r"), alpha=kw.get("alpha", 1.0))
        want = [definition(net, f, size, kw.get("mirror", True), refine, clean_largest if clean else None, **paint) for f in frames]
        if clean:
            plain = definition(net, frames[0], size, kw.get("mirror", True), refine, None, **paint)
            assert plain.tobytes() != want[0].tobytes()   # the cleaning matters here
        extra = dict(clean=CleanOptions(largest=True)) if clean else {}
        outs = []
        for depth in (1, 2):
            with FrameSegmenter(net, HF, WF, depth=depth, net_size=size, refine=refine, **kw, **extra) as seg:
                assert all(s.coeff.shape == (1, 2) + (size or (HF, WF)) and s.coeff.dtype == torch.float64 for s in seg._free)
                outs.append(list(seg.segment(frames)))
        for k in range(len(frames)):
            assert outs[0][k].tobytes() == outs[1][k].tobytes(), (kw, clean, k)
            assert outs[0][k].shape == want[k].shape and outs[0][k].tobytes() == want[k].tobytes(), (kw, clean, k)
    # the refined mask is not the bilinear one on these frames: the filter does something
    bilinear = R.apply_scaled(frames[0], RC.threshold_net_fn(R.prepare_frame_scaled(frames[0], *SIZE, True)), True, False) if size else None
    if bilinear is not None:
        assert bilinear.tobytes() != definition(net, frames[0], size, True, RefineOptions(), overlay_on=False).tobytes()


def test_segmenter_with_refine_jpeg_is_the_same_picture():
    from fosvos_hip.options import RefineOptions
    from fosvos_hip.stream import FrameSegmenter
    net = RedThreshold().to(DEV).eval()
    frames = RC.drifting_frames(3, HF, WF)
    refine = RefineOptions()
    want = [jpeg_layout.encode(definition(net, f, SIZE, True, refine), 90) for f in frames]
    with FrameSegmenter(net, HF, WF, depth=2, net_size=SIZE, refine=refine, encode="jpeg", quality=90) as seg:
        got = list(seg.segment(frames))
    assert [isinstance(g, bytes) for g in got] == [True] * 3 and got == want


def test_a_segmenter_without_refine_is_what_it_was():
    """``refine=None``: the bytes of ``frame_resample.apply_scaled`` and the launches of before; with it, the two ops in place of
    the overlay and nothing else."""
    from fosvos_hip import LaunchProfile
    from fosvos_hip.options import RefineOptions
    from fosvos_hip.stream import FrameSegmenter
    net = RedThreshold().to(DEV).eval()
    frames = RC.drifting_frames(3, HF, WF)

    def launched(**kw):
        with FrameSegmenter(net, HF, WF, **kw) as seg:
            off = kw.get("refine") is None
            assert (seg.refine is None) == off and all((s.coeff is None) == off for s in seg._free)
            with LaunchProfile(0) as prof:
                outs = [seg.apply(f) for f in frames]
        return {k: v["launches"] for k, v in prof.records.items()}, outs

    names, outs = launched(net_size=SIZE)
    assert names == {"k_frame_prep_scaled": 3, "k_overlay_scaled": 3}
    for f, o in zip(frames, outs):
        lg = RC.threshold_net_fn(R.prepare_frame_scaled(f, SIZE[0], SIZE[1], True))
        assert o.tobytes() == R.apply_scaled(f, lg, True).tobytes()
    names, outs = launched(net_size=SIZE, refine=None)
    assert names == {"k_frame_prep_scaled": 3, "k_overlay_scaled": 3}
    names, _ = launched()
    assert names == {"k_frame_prep": 3, "k_overlay": 3}
    names, _ = launched(net_size=SIZE, refine=RefineOptions())
    assert names == {"k_frame_prep_scaled": 3, "k_guided_fit": 3, "k_guided_smooth": 3, "k_overlay_guided": 3}
    names, _ = launched(refine=RefineOptions())
    assert names == {"k_frame_prep": 3, "k_guided_fit": 3, "k_guided_smooth": 3, "k_overlay_guided": 3}


def test_run_webcam_main_with_refine(tmp_path):
    import run_webcam
    from fosvos_hip.options import RefineOptions
    from networks.osvos_vgg import OSVOS_VGG
    from oracle import osvos_ref as O
    net = OSVOS_VGG(pretrained=0)
    net.load_state_dict(O.make_state_dict(2))
    path = tmp_path / "vgg.pth"
    torch.save(O.make_state_dict(2), str(path))
    out = tmp_path / "out"
    h, w = HF, WF
    rates = run_webcam.main(["--variant", "vgg", "--model", str(path), "--synthetic", "2", "--height", str(h), "--width", str(w),
                             "--net-height", str(SIZE[0]), "--net-width", str(SIZE[1]), "--refine", "--refine-radius", "2",
                             "--output", str(out)])
    assert len(rates) == 2 and sorted(os.listdir(str(out))) == ["00000.png", "00001.png"]
    from PIL import Image
    net = net.to(DEV).eval()
    for k in range(2):
        frame = run_webcam.synthetic_frame(h, w, k)
        want = definition(net, frame, SIZE, True, RefineOptions(radius=2))
        got = np.asarray(Image.open(str(out / ("%05d.png" % k))))[:, :, ::-1]
        assert np.array_equal(got, want), k
