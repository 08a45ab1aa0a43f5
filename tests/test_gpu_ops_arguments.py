"""The argument checks of ``fosvos_hip.ops`` from ``prob_bytes`` down and of the segmenters' constructors, seen from both
sides: a good call makes exactly the C calls written out below (entry, every integer, float and flag argument, the workspace
it asked for), and a call with exactly one fault raises the class and the message written out below before any launch.

``ops.lib`` is replaced by a proxy that records the entry's name and its non-pointer arguments (by the ctypes signature of
``fosvos_hip.SIGNATURES``) and forwards the call; ``ops._WS`` by a fresh workspace, so that the size handed to an entry is
the first growth of the buffer (1 MiB) and not what an earlier test left.  Nothing here looks at what a kernel computes."""
import contextlib
import ctypes
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fosvos_amd"))

import fosvos_hip  # noqa: E402
from fosvos_hip import ops, stream  # noqa: E402
from fosvos_hip.options import CleanOptions, RefineOptions, RoiOptions  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, H, W, HN, WN = 2, 12, 20, 6, 10
MIB = 1 << 20
NO_CPU = "tensor must live on the GPU (the HIP path has no CPU fallback)"
VALUES = (ctypes.c_int, ctypes.c_size_t, ctypes.c_float, ctypes.c_double, ctypes.c_int64)
F32, F64, U8, I32, I64 = torch.float32, torch.float64, torch.uint8, torch.int32, torch.int64


class Recorder:
    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        fn, argtypes = getattr(self.real, name), fosvos_hip.SIGNATURES[name][1]

        def call(*args):
            self.calls.append((name[len("fosvos_"):],) + tuple(a for a, t in zip(args, argtypes) if t in VALUES))
            return fn(*args)
        return call

    def launches(self):
        """Without the host-only size queries."""
        return [c for c in self.calls if not c[0].endswith("_bytes")]


@contextlib.contextmanager
def recording():
    rec = Recorder(fosvos_hip.lib())
    saved = ops.lib, ops._WS
    ops.lib, ops._WS = (lambda: rec), ops.Workspace()
    try:
        yield rec
    finally:
        ops.lib, ops._WS = saved


class Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))

    def forward(self, x):
        return [x[:, :1] * self.w]


class Tensors:
    """The operands of every case, made once."""

    def __init__(self):
        g = torch.Generator().manual_seed(7)
        rnd = lambda *s: torch.randn(*s, generator=g).to(DEV)  # noqa: E731
        byt = lambda *s: torch.randint(0, 256, s, generator=g, dtype=U8).to(DEV)  # noqa: E731
        self.fr, self.fr16 = byt(N, H, W, 3), byt(N, 16, 16, 3)
        self.lg, self.lgs, self.img = rnd(N, 1, H, W), rnd(N, 1, HN, WN), rnd(N, 3, HN, WN)
        self.maps, self.maps_s = [rnd(N, 1, H, W) for _ in range(3)], [rnd(N, 1, HN, WN) for _ in range(3)]
        self.u8, self.gt, self.odd = byt(N, H, W), byt(N, H, W) & 1, byt(N, 33, 9)
        self.labels = byt(N, H, W) % 4
        self.win = torch.tensor([[0, 0, H, W]] * N, dtype=I32, device=DEV)
        self.coeff = torch.randn(N, 2, HN, WN, generator=g, dtype=F64).to(DEV)
        self.pal = byt(256, 3)
        self.label = (rnd(N, 1, H, W) > 0).float()
        self.void = (byt(N, 1, H, W) > 200).to(U8)
        self.net = Net().to(DEV)
        self.nets = [Net().to(DEV) for _ in range(3)]
        flat = torch.full((N, 16, 16, 3), 90, dtype=U8, device=DEV)
        buf, lengths = ops.jpeg_encode(flat, 90)
        self.jpegs = [bytes(buf[i, :int(lengths[i])].cpu().numpy()) for i in range(N)]
        buf, lengths = ops.jpeg_encode(flat, 90, subsampling='4:2:0')
        self.jpegs420 = [bytes(buf[i, :int(lengths[i])].cpu().numpy()) for i in range(N)]

    def new(self, shape, dtype):
        return torch.empty(shape, dtype=dtype, device=DEV)


_T = None


def tensors():
    global _T
    if _T is None:
        _T = Tensors()
    return _T


def cap(entry, *args):
    return int(getattr(fosvos_hip.lib(), "fosvos_" + entry)(*args))


# ------------------------------------------------------------------------------------------------ good calls
def good_calls(T):
    """name -> (the call, the C calls it makes).  A size query is ('..._bytes', its arguments); a launch is (entry, its value
    arguments in the order of include/fosvos_hip.h, workspace bytes where it takes one, device)."""
    new = T.new
    png, pngi, png_odd = cap("png_capacity_bytes", N, H, W), cap("png_indexed_capacity_bytes", N, H, W), cap("png_capacity_bytes", N, 33, 9)
    j3, j1, j420 = cap("jpeg_capacity_bytes", N, H, W, 3, 444), cap("jpeg_capacity_bytes", N, H, W, 1, 444), \
        cap("jpeg_capacity_bytes", N, 16, 16, 3, 420)
    j_odd = cap("jpeg_capacity_bytes", N, 33, 9, 1, 420)
    nb, nb420 = sum(_scan_bytes(f) for f in T.jpegs), sum(_scan_bytes(f) for f in T.jpegs420)
    ns, ns420 = sum(_segments(f) for f in T.jpegs), sum(_segments(f) for f in T.jpegs420)
    return {
        "prob_bytes": (lambda: ops.prob_bytes(T.lg), [("prob_bytes", N, H, W, 0)]),
        "prob_bytes out": (lambda: ops.prob_bytes(T.lg, out=new((N, H, W), U8)), [("prob_bytes", N, H, W, 0)]),
        "jf_counts": (lambda: ops.jf_counts(T.lg, T.gt),
                      [("jf_workspace_bytes", N, H, W), ("jf_counts", N, H, W, 1, MIB, 0)]),
        "jf_counts radius out": (lambda: ops.jf_counts(T.lg, T.gt, radius=3, out=new((N, 6), I32)),
                                 [("jf_workspace_bytes", N, H, W), ("jf_counts", N, H, W, 3, MIB, 0)]),
        "component_roots": (lambda: ops.component_roots(T.lg), [("component_roots", N, H, W, 0, 0)]),
        "component_roots out": (lambda: ops.component_roots(T.lg, out=new((N, H, W), I32)), [("component_roots", N, H, W, 0, 0)]),
        "clean_components": (lambda: ops.clean_components(T.lg),
                             [("components_workspace_bytes", N, H, W), ("clean_components", N, H, W, 0, 0, 0, 0, -100.0, MIB, 0)]),
        "clean_components all": (lambda: ops.clean_components(T.lg, seed=T.u8, radius=8, min_area=3, largest=True, fill=-7.5,
                                                              out=new((N, 1, H, W), F32), kept=new((N, H, W), U8)),
                                 [("components_workspace_bytes", N, H, W), ("clean_components", N, H, W, 8, 3, 1, 0, -7.5, MIB, 0)]),
        "clean_components chain": (lambda: ops.clean_components(T.lg, seed=T.u8[:1], radius=2, chain=True, min_area=1),
                                   [("components_workspace_bytes", N, H, W),
                                    ("clean_components", N, H, W, 2, 1, 0, 1, -100.0, MIB, 0)]),
        "distance_gate": (lambda: ops.distance_gate(T.u8, 1000),
                          [("distance_gate_workspace_bytes", N, H, W), ("distance_gate", N, H, W, 1000, 0, MIB, 0)]),
        "distance_gate invert out": (lambda: ops.distance_gate(T.u8, 0, invert=True, out=new((N, H, W), U8)),
                                     [("distance_gate_workspace_bytes", N, H, W), ("distance_gate", N, H, W, 0, 1, MIB, 0)]),
        "adapt_labels": (lambda: ops.adapt_labels(T.lg, T.gt, 3.5, 4),
                         [("adapt_labels_workspace_bytes", N, H, W), ("adapt_labels", N, H, W, 3.5, 4, 0, MIB, 0)]),
        "adapt_labels erode out": (lambda: ops.adapt_labels(T.lg, T.gt, float("inf"), 1000, erode=2, label=new((N, 1, H, W), F32),
                                                            void=new((N, 1, H, W), U8), counts=new((N, 3), I32)),
                                   [("adapt_labels_workspace_bytes", N, H, W), ("adapt_labels", N, H, W, float("inf"), 1000, 2, MIB, 0)]),
        "cbce_loss_frames void": (lambda: ops.cbce_loss_frames(T.lg, T.label, size_average=False, void=T.void),
                                  [("cbce_void_workspace_bytes", H * W, N), ("cbce_loss_frames_void", H * W, N, 0, 1.0, MIB, 0)]),
        "png_capacity": (lambda: ops.png_capacity(H, W), [("png_capacity_bytes", 1, H, W)]),
        "png_encode": (lambda: ops.png_encode(T.u8),
                       [("png_capacity_bytes", N, H, W), ("png_workspace_bytes", N, H, W, 0), ("png_encode", N, H, W, 0, png, MIB, 0)]),
        "png_encode fitted out": (lambda: ops.png_encode(T.u8, out=new((N, png + 5), U8), lengths=new((N,), I32), huffman='fitted'),
                                  [("png_capacity_bytes", N, H, W), ("png_workspace_bytes", N, H, W, 1),
                                   ("png_encode", N, H, W, 1, png + 5, MIB, 0)]),
        "png_encode 33x9": (lambda: ops.png_encode(T.odd),
                            [("png_capacity_bytes", N, 33, 9), ("png_workspace_bytes", N, 33, 9, 0),
                             ("png_encode", N, 33, 9, 0, png_odd, MIB, 0)]),
        "merge_objects 1": (lambda: ops.merge_objects(T.maps[:1]), [("merge_objects", 1, N, H, W, 0)]),
        "merge_objects 3 out": (lambda: ops.merge_objects(T.maps, out=new((N, H, W), U8)), [("merge_objects", 3, N, H, W, 0)]),
        "jf_counts_labels": (lambda: ops.jf_counts_labels(T.labels, T.gt, 1),
                             [("jf_labels_workspace_bytes", N, 1, H, W), ("jf_counts_labels", N, 1, H, W, 1, MIB, 0)]),
        "jf_counts_labels 16 out": (lambda: ops.jf_counts_labels(T.labels, T.gt, 16, radius=2, out=new((N, 16, 6), I32)),
                                    [("jf_labels_workspace_bytes", N, 16, H, W), ("jf_counts_labels", N, 16, H, W, 2, MIB, 0)]),
        "png_indexed_capacity": (lambda: ops.png_indexed_capacity(H, W), [("png_indexed_capacity_bytes", 1, H, W)]),
        "png_encode_indexed": (lambda: ops.png_encode_indexed(T.labels),
                               [("png_indexed_capacity_bytes", N, H, W), ("png_workspace_bytes", N, H, W, 0),
                                ("png_encode_indexed", N, H, W, 0, pngi, MIB, 0)]),
        "png_encode_indexed fitted palette out": (
            lambda: ops.png_encode_indexed(T.labels, T.pal, out=new((N, pngi), U8), lengths=new((N,), I32), huffman='fitted'),
            [("png_indexed_capacity_bytes", N, H, W), ("png_workspace_bytes", N, H, W, 1),
             ("png_encode_indexed", N, H, W, 1, pngi, MIB, 0)]),
        "jpeg_capacity": (lambda: ops.jpeg_capacity(H, W, 3, '4:2:0'), [("jpeg_capacity_bytes", 1, H, W, 3, 420)]),
        "jpeg_encode": (lambda: ops.jpeg_encode(T.fr),
                        [("jpeg_capacity_bytes", N, H, W, 3, 444), ("jpeg_workspace_bytes", N, H, W, 3, 444),
                         ("jpeg_encode", N, H, W, 3, 444, 90, j3, MIB, 0)]),
        "jpeg_encode grey": (lambda: ops.jpeg_encode(T.u8, quality=1),
                             [("jpeg_capacity_bytes", N, H, W, 1, 444), ("jpeg_workspace_bytes", N, H, W, 1, 444),
                              ("jpeg_encode", N, H, W, 1, 444, 1, j1, MIB, 0)]),
        "jpeg_encode 4:2:0 out": (lambda: ops.jpeg_encode(T.fr16, 100.0, out=new((N, j420), U8), lengths=new((N,), I32),
                                                          subsampling='4:2:0'),
                                  [("jpeg_capacity_bytes", N, 16, 16, 3, 420), ("jpeg_workspace_bytes", N, 16, 16, 3, 420),
                                   ("jpeg_encode", N, 16, 16, 3, 420, 100, j420, MIB, 0)]),
        "jpeg_encode 33x9": (lambda: ops.jpeg_encode(T.odd, subsampling='4:2:0'),
                             [("jpeg_capacity_bytes", N, 33, 9, 1, 420), ("jpeg_workspace_bytes", N, 33, 9, 1, 420),
                              ("jpeg_encode", N, 33, 9, 1, 420, 90, j_odd, MIB, 0)]),
        "jpeg_decode_workspace": (lambda: ops.jpeg_decode_workspace(N, 16, 16, 3), [("jpeg_decode_workspace_bytes", N, 16, 16, 3, 444)]),
        "jpeg_decode": (lambda: ops.jpeg_decode(T.jpegs),
                        [("jpeg_decode_workspace_bytes", N, 16, 16, 3, 444), ("jpeg_decode", nb, ns, N, 16, 16, 3, 444, MIB, 0)]),
        "jpeg_decode 4:2:0 out": (lambda: ops.jpeg_decode(T.jpegs420, out=new((N, 16, 16, 3), U8), status=new((N,), I32)),
                                  [("jpeg_decode_workspace_bytes", N, 16, 16, 3, 420),
                                   ("jpeg_decode", nb420, ns420, N, 16, 16, 3, 420, MIB, 0)]),
        "frame_prep": (lambda: ops.frame_prep(T.fr), [("frame_prep", N, H, W, 0, 0)]),
        "frame_prep own size": (lambda: ops.frame_prep(T.fr, mirror=True, net_size=(H, W)), [("frame_prep", N, H, W, 1, 0)]),
        "frame_prep scaled out": (lambda: ops.frame_prep(T.fr, mirror=True, out=new((N, 3, HN, WN), F32), net_size=(HN, WN)),
                                  [("frame_prep_scaled", N, H, W, HN, WN, 1, 0)]),
        "overlay": (lambda: ops.overlay(T.fr, T.lg), [("overlay", N, H, W, 0, 0, 2, 1.0, 0)]),
        "overlay soft mask": (lambda: ops.overlay(T.fr, T.lg, mirror=True, boolean_mask=False, color='b', alpha=0, overlay=False),
                              [("overlay", N, H, W, 1, 3, 0, 0.0, 0)]),
        "overlay scaled soft": (lambda: ops.overlay(T.fr, T.lgs, boolean_mask=False, color='g', alpha=0.5, net_size=(HN, WN)),
                                [("overlay_scaled", N, H, W, HN, WN, 0, 1, 1, 0.5, 0)]),
        "overlay scaled mask out": (lambda: ops.overlay(T.fr, T.lgs, overlay=False, out=new((N, H, W), U8), net_size=(HN, WN)),
                                    [("overlay_scaled", N, H, W, HN, WN, 0, 2, 2, 1.0, 0)]),
        "guided_coefficients": (lambda: ops.guided_coefficients(T.img, T.lgs),
                                [("guided_coefficients_workspace_bytes", N, HN, WN),
                                 ("guided_coefficients", N, HN, WN, 4, 400.0, 6.0, MIB, 0)]),
        "guided_coefficients edges out": (lambda: ops.guided_coefficients(T.img, T.lgs, radius=8, eps=1e-3, clip=1e4,
                                                                          out=new((N, 2, HN, WN), F64)),
                                          [("guided_coefficients_workspace_bytes", N, HN, WN),
                                           ("guided_coefficients", N, HN, WN, 8, 1e-3, 1e4, MIB, 0)]),
        "overlay_guided": (lambda: ops.overlay_guided(T.fr, T.coeff), [("overlay_guided", N, H, W, HN, WN, 0, 0, 2, 1.0, 0)]),
        "overlay_guided soft mask out": (lambda: ops.overlay_guided(T.fr, T.coeff, mirror=True, boolean_mask=False, color='g', alpha=2,
                                                                    overlay=False, out=new((N, H, W), U8)),
                                         [("overlay_guided", N, H, W, HN, WN, 1, 3, 1, 2.0, 0)]),
        "frame_prep_window": (lambda: ops.frame_prep_window(T.fr, T.win, (HN, WN)), [("frame_prep_window", N, H, W, HN, WN, 0, 0)]),
        "frame_prep_window own size out": (lambda: ops.frame_prep_window(T.fr, T.win, (H, W), mirror=True, out=new((N, 3, H, W), F32)),
                                           [("frame_prep_window", N, H, W, H, W, 1, 0)]),
        "overlay_window": (lambda: ops.overlay_window(T.fr, T.lgs, T.win), [("overlay_window", N, H, W, HN, WN, 0, 0, 2, 1.0, 0)]),
        "overlay_window soft mask out": (lambda: ops.overlay_window(T.fr, T.lgs, T.win, mirror=True, boolean_mask=False, color='b',
                                                                    alpha=0.25, overlay=False, out=new((N, H, W), U8)),
                                         [("overlay_window", N, H, W, HN, WN, 1, 3, 0, 0.25, 0)]),
        "window_next": (lambda: ops.window_next(T.lgs, T.win, (H, W)),
                        [("window_next_workspace_bytes", N), ("window_next", N, H, W, HN, WN, 8, 250, 16, MIB, 0)]),
        "window_next out": (lambda: ops.window_next(T.lgs, T.win.clone(), (H, W), levels=3, margin=0.5, min_pad=2,
                                                          out=new((N, 4), I32)),
                                  [("window_next_workspace_bytes", N), ("window_next", N, H, W, HN, WN, 3, 500, 2, MIB, 0)]),
        "overlay_objects 1": (lambda: ops.overlay_objects(T.fr, T.maps[:1]), [("overlay_objects", 1, N, H, W, 0, 0.5, 0)]),
        "overlay_objects 3 palette": (lambda: ops.overlay_objects(T.fr, T.maps, mirror=True, palette=T.pal, alpha=1),
                                      [("overlay_objects", 3, N, H, W, 1, 1.0, 0)]),
        "overlay_objects 3 labels": (lambda: ops.overlay_objects(T.fr, T.maps, overlay=False), [("merge_objects", 3, N, H, W, 0)]),
        "overlay_objects 3 scaled": (lambda: ops.overlay_objects(T.fr, T.maps_s, alpha=0, net_size=(HN, WN)),
                                     [("overlay_objects_scaled", 3, N, H, W, HN, WN, 0, 0, 0.0, 0)]),
        "overlay_objects 3 scaled labels out": (lambda: ops.overlay_objects(T.fr, T.maps_s, mirror=True, overlay=False,
                                                                            out=new((N, H, W), U8), net_size=(HN, WN)),
                                                [("overlay_objects_scaled", 3, N, H, W, HN, WN, 1, 1, 0.5, 0)]),
        # the constructors: a size query where a file is encoded, nothing else
        "FrameSegmenter": (lambda: stream.FrameSegmenter(T.net, H, W).close(), []),
        "FrameSegmenter jpeg": (lambda: stream.FrameSegmenter(T.net, 16, 16, encode='jpeg', quality=100, subsampling='4:2:0',
                                                              budget=1, net_size=(8, 8)).close(),
                                [("jpeg_capacity_bytes", 1, 16, 16, 3, 420)]),
        "FrameSegmenter jpeg mask": (lambda: stream.FrameSegmenter(T.net, H, W, overlay=False, encode='jpeg', quality=1).close(),
                                     [("jpeg_capacity_bytes", 1, H, W, 1, 444)]),
        "FrameSegmenter roi": (lambda: stream.FrameSegmenter(T.net, H, W, net_size=(HN, WN), roi=RoiOptions()).close(), []),
        "FrameSegmenter refine clean": (lambda: stream.FrameSegmenter(T.net, H, W, net_size=(HN, WN), refine=RefineOptions(),
                                                                      clean=CleanOptions(temporal_radius=2)).close(), []),
        "ObjectSegmenter 1": (lambda: stream.ObjectSegmenter(T.nets[:1], H, W).close(), []),
        "ObjectSegmenter 3 png": (lambda: stream.ObjectSegmenter(T.nets, H, W, overlay=False, encode='png', huffman='fitted',
                                                                 palette=T.pal, net_size=(HN, WN)).close(),
                                  [("png_indexed_capacity_bytes", 1, H, W)]),
        "ObjectSegmenter 3 jpeg": (lambda: stream.ObjectSegmenter(T.nets, H, W, encode='jpeg', palette=T.pal.cpu().numpy(),
                                                                  budget=4096).close(),
                                   [("jpeg_capacity_bytes", 1, H, W, 3, 444)]),
    }


def _scan_bytes(f):
    from util import jpeg_read
    b0, b1 = jpeg_read.probe(f).scan
    return b1 - b0


def _segments(f):
    from util import jpeg_read
    return len(jpeg_read.probe(f).segments)


GOOD = ("prob_bytes", "prob_bytes out", "jf_counts", "jf_counts radius out", "component_roots", "component_roots out",
        "clean_components", "clean_components all", "clean_components chain", "distance_gate", "distance_gate invert out",
        "adapt_labels", "adapt_labels erode out", "cbce_loss_frames void", "png_capacity", "png_encode", "png_encode fitted out",
        "png_encode 33x9", "merge_objects 1", "merge_objects 3 out", "jf_counts_labels", "jf_counts_labels 16 out",
        "png_indexed_capacity", "png_encode_indexed", "png_encode_indexed fitted palette out", "jpeg_capacity", "jpeg_encode",
        "jpeg_encode grey", "jpeg_encode 4:2:0 out", "jpeg_encode 33x9", "jpeg_decode_workspace", "jpeg_decode",
        "jpeg_decode 4:2:0 out", "frame_prep", "frame_prep own size", "frame_prep scaled out", "overlay", "overlay soft mask",
        "overlay scaled soft", "overlay scaled mask out", "guided_coefficients", "guided_coefficients edges out", "overlay_guided",
        "overlay_guided soft mask out", "frame_prep_window", "frame_prep_window own size out", "overlay_window",
        "overlay_window soft mask out", "window_next", "window_next out", "overlay_objects 1", "overlay_objects 3 palette",
        "overlay_objects 3 labels", "overlay_objects 3 scaled", "overlay_objects 3 scaled labels out", "FrameSegmenter",
        "FrameSegmenter jpeg", "FrameSegmenter jpeg mask", "FrameSegmenter roi", "FrameSegmenter refine clean", "ObjectSegmenter 1",
        "ObjectSegmenter 3 png", "ObjectSegmenter 3 jpeg")


def test_the_list_of_good_calls_is_whole():
    assert sorted(GOOD) == sorted(good_calls(tensors()))


@pytest.mark.parametrize("name", GOOD)
def test_good_call_makes_these_c_calls(name):
    call, expected = good_calls(tensors())[name]
    with recording() as rec:
        call()
    torch.cuda.synchronize()
    assert rec.calls == expected


# ------------------------------------------------------------------------------------------------ single faults
def strided(t):
    """``t``'s shape and dtype, not contiguous."""
    wide = torch.zeros(tuple(t.shape[:-1]) + (2 * t.shape[-1],), dtype=t.dtype, device=t.device)
    return wide[..., ::2]


def operand(call, t, what, other, dtype_error=ValueError, tag=""):
    """The three faults of a tensor operand ``t`` of ``call(t)``: dtype, host memory, strides."""
    return [(f"{what}{tag}: dtype", lambda: call(t.to(other)), dtype_error, f"{what}: expected {t.dtype}, got {other}"),
            (f"{what}{tag}: cpu", lambda: call(t.cpu()), RuntimeError, f"{what}: {NO_CPU}"),
            (f"{what}{tag}: strided", lambda: call(strided(t)), ValueError, f"{what}: tensor must be contiguous")]


def out_buffer(call, shape, dtype, other, op, name="out", what=None):
    """... and of an output buffer of ``call(buffer)``, with a wrong shape as the fourth."""
    what = what or f"{op} {name}"
    t = torch.zeros(shape, dtype=dtype, device=DEV)
    wrong = tuple(shape[:-1]) + (shape[-1] + 1,)
    return operand(call, t, what, other, tag=f" {tuple(shape)}") + [
        (f"{what} {tuple(shape)}: shape", lambda: call(torch.zeros(wrong, dtype=dtype, device=DEV)), ValueError,
         f"{op}: {name} must be {tuple(shape)}, got {wrong}")]


def file_buffers(call, n, capacity, op):
    """The (out, lengths) pair of a file encoder, ``call(out=, lengths=)``."""
    out = torch.zeros((n, capacity), dtype=U8, device=DEV)
    rows = operand(lambda t: call(out=t), out, f"{op} out", I32)
    for wrong in ((n, capacity - 1), (n + 1, capacity), (n * capacity,)):
        rows.append((f"{op} out: shape {wrong}", lambda wrong=wrong: call(out=torch.zeros(wrong, dtype=U8, device=DEV)), ValueError,
                     f"{op}: out must be [{n}, >= {capacity}], got {wrong}"))
    return rows + out_buffer(lambda t: call(lengths=t), (n,), I32, I64, op, "lengths")


def scalar(call, op, name, values, expect):
    return [(f"{op} {name}={v!r}", lambda v=v: call(v), ValueError, f"{op}: {name} must be {expect}, got {v!r}") for v in values]


NAN, INF = float("nan"), float("inf")


def paint(call, op):
    """color and alpha of the three single-object paint launches, ``call(color=, alpha=)``."""
    return scalar(lambda v: call(color=v), op, "color", ('x', 'R', None), "one of ('b', 'g', 'r')") + \
        [(f"{op} alpha={v!r}", lambda v=v: call(alpha=v), ValueError, f"{op}: alpha must be a finite number >= 0, got {float(v)!r}")
         for v in (-0.5, NAN, INF, -INF)]


def net_size(call, op, frames=(H, W)):
    return scalar(call, op, "net_size", (7, (1, 2, 3)), "a pair (Hn, Wn)") + \
        scalar(call, op, "net_size", ((0, WN), (HN, -1), (True, WN), (6.0, WN), "ab"), "a pair of positive ints") + \
        [(f"{op} net_size too large", lambda: call((frames[0] + 1, WN)), ValueError,
          f"{op}: the net's size {(frames[0] + 1, WN)} exceeds the frames' {frames}")]


def faults(T):
    """op -> rows of (label, call with exactly one fault, exception class, full message)."""
    png, pngi = cap("png_capacity_bytes", N, H, W), cap("png_indexed_capacity_bytes", N, H, W)
    j3 = cap("jpeg_capacity_bytes", N, H, W, 3, 444)
    bad_lg = torch.zeros((N, 2, H, W), device=DEV)
    lg_msg = "logits must be a non-empty [N,1,H,W], got"
    wrong_maps = T.maps[:1] + [torch.zeros((N, 1, H, W + 1), device=DEV)]
    rows = {}
    rows["prob_bytes"] = operand(ops.prob_bytes, T.lg, "prob_bytes logits", F64) + [
        ("prob_bytes logits: shape", lambda: ops.prob_bytes(bad_lg), ValueError, f"prob_bytes: {lg_msg} {(N, 2, H, W)}"),
        ("prob_bytes logits: 3 dims", lambda: ops.prob_bytes(T.lg[:, 0]), ValueError, f"prob_bytes: {lg_msg} {(N, H, W)}"),
        ("prob_bytes logits: empty", lambda: ops.prob_bytes(T.lg[:0]), ValueError, f"prob_bytes: {lg_msg} {(0, 1, H, W)}"),
    ] + out_buffer(lambda t: ops.prob_bytes(T.lg, out=t), (N, H, W), U8, I32, "prob_bytes")

    rows["jf_counts"] = operand(lambda t: ops.jf_counts(t, T.gt), T.lg, "jf_counts logits", F64) + \
        operand(lambda t: ops.jf_counts(T.lg, t), T.gt, "jf_counts gt", I32) + [
        ("jf_counts logits: shape", lambda: ops.jf_counts(bad_lg, T.gt), ValueError, f"jf_counts: {lg_msg} {(N, 2, H, W)}"),
        ("jf_counts gt: shape", lambda: ops.jf_counts(T.lg, T.gt[:1]), ValueError, f"jf_counts: gt must be {(N, H, W)}, got {(1, H, W)}"),
    ] + scalar(lambda v: ops.jf_counts(T.lg, T.gt, radius=v), "jf_counts", "radius", (0, 64), "an integer in 1..63") + \
        out_buffer(lambda t: ops.jf_counts(T.lg, T.gt, out=t), (N, 6), I32, I64, "jf_counts")

    rows["component_roots"] = operand(ops.component_roots, T.lg, "component_roots logits", F64) + [
        ("component_roots logits: shape", lambda: ops.component_roots(bad_lg), ValueError, f"component_roots: {lg_msg} {(N, 2, H, W)}"),
    ] + out_buffer(lambda t: ops.component_roots(T.lg, out=t), (N, H, W), I32, I64, "component_roots")

    cc = lambda **kw: ops.clean_components(T.lg, **kw)  # noqa: E731
    rows["clean_components"] = operand(ops.clean_components, T.lg, "clean_components logits", F64) + [
        ("clean_components logits: shape", lambda: ops.clean_components(bad_lg), ValueError,
         f"clean_components: {lg_msg} {(N, 2, H, W)}"),
    ] + scalar(lambda v: cc(radius=v), "clean_components", "radius", (-1, 64, True, 2.0, NAN), "an integer in 0..63") + \
        scalar(lambda v: cc(min_area=v), "clean_components", "min_area", (-1, 1 << 31, True, 1.5), "an integer in 0..2147483647") + \
        [(f"clean_components fill={v!r}", lambda v=v: cc(fill=v), ValueError,
          f"clean_components: fill must be finite and negative, got {float(v)!r}") for v in (0.0, 1, NAN, -INF, -3.5e38)] + \
        operand(lambda t: cc(seed=t), T.u8, "clean_components seed", I32) + [
        ("clean_components seed: shape", lambda: cc(seed=T.u8[:1]), ValueError,
         f"clean_components: seed must be {(N, H, W)}, got {(1, H, W)}"),
        ("clean_components seed: shape with chain", lambda: cc(seed=T.u8, chain=True), ValueError,
         f"clean_components: seed must be {(1, H, W)} with chain, got {(N, H, W)}"),
    ] + out_buffer(lambda t: cc(out=t), (N, 1, H, W), F32, F64, "clean_components") + \
        out_buffer(lambda t: cc(kept=t), (N, H, W), U8, I32, "clean_components", "kept")

    dg = lambda **kw: ops.distance_gate(T.u8, kw.pop("distance", 5), **kw)  # noqa: E731
    rows["distance_gate"] = operand(lambda t: ops.distance_gate(t, 5), T.u8, "distance_gate mask", I32) + [
        ("distance_gate mask: shape", lambda: ops.distance_gate(T.u8[:, None], 5), ValueError,
         f"distance_gate: mask must be a non-empty [N,H,W], got {(N, 1, H, W)}"),
        ("distance_gate mask: empty", lambda: ops.distance_gate(T.u8[:0], 5), ValueError,
         f"distance_gate: mask must be a non-empty [N,H,W], got {(0, H, W)}"),
        ("distance_gate out: the mask", lambda: dg(out=T.u8), ValueError, "distance_gate: out must not be the mask itself"),
    ] + scalar(lambda v: dg(distance=v), "distance_gate", "distance", (-1, 4096, True, 5.0), "an integer in 0..4095") + \
        out_buffer(lambda t: dg(out=t), (N, H, W), U8, I32, "distance_gate")

    al = lambda **kw: ops.adapt_labels(T.lg, T.gt, kw.pop("pos_logit", 3.5), kw.pop("neg_distance", 4), **kw)  # noqa: E731
    rows["adapt_labels"] = operand(lambda t: ops.adapt_labels(t, T.gt, 3.5, 4), T.lg, "adapt_labels logits", F64) + \
        operand(lambda t: ops.adapt_labels(T.lg, t, 3.5, 4), T.gt, "adapt_labels last_mask", I32) + [
        ("adapt_labels logits: shape", lambda: ops.adapt_labels(bad_lg, T.gt, 3.5, 4), ValueError,
         f"adapt_labels: {lg_msg} {(N, 2, H, W)}"),
        ("adapt_labels last_mask: shape", lambda: ops.adapt_labels(T.lg, T.gt[:1], 3.5, 4), ValueError,
         f"adapt_labels: last_mask must be {(N, H, W)}, got {(1, H, W)}"),
    ] + scalar(lambda v: al(neg_distance=v), "adapt_labels", "neg_distance", (-1, 4096, True, 4.0), "an integer in 0..4095") + \
        scalar(lambda v: al(erode=v), "adapt_labels", "erode", (-1, 4096, False, NAN), "an integer in 0..4095") + \
        scalar(lambda v: al(pos_logit=v), "adapt_labels", "pos_logit", (True, NAN, "3"), "a number") + \
        out_buffer(lambda t: al(label=t), (N, 1, H, W), F32, F64, "adapt_labels label", "out", "adapt_labels label out") + \
        out_buffer(lambda t: al(void=t), (N, 1, H, W), U8, I32, "adapt_labels void", "out", "adapt_labels void out") + \
        out_buffer(lambda t: al(counts=t), (N, 3), I32, I64, "adapt_labels counts", "out", "adapt_labels counts out")

    lf = lambda t: ops.cbce_loss_frames(T.lg, T.label, void=t)  # noqa: E731
    rows["cbce_loss_frames void"] = operand(lf, T.void, "cbce_loss_frames void", F32, TypeError) + [
        ("cbce_loss_frames void: shape", lambda: lf(T.void[:, :, :, :W - 1].contiguous()), ValueError,
         f"cbce_loss_frames: logits {(N, 1, H, W)} vs void {(N, 1, H, W - 1)}")]

    pe = lambda **kw: ops.png_encode(T.u8, **kw)  # noqa: E731
    rows["png_encode"] = scalar(lambda v: pe(huffman=v), "png_encode", "huffman", ('best', None, 1), "one of ('fixed', 'fitted')") + \
        operand(ops.png_encode, T.u8, "png_encode bytes", I32) + [
        ("png_encode bytes: shape", lambda: ops.png_encode(T.fr), ValueError,
         f"png_encode: bytes must be a non-empty [N,H,W], got {(N, H, W, 3)}"),
        ("png_encode bytes: empty", lambda: ops.png_encode(T.u8[:, :0]), ValueError,
         f"png_encode: bytes must be a non-empty [N,H,W], got {(N, 0, W)}"),
    ] + file_buffers(pe, N, png, "png_encode")

    rows["merge_objects"] = [
        ("merge_objects K=0", lambda: ops.merge_objects([]), ValueError, "merge_objects: 0 logit maps, outside [1, 16]"),
        ("merge_objects K=17", lambda: ops.merge_objects(T.maps[:1] * 17), ValueError, "merge_objects: 17 logit maps, outside [1, 16]"),
        ("merge_objects first map: shape", lambda: ops.merge_objects([bad_lg]), ValueError, f"merge_objects: {lg_msg} {(N, 2, H, W)}"),
        ("merge_objects second map: shape", lambda: ops.merge_objects(wrong_maps), ValueError,
         f"merge_objects: every logit map must be {(N, 1, H, W)}, got {(N, 1, H, W + 1)}"),
    ] + operand(lambda t: ops.merge_objects([T.lg, t]), T.lg, "merge_objects logits", F64) + \
        out_buffer(lambda t: ops.merge_objects(T.maps, out=t), (N, H, W), U8, I32, "merge_objects")

    jl = lambda **kw: ops.jf_counts_labels(T.labels, T.gt, kw.pop("n_objects", 3), **kw)  # noqa: E731
    rows["jf_counts_labels"] = operand(lambda t: ops.jf_counts_labels(t, T.gt, 3), T.labels, "jf_counts_labels pred", I32) + \
        operand(lambda t: ops.jf_counts_labels(T.labels, t, 3), T.gt, "jf_counts_labels gt", I32) + [
        ("jf_counts_labels pred: shape", lambda: ops.jf_counts_labels(T.labels[:, None], T.gt, 3), ValueError,
         f"jf_counts_labels: pred must be a non-empty [N,H,W], got {(N, 1, H, W)}"),
        ("jf_counts_labels gt: shape", lambda: ops.jf_counts_labels(T.labels, T.gt[:1], 3), ValueError,
         f"jf_counts_labels: gt must be {(N, H, W)}, got {(1, H, W)}"),
    ] + scalar(lambda v: jl(n_objects=v), "jf_counts_labels", "n_objects", (0, 17), "an integer in 1..16") + \
        scalar(lambda v: jl(radius=v), "jf_counts_labels", "radius", (0, 64), "an integer in 1..63") + \
        out_buffer(lambda t: jl(out=t), (N, 3, 6), I32, I64, "jf_counts_labels")

    pi = lambda **kw: ops.png_encode_indexed(T.labels, **kw)  # noqa: E731
    rows["png_encode_indexed"] = scalar(lambda v: pi(huffman=v), "png_encode_indexed", "huffman", ('best',), "one of ('fixed', 'fitted')") + \
        operand(ops.png_encode_indexed, T.labels, "png_encode_indexed labels", I32) + [
        ("png_encode_indexed labels: shape", lambda: ops.png_encode_indexed(T.fr), ValueError,
         f"png_encode_indexed: labels must be a non-empty [N,H,W], got {(N, H, W, 3)}"),
        ("png_encode_indexed palette: shape", lambda: pi(palette=torch.zeros((256, 4), dtype=U8, device=DEV)), ValueError,
         "png_encode_indexed: palette must be (256, 3), got (256, 4)"),
    ] + operand(lambda t: pi(palette=t), T.pal, "png_encode_indexed palette", I32) + file_buffers(pi, N, pngi, "png_encode_indexed")

    je = lambda **kw: ops.jpeg_encode(T.fr, **kw)  # noqa: E731
    rows["jpeg_encode"] = scalar(lambda v: je(subsampling=v), "jpeg_encode", "subsampling", ('4:2:2', 420, None),
                                 "one of ('4:4:4', '4:2:0')") + \
        operand(ops.jpeg_encode, T.fr, "jpeg_encode frames", I32) + [
        ("jpeg_encode frames: shape", lambda: ops.jpeg_encode(torch.zeros((N, H, W, 4), dtype=U8, device=DEV)), ValueError,
         f"jpeg_encode: frames must be a non-empty [N,H,W,3] or [N,H,W], got {(N, H, W, 4)}"),
        ("jpeg_encode frames: empty", lambda: ops.jpeg_encode(T.fr[:0]), ValueError,
         f"jpeg_encode: frames must be a non-empty [N,H,W,3] or [N,H,W], got {(0, H, W, 3)}"),
    ] + scalar(lambda v: je(quality=v), "jpeg_encode", "quality", (0, 101, True, 90.5), "an integer in 1..100") + \
        file_buffers(je, N, j3, "jpeg_encode") + \
        scalar(lambda v: ops.jpeg_capacity(H, W, 3, v), "jpeg_capacity", "subsampling", ('4:2:2',), "one of ('4:4:4', '4:2:0')") + [
        ("jpeg_capacity components", lambda: ops.jpeg_capacity(H, W, 2), ValueError,
         f"jpeg_capacity: h, w in 1..65535 and components 1 or 3, got {H}, {W}, 2")]

    jd = lambda **kw: ops.jpeg_decode(T.jpegs, device=DEV, **kw)  # noqa: E731
    rows["jpeg_decode"] = [
        ("jpeg_decode no files", lambda: ops.jpeg_decode([]), ValueError, "jpeg_decode: no files"),
        ("jpeg_decode not a file", lambda: ops.jpeg_decode([b"abc"]), ValueError,
         "jpeg_decode: file 0 is not one the device decoder takes (util/jpeg_read.probe is None): decode it on the host"),
        ("jpeg_decode two shapes", lambda: ops.jpeg_decode([T.jpegs[0], T.jpegs420[0]]), ValueError,
         "jpeg_decode: the files of one call share shape, components and sampling; file 0 is (16, 16, 3, '4:4:4'), "
         "file 1 is (16, 16, 3, '4:2:0')"),
        ("jpeg_decode plans", lambda: ops.jpeg_decode(T.jpegs, plans=[None]), ValueError, "jpeg_decode: 2 files but 1 plans"),
        ("jpeg_decode device", lambda: ops.jpeg_decode(T.jpegs, device="cpu"), RuntimeError,
         "jpeg_decode: the device must be a GPU (the HIP path has no CPU fallback), got cpu"),
        ("jpeg_decode_workspace subsampling", lambda: ops.jpeg_decode_workspace(N, 16, 16, 3, '4:1:1'), ValueError,
         "jpeg_decode_workspace: subsampling must be one of ('4:4:4', '4:2:0'), got '4:1:1'"),
    ] + out_buffer(lambda t: jd(out=t), (N, 16, 16, 3), U8, I32, "jpeg_decode") + \
        out_buffer(lambda t: jd(status=t), (N,), I32, I64, "jpeg_decode", "status")

    fp = lambda **kw: ops.frame_prep(T.fr, **kw)  # noqa: E731
    rows["frame_prep"] = operand(ops.frame_prep, T.fr, "frame_prep frames", I32) + [
        ("frame_prep frames: shape", lambda: ops.frame_prep(T.u8), ValueError,
         f"frame_prep: frames must be a non-empty [N,H,W,3], got {(N, H, W)}"),
        ("frame_prep frames: empty", lambda: ops.frame_prep(T.fr[:0]), ValueError,
         f"frame_prep: frames must be a non-empty [N,H,W,3], got {(0, H, W, 3)}"),
    ] + net_size(lambda v: fp(net_size=v), "frame_prep") + out_buffer(lambda t: fp(out=t), (N, 3, H, W), F32, F64, "frame_prep") + \
        out_buffer(lambda t: fp(out=t, net_size=(HN, WN)), (N, 3, HN, WN), F32, F64, "frame_prep")

    ov = lambda **kw: ops.overlay(T.fr, kw.pop("logits", T.lg), **kw)  # noqa: E731
    rows["overlay"] = operand(lambda t: ops.overlay(t, T.lg), T.fr, "overlay frames", I32) + \
        operand(lambda t: ov(logits=t), T.lg, "overlay logits", F64) + [
        ("overlay logits: shape", lambda: ov(logits=T.lgs), ValueError, f"overlay: logits must be {(N, 1, H, W)}, got {(N, 1, HN, WN)}"),
        ("overlay logits: shape, scaled", lambda: ov(net_size=(HN, WN)), ValueError,
         f"overlay: logits must be {(N, 1, HN, WN)}, got {(N, 1, H, W)}"),
    ] + paint(ov, "overlay") + net_size(lambda v: ov(logits=T.lgs, net_size=v), "overlay") + \
        out_buffer(lambda t: ov(out=t), (N, H, W, 3), U8, I32, "overlay") + \
        out_buffer(lambda t: ov(out=t, overlay=False), (N, H, W), U8, I32, "overlay")

    gc = lambda **kw: ops.guided_coefficients(kw.pop("image", T.img), kw.pop("logits", T.lgs), **kw)  # noqa: E731
    who = "guided_coefficients"
    rows[who] = operand(lambda t: gc(image=t), T.img, f"{who} image", F64) + operand(lambda t: gc(logits=t), T.lgs, f"{who} logits", F64) + [
        (f"{who} image: shape", lambda: gc(image=T.lgs), ValueError,
         f"{who}: image must be a non-empty [N,3,Hn,Wn], got {(N, 1, HN, WN)}"),
        (f"{who} logits: shape", lambda: gc(logits=T.lg), ValueError, f"{who}: logits must be {(N, 1, HN, WN)}, got {(N, 1, H, W)}"),
    ] + scalar(lambda v: gc(radius=v), who, "radius", (0, 9, True, 4.0), "an integer in 1..8") + \
        scalar(lambda v: gc(eps=v), who, "eps", (9e-4, 1.1e9, NAN, INF, True), "a finite number in [0.001, 1e+09]") + \
        scalar(lambda v: gc(clip=v), who, "clip", (0, 0.0, 10000.5, NAN, INF, False), "a finite number in (0, 10000]") + \
        out_buffer(lambda t: gc(out=t), (N, 2, HN, WN), F64, F32, who)

    og = lambda **kw: ops.overlay_guided(T.fr, kw.pop("coeff", T.coeff), **kw)  # noqa: E731
    who = "overlay_guided"
    rows[who] = operand(lambda t: ops.overlay_guided(t, T.coeff), T.fr, f"{who} frames", I32) + \
        operand(lambda t: og(coeff=t), T.coeff, f"{who} coeff", F32) + [
        (f"{who} coeff: shape", lambda: og(coeff=T.coeff[:, :1].contiguous()), ValueError,
         f"{who}: coeff must be a non-empty {(N, 2, 'Hn', 'Wn')}, got {(N, 1, HN, WN)}"),
        (f"{who} coeff: larger than the frames", lambda: og(coeff=torch.zeros((N, 2, H + 1, W), dtype=F64, device=DEV)), ValueError,
         f"{who}: the net's size {(H + 1, W)} exceeds the frames' {(H, W)}"),
    ] + paint(og, who) + out_buffer(lambda t: og(out=t), (N, H, W, 3), U8, I32, who) + \
        out_buffer(lambda t: og(out=t, overlay=False), (N, H, W), U8, I32, who)

    fw = lambda **kw: ops.frame_prep_window(T.fr, kw.pop("windows", T.win), kw.pop("net_size", (HN, WN)), **kw)  # noqa: E731
    who = "frame_prep_window"
    win_msg = f"windows must be int32 {(N, 4)} = (y0, x0, Hw, Ww) a frame, got"
    rows[who] = operand(lambda t: ops.frame_prep_window(t, T.win, (HN, WN)), T.fr, f"{who} frames", I32) + \
        operand(lambda t: fw(windows=t), T.win, f"{who} windows", I64) + [
        (f"{who} windows: shape", lambda: fw(windows=T.win[:1]), ValueError, f"{who}: {win_msg} {(1, 4)}"),
        (f"{who} net_size=None", lambda: fw(net_size=None), ValueError,
         f"{who}: net_size=(Hn, Wn) is needed: a window is scaled to the net's size"),
    ] + net_size(lambda v: fw(net_size=v), who) + out_buffer(lambda t: fw(out=t), (N, 3, HN, WN), F32, F64, who)

    ow = lambda **kw: ops.overlay_window(T.fr, kw.pop("logits", T.lgs), kw.pop("windows", T.win), **kw)  # noqa: E731
    who = "overlay_window"
    rows[who] = operand(lambda t: ops.overlay_window(t, T.lgs, T.win), T.fr, f"{who} frames", I32) + \
        operand(lambda t: ow(logits=t), T.lgs, f"{who} logits", F64) + operand(lambda t: ow(windows=t), T.win, f"{who} windows", I64) + [
        (f"{who} logits: shape", lambda: ow(logits=T.lgs[:1]), ValueError,
         f"{who}: logits must be a non-empty {(N, 1, 'Hn', 'Wn')}, got {(1, 1, HN, WN)}"),
        (f"{who} logits: larger than the frames", lambda: ow(logits=torch.zeros((N, 1, H, W + 1), device=DEV)), ValueError,
         f"{who}: the net's size {(H, W + 1)} exceeds the frames' {(H, W)}"),
        (f"{who} windows: shape", lambda: ow(windows=T.win[:, :3].contiguous()), ValueError, f"{who}: {win_msg} {(N, 3)}"),
    ] + paint(ow, who) + out_buffer(lambda t: ow(out=t), (N, H, W, 3), U8, I32, who) + \
        out_buffer(lambda t: ow(out=t, overlay=False), (N, H, W), U8, I32, who)

    wn = lambda **kw: ops.window_next(kw.pop("logits", T.lgs), kw.pop("windows", T.win), kw.pop("frame_size", (H, W)), **kw)  # noqa: E731
    who = "window_next"
    rows[who] = operand(lambda t: wn(logits=t), T.lgs, f"{who} logits", F64) + operand(lambda t: wn(windows=t), T.win, f"{who} windows", I64) + [
        (f"{who} logits: shape", lambda: wn(logits=T.img), ValueError, f"{who}: {lg_msg} {(N, 3, HN, WN)}"),
        (f"{who} windows: shape", lambda: wn(windows=T.win[:1]), ValueError, f"{who}: {win_msg} {(1, 4)}"),
        (f"{who} frame_size too small", lambda: wn(frame_size=(HN - 1, W)), ValueError,
         f"{who}: the net's size {(HN, WN)} exceeds the frames' {(HN - 1, W)}"),
    ] + scalar(lambda v: wn(frame_size=v), who, "frame_size", (7, None, (1, 2, 3)), "a pair (Hf, Wf)") + \
        scalar(lambda v: wn(frame_size=v), who, "frame_size", ((0, W), (H, -1), (True, W), (12.0, W)), "a pair of positive ints") + \
        scalar(lambda v: wn(levels=v), who, "levels", (0, 65, True, 8.0), "an integer in 1..64") + \
        scalar(lambda v: wn(min_pad=v), who, "min_pad", (-1, 4096, False, 16.0), "an integer in 0..4095") + \
        scalar(lambda v: wn(margin=v), who, "margin", (-0.1, 4.5, NAN, INF, True, "1"), "a finite number in [0, 4]") + \
        out_buffer(lambda t: wn(out=t), (N, 4), I32, I64, who)

    oo = lambda **kw: ops.overlay_objects(T.fr, kw.pop("logits", T.maps), **kw)  # noqa: E731
    who = "overlay_objects"
    rows[who] = operand(lambda t: ops.overlay_objects(t, T.maps), T.fr, f"{who} frames", I32) + \
        operand(lambda t: oo(logits=[T.lg, t]), T.lg, f"{who} logits", F64) + [
        (f"{who} K=0", lambda: oo(logits=[]), ValueError, f"{who}: 0 logit maps, outside [1, 16]"),
        (f"{who} K=17", lambda: oo(logits=T.maps[:1] * 17), ValueError, f"{who}: 17 logit maps, outside [1, 16]"),
        (f"{who} a map: shape", lambda: oo(logits=wrong_maps), ValueError,
         f"{who}: every logit map must be {(N, 1, H, W)}, got {(N, 1, H, W + 1)}"),
        (f"{who} a map: shape, scaled", lambda: oo(net_size=(HN, WN)), ValueError,
         f"{who}: every logit map must be {(N, 1, HN, WN)}, got {(N, 1, H, W)}"),
        (f"{who} palette: shape", lambda: oo(palette=T.pal[:255].contiguous()), ValueError, f"{who}: palette must be (256, 3), got (255, 3)"),
    ] + [(f"{who} alpha={v!r}", lambda v=v: oo(alpha=v), ValueError, f"{who}: alpha must be a finite number in [0, 1], got {float(v)!r}")
         for v in (-0.1, 1.5, NAN, INF)] + \
        operand(lambda t: oo(palette=t), T.pal, f"{who} palette", I32) + net_size(lambda v: oo(logits=T.maps_s, net_size=v), who) + \
        out_buffer(lambda t: oo(out=t), (N, H, W, 3), U8, I32, who) + out_buffer(lambda t: oo(out=t, overlay=False), (N, H, W), U8, I32, who)

    fs = lambda **kw: stream.FrameSegmenter(T.net, H, W, **kw)  # noqa: E731
    who = "FrameSegmenter"
    rows[who] = scalar(lambda v: fs(encode='jpeg', quality=v), who, "quality", (0, 101, True, 90.0), "an integer in 1..100") + \
        scalar(lambda v: fs(encode='jpeg', subsampling=v), who, "subsampling", ('4:2:2', 420), "one of ('4:4:4', '4:2:0')") + \
        scalar(lambda v: fs(encode='jpeg', budget=v), who, "budget", (0, -1, True, 1024.0), "a positive number of bytes") + \
        net_size(lambda v: fs(net_size=v), who)

    os_ = lambda **kw: stream.ObjectSegmenter(kw.pop("nets", T.nets), H, W, **kw)  # noqa: E731
    who = "ObjectSegmenter"
    pal_msg = f"{who}: a palette must be a contiguous uint8 [256,3] array or tensor on {DEV}"
    rows[who] = [
        (f"{who} K=0", lambda: os_(nets=[]), ValueError, f"{who}: 0 nets, outside [1, 16]"),
        (f"{who} K=17", lambda: os_(nets=[Net().to(DEV) for _ in range(17)]), ValueError, f"{who}: 17 nets, outside [1, 16]"),
    ] + scalar(lambda v: os_(huffman=v), who, "huffman", ('best',), "one of ('fixed', 'fitted')") + \
        scalar(lambda v: os_(encode='jpeg', quality=v), who, "quality", (0, 101), "an integer in 1..100") + \
        scalar(lambda v: os_(overlay=False, encode='png', budget=v), who, "budget", (0, True), "a positive number of bytes") + \
        [(f"{who} palette: {label}", lambda p=p: os_(palette=p), ValueError, pal_msg)
         for label, p in (("dtype", T.pal.to(I32)), ("cpu", T.pal.cpu()), ("strided", strided(T.pal)),
                          ("shape", T.pal[:255].contiguous()), ("a list", [[0, 0, 0]] * 256))]
    return rows


OPS = ("prob_bytes", "jf_counts", "component_roots", "clean_components", "distance_gate", "adapt_labels", "cbce_loss_frames void",
       "png_encode", "merge_objects", "jf_counts_labels", "png_encode_indexed", "jpeg_encode", "jpeg_decode", "frame_prep", "overlay",
       "guided_coefficients", "overlay_guided", "frame_prep_window", "overlay_window", "window_next", "overlay_objects",
       "FrameSegmenter", "ObjectSegmenter")


def test_the_list_of_ops_is_whole():
    assert sorted(OPS) == sorted(faults(tensors()))


def run_rows(rows):
    """Every row's call: the class and the whole message, and no launch.  All misses of a table are reported together."""
    missed = []
    for label, call, error, message in rows:
        with recording() as rec:
            try:
                call()
                got = "no exception"
            except Exception as e:  # noqa: BLE001  (the row names the one it expects)
                got = (type(e), str(e))
        if got != (error, message) or rec.launches():
            missed.append(f"{label}: expected {(error, message)}, got {got}, launches {rec.launches()}")
    assert not missed, "\n".join(missed)


@pytest.mark.parametrize("op", OPS)
def test_a_single_fault_raises_before_any_launch(op):
    rows = faults(tensors())[op]
    labels = [r[0] for r in rows]
    assert len(set(labels)) == len(labels)
    run_rows(rows)


def other_gpu_rows(T):
    """One tensor of the call on another GPU: op -> rows."""
    on1 = lambda t: t.to("cuda:1")  # noqa: E731
    msg = lambda op: f"{op}: every tensor must be on {DEV}, got one on cuda:1"  # noqa: E731
    pngc, j3 = cap("png_capacity_bytes", N, H, W), cap("jpeg_capacity_bytes", N, H, W, 3, 444)
    calls = {
        "prob_bytes": [lambda: ops.prob_bytes(T.lg, out=on1(T.u8))],
        "jf_counts": [lambda: ops.jf_counts(T.lg, on1(T.gt)), lambda: ops.jf_counts(T.lg, T.gt, out=torch.zeros((N, 6), dtype=I32, device="cuda:1"))],
        "component_roots": [lambda: ops.component_roots(T.lg, out=torch.zeros((N, H, W), dtype=I32, device="cuda:1"))],
        "clean_components": [lambda: ops.clean_components(T.lg, seed=on1(T.u8)), lambda: ops.clean_components(T.lg, out=on1(T.lg)),
                             lambda: ops.clean_components(T.lg, kept=on1(T.u8))],
        "distance_gate": [lambda: ops.distance_gate(T.u8, 5, out=on1(T.u8))],
        "adapt_labels": [lambda: ops.adapt_labels(T.lg, on1(T.gt), 3.5, 4)],
        "cbce_loss_frames": [lambda: ops.cbce_loss_frames(T.lg, T.label, void=on1(T.void))],
        "png_encode": [lambda: ops.png_encode(T.u8, out=torch.zeros((N, pngc), dtype=U8, device="cuda:1")),
                       lambda: ops.png_encode(T.u8, lengths=torch.zeros((N,), dtype=I32, device="cuda:1"))],
        "merge_objects": [lambda: ops.merge_objects([T.lg, on1(T.lg)]), lambda: ops.merge_objects(T.maps, out=on1(T.u8))],
        "jf_counts_labels": [lambda: ops.jf_counts_labels(T.labels, on1(T.gt), 3)],
        "png_encode_indexed": [lambda: ops.png_encode_indexed(T.labels, palette=on1(T.pal))],
        "jpeg_encode": [lambda: ops.jpeg_encode(T.fr, out=torch.zeros((N, j3), dtype=U8, device="cuda:1")),
                        lambda: ops.jpeg_encode(T.fr, lengths=torch.zeros((N,), dtype=I32, device="cuda:1"))],
        "jpeg_decode": [lambda: ops.jpeg_decode(T.jpegs, device=DEV, status=torch.zeros((N,), dtype=I32, device="cuda:1"))],
        "frame_prep": [lambda: ops.frame_prep(T.fr, out=torch.zeros((N, 3, H, W), device="cuda:1"))],
        "overlay": [lambda: ops.overlay(T.fr, on1(T.lg)), lambda: ops.overlay(T.fr, T.lg, out=on1(T.fr))],
        "guided_coefficients": [lambda: ops.guided_coefficients(T.img, on1(T.lgs))],
        "overlay_guided": [lambda: ops.overlay_guided(T.fr, on1(T.coeff))],
        "frame_prep_window": [lambda: ops.frame_prep_window(T.fr, on1(T.win), (HN, WN))],
        "overlay_window": [lambda: ops.overlay_window(T.fr, on1(T.lgs), T.win), lambda: ops.overlay_window(T.fr, T.lgs, on1(T.win))],
        "window_next": [lambda: ops.window_next(T.lgs, on1(T.win), (H, W)), lambda: ops.window_next(T.lgs, T.win, (H, W), out=on1(T.win))],
        "overlay_objects": [lambda: ops.overlay_objects(T.fr, [T.lg, on1(T.lg)]), lambda: ops.overlay_objects(T.fr, T.maps, palette=on1(T.pal))],
    }
    return [(f"{op} #{i}", call, RuntimeError, msg(op)) for op, cs in calls.items() for i, call in enumerate(cs)]


def test_a_tensor_on_another_gpu_raises_before_any_launch():
    if torch.cuda.device_count() < 2:
        pytest.skip("one GPU is visible: the rows that put one tensor on another GPU need two")
    run_rows(other_gpu_rows(tensors()))
