"""Cleaning a mask by its shape on one MI355X (csrc/components.hip: fosvos_clean_components).  Three comparisons, one JSON line
(also written to profiles/components_bench.json), 480x854, three alternating rounds in one process after a warm-up:

* ``ops.clean_components`` alone (HIP events), at one and five frames a call, with ``min_area`` + ``largest`` and with the
  temporal gate as well, on three inputs - (i) a net-like map, one large blob plus about 30 small ones, (ii) the worst case for
  the union-find, a one-pixel serpentine through the whole frame, (iii) an 8-connected checkerboard - against the host path
  on the same logits: download, ``scipy.ndimage.label`` with the 3x3 structure, ``numpy.bincount``, re-upload (wall clock, one
  host core);
* ``FrameSegmenter.segment`` over 64 frames with and without ``clean``;
* ``experiment_helper.test_fast`` over 10 frames with and without ``clean``.
Every round is reported, nothing is asserted on the figures.  A diagnostic, not the headline metric - bench.py stays on the
fine-tune.
usage: python tests/bench_components.py [--json profiles/components_bench.json] [--reps 30]"""
import argparse
import json
import os
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "fosvos_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mask_component_cases as C  # noqa: E402
from fosvos_hip import ops  # noqa: E402
from fosvos_hip.options import CleanOptions  # noqa: E402
from networks.osvos_vgg import OSVOS_VGG  # noqa: E402
from oracle import osvos_ref as O  # noqa: E402  (seeded weights only)
from util import experiment_helper, io_helper  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "components_bench.json"))
ap.add_argument("--reps", type=int, default=30)
args = ap.parse_args()
dev = "cuda:0"
assert torch.cuda.is_available(), "bench_components.py measures on the GPU; there is no CPU timing"
H, W = 480, 854


def net_like(index=0):
    """One large ellipse with a noisy rim plus about 30 small stray blobs."""
    rng = np.random.default_rng(index)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    d = ((yy - H * 0.5) / (H * 0.3)) ** 2 + ((xx - W * (0.45 + 0.01 * index)) / (W * 0.22)) ** 2
    x = (1.0 - d) * 6.0 + rng.normal(0.0, 0.6, (H, W))
    x = np.minimum(x, np.where(d > 1.6, -3.0, np.inf))
    for _ in range(30):
        cy, cx, r = rng.integers(8, H - 8), rng.integers(8, W - 8), rng.integers(2, 7)
        if ((cy - H * 0.5) / (H * 0.3)) ** 2 + ((cx - W * 0.45) / (W * 0.22)) ** 2 > 2.2:
            x[cy - r:cy + r, cx - r:cx + r] = 2.0
    return x.astype(np.float32)


def time_us(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def host_path(logits, min_area):
    """What a user without the op runs: the map over the bus, scipy's labelling, the areas, the largest kept, back."""
    from scipy import ndimage
    x = logits.cpu().numpy()
    for f in range(x.shape[0]):
        labels, count = ndimage.label(x[f, 0] >= 0, np.ones((3, 3)))
        area = np.bincount(labels.ravel(), minlength=count + 1)
        area[0] = 0
        keep = np.zeros(count + 1, bool)
        if count and area.max() >= min_area:
            keep[int(np.argmax(area))] = True
        x[f, 0][(labels > 0) & ~keep[labels]] = -100.0
    return torch.from_numpy(x).to(logits.device)


def op_rounds():
    inputs = {"net_like": lambda f: net_like(f), "serpentine": lambda f: C.mask_logits(C.serpentine(H, W)),
              "checkerboard": lambda f: C.mask_logits(C.checkerboard(H, W))}
    out = {}
    for name, make in inputs.items():
        for n in (1, 5):
            x = torch.from_numpy(np.stack([make(f) for f in range(n)])).to(dev).view(n, 1, H, W)
            seed = (x[:1, 0] >= 0).to(torch.uint8).contiguous()
            dst, kept = torch.empty_like(x), torch.empty((n, H, W), dtype=torch.uint8, device=dev)
            rounds = []
            for _ in range(3):
                r = {"largest_us": time_us(lambda: ops.clean_components(x, None, 0, 50, True, out=dst), args.reps),
                     "gated_chain_r8_us": time_us(lambda: ops.clean_components(x, seed, 8, 50, True, chain=True, out=dst,
                                                                               kept=kept), args.reps),
                     "roots_only_us": time_us(lambda: ops.component_roots(x), args.reps)}
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(3):
                    host_path(x, 50)
                torch.cuda.synchronize()
                r["host_scipy_us"] = (time.perf_counter() - t0) * 1e6 / 3
                rounds.append({k: round(v / n, 1) for k, v in r.items()})
            with ops_profile() as prof:
                ops.clean_components(x, seed, 8, 50, True, chain=True, out=dst, kept=kept)
                torch.cuda.synchronize()
            out["%s_x%d" % (name, n)] = {"per_frame": rounds,
                                         "kernels_us_per_call": {k: round(v["ms"] * 1e3, 1) for k, v in prof.records.items()}}
    return out


def ops_profile():
    import fosvos_hip
    return fosvos_hip.LaunchProfile(0)


class Provider:
    def __init__(self, network):
        self.network = network


def small_vgg():
    net = OSVOS_VGG(pretrained=0)
    net.load_state_dict(O.make_state_dict(2))
    return net.to(dev).eval()


def stream_rounds(net):
    from fosvos_hip.stream import FrameSegmenter
    import run_webcam
    frames = [run_webcam.synthetic_frame(H, W, k) for k in range(64)]
    opts = CleanOptions(min_area=50, largest=True, temporal_radius=8)
    rounds = []
    for rnd in range(4):  # the first is the warm-up
        r = {}
        for key, clean in (("plain", None), ("clean", opts)):
            with FrameSegmenter(net, H, W, depth=2, clean=clean) as seg:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in seg.segment(iter(frames)):
                    pass
                torch.cuda.synchronize()
                r[key + "_ms_per_frame"] = round((time.perf_counter() - t0) * 1e3 / len(frames), 3)
        if rnd:
            rounds.append(r)
    return {"frames": len(frames), "options": opts.as_dict(), "rounds": rounds}


def pass_rounds(net):
    prov = Provider(net)
    opts = CleanOptions(min_area=50, largest=True, temporal_radius=8)
    rounds = []
    with tempfile.TemporaryDirectory() as tmp:
        loader = io_helper.get_data_loader_test(None, 1, "blob", synthetic=(H, W), n_frames=10)
        ann = loader.dataset.annotation
        seed = ann("blob", "00000")
        for rnd in range(4):  # the first is the warm-up
            r = {}
            for key, kw in (("plain", {}), ("clean", dict(clean=opts, clean_seed=seed))):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                experiment_helper.test_fast(prov, loader, Path(tmp) / ("%s%d" % (key, rnd)), ann, seq_name="blob", **kw)
                torch.cuda.synchronize()
                r[key + "_ms_per_frame"] = round((time.perf_counter() - t0) * 1e3 / 10, 3)
            if rnd:
                rounds.append(r)
    return {"frames": 10, "options": opts.as_dict(), "rounds": rounds}


def main():
    net = small_vgg()
    result = {"bench": "components", "device": torch.cuda.get_device_name(0), "size": "%dx%d" % (H, W), "ops": op_rounds(),
              "stream": stream_rounds(net), "test_fast": pass_rounds(net)}
    line = json.dumps(result)
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
