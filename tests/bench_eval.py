"""Scoring on one MI355X (csrc/eval.hip): microseconds per frame of ``ops.prob_bytes`` and ``ops.jf_counts`` (r = 8) on
5x480x854 and 1x480x854 logits resident on the device (HIP events after warm-up), the host's cost of the same counts
(``davis_measures.jf_counts_numpy`` and, where scipy imports, ``scipy.ndimage.binary_dilation`` - the fairer host figure),
and frames/s of the whole scored pass against ``experiment_helper.test`` on a 16-frame synthetic 480x854 sequence written to
a temporary folder (PNG encoding included in both).  A diagnostic, not the headline metric - bench.py stays on the fine-tune.
usage: python tests/bench_eval.py [--json out.json] [--reps 200]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "fosvos_amd"))

from fosvos_hip import LaunchProfile, ops  # noqa: E402
from networks.osvos_vgg import OSVOS_VGG  # noqa: E402
from oracle import osvos_ref as O  # noqa: E402  (seeded weights only)
from util import davis_measures as M, experiment_helper, io_helper  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--json", default=None)
ap.add_argument("--reps", type=int, default=200)
ap.add_argument("--hw", default="480x854")
ap.add_argument("--frames", type=int, default=16)
args = ap.parse_args()
H, W = (int(v) for v in args.hw.split("x"))
R = M.default_radius(H, W)
HBM = 6.3e12  # achievable HBM rate of the MI355X, bytes/s
dev = "cuda:0"
assert torch.cuda.is_available(), "bench_eval.py measures on the GPU; there is no CPU timing of the kernels"


def frames(n):
    loader = io_helper.get_data_loader_test(None, n, "bench", synthetic=(H, W), n_frames=n)
    batch = next(iter(loader))
    g = torch.Generator().manual_seed(3)
    # logits with the ground truth's shape plus noise: contours of a realistic length, and a full range for the bytes
    logits = (batch["gt"] * 6 - 3 + 2 * torch.randn(batch["gt"].shape, generator=g)).contiguous()
    return logits.to(dev), (batch["gt"][:, 0] >= 0.5).to(torch.uint8).to(dev)


def time_us(fn, reps):
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    best = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        best.append(e0.elapsed_time(e1) * 1e3 / reps)
    return sorted(best)


result = {"what": "eval", "hw": [H, W], "radius": R, "device": torch.cuda.get_device_name(0), "reps": args.reps}
for n in (5, 1):
    logits, gt = frames(n)
    png = torch.empty((n, H, W), dtype=torch.uint8, device=dev)
    counts = torch.empty((n, 6), dtype=torch.int32, device=dev)
    t_png = time_us(lambda: ops.prob_bytes(logits, out=png), args.reps)
    t_jf = time_us(lambda: ops.jf_counts(logits, gt, R, out=counts), args.reps)
    moved = 9 * H * W  # the logits read twice, one byte written
    torch.cuda.synchronize()
    with LaunchProfile(0) as prof:  # per-kernel event time, in a pass of its own (the brackets slow the stream down)
        for _ in range(20):
            ops.prob_bytes(logits, out=png)
            ops.jf_counts(logits, gt, R, out=counts)
    kernels = {k: v["ms"] * 1e3 / v["launches"] for k, v in prof.records.items()}
    result["n%d" % n] = {
        "prob_bytes_us_per_frame": t_png[1] / n, "prob_bytes_us_runs": [t / n for t in t_png],
        "prob_bytes_bytes_per_frame": moved, "prob_bytes_share_of_hbm": moved * n / (t_png[1] * 1e-6) / HBM,
        "jf_counts_us_per_frame": t_jf[1] / n, "jf_counts_us_runs": [t / n for t in t_jf],
        "jf_counts_bytes_per_frame": 5 * H * W, "kernel_us_per_launch": kernels}

# the host's cost of the same counts, on the cores this process is given
logits, gt = frames(1)
x, g = logits.cpu().numpy()[0, 0] >= 0, gt.cpu().numpy()[0] != 0
t0 = time.perf_counter()
want = M.jf_counts_numpy(x, g, R)
result["jf_counts_numpy_us_per_frame"] = (time.perf_counter() - t0) * 1e6
assert np.array_equal(ops.jf_counts(logits, gt, R).cpu().numpy()[0], want)
try:
    from scipy import ndimage
    yy, xx = np.mgrid[-R:R + 1, -R:R + 1]
    disk = yy * yy + xx * xx <= R * R
    t0 = time.perf_counter()
    ba, bb = M.boundary_map(x), M.boundary_map(g)
    got = [(x & g).sum(), (x | g).sum(), ba.sum(), bb.sum(), (ba & ndimage.binary_dilation(bb, structure=disk)).sum(),
           (bb & ndimage.binary_dilation(ba, structure=disk)).sum()]
    result["jf_counts_scipy_us_per_frame"] = (time.perf_counter() - t0) * 1e6
    assert list(want) == [int(v) for v in got]
except ImportError:
    result["jf_counts_scipy_us_per_frame"] = None


# the whole pass: test() against test_scored() on the same loader, alternating, three repetitions each
class Provider:
    pass


prov = Provider()
net = OSVOS_VGG(pretrained=0)
net.load_state_dict(O.make_state_dict(9))
prov.network = net.to(dev)
loader = io_helper.get_data_loader_test(None, 1, "bench", synthetic=(H, W), n_frames=args.frames)
fps = {"test": [], "test_scored": []}
with tempfile.TemporaryDirectory() as tmp:
    for rep in range(4):  # repetition 0 warms both up
        for name in ("test", "test_scored"):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if name == "test":
                experiment_helper.test(prov, loader, os.path.join(tmp, name), False, False, seq_name="bench")
            else:
                experiment_helper.test_scored(prov, loader, os.path.join(tmp, name), loader.dataset.annotation,
                                              seq_name="bench")
            torch.cuda.synchronize()
            if rep:
                fps[name].append(args.frames / (time.perf_counter() - t0))
result["pass_frames"] = args.frames
result["test_fps_runs"], result["test_scored_fps_runs"] = fps["test"], fps["test_scored"]
result["test_fps"], result["test_scored_fps"] = sorted(fps["test"])[1], sorted(fps["test_scored"])[1]
result["test_fps_spread"] = (max(fps["test"]) - min(fps["test"])) / result["test_fps"]
line = json.dumps(result)
print(line)
if args.json:
    with open(args.json, "w") as f:
        f.write(line + "\n")
