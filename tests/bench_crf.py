"""The CRF on the frame on one MI355X (csrc/crf.hip: fosvos_crf_refine).  One JSON line (also written to
profiles/crf_bench.json), 480x854:

* first, ``ops.crf_refine`` equals the numpy definition (util/mask_crf.py) at that size with the default options, bit for bit;
* ``ops.crf_refine`` alone (HIP events after a warm-up) at radius 3 and 5, 1 and 5 iterations, one and five frames a call;
* the host path it replaces on the same operands: download the frames and the logits, ``mask_crf.refine`` in numpy, upload the
  result (wall clock, one host core; at one frame a call - the host's work is per frame);
* one forward pass of the net beside it;
* ``experiment_helper.test_fast`` over a synthetic sequence without and with ``crf`` (the defaults).
Three alternating rounds in one process after a warm-up; every round is reported, no threshold is asserted.
A diagnostic, not the headline metric - bench.py stays on the fine-tune.
usage: python tests/bench_crf.py [--json profiles/crf_bench.json] [--frames 10] [--reps 20]"""
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

from fosvos_hip import ops  # noqa: E402
from fosvos_hip.options import CrfOptions  # noqa: E402
from networks.osvos_vgg import OSVOS_VGG  # noqa: E402
from oracle import osvos_ref as O  # noqa: E402  (seeded weights only)
from util import experiment_helper, io_helper, mask_crf  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "crf_bench.json"))
ap.add_argument("--frames", type=int, default=10)
ap.add_argument("--reps", type=int, default=20)
args = ap.parse_args()
dev = "cuda:0"
assert torch.cuda.is_available(), "bench_crf.py measures on the GPU; there is no CPU timing"
H, W = 480, 854


def time_us(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    runs = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        runs.append(e0.elapsed_time(e1) * 1e3 / reps)
    return sorted(runs)[1]  # the median of three


def operands(n, seed=0):
    """Frames of random bytes as the net sees them, and logits of sigma 3."""
    from dataloaders.davis_2016 import MEANVAL
    rng = np.random.default_rng(seed)
    frames = rng.integers(0, 256, (n, 3, H, W)).astype(np.float32)
    image = np.ascontiguousarray(frames - np.array(MEANVAL, dtype=np.float32)[None, :, None, None])
    return image, (3.0 * rng.standard_normal((n, 1, H, W))).astype(np.float32)


def check_equality():
    image, logits = operands(1, seed=1)
    got = ops.crf_refine(torch.from_numpy(image).to(dev), torch.from_numpy(logits).to(dev), CrfOptions()).cpu().numpy()
    want = mask_crf.refine_batch(image, logits, CrfOptions())
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "crf_refine differs from mask_crf.refine at %dx%d" % (H, W)
    return True


def op_timings():
    configs = [(r, t, n) for r in (3, 5) for t in (1, 5) for n in (1, 5)]
    held = {n: operands(n) for n in (1, 5)}
    on_device = {n: (torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev), torch.empty((n, 1, H, W), device=dev))
                 for n, (a, b) in held.items()}

    def host(options):
        image_t, logits_t, _ = on_device[1]
        return torch.from_numpy(mask_crf.refine_batch(image_t.cpu().numpy(), logits_t.cpu().numpy(), options)).to(dev)

    rounds = []
    for _ in range(3):
        r_ = {}
        for r, t, n in configs:
            options = CrfOptions(radius=r, iterations=t)
            image_t, logits_t, out = on_device[n]
            us = time_us(lambda: ops.crf_refine(image_t, logits_t, options, out=out), args.reps)
            entry = {"crf_refine_us_per_frame": round(us / n, 2), "us_per_launch": round(us / t, 2)}
            if n == 1:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                host(options)
                torch.cuda.synchronize()
                entry["host_us_per_frame"] = round((time.perf_counter() - t0) * 1e6, 1)
            r_["r%d_T%d_n%d" % (r, t, n)] = entry
        rounds.append(r_)
    return {"rounds": rounds, "fp64_operations_per_pixel_and_launch": {"r3": 9 * 48, "r5": 9 * 120},
            "host_bytes_over_the_bus_per_frame": 4 * (3 + 1 + 1) * H * W}


class Provider:
    def __init__(self, network):
        self.network = network


def forward_ms(net):
    x = torch.from_numpy(operands(1)[0]).to(dev)
    with torch.no_grad():
        return round(time_us(lambda: net.forward(x), 20) / 1e3, 3)


def passes():
    net = OSVOS_VGG(pretrained=0)
    net.load_state_dict(O.make_state_dict(2))
    provider = Provider(net.to(dev).eval())
    loader = io_helper.get_data_loader_test(None, 1, "bench", synthetic=(H, W), n_frames=args.frames)
    from torch.utils.data import DataLoader
    held = [loader.dataset[f] for f in range(args.frames)]  # the frames are generated once: the loader below only collates them
    held_loader = DataLoader(held, batch_size=1, shuffle=False, num_workers=0)
    runs = (("plain", None), ("crf", CrfOptions()))
    with tempfile.TemporaryDirectory() as tmp:
        def run(key, crf):
            kw = {} if crf is None else {"crf": crf}
            experiment_helper.test_fast(provider, held_loader, os.path.join(tmp, key), loader.dataset.annotation, seq_name="bench", **kw)

        for key, crf in runs:
            run(key, crf)  # warm-up
        rounds = []
        for _ in range(3):
            r = {}
            for key, crf in runs:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run(key, crf)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                r[key] = {"frames_per_s": round(args.frames / dt, 1), "ms_per_frame": round(1e3 * dt / args.frames, 3)}
            rounds.append(r)
    return {"frames": args.frames, "crf": CrfOptions().as_dict(), "rounds": rounds, "one_forward_ms": forward_ms(provider.network)}


def main():
    result = {"bench": "crf", "device": torch.cuda.get_device_name(0), "size": "%dx%d" % (H, W),
              "equal_to_definition": check_equality(), "ops": op_timings(), "pass": passes()}
    line = json.dumps(result)
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
