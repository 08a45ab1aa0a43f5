"""The test-time ensemble on one MI355X (csrc/ensemble.hip: fosvos_ensemble_views, fosvos_ensemble_merge).  One JSON line (also
written to profiles/test_ensemble_bench.json), 480x854, for the view sets {flip} = (1, F) (1, T) and {0.75, 1, 1.25} x flip:

* first, both ops equal the numpy definition (util/test_ensemble.py) at that size, bit for bit;
* ``ops.ensemble_views`` and ``ops.ensemble_merge`` alone (HIP events after a warm-up), at one and at five frames a call;
* the host path the merge replaces: download the V float32 logit maps, ``test_ensemble.merge`` in numpy, upload the mean (wall
  clock, one host core);
* ``experiment_helper.test_fast`` over a synthetic sequence without an ensemble, with the flip and with all six views.
Three alternating rounds in one process after a warm-up; every round is reported, no threshold is asserted.
A diagnostic, not the headline metric - bench.py stays on the fine-tune.
usage: python tests/bench_test_ensemble.py [--json profiles/test_ensemble_bench.json] [--frames 10] [--reps 50]"""
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
from fosvos_hip.options import EnsembleOptions  # noqa: E402
from networks.osvos_vgg import OSVOS_VGG  # noqa: E402
from oracle import osvos_ref as O  # noqa: E402  (seeded weights only)
from util import experiment_helper, io_helper, test_ensemble  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "test_ensemble_bench.json"))
ap.add_argument("--frames", type=int, default=10)
ap.add_argument("--reps", type=int, default=50)
args = ap.parse_args()
dev = "cuda:0"
assert torch.cuda.is_available(), "bench_test_ensemble.py measures on the GPU; there is no CPU timing"
H, W = 480, 854
OPTIONS = {"flip": EnsembleOptions(flip=True), "six": EnsembleOptions(flip=True, scales=(0.75, 1.0, 1.25))}


def time_us(fn, reps):
    for _ in range(5):
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


def operands(n, views, seed=0):
    rng = np.random.default_rng(seed)
    image = (rng.standard_normal((n, 3, H, W)) * 60.0).astype(np.float32)
    maps = [(rng.standard_normal((n, 1) + test_ensemble.view_sizes(H, W, s)) * 4.0).astype(np.float32) for s, _ in views]
    return image, maps


def same(got, want):
    return np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))


def check_equality():
    """Both ops against the definition at 480x854, one frame, the six views."""
    views = OPTIONS["six"].views()
    image, maps = operands(1, views, seed=1)
    got = ops.ensemble_views(torch.from_numpy(image).to(dev), views)
    for g, want in zip(got, test_ensemble.make_views(image, views)):
        assert same(g, want), "ensemble_views differs from test_ensemble.make_views at %dx%d" % (H, W)
    merged = ops.ensemble_merge([torch.from_numpy(m).to(dev) for m in maps], views, (H, W))
    assert same(merged, test_ensemble.merge(maps, views, H, W)), "ensemble_merge differs from test_ensemble.merge"
    return True


def ops_timings(name, n):
    views = OPTIONS[name].views()
    image, maps = operands(n, views)
    image_t, maps_t = torch.from_numpy(image).to(dev), [torch.from_numpy(m).to(dev) for m in maps]
    out_views = [None if (s, f) == (1.0, False) else torch.empty((n, 3) + test_ensemble.view_sizes(H, W, s), device=dev)
                 for s, f in views]
    out = torch.empty((n, 1, H, W), device=dev)

    def make():
        ops.ensemble_views(image_t, views, out=out_views)

    def merge():
        ops.ensemble_merge(maps_t, views, (H, W), out=out)

    def host():
        down = [m.cpu().numpy() for m in maps_t]           # V float32 maps a frame over the bus
        return torch.from_numpy(test_ensemble.merge(down, views, H, W)).to(dev)

    host()  # warm-up
    rounds = []
    for _ in range(3):
        r = {"ensemble_views_us_per_frame": round(time_us(make, args.reps) / n, 2),
             "ensemble_merge_us_per_frame": round(time_us(merge, args.reps) / n, 2)}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host()
        torch.cuda.synchronize()
        r["host_merge_us_per_frame"] = round((time.perf_counter() - t0) * 1e6 / n, 1)
        rounds.append(r)
    made = sum(t.numel() for t in out_views if t is not None)
    return {"views": len(views), "frames_per_call": n, "rounds": rounds,
            "views_bytes_written_per_frame": 4 * made // n, "merge_bytes_read_per_frame": 4 * sum(m.size for m in maps) // n,
            "host_bytes_over_the_bus_per_frame": 4 * (sum(m.size for m in maps) // n + H * W)}


class Provider:
    def __init__(self, network):
        self.network = network


def forward_ms(net):
    x = torch.from_numpy(operands(1, [(1.0, False)])[0]).to(dev)
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
    runs = (("plain", None), ("flip", OPTIONS["flip"]), ("six", OPTIONS["six"]))
    with tempfile.TemporaryDirectory() as tmp:
        def run(key, ensemble):
            kw = {} if ensemble is None else {"ensemble": ensemble}
            experiment_helper.test_fast(provider, held_loader, os.path.join(tmp, key), loader.dataset.annotation, seq_name="bench",
                                        **kw)

        for key, ensemble in runs:
            run(key, ensemble)  # warm-up
        rounds = []
        for _ in range(3):
            r = {}
            for key, ensemble in runs:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run(key, ensemble)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                r[key] = {"frames_per_s": round(args.frames / dt, 1), "ms_per_frame": round(1e3 * dt / args.frames, 3)}
            rounds.append(r)
    return {"frames": args.frames, "views": {"plain": 1, "flip": 2, "six": 6}, "rounds": rounds,
            "one_forward_ms": forward_ms(provider.network)}


def main():
    result = {"bench": "test_ensemble", "device": torch.cuda.get_device_name(0), "size": "%dx%d" % (H, W),
              "equal_to_definition": check_equality(),
              "ops": {"%s_%d" % (name, n): ops_timings(name, n) for name in ("flip", "six") for n in (1, 5)},
              "pass": passes()}
    line = json.dumps(result)
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
