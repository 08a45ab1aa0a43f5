"""The joint CRF over the objects of a frame on one MI355X (csrc/crf.hip: fosvos_crf_labels).  One JSON line (also written to
profiles/crf_labels_bench.json), 480x854, default options:

* first, ``ops.crf_labels`` equals the numpy definition (util/label_crf.py) at that size for K = 3: the labels, and the scores
  bit for bit;
* ``ops.crf_labels`` alone (HIP events after a warm-up) at K = 1, 3, 8, five frames a call and one;
* the path it replaces on the same operands, measured alone: K x ``ops.crf_refine`` + ``ops.merge_objects``;
* ``experiment_helper.test_objects`` over a synthetic sequence of three objects with ``crf`` per net against ``crf_joint``.
Three alternating rounds in one process after a warm-up; every round is reported, no threshold is asserted.
A diagnostic, not the headline metric - bench.py stays on the fine-tune.
usage: python tests/bench_crf_labels.py [--json profiles/crf_labels_bench.json] [--frames 10] [--reps 10]"""
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
from util import experiment_helper, label_crf  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "crf_labels_bench.json"))
ap.add_argument("--frames", type=int, default=10)
ap.add_argument("--reps", type=int, default=10)
args = ap.parse_args()
dev = "cuda:0"
assert torch.cuda.is_available(), "bench_crf_labels.py measures on the GPU; there is no CPU timing"
H, W = 480, 854
KS = (1, 3, 8)


def time_us(fn, reps):
    for _ in range(2):
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


def operands(n, k, seed=0):
    """Frames of random bytes as the net sees them, and K logit maps of sigma 3."""
    from dataloaders.davis_2016 import MEANVAL
    rng = np.random.default_rng(seed)
    frames = rng.integers(0, 256, (n, 3, H, W)).astype(np.float32)
    image = np.ascontiguousarray(frames - np.array(MEANVAL, dtype=np.float32)[None, :, None, None])
    return image, [(3.0 * rng.standard_normal((n, 1, H, W))).astype(np.float32) for _ in range(k)]


def check_equality():
    image, logits = operands(1, 3, seed=1)
    scores = torch.empty((1, 4, H, W), device=dev)
    got = ops.crf_labels(torch.from_numpy(image).to(dev), [torch.from_numpy(x).to(dev) for x in logits], CrfOptions(), scores=scores)
    want_labels, want_scores = label_crf.refine_labels_batch(image, logits, CrfOptions())
    assert np.array_equal(got.cpu().numpy(), want_labels), "crf_labels' labels differ from label_crf at %dx%d" % (H, W)
    assert np.array_equal(scores.cpu().numpy().view(np.uint32), want_scores.view(np.uint32)), "crf_labels' scores differ from label_crf"
    return True


def op_timings():
    options = CrfOptions()
    held = {}
    for n in (5, 1):
        image, logits = operands(n, max(KS))
        held[n] = (torch.from_numpy(image).to(dev), [torch.from_numpy(x).to(dev) for x in logits],
                   torch.empty((n, H, W), dtype=torch.uint8, device=dev))

    def per_net(image_t, logits_t, labels):
        # what test_objects(crf=) launches: every net's logits refined into a new tensor, then the merge
        ops.merge_objects([ops.crf_refine(image_t, x, options) for x in logits_t], out=labels)

    rounds = []
    for _ in range(3):
        r_ = {}
        for n in (5, 1):
            image_t, logits_t, labels = held[n]
            for k in KS:
                maps = logits_t[:k]
                joint = time_us(lambda: ops.crf_labels(image_t, maps, options, out=labels), args.reps)
                parent = time_us(lambda: per_net(image_t, maps, labels), args.reps)
                r_["K%d_n%d" % (k, n)] = {"crf_labels_us_per_frame": round(joint / n, 2),
                                          "per_net_refine_and_merge_us_per_frame": round(parent / n, 2),
                                          "launches": {"crf_labels": options.iterations, "per_net": k * options.iterations + 1}}
        rounds.append(r_)
    return {"options": options.as_dict(), "rounds": rounds,
            "workspace_bytes_n5": {"K%d" % k: 16 * (k + 1) * 5 * H * W for k in KS}}


class Provider:
    def __init__(self, network):
        self.network = network


def passes():
    from dataloaders.synthetic import SyntheticObjectsSequence
    from torch.utils.data import DataLoader
    providers = []
    for seed in (2, 3, 4):
        net = OSVOS_VGG(pretrained=0)
        net.load_state_dict(O.make_state_dict(seed))
        providers.append(Provider(net.to(dev).eval()))
    data = SyntheticObjectsSequence("bench", H, W, n_frames=args.frames, n_objects=3)
    held = [data[f] for f in range(args.frames)]  # the frames are generated once: the loader below only collates them
    held_loader = DataLoader(held, batch_size=1, shuffle=False, num_workers=0)
    crf = CrfOptions()
    runs = (("plain", {}), ("crf_per_net", {"crf": crf}), ("crf_joint", {"crf": crf, "crf_joint": True}))
    with tempfile.TemporaryDirectory() as tmp:
        def run(key, kw):
            return experiment_helper.test_objects(providers, held_loader, os.path.join(tmp, key), data.annotation, seq_name="bench", **kw)

        for key, kw in runs:
            run(key, kw)  # warm-up
        rounds = []
        for _ in range(3):
            r = {}
            for key, kw in runs:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                score = run(key, kw)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                r[key] = {"frames_per_s": round(args.frames / dt, 1), "ms_per_frame": round(1e3 * dt / args.frames, 3),
                          "J&F": round(score["J&F"], 4)}
            rounds.append(r)
    return {"frames": args.frames, "objects": 3, "crf": crf.as_dict(), "rounds": rounds}


def main():
    result = {"bench": "crf_labels", "device": torch.cuda.get_device_name(0), "size": "%dx%d" % (H, W),
              "equal_to_definition": check_equality(), "ops": op_timings(), "pass": passes()}
    line = json.dumps(result)
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
