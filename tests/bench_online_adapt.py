"""Online adaptation on one MI355X (csrc/adapt.hip, the void form of csrc/loss.hip, experiment_helper.test_adaptive).  Four
comparisons, one JSON line (also written to profiles/online_adapt_bench.json), 480x854 with neg_distance 220 and erode 15,
three alternating rounds in one process after a warm-up:

* ``ops.adapt_labels`` (HIP events; its kernels one by one from the launch profiler) against the host path on the same
  logits: download, two ``scipy.ndimage.distance_transform_edt``, the labelling in numpy, upload (wall clock, one host core);
* the void loss ``ops.cbce_loss_frames(void=)`` beside the plain per-frame loss, one and two frames;
* ``experiment_helper.test_adaptive`` over 10 frames at 0, 1 and 3 steps a frame beside ``test_fast``;
* mean J of ``train_online.py --synthetic --score`` with and without ``--adapt-steps 1``.
Every round is reported, nothing is asserted on the figures.  A diagnostic, not the headline metric - bench.py stays on the
fine-tune.
usage: python tests/bench_online_adapt.py [--json profiles/online_adapt_bench.json] [--reps 30]"""
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

import online_adapt_cases as C  # noqa: E402
import fosvos_hip  # noqa: E402
from fosvos_hip import ops  # noqa: E402
from fosvos_hip.options import AdaptOptions  # noqa: E402
from networks.osvos_vgg import OSVOS_VGG  # noqa: E402
from oracle import osvos_ref as O  # noqa: E402  (seeded weights only)
from util import experiment_helper, io_helper  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "online_adapt_bench.json"))
ap.add_argument("--reps", type=int, default=30)
args = ap.parse_args()
dev = "cuda:0"
assert torch.cuda.is_available(), "bench_online_adapt.py measures on the GPU; there is no CPU timing"
H, W = 480, 854
D, E = 220, 15
T = C.pos_logit(0.97)


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


def host_labels(logits, last_mask):
    """What a user without the op runs between two training steps: the logits over the bus, scipy's two transforms, back."""
    from scipy import ndimage
    x = logits.cpu().numpy()[0, 0]
    m = last_mask.cpu().numpy()[0] != 0
    core = ndimage.distance_transform_edt(m) > E            # distance to the nearest clear pixel
    far = ndimage.distance_transform_edt(~core) > D if core.any() else np.zeros_like(core)
    pos = ~far & (x >= np.float32(T))
    label, void = pos.astype(np.float32), (~far & ~pos).astype(np.uint8)
    return torch.from_numpy(label).to(logits.device), torch.from_numpy(void).to(logits.device)


def label_rounds():
    x_np, m_np = C.logits_for(H, W)
    x, m = torch.from_numpy(x_np).to(dev).view(1, 1, H, W), torch.from_numpy(m_np).to(dev).view(1, H, W)
    label, void = torch.empty_like(x), torch.empty((1, 1, H, W), dtype=torch.uint8, device=dev)
    counts = torch.zeros((1, 3), dtype=torch.int32, device=dev)
    gate_out = torch.empty((1, H, W), dtype=torch.uint8, device=dev)
    rounds = []
    for _ in range(3):
        r = {"adapt_labels_us": time_us(lambda: ops.adapt_labels(x, m, T, D, E, label=label, void=void, counts=counts), args.reps),
             "adapt_labels_no_erode_us": time_us(lambda: ops.adapt_labels(x, m, T, D, 0, label=label, void=void, counts=counts),
                                                 args.reps),
             "distance_gate_220_us": time_us(lambda: ops.distance_gate(m, D, out=gate_out), args.reps)}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(3):
            host_labels(x, m)
        torch.cuda.synchronize()
        r["host_scipy_us"] = (time.perf_counter() - t0) * 1e6 / 3
        rounds.append({k: round(v, 1) for k, v in r.items()})
    with fosvos_hip.LaunchProfile(0) as prof:
        ops.adapt_labels(x, m, T, D, E, label=label, void=void, counts=counts)
        torch.cuda.synchronize()
    return {"rounds": rounds, "counts": counts.cpu().tolist()[0],
            "kernels_us_per_call": {k: round(v["ms"] * 1e3, 1) for k, v in prof.records.items()}}


def loss_rounds():
    out = {}
    for n in (1, 2):
        x, y, v = (torch.from_numpy(a).to(dev) for a in C.loss_inputs(n, H, W))
        rounds = []
        for _ in range(3):
            rounds.append({"plain_us": round(time_us(lambda: ops.cbce_loss_frames(x, y, size_average=False), args.reps), 1),
                           "void_us": round(time_us(lambda: ops.cbce_loss_frames(x, y, size_average=False, void=v), args.reps), 1)})
        out["frames_%d" % n] = rounds
    return out


class Provider:
    def __init__(self, net):
        from util.network_provider import VGGOnlineProvider
        self.inner = VGGOnlineProvider.__new__(VGGOnlineProvider)
        self.inner.network = self.network = net

    def get_optimizer(self, learning_rate=1e-8):
        return self.inner.get_optimizer(learning_rate=learning_rate)


def pass_rounds():
    net = OSVOS_VGG(pretrained=0)
    net.load_state_dict(O.make_state_dict(2))
    prov = Provider(net.to(dev))
    loader = io_helper.get_data_loader_test(None, 1, "blob", synthetic=(H, W), n_frames=10)
    train = io_helper.get_data_loader_train(None, 1, "blob", synthetic=(H, W))
    first = {"image": train.dataset[0]["image"], "gt": train.dataset[0]["gt"]}
    ann = loader.dataset.annotation
    rounds = []
    with tempfile.TemporaryDirectory() as tmp:
        for rnd in range(4):  # the first is the warm-up
            r = {}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            experiment_helper.test_fast(prov, loader, Path(tmp) / ("fast%d" % rnd), ann, seq_name="blob")
            torch.cuda.synchronize()
            r["test_fast_fps"] = round(10 / (time.perf_counter() - t0), 2)
            for steps in (0, 1, 3):
                opts = AdaptOptions(steps=steps, neg_distance=D, erode=E)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                experiment_helper.test_adaptive(prov, loader, Path(tmp) / ("adapt%d_%d" % (steps, rnd)), first, opts, ann,
                                                seq_name="blob")
                torch.cuda.synchronize()
                r["test_adaptive_steps%d_fps" % steps] = round(10 / (time.perf_counter() - t0), 2)
            if rnd:
                rounds.append(r)
    return {"frames": 10, "rounds": rounds}


def synthetic_j():
    """``train_online.py --synthetic --score`` with and without ``--adapt-steps 1``: the mean J of the four test frames."""
    import train_online
    out = {}
    here = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        try:
            os.chdir(tmp)
            for key, flags in (("plain", ["--fast-test"]), ("adapt_steps1", ["--adapt-steps", "1"])):
                torch.manual_seed(0)
                train_online.main(["--synthetic", "--n-epochs", "200", "--score"] + flags)
                out[key + "_mean_j"] = round(train_online.scored_sequences[-1]["J_stats"]["mean"], 4)
        finally:
            os.chdir(here)
    return out


def main():
    result = {"bench": "online_adapt", "device": torch.cuda.get_device_name(0), "size": "%dx%d" % (H, W),
              "neg_distance": D, "erode": E, "adapt_labels": label_rounds(), "loss": loss_rounds(), "test_pass": pass_rounds(),
              "synthetic": synthetic_j()}
    line = json.dumps(result)
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
