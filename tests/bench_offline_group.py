"""The offline loop's batched accumulation cycle against the one-by-one loop on one MI355X: ``train_offline._train`` at
480x854 on resident synthetic one-frame minibatches, avg_grad_every_n = 10, at ``microbatch_group`` 1 and 5 in alternating
pairs, (a) with one of the reference's scales {1, 0.8, 0.5} drawn per iteration from a fixed seed
(src/dataloaders/custom_transforms.py:63-93) and (b) at one size.  Reports frames/s of every pair, passes per cycle and the
loss-kernel launches per frame from the launch profiler.  Prints ONE JSON line and writes it to
profiles/offline_group_bench.json.

    python tests/bench_offline_group.py [--pairs 3] [--iters 120] [--epochs 4]

Timing: a warm-up call of each leg first (every shape and batch size allocates its arena once), then a host clock around
whole `_train` calls, which end in a device synchronise."""
import argparse
import json
import os
import random
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "fosvos_amd"))

from oracle import osvos_ref as O  # noqa: E402

DEV = "cuda:0"
H, W = 480, 854
ACCUM = 10
GROUPS = (1, 5)
LOSS_KERNELS = ("k_count", "k_loss", "k_loss_multi", "k_finish")


class _NullWriter:
    def add_scalar(self, *a, **k):
        pass

    def close(self):
        pass


def _round_half_even(v):
    return int(round(v))  # (Python rounds halves to even, like cvRound)


def minibatches(scales, iters, seed=4321, per_size=4):
    """`iters` resident one-frame minibatches: a scale drawn per iteration, one of `per_size` frames of that size."""
    rng = random.Random(seed)
    pool = {}
    for k, sc in enumerate(scales):
        h, w = _round_half_even(H * sc), _round_half_even(W * sc)
        frames = [O.synthetic_frame(1, h, w, seed=seed + 10 * k + i) for i in range(per_size)]
        pool[sc] = [{"image": x.to(DEV), "gt": gt.to(DEV)} for x, gt in frames]
    draws = [scales[rng.randint(0, len(scales) - 1)] for _ in range(iters)]
    return [pool[sc][i % per_size] for i, sc in enumerate(draws)], draws


def run_config(scales, args):
    import fosvos_hip
    import train_offline
    from networks.osvos_vgg import OSVOS_VGG
    from util.network_provider import VGGOfflineProvider
    net = OSVOS_VGG(pretrained=0)
    net.load_state_dict(O.make_state_dict(2))
    prov = VGGOfflineProvider.__new__(VGGOfflineProvider)
    prov.network = net.to(DEV)
    prov.name = "vgg16"
    opt = prov.get_optimizer()
    loader, draws = minibatches(scales, args.iters)
    train_offline.data_parallel = False
    epoch = [0]

    def run(group, n_epochs):
        first, epoch[0] = epoch[0], epoch[0] + n_epochs
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ret = train_offline._train(prov, loader, None, opt, _NullWriter(), first, first + n_epochs, ACCUM, 10 ** 9, False, 5,
                                   microbatch_group=group)
        torch.cuda.synchronize()
        ret["wall"] = time.perf_counter() - t0
        return ret

    for group in GROUPS:
        run(group, 1)
    pairs, passes = [], {}
    for _ in range(args.pairs):
        fps = {}
        for group in GROUPS:
            ret = run(group, args.epochs)
            fps[str(group)] = ret["iterations"] / ret["wall"]
            passes[str(group)] = ret["passes"] / (ret["iterations"] / ACCUM)
        pairs.append(fps)
    launches = {}
    for group in GROUPS:
        with fosvos_hip.LaunchProfile(0) as prof:
            ret = run(group, 1)
        launches[str(group)] = {k: prof.records[k]["launches"] / ret["iterations"] for k in LOSS_KERNELS if k in prof.records}
        launches[str(group)]["all_loss_kernels"] = sum(launches[str(group)].values())
    ratios = [p["5"] / p["1"] for p in pairs]
    return {"scales": list(scales), "draws_per_epoch": args.iters, "epochs_per_leg": args.epochs,
            "frames_by_scale": {str(sc): draws.count(sc) for sc in scales}, "pairs_fps": pairs,
            "group5_over_group1": ratios, "group5_wins_every_pair": all(r > 1.0 for r in ratios),
            "passes_per_cycle": passes, "loss_launches_per_frame": launches}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--iters", type=int, default=120, help="one-frame minibatches per epoch")
    ap.add_argument("--epochs", type=int, default=4, help="epochs per timed leg")
    args = ap.parse_args()
    result = {"bench": "offline_group", "device": torch.cuda.get_device_name(0), "size": [H, W], "avg_grad_every_n": ACCUM,
              "groups": list(GROUPS), "unit": "frames/s",
              "mixed_scales": run_config((1, 0.8, 0.5), args), "one_size": run_config((1,), args)}
    line = json.dumps(result)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "offline_group_bench.json"), "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
