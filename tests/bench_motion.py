"""Block matching and the mask warp on one MI355X (csrc/motion.hip).  One JSON line (also written to
profiles/motion_bench.json), 480x854:

* first, ``ops.motion_luma``, ``ops.motion_estimate`` (block 8 and 16, search 8 and 16) and ``ops.motion_warp`` equal the numpy
  definition (util/block_motion.py) at that size, exactly;
* each of the three ops alone (HIP events after a warm-up) at one frame and at five frames a call, block 8 and 16, search 8 and
  16;
* the host path ``motion_estimate`` replaces on the same operands: download the two planes, the vectorised numpy definition,
  upload the field (wall clock, one host core; at one pair a call - the host's work is per pair);
* ``experiment_helper.test_fast`` over a synthetic sequence with ``clean`` alone and with ``clean + motion`` (the defaults);
* ``FrameSegmenter.segment`` over 64 frames with ``clean`` alone and with ``clean + motion``.
Three alternating rounds in one process after a warm-up; every round is reported, no threshold is asserted.
A diagnostic, not the headline metric - bench.py stays on the fine-tune.
usage: python tests/bench_motion.py [--json profiles/motion_bench.json] [--frames 10] [--stream-frames 64] [--reps 20]"""
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
from fosvos_hip.options import CleanOptions, MotionOptions  # noqa: E402
from fosvos_hip.stream import FrameSegmenter  # noqa: E402
from networks.osvos_vgg import OSVOS_VGG  # noqa: E402
from oracle import osvos_ref as O  # noqa: E402  (seeded weights only)
from util import block_motion, experiment_helper, io_helper  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "motion_bench.json"))
ap.add_argument("--frames", type=int, default=10)
ap.add_argument("--stream-frames", type=int, default=64)
ap.add_argument("--reps", type=int, default=20)
args = ap.parse_args()
dev = "cuda:0"
assert torch.cuda.is_available(), "bench_motion.py measures on the GPU; there is no CPU timing"
H, W = 480, 854
CONFIGS = [(b, s) for b in (8, 16) for s in (8, 16)]


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
    """(image float32 [n,3,H,W] of random bytes as the net sees them, prev and cur planes uint8 [n,H,W] - a random scene that
    moved by (3, -5) -, masks uint8 [n,H,W])."""
    from dataloaders.davis_2016 import MEANVAL
    rng = np.random.default_rng(seed)
    frames = rng.integers(0, 256, (n, 3, H, W)).astype(np.float32)
    image = np.ascontiguousarray(frames - np.array(MEANVAL, dtype=np.float32)[None, :, None, None])
    big = rng.integers(0, 256, (n, H + 16, W + 16), dtype=np.uint8)
    prev, cur = np.ascontiguousarray(big[:, 8:8 + H, 8:8 + W]), np.ascontiguousarray(big[:, 11:11 + H, 3:3 + W])
    mask = (rng.random((n, H, W)) < 0.3).astype(np.uint8)
    return image, prev, cur, mask


def check_equality():
    image, prev, cur, mask = operands(1, seed=1)
    assert np.array_equal(ops.motion_luma(torch.from_numpy(image).to(dev)).cpu().numpy(), block_motion.luma(image)), "motion_luma"
    prev_t, cur_t, mask_t = (torch.from_numpy(a).to(dev) for a in (prev, cur, mask))
    for block, search in CONFIGS:
        o = MotionOptions(block=block, search=search)
        field, cost = ops.motion_estimate(prev_t, cur_t, o)
        want_f, want_c = block_motion.estimate(prev, cur, options=o)
        assert np.array_equal(field.cpu().numpy(), want_f) and np.array_equal(cost.cpu().numpy(), want_c), \
            "motion_estimate differs from block_motion.estimate at %dx%d, block %d search %d" % (H, W, block, search)
        got = ops.motion_warp(mask_t, field, block).cpu().numpy()
        assert np.array_equal(got[0], block_motion.warp(mask[0], want_f[0], block)), "motion_warp"
    return True


def op_timings():
    on_device = {n: tuple(torch.from_numpy(a).to(dev) for a in operands(n)) for n in (1, 5)}
    rounds = []
    for _ in range(3):
        r_ = {}
        for n in (1, 5):
            image_t, prev_t, cur_t, mask_t = on_device[n]
            y = torch.empty((n, H, W), dtype=torch.uint8, device=dev)
            r_["luma_n%d" % n] = {"us_per_frame": round(time_us(lambda: ops.motion_luma(image_t, out=y), args.reps) / n, 2)}
            for block, search in CONFIGS:
                o = MotionOptions(block=block, search=search)
                field, cost = ops.motion_estimate(prev_t, cur_t, o)
                us = time_us(lambda: ops.motion_estimate(prev_t, cur_t, o, field=field, cost=cost), args.reps)
                entry = {"estimate_us_per_pair": round(us / n, 2)}
                if n == 1:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    torch.from_numpy(block_motion.estimate(prev_t.cpu().numpy(), cur_t.cpu().numpy(), options=o)[0]).to(dev)
                    torch.cuda.synchronize()
                    entry["host_us_per_pair"] = round((time.perf_counter() - t0) * 1e6, 1)
                if search == 8:
                    out = torch.empty((n, H, W), dtype=torch.uint8, device=dev)
                    entry["warp_us_per_frame"] = round(time_us(lambda: ops.motion_warp(mask_t, field, block, out=out), args.reps) / n, 2)
                r_["b%d_s%d_n%d" % (block, search, n)] = entry
        rounds.append(r_)
    return {"rounds": rounds, "sad_operations_per_pixel": {"s8": 289, "s16": 1089}}


class Provider:
    def __init__(self, network):
        self.network = network


def seeded_net():
    net = OSVOS_VGG(pretrained=0)
    net.load_state_dict(O.make_state_dict(2))
    return net.to(dev).eval()


def alternating(runs, run, frames):
    for key, kw in runs:
        run(key, kw)  # warm-up
    rounds = []
    for _ in range(3):
        r = {}
        for key, kw in runs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(key, kw)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            r[key] = {"frames_per_s": round(frames / dt, 1), "ms_per_frame": round(1e3 * dt / frames, 3)}
        rounds.append(r)
    return rounds


def passes(net):
    provider = Provider(net)
    loader = io_helper.get_data_loader_test(None, 1, "bench", synthetic=(H, W), n_frames=args.frames)
    from torch.utils.data import DataLoader
    held = [loader.dataset[f] for f in range(args.frames)]  # the frames are generated once: the loader below only collates them
    held_loader = DataLoader(held, batch_size=1, shuffle=False, num_workers=0)
    clean = CleanOptions(temporal_radius=8)
    seed = loader.dataset.annotation("bench", "00000")
    runs = (("clean", {}), ("clean_motion", {"motion": MotionOptions()}))
    with tempfile.TemporaryDirectory() as tmp:
        def run(key, kw):
            experiment_helper.test_fast(provider, held_loader, os.path.join(tmp, key), loader.dataset.annotation, seq_name="bench",
                                        clean=clean, clean_seed=seed, **kw)
        rounds = alternating(runs, run, args.frames)
    return {"frames": args.frames, "clean": clean.as_dict(), "motion": MotionOptions().as_dict(), "rounds": rounds}


def stream(net):
    rng = np.random.default_rng(5)
    frames = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(8)]
    clean = CleanOptions(temporal_radius=8)
    runs = (("clean", {}), ("clean_motion", {"motion": MotionOptions()}))

    def run(key, kw):
        with FrameSegmenter(net, H, W, depth=2, clean=clean, **kw) as seg:
            for _ in seg.segment(frames[k % len(frames)] for k in range(args.stream_frames)):
                pass
    return {"frames": args.stream_frames, "depth": 2, "rounds": alternating(runs, run, args.stream_frames)}


def main():
    net = seeded_net()
    result = {"bench": "motion", "device": torch.cuda.get_device_name(0), "size": "%dx%d" % (H, W),
              "equal_to_definition": check_equality(), "ops": op_timings(), "pass": passes(net), "stream": stream(net)}
    line = json.dumps(result)
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
