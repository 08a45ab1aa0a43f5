"""Streaming inference with the net at a size of its own on one MI355X (csrc/stream.hip: k_frame_prep_scaled, k_overlay_scaled;
``FrameSegmenter(net_size=)``).  Two measurements, one JSON line:

* the loop: ``FrameSegmenter.segment`` at depth 2 over the same frames with ``net_size`` against the same segmenter without
  it (the net at the frame's size) - VGG on 1080x1920 frames with the net at 480x854, ResNet-18 on 2160x3840 frames with
  the net at 1080x1920; seeded weights, frames pre-generated in host memory, three alternating rounds after a warm-up;
  frames/s and ms per frame of each, and whether the scaled loop is ahead in every pair;
* the kernels alone, microseconds per frame from HIP events after a warm-up: ``ops.frame_prep`` scaled 1080x1920 -> 480x854
  beside the unscaled op on the same frames, ``ops.overlay`` (boolean and soft, mirrored) scaled beside unscaled at 1080x1920.
A diagnostic, not the headline metric - bench.py stays on the fine-tune.
usage: python tests/bench_stream_scale.py [--json out.json] [--frames 64] [--reps 100]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "fosvos_amd"))

from fosvos_hip import ops  # noqa: E402
from fosvos_hip.stream import FrameSegmenter  # noqa: E402
from networks.osvos_resnet import OSVOS_RESNET  # noqa: E402
from networks.osvos_vgg import OSVOS_VGG  # noqa: E402
from oracle import osvos_ref as O  # noqa: E402  (seeded weights only)

ap = argparse.ArgumentParser()
ap.add_argument("--json", default=None)
ap.add_argument("--frames", type=int, default=64)
ap.add_argument("--reps", type=int, default=100)
args = ap.parse_args()
dev = "cuda:0"
assert torch.cuda.is_available(), "bench_stream_scale.py measures on the GPU; there is no CPU timing"


def time_us(fn, reps):
    for _ in range(10):
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


def kernels():
    out = {}
    g = torch.Generator().manual_seed(1)
    (hf, wf), size = (1080, 1920), (480, 854)
    for n in (1, 5):
        frames = torch.randint(0, 256, (n, hf, wf, 3), generator=g, dtype=torch.uint8).to(dev)
        logits = (3 * torch.randn((n, 1, hf, wf), generator=g)).to(dev)
        small = (3 * torch.randn((n, 1) + size, generator=g)).to(dev)
        image = torch.empty((n, 3, hf, wf), device=dev)
        image_small = torch.empty((n, 3) + size, device=dev)
        shown = torch.empty((n, hf, wf, 3), dtype=torch.uint8, device=dev)
        for name, fn in (
                ("frame_prep", lambda: ops.frame_prep(frames, True, out=image)),
                ("frame_prep_scaled", lambda: ops.frame_prep(frames, True, out=image_small, net_size=size)),
                ("overlay_boolean", lambda: ops.overlay(frames, logits, True, True, "r", 1.0, out=shown)),
                ("overlay_boolean_scaled", lambda: ops.overlay(frames, small, True, True, "r", 1.0, out=shown, net_size=size)),
                ("overlay_soft", lambda: ops.overlay(frames, logits, True, False, "r", 1.0, out=shown)),
                ("overlay_soft_scaled", lambda: ops.overlay(frames, small, True, False, "r", 1.0, out=shown, net_size=size))):
            out["%s_%dx%dx%d" % (name, n, hf, wf)] = {"us_per_frame": round(time_us(fn, args.reps) / n, 2)}
    return out


def loop(name, net, hf, wf, size):
    rng = np.random.default_rng(2)
    frames = [rng.integers(0, 256, (hf, wf, 3), dtype=np.uint8) for _ in range(args.frames)]
    segs = {"scaled": FrameSegmenter(net, hf, wf, depth=2, net_size=size), "frame_size": FrameSegmenter(net, hf, wf, depth=2)}
    for seg in segs.values():  # warm-up
        list(seg.segment(frames[:4]))
    rounds = []
    for _ in range(3):
        r = {}
        for key in ("scaled", "frame_size"):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n_out = sum(1 for _ in segs[key].segment(frames))
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            assert n_out == len(frames)
            r[key] = {"fps": round(len(frames) / dt, 1), "ms_per_frame": round(1e3 * dt / len(frames), 3)}
        rounds.append(r)
    for seg in segs.values():
        seg.close()
    return {"net": name, "frames_of": "%dx%d" % (hf, wf), "net_size": "%dx%d" % size, "frames": len(frames), "rounds": rounds,
            "scaled_ahead_in_every_pair": all(r["scaled"]["fps"] > r["frame_size"]["fps"] for r in rounds)}


def main():
    vgg = OSVOS_VGG(pretrained=0)
    vgg.load_state_dict(O.make_state_dict(2))
    torch.manual_seed(7)
    resnet = OSVOS_RESNET(pretrained=False, version=18)
    result = {"bench": "stream_scale", "device": torch.cuda.get_device_name(0), "kernels": kernels(),
              "loop": [loop("vgg", vgg.to(dev).eval(), 1080, 1920, (480, 854)),
                       loop("resnet18", resnet.to(dev).eval(), 2160, 3840, (1080, 1920))]}
    line = json.dumps(result)
    print(line)
    if args.json:
        with open(args.json, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
