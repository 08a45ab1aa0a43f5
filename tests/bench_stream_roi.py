"""Following the object in the stream on one MI355X (csrc/stream.hip: k_frame_prep_window, k_overlay_window, k_window_reset +
k_window_next; ``FrameSegmenter(roi=)``).  Two measurements, one JSON line:

* the loop: ``FrameSegmenter.segment`` at depth 2 over 64 frames of 1080x1920 with a drifting synthetic disc, the VGG at
  480x854 (seeded weights: what it segments means nothing, and no accuracy is claimed), with ``net_size`` alone against
  ``net_size`` + ``roi``; three alternating rounds in one process after a warm-up; frames/s and ms per frame of each, and the
  window the roi loop ended on;
* the kernels alone, microseconds per frame from HIP events after a warm-up, at one and at eight frames a call:
  ``ops.frame_prep_window`` (the whole-frame window, a window half way up the ladder, the net's own size) beside
  ``ops.frame_prep(net_size=)``, ``ops.overlay_window`` (boolean and soft, mirrored, the same three windows) beside
  ``ops.overlay(net_size=)``, and ``ops.window_next``.
The expectation - the window costs two small launches and nothing else - is what this measures; nothing here asserts a ratio.
A diagnostic, not the headline metric - bench.py stays on the fine-tune.
usage: python tests/bench_stream_roi.py [--json profiles/stream_roi_bench.json] [--frames 64] [--reps 100]"""
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
from fosvos_hip.options import RoiOptions  # noqa: E402
from fosvos_hip.stream import FrameSegmenter  # noqa: E402
from networks.osvos_vgg import OSVOS_VGG  # noqa: E402
from oracle import osvos_ref as O  # noqa: E402  (seeded weights only)
from util import frame_roi  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--json", default=None)
ap.add_argument("--frames", type=int, default=64)
ap.add_argument("--reps", type=int, default=100)
args = ap.parse_args()
dev = "cuda:0"
assert torch.cuda.is_available(), "bench_stream_roi.py measures on the GPU; there is no CPU timing"
HF, WF, SIZE = 1080, 1920, (480, 854)


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
    sizes = frame_roi.ladder(HF, WF, SIZE[0], SIZE[1], 8)
    named = {"whole": (0, 0, HF, WF), "level4": ((HF - sizes[4][0]) // 2, (WF - sizes[4][1]) // 2) + sizes[4],
             "net_size": ((HF - SIZE[0]) // 2, (WF - SIZE[1]) // 2) + SIZE}
    for n in (1, 8):
        frames = torch.randint(0, 256, (n, HF, WF, 3), generator=g, dtype=torch.uint8).to(dev)
        small = (3 * torch.randn((n, 1) + SIZE, generator=g)).to(dev)
        image = torch.empty((n, 3) + SIZE, device=dev)
        shown = torch.empty((n, HF, WF, 3), dtype=torch.uint8, device=dev)
        nxt = torch.empty((n, 4), dtype=torch.int32, device=dev)
        runs = [("frame_prep_scaled", lambda: ops.frame_prep(frames, True, out=image, net_size=SIZE)),
                ("overlay_boolean_scaled", lambda: ops.overlay(frames, small, True, True, "r", 1.0, out=shown, net_size=SIZE)),
                ("overlay_soft_scaled", lambda: ops.overlay(frames, small, True, False, "r", 1.0, out=shown, net_size=SIZE))]
        for key, window in named.items():
            w = torch.tensor([window] * n, dtype=torch.int32, device=dev)
            runs += [("frame_prep_window_" + key, lambda w=w: ops.frame_prep_window(frames, w, SIZE, True, out=image)),
                     ("overlay_boolean_window_" + key, lambda w=w: ops.overlay_window(frames, small, w, True, True, "r", 1.0, out=shown)),
                     ("overlay_soft_window_" + key, lambda w=w: ops.overlay_window(frames, small, w, True, False, "r", 1.0, out=shown)),
                     ("window_next_" + key, lambda w=w: ops.window_next(small, w, (HF, WF), out=nxt))]
        for name, fn in runs:
            out["%s_%dx%dx%d" % (name, n, HF, WF)] = {"us_per_frame": round(time_us(fn, args.reps) / n, 2)}
    return out


def disc_frames(count):
    """A bright disc of radius 150 that drifts by (3, 7) pixels a frame over noise."""
    rng = np.random.default_rng(2)
    yy, xx = np.mgrid[0:HF, 0:WF]
    frames = []
    for k in range(count):
        f = rng.integers(0, 96, (HF, WF, 3), dtype=np.uint8)
        f[(yy - (400 + 3 * k)) ** 2 + (xx - (600 + 7 * k)) ** 2 <= 150 ** 2] = 240
        frames.append(f)
    return frames


def loop(net):
    frames = disc_frames(args.frames)
    segs = {"roi": FrameSegmenter(net, HF, WF, depth=2, net_size=SIZE, roi=RoiOptions()),
            "net_size": FrameSegmenter(net, HF, WF, depth=2, net_size=SIZE)}
    for seg in segs.values():  # warm-up
        list(seg.segment(frames[:4]))
    rounds = []
    for _ in range(3):
        r = {}
        for key in ("roi", "net_size"):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n_out = sum(1 for _ in segs[key].segment(frames))
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            assert n_out == len(frames)
            r[key] = {"fps": round(len(frames) / dt, 1), "ms_per_frame": round(1e3 * dt / len(frames), 3)}
        r["roi"]["last_window"] = list(segs["roi"].last_window())
        rounds.append(r)
    for seg in segs.values():
        seg.close()
    return {"net": "vgg", "frames_of": "%dx%d" % (HF, WF), "net_size": "%dx%d" % SIZE, "frames": len(frames), "rounds": rounds}


def main():
    vgg = OSVOS_VGG(pretrained=0)
    vgg.load_state_dict(O.make_state_dict(2))
    result = {"bench": "stream_roi", "device": torch.cuda.get_device_name(0), "kernels": kernels(), "loop": loop(vgg.to(dev).eval())}
    line = json.dumps(result)
    print(line)
    if args.json:
        with open(args.json, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
