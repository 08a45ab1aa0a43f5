"""Several objects in streaming inference on one MI355X (csrc/stream.hip: k_overlay_objects, k_overlay_objects_scaled;
``fosvos_hip.stream.ObjectSegmenter``), K = 3 small-weight VGG nets.  Two measurements, one JSON line:

* the loop: ``ObjectSegmenter.segment`` at depth 2 over the same frames against the host path over the same nets - the prep
  on the device, K forwards, the download of the K float32 maps, then ``object_overlay.apply`` in numpy - at 480x854, and at
  1080x1920 with ``net_size=(480, 854)``; frames pre-generated in host memory, three alternating rounds after a warm-up;
  frames/s and ms per frame of each, and whether the device loop is ahead in every pair;
* the kernels alone, microseconds per frame from HIP events after a warm-up: ``ops.overlay_objects`` beside
  ``ops.merge_objects`` + ``ops.overlay`` (the two launches that come closest to it: they paint one object in one channel)
  at 480x854 and 1080x1920, one frame and eight frames a call, and the scaled launch at 1080x1920 from 480x854 maps, overlay
  and label map.
A diagnostic, not the headline metric - bench.py stays on the fine-tune.
usage: python tests/bench_stream_objects.py [--json profiles/stream_objects_bench.json] [--frames 64] [--reps 100]"""
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
from fosvos_hip.stream import ObjectSegmenter  # noqa: E402
from networks.osvos_vgg import OSVOS_VGG  # noqa: E402
from oracle import osvos_ref as O  # noqa: E402  (seeded weights only)
from util import object_overlay  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "stream_objects_bench.json"))
ap.add_argument("--frames", type=int, default=64)
ap.add_argument("--reps", type=int, default=100)
args = ap.parse_args()
dev = "cuda:0"
K = 3
assert torch.cuda.is_available(), "bench_stream_objects.py measures on the GPU; there is no CPU timing"


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
    size = (480, 854)
    for hf, wf in ((480, 854), (1080, 1920)):
        for n in (1, 8):  # one frame a call is bounded by the Python call; eight show the kernels
            frames = torch.randint(0, 256, (n, hf, wf, 3), generator=g, dtype=torch.uint8).to(dev)
            maps = [(3 * torch.randn((n, 1, hf, wf), generator=g)).to(dev) for _ in range(K)]
            shown = torch.empty((n, hf, wf, 3), dtype=torch.uint8, device=dev)
            labels = torch.empty((n, hf, wf), dtype=torch.uint8, device=dev)

            def two_launches():
                ops.merge_objects(maps, out=labels)
                ops.overlay(frames, maps[0], True, True, "r", 0.5, out=shown)

            runs = [("overlay_objects", lambda: ops.overlay_objects(frames, maps, True, out=shown)),
                    ("merge_objects_then_overlay", two_launches)]
            if (hf, wf) != size:
                small = [(3 * torch.randn((n, 1) + size, generator=g)).to(dev) for _ in range(K)]
                runs += [("overlay_objects_scaled_from_%dx%d" % size,
                          lambda: ops.overlay_objects(frames, small, True, out=shown, net_size=size)),
                         ("labels_scaled_from_%dx%d" % size,
                          lambda: ops.overlay_objects(frames, small, True, False, out=labels, net_size=size))]
            for name, fn in runs:
                out["%s_%dx%dx%d" % (name, n, hf, wf)] = {"us_per_frame": round(time_us(fn, args.reps) / n, 2)}
    return out


def host_path(nets, frames, hf, wf, size):
    """The same nets without the new op: K maps cross the bus as float32, the merge and the paint happen in numpy."""
    outs = []
    with torch.no_grad():
        for frame in frames:
            fd = torch.from_numpy(frame).to(dev)[None]
            image = ops.frame_prep(fd, True, net_size=size)
            maps = [net.forward(image)[-1][0, 0].cpu().numpy() for net in nets]
            outs.append(object_overlay.apply(frame, maps, True, True, None, 0.5, *((hf, wf) if size else (None, None))))
    return outs


def loop(nets, hf, wf, size):
    rng = np.random.default_rng(2)
    frames = [rng.integers(0, 256, (hf, wf, 3), dtype=np.uint8) for _ in range(args.frames)]
    seg = ObjectSegmenter(nets, hf, wf, depth=2, net_size=size)
    runs = {"device": lambda fs: sum(1 for _ in seg.segment(fs)), "host": lambda fs: len(host_path(nets, fs, hf, wf, size))}
    for run in runs.values():  # warm-up
        run(frames[:4])
    rounds = []
    for _ in range(3):
        r = {}
        for key in ("device", "host"):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n_out = runs[key](frames)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            assert n_out == len(frames)
            r[key] = {"fps": round(len(frames) / dt, 1), "ms_per_frame": round(1e3 * dt / len(frames), 3)}
        rounds.append(r)
    seg.close()
    return {"nets": "%d x vgg" % len(nets), "frames_of": "%dx%d" % (hf, wf), "net_size": "%dx%d" % (size or (hf, wf)),
            "frames": len(frames), "rounds": rounds,
            "device_ahead_in_every_pair": all(r["device"]["fps"] > r["host"]["fps"] for r in rounds)}


def main():
    nets = []
    for seed in range(2, 2 + K):
        net = OSVOS_VGG(pretrained=0)
        net.load_state_dict(O.make_state_dict(seed))
        net.compute_side_outputs = False  # for both paths: the segmenter asks for the last output only
        nets.append(net.to(dev).eval())
    result = {"bench": "stream_objects", "device": torch.cuda.get_device_name(0), "objects": K, "kernels": kernels(),
              "loop": [loop(nets, 480, 854, None), loop(nets, 1080, 1920, (480, 854))]}
    line = json.dumps(result)
    print(line)
    if args.json:
        with open(args.json, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
