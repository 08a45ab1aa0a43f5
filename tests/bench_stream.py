"""Streaming inference on one MI355X (csrc/stream.hip, fosvos_hip/stream.py).  Two measurements, one JSON line:

* the kernels alone: microseconds per frame of ``ops.frame_prep`` and ``ops.overlay`` (boolean and soft overlay, mirrored) at
  1 and 5 frames a call, 480x854 and 1080x1920, from HIP events after a warm-up, with the achieved GB/s of the bytes the
  definitions need (prep 15 B a pixel, overlay 10 B);
* ``FrameSegmenter.segment`` at depth 1 and 2 against the HOST PATH: the reference's per-frame arithmetic
  (src/run_webcam.py:81-133) in numpy around the same ``net.forward`` - mirror, float32 mean subtraction, a float32 upload,
  a synchronous download, float32 sigmoid, threshold and float64 overlay.  The host path is the yardstick, written here,
  never the code under test.  VGG at 480x854 and ResNet-18 at 1080x1920, seeded weights, frames pre-generated in host
  memory, three alternating rounds after a warm-up; frames/s and ms per frame of each.
A diagnostic, not the headline metric - bench.py stays on the fine-tune.
usage: python tests/bench_stream.py [--json out.json] [--frames 24] [--reps 100]"""
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
ap.add_argument("--frames", type=int, default=24)
ap.add_argument("--reps", type=int, default=100)
args = ap.parse_args()
dev = "cuda:0"
assert torch.cuda.is_available(), "bench_stream.py measures on the GPU; there is no CPU timing"
SIZES = [(480, 854), (1080, 1920)]
MEAN = np.array((104.00699, 116.66877, 122.67892), dtype=np.float32)  # the reference's mean_value, for the host path


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
    for h, w in SIZES:
        for n in (1, 5):
            frames = torch.randint(0, 256, (n, h, w, 3), generator=g, dtype=torch.uint8).to(dev)
            logits = (3 * torch.randn((n, 1, h, w), generator=g)).to(dev)
            image = torch.empty((n, 3, h, w), device=dev)
            shown = torch.empty((n, h, w, 3), dtype=torch.uint8, device=dev)
            px = n * h * w
            for name, nbytes, fn in (
                    ("frame_prep", 15 * px, lambda: ops.frame_prep(frames, True, out=image)),
                    ("overlay_boolean", 10 * px, lambda: ops.overlay(frames, logits, True, True, "r", 1.0, out=shown)),
                    ("overlay_soft", 10 * px, lambda: ops.overlay(frames, logits, True, False, "r", 1.0, out=shown))):
                us = time_us(fn, args.reps)
                out["%s_%dx%dx%d" % (name, n, h, w)] = {"us_per_frame": round(us / n, 2), "GBps": round(nbytes / us / 1e3, 1)}
    return out


def host_path(net, img, color_index=2, alpha=1.0):
    """One frame the way the reference does it (mirror on, boolean mask, red overlay, alpha 1)."""
    img = img[:, ::-1]
    x = img - MEAN
    t = torch.from_numpy(np.ascontiguousarray(x[np.newaxis].transpose((0, 3, 1, 2)))).cuda()
    with torch.no_grad():
        prediction = net.forward(t)[-1]
    p = prediction.cpu().numpy()[0]
    p = np.squeeze(1 / (1 + np.exp(-np.transpose(p, (1, 2, 0)))))
    p[p >= 0.5] = 1
    p[p < 0.5] = 0
    mask = np.zeros(img.shape, dtype=float)
    mask[..., color_index] = 255
    out = img + alpha * mask * p[..., np.newaxis]
    out[out > 255] = 255
    return out.astype("uint8")


def pipeline(name, net, h, w):
    rng = np.random.default_rng(2)
    frames = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(args.frames)]
    segs = {d: FrameSegmenter(net, h, w, depth=d) for d in (1, 2)}

    def run_host():
        return [host_path(net, f) for f in frames]

    def run_dev(d):
        return list(segs[d].segment(frames))

    # warm-up, and the two paths draw the same picture (the float32 sigmoid of the host path can only differ from
    # logit >= 0 for logits in (-2**-24, 0))
    a, b = run_host(), run_dev(2)
    run_dev(1)
    differing = sum(int((x != y).any(axis=2).sum()) for x, y in zip(a, b))
    rounds = []
    for _ in range(3):
        r = {}
        for key, fn in (("device_depth1", lambda: run_dev(1)), ("device_depth2", lambda: run_dev(2)), ("host", run_host)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            r[key] = {"fps": round(len(frames) / dt, 1), "ms_per_frame": round(1e3 * dt / len(frames), 3)}
        rounds.append(r)
    for s in segs.values():
        s.close()
    ahead = all(r[k]["fps"] > r["host"]["fps"] for r in rounds for k in ("device_depth1", "device_depth2"))
    return {"net": name, "size": "%dx%d" % (h, w), "frames": len(frames), "pixels_differing_from_host_path": differing,
            "rounds": rounds, "device_ahead_in_every_round": ahead}


def main():
    vgg = OSVOS_VGG(pretrained=0)
    vgg.load_state_dict(O.make_state_dict(2))
    torch.manual_seed(7)
    resnet = OSVOS_RESNET(pretrained=False, version=18)
    result = {"bench": "stream", "device": torch.cuda.get_device_name(0), "kernels": kernels(),
              "pipeline": [pipeline("vgg", vgg.to(dev).eval(), 480, 854),
                           pipeline("resnet18", resnet.to(dev).eval(), 1080, 1920)]}
    line = json.dumps(result)
    print(line)
    if args.json:
        with open(args.json, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
