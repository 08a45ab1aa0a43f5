"""Edge-aware upsampling in the stream on one MI355X (csrc/guided.hip: k_guided_fit, k_guided_smooth; csrc/stream.hip:
k_overlay_guided; ``FrameSegmenter(refine=)``).  Three measurements, one JSON line (also written to
profiles/stream_refine_bench.json):

* the kernels alone, microseconds per frame from HIP events after a warm-up: ``ops.guided_coefficients`` and
  ``ops.overlay_guided`` (boolean and soft overlay, boolean mask; mirrored) beside ``ops.overlay(net_size=)`` on the same frames -
  1080x1920 frames with the net at 480x854, and 480x854 unscaled; one and eight frames a call;
* the loop: ``FrameSegmenter.segment`` at depth 2 over the same 64 frames with ``refine=RefineOptions()`` and with ``refine=None``
  - VGG with seeded weights, 1080x1920 frames, the net at 480x854; frames pre-generated in host memory, three alternating
  rounds after a warm-up; frames/s and ms per frame of each;
* the host path it replaces: the logits and the image downloaded, then the same filter in numpy with cumsum box sums at the
  net's size and its application at the frame's size, on the same logits; milliseconds per frame.
A diagnostic, not the headline metric - bench.py stays on the fine-tune.
usage: python tests/bench_stream_refine.py [--json profiles/stream_refine_bench.json] [--frames 64] [--reps 100]"""
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
from fosvos_hip.options import RefineOptions  # noqa: E402
from fosvos_hip.stream import FrameSegmenter  # noqa: E402
from networks.osvos_vgg import OSVOS_VGG  # noqa: E402
from oracle import osvos_ref as O  # noqa: E402  (seeded weights only)
from util import guided_upsample as G  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "stream_refine_bench.json"))
ap.add_argument("--frames", type=int, default=64)
ap.add_argument("--reps", type=int, default=100)
args = ap.parse_args()
dev = "cuda:0"
assert torch.cuda.is_available(), "bench_stream_refine.py measures on the GPU; there is no CPU timing"


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
    o = RefineOptions()
    for (hf, wf), size in (((1080, 1920), (480, 854)), ((480, 854), (480, 854))):
        for n in (1, 8):
            frames = torch.randint(0, 256, (n, hf, wf, 3), generator=g, dtype=torch.uint8).to(dev)
            image = ops.frame_prep(frames, True, net_size=size)
            logits = (3 * torch.randn((n, 1) + size, generator=g)).to(dev)
            coeff = torch.empty((n, 2) + size, dtype=torch.float64, device=dev)
            shown = torch.empty((n, hf, wf, 3), dtype=torch.uint8, device=dev)
            mask = torch.empty((n, hf, wf), dtype=torch.uint8, device=dev)
            ops.guided_coefficients(image, logits, o.radius, o.eps, o.clip, out=coeff)
            for name, fn in (
                    ("guided_coefficients", lambda: ops.guided_coefficients(image, logits, o.radius, o.eps, o.clip, out=coeff)),
                    ("overlay_guided_boolean", lambda: ops.overlay_guided(frames, coeff, True, True, "r", 1.0, out=shown)),
                    ("overlay_guided_soft", lambda: ops.overlay_guided(frames, coeff, True, False, "r", 1.0, out=shown)),
                    ("overlay_guided_mask", lambda: ops.overlay_guided(frames, coeff, True, True, overlay=False, out=mask)),
                    ("overlay_boolean", lambda: ops.overlay(frames, logits, True, True, "r", 1.0, out=shown, net_size=size)),
                    ("overlay_soft", lambda: ops.overlay(frames, logits, True, False, "r", 1.0, out=shown, net_size=size)),
                    ("overlay_mask", lambda: ops.overlay(frames, logits, True, True, overlay=False, out=mask, net_size=size))):
                out["%s_%dx%dx%d_net_%dx%d" % ((name, n, hf, wf) + size)] = {"us_per_frame": round(time_us(fn, args.reps) / n, 2)}
    return out


def host_filter(image, logits, r, eps, clip):
    """The textbook guided filter with cumsum box sums: float64 [2,Hn,Wn]."""
    g = image.astype(np.float64).sum(axis=0)
    p = np.clip(np.nan_to_num(logits.astype(np.float64), nan=-clip, posinf=clip, neginf=-clip), -clip, clip)
    h, w = g.shape
    y, x = np.arange(h), np.arange(w)
    ya, yb, xa, xb = np.maximum(0, y - r), np.minimum(h - 1, y + r) + 1, np.maximum(0, x - r), np.minimum(w - 1, x + r) + 1
    cnt = ((yb - ya)[:, None] * (xb - xa)[None, :]).astype(np.float64)

    def mean(v):
        c = np.zeros((h + 1, w + 1))
        c[1:, 1:] = v.cumsum(0).cumsum(1)
        return (c[yb][:, xb] - c[ya][:, xb] - c[yb][:, xa] + c[ya][:, xa]) / cnt

    mg, mp = mean(g), mean(p)
    a = (mean(g * p) - mg * mp) / (mean(g * g) - mg * mg + eps)
    return np.stack([mean(a), mean(mp - a * mg)])


def host_path(net, hf, wf, size, reps=5):
    """What the device path replaces: per frame, the image and the logits come down, the filter runs in numpy."""
    o = RefineOptions()
    rng = np.random.default_rng(2)
    frame = rng.integers(0, 256, (hf, wf, 3), dtype=np.uint8)
    with torch.no_grad():
        image = ops.frame_prep(torch.from_numpy(frame[None]).to(dev), True, net_size=size)
        logits = net.forward(image)[-1].contiguous()
    torch.cuda.synchronize()
    t_down, t_fit, t_apply = [], [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        im, lg = image.cpu().numpy()[0], logits.cpu().numpy()[0, 0]
        t1 = time.perf_counter()
        coeff = host_filter(im, lg, o.radius, o.eps, o.clip)
        t2 = time.perf_counter()
        G.overlay_guided(frame, coeff, True)
        t3 = time.perf_counter()
        t_down.append(t1 - t0), t_fit.append(t2 - t1), t_apply.append(t3 - t2)
    exact = G.coefficients(im, lg, o.radius, o.eps, o.clip)
    return {"frames_of": "%dx%d" % (hf, wf), "net_size": "%dx%d" % size, "reps": reps,
            "download_ms": round(1e3 * sorted(t_down)[reps // 2], 3), "filter_cumsum_ms": round(1e3 * sorted(t_fit)[reps // 2], 2),
            "apply_numpy_ms": round(1e3 * sorted(t_apply)[reps // 2], 2),
            "cumsum_against_definition_max_abs": float(np.abs(coeff - exact).max())}


def loop(name, net, hf, wf, size):
    rng = np.random.default_rng(2)
    frames = [rng.integers(0, 256, (hf, wf, 3), dtype=np.uint8) for _ in range(args.frames)]
    segs = {"refine": FrameSegmenter(net, hf, wf, depth=2, net_size=size, refine=RefineOptions()),
            "plain": FrameSegmenter(net, hf, wf, depth=2, net_size=size)}
    for seg in segs.values():  # warm-up
        list(seg.segment(frames[:4]))
    rounds = []
    for _ in range(3):
        r = {}
        for key in ("refine", "plain"):
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
    return {"net": name, "frames_of": "%dx%d" % (hf, wf), "net_size": "%dx%d" % size, "frames": len(frames), "depth": 2,
            "rounds": rounds}


def main():
    vgg = OSVOS_VGG(pretrained=0)
    vgg.load_state_dict(O.make_state_dict(2))
    vgg = vgg.to(dev).eval()
    result = {"bench": "stream_refine", "device": torch.cuda.get_device_name(0), "refine": RefineOptions().as_dict(),
              "kernels": kernels(), "loop": [loop("vgg", vgg, 1080, 1920, (480, 854))],
              "host_path": host_path(vgg, 1080, 1920, (480, 854))}
    line = json.dumps(result)
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
