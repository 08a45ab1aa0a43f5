"""Fitted against fixed Huffman codes in the device PNG encoder on one MI355X: ``ops.png_encode`` in both modes, alternating
in one process, at 5 and 1 frames a call; the whole fast pass (``experiment_helper.test_fast``) in alternating pairs; and the
file sizes (fixed, fitted, PIL level 6, stored) of the probability map and of the synthetic sequence's frames.  Prints ONE JSON
line and writes it to profiles/png_fitted_bench.json.

    python tests/bench_png_fitted.py [--repeats 3] [--frames 16 64]

Timing as in tests/bench_test_pass.py: warm-up calls first, HIP events around 20 back-to-back calls, median of seven."""
import argparse
import io
import json
import os
import statistics
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "fosvos_amd"))

from oracle import osvos_ref as O  # noqa: E402
from util import experiment_helper, io_helper, png_layout  # noqa: E402

DEV = "cuda:0"
MODES = ("fixed", "fitted")


def probability_map(h=480, w=854, seed=0):
    """The map of tests/bench_test_pass.py: saturated inside and outside an ellipse, noisy edge."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    d = ((y - 0.5 * h) / (0.3 * h)) ** 2 + ((x - 0.5 * w) / (0.25 * w)) ** 2
    z = (1.0 - d) * 40.0 + rng.normal(0.0, 2.0, (h, w))
    return (np.clip(255.0 / (1.0 + np.exp(-z)), 0, 255) + 0.5).astype(np.uint8)


def pil_bytes(img):
    buf = io.BytesIO()
    Image.fromarray(img, mode="L").save(buf, format="PNG")
    return buf.tell()


def file_sizes(images):
    """Mean bytes a frame; the two device layouts from the numpy statement the kernels are tested against."""
    n = len(images)
    return {"fixed": sum(len(png_layout.encode(m)) for m in images) / n,
            "fitted": sum(len(png_layout.encode(m, huffman="fitted")) for m in images) / n,
            "pil_level6": sum(pil_bytes(m) for m in images) / n,
            "stored": sum(m.shape[0] * (m.shape[1] + 1) for m in images) / n}


def time_encode(frames, calls=20, repeats=7):
    """us a frame of both modes, a repetition of one following a repetition of the other."""
    from fosvos_hip import ops
    x = torch.from_numpy(frames).to(DEV)
    out, lengths = ops.png_encode(x)
    for mode in MODES:
        for _ in range(5):
            ops.png_encode(x, out=out, lengths=lengths, huffman=mode)
    torch.cuda.synchronize()
    samples, file_bytes = {mode: [] for mode in MODES}, {}
    for _ in range(repeats):
        for mode in MODES:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                ops.png_encode(x, out=out, lengths=lengths, huffman=mode)
            e1.record()
            e1.synchronize()
            samples[mode].append(e0.elapsed_time(e1) * 1000.0 / calls / frames.shape[0])
            file_bytes[mode] = int(lengths.sum().item()) / frames.shape[0]
    return {mode: {"us_per_frame": statistics.median(samples[mode]), "us_per_frame_min": min(samples[mode]),
                   "us_per_frame_max": max(samples[mode]), "file_bytes_per_frame": file_bytes[mode]} for mode in MODES}


class Provider:
    def __init__(self, network):
        self.network = network


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--frames", type=int, nargs="+", default=[16, 64])
    args = ap.parse_args()
    from networks.osvos_vgg import OSVOS_VGG

    result = {"bench": "png_fitted", "device": torch.cuda.get_device_name(0), "size": [480, 854]}
    pm = probability_map()
    five = np.stack([probability_map(seed=k) for k in range(5)])
    result["png_encode"] = {"frames_5": time_encode(five), "frames_1": time_encode(pm[None])}
    result["file_size_probability_map"] = file_sizes([pm])

    net = OSVOS_VGG(pretrained=0)
    net.load_state_dict(O.make_state_dict(2))
    prov = Provider(net.to(DEV))
    passes = {}
    with tempfile.TemporaryDirectory() as tmp:
        for n_frames in args.frames:
            loader = io_helper.get_data_loader_test(None, 1, "blob", synthetic=(480, 854), n_frames=n_frames)
            for mode in MODES:
                experiment_helper.test_fast(prov, loader, Path(tmp) / ("warm_" + mode), seq_name="blob", png_huffman=mode)
            pairs, png_bytes = [], {}
            for rep in range(args.repeats):
                fps = {}
                for mode in MODES:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    experiment_helper.test_fast(prov, loader, Path(tmp) / ("%s%d" % (mode, rep)), seq_name="blob",
                                                png_huffman=mode)
                    torch.cuda.synchronize()
                    fps[mode] = n_frames / (time.perf_counter() - t0)
                    png_bytes[mode] = experiment_helper.last_fast["png_bytes"] / n_frames
                pairs.append(fps)
            fixed = [p["fixed"] for p in pairs]
            frames = [np.asarray(Image.open(str(f))) for f in sorted((Path(tmp) / "fitted0" / "blob").iterdir())]
            same = all(np.array_equal(m, np.asarray(Image.open(str(Path(tmp) / "fixed0" / "blob" / ("%05d.png" % k)))))
                       for k, m in enumerate(frames))
            passes[str(n_frames)] = {
                "pairs_fps": pairs, "fixed_spread_fps": [min(fixed), max(fixed)],
                "fitted_within_fixed_spread": all(min(fixed) <= p["fitted"] <= max(fixed) or p["fitted"] > max(fixed)
                                                  for p in pairs),
                "same_pixels": same, "png_bytes_per_frame": png_bytes, "file_bytes_per_frame": file_sizes(frames)}
    result["passes"] = passes
    line = json.dumps(result)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "png_fitted_bench.json"), "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
