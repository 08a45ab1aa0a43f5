"""The PNG-writing test pass on one MI355X: ``ops.png_encode`` alone against PIL's encoder on the host, the whole fast pass
(``experiment_helper.test_fast``) against ``test_scored`` in alternating pairs, and the file sizes.  Prints ONE JSON line
(kept as profiles/test_pass_bench.json).

    python tests/bench_test_pass.py [--repeats 3] [--frames 16 64]

Timing: warm-up calls first, HIP events around back-to-back calls, median of repeats; the two passes alternate on one
device in one process."""
import argparse
import io
import json
import os
import statistics
import sys
import tempfile
import time
import zlib
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
HBM_GBPS = 8000.0  # MI355X peak HBM3E rate


def probability_map(h=480, w=854, seed=0):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    d = ((y - 0.5 * h) / (0.3 * h)) ** 2 + ((x - 0.5 * w) / (0.25 * w)) ** 2
    z = (1.0 - d) * 40.0 + rng.normal(0.0, 2.0, (h, w))
    return (np.clip(255.0 / (1.0 + np.exp(-z)), 0, 255) + 0.5).astype(np.uint8)


def time_encode(frames, calls=20, repeats=7):
    from fosvos_hip import ops
    x = torch.from_numpy(frames).to(DEV)
    out, lengths = ops.png_encode(x)
    for _ in range(5):
        ops.png_encode(x, out=out, lengths=lengths)
    torch.cuda.synchronize()
    samples = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            ops.png_encode(x, out=out, lengths=lengths)
        e1.record()
        e1.synchronize()
        samples.append(e0.elapsed_time(e1) * 1000.0 / calls / frames.shape[0])
    us = statistics.median(samples)
    n, h, w = frames.shape
    file_bytes = int(lengths.sum().item()) / n
    moved = 2 * h * w + file_bytes + 2 * 16 * png_layout.n_segments(h, w)  # the image read twice, the file and the records
    return {"us_per_frame": us, "file_bytes_per_frame": file_bytes, "bytes_moved_per_frame": moved,
            "fraction_of_hbm_rate": moved / (us * 1e-6) / (HBM_GBPS * 1e9)}


def time_pil(img, repeats=7):
    samples = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        Image.fromarray(img, mode="L").save(io.BytesIO(), format="PNG")
        samples.append((time.perf_counter() - t0) * 1e6)
    return statistics.median(samples)


class Provider:
    def __init__(self, network):
        self.network = network


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--frames", type=int, nargs="+", default=[16, 64])
    args = ap.parse_args()
    from networks.osvos_vgg import OSVOS_VGG

    result = {"bench": "test_pass", "device": torch.cuda.get_device_name(0), "size": [480, 854]}
    pm = probability_map()
    five = np.stack([probability_map(seed=k) for k in range(5)])
    result["png_encode"] = {"frames_1": time_encode(pm[None]), "frames_5": time_encode(five),
                            "pil_save_us_per_frame": time_pil(pm)}
    level6 = io.BytesIO()
    Image.fromarray(pm, mode="L").save(level6, format="PNG")
    result["file_size_probability_map"] = {"device_layout": len(png_layout.encode(pm)), "pil_level6": level6.tell(),
                                           "zlib_level6_stream": len(zlib.compress(png_layout.filtered_stream(pm).tobytes(), 6)),
                                           "stored": 480 * 855}

    net = OSVOS_VGG(pretrained=0)
    net.load_state_dict(O.make_state_dict(2))
    prov = Provider(net.to(DEV))
    passes = {}
    with tempfile.TemporaryDirectory() as tmp:
        for n_frames in args.frames:
            loader = io_helper.get_data_loader_test(None, 1, "blob", synthetic=(480, 854), n_frames=n_frames)
            ann = loader.dataset.annotation
            experiment_helper.test_fast(prov, loader, Path(tmp) / "warm_fast", ann, seq_name="blob")
            experiment_helper.test_scored(prov, loader, Path(tmp) / "warm_scored", ann, seq_name="blob")
            pairs, stages = [], []
            for rep in range(args.repeats):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                experiment_helper.test_scored(prov, loader, Path(tmp) / ("scored%d" % rep), ann, seq_name="blob")
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                experiment_helper.test_fast(prov, loader, Path(tmp) / ("fast%d" % rep), ann, seq_name="blob")
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                stages.append({k: v for k, v in experiment_helper.last_fast.items() if k.startswith("seconds")})
                experiment_helper.test_fast(prov, loader, Path(tmp) / ("fast5_%d" % rep), ann, seq_name="blob", forward_batch=5)
                torch.cuda.synchronize()
                t3 = time.perf_counter()
                pairs.append({"test_scored_fps": n_frames / (t1 - t0), "test_fast_fps": n_frames / (t2 - t1),
                              "test_fast_forward_batch_5_fps": n_frames / (t3 - t2)})
            # the loader alone: what the host spends making the synthetic frames
            t0 = time.perf_counter()
            for _ in loader:
                pass
            loader_s = time.perf_counter() - t0
            fast_bytes = experiment_helper.last_fast["png_bytes"] / n_frames
            scored_dir = Path(tmp) / "scored0" / "blob"
            passes[str(n_frames)] = {
                "pairs": pairs, "fast_ahead_in_every_pair": all(p["test_fast_fps"] > p["test_scored_fps"] for p in pairs),
                "test_fast_host_seconds": stages, "loader_alone_seconds": loader_s,
                "file_bytes_per_frame": {"test_fast": fast_bytes,
                                         "test_scored_pil": sum(p.stat().st_size for p in scored_dir.iterdir()) / n_frames,
                                         "stored": 480 * 855}}
    result["passes"] = passes
    print(json.dumps(result))


if __name__ == "__main__":
    main()
