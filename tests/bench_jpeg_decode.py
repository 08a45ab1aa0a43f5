"""The device JPEG decoder on one MI355X: ``ops.jpeg_decode`` alone at 8 / 32 / 64 files a launch against PIL's decode of the
same bytes in one thread, and the fast test pass (``experiment_helper.test_fast``) with the device-decode loader against
the loader as it is (``get_data_loader_test``, two workers) in alternating pairs, on a 64-frame 480x854 DAVIS tree of
quality-92 files, once 4:2:0 and once 4:4:4.  Prints ONE JSON line and writes it to profiles/jpeg_decode_bench.json.

    python tests/bench_jpeg_decode.py [--pairs 3] [--frames 64]

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
from pathlib import Path

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "fosvos_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import jpeg_cases as J  # noqa: E402
from oracle import osvos_ref as O  # noqa: E402
from util import experiment_helper, io_helper, jpeg_read  # noqa: E402

DEV = "cuda:0"
H, W = 480, 854
SUBSAMPLING = {"420": 2, "444": 0}


def frame_file(k, sub):
    rng = np.random.default_rng(k)
    img = np.clip(J.picture(H, W).astype(np.int32) + rng.integers(-12, 13, (H, W, 3)) + (k % 16), 0, 255).astype(np.uint8)
    b = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(img[..., ::-1])).save(b, "JPEG", quality=92, subsampling=SUBSAMPLING[sub])
    return b.getvalue()


def write_tree(root, files, seq="blob"):
    for d in ("ImageSets/480p", "JPEGImages/480p/" + seq, "Annotations/480p/" + seq):
        (root / d).mkdir(parents=True)
    lines = []
    for k, data in enumerate(files):
        (root / "JPEGImages" / "480p" / seq / ("%05d.jpg" % k)).write_bytes(data)
        lines.append("/JPEGImages/480p/%s/%05d.jpg /Annotations/480p/%s/%05d.png" % (seq, k, seq, k))
    for name in ("trainval.txt", "val.txt"):
        (root / "ImageSets" / "480p" / name).write_text("\n".join(lines) + "\n")
    y, x = np.mgrid[0:H, 0:W]
    mask = (((y - H / 2) ** 2 + (x - W / 2) ** 2) < (H / 3) ** 2).astype(np.uint8) * 255
    Image.fromarray(mask).save(str(root / "Annotations" / "480p" / seq / "00000.png"))


def time_decode(files, calls=4, repeats=5):
    from fosvos_hip import LaunchProfile, ops
    plans = [jpeg_read.probe(f) for f in files]
    out, status = ops.jpeg_decode(files, plans=plans)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0] * len(files)
    samples, host = [], []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        for _ in range(calls):
            ops.jpeg_decode(files, out=out, status=status, plans=plans)
        e1.record()
        host.append((time.perf_counter() - t0) * 1e6 / calls / len(files))
        e1.synchronize()
        samples.append(e0.elapsed_time(e1) * 1000.0 / calls / len(files))
    with LaunchProfile(0) as prof:
        ops.jpeg_decode(files, out=out, status=status, plans=plans)
    kernels = {k: v["ms"] * 1000.0 / len(files) for k, v in prof.records.items() if k.startswith("k_jpegd")}
    t0 = time.perf_counter()
    for f in files:
        jpeg_read.probe(f)
    probe_us = (time.perf_counter() - t0) * 1e6 / len(files)
    return {"us_per_file": statistics.median(samples), "host_enqueue_us_per_file": statistics.median(host),
            "kernel_us_per_file": kernels, "probe_us_per_file": probe_us}


def time_pil(files, repeats=3):
    samples = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for f in files:
            with Image.open(io.BytesIO(f)) as im:
                np.asarray(im.convert("RGB"))
        samples.append((time.perf_counter() - t0) * 1e6 / len(files))
    return statistics.median(samples)


class Provider:
    def __init__(self, network):
        self.network = network


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--frames", type=int, default=64)
    args = ap.parse_args()
    from networks.osvos_vgg import OSVOS_VGG
    net = OSVOS_VGG(pretrained=0)
    net.load_state_dict(O.make_state_dict(2))
    prov = Provider(net.to(DEV))
    result = {"bench": "jpeg_decode", "device": torch.cuda.get_device_name(0), "size": [H, W], "quality": 92, "frames": args.frames}
    for sub in ("420", "444"):
        files = [frame_file(k, sub) for k in range(args.frames)]
        entry = {"file_bytes_mean": sum(len(f) for f in files) / len(files), "pil_decode_us_per_file_one_thread": time_pil(files[:16]),
                 "ops_jpeg_decode": {str(n): time_decode(files[:n]) for n in (8, 32, 64) if n <= len(files)}}
        with tempfile.TemporaryDirectory() as tmp:
            root = Path(tmp) / "davis"
            write_tree(root, files)
            loaders = {"host_loader": lambda: io_helper.get_data_loader_test(root, 1, "blob"),
                       "device_decode": lambda: io_helper.get_data_loader_test(root, 1, "blob", device_decode=True)}
            for name, make in loaders.items():                              # warm-up
                experiment_helper.test_fast(prov, make(), Path(tmp) / ("warm_" + name), None, seq_name="blob")
            pairs = []
            for rep in range(args.pairs):
                pair = {}
                for name, make in loaders.items():
                    loader = make()
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    experiment_helper.test_fast(prov, loader, Path(tmp) / ("%s_%d" % (name, rep)), None, seq_name="blob")
                    torch.cuda.synchronize()
                    pair[name + "_fps"] = args.frames / (time.perf_counter() - t0)
                    pair[name + "_stages"] = {k: v for k, v in experiment_helper.last_fast.items() if k.startswith("seconds")}
                pairs.append(pair)
            same = all((Path(tmp) / "host_loader_0" / "blob" / ("%05d.png" % k)).read_bytes()
                       == (Path(tmp) / "device_decode_0" / "blob" / ("%05d.png" % k)).read_bytes() for k in range(args.frames))
            entry["test_fast"] = {"pairs": pairs, "same_png_files": same,
                                  "device_decode_ahead_in_every_pair": all(p["device_decode_fps"] > p["host_loader_fps"] for p in pairs)}
        result[sub] = entry
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "jpeg_decode_bench.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
