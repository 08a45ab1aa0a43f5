"""The multi-object ops and pass on one MI355X (csrc/eval.hip: fosvos_merge_objects, fosvos_jf_counts_labels; csrc/png.hip:
fosvos_png_encode_indexed).  Two comparisons, one JSON line (also written to profiles/multi_object_bench.json), 480x854, K = 3
nets, five frames a call:

* the three ops - merge, palette PNG, per-object J / F counts - together and alone (HIP events after a warm-up), against the
  host path they replace: download K float32 logit maps, ``object_merge.merge_labels`` in numpy, PIL ``save`` of a mode-``P``
  image into memory (wall clock, one host core);
* ``experiment_helper.test_objects`` over a synthetic sequence against K runs of ``experiment_helper.test_fast`` over the same
  frames (what a user without the merged pass would run: K passes, K sets of probability PNGs, and the merge still to do).
Three alternating rounds in one process after a warm-up; every round is reported, no threshold is asserted.
A diagnostic, not the headline metric - bench.py stays on the fine-tune.
usage: python tests/bench_multi_object.py [--json profiles/multi_object_bench.json] [--frames 10] [--reps 50]"""
import argparse
import io
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "fosvos_amd"))

from dataloaders.synthetic import SyntheticObjectsSequence  # noqa: E402
from fosvos_hip import ops  # noqa: E402
from networks.osvos_vgg import OSVOS_VGG  # noqa: E402
from oracle import osvos_ref as O  # noqa: E402  (seeded weights only)
from util import experiment_helper, object_merge  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "multi_object_bench.json"))
ap.add_argument("--frames", type=int, default=10)
ap.add_argument("--reps", type=int, default=50)
args = ap.parse_args()
dev = "cuda:0"
assert torch.cuda.is_available(), "bench_multi_object.py measures on the GPU; there is no CPU timing"
H, W, K, N = 480, 854, 3, 5


def time_us(fn, reps):
    for _ in range(5):
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


def object_logits():
    """K logit maps of N frames: each object's ellipse of the synthetic sequence above zero, noise on its rim."""
    data = SyntheticObjectsSequence("bench", H, W, n_frames=N, n_objects=K)
    ids = np.stack([data.annotation("bench", "%05d" % f) for f in range(N)])
    rng = np.random.default_rng(0)
    maps = [np.where(ids == k, 4.0, -4.0).astype(np.float32) + rng.normal(0.0, 3.0, ids.shape).astype(np.float32)
            for k in range(1, K + 1)]
    return [torch.from_numpy(m).to(dev).view(N, 1, H, W) for m in maps], torch.from_numpy(ids).to(dev)


def host_path(logits, palette):
    down = [x.cpu().numpy()[:, 0] for x in logits]     # K float32 maps a frame over the bus
    labels = object_merge.merge_labels(down)
    files = []
    for f in range(labels.shape[0]):
        im = Image.fromarray(labels[f], mode="P")
        im.putpalette(palette)
        b = io.BytesIO()
        im.save(b, "PNG")
        files.append(b.getvalue())
    return files


def ops_pair():
    logits, gt = object_logits()
    labels = torch.empty((N, H, W), dtype=torch.uint8, device=dev)
    files = torch.empty((N, ops.png_indexed_capacity(H, W)), dtype=torch.uint8, device=dev)
    lengths = torch.empty((N,), dtype=torch.int32, device=dev)
    counts = torch.empty((N, K, 6), dtype=torch.int32, device=dev)
    palette = object_merge.davis_palette().tobytes()

    def merge():
        ops.merge_objects(logits, out=labels)

    def png():
        ops.png_encode_indexed(labels, out=files, lengths=lengths)

    def count():
        ops.jf_counts_labels(labels, gt, K, out=counts)

    def together():
        merge()
        png()
        count()

    together()
    device_bytes = int(lengths.sum().item())
    host_files = host_path(logits, palette)  # warm-up
    rounds = []
    for _ in range(3):
        r = {"device_us_per_frame": round(time_us(together, args.reps) / N, 2)}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host_path(logits, palette)
        r["host_us_per_frame"] = round((time.perf_counter() - t0) * 1e6 / N, 1)   # (merge and file only: no counts)
        rounds.append(r)
    return {"rounds": rounds,
            "alone_us_per_frame": {"merge_objects": round(time_us(merge, args.reps) / N, 2),
                                   "png_encode_indexed": round(time_us(png, args.reps) / N, 2),
                                   "jf_counts_labels": round(time_us(count, args.reps) / N, 2)},
            "device_file_bytes_per_frame": device_bytes // N,
            "host_file_bytes_per_frame": sum(len(f) for f in host_files) // N,
            "host_download_bytes_per_frame": 4 * K * H * W, "device_download_bytes_per_frame": int(files.shape[1]) + 4}


class Provider:
    def __init__(self, network):
        self.network = network


def pass_pair():
    from torch.utils.data import DataLoader
    providers = []
    for seed in range(2, 2 + K):
        net = OSVOS_VGG(pretrained=0)
        net.load_state_dict(O.make_state_dict(seed))
        providers.append(Provider(net.to(dev).eval()))
    data = SyntheticObjectsSequence("bench", H, W, n_frames=args.frames, n_objects=K)
    held = [data[f] for f in range(args.frames)]  # the frames are generated once: the loader below only collates them
    loader = DataLoader(held, batch_size=1, shuffle=False, num_workers=0)
    binary = [(lambda seq, fname, k=k: (data.annotation(seq, fname) == k).astype(np.uint8)) for k in range(1, K + 1)]
    with tempfile.TemporaryDirectory() as tmp:
        def merged():
            experiment_helper.test_objects(providers, loader, os.path.join(tmp, "objects"), data.annotation, seq_name="bench")

        def k_passes():
            for k, p in enumerate(providers):
                experiment_helper.test_fast(p, loader, os.path.join(tmp, "fast%d" % k), binary[k], seq_name="bench")

        merged()
        k_passes()  # warm-up
        rounds = []
        for _ in range(3):
            r = {}
            for key, fn in (("test_objects", merged), ("k_runs_of_test_fast", k_passes)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                r[key] = {"frames_per_s": round(args.frames / dt, 1), "ms_per_frame": round(1e3 * dt / args.frames, 3)}
            rounds.append(r)
    return {"frames": args.frames, "rounds": rounds}


def main():
    result = {"bench": "multi_object", "device": torch.cuda.get_device_name(0), "size": "%dx%d" % (H, W), "objects": K,
              "frames_per_call": N, "ops": ops_pair(), "pass": pass_pair()}
    line = json.dumps(result)
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
