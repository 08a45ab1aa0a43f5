"""Offline training loop (train_offline._train, OSVOS_VGG on the HIP path) fed three ways on a DAVIS-shaped tree of
480x854 frames written to a temp dir: (a) the per-iteration DataLoader, (b) ResidentTrainSetLoader, (c) the same draws
pre-materialised as device tensors in a list (the upper bound for any loader).  Prints one JSON line: frames/s of each,
the loader's decode seconds and device bytes, and k_augment's mean time per sample (library launch profiler).

usage: python tools/offline_loader_probe.py [--seqs 3] [--frames 25] [--iters 150] [--dl-iters 20] [--only resident]
       (--only resident: (b) alone, for a `rocprofv3 --kernel-trace --stats -- python ...` run)
"""
import argparse
import itertools
import json
import os
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

import fosvos_hip  # noqa: E402
import train_offline  # noqa: E402
from dataloaders.resident import ResidentTrainSetLoader  # noqa: E402
from networks.osvos_vgg import OSVOS_VGG  # noqa: E402
from oracle import osvos_ref as O  # noqa: E402
from util import io_helper  # noqa: E402
from util.network_provider import VGGOfflineProvider  # noqa: E402

H, W = 480, 854


def write_tree(root: Path, n_seqs: int, n_frames: int) -> None:
    lines = []
    yy, xx = np.mgrid[0:H, 0:W]
    for s in range(n_seqs):
        seq = "seq%02d" % s
        (root / "JPEGImages" / "480p" / seq).mkdir(parents=True)
        (root / "Annotations" / "480p" / seq).mkdir(parents=True)
        rng = np.random.RandomState(s)
        for k in range(n_frames):
            base = (np.sin(xx / (20.0 + 5 * s) + k * 0.1)[..., None] * 60 + 128 +
                    rng.randint(-30, 30, size=(H, W, 3))).clip(0, 255).astype(np.uint8)
            Image.fromarray(base).save(str(root / "JPEGImages" / "480p" / seq / ("%05d.jpg" % k)), quality=90)
            cy, cx = 200 + 3 * k, 300 + 40 * s
            mask = (((yy - cy) / 120.0) ** 2 + ((xx - cx) / 180.0) ** 2 < 1).astype(np.uint8) * 255
            Image.fromarray(mask).save(str(root / "Annotations" / "480p" / seq / ("%05d.png" % k)))
            lines.append("/JPEGImages/480p/%s/%05d.jpg /Annotations/480p/%s/%05d.png \n" % (seq, k, seq, k))
    (root / "ImageSets" / "480p").mkdir(parents=True)
    for split in ("train", "val", "trainval"):
        (root / "ImageSets" / "480p" / (split + ".txt")).write_text("".join(lines))


class Take:
    """The first n minibatches of a loader, as one epoch."""

    def __init__(self, loader, n):
        self.loader, self.n = loader, n

    def __len__(self):
        return self.n

    def __iter__(self):
        return itertools.islice(iter(self.loader), self.n)


class Writer:
    def add_scalar(self, *a, **k):
        pass

    def close(self):
        pass


def make_provider():
    net = OSVOS_VGG(pretrained=0)
    net.load_state_dict(O.make_state_dict(0))
    prov = VGGOfflineProvider.__new__(VGGOfflineProvider)
    prov.network, prov.name = net.cuda(), "vgg16"
    return prov


def run(prov, loader) -> float:
    """frames/s of one epoch of train_offline._train over `loader` (a step every 10 iterations, as main() runs it)."""
    torch.manual_seed(7)
    train_offline.data_parallel = False
    ret = train_offline._train(prov, loader, None, prov.get_optimizer(), Writer(), 0, 1, 10, 10 ** 9, False, 5)
    return ret["iterations"] / ret["seconds"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seqs", type=int, default=3)
    ap.add_argument("--frames", type=int, default=25)
    ap.add_argument("--iters", type=int, default=150)
    ap.add_argument("--dl-iters", type=int, default=20)
    ap.add_argument("--only", choices=["resident"], default=None)
    args = ap.parse_args()
    out = {"frames": args.seqs * args.frames, "size": [H, W], "iters": args.iters, "dl_iters": args.dl_iters,
           "device": torch.cuda.get_device_name(0)}
    with tempfile.TemporaryDirectory() as tmp:
        root = Path(tmp)
        write_tree(root, args.seqs, args.frames)
        prov = make_provider()
        loader = io_helper.get_data_loader_train(str(root), 1, resident_set=True)
        out["decode_s"] = round(loader.decode_seconds, 3)
        out["device_bytes"] = loader.device_bytes
        torch.manual_seed(7)
        # the same draws (b) makes, held as device tensors: warm-up (every shape's arenas and plans) and bound (c)
        draws = list(Take(loader, args.iters))
        run(prov, draws)
        if args.only == "resident":
            out["resident_fps"] = round(run(prov, Take(loader, args.iters)), 1)
        else:
            out["resident_fps"] = round(run(prov, Take(loader, args.iters)), 1)
            out["materialised_fps"] = round(run(prov, draws), 1)
            out["resident_over_materialised"] = round(out["resident_fps"] / out["materialised_fps"], 3)
            dl = io_helper.get_data_loader_train(str(root), 1, resident=False)
            out["dataloader_fps"] = round(run(prov, Take(dl, args.dl_iters)), 2)
            out["resident_over_dataloader"] = round(out["resident_fps"] / out["dataloader_fps"], 1)
            del draws
            # the kernel alone: the library's launch profiler brackets every k_augment launch with events
            torch.cuda.synchronize()
            with fosvos_hip.LaunchProfile(0) as prof:
                for _ in Take(loader, 200):
                    pass
            rec = prof.records.get("k_augment")
            if rec:
                out["augment_us_per_sample"] = round(1e3 * rec["ms"] / rec["launches"], 2)
            t0 = time.perf_counter()
            for _ in Take(loader, 200):
                pass
            torch.cuda.synchronize()
            out["loader_alone_us_per_sample"] = round(1e6 * (time.perf_counter() - t0) / 200, 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
