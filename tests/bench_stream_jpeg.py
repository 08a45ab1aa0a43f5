"""The device JPEG encoder on one MI355X (csrc/jpeg.hip, ``FrameSegmenter(encode='jpeg')``).  Two measurements, one JSON line
(also written to profiles/stream_jpeg_bench.json):

* the encoder alone: microseconds per frame of ``ops.jpeg_encode`` (quality 90, BGR) at 1 and 5 frames a call, 480x854 and
  1080x1920, from HIP events after a warm-up, against PIL's ``save(..., 'JPEG')`` of the same frames with the same parameters
  on one host core (wall clock); the encoded size;
* ``FrameSegmenter.segment`` at depth 2 with ``encode='jpeg'`` (the loop of ``run_webcam.py --output-format jpeg`` up to the
  file write: the bytes are there) against ``encode=None`` followed by PIL's PNG save into memory (what ``--output`` does
  today, up to the file write).  VGG at 480x854 and ResNet-18 at 1080x1920, seeded weights, frames of the synthetic sequence
  pre-generated in host memory, three alternating rounds after a warm-up; frames/s of each, bytes over the bus per frame,
  and the frames that took the second copy.
A diagnostic, not the headline metric - bench.py stays on the fine-tune.
usage: python tests/bench_stream_jpeg.py [--json profiles/stream_jpeg_bench.json] [--frames 12] [--reps 50]"""
import argparse
import io
import json
import os
import sys
import time

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "fosvos_amd"))

import run_webcam  # noqa: E402
from fosvos_hip import ops  # noqa: E402
from fosvos_hip.stream import FrameSegmenter  # noqa: E402
from networks.osvos_resnet import OSVOS_RESNET  # noqa: E402
from networks.osvos_vgg import OSVOS_VGG  # noqa: E402
from oracle import osvos_ref as O  # noqa: E402  (seeded weights only)
from util import jpeg_layout  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "stream_jpeg_bench.json"))
ap.add_argument("--frames", type=int, default=12)
ap.add_argument("--reps", type=int, default=50)
args = ap.parse_args()
dev = "cuda:0"
assert torch.cuda.is_available(), "bench_stream_jpeg.py measures on the GPU; there is no CPU timing"
SIZES = [(480, 854), (1080, 1920)]
QUALITY = 90
_FRAMES = {}


def camera(h, w, count):
    """Frames of the synthetic sequence with sensor noise on top, generated once."""
    have = _FRAMES.setdefault((h, w), [])
    rng = np.random.default_rng(h + len(have))
    while len(have) < count:
        f = run_webcam.synthetic_frame(h, w, len(have)).astype(np.int16) + rng.integers(-3, 4, (h, w, 3))
        have.append(np.clip(f, 0, 255).astype(np.uint8))
    return have[:count]


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


def pil_jpeg(frame):
    b = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(frame[:, :, ::-1])).save(b, "JPEG", quality=QUALITY, subsampling=0, optimize=False,
                                                                  restart_marker_blocks=jpeg_layout.RI)
    return b.getvalue()


def pil_png(out):
    b = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(out[:, :, ::-1])).save(b, "PNG")
    return b.getvalue()


def kernels():
    out = {}
    for h, w in SIZES:
        frames = camera(h, w, 5)
        t0 = time.perf_counter()
        files = [pil_jpeg(f) for f in frames]
        pil_us = (time.perf_counter() - t0) * 1e6 / len(frames)
        for n in (1, 5):
            x = torch.from_numpy(np.stack(frames[:n])).to(dev)
            buf = torch.empty((n, ops.jpeg_capacity(h, w, 3)), dtype=torch.uint8, device=dev)
            lengths = torch.empty((n,), dtype=torch.int32, device=dev)
            us = time_us(lambda: ops.jpeg_encode(x, QUALITY, out=buf, lengths=lengths), args.reps)
            lens = lengths.cpu().tolist()
            same = all(buf[k, :lens[k]].cpu().numpy().tobytes() == files[k] for k in range(n))
            out["jpeg_encode_%dx%dx%d" % (n, h, w)] = {
                "us_per_frame": round(us / n, 2), "pil_us_per_frame": round(pil_us, 1), "bytes_per_frame": int(sum(lens) / n),
                "raw_bytes_per_frame": h * w * 3, "equal_to_pils_files": same}
    return out


def pipeline(name, net, h, w):
    frames = camera(h, w, args.frames)
    plain = FrameSegmenter(net, h, w, depth=2)
    coded = FrameSegmenter(net, h, w, depth=2, encode="jpeg", quality=QUALITY)

    def run_png():
        return [pil_png(a) for a in plain.segment(frames)]

    def run_jpeg():
        return list(coded.segment(frames))

    pngs, jpegs = run_png(), run_jpeg()  # warm-up
    coded.second_copies = coded.bytes_down = 0
    rounds = []
    for _ in range(3):
        r = {}
        for key, fn in (("jpeg_on_device", run_jpeg), ("png_by_pil", run_png)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            r[key] = {"fps": round(len(frames) / dt, 1), "ms_per_frame": round(1e3 * dt / len(frames), 3)}
        rounds.append(r)
    n = 3 * len(frames)
    result = {"net": name, "size": "%dx%d" % (h, w), "frames": len(frames), "quality": QUALITY, "rounds": rounds,
              "jpeg_ahead_in_every_round": all(r["jpeg_on_device"]["fps"] > r["png_by_pil"]["fps"] for r in rounds),
              "jpeg_file_bytes_per_frame": int(sum(len(f) for f in jpegs) / len(jpegs)),
              "png_file_bytes_per_frame": int(sum(len(f) for f in pngs) / len(pngs)),
              "bus_bytes_per_frame_jpeg": int(coded.bytes_down / n), "bus_bytes_per_frame_raw": h * w * 3,
              "download_budget_bytes": coded.budget, "frames_with_second_copy": coded.second_copies, "frames_timed": n}
    plain.close()
    coded.close()
    return result


def main():
    vgg = OSVOS_VGG(pretrained=0)
    vgg.load_state_dict(O.make_state_dict(2))
    torch.manual_seed(7)
    resnet = OSVOS_RESNET(pretrained=False, version=18)
    result = {"bench": "stream_jpeg", "device": torch.cuda.get_device_name(0), "kernels": kernels(),
              "pipeline": [pipeline("vgg", vgg.to(dev).eval(), 480, 854),
                           pipeline("resnet18", resnet.to(dev).eval(), 1080, 1920)]}
    line = json.dumps(result)
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
