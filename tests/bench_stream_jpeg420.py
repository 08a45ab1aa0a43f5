"""The 4:2:0 form of the device JPEG encoder against its 4:4:4 form on one MI355X, in one process.  One JSON line (also
written to profiles/stream_jpeg420_bench.json):

* ``ops.jpeg_encode`` (quality 90, BGR) with ``subsampling='4:4:4'`` and ``'4:2:0'``: five 480x854 frames a call and one
  1080x1920 frame, microseconds per frame from HIP events after a warm-up, three alternating rounds; the file sizes of
  both, and whether the 4:2:0 files are PIL's;
* the loop of ``run_webcam.py`` (``loop_frames`` over ``FrameSegmenter.segment``, VGG at 480x854, seeded weights, frames of
  the synthetic sequence pre-generated in host memory) writing one Motion-JPEG AVI (4:2:0) against writing ``%05d.jpg``
  files (4:4:4, what ``--output-format jpeg`` does without the new flags), three alternating rounds after a warm-up.
A diagnostic, not the headline metric - bench.py stays on the fine-tune.
usage: python tests/bench_stream_jpeg420.py [--json profiles/stream_jpeg420_bench.json] [--frames 12] [--reps 50]"""
import argparse
import io
import json
import os
import shutil
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

import run_webcam  # noqa: E402
from fosvos_hip import ops  # noqa: E402
from fosvos_hip.stream import FrameSegmenter  # noqa: E402
from networks.osvos_vgg import OSVOS_VGG  # noqa: E402
from oracle import osvos_ref as O  # noqa: E402  (seeded weights only)
from util import jpeg_layout  # noqa: E402
from util.mjpeg_avi import AviWriter  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "stream_jpeg420_bench.json"))
ap.add_argument("--frames", type=int, default=12)
ap.add_argument("--reps", type=int, default=50)
args = ap.parse_args()
dev = "cuda:0"
assert torch.cuda.is_available(), "bench_stream_jpeg420.py measures on the GPU; there is no CPU timing"
QUALITY = 90
SAMPLINGS = ("4:4:4", "4:2:0")
_FRAMES = {}


def camera(h, w, count):
    """Frames of the synthetic sequence with sensor noise on top, generated once."""
    have = _FRAMES.setdefault((h, w), [])
    rng = np.random.default_rng(h + len(have))
    while len(have) < count:
        f = run_webcam.synthetic_frame(h, w, len(have)).astype(np.int16) + rng.integers(-3, 4, (h, w, 3))
        have.append(np.clip(f, 0, 255).astype(np.uint8))
    return have[:count]


def event_us(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def pil_420(frame):
    b = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(frame[:, :, ::-1])).save(b, "JPEG", quality=QUALITY, subsampling=2, optimize=False,
                                                                  restart_marker_blocks=jpeg_layout.RI_420)
    return b.getvalue()


def kernels():
    out = {}
    for n, h, w in ((5, 480, 854), (1, 1080, 1920)):
        frames = camera(h, w, n)
        x = torch.from_numpy(np.stack(frames)).to(dev)
        calls, bufs = {}, {}
        for s in SAMPLINGS:
            buf = torch.empty((n, ops.jpeg_capacity(h, w, 3, s)), dtype=torch.uint8, device=dev)
            lengths = torch.empty((n,), dtype=torch.int32, device=dev)
            bufs[s] = (buf, lengths)
            calls[s] = (lambda s=s, buf=buf, lengths=lengths: ops.jpeg_encode(x, QUALITY, out=buf, lengths=lengths, subsampling=s))
            for _ in range(5):
                calls[s]()
        torch.cuda.synchronize()
        rounds = [{s: round(event_us(calls[s], args.reps) / n, 2) for s in SAMPLINGS} for _ in range(3)]
        lens = {s: bufs[s][1].cpu().tolist() for s in SAMPLINGS}
        buf, _ = bufs["4:2:0"]
        same = all(buf[k, :lens["4:2:0"][k]].cpu().numpy().tobytes() == pil_420(frames[k]) for k in range(n))
        out["jpeg_encode_%dx%dx%d" % (n, h, w)] = {
            "us_per_frame_rounds": rounds,
            "us_per_frame_median": {s: sorted(r[s] for r in rounds)[1] for s in SAMPLINGS},
            "bytes_per_frame": {s: int(sum(lens[s]) / n) for s in SAMPLINGS}, "raw_bytes_per_frame": h * w * 3,
            "files_420_equal_to_pils": same}
    return out


def loops(net, h, w):
    frames = camera(h, w, args.frames)
    plain = FrameSegmenter(net, h, w, depth=2, encode="jpeg", quality=QUALITY)
    sampled = FrameSegmenter(net, h, w, depth=2, encode="jpeg", quality=QUALITY, subsampling="4:2:0")
    work = Path(tempfile.mkdtemp(prefix="bench_jpeg420_"))
    sizes = {}

    def run_jpg():
        d = work / "jpg"
        d.mkdir(exist_ok=True)
        run_webcam.loop_frames(plain.segment(frames), d)
        sizes["jpg_444_directory"] = sum(p.stat().st_size for p in d.iterdir())

    def run_avi():
        with AviWriter(work / "x.avi", w, h, 25) as avi:
            run_webcam.loop_frames(sampled.segment(frames), None, avi=avi)
        sizes["avi_420_file"] = (work / "x.avi").stat().st_size

    run_webcam.log.setLevel("WARNING")  # (a log line a frame is not what is measured)
    try:
        run_jpg(), run_avi()  # warm-up
        rounds = []
        for _ in range(3):
            r = {}
            for key, fn in (("avi_420", run_avi), ("jpg_444", run_jpg)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                r[key] = {"fps": round(len(frames) / dt, 1), "ms_per_frame": round(1e3 * dt / len(frames), 3)}
            rounds.append(r)
    finally:
        plain.close()
        sampled.close()
        shutil.rmtree(str(work), ignore_errors=True)
    return {"net": "vgg", "size": "%dx%d" % (h, w), "frames": len(frames), "quality": QUALITY, "rounds": rounds,
            "bytes_written_per_frame": {k: int(v / len(frames)) for k, v in sizes.items()}}


def main():
    vgg = OSVOS_VGG(pretrained=0)
    vgg.load_state_dict(O.make_state_dict(2))
    result = {"bench": "stream_jpeg420", "device": torch.cuda.get_device_name(0), "kernels": kernels(),
              "loop": loops(vgg.to(dev).eval(), 480, 854)}
    line = json.dumps(result)
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
