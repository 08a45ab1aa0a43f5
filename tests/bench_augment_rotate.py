"""Rotating and zooming the training sample on one MI355X: ``ops.warp_sample`` alone (with and without the reference's
renormalisation, HIP events) beside ``ops.augment_sample`` at scale 1 and 0.8 on the same operands and beside the host path
(``custom_transforms.warp_affine`` on frame and mask plus the upload), and ``train_online._train`` on a one-sequence 480x854
DAVIS tree written to a temporary directory, with and without ``rotate``, in alternating pairs in one process (the leg without
it is the loop with the six precomputed variants).  Asserts equality with the numpy definition once at 480x854 before it
times anything.  Prints ONE JSON line and writes it to profiles/augment_rotate_bench.json.

    python tests/bench_augment_rotate.py [--pairs 3] [--epochs 400] [--reps 200]

Timing: the op from events around ``reps`` back-to-back calls after a warm-up; the loop from a host clock around whole
`_train` calls, which end in a device synchronise, after a warm-up call of each leg."""
import argparse
import json
import os
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "fosvos_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import osvos_ref as O  # noqa: E402

DEV = "cuda:0"
H, W = 480, 854
ACCUM = 5
TABLES = (("col_taps", np.int32), ("col_w", np.float32), ("row_taps", np.int32), ("row_w", np.float32),
          ("col_near", np.int32), ("row_near", np.int32))


class _NullWriter:
    def add_scalar(self, *a, **k):
        pass

    def close(self):
        pass


def event_us(fn, reps):
    for _ in range(10):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / reps


def bench_op(args):
    from dataloaders import custom_transforms as T
    from dataloaders.davis_2016 import DAVIS2016, MEANVAL
    from fosvos_hip import ops
    ds = DAVIS2016.__new__(DAVIS2016)
    ds.meanval = MEANVAL
    rng = np.random.RandomState(7)
    img = rng.randint(0, 256, size=(H, W, 3)).astype(np.uint8)
    lab = np.where(rng.rand(H, W) > 0.5, 255, 0).astype(np.uint8)
    ramp = np.repeat(np.arange(256, dtype=np.uint8)[:, None, None], 3, axis=2)
    img_lut = torch.from_numpy(np.ascontiguousarray(ds.convert_raw(ramp, None)[0].reshape(256, 3))).to(DEV)
    gt_lut = torch.from_numpy(np.arange(256, dtype=np.float32) / np.float32(255.0)).to(DEV)
    frame, mask = torch.from_numpy(img).to(DEV), torch.from_numpy(lab).to(DEV)
    image, gt = torch.empty((1, 3, H, W), device=DEV), torch.empty((1, 1, H, W), device=DEV)
    ws = torch.empty(ops.warp_workspace_bytes(H, W), dtype=torch.uint8, device=DEV)
    matrix = T.rotation_matrix((W / 2, H / 2), 17.0, 1.1)

    # equality with the numpy definition, once, at the size that is timed
    image_f, gt_f = ds.convert_raw(img, lab)
    t0 = time.perf_counter()
    want_img, want_gt = T.warp_affine(image_f, matrix), T.warp_affine(gt_f, matrix)
    host_warp_s = time.perf_counter() - t0
    for renormalize in (False, True):
        ops.warp_sample(frame, mask, False, matrix, img_lut, gt_lut, image, gt, renormalize=renormalize, workspace=ws)
        ref = T.ScaleNRotate([17.0], [1.1], renormalize=True).apply({"image": image_f}, 17.0, 1.1)["image"] \
            if renormalize else want_img
        assert np.array_equal(image[0].permute(1, 2, 0).cpu().numpy().view(np.uint32), ref.view(np.uint32)), renormalize
        assert np.array_equal(gt[0, 0].cpu().numpy().view(np.uint32), want_gt.view(np.uint32)), renormalize

    out = {"size": [H, W], "matrix": "rotation 17 degrees, zoom 1.1", "unit": "us per sample", "reps": args.reps,
           "equal_to_numpy": True}
    out["warp_sample"] = event_us(lambda: ops.warp_sample(frame, mask, False, matrix, img_lut, gt_lut, image, gt), args.reps)
    out["warp_sample_renormalize"] = event_us(
        lambda: ops.warp_sample(frame, mask, False, matrix, img_lut, gt_lut, image, gt, renormalize=True, workspace=ws), args.reps)
    out["augment_sample_scale_1"] = event_us(lambda: ops.augment_sample(frame, mask, False, img_lut, gt_lut, image, gt), args.reps)
    plan = T.resize_plan(H, W, 0.8, 0.8)
    tables = tuple(torch.from_numpy(np.ascontiguousarray(plan[k], dtype=dt)).to(DEV) for k, dt in TABLES)
    image8 = torch.empty((1, 3, plan["oh"], plan["ow"]), device=DEV)
    gt8 = torch.empty((1, 1, plan["oh"], plan["ow"]), device=DEV)
    out["augment_sample_scale_0.8"] = event_us(
        lambda: ops.augment_sample(frame, mask, False, img_lut, gt_lut, image8, gt8, tables), args.reps)

    # the host path: the numpy warp of frame and mask, then the upload of both tensors
    def upload():
        a = torch.from_numpy(np.ascontiguousarray(want_img.transpose(2, 0, 1)))[None].to(DEV)
        b = torch.from_numpy(want_gt)[None, None].to(DEV)
        torch.cuda.synchronize()
        return a, b

    upload()
    t0 = time.perf_counter()
    for _ in range(5):
        upload()
    out["host_warp_affine_s"] = host_warp_s
    out["host_upload_s"] = (time.perf_counter() - t0) / 5
    return out


def bench_loop(args):
    import train_online
    from fosvos_hip.options import RotateOptions
    from networks.osvos_vgg import OSVOS_VGG
    from test_resident_set_cpu import write_davis_tree
    from util import io_helper
    from util.network_provider import VGGOnlineProvider
    net = OSVOS_VGG(pretrained=0)
    net.load_state_dict(O.make_state_dict(2))
    prov = VGGOnlineProvider.__new__(VGGOnlineProvider)
    prov.network = net.to(DEV)
    prov.name = "vgg16"
    prov.save_model = lambda *a, **k: None
    opt = prov.get_optimizer()
    train_online.data_parallel = False
    with tempfile.TemporaryDirectory() as tmp:
        root = write_davis_tree(Path(tmp), seqs={"a": (2, H, W)}, train=["a"])
        torch.manual_seed(1)
        loaders = {"plain": io_helper.get_data_loader_train(str(root), 1, "a"),
                   "rotate": io_helper.get_data_loader_train(str(root), 1, "a", rotate=RotateOptions())}

    def run(leg, n_epochs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ret = train_online._train(prov, loaders[leg], opt, _NullWriter(), "a", 0, n_epochs, ACCUM, 10 ** 9)
        torch.cuda.synchronize()
        return ret["iterations"] / (time.perf_counter() - t0)

    for leg in loaders:
        run(leg, 60)
    pairs = [{leg: run(leg, args.epochs) for leg in loaders} for _ in range(args.pairs)]
    plain = [p["plain"] for p in pairs]
    ratios = [p["rotate"] / p["plain"] for p in pairs]
    return {"size": [H, W], "avg_grad_every_n": ACCUM, "epochs_per_leg": args.epochs, "unit": "frames/s", "pairs_fps": pairs,
            "rotate_over_plain": ratios, "plain_pair_to_pair_spread": (max(plain) - min(plain)) / min(plain),
            "rotate_slower_than_the_spread": max(ratios) < 1.0 - (max(plain) - min(plain)) / min(plain)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--epochs", type=int, default=400, help="epochs (= frames) per timed leg")
    ap.add_argument("--reps", type=int, default=200, help="calls per timed op")
    args = ap.parse_args()
    result = {"bench": "augment_rotate", "device": torch.cuda.get_device_name(0), "op": bench_op(args), "loop": bench_loop(args)}
    line = json.dumps(result)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "augment_rotate_bench.json"), "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
