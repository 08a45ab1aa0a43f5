"""Moving the object against its background on one MI355X: ``ops.lucid_sample`` alone (HIP events) beside ``ops.warp_sample``
on the same operands, and ``train_online._train`` on a one-sequence 480x854 DAVIS tree written to a temporary directory, with
and without ``lucid``, in alternating pairs in one process (the leg without it is the loop with the six precomputed variants).
Asserts equality with ``lucid.compose`` once at 480x854 before it times anything.  Prints ONE JSON line and writes it to
profiles/augment_lucid_bench.json.

    python tests/bench_augment_lucid.py [--pairs 3] [--epochs 400] [--reps 200]

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
from bench_augment_rotate import ACCUM, DEV, H, W, _NullWriter, event_us  # noqa: E402


def bench_op(args):
    from dataloaders import custom_transforms as T
    from dataloaders import lucid as L
    from dataloaders.davis_2016 import DAVIS2016, MEANVAL
    from fosvos_hip import ops
    from fosvos_hip.options import LucidOptions
    ds = DAVIS2016.__new__(DAVIS2016)
    ds.meanval = MEANVAL
    rng = np.random.RandomState(7)
    img = rng.randint(0, 256, size=(H, W, 3)).astype(np.uint8)
    y, x = np.mgrid[:H, :W]
    lab = np.where(((y - 250) / 120.0) ** 2 + ((x - 400) / 170.0) ** 2 <= 1.0, 255, 0).astype(np.uint8)  # 15.6 % of the frame
    opts = LucidOptions()
    t0 = time.perf_counter()
    filled = L.fill_background(img, lab, opts.dilate, opts.smooth)
    host_fill_s = time.perf_counter() - t0
    ramp = np.repeat(np.arange(256, dtype=np.uint8)[:, None, None], 3, axis=2)
    img_lut_h = np.ascontiguousarray(ds.convert_raw(ramp, None)[0].reshape(256, 3))
    gt_lut_h = np.arange(256, dtype=np.float32) / np.float32(255.0)
    img_lut, gt_lut = torch.from_numpy(img_lut_h).to(DEV), torch.from_numpy(gt_lut_h).to(DEV)
    frame, background, mask = (torch.from_numpy(a).to(DEV) for a in (img, filled, lab))
    image, gt = torch.empty((1, 3, H, W), device=DEV), torch.empty((1, 1, H, W), device=DEV)
    draws = L.Draws(7.0, 1.1, -11.0, 1.08, 0.1, -0.12, 1.1, 0.97, 1.0, 1.04, 9.0)
    m_bg, m_fg, gain, bias = opts.dream().matrices(draws, L.mask_box(lab), (H, W))

    # equality with the numpy definition, once, at the size that is timed
    t0 = time.perf_counter()
    want_img, want_gt = L.compose(img, filled, lab, img_lut_h, gt_lut_h, False, m_bg, m_fg, gain, bias)
    host_compose_s = time.perf_counter() - t0
    ops.lucid_sample(frame, background, mask, False, m_bg, m_fg, gain, bias, img_lut, gt_lut, image, gt)
    assert np.array_equal(image[0].permute(1, 2, 0).cpu().numpy().view(np.uint32), want_img.view(np.uint32))
    assert np.array_equal(gt[0, 0].cpu().numpy().view(np.uint32), want_gt.view(np.uint32))
    alpha = L.object_alpha(lab, m_fg)

    out = {"size": [H, W], "draws": list(draws), "unit": "us per sample", "reps": args.reps, "equal_to_numpy": True,
           "pixels_alpha_1": float((alpha == 1).mean()), "pixels_blended": float(((alpha > 0) & (alpha < 1)).mean())}
    out["lucid_sample"] = event_us(
        lambda: ops.lucid_sample(frame, background, mask, False, m_bg, m_fg, gain, bias, img_lut, gt_lut, image, gt), args.reps)
    out["lucid_sample_no_object"] = event_us(
        lambda: ops.lucid_sample(frame, background, mask, False, m_bg, None, gain, bias, img_lut, gt_lut, image, gt), args.reps)
    out["warp_sample"] = event_us(lambda: ops.warp_sample(frame, mask, False, m_bg, img_lut, gt_lut, image, gt), args.reps)
    out["warp_sample_rotation_17_zoom_1.1"] = event_us(
        lambda: ops.warp_sample(frame, mask, False, T.rotation_matrix((W / 2, H / 2), 17.0, 1.1), img_lut, gt_lut, image, gt),
        args.reps)
    out["lucid_over_warp"] = out["lucid_sample"] / out["warp_sample"]
    out["host_compose_s"] = host_compose_s
    out["host_fill_background_s"] = host_fill_s
    return out


def bench_loop(args):
    import train_online
    from fosvos_hip.options import LucidOptions
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
                   "lucid": io_helper.get_data_loader_train(str(root), 1, "a", lucid=LucidOptions())}

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
    ratios = [p["lucid"] / p["plain"] for p in pairs]
    return {"size": [H, W], "avg_grad_every_n": ACCUM, "epochs_per_leg": args.epochs, "unit": "frames/s", "pairs_fps": pairs,
            "lucid_over_plain": ratios, "plain_pair_to_pair_spread": (max(plain) - min(plain)) / min(plain),
            "note": "the plain leg draws among three scales (two of them smaller frames); the lucid leg always trains at 480x854"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--epochs", type=int, default=400, help="epochs (= frames) per timed leg")
    ap.add_argument("--reps", type=int, default=200, help="calls per timed op")
    args = ap.parse_args()
    result = {"bench": "augment_lucid", "device": torch.cuda.get_device_name(0), "op": bench_op(args), "loop": bench_loop(args)}
    line = json.dumps(result)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "augment_lucid_bench.json"), "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
