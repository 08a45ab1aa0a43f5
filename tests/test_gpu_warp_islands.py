"""fosvos_warp_sample on islands (tests/islands.py): frame, mask and the two value tables in; image and gt out; the
workspace.  A matrix decides which bytes of the frame a thread asks for, so the cases are the ones that ask for the most
outside of it: a shear with a shift (taps beyond all four sides) and a translation far off the frame, each with and without
the renormalisation.  Nothing outside the operands is read or written, and the workspace is used up to exactly the bytes
fosvos_warp_workspace_bytes reports."""
import os
import sys
import zlib

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fosvos_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import islands as I  # noqa: E402
from dataloaders import custom_transforms as T  # noqa: E402
from test_augment_rotate_cpu import _dataset, sample_bytes  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, U8 = torch.float32, torch.uint8
MATRICES = {"shear": np.array([[1.0, 0.3, -4.5], [-0.2, 1.1, 3.25]]),
            "far": np.array([[1.0, 0.0, 1000.0], [0.0, 1.0, 1000.0]])}


def _renormalized(tmp):
    if tmp.min() < 0.0:
        tmp = tmp - tmp.min()
    if tmp.max() > 1.0:
        tmp = tmp / tmp.max()
    return tmp


@pytest.mark.parametrize("size,offset", [((33, 130), 7), ((13, 17), 0)])
def test_warp_touches_nothing_outside_its_operands(size, offset):
    from fosvos_hip import check, lib
    L = lib()
    h, w = size
    ds = _dataset()
    img, lab = sample_bytes(h, w)
    ramp = np.repeat(np.arange(256, dtype=np.uint8)[:, None, None], 3, axis=2)
    img_lut = np.ascontiguousarray(ds.convert_raw(ramp, None)[0].reshape(256, 3))
    gt_lut = np.arange(256, dtype=np.float32) / np.float32(max(float(lab.max()), 1e-8))
    need = int(L.fosvos_warp_workspace_bytes(h, w))
    assert need > 0
    rep = I.Report("warp %dx%d" % size)
    for name, matrix in MATRICES.items():
        inv = np.linalg.inv(np.vstack([matrix, [0.0, 0.0, 1.0]]))
        coeff = [float(v) for v in inv[:2].reshape(-1)]
        for flip in (False, True):
            image, gt = ds.convert_raw(img, lab)
            if flip:
                image, gt = np.ascontiguousarray(image[:, ::-1]), np.ascontiguousarray(gt[:, ::-1])
            warped = {"image": T.warp_affine(image, matrix), "gt": T.warp_affine(gt, matrix)}
            for renormalize in (False, True):
                want = T.ToTensor()({k: (_renormalized(v) if renormalize else v) for k, v in warped.items()})
                operands = [I.inp("frame", torch.from_numpy(img), is_map=False, offset=offset),
                            I.inp("mask", torch.from_numpy(lab), is_map=False, offset=(offset + 5) % 16),
                            I.inp("img_lut", torch.from_numpy(img_lut)), I.inp("gt_lut", torch.from_numpy(gt_lut)),
                            I.out("image", (1, 3, h, w), F32, is_map=False), I.out("gt", (1, 1, h, w), F32, is_map=False)]
                if renormalize:
                    operands.append(I.workspace("workspace", need))

                def call(isl, renormalize=renormalize, flip=flip, coeff=coeff):
                    check(L.fosvos_warp_sample(isl.ptr("frame"), isl.ptr("mask"), h, w, 1 if flip else 0, *coeff,
                                               isl.ptr("img_lut"), isl.ptr("gt_lut"), isl.ptr("image"), isl.ptr("gt"),
                                               1 if renormalize else 0, isl.ptr("workspace") if renormalize else None,
                                               need if renormalize else 0, 0, torch.cuda.current_stream(0).cuda_stream),
                          "warp_sample")

                tag = "%s flip=%d renormalize=%d" % (name, flip, renormalize)
                rep.add(I.run_case(tag, operands, call, {"image": want["image"].unsqueeze(0), "gt": want["gt"].unsqueeze(0)},
                                   device=DEV, seed=zlib.crc32(tag.encode()) & 0xFFFF))
    rep.done()
