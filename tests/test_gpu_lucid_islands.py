"""fosvos_lucid_sample on islands (tests/islands.py): frame, filled background, mask and the two value tables in; image and gt
out; no workspace.  The two matrices and the mask decide which bytes a thread asks for, so the cases are the ones that ask for
the most outside of the frame: a shear with a shift under either matrix (taps beyond all four sides), a translation that maps
every corner off the frame under both, a drawn pair, and no object at all.  Nothing outside the operands is read or written."""
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
from dataloaders import lucid as L  # noqa: E402
from test_augment_lucid_cpu import FAR, ONE, SHEAR, ZERO, drawn_pairs, luts, sample  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = torch.float32
GAIN, BIAS = np.array([1.1, 0.9, 1.05], np.float32), np.array([3.0, -2.0, 0.5], np.float32)


@pytest.mark.parametrize("size,offset", [((19, 70), 7), ((43, 165), 0)])
def test_lucid_touches_nothing_outside_its_operands(size, offset):
    from fosvos_hip import check, lib
    lib_ = lib()
    h, w = size
    frame, background, mask = sample(h, w)
    img_lut, gt_lut = luts(mask)
    rep = I.Report("lucid %dx%d" % size)
    for flip in (False, True):
        pairs = [("shear/shear", SHEAR, SHEAR, GAIN, BIAS), ("far/far", FAR, FAR, ONE, ZERO), ("shear/none", SHEAR, None, GAIN, ZERO),
                 ("drawn",) + drawn_pairs(h, w, mask, flip, n=1)[0]]
        for name, m_bg, m_fg, gain, bias in pairs:
            want_img, want_gt = L.compose(frame, background, mask, img_lut, gt_lut, flip, m_bg, m_fg, gain, bias)
            inv = [np.linalg.inv(np.vstack([m, [0.0, 0.0, 1.0]])) for m in (m_bg, np.eye(3)[:2] if m_fg is None else m_fg)]
            coeff = [float(v) for m in inv for v in m[:2].reshape(-1)]
            scalars = [float(v) for v in gain] + [float(v) for v in bias]
            operands = [I.inp("frame", torch.from_numpy(frame), is_map=False, offset=offset),
                        I.inp("background", torch.from_numpy(background), is_map=False, offset=(offset + 2) % 16),
                        I.inp("mask", torch.from_numpy(mask), is_map=False, offset=(offset + 5) % 16),
                        I.inp("img_lut", torch.from_numpy(img_lut)), I.inp("gt_lut", torch.from_numpy(gt_lut)),
                        I.out("image", (1, 3, h, w), F32, is_map=False), I.out("gt", (1, 1, h, w), F32, is_map=False)]

            def call(isl, flip=flip, coeff=coeff, scalars=scalars, fg_on=m_fg is not None):
                check(lib_.fosvos_lucid_sample(isl.ptr("frame"), isl.ptr("background"), isl.ptr("mask"), h, w, 1 if flip else 0,
                                               *coeff, 1 if fg_on else 0, *scalars, isl.ptr("img_lut"), isl.ptr("gt_lut"),
                                               isl.ptr("image"), isl.ptr("gt"), 0, torch.cuda.current_stream(0).cuda_stream),
                      "lucid_sample")

            tag = "%s flip=%d" % (name, flip)
            want = {"image": torch.from_numpy(np.ascontiguousarray(want_img.transpose(2, 0, 1)))[None],
                    "gt": torch.from_numpy(want_gt)[None, None]}
            rep.add(I.run_case(tag, operands, call, want, device=DEV, seed=zlib.crc32(tag.encode()) & 0xFFFF))
    rep.done()
