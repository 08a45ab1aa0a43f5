"""The fitted-Huffman form of the device PNG encoder on a real MI355X: ``ops.png_encode(x, huffman='fitted')`` against
``png_layout.encode(img, huffman='fitted')`` byte for byte (no tolerance anywhere), and ``test_fast(png_huffman='fitted')``
against the fixed pass."""
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from oracle import osvos_ref as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fosvos_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from util import experiment_helper, io_helper, png_layout as P  # noqa: E402
import test_png_fitted_cpu as C  # noqa: E402  (the images)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILL = 0xA5
_WANT = {}


def want(name, img, huffman="fitted"):
    """The layout's file of a case, computed once."""
    key = (name, huffman)
    if key not in _WANT:
        _WANT[key] = P.encode(img, huffman=huffman)
    return _WANT[key]


def dirty_workspace():
    from fosvos_hip import ops
    torch.cuda.synchronize()
    for buf in ops._WS._buf.values():
        buf.fill_(FILL)


def encode_checked(name, frames, huffman="fitted"):
    """``frames`` uint8 [N,H,W] through the encoder into a 0xA5 buffer: every file equals the layout's, nothing behind it is
    written.  Returns (buffer, lengths) on the host."""
    from fosvos_hip import ops
    x = torch.from_numpy(np.ascontiguousarray(frames)).to(DEV)
    n, h, w = frames.shape
    out = torch.full((n, ops.png_capacity(h, w) + 9), FILL, dtype=torch.uint8, device=DEV)
    lengths = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    dirty_workspace()
    ops.png_encode(x, out=out, lengths=lengths, huffman=huffman)
    torch.cuda.synchronize()
    got, lens = out.cpu().numpy(), lengths.cpu().tolist()
    for k in range(n):
        ref = want("%s[%d]" % (name, k), frames[k], huffman)
        assert lens[k] == len(ref), (name, k, lens[k], len(ref))
        same = np.frombuffer(ref, dtype=np.uint8) == got[k, :lens[k]]
        assert same.all(), (name, k, "first differing byte", int(np.flatnonzero(~same)[0]), "of", len(ref))
        assert (got[k, lens[k]:] == FILL).all(), (name, k)
    return got, lens


@pytest.mark.parametrize("name", list(C.CASES))
def test_fitted_bytes_match_the_layout(name):
    img = C.CASES[name]
    got, lens = encode_checked(name, img[None])
    again, lens_again = encode_checked(name, img[None])      # a second call is bit-identical
    assert lens == lens_again and np.array_equal(got, again)
    if name in ("96x160_noise16", "lucas", "37x53_noisy_ellipse"):
        assert "fitted" in [f for _, f in P.encode_segment_forms(img, "fitted")]


def test_five_frames_of_mixed_forms_in_one_call():
    names = ["96x160_noisy_ellipse", "96x160_noise256", "96x160_constant", "96x160_noise16", "96x160_runs_and_rests"]
    frames = np.stack([C.CASES[k] for k in names])
    forms = {f for img in frames for _, f in P.encode_segment_forms(img, "fitted")}
    assert forms == {"fixed", "stored", "fitted"}
    got, lens = encode_checked("five", frames)
    again, lens_again = encode_checked("five", frames)
    assert lens == lens_again and np.array_equal(got, again)
    fixed, fixed_lens = encode_checked("five", frames, huffman="fixed")
    assert all(a <= b for a, b in zip(lens, fixed_lens)) and sum(lens) < sum(fixed_lens)


def test_fixed_mode_is_the_default_encoder():
    from fosvos_hip import ops
    frames = np.stack([C.CASES[k] for k in ("96x160_noisy_ellipse", "96x160_noise256", "96x160_runs_and_rests")])
    x = torch.from_numpy(frames).to(DEV)
    out0, len0 = ops.png_encode(x)
    out1, len1 = ops.png_encode(x, huffman="fixed")
    torch.cuda.synchronize()
    assert torch.equal(len0, len1)
    for k in range(frames.shape[0]):
        n = int(len0[k])
        assert torch.equal(out0[k, :n], out1[k, :n])
        assert out0[k, :n].cpu().numpy().tobytes() == want("default[%d]" % k, frames[k], "fixed")
    with pytest.raises(ValueError):
        ops.png_encode(x, huffman="dynamic")


class Centred(torch.nn.Module):
    """OSVOS_VGG with each frame's median taken off the fused logits: about half of the pixels are object."""

    def __init__(self, net):
        super().__init__()
        self.net = net

    def forward(self, x):
        outs = list(self.net.forward(x))
        outs[-1] = outs[-1] - outs[-1].flatten(1).median(dim=1).values.view(-1, 1, 1, 1)
        return outs


class Provider:
    def __init__(self, network):
        self.network = network


def test_fast_pass_fitted_against_fixed(tmp_path):
    from networks.osvos_vgg import OSVOS_VGG
    net = OSVOS_VGG(pretrained=0)
    net.load_state_dict(O.make_state_dict(2))
    prov = Provider(Centred(net.to(DEV)))
    runs = {}
    for mode in ("fixed", "fitted"):
        loader = io_helper.get_data_loader_test(None, 1, "blob", synthetic=(96, 160), n_frames=7)
        score = experiment_helper.test_fast(prov, loader, tmp_path / mode, loader.dataset.annotation, seq_name="blob",
                                            png_huffman=mode)
        last = dict(experiment_helper.last_fast)
        assert last["png_huffman"] == mode
        files = sorted((tmp_path / mode / "blob").iterdir())
        assert [f.name for f in files] == ["%05d.png" % k for k in range(7)]
        assert last["png_bytes"] == sum(f.stat().st_size for f in files)
        runs[mode] = (score, files, last["png_bytes"])
    for a, b in zip(runs["fixed"][1], runs["fitted"][1]):
        pixels = np.asarray(Image.open(str(b)))               # (PIL checks the CRCs and the Adler-32)
        assert np.array_equal(pixels, np.asarray(Image.open(str(a))))
        assert b.read_bytes() == P.encode(pixels, huffman="fitted") and b.stat().st_size <= a.stat().st_size
    print("test_fast 7 frames of 96x160: %d bytes fixed, %d fitted" % (runs["fixed"][2], runs["fitted"][2]))
    assert runs["fitted"][2] <= runs["fixed"][2]
    timed = ("seconds",)
    assert {k: v for k, v in runs["fixed"][0].items() if k not in timed} == \
        {k: v for k, v in runs["fitted"][0].items() if k not in timed}
