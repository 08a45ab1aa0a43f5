"""Scoring on a real MI355X (csrc/eval.hip through fosvos_hip.ops): ``ops.jf_counts`` against the plain numpy statement of
the DAVIS 2016 counts (util/davis_measures.jf_counts_numpy) - integers, so equality with no tolerance - ``ops.prob_bytes``
against the fp64 definition of the PNG bytes, and the scored test pass / the --score flag end to end."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
import yaml
from PIL import Image

from oracle import osvos_ref as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fosvos_amd"))

from util import davis_measures as M, experiment_helper, io_helper  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def reference(logits, gt, radius):
    x, g = logits.cpu().numpy(), gt.cpu().numpy()
    return np.stack([M.jf_counts_numpy(x[k, 0] >= 0, g[k] != 0, radius) for k in range(x.shape[0])])


def run_counts(logits, gt, radius=None, out=None):
    from fosvos_hip import ops
    return ops.jf_counts(logits.to(DEV), gt.to(DEV), radius, out=out).cpu().numpy().astype(np.int64)


def check(logits, gt, radius):
    got, want = run_counts(logits, gt, radius), reference(logits, gt, radius)
    assert np.array_equal(got, want), (tuple(logits.shape), radius, got.tolist(), want.tolist())


def random_frames(n, h, w, seed, densities=(0.5, 0.1, 0.02, 0.9, 0.3)):
    """Frames of different content: frame k has about densities[k] of its pixels set in both masks (independently)."""
    g = torch.Generator().manual_seed(seed)
    logits = torch.empty((n, 1, h, w))
    gt = torch.empty((n, h, w), dtype=torch.uint8)
    for k in range(n):
        d = densities[k % len(densities)]
        logits[k, 0] = torch.rand((h, w), generator=g) - (1.0 - d)  # >= 0 with probability d
        gt[k] = (torch.rand((h, w), generator=g) < d).to(torch.uint8) * (1 + 127 * (k % 3))  # any non-zero value counts
    return logits, gt


def ellipse_frames(n, h, w):
    yy = torch.arange(h, dtype=torch.float32).view(h, 1)
    xx = torch.arange(w, dtype=torch.float32).view(1, w)
    logits = torch.empty((n, 1, h, w))
    gt = torch.empty((n, h, w), dtype=torch.uint8)
    for k in range(n):
        cy, cx = h * (0.45 + 0.03 * k), w * (0.5 - 0.04 * k)
        logits[k, 0] = 1.0 - (((yy - cy) / (h * (0.2 + 0.02 * k))) ** 2 + ((xx - cx) / (w * 0.27)) ** 2)
        gt[k] = ((((yy - cy - 2 - k) / (h * 0.19)) ** 2 + ((xx - cx + 3) / (w * 0.28)) ** 2) <= 1).to(torch.uint8)
    return logits, gt


SIZES = [(480, 854), (384, 683), (240, 427), (61, 107), (24, 40), (1, 1), (1, 130), (130, 1), (1080, 1920),
         (20, 64), (20, 128), (20, 63), (20, 65), (20, 127), (20, 129)]


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_jf_counts_random_masks(size):
    h, w = size
    radii = sorted({1, 2, M.default_radius(h, w)})
    if size in ((480, 854), (240, 427)):
        radii.append(63)  # the disk reaches across most of a word and a fair part of the frame
    n = 1 if h * w > 500000 else 5
    logits, gt = random_frames(n, h, w, seed=h * 1000 + w)
    for r in radii:
        check(logits, gt, r)
    # sparse masks, where a match is the exception and the disk's exact shape shows
    logits, gt = random_frames(1, h, w, seed=h + w, densities=(0.001,))
    for r in radii:
        check(logits, gt, r)


@pytest.mark.parametrize("size", [(480, 854), (384, 683), (61, 107), (1080, 1920)], ids=lambda s: "%dx%d" % s)
def test_jf_counts_ellipse_pairs(size):
    h, w = size
    n = 1 if h * w > 500000 else 5
    logits, gt = ellipse_frames(n, h, w)
    for r in (1, 2, M.default_radius(h, w)):
        check(logits, gt, r)
    counts = run_counts(logits, gt)  # radius=None: the default
    assert np.array_equal(counts, reference(logits, gt, M.default_radius(h, w)))
    assert (counts[:, 0] > 0).all() and (counts[:, 4] > 0).all()
    if n > 1:  # different content per frame: a frame leaking into its neighbour's counters would show
        assert len({tuple(row) for row in counts.tolist()}) == n


def test_pinned_ellipse_pair():
    y, x = np.mgrid[0:96, 0:160]
    a = ((y - 45) / 20) ** 2 + ((x - 80) / 26) ** 2 <= 1
    b = ((y - 47) / 19) ** 2 + ((x - 77) / 27) ** 2 <= 1
    logits = torch.from_numpy(np.where(a, 1.0, -1.0).astype(np.float32)).view(1, 1, 96, 160)
    gt = torch.from_numpy(b.astype(np.uint8)).view(1, 96, 160)
    for r, matches in ((1, [74, 71]), (2, [102, 102]), (8, [188, 188])):
        assert run_counts(logits, gt, r).tolist() == [[1457, 1773, 188, 188] + matches]


@pytest.mark.parametrize("size", [(480, 854), (24, 40), (20, 64), (20, 65), (1, 1)], ids=lambda s: "%dx%d" % s)
def test_jf_counts_constant_frames(size):
    h, w = size
    r = M.default_radius(h, w)
    for value in (0.0, 1.0, -1.0):  # logits of exactly 0 are object
        for fill in (0, 1):
            logits = torch.full((1, 1, h, w), value)
            gt = torch.full((1, h, w), fill, dtype=torch.uint8)
            got = run_counts(logits, gt, r)
            assert np.array_equal(got, reference(logits, gt, r))
            a, b = value >= 0, fill != 0
            assert got.tolist() == [[h * w * (a and b), h * w * (a or b), 0, 0, 0, 0]]


@pytest.mark.parametrize("size", [(480, 854), (61, 107), (20, 128), (20, 129)], ids=lambda s: "%dx%d" % s)
def test_jf_counts_borders_and_corners(size):
    h, w = size
    logits = torch.full((6, 1, h, w), -1.0)
    gt = torch.zeros((6, h, w), dtype=torch.uint8)
    logits[0, 0] = 1.0          # frame 0: the prediction touches all four borders, the ground truth is its inside
    gt[0, 1:-1, 1:-1] = 1
    for k, (y, x) in enumerate([(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)], start=1):
        logits[k, 0, y, x] = 1.0   # frames 1..4: one set pixel in each corner, against a ground truth next to it
        gt[k, min(max(y, 1), h - 2), min(max(x, 1), w - 2)] = 255
    gt[5] = 1                   # frame 5: a ring along the border in the prediction, a full ground truth
    logits[5, 0, 0, :] = logits[5, 0, -1, :] = logits[5, 0, :, 0] = logits[5, 0, :, -1] = 2.0
    for r in (1, 2, M.default_radius(h, w)):
        check(logits, gt, r)


def test_jf_counts_signed_zero():
    h, w = 61, 107
    g = torch.Generator().manual_seed(5)
    pick = torch.rand((1, 1, h, w), generator=g)
    logits = torch.where(pick < 0.3, torch.tensor(0.0), torch.where(pick < 0.6, torch.tensor(-0.0), torch.tensor(-1e-30)))
    assert (torch.signbit(logits) & (logits == 0)).any()
    gt = (torch.rand((1, h, w), generator=g) < 0.5).to(torch.uint8)
    got = run_counts(logits, gt, 1)
    assert np.array_equal(got, reference(logits, gt, 1))
    # 0.0 and -0.0 both count as object: the mask is exactly the zeros
    assert got[0, 0] == int(((logits[0, 0] == 0) & (gt[0] != 0)).sum())


def test_jf_counts_repeatable_on_any_stream_with_dirty_buffers():
    from fosvos_hip import ops
    logits, gt = ellipse_frames(5, 240, 427)
    noise, _ = random_frames(5, 240, 427, seed=9)
    logits = (logits + 0.3 * noise).to(DEV)
    gt = gt.to(DEV)
    want = reference(logits, gt, 4)
    first = ops.jf_counts(logits, gt, 4)
    second = ops.jf_counts(logits, gt, 4)
    assert np.array_equal(first.cpu().numpy(), want) and torch.equal(first, second)
    # neither the counters nor the bit planes may depend on what their buffers held
    out = torch.full((5, 6), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    for buf in ops._WS._buf.values():
        buf.fill_(0xAB)
    assert ops.jf_counts(logits, gt, 4, out=out) is out
    assert np.array_equal(out.cpu().numpy(), want)
    # rows of a larger counter tensor, as the scored pass uses them; the other rows stay
    table = torch.full((9, 6), -7, dtype=torch.int32, device=DEV)
    ops.jf_counts(logits, gt, 4, out=table[2:7])
    assert np.array_equal(table[2:7].cpu().numpy(), want)
    assert (table[:2] == -7).all() and (table[7:] == -7).all()
    side = torch.cuda.Stream(DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):  # the launches go to the caller's (current) stream
        a = ops.jf_counts(logits, gt, 4)
        for buf in ops._WS._buf.values():
            buf.fill_(0xCD)
        b = ops.jf_counts(logits, gt, 4)
        png = ops.prob_bytes(logits)
    side.synchronize()
    assert np.array_equal(a.cpu().numpy(), want) and torch.equal(a, b)
    assert torch.equal(png, ops.prob_bytes(logits))


# ------------------------------------------------------------------------------------------ prob_bytes
def bytes_fp64(x):
    """(bytes, scaled) of one frame by the definition: the sigmoid, its own range and the stretch in fp64."""
    p = 1.0 / (1.0 + np.exp(-x.astype(np.float64)))
    cmin, cmax = p.min(), p.max()
    cscale = cmax - cmin
    if cscale == 0:
        cscale = 1.0
    scaled = (p - cmin) * (255.0 / cscale)
    return (scaled.clip(0, 255) + 0.5).astype(np.uint8), scaled.clip(0, 255)


def check_prob_bytes(logits):
    from fosvos_hip import ops
    got = ops.prob_bytes(logits.to(DEV)).cpu().numpy()
    x = logits.numpy()
    n_band = 0
    for k in range(x.shape[0]):
        want, scaled = bytes_fp64(x[k, 0])
        assert np.array_equal(want, experiment_helper.bytescale(1.0 / (1.0 + np.exp(-x[k, 0].astype(np.float64)))))
        frac = (scaled + 0.5) % 1.0
        band = (frac < 1e-9) | (frac > 1.0 - 1e-9)  # within 1e-9 of a rounding boundary: an ulp of exp() may decide
        n_band += int(band.sum())
        bad = (got[k] != want) & ~band
        assert not bad.any(), (k, int(bad.sum()), got[k][bad][:5], want[bad][:5])
        assert np.abs(got[k].astype(np.int32) - want.astype(np.int32)).max() <= 1
    # the exclusion must not hide a failure: at most 1 pixel per million may fall in the band
    assert n_band * 1000000 <= x.size, (n_band, x.size)
    return got


def test_prob_bytes_against_the_fp64_definition():
    g = torch.Generator().manual_seed(11)
    got = check_prob_bytes(4 * torch.randn((1, 1, 480, 854), generator=g))
    assert got.min() == 0 and got.max() == 255
    # five frames of different ranges and offsets: each is stretched to its own
    x = torch.randn((5, 1, 480, 854), generator=g) * torch.tensor([0.5, 1.0, 2.0, 4.0, 8.0]).view(5, 1, 1, 1) \
        + torch.tensor([0.0, -3.0, 2.0, 1.0, -5.0]).view(5, 1, 1, 1)
    got = check_prob_bytes(x)
    assert (got.reshape(5, -1).min(axis=1) == 0).all() and (got.reshape(5, -1).max(axis=1) == 255).all()
    # sizes off the vector path (H*W not a multiple of four) and a single pixel
    check_prob_bytes(3 * torch.randn((3, 1, 61, 107), generator=g))
    check_prob_bytes(3 * torch.randn((2, 1, 1, 1), generator=g))


def test_prob_bytes_constant_frame_is_zero():
    from fosvos_hip import ops
    x = torch.full((3, 1, 24, 40), 1.5)
    x[1] = -0.25
    x[2, 0, 3, 5] = 2.0  # frame 2 is not constant: its one larger pixel is 255, the rest 0
    got = ops.prob_bytes(x.to(DEV)).cpu()
    assert (got[:2] == 0).all()
    assert got[2, 3, 5] == 255 and int(got[2].sum()) == 255
    out = torch.full((3, 24, 40), 77, dtype=torch.uint8, device=DEV)
    assert ops.prob_bytes(x.to(DEV), out=out) is out and torch.equal(out.cpu(), got)


def test_prob_bytes_within_one_of_the_host_path():
    """test() takes the sigmoid in fp32 (1 / (1 + np.exp(-x)) on the fp32 logits) before bytescale; the device takes it in
    fp64.  The two differ only in the rounding of the sigmoid, about 1e-7 relative, far below the 1/255 step of a byte,
    so a byte can move across one rounding boundary at most: |difference| <= 1 is derived, not measured.  How many pixels
    differ is a measurement: printed, not asserted."""
    from fosvos_hip import ops
    g = torch.Generator().manual_seed(12)
    x = 4 * torch.randn((2, 1, 480, 854), generator=g)
    got = ops.prob_bytes(x.to(DEV)).cpu().numpy().astype(np.int32)
    n_diff = 0
    for k in range(2):
        host = experiment_helper.bytescale(1.0 / (1.0 + np.exp(-x[k, 0].numpy()))).astype(np.int32)
        assert np.abs(got[k] - host).max() <= 1
        n_diff += int((got[k] != host).sum())
    print("prob_bytes vs the fp32 host path: %d of %d pixels differ (by one)" % (n_diff, x.numel()))


# ------------------------------------------------------------------------------------------ arguments
def test_bad_arguments_raise():
    from fosvos_hip import lib, ops
    logits = torch.zeros((2, 1, 24, 40), device=DEV)
    gt = torch.zeros((2, 24, 40), dtype=torch.uint8, device=DEV)
    for bad in (lambda: ops.jf_counts(logits.double(), gt), lambda: ops.jf_counts(logits, gt.float()),
                lambda: ops.jf_counts(logits, gt.int()), lambda: ops.prob_bytes(logits.half()),
                lambda: ops.jf_counts(logits, gt[:, :, :39]), lambda: ops.jf_counts(logits, gt[:1]),
                lambda: ops.jf_counts(logits[:, 0], gt), lambda: ops.jf_counts(logits.expand(2, 3, 24, 40), gt),
                lambda: ops.jf_counts(logits, gt, 0), lambda: ops.jf_counts(logits, gt, 64),
                lambda: ops.jf_counts(logits, gt, out=torch.zeros((2, 5), dtype=torch.int32, device=DEV)),
                lambda: ops.jf_counts(logits, gt, out=torch.zeros((2, 6), dtype=torch.int64, device=DEV)),
                lambda: ops.prob_bytes(logits, out=torch.zeros((2, 24, 41), dtype=torch.uint8, device=DEV)),
                lambda: ops.prob_bytes(logits, out=torch.zeros((2, 24, 40), dtype=torch.int8, device=DEV)),
                lambda: ops.prob_bytes(torch.zeros((0, 1, 24, 40), device=DEV))):
        with pytest.raises(ValueError):
            bad()
    for bad in (lambda: ops.jf_counts(logits.cpu(), gt), lambda: ops.jf_counts(logits, gt.cpu()),
                lambda: ops.jf_counts(logits, gt, out=torch.zeros((2, 6), dtype=torch.int32)),
                lambda: ops.prob_bytes(logits.cpu()),
                lambda: ops.prob_bytes(logits, out=torch.zeros((2, 24, 40), dtype=torch.uint8))):
        with pytest.raises(RuntimeError):  # tensors on different devices
            bad()
    if torch.cuda.device_count() > 1:
        with pytest.raises(RuntimeError):
            ops.jf_counts(logits, gt.to("cuda:1"))
    # straight through the C ABI: the library's error codes, never a fault
    L = lib()
    need = L.fosvos_jf_workspace_bytes(2, 24, 40)
    assert need == 2 * 2 * 24 * 1 * 8 and L.fosvos_jf_workspace_bytes(1, 480, 854) == 2 * 480 * 14 * 8
    assert L.fosvos_jf_workspace_bytes(0, 24, 40) == 0
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    out = torch.full((2, 6), 5, dtype=torch.int32, device=DEV)
    mm = torch.zeros((2, 2), device=DEV)
    png = torch.zeros((2, 24, 40), dtype=torch.uint8, device=DEV)
    st = torch.cuda.current_stream().cuda_stream

    def jf(lg=logits.data_ptr(), g=gt.data_ptr(), n=2, h=24, w=40, r=2, o=out.data_ptr(), w_=ws.data_ptr(), nb=need):
        return L.fosvos_jf_counts(lg, g, n, h, w, r, o, w_, nb, 0, st)

    assert jf(nb=need - 8) == -3 and b"workspace" in L.fosvos_last_error()
    assert jf(nb=0) == -3
    assert jf(r=0) == -2 and jf(r=64) == -2
    assert jf(lg=None) == -2 and jf(g=None) == -2 and jf(o=None) == -2 and jf(w_=None) == -2
    assert jf(n=0) == -1 and jf(h=0) == -1 and jf(w=-3) == -1
    assert jf(w_=ws.data_ptr() + 4, nb=need) == -2  # misaligned workspace
    assert L.fosvos_prob_bytes(None, 2, 24, 40, mm.data_ptr(), png.data_ptr(), 0, st) == -2
    assert L.fosvos_prob_bytes(logits.data_ptr(), 2, 24, 40, None, png.data_ptr(), 0, st) == -2
    assert L.fosvos_prob_bytes(logits.data_ptr(), 2, 0, 40, mm.data_ptr(), png.data_ptr(), 0, st) == -1
    torch.cuda.synchronize()
    assert (out == 5).all()  # none of the refused calls launched anything
    assert jf() == 0
    torch.cuda.synchronize()
    assert out.cpu().tolist() == [[0, 960, 0, 0, 0, 0]] * 2  # logits of 0 are object everywhere, the ground truth is empty


# ------------------------------------------------------------------------------------------ the scored pass
class Centred(torch.nn.Module):
    """The real OSVOS_VGG forward with each frame's median taken off the fused logits, so that whatever the seeded
    weights make of a frame about half of its pixels are object and the masks have long, ragged contours.  It keeps the
    fused logits of every forward for the test to read back."""

    def __init__(self, net):
        super().__init__()
        self.net, self.seen = net, []

    def forward(self, x):
        outs = list(self.net.forward(x))
        fused = outs[-1]
        outs[-1] = fused - fused.flatten(1).median(dim=1).values.view(-1, 1, 1, 1)
        self.seen.append(outs[-1].detach().cpu())
        return outs


class Provider:
    def __init__(self, network):
        self.network = network


def make_provider(seed=2):
    from networks.osvos_vgg import OSVOS_VGG
    net = OSVOS_VGG(pretrained=0)
    net.load_state_dict(O.make_state_dict(seed))
    return Provider(Centred(net.to(DEV)))


@pytest.mark.parametrize("size", [(96, 160), (480, 854)], ids=lambda s: "%dx%d" % s)
def test_scored_pass_on_the_card(size, tmp_path):
    h, w = size
    prov = make_provider()
    loader = io_helper.get_data_loader_test(None, 2, "blob", synthetic=size, n_frames=4)
    score = experiment_helper.test_scored(prov, loader, tmp_path / "scored", loader.dataset.annotation, seq_name="blob")
    logits = torch.cat(prov.network.seen)
    assert tuple(logits.shape) == (4, 1, h, w) and score["scored"] == [True] * 4
    r = M.default_radius(h, w)
    want = np.stack([M.jf_counts_numpy(logits[k, 0].numpy() >= 0, loader.dataset.annotation("blob", "%05d" % k), r)
                     for k in range(4)])
    assert score["radius"] == r and score["counts"] == want.tolist()
    assert (want[:, 2] > 0).all() and (want[:, 3] > 0).all()  # both masks have contours
    j, f = M.jf_from_counts(want)
    assert score["J"] == list(j) and score["F"] == list(f)
    assert score["J_stats"] == M.sequence_statistics(j) and score["F_stats"] == M.sequence_statistics(f)
    assert score["J&F"] == (score["J_stats"]["mean"] + score["F_stats"]["mean"]) / 2
    assert score == experiment_helper.last_score
    # the same files as test() writes for the same loader, bytes within one
    experiment_helper.test(prov, loader, tmp_path / "plain", False, False, seq_name="blob")
    names = sorted(p.name for p in (tmp_path / "plain" / "blob").iterdir())
    assert names == ["%05d.png" % k for k in range(4)]
    assert sorted(p.name for p in (tmp_path / "scored" / "blob").iterdir()) == names
    n_diff = 0
    for name in names:
        a = np.asarray(Image.open(str(tmp_path / "scored" / "blob" / name))).astype(np.int32)
        b = np.asarray(Image.open(str(tmp_path / "plain" / "blob" / name))).astype(np.int32)
        assert a.shape == (h, w) and np.abs(a - b).max() <= 1
        n_diff += int((a != b).sum())
    print("scored pass vs test() at %dx%d: %d of %d PNG bytes differ (by one)" % (h, w, n_diff, 4 * h * w))


def test_train_online_score_flag(tmp_path, monkeypatch):
    import train_online
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(train_online, "save_dir_models", tmp_path / "models")
    monkeypatch.setattr(train_online, "save_dir_results", tmp_path / "results")
    common = ["--synthetic", "--height", "96", "--width", "160", "--n-epochs", "2", "-s", "blob"]
    train_online.main(common)
    seq_dir = tmp_path / "results" / "vgg16" / "online" / "blob"
    pngs = sorted(p.name for p in seq_dir.iterdir())
    assert pngs == ["%05d.png" % k for k in range(4)]  # no scores.yml without the flag
    plain = {name: np.asarray(Image.open(str(seq_dir / name))).astype(np.int32) for name in pngs}
    monkeypatch.setattr(train_online, "save_dir_results", tmp_path / "results_scored")
    try:
        train_online.main(common + ["--score"])
    finally:
        train_online.score = False
    seq_dir = tmp_path / "results_scored" / "vgg16" / "online" / "blob"
    assert sorted(p.name for p in seq_dir.iterdir()) == pngs + ["scores.yml"]
    score = yaml.safe_load((seq_dir / "scores.yml").read_text())
    assert score["seq_name"] == "blob" and score["fnames"] == ["%05d" % k for k in range(4)]
    assert score["radius"] == M.default_radius(96, 160) and len(score["counts"]) == 4
    j, f = M.jf_from_counts(np.array(score["counts"]))
    assert score["J"] == list(j) and score["F"] == list(f)
    assert score["J_stats"] == M.sequence_statistics(j)
    assert train_online.scored_sequences and train_online.scored_sequences[-1]["counts"] == score["counts"]
    for name in pngs:
        assert np.asarray(Image.open(str(seq_dir / name))).shape == plain[name].shape
