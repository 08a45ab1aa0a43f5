"""Several objects a sequence on a real MI355X: ``ops.merge_objects``, ``ops.jf_counts_labels`` and ``ops.png_encode_indexed``
against their numpy statements (util/object_merge.py, ``png_layout.encode_indexed``) - integers and comparisons only, so no
tolerance anywhere -, then ``experiment_helper.test_objects`` and ``train_online --multi-object`` end to end."""
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

from util import davis_measures as M, experiment_helper, object_merge as OM, png_layout as P  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILL = 0xA5
NAN, INF = float("nan"), float("inf")
SHAPES = [(1, 5, 67), (3, 33, 130), (2, 16, 64), (1, 96, 160)]     # no vector path and ragged words; odd; exact words; 4 | HW
SHAPE_IDS = ["1x5x67", "3x33x130", "2x16x64", "1x96x160"]


def planted_logits(k, n, h, w, seed):
    """Normal draws with ties between objects, signed zeros, NaN and infinities planted (about 3 % of the pixels each)."""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(k, n, h, w)).astype(np.float32)
    pick = rng.random((n, h, w))
    x[:, pick < 0.03] = 0.75                                        # every object ties
    if k > 1:
        x[k // 2:, (pick >= 0.03) & (pick < 0.06)] = 2.5            # the upper half ties above the rest
    for lo, value in ((0.06, 0.0), (0.09, -0.0), (0.12, NAN), (0.15, INF), (0.18, -INF)):
        where = (pick >= lo) & (pick < lo + 0.03)
        x[rng.integers(0, k, (n, h, w))[where], np.nonzero(where)[0], np.nonzero(where)[1], np.nonzero(where)[2]] = value
    both = (pick >= 0.21) & (pick < 0.23)
    x[0, both] = INF
    x[-1, both] = INF                                               # +inf twice
    x[:, (pick >= 0.23) & (pick < 0.25)] = NAN                      # nothing valid
    return x


def label_maps(n, h, w, k, seed):
    """Blobs that touch the frame edge, object 2 missing (where there is one), and a patch of an id above K."""
    rng = np.random.default_rng(seed)
    ids = np.zeros((n, h, w), dtype=np.uint8)
    for f in range(n):
        for obj in range(1, k + 1):
            if obj == 2:
                continue
            y0, x0 = int(rng.integers(-2, h - 1)), int(rng.integers(-2, w - 1))
            y1, x1 = y0 + int(rng.integers(2, h // 2 + 3)), x0 + int(rng.integers(2, w // 2 + 3))
            ids[f, max(y0, 0):y1, max(x0, 0):x1] = obj
        ids[f, h // 2:h // 2 + 2, w - 3:] = k + 1                    # belongs to no object
        ids[f, 0, :2] = 1                                           # a corner
    return ids


# ------------------------------------------------------------------------------------------ merge_objects
@pytest.mark.parametrize("k", [1, 2, 3, 7, 16])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_merge_objects_is_merge_labels(shape, k):
    from fosvos_hip import ops
    n, h, w = shape
    x = planted_logits(k, n, h, w, seed=h * w + k)
    want = OM.merge_labels(x)
    assert want.max() == k or k > 3                                  # (every id occurs for the small K)
    maps = [torch.from_numpy(x[i]).to(DEV).view(n, 1, h, w) for i in range(k)]
    got = ops.merge_objects(maps)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (n, h, w)
    assert np.array_equal(got.cpu().numpy(), want)
    # into a view at an odd byte offset (the 1-pixel path), the bytes around it untouched
    buf = torch.full((n * h * w + 8,), FILL, dtype=torch.uint8, device=DEV)
    out = buf[3:3 + n * h * w].view(n, h, w)
    assert ops.merge_objects(maps, out=out).data_ptr() == out.data_ptr()
    host = buf.cpu().numpy()
    assert np.array_equal(host[3:3 + n * h * w].reshape(n, h, w), want)
    assert (host[:3] == FILL).all() and (host[3 + n * h * w:] == FILL).all()
    # one logit map 4 bytes off a 16-byte boundary (again the 1-pixel path)
    shifted = torch.empty(n * h * w + 1, dtype=torch.float32, device=DEV)[1:].view(n, 1, h, w)
    shifted.copy_(maps[-1])
    assert np.array_equal(ops.merge_objects(maps[:-1] + [shifted]).cpu().numpy(), want)
    if k == 1:
        assert np.array_equal(want, (x[0] >= 0).astype(np.uint8))


def test_merge_objects_argument_checks():
    from fosvos_hip import FosvosHipError, ops
    maps = [torch.zeros((1, 1, 4, 8), device=DEV) for _ in range(17)]
    with pytest.raises(ValueError):
        ops.merge_objects([])
    with pytest.raises(ValueError):
        ops.merge_objects(maps)
    with pytest.raises(ValueError):
        ops.merge_objects([maps[0], torch.zeros((1, 1, 4, 9), device=DEV)])
    with pytest.raises(ValueError):
        ops.merge_objects(maps[:2], out=torch.zeros((1, 4, 9), dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError):
        ops.merge_objects([maps[0].double()])
    with pytest.raises(RuntimeError):
        ops.merge_objects([maps[0].cpu()])
    # the C entry's own checks
    import ctypes
    import fosvos_hip
    table = (ctypes.c_void_p * 17)(*[m.data_ptr() for m in maps])
    out = torch.zeros((1, 4, 8), dtype=torch.uint8, device=DEV)
    for bad in (0, 17):
        with pytest.raises(FosvosHipError):
            fosvos_hip.check(fosvos_hip.lib().fosvos_merge_objects(table, bad, 1, 4, 8, out.data_ptr(), 0, None), "merge")


# ------------------------------------------------------------------------------------------ jf_counts_labels
@pytest.mark.parametrize("k", [1, 3, 16])
@pytest.mark.parametrize("radius", [1, None, 63], ids=["r1", "rdefault", "r63"])
@pytest.mark.parametrize("shape", SHAPES + [(1, 40, 200)], ids=SHAPE_IDS + ["1x40x200"])
def test_jf_counts_labels_is_the_numpy_count(shape, radius, k):
    from fosvos_hip import ops
    n, h, w = shape
    pred, gt = label_maps(n, h, w, k, seed=h + w + k), label_maps(n, h, w, k, seed=h * w + k)
    r = M.default_radius(h, w) if radius is None else radius
    want = np.stack([OM.jf_counts_labels_numpy(pred[f], gt[f], k, r) for f in range(n)])
    rows = torch.full((n + 2, k, 6), -7, dtype=torch.int32, device=DEV)   # the op zeroes its own rows, and only those
    got = ops.jf_counts_labels(torch.from_numpy(pred).to(DEV), torch.from_numpy(gt).to(DEV), k, radius, out=rows[1:n + 1])
    assert got.dtype == torch.int32 and tuple(got.shape) == (n, k, 6)
    assert np.array_equal(got.cpu().numpy().astype(np.int64), want), (got.cpu().numpy(), want)
    assert (rows[0] == -7).all() and (rows[n + 1] == -7).all()
    if k >= 2:
        assert not want[:, 1].any()                                  # the empty object: all six counts 0
    assert want[:, 0, 0].sum() >= 0 and want[:, 0, 1].all()          # object 1 is somewhere in every frame


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_jf_counts_labels_of_one_object_is_jf_counts(shape):
    from fosvos_hip import ops
    n, h, w = shape
    x = torch.from_numpy(planted_logits(1, n, h, w, seed=w)[0]).to(DEV).view(n, 1, h, w)
    gt = torch.from_numpy((label_maps(n, h, w, 1, seed=h) == 1).astype(np.uint8)).to(DEV)
    labels = ops.merge_objects([x])
    assert torch.equal(ops.jf_counts_labels(labels, gt, 1)[:, 0], ops.jf_counts(x, gt))


def test_jf_counts_labels_argument_checks():
    from fosvos_hip import ops
    a = torch.zeros((1, 8, 8), dtype=torch.uint8, device=DEV)
    for bad_k in (0, 17):
        with pytest.raises(ValueError):
            ops.jf_counts_labels(a, a, bad_k)
    with pytest.raises(ValueError):
        ops.jf_counts_labels(a, a, 2, radius=64)
    with pytest.raises(ValueError):
        ops.jf_counts_labels(a, a[:, :4], 2)
    with pytest.raises(ValueError):
        ops.jf_counts_labels(a, a, 2, out=torch.zeros((1, 3, 6), dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):
        ops.jf_counts_labels(a.float(), a, 2)


# ------------------------------------------------------------------------------------------ png_encode_indexed
def label_frames(h, w, k=3):
    """Three frames: flat, blobs, noise over 0..k."""
    rng = np.random.default_rng(h * 131 + w)
    return np.stack([np.full((h, w), k, dtype=np.uint8), label_maps(1, h, w, k, seed=h + w)[0],
                     rng.integers(0, k + 1, (h, w), dtype=np.uint8)])


@pytest.mark.parametrize("huffman", P.HUFFMAN_MODES)
@pytest.mark.parametrize("random_palette", [False, True], ids=["davis_palette", "random_palette"])
@pytest.mark.parametrize("size", [(8, 8), (64, 64), (65, 67), (96, 160)], ids=["8x8", "64x64", "65x67", "96x160"])
def test_png_encode_indexed_is_encode_indexed(size, random_palette, huffman):
    from fosvos_hip import ops
    h, w = size
    frames = label_frames(h, w)
    n = frames.shape[0]
    palette = np.random.default_rng(w).integers(0, 256, (256, 3), dtype=np.uint8) if random_palette else None
    cap = ops.png_indexed_capacity(h, w)
    assert cap == P.max_file_bytes_indexed(h, w) == ops.png_capacity(h, w) + 780
    out = torch.full((n, cap), FILL, dtype=torch.uint8, device=DEV)
    lengths = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    dev_frames = torch.from_numpy(frames).to(DEV)
    got, got_lengths = ops.png_encode_indexed(dev_frames, None if palette is None else torch.from_numpy(palette).to(DEV),
                                              out=out, lengths=lengths, huffman=huffman)
    assert got.data_ptr() == out.data_ptr() and got_lengths.data_ptr() == lengths.data_ptr()
    host, host_lengths = out.cpu().numpy(), lengths.cpu().tolist()
    for f in range(n):
        want = P.encode_indexed(frames[f], palette, huffman)
        assert host_lengths[f] == len(want)
        assert host[f, :len(want)].tobytes() == want
        assert (host[f, len(want):] == FILL).all()                   # nothing behind the file is written
    tags = [t for t, _ in P.chunks(host[1, :host_lengths[1]].tobytes())]
    assert tags == [b"IHDR", b"PLTE"] + [b"IDAT"] * (P.n_segments(h, w) + 1) + [b"IEND"]
    # the greyscale encoder still writes the greyscale layout for the same bytes
    grey, grey_lengths = ops.png_encode(dev_frames, huffman=huffman)
    grey, grey_lengths = grey.cpu().numpy(), grey_lengths.cpu().tolist()
    for f in range(n):
        assert grey[f, :grey_lengths[f]].tobytes() == P.encode(frames[f], huffman)


def test_png_encode_indexed_argument_checks():
    from fosvos_hip import ops
    a = torch.zeros((1, 8, 8), dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError):
        ops.png_encode_indexed(a, huffman="best")
    with pytest.raises(ValueError):
        ops.png_encode_indexed(a, palette=torch.zeros((16, 3), dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError):
        ops.png_encode_indexed(a, out=torch.zeros((1, ops.png_capacity(8, 8)), dtype=torch.uint8, device=DEV))   # 780 short
    with pytest.raises(RuntimeError):
        ops.png_encode_indexed(a, palette=torch.zeros((256, 3), dtype=torch.uint8))
    assert ops.default_palette(DEV) is ops.default_palette(DEV)      # uploaded once
    assert np.array_equal(ops.default_palette(DEV).cpu().numpy(), OM.davis_palette())


# ------------------------------------------------------------------------------------------ the pass
class Centred(torch.nn.Module):
    """The real OSVOS_VGG forward with each frame's upper quartile taken off the fused logits: about a quarter of the pixels
    answer "mine", so K nets leave background, contested and uncontested pixels.  It keeps the fused logits of every forward."""

    def __init__(self, net):
        super().__init__()
        self.net, self.seen = net, []

    def forward(self, x):
        outs = list(self.net.forward(x))
        fused = outs[-1]
        outs[-1] = fused - fused.flatten(1).quantile(0.75, dim=1).view(-1, 1, 1, 1)
        self.seen.append(outs[-1].detach().float().cpu())
        return outs


class Provider:
    def __init__(self, network):
        self.network = network


def make_provider(seed):
    from networks.osvos_vgg import OSVOS_VGG
    net = OSVOS_VGG(pretrained=0)
    net.load_state_dict(O.make_state_dict(seed))
    return Provider(Centred(net.to(DEV)))


@pytest.mark.parametrize("k", [2, 3])
def test_objects_pass_on_the_card(k, tmp_path):
    """Every file against ``merge_labels`` of the nets' own one-frame forwards.  The pass forwards two frames a call, which
    the engine computes exactly as single frames, so no logit and no label is expected to differ; the figures are printed,
    and equality is asserted at every pixel where all K logits agree."""
    from dataloaders.synthetic import SyntheticObjectsSequence
    from torch.utils.data import DataLoader
    h, w, n_frames = 96, 160, 7
    data = SyntheticObjectsSequence("blobs", h, w, n_frames=n_frames, n_objects=k)
    loader = DataLoader(data, batch_size=1, shuffle=False, num_workers=0)
    providers = [make_provider(seed) for seed in range(2, 2 + k)]
    score = experiment_helper.test_objects(providers, loader, tmp_path, data.annotation, group=5, seq_name="blobs")
    assert score == experiment_helper.last_score
    batched = [torch.cat(p.network.seen) for p in providers]      # the logits the pass itself computed
    # groups of 5 and 2 frames, two frames a forward call: 2 2 1 | 2
    assert all([int(t.shape[0]) for t in p.network.seen] == [2, 2, 1, 2] for p in providers)
    names = sorted(p.name for p in (tmp_path / "blobs").iterdir())
    assert names == ["%05d.png" % f for f in range(n_frames)]
    radius = M.default_radius(h, w)
    n_logit_diff = n_label_diff = 0
    for f in range(n_frames):
        image = data[f]["image"][None].to(DEV)
        with torch.no_grad():
            single = [p.network.forward(image)[-1].detach().float().cpu() for p in providers]
        agree = np.ones((h, w), dtype=bool)
        for i in range(k):
            agree &= (single[i][0, 0] == batched[i][f, 0]).numpy()
        want = OM.merge_labels([s[:, 0].numpy() for s in single])[0]
        file = (tmp_path / "blobs" / names[f]).read_bytes()
        im = Image.open(str(tmp_path / "blobs" / names[f]))
        im.load()
        got = np.asarray(im)
        assert im.mode == "P" and got.shape == (h, w)
        print("frame %d: %d of %d pixels have a logit that differs between the two-a-call and the one-frame forward, %d "
              "labels differ; labels present %s" % (f, int((~agree).sum()), agree.size, int((got != want).sum()),
                                                    np.unique(got).tolist()))
        assert np.array_equal(got[agree], want[agree])
        n_logit_diff += int((~agree).sum())
        n_label_diff += int((got != want).sum())
        # the file is the layout's, with the DAVIS palette
        assert file == P.encode_indexed(got)
        assert np.array_equal(np.array(im.getpalette(), dtype=np.uint8).reshape(-1, 3), OM.davis_palette())
        assert [t for t, _ in P.chunks(file)] == [b"IHDR", b"PLTE"] + [b"IDAT"] * (P.n_segments(h, w) + 1) + [b"IEND"]
        # counts, J and F: numpy on the labels the file holds
        counts = OM.jf_counts_labels_numpy(got, data.annotation("blobs", "%05d" % f), k, radius)
        j, fm = M.jf_from_counts(counts)
        for obj in range(k):
            entry = score["objects"][obj]
            assert entry["counts"][f] == counts[obj].tolist() and entry["J"][f] == j[obj] and entry["F"][f] == fm[obj]
    print("objects pass vs one-frame forwards: %d pixels with a differing logit, %d labels differ" % (n_logit_diff, n_label_diff))
    assert score["n_objects"] == k and score["radius"] == radius and score["scored"] == [True] * n_frames
    assert [o["object_id"] for o in score["objects"]] == list(range(1, k + 1))
    for name in ("J_stats", "F_stats"):
        for obj in score["objects"]:
            values = np.array(obj[name[0]], dtype=np.float64)
            assert obj[name] == M.sequence_statistics(values)
        assert score[name]["mean"] == pytest.approx(np.mean([o[name]["mean"] for o in score["objects"]]), abs=1e-15)
    assert score["J&F"] == (score["J_stats"]["mean"] + score["F_stats"]["mean"]) / 2


def test_train_online_multi_object_flag(tmp_path, monkeypatch):
    import train_online
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(train_online, "save_dir_models", tmp_path / "models")
    monkeypatch.setattr(train_online, "save_dir_results", tmp_path / "results")
    try:
        train_online.main(["--synthetic", "--height", "96", "--width", "160", "--n-epochs", "3", "-s", "blobs",
                           "--multi-object", "--objects", "2", "--score"])
        assert train_online.multi_object and train_online.synthetic_objects == 2
        snapshots = sorted(p.name for p in (tmp_path / "models" / "vgg16" / "online").iterdir())
        assert snapshots == ["vgg16_blobs_1_epoch-2.pth", "vgg16_blobs_2_epoch-2.pth"]
        seq_dir = tmp_path / "results" / "vgg16" / "online" / "blobs"
        assert sorted(p.name for p in seq_dir.iterdir()) == ["%05d.png" % f for f in range(4)] + ["scores.yml"]
        for f in range(4):
            im = Image.open(str(seq_dir / ("%05d.png" % f)))
            im.load()
            assert im.mode == "P" and np.asarray(im).shape == (96, 160) and np.asarray(im).max() <= 2
        score = yaml.safe_load((seq_dir / "scores.yml").read_text())
        assert score["seq_name"] == "blobs" and score["n_objects"] == 2
        assert [o["object_id"] for o in score["objects"]] == [1, 2] and all(len(o["J"]) == 4 for o in score["objects"])
        assert np.isfinite(score["J&F"]) and 0.0 <= score["J&F"] <= 1.0
        assert train_online.scored_sequences and train_online.scored_sequences[-1]["objects"][0]["counts"] == \
            score["objects"][0]["counts"]
    finally:
        train_online.score = False
        train_online.multi_object = False
