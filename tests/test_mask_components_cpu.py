"""Cleaning a mask by its shape, host side: the numpy statement (util/mask_components.py) against scipy's labelling and rule
by rule, CleanOptions, the flag combinations run_webcam and train_online accept and refuse, and the argument checks of the C
entries, which answer with error codes before any device is touched.  No GPU."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fosvos_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mask_component_cases as C  # noqa: E402
from util import davis_measures  # noqa: E402
from util import mask_components as M  # noqa: E402

SHAPES = [(5, 67), (33, 130), (16, 64), (96, 160), (150, 300), (1, 1), (1, 200), (200, 1)]


def assert_same_partition(roots, mask):
    ndimage = pytest.importorskip("scipy.ndimage")
    labels, count = ndimage.label(mask, np.ones((3, 3)))
    assert roots.dtype == np.int32 and roots.shape == mask.shape
    assert np.array_equal(roots >= 0, mask) and np.all(roots[~mask] == -1)
    flat_l, flat_r = labels.ravel(), roots.ravel()
    fg = np.flatnonzero(flat_l)
    # every class of scipy's has one root, and that root is the class's smallest index
    first = np.full(count + 1, flat_l.size, dtype=np.int64)
    np.minimum.at(first, flat_l[fg], fg)
    assert np.array_equal(flat_r[fg], first[flat_l[fg]])


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_roots_are_scipys_partition_with_minimum_index_labels(shape):
    cases = C.mask_cases(*shape)
    if shape == (150, 300):
        cases += C.diagonal_cases(*shape)[::7] + C.diagonal_cases(*shape, centre=(80, 128))[::5]
        cases += [(name, logits) for name, logits, _, _, _ in C.gate_cases()[::4]]
    for name, logits in cases:
        mask = M.logits_mask(logits)
        assert_same_partition(M.component_roots(mask), mask)


def test_the_mask_rule():
    x = np.array([[np.nan, -0.0, 0.0, -1e-30, np.inf, -np.inf, 1e-30]], dtype=np.float32)
    assert M.logits_mask(x).tolist() == [[False, True, True, False, True, False, True]]
    with pytest.raises(ValueError):
        M.component_roots(np.zeros((2, 2, 2), bool))


def test_hand_labelled_map():
    m = np.array([[0, 1, 0, 0, 1],
                  [1, 0, 0, 0, 1],
                  [0, 0, 1, 0, 0],
                  [0, 1, 0, 0, 1]], dtype=bool)
    want = np.array([[-1, 1, -1, -1, 4],
                     [1, -1, -1, -1, 4],
                     [-1, -1, 12, -1, -1],
                     [-1, 12, -1, -1, 19]], dtype=np.int32)
    assert np.array_equal(M.component_roots(m), want)


def test_area_boundary():
    m = C.area_blobs(12, 40, 7)
    exact, short = m.copy(), m.copy()
    exact[-1] = False
    short[0] = False
    assert exact.sum() == 7 and short.sum() == 6
    assert np.array_equal(M.keep_components(m, min_area=7), exact)      # an area equal to min_area stays
    assert np.array_equal(M.keep_components(m, min_area=8), np.zeros_like(m))
    assert np.array_equal(M.keep_components(m, min_area=6), m)
    assert np.array_equal(M.keep_components(m, min_area=0), m) and np.array_equal(M.keep_components(m, min_area=1), m)
    for bad in (-1, 1.5, True):
        with pytest.raises(ValueError):
            M.keep_components(m, min_area=bad)


def test_empty_seed_means_gate_off():
    m = C.equal_blobs(20, 30)
    none = np.zeros(m.shape, np.uint8)
    assert np.array_equal(M.keep_components(m, None, 5), m)
    assert np.array_equal(M.keep_components(m, none, 5), m)
    far = none.copy()
    far[10, 0] = 1   # a seed that touches nothing: everything goes
    assert not M.keep_components(m, far, 0).any()
    with pytest.raises(ValueError):
        M.keep_components(m, np.zeros((3, 3), np.uint8), 1)
    for bad in (-1, 64, 2.5, True):
        with pytest.raises(ValueError):
            M.keep_components(m, none, bad)


@pytest.mark.parametrize("radius", [0, 1, 2, 5, 8, 63])
def test_dilation_is_davis_measures(radius):
    rng = np.random.default_rng(radius)
    for shape in ((40, 90), (1, 70), (70, 1), (130, 140)):
        seed = rng.random(shape) < 0.004
        seed[0, 0] = seed[-1, -1] = True
        assert np.array_equal(M.dilate_disk(seed, radius), davis_measures.dilate(seed, radius))


def test_radius_geometry():
    cases = C.gate_cases()
    assert len(cases) == 32 and {c[3] for c in cases} == {0, 1, 5, 63}
    for name, logits, seed, radius, near in cases:
        mask = M.logits_mask(logits)
        by, bx = np.argwhere(mask)[0]
        sy, sx = np.argwhere(seed)[0]
        d2 = (by - sy) ** 2 + (bx - sx) ** 2
        assert (d2 <= radius * radius) == near, name  # the cases are what they say
        kept = M.keep_components(mask, seed, radius)
        want = np.zeros_like(mask)
        want[by, bx] = near
        assert np.array_equal(kept, want), name       # the far blob never stays
        near_map = davis_measures.dilate(seed, radius)
        assert near_map[by, bx] == near, name
    # the exact diagonal (3, 4) at r = 5 is inside, and seed and blob sit in different 64-pixel words
    name, logits, seed, radius, near = [c for c in cases if c[0] == "r5_diagonal_in_fwd"][0]
    (by, bx), (sy, sx) = np.argwhere(logits >= 0)[0], np.argwhere(seed)[0]
    assert (sy - by, sx - bx) == (3, 4) and bx // 64 != sx // 64 and near


def test_largest_tie_and_eligibility():
    m = C.equal_blobs(20, 30)
    roots = M.component_roots(m)
    areas = {int(r): int((roots == r).sum()) for r in np.unique(roots[roots >= 0])}
    assert sorted(areas.values()) == [1, 6, 6]
    first = min(r for r, a in areas.items() if a == 6)
    assert np.array_equal(M.keep_components(m, largest=True), roots == first)   # the tie goes to the smaller root
    # largest picks among the eligible only: a seed on the later blob, or on the single pixel
    later = max(r for r, a in areas.items() if a == 6)
    seed = (roots == later).astype(np.uint8)
    assert np.array_equal(M.keep_components(m, seed, 0, largest=True), roots == later)
    single = [r for r, a in areas.items() if a == 1][0]
    seed = (roots == single).astype(np.uint8)
    assert np.array_equal(M.keep_components(m, seed, 0, largest=True), roots == single)
    assert not M.keep_components(m, seed, 0, min_area=2, largest=True).any()    # nothing eligible: nothing kept
    assert np.array_equal(M.keep_components(m, min_area=2), m & (roots != single))


def test_clean_logits_passes_bits():
    x = C.planted_logits(33, 130, 0.41)
    bits = x.view(np.int32)
    assert (x.view(np.uint32) == 0xffc12345).sum() == 1  # the NaN with a payload is there
    mask = M.logits_mask(x)
    kept = M.keep_components(mask, min_area=7)
    assert kept.any() and (mask & ~kept).any()
    out = M.clean_logits(x, kept, -100.0)
    assert out.dtype == np.float32 and out is not x
    dropped = mask & ~kept
    assert np.all(out[dropped] == np.float32(-100.0))
    assert np.array_equal(out.view(np.int32)[~dropped], bits[~dropped])  # NaN payloads and signed zeros included
    assert np.array_equal(M.clean_logits(x, kept, -0.5)[dropped], np.full(dropped.sum(), -0.5, np.float32))
    for bad in (0.0, -0.0, 1.0, -np.inf, np.inf, np.nan, -1e39):
        with pytest.raises(ValueError, match="fill"):
            M.clean_logits(x, kept, bad)
    with pytest.raises(ValueError):
        M.clean_logits(x.astype(np.float64), kept)
    with pytest.raises(ValueError):
        M.clean_logits(x, kept[:5])


def sequence_maps():
    """Four frames: an object that drifts and a far blob; frame 2 is all background."""
    h, w = 40, 100
    frames, obj = [], []
    for k in range(4):
        m = np.zeros((h, w), bool)
        m[10:20, 10 + 3 * k:25 + 3 * k] = True
        o = m.copy()
        m[30:36, 80:90] = True
        if k == 2:
            m[:] = o[:] = False
        frames.append(C.mask_logits(m))
        obj.append(o)
    return np.stack(frames), np.stack(obj)


def test_chain_drops_the_far_blob_and_recovers():
    x, obj = sequence_maps()
    seed0 = obj[0].astype(np.uint8)
    out, kept = M.clean_sequence(x, seed0, radius=4, chain=True)
    assert np.array_equal(kept[0], obj[0]) and np.array_equal(kept[1], obj[1])   # frame 1 is gated by frame 0's kept mask
    assert not kept[2].any()
    assert np.array_equal(kept[3], M.logits_mask(x[3]))   # after an all-background frame nothing gates: both come back
    assert np.array_equal(out[1] >= 0, obj[1]) and np.all(out[1][30:36, 80:90] == np.float32(-100))
    # radius too small for the drift: the object is lost in frame 1, so frame 2 ... are ungated
    _, lost = M.clean_sequence(x[[0, 0, 1]], np.pad(np.ones((1, 1), np.uint8), ((10, 29), (10, 89))), radius=0, chain=True)
    assert np.array_equal(lost[0], obj[0]) and np.array_equal(lost[1], obj[0]) and np.array_equal(lost[2], obj[1])
    # without a chain every frame takes its own seed
    seeds = np.stack([seed0, np.zeros_like(seed0), seed0, seed0])
    _, own = M.clean_sequence(x, seeds, radius=0, chain=False)
    assert np.array_equal(own[0], obj[0]) and np.array_equal(own[1], M.logits_mask(x[1])) and np.array_equal(own[3], obj[3])
    _, free = M.clean_sequence(x, None, chain=False, largest=True)
    assert np.array_equal(free[0], obj[0])
    with pytest.raises(ValueError):
        M.clean_sequence(x, seeds, chain=True)
    with pytest.raises(ValueError):
        M.clean_sequence(x, seed0, chain=False)
    with pytest.raises(ValueError):
        M.clean_sequence(x.astype(np.float64), None)


def test_clean_options():
    from fosvos_hip.options import CleanOptions
    o = CleanOptions()
    assert (o.min_area, o.largest, o.temporal_radius, o.fill, o.chain) == (0, False, None, -100.0, False)
    o = CleanOptions(min_area=7, largest=True, temporal_radius=0, fill=-3)
    assert o.chain and o.as_dict() == {"min_area": 7, "largest": True, "temporal_radius": 0, "fill": -3.0}
    assert CleanOptions(temporal_radius=63).temporal_radius == 63
    for bad in (dict(min_area=-1), dict(min_area=1.0), dict(min_area=True), dict(largest=1), dict(temporal_radius=64),
                dict(temporal_radius=-1), dict(temporal_radius=2.0), dict(fill=0.0), dict(fill=float("-inf")),
                dict(fill=float("nan")), dict(fill=5.0), dict(fill=-1e39), dict(fill="x")):
        with pytest.raises(ValueError, match="CleanOptions"):
            CleanOptions(**bad)
    with pytest.raises(Exception):
        o.min_area = 3  # frozen
    # no environment variable is read
    import inspect
    from fosvos_hip import options
    source = inspect.getsource(options.CleanOptions)
    assert "os.environ" not in source and "getenv" not in source and "from_env" not in source


# ------------------------------------------------------------------------------------------ run_webcam, train_online
class StubNet:
    def cuda(self):
        return self

    def eval(self):
        return self


class StubSegmenter:
    built, seeds = [], []

    def __init__(self, net, height, width, **kw):
        StubSegmenter.built.append(((height, width), kw))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False

    def seed(self, mask):
        StubSegmenter.seeds.append(mask)

    def segment(self, frames):
        yield from frames


@pytest.fixture
def webcam(monkeypatch):
    import run_webcam
    from fosvos_hip import stream
    StubSegmenter.built, StubSegmenter.seeds = [], []
    monkeypatch.setattr(run_webcam, "get_network", lambda *a, **k: StubNet())
    monkeypatch.setattr(stream, "FrameSegmenter", StubSegmenter)
    monkeypatch.setattr(stream, "ObjectSegmenter", StubSegmenter)
    return run_webcam


def test_run_webcam_clean_flags(webcam, tmp_path):
    from fosvos_hip.options import CleanOptions
    base = ["--synthetic", "2", "--height", "24", "--width", "40"]
    assert len(webcam.main(base)) == 2
    assert StubSegmenter.built[-1][0] == (24, 40) and "clean" not in StubSegmenter.built[-1][1]  # absent: built as it was
    webcam.main(base + ["--clean-min-area", "50"])
    assert StubSegmenter.built[-1][1]["clean"] == CleanOptions(min_area=50)
    webcam.main(base + ["--clean-largest"])
    assert StubSegmenter.built[-1][1]["clean"] == CleanOptions(largest=True)
    webcam.main(base + ["--clean-temporal", "0", "--clean-largest", "--clean-min-area", "3"])
    assert StubSegmenter.built[-1][1]["clean"] == CleanOptions(min_area=3, largest=True, temporal_radius=0)
    assert StubSegmenter.seeds == []
    from PIL import Image
    seed = np.zeros((24, 40), np.uint8)
    seed[3:9, 5:20] = 200
    Image.fromarray(seed, mode="L").save(str(tmp_path / "seed.png"))
    webcam.main(base + ["--clean-temporal", "8", "--clean-seed", str(tmp_path / "seed.png")])
    assert StubSegmenter.built[-1][1]["clean"] == CleanOptions(temporal_radius=8)
    assert len(StubSegmenter.seeds) == 1 and np.array_equal(StubSegmenter.seeds[0], (seed != 0).astype(np.uint8))


@pytest.mark.parametrize("extra,reason", [
    (["--clean-seed", "x.png"], "--clean-temporal"),
    (["--clean-seed", "x.png", "--clean-largest"], "--clean-temporal"),
    (["--clean-largest", "--no-network"], "--no-network"),
    (["--clean-min-area", "4", "--no-network"], "--no-network"),
    (["--clean-temporal", "4", "--no-network"], "--no-network"),
    (["--clean-largest", "--models", "a.pth", "b.pth"], "--models"),
    (["--clean-temporal", "2", "--models", "a.pth"], "--models"),
    (["--clean-min-area", "-1"], "--clean-min-area"),
    (["--clean-temporal", "64"], "--clean-temporal"),
    (["--clean-temporal", "-1"], "--clean-temporal"),
    (["--clean-min-area", "many"], "invalid int"),
])
def test_run_webcam_refuses_with_a_reason(webcam, capsys, extra, reason):
    with pytest.raises(SystemExit):
        webcam.main(["--synthetic", "1", "--height", "24", "--width", "40"] + extra)
    assert reason in capsys.readouterr().err
    assert StubSegmenter.built == []


def test_train_online_clean_flags(capsys):
    from util import args_helper
    a = args_helper.parse_args(is_online=True, argv=["--synthetic"])
    assert a.clean_min_area is None and a.clean_largest is False and a.clean_temporal is None
    a = args_helper.parse_args(is_online=True, argv=["--synthetic", "--fast-test", "--clean-min-area", "9", "--clean-largest",
                                                     "--clean-temporal", "12"])
    assert (a.clean_min_area, a.clean_largest, a.clean_temporal) == (9, True, 12)
    for argv, reason in ((["--clean-largest"], "--fast-test"), (["--clean-min-area", "3", "--score"], "--fast-test"),
                         (["--clean-temporal", "3"], "--fast-test"),
                         (["--fast-test", "--clean-largest", "--multi-object"], "--multi-object"),
                         (["--fast-test", "--clean-temporal", "64"], "0..63"),
                         (["--fast-test", "--clean-min-area", "-2"], ">= 0")):
        with pytest.raises(SystemExit):
            args_helper.parse_args(is_online=True, argv=["--synthetic"] + argv)
        assert reason in capsys.readouterr().err, argv
    with pytest.raises(SystemExit):  # an offline run has no such flag
        args_helper.parse_args(is_online=False, argv=["--clean-largest"])


def test_train_online_seed_choice():
    import train_online
    from dataloaders.synthetic import SyntheticSequence
    from torch.utils.data import DataLoader
    train = DataLoader(SyntheticSequence("blob", 24, 40, n_frames=1, seed=1234), batch_size=1)
    seed = train_online._train_annotation(train)
    assert seed.dtype == np.uint8 and seed.shape == (24, 40) and 0 < seed.sum() < seed.size
    assert np.array_equal(seed, (np.asarray(train.dataset[0]["gt"])[0] >= 0.5).astype(np.uint8))
    test = DataLoader(SyntheticSequence("blob", 24, 40, n_frames=3, seed=1234), batch_size=1)
    assert train_online._train_annotation(test) is None          # not a one-shot loader
    ann = test.dataset.annotation
    assert train_online._clean_seed(seed, ann, test, "blob") is seed                   # 1. this call trained
    assert np.array_equal(train_online._clean_seed(None, ann, test, "blob"), (ann("blob", "00000") != 0).astype(np.uint8))
    assert train_online._clean_seed(None, None, test, "blob") is None                  # 3. nothing: not gated


def test_test_fast_checks_its_clean_arguments(tmp_path):
    from fosvos_hip.options import CleanOptions
    from util import experiment_helper

    class Provider:
        network = None

    class Loader:
        dataset = []

        def __iter__(self):
            return iter(())

    seed = np.ones((4, 4), np.uint8)
    for kw in (dict(clean_seed=seed), dict(clean=CleanOptions(largest=True), clean_seed=seed), dict(clean={"largest": True}),
               dict(clean=CleanOptions(temporal_radius=1), clean_seed=np.ones((4, 4), np.float32)),
               dict(clean=CleanOptions(temporal_radius=1), clean_seed=np.ones((1, 4, 4), np.uint8))):
        with pytest.raises(ValueError, match="clean"):
            experiment_helper.test_fast(Provider(), Loader(), tmp_path, **kw)
    assert experiment_helper.test_fast(Provider(), Loader(), tmp_path, clean=CleanOptions(temporal_radius=1),
                                       clean_seed=seed) is None
    assert experiment_helper.last_fast["clean"] == CleanOptions(temporal_radius=1).as_dict()
    experiment_helper.test_fast(Provider(), Loader(), tmp_path)
    assert "clean" not in experiment_helper.last_fast


def test_fast_cpu_branch_is_clean_sequence(tmp_path):
    """The CPU-logits branch: the files and counts are those of clean_sequence's logits, the seed carried over the groups."""
    import torch
    from fosvos_hip.options import CleanOptions
    from util import experiment_helper, png_layout
    x, obj = sequence_maps()
    order = [0, 1, 3, 1, 0, 3]           # 6 frames: groups of 5 + 1, the seed crosses the group border
    x, obj = x[order], obj[order]
    n, h, w = x.shape

    class Net:
        at = 0

        def forward(self, inputs):
            k = int(inputs.shape[0])
            out = torch.from_numpy(x[self.at:self.at + k].copy())[:, None]
            self.at += k
            return [out]

    class Provider:
        def __init__(self):
            self.network = Net()

    class Frames(list):
        pass

    def loader():
        held = Frames({"image": torch.zeros((3, h, w)), "seq_name": "s", "fname": "%05d" % k} for k in range(n))
        from torch.utils.data import DataLoader
        return DataLoader(held, batch_size=1, shuffle=False)

    gts = obj.astype(np.uint8)

    def annotations(seq, fname):
        return gts[int(fname)]

    import util.gpu_handler as gpu_handler
    keep = gpu_handler.cast_cuda_if_possible
    gpu_handler.cast_cuda_if_possible = lambda ts: ts
    try:
        opts = CleanOptions(temporal_radius=4, min_area=2)
        score = experiment_helper.test_fast(Provider(), loader(), tmp_path / "clean", annotations, seq_name="s", clean=opts,
                                            clean_seed=obj[0])
        plain = experiment_helper.test_fast(Provider(), loader(), tmp_path / "plain", annotations, seq_name="s")
    finally:
        gpu_handler.cast_cuda_if_possible = keep
    assert score["clean"] == opts.as_dict() and "clean" not in plain
    want, kept = M.clean_sequence(x, obj[0], 4, 2, False, chain=True)
    assert not np.array_equal(want, x)
    radius = davis_measures.default_radius(h, w)
    for k in range(n):
        assert score["counts"][k] == [int(v) for v in davis_measures.jf_counts_numpy(want[k] >= 0, gts[k], radius)], k
        prob = experiment_helper.bytescale(1.0 / (1.0 + np.exp(-want[k].astype(np.float64))))
        assert (tmp_path / "clean" / "s" / ("%05d.png" % k)).read_bytes() == png_layout.encode(prob), k
    assert score["J"][1] == 1.0 and plain["J"][1] < 1.0   # the far blob is gone from frame 1
    assert np.array_equal(kept[5], obj[5]) and score["J"][5] == 1.0 and plain["J"][5] < 1.0   # ... and behind the group border


# ------------------------------------------------------------------------------------------ the C entries, no device
def lib():
    import fosvos_hip
    return fosvos_hip.lib()


def test_abi_and_workspace_query():
    import fosvos_hip
    L = lib()
    assert fosvos_hip.ABI_VERSION == 34 and L.fosvos_abi_version() == 34
    with open(fosvos_hip.HEADER_PATH) as f:
        assert "#define FOSVOS_ABI_VERSION 34" in f.read()
    q = L.fosvos_components_workspace_bytes
    for n, h, w in ((1, 1, 1), (3, 33, 130), (5, 480, 854)):
        words = h * ((w + 63) // 64)
        assert q(n, h, w) == n * (8 + 16 * words + 8 * h * w + 4)   # the formula
    assert q(0, 4, 4) == 0 and q(1, 0, 4) == 0 and q(1, 4, -1) == 0 and q(65536, 4, 4) == 0
    assert q(1, 46341, 46341) == 0 and q(1, 32768, 65536) == 0 and q(1, 32768, 65535) > 0   # H W < 2^31


def test_entries_return_error_codes_without_a_device():
    L = lib()
    E_SHAPE, E_ARG, E_WS = -1, -2, -3
    p = ctypes.c_void_p(4096)  # never dereferenced: every call below fails its checks first

    def clean(logits=p, seed=None, n=1, h=8, w=8, radius=0, min_area=0, largest=0, chain=0, fill=-100.0, out=p, kept=None,
              ws=p, ws_bytes=1 << 20):
        return L.fosvos_clean_components(logits, seed, n, h, w, radius, min_area, largest, chain, fill, out, kept, ws, ws_bytes,
                                         0, None)

    assert clean(logits=None) == E_ARG and b"null" in L.fosvos_last_error()
    assert clean(out=None) == E_ARG and clean(ws=None) == E_ARG
    assert clean(n=0) == E_SHAPE and clean(n=65536) == E_SHAPE and clean(h=0) == E_SHAPE and clean(w=-3) == E_SHAPE
    assert clean(h=65536, w=32768) == E_SHAPE and b"2^31" in L.fosvos_last_error()
    assert clean(radius=-1) == E_ARG and clean(radius=64) == E_ARG and b"radius" in L.fosvos_last_error()
    assert clean(min_area=-1) == E_ARG and b"min_area" in L.fosvos_last_error()
    for fill in (0.0, -0.0, 1.0, float("inf"), float("-inf"), float("nan")):
        assert clean(fill=fill) == E_ARG and b"fill" in L.fosvos_last_error(), fill
    assert clean(ws=ctypes.c_void_p(4100)) == E_ARG and b"aligned" in L.fosvos_last_error()
    need = L.fosvos_components_workspace_bytes(1, 8, 8)
    assert clean(ws_bytes=need - 1) == E_WS and clean(ws_bytes=0) == E_WS
    roots = L.fosvos_component_roots
    assert roots(None, 1, 8, 8, p, None, 0, 0, None) == E_ARG and roots(p, 1, 8, 8, None, None, 0, 0, None) == E_ARG
    assert roots(p, 0, 8, 8, p, None, 0, 0, None) == E_SHAPE and roots(p, 1, 65536, 32768, p, None, 0, 0, None) == E_SHAPE
