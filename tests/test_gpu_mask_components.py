"""Cleaning a mask by its shape on a real MI355X: ``ops.component_roots`` and ``ops.clean_components``
(csrc/components.hip) against the numpy statement (util/mask_components.py) with exact equality - the label map element for
element, the cleaned logits on their int32 view, the kept mask byte for byte - and ``FrameSegmenter(clean=)`` and
``test_fast(clean=)`` end to end on stub nets whose logits are planted maps."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fosvos_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mask_component_cases as C  # noqa: E402
from util import frame_overlay as F  # noqa: E402
from util import frame_resample as R  # noqa: E402
from util import mask_components as M  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(1, 5, 67), (3, 33, 130), (2, 16, 64), (1, 96, 160), (1, 150, 300), (1, 1, 1), (1, 1, 200), (1, 200, 1)]
IDS = ["%dx%dx%d" % s for s in SHAPES]
RADII, MIN_AREAS = (0, 1, 5, 63), (0, 1, 7)


# ------------------------------------------------------------------------------------------ the reference, computed once
@pytest.fixture(scope="module", autouse=True)
def cached_reference():
    """The labelling and the dilation of the numpy statement do not depend on the rules a case is cleaned by: both are
    computed once per mask / per seed and radius, and shared by every combination below.  The functions themselves are
    untouched."""
    roots_of, dilate_of, memo_r, memo_d = M.component_roots, M.dilate_disk, {}, {}

    def roots(mask):
        mask = np.ascontiguousarray(mask, dtype=bool)
        key = (mask.shape, mask.tobytes())
        if key not in memo_r:
            memo_r[key] = roots_of(mask)
        return memo_r[key]

    def dilate(seed, radius):
        seed = np.ascontiguousarray(seed, dtype=bool)
        key = (seed.shape, int(radius), seed.tobytes())
        if key not in memo_d:
            memo_d[key] = dilate_of(seed, radius)
        return memo_d[key]

    M.component_roots, M.dilate_disk = roots, dilate
    yield
    M.component_roots, M.dilate_disk = roots_of, dilate_of


_BATCHES = {}


def batches(n, h, w):
    """[(names, logits float32 [n,h,w])]: every case of the frame size, n frames a batch (the last one filled up from the
    front)."""
    if (n, h, w) not in _BATCHES:
        cases = C.mask_cases(h, w)
        if (h, w) == (150, 300):
            cases += [(name, logits) for name, logits, _, _, _ in C.gate_cases()[::5]]
        out = []
        for k in range(0, len(cases), n):
            chunk = (cases[k:k + n] + cases[:n])[:n]
            out.append(([c[0] for c in chunk], np.stack([c[1] for c in chunk])))
        _BATCHES[(n, h, w)] = out
    return _BATCHES[(n, h, w)]


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def run_clean(x, seed=None, **kw):
    """(out float32 [n,h,w], kept uint8 [n,h,w]) of the op, on the host."""
    n, h, w = x.shape
    kept = torch.full((n, h, w), 0xA5, dtype=torch.uint8, device=DEV)
    out = hip_ops().clean_components(dev(x)[:, None], None if seed is None else dev(seed), kept=kept, **kw)
    assert out.shape == (n, 1, h, w) and out.dtype == torch.float32
    return out[:, 0].cpu().numpy(), kept.cpu().numpy()


def hip_ops():
    from fosvos_hip import ops
    return ops


def assert_clean(x, seed, radius, min_area, largest, chain, what):
    got, got_kept = run_clean(x, seed, radius=radius, min_area=min_area, largest=largest, chain=chain)
    want, want_kept = M.clean_sequence(x, None if seed is None else (seed[0] if chain else seed), radius, min_area, largest,
                                       chain=chain)
    assert np.array_equal(got_kept, want_kept.astype(np.uint8)), what
    assert np.array_equal(got.view(np.int32), want.view(np.int32)), what


# ------------------------------------------------------------------------------------------ the label map
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_roots_element_for_element(shape):
    ops = hip_ops()
    n, h, w = shape
    for names, x in batches(n, h, w):
        got = ops.component_roots(dev(x)[:, None])
        assert got.dtype == torch.int32 and tuple(got.shape) == (n, h, w)
        want = np.stack([M.component_roots(M.logits_mask(f)) for f in x])
        assert np.array_equal(got.cpu().numpy(), want), names


@pytest.mark.parametrize("centre", [None, (80, 128), (80, 192), (64, 128)], ids=["frame", "80x128", "80x192", "64x128"])
def test_roots_of_a_diagonal_step_at_every_grid_position(centre):
    """Two blobs joined by one diagonal step, at all 256 offsets around the frame centre and around corners of 16 x 64 tiles
    (the kernel's own), both diagonals: the seams and the four-tile corner."""
    ops = hip_ops()
    cases = C.diagonal_cases(150, 300, centre)
    x = np.stack([c[1] for c in cases])
    assert x.shape == (512, 150, 300)
    got = ops.component_roots(dev(x)[:, None]).cpu().numpy()
    for k, (name, logits) in enumerate(cases):
        want = M.component_roots(M.logits_mask(logits))
        assert len(np.unique(want)) == 2, name   # background and ONE component
        assert np.array_equal(got[k], want), name


def test_roots_into_a_view_and_twice():
    ops = hip_ops()
    x = batches(3, 33, 130)[0][1]
    t = dev(x)[:, None]
    buf = torch.full((x.size + 7,), -77, dtype=torch.int32, device=DEV)
    out = buf[3:3 + x.size].view(3, 33, 130)
    assert ops.component_roots(t, out=out) is out
    first = out.cpu().numpy().copy()
    assert np.array_equal(first, np.stack([M.component_roots(M.logits_mask(f)) for f in x]))
    assert torch.all(buf[:3] == -77) and torch.all(buf[3 + x.size:] == -77)
    assert np.array_equal(ops.component_roots(t).cpu().numpy(), first)


# ------------------------------------------------------------------------------------------ clean_components
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_clean_every_case_and_rule(shape):
    n, h, w = shape
    for names, x in batches(n, h, w):
        seeds = np.stack([C.seed_for(f) for f in x])
        for radius, min_area, largest, seeded, chain in itertools.product(RADII, MIN_AREAS, (False, True), (False, True),
                                                                          (False, True)):
            if not seeded and radius and not (chain and n > 1):
                continue  # the radius is not read
            seed = (seeds[:1] if chain else seeds) if seeded else None
            assert_clean(x, seed, radius, min_area, largest, chain, (names, radius, min_area, largest, seeded, chain))


def test_clean_gate_geometry():
    """A seed pixel at distance exactly r and just beyond, horizontally and on the diagonal, r in {0, 1, 5, 63}; seed and blob
    in different 64-pixel words and tile rows."""
    for name, logits, seed, radius, near in C.gate_cases():
        got, kept = run_clean(logits[None], seed[None], radius=radius)
        by, bx = np.argwhere(logits >= 0)[0]
        assert kept[0, by, bx] == near and kept.sum() == int(near), name
        want, want_kept = M.clean_sequence(logits[None], seed, radius, chain=True)
        assert np.array_equal(kept, want_kept.astype(np.uint8)) and np.array_equal(got.view(np.int32), want.view(np.int32)), name


def chain_maps():
    """An object that drifts and a far blob over five frames at 33 x 130; frame 1 is all background in the second batch."""
    h, w = 33, 130
    frames, obj = [], []
    for k in range(5):
        m = np.zeros((h, w), bool)
        m[8:20, 50 + 5 * k:72 + 5 * k] = True   # crosses the word border at column 64
        o = m.copy()
        m[24:30, 110:126] = True
        frames.append(C.mask_logits(m))
        obj.append(o)
    return np.stack(frames), np.stack(obj)


def test_clean_chain():
    x, obj = chain_maps()
    seed0 = obj[:1].astype(np.uint8)
    for radius, largest in itertools.product(RADII, (False, True)):
        assert_clean(x, seed0, radius, 0, largest, True, ("chain", radius, largest))
        assert_clean(x, None, radius, 0, largest, True, ("chain, unseeded", radius, largest))
    got, kept = run_clean(x, seed0, radius=1, chain=True)
    assert np.array_equal(kept.astype(bool), obj)  # the far blob goes in every frame
    # N = 3 with frame 1 all background: frame 2 is not gated and takes both blobs back
    y = x[:3].copy()
    y[1] = C.mask_logits(np.zeros(y.shape[1:], bool))
    for radius, min_area, largest in itertools.product(RADII, MIN_AREAS, (False, True)):
        assert_clean(y, seed0, radius, min_area, largest, True, ("background frame", radius, min_area, largest))
    got, kept = run_clean(y, seed0, radius=5, chain=True)
    assert np.array_equal(kept[0].astype(bool), obj[0]) and not kept[1].any()
    assert np.array_equal(kept[2].astype(bool), M.logits_mask(x[2]))
    # an empty seed gates nothing, with and without a chain
    none = np.zeros_like(seed0)
    got, kept = run_clean(y, none, radius=3, chain=True)
    assert np.array_equal(kept[0].astype(bool), M.logits_mask(y[0]))
    got, kept = run_clean(y, np.zeros(y.shape, np.uint8), radius=3)
    assert np.array_equal(kept.astype(bool), M.logits_mask(y))


def test_clean_in_place_views_and_twice():
    ops = hip_ops()
    names, x = batches(3, 33, 130)[0]
    n, h, w = x.shape
    seeds = np.stack([C.seed_for(f) for f in x])
    want, want_kept = M.clean_sequence(x, seeds, 5, 7, False, chain=False)
    # in place
    t = dev(x)[:, None]
    assert ops.clean_components(t, dev(seeds), 5, 7, out=t) is t
    assert np.array_equal(t[:, 0].cpu().numpy().view(np.int32), want.view(np.int32))
    # views at an odd float / byte offset, guards around both
    logits_buf = torch.empty(x.size + 1, dtype=torch.float32, device=DEV)
    src = logits_buf[1:].view(n, 1, h, w)
    src.copy_(dev(x)[:, None])
    out_buf = torch.full((4 * (x.size + 8),), 0xA5, dtype=torch.uint8, device=DEV).view(torch.float32)
    out = out_buf[3:3 + x.size].view(n, 1, h, w)
    kept_buf = torch.full((x.size + 10,), 0xA5, dtype=torch.uint8, device=DEV)
    kept = kept_buf[5:5 + x.size].view(n, h, w)
    seed_buf = torch.zeros(x.size + 3, dtype=torch.uint8, device=DEV)
    seed = seed_buf[3:].view(n, h, w)
    seed.copy_(dev(seeds))
    assert src.data_ptr() % 8 == 4 and out.data_ptr() % 8 == 4 and kept.data_ptr() % 2 == 1 and seed.data_ptr() % 2 == 1
    for _ in range(2):  # twice on the same input: the same bytes
        ops.clean_components(src, seed, 5, 7, out=out, kept=kept)
        assert np.array_equal(out[:, 0].cpu().numpy().view(np.int32), want.view(np.int32))
        assert np.array_equal(kept.cpu().numpy(), want_kept.astype(np.uint8))
    guard = out_buf.view(torch.uint8)
    assert torch.all(guard[:12] == 0xA5) and torch.all(guard[12 + 4 * x.size:] == 0xA5)
    assert torch.all(kept_buf[:5] == 0xA5) and torch.all(kept_buf[5 + x.size:] == 0xA5)
    assert np.array_equal(src[:, 0].cpu().numpy().view(np.int32), x.view(np.int32))  # the input is read only
    # a fill of the caller's
    got, _ = run_clean(x, seeds, radius=5, min_area=7, fill=-0.25)
    want2, _ = M.clean_sequence(x, seeds, 5, 7, False, chain=False, fill=-0.25)
    assert np.array_equal(got.view(np.int32), want2.view(np.int32)) and (got == -0.25).any()


def test_op_argument_checks():
    ops = hip_ops()
    x = dev(C.planted_logits(16, 64, 0.41))[None, None]
    seed = torch.zeros((1, 16, 64), dtype=torch.uint8, device=DEV)
    bad_value = [dict(radius=-1), dict(radius=64), dict(radius=1.0), dict(radius=True), dict(min_area=-1), dict(min_area=2.5),
                 dict(fill=0.0), dict(fill=1.0), dict(fill=float("nan")), dict(fill=float("-inf")), dict(fill=-1e39),
                 dict(seed=seed[0]), dict(seed=seed.float()), dict(seed=seed.expand(2, 16, 64)),
                 dict(seed=torch.zeros((2, 16, 64), dtype=torch.uint8, device=DEV), chain=True),
                 dict(out=torch.empty((1, 16, 64), device=DEV)), dict(out=torch.empty((1, 1, 16, 64), dtype=torch.float64, device=DEV)),
                 dict(kept=torch.empty((1, 1, 16, 64), dtype=torch.uint8, device=DEV)),
                 dict(kept=torch.empty((1, 16, 64), dtype=torch.int32, device=DEV))]
    for kw in bad_value:
        with pytest.raises(ValueError, match="clean_components"):
            ops.clean_components(x, **kw)
    for t in (x[0], x.double(), x[..., ::2], torch.empty((0, 1, 4, 4), device=DEV)):
        with pytest.raises(ValueError):
            ops.clean_components(t)
        with pytest.raises(ValueError):
            ops.component_roots(t)
    for kw in (dict(seed=seed.cpu()), dict(out=torch.empty((1, 1, 16, 64))), dict(kept=torch.empty((1, 16, 64), dtype=torch.uint8))):
        with pytest.raises(RuntimeError):
            ops.clean_components(x, **kw)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.clean_components(x.cpu())
    with pytest.raises(RuntimeError, match="GPU"):
        ops.component_roots(x.cpu())
    with pytest.raises(ValueError):
        ops.component_roots(x, out=torch.empty((1, 16, 64), dtype=torch.int64, device=DEV))
    # and the call still works afterwards
    assert np.array_equal(ops.clean_components(x, seed, chain=True)[:, 0].cpu().numpy().view(np.int32),
                          M.clean_sequence(x[0].cpu().numpy(), None)[0].view(np.int32))


def test_entries_return_codes_with_real_pointers():
    import fosvos_hip
    L = fosvos_hip.lib()
    x = dev(C.planted_logits(16, 64, 0.41))[None, None]
    out = torch.empty_like(x)
    need = L.fosvos_components_workspace_bytes(1, 16, 64)
    ws = torch.empty(need + 8, dtype=torch.uint8, device=DEV)
    st = torch.cuda.current_stream().cuda_stream

    def clean(logits=x.data_ptr(), n=1, radius=0, min_area=0, fill=-100.0, o=out.data_ptr(), w=ws.data_ptr(), wn=need):
        return L.fosvos_clean_components(logits, None, n, 16, 64, radius, min_area, 0, 0, fill, o, None, w, wn, 0, st)

    assert clean(logits=None) == -2 and clean(o=None) == -2 and clean(w=None) == -2
    assert clean(n=0) == -1 and clean(n=65536) == -1
    assert clean(radius=64) == -2 and clean(radius=-1) == -2 and clean(min_area=-5) == -2
    for fill in (0.0, 2.0, float("inf"), float("-inf"), float("nan")):
        assert clean(fill=fill) == -2
    assert clean(w=ws.data_ptr() + 4) == -2 and clean(wn=need - 1) == -3
    assert b"workspace" in L.fosvos_last_error()
    assert clean() == 0
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), x.cpu().numpy(), equal_nan=True)  # no rule: everything stays


# ------------------------------------------------------------------------------------------ FrameSegmenter(clean=)
class PlantedNet(torch.nn.Module):
    """A net whose answer to its k-th call is the k-th planted map, whatever it is shown."""

    def __init__(self, maps):
        super().__init__()
        self.anchor = torch.nn.Parameter(torch.zeros(1))
        self.maps = torch.from_numpy(np.ascontiguousarray(maps))[:, None]
        self.at = 0
        self.compute_side_outputs = True

    def forward(self, x):
        n = int(x.shape[0])
        out = self.maps[self.at:self.at + n].clone().to(self.anchor.device)
        assert out.shape[0] == n, "more frames than planted maps"
        self.at += n
        return [out]


def camera_frames(count, h, w, seed=3):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(count)]


def stream_maps():
    x, obj = chain_maps()
    extra = C.planted_logits(33, 130, 0.41)
    background = C.mask_logits(np.zeros((33, 130), bool))
    return np.stack([x[0], x[1], x[2], extra, background, x[3], x[4]]), obj


@pytest.mark.filterwarnings("ignore:invalid value")  # the planted infinities, interpolated with weight 0 by the numpy statement
@pytest.mark.parametrize("scaled", [False, True], ids=["frame_size", "net_size"])
def test_segmenter_clean_is_the_definition(scaled):
    from fosvos_hip.options import CleanOptions
    from fosvos_hip.stream import FrameSegmenter
    maps, obj = stream_maps()
    hn, wn = maps.shape[1:]
    hf, wf = (2 * hn, 2 * wn) if scaled else (hn, wn)
    size = dict(net_size=(hn, wn)) if scaled else {}
    frames = camera_frames(len(maps), hf, wf)

    def paint(frame, logits, mirror=True, overlay=True):
        if scaled:
            return R.apply_scaled(frame, logits, mirror, overlay, True, "r", 1.0)
        return F.apply(frame, logits, mirror, overlay, True, "r", 1.0)

    def run(clean, depth, seed=None, **kw):
        net = PlantedNet(maps).to(DEV)
        with FrameSegmenter(net, hf, wf, depth=depth, clean=clean, **size, **kw) as seg:
            if seed is not None:
                seg.seed(seed)
            return list(seg.segment(iter(frames)))

    # a segmenter without clean gives the bytes it gave before
    plain = run(None, 2)
    for k, frame in enumerate(frames):
        assert np.array_equal(plain[k], paint(frame, maps[k])), k
    seed_net = obj[0].astype(np.uint8)   # in the net's coordinates; the segmenter mirrors by default
    for opts, seed in ((CleanOptions(min_area=7), None), (CleanOptions(largest=True), None),
                       (CleanOptions(temporal_radius=6), None), (CleanOptions(temporal_radius=6), seed_net),
                       (CleanOptions(min_area=3, largest=True, temporal_radius=0, fill=-7.5), seed_net)):
        cleaned, kept = M.clean_sequence(maps, seed, opts.temporal_radius or 0, opts.min_area, opts.largest, chain=opts.chain,
                                         fill=opts.fill)
        given = None if seed is None else np.ascontiguousarray(seed[:, ::-1])
        outs = {depth: run(opts, depth, given) for depth in (1, 2)}
        for k, frame in enumerate(frames):
            want = paint(frame, cleaned[k])
            assert np.array_equal(outs[1][k], want), (opts, k)
            assert np.array_equal(outs[2][k], want), (opts, k)   # depth 1 and depth 2: the same bytes
        if seed is not None and opts.temporal_radius == 6:
            assert np.array_equal(kept[1].astype(bool), obj[1]) and not np.array_equal(cleaned[1], maps[1])  # seed() is honoured
            assert np.array_equal(kept[5], M.logits_mask(maps[5]))  # taken up again after the all-background frame
    # the mask bytes, unmirrored, and a seed of the frame's size
    opts = CleanOptions(temporal_radius=2)
    cleaned, _ = M.clean_sequence(maps, seed_net, 2, chain=True)
    big = np.kron(seed_net, np.ones((hf // hn, wf // wn), np.uint8))
    got = run(opts, 2, big, mirror=False, overlay=False)
    for k, frame in enumerate(frames):
        assert np.array_equal(got[k], paint(frame, cleaned[k], False, False)), k


def test_segmenter_clean_argument_checks():
    from fosvos_hip.options import CleanOptions
    from fosvos_hip.stream import FrameSegmenter, ObjectSegmenter
    maps, _ = stream_maps()
    net = PlantedNet(maps).to(DEV)
    with pytest.raises(ValueError, match="CleanOptions"):
        FrameSegmenter(net, 33, 130, clean=dict(largest=True))
    with pytest.raises(ValueError, match="per-object"):
        ObjectSegmenter([net], 33, 130, clean=CleanOptions(largest=True))
    with FrameSegmenter(net, 33, 130, clean=CleanOptions(largest=True)) as seg:
        with pytest.raises(RuntimeError, match="temporal"):
            seg.seed(np.zeros((33, 130), np.uint8))
    seg = FrameSegmenter(net, 66, 260, net_size=(33, 130), clean=CleanOptions(temporal_radius=1))
    for bad in (np.zeros((33, 131), np.uint8), np.zeros((33, 130), np.float32), np.zeros((1, 33, 130), np.uint8)):
        with pytest.raises(ValueError, match="seed"):
            seg.seed(bad)
    seg.seed(np.ones((33, 130), bool))
    seg.seed(torch.ones((66, 260), dtype=torch.uint8))
    assert seg._seed is not None and int(seg._seed.sum()) == 33 * 130
    seg.close()
    assert seg._seed is None  # close() releases the buffer
    with pytest.raises(RuntimeError, match="closed"):
        seg.seed(np.ones((33, 130), bool))


# ------------------------------------------------------------------------------------------ test_fast(clean=)
class Provider:
    def __init__(self, network):
        self.network = network


def fast_pass(tmp, maps, gts, device, **kw):
    from torch.utils.data import DataLoader
    from util import experiment_helper
    n, h, w = maps.shape
    held = [{"image": torch.zeros((3, h, w)), "seq_name": "s", "fname": "%05d" % k} for k in range(n)]
    net = PlantedNet(maps).to(device)
    score = experiment_helper.test_fast(Provider(net), DataLoader(held, batch_size=1, shuffle=False), tmp,
                                        lambda seq, fname: gts[int(fname)], seq_name="s", **kw)
    files = [(tmp / "s" / ("%05d.png" % k)).read_bytes() for k in range(n)]
    return score, files


def test_fast_clean_is_the_cpu_branch(tmp_path):
    from fosvos_hip.options import CleanOptions
    x, obj = chain_maps()
    order = [0, 1, 2, 3, 4, 3, 2]        # 7 frames: groups of 5 + 2, the seed crosses the group border on the device
    maps, gts = x[order], obj[order].astype(np.uint8)
    plain, plain_files = fast_pass(tmp_path / "plain", maps, gts, DEV)
    none, none_files = fast_pass(tmp_path / "none", maps, gts, DEV, clean=None)
    assert none_files == plain_files and none["counts"] == plain["counts"] and "clean" not in none
    for k, (opts, seed) in enumerate(((CleanOptions(temporal_radius=8), obj[0]), (CleanOptions(temporal_radius=8), None),
                                      (CleanOptions(min_area=97), None), (CleanOptions(largest=True, fill=-3.0), None))):
        kw = dict(clean=opts) if seed is None else dict(clean=opts, clean_seed=seed)
        gpu, gpu_files = fast_pass(tmp_path / ("gpu%d" % k), maps, gts, DEV, **kw)
        cpu, cpu_files = fast_pass(tmp_path / ("cpu%d" % k), maps, gts, "cpu", **kw)
        assert gpu_files == cpu_files, opts          # the PNG files, byte for byte
        assert gpu["counts"] == cpu["counts"] and gpu["J"] == cpu["J"] and gpu["F"] == cpu["F"], opts
        assert gpu["clean"] == opts.as_dict() == cpu["clean"]
        if seed is not None or opts.min_area or opts.largest:
            assert gpu_files != plain_files and all(j == 1.0 for j in gpu["J"]) and min(plain["J"]) < 1.0, opts
