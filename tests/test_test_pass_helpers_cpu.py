"""The bookkeeping the four test passes of util/experiment_helper.py share: the frames seen so far, the per-frame counters,
the score dict of one object's sequence and the file writer, on hand-made inputs."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fosvos_amd"))

from util import experiment_helper as E  # noqa: E402

H, W = 4, 6


class Loader:
    def __init__(self, n_frames):
        self.dataset = [None] * n_frames


def minibatch(*indices):
    return {"seq_name": ["blob"] * len(indices), "fname": ["%05d" % k for k in indices]}


def annotation(seq, fname):
    """Object ids 0, 2 and 3; frame 1 has no annotation."""
    if int(fname) == 1:
        return None
    ann = np.zeros((H, W), dtype=np.int64)
    ann[1, 1:3], ann[2, 4] = 2, 3
    return ann


def test_frames_without_annotations(tmp_path):
    frames = E._Frames(Loader(3), tmp_path)
    first, gt, paths = frames.add([minibatch(0), minibatch(1)], H, W, None)
    assert (first, gt) == (0, None) and paths == [tmp_path / "blob" / "00000.png", tmp_path / "blob" / "00001.png"]
    first, gt, paths = frames.add([minibatch(2)], H, W, None)
    assert (first, gt) == (2, None) and paths == [tmp_path / "blob" / "00002.png"]
    assert len(frames) == 3 and frames.fnames == ["00000", "00001", "00002"] and frames.scored == [False] * 3
    assert frames.seqs == ["blob"] * 3


def test_frames_with_annotations_binary_and_ids(tmp_path):
    for ids, values in ((False, (1, 1)), (True, (2, 3))):
        frames = E._Frames(Loader(3), tmp_path)
        first, gt, paths = frames.add([minibatch(0, 1), minibatch(2)], H, W, annotation, ids=ids)
        want = np.zeros((H, W), dtype=np.uint8)
        want[1, 1:3], want[2, 4] = values
        assert first == 0 and gt.dtype == np.uint8 and gt.shape == (3, H, W) and len(paths) == 3
        assert np.array_equal(gt[0], want) and np.array_equal(gt[2], want)
        assert not gt[1].any() and frames.scored == [True, False, True]  # no annotation: a zero row, and not scored


def test_frames_refuse_a_frame_beyond_the_dataset(tmp_path):
    frames = E._Frames(Loader(2), tmp_path)
    frames.add([minibatch(0)], H, W, annotation)
    with pytest.raises(RuntimeError, match="more frames than its dataset holds"):
        frames.add([minibatch(1, 2)], H, W, annotation)
    frames.add([minibatch(1)], H, W, annotation)
    with pytest.raises(RuntimeError, match="more frames than its dataset holds"):
        frames.add([minibatch(2)], H, W, None)
    with pytest.raises(ValueError, match="annotation of blob/00000"):
        E._Frames(Loader(1), tmp_path).add([minibatch(0)], H + 1, W, annotation)


def test_sequence_score_hand_computed(tmp_path):
    """Three frames, the middle one without annotation.  J = inter / union, F from P = match_pred / n_pred_b and
    R = match_gt / n_gt_b: frame 0 has J 6/8, P = R = 1; frame 2 has J 1/4, P = R = 1/2.  Two scored values, so the
    statistics take both: decay is the first minus the last."""
    frames = E._Frames(Loader(5), tmp_path)
    frames.add([minibatch(0, 1, 2)], H, W, annotation)
    counts = np.array([[6, 8, 4, 4, 4, 4], [9, 9, 9, 9, 9, 9], [1, 4, 2, 2, 1, 1]], dtype=np.int64)
    score = E._sequence_score(frames, counts, 3, 1.5, None, adapt={"steps": 1})
    assert score == {"seq_name": "blob", "radius": 3, "fnames": ["00000", "00001", "00002"], "scored": [True, False, True],
                     "counts": [[6, 8, 4, 4, 4, 4], None, [1, 4, 2, 2, 1, 1]],
                     "J": [0.75, None, 0.25], "F": [1.0, None, 0.5],
                     "J_stats": {"mean": 0.5, "recall": 0.5, "decay": 0.5},
                     "F_stats": {"mean": 0.75, "recall": 0.5, "decay": 0.5},
                     "J&F": 0.625, "seconds": 1.5, "adapt": {"steps": 1}}
    assert all(type(v) is int for v in score["counts"][0]) and type(score["scored"][0]) is bool
    assert E._sequence_score(frames, counts, 3, 1.5, "named")["seq_name"] == "named"
    assert "adapt" not in E._sequence_score(frames, counts, 3, 1.5, "named")


def test_counters_host_and_tensor():
    counts = E._Counters(4, 2, 6)
    assert counts.host.shape == (4, 2, 6) and counts.host.dtype == np.int64 and counts.dev is None
    counts.host[1] = 7
    assert counts.read(3).shape == (3, 2, 6) and counts.read(3)[1, 1, 5] == 7
    counts = E._Counters(4, 3)
    rows = counts.rows(1, 2, "cpu")
    assert rows.dtype == torch.int32 and tuple(rows.shape) == (2, 3) and not rows.any()
    rows += 5
    counts.rows(3, 1, "cpu")[0, 2] = 1      # the same tensor: made once
    got = counts.read(4)
    assert got.dtype == np.int64 and got.tolist() == [[0, 0, 0], [5, 5, 5], [5, 5, 5], [0, 0, 1]]


def test_file_writer_counts_bytes(tmp_path):
    files = E._FileSlots()
    files.write([tmp_path / "a" / "0.png", tmp_path / "b" / "c" / "1.png"], [b"abc", np.arange(5, dtype=np.uint8).data])
    assert (tmp_path / "a" / "0.png").read_bytes() == b"abc"
    assert (tmp_path / "b" / "c" / "1.png").read_bytes() == bytes(range(5)) and files.png_bytes == 8
