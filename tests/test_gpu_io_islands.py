"""The byte-oriented kernels on islands (tests/islands.py): the stream's prep and overlay, the scoring kernels, the label merge,
both file encoders, the training-sample augmentation and the pseudo-label gate, each through the raw C ABI on the current
stream.  Every operand sits alone between margins at the least alignment its entry accepts, every workspace holds exactly
the bytes the size query reports, every form runs on zero, NaN and large random surroundings, and every output is compared
with the numpy / integer definition bit for bit (tests/io_island_cases.py holds the forms and the references, and
tests/test_io_island_cases_cpu.py checks them without a GPU).  The file encoders' ``out`` is an in-out operand: the bytes
behind a file are the pre-fill, under two different pre-fills."""
import ctypes
import os
import sys
import time

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fosvos_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import io_island_cases as C  # noqa: E402
import islands as I  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RAN = set()


def _stream():
    return torch.cuda.current_stream(0).cuda_stream


def _mean():
    return (ctypes.c_float * 3)(*C.MEANVAL)


def _ws(L, f, reported):
    """The workspace island holds exactly what the size query reports (and the cases module restates)."""
    need = f.op("workspace").shape[0]
    assert int(reported) == need > 0, (f.entry, f.tag, int(reported), need)
    return need


def call_frame_prep(L, f, isl):
    a = f.args
    return L.fosvos_frame_prep(isl.ptr("frames"), a["N"], a["H"], a["W"], a["mirror"], _mean(), isl.ptr("image"), 0, _stream())


def call_frame_prep_scaled(L, f, isl):
    a = f.args
    return L.fosvos_frame_prep_scaled(isl.ptr("frames"), a["N"], a["Hf"], a["Wf"], a["Hn"], a["Wn"], a["mirror"], _mean(),
                                      isl.ptr("image"), 0, _stream())


def call_overlay(L, f, isl):
    a = f.args
    frames = isl.ptr("frames") if f.has("frames") else None  # the mask modes: a null pointer
    return L.fosvos_overlay(frames, isl.ptr("logits"), a["N"], a["H"], a["W"], a["mirror"], a["mode"], a["channel"], a["alpha"],
                            isl.ptr("out"), 0, _stream())


def call_overlay_scaled(L, f, isl):
    a = f.args
    frames = isl.ptr("frames") if f.has("frames") else None
    return L.fosvos_overlay_scaled(frames, isl.ptr("logits"), a["N"], a["Hf"], a["Wf"], a["Hn"], a["Wn"], a["mirror"], a["mode"],
                                   a["channel"], a["alpha"], isl.ptr("out"), 0, _stream())


def call_prob_bytes(L, f, isl):
    a = f.args
    return L.fosvos_prob_bytes(isl.ptr("logits"), a["N"], a["H"], a["W"], isl.ptr("minmax"), isl.ptr("out"), 0, _stream())


def call_jf_counts(L, f, isl):
    a = f.args
    need = _ws(L, f, L.fosvos_jf_workspace_bytes(a["N"], a["H"], a["W"]))
    return L.fosvos_jf_counts(isl.ptr("logits"), isl.ptr("gt"), a["N"], a["H"], a["W"], a["radius"], isl.ptr("counts"),
                              isl.ptr("workspace"), need, 0, _stream())


def call_jf_counts_labels(L, f, isl):
    a = f.args
    need = _ws(L, f, L.fosvos_jf_labels_workspace_bytes(a["N"], a["K"], a["H"], a["W"]))
    return L.fosvos_jf_counts_labels(isl.ptr("pred"), isl.ptr("gt"), a["N"], a["K"], a["H"], a["W"], a["radius"], isl.ptr("counts"),
                                     isl.ptr("workspace"), need, 0, _stream())


def call_merge_objects(L, f, isl):
    a = f.args
    table = (ctypes.c_void_p * a["K"])(*[isl.ptr("map%d" % k) for k in range(a["K"])])
    return L.fosvos_merge_objects(table, a["K"], a["N"], a["H"], a["W"], isl.ptr("labels"), 0, _stream())


def call_png_encode(L, f, isl):
    a = f.args
    assert int(L.fosvos_png_capacity_bytes(a["N"], a["H"], a["W"])) == a["capacity"]
    need = _ws(L, f, L.fosvos_png_workspace_bytes(a["N"], a["H"], a["W"], a["huffman"]))
    return L.fosvos_png_encode(isl.ptr("bytes"), a["N"], a["H"], a["W"], a["huffman"], isl.ptr("out"), a["capacity"],
                               isl.ptr("lengths"), isl.ptr("workspace"), need, 0, _stream())


def call_png_encode_indexed(L, f, isl):
    a = f.args
    assert int(L.fosvos_png_indexed_capacity_bytes(a["N"], a["H"], a["W"])) == a["capacity"]
    need = _ws(L, f, L.fosvos_png_workspace_bytes(a["N"], a["H"], a["W"], a["huffman"]))
    return L.fosvos_png_encode_indexed(isl.ptr("bytes"), isl.ptr("palette"), a["N"], a["H"], a["W"], a["huffman"], isl.ptr("out"),
                                       a["capacity"], isl.ptr("lengths"), isl.ptr("workspace"), need, 0, _stream())


def call_jpeg_encode(L, f, isl):
    a = f.args
    shape = (a["N"], a["H"], a["W"], a["components"], a["sampling"])
    assert int(L.fosvos_jpeg_capacity_bytes(*shape)) == a["out_stride"]
    need = _ws(L, f, L.fosvos_jpeg_workspace_bytes(*shape))
    return L.fosvos_jpeg_encode(isl.ptr("frames"), *shape, a["quality"], isl.ptr("out"), a["out_stride"], isl.ptr("lengths"),
                                isl.ptr("workspace"), need, 0, _stream())


def call_augment_sample(L, f, isl):
    a = f.args
    tables = [isl.ptr(name) if f.has(name) else None for name, _ in C._AUG_TABLES]
    return L.fosvos_augment_sample(isl.ptr("frame"), isl.ptr("mask"), a["H"], a["W"], a["flip"], *tables, a["OH"], a["OW"],
                                   isl.ptr("img_lut"), isl.ptr("gt_lut"), isl.ptr("image"), isl.ptr("gt"), 0, _stream())


def call_distance_gate(L, f, isl):
    a = f.args
    need = _ws(L, f, L.fosvos_distance_gate_workspace_bytes(a["N"], a["H"], a["W"]))
    return L.fosvos_distance_gate(isl.ptr("mask"), a["N"], a["H"], a["W"], a["distance"], a["invert"], isl.ptr("out"),
                                  isl.ptr("workspace"), need, 0, _stream())


def call_adapt_labels(L, f, isl):
    a = f.args
    need = _ws(L, f, L.fosvos_adapt_labels_workspace_bytes(a["N"], a["H"], a["W"]))
    return L.fosvos_adapt_labels(isl.ptr("logits"), isl.ptr("last_mask"), a["N"], a["H"], a["W"], a["pos_logit"], a["neg_distance"],
                                 a["erode"], isl.ptr("label"), isl.ptr("void_px"), isl.ptr("counts"), isl.ptr("workspace"), need,
                                 0, _stream())


CALLS = {name[len("call_"):]: fn for name, fn in list(globals().items()) if name.startswith("call_")}


def test_every_entry_of_the_table_has_a_call():
    assert set(CALLS) == set(C.ENTRIES)


@pytest.mark.parametrize("entry", C.ENTRIES)
def test_entry_touches_nothing_outside_its_operands(entry):
    from fosvos_hip import check, lib
    L = lib()
    forms = C.forms(entry)
    expected = [C.island_expected(f, torch) for f in forms]  # (the references, outside the clock)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rep = I.Report(entry)
    for f, want in zip(forms, expected):
        def call(isl, f=f):
            check(CALLS[entry](L, f, isl), entry)

        rep.add(I.run_case(f.tag, C.island_operands(f, I, torch), call, want, device=DEV, seed=f.seed))
    print("io islands: %s, %d forms, %.2f s" % (entry, len(forms), time.perf_counter() - t0))
    RAN.add(entry)
    rep.done()


def test_every_entry_of_the_table_ran():
    """(After the entries' tests, in file order.)  No skip list, no sampling: what ran is the table."""
    assert RAN == set(C.ENTRIES), sorted(set(C.ENTRIES) - RAN)
