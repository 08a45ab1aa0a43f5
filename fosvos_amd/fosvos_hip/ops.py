"""Tensor-level wrappers over the C ABI: check devices/dtypes/contiguity, pass raw pointers and the
current HIP stream, raise on any non-zero return.  No arithmetic happens in Python here.

Activations are torch.bfloat16 NHWC tensors ([N,H,W,C]); frames / logits are fp32 NCHW as in the
reference; side maps are fp32 NHWC [N,h,w,16].
"""
from __future__ import annotations

import ctypes
import math
from typing import List, Optional, Sequence, Tuple

import torch

from . import CONV_OUT_F32, CONV_RELU, check, int_array4, lib, limits, ptr_array4

_BF16 = torch.bfloat16
_F32 = torch.float32


def _need(t: torch.Tensor, dtype, what: str, dtype_error=TypeError) -> torch.Tensor:
    """``t`` where it is a contiguous ``dtype`` tensor on the GPU.  A wrong dtype is a TypeError in the ops of the training
    step and a ValueError (``dtype_error``) in the ops from ``prob_bytes`` down, as each was written."""
    if not t.is_cuda:
        raise RuntimeError(f"{what}: tensor must live on the GPU (the HIP path has no CPU fallback)")
    if t.dtype != dtype:
        raise dtype_error(f"{what}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{what}: tensor must be contiguous")
    return t


def _ctx(t: torch.Tensor) -> Tuple[int, int]:
    dev = t.device.index if t.device.index is not None else torch.cuda.current_device()
    return dev, torch.cuda.current_stream(dev).cuda_stream


def _p(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _ru(a: int, b: int) -> int:
    return (a + b - 1) // b * b


class Workspace:
    """Grow-only scratch buffer per device AND stream (the library never allocates): ops on one stream are ordered and may
    share their scratch, two models driven on two streams (two host threads) must not."""

    def __init__(self) -> None:
        self._buf = {}

    def get(self, nbytes: int, device: torch.device) -> Tuple[Optional[int], int]:
        if nbytes <= 0:
            return None, 0
        idx = device.index if device.index is not None else torch.cuda.current_device()
        key = (idx, torch.cuda.current_stream(idx).cuda_stream)
        buf = self._buf.get(key)
        if buf is None or buf.numel() < nbytes:
            buf = torch.empty(_ru(nbytes, 1 << 20), dtype=torch.uint8, device=device)
            self._buf[key] = buf
        return buf.data_ptr(), buf.numel()


_WS = Workspace()


# ------------------------------------------------------------------------------------------ profiling
class OpProfiler:
    """Optional per-call timing with HIP events on the launch stream (the current torch stream, which is
    the stream every kernel here is launched on).  Off by default: bench.py turns it on for a few
    iterations AFTER its timed region to obtain per-kernel durations for the roofline line."""

    def __init__(self, detail: bool = False) -> None:
        self.records = []  # (name, flops, bytes, start_event, end_event)
        self.detail = detail  # per-shape names for the generic conv (tests/bench_resnet_infer.py --detail)

    def summary(self):
        torch.cuda.synchronize()
        agg = {}
        for name, flops, nbytes, e0, e1 in self.records:
            a = agg.setdefault(name, {"calls": 0, "ms": 0.0, "flops": 0.0, "bytes": 0.0})
            a["calls"] += 1
            a["ms"] += e0.elapsed_time(e1)
            a["flops"] += flops
            a["bytes"] += nbytes
        return agg


_PROF: Optional[OpProfiler] = None


def set_profiler(p: Optional[OpProfiler]) -> None:
    global _PROF
    _PROF = p


def _pb():
    if _PROF is None:
        return None
    e = torch.cuda.Event(enable_timing=True)
    e.record()
    return e


def _pe(e0, name: str, flops: float = 0.0, nbytes: float = 0.0) -> None:
    if e0 is None:
        return
    e1 = torch.cuda.Event(enable_timing=True)
    e1.record()
    _PROF.records.append((name, float(flops), float(nbytes), e0, e1))


def _launch(entry: str, like: torch.Tensor, *args, record=None, flops: float = 0.0, nbytes: float = 0.0) -> None:
    """The tail of every op: ``fosvos_<entry>(*args, device, stream)`` of ``like``'s device and its current stream, a
    non-zero return raised under the entry's name, the call between the profiler's events.  ``record`` is the profiler's
    name for the call where that is not the entry's (several entries share one); False: the op was never profiled."""
    dev, st = _ctx(like)
    e0 = None if record is False else _pb()
    check(getattr(lib(), "fosvos_" + entry)(*args, dev, st), entry)
    _pe(e0, record or entry, flops, nbytes)


# ------------------------------------------------------------------------------------------ layout
def nchw_to_nhwc_bf16(x: torch.Tensor, c_pad: Optional[int] = None) -> torch.Tensor:
    _need(x, _F32, "nchw_to_nhwc_bf16")
    n, c, h, w = x.shape
    c_pad = _ru(c, 8) if c_pad is None else c_pad
    out = torch.empty((n, h, w, c_pad), dtype=_BF16, device=x.device)
    _launch("nchw_f32_to_nhwc_bf16", x, x.data_ptr(), out.data_ptr(), n, c, h, w, c_pad, record=False)
    return out


def nhwc_bf16_to_nchw(x: torch.Tensor, c: Optional[int] = None) -> torch.Tensor:
    _need(x, _BF16, "nhwc_bf16_to_nchw")
    n, h, w, c_pad = x.shape
    c = c_pad if c is None else c
    out = torch.empty((n, c, h, w), dtype=_F32, device=x.device)
    _launch("nhwc_bf16_to_nchw_f32", x, x.data_ptr(), out.data_ptr(), n, c, h, w, c_pad, record=False)
    return out


def nhwc_f32_to_nchw(x: torch.Tensor) -> torch.Tensor:
    _need(x, _F32, "nhwc_f32_to_nchw")
    n, h, w, c = x.shape
    out = torch.empty((n, c, h, w), dtype=_F32, device=x.device)
    _launch("nhwc_f32_to_nchw_f32", x, x.data_ptr(), out.data_ptr(), n, c, h, w, record=False)
    return out


def nchw_to_nhwc_f32(x: torch.Tensor) -> torch.Tensor:
    _need(x, _F32, "nchw_to_nhwc_f32")
    n, c, h, w = x.shape
    out = torch.empty((n, h, w, c), dtype=_F32, device=x.device)
    _launch("nchw_f32_to_nhwc_f32", x, x.data_ptr(), out.data_ptr(), n, c, h, w, record=False)
    return out


# ------------------------------------------------------------------------------------------ weights
def pack_conv3x3_weights(w: torch.Tensor, want_fwd: bool = True, want_dgrad: bool = True):
    """fp32 OIHW -> (fwd image, dgrad image) as flat bf16 tensors (None when not wanted)."""
    _need(w, _F32, "pack_conv3x3_weights")
    co, ci, kh, kw = w.shape
    if (kh, kw) != (3, 3):
        raise ValueError("pack_conv3x3_weights: 3x3 kernels only")
    L = lib()
    fwd = torch.empty(L.fosvos_packed_weight_elems(co, ci), dtype=_BF16, device=w.device) if want_fwd else None
    dgr = torch.empty(L.fosvos_packed_weight_elems(ci, co), dtype=_BF16, device=w.device) if want_dgrad else None
    _launch("pack_conv3x3_weights", w, w.data_ptr(), co, ci, _p(fwd), _p(dgr), record="pack_weights",
            nbytes=w.numel() * 4 + 2 * ((fwd.numel() if fwd is not None else 0) + (dgr.numel() if dgr is not None else 0)))
    return fwd, dgr


def pack_conv3x3_weights_multi(ws: Sequence[torch.Tensor]):
    """[(fwd image, dgrad image)] of several fp32 OIHW weights in ONE launch (in channels a multiple of 32)."""
    from . import PackEntry
    if not ws:
        return []
    L = lib()
    arr = (PackEntry * len(ws))()
    out = []
    nbytes = 0
    for i, w in enumerate(ws):
        _need(w, _F32, "pack_conv3x3_weights_multi")
        co, ci, kh, kw = w.shape
        if (kh, kw) != (3, 3) or w.device != ws[0].device:
            raise ValueError("pack_conv3x3_weights_multi: 3x3 kernels on one device only")
        fwd = torch.empty(L.fosvos_packed_weight_elems(co, ci), dtype=_BF16, device=w.device)
        dgr = torch.empty(L.fosvos_packed_weight_elems(ci, co), dtype=_BF16, device=w.device)
        arr[i].w, arr[i].w_fwd, arr[i].w_dgrad, arr[i].Co, arr[i].Ci = w.data_ptr(), fwd.data_ptr(), dgr.data_ptr(), co, ci
        out.append((fwd, dgr))
        nbytes += w.numel() * 4 + 2 * (fwd.numel() + dgr.numel())
    _launch("pack_conv3x3_weights_multi", ws[0], arr, len(ws), record="pack_weights", nbytes=nbytes)
    return out


# ------------------------------------------------------------------------------------------ conv
def conv3x3_first_fwd(frame: torch.Tensor, w: torch.Tensor, b: torch.Tensor, want_bits: bool = False):
    """y bf16 NHWC; want_bits: (y, relu_bits) with relu_bits uint8 [N,H,W,Co/8], bit e of byte g = (y[..., 8 g + e] > 0)
    (what conv3x3_dgrad takes as ``relu_bits``)."""
    _need(frame, _F32, "conv3x3_first_fwd frame"); _need(w, _F32, "conv3x3_first_fwd weight"); _need(b, _F32, "conv3x3_first_fwd bias")
    n, c, h, wd = frame.shape
    if c != 3 or tuple(w.shape[1:]) != (3, 3, 3):
        raise ValueError("conv3x3_first_fwd: expects a 3-channel frame and [Co,3,3,3] weights")
    co = w.shape[0]
    y = torch.empty((n, h, wd, co), dtype=_BF16, device=frame.device)
    bits = torch.empty((n, h, wd, co // 8), dtype=torch.uint8, device=frame.device) if want_bits else None
    _launch("conv3x3_first_fwd", frame, frame.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), _p(bits), n, h, wd, co,
            record="conv1_1_fwd", flops=2.0 * n * h * wd * 27 * co, nbytes=n * h * wd * (12 + 2 * co))
    return (y, bits) if want_bits else y


def conv3x3_first_wgrad(frame: torch.Tensor, dy: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    _need(frame, _F32, "conv3x3_first_wgrad frame"); _need(dy, _BF16, "conv3x3_first_wgrad dy")
    n, c, h, wd = frame.shape
    co = dy.shape[3]
    if tuple(dy.shape[:3]) != (n, h, wd):
        raise ValueError("conv3x3_first_wgrad: dy shape mismatch")
    L = lib()
    dw = torch.empty((co, 3, 3, 3), dtype=_F32, device=frame.device)
    db = torch.empty((co,), dtype=_F32, device=frame.device)
    ws, wsn = _WS.get(L.fosvos_conv3x3_first_wgrad_workspace_bytes(n, h, wd, co), frame.device)
    _launch("conv3x3_first_wgrad", frame, frame.data_ptr(), dy.data_ptr(), dw.data_ptr(), db.data_ptr(), n, h, wd, co, ws, wsn,
            record="conv1_1_wgrad", flops=2.0 * n * h * wd * 27 * co, nbytes=n * h * wd * (12 + 2 * co))
    return dw, db


def conv3x3_plan(n: int, h: int, w: int, in_ch: int, out_ch: int) -> dict:
    """The igemm instantiation fosvos_conv3x3_dgrad (and the forward forms the persistent kernel does not take) launch for
    this shape (host arithmetic only): {"tile": (tile_h, tile_w, tile_co), "k_splits", "workgroups", "persistent"}."""
    from . import Conv3x3PlanInfo
    info = Conv3x3PlanInfo()
    check(lib().fosvos_conv3x3_plan(n, h, w, in_ch, out_ch, ctypes.byref(info)), "conv3x3_plan")
    return {"tile": (info.tile_h, info.tile_w, info.tile_co), "k_splits": info.k_splits, "workgroups": info.workgroups,
            "persistent": bool(info.persistent)}


def conv3x3_fwd_plan(n: int, h: int, w: int, in_ch: int, out_ch: int, relu: bool = True) -> dict:
    """What fosvos_conv3x3_fwd / _fwd_pool launch for a bf16-output forward conv of this shape: the persistent eight-wave
    kernel k_conv3x3_pp ("persistent": True, 256 workgroups) where its tiles fill the chip, else the igemm instantiation."""
    from . import Conv3x3PlanInfo
    info = Conv3x3PlanInfo()
    check(lib().fosvos_conv3x3_fwd_plan(n, h, w, in_ch, out_ch, CONV_RELU if relu else 0, ctypes.byref(info)), "conv3x3_fwd_plan")
    return {"tile": (info.tile_h, info.tile_w, info.tile_co), "k_splits": info.k_splits, "workgroups": info.workgroups,
            "persistent": bool(info.persistent)}


def vgg_arena_layout(n: int, h: int, w: int) -> dict:
    """fosvos_vgg_arena_layout as a dict (host arithmetic only): field name -> int, or list of ints for the per-layer arrays
    (byte offsets from the aligned arena base, byte sizes, stage resolutions)."""
    from . import VggArenaLayout
    info = VggArenaLayout()
    check(lib().fosvos_vgg_arena_layout(n, h, w, ctypes.byref(info)), "vgg_arena_layout")
    out = {}
    for name, _ in VggArenaLayout._fields_:
        v = getattr(info, name)
        out[name] = list(v) if isinstance(v, ctypes.Array) else int(v)
    return out


def conv3x3_first_plan(n: int, h: int, w: int) -> Tuple[int, int]:
    """(tiles, persistent workgroups) of fosvos_conv3x3_first_fwd."""
    tiles, wgs = ctypes.c_int(), ctypes.c_int()
    check(lib().fosvos_conv3x3_first_plan(n, h, w, ctypes.byref(tiles), ctypes.byref(wgs)), "conv3x3_first_plan")
    return tiles.value, wgs.value


def conv3x3_fwd(x: torch.Tensor, w_packed: torch.Tensor, bias: Optional[torch.Tensor], ci: int, co: int,
                relu: bool = True, out_f32: bool = False) -> torch.Tensor:
    _need(x, _BF16, "conv3x3_fwd x"); _need(w_packed, _BF16, "conv3x3_fwd packed weight")
    n, h, wd, cx = x.shape
    if cx != _ru(ci, 32):
        raise ValueError(f"conv3x3_fwd: x has {cx} channels, expected {_ru(ci, 32)} (Ci={ci} padded to 32)")
    L = lib()
    if w_packed.numel() != L.fosvos_packed_weight_elems(co, ci):
        raise ValueError("conv3x3_fwd: packed weight size does not match (Co, Ci)")
    if bias is not None:
        _need(bias, _F32, "conv3x3_fwd bias")
        if bias.numel() != co:
            raise ValueError("conv3x3_fwd: bias size")
    y = torch.empty((n, h, wd, co), dtype=_F32 if out_f32 else _BF16, device=x.device)
    flags = (CONV_RELU if relu else 0) | (CONV_OUT_F32 if out_f32 else 0)
    ws, wsn = _WS.get(L.fosvos_conv3x3_workspace_bytes(n, h, wd, ci, co), x.device)
    _launch("conv3x3_fwd", x, x.data_ptr(), w_packed.data_ptr(), _p(bias), y.data_ptr(), n, h, wd, ci, co, flags, ws, wsn,
            flops=2.0 * n * h * wd * 9 * ci * co, nbytes=n * h * wd * (2 * cx + (4 if out_f32 else 2) * co) + 2 * 9 * ci * co)
    return y


def conv3x3_fwd_pool(x: torch.Tensor, w_packed: torch.Tensor, bias: Optional[torch.Tensor], ci: int, co: int,
                     relu: bool = True) -> Tuple[torch.Tensor, torch.Tensor]:
    """conv3x3_fwd (bf16 output) and the 2x2 ceil-mode max pool of its output from one launch: (y, pooled y)."""
    _need(x, _BF16, "conv3x3_fwd_pool x"); _need(w_packed, _BF16, "conv3x3_fwd_pool packed weight")
    n, h, wd, cx = x.shape
    if cx != _ru(ci, 32):
        raise ValueError(f"conv3x3_fwd_pool: x has {cx} channels, expected {_ru(ci, 32)}")
    L = lib()
    if w_packed.numel() != L.fosvos_packed_weight_elems(co, ci):
        raise ValueError("conv3x3_fwd_pool: packed weight size does not match (Co, Ci)")
    if bias is not None:
        _need(bias, _F32, "conv3x3_fwd_pool bias")
    y = torch.empty((n, h, wd, co), dtype=_BF16, device=x.device)
    yp = torch.empty((n, (h + 1) // 2, (wd + 1) // 2, co), dtype=_BF16, device=x.device)
    ws, wsn = _WS.get(L.fosvos_conv3x3_workspace_bytes(n, h, wd, ci, co), x.device)
    _launch("conv3x3_fwd_pool", x, x.data_ptr(), w_packed.data_ptr(), _p(bias), y.data_ptr(), yp.data_ptr(), n, h, wd, ci, co,
            CONV_RELU if relu else 0, ws, wsn, record="conv3x3_fwd", flops=2.0 * n * h * wd * 9 * ci * co,
            nbytes=n * h * wd * (2 * cx + 2 * co) + 2 * 9 * ci * co + yp.numel() * 2)
    return y, yp


def conv3x3_pool_codes_shape(n: int, h: int, w: int, c: int) -> Tuple[int, int, int, int]:
    """Shape of the int32 winner-code tensor of a [n, h, w, c] map: one word per pooled pixel and 8 channels."""
    return (n, (h + 1) // 2, (w + 1) // 2, c // 8)


def conv3x3_fwd_pool_codes(x: torch.Tensor, w_packed: torch.Tensor, bias: Optional[torch.Tensor], ci: int, co: int,
                           out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """conv3x3 + ReLU + 2x2 ceil-mode max pool WITHOUT the dense output: (pooled y, the pool's winner codes as int32
    [N, ceil(H/2), ceil(W/2), Co/8]; fosvos_conv3x3_fwd_pool_codes has the code format).  Only shapes the persistent kernel
    takes; anything else raises.  ``out``: (pooled, codes) tensors to write into."""
    _need(x, _BF16, "conv3x3_fwd_pool_codes x"); _need(w_packed, _BF16, "conv3x3_fwd_pool_codes packed weight")
    n, h, wd, cx = x.shape
    if cx != _ru(ci, 32):
        raise ValueError(f"conv3x3_fwd_pool_codes: x has {cx} channels, expected {_ru(ci, 32)}")
    L = lib()
    if w_packed.numel() != L.fosvos_packed_weight_elems(co, ci):
        raise ValueError("conv3x3_fwd_pool_codes: packed weight size does not match (Co, Ci)")
    if bias is not None:
        _need(bias, _F32, "conv3x3_fwd_pool_codes bias")
        if bias.numel() != co:
            raise ValueError("conv3x3_fwd_pool_codes: bias size")
    if out is None:
        yp = torch.empty((n, (h + 1) // 2, (wd + 1) // 2, co), dtype=_BF16, device=x.device)
        codes = torch.empty(conv3x3_pool_codes_shape(n, h, wd, co), dtype=torch.int32, device=x.device)
    else:
        yp, codes = out
        _need(yp, _BF16, "conv3x3_fwd_pool_codes pooled output")
        if not (codes.is_cuda and codes.is_contiguous() and codes.dtype == torch.int32):
            raise ValueError("conv3x3_fwd_pool_codes: codes must be a contiguous int32 tensor on the GPU")
        if yp.numel() != n * ((h + 1) // 2) * ((wd + 1) // 2) * co or codes.numel() * 4 != L.fosvos_conv3x3_pool_codes_bytes(n, h, wd, co):
            raise ValueError("conv3x3_fwd_pool_codes: output sizes")
    _launch("conv3x3_fwd_pool_codes", x, x.data_ptr(), w_packed.data_ptr(), _p(bias), yp.data_ptr(), codes.data_ptr(), n, h, wd,
            ci, co, CONV_RELU, record="conv3x3_fwd", flops=2.0 * n * h * wd * 9 * ci * co,
            nbytes=n * h * wd * 2 * cx + 2 * 9 * ci * co + yp.numel() * 2 + codes.numel() * 4)
    return yp, codes


def conv3x3_dgrad(dy: torch.Tensor, w_dgrad_packed: torch.Tensor, ci: int, co: int,
                  relu_src: Optional[torch.Tensor] = None, addend: Optional[torch.Tensor] = None,
                  out: Optional[torch.Tensor] = None, relu_bits: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dx[N,H,W,Ci] = mask_{relu_src>0}(dgrad(dy)) + addend.  ``out`` may alias ``addend``.  ``relu_bits`` (uint8
    [N,H,W,Ci/8], instead of ``relu_src``): the same mask as one bit per element (fosvos_conv3x3_dgrad_bits)."""
    _need(dy, _BF16, "conv3x3_dgrad dy"); _need(w_dgrad_packed, _BF16, "conv3x3_dgrad packed weight")
    n, h, wd, cy = dy.shape
    if cy != _ru(co, 32):
        raise ValueError(f"conv3x3_dgrad: dy has {cy} channels, expected {_ru(co, 32)}")
    L = lib()
    if w_dgrad_packed.numel() != L.fosvos_packed_weight_elems(ci, co):
        raise ValueError("conv3x3_dgrad: packed weight size does not match (Ci, Co)")
    shape = (n, h, wd, ci)
    for t, nm in ((relu_src, "relu_src"), (addend, "addend"), (out, "out")):
        if t is not None:
            _need(t, _BF16, f"conv3x3_dgrad {nm}")
            if tuple(t.shape) != shape:
                raise ValueError(f"conv3x3_dgrad: {nm} shape {tuple(t.shape)} != {shape}")
    dx = out if out is not None else torch.empty(shape, dtype=_BF16, device=dy.device)
    ws, wsn = _WS.get(L.fosvos_conv3x3_workspace_bytes(n, h, wd, co, ci), dy.device)
    if relu_bits is not None:
        if relu_src is not None or relu_bits.dtype != torch.uint8 or tuple(relu_bits.shape) != (n, h, wd, ci // 8) or \
                not relu_bits.is_contiguous() or not relu_bits.is_cuda:
            raise ValueError("conv3x3_dgrad: relu_bits must be a contiguous uint8 [N,H,W,Ci/8] GPU tensor, given instead of relu_src")
    mask = relu_src if relu_bits is None else relu_bits
    _launch("conv3x3_dgrad" if relu_bits is None else "conv3x3_dgrad_bits", dy, dy.data_ptr(), w_dgrad_packed.data_ptr(),
            _p(mask), _p(addend), dx.data_ptr(), n, h, wd, ci, co, ws, wsn, record="conv3x3_dgrad",
            flops=2.0 * n * h * wd * 9 * ci * co,
            nbytes=n * h * wd * 2 * (cy + ci * (1 + (relu_src is not None) + (addend is not None))) + 2 * 9 * ci * co)
    return dx


def conv3x3_dgrad_unpool(dy: torch.Tensor, w_dgrad_packed: torch.Tensor, ci: int, co: int, x: torch.Tensor,
                         d_pooled: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dx[N,H,W,Ci] = [x > 0] * dgrad(dy) + maxpool2x2_ceil_bwd(x, d_pooled): the data gradient of a conv whose input ``x`` (a
    post-ReLU stage output) also feeds the 2x2 ceil-mode max pool, the pool's backward in the same pass
    (fosvos_conv3x3_dgrad_unpool; bit for bit ``conv3x3_dgrad(..., relu_src=x, addend=maxpool2x2_ceil_bwd(x, d_pooled))``)."""
    _need(dy, _BF16, "conv3x3_dgrad_unpool dy"); _need(w_dgrad_packed, _BF16, "conv3x3_dgrad_unpool packed weight")
    _need(x, _BF16, "conv3x3_dgrad_unpool x"); _need(d_pooled, _BF16, "conv3x3_dgrad_unpool d_pooled")
    n, h, wd, cy = dy.shape
    if cy != _ru(co, 32):
        raise ValueError(f"conv3x3_dgrad_unpool: dy has {cy} channels, expected {_ru(co, 32)}")
    L = lib()
    if w_dgrad_packed.numel() != L.fosvos_packed_weight_elems(ci, co):
        raise ValueError("conv3x3_dgrad_unpool: packed weight size does not match (Ci, Co)")
    if tuple(x.shape) != (n, h, wd, ci) or tuple(d_pooled.shape) != (n, (h + 1) // 2, (wd + 1) // 2, ci):
        raise ValueError(f"conv3x3_dgrad_unpool: x {tuple(x.shape)} / d_pooled {tuple(d_pooled.shape)} do not match "
                         f"{(n, h, wd, ci)} and its ceil-mode pooled map")
    if out is not None:
        _need(out, _BF16, "conv3x3_dgrad_unpool out")
        if tuple(out.shape) != (n, h, wd, ci) or out.data_ptr() == x.data_ptr():
            raise ValueError("conv3x3_dgrad_unpool: out must have x's shape and must not alias it")
    dx = out if out is not None else torch.empty((n, h, wd, ci), dtype=_BF16, device=dy.device)
    ws, wsn = _WS.get(L.fosvos_conv3x3_workspace_bytes(n, h, wd, co, ci), dy.device)
    _launch("conv3x3_dgrad_unpool", dy, dy.data_ptr(), w_dgrad_packed.data_ptr(), x.data_ptr(), d_pooled.data_ptr(), dx.data_ptr(),
            n, h, wd, ci, co, ws, wsn, flops=2.0 * n * h * wd * 9 * ci * co,
            nbytes=n * h * wd * 2 * (cy + 2 * ci + ci // 4) + 2 * 9 * ci * co)
    return dx


def conv3x3_wgrad(x: torch.Tensor, dy: torch.Tensor, ci: int, co: int, with_bias: bool = True,
                  dw: Optional[torch.Tensor] = None, db: Optional[torch.Tensor] = None, accumulate: bool = False):
    _need(x, _BF16, "conv3x3_wgrad x"); _need(dy, _BF16, "conv3x3_wgrad dy")
    n, h, wd, cx = x.shape
    if cx != ci or tuple(dy.shape) != (n, h, wd, _ru(co, 32)):
        raise ValueError(f"conv3x3_wgrad: shapes x={tuple(x.shape)} dy={tuple(dy.shape)} do not match Ci={ci} Co={co}")
    L = lib()
    if dw is None:
        if accumulate:
            raise ValueError("conv3x3_wgrad: accumulate needs an existing dw")
        dw = torch.empty((co, ci, 3, 3), dtype=_F32, device=x.device)
    if with_bias and db is None:
        if accumulate:
            raise ValueError("conv3x3_wgrad: accumulate needs an existing db")
        db = torch.empty((co,), dtype=_F32, device=x.device)
    _need(dw, _F32, "conv3x3_wgrad dw")
    ws, wsn = _WS.get(L.fosvos_conv3x3_wgrad_workspace_bytes(n, h, wd, ci, co), x.device)
    # the two halves of fosvos_conv3x3_wgrad, timed apart: the MFMA kernel, then the slab reduction (memory-bound; the
    # network call batches the reductions of all layers into two launches)
    _launch("conv3x3_wgrad_slabs", x, x.data_ptr(), dy.data_ptr(), 1 if with_bias else 0, n, h, wd, ci, co, ws, wsn,
            record="conv3x3_wgrad", flops=2.0 * n * h * wd * 9 * ci * co, nbytes=n * h * wd * 2 * (ci + dy.shape[3]))
    _launch("conv3x3_wgrad_reduce", x, dw.data_ptr(), _p(db) if with_bias else None, n, h, wd, ci, co, 1 if accumulate else 0,
            ws, wsn, record="wgrad_reduce", nbytes=4 * 9 * ci * co * 3)
    return dw, (db if with_bias else None)


def conv3x3_wgrad_one_call(x: torch.Tensor, dy: torch.Tensor, ci: int, co: int, with_bias: bool = True):
    """fosvos_conv3x3_wgrad: MFMA kernel and reduction behind one entry point (what a per-layer caller uses)."""
    _need(x, _BF16, "conv3x3_wgrad x"); _need(dy, _BF16, "conv3x3_wgrad dy")
    n, h, wd, _ = x.shape
    L = lib()
    dw = torch.empty((co, ci, 3, 3), dtype=_F32, device=x.device)
    db = torch.empty((co,), dtype=_F32, device=x.device) if with_bias else None
    ws, wsn = _WS.get(L.fosvos_conv3x3_wgrad_workspace_bytes(n, h, wd, ci, co), x.device)
    _launch("conv3x3_wgrad", x, x.data_ptr(), dy.data_ptr(), dw.data_ptr(), _p(db), n, h, wd, ci, co, 0, ws, wsn, record=False)
    return dw, db


# ------------------------------------------------------------------------------------------ pool
def maxpool_fwd(x: torch.Tensor) -> torch.Tensor:
    _need(x, _BF16, "maxpool_fwd")
    n, h, w, c = x.shape
    y = torch.empty((n, (h + 1) // 2, (w + 1) // 2, c), dtype=_BF16, device=x.device)
    _launch("maxpool2x2_ceil_fwd", x, x.data_ptr(), y.data_ptr(), n, h, w, c, record="maxpool_fwd", nbytes=2 * (x.numel() + y.numel()))
    return y


def maxpool_bwd(x: torch.Tensor, dy: torch.Tensor, relu_mask: bool = True) -> torch.Tensor:
    _need(x, _BF16, "maxpool_bwd x"); _need(dy, _BF16, "maxpool_bwd dy")
    n, h, w, c = x.shape
    if tuple(dy.shape) != (n, (h + 1) // 2, (w + 1) // 2, c):
        raise ValueError("maxpool_bwd: dy shape mismatch")
    dx = torch.empty_like(x)
    _launch("maxpool2x2_ceil_bwd", x, x.data_ptr(), dy.data_ptr(), dx.data_ptr(), n, h, w, c, 1 if relu_mask else 0,
            record="maxpool_bwd", nbytes=2 * (2 * x.numel() + dy.numel()))
    return dx


def maxpool_bwd_codes(codes: torch.Tensor, dy: torch.Tensor, h: int, w: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """maxpool_bwd(x, dy, relu_mask=True) of an [N, h, w, C] map from the winner codes conv3x3_fwd_pool_codes wrote for it."""
    _need(dy, _BF16, "maxpool_bwd_codes dy")
    n, oh, ow, c = dy.shape
    if (oh, ow) != ((h + 1) // 2, (w + 1) // 2) or c % 8:
        raise ValueError("maxpool_bwd_codes: dy shape mismatch")
    if not (codes.is_cuda and codes.is_contiguous() and codes.dtype == torch.int32) or codes.numel() != n * oh * ow * (c // 8):
        raise ValueError("maxpool_bwd_codes: codes must be a contiguous int32 [N, ceil(h/2), ceil(w/2), C/8] tensor on the GPU")
    dx = torch.empty((n, h, w, c), dtype=_BF16, device=dy.device) if out is None else out
    if out is not None:
        _need(out, _BF16, "maxpool_bwd_codes out")
        if out.numel() != n * h * w * c:
            raise ValueError("maxpool_bwd_codes: out size")
    _launch("maxpool2x2_ceil_bwd_codes", dy, codes.data_ptr(), dy.data_ptr(), dx.data_ptr(), n, h, w, c, record="maxpool_bwd",
            nbytes=2 * (dx.numel() + dy.numel()) + 4 * codes.numel())
    return dx


def vgg_stage1_compact(n: int, h: int, w: int, flag: bool = True) -> bool:
    """Does a pass of this shape run stage 1 in its compact form when ``PassFlags.compact_stage1`` is (``flag``) set?
    (fosvos_vgg_stage1_compact: host arithmetic only.)"""
    from . import VGG_COMPACT_STAGE1
    return bool(lib().fosvos_vgg_stage1_compact(VGG_COMPACT_STAGE1 if flag else 0, n, h, w))


# ------------------------------------------------------------------------------------------ head
def head_fwd(side: Sequence[torch.Tensor], filt: Sequence[torch.Tensor], filt1: Optional[Sequence[torch.Tensor]],
             dsn_w: Optional[torch.Tensor], dsn_b: Optional[torch.Tensor], fuse_w: torch.Tensor, fuse_b: torch.Tensor,
             H: int, W: int, with_side_out: bool = True, filt_uniform: int = 0):
    """side[s]: fp32 NHWC [N,hs,ws,16]; filt[s]: [k,k,16]; filt1[s]: [k,k]; dsn_w [4,16]; dsn_b [4];
    fuse_w [64]; fuse_b [1].  Returns (fused [N,1,H,W], [4 side outputs] or None).
    filt_uniform: bit s = the caller has checked that filt[s]'s 16 channel filters are identical (``filters_uniform_mask``)."""
    n = side[0].shape[0]
    for s in range(4):
        _need(side[s], _F32, "head_fwd side"); _need(filt[s], _F32, "head_fwd filt")
        k = 4 << s
        if side[s].shape[3] != 16 or tuple(filt[s].shape) != (k, k, 16):
            raise ValueError("head_fwd: side/filter shape")
    _need(fuse_w, _F32, "head_fwd fuse_w"); _need(fuse_b, _F32, "head_fwd fuse_b")
    dev_t = side[0].device
    fused = torch.empty((n, 1, H, W), dtype=_F32, device=dev_t)
    outs = None
    so_ptrs = [None] * 4
    f1_ptrs = [None] * 4
    if with_side_out:
        outs = [torch.empty((n, 1, H, W), dtype=_F32, device=dev_t) for _ in range(4)]
        so_ptrs = [o.data_ptr() for o in outs]
        for s in range(4):
            _need(filt1[s], _F32, "head_fwd filt1")
        f1_ptrs = [f.data_ptr() for f in filt1]
        _need(dsn_w, _F32, "head_fwd dsn_w"); _need(dsn_b, _F32, "head_fwd dsn_b")
    _launch("head_fwd", side[0], ptr_array4([t.data_ptr() for t in side]), int_array4([t.shape[1] for t in side]),
            int_array4([t.shape[2] for t in side]), ptr_array4([t.data_ptr() for t in filt]), ptr_array4(f1_ptrs),
            _p(dsn_w) if with_side_out else None, _p(dsn_b) if with_side_out else None, fuse_w.data_ptr(), fuse_b.data_ptr(),
            fused.data_ptr(), ptr_array4(so_ptrs), n, H, W, int(filt_uniform) & 15, flops=2.0 * n * H * W * 256,
            nbytes=4 * (sum(t.numel() for t in side) + n * H * W * (5 if with_side_out else 1)))
    return fused, outs


def filters_uniform_mask(filt: Sequence[torch.Tensor]) -> int:
    """Bit s set where filt[s] ([k,k,16], the diagonal of upscale[s].weight) holds the SAME k x k filter in all 16 channels,
    element for element - the promise head_fwd / head_bwd's ``filt_uniform`` asks for.  One device sync: call it when the
    weights change, not per step (engine.PackedWeights caches it with the filters)."""
    mask = 0
    for s, f in enumerate(filt):
        if bool((f == f[..., :1]).all().item()):
            mask |= 1 << s
    return mask


def head_bwd(side: Sequence[torch.Tensor], filt: Sequence[torch.Tensor], filt1: Optional[Sequence[torch.Tensor]],
             dsn_w: Optional[torch.Tensor], fuse_w: torch.Tensor, d_fused: Optional[torch.Tensor],
             d_side_out: Optional[Sequence[torch.Tensor]], H: int, W: int, filt_uniform: int = 0):
    """Returns (d_side[4] bf16 NHWC [N,hs,ws,32], d_fuse_w[64], d_fuse_b[1], d_dsn_w[4,16]|None, d_dsn_b[4]|None)."""
    n = side[0].shape[0]
    dev_t = side[0].device
    with_so = d_side_out is not None
    if d_fused is not None:
        _need(d_fused, _F32, "head_bwd d_fused")
    d_side = [torch.empty((n, t.shape[1], t.shape[2], 32), dtype=_BF16, device=dev_t) for t in side]
    d_fuse_w = torch.empty((64,), dtype=_F32, device=dev_t)
    d_fuse_b = torch.empty((1,), dtype=_F32, device=dev_t)
    d_dsn_w = torch.empty((4, 16), dtype=_F32, device=dev_t) if with_so else None
    d_dsn_b = torch.empty((4,), dtype=_F32, device=dev_t) if with_so else None
    dso_ptrs = [None] * 4
    f1_ptrs = [None] * 4
    if with_so:
        for s in range(4):
            _need(d_side_out[s], _F32, "head_bwd d_side_out"); _need(filt1[s], _F32, "head_bwd filt1")
        dso_ptrs = [t.data_ptr() for t in d_side_out]
        f1_ptrs = [t.data_ptr() for t in filt1]
        _need(dsn_w, _F32, "head_bwd dsn_w")
    ws, wsn = _WS.get(lib().fosvos_head_bwd_workspace_bytes(n, H, W), dev_t)
    _launch("head_bwd", side[0], ptr_array4([t.data_ptr() for t in side]), int_array4([t.shape[1] for t in side]),
            int_array4([t.shape[2] for t in side]), ptr_array4([t.data_ptr() for t in filt]), ptr_array4(f1_ptrs),
            _p(dsn_w) if with_so else None, fuse_w.data_ptr(), _p(d_fused), ptr_array4(dso_ptrs),
            ptr_array4([t.data_ptr() for t in d_side]), d_fuse_w.data_ptr(), d_fuse_b.data_ptr(), _p(d_dsn_w), _p(d_dsn_b),
            n, H, W, int(filt_uniform) & 15, ws, wsn, flops=2.0 * n * H * W * 256,
            nbytes=4 * (sum(t.numel() for t in side) + n * H * W * (5 if with_so else 1)) + 2 * sum(t.numel() for t in d_side))
    return d_side, d_fuse_w, d_fuse_b, d_dsn_w, d_dsn_b


# ------------------------------------------------------------------------------------------ loss
def cbce_loss(logits: torch.Tensor, label: torch.Tensor, size_average: bool = True, grad_scale: float = 1.0,
              want_grad: bool = True, batch_counts: Optional[torch.Tensor] = None):
    """Returns (loss: 0-dim fp32 tensor on the device, grad like logits or None).  batch_counts: device float64 [2]
    {positives, pixels} of the whole (data-parallel) batch this tensor is a shard of; None = count this tensor."""
    _need(logits, _F32, "cbce_loss logits"); _need(label, _F32, "cbce_loss label")
    if batch_counts is not None:
        if (not batch_counts.is_cuda or batch_counts.dtype != torch.float64 or batch_counts.numel() != 2
                or not batch_counts.is_contiguous()):
            raise ValueError("cbce_loss: batch_counts must be a contiguous float64 [2] tensor on the GPU")
    if logits.shape != label.shape:
        raise ValueError(f"cbce_loss: logits {tuple(logits.shape)} vs label {tuple(label.shape)}")
    # the kernels read float4: a slice of a batch (one rank's shard, one frame) may start off a 16-byte boundary
    if logits.data_ptr() % 16:
        logits = logits.clone()
    if label.data_ptr() % 16:
        label = label.clone()
    L = lib()
    loss = torch.empty((), dtype=_F32, device=logits.device)
    grad = torch.empty_like(logits) if want_grad else None
    # the loss keeps its own small workspace: it must stay valid until the kernels ran, and the shared
    # grow-only buffer may be re-used by the next op on the same stream (which is ordered after us)
    ws, wsn = _WS.get(L.fosvos_cbce_workspace_bytes(logits.numel()), logits.device)
    head = (logits.data_ptr(), label.data_ptr(), logits.numel(), 1 if size_average else 0, float(grad_scale))
    tail = (loss.data_ptr(), _p(grad), ws, wsn)
    if batch_counts is None:
        _launch("cbce_loss", logits, *head, *tail, nbytes=logits.numel() * (16 if want_grad else 12))
    else:
        _launch("cbce_loss_batch_counts", logits, *head, batch_counts.data_ptr(), *tail, record="cbce_loss",
                nbytes=logits.numel() * (16 if want_grad else 12))
    return loss, grad


def _cbce_loss_frames_void(logits: torch.Tensor, label: torch.Tensor, void: torch.Tensor, size_average: bool, want_grad: bool,
                           grad_scale: float):
    """cbce_loss_frames with ignored pixels (fosvos_cbce_loss_frames_void)."""
    _need(void, torch.uint8, "cbce_loss_frames void")
    _same_device("cbce_loss_frames", logits, void)
    if void.shape != logits.shape:
        raise ValueError(f"cbce_loss_frames: logits {tuple(logits.shape)} vs void {tuple(void.shape)}")
    n = logits.shape[0]
    per = logits.numel() // n
    if n > 1 and (per % 4 or logits.data_ptr() % 16 or label.data_ptr() % 16 or void.data_ptr() % 4):
        parts = [_cbce_loss_frames_void(logits[i:i + 1], label[i:i + 1], void[i:i + 1], size_average, want_grad, grad_scale)
                 for i in range(n)]
        return torch.cat([p[0] for p in parts]), (torch.cat([p[1] for p in parts]) if want_grad else None)
    # one frame (or a slice of a batch) may start off the boundaries the kernels read at
    if logits.data_ptr() % 16:
        logits = logits.clone()
    if label.data_ptr() % 16:
        label = label.clone()
    if void.data_ptr() % 4:
        void = void.clone()
    L = lib()
    losses = torch.empty((n,), dtype=_F32, device=logits.device)
    grad = torch.empty_like(logits) if want_grad else None
    ws, wsn = _WS.get(L.fosvos_cbce_void_workspace_bytes(per, n), logits.device)
    _launch("cbce_loss_frames_void", logits, logits.data_ptr(), label.data_ptr(), void.data_ptr(), per, n,
            1 if size_average else 0, float(grad_scale), losses.data_ptr(), _p(grad), ws, wsn, record="cbce_loss_void",
            nbytes=logits.numel() * (18 if want_grad else 14))
    return losses, grad


def cbce_loss_frames(logits: torch.Tensor, label: torch.Tensor, size_average: bool = True, want_grad: bool = True,
                     grad_scale: float = 1.0, void: Optional[torch.Tensor] = None):
    """The loss of every frame of [N,1,H,W] logits on its own: ([N] losses, grad like logits or None), one set of launches.
    Frames whose element count is not a multiple of 4 go through one call per frame (16-byte alignment of the kernels).
    ``void`` (uint8 like logits, non-zero = ignored; None: the call is what it was): the classes are balanced over the valid
    pixels only, a void pixel's logit reaches nothing and its gradient is +0.0 (util/online_adapt.cbce_void)."""
    _need(logits, _F32, "cbce_loss_frames logits"); _need(label, _F32, "cbce_loss_frames label")
    if logits.shape != label.shape or logits.dim() < 2:
        raise ValueError(f"cbce_loss_frames: logits {tuple(logits.shape)} vs label {tuple(label.shape)}")
    if void is not None:
        return _cbce_loss_frames_void(logits, label, void, bool(size_average), bool(want_grad), float(grad_scale))
    n = logits.shape[0]
    per = logits.numel() // n
    if per % 4 or logits.data_ptr() % 16 or label.data_ptr() % 16:
        parts = [cbce_loss(logits[i:i + 1], label[i:i + 1], size_average=size_average, grad_scale=grad_scale,
                           want_grad=want_grad) for i in range(n)]
        return torch.stack([p[0] for p in parts]), (torch.cat([p[1] for p in parts]) if want_grad else None)
    L = lib()
    losses = torch.empty((n,), dtype=_F32, device=logits.device)
    grad = torch.empty_like(logits) if want_grad else None
    ws, wsn = _WS.get(n * L.fosvos_cbce_workspace_bytes(per), logits.device)
    _launch("cbce_loss_frames", logits, logits.data_ptr(), label.data_ptr(), per, n, 1 if size_average else 0, float(grad_scale),
            losses.data_ptr(), _p(grad), ws, wsn, record="cbce_loss", nbytes=logits.numel() * (16 if want_grad else 12))
    return losses, grad


CBCE_COUNT, CBCE_LOSS, CBCE_FINISH = 1, 2, 4
CBCE_MAX_MAPS = 8


def _map_tables(tensors):
    """HOST array of device pointers (a NULL entry for None), as the multi-map loss takes its logits and gradients."""
    return (ctypes.c_void_p * max(len(tensors), 1))(*[None if t is None else t.data_ptr() for t in tensors])


def _multi_args(logits, label: torch.Tensor, map_scale, who: str):
    """The checks the multi-map loss makes on the tensors themselves (the library checks counts, shapes and alignment)."""
    _need(label, _F32, f"{who} label")
    if label.dim() < 2:
        raise ValueError(f"{who}: label {tuple(label.shape)}")
    if len(map_scale) != len(logits):
        raise ValueError(f"{who}: {len(logits)} logit maps, {len(map_scale)} scales")
    for t in logits:
        _need(t, _F32, f"{who} logits")
        if t.device != label.device:
            raise ValueError(f"{who}: logits on {t.device}, label on {label.device}")
        if t.shape != label.shape:
            raise ValueError(f"{who}: logits {tuple(t.shape)} vs label {tuple(label.shape)}")


def cbce_multi_workspace_bytes(label: torch.Tensor, n_maps: int) -> int:
    """Bytes of workspace the multi-map loss of ``label`` ([N,1,H,W]) and ``n_maps`` logit maps needs."""
    n = label.shape[0]
    return lib().fosvos_cbce_multi_workspace_bytes(label.numel() // max(n, 1), n, int(n_maps))


def cbce_loss_frames_multi(logits: Sequence[torch.Tensor], label: torch.Tensor, map_scale: Sequence[float],
                           size_average: bool = True, want_grad: bool = True, workspace: Optional[torch.Tensor] = None):
    """The per-frame loss of M logit maps [N,1,H,W] that share the label batch ``label``: ([N,M] UNWEIGHTED losses, list of M
    gradients or None); map m's gradient comes out multiplied by ``map_scale[m]``.  One count and one loss launch for all
    maps (fosvos_cbce_loss_frames_multi); every value equals ``cbce_loss_frames(logits[m], label, grad_scale=map_scale[m])``
    bit for bit.  workspace: a uint8 tensor of cbce_multi_workspace_bytes to use instead of the ops' scratch."""
    logits = list(logits)
    _multi_args(logits, label, map_scale, "cbce_loss_frames_multi")
    m = len(logits)
    n = label.shape[0]
    per = label.numel() // n
    L = lib()
    losses = torch.empty((n, m), dtype=_F32, device=label.device)
    grads = [torch.empty_like(t) for t in logits] if want_grad else None
    if workspace is None:
        ws, wsn = _WS.get(L.fosvos_cbce_multi_workspace_bytes(per, n, m), label.device)
    else:
        _need(workspace, torch.uint8, "cbce_loss_frames_multi workspace")
        ws, wsn = workspace.data_ptr(), workspace.numel()
    _launch("cbce_loss_frames_multi", label, _map_tables(logits), label.data_ptr(), per, n, m, 1 if size_average else 0,
            (ctypes.c_float * max(m, 1))(*[float(v) for v in map_scale]), losses.data_ptr(),
            _map_tables(grads) if want_grad else None, ws, wsn, CBCE_COUNT | CBCE_LOSS | CBCE_FINISH, record="cbce_loss",
            nbytes=label.numel() * (8 + m * (8 if want_grad else 4)))
    return losses, grads


class CbceFramesMultiStaged(object):
    """``cbce_loss_frames_multi`` in its three launches, for a loop that has a forward pass to put behind the first and a
    backward pass behind the second: the class counts need only the labels, the backward pass only the gradients - counting
    beside the forward pass and writing the loss VALUES behind the backward pass takes two small dependent launches (and the
    copy of the values to the host) off the path between the two passes.

        staged = CbceFramesMultiStaged(label, n_maps)        # counts; before the forward pass
        losses, grads = staged.loss(logits, map_scale, ...)  # `losses` [N,M] is allocated, NOT yet written
        ...backward pass...
        staged.finish()                                      # now `losses` holds the values (stream order)

    Same stream for all three calls."""

    def __init__(self, label: torch.Tensor, n_maps: int):
        self.who = type(self).__name__
        _need(label, _F32, f"{self.who} label")
        if label.dim() < 2:
            raise ValueError(f"{self.who}: label {tuple(label.shape)}")
        self.n, self.m = label.shape[0], int(n_maps)
        self.per = label.numel() // self.n
        self.label = label
        # the stages share this workspace across the passes in between: its own tensor, not the ops' scratch
        self.wsn = lib().fosvos_cbce_multi_workspace_bytes(self.per, self.n, self.m)
        self.ws = torch.empty((max(self.wsn, 8),), dtype=torch.uint8, device=label.device)
        self.losses = None
        self.size_average = None
        t0 = _pb()
        self._launch(CBCE_COUNT, "count")
        _pe(t0, "cbce_loss", 0.0, label.numel() * 4)

    def _launch(self, parts: int, stage: str, logits=None, map_scale=None, grads=None):
        """One call of the C entry point for the stages ``parts``; the maps' arguments only with the loss stage."""
        dev, st = _ctx(self.label)
        check(lib().fosvos_cbce_loss_frames_multi(None if logits is None else _map_tables(logits), self.label.data_ptr(),
                                                  self.per, self.n, self.m, 1 if self.size_average else 0,
                                                  None if map_scale is None else (ctypes.c_float * self.m)(*map_scale),
                                                  _p(self.losses), None if grads is None else _map_tables(grads),
                                                  self.ws.data_ptr(), self.wsn, parts, dev, st),
              f"cbce_loss_frames_multi({stage})")

    def loss(self, logits: Sequence[torch.Tensor], map_scale: Sequence[float], size_average: bool = True,
             want_grad: bool = True):
        logits = list(logits)
        _multi_args(logits, self.label, map_scale, self.who)
        if len(logits) != self.m:
            raise ValueError(f"{self.who}: staged for {self.m} maps, got {len(logits)}")
        self.losses = torch.empty((self.n, self.m), dtype=_F32, device=self.label.device)
        self.size_average = bool(size_average)
        grads = [torch.empty_like(t) for t in logits] if want_grad else None
        t0 = _pb()
        self._launch(CBCE_LOSS, "loss", logits, [float(v) for v in map_scale], grads)
        _pe(t0, "cbce_loss", 0.0, self.label.numel() * (4 + self.m * (8 if want_grad else 4)))
        return self.losses, grads

    def finish(self) -> torch.Tensor:
        if self.losses is None:
            raise RuntimeError(f"{self.who}.finish before loss")
        self._launch(CBCE_FINISH, "finish")
        return self.losses


class CbceFramesStaged(CbceFramesMultiStaged):
    """``cbce_loss_frames`` in its three launches (fosvos_cbce_loss_frames_parts): CbceFramesMultiStaged for one logit
    tensor, with the arguments and results of cbce_loss_frames ([N] losses, one gradient tensor).

        staged = CbceFramesStaged(label)              # counts; before the forward pass
        losses, grad = staged.loss(logits, ...)       # `losses` is allocated, NOT yet written
        ...backward pass...
        staged.finish()                               # now `losses` holds the values (stream order)

    Frames whose element count is not a multiple of 4 are not supported here (the caller falls back to cbce_loss_frames)."""

    def __init__(self, label: torch.Tensor):
        if label.dim() >= 2 and ((label.numel() // label.shape[0]) % 4 or label.data_ptr() % 16):
            raise ValueError("CbceFramesStaged: frames must be a multiple of 4 elements and 16-byte aligned")
        super().__init__(label, 1)

    def _launch(self, parts: int, stage: str, logits=(None,), map_scale=(1.0,), grads=None):
        dev, st = _ctx(self.label)
        check(lib().fosvos_cbce_loss_frames_parts(_p(logits[0]), self.label.data_ptr(), self.per, self.n,
                                                  1 if self.size_average else 0, map_scale[0], _p(self.losses),
                                                  None if grads is None else grads[0].data_ptr(), self.ws.data_ptr(),
                                                  self.wsn, parts, dev, st), f"cbce_loss_frames_parts({stage})")

    def loss(self, logits: torch.Tensor, size_average: bool = True, want_grad: bool = True, grad_scale: float = 1.0):
        if logits.data_ptr() % 16:
            raise ValueError("CbceFramesStaged: logits must be 16-byte aligned")
        _, grads = super().loss([logits], [grad_scale], size_average=size_average, want_grad=want_grad)
        self.losses = self.losses.view(self.n)  # (the same memory: finish() writes it)
        return self.losses, grads[0] if want_grad else None


# ------------------------------------------------------------------------------------------ thin-channel ResNet path
def _bn_args(bn: Optional[Sequence], co: int, who: str) -> list:
    """The (weight, bias, running_mean, running_var, eps) of an eval-mode BatchNorm2d over ``co`` channels, or None, as the
    pack entries take it: four pointers and eps."""
    if bn is None:
        return [None] * 4 + [0.0]
    for t in bn[:4]:
        _need(t, _F32, f"{who} BatchNorm tensor")
        if t.numel() != co:
            raise ValueError(f"{who}: BatchNorm size != out channels")
    return [t.data_ptr() for t in bn[:4]] + [float(bn[4])]


def fold_conv_bn(w: torch.Tensor, conv_bias: Optional[torch.Tensor] = None, bn: Optional[Sequence] = None):
    """(w * s, bn_bias - mean * s [+ conv_bias * s]) with s = bn_weight / sqrt(var + eps): fp32 OIHW in and out."""
    _need(w, _F32, "fold_conv_bn weight")
    co, ci, k, k2 = w.shape
    if k != k2:
        raise ValueError("fold_conv_bn: square kernels only")
    out = torch.empty_like(w)
    bias = torch.empty((co,), dtype=_F32, device=w.device)
    bnp = _bn_args(bn, co, "fold_conv_bn")
    if conv_bias is not None:
        _need(conv_bias, _F32, "fold_conv_bn conv bias")
    _launch("fold_conv_bn", w, w.data_ptr(), co, ci, k, _p(conv_bias), *bnp, out.data_ptr(), bias.data_ptr(), record=False)
    return out, bias


def conv3x3_fwd_add(x: torch.Tensor, w_packed: torch.Tensor, bias: torch.Tensor, ci: int, co: int, relu: bool = True,
                    addend: Optional[torch.Tensor] = None, out_f32: bool = False) -> torch.Tensor:
    """MFMA conv3x3 in its residual form: act(conv(x) + bias + addend), ReLU after the add; bf16 NHWC in and out."""
    _need(x, _BF16, "conv3x3_fwd_add x"); _need(w_packed, _BF16, "conv3x3_fwd_add packed weight")
    _need(bias, _F32, "conv3x3_fwd_add bias")
    n, h, wd, cx = x.shape
    L = lib()
    if cx != ci or ci % 32 or (co % 64 and co != 32 and not (co == 16 and addend is None)):
        raise ValueError(f"conv3x3_fwd_add: x has {cx} channels for Ci={ci}, Co={co} (Ci % 32 == 0, Co = 32 or Co % 64 == 0)")
    if out_f32 and co != 16:
        raise ValueError("conv3x3_fwd_add: fp32 output is the 16-channel side_prep form")
    if w_packed.numel() != L.fosvos_packed_weight_elems(co, ci) or bias.numel() != co:
        raise ValueError("conv3x3_fwd_add: packed weight / bias size does not match (Co, Ci)")
    y = torch.empty((n, h, wd, co), dtype=_F32 if out_f32 else _BF16, device=x.device)
    if addend is not None:
        _need(addend, _BF16, "conv3x3_fwd_add addend")
        if addend.shape != y.shape:
            raise ValueError(f"conv3x3_fwd_add: addend {tuple(addend.shape)} vs output {tuple(y.shape)}")
    _launch("conv3x3_fwd_add", x, x.data_ptr(), w_packed.data_ptr(), bias.data_ptr(), _p(addend), y.data_ptr(), n, h, wd, ci, co,
            (CONV_RELU if relu else 0) | (CONV_OUT_F32 if out_f32 else 0), None, 0,   # (never splits K: no workspace)
            record=f"mfma3x3s1 {ci}->{co} @{h}x{wd}" if _PROF is not None and _PROF.detail else "mfma3x3s1",
            flops=2.0 * n * h * wd * 9 * ci * co,
            nbytes=2 * (x.numel() + y.numel()) + (2 * addend.numel() if addend is not None else 0))
    return y


def conv3x3_s2_fwd(x: torch.Tensor, w_packed: torch.Tensor, bias: torch.Tensor, ci: int, co: int,
                   relu: bool = True) -> torch.Tensor:
    """Stride-2 conv3x3 (pad 1) on the MFMA path: [N,H,W,ci] -> [N,(H-1)//2+1,(W-1)//2+1,co], bf16 NHWC."""
    _need(x, _BF16, "conv3x3_s2_fwd x"); _need(w_packed, _BF16, "conv3x3_s2_fwd packed weight")
    _need(bias, _F32, "conv3x3_s2_fwd bias")
    n, h, wd, cx = x.shape
    L = lib()
    if cx != ci or ci % 32 or (co % 64 and co != 32):
        raise ValueError(f"conv3x3_s2_fwd: x has {cx} channels for Ci={ci}, Co={co} (Ci % 32 == 0, Co = 32 or Co % 64 == 0)")
    if w_packed.numel() != L.fosvos_packed_weight_elems(co, ci) or bias.numel() != co:
        raise ValueError("conv3x3_s2_fwd: packed weight / bias size does not match (Co, Ci)")
    ho, wo = (h - 1) // 2 + 1, (wd - 1) // 2 + 1
    y = torch.empty((n, ho, wo, co), dtype=_BF16, device=x.device)
    _launch("conv3x3_s2_fwd", x, x.data_ptr(), w_packed.data_ptr(), bias.data_ptr(), y.data_ptr(), n, h, wd, ci, co,
            CONV_RELU if relu else 0, None, 0,   # (never splits K: no workspace)
            record=f"mfma3x3s2 {ci}->{co} @{ho}x{wo}" if _PROF is not None and _PROF.detail else "mfma3x3s2",
            flops=2.0 * n * ho * wo * 9 * ci * co, nbytes=2 * (x.numel() + y.numel()))
    return y


def conv_out_size(h: int, k: int, stride: int) -> int:
    return (h + 2 * (k // 2) - k) // stride + 1


def pack_conv2d_bn(w: torch.Tensor, conv_bias: Optional[torch.Tensor] = None, bn: Optional[Sequence] = None):
    """w: fp32 OIHW [Co,Ci,k,k] (k = 1 or 3); bn = (weight, bias, running_mean, running_var, eps) of the eval-mode
    BatchNorm2d that follows the conv, or None.  Returns (packed int32 words, folded fp32 bias)."""
    _need(w, _F32, "pack_conv2d_bn weight")
    co, ci, k, k2 = w.shape
    if k != k2:
        raise ValueError("pack_conv2d_bn: square kernels only")
    L = lib()
    packed = torch.empty((L.fosvos_conv2d_packed_dwords(co, ci, k),), dtype=torch.int32, device=w.device)
    bias = torch.empty((L.fosvos_conv2d_bias_elems(co),), dtype=_F32, device=w.device)
    bnp = _bn_args(bn, co, "pack_conv2d_bn")
    if conv_bias is not None:
        _need(conv_bias, _F32, "pack_conv2d_bn conv bias")
    _launch("pack_conv2d_bn", w, w.data_ptr(), co, ci, k, _p(conv_bias), *bnp, packed.data_ptr(), bias.data_ptr(), record=False)
    return packed, bias


def conv2d_plan(n: int, h: int, w: int, ci: int, co: int, k: int, stride: int = 1, fp32_math: bool = False) -> dict:
    """What fosvos_conv2d_fwd launches for this shape (host arithmetic only): {"cob", "threads", "slices", "workgroups"}.
    k = 7, stride = 2, ci = 3: what fosvos_conv7x7s2_first_fwd launches - with fp32_math (or more than 64 channels) the same
    keys for its vector-ALU form, else {"mfma_frag_blocks", "workgroups"} of the MFMA form."""
    from . import Conv2dPlanInfo
    info = Conv2dPlanInfo()
    check(lib().fosvos_conv2d_plan(n, h, w, ci, co, k, stride, ctypes.byref(info)), "conv2d_plan")
    if (k, stride, ci) == (7, 2, 3) and not fp32_math and info.mfma_frag_blocks:
        return {"mfma_frag_blocks": info.mfma_frag_blocks, "workgroups": info.mfma_workgroups}
    return {"cob": info.cob, "threads": info.threads, "slices": info.slices, "workgroups": info.workgroups}


def conv2d_fwd(x: torch.Tensor, packed: torch.Tensor, bias: torch.Tensor, ci: int, co: int, k: int, stride: int = 1,
               relu: bool = False, addend: Optional[torch.Tensor] = None, out_f32: bool = False) -> torch.Tensor:
    """x: bf16 NHWC [N,H,W,ru8(ci)] -> bf16 (or fp32) NHWC [N,Ho,Wo,ru8(co)] = act(conv + bias + addend)."""
    _need(x, _BF16, "conv2d_fwd x")
    _need(packed, torch.int32, "conv2d_fwd packed weights"); _need(bias, _F32, "conv2d_fwd bias")
    n, h, w, cp = x.shape
    L = lib()
    if cp != _ru(ci, 8):
        raise ValueError(f"conv2d_fwd: x has {cp} channels, expected {_ru(ci, 8)} (ci={ci} padded to 8)")
    if packed.numel() != L.fosvos_conv2d_packed_dwords(co, ci, k) or bias.numel() != L.fosvos_conv2d_bias_elems(co):
        raise ValueError("conv2d_fwd: packed image / bias size does not match (co, ci, k)")
    ho, wo = conv_out_size(h, k, stride), conv_out_size(w, k, stride)
    y = torch.empty((n, ho, wo, _ru(co, 8)), dtype=_F32 if out_f32 else _BF16, device=x.device)
    if addend is not None:
        _need(addend, _BF16, "conv2d_fwd addend")
        if addend.shape != y.shape:
            raise ValueError(f"conv2d_fwd: addend {tuple(addend.shape)} vs output {tuple(y.shape)}")
    flags = (CONV_RELU if relu else 0) | (CONV_OUT_F32 if out_f32 else 0)
    _launch("conv2d_fwd", x, x.data_ptr(), packed.data_ptr(), bias.data_ptr(), _p(addend), y.data_ptr(), n, h, w, ci, co, k, stride,
            flags, record=f"conv{k}x{k}s{stride}" + (f" {ci}->{co} @{ho}x{wo}" if _PROF is not None and _PROF.detail else ""),
            flops=2.0 * n * ho * wo * k * k * ci * co,
            nbytes=2 * x.numel() + y.numel() * y.element_size() + (2 * addend.numel() if addend is not None else 0))
    return y


def pack_conv7x7_bn(w: torch.Tensor, bn: Optional[Sequence] = None):
    _need(w, _F32, "pack_conv7x7_bn weight")
    co, ci, k, k2 = w.shape
    if (ci, k, k2) != (3, 7, 7):
        raise ValueError(f"pack_conv7x7_bn: expected [Co,3,7,7], got {tuple(w.shape)}")
    L = lib()
    packed = torch.empty((L.fosvos_conv7x7_packed_elems(co),), dtype=_F32, device=w.device)
    bias = torch.empty((L.fosvos_conv2d_bias_elems(co),), dtype=_F32, device=w.device)
    bnp = _bn_args(bn, co, "pack_conv7x7_bn")
    _launch("pack_conv7x7_bn", w, w.data_ptr(), co, *bnp, packed.data_ptr(), bias.data_ptr(), record=False)
    return packed, bias


CONV_FP32_MATH = 4


def conv7x7s2_first_fwd(frame: torch.Tensor, packed: torch.Tensor, bias: torch.Tensor, co: int,
                        relu: bool = True, fp32_math: bool = False) -> torch.Tensor:
    """frame: fp32 NCHW [N,3,H,W] -> bf16 NHWC [N,(H-1)//2+1,(W-1)//2+1,ru8(co)].  Default: bf16 MFMA (frame and
    weights rounded to bf16, fp32 accumulate); fp32_math keeps both fp32 on the vector ALU."""
    _need(frame, _F32, "conv7x7s2_first_fwd frame")
    _need(packed, _F32, "conv7x7s2_first_fwd packed weights"); _need(bias, _F32, "conv7x7s2_first_fwd bias")
    n, c, h, w = frame.shape
    L = lib()
    if c != 3:
        raise ValueError("conv7x7s2_first_fwd: 3-channel frames only")
    if packed.numel() != L.fosvos_conv7x7_packed_elems(co) or bias.numel() != L.fosvos_conv2d_bias_elems(co):
        raise ValueError("conv7x7s2_first_fwd: packed image / bias size does not match co")
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    y = torch.empty((n, ho, wo, _ru(co, 8)), dtype=_BF16, device=frame.device)
    _launch("conv7x7s2_first_fwd", frame, frame.data_ptr(), packed.data_ptr(), bias.data_ptr(), y.data_ptr(), n, h, w, co,
            (CONV_RELU if relu else 0) | (CONV_FP32_MATH if fp32_math else 0), record="conv7x7s2_first",
            flops=2.0 * n * ho * wo * 147 * co, nbytes=4 * frame.numel() + 2 * y.numel())
    return y


def conv7x7s2_pool_first_fwd(frame: torch.Tensor, packed: torch.Tensor, bias: torch.Tensor, co: int) -> torch.Tensor:
    """layer_base in one launch (bf16 MFMA form): conv 7x7/2 + folded BatchNorm + ReLU + MaxPool2d(3, 2, 1);
    frame fp32 NCHW [N,3,H,W] -> bf16 NHWC [N,Hp,Wp,ru8(co)]."""
    _need(frame, _F32, "conv7x7s2_pool_first_fwd frame")
    _need(packed, _F32, "conv7x7s2_pool_first_fwd packed weights"); _need(bias, _F32, "conv7x7s2_pool_first_fwd bias")
    n, c, h, w = frame.shape
    L = lib()
    if c != 3:
        raise ValueError("conv7x7s2_pool_first_fwd: 3-channel frames only")
    if packed.numel() != L.fosvos_conv7x7_packed_elems(co) or bias.numel() != L.fosvos_conv2d_bias_elems(co):
        raise ValueError("conv7x7s2_pool_first_fwd: packed image / bias size does not match co")
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    hp, wp = (ho - 1) // 2 + 1, (wo - 1) // 2 + 1
    y = torch.empty((n, hp, wp, _ru(co, 8)), dtype=_BF16, device=frame.device)
    _launch("conv7x7s2_pool_first_fwd", frame, frame.data_ptr(), packed.data_ptr(), bias.data_ptr(), y.data_ptr(), n, h, w, co,
            record="conv7x7s2_pool_first", flops=2.0 * n * ho * wo * 147 * co, nbytes=4 * frame.numel() + 2 * y.numel())
    return y


def maxpool3x3s2_fwd(x: torch.Tensor) -> torch.Tensor:
    _need(x, _BF16, "maxpool3x3s2_fwd")
    n, h, w, c = x.shape
    y = torch.empty((n, (h - 1) // 2 + 1, (w - 1) // 2 + 1, c), dtype=_BF16, device=x.device)
    _launch("maxpool3x3s2_fwd", x, x.data_ptr(), y.data_ptr(), n, h, w, c, record="maxpool3x3s2", nbytes=2 * (x.numel() + y.numel()))
    return y


def deconv_head_fwd(side: Sequence[torch.Tensor], strides: Sequence[int], filt: Sequence[torch.Tensor],
                    filt1: Optional[Sequence[torch.Tensor]], dsn_w: Optional[torch.Tensor],
                    dsn_b: Optional[torch.Tensor], fuse_b: torch.Tensor, H: int, W: int, with_side_out: bool = True):
    """side[s]: fp32 NHWC [N,hs,ws,16]; filt[s]: [2f,2f,16] (upscale filter contracted with the fuse weights);
    filt1[s]: [2f,2f]; dsn_w [4,16]; dsn_b [4]; fuse_b [1].  Returns (fused [N,1,H,W], [4 side outputs] or None)."""
    n = side[0].shape[0]
    for s in range(4):
        _need(side[s], _F32, "deconv_head_fwd side"); _need(filt[s], _F32, "deconv_head_fwd filt")
        k = 2 * int(strides[s])
        if side[s].shape[3] != 16 or tuple(filt[s].shape) != (k, k, 16):
            raise ValueError("deconv_head_fwd: side/filter shape")
    _need(fuse_b, _F32, "deconv_head_fwd fuse_b")
    dev_t = side[0].device
    fused = torch.empty((n, 1, H, W), dtype=_F32, device=dev_t)
    outs = None
    so_ptrs = [None] * 4
    f1_ptrs = [None] * 4
    if with_side_out:
        outs = [torch.empty((n, 1, H, W), dtype=_F32, device=dev_t) for _ in range(4)]
        so_ptrs = [o.data_ptr() for o in outs]
        for s in range(4):
            _need(filt1[s], _F32, "deconv_head_fwd filt1")
            if tuple(filt1[s].shape) != (2 * int(strides[s]),) * 2:
                raise ValueError("deconv_head_fwd: filt1 shape")
        f1_ptrs = [f.data_ptr() for f in filt1]
        _need(dsn_w, _F32, "deconv_head_fwd dsn_w"); _need(dsn_b, _F32, "deconv_head_fwd dsn_b")
    _launch("deconv_head_fwd", side[0], ptr_array4([t.data_ptr() for t in side]), int_array4([t.shape[1] for t in side]),
            int_array4([t.shape[2] for t in side]), int_array4([int(f) for f in strides]),
            ptr_array4([t.data_ptr() for t in filt]), ptr_array4(f1_ptrs), _p(dsn_w) if with_side_out else None,
            _p(dsn_b) if with_side_out else None, fuse_b.data_ptr(), fused.data_ptr(), ptr_array4(so_ptrs), n, H, W,
            flops=2.0 * n * H * W * 256, nbytes=4 * (sum(t.numel() for t in side) + n * H * W * (5 if with_side_out else 1)))
    return fused, outs


# ------------------------------------------------------------------------------------------ training-sample augmentation
_AUG_TABLES = (("col_taps", torch.int32, 1), ("col_w", _F32, 1), ("row_taps", torch.int32, 0), ("row_w", _F32, 0),
               ("col_near", torch.int32, 1), ("row_near", torch.int32, 0))


def augment_sample(frame: torch.Tensor, mask: torch.Tensor, flip: bool, img_lut: torch.Tensor, gt_lut: torch.Tensor,
                   image: torch.Tensor, gt: torch.Tensor, tables: Optional[Sequence[torch.Tensor]] = None) -> None:
    """fosvos_augment_sample: uint8 frame [H,W,3] and mask [H,W] -> image [1,3,OH,OW] / gt [1,1,OH,OW] (fp32, written in
    place), mirrored first if ``flip``.  ``tables`` = (col_taps [OW,4] int32, col_w [OW,4] fp32, row_taps [OH,4] int32,
    row_w [OH,4] fp32, col_near [OW] int32, row_near [OH] int32) from custom_transforms.resize_plan, or None for the
    size-keeping copy.  img_lut fp32 [256,3], gt_lut fp32 [256]."""
    _need(frame, torch.uint8, "augment_sample frame")
    _need(mask, torch.uint8, "augment_sample mask")
    _need(img_lut, _F32, "augment_sample img_lut")
    _need(gt_lut, _F32, "augment_sample gt_lut")
    _need(image, _F32, "augment_sample image")
    _need(gt, _F32, "augment_sample gt")
    if frame.dim() != 3 or frame.shape[2] != 3:
        raise ValueError(f"augment_sample: frame must be [H,W,3], got {tuple(frame.shape)}")
    h, w = int(frame.shape[0]), int(frame.shape[1])
    if tuple(mask.shape) != (h, w):
        raise ValueError(f"augment_sample: mask {tuple(mask.shape)} does not match the frame's {(h, w)}")
    if tuple(img_lut.shape) != (256, 3) or tuple(gt_lut.shape) != (256,):
        raise ValueError("augment_sample: img_lut must be [256,3] and gt_lut [256]")
    if image.dim() != 4 or tuple(image.shape[:2]) != (1, 3):
        raise ValueError(f"augment_sample: image must be [1,3,OH,OW], got {tuple(image.shape)}")
    oh, ow = int(image.shape[2]), int(image.shape[3])
    if tuple(gt.shape) != (1, 1, oh, ow):
        raise ValueError(f"augment_sample: gt must be [1,1,{oh},{ow}], got {tuple(gt.shape)}")
    ptrs = [None] * 6
    if tables is not None:
        if len(tables) != 6:
            raise ValueError("augment_sample: six tables (col_taps, col_w, row_taps, row_w, col_near, row_near)")
        for k, (t, (name, dtype, is_col)) in enumerate(zip(tables, _AUG_TABLES)):
            _need(t, dtype, "augment_sample " + name)
            n = ow if is_col else oh
            want = (n, 4) if name.endswith(("taps", "_w")) else (n,)
            if tuple(t.shape) != want:
                raise ValueError(f"augment_sample: {name} must be {want}, got {tuple(t.shape)}")
            ptrs[k] = t.data_ptr()
    elif (oh, ow) != (h, w):
        raise ValueError(f"augment_sample: without tables the size is kept ({h}x{w}), got {oh}x{ow}")
    for t in (mask, img_lut, gt_lut, image, gt) + tuple(tables or ()):
        if t.device != frame.device:
            raise RuntimeError(f"augment_sample: every tensor must be on {frame.device}, got one on {t.device}")
    _launch("augment_sample", frame, frame.data_ptr(), mask.data_ptr(), h, w, 1 if flip else 0, *ptrs, oh, ow, img_lut.data_ptr(),
            gt_lut.data_ptr(), image.data_ptr(), gt.data_ptr(),
            nbytes=float(frame.numel() + mask.numel() + 4 * (image.numel() + gt.numel())))


def warp_workspace_bytes(h: int, w: int) -> int:
    """fosvos_warp_workspace_bytes: what ``warp_sample(renormalize=True)`` needs for an h x w frame."""
    limits.check_int("warp_workspace_bytes", "h", h, 1, limits.MAX_FRAME_SIDE)
    limits.check_int("warp_workspace_bytes", "w", w, 1, limits.MAX_FRAME_SIDE)
    return int(lib().fosvos_warp_workspace_bytes(h, w))


def warp_sample(frame: torch.Tensor, mask: torch.Tensor, flip: bool, matrix, img_lut: torch.Tensor, gt_lut: torch.Tensor,
                image: torch.Tensor, gt: torch.Tensor, renormalize: bool = False,
                workspace: Optional[torch.Tensor] = None) -> None:
    """fosvos_warp_sample: uint8 frame [H,W,3] and mask [H,W] -> image [1,3,H,W] / gt [1,1,H,W] (fp32, written in place),
    mirrored first if ``flip`` and then warped by ``matrix``, the 2x3 SOURCE -> DESTINATION matrix of
    custom_transforms.rotation_matrix, bit for bit custom_transforms.warp_affine.  The matrix is inverted here exactly as
    warp_affine inverts it (np.linalg.inv of the 3x3 in fp64), so kernel and definition start from the same six doubles.
    img_lut fp32 [256,3], gt_lut fp32 [256].

    renormalize: the reference's ScaleNRotate shifts the warped frame to min 0 and divides it by its max where that exceeds 1
    (custom_transforms.ScaleNRotate(renormalize=True)); it needs ``workspace``, a uint8 tensor of at least
    ``warp_workspace_bytes(H, W)`` bytes.  On a mask the renormalisation is a no-op, because its values are in [0, 1]: the
    gt is never rewritten."""
    _need(frame, torch.uint8, "warp_sample frame")
    _need(mask, torch.uint8, "warp_sample mask")
    _need(img_lut, _F32, "warp_sample img_lut")
    _need(gt_lut, _F32, "warp_sample gt_lut")
    _need(image, _F32, "warp_sample image")
    _need(gt, _F32, "warp_sample gt")
    if frame.dim() != 3 or frame.shape[2] != 3:
        raise ValueError(f"warp_sample: frame must be [H,W,3], got {tuple(frame.shape)}")
    h, w = int(frame.shape[0]), int(frame.shape[1])
    limits.check_int("warp_sample", "H", h, 1, limits.MAX_FRAME_SIDE)
    limits.check_int("warp_sample", "W", w, 1, limits.MAX_FRAME_SIDE)
    if tuple(mask.shape) != (h, w):
        raise ValueError(f"warp_sample: mask {tuple(mask.shape)} does not match the frame's {(h, w)}")
    if tuple(img_lut.shape) != (256, 3) or tuple(gt_lut.shape) != (256,):
        raise ValueError("warp_sample: img_lut must be [256,3] and gt_lut [256]")
    if tuple(image.shape) != (1, 3, h, w):
        raise ValueError(f"warp_sample: a warp keeps the size: image must be [1,3,{h},{w}], got {tuple(image.shape)}")
    if tuple(gt.shape) != (1, 1, h, w):
        raise ValueError(f"warp_sample: gt must be [1,1,{h},{w}], got {tuple(gt.shape)}")
    inv = _inverse_2x3("warp_sample", "matrix", matrix)
    if not isinstance(renormalize, bool):
        raise ValueError(f"warp_sample: renormalize must be a bool, got {renormalize!r}")
    ws_ptr, ws_bytes = None, 0
    if renormalize:
        need = warp_workspace_bytes(h, w)
        if workspace is None:
            raise ValueError(f"warp_sample: renormalize needs a workspace of {need} bytes (warp_workspace_bytes)")
        _need(workspace, torch.uint8, "warp_sample workspace")
        if workspace.numel() < need:
            raise ValueError(f"warp_sample: workspace of {workspace.numel()} bytes, {need} needed (warp_workspace_bytes)")
        if workspace.data_ptr() % 4:
            raise ValueError("warp_sample: the workspace must be 4-byte aligned")
        ws_ptr, ws_bytes = workspace.data_ptr(), workspace.numel()
    _same_device("warp_sample", frame, mask, img_lut, gt_lut, image, gt, *(() if workspace is None else (workspace,)))
    _launch("warp_sample", frame, frame.data_ptr(), mask.data_ptr(), h, w, 1 if flip else 0,
            *inv, img_lut.data_ptr(), gt_lut.data_ptr(), image.data_ptr(), gt.data_ptr(),
            1 if renormalize else 0, ws_ptr, ws_bytes,
            nbytes=float(49 * h * w + 4 * (image.numel() + gt.numel()) + (8 * image.numel() if renormalize else 0)))


def _inverse_2x3(what: str, name: str, matrix) -> Tuple[float, ...]:
    """The six doubles of destination -> source of a 2x3 SOURCE -> DESTINATION ``matrix``, inverted exactly as
    custom_transforms.warp_affine inverts it (np.linalg.inv of the 3x3 in fp64)."""
    import numpy as np
    try:
        m = np.array(matrix, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: {name} must be 2x3 numbers, got {matrix!r}") from None
    if m.shape != (2, 3):
        raise ValueError(f"{what}: {name} must be 2x3 (source -> destination), got shape {m.shape}")
    if not np.isfinite(m).all():
        raise ValueError(f"{what}: {name} must be finite, got {m.tolist()}")
    try:
        inv = np.linalg.inv(np.vstack([m, [0.0, 0.0, 1.0]]))  # warp_affine's own inversion
    except np.linalg.LinAlgError:
        raise ValueError(f"{what}: {name} is singular: {m.tolist()}") from None
    if not np.isfinite(inv).all():
        raise ValueError(f"{what}: the inverse of the {name} is not finite: {m.tolist()}")
    return tuple(float(v) for v in inv[:2].reshape(-1))


def lucid_sample(frame: torch.Tensor, background: torch.Tensor, mask: torch.Tensor, flip: bool, matrix_bg, matrix_fg, gain,
                 bias, img_lut: torch.Tensor, gt_lut: torch.Tensor, image: torch.Tensor, gt: torch.Tensor) -> None:
    """fosvos_lucid_sample: uint8 frame, background [H,W,3] (the frame with the object painted out) and mask [H,W] -> image
    [1,3,H,W] / gt [1,1,H,W] (fp32, written in place): the object under ``matrix_fg`` composed over the background under
    ``matrix_bg`` (2x3, SOURCE -> DESTINATION, inverted here as warp_sample inverts its matrix), then ``* gain[c] + bias[c]``;
    bit for bit dataloaders/lucid.compose.  ``matrix_fg=None`` is no object: the warped background alone and gt = 0.
    ``gain`` / ``bias``: three finite numbers each, taken as float32.  img_lut fp32 [256,3], gt_lut fp32 [256].  One launch."""
    import numpy as np
    what = "lucid_sample"
    _need(frame, torch.uint8, "lucid_sample frame")
    _need(background, torch.uint8, "lucid_sample background")
    _need(mask, torch.uint8, "lucid_sample mask")
    _need(img_lut, _F32, "lucid_sample img_lut")
    _need(gt_lut, _F32, "lucid_sample gt_lut")
    _need(image, _F32, "lucid_sample image")
    _need(gt, _F32, "lucid_sample gt")
    if frame.dim() != 3 or frame.shape[2] != 3:
        raise ValueError(f"{what}: frame must be [H,W,3], got {tuple(frame.shape)}")
    h, w = int(frame.shape[0]), int(frame.shape[1])
    limits.check_int(what, "H", h, 1, limits.MAX_FRAME_SIDE)
    limits.check_int(what, "W", w, 1, limits.MAX_FRAME_SIDE)
    if tuple(background.shape) != (h, w, 3):
        raise ValueError(f"{what}: background {tuple(background.shape)} does not match the frame's {(h, w, 3)}")
    if tuple(mask.shape) != (h, w):
        raise ValueError(f"{what}: mask {tuple(mask.shape)} does not match the frame's {(h, w)}")
    if tuple(img_lut.shape) != (256, 3) or tuple(gt_lut.shape) != (256,):
        raise ValueError(f"{what}: img_lut must be [256,3] and gt_lut [256]")
    if tuple(image.shape) != (1, 3, h, w):
        raise ValueError(f"{what}: the composition keeps the size: image must be [1,3,{h},{w}], got {tuple(image.shape)}")
    if tuple(gt.shape) != (1, 1, h, w):
        raise ValueError(f"{what}: gt must be [1,1,{h},{w}], got {tuple(gt.shape)}")
    inv_bg = _inverse_2x3(what, "matrix_bg", matrix_bg)
    inv_fg = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0) if matrix_fg is None else _inverse_2x3(what, "matrix_fg", matrix_fg)
    scalars = []
    for name, v in (("gain", gain), ("bias", bias)):
        try:
            a = np.array(v, dtype=np.float64)
        except (TypeError, ValueError):
            a = None
        if a is None or a.shape != (3,) or not (np.abs(a) <= np.finfo(np.float32).max).all():  # (a NaN compares False)
            raise ValueError(f"{what}: {name} must be three finite float32 numbers, got {v!r}")
        scalars += [float(x) for x in a.astype(np.float32)]
    _same_device(what, frame, background, mask, img_lut, gt_lut, image, gt)
    _launch(what, frame, frame.data_ptr(), background.data_ptr(), mask.data_ptr(), h, w, 1 if flip else 0, *inv_bg, *inv_fg,
            0 if matrix_fg is None else 1, *scalars, img_lut.data_ptr(), gt_lut.data_ptr(), image.data_ptr(), gt.data_ptr(),
            nbytes=float(49 * h * w + 4 * (image.numel() + gt.numel())))


# ------------------------------------------------------------------------------------------ shared argument checks
# (of the ops from here down: a wrong dtype is a ValueError; DESIGN.md section 21 lists who uses which)
MAX_OBJECTS = limits.MAX_OBJECTS
MAX_FRAME_SIDE = limits.MAX_FRAME_SIDE  # of a scaled call (util/frame_resample.MAX_SIDE)
_PALETTES = {}  # device -> the default palette (util/object_merge.davis_palette) on it


def _same_device(what: str, first, *others: torch.Tensor) -> None:
    """``first``: a tensor, or the device itself."""
    device = first.device if isinstance(first, torch.Tensor) else first
    for t in others:
        if t.device != device:
            raise RuntimeError(f"{what}: every tensor must be on {device}, got one on {t.device}")


def _out_like(out: Optional[torch.Tensor], shape, dtype, like, what: str, name: str = "out") -> torch.Tensor:
    """The output buffer ``name``: a new one on ``like``'s device (``like``: a tensor, or the device itself), or the
    caller's where it is a contiguous ``dtype`` tensor of ``shape`` on that device."""
    if out is None:
        return torch.empty(shape, dtype=dtype, device=like.device if isinstance(like, torch.Tensor) else like)
    _need(out, dtype, f"{what} {name}", ValueError)
    if tuple(out.shape) != tuple(shape):
        raise ValueError(f"{what}: {name} must be {tuple(shape)}, got {tuple(out.shape)}")
    _same_device(what, like, out)
    return out


def _file_buffers(out: Optional[torch.Tensor], lengths: Optional[torch.Tensor], n: int, cap: int, like: torch.Tensor,
                  what: str) -> Tuple[torch.Tensor, torch.Tensor]:
    """What a file encoder writes into: ``out`` uint8 [n, >= cap] and ``lengths`` int32 [n] on ``like``'s device."""
    if out is None:
        out = torch.empty((n, cap), dtype=torch.uint8, device=like.device)
    else:
        _need(out, torch.uint8, f"{what} out", ValueError)
        if out.dim() != 2 or out.shape[0] != n or out.shape[1] < cap:
            raise ValueError(f"{what}: out must be [{n}, >= {cap}], got {tuple(out.shape)}")
        _same_device(what, like, out)
    return out, _out_like(lengths, (n,), torch.int32, like, what, "lengths")


def _logit_shape(logits: torch.Tensor, what: str) -> Tuple[int, int, int]:
    if logits.dim() != 4 or logits.shape[1] != 1 or logits.numel() == 0:
        raise ValueError(f"{what}: logits must be a non-empty [N,1,H,W], got {tuple(logits.shape)}")
    return int(logits.shape[0]), int(logits.shape[2]), int(logits.shape[3])


def _map_shape(t: torch.Tensor, what: str, name: str) -> Tuple[int, int, int]:
    """(N, H, W) of ``t`` where it is a non-empty uint8 [N,H,W] map on the GPU."""
    _need(t, torch.uint8, f"{what} {name}", ValueError)
    if t.dim() != 3 or t.numel() == 0:
        raise ValueError(f"{what}: {name} must be a non-empty [N,H,W], got {tuple(t.shape)}")
    return int(t.shape[0]), int(t.shape[1]), int(t.shape[2])


def _logit_table(logits: Sequence[torch.Tensor], what: str, shape=None):
    """The K logit maps of several objects: (the maps as a list, their shape (N,1,H,W), the HOST array of their K device
    pointers).  Every map is checked against ``shape``, or - None - the first against ``_logit_shape`` and the rest against it."""
    logits = list(logits)
    k = len(logits)
    if not 1 <= k <= MAX_OBJECTS:
        raise ValueError(f"{what}: {k} logit maps, outside [1, {MAX_OBJECTS}]")
    for t in logits:
        _need(t, _F32, f"{what} logits", ValueError)
    if shape is None:
        n, h, w = _logit_shape(logits[0], what)
        shape = (n, 1, h, w)
    for t in logits:
        if tuple(t.shape) != shape:
            raise ValueError(f"{what}: every logit map must be {shape}, got {tuple(t.shape)}")
    return logits, shape, (ctypes.c_void_p * k)(*[t.data_ptr() for t in logits])


def default_palette(device) -> torch.Tensor:
    """``object_merge.davis_palette()`` as a uint8 [256,3] tensor on ``device``, uploaded once per device."""
    device = torch.device(device)
    if device.type != 'cuda':
        raise RuntimeError(f"default_palette: a GPU device, got {device} (the HIP path has no CPU fallback)")
    key = device.index if device.index is not None else torch.cuda.current_device()
    pal = _PALETTES.get(key)
    if pal is None:
        from util.object_merge import davis_palette
        pal = _PALETTES[key] = torch.from_numpy(davis_palette()).to(device)
    return pal


def _palette(palette: Optional[torch.Tensor], device: torch.device, what: str) -> torch.Tensor:
    """``palette`` where it is a uint8 [256,3] tensor on ``device``; None: the default one."""
    if palette is None:
        return default_palette(device)
    _need(palette, torch.uint8, f"{what} palette", ValueError)
    if tuple(palette.shape) != (256, 3):
        raise ValueError(f"{what}: palette must be (256, 3), got {tuple(palette.shape)}")
    _same_device(what, device, palette)
    return palette


def _jf_radius(radius: Optional[int], h: int, w: int, what: str) -> int:
    return limits.check_int(what, "radius", jf_default_radius(h, w) if radius is None else int(radius), *limits.JF_RADIUS)


# ------------------------------------------------------------------------------------------ scoring (eval.hip)
def prob_bytes(logits: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fosvos_prob_bytes: logits fp32 [N,1,H,W] -> uint8 [N,H,W], per frame ``bytescale(sigmoid(logits))`` of
    util/experiment_helper.py evaluated in fp64 (the bytes of the probability PNG).  Launched on the current stream, no
    synchronisation."""
    _need(logits, _F32, "prob_bytes logits", ValueError)
    n, h, w = _logit_shape(logits, "prob_bytes")
    out = _out_like(out, (n, h, w), torch.uint8, logits, "prob_bytes")
    ws, _ = _WS.get(8 * n, logits.device)
    _launch("prob_bytes", logits, logits.data_ptr(), n, h, w, ws, out.data_ptr(), nbytes=9.0 * n * h * w)
    return out


def jf_default_radius(h: int, w: int) -> int:
    """ceil(0.008 * diagonal), the DAVIS boundary tolerance (util/davis_measures.default_radius)."""
    return int(math.ceil(0.008 * math.sqrt(h * h + w * w)))


def jf_counts(logits: torch.Tensor, gt: torch.Tensor, radius: Optional[int] = None,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fosvos_jf_counts: logits fp32 [N,1,H,W] and gt uint8 [N,H,W] (non-zero = object) -> int32 [N,6] per frame: inter,
    union, n_pred_b, n_gt_b, match_pred, match_gt of the mask ``logits >= 0`` against ``gt`` (util/davis_measures.py states
    the definitions).  ``radius`` (1..63) defaults to ceil(0.008 * diagonal).  ``out`` may be any [N,6] int32 rows, e.g. a
    slice of a sequence's counter tensor; the op zeroes them itself.  Launched on the current stream, no synchronisation."""
    _need(logits, _F32, "jf_counts logits", ValueError)
    _need(gt, torch.uint8, "jf_counts gt", ValueError)
    n, h, w = _logit_shape(logits, "jf_counts")
    if tuple(gt.shape) != (n, h, w):
        raise ValueError(f"jf_counts: gt must be {(n, h, w)}, got {tuple(gt.shape)}")
    radius = _jf_radius(radius, h, w, "jf_counts")
    out = _out_like(out, (n, 6), torch.int32, logits, "jf_counts")
    _same_device("jf_counts", logits, gt)
    ws, wsn = _WS.get(lib().fosvos_jf_workspace_bytes(n, h, w), logits.device)
    _launch("jf_counts", logits, logits.data_ptr(), gt.data_ptr(), n, h, w, radius, out.data_ptr(), ws, wsn, nbytes=5.0 * n * h * w)
    return out


# ------------------------------------------------------------------------------------------ mask cleaning (components.hip)
def _components_shape(logits: torch.Tensor, what: str) -> Tuple[int, int, int]:
    _need(logits, _F32, f"{what} logits", ValueError)
    n, h, w = _logit_shape(logits, what)
    if h * w >= 1 << 31 or n > 65535:
        raise ValueError(f"{what}: N={n} (<= 65535) H={h} W={w} (H W < 2^31)")
    return n, h, w


def component_roots(logits: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fosvos_component_roots: logits fp32 [N,1,H,W] -> int32 [N,H,W]: -1 where ``logits >= 0`` does not hold, else the
    smallest raster index ``y * W + x`` of the pixel's 8-connected component (util/mask_components.component_roots).
    Launched on the current stream, no synchronisation."""
    n, h, w = _components_shape(logits, "component_roots")
    out = _out_like(out, (n, h, w), torch.int32, logits, "component_roots")
    _launch("component_roots", logits, logits.data_ptr(), n, h, w, out.data_ptr(), None, 0, nbytes=8.0 * n * h * w)
    return out


def clean_components(logits: torch.Tensor, seed: Optional[torch.Tensor] = None, radius: int = 0, min_area: int = 0,
                     largest: bool = False, chain: bool = False, fill: float = -100.0, out: Optional[torch.Tensor] = None,
                     kept: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fosvos_clean_components: logits fp32 [N,1,H,W] -> fp32 [N,1,H,W] with every foreground pixel (``logits >= 0``) of a
    component that is not kept set to ``fill`` (finite, < 0) and every other value passed bit for bit
    (util/mask_components.clean_sequence states the rules).  A component stays when its area is >= ``min_area`` and, with a
    non-empty seed, it has a pixel within ``radius`` (0..63) of it; ``largest`` keeps only the largest of those.  ``seed``:
    uint8 [N,H,W], a non-zero byte is a set pixel; with ``chain`` uint8 [1,H,W] or None for frame 0, and frame n is gated by
    what frame n - 1 kept.  ``out`` may be ``logits`` itself; ``kept`` (uint8 [N,H,W]) receives 1 on kept pixels.  Launched
    on the current stream, no synchronisation."""
    n, h, w = _components_shape(logits, "clean_components")
    limits.check_int("clean_components", "radius", radius, 0, limits.CLEAN_MAX_RADIUS)
    limits.check_int("clean_components", "min_area", min_area, 0, limits.CLEAN_MAX_AREA)
    fill = limits.check_real("clean_components", "fill", float(fill), *limits.FILL_RANGE, hi_open=True,
                             expect="finite and negative")  # finite as a float32 too
    if seed is not None:
        _need(seed, torch.uint8, "clean_components seed", ValueError)
        want = (1, h, w) if chain else (n, h, w)
        if tuple(seed.shape) != want:
            raise ValueError(f"clean_components: seed must be {want}{' with chain' if chain else ''}, got {tuple(seed.shape)}")
        _same_device("clean_components", logits, seed)
    out = _out_like(out, (n, 1, h, w), _F32, logits, "clean_components")
    if kept is not None:
        _out_like(kept, (n, h, w), torch.uint8, logits, "clean_components", "kept")
    ws, wsn = _WS.get(lib().fosvos_components_workspace_bytes(n, h, w), logits.device)
    _launch("clean_components", logits, logits.data_ptr(), _p(seed), n, h, w, radius, min_area, int(bool(largest)),
            int(bool(chain)), fill, out.data_ptr(), _p(kept), ws, wsn, nbytes=25.0 * n * h * w)
    return out


# ------------------------------------------------------------------------------------------ online adaptation (adapt.hip)
GATE_MAX_DISTANCE = limits.GATE_MAX_DISTANCE  # util/online_adapt.MAX_DISTANCE
GATE_MAX_SIDE = limits.GATE_MAX_SIDE


def _gate_shape(who: str, n: int, h: int, w: int) -> None:
    if n > 65535 or h > GATE_MAX_SIDE or w > GATE_MAX_SIDE:
        raise ValueError(f"{who}: N={n} (<= 65535) H={h} W={w} (<= {GATE_MAX_SIDE})")


def distance_gate(mask: torch.Tensor, distance: int, invert: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fosvos_distance_gate: mask uint8 [N,H,W] -> uint8 [N,H,W], 1 where every set pixel of the frame is further than
    ``distance`` (0..4095, Euclidean, exact in integers); a pixel is set when ``(mask != 0) != invert``, and a frame without
    a set pixel gives all 1 (util/online_adapt.far_from).  With ``invert`` it is the erosion of the mask by the disk.
    Launched on the current stream, no synchronisation."""
    n, h, w = _map_shape(mask, "distance_gate", "mask")
    _gate_shape("distance_gate", n, h, w)
    limits.check_int("distance_gate", "distance", distance, 0, GATE_MAX_DISTANCE)
    out = _out_like(out, (n, h, w), torch.uint8, mask, "distance_gate")
    if out.data_ptr() == mask.data_ptr():
        raise ValueError("distance_gate: out must not be the mask itself")
    ws, wsn = _WS.get(lib().fosvos_distance_gate_workspace_bytes(n, h, w), mask.device)
    _launch("distance_gate", mask, mask.data_ptr(), n, h, w, distance, int(bool(invert)), out.data_ptr(), ws, wsn,
            nbytes=6.0 * n * h * w)
    return out


def adapt_labels(logits: torch.Tensor, last_mask: torch.Tensor, pos_logit: float, neg_distance: int, erode: int = 0,
                 label: Optional[torch.Tensor] = None, void: Optional[torch.Tensor] = None,
                 counts: Optional[torch.Tensor] = None):
    """fosvos_adapt_labels: logits fp32 [N,1,H,W] and last_mask uint8 [N,H,W] (non-zero = object) -> (label fp32 [N,1,H,W],
    void uint8 [N,1,H,W], counts int32 [N,3] = positives, negatives, void): the pseudo-labels of online adaptation
    (util/online_adapt.adapt_labels).  Further than ``neg_distance`` from the mask eroded by ``erode`` (both 0..4095) is a
    negative - unless that core is empty -, elsewhere ``logits >= float32(pos_logit)`` is a positive, the rest is void.
    ``counts`` may be any [N,3] int32 rows, e.g. a slice of a sequence's counter tensor; the op zeroes them itself.
    Launched on the current stream, no synchronisation."""
    _need(logits, _F32, "adapt_labels logits", ValueError)
    _need(last_mask, torch.uint8, "adapt_labels last_mask", ValueError)
    n, h, w = _logit_shape(logits, "adapt_labels")
    _gate_shape("adapt_labels", n, h, w)
    if tuple(last_mask.shape) != (n, h, w):
        raise ValueError(f"adapt_labels: last_mask must be {(n, h, w)}, got {tuple(last_mask.shape)}")
    limits.check_int("adapt_labels", "neg_distance", neg_distance, 0, GATE_MAX_DISTANCE)
    limits.check_int("adapt_labels", "erode", erode, 0, GATE_MAX_DISTANCE)
    # (a threshold, not a range: an infinite one is a number here)
    if isinstance(pos_logit, bool) or not isinstance(pos_logit, (int, float)) or pos_logit != pos_logit:
        raise ValueError(f"adapt_labels: pos_logit must be a number, got {pos_logit!r}")
    label = _out_like(label, (n, 1, h, w), _F32, logits, "adapt_labels label")
    void = _out_like(void, (n, 1, h, w), torch.uint8, logits, "adapt_labels void")
    counts = _out_like(counts, (n, 3), torch.int32, logits, "adapt_labels counts")
    _same_device("adapt_labels", logits, last_mask)
    ws, wsn = _WS.get(lib().fosvos_adapt_labels_workspace_bytes(n, h, w), logits.device)
    _launch("adapt_labels", logits, logits.data_ptr(), last_mask.data_ptr(), n, h, w, float(pos_logit), neg_distance, erode,
            label.data_ptr(), void.data_ptr(), counts.data_ptr(), ws, wsn, nbytes=(15.0 if erode == 0 else 21.0) * n * h * w)
    return label, void, counts


# ------------------------------------------------------------------------------------------ PNG files (png.hip)
def png_capacity(h: int, w: int) -> int:
    """Bytes ``png_encode`` reserves per frame: the layout's size bound (util/png_layout.max_file_bytes)."""
    return int(lib().fosvos_png_capacity_bytes(1, int(h), int(w)))


PNG_HUFFMAN = {'fixed': 0, 'fitted': 1}


def png_encode(bytes_u8: torch.Tensor, out: Optional[torch.Tensor] = None, lengths: Optional[torch.Tensor] = None,
               huffman: str = 'fixed') -> Tuple[torch.Tensor, torch.Tensor]:
    """fosvos_png_encode: uint8 [N,H,W] (``prob_bytes``' output) -> (buffer uint8 [N,capacity], lengths int32 [N]): frame n's
    8-bit greyscale PNG file is ``buffer[n, :lengths[n]]``, in the layout util/png_layout.py states; the bytes behind it
    are not written.  ``out`` (uint8 [N, >= png_capacity(H, W)]) and ``lengths`` (int32 [N]) may be views of a caller's
    buffer.  ``huffman='fitted'``: a segment may also be a dynamic-Huffman block with a code fitted
    to it, where that is shorter - the same pixels in files that are never longer, ``png_layout.encode(img, 'fitted')``.
    Launched on the current stream, no synchronisation."""
    mode = PNG_HUFFMAN[limits.check_member("png_encode", "huffman", huffman, PNG_HUFFMAN)]
    n, h, w = _map_shape(bytes_u8, "png_encode", "bytes")
    L = lib()
    out, lengths = _file_buffers(out, lengths, n, int(L.fosvos_png_capacity_bytes(n, h, w)), bytes_u8, "png_encode")
    ws, wsn = _WS.get(L.fosvos_png_workspace_bytes(n, h, w, mode), bytes_u8.device)
    _launch("png_encode", bytes_u8, bytes_u8.data_ptr(), n, h, w, mode, out.data_ptr(), int(out.shape[1]), lengths.data_ptr(),
            ws, wsn, nbytes=2.0 * n * h * w)
    return out, lengths


# ------------------------------------------------------------------------------------------ several objects (eval.hip, png.hip)
def merge_objects(logits: Sequence[torch.Tensor], out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fosvos_merge_objects: the logits fp32 [N,1,H,W] of K per-object nets (1 <= K <= 16) -> labels uint8 [N,H,W]: 0 where
    no logit of the pixel is >= 0, else 1 + the lowest k holding the largest such logit (util/object_merge.merge_labels).
    The K pointers travel by value: nothing is concatenated.  ``out`` may be a view of a caller's buffer.  Launched on the
    current stream, no synchronisation."""
    logits, (n, _, h, w), table = _logit_table(logits, "merge_objects")
    out = _out_like(out, (n, h, w), torch.uint8, logits[0], "merge_objects")
    _same_device("merge_objects", logits[0], *logits[1:])
    k = len(logits)
    _launch("merge_objects", logits[0], table, k, n, h, w, out.data_ptr(), nbytes=(4.0 * k + 1.0) * n * h * w)
    return out


def jf_counts_labels(pred_labels: torch.Tensor, gt_labels: torch.Tensor, n_objects: int, radius: Optional[int] = None,
                     out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fosvos_jf_counts_labels: two label maps uint8 [N,H,W] -> int32 [N,K,6]: row (n, k-1) holds the six counts of
    ``jf_counts`` for the masks ``pred == k`` and ``gt == k`` (util/object_merge.jf_counts_labels_numpy); labels above
    ``n_objects`` belong to no object.  ``radius`` (1..63) defaults to ceil(0.008 * diagonal).  ``out`` may be any [N,K,6]
    int32 rows, e.g. a slice of a sequence's counter tensor; the op zeroes them itself.  Launched on the current stream, no
    synchronisation."""
    _need(gt_labels, torch.uint8, "jf_counts_labels gt", ValueError)
    n, h, w = _map_shape(pred_labels, "jf_counts_labels", "pred")
    if tuple(gt_labels.shape) != (n, h, w):
        raise ValueError(f"jf_counts_labels: gt must be {(n, h, w)}, got {tuple(gt_labels.shape)}")
    k = limits.check_int("jf_counts_labels", "n_objects", int(n_objects), 1, MAX_OBJECTS)
    radius = _jf_radius(radius, h, w, "jf_counts_labels")
    out = _out_like(out, (n, k, 6), torch.int32, pred_labels, "jf_counts_labels")
    _same_device("jf_counts_labels", pred_labels, gt_labels)
    ws, wsn = _WS.get(lib().fosvos_jf_labels_workspace_bytes(n, k, h, w), pred_labels.device)
    _launch("jf_counts_labels", pred_labels, pred_labels.data_ptr(), gt_labels.data_ptr(), n, k, h, w, radius, out.data_ptr(),
            ws, wsn, nbytes=2.0 * n * h * w)
    return out


def png_indexed_capacity(h: int, w: int) -> int:
    """Bytes ``png_encode_indexed`` reserves per frame (util/png_layout.max_file_bytes_indexed)."""
    return int(lib().fosvos_png_indexed_capacity_bytes(1, int(h), int(w)))


def png_encode_indexed(labels_u8: torch.Tensor, palette: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                       lengths: Optional[torch.Tensor] = None, huffman: str = 'fixed') -> Tuple[torch.Tensor, torch.Tensor]:
    """fosvos_png_encode_indexed: labels uint8 [N,H,W] -> (buffer uint8 [N,capacity], lengths int32 [N]): frame n's 8-bit
    palette PNG file is ``buffer[n, :lengths[n]]``, ``png_layout.encode_indexed(labels[n], palette, huffman)`` byte for byte.
    ``palette``: uint8 [256,3] RGB on the device; None = the DAVIS palette (``default_palette``).  ``out`` (uint8
    [N, >= png_indexed_capacity(H, W)]) and ``lengths`` (int32 [N]) may be views of a caller's buffer.  Launched on the
    current stream, no synchronisation."""
    mode = PNG_HUFFMAN[limits.check_member("png_encode_indexed", "huffman", huffman, PNG_HUFFMAN)]
    n, h, w = _map_shape(labels_u8, "png_encode_indexed", "labels")
    palette = _palette(palette, labels_u8.device, "png_encode_indexed")
    L = lib()
    out, lengths = _file_buffers(out, lengths, n, int(L.fosvos_png_indexed_capacity_bytes(n, h, w)), labels_u8,
                                 "png_encode_indexed")
    ws, wsn = _WS.get(L.fosvos_png_workspace_bytes(n, h, w, mode), labels_u8.device)
    _launch("png_encode_indexed", labels_u8, labels_u8.data_ptr(), palette.data_ptr(), n, h, w, mode, out.data_ptr(),
            int(out.shape[1]), lengths.data_ptr(), ws, wsn, nbytes=2.0 * n * h * w)
    return out, lengths


# ------------------------------------------------------------------------------------------ test-time ensemble (ensemble.hip)
ENSEMBLE_MAX_VIEWS = limits.ENSEMBLE_MAX_VIEWS  # util/test_ensemble.MAX_VIEWS


def _ensemble_views(views, h: int, w: int, what: str):
    """The views of an [h,w] frame as a list of (scale, flip, (hs, ws)); (hs, ws) = ``test_ensemble.view_sizes``."""
    from util.test_ensemble import view_sizes
    views = list(views)
    if not 1 <= len(views) <= ENSEMBLE_MAX_VIEWS:
        raise ValueError(f"{what}: {len(views)} views, outside [1, {ENSEMBLE_MAX_VIEWS}]")
    out = []
    for v in views:
        try:
            scale, flip = v
        except (TypeError, ValueError):
            raise ValueError(f"{what}: a view must be (scale, flip), got {v!r}") from None
        limits.check_real(what, "a view's scale", scale, *limits.ENSEMBLE_SCALE_RANGE)
        if not isinstance(flip, bool):
            raise ValueError(f"{what}: a view's flip must be a bool, got {flip!r}")
        hs, ws = view_sizes(h, w, scale)
        if hs > MAX_FRAME_SIDE or ws > MAX_FRAME_SIDE:
            raise ValueError(f"{what}: the view of scale {scale!r} is {(hs, ws)}, a side above {MAX_FRAME_SIDE}")
        out.append((scale, flip, (hs, ws)))
    return out


def _ensemble_frame(n: int, h: int, w: int, what: str) -> None:
    if n > 65535 or h > MAX_FRAME_SIDE or w > MAX_FRAME_SIDE:
        raise ValueError(f"{what}: N={n} (<= 65535) H={h} W={w} (<= {MAX_FRAME_SIDE})")


def _overlap(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Two contiguous tensors share a byte."""
    a0, b0 = a.data_ptr(), b.data_ptr()
    return a0 < b0 + b.numel() * b.element_size() and b0 < a0 + a.numel() * a.element_size()


def _ensemble_table(tensors, views):
    from . import EnsembleView
    table = (EnsembleView * len(tensors))()
    for entry, t, (_, flip, (hs, ws)) in zip(table, tensors, views):
        entry.data, entry.h, entry.w, entry.flip = t.data_ptr(), hs, ws, int(flip)
    return table


def ensemble_views(image: torch.Tensor, views, out=None) -> List[torch.Tensor]:
    """fosvos_ensemble_views: image fp32 [N,3,H,W] and up to 8 views ``(scale, flip)`` -> one fp32 [N,3,Hs,Ws] per view,
    ``test_ensemble.make_views(image, views)`` bit for bit, all of them from ONE launch.  (Hs, Ws) =
    ``test_ensemble.view_sizes(H, W, scale)``; a flipped view is mirrored along W; a view of the frame's size is a copy, any
    other is resampled bilinearly in fp64.  An unflipped view of the frame's size comes back as ``image`` itself, not a
    copy, and takes no part in the launch (with nothing else asked for, nothing is launched).  ``out``: a list with one
    entry per view - None for such an identity view, else the tensor to write; none may overlap the image or another.
    Launched on the current stream, no synchronisation."""
    what = "ensemble_views"
    _need(image, _F32, f"{what} image", ValueError)
    if image.dim() != 4 or image.shape[1] != 3 or image.numel() == 0:
        raise ValueError(f"{what}: image must be a non-empty [N,3,H,W], got {tuple(image.shape)}")
    n, h, w = int(image.shape[0]), int(image.shape[2]), int(image.shape[3])
    _ensemble_frame(n, h, w, what)
    views = _ensemble_views(views, h, w, what)
    if out is not None:
        out = list(out)
        if len(out) != len(views):
            raise ValueError(f"{what}: out must hold one entry per view ({len(views)}), got {len(out)}")
    result, made = [], []
    for k, (scale, flip, size) in enumerate(views):
        given = None if out is None else out[k]
        if size == (h, w) and not flip:
            if given is not None:
                raise ValueError(f"{what}: out[{k}] must be None: view {k} is the image itself")
            result.append(image)
            continue
        t = _out_like(given, (n, 3) + size, _F32, image, what, f"out[{k}]")
        if given is not None and (_overlap(t, image) or any(_overlap(t, other) for other, _ in made)):
            raise ValueError(f"{what}: out[{k}] must not overlap the image or another view")
        result.append(t)
        made.append((t, views[k]))
    if made:
        table = _ensemble_table([t for t, _ in made], [v for _, v in made])
        _launch(what, image, image.data_ptr(), n, h, w, table, len(made),
                nbytes=4.0 * (len(made) * image.numel() + sum(t.numel() for t, _ in made)))
    return result


def ensemble_merge(logits: Sequence[torch.Tensor], views, size: Tuple[int, int], out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fosvos_ensemble_merge: the logits fp32 [N,1,Hs_k,Ws_k] the net gave for the views ``(scale, flip)`` of a frame of
    ``size`` = (H, W) -> fp32 [N,1,H,W], ``test_ensemble.merge(logits, views, H, W)`` bit for bit: every map resampled to
    [H,W] (a map of that size as it is), mirrored back where its view was flipped, summed in fp64 in the order of the views
    and divided by their number.  The pointers travel by value: nothing is concatenated.  ``out`` must not overlap a map.
    Launched on the current stream, no synchronisation."""
    what = "ensemble_merge"
    h, w = limits.check_pair(what, "size", size, "(H, W)")
    logits = list(logits)
    views = _ensemble_views(views, h, w, what)
    if len(logits) != len(views):
        raise ValueError(f"{what}: {len(logits)} logit maps for {len(views)} views")
    for t in logits:
        _need(t, _F32, f"{what} logits", ValueError)
    n = _logit_shape(logits[0], what)[0]
    _ensemble_frame(n, h, w, what)
    for k, (t, (scale, flip, vsize)) in enumerate(zip(logits, views)):
        if tuple(t.shape) != (n, 1) + vsize:
            raise ValueError(f"{what}: the map of view {k} {(scale, flip)} must be {(n, 1) + vsize}, got {tuple(t.shape)}")
    _same_device(what, logits[0], *logits[1:])
    given = out
    out = _out_like(out, (n, 1, h, w), _F32, logits[0], what)
    if given is not None and any(_overlap(out, t) for t in logits):
        raise ValueError(f"{what}: out must not overlap a logit map")
    _launch(what, logits[0], _ensemble_table(logits, views), len(views), n, h, w, out.data_ptr(),
            nbytes=4.0 * (sum(t.numel() for t in logits) + out.numel()))
    return out


# ------------------------------------------------------------------------------------------ the CRF on the frame (crf.hip)
CRF_MAX_RADIUS = limits.CRF_MAX_RADIUS          # util/mask_crf.MAX_RADIUS
CRF_MAX_ITERATIONS = limits.CRF_MAX_ITERATIONS  # util/mask_crf.MAX_ITERATIONS
_CRF_TABLES = {}  # (CrfOptions, device index) -> the fp64 table vector on that device


def _crf_tables(options, device: torch.device, labels: bool = False) -> torch.Tensor:
    """``mask_crf.tables(options)`` - ``labels``: ``label_crf.tables(options)``, under a key of its own - on ``device``, made
    and uploaded at the first call with these options (the one moment a ``crf_refine`` / ``crf_labels`` call waits for the host
    copy) and kept."""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    key = (options, idx, "labels") if labels else (options, idx)
    tab = _CRF_TABLES.get(key)
    if tab is None:
        from util import label_crf, mask_crf
        tab = _CRF_TABLES[key] = torch.from_numpy((label_crf if labels else mask_crf).tables(options)).to(device)
    return tab


def _crf_frames(what: str, image: torch.Tensor, options):
    """The checks ``crf_refine`` and ``crf_labels`` share: (the options, N, H, W) of the net's input fp32 [N,3,H,W]."""
    from .options import CrfOptions
    if options is None:
        options = CrfOptions()
    if not isinstance(options, CrfOptions):
        raise ValueError(f"{what}: options must be a fosvos_hip.options.CrfOptions or None, got {options!r}")
    _need(image, _F32, f"{what} image", ValueError)
    if image.dim() != 4 or image.shape[1] != 3 or image.numel() == 0:
        raise ValueError(f"{what}: image must be a non-empty [N,3,H,W], got {tuple(image.shape)}")
    n, h, w = int(image.shape[0]), int(image.shape[2]), int(image.shape[3])
    if h > MAX_FRAME_SIDE or w > MAX_FRAME_SIDE:
        raise ValueError(f"{what}: maps may have sides of up to {MAX_FRAME_SIDE}, got {(h, w)}")
    return options, n, h, w


def crf_refine(image: torch.Tensor, logits: torch.Tensor, options=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fosvos_crf_refine: the net's input fp32 [N,3,H,W] (the frame minus MEANVAL) and logits fp32 [N,1,H,W] -> fp32 [N,1,H,W],
    the logits after ``options.iterations`` mean-field iterations of the local CRF whose guide is the frame's bytes
    (``mask_crf.refine(image[k], logits[k, 0], options)`` of every frame, bit for bit).  ``options``: a
    ``fosvos_hip.options.CrfOptions`` (None: its defaults).  ``out`` must not overlap the image or the logits.  The table
    vector (``mask_crf.tables(options)``) is kept on the device per (options, device).  ``options.iterations`` launches on the
    current stream, no synchronisation; z^t lives in the stream's workspace."""
    what = "crf_refine"
    options, n, h, w = _crf_frames(what, image, options)
    _need(logits, _F32, f"{what} logits", ValueError)
    if tuple(logits.shape) != (n, 1, h, w):
        raise ValueError(f"{what}: logits must be {(n, 1, h, w)}, got {tuple(logits.shape)}")
    _same_device(what, image, logits)
    given = out
    out = _out_like(out, (n, 1, h, w), _F32, image, what)
    if given is not None and (_overlap(out, image) or _overlap(out, logits)):
        raise ValueError(f"{what}: out must not overlap the image or the logits")
    tab = _crf_tables(options, image.device)
    ws, wsn = _WS.get(int(lib().fosvos_crf_refine_workspace_bytes(n, h, w)), image.device)
    window = (2 * options.radius + 1) ** 2 - 1
    _launch(what, image, image.data_ptr(), logits.data_ptr(), tab.data_ptr(), n, h, w, options.iterations, options.radius,
            float(options.weight_appearance), float(options.weight_smooth), float(options.clip), _mean_bgr(), out.data_ptr(), ws,
            wsn, flops=9.0 * window * options.iterations * n * h * w, nbytes=(16.0 * options.iterations + 4.0) * n * h * w)
    return out


def crf_labels(image: torch.Tensor, logits: Sequence[torch.Tensor], options=None, out: Optional[torch.Tensor] = None,
               scores: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fosvos_crf_labels: the net's input fp32 [N,3,H,W] and the logits fp32 [N,1,H,W] of K per-object nets (1 <= K <=
    ``MAX_OBJECTS``) -> labels uint8 [N,H,W]: ONE mean-field CRF over the labels 0..K whose guide is the frame's bytes, in the
    place of K ``crf_refine`` calls and ``merge_objects`` (``label_crf.refine_labels_batch(image, logits, options)``, bit for
    bit).  ``scores``: None, or an fp32 [N,K+1,H,W] tensor that takes ``float32(z^T)``.  The K pointers travel by value:
    nothing is concatenated.  ``out`` and ``scores`` may be views of a caller's buffer and must not overlap an input.  The table
    vector (``label_crf.tables(options)``) is kept on the device per (options, device), beside ``crf_refine``'s.
    ``options.iterations`` launches on the current stream, no synchronisation; z^t lives in the stream's workspace, 16 (K + 1)
    N H W bytes, which grows to that (557 MB at K = 16, five frames of 480x854): the batch is not walked in sub-batches."""
    what = "crf_labels"
    options, n, h, w = _crf_frames(what, image, options)
    logits, _, table = _logit_table(logits, what, (n, 1, h, w))
    k = len(logits)
    _same_device(what, image, *logits)
    given = [t for t in (out, scores) if t is not None]
    out = _out_like(out, (n, h, w), torch.uint8, image, what)
    if scores is not None:
        scores = _out_like(scores, (n, k + 1, h, w), _F32, image, what, "scores")
    if any(_overlap(t, x) for t in given for x in [image] + logits) or (len(given) == 2 and _overlap(out, scores)):
        raise ValueError(f"{what}: out and scores must not overlap the image, the logits or each other")
    tab = _crf_tables(options, image.device, labels=True)
    ws, wsn = _WS.get(int(lib().fosvos_crf_labels_workspace_bytes(n, k, h, w)), image.device)
    window = (2 * options.radius + 1) ** 2 - 1
    chunks = -(-(k + 1) // 4)
    _launch(what, image, image.data_ptr(), table, k, tab.data_ptr(), n, h, w, options.iterations, options.radius,
            float(options.weight_appearance), float(options.weight_smooth), float(options.clip), _mean_bgr(), out.data_ptr(),
            _p(scores), ws, wsn, flops=(5.0 * chunks + 4.0 * (k + 1)) * window * options.iterations * n * h * w,
            nbytes=(16.0 * (k + 1) * options.iterations + 4.0 * k + 1.0) * n * h * w)
    return out


# ------------------------------------------------------------------------------------------ block matching (motion.hip)
MOTION_BLOCKS = limits.MOTION_BLOCKS          # util/block_motion.BLOCKS
MOTION_MAX_SEARCH = limits.MOTION_MAX_SEARCH  # util/block_motion.MAX_SEARCH


def _motion_grid(h: int, w: int, block: int) -> Tuple[int, int]:
    return -(-h // block), -(-w // block)


def motion_luma(image: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fosvos_motion_luma: the net's input fp32 [N,3,H,W] (the frame minus MEANVAL) -> uint8 [N,H,W], the luma of the frame's
    bytes (``block_motion.luma``, bit for bit; a NaN is level 0).  One launch on the current stream, no synchronisation."""
    what = "motion_luma"
    _need(image, _F32, f"{what} image", ValueError)
    if image.dim() != 4 or image.shape[1] != 3 or image.numel() == 0:
        raise ValueError(f"{what}: image must be a non-empty [N,3,H,W], got {tuple(image.shape)}")
    n, h, w = int(image.shape[0]), int(image.shape[2]), int(image.shape[3])
    if h > MAX_FRAME_SIDE or w > MAX_FRAME_SIDE:
        raise ValueError(f"{what}: frames may have sides of up to {MAX_FRAME_SIDE}, got {(h, w)}")
    out = _out_like(out, (n, h, w), torch.uint8, image, what)
    _launch(what, image, image.data_ptr(), _mean_bgr(), n, h, w, out.data_ptr(), nbytes=13.0 * n * h * w)
    return out


def motion_estimate(prev_y: torch.Tensor, cur_y: torch.Tensor, options=None, field: Optional[torch.Tensor] = None,
                    cost: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """fosvos_motion_estimate: luma planes uint8 [N,H,W] of the frames before and the current frames -> (field int8
    [N,Hb,Wb,2], cost int32 [N,Hb,Wb]): for every ``options.block``-sized block of every pair the vector ``(dy, dx)`` within
    ``options.search`` with ``cur[p] ~ prev[p + (dy, dx)]`` and its sum of absolute differences (``block_motion.estimate``,
    bit for bit).  ``options``: a ``fosvos_hip.options.MotionOptions`` (None: its defaults).  The two planes may be views of one
    buffer one frame apart.  ONE launch for all N pairs on the current stream, no synchronisation."""
    from .options import MotionOptions
    what = "motion_estimate"
    if options is None:
        options = MotionOptions()
    if not isinstance(options, MotionOptions):
        raise ValueError(f"{what}: options must be a fosvos_hip.options.MotionOptions or None, got {options!r}")
    n, h, w = _map_shape(prev_y, what, "prev_y")
    _need(cur_y, torch.uint8, f"{what} cur_y", ValueError)
    if tuple(cur_y.shape) != (n, h, w):
        raise ValueError(f"{what}: cur_y must be {(n, h, w)}, got {tuple(cur_y.shape)}")
    if h > MAX_FRAME_SIDE or w > MAX_FRAME_SIDE:
        raise ValueError(f"{what}: planes may have sides of up to {MAX_FRAME_SIDE}, got {(h, w)}")
    _same_device(what, prev_y, cur_y)
    hb, wb = _motion_grid(h, w, options.block)
    field = _out_like(field, (n, hb, wb, 2), torch.int8, prev_y, what, "field")
    cost = _out_like(cost, (n, hb, wb), torch.int32, prev_y, what, "cost")
    cands = (2 * options.search + 1) ** 2
    _launch(what, prev_y, prev_y.data_ptr(), cur_y.data_ptr(), n, h, w, options.block, options.search, options.zero_bias,
            field.data_ptr(), cost.data_ptr(), flops=2.0 * cands * n * h * w, nbytes=2.0 * n * h * w)
    return field, cost


def motion_warp(mask: torch.Tensor, field: torch.Tensor, block: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fosvos_motion_warp: mask uint8 [N,H,W] (non-zero = set) and field int8 [N,Hb,Wb,2] -> uint8 [N,H,W] of 0 and 1:
    ``out[y, x] = mask[y + dy, x + dx] != 0`` with the vector of the pixel's block, 0 where the source lies outside the frame
    (``block_motion.warp``, bit for bit; the field may hold any values).  ``out`` must not overlap the mask.  One launch on
    the current stream, no synchronisation."""
    what = "motion_warp"
    n, h, w = _map_shape(mask, what, "mask")
    if h > MAX_FRAME_SIDE or w > MAX_FRAME_SIDE:
        raise ValueError(f"{what}: masks may have sides of up to {MAX_FRAME_SIDE}, got {(h, w)}")
    limits.check_member(what, "block", block, MOTION_BLOCKS)
    _need(field, torch.int8, f"{what} field", ValueError)
    want = (n,) + _motion_grid(h, w, block) + (2,)
    if tuple(field.shape) != want:
        raise ValueError(f"{what}: field must be {want}, got {tuple(field.shape)}")
    _same_device(what, mask, field)
    given = out
    out = _out_like(out, (n, h, w), torch.uint8, mask, what)
    if given is not None and _overlap(out, mask):
        raise ValueError(f"{what}: out must not overlap the mask")
    _launch(what, mask, mask.data_ptr(), field.data_ptr(), n, h, w, int(block), out.data_ptr(), nbytes=2.0 * n * h * w)
    return out


# ------------------------------------------------------------------------------------------ JPEG files (jpeg.hip)
JPEG_SUBSAMPLINGS = limits.JPEG_SUBSAMPLINGS


def _jpeg_sampling(subsampling, what: str) -> int:
    """The C ABI's code of a chroma sampling: 420 for '4:2:0', 444 for '4:4:4', ValueError for anything else."""
    return 420 if limits.check_member(what, "subsampling", subsampling, JPEG_SUBSAMPLINGS) == '4:2:0' else 444


def jpeg_capacity(h: int, w: int, components: int, subsampling: str = '4:4:4') -> int:
    """Bytes ``jpeg_encode`` reserves per frame: the layout's size bound (util/jpeg_layout.capacity)."""
    cap = int(lib().fosvos_jpeg_capacity_bytes(1, int(h), int(w), int(components), _jpeg_sampling(subsampling, "jpeg_capacity")))
    if cap == 0:
        raise ValueError(f"jpeg_capacity: h, w in 1..65535 and components 1 or 3, got {h}, {w}, {components}")
    return cap


def jpeg_encode(frames_u8: torch.Tensor, quality: int = 90, out: Optional[torch.Tensor] = None,
                lengths: Optional[torch.Tensor] = None, subsampling: str = '4:4:4') -> Tuple[torch.Tensor, torch.Tensor]:
    """fosvos_jpeg_encode: uint8 [N,H,W,3] BGR (``overlay``'s output) or [N,H,W] grey -> (buffer uint8 [N,capacity], lengths
    int32 [N]): frame n's baseline JPEG file is ``buffer[n, :lengths[n]]``, in the layout util/jpeg_layout.py states; the
    bytes behind it are not written.  ``out`` (uint8 [N, >= jpeg_capacity(H, W, components, subsampling)]) and ``lengths``
    (int32 [N]) may be views of a caller's buffer.  ``subsampling='4:2:0'`` halves the chroma
    planes of a colour frame; a grey frame ignores it.  Launched on the current stream, no synchronisation."""
    sampling = _jpeg_sampling(subsampling, "jpeg_encode")
    _need(frames_u8, torch.uint8, "jpeg_encode frames", ValueError)
    if frames_u8.numel() == 0 or not (frames_u8.dim() == 3 or (frames_u8.dim() == 4 and frames_u8.shape[3] == 3)):
        raise ValueError(f"jpeg_encode: frames must be a non-empty [N,H,W,3] or [N,H,W], got {tuple(frames_u8.shape)}")
    quality = limits.check_int("jpeg_encode", "quality", quality, *limits.JPEG_QUALITY, integral=True)
    n, h, w = (int(v) for v in frames_u8.shape[:3])
    comps = 3 if frames_u8.dim() == 4 else 1
    L = lib()
    cap = int(L.fosvos_jpeg_capacity_bytes(n, h, w, comps, sampling))
    if cap == 0:
        raise ValueError(f"jpeg_encode: H and W must be at most 65535, got {h}, {w}")
    out, lengths = _file_buffers(out, lengths, n, cap, frames_u8, "jpeg_encode")
    ws, wsn = _WS.get(L.fosvos_jpeg_workspace_bytes(n, h, w, comps, sampling), frames_u8.device)
    _launch("jpeg_encode", frames_u8, frames_u8.data_ptr(), n, h, w, comps, sampling, quality, out.data_ptr(), int(out.shape[1]),
            lengths.data_ptr(), ws, wsn, nbytes=2.0 * n * h * w * comps)
    return out, lengths


# ------------------------------------------------------------------------------------------ JPEG files in (jpeg_decode.hip)
def _jpeg_decode_plans(files, plans):
    from util import jpeg_read
    if len(files) == 0:
        raise ValueError("jpeg_decode: no files")
    if plans is None:
        plans = [jpeg_read.probe(f) for f in files]
    if len(plans) != len(files):
        raise ValueError(f"jpeg_decode: {len(files)} files but {len(plans)} plans")
    for i, p in enumerate(plans):
        if p is None:
            raise ValueError(f"jpeg_decode: file {i} is not one the device decoder takes (util/jpeg_read.probe is None): "
                             f"decode it on the host")
    key = lambda p: (p.height, p.width, p.components, p.subsampling)  # noqa: E731
    for i, p in enumerate(plans):
        if key(p) != key(plans[0]):
            raise ValueError(f"jpeg_decode: the files of one call share shape, components and sampling; file 0 is "
                             f"{key(plans[0])}, file {i} is {key(p)}")
    return plans


def jpeg_decode_workspace(n: int, h: int, w: int, components: int, subsampling: str = '4:4:4') -> int:
    """Bytes of scratch ``jpeg_decode`` needs for ``n`` files of this shape (fosvos_jpeg_decode_workspace_bytes)."""
    need = int(lib().fosvos_jpeg_decode_workspace_bytes(int(n), int(h), int(w), int(components),
                                                        _jpeg_sampling(subsampling, "jpeg_decode_workspace")))
    if need == 0:
        raise ValueError(f"jpeg_decode_workspace: n, h, w in 1..65535, components 1 or 3, 4:2:0 from w = 5, got {n}, {h}, {w}, "
                         f"{components}, {subsampling}")
    return need


def jpeg_decode_pack(files: Sequence[bytes], plans):
    """What one call sends, in ONE pinned uint8 buffer: the segment rows (int32 [n_segments][5]: file, byte offset, byte
    length, first MCU, MCU count) | the per-file tables (util/jpeg_read.pack_tables) | the scans of all files.  Returns
    (buffer, n_segments, offset of the tables, offset of the scans, bytes of scans)."""
    import numpy as np
    from util import jpeg_read
    n = len(files)
    n_seg = sum(len(p.segments) for p in plans)
    off_tables = _ru(20 * n_seg, 8)
    off_bytes = off_tables + jpeg_read.TABLES_BYTES * n
    n_bytes = sum(p.scan[1] - p.scan[0] for p in plans)
    if n_bytes <= 0 or n_bytes >= 1 << 31:
        raise ValueError(f"jpeg_decode: {n_bytes} bytes of entropy-coded data in one call (1 .. 2^31 - 1)")
    host = torch.empty(off_bytes + n_bytes, dtype=torch.uint8, pin_memory=True)
    hv = host.numpy()
    hv[20 * n_seg:off_tables] = 0
    rows = hv[:20 * n_seg].view(np.int32).reshape(n_seg, 5)
    seg_at, byte_at = 0, 0
    for i, (f, p) in enumerate(zip(files, plans)):
        k, (b0, b1) = len(p.segments), p.scan
        rows[seg_at:seg_at + k, 0] = i
        rows[seg_at:seg_at + k, 1:] = p.segments
        rows[seg_at:seg_at + k, 1] += byte_at - b0
        hv[off_tables + i * jpeg_read.TABLES_BYTES:off_tables + (i + 1) * jpeg_read.TABLES_BYTES] = np.frombuffer(
            jpeg_read.pack_tables(p, seg_at, k), dtype=np.uint8)
        hv[off_bytes + byte_at:off_bytes + byte_at + b1 - b0] = np.frombuffer(f, dtype=np.uint8, count=b1 - b0, offset=b0)
        seg_at += k
        byte_at += b1 - b0
    return host, n_seg, off_tables, off_bytes, n_bytes


def jpeg_decode(files: Sequence[bytes], out: Optional[torch.Tensor] = None, status: Optional[torch.Tensor] = None,
                device=None, plans=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """fosvos_jpeg_decode: baseline JPEG files of one shape -> (frames uint8 [N,H,W,3] BGR or [N,H,W] grey, status int32 [N]),
    byte for byte util/jpeg_read.decode.  Every file is probed (``plans``: the probes, where the caller has them already);
    ValueError where a probe is None or the files disagree in shape, components or sampling - a caller that wants the host
    fallback probes first.  The scans, the segment table and the per-file tables travel in ONE pinned buffer and one upload.
    ``out`` and ``status`` may be views of a caller's buffers.  A frame whose status is not 0 is not meaningful (the codes:
    util/jpeg_read.py); the status is the caller's to read.  Three launches on the current stream, no synchronisation."""
    from util import jpeg_read
    plans = _jpeg_decode_plans(files, plans)
    p0 = plans[0]
    n, h, w, comps = len(files), p0.height, p0.width, p0.components
    if device is None:
        device = out.device if out is not None else torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"jpeg_decode: the device must be a GPU (the HIP path has no CPU fallback), got {device}")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    shape = (n, h, w, 3) if comps == 3 else (n, h, w)
    out = _out_like(out, shape, torch.uint8, device, "jpeg_decode")
    status = _out_like(status, (n,), torch.int32, device, "jpeg_decode", "status")
    L = lib()
    sampling = jpeg_read.SAMPLING_CODE[p0.subsampling]
    need = int(L.fosvos_jpeg_decode_workspace_bytes(n, h, w, comps, sampling))
    if need == 0:
        raise ValueError(f"jpeg_decode: at most 65535 files, got {n}")
    host, n_seg, off_tables, off_bytes, n_bytes = jpeg_decode_pack(files, plans)
    with torch.cuda.device(device):
        dev_buf = host.to(device, non_blocking=True)
        base = dev_buf.data_ptr()
        ws, wsn = _WS.get(need, device)
        _launch("jpeg_decode", out, base + off_bytes, n_bytes, base, n_seg, base + off_tables, n, h, w, comps, sampling,
                out.data_ptr(), status.data_ptr(), ws, wsn, nbytes=float(n_bytes) + float(out.numel()))
    return out, status


# ------------------------------------------------------------------------------------------ streaming inference (stream.hip)
OVERLAY_CHANNEL = {'b': 0, 'g': 1, 'r': 2}
_MEAN_BGR = None


def _mean_bgr():
    """The dataset mean the frames lose in front of the net: the one constant of dataloaders/davis_2016.py."""
    global _MEAN_BGR
    if _MEAN_BGR is None:
        from dataloaders.davis_2016 import MEANVAL
        _MEAN_BGR = (ctypes.c_float * 3)(*MEANVAL)
    return _MEAN_BGR


def _frame_shape(frames: torch.Tensor, what: str) -> Tuple[int, int, int]:
    _need(frames, torch.uint8, f"{what} frames", ValueError)
    if frames.dim() != 4 or frames.shape[3] != 3 or frames.numel() == 0:
        raise ValueError(f"{what}: frames must be a non-empty [N,H,W,3], got {tuple(frames.shape)}")
    return int(frames.shape[0]), int(frames.shape[1]), int(frames.shape[2])


def _paint(what: str, color, alpha, overlay, boolean_mask) -> Tuple[int, float, int]:
    """What the single-object paint launches take beside their tensors: (the channel of ``color``, ``alpha`` as a finite
    float >= 0, the mode: 0 overlay of the mask, 1 of the probability, 2 / 3 the mask / the probability alone)."""
    channel = OVERLAY_CHANNEL[limits.check_member(what, "color", color, OVERLAY_CHANNEL)]
    alpha = limits.check_real(what, "alpha", float(alpha), 0.0)
    return channel, alpha, (0 if overlay else 2) + (0 if boolean_mask else 1)


def _net_size(net_size, h: int, w: int, what: str) -> Optional[Tuple[int, int]]:
    """``net_size`` of the scaled ops: None where it is unset or the frames' own size (the callers then take the unscaled
    launch), else (Hn, Wn) checked against the frames."""
    if net_size is None:
        return None
    hn, wn = limits.check_pair(what, "net_size", net_size, "(Hn, Wn)")
    if hn > h or wn > w:
        raise ValueError(f"{what}: the net's size {(hn, wn)} exceeds the frames' {(h, w)}")
    if h > MAX_FRAME_SIDE or w > MAX_FRAME_SIDE:
        raise ValueError(f"{what}: scaled frames may have sides of up to {MAX_FRAME_SIDE}, got {(h, w)}")
    return None if (hn, wn) == (h, w) else (hn, wn)


def frame_prep(frames_u8: torch.Tensor, mirror: bool = False, out: Optional[torch.Tensor] = None,
               net_size: Optional[Tuple[int, int]] = None) -> torch.Tensor:
    """fosvos_frame_prep: raw frames uint8 [N,H,W,3] (BGR) -> the net's input fp32 [N,3,H,W]: ``float32(byte) - MEANVAL[c]``,
    flipped left to right with ``mirror`` (util/frame_overlay.prepare_frame, bit for bit).  One launch on the current
    stream, no synchronisation.

    ``net_size=(Hn, Wn)`` (no larger than the frames): fosvos_frame_prep_scaled, the output is [N,3,Hn,Wn], the exact area
    average of the frame less the mean (util/frame_resample.prepare_frame_scaled, bit for bit).  The frames' own size is
    the launch above."""
    n, h, w = _frame_shape(frames_u8, "frame_prep")
    scaled = _net_size(net_size, h, w, "frame_prep")
    if scaled is not None:
        hn, wn = scaled
        out = _out_like(out, (n, 3, hn, wn), _F32, frames_u8, "frame_prep")
        _launch("frame_prep_scaled", frames_u8, frames_u8.data_ptr(), n, h, w, hn, wn, 1 if mirror else 0, _mean_bgr(),
                out.data_ptr(), nbytes=3.0 * n * h * w + 12.0 * n * hn * wn)
        return out
    out = _out_like(out, (n, 3, h, w), _F32, frames_u8, "frame_prep")
    _launch("frame_prep", frames_u8, frames_u8.data_ptr(), n, h, w, 1 if mirror else 0, _mean_bgr(), out.data_ptr(),
            nbytes=15.0 * n * h * w)
    return out


def overlay(frames_u8: torch.Tensor, logits: torch.Tensor, mirror: bool = False, boolean_mask: bool = True, color: str = 'r',
            alpha: float = 1.0, overlay: bool = True, out: Optional[torch.Tensor] = None,
            net_size: Optional[Tuple[int, int]] = None) -> torch.Tensor:
    """fosvos_overlay: raw frames uint8 [N,H,W,3] and the logits fp32 [N,1,H,W] the net made of them (of the mirrored
    frames, with ``mirror``) -> uint8 [N,H,W,3], the (mirrored) frames with ``alpha * 255 * p`` added to the channel of
    ``color`` and clamped at 255; p is the mask ``logit >= 0`` (``boolean_mask``) or the fp64 sigmoid.  ``overlay=False``:
    uint8 [N,H,W], the mask as 0 / 255 or ``255 p`` rounded half up.  util/frame_overlay.py states the bytes.  One launch on
    the current stream, no synchronisation.

    ``net_size=(Hn, Wn)`` (no larger than the frames): fosvos_overlay_scaled, the logits are [N,1,Hn,Wn] and are interpolated
    up to the frames' size inside the launch; the output keeps the frames' size in every mode
    (util/frame_resample.py states the bytes).  Scaling is never inferred from the shapes."""
    n, h, w = _frame_shape(frames_u8, "overlay")
    scaled = _net_size(net_size, h, w, "overlay")
    hn, wn = scaled if scaled is not None else (h, w)
    _need(logits, _F32, "overlay logits", ValueError)
    if tuple(logits.shape) != (n, 1, hn, wn):
        raise ValueError(f"overlay: logits must be {(n, 1, hn, wn)}, got {tuple(logits.shape)}")
    _same_device("overlay", frames_u8, logits)
    channel, alpha, mode = _paint("overlay", color, alpha, overlay, boolean_mask)
    out = _out_like(out, (n, h, w, 3) if overlay else (n, h, w), torch.uint8, frames_u8, "overlay")
    if scaled is not None:
        _launch("overlay_scaled", frames_u8, frames_u8.data_ptr(), logits.data_ptr(), n, h, w, hn, wn, 1 if mirror else 0, mode,
                channel, alpha, out.data_ptr(), nbytes=(6.0 if overlay else 1.0) * n * h * w + 4.0 * n * hn * wn)
        return out
    _launch("overlay", frames_u8, frames_u8.data_ptr(), logits.data_ptr(), n, h, w, 1 if mirror else 0, mode, channel, alpha,
            out.data_ptr(), nbytes=(10.0 if overlay else 5.0) * n * h * w)
    return out


# edge-aware upsampling: the guided filter on the frame (util/guided_upsample.py states both)
GUIDED_MAX_RADIUS = limits.GUIDED_MAX_RADIUS
GUIDED_EPS_RANGE = limits.GUIDED_EPS_RANGE
GUIDED_MAX_CLIP = limits.GUIDED_MAX_CLIP
_F64 = torch.float64


def guided_params(radius, eps, clip, what: str = "guided_coefficients") -> Tuple[int, float, float]:
    """The filter's three parameters, checked against the ranges the kernel and the numpy definition take."""
    return (limits.check_int(what, "radius", radius, 1, GUIDED_MAX_RADIUS),
            limits.check_real(what, "eps", eps, *GUIDED_EPS_RANGE),
            limits.check_real(what, "clip", clip, 0.0, GUIDED_MAX_CLIP, lo_open=True))


def guided_coefficients(image: torch.Tensor, logits: torch.Tensor, radius: int = 4, eps: float = 400.0, clip: float = 6.0,
                        out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fosvos_guided_coefficients: the net's input fp32 [N,3,Hn,Wn] (what ``frame_prep`` made) and its logits fp32 [N,1,Hn,Wn]
    -> fp64 [N,2,Hn,Wn], the smoothed coefficients [abar, bbar] of the guided filter whose guide is the sum of the image's
    planes and whose target is the logits clipped to ``[-clip, clip]`` (util/guided_upsample.coefficients, bit for bit).  Two
    launches on the current stream, no synchronisation; the unsmoothed maps live in the stream's workspace."""
    _need(image, _F32, "guided_coefficients image", ValueError)
    if image.dim() != 4 or image.shape[1] != 3 or image.numel() == 0:
        raise ValueError(f"guided_coefficients: image must be a non-empty [N,3,Hn,Wn], got {tuple(image.shape)}")
    n, hn, wn = int(image.shape[0]), int(image.shape[2]), int(image.shape[3])
    if hn > MAX_FRAME_SIDE or wn > MAX_FRAME_SIDE:
        raise ValueError(f"guided_coefficients: maps may have sides of up to {MAX_FRAME_SIDE}, got {(hn, wn)}")
    _need(logits, _F32, "guided_coefficients logits", ValueError)
    if tuple(logits.shape) != (n, 1, hn, wn):
        raise ValueError(f"guided_coefficients: logits must be {(n, 1, hn, wn)}, got {tuple(logits.shape)}")
    _same_device("guided_coefficients", image, logits)
    radius, eps, clip = guided_params(radius, eps, clip)
    out = _out_like(out, (n, 2, hn, wn), _F64, image, "guided_coefficients")
    ws, wsn = _WS.get(int(lib().fosvos_guided_coefficients_workspace_bytes(n, hn, wn)), image.device)
    _launch("guided_coefficients", image, image.data_ptr(), logits.data_ptr(), n, hn, wn, radius, eps, clip, out.data_ptr(), ws, wsn,
            nbytes=(16.0 + 3 * 16.0) * n * hn * wn)
    return out


def overlay_guided(frames_u8: torch.Tensor, coeff: torch.Tensor, mirror: bool = False, boolean_mask: bool = True,
                   color: str = 'r', alpha: float = 1.0, overlay: bool = True, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fosvos_overlay_guided: ``overlay(net_size=)`` with the refined logit ``A I + Bv`` in place of the interpolated one: the
    coefficients fp64 [N,2,Hn,Wn] (``guided_coefficients``) are interpolated up to the frames' size inside the launch and
    applied to every (mirrored) frame pixel's own bytes (util/guided_upsample.py states the bytes).  The net's size is the
    coefficients', no larger than the frames; the mask of ``overlay=False`` is the mirrored picture's with ``mirror``.  One
    launch, no synchronisation."""
    n, h, w = _frame_shape(frames_u8, "overlay_guided")
    _need(coeff, _F64, "overlay_guided coeff", ValueError)
    if coeff.dim() != 4 or coeff.shape[0] != n or coeff.shape[1] != 2 or coeff.numel() == 0:
        raise ValueError(f"overlay_guided: coeff must be a non-empty {(n, 2, 'Hn', 'Wn')}, got {tuple(coeff.shape)}")
    hn, wn = _roi_net_size((int(coeff.shape[2]), int(coeff.shape[3])), h, w, "overlay_guided")
    _same_device("overlay_guided", frames_u8, coeff)
    channel, alpha, mode = _paint("overlay_guided", color, alpha, overlay, boolean_mask)
    out = _out_like(out, (n, h, w, 3) if overlay else (n, h, w), torch.uint8, frames_u8, "overlay_guided")
    _launch("overlay_guided", frames_u8, frames_u8.data_ptr(), coeff.data_ptr(), n, h, w, hn, wn, 1 if mirror else 0, mode, channel,
            alpha, _mean_bgr(), out.data_ptr(), nbytes=(6.0 if overlay else 4.0) * n * h * w + 16.0 * n * hn * wn)
    return out


# following the object: the net on a window of the frame (util/frame_roi.py states all three)
ROI_MAX_LEVELS = limits.ROI_MAX_LEVELS
ROI_MAX_PAD = limits.ROI_MAX_PAD
ROI_MAX_MARGIN = limits.ROI_MAX_MARGIN


def _roi_net_size(net_size, h: int, w: int, what: str) -> Tuple[int, int]:
    """``net_size`` of the window ops: mandatory, ``_net_size``'s rules, and the frames' own size is a size like any other
    (a ladder of one level)."""
    if net_size is None:
        raise ValueError(f"{what}: net_size=(Hn, Wn) is needed: a window is scaled to the net's size")
    return _net_size(net_size, h, w, what) or (h, w)


def _windows(windows: torch.Tensor, n: int, like: torch.Tensor, what: str) -> torch.Tensor:
    _need(windows, torch.int32, f"{what} windows", ValueError)
    if tuple(windows.shape) != (n, 4):
        raise ValueError(f"{what}: windows must be int32 {(n, 4)} = (y0, x0, Hw, Ww) a frame, got {tuple(windows.shape)}")
    _same_device(what, like, windows)
    return windows


def roi_margin_permille(margin, what: str = "window_next") -> int:
    """``margin`` (a finite number in [0, 4], a share of the box's longer side) as the integer the kernel pads with."""
    return int(round(1000 * limits.check_real(what, "margin", margin, 0.0, ROI_MAX_MARGIN)))


def frame_prep_window(frames_u8: torch.Tensor, windows: torch.Tensor, net_size: Tuple[int, int], mirror: bool = False,
                      out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fosvos_frame_prep_window: raw frames uint8 [N,H,W,3] and one window int32 (y0, x0, Hw, Ww) a frame, in DEVICE memory
    [N,4] -> fp32 [N,3,Hn,Wn], the window of the (mirrored) frame area-averaged to the net's size less the mean
    (util/frame_roi.prepare_frame_window, bit for bit).  A window that is not valid is read as the whole frame.  One launch on
    the current stream, no synchronisation: the host never sees the windows."""
    n, h, w = _frame_shape(frames_u8, "frame_prep_window")
    hn, wn = _roi_net_size(net_size, h, w, "frame_prep_window")
    _windows(windows, n, frames_u8, "frame_prep_window")
    out = _out_like(out, (n, 3, hn, wn), _F32, frames_u8, "frame_prep_window")
    _launch("frame_prep_window", frames_u8, frames_u8.data_ptr(), windows.data_ptr(), n, h, w, hn, wn, 1 if mirror else 0,
            _mean_bgr(), out.data_ptr(), nbytes=3.0 * n * h * w + 12.0 * n * hn * wn)  # (at the most: the whole-frame window)
    return out


def overlay_window(frames_u8: torch.Tensor, logits: torch.Tensor, windows: torch.Tensor, mirror: bool = False,
                   boolean_mask: bool = True, color: str = 'r', alpha: float = 1.0, overlay: bool = True,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fosvos_overlay_window: ``overlay(net_size=)`` with the logits fp32 [N,1,Hn,Wn] painted into the frames' windows (int32
    [N,4] in device memory): interpolated up to the window's size inside it, nothing is object outside it
    (util/frame_roi.py states the bytes).  The net's size is the logits'.  One launch, no synchronisation."""
    n, h, w = _frame_shape(frames_u8, "overlay_window")
    _need(logits, _F32, "overlay_window logits", ValueError)
    if logits.dim() != 4 or logits.shape[0] != n or logits.shape[1] != 1 or logits.numel() == 0:
        raise ValueError(f"overlay_window: logits must be a non-empty {(n, 1, 'Hn', 'Wn')}, got {tuple(logits.shape)}")
    hn, wn = _roi_net_size((int(logits.shape[2]), int(logits.shape[3])), h, w, "overlay_window")
    _same_device("overlay_window", frames_u8, logits)
    _windows(windows, n, frames_u8, "overlay_window")
    channel, alpha, mode = _paint("overlay_window", color, alpha, overlay, boolean_mask)
    out = _out_like(out, (n, h, w, 3) if overlay else (n, h, w), torch.uint8, frames_u8, "overlay_window")
    _launch("overlay_window", frames_u8, frames_u8.data_ptr(), logits.data_ptr(), windows.data_ptr(), n, h, w, hn, wn,
            1 if mirror else 0, mode, channel, alpha, out.data_ptr(),
            nbytes=(6.0 if overlay else 1.0) * n * h * w + 4.0 * n * hn * wn)
    return out


def window_next(logits: torch.Tensor, windows: torch.Tensor, frame_size: Tuple[int, int], levels: int = 8,
                margin: float = 0.25, min_pad: int = 16, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fosvos_window_next: the logits fp32 [N,1,Hn,Wn] of N frames and the windows int32 [N,4] they were made through -> the
    windows of the next frames, int32 [N,4] (``out`` may be ``windows``): the box of ``logits >= 0``, padded by ``min_pad +
    margin * its longer side``, in the smallest of the ``levels + 1`` sizes between the net's and the frame's that holds it
    (util/frame_roi.next_window, exactly); no object: the whole frame.  Two launches, no synchronisation."""
    _need(logits, _F32, "window_next logits", ValueError)
    n, hn, wn = _logit_shape(logits, "window_next")
    hf, wf = limits.check_pair("window_next", "frame_size", frame_size, "(Hf, Wf)")
    _roi_net_size((hn, wn), hf, wf, "window_next")
    _windows(windows, n, logits, "window_next")
    limits.check_int("window_next", "levels", levels, 1, ROI_MAX_LEVELS)
    limits.check_int("window_next", "min_pad", min_pad, 0, ROI_MAX_PAD)
    permille = roi_margin_permille(margin)
    out = _out_like(out, (n, 4), torch.int32, logits, "window_next")
    ws, wsn = _WS.get(int(lib().fosvos_window_next_workspace_bytes(n)), logits.device)
    _launch("window_next", logits, logits.data_ptr(), windows.data_ptr(), n, hf, wf, hn, wn, levels, permille, min_pad,
            out.data_ptr(), ws, wsn, nbytes=4.0 * n * hn * wn)
    return out


def overlay_objects(frames_u8: torch.Tensor, logits: Sequence[torch.Tensor], mirror: bool = False, overlay: bool = True,
                    palette: Optional[torch.Tensor] = None, alpha: float = 0.5, out: Optional[torch.Tensor] = None,
                    net_size: Optional[Tuple[int, int]] = None) -> torch.Tensor:
    """fosvos_overlay_objects: raw frames uint8 [N,H,W,3] and the logits fp32 [N,1,H,W] that K per-object nets (1 <= K <= 16)
    made of them (of the mirrored frames, with ``mirror``) -> uint8 [N,H,W,3]: the (mirrored) frames with every pixel that
    ``merge_objects`` would label k > 0 blended towards ``palette[k]``, ``b + alpha * (colour - b)`` rounded half up, in all
    three channels; label 0 keeps its bytes.  ``palette``: uint8 [256,3] RGB on the device, None = ``default_palette``;
    ``alpha`` a finite number in [0, 1] (this overlay blends; ``overlay`` adds to one channel and takes more).
    ``overlay=False``: the label map uint8 [N,H,W] (``merge_objects`` itself).  util/object_overlay.py states the bytes.
    The K pointers travel by value, no label map is written in between; ``out`` may be a view of a caller's buffer at any
    byte offset.  One launch on the current stream, no synchronisation.

    ``net_size=(Hn, Wn)`` (no larger than the frames): fosvos_overlay_objects_scaled, the logits are [N,1,Hn,Wn] and every
    map is interpolated up to the frames' size inside the launch, in both forms.  The frames' own size is the launch above."""
    n, h, w = _frame_shape(frames_u8, "overlay_objects")
    scaled = _net_size(net_size, h, w, "overlay_objects")
    hn, wn = scaled if scaled is not None else (h, w)
    logits, _, table = _logit_table(logits, "overlay_objects", (n, 1, hn, wn))
    alpha = limits.check_real("overlay_objects", "alpha", float(alpha), 0.0, 1.0)
    palette = _palette(palette, frames_u8.device, "overlay_objects")
    out = _out_like(out, (n, h, w, 3) if overlay else (n, h, w), torch.uint8, frames_u8, "overlay_objects")
    _same_device("overlay_objects", frames_u8, *logits)
    if not overlay and scaled is None:
        return merge_objects(logits, out=out)
    k = len(logits)
    if scaled is not None:
        _launch("overlay_objects_scaled", frames_u8, frames_u8.data_ptr(), table, k, n, h, w, hn, wn, 1 if mirror else 0,
                0 if overlay else 1, palette.data_ptr(), alpha, out.data_ptr(),
                nbytes=(6.0 if overlay else 1.0) * n * h * w + 4.0 * k * n * hn * wn)
        return out
    _launch("overlay_objects", frames_u8, frames_u8.data_ptr(), table, k, n, h, w, 1 if mirror else 0, palette.data_ptr(), alpha,
            out.data_ptr(), nbytes=(4.0 * k + 6.0) * n * h * w)
    return out
