"""Streaming inference: raw uint8 camera frames through a net, the frame that is shown back, ``depth`` frames in flight.

What the reference does per frame on the host (src/run_webcam.py:81-133, ``apply_network``) happens on the device here:
``ops.frame_prep`` in front of the net and ``ops.overlay`` behind it (csrc/stream.hip; util/frame_overlay.py states both).
Only the raw bytes cross the bus, 3 B a pixel each way (1 B back without overlay).

A segmenter owns ``depth`` SLOTS; a slot is everything one frame in flight needs, allocated once:

    pinned host frame -> device frame (uint8) -> device image (fp32) -> [net] -> device output (uint8) -> pinned host output

and two events.  Per frame:

    upload stream    H2D frame, record slot.moved
    net's stream     wait slot.moved; frame_prep, net.forward, overlay; record slot.computed
    download stream  wait slot.computed; D2H output, record slot.moved

``slot.moved`` marks the slot's last copy: first the upload (the net's stream waits for it as soon as it is recorded),
then the download, which is the one event the host ever waits on - when it retires the slot.  Nothing synchronises a stream
or the device per frame.  A slot is reused only after it was retired, so its upload cannot overtake the overlay that still
reads the previous frame.  The net's stream is the current stream at ``submit``; the two copy streams are the segmenter's
own (two, so that the upload of frame k+1 does not queue behind the download of frame k, which waits for the net).

``encode='jpeg'`` (opt-in) adds ``ops.jpeg_encode`` behind the overlay (csrc/jpeg.hip; util/jpeg_layout.py states the file)
and the slot ends in a device file buffer with its length in front:

    ... -> device output (uint8) -> device [length | file, capacity bytes] -> pinned host [length | first ``budget`` bytes]

The download is ONE copy of the length and the first ``budget`` bytes of the file (a constructor-time constant, by default
a quarter of the raw output), so the host still waits on ``slot.moved`` alone; only a frame whose file is longer fetches the
rest with a second copy, on a stream of its own, when it is retired.  ``subsampling='4:2:0'`` chooses the encoder's 4:2:0
form (smaller files; the default budget stays the quarter).  ``encode=None`` is the object described above.

``net_size=(Hn, Wn)`` (opt-in, no larger than the frame) runs the net at a size of its own: the slot's image is [1,3,Hn,Wn],
``ops.frame_prep`` area-averages the frame down to it inside its launch and ``ops.overlay`` interpolates the logits back up
inside its own (csrc/stream.hip; util/frame_resample.py states both).  Everything else - the uploads, the output, the JPEG
capacity and budget, the downloads - stays at the frame's size.  ``None`` or the frame's own size is the object described above.

``clean=CleanOptions(...)`` (opt-in, ``fosvos_hip.options``) puts ONE ``ops.clean_components`` between the net and the overlay,
in place on the net's logits (csrc/components.hip; util/mask_components.py states the rules): connected components of the mask
that are too small, not the largest, or - ``temporal_radius`` - too far from what the frame before kept become background.
With ``net_size`` it runs at the net's size, the radius in net pixels.  The temporal gate needs one more device buffer, the
segmenter's seed: the kept mask of the last frame computed, written by that frame's call and read by the next one's;
``seed(mask)`` sets it by hand.  ``None`` is the object described above.

``motion=MotionOptions(...)`` (opt-in, with ``clean.temporal_radius``; ``fosvos_hip.options``) makes that gate follow the
picture: per frame ONE ``ops.motion_luma`` of the image the net saw (with ``net_size`` the net's map, where the seed lives) and -
once a frame before exists - ONE ``ops.motion_estimate`` against its luma plane and ONE ``ops.motion_warp`` of the seed into a
second buffer, which the clean call reads in place of the seed (csrc/motion.hip; util/block_motion.py states all three, and its
``track`` the whole chain).  Two luma planes, the field, the cost and the warped seed are allocated once; which plane is the
previous one is host state that changes in submit order, as the launches do.  ``seed(mask)`` drops the previous plane: a
hand-set seed belongs to the next submitted frame and is used unwarped.  ``None`` is the object described above.

``ObjectSegmenter`` (opt-in) is the same object for several objects a frame: K per-object nets run on the slot's one image and
ONE ``ops.overlay_objects`` merges their logits and paints the palette overlay (csrc/stream.hip; util/object_overlay.py
states the bytes).  Its label-map form can end in a palette PNG (``encode='png'``, ``ops.png_encode_indexed``), which leaves the
slot exactly like the JPEG: ``[length | file]`` on the device, ``[length | first budget bytes]`` on the host.  Only the
compute step differs from ``FrameSegmenter``, whose launches, order and bytes are what they were.

``roi=RoiOptions(...)`` (opt-in, with ``net_size``; ``fosvos_hip.options``) follows the object: the net sees a WINDOW of the
frame around the last mask, ``ops.frame_prep_window`` area-averages that window to the net's size, ``ops.overlay_window`` paints
the logits back into it, and ``ops.window_next`` makes the next frame's window of this frame's (cleaned) logits (csrc/stream.hip;
util/frame_roi.py states all three).  The window never leaves the device: the segmenter's ``_window`` (int32 [1,4]) is written
by frame t's ``window_next`` and copied into frame t + 1's slot on the one net's stream, in submit order - the hand-over of
the clean seed, no event and no host read of its own.  ``seed_window(mask)`` sets it from an annotation.  ``None`` is the object
described above.

``refine=RefineOptions(...)`` (opt-in, with or without ``net_size``; ``fosvos_hip.options``) upsamples by the frame's own edges:
``ops.guided_coefficients`` fits, at the net's size, a linear model between the (cleaned) logits and the image the net saw and
smooths it into the slot's coefficient maps (fp64 [1,2,Hn,Wn]), and ``ops.overlay_guided`` - in place of ``ops.overlay`` -
interpolates the coefficients, not the logits, and applies them to every frame pixel's own bytes (csrc/guided.hip,
csrc/stream.hip; util/guided_upsample.py states both).  The slot's image is read after the net: both nets' passes take their
input const.  ``None`` is the object described above.

Not thread-safe: one host thread drives a segmenter.
"""
from __future__ import annotations

from collections import deque
from contextlib import contextmanager
from typing import Deque, Iterable, Iterator, List, Optional, Tuple, Union

import numpy as np
import torch

from . import limits, ops
from .options import CleanOptions, MotionOptions, RefineOptions, RoiOptions


_HEAD = 8  # bytes in front of a slot's file: the int32 length, padded so that the file starts 8-byte aligned


class _Slot:
    def __init__(self, h: int, w: int, out_shape, device: torch.device, capacity: int = 0, budget: int = 0,
                 net_size=None, roi: bool = False, refine: bool = False) -> None:
        self.host_in = torch.empty((1, h, w, 3), dtype=torch.uint8, pin_memory=True)
        self.host_in_np = self.host_in.numpy()
        self.frame = torch.empty((1, h, w, 3), dtype=torch.uint8, device=device)
        self.image = torch.empty((1, 3) + tuple(net_size or (h, w)), dtype=torch.float32, device=device)
        self.out = torch.empty(out_shape, dtype=torch.uint8, device=device)
        self.window = torch.empty((1, 4), dtype=torch.int32, device=device) if roi else None  # the one this frame is seen through
        # refine: the smoothed coefficient maps of this frame (the unsmoothed ones live in the stream's workspace)
        self.coeff = torch.empty((1, 2) + tuple(net_size or (h, w)), dtype=torch.float64, device=device) if refine else None
        if capacity:
            self.store = torch.empty((_HEAD + capacity,), dtype=torch.uint8, device=device)
            self.length = self.store[:4].view(torch.int32)
            self.file = self.store[_HEAD:].view(1, capacity)
            self.host_out = torch.empty((_HEAD + budget,), dtype=torch.uint8, pin_memory=True)
        else:
            self.host_out = torch.empty(out_shape, dtype=torch.uint8, pin_memory=True)
        self.host_out_np = self.host_out.numpy()
        self.moved = torch.cuda.Event()
        self.computed = torch.cuda.Event()


class FrameSegmenter:
    """``FrameSegmenter(net, height, width, net_size=None)``: ``net`` is any module of this project (OSVOS_VGG, OSVOS_RESNET, a pruned
    whole-module pickle) on a GPU; the segmenter calls ``net.forward(x)[-1]`` under ``no_grad`` with
    ``net.compute_side_outputs = False`` for the call.

    submit(frame)    queue one uint8 [H,W,3] BGR frame - a numpy array, or a tensor already on the net's device, made on the
                     current stream (``ops.jpeg_decode``'s output: no upload); blocks only when all ``depth`` slots are in flight (it then retires
                     the oldest and keeps its output for ``result``)
    result()         the oldest frame's output as an array of its own: uint8 [H,W,3], or [H,W] with ``overlay=False``;
                     with ``encode='jpeg'`` the same picture as ``bytes``, a complete .jpg file of quality ``quality``
    segment(frames)  generator: outputs in input order, ``depth`` frames in flight
    apply(frame)     one frame, synchronously
    seed_window(mask)  with ``roi``: the window of the next submitted frame from an annotation (uint8 or bool, the frame's size,
                     in the frame's own coordinates; non-zero = object); never called, the first frame is seen whole
    last_window()    with ``roi``: the window the next frame will use, as a tuple (y0, x0, Hw, Ww); synchronises - for logs and
                     tests
    seed(mask)       with ``clean.temporal_radius``: the mask (uint8 or bool, the frame's size or the net's; non-zero = object)
                     the next submitted frame is gated by, e.g. the annotation the net was fine-tuned on; never called, the
                     first frame is not gated
    close()          wait for what is in flight and release every buffer
    """

    clean: Optional[CleanOptions] = None  # (ObjectSegmenter has none)
    roi: Optional[RoiOptions] = None      # (likewise)
    refine: Optional[RefineOptions] = None  # (likewise)
    motion: Optional[MotionOptions] = None  # (likewise)
    _seed = None
    _luma = None
    _luma_prev = None  # the index of the plane of self._luma that holds the frame before, or None
    _window = None

    def __init__(self, net, height: int, width: int, depth: int = 2, mirror: bool = True, overlay: bool = True,
                 boolean_mask: bool = True, color: str = 'r', alpha: float = 1.0, encode: Optional[str] = None,
                 quality: int = 90, subsampling: str = '4:4:4', budget: Optional[int] = None,
                 net_size: Optional[Tuple[int, int]] = None, clean: Optional[CleanOptions] = None,
                 roi: Optional[RoiOptions] = None, refine: Optional[RefineOptions] = None,
                 motion: Optional[MotionOptions] = None) -> None:
        from util import frame_overlay
        self._set_geometry(height, width, depth, net_size)
        if clean is not None and not isinstance(clean, CleanOptions):
            raise ValueError(f"{self._who}: clean must be a fosvos_hip.options.CleanOptions or None, got {type(clean).__name__}")
        self.clean = clean
        if roi is not None:
            if not isinstance(roi, RoiOptions):
                raise ValueError(f"{self._who}: roi must be a fosvos_hip.options.RoiOptions or None, got {type(roi).__name__}")
            if net_size is None:
                raise ValueError(f"{self._who}: roi needs net_size=(Hn, Wn): a window of the frame is scaled to the net's size, "
                                 "and without one the net sees the whole frame as it is")
            if clean is not None and clean.chain:
                raise ValueError(f"{self._who}: roi with clean.temporal_radius is not built: the chained seed lives on the "
                                 "net's map, whose coordinates move from frame to frame with the window")
        self.roi = roi
        if refine is not None:
            if not isinstance(refine, RefineOptions):
                raise ValueError(f"{self._who}: refine must be a fosvos_hip.options.RefineOptions or None, got "
                                 f"{type(refine).__name__}")
            if roi is not None:
                raise ValueError(f"{self._who}: refine with roi is not built: the filter's guide is the image the net saw, a "
                                 "window of the frame, and the guide of a window is not built")
        self.refine = refine
        if motion is not None:
            if not isinstance(motion, MotionOptions):
                raise ValueError(f"{self._who}: motion must be a fosvos_hip.options.MotionOptions or None, got "
                                 f"{type(motion).__name__}")
            if clean is None or not clean.chain:
                raise ValueError(f"{self._who}: motion carries the seed of the temporal gate along the picture's motion: it "
                                 "needs clean=CleanOptions(temporal_radius=...)")
        self.motion = motion
        frame_overlay.check_color(color)
        self.mirror, self.overlay, self.boolean_mask = bool(mirror), bool(overlay), bool(boolean_mask)
        self.color, self.alpha = color, frame_overlay.check_alpha(alpha)
        self.net = net
        self.device = self._device_of(net)
        if encode not in (None, 'jpeg'):
            raise ValueError(f"{self._who}: encode must be None or 'jpeg', got {encode!r}")
        self._set_jpeg(encode, quality, subsampling, budget)
        self._open()

    # ---------------------------------------------------------------------------------------------- construction, in steps
    @property
    def _who(self) -> str:
        return type(self).__name__

    def _set_geometry(self, height, width, depth, net_size) -> None:
        self.height, self.width, self.depth = int(height), int(width), int(depth)
        if self.height <= 0 or self.width <= 0 or self.depth <= 0:
            raise ValueError(f"{self._who}: height, width and depth must be positive, got {height}, {width}, {depth}")
        # None where the net runs at the frame's size: the unscaled launches, exactly
        self.net_size = ops._net_size(net_size, self.height, self.width, self._who)

    def _device_of(self, net) -> torch.device:
        param = next(iter(net.parameters()), None)
        if param is None or not param.is_cuda:
            raise RuntimeError(f"{self._who}: the net must live on the GPU (the HIP path has no CPU fallback)")
        return param.device

    def _set_budget(self, budget, default: int) -> None:
        """The download budget of an encoder whose capacity is set: ``default`` bytes where none is given."""
        budget = limits.check_int(self._who, "budget", default if budget is None else budget, 1,
                                  expect="a positive number of bytes")
        self.budget = min(budget, self.capacity)

    def _set_jpeg(self, encode, quality, subsampling, budget) -> None:
        """``encode`` is None or 'jpeg' (``self.overlay`` says how many components the output has)."""
        h, w = self.height, self.width
        self.encode, self.quality = encode, quality
        if subsampling != '4:4:4' and encode != 'jpeg':
            raise ValueError(f"{self._who}: subsampling is the chroma sampling of encode='jpeg'")
        self.subsampling = subsampling if encode else None
        self.capacity = self.budget = 0
        self.second_copies = 0  # frames whose file was longer than the budget
        self.bytes_down = 0     # bytes the downloads moved
        if encode:
            limits.check_int(self._who, "quality", quality, *limits.JPEG_QUALITY)
            limits.check_member(self._who, "subsampling", subsampling, limits.JPEG_SUBSAMPLINGS)
            self.capacity = ops.jpeg_capacity(h, w, 3 if self.overlay else 1, self.subsampling)
            raw = h * w * (3 if self.overlay else 1)
            self._set_budget(budget, max(raw // 4, 1024))
        elif budget is not None:
            raise ValueError(f"{self._who}: budget is the download budget of encode='jpeg'")

    def _open(self) -> None:
        """The streams, the slots and the queues, once everything above is decided."""
        h, w = self.height, self.width
        out_shape = (1, h, w, 3) if self.overlay else (1, h, w)
        self._closed = False
        with torch.cuda.device(self.device):
            self._up = torch.cuda.Stream(device=self.device)
            self._down = torch.cuda.Stream(device=self.device)
            self._rest = torch.cuda.Stream(device=self.device) if self.encode else None  # second copies of long files
            self._free: List[_Slot] = [_Slot(h, w, out_shape, self.device, self.capacity, self.budget, self.net_size,
                                             self.roi is not None, self.refine is not None) for _ in range(self.depth)]
            # roi: the window the next frame is seen through.  The whole frame until a frame or seed_window says otherwise
            self._window = torch.tensor([[0, 0, h, w]], dtype=torch.int32, device=self.device) if self.roi is not None else None
            # the temporal gate's seed: what the last frame computed kept, at the net's size.  Empty = no gate (the rule
            # of an empty seed), so a segmenter nobody seeded starts ungated
            chained = self.clean is not None and self.clean.chain
            self._seed = torch.zeros((1,) + tuple(self.net_size or (h, w)), dtype=torch.uint8, device=self.device) \
                if chained else None
            self._luma = self._luma_prev = None
            if self.motion is not None:
                # the luma planes of the frame before and of this one by turns, the field and cost of the pair, the warped seed
                hn, wn = self.net_size or (h, w)
                hb, wb = -(-hn // self.motion.block), -(-wn // self.motion.block)
                self._luma = torch.empty((2, 1, hn, wn), dtype=torch.uint8, device=self.device)
                self._field = torch.empty((1, hb, wb, 2), dtype=torch.int8, device=self.device)
                self._cost = torch.empty((1, hb, wb), dtype=torch.int32, device=self.device)
                self._warped = torch.empty((1, hn, wn), dtype=torch.uint8, device=self.device)
        self._flight: Deque[_Slot] = deque()     # submitted, oldest first
        self._ready: Deque[Union[np.ndarray, bytes]] = deque()  # retired by a submit that needed the slot, not yet asked for

    # ---------------------------------------------------------------------------------------------- checks
    def _check_open(self) -> None:
        if self._closed:
            raise RuntimeError(f"{self._who}: closed")

    def _check_frame(self, frame):
        if isinstance(frame, torch.Tensor):  # a frame that is on the device already (ops.jpeg_decode made it)
            if frame.dtype != torch.uint8 or frame.device != self.device or not frame.is_contiguous():
                raise ValueError(f"{self._who}: a device frame must be a contiguous uint8 tensor on {self.device}, got "
                                 f"{frame.dtype} on {frame.device}")
            if tuple(frame.shape) != (self.height, self.width, 3):
                raise ValueError(f"{self._who}: a frame must be {(self.height, self.width, 3)}, got {tuple(frame.shape)}")
            return frame
        if not isinstance(frame, np.ndarray) or frame.dtype != np.uint8:
            raise ValueError(f"{self._who}: a frame must be a uint8 numpy array, got {getattr(frame, 'dtype', type(frame))}")
        if frame.shape != (self.height, self.width, 3):
            raise ValueError(f"{self._who}: a frame must be {(self.height, self.width, 3)}, got {frame.shape}")
        return frame

    @property
    def pending(self) -> int:
        """Frames submitted whose output has not been returned yet."""
        return len(self._flight) + len(self._ready)

    # ---------------------------------------------------------------------------------------------- the pipeline
    def _retire(self) -> Union[np.ndarray, bytes]:
        slot = self._flight[0]
        slot.moved.synchronize()  # the download of this slot, nothing else
        if self.encode:
            length = int(slot.host_out_np[:4].view(np.int32)[0])
            if not 0 < length <= self.capacity:
                raise RuntimeError(f"{self._who}: the encoder reported a file of {length} bytes (capacity {self.capacity})")
            out = slot.host_out_np[_HEAD:_HEAD + min(length, self.budget)].tobytes()
            self.bytes_down += _HEAD + self.budget
            if length > self.budget:  # the slot's work is done: nothing to wait for but the copy itself
                with torch.cuda.stream(self._rest):
                    out += slot.file[0, self.budget:length].cpu().numpy().tobytes()
                self.second_copies += 1
                self.bytes_down += length - self.budget
        else:
            out = np.array(slot.host_out_np[0], copy=True)
        self._flight.popleft()
        self._free.append(slot)
        return out

    @staticmethod
    @contextmanager
    def _last_output_only(net):
        """``net.compute_side_outputs = False`` for the calls inside, and whatever it was (or was not) afterwards."""
        had, old = hasattr(net, 'compute_side_outputs'), getattr(net, 'compute_side_outputs', None)
        net.compute_side_outputs = False
        try:
            yield
        finally:
            if had:
                net.compute_side_outputs = old
            else:
                del net.compute_side_outputs

    def _compute(self, slot: _Slot) -> None:
        """What a frame needs on the net's stream, from ``slot.frame`` to ``slot.out`` (and the slot's file)."""
        roi = self.roi
        with self._last_output_only(self.net), torch.no_grad():
            if roi is not None:
                # the window this frame is seen through: what the frame before left in self._window, kept in the slot because
                # the overlay needs it after window_next has overwritten self._window.  All of it on the one net's stream
                slot.window.copy_(self._window, non_blocking=True)
                ops.frame_prep_window(slot.frame, slot.window, self._roi_size, self.mirror, out=slot.image)
            else:
                ops.frame_prep(slot.frame, self.mirror, out=slot.image, net_size=self.net_size)
            logits = self.net.forward(slot.image)[-1]
            if self.clean is not None:
                # in place on the net's output.  The seed is read AND written by this one call (chain over one frame: gated
                # by self._seed, the kept mask goes back into it).  Every slot's compute is issued on the one net's
                # stream in submit order, so frame t finds frame t - 1's kept mask there without an event of its own
                c = self.clean
                logits = logits.contiguous()
                seed = self._seed
                if self.motion is not None:
                    # the seed in this frame's coordinates: the luma of what the net saw, its motion against the frame
                    # before, the seed warped along it into a buffer of its own.  The planes change roles in submit order
                    now = 0 if self._luma_prev is None else 1 - self._luma_prev
                    ops.motion_luma(slot.image, out=self._luma[now])
                    if self._luma_prev is not None:
                        ops.motion_estimate(self._luma[self._luma_prev], self._luma[now], self.motion, field=self._field,
                                            cost=self._cost)
                        seed = ops.motion_warp(self._seed, self._field, self.motion.block, out=self._warped)
                    self._luma_prev = now
                ops.clean_components(logits, seed, 0 if c.temporal_radius is None else c.temporal_radius, c.min_area,
                                     c.largest, chain=c.chain, fill=c.fill, out=logits,
                                     kept=None if self._seed is None else self._seed)
            if roi is not None:
                logits = logits.contiguous()
                ops.window_next(logits, slot.window, (self.height, self.width), roi.levels, roi.margin, roi.min_pad,
                                out=self._window)
                ops.overlay_window(slot.frame, logits, slot.window, self.mirror, self.boolean_mask, self.color, self.alpha,
                                   self.overlay, out=slot.out)
            elif self.refine is not None:
                f = self.refine
                ops.guided_coefficients(slot.image, logits.contiguous(), f.radius, f.eps, f.clip, out=slot.coeff)
                ops.overlay_guided(slot.frame, slot.coeff, self.mirror, self.boolean_mask, self.color, self.alpha, self.overlay,
                                   out=slot.out)
            else:
                ops.overlay(slot.frame, logits, self.mirror, self.boolean_mask, self.color, self.alpha, self.overlay,
                            out=slot.out, net_size=self.net_size)
            if self.encode:
                ops.jpeg_encode(slot.out, self.quality, out=slot.file, lengths=slot.length, subsampling=self.subsampling)

    def _enqueue(self, slot: _Slot, main: torch.cuda.Stream, device_frame: Optional[torch.Tensor] = None) -> None:
        if device_frame is not None:  # made on the caller's stream, which is `main`: a copy in stream order, no upload
            slot.frame[0].copy_(device_frame, non_blocking=True)
        else:
            with torch.cuda.stream(self._up):
                slot.frame.copy_(slot.host_in, non_blocking=True)
                slot.moved.record(self._up)
            main.wait_event(slot.moved)
        self._compute(slot)
        slot.computed.record(main)
        with torch.cuda.stream(self._down):
            self._down.wait_event(slot.computed)
            if self.encode:
                slot.host_out.copy_(slot.store[:_HEAD + self.budget], non_blocking=True)
            else:
                slot.host_out.copy_(slot.out, non_blocking=True)
            slot.moved.record(self._down)

    def submit(self, frame: np.ndarray) -> None:
        self._check_open()
        frame = self._check_frame(frame)  # raises before anything is queued
        if not self._free:
            self._ready.append(self._retire())
        slot = self._free.pop()
        with torch.cuda.device(self.device):
            main = torch.cuda.current_stream(self.device)
            try:
                if isinstance(frame, torch.Tensor):
                    self._enqueue(slot, main, device_frame=frame)
                else:
                    np.copyto(slot.host_in_np[0], frame)
                    self._enqueue(slot, main)
            except BaseException:
                # never half-queued: whatever part of the frame was queued runs out, then the slot is free again
                try:
                    for st in (self._up, main, self._down):
                        st.synchronize()
                    self._free.append(slot)
                    self._luma_prev = None  # (motion) whichever plane the frame reached: the next frame's seed is not warped
                except Exception:
                    self.close()
                raise
        self._flight.append(slot)

    def result(self) -> np.ndarray:
        self._check_open()
        if self._ready:
            return self._ready.popleft()
        if not self._flight:
            raise RuntimeError(f"{self._who}.result: no frame is in flight")
        return self._retire()

    def segment(self, frames: Iterable[np.ndarray]) -> Iterator[np.ndarray]:
        self._check_open()
        if self.pending:
            raise RuntimeError(f"{self._who}.segment: fetch the results of the frames already submitted first")
        for frame in frames:
            if len(self._flight) == self.depth:
                yield self.result()
            self.submit(frame)
        while self.pending:
            yield self.result()

    def apply(self, frame: np.ndarray) -> np.ndarray:
        self._check_open()
        if self.pending:
            raise RuntimeError(f"{self._who}.apply: fetch the results of the frames already submitted first")
        self.submit(frame)
        return self.result()

    def seed(self, mask) -> None:
        """Set the temporal gate's seed (see the class)."""
        self._check_open()
        if self._seed is None:
            raise RuntimeError(f"{self._who}.seed: there is no temporal gate (clean=CleanOptions(temporal_radius=...))")
        if isinstance(mask, torch.Tensor):
            mask = mask.detach().cpu().numpy()
        mask = np.asarray(mask)
        if mask.dtype not in (np.uint8, np.bool_) or mask.ndim != 2:
            raise ValueError(f"{self._who}.seed: a uint8 or bool [H,W] mask, got {mask.dtype} {mask.shape}")
        hn, wn = self._seed.shape[1:]
        if mask.shape == (self.height, self.width) and (hn, wn) != (self.height, self.width):
            # to the net's size: a net pixel is set when a frame pixel it averages is (util/frame_resample.box_weights)
            from util import frame_resample
            rows = frame_resample.box_weights(self.height, hn) > 0
            cols = frame_resample.box_weights(self.width, wn) > 0
            mask = (rows.astype(np.int64) @ (mask != 0).astype(np.int64) @ cols.T.astype(np.int64)) > 0
        if mask.shape != (hn, wn):
            raise ValueError(f"{self._who}.seed: the mask must be {(self.height, self.width)} or the net's {(hn, wn)}, "
                             f"got {mask.shape}")
        if self.mirror:  # the mask is in the frame's coordinates, the net sees the mirrored frame
            mask = mask[:, ::-1]
        host = torch.from_numpy(np.ascontiguousarray((mask != 0).astype(np.uint8)))[None]
        with torch.cuda.device(self.device):
            self._seed.copy_(host)  # on the current stream, the net's: ordered with the frames before and behind
        self._luma_prev = None  # (motion) the mask belongs to the next submitted frame: used unwarped

    @property
    def _roi_size(self) -> Tuple[int, int]:
        """The net's size as the window ops take it: the frame's own is a size like any other there."""
        return self.net_size or (self.height, self.width)

    def seed_window(self, mask) -> None:
        """Set the window of the next submitted frame from an annotation (see the class)."""
        self._check_open()
        if self.roi is None:
            raise RuntimeError(f"{self._who}.seed_window: there is no window to seed (roi=RoiOptions(...))")
        if isinstance(mask, torch.Tensor):
            mask = mask.detach().cpu().numpy()
        mask = np.asarray(mask)
        if mask.dtype not in (np.uint8, np.bool_) or mask.shape != (self.height, self.width):
            raise ValueError(f"{self._who}.seed_window: a uint8 or bool mask of {(self.height, self.width)}, got {mask.dtype} "
                             f"{mask.shape}")
        from util import frame_roi
        if self.mirror:  # the mask is in the frame's coordinates, the windows in those of the mirrored picture
            mask = mask[:, ::-1]
        hn, wn = self._roi_size
        window = frame_roi.window_of_mask(mask, hn, wn, self.roi.levels, self.roi.margin_permille, self.roi.min_pad)
        host = torch.tensor([window], dtype=torch.int32)
        with torch.cuda.device(self.device):
            self._window.copy_(host)  # on the current stream, the net's: ordered with the frames before and behind

    def last_window(self) -> Tuple[int, int, int, int]:
        """The window the next frame will use (see the class).  Waits for the frames submitted so far."""
        self._check_open()
        if self.roi is None:
            raise RuntimeError(f"{self._who}.last_window: there is no window (roi=RoiOptions(...))")
        return tuple(int(v) for v in self._window.cpu()[0])

    def close(self) -> None:
        if self._closed:
            return
        self._closed = True
        self._seed = None
        self._window = None
        self._luma = self._luma_prev = None
        self._field = self._cost = self._warped = None
        for slot in self._flight:
            try:
                slot.moved.synchronize()
            except Exception:  # a failed device: the buffers go either way
                pass
        self._flight.clear()
        self._ready.clear()
        self._free = []
        self._up = self._down = self._rest = None
        self.net = None

    def __enter__(self) -> "FrameSegmenter":
        return self

    def __exit__(self, *exc) -> bool:
        self.close()
        return False


class ObjectSegmenter(FrameSegmenter):
    """``ObjectSegmenter(nets, height, width, ...)``: a FrameSegmenter for several objects.  ``nets`` are the 1..16 per-object
    nets of a sequence (``train_online.py --multi-object``: net k - 1 is object k), distinct module objects on one GPU.  The
    slots, events, copy streams, ``submit`` / ``result`` / ``segment`` / ``apply`` / ``close`` / ``pending``, device-frame input
    and failure handling are FrameSegmenter's; per frame the net's stream runs ``ops.frame_prep`` once,
    ``net.forward(image)[-1]`` of every net on that one image, and ONE ``ops.overlay_objects`` (csrc/stream.hip;
    util/object_overlay.py states the bytes): the K logit maps never leave the device and no label map is written in between.

    overlay=True    uint8 [H,W,3]: every labelled pixel blended towards ``palette[label]`` (uint8 [256,3] RGB, a numpy array
                    or a device tensor; None = the DAVIS palette) with ``alpha`` in [0, 1]; ``encode='jpeg'``: the .jpg bytes
    overlay=False   uint8 [H,W], the label map; ``encode='png'``: a palette PNG file of it (``ops.png_encode_indexed`` with
                    the palette and ``huffman``), downloaded as [length | first ``budget`` bytes] like the JPEG: the default
                    budget is a quarter of ``ops.png_indexed_capacity``, at least 1024

    A lossy label map means nothing and the frame's PNG is the host's job, so 'jpeg' goes with the overlay only and 'png'
    with the label map only.
    """

    def __init__(self, nets, height: int, width: int, depth: int = 2, mirror: bool = True, overlay: bool = True,
                 palette=None, alpha: float = 0.5, encode: Optional[str] = None, quality: int = 90,
                 subsampling: str = '4:4:4', budget: Optional[int] = None, huffman: str = 'fixed',
                 net_size: Optional[Tuple[int, int]] = None, clean=None, roi=None, refine=None, motion=None) -> None:
        from util import object_overlay
        if motion is not None:
            raise ValueError("ObjectSegmenter: motion= carries the temporal gate of ONE object's mask (FrameSegmenter); "
                             "per-object gates in front of the merge are not built")
        if refine is not None:
            raise ValueError("ObjectSegmenter: refine= refines the logits of ONE object (FrameSegmenter); K fits in front of the "
                             "merge are not built")
        if roi is not None:
            raise ValueError("ObjectSegmenter: roi= follows ONE object (FrameSegmenter); a window around K objects is not built")
        if clean is not None:
            raise ValueError("ObjectSegmenter: clean= cleans the mask of ONE object (FrameSegmenter); per-object cleaning of "
                             "K logit maps before the merge is not built")
        self._set_geometry(height, width, depth, net_size)
        self.mirror, self.overlay = bool(mirror), bool(overlay)
        self.alpha = object_overlay.check_alpha(alpha)
        self.nets = list(nets)
        if not 1 <= len(self.nets) <= ops.MAX_OBJECTS:
            raise ValueError(f"ObjectSegmenter: {len(self.nets)} nets, outside [1, {ops.MAX_OBJECTS}]")
        if len({id(net) for net in self.nets}) != len(self.nets):
            raise ValueError("ObjectSegmenter: the same net twice (a net's output buffer belongs to its next call): "
                             "one module object per object")
        self.device = self._device_of(self.nets[0])
        for net in self.nets[1:]:
            if self._device_of(net) != self.device:
                raise RuntimeError(f"ObjectSegmenter: every net must be on {self.device}, got one on {self._device_of(net)}")
        if encode not in (None, 'jpeg', 'png'):
            raise ValueError(f"ObjectSegmenter: encode must be None, 'jpeg' or 'png', got {encode!r}")
        if encode == 'jpeg' and not self.overlay:
            raise ValueError("ObjectSegmenter: encode='jpeg' is lossy and a lossy label map means nothing: "
                             "overlay=False goes with encode='png'")
        if encode == 'png' and self.overlay:
            raise ValueError("ObjectSegmenter: encode='png' is the palette file of the label map (overlay=False); "
                             "the frame's PNG is the host's job")
        limits.check_member("ObjectSegmenter", "huffman", huffman, ops.PNG_HUFFMAN)
        if huffman != 'fixed' and encode != 'png':
            raise ValueError("ObjectSegmenter: huffman is the table choice of encode='png'")
        self.huffman = huffman
        if encode == 'png':
            self._set_jpeg(None, quality, subsampling, None)   # no JPEG: its fields at rest
            self.encode = encode
            self.capacity = ops.png_indexed_capacity(self.height, self.width)
            self._set_budget(budget, max(self.capacity // 4, 1024))
        else:
            if encode is None and budget is not None:
                raise ValueError("ObjectSegmenter: budget is the download budget of an encoder (encode='jpeg' or 'png')")
            self._set_jpeg(encode, quality, subsampling, budget)
        if palette is None:
            self.palette = ops.default_palette(self.device)
        else:
            if isinstance(palette, np.ndarray):
                palette = torch.from_numpy(object_overlay.check_palette(palette)).to(self.device)
            try:  # the ops' rule; here one sentence says it, for arrays and tensors alike
                self.palette = ops._palette(palette, self.device, "ObjectSegmenter")
            except (AttributeError, ValueError, RuntimeError):
                raise ValueError(f"ObjectSegmenter: a palette must be a contiguous uint8 [256,3] array or tensor on "
                                 f"{self.device}") from None
        self._open()

    def _compute(self, slot: _Slot) -> None:
        with torch.no_grad():
            ops.frame_prep(slot.frame, self.mirror, out=slot.image, net_size=self.net_size)
            logits = []
            for net in self.nets:
                with self._last_output_only(net):
                    logits.append(net.forward(slot.image)[-1])
            ops.overlay_objects(slot.frame, logits, self.mirror, self.overlay, self.palette, self.alpha, out=slot.out,
                                net_size=self.net_size)
            if self.encode == 'jpeg':
                ops.jpeg_encode(slot.out, self.quality, out=slot.file, lengths=slot.length, subsampling=self.subsampling)
            elif self.encode == 'png':
                ops.png_encode_indexed(slot.out, self.palette, out=slot.file, lengths=slot.length, huffman=self.huffman)

    def close(self) -> None:
        super().close()
        self.nets = []
