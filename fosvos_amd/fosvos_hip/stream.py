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

Not thread-safe: one host thread drives a segmenter.
"""
from __future__ import annotations

from collections import deque
from typing import Deque, Iterable, Iterator, List, Optional, Tuple, Union

import numpy as np
import torch

from . import ops


_HEAD = 8  # bytes in front of a slot's file: the int32 length, padded so that the file starts 8-byte aligned


class _Slot:
    def __init__(self, h: int, w: int, out_shape, device: torch.device, capacity: int = 0, budget: int = 0,
                 net_size=None) -> None:
        self.host_in = torch.empty((1, h, w, 3), dtype=torch.uint8, pin_memory=True)
        self.host_in_np = self.host_in.numpy()
        self.frame = torch.empty((1, h, w, 3), dtype=torch.uint8, device=device)
        self.image = torch.empty((1, 3) + tuple(net_size or (h, w)), dtype=torch.float32, device=device)
        self.out = torch.empty(out_shape, dtype=torch.uint8, device=device)
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
    close()          wait for what is in flight and release every buffer
    """

    def __init__(self, net, height: int, width: int, depth: int = 2, mirror: bool = True, overlay: bool = True,
                 boolean_mask: bool = True, color: str = 'r', alpha: float = 1.0, encode: Optional[str] = None,
                 quality: int = 90, subsampling: str = '4:4:4', budget: Optional[int] = None,
                 net_size: Optional[Tuple[int, int]] = None) -> None:
        from util import frame_overlay
        self.height, self.width, self.depth = int(height), int(width), int(depth)
        if self.height <= 0 or self.width <= 0 or self.depth <= 0:
            raise ValueError(f"FrameSegmenter: height, width and depth must be positive, got {height}, {width}, {depth}")
        # None where the net runs at the frame's size: the unscaled launches, exactly
        self.net_size = ops._net_size(net_size, self.height, self.width, "FrameSegmenter")
        frame_overlay.check_color(color)
        self.mirror, self.overlay, self.boolean_mask = bool(mirror), bool(overlay), bool(boolean_mask)
        self.color, self.alpha = color, frame_overlay.check_alpha(alpha)
        self.net = net
        param = next(iter(net.parameters()), None)
        if param is None or not param.is_cuda:
            raise RuntimeError("FrameSegmenter: the net must live on the GPU (the HIP path has no CPU fallback)")
        self.device = param.device
        h, w = self.height, self.width
        out_shape = (1, h, w, 3) if self.overlay else (1, h, w)
        if encode not in (None, 'jpeg'):
            raise ValueError(f"FrameSegmenter: encode must be None or 'jpeg', got {encode!r}")
        self.encode, self.quality = encode, quality
        if subsampling != '4:4:4' and not encode:
            raise ValueError("FrameSegmenter: subsampling is the chroma sampling of encode='jpeg'")
        self.subsampling = subsampling if encode else None
        self.capacity = self.budget = 0
        self.second_copies = 0  # frames whose file was longer than the budget
        self.bytes_down = 0     # bytes the downloads moved
        if encode:
            if isinstance(quality, bool) or not isinstance(quality, int) or not 1 <= quality <= 100:
                raise ValueError(f"FrameSegmenter: quality must be an integer in 1..100, got {quality!r}")
            if self.subsampling not in ops.JPEG_SUBSAMPLINGS:
                raise ValueError(f"FrameSegmenter: subsampling must be one of {ops.JPEG_SUBSAMPLINGS}, got {subsampling!r}")
            self.capacity = ops.jpeg_capacity(h, w, 3 if self.overlay else 1, self.subsampling)
            raw = h * w * (3 if self.overlay else 1)
            if budget is None:
                budget = max(raw // 4, 1024)
            if isinstance(budget, bool) or not isinstance(budget, int) or budget <= 0:
                raise ValueError(f"FrameSegmenter: budget must be a positive number of bytes, got {budget!r}")
            self.budget = min(budget, self.capacity)
        elif budget is not None:
            raise ValueError("FrameSegmenter: budget is the download budget of encode='jpeg'")
        self._closed = False
        with torch.cuda.device(self.device):
            self._up = torch.cuda.Stream(device=self.device)
            self._down = torch.cuda.Stream(device=self.device)
            self._rest = torch.cuda.Stream(device=self.device) if encode else None  # second copies of long files
            self._free: List[_Slot] = [_Slot(h, w, out_shape, self.device, self.capacity, self.budget, self.net_size)
                                       for _ in range(self.depth)]
        self._flight: Deque[_Slot] = deque()     # submitted, oldest first
        self._ready: Deque[Union[np.ndarray, bytes]] = deque()  # retired by a submit that needed the slot, not yet asked for

    # ---------------------------------------------------------------------------------------------- checks
    def _check_open(self) -> None:
        if self._closed:
            raise RuntimeError("FrameSegmenter: closed")

    def _check_frame(self, frame):
        if isinstance(frame, torch.Tensor):  # a frame that is on the device already (ops.jpeg_decode made it)
            if frame.dtype != torch.uint8 or frame.device != self.device or not frame.is_contiguous():
                raise ValueError(f"FrameSegmenter: a device frame must be a contiguous uint8 tensor on {self.device}, got "
                                 f"{frame.dtype} on {frame.device}")
            if tuple(frame.shape) != (self.height, self.width, 3):
                raise ValueError(f"FrameSegmenter: a frame must be {(self.height, self.width, 3)}, got {tuple(frame.shape)}")
            return frame
        if not isinstance(frame, np.ndarray) or frame.dtype != np.uint8:
            raise ValueError(f"FrameSegmenter: a frame must be a uint8 numpy array, got {getattr(frame, 'dtype', type(frame))}")
        if frame.shape != (self.height, self.width, 3):
            raise ValueError(f"FrameSegmenter: a frame must be {(self.height, self.width, 3)}, got {frame.shape}")
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
                raise RuntimeError(f"FrameSegmenter: the encoder reported a file of {length} bytes (capacity {self.capacity})")
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

    def _enqueue(self, slot: _Slot, main: torch.cuda.Stream, device_frame: Optional[torch.Tensor] = None) -> None:
        if device_frame is not None:  # made on the caller's stream, which is `main`: a copy in stream order, no upload
            slot.frame[0].copy_(device_frame, non_blocking=True)
        else:
            with torch.cuda.stream(self._up):
                slot.frame.copy_(slot.host_in, non_blocking=True)
                slot.moved.record(self._up)
            main.wait_event(slot.moved)
        net = self.net
        had, old = hasattr(net, 'compute_side_outputs'), getattr(net, 'compute_side_outputs', None)
        net.compute_side_outputs = False
        try:
            with torch.no_grad():
                ops.frame_prep(slot.frame, self.mirror, out=slot.image, net_size=self.net_size)
                logits = net.forward(slot.image)[-1]
                ops.overlay(slot.frame, logits, self.mirror, self.boolean_mask, self.color, self.alpha, self.overlay,
                            out=slot.out, net_size=self.net_size)
                if self.encode:
                    ops.jpeg_encode(slot.out, self.quality, out=slot.file, lengths=slot.length, subsampling=self.subsampling)
        finally:
            if had:
                net.compute_side_outputs = old
            else:
                del net.compute_side_outputs
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
                except Exception:
                    self.close()
                raise
        self._flight.append(slot)

    def result(self) -> np.ndarray:
        self._check_open()
        if self._ready:
            return self._ready.popleft()
        if not self._flight:
            raise RuntimeError("FrameSegmenter.result: no frame is in flight")
        return self._retire()

    def segment(self, frames: Iterable[np.ndarray]) -> Iterator[np.ndarray]:
        self._check_open()
        if self.pending:
            raise RuntimeError("FrameSegmenter.segment: fetch the results of the frames already submitted first")
        for frame in frames:
            if len(self._flight) == self.depth:
                yield self.result()
            self.submit(frame)
        while self.pending:
            yield self.result()

    def apply(self, frame: np.ndarray) -> np.ndarray:
        self._check_open()
        if self.pending:
            raise RuntimeError("FrameSegmenter.apply: fetch the results of the frames already submitted first")
        self.submit(frame)
        return self.result()

    def close(self) -> None:
        if self._closed:
            return
        self._closed = True
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
