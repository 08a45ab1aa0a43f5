"""The switches of the Python face, declared: what the training loops decide (LoopOptions) and what a model's passes decide
(EngineOptions).  ``from_env`` of each is the ONLY place of the package that parses a ``FOSVOS_*`` switch; everything else
takes an options object.  The defaults are the measured best; every switch selects between two paths that both stay tested.
The table of all of them is in DESIGN.md (section 2).  CleanOptions (mask cleaning) is opt-in by being
passed and has no environment switch; so are AdaptOptions (online adaptation of the test pass), RoiOptions
and RefineOptions (following the object and edge-aware upsampling in a stream, DESIGN.md sections 12.2 and 12.3),
RotateOptions (rotating and zooming the training sample), EnsembleOptions (the test-time ensemble of the
test pass), CrfOptions (the CRF on the frame behind the test pass), MotionOptions
(the temporal gate's seed carried along the picture's motion) and LucidOptions (the one-shot sample with the
object moved against its background).

No torch and no library load here: importable anywhere.  The ranges and the scalar checks are ``limits``'.
"""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import Mapping, Optional, Union

from . import limits


def _on(environ: Mapping[str, str], name: str) -> bool:
    """A switch that is on unless the variable is exactly '0'."""
    return environ.get("FOSVOS_" + name, "1") != "0"


def _opt_in(environ: Mapping[str, str], name: str) -> bool:
    """A switch that is off unless the variable is exactly '1'."""
    return environ.get("FOSVOS_" + name, "0") == "1"


def _count(environ: Mapping[str, str], name: str, default: int) -> int:
    """A positive count; malformed -> the default, below 1 -> 1."""
    try:
        return max(1, int(environ.get("FOSVOS_" + name, default)))
    except ValueError:
        return default


@dataclass(frozen=True)
class LoopOptions:
    """What ``train_online._train`` / ``train_offline._train`` decide; resolved once at their entry (``options=`` or
    ``from_env()`` at that moment)."""

    # FOSVOS_MICROBATCH_GROUP.  Micro-batches of one accumulation cycle that may run as one batched pass (5 = the
    # reference's whole cycle, avg_grad_every_n; 1 = the reference's one-by-one order).  A group never crosses an optimizer
    # step, so the default runs a cycle of up to five same-size frames as ONE forward / backward pass: the fewest launches
    # and the fullest kernels (measured on the 480x854 step: 1086 frames/s against 1010 with 3 + 2 and 932 with 2 + 2 + 1).
    # Longer cycles are cut into groups of at most this many frames (activation memory grows with the group).
    microbatch_group: int = 5
    # FOSVOS_GROUP_WINDOW.  How many micro-batches of an accumulation cycle the loop looks at together before it forms its
    # batched passes (never more than the cycle itself, never fewer than a group).  The reference's augmentation draws a
    # random scale per iteration (src/dataloaders/custom_transforms.py:63-76), so consecutive frames rarely share a size;
    # gradients inside a cycle are a sum, so the micro-batches of the window are bucketed BY SHAPE and every bucket runs as
    # one batched pass.
    group_window: int = 16
    # FOSVOS_DEFER_JOIN=0 off.  Weights are constant inside an accumulation cycle: the next forward pass may overlap the
    # weight-gradient tail of this backward pass (PassFlags.defer_wgrad_join for the length of the loop).
    defer_join: bool = True
    # FOSVOS_SPLIT_STEP=0 = one optimizer step.  On the GPU the step is split by gradient bucket: stages 5-3 (97 % of the
    # parameters) are stepped, zeroed and repacked behind the data-gradient chain, while the weight-gradient stream still
    # works through stages 3-1; only the small rest waits for that stream (train_online: close_cycle).
    split_step: bool = True
    # FOSVOS_STAGE_LOSS (on only when exactly '1').  The loss of a batched pass in three stages (class counts in front of the
    # forward pass, values and host copy behind the backward pass; fosvos_cbce_loss_frames_parts): two launches and the copy
    # leave the chain of small kernels between the passes.  +0.5 % when that chain was 150 us long, neutral after the head
    # kernels got shorter, +0.3 % on the final build (5 of 5 interleaved rounds, profiles/r04_lab_step_ab_tunables.txt).
    # The same arithmetic either way (tested bit for bit); off = the loss as one call between the passes.
    stage_loss: bool = True
    # FOSVOS_GRAD_OVERWRITE=0: zero in the optimizer step, always add.  Gradient buffers without zeroing: a cycle that is ONE
    # batched pass (the usual case: nAveGrad frames of one shape) WRITES its gradients (PassFlags.overwrite_grads) instead of
    # adding them to buffers the previous optimizer step had to zero - one write and one read of every gradient less per
    # cycle, in the HBM-bound tail of the cycle (+0.6 %, profiles/r04_lab_step_ab_tunables.txt).  The optimizer step then
    # leaves the gradients in place ("stale"), and a cycle of several passes - which do add - zeroes the buffer first.  The
    # same values either way (a sum that starts from zero): tested bit for bit.
    grad_overwrite: bool = True
    # FOSVOS_PASS_STREAMS=0: one stream.  A cycle whose micro-batches cannot run as ONE batched pass (frames of different
    # sizes, or microbatch_group < nAveGrad) runs its passes on two alternating streams: the weights do not change inside a
    # cycle and every pass has its own arena, so the forward pass of one micro-batch may run beside the backward pass of the
    # previous one (their weight-gradient kernels share one stream and stay in order, so the accumulation into the gradients
    # does too).  Measured at 480x854, passes of 1 / 2 / 3+2 frames: +9.4 % / +2.0 % / -2.6 %, hence only for passes of at
    # most two frames (train_online: run_window).
    pass_streams: bool = True
    # FOSVOS_COMM_TIMING=1.  parallel.GradSync records events around every bucket's all-reduce (GPU only; timing_summary()).
    # ``parallel.COMM_TIMING``, which bench.py sets, turns the same on.
    comm_timing: bool = False

    @classmethod
    def from_env(cls, environ: Mapping[str, str] = os.environ) -> "LoopOptions":
        return cls(microbatch_group=_count(environ, "MICROBATCH_GROUP", 5), group_window=_count(environ, "GROUP_WINDOW", 16),
                   defer_join=_on(environ, "DEFER_JOIN"), split_step=_on(environ, "SPLIT_STEP"),
                   stage_loss=environ.get("FOSVOS_STAGE_LOSS", "1") == "1", grad_overwrite=_on(environ, "GRAD_OVERWRITE"),
                   pass_streams=_on(environ, "PASS_STREAMS"), comm_timing=_opt_in(environ, "COMM_TIMING"))


@dataclass(frozen=True)
class EngineOptions:
    """What the passes of one model decide; resolved when the model is constructed (``net.options``, replaceable with
    ``dataclasses.replace``).  ``stream_probe`` alone is process-level: engine.shared_stream resolves it when it creates a
    role's stream."""

    # FOSVOS_TWO_STREAMS=0 off.  The backward pass issues its weight-gradient kernels on the auxiliary stream, beside the
    # data-gradient chain (same kernels, same fixed-order reductions: tested bit for bit against one stream).
    two_streams: bool = True
    # FOSVOS_FWD_AUX=0: one stream.  Batched forward passes: the side_prep convs ride on the auxiliary stream beside the next
    # stage's backbone convs (+0.4 % on the five-frame training pass).  A single frame stays on one stream whatever this says:
    # its kernels are too short for the four event pairs to pay (inference protocol: 0.586 vs 0.564 ms per frame).
    fwd_aux: bool = True
    # FOSVOS_HEAD_UNIFORM=0 off (A/B).  Where the 16 channel filters of an upscale layer are identical - interp_surgery's
    # bilinear filters, which the optimizers never move (lr 0) - the head kernels contract the channels before the
    # upsampling (fosvos_head_fwd's ``filt_uniform``).  Checked on the weights themselves whenever they change.
    head_uniform: bool = True
    # FOSVOS_STREAM_PROBE=0 skips the ~1 ms probe.  The mapping of a shared stream onto a hardware queue is MEASURED when the
    # stream is created, and a stream that is serialised with an earlier one is parked (engine.shared_stream).
    stream_probe: bool = True
    # FOSVOS_RESNET_MFMA=0 keeps every ResNet layer on the vector-ALU kernel at its real channel count, fp32 first layer (A/B
    # runs); on, every map is widened to a channel count the MFMA implicit GEMM takes (resnet_engine.width).
    resnet_mfma: bool = True
    # FOSVOS_RESNET_FUSE_FIRST=0: the ResNet's first conv and max pool as two launches instead of one.
    resnet_fuse_first: bool = True
    # FOSVOS_RESNET_AUX=1 issues the ResNet's side_prep / downsample convs on a second stream beside the trunk.  Off by
    # default: measured at 1080p it LOSES 0.09-0.12 ms per frame on every net (the ~20 cross-stream event waits cost more than
    # the seven small kernels they take off the chain).
    resnet_aux: bool = False

    @classmethod
    def from_env(cls, environ: Mapping[str, str] = os.environ) -> "EngineOptions":
        return cls(two_streams=_on(environ, "TWO_STREAMS"), fwd_aux=_on(environ, "FWD_AUX"),
                   head_uniform=_on(environ, "HEAD_UNIFORM"), stream_probe=_on(environ, "STREAM_PROBE"),
                   resnet_mfma=_on(environ, "RESNET_MFMA"), resnet_fuse_first=_on(environ, "RESNET_FUSE_FIRST"),
                   resnet_aux=_opt_in(environ, "RESNET_AUX"))


@dataclass(frozen=True)
class CleanOptions:
    """Cleaning a mask by its shape (``ops.clean_components``; util/mask_components.py states the rules), for
    ``FrameSegmenter(clean=)`` and ``test_fast(clean=)``.  Opt-in: None where it is accepted means no cleaning, and this
    class reads no environment variable."""

    # components of fewer pixels are dropped (an area equal to min_area stays)
    min_area: int = 0
    # keep only the largest of the components that are left
    largest: bool = False
    # None: no temporal gate.  0..63: keep only components with a pixel within this many pixels of what the frame before
    # kept (of the initial seed for the first frame); a frame that kept nothing gates nothing in the next
    temporal_radius: Optional[int] = None
    # what a dropped pixel's logit becomes: finite (the overlay interpolates logits) and negative
    fill: float = -100.0

    def __post_init__(self) -> None:
        limits.check_int("CleanOptions", "min_area", self.min_area, 0, limits.CLEAN_MAX_AREA)
        if not isinstance(self.largest, bool):
            raise ValueError(f"CleanOptions: largest must be a bool, got {self.largest!r}")
        if self.temporal_radius is not None:
            limits.check_int("CleanOptions", "temporal_radius", self.temporal_radius, 0, limits.CLEAN_MAX_RADIUS,
                             expect=f"None or an integer in 0..{limits.CLEAN_MAX_RADIUS}")
        limits.check_real("CleanOptions", "fill", self.fill, *limits.FILL_RANGE, hi_open=True, expect="finite and negative")

    @property
    def chain(self) -> bool:
        return self.temporal_radius is not None

    def as_dict(self) -> dict:
        return {'min_area': self.min_area, 'largest': self.largest, 'temporal_radius': self.temporal_radius,
                'fill': float(self.fill)}


@dataclass(frozen=True)
class RoiOptions:
    """Following the object in a stream (``FrameSegmenter(roi=)``; util/frame_roi.py states the rules; DESIGN.md section
    12.2): the net looks at a window of the frame around the last mask.  Opt-in by being passed; this class reads no
    environment variable.  The defaults are unmeasured."""

    # the window sizes between the net's size (level 0) and the frame's (level ``levels``): 1..64
    levels: int = 8
    # the box of the mask is padded on every side by this share of its longer side: a finite number in [0, 4]
    margin: float = 0.25
    # ... and by this many frame pixels: 0..4095.  What the object may move from one frame to the next
    min_pad: int = 16

    def __post_init__(self) -> None:
        limits.check_int("RoiOptions", "levels", self.levels, 1, limits.ROI_MAX_LEVELS)
        limits.check_real("RoiOptions", "margin", self.margin, 0.0, limits.ROI_MAX_MARGIN)
        limits.check_int("RoiOptions", "min_pad", self.min_pad, 0, limits.ROI_MAX_PAD)

    @property
    def margin_permille(self) -> int:
        """The margin as the integer the kernel and the numpy definition pad with."""
        return int(round(1000 * self.margin))

    def as_dict(self) -> dict:
        return {'levels': self.levels, 'margin': float(self.margin), 'min_pad': self.min_pad}


@dataclass(frozen=True)
class RefineOptions:
    """Edge-aware upsampling in a stream (``FrameSegmenter(refine=)``; util/guided_upsample.py states the rules; DESIGN.md
    section 12.3): the guided filter with the frame as the guide, in place of the bilinear upsampling of the logits.  Opt-in
    by being passed; this class reads no environment variable.  The defaults are the design's and are unmeasured on trained
    nets."""

    # the fit's and the smoothing's window reaches this many net pixels to every side: 1..8
    radius: int = 4
    # the regulariser beside the guide's variance in the window (the guide is the sum of three mean-free bytes, so an edge of
    # 50 grey levels has a variance of about 5000): a finite number in [1e-3, 1e9].  Larger: smoother, less edge-following
    eps: float = 400.0
    # the logits are clipped to [-clip, clip] first, so that one confident pixel does not outweigh its window: (0, 1e4]
    clip: float = 6.0

    def __post_init__(self) -> None:
        limits.check_int("RefineOptions", "radius", self.radius, 1, limits.GUIDED_MAX_RADIUS)
        limits.check_real("RefineOptions", "eps", self.eps, *limits.GUIDED_EPS_RANGE)
        limits.check_real("RefineOptions", "clip", self.clip, 0.0, limits.GUIDED_MAX_CLIP, lo_open=True)

    def as_dict(self) -> dict:
        return {'radius': self.radius, 'eps': float(self.eps), 'clip': float(self.clip)}


@dataclass(frozen=True)
class AdaptOptions:
    """Online adaptation of the test pass (``experiment_helper.test_adaptive``; util/online_adapt.py states the rules;
    DESIGN.md section 17).  Opt-in by being passed; this class reads no environment variable.  The defaults are OnAVOS's
    published ones at 480p and are unmeasured here."""

    # fine-tune steps on every frame; 0 = the pass labels the frames and trains nothing
    steps: int = 1
    # a pixel whose probability is at least this is a positive (outside the negatives): 0.5 < p < 1
    pos_prob: float = 0.97
    # a pixel further than this many pixels from the eroded last mask is a negative: 0..4095
    neg_distance: int = 220
    # the last mask is eroded by the disk of this radius first: 0..4095
    erode: int = 15
    # weight of the current frame's pseudo-label loss in a step: > 0
    frame_weight: float = 1.0
    # weight of the annotated first frame's loss in a step: >= 0 (0: the first frame is not passed through the net at all)
    first_weight: float = 1.0
    # learning rate of the adaptation's optimizer (net_provider.get_optimizer(learning_rate=)): > 0
    learning_rate: float = 1e-8

    def __post_init__(self) -> None:
        limits.check_int("AdaptOptions", "steps", self.steps, 0)
        limits.check_real("AdaptOptions", "pos_prob", self.pos_prob, 0.5, 1.0, lo_open=True, hi_open=True,
                          expect="a probability in (0.5, 1)")
        limits.check_int("AdaptOptions", "neg_distance", self.neg_distance, 0, limits.GATE_MAX_DISTANCE)
        limits.check_int("AdaptOptions", "erode", self.erode, 0, limits.GATE_MAX_DISTANCE)
        limits.check_real("AdaptOptions", "frame_weight", self.frame_weight, 0.0, lo_open=True)
        limits.check_real("AdaptOptions", "first_weight", self.first_weight, 0.0)
        limits.check_real("AdaptOptions", "learning_rate", self.learning_rate, 0.0, lo_open=True)

    @property
    def pos_logit(self) -> float:
        """log(p / (1 - p)) in float64, rounded to float32 once (the value the kernel and the numpy definition compare with)."""
        import math
        import struct
        return struct.unpack("f", struct.pack("f", math.log(self.pos_prob / (1.0 - self.pos_prob))))[0]

    def as_dict(self) -> dict:
        return {'steps': self.steps, 'pos_prob': float(self.pos_prob), 'pos_logit': self.pos_logit,
                'neg_distance': self.neg_distance, 'erode': self.erode, 'frame_weight': float(self.frame_weight),
                'first_weight': float(self.first_weight), 'learning_rate': float(self.learning_rate)}


@dataclass(frozen=True)
class RotateOptions:
    """Rotating and zooming the training sample about its centre (the reference's ``ScaleNRotate``, commented out beside
    ``Resize`` in its training loader; ``get_data_loader_train(rotate=)`` and the resident loaders).
    Opt-in by being passed; this class reads no environment variable.  The ranges are the reference's.

    A tuple is a continuous range, drawn as ``(hi - lo) * random() - (hi - lo) / 2`` (plus 1 for the zoom): the reference
    centres the draw on 0 degrees and on zoom 1 whatever the ends are.  A list is a set of fixed choices.  Both fields are of
    one kind."""

    # degrees, counter-clockwise: every entry a finite number in [-360, 360]
    rots: Union[tuple, list] = (-30.0, 30.0)
    # zoom factors: every entry a finite number in [1/16, 16]
    scales: Union[tuple, list] = (0.75, 1.25)
    # True: the reference's renormalisation of the warped frame to [0, 1] (``ScaleNRotate(renormalize=True)``), which is not
    # what the nets are trained on; the default keeps the mean-subtracted values (a documented deviation)
    renormalize: bool = False

    def __post_init__(self) -> None:
        if type(self.rots) not in (tuple, list) or type(self.scales) is not type(self.rots):
            raise ValueError("RotateOptions: rots and scales must both be tuples (continuous ranges) or both be lists "
                             f"(fixed choices), got {self.rots!r} and {self.scales!r}")
        for name, v in (("rots", self.rots), ("scales", self.scales)):
            if isinstance(v, tuple) and len(v) != 2:
                raise ValueError(f"RotateOptions: {name} as a range must be (lo, hi), got {v!r}")
            if not v:
                raise ValueError(f"RotateOptions: {name} must not be empty")
        for v in self.rots:
            limits.check_real("RotateOptions", "rots", v, -limits.ROTATE_MAX_ANGLE, limits.ROTATE_MAX_ANGLE)
        for v in self.scales:
            limits.check_real("RotateOptions", "scales", v, *limits.ROTATE_SCALE_RANGE)
        if isinstance(self.rots, tuple):
            if self.rots[0] > self.rots[1] or self.scales[0] > self.scales[1]:
                raise ValueError(f"RotateOptions: a range must be (lo, hi) with lo <= hi, got {self.rots!r} and {self.scales!r}")
            # what the reference's draw can reach: 1 +- (hi - lo) / 2
            limits.check_real("RotateOptions", "scales", 1 - (self.scales[1] - self.scales[0]) / 2, *limits.ROTATE_SCALE_RANGE,
                              expect="a range whose draw 1 +- (hi - lo) / 2 stays in [1/16, 16]")
        if not isinstance(self.renormalize, bool):
            raise ValueError(f"RotateOptions: renormalize must be a bool, got {self.renormalize!r}")

    def transform(self):
        """The ``custom_transforms.ScaleNRotate`` these options describe."""
        from dataloaders import custom_transforms
        return custom_transforms.ScaleNRotate(self.rots, self.scales, self.renormalize)


@dataclass(frozen=True)
class EnsembleOptions:
    """Test-time ensemble of the test pass (``test_fast(ensemble=)`` and ``test_objects(ensemble=)``; util/test_ensemble.py
    states the rules): the net also sees the frame mirrored and at other sizes, and the logits are
    averaged back on the frame's grid.  Opt-in by being passed; this class reads no environment variable."""

    # every scale is also forwarded mirrored along W
    flip: bool = False
    # the sizes the net sees the frame at, as factors of the frame's: distinct finite numbers in [0.25, 4]
    scales: tuple = (1.0,)

    def __post_init__(self) -> None:
        if not isinstance(self.flip, bool):
            raise ValueError(f"EnsembleOptions: flip must be a bool, got {self.flip!r}")
        if type(self.scales) not in (tuple, list) or not self.scales:
            raise ValueError(f"EnsembleOptions: scales must be a non-empty tuple of numbers, got {self.scales!r}")
        object.__setattr__(self, "scales", tuple(self.scales))
        for v in self.scales:
            limits.check_real("EnsembleOptions", "scales", v, *limits.ENSEMBLE_SCALE_RANGE,
                              expect=f"finite numbers in [{limits.ENSEMBLE_SCALE_RANGE[0]:g}, {limits.ENSEMBLE_SCALE_RANGE[1]:g}]")
        if len(set(float(v) for v in self.scales)) != len(self.scales):
            raise ValueError(f"EnsembleOptions: scales must be distinct, got {self.scales!r}")
        n_views = len(self.scales) * (2 if self.flip else 1)
        if n_views == 1 and float(self.scales[0]) == 1.0:
            raise ValueError("EnsembleOptions: the frame as it is, once, is no ensemble: set flip or give further scales")
        if not 2 <= n_views <= limits.ENSEMBLE_MAX_VIEWS:
            raise ValueError(f"EnsembleOptions: {n_views} views, outside [2, {limits.ENSEMBLE_MAX_VIEWS}] "
                             f"({len(self.scales)} scales{', each also mirrored' if self.flip else ''})")

    def views(self) -> list:
        """``test_ensemble.views(flip, scales)``: per scale ``(s, False)`` and then, with ``flip``, ``(s, True)``."""
        return [(float(s), f) for s in self.scales for f in ((False, True) if self.flip else (False,))]

    def as_dict(self) -> dict:
        return {'flip': self.flip, 'scales': [float(s) for s in self.scales]}


@dataclass(frozen=True)
class CrfOptions:
    """Refining the test pass's logits with a local CRF on the frame's colours (``test_fast(crf=)`` and ``test_objects(crf=)``,
    ``ops.crf_refine``; util/mask_crf.py states the rules): mean-field inference over a window of the
    frame with an appearance and a smoothness kernel.  Opt-in by being passed; this class reads no environment variable.  The
    defaults are DenseCRF-like and are unmeasured on trained nets."""

    # mean-field iterations, one launch each: 1..10
    iterations: int = 5
    # the window reaches this many pixels to every side: 1..5
    radius: int = 5
    # the appearance kernel's width in pixels: a finite number in [0.25, 1e3]
    theta_pos: float = 8.0
    # ... and in grey levels of one channel: [1, 1e3].  Smaller: only pixels of nearly the same colour vote
    theta_rgb: float = 13.0
    # the smoothness kernel's width in pixels: [0.25, 1e3]
    theta_smooth: float = 3.0
    # what the two kernels' (normalised) messages weigh beside the clipped logit: [0, 100] each
    weight_appearance: float = 4.0
    weight_smooth: float = 3.0
    # the logits are clipped to [-clip, clip] first, so that the picture can outvote a confident net: (0, 1e4]
    clip: float = 6.0

    def __post_init__(self) -> None:
        limits.check_int("CrfOptions", "iterations", self.iterations, 1, limits.CRF_MAX_ITERATIONS)
        limits.check_int("CrfOptions", "radius", self.radius, 1, limits.CRF_MAX_RADIUS)
        limits.check_real("CrfOptions", "theta_pos", self.theta_pos, *limits.CRF_THETA_POS_RANGE)
        limits.check_real("CrfOptions", "theta_rgb", self.theta_rgb, *limits.CRF_THETA_RGB_RANGE)
        limits.check_real("CrfOptions", "theta_smooth", self.theta_smooth, *limits.CRF_THETA_SMOOTH_RANGE)
        limits.check_real("CrfOptions", "weight_appearance", self.weight_appearance, 0.0, limits.CRF_MAX_WEIGHT)
        limits.check_real("CrfOptions", "weight_smooth", self.weight_smooth, 0.0, limits.CRF_MAX_WEIGHT)
        limits.check_real("CrfOptions", "clip", self.clip, 0.0, limits.CRF_MAX_CLIP, lo_open=True)

    def as_dict(self) -> dict:
        return {'iterations': self.iterations, 'radius': self.radius, 'theta_pos': float(self.theta_pos),
                'theta_rgb': float(self.theta_rgb), 'theta_smooth': float(self.theta_smooth),
                'weight_appearance': float(self.weight_appearance), 'weight_smooth': float(self.weight_smooth),
                'clip': float(self.clip)}


@dataclass(frozen=True)
class MotionOptions:
    """Carrying the temporal gate's seed along the picture's motion (``test_fast(clean=, motion=)``,
    ``FrameSegmenter(clean=, motion=)``, ``ops.motion_estimate``; util/block_motion.py states the rules):
    full-search block matching on the frames' luma, and the kept mask of the frame before warped block by block.  It needs
    ``CleanOptions.temporal_radius``.  Opt-in by being passed; this class reads no environment variable.  The defaults are the
    design's and are unmeasured on real sequences."""

    # the side of a block in pixels: 8 or 16
    block: int = 16
    # a block is looked for up to this many pixels away in every direction: 1..16
    search: int = 8
    # what a non-zero vector must win by, in sixteenths of a grey level a pixel: 0..255.  Holds flat blocks still
    zero_bias: int = 8

    def __post_init__(self) -> None:
        limits.check_int("MotionOptions", "block", self.block, min(limits.MOTION_BLOCKS), max(limits.MOTION_BLOCKS),
                         expect=f"one of {limits.MOTION_BLOCKS}")
        limits.check_member("MotionOptions", "block", self.block, limits.MOTION_BLOCKS)
        limits.check_int("MotionOptions", "search", self.search, 1, limits.MOTION_MAX_SEARCH)
        limits.check_int("MotionOptions", "zero_bias", self.zero_bias, 0, limits.MOTION_MAX_ZERO_BIAS)

    def as_dict(self) -> dict:
        return {'block': self.block, 'search': self.search, 'zero_bias': self.zero_bias}


@dataclass(frozen=True)
class LucidOptions:
    """Moving the object against its background in the one-shot training sample (``ResidentOneShotLoader(lucid=)``,
    ``get_data_loader_train(lucid=)``, ``ops.lucid_sample``; dataloaders/lucid.py states the rules): per
    draw the background and the object are rotated, zoomed and (the object) shifted independently, the illumination is changed
    and the two are composed again.  Every range is ``(lo, hi)`` with lo <= hi; a draw is lo + (hi - lo) u.  Opt-in by being
    passed; this class reads no environment variable.  The defaults are the design's and are unmeasured on real sequences."""

    # the background about the frame's centre: degrees in [-360, 360], zoom factors in [1/16, 16]
    bg_rots: tuple = (-10.0, 10.0)
    bg_scales: tuple = (1.0, 1.2)
    # the object about the centre of its box: degrees, zoom factors, and a shift in box widths / heights in [-4, 4]
    fg_rots: tuple = (-15.0, 15.0)
    fg_scales: tuple = (0.85, 1.15)
    fg_shift: tuple = (-0.15, 0.15)
    # the illumination: out * (contrast * tint_c) + brightness; factors in [1/16, 16], grey levels in [-255, 255]
    contrast: tuple = (0.85, 1.15)
    tint: tuple = (0.95, 1.05)
    brightness: tuple = (-15.0, 15.0)
    # the painted-out background: the hole is the mask grown by `dilate` pixels (0..31), the fill smoothed `smooth` times (0..16)
    dilate: int = 5
    smooth: int = 2

    def __post_init__(self) -> None:
        angle = (-limits.ROTATE_MAX_ANGLE, limits.ROTATE_MAX_ANGLE)
        for name, (lo, hi) in (("bg_rots", angle), ("bg_scales", limits.ROTATE_SCALE_RANGE), ("fg_rots", angle),
                               ("fg_scales", limits.ROTATE_SCALE_RANGE),
                               ("fg_shift", (-limits.LUCID_MAX_SHIFT, limits.LUCID_MAX_SHIFT)),
                               ("contrast", limits.LUCID_GAIN_RANGE), ("tint", limits.LUCID_GAIN_RANGE),
                               ("brightness", (-limits.LUCID_MAX_BRIGHTNESS, limits.LUCID_MAX_BRIGHTNESS))):
            v = getattr(self, name)
            if type(v) not in (tuple, list) or len(v) != 2:
                raise ValueError(f"LucidOptions: {name} must be a range (lo, hi), got {v!r}")
            object.__setattr__(self, name, tuple(v))
            for x in v:
                limits.check_real("LucidOptions", name, x, lo, hi)
            if v[0] > v[1]:
                raise ValueError(f"LucidOptions: {name} must be (lo, hi) with lo <= hi, got {v!r}")
        limits.check_int("LucidOptions", "dilate", self.dilate, 0, limits.LUCID_MAX_DILATE)
        limits.check_int("LucidOptions", "smooth", self.smooth, 0, limits.LUCID_MAX_SMOOTH)

    def dream(self):
        """The ``lucid.LucidDream`` these options describe."""
        from dataloaders import lucid
        return lucid.LucidDream(self)

    def as_dict(self) -> dict:
        return {name: (list(v) if isinstance(v, tuple) else v) for name, v in self.__dict__.items()}


def native_loop_from_env(environ: Mapping[str, str] = os.environ) -> bool:
    """Initial value of ``engine.USE_NATIVE_LOOP``: FOSVOS_PY_ENGINE=1 selects the Python-driven per-op loop (debugging, and
    the reference point the native loop is tested against)."""
    return environ.get("FOSVOS_PY_ENGINE", "0") != "1"
