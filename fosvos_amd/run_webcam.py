"""The live demo's loop (reference: src/run_webcam.py) without its window: frames from a camera, a directory of images or
the synthetic sequence go through ``fosvos_hip.stream.FrameSegmenter`` - prep, net and overlay on the device, ``depth``
frames in flight - and the results are written as PNGs and / or timed.

The options carry the reference's names and defaults.  Additions: ``--model`` (a checkpoint file instead of
``models/<the reference's file name>``), ``--source DIR``, ``--synthetic N`` (with ``--height`` / ``--width``), ``--output DIR``,
``--depth``, and ``--output-format jpeg`` with ``--jpeg-quality``: the device encodes each result as a JPEG file
(``FrameSegmenter(encode='jpeg')``) and the loop only writes ``%05d.jpg``; ``--jpeg-subsampling 420`` chooses the encoder's
4:2:0 form, and ``--output NAME.avi`` (with ``--fps``) puts the same files into one Motion-JPEG AVI (util/mjpeg_avi.py)
instead of a directory.  ``--source NAME.avi`` reads such a file back (util/mjpeg_avi.AviReader), and ``--device-decode``
decodes the JPEG frames of either source on the device (``ops.jpeg_decode``, in groups of ``DECODE_GROUP``): the frames reach
the segmenter without ever being pixels on the host; other file types and files the device decoder does not take
(util/jpeg_read.probe is None, grey files, a non-zero status) go through PIL as before.  ``--net-height N --net-width N``
(both, no larger than the frames) run the net at that size: the device area-averages each frame down to it in front of the net
and interpolates the logits back up behind it (``FrameSegmenter(net_size=)``; util/frame_resample.py), and every output
keeps the frame's size.  ``--models A.pth B.pth ...`` (instead of ``--model``; file k is object k, ``--variant`` / ``--version``
say what all of them are) streams several objects: the nets a ``train_online.py --multi-object`` run left go through
``fosvos_hip.stream.ObjectSegmenter``, every frame through all of them, and the result is the frame with each object blended
towards its DAVIS palette colour (``--palette-alpha``, 0..1), or with ``--no-overlay`` the label map - written to ``--output DIR``
as palette PNG files that the device encoded.  ``--clean-min-area N``, ``--clean-largest`` and ``--clean-temporal R`` (any of them;
single object only) clean the net's mask on the device before the overlay (``FrameSegmenter(clean=)``;
util/mask_components.py): connected components that are too small, not the largest, or further than R net pixels from what the
frame before kept are dropped; ``--clean-seed FILE.png`` is the mask the first frame is gated by; ``--clean-motion`` (with
``--motion-block`` / ``--motion-search`` / ``--motion-zero-bias``) carries that kept mask along the motion of the picture first
(``FrameSegmenter(motion=)``; util/block_motion.py).  ``--roi`` (with
``--net-height`` / ``--net-width``; single object only) follows the object: the net sees a window of the frame around the last
mask, scaled to the net's size, and the logits are painted back into it (``FrameSegmenter(roi=)``; util/frame_roi.py);
``--roi-levels N``, ``--roi-margin F`` and ``--roi-min-pad P`` are the RoiOptions, ``--roi-seed FILE.png`` is the annotation the
first window is taken from.  ``--clean-largest`` is its recommended companion.  ``--refine`` (single object only, not with
``--roi``) upsamples by the frame's own edges: the guided filter with the frame as the guide replaces the bilinear upsampling of
the logits (``FrameSegmenter(refine=)``; util/guided_upsample.py); ``--refine-radius N``, ``--refine-eps F`` and ``--refine-clip F``
are the RefineOptions.  There is no CPU path (``--no-cuda`` is refused) and no display; ``--webcam`` needs OpenCV for the capture.
"""
import argparse
import os
import sys
import time
from pathlib import Path
from typing import Iterator, List, Optional, Tuple

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

from dataloaders import synthetic  # noqa: E402
from dataloaders.davis_2016 import MEANVAL, read_bgr  # noqa: E402
from networks.osvos_resnet import OSVOS_RESNET  # noqa: E402
from networks.osvos_vgg import OSVOS_VGG  # noqa: E402
from util.logger import get_logger  # noqa: E402

log = get_logger(__file__)
log.setLevel('INFO')

IMAGE_SUFFIXES = ('.jpg', '.jpeg', '.png', '.bmp')


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter, allow_abbrev=False)
    p.add_argument('--variant', '-var', choices=['vgg', 'resnet', 'prune', 'mimic'], default='resnet')
    p.add_argument('--version', '-ver', type=int, default=None)
    p.add_argument('--webcam', '-wc', type=int, default=0, help='camera index, used when neither --source nor --synthetic is given')

    def switch(on, off, dest, default=True):
        p.add_argument(*on, dest=dest, action='store_true', default=default)
        p.add_argument(*off, dest=dest, action='store_false')

    switch(('--mirror', '-m'), ('--no-mirror', '-nm'), 'mirror')
    switch(('--use-network', '-n'), ('--no-network', '-nn'), 'use_network')
    switch(('--use-cuda', '-c'), ('--no-cuda', '-nc'), 'use_cuda')
    switch(('--overlay', '-o'), ('--no-overlay', '-no'), 'overlay')
    switch(('--boolean-mask', '-bm'), ('--no-boolean-mask', '-nbm'), 'boolean_mask')
    p.add_argument('--overlay-color', '-oc', choices=['r', 'g', 'b'], default='r')
    p.add_argument('--overlay-alpha', '-oa', type=float, default=1.0)
    # not in the reference
    p.add_argument('--model', type=str, default=None, help='checkpoint file (default: models/<the variant\'s file name>)')
    p.add_argument('--source', type=str, default=None, help='directory of image files, read in sorted order')
    p.add_argument('--synthetic', type=int, default=None, metavar='N', help='N frames of the synthetic sequence')
    p.add_argument('--height', type=int, default=480)
    p.add_argument('--width', type=int, default=854)
    p.add_argument('--output', type=str, default=None,
                   help='directory the results are written to as PNGs; NAME.avi with --output-format jpeg: one Motion-JPEG file')
    p.add_argument('--depth', type=int, default=2, help='frames in flight')
    p.add_argument('--output-format', choices=['png', 'jpeg'], default='png',
                   help='files of --output: png (written by PIL on the host) or jpeg (encoded on the device)')
    p.add_argument('--jpeg-quality', type=int, default=90, help='1..100, with --output-format jpeg')
    p.add_argument('--jpeg-subsampling', choices=['444', '420'], default='444', help='chroma sampling, with --output-format jpeg')
    p.add_argument('--fps', type=float, default=25, help='frame rate written into --output NAME.avi')
    p.add_argument('--device-decode', action='store_true',
                   help='decode the JPEG frames of --source (a directory or NAME.avi) on the device')
    p.add_argument('--net-height', type=int, default=None, metavar='N',
                   help='run the net at N rows (with --net-width; no more than the frames have)')
    p.add_argument('--net-width', type=int, default=None, metavar='N', help='run the net at N columns (with --net-height)')
    p.add_argument('--models', type=str, nargs='+', default=None, metavar='FILE',
                   help='several objects: one checkpoint file per object, file k is object k (instead of --model)')
    p.add_argument('--palette-alpha', type=float, default=0.5,
                   help='0..1: how far an object\'s pixels go towards its palette colour, with --models')
    p.add_argument('--clean-min-area', type=int, default=None, metavar='N',
                   help='clean the mask on the device: drop connected components of fewer than N pixels')
    p.add_argument('--clean-largest', action='store_true', help='clean the mask on the device: keep the largest component only')
    p.add_argument('--clean-temporal', type=int, default=None, metavar='R',
                   help='clean the mask on the device: keep only components within R (0..63) net pixels of what the '
                        'frame before kept')
    from util import args_helper
    args_helper.add_motion_arguments(p)
    p.add_argument('--clean-seed', type=str, default=None, metavar='FILE.png',
                   help='the mask --clean-temporal starts from (non-zero = object; the frames\' or the net\'s size), '
                        'e.g. the annotation the net was fine-tuned on')
    p.add_argument('--roi', action='store_true',
                   help='follow the object: run the net on a window around the last mask (with --net-height and --net-width)')
    p.add_argument('--roi-levels', type=int, default=None, metavar='N',
                   help='with --roi: window sizes between the net\'s size and the frame\'s, 1..64 (default 8)')
    p.add_argument('--roi-margin', type=float, default=None, metavar='F',
                   help='with --roi: pad the mask\'s box by this share of its longer side, 0..4 (default 0.25)')
    p.add_argument('--roi-min-pad', type=int, default=None, metavar='P',
                   help='with --roi: ... and by this many frame pixels, 0..4095 (default 16)')
    p.add_argument('--roi-seed', type=str, default=None, metavar='FILE.png',
                   help='with --roi: the mask the first window is taken from (non-zero = object; the frames\' size)')
    p.add_argument('--refine', action='store_true',
                   help='upsample by the frame\'s own edges: the guided filter on the frame in place of the bilinear upsampling')
    p.add_argument('--refine-radius', type=int, default=None, metavar='N',
                   help='with --refine: the filter\'s window reaches N net pixels to every side, 1..8 (default 4)')
    p.add_argument('--refine-eps', type=float, default=None, metavar='F',
                   help='with --refine: the regulariser beside the guide\'s variance, 1e-3..1e9 (default 400)')
    p.add_argument('--refine-clip', type=float, default=None, metavar='F',
                   help='with --refine: the logits are clipped to [-F, F] first, 0 < F <= 1e4 (default 6)')
    return p


def refine_of(parser: argparse.ArgumentParser, args):
    """The RefineOptions of --refine [--refine-radius --refine-eps --refine-clip], or None without --refine; what it does not go
    with is refused with its reason."""
    for flag, value in (('--refine-radius', args.refine_radius), ('--refine-eps', args.refine_eps),
                        ('--refine-clip', args.refine_clip)):
        if value is not None and not args.refine:
            parser.error('{} is an option of --refine: give --refine'.format(flag))
    if not args.refine:
        return None
    if not args.use_network:
        parser.error('--refine refines the net\'s logits: --no-network runs no net')
    if args.models is not None:
        parser.error('--refine refines the logits of one object (--model): a fit per object in front of the merge (--models) '
                     'is not built')
    if args.roi:
        parser.error('--refine with --roi is not built: the filter\'s guide is the image the net saw, and the guide of a window '
                     'of the frame is not built')
    from fosvos_hip.options import RefineOptions
    given = {k: v for k, v in (('radius', args.refine_radius), ('eps', args.refine_eps), ('clip', args.refine_clip))
             if v is not None}
    try:
        return RefineOptions(**given)
    except ValueError as e:
        parser.error(str(e).replace('RefineOptions: radius', '--refine-radius').replace('RefineOptions: eps', '--refine-eps').replace(
            'RefineOptions: clip', '--refine-clip'))


def roi_of(parser: argparse.ArgumentParser, args, net_size):
    """The RoiOptions of --roi [--roi-levels --roi-margin --roi-min-pad], or None without --roi; what it does not go with is
    refused with its reason."""
    for flag, value in (('--roi-levels', args.roi_levels), ('--roi-margin', args.roi_margin), ('--roi-min-pad', args.roi_min_pad),
                        ('--roi-seed', args.roi_seed)):
        if value is not None and not args.roi:
            parser.error('{} is an option of --roi: give --roi'.format(flag))
    if not args.roi:
        return None
    if not args.use_network:
        parser.error('--roi follows the net\'s mask: --no-network runs no net')
    if args.models is not None:
        parser.error('--roi follows one object (--model): a window around several objects (--models) is not built')
    if args.clean_temporal is not None:
        parser.error('--roi with --clean-temporal is not built: the temporal gate\'s seed lives on the net\'s map, whose '
                     'coordinates move from frame to frame with the window')
    if net_size is None:
        parser.error('--roi needs --net-height and --net-width: a window of the frame is scaled to the net\'s size')
    from fosvos_hip.options import RoiOptions
    given = {k: v for k, v in (('levels', args.roi_levels), ('margin', args.roi_margin), ('min_pad', args.roi_min_pad))
             if v is not None}
    try:
        return RoiOptions(**given)
    except ValueError as e:
        parser.error(str(e).replace('RoiOptions: levels', '--roi-levels').replace('RoiOptions: margin', '--roi-margin').replace(
            'RoiOptions: min_pad', '--roi-min-pad'))


def clean_of(parser: argparse.ArgumentParser, args):
    """The CleanOptions of --clean-min-area / --clean-largest / --clean-temporal, or None when none of them is given; what
    they do not go with is refused with its reason."""
    wanted = args.clean_min_area is not None or args.clean_largest or args.clean_temporal is not None
    if args.clean_seed is not None and args.clean_temporal is None:
        parser.error('--clean-seed is the mask --clean-temporal starts from: give --clean-temporal R')
    if not wanted:
        return None
    if not args.use_network:
        parser.error('--clean-min-area / --clean-largest / --clean-temporal clean the net\'s mask: --no-network runs no net')
    if args.models is not None:
        parser.error('--clean-min-area / --clean-largest / --clean-temporal clean the mask of one object (--model): '
                     'per-object cleaning with --models is not built')
    from fosvos_hip.options import CleanOptions
    try:
        return CleanOptions(min_area=0 if args.clean_min_area is None else args.clean_min_area, largest=args.clean_largest,
                            temporal_radius=args.clean_temporal)
    except ValueError as e:
        parser.error(str(e).replace('CleanOptions: min_area', '--clean-min-area').replace(
            'CleanOptions: temporal_radius', '--clean-temporal'))


def read_seed(path: str) -> np.ndarray:
    """--clean-seed: uint8 [H,W], non-zero = object."""
    from PIL import Image
    with Image.open(path) as im:
        a = np.asarray(im)
    if a.ndim == 3:
        a = a.max(axis=2)
    return np.ascontiguousarray((a != 0).astype(np.uint8))


def net_size_of(parser: argparse.ArgumentParser, args) -> Optional[Tuple[int, int]]:
    """(--net-height, --net-width), or None: both are needed together."""
    if (args.net_height is None) != (args.net_width is None):
        parser.error('--net-height and --net-width are the net\'s size: give both or neither')
    if args.net_height is None:
        return None
    if args.net_height <= 0 or args.net_width <= 0:
        parser.error('--net-height and --net-width must be positive')
    return args.net_height, args.net_width


SINGLE_OBJECT_ONLY = (('--overlay-color', '-oc'), ('--overlay-alpha', '-oa'), ('--no-boolean-mask', '-nbm'))


def check_models(parser: argparse.ArgumentParser, args, argv) -> None:
    """What --models does not go with, each refused with its reason."""
    argv = sys.argv[1:] if argv is None else list(argv)

    def given(names) -> bool:
        return any(a == n or a.startswith(n + '=') for a in argv for n in names)

    if args.model is not None:
        parser.error('--models and --model exclude each other: one object with --model, several with --models')
    if not args.use_network:
        parser.error('--models with --no-network: there would be no net to run')
    for names in SINGLE_OBJECT_ONLY:
        if given(names):
            parser.error('{} belongs to the single-object overlay (one colour channel, soft or boolean); several objects '
                         'are decided by the arg-max and painted with the palette: use --palette-alpha'.format(names[0]))
    if len(args.models) > 16:
        parser.error('--models takes at most 16 files, got {}'.format(len(args.models)))
    if not 0.0 <= args.palette_alpha <= 1.0:
        parser.error('--palette-alpha must be a number in [0, 1], got {}'.format(args.palette_alpha))


def model_file_name(variant: str, version: Optional[int]) -> str:
    """The reference's file names (src/run_webcam.py:43-62)."""
    if variant == 'vgg':
        return 'vgg16.pth'
    if variant == 'resnet':
        return 'resnet{}.pth'.format(34 if version == 34 else 18)
    if variant == 'prune':
        return 'prune_64_1_{}.pth'.format(version)
    if variant == 'mimic':
        raise Exception('Not yet implemented')
    raise Exception('argparse should have prevented this')


def get_network(variant: str, version: Optional[int], path_models: str = 'models', model: Optional[str] = None) -> torch.nn.Module:
    path_file = Path(model) if model is not None else Path(path_models) / model_file_name(variant, version)
    if variant == 'mimic':
        raise Exception('Not yet implemented')

    def keep(storage, loc):
        return storage

    if variant == 'vgg':
        net = OSVOS_VGG(pretrained=False)
        net.load_state_dict(torch.load(str(path_file), map_location=keep))
    elif variant == 'resnet':
        net = OSVOS_RESNET(pretrained=False, version=34 if version == 34 else 18)
        net.load_state_dict(torch.load(str(path_file), map_location=keep))
    elif variant == 'prune':
        net = torch.load(str(path_file), map_location=keep, weights_only=False)  # a whole-module pickle
    else:
        raise Exception('argparse should have prevented this')
    return net


# ---------------------------------------------------------------------------------------------- frame sources
def synthetic_frame(h: int, w: int, index: int) -> np.ndarray:
    """Frame ``index`` of dataloaders/synthetic.py as a camera would deliver it: uint8 [H,W,3] BGR (the mean back on)."""
    img, _ = synthetic.make_frame(h, w, index=index)
    img = img + torch.tensor(MEANVAL).view(3, 1, 1)
    return np.ascontiguousarray(img.round().clamp(0, 255).to(torch.uint8).permute(1, 2, 0).numpy())


def synthetic_frames(n: int, h: int, w: int) -> Iterator[np.ndarray]:
    for k in range(n):
        yield synthetic_frame(h, w, k)


def source_files(directory: str) -> List[str]:
    names = sorted(f for f in os.listdir(directory) if f.lower().endswith(IMAGE_SUFFIXES))
    if not names:
        raise FileNotFoundError('--source {}: no image files'.format(directory))
    return [os.path.join(directory, f) for f in names]


DECODE_GROUP = 8   # files a launch of --device-decode


def bgr_of_bytes(data: bytes) -> np.ndarray:
    """``read_bgr`` of a file that is in memory."""
    import io
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        rgb = np.asarray(im.convert('RGB'))
    return np.ascontiguousarray(rgb[:, :, ::-1])


def avi_frames(path: str) -> Iterator[np.ndarray]:
    from util.mjpeg_avi import AviReader
    for payload in AviReader(path):
        yield bgr_of_bytes(payload)


def device_decoded_frames(items, group: int = DECODE_GROUP) -> Iterator:
    """``items``: (name, bytes or None, host decode) per frame, in order.  Consecutive JPEG files the device decoder takes,
    of one shape and sampling, are decoded ``group`` a launch on the current stream and yielded as uint8 [H,W,3] device
    tensors; everything else, and a file whose status comes back non-zero, as the host decode's array."""
    from fosvos_hip import ops
    from util import jpeg_read
    held = []

    def flush():
        if not held:
            return
        frames, status = ops.jpeg_decode([b for b, _, _ in held], plans=[p for _, p, _ in held])
        codes = status.tolist()
        for k, (_, _, host) in enumerate(held):
            yield frames[k] if codes[k] == 0 else host()
        del held[:]

    for name, blob, host in items:
        plan = jpeg_read.probe(blob) if blob is not None and name.lower().endswith(('.jpg', '.jpeg')) else None
        if plan is not None and plan.components != 3:
            plan = None
        if plan is None or len(held) == group or (held and (held[0][1].height, held[0][1].width, held[0][1].subsampling)
                                                  != (plan.height, plan.width, plan.subsampling)):
            yield from flush()
        if plan is None:
            yield host()
        else:
            held.append((blob, plan, host))
    yield from flush()


def source_items(source: str):
    """The (name, bytes, host decode) items of --source DIR or NAME.avi for ``device_decoded_frames``."""
    if source.lower().endswith('.avi'):
        from util.mjpeg_avi import AviReader
        for k, payload in enumerate(AviReader(source)):
            yield '%05d.jpg' % k, payload, (lambda payload=payload: bgr_of_bytes(payload))
        return
    for path in source_files(source):
        blob = None
        if path.lower().endswith(('.jpg', '.jpeg')):
            with open(path, 'rb') as f:
                blob = f.read()
        yield path, blob, (lambda path=path: read_bgr(path))


def open_webcam(index: int):
    try:
        import cv2
    except ImportError:
        raise RuntimeError('--webcam needs OpenCV (cv2) for the capture and it is not installed: '
                           'read frames from image files with --source DIR instead') from None
    return cv2.VideoCapture(index)


def webcam_frames(cam) -> Iterator[np.ndarray]:
    while True:
        ok, img = cam.read()
        if not ok:
            return
        yield np.ascontiguousarray(img)


# ---------------------------------------------------------------------------------------------- the loop
def write_png(directory: Path, index: int, out: np.ndarray) -> None:
    from PIL import Image
    if out.ndim == 3:
        im = Image.fromarray(np.ascontiguousarray(out[:, :, ::-1]))  # BGR -> RGB
    else:
        im = Image.fromarray(out, mode='L')
    im.save(str(directory / ('%05d.png' % index)))


SUBSAMPLING = {'444': '4:4:4', '420': '4:2:0'}


def write_jpeg_host(directory: Path, index: int, out: np.ndarray, quality: int, subsampling: str = '4:4:4', target=None) -> None:
    """The host path of --output-format jpeg (--no-network): PIL, with the parameters of util/jpeg_layout.py.  ``target``: a
    file object that takes the bytes instead of ``%05d.jpg``."""
    from PIL import Image
    from util import jpeg_layout
    im = Image.fromarray(np.ascontiguousarray(out[:, :, ::-1])) if out.ndim == 3 else Image.fromarray(out, mode='L')
    sampled = subsampling == '4:2:0' and out.ndim == 3
    im.save(target if target is not None else str(directory / ('%05d.jpg' % index)), 'JPEG', quality=quality,
            subsampling=2 if sampled else 0, optimize=False, restart_marker_blocks=jpeg_layout.RI_420 if sampled else jpeg_layout.RI)


def loop_frames(results: Iterator, output: Optional[Path], jpeg_quality: Optional[int] = None, subsampling: str = '4:4:4',
                avi=None, suffix: str = '.jpg') -> List[float]:
    """Takes the results as they come, logs the rate of each (the reference's line) and writes them: arrays as PNGs (as
    JPEGs by PIL where ``jpeg_quality`` is given), ``bytes`` - files the device encoded, named by ``suffix`` - as they are.  ``avi`` (a
    util.mjpeg_avi.AviWriter) takes the JPEG files instead of the directory ``output``."""
    rates = []
    start_time = time.time()
    for index, out in enumerate(results):
        if avi is not None:
            if not isinstance(out, bytes):
                import io
                buf = io.BytesIO()
                write_jpeg_host(None, index, out, jpeg_quality, subsampling, target=buf)
                out = buf.getvalue()
            avi.write(out)
        elif output is not None:
            if isinstance(out, bytes):
                (output / ('%05d%s' % (index, suffix))).write_bytes(out)
            elif jpeg_quality is not None:
                write_jpeg_host(output, index, out, jpeg_quality, subsampling)
            else:
                write_png(output, index, out)
        now = time.time()
        rates.append(1.0 / max(now - start_time, 1e-9))
        log.info('FPS: {0:0.1f}'.format(rates[-1]))
        start_time = now
    if rates:
        log.info('Mean FPS: {0:0.1f} over {1} frames'.format(len(rates) / sum(1.0 / r for r in rates), len(rates)))
    return rates


def chain_first(first: np.ndarray, rest: Iterator[np.ndarray]) -> Iterator[np.ndarray]:
    yield first
    yield from rest


def open_avi(path: str, first: np.ndarray, fps: float):
    """The Motion-JPEG file of --output NAME.avi, sized by the first frame."""
    from util.mjpeg_avi import AviWriter
    parent = os.path.dirname(os.path.abspath(path))
    os.makedirs(parent, exist_ok=True)
    return AviWriter(path, first.shape[1], first.shape[0], fps)


def main(argv=None) -> List[float]:
    parser = build_parser()
    args = parser.parse_args(argv)
    net_size = net_size_of(parser, args)
    clean = clean_of(parser, args)
    from util import args_helper
    motion = args_helper.motion_of(parser, args)  # (--clean-temporal's own refusals come first, in clean_of)
    roi = roi_of(parser, args, net_size)
    refine = refine_of(parser, args)
    if args.models is not None:
        check_models(parser, args, argv)
    if not args.use_cuda:
        raise RuntimeError('--no-cuda: the HIP path has no CPU fallback')
    if args.variant == 'mimic' and args.use_network:
        raise Exception('Not yet implemented')
    if args.source is not None and args.synthetic is not None:
        raise ValueError('choose one of --source and --synthetic')
    jpeg = args.output_format == 'jpeg'
    if jpeg and args.output is None:
        raise ValueError('--output-format jpeg chooses the files of --output: give --output DIR')
    if jpeg and not 1 <= args.jpeg_quality <= 100:
        raise ValueError('--jpeg-quality must be 1..100, got {}'.format(args.jpeg_quality))
    if args.jpeg_subsampling != '444' and not jpeg:
        raise ValueError('--jpeg-subsampling is the chroma sampling of --output-format jpeg')
    subsampling = SUBSAMPLING[args.jpeg_subsampling]
    to_avi = args.output is not None and args.output.lower().endswith('.avi')
    if to_avi and not jpeg:
        raise ValueError('--output NAME.avi is a Motion-JPEG file: give --output-format jpeg')
    if to_avi and not args.fps > 0:
        raise ValueError('--fps must be positive, got {}'.format(args.fps))
    if args.device_decode and args.source is None:
        raise ValueError('--device-decode decodes the JPEG files of --source: give --source DIR or NAME.avi')
    cam = None
    if args.synthetic is not None:
        frames = synthetic_frames(args.synthetic, args.height, args.width)
    elif args.source is not None and args.device_decode:
        frames = device_decoded_frames(source_items(args.source))
    elif args.source is not None and args.source.lower().endswith('.avi'):
        frames = avi_frames(args.source)
    elif args.source is not None:
        frames = (read_bgr(f) for f in source_files(args.source))
    else:
        cam = open_webcam(args.webcam)
        frames = webcam_frames(cam)
    output = None
    if args.output is not None and not to_avi:
        output = Path(args.output)
        output.mkdir(parents=True, exist_ok=True)
    avi = None
    try:
        if not args.use_network:
            if net_size is not None:
                log.info('--net-height / --net-width ignored: --no-network runs no net')
            frames = (f.cpu().numpy() if isinstance(f, torch.Tensor) else f for f in frames)
            mirrored = (np.ascontiguousarray(f[:, ::-1]) if args.mirror else f for f in frames)
            if to_avi:
                first = next(mirrored, None)
                if first is None:
                    return []
                avi = open_avi(args.output, first, args.fps)
                return loop_frames(chain_first(first, mirrored), None, args.jpeg_quality, subsampling, avi=avi)
            if jpeg and subsampling != '4:4:4':
                return loop_frames(mirrored, output, args.jpeg_quality, subsampling)
            return loop_frames(mirrored, output, args.jpeg_quality) if jpeg else loop_frames(mirrored, output)
        if args.models is not None:
            nets = [get_network(args.variant, args.version, model=m).cuda().eval() for m in args.models]
        else:
            net = get_network(args.variant, args.version, model=args.model).cuda().eval()  # (the nets here run eval-mode BatchNorm only)
        first = next(frames, None)
        if first is None:
            return []
        from fosvos_hip.stream import FrameSegmenter, ObjectSegmenter
        encode = dict(encode='jpeg', quality=args.jpeg_quality) if jpeg else {}
        if jpeg and subsampling != '4:4:4':
            encode['subsampling'] = subsampling
        if net_size is not None:
            encode['net_size'] = net_size
        if args.models is not None and not args.overlay and output is not None and not jpeg:
            encode['encode'] = 'png'  # the label maps as palette files, encoded on the device
        if to_avi:
            avi = open_avi(args.output, first, args.fps)
        if args.models is not None:
            with ObjectSegmenter(nets, first.shape[0], first.shape[1], depth=args.depth, mirror=args.mirror,
                                 overlay=args.overlay, alpha=args.palette_alpha, **encode) as seg:
                return loop_frames(seg.segment(chain_first(first, frames)), output, avi=avi,
                                   suffix='.png' if seg.encode == 'png' else '.jpg')
        if clean is not None:  # (absent: the segmenter is constructed exactly as it was)
            encode['clean'] = clean
        if motion is not None:
            encode['motion'] = motion
        if roi is not None:
            encode['roi'] = roi
        if refine is not None:
            encode['refine'] = refine
        with FrameSegmenter(net, first.shape[0], first.shape[1], depth=args.depth, mirror=args.mirror, overlay=args.overlay,
                            boolean_mask=args.boolean_mask, color=args.overlay_color, alpha=args.overlay_alpha, **encode) as seg:
            if args.clean_seed is not None:
                seg.seed(read_seed(args.clean_seed))
            if args.roi_seed is not None:
                seg.seed_window(read_seed(args.roi_seed))
            return loop_frames(seg.segment(chain_first(first, frames)), output, avi=avi)
    finally:
        if avi is not None:
            avi.close()
        if cam is not None:
            cam.release()


if __name__ == '__main__':
    main()
