"""Command-line flags of the train scripts (reference: src/util/args_helper.py:5-39).

Same flag names and meanings.  The reference declares ``type=Optional[str]`` for -s/-sg/-sgs, which
argparse cannot call; the intended types are used here.  Extensions (not in the
reference, all optional): --n-epochs, --avg-grad-every-n, --synthetic, --height/--width, --parent-model,
--data-parallel, --augment-rotate with --rotate-range / --zoom-range / --rotate-renormalize, --augment-lucid with its --lucid-*
options (refused offline with the reason), --resident-train-set and
--microbatch-group (offline only), --score, --fast-test, --png-fitted, --device-decode,
--multi-object, --objects, --clean-min-area, --clean-largest, --clean-temporal, --adapt-steps with its --adapt-* options,
--ensemble-flip and --ensemble-scales, --crf with its --crf-* options and --crf-joint, --clean-motion with its --motion-*
options (online only).
"""
import argparse
from typing import List, Optional


def _get_base_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(add_help=True)
    parser.add_argument('--gpu-id', default=None, type=int, help='The gpu id to use')
    parser.add_argument('--network', default='vgg16', type=str, choices=['vgg16', 'resnet18', 'resnet34'],
                        help='The network to use (only vgg16 is implemented on the HIP path)')
    parser.add_argument('--no-training', action='store_true', help='skip training')
    parser.add_argument('--no-testing', action='store_true', help='skip testing')
    parser.add_argument('--variant-offline', default=None, type=int, help='version to try')
    parser.add_argument('--eval-speeds', action='store_true', help='evaluates the network speeds')
    # ---- extensions
    parser.add_argument('--n-epochs', default=None, type=int, help='override the hard-coded epoch count')
    parser.add_argument('--avg-grad-every-n', default=None, type=int, help='override gradient accumulation length')
    parser.add_argument('--synthetic', action='store_true',
                        help='run on synthetic frames of --height x --width instead of DAVIS')
    parser.add_argument('--height', default=480, type=int)
    parser.add_argument('--width', default=854, type=int)
    parser.add_argument('--parent-model', default=None, type=str, help='state_dict (.pth) of the parent network')
    parser.add_argument('--data-parallel', action='store_true',
                        help='spread the gradient-accumulation micro-batches over the ranks of a torchrun job '
                             '(RCCL all-reduce per optimizer step)')
    parser.add_argument('--augment-rotate', action='store_true',
                        help='rotate and zoom every training sample about its centre (the reference\'s ScaleNRotate in '
                             'place of its rescale; the frame keeps its size).  The resident loaders warp on the GPU; the '
                             'offline loader without --resident-train-set warps in numpy on the host, slowly (about 0.16 s '
                             'a 480p sample)')
    parser.add_argument('--rotate-range', type=float, nargs=2, default=None, metavar=('LO', 'HI'),
                        help='with --augment-rotate: the angle is drawn from +-(HI - LO) / 2 degrees (default -30 30)')
    parser.add_argument('--zoom-range', type=float, nargs=2, default=None, metavar=('LO', 'HI'),
                        help='with --augment-rotate: the zoom is drawn from 1 +- (HI - LO) / 2 (default 0.75 1.25)')
    parser.add_argument('--rotate-renormalize', action='store_true',
                        help='with --augment-rotate: the reference\'s renormalisation of the warped frame to [0, 1] (off by '
                             'default: the nets are trained on mean-subtracted frames)')
    return parser


# the range options of --augment-lucid: flag suffix -> (LucidOptions field, what it is)
_LUCID_RANGES = (('bg-rotate', 'bg_rots', 'the background\'s angle about the frame\'s centre, in degrees'),
                 ('bg-zoom', 'bg_scales', 'the background\'s zoom factor'),
                 ('fg-rotate', 'fg_rots', 'the object\'s angle about the centre of its box, in degrees'),
                 ('fg-zoom', 'fg_scales', 'the object\'s zoom factor'),
                 ('fg-shift', 'fg_shift', 'the object\'s shift, in widths / heights of its box'),
                 ('contrast', 'contrast', 'the factor on every channel'),
                 ('tint', 'tint', 'the further factor of each channel'),
                 ('brightness', 'brightness', 'what is added to every channel, in grey levels'))
_LUCID_COUNTS = (('dilate', 'the object is painted out with a margin of D pixels (0..31)'),
                 ('smooth', 'smoothing passes over the painted-out hole (0..16)'))


def add_lucid_arguments(parser: argparse.ArgumentParser) -> None:
    """--augment-lucid and its options (the online command line)."""
    from fosvos_hip.options import LucidOptions
    defaults = LucidOptions()
    parser.add_argument('--augment-lucid', action='store_true',
                        help='one-shot augmentation that moves the object against its background (after Lucid Data Dreaming): '
                             'per draw the painted-out background and the object are rotated, zoomed and shifted '
                             'independently, the illumination is changed and the two are composed again on the GPU, in place '
                             'of the rescale (dataloaders/lucid.py)')
    for suffix, field, what in _LUCID_RANGES:
        parser.add_argument('--lucid-' + suffix, type=float, nargs=2, default=None, metavar=('LO', 'HI'),
                            help='with --augment-lucid: {}, drawn from [LO, HI] (default {:g} {:g})'.format(
                                what, *getattr(defaults, field)))
    for name, what in _LUCID_COUNTS:
        parser.add_argument('--lucid-' + name, type=int, default=None, metavar=name[0].upper(),
                            help='with --augment-lucid: {} (default {})'.format(what, getattr(defaults, name)))


def lucid_of(parser: argparse.ArgumentParser, args, is_online: bool):
    """The LucidOptions of --augment-lucid / --lucid-*, or None; what cannot be combined is refused with the reason."""
    fields = {field: getattr(args, 'lucid_' + suffix.replace('-', '_')) for suffix, field, _ in _LUCID_RANGES}
    fields.update({name: getattr(args, 'lucid_' + name) for name, _ in _LUCID_COUNTS})
    flags = {field: '--lucid-' + suffix for suffix, field, _ in _LUCID_RANGES}
    given = [flags.get(name, '--lucid-' + name) for name, v in fields.items() if v is not None]
    if not args.augment_lucid:
        if given:
            parser.error('{} set(s) an option of the lucid augmentation: it needs --augment-lucid'.format(' / '.join(given)))
        return None
    if not is_online:
        parser.error('--augment-lucid is built for the one-shot sample of train_online.py: the offline training set would '
                     'need a filled background per training frame')
    if args.augment_rotate:
        parser.error('--augment-lucid and --augment-rotate both stand in place of the rescale: give one of them')
    if args.synthetic:
        parser.error('--augment-lucid augments DAVIS samples: the loader of --synthetic augments nothing')
    if args.data_parallel:
        parser.error('--augment-lucid is not wired to the sharded loaders of --data-parallel')
    try:
        from fosvos_hip.options import LucidOptions
        return LucidOptions(**{name: (tuple(v) if isinstance(v, list) else v) for name, v in fields.items() if v is not None})
    except ValueError as err:
        parser.error(str(err).replace('LucidOptions: ', '--lucid-*: '))


def _rotate_options(parser: argparse.ArgumentParser, args: argparse.Namespace):
    """``args.rotate``: the RotateOptions of --augment-rotate and its options, or None."""
    given = [flag for flag, on in (('--rotate-range', args.rotate_range is not None), ('--zoom-range', args.zoom_range is not None),
                                   ('--rotate-renormalize', args.rotate_renormalize)) if on]
    if not args.augment_rotate:
        if given:
            parser.error('{} set(s) an option of the rotation: it needs --augment-rotate'.format(' / '.join(given)))
        return None
    if args.synthetic:
        parser.error('--augment-rotate augments DAVIS samples: the loader of --synthetic augments nothing')
    if args.data_parallel:
        parser.error('--augment-rotate is not wired to the sharded loaders of --data-parallel')
    try:
        from fosvos_hip.options import RotateOptions
        defaults = RotateOptions()
        return RotateOptions(rots=defaults.rots if args.rotate_range is None else tuple(args.rotate_range),
                             scales=defaults.scales if args.zoom_range is None else tuple(args.zoom_range),
                             renormalize=bool(args.rotate_renormalize))
    except ValueError as err:
        parser.error(str(err).replace('RotateOptions: ', '--augment-rotate: '))


def add_motion_arguments(parser: argparse.ArgumentParser) -> None:
    """--clean-motion and its options, the same on every command line that has --clean-temporal."""
    parser.add_argument('--clean-motion', action='store_true',
                        help='with --clean-temporal: carry what the frame before kept along the motion of the picture before '
                             'it gates this frame (block matching on the device; util/block_motion.py)')
    parser.add_argument('--motion-block', type=int, default=None, metavar='B',
                        help='with --clean-motion: the side of a block in pixels (8 or 16; default 16)')
    parser.add_argument('--motion-search', type=int, default=None, metavar='S',
                        help='with --clean-motion: a block is looked for up to S pixels away (1..16; default 8)')
    parser.add_argument('--motion-zero-bias', type=int, default=None, metavar='Z',
                        help='with --clean-motion: what a non-zero vector must win by, in sixteenths of a grey level a pixel '
                             '(0..255; default 8)')


def motion_of(parser: argparse.ArgumentParser, args):
    """The MotionOptions of --clean-motion / --motion-*, or None; what cannot be combined is refused with the reason.  (What
    --clean-temporal itself is refused with is said where that flag is checked.)"""
    fields = {'block': args.motion_block, 'search': args.motion_search, 'zero_bias': args.motion_zero_bias}
    given = ['--motion-' + name.replace('_', '-') for name, v in fields.items() if v is not None]
    if given and not args.clean_motion:
        parser.error('{} set(s) an option of the motion-compensated gate: it needs --clean-motion'.format(' / '.join(given)))
    if not args.clean_motion:
        return None
    if args.clean_temporal is None:
        parser.error('--clean-motion carries the seed of the temporal gate along the picture\'s motion: it needs '
                     '--clean-temporal R')
    try:
        from fosvos_hip.options import MotionOptions
        return MotionOptions(**{name: v for name, v in fields.items() if v is not None})
    except ValueError as err:
        parser.error(str(err).replace('MotionOptions: ', '--motion-*: '))


def parse_args(is_online: bool, argv: Optional[List[str]] = None) -> argparse.Namespace:
    parser = _get_base_parser()
    if is_online:
        parser.add_argument('-s', '--sequence-name', default=None, type=str)
        parser.add_argument('-sg', '--sequence-group', default=None, type=int)
        parser.add_argument('-sgs', '--sequence-group-size', default=None, type=int)
        parser.add_argument('--variant-online', default=None, type=int, help='version to try')
        parser.add_argument('--score', action='store_true',
                            help='score the test pass on the device (DAVIS 2016 J and F per sequence, scores.yml beside '
                                 'the PNGs)')
        parser.add_argument('--fast-test', action='store_true',
                            help='test pass in groups of frames with the PNG files encoded on the device (same pixels, '
                                 'larger files of many IDAT chunks)')
        parser.add_argument('--png-fitted', action='store_true',
                            help='with --fast-test: Huffman codes fitted to each segment of the PNG files (same pixels, '
                                 'smaller files)')
        parser.add_argument('--device-decode', action='store_true',
                            help='decode the test pass\'s JPEG frames on the device (same tensors; files the device decoder '
                                 'does not take go through PIL as before)')
        parser.add_argument('--multi-object', action='store_true',
                            help='several objects a sequence (a DAVIS 2017 tree): one net per object, fine-tuned on that '
                                 'object against everything else; the test pass merges the nets\' answers into palette PNGs '
                                 'on the device and scores J and F per object')
        parser.add_argument('--clean-min-area', type=int, default=None, metavar='N',
                            help='with --fast-test: clean each mask on the device, dropping connected components of fewer '
                                 'than N pixels')
        parser.add_argument('--clean-largest', action='store_true',
                            help='with --fast-test: clean each mask on the device, keeping its largest component only')
        parser.add_argument('--clean-temporal', type=int, default=None, metavar='R',
                            help='with --fast-test: keep only components within R (0..63) pixels of what the frame before '
                                 'kept; the first frame is gated by the training annotation')
        add_motion_arguments(parser)
        parser.add_argument('--adapt-steps', type=int, default=None, metavar='N',
                            help='online adaptation in the test pass: N (>= 1) fine-tune steps on every frame against '
                                 'pseudo-labels made from the net\'s own output (confident pixels positive, pixels far from '
                                 'the last mask negative, the rest ignored); the net leaves the pass adapted')
        parser.add_argument('--adapt-pos-prob', type=float, default=None, metavar='P',
                            help='with --adapt-steps: probability from which a pixel is a positive (0.5 < P < 1; default 0.97)')
        parser.add_argument('--adapt-distance', type=int, default=None, metavar='D',
                            help='with --adapt-steps: pixels further than D (0..4095) from the eroded last mask are negatives '
                                 '(default 220)')
        parser.add_argument('--adapt-erode', type=int, default=None, metavar='E',
                            help='with --adapt-steps: the last mask is eroded by the disk of radius E (0..4095) first '
                                 '(default 15)')
        parser.add_argument('--adapt-frame-weight', type=float, default=None, metavar='W',
                            help='with --adapt-steps: weight of the current frame\'s loss in a step (> 0; default 1)')
        parser.add_argument('--adapt-first-weight', type=float, default=None, metavar='W',
                            help='with --adapt-steps: weight of the annotated first frame\'s loss in a step (>= 0; default 1)')
        parser.add_argument('--adapt-lr', type=float, default=None, metavar='LR',
                            help='with --adapt-steps: learning rate of the adaptation steps (default: the online loop\'s, 1e-8)')
        parser.add_argument('--ensemble-flip', action='store_true',
                            help='with --fast-test or --multi-object: test-time ensemble - the net also sees every frame '
                                 'mirrored, and the logits are averaged on the device')
        parser.add_argument('--ensemble-scales', type=float, nargs='+', default=None, metavar='S',
                            help='with --fast-test or --multi-object: test-time ensemble - the net sees every frame at these '
                                 'sizes (distinct factors in [0.25, 4], e.g. 0.75 1 1.25), and the logits are averaged on '
                                 'the frame\'s grid on the device; at most 8 views with --ensemble-flip counted in')
        parser.add_argument('--crf', action='store_true',
                            help='with --fast-test or --multi-object: refine the logits with a local CRF on the frame\'s '
                                 'colours on the device (mean-field over a window; util/mask_crf.py), before cleaning, merging, '
                                 'scoring and the PNG files')
        parser.add_argument('--crf-joint', action='store_true',
                            help='with --crf and --multi-object: ONE joint CRF over the labels 0..K (util/label_crf.py) in the '
                                 'place of a CRF per net and the label merge: the objects compete at every pixel')
        parser.add_argument('--crf-iterations', type=int, default=None, metavar='N',
                            help='with --crf: mean-field iterations (1..10; default 5)')
        parser.add_argument('--crf-radius', type=int, default=None, metavar='R',
                            help='with --crf: the window reaches R pixels to every side (1..5; default 5)')
        parser.add_argument('--crf-theta-pos', type=float, default=None, metavar='F',
                            help='with --crf: width of the appearance kernel in pixels ([0.25, 1000]; default 8)')
        parser.add_argument('--crf-theta-rgb', type=float, default=None, metavar='F',
                            help='with --crf: width of the appearance kernel in grey levels ([1, 1000]; default 13)')
        parser.add_argument('--crf-theta-smooth', type=float, default=None, metavar='F',
                            help='with --crf: width of the smoothness kernel in pixels ([0.25, 1000]; default 3)')
        parser.add_argument('--crf-weight-appearance', type=float, default=None, metavar='F',
                            help='with --crf: weight of the appearance kernel\'s message ([0, 100]; default 4)')
        parser.add_argument('--crf-weight-smooth', type=float, default=None, metavar='F',
                            help='with --crf: weight of the smoothness kernel\'s message ([0, 100]; default 3)')
        parser.add_argument('--crf-clip', type=float, default=None, metavar='F',
                            help='with --crf: the logits are clipped to [-F, F] first ((0, 10000]; default 6)')
        parser.add_argument('--objects', default=2, type=int, metavar='K',
                            help='with --multi-object --synthetic: the number of objects of the synthetic sequence (1..16)')
    if not is_online:
        parser.add_argument('--resident-train-set', action='store_true',
                            help='decode the training set once, keep it on the GPU and flip / rescale each draw there '
                                 '(same samples as the per-iteration DataLoader under the same seed)')
        parser.add_argument('--microbatch-group', default=1, type=int, metavar='N',
                            help='run the one-frame minibatches of an accumulation cycle as batched passes of up to N '
                                 'frames of one shape (every frame keeps the class weights of its own label; 1 = one '
                                 'minibatch per pass, the reference\'s order)')
    add_lucid_arguments(parser)
    args = parser.parse_args(argv)
    args.rotate = _rotate_options(parser, args)
    args.lucid = lucid_of(parser, args, is_online)
    if not is_online and args.microbatch_group < 1:
        parser.error('--microbatch-group counts frames per pass: at least 1')
    if not is_online and args.microbatch_group > 1 and args.data_parallel:
        parser.error('--microbatch-group above 1 does not combine with --data-parallel (that mode splits every batch with '
                     'class counts of the whole batch)')
    if is_online and args.multi_object:
        if args.eval_speeds:
            parser.error('--multi-object is a PNG-writing test pass of K nets; --eval-speeds times one net and writes nothing')
        if args.data_parallel:
            parser.error('--multi-object fine-tunes K nets one after the other on one device; --data-parallel spreads ONE '
                         'net\'s accumulation cycle over the ranks')
        if args.device_decode:
            parser.error('--multi-object reads its frames through the host loader; --device-decode is not wired to it')
        if not 1 <= args.objects <= 16:
            parser.error('--objects counts the objects of the synthetic sequence: 1..16')
    if is_online and args.png_fitted and not args.fast_test and not args.multi_object and args.adapt_steps is None:
        parser.error('--png-fitted chooses the codes of the device PNG encoder: it needs --fast-test')
    if is_online and (args.clean_min_area is not None or args.clean_largest or args.clean_temporal is not None):
        if args.multi_object:
            parser.error('--clean-min-area / --clean-largest / --clean-temporal clean the mask of one object; per-object '
                         'cleaning under --multi-object is not built')
        if not args.fast_test:
            parser.error('--clean-min-area / --clean-largest / --clean-temporal clean the logits of the device test pass: '
                         'they need --fast-test')
        if args.clean_min_area is not None and args.clean_min_area < 0:
            parser.error('--clean-min-area must be >= 0, got {}'.format(args.clean_min_area))
        if args.clean_temporal is not None and not 0 <= args.clean_temporal <= 63:
            parser.error('--clean-temporal must be 0..63, got {}'.format(args.clean_temporal))
    if is_online:
        args.motion = motion_of(parser, args)
    if is_online:
        given = [flag for flag, v in (('--adapt-pos-prob', args.adapt_pos_prob), ('--adapt-distance', args.adapt_distance),
                                      ('--adapt-erode', args.adapt_erode), ('--adapt-frame-weight', args.adapt_frame_weight),
                                      ('--adapt-first-weight', args.adapt_first_weight), ('--adapt-lr', args.adapt_lr))
                 if v is not None]
        if args.adapt_steps is None and given:
            parser.error('{} set(s) an option of online adaptation: it needs --adapt-steps'.format(' / '.join(given)))
        if args.adapt_steps is not None:
            if args.adapt_steps < 1:
                parser.error('--adapt-steps counts fine-tune steps per frame: at least 1, got {}'.format(args.adapt_steps))
            if args.multi_object:
                parser.error('--adapt-steps adapts ONE net to its own output; adaptation of the K nets of --multi-object '
                             'is not built')
            if args.data_parallel:
                parser.error('--adapt-steps trains inside the test pass, frame by frame on one device; --data-parallel '
                             'spreads a training cycle over the ranks')
            if args.eval_speeds:
                parser.error('--adapt-steps is a PNG-writing test pass that trains; --eval-speeds times a frozen net and '
                             'writes nothing')
            if args.device_decode:
                parser.error('--adapt-steps reads its frames through the host loader; --device-decode is not wired to it')
            if args.clean_min_area is not None or args.clean_largest or args.clean_temporal is not None:
                parser.error('--adapt-steps trains the net on the stray blobs that --clean-min-area / --clean-largest / '
                             '--clean-temporal would filter from the output; the two are not combined')
            try:
                from fosvos_hip.options import AdaptOptions
                defaults = AdaptOptions()
                args.adapt = AdaptOptions(
                    steps=args.adapt_steps,
                    pos_prob=defaults.pos_prob if args.adapt_pos_prob is None else args.adapt_pos_prob,
                    neg_distance=defaults.neg_distance if args.adapt_distance is None else args.adapt_distance,
                    erode=defaults.erode if args.adapt_erode is None else args.adapt_erode,
                    frame_weight=defaults.frame_weight if args.adapt_frame_weight is None else args.adapt_frame_weight,
                    first_weight=defaults.first_weight if args.adapt_first_weight is None else args.adapt_first_weight,
                    learning_rate=defaults.learning_rate if args.adapt_lr is None else args.adapt_lr)
            except ValueError as err:
                parser.error(str(err).replace('AdaptOptions: ', '--adapt-*: '))
        else:
            args.adapt = None
    if is_online:
        args.ensemble = None
        if args.ensemble_flip or args.ensemble_scales is not None:
            if not args.fast_test and not args.multi_object:
                parser.error('--ensemble-flip / --ensemble-scales average the logits of the device test pass: they need '
                             '--fast-test or --multi-object')
            if args.adapt_steps is not None:
                parser.error('--ensemble-flip / --ensemble-scales average the answers of a frozen net; adaptation of an '
                             'ensemble (--adapt-steps) is not built')
            if args.eval_speeds:
                parser.error('--ensemble-flip / --ensemble-scales belong to a PNG-writing test pass; --eval-speeds times one '
                             'forward and writes nothing')
            if args.data_parallel:
                parser.error('--ensemble-flip / --ensemble-scales run every view on one device; --data-parallel spreads a '
                             'training cycle over the ranks')
            try:
                from fosvos_hip.options import EnsembleOptions
                args.ensemble = EnsembleOptions(flip=bool(args.ensemble_flip),
                                                scales=(1.0,) if args.ensemble_scales is None else tuple(args.ensemble_scales))
            except ValueError as err:
                parser.error(str(err).replace('EnsembleOptions: ', '--ensemble-*: '))
    if is_online:
        args.crf_options = None
        fields = {'iterations': args.crf_iterations, 'radius': args.crf_radius, 'theta_pos': args.crf_theta_pos,
                  'theta_rgb': args.crf_theta_rgb, 'theta_smooth': args.crf_theta_smooth,
                  'weight_appearance': args.crf_weight_appearance, 'weight_smooth': args.crf_weight_smooth,
                  'clip': args.crf_clip}
        given = ['--crf-' + name.replace('_', '-') for name, v in fields.items() if v is not None]
        if given and not args.crf:
            parser.error('{} set(s) an option of the CRF: it needs --crf'.format(' / '.join(given)))
        if args.crf_joint and not args.crf:
            parser.error('--crf-joint is the joint form of the CRF: it needs --crf')
        if args.crf_joint and not args.multi_object:
            parser.error('--crf-joint lets the objects of a frame compete: it needs --multi-object (the single-object pass of '
                         '--fast-test has one object)')
        if args.crf:
            if not args.fast_test and not args.multi_object:
                parser.error('--crf refines the logits of the device test pass: it needs --fast-test or --multi-object')
            if args.adapt_steps is not None:
                parser.error('--crf refines the answers of a frozen net; a CRF in the adaptive test pass (--adapt-steps) is '
                             'not built')
            if args.eval_speeds:
                parser.error('--crf belongs to a PNG-writing test pass; --eval-speeds times one forward and writes nothing')
            if args.data_parallel:
                parser.error('--crf runs in the test pass on one device; --data-parallel spreads a training cycle over the '
                             'ranks')
            try:
                from fosvos_hip.options import CrfOptions
                args.crf_options = CrfOptions(**{name: v for name, v in fields.items() if v is not None})
            except ValueError as err:
                parser.error(str(err).replace('CrfOptions: ', '--crf-*: '))
    if is_online and args.device_decode and args.synthetic:
        parser.error('--device-decode decodes JPEG files: the synthetic sequence has none')
    args.is_training = not args.no_training
    args.is_testing = not args.no_testing
    return args
