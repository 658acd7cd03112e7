"""People hidden in frames on the device (``csrc/pave_anon.hip``): the heads or the whole persons
of the poses pixelated or filled before a frame leaves the box.  ``anonymize_nv12`` works on the NV12 surfaces a
hardware decoder handed out, ``anonymize_bgr`` on [H, W, 3] BGR pictures; both in place, one launch per 32 surfaces,
and without reading a device value on the host: the fixed-shape ``dict(bboxes=, kpts=, keep=)`` of
``head.get_bboxes`` is taken as it is.  The usual order is anonymise, then ``draw_poses_*``: a skeleton over a
pixelated person.

The rule is integer-exact.  A pose has a region, a rectangle grown by a radius; the picture is cut into
``cell x cell`` pixel cells from its origin, and every cell a region touches is replaced as a whole, by the rounded
mean of its samples (per plane) or by one colour.  Whole cells only: what is hidden never shows a finer grid than the
cell, and pixelating twice equals pixelating once.
"""
import numpy as np

from . import native, ops
from .render import _bgr_triple, _per_surface, _scales, _surfaces_and_poses, bgr_to_yuv

# K -> the key points of the head, in the orders of ``keypoints.py``: COCO nose, eyes, ears; PoseTrack nose, head
# bottom, head top; CrowdPose head, neck
HEAD_KEYPOINTS = {17: (0, 1, 2, 3, 4), 15: (0, 1, 2), 14: (12, 13)}


def _int_in(v, lo, hi, name):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
        raise ValueError(f'PrivacyStyle: {name} is an integer in {lo} .. {hi}, got {v!r}')
    return int(v)


class PrivacyStyle:
    """What of a pose of K key points is hidden, and how.

    region 'head': the bounding rectangle of the visible `head` key points (built in for K = 17, 15, 14; up to 8
    indices < K otherwise), grown by max(head_scale / 16 of its larger side, head_min / 16 of the larger side of the
    pose's box) + `margin` pixels; a pose without a visible head key point takes its 'person' region
    (fallback='person') or none (fallback='skip').  region 'person': the box, grown by grow / 16 of its larger side
    + `margin` pixels.  mode 'pixelate': every `cell` x `cell` pixel cell (2, 4, 8, 16, 32 or 64) the region touches
    becomes its mean; 'fill': it becomes `fill_color` (B, G, R).  Poses with a box score > `score_thr` count, key
    points with a score > `kpt_thr` are visible.

    The default head region covers a head whose nose is visible; with only the top or the bottom of the head visible
    the disc is centred on an end of the head and may leave a rim of it out: head_min=3 covers that as well."""

    def __init__(self, K, region='head', mode='pixelate', cell=16, fill_color=(0, 0, 0), margin=0, grow=2, head=None,
                 head_scale=12, head_min=2, fallback='person', score_thr=0.3, kpt_thr=0.):
        K = _int_in(K, 1, native.DRAW_MAX_K, 'K')
        for value, name, allowed in ((region, 'region', ('head', 'person')), (mode, 'mode', ('pixelate', 'fill')),
                                     (fallback, 'fallback', ('person', 'skip'))):
            if value not in allowed:
                raise ValueError(f'PrivacyStyle: {name} is one of {allowed}, got {value!r}')
        if isinstance(cell, bool) or cell not in ops.ANON_CELLS:
            raise ValueError(f'PrivacyStyle: cell is one of {ops.ANON_CELLS}, got {cell!r}')
        if head is None:
            head = HEAD_KEYPOINTS.get(K, ())
        try:
            head = tuple(int(k) for k in head)
        except (TypeError, ValueError):
            raise ValueError('PrivacyStyle: head is a list of key-point indices') from None
        if len(head) > native.ANON_MAX_HEAD or any(not 0 <= k < K for k in head):
            raise ValueError(f'PrivacyStyle: head is at most {native.ANON_MAX_HEAD} indices in [0, {K}), got {head}')
        if region == 'head' and not head:
            raise ValueError(f"PrivacyStyle: no built-in head key points for K = {K} (built in: "
                             f"{sorted(HEAD_KEYPOINTS)}); pass head=, or region='person'")
        self.K, self.region, self.mode, self.cell, self.head, self.fallback = K, region, mode, int(cell), head, fallback
        self.fill_color = _bgr_triple(fill_color, 'PrivacyStyle: fill_color')
        self.margin = _int_in(margin, 0, native.ANON_MAX_MARGIN, 'margin')
        self.grow = _int_in(grow, 0, native.ANON_MAX_SIXTEENTHS, 'grow')
        self.head_scale = _int_in(head_scale, 0, native.ANON_MAX_SIXTEENTHS, 'head_scale')
        self.head_min = _int_in(head_min, 0, native.ANON_MAX_SIXTEENTHS, 'head_min')
        self.score_thr, self.kpt_thr = float(score_thr), float(kpt_thr)

    def fill_bytes(self, matrix=None, full_range=False):
        """The 3 bytes 'fill' stores: (B, G, R) (matrix None) or the (Y, U, V) of a matrix and range."""
        if matrix is None:
            return bytes(self.fill_color)
        return bgr_to_yuv(np.asarray(self.fill_color, np.uint8), matrix, full_range).tobytes()


def _gather(surfaces, results, style, who):
    """-> (surfaces, poses, style): lists of one entry per surface, read as the draw calls read them."""
    _, surf, poses = _surfaces_and_poses(surfaces, results, who)
    if style is None:
        style = PrivacyStyle(poses[0][0].shape[1])
    if not isinstance(style, PrivacyStyle):
        raise ValueError(f'{who}: style is a PrivacyStyle')
    for i, (kpts, _, _) in enumerate(poses):
        if kpts.shape[1] != style.K:
            raise ValueError(f'{who}: results[{i}] has K = {kpts.shape[1]}, the style K = {style.K}')
    return surf, poses, style


def _run(kind, items, fills, style):
    ops.anonymize(kind, items, fills, style.head, style.K, region=style.region, mode=style.mode, cell=style.cell,
                  margin=style.margin, grow=style.grow, head_scale=style.head_scale, head_min=style.head_min,
                  fallback=style.fallback, score_thr=style.score_thr, kpt_thr=style.kpt_thr)


def anonymize_nv12(surfaces, width, results, scale_factor=None, style=None, matrix='bt601', full_range=False):
    """Hides the people of `results` in NV12 `surfaces` in place and returns `surfaces`.  surfaces, width, results,
    scale_factor, matrix and full_range: as in ``draw_poses_nv12`` (one value or one per surface; the (bboxes, labels,
    kpts) tuple or dict(bboxes=, kpts=, keep=) per surface); matrix and range only choose the (Y, U, V) of the fill
    colour.  style: a ``PrivacyStyle`` (default: PrivacyStyle(K), pixelated heads).  Luma is averaged over a cell's
    pixels, U and V each over its cell / 2 x cell / 2 chroma samples.  More than 32 surfaces go in several launches."""
    who = 'anonymize_nv12'
    surf, poses, style = _gather(surfaces, results, style, who)
    n = len(surf)
    widths = _per_surface(width, n, 'width', (int, np.integer), who)
    modes = list(zip(_per_surface(matrix, n, 'matrix', str, who),
                     (bool(f) for f in _per_surface(full_range, n, 'full_range', (bool, int), who))))
    scales = _scales(scale_factor, n, who)
    combos = sorted(set(modes))
    fills = [style.fill_bytes(m, f) for m, f in combos]
    _run('nv12', [(s, w, kp, bb, keep, sc, combos.index(md))
                  for s, w, (kp, bb, keep), sc, md in zip(surf, widths, poses, scales, modes)], fills, style)
    return surfaces


def anonymize_bgr(images, results, scale_factor=None, style=None):
    """Hides the people of `results` in [H, W, 3] uint8 BGR device `images` (one tensor or a list, any sizes) in place
    and returns `images`; results, scale_factor and style as in ``anonymize_nv12``.  Each channel is averaged on its
    own."""
    who = 'anonymize_bgr'
    surf, poses, style = _gather(images, results, style, who)
    scales = _scales(scale_factor, len(surf), who)
    _run('bgr', [(s, None, kp, bb, keep, sc, 0) for s, (kp, bb, keep), sc in zip(surf, poses, scales)],
         [style.fill_bytes()], style)
    return images
