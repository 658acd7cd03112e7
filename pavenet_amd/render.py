"""Poses drawn into frames on the device (``csrc/pave_draw.hip``): the way back out of the live
path.  ``draw_poses_nv12`` writes into the NV12 surfaces a hardware decoder handed out (and an encoder takes back),
``draw_poses_bgr`` into [H, W, 3] BGR pictures; ``VideoPoseV1.show_result`` / ``PETR.show_result`` are the
reference's public method on top of the latter (opera/models/detectors/videoposev1.py:263-512, a matplotlib loop on
the host there).  Drawing is in place, one launch per 32 surfaces, and reads no device value on the host: the
fixed-shape ``dict(bboxes=, kpts=, keep=)`` of ``head.get_bboxes`` is drawn without the sync of ``results_to_list``.

Hard-edged integer coverage (no anti-aliasing, no blending; the only text is the digits of a track id; zones, lines
and their counts are ``overlay.py``'s).  With ``ids=`` (what ``PoseTracker.update`` returns, still on the device) a tracked pose takes a colour chosen by its id and
a small plate with the id above its box (``TrackStyle``).  Skeletons are written from the key-point
orders of ``keypoints.py`` (PoseTrack: nose, head bottom, head top, then left / right shoulder, elbow, wrist, hip,
knee, ankle); the palette is this project's: left limbs warm, right limbs cool, the middle green.
"""
import numpy as np
import torch

from . import native, ops
from .preprocess import NV12_MATRICES

# ---- skeletons: K -> (edges, side of every key point: 'l' | 'r' | 'c') ----
_COCO = ([(0, 1), (0, 2), (1, 3), (2, 4), (3, 5), (4, 6), (5, 6), (5, 7), (7, 9), (6, 8), (8, 10), (5, 11), (6, 12),
          (11, 12), (11, 13), (13, 15), (12, 14), (14, 16)], 'c' + 'lr' * 8)
_POSETRACK = ([(2, 0), (0, 1), (1, 3), (1, 4), (3, 5), (5, 7), (4, 6), (6, 8), (3, 9), (4, 10), (9, 10), (9, 11),
               (11, 13), (10, 12), (12, 14)], 'ccc' + 'lr' * 6)
_CROWDPOSE = ([(12, 13), (13, 0), (13, 1), (0, 2), (2, 4), (1, 3), (3, 5), (0, 6), (1, 7), (6, 7), (6, 8), (8, 10),
               (7, 9), (9, 11)], 'lr' * 6 + 'cc')
# BGR
LIMB_COLORS = {'l': (48, 132, 255), 'r': (255, 168, 56), 'c': (96, 214, 120)}
KPT_COLORS = {'l': (120, 186, 255), 'r': (255, 208, 140), 'c': (170, 240, 186)}
BBOX_COLOR = (72, 101, 241)
# BGR, one per track: id v takes row (v - 1) % 32.  Hues 11 / 32 of the circle apart from one id to the next, two
# brightness and two saturation levels; every colour is at least 64 of 255 darker in BT.601 luma than white ink.
TRACK_PALETTE = (
    (36, 36, 242), (37, 184, 28), (242, 97, 115), (73, 94, 184), (88, 242, 36), (184, 28, 76), (97, 151, 242),
    (122, 184, 73), (242, 36, 139), (28, 115, 184), (172, 221, 89), (184, 73, 149), (34, 178, 226), (154, 184, 28),
    (242, 97, 224), (73, 177, 184), (236, 236, 35), (174, 28, 184), (77, 194, 179), (184, 163, 73), (191, 36, 242),
    (28, 184, 135), (242, 188, 97), (135, 73, 184), (34, 227, 130), (184, 96, 28), (151, 97, 242), (73, 184, 108),
    (242, 88, 36), (57, 28, 184), (91, 227, 108), (184, 80, 73))
# The one definition of the digit face: 10 digits x 7 rows of 5 bits, bit 4 the left-most pixel.  It travels to the
# kernel in the plan and to the oracle as an argument.
DIGIT_FONT = tuple(tuple(int(row.replace('.', '0').replace('#', '1'), 2) for row in face.split()) for face in (
    '.###. #...# #..## #.#.# ##..# #...# .###.',
    '..#.. .##.. ..#.. ..#.. ..#.. ..#.. .###.',
    '.###. #...# ....# ...#. ..#.. .#... #####',
    '####. ....# ....# .###. ....# ....# ####.',
    '...#. ..##. .#.#. #..#. ##### ...#. ...#.',
    '##### #.... ####. ....# ....# #...# .###.',
    '..##. .#... #.... ####. #...# #...# .###.',
    '##### ....# ...#. ..#.. .#... .#... .#...',
    '.###. #...# #...# .###. #...# #...# .###.',
    '.###. #...# #...# .#### ....# ...#. .##..'))
# The 11th face, for counts that can be negative (overlay.py: a line's forward - backward): same cell, same encoding.
MINUS_FACE = tuple(int(row.replace('.', '0').replace('#', '1'), 2) for row in
                   '..... ..... ..... ##### ..... ..... .....'.split())


def _builtin(K):
    edges, sides = {17: _COCO, 15: _POSETRACK, 14: _CROWDPOSE}[K]
    limb = [LIMB_COLORS[sides[a] if sides[a] == sides[b] else 'c'] for a, b in edges]
    return list(edges), limb, [KPT_COLORS[s] for s in sides]


SKELETONS = {K: _builtin(K) for K in (17, 15, 14)}   # K -> (edges, edge_colors, kpt_colors)


def _bgr_triple(c, what):
    try:
        c = tuple(int(v) for v in c)
    except (TypeError, ValueError):
        c = ()
    if len(c) != 3 or not all(0 <= v <= 255 for v in c):
        raise ValueError(f'{what} must be three 8-bit values (B, G, R)')
    return c


def bgr_to_yuv(bgr, matrix='bt601', full_range=False):
    """8-bit (B, G, R) [..., 3] -> 8-bit (Y, U, V) of the Y'CbCr `matrix` ('bt601' | 'bt709') and range, in double:
    the forward transform of which ``preprocess.nv12_csc`` is the inverse.
      Y' = Kr R + Kg G + Kb B;  Y = rint(yoff + Y' / cy);  U = rint(128 + (B - Y') / (2 (1 - Kb)) / q);
      V = rint(128 + (R - Y') / (2 (1 - Kr)) / q);  each clamped to 0 .. 255
    with (yoff, cy, q) = (16, 255 / 219, 255 / 224) in limited range and (0, 1, 1) in full range."""
    if matrix not in NV12_MATRICES:
        raise ValueError(f'bgr_to_yuv: unknown matrix {matrix!r} (one of {sorted(NV12_MATRICES)})')
    x = np.asarray(bgr, dtype=np.float64)
    if x.shape[-1:] != (3,):
        raise ValueError('bgr_to_yuv: [..., 3] (B, G, R)')
    kr, kb = NV12_MATRICES[matrix]
    kg = 1.0 - kr - kb
    yoff, cy, q = (0.0, 1.0, 1.0) if full_range else (16.0, 255.0 / 219.0, 255.0 / 224.0)
    b, g, r = x[..., 0], x[..., 1], x[..., 2]
    yp = kr * r + kg * g + kb * b
    yuv = np.stack([np.rint(yoff + yp / cy), np.rint(128.0 + (b - yp) / (2.0 * (1.0 - kb)) / q),
                    np.rint(128.0 + (r - yp) / (2.0 * (1.0 - kr)) / q)], axis=-1)
    return np.clip(yuv, 0, 255).astype(np.uint8)


class PoseStyle:
    """How poses of K key points are drawn: line `thickness` 1 .. 32 px, disc `radius` 0 .. 32 px (0: no discs), poses
    with a box score > `score_thr`, key points with a score > `kpt_thr`, boxes only with `draw_boxes`.
    `skeleton=(edges, edge_colors, kpt_colors)` (K <= 32, at most 32 edges of indices < K, 8-bit BGR colours)
    replaces the built-in skeleton of K = 17 (COCO), 15 (PoseTrack) or 14 (CrowdPose)."""

    def __init__(self, K, thickness=4, radius=4, score_thr=0.3, kpt_thr=0., draw_boxes=False, skeleton=None,
                 bbox_color=BBOX_COLOR):
        K = int(K)
        if skeleton is None:
            if K not in SKELETONS:
                raise ValueError(f'PoseStyle: no built-in skeleton for K = {K} (built in: {sorted(SKELETONS)}); pass '
                                 'skeleton=(edges, edge_colors, kpt_colors)')
            skeleton = SKELETONS[K]
        if not 1 <= K <= native.DRAW_MAX_K:
            raise ValueError(f'PoseStyle: K in 1 .. {native.DRAW_MAX_K}, got {K}')
        try:
            edges, edge_colors, kpt_colors = skeleton
            edges = [(int(a), int(b)) for a, b in edges]
        except (TypeError, ValueError):
            raise ValueError('PoseStyle: skeleton is (edges, edge_colors, kpt_colors), edges pairs of indices') from None
        if len(edges) > native.DRAW_MAX_E:
            raise ValueError(f'PoseStyle: at most {native.DRAW_MAX_E} edges, got {len(edges)}')
        if any(not (0 <= a < K and 0 <= b < K) for a, b in edges):
            raise ValueError(f'PoseStyle: an edge index outside [0, {K})')
        if len(edge_colors) != len(edges) or len(kpt_colors) != K:
            raise ValueError(f'PoseStyle: one colour per edge ({len(edges)}) and per key point ({K}), got '
                             f'{len(edge_colors)} and {len(kpt_colors)}')
        if int(thickness) != thickness or not 1 <= thickness <= 32:
            raise ValueError(f'PoseStyle: thickness is an integer in 1 .. 32, got {thickness!r}')
        if int(radius) != radius or not 0 <= radius <= 32:
            raise ValueError(f'PoseStyle: radius is an integer in 0 .. 32, got {radius!r}')
        self.K, self.edges = K, edges
        self.edge_colors = [_bgr_triple(c, 'PoseStyle: an edge colour') for c in edge_colors]
        self.kpt_colors = [_bgr_triple(c, 'PoseStyle: a key-point colour') for c in kpt_colors]
        self.bbox_color = _bgr_triple(bbox_color, 'PoseStyle: bbox_color')
        self.thickness, self.radius = int(thickness), int(radius)
        self.score_thr, self.kpt_thr, self.draw_boxes = float(score_thr), float(kpt_thr), bool(draw_boxes)

    def color_table(self, convert=None):
        """The [65, 3] table of the draw plan (row 0 boxes, 1 .. 32 limbs, 33 .. 64 key points), through `convert`
        ([n, 3] BGR -> [n, 3] bytes to store) when given."""
        table = np.zeros((native.DRAW_COLORS, 3), dtype=np.uint8)
        table[0] = self.bbox_color
        if self.edges:
            table[1:1 + len(self.edges)] = self.edge_colors
        table[1 + native.DRAW_MAX_E:1 + native.DRAW_MAX_E + self.K] = self.kpt_colors
        return (table if convert is None else convert(table)).tolist()

    def table_bytes(self, matrix=None, full_range=False):
        """color_table as the 195 bytes of the plan: BGR (matrix None) or the (Y, U, V) of a matrix and range; kept
        per colour set, so a style drawn every frame converts its colours once."""
        key = (matrix, bool(full_range), tuple(self.edge_colors), tuple(self.kpt_colors), self.bbox_color)
        cache = self.__dict__.setdefault('_tables', {})
        if key not in cache:
            convert = None if matrix is None else (lambda t: bgr_to_yuv(t, matrix, full_range))
            cache[key] = bytes(c for row in self.color_table(convert) for c in row)
        return cache[key]


class TrackStyle(PoseStyle):
    """PoseStyle for poses with track ids: a pose with id v >= 1 has its limbs (and box) in `palette[(v - 1) % 32]`
    (32 BGR colours; the key points keep the style's colours) and, with `label_scale` g in 1 .. 8, a plate of that
    colour above its box with v in decimal digits of `label_color`, a font pixel g x g picture pixels; g = 0: colours
    only.  `untracked`: a pose with id <= 0 is drawn as PoseStyle draws it ('style') or not at all ('skip').  The
    other arguments are PoseStyle's."""

    def __init__(self, K, palette=TRACK_PALETTE, label_scale=2, label_color=(255, 255, 255), untracked='style', **kw):
        super().__init__(K, **kw)
        try:
            palette = list(palette)
        except TypeError:
            palette = []
        if len(palette) != native.DRAW_PALETTE:
            raise ValueError(f'TrackStyle: palette is {native.DRAW_PALETTE} colours, got {len(palette)}')
        self.palette = [_bgr_triple(c, 'TrackStyle: a palette colour') for c in palette]
        self.label_color = _bgr_triple(label_color, 'TrackStyle: label_color')
        if isinstance(label_scale, bool) or not isinstance(label_scale, (int, np.integer)) or not 0 <= label_scale <= 8:
            raise ValueError(f'TrackStyle: label_scale is an integer in 0 .. 8, got {label_scale!r}')
        if untracked not in ('style', 'skip'):
            raise ValueError(f"TrackStyle: untracked is 'style' or 'skip', got {untracked!r}")
        self.label_scale, self.untracked = int(label_scale), untracked

    def palette_bytes(self, matrix=None, full_range=False):
        """The 99 bytes of the ids plan (rows 0 .. 31 the palette, row 32 the ink): BGR (matrix None) or the
        (Y, U, V) of a matrix and range; kept per colour set like table_bytes."""
        key = ('palette', matrix, bool(full_range), tuple(self.palette), self.label_color)
        cache = self.__dict__.setdefault('_tables', {})
        if key not in cache:
            table = np.asarray(self.palette + [self.label_color], dtype=np.uint8)
            if matrix is not None:
                table = bgr_to_yuv(table, matrix, full_range)
            cache[key] = table.tobytes()
        return cache[key]


def _per_surface(v, n, name, scalar, who):
    if isinstance(v, scalar):
        return [v] * n
    v = list(v)
    if len(v) != n:
        raise ValueError(f'{who}: {name} is one value or one per surface ({n}), got {len(v)}')
    return v


def _is_number(v):
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool)


def _one_scale(v, who):
    if _is_number(v):
        return float(v), float(v)
    v = list(np.asarray(v).reshape(-1)) if isinstance(v, np.ndarray) else list(v)
    if len(v) not in (2, 4) or not all(_is_number(x) for x in v):
        raise ValueError(f"{who}: a scale factor is a number, (sx, sy) or an img_meta's (sx, sy, sx, sy)")
    return float(v[0]), float(v[1])


def _scales(scale_factor, n, who):
    """None -> (1, 1); a number, an (sx, sy) or an img_meta's 4-tuple -> that for every surface; else one per surface."""
    if scale_factor is None:
        return [(1.0, 1.0)] * n
    flat = _is_number(scale_factor) or (len(scale_factor) in (2, 4) and all(_is_number(x) for x in scale_factor))
    if flat:
        return [_one_scale(scale_factor, who)] * n
    if len(scale_factor) != n:
        raise ValueError(f'{who}: scale_factor is one value or one per surface ({n}), got {len(scale_factor)}')
    return [_one_scale(v, who) for v in scale_factor]


def _poses(result, i, who):
    """One surface's result -> (kpts [N, K, 3], bboxes [N, 5], keep [N] | None): the (bboxes, labels, kpts) tuple of
    push() / infer_video, or the fixed-shape dict(bboxes=, kpts=, keep=) of head.get_bboxes (a leading batch axis of
    one is dropped)."""
    if isinstance(result, dict):
        if 'bboxes' not in result or 'kpts' not in result:
            raise ValueError(f'{who}: results[{i}] needs bboxes and kpts')
        bboxes, kpts, keep = result['bboxes'], result['kpts'], result.get('keep')
    elif isinstance(result, (tuple, list)) and len(result) == 3:
        bboxes, kpts, keep = result[0], result[2], None
    else:
        raise ValueError(f'{who}: results[{i}] is a (bboxes, labels, kpts) tuple or a dict(bboxes=, kpts=, keep=)')
    for t, name in ((bboxes, 'bboxes'), (kpts, 'kpts'), (keep, 'keep')):
        if not (isinstance(t, torch.Tensor) or (t is None and name == 'keep')):
            raise ValueError(f'{who}: {name} of results[{i}] must be a tensor')
    if bboxes.dim() == 3 and bboxes.shape[0] == 1 and kpts.dim() == 4 and kpts.shape[0] == 1:
        bboxes, kpts, keep = bboxes[0], kpts[0], (keep[0] if keep is not None and keep.dim() == 2 else keep)
    if kpts.dim() != 3 or kpts.shape[2] != 3 or bboxes.dim() != 2 or tuple(bboxes.shape) != (kpts.shape[0], 5):
        raise ValueError(f'{who}: results[{i}] needs kpts [N, K, 3] and bboxes [N, 5], got {tuple(kpts.shape)} and '
                         f'{tuple(bboxes.shape)}')
    if kpts.dtype != torch.float32 or bboxes.dtype != torch.float32:
        raise ValueError(f'{who}: kpts and bboxes of results[{i}] must be float32')
    if keep is not None and (keep.dtype != torch.int32 or tuple(keep.shape) != (kpts.shape[0],)):
        raise ValueError(f'{who}: keep of results[{i}] must be int32 [{kpts.shape[0]}]')
    return kpts.contiguous(), bboxes.contiguous(), None if keep is None else keep.contiguous()


def _surfaces_and_poses(surfaces, results, who):
    """One tensor and its result, or lists of them -> (single, surfaces, poses): lists of one entry per surface."""
    single = isinstance(surfaces, torch.Tensor)
    surf = [surfaces] if single else (list(surfaces) if isinstance(surfaces, (list, tuple)) else None)
    if not surf:
        raise ValueError(f'{who}: one uint8 tensor or a non-empty list of them')
    results = [results] if single else (list(results) if isinstance(results, (list, tuple)) else None)
    if results is None or len(results) != len(surf):
        raise ValueError(f'{who}: one result per surface ({len(surf)})')
    return single, surf, [_poses(r, i, who) for i, r in enumerate(results)]


def _gather(surfaces, results, style, who, ids=None):
    """-> (surfaces, poses, style, ids): lists of one entry per surface; ids None when the call has none."""
    single, surf, poses = _surfaces_and_poses(surfaces, results, who)
    K = poses[0][0].shape[1]
    if ids is not None:
        ids = [ids] if single and isinstance(ids, torch.Tensor) else (list(ids) if isinstance(ids, (list, tuple)) else None)
        if ids is None or len(ids) != len(surf):
            raise ValueError(f'{who}: ids is one tensor for one surface, or a list of a tensor or None per surface '
                             f'({len(surf)})')
        if any(not (v is None or isinstance(v, torch.Tensor)) for v in ids):
            raise ValueError(f'{who}: an entry of ids is an int32 tensor or None')
        if style is None:
            style = TrackStyle(K)
        if not isinstance(style, TrackStyle):
            raise ValueError(f'{who}: with ids, style is a TrackStyle')
    if style is None:
        style = PoseStyle(K)
    if not isinstance(style, PoseStyle):
        raise ValueError(f'{who}: style is a PoseStyle')
    for i, (kpts, _, _) in enumerate(poses):
        if kpts.shape[1] != style.K:
            raise ValueError(f'{who}: results[{i}] has K = {kpts.shape[1]}, the style K = {style.K}')
    return surf, poses, style, ids


def _draw(kind, items, tables, style, ids=None, palettes=None):
    kw = dict(thickness=style.thickness, radius=style.radius, score_thr=style.score_thr, kpt_thr=style.kpt_thr,
              draw_boxes=style.draw_boxes)
    if ids is None:
        return ops.draw_poses(kind, items, tables, style.edges, style.K, **kw)
    ops.draw_tracks(kind, [it + (v,) for it, v in zip(items, ids)], tables, palettes, DIGIT_FONT, style.edges, style.K,
                    label_scale=style.label_scale, untracked=style.untracked, **kw)


def draw_poses_nv12(surfaces, width, results, scale_factor=None, style=None, matrix='bt601', full_range=False,
                    ids=None):
    """Draws `results` into NV12 `surfaces` in place and returns `surfaces`.  surfaces: one [H0 * 3 // 2, pitch] uint8
    device tensor or a list of them, of any sizes; `width`, `matrix`, `full_range` and `scale_factor` one value or one
    per surface, as in ``preprocess_surfaces_nv12``.  results, per surface: the (bboxes, labels, kpts) device tuple
    ``push()`` and ``infer_video`` yield, or dict(bboxes=, kpts=, keep=) with fixed shapes.  scale_factor: None for
    results made with rescale=True, else the img_meta's scale_factor (its first two entries divide x and y).  More
    than 32 surfaces go in several launches.  ids: the int32 [N] device tensor ``PoseTracker.update`` returned for
    the surface's result (a list for a list of surfaces, None where a surface has none): poses are coloured and
    labelled by id as `style`, a ``TrackStyle``, says.  An NV12 chroma sample under a digit takes the ink's U, V for
    its whole 2 x 2 block."""
    who = 'draw_poses_nv12'
    surf, poses, style, ids = _gather(surfaces, results, style, who, ids)
    n = len(surf)
    widths = _per_surface(width, n, 'width', (int, np.integer), who)
    modes = list(zip(_per_surface(matrix, n, 'matrix', str, who),
                     (bool(f) for f in _per_surface(full_range, n, 'full_range', (bool, int), who))))
    scales = _scales(scale_factor, n, who)
    combos = sorted(set(modes))
    tables = [style.table_bytes(m, f) for m, f in combos]
    items = [(s, w, kp, bb, keep, sc, combos.index(md))
             for s, w, (kp, bb, keep), sc, md in zip(surf, widths, poses, scales, modes)]
    _draw('nv12', items, tables, style, ids, None if ids is None else [style.palette_bytes(m, f) for m, f in combos])
    return surfaces


def draw_poses_bgr(images, results, scale_factor=None, style=None, ids=None):
    """Draws `results` into [H, W, 3] uint8 BGR device `images` (one tensor or a list, any sizes) in place and returns
    `images`; results, scale_factor, style and ids as in ``draw_poses_nv12``."""
    who = 'draw_poses_bgr'
    surf, poses, style, ids = _gather(images, results, style, who, ids)
    scales = _scales(scale_factor, len(surf), who)
    items = [(s, None, kp, bb, keep, sc, 0) for s, (kp, bb, keep), sc in zip(surf, poses, scales)]
    _draw('bgr', items, [style.table_bytes()], style, ids, None if ids is None else [style.palette_bytes()])
    return images


def show_result(model, img, result, score_thr=0.3, bbox_color=BBOX_COLOR, text_color=BBOX_COLOR, mask_color=None,
                thickness=4, font_size=10, win_name='', show=False, wait_time=0, out_file=None, radius=4, kpt_thr=0.,
                skeleton=None):
    """The detectors' ``show_result`` (videoposev1.py:263-350, petr.py:189): `img` a device or numpy [H, W, 3] uint8
    BGR picture, `result` one image's (bbox_results, kpt_results) as ``simple_test`` returns it (the per-class lists of
    numpy arrays; a one-image list of them is unwrapped), or a device (bboxes, labels, kpts) tuple / dict -> a drawn
    copy on the device, boxes included; `img` is left as it is.  text_color, mask_color, font_size, win_name and
    wait_time are accepted and unused: no text is drawn.  There is no display and no image codec here: show=True or
    out_file= raise NotImplementedError."""
    if show or out_file is not None:
        raise NotImplementedError('show_result: no display or image codec here (show=True / out_file=); take the '
                                  'returned device picture')
    K = model.bbox_head.num_keypoints
    dev = next(model.parameters()).device
    if isinstance(img, np.ndarray):
        img = torch.from_numpy(np.ascontiguousarray(img))
    if not (isinstance(img, torch.Tensor) and img.dim() == 3 and img.shape[2] == 3 and img.dtype == torch.uint8):
        raise ValueError('show_result: img is a [H, W, 3] uint8 BGR picture (tensor or numpy array)')
    if isinstance(result, list) and len(result) == 1 and isinstance(result[0], (tuple, dict)):
        result = result[0]
    if isinstance(result, tuple) and len(result) == 2:    # per-class lists of numpy arrays
        bboxes = np.concatenate([np.asarray(b, np.float32).reshape(-1, 5) for b in result[0]], 0)
        kpts = np.concatenate([np.asarray(k, np.float32).reshape(-1, K, 3) for k in result[1]], 0)
        result = (torch.from_numpy(bboxes).to(img.device if img.is_cuda else dev), None,
                  torch.from_numpy(kpts).to(img.device if img.is_cuda else dev))
    style = PoseStyle(K, thickness=thickness, radius=radius, score_thr=score_thr, kpt_thr=kpt_thr, draw_boxes=True,
                      skeleton=skeleton, bbox_color=bbox_color)
    out = (img if img.is_cuda else img.to(dev)).clone().contiguous()
    return draw_poses_bgr(out, result, style=style)
