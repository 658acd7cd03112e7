"""Track trails for the live path (``csrc/pave_trails.hip``): where each tracked person came from,
kept per camera as a ring of recent points per track on the device by an integer-exact rule, and the paths as tapered
lines in the picture.  ``TrackTrails.update`` sits beside ``ZoneMonitor.update`` and ``FootfallMap.update`` and takes
what they take -- a result in either form and the frame's track ids -- and stands every pose on the same 1/8-pixel
anchor.  A track's anchor is committed to its ring when the newest committed point is at least `stride` frames old and
at least `min_step` eighths of a pixel away, so a standing person does not use the ring up; the line always ends at the
track's latest anchor.  Nothing is read on the host.

``draw_trails_nv12`` / ``draw_trails_bgr`` draw the trails into frames in place, each in its track's colour of
``render.TRACK_PALETTE`` (the colour ``draw_poses_*`` gives the skeleton with ``ids=``), thick at the person and thin
at the old end.  In the loop the trails go over the zones and under the skeletons:

    fmap.update(result, ids); trails.update(result, ids)
    draw_heat_nv12(surface, width, fmap); draw_zones_nv12(...); draw_trails_nv12(surface, width, trails)
    draw_poses_nv12(...)

The outputs per pose -- count, span, dist, path -- give a mean speed (dist / span, 1/8 pixel per frame) and tell a walk
from a wander (path / dist).

Not built: per-key-point trails, anti-aliasing or alpha fades, export formats.  (Trails on the ground plane are these
trails fed with ``floor.GroundPlane``'s ``out['floor']``)
"""
import numpy as np
import torch

from . import native, ops
from .heatmap import MODES, _per_surface   # the (matrix, range) order of an NV12 launch's tables
from .preprocess import NV12_MATRICES
from .render import TRACK_PALETTE, _bgr_triple, bgr_to_yuv
from .tracked import Tracked
from .zones import ANKLES

_STATE = ('id', 'last', 'pos', 'head', 'count', 'box', 'frame', 'dropped')
_POINTS = ('pts', 'when', 'head', 'count')
_DRAWN = ('id', 'last', 'pos', 'head', 'count', 'box', 'pts', 'when', 'frame')


class TrackTrails(Tracked):
    """Trails of `cameras` cameras: per track the last `length` (1 .. 64) committed points.  Who takes part, the slots
    (`max_tracks` 1 .. 128, freed after `max_age` frames unseen), `anchor`, `anchor_kpts`, `score_thr` and `kpt_thr`
    are ``ZoneMonitor``'s.  A track's anchor is committed when the newest committed point is at least `stride` (1 ..
    255) frames old and at least `min_step` (0 .. 65535) eighths of a pixel away in x or in y."""
    _NOUN, _NOUNS = 'the trails', "the trails'"

    def __init__(self, K, cameras=1, max_tracks=128, max_age=30, length=32, stride=1, min_step=16, anchor='feet',
                 anchor_kpts=None, score_thr=0.3, kpt_thr=0.):
        who = 'TrackTrails'
        if isinstance(K, bool) or int(K) != K or not 1 <= K <= native.TRACK_MAX_K:
            raise ValueError(f'{who}: K is an integer in 1 .. {native.TRACK_MAX_K}, got {K!r}')
        for name, v, lo, hi in (('cameras', cameras, 1, native.TRACK_MAX_CAMERAS),
                                ('max_tracks', max_tracks, 1, native.TRACK_MAX_TRACKS),
                                ('length', length, 1, native.TRAIL_MAX_POINTS),
                                ('stride', stride, 1, native.TRAIL_MAX_STRIDE),
                                ('min_step', min_step, 0, native.TRAIL_MAX_STEP)):
            if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
                raise ValueError(f'{who}: {name} is an integer in {lo} .. {hi}, got {v!r}')
        if isinstance(max_age, bool) or int(max_age) != max_age or max_age < 0:
            raise ValueError(f'{who}: max_age is an integer >= 0, got {max_age!r}')
        if anchor not in ops.ZONE_ANCHORS:
            raise ValueError(f"{who}: anchor is 'feet', 'box' or 'centre', got {anchor!r}")
        K = int(K)
        if anchor_kpts is None:
            if anchor == 'feet' and K not in ANKLES:
                raise ValueError(f"{who}: anchor='feet' knows the ankles of K = 17, 15 and 14; K = {K} needs "
                                 f'anchor_kpts=')
            anchor_kpts = ANKLES.get(K, ())
        anchor_kpts = list(anchor_kpts)
        if len(anchor_kpts) > native.ZONE_MAX_ANCHOR_KPTS:
            raise ValueError(f'{who}: at most {native.ZONE_MAX_ANCHOR_KPTS} anchor_kpts, got {len(anchor_kpts)}')
        if any(isinstance(k, bool) or not isinstance(k, int) or not 0 <= k < K for k in anchor_kpts):
            raise ValueError(f'{who}: anchor_kpts are integers in [0, {K}), got {anchor_kpts!r}')
        self.K, self.cameras, self.max_tracks, self.max_age = K, cameras, max_tracks, int(max_age)
        self.length, self.stride, self.min_step = length, stride, min_step
        self.anchor, self.anchor_kpts = anchor, tuple(anchor_kpts) if anchor == 'feet' else ()
        self.score_thr, self.kpt_thr = float(score_thr), float(kpt_thr)
        self._state = None

    def _allocate(self, dev):
        C, S, L = self.cameras, self.max_tracks, self.length
        z = dict(dtype=torch.int32, device=dev)
        self._state = dict(id=torch.zeros((C, S), **z), last=torch.zeros((C, S), **z), pos=torch.zeros((C, S, 2), **z),
                           head=torch.zeros((C, S), **z), count=torch.zeros((C, S), **z), box=torch.zeros((C, S, 4), **z),
                           pts=torch.zeros((C, S, L, 2), **z), when=torch.zeros((C, S, L), **z),
                           frame=torch.zeros((C,), **z), dropped=torch.zeros((C,), **z))

    def update_many(self, items, scale_factor=None):
        """items: (camera, result, ids) triples, the entries of one camera in time order -> one dict per item of new
        int32 [N] device tensors: count (the committed points of the pose's track), span (frames since the oldest of
        them), dist (floor of the straight distance from it to the pose's anchor, 1/8 pixel) and path (the length
        along the committed points to the anchor); all 0 for a pose that takes no part.  result, ids and scale_factor
        are what `ZoneMonitor.update_many` takes.  One launch per 32 items on the current stream; no host copy, no
        sync."""
        items = list(items)
        entries = self._entries(items, scale_factor, 'TrackTrails.update')
        if not entries:
            return []
        return ops.trail_update(entries, self._state, K=self.K, stride=self.stride, min_step=self.min_step,
                                max_age=self.max_age, anchor=self.anchor, anchor_kpts=self.anchor_kpts,
                                score_thr=self.score_thr, kpt_thr=self.kpt_thr)

    def update(self, result, ids, scale_factor=None, camera=0):
        """One frame of `camera` with its track ids -> dict(count=, span=, dist=, path=)."""
        return self.update_many([(camera, result, ids)], scale_factor)[0]

    def reset(self, camera=None):
        """Frees the slots of `camera` (None: of every camera) and restarts its frame and drop counts at 0.  The state
        tensors stay where they are."""
        self._reset(camera)

    def state(self, camera=0):
        """Views of one camera's slots on the device: id, last, head, count [S], pos [S, 2], box [S, 4] (id 0 = free
        slot; its other fields mean nothing), frame, dropped (0-d); 1/8 pixel.  None before the first call."""
        return self._views(camera, 'state', _STATE)

    def points(self, camera=0):
        """Views of one camera's rings on the device: pts [S, L, 2] (1/8 pixel), when [S, L] (the frame a point was
        committed in), head and count [S]: slot t's committed points are, oldest first, pts[t, (head - count + 1 + j) %
        L] for j = 0 .. count - 1.  None before the first call."""
        return self._views(camera, 'points', _POINTS)

    def device_tensors(self):
        """The whole tensors a reader on the device needs, for every camera at once and read only (what
        `draw_trails_*` hands to its kernel).  None before the first call."""
        if self._state is None:
            return None
        return {name: self._state[name] for name in _DRAWN}


class TrailStyle:
    """How trails are drawn.  `palette`: 32 BGR triples, a track takes row (id - 1) % 32 as with ``TrackStyle``.
    `thickness` / `thickness_tail`: the line's width in pixels at the newest / the oldest end (1 .. 32, tail <=
    thickness).  `head_radius`: a disc at the track's latest anchor (0 .. 32 pixels; 0: none).  `tail_frames`: None or
    1 .. 2^30, segments that start at a point committed longer ago are not drawn.  `linger`: None draws every live
    slot, n >= 0 only tracks seen within the last n frames."""

    def __init__(self, palette=TRACK_PALETTE, thickness=3, thickness_tail=1, head_radius=0, tail_frames=None, linger=None):
        who = 'TrailStyle'
        try:
            rows = list(palette)
        except TypeError:
            rows = []
        if len(rows) != native.DRAW_PALETTE:
            raise ValueError(f'{who}: palette is {native.DRAW_PALETTE} colours, got {len(rows)}')
        self.palette = [_bgr_triple(c, f'{who}: a palette colour') for c in rows]
        for name, v, lo, hi in (('thickness', thickness, 1, native.TRAIL_MAX_THICKNESS),
                                ('thickness_tail', thickness_tail, 1, native.TRAIL_MAX_THICKNESS),
                                ('head_radius', head_radius, 0, native.TRAIL_MAX_RADIUS)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
                raise ValueError(f'{who}: {name} is an integer in {lo} .. {hi}, got {v!r}')
        if thickness_tail > thickness:
            raise ValueError(f'{who}: thickness_tail is at most thickness ({thickness}), got {thickness_tail}')
        for name, v, lo in (('tail_frames', tail_frames, 1), ('linger', linger, 0)):
            if v is not None and (isinstance(v, bool) or not isinstance(v, (int, np.integer))
                                  or not lo <= v <= native.TRAIL_MAX_FRAMES):
                raise ValueError(f'{who}: {name} is None or an integer in {lo} .. 2^30, got {v!r}')
        self.thickness, self.thickness_tail, self.head_radius = int(thickness), int(thickness_tail), int(head_radius)
        self.tail_frames = None if tail_frames is None else int(tail_frames)
        self.linger = None if linger is None else int(linger)
        self._tables = {}

    def palette_bytes(self, matrix=None, full_range=False):
        """The 96 bytes of one table of the draw plan: BGR (matrix None) or the (Y, U, V) of a matrix and range."""
        key = (matrix, bool(full_range))
        if key not in self._tables:
            table = np.asarray(self.palette, dtype=np.uint8)
            if matrix is not None:
                table = bgr_to_yuv(table, matrix, full_range)
            self._tables[key] = table.tobytes()
        return self._tables[key]


def _gather(surfaces, trails, camera, style, who):
    surf = [surfaces] if isinstance(surfaces, torch.Tensor) else (
        list(surfaces) if isinstance(surfaces, (list, tuple)) else None)
    if not surf or any(not (isinstance(s, torch.Tensor) and s.dtype == torch.uint8) for s in surf):
        raise ValueError(f'{who}: one uint8 tensor or a non-empty list of them')
    if not isinstance(trails, TrackTrails):
        raise ValueError(f'{who}: trails is a TrackTrails, got {type(trails).__name__}')
    if style is None:
        style = trails.__dict__.setdefault('_default_style', TrailStyle())
    if not isinstance(style, TrailStyle):
        raise ValueError(f'{who}: style is a TrailStyle')
    cams = [trails._camera(c, who) for c in _per_surface(camera, len(surf), 'camera', (int, np.integer), who)]
    return surf, cams, style, trails.device_tensors()


def _where(surf, state, who):
    for i, s in enumerate(surf):
        if not s.is_cuda:
            raise ValueError(f'{who}: surface {i} must be a HIP device tensor (pavenet_amd has no CPU path)')
        if state is not None and s.device != state['id'].device:
            raise ValueError(f"{who}: surface {i} is on {s.device}, the trails on {state['id'].device}")


def _draw(kind, items, state, palettes, style):
    ops.draw_trails(kind, items, state, palettes, thickness=style.thickness, thickness_tail=style.thickness_tail,
                    head_radius=style.head_radius, tail_frames=style.tail_frames, linger=style.linger)


def draw_trails_nv12(surfaces, width, trails, camera=0, style=None, matrix='bt601', full_range=False):
    """Draws the trails of `trails`, a ``TrackTrails``, into NV12 `surfaces` in place and returns `surfaces`.  surfaces,
    width, matrix and full_range: what ``draw_heat_nv12`` takes; camera: whose trails a surface shows, one index or one
    per surface; style: a ``TrailStyle``.  Geometry is in original-image pixels: a surface pixel (x, y) is the picture's
    (x, y).  More than 32 surfaces go in several launches.  Trails that have no state yet draw nothing."""
    from .overlay import _nv12_size
    who = 'draw_trails_nv12'
    surf, cams, style, state = _gather(surfaces, trails, camera, style, who)
    n = len(surf)
    widths = _per_surface(width, n, 'width', (int, np.integer), who)
    modes = list(zip(_per_surface(matrix, n, 'matrix', str, who),
                     (bool(f) for f in _per_surface(full_range, n, 'full_range', (bool, int), who))))
    for md in modes:
        if md not in MODES:
            raise ValueError(f'{who}: unknown matrix {md[0]!r} (one of {sorted(NV12_MATRICES)})')
    for i, (s, w) in enumerate(zip(surf, widths)):
        _nv12_size(s, w, i, who)
    _where(surf, state, who)
    if state is not None:
        _draw('nv12', [(s, int(w), c, MODES.index(md)) for s, w, c, md in zip(surf, widths, cams, modes)], state,
              [style.palette_bytes(m, f) for m, f in MODES], style)
    return surfaces


def draw_trails_bgr(images, trails, camera=0, style=None):
    """Draws the trails of `trails` into [H, W, 3] uint8 BGR device `images` (one tensor or a list, any sizes) in place
    and returns `images`; trails, camera and style as in ``draw_trails_nv12``."""
    who = 'draw_trails_bgr'
    surf, cams, style, state = _gather(images, trails, camera, style, who)
    for i, s in enumerate(surf):
        if s.dim() != 3 or s.shape[2] != 3 or s.shape[0] < 1 or s.shape[1] < 1:
            raise ValueError(f'{who}: surface {i} must be [H, W, 3], got {tuple(s.shape)}')
    _where(surf, state, who)
    if state is not None:
        _draw('bgr', [(s, None, c, 0) for s, c in zip(surf, cams)], state, [style.palette_bytes()], style)
    return images
