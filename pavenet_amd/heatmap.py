"""Footfall heat maps for the live path (``csrc/pave_heat.hip``): where tracked people stood and
walked, accumulated per camera on a grid of cells on the device by an integer-exact rule, and the map as a colour
overlay in the picture.  ``FootfallMap.update`` sits beside ``ZoneMonitor.update`` and takes what it takes -- a result
in either form and the frame's track ids -- and stands every pose on the same 1/8-pixel anchor.  It keeps two maps:
``dwell`` (every frame a pose stands on a cell adds a small tent of weights about it: person-frames) and ``visits``
(a track adds 1 when it comes into a cell: a count of entries).  Nothing is read on the host.

``draw_heat_nv12`` / ``draw_heat_bgr`` blend a map into frames in place through a 256-colour ramp, reading the map and
its peak where they live.  In the loop the map goes under the zones and the skeletons:

    fmap.update(result, ids); draw_heat_nv12(surface, width, fmap); draw_zones_nv12(...); draw_poses_nv12(...)

A cell of ``dwell`` gains at most 128 (radius + 1)^2 per frame: with ``half_life=0`` (never forget) the first frame at
which it could pass 2^31 is 2^31 / (128 (radius + 1)^2) -- 1 048 576 frames at radius 3 (under ten hours at 30 frames
per second with 128 people on one cell), 4 194 304 at radius 1 -- and ``reset`` is the remedy; with a half life of at
most 2^18 frames no cell can get there.

Not built: per-hour maps or export formats, Gaussian footprints, anti-aliased colour ramps with text legends.  (The path
of one track is ``trails.TrackTrails``.  A map on the ground plane is this map fed with ``floor.GroundPlane``'s
``out['floor']``)
"""
import numpy as np
import torch

from . import native, ops
from .preprocess import NV12_MATRICES
from .render import _bgr_triple, bgr_to_yuv
from .tracked import Tracked
from .zones import ANKLES

_STATE = ('id', 'last', 'cell', 'frame', 'dropped')
MODES = [(m, f) for m in sorted(NV12_MATRICES) for f in (False, True)]   # palette tables 1 ..: (matrix, full_range)


def _ramp():
    """Black-blue-cyan-green-yellow-red, 256 BGR rows by level: five linear pieces between six stops."""
    stops = ((48, 0, 0), (255, 64, 0), (255, 255, 0), (0, 255, 64), (0, 255, 255), (0, 0, 255))
    rows = []
    for level in range(256):
        seg, t = divmod(level * 5, 255)
        if seg >= 5:
            seg, t = 4, 255
        a, b = stops[seg], stops[seg + 1]
        rows.append(tuple((a[c] * (255 - t) + b[c] * t + 127) // 255 for c in range(3)))
    return tuple(rows)


HEAT_PALETTE = _ramp()


class FootfallMap(Tracked):
    """Footfall maps of `cameras` cameras over pictures of `size` = (width, height) original-image pixels (1 .. 8192
    each), one cell per `cell` x `cell` pixels (4, 8, 16, 32 or 64; at most 512 cells a side).  Who takes part, the
    slots (`max_tracks` 1 .. 128, freed after `max_age` frames unseen), `anchor`, `anchor_kpts`, `score_thr` and
    `kpt_thr` are ``ZoneMonitor``'s.  A pose adds (radius + 1 - |dx|)(radius + 1 - |dy|) to `dwell` at the cells within
    `radius` (0 .. 3) of its own, and 1 to `visits` at its own cell when its track comes into it.  Every `half_life`
    frames (0 .. 2^18; 0: never) both maps are halved."""
    _NOUN, _NOUNS = 'the map', "the map's"
    _RESET = ('id', 'frame', 'dropped', 'peak', 'dwell', 'visits')

    def __init__(self, K, size, cell=8, cameras=1, max_tracks=128, max_age=30, anchor='feet', anchor_kpts=None, radius=1,
                 half_life=0, score_thr=0.3, kpt_thr=0.):
        who = 'FootfallMap'
        if isinstance(K, bool) or int(K) != K or not 1 <= K <= native.TRACK_MAX_K:
            raise ValueError(f'{who}: K is an integer in 1 .. {native.TRACK_MAX_K}, got {K!r}')
        self.Gw, self.Gh = ops.heat_grid(who, size, cell)
        for name, v, lo, hi in (('cameras', cameras, 1, native.TRACK_MAX_CAMERAS),
                                ('max_tracks', max_tracks, 1, native.TRACK_MAX_TRACKS),
                                ('radius', radius, 0, native.HEAT_MAX_RADIUS),
                                ('half_life', half_life, 0, native.HEAT_MAX_HALF_LIFE)):
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
        self.K, self.size, self.cell, self.cameras = K, (int(size[0]), int(size[1])), cell, cameras
        self.max_tracks, self.max_age, self.radius, self.half_life = max_tracks, int(max_age), radius, half_life
        self.anchor, self.anchor_kpts = anchor, tuple(anchor_kpts) if anchor == 'feet' else ()
        self.score_thr, self.kpt_thr = float(score_thr), float(kpt_thr)
        self._state = None

    def _allocate(self, dev):
        C, S = self.cameras, self.max_tracks
        z = dict(dtype=torch.int32, device=dev)
        self._state = dict(id=torch.zeros((C, S), **z), last=torch.zeros((C, S), **z), cell=torch.zeros((C, S), **z),
                           frame=torch.zeros((C,), **z), dropped=torch.zeros((C,), **z), peak=torch.zeros((C, 2), **z),
                           dwell=torch.zeros((C, self.Gh, self.Gw), **z), visits=torch.zeros((C, self.Gh, self.Gw), **z))

    def update_many(self, items, scale_factor=None):
        """items: (camera, result, ids) triples, the entries of one camera in time order -> one dict per item of new
        int32 [N] device tensors: cell (the pose's cell gy Gw + gx; -1: it takes no part or stands off the map), dwell
        and visits (the two maps at that cell after the frame, else 0).  result, ids and scale_factor are what
        `ZoneMonitor.update_many` takes.  One launch per 32 items on the current stream; no host copy, no sync."""
        items = list(items)
        entries = self._entries(items, scale_factor, 'FootfallMap.update')
        if not entries:
            return []
        return ops.heat_update(entries, self._state, K=self.K, size=self.size, cell=self.cell, radius=self.radius,
                               half_life=self.half_life, max_age=self.max_age, anchor=self.anchor,
                               anchor_kpts=self.anchor_kpts, score_thr=self.score_thr, kpt_thr=self.kpt_thr)

    def update(self, result, ids, scale_factor=None, camera=0):
        """One frame of `camera` with its track ids -> dict(cell=, dwell=, visits=)."""
        return self.update_many([(camera, result, ids)], scale_factor)[0]

    def reset(self, camera=None):
        """Clears the maps and the peak of `camera` (None: of every camera), frees its slots and restarts its frame
        and drop counts at 0.  The state tensors stay where they are."""
        self._reset(camera)

    def maps(self, camera=0):
        """Views of one camera's maps on the device: dwell, visits [Gh, Gw] and peak [2] (their maxima), int32.  None
        before the first call."""
        return self._views(camera, 'maps', ('dwell', 'visits', 'peak'))

    def state(self, camera=0):
        """Views of one camera's slots on the device: id, last, cell [S] (id 0 = free slot; its other fields mean
        nothing; cell -1 = off the map), frame, dropped (0-d).  None before the first call."""
        return self._views(camera, 'state', _STATE)

    def device_tensors(self):
        """The whole tensors a reader on the device needs, for every camera at once and read only: dwell, visits
        [cameras, Gh, Gw] and peak [cameras, 2] (what `draw_heat_*` hands to its kernel).  None before the first
        call."""
        if self._state is None:
            return None
        return {name: self._state[name] for name in ('dwell', 'visits', 'peak')}


class HeatStyle:
    """How a map is drawn.  `source`: 'dwell' | 'visits'.  A cell's level is min(255, 255 v / scale), scale =
    `full_scale` (an integer 1 .. 2^31 - 1) or, None, the map's own peak as it is on the device at that moment.
    `palette`: 256 BGR triples by level (None: ``HEAT_PALETTE``).  A pixel is blended with (`alpha_max` level + 128) >>
    8 of 256 parts of its colour (`alpha_max` 0 .. 256) and left alone below level `floor` (0 .. 255).  `smooth`: levels
    are interpolated between cell centres; else every pixel takes its cell's."""

    def __init__(self, source='dwell', palette=None, full_scale=None, alpha_max=160, floor=1, smooth=True):
        who = 'HeatStyle'
        if source not in ops.HEAT_SOURCES:
            raise ValueError(f"{who}: source is 'dwell' or 'visits', got {source!r}")
        try:
            rows = list(HEAT_PALETTE if palette is None else palette)
        except TypeError:
            rows = []
        if len(rows) != 256:
            raise ValueError(f'{who}: palette is 256 BGR triples, got {len(rows)}')
        self.palette = [_bgr_triple(c, f'{who}: a palette colour') for c in rows]
        if full_scale is not None and (isinstance(full_scale, bool) or not isinstance(full_scale, (int, np.integer))
                                       or not 1 <= full_scale <= 2 ** 31 - 1):
            raise ValueError(f'{who}: full_scale is None or an integer in 1 .. 2^31 - 1, got {full_scale!r}')
        for name, v, lo, hi in (('alpha_max', alpha_max, 0, 256), ('floor', floor, 0, 255)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
                raise ValueError(f'{who}: {name} is an integer in {lo} .. {hi}, got {v!r}')
        self.source, self.full_scale = source, None if full_scale is None else int(full_scale)
        self.alpha_max, self.floor, self.smooth = int(alpha_max), int(floor), bool(smooth)
        self._device = {}

    def tables(self):
        """The [5, 256, 3] bytes the kernels read: table 0 the palette in BGR, tables 1 .. 4 its (Y, U, V) for
        ``MODES`` = (bt601, limited), (bt601, full), (bt709, limited), (bt709, full)."""
        bgr = np.asarray(self.palette, dtype=np.uint8)
        return np.stack([bgr] + [bgr_to_yuv(bgr, m, f) for m, f in MODES])

    def device_tables(self, device):
        """`tables()` on `device`: THE host-to-device copy of this module, made once per style and device (as
        ``ZoneMonitor.set_zones`` is for section 17), on the current stream."""
        key = (device.type, device.index)
        if key not in self._device:
            self._device[key] = torch.from_numpy(self.tables()).to(device)
        return self._device[key]


def _per_surface(v, n, name, scalar, who):
    """One value or one per surface -> a list of n (``render._per_surface``, with a ValueError for what is neither)."""
    if isinstance(v, scalar) or not isinstance(v, (list, tuple)):
        return [v] * n
    if len(v) != n:
        raise ValueError(f'{who}: {name} is one value or one per surface ({n}), got {len(v)}')
    return list(v)


def _gather(surfaces, fmap, camera, style, who):
    surf = [surfaces] if isinstance(surfaces, torch.Tensor) else (
        list(surfaces) if isinstance(surfaces, (list, tuple)) else None)
    if not surf or any(not (isinstance(s, torch.Tensor) and s.dtype == torch.uint8) for s in surf):
        raise ValueError(f'{who}: one uint8 tensor or a non-empty list of them')
    if not isinstance(fmap, FootfallMap):
        raise ValueError(f'{who}: fmap is a FootfallMap, got {type(fmap).__name__}')
    if style is None:
        style = fmap.__dict__.setdefault('_default_style', HeatStyle())
    if not isinstance(style, HeatStyle):
        raise ValueError(f'{who}: style is a HeatStyle')
    cams = [fmap._camera(c, who) for c in _per_surface(camera, len(surf), 'camera', (int, np.integer), who)]
    return surf, cams, style, fmap.device_tensors()


def _where(surf, state, who):
    for i, s in enumerate(surf):
        if not s.is_cuda:
            raise ValueError(f'{who}: surface {i} must be a HIP device tensor (pavenet_amd has no CPU path)')
        if state is not None and s.device != state['peak'].device:
            raise ValueError(f"{who}: surface {i} is on {s.device}, the map on {state['peak'].device}")


def _draw(kind, items, state, fmap, style):
    ops.draw_heat(kind, items, state, style.device_tables(state['peak'].device), size=fmap.size, cell=fmap.cell,
                  source=style.source, full_scale=style.full_scale, alpha_max=style.alpha_max, floor=style.floor,
                  smooth=style.smooth)


def draw_heat_nv12(surfaces, width, fmap, camera=0, style=None, matrix='bt601', full_range=False):
    """Blends a map of `fmap`, a ``FootfallMap``, into NV12 `surfaces` in place and returns `surfaces`.  surfaces,
    width, matrix and full_range: what ``draw_zones_nv12`` takes; camera: whose map a surface shows, one index or one
    per surface; style: a ``HeatStyle``.  A surface pixel (x, y) shows the map at (x, y); pixels beyond the map's size
    are left alone.  More than 32 surfaces go in several launches.  A map that has no state yet draws nothing."""
    from .overlay import _nv12_size
    who = 'draw_heat_nv12'
    surf, cams, style, state = _gather(surfaces, fmap, camera, style, who)
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
        _draw('nv12', [(s, int(w), c, 1 + MODES.index(md)) for s, w, c, md in zip(surf, widths, cams, modes)], state,
              fmap, style)
    return surfaces


def draw_heat_bgr(images, fmap, camera=0, style=None):
    """Blends a map of `fmap` into [H, W, 3] uint8 BGR device `images` (one tensor or a list, any sizes) in place and
    returns `images`; fmap, camera and style as in ``draw_heat_nv12``."""
    who = 'draw_heat_bgr'
    surf, cams, style, state = _gather(images, fmap, camera, style, who)
    for i, s in enumerate(surf):
        if s.dim() != 3 or s.shape[2] != 3 or s.shape[0] < 1 or s.shape[1] < 1:
            raise ValueError(f'{who}: surface {i} must be [H, W, 3], got {tuple(s.shape)}')
    _where(surf, state, who)
    if state is not None:
        _draw('bgr', [(s, None, c, 0) for s, c in zip(surf, cams)], state, fmap, style)
    return images
