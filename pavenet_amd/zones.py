"""Zones and counting lines for the live path (``csrc/pave_zones.hip``): who is inside which
polygon and for how long, who entered or left it, and who crossed which directed line in which direction, per track
id, on the device, by an integer-exact rule.  ``ZoneMonitor.update`` sits after ``PoseTracker.update`` (or after
``PoseSmoother.smooth``, with ``scale_factor=None``): it takes what ``PoseSmoother.smooth`` takes -- a result in
either form and the frame's track ids -- and returns a zone bitmask and dwell times per pose, the frame's events as
a fixed-shape table and keeps running counters, without reading a device value on the host.

Count on the raw result where latency matters and on the smoothed one where flicker matters.  A line's crossings are
not debounced: a track that jitters on a line crosses it forward and backward, and forward - backward is the robust
figure.

``overlay.draw_zones_nv12`` / ``draw_zones_bgr`` draw the zones, the lines and these counters into the picture.

Not built: a hysteresis band for lines, per-id exemptions in ``anonymize``.  (Zones in ground-plane coordinates are
zones drawn on the plan and fed with ``floor.GroundPlane``'s ``out['floor']``)
"""
import math

import torch

from . import native, ops
from .tracked import Tracked

ENTER, EXIT, DWELL, APPEAR, VANISH, CROSS_FWD, CROSS_BACK = (
    native.DEFINES['PAVE_ZONE_' + n] for n in ('ENTER', 'EXIT', 'DWELL', 'APPEAR', 'VANISH', 'CROSS_FWD', 'CROSS_BACK'))
KINDS = {ENTER: 'enter', EXIT: 'exit', DWELL: 'dwell', APPEAR: 'appear', VANISH: 'vanish', CROSS_FWD: 'cross_fwd',
         CROSS_BACK: 'cross_back'}
MAX_ZONES, MAX_LINES, MAX_VERTICES = native.ZONE_MAX_ZONES, native.ZONE_MAX_LINES, native.ZONE_MAX_VERTICES
MAX_COORD = 8191                                      # pixels: 8 * 8191 fits the 16 bits of a 1/8-pixel vertex
MAX_DWELL = 1 << 30
ANKLES = {17: (15, 16), 15: (13, 14), 14: (10, 11)}   # COCO, PoseTrack, CrowdPose
_G = {n: native.DEFINES['PAVE_ZONE_GEOM_' + n] for n in ('NZONES', 'NLINES', 'NVERT', 'DWELL', 'ZONES', 'LINES', 'WORDS')}
_C = {n: native.DEFINES['PAVE_ZONE_CNT_' + n] for n in ('OCCUPANCY', 'ENTERED', 'EXITED', 'APPEARED', 'VANISHED',
                                                        'CROSSED')}
_STATE = ('id', 'last', 'pos', 'inside', 'alerted', 'streak', 'since', 'frame', 'dropped')


def quantise_geometry(zones, lines, dwell_frames=None, who='ZoneMonitor.set_zones'):
    """Polygons [[(x, y), ...], ...] and lines [((ax, ay), (bx, by)), ...] in original-image pixels, dwell_frames one
    integer per zone (None: no DWELL events) -> the PAVE_ZONE_GEOM_WORDS integers of one camera's geometry row: a
    vertex is clamp(rint(8 x), 0, 65535), in double.  Every refusal of `set_zones` is raised here."""
    def vertex(p, what):
        try:
            x, y = (float(v) for v in p)
        except (TypeError, ValueError):
            raise ValueError(f'{who}: {what} is an (x, y) pair, got {p!r}') from None
        if not (math.isfinite(x) and math.isfinite(y) and 0 <= x <= MAX_COORD and 0 <= y <= MAX_COORD):
            raise ValueError(f'{who}: {what} must be finite and in 0 .. {MAX_COORD} pixels, got {(x, y)}')
        return [min(max(int(round(8.0 * v)), 0), 65535) for v in (x, y)]     # (round: half to even, as rint)
    zones, lines = list(zones), list(lines)
    if len(zones) > MAX_ZONES:
        raise ValueError(f'{who}: at most {MAX_ZONES} zones, got {len(zones)}')
    if len(lines) > MAX_LINES:
        raise ValueError(f'{who}: at most {MAX_LINES} lines, got {len(lines)}')
    dwell = [0] * len(zones) if dwell_frames is None else list(dwell_frames)
    if len(dwell) != len(zones):
        raise ValueError(f'{who}: dwell_frames holds one integer per zone ({len(zones)}), got {len(dwell)}')
    if any(isinstance(v, bool) or not isinstance(v, int) or not 0 <= v <= MAX_DWELL for v in dwell):
        raise ValueError(f'{who}: dwell_frames are integers in 0 .. 2^30 (0: no DWELL event), got {dwell!r}')
    row = [0] * _G['WORDS']
    row[_G['NZONES']], row[_G['NLINES']] = len(zones), len(lines)
    for z, polygon in enumerate(zones):
        polygon = list(polygon)
        if not 3 <= len(polygon) <= MAX_VERTICES:
            raise ValueError(f'{who}: zone {z} has {len(polygon)} vertices, a polygon has 3 .. {MAX_VERTICES}')
        row[_G['NVERT'] + z], row[_G['DWELL'] + z] = len(polygon), dwell[z]
        for i, p in enumerate(polygon):
            at = _G['ZONES'] + (z * MAX_VERTICES + i) * 2
            row[at:at + 2] = vertex(p, f'vertex {i} of zone {z}')
    for l, line in enumerate(lines):
        if not (isinstance(line, (tuple, list)) and len(line) == 2):
            raise ValueError(f'{who}: line {l} is ((ax, ay), (bx, by)), got {line!r}')
        a, b = vertex(line[0], f'end A of line {l}'), vertex(line[1], f'end B of line {l}')
        if a == b:
            raise ValueError(f'{who}: the ends of line {l} are one point in 1/8 pixel, {tuple(a)}')
        row[_G['LINES'] + l * 4:_G['LINES'] + l * 4 + 4] = a + b
    return row


class ZoneMonitor(Tracked):
    """Relates the tracks of `cameras` cameras to places: per camera up to 8 polygonal zones and 8 directed counting
    lines (`set_zones`), one slot per track id (`max_tracks`, 1 .. 128; a slot not seen for more than `max_age`
    frames is freed).  A pose takes part iff its box score is > `score_thr` (and keep, and finite coordinates), its id
    is >= 1 and no pose before it in the frame has the same id.

    A pose stands where its `anchor` is: 'feet' is the mean of its visible `anchor_kpts` (score > `kpt_thr`; at most
    4; the ankles of the 17-, 15- and 14-point skeletons are built in) and the bottom centre of its box when none is
    visible, 'box' always that bottom centre, 'centre' the centre of the box.  A track's zone bit flips once the
    inside test has disagreed with it `min_frames` (1 .. 255) frames in a row; a line crossing is not debounced.
    `max_events` (1 .. 4096) rows of events are stored per frame, and all of them are counted."""
    _NOUN, _NOUNS = 'the monitor', "the monitor's"
    _RESET = ('id', 'frame', 'dropped', 'counters')

    def __init__(self, K, cameras=1, max_tracks=128, max_age=30, anchor='feet', anchor_kpts=None, min_frames=2,
                 max_events=256, score_thr=0.3, kpt_thr=0.):
        who = 'ZoneMonitor'
        if isinstance(K, bool) or int(K) != K or not 1 <= K <= native.TRACK_MAX_K:
            raise ValueError(f'{who}: K is an integer in 1 .. {native.TRACK_MAX_K}, got {K!r}')
        for name, v, lo, hi in (('cameras', cameras, 1, native.TRACK_MAX_CAMERAS),
                                ('max_tracks', max_tracks, 1, native.TRACK_MAX_TRACKS),
                                ('min_frames', min_frames, 1, 255),
                                ('max_events', max_events, 1, native.ZONE_MAX_EVENTS)):
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
        self.anchor, self.anchor_kpts = anchor, tuple(anchor_kpts) if anchor == 'feet' else ()
        self.min_frames, self.max_events = min_frames, max_events
        self.score_thr, self.kpt_thr = float(score_thr), float(kpt_thr)
        self._state = None

    def _allocate(self, dev):
        C, S, Z = self.cameras, self.max_tracks, MAX_ZONES
        z = dict(dtype=torch.int32, device=dev)
        self._state = dict(id=torch.zeros((C, S), **z), last=torch.zeros((C, S), **z), pos=torch.zeros((C, S, 2), **z),
                           inside=torch.zeros((C, S), **z), alerted=torch.zeros((C, S), **z),
                           streak=torch.zeros((C, S, Z), **z), since=torch.zeros((C, S, Z), **z),
                           frame=torch.zeros((C,), **z), dropped=torch.zeros((C,), **z),
                           counters=torch.zeros((C, native.ZONE_COUNTER_WORDS), **z),
                           geometry=torch.zeros((C, native.ZONE_GEOM_WORDS), **z))

    def set_zones(self, camera, zones=(), lines=(), dwell_frames=None):
        """The geometry of `camera`, in original-image pixels (0 .. 8191): `zones` polygons of 3 .. 16 (x, y)
        vertices (even-odd, so a polygon may be concave), at most 8; `lines` ((ax, ay), (bx, by)) pairs, at most 8 --
        a track that goes from the left of A -> B to its right (seen along A -> B in the picture, y downwards: from
        the side where cross(B - A, P - A) < 0 to the other) crosses it forward; `dwell_frames` one integer per zone, the frames
        after which a stay is reported once (0 or None: never).  Quantised here to 1/8 pixel and written into that
        camera's row of the geometry tensor -- the one host -> device copy of this class -- and the camera is reset,
        so geometry never changes under live tracks.  Before the first `update` the state is allocated on the
        current HIP device."""
        who = 'ZoneMonitor.set_zones'
        camera = self._camera(camera, who)
        row = quantise_geometry(zones, lines, dwell_frames, who)
        if self._state is None:
            self._allocate(torch.device('cuda', torch.cuda.current_device()))
        self._state['geometry'][camera].copy_(torch.tensor(row, dtype=torch.int32))
        self.reset(camera)

    def update_many(self, items, scale_factor=None):
        """items: (camera, result, ids) triples, the entries of one camera in time order -> one dict per item of new
        int32 device tensors: zones [N] (bit z: the pose's track is inside zone z), dwell [N, 8] (frames inside, 0
        where it is not), events [max_events, 5] (rows (kind, index, id, pose, frame) in the rule's order; zero
        past the count) and n_events (0-d: all events of the frame, stored or not).  result, ids and scale_factor
        are what `PoseSmoother.smooth_many` takes.  One launch per 32 items."""
        items = list(items)
        entries = self._entries(items, scale_factor, 'ZoneMonitor.update')
        if not entries:
            return []
        return ops.zone_events(entries, self._state, K=self.K, max_age=self.max_age, anchor=self.anchor,
                               anchor_kpts=self.anchor_kpts, min_frames=self.min_frames, max_events=self.max_events,
                               score_thr=self.score_thr, kpt_thr=self.kpt_thr)

    def update(self, result, ids, scale_factor=None, camera=0):
        """One frame of `camera` with its track ids -> dict(zones=, dwell=, events=, n_events=)."""
        return self.update_many([(camera, result, ids)], scale_factor)[0]

    def reset(self, camera=None):
        """Frees the slots of `camera` (None: of every camera) without events; its frame count, drop count and
        counters restart at 0 and its geometry stays.  The state tensors stay where they are (a birth writes a
        slot, and a free slot is never read)."""
        self._reset(camera)

    def counts(self, camera=0):
        """Views of one camera's running counters on the device: occupancy, entered, exited, appeared, vanished [8]
        (per zone; occupancy = the live slots inside = entered + appeared - exited - vanished) and crossed [8, 2]
        (per line: forward, backward).  None before the first call."""
        camera = self._camera(camera, 'ZoneMonitor.counts')
        if self._state is None:
            return None
        row = self._state['counters'][camera]
        out = {name.lower(): row[_C[name]:_C[name] + MAX_ZONES] for name in ('OCCUPANCY', 'ENTERED', 'EXITED',
                                                                              'APPEARED', 'VANISHED')}
        out['crossed'] = row[_C['CROSSED']:_C['CROSSED'] + 2 * MAX_LINES].view(MAX_LINES, 2)
        return out

    def state(self, camera=0):
        """Views of one camera's state on the device: id, last, inside, alerted [S] (id 0 = free slot; its other
        fields mean nothing), pos [S, 2] (1/8 pixel), streak, since [S, 8], frame, dropped (0-d).  None before the
        first call."""
        return self._views(camera, 'state', _STATE)

    def device_tensors(self):
        """The whole tensors a reader on the device needs, for every camera at once and read only: geometry
        [cameras, 306], counters [cameras, 56] and id, alerted, inside [cameras, S] (what `overlay.draw_zones_*`
        hands to its kernel).  None before the first call."""
        if self._state is None:
            return None
        return {name: self._state[name] for name in ('geometry', 'counters', 'id', 'alerted', 'inside')}

    def geometry(self, camera=0):
        """Views of one camera's geometry on the device, in 1/8 pixel: n_zones, n_lines (0-d), n_vertices,
        dwell_frames [8], zones [8, 16, 2], lines [8, 2, 2].  None before the first call."""
        camera = self._camera(camera, 'ZoneMonitor.geometry')
        if self._state is None:
            return None
        row = self._state['geometry'][camera]
        return dict(n_zones=row[_G['NZONES']], n_lines=row[_G['NLINES']],
                    n_vertices=row[_G['NVERT']:_G['NVERT'] + MAX_ZONES], dwell_frames=row[_G['DWELL']:_G['DWELL'] + MAX_ZONES],
                    zones=row[_G['ZONES']:_G['LINES']].view(MAX_ZONES, MAX_VERTICES, 2),
                    lines=row[_G['LINES']:_G['WORDS']].view(MAX_LINES, 2, 2))


def events_to_list(out):
    """The events of one `update` as a list of dict(kind=, index=, id=, pose=, frame=) on the host, kind one of
    'enter', 'exit', 'dwell', 'appear', 'vanish', 'cross_fwd', 'cross_back', index the zone or the line, pose the
    row of the result (-1 for 'vanish').  THE host copy of this module: it reads n_events and the table from the
    device, which waits for the stream.  Only the rows that were stored are listed (`out['n_events']` may be
    larger)."""
    n = min(int(out['n_events']), out['events'].shape[0])
    return [dict(kind=KINDS[k], index=i, id=t, pose=p, frame=f) for k, i, t, p, f in out['events'][:n].tolist()]
