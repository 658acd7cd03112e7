"""The ground plane for the live path (``csrc/pave_floor.hip``): where every person stands on the
floor, in millimetres, through a calibrated homography per camera; how fast their track walks and how far it has
walked; how far the nearest other person is; and the poses restated in floor units, so that the anchor-based
consumers -- ``ZoneMonitor``, ``FootfallMap``, ``TrackTrails`` and their draw calls -- work on a plan of the floor
without a change.  ``GroundPlane.update`` sits where ``ZoneMonitor.update`` sits and takes what it takes -- a result in
either form and the frame's track ids -- and stands every pose on the same 1/8-pixel anchor.  The rule is
integer-exact and nothing is read on the host.

    plane = GroundPlane(K, unit=20)                               # a plan pixel is 20 mm
    plane.set_plane(0, points=[((px, py), (X_mm, Y_mm)), ...])    # four marks on the floor or more
    out = plane.update(result, ids, scale_factor)
    fmap.update(out['floor'], ids); trails.update(out['floor'], ids)      # scale_factor=None: floor units
    draw_heat_bgr(plan_picture, fmap); draw_trails_bgr(plan_picture, trails)

``out['floor']`` is for the consumers that stand a pose on its anchor only: every key point and the box of a pose are
that one point.  It is not for ``PostureMonitor``, ``draw_poses_*``, ``anonymize_*`` or ``PoseTracker``.

``nearest``, ``gap`` and ``near`` are one frame's answer.  Who stands with whom over time -- debounced pair contacts,
how long they last and the groups they form -- is ``contacts.ContactMonitor``, which takes the dict
``update`` returns.

Not built: lens distortion (undistort the calibration marks and accept the error, or calibrate close to where people
walk); calibration from vanishing points; identity across cameras; smoothing of the floor position (feed
``PoseSmoother``'s result); a plan-view draw of its own.
"""
import math

import numpy as np
import torch

from . import native, ops
from .tracked import Tracked
from .zones import ANKLES

_STATE = ('id', 'last', 'hits', 'pos', 'vel', 'travel', 'frame', 'dropped')
MAX_MM = native.FLOOR_MAX_MM
ROW_BITS = 61            # every row of the stored matrix: (|g0| + |g1|) 65535 + |g2| < 2^61
MAX_ANCHOR = 65535       # the largest 1/8-pixel anchor coordinate (2 * 32767 rounded up)


def solve_dlt(pairs, who='GroundPlane.set_plane'):
    """[((px, py), (X, Y)), ...], four pairs or more -> the 3 x 3 float64 homography pixels -> floor by the direct
    linear transform: both point sets are moved to their centroids and scaled to a mean distance of sqrt(2), the 2n x 9
    system is solved by ``numpy.linalg.svd``, and the normalisations are taken out again.  ValueError for fewer than 4
    pairs, a value that is not finite, picture or floor points on one line, or pairs that leave the plane open."""
    try:
        src = np.asarray([[float(v) for v in p[0]] for p in pairs], np.float64).reshape(-1, 2)
        dst = np.asarray([[float(v) for v in p[1]] for p in pairs], np.float64).reshape(-1, 2)
    except (TypeError, ValueError, IndexError):
        raise ValueError(f'{who}: points are ((px, py), (X_mm, Y_mm)) pairs') from None
    if len(src) < 4:
        raise ValueError(f'{who}: a plane needs at least 4 point pairs, got {len(src)}')
    if not (np.isfinite(src).all() and np.isfinite(dst).all()):
        raise ValueError(f'{who}: the points must be finite')
    norm = []
    for pts, what in ((src, 'picture'), (dst, 'floor')):
        centre = pts.mean(0)
        sv = np.linalg.svd(pts - centre, compute_uv=False)
        if not sv[1] > 1e-9 * sv[0]:
            raise ValueError(f'{who}: the {what} points lie on one line')
        s = math.sqrt(2.0) / np.sqrt(((pts - centre) ** 2).sum(1)).mean()
        norm.append(np.asarray([[s, 0.0, -s * centre[0]], [0.0, s, -s * centre[1]], [0.0, 0.0, 1.0]]))
    a = (src - src.mean(0)) * norm[0][0, 0]
    b = (dst - dst.mean(0)) * norm[1][0, 0]
    rows = []
    for (x, y), (u, v) in zip(a, b):
        rows.append([-x, -y, -1.0, 0.0, 0.0, 0.0, u * x, u * y, u])
        rows.append([0.0, 0.0, 0.0, -x, -y, -1.0, v * x, v * y, v])
    _, sv, vt = np.linalg.svd(np.asarray(rows, np.float64))
    if not sv[7] > 1e-9 * sv[0]:       # (a second null direction: three of four marks on one line, for one)
        raise ValueError(f'{who}: the points do not fix a plane, the system is singular')
    return np.linalg.inv(norm[1]) @ vt[-1].reshape(3, 3) @ norm[0]


def quantise_plane(H, who='GroundPlane.set_plane'):
    """A 3 x 3 homography pixels -> floor millimetres, its sign already chosen -> the nine integers G: H diag(1/8,
    1/8, 1) times the largest power of two for which every row has (|g0| + |g1|) 65535 + |g2| < 2^61 after rounding to
    nearest (ties to even).  Every step after the float64 matrix is exact.  ValueError for a matrix that is not
    finite or is singular."""
    H = np.asarray(H, np.float64)
    if H.shape != (3, 3) or not np.isfinite(H).all():
        raise ValueError(f'{who}: a plane is a finite 3 x 3 matrix')
    if not np.linalg.cond(H) < 1e12:
        raise ValueError(f'{who}: the matrix is singular')
    g = [float(v) for v in (H * np.asarray([0.125, 0.125, 1.0])).reshape(-1)]      # (exact: powers of two)
    bound = max((abs(g[3 * r]) + abs(g[3 * r + 1])) * MAX_ANCHOR + abs(g[3 * r + 2]) for r in range(3))
    k = ROW_BITS - math.frexp(bound)[1] + 2
    while True:
        words = [round(math.ldexp(v, k)) for v in g]   # (ldexp is exact here; round is half to even)
        if all((abs(words[3 * r]) + abs(words[3 * r + 1])) * MAX_ANCHOR + abs(words[3 * r + 2]) < 1 << ROW_BITS
               for r in range(3)):
            return words
        k -= 1


def calibrate(points=None, matrix=None, bounds=None, who='GroundPlane.set_plane'):
    """What `set_plane` computes on the host -> (H float64 [3, 3], the PAVE_FLOOR_CALIB_WORDS integers of one camera's
    calibration row).  Every refusal of `set_plane` but the camera's is raised here."""
    if (points is None) == (matrix is None):
        raise ValueError(f'{who}: give points= or matrix=, one of them')
    if points is not None:
        pairs = list(points)
        H = solve_dlt(pairs, who)
        w = np.asarray([[float(p[0][0]), float(p[0][1]), 1.0] for p in pairs], np.float64) @ H[2]
        if not ((w > 0).all() or (w < 0).all()):
            raise ValueError(f'{who}: the points lie on both sides of the horizon')
        at = np.asarray([[float(v) for v in p[0]] for p in pairs], np.float64).mean(0)
        if H[2, 0] * at[0] + H[2, 1] * at[1] + H[2, 2] < 0:     # positive at the centroid of the picture points
            H = -H
    else:
        try:
            H = np.asarray(matrix, np.float64)
        except (TypeError, ValueError):
            raise ValueError(f'{who}: a plane is a finite 3 x 3 matrix') from None
        if H.shape != (3, 3) or not np.isfinite(H).all():
            raise ValueError(f'{who}: a plane is a finite 3 x 3 matrix')
        if not H[2, 2] > 0:
            raise ValueError(f'{who}: the third row of the matrix must be positive at the picture point (0, 0)')
    G = quantise_plane(H, who)
    if bounds is None:
        bounds = (-MAX_MM, -MAX_MM, MAX_MM, MAX_MM)
    try:
        x0, y0, x1, y1 = bounds
    except (TypeError, ValueError):
        raise ValueError(f'{who}: bounds is (x0, y0, x1, y1) in mm, got {bounds!r}') from None
    if any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not -MAX_MM <= v <= MAX_MM for v in (x0, y0, x1, y1)) \
            or x0 > x1 or y0 > y1:
        raise ValueError(f'{who}: bounds are integers x0 <= x1, y0 <= y1 in -{MAX_MM} .. {MAX_MM} mm, got {bounds!r}')
    row = [0] * native.FLOOR_CALIB_WORDS
    row[:9] = G
    row[native.FLOOR_CALIB_BOUNDS:native.FLOOR_CALIB_BOUNDS + 4] = [int(x0), int(y0), int(x1), int(y1)]
    row[native.FLOOR_CALIB_VALID] = 1
    return H, row


class GroundPlane(Tracked):
    """The floor under `cameras` cameras.  Who takes part, the slots (`max_tracks` 1 .. 128, freed after `max_age`
    frames unseen), `anchor`, `anchor_kpts`, `score_thr` and `kpt_thr` are ``ZoneMonitor``'s, with one condition more:
    the pose's anchor projects onto the floor inside the camera's bounds.  `velocity_gain` (1 .. 16): sixteenths of a
    track's newest move that go into its velocity.  `near` (0 .. 2^20 mm): the radius within which neighbours are
    counted.  `unit` (1 .. 1000 mm) and `origin` ((x, y) in mm): a pixel of the plan that ``out['floor']`` is drawn on
    and the floor point of its corner."""
    _NOUN, _NOUNS = 'the plane', "the plane's"

    def __init__(self, K, cameras=1, max_tracks=128, max_age=30, anchor='feet', anchor_kpts=None, velocity_gain=4,
                 near=1500, unit=10, origin=(0, 0), score_thr=0.3, kpt_thr=0.):
        who = 'GroundPlane'
        if isinstance(K, bool) or int(K) != K or not 1 <= K <= native.TRACK_MAX_K:
            raise ValueError(f'{who}: K is an integer in 1 .. {native.TRACK_MAX_K}, got {K!r}')
        for name, v, lo, hi in (('cameras', cameras, 1, native.TRACK_MAX_CAMERAS),
                                ('max_tracks', max_tracks, 1, native.TRACK_MAX_TRACKS),
                                ('velocity_gain', velocity_gain, 1, native.FLOOR_MAX_GAIN),
                                ('near', near, 0, native.FLOOR_MAX_NEAR),
                                ('unit', unit, 1, native.FLOOR_MAX_UNIT)):
            if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
                raise ValueError(f'{who}: {name} is an integer in {lo} .. {hi}, got {v!r}')
        if not (isinstance(origin, (tuple, list)) and len(origin) == 2) or any(
                isinstance(v, bool) or not isinstance(v, int) or not -MAX_MM <= v <= MAX_MM for v in origin):
            raise ValueError(f'{who}: origin is two integers in -{MAX_MM} .. {MAX_MM} mm, got {origin!r}')
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
        self.velocity_gain, self.near, self.unit, self.origin = velocity_gain, near, unit, tuple(origin)
        self.anchor, self.anchor_kpts = anchor, tuple(anchor_kpts) if anchor == 'feet' else ()
        self.score_thr, self.kpt_thr = float(score_thr), float(kpt_thr)
        self.H = [None] * cameras          # the float64 homographies, pixels -> mm, on the host
        self._state = None
        self._calib = None

    def _allocate(self, dev):
        C, S = self.cameras, self.max_tracks
        z = dict(dtype=torch.int32, device=dev)
        self._state = dict(id=torch.zeros((C, S), **z), last=torch.zeros((C, S), **z), hits=torch.zeros((C, S), **z),
                           pos=torch.zeros((C, S, 2), **z), vel=torch.zeros((C, S, 2), **z),
                           travel=torch.zeros((C, S), **z), frame=torch.zeros((C,), **z),
                           dropped=torch.zeros((C,), **z))
        self._calib = torch.zeros((C, native.FLOOR_CALIB_WORDS), dtype=torch.int64, device=dev)

    def set_plane(self, camera, points=None, matrix=None, bounds=None):
        """The floor of `camera`: `points`, at least four ((px, py), (X_mm, Y_mm)) pairs of original-image pixels and
        floor millimetres, all on one side of the horizon and, if there are only four, no three on a line (solved by
        the direct linear transform in float64), or `matrix`, the 3 x 3 homography pixels -> mm whose third row is positive at the
        picture's (0, 0).  `bounds` (x0, y0, x1, y1), integers in mm within +-(2^20 - 1): a pose that projects outside
        is not on the floor (None: the whole range).  Quantised here to nine int64 words and written into that
        camera's row of the calibration tensor -- the one host -> device copy of this class -- and the camera is
        reset, so a plane never changes under live tracks.  The float64 matrix stays on the host as ``H[camera]``.
        Before the first `update` the state is allocated on the current HIP device."""
        who = 'GroundPlane.set_plane'
        camera = self._camera(camera, who)
        H, row = calibrate(points, matrix, bounds, who)
        if self._state is None:
            self._allocate(torch.device('cuda', torch.cuda.current_device()))
        self._calib[camera].copy_(torch.tensor(row, dtype=torch.int64))
        self.H[camera] = H
        self.reset(camera)

    def update_many(self, items, scale_factor=None):
        """items: (camera, result, ids) triples, the entries of one camera in time order -> one dict per item of new
        device tensors, int32 but for `floor`: on [N] (1: the pose is placed on the floor), xy [N, 2] (mm), vel [N, 2]
        and speed [N] (its track's, 1/256 mm per frame), travel [N] (its track's, mm), nearest [N] (the row of the
        nearest other placed pose, or -1), gap [N] (mm to it, or -1), near [N] (the others within `near` mm), and floor,
        the result in floor units in the form that went in (the tuple with the same labels tensor, the dict with the
        same keep tensor; give it to a consumer with scale_factor=None).  result, ids and scale_factor are what
        `ZoneMonitor.update_many` takes.  A camera without a plane places nobody.  One launch per 32 items on the
        current stream; no host copy, no sync."""
        items = list(items)
        entries = self._entries(items, scale_factor, 'GroundPlane.update')
        if not entries:
            return []
        outs = ops.floor_update(entries, self._state, self._calib, K=self.K, velocity_gain=self.velocity_gain,
                                near=self.near, unit=self.unit, origin=self.origin, max_age=self.max_age,
                                anchor=self.anchor, anchor_kpts=self.anchor_kpts, score_thr=self.score_thr,
                                kpt_thr=self.kpt_thr)
        for out, (_, result, _) in zip(outs, items):
            kpts, bboxes = out.pop('kpts'), out.pop('bboxes')
            if isinstance(result, dict):
                floor = dict(result)
                floor['bboxes'], floor['kpts'] = bboxes.view(result['bboxes'].shape), kpts.view(result['kpts'].shape)
            else:
                floor = (bboxes.view(result[0].shape), result[1], kpts.view(result[2].shape))
            out['floor'] = floor
        return outs

    def update(self, result, ids, scale_factor=None, camera=0):
        """One frame of `camera` with its track ids -> dict(on=, xy=, vel=, speed=, travel=, nearest=, gap=, near=,
        floor=)."""
        return self.update_many([(camera, result, ids)], scale_factor)[0]

    def reset(self, camera=None):
        """Frees the slots of `camera` (None: of every camera) and restarts its frame and drop counts at 0; its plane
        stays.  The state tensors stay where they are."""
        self._reset(camera)

    def state(self, camera=0):
        """Views of one camera's slots on the device: id, last, hits, travel [S] (id 0 = free slot; its other fields
        mean nothing), pos [S, 2] (mm), vel [S, 2] (1/256 mm per frame), frame, dropped (0-d).  None before the first
        call."""
        return self._views(camera, 'state', _STATE)

    def calibration(self, camera=0):
        """Views of one camera's calibration on the device, int64: G [3, 3] (1/8 pixel -> floor, times a power of
        two), bounds [4] (mm) and valid (0-d; 0: no plane was set).  None before the first call."""
        camera = self._camera(camera, 'GroundPlane.calibration')
        if self._calib is None:
            return None
        row, b = self._calib[camera], native.FLOOR_CALIB_BOUNDS
        return dict(G=row[:9].view(3, 3), bounds=row[b:b + 4], valid=row[native.FLOOR_CALIB_VALID])
