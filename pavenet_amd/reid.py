"""The same person again (``csrc/pave_reid.hip``): person ids that survive a gap.  A track id ends
when a person is hidden for longer than the tracker's ``max_age``; ``PersonReID`` sits after ``PoseTracker.update``,
reads a colour descriptor of every pose's torso and legs from the pixels of the frame, keeps a gallery of the people
it has seen per camera, and maps track ids to person ids: a new track whose colours match a person who left takes
that person's id back.  ``out['ids']`` goes wherever the track ids went -- ``PoseSmoother.smooth``,
``ZoneMonitor.update``, ``draw_poses_*(ids=)``, ``formats.posetrack_frame`` -- and nothing is read from the device on
the host.

Colour only: two people dressed alike swap or merge, a lighting change beyond the measured shift breaks a match, and
the decision is made in a track's first frame, so a person who comes back half hidden is not re-identified.

Not built: a learned embedding, identity across cameras, a second chance for a track that was born occluded,
descriptors that follow the limbs instead of two rectangles.
"""
import numpy as np
import torch

from . import native, ops
from .render import _per_surface, _poses, _scales, _surfaces_and_poses

TORSO = {17: ((5, 6), (11, 12)), 15: ((3, 4), (9, 10)), 14: ((0, 1), (6, 7))}       # (shoulders, hips)
LEGS = {17: ((11, 12), (13, 14)), 15: ((9, 10), (11, 12)), 14: ((6, 7), (8, 9))}    # (hips, knees)
NEVER = native.REID_NEVER
# The midpoint of the lowest same-person score and the highest different-person score that tests/test_reid_cpu.py
# measures on its synthetic scenes.
DEFAULT_MATCH_THR = 28138
_STATE = ('person', 'track', 'last', 'hits', 'hist', 'frame', 'next', 'dropped')


def _parts(value, K, name, who):
    try:
        upper, lower = value
        value = (tuple(upper), tuple(lower))
    except (TypeError, ValueError):
        raise ValueError(f'{who}: {name} is an (upper, lower) pair of key-point index lists, got {value!r}') from None
    for half in value:
        if not 1 <= len(half) <= native.REID_MAX_PART:
            raise ValueError(f'{who}: a part of {name} holds 1 .. {native.REID_MAX_PART} key points, got {len(half)}')
        if any(isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 0 <= k < K for k in half):
            raise ValueError(f'{who}: the key points of {name} are integers in [0, {K}), got {half!r}')
    return tuple(tuple(int(k) for k in half) for half in value)


class PersonReID:
    """Maps the track ids of `cameras` cameras to person ids.  Per camera `max_people` (1 .. 128) slots hold a person
    id, the track id it is bound to, and a smoothed colour descriptor of the torso and of the legs (`gain` 1 .. 16
    sixteenths: the weight of the newest sighting).  A slot not seen for more than `max_lost` frames is freed.  A
    pose takes part iff its box score is > `score_thr` (and keep, and finite coordinates), its id is >= 1 and no pose
    before it in the frame has the same id.  A pose whose track id is bound to a slot keeps that slot's person id; a
    new track id is compared with the slots whose tracks are not in the frame and whose torso has been seen
    `min_hits` times, and takes the best one scoring >= `match_thr` (0 .. 65536; 65537: never; None: the measured
    default); otherwise it becomes a new person.  Person ids start at 1 per camera and are never used twice.

    `torso` and `legs` are ((upper key points), (lower key points)) -- shoulders and hips, hips and knees; those of
    the 17-, 15- and 14-point skeletons are built in.  A key point is visible with a score > `kpt_thr`."""

    def __init__(self, K, cameras=1, max_people=128, max_lost=900, match_thr=None, min_hits=3, gain=2, torso=None,
                 legs=None, score_thr=0.3, kpt_thr=0.):
        who = 'PersonReID'
        if isinstance(K, bool) or int(K) != K or not 1 <= K <= native.TRACK_MAX_K:
            raise ValueError(f'{who}: K is an integer in 1 .. {native.TRACK_MAX_K}, got {K!r}')
        K = int(K)
        if match_thr is None:
            match_thr = DEFAULT_MATCH_THR
        for name, v, lo, hi in (('cameras', cameras, 1, native.TRACK_MAX_CAMERAS),
                                ('max_people', max_people, 1, native.TRACK_MAX_TRACKS),
                                ('match_thr', match_thr, 0, NEVER), ('min_hits', min_hits, 1, native.REID_MAX_HITS),
                                ('gain', gain, 1, 16)):
            if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
                raise ValueError(f'{who}: {name} is an integer in {lo} .. {hi}, got {v!r}')
        if isinstance(max_lost, bool) or int(max_lost) != max_lost or max_lost < 0:
            raise ValueError(f'{who}: max_lost is an integer >= 0, got {max_lost!r}')
        if (torso is None or legs is None) and K not in TORSO:
            raise ValueError(f'{who}: the shoulders, hips and knees of K = 17, 15 and 14 are built in; K = {K} needs '
                             'torso= and legs=')
        self.torso = TORSO[K] if torso is None else _parts(torso, K, 'torso', who)
        self.legs = LEGS[K] if legs is None else _parts(legs, K, 'legs', who)
        self.K, self.cameras, self.max_people, self.max_lost = K, cameras, max_people, int(max_lost)
        self.match_thr, self.min_hits, self.gain = match_thr, min_hits, gain
        self.score_thr, self.kpt_thr = float(score_thr), float(kpt_thr)
        self.kind = None          # 'nv12' or 'bgr' once the gallery has seen a picture
        self._state = self._scratch = None

    def _allocate(self, dev):
        C, S = self.cameras, self.max_people
        z = dict(dtype=torch.int32, device=dev)
        self._state = dict(person=torch.zeros((C, S), **z), track=torch.zeros((C, S), **z), last=torch.zeros((C, S), **z),
                           hits=torch.zeros((C, S, 2), **z), hist=torch.zeros((C, S, 2, native.REID_BINS), **z),
                           frame=torch.zeros((C,), **z), next=torch.ones((C,), **z), dropped=torch.zeros((C,), **z))
        self._scratch = ops.reid_scratch(dev)

    def _camera(self, camera, who):
        if isinstance(camera, bool) or int(camera) != camera or not 0 <= camera < self.cameras:
            raise ValueError(f'{who}: camera must be an integer in [0, {self.cameras}), got {camera!r}')
        return int(camera)

    def _entries(self, surfaces, widths, results, scale_factor, who):
        """-> [(surface, width, kpts, bboxes, keep, (sx, sy))], the checks of anonymize_nv12 / _bgr."""
        n = len(surfaces)
        poses = [_poses(r, i, who) for i, r in enumerate(results)]
        scales = _scales(scale_factor, n, who)
        if any(not (0 < sx < float('inf') and 0 < sy < float('inf')) for sx, sy in scales):
            raise ValueError(f'{who}: a scale factor must be positive and finite')
        for i, ((kpts, _, _), s) in enumerate(zip(poses, surfaces)):
            if kpts.shape[1] != self.K:
                raise ValueError(f'{who}: results[{i}] has K = {kpts.shape[1]}, the gallery K = {self.K}')
            if kpts.shape[0] > native.TRACK_MAX_POSES:
                raise ValueError(f'{who}: results[{i}] has {kpts.shape[0]} poses, at most {native.TRACK_MAX_POSES}')
            if not isinstance(s, torch.Tensor):
                raise ValueError(f'{who}: surface {i} must be a uint8 tensor')
            if not s.is_contiguous():
                raise ValueError(f'{who}: surface {i} must be contiguous')
        return [(s, w, kp, bb, keep, sc) for s, w, (kp, bb, keep), sc in zip(surfaces, widths, poses, scales)]

    @staticmethod
    def _on_device(i, entry, who):
        if not all(t is None or t.is_cuda for t in (entry[0], entry[2], entry[3], entry[4])):
            raise ValueError(f'{who}: surface {i} and results[{i}] must be HIP device tensors (pavenet_amd has no CPU '
                             'path)')

    def _update(self, kind, items, scale_factor, who):
        who = f'PersonReID.{who}_{kind}'
        items = list(items)
        want = 5 if kind == 'nv12' else 4
        if any(not (isinstance(it, (tuple, list)) and len(it) == want) for it in items):
            raise ValueError(f'{who}: items are (camera, surface, width, result, ids) tuples' if kind == 'nv12' else
                             f'{who}: items are (camera, image, result, ids) tuples')
        if not items:
            return []
        if self.kind not in (None, kind):
            raise ValueError(f'{who}: this gallery holds {self.kind} descriptors; a gallery is of one kind')
        cams = [self._camera(it[0], who) for it in items]
        widths = [it[2] if kind == 'nv12' else None for it in items]
        if kind == 'nv12' and any(isinstance(w, bool) or not isinstance(w, (int, np.integer)) for w in widths):
            raise ValueError(f'{who}: width is an integer')
        entries = self._entries([it[1] for it in items], widths, [it[-2] for it in items], scale_factor, who)
        full = []
        for i, (entry, it, cam) in enumerate(zip(entries, items, cams)):
            ids, N = it[-1], entry[2].shape[0]
            if not (isinstance(ids, torch.Tensor) and ids.dtype == torch.int32 and tuple(ids.shape) == (N,)):
                raise ValueError(f'{who}: ids of results[{i}] must be an int32 [{N}] tensor')
            self._on_device(i, entry, who)
            if not ids.is_cuda:
                raise ValueError(f'{who}: ids of results[{i}] must be a HIP device tensor (pavenet_amd has no CPU path)')
            if not ids.is_contiguous():
                raise ValueError(f'{who}: ids of results[{i}] must be contiguous')
            full.append(entry + (ids, cam))
        dev = full[0][0].device
        if self._state is not None and self._state['person'].device != dev:
            raise ValueError(f"{who}: the gallery's state is on {self._state['person'].device}, surface 0 on {dev}")
        # everything the host can see is checked by a dry pass before the first call allocates
        if self._state is None:
            ops._reid_items(who, kind, full, self.K, (self.torso, self.legs))
            self._allocate(dev)
        outs = ops.reid_update(kind, full, self._state, self._scratch, self.K, (self.torso, self.legs),
                               max_lost=self.max_lost, match_thr=self.match_thr, min_hits=self.min_hits, gain=self.gain,
                               score_thr=self.score_thr, kpt_thr=self.kpt_thr)
        self.kind = kind
        return outs

    def update_many_nv12(self, items, scale_factor=None):
        """items: (camera, surface, width, result, ids) tuples, the entries of one camera in time order -> one
        dict(ids=, sim=) of new int32 [N] device tensors per item: the person id of every pose (0: it takes no part,
        or the gallery is full of people in the picture) and the score at which it was re-identified in this frame
        (else 0).  surface, width, result and scale_factor are what ``anonymize_nv12`` takes, ids what
        ``PoseTracker.update`` returned for the result.  The surfaces are only read.  Two launches per 32 items."""
        return self._update('nv12', items, scale_factor, 'update_many')

    def update_nv12(self, surface, width, result, ids, scale_factor=None, camera=0):
        """One frame of `camera` -> dict(ids=, sim=)."""
        return self._update('nv12', [(camera, surface, width, result, ids)], scale_factor, 'update')[0]

    def update_many_bgr(self, items, scale_factor=None):
        """items: (camera, image [H, W, 3] uint8 BGR, result, ids) tuples; otherwise as `update_many_nv12`."""
        return self._update('bgr', items, scale_factor, 'update_many')

    def update_bgr(self, image, result, ids, scale_factor=None, camera=0):
        """One frame of `camera` -> dict(ids=, sim=)."""
        return self._update('bgr', [(camera, image, result, ids)], scale_factor, 'update')[0]

    def _describe(self, kind, surfaces, width, results, scale_factor, who):
        single, surf, _ = _surfaces_and_poses(surfaces, results, who)
        results = [results] if single else list(results)
        widths = _per_surface(width, len(surf), 'width', (int, np.integer), who) if kind == 'nv12' else [None] * len(surf)
        entries = self._entries(surf, widths, results, scale_factor, who)
        ops._reid_items(who, kind, entries, self.K, (self.torso, self.legs))
        for i, entry in enumerate(entries):
            self._on_device(i, entry, who)
        outs = ops.reid_describe(kind, entries, self.K, (self.torso, self.legs), score_thr=self.score_thr,
                                 kpt_thr=self.kpt_thr)
        return outs[0] if single else outs

    def describe_nv12(self, surfaces, width, results, scale_factor=None):
        """Stateless: the descriptors of the poses on one surface or a list of them -> dict(hist [N, 2, 256], count
        [N, 2]) of int32 device tensors (a list of them for a list): region 0 the torso, 1 the legs; count is the
        samples read, 0 where the region is invalid (hist is then zero)."""
        return self._describe('nv12', surfaces, width, results, scale_factor, 'PersonReID.describe_nv12')

    def describe_bgr(self, images, results, scale_factor=None):
        """`describe_nv12` for [H, W, 3] uint8 BGR pictures."""
        return self._describe('bgr', images, None, results, scale_factor, 'PersonReID.describe_bgr')

    def reset(self, camera=None):
        """Frees the slots of `camera` (None: of every camera); its frame count and drop count restart at 0.  The
        person-id counter goes on, so an id is never used twice; with every camera reset the gallery may take
        pictures of the other kind."""
        if camera is not None:
            camera = self._camera(camera, 'PersonReID.reset')
        else:
            self.kind = None
        if self._state is None:
            return
        c = slice(None) if camera is None else camera
        for name in ('person', 'frame', 'dropped'):
            self._state[name][c] = 0

    def state(self, camera=0):
        """Views of one camera's gallery on the device: person, track, last [S] (person 0 = free slot; its other
        fields mean nothing), hits [S, 2], hist [S, 2, 256], frame, next, dropped (0-d).  None before the first
        call."""
        camera = self._camera(camera, 'PersonReID.state')
        if self._state is None:
            return None
        return {name: self._state[name][camera] for name in _STATE}
