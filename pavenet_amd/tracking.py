"""Track ids for the live path (``csrc/pave_track.hip``): the unordered poses of a frame linked to
the poses of the frames before it, on the device, by an integer-exact greedy key-point-agreement rule.  ``update``
takes what ``push()`` / ``infer_video`` yield -- the (bboxes, labels, kpts) device tuple, or the fixed-shape
``dict(bboxes=, kpts=, keep=)`` of ``head.get_bboxes`` -- and returns a device int32 [N] tensor of ids (0 = not
tracked) without reading a device value on the host.  Ids are per camera, start at 1 and are never reused.

With ``motion='constant_velocity'`` (section 14, "Motion") a track also keeps a velocity, measured at every match
and smoothed, and a pose is compared with where the track is predicted to be, so links survive fast walks, gaps
and crossings.  The default, ``motion=None``, is the plain rule.

Not built: Kalman filtering, per-key-point velocities (``smoothing.PoseSmoother`` keeps them, for the picture only),
cross-camera identities, optimal assignment.  (Appearance re-identification is ``reid.PersonReID``, a stage after
this one: DESIGN section 18.)
"""
import math

import torch

from . import native, ops
from .heads import OKS_SIGMAS_POSETRACK15
from .render import _poses, _scales

# per-key-point OKS sigmas, in keypoints.py's orders
COCO_SIGMAS = [.026, .025, .025, .035, .035, .079, .079, .072, .072, .062, .062, .107, .107, .087, .087, .089, .089]
CROWDPOSE_SIGMAS = [.079, .079, .072, .072, .062, .062, .107, .107, .087, .087, .089, .089, .079, .079]
SIGMAS = {17: COCO_SIGMAS, 15: [s / 10.0 for s in OKS_SIGMAS_POSETRACK15], 14: CROWDPOSE_SIGMAS}


def pair_constants(sigmas, match_thr=0.5):
    """C[k] = max(1, rint(ln(1 / match_thr) (2 sigma_k)^2 2^20)) in double: key point k of a pair agrees iff
    (d2_k << 20) <= C[k] (area_d + area_t), which is "the OKS of key point k >= match_thr" with the mean of the two
    box areas as the object scale."""
    match_thr = float(match_thr)
    if not 0.0 < match_thr < 1.0:
        raise ValueError(f'PoseTracker: match_thr must lie in (0, 1), got {match_thr}')
    C = []
    for s in sigmas:
        s = float(s)
        if not (s > 0.0 and math.isfinite(s)):
            raise ValueError(f'PoseTracker: sigmas must be positive and finite, got {s}')
        c = max(1, int(round(math.log(1.0 / match_thr) * (2.0 * s) ** 2 * 2.0 ** 20)))
        if c >= 1 << 24:
            raise ValueError(f'PoseTracker: sigma {s} at match_thr {match_thr} gives a pair constant {c} >= 2^24')
        C.append(c)
    return C


class PoseTracker:
    """Links poses of K key points across the frames of `cameras` cameras.  A camera keeps `max_tracks` (1 .. 128)
    slots; a slot not matched for more than `max_age` frames is freed; a pose is tracked iff its box score is >
    `score_thr` (and keep, and finite coordinates), a key point counts iff its score is > `kpt_thr`; a pose and a
    track are linked only if at least `min_kpts` (default max(1, (K + 2) // 3)) key points visible in both lie
    within the distance at which their OKS term is `match_thr`.  `sigmas`: K per-key-point OKS sigmas; built in
    for K = 17 (COCO), 15 (PoseTrack) and 14 (CrowdPose).

    `motion`: None, or 'constant_velocity': a track keeps a velocity (one for the whole pose, 1/16 quarter pixel per
    frame), the mean displacement of the co-visible key points per frame at every match, mixed into the old one with
    weight `velocity_gain` / 16 (an integer 1 .. 16); a pose is compared with the track's points moved by velocity x
    min(frames since its last match, `max_predict`) (an integer 0 .. 255; None: min(max_age, 255)); a track matched
    only once has no velocity yet, and its agreement test is `new_gate` (an integer 1 .. 16) times wider in C[k],
    sqrt(new_gate) times in distance.  The three are arguments of the motion model: given without it they raise."""

    def __init__(self, K, cameras=1, max_tracks=128, max_age=30, match_thr=0.5, min_kpts=None, score_thr=0.3,
                 kpt_thr=0., sigmas=None, motion=None, velocity_gain=None, max_predict=None, new_gate=None):
        K = int(K)
        if not 1 <= K <= native.TRACK_MAX_K:
            raise ValueError(f'PoseTracker: K in 1 .. {native.TRACK_MAX_K}, got {K}')
        if sigmas is None:
            if K not in SIGMAS:
                raise ValueError(f'PoseTracker: no built-in sigmas for K = {K} (built in: {sorted(SIGMAS)}); pass '
                                 'sigmas=')
            sigmas = SIGMAS[K]
        sigmas = list(sigmas)
        if len(sigmas) != K:
            raise ValueError(f'PoseTracker: one sigma per key point ({K}), got {len(sigmas)}')
        self.C = pair_constants(sigmas, match_thr)
        if int(cameras) != cameras or not 1 <= cameras <= native.TRACK_MAX_CAMERAS:
            raise ValueError(f'PoseTracker: cameras is an integer in 1 .. {native.TRACK_MAX_CAMERAS}, got {cameras!r}')
        if int(max_tracks) != max_tracks or not 1 <= max_tracks <= native.TRACK_MAX_TRACKS:
            raise ValueError(f'PoseTracker: max_tracks is an integer in 1 .. {native.TRACK_MAX_TRACKS}, got '
                             f'{max_tracks!r}')
        if int(max_age) != max_age or max_age < 0:
            raise ValueError(f'PoseTracker: max_age is an integer >= 0, got {max_age!r}')
        if min_kpts is None:
            min_kpts = max(1, (K + 2) // 3)
        if int(min_kpts) != min_kpts or not 1 <= min_kpts <= K:
            raise ValueError(f'PoseTracker: min_kpts is an integer in 1 .. K = {K}, got {min_kpts!r}')
        self.K, self.cameras, self.max_tracks, self.max_age = K, int(cameras), int(max_tracks), int(max_age)
        self.min_kpts, self.score_thr, self.kpt_thr = int(min_kpts), float(score_thr), float(kpt_thr)
        self.match_thr = float(match_thr)
        if motion not in (None, 'constant_velocity'):
            raise ValueError(f"PoseTracker: motion is None or 'constant_velocity', got {motion!r}")
        if motion is None:
            given = [n for n, v in (('velocity_gain', velocity_gain), ('max_predict', max_predict),
                                    ('new_gate', new_gate)) if v is not None]
            if given:
                raise ValueError(f'PoseTracker: {", ".join(given)} given with motion=None: they are arguments of '
                                 "motion='constant_velocity'")
        else:
            velocity_gain = 8 if velocity_gain is None else velocity_gain
            new_gate = 4 if new_gate is None else new_gate
            max_predict = min(self.max_age, 255) if max_predict is None else max_predict
            for name, v, lo, hi in (('velocity_gain', velocity_gain, 1, 16), ('max_predict', max_predict, 0, 255),
                                    ('new_gate', new_gate, 1, 16)):
                if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
                    raise ValueError(f'PoseTracker: {name} is an integer in {lo} .. {hi}, got {v!r}')
        self.motion, self.velocity_gain, self.max_predict, self.new_gate = motion, velocity_gain, max_predict, new_gate
        self._state = self._scratch = None

    def _allocate(self, dev):
        C, M, K = self.cameras, self.max_tracks, self.K
        z = dict(dtype=torch.int32, device=dev)
        self._state = dict(id=torch.zeros((C, M), **z), last=torch.zeros((C, M), **z),
                           kpts=torch.zeros((C, M, K, 2), **z), vis=torch.zeros((C, M), **z),
                           area=torch.zeros((C, M), **z), frame=torch.zeros((C,), **z), next_id=torch.ones((C,), **z),
                           dropped=torch.zeros((C,), **z))
        if self.motion is not None:
            self._state.update(vel=torch.zeros((C, M, 2), **z), hits=torch.zeros((C, M), **z))
        self._scratch = ops.track_scratch(dev)

    def _camera(self, camera, who):
        if isinstance(camera, bool) or int(camera) != camera or not 0 <= camera < self.cameras:
            raise ValueError(f'{who}: camera must be an integer in [0, {self.cameras}), got {camera!r}')
        return int(camera)

    def update_many(self, items, scale_factor=None):
        """items: (camera, result) pairs, the entries of one camera in time order (as ``MultiLiveVideoPose.push``
        sorts its output) -> one int32 [N_i] device tensor of ids per item.  scale_factor: None for results made
        with rescale=True, else the img_meta's scale_factor, or one per item.  One launch per 32 items."""
        who = 'PoseTracker.update'
        items = list(items)
        if any(not (isinstance(it, (tuple, list)) and len(it) == 2) for it in items):
            raise ValueError(f'{who}: items are (camera, result) pairs')
        if not items:
            return []
        cams = [self._camera(c, who) for c, _ in items]
        poses = [_poses(r, i, who) for i, (_, r) in enumerate(items)]
        scales = _scales(scale_factor, len(items), who)
        if any(not (0 < sx < float('inf') and 0 < sy < float('inf')) for sx, sy in scales):
            raise ValueError(f'{who}: a scale factor must be positive and finite')
        for i, (kpts, bboxes, keep) in enumerate(poses):
            if kpts.shape[1] != self.K:
                raise ValueError(f'{who}: results[{i}] has K = {kpts.shape[1]}, the tracker K = {self.K}')
            if kpts.shape[0] > native.TRACK_MAX_POSES:
                raise ValueError(f'{who}: results[{i}] has {kpts.shape[0]} poses, at most {native.TRACK_MAX_POSES}')
            if not all(t is None or t.is_cuda for t in (kpts, bboxes, keep)):
                raise ValueError(f'{who}: results[{i}] must hold HIP device tensors (pavenet_amd has no CPU path)')
        dev = poses[0][0].device
        if self._state is not None and self._state['id'].device != dev:
            raise ValueError(f"{who}: the tracker's state is on {self._state['id'].device}, results[0] on {dev}")
        entries = [(kp, bb, keep, c, sc) for (kp, bb, keep), c, sc in zip(poses, cams, scales)]
        if self._state is None:
            self._allocate(dev)
        motion = None if self.motion is None else (self._state['vel'], self._state['hits'], self.velocity_gain,
                                                   self.max_predict, self.new_gate)
        return ops.track_poses(entries, self._state, self._scratch, self.C, min_kpts=self.min_kpts,
                               max_age=self.max_age, score_thr=self.score_thr, kpt_thr=self.kpt_thr, motion=motion)

    def update(self, result, scale_factor=None, camera=0):
        """One frame of `camera` -> int32 [N] ids on the device, 0 = not tracked."""
        return self.update_many([(camera, result)], scale_factor)[0]

    def reset(self, camera=None):
        """Frees the slots of `camera` (None: of every camera); its ids restart at 1 and its frame count and drop
        count at 0.  The state tensors stay where they are (a birth writes a slot's velocity and hits, and a free
        slot's are never read)."""
        if camera is not None:
            camera = self._camera(camera, 'PoseTracker.reset')
        if self._state is None:
            return
        c = slice(None) if camera is None else camera
        for name, v in (('id', 0), ('frame', 0), ('next_id', 1), ('dropped', 0)):
            self._state[name][c] = v

    def state(self, camera=0):
        """Views of one camera's state on the device: id, last, area [M] (id 0 = free slot; its other fields mean
        nothing), vis [M] (bit k = key point k visible; the uint32 mask as int32), kpts [M, K, 2] quarter pixels,
        frame, next_id, dropped (0-d); with a motion model also vel [M, 2] (1/16 quarter pixel per frame) and hits
        [M] (the matches of the track, its birth included).  None before the first update."""
        camera = self._camera(camera, 'PoseTracker.state')
        if self._state is None:
            return None
        return {name: t[camera] for name, t in self._state.items()}
