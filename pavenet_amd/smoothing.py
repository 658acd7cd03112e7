"""Steady poses for the live path (``csrc/pave_smooth.hip``): a per-track adaptive exponential
filter between ``PoseTracker.update`` and the draw, on the device, by an integer-exact rule.  ``smooth`` takes what
``push()`` / ``infer_video`` yield -- the (bboxes, labels, kpts) device tuple, or the fixed-shape
``dict(bboxes=, kpts=, keep=)`` of ``head.get_bboxes`` -- with the frame's track ids, and returns the result in the
same form with the key points and boxes filtered, in original-image pixels (downstream calls take
``scale_factor=None``), without reading a device value on the host.

The filter lags what it follows: anonymise with the raw result and draw the smoothed one.

Not built: per-axis gains, a look-ahead over the T // 2 frames of latency the live path already has, smoothing of
scores.
"""
import torch

from . import native, ops
from .tracked import Tracked

_STATE = ('id', 'last', 'pos', 'vel', 'frame', 'dropped')


class PoseSmoother(Tracked):
    """Filters the K key points and the box corners of tracked poses over the frames of `cameras` cameras.  A camera
    keeps `max_tracks` (1 .. 128) slots, one per track id; a slot not seen for more than `max_age` frames is freed.
    A pose is filtered iff its box score is > `score_thr` (and keep, and finite coordinates), its id is >= 1 and no
    pose before it in the frame has the same id; every other pose passes through, snapped to quarter pixels.  A key
    point with a score <= `kpt_thr` passes through and starts afresh when it is seen again.

    A point's position follows its detection with a gain of alpha / 256 per frame, alpha = min(256, `alpha_min` +
    `beta` u / 16), u the point's smoothed speed in 1/1024 of the pose's size per frame: `alpha_min` (1 .. 256) is
    the gain at rest (256: no filter), `beta` (0 .. 4096) how fast a moving point gets its detection back (0: a fixed
    exponential filter), `velocity_gain` / 16 (1 .. 16) the weight of the newest frame in the speed."""
    _NOUN, _NOUNS = 'the smoother', "the smoother's"

    def __init__(self, K, cameras=1, max_tracks=128, max_age=30, alpha_min=32, beta=128, velocity_gain=3,
                 score_thr=0.3, kpt_thr=0.):
        who = 'PoseSmoother'
        if isinstance(K, bool) or int(K) != K or not 1 <= K <= native.TRACK_MAX_K:
            raise ValueError(f'{who}: K is an integer in 1 .. {native.TRACK_MAX_K}, got {K!r}')
        for name, v, lo, hi in (('cameras', cameras, 1, native.TRACK_MAX_CAMERAS),
                                ('max_tracks', max_tracks, 1, native.TRACK_MAX_TRACKS),
                                ('alpha_min', alpha_min, 1, 256), ('beta', beta, 0, 4096),
                                ('velocity_gain', velocity_gain, 1, 16)):
            if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
                raise ValueError(f'{who}: {name} is an integer in {lo} .. {hi}, got {v!r}')
        if isinstance(max_age, bool) or int(max_age) != max_age or max_age < 0:
            raise ValueError(f'{who}: max_age is an integer >= 0, got {max_age!r}')
        self.K, self.cameras, self.max_tracks, self.max_age = int(K), cameras, max_tracks, int(max_age)
        self.alpha_min, self.beta, self.velocity_gain = alpha_min, beta, velocity_gain
        self.score_thr, self.kpt_thr = float(score_thr), float(kpt_thr)
        self._state = None

    def _allocate(self, dev):
        C, S, J = self.cameras, self.max_tracks, self.K + 2
        z = dict(dtype=torch.int32, device=dev)
        self._state = dict(id=torch.zeros((C, S), **z), last=torch.zeros((C, S), **z),
                           pos=torch.zeros((C, S, J, 2), **z), vel=torch.zeros((C, S, J, 2), **z),
                           frame=torch.zeros((C,), **z), dropped=torch.zeros((C,), **z))

    def smooth_many(self, items, scale_factor=None):
        """items: (camera, result, ids) triples, the entries of one camera in time order -> one result per item, in
        the form it was given: (bboxes, labels, kpts) with the same labels tensor, or dict(bboxes=, kpts=, keep=)
        with the same keep tensor.  ids: the int32 [N] device tensor `PoseTracker.update` returned for the result.
        scale_factor: what the tracker was given (None for results made with rescale=True); the results that come
        back are in original-image pixels.  One launch per 32 items."""
        items = list(items)
        entries = self._entries(items, scale_factor, 'PoseSmoother.smooth')
        if not entries:
            return []
        outs = ops.smooth_poses(entries, self._state, max_age=self.max_age, alpha_min=self.alpha_min, beta=self.beta,
                                velocity_gain=self.velocity_gain, score_thr=self.score_thr, kpt_thr=self.kpt_thr)
        results = []
        for (_, given, _), (kpts, bboxes) in zip(items, outs):
            if isinstance(given, dict):
                batched = given['bboxes'].dim() == 3
                results.append(dict(bboxes=bboxes[None] if batched else bboxes, kpts=kpts[None] if batched else kpts,
                                    keep=given.get('keep')))
            else:
                results.append((bboxes, given[1], kpts))
        return results

    def smooth(self, result, ids, scale_factor=None, camera=0):
        """One frame of `camera` with its track ids -> the result in the same form, filtered, in original-image
        pixels."""
        return self.smooth_many([(camera, result, ids)], scale_factor)[0]

    def reset(self, camera=None):
        """Frees the slots of `camera` (None: of every camera); its frame count and drop count restart at 0.  The
        state tensors stay where they are (a birth writes a slot's points, and a free slot's are never read)."""
        self._reset(camera)

    def state(self, camera=0):
        """Views of one camera's state on the device: id, last [S] (id 0 = free slot; its other fields mean
        nothing), pos, vel [S, K + 2, 2] (1/64 pixel and 1/64 pixel per frame; the key points, then the box corners;
        pos x < 0: the point is not initialised), frame, dropped (0-d).  None before the first call."""
        return self._views(camera, 'state', _STATE)
