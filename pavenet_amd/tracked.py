"""What the classes that follow track ids through per-camera slots share (the device side is
``csrc/pave_tracked.h``): ``PoseSmoother``, ``ZoneMonitor``, ``PostureMonitor``, ``FootfallMap``, ``TrackTrails`` and
``GroundPlane`` take the same (camera, result, ids) items, turn them into the entries of one ``ops`` call in the same
way, and reset and show a state of named int32 tensors whose first axis is the camera.  ``ContactMonitor`` takes
``GroundPlane``'s output and not a result: it checks its items itself and shares the camera check, the reset and the
views.  ``PoseTracker`` and ``PersonReID`` take other items and are not built on this.
"""
import torch

from . import native
from .render import _poses, _scales


class Tracked:
    """A subclass names itself in messages (`_NOUN`, `_NOUNS`: "the monitor", "the monitor's"), lists the tensors a
    reset zeroes (`_RESET`) and allocates `self._state`, a dict of device tensors with 'id' among them, in
    `_allocate(device)`; `self.K` and `self.cameras` are set by its constructor."""
    _NOUN, _NOUNS = None, None
    _RESET = ('id', 'frame', 'dropped')
    _state = None

    def _camera(self, camera, who):
        if isinstance(camera, bool) or int(camera) != camera or not 0 <= camera < self.cameras:
            raise ValueError(f'{who}: camera must be an integer in [0, {self.cameras}), got {camera!r}')
        return int(camera)

    def _entries(self, items, scale_factor, who):
        """The (kpts, bboxes, keep, ids, camera, (sx, sy)) entries of (camera, result, ids) items for an ``ops`` call,
        with the state allocated on their device; [] for no items."""
        if any(not (isinstance(it, (tuple, list)) and len(it) == 3) for it in items):
            raise ValueError(f'{who}: items are (camera, result, ids) triples')
        if not items:
            return []
        cams = [self._camera(c, who) for c, _, _ in items]
        poses = [_poses(r, i, who) for i, (_, r, _) in enumerate(items)]
        scales = _scales(scale_factor, len(items), who)
        if any(not (0 < sx < float('inf') and 0 < sy < float('inf')) for sx, sy in scales):
            raise ValueError(f'{who}: a scale factor must be positive and finite')
        all_ids = []
        for i, ((kpts, bboxes, keep), (_, _, ids)) in enumerate(zip(poses, items)):
            if kpts.shape[1] != self.K:
                raise ValueError(f'{who}: results[{i}] has K = {kpts.shape[1]}, {self._NOUN} K = {self.K}')
            if kpts.shape[0] > native.TRACK_MAX_POSES:
                raise ValueError(f'{who}: results[{i}] has {kpts.shape[0]} poses, at most {native.TRACK_MAX_POSES}')
            if not (isinstance(ids, torch.Tensor) and ids.dtype == torch.int32
                    and tuple(ids.shape) == (kpts.shape[0],)):
                raise ValueError(f'{who}: ids of results[{i}] must be an int32 [{kpts.shape[0]}] tensor')
            if not all(t is None or t.is_cuda for t in (kpts, bboxes, keep, ids)):
                raise ValueError(f'{who}: results[{i}] and its ids must be HIP device tensors (pavenet_amd has no CPU '
                                 'path)')
            all_ids.append(ids.contiguous())
        dev = poses[0][0].device
        if self._state is not None and self._state['id'].device != dev:
            raise ValueError(f"{who}: {self._NOUNS} state is on {self._state['id'].device}, results[0] on {dev}")
        if self._state is None:
            self._allocate(dev)
        return [(kp, bb, keep, ids, c, sc) for (kp, bb, keep), ids, c, sc in zip(poses, all_ids, cams, scales)]

    def _reset(self, camera):
        if camera is not None:
            camera = self._camera(camera, f'{type(self).__name__}.reset')
        if self._state is None:
            return
        c = slice(None) if camera is None else camera
        for name in self._RESET:
            self._state[name][c] = 0

    def _views(self, camera, method, names):
        """{name: one camera's part of state tensor `name`}, or None before the first call."""
        camera = self._camera(camera, f'{type(self).__name__}.{method}')
        if self._state is None:
            return None
        return {name: self._state[name][camera] for name in names}
