"""Live and long video: the frame-by-frame form of `streaming.VideoPoseStream` on a bounded ring.

A window only ever reads the last T frames, so a ring of R = T - 1 + max_push slots serves a video of any length:
frame f lives in slot f mod R, and the fused T-frame kernels, which address the projected values through a frame
table, take slot indices as that table -- the decoders run the kernels `infer_video` runs.

    live = LiveVideoPose(model, img_meta, max_push=1, decode_chunk=4, rescale=False)
    for frame in source:                          # [3, Hp, Wp] or [n, 3, Hp, Wp] fp32 canvas, n <= max_push
        for index, result in live.push(frame):    # zero or more (frame index, (bboxes, labels, kpts))
            ...
    for index, result in live.flush():            # the last T // 2 frames, right edge replicated
        ...
    live.reset()                                  # next video: the slots are reused, nothing is reallocated

Latency rule: the windows are exactly `VideoPoseStream.window_indices(N, T)` of the N frames seen between `reset()`
and `flush()`.  Centre c needs frame c + T // 2, so the push that delivers that frame emits it; `flush()` emits the
centres that wait for frames that will not come, with min(c + k, N - 1) in their place.

Resident memory: the ring holds, per slot, the encoder memory [S, C] and the five decoder layers' projected values
[S, 8, 32] each -- 137 MB per slot at 800x1344, i.e. R x 137 MB = 0.96 GB for T = 7 and max_push = 1, independent
of the video's length (`infer_video` keeps 137 MB per frame of the video).  Everything is allocated by the first
push.  Padded metas (img_shape smaller than the canvas) keep the memory slabs only (23 MB per slot), as `encode`
does, and decode projects the values per window.

Under `set_batch_invariant` the results equal `infer_video`'s bit for bit; in the default mode the same windows are
decoded with other launch shapes and agree to rounding.

Several cameras share one object, one ring and one launch chain:

    multi = MultiLiveVideoPose(model, img_meta, cameras=4, max_push=1, decode_chunk=4)
    for batch in source:                                   # {camera: [3, Hp, Wp] or [n, 3, Hp, Wp]}, any subset
        for camera, index, result in multi.push(batch):    # sorted by (camera, index)
            ...
    multi.flush(camera=None)                               # one camera's last T // 2 frames, or every camera's
    multi.reset(camera=None)                               # that camera's next video in the same rows

`CameraRing` holds cameras x R rows, frame f of camera c in row c * R + f mod R, so the windows of different cameras
are row lists into the same tensors and go through one decode batch; the frames of a push are encoded in one batch
and written to their rows by one `ops.scatter_rows` launch.  Per camera the semantics are `LiveVideoPose`'s, and
under `set_batch_invariant` so are the results, bit for bit.
"""
import torch

from . import ops
from .bricks import batch_invariant_scope
from .streaming import FrameSlabs, VideoPoseStream


class RingSlabs(FrameSlabs):
    """FrameSlabs over R reused slots: element s is row s of one [R, S, C] tensor, `values` are [R, S, 8, 32] per
    decoder layer, and the frames `VideoPoseStream._encode` appends are written to rows (frame index) mod R."""

    def __init__(self, n_slots):
        super().__init__()
        self.n_slots = n_slots
        self.memory = None       # [R, S, C], allocated by the first frames
        self.n_frames = 0        # frames written since reset(): frame f is in slot f % R while f >= n_frames - R

    def _rows(self, first, n):
        """Frames first .. first + n - 1 as (slot range, source range) pairs: two when the ring wraps."""
        assert n <= self.n_slots, 'more frames in one chunk than the ring has slots'
        start = first % self.n_slots
        head = min(n, self.n_slots - start)
        return [(slice(start, start + head), slice(0, head))] + ([(slice(0, n - head), slice(head, n))] if head < n else [])

    def _append_memory(self, memory):
        if self.memory is None:
            self.memory = memory.new_empty((self.n_slots,) + tuple(memory.shape[1:]))
            self.extend(self.memory.unbind(0))
        assert memory.shape[1:] == self.memory.shape[1:], 'frames of another canvas size than the ring was built for'
        for dst, src in self._rows(self.n_frames, memory.shape[0]):
            self.memory[dst].copy_(memory[src])
        self.n_frames += memory.shape[0]

    def _append_values(self, vals, n_pose, expected_total):
        if self.values is None:
            flat = [v.new_empty((self.n_slots,) + tuple(v.shape[1:])) for v in vals]
            self.values = (flat[:n_pose], flat[n_pose:])
        for dst, src in self._rows(self.n_cached, vals[0].shape[0]):
            for c, v in zip(self.values[0] + self.values[1], vals):
                c[dst].copy_(v[src])
        self.n_cached += vals[0].shape[0]

    def covers(self, indices):
        """`indices` are slots: every one holds a frame of this video, with its projected values."""
        return (self.values is not None and self.n_cached == self.n_frames
                and 0 <= min(indices) and max(indices) < min(self.n_frames, self.n_slots))

    def reset(self):
        """Next video: the slots (and their addresses) stay, none of them holds a frame."""
        self.n_frames = 0
        self.n_cached = 0

    def tensors(self):
        """What the ring keeps resident: the memory tensor and the value caches."""
        vals = [] if self.values is None else self.values[0] + self.values[1]
        return ([] if self.memory is None else [self.memory]) + vals

    def resident_bytes(self):
        return sum(t.numel() * t.element_size() for t in self.tensors())

    def fill_(self, value):
        """tests/: overwrite every slot (a window that reads a slot no frame of this video was written to shows)."""
        for t in self.tensors():
            t.fill_(value)


class LiveVideoPose:
    """Frame-by-frame `VideoPoseStream.infer_video` with bounded memory (module docstring)."""

    def __init__(self, model, img_meta, max_push=1, decode_chunk=4, rescale=False, cache_values=True):
        if max_push < 1 or decode_chunk < 1:
            raise ValueError('LiveVideoPose: max_push and decode_chunk are at least 1')
        self.stream = VideoPoseStream(model, img_meta, encode_chunk=max_push, decode_chunk=decode_chunk,
                                      cache_values=cache_values)
        self.model = model
        self.T = self.stream.T
        self.max_push = max_push
        self.decode_chunk = decode_chunk
        self.rescale = rescale
        self.ring = RingSlabs(self.T - 1 + max_push)
        self.n_seen = 0          # frames pushed since reset()
        self.next_centre = 0     # the first frame whose result has not been emitted
        self._canvas = None      # (H, W) of the first push

    @staticmethod
    def _windows(first, last, n_seen, T, n_slots):
        """Centres first .. last of a video of which n_seen frames exist -> (centres, windows of frame indices,
        windows of slots).  Frames beyond the last one seen are replaced by it (flush), those before 0 by 0."""
        h = T // 2
        centres = list(range(first, last + 1))
        frames = [[min(max(c + k, 0), n_seen - 1) for k in range(-h, h + 1)] for c in centres]
        return centres, frames, [[f % n_slots for f in w] for w in frames]

    @classmethod
    def schedule(cls, n_frames, T, pushes, max_push=None):
        """What a video of n_frames frames delivered in pushes of `pushes` frames emits, in pure Python: one
        (centres, windows as frame indices, windows as slots) tuple per push and a last one for the flush.  The
        ring has T - 1 + max_push slots (max_push: the largest push when not given)."""
        pushes = list(pushes)
        if sum(pushes) != n_frames or any(p < 1 for p in pushes):
            raise ValueError('schedule: the pushes are positive and add up to n_frames')
        max_push = max(pushes) if max_push is None else max_push
        if max(pushes) > max_push:
            raise ValueError('schedule: a push larger than max_push')
        R, h = T - 1 + max_push, T // 2
        out, seen, nxt = [], 0, 0
        for p in pushes:
            seen += p
            out.append(cls._windows(nxt, seen - 1 - h, seen, T, R))
            nxt = max(nxt, seen - h)
        out.append(cls._windows(nxt, seen - 1, seen, T, R))
        return out

    def _emit(self, last):
        """Decode centres next_centre .. last from the ring."""
        centres, _, slots = self._windows(self.next_centre, last, self.n_seen, self.T, self.ring.n_slots)
        out = []
        for i in range(0, len(centres), self.decode_chunk):
            res = self.stream._decode(self.ring, slots[i:i + self.decode_chunk], self.rescale, None, None)
            out.extend(zip(centres[i:i + self.decode_chunk], self.stream.head.results_to_list(res)))
        self.next_centre = max(self.next_centre, last + 1)
        return out

    @torch.no_grad()
    def push(self, frames):
        """frames [3, Hp, Wp] or [n, 3, Hp, Wp] (n <= max_push) fp32 canvases on the device, the next n frames of
        the video -> list of (frame index, (bboxes, labels, kpts)) of the centres these frames complete."""
        if not isinstance(frames, torch.Tensor) or frames.dim() not in (3, 4):
            raise ValueError('push: a [3, H, W] or [n, 3, H, W] tensor')
        if not frames.is_cuda:
            raise ValueError('push: frames must be on the device (pavenet_amd has no host path)')
        frames = frames[None] if frames.dim() == 3 else frames
        n = frames.shape[0]
        if n < 1 or n > self.max_push:
            raise ValueError(f'push: {n} frames, this ring takes 1 .. max_push = {self.max_push} per push')
        canvas = tuple(frames.shape[1:])
        if self._canvas is None:
            self._canvas = canvas
        elif canvas != self._canvas:
            raise ValueError(f'push: canvas {canvas}, the first push had {self._canvas}')
        with batch_invariant_scope(self.model):
            self.stream._encode(frames, self.ring)
            self.n_seen += n
            return self._emit(self.n_seen - 1 - self.T // 2)

    @torch.no_grad()
    def flush(self):
        """End of the video: the centres that wait for frames that will not come, right edge replicated."""
        if self.n_seen == 0:
            return []
        with batch_invariant_scope(self.model):
            return self._emit(self.n_seen - 1)

    def reset(self):
        """Start the next video at frame 0 in the same slots."""
        self.ring.reset()
        self.n_seen = 0
        self.next_centre = 0


class CameraRing(FrameSlabs):
    """FrameSlabs over cameras x R reused rows of one [cameras * R, S, C] tensor (and one [cameras * R, S, 8, 32]
    tensor per decoder layer): frame f of camera c lives in row c * R + f % R.  `plan()` names the (camera, frame)
    of the frames the next `_append_memory` / `_append_values` calls deliver, in their order."""

    def __init__(self, cameras, n_slots):
        self.cameras = cameras   # (before FrameSlabs.__init__, which assigns n_cached)
        self.n_slots = n_slots   # R, rows per camera
        super().__init__()
        self.memory = None                 # [cameras * R, S, C], allocated by the first frames
        self.n_frames = [0] * cameras      # per camera: frames written since its reset()
        self._plan_memory = []             # (camera, frame) of the frames still to come, for the memory ...
        self._plan_values = []             # ... and for the projected values
        self._held = None                  # (memory, rows) of a chunk whose write waits for its values

    @property
    def n_cached(self):
        """Per camera: frames whose projected values are in `values`."""
        return self._n_cached

    @n_cached.setter
    def n_cached(self, value):
        # FrameSlabs.__init__, and `_encode` after a chunk without values, assign 0: no camera has a cache
        assert value == 0, 'CameraRing.n_cached is per camera'
        self._n_cached = [0] * self.cameras

    def row(self, camera, frame):
        return camera * self.n_slots + frame % self.n_slots

    def plan(self, entries):
        """entries: (camera, frame) of every frame of the next `_encode` call, in batch order."""
        assert not self._plan_memory and self._held is None, 'frames of the last plan were not delivered'
        # (the values' plan is left over when a chunk came without values: padded metas, cache_values=False)
        self._plan_memory, self._plan_values = list(entries), list(entries)

    def _take(self, pending, n, counters):
        """The next n planned frames -> their rows; every frame is its camera's next one."""
        assert n <= len(pending), 'more frames than the plan names'
        taken = pending[:n]
        del pending[:n]
        rows = []
        for c, f in taken:
            assert f == counters[c], f'camera {c}: frame {f} planned, frame {counters[c]} is next'
            rows.append(self.row(c, f))
            counters[c] += 1
        assert len(set(rows)) == n, 'more frames of one camera in one chunk than it has rows'
        return rows

    @staticmethod
    def _write(srcs, dsts, rows):
        if dsts[0].is_cuda:
            ops.scatter_rows([s.contiguous() for s in srcs], dsts, rows)
        else:   # host tensors (CPU tests)
            for s, d in zip(srcs, dsts):
                d[rows] = s

    def commit(self):
        """Write a held chunk of memory whose values did not come (padded metas, cache_values=False)."""
        if self._held is not None:
            memory, rows = self._held
            self._held = None
            self._write([memory], [self.memory], rows)

    def _append_memory(self, memory):
        self.commit()
        if self.memory is None:
            self.memory = memory.new_empty((self.cameras * self.n_slots,) + tuple(memory.shape[1:]))
            self.extend(self.memory.unbind(0))
        assert memory.shape[1:] == self.memory.shape[1:], 'frames of another canvas size than the ring was built for'
        # the write waits for `_append_values` of the same chunk: one launch for all six tensors
        self._held = (memory, self._take(self._plan_memory, memory.shape[0], self.n_frames))

    def _append_values(self, vals, n_pose, expected_total):
        if self.values is None:
            flat = [v.new_empty((self.cameras * self.n_slots,) + tuple(v.shape[1:])) for v in vals]
            self.values = (flat[:n_pose], flat[n_pose:])
        rows = self._take(self._plan_values, vals[0].shape[0], self._n_cached)
        srcs, dsts = list(vals), self.values[0] + self.values[1]
        if self._held is not None:
            memory, held_rows = self._held
            assert held_rows == rows, 'values of other frames than the memory before them'
            self._held = None
            srcs, dsts = [memory] + srcs, [self.memory] + dsts
        self._write(srcs, dsts, rows)

    def covers(self, indices):
        """`indices` are rows: every one holds a frame of its camera's video, with its projected values."""
        if self.values is None or self._held is not None:
            return False
        for r in indices:
            c, s = divmod(int(r), self.n_slots)
            if not (0 <= c < self.cameras and self._n_cached[c] == self.n_frames[c]
                    and s < min(self.n_frames[c], self.n_slots)):
                return False
        return True

    def reset(self, camera=None):
        """That camera's (None: every camera's) next video: the rows and their addresses stay."""
        for c in range(self.cameras) if camera is None else [camera]:
            self.n_frames[c] = 0
            self._n_cached[c] = 0

    tensors = RingSlabs.tensors
    resident_bytes = RingSlabs.resident_bytes
    fill_ = RingSlabs.fill_


class MultiLiveVideoPose:
    """`LiveVideoPose` for several cameras on one `CameraRing`: one encode batch, one ring write and one decode
    batch per push, whatever cameras it names (module docstring)."""

    def __init__(self, model, img_meta, cameras, max_push=1, decode_chunk=4, encode_chunk=None, rescale=False,
                 cache_values=True):
        encode_chunk = cameras * max_push if encode_chunk is None else encode_chunk
        if cameras < 1 or max_push < 1 or decode_chunk < 1 or encode_chunk < 1:
            raise ValueError('MultiLiveVideoPose: cameras, max_push, decode_chunk and encode_chunk are at least 1')
        self.stream = VideoPoseStream(model, img_meta, encode_chunk=encode_chunk, decode_chunk=decode_chunk,
                                      cache_values=cache_values)
        self.model = model
        self.T = self.stream.T
        self.cameras = cameras
        self.max_push = max_push
        self.decode_chunk = decode_chunk
        self.rescale = rescale
        self.ring = CameraRing(cameras, self.T - 1 + max_push)
        self.n_seen = [0] * cameras        # per camera: frames pushed since its reset()
        self.next_centre = [0] * cameras   # per camera: the first frame whose result has not been emitted
        self._canvas = None                # (3, H, W) of the first push

    @staticmethod
    def _ready(T, R, camera, first, last, n_seen):
        """Centres first .. last of `camera` -> [(camera, centre, frame window, row window)]."""
        centres, frames, slots = LiveVideoPose._windows(first, last, n_seen, T, R)
        return [(camera, c, fw, [camera * R + s for s in sw]) for c, fw, sw in zip(centres, frames, slots)]

    @classmethod
    def schedule(cls, T, cameras, max_push, pushes):
        """What `pushes` (a list of {camera: number of frames}) and a final flush of all cameras emit, in pure
        Python: one list of (camera, centre, window as frame indices, window as ring rows) per push and a last one
        for the flush, each sorted by (camera, centre).  The ring has cameras x (T - 1 + max_push) rows."""
        R, h = T - 1 + max_push, T // 2
        seen, nxt, out = [0] * cameras, [0] * cameras, []
        for push in pushes:
            if not push or any(not 0 <= c < cameras or not 1 <= n <= max_push for c, n in push.items()):
                raise ValueError('schedule: a push names 1 or more cameras in range, 1 .. max_push frames each')
            step = []
            for c in sorted(push):
                seen[c] += push[c]
                step += cls._ready(T, R, c, nxt[c], seen[c] - 1 - h, seen[c])
                nxt[c] = max(nxt[c], seen[c] - h)
            out.append(step)
        out.append([item for c in range(cameras) if seen[c] for item in cls._ready(T, R, c, nxt[c], seen[c] - 1, seen[c])])
        return out

    def _emit(self, last):
        """Decode, in one run of decode batches, centres next_centre[c] .. last[c] of every camera c in `last`."""
        R = self.ring.n_slots
        items = [item for c in sorted(last)
                 for item in self._ready(self.T, R, c, self.next_centre[c], last[c], self.n_seen[c])]
        out = []
        for i in range(0, len(items), self.decode_chunk):
            part = items[i:i + self.decode_chunk]
            res = self.stream._decode(self.ring, [rows for _, _, _, rows in part], self.rescale, None, None)
            out.extend((c, centre, r) for (c, centre, _, _), r in zip(part, self.stream.head.results_to_list(res)))
        for c in last:
            self.next_centre[c] = max(self.next_centre[c], last[c] + 1)
        return out

    def _checked(self, batch):
        """The argument checks of a push, all before any device work -> [(camera, [n, 3, H, W])], cameras ascending."""
        if not isinstance(batch, dict) or not batch:
            raise ValueError('push: a non-empty {camera: frames} dict')
        canvas, out = self._canvas, []
        for c in batch:
            if isinstance(c, bool) or not isinstance(c, int) or not 0 <= c < self.cameras:
                raise ValueError(f'push: camera {c!r}, this ring serves cameras 0 .. {self.cameras - 1}')
        for c in sorted(batch):
            frames = batch[c]
            if not isinstance(frames, torch.Tensor) or frames.dim() not in (3, 4):
                raise ValueError(f'push: camera {c}: a [3, H, W] or [n, 3, H, W] tensor')
            if not frames.is_cuda:
                raise ValueError(f'push: camera {c}: frames must be on the device (pavenet_amd has no host path)')
            frames = frames[None] if frames.dim() == 3 else frames
            n = frames.shape[0]
            if n < 1 or n > self.max_push:
                raise ValueError(f'push: camera {c}: {n} frames, this ring takes 1 .. max_push = {self.max_push} '
                                 'per camera and push')
            if canvas is None:
                canvas = tuple(frames.shape[1:])
            elif tuple(frames.shape[1:]) != canvas:
                raise ValueError(f'push: camera {c}: canvas {tuple(frames.shape[1:])}, the first had {canvas}')
            out.append((c, frames))
        return canvas, out

    @torch.no_grad()
    def push(self, batch):
        """batch {camera: [3, Hp, Wp] or [n, 3, Hp, Wp] fp32 canvases on the device, n <= max_push}: the next frames
        of any subset of the cameras -> [(camera, frame index, (bboxes, labels, kpts))] of the centres these frames
        complete, sorted by (camera, index).  A push that fails its checks raises ValueError and changes nothing."""
        canvas, named = self._checked(batch)
        self._canvas = canvas
        frames = named[0][1] if len(named) == 1 else torch.cat([f for _, f in named], 0)
        with batch_invariant_scope(self.model):
            self.ring.plan([(c, self.n_seen[c] + j) for c, f in named for j in range(f.shape[0])])
            self.stream._encode(frames, self.ring)
            self.ring.commit()
            for c, f in named:
                self.n_seen[c] += f.shape[0]
            return self._emit({c: self.n_seen[c] - 1 - self.T // 2 for c, _ in named})

    @torch.no_grad()
    def flush(self, camera=None):
        """End of that camera's video (None: of every camera's): the centres that wait for frames that will not
        come, right edge replicated, of all of them in one batched decode."""
        cams = [c for c in (range(self.cameras) if camera is None else [self._camera(camera)]) if self.n_seen[c]]
        if not cams:
            return []
        with batch_invariant_scope(self.model):
            return self._emit({c: self.n_seen[c] - 1 for c in cams})

    def reset(self, camera=None):
        """Start that camera's (None: every camera's) next video at frame 0 in the same rows."""
        for c in range(self.cameras) if camera is None else [self._camera(camera)]:
            self.ring.reset(c)
            self.n_seen[c] = 0
            self.next_centre[c] = 0

    def _camera(self, camera):
        if isinstance(camera, bool) or not isinstance(camera, int) or not 0 <= camera < self.cameras:
            raise ValueError(f'camera {camera!r}, this ring serves cameras 0 .. {self.cameras - 1}')
        return camera
