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
"""
import torch

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
