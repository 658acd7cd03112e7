"""The track-trail rule of DESIGN section 22 in numpy and Python integers.  Who takes part, the slots, the births and the
1/8-pixel anchor are section 17's and are taken from its statement, tests/zones_ref.py (a ZoneRef without zones runs
beside the rings and owns id, last, pos, frame and dropped); the rings are restated here from the rule, not from the
kernel.  The state is kept as the arrays `TrackTrails.state()` and `points()` show, so a test compares them one for
one."""
import math

import numpy as np

from tests.smooth_ref import wrap32
from tests.zones_ref import ZoneRef


def length(a, b):
    """floor(sqrt(|a - b|^2)) in exact integers."""
    return math.isqrt((int(a[0]) - int(b[0])) ** 2 + (int(a[1]) - int(b[1])) ** 2)


def committed(pts, when, head, count):
    """One slot's ring -> its committed points, oldest first, as [(x, y, when)]; head and count reduced as the rule
    reduces them wherever they index."""
    L = pts.shape[0]
    head, count = (int(head) & 0xffffffff) % L, min(max(int(count), 1), L)
    order = [(head - count + 1 + j) % L for j in range(count)]
    return [(int(pts[i, 0]), int(pts[i, 1]), int(when[i])) for i in order]


def measures(points, pos, frame):
    """(count, span, dist, path) of a slot from its committed points, its pos and the camera's frame."""
    xy = [p[:2] for p in points] + [tuple(int(v) for v in pos)]
    return (len(points), wrap32(int(frame) - points[0][2]), length(xy[-1], xy[0]),
            sum(length(a, b) for a, b in zip(xy, xy[1:])))


class TrailRef:
    def __init__(self, K, cameras=1, max_tracks=128, max_age=30, length=32, stride=1, min_step=16, anchor='feet',
                 anchor_kpts=None, score_thr=0.3, kpt_thr=0.):
        self.z = ZoneRef(K, cameras=cameras, max_tracks=max_tracks, max_age=max_age, anchor=anchor, anchor_kpts=anchor_kpts,
                         score_thr=score_thr, kpt_thr=kpt_thr)
        self.K, self.S, self.L, self.cameras, self.max_age = K, max_tracks, length, cameras, max_age
        self.stride, self.min_step = stride, min_step
        C, S, L = cameras, max_tracks, length
        self.head = np.zeros((C, S), np.int32)
        self.count = np.zeros((C, S), np.int32)
        self.box = np.zeros((C, S, 4), np.int32)
        self.pts = np.zeros((C, S, L, 2), np.int32)
        self.when = np.zeros((C, S, L), np.int32)

    id = property(lambda self: self.z.id)
    last = property(lambda self: self.z.last)
    pos = property(lambda self: self.z.pos)
    frame = property(lambda self: self.z.frame)
    dropped = property(lambda self: self.z.dropped)

    def reset(self, camera=None):
        self.z.reset(camera)

    def state(self, c):
        return dict(id=self.id[c], last=self.last[c], pos=self.pos[c], head=self.head[c], count=self.count[c],
                    box=self.box[c], frame=self.frame[c], dropped=self.dropped[c])

    def points(self, c):
        return dict(pts=self.pts[c], when=self.when[c], head=self.head[c], count=self.count[c])

    def drawn(self, c):
        """What the draw rule reads of camera c."""
        return dict(self.state(c), **self.points(c))

    def update(self, kpts, bboxes, ids, keep=None, scale=(1.0, 1.0), camera=0):
        """kpts [N, K, 3], bboxes [N, 5] float32, ids [N], keep [N] or None -> dict(count, span, dist, path) int32 [N]."""
        c, L = camera, self.L
        kpts = np.asarray(kpts, np.float32).reshape(-1, self.K, 3)
        bboxes = np.asarray(bboxes, np.float32).reshape(-1, 5)
        ids = np.asarray(ids).reshape(-1)
        N = kpts.shape[0]
        # steps 1 and 2 and every pos: section 17.  A slot that holds the id it held before, and was not freed by step
        # 1 in this frame, was there before; every other slot seen in this frame was born in it.
        frame = wrap32(int(self.frame[c]) + 1)
        before = np.where((self.id[c] != 0) & (frame - self.last[c].astype(np.int64) > self.max_age), 0, self.id[c])
        self.z.update(kpts, bboxes, ids, keep, scale, camera)
        assert int(self.frame[c]) == frame
        # the pose of a slot seen in this frame: the first pose of its id that takes part
        usable = np.isfinite(bboxes[:, :4]).all(1) & np.isfinite(kpts[..., :2]).all((1, 2))
        with np.errstate(invalid='ignore'):
            valid = usable & (bboxes[:, 4] > self.z.score_thr)
        if keep is not None:
            valid &= np.asarray(keep).reshape(-1) != 0
        out = {name: np.zeros(N, np.int32) for name in ('count', 'span', 'dist', 'path')}
        for t in range(self.S):
            if self.id[c, t] == 0 or int(self.last[c, t]) != frame:
                continue
            a = (int(self.pos[c, t, 0]), int(self.pos[c, t, 1]))
            if before[t] != self.id[c, t]:
                # 3
                self.head[c, t], self.count[c, t] = 0, 1
                self.pts[c, t, 0], self.when[c, t, 0] = a, frame
                self.box[c, t] = a + a
            else:
                # 4
                head = int(self.head[c, t])
                q = self.pts[c, t, head]
                if frame - int(self.when[c, t, head]) >= self.stride and \
                        max(abs(a[0] - int(q[0])), abs(a[1] - int(q[1]))) >= self.min_step:
                    head = (head + 1) % L
                    self.head[c, t] = head
                    self.pts[c, t, head], self.when[c, t, head] = a, frame
                    self.count[c, t] = min(int(self.count[c, t]) + 1, L)
                xy = [p[:2] for p in committed(self.pts[c, t], self.when[c, t], self.head[c, t], self.count[c, t])] + [a]
                self.box[c, t] = [min(p[0] for p in xy), min(p[1] for p in xy), max(p[0] for p in xy),
                                  max(p[1] for p in xy)]
            # 5
            d = int(np.nonzero(valid & (ids == self.id[c, t]))[0][0])
            m = measures(committed(self.pts[c, t], self.when[c, t], self.head[c, t], self.count[c, t]), a, frame)
            for name, v in zip(('count', 'span', 'dist', 'path'), m):
                out[name][d] = v
        return out
