"""The ground-plane rule of DESIGN section 23 in numpy and Python integers: fp32 quantisation as in tests/track_ref.py,
the calibration in float64 up to the matrix and in exact integers after it, every other step in Python integers (which
cannot overflow, so an int64 that would is seen as a difference).  Restated from the rule, not from the kernel: the
state is kept as the arrays `GroundPlane.state()` and `calibration()` show, so a test compares them one for one."""
import math
from fractions import Fraction

import numpy as np

from tests.smooth_ref import wrap32
from tests.track_ref import quant

ANKLES = {17: (15, 16), 15: (13, 14), 14: (10, 11)}
MAX_MM = (1 << 20) - 1
OUTPUTS = ('on', 'xy', 'vel', 'speed', 'travel', 'nearest', 'gap', 'near')
STATE = ('id', 'last', 'hits', 'pos', 'vel', 'travel', 'frame', 'dropped')


def dlt(pairs):
    """Step 2's direct linear transform: Hartley's normalisation of both point sets, numpy.linalg.svd, float64."""
    src = np.asarray([p[0] for p in pairs], np.float64)
    dst = np.asarray([p[1] for p in pairs], np.float64)
    norm = []
    for pts in (src, dst):
        centre = pts.mean(0)
        s = math.sqrt(2.0) / np.sqrt(((pts - centre) ** 2).sum(1)).mean()
        norm.append(np.asarray([[s, 0.0, -s * centre[0]], [0.0, s, -s * centre[1]], [0.0, 0.0, 1.0]]))
    a, b = (src - src.mean(0)) * norm[0][0, 0], (dst - dst.mean(0)) * norm[1][0, 0]
    rows = []
    for (x, y), (u, v) in zip(a, b):
        rows.append([-x, -y, -1.0, 0.0, 0.0, 0.0, u * x, u * y, u])
        rows.append([0.0, 0.0, 0.0, -x, -y, -1.0, v * x, v * y, v])
    h = np.linalg.svd(np.asarray(rows, np.float64))[2][-1].reshape(3, 3)
    H = np.linalg.inv(norm[1]) @ h @ norm[0]
    at = src.mean(0)
    return -H if H[2, 0] * at[0] + H[2, 1] * at[1] + H[2, 2] < 0 else H


def row_ok(words):
    return all((abs(words[3 * r]) + abs(words[3 * r + 1])) * 65535 + abs(words[3 * r + 2]) < 1 << 61 for r in range(3))


def quantise(H):
    """The nine integers of a signed float64 matrix, in exact rationals: G = H diag(1/8, 1/8, 1) times the largest
    power of two that keeps every row's (|g0| + |g1|) 65535 + |g2| below 2^61 after rounding to nearest (even)."""
    g = [Fraction(float(v)) / (8 if i % 3 < 2 else 1) for i, v in enumerate(np.asarray(H, np.float64).reshape(-1))]
    k = 1200
    while True:
        words = [round(v * Fraction(2) ** k) for v in g]
        if row_ok(words):
            assert not row_ok([round(v * Fraction(2) ** (k + 1)) for v in g])
            return words
        k -= 1


def project(G, bounds, ax, ay):
    """Step 3 -> (X, Y) in mm, or None off the floor."""
    G = [int(v) for v in G]
    nx, ny, w = (G[3 * r] * ax + G[3 * r + 1] * ay + G[3 * r + 2] for r in range(3))
    assert all(abs(v) < 1 << 61 for v in (nx, ny, w)) and abs(2 * nx + w) < 1 << 63 and abs(2 * ny + w) < 1 << 63
    if w <= 0:
        return None
    X, Y = (2 * nx + w) // (2 * w), (2 * ny + w) // (2 * w)          # (Python's // is the floor)
    x0, y0, x1, y1 = (int(v) for v in bounds)
    return (X, Y) if x0 <= X <= x1 and y0 <= Y <= y1 else None


class FloorRef:
    def __init__(self, K, cameras=1, max_tracks=128, max_age=30, anchor='feet', anchor_kpts=None, velocity_gain=4,
                 near=1500, unit=10, origin=(0, 0), score_thr=0.3, kpt_thr=0.):
        self.K, self.S, self.cameras, self.max_age = K, max_tracks, cameras, max_age
        self.anchor = anchor
        self.anchor_kpts = tuple(ANKLES.get(K, ()) if anchor_kpts is None else anchor_kpts) if anchor == 'feet' else ()
        self.gain, self.near, self.unit, self.origin = velocity_gain, near, unit, origin
        self.score_thr, self.kpt_thr = np.float32(score_thr), np.float32(kpt_thr)
        C, S = cameras, max_tracks
        self.id = np.zeros((C, S), np.int32)
        self.last = np.zeros((C, S), np.int32)
        self.hits = np.zeros((C, S), np.int32)
        self.pos = np.zeros((C, S, 2), np.int32)
        self.vel = np.zeros((C, S, 2), np.int32)
        self.travel = np.zeros((C, S), np.int32)
        self.frame = np.zeros(C, np.int32)
        self.dropped = np.zeros(C, np.int32)
        self.G = np.zeros((C, 3, 3), np.int64)
        self.bounds = np.zeros((C, 4), np.int64)
        self.valid = np.zeros(C, np.int64)
        self.H = [None] * C

    def set_plane(self, camera, points=None, matrix=None, bounds=None):
        H = dlt(list(points)) if points is not None else np.asarray(matrix, np.float64)
        self.H[camera] = H
        self.G[camera] = np.asarray(quantise(H), np.int64).reshape(3, 3)
        self.bounds[camera] = (-MAX_MM, -MAX_MM, MAX_MM, MAX_MM) if bounds is None else bounds
        self.valid[camera] = 1
        self.reset(camera)

    def reset(self, camera=None):
        c = slice(None) if camera is None else camera
        for a in (self.id, self.frame, self.dropped):
            a[c] = 0

    def state(self, c):
        return {n: getattr(self, n)[c] for n in STATE}

    def calibration(self, c):
        return dict(G=self.G[c], bounds=self.bounds[c], valid=self.valid[c])

    def anchors(self, kpts, bboxes, scale):
        """Step 1: section 17's anchor of every pose, 1/8 pixel -> [(ax, ay)]."""
        sx, sy = scale
        with np.errstate(invalid='ignore'):
            seen = kpts[..., 2] > self.kpt_thr
        X = np.stack([quant(kpts[..., 0], sx), quant(kpts[..., 1], sy)], -1)
        B = np.stack([quant(bboxes[:, 0], sx), quant(bboxes[:, 1], sy), quant(bboxes[:, 2], sx), quant(bboxes[:, 3], sy)], 1)
        out = []
        for d in range(len(bboxes)):
            x1, y1, x2, y2 = (int(v) for v in B[d])
            P = (x1 + x2, y1 + y2) if self.anchor == 'centre' else (x1 + x2, 2 * y2)
            feet = [k for k in self.anchor_kpts if seen[d, k]]
            if self.anchor == 'feet' and feet:
                P = tuple(2 * sum(int(X[d, k, a]) for k in feet) // len(feet) for a in (0, 1))
            out.append(P)
        return out

    def update(self, kpts, bboxes, ids, keep=None, scale=(1.0, 1.0), camera=0):
        """kpts [N, K, 3], bboxes [N, 5] float32, ids [N], keep [N] or None -> dict of int32 on, speed, travel, nearest,
        gap, near [N], xy, vel [N, 2] and float32 kpts [N, K, 3], bboxes [N, 5] (the floor-unit result)."""
        c, K, S = camera, self.K, self.S
        kpts, bboxes = np.asarray(kpts, np.float32).reshape(-1, K, 3), np.asarray(bboxes, np.float32).reshape(-1, 5)
        ids = np.asarray(ids).reshape(-1)
        N = kpts.shape[0]
        # 4: the clock and the expiry
        self.frame[c] = wrap32(int(self.frame[c]) + 1)
        frame = int(self.frame[c])
        for t in range(S):
            if self.id[c, t] != 0 and frame - int(self.last[c, t]) > self.max_age:
                self.id[c, t] = 0
        # 1, 3, 4: who is placed, and where
        usable = np.isfinite(bboxes[:, :4]).all(1) & np.isfinite(kpts[..., :2]).all((1, 2))
        with np.errstate(invalid='ignore'):
            valid = usable & (bboxes[:, 4] > self.score_thr)
        if keep is not None:
            valid &= np.asarray(keep).reshape(-1) != 0
        anchors = self.anchors(kpts, bboxes, scale)
        where = [project(self.G[c].reshape(-1), self.bounds[c], *anchors[d]) if valid[d] and self.valid[c] else None
                 for d in range(N)]
        placed = [w is not None for w in where]
        # 4: who is followed
        slot, born, taken = [-1] * N, [False] * N, set()
        for d in range(N):
            ident = int(ids[d])
            if not placed[d] or ident < 1 or ident in taken:
                continue
            taken.add(ident)
            have = np.nonzero(self.id[c] == ident)[0]
            slot[d] = int(have[0]) if len(have) else -2
        for d in range(N):
            if slot[d] == -2:
                free = np.nonzero(self.id[c] == 0)[0]
                if len(free):
                    slot[d], born[d] = int(free[0]), True
                    self.id[c, slot[d]] = int(ids[d])
                else:
                    slot[d] = -1
                    self.dropped[c] = wrap32(int(self.dropped[c]) + 1)
        out = dict(on=np.zeros(N, np.int32), xy=np.zeros((N, 2), np.int32), vel=np.zeros((N, 2), np.int32),
                   speed=np.zeros(N, np.int32), travel=np.zeros(N, np.int32), nearest=np.full(N, -1, np.int32),
                   gap=np.full(N, -1, np.int32), near=np.zeros(N, np.int32))
        # 5
        for d in range(N):
            if not placed[d]:
                continue
            out['on'][d], out['xy'][d] = 1, where[d]
            t = slot[d]
            if t < 0:
                continue
            X, Y = where[d]
            if born[d]:
                vel, travel, hits = (0, 0), 0, 1
            else:
                dt = max(frame - int(self.last[c, t]), 1)
                dx, dy = X - int(self.pos[c, t, 0]), Y - int(self.pos[c, t, 1])
                m = ((256 * dx) // dt, (256 * dy) // dt)
                hits, old = int(self.hits[c, t]), [int(v) for v in self.vel[c, t]]
                vel = m if hits == 1 else tuple(old[a] + (self.gain * (m[a] - old[a])) // 16 for a in (0, 1))
                travel = min((1 << 31) - 1, int(self.travel[c, t]) + math.isqrt(dx * dx + dy * dy))
                hits = min(hits + 1, 1 << 30)
            assert all(abs(v) < 1 << 31 for v in vel)
            self.pos[c, t], self.vel[c, t], self.travel[c, t], self.hits[c, t], self.last[c, t] = (X, Y), vel, travel, hits, frame
            out['vel'][d], out['travel'][d] = vel, travel
            out['speed'][d] = math.isqrt(vel[0] ** 2 + vel[1] ** 2)
        # 6
        for i in range(N):
            if not placed[i]:
                continue
            d2 = [(where[i][0] - where[j][0]) ** 2 + (where[i][1] - where[j][1]) ** 2 if placed[j] and j != i else None
                  for j in range(N)]
            others = [j for j in range(N) if d2[j] is not None]
            if others:
                j = min(others, key=lambda j: (d2[j], j))
                out['nearest'][i], out['gap'][i] = j, math.isqrt(d2[j])
                out['near'][i] = sum(d2[j] <= self.near ** 2 for j in others)
        # 7
        fk, fb = kpts.copy(), bboxes.copy()
        fk[..., :2], fb[:, :4] = np.float32(np.nan), np.float32(np.nan)
        for d in range(N):
            if placed[d]:
                P = tuple((4 * (where[d][a] - self.origin[a])) // self.unit for a in (0, 1))
                if all(0 <= v <= 32767 for v in P):
                    fk[d, :, 0], fk[d, :, 1] = np.float32(P[0] / 4), np.float32(P[1] / 4)
                    fb[d, :4] = np.float32([P[0] / 4, P[1] / 4, P[0] / 4, P[1] / 4])
        out['kpts'], out['bboxes'] = fk, fb
        return out


def plan_points(out, unit, origin):
    """The (Px, Py) of step 7 per pose from an update's xy and on, or None: for the tests of the bridge."""
    pts = []
    for d in range(len(out['on'])):
        P = tuple((4 * (int(out['xy'][d, a]) - origin[a])) // unit for a in (0, 1))
        pts.append(P if out['on'][d] and all(0 <= v <= 32767 for v in P) else None)
    return pts
