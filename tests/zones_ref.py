"""The zone and line rule of DESIGN section 17 in numpy and Python integers: fp32 quantisation as in
tests/track_ref.py, every other step in exact integers.  Restated from the rule, not from the kernel: the state is
kept as the arrays `ZoneMonitor.state()`, `counts()` and `geometry()` show, so a test compares them one for one."""
import numpy as np

from tests.smooth_ref import wrap32
from tests.track_ref import quant

ENTER, EXIT, DWELL, APPEAR, VANISH, CROSS_FWD, CROSS_BACK = 1, 2, 3, 4, 5, 6, 7
Z, L, V = 8, 8, 16                                     # zones, lines, vertices of a zone at the most
ANKLES = {17: (15, 16), 15: (13, 14), 14: (10, 11)}
COUNTERS = ('occupancy', 'entered', 'exited', 'appeared', 'vanished')


def quantise(p):
    """A vertex in pixels -> 1/8 pixel: clamp(rint(8 x), 0, 65535) in double."""
    return [int(np.clip(np.rint(8.0 * float(v)), 0, 65535)) for v in p]


def inside(P, polygon):
    """Even-odd, half-open, in integers."""
    hit = False
    for i in range(len(polygon)):
        a, b = polygon[i], polygon[(i + 1) % len(polygon)]
        if (a[1] > P[1]) != (b[1] > P[1]):
            dy = b[1] - a[1]
            t = (P[0] - a[0]) * dy - (P[1] - a[1]) * (b[0] - a[0])
            if (t < 0) if dy > 0 else (t > 0):
                hit = not hit
    return hit


def side(A, B, P):
    """s(P) on A -> B: cross(B - A, P - A) >= 0."""
    return (B[0] - A[0]) * (P[1] - A[1]) - (B[1] - A[1]) * (P[0] - A[0]) >= 0


def crossing(Q, P, A, B):
    """0: the move Q -> P does not cross A -> B; CROSS_FWD or CROSS_BACK."""
    if Q == P or side(A, B, Q) == side(A, B, P) or side(Q, P, A) == side(Q, P, B):
        return 0
    return CROSS_BACK if side(A, B, Q) else CROSS_FWD


class ZoneRef:
    def __init__(self, K, cameras=1, max_tracks=128, max_age=30, anchor='feet', anchor_kpts=None, min_frames=2,
                 max_events=256, score_thr=0.3, kpt_thr=0.):
        self.K, self.S, self.cameras, self.max_age = K, max_tracks, cameras, max_age
        self.anchor = anchor
        self.anchor_kpts = tuple(ANKLES.get(K, ()) if anchor_kpts is None else anchor_kpts) if anchor == 'feet' else ()
        self.min_frames, self.max_events = min_frames, max_events
        self.score_thr, self.kpt_thr = np.float32(score_thr), np.float32(kpt_thr)
        C, S = cameras, max_tracks
        self.id = np.zeros((C, S), np.int32)
        self.last = np.zeros((C, S), np.int32)
        self.pos = np.zeros((C, S, 2), np.int32)
        self.inside = np.zeros((C, S), np.int32)
        self.alerted = np.zeros((C, S), np.int32)
        self.streak = np.zeros((C, S, Z), np.int32)
        self.since = np.zeros((C, S, Z), np.int32)
        self.frame = np.zeros(C, np.int32)
        self.dropped = np.zeros(C, np.int32)
        for name in COUNTERS:
            setattr(self, name, np.zeros((C, Z), np.int32))
        self.crossed = np.zeros((C, L, 2), np.int32)
        self.n_zones, self.n_lines = np.zeros(C, np.int32), np.zeros(C, np.int32)
        self.n_vertices, self.dwell_frames = np.zeros((C, Z), np.int32), np.zeros((C, Z), np.int32)
        self.zones, self.lines = np.zeros((C, Z, V, 2), np.int32), np.zeros((C, L, 2, 2), np.int32)

    def set_zones(self, camera, zones=(), lines=(), dwell_frames=None):
        c = camera
        for a in (self.n_vertices, self.dwell_frames, self.zones, self.lines):
            a[c] = 0
        self.n_zones[c], self.n_lines[c] = len(zones), len(lines)
        for z, polygon in enumerate(zones):
            self.n_vertices[c, z] = len(polygon)
            self.dwell_frames[c, z] = 0 if dwell_frames is None else dwell_frames[z]
            self.zones[c, z, :len(polygon)] = [quantise(p) for p in polygon]
        for l, (a, b) in enumerate(lines):
            self.lines[c, l] = [quantise(a), quantise(b)]
        self.reset(c)

    def reset(self, camera=None):
        c = slice(None) if camera is None else camera
        for a in (self.id, self.frame, self.dropped, self.crossed) + tuple(getattr(self, n) for n in COUNTERS):
            a[c] = 0

    def state(self, c):
        return {n: getattr(self, n)[c] for n in ('id', 'last', 'pos', 'inside', 'alerted', 'streak', 'since', 'frame',
                                                 'dropped')}

    def counts(self, c):
        return {n: getattr(self, n)[c] for n in COUNTERS + ('crossed',)}

    def geometry(self, c):
        return {n: getattr(self, n)[c] for n in ('n_zones', 'n_lines', 'n_vertices', 'dwell_frames', 'zones', 'lines')}

    def _bump(self, array, c, i, by=1):
        array[c][i] = wrap32(int(array[c][i]) + by)

    def update(self, kpts, bboxes, ids, keep=None, scale=(1.0, 1.0), camera=0):
        """kpts [N, K, 3], bboxes [N, 5] float32, ids [N], keep [N] or None -> dict(zones [N], dwell [N, 8], events
        [max_events, 5], n_events) int32."""
        c, K, S = camera, self.K, self.S
        kpts, bboxes = np.asarray(kpts, np.float32).reshape(-1, K, 3), np.asarray(bboxes, np.float32).reshape(-1, 5)
        ids = np.asarray(ids).reshape(-1)
        N = kpts.shape[0]
        sx, sy = scale
        nz, nl = int(self.n_zones[c]), int(self.n_lines[c])
        polygons = [[tuple(int(v) for v in p) for p in self.zones[c, z, :self.n_vertices[c, z]]] for z in range(nz)]
        lines = [tuple(tuple(int(v) for v in p) for p in self.lines[c, l]) for l in range(nl)]
        events = []
        # 1
        self.frame[c] = wrap32(int(self.frame[c]) + 1)
        frame = int(self.frame[c])
        for t in range(S):
            if self.id[c, t] != 0 and frame - int(self.last[c, t]) > self.max_age:
                for z in range(nz):
                    if (int(self.inside[c, t]) >> z) & 1:
                        events.append((VANISH, z, int(self.id[c, t]), -1, frame))
                        self._bump(self.vanished, c, z)
                        self._bump(self.occupancy, c, z, -1)
                self.id[c, t] = 0
        # 2: section 16's steps 2 and 3
        usable = np.isfinite(bboxes[:, :4]).all(1) & np.isfinite(kpts[..., :2]).all((1, 2))
        with np.errstate(invalid='ignore'):
            valid = usable & (bboxes[:, 4] > self.score_thr)
            seen = kpts[..., 2] > self.kpt_thr
        if keep is not None:
            valid &= np.asarray(keep).reshape(-1) != 0
        slot, born = np.full(N, -1), np.zeros(N, bool)
        cand = np.zeros(N, bool)
        named = np.nonzero(valid & (ids >= 1))[0]
        cand[named[np.unique(ids[named], return_index=True)[1]]] = True      # the first valid pose of every id
        for d in range(N):
            have = np.nonzero(self.id[c] == int(ids[d]))[0] if cand[d] else []
            if len(have):
                slot[d] = int(have[0])     # (the rule's own states hold an id once)
        for d in range(N):
            if cand[d] and slot[d] < 0:
                free = np.nonzero(self.id[c] == 0)[0]
                if len(free):
                    slot[d], born[d] = int(free[0]), True
                    self.id[c, slot[d]] = int(ids[d])
                else:
                    self.dropped[c] = wrap32(int(self.dropped[c]) + 1)
        # the anchors, 1/8 pixel
        X = np.stack([quant(kpts[..., 0], sx), quant(kpts[..., 1], sy)], -1)                       # [N, K, 2]
        B = np.stack([quant(bboxes[:, 0], sx), quant(bboxes[:, 1], sy), quant(bboxes[:, 2], sx), quant(bboxes[:, 3], sy)], 1)
        out_zones, out_dwell = np.zeros(N, np.int32), np.zeros((N, Z), np.int32)
        for d in range(N):
            t = int(slot[d])
            if t < 0:
                continue
            x1, y1, x2, y2 = (int(v) for v in B[d])
            P = (x1 + x2, y1 + y2) if self.anchor == 'centre' else (x1 + x2, 2 * y2)
            feet = [k for k in self.anchor_kpts if seen[d, k]]
            if self.anchor == 'feet' and feet:
                P = tuple(2 * sum(int(X[d, k, a]) for k in feet) // len(feet) for a in (0, 1))
            raw = [inside(P, polygons[z]) for z in range(nz)]
            ident = int(ids[d])
            if born[d]:
                # 3
                self.inside[c, t] = sum(1 << z for z in range(nz) if raw[z])
                self.alerted[c, t] = 0
                self.streak[c, t] = 0
                self.since[c, t] = frame
                for z in range(nz):
                    if raw[z]:
                        events.append((APPEAR, z, ident, d, frame))
                        self._bump(self.appeared, c, z)
                        self._bump(self.occupancy, c, z)
            else:
                # 4
                for z in range(nz):
                    bit = 1 << z
                    if raw[z] == bool(int(self.inside[c, t]) & bit):
                        self.streak[c, t, z] = 0
                    else:
                        self.streak[c, t, z] = wrap32(int(self.streak[c, t, z]) + 1)
                        if self.streak[c, t, z] >= self.min_frames:
                            self.streak[c, t, z] = 0
                            self.inside[c, t] ^= bit
                            if int(self.inside[c, t]) & bit:
                                self.since[c, t, z] = frame
                                events.append((ENTER, z, ident, d, frame))
                                self._bump(self.entered, c, z)
                                self._bump(self.occupancy, c, z)
                            else:
                                self.alerted[c, t] &= ~bit
                                events.append((EXIT, z, ident, d, frame))
                                self._bump(self.exited, c, z)
                                self._bump(self.occupancy, c, z, -1)
                    wait = int(self.dwell_frames[c, z])
                    if int(self.inside[c, t]) & bit and wait > 0 and frame - int(self.since[c, t, z]) >= wait \
                            and not int(self.alerted[c, t]) & bit:
                        self.alerted[c, t] |= bit
                        events.append((DWELL, z, ident, d, frame))
                # 5
                Q = (int(self.pos[c, t, 0]), int(self.pos[c, t, 1]))
                for l, (A, Bend) in enumerate(lines):
                    kind = crossing(Q, P, A, Bend)
                    if kind:
                        events.append((kind, l, ident, d, frame))
                        self._bump(self.crossed, c, (l, 0 if kind == CROSS_FWD else 1))
            self.pos[c, t] = P
            self.last[c, t] = frame
            # 6
            out_zones[d] = self.inside[c, t]
            for z in range(nz):
                if (int(self.inside[c, t]) >> z) & 1:
                    out_dwell[d, z] = wrap32(frame - int(self.since[c, t, z]))
        table = np.zeros((self.max_events, 5), np.int32)
        stored = events[:self.max_events]
        if stored:
            table[:len(stored)] = np.asarray(stored, np.int64).astype(np.int32)
        return dict(zones=out_zones, dwell=out_dwell, events=table, n_events=np.asarray(len(events), np.int32))
