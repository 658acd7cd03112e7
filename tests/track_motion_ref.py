"""The constant-velocity rule of DESIGN section 14, "Motion", in numpy, on top of tests/track_ref.py: the plain rule's
steps with 3b (predict), 4' (score against the prediction, a wider test for a track without a velocity), 6' (measure
and smooth the velocity) and 7' (a birth starts at rest).  Restated from the rule, not from the kernel; python's `//`
and numpy's `>>` on int64 are floor division, which is what the rule asks for."""
import numpy as np

from tests.track_ref import TrackRef, quant

QMAX = 32767


class TrackMotionRef(TrackRef):
    def __init__(self, K, velocity_gain=8, max_predict=None, new_gate=4, **kw):
        super().__init__(K, **kw)
        self.gain, self.new_gate = velocity_gain, new_gate
        self.max_predict = min(self.max_age, 255) if max_predict is None else max_predict
        self.vel = np.zeros((self.cameras, self.M, 2), np.int32)
        self.hits = np.zeros((self.cameras, self.M), np.int32)

    def state(self, c):
        return dict(super().state(c), vel=self.vel[c], hits=self.hits[c])

    def predict(self, c, frame):
        """3b for every slot (a free slot's row means nothing) -> P [M, K, 2] int64."""
        gap = frame - self.last[c].astype(np.int64)
        g = np.minimum(gap, self.max_predict)
        shift = (self.vel[c].astype(np.int64) * g[:, None] + 8) >> 4                       # [M, 2]
        return np.clip(self.kpts[c].astype(np.int64) + shift[:, None, :], 0, QMAX)

    def update(self, kpts, bboxes, keep=None, scale=(1.0, 1.0), camera=0):
        c, K, M = camera, self.K, self.M
        kpts, bboxes = np.asarray(kpts, np.float32).reshape(-1, K, 3), np.asarray(bboxes, np.float32).reshape(-1, 5)
        N = kpts.shape[0]
        sx, sy = scale
        # 1
        self.frame[c] += 1
        frame = int(self.frame[c])
        old = (self.id[c] != 0) & (frame - self.last[c].astype(np.int64) > self.max_age)
        self.id[c][old] = 0
        # 2
        with np.errstate(invalid='ignore'):
            valid = bboxes[:, 4] > self.score_thr
        if keep is not None:
            valid &= np.asarray(keep).reshape(-1) != 0
        valid &= np.isfinite(bboxes[:, :4]).all(1) & np.isfinite(kpts[..., :2]).all((1, 2))
        # 3
        X = np.stack([quant(kpts[..., 0], sx), quant(kpts[..., 1], sy)], -1)               # [N, K, 2]
        with np.errstate(invalid='ignore'):
            seen = kpts[..., 2] > self.kpt_thr
        vis = (seen.astype(np.uint64) << np.arange(K, dtype=np.uint64)).sum(1).astype(np.uint32)
        X1, Y1, X2, Y2 = (quant(bboxes[:, i], s) for i, s in enumerate((sx, sy, sx, sy)))
        area = np.maximum(X2 - X1, 1) * np.maximum(Y2 - Y1, 1)
        live = self.id[c] != 0
        tseen = (self.vis[c][:, None] >> np.arange(K, dtype=np.uint32)) & 1 != 0           # [M, K]
        det_slot = np.full(N, -1)
        if N and live.any() and valid.any():
            # 3b, 4'
            P = self.predict(c, frame)
            G = np.where(self.hits[c] == 1, self.new_gate, 1).astype(np.int64)             # [M]
            both = seen[:, None, :] & tseen[None, :, :]                                    # [N, M, K]
            d2 = ((X[:, None, :, :] - P[None, :, :, :]) ** 2).sum(-1)
            bound = self.C[None, None, :] * G[None, :, None] * (area[:, None, None] +
                                                                self.area[c].astype(np.int64)[None, :, None])
            agree = both & ((d2 << 20) <= bound)
            s, D = agree.sum(2), np.where(both, d2, 0).sum(2)
            cand = (s >= self.min_kpts) & valid[:, None] & live[None, :]
            # 5
            dd, tt = np.nonzero(cand)
            taken = np.zeros(M, bool)
            for _, _, t, d in sorted(zip(-s[dd, tt], D[dd, tt], tt, dd)):
                if det_slot[d] < 0 and not taken[t]:
                    det_slot[d], taken[t] = t, True
        # 6': the matched pairs, from the points the slots still hold
        for d in range(N):
            t = det_slot[d]
            if t < 0:
                continue
            cov = seen[d] & tseen[t]
            n, gap = int(cov.sum()), frame - int(self.last[c, t])
            first = int(self.hits[c, t]) == 1
            for a in range(2):
                S = int((X[d, cov, a] - self.kpts[c, t, cov, a].astype(np.int64)).sum())
                m = (32 * S + n * gap) // (2 * n * gap)
                v = m if first else (self.gain * m + (16 - self.gain) * int(self.vel[c, t, a]) + 8) >> 4
                self.vel[c, t, a] = min(max(v, -32768), 32767)
            self.hits[c, t] = min(int(self.hits[c, t]) + 1, 32767)
        # 7, 7'
        for d in range(N):
            if valid[d] and det_slot[d] < 0:
                free = np.nonzero(self.id[c] == 0)[0]
                if len(free):
                    t = int(free[0])
                    self.id[c, t] = self.next_id[c]
                    self.next_id[c] += 1
                    det_slot[d] = t
                    self.vel[c, t] = 0
                    self.hits[c, t] = 1
                else:
                    self.dropped[c] += 1
        # 6
        ids = np.zeros(N, np.int32)
        for d in range(N):
            t = det_slot[d]
            if t >= 0:
                ids[d] = self.id[c, t]
                self.kpts[c, t] = X[d]
                self.vis[c, t], self.area[c, t], self.last[c, t] = vis[d], area[d], frame
        return ids
