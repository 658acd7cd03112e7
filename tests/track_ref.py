"""The linking rule of DESIGN section 14 in numpy: fp32 quantisation, int64 scores, a sorted greedy assignment.
Restated from the rule, not from the kernel: the state is kept as the arrays `PoseTracker.state()` shows, so a test
compares them one for one."""
import math

import numpy as np

QMAX = 32767
COCO_SIGMAS = [.026, .025, .025, .035, .035, .079, .079, .072, .072, .062, .062, .107, .107, .087, .087, .089, .089]
POSETRACK_SIGMAS = [.026, .079, .079, .079, .079, .072, .072, .062, .062, .107, .107, .087, .087, .089, .089]
CROWDPOSE_SIGMAS = [.079, .079, .072, .072, .062, .062, .107, .107, .087, .087, .089, .089, .079, .079]
SIGMAS = {17: COCO_SIGMAS, 15: POSETRACK_SIGMAS, 14: CROWDPOSE_SIGMAS}


def pair_constants(sigmas, match_thr=0.5):
    """C[k] = max(1, rint(ln(1 / match_thr) (2 sigma_k)^2 2^20)), in double."""
    return [max(1, int(np.rint(math.log(1.0 / match_thr) * (2.0 * float(s)) ** 2 * 2.0 ** 20))) for s in sigmas]


def default_min_kpts(K):
    return max(1, (K + 2) // 3)


def quant(x, s):
    """clamp((int)rintf((x / s) * 4.f), 0, 32767) in fp32; a NaN becomes 0."""
    with np.errstate(all='ignore'):
        v = np.rint((np.asarray(x, np.float32) / np.float32(s)) * np.float32(4))
        v = np.where(np.isnan(v), np.float32(0), v)
        return np.clip(v, 0, QMAX).astype(np.int64)


class TrackRef:
    def __init__(self, K, cameras=1, max_tracks=128, max_age=30, match_thr=0.5, min_kpts=None, score_thr=0.3,
                 kpt_thr=0., sigmas=None):
        self.K, self.M, self.cameras, self.max_age = K, max_tracks, cameras, max_age
        self.C = np.asarray(pair_constants(SIGMAS[K] if sigmas is None else sigmas, match_thr), np.int64)
        self.min_kpts = default_min_kpts(K) if min_kpts is None else min_kpts
        self.score_thr, self.kpt_thr = np.float32(score_thr), np.float32(kpt_thr)
        M = max_tracks
        self.id = np.zeros((cameras, M), np.int32)
        self.last = np.zeros((cameras, M), np.int32)
        self.kpts = np.zeros((cameras, M, K, 2), np.int32)
        self.vis = np.zeros((cameras, M), np.uint32)
        self.area = np.zeros((cameras, M), np.int32)
        self.frame = np.zeros(cameras, np.int32)
        self.next_id = np.ones(cameras, np.int32)
        self.dropped = np.zeros(cameras, np.int32)

    def reset(self, camera=None):
        c = slice(None) if camera is None else camera
        self.id[c] = 0
        self.frame[c] = 0
        self.next_id[c] = 1
        self.dropped[c] = 0

    def state(self, c):
        """The arrays of PoseTracker.state(c) (vis as the int32 the device tensor holds)."""
        return dict(id=self.id[c], last=self.last[c], kpts=self.kpts[c], vis=self.vis[c].view(np.int32),
                    area=self.area[c], frame=self.frame[c], next_id=self.next_id[c], dropped=self.dropped[c])

    def update(self, kpts, bboxes, keep=None, scale=(1.0, 1.0), camera=0):
        """kpts [N, K, 3], bboxes [N, 5] float32, keep [N] or None -> ids [N] int32."""
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
        X, Y = quant(kpts[..., 0], sx), quant(kpts[..., 1], sy)
        with np.errstate(invalid='ignore'):
            seen = kpts[..., 2] > self.kpt_thr
        vis = (seen.astype(np.uint64) << np.arange(K, dtype=np.uint64)).sum(1).astype(np.uint32)
        X1, Y1, X2, Y2 = (quant(bboxes[:, i], s) for i, s in enumerate((sx, sy, sx, sy)))
        area = np.maximum(X2 - X1, 1) * np.maximum(Y2 - Y1, 1)
        # 4
        live = self.id[c] != 0
        ids = np.zeros(N, np.int32)
        det_slot = np.full(N, -1)
        if N and live.any() and valid.any():
            tk = self.kpts[c].astype(np.int64)
            tseen = (self.vis[c][:, None] >> np.arange(K, dtype=np.uint32)) & 1 != 0
            both = seen[:, None, :] & tseen[None, :, :]                                     # [N, M, K]
            d2 = (X[:, None, :] - tk[None, :, :, 0]) ** 2 + (Y[:, None, :] - tk[None, :, :, 1]) ** 2
            agree = both & ((d2 << 20) <= self.C[None, None, :] * (area[:, None, None] + self.area[c].astype(np.int64)[None, :, None]))
            s, D = agree.sum(2), np.where(both, d2, 0).sum(2)
            cand = (s >= self.min_kpts) & valid[:, None] & live[None, :]
            # 5
            dd, tt = np.nonzero(cand)
            order = sorted(zip(-s[dd, tt], D[dd, tt], tt, dd))
            taken = np.zeros(M, bool)
            for _, _, t, d in order:
                if det_slot[d] < 0 and not taken[t]:
                    det_slot[d], taken[t] = t, True
        # 7 (the slots of step 6 are not free: their ids are not 0)
        for d in range(N):
            if valid[d] and det_slot[d] < 0:
                free = np.nonzero((self.id[c] == 0))[0]
                if len(free):
                    t = int(free[0])
                    self.id[c, t] = self.next_id[c]
                    self.next_id[c] += 1
                    det_slot[d] = t
                else:
                    self.dropped[c] += 1
        # 6
        for d in range(N):
            t = det_slot[d]
            if t >= 0:
                ids[d] = self.id[c, t]
                self.kpts[c, t, :, 0], self.kpts[c, t, :, 1] = X[d], Y[d]
                self.vis[c, t], self.area[c, t], self.last[c, t] = vis[d], area[d], frame
        return ids
