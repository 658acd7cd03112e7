"""The smoothing rule of DESIGN section 16 in numpy: fp32 quantisation as in tests/track_ref.py, every other step in
int64 (which the rule never overflows on int32 state).  Restated from the rule, not from the kernel: the state is
kept as the arrays `PoseSmoother.state()` shows, so a test compares them one for one."""
import numpy as np

from tests.track_ref import quant

PMAX = 16 * 32767            # the largest state position, 1/64 pixel
NAN_BITS = 0x7fc00000        # every coordinate of an unusable pose


def wrap32(v):
    """What an int32 store keeps of an integer."""
    return ((int(v) + (1 << 31)) & 0xffffffff) - (1 << 31)


class SmoothRef:
    def __init__(self, K, cameras=1, max_tracks=128, max_age=30, alpha_min=32, beta=128, velocity_gain=3,
                 score_thr=0.3, kpt_thr=0.):
        self.K, self.J, self.S, self.cameras, self.max_age = K, K + 2, max_tracks, cameras, max_age
        self.alpha_min, self.beta, self.g = alpha_min, beta, velocity_gain
        self.score_thr, self.kpt_thr = np.float32(score_thr), np.float32(kpt_thr)
        S, J = self.S, self.J
        self.id = np.zeros((cameras, S), np.int32)
        self.last = np.zeros((cameras, S), np.int32)
        self.pos = np.zeros((cameras, S, J, 2), np.int32)
        self.vel = np.zeros((cameras, S, J, 2), np.int32)
        self.frame = np.zeros(cameras, np.int32)
        self.dropped = np.zeros(cameras, np.int32)

    def reset(self, camera=None):
        c = slice(None) if camera is None else camera
        self.id[c] = 0
        self.frame[c] = 0
        self.dropped[c] = 0

    def state(self, c):
        return dict(id=self.id[c], last=self.last[c], pos=self.pos[c], vel=self.vel[c], frame=self.frame[c],
                    dropped=self.dropped[c])

    def smooth(self, kpts, bboxes, ids, keep=None, scale=(1.0, 1.0), camera=0):
        """kpts [N, K, 3], bboxes [N, 5] float32, ids [N], keep [N] or None -> (out_kpts, out_bboxes) float32."""
        c, K, J, S = camera, self.K, self.J, self.S
        kpts, bboxes = np.asarray(kpts, np.float32).reshape(-1, K, 3), np.asarray(bboxes, np.float32).reshape(-1, 5)
        ids = np.asarray(ids).reshape(-1)
        N = kpts.shape[0]
        sx, sy = scale
        # 1
        self.frame[c] = wrap32(int(self.frame[c]) + 1)
        frame = int(self.frame[c])
        self.id[c][(self.id[c] != 0) & (frame - self.last[c].astype(np.int64) > self.max_age)] = 0
        # 2
        usable = np.isfinite(bboxes[:, :4]).all(1) & np.isfinite(kpts[..., :2]).all((1, 2))
        with np.errstate(invalid='ignore'):
            valid = usable & (bboxes[:, 4] > self.score_thr)
            seen = np.concatenate([kpts[..., 2] > self.kpt_thr, np.ones((N, 2), bool)], 1)       # [N, J]
        if keep is not None:
            valid &= np.asarray(keep).reshape(-1) != 0
        # the J points of a pose: its key points, then its box corners; Z = 16 X
        px = np.concatenate([kpts[..., 0], bboxes[:, [0, 2]]], 1)
        py = np.concatenate([kpts[..., 1], bboxes[:, [1, 3]]], 1)
        Z = np.stack([16 * quant(px, sx), 16 * quant(py, sy)], -1)                               # [N, J, 2] int64
        # 3
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
        # 4, 5: the filtered poses at once, [F, J, 2] in int64 (// is floor and >> arithmetic there)
        Q = Z.copy()
        sel = np.nonzero(slot >= 0)[0]
        if len(sel):
            t, z, vis = slot[sel], Z[sel], seen[sel]
            pos, vel = self.pos[c, t].astype(np.int64), self.vel[c, t].astype(np.int64)
            gap = np.maximum(frame - self.last[c, t].astype(np.int64), 1)[:, None, None]   # (>= 1 on the rule's own states)
            box = z[:, K:] // 16                                                           # the quantised corners
            s = np.maximum(np.abs(box[:, 1] - box[:, 0]).max(1), 1)[:, None]
            start = vis & (born[sel][:, None] | (pos[..., 0] < 0))                         # takes the detection
            run = (vis & ~start)[..., None]
            e = z - pos
            r = (2 * e + gap) // (2 * gap)
            v = (self.g * r + (16 - self.g) * vel + 8) >> 4
            u = (np.abs(v).sum(2) << 6) // s
            alpha = np.minimum(256, self.alpha_min + ((self.beta * u) >> 4))[..., None]
            p = np.clip(pos + ((alpha * e + 128) >> 8), 0, PMAX)
            pos = np.where(run, p, np.where(start[..., None], z, pos))
            pos[..., 0] = np.where(vis, pos[..., 0], -1)
            vel = np.where(run, v, np.where(start[..., None], 0, vel))
            self.pos[c, t], self.vel[c, t] = pos.astype(np.int32), vel.astype(np.int32)    # (an int32 store wraps)
            self.last[c, t] = frame
            Q[sel] = np.where(run, p, z)
        # 6
        out = (Q.astype(np.float32) / np.float32(64)).astype(np.float32)
        out[~usable] = np.asarray([NAN_BITS], np.uint32).view(np.float32)[0]
        out_kpts, out_bboxes = kpts.copy(), bboxes.copy()
        out_kpts[..., :2] = out[:, :K]
        out_bboxes[:, :4] = out[:, K:].reshape(N, 4)
        return out_kpts, out_bboxes
