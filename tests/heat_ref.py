"""The footfall-map rule of DESIGN section 21 in numpy and Python integers: fp32 quantisation as in tests/track_ref.py,
every other step in exact integers.  Restated from the rule, not from the kernel: the state is kept as the arrays
`FootfallMap.state()` and `maps()` show, so a test compares them one for one."""
import numpy as np

from tests.smooth_ref import wrap32
from tests.track_ref import quant

ANKLES = {17: (15, 16), 15: (13, 14), 14: (10, 11)}


class HeatRef:
    def __init__(self, K, size, cell=8, cameras=1, max_tracks=128, max_age=30, anchor='feet', anchor_kpts=None, radius=1,
                 half_life=0, score_thr=0.3, kpt_thr=0.):
        self.K, self.S, self.cameras, self.max_age = K, max_tracks, cameras, max_age
        self.width, self.height = size
        self.cell, self.shift = cell, 3 + int(cell).bit_length() - 1
        self.Gw, self.Gh = -(-self.width // cell), -(-self.height // cell)
        self.radius, self.half_life = radius, half_life
        self.anchor = anchor
        self.anchor_kpts = tuple(ANKLES.get(K, ()) if anchor_kpts is None else anchor_kpts) if anchor == 'feet' else ()
        self.score_thr, self.kpt_thr = np.float32(score_thr), np.float32(kpt_thr)
        C, S = cameras, max_tracks
        self.id = np.zeros((C, S), np.int32)
        self.last = np.zeros((C, S), np.int32)
        self.slot_cell = np.zeros((C, S), np.int32)
        self.frame = np.zeros(C, np.int32)
        self.dropped = np.zeros(C, np.int32)
        self.peak = np.zeros((C, 2), np.int32)
        self.dwell = np.zeros((C, self.Gh, self.Gw), np.int32)
        self.visits = np.zeros((C, self.Gh, self.Gw), np.int32)
        self.anchors = None            # of the last update: [N, 2] int64, rows of poses that take no part are -1

    def reset(self, camera=None):
        c = slice(None) if camera is None else camera
        for a in (self.id, self.frame, self.dropped, self.peak, self.dwell, self.visits):
            a[c] = 0

    def state(self, c):
        return dict(id=self.id[c], last=self.last[c], cell=self.slot_cell[c], frame=self.frame[c], dropped=self.dropped[c])

    def maps(self, c):
        return dict(dwell=self.dwell[c], visits=self.visits[c], peak=self.peak[c])

    def update(self, kpts, bboxes, ids, keep=None, scale=(1.0, 1.0), camera=0):
        """kpts [N, K, 3], bboxes [N, 5] float32, ids [N], keep [N] or None -> dict(cell, dwell, visits) int32 [N]."""
        c, K, S, r = camera, self.K, self.S, self.radius
        kpts, bboxes = np.asarray(kpts, np.float32).reshape(-1, K, 3), np.asarray(bboxes, np.float32).reshape(-1, 5)
        ids = np.asarray(ids).reshape(-1)
        N = kpts.shape[0]
        sx, sy = scale
        # 1
        self.frame[c] = wrap32(int(self.frame[c]) + 1)
        frame = int(self.frame[c])
        for t in range(S):
            if self.id[c, t] != 0 and frame - int(self.last[c, t]) > self.max_age:
                self.id[c, t] = 0
        # 2
        if self.half_life > 0 and frame % self.half_life == 0:
            self.dwell[c] >>= 1
            self.visits[c] >>= 1
            self.peak[c] >>= 1
        # 3: section 17's step 2
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
                slot[d] = int(have[0])
        for d in range(N):
            if cand[d] and slot[d] < 0:
                free = np.nonzero(self.id[c] == 0)[0]
                if len(free):
                    slot[d], born[d] = int(free[0]), True
                    self.id[c, slot[d]] = int(ids[d])
                else:
                    self.dropped[c] = wrap32(int(self.dropped[c]) + 1)
        # 4: the anchors, 1/8 pixel (section 17's), and the splat
        X = np.stack([quant(kpts[..., 0], sx), quant(kpts[..., 1], sy)], -1)
        B = np.stack([quant(bboxes[:, 0], sx), quant(bboxes[:, 1], sy), quant(bboxes[:, 2], sx), quant(bboxes[:, 3], sy)], 1)
        cell = np.full(N, -1, np.int32)
        self.anchors = np.full((N, 2), -1, np.int64)
        for d in range(N):
            t = int(slot[d])
            if t < 0:
                continue
            x1, y1, x2, y2 = (int(v) for v in B[d])
            P = (x1 + x2, y1 + y2) if self.anchor == 'centre' else (x1 + x2, 2 * y2)
            feet = [k for k in self.anchor_kpts if seen[d, k]]
            if self.anchor == 'feet' and feet:
                P = tuple(2 * sum(int(X[d, k, a]) for k in feet) // len(feet) for a in (0, 1))
            self.anchors[d] = P
            here = -1
            if 0 <= P[0] < 8 * self.width and 0 <= P[1] < 8 * self.height:
                gx, gy = P[0] >> self.shift, P[1] >> self.shift
                here = gy * self.Gw + gx
                for dy in range(-r, r + 1):
                    for dx in range(-r, r + 1):
                        if 0 <= gy + dy < self.Gh and 0 <= gx + dx < self.Gw:
                            self.dwell[c, gy + dy, gx + dx] = wrap32(int(self.dwell[c, gy + dy, gx + dx])
                                                                     + (r + 1 - abs(dx)) * (r + 1 - abs(dy)))
                            self.peak[c, 0] = max(self.peak[c, 0], self.dwell[c, gy + dy, gx + dx])
                if born[d] or int(self.slot_cell[c, t]) != here:
                    self.visits[c, gy, gx] = wrap32(int(self.visits[c, gy, gx]) + 1)
                    self.peak[c, 1] = max(self.peak[c, 1], self.visits[c, gy, gx])
            cell[d] = here
            self.slot_cell[c, t] = here
            self.last[c, t] = frame
        # 6: the maps after the whole frame
        on = cell >= 0
        flat_d, flat_v = self.dwell[c].reshape(-1), self.visits[c].reshape(-1)
        return dict(cell=cell, dwell=np.where(on, flat_d[np.maximum(cell, 0)], 0).astype(np.int32),
                    visits=np.where(on, flat_v[np.maximum(cell, 0)], 0).astype(np.int32))
