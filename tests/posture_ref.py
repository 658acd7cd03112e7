"""The posture rule of DESIGN section 20 in numpy and Python integers: fp32 quantisation as in tests/track_ref.py,
every other step in exact integers.  Restated from the rule, not from the kernel: the state is kept as the arrays
`PostureMonitor.state()` and `counts()` show, so a test compares them one for one."""
import numpy as np

from tests.smooth_ref import wrap32
from tests.track_ref import quant

UNKNOWN, UPRIGHT, LOW, LEANING, LYING = 0, 1, 2, 3, 4
POSTURE, FALL, DOWN, HANDS_UP, HANDS_DOWN = 1, 2, 3, 4, 5
PART_NAMES = ('shoulders', 'hips', 'ankles', 'wrists')
PARTS = {17: dict(shoulders=(5, 6), hips=(11, 12), ankles=(15, 16), wrists=(9, 10)),
         15: dict(shoulders=(3, 4), hips=(9, 10), ankles=(13, 14), wrists=(7, 8)),
         14: dict(shoulders=(0, 1), hips=(6, 7), ankles=(10, 11), wrists=(4, 5))}
SLOTS = ('id', 'last', 'posture', 'since', 'upright', 'streak', 'alerted', 'hands', 'hand_streak')
STATE = SLOTS + ('frame', 'dropped')
COUNTERS = ('now', 'hands_up', 'falls', 'downs')


def centre(X, seen):
    """X [k, 2] quarter pixels, seen [k] -> floor(2 sum X / n) per axis over the n visible points in 1/8 pixel, or
    None when there is none."""
    pts = [(int(x), int(y)) for (x, y), s in zip(X, seen) if s]
    if not pts:
        return None
    return tuple(2 * sum(p[a] for p in pts) // len(pts) for a in (0, 1))


def classify(shoulders, hips, ankles, lean=11, flat=11, squat=18):
    """The raw class from the centres (1/8 pixel, or None) in Python integers, which do not overflow."""
    if shoulders is None or hips is None:
        return UNKNOWN
    dx, dy = hips[0] - shoulders[0], hips[1] - shoulders[1]
    if dx == 0 and dy == 0:
        return UNKNOWN
    if 16 * abs(dy) <= flat * abs(dx):
        return LYING
    if dy > 0 and 16 * abs(dx) <= lean * dy:
        if squat > 0 and ankles is not None and 16 * (ankles[1] - hips[1]) < squat * dy:
            return LOW
        return UPRIGHT
    return LEANING


class PostureRef:
    def __init__(self, K, cameras=1, max_tracks=128, max_age=30, parts=None, min_frames=3, lean=11, flat=11, squat=18,
                 hand_up=4, fall_window=30, down_frames=75, max_events=256, score_thr=0.3, kpt_thr=0.):
        self.K, self.S, self.cameras, self.max_age = K, max_tracks, cameras, max_age
        self.parts = {n: tuple((PARTS[K] if parts is None else parts)[n]) for n in PART_NAMES}
        self.min_frames, self.lean, self.flat, self.squat, self.hand_up = min_frames, lean, flat, squat, hand_up
        self.fall_window, self.down_frames, self.max_events = fall_window, down_frames, max_events
        self.score_thr, self.kpt_thr = np.float32(score_thr), np.float32(kpt_thr)
        C, S = cameras, max_tracks
        for name in SLOTS:
            setattr(self, name, np.zeros((C, S), np.int32))
        self.frame = np.zeros(C, np.int32)
        self.dropped = np.zeros(C, np.int32)
        self.now = np.zeros((C, 5), np.int32)
        self.hands_up, self.falls, self.downs = (np.zeros(C, np.int32) for _ in range(3))

    def reset(self, camera=None):
        c = slice(None) if camera is None else camera
        for a in (self.id, self.frame, self.dropped, self.now, self.hands_up, self.falls, self.downs):
            a[c] = 0

    def state(self, c):
        return {n: getattr(self, n)[c] for n in STATE}

    def counts(self, c):
        return {n: getattr(self, n)[c] for n in COUNTERS}

    def _bump(self, array, at, by=1):
        array[at] = wrap32(int(array[at]) + by)

    def update(self, kpts, bboxes, ids, keep=None, scale=(1.0, 1.0), camera=0):
        """kpts [N, K, 3], bboxes [N, 5] float32, ids [N], keep [N] or None -> dict(posture, raw, hands, since [N],
        events [max_events, 5], n_events) int32."""
        c, K, S = camera, self.K, self.S
        kpts, bboxes = np.asarray(kpts, np.float32).reshape(-1, K, 3), np.asarray(bboxes, np.float32).reshape(-1, 5)
        ids = np.asarray(ids).reshape(-1)
        N = kpts.shape[0]
        sx, sy = scale
        events = []
        # the clock; slots that were not seen for too long
        self.frame[c] = wrap32(int(self.frame[c]) + 1)
        frame = int(self.frame[c])
        for t in range(S):
            if self.id[c, t] != 0 and frame - int(self.last[c, t]) > self.max_age:
                self._bump(self.now, (c, int(self.posture[c, t])), -1)
                if self.hands[c, t]:
                    self._bump(self.hands_up, c, -1)
                self.id[c, t] = 0
        # who takes part, and in which slot: section 17's step 2
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
        X = np.stack([quant(kpts[..., 0], sx), quant(kpts[..., 1], sy)], -1)                       # [N, K, 2]
        out = {n: np.zeros(N, np.int32) for n in ('posture', 'raw', 'hands', 'since')}
        out['posture'][:], out['raw'][:] = -1, -1
        for d in range(N):
            t = int(slot[d])
            if t < 0:
                continue
            # the raw class and the raw hands of this frame
            P = {n: centre(X[d, list(k)], seen[d, list(k)]) for n, k in self.parts.items()}
            raw = classify(P['shoulders'], P['hips'], P['ankles'], self.lean, self.flat, self.squat)
            mask = 0
            if self.hand_up is not None and raw in (UPRIGHT, LOW):
                dy = P['hips'][1] - P['shoulders'][1]
                for i, k in enumerate(self.parts['wrists']):
                    if seen[d, k] and 16 * (P['shoulders'][1] - 2 * int(X[d, k, 1])) >= self.hand_up * dy:
                        mask |= 1 << i
            bit = int(mask != 0)
            ident = int(ids[d])
            if born[d]:
                self.posture[c, t], self.since[c, t], self.upright[c, t] = raw, frame, 0
                self.streak[c, t], self.alerted[c, t], self.hands[c, t], self.hand_streak[c, t] = 0, 0, bit, 0
                self._bump(self.now, (c, raw))
                self._bump(self.hands_up, c, bit)
            else:
                if raw != UNKNOWN:
                    if raw == self.posture[c, t]:
                        self.streak[c, t] = 0
                    else:
                        self.streak[c, t] = wrap32(int(self.streak[c, t]) + 1)
                        if self.streak[c, t] >= self.min_frames:
                            self._bump(self.now, (c, int(self.posture[c, t])), -1)
                            self._bump(self.now, (c, raw))
                            self.posture[c, t], self.streak[c, t], self.since[c, t], self.alerted[c, t] = raw, 0, frame, 0
                            events.append((POSTURE, raw, ident, d, frame))
                            up = int(self.upright[c, t])
                            if raw == LYING and up != 0 and frame - up <= self.fall_window:
                                events.append((FALL, wrap32(frame - up), ident, d, frame))
                                self._bump(self.falls, c)
                if self.posture[c, t] == LYING and not self.alerted[c, t] and self.down_frames > 0 \
                        and frame - int(self.since[c, t]) >= self.down_frames:
                    self.alerted[c, t] = 1
                    events.append((DOWN, wrap32(frame - int(self.since[c, t])), ident, d, frame))
                    self._bump(self.downs, c)
                if raw != UNKNOWN:
                    if bit == self.hands[c, t]:
                        self.hand_streak[c, t] = 0
                    else:
                        self.hand_streak[c, t] = wrap32(int(self.hand_streak[c, t]) + 1)
                        if self.hand_streak[c, t] >= self.min_frames:
                            self.hands[c, t], self.hand_streak[c, t] = bit, 0
                            events.append((HANDS_UP if bit else HANDS_DOWN, mask, ident, d, frame))
                            self._bump(self.hands_up, c, 1 if bit else -1)
            if self.posture[c, t] == UPRIGHT:
                self.upright[c, t] = frame
            self.last[c, t] = frame
            out['posture'][d], out['raw'][d], out['hands'][d] = self.posture[c, t], raw, mask
            out['since'][d] = wrap32(frame - int(self.since[c, t]))
        table = np.zeros((self.max_events, 5), np.int32)
        stored = events[:self.max_events]
        if stored:
            table[:len(stored)] = np.asarray(stored, np.int64).astype(np.int32)
        return dict(out, events=table, n_events=np.asarray(len(events), np.int32))
