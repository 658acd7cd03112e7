"""The re-identification rule of DESIGN section 18 in numpy and Python integers: fp32 quantisation as in
tests/track_ref.py, every other step in exact integers.  Restated from the rule, not from the kernel: the state is
kept as the arrays `PersonReID.state()` shows, so a test compares them one for one."""
import numpy as np

from tests.smooth_ref import wrap32
from tests.track_ref import quant

TORSO = {17: ((5, 6), (11, 12)), 15: ((3, 4), (9, 10)), 14: ((0, 1), (6, 7))}       # (shoulders, hips)
LEGS = {17: ((11, 12), (13, 14)), 15: ((9, 10), (11, 12)), 14: ((6, 7), (8, 9))}    # (hips, knees)
BINS = (4, 8, 8)          # Y, U, V (BGR: G, B, R)
CAP = 1024                # samples of a region at the most
MIN_SAMPLES = 16          # a region of fewer samples is invalid
MAX_HITS = 32767
NEVER = 65537             # a match_thr no score reaches


def soft_bins(c, n):
    """A byte value (array) on an axis of n bins -> (bin0, bin1, weight0, weight1), the weights summing to 8."""
    c = np.asarray(c, np.int64)
    w = 256 // n
    t = np.clip(c - w // 2, 0, (n - 1) * w)
    b0 = t // w
    f = (t % w) * 8 // w
    return b0, np.minimum(b0 + 1, n - 1), 8 - f, f


def histogram(Y, U, V):
    """Samples (three equal-length arrays of bytes) -> the 256 soft-binned counts, each sample adding 512."""
    axes = [soft_bins(v, n) for v, n in zip((Y, U, V), BINS)]
    h = np.zeros(256, np.int64)
    for iy in (0, 1):
        for iu in (0, 1):
            for iv in (0, 1):
                b = (axes[0][iy] * 8 + axes[1][iu]) * 8 + axes[2][iv]
                w = axes[0][2 + iy] * axes[1][2 + iu] * axes[2][2 + iv]
                h += np.bincount(b.reshape(-1), weights=w.reshape(-1), minlength=256).astype(np.int64)
    return h


def normalise(h, n):
    return (h * 128) // n


def stride_of(w, h):
    s = 1
    while -(-w // s) * -(-h // s) > CAP:
        s *= 2
    return s


def region_rect(X, seen, upper, lower, B, fallback):
    """One region of one pose in quarter pixels, (x0, y0, x1, y1), or None: the bounding rectangle of the visible
    `upper` and `lower` key points (one of each at least), shrunk by an eighth of its extent on every side; else,
    with `fallback`, the box's central half in x and second quarter in y; then widened about its centre to a quarter
    of the box's width."""
    u, l = [k for k in upper if seen[k]], [k for k in lower if seen[k]]
    x1b, y1b, x2b, y2b = (int(v) for v in B)
    if u and l:
        xs, ys = [int(X[k, 0]) for k in u + l], [int(X[k, 1]) for k in u + l]
        x0, y0, x1, y1 = min(xs), min(ys), max(xs), max(ys)
        dx, dy = (x1 - x0) >> 3, (y1 - y0) >> 3
        x0, y0, x1, y1 = x0 + dx, y0 + dy, x1 - dx, y1 - dy
    elif fallback:
        w, h = x2b - x1b, y2b - y1b
        x0, y0, x1, y1 = x1b + (w >> 2), y1b + (h >> 2), x2b - (w >> 2), y1b + (h >> 1)
    else:
        return None
    min_w = (x2b - x1b) >> 2
    if x1 - x0 < min_w:
        x0 = (x0 + x1 - min_w) >> 1
        x1 = x0 + min_w
    return x0, y0, x1, y1


def blocks_of(rect, W, H):
    """A rectangle in quarter pixels on a W x H picture -> (bx0, by0, nx, ny, s): the first 2 x 2 block, the samples
    per row and per column and their stride in blocks; None when the region is off the picture or too small."""
    if rect is None:
        return None
    bx0, by0 = max(rect[0] >> 3, 0), max(rect[1] >> 3, 0)
    bx1, by1 = min(rect[2] >> 3, (W >> 1) - 1), min(rect[3] >> 3, (H >> 1) - 1)
    if bx0 > bx1 or by0 > by1:
        return None
    w, h = bx1 - bx0 + 1, by1 - by0 + 1
    s = stride_of(w, h)
    nx, ny = -(-w // s), -(-h // s)
    if nx * ny < MIN_SAMPLES:
        return None
    return bx0, by0, nx, ny, s


def samples(kind, picture, W, H, blocks):
    """The (Y, U, V) of the samples of a region ((G, B, R) of a BGR picture), as int64 arrays [ny, nx]."""
    bx0, by0, nx, ny, s = blocks
    bx, by = bx0 + s * np.arange(nx), by0 + s * np.arange(ny)
    p = np.asarray(picture).astype(np.int64)
    if kind == 'nv12':
        r, c = 2 * by[:, None], 2 * bx[None, :]
        Y = (p[r, c] + p[r, c + 1] + p[r + 1, c] + p[r + 1, c + 1] + 2) >> 2
        return Y, p[H + by[:, None], c], p[H + by[:, None], c + 1]
    r, c = 2 * by[:, None], 2 * bx[None, :]
    mean = (p[r, c] + p[r, c + 1] + p[r + 1, c] + p[r + 1, c + 1] + 2) >> 2      # [ny, nx, 3] (B, G, R)
    return mean[..., 1], mean[..., 0], mean[..., 2]


def geometry(kind, picture, width):
    picture = np.asarray(picture)
    if kind == 'nv12':
        return int(width), picture.shape[0] * 2 // 3
    return picture.shape[1], picture.shape[0]


def describe(kind, picture, width, kpts, bboxes, keep=None, scale=(1.0, 1.0), K=17, torso=None, legs=None,
             score_thr=0.3, kpt_thr=0.):
    """-> dict(hist [N, 2, 256], count [N, 2] int32; valid [N], rect [N, 2, 4], box [N, 4] for the gallery)."""
    kpts, bboxes = np.asarray(kpts, np.float32).reshape(-1, K, 3), np.asarray(bboxes, np.float32).reshape(-1, 5)
    N = kpts.shape[0]
    W, H = geometry(kind, picture, width)
    torso, legs = TORSO[K] if torso is None else torso, LEGS[K] if legs is None else legs
    usable = np.isfinite(bboxes[:, :4]).all(1) & np.isfinite(kpts[..., :2]).all((1, 2))
    with np.errstate(invalid='ignore'):
        valid = usable & (bboxes[:, 4] > np.float32(score_thr))
        seen = kpts[..., 2] > np.float32(kpt_thr)
    if keep is not None:
        valid &= np.asarray(keep).reshape(-1) != 0
    sx, sy = scale
    X = np.stack([quant(kpts[..., 0], sx), quant(kpts[..., 1], sy)], -1)
    B = np.stack([quant(bboxes[:, 0], sx), quant(bboxes[:, 1], sy), quant(bboxes[:, 2], sx), quant(bboxes[:, 3], sy)], 1)
    hist, count = np.zeros((N, 2, 256), np.int32), np.zeros((N, 2), np.int32)
    rect = np.zeros((N, 2, 4), np.int64)
    for d in range(N):
        if not valid[d]:
            continue
        for r, (parts, fallback) in enumerate(((torso, True), (legs, False))):
            R = region_rect(X[d], seen[d], parts[0], parts[1], B[d], fallback)
            blocks = blocks_of(R, W, H)
            if blocks is None:
                continue
            rect[d, r] = R
            Y, U, V = samples(kind, picture, W, H, blocks)
            n = blocks[2] * blocks[3]
            hist[d, r], count[d, r] = normalise(histogram(Y, U, V), n), n
    return dict(hist=hist, count=count, valid=valid, rect=rect, box=B)


def similarity(a, b):
    return int(np.minimum(np.asarray(a, np.int64), np.asarray(b, np.int64)).sum())


class ReIDRef:
    def __init__(self, K, cameras=1, max_people=128, max_lost=900, match_thr=None, min_hits=3, gain=2, torso=None,
                 legs=None, score_thr=0.3, kpt_thr=0., default_thr=None):
        self.K, self.S, self.cameras, self.max_lost = K, max_people, cameras, max_lost
        self.match_thr = default_thr if match_thr is None else match_thr
        self.min_hits, self.gain = min_hits, gain
        self.torso, self.legs = TORSO.get(K) if torso is None else torso, LEGS.get(K) if legs is None else legs
        self.score_thr, self.kpt_thr = score_thr, kpt_thr
        C, S = cameras, max_people
        self.person = np.zeros((C, S), np.int32)
        self.track = np.zeros((C, S), np.int32)
        self.last = np.zeros((C, S), np.int32)
        self.hits = np.zeros((C, S, 2), np.int32)
        self.hist = np.zeros((C, S, 2, 256), np.int32)
        self.frame = np.zeros(C, np.int32)
        self.next = np.ones(C, np.int32)
        self.dropped = np.zeros(C, np.int32)

    def reset(self, camera=None):
        c = slice(None) if camera is None else camera
        for a in (self.person, self.frame, self.dropped):
            a[c] = 0

    def state(self, c):
        return {n: getattr(self, n)[c] for n in ('person', 'track', 'last', 'hits', 'hist', 'frame', 'next', 'dropped')}

    def describe(self, kind, picture, width, kpts, bboxes, keep=None, scale=(1.0, 1.0)):
        return describe(kind, picture, width, kpts, bboxes, keep, scale, self.K, self.torso, self.legs, self.score_thr,
                        self.kpt_thr)

    def score(self, c, t, q, count):
        """The score of a pose (its descriptors q [2, 256] and counts [2]) against slot t, or None."""
        if count[0] == 0 or self.hits[c, t, 0] == 0:
            return None
        s = similarity(q[0], self.hist[c, t, 0])
        if count[1] > 0 and self.hits[c, t, 1] > 0:
            s = (s + similarity(q[1], self.hist[c, t, 1])) >> 1
        return s

    def update(self, kind, picture, width, kpts, bboxes, ids, keep=None, scale=(1.0, 1.0), camera=0):
        """-> dict(ids [N], sim [N]) int32."""
        c, S = camera, self.S
        ids = np.asarray(ids).reshape(-1).astype(np.int64)
        d = self.describe(kind, picture, width, kpts, bboxes, keep, scale)
        q, count, rect, box = d['hist'], d['count'], d['rect'], d['box']
        N = len(ids)
        self.frame[c] = wrap32(int(self.frame[c]) + 1)
        frame = int(self.frame[c])
        # 1
        for t in range(S):
            if self.person[c, t] != 0 and frame - int(self.last[c, t]) > self.max_lost:
                self.person[c, t] = 0
        part = np.zeros(N, bool)
        named = np.nonzero(d['valid'] & (ids >= 1))[0]
        part[named[np.unique(ids[named], return_index=True)[1]]] = True
        out_ids, sim, slot = np.zeros(N, np.int32), np.zeros(N, np.int32), np.full(N, -1)
        # 2
        for p in np.nonzero(part)[0]:
            have = np.nonzero((self.person[c] != 0) & (self.track[c] == ids[p]))[0]
            if len(have):
                slot[p] = int(have[0])
                self.last[c, slot[p]] = frame
        # 3
        here = set(int(v) for v in ids[part])
        cands = [t for t in range(S) if self.person[c, t] != 0 and int(self.track[c, t]) not in here
                 and int(self.last[c, t]) < frame and int(self.hits[c, t, 0]) >= self.min_hits]
        pairs = []
        for p in np.nonzero(part & (slot < 0))[0]:
            for t in cands:
                s = self.score(c, t, q[p], count[p])
                if s is not None and s >= self.match_thr:
                    pairs.append((-s, int(p), t))
        taken_p, taken_t = set(), set()
        for s, p, t in sorted(pairs):
            if p in taken_p or t in taken_t:
                continue
            taken_p.add(p), taken_t.add(t)
            slot[p], sim[p] = t, -s
            self.track[c, t], self.last[c, t] = ids[p], frame
        # 4
        for p in np.nonzero(part & (slot < 0))[0]:
            free = np.nonzero(self.person[c] == 0)[0]
            lost = np.nonzero((self.person[c] != 0) & (self.last[c] < frame))[0]
            if len(free):
                t = int(free[0])
            elif len(lost):
                t = int(lost[np.argmin(self.last[c, lost])])      # (argmin: the first of equals)
            else:
                self.dropped[c] = wrap32(int(self.dropped[c]) + 1)
                continue
            slot[p] = t
            self.person[c, t], self.next[c] = self.next[c], wrap32(int(self.next[c]) + 1)
            self.track[c, t], self.last[c, t] = ids[p], frame
            self.hits[c, t], self.hist[c, t] = 0, 0
        # the descriptors of every pose that has a slot
        for p in np.nonzero(slot >= 0)[0]:
            t = int(slot[p])
            out_ids[p] = self.person[c, t]
            for r in (0, 1):
                if count[p, r] == 0:
                    continue
                x0, y0, x1, y1 = (int(v) for v in rect[p, r])
                if any(e != p and part[e] and x0 <= box[e, 2] and box[e, 0] <= x1 and y0 <= box[e, 3] and box[e, 1] <= y1
                       for e in range(N)):
                    continue
                if self.hits[c, t, r] == 0:
                    self.hist[c, t, r] = q[p, r]
                else:
                    old = self.hist[c, t, r].astype(np.int64)
                    self.hist[c, t, r] = old + (((q[p, r].astype(np.int64) - old) * self.gain + 8) >> 4)
                self.hits[c, t, r] = min(int(self.hits[c, t, r]) + 1, MAX_HITS)
        return dict(ids=out_ids, sim=sim)
