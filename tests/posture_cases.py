"""Scenarios for the posture rule of DESIGN section 20 that the CPU and the GPU tests share: the edges of the rule as
small scripts with values worked out by hand.  A script drives a harness `make(K, **arguments)` with
  h.frame(kpts, bboxes, ids, keep=None, camera=0) -> dict(posture, raw, hands, since, events, n_events) as numpy int32
  h.poke(field, index, value, camera=0)              a write into a camera's state
  h.get(field, camera=0)                             a camera's state or counter tensor as numpy
The CPU harness is the oracle alone; the GPU harness runs the device beside it and compares everything after every
frame, so the hand-worked values below hold for both.  Both call `invariant` after every frame.

Most scripts use K = 8 with two key points per part (`TWO`): the centre of a part with both points visible is
floor(2 (X0 + X1) / 2) = X0 + X1 in 1/8 pixel, so `body` places a centre on any integer and the scripts think in
1/8 pixel -- the unit of every threshold."""
import numpy as np

UNKNOWN, UPRIGHT, LOW, LEANING, LYING = 0, 1, 2, 3, 4
POSTURE, FALL, DOWN, HANDS_UP, HANDS_DOWN = 1, 2, 3, 4, 5
TWO = dict(parts=dict(shoulders=(0, 1), hips=(2, 3), ankles=(4, 5), wrists=(6, 7)))
FOUR = dict(parts=dict(shoulders=(0, 1, 2, 3), hips=(4, 5, 6, 7), ankles=(8, 9, 10, 11), wrists=(12, 13, 14, 15)))


def invariant(state, counts):
    """now[c] == the live slots whose posture is c (so their sum is the live slots); hands_up == those with the bit."""
    live = np.asarray(state['id']) != 0
    posture = np.asarray(state['posture'])[live]
    for c in range(5):
        assert int(counts['now'][c]) == int((posture == c).sum()), (c, counts['now'].tolist(), posture.tolist())
    assert int(np.asarray(counts['now']).sum()) == int(live.sum())
    assert int(counts['hands_up']) == int((np.asarray(state['hands'])[live] != 0).sum())


def body(sh, hip, ank=None, wrists=(None, None), box_score=0.8):
    """One K = 8 pose: sh, hip, ank the centres of its shoulders, hips and ankles in 1/8 pixel (None: both points
    with score 0, not visible), wrists two (X, Y) in quarter pixels or None.  A centre v is split into the quarter
    pixel coordinates v // 2 and v - v // 2, which fp32 holds exactly."""
    kp = np.zeros((1, 8, 3), np.float32)
    for p, c in enumerate((sh, hip, ank)):
        if c is not None:
            for a in (0, 1):
                kp[0, 2 * p, a], kp[0, 2 * p + 1, a] = (c[a] // 2) / 4.0, (c[a] - c[a] // 2) / 4.0
            kp[0, 2 * p:2 * p + 2, 2] = 0.9
    for i, w in enumerate(wrists):
        if w is not None:
            kp[0, 6 + i] = (w[0] / 4.0, w[1] / 4.0, 0.9)
    return kp, np.asarray([[0.0, 0.0, 50.0, 100.0, box_score]], np.float32)


def group(*bodies):
    return np.concatenate([b[0] for b in bodies]), np.concatenate([b[1] for b in bodies])


def none(K=8):
    return np.zeros((0, K, 3), np.float32), np.zeros((0, 5), np.float32), np.zeros(0, np.int32)


def ev(out):
    """The stored events of a frame as tuples."""
    n = min(int(out['n_events']), len(out['events']))
    assert not out['events'][n:].any()
    return [tuple(int(v) for v in row) for row in out['events'][:n]]


def born(make, bodies, **kw):
    """The raw classes and raw hands of poses born in one frame (a born slot takes them as they are)."""
    h = make(8, **dict(TWO, **kw))
    out = h.frame(*group(*bodies), list(range(1, len(bodies) + 1)))
    assert out['posture'].tolist() == out['raw'].tolist() and int(out['n_events']) == 0 and not out['since'].any()
    return out['raw'].tolist(), out['hands'].tolist()


S0 = (400, 400)                                       # where the shoulders stand in most scripts
STAND = body(S0, (400, 560), (400, 800))              # dy = 160, ankles 240 below the hips (>= 180: not LOW)
CROUCH = body(S0, (400, 560), (400, 700))             # ankles 140 below the hips
LEAN = body(S0, (520, 520), (400, 800))               # dx = dy = 120: neither test holds
LIE = body(S0, (560, 400), (800, 400))                # dy = 0
NOBODY = body(None, (400, 560), (400, 800))           # no shoulder: UNKNOWN
HANDS = dict(wrists=((90, 100), (110, 100)))          # both wrists far above the shoulders
STAND_UP = body(S0, (400, 560), (400, 800), **HANDS)


def flat_threshold(make):
    """flat = 11, dx = 160: 16 |dy| <= 1760 iff |dy| <= 110.  At 110 LYING, at 111 LEANING (16 * 160 > 11 * 111, so
    not UPRIGHT either), either sign of dy and of dx."""
    want = [(110, LYING), (111, LEANING), (109, LYING), (-110, LYING), (-111, LEANING), (0, LYING)]
    for sign in (1, -1):
        raw, _ = born(make, [body(S0, (400 + sign * 160, 400 + dy)) for dy, _ in want])
        assert raw == [c for _, c in want], (sign, raw)
    # flat = 1: 16 |dy| <= |dx|: dx = 160 allows |dy| <= 10;  flat = 255: dx = 16 allows |dy| <= 255
    raw, _ = born(make, [body(S0, (560, 410)), body(S0, (560, 411))], flat=1)
    assert raw == [LYING, LEANING]
    raw, _ = born(make, [body(S0, (416, 655)), body(S0, (416, 656))], flat=255)
    assert raw == [LYING, UPRIGHT]                    # (16 * 16 = 256 <= 11 * 256)


def lean_threshold(make):
    """lean = 11, dy = 160: 16 |dx| <= 1760 iff |dx| <= 110.  At 110 UPRIGHT, at 111 LEANING; the head below the hips
    (dy < 0) is LEANING however straight."""
    want = [(110, UPRIGHT), (111, LEANING), (109, UPRIGHT), (-110, UPRIGHT), (-111, LEANING), (0, UPRIGHT)]
    raw, _ = born(make, [body(S0, (400 + dx, 560)) for dx, _ in want])
    assert raw == [c for _, c in want], raw
    raw, _ = born(make, [body(S0, (400, 240)), body(S0, (410, 240)), body(S0, (400, 399)), body(S0, (400, 401))])
    assert raw == [LEANING, LEANING, LEANING, UPRIGHT]
    raw, _ = born(make, [body(S0, (410, 560)), body(S0, (411, 560))], lean=1)
    assert raw == [UPRIGHT, LEANING]                  # 16 |dx| <= 160


def lying_wins(make):
    """flat = lean = 255, dx = dy = 100: both 16 * 100 <= 255 * 100 hold: LYING is tested first.  dx = 0 cannot be
    LYING (16 dy <= 0 fails): UPRIGHT."""
    raw, _ = born(make, [body(S0, (500, 500)), body(S0, (400, 500)), body(S0, (500, 400))], flat=255, lean=255)
    assert raw == [LYING, UPRIGHT, LYING]


def squat_threshold(make):
    """squat = 18, dy = 160: LOW iff 16 (ankles.y - hips.y) < 2880 iff the ankles are less than 180 below the hips:
    179 LOW, 180 and 181 UPRIGHT; ankles above the hips LOW; no ankle visible UPRIGHT; squat = 0 never LOW."""
    rows = [body(S0, (400, 560), (400, 560 + a)) for a in (179, 180, 181, -50)] + [body(S0, (400, 560))]
    raw, _ = born(make, rows)
    assert raw == [LOW, UPRIGHT, UPRIGHT, LOW, UPRIGHT]
    raw, _ = born(make, rows, squat=0)
    assert raw == [UPRIGHT] * 5
    raw, _ = born(make, [body(S0, (400, 560), (400, 560 + a)) for a in (2549, 2550)], squat=255)
    assert raw == [LOW, UPRIGHT]                      # 16 a < 255 * 160 = 40800 iff a < 2550
    # a LEANING or LYING trunk is never LOW
    raw, _ = born(make, [body(S0, (520, 520), (520, 530)), body(S0, (560, 400), (560, 400))])
    assert raw == [LEANING, LYING]


def hand_threshold(make):
    """hand_up = 4, dy = 160: wrist at quarter-pixel Y is raised iff 16 (shoulders.y - 2 Y) >= 640 iff shoulders.y -
    2 Y >= 40.  shoulders.y = 400: Y = 180 gives 40 (raised), Y = 181 gives 38; shoulders.y = 401 (hips.y 561): Y =
    180 gives 41, Y = 181 gives 39: one unit either side.  Bit i is wrist i; a wrist that is not visible sets
    nothing."""
    def up(sy, y0=None, y1=None):
        return body((400, sy), (400, sy + 160), (400, sy + 400), wrists=(None if y0 is None else (100, y0),
                                                                          None if y1 is None else (100, y1)))
    rows = [up(400, 180), up(400, 181), up(401, 180), up(401, 181), up(400, None, 180), up(400, 180, 0), up(400, 181, 0),
            up(400)]
    raw, hands = born(make, rows)
    assert raw == [UPRIGHT] * 8 and hands == [1, 0, 1, 0, 2, 3, 2, 0]
    _, hands = born(make, rows, hand_up=None)
    assert hands == [0] * 8
    _, hands = born(make, [up(400, 200), up(400, 201), up(401, 200)], hand_up=0)
    assert hands == [1, 0, 1]                         # level with the shoulders: 400 - 400 >= 0
    _, hands = born(make, [up(2549, 0), up(2550, 0)], hand_up=255)
    assert hands == [0, 1]                            # 16 * 2549 = 40784 < 255 * 160 = 40800 = 16 * 2550
    # LOW counts, LEANING, LYING and UNKNOWN do not, wherever the wrists are
    raw, hands = born(make, [body(S0, (400, 560), (400, 700), **HANDS), body(S0, (520, 520), **HANDS),
                             body(S0, (560, 400), **HANDS), body(None, (400, 560), **HANDS)])
    assert raw == [LOW, LEANING, LYING, UNKNOWN] and hands == [3, 0, 0, 0]


def ends_of_the_range(make):
    """Quarter-pixel coordinates end at 32767 (8191.75 px), centres at 65534: with the shoulders at 0, dx = 65534 and
    16 dy <= 11 * 65534 = 720874 iff dy <= 45054 -- the same answers as in the small, whatever the word size of the
    products.  A coordinate beyond the range is clamped to it, one below 0 to 0."""
    raw, _ = born(make, [body((0, 0), (65534, 45054)), body((0, 0), (65534, 45055)), body((0, 0), (45054, 65534)),
                         body((0, 0), (45055, 65534)), body((0, 65534), (0, 0))])
    assert raw == [LYING, LEANING, UPRIGHT, LEANING, LEANING]
    raw, hands = born(make, [body((65534, 30000), (65534, 65534), (65534, 65534), wrists=((32767, 0), (0, 32767)))],
                      squat=255, hand_up=255)
    assert raw == [LOW] and hands == [0]              # 16 * 30000 < 255 * 35534
    kp, bb = body((0, 0), (800, 0))
    kp[0, 2:4, 0] = (9000.0, 1e30)                    # both clamp to 32767: dx = 65534
    kp[0, 2:4, 1] = (-3.0, -1e30)                     # both clamp to 0
    kp2, bb2 = body((0, 0), (0, 0))
    h = make(8, **TWO)
    out = h.frame(*group((kp, bb), (kp2, bb2)), [1, 2])
    assert out['raw'].tolist() == [LYING, UNKNOWN]    # dx = dy = 0 is UNKNOWN
    assert h.get('now').tolist() == [1, 0, 0, 0, 1]


def _figure16(points):
    """K = 16, four key points per part: points[p] a list of (X, Y, score) in quarter pixels for part p."""
    kp = np.zeros((1, 16, 3), np.float32)
    for p, rows in enumerate(points):
        for i, (x, y, s) in enumerate(rows):
            kp[0, 4 * p + i] = (x / 4.0, y / 4.0, s)
    return kp, np.asarray([[0.0, 0.0, 50.0, 100.0, 0.8]], np.float32)


def _pair16(v):
    """Two visible points and two that are not, whose centre is v (1/8 pixel)."""
    return [(v[0] // 2, v[1] // 2, 0.9), (v[0] - v[0] // 2, v[1] - v[1] // 2, 0.9), (7, 9, 0.0), (30000, 5, -1.0)]


# 1, 3 and 4 visible points about (1000, 1000) quarter pixels and their centres floor(2 sum / n):
# n = 3: x (3034 * 2) / 3 = 2022.67 -> 2022, y (3065 * 2) / 3 = 2043.33 -> 2043;  n = 4: x 8094 / 4 = 2023.5 -> 2023,
# y 8174 / 4 = 2043.5 -> 2043
SEEN = {1: ([(1010, 1020)], (2020, 2040)),
        3: ([(1010, 1020), (1011, 1021), (1013, 1024)], (2022, 2043)),
        4: ([(1010, 1020), (1011, 1021), (1013, 1024), (1013, 1022)], (2023, 2043))}


def visible_points_of_a_part(make):
    """Each of shoulders, hips and ankles with 1, 3 and 4 visible points (the others with score 0, far away): the
    centre is pinned to the unit by poses at a threshold and one unit past it.  Shoulders at C: hips at C + (160,
    110) LYING and C + (159, 110) LEANING pin C.x; C + (110, 160) UPRIGHT and C + (110, 159) LEANING pin C.y.  Hips at
    C likewise with the shoulders at C - those.  Ankles at C: hips 180 above are UPRIGHT, 179 above LOW.  No visible
    point: UNKNOWN for shoulders and hips, UPRIGHT (never LOW) for ankles."""
    offsets = [((160, 110), LYING), ((159, 110), LEANING), ((110, 160), UPRIGHT), ((110, 159), LEANING)]
    for n, (pts, C) in SEEN.items():
        rows = [(x, y, 0.9) for x, y in pts] + [(5, 31000, 0.0)] * (4 - n)
        poses, want = [], []
        for (ox, oy), c in offsets:
            poses.append(_figure16([rows, _pair16((C[0] + ox, C[1] + oy)), [], []]))
            poses.append(_figure16([_pair16((C[0] - ox, C[1] - oy)), rows, [], []]))
            want += [c, c]
        for above, c in ((180, UPRIGHT), (179, LOW)):
            poses.append(_figure16([_pair16((C[0], C[1] - above - 160)), _pair16((C[0], C[1] - above)), rows, []]))
            want.append(c)
        h = make(16, **FOUR)
        out = h.frame(*group(*poses), list(range(1, len(poses) + 1)))
        assert out['raw'].tolist() == want, (n, out['raw'].tolist(), want)
    unseen = [(1000, 1000, 0.0)] * 4
    h = make(16, **FOUR)
    out = h.frame(*group(_figure16([unseen, _pair16((2000, 2160)), [], []]), _figure16([_pair16((2000, 2000)), unseen, [], []]),
                         _figure16([_pair16((2000, 2000)), _pair16((2000, 2160)), unseen, []]),
                         _figure16([_pair16((2000, 2000)), _pair16((2000, 2160)), _pair16((2000, 2200)), []])), [1, 2, 3, 4])
    assert out['raw'].tolist() == [UNKNOWN, UNKNOWN, UPRIGHT, LOW]
    # the wrists one by one: shoulders.y = 2000, dy = 160: raised iff 2000 - 2 Y >= 40 iff Y <= 980
    trunk = [_pair16((2000, 2000)), _pair16((2000, 2160)), _pair16((2000, 2400))]
    masks = []
    for wr in ([(0, 990, 0.9), (0, 980, 0.0), (0, 980, 0.0), (0, 980, 0.0)],          # 0 raised of 1 visible
               [(0, 990, 0.0), (0, 980, 0.9), (0, 980, 0.0), (0, 980, 0.0)],          # 1 visible
               [(0, 981, 0.9), (0, 980, 0.9), (0, 0, 0.0), (0, 979, 0.9)],            # 3 visible, 2 raised
               [(0, 980, 0.9), (0, 981, 0.9), (0, 980, 0.9), (0, 100, 0.9)],          # 4 visible, 3 raised
               [(0, 0, 0.0)] * 4):
        h = make(16, **FOUR)
        masks.append(int(h.frame(*_figure16(trunk + [wr]), [1])['hands'][0]))
    assert masks == [0, 2, 10, 13, 0]


def score_at_the_threshold(make):
    """kpt_thr = 0.5: a key point with score exactly 0.5 is not visible.  One shoulder at x = 100 with 0.9 and one at x
    = 300 with 0.5 over hips at x = 100: with the second shoulder the trunk would be LEANING (dx = -200, dy = 160),
    without it it is UPRIGHT; just above the threshold it counts."""
    kp, bb = body((200, 400), (200, 560))
    kp[0, 0, :2], kp[0, 1, :2] = (25.0, 50.0), (75.0, 50.0)          # X = 100 and 300: centre 400 with both, 200 with one
    kp[0, 1, 2] = 0.5
    kp2 = kp.copy()
    kp2[0, 1, 2] = np.nextafter(np.float32(0.5), np.float32(1))
    h = make(8, kpt_thr=0.5, **TWO)
    assert h.frame(*group((kp, bb), (kp2, bb)), [1, 2])['raw'].tolist() == [UPRIGHT, LEANING]


def unknown_inside_a_streak(make):
    """min_frames 3: born UPRIGHT; LYING, LYING, UNKNOWN, LYING: the UNKNOWN frame changes nothing (streak 1, 2, 2, 3),
    so the posture follows in frame 5.  The slot stayed UPRIGHT up to frame 4, so the fall is 1 frame old."""
    h = make(8, **TWO)
    seen = []
    for f, b in enumerate((STAND, LIE, LIE, NOBODY, LIE, LIE)):
        out = h.frame(*b, [9])
        seen.append((int(out['posture'][0]), int(out['raw'][0]), int(h.get('streak')[0]), int(out['since'][0]), ev(out)))
    assert [s[:4] for s in seen] == [(1, 1, 0, 0), (1, 4, 1, 1), (1, 4, 2, 2), (1, 0, 2, 3), (4, 4, 0, 0), (4, 4, 0, 1)]
    assert [s[4] for s in seen] == [[], [], [], [], [(POSTURE, LYING, 9, 0, 5), (FALL, 1, 9, 0, 5)], []]
    assert h.get('upright')[0] == 4 and h.get('since')[0] == 5 and h.get('falls') == 1
    # a frame of the old posture ends the streak
    h = make(8, **TWO)
    streaks = []
    for b in (STAND, LIE, LIE, STAND, LIE, LIE):
        out = h.frame(*b, [9])
        streaks.append(int(h.get('streak')[0]))
        assert int(out['posture'][0]) == UPRIGHT and int(out['n_events']) == 0
    assert streaks == [0, 1, 2, 0, 1, 2]


def the_class_that_completes_the_streak(make):
    """min_frames 3: UPRIGHT, then LEANING, LEANING, LYING: three frames that differ from the posture, and the posture
    becomes the class of the third, LYING, though LYING was seen once."""
    h = make(8, **TWO)
    for b in (STAND, LEAN, LEAN):
        assert ev(h.frame(*b, [3])) == []
    out = h.frame(*LIE, [3])
    assert ev(out) == [(POSTURE, LYING, 3, 0, 4), (FALL, 1, 3, 0, 4)] and out['posture'].tolist() == [LYING]
    assert h.get('now').tolist() == [0, 0, 0, 0, 1]


def min_frames_one(make):
    """min_frames 1: the posture is the raw class of every frame that has one.  The slot was UPRIGHT in frame 1 only, so
    LYING in frame 5 is a FALL of 4 frames (<= 30)."""
    h = make(8, min_frames=1, **TWO)
    got = []
    for b in (STAND, CROUCH, NOBODY, LEAN, LIE, STAND):
        out = h.frame(*b, [2])
        got.append((int(out['posture'][0]), ev(out)))
    assert got == [(UPRIGHT, []), (LOW, [(POSTURE, LOW, 2, 0, 2)]), (LOW, []), (LEANING, [(POSTURE, LEANING, 2, 0, 4)]),
                   (LYING, [(POSTURE, LYING, 2, 0, 5), (FALL, 4, 2, 0, 5)]), (UPRIGHT, [(POSTURE, UPRIGHT, 2, 0, 6)])]
    assert h.get('upright')[0] == 6 and h.get('falls') == 1


def fall_window_edges(make):
    """min_frames 1, fall_window 3.  Id 1: UPRIGHT in frame 1, LEANING in 2 and 3, LYING in 4: 4 - 1 = 3 <= 3, a FALL of
    3 frames.  Id 2 leans one frame longer: 5 - 1 = 4: a POSTURE event alone.  fall_window 0: no fall is ever quick
    enough (a LYING slot was UPRIGHT at least one frame ago)."""
    h = make(8, min_frames=1, fall_window=3, **TWO)
    h.frame(*group(STAND, STAND), [1, 2])
    for _ in range(2):
        h.frame(*group(LEAN, LEAN), [1, 2])
    assert ev(h.frame(*group(LIE, LEAN), [1, 2])) == [(POSTURE, LYING, 1, 0, 4), (FALL, 3, 1, 0, 4)]
    assert ev(h.frame(*group(LIE, LIE), [1, 2])) == [(POSTURE, LYING, 2, 1, 5)]
    assert h.get('falls') == 1 and h.get('upright')[:2].tolist() == [1, 1]
    h = make(8, min_frames=1, fall_window=0, **TWO)
    h.frame(*STAND, [1])
    assert ev(h.frame(*LIE, [1])) == [(POSTURE, LYING, 1, 0, 2)] and h.get('falls') == 0


def born_lying(make):
    """A track that is LYING when it is first seen never was upright: no event at its birth, no FALL when it is seen
    LYING again after getting up to LEANING only; DOWN after down_frames frames counts from its birth."""
    h = make(8, min_frames=1, down_frames=3, **TWO)
    out = h.frame(*LIE, [6])
    assert ev(out) == [] and out['posture'].tolist() == [LYING] and h.get('upright')[0] == 0
    assert ev(h.frame(*LEAN, [6])) == [(POSTURE, LEANING, 6, 0, 2)]
    assert ev(h.frame(*LIE, [6])) == [(POSTURE, LYING, 6, 0, 3)]
    assert ev(h.frame(*LIE, [6])) == [] and ev(h.frame(*LIE, [6])) == []
    assert ev(h.frame(*LIE, [6])) == [(DOWN, 3, 6, 0, 6)]
    assert h.get('falls') == 0 and h.get('downs') == 1


def down_once_per_stay(make):
    """min_frames 1, down_frames 2: born LYING in frame 1; frame 3 is 2 frames in: DOWN, once; not again in 4 and 5;
    up in 6 (alerted cleared), LYING again in 7 (a FALL, 1 frame after UPRIGHT), DOWN again in 9.  An UNKNOWN frame
    still counts the time.  down_frames 0 never reports."""
    h = make(8, min_frames=1, down_frames=2, **TWO)
    got = []
    for b in (LIE, LIE, LIE, LIE, LIE, STAND, LIE, NOBODY, NOBODY, LIE):
        out = h.frame(*b, [5])
        got.append((ev(out), int(out['since'][0])))
    assert got == [([], 0), ([], 1), ([(DOWN, 2, 5, 0, 3)], 2), ([], 3), ([], 4), ([(POSTURE, UPRIGHT, 5, 0, 6)], 0),
                   ([(POSTURE, LYING, 5, 0, 7), (FALL, 1, 5, 0, 7)], 0), ([], 1), ([(DOWN, 2, 5, 0, 9)], 2), ([], 3)]
    assert h.get('downs') == 2 and h.get('falls') == 1 and h.get('alerted')[0] == 1
    h = make(8, min_frames=1, down_frames=0, **TWO)
    for _ in range(5):
        assert ev(h.frame(*LIE, [5])) == []
    assert h.get('downs') == 0 and h.get('alerted')[0] == 0


def hands_are_debounced(make):
    """min_frames 2: the bit "any hand raised" follows after two frames in a row; HANDS_UP and HANDS_DOWN carry the
    raw mask of the frame; a slot born with a hand up has the bit at once, without an event; an UNKNOWN frame changes
    nothing.  One wrist alone is enough."""
    one = body(S0, (400, 560), (400, 800), wrists=(None, (110, 100)))
    h = make(8, min_frames=2, **TWO)
    got = []
    for b in (STAND, STAND_UP, STAND, one, NOBODY, one, STAND, STAND_UP, STAND, STAND):
        out = h.frame(*b, [4])
        got.append((int(out['hands'][0]), int(h.get('hands')[0]), int(h.get('hand_streak')[0]), ev(out)))
    assert got == [(0, 0, 0, []), (3, 0, 1, []), (0, 0, 0, []), (2, 0, 1, []), (0, 0, 1, []),
                   (2, 1, 0, [(HANDS_UP, 2, 4, 0, 6)]), (0, 1, 1, []), (3, 1, 0, []), (0, 1, 1, []),
                   (0, 0, 0, [(HANDS_DOWN, 0, 4, 0, 10)])]
    h = make(8, min_frames=2, **TWO)
    out = h.frame(*STAND_UP, [4])
    assert ev(out) == [] and h.get('hands')[0] == 1 and h.get('hands_up') == 1


def order_of_events(make):
    """min_frames 1: two people with their hands up fall in one frame: per pose in ascending index POSTURE, FALL, then
    the hands event (a LYING pose has no raised hands).  A third stays as they are."""
    h = make(8, min_frames=1, **TWO)
    h.frame(*group(STAND_UP, STAND, STAND_UP), [7, 8, 9])
    assert h.get('hands_up') == 2
    out = h.frame(*group(LIE, STAND, LIE), [7, 8, 9])
    assert ev(out) == [(POSTURE, LYING, 7, 0, 2), (FALL, 1, 7, 0, 2), (HANDS_DOWN, 0, 7, 0, 2),
                       (POSTURE, LYING, 9, 2, 2), (FALL, 1, 9, 2, 2), (HANDS_DOWN, 0, 9, 2, 2)]
    assert h.get('now').tolist() == [0, 1, 0, 0, 2] and h.get('hands_up') == 0 and h.get('falls') == 2


def expiry_leaves_the_counters(make):
    """max_age 2: a LYING track and an UPRIGHT one with a hand up, seen in frame 1 and not again: frame 4 frees both
    slots (4 - 1 > 2) and `now` and `hands_up` let them go, without events.  The id comes back as a birth."""
    h = make(8, max_age=2, min_frames=1, **TWO)
    h.frame(*group(LIE, STAND_UP), [1, 2])
    assert h.get('now').tolist() == [0, 1, 0, 0, 1] and h.get('hands_up') == 1
    for _ in range(2):
        assert int(h.frame(*none())['n_events']) == 0
    assert h.get('now').tolist() == [0, 1, 0, 0, 1] and h.get('id')[:2].tolist() == [1, 2]
    assert int(h.frame(*none())['n_events']) == 0
    assert h.get('now').tolist() == [0] * 5 and h.get('hands_up') == 0 and not h.get('id').any()
    out = h.frame(*STAND, [1])                      # born again: no FALL history, no event
    assert ev(out) == [] and h.get('since')[0] == 5 and h.get('now').tolist() == [0, 1, 0, 0, 0]
    # seen again max_age frames later: the last moment (7 - 5 = 2 is not > 2)
    h.frame(*none())
    assert ev(h.frame(*LIE, [1])) == [(POSTURE, LYING, 1, 0, 7), (FALL, 2, 1, 0, 7)]


def duplicate_and_unusable(make):
    """Of two valid poses with one id the first takes part and the second gets -1; a pose that is not valid does not
    count as the first; ids <= 0 take no slot; a score at the threshold, a NaN key point anywhere in the pose and
    an infinite box corner make a pose unusable."""
    h = make(8, min_frames=1, **TWO)
    out = h.frame(*group(STAND, LIE), [7, 7])
    assert out['posture'].tolist() == [UPRIGHT, -1] and out['raw'].tolist() == [UPRIGHT, -1]
    assert h.get('id')[:2].tolist() == [7, 0]
    out = h.frame(*group(STAND, LIE, CROUCH), [7, 7, 5], keep=[0, 1, 1])
    assert out['posture'].tolist() == [-1, LYING, LOW] and h.get('id')[:3].tolist() == [7, 5, 0]
    assert ev(out) == [(POSTURE, LYING, 7, 1, 2), (FALL, 1, 7, 1, 2)]
    h = make(8, **TWO)
    out = h.frame(*group(STAND_UP, STAND_UP, STAND_UP), [0, -3, -(2 ** 31)])
    assert not h.get('id').any() and h.get('dropped') == 0 and h.get('frame') == 1 and int(out['n_events']) == 0
    assert out['posture'].tolist() == [-1] * 3 and out['raw'].tolist() == [-1] * 3 and not out['hands'].any()
    assert not out['since'].any()
    kp, bb = group(STAND, STAND, STAND, STAND)
    bb[0, 4] = np.float32(0.3)
    kp[1, 7, 1] = np.nan                             # a wrist that is not even visible
    bb[2, 2] = np.inf
    out = h.frame(kp, bb, [1, 2, 3, 4])
    assert out['posture'].tolist() == [-1, -1, -1, UPRIGHT] and h.get('id')[:2].tolist() == [4, 0]


def one_slot(make):
    """max_tracks 1: a second id is dropped, counted, and gets -1; the slot is taken again once it has expired."""
    h = make(8, max_tracks=1, max_age=1, min_frames=1, **TWO)
    out = h.frame(*group(STAND, LIE), [11, 12])
    assert h.get('id').tolist() == [11] and h.get('dropped') == 1 and out['posture'].tolist() == [UPRIGHT, -1]
    out = h.frame(*LIE, [12])                        # 11 is away but not yet expired
    assert h.get('dropped') == 2 and out['posture'].tolist() == [-1] and h.get('now').tolist() == [0, 1, 0, 0, 0]
    out = h.frame(*LIE, [12])
    assert h.get('id').tolist() == [12] and h.get('dropped') == 2 and out['posture'].tolist() == [LYING]
    assert h.get('now').tolist() == [0, 0, 0, 0, 1] and int(out['n_events']) == 0


def more_events_than_rows(make):
    """max_events 2: three people fall in one frame: six events; n_events says 6, the table holds the first two of
    the fixed order and the counters count all three falls.  max_events 1: one row."""
    for rows in (2, 1):
        h = make(8, min_frames=1, max_events=rows, **TWO)
        h.frame(*group(STAND, STAND, STAND), [1, 2, 3])
        out = h.frame(*group(LIE, LIE, LIE), [1, 2, 3])
        assert int(out['n_events']) == 6 and out['events'].shape == (rows, 5)
        assert out['events'].tolist() == [[POSTURE, LYING, 1, 0, 2], [FALL, 1, 1, 0, 2]][:rows]
        assert h.get('falls') == 3


def garbage_is_never_read(make):
    """Whatever free slots hold, the outputs, the events and the live state are the same."""
    results = []
    for garbage in (False, True):
        h = make(8, max_tracks=3, min_frames=1, down_frames=1, **TWO)
        if garbage:
            for t in range(3):
                for f, v in (('last', -2 ** 31), ('posture', 77), ('since', 2 ** 31 - 1), ('upright', -5), ('streak', 2 ** 31 - 1),
                             ('alerted', -1), ('hands', -1), ('hand_streak', 2 ** 31 - 1)):
                    h.poke(f, (t,), v)
        outs = [h.frame(*STAND_UP, [2 ** 31 - 1]), h.frame(*LIE, [2 ** 31 - 1]), h.frame(*group(LIE, CROUCH), [2 ** 31 - 1, 8])]
        results.append((outs, [h.get(f)[:2].copy() for f in ('id', 'last', 'posture', 'since', 'upright', 'streak', 'alerted',
                                                             'hands', 'hand_streak')]))
    for a, b in zip(results[0][0], results[1][0]):
        assert all(np.array_equal(a[k], b[k]) for k in ('posture', 'raw', 'hands', 'since', 'events', 'n_events'))
    assert all((a == b).all() for a, b in zip(results[0][1], results[1][1]))
    assert ev(results[0][0][1]) == [(POSTURE, LYING, 2 ** 31 - 1, 0, 2), (FALL, 1, 2 ** 31 - 1, 0, 2),
                                    (HANDS_DOWN, 0, 2 ** 31 - 1, 0, 2)]
    assert ev(results[0][0][2]) == [(DOWN, 1, 2 ** 31 - 1, 0, 3)]


def two_cameras(make):
    """Two cameras keep their own clocks, slots and counters."""
    h = make(8, cameras=2, min_frames=1, **TWO)
    h.frame(*STAND, [1], camera=0)
    h.frame(*STAND, [1], camera=1)
    h.frame(*STAND, [1], camera=1)
    assert ev(h.frame(*LIE, [1], camera=1)) == [(POSTURE, LYING, 1, 0, 3), (FALL, 1, 1, 0, 3)]
    assert ev(h.frame(*CROUCH, [1], camera=0)) == [(POSTURE, LOW, 1, 0, 2)]
    assert h.get('now', 0).tolist() == [0, 0, 1, 0, 0] and h.get('now', 1).tolist() == [0, 0, 0, 0, 1]
    assert h.get('falls', 0) == 0 and h.get('falls', 1) == 1 and h.get('frame', 0) == 2 and h.get('frame', 1) == 3


SCRIPTS = [flat_threshold, lean_threshold, lying_wins, squat_threshold, hand_threshold, ends_of_the_range,
           visible_points_of_a_part, score_at_the_threshold, unknown_inside_a_streak, the_class_that_completes_the_streak,
           min_frames_one, fall_window_edges, born_lying, down_once_per_stay, hands_are_debounced, order_of_events,
           expiry_leaves_the_counters, duplicate_and_unusable, one_slot, more_events_than_rows, garbage_is_never_read,
           two_cameras]
