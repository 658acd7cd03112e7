"""Scenarios for the zone and line rule of DESIGN section 17 that the CPU and the GPU tests share: the edges of the rule
as small scripts with values worked out by hand.  A script drives a harness `make(K, **arguments)` with
  h.set_zones(zones, lines, dwell_frames=None, camera=0)
  h.frame(kpts, bboxes, ids, keep=None, camera=0) -> dict(zones, dwell, events, n_events) as numpy int32
  h.poke(field, index, value, camera=0)              a write into a camera's state
  h.get(field, camera=0)                             a camera's state or counter tensor as numpy
The CPU harness is the oracle alone; the GPU harness runs the device beside it and compares everything after every
frame, so the hand-worked values below hold for both.  Both call `invariant` after every frame.

Most scripts use K = 1 with anchor_kpts = (0,): the anchor of a pose is then its key point, 8 x in 1/8 pixel for a
key point at x pixels, and a vertex at x pixels is 8 x as well, so the scripts think in pixels."""
import math

import numpy as np

ENTER, EXIT, DWELL, APPEAR, VANISH, CROSS_FWD, CROSS_BACK = 1, 2, 3, 4, 5, 6, 7
ONE = dict(anchor_kpts=(0,))


def invariant(state, counts):
    """occupancy[z] == the live slots with bit z == entered + appeared - exited - vanished."""
    live = np.asarray(state['id']) != 0
    bits = np.asarray(state['inside'])[live]
    for z in range(8):
        n = int(((bits >> z) & 1).sum())
        flow = int(counts['entered'][z]) + int(counts['appeared'][z]) - int(counts['exited'][z]) - int(counts['vanished'][z])
        assert int(counts['occupancy'][z]) == n == flow, (z, int(counts['occupancy'][z]), n, flow)


def pts(*xy, score=0.9, box_score=0.8):
    """K = 1 poses with their key point at (x, y) pixels and a 10 x 20 box standing on it."""
    kp = np.asarray([[(x, y, score)] for x, y in xy], np.float32).reshape(-1, 1, 3)
    bb = np.asarray([(x - 5, y - 20, x + 5, y, box_score) for x, y in xy], np.float32).reshape(-1, 5)
    return kp, bb


def none(K=1):
    return np.zeros((0, K, 3), np.float32), np.zeros((0, 5), np.float32), np.zeros(0, np.int32)


def ev(out):
    """The stored events of a frame as tuples."""
    n = min(int(out['n_events']), len(out['events']))
    assert not out['events'][n:].any()
    return [tuple(int(v) for v in row) for row in out['events'][:n]]


SQUARE = [(10, 10), (20, 10), (20, 20), (10, 20)]


def points_on_the_boundary(make):
    """The square (10, 10) .. (20, 20), every pose born in one frame, so `zones` is the raw test.  An edge counts iff
    its ends are on different sides of `y > P.y`, so the horizontal edges never count, and of the vertical ones
    x = 20 (dy > 0) toggles iff P.x < 20 and x = 10 (dy < 0) iff P.x < 10 -- t = +-10 (P.x - x) 64 with nothing
    else in it.  Half-open: the left and top edges and the top-left vertex are inside, the right and bottom edges
    and the other three vertices are outside."""
    h = make(1, **ONE)
    h.set_zones([SQUARE], [])
    where = [(10, 10), (15, 10), (10, 15), (15, 15), (20, 15), (15, 20), (20, 20), (20, 10), (10, 20), (9.75, 15),
             (19.75, 19.75)]
    out = h.frame(*pts(*where), list(range(1, len(where) + 1)))
    assert out['zones'].tolist() == [1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 1]
    assert ev(out) == [(APPEAR, 0, d + 1, d, 1) for d in (0, 1, 2, 3, 10)]
    assert h.get('occupancy')[0] == 5 and h.get('appeared')[0] == 5
    assert h.get('pos')[4].tolist() == [160, 120] and h.get('pos')[9].tolist() == [78, 120]


def concave_polygon(make):
    """A U: the bar y in [0, 10) over the whole width and two legs x in [0, 10) and [20, 30) down to y = 30.  The
    notch between the legs is outside (two edges toggle), the bar above it inside."""
    h = make(1, **ONE)
    h.set_zones([[(0, 0), (30, 0), (30, 30), (20, 30), (20, 10), (10, 10), (10, 30), (0, 30)]], [])
    out = h.frame(*pts((5, 20), (15, 20), (25, 20), (15, 5), (15, 10), (35, 20), (10, 20), (20, 20)), [1, 2, 3, 4, 5, 6, 7, 8])
    # (15, 10) is on the notch's horizontal edge.  The edges with ends on different sides of y > 10 are x = 30 (dy > 0,
    # P.x < 30: toggles), x = 20 going up (dy < 0, t = (15 - 20)(-20) 64 > 0: toggles), x = 10 going down (dy > 0, t =
    # (15 - 10) 20 64 > 0: no) and x = 0 going up (dy < 0, t < 0: no): two toggles, outside.  (10, 20) is on the left
    # leg's right edge: outside; (20, 20) on the right leg's left edge: inside
    assert out['zones'].tolist() == [1, 0, 1, 1, 0, 0, 0, 1]


def sixteen_vertices(make):
    """A regular 16-gon of radius 50 about (100, 100), its first vertex at angle 0: the apothem is 50 cos(pi / 16)
    = 49.04, so along a vertex's direction 49.5 is inside and along an edge's middle (angle pi / 16) it is
    outside, where 48.5 is inside."""
    h = make(1, **ONE)
    ring = [(100 + 50 * math.cos(i * math.pi / 8), 100 + 50 * math.sin(i * math.pi / 8)) for i in range(16)]
    h.set_zones([SQUARE, ring], [])
    mid = math.pi / 16
    q = lambda r, a: (round(4 * (100 + r * math.cos(a))) / 4, round(4 * (100 + r * math.sin(a))) / 4)
    out = h.frame(*pts((100, 100), q(49.5, 0), q(49.5, mid), q(48.5, mid), (160, 100), q(49.5, 9 * mid), q(48.5, 9 * mid),
                       q(49.5, math.pi)), list(range(1, 9)))
    assert out['zones'].tolist() == [2, 2, 0, 2, 0, 0, 2, 2]
    assert h.get('appeared').tolist()[:2] == [0, 5]


def fig15(ankles, box=(80, 100, 120, 200), scores=(0.9, 0.9)):
    """A K = 15 pose whose ankles (key points 13, 14) are at `ankles` (quarter pixels), everything else at (1, 1)."""
    kp = np.ones((1, 15, 3), np.float32)
    for k, (x, y), s in zip((13, 14), ankles, scores):
        kp[0, k] = (x / 4.0, y / 4.0, s)
    return kp, np.asarray([[v / 4.0 for v in box] + [0.8]], np.float32)


def anchors(make):
    """K = 15, 'feet': two ankles at quarter pixels (100, 200), (101, 203): floor(2 (201) / 2) = 201 and 403; one
    visible: twice its X; none: the bottom centre of the box (X1 + X2, 2 Y2).  Three anchor key points with sum
    301, 604: floor(602 / 3) = 200 and floor(1208 / 3) = 402.  'box' and 'centre' never look at key points."""
    both = ((100, 200), (101, 203))
    for kw, scores, want in ((dict(), (0.9, 0.9), [201, 403]), (dict(), (0.9, 0.0), [200, 400]),
                             (dict(), (-1.0, 0.9), [202, 406]), (dict(), (0.0, 0.0), [200, 400]),
                             (dict(kpt_thr=0.9), (0.9, 0.9), [200, 400]),
                             (dict(anchor='box'), (0.9, 0.9), [200, 400]),
                             (dict(anchor='centre'), (0.9, 0.9), [200, 300])):
        h = make(15, **kw)
        h.frame(*fig15(both, scores=scores), [1])
        assert h.get('pos')[0].tolist() == want, (kw, scores)
    h = make(15, anchor_kpts=(0, 13, 14))
    kp, bb = fig15(both)
    kp[0, 0] = (25.0, 50.25, 0.9)                    # X = (100, 201)
    h.frame(kp, bb, [1])
    assert h.get('pos')[0].tolist() == [200, 402]
    # the fallback of the second row is the box, not an ankle that is not seen: a box elsewhere shows it
    h = make(15)
    h.frame(*fig15(both, box=(0, 0, 40, 90), scores=(0.0, 0.0)), [1])
    assert h.get('pos')[0].tolist() == [40, 180]


LINE = ((50, 0), (50, 100))      # downwards: s(P) = -800 * 8 (P.x - 50) >= 0 iff P.x <= 50: the line itself is on the true side


def crossings_on_and_off_the_line(make):
    """60 -> 50 ends on the line: s false -> true, forward.  50 -> 40 starts on it: true -> true, nothing.  40 -> 50:
    nothing; 50 -> 60 starts on it: true -> false, backward.  So a walk over the line counts once either way.  A
    move at y = 150, beyond B: the sides of Q and P differ but A and B are on one side of Q -> P: no crossing.  A
    pose that stands still (Q == P) crosses nothing."""
    h = make(1, **ONE)
    h.set_zones([], [LINE])
    got = []
    for x in (60, 50, 40, 40, 50, 60):
        got.append(ev(h.frame(*pts((x, 50)), [7])))
    assert got == [[], [(CROSS_FWD, 0, 7, 0, 2)], [], [], [], [(CROSS_BACK, 0, 7, 0, 6)]]
    assert h.get('crossed')[0].tolist() == [1, 1]
    for x in (40, 60, 40):
        assert ev(h.frame(*pts((x, 150)), [8])) == []
    assert h.get('crossed')[0].tolist() == [1, 1]
    # exactly through the end B: Q = (40, 100), P = (60, 100): side(A) = cross((20, 0), (10, -100)) < 0 is false,
    # side(B) = cross((20, 0), (10, 0)) = 0 is true: a crossing, backward
    h.frame(*pts((40, 100)), [9])
    assert ev(h.frame(*pts((60, 100)), [9])) == [(CROSS_BACK, 0, 9, 0, 11)]
    # and through A the other way: Q = (60, 0), P = (40, 0): side(A) = cross((-20, 0), (-10, 0)) = 0 true, side(B) =
    # cross((-20, 0), (-10, 100)) = -2000 * 64 false: forward
    h.frame(*pts((60, 0)), [10])
    assert ev(h.frame(*pts((40, 0)), [10])) == [(CROSS_FWD, 0, 10, 0, 13)]
    assert h.get('crossed')[0].tolist() == [2, 2]


def two_lines_in_one_move(make):
    """One move over two lines of opposite direction: events in ascending line index, one forward, one backward."""
    h = make(1, **ONE)
    h.set_zones([], [LINE, ((70, 100), (70, 0))])
    h.frame(*pts((40, 50)), [3])
    assert ev(h.frame(*pts((90, 50)), [3])) == [(CROSS_BACK, 0, 3, 0, 2), (CROSS_FWD, 1, 3, 0, 2)]
    assert h.get('crossed')[:2].tolist() == [[0, 1], [1, 0]]


def gaps_and_rebirth(make):
    """max_age 3: a track seen in frame 1 and again in frame 4 (gap 3) is the same slot and its move spans the gap: it
    left the zone x < 45 and crossed the line at x = 50 in one move.  Seen in frame 5 and then in frame 9 (gap 4)
    it has expired: VANISH for the zone it was in, then a birth on the far side: no crossing and no EXIT."""
    h = make(1, max_age=3, min_frames=1, **ONE)
    h.set_zones([[(0, 0), (45, 0), (45, 100), (0, 100)]], [LINE])
    assert ev(h.frame(*pts((40, 50)), [5])) == [(APPEAR, 0, 5, 0, 1)]
    h.frame(*none())
    h.frame(*none())
    assert ev(h.frame(*pts((60, 50)), [5])) == [(EXIT, 0, 5, 0, 4), (CROSS_BACK, 0, 5, 0, 4)]
    assert ev(h.frame(*pts((40, 50)), [5])) == [(ENTER, 0, 5, 0, 5), (CROSS_FWD, 0, 5, 0, 5)]
    for _ in range(3):
        assert ev(h.frame(*none())) == [] and h.get('id')[0] == 5
    out = h.frame(*pts((60, 50)), [5])
    assert ev(out) == [(VANISH, 0, 5, -1, 9)] and out['zones'].tolist() == [0] and h.get('last')[0] == 9
    assert h.get('crossed')[0].tolist() == [1, 1] and h.get('exited')[0] == 1 and h.get('vanished')[0] == 1


def expiry_and_rebirth(make):
    """max_age 2: seen in frame 1 inside two zones, then not for three frames: frame 4 frees the slot (4 - 1 > 2) with
    a VANISH per zone in ascending order and pose -1; the id comes back on the far side of the line in frame 5: a
    birth (APPEAR where it is now), no crossing."""
    h = make(1, max_age=2, **ONE)
    big = [(0, 0), (100, 0), (100, 100), (0, 100)]
    h.set_zones([big, [(30, 30), (45, 30), (45, 70), (30, 70)], [(55, 0), (100, 0), (100, 100), (55, 100)]], [LINE])
    assert ev(h.frame(*pts((40, 50)), [9])) == [(APPEAR, 0, 9, 0, 1), (APPEAR, 1, 9, 0, 1)]
    assert ev(h.frame(*none())) == [] and ev(h.frame(*none())) == []
    assert h.get('occupancy')[:3].tolist() == [1, 1, 0]
    assert ev(h.frame(*none())) == [(VANISH, 0, 9, -1, 4), (VANISH, 1, 9, -1, 4)]
    assert h.get('id')[0] == 0 and h.get('vanished')[:3].tolist() == [1, 1, 0] and h.get('occupancy')[:3].tolist() == [0, 0, 0]
    out = h.frame(*pts((60, 50)), [9])
    assert ev(out) == [(APPEAR, 0, 9, 0, 5), (APPEAR, 2, 9, 0, 5)] and out['zones'].tolist() == [5]
    assert h.get('crossed').sum() == 0 and h.get('appeared')[:3].tolist() == [2, 1, 1]
    # a VANISH and the events of poses in one frame: VANISH first
    h.frame(*none())
    h.frame(*none())
    assert ev(h.frame(*pts((40, 50)), [4])) == [(VANISH, 0, 9, -1, 8), (VANISH, 2, 9, -1, 8), (APPEAR, 0, 4, 0, 8),
                                                (APPEAR, 1, 4, 0, 8)]


def debounce(make):
    """min_frames 3: born outside; two raw frames inside and one outside again: streak 1, 2, 0 and no flip, one frame
    short.  Three in a row: ENTER on the third, since = that frame.  min_frames 1: the bit is the raw test."""
    h = make(1, min_frames=3, **ONE)
    h.set_zones([SQUARE], [])
    seen = []
    for x in (5, 15, 15, 5, 15, 15, 15, 5, 5, 15, 5, 5, 5):
        out = h.frame(*pts((x, 15)), [2])
        seen.append((int(out['zones'][0]), int(h.get('streak')[0, 0]), ev(out)))
    assert [s[:2] for s in seen] == [(0, 0), (0, 1), (0, 2), (0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (1, 2), (1, 0),
                                     (1, 1), (1, 2), (0, 0)]
    assert [s[2] for s in seen if s[2]] == [[(ENTER, 0, 2, 0, 7)], [(EXIT, 0, 2, 0, 13)]]
    assert h.get('since')[0, 0] == 7
    h = make(1, min_frames=1, **ONE)
    h.set_zones([SQUARE], [])
    bits = [int(h.frame(*pts((x, 15)), [2])['zones'][0]) for x in (5, 15, 5, 15, 15)]
    assert bits == [0, 1, 0, 1, 1] and h.get('entered')[0] == 2 and h.get('exited')[0] == 1


def dwell_once_per_stay(make):
    """dwell_frames 2, min_frames 1: born inside in frame 1 (since 1); frame 3 is 2 frames in: DWELL, once; not again
    in frames 4 and 5; EXIT in 6 clears the alert; ENTER in 7 (since 7), DWELL again in 9.  `dwell` counts the frames
    inside and is 0 outside.  A zone with dwell_frames 0 never reports."""
    h = make(1, min_frames=1, **ONE)
    h.set_zones([SQUARE, [(0, 0), (100, 0), (100, 100), (0, 100)]], [], dwell_frames=[2, 0])
    got, dwell = [], []
    for x in (15, 15, 15, 15, 15, 5, 15, 15, 15, 15):
        out = h.frame(*pts((x, 15)), [6])
        got.append([e for e in ev(out) if e[1] == 0])
        dwell.append(out['dwell'][0, :2].tolist())
    assert got == [[(APPEAR, 0, 6, 0, 1)], [], [(DWELL, 0, 6, 0, 3)], [], [], [(EXIT, 0, 6, 0, 6)], [(ENTER, 0, 6, 0, 7)], [],
                   [(DWELL, 0, 6, 0, 9)], []]
    assert dwell == [[0, 0], [1, 1], [2, 2], [3, 3], [4, 4], [0, 5], [0, 6], [1, 7], [2, 8], [3, 9]]
    assert h.get('alerted')[0] == 1


def duplicate_and_unusable_ids(make):
    """Of two valid poses with one id the first takes part and the second gets zeros; a pose that is not valid does
    not count as the first; ids <= 0 take no slot."""
    h = make(1, **ONE)
    h.set_zones([SQUARE], [])
    out = h.frame(*pts((15, 15), (16, 16)), [7, 7])
    assert out['zones'].tolist() == [1, 0] and h.get('id')[:2].tolist() == [7, 0] and h.get('pos')[0].tolist() == [120, 120]
    out = h.frame(*pts((15, 15), (16, 16), (17, 17)), [7, 7, 5], keep=[0, 1, 1])
    assert out['zones'].tolist() == [0, 1, 1] and h.get('pos')[0].tolist() == [128, 128] and h.get('id')[:3].tolist() == [7, 5, 0]
    h = make(1, **ONE)
    h.set_zones([SQUARE], [])
    out = h.frame(*pts((15, 15), (15, 15), (15, 15)), [0, -3, -(2 ** 31)])
    assert not h.get('id').any() and h.get('dropped') == 0 and h.get('frame') == 1 and int(out['n_events']) == 0
    assert not out['zones'].any() and not out['dwell'].any()
    # not valid: a score at the threshold, a NaN key point that is not an anchor's business but makes the pose
    # unusable, an infinite box corner
    kp, bb = pts((15, 15), (15, 15), (15, 15), (15, 15))
    bb[0, 4] = np.float32(0.3)
    kp[1, 0, 0] = np.nan
    bb[2, 2] = np.inf
    out = h.frame(kp, bb, [1, 2, 3, 4])
    assert out['zones'].tolist() == [0, 0, 0, 1] and h.get('id')[:2].tolist() == [4, 0]


def two_slots(make):
    """S = 2: a third id is dropped and gets zeros; an expired slot is taken again, the lowest first."""
    h = make(1, max_tracks=2, max_age=1, **ONE)
    h.set_zones([SQUARE], [])
    out = h.frame(*pts((15, 15), (15, 15), (15, 15)), [11, 12, 13])
    assert h.get('id').tolist() == [11, 12] and h.get('dropped') == 1 and out['zones'].tolist() == [1, 1, 0]
    assert int(out['n_events']) == 2
    out = h.frame(*pts((15, 15), (15, 15)), [13, 12])       # 11 is away but not yet expired: 13 finds no slot
    assert h.get('id').tolist() == [11, 12] and h.get('dropped') == 2 and out['zones'].tolist() == [0, 1]
    out = h.frame(*pts((15, 15), (15, 15)), [13, 12])       # slot 0 is free now
    assert ev(out) == [(VANISH, 0, 11, -1, 3), (APPEAR, 0, 13, 0, 3)]
    assert h.get('id').tolist() == [13, 12] and h.get('dropped') == 2 and h.get('last').tolist() == [3, 3]


def more_events_than_rows(make):
    """max_events 2: three poses born inside two zones are six events; n_events says 6 and the table holds the first
    two of the fixed order; the counters count all six."""
    h = make(1, max_events=2, **ONE)
    big = [(0, 0), (100, 0), (100, 100), (0, 100)]
    h.set_zones([SQUARE, big], [])
    out = h.frame(*pts((15, 15), (15, 15), (15, 15)), [1, 2, 3])
    assert int(out['n_events']) == 6 and out['events'].shape == (2, 5)
    assert out['events'].tolist() == [[APPEAR, 0, 1, 0, 1], [APPEAR, 1, 1, 0, 1]]
    assert h.get('appeared')[:2].tolist() == [3, 3]
    h = make(1, max_events=1, max_age=0, **ONE)
    h.set_zones([SQUARE, big], [])
    h.frame(*pts((15, 15)), [1])
    out = h.frame(*pts((50, 50)), [2])                      # max_age 0: id 1 expires at once: VANISH rows come first
    assert int(out['n_events']) == 3 and out['events'].tolist() == [[VANISH, 0, 1, -1, 2]]


def set_zones_resets_its_camera_only(make):
    """Two cameras with tracks; set_zones(1) frees camera 1's slots and zeroes its clock and counters, without
    events, and leaves camera 0 as it is."""
    h = make(1, cameras=2, **ONE)
    h.set_zones([SQUARE], [LINE], camera=0)
    h.set_zones([SQUARE], [], camera=1)
    for c in (0, 1):
        h.frame(*pts((15, 15)), [3 + c], camera=c)
        h.frame(*pts((15, 15)), [3 + c], camera=c)
    before = {f: h.get(f, 0).copy() for f in ('id', 'last', 'pos', 'inside', 'since', 'frame', 'occupancy', 'appeared')}
    h.set_zones([[(0, 0), (5, 0), (5, 5)]], [], camera=1)
    for f in ('id', 'frame', 'dropped', 'occupancy', 'appeared'):
        assert not np.asarray(h.get(f, 1)).any(), f
    for f, v in before.items():
        assert (h.get(f, 0) == v).all(), f
    out = h.frame(*pts((15, 15)), [4], camera=1)            # born again, outside the new triangle
    assert out['zones'].tolist() == [0] and h.get('frame', 1) == 1 and int(out['n_events']) == 0
    out = h.frame(*pts((60, 15)), [3], camera=0)
    assert ev(out) == [(CROSS_BACK, 0, 3, 0, 3)] and h.get('frame', 0) == 3    # (EXIT needs a second frame)


def camera_without_geometry(make):
    """A camera that was never configured has no zones and no lines: slots are still kept, nothing is reported."""
    h = make(1, max_tracks=1, **ONE)
    out = h.frame(*pts((15, 15), (16, 16)), [1, 2])
    assert int(out['n_events']) == 0 and h.get('id').tolist() == [1] and h.get('dropped') == 1
    assert h.get('pos')[0].tolist() == [120, 120] and not out['zones'].any()


def garbage_is_never_read(make):
    """Whatever free slots hold, the outputs, the events and the live state are the same."""
    results = []
    for garbage in (False, True):
        h = make(1, max_tracks=3, min_frames=1, **ONE)
        h.set_zones([SQUARE], [LINE], dwell_frames=[1])
        if garbage:
            for t in range(3):
                for f, v in (('pos', (-2 ** 31, 2 ** 31 - 1)), ('last', -2 ** 31), ('inside', -1), ('alerted', -1)):
                    h.poke(f, (t,), v)
                h.poke('streak', (t,), np.full(8, 2 ** 31 - 1, np.int64))
                h.poke('since', (t,), np.full(8, -2 ** 31, np.int64))
        outs = [h.frame(*pts((15, 15)), [2 ** 31 - 1]), h.frame(*pts((60, 15)), [2 ** 31 - 1]),
                h.frame(*pts((15, 15), (15, 16)), [2 ** 31 - 1, 8])]
        results.append((outs, [h.get(f)[:2].copy() for f in ('id', 'last', 'pos', 'inside', 'alerted', 'streak', 'since')]))
    for a, b in zip(results[0][0], results[1][0]):
        assert all(np.array_equal(a[k], b[k]) for k in ('zones', 'dwell', 'events', 'n_events'))
    assert all((a == b).all() for a, b in zip(results[0][1], results[1][1]))
    assert ev(results[0][0][2]) == [(ENTER, 0, 2 ** 31 - 1, 0, 3), (CROSS_FWD, 0, 2 ** 31 - 1, 0, 3), (APPEAR, 0, 8, 1, 3)]


SCRIPTS = [points_on_the_boundary, concave_polygon, sixteen_vertices, anchors, crossings_on_and_off_the_line,
           two_lines_in_one_move, gaps_and_rebirth, expiry_and_rebirth, debounce, dwell_once_per_stay,
           duplicate_and_unusable_ids, two_slots, more_events_than_rows, set_zones_resets_its_camera_only,
           camera_without_geometry, garbage_is_never_read]
