"""Scenarios for the footfall-map rule of DESIGN section 21 that the CPU and the GPU tests share: the edges of the rule
as small scripts with values worked out by hand.  A script drives a harness `make(K, **arguments)` with
  h.frame(kpts, bboxes, ids, entries, keep=None, camera=0) -> dict(cell, dwell, visits) as numpy int32;
                                                     entries: the cell entries (visits) the script counts in the frame
  h.get(field, camera=0)                             dwell, visits, peak, id, last, cell, frame, dropped as numpy
The CPU harness is the oracle alone; the GPU harness runs the device beside it and compares everything after every
frame, so the hand-worked values below hold for both.  Both call `invariant` after every frame.

The scripts use a 64 x 48 picture at cell 8 (a grid of 8 x 6) and K = 1 with anchor_kpts = (0,): the anchor of a pose
is then its key point, 8 x in 1/8 pixel for a key point at x pixels, and its cell is (x // 8, y // 8)."""
import numpy as np

SIZE, CELL, GW, GH = (64, 48), 8, 8, 6
ONE = dict(anchor_kpts=(0,), size=SIZE, cell=CELL)


def invariant(before, after, out, radius, forgot, entries):
    """before, after: dict(dwell, visits, peak) around one frame; out: the frame's outputs.  peak[m] is the maximum of
    map m; without forgetting, the dwell sum grows by (radius + 1)^4 per on-map pose whose footprint is clear of the
    border (and by less for one at the border), and the visits sum by the entries the script counted."""
    assert int(after['peak'][0]) == int(after['dwell'].max()) and int(after['peak'][1]) == int(after['visits'].max())
    if forgot:
        return
    Gh, Gw = after['dwell'].shape
    on = out['cell'][out['cell'] >= 0]
    gx, gy = on % Gw, on // Gw
    clear = (gx >= radius) & (gx + radius < Gw) & (gy >= radius) & (gy + radius < Gh)
    grown = int(after['dwell'].astype(np.int64).sum() - before['dwell'].astype(np.int64).sum())
    full = (radius + 1) ** 4
    if clear.all():
        assert grown == full * len(on), (grown, len(on))
    else:
        assert full * int(clear.sum()) < grown < full * len(on), (grown, len(on))
    assert int(after['visits'].astype(np.int64).sum() - before['visits'].astype(np.int64).sum()) == entries


def pts(*xy, score=0.9, box_score=0.8):
    """K = 1 poses with their key point at (x, y) pixels and a 10 x 20 box standing on it."""
    kp = np.asarray([[(x, y, score)] for x, y in xy], np.float32).reshape(-1, 1, 3)
    bb = np.asarray([(x - 5, y - 20, x + 5, y, box_score) for x, y in xy], np.float32).reshape(-1, 5)
    return kp, bb


def none(K=1):
    return np.zeros((0, K, 3), np.float32), np.zeros((0, 5), np.float32), np.zeros(0, np.int32)


def standing(make):
    """One pose standing three frames at (20, 20), cell (2, 2) = index 18, radius 0: dwell 3, visits 1."""
    h = make(1, radius=0, **ONE)
    outs = [h.frame(*pts((20, 20)), [4], entries=1 if f == 0 else 0) for f in range(3)]
    assert [int(o['cell'][0]) for o in outs] == [18, 18, 18]
    assert [int(o['dwell'][0]) for o in outs] == [1, 2, 3] and [int(o['visits'][0]) for o in outs] == [1, 1, 1]
    assert h.get('dwell')[2, 2] == 3 and h.get('dwell').sum() == 3
    assert h.get('visits')[2, 2] == 1 and h.get('visits').sum() == 1
    assert h.get('peak').tolist() == [3, 1] and h.get('cell')[0] == 18 and h.get('frame') == 3


def step_and_back(make):
    """A step into the next cell and back: the visits at the pose's cell are 1, 1 and then 2."""
    h = make(1, radius=0, **ONE)
    seen = [int(h.frame(*pts((x, 20)), [4], entries=1)['visits'][0]) for x in (20, 28, 20)]
    assert seen == [1, 1, 2]
    assert h.get('visits')[2, 2] == 2 and h.get('visits')[2, 3] == 1 and h.get('visits').sum() == 3
    assert h.get('dwell')[2, 2] == 2 and h.get('dwell')[2, 3] == 1 and h.get('peak').tolist() == [2, 2]


def a_gap_longer_than_max_age(make):
    """max_age 2: seen in frame 1 and again in frame 3 (3 - 1 = 2 is not > 2): the same slot in the same cell, no new
    visit.  Then not for three frames: frame 6 frees the slot (6 - 3 > 2), and frame 7 is a birth: a second visit."""
    h = make(1, radius=0, max_age=2, **ONE)
    assert h.frame(*pts((20, 20)), [9], entries=1)['visits'].tolist() == [1]
    h.frame(*none(), entries=0)
    assert h.frame(*pts((20, 20)), [9], entries=0)['visits'].tolist() == [1]
    for f in (4, 5, 6):
        h.frame(*none(), entries=0)
        assert h.get('id')[0] == (9 if f < 6 else 0)
    assert h.frame(*pts((20, 20)), [9], entries=1)['visits'].tolist() == [2]
    assert h.get('dwell')[2, 2] == 3 and h.get('last')[0] == 7


def who_takes_no_part(make):
    """A duplicate id, an id of 0, keep = 0, a score at the threshold, NaN and inf coordinates add nothing."""
    h = make(1, radius=0, **ONE)
    kp, bb = pts((20, 20), (30, 20), (20, 30), (20, 30), (20, 30), (20, 30), (20, 30))
    bb[4, 4] = np.float32(0.3)
    kp[5, 0, 0] = np.nan
    bb[6, 2] = np.inf
    out = h.frame(kp, bb, [7, 7, 0, 3, 4, 5, 6], entries=1, keep=[1, 1, 1, 0, 1, 1, 1])
    assert out['cell'].tolist() == [18, -1, -1, -1, -1, -1, -1]
    assert out['dwell'].tolist() == [1, 0, 0, 0, 0, 0, 0] and out['visits'].tolist() == [1, 0, 0, 0, 0, 0, 0]
    assert h.get('dwell').sum() == 1 and h.get('id')[:2].tolist() == [7, 0] and h.get('dropped') == 0
    # a pose that is not valid is not the first of its id: the second one takes part
    out = h.frame(*pts((30, 20), (20, 20)), [7, 7], entries=0, keep=[0, 1])
    assert out['cell'].tolist() == [-1, 18] and h.get('dwell')[2, 2] == 2


def pts2(a, b):
    """One K = 2 pose with its key points at a and b (pixels): with anchor_kpts (0, 1) its anchor is X(a) + X(b) in
    1/8 pixel, X in quarter pixels."""
    kp = np.asarray([[(a[0], a[1], 0.9), (b[0], b[1], 0.9)]], np.float32)
    return kp, np.asarray([[1, 1, 9, 9, 0.8]], np.float32)


def the_last_eighth_of_a_pixel(make):
    """Width 64: an anchor at 8 * 64 - 1 = 511 (quarter pixels 255 + 256) is on the map, in the last column, and one
    at 512 is off it; height 48: 383 (191 + 192) is on, 384 is off."""
    h = make(2, radius=0, anchor_kpts=(0, 1), size=SIZE, cell=CELL)
    out = h.frame(*pts2((63.75, 20), (64, 20)), [1], entries=1)
    assert out['cell'].tolist() == [2 * GW + 7]
    out = h.frame(*pts2((64, 20), (64, 20)), [1], entries=0)
    assert out['cell'].tolist() == [-1] and h.get('cell')[0] == -1
    out = h.frame(*pts2((20, 47.75), (20, 48)), [2], entries=1)
    assert out['cell'].tolist() == [5 * GW + 2]
    out = h.frame(*pts2((20, 48), (20, 48)), [2], entries=0)
    assert out['cell'].tolist() == [-1] and h.get('dwell').sum() == 2
    out = h.frame(*pts2((0, 0), (0, 0)), [3], entries=1)
    assert out['cell'].tolist() == [0]


def off_the_map_and_back(make):
    """A pose that takes part off the map adds nothing and its slot forgets its cell: coming back counts a visit."""
    h = make(1, radius=0, **ONE)
    h.frame(*pts((20, 20)), [4], entries=1)
    out = h.frame(*pts((70, 20)), [4], entries=0)
    assert out['cell'].tolist() == [-1] and out['dwell'].tolist() == [0] and out['visits'].tolist() == [0]
    assert h.get('cell')[0] == -1 and h.get('last')[0] == 2 and h.get('dwell').sum() == 1
    out = h.frame(*pts((20, 20)), [4], entries=1)
    assert out['visits'].tolist() == [2] and out['dwell'].tolist() == [2]


def radius_three_in_a_corner(make):
    """radius 3 at cell (0, 0): the 16 cells dx, dy in 0 .. 3 keep (4 - dx)(4 - dy), 100 of the 256 in all."""
    h = make(1, radius=3, **ONE)
    h.frame(*pts((2, 2)), [1], entries=1)
    want = np.zeros((GH, GW), np.int64)
    want[:4, :4] = np.outer([4, 3, 2, 1], [4, 3, 2, 1])
    assert (h.get('dwell') == want).all() and h.get('dwell').sum() == 100 and h.get('peak').tolist() == [16, 1]
    # and the opposite corner, cell (7, 5)
    h.frame(*pts((63, 47)), [2], entries=1)
    assert h.get('dwell')[5, 7] == 16 and h.get('dwell')[2, 4] == 1 and h.get('dwell').sum() == 200


def half_life_two(make):
    """half_life 2, radius 1, one pose standing five frames: the centre gains 4, an edge cell 2, a corner 1 per frame,
    and frames 2 and 4 halve first: centre 4, 2 + 4 = 6, 10, 5 + 4 = 9, 13; edge 2, 1 + 2 = 3, 5, 2 + 2 = 4, 6 (5 >> 1
    = 2: an odd value); corner 1, 0 + 1 = 1, 2, 1 + 1 = 2, 3.  The visit of frame 1 is halved away in frame 2."""
    h = make(1, radius=1, half_life=2, **ONE)
    seen = []
    for f in range(5):
        out = h.frame(*pts((20, 20)), [4], entries=1 if f == 0 else 0)
        d = h.get('dwell')
        seen.append((int(d[2, 2]), int(d[2, 3]), int(d[1, 1]), int(out['dwell'][0]), int(out['visits'][0]),
                     h.get('peak').tolist()))
    assert seen == [(4, 2, 1, 4, 1, [4, 1]), (6, 3, 1, 6, 0, [6, 0]), (10, 5, 2, 10, 0, [10, 0]), (9, 4, 2, 9, 0, [9, 0]),
                    (13, 6, 3, 13, 0, [13, 0])]


def slots_full(make):
    """max_tracks 2: a third id finds no slot, is counted in dropped, gets -1 and zeros and adds nothing."""
    h = make(1, radius=0, max_tracks=2, **ONE)
    out = h.frame(*pts((20, 20), (20, 20), (20, 20)), [11, 12, 13], entries=2)
    assert out['cell'].tolist() == [18, 18, -1] and out['dwell'].tolist() == [2, 2, 0] and out['visits'].tolist() == [2, 2, 0]
    assert h.get('id').tolist() == [11, 12] and h.get('dropped') == 1 and h.get('dwell')[2, 2] == 2


SCRIPTS = [standing, step_and_back, a_gap_longer_than_max_age, who_takes_no_part, the_last_eighth_of_a_pixel,
           off_the_map_and_back, radius_three_in_a_corner, half_life_two, slots_full]
