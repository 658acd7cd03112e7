"""Scenarios for the track-trail rule of DESIGN section 22 that the CPU and the GPU tests share: the edges of the rule
as small scripts with values worked out by hand.  A script drives a harness `make(K, **arguments)` with
  h.frame(kpts, bboxes, ids, keep=None, camera=0) -> dict(count, span, dist, path) as numpy int32
  h.get(field, camera=0)          id, last, pos, head, count, box, pts, when, frame, dropped as numpy
The CPU harness is the oracle alone; the GPU harness runs the device beside it and compares everything after every
frame, so the hand-worked values below hold for both.  Both call `invariant` after every frame.

The scripts use K = 1 with anchor_kpts = (0,): the anchor of a pose is then its key point, 8 x in 1/8 pixel for a key
point at x pixels."""
import numpy as np

from tests.heat_cases import none, pts
from tests.trail_ref import committed, measures

ONE = dict(anchor_kpts=(0,))


def invariant(views, L, stride, min_step, out, ids):
    """views: dict(id, last, pos, head, count, box, pts, when, frame) of one camera after a frame; out: the frame's
    outputs; ids: the frame's ids.  count <= L; consecutive committed points are at least min_step apart (Chebyshev)
    and at least stride frames; box contains every committed point and pos; span, dist and path of every pose that takes
    part are what the ring gives."""
    frame = int(views['frame'])
    for t in np.nonzero(views['id'])[0]:
        assert 1 <= int(views['count'][t]) <= L and 0 <= int(views['head'][t]) < L
        ring = committed(views['pts'][t], views['when'][t], views['head'][t], views['count'][t])
        for a, b in zip(ring, ring[1:]):
            assert max(abs(a[0] - b[0]), abs(a[1] - b[1])) >= min_step and b[2] - a[2] >= stride, (a, b)
        x0, y0, x1, y1 = (int(v) for v in views['box'][t])
        for x, y in [p[:2] for p in ring] + [tuple(int(v) for v in views['pos'][t])]:
            assert x0 <= x <= x1 and y0 <= y <= y1, (x, y, views['box'][t])
        assert ring[-1][2] <= int(views['last'][t]) <= frame
    ids = np.asarray(ids).reshape(-1)
    for d in np.nonzero(out['count'])[0]:
        t = int(np.nonzero(views['id'] == ids[d])[0][0])
        ring = committed(views['pts'][t], views['when'][t], views['head'][t], views['count'][t])
        assert tuple(int(out[k][d]) for k in ('count', 'span', 'dist', 'path')) == measures(ring, views['pos'][t], frame)
    for k in ('span', 'dist', 'path'):
        assert not out[k][out['count'] == 0].any()


def row(out, d=0):
    return tuple(int(out[k][d]) for k in ('count', 'span', 'dist', 'path'))


def standing(make):
    """One pose standing three frames at (20, 20): one committed point, the birth's; the span grows, nothing else."""
    h = make(1, **ONE)
    assert [row(h.frame(*pts((20, 20)), [4])) for _ in range(3)] == [(1, 0, 0, 0), (1, 1, 0, 0), (1, 2, 0, 0)]
    assert h.get('pts')[0, 0].tolist() == [160, 160] and h.get('when')[0, 0] == 1 and h.get('head')[0] == 0
    assert h.get('box')[0].tolist() == [160, 160, 160, 160] and h.get('pos')[0].tolist() == [160, 160]


def walking(make):
    """5 pixels = 40 eighths per frame along x: a commit per frame; dist and path are the distance walked."""
    h = make(1, **ONE)
    assert [row(h.frame(*pts((20 + 5 * f, 20)), [4])) for f in range(3)] == [(1, 0, 0, 0), (2, 1, 40, 40), (3, 2, 80, 80)]
    assert h.get('pts')[0, :3].tolist() == [[160, 160], [200, 160], [240, 160]] and h.get('when')[0, :3].tolist() == [1, 2, 3]
    assert h.get('head')[0] == 2 and h.get('box')[0].tolist() == [160, 160, 240, 160]


def the_step_that_commits(make):
    """min_step 16: 1.75 pixels = 14 eighths from the newest committed point is not committed -- the line still ends at
    pos: dist and path 14 -- and 2 pixels = 16 is, measured from the committed point and not from the frame before."""
    h = make(1, min_step=16, **ONE)
    h.frame(*pts((20, 20)), [4])
    assert row(h.frame(*pts((21.75, 20)), [4])) == (1, 1, 14, 14) and h.get('pos')[0].tolist() == [174, 160]
    assert h.get('box')[0].tolist() == [160, 160, 174, 160]
    assert row(h.frame(*pts((22, 20)), [4])) == (2, 2, 16, 16) and h.get('pts')[0, 1].tolist() == [176, 160]
    # Chebyshev: 14 in x and 16 in y commits
    assert row(h.frame(*pts((23.75, 22)), [4])) == (3, 3, 34, 37)          # isqrt(30^2 + 16^2) = 34; 16 + isqrt(14^2 + 16^2) = 16 + 21


def every_third_frame(make):
    """stride 3: born in frame 1, the next commit is in frame 4 (4 - 1 >= 3) and then in frame 7; between them the path
    runs from the newest committed point straight to pos."""
    h = make(1, stride=3, **ONE)
    rows = [row(h.frame(*pts((20 + 5 * f, 20)), [4])) for f in range(7)]
    assert rows == [(1, 0, 0, 0), (1, 1, 40, 40), (1, 2, 80, 80), (2, 3, 120, 120), (2, 4, 160, 160), (2, 5, 200, 200),
                    (3, 6, 240, 240)]
    assert h.get('when')[0, :3].tolist() == [1, 4, 7] and h.get('pts')[0, :3, 0].tolist() == [160, 280, 400]


def a_ring_of_two(make):
    """length 2: the third commit overwrites the first; count stays 2 and the oldest point is one commit back."""
    h = make(1, length=2, **ONE)
    rows = [row(h.frame(*pts((20 + 5 * f, 20)), [4])) for f in range(5)]
    assert rows == [(1, 0, 0, 0), (2, 1, 40, 40), (2, 1, 40, 40), (2, 1, 40, 40), (2, 1, 40, 40)]
    assert h.get('head')[0] == 0 and h.get('pts')[0].tolist() == [[320, 160], [280, 160]] and h.get('when')[0].tolist() == [5, 4]
    assert h.get('box')[0].tolist() == [280, 160, 320, 160]


def a_diagonal_and_a_floor(make):
    """min_step 0: (3, 4) pixels is 40 eighths exactly; (1, 1) more is isqrt(128) = 11, and the straight distance from
    the first point is isqrt(32^2 + 40^2) = 51 while the path is 40 + 11."""
    h = make(1, min_step=0, **ONE)
    h.frame(*pts((20, 20)), [4])
    assert row(h.frame(*pts((23, 24)), [4])) == (2, 1, 40, 40)
    assert row(h.frame(*pts((24, 25)), [4])) == (3, 2, 51, 51)
    # min_step 0 commits a pose that has not moved at all
    assert row(h.frame(*pts((24, 25)), [4])) == (4, 3, 51, 51) and h.get('head')[0] == 3


def gaps_and_max_age(make):
    """max_age 2: seen in frame 1 and again in frame 3 (3 - 1 = 2 is not > 2): the same slot, and the move spans the
    gap.  Then not for three frames: frame 6 frees the slot (6 - 3 > 2), and frame 7 is a birth: the ring starts over."""
    h = make(1, max_age=2, **ONE)
    h.frame(*pts((20, 20)), [9])
    h.frame(*none())
    assert row(h.frame(*pts((30, 20)), [9])) == (2, 2, 80, 80)
    for f in (4, 5, 6):
        h.frame(*none())
        assert h.get('id')[0] == (9 if f < 6 else 0)
    assert row(h.frame(*pts((60, 20)), [9])) == (1, 0, 0, 0)
    assert h.get('head')[0] == 0 and h.get('pts')[0, 0].tolist() == [480, 160] and h.get('when')[0, 0] == 7
    assert h.get('box')[0].tolist() == [480, 160, 480, 160] and h.get('last')[0] == 7


def who_takes_no_part(make):
    """A duplicate id, an id of 0, keep = 0, a score at the threshold, NaN and inf coordinates leave no point."""
    h = make(1, **ONE)
    kp, bb = pts((20, 20), (30, 20), (20, 30), (20, 30), (20, 30), (20, 30), (20, 30))
    bb[4, 4] = np.float32(0.3)
    kp[5, 0, 0] = np.nan
    bb[6, 2] = np.inf
    out = h.frame(kp, bb, [7, 7, 0, 3, 4, 5, 6], keep=[1, 1, 1, 0, 1, 1, 1])
    assert out['count'].tolist() == [1, 0, 0, 0, 0, 0, 0] and h.get('id')[:2].tolist() == [7, 0] and h.get('dropped') == 0
    # a pose that is not valid is not the first of its id: the second one takes part
    out = h.frame(*pts((30, 20), (25, 20)), [7, 7], keep=[0, 1])
    assert [row(out, d) for d in (0, 1)] == [(0, 0, 0, 0), (2, 1, 40, 40)]


def slots_full(make):
    """max_tracks 2: a third id finds no slot, is counted in dropped and gets zeros."""
    h = make(1, max_tracks=2, **ONE)
    out = h.frame(*pts((20, 20), (30, 20), (40, 20)), [11, 12, 13])
    assert out['count'].tolist() == [1, 1, 0] and h.get('id').tolist() == [11, 12] and h.get('dropped') == 1
    out = h.frame(*pts((45, 20), (25, 20)), [13, 11])
    assert [row(out, d) for d in (0, 1)] == [(0, 0, 0, 0), (2, 1, 40, 40)] and h.get('dropped') == 2


def there_and_back(make):
    """A walk out and back: dist returns to 0, the path does not, and the box keeps the far point while it is in the
    ring."""
    h = make(1, length=4, **ONE)
    rows = [row(h.frame(*pts((x, 20)), [4])) for x in (20, 30, 40, 30, 20)]
    assert rows == [(1, 0, 0, 0), (2, 1, 80, 80), (3, 2, 160, 160), (4, 3, 80, 240), (4, 3, 80, 240)]
    assert h.get('box')[0].tolist() == [160, 160, 320, 160] and h.get('head')[0] == 0


SCRIPTS = [standing, walking, the_step_that_commits, every_third_frame, a_ring_of_two, a_diagonal_and_a_floor,
           gaps_and_max_age, who_takes_no_part, slots_full, there_and_back]
