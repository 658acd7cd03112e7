"""Hand-worked scripts for the contact rule of DESIGN section 24: every expected number below was worked out on paper
from the rule, not taken from a run.  A script drives a harness -- `Harness(**kw)` with `frame(xy, ids, on=None,
camera=0)` -> the outputs as numpy arrays, `counts(camera=0)` -> {name: int}, `get(field, camera=0)` -> a slot array and
`pair(field, camera=0)` -> a pair-word array -- so the same scripts run on the numpy statement and on the device.

Poses are floor positions in mm.  An event row is (kind, a, b, frames, pose_a, pose_b, frame) with a < b."""
import numpy as np

MEET, PART, LONG = 1, 2, 3


def expect(out, **fields):
    for name, want in fields.items():
        assert np.asarray(out[name]).tolist() == want, (name, np.asarray(out[name]).tolist(), want)


def events(out):
    """The stored rows; every row past them must be zero."""
    n = min(int(out['n_events']), len(out['events']))
    assert not np.asarray(out['events'])[n:].any()
    return [tuple(r) for r in np.asarray(out['events'])[:n].tolist()]


def counts(h, camera=0, **fields):
    got = h.counts(camera)
    for name, want in fields.items():
        assert int(got[name]) == want, (name, int(got[name]), want)
    assert int(got['contacts']) == int(got['meets']) - int(got['parts'])


def meet_hold_and_part_with_hysteresis(Harness):
    """radius 1500, release 1800, min_frames 2.  Pose 0 is id 7 (slot 0), pose 1 id 3 (slot 1).  (900, 1200) is 1500
    away, (1080, 1440) is 1800, (1081, 1440) is further: 1081^2 + 1440^2 = 3 242 161 > 3 240 000."""
    h = Harness(radius=1500, release=1800, min_frames=2)
    out = h.frame([(0, 0), (900, 1200)], [7, 3])                    # near, run 1
    expect(out, group=[7, 3], size=[1, 1], contacts=[0, 0], partner=[0, 0], together=[0, 0], n_events=0)
    assert h.pair('link')[0, 1] == 1 << 8 and h.get('id')[:2].tolist() == [7, 3]
    counts(h, contacts=0, meets=0, groups=0, grouped=0, largest=1)
    out = h.frame([(0, 0), (900, 1200)], [7, 3])                    # run 2: the bit is set in frame 2
    assert events(out) == [(MEET, 3, 7, 0, 1, 0, 2)]
    expect(out, group=[3, 3], size=[2, 2], contacts=[1, 1], partner=[3, 7], together=[0, 0], n_events=1)
    assert h.pair('link')[0, 1] == 1 and h.pair('since')[0, 1] == 2
    counts(h, contacts=1, meets=1, parts=0, groups=1, grouped=2, largest=2)
    out = h.frame([(0, 0), (1080, 1440)], [7, 3])                   # beyond radius, on release: still near
    expect(out, together=[1, 1], n_events=0)
    assert h.pair('link')[0, 1] == 1
    out = h.frame([(0, 0), (1081, 1440)], [7, 3])                   # past release: run 1
    expect(out, contacts=[1, 1], together=[2, 2], n_events=0)
    assert h.pair('link')[0, 1] == 1 | 1 << 8
    h.frame([(0, 0), (900, 1200)], [7, 3])                          # back: run 0
    assert h.pair('link')[0, 1] == 1
    out = h.frame([(0, 0), (2000, 0)], [7, 3])
    expect(out, partner=[3, 7], together=[4, 4], n_events=0)
    out = h.frame([(0, 0), (2000, 0)], [7, 3])                      # frame 7: parted after 7 - 2 = 5 frames
    assert events(out) == [(PART, 3, 7, 5, 1, 0, 7)]
    expect(out, group=[7, 3], size=[1, 1], contacts=[0, 0], partner=[0, 0], together=[0, 0])
    assert h.pair('link')[0, 1] == 0 and h.pair('since')[0, 1] == 0
    counts(h, contacts=0, meets=1, parts=1, longs=0, groups=0, grouped=0, largest=1)
    out = h.frame([(0, 0), (1600, 0)], [7, 3])                      # inside release but not inside radius: not near
    assert h.pair('link')[0, 1] == 0 and int(out['n_events']) == 0


def on_the_threshold_and_one_past_it(Harness):
    """radius = release = 1500, min_frames 1: 900^2 + 1200^2 = 1500^2 is near, 901^2 + 1200^2 is not; and the same
    when the pair is in contact."""
    h = Harness(radius=1500, min_frames=1)
    out = h.frame([(0, 0), (900, 1200), (100000, 0), (100901, 1200)], [1, 2, 3, 4])
    assert events(out) == [(MEET, 1, 2, 0, 0, 1, 1)]
    expect(out, group=[1, 1, 3, 4], size=[2, 2, 1, 1])
    out = h.frame([(0, 0), (900, 1200), (100000, 0), (100900, 1200)], [1, 2, 3, 4])
    assert events(out) == [(MEET, 3, 4, 0, 2, 3, 2)]
    out = h.frame([(0, 0), (901, 1200), (100000, 0), (100900, 1200)], [1, 2, 3, 4])
    assert events(out) == [(PART, 1, 2, 2, 0, 1, 3)]
    expect(out, group=[1, 2, 3, 3], partner=[0, 0, 4, 3], together=[0, 0, 1, 1])
    counts(h, contacts=1, meets=2, parts=1, groups=1, grouped=2, largest=2)


def an_unseen_partner_holds_the_run(Harness):
    """min_frames 3: two near frames, a frame without id 2, and the third near frame sets the bit in frame 4."""
    h = Harness(radius=1500, min_frames=3)
    h.frame([(0, 0), (1000, 0)], [1, 2])
    h.frame([(0, 0), (1000, 0)], [1, 2])
    assert h.pair('link')[0, 1] == 2 << 8
    out = h.frame([(0, 0)], [1])
    expect(out, group=[1], size=[1], n_events=0)
    assert h.pair('link')[0, 1] == 2 << 8
    out = h.frame([(1000, 0), (0, 0)], [2, 1])                      # (the rows swapped: pose 0 is id 2)
    assert events(out) == [(MEET, 1, 2, 0, 1, 0, 4)]
    expect(out, group=[1, 1], partner=[1, 2])


def a_gap_of_max_age_and_one_frame_more(Harness):
    """max_age 2, min_frames 1.  Id 2 is seen in frames 1 and 3 (3 - 1 is not > 2: the contact goes on), then never:
    frame 6 frees its slot (6 - 3 > 2) and the contact parts after 6 - 1 = 5 frames, without poses."""
    h = Harness(radius=1500, min_frames=1, max_age=2)
    out = h.frame([(0, 0), (1000, 0)], [1, 2])
    assert events(out) == [(MEET, 1, 2, 0, 0, 1, 1)]
    out = h.frame([(0, 0)], [1])
    expect(out, group=[1], size=[2], contacts=[1], partner=[2], together=[1], n_events=0)
    out = h.frame([(0, 0), (1000, 0)], [1, 2])
    expect(out, together=[2, 2], n_events=0)
    for f in (4, 5):
        out = h.frame([(0, 0)], [1])
        expect(out, size=[2], together=[f - 1], n_events=0)
    out = h.frame([(0, 0)], [1])
    assert events(out) == [(PART, 1, 2, 5, -1, -1, 6)]
    expect(out, group=[1], size=[1], contacts=[0], partner=[0], together=[0])
    assert h.get('id')[:2].tolist() == [1, 0]
    counts(h, contacts=0, meets=1, parts=1, groups=0, grouped=0, largest=1)


def a_slot_that_expires_and_is_born_again_in_one_frame(Harness):
    """max_age 2, min_frames 1, max_events 1.  Id 2 is seen in frame 1 and again in frame 4: its slot is freed there (4 -
    1 > 2), the contact parts after 3 frames, id 2 is born into the same slot and meets id 1 again, in that order; the
    table holds one row of the two."""
    h = Harness(radius=1500, min_frames=1, max_age=2, max_events=1)
    h.frame([(0, 0), (1000, 0)], [1, 2])
    h.frame([(0, 0)], [1])
    h.frame([(0, 0)], [1])
    out = h.frame([(0, 0), (1000, 0)], [1, 2])
    assert int(out['n_events']) == 2 and events(out) == [(PART, 1, 2, 3, -1, -1, 4)]
    expect(out, group=[1, 1], size=[2, 2], together=[0, 0])
    assert h.get('id')[:2].tolist() == [1, 2] and h.pair('since')[0, 1] == 4
    counts(h, contacts=1, meets=2, parts=1)


def a_long_contact_is_reported_once(Harness):
    """long_frames 3, min_frames 1: met in frame 1, LONG in frame 4 whether or not both are seen, and never again."""
    h = Harness(radius=1500, min_frames=1, long_frames=3)
    h.frame([(0, 0), (1000, 0)], [1, 2])
    for _ in range(2):
        expect(h.frame([(0, 0), (1000, 0)], [1, 2]), n_events=0)
    out = h.frame([(0, 0)], [1])
    assert events(out) == [(LONG, 1, 2, 3, 0, -1, 4)]
    for _ in range(4):
        expect(h.frame([(0, 0), (1000, 0)], [1, 2]), n_events=0)
    counts(h, contacts=1, meets=1, parts=0, longs=1)


def two_parties_merge_and_split(Harness):
    """radius 1000, min_frames 1; ids 10, 20, 30, 40 in slots 0 .. 3 on a line."""
    h = Harness(radius=1000, min_frames=1)
    out = h.frame([(0, 0), (900, 0), (5000, 0), (5900, 0)], [10, 20, 30, 40])
    assert events(out) == [(MEET, 10, 20, 0, 0, 1, 1), (MEET, 30, 40, 0, 2, 3, 1)]
    expect(out, group=[10, 10, 30, 30], size=[2, 2, 2, 2], contacts=[1, 1, 1, 1], partner=[20, 10, 40, 30])
    counts(h, contacts=2, meets=2, groups=2, grouped=4, largest=2)
    out = h.frame([(0, 0), (900, 0), (1800, 0), (2700, 0)], [10, 20, 30, 40])
    assert events(out) == [(MEET, 20, 30, 0, 1, 2, 2)]
    # id 20 has 10 (since 1) and 30 (since 2): the older; id 30 has 20 (since 2) and 40 (since 1)
    expect(out, group=[10, 10, 10, 10], size=[4, 4, 4, 4], contacts=[1, 2, 2, 1], partner=[20, 10, 40, 30],
           together=[1, 1, 1, 1])
    counts(h, contacts=3, meets=3, groups=1, grouped=4, largest=4)
    out = h.frame([(0, 0), (900, 50000), (1800, 0), (2700, 0)], [10, 20, 30, 40])
    assert events(out) == [(PART, 10, 20, 2, 0, 1, 3), (PART, 20, 30, 1, 1, 2, 3)]
    expect(out, group=[10, 20, 30, 30], size=[1, 1, 2, 2], contacts=[0, 0, 1, 1], partner=[0, 0, 40, 30], together=[0, 0, 2, 2])
    counts(h, contacts=1, meets=3, parts=2, groups=1, grouped=2, largest=2)


def who_takes_part_and_who_is_dropped(Harness):
    """max_tracks 2: a duplicate id, ids 0 and -3, a pose that is not on the floor and a pose that finds no slot."""
    h = Harness(radius=1500, min_frames=1, max_tracks=2)
    out = h.frame([(0, 0), (100, 0), (0, 100), (50, 50), (10, 10), (200, 0), (300, 0)], [5, 5, 0, -3, 6, 7, 8],
                  on=[1, 1, 1, 1, 0, 1, 1])
    assert events(out) == [(MEET, 5, 7, 0, 0, 5, 1)]
    expect(out, group=[5, 0, 0, 0, 0, 5, 0], size=[2, 0, 0, 0, 0, 2, 0], contacts=[1, 0, 0, 0, 0, 1, 0],
           partner=[7, 0, 0, 0, 0, 5, 0])
    assert h.get('id').tolist() == [5, 7] and h.get('dropped') == 1 and h.get('frame') == 1
    assert h.get('pos').tolist() == [[0, 0], [200, 0]]


def radius_zero_and_positions_past_the_floor(Harness):
    """radius 0: two on one point are near.  Positions are read clamped to +-(2^20 - 1): two far past it stand on one
    point too."""
    h = Harness(radius=0, min_frames=1)
    far = 1 << 20
    out = h.frame([(5, 5), (5, 5), (far + 5000, 0), (far + 9000, 0), (5, 6)], [1, 2, 3, 4, 9])
    assert events(out) == [(MEET, 1, 2, 0, 0, 1, 1), (MEET, 3, 4, 0, 2, 3, 1)]
    expect(out, group=[1, 1, 3, 3, 9], size=[2, 2, 2, 2, 1])
    assert h.get('pos')[2].tolist() == [far - 1, 0] and h.get('pos')[3].tolist() == [far - 1, 0]


SCRIPTS = [meet_hold_and_part_with_hysteresis, on_the_threshold_and_one_past_it, an_unseen_partner_holds_the_run,
           a_gap_of_max_age_and_one_frame_more, a_slot_that_expires_and_is_born_again_in_one_frame,
           a_long_contact_is_reported_once, two_parties_merge_and_split, who_takes_part_and_who_is_dropped,
           radius_zero_and_positions_past_the_floor]
