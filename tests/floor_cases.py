"""Hand-worked scripts for the ground-plane rule of DESIGN section 23: every expected number below was worked out on
paper from the rule, not taken from a run.  A script drives a harness -- `Harness(K, **kw)` with `set_plane(camera,
**kw)`, `frame(kpts, bboxes, ids, keep=None, camera=0)` -> the outputs as numpy arrays (the floor-unit result as
`kpts` and `bboxes`) and `get(field, camera=0)` -> a state array -- so the same scripts run on the numpy statement and
on the device.

All scripts use anchor='box': a person is a box whose bottom centre (cx, by) is the anchor, (8 cx, 8 by) in 1/8 pixel.
With H = diag(10, 10, 1) a pixel is 10 mm and X = floor(1.25 ax + 1/2)."""
import numpy as np

K = 3
FLAT = [[10.0, 0.0, 0.0], [0.0, 10.0, 0.0], [0.0, 0.0, 1.0]]


def people(feet, score=0.8):
    """Boxes 10 pixels wide and 20 high with their bottom centres at `feet` [(cx, by), ...]."""
    feet = np.asarray(feet, np.float64).reshape(-1, 2)
    bboxes = np.zeros((len(feet), 5), np.float32)
    bboxes[:, 0], bboxes[:, 1] = feet[:, 0] - 5, feet[:, 1] - 20
    bboxes[:, 2], bboxes[:, 3] = feet[:, 0] + 5, feet[:, 1]
    bboxes[:, 4] = score
    kpts = np.zeros((len(feet), K, 3), np.float32)
    kpts[..., 2] = np.linspace(0.5, 0.9, K, dtype=np.float32)
    return kpts, bboxes


NONE = (np.zeros((0, K, 3), np.float32), np.zeros((0, 5), np.float32))


def expect(out, **fields):
    for name, want in fields.items():
        assert np.asarray(out[name]).tolist() == want, (name, np.asarray(out[name]).tolist(), want)


def a_walk_its_speed_and_its_distance(Harness):
    """One person, id 7, velocity_gain 4.  (20, 100) px -> (200, 1000) mm; two moves of (30, 40) mm, a frame standing,
    two frames away and a move of (-5, 0) over dt = 3."""
    h = Harness(K, anchor='box')
    h.set_plane(0, matrix=FLAT)
    out = h.frame(*people([(20, 100)]), [7])
    expect(out, on=[1], xy=[[200, 1000]], vel=[[0, 0]], speed=[0], travel=[0], nearest=[-1], gap=[-1], near=[0])
    assert h.get('hits')[0] == 1 and h.get('id')[0] == 7 and h.get('last')[0] == 1
    out = h.frame(*people([(23, 104)]), [7])
    # d = (30, 40), dt = 1: m = (7680, 10240); hits was 1, so vel = m; |v| = 256 * 50
    expect(out, xy=[[230, 1040]], vel=[[7680, 10240]], speed=[12800], travel=[50])
    out = h.frame(*people([(26, 108)]), [7])
    expect(out, xy=[[260, 1080]], vel=[[7680, 10240]], speed=[12800], travel=[100])
    out = h.frame(*people([(26, 108)]), [7])
    # m = 0: vel += floor(4 (0 - vel) / 16) = (-1920, -2560) -> (5760, 7680), |v| = 9600
    expect(out, xy=[[260, 1080]], vel=[[5760, 7680]], speed=[9600], travel=[100])
    assert h.get('hits')[0] == 4
    for _ in range(2):
        expect(h.frame(*NONE, []), on=[])
    out = h.frame(*people([(25.5, 108)]), [7])
    # frame 7, last 4: dt = 3; ax = 62 + 142 = 204, X = floor(255.5) = 255, d = (-5, 0); mx = floor(-1280 / 3) = -427
    # vx = 5760 + floor(4 (-427 - 5760) / 16) = 5760 + floor(-1546.75) = 4213; vy = 7680 - 1920 = 5760
    # 4213^2 + 5760^2 = 50 926 969; 7136^2 = 50 922 496 <= it < 7137^2 = 50 936 769
    expect(out, xy=[[255, 1080]], vel=[[4213, 5760]], speed=[7136], travel=[105])
    assert h.get('hits')[0] == 5 and h.get('last')[0] == 7 and h.get('frame') == 7
    assert h.get('pos')[0].tolist() == [255, 1080] and h.get('travel')[0] == 105


def neighbours_ties_and_who_counts(Harness):
    """near = 100 mm.  Poses 0 and 1 on one point, 2 and 3 both 100 mm from it (60, 80), pose 4 untracked (id 0) but
    placed, pose 5 at the score threshold and so not placed."""
    h = Harness(K, anchor='box', near=100)
    h.set_plane(0, matrix=FLAT)
    kpts, bboxes = people([(20, 10), (20, 10), (26, 18), (14, 2), (20, 30), (20, 12)])
    bboxes[5, 4] = 0.3
    out = h.frame(kpts, bboxes, [1, 2, 3, 4, 0, 6])
    expect(out, on=[1, 1, 1, 1, 1, 0],
           xy=[[200, 100], [200, 100], [260, 180], [140, 20], [200, 300], [0, 0]],
           # 2: 100 to 0 and to 1 (the lower index), 134 to 4 (60^2 + 120^2 = 18 000, 134^2 = 17 956), 200 to 3
           # 4: 200 to 0 and 1, 134 to 2, 286 to 3 (60^2 + 280^2 = 82 000, 286^2 = 81 796)
           nearest=[1, 0, 0, 0, 2, -1], gap=[0, 0, 100, 100, 134, -1], near=[3, 3, 2, 2, 0, 0])
    assert h.get('id')[:5].tolist() == [1, 2, 3, 4, 0] and h.get('dropped') == 0


def the_horizon_and_the_bounds(Harness):
    """w = 1 - by / 100: the horizon is the row by = 100.  At by = 50 a pixel is 20 mm.  Bounds (0, 0, 3000, 4000), ends
    included: cx = 150 lands on X = 3000, cx = 150.25 on 3005."""
    h = Harness(K, anchor='box')
    h.set_plane(0, matrix=[[10.0, 0.0, 0.0], [0.0, 10.0, 0.0], [0.0, -0.01, 1.0]], bounds=(0, 0, 3000, 4000))
    out = h.frame(*people([(10, 50), (10, 120), (150, 50), (150.25, 50), (10, 100.5)]), [1, 2, 3, 4, 5])
    expect(out, on=[1, 0, 1, 0, 0], xy=[[200, 1000], [0, 0], [3000, 1000], [0, 0], [0, 0]],
           nearest=[2, -1, 0, -1, -1], gap=[2800, -1, 2800, -1, -1])
    assert h.get('id')[:3].tolist() == [1, 3, 0]
    assert np.isnan(out['bboxes'][[1, 3, 4], :4]).all() and np.isnan(out['kpts'][[1, 3, 4], :, :2]).all()


def the_bridge_to_floor_pixels(Harness):
    """unit 20 mm, origin (100, -40) mm.  (100, 100) mm -> P = (0, 28) -> (0, 7) floor pixels; X = 95 -> Px = floor(-1)
    and the pose leaves the plan; (138, 103) mm -> P = (floor(7.6), floor(28.6)) = (7, 28) -> (1.75, 7)."""
    h = Harness(K, anchor='box', unit=20, origin=(100, -40))
    h.set_plane(0, matrix=FLAT)
    kpts, bboxes = people([(10, 10), (9.5, 10), (13.75, 10.3)])
    out = h.frame(kpts, bboxes, [1, 2, 3])
    expect(out, on=[1, 1, 1], xy=[[100, 100], [95, 100], [138, 103]])
    assert out['bboxes'][0].tolist() == [0.0, 7.0, 0.0, 7.0, np.float32(0.8)]
    assert out['bboxes'][2].tolist() == [1.75, 7.0, 1.75, 7.0, np.float32(0.8)]
    assert np.isnan(out['bboxes'][1, :4]).all() and out['bboxes'][1, 4] == np.float32(0.8)
    assert (out['kpts'][0, :, :2] == [0.0, 7.0]).all() and (out['kpts'][2, :, :2] == [1.75, 7.0]).all()
    assert np.isnan(out['kpts'][1, :, :2]).all()
    assert out['kpts'][..., 2].tobytes() == kpts[..., 2].tobytes()


def one_slot_drops_gaps_and_duplicates(Harness):
    """max_tracks 1, max_age 2."""
    h = Harness(K, anchor='box', max_tracks=1, max_age=2)
    h.set_plane(0, matrix=FLAT)
    out = h.frame(*people([(10, 10), (20, 10)]), [5, 6])           # frame 1: 5 takes the slot, 6 finds none
    expect(out, on=[1, 1], travel=[0, 0])
    assert h.get('id').tolist() == [5] and h.get('dropped') == 1
    h.frame(*people([(21, 10)]), [6])                               # frame 2: the slot is 5's
    assert h.get('id').tolist() == [5] and h.get('dropped') == 2
    h.frame(*NONE, [])                                              # frame 3: 3 - 1 = 2 is not > 2
    assert h.get('id').tolist() == [5]
    out = h.frame(*people([(20, 10), (30, 10)]), [6, 6])            # frame 4: 4 - 1 > 2 frees it; the first 6 is born
    expect(out, on=[1, 1], vel=[[0, 0], [0, 0]], nearest=[1, 0], gap=[100, 100])
    assert h.get('id').tolist() == [6] and h.get('dropped') == 2 and h.get('pos')[0].tolist() == [200, 100]
    h.frame(*NONE, [])
    out = h.frame(*people([(20, 13)]), [6])                         # frame 6: away for max_age frames, dt = 2
    expect(out, vel=[[0, 3840]], speed=[3840], travel=[30])         # floor(256 * 30 / 2)
    assert h.get('hits').tolist() == [2]
    h.frame(*NONE, [])
    h.frame(*NONE, [])
    out = h.frame(*people([(20, 16)]), [6])                         # frame 9: 9 - 6 > 2: born again
    expect(out, vel=[[0, 0]], speed=[0], travel=[0])
    assert h.get('hits').tolist() == [1] and h.get('last').tolist() == [9] and h.get('frame') == 9


SCRIPTS = [a_walk_its_speed_and_its_distance, neighbours_ties_and_who_counts, the_horizon_and_the_bounds,
           the_bridge_to_floor_pixels, one_slot_drops_gaps_and_duplicates]
