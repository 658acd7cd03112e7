"""The ground plane on the device (csrc/pave_floor.hip, pave_floor_update) against the rule of DESIGN section 23 in
numpy (tests/floor_ref.py): after every frame every output, every state tensor (live slots), the calibration words and
the floor-unit result (bytewise, NaNs included) are compared with the oracle by torch.equal, and the inputs with what
they were.  Needs an MI355X."""
import numpy as np
import pytest
import torch

from tests import floor_cases as FC
from tests import floor_ref as FR
from tests.heat_ref import HeatRef
from tests.test_floor_cpu import FRONTO, HORIZON, TILTED, to_floor
from tests.test_track_gpu import FIGURE15, poses, result
from tests.trail_draw_ref import draw_bgr
from tests.trail_ref import TrailRef
from tests.zones_ref import ZoneRef

pytestmark = pytest.mark.gpu

OUTPUTS = list(FR.OUTPUTS)
STATE = list(FR.STATE)
MARKS = [(x, y) for y in (1500.0, 4000.0, 7900.0) for x in (300.0, 4100.0, 7800.0)]


class Pair:
    """A GroundPlane and the oracle, configured alike."""

    def __init__(self, K=15, **kw):
        from pavenet_amd import GroundPlane
        self.plane, self.ref = GroundPlane(K, **kw), FR.FloorRef(K, **kw)

    def set_plane(self, camera, **kw):
        self.plane.set_plane(camera, **kw)
        self.ref.set_plane(camera, **kw)
        assert np.array_equal(self.plane.H[camera], self.ref.H[camera])
        same_calibration(self, camera)


def same(got, exp, what, dtype=torch.int32):
    g, e = got.detach().cpu(), torch.from_numpy(np.array(exp))
    assert g.dtype == dtype and e.dtype == dtype and g.shape == e.shape, (what, g.dtype, tuple(g.shape), tuple(e.shape))
    assert torch.equal(g, e), f'{what}: {int((g != e).sum())} words differ, first at {(g != e).nonzero()[:4].tolist()}: ' \
                              f'{g[g != e][:4].tolist()} for {e[g != e][:4].tolist()}'


def same_calibration(p, camera):
    got, exp = p.plane.calibration(camera), p.ref.calibration(camera)
    assert list(got) == ['G', 'bounds', 'valid']
    for name in got:
        same(got[name], exp[name], f'camera {camera} calibration {name}', torch.int64)


def same_bytes(got, exp, what):
    g, e = got.detach().cpu().contiguous(), torch.from_numpy(np.ascontiguousarray(exp))
    assert g.dtype == torch.float32 and g.shape == e.shape, (what, g.dtype, tuple(g.shape), tuple(e.shape))
    assert torch.equal(g.view(torch.int32), e.view(torch.int32)), f'{what}: the bytes differ'


def same_outputs(got, exp, what, res=None):
    assert sorted(got) == sorted(OUTPUTS + ['floor'])
    for name in OUTPUTS:
        assert got[name].is_cuda
        same(got[name], exp[name], f'{what}: {name}')
    floor = got['floor']
    if isinstance(floor, dict):
        assert sorted(floor) == ['bboxes', 'keep', 'kpts'] and (res is None or floor['keep'] is res['keep'])
        bb, kp = floor['bboxes'], floor['kpts']
        assert res is None or (bb.shape == res['bboxes'].shape and kp.shape == res['kpts'].shape)
        bb, kp = bb.reshape(exp['bboxes'].shape), kp.reshape(exp['kpts'].shape)
    else:
        assert isinstance(floor, tuple) and len(floor) == 3 and (res is None or floor[1] is res[1])
        bb, kp = floor[0], floor[2]
    same_bytes(bb, exp['bboxes'], f'{what}: floor bboxes')
    same_bytes(kp, exp['kpts'], f'{what}: floor kpts')


def same_all(p, cameras, what):
    """The slots of the oracle that are live, and everything else whole (a free slot's other fields are never
    read)."""
    for c in cameras:
        got, exp = p.plane.state(c), p.ref.state(c)
        assert list(got) == STATE
        live = exp['id'] != 0
        for name in STATE:
            g, e = got[name], np.asarray(exp[name])
            if e.ndim >= 1 and name != 'id':
                g, e = g[torch.from_numpy(live).to(g.device)], e[live]
            same(g, e, f'{what}: camera {c} state {name}')
        same_calibration(p, c)


def flat(res):
    return [t for t in (res.values() if isinstance(res, dict) else res) if isinstance(t, torch.Tensor)]


def step(p, kpts, bboxes, ids, what, keep=None, scale=None, camera=0, form='tuple'):
    """One frame through the device and the reference; everything compared, the inputs included.  Returns the oracle's
    outputs and the device's."""
    ids = np.asarray(ids, np.int64).astype(np.int32)
    exp = p.ref.update(kpts, bboxes, ids, keep, (1.0, 1.0) if scale is None else scale, camera)
    res, dev_ids = result(kpts, bboxes, keep, form), torch.from_numpy(ids).cuda()
    before = [t.clone() for t in flat(res) + [dev_ids]]
    got = p.plane.update(res, dev_ids, scale_factor=scale, camera=camera)
    same_outputs(got, exp, what, res)
    same_all(p, [camera], what)
    for t, b in zip(flat(res) + [dev_ids], before):
        assert torch.equal(t.view(torch.uint8), b.view(torch.uint8)) if t.numel() else True, f'{what}: an input changed'
    return exp, got


@pytest.mark.parametrize('script', FC.SCRIPTS, ids=lambda s: s.__name__)
def test_hand_worked_scripts_on_the_device(script):
    class Harness:
        def __init__(self, K, **kw):
            self.p = Pair(K, **kw)
            self.frames = 0

        def set_plane(self, camera, **kw):
            self.p.set_plane(camera, **kw)

        def frame(self, kpts, bboxes, ids, keep=None, camera=0):
            self.frames += 1
            _, got = step(self.p, kpts, bboxes, ids, f'{script.__name__} frame {self.frames}',
                          None if keep is None else np.asarray(keep, np.int32), camera=camera,
                          form='tuple' if keep is None else 'dict')
            out = {name: got[name].cpu().numpy() for name in OUTPUTS}
            out['bboxes'], out['kpts'] = got['floor'][0].cpu().numpy(), got['floor'][2].cpu().numpy()
            return out

        def get(self, field, camera=0):
            return self.p.plane.state(camera)[field].cpu().numpy()
    script(Harness)


def marks(H, at=MARKS):
    return [((x, y), to_floor(H, x, y)[:2]) for x, y in at]


def people(rng, pos, height=300.0, scale=(1.0, 1.0), **kw):
    return poses(rng, FIGURE15, np.asarray(pos, np.float64).reshape(-1, 2), height=height, scale=scale, **kw)


NONE = np.zeros((0, 15, 3), np.float32), np.zeros((0, 5), np.float32)


@pytest.mark.parametrize('max_tracks', [1, 2, 128])
def test_no_pose_one_two_and_128_poses_with_drops(max_tracks):
    """N = 0 (the clock still runs), 1, 2 and then 128 poses with 128 ids for three frames under the tilted camera:
    max_tracks 1 and 2 drop all but the first ids, 128 holds them all; 129 poses are refused."""
    rng = np.random.default_rng(241)
    p = Pair(15, max_tracks=max_tracks, near=3000)
    p.set_plane(0, points=marks(TILTED))
    exp, _ = step(p, *NONE, [], 'N = 0')
    assert exp['on'].shape == (0,) and p.ref.frame[0] == 1
    step(p, *people(rng, [(1000.0, 4000.0)]), [9], 'N = 1')
    step(p, *people(rng, [(1000.0, 4030.0), (5000.0, 2000.0)]), [9, 3], 'N = 2')
    start = np.stack([200.0 + 480.0 * (np.arange(128) % 16), 100.0 + 900.0 * (np.arange(128) // 16)], 1)
    for f in range(3):
        order = rng.permutation(128)
        kpts, bboxes = people(rng, start + (30.0 * f, 20.0 * f))
        exp, _ = step(p, kpts[order], bboxes[order], (np.arange(1, 129))[order], f'N = 128 frame {f}')
    assert exp['on'].all() and (exp['nearest'] >= 0).all() and (p.ref.id[0] != 0).sum() == max_tracks
    assert (p.ref.dropped[0] > 0) == (max_tracks < 128) and (exp['speed'] > 0).sum() >= min(max_tracks, 100)
    res = result(np.zeros((129, 15, 3), np.float32), np.zeros((129, 5), np.float32))
    with pytest.raises(ValueError, match='at most 128'):
        p.plane.update(res, torch.zeros(129, dtype=torch.int32, device='cuda'))


def test_two_on_one_point_three_equidistant_and_far_apart():
    """anchor 'box' on a plane of 250 mm a pixel: 65 poses on one point (gap 0, the lowest other index the nearest),
    three poses 1250 mm from that point and further from each other, so each has 65 equidistant candidates spread over
    both halves of the neighbour pass and takes index 0; and two in the far corners, 2.8 km apart, whose speed after
    they swap places is the largest the rule can produce."""
    plane = [[250.0, 0.0, -1000000.0], [0.0, 250.0, -1000000.0], [0.0, 0.0, 1.0]]
    p = Pair(3, anchor='box', near=1500, max_tracks=8)
    p.set_plane(0, matrix=plane)
    feet = [(4000.0, 4000.0)] * 70
    feet[3], feet[40], feet[69] = (4005.0, 4000.0), (3995.0, 4000.0), (4000.0, 4005.0)       # 1250 mm from the crowd's point
    feet[10], feet[50] = (0.5, 0.5), (7999.5, 7999.5)                                        # the far corners
    kpts, bboxes = FC.people(feet)
    ids = np.arange(1, 71)
    exp, _ = step(p, kpts, bboxes, ids, 'frame 1')
    assert exp['gap'][0] == 0 and exp['nearest'][0] == 1 and exp['nearest'][1] == 0 and exp['nearest'][68] == 0
    assert exp['gap'][[3, 40, 69]].tolist() == [1250, 1250, 1250] and exp['nearest'][[3, 40, 69]].tolist() == [0, 0, 0]
    assert exp['near'][0] == 64 + 3 and exp['near'][3] == 65 and exp['near'][10] == 0 and exp['gap'][10] > 1400000
    assert exp['nearest'][10] == 40 and exp['nearest'][50] == 3        # (3 and 69 are as far from 50: a tie across the halves)
    swap = list(feet)
    swap[10], swap[50] = feet[50], feet[10]
    exp, _ = step(p, *FC.people(swap), ids, 'frame 2')
    assert exp['travel'][10] == 0 and p.ref.dropped[0] == 2 * 62          # (eight slots: ids 1 .. 8 are followed)
    q = Pair(3, anchor='box', max_tracks=2)
    q.set_plane(0, matrix=plane)
    step(q, *FC.people([feet[10], feet[50]]), [1, 2], 'corners')
    exp, _ = step(q, *FC.people([feet[50], feet[10]]), [1, 2], 'corners swapped')
    assert exp['speed'].min() > 2 ** 29 and exp['travel'].min() > 2800000


@pytest.mark.parametrize('form', ['tuple', 'dict'])
def test_both_result_forms_a_scale_factor_and_who_is_placed(form):
    """Twelve people crossing a picture made at scale (0.694, 0.7) under the camera whose horizon crosses it, in both
    result forms, with poses that are not placed: keep = 0 (dict form), a score at the threshold, NaN and inf
    coordinates, a person above the horizon (w <= 0); and placed ones that are not followed: ids 0 and -3 and a
    duplicate id."""
    rng = np.random.default_rng(242)
    scale = (0.694, 0.7)
    p = Pair(15, max_age=3, max_tracks=16, velocity_gain=3)
    p.set_plane(0, points=marks(HORIZON))
    start = np.stack([300.0 + 600.0 * np.arange(12), 1500.0 + 450.0 * np.arange(12)], 1)
    speed = np.stack([np.where(np.arange(12) % 2 == 0, 26.5, -26.5), np.where(np.arange(12) % 3 == 0, 12.5, -9.5)], 1)
    for f in range(12):
        there = [q for q in range(12) if not (q == 3 and 5 <= f < 7) and not (q == 5 and 4 <= f < 9)]
        kpts, bboxes = people(rng, (start + speed * f)[there], scale=scale)
        junk_k, junk_b = people(rng, np.stack([rng.uniform(0, 7000, 8), rng.uniform(1000, 7000, 8)], 1), scale=scale)
        junk_b[1, 4] = 0.3
        junk_k[2, rng.integers(15), 1] = np.nan
        junk_b[3, 0] = -np.inf
        junk_k[4], junk_b[4] = people(rng, [(3000.0, 10.0)], scale=scale)                  # its feet at row 310: the sky
        keep = np.ones(len(there) + 8, np.int32)
        keep[len(there)] = 0
        ids = np.concatenate([np.asarray(there) + 1, [40, 41, 42, 43, 44, 0, -3, 1]])      # (id 1 is there[0]'s: a duplicate)
        if form == 'tuple':
            junk_k, junk_b, ids, keep = junk_k[1:], junk_b[1:], np.delete(ids, len(there)), None
        kpts, bboxes = np.concatenate([kpts, junk_k]), np.concatenate([bboxes, junk_b])
        order = np.concatenate([[0], 1 + rng.permutation(len(bboxes) - 1)])                # (the first of id 1 stays first)
        exp, _ = step(p, kpts[order], bboxes[order], ids[order], f'{form} frame {f}', None if keep is None else keep[order],
                      scale, form=form)
        off = np.isin(ids[order], [40, 41, 42, 43, 44])
        assert not exp['on'][off].any() and exp['on'][~off].all() and (exp['nearest'][off] == -1).all()
        unfollowed = np.isin(ids[order], [0, -3]) | (np.arange(len(order)) == int(np.nonzero(order == len(order) - 1)[0][0]))
        assert not exp['travel'][unfollowed].any() and (exp['nearest'][unfollowed] >= 0).all()
    assert p.ref.frame[0] == 12 and p.ref.dropped[0] == 0 and exp['travel'].max() > 0


def test_a_point_exactly_on_the_bounds_and_one_past_them():
    """The fronto-parallel plane (2.5 mm a pixel), anchor 'box', bounds whose ends are floor positions of the frame's
    own poses: on the end is on the floor, 1 mm past it is not (a quarter pixel is 0.625 mm: two of them move X by
    1 or 2)."""
    p = Pair(3, anchor='box')
    p.set_plane(0, matrix=FRONTO, bounds=(-500, -1000, 2000, 3000))
    # X = 2.5 cx - 3000, Y = 2.5 by - 2000: cx = 2000 -> 2000, cx = 2000.5 -> 2001; by = 400 -> -1000, by = 399.5 -> -1001
    feet = [(2000.0, 1000.0), (2000.5, 1000.0), (1000.0, 400.0), (1000.0, 399.5), (1000.0, 2000.0), (1000.0, 2000.5)]
    exp, _ = step(p, *FC.people(feet), [1, 2, 3, 4, 5, 6], 'bounds')
    assert exp['on'].tolist() == [1, 0, 1, 0, 1, 0]
    assert exp['xy'].tolist() == [[2000, 500], [0, 0], [-500, -1000], [0, 0], [-500, 3000], [0, 0]]


@pytest.mark.parametrize('velocity_gain', [1, 16])
def test_gaps_of_max_age_and_one_more_and_both_ends_of_the_gain(velocity_gain):
    """max_age 3: a track seen in frame 3 and again in frame 6 (6 - 3 is not > 3) keeps its slot and its move is divided
    by dt = 3; one that misses four frames is freed in the fourth and born again.  velocity_gain 16 makes the velocity
    the newest move, 1 a sixteenth of the way to it."""
    rng = np.random.default_rng(243)
    p = Pair(15, max_age=3, max_tracks=4, velocity_gain=velocity_gain)
    p.set_plane(0, points=marks(TILTED))
    for f in range(3):
        step(p, *people(rng, [(1000.0 + 50.0 * f, 3000.0 - 20.0 * f)]), [6], f'frame {f}')
    for f in range(2):
        step(p, *NONE, [], f'gap frame {f}')
    exp, _ = step(p, *people(rng, [(1300.0, 2900.0)]), [6], 'back in frame 6')
    assert p.ref.hits[0, 0] == 4 and exp['travel'][0] > 0
    for f in range(4):
        step(p, *NONE, [], f'second gap frame {f}')
    assert p.ref.id[0, 0] == 0
    exp, _ = step(p, *people(rng, [(1500.0, 2800.0)]), [6], 'back in frame 11')
    assert p.ref.hits[0, 0] == 1 and exp['travel'].tolist() == [0] and exp['speed'].tolist() == [0]


@pytest.mark.parametrize('anchor', ['feet', 'box', 'centre'])
def test_anchors_are_the_zone_monitors(anchor):
    """The plane diag(8, 8, 1), 8 mm a pixel, maps the 1/8-pixel anchor onto itself: slot for slot, pos is the
    ZoneMonitor's pos on the same frames.  Key-point scores around kpt_thr, so 'feet' uses two, one or no ankle."""
    from pavenet_amd import ZoneMonitor
    rng = np.random.default_rng(244)
    scale = (1.3, 0.9)
    kw = dict(anchor=anchor, max_tracks=8, kpt_thr=0.4, max_age=1)
    p, mon = Pair(15, **kw), ZoneMonitor(15, **kw)
    p.set_plane(0, matrix=[[8.0, 0.0, 0.0], [0.0, 8.0, 0.0], [0.0, 0.0, 1.0]])
    for f in range(6):
        pos = np.stack([30.0 + 45.0 * np.arange(6) + 2.5 * f, 20.0 + 30.0 * np.arange(6)], 1)
        kpts, bboxes = poses(rng, FIGURE15, pos, height=90.0, scale=scale,
                             kpt_scores=rng.uniform(0.0, 1.0, (6, 15)).astype(np.float32))
        ids = np.asarray([1, 2, 3, 4, 5, 6], np.int32)
        step(p, kpts, bboxes, ids, f'{anchor} frame {f}', scale=scale)
        mon.update(result(kpts, bboxes), torch.from_numpy(ids).cuda(), scale_factor=scale)
        zs, ts = mon.state(0), p.plane.state(0)
        assert torch.equal(zs['id'], ts['id']) and torch.equal(zs['last'], ts['last']) and int((zs['id'] != 0).sum()) == 6
        assert torch.equal(zs['pos'][:6], ts['pos'][:6])


def test_three_cameras_one_uncalibrated_in_33_entries_of_two_launches():
    """update_many with 33 entries: camera 0 (tilted) 5 times, camera 1 (no plane: it places nobody and its clock runs)
    14 times, camera 2 (the horizon in the picture) 14 times, interleaved.  Against the same frames in single calls on a
    second object; the oracle runs beside both."""
    from pavenet_amd import GroundPlane
    rng = np.random.default_rng(245)
    kw = dict(cameras=3, max_age=2, max_tracks=6, near=4000)
    many, single = Pair(15, **kw), GroundPlane(15, **kw)
    for plane in (many, single):
        plane.set_plane(0, points=marks(TILTED))
        plane.set_plane(2, points=marks(HORIZON), bounds=(-20000, 0, 20000, 60000))
    cams = [0 if i % 7 == 0 else 1 + i % 2 for i in range(33)]
    assert cams.count(0) == 5
    frames = []
    for i, cam in enumerate(cams):
        n = int(rng.integers(0, 7))
        pos = np.stack([rng.uniform(0, 7500, n) + 10.0 * i, rng.uniform(500, 7000, n)], 1)
        kpts, bboxes = people(rng, pos)
        ids = rng.permutation(9)[:n].astype(np.int32)            # an id of 0 among them now and then
        frames.append((cam, kpts, bboxes, ids))
    items = [(cam, result(k, b), torch.from_numpy(ids).cuda()) for cam, k, b, ids in frames]
    outs = many.plane.update_many(items)
    assert len(outs) == 33
    for i, ((cam, kpts, bboxes, ids), item, out) in enumerate(zip(frames, items, outs)):
        exp = many.ref.update(kpts, bboxes, ids, camera=cam)
        same_outputs(out, exp, f'entry {i}', item[1])
        same_outputs(single.update(item[1], item[2], camera=cam), exp, f'entry {i} alone', item[1])
        assert cam != 1 or not exp['on'].any()
    same_all(many, [0, 1, 2], 'after 33 entries')
    assert many.ref.frame.tolist() == [5, 14, 14] and not many.ref.id[1].any() and many.ref.hits.max() >= 2
    for cam in range(3):
        live = many.plane.state(cam)['id'] != 0
        for name in STATE:
            a, b = many.plane.state(cam)[name], single.state(cam)[name]
            if a.dim() >= 1 and name != 'id':
                a, b = a[live], b[live]
            assert torch.equal(a, b), name


def test_reset_of_one_camera_set_plane_between_frames_and_a_side_stream():
    """reset(camera=1) frees camera 1's slots and leaves camera 0's tensors, both planes and every data_ptr as they
    were; set_plane between frames swaps camera 0's plane and resets it alone; frames whose results were made on a side
    stream are counted on that stream."""
    rng = np.random.default_rng(246)
    p = Pair(15, cameras=2, max_tracks=4)
    p.set_plane(0, points=marks(TILTED))
    p.set_plane(1, matrix=FRONTO)
    for cam in (0, 1):
        for f in range(2):
            step(p, *people(rng, [(2000.0 + 90 * f, 3000.0), (5000.0, 4000.0 + 50 * f)]), [1, 2], f'camera {cam} frame {f}',
                 camera=cam)
    ptrs = {k: v.data_ptr() for k, v in p.plane._state.items()}
    zero = {k: v[0].clone() for k, v in p.plane._state.items()}
    p.plane.reset(camera=1)
    p.ref.reset(1)
    assert {k: v.data_ptr() for k, v in p.plane._state.items()} == ptrs
    for k, v in zero.items():
        assert torch.equal(p.plane._state[k][0], v), k
    for k in ('id', 'frame', 'dropped'):
        assert not p.plane._state[k][1].any(), k
    same_all(p, [0, 1], 'after reset(1)')
    step(p, *people(rng, [(2100.0, 3000.0)]), [1], 'camera 1 after its reset', camera=1)
    p.set_plane(0, points=marks(HORIZON), bounds=(-30000, 0, 30000, 80000))
    assert p.ref.frame.tolist() == [0, 1] and not p.ref.id[0].any()
    same_all(p, [0, 1], 'after set_plane(0)')
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for f in range(3):
            step(p, *people(rng, [(3000.0 + 80 * f, 5000.0)]), [5], f'side stream frame {f}', camera=0)
    torch.cuda.current_stream().wait_stream(side)
    assert p.ref.frame.tolist() == [3, 1]
    p.plane.reset()
    p.ref.reset()
    same_all(p, [0, 1], 'after reset()')


def test_forty_random_frames_on_the_tilted_plane():
    """0 .. 128 poses a frame for 40 frames: ids drawn from 1 .. 140 with repeats, zeros and negatives, scores, keep
    flags and key-point scores at random, a coordinate that is not finite now and then, 96 slots so that some poses
    drop, bounds that cut the floor."""
    rng = np.random.default_rng(247)
    p = Pair(15, max_tracks=96, max_age=2, near=2500, velocity_gain=5, unit=40, origin=(-9000, 500), kpt_thr=0.3)
    p.set_plane(0, points=marks(TILTED), bounds=(-3000, 0, 3500, 9000))
    walkers = np.stack([rng.uniform(0, 7800, 140), rng.uniform(0, 7600, 140)], 1)
    placed = followed = 0
    for f in range(40):
        n = int(rng.integers(0, 129)) if f % 8 else (0, 128, 1, 127, 2)[f // 8]
        who = rng.integers(-2, 141, n)
        walkers += rng.normal(0, 12, walkers.shape)
        kpts, bboxes = people(rng, walkers[np.clip(who, 1, 140) - 1], kpt_scores=rng.uniform(0, 1, (n, 15)).astype(np.float32))
        bboxes[:, 4] = rng.uniform(0.2, 1.0, n)
        for d in np.nonzero(rng.uniform(size=n) < 0.03)[0]:
            kpts[d, rng.integers(15), rng.integers(2)] = (np.nan, np.inf, -np.inf)[rng.integers(3)]
        keep = (rng.uniform(size=n) < 0.9).astype(np.int32)
        exp, _ = step(p, kpts, bboxes, who, f'frame {f}', keep, form='dict')
        placed += int(exp['on'].sum())
        followed += int((exp['travel'] > 0).sum())
    assert placed > 400 and followed > 100 and p.ref.dropped[0] > 0 and (p.ref.id[0] != 0).sum() > 60


def test_the_bridge_into_the_monitor_the_map_the_trails_and_a_plan_picture():
    """out['floor'] of the device into the real ZoneMonitor (a zone drawn on the plan), FootfallMap and TrackTrails, and
    one draw_trails_bgr onto a 256 x 256 plan picture: states, maps, rings and the picture equal the numpy chain
    (floor_ref -> zones_ref, heat_ref, trail_ref -> trail_draw_ref)."""
    from pavenet_amd import FootfallMap, TrackTrails, ZoneMonitor, draw_trails_bgr
    rng = np.random.default_rng(248)
    kw = dict(max_tracks=8, max_age=5)
    unit, origin = 40, (-4000, 1000)                        # a 256 x 256 plan of 10.24 m a side
    p = Pair(15, unit=unit, origin=origin, **kw)
    p.set_plane(0, points=marks(TILTED))
    zone = [(40.0, 30.0), (200.0, 40.0), (180.0, 220.0), (30.0, 200.0)]
    mon, mon_ref = ZoneMonitor(15, min_frames=1, **kw), ZoneRef(15, min_frames=1, **kw)
    mon.set_zones(0, zones=[zone])
    mon_ref.set_zones(0, zones=[zone])
    fmap, fmap_ref = FootfallMap(15, size=(256, 256), **kw), HeatRef(15, (256, 256), **kw)
    trails, trails_ref = TrackTrails(15, min_step=4, **kw), TrailRef(15, min_step=4, **kw)
    start = np.stack([rng.uniform(1000, 7000, 6), rng.uniform(1500, 6500, 6)], 1)
    drift = rng.uniform(-60, 60, (6, 2))
    ids = np.arange(1, 7, dtype=np.int32)
    inside = 0
    for f in range(12):
        kpts, bboxes = people(rng, start + drift * f)
        exp, got = step(p, kpts, bboxes, ids, f'frame {f}')
        dev_ids = torch.from_numpy(ids).cuda()
        z, h, t = mon.update(got['floor'], dev_ids), fmap.update(got['floor'], dev_ids), trails.update(got['floor'], dev_ids)
        ze, he, te = (r.update(exp['kpts'], exp['bboxes'], ids) for r in (mon_ref, fmap_ref, trails_ref))
        for name in ('zones', 'dwell', 'events', 'n_events'):
            same(z[name], ze[name], f'frame {f}: zone output {name}')
        for name in ('cell', 'dwell', 'visits'):
            same(h[name], he[name], f'frame {f}: map output {name}')
        for name in ('count', 'span', 'dist', 'path'):
            same(t[name], te[name], f'frame {f}: trail output {name}')
        inside += int((ze['zones'] != 0).sum())
        want = FR.plan_points(exp, unit, origin)
        for d, pt in enumerate(want):
            if pt is not None:
                slot = int(np.nonzero(mon_ref.id[0] == ids[d])[0][0])
                assert mon_ref.pos[0, slot].tolist() == [2 * pt[0], 2 * pt[1]]
    assert inside > 0 and sum(pt is not None for pt in want) >= 4
    live = torch.from_numpy(mon_ref.id[0] != 0).cuda()
    same(mon.state(0)['pos'][live], mon_ref.pos[0][mon_ref.id[0] != 0], 'the monitor pos')
    for name in ('dwell', 'visits', 'peak'):
        same(fmap.maps(0)[name], fmap_ref.maps(0)[name], f'the map {name}')
    tl = trails_ref.id[0] != 0
    for name in ('pts', 'when'):
        same(trails.points(0)[name][torch.from_numpy(tl).cuda()], trails_ref.points(0)[name][tl], f'the rings {name}')
    picture = torch.full((256, 256, 3), 30, dtype=torch.uint8, device='cuda')
    from pavenet_amd import TrailStyle
    draw_trails_bgr(picture, trails, style=TrailStyle(thickness=3, head_radius=3))
    expect = draw_bgr(np.full((256, 256, 3), 30, np.uint8), trails_ref.drawn(0), TrailStyle(thickness=3, head_radius=3))
    assert (expect != 30).any()
    assert torch.equal(picture.cpu(), torch.from_numpy(expect))


def test_updates_allocate_no_growing_memory():
    rng = np.random.default_rng(249)
    from pavenet_amd import GroundPlane
    plane = GroundPlane(15)
    plane.set_plane(0, matrix=FRONTO)
    res, ids = result(*people(rng, [(2000.0, 2000.0), (3000.0, 2500.0)])), torch.tensor([1, 2], dtype=torch.int32, device='cuda')
    plane.update(res, ids)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    for _ in range(100):
        out = plane.update(res, ids)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - base <= 8 * 512     # (the two small outputs of a call or two)
    assert int(plane.state(0)['frame']) == 101 and out['on'].tolist() == [1, 1] and out['travel'].tolist() == [0, 0]
    assert out['speed'].tolist() == [0, 0] and int(plane.state(0)['hits'][0]) == 101
