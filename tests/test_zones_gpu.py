"""Zones and counting lines on the device (csrc/pave_zones.hip) against the rule of DESIGN section 17 in numpy
(tests/zones_ref.py): after every frame the four outputs and every state, counter and geometry tensor of the monitor
are compared with the oracle by torch.equal.  Needs an MI355X."""
import math

import numpy as np
import pytest
import torch

from tests import smooth_ref as SR
from tests import track_ref as TR
from tests import zones_cases as ZC
from tests import zones_ref as ZR
from tests.test_track_gpu import FIGURE15, figure, poses, result

pytestmark = pytest.mark.gpu

OUTPUTS = ['zones', 'dwell', 'events', 'n_events']
STATE = ['id', 'last', 'pos', 'inside', 'alerted', 'streak', 'since', 'frame', 'dropped']
COUNTS = ['occupancy', 'entered', 'exited', 'appeared', 'vanished', 'crossed']
GEOMETRY = ['n_zones', 'n_lines', 'n_vertices', 'dwell_frames', 'zones', 'lines']


@pytest.fixture(autouse=True)
def _split_gemm_mode():
    """The end-to-end test's model runs under set_batch_invariant, which needs the library's default GEMM mode,
    whatever mode an earlier module left behind."""
    from pavenet_amd import bricks
    old = bricks.get_gemm_mode()
    bricks.set_gemm_mode('bf16x3')
    yield
    bricks.set_gemm_mode(old)


class Pair:
    """A ZoneMonitor and the oracle, configured alike."""

    def __init__(self, K=15, **kw):
        from pavenet_amd.zones import ZoneMonitor
        self.mon, self.ref = ZoneMonitor(K, **kw), ZR.ZoneRef(K, **kw)

    def set_zones(self, camera, zones=(), lines=(), dwell_frames=None):
        self.mon.set_zones(camera, zones, lines, dwell_frames)
        self.ref.set_zones(camera, zones, lines, dwell_frames)


def same(got, exp, what):
    g, e = got.detach().cpu(), torch.from_numpy(np.array(exp))
    assert g.dtype == torch.int32 and e.dtype == torch.int32 and g.shape == e.shape, (what, g.dtype, tuple(g.shape), tuple(e.shape))
    assert torch.equal(g, e), f'{what}: {int((g != e).sum())} words differ, first at {(g != e).nonzero()[:4].tolist()}: ' \
                              f'{g[g != e][:4].tolist()} for {e[g != e][:4].tolist()}'


def same_outputs(got, exp, what):
    assert sorted(got) == sorted(OUTPUTS)
    for name in OUTPUTS:
        assert got[name].is_cuda
        same(got[name], exp[name], f'{what}: {name}')


def same_all(p, cameras, what, live_only=False):
    for c in cameras:
        got, exp = p.mon.state(c), p.ref.state(c)
        assert list(got) == STATE
        live = exp['id'] != 0
        for name in STATE:
            g, e = got[name], np.asarray(exp[name])
            if live_only and e.ndim >= 1 and name != 'id':
                g, e = g[torch.from_numpy(live).to(g.device)], e[live]
            same(g, e, f'{what}: camera {c} state {name}')
        got, exp = p.mon.counts(c), p.ref.counts(c)
        assert list(got) == COUNTS
        for name in COUNTS:
            same(got[name], exp[name], f'{what}: camera {c} counter {name}')
        got, exp = p.mon.geometry(c), p.ref.geometry(c)
        assert list(got) == GEOMETRY
        for name in GEOMETRY:
            same(got[name], np.asarray(exp[name]), f'{what}: camera {c} geometry {name}')
        ZC.invariant(p.ref.state(c), p.ref.counts(c))


def step(p, kpts, bboxes, ids, what, keep=None, scale=None, camera=0, form='tuple'):
    """One frame through the device and the reference; everything compared.  Returns the oracle's outputs."""
    ids = np.asarray(ids, np.int64).astype(np.int32)
    exp = p.ref.update(kpts, bboxes, ids, keep, (1.0, 1.0) if scale is None else scale, camera)
    got = p.mon.update(result(kpts, bboxes, keep, form), torch.from_numpy(ids).cuda(), scale_factor=scale, camera=camera)
    same_outputs(got, exp, what)
    same_all(p, [camera], what)
    return exp


# three zones and two lines on the paths of `scenario`'s walkers, in original-image pixels
U_ZONE = [(40, 100), (520, 100), (520, 400), (380, 400), (380, 200), (200, 200), (200, 400), (40, 400)]
SCENARIO_ZONES = [[(0, 0), (700.5, 0), (700.5, 1000), (0, 1000)], U_ZONE, [(700.5, 0), (2400, 0), (2400, 1000), (700.5, 1000)]]
SCENARIO_LINES = [((700.5, 1000), (700.5, 0)), ((0, 160.25), (2400, 150.75))]


def scenario(form, scale=(0.694, 0.7), frames=60):
    """12 people 100 px tall for 60 frames, shuffled: three stand under the U's bar, the
    others walk 2.5 px per frame to the right or to the left and half a pixel up or down, over the upright line at
    x = 700.5 between zones 0 and 2 and over the slanted one; person 3 is away for 2 frames and person 5 for 7;
    every frame carries poses that take no part: keep = 0 (dict form), a score at the threshold, NaN and inf
    coordinates, a NaN score.  Yields (kpts, bboxes, keep, people there)."""
    rng = np.random.default_rng(191)
    start = np.stack([60.0 + 150.0 * np.arange(12), 40.0 + 11.0 * np.arange(12)], 1)
    speed = np.stack([np.where(np.arange(12) % 2 == 0, 2.5, -2.5), np.where(np.arange(12) % 3 == 0, 0.5, -0.5)], 1)
    speed[:3] = 0.0
    for f in range(frames):
        there = [p for p in range(12) if not (p == 3 and 10 <= f < 12) and not (p == 5 and 20 <= f < 27)]
        kpts, bboxes = poses(rng, FIGURE15, (start + speed * f)[there], scale=scale)
        junk_k, junk_b = poses(rng, FIGURE15, rng.uniform(0, 1500, (5, 2)), scale=scale)
        junk_b[1, 4] = 0.3                       # not > score_thr
        junk_k[2, rng.integers(15), 0] = np.nan
        junk_b[3, 2] = np.inf
        junk_b[4, 4] = np.nan
        keep = np.ones(len(there) + 5, np.int32)
        keep[len(there)] = 0                     # junk 0: a good pose NMS removed
        if form == 'tuple':                      # (no keep there: the pose is left out)
            junk_k, junk_b = junk_k[1:], junk_b[1:]
            keep = None
        kpts, bboxes = np.concatenate([kpts, junk_k]), np.concatenate([bboxes, junk_b])
        order = rng.permutation(len(bboxes))
        yield kpts[order], bboxes[order], None if keep is None else keep[order], there


@pytest.mark.parametrize('form', ['tuple', 'dict'])
def test_random_scenario(form):
    """`scenario` at scale (0.694, 0.7) under the ids of a real PoseTracker (max_age 10; the monitor's is 5, so person
    5's slot expires inside zone 2 and the id is born again), with a dwell time on the U.  Every kind of event occurs,
    so an idle kernel cannot pass."""
    from pavenet_amd.tracking import PoseTracker
    scale = (0.694, 0.7)
    tracker = PoseTracker(15, max_age=10)
    p = Pair(15, max_age=5, max_tracks=16)
    p.set_zones(0, SCENARIO_ZONES, SCENARIO_LINES, dwell_frames=[0, 6, 0])
    kinds = np.zeros(8, np.int64)
    for f, (kpts, bboxes, keep, there) in enumerate(scenario(form)):
        ids = tracker.update(result(kpts, bboxes, keep, form), scale_factor=scale).cpu().numpy()
        out = step(p, kpts, bboxes, ids, f'{form} frame {f}', keep, scale, form=form)
        assert (ids >= 1).sum() == len(there)
        assert not out['zones'][ids == 0].any() and not out['dwell'][ids == 0].any()
        kinds += np.bincount(out['events'][:int(out['n_events']), 0], minlength=8)
    assert p.ref.frame[0] == 60 and p.ref.dropped[0] == 0
    print('events by kind (ENTER, EXIT, DWELL, APPEAR, VANISH, CROSS_FWD, CROSS_BACK):', kinds[1:].tolist())
    assert kinds[0] == 0 and (kinds[1:] >= 1).all(), kinds.tolist()


@pytest.mark.parametrize('script', ZC.SCRIPTS, ids=lambda s: s.__name__)
def test_hand_worked_scripts_on_the_device(script):
    class Harness:
        def __init__(self, K, **kw):
            self.p = Pair(K, **kw)
            self.p.mon._allocate(torch.device('cuda', torch.cuda.current_device()))
            self.frames = 0

        def set_zones(self, zones, lines, dwell_frames=None, camera=0):
            self.p.set_zones(camera, zones, lines, dwell_frames)
            same_all(self.p, range(self.p.ref.cameras), f'{script.__name__} set_zones', live_only=True)

        def frame(self, kpts, bboxes, ids, keep=None, camera=0):
            self.frames += 1
            form = 'tuple' if keep is None else 'dict'
            return step(self.p, kpts, bboxes, ids, f'{script.__name__} frame {self.frames}',
                        None if keep is None else np.asarray(keep, np.int32), camera=camera, form=form)

        def poke(self, field, index, value, camera=0):
            at = (camera,) + tuple(index)
            getattr(self.p.ref, field)[at] = value
            self.p.mon._state[field][at] = torch.from_numpy(np.asarray(getattr(self.p.ref, field)[at])).cuda()

        def get(self, field, camera=0):
            views = dict(self.p.mon.state(camera), **self.p.mon.counts(camera))
            return views[field].cpu().numpy()
    script(Harness)


def _ring(cx, cy, r, n=16, turn=0.0):
    return [(cx + r * math.cos(turn + 2 * math.pi * i / n), cy + r * math.sin(turn + 2 * math.pi * i / n)) for i in range(n)]


@pytest.mark.parametrize('geometry', ['none', 'full'])
@pytest.mark.parametrize('K', [1, 32])
def test_shape_edges(K, geometry):
    """K = 1 and K = 32, with no zone and no line, and with 8 zones of 16 vertices and 8 lines; the first frame, a
    frame without poses (the clock still runs), a frame without a valid pose, odd counts of poses."""
    rng = np.random.default_rng(196 + K)
    fig = figure(K)
    p = Pair(K, max_age=3, max_tracks=7, min_frames=1, anchor_kpts=(0,) if K == 1 else (31, 5, 0, 17))
    if geometry == 'full':
        p.set_zones(0, [_ring(150 + 60 * z, 140 + 5 * z, 70 + 8 * z, turn=0.1 * z) for z in range(8)],
                    [((100 + 70 * l, 0), (130 + 70 * l, 400)) if l % 2 else ((140 + 70 * l, 400), (90 + 70 * l, 0))
                     for l in range(8)], dwell_frames=[2, 0, 3, 0, 1, 0, 0, 4])
    pos = np.stack([40.0 + 130.0 * np.arange(5), np.full(5, 30.0)], 1)
    events = 0
    for f in range(10):
        kpts, bboxes = poses(rng, fig, pos + (9.0 * f, 2.0 * f), jitter=0.005,
                             kpt_scores=rng.uniform(-0.2, 1.0, (5, K)).astype(np.float32))
        ids = np.arange(1, 6)
        if f == 3:
            kpts, bboxes, ids = kpts[:0], bboxes[:0], ids[:0]
        if f == 4:
            bboxes[:, 4] = 0.1
        if f == 6:
            kpts, bboxes, ids = kpts[:3], bboxes[:3], ids[:3]
        order = rng.permutation(len(bboxes))
        out = step(p, kpts[order], bboxes[order], ids[order], f'K = {K} {geometry} frame {f}')
        events += int(out['n_events'])
    assert p.ref.frame[0] == 10 and sorted(p.ref.id[0].tolist()) == [0, 0, 1, 2, 3, 4, 5]
    assert (events > 20) if geometry == 'full' else (events == 0)


def _everywhere(z):
    return [(0, 0), (2000 + z, 0), (2000 + z, 1100 + z), (0, 1100 + z)]


def test_full_capacity_and_more_events_than_rows():
    """N = 128 on S = 128 with every pose inside all 8 zones at its birth: 1 024 APPEAR events against max_events =
    256 -- n_events says 1 024, the table holds the first 256 -- then a 129th id is dropped."""
    rng = np.random.default_rng(198)
    p = Pair(15)
    p.set_zones(0, [_everywhere(z) for z in range(8)], [((1000, 0), (1000, 1100))])
    pos = np.stack([30.0 + 60.0 * (np.arange(128) % 16), 20.0 + 120.0 * (np.arange(128) // 16)], 1)
    for f in range(3):
        kpts, bboxes = poses(rng, FIGURE15, pos + 1.5 * f)
        order = rng.permutation(128)
        out = step(p, kpts[order], bboxes[order], (np.arange(128) + 1000)[order], f'frame {f}')
        if f == 0:
            assert int(out['n_events']) == 1024 and (out['events'][:, 0] == ZR.APPEAR).all()
            assert out['events'][:, 3].tolist() == [d for d in range(32) for _ in range(8)]
            assert (out['zones'] == 255).all()
    assert (p.ref.id[0] != 0).all() and p.ref.dropped[0] == 0 and p.ref.occupancy[0].tolist() == [128] * 8
    kpts, bboxes = poses(rng, FIGURE15, pos[:2])
    out = step(p, kpts, bboxes, [5000, 1000], 'no slot left')
    assert p.ref.dropped[0] == 1 and out['zones'].tolist() == [0, 255]


def test_one_row_of_events():
    """max_events = 1: the table is one row, the first event of the fixed order, and n_events counts them all."""
    rng = np.random.default_rng(199)
    p = Pair(15, max_events=1, max_age=1, min_frames=1)
    p.set_zones(0, [_everywhere(0), _everywhere(1)], [((300, 0), (300, 1100))])
    pos = np.stack([100.0 + 150.0 * np.arange(4), np.full(4, 50.0)], 1)
    counts = []
    for f, who in enumerate(([0, 1, 2, 3], [0, 1], [], [], [2, 3, 0])):
        kpts, bboxes = poses(rng, FIGURE15, (pos + 60.0 * f)[who])
        out = step(p, kpts, bboxes, np.asarray(who, np.int32) + 1, f'frame {f}')
        assert out['events'].shape == (1, 5)
        counts.append(int(out['n_events']))
    assert counts == [8, 1, 4, 4, 6], counts     # births; a crossing; two expiries of two; two more; three births


def _camera_frames(rng, n_cams, schedule):
    """schedule: the camera of every entry -> [(camera, kpts, bboxes, ids)], every camera with its own walking
    people; an id is now and then 0 or a duplicate."""
    clock = [0] * n_cams
    out = []
    for c in schedule:
        P = 3 + c
        pos = np.stack([50.0 + 140.0 * np.arange(P), np.full(P, 40.0 + 9.0 * c)], 1) + (12.0 + 3 * c) * clock[c]
        kpts, bboxes = poses(rng, FIGURE15, pos)
        ids = np.arange(1, P + 1, dtype=np.int32) + 10 * c
        if clock[c] % 4 == 2:
            ids[0] = 0
        if clock[c] % 5 == 3:
            ids[1] = ids[2]
        order = rng.permutation(P)
        out.append((c, kpts[order], bboxes[order], ids[order]))
        clock[c] += 1
    return out


def _items(frames, form='tuple'):
    return [(c, result(k, b, form=form), torch.from_numpy(i).cuda()) for c, k, b, i in frames]


def _three_cameras(p):
    p.set_zones(0, [[(0, 0), (250, 0), (250, 500), (0, 500)], U_ZONE], [((300, 500), (300, 0))], dwell_frames=[3, 0])
    p.set_zones(1, [_ring(300, 150, 120)], [((200, 0), (260, 500)), ((420, 500), (400, 0))])
    p.set_zones(2, [[(100 * z, 0), (100 * z + 150, 0), (100 * z + 150, 600)] for z in range(5)], [], dwell_frames=[0, 2, 0, 2, 0])


def test_update_many_equals_single_calls():
    """Three cameras with different geometry, camera 1 with three frames in a row, 33 entries (two launches):
    update_many == one call at a time == the reference.  reset(camera=1) and set_zones(1, ...) leave cameras 0 and
    2 bit-identical; garbage in freed slots does not matter."""
    rng = np.random.default_rng(201)
    schedule = [0, 1, 1, 1, 2] + [int(c) for c in rng.integers(0, 3, 28)]
    assert len(schedule) == 33
    frames = _camera_frames(rng, 3, schedule)
    kw = dict(cameras=3, max_tracks=9, max_age=2, min_frames=1)
    many, single = Pair(15, **kw), Pair(15, **kw)
    _three_cameras(many)
    _three_cameras(single)
    got = many.mon.update_many(_items(frames))
    assert len(got) == 33
    total = 0
    for i, (c, k, b, ids) in enumerate(frames):
        exp = many.ref.update(k, b, ids, camera=c)
        single.ref.update(k, b, ids, camera=c)
        one = single.mon.update(result(k, b, form='dict'), torch.from_numpy(ids).cuda(), camera=c)
        same_outputs(one, exp, f'single entry {i}')
        same_outputs(got[i], exp, f'many entry {i}')
        total += int(exp['n_events'])
    same_all(many, range(3), 'update_many')
    same_all(single, range(3), 'single calls')
    assert int(many.ref.frame.sum()) == 33 and many.ref.frame.min() >= 3 and total > 30

    def snapshot(cams):
        return {c: [t.clone() for views in (many.mon.state(c), many.mon.counts(c), many.mon.geometry(c))
                    for t in views.values()] for c in cams}

    def unchanged(before, what):
        for c, tensors in before.items():
            assert all(torch.equal(a, b) for a, b in zip(snapshot([c])[c], tensors)), f'camera {c} after {what}'
    before = snapshot((0, 2))
    ptrs = [t.data_ptr() for t in many.mon._state.values()]
    for name in ('last', 'pos', 'inside', 'alerted', 'streak', 'since'):      # garbage where camera 1 kept its tracks
        many.mon._state[name][1].fill_(-7)
    many.mon.reset(camera=1)
    many.ref.reset(camera=1)
    unchanged(before, 'reset(1)')
    assert [t.data_ptr() for t in many.mon._state.values()] == ptrs
    more = _camera_frames(rng, 3, [1, 0, 1, 2, 1])
    got = many.mon.update_many(_items(more), scale_factor=[1.0] * 5)
    for i, (c, k, b, ids) in enumerate(more):
        same_outputs(got[i], many.ref.update(k, b, ids, camera=c), f'after reset: entry {i}')
    assert many.ref.frame[1] == 3
    same_all(many, [0, 2], 'after reset')
    same_all(many, [1], 'after reset', live_only=True)
    before = snapshot((0, 2))
    many.set_zones(1, [U_ZONE], [((10, 10), (600, 300))], dwell_frames=[1])
    unchanged(before, 'set_zones(1)')
    assert [t.data_ptr() for t in many.mon._state.values()] == ptrs
    assert int(many.mon.state(1)['frame']) == 0 and not many.mon.counts(1)['appeared'].any()
    more = _camera_frames(rng, 3, [1, 1, 2, 1, 0])
    got = many.mon.update_many(_items(more))
    for i, (c, k, b, ids) in enumerate(more):
        same_outputs(got[i], many.ref.update(k, b, ids, camera=c), f'after set_zones: entry {i}')
    same_all(many, [0, 2], 'after set_zones')
    same_all(many, [1], 'after set_zones', live_only=True)
    many.mon.reset()
    assert all(int(many.mon.state(c)[n].sum()) == 0 for c in range(3) for n in ('id', 'frame', 'dropped'))
    assert all(not t.any() for c in range(3) for t in many.mon.counts(c).values())
    assert int(many.mon.geometry(0)['n_zones']) == 2


def test_seven_frames_of_one_camera_in_one_launch():
    """Frame f + 1 reads what frame f stored, through one block: people who walk through zones and over a line, one
    who is away for two frames (gap 3 = max_age), a slot that expires inside a zone (gap 4: VANISH) and is born
    again (APPEAR) within the launch."""
    rng = np.random.default_rng(203)
    p = Pair(15, max_age=3, max_tracks=4, min_frames=1)
    p.set_zones(0, [[(0, 0), (270, 0), (270, 500), (0, 500)], [(270, 0), (2000, 0), (2000, 500), (270, 500)]],
                [((270, 500), (270, 0))], dwell_frames=[2, 2])
    pos = np.stack([50.0 + 140.0 * np.arange(4), np.full(4, 40.0)], 1)
    frames = []
    for f in range(7):
        kpts, bboxes = poses(rng, FIGURE15, pos + (15.0 * f, 1.0 * f))
        there = [q for q in range(4) if not (q == 1 and f in (2, 3)) and not (q == 2 and f in (1, 2, 3))]
        order = rng.permutation(len(there))
        frames.append((0, kpts[there][order], bboxes[there][order], (np.asarray(there, np.int32) + 1)[order]))
    got = p.mon.update_many(_items(frames))
    kinds = np.zeros(8, np.int64)
    for f, (_, k, b, ids) in enumerate(frames):
        exp = p.ref.update(k, b, ids)
        same_outputs(got[f], exp, f'frame {f}')
        kinds += np.bincount(exp['events'][:int(exp['n_events']), 0], minlength=8)
    same_all(p, [0], 'seven frames')
    assert p.ref.frame[0] == 7 and sorted(p.ref.id[0].tolist()) == [1, 2, 3, 4]
    assert kinds[ZR.VANISH] == 1 and kinds[ZR.APPEAR] == 5 and kinds[ZR.CROSS_FWD] >= 1 and kinds[ZR.DWELL] >= 1, kinds.tolist()


def test_live_results_tracked_smoothed_and_watched():
    """Five NV12 frames through preprocess_surfaces_nv12 -> LiveVideoPose -> PoseTracker.update ->
    PoseSmoother.smooth -> ZoneMonitor.update(steady, ids, scale_factor=None), against the three oracles in that
    order; device values come to the host only afterwards."""
    from pavenet_amd.live import LiveVideoPose
    from pavenet_amd.preprocess import preprocess_surfaces_nv12
    from pavenet_amd.smoothing import PoseSmoother
    from pavenet_amd.tracking import PoseTracker
    from tests.test_live_gpu import _model
    from tests.test_render_ids_gpu import _surface
    m = _model(3)
    K = m.bbox_head.num_keypoints
    surfaces = [_surface(96, 120, 128, seed=500 + i).cuda() for i in range(5)]
    img, meta = preprocess_surfaces_nv12(surfaces, 120, img_scale=(160, 128), size_divisor=32)
    live = LiveVideoPose(m, meta, max_push=1)
    kw = dict(score_thr=0.0, max_tracks=128)
    tracker, track_ref = PoseTracker(K, **kw), TR.TrackRef(K, **kw)
    smoother, smooth_ref = PoseSmoother(K, **kw), SR.SmoothRef(K, **kw)
    p = Pair(K, min_frames=1, anchor='centre', **kw)
    p.set_zones(0, [[(0, 0), (60, 0), (60, 96), (0, 96)], [(30, 20), (100, 10), (110, 80), (60, 50), (20, 90)]],
                [((60, 96), (60, 0)), ((0, 48), (120, 48))], dwell_frames=[2, 1])
    got = []
    for i in range(5):
        got += live.push(img[i])
    got += live.flush()
    assert [c for c, _ in got] == [0, 1, 2, 3, 4]
    kept = []
    for c, res in got:
        ids = tracker.update(res, scale_factor=meta['scale_factor'])
        steady = smoother.smooth(res, ids, scale_factor=meta['scale_factor'])
        kept.append((ids, steady, p.mon.update(steady, ids, scale_factor=None)))
    scale = tuple(float(v) for v in meta['scale_factor'][:2])
    tracked = 0
    for (c, res), (ids, steady, out) in zip(got, kept):
        bboxes, _, kpts = (t.cpu().numpy() for t in res)
        exp_ids = track_ref.update(kpts, bboxes, None, scale)
        assert torch.equal(ids.cpu(), torch.from_numpy(exp_ids)), c
        exp_k, exp_b = smooth_ref.smooth(kpts, bboxes, exp_ids, None, scale)
        assert torch.equal(steady[2].cpu().view(torch.int32), torch.from_numpy(exp_k).view(torch.int32)), c
        same_outputs(out, p.ref.update(exp_k, exp_b, exp_ids), f'frame {c}')
        tracked += int((exp_ids >= 1).sum())
    same_all(p, [0], 'live')
    assert tracked > 0


def test_calls_allocate_no_growing_memory():
    """The allocator's peak does not grow over 100 calls, and the state and geometry tensors stay where they are."""
    rng = np.random.default_rng(202)
    p = Pair(15)
    p.set_zones(0, SCENARIO_ZONES, SCENARIO_LINES)
    mon = p.mon
    pos = np.stack([40.0 + 150.0 * np.arange(6), np.full(6, 30.0)], 1)
    frames = [result(*poses(rng, FIGURE15, pos + f)) for f in range(10)]
    ids = torch.arange(1, 7, dtype=torch.int32).cuda()
    for f in range(3):
        mon.update(frames[f], ids)
    ptrs = [t.data_ptr() for t in mon._state.values()]

    def span(calls):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        for f in range(calls):
            mon.update(frames[f % 10], ids)
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated()
    early, late = span(10), span(100)
    print(f'peak bytes allocated: 10 calls {early}, 100 calls {late}')
    assert late <= early
    mon.reset()
    mon.update(frames[0], ids)
    mon.set_zones(0, SCENARIO_ZONES[:1], [])
    mon.update(frames[0], ids)
    assert [t.data_ptr() for t in mon._state.values()] == ptrs
