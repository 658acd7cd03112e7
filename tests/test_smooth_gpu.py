"""Steady poses on the device (csrc/pave_smooth.hip) against the rule of DESIGN section 16 in numpy
(tests/smooth_ref.py): after every frame the outputs are compared as int32 bit patterns (the NaN of an unusable pose
included) and every tensor of the smoother's state by torch.equal.  Needs an MI355X."""
import numpy as np
import pytest
import torch

from tests import smooth_cases as SC
from tests import smooth_ref as SR
from tests import track_ref as TR
from tests.test_track_gpu import FIGURE15, figure, poses, result

pytestmark = pytest.mark.gpu

STATE = ['id', 'last', 'pos', 'vel', 'frame', 'dropped']


@pytest.fixture(autouse=True)
def _split_gemm_mode():
    """The end-to-end test's model runs under set_batch_invariant, which needs the library's default GEMM mode,
    whatever mode an earlier module left behind."""
    from pavenet_amd import bricks
    old = bricks.get_gemm_mode()
    bricks.set_gemm_mode('bf16x3')
    yield
    bricks.set_gemm_mode(old)


def pair(K=15, **kw):
    from pavenet_amd.smoothing import PoseSmoother
    return PoseSmoother(K, **kw), SR.SmoothRef(K, **kw)


def same_bits(got, exp, what):
    g, e = got.detach().cpu().contiguous().view(torch.int32), torch.from_numpy(np.ascontiguousarray(exp)).view(torch.int32)
    assert g.shape == e.shape, (what, tuple(g.shape), tuple(e.shape))
    assert torch.equal(g, e), f'{what}: {int((g != e).sum())} words differ, first at {(g != e).nonzero()[:4].tolist()}'


def same_state(smoother, ref, cameras, what, live_only=False):
    for c in cameras:
        got, exp = smoother.state(c), ref.state(c)
        assert list(got) == STATE
        live = exp['id'] != 0
        for name in STATE:
            g, e = got[name].cpu(), torch.from_numpy(np.asarray(exp[name]))
            assert g.dtype == torch.int32 and g.shape == e.shape, (what, c, name)
            if live_only and e.dim() >= 1 and name != 'id':
                g, e = g[live], e[live]
            assert torch.equal(g, e), f'{what}: camera {c} state {name}'


def parts(res):
    """(kpts, bboxes) of a result in either form, without its batch axis."""
    if isinstance(res, dict):
        return res['kpts'].reshape(-1, *res['kpts'].shape[-2:]), res['bboxes'].reshape(-1, 5)
    return res[2], res[0]


def step(smoother, ref, kpts, bboxes, ids, what, keep=None, scale=None, camera=0, form='tuple'):
    """One frame through the device and the reference; everything compared.  Returns the outputs (numpy)."""
    ids = np.asarray(ids, np.int32)
    exp_k, exp_b = ref.smooth(kpts, bboxes, ids, keep, (1.0, 1.0) if scale is None else scale, camera)
    given = result(kpts, bboxes, keep, form)
    got = smoother.smooth(given, torch.from_numpy(ids).cuda(), scale_factor=scale, camera=camera)
    if form == 'tuple':
        assert isinstance(got, tuple) and len(got) == 3 and got[1] is given[1]
    else:
        assert sorted(got) == ['bboxes', 'keep', 'kpts'] and got['keep'] is given['keep']
        assert got['kpts'].shape == given['kpts'].shape and got['bboxes'].shape == given['bboxes'].shape
    got_k, got_b = parts(got)
    assert got_k.dtype == got_b.dtype == torch.float32 and got_k.is_cuda and got_b.is_cuda
    same_bits(got_k, exp_k, f'{what}: out kpts')
    same_bits(got_b, exp_b, f'{what}: out bboxes')
    same_state(smoother, ref, [camera], what)
    return exp_k, exp_b


@pytest.mark.parametrize('form', ['tuple', 'dict'])
def test_random_scenario(form):
    """12 people for 60 frames at scale (0.694, 0.7), shuffled, under the ids of a real PoseTracker (max_age 10);
    one leaves for 2 frames and one for 7 (the smoother's max_age is 5: its slot expires and the id is born again);
    every frame carries poses that are not filtered: keep = 0 (dict form), a score at the threshold, NaN and inf
    coordinates, a NaN score."""
    from pavenet_amd.tracking import PoseTracker
    rng = np.random.default_rng(171)
    scale = (0.694, 0.7)
    tracker = PoseTracker(15, max_age=10)
    smoother, ref = pair(15, max_age=5, max_tracks=16)
    start = np.stack([60.0 + 150.0 * np.arange(12), 40.0 + 11.0 * np.arange(12)], 1)
    speed = rng.uniform(-3, 3, (12, 2))
    speed[:3] = 0.0
    filtered = moved = 0
    for f in range(60):
        there = [p for p in range(12) if not (p == 3 and 10 <= f < 12) and not (p == 5 and 20 <= f < 27)]
        kpts, bboxes = poses(rng, FIGURE15, (start + speed * f)[there], scale=scale)
        junk_k, junk_b = poses(rng, FIGURE15, rng.uniform(0, 1500, (5, 2)), scale=scale)
        junk_b[1, 4] = 0.3                       # not > score_thr
        junk_k[2, rng.integers(15), 0] = np.nan
        junk_b[3, 2] = np.inf
        junk_b[4, 4] = np.nan
        if f % 7 == 3:
            junk_k[2, 4, 1] = -np.inf
        keep = np.ones(len(there) + 5, np.int32)
        keep[len(there)] = 0                     # junk 0: a good pose NMS removed
        if form == 'tuple':                      # (no keep there: the pose is left out)
            junk_k, junk_b = junk_k[1:], junk_b[1:]
            keep = None
        kpts, bboxes = np.concatenate([kpts, junk_k]), np.concatenate([bboxes, junk_b])
        order = rng.permutation(len(bboxes))
        kpts, bboxes, keep = kpts[order], bboxes[order], None if keep is None else keep[order]
        ids = tracker.update(result(kpts, bboxes, keep, form), scale_factor=scale).cpu().numpy()
        out_k, _ = step(smoother, ref, kpts, bboxes, ids, f'{form} frame {f}', keep, scale, form=form)
        assert (ids >= 1).sum() == len(there)
        filtered += int((ids >= 1).sum())
        usable = np.isfinite(kpts[..., :2]).all((1, 2)) & np.isfinite(bboxes[:, :4]).all(1)
        with np.errstate(invalid='ignore'):
            snapped = np.rint(kpts[..., :2] / np.asarray(scale, np.float32) * np.float32(4)) / np.float32(4)
        moved += int((out_k[ids >= 1][..., :2] != snapped[ids >= 1]).any((1, 2)).sum())
        assert (out_k[usable & (ids == 0)][..., :2] == snapped[usable & (ids == 0)]).all()
        assert np.isnan(out_k[~usable][..., :2]).all() and (~usable).sum() >= 2
    assert ref.frame[0] == 60
    # the filter was at work, not the pass-through: the three people who stand still never come out as detected
    assert filtered == 60 * 12 - 2 - 7 and moved >= 3 * 59


@pytest.mark.parametrize('script', SC.SCRIPTS, ids=lambda s: s.__name__)
def test_hand_worked_scripts_on_the_device(script):
    class Harness:
        def __init__(self, K, **kw):
            self.smoother, self.ref = pair(K, **kw)
            self.smoother._allocate(torch.device('cuda', torch.cuda.current_device()))
            self.frames = 0

        def frame(self, kpts, bboxes, ids, keep=None):
            self.frames += 1
            form = 'tuple' if keep is None else 'dict'
            return step(self.smoother, self.ref, kpts, bboxes, ids, f'{script.__name__} frame {self.frames}',
                        None if keep is None else np.asarray(keep, np.int32), form=form)

        def poke(self, field, index, value):
            getattr(self.ref, field)[(0,) + tuple(index)] = value
            self.smoother._state[field][(0,) + tuple(index)] = torch.from_numpy(
                np.asarray(getattr(self.ref, field)[(0,) + tuple(index)])).cuda()

        def get(self, field):
            return self.smoother.state(0)[field].cpu().numpy()
    script(Harness)


@pytest.mark.parametrize('K', [1, 32])
def test_shape_edges(K):
    """K = 1 and K = 32; the first frame, a frame without poses (the clock still runs), a frame without a valid
    pose, odd counts of poses."""
    rng = np.random.default_rng(176 + K)
    fig = figure(K)
    smoother, ref = pair(K, max_age=3, max_tracks=7)
    pos = np.stack([40.0 + 130.0 * np.arange(5), np.full(5, 30.0)], 1)
    for f in range(8):
        kpts, bboxes = poses(rng, fig, pos + (1.0 * f, 0.0), jitter=0.005,
                             kpt_scores=rng.uniform(-0.2, 1.0, (5, K)).astype(np.float32))
        ids = np.arange(1, 6)
        if f == 3:
            kpts, bboxes, ids = kpts[:0], bboxes[:0], ids[:0]
        if f == 4:
            bboxes[:, 4] = 0.1
        if f == 6:
            kpts, bboxes, ids = kpts[:3], bboxes[:3], ids[:3]
        order = rng.permutation(len(bboxes))
        step(smoother, ref, kpts[order], bboxes[order], ids[order], f'K = {K} frame {f}')
    assert ref.frame[0] == 8 and sorted(ref.id[0].tolist()) == [0, 0, 1, 2, 3, 4, 5]


def test_full_capacity_128_poses_on_128_slots():
    """N = 128 on S = 128, K = 32: 4352 points of a frame, every slot taken, in a shuffled order."""
    rng = np.random.default_rng(178)
    fig = figure(32)
    smoother, ref = pair(32)
    pos = np.stack([30.0 + 60.0 * (np.arange(128) % 16), 20.0 + 120.0 * (np.arange(128) // 16)], 1)
    for f in range(3):
        kpts, bboxes = poses(rng, fig, pos + 1.5 * f)
        order = rng.permutation(128)
        step(smoother, ref, kpts[order], bboxes[order], (np.arange(128) + 1000)[order], f'frame {f}')
    assert (ref.id[0] != 0).all() and ref.dropped[0] == 0
    kpts, bboxes = poses(rng, fig, pos[:2])
    step(smoother, ref, kpts, bboxes, [5000, 1000], 'no slot left')
    assert ref.dropped[0] == 1


def _camera_frames(rng, n_cams, schedule):
    """schedule: the camera of every entry -> [(camera, kpts, bboxes, ids)], every camera with its own walking
    people; an id is now and then 0 or a duplicate."""
    clock = [0] * n_cams
    out = []
    for c in schedule:
        P = 3 + c
        pos = np.stack([50.0 + 140.0 * np.arange(P), np.full(P, 40.0 + 9.0 * c)], 1) + (2.0 + c) * clock[c]
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


def test_smooth_many_equals_single_calls():
    """Three cameras, camera 1 with three frames in a row, 33 entries (two launches): smooth_many == one call at a
    time == the reference; reset(camera=1) leaves cameras 0 and 2 as they are; garbage in freed slots does not
    matter."""
    from pavenet_amd.smoothing import PoseSmoother
    rng = np.random.default_rng(181)
    schedule = [0, 1, 1, 1, 2] + [int(c) for c in rng.integers(0, 3, 28)]
    assert len(schedule) == 33
    frames = _camera_frames(rng, 3, schedule)
    kw = dict(cameras=3, max_tracks=9, max_age=2)
    many, single, ref = PoseSmoother(15, **kw), PoseSmoother(15, **kw), SR.SmoothRef(15, **kw)
    got = many.smooth_many(_items(frames))
    assert len(got) == 33
    for i, (c, k, b, ids) in enumerate(frames):
        exp_k, exp_b = ref.smooth(k, b, ids, camera=c)
        one = single.smooth(result(k, b, form='dict'), torch.from_numpy(ids).cuda(), camera=c)
        same_bits(one['kpts'][0], exp_k, f'entry {i} kpts')
        same_bits(one['bboxes'][0], exp_b, f'entry {i} bboxes')
        assert torch.equal(got[i][2].view(torch.int32), one['kpts'][0].view(torch.int32)), f'entry {i}'
        assert torch.equal(got[i][0].view(torch.int32), one['bboxes'][0].view(torch.int32)), f'entry {i}'
    same_state(many, ref, range(3), 'smooth_many')
    same_state(single, ref, range(3), 'single calls')
    assert int(ref.frame.sum()) == 33 and ref.frame.min() >= 3

    before = {c: {n: t.clone() for n, t in many.state(c).items()} for c in (0, 2)}
    ptrs = [t.data_ptr() for t in many._state.values()]
    for name in ('last', 'pos', 'vel'):                    # garbage where camera 1 kept its tracks
        many._state[name][1].fill_(-7)
    many.reset(camera=1)
    ref.reset(camera=1)
    for c in (0, 2):
        assert all(torch.equal(many.state(c)[n], before[c][n]) for n in STATE), f'camera {c} after reset(1)'
    assert [t.data_ptr() for t in many._state.values()] == ptrs
    more = _camera_frames(rng, 3, [1, 0, 1, 2, 1])
    got = many.smooth_many(_items(more), scale_factor=[1.0] * 5)
    for i, (c, k, b, ids) in enumerate(more):
        exp_k, exp_b = ref.smooth(k, b, ids, camera=c)
        same_bits(got[i][2], exp_k, f'after reset: entry {i} kpts')
        same_bits(got[i][0], exp_b, f'after reset: entry {i} bboxes')
    assert ref.frame[1] == 3
    same_state(many, ref, [0, 2], 'after reset')
    same_state(many, ref, [1], 'after reset', live_only=True)
    # (a live slot's points are all written at its birth: what the garbage left is in free slots only)
    many.reset()
    assert all(int(many.state(c)[n].sum()) == 0 for c in range(3) for n in ('id', 'frame', 'dropped'))


def test_seven_frames_of_one_camera_in_one_launch():
    """Frame f + 1 reads what frame f stored, through one block: people who move, one who is away for two frames
    (gap 3 = max_age), a slot that expires (gap 4) and is born again within the launch."""
    rng = np.random.default_rng(183)
    smoother, ref = pair(15, max_age=3, max_tracks=4)
    pos = np.stack([50.0 + 140.0 * np.arange(4), np.full(4, 40.0)], 1)
    frames = []
    for f in range(7):
        kpts, bboxes = poses(rng, FIGURE15, pos + (3.0 * f, 1.0 * f))
        there = [p for p in range(4) if not (p == 1 and f in (2, 3)) and not (p == 2 and f in (1, 2, 3))]
        order = rng.permutation(len(there))
        frames.append((0, kpts[there][order], bboxes[there][order], (np.asarray(there, np.int32) + 1)[order]))
    got = smoother.smooth_many(_items(frames))
    for f, (_, k, b, ids) in enumerate(frames):
        exp_k, exp_b = ref.smooth(k, b, ids)
        same_bits(got[f][2], exp_k, f'frame {f} kpts')
        same_bits(got[f][0], exp_b, f'frame {f} bboxes')
    same_state(smoother, ref, [0], 'seven frames')
    assert ref.frame[0] == 7 and sorted(ref.id[0].tolist()) == [1, 2, 3, 4]


def test_live_results_tracked_smoothed_and_drawn():
    """Five NV12 frames through preprocess_surfaces_nv12 -> LiveVideoPose -> PoseTracker.update ->
    PoseSmoother.smooth -> draw_poses_nv12(scale_factor=None, ids=) on their own surfaces, against the three oracles
    in that order; device values come to the host only afterwards."""
    from pavenet_amd.live import LiveVideoPose
    from pavenet_amd.preprocess import preprocess_surfaces_nv12
    from pavenet_amd.render import DIGIT_FONT, TrackStyle, draw_poses_nv12
    from pavenet_amd.smoothing import PoseSmoother
    from pavenet_amd.tracking import PoseTracker
    from tests import render_ids_ref as IR
    from tests.test_live_gpu import _model
    from tests.test_render_ids_gpu import _surface
    m = _model(3)
    K = m.bbox_head.num_keypoints
    befores = [_surface(96, 120, 128, seed=400 + i) for i in range(5)]
    surfaces = [b.cuda() for b in befores]
    img, meta = preprocess_surfaces_nv12(surfaces, 120, img_scale=(160, 128), size_divisor=32)
    live = LiveVideoPose(m, meta, max_push=1)
    kw = dict(score_thr=0.0, max_tracks=128)
    tracker, track_ref = PoseTracker(K, **kw), TR.TrackRef(K, **kw)
    smoother, smooth_ref = PoseSmoother(K, **kw), SR.SmoothRef(K, **kw)
    style = TrackStyle(K, score_thr=-1.0, draw_boxes=True, label_scale=1)
    got = []
    for i in range(5):
        got += live.push(img[i])
    got += live.flush()
    assert [c for c, _ in got] == [0, 1, 2, 3, 4]
    kept = []
    for c, res in got:
        ids = tracker.update(res, scale_factor=meta['scale_factor'])
        steady = smoother.smooth(res, ids, scale_factor=meta['scale_factor'])
        assert steady[1] is res[1]
        draw_poses_nv12(surfaces[c], 120, steady, scale_factor=None, style=style, ids=ids)
        kept.append((ids, steady))
    scale = tuple(float(v) for v in meta['scale_factor'][:2])
    tracked = 0
    for (c, res), (ids, steady) in zip(got, kept):
        bboxes, _, kpts = (t.cpu().numpy() for t in res)
        exp_ids = track_ref.update(kpts, bboxes, None, scale)
        assert torch.equal(ids.cpu(), torch.from_numpy(exp_ids)), c
        exp_k, exp_b = smooth_ref.smooth(kpts, bboxes, exp_ids, None, scale)
        same_bits(steady[2], exp_k, f'frame {c} kpts')
        same_bits(steady[0], exp_b, f'frame {c} bboxes')
        want = IR.draw_nv12(befores[c].numpy(), 120, exp_k, exp_b, None, exp_ids, (1.0, 1.0), style, style.palette,
                            DIGIT_FONT)
        assert torch.equal(surfaces[c].cpu(), torch.from_numpy(want)), c
        tracked += int((exp_ids >= 1).sum())
    same_state(smoother, smooth_ref, [0], 'live')
    assert tracked > 0


def test_calls_allocate_no_growing_memory():
    """The allocator's peak does not grow over 100 calls, and the state stays where it is."""
    from pavenet_amd.smoothing import PoseSmoother
    rng = np.random.default_rng(182)
    smoother = PoseSmoother(15)
    pos = np.stack([40.0 + 150.0 * np.arange(6), np.full(6, 30.0)], 1)
    frames = [result(*poses(rng, FIGURE15, pos + f)) for f in range(10)]
    ids = torch.arange(1, 7, dtype=torch.int32).cuda()
    for f in range(3):
        smoother.smooth(frames[f], ids)
    ptrs = [t.data_ptr() for t in smoother._state.values()]

    def span(calls):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        for f in range(calls):
            smoother.smooth(frames[f % 10], ids)
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated()
    early, late = span(10), span(100)
    print(f'peak bytes allocated: 10 calls {early}, 100 calls {late}')
    assert late <= early
    smoother.reset()
    smoother.smooth(frames[0], ids)
    assert [t.data_ptr() for t in smoother._state.values()] == ptrs
