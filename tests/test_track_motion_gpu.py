"""The pose tracker's constant-velocity motion model on the device (csrc/pave_track.hip, MOTION = true) against the
rule of DESIGN section 14 "Motion" in numpy (tests/track_motion_ref.py): the ids and every tensor of the tracker's
state, vel and hits among them, are compared by torch.equal after every frame.  Needs an MI355X."""
import numpy as np
import pytest
import torch

from tests import track_motion_cases as TC
from tests import track_ref as TR
from tests.test_track_gpu import FIGURE15, _camera_frames, figure, poses, result
from tests.track_motion_ref import TrackMotionRef

pytestmark = pytest.mark.gpu
CV = 'constant_velocity'


@pytest.fixture(autouse=True)
def _split_gemm_mode():
    """As in test_track_gpu: the library's default GEMM mode, whatever mode an earlier module left behind."""
    from pavenet_amd import bricks
    old = bricks.get_gemm_mode()
    bricks.set_gemm_mode('bf16x3')
    yield
    bricks.set_gemm_mode(old)


SHARED = ['id', 'last', 'kpts', 'vis', 'area', 'frame', 'next_id', 'dropped']
STATE = SHARED + ['vel', 'hits']


def pair(K=15, **kw):
    from pavenet_amd.tracking import PoseTracker
    return PoseTracker(K, motion=CV, **kw), TrackMotionRef(K, **kw)


def same_state(tracker, ref, cameras, what, live_only=False):
    for c in cameras:
        got, exp = tracker.state(c), ref.state(c)
        assert list(got) == STATE == list(exp)
        live = exp['id'] != 0
        for name in STATE:
            g, e = got[name].cpu(), torch.from_numpy(np.asarray(exp[name]))
            assert g.dtype == torch.int32 and g.shape == e.shape, (what, c, name)
            if live_only and e.dim() >= 1 and name != 'id':
                g, e = g[live], e[live]
            assert torch.equal(g, e), f'{what}: camera {c} state {name}'


def step(tracker, ref, kpts, bboxes, what, keep=None, scale=None, camera=0, form='tuple', live_only=False):
    """One frame through the device and the reference; everything compared.  Returns the ids (numpy)."""
    exp = ref.update(kpts, bboxes, keep, (1.0, 1.0) if scale is None else scale, camera)
    got = tracker.update(result(kpts, bboxes, keep, form), scale_factor=scale, camera=camera)
    assert got.dtype == torch.int32 and got.is_cuda and tuple(got.shape) == (len(bboxes),)
    assert torch.equal(got.cpu(), torch.from_numpy(exp)), f'{what}: ids {got.cpu().tolist()} != {exp.tolist()}'
    same_state(tracker, ref, [camera], what, live_only)
    return exp


@pytest.mark.parametrize('form', ['tuple', 'dict'])
def test_random_scenario(form):
    """12 people for 60 frames at scale (0.694, 0.7), shuffled, walking up to 7 px per frame in every direction; one
    leaves for 2 frames and one for 7 and both are linked again where they are predicted to be; every frame carries
    poses that must not be tracked: keep = 0 (dict form), a score at the threshold, NaN and inf coordinates."""
    rng = np.random.default_rng(171)
    scale = (0.694, 0.7)
    tracker, ref = pair(15, max_age=10)
    start = np.stack([300.0 + 160.0 * np.arange(12), 250.0 + 11.0 * np.arange(12)], 1)
    speed = rng.uniform(-4, 4, (12, 2))
    speed[0], speed[3], speed[5], speed[7] = (-7.0, 0.5), (6.0, -3.0), (-5.0, -4.0), (0.0, 0.0)
    by_person = np.zeros((60, 12), np.int64)
    for f in range(60):
        there = [p for p in range(12) if not (p == 3 and 10 <= f < 12) and not (p == 5 and 20 <= f < 27)]
        kpts, bboxes = poses(rng, FIGURE15, (start + speed * f)[there], scale=scale)
        junk_k, junk_b = poses(rng, FIGURE15, rng.uniform(0, 1500, (5, 2)) + (0.0, 900.0), scale=scale)
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
        ids = step(tracker, ref, kpts[order], bboxes[order], f'{form} frame {f}', None if keep is None else keep[order],
                   scale, form=form)
        back = np.empty(len(order), np.int64)
        back[order] = ids
        by_person[f, there] = back[:len(there)]
        assert (back[len(there):] == 0).all()
    present = by_person != 0
    assert all(len(set(by_person[present[:, p], p].tolist())) == 1 for p in range(12))
    assert (by_person[10:12, 3] == 0).all() and (by_person[20:27, 5] == 0).all() and present.sum() == 60 * 12 - 9
    assert ref.next_id[0] == 13 and ref.frame[0] == 60
    assert (ref.vel[0][:12] < 0).any() and (ref.vel[0][:12] > 0).any()


def test_degenerate_model_equals_the_plain_tracker():
    """max_predict = 0, new_gate = 1 on the device against a motion=None tracker on the same frames: the ids and the
    eight shared state tensors are equal (and the plain state has no others)."""
    from pavenet_amd.tracking import PoseTracker
    rng = np.random.default_rng(172)
    kw = dict(max_age=3, max_tracks=10)
    motion, plain = PoseTracker(15, motion=CV, max_predict=0, new_gate=1, **kw), PoseTracker(15, **kw)
    start = np.stack([60.0 + 150.0 * np.arange(9), 40.0 + 11.0 * np.arange(9)], 1)
    speed = rng.uniform(-3, 3, (9, 2))
    for f in range(30):
        there = [p for p in range(9) if not (p == 2 and 8 <= f < 10) and not (p == 6 and 14 <= f < 20)]
        kpts, bboxes = poses(rng, FIGURE15, (start + speed * f)[there] + (0.0 if f != 22 else 400.0))
        keep = (rng.uniform(size=len(there)) > 0.15).astype(np.int32)
        order = rng.permutation(len(there))
        res = result(kpts[order], bboxes[order], keep[order], 'dict')
        a, b = motion.update(res), plain.update(res)
        assert torch.equal(a, b), f'frame {f}: {a.tolist()} != {b.tolist()}'
        got, exp = motion.state(0), plain.state(0)
        assert list(exp) == SHARED and list(got) == STATE
        for name in SHARED:
            assert torch.equal(got[name], exp[name]), f'frame {f}: state {name}'
    assert int(plain.state(0)['next_id']) > 10 and int(plain.state(0)['dropped']) > 0   # (births after frame 0, drops)
    assert int(motion.state(0)['hits'].max()) > 5


@pytest.mark.parametrize('name', list(TC.edge_scripts()))
def test_arithmetic_edges(name):
    """The hand-worked scripts of tests/track_motion_cases.py on the device and the oracle side by side; a state that
    no detection produces is written into the views of state(), which are the tracker's own tensors."""
    K, kw, steps = TC.edge_scripts()[name]
    tracker, ref = pair(K, **kw)
    count = [0]

    def update(kpts, bboxes):
        count[0] += 1
        return step(tracker, ref, kpts, bboxes, f'{name}: frame {count[0]}')

    def poke(slot, field, value):
        getattr(ref, field)[0, slot] = value
        tracker.state(0)[field][slot] = torch.tensor(value, dtype=torch.int32, device='cuda')
        same_state(tracker, ref, [0], f'{name}: poke')
    TC.run_script(K, steps, update, poke, lambda slot, field: tracker.state(0)[field][slot].cpu().numpy())


@pytest.mark.parametrize('K', [1, 32])
def test_custom_sigmas_and_empty_frames(K):
    """K = 1 and K = 32 with sigmas=; frames without poses and without a valid pose between matches, so the gap grows
    and the prediction runs over it; 5 px per frame with max_predict = 3."""
    rng = np.random.default_rng(176 + K)
    fig = figure(K)
    sigmas = rng.uniform(0.05, 0.1, K).tolist()
    tracker, ref = pair(K, sigmas=sigmas, max_age=6, max_tracks=7, max_predict=3, velocity_gain=5, new_gate=9)
    pos = np.stack([40.0 + 130.0 * np.arange(5), np.full(5, 30.0)], 1)
    seen = []
    for f in range(16):
        kpts, bboxes = poses(rng, fig, pos + (5.0 * f, 1.0 * f), jitter=0.005)
        if f in (3, 4, 9, 10, 11, 12):
            kpts, bboxes = kpts[:0], bboxes[:0]
        if f == 5:
            bboxes[:, 4] = 0.1
        order = rng.permutation(len(bboxes))
        ids = step(tracker, ref, kpts[order], bboxes[order], f'K = {K} frame {f}')
        back = np.empty(len(order), np.int64)
        back[order] = ids
        seen.append(back.tolist())
    assert sorted(seen[0]) == [1, 2, 3, 4, 5] and seen[5] == [0] * 5 and seen[3] == []
    assert ref.frame[0] == 16 and (ref.hits[0][ref.id[0] != 0] > 1).all()


def test_full_capacity_128_moving_tracks():
    """N = 128 on M = 128 slots, all moving, all matching: 128 greedy rounds and 128 velocities per frame."""
    rng = np.random.default_rng(178)
    tracker, ref = pair(15)
    pos = np.stack([200.0 + 60.0 * (np.arange(128) % 16), 200.0 + 120.0 * (np.arange(128) // 16)], 1)
    speed = rng.uniform(-6, 6, (128, 2))
    first = None
    for f in range(4):
        kpts, bboxes = poses(rng, FIGURE15, pos + speed * f)
        order = rng.permutation(128)
        ids = step(tracker, ref, kpts[order], bboxes[order], f'frame {f}')
        back = np.empty(128, np.int64)
        back[order] = ids
        first = back if first is None else first
        assert sorted(back) == list(range(1, 129)) and (back == first).all()
    assert ref.next_id[0] == 129 and ref.dropped[0] == 0 and (ref.hits[0] == 4).all()
    assert (np.abs(ref.vel[0]).max(1) > 0).sum() > 120


def test_drops_and_slot_reuse():
    """M = 4 with 7 births: three ids 0 and dropped == 3; expired slots are reused in ascending order, and what a freed
    slot holds in vel and hits does not matter: a birth writes both."""
    rng = np.random.default_rng(179)
    tracker, ref = pair(15, max_tracks=4, max_age=1)
    pos = np.stack([40.0 + 150.0 * np.arange(7), np.full(7, 30.0)], 1)
    kpts, bboxes = poses(rng, FIGURE15, pos)
    assert step(tracker, ref, kpts, bboxes, 'seven births').tolist() == [1, 2, 3, 4, 0, 0, 0]
    assert tracker.state(0)['dropped'].item() == 3
    for f in (2, 3):   # only the people of slots 1 and 3 stay; the three others are not there
        assert step(tracker, ref, kpts[[3, 1]], bboxes[[3, 1]], f'frame {f}').tolist() == [4, 2]
    assert tracker.state(0)['id'].cpu().tolist() == [0, 2, 0, 4]
    for t in (0, 2):   # garbage where the freed slots kept their fields, on the device only
        tracker.state(0)['vel'][t] = torch.tensor([-2000000000, 2000000000], dtype=torch.int32, device='cuda')
        tracker.state(0)['hits'][t] = -5
        tracker.state(0)['last'][t] = 2000000000
    assert step(tracker, ref, kpts[[6, 1, 5, 4]], bboxes[[6, 1, 5, 4]], 'reuse', live_only=True).tolist() == [5, 2, 6, 0]
    same_state(tracker, ref, [0], 'after the births')       # every slot is live again, with the oracle's fields
    assert tracker.state(0)['id'].cpu().tolist() == [5, 2, 6, 4]
    assert tracker.state(0)['hits'].cpu().tolist() == [1, 4, 1, 3]
    assert tracker.state(0)['vel'][[0, 2]].cpu().tolist() == [[0, 0], [0, 0]]
    assert tracker.state(0)['dropped'].item() == 4 and ref.next_id[0] == 7


def _many(frames, **kw):
    """update_many of all `frames` at once, single updates and the oracle: all equal."""
    from pavenet_amd.tracking import PoseTracker
    cameras = kw['cameras']
    many, single, ref = PoseTracker(15, motion=CV, **kw), PoseTracker(15, motion=CV, **kw), TrackMotionRef(15, **kw)
    got = many.update_many([(c, result(k, b)) for c, k, b in frames])
    assert len(got) == len(frames)
    for i, (c, k, b) in enumerate(frames):
        exp = ref.update(k, b, camera=c)
        one = single.update(result(k, b, form='dict'), camera=c)
        assert torch.equal(one.cpu(), torch.from_numpy(exp)) and torch.equal(got[i], one), f'entry {i}'
        same_state(single, ref, [c], f'single updates, entry {i}')
    same_state(many, ref, range(cameras), 'update_many')
    return many, ref


def test_update_many_equals_single_updates():
    """Three cameras, camera 1 with three frames in a row, 33 entries (two launches): update_many == one update at a
    time == the reference; reset(camera=1) leaves the other cameras' state, vel and hits included, as it is."""
    rng = np.random.default_rng(181)
    schedule = [0, 1, 1, 1, 2] + [int(c) for c in rng.integers(0, 3, 28)]
    assert len(schedule) == 33
    many, ref = _many(_camera_frames(rng, 3, schedule), cameras=3, max_tracks=9, max_age=2)
    assert int(ref.frame.sum()) == 33 and ref.frame.min() >= 3 and (ref.vel != 0).any()

    before = {c: {n: t.clone() for n, t in many.state(c).items()} for c in (0, 2)}
    ptrs = [t.data_ptr() for t in many._state.values()]
    for name in ('last', 'kpts', 'vis', 'area', 'vel', 'hits'):          # garbage where camera 1 kept its tracks
        many._state[name][1].fill_(-7)
    many.reset(camera=1)
    ref.reset(camera=1)
    for c in (0, 2):
        assert all(torch.equal(many.state(c)[n], before[c][n]) for n in STATE), f'camera {c} after reset(1)'
    assert [t.data_ptr() for t in many._state.values()] == ptrs
    more = _camera_frames(rng, 3, [1, 0, 1, 2, 1])
    got = many.update_many([(c, result(k, b)) for c, k, b in more], scale_factor=[1.0] * 5)
    for i, (c, k, b) in enumerate(more):
        assert torch.equal(got[i].cpu(), torch.from_numpy(ref.update(k, b, camera=c))), f'after reset: entry {i}'
    assert sorted(got[0].cpu().tolist()) == [1, 2, 3, 4] and ref.frame[1] == 3
    same_state(many, ref, [0, 2], 'after reset')
    same_state(many, ref, [1], 'after reset', live_only=True)


def test_consecutive_frames_of_one_camera_in_one_launch():
    """Seven frames of one camera in one launch, 6 px per frame: one block takes them in turn, and the velocity that
    frame f stores is what frame f + 1 predicts with (without it the people of frame 3 on would be new tracks: the
    same frames through the plain rule end above id 4)."""
    rng = np.random.default_rng(183)
    frames = []
    for f in range(7):
        kpts, bboxes = poses(rng, FIGURE15, np.stack([50.0 + 140.0 * np.arange(4), np.full(4, 40.0)], 1) + 6.0 * f,
                             height=40.0)
        order = rng.permutation(4)
        frames.append((0, kpts[order], bboxes[order]))
    many, ref = _many(frames, cameras=1)
    assert ref.next_id[0] == 5 and (ref.hits[0][:4] == 7).all() and (ref.vel[0][:4] > 300).all()
    plain = TR.TrackRef(15)
    for _, k, b in frames:
        plain.update(k, b)
    assert plain.next_id[0] > 5


def test_updates_allocate_no_growing_memory():
    from pavenet_amd.tracking import PoseTracker
    rng = np.random.default_rng(182)
    tracker = PoseTracker(15, motion=CV)
    pos = np.stack([40.0 + 150.0 * np.arange(6), np.full(6, 30.0)], 1)
    frames = [result(*poses(rng, FIGURE15, pos + f)) for f in range(12)]
    for f in range(3):
        tracker.update(frames[f])
    assert list(tracker._state) == STATE
    ptrs = [t.data_ptr() for t in tracker._state.values()] + [tracker._scratch.data_ptr()]

    def span(lo, hi):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        for f in range(lo, hi):
            tracker.update(frames[f])
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated()
    early, late = span(3, 6), span(6, 12)
    print(f'peak bytes allocated: updates 3..6 {early}, updates 6..12 {late}')
    assert late <= early
    tracker.reset()
    tracker.update(frames[0])
    assert [t.data_ptr() for t in tracker._state.values()] + [tracker._scratch.data_ptr()] == ptrs
