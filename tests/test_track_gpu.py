"""Track ids on the device (csrc/pave_track.hip) against the rule of DESIGN section 14 in numpy (tests/track_ref.py):
the ids and every tensor of the tracker's state are compared by torch.equal after every frame.  Needs an MI355X."""
import math

import numpy as np
import pytest
import torch

from tests import track_ref as TR

pytestmark = pytest.mark.gpu

@pytest.fixture(autouse=True)
def _split_gemm_mode():
    """The end-to-end test's model runs under set_batch_invariant, which needs the library's default GEMM mode,
    whatever mode an earlier module left behind."""
    from pavenet_amd import bricks
    old = bricks.get_gemm_mode()
    bricks.set_gemm_mode('bf16x3')
    yield
    bricks.set_gemm_mode(old)


STATE = ['id', 'last', 'kpts', 'vis', 'area', 'frame', 'next_id', 'dropped']
FIGURE15 = np.asarray([(.20, .08), (.20, .14), (.20, .00), (.05, .20), (.35, .20), (.00, .36), (.40, .36), (.02, .50),
                       (.38, .50), (.10, .52), (.30, .52), (.09, .76), (.31, .76), (.08, 1.0), (.32, 1.0)], np.float64)


def figure(K, seed=1):
    if K == 15:
        return FIGURE15
    return np.random.default_rng(seed).uniform(0, 1, (K, 2)) * (0.4, 1.0)


def poses(rng, fig, pos, height=100.0, scale=(1.0, 1.0), jitter=0.01, kpt_scores=None):
    """People with their top-left corners at pos [P, 2] (picture pixels) -> kpts [P, K, 3], bboxes [P, 5] float32 in
    the coordinates of the scaled picture; the box is the figure's 0.4 height x height frame."""
    pos = np.asarray(pos, np.float64).reshape(-1, 2)
    P, K = len(pos), len(fig)
    xy = fig[None] * height + pos[:, None, :] + rng.uniform(-jitter, jitter, (P, K, 2)) * height
    kpts = np.empty((P, K, 3), np.float32)
    kpts[..., :2] = xy * np.asarray(scale)
    kpts[..., 2] = 0.9 if kpt_scores is None else kpt_scores
    bboxes = np.empty((P, 5), np.float32)
    bboxes[:, :2] = pos * np.asarray(scale)
    bboxes[:, 2:4] = (pos + (0.4 * height, height)) * np.asarray(scale)
    bboxes[:, 4] = 0.8
    return kpts, bboxes


def result(kpts, bboxes, keep=None, form='tuple'):
    kp, bb = torch.from_numpy(np.ascontiguousarray(kpts)).cuda(), torch.from_numpy(np.ascontiguousarray(bboxes)).cuda()
    if form == 'tuple':
        assert keep is None
        return (bb, torch.zeros(len(bb), dtype=torch.int64, device='cuda'), kp)
    keep = torch.ones(1, len(bb), dtype=torch.int32).cuda() if keep is None else \
        torch.from_numpy(np.asarray(keep, np.int32))[None].cuda()
    return dict(bboxes=bb[None], kpts=kp[None], keep=keep)


def pair(K=15, **kw):
    from pavenet_amd.tracking import PoseTracker
    return PoseTracker(K, **kw), TR.TrackRef(K, **kw)


def same_state(tracker, ref, cameras, what, live_only=False):
    for c in cameras:
        got, exp = tracker.state(c), ref.state(c)
        assert list(got) == STATE
        live = exp['id'] != 0
        for name in STATE:
            g, e = got[name].cpu(), torch.from_numpy(np.asarray(exp[name]))
            assert g.dtype == torch.int32 and g.shape == e.shape, (what, c, name)
            if live_only and e.dim() >= 1 and name != 'id':
                g, e = g[live], e[live]
            assert torch.equal(g, e), f'{what}: camera {c} state {name}'


def step(tracker, ref, kpts, bboxes, what, keep=None, scale=None, camera=0, form='tuple'):
    """One frame through the device and the reference; everything compared.  Returns the ids (numpy)."""
    exp = ref.update(kpts, bboxes, keep, (1.0, 1.0) if scale is None else scale, camera)
    got = tracker.update(result(kpts, bboxes, keep, form), scale_factor=scale, camera=camera)
    assert got.dtype == torch.int32 and got.is_cuda and tuple(got.shape) == (len(bboxes),)
    assert torch.equal(got.cpu(), torch.from_numpy(exp)), f'{what}: ids {got.cpu().tolist()} != {exp.tolist()}'
    same_state(tracker, ref, [camera], what)
    return exp


@pytest.mark.parametrize('form', ['tuple', 'dict'])
def test_random_scenario(form):
    """12 people for 60 frames at scale (0.694, 0.7), shuffled; one leaves for 2 frames and is linked again, one
    for 5 frames and comes back under a new id (max_age = 3); every frame carries poses that must not be tracked:
    keep = 0 (dict form), a score at the threshold, NaN and inf coordinates, a NaN score."""
    rng = np.random.default_rng(71)
    scale = (0.694, 0.7)
    tracker, ref = pair(15, max_age=3)
    start = np.stack([60.0 + 150.0 * np.arange(12), 40.0 + 11.0 * np.arange(12)], 1)
    speed = rng.uniform(-3, 3, (12, 2))
    speed[3], speed[5] = (2.0, -1.0), (1.0, 1.0)
    by_person = np.zeros((60, 12), np.int64)
    for f in range(60):
        there = [p for p in range(12) if not (p == 3 and 10 <= f < 12) and not (p == 5 and 20 <= f < 25)]
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
        ids = step(tracker, ref, kpts[order], bboxes[order], f'{form} frame {f}', None if keep is None else keep[order],
                   scale, form=form)
        back = np.empty(len(order), np.int64)
        back[order] = ids
        by_person[f, there] = back[:len(there)]
        assert (back[len(there):] == 0).all()
    assert (by_person[:, [0, 1, 2, 4] + list(range(6, 12))] == by_person[0, [0, 1, 2, 4] + list(range(6, 12))]).all()
    assert by_person[9, 3] == by_person[12, 3] != 0 and (by_person[10:12, 3] == 0).all()
    assert by_person[19, 5] != 0 and by_person[25, 5] == 13 and (by_person[25:, 5] == 13).all()
    assert ref.next_id[0] == 14 and ref.frame[0] == 60


def test_max_age_boundary():
    """frame - last == max_age links, == max_age + 1 expires."""
    rng = np.random.default_rng(72)
    kpts, bboxes = poses(rng, FIGURE15, [(50, 50)])
    none = poses(rng, FIGURE15, np.zeros((0, 2)))
    for max_age, again in ((3, 1), (2, 2)):
        tracker, ref = pair(15, max_age=max_age)
        assert step(tracker, ref, kpts, bboxes, 'birth').tolist() == [1]
        for f in (2, 3):
            step(tracker, ref, *none, f'empty frame {f}')
        assert step(tracker, ref, kpts, bboxes, f'max_age {max_age}').tolist() == [again]
        assert int(tracker.state(0)['id'][0].cpu()) == again and int(tracker.state(0)['last'][0].cpu()) == 4


def test_min_kpts_boundary():
    """min_kpts - 1 agreeing key points make a new track, min_kpts keep the old one."""
    rng = np.random.default_rng(73)
    kpts, bboxes = poses(rng, FIGURE15, [(50, 50)], jitter=0.0)
    for agreeing, again in ((5, 1), (4, 2)):
        tracker, ref = pair(15)
        assert tracker.min_kpts == 5
        step(tracker, ref, kpts, bboxes, 'birth')
        moved = kpts.copy()
        moved[0, agreeing:, 0] += 200.0
        assert step(tracker, ref, moved, bboxes, f'{agreeing} agreeing').tolist() == [again]


def test_agreement_boundary_is_inclusive():
    """(d2 << 20) <= C (area_d + area_t) at equality: C = 2^20, areas 9 + 8, d2 = 17 agrees and d2 = 18 does not."""
    sig = dict(sigmas=[0.5], match_thr=math.exp(-1.0), min_kpts=1)
    birth_k = np.asarray([[[10.0, 10.0, 0.9]]], np.float32)
    birth_b = np.asarray([[10.0, 10.0, 10.75, 10.75, 0.8]], np.float32)       # 3 x 3 quarter pixels
    box = np.asarray([[10.0, 10.0, 10.5, 11.0, 0.8]], np.float32)             # 2 x 4
    for (dx, dy), again in (((1.0, 0.25), 1), ((0.75, 0.75), 2)):
        tracker, ref = pair(1, **sig)
        assert tracker.C == [1 << 20] == ref.C.tolist()
        step(tracker, ref, birth_k, birth_b, 'birth')
        assert tracker.state(0)['area'][0].item() == 9
        kp = birth_k + np.asarray([dx, dy, 0], np.float32)
        assert step(tracker, ref, kp, box, f'd = {(dx, dy)}').tolist() == [again]


def test_ties_resolve_by_slot_then_detection():
    rng = np.random.default_rng(74)
    one_k, one_b = poses(rng, FIGURE15, [(80, 60)], jitter=0.0)
    tracker, ref = pair(15)
    two = np.repeat(one_k, 2, 0), np.repeat(one_b, 2, 0)
    assert step(tracker, ref, *two, 'two equal births').tolist() == [1, 2]
    # one pose, two equal tracks: the smaller slot
    assert step(tracker, ref, one_k, one_b, 'two equal tracks').tolist() == [1]
    # three equal poses: every row's best is slot 0; detection 0 takes it, 1 takes slot 1, 2 is born
    three = np.repeat(one_k, 3, 0), np.repeat(one_b, 3, 0)
    assert step(tracker, ref, *three, 'three equal poses').tolist() == [1, 2, 3]
    # equal s: the smaller D goes first, wherever the pose stands in the list
    near = one_k.copy()
    near[0, :, 0] += 0.25
    k4, b4 = np.concatenate([near, one_k, near, one_k]), np.repeat(one_b, 4, 0)
    # (both exact poses first, by slot; then a moved one takes slot 2 and the other is born)
    assert step(tracker, ref, k4, b4, 'mixed').tolist() == [3, 1, 4, 2]


def test_quantisation_ties_round_to_even():
    """x / sx * 4 at .5: rint, in fp32, after a correctly rounded division."""
    tracker, ref = pair(2, sigmas=[0.05, 0.05], min_kpts=1)
    kp = np.asarray([[[10.125, 10.375, 0.9], [10.625, 10.875, 0.9]]], np.float32)
    bb = np.asarray([[10.125, 10.375, 20.625, 20.875, 0.8]], np.float32)
    step(tracker, ref, kp, bb, 'scale 1')
    assert tracker.state(0)['kpts'][0].cpu().tolist() == [[40, 42], [42, 44]]
    assert tracker.state(0)['area'][0].item() == (82 - 40) * (84 - 42)
    tracker, ref = pair(2, sigmas=[0.05, 0.05], min_kpts=1)
    step(tracker, ref, kp, bb, 'scale 1 / 4, 1 / 2', scale=(0.25, 0.5))
    assert tracker.state(0)['kpts'][0].cpu().tolist() == [[162, 83], [170, 87]]
    # a scale that is no power of two: the quotient is rounded once, then scaled
    tracker, ref = pair(2, sigmas=[0.05, 0.05], min_kpts=1)
    rng = np.random.default_rng(75)
    kp = np.concatenate([rng.uniform(0, 900, (64, 2, 2)), np.full((64, 2, 1), 0.9)], -1).astype(np.float32)
    bb = np.concatenate([kp[:, 0, :2], kp[:, 1, :2], np.full((64, 1), 0.8)], -1).astype(np.float32)
    step(tracker, ref, kp, bb, 'scale 0.694, 0.7', scale=(0.694, 0.7))


@pytest.mark.parametrize('K', [1, 32])
def test_custom_sigmas_and_empty_frames(K):
    """K = 1 and K = 32 with sigmas=; the first frame, a frame without poses and a frame without a valid pose."""
    rng = np.random.default_rng(76 + K)
    fig = figure(K)
    sigmas = rng.uniform(0.05, 0.1, K).tolist()
    tracker, ref = pair(K, sigmas=sigmas, max_age=3, max_tracks=7)
    pos = np.stack([40.0 + 130.0 * np.arange(5), np.full(5, 30.0)], 1)
    seen = []
    for f in range(8):
        kpts, bboxes = poses(rng, fig, pos + (1.0 * f, 0.0), jitter=0.005)
        if f == 3:
            kpts, bboxes = kpts[:0], bboxes[:0]
        if f == 4:
            bboxes[:, 4] = 0.1
        order = rng.permutation(len(bboxes))
        ids = step(tracker, ref, kpts[order], bboxes[order], f'K = {K} frame {f}')
        back = np.empty(len(order), np.int64)
        back[order] = ids
        seen.append(back.tolist())
    assert sorted(seen[0]) == [1, 2, 3, 4, 5] and seen[1] == seen[2] == seen[5] == seen[7] == seen[0]
    assert seen[3] == [] and seen[4] == [0] * 5 and ref.frame[0] == 8


def test_full_capacity_128_rounds():
    """N = 128 on M = 128 slots, all matching: 128 greedy rounds."""
    rng = np.random.default_rng(78)
    tracker, ref = pair(15)
    pos = np.stack([30.0 + 60.0 * (np.arange(128) % 16), 20.0 + 120.0 * (np.arange(128) // 16)], 1)
    first = None
    for f in range(3):
        kpts, bboxes = poses(rng, FIGURE15, pos + 1.5 * f)
        order = rng.permutation(128)
        ids = step(tracker, ref, kpts[order], bboxes[order], f'frame {f}')
        back = np.empty(128, np.int64)
        back[order] = ids
        first = back if first is None else first
        assert sorted(back) == list(range(1, 129)) and (back == first).all()
    assert ref.next_id[0] == 129 and ref.dropped[0] == 0


def test_drops_and_slot_reuse():
    """M = 4 with 7 births: three ids 0 and dropped == 3; expired slots are reused in ascending order."""
    rng = np.random.default_rng(79)
    tracker, ref = pair(15, max_tracks=4, max_age=1)
    pos = np.stack([40.0 + 150.0 * np.arange(7), np.full(7, 30.0)], 1)
    kpts, bboxes = poses(rng, FIGURE15, pos)
    assert step(tracker, ref, kpts, bboxes, 'seven births').tolist() == [1, 2, 3, 4, 0, 0, 0]
    assert tracker.state(0)['dropped'].item() == 3
    for f in (2, 3):   # only the people of slots 1 and 3 stay; the three others are not there
        assert step(tracker, ref, kpts[[3, 1]], bboxes[[3, 1]], f'frame {f}').tolist() == [4, 2]
    assert tracker.state(0)['id'].cpu().tolist() == [0, 2, 0, 4]
    assert step(tracker, ref, kpts[[6, 1, 5, 4]], bboxes[[6, 1, 5, 4]], 'reuse').tolist() == [5, 2, 6, 0]
    # (slot 3 was matched in frame 3 and is not yet expired in frame 4: the last pose finds no free slot)
    assert tracker.state(0)['id'].cpu().tolist() == [5, 2, 6, 4]
    assert tracker.state(0)['dropped'].item() == 4 and ref.next_id[0] == 7


def test_invisible_key_points():
    """kpt_thr = 0.5 with mixed scores: only co-visible key points count, in s and in D."""
    rng = np.random.default_rng(80)
    tracker, ref = pair(15, kpt_thr=0.5, min_kpts=3)
    pos = np.stack([40.0 + 60.0 * np.arange(9), 30.0 + 5.0 * np.arange(9)], 1)   # overlapping people
    masks = set()
    for f in range(10):
        scores = rng.uniform(0.0, 1.0, (9, 15)).astype(np.float32)
        scores[0] = 0.5                                                           # not > kpt_thr: nothing visible
        scores[1, 3] = np.nan
        kpts, bboxes = poses(rng, FIGURE15, pos + rng.uniform(-4, 4, (9, 2)), kpt_scores=scores, jitter=0.02)
        order = rng.permutation(9)
        step(tracker, ref, kpts[order], bboxes[order], f'frame {f}')
        masks |= set(ref.vis[0][ref.id[0] != 0].tolist())
    assert 0 in masks and len(masks) > 20


def _camera_frames(rng, n_cams, schedule):
    """schedule: the camera of every entry -> [(camera, kpts, bboxes)], every camera with its own walking people."""
    clock = [0] * n_cams
    out = []
    for c in schedule:
        P = 3 + c
        pos = np.stack([50.0 + 140.0 * np.arange(P), np.full(P, 40.0 + 9.0 * c)], 1) + (2.0 + c) * clock[c]
        kpts, bboxes = poses(rng, FIGURE15, pos)
        order = rng.permutation(P)
        out.append((c, kpts[order], bboxes[order]))
        clock[c] += 1
    return out


def test_update_many_equals_single_updates():
    """Three cameras, camera 1 with three frames in a row, 33 entries (two launches): update_many == one update at
    a time == the reference; reset(camera=1) leaves cameras 0 and 2 as they are; rows of garbage in freed slots do
    not matter."""
    from pavenet_amd.tracking import PoseTracker
    rng = np.random.default_rng(81)
    schedule = [0, 1, 1, 1, 2] + [int(c) for c in rng.integers(0, 3, 28)]
    assert len(schedule) == 33
    frames = _camera_frames(rng, 3, schedule)
    kw = dict(cameras=3, max_tracks=9, max_age=2)
    many, single, ref = PoseTracker(15, **kw), PoseTracker(15, **kw), TR.TrackRef(15, **kw)
    got = many.update_many([(c, result(k, b)) for c, k, b in frames])
    assert len(got) == 33
    for i, (c, k, b) in enumerate(frames):
        exp = ref.update(k, b, camera=c)
        one = single.update(result(k, b, form='dict'), camera=c)
        assert torch.equal(one.cpu(), torch.from_numpy(exp)) and torch.equal(got[i], one), f'entry {i}'
    same_state(many, ref, range(3), 'update_many')
    same_state(single, ref, range(3), 'single updates')
    assert int(ref.frame.sum()) == 33 and ref.frame.min() >= 3

    before = {c: {n: t.clone() for n, t in many.state(c).items()} for c in (0, 2)}
    ptrs = [t.data_ptr() for t in many._state.values()]
    for name in ('last', 'kpts', 'vis', 'area'):          # garbage where camera 1 kept its tracks
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
    many.reset()
    assert all(int(many.state(c)[n].sum()) == (1 if n == 'next_id' else 0) for c in range(3)
               for n in ('id', 'frame', 'next_id', 'dropped'))


def test_live_video_end_to_end():
    """Five frames through LiveVideoPose (the small model of test_live_gpu), linked frame by frame."""
    from pavenet_amd.formats import posetrack_frame
    from pavenet_amd.live import LiveVideoPose
    from pavenet_amd.tracking import PoseTracker
    from tests.test_live_gpu import _meta, _model, _rand
    m, meta = _model(3), _meta()
    video = _rand(5, 3, 128, 160, seed=91)
    live = LiveVideoPose(m, meta, max_push=1, decode_chunk=4)
    kw = dict(score_thr=0.0, max_tracks=16)
    tracker, ref = PoseTracker(15, **kw), TR.TrackRef(15, **kw)
    results = []
    for f in range(5):
        results += live.push(video[f])
    results += live.flush()
    assert [i for i, _ in results] == [0, 1, 2, 3, 4]
    annolist = []
    for i, res in results:
        ids = tracker.update(res)
        exp = ref.update(res[2].cpu().numpy(), res[0].cpu().numpy())
        assert torch.equal(ids.cpu(), torch.from_numpy(exp)), f'frame {i}'
        same_state(tracker, ref, [0], f'frame {i}')
        frame = posetrack_frame(f'images/clip/{i:08d}.jpg', i + 1, res, ids)
        assert [r['track_id'][0] for r in frame['annorect']] == [int(v) for v in exp if v != 0]
        annolist.append(frame)
    assert len(results[0][1][0]) > 0 and len(annolist[0]['annorect']) > 0
    assert ref.frame[0] == 5


def test_updates_allocate_no_growing_memory():
    from pavenet_amd.tracking import PoseTracker
    rng = np.random.default_rng(82)
    tracker = PoseTracker(15)
    pos = np.stack([40.0 + 150.0 * np.arange(6), np.full(6, 30.0)], 1)
    frames = [result(*poses(rng, FIGURE15, pos + f)) for f in range(12)]
    for f in range(3):
        tracker.update(frames[f])
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
