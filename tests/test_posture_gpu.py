"""Postures and falls on the device (csrc/pave_posture.hip) against the rule of DESIGN section 20 in numpy
(tests/posture_ref.py): after every frame the six outputs and every state and counter tensor of the monitor are
compared with the oracle by torch.equal.  Needs an MI355X."""
import numpy as np
import pytest
import torch

from tests import posture_cases as PC
from tests import posture_ref as PR
from tests.test_posture_cpu import hands_up, standing, turned
from tests.test_track_gpu import result

pytestmark = pytest.mark.gpu

OUTPUTS = ['posture', 'raw', 'hands', 'since', 'events', 'n_events']
STATE = list(PR.STATE)
COUNTS = list(PR.COUNTERS)
ONE = dict(parts=dict(shoulders=(0,), hips=(0,), ankles=(0,), wrists=(0,)))


class Pair:
    """A PostureMonitor and the oracle, configured alike."""

    def __init__(self, K=15, **kw):
        from pavenet_amd.posture import PostureMonitor
        self.mon, self.ref = PostureMonitor(K, **kw), PR.PostureRef(K, **kw)


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
        PC.invariant(p.ref.state(c), p.ref.counts(c))


def step(p, kpts, bboxes, ids, what, keep=None, scale=None, camera=0, form='tuple', live_only=False):
    """One frame through the device and the reference; everything compared; the inputs are what they were.  Returns
    the oracle's outputs."""
    ids = np.asarray(ids, np.int64).astype(np.int32)
    exp = p.ref.update(kpts, bboxes, ids, keep, (1.0, 1.0) if scale is None else scale, camera)
    res, dev_ids = result(kpts, bboxes, keep, form), torch.from_numpy(ids).cuda()
    tensors = [t for t in (res.values() if isinstance(res, dict) else res)] + [dev_ids]
    before = [t.clone() for t in tensors]
    got = p.mon.update(res, dev_ids, scale_factor=scale, camera=camera)
    same_outputs(got, exp, what)
    same_all(p, [camera], what, live_only)
    assert all(a.numel() == 0 or torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8))
               for a, b in zip(tensors, before)), f'{what}: an input changed'          # (bytes: a NaN equals itself)
    return exp


@pytest.mark.parametrize('script', PC.SCRIPTS, ids=lambda s: s.__name__)
def test_hand_worked_scripts_on_the_device(script):
    class Harness:
        def __init__(self, K, **kw):
            self.p = Pair(K, **kw)
            self.p.mon._allocate(torch.device('cuda', torch.cuda.current_device()))
            self.frames = 0

        def frame(self, kpts, bboxes, ids, keep=None, camera=0):
            self.frames += 1
            form = 'tuple' if keep is None else 'dict'
            return step(self.p, kpts, bboxes, ids, f'{script.__name__} frame {self.frames}',
                        None if keep is None else np.asarray(keep, np.int32), camera=camera, form=form, live_only=True)

        def poke(self, field, index, value, camera=0):
            at = (camera,) + tuple(index)
            getattr(self.p.ref, field)[at] = value
            self.p.mon._state[field][at] = torch.from_numpy(np.asarray(getattr(self.p.ref, field)[at])).cuda()

        def get(self, field, camera=0):
            views = dict(self.p.mon.state(camera), **self.p.mon.counts(camera))
            return views[field].cpu().numpy()
    script(Harness)


FALL_T = (4, 6, 8, 10, 3, 5)


def falling_people(form, scale, frames=40, height=100.0):
    """Six people 100 px tall, 350 px apart, 1 % jitter, shuffled on every frame: persons 0 and 1 hold their hands up
    in frames 3 .. 9; person p falls from frame 10 + p on over FALL_T[p] frames, to the right or to the left, and
    stays down; person 5 is away in frames 20 .. 22.  Every frame carries poses that take no part: keep = 0 (dict
    form), a score at the threshold, NaN and inf coordinates, a NaN score, an id of 0.  Yields (kpts, bboxes, keep,
    ids)."""
    rng = np.random.default_rng(211)

    def paint(fig, p):
        xy = fig * height + (300.0 + 350.0 * p, 200.0 + 9.0 * p)
        k = np.empty((15, 3), np.float32)
        k[:, :2] = (xy + rng.uniform(-0.01, 0.01, xy.shape) * height) * np.asarray(scale)
        k[:, 2] = 0.9
        return k, np.asarray([k[:, 0].min(), k[:, 1].min(), k[:, 0].max(), k[:, 1].max(), 0.8], np.float32)
    for f in range(frames):
        there = [p for p in range(6) if not (p == 5 and 20 <= f < 23)]
        rows = []
        for p in there:
            turn = min(max(f - (10 + p), 0), FALL_T[p]) / FALL_T[p] * (90.0 if p % 2 == 0 else -90.0)
            fig = hands_up() if p < 2 and 3 <= f < 10 else standing()
            rows.append(paint(turned(fig, turn), p))
        junk = [paint(standing(), 6 + j) for j in range(6)]
        junk[1][1][4] = 0.3                      # not > score_thr
        junk[2][0][rng.integers(15), 0] = np.nan
        junk[3][1][2] = np.inf
        junk[4][1][4] = np.nan
        ids = [100 + p for p in there] + [200, 201, 202, 203, 204, 0]          # (junk 5: a good pose without a track)
        keep = np.ones(len(rows) + 6, np.int32)
        keep[len(rows)] = 0                      # junk 0: a good pose NMS removed
        if form == 'tuple':                      # (no keep there: the pose is left out)
            junk, ids, keep = junk[1:], ids[:len(rows)] + ids[len(rows) + 1:], None
        kpts = np.stack([k for k, _ in rows + junk])
        bboxes = np.stack([b for _, b in rows + junk])
        order = rng.permutation(len(bboxes))
        yield kpts[order], bboxes[order], None if keep is None else keep[order], np.asarray(ids, np.int32)[order]


@pytest.mark.parametrize('form,scale', [('tuple', (1.0, 1.0)), ('dict', (0.694, 0.7))])
def test_six_people_fall(form, scale):
    """`falling_people` in both result forms, the second at a non-unit scale factor: every kind of event occurs, so an
    idle kernel cannot pass; six falls, six people down."""
    p = Pair(15, max_age=5, max_tracks=8, min_frames=2, down_frames=5)
    kinds = np.zeros(6, np.int64)
    for f, (kpts, bboxes, keep, ids) in enumerate(falling_people(form, scale)):
        out = step(p, kpts, bboxes, ids, f'{form} frame {f}', keep, None if form == 'tuple' else scale, form=form)
        kinds += np.bincount(out['events'][:int(out['n_events']), 0], minlength=6)
    assert p.ref.frame[0] == 40 and p.ref.dropped[0] == 0
    print('events by kind (POSTURE, FALL, DOWN, HANDS_UP, HANDS_DOWN):', kinds[1:].tolist())
    assert kinds[0] == 0 and (kinds[1:] >= 1).all(), kinds.tolist()
    assert int(p.ref.falls[0]) == 6 and int(p.ref.downs[0]) >= 6 and p.ref.now[0].tolist() == [0, 0, 0, 0, 6]


def people(rng, n, f=0, K=15, height=60.0):
    """n standing, crouching or lying K = 15 figures on a grid, the class changing with the frame."""
    kpts, bboxes = np.empty((n, 15, 3), np.float32), np.empty((n, 5), np.float32)
    for d in range(n):
        fig = (standing(), turned(standing(), 90), hands_up(), turned(standing(), 45))[(d + (f // 2) * (d % 3)) % 4]
        xy = fig * height + (150.0 + 110.0 * (d % 16), 100.0 + 130.0 * (d // 16))
        kpts[d, :, :2] = xy + rng.uniform(-0.01, 0.01, xy.shape) * height
        kpts[d, :, 2] = 0.9
        bboxes[d] = (kpts[d, :, 0].min(), kpts[d, :, 1].min(), kpts[d, :, 0].max(), kpts[d, :, 1].max(), 0.8)
    return kpts, bboxes


def test_no_pose_one_pose_and_full_capacity():
    """N = 0 (the outputs are empty tensors and the plan carries null pointers for them; the clock still runs), N = 1,
    and N = 128 on 128 slots for eight frames in which most tracks change their class; then a 129th id is dropped and
    129 poses are refused."""
    rng = np.random.default_rng(212)
    p = Pair(15, min_frames=1, down_frames=2)
    out = step(p, *PC.none(15)[:2], [], 'no pose')
    assert out['posture'].shape == (0,) and int(out['n_events']) == 0 and p.ref.frame[0] == 1
    step(p, *people(rng, 1), [77], 'one pose')
    events = 0
    for f in range(8):
        kpts, bboxes = people(rng, 128, f)
        order = rng.permutation(128)
        events += int(step(p, kpts[order], bboxes[order], (np.arange(128) + 1000)[order], f'128 poses, frame {f}')['n_events'])
    assert (p.ref.id[0] != 0).all() and p.ref.id[0, 0] == 77 and p.ref.dropped[0] == 8 and events > 128     # (77 holds a slot)
    step(p, *PC.none(15)[:2], [], 'no pose again')
    kpts, bboxes = people(rng, 129)
    with pytest.raises(ValueError, match='at most 128'):
        p.mon.update(result(kpts, bboxes), torch.arange(1, 130, dtype=torch.int32).cuda())


def test_more_events_than_rows_at_full_capacity():
    """128 people with their hands up fall in one frame: 384 events against max_events = 256."""
    rng = np.random.default_rng(213)
    p = Pair(15, min_frames=1)
    up, down = people(rng, 128), people(rng, 128)
    for d in range(128):
        xy0 = (150.0 + 110.0 * (d % 16), 100.0 + 130.0 * (d // 16))
        up[0][d, :, :2] = hands_up() * 60.0 + xy0
        down[0][d, :, :2] = turned(standing(), -90) * 60.0 + xy0
    ids = np.arange(1, 129)
    step(p, *up, ids, 'up')
    out = step(p, *down, ids, 'down')
    assert int(out['n_events']) == 384 and out['events'][:, 3].tolist() == [d for d in range(85) for _ in range(3)] + [85]
    assert p.ref.falls[0] == 128 and p.ref.now[0, 4] == 128 and p.ref.hands_up[0] == 0


def test_one_key_point_and_one_slot():
    """K = 1 with `parts` naming key point 0 for all four parts: every pose is UNKNOWN (dx = dy = 0), which is a class
    like another for the slots and the counters.  max_tracks = 1: whoever comes second is dropped."""
    p = Pair(1, max_tracks=1, max_age=1, min_frames=1, **ONE)
    kp = np.asarray([[[10.0, 20.0, 0.9]], [[30.0, 40.0, 0.9]]], np.float32)
    bb = np.asarray([[0, 0, 20, 40, 0.8], [20, 20, 40, 60, 0.8]], np.float32)
    out = step(p, kp, bb, [5, 6], 'frame 0')
    assert out['posture'].tolist() == [0, -1] and p.ref.dropped[0] == 1 and p.ref.now[0].tolist() == [1, 0, 0, 0, 0]
    step(p, kp[1:], bb[1:], [6], 'frame 1')
    out = step(p, kp[1:], bb[1:], [6], 'frame 2')
    assert out['posture'].tolist() == [0] and p.ref.id[0].tolist() == [6] and p.ref.dropped[0] == 2


def _items(frames, form='tuple'):
    return [(c, result(k, b, form=form), torch.from_numpy(np.asarray(i, np.int32)).cuda()) for c, k, b, i in frames]


def test_update_many_33_entries_two_cameras():
    """Two cameras interleaved (camera 1 also with frames in a row), 33 entries, so two launches whose state carries
    over: update_many == two single-camera monitors called frame by frame == the reference.  reset(camera=1) leaves
    camera 0 as it is."""
    rng = np.random.default_rng(214)
    schedule = [0, 1, 1, 1, 0] + [int(c) for c in rng.integers(0, 2, 28)]
    assert len(schedule) == 33
    clock, frames = [0, 0], []
    for c in schedule:
        n = 5 + 2 * c
        kpts, bboxes = people(rng, n, clock[c])
        ids = np.arange(1, n + 1, dtype=np.int32) + 10 * c
        if clock[c] % 4 == 2:
            ids[0] = 0
        if clock[c] % 5 == 3:
            ids[1] = ids[2]
        order = rng.permutation(n)
        frames.append((c, kpts[order], bboxes[order], ids[order]))
        clock[c] += 1
    kw = dict(max_tracks=9, max_age=2, min_frames=1, down_frames=3)
    many = Pair(15, cameras=2, **kw)
    singles = [Pair(15, **kw), Pair(15, **kw)]
    got = many.mon.update_many(_items(frames))
    assert len(got) == 33
    total = 0
    for i, (c, k, b, ids) in enumerate(frames):
        exp = many.ref.update(k, b, ids, camera=c)
        singles[c].ref.update(k, b, ids)
        one = singles[c].mon.update(result(k, b, form='dict'), torch.from_numpy(ids).cuda())
        same_outputs(one, exp, f'single entry {i}')
        same_outputs(got[i], exp, f'many entry {i}')
        total += int(exp['n_events'])
    same_all(many, range(2), 'update_many')
    for c in range(2):
        same_all(singles[c], [0], f'single monitor {c}')
        for name in STATE:
            assert torch.equal(many.mon.state(c)[name], singles[c].mon.state(0)[name]), (c, name)
    assert int(many.ref.frame.sum()) == 33 and many.ref.frame.min() >= 3 and total > 30
    before = [t.clone() for views in (many.mon.state(0), many.mon.counts(0)) for t in views.values()]
    ptrs = [t.data_ptr() for t in many.mon._state.values()]
    many.mon.reset(camera=1)
    many.ref.reset(camera=1)
    after = [t for views in (many.mon.state(0), many.mon.counts(0)) for t in views.values()]
    assert all(torch.equal(a, b) for a, b in zip(after, before)) and [t.data_ptr() for t in many.mon._state.values()] == ptrs
    more = [(1, *people(rng, 4, 0), np.arange(1, 5, dtype=np.int32)), (0, *people(rng, 5, clock[0]), np.arange(1, 6, dtype=np.int32))]
    got = many.mon.update_many(_items(more), scale_factor=[1.0, 1.0])
    for i, (c, k, b, ids) in enumerate(more):
        same_outputs(got[i], many.ref.update(k, b, ids, camera=c), f'after reset: entry {i}')
    assert many.ref.frame[1] == 1
    same_all(many, [0], 'after reset')
    same_all(many, [1], 'after reset', live_only=True)


def test_results_on_another_stream():
    """The launch goes to the current stream: results made on a side stream are read in order without a wait."""
    rng = np.random.default_rng(215)
    p = Pair(15, min_frames=1)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        for f in range(4):
            kpts, bboxes = people(rng, 7, f)
            kp, bb = torch.from_numpy(kpts).cuda(non_blocking=True), torch.from_numpy(bboxes).cuda(non_blocking=True)
            kp, bb = kp * 1.0, bb * 1.0                                   # made by a kernel of the side stream
            ids = torch.arange(1, 8, dtype=torch.int32, device='cuda')
            got = p.mon.update((bb, None, kp), ids)
            side.synchronize()
            same_outputs(got, p.ref.update(kpts, bboxes, np.arange(1, 8, dtype=np.int32)), f'side stream frame {f}')
        same_all(p, [0], 'side stream')
    assert p.ref.frame[0] == 4
