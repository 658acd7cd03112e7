"""Track trails on the device (csrc/pave_trails.hip, pave_trail_update) against the rule of DESIGN section 22 in numpy
(tests/trail_ref.py): after every frame the four outputs, every state tensor and the rings are compared with the oracle
by torch.equal, and the inputs with what they were.  Needs an MI355X."""
import numpy as np
import pytest
import torch

from tests import trail_cases as TC
from tests import trail_ref as TR
from tests.test_track_gpu import FIGURE15, poses, result

pytestmark = pytest.mark.gpu

OUTPUTS = ['count', 'span', 'dist', 'path']
STATE = ['id', 'last', 'pos', 'head', 'count', 'box', 'frame', 'dropped']
POINTS = ['pts', 'when', 'head', 'count']


class Pair:
    """A TrackTrails and the oracle, configured alike."""

    def __init__(self, K=15, **kw):
        from pavenet_amd import TrackTrails
        self.trails, self.ref = TrackTrails(K, **kw), TR.TrailRef(K, **kw)


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


def same_all(p, cameras, what):
    """The slots of the oracle that are live, their whole rings among them, and everything else whole (a free slot's
    other fields are never read)."""
    for c in cameras:
        got, exp = p.trails.state(c), p.ref.state(c)
        assert list(got) == STATE
        live = exp['id'] != 0
        for name in STATE:
            g, e = got[name], np.asarray(exp[name])
            if e.ndim >= 1 and name != 'id':
                g, e = g[torch.from_numpy(live).to(g.device)], e[live]
            same(g, e, f'{what}: camera {c} state {name}')
        got, exp = p.trails.points(c), p.ref.points(c)
        assert list(got) == POINTS
        for name in ('pts', 'when'):
            same(got[name][torch.from_numpy(live).to(got[name].device)], exp[name][live], f'{what}: camera {c} ring {name}')


def flat(res):
    return [t for t in (res.values() if isinstance(res, dict) else res) if isinstance(t, torch.Tensor)]


def step(p, kpts, bboxes, ids, what, keep=None, scale=None, camera=0, form='tuple'):
    """One frame through the device and the reference; everything compared, the inputs included.  Returns the oracle's
    outputs."""
    ids = np.asarray(ids, np.int64).astype(np.int32)
    exp = p.ref.update(kpts, bboxes, ids, keep, (1.0, 1.0) if scale is None else scale, camera)
    res, dev_ids = result(kpts, bboxes, keep, form), torch.from_numpy(ids).cuda()
    before = [t.clone() for t in flat(res) + [dev_ids]]
    got = p.trails.update(res, dev_ids, scale_factor=scale, camera=camera)
    same_outputs(got, exp, what)
    same_all(p, [camera], what)
    for t, b in zip(flat(res) + [dev_ids], before):
        assert torch.equal(t.view(torch.uint8), b.view(torch.uint8)) if t.numel() else True, f'{what}: an input changed'
    return exp


@pytest.mark.parametrize('script', TC.SCRIPTS, ids=lambda s: s.__name__)
def test_hand_worked_scripts_on_the_device(script):
    class Harness:
        def __init__(self, K, **kw):
            self.p = Pair(K, **kw)
            self.frames = 0

        def frame(self, kpts, bboxes, ids, keep=None, camera=0):
            self.frames += 1
            out = step(self.p, kpts, bboxes, ids, f'{script.__name__} frame {self.frames}',
                       None if keep is None else np.asarray(keep, np.int32), camera=camera,
                       form='tuple' if keep is None else 'dict')
            ref = self.p.ref
            views = {k: v.cpu().numpy() for k, v in dict(self.p.trails.state(camera), **self.p.trails.points(camera)).items()}
            TC.invariant(views, ref.L, ref.stride, ref.min_step, out, ids)
            return out

        def get(self, field, camera=0):
            return dict(self.p.trails.state(camera), **self.p.trails.points(camera))[field].cpu().numpy()
    script(Harness)


def people(rng, pos, height=60.0, scale=(1.0, 1.0)):
    return poses(rng, FIGURE15, np.asarray(pos, np.float64), height=height, scale=scale)


@pytest.mark.parametrize('length', [1, 2, 64])
def test_a_walker_wraps_the_ring_twice(length):
    """2 L + 3 commits of a walker beside a stander who commits nothing after the birth: the ring wraps twice and the
    oldest point is always L - 1 commits back."""
    rng = np.random.default_rng(221)
    p = Pair(15, length=length, max_tracks=4)
    frames = 2 * length + 4
    for f in range(frames):
        kpts, bboxes = people(rng, [(10.0 + 4.0 * f, 20.0 + 0.5 * f), (300.0, 50.0)])
        out = step(p, kpts, bboxes, [3, 8], f'length {length} frame {f}')
        assert out['count'][0] == min(f + 1, length) and out['span'][0] == min(f, length - 1)
    assert p.ref.count[0, 0] == length and p.ref.head[0, 0] == (frames - 1) % length
    assert p.ref.count[0, 1] == 1 and p.ref.when[0, 1, 0] == 1


def test_stride_three_and_a_large_step_for_a_stander_and_a_walker():
    """stride 3 with min_step 40 (5 pixels): the walker (6 pixels a frame) commits every third frame, the stander
    never, whatever the jitter."""
    rng = np.random.default_rng(222)
    p = Pair(15, stride=3, min_step=40, length=8, max_tracks=4)
    for f in range(30):
        kpts, bboxes = people(rng, [(10.0 + 6.0 * f, 20.0), (300.0, 50.0)])
        out = step(p, kpts, bboxes, [1, 2], f'frame {f}')
        assert out['count'][0] == min(1 + f // 3, 8) and out['count'][1] == 1
    assert sorted(p.ref.when[0, 0].tolist()) == list(range(7, 29, 3))


def test_gaps_shorter_and_longer_than_max_age():
    """max_age 3: a track seen in frame 3 and again in frame 6 (6 - 3 is not > 3) keeps its ring and the move spans the
    gap; one that misses four frames is freed in the fourth (10 - 6 > 3) and born again with a ring of one point."""
    rng = np.random.default_rng(223)
    p = Pair(15, max_age=3, length=8, max_tracks=4)
    none = np.zeros((0, 15, 3), np.float32), np.zeros((0, 5), np.float32)
    for f in range(3):
        step(p, *people(rng, [(10.0 + 5.0 * f, 20.0)]), [6], f'frame {f}')
    for f in range(2):
        step(p, *none, [], f'gap frame {f}')
    out = step(p, *people(rng, [(60.0, 20.0)]), [6], 'back in frame 6')
    assert out['count'].tolist() == [4] and out['span'].tolist() == [5]
    for f in range(4):
        step(p, *none, [], f'second gap frame {f}')
    assert p.ref.id[0, 0] == 0
    out = step(p, *people(rng, [(90.0, 20.0)]), [6], 'back in frame 11')
    assert out['count'].tolist() == [1] and out['span'].tolist() == [0] and p.ref.head[0, 0] == 0


def test_no_pose_one_pose_and_128_tracks():
    """N = 0 (the clock still runs), N = 1, then 128 poses with 128 ids walking for three frames; 129 poses are
    refused."""
    rng = np.random.default_rng(224)
    p = Pair(15, length=4)
    none = np.zeros((0, 15, 3), np.float32), np.zeros((0, 5), np.float32)
    out = step(p, *none, [], 'N = 0')
    assert out['count'].shape == (0,) and p.ref.frame[0] == 1
    step(p, *people(rng, [(100.0, 40.0)]), [9], 'N = 1')
    start = np.stack([20.0 + 14.0 * (np.arange(128) % 16), 10.0 + 30.0 * (np.arange(128) // 16)], 1)
    for f in range(3):
        order = rng.permutation(128)
        kpts, bboxes = people(rng, start + (6.0 * f, 4.0 * f))
        out = step(p, kpts[order], bboxes[order], (np.arange(1, 129))[order], f'N = 128 frame {f}')
    assert sorted(out['count'].tolist()) == [3] * 127 + [4] and p.ref.dropped[0] == 0 and (p.ref.id[0] != 0).sum() == 128   # (id 9)
    res = result(np.zeros((129, 15, 3), np.float32), np.zeros((129, 5), np.float32))
    with pytest.raises(ValueError, match='at most 128'):
        p.trails.update(res, torch.zeros(129, dtype=torch.int32, device='cuda'))


@pytest.mark.parametrize('form', ['tuple', 'dict'])
def test_both_result_forms_and_a_scale_factor(form):
    """Twelve people crossing a picture made at scale (0.694, 0.7), in both result forms, with junk that takes no part:
    keep = 0 (dict form), a score at the threshold, NaN and inf coordinates, an id of 0 and a duplicate id."""
    rng = np.random.default_rng(225)
    scale = (0.694, 0.7)
    p = Pair(15, max_age=3, max_tracks=16, length=6, stride=2, min_step=24)
    start = np.stack([-30.0 + 60.0 * np.arange(12), 20.0 + 22.0 * np.arange(12)], 1)
    speed = np.stack([np.where(np.arange(12) % 2 == 0, 6.5, -6.5), np.where(np.arange(12) % 3 == 0, 2.5, -1.5)], 1)
    for f in range(24):
        there = [q for q in range(12) if not (q == 3 and 5 <= f < 7) and not (q == 5 and 8 <= f < 14)]
        kpts, bboxes = people(rng, (start + speed * f)[there], scale=scale)
        junk_k, junk_b = people(rng, rng.uniform(0, 300, (6, 2)), scale=scale)
        junk_b[1, 4] = 0.3
        junk_k[2, rng.integers(15), 1] = np.nan
        junk_b[3, 0] = -np.inf
        keep = np.ones(len(there) + 6, np.int32)
        keep[len(there)] = 0
        ids = np.concatenate([np.asarray(there) + 1, [40, 41, 42, 43, 0, 1]])         # (id 1 is there[0]'s: a duplicate)
        if form == 'tuple':
            junk_k, junk_b, ids, keep = junk_k[1:], junk_b[1:], np.delete(ids, len(there)), None
        kpts, bboxes = np.concatenate([kpts, junk_k]), np.concatenate([bboxes, junk_b])
        order = np.concatenate([[0], 1 + rng.permutation(len(bboxes) - 1)])          # (the first of id 1 stays first)
        out = step(p, kpts[order], bboxes[order], ids[order], f'{form} frame {f}', None if keep is None else keep[order],
                   scale, form=form)
        junk = np.concatenate([np.zeros(len(there), bool), np.ones(len(bboxes) - len(there), bool)])[order]
        assert not out['count'][junk].any() and out['count'][~junk].all()
    assert p.ref.frame[0] == 24 and p.ref.count[0].max() == 6 and p.ref.dropped[0] == 0


def test_33_entries_of_two_cameras_in_two_launches():
    """update_many with 33 entries, 17 of camera 0 and 16 of camera 1 interleaved.  Against the same frames in single
    calls on a second object, and against two one-camera objects; the oracle runs beside all of them."""
    from pavenet_amd import TrackTrails
    rng = np.random.default_rng(226)
    kw = dict(max_age=2, max_tracks=6, length=5, min_step=8)
    many, single = Pair(15, cameras=2, **kw), TrackTrails(15, cameras=2, **kw)
    alone = [TrackTrails(15, **kw), TrackTrails(15, **kw)]
    frames = []
    for i in range(33):
        cam = i % 2
        n = int(rng.integers(0, 6))
        pos = np.stack([rng.uniform(-20, 200, n) + 3.0 * i, rng.uniform(-30, 90, n)], 1)
        kpts, bboxes = people(rng, pos, height=50.0)
        ids = rng.permutation(8)[:n].astype(np.int32)            # an id of 0 among them now and then
        frames.append((cam, kpts, bboxes, ids))
    items = [(cam, result(k, b), torch.from_numpy(ids).cuda()) for cam, k, b, ids in frames]
    outs = many.trails.update_many(items)
    assert len(outs) == 33
    for i, ((cam, kpts, bboxes, ids), item, out) in enumerate(zip(frames, items, outs)):
        exp = many.ref.update(kpts, bboxes, ids, camera=cam)
        same_outputs(out, exp, f'entry {i}')
        same_outputs(single.update(item[1], item[2], camera=cam), exp, f'entry {i} alone')
        same_outputs(alone[cam].update(item[1], item[2]), exp, f'entry {i} on a one-camera object')
    same_all(many, [0, 1], 'after 33 entries')
    assert many.ref.frame.tolist() == [17, 16] and many.ref.count.max() >= 3
    for cam in (0, 1):
        live = many.trails.state(cam)['id'] != 0
        for name in STATE + ['pts', 'when']:
            views = lambda m, c: dict(m.state(c), **m.points(c))[name]
            a, b, c = views(many.trails, cam), views(single, cam), views(alone[cam], 0)
            if a.dim() >= 1 and name != 'id':
                a, b, c = a[live], b[live], c[live]
            assert torch.equal(a, b) and torch.equal(a, c), name


def test_reset_of_one_camera_and_a_side_stream():
    """reset(camera=1) frees camera 1's slots and leaves camera 0's tensors and every data_ptr as they were; frames
    whose results were made on a side stream are counted on that stream."""
    rng = np.random.default_rng(227)
    p = Pair(15, cameras=2, max_tracks=4, length=4)
    for cam in (0, 1):
        for f in range(2):
            step(p, *people(rng, [(20.0 + 9 * f, 10.0), (120.0, 30.0 + 5 * f)], height=50.0), [1, 2], f'camera {cam} frame {f}',
                 camera=cam)
    ptrs = {k: v.data_ptr() for k, v in p.trails._state.items()}
    zero = {k: v[0].clone() for k, v in p.trails._state.items()}
    assert sorted(p.trails.device_tensors()) == sorted(set(ptrs) - {'dropped'})
    assert all(p.trails.device_tensors()[k].data_ptr() == ptrs[k] for k in p.trails.device_tensors())
    p.trails.reset(camera=1)
    p.ref.reset(1)
    assert {k: v.data_ptr() for k, v in p.trails._state.items()} == ptrs
    for k, v in zero.items():
        assert torch.equal(p.trails._state[k][0], v), k
    for k in ('id', 'frame', 'dropped'):
        assert not p.trails._state[k][1].any(), k
    same_all(p, [0, 1], 'after reset(1)')
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for f in range(3):
            step(p, *people(rng, [(30.0 + 8 * f, 12.0)], height=50.0), [5], f'side stream frame {f}', camera=1)
    torch.cuda.current_stream().wait_stream(side)
    assert p.ref.frame.tolist() == [2, 3]
    p.trails.reset()
    p.ref.reset()
    same_all(p, [0, 1], 'after reset()')


@pytest.mark.parametrize('anchor', ['feet', 'box', 'centre'])
def test_anchors_are_the_zone_monitors(anchor):
    """The same frames through a ZoneMonitor and a TrackTrails: slot for slot id, last and pos are equal, and with
    min_step 0 the newest committed point is that pos.  Key-point scores around kpt_thr, so 'feet' uses two, one or no
    ankle."""
    from pavenet_amd import ZoneMonitor
    rng = np.random.default_rng(228)
    scale = (1.3, 0.9)
    kw = dict(anchor=anchor, max_tracks=8, kpt_thr=0.4, max_age=1)
    p, mon = Pair(15, min_step=0, length=4, **kw), ZoneMonitor(15, **kw)
    for f in range(8):
        pos = np.stack([30.0 + 45.0 * np.arange(6) + 2.5 * f, 20.0 + 30.0 * np.arange(6)], 1)
        kpts, bboxes = poses(rng, FIGURE15, pos, height=90.0, scale=scale,
                             kpt_scores=rng.uniform(0.0, 1.0, (6, 15)).astype(np.float32))
        ids = np.asarray([1, 2, 3, 4, 5, 6], np.int32)
        step(p, kpts, bboxes, ids, f'{anchor} frame {f}', scale=scale)
        mon.update(result(kpts, bboxes), torch.from_numpy(ids).cuda(), scale_factor=scale)
        zs, ts, ring = mon.state(0), p.trails.state(0), p.trails.points(0)
        assert torch.equal(zs['id'], ts['id']) and torch.equal(zs['last'], ts['last']) and int((zs['id'] != 0).sum()) == 6
        assert torch.equal(zs['pos'][:6], ts['pos'][:6])
        newest = ring['pts'][torch.arange(6, device='cuda'), ring['head'][:6].long()]
        assert torch.equal(newest, zs['pos'][:6])


def test_updates_allocate_no_growing_memory():
    rng = np.random.default_rng(229)
    from pavenet_amd import TrackTrails
    trails = TrackTrails(15)
    res, ids = result(*people(rng, [(50.0, 40.0), (150.0, 80.0)])), torch.tensor([1, 2], dtype=torch.int32, device='cuda')
    trails.update(res, ids)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    for _ in range(100):
        out = trails.update(res, ids)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - base <= 8 * 512     # (the four small outputs of a call or two)
    assert int(trails.state(0)['frame']) == 101 and out['count'].tolist() == [1, 1] and out['span'].tolist() == [100, 100]
