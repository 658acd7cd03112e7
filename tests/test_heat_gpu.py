"""Footfall maps on the device (csrc/pave_heat.hip, pave_heat_update) against the rule of DESIGN section 21 in numpy
(tests/heat_ref.py): after every frame the three outputs, every state tensor and both maps with their peak are
compared with the oracle by torch.equal, and the inputs with what they were.  Needs an MI355X."""
import numpy as np
import pytest
import torch

from tests import heat_cases as HC
from tests import heat_ref as HR
from tests.test_track_gpu import FIGURE15, poses, result

pytestmark = pytest.mark.gpu

OUTPUTS = ['cell', 'dwell', 'visits']
STATE = ['id', 'last', 'cell', 'frame', 'dropped']
MAPS = ['dwell', 'visits', 'peak']


class Pair:
    """A FootfallMap and the oracle, configured alike."""

    def __init__(self, K=15, **kw):
        from pavenet_amd import FootfallMap
        self.map, self.ref = FootfallMap(K, **kw), HR.HeatRef(K, **kw)


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


def same_all(p, cameras, what, live_only=True):
    """The slots of the oracle that are live, and everything else whole (a free slot's other fields are never read)."""
    for c in cameras:
        got, exp = p.map.state(c), p.ref.state(c)
        assert list(got) == STATE
        live = exp['id'] != 0
        for name in STATE:
            g, e = got[name], np.asarray(exp[name])
            if live_only and e.ndim >= 1 and name != 'id':
                g, e = g[torch.from_numpy(live).to(g.device)], e[live]
            same(g, e, f'{what}: camera {c} state {name}')
        got, exp = p.map.maps(c), p.ref.maps(c)
        assert list(got) == MAPS
        for name in MAPS:
            same(got[name], exp[name], f'{what}: camera {c} {name}')


def flat(res):
    return [t for t in (res.values() if isinstance(res, dict) else res) if isinstance(t, torch.Tensor)]


def step(p, kpts, bboxes, ids, what, keep=None, scale=None, camera=0, form='tuple'):
    """One frame through the device and the reference; everything compared, the inputs included.  Returns the oracle's
    outputs."""
    ids = np.asarray(ids, np.int64).astype(np.int32)
    exp = p.ref.update(kpts, bboxes, ids, keep, (1.0, 1.0) if scale is None else scale, camera)
    res, dev_ids = result(kpts, bboxes, keep, form), torch.from_numpy(ids).cuda()
    before = [t.clone() for t in flat(res) + [dev_ids]]
    got = p.map.update(res, dev_ids, scale_factor=scale, camera=camera)
    same_outputs(got, exp, what)
    same_all(p, [camera], what)
    for t, b in zip(flat(res) + [dev_ids], before):
        assert torch.equal(t.view(torch.uint8), b.view(torch.uint8)) if t.numel() else True, f'{what}: an input changed'
    return exp


@pytest.mark.parametrize('script', HC.SCRIPTS, ids=lambda s: s.__name__)
def test_hand_worked_scripts_on_the_device(script):
    class Harness:
        def __init__(self, K, **kw):
            self.p = Pair(K, **kw)
            self.frames = 0

        def frame(self, kpts, bboxes, ids, entries, keep=None, camera=0):
            self.frames += 1
            ref = self.p.ref
            before = {k: v.copy() for k, v in ref.maps(camera).items()}
            out = step(self.p, kpts, bboxes, ids, f'{script.__name__} frame {self.frames}',
                       None if keep is None else np.asarray(keep, np.int32), camera=camera,
                       form='tuple' if keep is None else 'dict')
            frame, hl = int(ref.frame[camera]), ref.half_life
            HC.invariant(before, ref.maps(camera), out, ref.radius, hl > 0 and frame % hl == 0, entries)
            return out

        def get(self, field, camera=0):
            views = dict(self.p.map.state(camera), **self.p.map.maps(camera))
            return views[field].cpu().numpy()
    script(Harness)


def people(rng, pos, height=60.0, scale=(1.0, 1.0)):
    return poses(rng, FIGURE15, np.asarray(pos, np.float64), height=height, scale=scale)


@pytest.mark.parametrize('size, cell, radius', [((3, 2), 4, 3), ((37, 19), 8, 2), ((37, 19), 8, 0), ((100, 70), 64, 1)])
def test_small_and_ragged_grids(size, cell, radius):
    """A grid of one cell (every footprint loses all but its centre), a ragged 5 x 3 one whose last column and row are
    cut by the picture's edge, and a 2 x 2 one at the largest cell: people walk in from outside, across and out."""
    rng = np.random.default_rng(211)
    p = Pair(15, size=size, cell=cell, radius=radius, max_age=2, max_tracks=5)
    assert (p.map.Gw, p.map.Gh) == {(3, 2): (1, 1), (37, 19): (5, 3), (100, 70): (2, 2)}[size]
    h = 0.4 * min(size)
    on = off = 0
    for f in range(12):
        # feet at y = top + h; four people on a diagonal drift that starts left of and above the picture
        pos = [(-0.3 * size[0] + (0.12 * f + 0.3 * i) * size[0], -h + (0.1 * f + 0.2 * i) * size[1]) for i in range(4)]
        kpts, bboxes = people(rng, pos, height=h)
        ids = [1, 2, 3, 4] if f != 5 else [1, 2, 2, 0]
        out = step(p, kpts, bboxes, ids, f'{size} frame {f}')
        on += int((out['cell'] >= 0).sum())
        off += int((p.ref.slot_cell[0][p.ref.id[0] != 0] == -1).any())
    assert on >= 4 and off >= 1, 'somebody was on the map and somebody off it'
    assert p.ref.dwell[0].sum() > 0 and p.ref.visits[0].sum() >= 2


def test_the_largest_grid_forgets_every_frame():
    """512 x 512 cells, half_life 1: three frames, each halving all 2 x 262 144 words inside the launch before its
    splats.  The maps start from words written here, odd and large ones among them, so the halving is seen on
    every word and not only under the poses."""
    rng = np.random.default_rng(212)
    p = Pair(15, size=(2048, 2048), cell=4, radius=3, half_life=1, max_tracks=8)
    p.map._allocate(torch.device('cuda', torch.cuda.current_device()))
    for name in ('dwell', 'visits'):
        start = rng.integers(0, 2 ** 31 - 1, (512, 512), dtype=np.int64).astype(np.int32)
        start[rng.random((512, 512)) < 0.5] = 0
        start[511, 511], start[0, 0] = 2 ** 31 - 1 - 2048, 7
        getattr(p.ref, name)[0] = start
        p.map.maps(0)[name].copy_(torch.from_numpy(start))
    p.ref.peak[0] = [p.ref.dwell[0].max(), p.ref.visits[0].max()]
    p.map.maps(0)['peak'].copy_(torch.from_numpy(p.ref.peak[0]))
    for f in range(3):
        kpts, bboxes = people(rng, [(2.0 + 300.0 * f, -55.0), (1000.0, 900.0), (2020.0, 1985.0), (1500.0 + 4 * f, 20.0)])
        step(p, kpts, bboxes, [1, 2, 3, 4], f'frame {f}')
    assert p.ref.frame[0] == 3 and p.ref.dwell[0, 511, 511] >= (2 ** 31 - 1 - 2048) >> 3


def test_no_pose_one_pose_and_128_on_one_cell():
    """N = 0 (the clock still runs), N = 1, then 128 poses with 128 ids whose feet stand on one cell at radius 3: 49
    cells take 128 atomic adds each in one frame and must come out exact; 129 poses are refused."""
    rng = np.random.default_rng(213)
    p = Pair(15, size=(320, 240), cell=8, radius=3)
    none = np.zeros((0, 15, 3), np.float32), np.zeros((0, 5), np.float32)
    out = step(p, *none, [], 'N = 0')
    assert out['cell'].shape == (0,) and p.ref.frame[0] == 1
    step(p, *people(rng, [(100.0, 40.0)]), [9], 'N = 1')
    # feet at (150 + 12, 64 + 60) with a jitter below a pixel: all within cell (20, 15), x in 160 .. 168, y in 120 .. 128
    kpts, bboxes = people(rng, np.tile([[150.0, 64.0]], (128, 1)), height=60.0)
    kpts[..., :2] += rng.uniform(-0.3, 0.3, (128, 15, 2)).astype(np.float32)
    out = step(p, kpts, bboxes, np.arange(1, 129), 'N = 128')
    assert (out['cell'] == out['cell'][0]).all() and out['cell'][0] >= 0
    assert out['dwell'].tolist() == [128 * 16] * 128 and out['visits'].tolist() == [128] * 128
    assert p.ref.dropped[0] == 0 and p.ref.peak[0].tolist() == [2048, 128]        # (id 9 came over from its own cell)
    again = step(p, kpts, bboxes, np.arange(1, 129), 'N = 128 again')
    assert again['dwell'].tolist() == [256 * 16] * 128 and again['visits'].tolist() == [128] * 128
    res = result(np.zeros((129, 15, 3), np.float32), np.zeros((129, 5), np.float32))
    with pytest.raises(ValueError, match='at most 128'):
        p.map.update(res, torch.zeros(129, dtype=torch.int32, device='cuda'))


@pytest.mark.parametrize('form', ['tuple', 'dict'])
def test_both_result_forms_and_a_scale_factor(form):
    """Twelve people crossing a 640 x 360 picture made at scale (0.694, 0.7), in both result forms, with junk that takes
    no part: keep = 0 (dict form), a score at the threshold, NaN and inf coordinates."""
    rng = np.random.default_rng(214)
    scale = (0.694, 0.7)
    p = Pair(15, size=(640, 360), cell=16, radius=1, half_life=7, max_age=3, max_tracks=16)
    start = np.stack([-30.0 + 60.0 * np.arange(12), 20.0 + 22.0 * np.arange(12)], 1)
    speed = np.stack([np.where(np.arange(12) % 2 == 0, 6.5, -6.5), np.where(np.arange(12) % 3 == 0, 2.5, -1.5)], 1)
    for f in range(24):
        there = [q for q in range(12) if not (q == 3 and 5 <= f < 7) and not (q == 5 and 8 <= f < 14)]
        kpts, bboxes = people(rng, (start + speed * f)[there], scale=scale)
        junk_k, junk_b = people(rng, rng.uniform(0, 300, (4, 2)), scale=scale)
        junk_b[1, 4] = 0.3
        junk_k[2, rng.integers(15), 1] = np.nan
        junk_b[3, 0] = -np.inf
        keep = np.ones(len(there) + 4, np.int32)
        keep[len(there)] = 0
        ids = np.concatenate([np.asarray(there) + 1, [40, 41, 42, 43]])
        if form == 'tuple':
            junk_k, junk_b, ids, keep = junk_k[1:], junk_b[1:], np.delete(ids, len(there)), None
        kpts, bboxes = np.concatenate([kpts, junk_k]), np.concatenate([bboxes, junk_b])
        order = rng.permutation(len(bboxes))
        out = step(p, kpts[order], bboxes[order], ids[order], f'{form} frame {f}', None if keep is None else keep[order],
                   scale, form=form)
        assert (out['cell'][ids[order] >= 40] == -1).all()
    assert p.ref.frame[0] == 24 and p.ref.visits[0].sum() > 0 and (p.ref.slot_cell[0][p.ref.id[0] != 0] == -1).any()


def test_33_entries_of_two_cameras_in_two_launches():
    """update_many with 33 entries, 17 of camera 0 and 16 of camera 1 interleaved, half_life 3: forget frames fall
    between two entries of one camera inside the first launch (frames 3, 6, ...).  Against the same frames in single
    calls on a second map, and against two one-camera maps; the oracle runs beside all of them."""
    from pavenet_amd import FootfallMap
    rng = np.random.default_rng(215)
    kw = dict(size=(200, 120), cell=8, radius=2, half_life=3, max_age=2, max_tracks=6)
    many, single = Pair(15, cameras=2, **kw), FootfallMap(15, cameras=2, **kw)
    alone = [FootfallMap(15, **kw), FootfallMap(15, **kw)]
    frames = []
    for i in range(33):
        cam = i % 2
        n = int(rng.integers(0, 6))
        pos = np.stack([rng.uniform(-20, 200, n) + 3.0 * i, rng.uniform(-30, 90, n)], 1)
        kpts, bboxes = people(rng, pos, height=50.0)
        ids = rng.permutation(8)[:n].astype(np.int32)            # an id of 0 among them now and then
        frames.append((cam, kpts, bboxes, ids))
    items = [(cam, result(k, b), torch.from_numpy(ids).cuda()) for cam, k, b, ids in frames]
    outs = many.map.update_many(items)
    assert len(outs) == 33
    for i, ((cam, kpts, bboxes, ids), item, out) in enumerate(zip(frames, items, outs)):
        exp = many.ref.update(kpts, bboxes, ids, camera=cam)
        same_outputs(out, exp, f'entry {i}')
        same_outputs(single.update(item[1], item[2], camera=cam), exp, f'entry {i} alone')
        same_outputs(alone[cam].update(item[1], item[2]), exp, f'entry {i} on a one-camera map')
    same_all(many, [0, 1], 'after 33 entries')
    assert many.ref.frame.tolist() == [17, 16] and many.ref.dwell.sum() > 0
    for name in STATE + MAPS:
        for cam in (0, 1):
            views = lambda m, c: dict(m.state(c), **m.maps(c))[name]
            assert torch.equal(views(many.map, cam), views(single, cam)), name
            assert torch.equal(views(many.map, cam), views(alone[cam], 0)), name


def test_reset_of_one_camera_and_a_side_stream():
    """reset(camera=1) clears camera 1 and leaves camera 0's tensors and every data_ptr as they were; frames whose
    results were made on a side stream are counted on that stream."""
    rng = np.random.default_rng(216)
    p = Pair(15, cameras=2, size=(200, 120), cell=8, max_tracks=4)
    for cam in (0, 1):
        for f in range(2):
            step(p, *people(rng, [(20.0 + 9 * f, 10.0), (120.0, 30.0 + 5 * f)], height=50.0), [1, 2], f'camera {cam} frame {f}',
                 camera=cam)
    ptrs = {k: v.data_ptr() for k, v in p.map._state.items()}
    zero = {k: v[0].clone() for k, v in p.map._state.items()}
    p.map.reset(camera=1)
    p.ref.reset(1)
    assert {k: v.data_ptr() for k, v in p.map._state.items()} == ptrs
    for k, v in zero.items():
        assert torch.equal(p.map._state[k][0], v), k
    for k in ('id', 'frame', 'dropped', 'peak', 'dwell', 'visits'):
        assert not p.map._state[k][1].any(), k
    same_all(p, [0, 1], 'after reset(1)')
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for f in range(3):
            step(p, *people(rng, [(30.0 + 8 * f, 12.0)], height=50.0), [5], f'side stream frame {f}', camera=1)
    torch.cuda.current_stream().wait_stream(side)
    assert p.ref.frame.tolist() == [2, 3]
    p.map.reset()
    p.ref.reset()
    same_all(p, [0, 1], 'after reset()')


@pytest.mark.parametrize('anchor', ['feet', 'box', 'centre'])
def test_anchors_are_the_zone_monitors(anchor):
    """The same frames through a ZoneMonitor and a FootfallMap (cell 4, the finest): slot for slot the map's cell is
    the cell of the monitor's pos, and the oracle's anchors -- which give the map the device was compared with -- ARE
    the monitor's pos, to the 1/8 pixel.  Key-point scores around kpt_thr, so 'feet' uses two, one or no ankle."""
    from pavenet_amd import ZoneMonitor
    rng = np.random.default_rng(217)
    scale = (1.3, 0.9)
    kw = dict(anchor=anchor, max_tracks=8, kpt_thr=0.4, max_age=1)
    p, mon = Pair(15, size=(400, 300), cell=4, **kw), ZoneMonitor(15, **kw)
    for f in range(8):
        pos = np.stack([30.0 + 45.0 * np.arange(6) + 2.5 * f, 20.0 + 30.0 * np.arange(6)], 1)
        kpts, bboxes = poses(rng, FIGURE15, pos, height=90.0, scale=scale,
                             kpt_scores=rng.uniform(0.0, 1.0, (6, 15)).astype(np.float32))
        ids = np.asarray([1, 2, 3, 4, 5, 6], np.int32)
        step(p, kpts, bboxes, ids, f'{anchor} frame {f}', scale=scale)
        mon.update(result(kpts, bboxes), torch.from_numpy(ids).cuda(), scale_factor=scale)
        zs, ms = mon.state(0), p.map.state(0)
        assert torch.equal(zs['id'], ms['id']) and torch.equal(zs['last'], ms['last']) and int((zs['id'] != 0).sum()) == 6
        live = zs['id'] != 0
        pos8 = zs['pos'][live].cpu().numpy().astype(np.int64)
        on = (pos8[:, 0] < 8 * 400) & (pos8[:, 1] < 8 * 300)
        want = np.where(on, (pos8[:, 1] >> 5) * p.map.Gw + (pos8[:, 0] >> 5), -1)
        assert ms['cell'][live].cpu().numpy().tolist() == want.tolist()
        assert zs['id'][:6].tolist() == ids.tolist()          # slot t holds pose t: the anchors line up
        assert pos8.tolist() == p.ref.anchors.tolist()


def test_updates_allocate_no_growing_memory():
    rng = np.random.default_rng(218)
    from pavenet_amd import FootfallMap
    fmap = FootfallMap(15, size=(320, 240))
    res, ids = result(*people(rng, [(50.0, 40.0), (150.0, 80.0)])), torch.tensor([1, 2], dtype=torch.int32, device='cuda')
    fmap.update(res, ids)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    for _ in range(100):
        out = fmap.update(res, ids)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - base <= 8 * 512     # (the three small outputs of a call or two)
    assert int(fmap.state(0)['frame']) == 101 and int(fmap.maps(0)['peak'][0]) == 101 * 4
