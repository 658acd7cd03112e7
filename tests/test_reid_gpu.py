"""Re-identification on the device (csrc/pave_reid.hip) against the rule of DESIGN section 18 in numpy
(tests/reid_ref.py): every output and every state tensor of the gallery is compared with the oracle by torch.equal
after every frame, and the whole surface allocation with its copy from before the call.  Needs an MI355X."""
import numpy as np
import pytest
import torch

from tests import reid_cases as RC
from tests import reid_ref as RR
from tests import track_ref as TR
from tests import zones_ref as ZR

pytestmark = pytest.mark.gpu

STATE = ['person', 'track', 'last', 'hits', 'hist', 'frame', 'next', 'dropped']
THR = 28138


def same(got, exp, what):
    g, e = got.detach().cpu(), torch.from_numpy(np.array(exp, np.int32))
    assert g.dtype == torch.int32 and g.shape == e.shape, (what, g.dtype, tuple(g.shape), tuple(e.shape))
    assert torch.equal(g, e), f'{what}: {int((g != e).sum())} words differ, first at {(g != e).nonzero()[:4].tolist()}: ' \
                              f'{g[g != e][:4].tolist()} for {e[g != e][:4].tolist()}'


def result(kpts, bboxes, keep=None, form='tuple'):
    kp, bb = torch.from_numpy(np.ascontiguousarray(kpts)).cuda(), torch.from_numpy(np.ascontiguousarray(bboxes)).cuda()
    if form == 'tuple':
        assert keep is None
        return (bb, torch.zeros(len(bb), dtype=torch.int64, device='cuda'), kp)
    keep = torch.ones(1, len(bb), dtype=torch.int32).cuda() if keep is None else \
        torch.from_numpy(np.asarray(keep, np.int32))[None].cuda()
    return dict(bboxes=bb[None], kpts=kp[None], keep=keep)


class Pair:
    """A PersonReID and the oracle, configured alike."""

    def __init__(self, K=15, **kw):
        from pavenet_amd.reid import PersonReID
        self.dev, self.ref = PersonReID(K, **kw), RR.ReIDRef(K, default_thr=THR, **kw)

    def same_state(self, cameras, what):
        for c in cameras:
            got, exp = self.dev.state(c), self.ref.state(c)
            assert list(got) == STATE
            for name in STATE:
                same(got[name], exp[name], f'{what}: camera {c} state {name}')

    def step(self, surface, W, kpts, bboxes, ids, what, keep=None, scale=None, camera=0, form='tuple', kind='nv12'):
        """One frame through the device and the reference; everything compared.  Returns the oracle's outputs."""
        ids = np.asarray(ids, np.int64).astype(np.int32)
        exp = self.ref.update(kind, surface, W, kpts, bboxes, ids, keep, (1.0, 1.0) if scale is None else scale, camera)
        dev = torch.from_numpy(surface).cuda()
        res, tid = result(kpts, bboxes, keep, form), torch.from_numpy(ids).cuda()
        got = self.dev.update_nv12(dev, W, res, tid, scale_factor=scale, camera=camera) if kind == 'nv12' else \
            self.dev.update_bgr(dev, res, tid, scale_factor=scale, camera=camera)
        assert sorted(got) == ['ids', 'sim'] and all(v.is_cuda for v in got.values())
        same(got['ids'], exp['ids'], f'{what}: ids')
        same(got['sim'], exp['sim'], f'{what}: sim')
        assert torch.equal(dev.cpu(), torch.from_numpy(surface)), f'{what}: the surface was written'
        self.same_state([camera], what)
        return exp


def check_describe(kind, picture, W, kpts, bboxes, keep=None, scale=None, K=15, what='', **kw):
    """describe on the device against the oracle, the whole allocation compared -> the oracle's dict."""
    from pavenet_amd.reid import PersonReID
    g = PersonReID(K, **kw)
    dev = picture if isinstance(picture, torch.Tensor) else torch.from_numpy(picture).cuda()
    host = dev.cpu().numpy().copy()
    res = result(kpts, bboxes, keep, 'tuple' if keep is None else 'dict')
    got = g.describe_nv12(dev, W, res, scale_factor=scale) if kind == 'nv12' else g.describe_bgr(dev, res, scale_factor=scale)
    exp = RR.describe(kind, host, W, kpts, bboxes, keep, (1.0, 1.0) if scale is None else scale, K, kw.get('torso'),
                      kw.get('legs'))
    assert sorted(got) == ['count', 'hist']
    same(got['count'], exp['count'], f'{what}: count')
    same(got['hist'], exp['hist'], f'{what}: hist')
    assert np.array_equal(dev.cpu().numpy(), host), f'{what}: the picture was written'
    assert g.state(0) is None
    return exp


def figures(rng, n, W, H, height, scale=(1.0, 1.0)):
    pos = np.stack([rng.uniform(-0.1 * height, W - 0.3 * height, n), rng.uniform(-0.2 * height, H - 0.6 * height, n)], 1)
    return RC.poses15(rng, pos, height, scale)


@pytest.mark.parametrize('scale', [None, (0.694, 0.7)])
@pytest.mark.parametrize('W,H,pitch', [(70, 50, 96), (130, 70, 160)])
def test_describe_nv12_odd_chroma_extents(W, H, pitch, scale):
    """Surfaces with odd chroma extents.  Poses 0 .. 3 stand on the left, top, right and bottom border, so a valid
    region is clipped at each of the four (asserted); 16 more lie anywhere over the picture, 4 are too small for 16
    samples and 4 are wholly outside (count 0).  The device equals the oracle.  The (matrix, range) labels of a
    surface cannot matter: the describe and update calls take none, the descriptor is made of the stored bytes."""
    rng = np.random.default_rng(W)
    sc = (1.0, 1.0) if scale is None else scale
    edge_k, edge_b = RC.poses15(rng, [(-12, 5), (20, -20), (W - 12, 5), (20, H - 25)], 60.0, sc)
    kpts, bboxes = figures(rng, 24, W, H, 40.0, sc)
    kpts, bboxes = np.concatenate([edge_k, kpts]), np.concatenate([edge_b, bboxes])
    kpts[24:] += np.float32(400.0)          # wholly outside
    bboxes[24:, :4] += np.float32(400.0)
    kpts[20:24, :, :2] = kpts[20:24, :1, :2] + (kpts[20:24, :, :2] - kpts[20:24, :1, :2]) * np.float32(0.2)   # tiny
    exp = check_describe('nv12', RC.noise_nv12(H, W, pitch, 3), W, kpts, bboxes, scale=scale, what=f'{W}x{H}')
    count, rect = exp['count'], exp['rect']
    assert (count[:4, 0] >= RR.MIN_SAMPLES).all()
    assert kpts[0, 3, 0] < 0 and kpts[1, 3, 1] < 0                                     # left, top: clamped to 0
    assert (rect[2, 0, 2] >> 3) > W // 2 - 1 and (rect[3, 0, 3] >> 3) > H // 2 - 1     # right, bottom: clipped
    assert (count[24:] == 0).all() and (count[20:24] == 0).all() and (count[4:20] > 0).any()
    assert (count >= RR.MIN_SAMPLES)[count > 0].all() and exp['hist'][count == 0].sum() == 0


def test_describe_strides_fallback_widening_and_keep():
    """288 x 208: a figure large enough for stride 2 and small ones at stride 1; a side view (shoulders and hips at
    one x: the rectangle is widened), invisible shoulders (the box fallback; no legs fallback), keep = 0, a score at
    the threshold and a NaN, which give count 0."""
    W, H, pitch = 288, 208, 320
    rng = np.random.default_rng(11)
    kpts, bboxes = RC.poses15(rng, [(10, 4), (150, 20), (200, 30), (230, 90), (60, 100), (100, 100), (120, 30)], 80.0)
    big_k, big_b = RC.poses15(rng, [(20, -100)], 400.0)
    kpts, bboxes = np.concatenate([big_k, kpts]), np.concatenate([big_b, bboxes])
    kpts[1, [3, 4, 9, 10], 0] = kpts[1, 3, 0]         # a side view
    kpts[2, [3, 4], 2] = 0.0                          # no shoulders: the torso falls back to the box
    kpts[3, [9, 10], 2] = 0.0                         # no hips: a box torso and no legs
    bboxes[5, 4] = 0.3
    kpts[6, 7, 1] = np.nan
    keep = np.ones(8, np.int32)
    keep[4] = 0
    exp = check_describe('nv12', RC.noise_nv12(H, W, pitch, 5), W, kpts, bboxes, keep=keep, what='288x208')
    count = exp['count']
    blocks = RR.blocks_of(tuple(int(v) for v in exp['rect'][0, 0]), W, H)
    assert count[0, 0] > 0 and blocks[4] >= 2                       # the large torso is read at a stride
    assert count[3, 0] > 0 and count[3, 1] == 0 and (count[4:7] == 0).all() and count[7, 0] > 0


@pytest.mark.parametrize('K', [17, 14, 5])
def test_describe_other_skeletons(K):
    rng = np.random.default_rng(K)
    kw = dict(torso=((0, 1), (2,)), legs=((2,), (3, 4))) if K == 5 else {}
    W, H = 160, 120
    kpts = np.empty((6, K, 3), np.float32)
    kpts[..., 0] = rng.uniform(0, W, (6, 1)) + rng.uniform(-30, 30, (6, K))
    kpts[..., 1] = rng.uniform(0, H, (6, 1)) + rng.uniform(-40, 40, (6, K))
    kpts[..., 2] = rng.uniform(-0.2, 1.0, (6, K))
    bboxes = np.stack([kpts[..., 0].min(1), kpts[..., 1].min(1), kpts[..., 0].max(1), kpts[..., 1].max(1), np.full(6, 0.9)],
                      1).astype(np.float32)
    exp = check_describe('nv12', RC.noise_nv12(H, W, 160, K), W, kpts, bboxes, K=K, what=f'K {K}', **kw)
    assert (exp['count'] > 0).any()


def test_describe_bgr_and_an_odd_base():
    """[49, 71, 3] (the last odd row and column are not sampled), and the same picture as a view that starts at an
    odd byte of its allocation (the byte path)."""
    rng = np.random.default_rng(2)
    H, W = 49, 71
    picture = torch.from_numpy(rng.integers(0, 256, (H, W, 3), dtype=np.uint8))
    kpts, bboxes = figures(rng, 12, W, H, 40.0)
    a = check_describe('bgr', picture.cuda(), None, kpts, bboxes, what='bgr')
    flat = torch.full((H * W * 3 + 8,), RC.SENTINEL, dtype=torch.uint8).cuda()
    view = flat[1:1 + H * W * 3].view(H, W, 3)
    view.copy_(picture)
    b = check_describe('bgr', view, None, kpts, bboxes, what='bgr odd base')
    assert np.array_equal(a['hist'], b['hist']) and (a['count'] > 0).any()
    assert (flat[0] == RC.SENTINEL) and (flat[1 + H * W * 3:] == RC.SENTINEL).all()
    wide = torch.from_numpy(rng.integers(0, 256, (40, 64, 3), dtype=np.uint8)).cuda()     # rows of 192 bytes: the dword path
    kpts, bboxes = figures(rng, 8, 64, 40, 36.0)
    assert (check_describe('bgr', wide, None, kpts, bboxes, what='bgr dwords')['count'] > 0).any()


def scene(rng, W, H, there, shirts, trousers, height=60):
    """-> (surface, kpts, bboxes) of the people `there`: (person, x, y)."""
    people = [(x, y, height, shirts[p], trousers[p]) for p, x, y in there]
    kpts, bboxes = RC.poses15(rng, np.asarray([(x, y) for _, x, y in there], np.float64).reshape(-1, 2), height)
    return RC.paint_nv12(rng, W, H, W + 16, people), kpts, bboxes


@pytest.mark.parametrize('form', ['tuple', 'dict'])
def test_a_gallery_script(form):
    """People come, leave and return under new track ids; poses that take no part (keep 0, id 0, a duplicate id,
    NaN) ride along; an empty frame; slots expire after max_lost; the device equals the oracle after every frame
    and a return is re-identified (asserted, so an idle kernel cannot pass)."""
    rng = np.random.default_rng(4)
    shirts, trousers = RC.colours(6, 4)
    W, H = 400, 96
    p = Pair(15, max_people=8, max_lost=12, match_thr=THR, min_hits=2)
    spots = [(10 + 64 * i, 10 + 3 * i) for i in range(6)]
    script = [([0, 1, 2], [1, 2, 3])] * 3 + [([0, 2], [1, 3])] * 2 + [([0, 2, 1], [1, 3, 4])] * 2 + [([], [])] + \
             [([3], [5])] * 2 + [([1, 3, 0], [6, 5, 7])] * 2 + [([4], [8])] * 13 + [([0, 4], [9, 8])] * 2
    sims = 0
    for f, (who, ids) in enumerate(script):
        surface, kpts, bboxes = scene(rng, W, H, [(q, *spots[q]) for q in who], shirts, trousers)
        ids, keep = list(ids), None
        if f % 3 == 1 and who:       # riders: a duplicate of the first id, id 0, a NaN pose, and in dict form keep = 0
            k2, b2 = RC.poses15(rng, [(300, 20), (330, 20), (350, 20), (370, 20)], 60)
            k2[2, 4, 0] = np.nan
            kpts, bboxes, ids = np.concatenate([kpts, k2]), np.concatenate([bboxes, b2]), ids + [ids[0], 0, 30, 31]
            if form == 'dict':
                keep = np.ones(len(ids), np.int32)
                keep[-1] = 0
            else:
                kpts, bboxes, ids = kpts[:-1], bboxes[:-1], ids[:-1]
        exp = p.step(surface, W, kpts, bboxes, ids, f'{form} frame {f}', keep=keep, form=form)
        sims += int((exp['sim'] > 0).sum())
    assert sims >= 3 and p.ref.next[0] >= 6


def test_ties_overlap_min_hits_eviction_and_drops():
    """An exact tie: one painted figure pasted at two places gives two slots and later two new poses the same
    descriptors; the lower pose row takes the lower slot.  Then the overlap guard (two boxes over each other: no
    update), a slot below min_hits that is no candidate, eviction of the oldest lost slot and a drop with every slot
    live."""
    rng = np.random.default_rng(9)
    shirts, trousers = RC.colours(4, 9)
    W, H = 320, 96
    one, k1, b1 = scene(rng, 80, H, [(0, 10, 10)], shirts, trousers)
    surface = np.full((H * 3 // 2, W + 16), RC.SENTINEL, np.uint8)
    surface[:, :W] = np.tile(one[:, :80], (1, 4))
    k1[..., :2], b1[:, :4] = np.round(k1[..., :2] * 4) / 4, np.round(b1[:, :4] * 4) / 4     # so that + 160 is exact
    kpts, bboxes = np.concatenate([k1, k1]), np.concatenate([b1, b1])
    kpts[1, :, 0] += 160
    bboxes[1, [0, 2]] += 160
    p = Pair(15, max_people=3, max_lost=50, match_thr=THR, min_hits=2)
    for f in range(2):
        p.step(surface, W, kpts, bboxes, [1, 2], f'tie frame {f}')
    p.step(surface, W, kpts[:0], bboxes[:0], [], 'tie: nobody')
    exp = p.step(surface, W, kpts[::-1], bboxes[::-1], [3, 4], 'tie: both return')
    assert exp['ids'].tolist() == [1, 2] and exp['sim'][0] == exp['sim'][1] > THR     # row 0 took slot 0
    # the overlap guard: two poses over each other, nothing is learnt
    before = p.ref.hits[0].copy()
    k2, b2 = kpts.copy(), bboxes.copy()
    k2[1], b2[1] = k2[0], b2[0]
    p.step(surface, W, k2, b2, [3, 4], 'overlap')
    assert np.array_equal(before, p.ref.hits[0])
    # a person seen once (min_hits 2) is no candidate: a new person id, then the oldest lost slot is evicted and
    # with every slot live a pose is dropped
    q = Pair(15, max_people=2, max_lost=50, match_thr=THR, min_hits=2)
    q.step(surface, W, kpts[:1], bboxes[:1], [1], 'min_hits: seen once')
    q.step(surface, W, kpts[:0], bboxes[:0], [], 'min_hits: gone')
    exp = q.step(surface, W, kpts[:1], bboxes[:1], [2], 'min_hits: back')
    assert exp['ids'].tolist() == [2] and exp['sim'].tolist() == [0]
    exp = q.step(surface, W, kpts[1:], bboxes[1:], [3], 'evict the oldest')
    assert exp['ids'].tolist() == [3] and q.ref.person[0].tolist() == [3, 2]
    three = np.concatenate([kpts, kpts[:1]])
    three[2, :, 0] += 80
    exp = q.step(surface, W, three, np.concatenate([bboxes, bboxes[:1] + np.float32([80, 0, 80, 0, 0])]), [7, 8, 9], 'drop')
    assert exp['ids'].tolist()[2] == 0 and q.ref.dropped[0] == 1


def test_a_revived_track_gets_no_duplicate_person_id():
    """Track 1's person leaves, track 2 takes its slot over (the same clothes), then the tracker revives track 1 beside
    track 2: two different person ids."""
    rng = np.random.default_rng(6)
    shirts, trousers = RC.colours(1, 6)
    W, H = 240, 96
    p = Pair(15, max_people=4, match_thr=THR, min_hits=2)
    for f, (there, ids) in enumerate([([(0, 10, 10)], [1])] * 3 + [([], [])] + [([(0, 120, 12)], [2])] * 2 +
                                     [([(0, 120, 12), (0, 10, 10)], [2, 1])] * 2):
        surface, kpts, bboxes = scene(rng, W, H, there, shirts, trousers)
        exp = p.step(surface, W, kpts, bboxes, ids, f'revive frame {f}')
    assert exp['ids'].tolist() == [1, 2] and p.ref.track[0, :2].tolist() == [2, 1]


def test_128_poses_many_entries_and_cameras():
    """N = 128 in a frame (and N = 0, N = 1); 33 entries of three interleaved cameras in one call (two launches)
    against three galleries of one camera each fed frame by frame; reset(camera)."""
    from pavenet_amd.reid import PersonReID
    rng = np.random.default_rng(12)
    W, H = 640, 240
    surface = RC.noise_nv12(H, W, W, 8)
    pos = np.stack([8.0 + 38 * (np.arange(128) % 16), 4.0 + 28 * (np.arange(128) // 16)], 1)
    kpts, bboxes = RC.poses15(rng, pos, 36.0)
    p = Pair(15, max_people=128, match_thr=THR, min_hits=1)
    p.step(surface, W, kpts, bboxes, np.arange(1, 129), '128 poses')
    p.step(surface, W, kpts[:0], bboxes[:0], [], 'no pose')
    exp = p.step(surface, W, kpts[::-1], bboxes[::-1], np.arange(201, 329), '128 poses return')
    assert (exp['sim'] > 0).sum() > 64
    p.step(surface, W, kpts[:1], bboxes[:1], [500], 'one pose')

    many, ones = PersonReID(15, cameras=3, max_people=16, min_hits=1), [PersonReID(15, max_people=16, min_hits=1) for _ in range(3)]
    dev = torch.from_numpy(surface).cuda()
    items, want = [], []
    for i in range(33):
        c = (i * 2) % 3
        pick = rng.permutation(128)[:int(rng.integers(0, 9))]
        res, ids = result(kpts[pick], bboxes[pick]), torch.from_numpy((pick + 1 + 200 * (i // 11)).astype(np.int32)).cuda()
        items.append((c, dev, W, res, ids))
        want.append(ones[c].update_nv12(dev, W, res, ids))
    got = many.update_many_nv12(items)
    for i, (g, w) in enumerate(zip(got, want)):
        assert torch.equal(g['ids'], w['ids']) and torch.equal(g['sim'], w['sim']), f'entry {i}'
    for c in range(3):
        for name in STATE:
            assert torch.equal(many.state(c)[name], ones[c].state(0)[name]), (c, name)
    assert sum(int((g['sim'] > 0).sum()) for g in got) > 0
    many.reset(1)
    assert int(many.state(1)['person'].abs().sum()) == 0 and int(many.state(1)['frame']) == 0
    assert int(many.state(1)['next']) == int(ones[1].state(0)['next']) and int(many.state(0)['frame']) > 0


def test_the_chain_tracker_reid_smoother_zones_draw():
    """Painted figures through PoseTracker.update -> PersonReID.update_nv12 -> PoseSmoother.smooth and
    ZoneMonitor.update with the person ids -> draw_poses_nv12(ids=) of the smoothed poses, each against its oracle
    in that order.  Figure 0 is hidden for max_age + 5 frames: its track id changes, its person id does not, and the
    zone, whose max_age is the gallery's max_lost, reports no VANISH / APPEAR for it."""
    from pavenet_amd.render import DIGIT_FONT, TrackStyle, draw_poses_nv12
    from pavenet_amd.smoothing import PoseSmoother
    from pavenet_amd.tracking import PoseTracker
    from pavenet_amd.zones import ZoneMonitor
    from tests import render_ids_ref as IR
    from tests import smooth_ref as SR
    rng = np.random.default_rng(21)
    shirts, trousers = RC.colours(2, 21)
    W, H, max_age, max_lost = 320, 128, 4, 40
    tracker, tref = PoseTracker(15, max_age=max_age), TR.TrackRef(15, max_age=max_age)
    p = Pair(15, max_people=8, max_lost=max_lost, match_thr=THR, min_hits=2)
    smoother, sref = PoseSmoother(15, max_age=max_lost), SR.SmoothRef(15, max_age=max_lost)
    zone, zref = ZoneMonitor(15, max_age=max_lost), ZR.ZoneRef(15, max_age=max_lost)
    style = TrackStyle(15)
    whole = [(0, 0), (W, 0), (W, H), (0, H)]
    zone.set_zones(0, [whole])
    zref.set_zones(0, [whole])
    kinds, seen = [], []
    for f in range(4 + max_age + 5 + 3):
        hidden = 4 <= f < 4 + max_age + 5
        there = [(1, 200, 20)] + ([] if hidden else [(0, 20 + 2 * f, 10)])
        surface, kpts, bboxes = scene(rng, W, H, there, shirts, trousers, height=90)
        res = result(kpts, bboxes)
        ids = tracker.update(res)
        same(ids, tref.update(kpts, bboxes), f'frame {f}: track ids')
        exp = p.step(surface, W, kpts, bboxes, ids.cpu().numpy(), f'frame {f}')
        dev = torch.from_numpy(surface).cuda()
        person = torch.from_numpy(exp['ids']).cuda()
        steady = smoother.smooth(res, person)
        exp_k, exp_b = sref.smooth(kpts, bboxes, exp['ids'], None, (1.0, 1.0))
        for got, want, name in ((steady[2], exp_k, 'kpts'), (steady[0], exp_b, 'bboxes')):
            assert torch.equal(got.cpu().contiguous().view(torch.int32),
                               torch.from_numpy(np.ascontiguousarray(want)).view(torch.int32)), f'frame {f}: smoothed {name}'
        z = zone.update(res, person)
        zexp = zref.update(kpts, bboxes, exp['ids'])
        for name in ('zones', 'dwell', 'events', 'n_events'):
            same(z[name], zexp[name], f'frame {f}: zone {name}')
        kinds += [int(k) for k in zexp['events'][:int(zexp['n_events']), 0]]
        draw_poses_nv12(dev, W, steady, scale_factor=None, style=style, ids=person)
        want = IR.draw_nv12(surface, W, exp_k, exp_b, None, exp['ids'], (1.0, 1.0), style, style.palette, DIGIT_FONT)
        assert torch.equal(dev.cpu(), torch.from_numpy(want)), f'frame {f}: the drawn surface'
        assert not np.array_equal(want, surface)
        seen.append((ids.cpu().tolist(), exp['ids'].tolist()))
    first, last = seen[3], seen[-1]
    assert last[0][1] != first[0][1] and last[1][1] == first[1][1] and last[1][0] == first[1][0]
    assert kinds.count(ZR.APPEAR) == 2 and ZR.VANISH not in kinds


def test_a_bgr_gallery():
    """pave_reid_update_bgr: people on [H, W, 3] pictures come, leave and return under new track ids, frame by frame
    against the oracle; then the same frames through one update_many_bgr call on a second gallery."""
    from pavenet_amd.reid import PersonReID
    rng = np.random.default_rng(31)
    H, W = 97, 203
    picture = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    picture[:, :100] //= 4                       # two halves of different colours
    kpts, bboxes = RC.poses15(rng, [(10, 10), (60, 20), (120, 8), (160, 25)], 60.0)
    script = [([0, 1, 2], [1, 2, 3])] * 2 + [([1], [2])] + [([3, 1, 0], [4, 2, 5])] * 2 + [([2, 3], [6, 4])]
    p = Pair(15, max_people=4, match_thr=THR, min_hits=2)
    sims, items, want = 0, [], []
    dev = torch.from_numpy(picture).cuda()
    for f, (who, ids) in enumerate(script):
        exp = p.step(picture, None, kpts[who], bboxes[who], ids, f'bgr frame {f}', kind='bgr')
        sims += int((exp['sim'] > 0).sum())
        items.append((0, dev, result(kpts[who], bboxes[who]), torch.tensor(ids, dtype=torch.int32).cuda()))
        want.append(exp)
    assert sims >= 2
    many = PersonReID(15, max_people=4, match_thr=THR, min_hits=2)
    for f, (got, exp) in enumerate(zip(many.update_many_bgr(items), want)):
        same(got['ids'], exp['ids'], f'update_many_bgr entry {f}: ids')
        same(got['sim'], exp['sim'], f'update_many_bgr entry {f}: sim')
    for name in STATE:
        same(many.state(0)[name], p.ref.state(0)[name], f'update_many_bgr: state {name}')
    with pytest.raises(ValueError, match='one kind'):
        many.update_nv12(torch.zeros(72, 64, dtype=torch.uint8).cuda(), 64, result(kpts[:1], bboxes[:1]),
                         torch.ones(1, dtype=torch.int32).cuda())


def test_the_calls_run_no_torch_operator_and_read_nothing_on_the_host():
    """A warm update_nv12, update_many_nv12 and describe_nv12 under census.LaunchCensus: no torch compute operator on
    a device tensor, no other ATen launch (allocations are none) and no host read or sync."""
    from pavenet_amd.census import LaunchCensus
    from pavenet_amd.reid import PersonReID
    rng = np.random.default_rng(41)
    W, H = 160, 96
    dev = torch.from_numpy(RC.noise_nv12(H, W, 192, 2)).cuda()
    kpts, bboxes = RC.poses15(rng, [(10, 10), (60, 20), (110, 8)], 60.0)
    forms = [result(kpts, bboxes), result(kpts, bboxes, np.ones(3, np.int32), 'dict')]
    ids = torch.tensor([1, 2, 3], dtype=torch.int32).cuda()
    g = PersonReID(15, cameras=2)
    g.update_nv12(dev, W, forms[0], ids)        # the first call allocates the gallery
    torch.cuda.synchronize()
    with LaunchCensus() as c:
        for res in forms:
            out = g.update_nv12(dev, W, res, ids, scale_factor=(1.0, 1.0))
            outs = g.update_many_nv12([(0, dev, W, res, ids), (1, dev, W, res, ids)])
            desc = g.describe_nv12([dev, dev], W, [res, res])
    assert not c.fallback_ops and not c.aten_launches and not c.host_syncs, c.summary()
    assert out['ids'].cpu().tolist() == [1, 2, 3] and outs[1]['ids'].cpu().tolist() == [1, 2, 3]
    assert int(desc[1]['count'].sum()) > 0
