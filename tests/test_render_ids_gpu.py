"""Track ids drawn into NV12 and BGR frames on the device (pave_draw.hip, the IDS instantiations) against the numpy
statement of the rule (tests/render_ids_ref.py): torch.equal of the WHOLE allocation -- noise in the picture, a
sentinel in the pitch padding -- as tests/test_render_gpu.py does for the plain draw.  The default surface is
96 x 64 NV12 at pitch 128: three tiles across, two down.  Needs an MI355X."""
import numpy as np
import pytest
import torch

from tests import render_ids_ref as IR
from tests import render_ref as RR

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5
W0, H0, PITCH0 = 96, 64, 128
INT_MAX = 2147483647


@pytest.fixture(autouse=True)
def _split_gemm_mode():
    """The live test's model runs under set_batch_invariant, which needs the library's default GEMM mode, whatever
    mode an earlier module left behind."""
    from pavenet_amd import bricks
    old = bricks.get_gemm_mode()
    bricks.set_gemm_mode('bf16x3')
    yield
    bricks.set_gemm_mode(old)


def _surface(H, W, pitch, seed=0):
    g = torch.Generator().manual_seed(seed)
    s = torch.full((H * 3 // 2, pitch), SENTINEL, dtype=torch.uint8)
    s[:, :W] = torch.randint(0, 256, (H * 3 // 2, W), dtype=torch.uint8, generator=g)
    return s


def _figures(boxes, K, seed=0, score=0.9):
    """One pose per (x0, y0, x1, y1): K seeded key points inside the box, which is also its bbox."""
    rng = np.random.default_rng(seed)
    n = len(boxes)
    kpts = np.empty((n, K, 3), np.float32)
    bboxes = np.empty((n, 5), np.float32)
    for p, (x0, y0, x1, y1) in enumerate(boxes):
        kpts[p, :, 0] = rng.uniform(x0, x1, K)
        kpts[p, :, 1] = rng.uniform(y0, y1, K)
        bboxes[p] = (x0, y0, x1, y1, score)
    kpts[..., 2] = rng.uniform(0.1, 1.0, (n, K))
    return kpts, bboxes


def _dev(kpts, bboxes, keep=None):
    res = dict(bboxes=torch.from_numpy(bboxes).cuda(), kpts=torch.from_numpy(kpts).cuda())
    if keep is not None:
        res['keep'] = torch.from_numpy(np.asarray(keep, np.int32)).cuda()
    return res


def _ids(ids):
    return None if ids is None else torch.from_numpy(np.asarray(ids, np.int32)).cuda()


def _check_nv12(kpts, bboxes, ids, style, H=H0, W=W0, pitch=PITCH0, keep=None, scale=None, matrix='bt601',
                full_range=False, seed=0):
    """One surface through draw_poses_nv12(ids=) against the oracle, whole allocation -> (drawn, untouched)."""
    from pavenet_amd.render import DIGIT_FONT, draw_poses_nv12
    before = _surface(H, W, pitch, seed)
    dev = before.cuda()
    out = draw_poses_nv12(dev, W, _dev(kpts, bboxes, keep), scale_factor=scale, style=style, matrix=matrix,
                          full_range=full_range, ids=_ids(ids))
    assert out is dev
    ids = None if ids is None else np.asarray(ids, np.int32)
    want = torch.from_numpy(IR.draw_nv12(before.numpy(), W, kpts, bboxes, keep, ids, scale or (1.0, 1.0), style,
                                         style.palette, DIGIT_FONT, matrix, full_range))
    got = dev.cpu()
    diff = (got != want).nonzero()
    assert torch.equal(got, want), f'{len(diff)} bytes differ, first at (row, column) {diff[:5].tolist()}'
    return got, before


def _id_map(kpts, bboxes, ids, style, W=W0, H=H0, keep=None):
    from pavenet_amd.render import DIGIT_FONT
    return IR.id_map_and_colours(W, H, kpts, bboxes, keep, np.asarray(ids, np.int32), (1.0, 1.0), style, style.palette,
                                 DIGIT_FONT)[0]


@pytest.mark.parametrize('matrix,full_range', [('bt601', False), ('bt601', True), ('bt709', False), ('bt709', True)])
def test_all_four_tables(matrix, full_range):
    from pavenet_amd.render import TrackStyle
    kpts, bboxes = _figures([(6, 24, 40, 60), (50, 30, 90, 58), (30, 20, 70, 50)], 15, seed=1)
    got, before = _check_nv12(kpts, bboxes, [3, 12, 0], TrackStyle(15, draw_boxes=True), matrix=matrix,
                              full_range=full_range)
    assert (got != before).any() and torch.equal(got[:, W0:], before[:, W0:])


def test_label_across_tile_borders_and_tiles_only_a_label_touches():
    """The skeleton sits in the lower-left tile; its 62 x 18 label crosses x = 32, x = 64 and y = 32, and the two
    upper-right tiles are touched by the label and by no capsule: the pose cull must keep the pose for them."""
    from pavenet_amd.render import TrackStyle
    kpts, bboxes = _figures([(4, 40, 27, 60)], 15, seed=2)
    style = TrackStyle(15)
    plate = 1 * 34
    m = _id_map(kpts, bboxes, [99999], style)
    ys, xs = np.nonzero(m >= plate)
    assert (xs.min(), xs.max(), ys.min(), ys.max()) == (4, 65, 22, 39)
    assert (m[:32, 32:] >= plate).any() and not ((m[:32, 32:] >= 0) & (m[:32, 32:] < plate)).any()
    assert (m[:32, 64:] >= plate).any() and (m[32:, 32:64] >= plate).any()
    _check_nv12(kpts, bboxes, [99999], style)


@pytest.mark.parametrize('g', [2, 1])
def test_id_values(g):
    """0, -5 (untracked), 1, 9, 10 (a second digit), 32, 33 (the colour of 1), 99 999 and, at g = 1, 2^31 - 1."""
    from pavenet_amd.render import TrackStyle, draw_poses_nv12
    ids = [0, -5, 1, 9, 10, 32, 33, 99999] + ([INT_MAX] if g == 1 else [])
    boxes = [(2 + 10 * i, 20 + 4 * (i % 3), 30 + 7 * i, 44 + 2 * i) for i in range(len(ids))]
    if g == 1:
        boxes[-1] = (20, 50, 70, 62)
    kpts, bboxes = _figures(boxes, 15, seed=3)
    style = TrackStyle(15, label_scale=g, draw_boxes=True)
    _check_nv12(kpts, bboxes, ids, style)
    if g == 1:   # 10 digits: 61 x 9 pixels from (20, 41)
        ys, xs = np.nonzero(_id_map(kpts, bboxes, ids, style) >= len(ids) * 34 + 2 * 8)
        assert (xs.min(), xs.max(), ys.min(), ys.max()) == (20, 80, 41, 49)
    # id 33 is drawn in the colour of id 1
    a, b = _surface(H0, W0, PITCH0).cuda(), _surface(H0, W0, PITCH0).cuda()
    colours = TrackStyle(15, label_scale=0)
    draw_poses_nv12(a, W0, _dev(kpts[:1], bboxes[:1]), style=colours, ids=_ids([1]))
    draw_poses_nv12(b, W0, _dev(kpts[:1], bboxes[:1]), style=colours, ids=_ids([33]))
    assert torch.equal(a, b) and not torch.equal(a.cpu(), _surface(H0, W0, PITCH0))


@pytest.mark.parametrize('g', [0, 1, 2, 8])
def test_label_scales(g):
    """g = 0 draws colours only; g = 8 makes a 104 x 72 plate for two digits, clipped at the right and bottom edges
    of the 96 x 64 surface (ay clamps at 0)."""
    from pavenet_amd.render import TrackStyle
    kpts, bboxes = _figures([(10, 30, 60, 60), (40, 26, 90, 50)], 15, seed=4)
    style = TrackStyle(15, label_scale=g)
    m = _id_map(kpts, bboxes, [47, 5], style)
    assert (m >= 2 * 34).any() == (g > 0)
    if g == 8:
        assert (m[:, W0 - 1] >= 2 * 34).any() and (m[H0 - 1] >= 2 * 34).any() and (m[0] >= 2 * 34).any()
    _check_nv12(kpts, bboxes, [47, 5], style)


def test_clamp_at_the_top_and_clipping_at_the_right_and_bottom():
    """A box at y = 0 (the plate lies over the box from row 0), a box near the right edge (the plate is cut at x = W),
    and a box whose top is below the surface (the plate is cut at y = H)."""
    from pavenet_amd.render import TrackStyle
    kpts, bboxes = _figures([(8, 0, 40, 30), (80, 30, 95, 60), (30, 70, 60, 90)], 15, seed=5)
    kpts[2, :, 1] = np.clip(kpts[2, :, 1], 0, 63)
    style = TrackStyle(15, draw_boxes=True)
    ids = [120, 4321, 77]
    m = _id_map(kpts, bboxes, ids, style)
    rects = []
    for p in range(3):
        ys, xs = np.nonzero((m == 3 * 34 + 2 * p) | (m == 3 * 34 + 2 * p + 1))
        rects.append((xs.min(), xs.max(), ys.min(), ys.max()))
    assert rects == [(8, 45, 0, 17), (80, 95, 12, 29), (30, 55, 52, 63)]
    _check_nv12(kpts, bboxes, ids, style)


def test_labels_lie_above_every_skeleton_and_the_later_label_wins():
    """Pose 0's label under the limbs of pose 1: the label wins.  Two overlapping labels: the larger p wins."""
    from pavenet_amd.render import TrackStyle
    kpts, bboxes = _figures([(20, 40, 60, 62), (10, 10, 80, 50), (30, 44, 70, 60)], 15, seed=6)
    kpts[..., 2] = 0.9
    style = TrackStyle(15)
    ids = [2024, 7, 31]
    m = _id_map(kpts, bboxes, ids, style)
    label0 = np.zeros_like(m, bool)
    label0[22:40, 20:20 + 2 * 25] = True                     # pose 0's plate: 50 x 18 from (20, 22)
    alone = RR.id_map(W0, H0, [pr for pr in RR.primitives(kpts, bboxes, None, (1.0, 1.0), style) if pr[0] // 34 == 1])
    assert ((alone >= 0) & label0).sum() > 20               # pose 1's capsules cross it ...
    label2 = np.zeros_like(m, bool)
    label2[26:44, 30:30 + 2 * 13] = True                     # pose 2's plate: 26 x 18 from (30, 26)
    assert (m[label0 & ~label2] >= 3 * 34).all() and (m[label0 & ~label2] <= 3 * 34 + 1).all()   # ... and lose
    assert (label0 & label2).sum() > 100 and (m[label2] >= 3 * 34 + 4).all()
    _check_nv12(kpts, bboxes, ids, style)


def test_untracked_style_against_skip():
    from pavenet_amd.render import PoseStyle, TrackStyle
    kpts, bboxes = _figures([(6, 24, 40, 60), (50, 30, 90, 58), (30, 20, 70, 50)], 15, seed=7)
    ids = [0, 5, -1]
    a, before = _check_nv12(kpts, bboxes, ids, TrackStyle(15, draw_boxes=True))
    b, _ = _check_nv12(kpts, bboxes, ids, TrackStyle(15, draw_boxes=True, untracked='skip'))
    only, _ = _check_nv12(kpts[1:2], bboxes[1:2], [5], TrackStyle(15, draw_boxes=True))
    assert not torch.equal(a, b) and (b != before).any()
    # under 'skip' the picture holds pose 1 alone, but its label keeps the primitive id of p = 1 among N = 3 poses
    assert torch.equal(b, only)
    # nothing tracked: 'skip' writes nothing, 'style' is the plain draw
    c, _ = _check_nv12(kpts, bboxes, [0, 0, -7], TrackStyle(15, untracked='skip'))
    assert torch.equal(c, before)
    d, _ = _check_nv12(kpts, bboxes, [0, 0, -7], TrackStyle(15))
    want = RR.draw_nv12(before.numpy(), W0, kpts, bboxes, None, (1.0, 1.0), PoseStyle(15))
    assert torch.equal(d, torch.from_numpy(want))


def test_poses_that_are_not_drawn_have_no_label():
    """keep = 0, a score at the threshold, NaN and inf coordinates, each with a valid id: no label and no write."""
    from pavenet_amd.render import TrackStyle
    boxes = [(6 + 14 * i, 24, 30 + 12 * i, 60) for i in range(6)]
    kpts, bboxes = _figures(boxes, 15, seed=8)
    bboxes[1, 4] = np.float32(0.3)
    kpts[2, 4, 0] = np.nan
    bboxes[3, 1] = np.inf
    kpts[4, 9, 1] = -np.inf
    keep, ids = [0, 1, 1, 1, 1, 1], [11, 12, 13, 14, 15, 16]
    style = TrackStyle(15, score_thr=0.3)
    got, before = _check_nv12(kpts, bboxes, ids, style, keep=keep)
    alone, _ = _check_nv12(kpts[5:], bboxes[5:], ids[5:], style)
    m = _id_map(kpts, bboxes, ids, style, keep=keep)
    assert set(np.unique(m[m >= 6 * 34]).tolist()) == {6 * 34 + 10, 6 * 34 + 11}
    assert torch.equal(got, alone) and (got != before).any()
    got, before = _check_nv12(kpts[:5], bboxes[:5], ids[:5], style, keep=keep[:5])
    assert torch.equal(got, before)


def test_no_poses():
    from pavenet_amd.render import TrackStyle
    got, before = _check_nv12(np.zeros((0, 15, 3), np.float32), np.zeros((0, 5), np.float32), np.zeros(0, np.int32),
                              TrackStyle(15))
    assert torch.equal(got, before)


@pytest.mark.parametrize('boxes', [False, True])
def test_boxes_on_and_off(boxes):
    """The label is placed by the box also when the box is not drawn; a drawn box takes the id's colour."""
    from pavenet_amd.render import TrackStyle
    kpts, bboxes = _figures([(10, 30, 50, 60), (44, 22, 90, 56)], 15, seed=9)
    bboxes[:, :4] += np.float32([-3, -4, 3, 2])          # the boxes are wider than their key points
    style = TrackStyle(15, draw_boxes=boxes, thickness=2, radius=3, kpt_thr=0.5)
    m = _id_map(kpts, bboxes, [8, 0], style)
    ys, xs = np.nonzero(m >= 2 * 34)
    assert (xs.min(), ys.max()) == (7, 25)
    assert ((m >= 0) & (m < 4)).any() == boxes
    _check_nv12(kpts, bboxes, [8, 0], style)


@pytest.mark.parametrize('K', [15, 14, 32])
def test_skeleton_variants(K):
    from pavenet_amd.render import TrackStyle
    skeleton = None
    if K == 32:
        skeleton = ([(e, (e * 7 + 3) % 32) for e in range(32)], [(e * 8, 255 - e * 8, (e * 37) % 256) for e in range(32)],
                    [(255 - k * 8, (k * 53) % 256, k * 8) for k in range(32)])
    kpts, bboxes = _figures([(6, 24, 40, 60), (50, 30, 90, 58), (30, 20, 70, 50)], K, seed=10 + K)
    _check_nv12(kpts, bboxes, [64, 0, 1000], TrackStyle(K, thickness=2, radius=3, skeleton=skeleton, draw_boxes=True),
                matrix='bt709')


def test_33_surfaces_take_two_launches():
    """33 surfaces of different sizes, pitches, matrices, ranges, scales and N in one call, every third one without
    ids: each equals the oracle."""
    from pavenet_amd.render import DIGIT_FONT, TrackStyle, draw_poses_nv12
    style = TrackStyle(15, draw_boxes=True)
    specs = []
    for i in range(33):
        W, H = 34 + 2 * (i % 7) * 6, 28 + 2 * (i % 5) * 7
        specs.append(dict(W=W, H=H, pitch=W + (i % 3) * 5, matrix=('bt601', 'bt709')[i % 2], full_range=bool(i % 4 >= 2),
                          scale=(1.0 + 0.01 * i, 1.0 + 0.02 * (i % 3)), n=i % 4))
    befores = [_surface(s['H'], s['W'], s['pitch'], seed=100 + i) for i, s in enumerate(specs)]
    poses, ids = [], []
    for i, s in enumerate(specs):
        boxes = [(2 + 5 * p, 12 + 2 * p, s['W'] - 4 - 3 * p, s['H'] - 2 - p) for p in range(s['n'])]
        kpts, bboxes = _figures(boxes, 15, seed=200 + i)
        kpts[..., :2] *= np.float32(s['scale'])
        bboxes[:, :4] *= np.float32(s['scale'] * 2)
        poses.append((kpts, bboxes))
        ids.append(None if i % 3 == 2 else np.asarray([(7 * i + 30 * p) % 41 - 3 for p in range(s['n'])], np.int32))
    together = [b.cuda() for b in befores]
    out = draw_poses_nv12(together, [s['W'] for s in specs], [_dev(k, b) for k, b in poses],
                          scale_factor=[s['scale'] for s in specs], style=style, matrix=[s['matrix'] for s in specs],
                          full_range=[s['full_range'] for s in specs], ids=[_ids(v) for v in ids])
    assert out is together
    labelled = 0
    for i, s in enumerate(specs):
        want = IR.draw_nv12(befores[i].numpy(), s['W'], poses[i][0], poses[i][1], None, ids[i], s['scale'], style,
                            style.palette, DIGIT_FONT, s['matrix'], s['full_range'])
        assert torch.equal(together[i].cpu(), torch.from_numpy(want)), i
        labelled += int(ids[i] is not None and (ids[i] >= 1).any())
    assert labelled >= 10


def test_bgr_at_odd_sizes():
    """draw_poses_bgr(ids=) on [49, 71, 3]: 2 x 2 blocks that hang over the right and bottom borders, a label cut
    at the right border."""
    from pavenet_amd.render import DIGIT_FONT, TrackStyle, draw_poses_bgr
    g = torch.Generator().manual_seed(11)
    before = torch.randint(0, 256, (49, 71, 3), dtype=torch.uint8, generator=g)
    kpts, bboxes = _figures([(4, 22, 40, 48), (44, 20, 70, 48), (20, 30, 60, 44)], 15, seed=11)
    kpts[1, 0, :2] = (70.0, 48.0)
    style = TrackStyle(15, draw_boxes=True)
    for ids, scale in (([15, 123456, 0], None), ([1, 2, 3], (0.694, 0.6944))):
        dev = before.cuda()
        res = _dev(kpts * np.float32((scale or (1, 1)) + (1,)), bboxes * np.float32((scale or (1, 1)) * 2 + (1,)))
        assert draw_poses_bgr(dev, res, scale_factor=scale, style=style, ids=_ids(ids)) is dev
        want = IR.draw_bgr(before.numpy(), res['kpts'].cpu().numpy(), res['bboxes'].cpu().numpy(), None,
                           np.asarray(ids, np.int32), scale or (1.0, 1.0), style, style.palette, DIGIT_FONT)
        assert torch.equal(dev.cpu(), torch.from_numpy(want))
        assert (dev.cpu() != before).any()
    dev = before.cuda()
    draw_poses_bgr([dev], [_dev(kpts, bboxes)], ids=[None], style=style)
    assert torch.equal(dev.cpu(), torch.from_numpy(RR.draw_bgr(before.numpy(), kpts, bboxes, None, (1.0, 1.0), style)))


def test_without_ids_the_call_is_todays():
    """ids=None goes through the plain entry point: byte for byte the plain draw, with a TrackStyle too; and a list
    of ids that are all None, through the new entry point, draws the same picture."""
    from pavenet_amd.render import PoseStyle, TrackStyle, draw_poses_nv12
    kpts, bboxes = _figures([(6, 24, 40, 60), (50, 30, 90, 58), (30, 20, 70, 50)], 15, seed=12)
    before = _surface(H0, W0, PITCH0, seed=12)
    want = torch.from_numpy(RR.draw_nv12(before.numpy(), W0, kpts, bboxes, None, (1.0, 1.0), PoseStyle(15)))
    for kw in (dict(), dict(ids=None), dict(ids=None, style=TrackStyle(15)), dict(ids=[None])):
        dev = before.cuda()
        surfaces, results = ([dev], [_dev(kpts, bboxes)]) if 'ids' in kw and kw['ids'] is not None else (dev, _dev(kpts, bboxes))
        draw_poses_nv12(surfaces, W0, results, **kw)
        assert torch.equal(dev.cpu(), want), kw


def test_live_results_tracked_and_drawn_onto_their_surfaces():
    """Five NV12 frames through preprocess_surfaces_nv12 -> LiveVideoPose -> PoseTracker.update ->
    draw_poses_nv12(ids=) on their own surfaces; the ids come to the host only afterwards, for the oracle."""
    from pavenet_amd.live import LiveVideoPose
    from pavenet_amd.preprocess import preprocess_surfaces_nv12
    from pavenet_amd.render import DIGIT_FONT, TrackStyle, draw_poses_nv12
    from pavenet_amd.tracking import PoseTracker
    from tests.test_live_gpu import _model
    m = _model(3)
    K = m.bbox_head.num_keypoints
    befores = [_surface(96, 120, 128, seed=300 + i) for i in range(5)]
    surfaces = [b.cuda() for b in befores]
    img, meta = preprocess_surfaces_nv12(surfaces, 120, img_scale=(160, 128), size_divisor=32)
    live = LiveVideoPose(m, meta, max_push=1)
    tracker = PoseTracker(K, score_thr=0.0)
    style = TrackStyle(K, score_thr=-1.0, draw_boxes=True, label_scale=1)
    got = []
    for i in range(5):
        got += live.push(img[i])
    got += live.flush()
    assert [c for c, _ in got] == [0, 1, 2, 3, 4]
    kept = []
    for c, res in got:
        ids = tracker.update(res, scale_factor=meta['scale_factor'])
        draw_poses_nv12(surfaces[c], 120, res, scale_factor=meta['scale_factor'], style=style, ids=ids)
        kept.append(ids)
    tracked = 0
    for (c, res), ids in zip(got, kept):
        bboxes, _, kpts = (t.cpu().numpy() for t in res)
        ids = ids.cpu().numpy()
        want = IR.draw_nv12(befores[c].numpy(), 120, kpts, bboxes, None, ids, meta['scale_factor'][:2], style,
                            style.palette, DIGIT_FONT)
        assert torch.equal(surfaces[c].cpu(), torch.from_numpy(want)), c
        tracked += int((ids >= 1).sum())
    assert tracked > 0
