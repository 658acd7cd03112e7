"""Poses drawn into NV12 and BGR frames on the device (pave_draw.hip) against the numpy statement of DESIGN section 13
(tests/render_ref.py): torch.equal of the WHOLE allocation -- the picture is pre-filled with noise and the pitch
padding with a sentinel, so a byte written where the rule covers nothing fails the test too.  Needs an MI355X."""
import functools

import numpy as np
import pytest
import torch

from tests import render_ref as RR

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5


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
    """[H * 3 // 2, pitch] uint8 on the host: noise in the picture's columns, SENTINEL in the pitch padding."""
    g = torch.Generator().manual_seed(seed)
    s = torch.full((H * 3 // 2, pitch), SENTINEL, dtype=torch.uint8)
    s[:, :W] = torch.randint(0, 256, (H * 3 // 2, W), dtype=torch.uint8, generator=g)
    return s


def _poses(n, K, W, H, seed=0, spread=1.0, score=0.9):
    """n seeded poses over a W x H picture -> (kpts [n, K, 3], bboxes [n, 5]) float32 numpy."""
    rng = np.random.default_rng(seed)
    kpts = np.empty((n, K, 3), np.float32)
    cx, cy = rng.uniform(0.2 * W, 0.8 * W, (n, 1)), rng.uniform(0.2 * H, 0.8 * H, (n, 1))
    kpts[..., 0] = np.clip(cx + rng.uniform(-0.5, 0.5, (n, K)) * W * spread, 0, W - 1)
    kpts[..., 1] = np.clip(cy + rng.uniform(-0.5, 0.5, (n, K)) * H * spread, 0, H - 1)
    kpts[..., 2] = rng.uniform(0.1, 1.0, (n, K))
    bboxes = np.stack([kpts[..., 0].min(1), kpts[..., 1].min(1), kpts[..., 0].max(1), kpts[..., 1].max(1),
                       np.full(n, score)], 1).astype(np.float32)
    return kpts, bboxes


def _dev(kpts, bboxes, keep=None):
    res = dict(bboxes=torch.from_numpy(bboxes).cuda(), kpts=torch.from_numpy(kpts).cuda())
    if keep is not None:
        res['keep'] = torch.from_numpy(np.asarray(keep, np.int32)).cuda()
    return res


def _check_nv12(H, W, pitch, kpts, bboxes, style, keep=None, scale=None, matrix='bt601', full_range=False, seed=0):
    """One surface through draw_poses_nv12 against the oracle, whole allocation -> (drawn, untouched) host tensors."""
    from pavenet_amd.render import draw_poses_nv12
    before = _surface(H, W, pitch, seed)
    dev = before.cuda()
    out = draw_poses_nv12(dev, W, _dev(kpts, bboxes, keep), scale_factor=scale, style=style, matrix=matrix,
                          full_range=full_range)
    assert out is dev
    sc = (1.0, 1.0) if scale is None else scale
    want = torch.from_numpy(RR.draw_nv12(before.numpy(), W, kpts, bboxes, keep, sc, style, matrix, full_range))
    got = dev.cpu()
    diff = (got != want).nonzero()
    assert torch.equal(got, want), f'{len(diff)} bytes differ, first at (row, column) {diff[:5].tolist()}'
    return got, before


@pytest.mark.parametrize('matrix,full_range', [('bt601', False), ('bt601', True), ('bt709', False), ('bt709', True)])
def test_base_case_nv12(matrix, full_range):
    """70 x 50, pitch 96, K = 17, three poses whose primitives cross the tile borders at x = 32 and y = 32."""
    from pavenet_amd.render import PoseStyle
    kpts, bboxes = _poses(3, 17, 70, 50, seed=1)
    style = PoseStyle(17)
    prims = RR.primitives(kpts, bboxes, None, (1.0, 1.0), style)
    assert any(min(A[0], B[0]) < 4 * 32 < max(A[0], B[0]) for _, A, B, _, _ in prims)
    assert any(min(A[1], B[1]) < 4 * 32 < max(A[1], B[1]) for _, A, B, _, _ in prims)
    got, before = _check_nv12(50, 70, 96, kpts, bboxes, style, matrix=matrix, full_range=full_range)
    assert (got != before).any() and torch.equal(got[:, 70:], before[:, 70:])


def test_painters_order():
    """Two overlapping poses: the later pose is on top, and swapping them changes the picture as the oracle says."""
    from pavenet_amd.render import PoseStyle
    kpts, bboxes = _poses(2, 17, 70, 50, seed=2)
    kpts[1, :, :2] = kpts[0, :, :2] + 1.5     # nearly the same figure
    style = PoseStyle(17, kpt_thr=0.0)
    a, _ = _check_nv12(50, 70, 96, kpts, bboxes, style)
    b, _ = _check_nv12(50, 70, 96, kpts[::-1].copy(), bboxes[::-1].copy(), style)
    assert not torch.equal(a, b)


def test_thresholds_and_skipped_poses():
    """score == score_thr is not drawn; a key point at or below kpt_thr hides itself and its limbs; NaN / inf
    coordinates and a NaN score skip the pose; keep masks poses."""
    from pavenet_amd.render import PoseStyle
    kpts, bboxes = _poses(8, 17, 70, 50, seed=3, spread=0.5)
    kpts[..., 2] = 0.9
    bboxes[0, 4] = np.float32(0.3)            # equal to the threshold
    kpts[1, 5, 2], kpts[1, 6, 2] = 0.5, 0.4   # at and below kpt_thr
    kpts[2, 3, 0] = np.nan
    kpts[3, 16, 1] = np.inf
    bboxes[4, 4] = np.nan
    bboxes[5, 2] = -np.inf                    # a box coordinate, boxes not drawn
    keep = [1, 1, 1, 1, 1, 1, 0, 1]
    style = PoseStyle(17, score_thr=0.3, kpt_thr=0.5)
    prims = RR.primitives(kpts, bboxes, keep, (1.0, 1.0), style)
    per_pose = 4 + len(style.edges) + 17
    assert {pid // per_pose for pid, *_ in prims} == {1, 7}
    kinds = {(kind, i) for pid, _, _, _, (kind, i) in prims if pid // per_pose == 1}
    assert ('kpt', 5) not in kinds and ('kpt', 6) not in kinds and ('kpt', 7) in kinds
    assert not any(kind == 'limb' and {5, 6} & set(style.edges[i]) for kind, i in kinds)
    got, before = _check_nv12(50, 70, 96, kpts, bboxes, style, keep=keep)
    assert (got != before).any()
    # without keep pose 6 is drawn as well
    got2, _ = _check_nv12(50, 70, 96, kpts, bboxes, style)
    assert not torch.equal(got, got2)


@pytest.mark.parametrize('thickness,radius,boxes', [(1, 1, False), (32, 32, True), (4, 0, True), (3, 5, False)])
def test_edges_of_the_rule(thickness, radius, boxes):
    """A zero-length limb, key points on the corners (0, 0) and (W - 1, H - 1), coordinates below 0 and beyond the
    surface (clamped), the smallest and largest thickness / radius, radius 0 and boxes."""
    from pavenet_amd.render import PoseStyle
    W, H = 70, 50
    kpts, bboxes = _poses(3, 17, W, H, seed=4)
    kpts[..., 2] = 0.9
    kpts[0, 5, :2] = kpts[0, 7, :2]                     # limb (5, 7) has no length
    kpts[0, 0, :2], kpts[0, 16, :2] = (0.0, 0.0), (W - 1, H - 1)
    kpts[1, 9, :2], kpts[1, 10, :2] = (-7.3, 12.0), (W + 40.0, -3.0)
    kpts[2, 15, :2], kpts[2, 14, :2] = (20.0, H + 9000.0), (1e9, 1e9)
    bboxes[1, :4] = (-5.0, -5.0, W + 5.0, H + 5.0)
    style = PoseStyle(17, thickness=thickness, radius=radius, draw_boxes=boxes)
    got, before = _check_nv12(H, W, 96, kpts, bboxes, style)
    assert (got != before).any()


def test_scale_factor_divides_before_the_quantisation():
    """(0.694, 0.6944): rint((x / s) * 4) in fp32, the division first."""
    from pavenet_amd.render import PoseStyle
    scale = (0.694, 0.6944)
    kpts, bboxes = _poses(3, 17, 70, 50, seed=5)
    kpts[..., 0] *= scale[0]
    kpts[..., 1] *= scale[1]
    bboxes[:, [0, 2]] *= scale[0]
    bboxes[:, [1, 3]] *= scale[1]
    # pose 0's x coordinates sit on rounding ties of (x / s) * 4, where another order of the operations (x * (4 / s),
    # a reciprocal, a fused multiply) lands on the other side
    s32 = np.float32(scale[0])
    ties = (np.arange(8, 4 * 69, dtype=np.float32) + np.float32(0.5)) * np.float32(0.25) * s32
    cand = np.concatenate([np.nextafter(ties, np.float32(0)), ties, np.nextafter(ties, np.float32(1e9))])
    moved = cand[RR.quantise(cand, s32) != np.rint(cand * (np.float32(4.0) / s32)).astype(np.int64)]
    print(f'{len(moved)} of {len(cand)} candidates are quantised differently by x * (4 / s)')
    assert len(moved) >= 17
    kpts[0, :, 0] = moved[np.linspace(0, len(moved) - 1, 17).astype(int)]
    _check_nv12(50, 70, 96, kpts, bboxes, PoseStyle(17, draw_boxes=True), scale=scale)


def test_many_primitives_in_one_tile():
    """100 poses x 17 key points packed into the first tile of a 64 x 64 surface: 3 900 primitives on one tile, more
    than the 256-entry candidate list holds at once."""
    from pavenet_amd.render import PoseStyle
    rng = np.random.default_rng(6)
    kpts = np.empty((100, 17, 3), np.float32)
    kpts[..., :2] = rng.uniform(2, 29, (100, 17, 2))
    kpts[..., 2] = 0.9
    bboxes = np.concatenate([kpts[..., :2].min(1), kpts[..., :2].max(1), np.full((100, 1), 0.9)], 1).astype(np.float32)
    style = PoseStyle(17, thickness=1, radius=1, draw_boxes=True)
    assert len(RR.primitives(kpts, bboxes, None, (1.0, 1.0), style)) == 100 * (4 + 18 + 17)
    got, before = _check_nv12(64, 64, 64, kpts, bboxes, style)
    assert torch.equal(got[32:64, :], before[32:64, :]) and torch.equal(got[:32, 36:], before[:32, 36:])


def test_no_poses_leaves_the_surface_unchanged():
    from pavenet_amd.render import PoseStyle
    got, before = _check_nv12(50, 70, 96, np.zeros((0, 17, 3), np.float32), np.zeros((0, 5), np.float32), PoseStyle(17))
    assert torch.equal(got, before)
    kpts, bboxes = _poses(3, 17, 70, 50, seed=1)
    got, before = _check_nv12(50, 70, 96, kpts, bboxes, PoseStyle(17), keep=[0, 0, 0])
    assert torch.equal(got, before)


@pytest.mark.parametrize('K', [14, 15, 5, 32])
def test_skeleton_variants(K):
    """The built-in skeletons of K = 14 and 15, a small custom skeleton and the largest one (K = 32, 32 edges)."""
    from pavenet_amd.render import PoseStyle
    skeleton = None
    if K == 5:
        skeleton = ([(0, 1), (1, 2), (2, 3), (3, 4), (4, 0)], [(10 + 40 * e, 200 - 30 * e, 90) for e in range(5)],
                    [(250 - 20 * k, 15 * k, 128 + k) for k in range(5)])
    if K == 32:
        skeleton = ([(e, (e * 7 + 3) % 32) for e in range(32)], [(e * 8, 255 - e * 8, (e * 37) % 256) for e in range(32)],
                    [(255 - k * 8, (k * 53) % 256, k * 8) for k in range(32)])
    kpts, bboxes = _poses(3, K, 70, 50, seed=7 + K)
    _check_nv12(50, 70, 80, kpts, bboxes, PoseStyle(K, thickness=2, radius=3, skeleton=skeleton, draw_boxes=True),
                matrix='bt709')


def test_33_surfaces_take_two_launches():
    """33 surfaces of different sizes, pitches, matrices, ranges, scales and N in one call: each equals its own
    single-surface call (and the first and last the oracle)."""
    from pavenet_amd.render import PoseStyle, draw_poses_nv12
    style = PoseStyle(17, draw_boxes=True)
    specs = []
    for i in range(33):
        W, H = 34 + 2 * (i % 7) * 6, 20 + 2 * (i % 5) * 7
        specs.append(dict(W=W, H=H, pitch=W + (i % 3) * 5, matrix=('bt601', 'bt709')[i % 2], full_range=bool(i % 4 >= 2),
                          scale=(1.0 + 0.01 * i, 1.0 + 0.02 * (i % 3)), n=i % 4))
    befores = [_surface(s['H'], s['W'], s['pitch'], seed=100 + i) for i, s in enumerate(specs)]
    poses = [_poses(s['n'], 17, s['W'], s['H'], seed=200 + i) for i, s in enumerate(specs)]
    results = [_dev(k, b) for k, b in poses]
    together = [b.cuda() for b in befores]
    out = draw_poses_nv12(together, [s['W'] for s in specs], results, scale_factor=[s['scale'] for s in specs],
                          style=style, matrix=[s['matrix'] for s in specs], full_range=[s['full_range'] for s in specs])
    assert out is together
    for i, s in enumerate(specs):
        alone = befores[i].cuda()
        draw_poses_nv12(alone, s['W'], results[i], scale_factor=s['scale'], style=style, matrix=s['matrix'],
                        full_range=s['full_range'])
        assert torch.equal(together[i], alone), i
        assert s['n'] == 0 or not torch.equal(alone.cpu(), befores[i]), i
    for i in (1, 32):
        s = specs[i]
        want = RR.draw_nv12(befores[i].numpy(), s['W'], poses[i][0], poses[i][1], None, s['scale'], style, s['matrix'],
                            s['full_range'])
        assert torch.equal(together[i].cpu(), torch.from_numpy(want)), i


def test_bgr():
    """draw_poses_bgr on [50, 70, 3] (odd tile remainders in both directions), with boxes and a scale."""
    from pavenet_amd.render import PoseStyle, draw_poses_bgr
    g = torch.Generator().manual_seed(8)
    before = torch.randint(0, 256, (50, 70, 3), dtype=torch.uint8, generator=g)
    kpts, bboxes = _poses(3, 17, 70, 50, seed=8)
    style = PoseStyle(17, draw_boxes=True)
    for scale in (None, (0.694, 0.6944)):
        dev = before.cuda()
        assert draw_poses_bgr(dev, _dev(kpts, bboxes), scale_factor=scale, style=style) is dev
        want = RR.draw_bgr(before.numpy(), kpts, bboxes, None, scale or (1.0, 1.0), style)
        assert torch.equal(dev.cpu(), torch.from_numpy(want))
        assert (dev.cpu() != before).any()
    # an odd size: 2 x 2 blocks that hang over the right and bottom borders
    before = torch.randint(0, 256, (37, 45, 3), dtype=torch.uint8, generator=g)
    kpts, bboxes = _poses(2, 17, 45, 37, seed=9)
    kpts[0, 0, :2] = (44.0, 36.0)
    dev = before.cuda()
    draw_poses_bgr([dev], [_dev(kpts, bboxes)], style=style)
    assert torch.equal(dev.cpu(), torch.from_numpy(RR.draw_bgr(before.numpy(), kpts, bboxes, None, (1.0, 1.0), style)))


@functools.lru_cache(maxsize=None)
def _model():
    from tests.test_live_gpu import _model as live_model
    return live_model(3)


def test_show_result():
    """show_result == draw_poses_bgr with boxes on a copy; the input is unchanged; host and device inputs agree."""
    from pavenet_amd.render import PoseStyle, draw_poses_bgr
    m = _model()
    K = m.bbox_head.num_keypoints
    g = torch.Generator().manual_seed(10)
    img = torch.randint(0, 256, (50, 70, 3), dtype=torch.uint8, generator=g)
    kpts, bboxes = _poses(3, K, 70, 50, seed=10)
    bboxes[2, 4] = 0.2        # below the default score_thr
    result = ([bboxes], [kpts])                        # one image's entry of simple_test: per-class lists
    dev = img.cuda()
    out = m.show_result(dev, result, thickness=3)
    assert out.is_cuda and out.data_ptr() != dev.data_ptr() and torch.equal(dev.cpu(), img)
    want = draw_poses_bgr(img.cuda(), _dev(kpts, bboxes), style=PoseStyle(K, thickness=3, draw_boxes=True))
    assert torch.equal(out, want) and (out.cpu() != img).any()
    oracle = RR.draw_bgr(img.numpy(), kpts, bboxes, None, (1.0, 1.0), PoseStyle(K, thickness=3, draw_boxes=True))
    assert torch.equal(out.cpu(), torch.from_numpy(oracle))
    assert torch.equal(m.show_result(img.numpy(), [result], thickness=3), out)
    on_dev = _dev(kpts, bboxes)
    assert torch.equal(m.show_result(dev, on_dev, thickness=3), out)
    assert torch.equal(m.show_result(dev, (on_dev['bboxes'], None, on_dev['kpts']), thickness=3), out)
    with pytest.raises(NotImplementedError):
        m.show_result(dev, result, show=True)


def test_live_results_drawn_onto_their_surfaces():
    """Five NV12 frames through preprocess_surfaces_nv12 into LiveVideoPose (T = 3: frame c's result arrives with
    frame c + 1), each result drawn onto its kept surface with score_thr = -1: the oracle on the downloaded results."""
    from pavenet_amd.live import LiveVideoPose
    from pavenet_amd.preprocess import preprocess_surfaces_nv12
    from pavenet_amd.render import PoseStyle, draw_poses_nv12
    m = _model()
    befores = [_surface(96, 120, 128, seed=300 + i) for i in range(5)]
    surfaces = [b.cuda() for b in befores]
    img, meta = preprocess_surfaces_nv12(surfaces, 120, img_scale=(160, 128), size_divisor=32)
    assert img.shape == (5, 3, 128, 160)
    live = LiveVideoPose(m, meta, max_push=1)
    style = PoseStyle(m.bbox_head.num_keypoints, score_thr=-1.0, draw_boxes=True)
    got = []
    for i in range(5):
        got += live.push(img[i])
    got += live.flush()
    assert [c for c, _ in got] == [0, 1, 2, 3, 4]
    changed = 0
    for c, res in got:
        draw_poses_nv12(surfaces[c], 120, res, scale_factor=meta['scale_factor'], style=style)
        bboxes, _, kpts = (t.cpu().numpy() for t in res)
        want = RR.draw_nv12(befores[c].numpy(), 120, kpts, bboxes, None, meta['scale_factor'][:2], style)
        assert torch.equal(surfaces[c].cpu(), torch.from_numpy(want)), c
        changed += int((surfaces[c].cpu() != befores[c]).sum())
    assert changed > 0
