"""People hidden in NV12 and BGR frames on the device (pave_anon.hip) against the numpy statement of DESIGN section 15
(tests/anon_ref.py): torch.equal of the WHOLE allocation -- the picture is pre-filled with noise and the pitch padding
with a sentinel, so a byte written outside a masked cell fails the test too.  Needs an MI355X."""
import functools

import numpy as np
import pytest
import torch

from tests import anon_ref as AR
from tests import render_ref as RR

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5
CELLS = (2, 4, 8, 16, 32, 64)
MODES = (('bt601', False), ('bt601', True), ('bt709', False), ('bt709', True))


@pytest.fixture(autouse=True)
def _split_gemm_mode():
    """The live test's model runs under set_batch_invariant, which needs the library's default GEMM mode, whatever
    mode an earlier module left behind."""
    from pavenet_amd import bricks
    old = bricks.get_gemm_mode()
    bricks.set_gemm_mode('bf16x3')
    yield
    bricks.set_gemm_mode(old)


def _style(K=17, **kw):
    from pavenet_amd.anonymize import PrivacyStyle
    return PrivacyStyle(K, **kw)


def _surface(H, W, pitch, seed=0):
    """[H * 3 // 2, pitch] uint8 on the host: noise in the picture's columns, SENTINEL in the pitch padding."""
    g = torch.Generator().manual_seed(seed)
    s = torch.full((H * 3 // 2, pitch), SENTINEL, dtype=torch.uint8)
    s[:, :W] = torch.randint(0, 256, (H * 3 // 2, W), dtype=torch.uint8, generator=g)
    return s


def _figures(n, K, W, H, head=(0, 1, 2, 3, 4), seed=0, scale=(1.0, 1.0), score=0.9):
    """n seeded figures over a W x H picture, heads in its upper part, in the coordinates of the picture scaled by
    `scale` -> (kpts [n, K, 3], bboxes [n, 5]) float32 numpy."""
    rng = np.random.default_rng(seed)
    kpts = np.empty((n, K, 3), np.float32)
    cx, cy = rng.uniform(0.15 * W, 0.85 * W, (n, 1)), rng.uniform(0.1 * H, 0.5 * H, (n, 1))
    size = rng.uniform(0.25, 0.6, (n, 1)) * H
    kpts[..., 0] = cx + rng.uniform(-0.25, 0.25, (n, K)) * size
    kpts[..., 1] = cy + rng.uniform(0.15, 1.0, (n, K)) * size
    for k in head:
        kpts[:, k, 0] = cx[:, 0] + rng.uniform(-0.08, 0.08, n) * size[:, 0]
        kpts[:, k, 1] = cy[:, 0] + rng.uniform(-0.08, 0.08, n) * size[:, 0]
    kpts[..., 0] = np.clip(kpts[..., 0], 0, W - 1) * scale[0]
    kpts[..., 1] = np.clip(kpts[..., 1], 0, H - 1) * scale[1]
    kpts[..., 2] = 0.9
    bboxes = np.stack([kpts[..., 0].min(1), kpts[..., 1].min(1), kpts[..., 0].max(1), kpts[..., 1].max(1),
                       np.full(n, score)], 1).astype(np.float32)
    return kpts, bboxes


def _dev(kpts, bboxes, keep=None):
    res = dict(bboxes=torch.from_numpy(bboxes).cuda(), kpts=torch.from_numpy(kpts).cuda())
    if keep is not None:
        res['keep'] = torch.from_numpy(np.asarray(keep, np.int32)).cuda()
    return res


def _same(got, want, what=''):
    diff = (got != want).nonzero()
    assert torch.equal(got, want), f'{what}: {len(diff)} bytes differ, first at {diff[:5].tolist()}'


def _check_nv12(before, W, kpts, bboxes, style, keep=None, scale=None, matrix='bt601', full_range=False, result=None):
    """One surface through anonymize_nv12 against the oracle, whole allocation -> the anonymised host tensor."""
    from pavenet_amd.anonymize import anonymize_nv12
    dev = before.cuda()
    out = anonymize_nv12(dev, W, _dev(kpts, bboxes, keep) if result is None else result, scale_factor=scale, style=style,
                         matrix=matrix, full_range=full_range)
    assert out is dev
    sc = (1.0, 1.0) if scale is None else scale
    want = torch.from_numpy(AR.anonymize_nv12(before.numpy(), W, kpts, bboxes, keep, sc, style, matrix, full_range))
    got = dev.cpu()
    _same(got, want, f'cell {style.cell} {style.region} {style.mode} {matrix} {full_range} {sc}')
    return got


@pytest.mark.parametrize('region', ['head', 'person'])
@pytest.mark.parametrize('cell', CELLS)
@pytest.mark.parametrize('W,H,pitch', [(70, 50, 96), (130, 70, 160)])
def test_nv12_cells_modes_regions(W, H, pitch, cell, region):
    """Regions across the tile borders at 64 and cells clipped at the right and bottom; 'pixelate' and 'fill' under
    the four (matrix, range) pairs, at scale (1, 1) and (0.694, 0.7)."""
    before = _surface(H, W, pitch, seed=W + cell)
    for scale in (None, (0.694, 0.7)):
        kpts, bboxes = _figures(3, 17, W, H, seed=3, scale=scale or (1.0, 1.0))
        kpts[0, :5, 0], kpts[0, :5, 1] = 63.0 * (scale or (1, 1))[0], 20.0 * (scale or (1, 1))[1]   # a head on x = 64
        kpts[1, :5, 0], kpts[1, :5, 1] = (W - 2.0) * (scale or (1, 1))[0], (H - 2.0) * (scale or (1, 1))[1]   # the corner
        bboxes[:, :2], bboxes[:, 2:4] = kpts[..., :2].min(1), kpts[..., :2].max(1)
        style = _style(cell=cell, region=region)
        pix = AR.pixel_mask(W, H, cell, AR.regions(kpts, bboxes, None, scale or (1.0, 1.0), style))
        assert pix[:, :64].any() and pix[:, 64:].any() and pix[H - 1, W - 1]
        got = _check_nv12(before, W, kpts, bboxes, style, scale=scale)
        assert (got != before).any() and torch.equal(got[:, W:], before[:, W:])
        for matrix, full_range in MODES:
            fill = _style(cell=cell, region=region, mode='fill', fill_color=(200, 30, 90))
            _check_nv12(before, W, kpts, bboxes, fill, scale=scale, matrix=matrix, full_range=full_range)


@pytest.mark.parametrize('cell', CELLS)
def test_bgr_odd_sizes_and_an_odd_base(cell):
    """[49, 71, 3] BGR: odd sizes, and the same picture as a view that starts at an odd byte of its allocation, where
    only the byte path can run; the bytes around the view keep their sentinel."""
    from pavenet_amd.anonymize import anonymize_bgr
    g = torch.Generator().manual_seed(40 + cell)
    before = torch.randint(0, 256, (49, 71, 3), dtype=torch.uint8, generator=g)
    kpts, bboxes = _figures(3, 17, 71, 49, seed=5)
    kpts[0, :5, :2] = (69.0, 47.0)
    for region, mode, scale in (('head', 'pixelate', None), ('person', 'pixelate', (0.694, 0.7)), ('head', 'fill', None)):
        style = _style(cell=cell, region=region, mode=mode, fill_color=(9, 200, 77))
        want = torch.from_numpy(AR.anonymize_bgr(before.numpy(), kpts, bboxes, None, scale or (1.0, 1.0), style))
        assert (want != before).any()
        dev = before.cuda()
        assert dev.data_ptr() % 4 == 0
        assert anonymize_bgr(dev, _dev(kpts, bboxes), scale_factor=scale, style=style) is dev
        _same(dev.cpu(), want, f'{region} {mode} aligned')
        for offset in (1, 2, 3):
            buf = torch.full((offset + before.numel() + 5,), SENTINEL, dtype=torch.uint8).cuda()
            view = buf[offset:offset + before.numel()].view(49, 71, 3)
            view.copy_(before.cuda())
            assert view.data_ptr() % 4 == offset and view.is_contiguous()
            anonymize_bgr([view], [_dev(kpts, bboxes)], scale_factor=scale, style=style)
            _same(view.cpu(), want, f'{region} {mode} offset {offset}')
            assert (buf[:offset] == SENTINEL).all() and (buf[offset + before.numel():] == SENTINEL).all()


def test_nv12_pitch_and_base_off_the_word():
    """An NV12 surface whose pitch is not a multiple of 4 (pitch 75) and one at an odd base: the byte path on NV12."""
    from pavenet_amd.anonymize import anonymize_nv12
    kpts, bboxes = _figures(3, 17, 70, 50, seed=6)
    for cell in (4, 16):
        style = _style(cell=cell, region='person')
        _check_nv12(_surface(50, 70, 75, seed=7), 70, kpts, bboxes, style)
        before = _surface(50, 70, 96, seed=8)
        buf = torch.full((1 + before.numel() + 3,), SENTINEL, dtype=torch.uint8).cuda()
        view = buf[1:1 + before.numel()].view(75, 96)
        view.copy_(before.cuda())
        anonymize_nv12(view, 70, _dev(kpts, bboxes), style=style)
        want = AR.anonymize_nv12(before.numpy(), 70, kpts, bboxes, None, (1.0, 1.0), style)
        _same(view.cpu(), torch.from_numpy(want), f'cell {cell} odd base')
        assert buf[0] == SENTINEL and (buf[1 + before.numel():] == SENTINEL).all()


def test_thresholds_and_skipped_poses():
    """keep = 0, a score at the threshold, NaN and inf coordinates and scores: no region; a key point at kpt_thr is
    invisible."""
    W, H = 70, 50
    kpts, bboxes = _figures(9, 17, W, H, seed=9)
    bboxes[0, 4] = np.float32(0.3)            # equal to the threshold
    kpts[1, 0, 2], kpts[1, 1, 2] = 0.5, 0.4   # at and below kpt_thr: the head's rectangle is of key points 2, 3, 4
    kpts[2, 9, 0] = np.nan                    # a body key point
    kpts[3, 16, 1] = np.inf
    bboxes[4, 4] = np.nan
    bboxes[5, 2] = -np.inf
    bboxes[7, 4] = np.inf                     # an infinite score is above the threshold
    keep = [1, 1, 1, 1, 1, 1, 0, 1, 1]
    before = _surface(H, W, 96, seed=9)
    for region in ('head', 'person'):
        style = _style(cell=4, region=region, score_thr=0.3, kpt_thr=0.5)
        assert len(AR.regions(kpts, bboxes, keep, (1.0, 1.0), style)) == 3      # poses 1, 7, 8
        got = _check_nv12(before, W, kpts, bboxes, style, keep=keep)
        got2 = _check_nv12(before, W, kpts, bboxes, style)                       # without keep pose 6 counts as well
        assert not torch.equal(got, got2)
    one = _style(cell=4, kpt_thr=0.5)
    a = AR.regions(kpts[1:2], bboxes[1:2], None, (1.0, 1.0), one)
    kpts[1, 0, 2] = 0.51
    assert AR.regions(kpts[1:2], bboxes[1:2], None, (1.0, 1.0), one) != a


def test_invisible_heads_fall_back_or_are_skipped():
    W, H = 70, 50
    kpts, bboxes = _figures(3, 17, W, H, seed=10)
    kpts[0, :5, 2] = 0.0
    kpts[2, :5, 2] = 0.0
    before = _surface(H, W, 96, seed=10)
    person = _check_nv12(before, W, kpts, bboxes, _style(cell=8, fallback='person'))
    skip = _check_nv12(before, W, kpts, bboxes, _style(cell=8, fallback='skip'))
    assert not torch.equal(person, skip) and (skip != before).any()
    kpts[1, :5, 2] = 0.0
    assert torch.equal(_check_nv12(before, W, kpts, bboxes, _style(cell=8, fallback='skip')), before)


def test_edges_of_the_rule():
    """Swapped box corners, coordinates clamped at 0 and 32767, a region larger than the picture, and r = 0."""
    W, H = 70, 50
    before = _surface(H, W, 96, seed=11)
    kpts, bboxes = _figures(3, 17, W, H, seed=11)
    bboxes[0, :4] = bboxes[0, [2, 3, 0, 1]]                       # (x2, y2, x1, y1)
    bboxes[1, :4] = (-9.0, -4.0, 30.0, 1e9)                       # clamped at 0 and at 32767
    kpts[2, 0, :2] = (-3.0, 1e9)
    for cell in (2, 16):
        for region in ('head', 'person'):
            got = _check_nv12(before, W, kpts, bboxes, _style(cell=cell, region=region))
            assert (got != before).any()
    # margin 64 with grow 32: every cell of the picture
    big = _style(cell=16, region='person', margin=64, grow=32)
    assert AR.cell_mask(W, H, 16, AR.regions(kpts, bboxes, None, (1.0, 1.0), big)).all()
    _check_nv12(before, W, kpts, bboxes, big)
    _check_nv12(before, W, kpts, bboxes, _style(cell=64, margin=64, head_scale=32, head_min=32, mode='fill'))
    # r = 0 with one visible key point: exactly the cells holding that point
    kpts[:, :5, 2] = 0.0
    kpts[:, 0, 2] = 0.9
    kpts[0, 0, :2], kpts[1, 0, :2], kpts[2, 0, :2] = (16.0, 16.0), (63.0, 27.25), (69.0, 49.0)
    for cell in (4, 16):
        style = _style(cell=cell, head_scale=0, head_min=0)
        mask = AR.cell_mask(W, H, cell, AR.regions(kpts, bboxes, None, (1.0, 1.0), style))
        # (16, 16) is the first point of a cell and the last of none; (63, 27.25) is in the last column of a tile and,
        # at cell 4, a quarter pixel below the last row of a cell, in the gap between two cells: the rule masks neither
        assert mask[16 // cell, 16 // cell] and not mask[16 // cell - 1, 16 // cell - 1]
        assert mask[27 // cell, 63 // cell] == (cell == 16) and not mask[27 // cell, 64 // cell]
        assert mask[49 // cell, 69 // cell] and mask.sum() == 2 + (cell == 16)
        _check_nv12(before, W, kpts, bboxes, style)


def test_no_poses_leaves_the_surface_unchanged():
    before = _surface(50, 70, 96, seed=12)
    got = _check_nv12(before, 70, np.zeros((0, 17, 3), np.float32), np.zeros((0, 5), np.float32), _style())
    assert torch.equal(got, before)
    kpts, bboxes = _figures(3, 17, 70, 50, seed=12)
    assert torch.equal(_check_nv12(before, 70, kpts, bboxes, _style(), keep=[0, 0, 0]), before)


@pytest.mark.parametrize('cell', [2, 16])
def test_4096_poses_on_one_tile(cell):
    """4096 poses piled on one 64 x 64 picture: sixteen rounds of the 256-entry region list."""
    rng = np.random.default_rng(13)
    kpts = np.empty((4096, 17, 3), np.float32)
    kpts[..., :2] = rng.uniform(0, 64, (4096, 1, 2)) + rng.uniform(-1.5, 1.5, (4096, 17, 2))
    kpts[..., 2] = 0.9
    bboxes = np.concatenate([kpts[..., :2].min(1), kpts[..., :2].max(1), np.full((4096, 1), 0.9)], 1).astype(np.float32)
    keep = (np.arange(4096) % 64 == 63).astype(np.int32)      # 64 poses count, one in the last lanes of every round
    before = _surface(64, 64, 64, seed=13)
    style = _style(cell=cell, head_min=0, head_scale=4)
    mask = AR.cell_mask(64, 64, cell, AR.regions(kpts, bboxes, keep, (1.0, 1.0), style))
    assert mask.any() and (cell == 16 or not mask.all())
    _check_nv12(before, 64, kpts, bboxes, style, keep=keep)
    got = _check_nv12(before, 64, kpts, bboxes, _style(cell=cell, region='person'))
    assert (got != before).any()


@pytest.mark.parametrize('K,head', [(14, None), (14, [13]), (17, [0]), (17, [3, 4, 1, 2, 0, 5, 6, 16]), (32, [31, 7, 19])])
def test_head_indices(K, head):
    kpts, bboxes = _figures(3, K, 70, 50, head=head or (12, 13), seed=14 + K)
    before = _surface(50, 70, 80, seed=14)
    style = _style(K, cell=8, head=head)
    got = _check_nv12(before, 70, kpts, bboxes, style, matrix='bt709')
    assert (got != before).any()


def test_33_surfaces_take_two_launches():
    """33 surfaces of different sizes, pitches, matrices, ranges, scales and N in one call: each equals the oracle, and
    a surface without poses keeps every byte."""
    from pavenet_amd.anonymize import anonymize_nv12
    style = _style(cell=8, mode='fill', fill_color=(10, 120, 250))
    specs = []
    for i in range(33):
        W, H = 34 + 2 * (i % 7) * 6, 20 + 2 * (i % 5) * 7
        specs.append(dict(W=W, H=H, pitch=W + (i % 3) * 5, matrix=('bt601', 'bt709')[i % 2], full_range=bool(i % 4 >= 2),
                          scale=(1.0 + 0.01 * i, 1.0 + 0.02 * (i % 3)), n=i % 4))
    befores = [_surface(s['H'], s['W'], s['pitch'], seed=100 + i) for i, s in enumerate(specs)]
    poses = [_figures(s['n'], 17, s['W'], s['H'], seed=200 + i, scale=s['scale']) for i, s in enumerate(specs)]
    together = [b.cuda() for b in befores]
    out = anonymize_nv12(together, [s['W'] for s in specs], [_dev(k, b) for k, b in poses],
                         scale_factor=[s['scale'] for s in specs], style=style, matrix=[s['matrix'] for s in specs],
                         full_range=[s['full_range'] for s in specs])
    assert out is together
    for i, s in enumerate(specs):
        want = AR.anonymize_nv12(befores[i].numpy(), s['W'], poses[i][0], poses[i][1], None, s['scale'], style,
                                 s['matrix'], s['full_range'])
        _same(together[i].cpu(), torch.from_numpy(want), f'surface {i}')
        assert (s['n'] == 0) == torch.equal(together[i].cpu(), befores[i]), i
    # pixelate as well, the second launch's surface included
    style = _style(cell=4, region='person')
    together = [b.cuda() for b in befores]
    anonymize_nv12(together, [s['W'] for s in specs], [_dev(k, b) for k, b in poses],
                   scale_factor=[s['scale'] for s in specs], style=style)
    for i in (1, 31, 32):
        s = specs[i]
        want = AR.anonymize_nv12(befores[i].numpy(), s['W'], poses[i][0], poses[i][1], None, s['scale'], style)
        _same(together[i].cpu(), torch.from_numpy(want), f'surface {i}')


def test_both_result_forms_and_twice_equals_once():
    from pavenet_amd.anonymize import anonymize_nv12
    W, H = 130, 70
    kpts, bboxes = _figures(4, 17, W, H, seed=15)
    before = _surface(H, W, 160, seed=15)
    for style in (_style(cell=8), _style(cell=16, region='person')):
        on_dev = _dev(kpts, bboxes, keep=[1, 0, 1, 1])
        as_dict = _check_nv12(before, W, kpts, bboxes, style, keep=[1, 0, 1, 1], result=on_dev)
        batched = dict(bboxes=on_dev['bboxes'][None], kpts=on_dev['kpts'][None], keep=on_dev['keep'][None])
        assert torch.equal(_check_nv12(before, W, kpts, bboxes, style, keep=[1, 0, 1, 1], result=batched), as_dict)
        sel = [0, 2, 3]
        as_tuple = _check_nv12(before, W, kpts[sel], bboxes[sel], style,
                               result=(on_dev['bboxes'][sel], None, on_dev['kpts'][sel]))
        assert torch.equal(as_tuple, as_dict)
        dev = before.cuda()
        anonymize_nv12(dev, W, on_dev, style=style)
        anonymize_nv12(dev, W, on_dev, style=style)
        assert torch.equal(dev.cpu(), as_dict)


def test_anonymise_then_draw():
    """The usual order: the skeleton over the pixelated person equals the two oracles applied in that order."""
    from pavenet_amd.anonymize import anonymize_nv12
    from pavenet_amd.render import PoseStyle, draw_poses_nv12
    W, H = 130, 70
    kpts, bboxes = _figures(3, 17, W, H, seed=16)
    before = _surface(H, W, 160, seed=16)
    privacy, pose = _style(cell=8, region='person'), PoseStyle(17, thickness=2, radius=2)
    dev = before.cuda()
    res = _dev(kpts, bboxes)
    draw_poses_nv12(anonymize_nv12(dev, W, res, style=privacy, matrix='bt709'), W, res, style=pose, matrix='bt709')
    hidden = AR.anonymize_nv12(before.numpy(), W, kpts, bboxes, None, (1.0, 1.0), privacy, 'bt709', False)
    want = RR.draw_nv12(hidden, W, kpts, bboxes, None, (1.0, 1.0), pose, 'bt709', False)
    assert (want != hidden).any() and (hidden != before.numpy()).any()
    _same(dev.cpu(), torch.from_numpy(want), 'anonymise then draw')


def test_allocator_peak_is_unchanged_by_a_second_call():
    from pavenet_amd.anonymize import anonymize_bgr, anonymize_nv12
    kpts, bboxes = _figures(3, 17, 130, 70, seed=17)
    res = _dev(kpts, bboxes, keep=[1, 1, 1])
    surfaces = [_surface(70, 130, 160, seed=17 + i).cuda() for i in range(3)]
    img = torch.zeros(70, 130, 3, dtype=torch.uint8).cuda()
    for call in (lambda: anonymize_nv12(surfaces, 130, [res] * 3, style=_style(cell=16)),
                 lambda: anonymize_bgr(img, res, style=_style(cell=16, region='person'))):
        call()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        now, peak = torch.cuda.memory_allocated(), torch.cuda.max_memory_allocated()
        call()
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated() == now and torch.cuda.max_memory_allocated() == peak


@functools.lru_cache(maxsize=None)
def _model():
    from tests.test_live_gpu import _model as live_model
    return live_model(3)


def test_live_results_hidden_on_their_surfaces():
    """Five NV12 frames through preprocess_surfaces_nv12 into LiveVideoPose (T = 3: frame c's result arrives with
    frame c + 1), each result anonymised on its kept surface with score_thr = -1: the oracle on the downloaded
    results."""
    from pavenet_amd.anonymize import HEAD_KEYPOINTS, anonymize_nv12
    from pavenet_amd.live import LiveVideoPose
    from pavenet_amd.preprocess import preprocess_surfaces_nv12
    m = _model()
    K = m.bbox_head.num_keypoints
    befores = [_surface(96, 120, 128, seed=300 + i) for i in range(5)]
    surfaces = [b.cuda() for b in befores]
    img, meta = preprocess_surfaces_nv12(surfaces, 120, img_scale=(160, 128), size_divisor=32)
    assert img.shape == (5, 3, 128, 160)
    live = LiveVideoPose(m, meta, max_push=1)
    style = _style(K, cell=8, score_thr=-1.0, kpt_thr=-1.0, head=None if K in HEAD_KEYPOINTS else [0])
    got = []
    for i in range(5):
        got += live.push(img[i])
    got += live.flush()
    assert [c for c, _ in got] == [0, 1, 2, 3, 4]
    changed = 0
    for c, res in got:
        anonymize_nv12(surfaces[c], 120, res, scale_factor=meta['scale_factor'], style=style)
        bboxes, _, kpts = (t.cpu().numpy() for t in res)
        want = AR.anonymize_nv12(befores[c].numpy(), 120, kpts, bboxes, None, meta['scale_factor'][:2], style)
        _same(surfaces[c].cpu(), torch.from_numpy(want), f'frame {c}')
        changed += int((surfaces[c].cpu() != befores[c]).sum())
    assert changed > 0
