"""Test-time augmentation on the MI355X: the merge kernel against the host restatement, the input flips, PETR's
aug_test against the reference's own recorded run, the four-augmentation composition, forward's dispatch and the
strict mode."""
import json
import os

import numpy as np
import pytest
import torch

from oracle.seeded import seeded_array, seeded_state_dict
from tests import aug_ref

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
FLIP_CFG = json.load(open(os.path.join(GOLDEN, 'aug_flip_test_config.json')))


def _assert_same_selection(values, ref_idx, tol, what):
    """(as tests/test_model_gpu.py) `ref_idx` is a valid top-k of `values` up to near-ties at the boundary."""
    values = values.flatten().float().cpu()
    ref_idx = torch.as_tensor(np.asarray(ref_idx)).flatten().long()
    top_v, top_i = values.topk(ref_idx.numel())
    kth = top_v[-1]
    worst = values[ref_idx].min()
    assert worst >= kth - tol, f'{what}: reference-selected member {float(worst)} vs k-th {float(kth)}'
    ref_set = set(ref_idx.tolist())
    for v, i in zip(top_v.tolist(), top_i.tolist()):
        if i not in ref_set:
            assert v <= float(kth) + tol, f'{what}: member {i} ({v}) is not a near-tie of the k-th value'


def _case(seed, A, B, N, K, low_scores=False):
    rng = np.random.default_rng(seed)
    bbs, kps, keeps, flips, ws, sfs = [], [], [], [], [], []
    for a in range(A):
        ctr = rng.uniform(0, 300, size=(B, 10, 2)).astype(np.float32)
        c = ctr[:, rng.integers(0, 10, size=N)] + rng.normal(0, 6, size=(B, N, 2)).astype(np.float32)
        wh = rng.uniform(10, 60, size=(B, N, 2)).astype(np.float32)
        sc = rng.uniform(1e-5, 1e-3, size=(B, N)) if low_scores else rng.uniform(0, 1, size=(B, N))
        sc = sc.astype(np.float32)
        if N > 1:
            sc[:, ::5] = sc[:, 1:2]                           # equal scores
        bb = np.concatenate([c, c + wh, sc[..., None]], -1).astype(np.float32)
        if N > 3:
            bb[:, 3] = bb[:, 2]                               # a duplicate box with an equal score
        kp = np.concatenate([rng.uniform(0, 320, size=(B, N, K, 2)), np.ones((B, N, K, 1))], -1).astype(np.float32)
        keep = (rng.uniform(size=(B, N)) > 0.2).astype(np.int32) if a == 1 else None
        bbs.append(bb)
        kps.append(kp)
        keeps.append(keep)
        flips.append(a % 2 == 1)
        ws.append([float(rng.integers(200, 330)) for _ in range(B)])
        s = [float(np.float32(rng.uniform(0.5, 2.0))) for _ in range(B)]
        sfs.append([[v, v * 1.25, v, v * 1.25] for v in s])
    return bbs, kps, keeps, flips, ws, sfs


def _host(bbs, kps, keeps, flips, ws, sfs, perm, b, score_thr, nms_cfg, max_num):
    aug, metas = [], []
    for a in range(len(bbs)):
        m = np.ones(bbs[a].shape[1], bool) if keeps[a] is None else keeps[a][b].astype(bool)
        aug.append((bbs[a][b][m], kps[a][b][m]))
        metas.append(dict(img_w=ws[a][b], scale_factor=sfs[a][b], flip=flips[a]))
    with np.errstate(invalid='ignore', divide='ignore'):
        return aug_ref.merge_aug(aug, metas, perm, score_thr, nms_cfg, max_num)


def _run(case, perm, score_thr, nms_cfg, max_num):
    from pavenet_amd import ops
    from pavenet_amd.tta import parse_nms_cfg
    bbs, kps, keeps, flips, ws, sfs = case
    method, iou, sigma, min_score, offset = parse_nms_cfg(nms_cfg)
    out = ops.aug_merge_nms([torch.from_numpy(x).cuda() for x in bbs], [torch.from_numpy(x).cuda() for x in kps],
                            [None if k is None else torch.from_numpy(k).cuda() for k in keeps], flips, ws, sfs,
                            perm, score_thr=score_thr, max_num=max_num, method=method, iou_thr=iou, sigma=sigma,
                            min_score=min_score, offset=offset)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _check(out, case, perm, score_thr, nms_cfg, max_num):
    B = case[0][0].shape[0]
    gauss = nms_cfg.get('method') == 'gaussian'
    for b in range(B):
        dets, labels, inds, kpts, _ = _host(*case, perm, b, score_thr, nms_cfg, max_num)
        n = int(out['count'][b])
        assert n == len(inds), f'image {b}: {n} rows vs the restatement\'s {len(inds)}'
        assert np.array_equal(out['inds'][b, :n], inds), f'image {b}: inds differ'
        assert (out['inds'][b, n:] == -1).all() and (out['keep'][b, :n] == 1).all() and (out['keep'][b, n:] == 0).all()
        assert not out['labels'][b].any()
        assert np.array_equal(out['dets'][b, :n, :4], dets[:, :4])
        if gauss:
            np.testing.assert_allclose(out['dets'][b, :n, 4], dets[:, 4], rtol=3e-7 * 4, atol=0)
        else:
            assert np.array_equal(out['dets'][b, :n, 4], dets[:, 4])
        assert np.array_equal(out['kpts'][b, :n], kpts)


CFGS = {'nms': dict(type='nms', iou_thr=0.5), 'naive': dict(type='soft_nms', iou_thr=0.3, method='naive'),
        'linear': dict(type='soft_nms', iou_thr=0.5), 'gaussian': dict(type='soft_nms', iou_thr=0.5,
                                                                         method='gaussian', sigma=0.5)}
SHAPES = {1: (1, 1), 7: (1, 7), 200: (2, 100), 600: (3, 200), 4096: (4, 1024)}


@pytest.mark.parametrize('n', sorted(SHAPES))
@pytest.mark.parametrize('method', sorted(CFGS))
@pytest.mark.parametrize('offset', [0, 1])
def test_merge_kernel_vs_restatement(n, method, offset):
    from pavenet_amd.keypoints import flip_permutation
    A, N = SHAPES[n]
    case = _case(n * 10 + offset, A, 3, N, 17)
    cfg = dict(CFGS[method], offset=offset)
    for max_num in ((100, -1) if n <= 600 else (100,)):
        _check(_run(case, flip_permutation(17), 0.05, cfg, max_num), case, flip_permutation(17), 0.05, cfg, max_num)


@pytest.mark.parametrize('method', sorted(CFGS))
def test_merge_kernel_edge_cases(method):
    from pavenet_amd.keypoints import flip_permutation
    perm = flip_permutation(14)
    cfg = CFGS[method]
    low = _case(5, 2, 3, 60, 14, low_scores=True)        # every score below min_score
    _check(_run(low, perm, 0.0, cfg, 100), low, perm, 0.0, cfg, 100)
    case = _case(6, 2, 3, 60, 14)
    out = _run(case, perm, 2.0, cfg, 100)                 # nothing passes score_thr: empty
    assert (out['count'] == 0).all() and (out['inds'] == -1).all() and (out['keep'] == 0).all()
    _check(_run(case, perm, 0.0, cfg, 5), case, perm, 0.0, cfg, 5)   # max_num truncation
    assert (_run(case, perm, 0.0, cfg, 5)['count'] <= 5).all()


def test_merge_kernel_rejects_what_it_cannot_hold():
    from pavenet_amd import ops
    from pavenet_amd.keypoints import flip_permutation
    bb = torch.zeros((1, 2049, 5), device='cuda')
    kp = torch.zeros((1, 2049, 17, 3), device='cuda')
    with pytest.raises(RuntimeError, match='4096'):
        ops.aug_merge_nms([bb, bb], [kp, kp], [None, None], [False, True], [[10.], [10.]], [[[1.] * 4]] * 2,
                          flip_permutation(17), score_thr=0.0, max_num=100, method='linear')


def test_flipped_preprocess_and_canvas_flip_are_bit_exact():
    from pavenet_amd.ops import hflip_canvas
    from pavenet_amd.preprocess import preprocess_clip
    frames = torch.from_numpy((seeded_array('aug.frames', (2, 57, 83, 3), 1.0) * 100 + 128).clip(0, 255)
                              .astype(np.uint8)).cuda()
    img, meta = preprocess_clip(frames, (160, 96), size_divisor=32)
    fimg, fmeta = preprocess_clip(frames, (160, 96), size_divisor=32, flip=True)
    Wn = meta['img_shape'][1]
    assert fmeta['flip'] is True and fmeta['flip_direction'] == 'horizontal' and Wn < img.shape[-1]
    exp = img.clone().cpu()
    exp[..., :Wn] = exp[..., :Wn].flip(-1)
    assert torch.equal(fimg.cpu(), exp)
    assert (fimg[..., Wn:] == 0).all()
    canv = img[0]                                          # [T, 3, Hp, Wp]
    got = hflip_canvas(canv, Wn)
    assert torch.equal(got.cpu(), exp[0])
    w = torch.tensor([Wn, Wn - 5], dtype=torch.int32, device='cuda')
    got = hflip_canvas(canv, w).cpu()
    c = canv.cpu()
    assert torch.equal(got[0, :, :, :Wn], c[0, :, :, :Wn].flip(-1))
    assert torch.equal(got[1, :, :, :Wn - 5], c[1, :, :, :Wn - 5].flip(-1))
    assert torch.equal(got[1, :, :, Wn - 5:], c[1, :, :, Wn - 5:])   # the columns from w on: untouched


def _petr(K, N, nms_cfg, keys=None):
    from pavenet_amd.models import build_model, petr_r50_cfg
    m = build_model(petr_r50_cfg(num_keypoints=K, max_per_img=N))
    shapes = json.loads(str(keys)) if keys is not None else {k: list(v.shape) for k, v in m.state_dict().items()}
    m.load_state_dict(seeded_state_dict(shapes, like=m.state_dict()), strict=True)
    m.test_cfg = dict(FLIP_CFG['test_cfg'], max_per_img=N, nms=nms_cfg)
    return m.cuda().eval()


def _metas(flip, hw=(120, 150), canvas=(128, 160), sf=1.0):
    return [dict(batch_input_shape=canvas, img_shape=hw + (3,), pad_shape=canvas + (3,), scale_factor=(sf,) * 4,
                 flip=flip, flip_direction='horizontal' if flip else None)]


@pytest.mark.parametrize('prefix', ['', 'nms_'])
def test_petr_aug_test_vs_reference_golden(prefix):
    g = np.load(os.path.join(GOLDEN, 'aug_petr_r50.npz'))
    nms_cfg = FLIP_CFG['test_cfg']['nms'] if not prefix else dict(type='nms', iou_thr=0.5)
    # the golden's NMS decisions are not knife-edge: no pair's overlap within 1e-4 of the threshold
    mb = g[prefix + 'merged_bboxes']
    for i in range(len(mb)):
        ovr = aug_ref._iou(mb[i], aug_ref._areas(mb[i:i + 1], 0)[0], mb, aug_ref._areas(mb, 0), 0)
        ovr = np.delete(ovr, i)
        assert (np.abs(ovr - 0.5) > 1e-4).all()
    m = _petr(17, 20, nms_cfg, g['keys'])
    img = torch.from_numpy(seeded_array('aug_petr_r50.img', (1, 3, 128, 160))).cuda()
    fimg = img.clone()
    fimg[..., :150] = img[..., :150].flip(-1)
    imgs, metas = [img, fimg], [_metas(False), _metas(True)]
    with torch.no_grad():
        for a in range(2):
            outs = m.bbox_head(m.extract_feat(imgs[a]), metas[a])
            _assert_same_selection(outs['enc_cls_scores'][0, :, 0], g[f'{prefix}enc_topk_{a}'], 1e-4, 'proposals')
            outs = m.bbox_head(m.extract_feat(imgs[a]), metas[a],
                               force_topk_proposals=torch.from_numpy(g[f'{prefix}enc_topk_{a}']).cuda())
            _assert_same_selection(outs['all_cls_scores'][-1][0].sigmoid(), g[f'{prefix}score_topk_{a}'], 1e-5,
                                   'score top-k')
        res = m.aug_test_device(imgs, metas,
                                force_topk_proposals=[torch.from_numpy(g[f'{prefix}enc_topk_{a}']).cuda()
                                                      for a in range(2)],
                                force_score_topk=[torch.from_numpy(g[f'{prefix}score_topk_{a}'])[None].cuda()
                                                  for a in range(2)])
        n = int(res['count'][0])
    assert res['inds'][0, :n].cpu().numpy().tolist() == g[prefix + 'det_inds'].tolist()
    np.testing.assert_allclose(res['kpts'][0, :n].cpu().numpy(), g[prefix + 'det_kpts'], rtol=1e-4, atol=1e-2)
    np.testing.assert_allclose(res['bboxes'][0, :n].cpu().numpy(), g[prefix + 'det_bboxes'], rtol=1e-4, atol=1e-2)


def _four_augs(K):
    from pavenet_amd.preprocess import multi_scale_flip_aug
    frames = torch.from_numpy((seeded_array('aug.four', (1, 120, 150, 3), 1.0) * 100 + 128).clip(0, 255)
                              .astype(np.uint8)).cuda()
    imgs, metas = multi_scale_flip_aug(frames, [(160, 128), (200, 160)], flip=True, size_divisor=32)
    return [i[:, 0] for i in imgs], metas


@pytest.mark.parametrize('K', [17, 14])
def test_two_scales_times_flip_equals_host_composition(K):
    from pavenet_amd.keypoints import flip_permutation
    m = _petr(K, 30, FLIP_CFG['test_cfg']['nms'])
    imgs, metas = _four_augs(K)
    assert [mm[0]['flip'] for mm in metas] == [False, True, False, True]
    with torch.no_grad():
        res = m.aug_test_device(imgs, metas)
        per = [m.bbox_head.results_to_list(m.forward_device(imgs[a], metas[a]))[0] for a in range(4)]
    aug = [(b.cpu().numpy(), k.cpu().numpy()) for b, _, k in per]
    hm = [dict(img_w=mm[0]['img_shape'][1], scale_factor=mm[0]['scale_factor'], flip=mm[0]['flip']) for mm in metas]
    with np.errstate(invalid='ignore', divide='ignore'):
        dets, _, inds, kpts, _ = aug_ref.merge_aug(aug, hm, flip_permutation(K), 0.0, FLIP_CFG['test_cfg']['nms'], 30)
    n = int(res['count'][0])
    assert res['inds'][0, :n].cpu().numpy().tolist() == inds.tolist()
    np.testing.assert_allclose(res['bboxes'][0, :n].cpu().numpy(), dets, rtol=1e-5, atol=1e-4)
    np.testing.assert_allclose(res['kpts'][0, :n].cpu().numpy(), kpts, rtol=1e-5, atol=1e-4)


def test_forward_with_two_augmentations_returns_the_merge():
    m = _petr(17, 20, FLIP_CFG['test_cfg']['nms'])
    imgs, metas = _four_augs(17)
    with torch.no_grad():
        got = m.forward(imgs[:2], metas[:2])
        exp = m.aug_test(imgs[:2], metas[:2])
        single = m.forward(imgs[:1], metas[:1])
    assert len(got) == 1
    np.testing.assert_array_equal(got[0][0][0], exp[0][0][0])
    np.testing.assert_array_equal(got[0][1][0], exp[0][1][0])
    assert (got[0][1][0][..., 2] == 1).all()             # the merge's key-point score channel
    assert got[0][0][0].shape != single[0][0][0].shape or not np.array_equal(got[0][0][0], single[0][0][0])


def test_strict_aug_test_has_no_fallback_and_a_launch_free_merge():
    m = _petr(17, 20, FLIP_CFG['test_cfg']['nms'])
    imgs, metas = _four_augs(17)
    with torch.no_grad():
        res = m.aug_test_device(imgs[:2], metas[:2], strict=True)
    c = m.last_merge_census
    assert not c.fallback_ops and not c.aten_launches and not c.host_syncs, c.summary()
    assert m.last_census.summary()['fallback_ops'] == 0
    assert int(res['count'][0]) > 0
