"""Fixtures of the test-time augmentation tests (tests/test_aug_cpu.py, tests/test_aug_gpu.py), generated from the
reference in the build container:

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_aug.py

* ``aug_petr_r50.npz``: the reference's own ``PETR.aug_test`` (opera/models/detectors/petr.py:151-187) with
  name-seeded weights on a 120 x 150 image in a 128 x 160 canvas, two augmentations (original, horizontal flip),
  the flip-test config's test_cfg with max_per_img=20.  Stored per augmentation: the proposal / score top-k
  selections and the raw head results; the merged NMS inputs; the final dets / labels / inds / kpts.  Variant
  ``nms_*``: test_cfg.nms type='nms'.  (K = 14 is not generated: the R-50 config's K = 17 layer settings do not
  carry over by overriding num_keypoints alone; tests/test_aug_gpu.py covers the CrowdPose pairs against the host
  composition instead.)
  mmcv's ``nms`` / ``softnms`` are compiled C++ (mmcv._ext) that this repository cannot build: the generator swaps
  in the tests' restatement of the two ops (tests/aug_ref.py); everything else -- head, get_bboxes, the mapping
  back, merge_aug_results, multiclass_nms, batched_nms -- is the reference's own code.
* ``aug_flip_test_config.json``: the flip-test config's resolved test_cfg and test pipeline.
* ``flip_pairs.json``: the reference's FLIP_PAIRS (opera/datasets/coco_pose.py:44, crowd_pose.py:42).

Uses oracle/ref_shim.py and oracle/seeded.py read-only.
"""
import ast
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
import ref_shim  # noqa: E402
from seeded import seeded_array, seeded_state_dict  # noqa: E402
from tests import aug_ref  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden')
FLIP_CFG = 'configs/petr/petr_swin-l-p4-w7-224-22kto1k_16x1_100e_crowdpose_flip_test.py'
PETR_CFG = 'configs/petr/petr_r50_16x2_100e_coco.py'


def _flip_pairs(rel, cls):
    tree = ast.parse(open(os.path.join(ref_shim.REF, rel)).read())
    for node in ast.walk(tree):
        if isinstance(node, ast.ClassDef) and node.name == cls:
            for st in node.body:
                if isinstance(st, ast.Assign) and st.targets[0].id == 'FLIP_PAIRS':
                    return ast.literal_eval(st.value)
    raise KeyError(cls)


def gen_flip_pairs():
    pairs = dict(coco=_flip_pairs('opera/datasets/coco_pose.py', 'CocoPoseDataset'),
                 crowdpose=_flip_pairs('opera/datasets/crowd_pose.py', 'CrowdPoseDataset'))
    path = os.path.join(OUT, 'flip_pairs.json')
    json.dump(pairs, open(path, 'w'), indent=1)
    print('wrote', path)


def _plain(x):
    if isinstance(x, dict):
        return {k: _plain(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_plain(v) for v in x]
    return x


def gen_config():
    ref_shim.install()
    from mmcv import Config
    cfg = Config.fromfile(os.path.join(ref_shim.REF, FLIP_CFG))
    out = dict(test_cfg=_plain(dict(cfg.model['test_cfg'])),
               data=dict(test=dict(pipeline=_plain(list(cfg.data['test']['pipeline'])))))
    path = os.path.join(OUT, 'aug_flip_test_config.json')
    json.dump(out, open(path, 'w'), indent=1)
    print('wrote', path)
    return out['test_cfg']


def _nms_ops():
    """mmcv.ops.nms's two compiled ops -> the restatement (batched_nms looks them up by name in that module)."""
    import mmcv.ops  # noqa: F401
    mnms = sys.modules['mmcv.ops.nms']   # (the package attribute `nms` is the function, not the module)

    def soft_nms(boxes, scores, iou_threshold=0.3, sigma=0.5, min_score=1e-3, method='linear', offset=0,
                 iou_thr=None):
        if iou_thr is not None:
            iou_threshold = iou_thr
        dets, inds = aug_ref.soft_nms(boxes.cpu().numpy(), scores.cpu().numpy(), iou_threshold, sigma, min_score,
                                      method, offset)
        return torch.from_numpy(dets), torch.from_numpy(inds)

    def nms(boxes, scores, iou_threshold=None, offset=0, score_threshold=0, max_num=-1, iou_thr=None):
        if iou_thr is not None:
            iou_threshold = iou_thr
        dets, inds = aug_ref.nms(boxes.cpu().numpy(), scores.cpu().numpy(), iou_threshold, offset)
        return torch.from_numpy(dets), torch.from_numpy(inds)
    mnms.soft_nms = soft_nms
    mnms.nms = nms


def gen_petr(test_cfg):
    ref_shim.install()
    _nms_ops()
    arrays = {}
    for prefix, K, nms_cfg in (('', 17, test_cfg['nms']), ('nms_', 17, dict(type='nms', iou_thr=0.5))):
        def small(cfg):
            cfg.model['test_cfg'] = dict(test_cfg, max_per_img=20, nms=nms_cfg)
            if K != 17:
                head = cfg.model['bbox_head']
                head['num_keypoints'] = K
                head['transformer']['num_keypoints'] = K
                head['transformer']['decoder']['num_keypoints'] = K
                for lay in ('decoder', 'refine_decoder'):
                    if 'num_keypoints' in head['transformer'][lay]:
                        head['transformer'][lay]['num_keypoints'] = K
                    tl = head['transformer'][lay]['transformerlayers']
                    for a in (tl['attn_cfgs'] if isinstance(tl['attn_cfgs'], (list, tuple)) else [tl['attn_cfgs']]):
                        if 'num_points' in a and a['num_points'] == 17:
                            a['num_points'] = K
                for k in ('loss_oks', 'loss_oks_refine'):
                    if k in head and 'num_keypoints' in head[k]:
                        head[k]['num_keypoints'] = K
        model, cfg = ref_shim.build_reference_model(PETR_CFG, cfg_overrides=small)
        from mmcv import ConfigDict
        model.test_cfg = ConfigDict(model.test_cfg)   # aug_test reads test_cfg.score_thr as an attribute
        sd = model.state_dict()
        shapes = {k: list(v.shape) for k, v in sd.items()}
        model.load_state_dict(seeded_state_dict(shapes, 0, like=sd))
        H, W = 128, 160
        img = torch.from_numpy(seeded_array('aug_petr_r50.img', (1, 3, H, W)))   # (regenerated by the tests)
        # the flipped augmentation: the 150-wide image mirrored within its columns, padding on the right
        fimg = img.clone()
        fimg[..., :150] = img[..., :150].flip(-1)
        base = dict(batch_input_shape=(H, W), img_shape=(120, 150, 3), ori_shape=(120, 150, 3),
                    pad_shape=(H, W, 3), scale_factor=np.array([1., 1., 1., 1.], np.float32))
        metas = [[dict(base, flip=False, flip_direction=None)],
                 [dict(base, flip=True, flip_direction='horizontal')]]
        taps = []
        head_forward = model.bbox_head.forward
        get_bboxes = model.bbox_head.get_bboxes

        def tapped_forward(*a, **k):
            out = head_forward(*a, **k)
            taps.append(dict(cls_all=out[0].detach().clone(),
                             enc_cls=next(o for o in out[2:4] if o.dim() == 3 and o.shape[-1] == 1).detach().clone()))
            return out

        def tapped_get_bboxes(*a, **k):
            res = get_bboxes(*a, **k)
            taps[-1]['res'] = [(b.clone(), l.clone(), kp.clone()) for b, l, kp in res]
            return res
        model.bbox_head.forward = tapped_forward
        model.bbox_head.get_bboxes = tapped_get_bboxes
        import mmdet.core.post_processing.bbox_nms as bn
        captured = {}
        mc = bn.multiclass_nms

        def tapped_mc(multi_bboxes, multi_scores, *a, **k):
            captured['bboxes'], captured['scores'] = multi_bboxes.clone(), multi_scores.clone()
            return mc(multi_bboxes, multi_scores, *a, **k)
        import opera.models.detectors.petr as petr_mod
        petr_mod.multiclass_nms = tapped_mc
        with torch.no_grad():
            out = model.aug_test([img, fimg], metas)
        petr_mod.multiclass_nms = mc
        N = model.bbox_head.test_cfg['max_per_img']
        for a, t in enumerate(taps):
            arrays[f'{prefix}score_topk_{a}'] = t['cls_all'][-1][0].sigmoid().view(-1).topk(N)[1].numpy()
            arrays[f'{prefix}enc_topk_{a}'] = torch.topk(t['enc_cls'][..., 0], model.bbox_head.num_query,
                                                         dim=1)[1].numpy()
            b, _, kp = t['res'][0]
            arrays[f'{prefix}aug_bboxes_{a}'] = b.numpy()
            arrays[f'{prefix}aug_kpts_{a}'] = kp.numpy()
        arrays[f'{prefix}merged_bboxes'] = captured['bboxes'].numpy()
        arrays[f'{prefix}merged_scores'] = captured['scores'][:, 0].numpy()
        bbox_res, kpt_res = out[0]
        arrays[f'{prefix}det_bboxes'] = bbox_res[0]
        arrays[f'{prefix}det_kpts'] = kpt_res[0]
        # inds: recompute from the merged inputs with the same restatement (multiclass_nms returns them, aug_test
        # drops them); checked against the reference's dets below
        dets, labels, inds = aug_ref.multiclass_nms(captured['bboxes'].numpy(), captured['scores'][:, 0].numpy(),
                                                    test_cfg['score_thr'], nms_cfg, N)
        assert np.array_equal(dets, bbox_res[0]), 'restated merge != the reference aug_test'
        arrays[f'{prefix}det_inds'] = inds
        arrays[f'{prefix}det_labels'] = labels
        arrays['keys'] = json.dumps(shapes)
    path = os.path.join(OUT, 'aug_petr_r50.npz')
    np.savez_compressed(path, **arrays)
    print('wrote', path, os.path.getsize(path) // 1024, 'KiB')


if __name__ == '__main__':
    gen_flip_pairs()
    tc = gen_config()
    gen_petr(tc)
