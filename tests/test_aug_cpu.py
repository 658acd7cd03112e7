"""Test-time augmentation, host side: the NMS restatement (tests/aug_ref.py) against mmcv's docstring examples and
the reference's recorded merge, the flip pairs, the augmentation plan of the flip-test config, the C ABI."""
import json
import os

import numpy as np
import pytest

from tests import aug_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def test_restatement_reproduces_mmcv_docstring_examples():
    # mmcv/ops/nms.py nms docstring: 3 boxes survive
    boxes = np.array([[49.1, 32.4, 51.0, 35.9], [49.3, 32.9, 51.0, 35.3], [49.2, 31.8, 51.0, 35.4],
                      [35.1, 11.5, 39.1, 15.7], [35.6, 11.8, 39.3, 14.2], [35.3, 11.5, 39.9, 14.5],
                      [35.2, 11.7, 39.7, 15.7]], dtype=np.float32)
    scores = np.array([0.9, 0.9, 0.5, 0.5, 0.5, 0.4, 0.3], dtype=np.float32)
    dets, inds = aug_ref.nms(boxes, scores, 0.6)
    assert len(inds) == len(dets) == 3
    # soft_nms docstring: 5 boxes survive
    boxes = np.array([[4., 3., 5., 3.], [4., 3., 5., 4.], [3., 1., 3., 1.], [3., 1., 3., 1.], [3., 1., 3., 1.],
                      [3., 1., 3., 1.]], dtype=np.float32)
    scores = np.array([0.9, 0.9, 0.5, 0.5, 0.4, 0.0], dtype=np.float32)
    with np.errstate(invalid='ignore'):
        dets, inds = aug_ref.soft_nms(boxes, scores, 0.6, sigma=0.5)
    assert len(inds) == len(dets) == 5


@pytest.mark.parametrize('method', ['naive', 'linear', 'gaussian'])
@pytest.mark.parametrize('offset', [0, 1])
def test_vectorised_soft_nms_equals_the_literal_loop(method, offset):
    rng = np.random.default_rng(7)
    n = 150
    base = rng.uniform(0, 100, size=(12, 2)).astype(np.float32)
    c = base[rng.integers(0, 12, size=n)] + rng.normal(0, 4, size=(n, 2)).astype(np.float32)
    wh = rng.uniform(5, 30, size=(n, 2)).astype(np.float32)
    boxes = np.concatenate([c, c + wh], 1).astype(np.float32)
    scores = rng.uniform(0, 1, size=n).astype(np.float32)
    scores[::7] = scores[3]   # equal scores
    d1, i1 = aug_ref.soft_nms(boxes, scores, 0.4, 0.5, 1e-3, method, offset)
    d2, i2 = aug_ref.soft_nms_literal(boxes, scores, 0.4, 0.5, 1e-3, method, offset)
    assert np.array_equal(i1, i2)
    assert np.array_equal(d1, d2)


@pytest.mark.parametrize('prefix,nms_cfg', [('', None), ('nms_', dict(type='nms', iou_thr=0.5))])
def test_restatement_reproduces_the_reference_merge(prefix, nms_cfg):
    g = np.load(os.path.join(GOLDEN, 'aug_petr_r50.npz'))
    cfg = json.load(open(os.path.join(GOLDEN, 'aug_flip_test_config.json')))['test_cfg']
    dets, labels, inds = aug_ref.multiclass_nms(g[prefix + 'merged_bboxes'], g[prefix + 'merged_scores'],
                                                cfg['score_thr'], nms_cfg or cfg['nms'], 20)
    assert np.array_equal(dets, g[prefix + 'det_bboxes'])
    assert np.array_equal(inds, g[prefix + 'det_inds'])
    assert not labels.any()
    # and the whole merge (mapping back included) from the per-augmentation head results
    from pavenet_amd.keypoints import flip_permutation
    metas = [dict(img_w=150, scale_factor=[1.] * 4, flip=False), dict(img_w=150, scale_factor=[1.] * 4, flip=True)]
    aug = [(g[f'{prefix}aug_bboxes_{a}'], g[f'{prefix}aug_kpts_{a}']) for a in range(2)]
    d2, _, i2, k2, (mb, ms, _) = aug_ref.merge_aug(aug, metas, flip_permutation(17), cfg['score_thr'],
                                                   nms_cfg or cfg['nms'], 20)
    assert np.array_equal(mb, g[prefix + 'merged_bboxes']) and np.array_equal(ms, g[prefix + 'merged_scores'])
    assert np.array_equal(d2, g[prefix + 'det_bboxes']) and np.array_equal(i2, g[prefix + 'det_inds'])
    np.testing.assert_array_equal(k2, g[prefix + 'det_kpts'])


def test_flip_pairs_match_the_reference():
    from pavenet_amd import keypoints
    ref = json.load(open(os.path.join(GOLDEN, 'flip_pairs.json')))
    assert keypoints.flip_pairs(17) == ref['coco']
    assert keypoints.flip_pairs(14) == ref['crowdpose']
    for K in (15, 13):
        with pytest.raises(NotImplementedError):
            keypoints.flip_permutation(K)
    p = keypoints.flip_permutation(17)
    assert sorted(p) == list(range(17)) and p[0] == 0 and p[1] == 2 and p[16] == 15


def test_augmentation_plan_of_the_flip_test_config():
    from pavenet_amd.preprocess import aug_plan, tta_from_config
    cfg = json.load(open(os.path.join(GOLDEN, 'aug_flip_test_config.json')))
    kw = tta_from_config(cfg)
    assert kw['img_scale'] == (1333, 800) and kw['flip'] is True and kw['size_divisor'] == 1
    assert aug_plan(kw['img_scale'], kw['flip'], kw['flip_direction']) == \
        [((1333, 800), False, None), ((1333, 800), True, 'horizontal')]
    # mmdet's order: scales outer, flips inner
    assert aug_plan([(1333, 800), (1000, 600)], True, ['horizontal']) == \
        [((1333, 800), False, None), ((1333, 800), True, 'horizontal'),
         ((1000, 600), False, None), ((1000, 600), True, 'horizontal')]
    step = cfg['data']['test']['pipeline'][1]
    bad = dict(data=dict(test=dict(pipeline=[dict(step, scale_factor=[1.0, 2.0], img_scale=None)])))
    with pytest.raises(NotImplementedError):
        tta_from_config(bad)


def test_nms_cfg_reading():
    from pavenet_amd.tta import parse_nms_cfg
    assert parse_nms_cfg(dict(type='soft_nms', iou_thr=0.5)) == ('linear', 0.5, 0.5, 1e-3, 0)
    assert parse_nms_cfg(dict(type='nms', iou_threshold=0.6, offset=1)) == ('nms', 0.6, 0.5, 1e-3, 1)
    with pytest.raises(NotImplementedError):
        parse_nms_cfg(dict(type='soft_nms', iou_thr=0.5, score_threshold=0.1))
    with pytest.raises(ValueError):
        parse_nms_cfg(dict(type='nms'))


def test_tta_without_nms_config_names_the_key():
    from pavenet_amd.detectors import VideoPoseV1
    m = VideoPoseV1.__new__(VideoPoseV1)
    object.__setattr__(m, '_modules', {})
    m.__dict__['test_cfg'] = dict(max_per_img=100, score_thr=0.0)
    with pytest.raises(ValueError, match='nms'):
        m._tta_cfg()


def test_aug_abi_symbols_are_exported():
    import subprocess
    from pavenet_amd import native
    from pavenet_amd.build_native import build_native
    build_native()
    for name in ('pave_aug_merge_nms_f32', 'pave_hflip_canvas_f32', 'pave_preprocess_frames_flip'):
        assert name in native.SIGNATURES and name in native.EXPORTED
    out = subprocess.run(['nm', '-D', '--defined-only', native.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    syms = {ln.split()[-1] for ln in out.splitlines() if ' T ' in ln}
    assert {'pave_aug_merge_nms_f32', 'pave_hflip_canvas_f32', 'pave_preprocess_frames_flip'} <= syms
    assert native.ABI_VERSION == 21


def test_aug_plan_struct_layout_equals_the_header(tmp_path):
    import ctypes
    import shutil
    import subprocess
    from pavenet_amd import native
    if not shutil.which('gcc'):
        pytest.skip('no gcc')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    fields = [f for f, _ in native.AugPlan._fields_]
    src = tmp_path / 'layout.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pave_hip.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(pave_aug_plan));\n'
                   + ''.join(f'  printf(" %zu", offsetof(pave_aug_plan, {f}));\n' for f in fields)
                   + '  return 0;\n}\n')
    exe = tmp_path / 'layout'
    subprocess.run(['gcc', '-std=c99', '-I', os.path.join(root, 'include'), str(src), '-o', str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == ctypes.sizeof(native.AugPlan)
    assert got[1:] == [getattr(native.AugPlan, f).offset for f in fields]
