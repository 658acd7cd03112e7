"""Test-time augmentation timings: PETR R-50 ``simple_test`` against the flip ``aug_test`` (two augmentations) at
800 x 1333, and the merge kernel (pave_aug_merge_nms_f32) alone at n = A * N = 200, 600 and 2048 boxes per image.

    python tools/bench_aug.py [--iters 20] [--skip-model]

Prints one JSON line.  Device time with events around `iters` back-to-back calls after a warm-up; the model rows
are end-to-end wall times of the public entry points (results_to_list's host copy included)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _merge_case(A, N, K=17, B=1, seed=0):
    rng = np.random.default_rng(seed)
    bbs, kps = [], []
    for _ in range(A):
        c = rng.uniform(0, 1200, size=(B, N, 2)).astype(np.float32)
        wh = rng.uniform(20, 300, size=(B, N, 2)).astype(np.float32)
        sc = rng.uniform(0, 1, size=(B, N, 1)).astype(np.float32)
        bbs.append(torch.from_numpy(np.concatenate([c, c + wh, sc], -1)).cuda())
        kps.append(torch.from_numpy(rng.uniform(0, 1300, size=(B, N, K, 3)).astype(np.float32)).cuda())
    return bbs, kps


def time_merge(n, method, iters):
    from pavenet_amd import ops
    from pavenet_amd.keypoints import flip_permutation
    A = 2 if n <= 600 else 4
    N = n // A
    bbs, kps = _merge_case(A, N)
    kw = dict(score_thr=0.0, max_num=100, method=method, iou_thr=0.5)
    args = (bbs, kps, [None] * A, [a % 2 == 1 for a in range(A)], [[1333.0]] * A, [[[1.0] * 4]] * A,
            flip_permutation(17))
    for _ in range(3):
        ops.aug_merge_nms(*args, **kw)
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        ops.aug_merge_nms(*args, **kw)
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1000.0 / iters


def time_model(iters):
    from oracle.seeded import seeded_array, seeded_state_dict
    from pavenet_amd.models import build_model, petr_r50_cfg
    m = build_model(petr_r50_cfg(num_keypoints=17, max_per_img=100))
    m.load_state_dict(seeded_state_dict({k: list(v.shape) for k, v in m.state_dict().items()}, like=m.state_dict()))
    m.test_cfg = dict(max_per_img=100, score_thr=0.0, nms=dict(type='soft_nms', iou_thr=0.5))
    m = m.cuda().eval()
    H, W = 800, 1333
    img = torch.from_numpy(seeded_array('bench_aug.img', (1, 3, H, W))).cuda()
    fimg = img.flip(-1).contiguous()
    meta = dict(batch_input_shape=(H, W), img_shape=(H, W, 3), pad_shape=(H, W, 3), scale_factor=(1.0,) * 4)
    metas = [[dict(meta, flip=False, flip_direction=None)], [dict(meta, flip=True, flip_direction='horizontal')]]
    out = {}
    for name, fn in (('simple_test_ms', lambda: m.simple_test(img, metas[0])),
                     ('aug_test_flip_ms', lambda: m.aug_test([img, fimg], metas))):
        with torch.no_grad():
            for _ in range(2):
                fn()
            torch.cuda.synchronize()
            t = []
            for _ in range(iters):
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                t.append((time.perf_counter() - t0) * 1000.0)
        out[name] = float(np.median(t))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--skip-model', action='store_true')
    a = ap.parse_args()
    res = dict(device=torch.cuda.get_device_name(0))
    for n in (200, 600, 2048):
        for method in ('linear', 'nms'):
            res[f'merge_{method}_n{n}_us'] = round(time_merge(n, method, a.iters * 5), 1)
    if not a.skip_model:
        res.update({k: round(v, 2) for k, v in time_model(a.iters).items()})
    print(json.dumps(res))


if __name__ == '__main__':
    main()
