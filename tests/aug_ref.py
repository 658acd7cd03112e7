"""Host restatement of the test-time augmentation merge, in fp32 NumPy:

* ``nms`` / ``soft_nms``: mmcv/ops/csrc/pytorch/cpu/nms.cpp:5-160 (nms_cpu, softnms_cpu), with the wrappers of
  mmcv/ops/nms.py (iou_thr alias, dets = boxes ++ scores).  ``soft_nms_literal`` is the C++ loop line by line;
  ``soft_nms`` the same result with the per-iteration weighting vectorised (every box of (i, n) receives one weight
  per iteration; the swap-with-last removal is a two-pointer partition).  Equal scores in hard NMS: lower index
  first (the reference leaves that order unspecified).
* ``multiclass_nms``: mmdet/core/post_processing/bbox_nms.py:8-93 for one class with return_inds.
* ``merge_aug``: opera/models/detectors/petr.py:118-187 (bbox_mapping_back / kpt_mapping_back / concatenation) +
  the merge -> (dets, labels, inds, kpts).
"""
import numpy as np

f32 = np.float32


def _areas(b, offset):
    o = f32(offset)
    return ((b[:, 2] - b[:, 0]) + o) * ((b[:, 3] - b[:, 1]) + o)


def _iou(box, iarea, boxes, areas, offset):
    """nms.cpp's ovr of one box against many (std::max / std::min operand order kept)."""
    o = f32(offset)
    xx1 = np.where(box[0] < boxes[:, 0], boxes[:, 0], box[0])
    yy1 = np.where(box[1] < boxes[:, 1], boxes[:, 1], box[1])
    xx2 = np.where(boxes[:, 2] < box[2], boxes[:, 2], box[2])
    yy2 = np.where(boxes[:, 3] < box[3], boxes[:, 3], box[3])
    w = (xx2 - xx1) + o
    h = (yy2 - yy1) + o
    w = np.where(f32(0) < w, w, f32(0))
    h = np.where(f32(0) < h, h, f32(0))
    inter = w * h
    return (inter / ((iarea + areas) - inter)).astype(f32)


def nms(boxes, scores, iou_threshold, offset=0):
    """-> (dets [k, 5], inds [k]) in descending-score order; ovr > thr suppresses."""
    boxes = np.asarray(boxes, f32).reshape(-1, 4)
    scores = np.asarray(scores, f32).reshape(-1)
    n = boxes.shape[0]
    if n == 0:
        return np.zeros((0, 5), f32), np.zeros((0,), np.int64)
    thr = f32(iou_threshold)
    areas = _areas(boxes, offset)
    order = np.argsort(-scores, kind='stable')
    select = np.ones(n, bool)
    for _i in range(n):
        if not select[_i]:
            continue
        i = order[_i]
        rest = order[_i + 1:]
        ovr = _iou(boxes[i], areas[i], boxes[rest], areas[rest], offset)
        select[_i + 1:] &= ~(ovr > thr)
    inds = order[select].astype(np.int64)
    return np.concatenate([boxes[inds], scores[inds, None]], 1), inds


_METHODS = {'naive': 0, 'linear': 1, 'gaussian': 2}


def _weight(ovr, method, thr, sigma):
    if method == 0:
        return np.where(ovr >= thr, f32(0), f32(1)).astype(f32)
    if method == 1:
        return np.where(ovr >= thr, (f32(1) - ovr).astype(f32), f32(1)).astype(f32)
    return np.exp((-(ovr * ovr) / f32(sigma)).astype(f32)).astype(f32)


def soft_nms_literal(boxes, scores, iou_threshold=0.3, sigma=0.5, min_score=1e-3, method='linear', offset=0):
    """softnms_cpu line by line (slow: for checking ``soft_nms``)."""
    b = np.array(boxes, f32).reshape(-1, 4)
    sc = np.array(scores, f32).reshape(-1)
    nb = b.shape[0]
    m, thr, ms = _METHODS[method], f32(iou_threshold), f32(min_score)
    areas = _areas(b, offset)
    inds = np.arange(nb, dtype=np.int64)
    dets = np.zeros((nb, 5), f32)
    i = 0
    while i < nb:
        max_pos = i
        for pos in range(i + 1, nb):
            if sc[max_pos] < sc[pos]:
                max_pos = pos
        for arr in (b, sc, areas, inds):
            t = arr[max_pos].copy()
            arr[max_pos] = arr[i]
            arr[i] = t
        dets[i, :4], dets[i, 4] = b[i], sc[i]
        pos = i + 1
        while pos < nb:
            ovr = _iou(b[i], areas[i], b[pos:pos + 1], areas[pos:pos + 1], offset)
            sc[pos] = sc[pos] * _weight(ovr, m, thr, sigma)[0]
            if sc[pos] < ms:
                b[pos], sc[pos], areas[pos], inds[pos] = b[nb - 1], sc[nb - 1], areas[nb - 1], inds[nb - 1]
                nb -= 1
                pos -= 1
            pos += 1
        i += 1
    return dets[:nb], inds[:nb]


def soft_nms(boxes, scores, iou_threshold=0.3, sigma=0.5, min_score=1e-3, method='linear', offset=0,
             max_rows=None):
    """softnms_cpu with the per-iteration weighting vectorised; max_rows stops after that many selections (the
    later ones cannot change the first max_rows rows)."""
    b = np.array(boxes, f32).reshape(-1, 4)
    sc = np.array(scores, f32).reshape(-1)
    nb = b.shape[0]
    m, thr, ms = _METHODS[method], f32(iou_threshold), f32(min_score)
    areas = _areas(b, offset)
    inds = np.arange(nb, dtype=np.int64)
    i = 0
    while i < nb and (max_rows is None or i < max_rows):
        seg = sc[i:nb]
        max_pos = i if np.isnan(seg[0]) else i + int(np.argmax(np.where(np.isnan(seg), -np.inf, seg)))
        for arr in (b, sc, areas, inds):
            t = arr[max_pos].copy()
            arr[max_pos] = arr[i]
            arr[i] = t
        if i + 1 < nb:
            ovr = _iou(b[i], areas[i], b[i + 1:nb], areas[i + 1:nb], offset)
            sc[i + 1:nb] = (sc[i + 1:nb] * _weight(ovr, m, thr, sigma)).astype(f32)
            alive = ~(sc[i + 1:nb] < ms)
            S = int(alive.sum())
            head = np.arange(i + 1, i + 1 + S)
            holes = head[~alive[:S]]
            tail = np.arange(i + 1 + S, nb)[alive[S:]][::-1]   # survivors beyond the head, from the back
            for arr in (b, sc, areas, inds):
                arr[holes] = arr[tail]
            nb = i + 1 + S
        i += 1
    return np.concatenate([b[:i], sc[:i, None]], 1), inds[:i]


def parse_nms_cfg(nms_cfg):
    """test_cfg.nms -> (method, iou_thr, sigma, min_score, offset) as the package reads it."""
    from pavenet_amd.tta import parse_nms_cfg as p
    return p(nms_cfg)


def multiclass_nms(bboxes, scores, score_thr, nms_cfg, max_num=-1):
    """One class, return_inds=True -> (dets [k, 5], labels [k], inds [k])."""
    method, iou_thr, sigma, min_score, offset = parse_nms_cfg(nms_cfg)
    bboxes = np.asarray(bboxes, f32).reshape(-1, 4)
    scores = np.asarray(scores, f32).reshape(-1)
    valid = np.nonzero(scores > f32(score_thr))[0].astype(np.int64)
    if valid.size == 0:
        return np.zeros((0, 5), f32), np.zeros((0,), np.int64), valid
    b, s = bboxes[valid], scores[valid]
    if method == 'nms':
        dets, keep = nms(b, s, iou_thr, offset)
    else:
        dets, keep = soft_nms(b, s, iou_thr, sigma, min_score, method, offset,
                              max_rows=max_num if max_num > 0 else None)
    dets = np.concatenate([b[keep], dets[:, -1:]], 1)
    if max_num > 0:
        dets, keep = dets[:max_num], keep[:max_num]
    return dets, np.zeros(keep.shape, np.int64), valid[keep]


def map_back(bboxes, kpts, img_w, scale_factor, flip, flip_perm):
    """bbox_mapping_back + kpt_mapping_back of one augmentation: bboxes [n, 4], kpts [n, K, 2]."""
    bboxes = np.array(bboxes, f32)
    kpts = np.array(kpts, f32)
    w = f32(img_w)
    if flip:
        fb = bboxes.copy()
        fb[:, 0] = w - bboxes[:, 2]
        fb[:, 2] = w - bboxes[:, 0]
        bboxes = fb
        kpts = kpts.copy()
        kpts[..., 0] = w - kpts[..., 0]
        kpts = kpts[:, list(flip_perm)]
    sf = np.asarray(scale_factor, f32)
    return (bboxes / sf).astype(f32), (kpts / sf[:2]).astype(f32)


def merge_aug(aug_results, metas, flip_perm, score_thr, nms_cfg, max_num):
    """aug_results: per augmentation (bboxes [n, 5], kpts [n, K, >=2]) rows in results_to_list order;
    metas: per augmentation dict(img_w, scale_factor, flip) -> (dets, labels, inds, kpts [k, K, 3],
    merged (bboxes, scores, kpts))."""
    mb, ms, mk = [], [], []
    for (bb, kp), meta in zip(aug_results, metas):
        bb = np.asarray(bb, f32)
        b, k = map_back(bb[:, :4], np.asarray(kp, f32)[..., :2], meta['img_w'], meta['scale_factor'],
                        meta['flip'], flip_perm)
        mb.append(b)
        ms.append(bb[:, 4])
        mk.append(k)
    mb, ms, mk = np.concatenate(mb), np.concatenate(ms), np.concatenate(mk)
    dets, labels, inds = multiclass_nms(mb, ms, score_thr, nms_cfg, max_num)
    k = mk[inds]
    k = np.concatenate([k, np.ones(k[..., :1].shape, f32)], -1)
    return dets, labels, inds, k, (mb, ms, mk)
