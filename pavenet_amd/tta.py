"""Test-time augmentation helpers shared by the detectors (opera/models/detectors/petr.py:118-187,
videoposev1.py:192-261): reading ``test_cfg.nms`` the way mmcv's ``batched_nms`` does, and the per-augmentation
meta the merge kernel takes."""
# mmcv/ops/nms.py: soft_nms defaults (sigma=0.5, min_score=1e-3, method='linear', offset=0); nms offset=0
_SOFT_KEYS = {'iou_threshold', 'iou_thr', 'sigma', 'min_score', 'method', 'offset'}
_NMS_KEYS = {'iou_threshold', 'iou_thr', 'offset'}
_IGNORED = {'class_agnostic', 'split_thr'}   # one class, at most 4096 boxes: neither changes the result


def parse_nms_cfg(nms_cfg):
    """test_cfg.nms -> (method, iou_thr, sigma, min_score, offset); method is 'nms' or the soft-NMS kind
    ('naive' / 'linear' / 'gaussian').  ``iou_thr`` is accepted as mmcv's alias of ``iou_threshold``."""
    cfg = dict(nms_cfg)
    kind = cfg.pop('type', 'nms')
    if kind not in ('nms', 'soft_nms'):
        raise NotImplementedError(f"test_cfg.nms.type {kind!r}: 'nms' and 'soft_nms' are supported")
    for k in _IGNORED:
        cfg.pop(k, None)
    unknown = set(cfg) - (_SOFT_KEYS if kind == 'soft_nms' else _NMS_KEYS)
    if unknown:
        raise NotImplementedError(f'test_cfg.nms keys {sorted(unknown)} are not supported for {kind}')
    if 'iou_threshold' in cfg and 'iou_thr' in cfg:
        raise ValueError('test_cfg.nms: give iou_threshold or its alias iou_thr, not both')
    if 'iou_threshold' not in cfg and 'iou_thr' not in cfg:
        raise ValueError(f'test_cfg.nms ({kind}) needs iou_threshold')
    iou = float(cfg.get('iou_threshold', cfg.get('iou_thr')))
    offset = int(cfg.get('offset', 0))
    if offset not in (0, 1):
        raise ValueError('test_cfg.nms.offset must be 0 or 1')
    if kind == 'nms':
        return 'nms', iou, 0.5, 1e-3, offset
    method = cfg.get('method', 'linear')
    if method not in ('naive', 'linear', 'gaussian'):
        raise ValueError(f"soft_nms method {method!r}: 'naive', 'linear' or 'gaussian'")
    return method, iou, float(cfg.get('sigma', 0.5)), float(cfg.get('min_score', 1e-3)), offset


def aug_meta(img_metas):
    """One augmentation's per-image metas -> (flip, img_w [B], scale_factor [B][4]); horizontal flips only."""
    flips = {bool(m.get('flip', False)) for m in img_metas}
    if len(flips) != 1:
        raise ValueError('the images of one augmentation must share its flip')
    flip = flips.pop()
    for m in img_metas:
        if flip and m.get('flip_direction', 'horizontal') != 'horizontal':
            raise NotImplementedError(f"flip_direction {m.get('flip_direction')!r}: the reference maps key points "
                                      'back for horizontal flips only (opera/core/keypoint/transforms.py:171)')
    sfs = []
    for m in img_metas:
        sf = m['scale_factor']
        sf = [float(sf)] * 4 if isinstance(sf, (int, float)) else [float(v) for v in sf]
        if len(sf) != 4:
            raise ValueError(f'scale_factor needs 4 values (w, h, w, h), got {sf}')
        sfs.append(sf)
    return flip, [float(m['img_shape'][1]) for m in img_metas], sfs
