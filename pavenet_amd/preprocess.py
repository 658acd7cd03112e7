"""GPU input pipeline: raw decoded frames -> the network's input tensor
and ``img_metas``, on the device, in one HIP launch per clip.

Restates the reference's test pipeline
(configs/_base_/datasets/posetrack17_video_keypoint.py:71-84): Resize(img_scale=(1333, 800),
keep_ratio=True) [mmcv.imrescale -> rescale_size + cv2 INTER_LINEAR on float32 frames, since
the loader uses to_float32=True], RandomFlip(off), Normalize(mean, std, to_rgb=True),
Pad(size_divisor), MulImageToTensor / stacking of the T frames
(mmdet/datasets/pipelines/formatting.py:502-546).
"""
import ctypes

import torch

from .ops import _launch, _require

MEAN = (123.675, 116.28, 103.53)
STD = (58.395, 57.12, 57.375)


def rescale_size(old_size, scale):
    """mmcv.image.rescale_size for a (long_edge, short_edge) tuple scale: old_size = (w, h)."""
    w, h = old_size
    max_long_edge, max_short_edge = max(scale), min(scale)
    f = min(max_long_edge / max(h, w), max_short_edge / min(h, w))
    return int(w * float(f) + 0.5), int(h * float(f) + 0.5)


def plan_clip(H0, W0, img_scale=(1333, 800), size_divisor=1):
    """Host arithmetic of Resize(keep_ratio=True) + Pad(size_divisor) for an H0 x W0 source:
    -> (Hn, Wn, Hp, Wp, scale_factor) exactly as mmcv.rescale_size, mmdet's Resize._resize_img
    (w_scale = new_w / w, h_scale = new_h / h) and mmcv.impad_to_multiple compute them."""
    Wn, Hn = rescale_size((W0, H0), img_scale)
    d = max(int(size_divisor), 1)
    Hp, Wp = -(-Hn // d) * d, -(-Wn // d) * d
    ws, hs = Wn / W0, Hn / H0
    return Hn, Wn, Hp, Wp, (ws, hs, ws, hs)


def preprocess_clip(frames, img_scale=(1333, 800), size_divisor=1, mean=MEAN, std=STD,
                    to_rgb=True, flip=False):
    """frames [T, H0, W0, 3] uint8 / float32 BGR on the device -> (img [1, T, 3, Hp, Wp] fp32,
    img_meta dict with ori_shape / img_shape / pad_shape / batch_input_shape / scale_factor / flip).

    flip=True: mmdet's RandomFlip(horizontal) between Resize and Normalize -- the resized image is mirrored
    within its Wn columns (pave_preprocess_frames_flip), the padding stays on the right."""
    _require(frames.is_cuda and frames.dim() == 4 and frames.shape[-1] == 3 and
             frames.is_contiguous(), 'preprocess_clip: frames must be a contiguous device '
             '[T, H, W, 3] tensor')
    _require(frames.dtype in (torch.uint8, torch.float32), 'preprocess_clip: uint8 or float32')
    T, H0, W0, _ = frames.shape
    Hn, Wn, Hp, Wp, scale_factor = plan_clip(H0, W0, img_scale, size_divisor)
    out = torch.empty((1, T, 3, Hp, Wp), dtype=torch.float32, device=frames.device)
    m = (ctypes.c_float * 3)(*mean)
    s = (ctypes.c_float * 3)(*std)
    _launch('pave_preprocess_frames_flip' if flip else 'pave_preprocess_frames', 'preprocess_frames', frames.device,
            frames.data_ptr(), int(frames.dtype == torch.uint8), out.data_ptr(), T, H0, W0, Hn, Wn, Hp, Wp,
            ctypes.cast(m, ctypes.c_void_p), ctypes.cast(s, ctypes.c_void_p), int(bool(to_rgb)))
    meta = dict(ori_shape=(H0, W0, 3), img_shape=(Hn, Wn, 3), pad_shape=(Hp, Wp, 3),
                batch_input_shape=(Hp, Wp), scale_factor=scale_factor, flip=bool(flip),
                flip_direction='horizontal' if flip else None)
    return out, meta


def aug_plan(img_scale, flip=False, flip_direction='horizontal'):
    """mmdet MultiScaleFlipAug's order (mmdet/datasets/pipelines/test_time_aug.py:54-110): scales outer, flips
    inner, [(False, None)] + [(True, d) for d in flip_direction] -> [(scale, flip, direction), ...]."""
    scales = list(img_scale) if isinstance(img_scale, list) else [img_scale]
    dirs = list(flip_direction) if isinstance(flip_direction, list) else [flip_direction]
    flips = [(False, None)] + ([(True, d) for d in dirs] if flip else [])
    return [(tuple(s), f, d) for s in scales for f, d in flips]


def multi_scale_flip_aug(frames, img_scale=(1333, 800), flip=False, flip_direction='horizontal', size_divisor=1,
                         mean=MEAN, std=STD, to_rgb=True):
    """Every augmentation of MultiScaleFlipAug on the device -> (imgs, img_metas), one entry per augmentation in
    mmdet's order: imgs[a] [1, T, 3, Hp, Wp] (a PETR image is imgs[a][:, 0]), img_metas[a] = [meta] (mmdet's
    nesting: one list of per-image metas per augmentation).  Horizontal flips only, as the reference's
    kpt_flip asserts."""
    imgs, metas = [], []
    for scale, f, d in aug_plan(img_scale, flip, flip_direction):
        if f and d != 'horizontal':
            raise NotImplementedError(f'flip_direction {d!r}: the reference flips key points horizontally only '
                                      '(opera/core/keypoint/transforms.py:171)')
        img, meta = preprocess_clip(frames, scale, size_divisor, mean, std, to_rgb, flip=f)
        imgs.append(img)
        metas.append([meta])
    return imgs, metas


def tta_from_config(cfg):
    """The MultiScaleFlipAug arguments of a loaded config's ``data.test.pipeline`` -> kwargs of
    ``multi_scale_flip_aug`` (img_scale, flip, flip_direction, size_divisor, mean, std, to_rgb).  Supports the
    img_scale form; scale_factor raises NotImplementedError."""
    data = cfg['data'] if 'data' in cfg else {}
    pipeline = data.get('test', {}).get('pipeline')
    if pipeline is None:
        raise KeyError('config has no data.test.pipeline')
    step = next((t for t in pipeline if str(t.get('type', '')).split('.')[-1] == 'MultiScaleFlipAug'), None)
    if step is None:
        raise ValueError('data.test.pipeline has no MultiScaleFlipAug step')
    if step.get('scale_factor') is not None:
        raise NotImplementedError('MultiScaleFlipAug(scale_factor=...) is not supported: use img_scale')
    img_scale = step.get('img_scale')
    if img_scale is None:
        raise ValueError('MultiScaleFlipAug needs img_scale')
    multi = isinstance(img_scale, list) and not isinstance(img_scale[0], (int, float))   # (a JSON pair is a list)
    out = dict(img_scale=[tuple(s) for s in img_scale] if multi else tuple(img_scale),
               flip=bool(step.get('flip', False)), flip_direction=step.get('flip_direction', 'horizontal'),
               size_divisor=1, mean=MEAN, std=STD, to_rgb=True)
    for t in step.get('transforms', []):
        kind = str(t.get('type', '')).split('.')[-1]
        if kind == 'Resize' and not t.get('keep_ratio', True):
            raise NotImplementedError('Resize(keep_ratio=False) is not supported')
        if kind == 'Normalize':
            out.update(mean=tuple(t['mean']), std=tuple(t['std']), to_rgb=bool(t.get('to_rgb', True)))
        if kind == 'Pad':
            if t.get('size') is not None:
                raise NotImplementedError('Pad(size=...) is not supported: use size_divisor')
            out['size_divisor'] = int(t.get('size_divisor') or 1)
    return out
