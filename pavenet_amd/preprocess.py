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

from . import native
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


NV12_MATRICES = {'bt601': (0.299, 0.114), 'bt709': (0.2126, 0.0722)}   # (Kr, Kb); Kg = 1 - Kr - Kb


def nv12_csc(matrix='bt601', full_range=False):
    """The six coefficients (yoff, cy, crv, cgu, cgv, cbu) of pave_preprocess_frames_nv12 for a Y'CbCr matrix
    ('bt601' | 'bt709') and range, computed in double: limited range has Y in 16 .. 235 and chroma in 16 .. 240
    (yoff 16, cy = 255 / 219, chroma factor q = 255 / 224), full range uses all 256 codes (0, 1, 1)."""
    if matrix not in NV12_MATRICES:
        raise ValueError(f'nv12_csc: unknown matrix {matrix!r} (one of {sorted(NV12_MATRICES)})')
    kr, kb = NV12_MATRICES[matrix]
    kg = 1.0 - kr - kb
    yoff, cy, q = (0.0, 1.0, 1.0) if full_range else (16.0, 255.0 / 219.0, 255.0 / 224.0)
    return (yoff, cy, 2.0 * (1.0 - kr) * q, -2.0 * kb * (1.0 - kb) * q / kg, -2.0 * kr * (1.0 - kr) * q / kg,
            2.0 * (1.0 - kb) * q)


def preprocess_clip_nv12(surfaces, width, img_scale=(1333, 800), size_divisor=1, mean=MEAN, std=STD,
                         to_rgb=True, matrix='bt601', full_range=False):
    """surfaces [T, H0 * 3 // 2, pitch] uint8 NV12 on the device (H0 rows of Y, then H0 / 2 rows of interleaved
    U, V, `pitch` bytes each, of which the first `width` belong to the picture) -> the same (img [1, T, 3, Hp, Wp]
    fp32, img_meta) as preprocess_clip gives for the H0 x width BGR picture the conversion of nv12_csc(matrix,
    full_range) produces, in one launch and without that picture ever being stored."""
    if not (isinstance(surfaces, torch.Tensor) and surfaces.dim() == 3 and surfaces.dtype == torch.uint8):
        raise ValueError('preprocess_clip_nv12: surfaces must be a [T, H0 * 3 // 2, pitch] uint8 tensor')
    T, rows, pitch = surfaces.shape
    H0, W0 = rows * 2 // 3, int(width)
    if rows % 3 != 0 or H0 % 2 != 0 or H0 <= 0:
        raise ValueError(f'preprocess_clip_nv12: {rows} rows are not the 3/2 of an even height')
    if W0 <= 0 or W0 % 2 != 0:
        raise ValueError(f'preprocess_clip_nv12: width {W0} must be even and positive')
    if W0 > pitch:
        raise ValueError(f'preprocess_clip_nv12: width {W0} exceeds the pitch {pitch}')
    csc = (ctypes.c_float * 6)(*nv12_csc(matrix, full_range))
    _require(surfaces.is_cuda and surfaces.is_contiguous() and T > 0,
             'preprocess_clip_nv12: surfaces must be a contiguous device tensor')
    Hn, Wn, Hp, Wp, scale_factor = plan_clip(H0, W0, img_scale, size_divisor)
    out = torch.empty((1, T, 3, Hp, Wp), dtype=torch.float32, device=surfaces.device)
    m = (ctypes.c_float * 3)(*mean)
    s = (ctypes.c_float * 3)(*std)
    _launch('pave_preprocess_frames_nv12', 'preprocess_frames_nv12', surfaces.device,
            surfaces.data_ptr(), rows * pitch, pitch, out.data_ptr(), T, H0, W0, Hn, Wn, Hp, Wp,
            ctypes.cast(csc, ctypes.c_void_p), ctypes.cast(m, ctypes.c_void_p), ctypes.cast(s, ctypes.c_void_p),
            int(bool(to_rgb)))
    meta = dict(ori_shape=(H0, W0, 3), img_shape=(Hn, Wn, 3), pad_shape=(Hp, Wp, 3),
                batch_input_shape=(Hp, Wp), scale_factor=scale_factor, flip=False, flip_direction=None)
    return out, meta


def preprocess_surfaces_nv12(surfaces, width, img_scale=(1333, 800), size_divisor=1, mean=MEAN, std=STD,
                             to_rgb=True, matrix='bt601', full_range=False):
    """surfaces: a list of n separately allocated [H0 * 3 // 2, pitch_i] uint8 NV12 device tensors of one H0 x width
    picture size (several cameras: each with its own pitch); `matrix` and `full_range` one value or one per
    surface -> (img [n, 3, Hp, Wp] fp32, img_meta): img[i] equals preprocess_clip_nv12(surfaces[i][None], ...)
    with surface i's settings bit for bit, the meta is that call's.  One launch per 32 surfaces
    (pave_preprocess_surfaces_nv12)."""
    surfaces = list(surfaces) if isinstance(surfaces, (list, tuple)) else None
    if not surfaces:
        raise ValueError('preprocess_surfaces_nv12: surfaces must be a non-empty list of [H0 * 3 // 2, pitch] tensors')
    n, W0 = len(surfaces), int(width)
    for i, s in enumerate(surfaces):
        if not (isinstance(s, torch.Tensor) and s.dim() == 2 and s.dtype == torch.uint8):
            raise ValueError(f'preprocess_surfaces_nv12: surfaces[{i}] must be a [H0 * 3 // 2, pitch] uint8 tensor')
    rows = surfaces[0].shape[0]
    H0 = rows * 2 // 3
    if rows % 3 != 0 or H0 % 2 != 0 or H0 <= 0:
        raise ValueError(f'preprocess_surfaces_nv12: {rows} rows are not the 3/2 of an even height')
    if W0 <= 0 or W0 % 2 != 0:
        raise ValueError(f'preprocess_surfaces_nv12: width {W0} must be even and positive')
    for i, s in enumerate(surfaces):
        if s.shape[0] != rows:
            raise ValueError(f'preprocess_surfaces_nv12: surfaces[{i}] has {s.shape[0]} rows, surfaces[0] {rows} '
                             '(one launch takes one source size)')
        if W0 > s.shape[1]:
            raise ValueError(f'preprocess_surfaces_nv12: width {W0} exceeds the pitch {s.shape[1]} of surfaces[{i}]')

    def per_surface(v, name, scalar):
        if isinstance(v, scalar):
            return [v] * n
        v = list(v)
        if len(v) != n:
            raise ValueError(f'preprocess_surfaces_nv12: {name} is one value or one per surface ({n}), got {len(v)}')
        return v
    cscs = [nv12_csc(m, bool(f)) for m, f in zip(per_surface(matrix, 'matrix', str),
                                                 per_surface(full_range, 'full_range', (bool, int)))]
    dev = surfaces[0].device
    _require(all(s.is_cuda and s.is_contiguous() and s.device == dev for s in surfaces),
             'preprocess_surfaces_nv12: surfaces must be contiguous tensors on one device')
    Hn, Wn, Hp, Wp, scale_factor = plan_clip(H0, W0, img_scale, size_divisor)
    out = torch.empty((n, 3, Hp, Wp), dtype=torch.float32, device=dev)
    m = (ctypes.c_float * 3)(*mean)
    s = (ctypes.c_float * 3)(*std)
    for at in range(0, n, native.INGEST_MAX_SURFACES):
        plan = native.IngestPlan()
        part = surfaces[at:at + native.INGEST_MAX_SURFACES]
        for i, surf in enumerate(part):
            plan.src[i] = surf.data_ptr()
            plan.pitch[i] = surf.shape[1]
            for j, c in enumerate(cscs[at + i]):
                plan.csc[i][j] = c
        plan.n = len(part)
        _launch('pave_preprocess_surfaces_nv12', 'preprocess_surfaces_nv12', dev, ctypes.byref(plan),
                out[at:].data_ptr(), H0, W0, Hn, Wn, Hp, Wp, ctypes.cast(m, ctypes.c_void_p),
                ctypes.cast(s, ctypes.c_void_p), int(bool(to_rgb)))
    meta = dict(ori_shape=(H0, W0, 3), img_shape=(Hn, Wn, 3), pad_shape=(Hp, Wp, 3),
                batch_input_shape=(Hp, Wp), scale_factor=scale_factor, flip=False, flip_direction=None)
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
