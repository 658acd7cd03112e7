"""Torch-facing wrappers of the HIP kernels (device tensors in, device tensors out).

Mirrors the reference operator surface for this path:

* ``ms_deform_attn_forward`` -- same name and keyword names as the pybind export
  ``mmcv._ext.ms_deform_attn_forward``
  (third_party/mmcv/mmcv/ops/csrc/pytorch/pybind.cpp:737-741);
* ``MultiScaleDeformableAttnFunction`` -- same ``apply`` signature as
  third_party/mmcv/mmcv/ops/multi_scale_deform_attn.py:20-57;
* ``deform_attn_grid_fused`` / ``deform_attn_pose_fused`` -- the fused T-frame
  launches that replace the per-frame softmax / location / sampling / fusion
  chain of MO:1388-1587 and OT:1644-1863.

PyTorch is used here only for device memory and the current HIP stream.  There
is no CPU path: a non-device tensor raises, exactly as the reference's
``AT_ASSERTM(value.is_cuda())`` does (ms_deform_attn_cuda.cu:221-230).
"""
import contextlib
import ctypes
import numbers

import torch

from . import native


# When set to a list, launches whose tag is in KERNEL_EVENT_TAGS append (tag, start_event,
# end_event, flops) recorded on the stream they launch on (bench.py times the dominant kernel this way
# inside its timed region; every other launch records nothing).
KERNEL_EVENTS = None
KERNEL_EVENT_TAGS = ('enc_tile', 'enc_grid_T1')
KERNEL_EVENT_SHAPES = None   # tools/gemm_census.py: a list that receives the shape note of every recorded launch


def _stream_ptr():
    return torch.cuda.current_stream().cuda_stream


# Form policy of the GEMM / convolution dispatchers (pave_set_form_policy, include/pave_hip.h): 0 = the selection
# by row count, 1 = tile order, 2 = K-split order where it applies.  Under 1 and 2 an output row is a function of
# its own input row only, whatever the batch (bricks.set_batch_invariant).
FORM_ROWS, FORM_ROWS_SPLITK, FORM_ROWS_TILE, FORM_LN, FORM_CONV3X3, FORM_CONV1X1S, FORM_ENCPROJ = (
    native.DEFINES['PAVE_FORM_' + n] for n in ('ROWS', 'ROWS_SPLITK', 'ROWS_TILE', 'LN', 'CONV3X3', 'CONV1X1S',
                                               'ENCPROJ'))
ORDER_TILE, ORDER_KSPLIT, ORDER_SPLITK, ORDER_TILE_LNPASS, ORDER_KSPLIT_LNPASS, ORDER_TILE_LN8 = (
    native.DEFINES['PAVE_ORDER_' + n] for n in ('TILE', 'KSPLIT', 'SPLITK', 'TILE_LNPASS', 'KSPLIT_LNPASS',
                                                'TILE_LN8'))


def current_form_policy():
    """The calling thread's form policy (the library keeps one per host thread: a batch-invariant forward on one
    Python thread leaves another thread's default-mode forward alone)."""
    return native.load().pave_get_form_policy()


@contextlib.contextmanager
def form_policy(p):
    """Run the block's launches under form policy p (0 | 1 | 2) on the calling thread; the previous policy is back on
    exit, on an exception too.  The policy is the library's at the time of entry: enter native.diag_build() first."""
    _require(p in (0, 1, 2), 'form_policy: 0, 1 or 2')
    lib = native.load()
    prev = lib.pave_get_form_policy()
    native.check(lib.pave_set_form_policy(int(p)), 'set_form_policy')
    try:
        yield
    finally:
        lib.pave_set_form_policy(prev)


def form_plan(M, K, N, kind=FORM_ROWS, policy=None, planes=3):
    """(order, ksplit) the dispatchers take for an [M, K] x [K, N] launch of `kind` (FORM_*) under `policy` (None:
    the current one): pave_form_plan, a pure host function."""
    lib = native.load()
    order, parts = ctypes.c_int(), ctypes.c_int()
    st = lib.pave_form_plan(int(M), int(K), int(N), int(kind), 16 if planes == PLANES_FP16 else int(planes),
                            current_form_policy() if policy is None else int(policy), ctypes.byref(order),
                            ctypes.byref(parts))
    native.check(st, 'form_plan')
    return order.value, parts.value


class _Timed:
    def __init__(self, tag, flops=0, shape=None):
        self.tag = tag if (KERNEL_EVENTS is not None and tag in KERNEL_EVENT_TAGS) else None
        self.flops = flops
        if self.tag is not None and KERNEL_EVENT_SHAPES is not None:
            KERNEL_EVENT_SHAPES.append(shape)

    def __enter__(self):
        if self.tag is not None:
            self.s = torch.cuda.Event(enable_timing=True)
            self.e = torch.cuda.Event(enable_timing=True)
            self.s.record()

    def __exit__(self, *a):
        if self.tag is not None:
            self.e.record()
            KERNEL_EVENTS.append((self.tag, self.s, self.e, self.flops))


SMALL_ROWS = 8192   # GEMM launches with fewer rows are latency-bound by shape (the decoders' few hundred
#                     query rows): timed under their own tag, reported beside the dominant class


def _gemm_tag(tag, M):
    return tag if M >= SMALL_ROWS else tag + '_small'


def _require(cond, msg):
    if not cond:
        raise RuntimeError(msg)


def _dev(t, name, dtype=None):
    _require(isinstance(t, torch.Tensor), f'{name} must be a tensor')
    _require(t.is_cuda, f'{name} must be a HIP device tensor (pavenet_amd has no CPU path)')
    _require(t.is_contiguous(), f'{name} tensor has to be contiguous')
    if dtype is not None:
        _require(t.dtype == dtype, f'{name} must be {dtype}, got {t.dtype}')
    return t


def _nhwc(x, who):
    _require(x.is_cuda and x.dtype == torch.float32 and x.dim() == 4, f'{who}: fp32 4-D')
    _require(x.is_contiguous(memory_format=torch.channels_last), f'{who}: channels_last input')


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _launch(entry, what, dev, *args, tag=None, flops=0, shape=None):
    """What every launch must meet, in one place: the entry point of include/pave_hip.h looked up on the library of
    the moment (native.diag_build() swaps it), called on `dev` with the current stream as its last argument, timed
    when `tag` is one bench.py asked for, and its status checked under the name `what`."""
    fn = getattr(native.load(), entry)
    with torch.cuda.device(dev), _Timed(tag, flops, shape):
        st = fn(*args, _stream_ptr())
    native.check(st, what)


PLANES_FP16 = native.DEFINES['PAVE_PLANES_FP16']   # one plane of fp16 operands


def _planes(w_planes, name='w_planes', fp16=False, only=None):
    """Checks a split-weight operand and returns the C ABI's `nplanes` for it: int16 tensors hold
    shape[1] bf16 planes, float16 tensors ONE plane of fp16 operands (split_weight_bf16x3(..., PLANES_FP16));
    `fp16=True` with an int16 single plane = the same bits under the old dtype.  only: allowed values."""
    # (one combined test on the way every launch takes; the messages are built on failure only)
    dt = w_planes.dtype if isinstance(w_planes, torch.Tensor) else None
    if not (dt in (torch.int16, torch.float16) and w_planes.is_cuda and w_planes.is_contiguous()
            and w_planes.dim() == 4 and w_planes.shape[3] == 16):
        _dev(w_planes, name)
        _require(dt in (torch.int16, torch.float16), f'{name} must be int16 (bf16 planes) or float16 (fp16 plane)')
        _require(False, f'{name}: [K/16, planes, N, 16] (split_weight_bf16x3)')
    n = w_planes.shape[1]
    if dt == torch.float16 or fp16:
        _require(n == 1, f'{name}: fp16 operands are a single plane')
        n = PLANES_FP16
    if only is not None and n not in only:
        _require(False, f'{name}: this entry point takes 3 bf16 planes or one fp16 plane')
    return n


_Q_PLANES = (3, PLANES_FP16)   # the modes of the LDS-DMA generation (every fused form)


def ms_deform_attn_forward(value, value_spatial_shapes, value_level_start_index,
                           sampling_locations, attention_weights, im2col_step=64):
    """[R1] value [bs,S,M,D], shapes [L,2] i64, lsi [L] i64, loc [bs,Lq,M,L,P,2],
    weights [bs,Lq,M,L,P] -> [bs, Lq, M*D]."""
    _require(value.dtype in (torch.float32, torch.float64),
             'ms_deform_attn_forward: value must be float32 or float64')
    dt = value.dtype
    _dev(value, 'value', dt)
    _dev(value_spatial_shapes, 'spatial_shapes', torch.int64)
    _dev(value_level_start_index, 'level_start_index', torch.int64)
    _dev(sampling_locations, 'sampling_loc', dt)
    _dev(attention_weights, 'attn_weight', dt)
    _require(value.dim() == 4 and sampling_locations.dim() == 6 and attention_weights.dim() == 5,
             'ms_deform_attn_forward: bad tensor ranks')
    bs, S, M, D = value.shape
    _, Lq, M2, L, P, two = sampling_locations.shape
    _require(M2 == M and two == 2 and sampling_locations.shape[0] == bs,
             'ms_deform_attn_forward: sampling_loc shape mismatch')
    _require(tuple(attention_weights.shape) == (bs, Lq, M, L, P),
             'ms_deform_attn_forward: attn_weight shape mismatch')
    _require(tuple(value_spatial_shapes.shape) == (L, 2) and
             tuple(value_level_start_index.shape) == (L,),
             'ms_deform_attn_forward: spatial_shapes / level_start_index shape mismatch')
    out = torch.empty((bs, Lq, M * D), dtype=dt, device=value.device)
    if out.numel() == 0:   # no queries (or empty batch): empty result, as the PyTorch formulation
        return out         # (MO:92-149) gives; the C entry point rejects non-positive sizes
    _launch('pave_ms_deform_attn_forward_f32' if dt == torch.float32 else 'pave_ms_deform_attn_forward_f64',
            'ms_deform_attn_forward', value.device,
            value.data_ptr(), value_spatial_shapes.data_ptr(),
            value_level_start_index.data_ptr(), sampling_locations.data_ptr(),
            attention_weights.data_ptr(), out.data_ptr(), bs, S, M, D, L, Lq, P,
            int(im2col_step))
    return out


def ms_deform_attn_backward(value, value_spatial_shapes, value_level_start_index,
                            sampling_locations, attention_weights, grad_output, grad_value,
                            grad_sampling_loc, grad_attn_weight, im2col_step=64):
    """Same positional / keyword surface as ``mmcv._ext.ms_deform_attn_backward``
    (pybind.cpp:743-748): grad_value is accumulated into, the other two are overwritten."""
    dt = value.dtype
    _require(dt in (torch.float32, torch.float64), 'ms_deform_attn_backward: fp32 / fp64 only')
    for t, n in ((value, 'value'), (sampling_locations, 'sampling_loc'),
                 (attention_weights, 'attn_weight'), (grad_output, 'grad_output'),
                 (grad_value, 'grad_value'), (grad_sampling_loc, 'grad_sampling_loc'),
                 (grad_attn_weight, 'grad_attn_weight')):
        _dev(t, n, dt)
    _dev(value_spatial_shapes, 'spatial_shapes', torch.int64)
    _dev(value_level_start_index, 'level_start_index', torch.int64)
    bs, S, M, D = value.shape
    _, Lq, _, L, P, _ = sampling_locations.shape
    _require(grad_output.numel() == bs * Lq * M * D and grad_value.shape == value.shape and
             grad_sampling_loc.shape == sampling_locations.shape and
             grad_attn_weight.shape == attention_weights.shape,
             'ms_deform_attn_backward: gradient shapes mismatch')
    if grad_output.numel() == 0:   # no queries: nothing to add (the forward's empty result, as _ext does)
        return
    _launch('pave_ms_deform_attn_backward_f32' if dt == torch.float32 else 'pave_ms_deform_attn_backward_f64',
            'ms_deform_attn_backward', value.device,
            value.data_ptr(), value_spatial_shapes.data_ptr(),
            value_level_start_index.data_ptr(), sampling_locations.data_ptr(),
            attention_weights.data_ptr(), grad_output.data_ptr(), grad_value.data_ptr(),
            grad_sampling_loc.data_ptr(), grad_attn_weight.data_ptr(), bs, S, M, D, L, Lq, P,
            int(im2col_step))


class MultiScaleDeformableAttnFunction(torch.autograd.Function):
    """Same ``apply(value, shapes, lsi, loc, weights, im2col_step)`` and gradients as MO:20-89."""

    @staticmethod
    def forward(ctx, value, value_spatial_shapes, value_level_start_index,
                sampling_locations, attention_weights, im2col_step):
        ctx.im2col_step = im2col_step
        out = ms_deform_attn_forward(
            value, value_spatial_shapes, value_level_start_index,
            sampling_locations, attention_weights, im2col_step=im2col_step)
        ctx.save_for_backward(value, value_spatial_shapes, value_level_start_index,
                              sampling_locations, attention_weights)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_output):
        value, shapes, lsi, loc, aw = ctx.saved_tensors
        grad_value = torch.zeros_like(value)
        grad_loc = torch.zeros_like(loc)
        grad_aw = torch.zeros_like(aw)
        ms_deform_attn_backward(value, shapes, lsi, loc, aw, grad_output.contiguous(), grad_value,
                                grad_loc, grad_aw, im2col_step=ctx.im2col_step)
        return grad_value, None, None, grad_loc, grad_aw, None


def _level_rows(ref, L, name):
    """(dense tensor, ref_levels) of a reference tensor [.., L, c]: a level axis that is a broadcast
    (`reference_points[:, :, None].expand(..)`, stride 0: un-padded batches) is passed as ONE row per entry
    (ref_levels = 1, no materialised copy); anything else must be dense with L rows."""
    if ref.dim() >= 2 and ref.shape[-2] == L and L > 1 and ref.stride(-2) == 0:
        base = ref.select(-2, 0)
        if base.is_contiguous():
            return base, 1
        ref = ref.contiguous()
    _dev(ref, name, torch.float32)
    return ref, L


def deform_attn_grid_fused(value, spatial_shapes, level_start_index, proj, ref, *, T,
                           n_clips, units_per_clip, unit_clip=None, order=None,
                           return_stats=False, frame_table=None):
    """Fused grid-offset deformable attention over T frames ([R2] with T=1, [R4]).

    value [n_clips*T, S, 8, 32]; proj [n_units, >= T*8*16*3]; ref [T, n_units, 4, 2]
    -> out [n_units, 256] (+ (max, sum) [n_units, 8] if return_stats).
    Differentiable in value / proj / ref (pavenet_amd/fused_autograd.py).
    """
    if torch.is_grad_enabled() and not return_stats and \
            (value.requires_grad or proj.requires_grad or ref.requires_grad):
        from .fused_autograd import GridFusedFunction
        _require(frame_table is None, 'deform_attn_grid_fused: frame_table is an inference-only option')
        return GridFusedFunction.apply(value, spatial_shapes, level_start_index, proj, ref, T,
                                       n_clips, units_per_clip, unit_clip, order)
    f32 = torch.float32
    _dev(value, 'value', f32)
    _dev(spatial_shapes, 'spatial_shapes', torch.int64)
    _dev(level_start_index, 'level_start_index', torch.int64)
    _dev(proj, 'proj', f32)
    _require(ref.is_cuda and ref.dtype == f32, 'deform_attn_grid_fused: ref fp32 on the device')
    _require(value.dim() == 4 and value.shape[2] == 8 and value.shape[3] == 32,
             'deform_attn_grid_fused: value must be [frames, S, 8, 32]')
    if frame_table is not None:   # value = per-frame cache, slab of (clip, t) = frame_table[clip*T + t]
        # (entries must be < value.shape[0]: checked where the table is built, streaming.decode; the
        # kernel clamps every slab index into the value tensor, so a bad table cannot fault)
        _dev(frame_table, 'frame_table', torch.int32)
        _require(frame_table.numel() == n_clips * T, 'deform_attn_grid_fused: frame_table [n_clips*T]')
    else:
        _require(value.shape[0] == n_clips * T, 'deform_attn_grid_fused: value frames != n_clips*T')
    S = value.shape[1]
    L = spatial_shapes.shape[0]
    _require(proj.dim() == 2, 'deform_attn_grid_fused: proj must be 2-D')
    n_units = proj.shape[0]
    _require(tuple(ref.shape) == (T, n_units, L, 2),
             f'deform_attn_grid_fused: ref must be [T, n_units, L, 2], got {tuple(ref.shape)}')
    ref, ref_levels = _level_rows(ref, L, 'ref')
    if unit_clip is not None:
        _dev(unit_clip, 'unit_clip', torch.int32)
        _require(unit_clip.numel() == n_units, 'deform_attn_grid_fused: unit_clip length')
    if order is not None:
        _dev(order, 'order', torch.int32)
        _require(order.numel() == n_units, 'deform_attn_grid_fused: order length')
    out = torch.empty((n_units, 256), dtype=f32, device=value.device)
    smax = ssum = None
    if return_stats:
        smax = torch.empty((n_units, 8), dtype=f32, device=value.device)
        ssum = torch.empty((n_units, 8), dtype=f32, device=value.device)
    tag = 'enc_grid_T1' if (T == 1 and unit_clip is None) else f'grid_T{T}'
    _launch('pave_deform_attn_grid_fused_f32', 'deform_attn_grid_fused', value.device,
            value.data_ptr(), spatial_shapes.data_ptr(), level_start_index.data_ptr(),
            proj.data_ptr(), ref.data_ptr(), _ptr(unit_clip), _ptr(order), out.data_ptr(),
            _ptr(smax), _ptr(ssum), n_units, int(units_per_clip),
            int(n_clips), int(T), S, L, 4, proj.stride(0),
            _ptr(frame_table), int(value.shape[0]), ref_levels, tag=tag)
    if return_stats:
        return out, smax, ssum
    return out


def deform_attn_pose_fused(value, spatial_shapes, level_start_index, proj, ref, *, T,
                           n_clips, num_query, num_keypoints, return_stats=False, frame_table=None):
    """Fused pose-aware deformable attention over T frames ([R3]).

    value [n_clips*T, S, 8, 32]; proj [n_clips*Q, >= T*8*L*K*3];
    ref [n_clips, T*Q, L, 2K] -> out [n_clips*Q, 256].
    Differentiable in value / proj / ref (pavenet_amd/fused_autograd.py).
    """
    if torch.is_grad_enabled() and not return_stats and \
            (value.requires_grad or proj.requires_grad or ref.requires_grad):
        from .fused_autograd import PoseFusedFunction
        _require(frame_table is None, 'deform_attn_pose_fused: frame_table is an inference-only option')
        return PoseFusedFunction.apply(value, spatial_shapes, level_start_index, proj, ref, T,
                                       n_clips, int(num_query), int(num_keypoints))
    f32 = torch.float32
    _dev(value, 'value', f32)
    _dev(spatial_shapes, 'spatial_shapes', torch.int64)
    _dev(level_start_index, 'level_start_index', torch.int64)
    _dev(proj, 'proj', f32)
    _require(ref.is_cuda and ref.dtype == f32, 'deform_attn_pose_fused: ref fp32 on the device')
    _require(value.dim() == 4 and value.shape[2] == 8 and value.shape[3] == 32,
             'deform_attn_pose_fused: value must be [frames, S, 8, 32]')
    if frame_table is not None:
        _dev(frame_table, 'frame_table', torch.int32)
        _require(frame_table.numel() == n_clips * T, 'deform_attn_pose_fused: frame_table [n_clips*T]')
    else:
        _require(value.shape[0] == n_clips * T, 'deform_attn_pose_fused: value frames != n_clips*T')
    S = value.shape[1]
    L = spatial_shapes.shape[0]
    Q, K = int(num_query), int(num_keypoints)
    _require(proj.dim() == 2 and proj.shape[0] == n_clips * Q,
             'deform_attn_pose_fused: proj must be [n_clips*Q, cols]')
    _require(ref.numel() == n_clips * T * Q * L * 2 * K and ref.shape[-2:] == (L, 2 * K),
             'deform_attn_pose_fused: ref must be [n_clips, T*Q, L, 2K]')
    ref, ref_levels = _level_rows(ref, L, 'ref')
    out = torch.empty((n_clips * Q, 256), dtype=f32, device=value.device)
    smax = ssum = None
    if return_stats:
        smax = torch.empty((n_clips * Q, 8), dtype=f32, device=value.device)
        ssum = torch.empty((n_clips * Q, 8), dtype=f32, device=value.device)
    _launch('pave_deform_attn_pose_fused_f32', 'deform_attn_pose_fused', value.device,
            value.data_ptr(), spatial_shapes.data_ptr(), level_start_index.data_ptr(),
            proj.data_ptr(), ref.data_ptr(), out.data_ptr(), _ptr(smax), _ptr(ssum),
            int(n_clips), Q, int(T), S, L, K, proj.stride(0), _ptr(frame_table),
            int(value.shape[0]), ref_levels, tag=f'pose_T{T}')
    if return_stats:
        return out, smax, ssum
    return out


def oks_nms(kpts, scores, sigmas, thresh):
    """Device OKS-NMS (HEAD:1624-1665).  kpts [n_clips, N, K, 3], scores [n_clips, N],
    sigmas [K] float64 -> (keep [n_clips, N] int32, order [n_clips, N] int32)."""
    _dev(kpts, 'kpts', torch.float32)
    _dev(scores, 'scores', torch.float32)
    _dev(sigmas, 'sigmas', torch.float64)
    _require(kpts.dim() == 4 and kpts.shape[-1] == 3, 'oks_nms: kpts must be [n_clips, N, K, 3]')
    n_clips, N, K, _ = kpts.shape
    _require(tuple(scores.shape) == (n_clips, N) and sigmas.numel() == K,
             'oks_nms: scores / sigmas shape mismatch')
    keep = torch.empty((n_clips, N), dtype=torch.int32, device=kpts.device)
    order = torch.empty((n_clips, N), dtype=torch.int32, device=kpts.device)
    if keep.numel() == 0:  # nothing to suppress (the NumPy loop of HEAD:1624-1665 returns [])
        return keep, order
    _launch('pave_oks_nms_f32', 'oks_nms', kpts.device, kpts.data_ptr(), scores.data_ptr(), sigmas.data_ptr(),
            float(thresh), keep.data_ptr(), order.data_ptr(), n_clips, N, K)
    return keep, order


NMS_METHODS = {'nms': 0, 'naive': 1, 'linear': 2, 'gaussian': 3}   # include/pave_hip.h pave_aug_merge_nms_f32


def aug_merge_nms(bboxes, kpts, keeps, flips, img_w, scale_factor, flip_perm, *, score_thr, max_num,
                  method='linear', iou_thr=0.5, sigma=0.5, min_score=1e-3, offset=0):
    """Test-time augmentation merge + box NMS in one launch (pave_aug_merge_nms_f32).

    bboxes / kpts / keeps: one entry per augmentation -- [B, N, 5], [B, N, K, 3] fp32 and [B, N] int32 (or None:
    every row enters); flips [A] bools; img_w [A][B] and scale_factor [A][B][4] host numbers; flip_perm [K] ints.
    method: 'nms' (hard) or the soft-NMS kinds 'naive' / 'linear' / 'gaussian'.
    -> dict(dets [B, M, 5], labels [B, M] int64, kpts [B, M, K, 3], inds [B, M] int64, keep [B, M] int32,
    count [B] int32), M = min(max_num, A N) (A N when max_num <= 0); rows past count[b] have keep 0 and inds -1."""
    A = len(bboxes)
    _require(0 < A <= native.AUG_MAX_AUGS, f'aug_merge_nms: 1 .. {native.AUG_MAX_AUGS} augmentations, got {A}')
    _require(len(kpts) == A and len(keeps) == A and len(flips) == A and len(img_w) == A and
             len(scale_factor) == A, 'aug_merge_nms: one bboxes / kpts / keep / flip / img_w / scale_factor '
             'entry per augmentation')
    _require(method in NMS_METHODS, f'aug_merge_nms: method must be one of {sorted(NMS_METHODS)}, got {method!r}')
    _require(int(offset) in (0, 1), 'aug_merge_nms: offset 0 or 1')
    for a in range(A):
        _dev(bboxes[a], f'bboxes[{a}]', torch.float32)
        _dev(kpts[a], f'kpts[{a}]', torch.float32)
        if keeps[a] is not None:
            _dev(keeps[a], f'keep[{a}]', torch.int32)
    B, N = bboxes[0].shape[:2]
    K = kpts[0].shape[2]
    dev = bboxes[0].device
    for a in range(A):
        _require(tuple(bboxes[a].shape) == (B, N, 5) and tuple(kpts[a].shape) == (B, N, K, 3),
                 'aug_merge_nms: every augmentation needs bboxes [B, N, 5] and kpts [B, N, K, 3] of one shape')
        _require(keeps[a] is None or tuple(keeps[a].shape) == (B, N), 'aug_merge_nms: keep must be [B, N]')
        _require(bboxes[a].device == dev and kpts[a].device == dev and (keeps[a] is None or keeps[a].device == dev),
                 'aug_merge_nms: all inputs on one device')
        _require(len(img_w[a]) == B and len(scale_factor[a]) == B, 'aug_merge_nms: img_w / scale_factor [A][B]')
    _require(A * B <= native.AUG_MAX_SLOTS, f'aug_merge_nms: at most {native.AUG_MAX_SLOTS} (augmentation, image) '
             'pairs per launch')
    _require(A * N <= 4096, f'aug_merge_nms: {A} x {N} = {A * N} boxes per image; the kernel keeps at most 4096 '
             'in LDS')
    _require(K <= native.AUG_MAX_K and len(flip_perm) == K and sorted(int(v) for v in flip_perm) == list(range(K)),
             f'aug_merge_nms: flip_perm must be a permutation of range(K), K <= {native.AUG_MAX_K}')
    plan = native.AugPlan()
    for a in range(A):
        plan.bboxes[a] = bboxes[a].data_ptr()
        plan.kpts[a] = kpts[a].data_ptr()
        plan.keep[a] = _ptr(keeps[a])
        plan.flip[a] = int(bool(flips[a]))
        for b in range(B):
            plan.img_w[a * B + b] = float(img_w[a][b])
            sf = [float(v) for v in scale_factor[a][b]]
            _require(len(sf) == 4, 'aug_merge_nms: scale_factor entries have 4 values')
            for i in range(4):
                plan.scale_factor[a * B + b][i] = sf[i]
    for k in range(K):
        plan.flip_perm[k] = int(flip_perm[k])
    plan.n_aug, plan.B, plan.N, plan.K = A, B, N, K
    total = A * N
    M = min(int(max_num), total) if int(max_num) > 0 else total
    dets = torch.empty((B, M, 5), dtype=torch.float32, device=dev)
    labels = torch.empty((B, M), dtype=torch.int64, device=dev)
    out_k = torch.empty((B, M, K, 3), dtype=torch.float32, device=dev)
    inds = torch.empty((B, M), dtype=torch.int64, device=dev)
    keep = torch.empty((B, M), dtype=torch.int32, device=dev)
    count = torch.empty((B,), dtype=torch.int32, device=dev)
    _launch('pave_aug_merge_nms_f32', 'aug_merge_nms', dev, ctypes.byref(plan), float(score_thr), int(max_num),
            NMS_METHODS[method], float(iou_thr), float(sigma), float(min_score), int(offset),
            dets.data_ptr(), labels.data_ptr(), out_k.data_ptr(), inds.data_ptr(),
            keep.data_ptr(), count.data_ptr())
    return dict(dets=dets, labels=labels, kpts=out_k, inds=inds, keep=keep, count=count)


def hflip_canvas(x, valid_w):
    """Horizontal flip of preprocessed canvases x [n, C, Hp, Wp] fp32 (pave_hflip_canvas_f32), out of place:
    columns [0, w) of image i mirrored within themselves, w = valid_w (an int for all images, or a device int32
    tensor [n]); the padding columns from w on are copied unchanged."""
    _dev(x, 'x', torch.float32)
    _require(x.dim() == 4, 'hflip_canvas: x must be [n, C, Hp, Wp]')
    n, C, Hp, Wp = x.shape
    if isinstance(valid_w, torch.Tensor):
        _dev(valid_w, 'valid_w', torch.int32)
        _require(valid_w.numel() == n and valid_w.device == x.device, 'hflip_canvas: valid_w [n] on x\'s device')
        w_ptr, w_all = valid_w.data_ptr(), 0
    else:
        _require(0 <= int(valid_w) <= Wp, 'hflip_canvas: 0 <= valid_w <= Wp')
        w_ptr, w_all = None, int(valid_w)
    y = torch.empty_like(x)
    if x.numel() == 0:
        return y
    _launch('pave_hflip_canvas_f32', 'hflip_canvas', x.device, x.data_ptr(), y.data_ptr(), w_ptr, w_all, n, C, Hp, Wp)
    return y


def scatter_rows(srcs, dsts, rows):
    """dsts[t][rows[i]] = srcs[t][i] for every tensor pair t and source row i, in one launch per 64 rows
    (pave_scatter_rows_f32; the live ring's write).  srcs[t] [n, ...] and dsts[t] [dst_rows, ...] are contiguous fp32
    device tensors, all with the same number of elements per row (a multiple of 4) and 16-byte aligned; `rows` are n
    distinct ints in [0, dst_rows).  A plain copy: bit-identical to the indexed assignment."""
    K, N = native.SCATTER_MAX_TENSORS, native.SCATTER_MAX_ROWS
    srcs, dsts, rows = list(srcs), list(dsts), [int(r) for r in rows]
    if not 0 < len(srcs) <= K or len(dsts) != len(srcs):
        raise ValueError(f'scatter_rows: 1 .. {K} (src, dst) tensor pairs, got {len(srcs)} and {len(dsts)}')
    if not all(isinstance(x, torch.Tensor) and x.dim() >= 2 and x.dtype == torch.float32 for x in srcs + dsts):
        raise ValueError('scatter_rows: srcs and dsts are fp32 tensors of [rows, ...]')
    n, dst_rows, row_elems = len(rows), dsts[0].shape[0], srcs[0][0].numel() if srcs[0].shape[0] else 0
    if n == 0 or len(set(rows)) != n:
        raise ValueError('scatter_rows: `rows` are 1 or more distinct destination rows')
    if min(rows) < 0 or max(rows) >= dst_rows:
        raise ValueError(f'scatter_rows: rows must lie in [0, {dst_rows})')
    if row_elems < 4 or row_elems % 4 != 0:
        raise ValueError(f'scatter_rows: {row_elems} elements per row, a positive multiple of 4 is needed')
    for t, (s, d) in enumerate(zip(srcs, dsts)):
        for x, name, lead in ((s, f'srcs[{t}]', n), (d, f'dsts[{t}]', dst_rows)):
            if x.shape[0] != lead or x.numel() != lead * row_elems:
                raise ValueError(f'scatter_rows: {name} must hold {lead} rows of {row_elems} elements, '
                                 f'got {tuple(x.shape)}')
            if x.data_ptr() % 16 != 0:
                raise ValueError(f'scatter_rows: {name} is not 16-byte aligned')
    dev = dsts[0].device
    for t, x in enumerate(srcs + dsts):
        _dev(x, f'tensor {t}', torch.float32)
        _require(x.device == dev, 'scatter_rows: all tensors on one device')
    for at in range(0, n, N):
        part = rows[at:at + N]
        plan = native.ScatterPlan()
        for t, (s, d) in enumerate(zip(srcs, dsts)):
            plan.src[t] = s.data_ptr() + at * row_elems * 4
            plan.dst[t] = d.data_ptr()
        for i, r in enumerate(part):
            plan.row[i] = r
        plan.n, plan.k, plan.dst_rows, plan.row_elems = len(part), len(srcs), dst_rows, row_elems
        _launch('pave_scatter_rows_f32', 'scatter_rows', dev, ctypes.byref(plan))


def _draw_shapes(who, kind, items, colors, edges, K, thickness, radius):
    """The checks of shapes, types and ranges draw_poses and draw_tracks share (an item's first seven entries), all
    ValueError -> (items, edges, K, geometry, the tables' bytes)."""
    if kind not in ('nv12', 'bgr'):
        raise ValueError(f"{who}: kind {kind!r} is not 'nv12' or 'bgr'")
    items, edges, K = list(items), [(int(a), int(b)) for a, b in edges], int(K)
    if not 1 <= K <= native.DRAW_MAX_K or len(edges) > native.DRAW_MAX_E:
        raise ValueError(f'{who}: K in 1 .. {native.DRAW_MAX_K} and at most {native.DRAW_MAX_E} edges, got K = {K} '
                         f'and {len(edges)} edges')
    if any(not (0 <= a < K and 0 <= b < K) for a, b in edges):
        raise ValueError(f'{who}: an edge index outside [0, {K})')
    if not 1 <= int(thickness) <= 32 or not 0 <= int(radius) <= 32:
        raise ValueError(f'{who}: thickness in 1 .. 32 and radius in 0 .. 32, got {thickness} and {radius}')
    try:   # (a table may come as the 195 bytes themselves: PoseStyle caches them)
        colors = [tab if isinstance(tab, bytes) else bytes(int(c) for row in tab for c in (row if len(row) == 3 else ()))
                  for tab in colors]
    except (TypeError, ValueError):
        colors = []
    if not 1 <= len(colors) <= native.DRAW_MAX_TABLES or any(len(tab) != 3 * native.DRAW_COLORS for tab in colors):
        raise ValueError(f'{who}: colors are 1 .. {native.DRAW_MAX_TABLES} tables of {native.DRAW_COLORS} x 3 bytes')
    return items, edges, K, _surface_geometry(who, kind, items, K, len(colors)), b''.join(colors)   # [tables][65][3]


def _surface_geometry(who, kind, items, K, tables, table_name='colour table'):
    """The checks of an item's first seven entries (surface, width, kpts, bboxes, keep, (sx, sy), table), all
    ValueError -> [(pitch, W, H, N, sx, sy, table)]."""
    if not items:
        raise ValueError(f'{who}: no surface')
    geometry = []
    for i, it in enumerate(items):
        surf, width, kpts, bboxes, keep, scale, table = it[:7]
        if not (isinstance(surf, torch.Tensor) and surf.dtype == torch.uint8):
            raise ValueError(f'{who}: surface {i} must be a uint8 tensor')
        if kind == 'nv12':
            if surf.dim() != 2:
                raise ValueError(f'{who}: surface {i} must be [H * 3 // 2, pitch], got {tuple(surf.shape)}')
            rows, pitch = surf.shape
            H, W, row_bytes = rows * 2 // 3, int(width), int(width)
            if rows % 3 != 0 or H % 2 != 0 or H <= 0:
                raise ValueError(f'{who}: surface {i}: {rows} rows are not the 3/2 of an even height')
            if W <= 0 or W % 2 != 0:
                raise ValueError(f'{who}: surface {i}: width {W} must be even and positive')
        else:
            if surf.dim() != 3 or surf.shape[2] != 3 or surf.shape[0] < 1 or surf.shape[1] < 1:
                raise ValueError(f'{who}: surface {i} must be [H, W, 3], got {tuple(surf.shape)}')
            H, W = surf.shape[:2]
            pitch = row_bytes = 3 * W
        if row_bytes > pitch:
            raise ValueError(f'{who}: surface {i}: width {W} exceeds the pitch {pitch}')
        if W > native.DRAW_MAX_SIZE or H > native.DRAW_MAX_SIZE:
            raise ValueError(f'{who}: surface {i}: {W} x {H} exceeds {native.DRAW_MAX_SIZE} x {native.DRAW_MAX_SIZE}')
        if not (isinstance(kpts, torch.Tensor) and kpts.dtype == torch.float32 and kpts.dim() == 3
                and tuple(kpts.shape[1:]) == (K, 3)):
            raise ValueError(f'{who}: kpts of surface {i} must be a [N, {K}, 3] float32 tensor')
        N = kpts.shape[0]
        if not (isinstance(bboxes, torch.Tensor) and bboxes.dtype == torch.float32 and tuple(bboxes.shape) == (N, 5)):
            raise ValueError(f'{who}: bboxes of surface {i} must be a [{N}, 5] float32 tensor')
        if keep is not None and not (isinstance(keep, torch.Tensor) and keep.dtype == torch.int32
                                     and tuple(keep.shape) == (N,)):
            raise ValueError(f'{who}: keep of surface {i} must be a [{N}] int32 tensor')
        if N > native.DRAW_MAX_POSES:
            raise ValueError(f'{who}: surface {i} has {N} poses, at most {native.DRAW_MAX_POSES}')
        sx, sy = (float(v) for v in scale)
        if not (0 < sx < float('inf') and 0 < sy < float('inf')):
            raise ValueError(f'{who}: the scale of surface {i} must be positive and finite, got {(sx, sy)}')
        if not 0 <= int(table) < tables:
            raise ValueError(f'{who}: surface {i} names {table_name} {table} of {tables}')
        geometry.append((int(pitch), int(W), int(H), N, sx, sy, int(table)))
    return geometry


def _draw_device(who, items):
    """Where the tensors of checked items live: one HIP device."""
    dev = items[0][0].device
    for i, it in enumerate(items):
        for t, name in ((it[0], 'surface'), (it[2], 'kpts'), (it[3], 'bboxes'), (it[4], 'keep')):
            if t is not None:
                _dev(t, f'{who}: {name} of surface {i}')
                _require(t.device == dev, f'{who}: all tensors on one device')
    return dev


def _draw_fill(plan, part, geometry, raw_colors, edges, K, thickness, radius, score_thr, kpt_thr, draw_boxes):
    """A pave_draw_plan for the surfaces `part`."""
    for i, it in enumerate(part):
        pitch, W, H, N, sx, sy, table = geometry[i]
        plan.dst[i], plan.kpts[i], plan.bboxes[i], plan.keep[i] = it[0].data_ptr(), it[2].data_ptr(), \
            it[3].data_ptr(), _ptr(it[4])
        plan.pitch[i], plan.width[i], plan.height[i], plan.n_poses[i] = pitch, W, H, N
        plan.scale[i][0], plan.scale[i][1], plan.table[i] = sx, sy, table
    ctypes.memmove(plan.color, raw_colors, len(raw_colors))
    for e, (a, b) in enumerate(edges):
        plan.edge[e][0], plan.edge[e][1] = a, b
    plan.n, plan.K, plan.E, plan.thickness, plan.radius = len(part), K, len(edges), int(thickness), int(radius)
    plan.draw_boxes, plan.score_thr, plan.kpt_thr = int(bool(draw_boxes)), float(score_thr), float(kpt_thr)


def draw_poses(kind, items, colors, edges, K, *, thickness=4, radius=4, score_thr=0.3, kpt_thr=0., draw_boxes=False):
    """Poses drawn into surfaces in place, one launch per 32 surfaces (pave_draw_poses_nv12 / _bgr; the rule is
    DESIGN section 13).  kind 'nv12': a surface is a [H * 3 // 2, pitch] uint8 tensor whose first `width` columns are
    the picture; 'bgr': a [H, W, 3] uint8 tensor (`width` is not read).  items: one (surface, width, kpts [N, K, 3]
    fp32, bboxes [N, 5] fp32, keep [N] int32 or None, (sx, sy), table) per surface; colors [tables <= 4, 65, 3] bytes
    stored as they are (row 0 boxes, 1 .. 32 limbs, 33 .. 64 key points; a table nested or as its 195 bytes); edges: E <= 32 pairs of key-point indices.
    Shapes, types and ranges raise ValueError before anything is asked of a device."""
    items, edges, K, geometry, raw_colors = _draw_shapes('draw_poses', kind, items, colors, edges, K, thickness, radius)
    dev = _draw_device('draw_poses', items)
    entry = 'pave_draw_poses_nv12' if kind == 'nv12' else 'pave_draw_poses_bgr'
    for at in range(0, len(items), native.DRAW_MAX_SURFACES):
        plan = native.DrawPlan()
        part = items[at:at + native.DRAW_MAX_SURFACES]
        _draw_fill(plan, part, geometry[at:at + len(part)], raw_colors, edges, K, thickness, radius, score_thr, kpt_thr,
                   draw_boxes)
        _launch(entry, 'draw_poses', dev, ctypes.byref(plan))


def draw_tracks(kind, items, colors, palettes, font, edges, K, *, label_scale=2, untracked='style', thickness=4,
                radius=4, score_thr=0.3, kpt_thr=0., draw_boxes=False):
    """draw_poses with track ids in the picture, one launch per 32 surfaces (pave_draw_tracks_nv12 / _bgr; DESIGN
    section 13, "Track ids in the picture").  items: draw_poses' seven entries and `ids`: a contiguous int32 [N]
    tensor on the surface's device (what PoseTracker.update returns), or None for a surface drawn as draw_poses
    draws it.  palettes: one per colour table, 33 x 3 bytes stored as they are (rows 0 .. 31: id v takes row
    (v - 1) % 32; row 32: the digits' ink; nested or as the 99 bytes); font: 10 digits x 7 rows of 5 bits (bit 4 the
    left-most pixel); label_scale 0 .. 8 (0: colours only); untracked 'style' | 'skip': a pose with id <= 0 is drawn
    as draw_poses draws it, or not at all.  Shapes, types and ranges raise ValueError before anything is asked of a
    device."""
    who = 'draw_tracks'
    items = list(items)
    if any(not (isinstance(it, (tuple, list)) and len(it) == 8) for it in items):
        raise ValueError(f'{who}: an item is (surface, width, kpts, bboxes, keep, (sx, sy), table, ids)')
    if isinstance(label_scale, bool) or not isinstance(label_scale, int) or not 0 <= label_scale <= 8:
        raise ValueError(f'{who}: label_scale is an integer in 0 .. 8, got {label_scale!r}')
    if untracked not in ('style', 'skip'):
        raise ValueError(f"{who}: untracked {untracked!r} is not 'style' or 'skip'")
    try:
        font = [[int(r) for r in rows] for rows in font]
    except (TypeError, ValueError):
        font = []
    if len(font) != 10 or any(len(rows) != 7 or any(not 0 <= r < 32 for r in rows) for rows in font):
        raise ValueError(f'{who}: font is 10 digits of 7 rows of 5 bits')
    rows = native.DRAW_PALETTE + 1
    try:
        palettes = [tab if isinstance(tab, bytes) else bytes(int(c) for row in tab for c in (row if len(row) == 3 else ()))
                    for tab in palettes]
    except (TypeError, ValueError):
        palettes = []
    if not 1 <= len(palettes) <= native.DRAW_MAX_TABLES or any(len(tab) != 3 * rows for tab in palettes):
        raise ValueError(f'{who}: palettes are 1 .. {native.DRAW_MAX_TABLES} tables of {rows} x 3 bytes')
    items, edges, K, geometry, raw_colors = _draw_shapes(who, kind, items, colors, edges, K, thickness, radius)
    if len(palettes) != len(raw_colors) // (3 * native.DRAW_COLORS):
        raise ValueError(f'{who}: one palette per colour table ({len(raw_colors) // (3 * native.DRAW_COLORS)}), got '
                         f'{len(palettes)}')
    for i, it in enumerate(items):
        ids, N = it[7], geometry[i][3]
        if ids is None:
            continue
        if not (isinstance(ids, torch.Tensor) and ids.dtype == torch.int32 and tuple(ids.shape) == (N,)):
            raise ValueError(f'{who}: ids of surface {i} must be a [{N}] int32 tensor or None')
        if not ids.is_contiguous():
            raise ValueError(f'{who}: ids of surface {i} must be contiguous')
        if ids.device != it[0].device:
            raise ValueError(f'{who}: ids of surface {i} are on {ids.device}, the surface on {it[0].device}')
    dev = _draw_device(who, items)
    entry = 'pave_draw_tracks_nv12' if kind == 'nv12' else 'pave_draw_tracks_bgr'
    raw_palettes, raw_font = b''.join(palettes), bytes(r for rows in font for r in rows)
    for at in range(0, len(items), native.DRAW_MAX_SURFACES):
        plan = native.DrawIdsPlan()
        part = items[at:at + native.DRAW_MAX_SURFACES]
        _draw_fill(plan.base, part, geometry[at:at + len(part)], raw_colors, edges, K, thickness, radius, score_thr,
                   kpt_thr, draw_boxes)
        for i, it in enumerate(part):
            plan.ids[i] = _ptr(it[7])
        ctypes.memmove(plan.palette, raw_palettes, len(raw_palettes))
        ctypes.memmove(plan.font, raw_font, len(raw_font))
        plan.label_scale, plan.untracked_skip = int(label_scale), int(untracked == 'skip')
        _launch(entry, who, dev, ctypes.byref(plan))


ANON_CELLS = (2, 4, 8, 16, 32, 64)


def anonymize(kind, items, fills, head, K, *, region='head', mode='pixelate', cell=16, margin=0, grow=2, head_scale=12,
              head_min=2, fallback='person', score_thr=0.3, kpt_thr=0.):
    """People hidden in surfaces in place, one launch per 32 surfaces (pave_anonymize_nv12 / _bgr; the rule is DESIGN
    section 15).  kind and items: as in draw_poses, an item's table naming one of `fills`: 1 .. 4 triples of bytes
    stored as they are by mode 'fill'.  head: up to 8 key-point indices < K (needed by region 'head').  region 'head' |
    'person', mode 'pixelate' | 'fill', cell one of 2, 4, 8, 16, 32, 64 pixels, margin 0 .. 64 pixels, grow, head_scale
    and head_min 0 .. 32 sixteenths, fallback 'person' | 'skip'.  Shapes, types and ranges raise ValueError before
    anything is asked of a device."""
    who = 'anonymize'
    if kind not in ('nv12', 'bgr'):
        raise ValueError(f"{who}: kind {kind!r} is not 'nv12' or 'bgr'")
    items, K = list(items), int(K)
    if not 1 <= K <= native.DRAW_MAX_K:
        raise ValueError(f'{who}: K in 1 .. {native.DRAW_MAX_K}, got {K}')
    for value, name, allowed in ((region, 'region', ('head', 'person')), (mode, 'mode', ('pixelate', 'fill')),
                                 (fallback, 'fallback', ('person', 'skip')), (cell, 'cell', ANON_CELLS)):
        if isinstance(value, bool) or value not in allowed:
            raise ValueError(f'{who}: {name} is one of {allowed}, got {value!r}')
    for value, name, top in ((margin, 'margin', native.ANON_MAX_MARGIN), (grow, 'grow', native.ANON_MAX_SIXTEENTHS),
                             (head_scale, 'head_scale', native.ANON_MAX_SIXTEENTHS),
                             (head_min, 'head_min', native.ANON_MAX_SIXTEENTHS)):
        if isinstance(value, bool) or not isinstance(value, int) or not 0 <= value <= top:
            raise ValueError(f'{who}: {name} is an integer in 0 .. {top}, got {value!r}')
    try:
        head = [int(k) for k in head]
    except (TypeError, ValueError):
        raise ValueError(f'{who}: head is a list of key-point indices') from None
    if len(head) > native.ANON_MAX_HEAD or any(not 0 <= k < K for k in head):
        raise ValueError(f'{who}: head is at most {native.ANON_MAX_HEAD} indices in [0, {K}), got {head}')
    if region == 'head' and not head:
        raise ValueError(f"{who}: region 'head' needs head indices")
    try:
        fills = [bytes(int(c) for c in f) for f in fills]
    except (TypeError, ValueError):
        fills = []
    if not 1 <= len(fills) <= native.DRAW_MAX_TABLES or any(len(f) != 3 for f in fills):
        raise ValueError(f'{who}: fills are 1 .. {native.DRAW_MAX_TABLES} triples of bytes')
    geometry = _surface_geometry(who, kind, items, K, len(fills), 'fill')
    dev = _draw_device(who, items)
    entry = 'pave_anonymize_nv12' if kind == 'nv12' else 'pave_anonymize_bgr'
    raw_fills = b''.join(fills)
    for at in range(0, len(items), native.DRAW_MAX_SURFACES):
        plan = native.AnonPlan()
        part = items[at:at + native.DRAW_MAX_SURFACES]
        for i, it in enumerate(part):
            pitch, W, H, N, sx, sy, table = geometry[at + i]
            plan.dst[i], plan.kpts[i], plan.bboxes[i], plan.keep[i] = it[0].data_ptr(), it[2].data_ptr(), \
                it[3].data_ptr(), _ptr(it[4])
            plan.pitch[i], plan.width[i], plan.height[i], plan.n_poses[i] = pitch, W, H, N
            plan.scale[i][0], plan.scale[i][1], plan.table[i] = sx, sy, table
        ctypes.memmove(plan.fill, raw_fills, len(raw_fills))
        for h, k in enumerate(head):
            plan.head[h] = k
        plan.n, plan.K, plan.n_head = len(part), K, len(head)
        plan.region, plan.mode = int(region == 'person'), int(mode == 'fill')
        plan.fallback_skip, plan.cell, plan.margin, plan.grow = int(fallback == 'skip'), int(cell), int(margin), int(grow)
        plan.head_scale, plan.head_min = int(head_scale), int(head_min)
        plan.score_thr, plan.kpt_thr = float(score_thr), float(kpt_thr)
        _launch(entry, who, dev, ctypes.byref(plan))


_TRACK_STATE =(('id', 1), ('last', 1), ('kpts', 2), ('vis', 1), ('area', 1), ('frame', 0), ('next_id', 0),
                ('dropped', 0))   # name, kind: 0 [cameras], 1 [cameras, M], 2 [cameras, M, K, 2]


def track_scratch(device):
    """The pair-key area of pave_track_poses: 32 blocks x 128 x 128 int64 (4 MiB), allocated once per tracker."""
    return torch.empty((native.TRACK_MAX_FRAMES, native.TRACK_MAX_POSES, native.TRACK_MAX_TRACKS), dtype=torch.int64,
                       device=device)


_TRACK_MOTION = ('vel', 'hits', 'gain', 'max_predict', 'new_gate')


def track_poses(entries, state, scratch, C, *, min_kpts, max_age=30, score_thr=0.3, kpt_thr=0., motion=None):
    """Track ids for frames of poses, one launch per 32 frames (pave_track_poses; the rule is DESIGN section 14).
    entries: one (kpts [N, K, 3] fp32, bboxes [N, 5] fp32, keep [N] int32 or None, camera, (sx, sy)) per frame, N <=
    128, the frames of one camera in time order; state: int32 device tensors id, last, vis, area [cameras, M], kpts
    [cameras, M, K, 2], frame, next_id, dropped [cameras], read and written; scratch: track_scratch(device); C: K
    pair constants in [1, 2^24).  motion: None, or the constant-velocity model of section 14 "Motion"
    (pave_track_poses_motion) as a dict or a tuple of (vel, hits, gain, max_predict, new_gate): int32 device tensors
    vel [cameras, M, 2] (1/16 quarter pixel per frame) and hits [cameras, M], read and written, and integers gain
    1 .. 16, max_predict 0 .. 255, new_gate 1 .. 16.  Returns one int32 [N] tensor of ids per entry.  Shapes, types
    and ranges raise ValueError before anything is asked of a device."""
    who = 'track_poses'
    entries = list(entries)
    if not isinstance(state, dict) or any(not isinstance(state.get(name), torch.Tensor) for name, _ in _TRACK_STATE):
        raise ValueError(f'{who}: state holds the tensors {", ".join(n for n, _ in _TRACK_STATE)}')
    if state['kpts'].dim() != 4 or state['kpts'].shape[3] != 2:
        raise ValueError(f'{who}: state kpts must be [cameras, M, K, 2], got {tuple(state["kpts"].shape)}')
    cameras, M, K = state['kpts'].shape[:3]
    if not (1 <= cameras <= native.TRACK_MAX_CAMERAS and 1 <= M <= native.TRACK_MAX_TRACKS
            and 1 <= K <= native.TRACK_MAX_K):
        raise ValueError(f'{who}: cameras in 1 .. {native.TRACK_MAX_CAMERAS}, M in 1 .. {native.TRACK_MAX_TRACKS} and K '
                         f'in 1 .. {native.TRACK_MAX_K}, got {cameras}, {M} and {K}')
    dev = state['kpts'].device
    for name, kind in _TRACK_STATE:
        t = state[name]
        want = ((cameras,), (cameras, M), (cameras, M, K, 2))[kind]
        if t.dtype != torch.int32 or tuple(t.shape) != want or not t.is_contiguous():
            raise ValueError(f'{who}: state {name} must be a contiguous int32 {list(want)} tensor')
    if not (isinstance(scratch, torch.Tensor) and scratch.dtype == torch.int64 and scratch.is_contiguous()
            and scratch.numel() >= native.TRACK_MAX_FRAMES * native.TRACK_MAX_POSES * native.TRACK_MAX_TRACKS):
        raise ValueError(f'{who}: scratch is track_scratch(device)')
    C = [int(c) for c in C]
    if len(C) != K or any(not 1 <= c < 1 << 24 for c in C):
        raise ValueError(f'{who}: C holds K = {K} pair constants in [1, 2^24)')
    if int(min_kpts) != min_kpts or not 1 <= min_kpts <= K:
        raise ValueError(f'{who}: min_kpts in 1 .. K = {K}, got {min_kpts!r}')
    if int(max_age) != max_age or max_age < 0:
        raise ValueError(f'{who}: max_age must be an integer >= 0, got {max_age!r}')
    if motion is not None:
        if isinstance(motion, dict):
            if sorted(motion) != sorted(_TRACK_MOTION):
                raise ValueError(f'{who}: motion holds {", ".join(_TRACK_MOTION)}')
            motion = tuple(motion[n] for n in _TRACK_MOTION)
        if not (isinstance(motion, (tuple, list)) and len(motion) == 5):
            raise ValueError(f'{who}: motion is None or ({", ".join(_TRACK_MOTION)})')
        vel, hits, gain, max_predict, new_gate = motion
        for name, t, want in (('vel', vel, (cameras, M, 2)), ('hits', hits, (cameras, M))):
            if not (isinstance(t, torch.Tensor) and t.dtype == torch.int32 and tuple(t.shape) == want
                    and t.is_contiguous()):
                raise ValueError(f'{who}: motion {name} must be a contiguous int32 {list(want)} tensor')
        for name, v, lo, hi in (('gain', gain, 1, 16), ('max_predict', max_predict, 0, 255), ('new_gate', new_gate, 1, 16)):
            if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
                raise ValueError(f'{who}: motion {name} must be an integer in {lo} .. {hi}, got {v!r}')
    checked = []
    for i, entry in enumerate(entries):
        if not (isinstance(entry, (tuple, list)) and len(entry) == 5):
            raise ValueError(f'{who}: entry {i} is (kpts, bboxes, keep, camera, (sx, sy))')
        kpts, bboxes, keep, camera, scale = entry
        if not (isinstance(kpts, torch.Tensor) and kpts.dtype == torch.float32 and kpts.dim() == 3
                and tuple(kpts.shape[1:]) == (K, 3)):
            raise ValueError(f'{who}: kpts of entry {i} must be a [N, {K}, 3] float32 tensor')
        N = kpts.shape[0]
        if not (isinstance(bboxes, torch.Tensor) and bboxes.dtype == torch.float32 and tuple(bboxes.shape) == (N, 5)):
            raise ValueError(f'{who}: bboxes of entry {i} must be a [{N}, 5] float32 tensor')
        if keep is not None and not (isinstance(keep, torch.Tensor) and keep.dtype == torch.int32
                                     and tuple(keep.shape) == (N,)):
            raise ValueError(f'{who}: keep of entry {i} must be a [{N}] int32 tensor')
        if N > native.TRACK_MAX_POSES:
            raise ValueError(f'{who}: entry {i} has {N} poses, at most {native.TRACK_MAX_POSES}')
        if isinstance(camera, bool) or int(camera) != camera or not 0 <= camera < cameras:
            raise ValueError(f'{who}: the camera of entry {i} must be an integer in [0, {cameras}), got {camera!r}')
        try:
            sx, sy = (float(v) for v in scale)
        except (TypeError, ValueError):
            raise ValueError(f'{who}: the scale of entry {i} is (sx, sy)') from None
        if not (0 < sx < float('inf') and 0 < sy < float('inf')):
            raise ValueError(f'{who}: the scale of entry {i} must be positive and finite, got {(sx, sy)}')
        if any(t is not None and not t.is_contiguous() for t in (kpts, bboxes, keep)):
            raise ValueError(f'{who}: the tensors of entry {i} must be contiguous')
        checked.append((kpts, bboxes, keep, int(camera), sx, sy, N))
    # the shapes are right: now where the tensors live
    if not dev.type == 'cuda':
        raise ValueError(f'{who}: the state must be on a HIP device (pavenet_amd has no CPU path), got {dev}')
    if any(t.device != dev for t in [state[n] for n, _ in _TRACK_STATE] + [scratch]):
        raise ValueError(f'{who}: the state tensors and the scratch area must be on one device ({dev})')
    if motion is not None and (vel.device != dev or hits.device != dev):
        raise ValueError(f'{who}: motion vel and hits must be on the HIP device of the state ({dev})')
    for i, c in enumerate(checked):
        if any(t is not None and t.device != dev for t in c[:3]):
            raise ValueError(f'{who}: the tensors of entry {i} must be on the HIP device of the state ({dev})')
    ids = [torch.empty((c[6],), dtype=torch.int32, device=dev) for c in checked]
    for at in range(0, len(checked), native.TRACK_MAX_FRAMES):
        full = native.TrackMotionPlan() if motion is not None else native.TrackPlan()
        plan = full.base if motion is not None else full
        part = checked[at:at + native.TRACK_MAX_FRAMES]
        for i, (kpts, bboxes, keep, camera, sx, sy, N) in enumerate(part):
            plan.kpts[i], plan.bboxes[i], plan.keep[i], plan.ids[i] = _ptr(kpts) or None, _ptr(bboxes) or None, \
                _ptr(keep) or None, ids[at + i].data_ptr() or None
            plan.n[i], plan.camera[i], plan.scale[i][0], plan.scale[i][1] = N, camera, sx, sy
        plan.track_id, plan.track_last, plan.track_kpts, plan.track_vis, plan.track_area = (
            state[n].data_ptr() for n in ('id', 'last', 'kpts', 'vis', 'area'))
        plan.frame, plan.next_id, plan.dropped = (state[n].data_ptr() for n in ('frame', 'next_id', 'dropped'))
        plan.scratch = scratch.data_ptr()
        for k, c in enumerate(C):
            plan.C[k] = c
        plan.entries, plan.cameras, plan.M, plan.K = len(part), cameras, M, K
        plan.min_kpts, plan.max_age, plan.score_thr, plan.kpt_thr = int(min_kpts), int(max_age), float(score_thr), \
            float(kpt_thr)
        if motion is not None:
            full.track_vel, full.track_hits = vel.data_ptr(), hits.data_ptr()
            full.gain, full.max_predict, full.new_gate = gain, max_predict, new_gate
        _launch('pave_track_poses_motion' if motion is not None else 'pave_track_poses', who, dev, ctypes.byref(full))
    return ids


ZONE_ANCHORS = ('feet', 'box', 'centre')       # PAVE_ZONE_ANCHOR_*


# ---- what the six updates that follow track ids share (csrc/pave_tracked.h) ----
def _tracked_entries(who, entries, K, cameras):
    """The (kpts, bboxes, keep, ids, camera, sx, sy, N) of every (kpts, bboxes, keep, ids, camera, (sx, sy)) entry of
    an update that follows track ids, or the ValueError."""
    checked = []
    for i, entry in enumerate(entries):
        if not (isinstance(entry, (tuple, list)) and len(entry) == 6):
            raise ValueError(f'{who}: entry {i} is (kpts, bboxes, keep, ids, camera, (sx, sy))')
        kpts, bboxes, keep, ids, camera, scale = entry
        if not (isinstance(kpts, torch.Tensor) and kpts.dtype == torch.float32 and kpts.dim() == 3
                and tuple(kpts.shape[1:]) == (K, 3)):
            raise ValueError(f'{who}: kpts of entry {i} must be a [N, {K}, 3] float32 tensor')
        N = kpts.shape[0]
        if not (isinstance(bboxes, torch.Tensor) and bboxes.dtype == torch.float32 and tuple(bboxes.shape) == (N, 5)):
            raise ValueError(f'{who}: bboxes of entry {i} must be a [{N}, 5] float32 tensor')
        if keep is not None and not (isinstance(keep, torch.Tensor) and keep.dtype == torch.int32
                                     and tuple(keep.shape) == (N,)):
            raise ValueError(f'{who}: keep of entry {i} must be a [{N}] int32 tensor')
        if not (isinstance(ids, torch.Tensor) and ids.dtype == torch.int32 and tuple(ids.shape) == (N,)):
            raise ValueError(f'{who}: ids of entry {i} must be a [{N}] int32 tensor')
        if N > native.TRACK_MAX_POSES:
            raise ValueError(f'{who}: entry {i} has {N} poses, at most {native.TRACK_MAX_POSES}')
        if isinstance(camera, bool) or int(camera) != camera or not 0 <= camera < cameras:
            raise ValueError(f'{who}: the camera of entry {i} must be an integer in [0, {cameras}), got {camera!r}')
        try:
            sx, sy = (float(v) for v in scale)
        except (TypeError, ValueError):
            raise ValueError(f'{who}: the scale of entry {i} is (sx, sy)') from None
        if not (0 < sx < float('inf') and 0 < sy < float('inf')):
            raise ValueError(f'{who}: the scale of entry {i} must be positive and finite, got {(sx, sy)}')
        if not (kpts.is_contiguous() and bboxes.is_contiguous() and ids.is_contiguous()
                and (keep is None or keep.is_contiguous())):
            raise ValueError(f'{who}: the tensors of entry {i} must be contiguous')
        checked.append((kpts, bboxes, keep, ids, int(camera), sx, sy, N))
    return checked


def _max_age(who, max_age):
    if isinstance(max_age, bool) or int(max_age) != max_age or max_age < 0:
        raise ValueError(f'{who}: max_age must be an integer >= 0, got {max_age!r}')
    return int(max_age)


def _anchor(who, anchor, anchor_kpts, K):
    """(PAVE_ZONE_ANCHOR_*, the key points of 'feet') of an update that places a pose by its anchor."""
    if anchor not in ZONE_ANCHORS:
        raise ValueError(f'{who}: anchor must be one of {", ".join(ZONE_ANCHORS)}, got {anchor!r}')
    anchor_kpts = list(anchor_kpts)
    if len(anchor_kpts) > native.ZONE_MAX_ANCHOR_KPTS or any(
            isinstance(k, bool) or not isinstance(k, int) or not 0 <= k < K for k in anchor_kpts):
        raise ValueError(f'{who}: anchor_kpts holds at most {native.ZONE_MAX_ANCHOR_KPTS} integers in [0, {K}), got '
                         f'{anchor_kpts!r}')
    return ZONE_ANCHORS.index(anchor), anchor_kpts


def _tracked_devices(who, dev, tensors, checked, what='the state tensors'):
    if not dev.type == 'cuda':
        raise ValueError(f'{who}: the state must be on a HIP device (pavenet_amd has no CPU path), got {dev}')
    if any(t.device != dev for t in tensors):
        raise ValueError(f'{who}: {what} must be on one device ({dev})')
    for i, c in enumerate(checked):   # (spelt out: this runs per entry of every call)
        if c[0].device != dev or c[1].device != dev or c[3].device != dev or (c[2] is not None and c[2].device != dev):
            raise ValueError(f'{who}: the tensors of entry {i} must be on the HIP device of the state ({dev})')


def _tracked_fill(plan, part, cameras, S, K, max_age, score_thr, kpt_thr, anchor=None):
    """The fields every plan of these updates has: the entries of _tracked_entries, the sizes, who takes part and,
    where the plan has one, the anchor of _anchor."""
    for i, (kpts, bboxes, keep, ids, camera, sx, sy, N) in enumerate(part):
        plan.kpts[i], plan.bboxes[i], plan.keep[i], plan.ids[i] = _ptr(kpts) or None, _ptr(bboxes) or None, \
            _ptr(keep) or None, _ptr(ids) or None
        plan.n[i], plan.camera[i], plan.scale[i][0], plan.scale[i][1] = N, camera, sx, sy
    plan.entries, plan.cameras, plan.S, plan.K, plan.max_age = len(part), cameras, S, K, max_age
    plan.score_thr, plan.kpt_thr = float(score_thr), float(kpt_thr)
    if anchor is not None:
        plan.anchor, plan.n_anchor = anchor[0], len(anchor[1])
        for i, k in enumerate(anchor[1]):
            plan.anchor_kpt[i] = k


_SMOOTH_STATE = (('id', 1), ('last', 1), ('pos', 2), ('vel', 2), ('frame', 0), ('dropped', 0))
# name, kind: 0 [cameras], 1 [cameras, S], 2 [cameras, S, K + 2, 2]


def smooth_poses(entries, state, *, max_age=30, alpha_min=32, beta=128, velocity_gain=3, score_thr=0.3, kpt_thr=0.):
    """Steady poses for frames of tracked poses, one launch per 32 frames (pave_smooth_poses; the rule is DESIGN
    section 16).  entries: one (kpts [N, K, 3] fp32, bboxes [N, 5] fp32, keep [N] int32 or None, ids [N] int32,
    camera, (sx, sy)) per frame, N <= 128, the frames of one camera in time order; state: int32 device tensors id,
    last [cameras, S], pos, vel [cameras, S, K + 2, 2] (1/64 pixel, and per frame), frame, dropped [cameras], read
    and written; alpha_min 1 .. 256, beta 0 .. 4096 and velocity_gain 1 .. 16 are integers.  Returns one (out_kpts
    [N, K, 3], out_bboxes [N, 5]) pair of new fp32 tensors per entry, in original-image pixels.  Shapes, types and
    ranges raise ValueError before anything is asked of a device."""
    who = 'smooth_poses'
    entries = list(entries)
    if not isinstance(state, dict) or any(not isinstance(state.get(name), torch.Tensor) for name, _ in _SMOOTH_STATE):
        raise ValueError(f'{who}: state holds the tensors {", ".join(n for n, _ in _SMOOTH_STATE)}')
    if state['pos'].dim() != 4 or state['pos'].shape[3] != 2 or state['pos'].shape[2] < 3:
        raise ValueError(f'{who}: state pos must be [cameras, S, K + 2, 2], got {tuple(state["pos"].shape)}')
    cameras, S, J = state['pos'].shape[:3]
    K = J - 2
    if not (1 <= cameras <= native.TRACK_MAX_CAMERAS and 1 <= S <= native.TRACK_MAX_TRACKS
            and 1 <= K <= native.TRACK_MAX_K):
        raise ValueError(f'{who}: cameras in 1 .. {native.TRACK_MAX_CAMERAS}, S in 1 .. {native.TRACK_MAX_TRACKS} and K '
                         f'in 1 .. {native.TRACK_MAX_K}, got {cameras}, {S} and {K}')
    dev = state['pos'].device
    for name, kind in _SMOOTH_STATE:
        t = state[name]
        want = ((cameras,), (cameras, S), (cameras, S, J, 2))[kind]
        if t.dtype != torch.int32 or tuple(t.shape) != want or not t.is_contiguous():
            raise ValueError(f'{who}: state {name} must be a contiguous int32 {list(want)} tensor')
    for name, v, lo, hi in (('alpha_min', alpha_min, 1, 256), ('beta', beta, 0, 4096),
                            ('velocity_gain', velocity_gain, 1, 16)):
        if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
            raise ValueError(f'{who}: {name} must be an integer in {lo} .. {hi}, got {v!r}')
    max_age = _max_age(who, max_age)
    checked = _tracked_entries(who, entries, K, cameras)
    # the shapes are right: now where the tensors live
    _tracked_devices(who, dev, (state[n] for n, _ in _SMOOTH_STATE), checked)
    outs = [(torch.empty((c[7], K, 3), dtype=torch.float32, device=dev),
             torch.empty((c[7], 5), dtype=torch.float32, device=dev)) for c in checked]
    for at in range(0, len(checked), native.TRACK_MAX_FRAMES):
        plan = native.SmoothPlan()
        part = checked[at:at + native.TRACK_MAX_FRAMES]
        _tracked_fill(plan, part, cameras, S, K, max_age, score_thr, kpt_thr)
        for i in range(len(part)):
            plan.out_kpts[i], plan.out_bboxes[i] = (t.data_ptr() or None for t in outs[at + i])
        plan.slot_id, plan.slot_last, plan.slot_pos, plan.slot_vel, plan.frame, plan.dropped = (
            state[n].data_ptr() for n, _ in _SMOOTH_STATE)
        plan.alpha_min, plan.beta, plan.velocity_gain = alpha_min, beta, velocity_gain
        _launch('pave_smooth_poses', who, dev, ctypes.byref(plan))
    return outs


_ZONE_STATE = (('id', 1), ('last', 1), ('pos', 2), ('inside', 1), ('alerted', 1), ('streak', 3), ('since', 3),
               ('frame', 0), ('dropped', 0), ('counters', 4), ('geometry', 5))
# name, kind: 0 [cameras], 1 [cameras, S], 2 [cameras, S, 2], 3 [cameras, S, 8], 4 [cameras, 56], 5 [cameras, 306]


def zone_events(entries, state, *, K, max_age=30, anchor='feet', anchor_kpts=(), min_frames=2, max_events=256,
                score_thr=0.3, kpt_thr=0.):
    """Zone and line events for frames of tracked poses, one launch per 32 frames (pave_zone_events; the rule is
    DESIGN section 17).  entries: one (kpts [N, K, 3] fp32, bboxes [N, 5] fp32, keep [N] int32 or None, ids [N] int32,
    camera, (sx, sy)) per frame, N <= 128, the frames of one camera in time order; state: int32 device tensors id,
    last, inside, alerted [cameras, S], pos [cameras, S, 2] (1/8 pixel), streak, since [cameras, S, 8], frame, dropped
    [cameras], counters [cameras, 56], read and written, and geometry [cameras, 306], read (the layouts are
    PAVE_ZONE_CNT_* and PAVE_ZONE_GEOM_* of include/pave_hip.h); anchor 'feet' | 'box' | 'centre', anchor_kpts at
    most 4 key points in [0, K), min_frames 1 .. 255, max_events 1 .. 4096.  Returns one dict(zones [N], dwell [N, 8],
    events [max_events, 5], n_events 0-d) of new int32 tensors per entry.  Shapes, types and ranges raise ValueError
    before anything is asked of a device."""
    who = 'zone_events'
    entries = list(entries)
    if not isinstance(state, dict) or any(not isinstance(state.get(name), torch.Tensor) for name, _ in _ZONE_STATE):
        raise ValueError(f'{who}: state holds the tensors {", ".join(n for n, _ in _ZONE_STATE)}')
    if state['pos'].dim() != 3 or state['pos'].shape[2] != 2:
        raise ValueError(f'{who}: state pos must be [cameras, S, 2], got {tuple(state["pos"].shape)}')
    cameras, S = state['pos'].shape[:2]
    if isinstance(K, bool) or not isinstance(K, int):
        raise ValueError(f'{who}: K must be an integer, got {K!r}')
    if not (1 <= cameras <= native.TRACK_MAX_CAMERAS and 1 <= S <= native.TRACK_MAX_TRACKS
            and 1 <= K <= native.TRACK_MAX_K):
        raise ValueError(f'{who}: cameras in 1 .. {native.TRACK_MAX_CAMERAS}, S in 1 .. {native.TRACK_MAX_TRACKS} and K '
                         f'in 1 .. {native.TRACK_MAX_K}, got {cameras}, {S} and {K}')
    dev = state['pos'].device
    for name, kind in _ZONE_STATE:
        t = state[name]
        want = ((cameras,), (cameras, S), (cameras, S, 2), (cameras, S, native.ZONE_MAX_ZONES),
                (cameras, native.ZONE_COUNTER_WORDS), (cameras, native.ZONE_GEOM_WORDS))[kind]
        if t.dtype != torch.int32 or tuple(t.shape) != want or not t.is_contiguous():
            raise ValueError(f'{who}: state {name} must be a contiguous int32 {list(want)} tensor')
    for name, v, lo, hi in (('min_frames', min_frames, 1, 255), ('max_events', max_events, 1, native.ZONE_MAX_EVENTS)):
        if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
            raise ValueError(f'{who}: {name} must be an integer in {lo} .. {hi}, got {v!r}')
    max_age = _max_age(who, max_age)
    anchor = _anchor(who, anchor, anchor_kpts, K)
    checked = _tracked_entries(who, entries, K, cameras)
    # the shapes are right: now where the tensors live
    _tracked_devices(who, dev, (state[n] for n, _ in _ZONE_STATE), checked)
    z = dict(dtype=torch.int32, device=dev)
    outs = [dict(zones=torch.empty((c[7],), **z), dwell=torch.empty((c[7], native.ZONE_MAX_ZONES), **z),
                 events=torch.empty((max_events, native.ZONE_EVENT_WORDS), **z), n_events=torch.empty((), **z))
            for c in checked]
    for at in range(0, len(checked), native.TRACK_MAX_FRAMES):
        plan = native.ZonePlan()
        part = checked[at:at + native.TRACK_MAX_FRAMES]
        _tracked_fill(plan, part, cameras, S, K, max_age, score_thr, kpt_thr, anchor)
        for i in range(len(part)):
            out = outs[at + i]
            plan.out_zones[i], plan.out_dwell[i] = out['zones'].data_ptr() or None, out['dwell'].data_ptr() or None
            plan.out_events[i], plan.out_n_events[i] = out['events'].data_ptr(), out['n_events'].data_ptr()
        (plan.slot_id, plan.slot_last, plan.slot_pos, plan.slot_inside, plan.slot_alerted, plan.slot_streak,
         plan.slot_since, plan.frame, plan.dropped, plan.counters, plan.geometry) = (
            state[n].data_ptr() for n, _ in _ZONE_STATE)
        plan.min_frames, plan.max_events = min_frames, max_events
        _launch('pave_zone_events', who, dev, ctypes.byref(plan))
    return outs


_POSTURE_STATE = (('id', 1), ('last', 1), ('posture', 1), ('since', 1), ('upright', 1), ('streak', 1), ('alerted', 1),
                  ('hands', 1), ('hand_streak', 1), ('frame', 0), ('dropped', 0), ('counters', 2))
# name, kind: 0 [cameras], 1 [cameras, S], 2 [cameras, 8]
POSTURE_PARTS = ('shoulders', 'hips', 'ankles', 'wrists')   # PAVE_POSTURE_PART_*


def posture_events(entries, state, *, K, parts, max_age=30, min_frames=3, lean=11, flat=11, squat=18, hand_up=4,
                   fall_window=30, down_frames=75, max_events=256, score_thr=0.3, kpt_thr=0.):
    """Postures, falls and raised hands for frames of tracked poses, one launch per 32 frames (pave_posture_events;
    the rule is DESIGN section 20).  entries: one (kpts [N, K, 3] fp32, bboxes [N, 5] fp32, keep [N] int32 or None, ids
    [N] int32, camera, (sx, sy)) per frame, N <= 128, the frames of one camera in time order; state: int32 device
    tensors id, last, posture, since, upright, streak, alerted, hands, hand_streak [cameras, S], frame, dropped
    [cameras] and counters [cameras, 8] (PAVE_POSTURE_CNT_* of include/pave_hip.h), read and written; parts: four
    lists of at most 4 key points in [0, K), the shoulders, hips, ankles and wrists; min_frames 1 .. 255, lean and
    flat 1 .. 255, squat 0 .. 255, hand_up 0 .. 255 or None, fall_window and down_frames 0 .. 2^30, max_events
    1 .. 4096.  Returns one dict(posture, raw, hands, since [N], events [max_events, 5], n_events 0-d) of new int32
    tensors per entry.  Shapes, types and ranges raise ValueError before anything is asked of a device."""
    who = 'posture_events'
    entries = list(entries)
    if not isinstance(state, dict) or any(not isinstance(state.get(name), torch.Tensor) for name, _ in _POSTURE_STATE):
        raise ValueError(f'{who}: state holds the tensors {", ".join(n for n, _ in _POSTURE_STATE)}')
    if state['id'].dim() != 2:
        raise ValueError(f'{who}: state id must be [cameras, S], got {tuple(state["id"].shape)}')
    cameras, S = state['id'].shape
    if isinstance(K, bool) or not isinstance(K, int):
        raise ValueError(f'{who}: K must be an integer, got {K!r}')
    if not (1 <= cameras <= native.TRACK_MAX_CAMERAS and 1 <= S <= native.TRACK_MAX_TRACKS
            and 1 <= K <= native.TRACK_MAX_K):
        raise ValueError(f'{who}: cameras in 1 .. {native.TRACK_MAX_CAMERAS}, S in 1 .. {native.TRACK_MAX_TRACKS} and K '
                         f'in 1 .. {native.TRACK_MAX_K}, got {cameras}, {S} and {K}')
    dev = state['id'].device
    for name, kind in _POSTURE_STATE:
        t = state[name]
        want = ((cameras,), (cameras, S), (cameras, native.POSTURE_COUNTER_WORDS))[kind]
        if t.dtype != torch.int32 or tuple(t.shape) != want or not t.is_contiguous():
            raise ValueError(f'{who}: state {name} must be a contiguous int32 {list(want)} tensor')
    for name, v, lo, hi in (('min_frames', min_frames, 1, 255), ('max_events', max_events, 1, native.POSTURE_MAX_EVENTS),
                            ('lean', lean, 1, native.POSTURE_MAX_SLOPE), ('flat', flat, 1, native.POSTURE_MAX_SLOPE),
                            ('squat', squat, 0, native.POSTURE_MAX_SLOPE),
                            ('hand_up', 0 if hand_up is None else hand_up, 0, native.POSTURE_MAX_SLOPE),
                            ('fall_window', fall_window, 0, native.POSTURE_MAX_WAIT),
                            ('down_frames', down_frames, 0, native.POSTURE_MAX_WAIT)):
        if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
            raise ValueError(f'{who}: {name} must be an integer in {lo} .. {hi}, got {v!r}')
    max_age = _max_age(who, max_age)
    try:
        parts = [list(p) for p in parts]
    except TypeError:
        raise ValueError(f'{who}: parts are the key points of {", ".join(POSTURE_PARTS)}') from None
    if len(parts) != native.POSTURE_PARTS:
        raise ValueError(f'{who}: parts are the key points of {", ".join(POSTURE_PARTS)}, got {len(parts)} lists')
    for name, p in zip(POSTURE_PARTS, parts):
        if len(p) > native.POSTURE_MAX_PART or any(
                isinstance(k, bool) or not isinstance(k, int) or not 0 <= k < K for k in p):
            raise ValueError(f'{who}: part {name} holds at most {native.POSTURE_MAX_PART} integers in [0, {K}), got '
                             f'{p!r}')
    checked = _tracked_entries(who, entries, K, cameras)
    # the shapes are right: now where the tensors live
    _tracked_devices(who, dev, (state[n] for n, _ in _POSTURE_STATE), checked)
    z = dict(dtype=torch.int32, device=dev)
    outs = [dict(posture=torch.empty((c[7],), **z), raw=torch.empty((c[7],), **z), hands=torch.empty((c[7],), **z),
                 since=torch.empty((c[7],), **z), events=torch.empty((max_events, native.POSTURE_EVENT_WORDS), **z),
                 n_events=torch.empty((), **z)) for c in checked]
    for at in range(0, len(checked), native.TRACK_MAX_FRAMES):
        plan = native.PosturePlan()
        part = checked[at:at + native.TRACK_MAX_FRAMES]
        _tracked_fill(plan, part, cameras, S, K, max_age, score_thr, kpt_thr)
        for i in range(len(part)):
            out = outs[at + i]
            plan.out_posture[i], plan.out_raw[i] = out['posture'].data_ptr() or None, out['raw'].data_ptr() or None
            plan.out_hands[i], plan.out_since[i] = out['hands'].data_ptr() or None, out['since'].data_ptr() or None
            plan.out_events[i], plan.out_n_events[i] = out['events'].data_ptr(), out['n_events'].data_ptr()
        (plan.slot_id, plan.slot_last, plan.slot_posture, plan.slot_since, plan.slot_upright, plan.slot_streak,
         plan.slot_alerted, plan.slot_hands, plan.slot_hand_streak, plan.frame, plan.dropped, plan.counters) = (
            state[n].data_ptr() for n, _ in _POSTURE_STATE)
        for p, keys in enumerate(parts):
            plan.n_part[p] = len(keys)
            for i, k in enumerate(keys):
                plan.part[p][i] = k
        plan.min_frames, plan.lean, plan.flat, plan.squat = min_frames, lean, flat, squat
        plan.hand_up = native.POSTURE_HANDS_OFF if hand_up is None else hand_up
        plan.fall_window, plan.down_frames, plan.max_events = fall_window, down_frames, max_events
        _launch('pave_posture_events', who, dev, ctypes.byref(plan))
    return outs


ZONE_LABELS = ('none', 'occupancy', 'entered')              # PAVE_ZONE_LABEL_*
LINE_LABELS = ('none', 'net', 'forward', 'backward')        # PAVE_LINE_LABEL_*
_ZONE_DRAW_STATE = (('geometry', native.ZONE_GEOM_WORDS), ('counters', native.ZONE_COUNTER_WORDS), ('id', 0),
                    ('alerted', 0), ('inside', 0))           # name, columns (0: S)


def draw_zones(kind, items, state, tables, font, *, alpha=48, alpha_occupied=96, alpha_alert=128, outline=2,
               thickness=3, arrow=24, label_scale=2, zone_label='occupancy', line_label='net'):
    """Zones, counting lines and their counts drawn into surfaces in place, one launch per 32 surfaces
    (pave_draw_zones_nv12 / _bgr; the rule is DESIGN section 19).  kind 'nv12' | 'bgr' as in draw_poses.  items: one
    (surface, width, camera, table) per surface (`width` is not read for 'bgr'; a 'bgr' surface may be the rows of a
    wider buffer: strides (pitch, 3, 1)).  state: the monitor's int32 device
    tensors geometry [cameras, 306], counters [cameras, 56] and id, alerted, inside [cameras, S], read only.  tables:
    1 .. 4 of 18 x 3 bytes stored or blended as they are (rows 0 .. 7 zones, 8 .. 15 lines, 16 an alerted zone, 17 the
    ink; nested or as the 54 bytes); font: 11 faces (the digits and a minus) of 7 rows of 5 bits.  The alphas 0 .. 256,
    outline 0 .. 32, thickness 1 .. 32, arrow 0 .. 255, label_scale 0 .. 8, zone_label 'occupancy' | 'entered' | 'none',
    line_label 'net' | 'forward' | 'backward' | 'none'.  Shapes, types and ranges raise ValueError before anything is
    asked of a device."""
    who = 'draw_zones'
    if kind not in ('nv12', 'bgr'):
        raise ValueError(f"{who}: kind {kind!r} is not 'nv12' or 'bgr'")
    items = list(items)
    if not items:
        raise ValueError(f'{who}: no surface')
    if any(not (isinstance(it, (tuple, list)) and len(it) == 4) for it in items):
        raise ValueError(f'{who}: an item is (surface, width, camera, table)')
    for name, v, lo, hi in (('alpha', alpha, 0, 256), ('alpha_occupied', alpha_occupied, 0, 256),
                            ('alpha_alert', alpha_alert, 0, 256), ('outline', outline, 0, 32),
                            ('thickness', thickness, 1, 32), ('arrow', arrow, 0, 255), ('label_scale', label_scale, 0, 8)):
        if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
            raise ValueError(f'{who}: {name} is an integer in {lo} .. {hi}, got {v!r}')
    if zone_label not in ZONE_LABELS:
        raise ValueError(f'{who}: zone_label is one of {", ".join(ZONE_LABELS)}, got {zone_label!r}')
    if line_label not in LINE_LABELS:
        raise ValueError(f'{who}: line_label is one of {", ".join(LINE_LABELS)}, got {line_label!r}')
    try:
        font = [[int(r) for r in rows] for rows in font]
    except (TypeError, ValueError):
        font = []
    if len(font) != native.ZONE_DRAW_FACES or any(len(rows) != 7 or any(not 0 <= r < 32 for r in rows) for rows in font):
        raise ValueError(f'{who}: font is {native.ZONE_DRAW_FACES} faces of 7 rows of 5 bits')
    try:
        tables = [tab if isinstance(tab, bytes) else bytes(int(c) for row in tab for c in (row if len(row) == 3 else ()))
                  for tab in tables]
    except (TypeError, ValueError):
        tables = []
    if not 1 <= len(tables) <= native.DRAW_MAX_TABLES or any(len(t) != 3 * native.ZONE_DRAW_COLORS for t in tables):
        raise ValueError(f'{who}: tables are 1 .. {native.DRAW_MAX_TABLES} of {native.ZONE_DRAW_COLORS} x 3 bytes')
    if not isinstance(state, dict) or any(not isinstance(state.get(n), torch.Tensor) for n, _ in _ZONE_DRAW_STATE):
        raise ValueError(f'{who}: state holds the tensors {", ".join(n for n, _ in _ZONE_DRAW_STATE)}')
    if state['id'].dim() != 2:
        raise ValueError(f'{who}: state id must be [cameras, S], got {tuple(state["id"].shape)}')
    cameras, S = state['id'].shape
    if not (1 <= cameras <= native.TRACK_MAX_CAMERAS and 1 <= S <= native.TRACK_MAX_TRACKS):
        raise ValueError(f'{who}: cameras in 1 .. {native.TRACK_MAX_CAMERAS} and S in 1 .. {native.TRACK_MAX_TRACKS}, got '
                         f'{cameras} and {S}')
    for name, columns in _ZONE_DRAW_STATE:
        t, want = state[name], (cameras, columns or S)
        if t.dtype != torch.int32 or tuple(t.shape) != want or not t.is_contiguous():
            raise ValueError(f'{who}: state {name} must be a contiguous int32 {list(want)} tensor')
    geometry = []
    for i, (surf, width, camera, table) in enumerate(items):
        if not (isinstance(surf, torch.Tensor) and surf.dtype == torch.uint8):
            raise ValueError(f'{who}: surface {i} must be a uint8 tensor')
        if kind == 'nv12':
            if surf.dim() != 2:
                raise ValueError(f'{who}: surface {i} must be [H * 3 // 2, pitch], got {tuple(surf.shape)}')
            if isinstance(width, bool) or not isinstance(width, numbers.Integral):
                raise ValueError(f'{who}: the width of surface {i} must be an integer, got {width!r}')
            rows, pitch = surf.shape
            H, W, row_bytes = rows * 2 // 3, int(width), int(width)
            if rows % 3 != 0 or H % 2 != 0 or H <= 0:
                raise ValueError(f'{who}: surface {i}: {rows} rows are not the 3/2 of an even height')
            if W <= 0 or W % 2 != 0:
                raise ValueError(f'{who}: surface {i}: width {W} must be even and positive')
        else:
            if surf.dim() != 3 or surf.shape[2] != 3 or surf.shape[0] < 1 or surf.shape[1] < 1:
                raise ValueError(f'{who}: surface {i} must be [H, W, 3], got {tuple(surf.shape)}')
            H, W = surf.shape[:2]
            row_bytes = 3 * W
            pitch = row_bytes if surf.is_contiguous() else surf.stride(0)     # (rows of a wider buffer)
            if not surf.is_contiguous() and (surf.stride(2) != 1 or surf.stride(1) != 3):
                raise ValueError(f'{who}: surface {i} must be contiguous, or contiguous rows of a wider buffer')
        if row_bytes > pitch:
            raise ValueError(f'{who}: surface {i}: width {W} exceeds the pitch {pitch}')
        if W > native.DRAW_MAX_SIZE or H > native.DRAW_MAX_SIZE:
            raise ValueError(f'{who}: surface {i}: {W} x {H} exceeds {native.DRAW_MAX_SIZE} x {native.DRAW_MAX_SIZE}')
        if kind == 'nv12' and not surf.is_contiguous():
            raise ValueError(f'{who}: surface {i} must be contiguous')
        if isinstance(camera, bool) or not isinstance(camera, numbers.Integral) or not 0 <= camera < cameras:
            raise ValueError(f'{who}: the camera of surface {i} must be an integer in [0, {cameras}), got {camera!r}')
        if isinstance(table, bool) or not isinstance(table, numbers.Integral) or not 0 <= table < len(tables):
            raise ValueError(f'{who}: surface {i} names colour table {table} of {len(tables)}')
        geometry.append((int(pitch), int(W), int(H), int(camera), int(table)))
    # the shapes are right: now where the tensors live
    dev = state['id'].device
    if dev.type != 'cuda':
        raise ValueError(f'{who}: the state must be on a HIP device (pavenet_amd has no CPU path), got {dev}')
    if any(state[n].device != dev for n, _ in _ZONE_DRAW_STATE):
        raise ValueError(f'{who}: the state tensors must be on one device ({dev})')
    for i, it in enumerate(items):
        if it[0].device != dev:
            raise ValueError(f"{who}: surface {i} is on {it[0].device}, the monitor's state on {dev}")
    entry = 'pave_draw_zones_nv12' if kind == 'nv12' else 'pave_draw_zones_bgr'
    raw_tables, raw_font = b''.join(tables), bytes(r for rows in font for r in rows)
    for at in range(0, len(items), native.DRAW_MAX_SURFACES):
        plan = native.ZoneDrawPlan()
        part = items[at:at + native.DRAW_MAX_SURFACES]
        for i, it in enumerate(part):
            plan.dst[i] = it[0].data_ptr()
            plan.pitch[i], plan.width[i], plan.height[i], plan.camera[i], plan.table[i] = geometry[at + i]
        plan.geometry, plan.counters, plan.slot_id, plan.slot_alerted, plan.slot_inside = (
            state[n].data_ptr() for n, _ in _ZONE_DRAW_STATE)
        ctypes.memmove(plan.color, raw_tables, len(raw_tables))
        ctypes.memmove(plan.font, raw_font, len(raw_font))
        plan.n, plan.cameras, plan.S = len(part), cameras, S
        plan.alpha, plan.alpha_occupied, plan.alpha_alert = alpha, alpha_occupied, alpha_alert
        plan.outline, plan.thickness, plan.arrow, plan.label_scale = outline, thickness, arrow, label_scale
        plan.zone_label, plan.line_label = ZONE_LABELS.index(zone_label), LINE_LABELS.index(line_label)
        _launch(entry, who, dev, ctypes.byref(plan))


_HEAT_STATE = (('id', 1), ('last', 1), ('cell', 1), ('frame', 0), ('dropped', 0), ('peak', 2), ('dwell', 3),
               ('visits', 3))   # name, kind: 0 [cameras], 1 [cameras, S], 2 [cameras, 2], 3 [cameras, Gh, Gw]
HEAT_CELLS = (4, 8, 16, 32, 64)
HEAT_SOURCES = ('dwell', 'visits')             # PAVE_HEAT_DWELL, PAVE_HEAT_VISITS


def heat_grid(who, size, cell):
    """The (Gw, Gh) of a map of `size` = (width, height) original-image pixels at `cell`, or the ValueError."""
    try:
        width, height = size
    except (TypeError, ValueError):
        raise ValueError(f'{who}: size is (width, height), got {size!r}') from None
    for v in (width, height):
        if isinstance(v, bool) or not isinstance(v, numbers.Integral) or not 1 <= v <= native.DRAW_MAX_SIZE:
            raise ValueError(f'{who}: size is (width, height) in 1 .. {native.DRAW_MAX_SIZE} pixels, got {size!r}')
    if isinstance(cell, bool) or cell not in HEAT_CELLS:
        raise ValueError(f'{who}: cell is one of {", ".join(str(c) for c in HEAT_CELLS)}, got {cell!r}')
    Gw, Gh = -(-int(width) // cell), -(-int(height) // cell)
    if Gw > native.HEAT_MAX_GRID or Gh > native.HEAT_MAX_GRID:
        raise ValueError(f'{who}: the grid is at most {native.HEAT_MAX_GRID} cells a side, {size!r} at cell {cell} gives '
                         f'{Gw} x {Gh}')
    return Gw, Gh


def _heat_state(who, state, names, size, cell):
    """The shapes of the monitor's tensors `names` of _HEAT_STATE -> (cameras, S, Gw, Gh)."""
    Gw, Gh = heat_grid(who, size, cell)
    if not isinstance(state, dict) or any(not isinstance(state.get(name), torch.Tensor) for name in names):
        raise ValueError(f'{who}: state holds the tensors {", ".join(names)}')
    if state['peak'].dim() != 2:
        raise ValueError(f'{who}: state peak must be [cameras, 2], got {tuple(state["peak"].shape)}')
    cameras = state['peak'].shape[0]
    S = state['id'].shape[1] if 'id' in names and state['id'].dim() == 2 else 1
    if not (1 <= cameras <= native.TRACK_MAX_CAMERAS and 1 <= S <= native.TRACK_MAX_TRACKS):
        raise ValueError(f'{who}: cameras in 1 .. {native.TRACK_MAX_CAMERAS} and S in 1 .. {native.TRACK_MAX_TRACKS}, got '
                         f'{cameras} and {S}')
    for name, kind in _HEAT_STATE:
        if name not in names:
            continue
        t, want = state[name], ((cameras,), (cameras, S), (cameras, 2), (cameras, Gh, Gw))[kind]
        if t.dtype != torch.int32 or tuple(t.shape) != want or not t.is_contiguous():
            raise ValueError(f'{who}: state {name} must be a contiguous int32 {list(want)} tensor')
    return cameras, S, Gw, Gh


def heat_update(entries, state, *, K, size, cell=8, radius=1, half_life=0, max_age=30, anchor='feet', anchor_kpts=(),
                score_thr=0.3, kpt_thr=0.):
    """Footfall maps from frames of tracked poses, one launch per 32 frames (pave_heat_update; the rule is DESIGN
    section 21).  entries: what `zone_events` takes, one (kpts, bboxes, keep, ids, camera, (sx, sy)) per frame, the
    frames of one camera in time order; state: int32 device tensors id, last, cell [cameras, S], frame, dropped
    [cameras], peak [cameras, 2] and dwell, visits [cameras, Gh, Gw], read and written; size (width, height) in
    original-image pixels 1 .. 8192, cell 4 | 8 | 16 | 32 | 64 with at most 512 cells a side, radius 0 .. 3, half_life
    0 .. 2^18; anchor and anchor_kpts as in `zone_events`.  Returns one dict(cell [N], dwell [N], visits [N]) of new
    int32 tensors per entry.  Shapes, types and ranges raise ValueError before anything is asked of a device."""
    who = 'heat_update'
    entries = list(entries)
    if isinstance(K, bool) or not isinstance(K, int) or not 1 <= K <= native.TRACK_MAX_K:
        raise ValueError(f'{who}: K must be an integer in 1 .. {native.TRACK_MAX_K}, got {K!r}')
    cameras, S, Gw, Gh = _heat_state(who, state, [n for n, _ in _HEAT_STATE], size, cell)
    for name, v, lo, hi in (('radius', radius, 0, native.HEAT_MAX_RADIUS),
                            ('half_life', half_life, 0, native.HEAT_MAX_HALF_LIFE)):
        if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
            raise ValueError(f'{who}: {name} must be an integer in {lo} .. {hi}, got {v!r}')
    max_age = _max_age(who, max_age)
    anchor = _anchor(who, anchor, anchor_kpts, K)
    checked = _tracked_entries(who, entries, K, cameras)
    # the shapes are right: now where the tensors live
    dev = state['peak'].device
    _tracked_devices(who, dev, (state[n] for n, _ in _HEAT_STATE), checked)
    z = dict(dtype=torch.int32, device=dev)
    outs = [dict(cell=torch.empty((c[7],), **z), dwell=torch.empty((c[7],), **z), visits=torch.empty((c[7],), **z))
            for c in checked]
    for at in range(0, len(checked), native.TRACK_MAX_FRAMES):
        plan = native.HeatPlan()
        part = checked[at:at + native.TRACK_MAX_FRAMES]
        _tracked_fill(plan, part, cameras, S, K, max_age, score_thr, kpt_thr, anchor)
        for i in range(len(part)):
            out = outs[at + i]
            plan.out_cell[i], plan.out_dwell[i], plan.out_visits[i] = (out[n].data_ptr() or None
                                                                       for n in ('cell', 'dwell', 'visits'))
        (plan.slot_id, plan.slot_last, plan.slot_cell, plan.frame, plan.dropped, plan.peak, plan.dwell, plan.visits) = (
            state[n].data_ptr() for n, _ in _HEAT_STATE)
        plan.width, plan.height, plan.cell, plan.radius = int(size[0]), int(size[1]), cell, radius
        plan.half_life = half_life
        _launch('pave_heat_update', who, dev, ctypes.byref(plan))
    return outs


def _camera_surfaces(who, kind, items, cameras, tables):
    """The (pitch, W, H, camera, table) of every (surface, width, camera, table) item of a draw call that reads a
    monitor's state, or the ValueError."""
    geometry = []
    for i, (surf, width, camera, table) in enumerate(items):
        if not (isinstance(surf, torch.Tensor) and surf.dtype == torch.uint8):
            raise ValueError(f'{who}: surface {i} must be a uint8 tensor')
        if kind == 'nv12':
            if surf.dim() != 2:
                raise ValueError(f'{who}: surface {i} must be [H * 3 // 2, pitch], got {tuple(surf.shape)}')
            if isinstance(width, bool) or not isinstance(width, numbers.Integral):
                raise ValueError(f'{who}: the width of surface {i} must be an integer, got {width!r}')
            rows, pitch = surf.shape
            H, W, row_bytes = rows * 2 // 3, int(width), int(width)
            if rows % 3 != 0 or H % 2 != 0 or H <= 0:
                raise ValueError(f'{who}: surface {i}: {rows} rows are not the 3/2 of an even height')
            if W <= 0 or W % 2 != 0:
                raise ValueError(f'{who}: surface {i}: width {W} must be even and positive')
        else:
            if surf.dim() != 3 or surf.shape[2] != 3 or surf.shape[0] < 1 or surf.shape[1] < 1:
                raise ValueError(f'{who}: surface {i} must be [H, W, 3], got {tuple(surf.shape)}')
            H, W = surf.shape[:2]
            row_bytes = 3 * W
            pitch = row_bytes if surf.is_contiguous() else surf.stride(0)     # (rows of a wider buffer)
            if not surf.is_contiguous() and (surf.stride(2) != 1 or surf.stride(1) != 3):
                raise ValueError(f'{who}: surface {i} must be contiguous, or contiguous rows of a wider buffer')
        if row_bytes > pitch:
            raise ValueError(f'{who}: surface {i}: width {W} exceeds the pitch {pitch}')
        if W > native.DRAW_MAX_SIZE or H > native.DRAW_MAX_SIZE:
            raise ValueError(f'{who}: surface {i}: {W} x {H} exceeds {native.DRAW_MAX_SIZE} x {native.DRAW_MAX_SIZE}')
        if kind == 'nv12' and not surf.is_contiguous():
            raise ValueError(f'{who}: surface {i} must be contiguous')
        if isinstance(camera, bool) or not isinstance(camera, numbers.Integral) or not 0 <= camera < cameras:
            raise ValueError(f'{who}: the camera of surface {i} must be an integer in [0, {cameras}), got {camera!r}')
        if isinstance(table, bool) or not isinstance(table, numbers.Integral) or not 0 <= table < tables:
            raise ValueError(f'{who}: surface {i} names palette table {table} of {tables}')
        geometry.append((int(pitch), int(W), int(H), int(camera), int(table)))
    return geometry


def draw_heat(kind, items, state, palette, *, size, cell=8, source='dwell', full_scale=None, alpha_max=160, floor=1,
              smooth=True):
    """A footfall map blended into surfaces in place, one launch per 32 surfaces (pave_draw_heat_nv12 / _bgr; the rule
    is DESIGN section 21).  kind 'nv12' | 'bgr' and a surface as in draw_zones.  items: one (surface, width, camera,
    table) per surface.  state: the map's int32 device tensors dwell, visits [cameras, Gh, Gw] and peak [cameras, 2],
    read only.  palette: a uint8 device tensor [tables, 256, 3], 1 .. 8 tables of the 256 colours by level, stored or
    blended as they are.  size, cell: the map's; source 'dwell' | 'visits'; full_scale an integer 1 .. 2^31 - 1 or None
    (the map's peak, read on the device); alpha_max 0 .. 256, floor 0 .. 255.  Shapes, types and ranges raise
    ValueError before anything is asked of a device."""
    who = 'draw_heat'
    if kind not in ('nv12', 'bgr'):
        raise ValueError(f"{who}: kind {kind!r} is not 'nv12' or 'bgr'")
    items = list(items)
    if not items:
        raise ValueError(f'{who}: no surface')
    if any(not (isinstance(it, (tuple, list)) and len(it) == 4) for it in items):
        raise ValueError(f'{who}: an item is (surface, width, camera, table)')
    if source not in HEAT_SOURCES:
        raise ValueError(f'{who}: source is one of {", ".join(HEAT_SOURCES)}, got {source!r}')
    for name, v, lo, hi in (('alpha_max', alpha_max, 0, 256), ('floor', floor, 0, 255)):
        if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
            raise ValueError(f'{who}: {name} is an integer in {lo} .. {hi}, got {v!r}')
    if full_scale is not None and (isinstance(full_scale, bool) or not isinstance(full_scale, int)
                                   or not 1 <= full_scale <= 2 ** 31 - 1):
        raise ValueError(f'{who}: full_scale is None or an integer in 1 .. 2^31 - 1, got {full_scale!r}')
    cameras, _, Gw, Gh = _heat_state(who, state, ('peak', 'dwell', 'visits'), size, cell)
    if not (isinstance(palette, torch.Tensor) and palette.dtype == torch.uint8 and palette.dim() == 3
            and 1 <= palette.shape[0] <= native.HEAT_MAX_TABLES and tuple(palette.shape[1:]) == (256, 3)
            and palette.is_contiguous()):
        raise ValueError(f'{who}: palette is a contiguous uint8 [1 .. {native.HEAT_MAX_TABLES}, 256, 3] tensor')
    tables = palette.shape[0]
    geometry = _camera_surfaces(who, kind, items, cameras, tables)
    # the shapes are right: now where the tensors live
    dev = state['peak'].device
    if dev.type != 'cuda':
        raise ValueError(f'{who}: the state must be on a HIP device (pavenet_amd has no CPU path), got {dev}')
    if any(state[n].device != dev for n in ('dwell', 'visits')) or palette.device != dev:
        raise ValueError(f'{who}: the state tensors and the palette must be on one device ({dev})')
    for i, it in enumerate(items):
        if it[0].device != dev:
            raise ValueError(f"{who}: surface {i} is on {it[0].device}, the map on {dev}")
    entry = 'pave_draw_heat_nv12' if kind == 'nv12' else 'pave_draw_heat_bgr'
    for at in range(0, len(items), native.DRAW_MAX_SURFACES):
        plan = native.HeatDrawPlan()
        part = items[at:at + native.DRAW_MAX_SURFACES]
        for i, it in enumerate(part):
            plan.dst[i] = it[0].data_ptr()
            plan.pitch[i], plan.width[i], plan.height[i], plan.camera[i], plan.table[i] = geometry[at + i]
        plan.map, plan.peak, plan.palette = state[source].data_ptr(), state['peak'].data_ptr(), palette.data_ptr()
        plan.n, plan.cameras, plan.tables = len(part), cameras, tables
        plan.map_width, plan.map_height, plan.cell = int(size[0]), int(size[1]), cell
        plan.source, plan.full_scale = HEAT_SOURCES.index(source), 0 if full_scale is None else full_scale
        plan.alpha_max, plan.floor, plan.smooth = alpha_max, floor, 1 if smooth else 0
        _launch(entry, who, dev, ctypes.byref(plan))


_TRAIL_STATE = (('id', 1), ('last', 1), ('pos', 2), ('head', 1), ('count', 1), ('box', 3), ('pts', 4), ('when', 5),
                ('frame', 0), ('dropped', 0))
# name, kind: 0 [cameras], 1 [cameras, S], 2 [cameras, S, 2], 3 [cameras, S, 4], 4 [cameras, S, L, 2], 5 [cameras, S, L]


def _trail_state(who, state, names):
    """The shapes of the trails' tensors `names` of _TRAIL_STATE -> (cameras, S, L)."""
    if not isinstance(state, dict) or any(not isinstance(state.get(name), torch.Tensor) for name in names):
        raise ValueError(f'{who}: state holds the tensors {", ".join(names)}')
    if state['when'].dim() != 3:
        raise ValueError(f'{who}: state when must be [cameras, S, L], got {tuple(state["when"].shape)}')
    cameras, S, L = state['when'].shape
    if not (1 <= cameras <= native.TRACK_MAX_CAMERAS and 1 <= S <= native.TRACK_MAX_TRACKS
            and 1 <= L <= native.TRAIL_MAX_POINTS):
        raise ValueError(f'{who}: cameras in 1 .. {native.TRACK_MAX_CAMERAS}, S in 1 .. {native.TRACK_MAX_TRACKS} and L in '
                         f'1 .. {native.TRAIL_MAX_POINTS}, got {cameras}, {S} and {L}')
    for name, kind in _TRAIL_STATE:
        if name not in names:
            continue
        t = state[name]
        want = ((cameras,), (cameras, S), (cameras, S, 2), (cameras, S, 4), (cameras, S, L, 2), (cameras, S, L))[kind]
        if t.dtype != torch.int32 or tuple(t.shape) != want or not t.is_contiguous():
            raise ValueError(f'{who}: state {name} must be a contiguous int32 {list(want)} tensor')
    return cameras, S, L


def _int_in(who, name, v, lo, hi):
    if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
        raise ValueError(f'{who}: {name} must be an integer in {lo} .. {hi}, got {v!r}')


def trail_update(entries, state, *, K, stride=1, min_step=16, max_age=30, anchor='feet', anchor_kpts=(), score_thr=0.3,
                 kpt_thr=0.):
    """Track trails from frames of tracked poses, one launch per 32 frames (pave_trail_update; the rule is DESIGN
    section 22).  entries: what `zone_events` takes, one (kpts, bboxes, keep, ids, camera, (sx, sy)) per frame, the
    frames of one camera in time order; state: int32 device tensors id, last, head, count [cameras, S], pos [cameras,
    S, 2], box [cameras, S, 4], pts [cameras, S, L, 2], when [cameras, S, L] and frame, dropped [cameras], read and
    written (L 1 .. 64 is the ring's length); stride 1 .. 255 frames and min_step 0 .. 65535 eighths of a pixel between
    two committed points; anchor and anchor_kpts as in `zone_events`.  Returns one dict(count [N], span [N], dist [N],
    path [N]) of new int32 tensors per entry.  Shapes, types and ranges raise ValueError before anything is asked of a
    device."""
    who = 'trail_update'
    entries = list(entries)
    if isinstance(K, bool) or not isinstance(K, int) or not 1 <= K <= native.TRACK_MAX_K:
        raise ValueError(f'{who}: K must be an integer in 1 .. {native.TRACK_MAX_K}, got {K!r}')
    cameras, S, L = _trail_state(who, state, [n for n, _ in _TRAIL_STATE])
    _int_in(who, 'stride', stride, 1, native.TRAIL_MAX_STRIDE)
    _int_in(who, 'min_step', min_step, 0, native.TRAIL_MAX_STEP)
    max_age = _max_age(who, max_age)
    anchor = _anchor(who, anchor, anchor_kpts, K)
    checked = _tracked_entries(who, entries, K, cameras)
    # the shapes are right: now where the tensors live
    dev = state['when'].device
    _tracked_devices(who, dev, (state[n] for n, _ in _TRAIL_STATE), checked)
    names = ('count', 'span', 'dist', 'path')
    outs = [{n: torch.empty((c[7],), dtype=torch.int32, device=dev) for n in names} for c in checked]
    for at in range(0, len(checked), native.TRACK_MAX_FRAMES):
        plan = native.TrailPlan()
        part = checked[at:at + native.TRACK_MAX_FRAMES]
        _tracked_fill(plan, part, cameras, S, K, max_age, score_thr, kpt_thr, anchor)
        for i in range(len(part)):
            out = outs[at + i]
            plan.out_count[i], plan.out_span[i], plan.out_dist[i], plan.out_path[i] = (out[n].data_ptr() or None
                                                                                       for n in names)
        (plan.slot_id, plan.slot_last, plan.slot_pos, plan.slot_head, plan.slot_count, plan.slot_box, plan.pts, plan.when,
         plan.frame, plan.dropped) = (state[n].data_ptr() for n, _ in _TRAIL_STATE)
        plan.L, plan.stride, plan.min_step = L, stride, min_step
        _launch('pave_trail_update', who, dev, ctypes.byref(plan))
    return outs


def draw_trails(kind, items, state, palettes, *, thickness=3, thickness_tail=1, head_radius=0, tail_frames=None,
                linger=None):
    """Track trails drawn into surfaces in place, one launch per 32 surfaces (pave_draw_trails_nv12 / _bgr; the rule is
    DESIGN section 22).  kind 'nv12' | 'bgr' and a surface as in draw_zones.  items: one (surface, width, camera, table)
    per surface.  state: the trails' int32 device tensors (all of `trail_update`'s but dropped), read only.  palettes: 1
    .. 4 tables of 96 bytes, the 32 colours as they are stored: (Y, U, V) or (B, G, R); a track takes row (id - 1) % 32.
    thickness, thickness_tail 1 .. 32 pixels at the newest and the oldest end (thickness_tail <= thickness); head_radius
    0 .. 32; tail_frames None or 1 .. 2^30; linger None or 0 .. 2^30.  Shapes, types and ranges raise ValueError before
    anything is asked of a device."""
    who = 'draw_trails'
    if kind not in ('nv12', 'bgr'):
        raise ValueError(f"{who}: kind {kind!r} is not 'nv12' or 'bgr'")
    items = list(items)
    if not items:
        raise ValueError(f'{who}: no surface')
    if any(not (isinstance(it, (tuple, list)) and len(it) == 4) for it in items):
        raise ValueError(f'{who}: an item is (surface, width, camera, table)')
    _int_in(who, 'thickness', thickness, 1, native.TRAIL_MAX_THICKNESS)
    _int_in(who, 'thickness_tail', thickness_tail, 1, thickness)
    _int_in(who, 'head_radius', head_radius, 0, native.TRAIL_MAX_RADIUS)
    if tail_frames is not None:
        _int_in(who, 'tail_frames', tail_frames, 1, native.TRAIL_MAX_FRAMES)
    if linger is not None:
        _int_in(who, 'linger', linger, 0, native.TRAIL_MAX_FRAMES)
    names = [n for n, _ in _TRAIL_STATE if n != 'dropped']
    cameras, S, L = _trail_state(who, state, names)
    palettes = list(palettes)
    if not 1 <= len(palettes) <= native.DRAW_MAX_TABLES or any(
            not isinstance(p, (bytes, bytearray)) or len(p) != 3 * native.DRAW_PALETTE for p in palettes):
        raise ValueError(f'{who}: palettes are 1 .. {native.DRAW_MAX_TABLES} tables of {3 * native.DRAW_PALETTE} bytes')
    geometry = _camera_surfaces(who, kind, items, cameras, len(palettes))
    # the shapes are right: now where the tensors live
    dev = state['when'].device
    if dev.type != 'cuda':
        raise ValueError(f'{who}: the state must be on a HIP device (pavenet_amd has no CPU path), got {dev}')
    if any(state[n].device != dev for n in names):
        raise ValueError(f'{who}: the state tensors must be on one device ({dev})')
    for i, it in enumerate(items):
        if it[0].device != dev:
            raise ValueError(f"{who}: surface {i} is on {it[0].device}, the trails on {dev}")
    entry = 'pave_draw_trails_nv12' if kind == 'nv12' else 'pave_draw_trails_bgr'
    for at in range(0, len(items), native.DRAW_MAX_SURFACES):
        plan = native.TrailDrawPlan()
        part = items[at:at + native.DRAW_MAX_SURFACES]
        for i, it in enumerate(part):
            plan.dst[i] = it[0].data_ptr()
            plan.pitch[i], plan.width[i], plan.height[i], plan.camera[i], plan.table[i] = geometry[at + i]
        (plan.slot_id, plan.slot_last, plan.slot_pos, plan.slot_head, plan.slot_count, plan.slot_box, plan.pts, plan.when,
         plan.frame) = (state[n].data_ptr() for n in names)
        for t, p in enumerate(palettes):
            ctypes.memmove(plan.palette[t], bytes(p), len(p))
        plan.n, plan.cameras, plan.S, plan.L = len(part), cameras, S, L
        plan.thickness, plan.thickness_tail, plan.head_radius = thickness, thickness_tail, head_radius
        plan.tail_frames, plan.linger = 0 if tail_frames is None else tail_frames, -1 if linger is None else linger
        _launch(entry, who, dev, ctypes.byref(plan))


_FLOOR_STATE = (('id', 1), ('last', 1), ('hits', 1), ('pos', 2), ('vel', 2), ('travel', 1), ('frame', 0), ('dropped', 0))
# name, kind: 0 [cameras], 1 [cameras, S], 2 [cameras, S, 2]
FLOOR_OUTPUTS = (('on', 1), ('xy', 2), ('vel', 2), ('speed', 1), ('travel', 1), ('nearest', 1), ('gap', 1), ('near', 1))
# name, words per pose: the sections of one launch output, one after the other


def floor_update(entries, state, calib, *, K, velocity_gain=4, near=1500, unit=10, origin=(0, 0), max_age=30,
                 anchor='feet', anchor_kpts=(), score_thr=0.3, kpt_thr=0.):
    """Floor positions, speeds and neighbours from frames of tracked poses, one launch per 32 frames
    (pave_floor_update; the rule is DESIGN section 23).  entries: what `zone_events` takes, one (kpts, bboxes, keep,
    ids, camera, (sx, sy)) per frame, the frames of one camera in time order; state: int32 device tensors id, last,
    hits, travel [cameras, S], pos, vel [cameras, S, 2] and frame, dropped [cameras], read and written; calib: the int64
    [cameras, 16] device tensor of the calibrations, read; velocity_gain 1 .. 16, near 0 .. 2^20 mm, unit 1 .. 1000 mm
    per floor pixel, origin (x, y) in mm within +-(2^20 - 1); anchor and anchor_kpts as in `zone_events`.  Returns one
    dict per entry of new tensors: int32 on, speed, travel, nearest, gap, near [N] and xy, vel [N, 2], and float32 kpts
    [N, K, 3] and bboxes [N, 5], the poses in floor units.  Shapes, types and ranges raise ValueError before anything
    is asked of a device."""
    who = 'floor_update'
    entries = list(entries)
    if isinstance(K, bool) or not isinstance(K, int) or not 1 <= K <= native.TRACK_MAX_K:
        raise ValueError(f'{who}: K must be an integer in 1 .. {native.TRACK_MAX_K}, got {K!r}')
    names = [n for n, _ in _FLOOR_STATE]
    if not isinstance(state, dict) or any(not isinstance(state.get(name), torch.Tensor) for name in names):
        raise ValueError(f'{who}: state holds the tensors {", ".join(names)}')
    if state['id'].dim() != 2:
        raise ValueError(f'{who}: state id must be [cameras, S], got {tuple(state["id"].shape)}')
    cameras, S = state['id'].shape
    if not (1 <= cameras <= native.TRACK_MAX_CAMERAS and 1 <= S <= native.TRACK_MAX_TRACKS):
        raise ValueError(f'{who}: cameras in 1 .. {native.TRACK_MAX_CAMERAS} and S in 1 .. {native.TRACK_MAX_TRACKS}, got '
                         f'{cameras} and {S}')
    for name, kind in _FLOOR_STATE:
        t, want = state[name], ((cameras,), (cameras, S), (cameras, S, 2))[kind]
        if t.dtype != torch.int32 or tuple(t.shape) != want or not t.is_contiguous():
            raise ValueError(f'{who}: state {name} must be a contiguous int32 {list(want)} tensor')
    if not (isinstance(calib, torch.Tensor) and calib.dtype == torch.int64 and calib.is_contiguous()
            and tuple(calib.shape) == (cameras, native.FLOOR_CALIB_WORDS)):
        raise ValueError(f'{who}: calib must be a contiguous int64 [{cameras}, {native.FLOOR_CALIB_WORDS}] tensor')
    _int_in(who, 'velocity_gain', velocity_gain, 1, native.FLOOR_MAX_GAIN)
    _int_in(who, 'near', near, 0, native.FLOOR_MAX_NEAR)
    _int_in(who, 'unit', unit, 1, native.FLOOR_MAX_UNIT)
    if not (isinstance(origin, (tuple, list)) and len(origin) == 2):
        raise ValueError(f'{who}: origin is (x, y) in mm, got {origin!r}')
    for v in origin:
        _int_in(who, 'origin', v, -native.FLOOR_MAX_MM, native.FLOOR_MAX_MM)
    max_age = _max_age(who, max_age)
    anchor = _anchor(who, anchor, anchor_kpts, K)
    checked = _tracked_entries(who, entries, K, cameras)
    # the shapes are right: now where the tensors live
    dev = state['id'].device
    _tracked_devices(who, dev, [calib] + [state[n] for n in names], checked, 'the state tensors and calib')
    words = [torch.empty((native.FLOOR_OUT_WORDS * c[7],), dtype=torch.int32, device=dev) for c in checked]
    floats = [torch.empty((c[7] * (K * 3 + 5),), dtype=torch.float32, device=dev) for c in checked]
    for at in range(0, len(checked), native.TRACK_MAX_FRAMES):
        plan = native.FloorPlan()
        part = checked[at:at + native.TRACK_MAX_FRAMES]
        _tracked_fill(plan, part, cameras, S, K, max_age, score_thr, kpt_thr, anchor)
        for i in range(len(part)):
            plan.out[i], plan.out_floor[i] = words[at + i].data_ptr() or None, floats[at + i].data_ptr() or None
        (plan.slot_id, plan.slot_last, plan.slot_hits, plan.slot_pos, plan.slot_vel, plan.slot_travel, plan.frame,
         plan.dropped) = (state[n].data_ptr() for n in names)
        plan.calib = calib.data_ptr()
        plan.velocity_gain, plan.near, plan.unit = velocity_gain, near, unit
        plan.origin_x, plan.origin_y = origin
        _launch('pave_floor_update', who, dev, ctypes.byref(plan))
    outs = []
    for c, w, f in zip(checked, words, floats):
        N, at, out = c[7], 0, {}
        for name, per in FLOOR_OUTPUTS:
            out[name] = w[at:at + per * N].view((N,) if per == 1 else (N, per))
            at += per * N
        out['kpts'], out['bboxes'] = f[:N * K * 3].view(N, K, 3), f[N * K * 3:].view(N, 5)
        outs.append(out)
    return outs


_CONTACT_STATE = (('id', 1), ('last', 1), ('pos', 2), ('link', 3), ('since', 3), ('frame', 0), ('dropped', 0),
                  ('counters', 4))
# name, kind: 0 [cameras], 1 [cameras, S], 2 [cameras, S, 2], 3 [cameras, S, S], 4 [cameras, 8]
CONTACT_OUTPUTS = ('group', 'size', 'contacts', 'partner', 'together')      # the [N] sections of one launch output


def contact_update(entries, state, *, radius=1500, release=None, min_frames=3, long_frames=0, max_events=256,
                   max_age=30):
    """Debounced pair contacts, their durations, the groups they form and the frame's events from frames of floor
    positions, one launch per 32 frames (pave_contact_update; the rule is DESIGN section 24).  entries: one (on [N]
    int32, xy [N, 2] int32 mm, ids [N] int32, camera) per frame -- `floor_update`'s on and xy and the frame's track ids
    -- N <= 128, the frames of one camera in time order; state: int32 device tensors id, last [cameras, S], pos
    [cameras, S, 2], link, since [cameras, S, S], frame, dropped [cameras] and counters [cameras, 8]
    (PAVE_CONTACT_CNT_* of include/pave_hip.h), read and written; radius 0 .. 2^20 mm, release radius .. 2^21 mm (None:
    radius), min_frames 1 .. 255, long_frames 0 .. 2^30 (0: never), max_events 1 .. 4096.  Returns one dict(group, size,
    contacts, partner, together [N], events [max_events, 7], n_events 0-d) per entry, int32 views of one new
    allocation.  Shapes, types and ranges raise ValueError before anything is asked of a device."""
    who = 'contact_update'
    entries = list(entries)
    names = [n for n, _ in _CONTACT_STATE]
    if not isinstance(state, dict) or any(not isinstance(state.get(name), torch.Tensor) for name in names):
        raise ValueError(f'{who}: state holds the tensors {", ".join(names)}')
    if state['id'].dim() != 2:
        raise ValueError(f'{who}: state id must be [cameras, S], got {tuple(state["id"].shape)}')
    cameras, S = state['id'].shape
    if not (1 <= cameras <= native.TRACK_MAX_CAMERAS and 1 <= S <= native.TRACK_MAX_TRACKS):
        raise ValueError(f'{who}: cameras in 1 .. {native.TRACK_MAX_CAMERAS} and S in 1 .. {native.TRACK_MAX_TRACKS}, got '
                         f'{cameras} and {S}')
    for name, kind in _CONTACT_STATE:
        t = state[name]
        want = ((cameras,), (cameras, S), (cameras, S, 2), (cameras, S, S), (cameras, native.CONTACT_COUNTER_WORDS))[kind]
        if t.dtype != torch.int32 or tuple(t.shape) != want or not t.is_contiguous():
            raise ValueError(f'{who}: state {name} must be a contiguous int32 {list(want)} tensor')
    _int_in(who, 'radius', radius, 0, native.CONTACT_MAX_RADIUS)
    if release is None:
        release = radius
    _int_in(who, 'release', release, radius, native.CONTACT_MAX_RELEASE)
    _int_in(who, 'min_frames', min_frames, 1, 255)
    _int_in(who, 'long_frames', long_frames, 0, native.CONTACT_MAX_LONG)
    _int_in(who, 'max_events', max_events, 1, native.CONTACT_MAX_EVENTS)
    max_age = _max_age(who, max_age)
    checked = []
    for i, entry in enumerate(entries):
        if not (isinstance(entry, (tuple, list)) and len(entry) == 4):
            raise ValueError(f'{who}: entry {i} is (on, xy, ids, camera)')
        on, xy, ids, camera = entry
        if not (isinstance(on, torch.Tensor) and on.dtype == torch.int32 and on.dim() == 1):
            raise ValueError(f'{who}: on of entry {i} must be a [N] int32 tensor')
        N = on.shape[0]
        if not (isinstance(xy, torch.Tensor) and xy.dtype == torch.int32 and tuple(xy.shape) == (N, 2)):
            raise ValueError(f'{who}: xy of entry {i} must be a [{N}, 2] int32 tensor')
        if not (isinstance(ids, torch.Tensor) and ids.dtype == torch.int32 and tuple(ids.shape) == (N,)):
            raise ValueError(f'{who}: ids of entry {i} must be a [{N}] int32 tensor')
        if N > native.TRACK_MAX_POSES:
            raise ValueError(f'{who}: entry {i} has {N} poses, at most {native.TRACK_MAX_POSES}')
        if isinstance(camera, bool) or int(camera) != camera or not 0 <= camera < cameras:
            raise ValueError(f'{who}: the camera of entry {i} must be an integer in [0, {cameras}), got {camera!r}')
        if not (on.is_contiguous() and xy.is_contiguous() and ids.is_contiguous()):
            raise ValueError(f'{who}: the tensors of entry {i} must be contiguous')
        checked.append((on, xy, ids, int(camera), N))
    # the shapes are right: now where the tensors live
    dev = state['id'].device
    if not dev.type == 'cuda':
        raise ValueError(f'{who}: the state must be on a HIP device (pavenet_amd has no CPU path), got {dev}')
    if any(state[n].device != dev for n in names):
        raise ValueError(f'{who}: the state tensors must be on one device ({dev})')
    for i, c in enumerate(checked):
        if c[0].device != dev or c[1].device != dev or c[2].device != dev:
            raise ValueError(f'{who}: the tensors of entry {i} must be on the HIP device of the state ({dev})')
    OW, EW = native.CONTACT_OUT_WORDS, native.CONTACT_EVENT_WORDS
    words = [torch.empty((OW * c[4] + EW * max_events + 1,), dtype=torch.int32, device=dev) for c in checked]
    for at in range(0, len(checked), native.TRACK_MAX_FRAMES):
        plan = native.ContactPlan()
        part = checked[at:at + native.TRACK_MAX_FRAMES]
        for i, (on, xy, ids, camera, N) in enumerate(part):
            base = words[at + i].data_ptr()
            plan.on[i], plan.xy[i], plan.ids[i] = on.data_ptr() or None, xy.data_ptr() or None, ids.data_ptr() or None
            plan.out[i] = base if N else None
            plan.out_events[i], plan.out_n_events[i] = base + 4 * OW * N, base + 4 * (OW * N + EW * max_events)
            plan.n[i], plan.camera[i] = N, camera
        (plan.slot_id, plan.slot_last, plan.slot_pos, plan.link, plan.since, plan.frame, plan.dropped,
         plan.counters) = (state[n].data_ptr() for n in names)
        plan.entries, plan.cameras, plan.S, plan.max_age = len(part), cameras, S, max_age
        plan.radius, plan.release, plan.min_frames = radius, release, min_frames
        plan.long_frames, plan.max_events = long_frames, max_events
        _launch('pave_contact_update', who, dev, ctypes.byref(plan))
    outs = []
    for c, w in zip(checked, words):
        N = c[4]
        out = {name: w[i * N:(i + 1) * N] for i, name in enumerate(CONTACT_OUTPUTS)}
        out['events'] = w[OW * N:OW * N + EW * max_events].view(max_events, EW)
        out['n_events'] = w[OW * N + EW * max_events]
        outs.append(out)
    return outs


_REID_STATE =(('person', 1), ('track', 1), ('last', 1), ('hits', 2), ('hist', 3), ('frame', 0), ('next', 0),
               ('dropped', 0))   # name, kind: 0 [cameras], 1 [cameras, S], 2 [cameras, S, 2], 3 [cameras, S, 2, 256]


def reid_scratch(device):
    """The areas pave_reid_update_* works in, allocated once per gallery: the descriptors (8 MiB), the sample counts
    and the pair scores (2 MiB) of the 32 entries of a launch."""
    F, P, S = native.TRACK_MAX_FRAMES, native.TRACK_MAX_POSES, native.TRACK_MAX_TRACKS
    z = dict(dtype=torch.int32, device=device)
    return dict(hist=torch.empty((F, P, 2, native.REID_BINS), **z), count=torch.empty((F, P, 2), **z),
                pairs=torch.empty((F, P, S), **z))


def _reid_items(who, kind, items, K, parts):
    """The checks reid_describe and reid_update share, all ValueError -> (geometry, parts)."""
    if kind not in ('nv12', 'bgr'):
        raise ValueError(f"{who}: kind {kind!r} is not 'nv12' or 'bgr'")
    if isinstance(K, bool) or not isinstance(K, int) or not 1 <= K <= native.TRACK_MAX_K:
        raise ValueError(f'{who}: K must be an integer in 1 .. {native.TRACK_MAX_K}, got {K!r}')
    try:
        parts = [[[k for k in half] for half in region] for region in parts]
    except TypeError:
        parts = []
    if len(parts) != 2 or any(len(region) != 2 for region in parts):
        raise ValueError(f'{who}: parts is ((torso upper, torso lower), (legs upper, legs lower)) index lists')
    for region in parts:
        for half in region:
            if len(half) > native.REID_MAX_PART or any(isinstance(k, bool) or not isinstance(k, int) or not 0 <= k < K
                                                       for k in half):
                raise ValueError(f'{who}: a part holds at most {native.REID_MAX_PART} integers in [0, {K}), got {half!r}')
    geometry = _surface_geometry(who, kind, [tuple(it[:6]) + (0,) for it in items], K, 1)
    for i, g in enumerate(geometry):
        if g[3] > native.TRACK_MAX_POSES:
            raise ValueError(f'{who}: entry {i} has {g[3]} poses, at most {native.TRACK_MAX_POSES}')
    return geometry, parts


def _reid_fill(d, part, geometry, hists, counts, K, parts, score_thr, kpt_thr):
    """A pave_reid_describe_plan for the entries `part`."""
    for i, it in enumerate(part):
        pitch, W, H, N, sx, sy, _ = geometry[i]
        d.src[i], d.kpts[i], d.bboxes[i], d.keep[i] = it[0].data_ptr(), _ptr(it[2]) or None, _ptr(it[3]) or None, \
            _ptr(it[4]) or None
        d.hist[i], d.count[i] = hists[i], counts[i]
        d.pitch[i], d.width[i], d.height[i], d.n[i], d.scale[i][0], d.scale[i][1] = pitch, W, H, N, sx, sy
    for r, region in enumerate(parts):
        for h, half in enumerate(region):
            d.n_part[r][h] = len(half)
            for i, k in enumerate(half):
                d.part[r][h][i] = k
    d.entries, d.K, d.score_thr, d.kpt_thr = len(part), K, float(score_thr), float(kpt_thr)


def reid_describe(kind, items, K, parts, *, score_thr=0.3, kpt_thr=0.):
    """The colour descriptors of the poses on surfaces, one launch per 32 surfaces (pave_reid_describe_nv12 / _bgr; the
    rule is DESIGN section 18).  kind and items: (surface, width, kpts, bboxes, keep, (sx, sy)) as in draw_poses, at
    most 128 poses each; parts ((torso upper, torso lower), (legs upper, legs lower)): at most 4 key points each.
    Returns one dict(hist [N, 2, 256], count [N, 2]) of new int32 tensors per item; the surfaces are only read.
    Shapes, types and ranges raise ValueError before anything is asked of a device."""
    who = 'reid_describe'
    items = list(items)
    geometry, parts = _reid_items(who, kind, items, K, parts)
    dev = items[0][0].device
    if dev.type != 'cuda':
        raise ValueError(f'{who}: surface 0 must be on a HIP device (pavenet_amd has no CPU path), got {dev}')
    for i, it in enumerate(items):
        if any(t is not None and (t.device != dev or not t.is_contiguous()) for t in (it[0], it[2], it[3], it[4])):
            raise ValueError(f'{who}: the tensors of entry {i} must be contiguous and on one HIP device ({dev})')
    z = dict(dtype=torch.int32, device=dev)
    outs = [dict(hist=torch.empty((g[3], 2, native.REID_BINS), **z), count=torch.empty((g[3], 2), **z)) for g in geometry]
    pad = torch.empty((1,), **z)    # (an empty tensor has no address; the entry asks for one)
    for at in range(0, len(items), native.TRACK_MAX_FRAMES):
        plan = native.ReidDescribePlan()
        part = items[at:at + native.TRACK_MAX_FRAMES]
        o = outs[at:at + native.TRACK_MAX_FRAMES]
        _reid_fill(plan, part, geometry[at:], [v['hist'].data_ptr() or pad.data_ptr() for v in o],
                   [v['count'].data_ptr() or pad.data_ptr() for v in o], K, parts, score_thr, kpt_thr)
        _launch('pave_reid_describe_' + kind, who, dev, ctypes.byref(plan))
    return outs


def reid_update(kind, entries, state, scratch, K, parts, *, max_lost=900, match_thr, min_hits=3, gain=2, score_thr=0.3,
                kpt_thr=0.):
    """Person ids for frames of tracked poses, two launches per 32 frames (pave_reid_update_nv12 / _bgr; the rule is
    DESIGN section 18).  entries: one (surface, width, kpts, bboxes, keep, (sx, sy), ids [N] int32, camera) per frame,
    N <= 128, the frames of one camera in time order; state: int32 device tensors person, track, last [cameras, S],
    hits [cameras, S, 2], hist [cameras, S, 2, 256], frame, next, dropped [cameras], read and written; scratch:
    reid_scratch().  Returns one dict(ids [N], sim [N]) of new int32 tensors per entry.  Shapes, types and ranges
    raise ValueError before anything is asked of a device."""
    who = 'reid_update'
    entries = list(entries)
    if not isinstance(state, dict) or any(not isinstance(state.get(name), torch.Tensor) for name, _ in _REID_STATE):
        raise ValueError(f'{who}: state holds the tensors {", ".join(n for n, _ in _REID_STATE)}')
    if state['person'].dim() != 2:
        raise ValueError(f'{who}: state person must be [cameras, S], got {tuple(state["person"].shape)}')
    cameras, S = state['person'].shape
    if not (1 <= cameras <= native.TRACK_MAX_CAMERAS and 1 <= S <= native.TRACK_MAX_TRACKS):
        raise ValueError(f'{who}: cameras in 1 .. {native.TRACK_MAX_CAMERAS} and S in 1 .. {native.TRACK_MAX_TRACKS}, got '
                         f'{cameras} and {S}')
    dev = state['person'].device
    for name, kind_ in _REID_STATE:
        t = state[name]
        want = ((cameras,), (cameras, S), (cameras, S, 2), (cameras, S, 2, native.REID_BINS))[kind_]
        if t.dtype != torch.int32 or tuple(t.shape) != want or not t.is_contiguous():
            raise ValueError(f'{who}: state {name} must be a contiguous int32 {list(want)} tensor')
    for name, v, lo, hi in (('match_thr', match_thr, 0, native.REID_NEVER), ('min_hits', min_hits, 1, native.REID_MAX_HITS),
                            ('gain', gain, 1, 16)):
        if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
            raise ValueError(f'{who}: {name} must be an integer in {lo} .. {hi}, got {v!r}')
    if isinstance(max_lost, bool) or int(max_lost) != max_lost or max_lost < 0:
        raise ValueError(f'{who}: max_lost must be an integer >= 0, got {max_lost!r}')
    if any(not (isinstance(it, (tuple, list)) and len(it) == 8) for it in entries):
        raise ValueError(f'{who}: an entry is (surface, width, kpts, bboxes, keep, (sx, sy), ids, camera)')
    geometry, parts = _reid_items(who, kind, entries, K, parts)
    for i, (it, g) in enumerate(zip(entries, geometry)):
        ids, camera = it[6], it[7]
        if not (isinstance(ids, torch.Tensor) and ids.dtype == torch.int32 and tuple(ids.shape) == (g[3],)
                and ids.is_contiguous()):
            raise ValueError(f'{who}: ids of entry {i} must be a contiguous [{g[3]}] int32 tensor')
        if isinstance(camera, bool) or int(camera) != camera or not 0 <= camera < cameras:
            raise ValueError(f'{who}: the camera of entry {i} must be an integer in [0, {cameras}), got {camera!r}')
    want = reid_scratch('meta')
    if not isinstance(scratch, dict) or any(
            not isinstance(scratch.get(n), torch.Tensor) or scratch[n].shape != want[n].shape
            or scratch[n].dtype != torch.int32 or not scratch[n].is_contiguous() for n in want):
        raise ValueError(f'{who}: scratch is what reid_scratch() returns')
    # the shapes are right: now where the tensors live
    if dev.type != 'cuda':
        raise ValueError(f'{who}: the state must be on a HIP device (pavenet_amd has no CPU path), got {dev}')
    if any(state[n].device != dev for n, _ in _REID_STATE) or any(scratch[n].device != dev for n in want):
        raise ValueError(f'{who}: the state and scratch tensors must be on one device ({dev})')
    for i, it in enumerate(entries):
        if any(t is not None and (t.device != dev or not t.is_contiguous()) for t in (it[0], it[2], it[3], it[4], it[6])):
            raise ValueError(f'{who}: the tensors of entry {i} must be contiguous and on the HIP device of the state ({dev})')
    z = dict(dtype=torch.int32, device=dev)
    outs = [dict(ids=torch.empty((g[3],), **z), sim=torch.empty((g[3],), **z)) for g in geometry]
    hist_at, count_at = scratch['hist'].data_ptr(), scratch['count'].data_ptr()
    hist_step, count_step = scratch['hist'][0].numel() * 4, scratch['count'][0].numel() * 4
    for at in range(0, len(entries), native.TRACK_MAX_FRAMES):
        plan = native.ReidPlan()
        part = entries[at:at + native.TRACK_MAX_FRAMES]
        _reid_fill(plan.d, part, geometry[at:], [hist_at + i * hist_step for i in range(len(part))],
                   [count_at + i * count_step for i in range(len(part))], K, parts, score_thr, kpt_thr)
        for i, it in enumerate(part):
            out = outs[at + i]
            plan.ids[i], plan.out_ids[i], plan.out_sim[i] = it[6].data_ptr() or None, out['ids'].data_ptr() or None, \
                out['sim'].data_ptr() or None
            plan.camera[i] = int(it[7])
        (plan.person, plan.track, plan.last, plan.hits, plan.hist, plan.frame, plan.next, plan.dropped) = (
            state[n].data_ptr() for n, _ in _REID_STATE)
        plan.pairs = scratch['pairs'].data_ptr()
        plan.cameras, plan.S, plan.max_lost, plan.match_thr = cameras, S, int(max_lost), match_thr
        plan.min_hits, plan.gain = min_hits, gain
        _launch('pave_reid_update_' + kind, who, dev, ctypes.byref(plan))
    return outs


def fuse_sum_nhwc(terms, relu=True):
    """HRNet fuse layer in one pass (pave_fuse_sum_nhwc_f32): terms = [(map, shift), ...] (1..4), map
    [N, C, H >> shift, W >> shift] fp32 channels_last; returns relu(sum of the maps, the coarser ones
    read through a nearest-neighbour up-sampling by 2^shift) [N, C, H, W] channels_last, summed in
    the order given (hrnet.py:197-214)."""
    _require(1 <= len(terms) <= 4, 'fuse_sum_nhwc: 1..4 terms')
    t0, s0 = terms[0]
    N, C = t0.shape[0], t0.shape[1]
    H, W = t0.shape[2] << s0, t0.shape[3] << s0
    args = []
    for t, sh in terms:
        _require(t.is_cuda and t.dtype == torch.float32 and t.dim() == 4
                 and t.is_contiguous(memory_format=torch.channels_last)
                 and tuple(t.shape) == (N, C, H >> sh, W >> sh) and (H >> sh) << sh == H
                 and (W >> sh) << sh == W,
                 'fuse_sum_nhwc: terms [N, C, H >> s, W >> s] fp32 channels_last')
        args += [t.data_ptr(), int(sh)]
    args += [None, 0] * (4 - len(terms))
    y = torch.empty((N, H, W, C), dtype=torch.float32, device=t0.device)
    _launch('pave_fuse_sum_nhwc_f32', 'fuse_sum_nhwc', t0.device, *args, y.data_ptr(), N, H, W, C, int(bool(relu)),
            tag='fuse_sum')
    return y.permute(0, 3, 1, 2)


def bias_act_rows_(x, bias=None, res=None, relu=True):
    """In place: x[r, c] = act(x[r, c] + bias[c] + res[r, c]) over the last (channel) dim.
    `x` must be dense with channels innermost (token matrix, or an NHWC / channels_last map)."""
    _require(x.is_cuda and x.dtype == torch.float32, 'bias_act_rows_: fp32 device tensor')
    # (a 1x1 map [N, C, 1, 1] is dense in both layouts: its rows are the N pixels' channels either way)
    nhwc = x.dim() == 4 and x.is_contiguous(memory_format=torch.channels_last) \
        and (not x.is_contiguous() or (x.shape[2] == 1 and x.shape[3] == 1))
    C = bias.numel() if bias is not None else (x.shape[1] if nhwc else x.shape[-1])
    if nhwc:
        _require(x.shape[1] == C, 'bias_act_rows_: channel mismatch')
        if res is not None:
            _require(res.shape == x.shape and res.is_contiguous(memory_format=torch.channels_last),
                     'bias_act_rows_: residual layout mismatch')
    else:
        _require(x.is_contiguous() and x.shape[-1] == C, 'bias_act_rows_: channels must be innermost')
        if res is not None:
            _require(res.shape == x.shape and res.is_contiguous(), 'bias_act_rows_: residual layout')
    rows = x.numel() // C
    _launch('pave_bias_act_rows_f32', 'bias_act_rows', x.device,
            x.data_ptr(), _ptr(bias), _ptr(res), x.data_ptr(), rows, C, int(bool(relu)), tag='bias_act_rows')
    return x


def fill_rows_(x, rows, values=None):
    """x[rows] = values (zeros when None), in place: x [R, C] fp32 (a row-strided view is fine), rows int32
    indices on the device, values [C] -- pave_fill_rows_f32."""
    _require(x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1,
             'fill_rows_: x [R, C] fp32 on the device, unit column stride')
    _dev(rows, 'rows', torch.int32)
    if values is not None:
        _dev(values, 'values', torch.float32)
        _require(values.numel() == x.shape[1], 'fill_rows_: values [C]')
    _launch('pave_fill_rows_f32', 'fill_rows_', x.device, x.data_ptr(), x.stride(0), x.shape[0], rows.data_ptr(),
            rows.numel(), _ptr(values), x.shape[1])
    return x


def bias_add_layernorm(x, bias, res, gamma, beta, eps=1e-5, pos=None):
    """LayerNorm(x + bias + res) over the last dim; x / res dense row-major [..., C].
    With pos ([P, C] rows, P dividing the row count pattern r % P): returns (y, y + pos) from the
    same pass (the next layer's `query + query_pos`)."""
    _dev(x, 'x', torch.float32)
    C = x.shape[-1]
    if res is not None:
        _require(res.shape == x.shape and res.is_contiguous() and res.dtype == torch.float32,
                 'bias_add_layernorm: residual must match x')
    out = torch.empty_like(x)
    rows = x.numel() // C
    if pos is None:
        _launch('pave_bias_add_layernorm_f32', 'bias_add_layernorm', x.device,
                x.data_ptr(), _ptr(bias), _ptr(res), gamma.data_ptr(), beta.data_ptr(), out.data_ptr(), rows, C,
                float(eps), tag='bias_add_layernorm')
        return out
    _dev(pos, 'pos', torch.float32)
    _require(pos.shape[-1] == C and rows % (pos.numel() // C) == 0,
             'bias_add_layernorm: pos [P, C] with P dividing the number of rows')
    out_plus = torch.empty_like(x)
    _launch('pave_bias_add_layernorm_pos_f32', 'bias_add_layernorm', x.device,
            x.data_ptr(), _ptr(bias), _ptr(res), gamma.data_ptr(), beta.data_ptr(), out.data_ptr(),
            pos.data_ptr(), pos.numel() // C, out_plus.data_ptr(), rows, C, float(eps), tag='bias_add_layernorm')
    return out, out_plus


def enc_tile_supported(levels_hw):
    """The LDS-tile encoder kernel covers 4-level halving pyramids: every token of level l sits
    in exactly one 8 x 8-pixel image tile (H_l <= (8 >> l) * ceil(H_0 / 8), same for W)."""
    if len(levels_hw) != 4:
        return False
    ny, nx = (int(levels_hw[0][0]) + 7) // 8, (int(levels_hw[0][1]) + 7) // 8
    return all(int(h) <= (8 >> l) * ny and int(w) <= (8 >> l) * nx
               for l, (h, w) in enumerate(levels_hw))


def enc_tile_window_shift(offset_bias):
    """Window shift table for `deform_attn_enc_tile` from a `sampling_offsets.bias` [8*4*4*2]: the
    mean offset of each (head, level) over its 4 points, rounded -> tuple of 64 ints (host values:
    one device read, cache it per bias version)."""
    m = offset_bias.detach().float().view(8, 4, 4, 2).mean(2).round().clamp_(-16, 16)
    return tuple(int(v) for v in m.flatten().tolist())


def gemm_bf16x3_encproj(a, w_planes, table, ref, levels_hw, value_bias=None, out=None):
    """The encoder layer's merged N = 640 projection with the sampler's softmax / location
    arithmetic in the GEMM epilogue (pave_gemm_bf16x3_encproj_f32): a [M, K], w_planes = 3-plane
    split of the [640, K] weight, table [rows, 640] (row m adds table[m % rows]), ref [M, 4, 2]
    -> (value [M, 256], samp [M, 384]): samp = level pixel coordinates + attention weights, the
    `prepared=True` input of deform_attn_enc_tile.  value_bias [256]: added to the value columns
    instead of table[:, :256] (not read then: value_proj has no positional term)."""
    for t, nm in ((a, 'a'), (table, 'table'), (ref, 'ref')):
        _dev(t, nm, torch.float32)
    npl = _planes(w_planes, only=_Q_PLANES)
    M, K = a.shape
    _require(w_planes.shape[2] == 640 and w_planes.shape[0] * 16 == K,
             'gemm_bf16x3_encproj: w_planes [K/16, planes, 640, 16]')
    _require(table.dim() == 2 and table.shape[1] == 640 and ref.numel() == M * 8,
             'gemm_bf16x3_encproj: table [rows, 640], ref [M, 4, 2]')
    _require(len(levels_hw) == 4, 'gemm_bf16x3_encproj: four (h, w) levels')
    if value_bias is not None:
        _dev(value_bias, 'value_bias', torch.float32)
        _require(value_bias.numel() == 256 and value_bias.is_contiguous(), 'gemm_bf16x3_encproj: value_bias [256]')
    hw_arr = (ctypes.c_int * 8)(*[int(v) for hw in levels_hw for v in hw])
    if out is not None:     # (value [M, 256], samp [M, 384]) given: row slices of larger dense matrices
        value, samp = out
        _dev(value, 'out value', torch.float32)
        _dev(samp, 'out samp', torch.float32)
        _require(tuple(value.shape) == (M, 256) and tuple(samp.shape) == (M, 384), 'gemm_bf16x3_encproj: out shapes')
    else:
        value = torch.empty((M, 256), dtype=torch.float32, device=a.device)
        samp = torch.empty((M, 384), dtype=torch.float32, device=a.device)
    _launch('pave_gemm_bf16x3_encproj_f32', 'gemm_bf16x3_encproj', a.device,
            a.data_ptr(), w_planes.data_ptr(), table.data_ptr(), table.shape[0], _ptr(value_bias), ref.data_ptr(),
            ctypes.cast(hw_arr, ctypes.c_void_p), value.data_ptr(), samp.data_ptr(), M, K, npl,
            tag='gemm_bf16x3', flops=2 * M * K * 640, shape=(M, K, 640, 'encproj'))
    return value, samp


def deform_attn_enc_tile(value, proj, ref, *, levels_hw, variant=0, window_shift=None, prepared=False,
                         out_half=False):
    """Encoder deformable attention ([R2], T = 1) with LDS-staged value windows per image tile.
    value [F, S, 8, 32]; proj [F*S, >= 384]; ref [.., F*S, 4, 2] -> out [F*S, 256].
    Same results as ``deform_attn_grid_fused(..., T=1)``.  Differentiable (fused_autograd.py).
    window_shift: optional 64 host ints [8 heads][4 levels][(dx, dy)] (`enc_tile_window_shift`):
    moves each head's LDS window onto its mean sampling offset -- speed only, same results.
    prepared=True: `proj` comes from gemm_bf16x3_encproj (level pixel coordinates + attention
    weights instead of offsets + logits; ref is not read and may be None) -- same bits."""
    if not prepared and torch.is_grad_enabled() and \
            (value.requires_grad or proj.requires_grad or ref.requires_grad):
        from .fused_autograd import EncTileFunction
        return EncTileFunction.apply(value, proj, ref, levels_hw, variant)
    f32 = torch.float32
    _dev(value, 'value', f32)
    _dev(proj, 'proj', f32)
    if prepared:
        _require(variant == 0, 'deform_attn_enc_tile: prepared input with the default windows only')
        variant = 4
    if out_half:     # fp16 output rows (fp16 operand mode: they only feed output_proj's MFMA)
        variant |= 8
    if ref is not None or not prepared:
        _dev(ref, 'ref', f32)
    _require(value.dim() == 4 and value.shape[2] == 8 and value.shape[3] == 32,
             'deform_attn_enc_tile: value must be [frames, S, 8, 32]')
    F_, S = value.shape[0], value.shape[1]
    _require(proj.dim() == 2 and proj.shape[0] == F_ * S, 'deform_attn_enc_tile: proj rows')
    _require(ref is None or ref.numel() == F_ * S * 8, 'deform_attn_enc_tile: ref must be [F*S, 4, 2]')
    _require(enc_tile_supported(levels_hw), 'deform_attn_enc_tile: needs a 4-level halving pyramid')
    flat = [int(v) for hw in levels_hw for v in hw]
    hw_arr = (ctypes.c_int * 8)(*flat)
    sh_arr = None
    if window_shift is not None:
        _require(len(window_shift) == 64, 'deform_attn_enc_tile: window_shift has 64 entries')
        sh_arr = (ctypes.c_int * 64)(*[int(v) for v in window_shift])
    out = torch.empty((F_ * S, 256), dtype=torch.float16 if out_half else f32, device=value.device)
    _launch('pave_enc_deform_attn_tile_f32', 'deform_attn_enc_tile', value.device,
            value.data_ptr(), proj.data_ptr(), _ptr(ref),
            out.data_ptr(), F_, S, ctypes.cast(hw_arr, ctypes.c_void_p), proj.stride(0), int(variant),
            ctypes.cast(sh_arr, ctypes.c_void_p) if sh_arr is not None else None, tag='enc_tile')
    return out


def conv3x3_nhwc(x, w_taps, bias, stride=1, relu=False):
    """3x3 / pad 1 convolution of a channels_last map on the fp32 MFMA, bias (+ReLU) fused.
    x [N, Cin, H, W] in channels_last storage; w_taps [3, 3, Cin, Cout] contiguous;
    -> [N, Cout, Ho, Wo] channels_last."""
    _nhwc(x, 'conv3x3_nhwc')
    _dev(w_taps, 'w_taps', torch.float32)
    N, Cin, H, W = x.shape
    _require(tuple(w_taps.shape[:3]) == (3, 3, Cin), 'conv3x3_nhwc: weight must be [3,3,Cin,Cout]')
    Cout = w_taps.shape[3]
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    y = torch.empty((N, Ho, Wo, Cout), dtype=torch.float32, device=x.device)
    _launch('pave_conv3x3_nhwc_f32', 'conv3x3_nhwc', x.device, x.data_ptr(), w_taps.data_ptr(), _ptr(bias),
            y.data_ptr(), N, H, W, Cin, Cout, int(stride), int(bool(relu)), tag='conv3x3')
    return y.permute(0, 3, 1, 2)


def rows_gemm_bias_res_act(a, w_kn, bias=None, residual=None, relu=False, out=None, a_bias=None,
                           a2=None):
    """out[M, N] = act([A1 | a2] @ w_kn + bias + residual) on the fp32 MFMA in one pass, with
    A1 = relu(a + a_bias) if a_bias is given else a  (the Bottleneck tail `bn2 -> relu -> conv3 ->
    bn3 -> += identity | downsample(x) -> relu`, resnet.py:264-283).  w_kn is [K (+ K2), N].
    `residual` may be the tensor given as `out` (in-place accumulate into the identity)."""
    _dev(a, 'a', torch.float32)
    _dev(w_kn, 'w_kn', torch.float32)
    _require(a.dim() == 2 and w_kn.dim() == 2, 'rows_gemm: a [M,K], w [K,N]')
    M, K = a.shape
    K2 = 0
    if a2 is not None:
        _dev(a2, 'a2', torch.float32)
        _require(a2.dim() == 2 and a2.shape[0] == M, 'rows_gemm: a2 [M,K2]')
        K2 = a2.shape[1]
    _require(w_kn.shape[0] == K + K2, 'rows_gemm: w must be [K + K2, N]')
    N = w_kn.shape[1]
    for t, nm, n in ((bias, 'bias', N), (a_bias, 'a_bias', K)):
        if t is not None:
            _dev(t, nm, torch.float32)
            _require(t.numel() == n, f'rows_gemm: {nm} has {t.numel()} elements, expected {n}')
    if residual is not None:
        _dev(residual, 'residual', torch.float32)
        _require(tuple(residual.shape) == (M, N), 'rows_gemm: residual [M,N]')
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=a.device)
    else:
        _dev(out, 'out', torch.float32)
        _require(tuple(out.shape) == (M, N), 'rows_gemm: out [M,N]')
    _launch('pave_rows_gemm_bias_res_act_f32', 'rows_gemm_bias_res_act', a.device,
            a.data_ptr(), _ptr(a_bias), _ptr(a2), w_kn.data_ptr(), _ptr(bias), _ptr(residual),
            out.data_ptr(), M, K, K2, N, int(bool(relu)), tag='rows_gemm')
    return out


def bias_relu_maxpool_nhwc(x, bias):
    """maxpool3x3/s2/p1(relu(x + bias)) of a channels_last map in one pass (ResNet stem tail)."""
    _nhwc(x, 'bias_relu_maxpool')
    _dev(bias, 'bias', torch.float32)
    N, C, H, W = x.shape
    _require(bias.numel() == C, 'bias_relu_maxpool: bias [C]')
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    y = torch.empty((N, Ho, Wo, C), dtype=torch.float32, device=x.device)
    _launch('pave_bias_relu_maxpool_nhwc_f32', 'bias_relu_maxpool_nhwc', x.device,
            x.data_ptr(), bias.data_ptr(), y.data_ptr(), N, H, W, C, tag='stem_pool')
    return y.permute(0, 3, 1, 2)


def split_bf16x3(x, planes=3):
    """fp32 tensor -> int16 tensor [planes, *x.shape] of bf16 bit patterns.  planes = 3: rounded terms,
    x == p0 + p1 + p2 exactly (the weight operand: include/pave_hip.h says why rounded);  2: a truncation
    term and the rounded remainder;  1: x rounded.  planes = PLANES_FP16: one plane of fp16 bit patterns."""
    _dev(x, 'x', torch.float32)
    _require(planes in (1, 2, 3, PLANES_FP16), 'split_bf16x3: planes must be 1, 2, 3 or PLANES_FP16')
    n_out = 1 if planes == PLANES_FP16 else planes
    out = torch.empty((n_out,) + tuple(x.shape), dtype=torch.int16, device=x.device)
    _launch('pave_split_bf16x3_f32', 'split_bf16x3', x.device, x.data_ptr(), out.data_ptr(), x.numel(), planes)
    return out.view(torch.float16) if planes == PLANES_FP16 else out


def split_weight_bf16x3(weight, planes=3, pad=False):
    """nn.Linear weight [N, K] -> the W operand of `gemm_bf16x3`: int16 [K/16, planes, N, 16],
    i.e. the bf16 planes cut into 16-wide K slabs, slab-major, so that one slab of a column tile
    is contiguous in memory (every 128-byte line is fetched once).  pad=True (3-plane kernels):
    zero rows / columns up to N % 64 == 0, K % 32 == 0 (the kernels store the real N columns)."""
    _require(weight.dim() == 2, 'split_weight_bf16x3: weight [N, K]')
    N, K = weight.shape
    if pad and (N % 64 or K % 32):
        Np, Kp = (N + 63) // 64 * 64, (K + 31) // 32 * 32
        wpad = torch.zeros((Np, Kp), dtype=weight.dtype, device=weight.device)
        wpad[:N, :K] = weight
        weight, N, K = wpad, Np, Kp
    _require((K % 64 == 0 and N % 64 == 0) or (pad and K % 32 == 0 and N % 64 == 0),
             'split_weight_bf16x3: weight [N % 64 == 0, K % 64 == 0] (pad=True: any N, K)')
    pl = split_bf16x3(weight.contiguous(), planes)
    return pl.view(pl.shape[0], N, K // 16, 16).permute(2, 0, 1, 3).contiguous()


BLOCK_SLOTS = 512         # resident GEMM blocks of the chip: 256 CUs x 2 blocks of the wide / LayerNorm forms
ROUND_SPLIT = True        # A/B switch of round_split_rows (tools/ab_switch.py)


def round_split_rows(M, tiles_per_row_tile):
    """Block-slot quantisation: a launch whose tile count lands just above a multiple of the chip's 512 block slots
    runs a whole extra round for a handful of tiles (3 x 22 323 rows = 524 row tiles: every LayerNorm-epilogue launch
    of a one-clip T = 3 step ran a second round of 12 tiles -- 227 us where one round takes 110).  Returns the row
    count M1 of the FULL rounds when the last round would be less than an eighth full and its rows (at most 2 048)
    fit the small-row forms -- the caller launches rows [0, M1) and [M1, M) separately (GEMM rows are independent:
    the same values up to the summation order of the form each part takes) -- else None."""
    if not ROUND_SPLIT:
        return None
    rt = (M + 127) // 128
    per_round = BLOCK_SLOTS // max(1, tiles_per_row_tile)      # row tiles per round
    if per_round < 1 or rt <= per_round:
        return None
    r = rt % per_round
    if r == 0 or r * tiles_per_row_tile > BLOCK_SLOTS // 8:
        return None
    M1 = (rt - r) * 128
    return M1 if 0 < M - M1 <= 2048 else None


_ACT_CODE = {'gelu': 2, 'sigmoid': 3}     # pave_gemm_bf16x3_f32's `relu` argument beyond 0 / 1
SPLITK_ROWS = True     # plain row GEMMs with a split-K plan take pave_gemm_bf16x3_splitk_f32 (tools: A/B switch)


def gemm_bf16x3(a, w_planes, bias=None, residual=None, relu=False, out=None, a_bias=None,
                fp16=False, n_out=None):
    """out[M, N] = act(A' @ W^T + bias + residual), A' = relu(a + a_bias) if a_bias is given, on
    the bf16 matrix cores with both operands split into P = w_planes.shape[1] bf16 terms
    (relu: False | True | 'gelu' = exact GELU | 'sigmoid'; the last two: 3 planes / fp16 only)
    (P = 3: exact split, 6 MFMA products, fp32-level accuracy;  2: 3 products, ~2^-16;
    1: plain bf16 operands, or fp16 operands with fp16=True and a PLANES_FP16 weight), fp32
    accumulate, fp32 in / out.
    w_planes = split_weight_bf16x3(weight [N, K]).  `residual` may be the tensor given as `out`.
    n_out (3 planes): the real output width when the planes were zero-padded to N % 64 == 0
    (split_weight_bf16x3(..., pad=True)); out / bias / residual then have n_out columns."""
    lib = native.load()
    _dev(a, 'a', torch.float32)
    npl = _planes(w_planes, fp16=fp16)
    _require(a.dim() == 2 and w_planes.shape[1] in (1, 2, 3) and w_planes.shape[0] * 16 == a.shape[1],
             'gemm_bf16x3: a [M,K], w_planes [K/16,3,N,16] (split_weight_bf16x3)')
    M, K = a.shape
    N = w_planes.shape[2]
    if n_out is not None and n_out != N:
        _require(npl in _Q_PLANES and n_out % 4 == 0 and (n_out + 63) // 64 * 64 == N,
                 'gemm_bf16x3: n_out % 4 == 0 with 3 planes / fp16 padded to roundup(n_out, 64) rows')
        N = int(n_out)
    else:
        _require(N % 128 == 0 or (N % 64 == 0 and npl in _Q_PLANES),
                 'gemm_bf16x3: N % 128 == 0 (or N % 64 == 0 with 3 planes / fp16)')
    for t, nm, n in ((bias, 'bias', N), (a_bias, 'a_bias', K)):
        if t is not None:
            _dev(t, nm, torch.float32)
            _require(t.numel() == n, f'gemm_bf16x3: {nm} has {t.numel()} elements, expected {n}')
    if residual is not None:
        _dev(residual, 'residual', torch.float32)
        _require(tuple(residual.shape) == (M, N), 'gemm_bf16x3: residual [M,N]')
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=a.device)
    else:
        _dev(out, 'out', torch.float32)
        _require(tuple(out.shape) == (M, N), 'gemm_bf16x3: out [M,N]')
    if N % 256 == 0 and npl in _Q_PLANES and a_bias is None and N == w_planes.shape[2]:
        M1 = round_split_rows(M, N // 256)          # (the wide form's tiles: N / 256 per row tile)
        if M1 is not None:
            gemm_bf16x3(a[:M1], w_planes, bias, residual[:M1] if residual is not None else None, relu=relu,
                        out=out[:M1], fp16=fp16)
            gemm_bf16x3(a[M1:], w_planes, bias, residual[M1:] if residual is not None else None, relu=relu,
                        out=out[M1:], fp16=fp16)
            return out
    # few row tiles and a long K (a one-clip batch's layer4 1x1 reductions, the neck's C5 lateral): the split-K
    # form, as for the 3x3 convolutions (workspace from torch's stream-aware caching allocator)
    # (a plan exists only for K >= 2048 on fewer than 200 row tiles -- pave_internal_splitk_plan --, so the ~170
    # K = 256 / 1024 launches of the decoder tail do not pay a library call to learn that)
    ws_bytes = lib.pave_gemm_splitk_workspace_bytes(M, K, N) \
        if (SPLITK_ROWS and K >= 2048 and M < 200 * 128 and npl in _Q_PLANES and a_bias is None
            and relu in (False, True, 0, 1)) else 0
    if ws_bytes > 0:
        ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=a.device)
        _launch('pave_gemm_bf16x3_splitk_f32', 'gemm_bf16x3_splitk', a.device,
                a.data_ptr(), w_planes.data_ptr(), _ptr(bias), _ptr(residual),
                out.data_ptr(), M, K, N, int(bool(relu)), npl, ws.data_ptr(), ws_bytes,
                tag=_gemm_tag('gemm_bf16x3', M), flops=2 * M * K * N,
                shape=(M, K, N, 'relu' if relu else '', 'res' if residual is not None else '', 'split-K'))
        return out
    _launch('pave_gemm_bf16x3_f32', 'gemm_bf16x3', a.device,
            a.data_ptr(), _ptr(a_bias), w_planes.data_ptr(), _ptr(bias),
            _ptr(residual), out.data_ptr(), M, K, N, _ACT_CODE.get(relu, int(bool(relu))), npl,
            tag=_gemm_tag('gemm_bf16x3', M), flops=2 * M * K * N,
            shape=(M, K, N, 'relu' if relu else '', 'res' if residual is not None else '',
                   'abias' if a_bias is not None else ''))
    return out


def gemm_bf16x3_cat(a, a2, w_planes, bias=None, residual=None, relu=False, out=None):
    """out[M, N] = act([a | a2] @ W^T + bias + residual): two row matrices share the K axis and one
    accumulator (the Bottleneck tail with a stride-1 downsample: conv3 and the downsample
    convolution in one launch, no concatenation copy).  w_planes = split_weight_bf16x3 of the
    [N, K1 + K2] row-concatenated weight."""
    _dev(a, 'a', torch.float32)
    _dev(a2, 'a2', torch.float32)
    npl = _planes(w_planes, only=_Q_PLANES)
    _require(a.dim() == 2 and a2.dim() == 2 and a.shape[0] == a2.shape[0],
             'gemm_bf16x3_cat: a [M, K1], a2 [M, K2]')
    M, K1 = a.shape
    K = K1 + a2.shape[1]
    _require(w_planes.shape[0] * 16 == K, 'gemm_bf16x3_cat: w_planes [(K1+K2)/16, 3, N, 16]')
    N = w_planes.shape[2]
    _require(K % 32 == 0 and N % 64 == 0 and K1 % 16 == 0, 'gemm_bf16x3_cat: K % 32, N % 64, K1 % 16')
    if bias is not None:
        _dev(bias, 'bias', torch.float32)
        _require(bias.numel() == N, 'gemm_bf16x3_cat: bias [N]')
    if residual is not None:
        _dev(residual, 'residual', torch.float32)
        _require(tuple(residual.shape) == (M, N), 'gemm_bf16x3_cat: residual [M, N]')
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=a.device)
    else:
        _dev(out, 'out', torch.float32)
        _require(tuple(out.shape) == (M, N), 'gemm_bf16x3_cat: out [M, N]')
    _launch('pave_gemm_bf16x3_cat_f32', 'gemm_bf16x3_cat', a.device,
            a.data_ptr(), K1, a2.data_ptr(), w_planes.data_ptr(), _ptr(bias), _ptr(residual), out.data_ptr(), M, K, N,
            int(bool(relu)), npl,
            tag=_gemm_tag('gemm_bf16x3', M), flops=2 * M * K * N, shape=(M, K, N, 'cat', f'k1={K1}'))
    return out


def gemm_bf16x3_grouped(a, w_planes, bias, group_n, relu=False):
    """Grouped row GEMM: a [M, G*K] (group i = columns [i K, (i+1) K)), w_planes = planes of the
    [G*group_n, K] row-concatenated per-group weights -> out [M, G*group_n] with
    out[:, i*group_n:(i+1)*group_n] = act(a_i @ W_i^T + bias_i).  One launch for G Linears."""
    _dev(a, 'a', torch.float32)
    npl = _planes(w_planes, only=_Q_PLANES)
    _require(a.dim() == 2, 'gemm_bf16x3_grouped: a [M, G*K], w_planes [K/16, 3, N, 16]')
    M, lda = a.shape
    K, N = w_planes.shape[0] * 16, w_planes.shape[2]
    G = N // int(group_n)
    _require(G * group_n == N and G * K == lda, 'gemm_bf16x3_grouped: a has G*K columns, N = G*group_n')
    if bias is not None:
        _dev(bias, 'bias', torch.float32)
        _require(bias.numel() == N, 'gemm_bf16x3_grouped: bias [N]')
    out = torch.empty((M, N), dtype=torch.float32, device=a.device)
    _launch('pave_gemm_bf16x3_grouped_f32', 'gemm_bf16x3_grouped', a.device,
            a.data_ptr(), lda, w_planes.data_ptr(), _ptr(bias), out.data_ptr(), M, K, N, int(group_n),
            int(bool(relu)), npl,
            tag=_gemm_tag('gemm_bf16x3', M), flops=2 * M * K * N, shape=(M, K, N, 'grouped', f'g{G}'))
    return out


def conv1x1_strided_split(x, w_planes, bias=None, stride=2, relu=False):
    """1x1 convolution with a stride on a channels_last map through the 3-plane split GEMM (the A
    rows are the strided input pixels: no slice copy).  x [N, Cin, H, W] channels_last;
    w_planes = split_weight_bf16x3(weight [Cout, Cin]) -> [N, Cout, Ho, Wo] channels_last."""
    _nhwc(x, 'conv1x1_strided_split')
    npl = _planes(w_planes, only=_Q_PLANES)
    N, Cin, H, W = x.shape
    _require(w_planes.shape[0] * 16 == Cin, 'conv1x1_strided_split: w_planes [Cin/16, 3, Cout, 16]')
    Cout = w_planes.shape[2]
    if bias is not None:
        _dev(bias, 'bias', torch.float32)
        _require(bias.numel() == Cout, 'conv1x1_strided_split: bias [Cout]')
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    y = torch.empty((N, Ho, Wo, Cout), dtype=torch.float32, device=x.device)
    _launch('pave_conv1x1_strided_split_f32', 'conv1x1_strided_split', x.device,
            x.data_ptr(), w_planes.data_ptr(), _ptr(bias),
            y.data_ptr(), N, H, W, Cin, Cout, int(stride), int(bool(relu)), npl,
            tag='conv1x1_strided', flops=2 * N * Ho * Wo * Cin * Cout, shape=(N * Ho * Wo, Cin, Cout, f's{stride}'))
    return y.permute(0, 3, 1, 2)


def conv3x3s2_c3_nchw(x, w_taps, bias=None, relu=False):
    """HRNet stem conv1: 3x3 / stride 2 / pad 1, 3 -> 64 channels, read straight from the NCHW batch
    x [N, 3, H, W] (contiguous) -> [N, 64, Ho, Wo] channels_last; w_taps [27, 64] =
    weight.permute(1, 2, 3, 0).reshape(27, 64) (pave_conv3x3s2_c3_nchw_f32)."""
    _dev(x, 'x', torch.float32)
    _dev(w_taps, 'w_taps', torch.float32)
    _require(x.dim() == 4 and x.shape[1] == 3 and tuple(w_taps.shape) == (27, 64),
             'conv3x3s2_c3_nchw: x [N, 3, H, W], w_taps [27, 64]')
    if bias is not None:
        _dev(bias, 'bias', torch.float32)
        _require(bias.numel() == 64, 'conv3x3s2_c3_nchw: bias [64]')
    N, _, H, W = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    y = torch.empty((N, Ho, Wo, 64), dtype=torch.float32, device=x.device)
    _launch('pave_conv3x3s2_c3_nchw_f32', 'conv3x3s2_c3_nchw', x.device, x.data_ptr(), w_taps.data_ptr(), _ptr(bias),
            y.data_ptr(), N, H, W, int(bool(relu)))
    return y.permute(0, 3, 1, 2)


def split_stem7x7_weight(weight, planes=3):
    """Stem weight [64, 3, 7, 7] -> operand of conv7x7s2_nchw_split, int16 [23, 3, 64, 16]: the 3
    bf16 planes in two K layouts (include/pave_hip.h): 12 slabs of (c, ky, kx | pad) (K = 192)
    followed by 11 slabs of (c, ky, kx + 1) with a zero 22nd row (K = 176).  planes = PLANES_FP16:
    float16 [23, 1, 64, 16], one plane of fp16 operands in the same two layouts."""
    _require(tuple(weight.shape[1:]) == (3, 7, 7), 'split_stem7x7_weight: weight [Cout, 3, 7, 7]')
    _require(planes in _Q_PLANES, 'split_stem7x7_weight: 3 bf16 planes or PLANES_FP16')
    co = weight.shape[0]
    w = torch.zeros((co, 24, 8), dtype=torch.float32, device=weight.device)
    w[:, :21, :7] = weight.reshape(co, 21, 7)
    a = split_weight_bf16x3(w.reshape(co, 192).contiguous(), planes)
    w2 = torch.zeros((co, 22, 8), dtype=torch.float32, device=weight.device)
    w2[:, :21, 1:] = weight.reshape(co, 21, 7)
    pl = split_bf16x3(w2.reshape(co, 176).contiguous(), planes)          # [planes, co, 176]
    b = pl.view(pl.shape[0], co, 11, 16).permute(2, 0, 1, 3).contiguous()
    return torch.cat([a, b], 0)


def repitch_rows(x):
    """x [..., W] dense fp32 -> the same rows at a pitch of roundup(W, 4) elements with zero pad columns
    (pave_repitch_rows_f32): 16-byte aligned rows for the LDS-DMA stem when W % 4 != 0 (the 750 x 1333 frames of
    the reference's PoseTrack pipeline).  Returns the padded tensor [..., roundup(W, 4)]."""
    _dev(x, 'x', torch.float32)
    W = x.shape[-1]
    pitch = (W + 3) // 4 * 4
    out = torch.empty(tuple(x.shape[:-1]) + (pitch,), dtype=torch.float32, device=x.device)
    rows = x.numel() // W
    _launch('pave_repitch_rows_f32', 'repitch_rows', x.device, x.data_ptr(), out.data_ptr(), rows, W, pitch)
    return out


def conv7x7s2_nchw_split(x, w_planes, bias=None, relu=False, valid_w=None):
    """7x7 / stride 2 / pad 3 stem convolution of the NCHW image batch x [N, 3, H, W] through the
    3-plane split kernel -> [N, 64, Ho, Wo] channels_last.  valid_w: x is a `repitch_rows` result whose real
    width is valid_w (columns valid_w .. W - 1 are zero): the output is that of the valid_w-wide image."""
    _dev(x, 'x', torch.float32)
    npl = _planes(w_planes, only=_Q_PLANES)
    _require(x.dim() == 4 and x.shape[1] == 3, 'conv7x7s2_nchw_split: x [N, 3, H, W] (NCHW, dense)')
    _require(w_planes.shape[0] == 23, 'conv7x7s2_nchw_split: w_planes from split_stem7x7_weight')
    N, _, H, pitch = x.shape
    W = pitch if valid_w is None else int(valid_w)
    _require(0 < W <= pitch and (W == pitch or pitch % 4 == 0), 'conv7x7s2_nchw_split: valid_w <= W, W % 4 == 0')
    Cout = w_planes.shape[2]
    if bias is not None:
        _dev(bias, 'bias', torch.float32)
        _require(bias.numel() == Cout, 'conv7x7s2_nchw_split: bias [Cout]')
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    y = torch.empty((N, Ho, Wo, Cout), dtype=torch.float32, device=x.device)
    _launch('pave_conv7x7s2_nchw_split_f32', 'conv7x7s2_nchw_split', x.device,
            x.data_ptr(), w_planes.data_ptr(), _ptr(bias),
            y.data_ptr(), N, H, W, pitch, Cout, int(bool(relu)), npl,
            tag='conv7x7_stem', flops=2 * N * Ho * Wo * Cout * 147, shape=(N * Ho * Wo, 147, Cout))
    return y.permute(0, 3, 1, 2)


def ref_update(tmp, ref, eps=1e-5):
    """sigmoid(tmp + inverse_sigmoid(ref)) in one launch (decoder reference-point update)."""
    _require(tmp.is_cuda and tmp.dtype == torch.float32 and ref.dtype == torch.float32
             and tuple(tmp.shape) == tuple(ref.shape), 'ref_update: fp32 device tensors, same shape')
    if (tmp.dim() >= 2 and not tmp.is_contiguous() and tmp.stride(-1) == 1 and ref.is_contiguous()
            and tmp.numel() > 0 and tmp.stride(-2) >= tmp.shape[-1]
            and all(tmp.stride(i) == tmp.stride(i + 1) * tmp.shape[i + 1] for i in range(tmp.dim() - 2))):
        # a column slice of a wider matrix (a branch output padded to the 4-column grid): read in place
        # by the strided form of the same kernel (T = 1: rows [R, ld], the first o columns)
        R, o = tmp.numel() // tmp.shape[-1], tmp.shape[-1]
        out = torch.empty_like(ref)
        _launch('pave_ref_update_frames_f32', 'ref_update', tmp.device, tmp.data_ptr(), ref.data_ptr(), out.data_ptr(),
                R, 1, tmp.stride(-2), o, R, float(eps), tag='ref_update')
        return out
    tmp, ref = tmp.contiguous(), ref.contiguous()
    out = torch.empty_like(tmp)
    if tmp.numel() == 0:
        return out
    _launch('pave_ref_update_f32', 'ref_update', tmp.device, tmp.data_ptr(), ref.data_ptr(), out.data_ptr(),
            tmp.numel(), float(eps), tag='ref_update')
    return out


def ref_update_frames(y, ref, T, o, group, eps=1e-5, out=None):
    """sigmoid(y_t + inverse_sigmoid(ref)) read straight from the grouped per-frame MLP output
    y [R, T * op] (frame t's `o` outputs at columns [t op, t op + o)); ref [..., o] with R * T rows
    ordered (r // group, t, r % group) -> same shape as ref.  One launch, no layout copy."""
    _dev(y, 'y', torch.float32)
    _dev(ref, 'ref', torch.float32)
    R = y.shape[0]
    op = y.shape[1] // int(T)
    _require(y.dim() == 2 and op * T == y.shape[1] and op >= o and ref.shape[-1] == o
             and ref.numel() == R * T * o and R % int(group) == 0,
             'ref_update_frames: y [R, T*op], ref [R*T rows, o], R % group == 0')
    if out is None:
        out = torch.empty_like(ref)
    else:       # (a level of the decoder's preallocated [levels, ...] stack of intermediate references)
        _dev(out, 'out', torch.float32)
        _require(tuple(out.shape) == tuple(ref.shape), 'ref_update_frames: out shaped like ref')
    _launch('pave_ref_update_frames_f32', 'ref_update_frames', y.device, y.data_ptr(), ref.data_ptr(), out.data_ptr(),
            R, int(T), op, int(o), int(group), float(eps), tag='ref_update')
    return out


def groupnorm_nhwc_into(x_rows, gamma, beta, num_groups, eps, dst):
    """GroupNorm of an NHWC map given as rows x_rows [N, HW, C] (dense), written into dst
    [N, HW, C] whose batch stride may be larger than HW * C (a slice of a [N, S, C] token buffer).
    fp64 statistics in a fixed order."""
    _dev(x_rows, 'x', torch.float32)
    _require(x_rows.dim() == 3, 'groupnorm_nhwc_into: x [N, HW, C]')
    N, HW, C = x_rows.shape
    _dev(gamma, 'gamma', torch.float32)
    _dev(beta, 'beta', torch.float32)
    _require(gamma.numel() == C and beta.numel() == C, 'groupnorm_nhwc_into: gamma / beta [C]')
    _require(dst.is_cuda and dst.dtype == torch.float32 and tuple(dst.shape) == (N, HW, C)
             and dst.stride(2) == 1 and dst.stride(1) == C and (N == 1 or dst.stride(0) >= HW * C),
             'groupnorm_nhwc_into: dst [N, HW, C] with dense rows')
    nchunks = max(1, min(128, (HW + 63) // 64))
    partial = torch.empty((N, nchunks, num_groups, 2), dtype=torch.float64, device=x_rows.device)
    ab = torch.empty((N, 2, C), dtype=torch.float32, device=x_rows.device)
    _launch('pave_groupnorm_nhwc_f32', 'groupnorm_nhwc_into', x_rows.device,
            x_rows.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
            dst.data_ptr(), dst.stride(0) if N > 1 else HW * C, N, HW,
            C, int(num_groups), float(eps), partial.data_ptr(), nchunks, ab.data_ptr(), tag='groupnorm')
    return dst


def groupnorm_levels_into(levels, num_groups):
    """GroupNorm of several NHWC maps of one N and C at once -- the neck's levels -- as three launches in all
    (statistics, scale / shift, apply) instead of three per level; per level the values of `groupnorm_nhwc_into`,
    bit for bit.  levels: [(x_rows [N, HW_l, C], gamma, beta, eps, dst [N, HW_l, C])]."""
    _require(len(levels) >= 1, 'groupnorm_levels_into: at least one level')
    N, _, C = levels[0][0].shape
    dev = levels[0][0].device
    for i0 in range(0, len(levels), 4):       # (the entry takes up to four maps per call)
        part = levels[i0:i0 + 4]
        arr = (native.GnLevel * len(part))()
        total_chunks = 0
        for j, (x_rows, gamma, beta, eps, dst) in enumerate(part):
            _dev(x_rows, 'x', torch.float32)
            _dev(gamma, 'gamma', torch.float32)
            _dev(beta, 'beta', torch.float32)
            _require(x_rows.dim() == 3 and x_rows.shape[0] == N and x_rows.shape[2] == C and x_rows.device == dev,
                     'groupnorm_levels_into: every x [N, HW_l, C] on one device')
            HW = x_rows.shape[1]
            _require(gamma.numel() == C and beta.numel() == C, 'groupnorm_levels_into: gamma / beta [C]')
            _require(dst.is_cuda and dst.dtype == torch.float32 and tuple(dst.shape) == (N, HW, C)
                     and dst.stride(2) == 1 and dst.stride(1) == C and (N == 1 or dst.stride(0) >= HW * C),
                     'groupnorm_levels_into: dst [N, HW, C] with dense rows')
            nchunks = max(1, min(128, (HW + 63) // 64))       # (as groupnorm_nhwc_into)
            arr[j] = native.GnLevel(x_rows.data_ptr(), gamma.data_ptr(), beta.data_ptr(), dst.data_ptr(),
                                    dst.stride(0) if N > 1 else HW * C, HW, nchunks, float(eps))
            total_chunks += nchunks
        partial = torch.empty((N * total_chunks * num_groups * 2,), dtype=torch.float64, device=dev)
        ab = torch.empty((len(part), N, 2, C), dtype=torch.float32, device=dev)
        _launch('pave_groupnorm_levels_nhwc_f32', 'groupnorm_levels_into', dev,
                ctypes.cast(arr, ctypes.c_void_p), len(part), N, C, int(num_groups), partial.data_ptr(), ab.data_ptr(),
                tag='groupnorm')
    return [lv[4] for lv in levels]


def gemm_bf16x3_ln(a, w_planes, bias, residual, gamma, beta, eps, out=None):
    """out[M, 256] = LayerNorm(a @ W^T + bias + residual) * gamma + beta in ONE launch (3 bf16
    planes; the 128 x 256 block tile owns whole rows).  `residual` may be None or the tensor given
    as `out`."""
    _dev(a, 'a', torch.float32)
    npl = _planes(w_planes, only=_Q_PLANES)
    _require(a.dim() == 2 and w_planes.shape[0] * 16 == a.shape[1],
             'gemm_bf16x3_ln: a [M,K], w_planes [K/16,3,N,16] (split_weight_bf16x3, 3 planes or fp16)')
    M, K = a.shape
    N = w_planes.shape[2]
    _require(N == 256, 'gemm_bf16x3_ln: N == 256')
    for t, nm in ((bias, 'bias'), (gamma, 'gamma'), (beta, 'beta')):
        if t is not None:
            _dev(t, nm, torch.float32)
            _require(t.numel() == N, f'gemm_bf16x3_ln: {nm} has {t.numel()} elements, expected {N}')
    _require(gamma is not None and beta is not None, 'gemm_bf16x3_ln: gamma and beta are required')
    if residual is not None:
        _dev(residual, 'residual', torch.float32)
        _require(tuple(residual.shape) == (M, N), 'gemm_bf16x3_ln: residual [M,N]')
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=a.device)
    else:
        _dev(out, 'out', torch.float32)
        _require(tuple(out.shape) == (M, N), 'gemm_bf16x3_ln: out [M,N]')
    # (the last, nearly empty round of block slots as a launch of the small-row form -- under a form policy
    # (set_batch_invariant) the tail would take the head's LayerNorm form anyway: no split, one launch)
    M1 = round_split_rows(M, 1) if current_form_policy() == 0 else None
    if M1 is not None:
        gemm_bf16x3_ln(a[:M1], w_planes, bias, residual[:M1] if residual is not None else None, gamma, beta, eps,
                       out=out[:M1])
        gemm_bf16x3_ln(a[M1:], w_planes, bias, residual[M1:] if residual is not None else None, gamma, beta, eps,
                       out=out[M1:])
        return out
    _launch('pave_gemm_bf16x3_ln_f32', 'gemm_bf16x3_ln', a.device,
            a.data_ptr(), w_planes.data_ptr(), _ptr(bias), _ptr(residual),
            gamma.data_ptr(), beta.data_ptr(), float(eps), out.data_ptr(), M, K, N, npl,
            tag=_gemm_tag('gemm_bf16x3_ln', M), flops=2 * M * K * N,
            shape=(M, K, N, 'ln', 'res' if residual is not None else ''))
    return out


def gemm_fp16_act(a, w_plane, bias=None, relu=False, out_half=False, residual=None, ln=None, out=None):
    """fp16 operand mode with fp16 activations around the launch (pave_gemm_fp16_act_f32; wide tile forms):
    a [M, K] fp32 or float16, w_plane = the ONE fp16 plane of split_weight_bf16x3(weight, PLANES_FP16), N % 256 == 0.
    ln = None: act(a W^T + bias) -> [M, N] fp32, or float16 with out_half (an activation that only feeds the next
    GEMM).  ln = (gamma, beta, eps): LayerNorm(a W^T + bias + residual) gamma + beta -> [M, 256] fp32 (`residual`
    may be the tensor given as `out`)."""
    _require(isinstance(a, torch.Tensor) and a.is_cuda and a.is_contiguous() and a.dim() == 2
             and a.dtype in (torch.float32, torch.float16), 'gemm_fp16_act: a [M, K] fp32 or float16 on the device')
    _require(_planes(w_plane) == PLANES_FP16, 'gemm_fp16_act: one fp16 plane (split_weight_bf16x3(w, PLANES_FP16))')
    M, K = a.shape
    N = w_plane.shape[2]
    _require(w_plane.shape[0] * 16 == K and N % 256 == 0, 'gemm_fp16_act: w_plane [K/16, 1, N % 256 == 0, 16]')
    if bias is not None:
        _dev(bias, 'bias', torch.float32)
        _require(bias.numel() == N, 'gemm_fp16_act: bias [N]')
    if ln is not None:
        gamma, beta, eps = ln
        _dev(gamma, 'gamma', torch.float32)
        _dev(beta, 'beta', torch.float32)
        _require(N == 256 and gamma.numel() == 256 and beta.numel() == 256 and not out_half and not relu,
                 'gemm_fp16_act: the LayerNorm form has N == 256 and an fp32 output')
        if residual is not None:
            _dev(residual, 'residual', torch.float32)
            _require(tuple(residual.shape) == (M, N), 'gemm_fp16_act: residual [M, N]')
        if out is None:
            out = torch.empty((M, N), dtype=torch.float32, device=a.device)
        _require(out.dtype == torch.float32 and tuple(out.shape) == (M, N) and out.is_contiguous(), 'gemm_fp16_act: out')
        args = (_ptr(residual), gamma.data_ptr(), beta.data_ptr(), float(eps))
        tag = _gemm_tag('gemm_bf16x3_ln', M)
    else:
        _require(residual is None and out is None, 'gemm_fp16_act: the plain form takes bias + activation only')
        out = torch.empty((M, N), dtype=torch.float16 if out_half else torch.float32, device=a.device)
        args = (None, None, None, 0.0)
        tag = _gemm_tag('gemm_bf16x3', M)
    note = (M, K, N, 'f16act', 'a16' if a.dtype == torch.float16 else '', 'o16' if out_half else '',
            'ln' if ln is not None else ('relu' if relu else ''), 'res' if residual is not None else '')
    _launch('pave_gemm_fp16_act_f32', 'gemm_fp16_act', a.device,
            a.data_ptr(), int(a.dtype == torch.float16), w_plane.data_ptr(), _ptr(bias),
            *args, out.data_ptr(), int(bool(out_half)), M, K, N, 2 if relu == 'gelu' else int(bool(relu)),
            tag=tag, flops=2 * M * K * N, shape=note)
    return out


def gemm_bf16x3_ex(a, w_planes, bias=None, residual=None, residual_rows=0, n_split=0, relu=False,
                   a_bias=None, fp16=False, _out=None):
    """gemm_bf16x3 with a row-periodic residual table (`residual` [residual_rows, N], row m adds
    residual[m % residual_rows]) and / or the output cut at column `n_split` into two dense
    matrices -> out [M, n_split], out2 [M, N - n_split] (n_split = 0: one output, out2 = None)."""
    _dev(a, 'a', torch.float32)
    npl = _planes(w_planes, fp16=fp16)
    _require(a.dim() == 2 and w_planes.shape[1] in (1, 2, 3) and w_planes.shape[0] * 16 == a.shape[1],
             'gemm_bf16x3_ex: a [M,K], w_planes [K/16,3,N,16] (split_weight_bf16x3)')
    M, K = a.shape
    N = w_planes.shape[2]
    _require(N % 128 == 0, 'gemm_bf16x3_ex: N % 128 == 0')
    for t, nm, n in ((bias, 'bias', N), (a_bias, 'a_bias', K)):
        if t is not None:
            _dev(t, nm, torch.float32)
            _require(t.numel() == n, f'gemm_bf16x3_ex: {nm} has {t.numel()} elements, expected {n}')
    rr = int(residual_rows)
    if residual is not None:
        _dev(residual, 'residual', torch.float32)
        _require(tuple(residual.shape) == ((rr if rr > 0 else M), N),
                 'gemm_bf16x3_ex: residual [residual_rows or M, N]')
    else:
        _require(rr == 0, 'gemm_bf16x3_ex: residual_rows without a residual')
    n_split = int(n_split)
    _require(n_split == 0 or (0 < n_split < N and n_split % 128 == 0),
             'gemm_bf16x3_ex: 0 < n_split < N, n_split % 128 == 0')
    if N % 256 == 0 and npl in _Q_PLANES and a_bias is None and rr == 0 and (n_split == 0 or n_split % 256 == 0) \
            and _out is None:
        M1 = round_split_rows(M, N // 256)      # (a nearly empty last round of block slots: see round_split_rows)
        if M1 is not None:
            out = torch.empty((M, n_split or N), dtype=torch.float32, device=a.device)
            out2 = torch.empty((M, N - n_split), dtype=torch.float32, device=a.device) if n_split else None
            for r0, r1 in ((0, M1), (M1, M)):
                gemm_bf16x3_ex(a[r0:r1], w_planes, bias, residual[r0:r1] if residual is not None else None, 0, n_split,
                               relu, None, fp16, _out=(out[r0:r1], out2[r0:r1] if out2 is not None else None))
            return out, out2
    if _out is not None:
        out, out2 = _out
    else:
        out = torch.empty((M, n_split or N), dtype=torch.float32, device=a.device)
        out2 = torch.empty((M, N - n_split), dtype=torch.float32, device=a.device) if n_split else None
    _launch('pave_gemm_bf16x3_ex_f32', 'gemm_bf16x3_ex', a.device,
            a.data_ptr(), _ptr(a_bias), w_planes.data_ptr(), _ptr(bias),
            _ptr(residual), rr, out.data_ptr(), _ptr(out2), n_split, M, K, N, int(bool(relu)), npl,
            tag=_gemm_tag('gemm_bf16x3', M), flops=2 * M * K * N,
            shape=(M, K, N, 'ex', f'rows{rr}', f'split{n_split}'))
    return out, out2


def swin_window_attn(qkv, bias_t, pad_qkv, heads, window, shift, scale):
    """The (shifted-)window attention core of a Swin block on the un-partitioned token map
    (pave_swin_window_attn_f32): qkv [B, H, W, 3C], bias_t [heads, ws^2, ws^2] (relative-position bias, key-major),
    pad_qkv [3C] (the qkv Linear's bias) -> [B, H, W, C]."""
    for t, nm in ((qkv, 'qkv'), (bias_t, 'bias_t'), (pad_qkv, 'pad_qkv')):
        _dev(t, nm, torch.float32)
    _require(qkv.dim() == 4 and qkv.shape[3] % 3 == 0, 'swin_window_attn: qkv [B, H, W, 3C]')
    B, H, W, C3 = qkv.shape
    C = C3 // 3
    n = window * window
    _require(tuple(bias_t.shape) == (heads, n, n) and pad_qkv.numel() == C3 and C == heads * 32,
             'swin_window_attn: bias_t [heads, ws^2, ws^2], pad_qkv [3C], head dim 32')
    out = torch.empty((B, H, W, C), dtype=torch.float32, device=qkv.device)
    _launch('pave_swin_window_attn_f32', 'swin_window_attn', qkv.device,
            qkv.data_ptr(), bias_t.data_ptr(), pad_qkv.data_ptr(), out.data_ptr(),
            B, H, W, C, int(heads), int(window), int(shift), float(scale))
    return out


def merge_softmax_partials(parts, C, H):
    """parts [G, U, C + 2 H] (all-gathered partial rows | per-head max | per-head sum-exp) -> [U, C]: the
    exact full-softmax row (pave_merge_softmax_partials_f32), one launch."""
    _dev(parts, 'parts', torch.float32)
    _require(parts.dim() == 3 and parts.shape[2] == C + 2 * H, 'merge_softmax_partials: parts [G, U, C + 2 H]')
    G, U = parts.shape[0], parts.shape[1]
    out = torch.empty((U, C), dtype=torch.float32, device=parts.device)
    _launch('pave_merge_softmax_partials_f32', 'merge_softmax_partials', parts.device,
            parts.data_ptr(), out.data_ptr(), G, U, int(C), int(H))
    return out


def mha_core(qkv, n_seq, seq_len, num_heads):
    """Scaled-dot-product core of the decoders' self-attention: qkv [n_seq * seq_len, >= 3 * E]
    (q | k | v columns, E = num_heads * 32; row = (sequence, position)) -> [n_seq * seq_len, E] =
    softmax(q k^T / sqrt(32)) v per (sequence, head).  pave_mha_core_f32 (csrc/pave_decoder.hip)."""
    _dev(qkv, 'qkv', torch.float32)
    E = int(num_heads) * 32
    _require(qkv.dim() == 2 and qkv.shape[0] == n_seq * seq_len and qkv.shape[1] >= 3 * E,
             'mha_core: qkv [n_seq * seq_len, >= 3 * num_heads * 32]')
    out = torch.empty((qkv.shape[0], E), dtype=torch.float32, device=qkv.device)
    _launch('pave_mha_core_f32', 'mha_core', qkv.device, qkv.data_ptr(), out.data_ptr(), int(n_seq), int(seq_len),
            int(num_heads), qkv.stride(0))
    return out


def topk_rows(x, k):
    """torch.topk(x, k, dim=1) for a 2-D fp32 device tensor as ONE launch (pave_topk_rows_f32):
    -> (values [rows, k], indices [rows, k] int64), sorted by value descending, ties by the
    lower index (-0.0 == +0.0; a NaN of either sign ranks above +inf).  x may be any strided 2-D view (no copy)."""
    _require(isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 2
             and x.shape[0] > 0 and x.stride(1) > 0 and (x.shape[0] == 1 or x.stride(0) > 0),
             'topk_rows: x [rows, n] fp32 on the device, positive strides')
    rows, n = x.shape
    k = int(k)
    _require(0 < k <= n and n <= 32768 and k <= 1024, 'topk_rows: 0 < k <= n <= 32768, k <= 1024')
    values = torch.empty((rows, k), dtype=torch.float32, device=x.device)
    index = torch.empty((rows, k), dtype=torch.int64, device=x.device)
    _launch('pave_topk_rows_f32', 'topk_rows', x.device, x.data_ptr(), values.data_ptr(), index.data_ptr(), rows, n,
            x.stride(0), x.stride(1), k)
    return values, index


def gather_frame_poses(poses, index, T):
    """poses [B, T*Q, C] (frame-major rows), index [B, N] int64 -> [T, B*N, C]: the selected
    queries of every frame, frame-major (pave_gather_frame_poses_f32)."""
    _dev(poses, 'poses', torch.float32)
    _dev(index, 'index', torch.int64)
    _require(poses.dim() == 3 and poses.shape[1] % T == 0 and index.dim() == 2
             and index.shape[0] == poses.shape[0], 'gather_frame_poses: poses [B, T*Q, C], index [B, N]')
    B, TQ, C = poses.shape
    N = index.shape[1]
    out = torch.empty((T, B * N, C), dtype=torch.float32, device=poses.device)
    _launch('pave_gather_frame_poses_f32', 'gather_frame_poses', poses.device,
            poses.data_ptr(), index.data_ptr(), out.data_ptr(), B, int(T), TQ // T, N, C)
    return out


def gather_rows_add(src, index, add=None):
    """src [n, S, C] fp32 (rows dense, any batch stride), index [n, Q] int64 -> rows [n, Q, C] = src[b, index[b, q]]
    and, with add [Q, C], (rows, rows + add): the proposal top-k's `tgt` and `query = tgt + query`
    (OT:21386, 21417) in one launch -- pave_gather_rows_add_f32."""
    _require(src.is_cuda and src.dtype == torch.float32 and src.dim() == 3 and src.stride(2) == 1
             and src.stride(1) == src.shape[2], 'gather_rows_add: src [n, S, C] fp32 on the device, dense rows')
    _dev(index, 'index', torch.int64)
    n, S, C = src.shape
    _require(index.dim() == 2 and index.shape[0] == n, 'gather_rows_add: index [n, Q]')
    Q = index.shape[1]
    rows = torch.empty((n, Q, C), dtype=torch.float32, device=src.device)
    total = None
    if add is not None:
        _dev(add, 'add', torch.float32)
        _require(tuple(add.shape) == (Q, C), 'gather_rows_add: add [Q, C]')
        total = torch.empty_like(rows)
    _launch('pave_gather_rows_add_f32', 'gather_rows_add', src.device,
            src.data_ptr(), src.stride(0) if n > 1 else 0, index.data_ptr(), _ptr(add), rows.data_ptr(),
            _ptr(total), n, Q, S, C)
    return rows if add is None else (rows, total)


def proposal_refs_(kpt, props, index, T):
    """kpt [n, Q, 2K] fp32 (unit column stride; a column slice of a padded matrix is fine), in place:
    kpt[..., 0::2] += props[b, index, 0], kpt[..., 1::2] += props[b, index, 1] (props [n or 1, S, 2]); returns
    refs [n, T*Q, 2K] = sigmoid(kpt) repeated for the T frames (OT:21390-21391, 21412) -- pave_proposal_refs_f32."""
    _require(kpt.is_cuda and kpt.dtype == torch.float32 and kpt.dim() == 3 and kpt.stride(2) == 1
             and kpt.stride(0) == kpt.shape[1] * kpt.stride(1), 'proposal_refs_: kpt [n, Q, 2K] fp32, rows evenly strided')
    _dev(index, 'index', torch.int64)
    n, Q, K2 = kpt.shape
    _require(props.is_cuda and props.dtype == torch.float32 and props.dim() == 3 and props.shape[2] == 2
             and props.shape[0] in (1, n) and props[0].is_contiguous(), 'proposal_refs_: props [n | 1, S, 2] fp32')
    _require(tuple(index.shape) == (n, Q), 'proposal_refs_: index [n, Q]')
    refs = torch.empty((n, int(T) * Q, K2), dtype=torch.float32, device=kpt.device)
    _launch('pave_proposal_refs_f32', 'proposal_refs_', kpt.device,
            kpt.data_ptr(), kpt.stride(1), props.data_ptr(),
            props.stride(0) if props.shape[0] > 1 else 0, index.data_ptr(),
            refs.data_ptr(), n, Q, props.shape[1], K2, int(T))
    return refs


def pose_finalize(kpts, sigmas, scores, wh, sf=None):
    """Post-processing of the refined poses (HEAD:1440-1490 + get_p) in one launch:
    kpts, sigmas [B, N, K, 2], scores [B, N], wh [B, 2] (image w, h), sf [B, 2] or None (rescale)
    -> (det_kpts [B, N, K, 3], det_bboxes [B, N, 5])."""
    for t, nm in ((kpts, 'kpts'), (scores, 'scores'), (wh, 'wh')):
        _dev(t, nm, torch.float32)
    # sigmas: dense, or evenly strided (x, y) rows -- a 2-column slice of the sigma branch's padded output
    _require(sigmas.is_cuda and sigmas.dtype == torch.float32 and sigmas.dim() == 4 and sigmas.stride(3) == 1
             and sigmas.stride(1) == sigmas.shape[2] * sigmas.stride(2)
             and sigmas.stride(0) == sigmas.shape[1] * sigmas.stride(1) and sigmas.stride(2) >= 2,
             'pose_finalize: sigmas [B, N, K, 2] fp32 on the device, rows evenly strided')
    sigma_ld = sigmas.stride(2)
    _require(kpts.dim() == 4 and kpts.shape[-1] == 2 and kpts.shape == sigmas.shape
             and tuple(scores.shape) == tuple(kpts.shape[:2]) and wh.numel() == 2 * kpts.shape[0],
             'pose_finalize: kpts / sigmas [B, N, K, 2], scores [B, N], wh [B, 2]')
    B, N, K, _ = kpts.shape
    if sf is not None:
        _dev(sf, 'sf', torch.float32)
        _require(sf.numel() == 2 * B, 'pose_finalize: sf [B, 2]')
    det_kpts = torch.empty((B, N, K, 3), dtype=torch.float32, device=kpts.device)
    det_bboxes = torch.empty((B, N, 5), dtype=torch.float32, device=kpts.device)
    _launch('pave_pose_finalize_f32', 'pose_finalize', kpts.device,
            kpts.data_ptr(), sigmas.data_ptr(), scores.data_ptr(), wh.data_ptr(), _ptr(sf),
            det_kpts.data_ptr(), det_bboxes.data_ptr(), B, N, K, int(sf is not None), sigma_ld)
    return det_kpts, det_bboxes


def split_conv3x3_weight(weight, planes=3):
    """Conv2d weight [Cout, Cin, 3, 3] -> the operand of `conv3x3_split`: rows [Cout, (ky, kx, cin)]
    split and re-laid by `split_weight_bf16x3`."""
    _require(weight.dim() == 4 and tuple(weight.shape[2:]) == (3, 3), 'split_conv3x3_weight: [Cout,Cin,3,3]')
    cout, cin = weight.shape[:2]
    # 3 planes: rows / columns zero-padded to Cout % 64 == 0, 9 Cin % 32 == 0 (HRNet's 48 / 96 channels)
    return split_weight_bf16x3(weight.permute(0, 2, 3, 1).reshape(cout, 9 * cin).contiguous(), planes,
                               pad=planes in _Q_PLANES)


def bottleneck_chain(c1, w2_planes, b2, w3_planes, b3, residual=None, a2=None, w1n_planes=None,
                     b1n=None, out=None, c2=None):
    """One launch for a 64-channel ResNet Bottleneck from its 3x3 convolution on, chained with the
    next block's conv1 (pave_bottleneck_chain_f32):  c1 [N, 64, H, W] channels_last ->
    out = relu(conv3(relu(conv3x3(c1) + b2)) (+ downsample(a2)) + b3 + residual) [N, 256, H, W] and
    c1n = relu(conv1_next(out) + b1n) [N, cn, H, W] (None without w1n_planes).  residual
    [N, 256, H, W] channels_last (may be given as `out`: in place) or a2 [N, k2, H, W] channels_last
    with w3_planes = the planes of the [256, 64 + k2] concatenated weight.
    c1 = w2_planes = None with c2 [N, 64, H, W] channels_last given: the launch starts at conv3
    (the 3x3 was run by conv3x3_split)."""
    tail_only = c1 is None
    src = c2 if tail_only else c1
    _require(src is not None and src.is_cuda and src.dtype == torch.float32 and src.dim() == 4
             and src.shape[1] == 64 and src.is_contiguous(memory_format=torch.channels_last),
             'bottleneck_chain: c1 (or c2) [N, 64, H, W] fp32 channels_last')
    _require((w2_planes is None) == tail_only, 'bottleneck_chain: c1 and w2_planes go together')
    N, _, H, W = src.shape
    M = N * H * W
    npl = _planes(w3_planes, 'w3_planes', only=_Q_PLANES)
    k2 = 0
    if a2 is not None:
        _require(residual is None and a2.is_cuda and a2.dtype == torch.float32 and a2.dim() == 4
                 and tuple(a2.shape[0:1] + a2.shape[2:]) == (N, H, W)
                 and a2.is_contiguous(memory_format=torch.channels_last),
                 'bottleneck_chain: a2 [N, k2, H, W] channels_last, no residual')
        k2 = a2.shape[1]
    if not tail_only:
        _require(_planes(w2_planes, 'w2_planes') == npl, 'bottleneck_chain: one operand mode for all weights')
        _require(tuple(w2_planes.shape) == (36, w3_planes.shape[1], 64, 16), 'bottleneck_chain: w2_planes [36, 3, 64, 16]')
    _require(tuple(w3_planes.shape) == ((64 + k2) // 16, w3_planes.shape[1], 256, 16),
             'bottleneck_chain: w3_planes [(64 + k2)/16, 3, 256, 16]')
    if residual is not None:
        _require(residual.is_cuda and residual.dtype == torch.float32
                 and tuple(residual.shape) == (N, 256, H, W)
                 and residual.is_contiguous(memory_format=torch.channels_last),
                 'bottleneck_chain: residual [N, 256, H, W] channels_last')
    cn = 0
    if w1n_planes is not None:
        _require(_planes(w1n_planes, 'w1n_planes') == npl, 'bottleneck_chain: one operand mode for all weights')
        cn = w1n_planes.shape[2]
        _require(tuple(w1n_planes.shape) == (16, w3_planes.shape[1], cn, 16) and cn in (64, 128),
                 'bottleneck_chain: w1n_planes [16, 3, 64 | 128, 16]')
    for b, n in ((b2, 64), (b3, 256), (b1n, cn)):
        if b is not None:
            _dev(b, 'bias', torch.float32)
            _require(b.numel() == n, 'bottleneck_chain: bias sizes 64 / 256 / cn')
    if out is None:
        out = torch.empty((N, H, W, 256), dtype=torch.float32, device=src.device).permute(0, 3, 1, 2)
    else:
        _require(out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (N, 256, H, W)
                 and out.is_contiguous(memory_format=torch.channels_last),
                 'bottleneck_chain: out [N, 256, H, W] channels_last')
    if not tail_only:
        c2 = torch.empty((M, 64), dtype=torch.float32, device=src.device)
    c1n = torch.empty((N, H, W, cn), dtype=torch.float32, device=src.device) if cn else None
    flops = 2 * M * ((0 if tail_only else 576 * 64) + (64 + k2) * 256 + 256 * cn)
    _launch('pave_bottleneck_chain_f32', 'bottleneck_chain', src.device,
            _ptr(c1), _ptr(w2_planes), _ptr(b2), c2.data_ptr(), w3_planes.data_ptr(), _ptr(b3),
            _ptr(residual), _ptr(a2), k2, out.data_ptr(), _ptr(w1n_planes), _ptr(b1n), _ptr(c1n), cn,
            N, H, W, npl,
            tag='bottleneck_chain', flops=flops, shape=(M, 64, 256, cn, f'k2={k2}', 'tail' if tail_only else ''))
    return out, (c1n.permute(0, 3, 1, 2) if cn else None)


def conv3x3_split(x, w_planes, bias=None, stride=1, relu=False, fp16=False, residual=None, cout=None):
    """3x3 / pad 1 convolution of a channels_last map through the split-operand GEMM kernel
    (implicit GEMM), bias (+ residual) (+ReLU) fused.  x [N, Cin, H, W] channels_last; w_planes =
    split_conv3x3_weight(weight) -> [N, Cout, Ho, Wo] channels_last.  `cout` = the real number of
    output channels when the planes were zero-padded (3 planes: Cin % 16 == 0, Cout % 4 == 0);
    residual [N, Cout, Ho, Wo] channels_last is added before the ReLU (3 planes)."""
    lib = native.load()
    _nhwc(x, 'conv3x3_split')
    npl = _planes(w_planes, fp16=fp16)
    N, Cin, H, W = x.shape
    kp = 9 * Cin if npl not in _Q_PLANES else (9 * Cin + 31) // 32 * 32
    _require(w_planes.shape[0] * 16 == kp, 'conv3x3_split: w_planes [9*Cin/16, P, Cout, 16] (split_conv3x3_weight)')
    Cout = int(cout) if cout is not None else w_planes.shape[2]
    _require((Cout + 63) // 64 * 64 == w_planes.shape[2], 'conv3x3_split: cout does not match the planes')
    if bias is not None:
        _dev(bias, 'bias', torch.float32)
        _require(bias.numel() == Cout, 'conv3x3_split: bias [Cout]')
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    if residual is not None:
        _require(residual.is_cuda and residual.dtype == torch.float32
                 and tuple(residual.shape) == (N, Cout, Ho, Wo)
                 and residual.is_contiguous(memory_format=torch.channels_last),
                 'conv3x3_split: residual [N, Cout, Ho, Wo] channels_last')
    y = torch.empty((N, Ho, Wo, Cout), dtype=torch.float32, device=x.device)
    # few output pixels, many input channels: the split-K form (parts of the K axis on their own
    # workgroups, ordered sum in a second launch); the workspace comes from torch's stream-aware
    # caching allocator
    ws_bytes = lib.pave_conv3x3_splitk_workspace_bytes(N, H, W, Cin, Cout, int(stride)) \
        if npl in _Q_PLANES else 0
    if ws_bytes > 0:
        ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=x.device)
        _launch('pave_conv3x3_splitk_f32', 'conv3x3_splitk', x.device,
                x.data_ptr(), w_planes.data_ptr(), _ptr(bias), _ptr(residual),
                y.data_ptr(), N, H, W, Cin, Cout, int(stride), int(bool(relu)), ws.data_ptr(), ws_bytes, npl,
                tag='conv3x3_split', flops=2 * N * Ho * Wo * Cout * 9 * Cin,
                shape=(N * Ho * Wo, 9 * Cin, Cout, f'3x3 s{stride} split-K', 'res' if residual is not None else ''))
        return y.permute(0, 3, 1, 2)
    _launch('pave_conv3x3_split_f32', 'conv3x3_split', x.device,
            x.data_ptr(), w_planes.data_ptr(), _ptr(bias), _ptr(residual),
            y.data_ptr(), N, H, W, Cin, Cout, int(stride), int(bool(relu)), npl,
            tag='conv3x3_split', flops=2 * N * Ho * Wo * Cout * 9 * Cin,
            shape=(N * Ho * Wo, 9 * Cin, Cout, f'3x3 s{stride}', 'res' if residual is not None else ''))
    return y.permute(0, 3, 1, 2)
