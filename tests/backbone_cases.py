"""Cases, references and the error metric shared by tests/test_backbone_cpu.py and tests/test_backbone_gpu.py:
the backbones (ResNet-50, HRNet-w48, Swin) and the ChannelMapper neck, stage by stage against fp64.

Weights: the name-seeded recipe (oracle.seeded) under the `backbone.` / `neck.` prefixes the whole model gives
these modules, so a stage here sees the very tensors the end-to-end tests load.  Nothing is rescaled: under these
weights HRNet-w48's activations reach 1e8 (RMS 2e7 .. 4e7) and every value stays finite, which is why the metric
below is relative to the level's RMS and has no absolute term.

References, always fp64 on the CPU:
  ResNet         oracle.pavenet_ref.resnet_forward(..., out_indices=(0, 1, 2, 3))
  HRNet          oracle.pavenet_ref.hrnet_forward
  ChannelMapper  oracle.pavenet_ref.channel_mapper
  Swin           the module's OWN non-device path, `copy.deepcopy(m).double()` on the CPU image.  The oracle has no
                 Swin; pavenet_amd/swin.py's torch formulation is the restatement that is pinned bit for bit to the
                 reference backbone on the CPU (tests/test_oracle_golden.py), and the device path
                 (`SwinTransformer._forward_device`) shares none of its arithmetic with it.

Metric, per output level:  e = max|got - ref64| / rms(ref64).
Floor:  e_cpu32 = the same metric for the plain fp32 CPU run of the same reference against its fp64 run -- what
fp32 arithmetic costs on this network at this canvas, computed from the reference alone.
Every reference is computed once per session (functools.lru_cache) and never modified.
"""
import contextlib
import copy
import functools

import torch

from oracle import pavenet_ref as R
from oracle.seeded import seeded_array, seeded_state_dict

# ---- the cases ------------------------------------------------------------------------------------------------
# ResNet-50, input_type='mul_frames', out_indices=(0, 1, 2, 3), frames [1, n, 3, H, W]:  (canvas, n)
RESNET_CASES = (((64, 96), 2),      # aligned baseline
                ((75, 133), 2),     # W % 4 != 0: the stem re-pitch; maps 38x67, 19x34, 10x17, 5x9, 3x5
                ((96, 100), 3),     # W % 4 == 0, no multiple of 32: maps 25, 13, 7, 4 wide, rows off the 128-row tile
                ((32, 32), 1),      # layer4 is a 1x1 map
                ((40, 7), 1))       # W < 8: the split stem declines, the library stem feeds the max-pool kernel
RESNET_SWITCH_CASE = ((75, 133), 2)

# HRNet-w48 (canvases: multiples of 32 -- the reference itself cannot sum other sizes):  (canvas, n, input layout)
HRNET_CASES = (((64, 96), 3, '5d'),
               ((96, 160), 1, '4d'),
               ((32, 32), 1, '4d'),              # the coarsest branch is 1x1
               ((64, 96), 3, 'channels_last'))   # the `elif fast` stem branch

SWIN_SHAPES = {
    'swin_t': dict(embed_dims=96, depths=(2, 2, 6, 2), num_heads=(3, 6, 12, 24)),
    # Swin-L's widths (the 1536- / 3072-wide LayerNorm forms, 48-head windows), depths trimmed from (2, 2, 18, 2)
    'swin_l_w': dict(embed_dims=192, depths=(2, 2, 2, 2), num_heads=(6, 12, 24, 48)),
}
SWIN_CANVASES = ((75, 133),     # AdaptivePadding to 76x136, then an odd-map merge at every stage
                 (224, 352),    # stage maps are exact multiples of the 7x7 window
                 (100, 60),
                 (28, 28))      # a single 7x7 window, then 4x4 and smaller maps under a shifted window
SWIN_FRAMES = (2, 1)

# ChannelMapper(kernel_size=1, GN(32), act_cfg=None, num_outs=4) on the fp64 backbone reference's outputs cast to
# fp32:  in_channels -> {canvas: (backbone model, levels taken)}.  HRNet cannot run 75x133, so the [96, 192, 384]
# pyramid at that canvas is Swin-T's first three stages (the same widths; maps 19x34, 10x17, 5x9).
NECK_SOURCES = {
    (512, 1024, 2048): {(75, 133): ('resnet50', (1, 2, 3)), (64, 96): ('resnet50', (1, 2, 3))},
    (96, 192, 384): {(75, 133): ('swin_t', (0, 1, 2)), (64, 96): ('hrnet_w48', (0, 1, 2))},
    (384, 768, 1536): {(75, 133): ('swin_l_w', (1, 2, 3)), (64, 96): ('swin_l_w', (1, 2, 3))},
}
NECK_FRAMES = 2
NECK_CASES = tuple((chans, canvas, 256) for chans in NECK_SOURCES for canvas in ((75, 133), (64, 96)))
# C / G = 3: the HIP GroupNorm's shape rule refuses, _forward_flat must take its torch statistics branch
NECK_CASE_C96 = ((512, 1024, 2048), (75, 133), 96)


def case_id(case):
    out = []
    for v in case:
        if isinstance(v, tuple) and len(v) == 2:
            out.append(f'{v[0]}x{v[1]}')
        elif isinstance(v, tuple):
            out.append('-'.join(str(c) for c in v))
        else:
            out.append(str(v))
    return '_'.join(out)


# ---- modules and weights ----------------------------------------------------------------------------------------
def _seed(module, prefix):
    """The name-seeded weights of oracle.seeded under `prefix.` (as tests/test_model_gpu._seed gives the whole
    model); returns the fp32 state dict WITH the prefix, the oracle's input."""
    like = module.state_dict()
    sd = seeded_state_dict({f'{prefix}.{k}': list(v.shape) for k, v in like.items()},
                           like={f'{prefix}.{k}': v for k, v in like.items()})
    module.load_state_dict({k[len(prefix) + 1:]: v for k, v in sd.items()}, strict=True)
    return sd


@functools.lru_cache(maxsize=None)
def _template(model):
    """(never-run fp32 CPU module in eval mode, its prefixed state dict).  Callers take `new_module`: a module that
    has run carries derived caches (folded BatchNorm, split planes) tied to its tensors."""
    from pavenet_amd import models
    from pavenet_amd.backbones import HRNet, ResNet
    from pavenet_amd.swin import SwinTransformer
    if model == 'resnet50':
        m = ResNet(depth=50, input_type='mul_frames', out_indices=(0, 1, 2, 3))
    elif model == 'hrnet_w48':
        m = HRNet(extra=copy.deepcopy(models.HRNET_W48_EXTRA))
    else:
        m = SwinTransformer(out_indices=(0, 1, 2, 3), **SWIN_SHAPES[model])
    sd = _seed(m, 'backbone')
    return m.eval(), sd


def new_module(model):
    return copy.deepcopy(_template(model)[0])


def state_dict(model, dtype=torch.float32):
    return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in _template(model)[1].items()}


@functools.lru_cache(maxsize=None)
def _neck_template(in_channels, out_channels):
    from pavenet_amd.necks import ChannelMapper
    m = ChannelMapper(list(in_channels), out_channels, kernel_size=1, norm_cfg=dict(type='GN', num_groups=32),
                      act_cfg=None, num_outs=4)
    sd = _seed(m, 'neck')
    return m.eval(), sd


def new_neck(in_channels, out_channels=256):
    return copy.deepcopy(_neck_template(tuple(in_channels), out_channels)[0])


def neck_state_dict(in_channels, out_channels=256, dtype=torch.float32):
    return {k: v.to(dtype) for k, v in _neck_template(tuple(in_channels), out_channels)[1].items()}


# ---- inputs and references --------------------------------------------------------------------------------------
def frames(canvas, n, which='a'):
    """fp32 frames [n, 3, H, W] (`which`: 'a' the case's image, 'b' the other image of the second forward)."""
    return torch.from_numpy(seeded_array(f'backbone.{canvas[0]}x{canvas[1]}.{n}.{which}', (n, 3) + tuple(canvas)))


def _run_reference(model, img, dtype):
    img = img.to(dtype)
    with torch.no_grad():
        if model == 'resnet50':
            outs = R.resnet_forward(state_dict(model, dtype), 'backbone', img, out_indices=(0, 1, 2, 3))
        elif model == 'hrnet_w48':
            outs = R.hrnet_forward(state_dict(model, dtype), 'backbone', img)
        else:
            m = new_module(model)
            outs = (m.double() if dtype == torch.float64 else m)(img)
    return tuple(o.contiguous() for o in outs)


@functools.lru_cache(maxsize=None)
def reference(model, canvas, n, which='a'):
    """fp64 stage outputs of `model` on frames(canvas, n, which)."""
    return _run_reference(model, frames(canvas, n, which), torch.float64)


@functools.lru_cache(maxsize=None)
def floor(model, canvas, n):
    """e_cpu32 per level: the fp32 CPU run of the reference against its fp64 run."""
    got = _run_reference(model, frames(canvas, n), torch.float32)
    return tuple(rel_err(g, r) for g, r in zip(got, reference(model, canvas, n)))


@functools.lru_cache(maxsize=None)
def neck_inputs(in_channels, canvas, which='a'):
    """The fp64 backbone reference's outputs cast to fp32: the neck is tested in isolation from backbone error."""
    model, levels = NECK_SOURCES[tuple(in_channels)][tuple(canvas)]
    outs = reference(model, tuple(canvas), NECK_FRAMES, which)
    feats = tuple(outs[i].float().contiguous() for i in levels)
    assert tuple(f.shape[1] for f in feats) == tuple(in_channels)
    return feats


def _run_neck_reference(in_channels, canvas, out_channels, which, dtype):
    feats = [f.to(dtype) for f in neck_inputs(in_channels, canvas, which)]
    with torch.no_grad():
        return tuple(R.channel_mapper(neck_state_dict(in_channels, out_channels, dtype), 'neck', feats))


@functools.lru_cache(maxsize=None)
def neck_reference(in_channels, canvas, out_channels=256, which='a'):
    return _run_neck_reference(in_channels, canvas, out_channels, which, torch.float64)


@functools.lru_cache(maxsize=None)
def neck_floor(in_channels, canvas, out_channels=256):
    got = _run_neck_reference(in_channels, canvas, out_channels, 'a', torch.float32)
    return tuple(rel_err(g, r) for g, r in zip(got, neck_reference(in_channels, canvas, out_channels)))


# ---- metric -----------------------------------------------------------------------------------------------------
def rel_err(got, ref64):
    """max|got - ref64| / rms(ref64) of one level; no absolute term."""
    ref64 = ref64.detach().double().cpu()
    got = got.detach().double().cpu()
    assert got.shape == ref64.shape, (tuple(got.shape), tuple(ref64.shape))
    assert bool(torch.isfinite(got).all()), 'non-finite values'
    rms = float(ref64.pow(2).mean().sqrt())
    assert rms > 0
    return float((got - ref64).abs().max()) / rms


# ---- which path ran ---------------------------------------------------------------------------------------------
@contextlib.contextmanager
def record_launches(monkeypatch):
    """Wraps pavenet_amd.ops._launch -- the one way every kernel of the package is launched -- for the `with` body
    and yields the list that collects the entry-point names, in launch order."""
    from pavenet_amd import ops
    names = []
    real = ops._launch

    def spy(entry, *args, **kwargs):
        names.append(entry)
        return real(entry, *args, **kwargs)
    with monkeypatch.context() as mp:
        mp.setattr(ops, '_launch', spy)
        yield names
