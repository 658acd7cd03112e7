"""What tests/test_backbone_gpu.py stands on, checked without a GPU:

1. the modules' CPU fallback in fp64 IS the oracle's network at every canvas of the GPU cases, the odd ones
   included (ResNet with out_indices=(0, 1, 2, 3) and the 5-D `mul_frames` input, HRNet, ChannelMapper);
2. the fp32 floor of every case is small enough for the GPU bound (8 x floor) to mean something.
"""
import pytest
import torch

from tests import backbone_cases as BC

MODULE_EQ_ORACLE = 1e-10    # fp64 against fp64: BatchNorm as an affine map vs folded into the weights
FLOOR_MAX = 2e-5            # a condition on the cases, not a measurement (largest seen: 1.03e-5, Swin-L widths,
#                             stage 3 at 75x133); a case that breaks it gets another canvas


@pytest.mark.parametrize('case', BC.RESNET_CASES, ids=BC.case_id)
def test_resnet_module_fp64_is_the_oracle(case):
    canvas, n = case
    m = BC.new_module('resnet50').double()
    assert m.out_indices == (0, 1, 2, 3) and m.input_type == 'mul_frames'
    img = BC.frames(canvas, n).double()[None]                  # [1, n, 3, H, W]
    with torch.no_grad():
        outs = m(img)
    ref = BC.reference('resnet50', canvas, n)
    assert len(outs) == len(ref) == 4
    for lvl, (o, r) in enumerate(zip(outs, ref)):
        e = BC.rel_err(o, r)
        assert e <= MODULE_EQ_ORACLE, (lvl, e)


@pytest.mark.parametrize('case', BC.HRNET_CASES, ids=BC.case_id)
def test_hrnet_module_fp64_is_the_oracle(case):
    canvas, n, layout = case
    m = BC.new_module('hrnet_w48').double()
    img = BC.frames(canvas, n).double()
    if layout == '5d':
        img = img[None]
    elif layout == 'channels_last':
        img = img.contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        outs = m(img)
    ref = BC.reference('hrnet_w48', canvas, n)
    assert len(outs) == len(ref) == 3
    for lvl, (o, r) in enumerate(zip(outs, ref)):
        e = BC.rel_err(o, r)
        assert e <= MODULE_EQ_ORACLE, (lvl, e)


@pytest.mark.parametrize('case', BC.NECK_CASES + (BC.NECK_CASE_C96,), ids=BC.case_id)
def test_channel_mapper_module_fp64_is_the_oracle(case):
    chans, canvas, cout = case
    m = BC.new_neck(chans, cout).double()
    feats = [f.double() for f in BC.neck_inputs(chans, canvas)]
    with torch.no_grad():
        outs = m(feats)
    ref = BC.neck_reference(chans, canvas, cout)
    assert len(outs) == len(ref) == 4
    for lvl, (o, r) in enumerate(zip(outs, ref)):
        e = BC.rel_err(o, r)
        assert e <= MODULE_EQ_ORACLE, (lvl, e)


def _assert_floor(what, floors):
    print(f'{what}: e_cpu32 = ' + ' '.join(f'{e:.2e}' for e in floors))
    for lvl, e in enumerate(floors):
        assert 0 < e <= FLOOR_MAX, (what, lvl, e)


@pytest.mark.parametrize('case', BC.RESNET_CASES, ids=BC.case_id)
def test_resnet_floor(case):
    _assert_floor(BC.case_id(case), BC.floor('resnet50', *case))


@pytest.mark.parametrize('case', BC.HRNET_CASES[:3], ids=BC.case_id)
def test_hrnet_floor(case):
    _assert_floor(BC.case_id(case), BC.floor('hrnet_w48', case[0], case[1]))


@pytest.mark.parametrize('n', BC.SWIN_FRAMES)
@pytest.mark.parametrize('canvas', BC.SWIN_CANVASES, ids=BC.case_id)
@pytest.mark.parametrize('shape', sorted(BC.SWIN_SHAPES))
def test_swin_floor(shape, canvas, n):
    _assert_floor(f'{shape} {canvas} n={n}', BC.floor(shape, canvas, n))


@pytest.mark.parametrize('case', BC.NECK_CASES + (BC.NECK_CASE_C96,), ids=BC.case_id)
def test_channel_mapper_floor(case):
    _assert_floor(BC.case_id(case), BC.neck_floor(*case))
