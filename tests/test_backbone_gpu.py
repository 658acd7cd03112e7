"""The backbones' and the neck's DEVICE paths, stage by stage against fp64 (cases, references and the metric:
tests/backbone_cases.py).  Needs an MI355X.

Every case runs the module under no_grad on the device, reads all outputs after the whole forward has finished,
and asserts for every output level

    e_dev = max|got - ref64| / rms(ref64)  <=  8 * e_cpu32,

e_cpu32 being the same metric for the plain fp32 CPU run of the reference (2e-6 .. 1e-5; asserted <= 2e-5 in
tests/test_backbone_cpu.py).  Why 8: folding BatchNorm into the weights alone moves the CPU fp32 result to up to
2.3 x the unfused floor; the three-plane operand split, other tile summation orders and fused epilogues add a few
roundings more; 8 leaves about 3.5 x over that and is still more than 50 times tighter than the end-to-end
comparison of the encoder memory (rtol 2e-3).  There is no absolute tolerance.

Every case also asserts: the input is bit-unchanged; the outputs of a first call are bit-unchanged after a second
forward of the same module on another image (a stage output reused as a temporary would show); the entry points the
case exists for were launched (recorded through ops._launch), and those it must NOT take were not; in 'bf16x3'
mode with bricks._GEMM['min_rows'] = 1 the LaunchCensus of the forward has no fallback operator except the ones the
case lists.

Largest e_dev / e_cpu32 per model family over all cases and levels, measured on the MI355X (a ratio above 8 is a
finding to explain and fix, not a constant to raise):

    family            'native'   'bf16x3'
    ResNet-50           2.19       2.62      (96x100, n = 3)
    HRNet-w48           2.28       4.65      (96x160, n = 1)
    Swin-T / Swin-L w.   --        1.34      (the device path runs in the split mode only)
    ChannelMapper       3.54       2.61 flat, 3.54 per level   (the extra level; per level: a library convolution)

Findings of the first run, fixed with it:
  * HRNet-w48 in 'bf16x3' mode sat at 9.25 / 8.47 / 8.49 x the floor (ResNet-50: 3.1).  Both operands of the split
    GEMMs were split by truncation, so the three products the kernels leave out all had the sign of a b and every
    product came out about 2^-24 short -- a same-signed error that adds up over ~80 convolutions in a row instead of
    averaging out.  The weights' terms are now rounded (pave_split_bf16x3_f32; still an exact split): 4.65 and 2.62.
  * a 1x1 map (ResNet layer4 of a 32x32 frame, HRNet's coarsest branch) was refused by ops.bias_act_rows_ in
    'native' mode ("channels must be innermost"): [N, C, 1, 1] is dense in both layouts.
  * ChannelMapper with out_channels = 96 in the split mode: the extra level's 3x3 launch was not told the real width
    and came back 128 channels wide (necks._conv_split).
Sensitivity, measured once and not committed: one folded bias of layer3 (layer3.0 conv2) times 1 + 1e-3 puts levels 2
and 3 of every ResNet case at 10 .. 16 x the floor (all ten default cases fail, levels 0 and 1 untouched) while the
end-to-end encoder-memory comparison still passes; times 1 + 1e-4 the shift (about 1.4e-6 of the level's RMS) stays
inside fp32 rounding: level 2 moves from 1.5 to 2.1 x the floor and nothing fails.
"""
import collections
import time

import pytest
import torch

from tests import backbone_cases as BC

pytestmark = pytest.mark.gpu

MARGIN = 8

S7 = 'pave_conv7x7s2_nchw_split_f32'
RP = 'pave_repitch_rows_f32'
MP = 'pave_bias_relu_maxpool_nhwc_f32'
CH = 'pave_bottleneck_chain_f32'
ST = 'pave_conv1x1_strided_split_f32'
C3 = ('pave_conv3x3_split_f32', 'pave_conv3x3_splitk_f32')      # (the split-K form: few pixels, long K)
G = ('pave_gemm_bf16x3_f32', 'pave_gemm_bf16x3_splitk_f32')
CAT = 'pave_gemm_bf16x3_cat_f32'
RG = 'pave_rows_gemm_bias_res_act_f32'
BA = 'pave_bias_act_rows_f32'
C3N = 'pave_conv3x3_nhwc_f32'
HS = 'pave_conv3x3s2_c3_nchw_f32'
FS = 'pave_fuse_sum_nhwc_f32'
WA = 'pave_swin_window_attn_f32'
LN = 'pave_bias_add_layernorm_f32'
GN = 'pave_groupnorm_levels_nhwc_f32'
GN1 = 'pave_groupnorm_nhwc_f32'


@pytest.fixture
def gemm_mode(request):
    """'native' | 'bf16x3' | ('bf16x3', None): the GEMM mode of the case, set and restored here.  The split mode
    runs with min_rows = 1 (the hand-written kernels at test sizes too) unless the case asks for the default."""
    from pavenet_amd import bricks
    param = request.param
    mode, rows = param if isinstance(param, tuple) else (param, 1)
    old_mode, old_rows = bricks.get_gemm_mode(), bricks._GEMM['min_rows']
    bricks.set_gemm_mode(mode)
    if mode != 'native' and rows is not None:
        bricks._GEMM['min_rows'] = rows
    try:
        yield mode
    finally:
        bricks.set_gemm_mode(old_mode)
        bricks._GEMM['min_rows'] = old_rows


BOTH = pytest.mark.parametrize('gemm_mode', ['native', 'bf16x3'], indirect=True)
SPLIT = pytest.mark.parametrize('gemm_mode', ['bf16x3'], indirect=True)


def _count(counter, name):
    return sum(counter[n] for n in name) if isinstance(name, tuple) else counter[name]


def _check_launches(names, present=(), absent=(), counts=None):
    c = collections.Counter(names)
    for p in present:
        assert _count(c, p) > 0, f'{p} was not launched: {dict(c)}'
    for a in absent:
        assert _count(c, a) == 0, f'{a} was launched {_count(c, a)} x: {dict(c)}'
    for name, n in (counts or {}).items():
        assert _count(c, name) == n, f'{name}: {_count(c, name)} launches, expected {n}: {dict(c)}'


def _assert_levels(what, outs, ref, floors):
    assert len(outs) == len(ref) == len(floors)
    ratios = []
    for o, r, fl in zip(outs, ref, floors):
        assert tuple(o.shape) == tuple(r.shape), (tuple(o.shape), tuple(r.shape))
        ratios.append(BC.rel_err(o, r) / fl)
    print(f'\n[{what}] e_dev / e_cpu32 = ' + ' '.join(f'{x:.2f}' for x in ratios)
          + '   (e_cpu32 = ' + ' '.join(f'{x:.2e}' for x in floors) + ')')
    for lvl, x in enumerate(ratios):
        assert x <= MARGIN, f'{what}: level {lvl}: e_dev = {x:.2f} x e_cpu32 ({x * floors[lvl]:.3e})'
    return ratios


def _run(monkeypatch, what, module, make_input, ref, floors, mode, present=(), absent=(), counts=None,
         census_expected=(), assert_census=True):
    """Two forwards of `module`: image 'a' under the launch recorder (values, input, entry points), image 'b' under
    the census (fallback operators; and the first call's outputs must survive it).  make_input(which) -> the device
    input (a tensor or a list of tensors)."""
    from pavenet_amd.census import LaunchCensus
    t0 = time.perf_counter()
    xa, xb = make_input('a'), make_input('b')
    tensors = lambda x: [x] if isinstance(x, torch.Tensor) else list(x)    # noqa: E731
    keep_in = [t.clone() for t in tensors(xa)]
    with torch.no_grad(), BC.record_launches(monkeypatch) as names:
        outs = module(xa)
    torch.cuda.synchronize()
    first = [o.clone() for o in outs]
    with torch.no_grad(), LaunchCensus() as census:
        outs_b = module(xb)
    torch.cuda.synchronize()
    for t, k in zip(tensors(xa), keep_in):
        assert torch.equal(t, k), f'{what}: the forward wrote into its input'
    for lvl, (o, k) in enumerate(zip(outs, first)):
        assert torch.equal(o, k), f'{what}: output level {lvl} of the first call changed during the second forward'
    assert len(outs_b) == len(outs) and all(bool(torch.isfinite(o).all()) for o in outs_b)
    ratios = _assert_levels(what, outs, ref, floors)
    _check_launches(names, present, absent, counts)
    fb = dict(census.fallback_ops)
    print(f'[{what}] fallback_ops = {fb}   {time.perf_counter() - t0:.2f} s')
    if mode == 'bf16x3' and assert_census:
        for op in census_expected:
            assert op in fb, f'{what}: expected the fallback operator {op}: {fb}'
        assert set(fb) <= set(census_expected), f'{what}: fallback operators on the device path: {fb}'
    return outs, ratios


# ---- ResNet-50 --------------------------------------------------------------------------------------------------
def _resnet(monkeypatch, mode, canvas, n, what, setup=None, **kw):
    m = BC.new_module('resnet50')
    if setup is not None:
        setup(m)                    # (before the first forward: the folded operands are cached per parameter set)
    m = m.cuda()
    outs, _ = _run(monkeypatch, f'resnet50 {what} {canvas[0]}x{canvas[1]} n={n} {mode}', m,
                   lambda which: BC.frames(canvas, n, which)[None].cuda(),          # [1, n, 3, H, W]
                   BC.reference('resnet50', canvas, n), BC.floor('resnet50', canvas, n), mode, **kw)
    for o in outs:
        assert o.is_contiguous(memory_format=torch.channels_last)
    return m


@BOTH
@pytest.mark.parametrize('case', BC.RESNET_CASES, ids=BC.case_id)
def test_resnet50_stages_vs_fp64(monkeypatch, gemm_mode, case):
    canvas, n = case
    W = canvas[1]
    if gemm_mode == 'bf16x3':
        # the split stem (re-pitched rows for W % 4 != 0; declined below 8 columns), the max-pool pass, layer1 as
        # three chained launches that also run layer2.0's conv1, the strided downsample GEMM of layers 2 - 4
        present = [MP, CH, ST, C3, G] + ([S7] if W >= 8 else []) + ([RP] if W % 4 and W >= 8 else [])
        absent = [CAT, RG, BA, C3N] + ([S7, RP] if W < 8 else []) + ([RP] if W % 4 == 0 else [])
        counts = {CH: 3, ST: 3, C3: 13}
    else:
        # vendor GEMMs / convolutions + this package's max-pool, one-kernel tails (K <= 256) and bias passes (layer4)
        present, absent, counts = [MP, RG, BA], [S7, RP, CH, ST, C3, G, CAT, C3N], {RG: 13}
    _resnet(monkeypatch, gemm_mode, canvas, n, 'default', present=present, absent=absent, counts=counts,
            census_expected=('convolution',) if W < 8 else ())


def _set(**attrs):
    def setup(m):
        for k, v in attrs.items():
            assert hasattr(m, k)
            setattr(m, k, v)
    return setup


@SPLIT
def test_resnet50_layer1_per_block_path(monkeypatch, gemm_mode):
    """chain_stage64=False: layer1 block by block -- layer1.0's conv3 + downsample as the two-source GEMM."""
    canvas, n = BC.RESNET_SWITCH_CASE
    _resnet(monkeypatch, gemm_mode, canvas, n, 'chain_stage64=False', _set(chain_stage64=False),
            present=[S7, RP, MP, ST, C3, G, CAT], absent=[CH, RG, BA], counts={CAT: 1, C3: 16, ST: 3})


@SPLIT
def test_resnet50_tail_chain(monkeypatch, gemm_mode):
    """chain_mode='tail': the 3x3 of every layer1 block as a launch of its own, the chain from conv3 on."""
    canvas, n = BC.RESNET_SWITCH_CASE
    _resnet(monkeypatch, gemm_mode, canvas, n, "chain_mode='tail'", _set(chain_mode='tail'),
            present=[S7, RP, MP, CH, ST, C3, G], absent=[CAT, RG, BA], counts={CH: 3, C3: 16, ST: 3})


@pytest.mark.parametrize('gemm_mode', ['native'], indirect=True)
def test_resnet50_deterministic_conv3x3(monkeypatch, gemm_mode):
    """deterministic_conv3x3=True is read where the split 3x3 is not taken (native mode): all 16 3x3 convolutions
    through pave_conv3x3_nhwc_f32."""
    canvas, n = BC.RESNET_SWITCH_CASE
    _resnet(monkeypatch, gemm_mode, canvas, n, 'deterministic_conv3x3', _set(deterministic_conv3x3=True),
            present=[MP, C3N, RG, BA], absent=[S7, CH, ST, C3, G, CAT], counts={C3N: 16, RG: 13})


@pytest.mark.parametrize('gemm_mode', [('bf16x3', None)], indirect=True)
def test_resnet50_default_min_rows(monkeypatch, gemm_mode):
    """bricks._GEMM['min_rows'] at its default (8192 > the 2 584 pixels of layer1 here): the chain gate refuses, and
    every 1x1 takes the small-row form of the split GEMM (layer1.0: the two-source GEMM)."""
    from pavenet_amd import bricks
    canvas, n = BC.RESNET_SWITCH_CASE
    assert 2 * 19 * 34 < bricks._GEMM['min_rows']
    _resnet(monkeypatch, gemm_mode, canvas, n, 'min_rows=default',
            present=[S7, RP, MP, ST, C3, G, CAT], absent=[CH, RG], counts={CAT: 1, C3: 16, ST: 3},
            assert_census=False)


@BOTH
def test_resnet50_no_fused_tails(monkeypatch, gemm_mode):
    """fused_tail_max_k=0: no [K, N] tail operand is built -- in native mode every tail is a vendor GEMM + the
    bias / ReLU pass; in the split mode the concatenated layer1.0 tail goes with it, so the chain gate refuses and
    layer1 runs block by block on the split GEMM."""
    canvas, n = BC.RESNET_SWITCH_CASE
    if gemm_mode == 'bf16x3':
        kw = dict(present=[S7, RP, MP, ST, C3, G], absent=[CH, CAT, RG, BA], counts={C3: 16, ST: 3})
    else:
        kw = dict(present=[MP, BA], absent=[RG, S7, CH, ST, C3, G, CAT])
    m = _resnet(monkeypatch, gemm_mode, canvas, n, 'fused_tail_max_k=0', _set(fused_tail_max_k=0), **kw)
    assert not any(isinstance(k, tuple) and k[2] in ('conv3_kn', 'tail_ds_kn') for k in m._folded[1])


@BOTH
def test_resnet50_no_fused_downsample_tail(monkeypatch, gemm_mode):
    """fused_ds_max_k=0: layer1.0's concatenated [W3; Wd] tail disappears, and the chain gate must refuse (the
    chained launch of a downsample block needs exactly that operand)."""
    canvas, n = BC.RESNET_SWITCH_CASE
    if gemm_mode == 'bf16x3':
        kw = dict(present=[S7, RP, MP, ST, C3, G], absent=[CH, CAT, RG, BA], counts={C3: 16, ST: 3})
    else:
        kw = dict(present=[MP, RG, BA], absent=[S7, CH, ST, C3, G, CAT], counts={RG: 13})
    m = _resnet(monkeypatch, gemm_mode, canvas, n, 'fused_ds_max_k=0', _set(fused_ds_max_k=0), **kw)
    keys = [k for k in m._folded[1] if isinstance(k, tuple)]
    assert not any(k[2] == 'tail_ds_kn' for k in keys) and any(k[2] == 'conv3_kn' for k in keys)


# ---- HRNet-w48 --------------------------------------------------------------------------------------------------
@BOTH
@pytest.mark.parametrize('case', BC.HRNET_CASES, ids=BC.case_id)
def test_hrnet_w48_branches_vs_fp64(monkeypatch, gemm_mode, case):
    canvas, n, layout = case

    def make_input(which):
        x = BC.frames(canvas, n, which).cuda()
        if layout == '5d':
            return x[None]
        if layout == 'channels_last':
            x = x.contiguous(memory_format=torch.channels_last)
            assert not x.is_contiguous()
        return x
    nchw = layout != 'channels_last'
    if gemm_mode == 'bf16x3':
        # stem conv1 from the NCHW batch (a channels_last batch: the library convolution + the bias pass, Cin = 3
        # is off the split kernel's grid), every other 3x3 and 1x1 on the split kernels, the fuse sums in one pass
        present = [FS, C3, G] + ([HS] if nchw else [BA])
        absent = [BA] if nchw else [HS]
    else:
        present, absent = [FS, BA] + ([HS] if nchw else []), [C3, G] + ([] if nchw else [HS])
    m = BC.new_module('hrnet_w48').cuda()
    _run(monkeypatch, f'hrnet_w48 {layout} {canvas[0]}x{canvas[1]} n={n} {gemm_mode}', m, make_input,
         BC.reference('hrnet_w48', canvas, n), BC.floor('hrnet_w48', canvas, n), gemm_mode,
         present=present, absent=absent, census_expected=() if nchw else ('convolution',))


# ---- Swin -------------------------------------------------------------------------------------------------------
@SPLIT      # (the device path runs in the fused GEMM modes only; elsewhere the module is its torch formulation)
@pytest.mark.parametrize('n', BC.SWIN_FRAMES)
@pytest.mark.parametrize('canvas', BC.SWIN_CANVASES, ids=BC.case_id)
@pytest.mark.parametrize('shape', sorted(BC.SWIN_SHAPES))
def test_swin_stages_vs_fp64(monkeypatch, gemm_mode, shape, canvas, n):
    m = BC.new_module(shape).cuda()
    blocks = sum(BC.SWIN_SHAPES[shape]['depths'])
    _run(monkeypatch, f'{shape} {canvas[0]}x{canvas[1]} n={n}', m,
         lambda which: BC.frames(canvas, n, which).cuda(),
         BC.reference(shape, canvas, n), BC.floor(shape, canvas, n), gemm_mode,
         present=[WA, G, LN], counts={WA: blocks})


# ---- ChannelMapper, isolated ------------------------------------------------------------------------------------
def _neck_input(chans, canvas):
    return lambda which: [f.cuda() for f in BC.neck_inputs(chans, canvas, which)]


def _assert_flat_layout(outs):
    """The four maps are consecutive row ranges of ONE [n, S, C] buffer, in level order."""
    n, C = outs[0].shape[:2]
    S = sum(o.shape[2] * o.shape[3] for o in outs)
    base = outs[0].untyped_storage().data_ptr()
    st = 0
    for o in outs:
        h, w = o.shape[2:]
        rows = o.permute(0, 2, 3, 1)
        assert o.untyped_storage().data_ptr() == base and o.storage_offset() == st * C
        assert all(rows.stride(d) == s for d, s in enumerate((S * C, w * C, C, 1)) if rows.shape[d] > 1)
        st += h * w
    assert outs[0].untyped_storage().nbytes() == n * S * C * 4


@BOTH
@pytest.mark.parametrize('case', BC.NECK_CASES, ids=BC.case_id)
def test_channel_mapper_vs_fp64(monkeypatch, gemm_mode, case):
    chans, canvas, cout = case
    ref, floors = BC.neck_reference(chans, canvas, cout), BC.neck_floor(chans, canvas, cout)
    what = f'channel_mapper {BC.case_id(case)} {gemm_mode}'
    m = BC.new_neck(chans, cout).cuda()
    assert m.flat_output
    # flat: every level's GroupNorm in the same launches; split mode: the 1x1 laterals (K = 96: zero-padded planes)
    # and the stride-2 3x3 on the split kernels
    present = [GN] + ([G, C3] if gemm_mode == 'bf16x3' else [])
    absent = [GN1] + ([] if gemm_mode == 'bf16x3' else [G, C3])
    flat, _ = _run(monkeypatch, what + ' flat', m, _neck_input(chans, canvas), ref, floors, gemm_mode,
                   present=present, absent=absent)
    _assert_flat_layout(flat)
    # flat_output=False: ConvModule by ConvModule (library convolution + torch GroupNorm, no kernel shared with the
    # flat path): the same network within the same bound
    m2 = BC.new_neck(chans, cout).cuda()
    m2.flat_output = False
    plain, _ = _run(monkeypatch, what + ' per-level', m2, _neck_input(chans, canvas), ref, floors, gemm_mode,
                    absent=[GN, GN1, G, C3], assert_census=False)
    for a, b in zip(flat, plain):
        assert a.shape == b.shape


@BOTH
def test_channel_mapper_groupnorm_torch_branch(monkeypatch, gemm_mode):
    """out_channels = 96: C / G = 3 is off the HIP GroupNorm's grid, so _forward_flat takes its torch statistics
    branch level by level (var_mean in the census) -- still into the one flat buffer."""
    chans, canvas, cout = BC.NECK_CASE_C96
    m = BC.new_neck(chans, cout).cuda()
    outs, _ = _run(monkeypatch, f'channel_mapper {BC.case_id(BC.NECK_CASE_C96)} {gemm_mode}', m,
                   _neck_input(chans, canvas), BC.neck_reference(chans, canvas, cout),
                   BC.neck_floor(chans, canvas, cout), gemm_mode,
                   present=[G, C3] if gemm_mode == 'bf16x3' else [], absent=[GN, GN1],
                   census_expected=('var_mean',))
    _assert_flat_layout(outs)
