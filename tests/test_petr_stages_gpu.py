"""The single-image family of pavenet_amd/petr.py on the DEVICE, tap by tap against fp64: the encoder (after each of
its six layers), the un-fused proposal stage, PetrTransformerDecoder, the head's branches at every level, the stock
refine decoder over `memory_clip_index`, the result of PETRHead and VedPoseHeadV2 (cases, references, floors:
tests/petr_cases.py; what this file stands on: tests/test_petr_stages_cpu.py).  The sibling of
tests/test_head_stages_gpu.py (the video family); `gemm_mode`, `_check_launches` and `_assert_same_selection` are the
project's own.  Needs an MI355X.

Every case runs bbox_head.forward + get_bboxes under no_grad with the fp64 run's proposals and scores forced, reads
all taps after the whole forward, and asserts for every ratio tap

    e_dev = max|got - ref64| / rms(ref64)  <=  8 * e_cpu32,

e_cpu32 being the same metric for the oracle's own fp32 run with the same forced selections (9e-7 .. 3e-5, recorded
in the CPU file).  There is no absolute tolerance.  The ratio of every tap is printed.  The taps whose reference
leaves no room for error (PETRHead's key-point scores = 1, labels = 0, keep = 1, order = arange(N)) are compared
with torch.equal.

Chained: from the features, in both input forms.  Isolated: the decoder from the fp64 reference memory cast to fp32
(`encode_frames`' result substituted by a monkeypatch), forward_refine from the reference memory and the reference
poses.  Every chained case also asserts: the inputs are bit-unchanged; the first call's taps are bit-unchanged after a
second forward on other features; the entry points the default path stands for were launched; the LaunchCensus of the
second forward lists neither of MultiScaleDeformableAttention's slow-path notes.  A free run (nothing forced) must make
the fp64 run's selections up to near-ties.  p6_first then p2 run on one module, each against its own reference.

Largest e_dev / e_cpu32 per stage over all cases and forms, measured on the MI355X (a ratio above 8 is a finding to
explain and fix, not a constant to raise):

    stage (taps)                                        'native'   'bf16x3'   (where: 'native'; 'bf16x3')
    encoder (mem0 .. mem5)                               1.89       1.49   (p4, three padded images; p1)
    proposals (enc_cls, init_reference)                  1.81       1.41   (p2; p1)
    decoder (hs0 .. hs2, ref0 .. ref2)                   2.95       1.17   (p2; p6_first)
    head (cls0 .. cls2, kpt0 .. kpt2)                    2.48       1.13   (p2)
    refine (refine_hs0/1, refine_kpts, refine_sigma)     2.66       1.20   (p2; p3)
    result (det_kpts, det_kpt_scores, det_bboxes,        3.34       1.83   (p6_first, det_bboxes; p3, det_bboxes)
            the rescaled pair of p2)

The isolated stages sit lower (decoder from the reference memory: at most 2.24 / 1.20; refine from the reference memory
and poses: 0.83 / 0.59).  The exact taps are reproduced bit for bit in every run.
Sensitivity on the device, measured once and not committed: decoder.layers.1.norms.1.bias of the device module
x (1 + 1e-3) on p1 puts hs1 at 42 x the floor in both modes (hs2 at 50 x, thirteen taps over the bound; hs0 unmoved);
unperturbed, the same script gives at most 2.00 ('native') and 1.49 ('bf16x3').

Findings:
  * models.petr_r50_cfg(num_query=Q) did not tell the transformer: it kept two_stage_num_proposals = 300 and selected
    300 proposals for Q query embeddings (p3, p4 and p5, Q = 100, could not run).  Fixed; the regression test is
    tests/test_petr_stages_cpu.py::test_num_query_reaches_the_transformer.
  * No device kernel and no module of this family was found wrong: every tap of every case, form and mode is within
    3.4 x the floor, and the modules' CPU run within 1.7 x.
  * Census: in 'bf16x3' (min_rows = 1) `fallback_ops` was empty on the first run and is asserted empty; `slow_paths` is
    empty in both modes.  In 'native' the projections, FFNs and the attention core are vendor operators by design
    (addmm, _addmm_activation, mm, _scaled_dot_product_efficient_attention, one native_layer_norm), which is why that
    mode's launch list has neither pave_gemm_bf16x3_encproj_f32 nor pave_mha_core_f32.
  * pave_fill_rows_f32 runs in the padded cases (the value rows of masked tokens, after the merged projection) and in
    p5 (the invalid border proposals) in 'bf16x3'; p1 and p3 do not launch it.
"""
import collections
import time

import pytest
import torch

from tests import petr_cases as PC
from tests.test_backbone_gpu import _check_launches, gemm_mode  # noqa: F401  (the fixture is used by name)
from tests.test_model_gpu import _assert_same_selection

pytestmark = pytest.mark.gpu

MARGIN = PC.MARGIN
BOTH = pytest.mark.parametrize('gemm_mode', ['native', 'bf16x3'], indirect=True)
CASE_IDS = [c.name for c in PC.CASES]

TILE = 'pave_enc_deform_attn_tile_f32'
ENCPROJ = 'pave_gemm_bf16x3_encproj_f32'
POSE = 'pave_deform_attn_pose_fused_f32'     # the decoder at T = 1, K = 17 / 15
GRID = 'pave_deform_attn_grid_fused_f32'     # the refine decoder through unit_clip
MHA = 'pave_mha_core_f32'
TOPK = 'pave_topk_rows_f32'
# what the default path launches in every case.  'native': the projections are vendor GEMMs, so the entries that ARE
# split GEMM forms (the merged encoder projection) or are gated on the split modes (the attention core) are not taken
DEFAULT_LAUNCHES = {
    'bf16x3': [TILE, ENCPROJ, POSE, GRID, MHA, TOPK],
    'native': [TILE, POSE, GRID, TOPK],
}
# pave_fill_rows_f32 zeroes the value rows of padded tokens behind the merged projection and overwrites the rows of
# invalid proposals (split modes only).  p1 and p3 have neither and must not launch it; the padded batches and the
# 52-wide level of p5 must
FILL = 'pave_fill_rows_f32'
FILL_CASES = (PC.P2, PC.P4, PC.P5, PC.P6_FIRST)
SLOW_NOTES = ('MultiScaleDeformableAttention: un-fused softmax / locations + generic sampler',
              'encoder layer off the merged-projection path (separate value / offset GEMMs)')


def _assert_taps(what, case, got, names=None):
    names = tuple(names or case.ratio_taps())
    ref, fl = PC.reference(case), PC.floor(case)
    for n in names:
        assert tuple(got[n].shape) == tuple(ref[n].shape), (n, tuple(got[n].shape), tuple(ref[n].shape))
    r = PC.ratios(PC.errors(got, case, names), fl)
    print('\n' + PC.fmt(what, r))
    worst = collections.defaultdict(float)
    for n, v in r.items():
        worst[PC.STAGE[n]] = max(worst[PC.STAGE[n]], v)
    print(f'[{what}] worst per stage: ' + ' '.join(f'{s}={v:.2f}' for s, v in worst.items()))
    for n, v in r.items():
        assert v <= MARGIN, f'{what}: {n}: e_dev = {v:.2f} x e_cpu32 ({v * fl[n]:.3e})'
    return r


def _chained(monkeypatch, case, mode, form, head=None, what=''):
    """Two forwards of the head: the case's features under the launch recorder (taps, inputs, entry points), other
    features under the census (slow paths, fallback operators; the first call's taps must survive it)."""
    from pavenet_amd.census import LaunchCensus
    t0 = time.perf_counter()
    what = f'{case} {form} {mode} {what}'.strip()
    if head is None:
        head = PC.new_head(case).cuda()
    fs, keep_in = PC.feats(case, form, 'cuda')
    before = [t.clone() for t in keep_in]
    with torch.no_grad(), PC.record_launches(monkeypatch) as names:
        got, _, _ = PC.run_head(case, head, fs)
    torch.cuda.synchronize()
    taps = case.ratio_taps() + PC.EXACT_TAPS + ('det_kpt_scores',)
    first = {n: got[n].clone() for n in taps}
    fs_b, _ = PC.feats(case, form, 'cuda', which='other')
    with torch.no_grad(), LaunchCensus() as census:
        got_b, _, _ = PC.run_head(case, head, fs_b)
    torch.cuda.synchronize()
    for t, k in zip(keep_in, before):
        assert torch.equal(t, k), f'{what}: the forward wrote into its input'
    for n in taps:
        assert torch.equal(got[n], first[n]), f'{what}: {n} of the first call changed during the second forward'
        assert bool(torch.isfinite(got_b[n].float()).all()), (what, n)
    assert not torch.equal(got_b['mem5'], got['mem5'])
    _assert_taps(what, case, got)
    assert PC.exact_mismatches(got, case) == [], what
    c = collections.Counter(names)
    fb, slow = dict(census.fallback_ops), dict(census.slow_paths)
    print(f'[{what}] launches = {dict(c)}\n[{what}] fallback_ops = {fb} slow_paths = {slow}   '
          f'{time.perf_counter() - t0:.2f} s')
    fills = mode == 'bf16x3' and case in FILL_CASES
    _check_launches(names, DEFAULT_LAUNCHES[mode] + ([FILL] if fills else []), [] if fills else [FILL])
    for note in SLOW_NOTES:
        assert note not in slow, f'{what}: {note}'
    if mode == 'bf16x3':    # (empty on the first honest run; 'native' runs its projections as vendor GEMMs by design)
        assert not fb, f'{what}: fallback operators on the device path: {fb}'
    return head, got


@BOTH
@pytest.mark.parametrize('form', ['nchw', 'flat'])
@pytest.mark.parametrize('case', PC.CASES, ids=CASE_IDS)
def test_petr_chained_vs_fp64(monkeypatch, gemm_mode, case, form):
    _chained(monkeypatch, case, gemm_mode, form)


@BOTH
def test_p6_first_then_p2_on_the_same_module(monkeypatch, gemm_mode):
    """p2 run SECOND on one module, after a forward with other img_shapes (same levels, same batch size); both
    forwards against their own references.  A stale mask / positional table / valid ratio / reference grid / scale
    entry fails the second."""
    head, _ = _chained(monkeypatch, PC.P6_FIRST, gemm_mode, 'flat', what='(first forward)')
    _chained(monkeypatch, PC.P2, gemm_mode, 'flat', head=head, what='(second forward, after p6_first)')


@BOTH
@pytest.mark.parametrize('case', PC.CASES, ids=CASE_IDS)
def test_decoder_and_refine_isolated_vs_fp64(monkeypatch, gemm_mode, case):
    """The decoder from the fp64 reference memory cast to fp32, entered through PETRTransformer.forward with
    encode_frames' result substituted; forward_refine from the reference memory and the reference poses."""
    N, B = case.N, case.B
    ref, sel = PC.reference(case), PC.selections(case)
    head = PC.new_head(case).cuda()
    fs, _ = PC.feats(case, 'flat', 'cuda')
    metas = case.metas()
    mem = ref['mem5'].float().cuda().contiguous()                     # [B, S, C]
    with torch.no_grad():
        masks, pos, has_padding = head.make_masks(fs, metas, 1)
        _, mask_flatten, valid_ratios, geom = head.transformer.encode_frames(fs, masks, pos, has_padding)
        keep_mem = mem.clone()
        monkeypatch.setattr(head.transformer, 'encode_frames',
                            lambda *a, **k: (mem, mask_flatten, valid_ratios, geom))
        outs = head(fs, metas, force_topk_proposals=sel['topk_idx'].cuda())
        got = PC.head_taps(case, outs)
        _assert_taps(f'{case} {gemm_mode} decoder from the reference memory', case, got,
                     PC.stage_taps(case, PC.DECODER_STAGES))
        assert torch.equal(mem, keep_mem), 'the decoder wrote into the encoder memory'
        poses = sel['ref_pose'].float().cuda().contiguous()           # [B*N, 2K]
        keep_poses = poses.clone()
        img_inds = torch.arange(B, device='cuda').repeat_interleave(N)
        r_kpts, r_sigmas, r_hs = head.forward_refine(mem.transpose(0, 1), masks, poses, img_inds,
                                                     has_padding=has_padding)
        got = PC.refine_taps(case, r_hs, r_kpts[-1], r_sigmas[-1] if case.vedpose else None)
        _assert_taps(f'{case} {gemm_mode} refine from the reference memory and poses', case, got,
                     PC.stage_taps(case, ('refine',)))
        assert torch.equal(mem, keep_mem) and torch.equal(poses, keep_poses)


@BOTH
@pytest.mark.parametrize('case', PC.CASES, ids=CASE_IDS)
def test_free_run_makes_the_reference_selections(gemm_mode, case):
    """Nothing forced: the proposals of the free run, and the scores of the run that follows the reference's
    proposals, are the fp64 run's selections up to near-ties at the selection boundary."""
    tol_enc, tol_cls, sel = PC.selection_tols(case)
    head = PC.new_head(case).cuda()
    fs, _ = PC.feats(case, 'flat', 'cuda')
    with torch.no_grad():
        _, outs, res = PC.run_head(case, head, fs, free=True)
        assert res['keep'].shape == (case.B, case.N) and bool(torch.isfinite(res['kpts']).all())
        forced = head(fs, case.metas(), force_topk_proposals=sel['topk_idx'].cuda())
    for b in range(case.B):
        _assert_same_selection(outs['enc_cls_scores'][b, :, 0], sel['topk_idx'][b], tol_enc, f'{case} proposals')
        _assert_same_selection(forced['all_cls_scores'][-1][b].sigmoid(), sel['score_topk_idx'][b], tol_cls,
                               f'{case} score top-k')
