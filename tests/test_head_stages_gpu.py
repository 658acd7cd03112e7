"""Everything behind the neck on the DEVICE, tap by tap against fp64: the encoder (after each of its six layers), the
proposal stage, the pose decoder, the head's branches, the joint refine decoder, the result and the OKS-NMS keep set
(cases, references, floors: tests/head_cases.py; what this file stands on: tests/test_head_stages_cpu.py).  The sequel
of tests/test_backbone_gpu.py, whose `gemm_mode` fixture and `_check_launches` it uses.  Needs an MI355X.

Every case runs bbox_head.forward + get_bboxes under no_grad with the fp64 run's proposals and scores forced, reads
all taps after the whole forward, and asserts for every tap

    e_dev = max|got - ref64| / rms(ref64)  <=  8 * e_cpu32,

e_cpu32 being the same metric for the oracle's own fp32 run with the same forced selections (1e-6 .. 4e-5, recorded
in the CPU file).  There is no absolute tolerance.  The ratio of every tap is printed.

Chained: from the features, in both input forms (four NCHW tensors; slices of one token-major buffer, the encoder's
`input_is_shared` path).  Isolated: the decoder from the fp64 reference memory cast to fp32 (the head's `precomputed`),
forward_refine from the reference memory and the reference poses -- encoder error neither excuses nor masks a later
stage.  Every chained case also asserts: the inputs are bit-unchanged; the first call's outputs are bit-unchanged
after a second forward on other features; the keep set is the reference's; the entry points the default path
stands for were launched (recorded through ops._launch); in 'bf16x3' mode with bricks._GEMM['min_rows'] = 1 the
LaunchCensus of the second forward lists no fallback operator.  A free run (nothing forced) must make the fp64 run's
selections up to near-ties (tests/test_model_gpu._assert_same_selection, tolerance 8 x floor x rms of the values).
Case 5 is case 2 as the second forward of a module that first saw other img_shapes.

Largest e_dev / e_cpu32 per stage over all cases, forms and switches, measured on the MI355X (a ratio above 8 is a
finding to explain and fix, not a constant to raise):

    stage (taps)                                   'native'   'bf16x3'   (where: 'native'; 'bf16x3')
    encoder (mem0 .. mem5)                          1.85       1.81   (64x96 T = 7; the padded two-clip batch)
    proposals (enc_cls, init_reference)             2.04       2.25   (75x133 T = 5; padded batch, head-major sampler)
    decoder (hs0 .. hs2, ref0 .. ref2)              1.93       1.66   (64x416; 64x96 T = 7)
    head (cls_last, poses)                          2.15       1.22   (64x416)
    refine (refine_hs0/1, refine_kpts, _sigma)      2.32       1.90   (64x416)
    result (det_kpts, det_kpt_scores, det_bboxes)   2.44       2.44   (64x416; padded batch, head-major sampler)

The isolated stages sit lower (decoder from the reference memory: at most 1.33 / 0.94; refine from the reference memory
and poses: 1.47 / 0.65).  Whether 8 fits these stages: it does, with a factor of three to spare in both modes.
Sensitivity on the device, measured once and not committed: one bias of the device
module x (1 + 1e-3) on case 1 puts hs1 at 50 x the floor (decoder.layers.1.norms.1.bias), mem3 at 36 x and every
later tap at 25 .. 56 x (encoder.layers.3.ffns.0.layers.1.bias), ref0 at 25 x (pre_kpt_branches.0.6.bias), the same in
both modes; unperturbed, the same script gives at most 1.21 ('bf16x3') and 1.92 ('native').

Findings of the first run, fixed with it:
  * bricks.BaseTransformerLayer skipped the LayerNorm after an FFN whenever `inplace_residual` was set, whether or not
    the FFN had been handed that LayerNorm to fuse: off the device (where nothing is fused) every encoder layer lost
    its second norm -- the CPU run of the modules sat at 1e6 x the floor from mem0 on.  The norm is now skipped only
    when the module took it (tests/test_head_stages_cpu.py::test_modules_on_cpu_meet_the_bound).
  * models.videopose_r50_cfg(num_query=Q) did not tell the transformer: it kept two_stage_num_proposals = 300 and
    selected 300 proposals for Q query embeddings (cases 3, 4 and 6, Q = 100, could not run).
No device kernel was found wrong: every tap of every case, form, mode and switch is within 2.5 x the floor.
What this size cannot reach: pave_fill_rows_f32 on an UN-padded 128x160 batch (case 1) -- no level is more than 50 wide,
so no proposal is invalid and nothing is filled; case 6 (a 52-wide level) is the un-padded case that fills rows.
"""
import collections
import time

import pytest
import torch

from tests import head_cases as HC
from tests.test_backbone_gpu import _check_launches, gemm_mode  # noqa: F401  (the fixture is used by name)
from tests.test_model_gpu import _assert_same_selection

pytestmark = pytest.mark.gpu

MARGIN = HC.MARGIN
BOTH = pytest.mark.parametrize('gemm_mode', ['native', 'bf16x3'], indirect=True)
CASE_IDS = [c.name for c in HC.CASES]

TILE = 'pave_enc_deform_attn_tile_f32'
ENCPROJ = 'pave_gemm_bf16x3_encproj_f32'
POSE = 'pave_deform_attn_pose_fused_f32'
GRID = 'pave_deform_attn_grid_fused_f32'
MHA = 'pave_mha_core_f32'
TOPK = 'pave_topk_rows_f32'
GATHER_ADD = 'pave_gather_rows_add_f32'
PROP_REFS = 'pave_proposal_refs_f32'
FILL = 'pave_fill_rows_f32'
REF_FRAMES = 'pave_ref_update_frames_f32'
GATHER_POSES = 'pave_gather_frame_poses_f32'
FINALIZE = 'pave_pose_finalize_f32'
NMS = 'pave_oks_nms_f32'
# what the default path launches in every case.  'native': the projections are vendor GEMMs, so the entries that ARE
# split GEMM forms (the merged encoder projection) or are gated on the split modes (the Linear + LayerNorm proposal
# rows and their filled borders, the grouped per-frame branches with the T-frame reference update, the attention
# core) are not taken
DEFAULT_LAUNCHES = {
    'bf16x3': [TILE, ENCPROJ, POSE, GRID, MHA, TOPK, GATHER_ADD, PROP_REFS, REF_FRAMES, GATHER_POSES, FINALIZE, NMS],
    'native': [TILE, POSE, GRID, TOPK, GATHER_ADD, PROP_REFS, GATHER_POSES, FINALIZE, NMS],
}
# pave_fill_rows_f32 overwrites the rows of invalid proposals and of padded tokens.  Case 1 has neither (no level of
# a 128x160 canvas is more than 50 wide, so every proposal lies inside (0.01, 0.99)) and must not launch it; the padded
# batch of case 2 and the 52-wide level of case 6 must
FILL_CASES = (HC.CASE2, HC.CASE6)


def _assert_taps(what, case, got, names=None):
    names = tuple(names or HC.TAP_NAMES)
    ref, fl = HC.reference(case), HC.floor(case)
    for n in names:
        assert tuple(got[n].shape) == tuple(ref[n].shape), (n, tuple(got[n].shape), tuple(ref[n].shape))
    r = HC.ratios(HC.errors(got, case, names), fl)
    print('\n' + HC.fmt(what, r))
    worst = collections.defaultdict(float)
    for n, v in r.items():
        worst[HC.STAGE[n]] = max(worst[HC.STAGE[n]], v)
    print(f'[{what}] worst per stage: ' + ' '.join(f'{s}={v:.2f}' for s, v in worst.items()))
    for n, v in r.items():
        assert v <= MARGIN, f'{what}: {n}: e_dev = {v:.2f} x e_cpu32 ({v * fl[n]:.3e})'
    return r


def _set(head, switches):
    for k, v in (switches or {}).items():
        assert hasattr(head.transformer, k), k
        setattr(head.transformer, k, v)


def _chained(monkeypatch, case, mode, form, head=None, switches=None, present=(), absent=(), assert_census=True,
             what=''):
    """Two forwards of the head: the case's features under the launch recorder (taps, inputs, entry points), other
    features under the census (fallback operators; the first call's outputs must survive it)."""
    from pavenet_amd.census import LaunchCensus
    t0 = time.perf_counter()
    what = f'{case} {form} {mode} {what}'.strip()
    if head is None:
        head = HC.new_head(case)
        _set(head, switches)
        head = head.cuda()
    fs, keep_in = HC.feats(case, form, 'cuda')
    before = [t.clone() for t in keep_in]
    with torch.no_grad(), HC.record_launches(monkeypatch) as names:
        got, outs, res = HC.run_head(case, head, fs)
    torch.cuda.synchronize()
    first = {n: got[n].clone() for n in HC.TAP_NAMES}
    fs_b, _ = HC.feats(case, form, 'cuda', which='other')
    with torch.no_grad(), LaunchCensus() as census:
        got_b, _, _ = HC.run_head(case, head, fs_b)
    torch.cuda.synchronize()
    for t, k in zip(keep_in, before):
        assert torch.equal(t, k), f'{what}: the forward wrote into its input'
    for n in HC.TAP_NAMES:
        assert torch.equal(got[n], first[n]), f'{what}: {n} of the first call changed during the second forward'
        assert bool(torch.isfinite(got_b[n]).all()), (what, n)
    assert not torch.equal(got_b['mem5'], got['mem5'])
    _assert_taps(what, case, got)
    assert got['keep'] == HC.reference(case)['keep'], f'{what}: keep set {got["keep"]}'
    c = collections.Counter(names)
    fb = dict(census.fallback_ops)
    print(f'[{what}] launches = {dict(c)}\n[{what}] fallback_ops = {fb} slow_paths = {dict(census.slow_paths)}   '
          f'{time.perf_counter() - t0:.2f} s')
    _check_launches(names, present, absent)
    if mode == 'bf16x3' and assert_census:
        assert not fb, f'{what}: fallback operators on the device path: {fb}'
    return head, got, outs, names


@BOTH
@pytest.mark.parametrize('form', ['nchw', 'flat'])
@pytest.mark.parametrize('case', HC.CASES, ids=CASE_IDS)
def test_head_chained_vs_fp64(monkeypatch, gemm_mode, case, form):
    fills = gemm_mode == 'bf16x3' and case in FILL_CASES
    _chained(monkeypatch, case, gemm_mode, form, present=DEFAULT_LAUNCHES[gemm_mode] + ([FILL] if fills else []),
             absent=[] if fills else [FILL])


@BOTH
def test_case5_second_forward_on_the_same_module(monkeypatch, gemm_mode):
    """Case 2 run SECOND on one module, after a forward with other img_shapes (same levels, same batch size); both
    forwards against their own references.  A stale flat_pos / refs_padded / proposals_padded / proposal_fill /
    refine_padded / vr_rows entry fails the second."""
    head, _, _, _ = _chained(monkeypatch, HC.CASE5_FIRST, gemm_mode, 'flat', what='(case 5, first forward)')
    _chained(monkeypatch, HC.CASE2, gemm_mode, 'flat', head=head, what='(case 5, second forward)')


@BOTH
@pytest.mark.parametrize('case', HC.CASES, ids=CASE_IDS)
def test_decoder_and_refine_isolated_vs_fp64(gemm_mode, case):
    """The decoder from the fp64 reference memory cast to fp32 (the head's `precomputed`), forward_refine from the
    reference memory and the reference poses."""
    T, N, B = case.T, case.N, case.B
    ref, sel = HC.reference(case), HC.selections(case)
    head = HC.new_head(case).cuda()
    fs, _ = HC.feats(case, 'flat', 'cuda')
    metas = case.metas()
    mem = ref['mem5'].float().cuda().contiguous()                     # [B*T, S, C]
    with torch.no_grad():
        masks, pos, has_padding = head.make_masks(fs, metas)
        _, mask_flatten, valid_ratios, geom = head.transformer.encode_frames(fs, masks, pos, has_padding)
        keep_mem = mem.clone()
        outs = head(fs, metas, precomputed=(masks, pos, has_padding, (mem, mask_flatten, valid_ratios, geom)),
                    force_topk_proposals=sel['topk_idx'].cuda())
        got = HC.head_taps(case, outs)
        _assert_taps(f'{case} {gemm_mode} decoder from the reference memory', case, got, HC.DECODER_TAPS)
        assert torch.equal(mem, keep_mem), 'the decoder wrote into the encoder memory'
        poses = sel['ref_pose'].float().cuda().contiguous()           # [T, B*N, 2K]
        keep_poses = poses.clone()
        img_inds = torch.arange(B, device='cuda').repeat_interleave(N)
        r_kpts, _, r_sigmas, r_hs = head.forward_refine(mem.transpose(0, 1), masks, poses, img_inds,
                                                        has_padding=has_padding, last_level_only=False)
        got = HC.refine_taps(case, r_hs, r_kpts[-1], r_sigmas[-1])
        _assert_taps(f'{case} {gemm_mode} refine from the reference memory and poses', case, got,
                     [n for n in HC.REFINE_TAPS if HC.STAGE[n] == 'refine'])
        assert torch.equal(mem, keep_mem) and torch.equal(poses, keep_poses)


@BOTH
@pytest.mark.parametrize('case', HC.CASES, ids=CASE_IDS)
def test_free_run_makes_the_reference_selections(gemm_mode, case):
    """Nothing forced: the proposals of the free run, and the scores of the run that follows the reference's
    proposals, are the fp64 run's selections up to near-ties at the selection boundary."""
    tol_enc, tol_cls, sel = HC.selection_tols(case)
    head = HC.new_head(case).cuda()
    fs, _ = HC.feats(case, 'flat', 'cuda')
    with torch.no_grad():
        _, outs, res = HC.run_head(case, head, fs, free=True)
        assert res['keep'].shape == (case.B, case.N) and bool(torch.isfinite(res['kpts']).all())
        forced = head(fs, case.metas(), force_topk_proposals=sel['topk_idx'].cuda())
    for b in range(case.B):
        _assert_same_selection(outs['enc_cls_scores'][b, :, 0], sel['topk_idx'][b], tol_enc, f'{case} proposals')
        _assert_same_selection(forced['all_cls_scores'][-1][b].sigmoid(), sel['score_topk_idx'][b], tol_cls,
                               f'{case} score top-k')


# ---- switches -----------------------------------------------------------------------------------------------------
SWITCH_CASES = pytest.mark.parametrize('case', [HC.CASE1, HC.CASE2], ids=CASE_IDS[:2])


@BOTH
@SWITCH_CASES
@pytest.mark.parametrize('xcd', [True, False], ids=['xcd_unit_order', 'natural_order'])
def test_encoder_head_major_sampler(monkeypatch, gemm_mode, case, xcd):
    """enc_lds_tile = False: the direct-gather kernel samples the encoder (with and without the XCD unit order); no
    LDS-tile launch and no merged projection + sampling-table GEMM."""
    _, _, _, names = _chained(monkeypatch, case, gemm_mode, 'flat',
                              switches=dict(enc_lds_tile=False, xcd_unit_order=xcd), present=[GRID],
                              absent=[TILE, ENCPROJ], assert_census=False, what=f'enc_lds_tile=False xcd={xcd}')
    # six encoder layers + two refine layers on the grid kernel
    assert collections.Counter(names)[GRID] == HC.N_ENC + HC.N_REF


@BOTH
@SWITCH_CASES
def test_unfused_proposal_stage(monkeypatch, gemm_mode, case):
    """fused_proposal_stage = False: the tensor expressions of the proposal stage."""
    _chained(monkeypatch, case, gemm_mode, 'flat', switches=dict(fused_proposal_stage=False),
             present=[TOPK], absent=[GATHER_ADD, PROP_REFS], assert_census=False, what='fused_proposal_stage=False')


@BOTH
@SWITCH_CASES
def test_value_projections_per_layer(monkeypatch, gemm_mode, case):
    """hoist_value_proj = False: every T-frame attention projects its own values; on: both decoders hand their
    layers' projections to project_values_hoisted."""
    from pavenet_amd import transformer as TR
    calls = []
    real = TR.project_values_hoisted

    def spy(*a, **k):
        calls.append(len(a[0]))
        return real(*a, **k)
    monkeypatch.setattr(TR, 'project_values_hoisted', spy)
    _chained(monkeypatch, case, gemm_mode, 'flat', switches=dict(hoist_value_proj=False), assert_census=False,
             what='hoist_value_proj=False')
    assert calls == []
    _chained(monkeypatch, case, gemm_mode, 'flat', what='hoist_value_proj=True')
    assert calls == [HC.N_DEC, HC.N_REF] * 2       # (two forwards: decoder, refine decoder)
