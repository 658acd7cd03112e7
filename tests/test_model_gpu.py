"""Product modules / whole model (HIP path) vs the reference's golden vectors and the oracle.
Needs an MI355X."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import pavenet_ref as R
from oracle.seeded import seeded_array, seeded_state_dict

pytestmark = pytest.mark.gpu

# Tests that pick their own GEMM mode (or run the model in a child process) are not doubled.
_OWN_MODE = ('test_split_gemm_mode_matches_native', 'test_fp16_projection_mode_within_half_pixel',
             'test_forward_is_the_same_from_the_first_call_and_reads_no_stale_memory',
             'test_frame_sharded_two_ranks', 'test_t15_frame_sharded_vs_oracle',
             'test_frame_sharded_center_frame_on_a_single_frame_rank_vs_oracle',
             'test_bench_multi_rank_code_path_on_one_gpu', 'test_split_caches_follow_reloaded_weights',
             'test_derived_operand_caches_follow_reloaded_weights',
             'test_oks_nms_kernel_vs_oracle', 'test_oks_nms_kernel_survives_nan_and_inf',
             'test_deterministic_mode_is_bit_reproducible_and_matches_default',
             'test_hipgraph_replay_equals_eager', 'test_tail_hipgraph_replay_equals_eager',
             'test_bench_batch_full_size_t7_b4_vs_oracle',
             'test_hrnet_w48_full_size_t7_vs_oracle', 'test_t15_full_size_unsharded_vs_oracle',
             'test_t15_full_size_fp16_vs_oracle', 'test_padded_batch_full_size_vs_oracle',
             'test_posetrack_canvas_750x1333_full_size_vs_oracle', 'test_no_fallback_ops_on_the_baseline_workloads',
             'test_neck_eval_with_grad_keeps_the_differentiable_path')


@pytest.fixture(autouse=True, params=['native', 'bf16x3'])
def gemm_mode(request):
    """Every golden / oracle comparison of this module runs twice at UNCHANGED tolerances: with
    the projections / FFN / 1x1 and 3x3 convolutions on the vendor fp32 MFMA kernels ('native')
    and on the hand-written exact 3-term bf16 split kernels ('bf16x3', the mode bench.py's
    headline runs in; judge's ruling of round 1)."""
    from pavenet_amd import bricks
    mode = request.param
    if request.node.originalname in _OWN_MODE:
        if mode != 'native':
            pytest.skip('sets its own GEMM mode')
        bricks.set_gemm_mode('native')     # these tests start from the vendor-kernel mode
        yield mode
        bricks.set_gemm_mode('native')
        return
    old_rows = bricks._GEMM['min_rows']
    bricks.set_gemm_mode(mode)
    if mode != 'native':
        bricks._GEMM['min_rows'] = 1   # take the hand-written kernels at test sizes too
    made = bricks._SPLIT_STATS['made']
    _STRICT[0] = mode == 'bf16x3'
    try:
        yield mode
    finally:
        _STRICT[0] = False
        bricks.set_gemm_mode('native')
        bricks._GEMM['min_rows'] = old_rows
    if mode != 'native' and request.node.originalname not in ('test_oks_nms_kernel_vs_oracle',):
        assert bricks._SPLIT_STATS['made'] > made or made > 0, 'split kernels were not exercised'


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


_STRICT = [False]   # set by the gemm_mode fixture: True in the bit-reproducible 'bf16x3' mode


def _close(actual, desired, rtol=1e-7, atol=0.0):
    """np.testing.assert_allclose with the tolerances of the mode under test.  'native' (vendor
    fp32 kernels, not run-to-run deterministic): the values written at the call.  'bf16x3' (the
    headline mode; bit-reproducible forward, tools/soak.py): pixel quantities (written atol = 1e-2
    px: det_kpts / det_bboxes) are asserted at BASELINE.md section 4's goal of 1e-3 px, and the
    encoder-memory / decoder-state comparisons (written rtol = 2e-3) at half their tolerances.
    PAVE_TOL_REPORT=<file>: append the worst |err| / tolerance ratio of every comparison."""
    if _STRICT[0]:
        if atol == 1e-2:
            atol = 1e-3
        elif rtol == 2e-3:
            rtol, atol = 1e-3, atol / 2
    a, d = np.asarray(actual, dtype=np.float64), np.asarray(desired, dtype=np.float64)
    rep = os.environ.get('PAVE_TOL_REPORT')
    if rep and a.shape == d.shape and a.size:
        import inspect
        err = np.abs(a - d)
        ratio = float(np.nanmax(err / (atol + rtol * np.abs(d))))
        fr = inspect.stack()[1]
        with open(rep, 'a') as f:
            f.write(f'{fr.function}:{fr.lineno} strict={_STRICT[0]} rtol={rtol:g} atol={atol:g} '
                    f'max_abs_err={float(np.nanmax(err)):.3e} worst_ratio={ratio:.3f}\n')
    np.testing.assert_allclose(actual, desired, rtol=rtol, atol=atol)


def _g(golden_dir, name):
    return np.load(os.path.join(golden_dir, name + '.npz'))


def _seed(module, g=None):
    shapes = json.loads(str(g['keys'])) if g is not None else \
        {k: list(v.shape) for k, v in module.state_dict().items()}
    module.load_state_dict(seeded_state_dict(shapes, like=module.state_dict()), strict=True)
    return module


def _lsi(shapes):
    return torch.cat((shapes.new_zeros((1,)), shapes.prod(1).cumsum(0)[:-1]))


def test_encoder_msda_module(golden_dir):
    from pavenet_amd.deform_attn import MultiScaleDeformableAttention
    g = _g(golden_dir, 'mod_enc_msda')
    m = _seed(MultiScaleDeformableAttention(embed_dims=256), g).cuda().eval()
    shapes = _t(g['levels']).cuda()
    with torch.no_grad():
        out = m(_t(g['query']).cuda(), None, None, query_pos=_t(g['pos']).cuda(),
                key_padding_mask=_t(g['mask']).cuda(), reference_points=_t(g['ref']).cuda(),
                spatial_shapes=shapes, level_start_index=_lsi(shapes))
    _close(out.cpu().numpy(), g['out'], rtol=1e-4, atol=5e-5)


def test_encoder_msda_shared_pos_merged_projection_vs_oracle(gemm_mode):
    """Un-padded frame batch: the positional table is one [S, C] tensor expanded over the frames,
    and (in the split GEMM modes) value_proj + offsets + logits run as ONE N = 640 launch with the
    pos term folded into a per-token epilogue table.  Against the oracle's un-fused module."""
    from pavenet_amd import bricks
    from pavenet_amd.deform_attn import MultiScaleDeformableAttention
    from pavenet_amd.transformer import VideoPoseTransformerMulFrames as VT
    hw = [(24, 40), (12, 20), (6, 10), (3, 5)]
    S, bs = sum(h * w for h, w in hw), 3
    m = _seed(MultiScaleDeformableAttention(embed_dims=256)).eval()
    sd = {'a.' + k: v for k, v in m.state_dict().items()}
    g = torch.Generator().manual_seed(5)
    query = torch.randn(S, bs, 256, generator=g)
    pos = torch.randn(S, 1, 256, generator=g).expand(S, bs, 256)
    shapes = torch.as_tensor(hw, dtype=torch.long)
    vr = torch.ones(bs, 4, 2)
    ref = VT.get_reference_points(hw, vr, device='cpu')
    with torch.no_grad():
        exp = R.msda_module(sd, 'a', query, pos, None, ref, shapes, _lsi(shapes))
        md = m.cuda()
        qd = query.transpose(0, 1).contiguous().cuda().transpose(0, 1)    # seq-first view
        posd = pos[:, :1].cuda().expand(S, bs, 256)
        made = bricks._SPLIT_STATS['made']
        out = md(qd, None, None, query_pos=posd, key_padding_mask=None,
                 reference_points=ref.cuda(), spatial_shapes=shapes.cuda(),
                 level_start_index=_lsi(shapes).cuda(), tile_levels=hw)
    if gemm_mode != 'native':
        assert hasattr(md, '_merged_w') and bricks._SPLIT_STATS['made'] > made   # merged path ran
    _close(out.cpu().numpy(), exp.numpy(), rtol=1e-4, atol=5e-5)


def test_pose_single_module(golden_dir):
    from pavenet_amd.deform_attn import MultiScaleDeformablePoseAttention
    g = _g(golden_dir, 'mod_pose_single')
    m = _seed(MultiScaleDeformablePoseAttention(embed_dims=256, num_points=17), g).cuda().eval()
    shapes = _t(g['levels']).cuda()
    with torch.no_grad():
        out = m(_t(g['query']).cuda(), None, _t(g['value']).cuda(), query_pos=_t(g['pos']).cuda(),
                key_padding_mask=_t(g['mask']).cuda(), reference_points=_t(g['ref']).cuda(),
                spatial_shapes=shapes, level_start_index=_lsi(shapes))
    _close(out.cpu().numpy(), g['out'], rtol=1e-4, atol=5e-5)


@pytest.mark.parametrize('T', [3, 5])
def test_pose_mulframes_module(golden_dir, T):
    from pavenet_amd import models  # noqa: F401
    from pavenet_amd.registry import build_attention
    g = _g(golden_dir, f'mod_pose_t{T}')
    kw = dict(num_frames=3) if T == 3 else {}
    m = build_attention(dict(type=f'opera.MulFramesMultiScaleDeformablePoseAttentionNumFrames{T}',
                             embed_dims=256, num_points=15, **kw))
    m = _seed(m, g).cuda().eval()
    shapes = _t(g['levels']).cuda()
    with torch.no_grad():
        out = m(_t(g['query']).cuda(), None, _t(g['value']).cuda(), query_pos=_t(g['pos']).cuda(),
                key_padding_mask=_t(g['mask']).cuda(), reference_points=_t(g['ref']).cuda(),
                spatial_shapes=shapes, level_start_index=_lsi(shapes))
    _close(out.cpu().numpy(), g['out'], rtol=1e-4, atol=5e-5)


@pytest.mark.parametrize('T', [3, 5])
@pytest.mark.parametrize('convention', ['replicated', 'expanded', 'native'])
def test_joint_mulframes_module(golden_dir, T, convention):
    """The reference's replicated-memory call, a stride-0 expand of it, and the native
    un-replicated call must all give the reference's numbers."""
    from pavenet_amd import models  # noqa: F401
    from pavenet_amd.registry import build_attention
    g = _g(golden_dir, f'mod_joint_t{T}')
    kw = dict(num_frames=3) if T == 3 else {}
    m = build_attention(dict(type=f'mmcv.MulFramesMultiScaleDeformableAttentionNumFrames{T}',
                             embed_dims=256, im2col_step=128, **kw))
    m = _seed(m, g).cuda().eval()
    shapes = _t(g['levels']).cuda()
    N = g['query'].shape[1]
    mem = _t(g['memory']).cuda()              # [S, 1, T, C]
    mask1 = _t(g['mask']).cuda()              # [T, S]
    extra = {}
    if convention == 'replicated':
        value, mask = mem[:, [0] * N].contiguous(), mask1[None].expand(N, -1, -1).contiguous()
    elif convention == 'expanded':
        value, mask = mem.expand(-1, N, -1, -1), mask1[None].expand(N, -1, -1)
    else:
        value, mask = mem, mask1[None]
        extra['memory_clip_index'] = torch.zeros(N, dtype=torch.long, device='cuda')
    with torch.no_grad():
        out = m(_t(g['query']).cuda(), None, value, query_pos=_t(g['pos']).cuda(),
                key_padding_mask=mask, reference_points=_t(g['ref']).cuda(),
                spatial_shapes=shapes, level_start_index=_lsi(shapes), **extra)
    _close(out.cpu().numpy(), g['out'], rtol=1e-4, atol=5e-5)


def _assert_same_selection(values, ref_idx, tol, what):
    """The reference's top-k selection `ref_idx` is a valid top-k of OUR `values` up to near-ties:
    every member the reference picked is within `tol` of our k-th largest value, and every member
    of OUR top-k that the reference did not pick is within `tol` of it too -- a member may differ
    only when it sits on the selection boundary (under random weights the 300-of-S proposal
    logits and the N-of-300 scores have near-ties there); there is no allowance for
    members that are clearly inside or outside.  A wrong logit fails this by orders of magnitude."""
    values = values.flatten().float().cpu()
    ref_idx = torch.as_tensor(np.asarray(ref_idx)).flatten().long()
    top_v, top_i = values.topk(ref_idx.numel())
    kth = top_v[-1]
    worst = values[ref_idx].min()
    assert worst >= kth - tol, f'{what}: reference-selected member {float(worst)} vs k-th {float(kth)}'
    ref_set = set(ref_idx.tolist())
    for v, i in zip(top_v.tolist(), top_i.tolist()):
        if i not in ref_set:
            assert v <= float(kth) + tol, \
                f'{what}: our member {i} ({v}) is not in the reference selection and not a near-tie ' \
                f'of the k-th value {float(kth)}'


def _build(T, max_per_img, g=None):
    from pavenet_amd.models import build_model, videopose_r50_cfg
    m = build_model(videopose_r50_cfg(num_frames=T, max_per_img=max_per_img))
    return _seed(m, g).cuda().eval()


@pytest.mark.parametrize('T', [3, 5])
def test_end_to_end_vs_reference_golden(golden_dir, T):
    """Whole simple_test (backbone .. OKS-NMS) at 128x160 with name-seeded weights against
    the reference's own outputs.  Tolerance: keypoints within 1e-2 px."""
    g = _g(golden_dir, f'e2e_videopose_r50_t{T}')
    N = int(g['score_topk'].shape[0])
    m = _build(T, N, g)
    img = _t(g['img']).cuda()
    hs_, ws_ = int(g['img_shape'][0]), int(g['img_shape'][1])
    metas = [dict(batch_input_shape=(128, 160), img_shape=(hs_, ws_, 3),
                  scale_factor=(1., 1., 1., 1.))]
    with torch.no_grad():
        feat = m.extract_feat(img)
        outs = m.bbox_head(feat, metas)
        memory = outs['memory'].permute(1, 0, 2)  # [B*T, S, C]
        if 'memory' in g.files:
            _close(memory.cpu().numpy(), g['memory'], rtol=2e-3, atol=5e-4)
        else:
            _close(memory[T // 2::T].cpu().numpy(), g['memory_center'],
                                       rtol=2e-3, atol=5e-4)
        _assert_same_selection(outs['enc_cls_scores'][0, :, 0], g['enc_topk'], 1e-4, 'proposals')
        # follow the reference's exact proposal order for the value-level comparison
        outs = m.bbox_head(feat, metas, force_topk_proposals=_t(g['enc_topk']).cuda())
        _close(outs['hs'].permute(0, 2, 1, 3).cpu().numpy(), g['hs'],
                                   rtol=2e-3, atol=1e-3)
        _close(outs['inter_references'].cpu().numpy(),
                                   g['inter_references'], rtol=1e-3, atol=2e-4)
        _close(outs['all_cls_scores'][-1].cpu().numpy(), g['cls_last'],
                                   rtol=1e-3, atol=1e-3)
        _assert_same_selection(outs['all_cls_scores'][-1][0].sigmoid(), g['score_topk'], 1e-5,
                               'score top-k')
        res = m.bbox_head.get_bboxes(outs, metas, rescale=False,
                                     force_score_topk=_t(g['score_topk'])[None].cuda())
        assert res['order'][0].tolist() == list(range(N))
        (bboxes, labels, kpts), = m.bbox_head.results_to_list(res)
    assert kpts.shape == g['det_kpts'].shape, 'OKS-NMS keep set differs from the reference'
    _close(kpts.cpu().numpy(), g['det_kpts'], rtol=1e-4, atol=1e-2)
    _close(bboxes.cpu().numpy(), g['det_bboxes'], rtol=1e-4, atol=1e-2)
    assert labels.cpu().tolist() == g['det_labels'].tolist()


@pytest.mark.parametrize('T,B', [(7, 1), (3, 2), (7, 4), (15, 1)])
def test_end_to_end_vs_oracle(T, B):
    """T = 7 has no reference implementation (the reference hard-codes 3 / 5): the oracle's
    generalised restatement defines it.  B = 2 checks the batched-clip path against two
    independent single-clip oracle runs (the reference asserts B = 1)."""
    N = 12
    m = _build(T, N)
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    H, W = 128, 160  # S = 426 tokens >= 300 queries
    img = _t(seeded_array(f'e2e.oracle.{T}.{B}', (B, T, 3, H, W)))
    metas = [dict(batch_input_shape=(H, W), img_shape=(H, W, 3), scale_factor=(1., 1., 1., 1.))
             for _ in range(B)]
    cfg = dict(num_frames=T, num_keypoints=15, num_query=300, max_per_img=N)
    exp, taps = [], []
    for b in range(B):
        taps.append({})
        with torch.no_grad():
            exp.append(R.videopose_simple_test(sd, cfg, img[b:b + 1], taps=taps[b]))
    prop = torch.cat([t['topk_idx'] for t in taps], 0)
    score = torch.stack([t['score_topk_idx'].view(-1) for t in taps], 0)
    with torch.no_grad():
        m.forward_device(img.cuda(), metas)  # free run: our selection == the oracle's up to ties
        for b in range(B):
            _assert_same_selection(m.bbox_head.transformer.last_enc_cls[b, :, 0], prop[b], 1e-4,
                                   'proposals')
        res = m.forward_device(img.cuda(), metas, force_topk_proposals=prop.cuda(),
                               force_score_topk=score.cuda())
        got = m.bbox_head.results_to_list(res)
    for b in range(B):
        eb, el, ek = exp[b]
        gb, gl, gk = got[b]
        assert gk.shape == ek.shape
        _close(gk.cpu().numpy(), ek.numpy(), rtol=1e-4, atol=1e-2)
        _close(gb.cpu().numpy(), eb.numpy(), rtol=1e-4, atol=1e-2)


def test_oks_nms_kernel_survives_nan_and_inf():
    """Non-finite scores / keypoints (e.g. an fp16-operand mode overflowing on un-normalised
    weights) must still give a valid permutation and no out-of-range access."""
    from pavenet_amd.ops import oks_nms
    g = torch.Generator().manual_seed(3)
    kp = torch.rand(2, 30, 15, 3, generator=g) * 100
    sc = torch.rand(2, 30, generator=g)
    sc[0, ::3] = float('nan')
    sc[1, 5] = float('inf')
    kp[0, 4] = float('nan')
    kp[1, 7, :, 0] = float('inf')
    keep, order = oks_nms(kp.cuda(), sc.cuda(), _t(R.OKS_SIGMAS_15).cuda(), 0.45)
    torch.cuda.synchronize()
    for b in range(2):
        assert sorted(order[b].cpu().tolist()) == list(range(30))
    assert set(order[0, :10].cpu().tolist()) == set(range(0, 30, 3))   # NaNs first, as numpy [::-1]


def test_oks_nms_kernel_vs_oracle():
    from pavenet_amd.ops import oks_nms
    rng = np.random.default_rng(0)
    B, N, K = 3, 40, 15
    base = rng.uniform(0, 200, size=(B, 8, K, 2)).astype(np.float32)
    # clusters of near-duplicates so that suppression actually happens
    kp = base[:, rng.integers(0, 8, size=N)] + rng.normal(0, 3, size=(B, N, K, 2)).astype(np.float32)
    sc = np.sort(rng.uniform(0.05, 1, size=(B, N)).astype(np.float32), axis=1)[:, ::-1].copy()
    kpts = np.concatenate([kp, np.ones((B, N, K, 1), np.float32)], -1)
    sig = R.OKS_SIGMAS_15
    keep, order = oks_nms(_t(kpts).cuda(), _t(sc).cuda(), _t(sig).cuda(), 0.45)
    for b in range(B):
        exp = R.oks_nms(_t(kpts[b]), _t(sc[b]), 0.45, sig)
        assert sorted(np.nonzero(keep[b].cpu().numpy())[0].tolist()) == sorted(int(i) for i in exp)
        assert order[b].cpu().tolist() == list(range(N))
    assert 0 < int(keep.sum()) < B * N


def _run_sharded_worker(args, nproc=2):
    import socket
    import subprocess
    import sys
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', f'--nproc-per-node={nproc}',
           '--master-addr', '127.0.0.1', '--master-port', str(port),
           os.path.join(root, 'tests', 'sharded_worker.py')] + [str(a) for a in args]
    torch.cuda.empty_cache()  # the workers share this process's GPU
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)   # one run, no retry
    assert r.returncode == 0, (r.stdout[-1500:] + '\n---\n' + r.stderr[-6000:])
    return r.stdout


@pytest.mark.parametrize('T', [3, 5])
def test_frame_sharded_two_ranks(T):
    """Frame-sharded path (SURVEY 8e ii) with REAL collectives: two processes on this box's one
    GPU, frames t % 2 == rank each, partial-softmax rows merged by all-gather; must equal the
    un-sharded model."""
    assert 'sharded == unsharded: True' in _run_sharded_worker([T])


@pytest.mark.parametrize('gemm,tol_px,nproc', [('native', 1e-2, 2), ('fp16', 0.5, 2),
                                               ('fp16', 0.5, 4)])
def test_t15_frame_sharded_vs_oracle(gemm, tol_px, nproc):
    """BASELINE configs[4]: R-50, T = 15 long clip, frames sharded over ranks (t % G), partial
    softmax rows merged by all-gather, projections in fp32 or with fp16 MFMA operands -- against
    the ORACLE's un-sharded fp32 run (fp32: 1e-2 px; fp16 projections: 0.5 px)."""
    assert 'sharded == oracle: True' in _run_sharded_worker([15, gemm, tol_px], nproc)


def test_frame_sharded_center_frame_on_a_single_frame_rank_vs_oracle():
    """The shape of the driver's 8-GPU run of BASELINE configs[4] (T = 15 over 8 ranks: 2, ..., 2, 1 frames, the
    centre frame on the LAST rank, the only one that owns a single frame) at the largest world the box's
    process guard allows on one GPU (6 processes with the device open: this one, the launcher and 4 ranks):
    T = 7 over 4 ranks = 2, 2, 2, 1 frames, centre frame 3 on rank 3 -- proposals broadcast from the
    single-frame rank, five all-gather merges -- against the oracle's un-sharded run (the world-size-8
    collectives themselves run on gloo / CPU in tests/test_dist_cpu.py)."""
    assert 'sharded == oracle: True' in _run_sharded_worker([7, 'native', 1e-2], 4)


@pytest.mark.parametrize('name,K,head', [('e2e_petr_r50', 17, 'opera.PETRHead'),
                                         ('e2e_vedpose_r50', 15, 'opera.VedPoseHeadV2')])
def test_petr_end_to_end_vs_reference_golden(golden_dir, name, K, head):
    """BASELINE configs[0] (single-image PETR R-50) and the configs/vedpose single-frame head
    against the reference's own outputs."""
    from pavenet_amd.models import build_model, petr_r50_cfg
    g = _g(golden_dir, name)
    N = int(g['score_topk'].shape[0])
    m = _seed(build_model(petr_r50_cfg(num_keypoints=K, max_per_img=N, head=head)), g).cuda().eval()
    hs_, ws_ = int(g['img_shape'][0]), int(g['img_shape'][1])
    metas = [dict(batch_input_shape=(128, 160), img_shape=(hs_, ws_, 3),
                  scale_factor=(1., 1., 1., 1.))]
    with torch.no_grad():
        feat = m.extract_feat(_t(g['img']).cuda())
        outs = m.bbox_head(feat, metas)
        _close(outs['memory'].permute(1, 0, 2).cpu().numpy(), g['memory'],
                                   rtol=2e-3, atol=5e-4)
        _assert_same_selection(outs['enc_cls_scores'][0, :, 0], g['enc_topk'], 1e-4, 'proposals')
        outs = m.bbox_head(feat, metas, force_topk_proposals=_t(g['enc_topk']).cuda())
        _close(outs['hs'].permute(0, 2, 1, 3).cpu().numpy(), g['hs'],
                                   rtol=2e-3, atol=1e-3)
        _close(outs['inter_references'].cpu().numpy(), g['inter_references'],
                                   rtol=1e-3, atol=2e-4)
        _assert_same_selection(outs['all_cls_scores'][-1][0].sigmoid(), g['score_topk'], 1e-5,
                               'score top-k')
        res = m.bbox_head.get_bboxes(outs, metas,
                                     force_score_topk=_t(g['score_topk'])[None].cuda())
        (bboxes, labels, kpts), = m.bbox_head.results_to_list(res)
    _close(kpts.cpu().numpy(), g['det_kpts'], rtol=1e-4, atol=1e-2)
    _close(bboxes.cpu().numpy(), g['det_bboxes'], rtol=1e-4, atol=1e-2)


def test_petr_batched_vs_oracle():
    from pavenet_amd.models import build_model, petr_r50_cfg
    m = _seed(build_model(petr_r50_cfg(num_keypoints=17, max_per_img=10))).cuda().eval()
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    img = _t(seeded_array('petr.batched', (2, 3, 128, 160)))
    metas = [dict(batch_input_shape=(128, 160), img_shape=(128, 160, 3),
                  scale_factor=(1., 1., 1., 1.)) for _ in range(2)]
    exp, taps = [], [{}, {}]
    for b in range(2):
        with torch.no_grad():
            exp.append(R.petr_simple_test(sd, dict(num_keypoints=17, num_query=300, max_per_img=10),
                                          img[b:b + 1], taps=taps[b]))
    prop = torch.cat([t['topk_idx'] for t in taps], 0)
    score = torch.stack([t['score_topk_idx'].view(-1) for t in taps], 0)
    m.forward_device(img.cuda(), metas)  # free run: same selection as the oracle up to ties
    for b in range(2):
        _assert_same_selection(m.bbox_head.transformer.last_enc_cls[b, :, 0], prop[b], 1e-4,
                               'proposals')
    got = m.bbox_head.results_to_list(m.forward_device(
        img.cuda(), metas, force_topk_proposals=prop.cuda(), force_score_topk=score.cuda()))
    for b in range(2):
        _close(got[b][2].cpu().numpy(), exp[b][2].numpy(), rtol=1e-4, atol=1e-2)


def test_petr_hrnet_w48_vs_reference_golden(golden_dir):
    """HRNet-w48 backbone (BASELINE configs[3]) under the PETR head against the reference."""
    from pavenet_amd.models import build_model, petr_r50_cfg, with_hrnet_w48
    g = _g(golden_dir, 'e2e_petr_hrnetw48')
    N = int(g['score_topk'].shape[0])
    m = build_model(with_hrnet_w48(petr_r50_cfg(num_keypoints=17, max_per_img=N)))
    m = _seed(m, g).cuda().eval()
    metas = [dict(batch_input_shape=(128, 160), img_shape=(120, 150, 3),
                  scale_factor=(1., 1., 1., 1.))]
    with torch.no_grad():
        feat = m.extract_feat(_t(g['img']).cuda())
        outs = m.bbox_head(feat, metas)
        _close(outs['memory'].permute(1, 0, 2).cpu().numpy(), g['memory'],
                                   rtol=2e-3, atol=5e-4)
        _assert_same_selection(outs['enc_cls_scores'][0, :, 0], g['enc_topk'], 1e-4, 'proposals')
        outs = m.bbox_head(feat, metas, force_topk_proposals=_t(g['enc_topk']).cuda())
        _assert_same_selection(outs['all_cls_scores'][-1][0].sigmoid(), g['score_topk'], 1e-5,
                               'score top-k')
        res = m.bbox_head.get_bboxes(outs, metas,
                                     force_score_topk=_t(g['score_topk'])[None].cuda())
        (bboxes, labels, kpts), = m.bbox_head.results_to_list(res)
    _close(kpts.cpu().numpy(), g['det_kpts'], rtol=1e-4, atol=1e-2)


@pytest.mark.parametrize('B', [1, 2])
def test_videopose_hrnet_w48_t7_vs_oracle(B):
    """BASELINE configs[3]: HRNet-w48 + MulFrames head, T = 7, 300 pose queries.  No reference
    config composes these two, so the oracle does: its HRNet is pinned by the reference's
    HRNet-w48 PETR golden (tests/test_oracle_golden.py), its T-frame head by the T = 3 / 5 goldens."""
    from pavenet_amd.models import build_model, videopose_r50_cfg, with_hrnet_w48
    T, N = 7, 10
    m = _seed(build_model(with_hrnet_w48(videopose_r50_cfg(num_frames=T, max_per_img=N))))
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    m = m.cuda().eval()
    img = _t(seeded_array(f'hrnet.t7.{B}', (B, T, 3, 128, 160)))
    metas = [dict(batch_input_shape=(128, 160), img_shape=(128, 160, 3),
                  scale_factor=(1., 1., 1., 1.)) for _ in range(B)]
    cfg = dict(num_frames=T, num_keypoints=15, num_query=300, max_per_img=N, backbone='hrnet')
    exp, taps = [], []
    for b in range(B):
        taps.append({})
        with torch.no_grad():
            exp.append(R.videopose_simple_test(sd, cfg, img[b:b + 1], taps=taps[b]))
    prop = torch.cat([t['topk_idx'] for t in taps], 0)
    score = torch.stack([t['score_topk_idx'].view(-1) for t in taps], 0)
    with torch.no_grad():
        outs = m.bbox_head(m.extract_feat(img.cuda()), metas)
        for b in range(B):
            _close(outs['memory'].permute(1, 0, 2)[b * T:(b + 1) * T].cpu().numpy(),
                                       taps[b]['memory'].numpy(), rtol=2e-3, atol=5e-4)
            _assert_same_selection(m.bbox_head.transformer.last_enc_cls[b, :, 0], prop[b], 1e-4,
                                   'proposals')
        res = m.forward_device(img.cuda(), metas, force_topk_proposals=prop.cuda(),
                               force_score_topk=score.cuda())
        got = m.bbox_head.results_to_list(res)
    for b in range(B):
        assert got[b][2].shape == exp[b][2].shape
        _close(got[b][2].cpu().numpy(), exp[b][2].numpy(), rtol=1e-4, atol=1e-2)
        _close(got[b][0].cpu().numpy(), exp[b][0].numpy(), rtol=1e-4, atol=1e-2)


def test_deterministic_mode_is_bit_reproducible_and_matches_default():
    """set_deterministic: no MIOpen convolution on the path -> two runs are bit-identical (the
    default path is not: MIOpen's fp32 3x3 kernels accumulate in a run-dependent order); both
    agree to rounding."""
    from pavenet_amd.bricks import set_deterministic
    m = _build(3, 12)
    metas = [dict(batch_input_shape=(128, 160), img_shape=(120, 150, 3),
                  scale_factor=(1., 1., 1., 1.))]
    img = _t(seeded_array('det.img', (1, 3, 3, 128, 160))).cuda()
    with torch.no_grad():
        feat_default = m.extract_feat(img)
        set_deterministic(m, True)
        feats = [m.extract_feat(img) for _ in range(3)]
        res = [m.forward_device(img, metas) for _ in range(3)]
    for f in feats[1:]:
        assert all(torch.equal(a, b) for a, b in zip(feats[0], f))
    for r in res[1:]:
        assert torch.equal(r['kpts'], res[0]['kpts']) and torch.equal(r['keep'], res[0]['keep'])
    for a, b in zip(feat_default, feats[0]):
        _close(a.cpu().numpy(), b.cpu().numpy(), rtol=1e-3, atol=1e-4)


def test_hipgraph_replay_equals_eager():
    from pavenet_amd.bricks import set_deterministic
    from pavenet_amd.graph import GraphedForward
    m = set_deterministic(_build(3, 12))  # two separate runs are compared value by value
    metas = [dict(batch_input_shape=(128, 160), img_shape=(120, 150, 3),
                  scale_factor=(1., 1., 1., 1.))]
    a = _t(seeded_array('graph.a', (1, 3, 3, 128, 160))).cuda()
    b = _t(seeded_array('graph.b', (1, 3, 3, 128, 160))).cuda()
    g = GraphedForward(m, a, metas)
    for img in (a, b, a):
        got = {k: v.clone() for k, v in g(img).items()}
        exp = m.forward_device(img, metas)
        for k in ('bboxes', 'kpts', 'keep'):
            _close(got[k].float().cpu().numpy(),
                                       exp[k].float().cpu().numpy(), rtol=1e-5, atol=1e-4)


def test_tail_hipgraph_replay_equals_eager():
    """pavenet_amd.graph.TailGraphedForward: backbone / neck / encoder eager, everything behind the encoder
    (proposals, top-k, both decoders, post-processing, OKS-NMS) replayed as one hipGraph -- the same values as
    the eager forward, for new inputs too, on a padded two-clip batch (per-clip masks, valid ratios and the
    masked-row fills are inside the capture) and in the headline GEMM mode."""
    from pavenet_amd import bricks
    from pavenet_amd.graph import TailGraphedForward
    m = _build(3, 12)
    metas = [dict(batch_input_shape=(128, 160), img_shape=(120, 150, 3), scale_factor=(1., 1., 1., 1.)),
             dict(batch_input_shape=(128, 160), img_shape=(128, 141, 3), scale_factor=(1., 1., 1., 1.))]
    a = _t(seeded_array('tailgraph.a', (2, 3, 3, 128, 160))).cuda()
    b = _t(seeded_array('tailgraph.b', (2, 3, 3, 128, 160))).cuda()
    bricks.set_gemm_mode('bf16x3')
    old_rows = bricks._GEMM['min_rows']
    bricks._GEMM['min_rows'] = 1
    try:
        with torch.no_grad():
            g = TailGraphedForward(m, a, metas)
            for img in (a, b, a):
                got = {k: v.clone() for k, v in g(img).items()}
                exp = m.forward_device(img, metas)
                for k in ('bboxes', 'kpts', 'keep'):
                    assert torch.equal(got[k], exp[k]), k      # (the split kernels are run-to-run reproducible)
    finally:
        bricks._GEMM['min_rows'] = old_rows
        bricks.set_gemm_mode('native')


def test_swin_l_t3_vs_reference_golden(golden_dir):
    """Swin-L T = 3 PAVE-Net (configs/videopose/2025-2-7/2025_2_7_swin_num_frames_3_posetrack17.py)
    against the reference's outputs."""
    from pavenet_amd.models import build_model, videopose_r50_cfg, with_swin_l
    g = _g(golden_dir, 'e2e_videopose_swinl_t3')
    N = int(g['score_topk'].shape[0])
    m = build_model(with_swin_l(videopose_r50_cfg(num_frames=3, max_per_img=N), num_frames=3))
    m = _seed(m, g).cuda().eval()
    metas = [dict(batch_input_shape=(128, 160), img_shape=(120, 150, 3),
                  scale_factor=(1., 1., 1., 1.))]
    with torch.no_grad():
        feat = m.extract_feat(_t(g['img']).cuda())
        outs = m.bbox_head(feat, metas)
        memory = outs['memory'].permute(1, 0, 2)
        _close(memory[1::3].cpu().numpy(), g['memory_center'],
                                   rtol=2e-3, atol=1e-3)
        _assert_same_selection(outs['enc_cls_scores'][0, :, 0], g['enc_topk'], 2e-4, 'proposals')
        outs = m.bbox_head(feat, metas, force_topk_proposals=_t(g['enc_topk']).cuda())
        _close(outs['hs'].permute(0, 2, 1, 3).cpu().numpy(), g['hs'],
                                   rtol=2e-3, atol=2e-3)
        res = m.bbox_head.get_bboxes(outs, metas, force_score_topk=_t(g['score_topk'])[None].cuda())
        (bboxes, labels, kpts), = m.bbox_head.results_to_list(res)
    assert kpts.shape == g['det_kpts'].shape
    _close(kpts.cpu().numpy(), g['det_kpts'], rtol=1e-4, atol=2e-2)


def test_streaming_video_equals_per_window_simple_test():
    """Per-frame encoder-memory cache: every frame of a 6-frame video, decoded from
    cached slabs, equals simple_test on its edge-replicated T = 3 window."""
    from pavenet_amd.streaming import VideoPoseStream
    m = _build(3, 12)
    meta = dict(batch_input_shape=(128, 160), img_shape=(120, 150, 3), scale_factor=(1., 1., 1., 1.))
    video = _t(seeded_array('stream.video', (6, 3, 128, 160))).cuda()
    stream = VideoPoseStream(m, meta, encode_chunk=4, decode_chunk=4)
    got = stream.infer_video(video)
    wins = stream.window_indices(6, 3)
    assert wins[0] == [0, 0, 1] and wins[5] == [4, 5, 5] and wins[2] == [1, 2, 3]
    assert len(got) == 6 and all(torch.isfinite(r[2]).all() for r in got)
    slabs = stream.encode(video)
    for c, w in enumerate(wins):
        clip = video[w][None]  # [1, T, 3, H, W]
        res = m.forward_device(clip, [meta])
        exp = m.bbox_head.results_to_list(res)[0]
        # same selections on both sides: the two paths run the backbone at different batch
        # sizes, and the vendor kernels' rounding noise may swap near-tied top-k members
        res_s = stream.decode(slabs, [w],
                              force_topk_proposals=m.bbox_head.transformer.last_topk_proposals,
                              force_score_topk=res['score_index'])
        got_c = m.bbox_head.results_to_list(res_s)[0]
        assert got_c[2].shape == exp[2].shape
        _close(got_c[2].cpu().numpy(), exp[2].cpu().numpy(),
                                   rtol=1e-4, atol=1e-2)


def test_streaming_value_cache_is_tied_to_its_slabs():
    """Advisor finding (round 3): the per-frame projected-value cache belongs to the slab list that
    encode() returned.  Incremental encoding (`into=`) extends slabs and cache together and decodes
    exactly like a one-shot encode; slabs of an EARLIER encode keep decoding correctly after the
    stream has encoded another video (their own cache, not the stream's latest); a plain list of
    slabs takes the per-window projection (no frame table) and agrees to rounding."""
    from pavenet_amd.streaming import FrameSlabs, VideoPoseStream
    m = _build(3, 12)
    meta = dict(batch_input_shape=(128, 160), img_shape=(128, 160, 3), scale_factor=(1., 1., 1., 1.))
    video = _t(seeded_array('stream.video.a', (7, 3, 128, 160))).cuda()
    other = _t(seeded_array('stream.video.b', (3, 3, 128, 160))).cuda()
    stream = VideoPoseStream(m, meta, encode_chunk=4, decode_chunk=4)
    wins = stream.window_indices(7, 3)

    def dec(slabs, w, **kw):
        res = stream.decode(slabs, w, **kw)
        return res, [r[2].clone() for r in m.bbox_head.results_to_list(res)]
    one = stream.encode(video)
    assert isinstance(one, FrameSlabs) and one.covers([0, 6]) and one.n_cached == 7
    res1, exp = dec(one, wins[2:5])
    pin = dict(force_topk_proposals=m.bbox_head.transformer.last_topk_proposals,
               force_score_topk=res1['score_index'])
    inc = stream.encode(video[:3])
    assert inc.values[0][0].shape[0] == 3
    stream.encode(video[3:], into=inc)          # grows slabs and cache (capacity 3 -> 7)
    assert len(inc) == 7 and inc.n_cached == 7 and inc.covers([0, 6])
    def same(got, exp, atol):
        for a, b in zip(got, exp):
            assert a.shape == b.shape
            _close(a.cpu().numpy(), b.cpu().numpy(), rtol=1e-4, atol=atol)
    # (the two encodes run the backbone at other batch sizes: vendor kernels round differently)
    for a, b in zip(one.values[0] + one.values[1], inc.values[0] + inc.values[1]):
        _close(a[:7].cpu().numpy(), b[:7].cpu().numpy(), rtol=2e-3, atol=2e-3)
    _, got = dec(inc, wins[2:5], **pin)
    same(got, exp, 1e-2)
    stream.encode(other)                        # another video through the same stream object
    _, got = dec(one, wins[2:5], **pin)         # the earlier slabs still use THEIR cache:
    assert all(torch.equal(a, b) for a, b in zip(got, exp))     # the very same computation
    _, got = dec(list(one), wins[2:5], **pin)   # plain list: per-window projection, no table
    same(got, exp, 1e-3)
    with pytest.raises(AssertionError):
        stream.decode(one, [[5, 6, 7]])         # index past the end of the slab list


def test_split_gemm_mode_matches_native():
    """Opt-in bf16x3 split GEMM under the whole model: encoder memory and final keypoints agree
    with the native fp32 path to fp32 rounding (selections pinned: near-tie robust)."""
    from pavenet_amd import bricks
    m = _build(3, 12)
    metas = [dict(batch_input_shape=(128, 160), img_shape=(120, 150, 3),
                  scale_factor=(1., 1., 1., 1.))]
    img = _t(seeded_array('split.img', (1, 3, 3, 128, 160))).cuda()
    old_rows = bricks._GEMM['min_rows']
    try:
        with torch.no_grad():
            feat = m.extract_feat(img)
            outs = m.bbox_head(feat, metas)
            res = m.bbox_head.get_bboxes(outs, metas)
            prop = m.bbox_head.transformer.last_topk_proposals
            bricks.set_gemm_mode('bf16x3')
            bricks._GEMM['min_rows'] = 1          # exercise it at test sizes
            feat2 = m.extract_feat(img)
            outs2 = m.bbox_head(feat2, metas, force_topk_proposals=prop)
            res2 = m.bbox_head.get_bboxes(outs2, metas, force_score_topk=res['score_index'])
    finally:
        bricks.set_gemm_mode('native')
        bricks._GEMM['min_rows'] = old_rows
    assert bricks._SPLIT_STATS['made'] > 10, 'the split GEMM was not exercised'
    for a, b in zip(feat, feat2):
        _close(b.cpu().numpy(), a.cpu().numpy(), rtol=1e-4, atol=1e-4)
    _close(outs2['memory'].cpu().numpy(), outs['memory'].cpu().numpy(),
                               rtol=1e-3, atol=2e-4)
    _close(res2['kpts'].cpu().numpy(), res['kpts'].cpu().numpy(),
                               rtol=1e-4, atol=1e-2)


def test_fp16_projection_mode_within_half_pixel():
    """BASELINE config 5's reduced-precision projections (`set_gemm_mode('fp16')`: fp16 operands,
    fp32 accumulate, sampling / softmax / LayerNorm in fp32): keypoints within 0.5 px of the fp32
    path (SURVEY 8c tolerance for fp16 projections), selections pinned."""
    from pavenet_amd import bricks
    m = _build(3, 12)
    metas = [dict(batch_input_shape=(128, 160), img_shape=(120, 150, 3),
                  scale_factor=(1., 1., 1., 1.))]
    img = _t(seeded_array('fp16.img', (1, 3, 3, 128, 160))).cuda()
    old_rows = bricks._GEMM['min_rows']
    try:
        with torch.no_grad():
            res = m.forward_device(img, metas)
            prop = m.bbox_head.transformer.last_topk_proposals
            bricks.set_gemm_mode('fp16')
            bricks._GEMM['min_rows'] = 1
            res2 = m.forward_device(img, metas, force_topk_proposals=prop,
                                    force_score_topk=res['score_index'])
    finally:
        bricks.set_gemm_mode('native')
        bricks._GEMM['min_rows'] = old_rows
    d = (res2['kpts'][..., :2] - res['kpts'][..., :2]).abs().max().item()
    assert 0 < d < 0.5, d


def test_full_size_800x1344_vs_reference_golden(golden_dir):
    """outputs at the BENCHMARK size.  T = 3 R-50 at 800 x 1344 (S = 22 323 tokens;
    XCD band ordering, tile kernel, shipped per-shape GEMM selections, tail kernel at 1.9 M rows --
    everything bench.py runs) against artefacts of the real reference: per-stage statistics,
    sampled memory rows, all proposal logits, decoder states, detections within 1e-2 px."""
    from pavenet_amd import tuning
    g = _g(golden_dir, 'full_videopose_r50_t3')
    stats = json.loads(str(g['stats']))
    N = int(g['score_topk'].shape[0])
    m = _build(3, N, g)
    img = _t(seeded_array('full_videopose_r50_t3.img', (1, 3, 3, 800, 1344))).cuda()
    metas = [dict(batch_input_shape=(800, 1344), img_shape=(800, 1344, 3),
                  scale_factor=(1., 1., 1., 1.))]
    tuning.use_tuned_gemms()
    try:
        with torch.no_grad():
            feat = m.extract_feat(img)
            for i, f in enumerate(feat):
                mean, amax, _ = stats[f'neck{i}']
                assert abs(float(f.mean()) - mean) < 1e-4
                assert abs(float(f.abs().max()) - amax) < 1e-3 * amax
            _close(feat[3].cpu().numpy(), g['neck3'], rtol=1e-3, atol=3e-4)
            outs = m.bbox_head(feat, metas)
            memory = outs['memory'].permute(1, 0, 2)  # [B*T, S, C]
            mean, amax, _ = stats['memory']
            assert abs(float(memory.mean()) - mean) < 1e-4
            assert abs(float(memory.abs().max()) - amax) < 2e-3 * amax
            rows = _t(g['rows']).cuda()
            _close(memory[:, rows].cpu().numpy(), g['memory_rows'],
                                       rtol=2e-3, atol=5e-4)
            _close(outs['enc_cls_scores'][0, :, 0].cpu().numpy(), g['enc_cls'],
                                       rtol=1e-3, atol=1e-3)
            _assert_same_selection(outs['enc_cls_scores'][0, :, 0], g['enc_topk'], 1e-4, 'proposals')
            outs = m.bbox_head(feat, metas, force_topk_proposals=_t(g['enc_topk']).cuda())
            _close(outs['hs'][-1].permute(1, 0, 2).cpu().numpy(), g['hs_last'],
                                       rtol=2e-3, atol=1e-3)
            _close(outs['inter_references'].cpu().numpy(),
                                       g['inter_references'], rtol=1e-3, atol=2e-4)
            _close(outs['all_cls_scores'][-1].cpu().numpy(), g['cls_last'],
                                       rtol=1e-3, atol=1e-3)
            _assert_same_selection(outs['all_cls_scores'][-1][0].sigmoid(), g['score_topk'], 1e-5,
                                   'score top-k')
            res = m.bbox_head.get_bboxes(outs, metas, rescale=False,
                                         force_score_topk=_t(g['score_topk'])[None].cuda())
            (bboxes, labels, kpts), = m.bbox_head.results_to_list(res)
    finally:
        tuning.disable()
    assert kpts.shape == g['det_kpts'].shape, 'OKS-NMS keep set differs from the reference'
    _close(kpts.cpu().numpy(), g['det_kpts'], rtol=1e-4, atol=1e-2)
    _close(bboxes.cpu().numpy(), g['det_bboxes'], rtol=1e-4, atol=1e-2)


_ORACLE_RUNS = {}   # (T, backbone) -> the oracle's result on clip 0 (one CPU run shared by the tests of a shape)


def _full_size_vs_oracle(T, B, backbone='r50', seed=1234, gemm='bf16x3', tol_px=1e-3, img_shapes=None,
                         canvas=(800, 1344)):
    """bench.py's batch of a BASELINE configuration at 800 x 1344 (bench weights, headline GEMM mode
    'bf16x3', shipped GEMM selections): clip 0 against ONE run of the CPU oracle -- key points within
    1e-3 px with the oracle's two top-k selections pinned, equal OKS-NMS keep sets, and the FREE run
    (nothing pinned) making a valid selection and reproducing every pose the oracle keeps under it.  gemm='fp16' (BASELINE configs[4]'s fp16 MFMA
    projections, BASELINE.md section 4: <= 0.5 px): the pinned comparison at tol_px and equal keep sets."""
    import bench
    from pavenet_amd import bricks, tuning
    from pavenet_amd.models import build_model, videopose_r50_cfg, with_hrnet_w48
    from pavenet_amd.weights import init_random_weights
    N, K = 20, 15
    H, W = canvas
    mcfg = videopose_r50_cfg(num_frames=T, max_per_img=N)
    if backbone == 'hrnet_w48':
        mcfg = with_hrnet_w48(mcfg)
    m = build_model(mcfg)
    init_random_weights(m, seed=0)
    m = m.cuda().eval()

    class A:
        height, width = H, W
    clip0 = bench.clip0_image(A, T)
    g = torch.Generator(device='cuda').manual_seed(seed)
    img = torch.randn(B, T, 3, H, W, device='cuda', generator=g)
    img[0].copy_(clip0[0])
    # img_shapes: per-clip valid sizes (h, w) inside the H x W batch -- a PADDED batch (HEAD:429-445)
    shapes = [tuple(s) + (3,) for s in img_shapes] if img_shapes is not None else [(H, W, 3)] * B
    metas = [dict(batch_input_shape=(H, W), img_shape=shapes[i], scale_factor=(1., 1., 1., 1.))
             for i in range(B)]
    sd = {k: v.detach().float().cpu() for k, v in m.state_dict().items()}
    cfg = dict(num_frames=T, num_keypoints=K, num_query=300, max_per_img=N)
    if backbone == 'hrnet_w48':
        cfg['backbone'] = 'hrnet'
    okey = (T, backbone, shapes[0], (H, W))
    if okey not in _ORACLE_RUNS:
        taps = {}
        old = R.SAMPLER
        R.SAMPLER = 'torch'
        try:
            with torch.no_grad():
                eb, el, ek = R.videopose_simple_test(sd, cfg, clip0, img_shape=shapes[0], taps=taps)
        finally:
            R.SAMPLER = old
        _ORACLE_RUNS[okey] = (eb, el, ek, {k: taps[k] for k in ('topk_idx', 'score_topk_idx')})
    eb, el, ek, taps = _ORACLE_RUNS[okey]
    bricks.set_gemm_mode(gemm)
    tuning.use_tuned_gemms()
    try:
        with torch.no_grad():
            # (strict: the forward raises if a torch / vendor compute operator ran on a device tensor)
            free_res = m.forward_device(img, metas, strict=True)
            free = m.bbox_head.results_to_list(free_res)[0][2].cpu()
            assert not m.last_census.slow_paths, m.last_census.slow_paths
            free_sel = (m.bbox_head.transformer.last_topk_proposals[0].cpu().clone(),
                        free_res['score_index'][0].cpu().clone(),
                        m.bbox_head.transformer.last_enc_cls[0, :, 0].cpu().clone())
            res = m.forward_device(img[:1], metas[:1],
                                   force_topk_proposals=taps['topk_idx'].cuda(),
                                   force_score_topk=taps['score_topk_idx'].view(1, -1).cuda())
            (gb, gl, gk), = m.bbox_head.results_to_list(res)
    finally:
        tuning.disable()
        bricks.set_gemm_mode('native')
    assert tuple(gk.shape) == tuple(ek.shape), 'OKS-NMS keep set differs from the oracle'
    assert ek.shape[0] >= 5, 'degenerate clip: too few poses survive NMS to mean anything'
    max_px = float((gk.cpu()[..., :2] - ek[..., :2]).abs().max())
    assert max_px <= tol_px, max_px
    if gemm != 'bf16x3':
        assert max_px > 1e-5, 'suspiciously exact: did the 16-bit mode run?'
        _close(gb.cpu().numpy()[:, :4], eb.numpy()[:, :4], rtol=0, atol=tol_px)
        _close(gk.cpu().numpy()[..., 2], ek.numpy()[..., 2], rtol=2e-2, atol=2e-3)   # key-point scores
        assert free.shape[0] >= 1
        return
    _close(gb.cpu().numpy()[:, :4], eb.numpy()[:, :4], rtol=0, atol=1e-3)
    _close(gk.cpu().numpy()[..., 2], ek.numpy()[..., 2], rtol=1e-4, atol=1e-5)   # key-point scores
    if img_shapes is not None:
        # a padded batch: EVERY clip INSIDE the batch (runs of frames with their own positional table, mask rows and
        # valid ratios; deform_attn._forward_merged_groups, the fill_rows_ passes of project_values_hoisted,
        # MaskList.masked_rows) against its own oracle run on its own valid size -- final key points <= tol_px with
        # the oracle's two selections pinned per clip, equal OKS-NMS keep sets (advisor finding of round 5: only
        # clip 0, the first run of frames, used to be compared, and only on decoder states)
        runs = [(eb, el, ek, taps)]
        old = R.SAMPLER
        R.SAMPLER = 'torch'
        try:
            for c in range(1, B):
                tc = {}
                with torch.no_grad():
                    r = R.videopose_simple_test(sd, cfg, img[c:c + 1].cpu(), img_shape=shapes[c], taps=tc)
                runs.append(r + ({k: tc[k] for k in ('topk_idx', 'score_topk_idx')},))
        finally:
            R.SAMPLER = old
        sel_p = torch.stack([r[3]['topk_idx'].view(-1) for r in runs]).cuda()
        sel_s = torch.stack([r[3]['score_topk_idx'].view(-1) for r in runs]).cuda()
        bricks.set_gemm_mode(gemm)
        tuning.use_tuned_gemms()
        try:
            with torch.no_grad():
                res = m.forward_device(img, metas, force_topk_proposals=sel_p, force_score_topk=sel_s)
                got = m.bbox_head.results_to_list(res)
        finally:
            tuning.disable()
            bricks.set_gemm_mode('native')
        for c, ((cb, cl, ck, _), (gb_, gl_, gk_)) in enumerate(zip(runs, got)):
            assert tuple(gk_.shape) == tuple(ck.shape), f'clip {c}: OKS-NMS keep set differs from the oracle'
            assert ck.shape[0] >= 5, f'clip {c}: degenerate, too few poses survive NMS'
            px = float((gk_.cpu()[..., :2] - ck[..., :2]).abs().max())
            assert px <= tol_px, f'clip {c} inside the padded batch: {px} px from its oracle run'
            _close(gb_.cpu().numpy()[:, :4], cb.numpy()[:, :4], rtol=0, atol=1e-3)
            _close(gk_.cpu().numpy()[..., 2], ck.numpy()[..., 2], rtol=1e-4, atol=1e-5)
        return
    # the un-pinned batch run (its own top-k selections, its own NMS).  The proposal top-k is a SORTED list of 300 of
    # ~22 000 logits and query i adds its own embedding to proposal i (OT:21400-21403), so two logits a few 1e-6
    # apart that swap places between the CPU oracle and the device give two queries other inputs: a free run can
    # only be expected to reproduce the oracle's poses where it makes the oracle's selections.  Hence: the free
    # selection must be a valid top-k of OUR logits up to near-ties; if it IS the oracle's, every oracle pose is
    # reproduced within 1e-3 px; if it differs on near-ties, the oracle is run once more with the device's own
    # selections forced and must then give the device's poses (<= 1e-3 px, same keep set).
    free_prop, free_score, free_logits = free_sel
    _assert_same_selection(free_logits, taps['topk_idx'], 1e-4, 'proposals (free run)')
    same = torch.equal(free_prop, taps['topk_idx'].view(-1)) and torch.equal(free_score, taps['score_topk_idx'].view(-1))
    ek_free = ek
    if not same:
        old = R.SAMPLER
        R.SAMPLER = 'torch'
        try:
            with torch.no_grad():
                t2 = {'force_topk_idx': free_prop.view(1, -1), 'force_score_topk_idx': free_score.view(-1)}
                _, _, ek_free = R.videopose_simple_test(sd, cfg, clip0, img_shape=shapes[0], taps=t2)
        finally:
            R.SAMPLER = old
    assert free.shape[0] == ek_free.shape[0], (free.shape, ek_free.shape, same)
    for pose in ek_free[..., :2]:
        assert float((free[..., :2] - pose).abs().amax(dim=(1, 2)).min()) <= 1e-3, same


def test_bench_batch_full_size_t7_b4_vs_oracle():
    """BASELINE configs[2] at FULL size inside the GPU suite: bench.py's own batch (R-50, T = 7,
    4 clips of 800 x 1344), clip 0 against one oracle run (about a minute on the box's host cores)."""
    _full_size_vs_oracle(7, 4)


def test_hrnet_w48_full_size_t7_vs_oracle():
    """BASELINE configs[3] at FULL size: HRNet-w48 + MulFrames head, T = 7, one 800 x 1344 clip --
    the size-gated convolution forms of the 48 / 96 / 192 / 384-channel branches (wide tiles,
    96-column tiles, three blocks per CU, the LDS-window 3x3) that a 128 x 160 input never takes."""
    _full_size_vs_oracle(7, 1, backbone='hrnet_w48')


def test_t15_full_size_unsharded_vs_oracle():
    """The BASELINE configs[4] shape at FULL size, un-sharded, exact arithmetic: R-50, T = 15, one
    800 x 1344 clip (15-frame T-frame attention kernels, 15 x 22 323-token memory)."""
    _full_size_vs_oracle(15, 1)


def test_padded_batch_full_size_vs_oracle():
    """A PADDED batch at full size on the encoder's fast path: two clips of T = 7 in an 800 x 1344 batch with
    valid sizes 800 x 1333 and 750 x 1333 (the reference's test pipeline pads to a multiple of 32,
    configs/_base_/datasets/coco_keypoint.py:79; masks per clip from img_shape, HEAD:429-445) -- two runs of
    frames with their own positional table, padding pattern and valid ratios through the merged projection
    GEMM + one sampler launch, value rows of masked tokens zeroed (MO:369-371), the decoders' masked memory
    (OT:1706-1711, MO:1454-1458) as bias rows.  Clip 0 alone and EVERY clip inside the batch against its own
    oracle run: final key points <= 1e-3 px with the oracle's selections pinned, equal OKS-NMS keep sets."""
    _full_size_vs_oracle(7, 2, img_shapes=[(800, 1333), (750, 1333)])


def test_t15_full_size_fp16_vs_oracle():
    """BASELINE configs[4] as written -- R-50, T = 15, "fp16 MFMA projections" -- at FULL size, un-sharded:
    every GEMM / convolution of the forward on the fp16-operand form of the LDS-DMA kernels (sampling,
    softmax, LayerNorm statistics, residuals and accumulation stay fp32), key points within 0.5 px of the
    fp32 oracle with its selections pinned, equal OKS-NMS keep set (the oracle run is shared with the exact
    T = 15 test above)."""
    _full_size_vs_oracle(15, 1, gemm='fp16', tol_px=0.5)


def test_posetrack_canvas_750x1333_full_size_vs_oracle():
    """The canvas the reference's own video test pipeline produces (configs/_base_/datasets/
    posetrack17_video_keypoint.py:68-84: keep-ratio resize to (1333, 800), Pad(size_divisor=1) -- i.e. no padding):
    a 1080p clip is a 750 x 1333 batch, un-padded, ODD width, maps of 375 x 667 -> 94 x 167, 47 x 84, 24 x 42,
    12 x 21.  BASELINE configs[1] (R-50, T = 3, one clip) on it: the stem through the re-laid rows + LDS-window
    kernel, every later map on an odd pitch, the tile sampler on a pyramid whose levels do not halve exactly --
    <= 1e-3 px against the oracle with its selections pinned, equal keep set, the free run (strict: no torch /
    vendor compute operator, no slow-path kernel) reproducing every oracle pose."""
    _full_size_vs_oracle(3, 1, canvas=(750, 1333))


_CENSUS_CASES = [
    ('configs[0] PETR R-50 single image', 'petr', 1, 1, 'bf16x3', None, (800, 1344)),
    ('configs[1] R-50 T=3', 'r50', 3, 1, 'bf16x3', None, (800, 1344)),
    ('configs[2] R-50 T=7 x 4 clips', 'r50', 7, 4, 'bf16x3', None, (800, 1344)),
    ('configs[2] as a padded batch', 'r50', 7, 2, 'bf16x3', [(800, 1333), (750, 1333)], (800, 1344)),
    ('configs[3] HRNet-w48 T=7', 'hrnet_w48', 7, 1, 'bf16x3', None, (800, 1344)),
    ('configs[4] R-50 T=15', 'r50', 15, 1, 'bf16x3', None, (800, 1344)),
    ('configs[4] R-50 T=15, fp16 projections', 'r50', 15, 1, 'fp16', None, (800, 1344)),
    ('Swin-L T=3', 'swin_l', 3, 1, 'bf16x3', None, (800, 1344)),
    ('PoseTrack canvas 750x1333 T=3', 'r50', 3, 1, 'bf16x3', None, (750, 1333)),
]


@pytest.mark.parametrize('case', _CENSUS_CASES, ids=[c[0] for c in _CENSUS_CASES])
def test_no_fallback_ops_on_the_baseline_workloads(case):
    """the module layer chooses between this package's launches and torch / vendor
    operators through ~60 shape / dtype gates; a workload that drops off a fast path used to do so silently.
    `forward_device(strict=True)` runs the (warm) forward under pavenet_amd.census.LaunchCensus and raises if a GEMM,
    convolution, attention, normalisation, pooling, top-k or interpolation operator of torch ran on a device
    tensor -- asserted here for every BASELINE configuration, a padded batch, Swin-L and the reference's own
    750 x 1333 PoseTrack canvas at full size, together with: no host sync inside the forward, no slow-path kernel,
    and a bounded number of other ATen launches (elementwise / copies; the un-padded R-50 workloads: <= 12)."""
    from pavenet_amd import bricks
    from pavenet_amd.models import (build_model, petr_r50_cfg, videopose_r50_cfg, with_hrnet_w48, with_swin_l)
    from pavenet_amd.weights import init_random_weights
    name, backbone, T, B, gemm, img_shapes, (H, W) = case
    if backbone == 'petr':
        mcfg = petr_r50_cfg(num_keypoints=17, max_per_img=20)
    else:
        mcfg = videopose_r50_cfg(num_frames=T, max_per_img=20)
        if backbone == 'hrnet_w48':
            mcfg = with_hrnet_w48(mcfg)
        elif backbone == 'swin_l':
            mcfg = with_swin_l(mcfg, num_frames=T)
    m = init_random_weights(build_model(mcfg), seed=0).cuda().eval()
    g = torch.Generator(device='cuda').manual_seed(7)
    img = torch.randn((B, 3, H, W) if backbone == 'petr' else (B, T, 3, H, W), device='cuda', generator=g)
    shapes = [tuple(s) + (3,) for s in img_shapes] if img_shapes else [(H, W, 3)] * B
    metas = [dict(batch_input_shape=(H, W), img_shape=shapes[i], scale_factor=(1., 1., 1., 1.)) for i in range(B)]
    bricks.set_gemm_mode(gemm)
    try:
        try:
            res = m.forward_device(img, metas, strict='where')   # raises census.FallbackError on a vendor operator
        except Exception:
            print('call sites:', m.last_census.summary().get('sites'))
            raise
        torch.cuda.synchronize()
    finally:
        bricks.set_gemm_mode('native')
    c = m.last_census
    print(f'{name}: call sites of the ATen launches: {c.summary().get("sites")}')
    assert not c.fallback_ops, dict(c.fallback_ops)
    assert not c.host_syncs, dict(c.host_syncs)
    assert not c.slow_paths, dict(c.slow_paths)
    n_aten = sum(c.aten_launches.values())
    print(f'{name}: {n_aten} ATen launches per step: {dict(c.aten_launches)}')
    # (PETR -- BASELINE configs[0], the reference's CPU-plumbing case -- keeps the tensor formulation of its
    # proposal / post-processing stages: ~180 small elementwise launches, none of them a fallback operator)
    limit = 12 if (backbone == 'r50' and img_shapes is None) else (200 if backbone == 'petr' else 60)
    assert n_aten <= limit, dict(c.aten_launches)
    assert int(res['keep'].sum()) >= 1


@pytest.mark.parametrize('B', [2, 4])
def test_forward_is_the_same_from_the_first_call_and_reads_no_stale_memory(B):
    """The size-gated fast paths and the derived-operand caches must not change a value: at a batch
    large enough to take every one of them (T = 7 x 2 and x 4 clips -- the bench batch: 698 row tiles of
    centre-frame memory, past the 512 from which the LayerNorm-epilogue GEMM changes form; round 5's first cut of
    the per-clip proposal path differed from the cold path there --, 800x1344, headline GEMM mode) the FIRST
    forward of a fresh model (every cache cold) is bit-identical to the second, and to a third run
    after the allocator's free memory was filled with NaN (a kernel reading memory it did not write
    -- split-K workspace, chain scratch, LDS-DMA tails -- would show).  Found in round 3: the cold
    path of the two-stage proposals ran Linear + LayerNorm as two torch ops, the cached path as the
    fused kernel; near-tie top-k selections then differed between the first and later forwards."""
    from pavenet_amd import bricks, tuning
    from pavenet_amd.models import build_model, videopose_r50_cfg
    from pavenet_amd.weights import init_random_weights
    T, H, W = 7, 800, 1344
    m = build_model(videopose_r50_cfg(num_frames=T, max_per_img=20))
    init_random_weights(m, seed=0)
    m = m.cuda().eval()
    g = torch.Generator(device='cuda').manual_seed(99)
    img = torch.randn(B, T, 3, H, W, device='cuda', generator=g)
    metas = [dict(batch_input_shape=(H, W), img_shape=(H, W, 3), scale_factor=(1., 1., 1., 1.))
             for _ in range(B)]

    def fwd():
        with torch.no_grad():
            res = m.forward_device(img, metas)
        return {k: v.clone() for k, v in res.items() if torch.is_tensor(v)}

    def poison():
        torch.cuda.synchronize()
        blocks = []
        for sz in (4 << 30, 2 << 30, 1 << 30, 1 << 30, 512 << 20, 256 << 20, 128 << 20, 64 << 20,
                   32 << 20, 16 << 20, 8 << 20, 4 << 20, 2 << 20, 1 << 20):
            blocks.append(torch.full((sz // 4,), float('nan'), dtype=torch.float32, device='cuda'))
        torch.cuda.synchronize()
        del blocks

    bricks.set_gemm_mode('bf16x3')
    tuning.use_tuned_gemms()
    try:
        cold = fwd()
        warm = fwd()
        poison()
        again = fwd()
    finally:
        tuning.disable()
        bricks.set_gemm_mode('native')
    for k in cold:
        assert torch.equal(cold[k], warm[k]), f'{k}: the first forward differs from the second'
        assert torch.equal(warm[k], again[k]), f'{k}: result depends on the contents of free memory'
        assert not torch.isnan(again[k].float()).any(), k


def test_neck_eval_with_grad_keeps_the_differentiable_path():
    """Advisor finding (round 2): the neck's flat path writes through raw pointers (no grad_fn), so
    with grad mode ON (frozen-neck fine-tuning, saliency maps) an eval() neck must fall back to
    the differentiable ConvModule path -- same values, gradients reach GroupNorm, the conv and the
    input."""
    from pavenet_amd import bricks
    from pavenet_amd.models import build_model, videopose_r50_cfg
    m = _build(3, 12)
    neck = m.neck
    feats = [_t(seeded_array(f'neckgrad.{i}', (2, c, h, w))).cuda()
             for i, (c, h, w) in enumerate(((512, 16, 20), (1024, 8, 10), (2048, 4, 5)))]
    for mode in ('native', 'bf16x3'):
        bricks.set_gemm_mode(mode)
        try:
            with torch.no_grad():
                flat = neck(feats)
            xs = [f.clone().requires_grad_(True) for f in feats]
            outs = neck(xs)
            assert all(o.grad_fn is not None for o in outs)
            for a, b in zip(flat, outs):
                _close(b.detach().cpu().numpy(), a.cpu().numpy(), rtol=1e-3, atol=1e-4)
            sum(o.square().mean() for o in outs).backward()
            gn = getattr(neck.convs[0], neck.convs[0].norm_name)
            assert gn.weight.grad is not None and float(gn.weight.grad.abs().sum()) > 0
            assert neck.convs[0].conv.weight.grad is not None and xs[0].grad is not None
            neck.zero_grad()
        finally:
            bricks.set_gemm_mode('native')


@pytest.mark.parametrize('shard', ['clips', 'frames'])
def test_bench_multi_rank_code_path_on_one_gpu(shard):
    """bench.py's N > 1 code (rank set-up, clip-parallel result all-gather / frame-sharded forward,
    max-over-ranks timing, the JSON line) executed every round, started EXACTLY as the driver
    starts it -- `python bench.py --gpus 2 ...`, no launcher in the command: bench.py spawns its own
    ranks (tools/dist_test.sh:8-10).  Two ranks share this box's GPU over gloo
    (PAVE_BENCH_ONE_DEVICE=1; on the 8-GPU node the same code runs on nccl = RCCL)."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, 'bench.py'),
           '--gpus', '2', '--steps', '2', '--warmup', '1', '--height', '128', '--width', '160',
           '--shard', shard, '--frames', '5' if shard == 'frames' else '3', '--full', '--no-cpu-baseline',
           '--gemm-select', 'default']
    env = dict(os.environ, PAVE_BENCH_ONE_DEVICE='1')
    env.pop('WORLD_SIZE', None)
    torch.cuda.empty_cache()
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, (r.stdout[-1500:] + '\n---\n' + r.stderr[-4000:])
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('{')][-1])
    assert line['n_gpus'] == 2 and line['value'] > 0 and line['steps'] == 2
    assert line['scaling'] == ('strong' if shard == 'frames' else 'weak')
    assert line['backend'] == 'gloo' and line['ranks_seen'] == [0, 1] and len(line['devices']) == 2


def test_split_caches_follow_reloaded_weights():
    """The pre-split weight planes are cached on the tensor that owns them, never by address:
    after every reload (which frees and re-allocates the folded-BN weights, typically at the very
    same addresses) the split-GEMM model must follow the NEW weights (advisor finding, round 1)."""
    from pavenet_amd import bricks
    m = _build(3, 12)
    metas = [dict(batch_input_shape=(128, 160), img_shape=(120, 150, 3),
                  scale_factor=(1., 1., 1., 1.))]
    img = _t(seeded_array('cache.img', (1, 3, 3, 128, 160))).cuda()
    shapes = {k: list(v.shape) for k, v in m.state_dict().items()}
    old_rows = bricks._GEMM['min_rows']
    try:
        for salt in (0, 1, 2, 3):
            m.load_state_dict(seeded_state_dict(shapes, salt, like=m.state_dict()), strict=True)
            with torch.no_grad():
                bricks.set_gemm_mode('native')
                ref = [f.clone() for f in m.extract_feat(img)]
                bricks.set_gemm_mode('bf16x3')
                bricks._GEMM['min_rows'] = 1
                got = m.extract_feat(img)
                bricks._GEMM['min_rows'] = old_rows
            for a, b in zip(got, ref):
                _close(a.cpu().numpy(), b.cpu().numpy(), rtol=1e-4, atol=1e-4)
    finally:
        bricks.set_gemm_mode('native')
        bricks._GEMM['min_rows'] = old_rows


def test_derived_operand_caches_follow_reloaded_weights():
    """Everything derived from parameters and cached across steps -- merged / paired / stacked
    projection weights, the merged projection's per-token epilogue table, `pos + level_embed`, the
    tile kernel's window shift -- must follow a weight reload: the whole forward of an UN-padded
    clip (the path that uses them) in the split mode equals the vendor-kernel forward, reload after
    reload, with the proposal / score selections pinned to the latter's."""
    from pavenet_amd import bricks
    m = _build(3, 12)
    head, tr = m.bbox_head, m.bbox_head.transformer
    metas = [dict(batch_input_shape=(128, 160), img_shape=(128, 160, 3),
                  scale_factor=(1., 1., 1., 1.))] * 2
    img = _t(seeded_array('cache2.img', (2, 3, 3, 128, 160))).cuda()
    shapes = {k: list(v.shape) for k, v in m.state_dict().items()}
    old_rows = bricks._GEMM['min_rows']

    def run(force_topk=None, force_score=None):
        kw = {} if force_topk is None else dict(force_topk_proposals=force_topk)
        outs = head(m.extract_feat(img), metas, **kw)
        taps = {}
        res = head.get_bboxes(outs, metas, force_score_topk=force_score, taps=taps)
        return res, tr.last_topk_proposals.clone(), taps['score_topk'].clone()

    try:
        for salt in (0, 1, 2):
            m.load_state_dict(seeded_state_dict(shapes, salt, like=m.state_dict()), strict=True)
            with torch.no_grad():
                bricks.set_gemm_mode('native')
                ref, topk, sel = run()
                bricks.set_gemm_mode('bf16x3')
                bricks._GEMM['min_rows'] = 1
                got, _, _ = run(topk, sel)
                bricks._GEMM['min_rows'] = old_rows
            enc0 = tr.encoder.layers[0].attentions[0]
            assert hasattr(enc0, '_merged_w') and hasattr(enc0, '_table')      # the cached path ran
            _close(got['kpts'].cpu().numpy(), ref['kpts'].cpu().numpy(),
                                       rtol=0, atol=2e-2)
    finally:
        bricks.set_gemm_mode('native')
        bricks._GEMM['min_rows'] = old_rows


def test_simple_test_rescale_result_lists_vs_reference_golden(golden_dir):
    """f3: the public entry `simple_test(img, img_metas, rescale=True)` with a non-unit
    scale_factor, down to the per-class lists of `bbox_kpt2result`
    (opera/core/keypoint/transforms.py:132-154, videoposev1.py:159-190) against the reference's own
    return value.  Keypoints are divided by the scale factor, so 1e-2 px at network scale is
    2.7e-2 px here."""
    from pavenet_amd.detectors import bbox_kpt2result
    g0 = _g(golden_dir, 'e2e_videopose_r50_t3')
    g = _g(golden_dir, 'e2e_videopose_r50_t3_rescale')
    N = int(g0['score_topk'].shape[0])
    m = _build(3, N, g0)
    img = _t(g0['img']).cuda()
    sf = tuple(float(v) for v in g['scale_factor'])
    metas = [dict(batch_input_shape=(128, 160), img_shape=(120, 150, 3), scale_factor=sf)]
    with torch.no_grad():
        res = m.forward_device(img, metas, rescale=True,
                               force_topk_proposals=_t(g0['enc_topk']).cuda(),
                               force_score_topk=_t(g0['score_topk'])[None].cuda())
        (b, l, k), = m.bbox_head.results_to_list(res)
    bbox_results, kpt_results = bbox_kpt2result(b, l, k, m.bbox_head.num_classes)
    assert len(bbox_results) == 1 and len(kpt_results) == 1
    assert isinstance(bbox_results[0], np.ndarray) and kpt_results[0].shape == g['kpt_results'].shape
    _close(kpt_results[0], g['kpt_results'], rtol=1e-4, atol=3e-2)
    _close(bbox_results[0], g['bbox_results'], rtol=1e-4, atol=3e-2)
    # the un-forced public call: same list structure; same numbers whenever its own top-k
    # selections coincide with the reference's (near-ties under random weights may differ)
    (pb, pk), = m.simple_test(img, metas, rescale=True)
    assert len(pb) == 1 and pb[0].shape[1] == 5 and pk[0].shape[1:] == (15, 3)
    if pk[0].shape == g['kpt_results'].shape and \
            set(m.bbox_head.transformer.last_topk_proposals.flatten().tolist()) == \
            set(g0['enc_topk'].flatten().tolist()):
        _close(pk[0], g['kpt_results'], rtol=1e-4, atol=3e-2)
    # empty result lists keep the reference's shapes (transforms.py:145-148)
    eb, ek = bbox_kpt2result(torch.zeros(0, 5), torch.zeros(0, dtype=torch.long),
                             torch.zeros(0, 15, 3), 1)
    assert eb[0].shape == (0, 5) and ek[0].shape == (0, 15, 3)


@pytest.mark.parametrize('padded', [True, False])
def test_streaming_windows_vs_oracle(padded):
    """f2 against the ORACLE (not the product's own per-window path): two windows of a 4-frame
    video decoded from the per-frame encoder-memory cache -- the edge-replicated first window
    [0, 0, 1] and an interior one [1, 2, 3] -- equal `oracle.videopose_simple_test` on the clips
    built by the reference dataset's window rule (posetrack_video_pose.py:578-623).  Un-padded
    frames also take the per-frame PROJECTED-VALUE cache of the five decoder layers, addressed by
    the fused kernels through a frame table (no per-window re-projection)."""
    from pavenet_amd.streaming import VideoPoseStream
    N = 12
    m = _build(3, N)
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    ishape = (120, 150, 3) if padded else (128, 160, 3)
    meta = dict(batch_input_shape=(128, 160), img_shape=ishape, scale_factor=(1., 1., 1., 1.))
    video = _t(seeded_array('stream.oracle.video', (4, 3, 128, 160)))
    stream = VideoPoseStream(m, meta, encode_chunk=3, decode_chunk=2)
    wins = stream.window_indices(4, 3)
    assert wins[0] == [0, 0, 1] and wins[2] == [1, 2, 3]
    slabs = stream.encode(video.cuda())
    assert (slabs.values is None) == padded
    cfg = dict(num_frames=3, num_keypoints=15, num_query=300, max_per_img=N)
    for c in (0, 2):
        taps = {}
        with torch.no_grad():
            eb, el, ek = R.videopose_simple_test(sd, cfg, video[wins[c]][None],
                                                 img_shape=ishape, taps=taps)
        _close(torch.stack([slabs[i] for i in wins[c]]).cpu().numpy(),
                                   taps['memory'].numpy(), rtol=2e-3, atol=5e-4)
        res = stream.decode(slabs, [wins[c]], force_topk_proposals=taps['topk_idx'].cuda(),
                            force_score_topk=taps['score_topk_idx'].view(1, -1).cuda())
        (gb, gl, gk), = m.bbox_head.results_to_list(res)
        assert gk.shape == ek.shape
        _close(gk.cpu().numpy(), ek.numpy(), rtol=1e-4, atol=1e-2)
        _close(gb.cpu().numpy(), eb.numpy(), rtol=1e-4, atol=1e-2)
