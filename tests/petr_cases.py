"""Cases, references and floors shared by tests/test_petr_stages_cpu.py and tests/test_petr_stages_gpu.py: the
single-image family of pavenet_amd/petr.py -- PETRTransformer (encoder, un-fused proposal stage, PetrTransformerDecoder,
the stock DeformableDetrTransformerDecoder as refine decoder) under PETRHead and VedPoseHeadV2 (forward, forward_refine,
get_bboxes) -- tap by tap against fp64.  The sibling of tests/head_cases.py (the video family), whose metric, margin,
launch recorder, encoder hooks and input layout it imports.

Model: build_model(petr_r50_cfg(num_keypoints=K, num_query=Q, max_per_img=N, head=...)) seeded as
tests/test_model_gpu._seed does.  Only `bbox_head` is used, a fresh deep copy per run.

Input: four levels [B, 256, h, w] from oracle.seeded.seeded_array at unit scale, in the two forms of head_cases
('nchw': four dense tensors;  'flat': slices of one token-major buffer).

Reference: fp64 on the CPU, one run per image, joined.  oracle.pavenet_ref.petr_simple_test cannot start behind the
neck, takes no forced selection and keeps no per-layer values, so its tail (everything behind channel_mapper) is
restated in `_image_run` from the oracle's stage functions (make_masks_and_pos, flatten_levels, get_reference_points,
encoder_forward, gen_encoder_output_proposals, mha, pose_attn_single, msda_module, ffn, layer_norm, the branch helpers,
get_p), as head_cases._clip_run does for the video family.

Discrete choices (the Q-of-S proposals, the N-of-Q scores) are taken from the fp64 run and forced on every other run.

Metric, per tap:  e = max|got - ref64| / rms(ref64)   (backbone_cases.rel_err; no absolute term).
Floor:  e_cpu32 = the metric of the oracle's own fp32 run, same forced selections, against its fp64 run.
Taps whose reference leaves no room for error (PETRHead's key-point scores, identically 1; the labels, identically 0;
keep, all ones; order, arange(N)) are compared with torch.equal (`exact_mismatches`), not by ratio.
Every reference is computed once per session (functools.lru_cache) and never modified.
"""
import contextlib
import copy
import functools

import torch

from oracle import pavenet_ref as R
from oracle.seeded import seeded_array
from tests.head_cases import (MARGIN, _views, fmt, memory_hooks, ratios, record_launches,  # noqa: F401  (re-exported)
                              rel_err)

C = 256
N_ENC, N_DEC, N_REF = 6, 3, 2
HEAD_TYPES = {'petr': 'opera.PETRHead', 'vedpose': 'opera.VedPoseHeadV2'}


class Case:
    def __init__(self, name, head, K, canvas, levels, Q, N, img_shapes, seed='a', scale_factors=None):
        self.name, self.head, self.K, self.canvas, self.levels, self.Q, self.N = name, head, K, canvas, levels, Q, N
        self.img_shapes = tuple(img_shapes)       # one (h, w) per image
        self.B = len(self.img_shapes)
        self.S = sum(h * w for h, w in levels)
        self.seed = seed
        # (w_scale, h_scale) per image: get_bboxes runs a second time with rescale=True under these
        self.scale_factors = tuple(scale_factors) if scale_factors else None
        assert Q <= self.S and N <= Q and (scale_factors is None or len(scale_factors) == self.B)

    def __repr__(self):
        return self.name

    @property
    def vedpose(self):
        return self.head == 'vedpose'

    def metas(self, scaled=False):
        sf = self.scale_factors if scaled else [(1., 1.)] * self.B
        return [dict(batch_input_shape=self.canvas, img_shape=s + (3,), scale_factor=(f[0], f[1], f[0], f[1]))
                for s, f in zip(self.img_shapes, sf)]

    def ratio_taps(self):
        """The taps compared by ratio, in stage order."""
        names = [n for n, _ in TAPS]
        if not self.vedpose:
            names = [n for n in names if n not in ('refine_sigma', 'det_kpt_scores')]
        if self.scale_factors:
            names += [n for n, _ in RESCALED_TAPS]
        return tuple(names)


_L128 = ((16, 20), (8, 10), (4, 5), (2, 3))
P1 = Case('p1_petr_128x160_B1', 'petr', 17, (128, 160), _L128, 300, 12, [(128, 160)])
# image 0 un-padded, image 1 padded: the mask AFTER the pose attention's value projection (its bias is not zero under
# the seeded weights), the padded encoder path at T = 1 (one frame group per image), refine slabs / masks / valid
# ratios per image; get_bboxes also with rescale=True and two different non-unit scale factors
P2 = Case('p2_petr_128x160_B2_padded', 'petr', 17, (128, 160), _L128, 300, 12, [(128, 160), (120, 150)],
          scale_factors=[(1.25, 1.5), (0.8, 0.625)])
# odd maps; the sigma branches, get_p and the key-point scores.  Q = 100 needs petr_r50_cfg's num_query to reach the
# transformer
P3 = Case('p3_vedpose_75x133_B1', 'vedpose', 15, (75, 133), ((10, 17), (5, 9), (3, 5), (2, 3)), 100, 10, [(75, 133)])
# a one-row level; three slabs behind one unit_clip table, N * K = 150 poses-times-joints per image
P4 = Case('p4_vedpose_64x96_B3_padded', 'vedpose', 15, (64, 96), ((8, 12), (4, 6), (2, 3), (1, 2)), 100, 10,
          [(64, 96), (56, 96), (64, 80)])
# level 0 is 52 wide: the proposals of its first and last column are invalid (x = 0.5 / 52 < 0.01, OT:21200) in an
# UN-padded image
P5 = Case('p5_petr_64x416_B1', 'petr', 17, (64, 416), ((8, 52), (4, 26), (2, 13), (1, 7)), 100, 10, [(64, 416)])
# runs BEFORE p2 on the same module: same level sizes, same batch size, other img_shapes, another seed -- every cache
# keyed by geometry alone then meets a stale entry
P6_FIRST = Case('p6_first_petr_128x160_B2', 'petr', 17, (128, 160), _L128, 300, 12, [(112, 160), (128, 160)], seed='b')
CASES = (P1, P2, P3, P4, P5)
ALL_CASES = CASES + (P6_FIRST,)

# the taps compared by ratio, in stage order:  name -> stage (the stage groups the docstring table of the GPU file)
TAPS = tuple([(f'mem{i}', 'encoder') for i in range(N_ENC)]
             + [('enc_cls', 'proposals'), ('init_reference', 'proposals')]
             + [(f'hs{i}', 'decoder') for i in range(N_DEC)] + [(f'ref{i}', 'decoder') for i in range(N_DEC)]
             + [(f'cls{i}', 'head') for i in range(N_DEC)] + [(f'kpt{i}', 'head') for i in range(N_DEC)]
             + [(f'refine_hs{i}', 'refine') for i in range(N_REF)]
             + [('refine_kpts', 'refine'), ('refine_sigma', 'refine')]
             + [('det_kpts', 'result'), ('det_kpt_scores', 'result'), ('det_bboxes', 'result')])
RESCALED_TAPS = (('det_kpts_rescaled', 'result'), ('det_bboxes_rescaled', 'result'))
STAGE = dict(TAPS + RESCALED_TAPS)
EXACT_TAPS = ('det_labels', 'keep', 'order')          # + det_kpt_scores under PETRHead
DECODER_STAGES = ('proposals', 'decoder', 'head')


def stage_taps(case, stages):
    return tuple(n for n in case.ratio_taps() if STAGE[n] in stages)


# ---- model and weights ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _template(head, K, Q, N):
    """(never-run fp32 CPU bbox_head in eval mode, its state dict under the `bbox_head.` prefix)."""
    from pavenet_amd.models import build_model, petr_r50_cfg
    from tests.test_model_gpu import _seed
    m = _seed(build_model(petr_r50_cfg(num_keypoints=K, num_query=Q, max_per_img=N, head=HEAD_TYPES[head]))).eval()
    sd = {k: v.detach().clone() for k, v in m.state_dict().items() if k.startswith('bbox_head.')}
    return m.bbox_head, sd


def new_head(case):
    """A fresh head: a module that has run carries derived caches (split planes, geometry constants)."""
    return copy.deepcopy(_template(case.head, case.K, case.Q, case.N)[0])


def state_dict(case, dtype=torch.float32):
    sd = _template(case.head, case.K, case.Q, case.N)[1]
    return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}


# ---- inputs -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _flat(case, which=None):
    """fp32 [B, S, 256], token-major: the one buffer both input forms are views / copies of.  which: the case's own
    features (default) or, under another name, the features of a second forward that has no reference."""
    return torch.from_numpy(seeded_array(f'petr.{case.name}.{which or case.seed}', (case.B, case.S, C)))


def feats(case, form='nchw', device='cpu', which=None):
    """-> (list of four [B, 256, h, w] fp32 tensors on `device`, the tensors to check for bit-equality afterwards).
    'flat': consecutive slices of one token-major buffer;  'nchw': four separate dense NCHW tensors."""
    flat = _flat(case, which).to(device).clone()
    if form == 'flat':
        return _views(flat, case.levels), [flat]
    assert form == 'nchw'
    lv = [v.contiguous() for v in _views(flat, case.levels)]
    return lv, lv


# ---- the oracle, one image --------------------------------------------------------------------------------------
FAULTS = ('query_plus_memory_rows', 'refine_geometry_of_image0', 'kpt_score_is_p')


def _image_run(case, b, dtype, force=None, sd=None, fault=None):
    """The oracle on image `b` of `case` in `dtype` -> dict of taps (batch dim 1) + the selections it took.
    force: (topk_idx [1, Q], score_topk_idx [N]) to follow;  sd: a (perturbed) state dict;  fault: one of FAULTS."""
    assert fault is None or fault in FAULTS
    K, Q, N = case.K, case.Q, case.N
    sd = state_dict(case, dtype) if sd is None else sd
    hpre, tpre = 'bbox_head', 'bbox_head.transformer'
    img_shape = case.img_shapes[b]
    fs = [v.contiguous().to(dtype) for v in _views(_flat(case)[b:b + 1], case.levels)]
    masks, poss = R.make_masks_and_pos(fs, case.canvas, img_shape)
    poss = [p.to(dtype) for p in poss]
    # PETRTransformer.forward OT:4448-4636
    feat_f, mask_f, pos_f, shapes, lsi, valid_ratios = R.flatten_levels(sd, tpre, fs, masks, poss)
    reference_points = R.get_reference_points(shapes, valid_ratios)
    taps = {}
    memory = R.encoder_forward(sd, tpre + '.encoder', N_ENC, feat_f.permute(1, 0, 2), pos_f.permute(1, 0, 2), mask_f,
                               reference_points, shapes, lsi, taps=taps).permute(1, 0, 2)       # [1, S, C]
    out = {f'mem{i}': m.permute(1, 0, 2) for i, m in enumerate(taps['memory_layers'])}
    output_memory, output_proposals = R.gen_encoder_output_proposals(sd, tpre, memory, mask_f, shapes)
    enc_cls = R.linear(sd, f'{hpre}.cls_branches.{N_DEC}', output_memory)
    enc_kpt = R.kpt_branch(sd, f'{hpre}.kpt_branches.{N_DEC}', output_memory)
    enc_kpt[..., 0::2] += output_proposals[..., 0:1]
    enc_kpt[..., 1::2] += output_proposals[..., 1:2]
    out['enc_cls'] = enc_cls
    sel = dict(topk_idx=torch.topk(enc_cls[..., 0], Q, dim=1)[1], enc_logits=enc_cls[0, :, 0])
    topk_idx = sel['topk_idx'] if force is None else force[0]
    topk_kpts = torch.gather(enc_kpt, 1, topk_idx.unsqueeze(-1).repeat(1, 1, enc_kpt.size(-1)))
    reference_points = topk_kpts.sigmoid()
    init_reference = reference_points
    out['init_reference'] = init_reference
    query_pos, query = torch.split(sd[hpre + '.query_embedding.weight'], C, dim=1)
    query_pos = query_pos.unsqueeze(0).permute(1, 0, 2)
    x = query.unsqueeze(0)                                               # no memory rows added (OT:4596)
    if fault == 'query_plus_memory_rows':                                # (what the video transformer does, OT:21376)
        x = x + torch.gather(output_memory, 1, topk_idx.unsqueeze(-1).repeat(1, 1, C))
    x = x.permute(1, 0, 2)
    value = memory.permute(1, 0, 2)
    # PetrTransformerDecoder OT:4148-4231
    hs, refs = [], []
    for lid in range(N_DEC):
        lp = f'{tpre}.decoder.layers.{lid}'
        ref_in = reference_points[:, :, None] * valid_ratios.repeat(1, 1, K)[:, None]
        x = R.mha(sd, lp + '.attentions.0', x, query_pos)
        x = R.layer_norm(sd, lp + '.norms.0', x)
        x = R.pose_attn_single(sd, lp + '.attentions.1', x, value, query_pos, mask_f, ref_in, shapes, lsi, K=K)
        x = R.layer_norm(sd, lp + '.norms.1', x)
        x = R.ffn(sd, lp + '.ffns.0', x)
        x = R.layer_norm(sd, lp + '.norms.2', x)
        tmp = R.kpt_branch(sd, f'{hpre}.kpt_branches.{lid}', x.permute(1, 0, 2))
        reference_points = (tmp + R.inverse_sigmoid(reference_points)).sigmoid()
        hs.append(x.permute(1, 0, 2))
        refs.append(reference_points)
    # PETRHead.forward petr_head.py:213-300: every level
    for lvl in range(N_DEC):
        reference = init_reference if lvl == 0 else refs[lvl - 1]
        out[f'hs{lvl}'], out[f'ref{lvl}'] = hs[lvl], refs[lvl]
        out[f'cls{lvl}'] = R.linear(sd, f'{hpre}.cls_branches.{lvl}', hs[lvl])
        out[f'kpt{lvl}'] = (R.kpt_branch(sd, f'{hpre}.kpt_branches.{lvl}', hs[lvl])
                            + R.inverse_sigmoid(reference)).sigmoid()
    # _get_bboxes_single petr_head.py:956-1037 / vedpose_head_v2.py:1066-1180
    cls_score = out[f'cls{N_DEC - 1}'][0].sigmoid().view(-1)
    scores, indexs = cls_score.topk(N)
    sel['score_topk_idx'], sel['scores_all'] = indexs, cls_score
    if force is not None:
        indexs = force[1]
        scores = cls_score[indexs]
    kpt_pred = out[f'kpt{N_DEC - 1}'][0][indexs]                         # [N, 2K]
    sel['ref_pose'] = kpt_pred
    # forward_refine OT:4638-4693 + DeformableDetrTransformerDecoder MT:705-791 (memory replicated per pose)
    img_inds = torch.zeros(N, dtype=torch.int64)
    rq = sd[tpre + '.refine_query_embedding.weight']
    rpos, rquery = torch.split(rq, rq.size(1) // 2, dim=1)
    rpos = rpos.unsqueeze(0).expand(N, -1, -1).permute(1, 0, 2)
    rx = rquery.unsqueeze(0).expand(N, -1, -1).permute(1, 0, 2)
    rref = kpt_pred.reshape(N, K, 2)
    pos_memory = value[:, img_inds, :]
    rmask_src, rvr_src = mask_f, valid_ratios
    if fault == 'refine_geometry_of_image0':                             # valid_ratios[0] / mask[0] for every pose
        masks0, _ = R.make_masks_and_pos(fs, case.canvas, case.img_shapes[0])
        rmask_src = torch.cat([m.flatten(1) for m in masks0], 1)
        rvr_src = torch.stack([R.get_valid_ratio(m) for m in masks0], 1)
    rmask, rvr = rmask_src[img_inds, :], rvr_src[img_inds, ...]
    rinit, rhs, rrefs = rref, [], []
    for lid in range(N_REF):
        lp = f'{tpre}.refine_decoder.layers.{lid}'
        ref_in = rref[:, :, None] * rvr[:, None]
        rx = R.mha(sd, lp + '.attentions.0', rx, rpos)
        rx = R.layer_norm(sd, lp + '.norms.0', rx)
        rx = R.msda_module(sd, lp + '.attentions.1', rx, rpos, rmask, ref_in, shapes, lsi, value=pos_memory)
        rx = R.layer_norm(sd, lp + '.norms.1', rx)
        rx = R.ffn(sd, lp + '.ffns.0', rx)
        rx = R.layer_norm(sd, lp + '.norms.2', rx)
        tmp = R.refine_kpt_branch(sd, f'{hpre}.refine_kpt_branches.{lid}', rx.permute(1, 0, 2))
        rref = (tmp + R.inverse_sigmoid(rref)).sigmoid()
        rhs.append(rx.permute(1, 0, 2))                                  # [N, K, C]
        rrefs.append(rref)
    rl = N_REF - 1
    reference = R.inverse_sigmoid(rinit if rl == 0 else rrefs[rl - 1])
    kp = (R.refine_kpt_branch(sd, f'{hpre}.refine_kpt_branches.{rl}', rhs[rl]) + reference).sigmoid()
    for i in range(N_REF):
        out[f'refine_hs{i}'] = rhs[i]
    out['refine_kpts'] = kp[None]                                        # [1, N, K, 2]
    wh = torch.tensor([img_shape[1], img_shape[0]], dtype=kp.dtype)
    px = torch.minimum((kp * wh).clamp(min=0), wh)
    p5 = None
    if case.vedpose:
        sg = R.sigma_branch(sd, f'{hpre}.refine_fc_sigma_branches.{rl}', rhs[rl]).sigmoid()
        out['refine_sigma'] = sg[None]
        p = R.get_p(sg)
        p5 = p**5
        out['det_kpt_scores'] = (p if fault == 'kpt_score_is_p' else scores[:, None, None] * p)[None]
    else:
        out['det_kpt_scores'] = px.new_ones((1, N, K, 1))

    def result(px):
        box = torch.stack([px[..., 0].min(1)[0], px[..., 1].min(1)[0], px[..., 0].max(1)[0], px[..., 1].max(1)[0],
                           scores], -1)
        if p5 is not None:
            px = (px * p5) / (p5 + 1e-10)
        return px[None], box[None]
    out['det_kpts'], out['det_bboxes'] = result(px)
    if case.scale_factors:                                               # rescale=True: the pixels / the factors
        out['det_kpts_rescaled'], out['det_bboxes_rescaled'] = result(
            px / torch.tensor(case.scale_factors[b], dtype=kp.dtype))
    out['det_labels'] = (indexs % 1)[None]
    out['keep'] = torch.ones((1, N), dtype=torch.int32)
    out['order'] = torch.arange(N, dtype=torch.int32)[None]
    return out, sel


def _join(runs):
    """Per-image tap dicts -> the batch's: concatenated along dim 0."""
    return {k: torch.cat([r[k] for r in runs], 0).contiguous() for k in runs[0]}


@functools.lru_cache(maxsize=None)
def _reference_runs(case):
    with torch.no_grad():
        return tuple(_image_run(case, b, torch.float64) for b in range(case.B))


@functools.lru_cache(maxsize=None)
def reference(case):
    """fp64 taps of the whole batch (see TAPS, RESCALED_TAPS, EXACT_TAPS)."""
    return _join([r[0] for r in _reference_runs(case)])


@functools.lru_cache(maxsize=None)
def selections(case):
    """The fp64 run's discrete choices and what the isolated stages start from:  topk_idx [B, Q], score_topk_idx
    [B, N], enc_logits [B, S], scores_all [B, Q] (fp64, for _assert_same_selection), ref_pose [B*N, 2K] (fp64)."""
    sels = [r[1] for r in _reference_runs(case)]
    return dict(topk_idx=torch.cat([s['topk_idx'] for s in sels], 0),
                score_topk_idx=torch.stack([s['score_topk_idx'] for s in sels], 0),
                enc_logits=torch.stack([s['enc_logits'] for s in sels], 0),
                scores_all=torch.stack([s['scores_all'] for s in sels], 0),
                ref_pose=torch.cat([s['ref_pose'] for s in sels], 0))


def _forced(case, b):
    s = _reference_runs(case)[b][1]
    return s['topk_idx'], s['score_topk_idx']


def oracle_fp32(case, sd=None, fault=None):
    """The oracle's fp32 run of the batch with the fp64 run's selections forced (sd / fault: a sensitivity fault)."""
    with torch.no_grad():
        return _join([_image_run(case, b, torch.float32, force=_forced(case, b), sd=sd, fault=fault)[0]
                      for b in range(case.B)])


@functools.lru_cache(maxsize=None)
def oracle_fp32_free(case):
    """The oracle's fp32 run with NO forced selection -> its own (topk_idx [B, Q], score_topk_idx [B, N])."""
    with torch.no_grad():
        runs = [_image_run(case, b, torch.float32) for b in range(case.B)]
    return (torch.cat([r[1]['topk_idx'] for r in runs], 0), torch.stack([r[1]['score_topk_idx'] for r in runs], 0))


def errors(got, case, names=None):
    """{tap: rel_err(got[tap], reference[tap])} for the ratio taps of the case (or `names`)."""
    ref = reference(case)
    return {n: rel_err(got[n], ref[n]) for n in (names or case.ratio_taps())}


def exact_mismatches(got, case):
    """The taps whose reference leaves no room for error and that `got` does not reproduce bit for bit."""
    ref = reference(case)
    names = EXACT_TAPS + (() if case.vedpose else ('det_kpt_scores',))
    bad = []
    for n in names:
        g, r = got[n].detach().cpu(), ref[n]
        if tuple(g.shape) != tuple(r.shape) or not torch.equal(g.to(r.dtype), r):
            bad.append(n)
    return bad


@functools.lru_cache(maxsize=None)
def floor(case):
    """{tap: e_cpu32} of the ratio taps."""
    got = oracle_fp32(case)
    assert exact_mismatches(got, case) == []
    return errors(got, case)


def selection_tols(case):
    """head_cases.selection_tols's rule: MARGIN x floor x rms of the compared values -- what the bound allows a
    compared value to be off by (the scores are sigmoids of the last level's logits: |d sigmoid| <= |d logit| / 4,
    taken as 1 x)."""
    fl, ref = floor(case), reference(case)
    rms = lambda t: float(t.double().pow(2).mean().sqrt())      # noqa: E731
    last = f'cls{N_DEC - 1}'
    return MARGIN * fl['enc_cls'] * rms(ref['enc_cls']), MARGIN * fl[last] * rms(ref[last]), selections(case)


# ---- the package's modules: run + taps ---------------------------------------------------------------------------
def head_taps(case, outs, res=None, gtaps=None, store=None, res_scaled=None):
    """The package's outputs under the names of the taps.  outs: bbox_head.forward's dict;  res / gtaps: get_bboxes'
    result and its `taps` dict;  store: what memory_hooks collected;  res_scaled: get_bboxes(rescale=True)'s."""
    got = dict(store or {})
    got['enc_cls'] = outs['enc_cls_scores']
    got['init_reference'] = outs['init_reference']
    for i in range(N_DEC):
        got[f'hs{i}'] = outs['hs'][i]
        got[f'ref{i}'] = outs['inter_references'][i]
        got[f'cls{i}'] = outs['all_cls_scores'][i]
        got[f'kpt{i}'] = outs['all_kpt_preds'][i]
    if res is not None:
        got.update(refine_taps(case, gtaps['refine_hs'], gtaps['refine_kpts'], gtaps.get('refine_sigma')))
        got['det_kpts'] = res['kpts'][..., :2]
        got['det_kpt_scores'] = res['kpts'][..., 2:]
        got['det_bboxes'] = res['bboxes']
        got['det_labels'], got['keep'], got['order'] = res['labels'], res['keep'], res['order']
    if res_scaled is not None:
        got['det_kpts_rescaled'] = res_scaled['kpts'][..., :2]
        got['det_bboxes_rescaled'] = res_scaled['bboxes']
    return got


def refine_taps(case, r_hs, kpts, sigma=None):
    got = {f'refine_hs{i}': r_hs[i] for i in range(N_REF)}
    got['refine_kpts'] = kpts.reshape(case.B, case.N, case.K, 2)
    if sigma is not None:
        got['refine_sigma'] = sigma.reshape(case.B, case.N, case.K, 2)
    return got


def run_head(case, head, fs, store=None, free=False):
    """bbox_head.forward + get_bboxes from the features with the fp64 run's selections forced (free=True: none
    forced) -> (taps dict, outs, res)."""
    sel = selections(case)
    dev = fs[0].device
    kw, force_score = {}, None
    if not free:
        kw['force_topk_proposals'] = sel['topk_idx'].to(dev)
        force_score = sel['score_topk_idx'].to(dev)
    store = {} if store is None else store
    gtaps = {}
    with memory_hooks(head, store):
        outs = head(fs, case.metas(), **kw)
    res = head.get_bboxes(outs, case.metas(), rescale=False, force_score_topk=force_score, taps=gtaps)
    res_scaled = None
    if case.scale_factors:
        res_scaled = head.get_bboxes(outs, case.metas(scaled=True), rescale=True, force_score_topk=force_score)
    return head_taps(case, outs, res, gtaps, store, res_scaled), outs, res


# ---- sensitivity faults (injected into the oracle's fp32 run only) ------------------------------------------------
def perturbed_sd(case, key, factor=1 + 1e-3):
    sd = state_dict(case)
    assert key in sd, key
    sd[key] = sd[key] * factor
    return sd


@contextlib.contextmanager
def pose_attention_masks_before_projection():
    """The pose decoder's cross-attention with the padding mask applied BEFORE the value projection (the T-frame
    classes' convention, OT:1706-1707) instead of after it (OT:386-388): masked rows then hold the projection's bias,
    not 0."""
    real = R.pose_attn_single

    def faulty(sd, pre, query, value, query_pos, key_padding_mask, *a, **k):
        if key_padding_mask is not None:
            value = value.masked_fill(key_padding_mask.t()[..., None], 0.0)      # value [S, B, C], mask [B, S]
        return real(sd, pre, query, value, query_pos, None, *a, **k)
    R.pose_attn_single = faulty
    try:
        yield
    finally:
        R.pose_attn_single = real
