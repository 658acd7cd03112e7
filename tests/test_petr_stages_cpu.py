"""What tests/test_petr_stages_gpu.py stands on, checked without a GPU (cases, references: tests/petr_cases.py):

1. the floors e_cpu32 of every case and ratio tap are finite, positive and no more than twice the values recorded below.
   A floor is the largest error of ONE fp32 run, and over a tap of 50 .. 300 numbers it moves with the host's BLAS
   paths: measured on the development host and on the CPU of the MI355X host, the two differ by up to 4.5 x
   (p5's det_bboxes, 1.11e-6 and 4.98e-6) in either direction.  Recorded is the larger of the two per tap;
2. without forcing, the oracle's fp32 and fp64 runs of p1 take the same proposals and the same scores;
3. the package's OWN modules, run on the CPU in fp32 through bbox_head.forward + get_bboxes with the fp64 run's
   selections forced, meet the GPU file's bound  e <= 8 * e_cpu32  on every tap, for both input forms and all six
   cases, and reproduce the exact taps bit for bit: what fails here is module logic, what fails only on the device is
   a kernel or a device fast path.  The one primitive the package has on the device alone -- the deformable-attention
   sampler -- is the oracle's here;
4. sensitivity: seven faults, each injected into the ORACLE's fp32 run only, each put a named tap above the bound;
   the measured multiple of the floor stands beside each;
5. petr_r50_cfg(num_query=Q) reaches the transformer, for both heads.

Sensitivity as measured on the development host (e / e_cpu32 at the named tap; the bound is 8).  No fault stays inside:
    decoder.layers.1.norms.1.bias x (1 + 1e-3), p1                  hs1             36 x   (later taps 13 .. 50 x)
    refine_kpt_branches.0.4.bias x (1 + 1e-3), p1                   det_kpts        15 x   (refine_hs1 11 x; on the
                                                                    MI355X host's CPU: det_kpts 11 x, refine_hs1 9.6 x)
    encoder.layers.3.ffns.0.layers.1.bias x (1 + 1e-3), p1          mem3            28 x   (later taps 21 .. 52 x)
    padding mask BEFORE the pose attention's value projection, p2   hs0           4990 x
    the proposals' memory rows added to the query, p1               hs0         681688 x
    refine valid ratios and mask of image 0 for every pose, p2      refine_hs0   56578 x
    the same, p4                                                    refine_hs0  124817 x
    VedPose key-point score p in place of scores * p, p3            det_kpt_scores 1.98e6 x
The taps before each fault stay at or below 2 x (asserted).
"""
import numpy as np
import pytest
import torch

from oracle import pavenet_ref as R
from tests import petr_cases as PC

# e_cpu32 per case and tap as measured (per tap the larger of two hosts); asserted 0 < e <= FLOOR_CAP * these
FLOOR_CAP = 2
FLOORS = {
    'p1_petr_128x160_B1': dict(
        mem0=4.44e-06, mem1=4.12e-06, mem2=4.92e-06, mem3=5.25e-06,
        mem4=5.58e-06, mem5=4.96e-06, enc_cls=6.43e-06, init_reference=1.18e-06,
        hs0=5.47e-06, hs1=8.14e-06, hs2=9.33e-06, ref0=1.41e-06,
        ref1=2.27e-06, ref2=2.87e-06, cls0=3.51e-06, cls1=4.12e-06,
        cls2=3.79e-06, kpt0=1.41e-06, kpt1=2.27e-06, kpt2=2.87e-06,
        refine_hs0=8.15e-06, refine_hs1=9.62e-06, refine_kpts=2.52e-06, det_kpts=2.25e-06,
        det_bboxes=1.85e-06,
    ),
    'p2_petr_128x160_B2_padded': dict(
        mem0=3.35e-06, mem1=5.18e-06, mem2=6.30e-06, mem3=5.00e-06,
        mem4=5.51e-06, mem5=6.72e-06, enc_cls=6.42e-06, init_reference=1.07e-06,
        hs0=5.46e-06, hs1=1.19e-05, hs2=1.27e-05, ref0=1.69e-06,
        ref1=3.04e-06, ref2=2.95e-06, cls0=4.11e-06, cls1=6.30e-06,
        cls2=4.29e-06, kpt0=1.69e-06, kpt1=3.04e-06, kpt2=2.95e-06,
        refine_hs0=9.45e-06, refine_hs1=1.00e-05, refine_kpts=2.63e-06, det_kpts=2.81e-06,
        det_bboxes=2.86e-06, det_kpts_rescaled=3.19e-06, det_bboxes_rescaled=2.07e-06,
    ),
    'p3_vedpose_75x133_B1': dict(
        mem0=3.11e-06, mem1=4.91e-06, mem2=4.84e-06, mem3=4.54e-06,
        mem4=4.55e-06, mem5=5.26e-06, enc_cls=7.50e-06, init_reference=9.40e-07,
        hs0=5.44e-06, hs1=6.65e-06, hs2=5.89e-06, ref0=1.47e-06,
        ref1=1.80e-06, ref2=2.99e-06, cls0=3.74e-06, cls1=2.94e-06,
        cls2=2.90e-06, kpt0=1.47e-06, kpt1=1.80e-06, kpt2=2.99e-06,
        refine_hs0=8.31e-06, refine_hs1=8.13e-06, refine_kpts=2.28e-06, refine_sigma=1.11e-05,
        det_kpts=2.36e-06, det_kpt_scores=1.63e-05, det_bboxes=2.63e-06,
    ),
    'p4_vedpose_64x96_B3_padded': dict(
        mem0=2.79e-06, mem1=4.03e-06, mem2=4.27e-06, mem3=4.80e-06,
        mem4=6.95e-06, mem5=6.72e-06, enc_cls=5.47e-06, init_reference=1.04e-06,
        hs0=5.90e-06, hs1=6.21e-06, hs2=6.07e-06, ref0=1.23e-06,
        ref1=1.84e-06, ref2=1.91e-06, cls0=3.29e-06, cls1=2.88e-06,
        cls2=3.41e-06, kpt0=1.23e-06, kpt1=1.84e-06, kpt2=1.91e-06,
        refine_hs0=7.45e-06, refine_hs1=9.52e-06, refine_kpts=2.92e-06, refine_sigma=1.16e-05,
        det_kpts=3.68e-06, det_kpt_scores=2.44e-05, det_bboxes=3.03e-06,
    ),
    'p5_petr_64x416_B1': dict(
        mem0=4.39e-06, mem1=6.11e-06, mem2=1.05e-05, mem3=6.77e-06,
        mem4=6.19e-06, mem5=6.96e-06, enc_cls=5.37e-06, init_reference=1.31e-06,
        hs0=1.45e-05, hs1=1.22e-05, hs2=1.65e-05, ref0=2.92e-06,
        ref1=3.07e-06, ref2=4.66e-06, cls0=1.12e-05, cls1=7.88e-06,
        cls2=5.83e-06, kpt0=2.92e-06, kpt1=3.07e-06, kpt2=4.66e-06,
        refine_hs0=2.60e-05, refine_hs1=2.44e-05, refine_kpts=4.49e-06, det_kpts=5.49e-06,
        det_bboxes=4.98e-06,
    ),
    'p6_first_petr_128x160_B2': dict(
        mem0=3.25e-06, mem1=4.99e-06, mem2=4.46e-06, mem3=6.95e-06,
        mem4=6.46e-06, mem5=6.90e-06, enc_cls=5.77e-06, init_reference=1.22e-06,
        hs0=6.47e-06, hs1=7.17e-06, hs2=9.22e-06, ref0=1.68e-06,
        ref1=2.21e-06, ref2=2.78e-06, cls0=4.39e-06, cls1=6.36e-06,
        cls2=4.12e-06, kpt0=1.68e-06, kpt1=2.21e-06, kpt2=2.78e-06,
        refine_hs0=9.70e-06, refine_hs1=1.05e-05, refine_kpts=2.86e-06, det_kpts=2.60e-06,
        det_bboxes=1.67e-06,
    ),
}


CASE_IDS = [c.name for c in PC.ALL_CASES]


@pytest.mark.parametrize('case', PC.ALL_CASES, ids=CASE_IDS)
def test_floors(case):
    fl = PC.floor(case)
    names = case.ratio_taps()
    print(f'{case}: e_cpu32 = ' + ' '.join(f'{n}={fl[n]:.2e}' for n in names))
    assert set(FLOORS[case.name]) == set(names) == set(fl)
    for n in names:
        assert np.isfinite(fl[n]) and 0 < fl[n] <= FLOOR_CAP * FLOORS[case.name][n], (case, n, fl[n])


def test_p1_free_selections_are_equal():
    """No near-tie at either selection boundary of p1: the un-forced fp32 run picks what the fp64 run picks (a case
    that fails this gets another seed, not an allowance)."""
    topk, score = PC.oracle_fp32_free(PC.P1)
    sel = PC.selections(PC.P1)
    assert torch.equal(topk.sort(1)[0], sel['topk_idx'].sort(1)[0])
    assert torch.equal(score, sel['score_topk_idx'])


def test_the_cases_reach_what_they_are_for():
    """The exact taps of the reference are the constants they are compared as; p5's un-padded image has invalid
    border proposals (a level more than 50 wide) and p1, p3, p4 have none."""
    for case in PC.ALL_CASES:
        ref = PC.reference(case)
        assert bool((ref['det_labels'] == 0).all()) and bool((ref['keep'] == 1).all())
        assert torch.equal(ref['order'], torch.arange(case.N, dtype=torch.int32).expand(case.B, case.N))
        if not case.vedpose:
            assert bool((ref['det_kpt_scores'] == 1).all())
        assert bool(torch.isfinite(ref['init_reference']).all())
    w0 = PC.P5.levels[0][1]
    assert 0.5 / w0 < 0.01                      # the first and last column of level 0 are invalid (OT:21200)
    assert all(0.5 / max(h, w) >= 0.01 for c in (PC.P1, PC.P3, PC.P4) for h, w in c.levels)


# ---- the package's modules on the CPU -----------------------------------------------------------------------------
@pytest.fixture
def cpu_sampler(monkeypatch):
    from pavenet_amd import ops
    monkeypatch.setattr(ops, 'ms_deform_attn_forward',
                        lambda v, shapes, lsi, loc, aw, im2col_step=64: R.msda(v, shapes, lsi, loc, aw))


def _assert_bound(what, case, got, names=None):
    names = tuple(names or case.ratio_taps())
    r = PC.ratios(PC.errors(got, case, names), PC.floor(case))
    print(PC.fmt(what, r))
    assert set(r) == set(names)
    for n, v in r.items():
        assert v <= PC.MARGIN, f'{what}: {n}: {v:.2f} x e_cpu32'
    return r


@pytest.mark.parametrize('form', ['nchw', 'flat'])
@pytest.mark.parametrize('case', PC.CASES, ids=[c.name for c in PC.CASES])
def test_modules_on_cpu_meet_the_bound(cpu_sampler, case, form):
    head = PC.new_head(case)
    fs, keep_in = PC.feats(case, form)
    before = [t.clone() for t in keep_in]
    with torch.no_grad():
        got, _, _ = PC.run_head(case, head, fs)
    for t, k in zip(keep_in, before):
        assert torch.equal(t, k), 'the forward wrote into its input'
    _assert_bound(f'cpu modules {case} {form}', case, got)
    assert PC.exact_mismatches(got, case) == []


@pytest.mark.parametrize('form', ['nchw', 'flat'])
def test_p6_first_then_p2_on_the_same_module_on_cpu(cpu_sampler, form):
    """p2 as the SECOND forward of a module whose first forward saw other img_shapes, each against its own
    reference (p6_first is the sixth case of the module test above)."""
    head = PC.new_head(PC.P2)
    f1, in1 = PC.feats(PC.P6_FIRST, form)
    f2, in2 = PC.feats(PC.P2, form)
    before = [t.clone() for t in in1 + in2]
    with torch.no_grad():
        first, _, _ = PC.run_head(PC.P6_FIRST, head, f1)
        second, _, _ = PC.run_head(PC.P2, head, f2)
    for t, k in zip(in1 + in2, before):
        assert torch.equal(t, k), 'the forward wrote into its input'
    _assert_bound(f'cpu modules p6_first {form}', PC.P6_FIRST, first)
    _assert_bound(f'cpu modules p2 after p6_first {form}', PC.P2, second)
    assert PC.exact_mismatches(first, PC.P6_FIRST) == [] and PC.exact_mismatches(second, PC.P2) == []


@pytest.mark.parametrize('head', ['petr', 'vedpose'])
@pytest.mark.parametrize('Q', [100, 300])
def test_num_query_reaches_the_transformer(head, Q):
    """petr_r50_cfg(num_query=Q): the transformer takes Q proposals, one per query embedding row (it kept its default
    of 300 whatever Q was; p3, p4 and p5 could not run)."""
    from pavenet_amd.models import build_model, petr_r50_cfg
    h = build_model(petr_r50_cfg(num_keypoints=15, num_query=Q, head=PC.HEAD_TYPES[head])).bbox_head
    assert h.transformer.two_stage_num_proposals == Q == h.query_embedding.num_embeddings == h.num_query


# ---- sensitivity --------------------------------------------------------------------------------------------------
def _assert_trips(what, case, got, tap, quiet=()):
    r = PC.ratios(PC.errors(got, case), PC.floor(case))
    print(PC.fmt(what, {n: v for n, v in r.items() if v > PC.MARGIN}))
    assert r[tap] > PC.MARGIN, f'{what}: {tap} stays at {r[tap]:.2f} x e_cpu32: the case set is too weak'
    for n in quiet:                      # the taps before the fault do not move
        assert r[n] <= 2.0, (what, n, r[n])
    return r


@pytest.mark.parametrize('key,tap,quiet', [
    ('bbox_head.transformer.decoder.layers.1.norms.1.bias', 'hs1', ('mem5', 'enc_cls', 'hs0', 'ref0')),
    # (the refine decoder's reference after layer 0 is not a tap of its own: the fault shows in layer 1's hidden state
    # and, with the widest margin on both hosts measured, in the final key points)
    ('bbox_head.refine_kpt_branches.0.4.bias', 'det_kpts', ('hs2', 'kpt2', 'refine_hs0')),
    ('bbox_head.transformer.encoder.layers.3.ffns.0.layers.1.bias', 'mem3', ('mem0', 'mem1', 'mem2')),
])
def test_one_bias_off_by_a_thousandth_trips_the_bound(key, tap, quiet):
    """One fp32 bias x (1 + 1e-3): the named tap leaves the bound, the taps before the parameter do not move."""
    _assert_trips(key, PC.P1, PC.oracle_fp32(PC.P1, sd=PC.perturbed_sd(PC.P1, key)), tap, quiet)


def test_mask_before_the_pose_value_projection_trips_the_bound():
    with PC.pose_attention_masks_before_projection():
        got = PC.oracle_fp32(PC.P2)
    _assert_trips('padding mask before the value projection', PC.P2, got, 'hs0', ('mem5', 'enc_cls', 'init_reference'))
    assert R.pose_attn_single.__name__ == 'pose_attn_single'


def test_memory_rows_added_to_the_query_trip_the_bound():
    _assert_trips('query + the proposals\' memory rows', PC.P1, PC.oracle_fp32(PC.P1, fault='query_plus_memory_rows'),
                  'hs0', ('mem5', 'enc_cls', 'init_reference'))


@pytest.mark.parametrize('case', [PC.P2, PC.P4], ids=[PC.P2.name, PC.P4.name])
def test_refine_geometry_of_image0_for_every_pose_trips_the_bound(case):
    _assert_trips('refine valid ratios / mask of image 0', case,
                  PC.oracle_fp32(case, fault='refine_geometry_of_image0'), 'refine_hs0', ('hs2', f'kpt{PC.N_DEC - 1}'))


def test_vedpose_keypoint_score_without_the_pose_score_trips_the_bound():
    _assert_trips('key-point score p instead of scores * p', PC.P3, PC.oracle_fp32(PC.P3, fault='kpt_score_is_p'),
                  'det_kpt_scores', ('refine_sigma', 'det_kpts', 'det_bboxes'))
