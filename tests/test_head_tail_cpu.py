"""The references and input generators of tests/test_head_tail_gpu.py, checked without a GPU: the OKS-NMS
restatement against the oracle where the oracle is defined, and the conditions the GPU tests rely on (no OKS on
the threshold, enough pairs near it, the special values really present) for every case and seed they use."""
import numpy as np
import pytest
import torch

from oracle import pavenet_ref as R
from tests import head_tail_ref as HT


def test_oks_sigmas_are_the_oracles():
    assert np.array_equal(HT.OKS_SIGMAS_15, R.OKS_SIGMAS_15)


@pytest.mark.parametrize('N,K,seed', [(40, 15, 0), (120, 15, 1), (60, 17, 2)])
def test_oks_nms_ref_equals_the_oracle_on_sorted_tie_free_scores(N, K, seed):
    """Descending, distinct scores leave the oracle's unstable argsort no choice: both must keep the same poses."""
    kpts, _ = HT.oks_inputs(N, K, seed)
    rng = np.random.default_rng(seed)
    sc = np.sort(rng.uniform(0.05, 1, N).astype(np.float32))[::-1].copy()
    assert len(np.unique(sc)) == N
    sig = HT.oks_sigmas(K)
    keep, order, gap = HT.oks_nms_ref(kpts, sc, HT.OKS_THRESH, sig)
    exp = R.oks_nms(torch.from_numpy(kpts), torch.from_numpy(sc), HT.OKS_THRESH, sig)
    assert order.tolist() == list(range(N))
    assert np.nonzero(keep)[0].tolist() == sorted(int(i) for i in exp)
    assert 0 < keep.sum() < N and gap > 0


def test_oks_nms_ref_orders_ties_larger_index_first_and_nan_as_inf():
    kpts, _ = HT.oks_inputs(8, 15, 0)
    sc = np.array([0.5, 0.9, 0.5, np.nan, 0.9, np.inf, 0.1, np.nan], np.float32)
    order = HT.oks_nms_ref(kpts, sc, HT.OKS_THRESH, HT.OKS_SIGMAS_15)[1]
    assert order.tolist() == [7, 5, 3, 4, 1, 2, 0, 6]


@pytest.mark.parametrize('ci', range(len(HT.OKS_CASES)), ids=['%dx%dx%d' % c for c in HT.OKS_CASES])
def test_oks_cases_keep_clear_of_the_threshold_and_crowd_it(ci):
    """Every clip of every GPU case: gap >= 1e-6 (what lets the GPU test ask for exact equality), scores unsorted
    with exact ties, and -- for N >= 257 -- more than 10 compared pairs within 0.05 of the threshold.  (K = 1 is
    exempt from the last: with one key point every area is 0, an OKS is exactly 0 or 1.)"""
    n_clips, N, K = HT.OKS_CASES[ci]
    kpts, sc, sig = HT.oks_case(ci)
    assert kpts.shape == (n_clips, N, K, 3) and kpts.dtype == np.float32 and sc.dtype == np.float32
    for b in range(n_clips):
        keep, order, gap = HT.oks_nms_ref(kpts[b], sc[b], HT.OKS_THRESH, sig)
        assert gap >= HT.OKS_GUARD
        assert sorted(order.tolist()) == list(range(N)) and order.tolist() != list(range(N))
        assert len(np.unique(sc[b])) < N - 4
        assert 0 < keep.sum() < N
        if N >= 257 and K > 1:
            assert HT.near_threshold_pairs(kpts[b], sc[b], HT.OKS_THRESH, sig) > 10
        if K == 1:
            assert keep.sum() == N - 10        # only the ten exact duplicates are suppressed
        if b:
            assert not np.array_equal(kpts[b], kpts[0])


def test_mha_large_logit_inputs_span_60_and_move_the_maximum_around():
    n_seq, L, H = HT.MHA_BIG
    qkv = HT.mha_big_logit_inputs()
    logits = HT.mha_logits(qkv, n_seq, L, H)
    assert 50 < float(logits.max()) < 80 and -80 < float(logits.min()) < -50
    top = logits.argmax(-1)
    assert len(set((top % 16).flatten().tolist())) == 16 and len(set((top // 16).flatten().tolist())) == 7
    exp = HT.mha_ref(qkv.double(), n_seq, L, H)
    err32 = float((HT.mha_ref(qkv, n_seq, L, H).double() - exp).abs().max())
    assert 0 < err32 < 1e-4          # the scale of the GPU test's bound: fp32 rounding of logits of ~60


@pytest.mark.parametrize('K', [1, 17, 64])
def test_pose_finalize_inputs_hold_the_special_values(K):
    kp, sg, sc, wh, sf = HT.pose_finalize_inputs(K, 40 + K)
    for val in (0.0, 1.0):
        assert bool((kp == val).any()) and bool((sg == val).any())
    assert bool((kp < 0).any()) and bool((kp > 1).any())
    for val in (1e-6, 0.02, 0.5):
        assert bool((sg == val).any())
    ek, eb = HT.pose_finalize_ref(kp, sg, sc, wh, sf)
    assert bool(torch.isfinite(ek).all()) and bool(torch.isfinite(eb).all())
