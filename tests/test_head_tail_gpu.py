"""The head's tail between the decoder and the result (pave_oks_nms_f32, pave_topk_rows_f32, pave_mha_core_f32,
pave_pose_finalize_f32, pave_gather_frame_poses_f32) at the sizes and values where each kernel takes another
branch: the staged / unstaged OKS paths and their 256-strided loops, unsorted tied scores, both NaN sign patterns
and signed zeros in the top-k, the L thresholds of the attention core's dispatch and a softmax whose running
maximum is overtaken by large steps, K = 1 / 64 and saturated sigmas in the post-processing, indices outside
[0, Q) in the gather.  References and input generators: tests/head_tail_ref.py (checked without a GPU by
tests/test_head_tail_cpu.py).  Needs an MI355X."""
import numpy as np
import pytest
import torch

from tests import head_tail_ref as HT

pytestmark = pytest.mark.gpu


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


# ---------------------------------------------------------------------------
# OKS-NMS
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('ci', range(len(HT.OKS_CASES)), ids=['%dx%dx%d' % c for c in HT.OKS_CASES])
def test_oks_nms_vs_reference(ci):
    """keep and order of pave_oks_nms_f32 equal head_tail_ref.oks_nms_ref exactly, on unsorted scores with exact
    ties, at N on both sides of the staging limit (K = 15: staged up to N = 371), past one trip of the 256-strided
    loops, and at K = 1, 17, 64; every clip of a launch has its own inputs.

    Exact equality needs no pair's OKS to sit on the threshold, so the reference's `gap` (smallest |OKS - thresh|
    over the pairs it compared) must be >= 1e-6.  Why 1e-6: the kernel may contract dx*dx + dy*dy into an fma where
    NumPy does not, which moves d^2 by at most one fp32 ulp (1.2e-7 relative) and one key point's exp(-e) by at most
    e exp(-e) 1.2e-7 <= 4.5e-8; every other operation is the same in both.  The guard is 20 x that."""
    from pavenet_amd.ops import oks_nms
    n_clips, N, K = HT.OKS_CASES[ci]
    kpts, sc, sig = HT.oks_case(ci)
    refs = [HT.oks_nms_ref(kpts[b], sc[b], HT.OKS_THRESH, sig) for b in range(n_clips)]
    for keep, order, gap in refs:
        assert gap >= HT.OKS_GUARD
    keep, order = oks_nms(_t(kpts).cuda(), _t(sc).cuda(), _t(sig).cuda(), HT.OKS_THRESH)
    keep, order = keep.cpu().numpy(), order.cpu().numpy()
    for b, (ekeep, eorder, gap) in enumerate(refs):
        assert np.array_equal(order[b], eorder), f'clip {b}: order'
        assert np.array_equal(keep[b] != 0, ekeep), f'clip {b}: keep'
        assert 0 < ekeep.sum() < N


def test_oks_nms_at_the_4096_pose_limit():
    """N = 4096 (the limit) of identical poses: every pair has OKS 1, so exactly the first pose in `order`
    survives; order is the reverse of a stable ascending sort of the (tied) scores.  N = 4097 is refused."""
    from pavenet_amd.ops import oks_nms
    rng = np.random.default_rng(4096)
    N, K = 4096, 15
    pose = rng.uniform(0, 400, (K, 3)).astype(np.float32)
    kpts = np.broadcast_to(pose, (2, N, K, 3)).copy()
    sc = rng.uniform(0.05, 1, (2, N)).astype(np.float32)
    sc[:, ::7] = sc[:, 3:4]
    sig = _t(HT.OKS_SIGMAS_15).cuda()
    keep, order = oks_nms(_t(kpts).cuda(), _t(sc).cuda(), sig, HT.OKS_THRESH)
    keep, order = keep.cpu().numpy(), order.cpu().numpy()
    for b in range(2):
        eorder = np.argsort(sc[b], kind='stable')[::-1]
        assert np.array_equal(order[b], eorder)
        assert keep[b].sum() == 1 and keep[b, eorder[0]] == 1
    with pytest.raises(RuntimeError):
        oks_nms(torch.zeros(1, N + 1, K, 3, device='cuda'), torch.zeros(1, N + 1, device='cuda'), sig, HT.OKS_THRESH)


# ---------------------------------------------------------------------------
# top-k
# ---------------------------------------------------------------------------
def _neg_nan():
    return torch.tensor([-4194304], dtype=torch.int32).view(torch.float32)[0]      # 0xffc00000: x86's inf - inf


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize('n,k', [(2000, 64), (300, 3), (9, 9)])
def test_topk_rows_nan_of_either_sign_ranks_first(n, k):
    """A row holding NaNs with the sign bit clear (float('nan')) and set (0xffc00000, what x86 makes for
    inf - inf), +-inf and finite values: every NaN ranks before +inf, NaNs among themselves by ascending index
    (k = 3 of 6 NaNs: the three lowest), then torch.topk's values of the rest."""
    from pavenet_amd.ops import topk_rows
    g = torch.Generator().manual_seed(n + k)
    x = torch.randn(3, n, generator=g)
    nan_at = [[5, 2, 8, 1, 7, 4], [0, 8, 3, 6, 7, 2], [8, 3]]       # alternately positive, negative
    for r, at in enumerate(nan_at):
        x[r, 0] = float('-inf')
        x[r, 6 - r] = float('inf')
        for a, i in enumerate(at):
            x[r, i] = _neg_nan() if a % 2 else float('nan')
    assert int((x.view(torch.int32) < 0).logical_and(x.isnan()).sum()) == 7
    v, i = topk_rows(x.cuda(), k)
    v, i = v.cpu(), i.cpu()
    ev = torch.topk(x, k, dim=1)[0]                   # torch puts a NaN of either sign first too
    for r, at in enumerate(nan_at):
        m = min(len(at), k)
        assert i[r, :m].tolist() == sorted(at)[:m]
        assert bool(v[r, :m].isnan().all()) and bool(ev[r, :m].isnan().all())
        assert torch.equal(v[r, m:], ev[r, m:]) and not bool(v[r, m:].isnan().any())
        assert len(set(i[r].tolist())) == k
    assert _same_bits(torch.gather(x, 1, i), v)


@pytest.mark.parametrize('n', [1500, 40])
def test_topk_rows_signed_zeros_are_equal_values(n):
    """Rows of negative values with five positive ones and 24 zeros of mixed sign, cut by k inside the zeros and
    after them: -0.0 == +0.0, so the zeros come out by ascending index whatever their sign and the zeros SELECTED
    at the k-th position are those with the lowest indices; the returned values keep the row's sign bits."""
    from pavenet_amd.ops import topk_rows
    g = torch.Generator().manual_seed(n)
    x = -torch.rand(4, n, generator=g) - 0.5
    pos, zeros = [], []
    for r in range(4):
        perm = torch.randperm(n, generator=g).tolist()
        pos.append(perm[:5])
        zeros.append(sorted(perm[5:29]))
        x[r, perm[:5]] = torch.tensor([5., 4., 3., 2., 1.])
        # the lowest-index zeros are negative in rows 0 and 1, alternate in row 2, random in row 3
        for a, i in enumerate(zeros[r]):
            neg = (a < 12) if r < 2 else (a % 2 == 0 if r == 2 else bool(torch.rand((), generator=g) < 0.5))
            x[r, i] = -0.0 if neg else 0.0
    assert int(((x == 0) & (x.view(torch.int32) < 0)).sum()) >= 30
    for k in (5 + 7, 5 + 24, 5 + 24 + 6):
        v, i = topk_rows(x.cuda(), k)
        v, i = v.cpu(), i.cpu()
        ev = torch.topk(x, k, dim=1)[0]
        assert bool((v == ev).all())
        for r in range(4):
            nz = min(24, k - 5)
            assert i[r, :5].tolist() == pos[r]
            assert i[r, 5:5 + nz].tolist() == zeros[r][:nz]
            assert len(set(i[r].tolist())) == k
        assert _same_bits(torch.gather(x, 1, i), v)


@pytest.mark.parametrize('n,k', [(1, 1), (1024, 1024), (1025, 1024), (32768, 1)])
def test_topk_rows_whole_row_and_single_winner(n, k):
    """k == n (the radix select ends on the smallest key: n = 1, n = 1024 = one element per thread) and the two
    extremes of the other dimension; with exact ties, so the order is (value descending, index ascending) of a
    full stable sort.  k == n at n = 1025 is past the k <= 1024 limit and must raise."""
    from pavenet_amd.ops import topk_rows
    g = torch.Generator().manual_seed(n * 3 + k)
    x = torch.randn(3, n, generator=g)
    if n > 1:
        x[:, ::5] = x[:, 1:2]
        x[1] = x[1].abs()
        x[2, n // 2:] = x[2, :n - n // 2].clone()
    v, i = topk_rows(x.cuda(), k)
    order = torch.sort(x, dim=1, descending=True, stable=True)[1][:, :k]
    assert torch.equal(i.cpu(), order)
    assert torch.equal(v.cpu(), torch.gather(x, 1, order)) and torch.equal(v.cpu(), torch.topk(x, k, dim=1)[0])
    if n == 1025:
        with pytest.raises(RuntimeError):
            topk_rows(x.cuda(), 1025)


def test_topk_rows_of_one_repeated_value_returns_the_first_indices():
    from pavenet_amd.ops import topk_rows
    x = torch.full((2, 5000), 0.25)
    x[1] = -3.0
    v, i = topk_rows(x.cuda(), 1024)
    assert torch.equal(i.cpu(), torch.arange(1024).expand(2, -1))
    assert torch.equal(v.cpu(), x[:, :1024])


# ---------------------------------------------------------------------------
# self-attention core
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('pad', [0, 64])
@pytest.mark.parametrize('n_seq,L,H', [(3, 16, 8), (3, 17, 8), (2, 64, 8), (2, 65, 8), (5, 5, 8), (1, 130, 1),
                                       (2, 40, 3)])
def test_mha_core_at_the_dispatch_thresholds_vs_fp64(n_seq, L, H, pad):
    """pave_mha_core_f32 on both sides of its two dispatch thresholds (L <= 16: one wave, four lanes per query;
    L <= 64: four waves; above: eight), at head counts other than 8, with a dense and a padded row; reference
    and tolerance of test_mha_core_vs_fp64."""
    from pavenet_amd.ops import mha_core
    E = H * 32
    g = torch.Generator().manual_seed(n_seq * 1000 + L * 10 + H)
    qkv = torch.randn(n_seq * L, 3 * E + pad, generator=g)
    qkv[:, :E] *= 1.5
    got = mha_core(qkv.cuda(), n_seq, L, H).cpu()
    exp = HT.mha_ref(qkv.double(), n_seq, L, H)
    assert tuple(got.shape) == (n_seq * L, E)
    np.testing.assert_allclose(got.numpy(), exp.numpy(), rtol=2e-5, atol=2e-6)


def test_mha_core_online_softmax_with_large_logit_steps():
    """(n_seq, L, H) = (2, 97, 8) with q scaled so that the logits have a standard deviation of 12 and span about
    +-60: a lane's running maximum is overtaken by steps of tens of units, early in some lanes and late in others
    (the largest-logit key of a query falls on every j mod 16 and every j // 16 over the queries).

    The bound is not fixed in advance: it is 4 x the largest absolute error of the plain fp32 formulation
    (torch.softmax(q k^T / sqrt(32)) v on the CPU) against the fp64 reference on the same inputs.  Measured on an
    MI355X: fp32 formulation 8.84e-6, kernel 1.02e-5 (1.15 x)."""
    from pavenet_amd.ops import mha_core
    n_seq, L, H = HT.MHA_BIG
    qkv = HT.mha_big_logit_inputs()
    logits = HT.mha_logits(qkv, n_seq, L, H)
    assert float(logits.max()) > 50 and float(logits.min()) < -50
    top = logits.argmax(-1)
    assert len(set((top % 16).flatten().tolist())) == 16 and len(set((top // 16).flatten().tolist())) == 7
    exp = HT.mha_ref(qkv.double(), n_seq, L, H)
    err32 = float((HT.mha_ref(qkv, n_seq, L, H).double() - exp).abs().max())
    got = mha_core(qkv.cuda(), n_seq, L, H).cpu().double()
    err = float((got - exp).abs().max())
    print(f'mha large logits: fp32 formulation {err32:.3e}, kernel {err:.3e}')
    assert bool(torch.isfinite(got).all())
    assert err <= 4 * err32


# ---------------------------------------------------------------------------
# pose post-processing and the selection gather
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('K', [1, 17, 64])
def test_pose_finalize_at_k_1_17_64_with_saturated_sigmas(K):
    """pave_pose_finalize_f32 at K = 64 (every lane active: no +-inf fillers in the min / max butterfly), K = 1
    and K = 17, with sigmas of exactly 0.0 and 1.0 (a saturated sigmoid), 1e-6, 0.02, 0.5 and random ones, key
    points of exactly 0 and 1, below 0 and above 1, with and without the scale factor, sigma rows of 2 and of 4
    floats; reference expressions and tolerances of test_gather_frame_poses_and_pose_finalize_vs_torch."""
    from pavenet_amd.ops import pose_finalize
    kp, sg, sc, wh, sf = (t.cuda() for t in HT.pose_finalize_inputs(K, 40 + K))
    for val in (0.0, 1.0):
        assert bool((kp == val).any()) and bool((sg == val).any())
    assert bool((kp < 0).any()) and bool((kp > 1).any()) and bool((sg == 1e-6).any())
    sg4 = torch.full(kp.shape[:3] + (4,), float('nan'), device='cuda')
    sg4[..., :2] = sg
    for rescale in (False, True):
        s = sf if rescale else None
        dk, db = pose_finalize(kp, sg, sc, wh, s)
        dk4, db4 = pose_finalize(kp, sg4[..., :2], sc, wh, s)
        assert torch.equal(dk, dk4) and torch.equal(db, db4)
        ek, eb = HT.pose_finalize_ref(kp, sg, sc, wh, s)
        assert torch.equal(db, eb)
        np.testing.assert_allclose(dk.cpu().numpy(), ek.cpu().numpy(), rtol=2e-6, atol=1e-6)


def test_pose_finalize_refuses_more_than_64_key_points():
    from pavenet_amd.ops import pose_finalize
    kp = torch.rand(1, 2, 65, 2, device='cuda')
    with pytest.raises(RuntimeError):
        pose_finalize(kp, kp + 0.1, torch.rand(1, 2, device='cuda'), torch.tensor([[640., 480.]], device='cuda'))


def test_gather_frame_poses_clamps_indices_outside_the_queries():
    """index values of -1, Q, Q + 5 and 2^40 return the rows of 0, Q - 1, Q - 1 and Q - 1 (the documented clamp
    into [0, Q)); every other row matches torch.gather."""
    from pavenet_amd.ops import gather_frame_poses
    g = torch.Generator().manual_seed(5)
    B, T, Q, N, C = 3, 5, 300, 20, 34
    poses = torch.rand(B, T * Q, C, generator=g)
    idx = torch.stack([torch.randperm(Q, generator=g)[:N] for _ in range(B)])
    idx[0, 0], idx[0, 7], idx[1, 19], idx[2, 3], idx[2, 4] = -1, Q, Q + 5, 2 ** 40, -2 ** 40
    clamped = idx.clamp(0, Q - 1)
    assert clamped[0, 0] == 0 and clamped[0, 7] == clamped[1, 19] == clamped[2, 3] == Q - 1
    got = gather_frame_poses(poses.cuda(), idx.cuda(), T).cpu()
    gidx = clamped.unsqueeze(-1).expand(-1, -1, C)
    exp = torch.stack([torch.gather(poses[:, t * Q:(t + 1) * Q], 1, gidx).reshape(B * N, C) for t in range(T)], 0)
    assert torch.equal(got, exp)
