"""Plain NumPy / torch references and input generators for the head's tail (tests/test_head_tail_gpu.py runs the
kernels against them, tests/test_head_tail_cpu.py checks the references and the input conditions without a GPU).

oks_nms_ref restates the greedy OKS-NMS (HEAD:1624-1665) with the order pave_oks_nms_f32 documents: descending
score, equal scores larger index first, a NaN score as +inf -- the reverse of a STABLE ascending sort (the oracle's
plain argsort is not stable and does not define ties).  The arithmetic is oracle.pavenet_ref.oks_iou's: squared
distances and areas in fp32, everything after them in fp64.
"""
import math

import numpy as np
import torch

OKS_THRESH = 0.45
OKS_GUARD = 1e-6     # smallest |OKS - thresh| a case may have: see test_head_tail_gpu.test_oks_nms_vs_reference
# (n_clips, N, K) of the OKS-NMS cases; clip b of a case is generated with seed 100 * case index + b
OKS_CASES = [(3, 40, 15), (2, 257, 15), (2, 371, 15), (2, 372, 15), (1, 1100, 17), (2, 64, 64), (2, 300, 1)]
OKS_SIGMAS_15 = np.array([.26, .79, .79, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89]) / 10.0


def oks_sigmas(K):
    return OKS_SIGMAS_15 if K == 15 else np.full(K, 0.07)


def _oks_sweep(kpts, scores, thresh, sigmas, band):
    kpts = np.asarray(kpts, np.float32)
    scores = np.asarray(scores, np.float32)
    N, K = kpts.shape[:2]
    x, y = kpts[:, :, 0], kpts[:, :, 1]
    areas = (x.max(1) - x.min(1)) * (y.max(1) - y.min(1))                     # fp32
    s = np.where(np.isnan(scores), np.float32(np.inf), scores)
    order = np.argsort(s, kind='stable')[::-1]
    vars_ = (np.asarray(sigmas, np.float64) * 2) ** 2
    dead = np.zeros(N, bool)
    gap, near = math.inf, 0
    for ii in range(N):
        i = order[ii]
        if dead[i]:
            continue
        rest = order[ii + 1:]
        rest = rest[~dead[rest]]
        if rest.size == 0:
            continue
        dx, dy = x[rest] - x[i], y[rest] - y[i]                               # fp32
        e = (dx ** 2 + dy ** 2) / vars_ / ((areas[i] + areas[rest]) / 2 + np.spacing(1))[:, None] / 2
        ovr = np.sum(np.exp(-e), axis=1) / K
        dist = np.abs(ovr - thresh)
        gap = min(gap, float(dist.min()))
        near += int((dist < band).sum())
        dead[rest[ovr > thresh]] = True
    return ~dead, order, gap, near


def oks_nms_ref(kpts, scores, thresh, sigmas):
    """kpts [N, K, >= 2] fp32, scores [N] fp32, sigmas [K] fp64 -> (keep [N] bool, order [N] int, gap):
    gap = the smallest |OKS - thresh| over every pair that was compared (inf when none was)."""
    return _oks_sweep(kpts, scores, thresh, sigmas, 0.0)[:3]


def near_threshold_pairs(kpts, scores, thresh, sigmas, band=0.05):
    """How many of the pairs oks_nms_ref compares have an OKS within `band` of the threshold."""
    return _oks_sweep(kpts, scores, thresh, sigmas, band)[3]


def oks_inputs(N, K, seed):
    """Clusters of near-duplicate poses at mixed noise levels (so that OKS values spread over (0, 1) and many
    land near the threshold), scores unsorted with exact ties.  -> kpts [N, K, 3] fp32, scores [N] fp32."""
    rng = np.random.default_rng(seed)
    nb = max(4, N // 8)
    base = rng.uniform(0, 400, (nb, K, 2)).astype(np.float32)
    kp = base[rng.integers(0, nb, N)] + (rng.normal(0, 1, (N, K, 2)) * rng.uniform(3, 60, (N, 1, 1))).astype(np.float32)
    scores = rng.uniform(0.05, 1, N).astype(np.float32)
    scores[::7] = scores[3]
    if K == 1:   # every area is 0, the denominator is np.spacing(1) alone: only an exact duplicate suppresses
        dup = rng.permutation(N)[:20]
        kp[dup[:10]] = kp[dup[10:]]
    kpts = np.concatenate([kp.astype(np.float32), np.ones((N, K, 1), np.float32)], -1)
    return kpts, scores


def oks_case(ci):
    """Inputs of OKS case `ci`: (kpts [n_clips, N, K, 3], scores [n_clips, N], sigmas [K])."""
    n_clips, N, K = OKS_CASES[ci]
    clips = [oks_inputs(N, K, 100 * ci + b) for b in range(n_clips)]
    return np.stack([c[0] for c in clips]), np.stack([c[1] for c in clips]), oks_sigmas(K)


def mha_ref(qkv, n_seq, L, H):
    """softmax(q k^T / sqrt(32)) v per (sequence, head) in the dtype of `qkv` (fp64: the reference; fp32: the
    plain formulation whose error scales the large-logit bound).  qkv [n_seq * L, >= 3 H 32] -> [n_seq * L, H 32]."""
    d, E = 32, H * 32
    x = qkv[:, :3 * E].reshape(n_seq, L, 3, H, d)
    q, k, v = x[:, :, 0].transpose(1, 2), x[:, :, 1].transpose(1, 2), x[:, :, 2].transpose(1, 2)
    p = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(d), -1)
    return (p @ v).transpose(1, 2).reshape(n_seq * L, E)


MHA_BIG = (2, 97, 8)      # (n_seq, L, H) of the large-logit case


def mha_big_logit_inputs():
    """qkv [2 * 97, 768] fp32 with q scaled by 12: logits q k / sqrt(32) have a standard deviation of 12, so over
    97 keys they span about +-60 and every softmax row is close to one-hot at a key whose position differs from
    query to query."""
    n_seq, L, H = MHA_BIG
    g = torch.Generator().manual_seed(97)
    qkv = torch.randn(n_seq * L, 3 * H * 32, generator=g)
    qkv[:, :H * 32] *= 12.0
    return qkv


def mha_logits(qkv, n_seq, L, H):
    x = qkv[:, :3 * H * 32].double().reshape(n_seq, L, 3, H, 32)
    return x[:, :, 0].transpose(1, 2) @ x[:, :, 1].transpose(1, 2).transpose(-1, -2) / math.sqrt(32)


def pose_finalize_ref(kp, sg, sc, wh, sf):
    """The tensor expressions of HEAD:1440-1490 + get_p (the reference of
    test_gather_frame_poses_and_pose_finalize_vs_torch), in the tensors' own dtype and device."""
    B = kp.shape[0]
    whb = wh.view(B, 1, 1, 2)
    k = kp * whb
    k = torch.minimum(k.clamp(min=0), whb)
    if sf is not None:
        k = k / sf.view(B, 1, 1, 2)
    x1, y1 = k[..., 0].min(2, keepdim=True)[0], k[..., 1].min(2, keepdim=True)[0]
    x2, y2 = k[..., 0].max(2, keepdim=True)[0], k[..., 1].max(2, keepdim=True)[0]
    eb = torch.cat([x1, y1, x2, y2, sc.unsqueeze(-1)], 2)
    p = 1 - torch.exp(-(0.2 / sg))
    p = (p[..., 0] * p[..., 1])[..., None] * 0.7
    p5 = p ** 5
    ek = torch.cat(((k * p5) / (p5 + 1e-10), sc[:, :, None, None] * p), 3)
    return ek, eb


def pose_finalize_inputs(K, seed):
    """kp with exact 0, exact 1, values below 0 and above 1; sigmas drawn per element from
    {0.0, 1e-6, 0.02, 0.5, 1.0} (0.0 and 1.0: a saturated fp32 sigmoid) or uniform in [0.02, 0.52)."""
    g = torch.Generator().manual_seed(seed)
    B, N = 3, 7
    kp = torch.rand(B, N, K, 2, generator=g) * 1.4 - 0.2
    pick = torch.randint(0, 6, (B, N, K, 2), generator=g)
    kp = torch.where(pick == 0, torch.zeros(()), kp)
    kp = torch.where(pick == 1, torch.ones(()), kp)
    special = torch.tensor([0.0, 1e-6, 0.02, 0.5, 1.0])
    choice = torch.randint(0, 8, (B, N, K, 2), generator=g)
    sg = torch.where(choice < 5, special[choice.clamp(max=4)], torch.rand(B, N, K, 2, generator=g) * 0.5 + 0.02)
    sc = torch.rand(B, N, generator=g)
    wh = torch.tensor([[1344., 800.], [1200., 780.], [640., 480.]])
    sf = torch.tensor([[1.5, 1.25], [0.8, 0.9], [1., 1.]])
    return kp, sg, sc, wh, sf
