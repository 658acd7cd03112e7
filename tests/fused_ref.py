"""fp64 restatement of the fused T-frame deformable-attention ops (``deform_attn_grid_fused``,
``deform_attn_pose_fused``, and with T = 1 the encoder's tile kernel), in plain torch on top of
``tests/msda_ref.py::msda_ref``.  Test helper (CPU); nothing here touches the C oracle.

Semantics (what the kernels compute between the Linears):

* ONE stabilised softmax over all T * L * P logits of a (unit, head) -- mathematically the oracle's per-frame
  softmax re-weighted by Z_t / sum Z (tests/fused_expected.py), without its un-stabilised exp;
* grid locations = ref + offset / (W, H) of the level;
* pose locations = ref + offset * max(extent of the key points, 1e-4) / 2 per (frame, level);
* ``slab_of[unit, t]`` is the slab of ``value`` the unit samples in frame t: frame tables, ``unit_clip`` and the
  clamp into the value tensor are spelled out by the caller, not hidden in here;
* stat_max = the largest logit, stat_sum = sum exp(logit - stat_max).

Everything is returned in fp64: (out [U, 256], stat_max [U, 8], stat_sum [U, 8]).
"""
import torch

from tests.msda_ref import msda_ref

M, D = 8, 32


def _softmax_all(lg):
    """lg [U, T, M, LP] (any float dtype) -> weights [U, T, M, LP], max [U, M], sum [U, M] in fp64."""
    U, T, _, LP = lg.shape
    x = lg.to(torch.float64).permute(0, 2, 1, 3).reshape(U, M, T * LP)
    mx = x.max(-1, keepdim=True)[0]
    e = torch.exp(x - mx)
    sm = e.sum(-1, keepdim=True)
    w = (e / sm).view(U, M, T, LP).permute(0, 2, 1, 3)
    return w, mx.squeeze(-1), sm.squeeze(-1)


def _sample(value, shapes, lsi, loc, w, slab_of):
    """loc [U, T, M, L, P, 2], w [U, T, M, L, P] fp64, slab_of [U, T] -> out [U, 256]: every (unit, frame)
    samples its own slab; units that share a slab go through msda_ref together."""
    U, T = loc.shape[:2]
    slab_of = torch.as_tensor(slab_of, dtype=torch.long).reshape(U, T)
    assert int(slab_of.min()) >= 0 and int(slab_of.max()) < value.shape[0], 'slab_of outside value'
    out = torch.zeros(U, M * D, dtype=torch.float64)
    for t in range(T):
        for s in slab_of[:, t].unique().tolist():
            u = (slab_of[:, t] == s).nonzero().squeeze(1)
            out[u] += msda_ref(value[s:s + 1], shapes, lsi, loc[u, t][None], w[u, t][None])[0]
    return out


def grid_ref64(value, shapes, lsi, proj, ref, T, slab_of):
    """value [n_slabs, S, 8, 32]; shapes [L, 2] (H, W); proj [U, >= T*8*L*4*3]; ref [T, U, L, 2];
    slab_of [U, T]."""
    U, L, P = proj.shape[0], shapes.shape[0], 4
    n = T * M * L * P
    off = proj[:, :2 * n].to(torch.float64).view(U, T, M, L, P, 2)
    w, mx, sm = _softmax_all(proj[:, 2 * n:3 * n].reshape(U, T, M, L * P))
    norm = torch.stack([shapes[:, 1], shapes[:, 0]], -1).to(torch.float64)           # (W, H)
    r = ref.to(torch.float64).permute(1, 0, 2, 3)                                       # [U, T, L, 2]
    loc = r[:, :, None, :, None, :] + off / norm[None, None, None, :, None, :]
    return _sample(value, shapes, lsi, loc, w.reshape(U, T, M, L, P), slab_of), mx, sm


def pose_ref64(value, shapes, lsi, proj, ref, T, n_clips, Q, K, slab_of):
    """value [n_slabs, S, 8, 32]; proj [n_clips*Q, >= T*8*L*K*3]; ref [n_clips, T*Q, L, 2K] (the level axis may
    be a broadcast view); slab_of [n_clips*Q, T]."""
    U, L = n_clips * Q, shapes.shape[0]
    n = T * M * L * K
    off = proj[:, :2 * n].to(torch.float64).view(U, T, M, L, K, 2)
    w, mx, sm = _softmax_all(proj[:, 2 * n:3 * n].reshape(U, T, M, L * K))
    rp = ref.to(torch.float64).reshape(n_clips, T, Q, L, K, 2).permute(0, 2, 1, 3, 4, 5).reshape(U, T, L, K, 2)
    extent = (rp.max(-2)[0] - rp.min(-2)[0]).clamp(min=1e-4)                            # [U, T, L, 2]
    loc = rp[:, :, None] + off * extent[:, :, None, :, None, :] * 0.5
    return _sample(value, shapes, lsi, loc, w.reshape(U, T, M, L, K), slab_of), mx, sm
