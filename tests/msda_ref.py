"""fp64 restatement of the multi-scale deformable attention sampler (``ms_deform_attn_forward``) that
addresses the levels through ``level_start_index`` and reads only the value rows the asked-for queries touch.

Semantics of mmcv's CUDA kernel (ms_deform_attn_cuda_kernel.cuh:17-64, 200-254, restated in
``msda_fwd_scalar_kernel``):

* pixel = loc * size - 0.5 on both axes (x = loc[..., 0] * W, y = loc[..., 1] * H);
* a point counts only if -1 < pixel < size on both axes (false for NaN, so such a point drops out);
* a corner outside the map contributes 0;
* level l's row (y, x) is value row ``lsi[l] + y * W + x``.

Everything is torch in fp64, so autograd through ``msda_ref`` gives the reference gradients of value,
locations and weights (the one-sided derivative at an integer pixel is floor's, as in the kernels).  ``value``
may live on any device and in any dtype: corner rows are gathered where it lives and only those rows come to
the host, so a multi-GiB device tensor is never copied whole.
"""
import torch


def msda_ref(value, shapes, lsi, loc, attw, queries=None):
    """value [bs, S, M, D], shapes [L, 2] (H, W), lsi [L], loc [bs, Lq, M, L, P, 2], attw [bs, Lq, M, L, P]
    -> fp64 [bs, nq, M * D] on the host, for the query indices `queries` (a 1-D index, default all Lq)."""
    if queries is not None:
        q = torch.as_tensor(queries, dtype=torch.long)
        loc, attw = loc[:, q.to(loc.device)], attw[:, q.to(attw.device)]
    loc = loc.to('cpu', torch.float64)
    attw = attw.to('cpu', torch.float64)
    bs, S, M, D = value.shape
    _, nq, _, L, P, _ = loc.shape
    hw = [(int(h), int(w)) for h, w in shapes.tolist()]
    starts = [int(s) for s in lsi.tolist()]
    dev = value.device
    b_i = torch.arange(bs, device=dev).view(bs, 1, 1, 1)
    m_i = torch.arange(M, device=dev).view(1, 1, M, 1)
    out = torch.zeros(bs, nq, M, D, dtype=torch.float64)
    for l, ((H, W), st) in enumerate(zip(hw, starts)):
        x = loc[:, :, :, l, :, 0] * W - 0.5                      # [bs, nq, M, P]
        y = loc[:, :, :, l, :, 1] * H - 0.5
        inside = (y > -1) & (x > -1) & (y < H) & (x < W)
        x = torch.where(inside, x, torch.zeros_like(x))          # keeps NaN / inf out of floor and of the gradient
        y = torch.where(inside, y, torch.zeros_like(y))
        x0, y0 = torch.floor(x).detach(), torch.floor(y).detach()
        lx, ly = x - x0, y - y0
        hx, hy = 1 - lx, 1 - ly
        a = attw[:, :, :, l, :]
        x0, y0 = x0.long(), y0.long()
        for cy, cx, w in ((y0, x0, hy * hx), (y0, x0 + 1, hy * lx), (y0 + 1, x0, ly * hx),
                          (y0 + 1, x0 + 1, ly * lx)):
            ok = inside & (cy >= 0) & (cy < H) & (cx >= 0) & (cx < W)
            row = st + cy.clamp(0, H - 1) * W + cx.clamp(0, W - 1)
            v = value[b_i, row.to(dev), m_i].to('cpu', torch.float64)   # [bs, nq, M, P, D]
            wa = torch.where(ok, w, torch.zeros_like(w)) * a
            out = out + (wa.unsqueeze(-1) * v).sum(3)
    return out.reshape(bs, nq, M * D)


def contiguous_lsi(shapes):
    """Exclusive cumulative sum of the level sizes: the level_start_index every caller of mmcv passes."""
    shapes = torch.as_tensor(shapes, dtype=torch.long)
    return torch.cat((shapes.new_zeros((1,)), shapes.prod(1).cumsum(0)[:-1]))
