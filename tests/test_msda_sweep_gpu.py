"""ms_deform_attn_forward / _backward, the op this package ships as mmcv._ext's device implementation, against
the fp64 gather reference (tests/msda_ref.py) at every kernel msda_forward_impl / msda_backward_impl
(pave_kernels.hip) dispatch to:

* forward fp32: msda_fwd_vec_kernel<G = D / 4> for D = 4 .. 256 (G a power of two), msda_fwd_scalar_kernel<float>
  for every other D; forward fp64: msda_fwd_scalar_kernel<double>;
* backward fp32: msda_bwd_kernel<float, G, 4> for D = 4, 8, 16, 32, 64, msda_bwd_kernel<float, 1, 1> otherwise;
  backward fp64: msda_bwd_kernel<double, 1, 1>;

at level counts 1 .. 8 with uneven shapes (1 x 1 and 1 x W included), non-contiguous level_start_index, past the
launch grid caps, next to the 2 GiB value slab limit, with non-finite locations, and with the backward's
accumulate / overwrite contract.  Needs an MI355X.
"""
import math

import numpy as np
import pytest
import torch

from pavenet_amd import ops
from tests.msda_ref import contiguous_lsi, msda_ref

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
D_LIST = [1, 2, 3, 4, 8, 12, 16, 20, 32, 64, 128, 256, 260, 1025]
LEVEL_POOL = [(1, 1), (1, 13), (7, 3), (12, 20), (5, 9), (2, 1), (16, 16), (3, 17)]
BAD = (float('nan'), float('inf'), -float('inf'), 1e30, -1e30)
GRID_CAP_BLOCKS = 65536 * 4   # msda_forward_impl / msda_backward_impl: at most this many blocks of 256 threads


def _ext():
    from pavenet_amd import _ext
    return _ext


def _id(v):
    return {F32: 'f32', F64: 'f64'}.get(v, str(v))


def _configs(i):
    """(M, L, P, bs) of the covering set for the i-th D: over its three configurations every D meets
    M in {1, 3, 8}, L in {1, 3, 8}, P in {1, 4, 8} and bs in {1, 3}; the pairings rotate with i."""
    Ms, Ls, Ps, bss = (1, 3, 8), (1, 3, 8), (1, 4, 8), (1, 3)
    return [(Ms[j], Ls[(j + i) % 3], Ps[(j + 2 * i) % 3], bss[(j + i) % 2]) for j in range(3)]


def _levels(L, rot):
    return [LEVEL_POOL[(rot + i) % len(LEVEL_POOL)] for i in range(L)]


def _wh(levels, device='cpu'):
    """(W, H) per level shaped [L, 1, 2], to broadcast against loc[..., L, P, 2]."""
    return torch.tensor([[w, h] for h, w in levels], dtype=F64, device=device).view(len(levels), 1, 2)


def _kink_free(loc, levels):
    """Moves every pixel coordinate (loc * size - 0.5) that lies within 1e-3 px of an integer to the middle of the
    nearest quarter: the bilinear form has a kink there (the map border -1 / size included), where the
    one-sided derivative is a convention."""
    sz = _wh(levels, loc.device)
    px = loc * sz - 0.5
    f = px - torch.floor(px)
    near = (f < 1e-3) | (f > 1 - 1e-3)
    return torch.where(near, (torch.round(px) + 0.25 + 0.5) / sz, loc)


def _locs(g, shape5, levels, borders=False, kink_free=False, device='cpu'):
    """fp64 locations [bs, Lq, M, L, P, 2] uniform in [-0.15, 1.15].  borders: about 30 % of the coordinates
    pinned at 0, 1, +-0.5 / size, 1 -+ 0.5 / size (pixel -0.5, size - 0.5, 0, -1, size - 1, size) or at an exact
    pixel centre.  kink_free: see _kink_free."""
    shape = tuple(shape5) + (2,)
    loc = torch.rand(shape, generator=g, dtype=F64, device=device) * 1.3 - 0.15
    if borders:
        sz = _wh(levels, device).expand(shape)
        half = 0.5 / sz
        centre = (torch.floor(torch.rand(shape, generator=g, dtype=F64, device=device) * sz) + 0.5) / sz
        cands = torch.stack((torch.zeros_like(loc), torch.ones_like(loc), half, -half, 1 - half, 1 + half, centre))
        kind = torch.randint(0, len(cands), shape, generator=g, device=device)
        pick = torch.rand(shape, generator=g, dtype=F64, device=device) < 0.3
        loc = torch.where(pick, cands.gather(0, kind[None])[0], loc)
    return _kink_free(loc, levels) if kink_free else loc


def _weights(g, shape5, device='cpu'):
    """Positive attention weights normalised per (query, head), so that outputs are O(1)."""
    aw = torch.rand(shape5, generator=g, dtype=F64, device=device) + 0.05
    return aw / aw.sum((-1, -2), keepdim=True)


def _case(seed, bs, M, D, levels, Lq, P, dtype, borders=False, kink_free=False):
    g = torch.Generator().manual_seed(seed)
    shapes = torch.as_tensor(levels, dtype=torch.long)
    lsi = contiguous_lsi(shapes)
    S, L = int(shapes.prod(1).sum()), len(levels)
    value = (torch.rand(bs, S, M, D, generator=g, dtype=F64) * 2 - 1).to(dtype)
    loc = _locs(g, (bs, Lq, M, L, P), levels, borders, kink_free).to(dtype)
    aw = _weights(g, (bs, Lq, M, L, P)).to(dtype)
    gout = torch.rand(bs, Lq, M * D, generator=g, dtype=F64).to(dtype)
    return g, shapes, lsi, value, loc, aw, gout


def _cuda(*ts):
    return [t.cuda() for t in ts]


def _fwd_tol(dtype, L, P):
    """fp32: the golden tests' rtol 1e-5 / atol 2e-6 up to 16 points per (query, head), atol growing as
    sqrt(L * P / 16) above that; fp64: 1e-12."""
    if dtype == F64:
        return dict(rtol=1e-12, atol=1e-12)
    return dict(rtol=1e-5, atol=2e-6 * max(1.0, math.sqrt(L * P / 16)))


def _assert_grad(got, exp, dtype, what):
    """fp32: rtol 2e-4 and an atol of 1e-5 x the gradient's largest magnitude; fp64: rtol 1e-9, atol 1e-12 x it."""
    exp = exp.detach().double().cpu().numpy()
    scale = float(np.abs(exp).max()) if exp.size else 0.0
    tol = dict(rtol=1e-9, atol=1e-12 * scale) if dtype == F64 else dict(rtol=2e-4, atol=1e-5 * scale)
    np.testing.assert_allclose(got.detach().double().cpu().numpy(), exp, err_msg=what, **tol)


def _ref_grads(value, shapes, lsi, loc, aw, gout, value_grad=True):
    """fp64 autograd through the reference: (grad_value or None, grad_loc, grad_aw).  value_grad=False leaves
    value where it is (a device tensor: only the gathered rows come to the host)."""
    v = value.detach().double().requires_grad_(True) if value_grad else value
    lo = loc.detach().cpu().double().requires_grad_(True)
    a = aw.detach().cpu().double().requires_grad_(True)
    msda_ref(v, shapes, lsi, lo, a).backward(gout.detach().cpu().double())
    return (v.grad if value_grad else None), lo.grad, a.grad


def _backward(fn, dev, gout, gv0, step=64):
    """Runs fn (ops or _ext ms_deform_attn_backward) on grad_value = gv0 (accumulated into) and NaN-filled
    grad_sampling_loc / grad_attn_weight (overwritten)."""
    value, shapes, lsi, loc, aw = dev
    gv = gv0.clone()
    gl = torch.full_like(loc, float('nan'))
    ga = torch.full_like(aw, float('nan'))
    fn(value, shapes, lsi, loc, aw, gout, gv, gl, ga, im2col_step=step)
    torch.cuda.synchronize()
    return gv, gl, ga


# ---------------------------------------------------------------------------------------------------------------
# a. forward sweep
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [F32, F64], ids=['f32', 'f64'])
@pytest.mark.parametrize('D', D_LIST)
def test_forward_sweep_vs_fp64_reference(D, dtype):
    i = D_LIST.index(D)
    for j, (M, L, P, bs) in enumerate(_configs(i)):
        levels = _levels(L, i + j)
        Lq = max(2, min(48, 600_000 // (bs * M * L * P * D)))
        _, shapes, lsi, value, loc, aw, _ = _case(1000 * i + j, bs, M, D, levels, Lq, P, dtype, borders=True)
        dev = _cuda(value, shapes, lsi, loc, aw)
        out = ops.ms_deform_attn_forward(*dev, im2col_step=64)
        exp = msda_ref(value, shapes, lsi, loc, aw)
        np.testing.assert_allclose(out.cpu().double().numpy(), exp.numpy(), **_fwd_tol(dtype, L, P),
                                   err_msg=f'M={M} L={L} P={P} bs={bs} levels={levels}')
        if j == 0:   # the pybind boundary runs the same launch: bit-equal
            assert torch.equal(_ext().ms_deform_attn_forward(*dev, im2col_step=64), out)


# ---------------------------------------------------------------------------------------------------------------
# b. + c. backward sweep with the accumulate / overwrite contract
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [F32, F64], ids=['f32', 'f64'])
@pytest.mark.parametrize('D', D_LIST)
def test_backward_sweep_vs_fp64_autograd_and_contract(D, dtype):
    """grad_value is accumulated into a non-zero initial tensor; grad_sampling_loc / grad_attn_weight start as NaN
    and every entry must be written, with exact zeros for the points far outside every map."""
    i = D_LIST.index(D)
    for j, (M, L, P, bs) in enumerate(_configs(i)[:2]):
        levels = _levels(L, 3 * i + j)
        Lq = max(2, min(24, 200_000 // (bs * M * L * P * D)))
        g, shapes, lsi, value, loc, aw, gout = _case(500 + 1000 * i + j, bs, M, D, levels, Lq, P, dtype,
                                                     kink_free=True)
        far = torch.zeros(aw.shape, dtype=torch.bool)
        far.view(-1)[j::5] = True
        loc[far] = torch.tensor([7.5, -3.25], dtype=dtype)
        rgv, rgl, rga = _ref_grads(value, shapes, lsi, loc, aw, gout)
        gv0 = (torch.rand(value.shape, generator=g, dtype=F64) * 2 - 1) * float(rgv.abs().max())
        gv0 = gv0.to(dtype)
        dev = _cuda(value, shapes, lsi, loc, aw)
        gv, gl, ga = _backward(ops.ms_deform_attn_backward, dev, gout.cuda(), gv0.cuda())
        what = f'D={D} M={M} L={L} P={P} bs={bs} levels={levels}'
        assert torch.isfinite(gl).all() and torch.isfinite(ga).all(), what
        assert (gl.cpu()[far] == 0).all() and (ga.cpu()[far] == 0).all(), what
        _assert_grad(gl, rgl, dtype, 'grad_sampling_loc ' + what)
        _assert_grad(ga, rga, dtype, 'grad_attn_weight ' + what)
        _assert_grad(gv.cpu().double() - gv0.double(), rgv, dtype, 'grad_value ' + what)
        if j == 0:   # the pybind boundary: the same per-point results bit for bit, grad_value up to atomic order
            egv, egl, ega = _backward(_ext().ms_deform_attn_backward, dev, gout.cuda(), gv0.cuda())
            assert torch.equal(egl, gl) and torch.equal(ega, ga), what
            _assert_grad(egv.cpu().double() - gv0.double(), rgv, dtype, 'ext grad_value ' + what)


@pytest.mark.parametrize('D,dtype', [(32, F32), (71, F32), (16, F64)], ids=_id)
def test_backward_contended_grad_value(D, dtype):
    """Thousands of points on a 2 x 2 level: every grad_value entry of it is an atomic sum of Lq * P terms, all
    positive, compared with a tolerance that grows as sqrt(terms) (a lost update costs 1 / terms)."""
    levels = [(2, 2), (1, 3)]
    bs, M, Lq, P = 2, 2, 2048, 4
    g, shapes, lsi, value, loc, aw, gout = _case(77 + D, bs, M, D, levels, Lq, P, dtype)
    value = value.abs() + 0.1                                          # positive terms only
    loc[..., 0, :, :] = 0.25 + 0.5 * torch.rand(loc[..., 0, :, :].shape, generator=g, dtype=F64).to(dtype)
    loc = _kink_free(loc.double(), levels).to(dtype)
    rgv, rgl, rga = _ref_grads(value, shapes, lsi, loc, aw, gout)
    gv, gl, ga = _backward(ops.ms_deform_attn_backward, _cuda(value, shapes, lsi, loc, aw), gout.cuda(),
                           torch.zeros(value.shape, dtype=dtype, device='cuda'))
    terms = Lq * P
    rtol = 16 * math.sqrt(terms) * 2.0 ** -24 if dtype == F32 else 1e-12 * math.sqrt(terms)
    np.testing.assert_allclose(gv.cpu()[:, :4].double().numpy(), rgv[:, :4].numpy(), rtol=rtol)
    _assert_grad(gv, rgv, dtype, 'grad_value')
    _assert_grad(gl, rgl, dtype, 'grad_sampling_loc')
    _assert_grad(ga, rga, dtype, 'grad_attn_weight')


# ---------------------------------------------------------------------------------------------------------------
# d. level_start_index is honoured
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('D,dtype', [(32, F32), (8, F32), (12, F32), (8, F64)], ids=_id)
def test_level_start_index_reversed_levels_with_a_gap(D, dtype):
    """Levels stored last-first with unused rows between two of them: both directions follow lsi, never the
    cumulative shapes; the gap rows (value 1e3) are never read and their grad_value rows are never written."""
    levels = [(3, 5), (1, 7), (4, 4), (2, 1)]
    sizes = [h * w for h, w in levels]
    gap = 6
    lsi = torch.zeros(len(levels), dtype=torch.long)
    pos = 0
    for l in reversed(range(len(levels))):
        lsi[l] = pos
        pos += sizes[l] + (gap if l == 2 else 0)
    gap_rows = slice(int(lsi[2]) + sizes[2], int(lsi[2]) + sizes[2] + gap)
    bs, M, Lq, P = 2, 3, 12, 3
    g, shapes, _, _, loc, aw, gout = _case(31 + D, bs, M, D, levels, Lq, P, dtype, borders=False, kink_free=True)
    value = (torch.rand(bs, pos, M, D, generator=g, dtype=F64) * 2 - 1).to(dtype)
    value[:, gap_rows] = 1e3
    dev = _cuda(value, shapes, lsi, loc, aw)
    out = ops.ms_deform_attn_forward(*dev, im2col_step=64)
    np.testing.assert_allclose(out.cpu().double().numpy(), msda_ref(value, shapes, lsi, loc, aw).numpy(),
                               **_fwd_tol(dtype, len(levels), P))
    rgv, rgl, rga = _ref_grads(value, shapes, lsi, loc, aw, gout)
    gv0 = (torch.rand(value.shape, generator=g, dtype=F64) * 2 - 1).to(dtype)
    gv, gl, ga = _backward(ops.ms_deform_attn_backward, dev, gout.cuda(), gv0.cuda())
    assert torch.equal(gv.cpu()[:, gap_rows], gv0[:, gap_rows])
    _assert_grad(gv.cpu().double() - gv0.double(), rgv, dtype, 'grad_value')
    _assert_grad(gl, rgl, dtype, 'grad_sampling_loc')
    _assert_grad(ga, rga, dtype, 'grad_attn_weight')


# ---------------------------------------------------------------------------------------------------------------
# e. im2col_step
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('D,dtype', [(32, F32), (20, F64)], ids=_id)
def test_im2col_step_changes_no_bit(D, dtype):
    levels = _levels(3, 2)
    bs, M, Lq, P = 6, 2, 10, 2
    _, shapes, lsi, value, loc, aw, gout = _case(55 + D, bs, M, D, levels, Lq, P, dtype, kink_free=True)
    dev = _cuda(value, shapes, lsi, loc, aw)
    gout, gv0 = gout.cuda(), torch.zeros(value.shape, dtype=dtype, device='cuda')
    outs = [ops.ms_deform_attn_forward(*dev, im2col_step=s) for s in (1, 2, 3, 6, 64)]
    np.testing.assert_allclose(outs[0].cpu().double().numpy(), msda_ref(value, shapes, lsi, loc, aw).numpy(),
                               **_fwd_tol(dtype, 3, P))
    grads = [_backward(ops.ms_deform_attn_backward, dev, gout, gv0, step=s) for s in (1, 2, 3, 6, 64)]
    for o, (gv, gl, ga) in zip(outs[1:], grads[1:]):
        assert torch.equal(o, outs[0])
        assert torch.equal(gl, grads[0][1]) and torch.equal(ga, grads[0][2])
        _assert_grad(gv, grads[0][0], dtype, 'grad_value')
    for fn in (ops.ms_deform_attn_backward, _ext().ms_deform_attn_backward):
        with pytest.raises(RuntimeError):   # 6 % 4 != 0 (ms_deform_attn_cuda.cu:242-245)
            _backward(fn, dev, gout, gv0, step=4)


# ---------------------------------------------------------------------------------------------------------------
# f. level count limits
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('D,dtype', [(32, F32), (12, F32), (8, F64)], ids=_id)
def test_eight_levels_accepted_nine_refused(D, dtype):
    _, shapes, lsi, value, loc, aw, _ = _case(88 + D, 2, 2, D, LEVEL_POOL, 6, 2, dtype, borders=True)
    dev = _cuda(value, shapes, lsi, loc, aw)
    out = ops.ms_deform_attn_forward(*dev, im2col_step=64)
    np.testing.assert_allclose(out.cpu().double().numpy(), msda_ref(value, shapes, lsi, loc, aw).numpy(),
                               **_fwd_tol(dtype, 8, 2))
    _, shapes, lsi, value, loc, aw, _ = _case(99 + D, 2, 2, D, LEVEL_POOL + [(2, 2)], 6, 2, dtype)
    dev = _cuda(value, shapes, lsi, loc, aw)
    for fn in (ops.ms_deform_attn_forward, _ext().ms_deform_attn_forward):
        with pytest.raises(RuntimeError):   # msda_forward_impl refuses L > kMaxLevels before launching
            fn(*dev, im2col_step=64)


# ---------------------------------------------------------------------------------------------------------------
# g. non-finite locations
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('D,dtype', [(64, F32), (12, F32), (8, F64)], ids=_id)
def test_non_finite_locations_drop_out(D, dtype):
    """+-inf, +-1e30 and NaN in location entries (weights finite): such a point fails mmcv's range test (its
    comparisons are false for NaN), so the output equals the reference with the point's weight set to 0 and its
    grad_attn_weight / grad_sampling_loc are exact zeros."""
    levels = _levels(4, 1)
    bs, M, Lq, P = 2, 3, 16, 4
    g, shapes, lsi, value, loc, aw, gout = _case(123 + D, bs, M, D, levels, Lq, P, dtype, kink_free=True)
    flat = loc.view(-1)
    idx = torch.arange(3, flat.numel(), 7)
    flat[idx] = torch.tensor(BAD, dtype=dtype).repeat(len(idx) // len(BAD) + 1)[:len(idx)]
    bad = ~torch.isfinite(loc).all(-1) | (loc.abs() > 1e20).any(-1)
    assert bad.any() and not bad.all()
    clean_loc = torch.where(bad[..., None], torch.full_like(loc, 0.5), loc)
    clean_aw = torch.where(bad, torch.zeros_like(aw), aw)
    dev = _cuda(value, shapes, lsi, loc, aw)
    out = ops.ms_deform_attn_forward(*dev, im2col_step=64)
    np.testing.assert_allclose(out.cpu().double().numpy(),
                               msda_ref(value, shapes, lsi, clean_loc, clean_aw).numpy(), **_fwd_tol(dtype, 4, P))
    rgv, rgl, rga = _ref_grads(value, shapes, lsi, clean_loc, clean_aw, gout)
    gv, gl, ga = _backward(ops.ms_deform_attn_backward, dev, gout.cuda(),
                           torch.zeros(value.shape, dtype=dtype, device='cuda'))
    gl, ga = gl.cpu(), ga.cpu()
    assert (gl[bad] == 0).all() and (ga[bad] == 0).all()
    assert torch.isfinite(gl).all() and torch.isfinite(ga).all()
    _assert_grad(gl[~bad], rgl[~bad], dtype, 'grad_sampling_loc')
    _assert_grad(ga[~bad], rga[~bad], dtype, 'grad_attn_weight')
    _assert_grad(gv, rgv, dtype, 'grad_value')


# ---------------------------------------------------------------------------------------------------------------
# h. past the grid caps: the grid-stride loops of every kernel
# ---------------------------------------------------------------------------------------------------------------
def _dyadic(loc):
    """Locations on multiples of 2^-14: loc * size - 0.5 is then exact in fp32 for every size up to 512, so a map
    of any width adds no rounding of the sample position to the comparison (the golden tolerances assume maps
    of at most ~20 pixels, where that rounding stays below them)."""
    return torch.round(loc * 2.0 ** 14) / 2.0 ** 14


def _big_inputs(seed, Lq, M, D, levels, P, kink_free=False, dyadic=False):
    """fp32 device inputs drawn on the device (bs = 1)."""
    g = torch.Generator(device='cuda').manual_seed(seed)
    shapes = torch.as_tensor(levels, dtype=torch.long)
    lsi = contiguous_lsi(shapes)
    S, L = int(shapes.prod(1).sum()), len(levels)
    value = torch.rand(1, S, M, D, generator=g, device='cuda') * 2 - 1
    loc = _locs(g, (1, Lq, M, L, P), levels, kink_free=kink_free, device='cuda')
    loc = (_dyadic(loc) if dyadic else loc).float()
    aw = _weights(g, (1, Lq, M, L, P), device='cuda').float()
    return g, shapes, lsi, value, loc, aw


def _sample(Lq, n_groups_tail, M, seed):
    """Query indices: the queries of the last n_groups_tail (query, head) groups, a few spread over the rest."""
    tail = max(1, n_groups_tail // M)
    g = torch.Generator().manual_seed(seed)
    spread = torch.randint(0, Lq - tail, (1024,), generator=g)
    return torch.cat((torch.tensor([0, 1]), spread.sort().values, torch.arange(Lq - tail, Lq))).unique()


@pytest.mark.parametrize('D,Lq', [(256, 1_100_000), (71, 950_000)])
def test_forward_past_the_grid_cap(D, Lq):
    """vec G = 64: ngroups = Lq > 65536 * 4 blocks x 4 groups; scalar fp32: Lq * 71 outputs > 65536 * 4 x 256.
    Sampled rows (the last 4096 groups included) against the reference, and bit-equal to the same queries run in
    a call of their own (every group is computed independently, in a fixed order)."""
    levels, P = [(48, 64)], 2
    if D == 256:
        assert Lq > GRID_CAP_BLOCKS * (256 // 64)
    else:
        assert Lq * D > GRID_CAP_BLOCKS * 256
    _, shapes, lsi, value, loc, aw = _big_inputs(D, Lq, 1, D, levels, P, dyadic=True)
    sd, ld = shapes.cuda(), lsi.cuda()
    out = ops.ms_deform_attn_forward(value, sd, ld, loc, aw, im2col_step=64)
    q = _sample(Lq, 4096, 1, D)
    got = out[:, q.cuda()].cpu()
    del out
    np.testing.assert_allclose(got.double().numpy(), msda_ref(value, shapes, lsi, loc, aw, q).numpy(),
                               **_fwd_tol(F32, 1, P))
    qd = q.cuda()
    small = ops.ms_deform_attn_forward(value, sd, ld, loc[:, qd].contiguous(), aw[:, qd].contiguous(), im2col_step=64)
    assert torch.equal(small.cpu(), got)


def test_backward_past_the_grid_cap():
    """msda_bwd_kernel<float, 16, 4> (D = 64) with ngroups > 65536 * 4 blocks x 16 groups, over a 1024 x 1024 level
    so that the grad_value atomics stay uncontended: sampled points' grad_sampling_loc / grad_attn_weight against
    the reference and bit-equal to the same queries in a call of their own."""
    D, Lq, P, levels = 64, 4_300_000, 1, [(1024, 1024)]
    assert Lq > GRID_CAP_BLOCKS * (256 // 16)
    g, shapes, lsi, value, loc, aw = _big_inputs(7, Lq, 1, D, levels, P, kink_free=True)
    gout = torch.rand(1, Lq, D, generator=g, device='cuda')
    sd, ld = shapes.cuda(), lsi.cuda()
    gv, gl, ga = _backward(ops.ms_deform_attn_backward, (value, sd, ld, loc, aw), gout, torch.zeros_like(value))
    del gv
    assert torch.isfinite(gl).all() and torch.isfinite(ga).all()
    q = _sample(Lq, 4096, 1, 64)
    qd = q.cuda()
    sl, sa, sg = loc[:, qd].contiguous(), aw[:, qd].contiguous(), gout[:, qd].contiguous()
    _, rgl, rga = _ref_grads(value, shapes, lsi, sl, sa, sg, value_grad=False)
    _assert_grad(gl[:, qd], rgl, F32, 'grad_sampling_loc')
    _assert_grad(ga[:, qd], rga, F32, 'grad_attn_weight')
    _, sgl, sga = _backward(ops.ms_deform_attn_backward, (value, sd, ld, sl, sa), sg, torch.zeros_like(value))
    assert torch.equal(sgl, gl[:, qd]) and torch.equal(sga, ga[:, qd])


# ---------------------------------------------------------------------------------------------------------------
# i. next to the 2 GiB slab limit of the vector forward's 32-bit byte offsets
# ---------------------------------------------------------------------------------------------------------------
def test_vec_forward_next_to_the_2gib_slab():
    """M = 8, D = 256 (8 KiB rows), S = 262140 rows: one value slab is 32 KiB short of 2 GiB, the largest the
    forward accepts; with bs = 3 the second slab straddles 2 GiB and the third starts past 4 GiB.  Queries sample
    the last rows of the last level (and the first level) in every batch; the reference gathers just those rows."""
    M, D, P = 8, 256, 2
    levels = [(511, 512), (4, 127)]
    shapes = torch.as_tensor(levels, dtype=torch.long)
    lsi = contiguous_lsi(shapes)
    S = int(shapes.prod(1).sum())
    assert S * M * D * 4 < 2 ** 31 <= (S + 4) * M * D * 4
    bs, Lq = 3, 40
    g = torch.Generator(device='cuda').manual_seed(3)
    value = torch.rand(bs, S, M, D, generator=g, device='cuda') * 2 - 1
    loc = _locs(g, (bs, Lq, M, 2, P), levels, borders=True, device='cuda')
    loc[:, :, :, 1] = 1 - loc[:, :, :, 1].remainder(0.25)             # last level: its last rows and columns
    loc = _dyadic(loc).float()
    aw = _weights(g, (bs, Lq, M, 2, P), device='cuda').float()
    sd, ld = shapes.cuda(), lsi.cuda()
    out = ops.ms_deform_attn_forward(value, sd, ld, loc, aw, im2col_step=64)
    np.testing.assert_allclose(out.cpu().double().numpy(), msda_ref(value, shapes, lsi, loc, aw).numpy(),
                               **_fwd_tol(F32, 2, P))
    del value
    torch.cuda.empty_cache()
    big = torch.empty(1, S + 4, M, D, device='cuda')
    with pytest.raises(RuntimeError):   # S * M * D * 4 >= 2 GiB: refused before launching
        ops.ms_deform_attn_forward(big, sd, ld + torch.tensor([0, 4], device='cuda'), loc[:1], aw[:1])


def test_empty_query_set_backward():
    """No queries: the forward gives an empty result and the backward (autograd included) adds nothing to
    grad_value, on both surfaces (the C entry point refuses non-positive sizes, so neither may call it)."""
    _, shapes, lsi, value, loc, aw, _ = _case(5, 2, 3, 32, _levels(2, 0), 4, 2, F32)
    value, shapes, lsi = _cuda(value, shapes, lsi)
    loc = torch.zeros(2, 0, 3, 2, 2, 2, device='cuda', requires_grad=True)
    aw = torch.zeros(2, 0, 3, 2, 2, device='cuda', requires_grad=True)
    v = value.clone().requires_grad_(True)
    out = ops.MultiScaleDeformableAttnFunction.apply(v, shapes, lsi, loc, aw, 2)
    assert out.shape == (2, 0, 96)
    out.sum().backward()
    assert torch.count_nonzero(v.grad) == 0 and loc.grad.shape == loc.shape and aw.grad.shape == aw.shape
    gout = torch.zeros(2, 0, 96, device='cuda')
    for fn in (ops.ms_deform_attn_backward, _ext().ms_deform_attn_backward):
        gv, _, _ = _backward(fn, (value, shapes, lsi, loc.detach(), aw.detach()), gout, value)
        assert torch.equal(gv, value)
