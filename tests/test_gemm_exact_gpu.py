"""Every GEMM and convolution form against an exact integer reference (tests/int_gemm_ref.py).

On integer operands whose partial sums stay inside fp32's exact range every kernel form -- tile order, K-split
order, split-K parts + reduction, either generation, any tile shape -- must give the bits of the int64 result:
the comparisons below are torch.equal, the LayerNorm outputs excepted (rtol = atol = 2e-5, the budget of
test_gemm_bf16x3_layernorm_epilogue_vs_fp64 -- the GEMM in front of the row statistics contributes none of it).
tests/test_int_gemm_ref_cpu.py proves on the CPU that every case here meets the exactness conditions, that the
faults this sweep exists for would show, and which forms the shape lists reach.  Each case runs twice: the two
outputs must be equal (split-K parts are added in order by design)."""
import contextlib

import numpy as np
import pytest
import torch

from tests import int_gemm_ref as G

pytestmark = pytest.mark.gpu
SHIPPED = ((None, 0), (None, 1), (None, 2))      # the default build under every form policy


def _d(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _cl(x):
    """numpy NCHW -> device tensor in channels_last storage."""
    return _d(x).contiguous(memory_format=torch.channels_last)


def _rows_as_map(rows, n, H, W):
    """rows [n H W, C] -> NCHW numpy."""
    return np.ascontiguousarray(rows.reshape(n, H, W, -1).transpose(0, 3, 1, 2))


@contextlib.contextmanager
def _mode(variant, policy):
    from pavenet_amd import native, ops
    with contextlib.ExitStack() as st:
        if variant is not None:
            st.enter_context(native.diag_build(variant))
        st.enter_context(ops.form_policy(policy))
        yield


class _Sweep:
    """Runs cases under kernel-form modes and collects every mismatch, so that one run names them all."""

    def __init__(self):
        self.bad = []

    def exact(self, what, modes, run, *exps):
        exps = [torch.from_numpy(np.ascontiguousarray(e)).double() for e in exps]
        for variant, policy in modes:
            with _mode(variant, policy):
                first = run()
                second = run()
                torch.cuda.synchronize()
            first = first if isinstance(first, (tuple, list)) else (first,)
            second = second if isinstance(second, (tuple, list)) else (second,)
            for o1, o2, exp in zip(first, second, exps):
                got = o1.detach().cpu().double()
                tag = f'{what} [diag {variant}, policy {policy}]'
                if tuple(got.shape) != tuple(exp.shape):
                    self.bad.append(f'{tag}: shape {tuple(got.shape)} != {tuple(exp.shape)}')
                elif not torch.equal(got, exp):
                    d = (got - exp).abs()
                    self.bad.append(f'{tag}: {int((d != 0).sum())} of {d.numel()} differ, max |diff| {d.max().item():g} '
                                    f'at {tuple(int(v) for v in np.unravel_index(int(d.argmax()), d.shape))}')
                if not torch.equal(o1, o2):
                    self.bad.append(f'{tag}: two runs differ')

    def done(self):
        assert not self.bad, '\n'.join(self.bad)


def _epi_dev(fam, epi, M, K, n):
    bias, res, a_bias, relu = G.epilogue_args(fam, epi, M, K, n)
    return (bias, res, a_bias, relu), (_d(bias), _d(a_bias))


def _row_runner(ops, ad, wp, args, dev, epi, n_out=None):
    (bias, res, a_bias, relu), (bd, abd) = args, dev

    def run():
        r = _d(res)      # fresh: the in-place form overwrites it
        return ops.gemm_bf16x3(ad, wp, bd, r, relu=relu, out=r if epi == 'res_inplace' else None, a_bias=abd,
                               n_out=n_out)
    return run


@pytest.mark.parametrize('i', range(len(G.ROW_MS)), ids=lambda i: f'M{G.ROW_MS[i]}')
def test_row_gemm_every_edge_family_epilogue_and_form(i):
    """gemm_bf16x3 over the covering set of one M edge (int_gemm_ref.row_cases): default build under form policies
    0, 1 and 2 (from 2 049 rows on policy 2 is the multi-tile K-split form) and one diag variant per case."""
    from pavenet_amd import ops
    sw = _Sweep()
    for M, K, N, n_out, fam, epi, variant in G.row_cases(i):
        n = n_out or N
        a, w = G.operands(fam, M, K, n)
        args, dev = _epi_dev(fam, epi, M, K, n)
        exp = G.expect(a, w, args[0], args[1], args[2], args[3])
        wp = ops.split_weight_bf16x3(_d(w), pad=True)
        assert wp.shape[2] == N
        sw.exact(f'rows {M}x{K}x{n} {fam} {epi}', SHIPPED + ((variant, 0),),
                 _row_runner(ops, _d(a), wp, args, dev, epi, n_out), exp)
    sw.done()


@pytest.mark.parametrize('case', G.SPLITK_ROWS, ids=str)
def test_row_gemm_split_k_parts_and_reduction(case):
    """PAVE_ORDER_SPLITK of the plain row GEMM: 4, 8 and 32 parts, a shorter last part (K = 2208), bias / residual
    (in place too) / ReLU in the reduction launch; the same case without a plan (form policy 1, diag 6) and on the
    wide tiles (diag 7)."""
    from pavenet_amd import ops
    M, K, N, fam, epi, parts = case
    assert ops.form_plan(M, K, N, ops.FORM_ROWS_SPLITK, 0) == (ops.ORDER_SPLITK, parts)
    a, w = G.operands(fam, M, K, N)
    args, dev = _epi_dev(fam, epi, M, K, N)
    sw = _Sweep()
    sw.exact(f'split-K rows {M}x{K}x{N} {fam} {epi}', ((None, 0), (None, 1), (6, 0), (7, 0)),
             _row_runner(ops, _d(a), ops.split_weight_bf16x3(_d(w), pad=True), args, dev, epi),
             G.expect(a, w, args[0], args[1], args[2], args[3]))
    sw.done()


@pytest.mark.parametrize('case', G.KSPLIT_ROWS, ids=str)
def test_row_gemm_k_split_order(case):
    """PAVE_ORDER_KSPLIT: policy 0 at few rows, policy 2 at every M, slab counts off the multiple of 4, and the
    ksplit_order_applies edge (K = 256: N = 512 inside, N = 576 outside); diag 21 keeps the one-tile kernel above
    2 048 rows, diag 19 is the selection without the K-split form."""
    from pavenet_amd import ops
    M, K, N, policy, fam, epi, ksplit = case
    assert (ops.form_plan(M, K, N, ops.FORM_ROWS, policy)[0] == ops.ORDER_KSPLIT) == ksplit
    n_out = N if N % 64 else None
    a, w = G.operands(fam, M, K, N)
    args, dev = _epi_dev(fam, epi, M, K, N)
    sw = _Sweep()
    sw.exact(f'K-split rows {M}x{K}x{N} {fam} {epi}', ((None, policy), (21, policy), (19, policy)),
             _row_runner(ops, _d(a), ops.split_weight_bf16x3(_d(w), pad=True), args, dev, epi, n_out),
             G.expect(a, w, args[0], args[1], args[2], args[3]))
    sw.done()


@pytest.mark.parametrize('M,K,N,rr,n_split,fam,variant', G.EX_CASES)
def test_gemm_ex_row_table_and_two_outputs(M, K, N, rr, n_split, fam, variant):
    """gemm_bf16x3_ex: a row-periodic table whose period does not divide the tile (and one of >= M rows), two
    outputs cut at 128 / 256, wide tiles plus the narrow tail (N = 640) and N = 768."""
    from pavenet_amd import ops
    a, w = G.operands(fam, M, K, N)
    bias, table, _ = G.epilogue_operands(fam, M, K, N, rows=rr)
    exp = G.expect(a, w, bias, table[:M], relu=True, residual_rows=rr if rr < M else 0)
    exps = (exp[:, :n_split], exp[:, n_split:]) if n_split else (exp,)
    ad, wp, bd, td = _d(a), ops.split_weight_bf16x3(_d(w), pad=True), _d(bias), _d(table)

    def run():
        out, out2 = ops.gemm_bf16x3_ex(ad, wp, bd, td, residual_rows=rr, n_split=n_split, relu=True)
        return (out, out2) if n_split else out
    sw = _Sweep()
    sw.exact(f'ex {M}x{K}x{N} rows {rr} split {n_split} {fam}', SHIPPED + ((variant, 0),), run, *exps)
    sw.done()


@pytest.mark.parametrize('M,K1,K,N,fam,epi', G.CAT_CASES)
def test_gemm_cat_two_sources(M, K1, K, N, fam, epi):
    """gemm_bf16x3_cat: the K axis cut at K1 in {16, 48, 64} inside a 32-column step (K - K1 off the multiple of
    32), both sources dense matrices of their own."""
    from pavenet_amd import ops
    a, w = G.operands(fam, M, K, N)
    bias, res, _, relu = G.epilogue_args(fam, epi, M, K, N)
    a1d, a2d, wp, bd = _d(a[:, :K1]), _d(a[:, K1:]), ops.split_weight_bf16x3(_d(w), pad=True), _d(bias)

    def run():
        r = _d(res)
        return ops.gemm_bf16x3_cat(a1d, a2d, wp, bd, r, relu=relu, out=r if epi == 'res_inplace' else None)
    sw = _Sweep()
    sw.exact(f'cat {M}x({K1}+{K - K1})x{N} {fam} {epi}', SHIPPED + ((8, 0), (16, 0), (7, 0)), run,
             G.expect(a, w, bias, res, relu=relu))
    sw.done()


@pytest.mark.parametrize('M,K,Gn,gn,pad,fam', G.GROUPED_CASES)
def test_gemm_grouped_row_stride_and_narrow_groups(M, K, Gn, gn, pad, fam):
    """gemm_bf16x3_grouped: 64-column groups (the narrow-groups path) and 128- / 256-column ones, and through the C
    entry a row stride beyond G K (the columns between hold values that must not be read)."""
    from pavenet_amd import ops
    N = Gn * gn
    a, ws = G.grouped_operands(fam, M, K, Gn, gn)
    bias, _, _ = G.epilogue_operands(fam, M, K, N)
    exp = np.concatenate([G.expect(a[:, g * K:(g + 1) * K], ws[g], bias[g * gn:(g + 1) * gn], relu=True)
                          for g in range(Gn)], 1)
    lda = Gn * K + pad
    abuf = np.full((M, lda), 4097.0, dtype=np.float32)
    abuf[:, :Gn * K] = a
    ad, wp, bd = _d(abuf), ops.split_weight_bf16x3(_d(np.concatenate(ws, 0)), pad=True), _d(bias)

    def run():
        if not pad:
            return ops.gemm_bf16x3_grouped(ad, wp, bd, gn, relu=True)
        out = torch.empty((M, N), dtype=torch.float32, device='cuda')
        ops._launch('pave_gemm_bf16x3_grouped_f32', 'gemm_bf16x3_grouped', ad.device, ad.data_ptr(), lda,
                    wp.data_ptr(), bd.data_ptr(), out.data_ptr(), M, K, N, gn, 1, 3)
        return out
    sw = _Sweep()
    sw.exact(f'grouped {M}x{Gn}x{K}x{gn} lda {lda} {fam}', SHIPPED + ((8, 0), (19, 0)), run, exp)
    sw.done()


# ---- LayerNorm GEMM
def _ln_operands(M, K, fam):
    a, w = G.operands(fam, M, K, 256)
    bias, res, _ = G.epilogue_operands(fam, M, K, 256)
    rng = np.random.default_rng([M, K])
    gamma = rng.standard_normal(256).astype(np.float32)
    beta = rng.standard_normal(256).astype(np.float32)
    return a, w, bias, res, gamma, beta


@pytest.mark.parametrize('case', G.LN_CASES, ids=str)
def test_layernorm_gemm_on_an_exact_pre_norm_matrix(case):
    """gemm_bf16x3_ln in its wide, 8-wave, pass-after-tile-order and pass-after-K-split forms: the pre-norm
    matrix is the integer matrix exactly, so the whole 2e-5 is the row statistics' and the normalisation's."""
    from pavenet_amd import ops
    M, K, fam, policy, variant, order = case
    if order is not None:
        assert ops.form_plan(M, K, 256, ops.FORM_LN, policy)[0] == getattr(ops, 'ORDER_' + order)
    a, w, bias, res, gamma, beta = _ln_operands(M, K, fam)
    eps = 1e-5
    exp = G.layernorm64(G.expect(a, w, bias, res), gamma, beta, eps)
    ad, wp = _d(a), ops.split_weight_bf16x3(_d(w))
    bd, gd, bed = _d(bias), _d(gamma), _d(beta)
    with _mode(variant, policy):
        outs = []
        for inplace in (False, True, False):
            r = _d(res)
            outs.append(ops.gemm_bf16x3_ln(ad, wp, bd, r, gd, bed, eps, out=r if inplace else None))
        torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    np.testing.assert_allclose(outs[0].cpu().numpy(), exp, rtol=2e-5, atol=2e-5)


@pytest.mark.parametrize('M', [129, 4000])
def test_layernorm_gemm_constant_rows_give_beta_bit_for_bit(M):
    """a row zero, no bias, the residual a constant integer c per row (256 |c| < 2^24): the mean and the centred
    values are exact in every form, 0 * rsqrt(var + eps) is 0, so the output is beta bit for bit -- on 3 planes in
    every LayerNorm form and through gemm_fp16_act."""
    from pavenet_amd import ops
    K, eps = 256, 1e-5
    rng = np.random.default_rng(M)
    c = rng.integers(-65535, 65536, size=(M, 1)).astype(np.float32)
    c[:3, 0] = (65535, -65535, 0)
    res = np.repeat(c, 256, 1)
    _, w = G.operands('A3', M, K, 256)
    gamma = rng.standard_normal(256).astype(np.float32)
    beta = rng.standard_normal(256).astype(np.float32)
    ad, gd, bed = torch.zeros((M, K), device='cuda'), _d(gamma), _d(beta)
    wp, wh = ops.split_weight_bf16x3(_d(w)), ops.split_weight_bf16x3(_d(w), ops.PLANES_FP16)
    exp = np.repeat(beta[None, :], M, 0)
    sw = _Sweep()
    sw.exact(f'constant rows {M}', SHIPPED + ((13, 0), (14, 0), (19, 0), (9, 0), (21, 2)),
             lambda: ops.gemm_bf16x3_ln(ad, wp, None, _d(res), gd, bed, eps), exp)
    sw.exact(f'constant rows {M} fp16 operands', SHIPPED + ((13, 0), (14, 0)),
             lambda: ops.gemm_bf16x3_ln(ad, wh, None, _d(res), gd, bed, eps), exp)
    sw.exact(f'constant rows {M} fp16_act', ((None, 0),),
             lambda: ops.gemm_fp16_act(ad.half(), wh, None, residual=_d(res), ln=(gd, bed, eps)), exp)
    sw.done()


# ---- fp16 operand mode, fp16 activations, the 1- and 2-plane first-generation modes
@pytest.mark.parametrize('M,K,N', G.F16_SHAPES)
def test_fp16_operand_mode_and_fp16_activations(M, K, N):
    """PAVE_PLANES_FP16 on P0 and H11 (odd 11-bit integers: an operand cut to bf16 shows): the row GEMM on both
    generations, gemm_fp16_act with fp32 / fp16 activations in and an fp16 output (|out| <= 2048: the stored half
    is exact), and its LayerNorm form at the LayerNorm budget."""
    from pavenet_amd import ops
    sw = _Sweep()
    for fam in ('P0', 'H11'):
        a, w = G.operands(fam, M, K, N)
        bias, _, _ = G.epilogue_operands(fam, M, K, N)
        exp = G.expect(a, w, bias, relu=True)
        ad, bd = _d(a), _d(bias)
        wh = ops.split_weight_bf16x3(_d(w), ops.PLANES_FP16)
        sw.exact(f'fp16 rows {M}x{K}x{N} {fam}', SHIPPED + ((9, 0), (7, 0), (19, 0)),
                 lambda: ops.gemm_bf16x3(ad, wh, bd, relu=True, fp16=True), exp)
        for a_half in (False, True):
            ain = ad.half() if a_half else ad
            sw.exact(f'fp16_act {M}x{K}x{N} {fam} a16={a_half}', ((None, 0),),
                     lambda: ops.gemm_fp16_act(ain, wh, bd, relu=True), exp)
            if fam == 'H11':
                assert np.abs(exp).max() <= 2048
                sw.exact(f'fp16_act {M}x{K}x{N} {fam} a16={a_half} o16', ((None, 0),),
                         lambda: ops.gemm_fp16_act(ain, wh, bd, relu=True, out_half=True), exp)
        if N == 256:
            _, res, _ = G.epilogue_operands(fam, M, K, N)
            rng = np.random.default_rng(K)
            gamma, beta = rng.standard_normal(256).astype(np.float32), rng.standard_normal(256).astype(np.float32)
            expln = G.layernorm64(G.expect(a, w, bias, res), gamma, beta, 1e-5)
            for ain in (ad, ad.half()):
                got = ops.gemm_fp16_act(ain, wh, bd, residual=_d(res), ln=(_d(gamma), _d(beta), 1e-5))
                np.testing.assert_allclose(got.cpu().numpy(), expln, rtol=2e-5, atol=2e-5)
    sw.done()


@pytest.mark.parametrize('planes,fam', [(1, 'P0'), (2, 'A2')])
@pytest.mark.parametrize('M,K,N', G.PLANE_SHAPES)
def test_one_and_two_plane_first_generation_modes(planes, fam, M, K, N):
    """1 plane on P0 (bf16 values), 2 planes on the 9-bit a of X2 against P0's w (a0 b0 + a1 b0; the products a
    2-plane kernel leaves out are zero)."""
    from pavenet_amd import ops
    a, w = G.operands(fam, M, K, N)
    sw = _Sweep()
    for epi in ('res', 'a_bias'):
        args, dev = _epi_dev('P0', epi, M, K, N)
        sw.exact(f'{planes} planes {M}x{K}x{N} {epi}', ((None, 0), (2, 0)),
                 _row_runner(ops, _d(a), ops.split_weight_bf16x3(_d(w), planes), args, dev, epi),
                 G.expect(a, w, args[0], args[1], args[2], args[3]))
    sw.done()


# ---- convolutions through the same kernels
def _conv3_modes(Cin, Cout, has_res):
    modes = SHIPPED + ((17, 0), (5, 0), (15, 0), (16, 0), (8, 0))
    return modes + (((9, 0),) if Cin % 64 == 0 and Cout % 64 == 0 and not has_res else ())


@pytest.mark.parametrize('case', G.CONV3_CASES, ids=str)
def test_conv3x3_split_exact(case):
    """conv3x3_split at stride 1 and 2, padded Cin / Cout (the half-tail form at 33 .. 48 columns against diag 17),
    with and without residual, on 1 x 1, 1 x W and odd maps."""
    from pavenet_amd import ops
    n, H, W, Cin, Cout, stride, fam, has_res, relu = case
    x, w = G.conv_operands(fam, n, H, W, Cin, Cout)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    bias, res, _ = G.epilogue_operands(fam, n * Ho * Wo, 9 * Cin, Cout)
    resm = _rows_as_map(res, n, Ho, Wo) if has_res else None
    exp = G.expect_conv(x, w, bias, resm, relu, stride, 1)
    xd, wp, bd = _cl(x), ops.split_conv3x3_weight(_d(w)), _d(bias)
    rd = _cl(resm) if has_res else None
    sw = _Sweep()
    sw.exact(f'conv3x3 {case}', _conv3_modes(Cin, Cout, has_res),
             lambda: ops.conv3x3_split(xd, wp, bd, stride=stride, relu=relu, residual=rd,
                                       cout=Cout if Cout % 64 else None), exp)
    sw.done()


@pytest.mark.parametrize('case', G.CONV3_SPLITK, ids=str)
def test_conv3x3_split_k_exact(case):
    """conv3x3_splitk: 4, 8 and 32 parts (K = 9 * 240 is padded to the 32-column step), bias + residual + ReLU in the
    reduction launch; the same shapes without a plan (policy 1, diag 6)."""
    from pavenet_amd import ops
    n, H, W, Cin, Cout, stride, fam, parts = case
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    assert ops.form_plan(n * Ho * Wo, 9 * Cin, Cout, ops.FORM_CONV3X3, 0) == (ops.ORDER_SPLITK, parts)
    x, w = G.conv_operands(fam, n, H, W, Cin, Cout)
    bias, res, _ = G.epilogue_operands(fam, n * Ho * Wo, 9 * Cin, Cout)
    resm = _rows_as_map(res, n, Ho, Wo)
    xd, wp, bd, rd = _cl(x), ops.split_conv3x3_weight(_d(w)), _d(bias), _cl(resm)
    sw = _Sweep()
    sw.exact(f'conv3x3 split-K {case}', ((None, 0), (None, 1), (6, 0)),
             lambda: ops.conv3x3_split(xd, wp, bd, stride=stride, relu=True, residual=rd,
                                       cout=Cout if Cout % 64 else None),
             G.expect_conv(x, w, bias, resm, True, stride, 1))
    sw.done()


@pytest.mark.parametrize('n,H,W,Cin,Cout,stride,fam', G.CONV1_CASES)
def test_conv1x1_strided_split_exact(n, H, W, Cin, Cout, stride, fam):
    from pavenet_amd import ops
    a, w = G.operands(fam, n * H * W, Cin, Cout)
    bias, _, _ = G.epilogue_operands(fam, n * H * W, Cin, Cout)
    x = _rows_as_map(a, n, H, W)
    exp = G.expect_conv(x, w.reshape(Cout, Cin, 1, 1), bias, None, True, stride, 0)
    xd, wp, bd = _cl(x), ops.split_weight_bf16x3(_d(w)), _d(bias)
    sw = _Sweep()
    sw.exact(f'conv1x1 s{stride} {n}x{H}x{W} {Cin}->{Cout} {fam}', SHIPPED + ((9, 0), (7, 0), (8, 0)),
             lambda: ops.conv1x1_strided_split(xd, wp, bd, stride=stride, relu=True), exp)
    sw.done()


@pytest.mark.parametrize('form', ['identity_next64', 'identity_inplace_next128', 'downsample_next64',
                                  'identity_last', 'tail_downsample_next128'])
def test_bottleneck_chain_exact(form):
    """bottleneck_chain on an odd map of two ragged 128-pixel tiles: every stage's input is an integer map inside
    the bound (c2 has 8 bits, the 256-channel output behind an identity 17 or more: the next conv1 sees all three
    A planes), so the output and the chained conv1 are the fp64 convolutions' integers; default, diag 15 and 16."""
    from pavenet_amd import ops
    F = torch.nn.functional
    n, H, W = 2, 9, 11
    rng = np.random.default_rng(len(form))
    down = 'downsample' in form
    k2 = 64 if down else 0
    cn = 0 if form.endswith('last') else (128 if form.endswith('128') else 64)
    c1 = rng.integers(0, 16, size=(n, 64, H, W)).astype(np.float32)
    w2 = np.ascontiguousarray(G._sparse_signs(rng, 64, 576, 16).reshape(64, 3, 3, 64).transpose(0, 3, 1, 2))
    b2 = rng.integers(-15, 16, size=64).astype(np.float32)
    w3 = rng.integers(-15, 16, size=(256, 64 + k2)).astype(np.float32)
    b3 = rng.integers(-15, 16, size=256).astype(np.float32)
    # (the identity has 17 bits: the chained conv1 then sees all three A planes; a downsample source is small)
    x_in = rng.integers(-15, 16, size=(n, 64, H, W)).astype(np.float32) if down else \
        np.abs(G._wide(rng, (n, 256, H, W), 16))
    w1n = G._sparse_signs(rng, cn, 256, 40) if cn else None
    b1n = rng.integers(-15, 16, size=cn).astype(np.float32) if cn else None
    t = lambda v: torch.from_numpy(v).double()      # noqa: E731
    c2 = torch.relu(F.conv2d(t(c1), t(w2), t(b2), 1, 1))
    assert c2.max() <= 255
    rows = lambda m: m.permute(0, 2, 3, 1).reshape(-1, m.shape[1]).numpy().astype(np.float32)      # noqa: E731
    a3 = np.concatenate([rows(c2), rows(t(x_in))], 1) if down else rows(c2)
    G.check_case(a3, w3, b3, None if down else rows(t(x_in)), None, 3)
    exp_out = G.expect(a3, w3, b3, None if down else rows(t(x_in)), relu=True)
    exps = [_rows_as_map(exp_out, n, H, W)]
    if cn:
        G.check_case(exp_out.astype(np.float32), w1n, b1n, None, None, 3, 'A2' if down else 'A3')
        exps.append(_rows_as_map(G.expect(exp_out.astype(np.float32), w1n, b1n, relu=True), n, H, W))
    c1d, w2p, b2d = _cl(c1), ops.split_conv3x3_weight(_d(w2)), _d(b2)
    w3p, b3d, xd = ops.split_weight_bf16x3(_d(w3)), _d(b3), _cl(x_in)
    w1np, b1nd = (ops.split_weight_bf16x3(_d(w1n)), _d(b1n)) if cn else (None, None)
    inplace, tail = 'inplace' in form, form.startswith('tail')
    c2d = _cl(c2.numpy().astype(np.float32))

    def run():
        res = xd.clone(memory_format=torch.channels_last) if inplace else xd
        out, c1n = ops.bottleneck_chain(None if tail else c1d, None if tail else w2p, None if tail else b2d, w3p, b3d,
                                        residual=None if down else res, a2=xd if down else None, w1n_planes=w1np,
                                        b1n=b1nd, out=res if inplace else None, c2=c2d if tail else None)
        return (out, c1n) if cn else out
    sw = _Sweep()
    sw.exact(f'chain {form}', ((None, 0), (15, 0), (16, 0)), run, *exps)
    sw.done()


@pytest.mark.parametrize('n,H,W,fam,how', G.STEM_CASES)
def test_stem_conv7x7_exact(n, H, W, fam, how):
    """conv7x7s2_nchw_split, both kernels: W % 4 == 0 (the LDS-window kernel; W = 100 has a ragged second segment),
    an odd W dense (the per-lane window kernel) and through repitch_rows, and W % 4 == 0 at an image that starts
    off the 16-byte grid (the per-lane kernel again); diag 9 keeps the per-lane kernel wherever the rows are
    dense."""
    from pavenet_amd import ops
    x, w = G.stem_operands(fam, n, H, W)
    bias, _, _ = G.epilogue_operands(fam, n * H * W, 147, 64)
    exp = G.expect_conv(x, w, bias, None, True, 2, 3)
    wp, bd = ops.split_stem7x7_weight(_d(w)), _d(bias)
    if how == 'misaligned':
        buf = torch.zeros(x.size + 1, device='cuda')
        xd = buf[1:].view(x.shape)
        xd.copy_(_d(x))
        assert xd.data_ptr() % 16 == 4
    else:
        xd = _d(x)
    if how == 'repitch':
        xp = ops.repitch_rows(xd)
        run = lambda: ops.conv7x7s2_nchw_split(xp, wp, bd, relu=True, valid_w=W)      # noqa: E731
    else:
        run = lambda: ops.conv7x7s2_nchw_split(xd, wp, bd, relu=True)      # noqa: E731
    sw = _Sweep()
    sw.exact(f'stem {n}x{H}x{W} {fam} {how}', ((None, 0), (9, 0)), run, exp)
    sw.done()


@pytest.mark.parametrize('fam', G.FAMILIES)
def test_fp32_mfma_kernels_exact(fam):
    """The fp32-MFMA kernels on the same integers (fp32 products of these operands are exact): conv3x3_nhwc at
    stride 1 and 2, rows_gemm_bias_res_act with its prologue and second source, and conv3x3s2_c3_nchw."""
    from pavenet_amd import ops
    sw = _Sweep()
    for n, H, W, Cin, Cout, stride in G.MFMA_CONV3:
        x, w = G.conv_operands(fam, n, H, W, Cin, Cout)
        bias, _, _ = G.epilogue_operands(fam, n * H * W, 9 * Cin, Cout)
        taps = _d(np.ascontiguousarray(w.transpose(2, 3, 1, 0)))
        xd, bd = _cl(x), _d(bias)
        sw.exact(f'conv3x3_nhwc {n}x{H}x{W} {Cin}->{Cout} s{stride} {fam}', ((None, 0),),
                 lambda: ops.conv3x3_nhwc(xd, taps, bd, stride=stride, relu=True),
                 G.expect_conv(x, w, bias, None, True, stride, 1))
    for M, K, K2, N, epi in G.MFMA_ROWS:
        a, w = G.operands(fam, M, K + K2, N)
        bias, res, a_bias, relu = G.epilogue_args(fam, epi, M, K, N)
        a1, a2 = a[:, :K], (a[:, K:] if K2 else None)
        full = np.concatenate([G.prologue(a1, a_bias), a2], 1) if K2 else G.prologue(a1, a_bias)
        a1d, a2d, wd, bd, abd = _d(a1), _d(a2), _d(np.ascontiguousarray(w.T)), _d(bias), _d(a_bias)

        def run():
            r = _d(res)
            return ops.rows_gemm_bias_res_act(a1d, wd, bd, r, relu=relu, out=r if epi == 'res_inplace' else None,
                                              a_bias=abd, a2=a2d)
        sw.exact(f'rows_gemm {M}x({K}+{K2})x{N} {fam} {epi}', ((None, 0),), run,
                 G.expect(full, w, bias, res, relu=relu))
    for n, H, W in G.MFMA_C3:
        x, w = G.stem_operands(fam, n, H, W, 3)
        bias, _, _ = G.epilogue_operands(fam, n * H * W, 27, 64)
        xd, bd = _d(x), _d(bias)
        taps = _d(np.ascontiguousarray(w.transpose(1, 2, 3, 0).reshape(27, 64)))
        sw.exact(f'conv3x3s2_c3 {n}x{H}x{W} {fam}', ((None, 0),),
                 lambda: ops.conv3x3s2_c3_nchw(xd, taps, bd, relu=True), G.expect_conv(x, w, bias, None, True, 2, 1))
    sw.done()
