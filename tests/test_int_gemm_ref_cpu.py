"""The exact-integer anchor of the GEMM / convolution family on the CPU (tests/int_gemm_ref.py): every case of
the GPU sweep (tests/test_gemm_exact_gpu.py) meets the conditions under which all summation orders give the same
bits, the faults the sweep exists to catch do change an output of the family that claims to cover them, and the
sweep's shape list still reaches every kernel form it is meant to."""
import numpy as np
import pytest

from tests import int_gemm_ref as G

K_SMALL, K_LARGE = min(G.ROW_KS), max(G.ROW_KS)


@pytest.mark.parametrize('i', range(len(G.ROW_MS)))
def test_row_sweep_cases_meet_the_exactness_conditions(i):
    for M, K, N, n_out, fam, epi, _ in G.row_cases(i):
        n = n_out or N
        a, w = G.operands(fam, M, K, n)
        bias, res, a_bias, _ = G.epilogue_args(fam, epi, M, K, n)
        G.check_case(a, w, bias, res, a_bias, 3, fam)


def test_row_sweep_is_a_covering_set():
    """Every M edge meets every N class (with two families each), every family, every epilogue and every diag
    variant; every K meets every N class."""
    kn = set()
    for i, M in enumerate(G.ROW_MS):
        cases = G.row_cases(i)
        assert {(c[2], c[3]) for c in cases} == set(G.ROW_NS)
        assert {c[4] for c in cases} == set(G.FAMILIES)
        assert {c[5] for c in cases} == set(G.EPILOGUES)
        assert {c[6] for c in cases} == set(G.ROW_VARIANTS)
        assert len({(c[2], c[3], c[4]) for c in cases}) == 2 * len(G.ROW_NS)      # two families per N class
        kn |= {(c[1], c[2], c[3]) for c in cases}
    assert kn == {(K, N, n_out) for K in G.ROW_KS for N, n_out in G.ROW_NS}


@pytest.mark.parametrize('case', G.SPLITK_ROWS + tuple(c[:3] + c[4:6] for c in G.KSPLIT_ROWS), ids=str)
def test_split_k_and_k_split_cases_meet_the_exactness_conditions(case):
    M, K, N, fam, epi = case[:5]
    a, w = G.operands(fam, M, K, N)
    bias, res, a_bias, _ = G.epilogue_args(fam, epi, M, K, N)
    G.check_case(a, w, bias, res, a_bias, 3, fam)


@pytest.mark.parametrize('case', G.LN_CASES, ids=str)
def test_layernorm_cases_meet_the_exactness_conditions(case):
    M, K, fam = case[:3]
    a, w = G.operands(fam, M, K, 256)
    bias, res, _ = G.epilogue_operands(fam, M, K, 256)
    G.check_case(a, w, bias, res, None, 3, fam)


@pytest.mark.parametrize('case', G.CONV3_CASES + tuple(c[:7] + (True, True) for c in G.CONV3_SPLITK), ids=str)
def test_conv3x3_cases_meet_the_exactness_conditions(case):
    n, H, W, Cin, Cout, stride, fam, has_res, _ = case
    x, w = G.conv_operands(fam, n, H, W, Cin, Cout)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    bias, res, _ = G.epilogue_operands(fam, n * Ho * Wo, 9 * Cin, Cout)
    # (a 1 x 1 map sees the centre tap only: the family's products must show, not every tap)
    G.check_case(G.im2col(x, 3, stride, 1), G.conv_rows(w), bias, res if has_res else None, None, 3,
                 fam if H * W > 1 else None)


@pytest.mark.parametrize('fam,planes', [('P0', 1), ('A2', 2), ('P0', 'fp16'), ('H11', 'fp16')])
def test_reduced_plane_and_fp16_families_meet_the_exactness_conditions(fam, planes):
    for M, K, N in (G.F16_SHAPES if planes == 'fp16' else G.PLANE_SHAPES):
        a, w = G.operands(fam, M, K, N)
        bias, res, a_bias = G.epilogue_operands('P0' if planes != 'fp16' else fam, M, K, N)
        G.check_case(a, w, bias, None, None, planes, fam)
        if planes != 'fp16':      # the prologue form of the 1- / 2-plane kernels
            G.check_case(a, w, bias, res, a_bias, planes)
        if fam == 'H11':      # the stored half is exact: |out| <= 2048
            assert np.abs(G.expect(a, w, bias)).max() <= 2048


@pytest.mark.parametrize('M,K,N,rr,n_split,fam,variant', G.EX_CASES)
def test_ex_cases_meet_the_exactness_conditions(M, K, N, rr, n_split, fam, variant):
    a, w = G.operands(fam, M, K, N)
    bias, table, _ = G.epilogue_operands(fam, M, K, N, rows=rr)
    G.check_case(a, w, bias, table, None, 3, fam)
    assert len({tuple(r) for r in table}) == rr      # a table read one row off shows


@pytest.mark.parametrize('M,K1,K,N,fam,epi', G.CAT_CASES)
def test_cat_cases_meet_the_exactness_conditions(M, K1, K, N, fam, epi):
    a, w = G.operands(fam, M, K, N)
    bias, res, _, _ = G.epilogue_args(fam, epi, M, K, N)
    G.check_case(a, w, bias, res, None, 3, fam)
    assert K1 % 16 == 0 and K % 32 == 0


@pytest.mark.parametrize('M,K,Gn,gn,pad,fam', G.GROUPED_CASES)
def test_grouped_cases_meet_the_exactness_conditions(M, K, Gn, gn, pad, fam):
    a, ws = G.grouped_operands(fam, M, K, Gn, gn)
    bias, _, _ = G.epilogue_operands(fam, M, K, Gn * gn)
    for g in range(Gn):
        G.check_case(a[:, g * K:(g + 1) * K], ws[g], bias[g * gn:(g + 1) * gn], None, None, 3, fam)


@pytest.mark.parametrize('n,H,W,Cin,Cout,stride,fam', G.CONV1_CASES)
def test_conv1x1_cases_meet_the_exactness_conditions(n, H, W, Cin, Cout, stride, fam):
    a, w = G.operands(fam, n * H * W, Cin, Cout)
    bias, _, _ = G.epilogue_operands(fam, n * H * W, Cin, Cout)
    G.check_case(a, w, bias, None, None, 3, fam)


@pytest.mark.parametrize('n,H,W,fam,how', G.STEM_CASES)
def test_stem_cases_meet_the_exactness_conditions(n, H, W, fam, how):
    x, w = G.stem_operands(fam, n, H, W)
    bias, _, _ = G.epilogue_operands(fam, n * H * W, 147, 64)
    G.check_case(G.im2col(x, 7, 2, 3), G.conv_rows(w), bias, None, None, 3, fam)


@pytest.mark.parametrize('fam', G.FAMILIES)
def test_fp32_mfma_cases_meet_the_exactness_conditions(fam):
    """fp32 operands: the bound alone matters (every fp32 product of these integers is below 2^24)."""
    for n, H, W, Cin, Cout, stride in G.MFMA_CONV3:
        x, w = G.conv_operands(fam, n, H, W, Cin, Cout)
        bias, _, _ = G.epilogue_operands(fam, n * H * W, 9 * Cin, Cout)
        G.check_case(G.im2col(x, 3, stride, 1), G.conv_rows(w), bias, None, None, 3)
    for M, K, K2, N, epi in G.MFMA_ROWS:
        a, w = G.operands(fam, M, K + K2, N)
        bias, res, a_bias, _ = G.epilogue_args(fam, epi, M, K, N)
        full = np.concatenate([G.prologue(a[:, :K], a_bias), a[:, K:]], 1)
        G.check_case(full, w, bias, res, None, 3)
    for n, H, W in G.MFMA_C3:
        x, w = G.stem_operands(fam, n, H, W, 3)
        bias, _, _ = G.epilogue_operands(fam, n * H * W, 27, 64)
        G.check_case(G.im2col(x, 3, 2, 1), G.conv_rows(w), bias, None, None, 3)


def _small(fam, K, M=6, N=8):
    a, w = G.operands(fam, M, K, N, seed=3)
    G.check_case(a, w, None, None, None, 3, fam)
    return a, w


@pytest.mark.parametrize('K', [K_SMALL, K_LARGE])
@pytest.mark.parametrize('fam', G.FAMILIES)
def test_emulation_equals_the_integer_result_in_every_order(fam, K):
    """Natural, reversed and shuffled k order, and a split-K plan with a short last part: the same bits."""
    a, w = _small(fam, K)
    exp = G.expect(a, w)
    ks = np.arange(K)
    for order in (None, ks[::-1], np.random.default_rng(K).permutation(K)):
        assert np.array_equal(G.emulate(a, w, k_order=order).astype(np.float64), exp)
    assert np.array_equal(G.emulate_splitk(a, w, per=K // 16 // 4 + 1).astype(np.float64), exp)
    assert np.array_equal(G.emulate(a, w, G.ALL_PRODUCTS[::-1]).astype(np.float64), exp)


@pytest.mark.parametrize('K', [K_SMALL, K_LARGE])
@pytest.mark.parametrize('fam,product', [(f, p) for f in G.FAMILIES for p in G.PRODUCTS[f]])
def test_dropping_a_product_shows_in_the_family_that_claims_it(fam, product, K):
    a, w = _small(fam, K)
    rest = tuple(p for p in G.ALL_PRODUCTS if p != product)
    assert not np.array_equal(G.emulate(a, w, rest).astype(np.float64), G.expect(a, w))


def test_the_families_together_claim_all_six_products():
    assert {p for f in G.FAMILIES for p in G.PRODUCTS[f]} == set(G.ALL_PRODUCTS)


@pytest.mark.parametrize('K', [K_SMALL, K_LARGE])
@pytest.mark.parametrize('fam', G.FAMILIES)
def test_k_axis_and_epilogue_faults_show_in_every_family(fam, K):
    a, w = _small(fam, K)
    exp = G.expect(a, w)
    # the last K slab dropped
    assert not np.array_equal(G.emulate(a, w, k_order=range(K - 16)).astype(np.float64), exp)
    # the last split-K part dropped (a plan with a shorter last part, as K = 2208 has)
    assert not np.array_equal(G.emulate_splitk(a, w, K // 16 // 4 + 1, drop_last=True).astype(np.float64), exp)
    # two output columns swapped
    got = G.emulate(a, w)
    assert not np.array_equal(got[:, [1, 0] + list(range(2, got.shape[1]))].astype(np.float64), exp)
    # the residual table read one row off
    _, table, _ = G.epilogue_operands(fam, a.shape[0], K, w.shape[0], rows=5)
    m = np.arange(a.shape[0])
    assert not np.array_equal(got.astype(np.float64) + table[(m + 1) % 5], G.expect(a, w, None, table, residual_rows=5))
    assert np.array_equal(got.astype(np.float64) + table[m % 5], G.expect(a, w, None, table, residual_rows=5))


@pytest.mark.parametrize('K', [K_SMALL, K_LARGE])
def test_bf16_in_place_of_fp16_operands_shows_in_h11(K):
    a, w = G.operands('H11', 6, K, 8, seed=3)
    exp = G.expect(a, w)
    assert np.array_equal(G.emulate_fp16(a, w).astype(np.float64), exp)
    assert not np.array_equal(G.emulate_fp16(a, w, cut=G.bf16_trunc).astype(np.float64), exp)


def test_sweep_reaches_every_kernel_form():
    """ops.form_plan (a pure host function) over the sweep's (entry, M, K, N, policy): a shape list that stops
    reaching a form fails here.  Every form is reachable at the small shapes below: the wide LayerNorm form, which
    the shipped selection takes from 65 536 rows on, is what form policy 1 names at every M."""
    from pavenet_amd import ops
    order_name = {getattr(ops, 'ORDER_' + n): n for n in ('TILE', 'KSPLIT', 'SPLITK', 'TILE_LNPASS', 'KSPLIT_LNPASS',
                                                          'TILE_LN8')}
    reached = set()

    def plan(kind_name, M, K, N, policy):
        order, parts = ops.form_plan(M, K, N, getattr(ops, 'FORM_' + kind_name), policy)
        reached.add((kind_name, order_name[order], parts))
        return order_name[order], parts

    for i in range(len(G.ROW_MS)):
        for M, K, N, n_out, fam, epi, _ in G.row_cases(i):
            if epi != 'a_bias':      # (the prologue form keeps the tile kernels)
                for policy in (0, 1, 2):
                    plan('ROWS', M, K, n_out or N, policy)
    for M, K, N, policy, fam, epi, ksplit in G.KSPLIT_ROWS:
        assert plan('ROWS', M, K, N, policy)[0] == ('KSPLIT' if ksplit else 'TILE')
    for M, K, N, fam, epi, parts in G.SPLITK_ROWS:
        assert plan('ROWS_SPLITK', M, K, N, 0) == ('SPLITK', parts)
        assert plan('ROWS_SPLITK', M, K, N, 1)[1] == 1      # no parts under a form policy
    for M, K, fam, policy, variant, order in G.LN_CASES:
        if variant is None:
            assert plan('LN', M, K, 256, policy)[0] == order
    for n, H, W, Cin, Cout, stride, fam, _, _ in G.CONV3_CASES:
        assert plan('CONV3X3', n * ((H - 1) // stride + 1) * ((W - 1) // stride + 1), 9 * Cin, Cout, 0)[1] == 1
    for n, H, W, Cin, Cout, stride, fam, parts in G.CONV3_SPLITK:
        assert plan('CONV3X3', n * ((H - 1) // stride + 1) * ((W - 1) // stride + 1), 9 * Cin, Cout, 0) == \
            ('SPLITK', parts)
    need = {('ROWS', 'TILE', 1), ('ROWS', 'KSPLIT', 1),
            ('ROWS_SPLITK', 'SPLITK', 4), ('ROWS_SPLITK', 'SPLITK', 8), ('ROWS_SPLITK', 'SPLITK', 32),
            ('LN', 'TILE', 1), ('LN', 'TILE_LN8', 1), ('LN', 'TILE_LNPASS', 1), ('LN', 'KSPLIT_LNPASS', 1),
            ('CONV3X3', 'TILE', 1), ('CONV3X3', 'SPLITK', 4), ('CONV3X3', 'SPLITK', 8), ('CONV3X3', 'SPLITK', 32)}
    assert need <= reached, sorted(need - reached)
