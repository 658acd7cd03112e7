"""Exact-integer anchor of the split GEMM / convolution family: operand generators, the conditions under which
every summation order gives the same fp32 bits, the int64-exact expected values, and an fp32 emulation of the
six-product accumulation (numpy / torch on the CPU only; tests/test_int_gemm_ref_cpu.py, tests/test_gemm_exact_gpu.py).

Why a zero tolerance holds.  The kernels split an activation by truncation (csrc/pave_gemm_split.hip): planes of
the value's own sign, so sum_i |a_i| == |a|.  The three weight planes are ROUNDED terms (split_bf16x3_kernel: with both
operands truncated the products a kernel leaves out would all have the sign of a b), so they may differ in sign and
sum_j |w_j| can exceed |w| by up to 2^-7 |w|.  The planes of an integer are integers either way, and a product of two
bf16 (or fp16) values is exact in the matrix core's fp32 datapath.  Every partial sum of any subset of the plane
products, in any order, is then an integer of magnitude <= sum_k |a_ik| sum_j |w_j|_jk (+ |bias| + |residual|).  Where
that bound is <= 2^24 no addition rounds, whatever the kernel's tile order, K-split or split-K plan: the output IS the
integer result, provided the products the kernel does not compute (a1 b2 + a2 b1 + a2 b2 with three planes) are zero.
"""
import numpy as np
import torch

EXACT = float(1 << 24)
FAMILIES = ('P0', 'A3', 'W3', 'X2')
# the plane products (i, j) = a_i * b_j a family is meant to exercise
PRODUCTS = {
    'P0': ((0, 0),),
    'A3': ((0, 0), (1, 0), (2, 0)),
    'W3': ((0, 0), (0, 1), (0, 2)),
    'X2': ((0, 1), (1, 0), (1, 1)),
    'A2': ((0, 0), (1, 0)),     # the 2-plane first-generation mode: X2's 9-bit a on P0's w
    'H11': (),                  # fp16 operands: one plane
}
ALL_PRODUCTS = ((0, 0), (0, 1), (1, 0), (0, 2), (1, 1), (2, 0))      # what a 3-plane kernel computes
COMPUTED = {3: ALL_PRODUCTS, 2: ((0, 0), (0, 1), (1, 0)), 1: ((0, 0),)}
A3_NNZ, X2_NNZ = 120, 60      # non-zeros per sparse row (the issue's caps are 128 and 64; the slack pays for the
#                               a_bias prologue, which raises |a'| by up to 15)
W3_NNZ = 40                   # W3's sparse a: its weights have 18 bits (a rounded split puts 17 into two planes), and
#                               the four columns that are always non-zero weigh more in the 3x3 / 7x7 forms' rows


def _hi16(x):
    return (np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) & np.uint32(0xffff0000)).view(np.float32)


def _rne16(x):
    """x rounded to nearest even at bf16 (finite values below the largest bf16)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return ((u + np.uint32(0x7fff) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xffff0000)).view(np.float32)


def split3_w(x):
    """The split of a WEIGHT (csrc/pave_gemm_split.hip, split_bf16x3_kernel with three planes) on the host: two
    rounded terms and the exact remainder, x == p0 + p1 + p2, each a bf16 value."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    p0 = _rne16(x)
    r1 = x - p0
    p1 = _rne16(r1)
    p2 = r1 - p1
    assert np.array_equal(_hi16(p2), p2)
    return p0, p1, p2


def split3(x):
    """The truncation split of an ACTIVATION (csrc/pave_gemm_split.hip, and of the weights of the 2-plane mode) on
    the host: x == p0 + p1 + p2, each a bf16 value."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    p0 = _hi16(x)
    r1 = x - p0
    p1 = _hi16(r1)
    p2 = r1 - p1
    return p0, p1, p2


def bf16_trunc(x):
    """x cut to bf16 (what an fp16 operand would become in a kernel that took the bf16 path by mistake)."""
    return _hi16(x)


def _sparse_signs(rng, rows, K, nnz):
    """[rows, K] in {-1, 0, 1} with at most `nnz` non-zeros per row; k = 0, K - 1 and both sides of the first
    16-slab boundary (k = 15, 16) are always non-zero, the rest fall at random."""
    s = np.zeros((rows, K), dtype=np.float32)
    extra = max(0, min(nnz - 4, K // 2))
    if extra:
        pos = rng.integers(0, K, size=(rows, extra))
        np.put_along_axis(s, pos, rng.choice(np.float32([-1, 1]), size=(rows, extra)), axis=1)
    for k in (0, 15, 16, K - 1):
        s[:, k] = rng.choice(np.float32([-1, 1]), size=rows)
    return s


def _wide(rng, shape, bits):
    """+-(2^bits + odd r), r < 2^bits: bits + 1 significant bits, the lowest set."""
    r = rng.integers(0, 1 << (bits - 1), size=shape) * 2 + 1
    return ((1 << bits) + r).astype(np.float32) * rng.choice(np.float32([-1, 1]), size=shape)


def operands(family, M, K, N, seed=0):
    """fp32 a [M, K] and w [N, K] of a family, holding integers."""
    rng = np.random.default_rng([seed, M, K, N, sum(map(ord, family))])
    if family == 'P0':
        a = rng.integers(-15, 16, size=(M, K)).astype(np.float32)
        w = rng.integers(-15, 16, size=(N, K)).astype(np.float32)
    elif family == 'A3':
        a, w = _wide(rng, (M, K), 16), _sparse_signs(rng, N, K, A3_NNZ)
    elif family == 'W3':
        a, w = _sparse_signs(rng, M, K, W3_NNZ), _wide(rng, (N, K), 17)
    elif family == 'X2':
        a = _wide(rng, (M, K), 8)
        w = _sparse_signs(rng, N, K, X2_NNZ) * np.abs(_wide(rng, (N, K), 8))
    elif family == 'A2':
        a = _wide(rng, (M, K), 8)
        w = rng.integers(-15, 16, size=(N, K)).astype(np.float32)
    elif family == 'H11':
        a = (rng.integers(512, 1024, size=(M, K)) * 2 + 1).astype(np.float32)          # odd, 1025 .. 2047
        # +1 / -1 pairs: |a_k1 - a_k2| <= 1022 per pair, two pairs in the odd rows -> |out| <= 2044 (+ bias <= 4)
        w = np.zeros((N, K), dtype=np.float32)
        fixed = ((0, K - 1), (15, 16))
        for j in range(N):
            k1, k2 = fixed[j % 2] if j % 4 < 2 else rng.choice(K, size=2, replace=False)
            w[j, k1], w[j, k2] = 1, -1
            if j % 2:
                k3, k4 = rng.choice(np.setdiff1d(np.arange(K), (k1, k2)), size=2, replace=False)
                w[j, k3], w[j, k4] = 1, -1
    else:
        raise ValueError(family)
    return a, w


def epilogue_operands(family, M, K, N, seed=0, rows=None):
    """Small-integer bias [N], residual [rows or M, N] and a_bias [K] that keep a family inside its bound."""
    rng = np.random.default_rng([seed, M, K, N, 7])
    lim = 4 if family == 'H11' else 15
    bias = rng.integers(-lim, lim + 1, size=N).astype(np.float32)
    res = rng.integers(-15, 16, size=(rows or M, N)).astype(np.float32)
    if family == 'W3':      # a in {-1, 0, 1}: relu(a + a_bias) stays sparse only for a_bias in {-1, 0}
        a_bias = -rng.integers(0, 2, size=K).astype(np.float32)
    else:
        a_bias = rng.integers(-15, 16, size=K).astype(np.float32)
    return bias, res, a_bias


def prologue(a, a_bias=None):
    return a if a_bias is None else np.maximum(a + a_bias[None, :], 0).astype(np.float32)


def check_case(a, w, bias=None, residual=None, a_bias=None, planes=3, family=None):
    """Asserts what makes exactness independent of the kernel form (conditions, not measurements): the magnitude
    bound, integer operands, zero dropped products for the plane count (3 | 2 | 1 | 'fp16'), and a non-zero
    instance of every product `family` is meant to exercise."""
    ap = prologue(a, a_bias)
    for name, t in (('a', ap), ('w', w), ('bias', bias), ('residual', residual)):
        assert t is None or np.array_equal(t, np.rint(t)), f'{name}: integers only'
    # (three planes: the rounded weight terms may differ in sign -- the partial sums are bounded by sum_j |w_j|)
    wmag = np.abs(w) if planes != 3 else sum(np.abs(p) for p in split3_w(w))
    bound = np.abs(ap).astype(np.float64) @ wmag.astype(np.float64).T
    bound = bound + (0 if bias is None else np.abs(bias)[None, :])
    bound = bound.max() + (0 if residual is None else np.abs(residual).max())
    assert bound <= EXACT, f'sum |a||w| + |bias| + |res| = {bound} > 2^24'
    if planes == 'fp16':
        for name, t in (('a', ap), ('w', w)):
            assert np.array_equal(t.astype(np.float16).astype(np.float32), t), f'{name}: not an fp16 value'
        return bound
    sa, sw = split3(ap), (split3_w if planes == 3 else split3)(w)
    assert np.array_equal(sa[0] + sa[1] + sa[2], ap) and np.array_equal(sw[0] + sw[1] + sw[2], w)
    live_a = [bool(p.any()) for p in sa]
    live_w = [bool(p.any()) for p in sw]
    for i in range(3):
        for j in range(3):
            if (i, j) not in COMPUTED[planes]:
                assert not (live_a[i] and live_w[j]), f'dropped product a{i} b{j} is not identically zero'
    for i, j in PRODUCTS.get(family, ()):
        hit = (sa[i] != 0).any(0) & (sw[j] != 0).any(0)       # some k with a_i[., k] != 0 and b_j[., k] != 0
        assert hit.any(), f'{family}: product a{i} b{j} is zero everywhere'
    return bound


def expect(a, w, bias=None, residual=None, a_bias=None, relu=False, a2=None, residual_rows=0):
    """act([a' | a2] W^T + bias + residual) in fp64 (every value an integer below 2^53: identical to int64).
    residual_rows > 0: the residual is a table, row m adds residual[m % residual_rows]."""
    ap = prologue(a, a_bias)
    if a2 is not None:
        ap = np.concatenate([ap, a2], 1)
    out = torch.from_numpy(ap).double() @ torch.from_numpy(np.ascontiguousarray(w)).double().t()
    out = out.numpy()
    if bias is not None:
        out = out + bias[None, :].astype(np.float64)
    if residual is not None:
        r = residual.astype(np.float64)
        out = out + (r[np.arange(out.shape[0]) % residual_rows] if residual_rows else r)
    return np.maximum(out, 0) if relu else out


def expect_conv(x, w, bias=None, residual=None, relu=False, stride=1, padding=1):
    """The convolution counterpart: F.conv2d in fp64 on integer images / weights (NCHW)."""
    out = torch.nn.functional.conv2d(torch.from_numpy(x).double(), torch.from_numpy(w).double(),
                                     None if bias is None else torch.from_numpy(bias).double(), stride, padding)
    if residual is not None:
        out = out + torch.from_numpy(residual).double()
    return (torch.relu(out) if relu else out).numpy()


def layernorm64(x, gamma, beta, eps):
    x = np.asarray(x, dtype=np.float64)
    mu = x.mean(1, keepdims=True)
    var = ((x - mu) ** 2).mean(1, keepdims=True)
    return (x - mu) / np.sqrt(var + eps) * gamma[None, :].astype(np.float64) + beta[None, :].astype(np.float64)


def emulate(a, w, products=ALL_PRODUCTS, k_order=None, planes_of=None):
    """fp32 accumulation of the plane products a_i[:, k] b_j[:, k] over k in `k_order` (default: natural), the
    products of one k in the order given: what a kernel that sums in this order computes.  planes_of: the split of
    both operands (default: the 3-plane kernels' -- activations truncated, weights rounded)."""
    sa, sw = (split3(a), split3_w(w)) if planes_of is None else (planes_of(a), planes_of(w))
    acc = np.zeros((a.shape[0], w.shape[0]), dtype=np.float32)
    for k in (range(a.shape[1]) if k_order is None else k_order):
        for i, j in products:
            acc = acc + sa[i][:, k, None] * sw[j][None, :, k]
    return acc


def emulate_fp16(a, w, cut=None):
    """One plane of fp16 operands, fp32 accumulation.  cut: applied to `a` first (bf16_trunc: the fault)."""
    a16 = (a if cut is None else cut(a)).astype(np.float16).astype(np.float32)
    one = lambda x: (x,)      # noqa: E731
    return emulate(a16, w.astype(np.float16).astype(np.float32), ((0, 0),), planes_of=one)


def emulate_splitk(a, w, per, drop_last=False, products=ALL_PRODUCTS):
    """Split-K: parts of `per` 16-wide slabs summed on their own, then added in order (the reduction launch)."""
    K = a.shape[1]
    starts = list(range(0, K, per * 16))
    if drop_last:
        starts = starts[:-1]
    acc = np.zeros((a.shape[0], w.shape[0]), dtype=np.float32)
    for s in starts:
        acc = acc + emulate(a, w, products, range(s, min(K, s + per * 16)))
    return acc


# ---- the GPU sweep's shape lists (tests/test_gemm_exact_gpu.py runs them, tests/test_int_gemm_ref_cpu.py checks
# ---- their bounds on the CPU and the kernel forms they reach)
ROW_MS = (1, 31, 32, 33, 127, 128, 129, 255, 256, 257, 2048, 2049, 2100)
ROW_KS = (64, 96, 192, 256, 512, 1024)
ROW_NS = ((64, None), (128, None), (256, None), (384, None), (512, None), (640, None),   # (N of the planes, n_out)
          (64, 36), (64, 48), (128, 96), (320, 300))
EPILOGUES = ('none', 'bias', 'res', 'res_inplace', 'relu', 'a_bias')
ROW_VARIANTS = (9, 8, 7, 19, 15, 16)


def row_cases(i):
    """The covering set of the i-th M of ROW_MS: twenty cases (M, K, N, n_out, family, epilogue, variant), two per
    N class, so that over them M meets every N class, every family, every epilogue and every diag variant (the
    first generation's included); the pairings rotate with i, so every K of ROW_KS meets every N class over the
    M list."""
    M = ROW_MS[i]
    out = []
    for r in range(2):
        for j, (N, n_out) in enumerate(ROW_NS):
            K = ROW_KS[(i + j + 3 * r) % 6]
            fam = FAMILIES[(i + j + 2 * r) % 4]
            epi = EPILOGUES[(i + j // 4 + 2 * j + 3 * r) % 6]
            out.append((M, K, N, n_out, fam, epi, variant_for(ROW_VARIANTS[(2 * i + j + 3 * r) % 6], K, N, n_out)))
    if all(c[6] != 9 for c in out):      # the first generation at every M: on the first shape it takes
        j = next(j for j, c in enumerate(out) if variant_for(9, c[1], c[2], c[3]) == 9)
        out[j] = out[j][:6] + (9,)
    return out


def variant_for(v, K, N, n_out):
    """v, or the next diag variant of ROW_VARIANTS whose kernels take the shape: the first generation (9) has
    K % 64 == 0, N % 128 == 0 (or N == 64) and no padded width."""
    if v == 9 and (K % 64 or n_out is not None or (N % 128 and N != 64)):
        return 8
    return v


def epilogue_args(family, epi, M, K, n, seed=0):
    """(bias, residual, a_bias, relu) as numpy arrays / None for an epilogue name; n = the real output width."""
    bias, res, a_bias = epilogue_operands(family, M, K, n, seed)
    return {'none': (None, None, None, False), 'bias': (bias, None, None, False), 'res': (bias, res, None, False),
            'res_inplace': (None, res, None, True), 'relu': (bias, None, None, True),
            'a_bias': (bias, res, a_bias, True)}[epi]


# split-K of the plain row GEMM: (M, K, N, family, epilogue, parts expected from the plan)
SPLITK_ROWS = ((129, 2048, 256, 'P0', 'res_inplace', 4), (300, 2048, 128, 'A3', 'relu', 4),
               (257, 2208, 256, 'X2', 'res', 4), (33, 2208, 320, 'W3', 'bias', 4),
               (130, 8192, 256, 'P0', 'res', 32), (65, 8192, 64, 'A3', 'res_inplace', 32),
               (641, 8192, 384, 'W3', 'relu', 8), (385, 8192, 1024, 'A3', 'none', 8))
# K-split order: (M, K, N, policy, family, epilogue, K-split order expected)
KSPLIT_ROWS = ((33, 288, 256, 0, 'A3', 'res', True), (129, 544, 128, 0, 'W3', 'relu', True),
               (257, 608, 640, 0, 'X2', 'bias', True), (31, 256, 512, 0, 'P0', 'res_inplace', True),
               (300, 256, 512, 2, 'A3', 'res', True), (300, 256, 576, 2, 'A3', 'res', False),
               (2049, 288, 512, 2, 'X2', 'relu', True), (2100, 544, 384, 2, 'W3', 'none', True),
               (2049, 608, 96, 2, 'A3', 'bias', True))
# LayerNorm GEMM (N = 256): (M, K, family, policy, diag variant or None, order expected of the shipped selection)
LN_CASES = ((129, 64, 'P0', 0, None, 'TILE_LNPASS'), (257, 512, 'A3', 0, None, 'KSPLIT_LNPASS'),
            (4000, 64, 'X2', 0, None, 'TILE_LN8'), (333, 256, 'W3', 1, None, 'TILE'),
            (300, 1024, 'A3', 2, None, 'KSPLIT_LNPASS'), (2100, 512, 'X2', 2, None, 'KSPLIT_LNPASS'),
            (255, 192, 'A3', 0, 13, None), (255, 192, 'W3', 0, 14, None), (129, 256, 'P0', 0, 19, None))
# conv3x3_split: (n, H, W, Cin, Cout, stride, family, residual, relu)
CONV3_CASES = ((2, 7, 9, 16, 36, 1, 'P0', True, True), (1, 1, 1, 48, 48, 1, 'A3', False, False),
               (1, 1, 13, 64, 64, 2, 'X2', True, False), (2, 5, 7, 96, 96, 1, 'W3', False, True),
               (1, 9, 11, 64, 256, 2, 'A3', True, True), (1, 13, 11, 48, 48, 2, 'X2', True, True),
               (2, 11, 13, 16, 64, 1, 'W3', True, False), (1, 12, 11, 96, 36, 1, 'A3', False, True),
               (1, 7, 9, 64, 128, 1, 'P0', False, True))
# conv3x3 split-K: (n, H, W, Cin, Cout, stride, family, parts expected)
CONV3_SPLITK = ((1, 5, 7, 256, 64, 1, 'P0', 4), (2, 9, 7, 240, 48, 2, 'A3', 4), (1, 3, 5, 1024, 64, 1, 'A3', 32),
                (1, 40, 52, 1024, 64, 1, 'P0', 8))

# gemm_bf16x3_ex: (M, K, N, residual_rows, n_split, family, diag variant)
EX_CASES = ((257, 64, 640, 7, 128, 'A3', 9), (129, 256, 768, 53, 256, 'W3', 7), (300, 96, 640, 1, 0, 'X2', 8),
            (33, 192, 768, 53, 128, 'P0', 9), (255, 512, 256, 7, 128, 'A3', 19), (128, 1024, 640, 53, 256, 'X2', 7),
            (300, 256, 768, 301, 0, 'W3', 16), (31, 512, 128, 7, 0, 'A3', 19))
# gemm_bf16x3_cat: (M, K1, K, N, family, epilogue)
CAT_CASES = ((129, 16, 64, 64, 'A3', 'res'), (257, 48, 96, 128, 'W3', 'relu'), (33, 64, 160, 256, 'X2', 'bias'),
             (300, 16, 96, 320, 'P0', 'res_inplace'), (255, 48, 1056, 256, 'A3', 'none'))
# gemm_bf16x3_grouped: (M, K, groups, group_n, columns of a beyond groups * K, family)
GROUPED_CASES = ((129, 64, 3, 64, 0, 'A3'), (257, 96, 2, 128, 32, 'W3'), (33, 256, 5, 64, 64, 'X2'),
                 (300, 64, 2, 256, 4, 'P0'), (2100, 512, 2, 128, 0, 'A3'))
# conv1x1_strided_split: (n, H, W, Cin, Cout, stride, family)
CONV1_CASES = ((2, 7, 9, 64, 128, 2, 'A3'), (1, 13, 5, 128, 256, 2, 'W3'), (1, 1, 1, 64, 128, 2, 'P0'),
               (1, 9, 11, 192, 128, 3, 'X2'), (3, 11, 13, 64, 384, 2, 'A3'))
# conv7x7s2_nchw_split: (n, H, W, family, 'dense' | 'repitch' | 'misaligned')
STEM_CASES = ((1, 9, 16, 'P0', 'dense'), (2, 7, 100, 'A3', 'dense'), (1, 11, 13, 'X2', 'dense'),
              (2, 9, 53, 'A3', 'repitch'), (1, 8, 101, 'W3', 'repitch'), (1, 9, 24, 'A3', 'misaligned'),
              (1, 5, 8, 'W3', 'dense'))
F16_SHAPES = ((129, 64, 256), (257, 1024, 256), (33, 192, 512), (300, 512, 768))      # fp16 operands: (M, K, N)
PLANE_SHAPES = ((129, 64, 128), (257, 1024, 256), (33, 192, 384))      # the 1- / 2-plane modes: (M, K, N)
# the fp32-MFMA kernels: conv3x3_nhwc (n, H, W, Cin, Cout, stride), rows_gemm_bias_res_act (M, K, K2, N, epilogue),
# conv3x3s2_c3_nchw (n, H, W)
MFMA_CONV3 = ((2, 7, 9, 32, 64, 1), (1, 11, 13, 64, 128, 2), (1, 1, 5, 32, 192, 1))
MFMA_ROWS = ((129, 32, 0, 64, 'res'), (257, 64, 32, 128, 'a_bias'), (33, 96, 0, 192, 'res_inplace'),
             (300, 32, 64, 256, 'relu'))
MFMA_C3 = ((2, 9, 11), (1, 1, 7), (1, 34, 16))


def grouped_operands(family, M, K, groups, group_n):
    """a [M, groups K] and the per-group weights [group_n, K]: group g is columns [g K, (g + 1) K) of a."""
    a, _ = operands(family, M, groups * K, group_n)
    return a, [operands(family, M, K, group_n, seed=g + 1)[1] for g in range(groups)]


def stem_operands(family, n, H, W, ksize=7):
    """Integer image [n, 3, H, W] and weight [64, 3, k, k] (rows (ky, kx, c) of the family's w)."""
    a, wr = operands(family, n * H * W, 3 * ksize * ksize, 64)
    x = np.ascontiguousarray(a[:, :3].reshape(n, H, W, 3).transpose(0, 3, 1, 2))
    return x, np.ascontiguousarray(wr.reshape(64, ksize, ksize, 3).transpose(0, 3, 1, 2))


def conv_operands(family, n, H, W, Cin, Cout, seed=0, ksize=3):
    """Integer image x [n, Cin, H, W] and weight w [Cout, Cin, k, k] of a family: the family's `a` values fill the
    image (its sparse side too), its `w` rows are the (ky, kx, cin) weight rows."""
    Kk = ksize * ksize * Cin
    a, w = operands(family, n * H * W, max(Kk, 17), Cout, seed)
    x = np.ascontiguousarray(a[:, :Cin].reshape(n, H, W, Cin).transpose(0, 3, 1, 2))
    w = np.ascontiguousarray(w[:, :Kk].reshape(Cout, ksize, ksize, Cin).transpose(0, 3, 1, 2))
    return x, w


def im2col(x, ksize=3, stride=1, padding=1):
    """[n, C, H, W] -> rows [n Ho Wo, (ky, kx, c)] of the implicit GEMM (zero padding), for check_case."""
    cols = torch.nn.functional.unfold(torch.from_numpy(x), ksize, padding=padding, stride=stride)   # [n, C k k, L]
    n, C = x.shape[:2]
    cols = cols.view(n, C, ksize * ksize, -1).permute(0, 3, 2, 1).reshape(-1, ksize * ksize * C)
    return cols.numpy()


def conv_rows(w):
    """[Cout, Cin, k, k] -> the weight rows [Cout, (ky, kx, cin)] of the implicit GEMM."""
    return np.ascontiguousarray(w.transpose(0, 2, 3, 1).reshape(w.shape[0], -1))
