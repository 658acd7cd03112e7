"""The kernels that carry the model's own attention -- fused_deform_attn_kernel<MODE, PPL, WQ>,
enc_head_major_kernel (csrc/pave_kernels.hip) and the LDS-tile encoder kernel (csrc/pave_enc_tile.hip) --
against the fp64 reference of tests/fused_ref.py, whole outputs, at every dispatch point and at the edges:
unit counts on both sides of each form's work unit, samples on and around every map border (1 x 1, 1 x W and
H x 1 levels included), every (L, K) corner of the pose kernel, frame tables and slab clamping at T = 1, and
pyramids of one or two tiles.  Needs an MI355X.

Tolerance: rtol = atol = 2e-5, the bound these kernels carry against the fp32 oracle composition.  That
composition (grid_expected / pose_expected on fp32 inputs) is itself within 2.1e-6 of the fp64 reference at the
standard shapes and within 3.9e-6 over every case of this file (largest: 3.4e-6 for the single-point pose sample
L = K = 1, 3.8e-6 for 12-pixel offsets on the small pyramids), so 2e-5 is five to ten times the reference's own
error.
"""
import numpy as np
import pytest
import torch

from oracle.seeded import seeded_array
from tests.fused_ref import grid_ref64, pose_ref64
from tests.msda_ref import contiguous_lsi

pytestmark = pytest.mark.gpu
STD = [(12, 20), (6, 10), (3, 5), (2, 3)]
THIN = [(1, 1), (1, 7), (5, 1), (2, 3)]
TILE = [(16, 20), (8, 10), (4, 5), (2, 3)]
TOL = dict(rtol=2e-5, atol=2e-5)


def _t(name, shape, scale=1.0):
    return torch.from_numpy(seeded_array(name, shape, scale))


def _levels(levels):
    shapes = torch.as_tensor(levels, dtype=torch.long)
    lsi = contiguous_lsi(shapes)
    return shapes, lsi, shapes.cuda(), lsi.cuda(), int(shapes.prod(1).sum())


def _i32(x):
    return None if x is None else torch.as_tensor(x).to(torch.int32).cuda()


def _grid(value_d, lv, proj, ref, *, T, n_clips, unit_clip=None, order=None, frame_table=None, per_query=False):
    """deform_attn_grid_fused on host inputs -> (out, stat_max, stat_sum) on the host.  per_query: through the
    C ABI with a row stride one float past the dense row (385 at T = 1), which the head-major kernel's 16-byte
    loads cannot take: T = 1 then runs fused_deform_attn_kernel<GRID, 2, 1>.  The pad column holds 1e30."""
    _, _, sd, ld, S = lv
    U = proj.shape[0]
    uc, od = _i32(unit_clip), _i32(order)
    if not per_query:
        from pavenet_amd.ops import deform_attn_grid_fused
        res = deform_attn_grid_fused(value_d, sd, ld, proj.cuda(), ref.cuda(), T=T, n_clips=n_clips,
                                     units_per_clip=U, unit_clip=uc, order=od, return_stats=True,
                                     frame_table=frame_table)
    else:
        from pavenet_amd import native
        lib = native.load()
        stride = proj.shape[1] + 1
        assert stride % 4 == 1
        wide = torch.full((U, stride), 1e30)
        wide[:, :-1] = proj
        pd, rd = wide.cuda(), ref.contiguous().cuda()
        res = (torch.empty(U, 256, device='cuda'), torch.empty(U, 8, device='cuda'), torch.empty(U, 8, device='cuda'))
        st = lib.pave_deform_attn_grid_fused_f32(
            value_d.data_ptr(), sd.data_ptr(), ld.data_ptr(), pd.data_ptr(), rd.data_ptr(),
            None if uc is None else uc.data_ptr(), None if od is None else od.data_ptr(),
            res[0].data_ptr(), res[1].data_ptr(), res[2].data_ptr(), U, U, n_clips, T, S, 4, 4, stride,
            None if frame_table is None else frame_table.data_ptr(),
            value_d.shape[0] if frame_table is not None else 0, 4, torch.cuda.current_stream().cuda_stream)
        native.check(st, 'grid_fused (C ABI)')
    torch.cuda.synchronize()
    return tuple(r.cpu() for r in res)


def _check(got, exp, what):
    out, smax, ssum = got
    eo, emx, esm = exp
    np.testing.assert_allclose(out.double().numpy(), eo.numpy(), err_msg=what, **TOL)
    np.testing.assert_array_equal(smax.double().numpy(), emx.numpy(), err_msg=what)
    np.testing.assert_allclose(ssum.double().numpy(), esm.numpy(), rtol=1e-5, atol=0, err_msg=what)


def _frames_of(clip, T):
    """slab_of without a frame table: clip * T + t"""
    return torch.as_tensor(clip).long()[:, None] * T + torch.arange(T)[None]


# ---------------------------------------------------------------------------------------------------------
# a. grid dispatch: every kernel form, unit counts on both sides of its work unit
# ---------------------------------------------------------------------------------------------------------
GRID_FORMS = {'head_major': [(1, U) for U in (1, 31, 32, 33, 63, 64, 65)],       # patches of 32, two per block
              'per_query_T1': [(1, U) for U in (1, 3, 4, 5)],                      # <GRID,2,1>: 4 units per block
              'T2': [(2, U) for U in (1, 2, 3)],                                   # <GRID,2,2>: 2 units per block
              'T3_and_up': [(T, U) for T in (3, 4, 9, 15) for U in (1, 5)]}        # <GRID,2,4>: 1 unit per block


def _grid_cases(form):
    return [(T, U, clips) for T, U in GRID_FORMS[form] for clips in (1, 3)]


@pytest.mark.parametrize('form,n_cases', [('head_major', 14), ('per_query_T1', 8), ('T2', 6), ('T3_and_up', 16)])
def test_grid_dispatch_vs_fp64(form, n_cases):
    cases = _grid_cases(form)
    assert len(cases) == n_cases and len(set(cases)) == n_cases
    lv = _levels(STD)
    shapes, lsi, _, _, S = lv
    for T, U, clips in cases:
        value = _t(f'fs.a.value.{T}.{clips}', (clips * T, S, 8, 32))
        proj = _t(f'fs.a.proj.{form}.{T}.{U}.{clips}', (U, T * 384))
        proj[:, :T * 256] *= 2.0                                                   # offsets: a few pixels
        ref = _t(f'fs.a.ref.{form}.{T}.{U}', (T, U, 4, 2), 0.35) + 0.5             # some outside [0, 1]
        unit_clip = (torch.arange(U) * 5 + 2) % clips                              # 2, 1, 0, 2, .. : not monotone
        order = torch.randperm(U, generator=torch.Generator().manual_seed(U))
        exp = grid_ref64(value, shapes, lsi, proj, ref, T, _frames_of(unit_clip, T))
        got = _grid(value.cuda(), lv, proj, ref, T=T, n_clips=clips, unit_clip=unit_clip, order=order,
                    per_query=form == 'per_query_T1')
        _check(got, exp, f'{form} T={T} U={U} clips={clips}')


# ---------------------------------------------------------------------------------------------------------
# b. border placement
# ---------------------------------------------------------------------------------------------------------
STEPS = (0.0, 0.25, 0.5, 0.75)


def _axis_table(n):
    """pixel positions around both borders of an axis of n pixels (pixel = loc * n - 0.5)"""
    return [-1.5, -1.0, -1.0 + 2.0 ** -10, -0.5, 0.0, 0.5, n - 1.5, n - 1.0, n - 0.5, n - 2.0 ** -10, float(n), n + 0.5]


def _border_pixels(levels):
    """-> (px, py) fp64 [144, L, 4]: row u = ix * 12 + iy is the pair (x table[ix], y table[iy]) of each level's
    OWN table; the level's four points sit at the pair plus 0, 1/4, 1/2, 3/4 px on both axes."""
    px = torch.empty(144, len(levels), 4, dtype=torch.float64)
    py = torch.empty_like(px)
    step = torch.tensor(STEPS, dtype=torch.float64)
    for l, (H, W) in enumerate(levels):
        tx = torch.tensor(_axis_table(W), dtype=torch.float64)
        ty = torch.tensor(_axis_table(H), dtype=torch.float64)
        assert tx.numel() == 12 and ty.numel() == 12
        px[:, l] = tx[:, None].expand(12, 12).reshape(144, 1) + step
        py[:, l] = ty[None, :].expand(12, 12).reshape(144, 1) + step
    return px, py


def _grid_border_inputs(levels, mode, U, T, name):
    """Grid inputs whose unit u samples table row u % 144 in every frame.  mode 'ref': the reference point
    carries the pair (offsets are zero but for the quarter-pixel steps of points 1 .. 3); mode 'offset':
    ref = 0.5 and the offset carries the whole position (the offset / W arithmetic)."""
    px, py = _border_pixels(levels)
    assert px.shape == (144, 4, 4)
    rows = torch.arange(U) % 144
    px, py = px[rows], py[rows]
    W = torch.tensor([w for _, w in levels], dtype=torch.float64).view(1, 4, 1)
    H = torch.tensor([h for h, _ in levels], dtype=torch.float64).view(1, 4, 1)
    if mode == 'ref':
        ref = torch.stack([(px[:, :, 0] + 0.5) / W[..., 0], (py[:, :, 0] + 0.5) / H[..., 0]], -1)   # [U, 4, 2]
        off = torch.stack([px - px[:, :, :1], py - py[:, :, :1]], -1)                               # [U, 4, 4, 2]
        assert (off[:, :, 0] == 0).all()
    else:
        ref = torch.full((U, 4, 2), 0.5, dtype=torch.float64)
        off = torch.stack([px - (0.5 * W - 0.5), py - (0.5 * H - 0.5)], -1)
    off = off[:, None, None].expand(U, T, 8, 4, 4, 2).reshape(U, T * 256)
    proj = torch.cat([off.float(), _t(f'{name}.logits', (U, T * 128))], 1).contiguous()
    return proj, ref.float()[None].expand(T, U, 4, 2).contiguous()


_border_cache = {}


def _grid_border(levels, mode, U, T):
    """(value, proj, ref, fp64 expectation), computed once per input set and shared by the kernels that take it"""
    key = (tuple(levels), mode, U, T)
    if key not in _border_cache:
        shapes, lsi, _, _, S = _levels(levels)
        name = f'fs.b.{levels[1]}.{mode}.{U}.{T}'
        value = _t(name + '.value', (T, S, 8, 32))
        proj, ref = _grid_border_inputs(levels, mode, U, T, name)
        exp = grid_ref64(value, shapes, lsi, proj, ref, T, _frames_of(torch.zeros(U), T))
        _border_cache[key] = (value, proj, ref, exp)
    return _border_cache[key]


@pytest.mark.parametrize('mode', ['ref', 'offset'])
@pytest.mark.parametrize('levels', [STD, THIN], ids=['std', 'thin'])
@pytest.mark.parametrize('kernel', ['head_major', 'per_query_T1', 'grid_T3'])
def test_border_placement_grid_kernels_vs_fp64(kernel, levels, mode):
    T = 3 if kernel == 'grid_T3' else 1
    value, proj, ref, exp = _grid_border(levels, mode, 144, T)
    assert proj.shape[0] == 144
    got = _grid(value.cuda(), _levels(levels), proj, ref, T=T, n_clips=1, per_query=kernel == 'per_query_T1')
    _check(got, exp, f'{kernel} {mode}')


@pytest.mark.parametrize('mode', ['ref', 'offset'])
@pytest.mark.parametrize('levels', [STD, THIN], ids=['std', 'thin'])
def test_border_placement_pose_kernel_vs_fp64(levels, mode):
    """K = 17 (PPL = 3): key point k of (query u, level l) is table row u's point k % 4.  mode 'ref': the key
    point itself sits there and the offsets are zero; mode 'offset': the key points alternate between 0.25 and
    0.75 on both axes (extent 0.5, so a unit offset moves 0.25) and the offset carries the position."""
    from pavenet_amd.ops import deform_attn_pose_fused
    shapes, lsi, sd, ld, S = _levels(levels)
    Q, K, L = 144, 17, 4
    px, py = _border_pixels(levels)
    assert px.shape == (Q, L, 4)
    k4 = torch.arange(K) % 4
    W = torch.tensor([w for _, w in levels], dtype=torch.float64).view(1, 4, 1)
    H = torch.tensor([h for h, _ in levels], dtype=torch.float64).view(1, 4, 1)
    loc = torch.stack([(px[:, :, k4] + 0.5) / W, (py[:, :, k4] + 0.5) / H], -1)       # [Q, L, K, 2]
    if mode == 'ref':
        kp, off = loc, torch.zeros_like(loc)
    else:
        kp = torch.where(torch.arange(K) % 2 == 0, 0.25, 0.75).double().view(1, 1, K, 1).expand(Q, L, K, 2)
        off = (loc - kp) * 4.0
    ref = kp.float().reshape(1, Q, L, 2 * K).contiguous()
    name = f'fs.b.pose.{levels[1]}.{mode}'
    proj = torch.cat([off.float()[:, None].expand(Q, 8, L, K, 2).reshape(Q, -1), _t(name + '.logits', (Q, 8 * L * K))], 1)
    value = _t(name + '.value', (1, S, 8, 32))
    exp = pose_ref64(value, shapes, lsi, proj, ref, 1, 1, Q, K, torch.zeros(Q, 1))
    got = deform_attn_pose_fused(value.cuda(), sd, ld, proj.contiguous().cuda(), ref.cuda(), T=1, n_clips=1,
                                 num_query=Q, num_keypoints=K, return_stats=True)
    torch.cuda.synchronize()
    _check(tuple(g.cpu() for g in got), exp, f'pose border {mode}')


@pytest.mark.parametrize('variant', [0, 1])
@pytest.mark.parametrize('mode', ['ref', 'offset'])
def test_border_placement_tile_kernel_vs_fp64(mode, variant):
    """token i of the 2 x 3-tile pyramid takes table row i % 144: most footprints are far from the token's own
    tile, so both the LDS pass and the global second pass meet every border"""
    from pavenet_amd.ops import deform_attn_enc_tile, enc_tile_supported
    assert enc_tile_supported(TILE)
    S = sum(h * w for h, w in TILE)
    assert S > 2 * 144
    value, proj, ref, exp = _grid_border(TILE, mode, S, 1)
    out = deform_attn_enc_tile(value.cuda(), proj.cuda(), ref.cuda(), levels_hw=TILE, variant=variant)
    torch.cuda.synchronize()
    np.testing.assert_allclose(out.cpu().double().numpy(), exp[0].numpy(), **TOL)


# ---------------------------------------------------------------------------------------------------------
# c. pose kernel: every (L, K) corner, PPL = 2 | 3, the extent clamps
# ---------------------------------------------------------------------------------------------------------
POSE_LK = [(1, 1), (1, 24), (2, 16), (3, 17), (4, 1), (4, 2), (4, 16), (4, 17), (4, 24)]


def _pose_inputs(L, K, T, Q, clips, name, levels=STD):
    S = sum(h * w for h, w in levels[:L])
    value = _t(name + '.value', (clips * T, S, 8, 32))
    proj = _t(name + '.proj', (clips * Q, T * 8 * L * K * 3))
    ref = (_t(name + '.ref', (clips, T * Q, L, 2 * K), 0.4) + 0.5).view(clips, T, Q, L, K, 2)   # some outside [0, 1]
    if Q >= 5:
        # query 1: every key point of a (frame, level) at one place -> both 1e-4 clamps; its offsets are made
        # 1000 x larger so that 1000 * 5e-5 * W is of the order of a pixel
        ref[:, :, 1] = ref[:, :, 1, :, :1].clone()
        off = proj[:, :T * 8 * L * K * 2].view(clips, Q, -1)
        off[:, 1] *= 1000.0
        # query 2: zero width only (one x for all key points, y spread)
        ref[:, :, 2, :, :, 0] = ref[:, :, 2, :, :1, 0].clone()
        # query 3: every key point outside [0, 1], just past the right and the upper border (footprints
        # partly on the map)
        ref[:, :, 3, :, :, 0] = 1.0 + 0.05 * (ref[:, :, 3, :, :, 0] - 0.5).abs()
        ref[:, :, 3, :, :, 1] = -0.05 * (ref[:, :, 3, :, :, 1] - 0.5).abs()
    return value, proj, ref.reshape(clips, T * Q, L, 2 * K).contiguous()


@pytest.mark.parametrize('L,K', POSE_LK)
def test_pose_kernel_vs_fp64(L, K):
    from pavenet_amd.ops import deform_attn_pose_fused
    cases = [(T, Q, clips) for T in (1, 3) for Q in (1, 5) for clips in (1, 2)]
    assert len(cases) == 8
    shapes, lsi, sd, ld, S = _levels(STD[:L])
    for T, Q, clips in cases:
        value, proj, ref = _pose_inputs(L, K, T, Q, clips, f'fs.c.{L}.{K}.{T}.{Q}.{clips}')
        if Q == 5:
            r = ref.view(clips, T, Q, L, K, 2)
            assert (r[:, :, 1].amax(-2) == r[:, :, 1].amin(-2)).all()
            assert (r[:, :, 2, :, :, 0].amax(-1) == r[:, :, 2, :, :, 0].amin(-1)).all()
            assert K == 1 or (r[:, :, 2, :, :, 1].amax(-1) > r[:, :, 2, :, :, 1].amin(-1)).all()
            assert ((r[:, :, 3] < 0) | (r[:, :, 3] > 1)).all()
        exp = pose_ref64(value, shapes, lsi, proj, ref, T, clips, Q, K, _frames_of(torch.arange(clips * Q) // Q, T))
        got = deform_attn_pose_fused(value.cuda(), sd, ld, proj.cuda(), ref.cuda(), T=T, n_clips=clips,
                                     num_query=Q, num_keypoints=K, return_stats=True)
        torch.cuda.synchronize()
        _check(tuple(g.cpu() for g in got), exp, f'pose L={L} K={K} T={T} Q={Q} clips={clips}')


@pytest.mark.parametrize('L', [2, 3])
def test_pose_kernel_broadcast_level_axis_vs_fp64(L):
    """ref_levels = 1: one row of key points shared by the L levels, handed over as an expanded stride-0 view"""
    from pavenet_amd.ops import deform_attn_pose_fused
    cases = [(K, T) for K in (16, 17) for T in (1, 3)]
    assert len(cases) == 4
    shapes, lsi, sd, ld, S = _levels(STD[:L])
    clips, Q = 2, 5
    for K, T in cases:
        value, proj, _ = _pose_inputs(L, K, T, Q, clips, f'fs.c.bc.{L}.{K}.{T}')
        base = _t(f'fs.c.bc.ref.{L}.{K}.{T}', (clips, T * Q, 2 * K), 0.4) + 0.5
        exp = pose_ref64(value, shapes, lsi, proj, base[:, :, None].expand(-1, -1, L, -1), T, clips, Q, K,
                         _frames_of(torch.arange(clips * Q) // Q, T))
        ref = base.cuda()[:, :, None].expand(-1, -1, L, -1)
        assert ref.stride(2) == 0 and not ref.is_contiguous()
        got = deform_attn_pose_fused(value.cuda(), sd, ld, proj.cuda(), ref, T=T, n_clips=clips, num_query=Q,
                                     num_keypoints=K, return_stats=True)
        torch.cuda.synchronize()
        _check(tuple(g.cpu() for g in got), exp, f'broadcast L={L} K={K} T={T}')


@pytest.mark.parametrize('L,K', [(4, 25), (5, 15)])
def test_pose_kernel_refuses_what_it_was_not_built_for(L, K):
    """K > 24 and L > 4 are errors, raised before anything is enqueued: the output buffer keeps its bits"""
    from pavenet_amd import native
    from pavenet_amd.ops import deform_attn_pose_fused
    levels = (STD + [(1, 2)])[:L]
    shapes, lsi, sd, ld, S = _levels(levels)
    Q = 3
    value = _t('fs.c.err.value', (1, S, 8, 32)).cuda()
    proj = _t(f'fs.c.err.proj.{L}.{K}', (Q, 8 * L * K * 3)).cuda()
    ref = torch.rand(1, Q, L, 2 * K, generator=torch.Generator().manual_seed(0)).cuda()
    with pytest.raises(RuntimeError):
        deform_attn_pose_fused(value, sd, ld, proj, ref, T=1, n_clips=1, num_query=Q, num_keypoints=K)
    out = torch.full((Q, 256), -7.0, device='cuda')
    st = native.load().pave_deform_attn_pose_fused_f32(
        value.data_ptr(), sd.data_ptr(), ld.data_ptr(), proj.data_ptr(), ref.data_ptr(), out.data_ptr(), None, None,
        1, Q, 1, S, L, K, proj.stride(0), None, 0, L, torch.cuda.current_stream().cuda_stream)
    assert st != 0
    torch.cuda.synchronize()
    assert (out == -7.0).all()


# ---------------------------------------------------------------------------------------------------------
# d. frame tables and slab clamping at T = 1
# ---------------------------------------------------------------------------------------------------------
N_SLABS = 4


def _t1_table_inputs():
    """`value` is the middle N_SLABS slabs of an allocation of N_SLABS + 2: a kernel that does not clamp a slab
    index of -1 or N_SLABS reads allocated memory and fails by value, never by fault.  The frame table is the
    middle of a longer tensor in the same way."""
    lv = _levels(STD)
    S = lv[4]
    U = 37
    big = _t('fs.d.value', (N_SLABS + 2, S, 8, 32))
    proj = _t('fs.d.proj', (U, 384))
    proj[:, :256] *= 2.0
    ref = _t('fs.d.ref', (1, U, 4, 2), 0.35) + 0.5
    unit_clip = (torch.arange(U) * 3 + 1) % N_SLABS                                   # 1, 0, 3, 2, ..
    big_d = big.cuda()
    value_d = big_d[1:N_SLABS + 1]
    assert value_d.is_contiguous() and value_d.data_ptr() == big_d.data_ptr() + S * 1024
    return lv, big[1:N_SLABS + 1], value_d, proj, ref, unit_clip


def _table(entries):
    padded = torch.tensor([N_SLABS + 5] + list(entries) + [-9], dtype=torch.int32).cuda()
    return padded[1:-1]


@pytest.mark.parametrize('kernel', ['head_major', 'per_query_T1'])
def test_T1_frame_table_of_valid_entries_vs_fp64(kernel):
    """a permuting frame table at T = 1: slab of a unit = table[unit_clip[unit]]"""
    lv, value, value_d, proj, ref, unit_clip = _t1_table_inputs()
    entries = [2, 0, 3, 1]
    assert sorted(entries) == list(range(N_SLABS)) and all(e != i for i, e in enumerate(entries))
    exp = grid_ref64(value, lv[0], lv[1], proj, ref, 1, torch.tensor(entries)[unit_clip][:, None])
    got = _grid(value_d, lv, proj, ref, T=1, n_clips=N_SLABS, unit_clip=unit_clip, frame_table=_table(entries),
                per_query=kernel == 'per_query_T1')
    _check(got, exp, kernel)


@pytest.mark.parametrize('kernel', ['head_major', 'per_query_T1'])
def test_T1_slab_indices_are_clamped_into_the_value_tensor(kernel):
    """entries of -1 and n_slabs, in the frame table and (separately) in unit_clip, give what the clamped entries
    give; so does a unit_clip entry outside a frame table (the index into the table is clamped)"""
    lv, value, value_d, proj, ref, unit_clip = _t1_table_inputs()
    pq = kernel == 'per_query_T1'
    U = proj.shape[0]
    bad, clamped = [-1, N_SLABS, 2, 0], [0, N_SLABS - 1, 2, 0]
    exp = grid_ref64(value, lv[0], lv[1], proj, ref, 1, torch.tensor(clamped)[unit_clip][:, None])
    got = _grid(value_d, lv, proj, ref, T=1, n_clips=N_SLABS, unit_clip=unit_clip, frame_table=_table(bad), per_query=pq)
    _check(got, exp, kernel + ': frame table')
    bad_clip = unit_clip.clone()
    bad_clip[::5] = -1
    bad_clip[2::5] = N_SLABS
    assert (bad_clip == -1).any() and (bad_clip == N_SLABS).any()
    ok_clip = bad_clip.clamp(0, N_SLABS - 1)
    exp = grid_ref64(value, lv[0], lv[1], proj, ref, 1, ok_clip[:, None])
    got = _grid(value_d, lv, proj, ref, T=1, n_clips=N_SLABS, unit_clip=bad_clip, per_query=pq)
    _check(got, exp, kernel + ': unit_clip')
    entries = [2, 0, 3, 1]
    exp = grid_ref64(value, lv[0], lv[1], proj, ref, 1, torch.tensor(entries)[ok_clip][:, None])
    got = _grid(value_d, lv, proj, ref, T=1, n_clips=N_SLABS, unit_clip=bad_clip, frame_table=_table(entries),
                per_query=pq)
    _check(got, exp, kernel + ': unit_clip into a frame table')


# ---------------------------------------------------------------------------------------------------------
# e. tile kernel on pyramids of one or two tiles
# ---------------------------------------------------------------------------------------------------------
SMALL_PYRAMIDS = [[(5, 7), (3, 4), (2, 2), (1, 1)], [(8, 8), (4, 4), (2, 2), (1, 1)], [(9, 8), (5, 4), (3, 2), (2, 1)],
                  [(40, 3), (20, 2), (10, 1), (5, 1)], [(3, 40), (2, 20), (1, 10), (1, 5)]]
VALID_RATIOS = torch.tensor([[0.83, 0.9], [1.0, 0.7], [0.6, 1.0]])


def _token_centres(levels):
    ys = torch.cat([((torch.arange(h * w) // w).float() + 0.5) / h for h, w in levels])
    xs = torch.cat([((torch.arange(h * w) % w).float() + 0.5) / w for h, w in levels])
    return torch.stack([xs, ys], -1)


@pytest.mark.parametrize('levels', SMALL_PYRAMIDS, ids=lambda lv: 'x'.join(map(str, lv[0])))
def test_tile_kernel_small_pyramids_every_row_vs_fp64(levels):
    from pavenet_amd.ops import deform_attn_enc_tile, deform_attn_grid_fused, enc_tile_supported
    assert enc_tile_supported(levels)
    cases = [(F, sigma, padded) for F in (1, 3) for sigma in (0.7, 12.0) for padded in (False, True)]
    assert len(cases) == 8
    shapes, lsi, sd, ld, S = _levels(levels)
    for F, sigma, padded in cases:
        name = f'fs.e.{levels[0]}.{F}.{sigma}'
        value = _t(name + '.value', (F, S, 8, 32))
        proj = _t(name + '.proj', (F * S, 384))
        proj[:, :256] *= sigma
        vr = (VALID_RATIOS[:F] if padded else torch.ones(F, 2)).view(F, 1, 1, 2)
        ref = (_token_centres(levels)[None, :, None, :] * vr).expand(F, S, 4, 2).reshape(1, F * S, 4, 2).contiguous()
        exp = grid_ref64(value, shapes, lsi, proj, ref, 1, (torch.arange(F * S) // S)[:, None])[0].numpy()
        vd, pd, rd = value.cuda(), proj.cuda(), ref.cuda()
        direct = deform_attn_grid_fused(vd, sd, ld, pd, rd, T=1, n_clips=F, units_per_clip=S).cpu()
        np.testing.assert_allclose(direct.double().numpy(), exp, **TOL)
        for variant in (0, 1):
            out = deform_attn_enc_tile(vd, pd, rd, levels_hw=levels, variant=variant).cpu()
            what = f'F={F} sigma={sigma} padded={padded} variant={variant}'
            np.testing.assert_allclose(out.double().numpy(), exp, err_msg=what, **TOL)
            np.testing.assert_allclose(out.numpy(), direct.numpy(), rtol=1e-5, atol=1e-5, err_msg=what)


@pytest.mark.parametrize('F', [1, 3])
@pytest.mark.parametrize('levels', SMALL_PYRAMIDS, ids=lambda lv: 'x'.join(map(str, lv[0])))
def test_tile_kernel_small_pyramids_prepared_path_keeps_the_bits(levels, F):
    """gemm_bf16x3_encproj -> deform_attn_enc_tile(prepared=True) == merged GEMM -> the sampler doing its own
    arithmetic, bit for bit, and both are the fp64 sampling of the GEMM's value / projection rows"""
    from pavenet_amd import ops
    assert ops.enc_tile_supported(levels)
    shapes, lsi, _, _, S = _levels(levels)
    M, K = F * S, 256
    a = _t(f'fs.e.prep.a.{levels[0]}.{F}', (M, K)).cuda()
    w = _t('fs.e.prep.w', (640, K), 0.05)
    w[256:512] *= 4.0                   # offsets of ~3 pixels
    table = _t(f'fs.e.prep.table.{levels[0]}', (S, 640), 0.1).cuda()
    wp = ops.split_weight_bf16x3(w.cuda())
    vr = VALID_RATIOS[:F].view(F, 1, 1, 2)
    ref = (_token_centres(levels)[None, :, None, :] * vr).expand(F, S, 4, 2).reshape(M, 4, 2).contiguous().cuda()
    v0, proj = ops.gemm_bf16x3_ex(a, wp, None, table, residual_rows=S, n_split=256)
    v1, samp = ops.gemm_bf16x3_encproj(a, wp, table, ref, levels)
    assert torch.equal(v0, v1)
    raw = ops.deform_attn_enc_tile(v0.view(F, S, 8, 32), proj, ref.view(1, M, 4, 2), levels_hw=levels)
    pre = ops.deform_attn_enc_tile(v1.view(F, S, 8, 32), samp, None, levels_hw=levels, prepared=True)
    torch.cuda.synchronize()
    assert torch.equal(raw, pre), float((raw - pre).abs().max())
    exp = grid_ref64(v0.cpu().view(F, S, 8, 32), shapes, lsi, proj.cpu(), ref.cpu().view(1, M, 4, 2), 1,
                     (torch.arange(M) // S)[:, None])[0]
    np.testing.assert_allclose(raw.cpu().double().numpy(), exp.numpy(), **TOL)
