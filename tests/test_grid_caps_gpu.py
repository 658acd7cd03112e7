"""Every launcher that caps its grid and lets the kernel loop (`i += gridDim.x * 256`), at a size just past the cap.

The other tests of these kernels stay below the cap, where every thread makes exactly one trip through the loop; the
real workload is past it on most of them.  Here each entry point runs at about 1.3 x (cap x 256) units, not a multiple
of 256: some threads make two trips, some one, and the last block is ragged.  A wrong stride, a 32-bit index product
in the loop body, or a cap and a kernel that disagree on the unit (float against float4) corrupt everything after the
first cap x 256 units and fail here.  Reference expression and tolerance of every case are those of the kernel's
small-shape test (none of these kernels changes its arithmetic with size); what a kernel must not write is filled
with NaN or a sentinel first and checked afterwards.

Left out: the two sampler fallbacks and pave_split_bf16x3_f32.  Their caps are 262 144 blocks, so a size past them
takes 268 MB and more of output.

(The full-size model tests of tests/test_model_gpu.py also drive several of these launchers past their caps, but end
to end and within a pixel tolerance; every row below has a case of its own against the kernel's own reference.)
Needs an MI355X."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# entry point: (cap in blocks of 256 threads, units per block, loop unit)          the launcher line it mirrors
CAPS = {
    'pave_bias_act_rows_f32': (4096, 256, 'float4'),                    # pave_kernels.hip: nb > 256 * 16
    'pave_fill_rows_f32': (4096, 256, 'float4 of the listed rows'),     # pave_kernels.hip: nb > 256 * 16
    'pave_repitch_rows_f32': (8192, 256, 'float4 of dst'),              # pave_kernels.hip: nb > 256 * 32
    'pave_fuse_sum_nhwc_f32': (8192, 256, 'float4'),                    # pave_kernels.hip: nb > 256 * 32
    'pave_bias_add_layernorm_f32': (4096, 4, 'row (one wave each)'),    # pave_kernels.hip: nb = (rows + 3) / 4 > 256 * 16
    'pave_bias_add_layernorm_pos_f32': (4096, 4, 'row (one wave each)'),
    'pave_bias_relu_maxpool_nhwc_f32': (16384, 256, 'float4 of the output'),   # pave_kernels.hip: min(.., 256 * 64)
    'pave_groupnorm_nhwc_f32': (8192, 256, 'float4 (apply pass)'),      # pave_kernels.hip: min(.., 256 * 32)
    'pave_groupnorm_levels_nhwc_f32': (8192, 256, 'float4 per level (apply pass)'),
    'pave_ref_update_f32': (1024, 256, 'float'),                        # pave_kernels.hip: min(.., 1024)
    'pave_ref_update_frames_f32': (1024, 256, 'float'),                 # pave_decoder.hip: > 1024 ? 1024
    'pave_gather_frame_poses_f32': (4096, 256, 'float'),                # pave_decoder.hip: > 4096 ? 4096
    'pave_gather_rows_add_f32': (4096, 256, 'float4'),                  # pave_decoder.hip: > 4096 ? 4096
    'pave_proposal_refs_f32': (4096, 256, 'float'),                     # pave_decoder.hip: > 4096 ? 4096
    'pave_preprocess_frames': (8192, 256, 'canvas pixel'),              # pave_kernels.hip: nb > 256 * 32
    'pave_preprocess_frames_flip': (8192, 256, 'canvas pixel'),
    'pave_preprocess_frames_nv12': (8192, 256, 'canvas pixel'),         # pave_ingest.hip: nb > 256 * 32
    'pave_preprocess_surfaces_nv12': (8192, 256, 'canvas pixel of one surface'),   # pave_ingest.hip: nb > 256 * 32
    'pave_hflip_canvas_f32': (8192, 256, 'float'),                      # pave_aug.hip: nb > 256 * 32
    'pave_scatter_rows_f32': (1024, 256, 'float4 of one row'),          # pave_ingest.hip: nb > 1024
}


def _past_cap(entry, total):
    """The case's own guard: `total` units are past one trip of the capped grid, by 1.2 - 1.45 x, and ragged."""
    cap, per_block, _ = CAPS[entry]
    one_trip = cap * per_block
    assert total > one_trip, f'{entry}: {total} units do not pass the cap of {one_trip}'
    assert 1.2 * one_trip < total < 1.45 * one_trip and total % per_block != 0, (entry, total / one_trip)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def test_bias_act_rows_past_the_cap():
    from pavenet_amd.ops import bias_act_rows_
    rows, C = 21337, 256
    _past_cap('pave_bias_act_rows_f32', rows * C // 4)
    g = torch.Generator().manual_seed(1)
    x, res, bias = torch.randn(rows, C, generator=g), torch.randn(rows, C, generator=g), torch.randn(C, generator=g)
    exp = torch.relu(x + bias + res)
    xd, rd = x.cuda(), res.cuda()
    out = bias_act_rows_(xd, bias.cuda(), rd, relu=True)
    assert out.data_ptr() == xd.data_ptr()
    np.testing.assert_allclose(out.cpu().numpy(), exp.numpy(), rtol=0, atol=0)
    assert torch.equal(rd.cpu(), res)


def test_fill_rows_past_the_cap():
    from pavenet_amd.ops import fill_rows_
    R, n, C = 26000, 21337, 256
    _past_cap('pave_fill_rows_f32', n * C // 4)
    g = torch.Generator().manual_seed(2)
    listed = torch.randperm(R, generator=g)[:n]
    rows = listed.to(torch.int32)
    rows[5], rows[n - 1] = -1, R                      # outside the matrix: skipped
    valid = torch.cat([listed[:5], listed[6:n - 1]])
    x = torch.randn(R, 2 * C, generator=g)
    vals = torch.randn(C, generator=g)
    exp = x.clone()
    exp[valid, :C] = vals
    xd = x.cuda()
    fill_rows_(xd[:, :C], rows.cuda(), vals.cuda())
    assert torch.equal(xd.cpu(), exp)                 # the unlisted rows and the other half of every row: untouched
    exp[valid, C:] = 0
    fill_rows_(xd[:, C:], rows.cuda(), None)
    assert torch.equal(xd.cpu(), exp)


def test_repitch_rows_past_the_cap():
    from pavenet_amd.ops import repitch_rows
    rows, W, pitch = 8001, 1333, 1336
    _past_cap('pave_repitch_rows_f32', rows * pitch // 4)
    x = torch.randn(rows, W, generator=torch.Generator().manual_seed(3))
    poison = torch.full((rows, pitch), float('nan'), device='cuda')    # the allocator hands this block back
    del poison
    xp = repitch_rows(x.cuda()).cpu()
    assert tuple(xp.shape) == (rows, pitch)
    assert torch.equal(xp[:, :W], x) and bool((xp[:, W:] == 0).all())


def test_fuse_sum_nhwc_past_the_cap():
    from pavenet_amd.ops import fuse_sum_nhwc
    N, C, H, W, shifts = 2, 100, 200, 264, (0, 1, 2, 3)
    _past_cap('pave_fuse_sum_nhwc_f32', N * H * W * C // 4)
    g = torch.Generator().manual_seed(4)
    maps = [torch.randn(N, C, H >> s, W >> s, generator=g) for s in shifts]
    y = 0
    for t, s in zip(maps, shifts):
        y = y + (torch.nn.functional.interpolate(t, scale_factor=2 ** s, mode='nearest') if s else t)
    terms = [(t.cuda().contiguous(memory_format=torch.channels_last), s) for t, s in zip(maps, shifts)]
    out = fuse_sum_nhwc(terms, relu=True)
    assert out.is_contiguous(memory_format=torch.channels_last) and tuple(out.shape) == (N, C, H, W)
    assert torch.equal(out.cpu(), torch.relu(y))
    assert torch.equal(fuse_sum_nhwc(terms, relu=False).cpu(), y)


def test_bias_add_layernorm_past_the_cap():
    from pavenet_amd.ops import bias_add_layernorm
    rows, C, P = 21375, 256, 125
    _past_cap('pave_bias_add_layernorm_f32', rows)
    _past_cap('pave_bias_add_layernorm_pos_f32', rows)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(rows // P, P, C, generator=g) * 3
    res = torch.randn(rows // P, P, C, generator=g)
    bias, gamma, beta = (torch.randn(C, generator=g) for _ in range(3))
    pos = torch.randn(P, C, generator=g)
    exp = torch.nn.functional.layer_norm(x + bias + res, (C,), gamma, beta, 1e-5)
    out = bias_add_layernorm(x.cuda(), bias.cuda(), res.cuda(), gamma.cuda(), beta.cuda(), 1e-5)
    np.testing.assert_allclose(out.cpu().numpy(), exp.numpy(), rtol=2e-5, atol=2e-5)
    y, yp = bias_add_layernorm(x.cuda(), bias.cuda(), res.cuda(), gamma.cuda(), beta.cuda(), 1e-5, pos=pos.cuda())
    assert torch.equal(y, out)
    assert torch.equal(yp.cpu(), y.cpu() + pos)


def test_bias_relu_maxpool_past_the_cap():
    from pavenet_amd.ops import bias_relu_maxpool_nhwc
    N, C, H, W = 2, 64, 641, 1061
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    _past_cap('pave_bias_relu_maxpool_nhwc_f32', N * Ho * Wo * C // 4)
    g = torch.Generator().manual_seed(6)
    x = torch.randn(N, C, H, W, generator=g)
    b = torch.randn(C, generator=g)
    exp = torch.nn.functional.max_pool2d(torch.relu(x + b[None, :, None, None]), 3, 2, 1)
    out = bias_relu_maxpool_nhwc(x.cuda().contiguous(memory_format=torch.channels_last), b.cuda())
    assert out.shape == exp.shape
    assert torch.equal(out.cpu(), exp)


def test_groupnorm_apply_pass_past_the_cap():
    """One-level entry against fp64 torch, written into a slice of a larger token buffer; then the levels entry (that
    map plus a small one, so the big level's capped share of the apply grid is followed by another level's blocks)
    bit-equal to the one-level entry."""
    from pavenet_amd.ops import groupnorm_levels_into, groupnorm_nhwc_into
    N, HW, C, G, small = 2, 21337, 256, 32, 35
    _past_cap('pave_groupnorm_nhwc_f32', N * HW * C // 4)
    _past_cap('pave_groupnorm_levels_nhwc_f32', N * HW * C // 4)
    g = torch.Generator().manual_seed(7)
    xs = [(torch.randn(N, hw, C, generator=g) * 3 + 1.5) for hw in (HW, small)]
    gbs = [(torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)) for _ in xs]
    S = HW + small + 13
    ref = torch.full((N, S, C), 7.0).cuda()
    buf = torch.full((N, S, C), 7.0).cuda()
    levels, st = [], 5
    for x, (gam, bet) in zip(xs, gbs):
        hw = x.shape[1]
        groupnorm_nhwc_into(x.cuda(), gam.cuda(), bet.cuda(), G, 1e-5, ref[:, st:st + hw])
        exp = torch.nn.functional.group_norm(x.double().permute(0, 2, 1), G, gam.double(), bet.double(),
                                             1e-5).permute(0, 2, 1)
        np.testing.assert_allclose(ref[:, st:st + hw].cpu().numpy(), exp.numpy(), rtol=1e-5, atol=1e-5)
        levels.append((x.cuda(), gam.cuda(), bet.cuda(), 1e-5, buf[:, st:st + hw]))
        st += hw
    assert float(ref[:, :5].min()) == 7.0 and float(ref[:, st:].max()) == 7.0
    groupnorm_levels_into(levels, G)
    assert torch.equal(buf, ref)


def test_ref_update_past_the_cap():
    from pavenet_amd.bricks import inverse_sigmoid
    from pavenet_amd.ops import ref_update
    n = 340001
    _past_cap('pave_ref_update_f32', n)
    g = torch.Generator().manual_seed(8)
    ref = torch.rand(n, generator=g) * 1.2 - 0.1       # some outside [0, 1]
    ref[-4:] = torch.tensor([0.0, 1.0, 1e-7, 1 - 1e-7])
    tmp = torch.randn(n, generator=g) * 3
    exp = (tmp.double() + inverse_sigmoid(ref.double())).sigmoid()
    got = ref_update(tmp.cuda(), ref.cuda())
    np.testing.assert_allclose(got.cpu().numpy(), exp.numpy(), rtol=2e-6, atol=1e-7)


@pytest.mark.parametrize('cat_dim', [0, 1])
def test_ref_update_frames_past_the_cap(cat_dim):
    """Both group forms (G = R: frame-major over all rows; G = queries per clip), bit-equal to the layout copy + the
    plain update the launch replaces -- and, since pave_ref_update_f32 at this size is past its own cap too, also
    against that formulation on the CPU in fp64 with ref_update's tolerance."""
    from pavenet_amd.bricks import inverse_sigmoid
    from pavenet_amd.ops import ref_update, ref_update_frames
    R, T, o, op = 2400, 5, 30, 64
    _past_cap('pave_ref_update_frames_f32', R * T * o)
    lead = (8, 300)
    g = torch.Generator().manual_seed(11 + cat_dim)
    y = torch.randn(R, T * op, generator=g)
    yt = y.view(R, T, op)[:, :, :o].permute(1, 0, 2).reshape((T,) + lead + (o,))
    if cat_dim == 0:
        cat = yt.reshape((T * lead[0], lead[1], o))
    else:
        cat = yt.permute(1, 0, 2, 3).reshape(lead[0], T * lead[1], o)
    ref = torch.rand(cat.shape, generator=g)
    exp = (cat.double() + inverse_sigmoid(ref.double())).sigmoid()
    got = ref_update_frames(y.cuda(), ref.cuda(), T, o, lead[1] if cat_dim else R)
    assert torch.equal(got, ref_update(cat.contiguous().cuda(), ref.cuda()))
    np.testing.assert_allclose(got.cpu().numpy(), exp.numpy(), rtol=2e-6, atol=1e-7)


def test_gather_frame_poses_past_the_cap():
    from pavenet_amd.ops import gather_frame_poses
    B, T, Q, N, C = 8, 7, 300, 300, 82
    _past_cap('pave_gather_frame_poses_f32', T * B * N * C)
    g = torch.Generator().manual_seed(9)
    poses = torch.rand(B, T * Q, C, generator=g)
    idx = torch.stack([torch.randperm(Q, generator=g)[:N] for _ in range(B)])
    got = gather_frame_poses(poses.cuda(), idx.cuda(), T).cpu()
    gidx = idx.unsqueeze(-1).expand(-1, -1, C)
    exp = torch.stack([torch.gather(poses[:, t * Q:(t + 1) * Q], 1, gidx).reshape(B * N, C) for t in range(T)], 0)
    assert torch.equal(got, exp)


def test_gather_rows_add_past_the_cap():
    from pavenet_amd.ops import gather_rows_add
    n, Q, S, C = 71, 301, 997, 256
    _past_cap('pave_gather_rows_add_f32', n * Q * C // 4)
    g = torch.Generator().manual_seed(10)
    src = torch.randn(n, S, C, generator=g)
    idx = torch.stack([torch.randperm(S, generator=g)[:Q] for _ in range(n)])
    add = torch.randn(Q, C, generator=g)
    rows, total = gather_rows_add(src.cuda(), idx.cuda(), add.cuda())
    exp = torch.gather(src, 1, idx.unsqueeze(-1).repeat(1, 1, C))
    assert torch.equal(rows.cpu(), exp) and torch.equal(total.cpu(), exp + add.unsqueeze(0))
    assert torch.equal(gather_rows_add(src.cuda(), idx.cuda()).cpu(), exp)


def test_proposal_refs_past_the_cap():
    """One shared `props` table with +inf rows; kpt is the 30-column slice of a 32-column matrix whose columns
    30 and 31 must stay as they were."""
    from pavenet_amd.ops import proposal_refs_
    n, Q, S, K2, T = 150, 300, 997, 30, 3
    _past_cap('pave_proposal_refs_f32', n * Q * K2)
    g = torch.Generator().manual_seed(12)
    idx = torch.stack([torch.randperm(S, generator=g)[:Q] for _ in range(n)])
    props = torch.randn(1, S, 2, generator=g) * 3
    props[:, ::13] = float('inf')
    wide = torch.randn(n * Q, 32, generator=g)
    ref = wide[:, :K2].unflatten(0, (n, Q)).clone()
    tp = torch.gather(props.expand(n, -1, -1), 1, idx.unsqueeze(-1).repeat(1, 1, 2))
    ref[..., 0::2] += tp[..., 0:1]
    ref[..., 1::2] += tp[..., 1:2]
    wd = wide.cuda()
    kpt = wd[:, :K2].unflatten(0, (n, Q))
    refs = proposal_refs_(kpt, props.cuda(), idx.cuda(), T)
    assert torch.equal(kpt.cpu(), ref) and torch.equal(wd[:, K2:].cpu(), wide[:, K2:])
    assert refs.shape == (n, T * Q, K2)
    np.testing.assert_allclose(refs.cpu().numpy(), ref.sigmoid().repeat(1, T, 1).numpy(), rtol=0, atol=1.2e-7)
    assert torch.equal(refs[:, :Q], refs[:, (T - 1) * Q:])


# ---- the input pipeline: two 1000 x 1400 canvases (resized picture 990 x 1393: padding on both sides) ----
CLIP = dict(T=2, H0=270, W0=380, img_scale=(1400, 990), size_divisor=50, canvas=(1000, 1400), resized=(990, 1393))


def _bgr_frames(seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, size=(CLIP['T'], CLIP['H0'], CLIP['W0'], 3)).astype(np.uint8)


def test_preprocess_frames_and_flip_past_the_cap():
    """Against the NumPy oracle (oracle/preprocess_ref.py) directly, bit for bit as at the small sizes: it takes
    0.5 s for these two canvases, so no chaining through per-frame launches is needed."""
    from oracle import preprocess_ref as PR
    from pavenet_amd.preprocess import preprocess_clip
    T, (Hp, Wp), (Hn, Wn) = CLIP['T'], CLIP['canvas'], CLIP['resized']
    _past_cap('pave_preprocess_frames', T * Hp * Wp)
    _past_cap('pave_preprocess_frames_flip', T * Hp * Wp)
    frames = _bgr_frames(13)
    exp, emeta = PR.preprocess_clip(frames, img_scale=CLIP['img_scale'], size_divisor=CLIP['size_divisor'])
    out, meta = preprocess_clip(_t(frames).cuda(), CLIP['img_scale'], CLIP['size_divisor'])
    assert tuple(out.shape) == exp.shape == (1, T, 3, Hp, Wp) and meta['img_shape'] == emeta['img_shape'] == (Hn, Wn, 3)
    assert Hn < Hp and Wn < Wp
    np.testing.assert_array_equal(out.cpu().numpy(), exp)
    fout, fmeta = preprocess_clip(_t(frames).cuda(), CLIP['img_scale'], CLIP['size_divisor'], flip=True)
    fexp = exp.copy()
    fexp[..., :Wn] = fexp[..., :Wn][..., ::-1]
    assert fmeta['flip'] is True
    np.testing.assert_array_equal(fout.cpu().numpy(), fexp)


def _surface(H0, W0, pitch, g):
    """One [H0 * 3 // 2, pitch] NV12 surface on which every byte value occurs on every plane."""
    s = torch.randint(0, 256, (H0 * 3 // 2, pitch), dtype=torch.uint8, generator=g)

    def uniform(n):
        return (torch.arange(n) % 256)[torch.randperm(n, generator=g)].to(torch.uint8)
    s[:H0, :W0] = uniform(H0 * W0).view(H0, W0)
    s[H0:, 0:W0:2] = uniform(H0 * W0 // 4).view(H0 // 2, W0 // 2)
    s[H0:, 1:W0:2] = uniform(H0 * W0 // 4).view(H0 // 2, W0 // 2)
    return s


def _nv12_to_bgr_host(surfaces, H0, W0, csc):
    """The conversion of include/pave_hip.h restated in torch fp32 on the CPU, one rounding per op:
    surfaces [T, H0 * 3 // 2, pitch] uint8 -> [T, H0, W0, 3] uint8 BGR."""
    s = surfaces.cpu()
    yoff, cy, crv, cgu, cgv, cbu = (torch.tensor(c, dtype=torch.float32) for c in csc)
    Y = s[:, :H0, :W0].float()
    uv = s[:, H0:, :W0].reshape(s.shape[0], H0 // 2, W0 // 2, 2).float()
    uv = uv.repeat_interleave(2, 1).repeat_interleave(2, 2)      # block (y >> 1, x >> 1)
    U, V = uv[..., 0] - 128.0, uv[..., 1] - 128.0
    t = (Y - yoff) * cy
    bgr = torch.stack([t + U * cbu, (t + U * cgu) + V * cgv, t + V * crv], -1)
    return torch.round(bgr).clamp(0, 255).to(torch.uint8)


def test_preprocess_frames_nv12_past_the_cap():
    """The same two canvases fed from NV12 surfaces with pitch > width, against pave_preprocess_frames on the
    host-converted picture (itself pinned to the oracle at this size by the case above) and against the oracle."""
    from oracle import preprocess_ref as PR
    from pavenet_amd.preprocess import nv12_csc, preprocess_clip, preprocess_clip_nv12
    T, H0, W0, (Hp, Wp), pitch = CLIP['T'], CLIP['H0'], CLIP['W0'], CLIP['canvas'], 384
    _past_cap('pave_preprocess_frames_nv12', T * Hp * Wp)
    g = torch.Generator().manual_seed(14)
    surfaces = torch.stack([_surface(H0, W0, pitch, g) for _ in range(T)])
    bgr = _nv12_to_bgr_host(surfaces, H0, W0, nv12_csc('bt709', False))
    exp, exp_meta = preprocess_clip(bgr.cuda(), CLIP['img_scale'], CLIP['size_divisor'])
    got, meta = preprocess_clip_nv12(surfaces.cuda(), W0, CLIP['img_scale'], CLIP['size_divisor'], matrix='bt709')
    assert tuple(got.shape) == (1, T, 3, Hp, Wp) and meta == exp_meta
    assert torch.equal(got, exp)
    oracle = PR.preprocess_clip(bgr.numpy(), img_scale=CLIP['img_scale'], size_divisor=CLIP['size_divisor'])[0]
    np.testing.assert_array_equal(got.cpu().numpy(), oracle)


def test_preprocess_surfaces_nv12_past_the_cap():
    """Two separately allocated surfaces (own pitch, own matrix and range) into 1400 x 2000 canvases: each surface's
    share of the grid is capped on its own, so ONE canvas is past the cap.  Against the oracle on each surface's
    host-converted picture (no launch of another entry below its cap exists at this canvas size)."""
    from oracle import preprocess_ref as PR
    from pavenet_amd.preprocess import nv12_csc, preprocess_surfaces_nv12
    H0, W0, img_scale, divisor, (Hp, Wp) = CLIP['H0'], CLIP['W0'], (2000, 1390), 50, (1400, 2000)
    _past_cap('pave_preprocess_surfaces_nv12', Hp * Wp)
    g = torch.Generator().manual_seed(15)
    settings = [('bt601', False), ('bt709', True)]
    surfaces = [_surface(H0, W0, pitch, g) for pitch in (384, 448)]
    got, meta = preprocess_surfaces_nv12([s.cuda() for s in surfaces], W0, img_scale, divisor,
                                         matrix=[m for m, _ in settings], full_range=[f for _, f in settings])
    assert tuple(got.shape) == (2, 3, Hp, Wp) and meta['img_shape'] == (1390, 1956, 3)
    for i, (m, f) in enumerate(settings):
        bgr = _nv12_to_bgr_host(surfaces[i][None], H0, W0, nv12_csc(m, f))
        oracle = PR.preprocess_clip(bgr.numpy(), img_scale=img_scale, size_divisor=divisor)[0]
        np.testing.assert_array_equal(got[i].cpu().numpy(), oracle[0, 0], err_msg=f'surface {i}')


def test_hflip_canvas_past_the_cap():
    """The kernel's loop unit is one float of [n, C, Hp, Wp]; per-image valid_w and one width for all."""
    from pavenet_amd.ops import hflip_canvas
    n, C, Hp, Wp = 2, 3, 500, 909
    _past_cap('pave_hflip_canvas_f32', n * C * Hp * Wp)
    x = torch.randn(n, C, Hp, Wp, generator=torch.Generator().manual_seed(16))
    ws = [871, 640]
    got = hflip_canvas(x.cuda(), torch.tensor(ws, dtype=torch.int32, device='cuda')).cpu()
    for i, w in enumerate(ws):
        assert torch.equal(got[i, :, :, :w], x[i, :, :, :w].flip(-1))
        assert torch.equal(got[i, :, :, w:], x[i, :, :, w:])     # the columns from w on: copied as they are
    got = hflip_canvas(x.cuda(), ws[0]).cpu()
    assert torch.equal(got[..., :ws[0]], x[..., :ws[0]].flip(-1)) and torch.equal(got[..., ws[0]:], x[..., ws[0]:])


def test_scatter_rows_past_the_cap():
    from pavenet_amd import ops
    row_elems, n, k, dst_rows, rows = 1310724, 2, 2, 3, [2, 0]
    _past_cap('pave_scatter_rows_f32', row_elems // 4)
    g = torch.Generator().manual_seed(17)
    srcs = [torch.randn(n, row_elems, generator=g) for _ in range(k)]
    dsts = [torch.full((dst_rows, row_elems), float('nan'), device='cuda') for _ in range(k)]
    dev = [s.cuda() for s in srcs]
    ops.scatter_rows(dev, dsts, rows)
    for s, sd, d in zip(srcs, dev, dsts):
        assert torch.equal(d[rows].cpu(), s) and torch.equal(sd.cpu(), s)
        assert bool(torch.isnan(d[1]).all()), 'row 1 was not written'
