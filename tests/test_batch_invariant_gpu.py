"""Batch-invariant inference on the device: under form policies 1 and 2 a row's / an image's / a clip's outputs
do not depend on what shares its launch or batch, bit for bit; the multi-tile K-split form equals gemm_sk_kernel;
the default mode is unchanged after the batch-invariant one.  Needs an MI355X."""
import pytest
import torch

pytestmark = pytest.mark.gpu

# every threshold of the dispatchers (+ 1): K-split form 2 048 rows, small-row 64 tiles / 8 192 rows,
# split-K classes, the wide form's 400 tiles
ROWS = [1, 37, 300, 1200, 2047, 2048, 2049, 2400, 3969, 4097, 8191, 8193, 16385, 25601, 51201]


def _rand(*shape, scale=1.0, seed=0):
    g = torch.Generator(device='cuda').manual_seed(seed)
    return torch.randn(*shape, device='cuda', generator=g) * scale


def _prefix_equal(run, a, ms=ROWS):
    """run(a_rows) -> output rows; every launch over a[:m] equals the first m rows of the launch over all of a."""
    full = run(a)
    for m in ms:
        got = run(a[:m].contiguous())
        assert torch.equal(got, full[:m]), f'rows [0, {m}) differ from the {a.shape[0]}-row launch'


@pytest.mark.parametrize('policy', [1, 2])
@pytest.mark.parametrize('K,N,epi', [(1024, 256, 'bias+res'), (256, 256, 'bias+relu'), (256, 1024, 'gelu'),
                                     (2048, 512, 'bias+res+relu'), (512, 30, 'bias'), (256, 2688, 'bias')])
def test_row_gemm_rows_do_not_depend_on_m(policy, K, N, epi):
    from pavenet_amd import ops
    Mx = ROWS[-1]
    a = _rand(Mx, K, seed=1)
    w = _rand(N, K, scale=K ** -0.5, seed=2)
    n4 = (N + 3) // 4 * 4
    pad = n4 != N or N % 64 != 0
    wp = ops.split_weight_bf16x3(w, 3, pad=pad) if pad else ops.split_weight_bf16x3(w, 3)
    bias = _rand(n4, seed=3)
    res = _rand(Mx, n4, seed=4) if 'res' in epi else None
    act = 'gelu' if epi == 'gelu' else ('relu' in epi)
    with ops.form_policy(policy):
        _prefix_equal(lambda x: ops.gemm_bf16x3(x, wp, bias, None if res is None else res[:x.shape[0]], relu=act,
                                                n_out=n4 if pad else None), a)


@pytest.mark.parametrize('policy', [1, 2])
def test_row_gemm_epilogue_forms_do_not_depend_on_m(policy):
    """_ex with a row-periodic identity table (the decoders' folded positional term), _ln (LayerNorm epilogue)
    at K = 256 / 1024, and fp16 operand planes."""
    from pavenet_amd import ops
    # (LayerNorm: past the fused epilogue's 512-row-tile switch, 65 409 rows, and at 66 969 rows -- one R-50 T = 3
    # clip's encoder at 800 x 1344, 524 row tiles, which policy 0 cuts into a round of 65 536 and a tail)
    Mx = 70001
    for K in (64, 256, 1024):
        a = _rand(Mx, K, seed=5)
        w = _rand(256, K, scale=K ** -0.5, seed=6)
        wp = ops.split_weight_bf16x3(w, 3)
        b, g, be = _rand(256, seed=7), 1 + 0.1 * _rand(256, seed=8), _rand(256, seed=9)
        idt = _rand(Mx, 256, seed=10)
        tab = _rand(300, 256, seed=11)
        wf = ops.split_weight_bf16x3(w, ops.PLANES_FP16)
        with ops.form_policy(policy):
            _prefix_equal(lambda x: ops.gemm_bf16x3_ln(x, wp, b, idt[:x.shape[0]].clone(), g, be, 1e-5), a,
                          [1, 300, 1200, 2048, 2049, 2400, 3969, 8192, 65408, 65409, 66969])
            if K == 64:
                continue
            _prefix_equal(lambda x: ops.gemm_bf16x3_ex(x, wp, None, tab, residual_rows=300)[0], a,
                          [300, 1200, 2048, 2400, 4200])
            _prefix_equal(lambda x: ops.gemm_bf16x3(x, wf, b, None, fp16=True), a, [1, 300, 2048, 2049, 8192])


@pytest.mark.parametrize('policy', [1, 2])
def test_layernorm_gemm_beyond_its_identity_buffer_limit(policy):
    """Past 2^22 rows the wide LayerNorm form runs in row chunks under a form policy (policy 0 takes the 8-wave
    block there): a row's values are those of a launch over a few rows around it."""
    from pavenet_amd import ops
    M, K = (1 << 22) + 300, 64
    a = _rand(M, K, seed=40)
    w = _rand(256, K, scale=K ** -0.5, seed=41)
    wp = ops.split_weight_bf16x3(w, 3)
    b, g, be = _rand(256, seed=42), 1 + 0.1 * _rand(256, seed=43), _rand(256, seed=44)
    with ops.form_policy(policy):
        full = ops.gemm_bf16x3_ln(a, wp, b, None, g, be, 1e-5)
        for r0, r1 in ((0, 300), ((1 << 22) - 1000, (1 << 22) + 200), (M - 77, M)):
            assert torch.equal(ops.gemm_bf16x3_ln(a[r0:r1].contiguous(), wp, b, None, g, be, 1e-5), full[r0:r1])


def test_multi_tile_ksplit_form_equals_gemm_sk_kernel():
    """Policy 2 above 2 048 rows: gemm_skm_kernel (4 column tiles per block) against gemm_sk_kernel on the same
    launch (diag variant 21), bit for bit, with every epilogue."""
    from pavenet_amd import native, ops
    for K, N, M in ((1024, 256, 2400), (256, 512, 4801), (512, 192, 3000), (768, 1024, 2049)):
        a = _rand(M, K, seed=12)
        w = _rand(N, K, scale=K ** -0.5, seed=13)
        b, r = _rand(N, seed=14), _rand(M, N, seed=15)
        for act in (False, True, 'gelu', 'sigmoid'):
            outs = []
            for variant in (None, 21):
                if variant is None:
                    with ops.form_policy(2):
                        outs.append(ops.gemm_bf16x3(a, ops.split_weight_bf16x3(w, 3), b, r, relu=act))
                else:
                    with native.diag_build(variant), ops.form_policy(2):
                        outs.append(ops.gemm_bf16x3(a, ops.split_weight_bf16x3(w, 3), b, r, relu=act))
            assert torch.equal(outs[0], outs[1]), (K, N, M, act)
        g, be = 1 + 0.1 * _rand(256, seed=16), _rand(256, seed=17)
        if N == 256:
            outs = []
            for variant in (None, 21):
                wp = ops.split_weight_bf16x3(w, 3)
                if variant is None:
                    with ops.form_policy(2):
                        outs.append(ops.gemm_bf16x3_ln(a, wp, b, r.clone(), g, be, 1e-5))
                else:
                    with native.diag_build(variant), ops.form_policy(2):
                        outs.append(ops.gemm_bf16x3_ln(a, wp, b, r.clone(), g, be, 1e-5))
            assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize('policy', [1, 2])
def test_convolutions_of_one_image_equal_its_slot_in_a_batch(policy):
    """3x3 (K = 9 x 256 = 2 304: split-K parts for one 64 x 64 image, the tile kernels for four under policy 0),
    strided 1x1 with K = 2 048, and a backbone (bottleneck chains) on one image against a batch of 4.  (The strided
    1x1 has no split-K path: its part guards the narrow / wide switch by tile count -- 10 000 rows alone, 40 000 in
    the batch -- which must stay bit-identical under the policies.)"""
    from pavenet_amd import ops
    x = _rand(4, 256, 64, 64, seed=20).contiguous(memory_format=torch.channels_last)
    w = _rand(256, 256, 3, 3, scale=(9 * 256) ** -0.5, seed=21)
    wp = ops.split_conv3x3_weight(w)
    b = _rand(256, seed=22)
    x2 = _rand(4, 2048, 200, 200, seed=23).contiguous(memory_format=torch.channels_last)
    w2 = _rand(512, 2048, scale=2048 ** -0.5, seed=24)
    wp2 = ops.split_weight_bf16x3(w2, 3)
    with ops.form_policy(policy):
        full = ops.conv3x3_split(x, wp, b, relu=True)
        full2 = ops.conv1x1_strided_split(x2, wp2, b[:0].new_zeros(512), stride=2)
        for i in range(4):
            one = ops.conv3x3_split(x[i:i + 1].contiguous(memory_format=torch.channels_last), wp, b, relu=True)
            assert torch.equal(one, full[i:i + 1])
            one2 = ops.conv1x1_strided_split(x2[i:i + 1].contiguous(memory_format=torch.channels_last), wp2,
                                             b[:0].new_zeros(512), stride=2)
            assert torch.equal(one2, full2[i:i + 1])
    if policy != 1:
        return   # (pixel rows run under policy 1: the backbone picks its fused chains by row count in Python)
    from pavenet_amd.models import build_model, videopose_r50_cfg
    from pavenet_amd.weights import init_random_weights
    m = init_random_weights(build_model(videopose_r50_cfg(num_frames=3, max_per_img=4)), seed=0).cuda().eval()
    # 256 x 320 frames: layer1 is 5 120 pixel rows per frame -- the 64-channel chain takes four frames, not one
    img = _rand(4, 3, 256, 320, seed=25)
    with torch.no_grad(), ops.form_policy(policy):
        feats = m.backbone(img)
        for i in range(4):
            fi = m.backbone(img[i:i + 1])
            for a_, b_ in zip(fi, feats):
                assert torch.equal(a_, b_[i:i + 1])


def _model(backbone):
    from pavenet_amd.models import build_model, videopose_r50_cfg, with_hrnet_w48, with_swin_l
    from pavenet_amd.weights import init_random_weights
    cfg = videopose_r50_cfg(num_frames=3, max_per_img=12)
    if backbone == 'hrnet_w48':
        cfg = with_hrnet_w48(cfg)
    elif backbone == 'swin_l':
        cfg = with_swin_l(cfg, num_frames=3)
    return init_random_weights(build_model(cfg), seed=0).cuda().eval()


def _same_result(a, b, what):
    for k in ('bboxes', 'kpts', 'scores', 'keep'):
        assert torch.equal(a[k], b[k]), f'{what}: {k} differs'


def _meta(hw):
    return dict(batch_input_shape=(128, 160), img_shape=hw + (3,), scale_factor=(1., 1., 1., 1.))


@pytest.mark.parametrize('backbone', ['r50', 'hrnet_w48', 'swin_l'])
def test_clip_alone_equals_its_slot_in_the_batch(backbone):
    """T = 3, 128 x 160 canvas, 3 clips of which one is padded: each clip run alone equals its slot in the batch,
    bit for bit, with no forced selection."""
    from pavenet_amd.bricks import set_batch_invariant
    m = set_batch_invariant(_model(backbone))
    metas = [_meta((128, 160)), _meta((120, 150)), _meta((128, 160))]
    img = _rand(3, 3, 3, 128, 160, seed=30)
    with torch.no_grad():
        batch = m.forward_device(img, metas)
        for i in range(3):
            alone = m.forward_device(img[i:i + 1], metas[i:i + 1])
            _same_result({k: alone[k][0] for k in ('bboxes', 'kpts', 'scores', 'keep')},
                         {k: batch[k][i] for k in ('bboxes', 'kpts', 'scores', 'keep')}, f'{backbone} clip {i}')
        # simple_test / forward run under the same mode
        r1 = m.simple_test(img[1:2], metas[1:2])[0]
        r2 = m.forward(img, metas)[1]
        for x, y in zip(r1, r2):
            for u, v in zip(x, y):
                assert (u == v).all()


def test_streaming_equals_per_window_forward_device():
    from pavenet_amd.bricks import set_batch_invariant
    from pavenet_amd.streaming import VideoPoseStream
    m = set_batch_invariant(_model('r50'))
    meta = _meta((128, 160))
    video = _rand(6, 3, 128, 160, seed=31)
    stream = VideoPoseStream(m, meta, encode_chunk=4, decode_chunk=4)
    got = stream.infer_video(video)
    for c, w in enumerate(stream.window_indices(6, 3)):
        exp = m.bbox_head.results_to_list(m.forward_device(video[w][None], [meta]))[0]
        for x, y in zip(got[c], exp):
            assert torch.equal(x, y), f'frame {c}'


def test_default_mode_is_unchanged_after_the_batch_invariant_mode():
    from pavenet_amd import native
    from pavenet_amd.bricks import set_batch_invariant
    m = _model('r50')
    metas = [_meta((128, 160)), _meta((120, 150))]
    img = _rand(2, 3, 3, 128, 160, seed=32)
    with torch.no_grad():
        before = m.forward_device(img, metas)
        set_batch_invariant(m)
        m.forward_device(img, metas)
        set_batch_invariant(m, False)
        assert native.load().pave_get_form_policy() == 0
        after = m.forward_device(img, metas)
    _same_result(before, after, 'default mode')


def test_bench_batch_clip_alone_equals_its_slot():
    """configs[2] at full size (R-50, T = 7, 4 clips, 800 x 1344, seeded init_random_weights as bench.py builds it):
    clip 0 alone equals clip 0 of the 4-clip batch."""
    from pavenet_amd.bricks import set_batch_invariant
    from pavenet_amd.models import build_model, videopose_r50_cfg
    from pavenet_amd.weights import init_random_weights
    m = init_random_weights(build_model(videopose_r50_cfg(num_frames=7, max_per_img=20)), seed=0).cuda().eval()
    set_batch_invariant(m)
    metas = [dict(batch_input_shape=(800, 1344), img_shape=(800, 1344, 3), scale_factor=(1., 1., 1., 1.))] * 4
    g = torch.Generator(device='cuda').manual_seed(4321)
    img = torch.randn(4, 7, 3, 800, 1344, device='cuda', generator=g)
    with torch.no_grad():
        batch = m.forward_device(img, metas)
        alone = m.forward_device(img[:1], metas[:1])
    _same_result({k: alone[k][0] for k in ('bboxes', 'kpts', 'scores', 'keep')},
                 {k: batch[k][0] for k in ('bboxes', 'kpts', 'scores', 'keep')}, 'configs[2] clip 0')


def test_full_canvas_crosses_the_layernorm_forms():
    """R-50, T = 3 at 800 x 1344: one clip's encoder is 66 969 rows (524 row tiles, which policy 0 cuts into a
    round and a tail of the 8-wave LayerNorm form), two clips 133 938; streaming encodes 9 frames as chunks of 8 and
    1 (22 323 rows: the 8-wave form under policy 0) and decodes what per-window forward_device computes from 66 969
    rows.  Alone equals its slot, streaming equals forward_device, bit for bit."""
    from pavenet_amd.bricks import set_batch_invariant
    from pavenet_amd.streaming import VideoPoseStream
    m = set_batch_invariant(_model('r50'))
    meta = dict(batch_input_shape=(800, 1344), img_shape=(800, 1344, 3), scale_factor=(1., 1., 1., 1.))
    img = _rand(2, 3, 3, 800, 1344, seed=50)
    with torch.no_grad():
        batch = m.forward_device(img, [meta] * 2)
        for i in range(2):
            alone = m.forward_device(img[i:i + 1], [meta])
            _same_result({k: alone[k][0] for k in ('bboxes', 'kpts', 'scores', 'keep')},
                         {k: batch[k][i] for k in ('bboxes', 'kpts', 'scores', 'keep')}, f'800x1344 clip {i}')
    video = _rand(9, 3, 800, 1344, seed=51)
    stream = VideoPoseStream(m, meta, encode_chunk=8, decode_chunk=4)
    got = stream.infer_video(video)
    for c, w in enumerate(stream.window_indices(9, 3)):
        exp = m.bbox_head.results_to_list(m.forward_device(video[w][None], [meta]))[0]
        for x, y in zip(got[c], exp):
            assert torch.equal(x, y), f'frame {c}'
