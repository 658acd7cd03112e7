"""Live video on the device: LiveVideoPose's ring against VideoPoseStream.infer_video, bit for bit under
set_batch_invariant (128 x 160 canvases, R-50, max_per_img = 12, seeded random weights), and the NV12 ingest kernel
against preprocess_clip on a host restatement of the colour conversion.  Needs an MI355X."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu


def _rand(*shape, seed=0):
    g = torch.Generator(device='cuda').manual_seed(seed)
    return torch.randn(*shape, device='cuda', generator=g)


@functools.lru_cache(maxsize=None)
def _model(T):
    from pavenet_amd.bricks import set_batch_invariant
    from pavenet_amd.models import build_model, videopose_r50_cfg
    from pavenet_amd.weights import init_random_weights
    m = init_random_weights(build_model(videopose_r50_cfg(num_frames=T, max_per_img=12)), seed=0).cuda().eval()
    return set_batch_invariant(m)


def _meta(hw=(128, 160)):
    return dict(batch_input_shape=(128, 160), img_shape=hw + (3,), scale_factor=(1., 1., 1., 1.))


def _offline(T, video, meta):
    from pavenet_amd.streaming import VideoPoseStream
    return VideoPoseStream(_model(T), meta, encode_chunk=4, decode_chunk=4).infer_video(video)


def _run(live, video, pushes):
    """push ... flush -> ([(index, result)] of the pushes, [(index, result)] of the flush)."""
    assert sum(pushes) == video.shape[0]
    got, at = [], 0
    for p in pushes:
        got += live.push(video[at] if p == 1 and at % 2 == 0 else video[at:at + p])   # both input forms
        at += p
    return got, live.flush()


def _assert_equal(got, exp, what):
    assert [i for i, _ in got] == list(range(len(exp))), f'{what}: frame indices {[i for i, _ in got]}'
    for i, res in got:
        assert len(res) == 3
        for x, y, name in zip(res, exp[i], ('bboxes', 'labels', 'kpts')):
            assert x.shape == y.shape and torch.equal(x, y), f'{what}: frame {i} {name}'


def test_live_equals_offline_t3():
    from pavenet_amd.live import LiveVideoPose
    m, meta = _model(3), _meta()
    video = _rand(7, 3, 128, 160, seed=61)
    exp = _offline(3, video, meta)
    live = LiveVideoPose(m, meta, max_push=1, decode_chunk=4)
    pushed, flushed = _run(live, video, [1] * 7)
    assert [i for i, _ in pushed] == [0, 1, 2, 3, 4, 5] and [i for i, _ in flushed] == [6]
    _assert_equal(pushed + flushed, exp, 'T = 3')
    assert all(torch.isfinite(r[2]).all() for _, r in pushed + flushed) and len(exp[3][2]) > 0
    with torch.no_grad():
        fd = m.bbox_head.results_to_list(m.forward_device(video[[2, 3, 4]][None], [meta]))[0]
    for x, y in zip(pushed[3][1], fd):
        assert torch.equal(x, y), 'frame 3 against forward_device on its window'
    # the ring is what the docstring says: T - 1 + max_push slots of memory and five value caches
    S = live.ring.memory.shape[1]
    assert live.ring.memory.shape == (3, S, 256) and live.ring.n_slots == 3
    assert [tuple(v.shape) for v in live.ring.values[0] + live.ring.values[1]] == [(3, S, 8, 32)] * 5
    assert live.ring.resident_bytes() == 3 * S * 256 * 4 * 6


def test_ring_wraps_more_than_twice_t5():
    """R = 7 slots, 17 frames; the slots hold NaN before the run, so a window that read a slot no frame of this
    video was written to (or a stale one) cannot equal the offline result."""
    from pavenet_amd.live import LiveVideoPose
    m, meta = _model(5), _meta()
    video = _rand(17, 3, 128, 160, seed=62)
    exp = _offline(5, video, meta)
    live = LiveVideoPose(m, meta, max_push=3, decode_chunk=4)
    assert live.ring.n_slots == 7
    live.push(video[:1])          # a first video allocates the ring ...
    live.flush()
    live.reset()
    live.ring.fill_(float('nan'))  # ... which is then poisoned
    assert all(torch.isnan(t).all() for t in live.ring.tensors()) and len(live.ring.tensors()) == 6
    pushed, flushed = _run(live, video, [1, 3, 2, 3, 1, 3, 3, 1])
    assert [i for i, _ in flushed] == [15, 16]
    _assert_equal(pushed + flushed, exp, 'T = 5, 17 frames')
    assert all(torch.isfinite(x).all() for _, r in pushed + flushed for x in (r[0], r[2]))


def test_padded_meta_keeps_memory_slabs_only():
    from pavenet_amd.live import LiveVideoPose
    m, meta = _model(3), _meta((120, 150))
    video = _rand(6, 3, 128, 160, seed=63)
    exp = _offline(3, video, meta)
    live = LiveVideoPose(m, meta, max_push=2, decode_chunk=2)
    pushed, flushed = _run(live, video, [2, 1, 2, 1])
    assert live.ring.values is None and live.ring.memory.shape[0] == 4 and not live.ring.covers([0])
    _assert_equal(pushed + flushed, exp, 'padded')


def test_reset_starts_a_new_video_in_the_same_slots():
    from pavenet_amd.live import LiveVideoPose
    m, meta = _model(3), _meta()
    a, b = _rand(5, 3, 128, 160, seed=64), _rand(4, 3, 128, 160, seed=65)
    live = LiveVideoPose(m, meta, max_push=2)
    _run(live, a, [2, 2, 1])
    ptrs = [t.data_ptr() for t in live.ring.tensors()]
    live.reset()
    pushed, flushed = _run(live, b, [1, 2, 1])
    assert [t.data_ptr() for t in live.ring.tensors()] == ptrs
    fresh = LiveVideoPose(m, meta, max_push=2)
    fp, ff = _run(fresh, b, [1, 2, 1])
    _assert_equal(pushed + flushed, [r for _, r in fp + ff], 'after reset()')
    assert [i for i, _ in fp + ff] == [0, 1, 2, 3]


@pytest.mark.parametrize('n', [1, 2])
def test_short_videos_come_out_of_flush(n):
    from pavenet_amd.live import LiveVideoPose
    m, meta = _model(5), _meta()
    video = _rand(n, 3, 128, 160, seed=66)
    exp = _offline(5, video, meta)
    live = LiveVideoPose(m, meta, max_push=1)
    pushed, flushed = _run(live, video, [1] * n)
    assert pushed == [] and len(flushed) == n
    _assert_equal(flushed, exp, f'N = {n}')
    assert live.flush() == []        # nothing is emitted twice


def test_memory_is_bounded():
    from pavenet_amd.live import LiveVideoPose
    m, meta = _model(3), _meta()
    R = 3
    video = _rand(4 * R + 2, 3, 128, 160, seed=67)
    live = LiveVideoPose(m, meta, max_push=1)
    assert live.ring.n_slots == R

    def span(lo, hi):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        for f in range(lo, hi):
            assert [i for i, _ in live.push(video[f])] == [f - 1]
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated()
    for f in range(R):
        live.push(video[f])
    ptrs = [t.data_ptr() for t in live.ring.tensors()]
    early = span(R, 2 * R)
    late = span(2 * R, 4 * R)
    print(f'peak bytes allocated: pushes R..2R {early}, pushes 2R..4R {late}')
    assert late <= early
    for f in range(4 * R, 4 * R + 2):
        live.push(video[f])
    assert [t.data_ptr() for t in live.ring.tensors()] == ptrs and len(ptrs) == 6


def test_infer_frames_over_chunks_equals_infer_video():
    from pavenet_amd.streaming import VideoPoseStream
    m, meta = _model(3), _meta()
    video = _rand(7, 3, 128, 160, seed=68)
    exp = _offline(3, video, meta)
    stream = VideoPoseStream(m, meta, encode_chunk=4, decode_chunk=4)
    got = list(stream.infer_frames(video[i:i + 2] for i in range(0, 7, 2)))
    _assert_equal(got, exp, 'infer_frames')


def test_push_argument_errors():
    from pavenet_amd.live import LiveVideoPose
    live = LiveVideoPose(_model(3), _meta(), max_push=2)
    with pytest.raises(ValueError, match='max_push'):
        live.push(_rand(3, 3, 128, 160))
    with pytest.raises(ValueError, match='device'):
        live.push(torch.zeros(3, 128, 160))
    live.push(_rand(3, 128, 160))
    with pytest.raises(ValueError, match='canvas'):
        live.push(_rand(3, 128, 192))
    assert live.n_seen == 1


# ---- NV12 ingest ----

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
    B = t + U * cbu
    G = (t + U * cgu) + V * cgv
    R = t + V * crv
    bgr = torch.stack([B, G, R], -1)
    assert bgr.dtype == torch.float32
    return torch.round(bgr).clamp(0, 255).to(torch.uint8), bgr


@pytest.mark.parametrize('pitch', [64, 50])
def test_nv12_ingest_equals_preprocess_clip_on_the_converted_image(pitch):
    from pavenet_amd.preprocess import nv12_csc, preprocess_clip, preprocess_clip_nv12
    T, H0, W0 = 2, 36, 50
    g = torch.Generator().manual_seed(70 + pitch)
    surfaces = torch.randint(0, 256, (T, H0 * 3 // 2, pitch), dtype=torch.uint8, generator=g)

    def uniform(n):     # n bytes in random order, every value as often as the next (n >= 256: each at least once)
        return (torch.arange(n) % 256)[torch.randperm(n, generator=g)].to(torch.uint8)
    surfaces[:, :H0, :W0] = uniform(T * H0 * W0).view(T, H0, W0)
    surfaces[:, H0:, 0:W0:2] = uniform(T * H0 * W0 // 4).view(T, H0 // 2, W0 // 2)
    surfaces[:, H0:, 1:W0:2] = uniform(T * H0 * W0 // 4).view(T, H0 // 2, W0 // 2)
    for plane in (surfaces[:, :H0, :W0], surfaces[:, H0:, 0:W0:2], surfaces[:, H0:, 1:W0:2]):
        assert len(plane.unique()) == 256, 'every byte value on every plane'
    other = surfaces.clone()
    if pitch > W0:     # what lies beyond the width must not matter
        other[:, :, W0:] = torch.randint(0, 256, (T, H0 * 3 // 2, pitch - W0), dtype=torch.uint8, generator=g)
        assert not torch.equal(other, surfaces)
    dev, dev_other = surfaces.cuda(), other.cuda()
    for matrix in ('bt601', 'bt709'):
        for full_range in (False, True):
            bgr, raw = _nv12_to_bgr_host(surfaces, H0, W0, nv12_csc(matrix, full_range))
            assert (raw < -0.5).any() and (raw > 255.5).any(), 'both clamps occur'
            frames = bgr.cuda()
            for img_scale in ((80, 48), (30, 20)):
                for size_divisor in (1, 32):
                    exp, exp_meta = preprocess_clip(frames, img_scale, size_divisor)
                    got, meta = preprocess_clip_nv12(dev, W0, img_scale, size_divisor, matrix=matrix,
                                                     full_range=full_range)
                    what = f'{matrix} full_range={full_range} {img_scale} / {size_divisor}'
                    assert got.shape == exp.shape and torch.equal(got, exp), what
                    assert meta == exp_meta, what
                    again, _ = preprocess_clip_nv12(dev_other, W0, img_scale, size_divisor, matrix=matrix,
                                                    full_range=full_range)
                    assert torch.equal(again, exp), what + ': bytes beyond the width'
    # the other switches of the pipeline go through unchanged
    bgr, _ = _nv12_to_bgr_host(surfaces, H0, W0, nv12_csc('bt709', False))
    exp, _ = preprocess_clip(bgr.cuda(), (80, 48), 32, mean=(1., 2., 3.), std=(4., 5., 6.), to_rgb=False)
    got, _ = preprocess_clip_nv12(dev, W0, (80, 48), 32, mean=(1., 2., 3.), std=(4., 5., 6.), to_rgb=False,
                                  matrix='bt709')
    assert torch.equal(got, exp)


def test_nv12_surfaces_into_live():
    from pavenet_amd.live import LiveVideoPose
    from pavenet_amd.preprocess import preprocess_clip_nv12
    g = torch.Generator().manual_seed(71)
    surfaces = torch.randint(0, 256, (3, 96 * 3 // 2, 128), dtype=torch.uint8, generator=g).cuda()
    img, meta = preprocess_clip_nv12(surfaces, 120, img_scale=(160, 128), size_divisor=32)
    assert img.shape == (1, 3, 3, 128, 160) and meta['img_shape'] == (128, 160, 3) and meta['ori_shape'] == (96, 120, 3)
    live = LiveVideoPose(_model(3), meta, max_push=3, rescale=True)
    got = live.push(img[0]) + live.flush()
    assert [i for i, _ in got] == [0, 1, 2]
    for _, (bboxes, labels, kpts) in got:
        n = bboxes.shape[0]
        assert n <= 12 and bboxes.shape == (n, 5) and labels.shape == (n,) and kpts.shape == (n, 15, 3)
        assert torch.isfinite(bboxes).all() and torch.isfinite(kpts).all()
