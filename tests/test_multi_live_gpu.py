"""Multi-camera live video on the device: every camera of a MultiLiveVideoPose against a LiveVideoPose of its own
and against VideoPoseStream.infer_video, bit for bit under set_batch_invariant (128 x 160 canvases, R-50,
max_per_img = 12, seeded random weights); the ring write (ops.scatter_rows) against the indexed assignment and the
multi-surface NV12 ingest against preprocess_clip_nv12 surface by surface.  Needs an MI355X."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _split_gemm_mode():
    """set_batch_invariant needs the library's default GEMM mode, whatever mode an earlier module left behind."""
    from pavenet_amd import bricks
    old = bricks.get_gemm_mode()
    bricks.set_gemm_mode('bf16x3')
    yield
    bricks.set_gemm_mode(old)


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


def _run_multi(multi, videos, pushes, at=None, flush=True):
    """videos {camera: [N, 3, H, W]} delivered as `pushes` (a list of {camera: n}), then flush() -> {camera: one
    [(index, result)] list per push that named it and a last one for the flush}."""
    at = {c: 0 for c in videos} if at is None else at
    out = {c: [] for c in videos}
    for push in pushes:
        batch = {}
        for c, n in push.items():
            clip = videos[c][at[c]:at[c] + n]
            batch[c] = clip[0] if n == 1 and at[c] % 2 == 0 else clip      # both input forms
            at[c] += n
        got = multi.push(batch)
        assert [(c, i) for c, i, _ in got] == sorted((c, i) for c, i, _ in got) and {c for c, _, _ in got} <= set(push)
        for c in push:
            out[c].append([(i, r) for cc, i, r in got if cc == c])
    if flush:
        got = multi.flush()
        assert [(c, i) for c, i, _ in got] == sorted((c, i) for c, i, _ in got)
        for c in videos:
            out[c].append([(i, r) for cc, i, r in got if cc == c])
    return out


def _run_alone(live, video, own):
    """The same camera on a LiveVideoPose of its own -> one [(index, result)] list per push and one for the flush."""
    steps, at = [], 0
    for n in own:
        steps.append(live.push(video[at:at + n]))
        at += n
    assert at == video.shape[0]
    return steps + [live.flush()]


def _assert_steps_equal(got, exp, what):
    assert [[i for i, _ in s] for s in got] == [[i for i, _ in s] for s in exp], f'{what}: what each push emits'
    for s, t in zip(got, exp):
        for (i, res), (_, ref) in zip(s, t):
            assert len(res) == 3
            for x, y, name in zip(res, ref, ('bboxes', 'labels', 'kpts')):
                assert x.shape == y.shape and torch.equal(x, y), f'{what}: frame {i} {name}'


def _assert_equal_offline(steps, exp, what):
    flat = [item for s in steps for item in s]
    assert [i for i, _ in flat] == list(range(len(exp))), f'{what}: frame indices {[i for i, _ in flat]}'
    for i, res in flat:
        for x, y, name in zip(res, exp[i], ('bboxes', 'labels', 'kpts')):
            assert x.shape == y.shape and torch.equal(x, y), f'{what}: frame {i} {name} against infer_video'


def _poison(multi, videos):
    """A first throw-away video allocates the ring, which is then filled with NaN: a window that read a row no
    frame of this video was written to (or another camera's) cannot equal the reference."""
    multi.push({c: v[0] for c, v in videos.items()})
    multi.flush()
    multi.reset()
    multi.ring.fill_(float('nan'))
    assert all(torch.isnan(t).all() for t in multi.ring.tensors())


def test_three_cameras_equal_their_own_live_video_pose():
    from pavenet_amd.live import LiveVideoPose, MultiLiveVideoPose
    T, m, meta = 3, _model(3), _meta()
    videos = {0: _rand(7, 3, 128, 160, seed=81), 1: _rand(5, 3, 128, 160, seed=82), 2: _rand(1, 3, 128, 160, seed=83)}
    pushes = [{0: 1, 1: 2}, {0: 2}, {0: 1, 1: 1, 2: 1}, {1: 2}, {0: 2}, {0: 1}]
    multi = MultiLiveVideoPose(m, meta, cameras=3, max_push=2, decode_chunk=4)
    R = multi.ring.n_slots
    assert R == 4 and multi.ring.cameras == 3
    _poison(multi, videos)
    assert len(multi.ring.tensors()) == 6
    got = _run_multi(multi, videos, pushes)
    for c, video in videos.items():
        own = [p[c] for p in pushes if c in p]
        alone = _run_alone(LiveVideoPose(m, meta, max_push=2, decode_chunk=4), video, own)
        _assert_steps_equal(got[c], alone, f'camera {c}')
        _assert_equal_offline(got[c], _offline(T, video, meta), f'camera {c}')
        assert all(torch.isfinite(x).all() for s in got[c] for _, r in s for x in (r[0], r[2]))
    assert got[2][0] == [] and [i for i, _ in got[2][1]] == [0], 'the one-frame camera comes out of flush'
    assert sum(len(r[2]) for s in got[0] for _, r in s) > 0, 'some poses are found'
    assert multi.flush() == [], 'nothing is emitted twice'
    S = multi.ring.memory.shape[1]
    assert multi.ring.memory.shape == (3 * R, S, 256)
    assert [tuple(v.shape) for v in multi.ring.values[0] + multi.ring.values[1]] == [(3 * R, S, 8, 32)] * 5
    assert multi.ring.resident_bytes() == 3 * R * S * 256 * 4 * 6


def test_ring_wraps_t5_two_cameras():
    """R = 7 rows per camera, 17 and 11 frames: camera 0's rows wrap more than twice, camera 1's once, in pushes
    of 1 .. 3 frames that sometimes omit camera 1; rows poisoned with NaN before the run."""
    from pavenet_amd.live import MultiLiveVideoPose
    T, m, meta = 5, _model(5), _meta()
    videos = {0: _rand(17, 3, 128, 160, seed=84), 1: _rand(11, 3, 128, 160, seed=85)}
    pushes = [{0: 1, 1: 3}, {0: 3}, {0: 2, 1: 3}, {0: 3, 1: 2}, {0: 1}, {0: 3, 1: 3}, {0: 3}, {0: 1}]
    multi = MultiLiveVideoPose(m, meta, cameras=2, max_push=3, decode_chunk=4)
    assert multi.ring.n_slots == 7
    _poison(multi, videos)
    got = _run_multi(multi, videos, pushes)
    assert multi.ring.n_frames == [17, 11] and multi.ring.n_cached == [17, 11]
    for c, video in videos.items():
        _assert_equal_offline(got[c], _offline(T, video, meta), f'camera {c}')
        assert [i for i, _ in got[c][-1]] == [len(video) - 2, len(video) - 1]
        assert all(torch.isfinite(x).all() for s in got[c] for _, r in s for x in (r[0], r[2]))


def test_encode_chunk_smaller_than_a_push():
    from pavenet_amd.live import MultiLiveVideoPose
    T, m, meta = 3, _model(3), _meta()
    videos = {0: _rand(5, 3, 128, 160, seed=86), 1: _rand(4, 3, 128, 160, seed=87)}
    multi = MultiLiveVideoPose(m, meta, cameras=2, max_push=2, decode_chunk=3, encode_chunk=3)
    got = _run_multi(multi, videos, [{0: 2, 1: 2}, {0: 2, 1: 2}, {0: 1}])
    for c, video in videos.items():
        _assert_equal_offline(got[c], _offline(T, video, meta), f'camera {c}')


def test_flush_and_reset_of_one_camera():
    from pavenet_amd.live import LiveVideoPose, MultiLiveVideoPose
    m, meta = _model(3), _meta()
    a = _rand(8, 3, 128, 160, seed=88)
    b1, b2 = _rand(3, 3, 128, 160, seed=89), _rand(4, 3, 128, 160, seed=90)
    multi = MultiLiveVideoPose(m, meta, cameras=2, max_push=2, decode_chunk=4)
    at = {0: 0, 1: 0}
    first = _run_multi(multi, {0: a, 1: b1}, [{0: 2, 1: 1}, {0: 1, 1: 2}], at, flush=False)
    ptrs = [t.data_ptr() for t in multi.ring.tensors()]
    flushed = multi.flush(camera=1)
    assert [(c, i) for c, i, _ in flushed] == [(1, 2)] and multi.flush(camera=1) == []
    multi.reset(camera=1)
    assert multi.n_seen == [3, 0] and multi.ring.n_frames == [3, 0]
    at[1] = 0
    second = _run_multi(multi, {0: a, 1: b2}, [{0: 2, 1: 2}, {1: 1}, {0: 2, 1: 1}, {0: 1}], at)
    assert [t.data_ptr() for t in multi.ring.tensors()] == ptrs and len(ptrs) == 6
    alone0 = _run_alone(LiveVideoPose(m, meta, max_push=2), a, [2, 1, 2, 2, 1])
    _assert_steps_equal(first[0] + second[0], alone0, 'camera 0, uninterrupted')
    alone1 = _run_alone(LiveVideoPose(m, meta, max_push=2), b1, [1, 2])
    _assert_steps_equal(first[1] + [[(i, r) for _, i, r in flushed]], alone1, 'camera 1, first video')
    fresh = _run_alone(LiveVideoPose(m, meta, max_push=2), b2, [2, 1, 1])
    _assert_steps_equal(second[1], fresh, 'camera 1, second video')


def test_padded_meta_keeps_memory_only():
    from pavenet_amd.live import MultiLiveVideoPose
    m, meta = _model(3), _meta((120, 150))
    videos = {0: _rand(5, 3, 128, 160, seed=91), 1: _rand(3, 3, 128, 160, seed=92)}
    multi = MultiLiveVideoPose(m, meta, cameras=2, max_push=2, decode_chunk=2)
    got = _run_multi(multi, videos, [{0: 2, 1: 1}, {0: 1}, {0: 2, 1: 2}])
    assert multi.ring.values is None and multi.ring.memory.shape[0] == 2 * 4 and not multi.ring.covers([0])
    assert len(multi.ring.tensors()) == 1
    for c, video in videos.items():
        _assert_equal_offline(got[c], _offline(3, video, meta), f'camera {c}, padded')


def test_memory_is_bounded_with_two_cameras():
    from pavenet_amd.live import MultiLiveVideoPose
    m, meta = _model(3), _meta()
    R = 3
    videos = [_rand(4 * R + 2, 3, 128, 160, seed=93 + c) for c in range(2)]
    multi = MultiLiveVideoPose(m, meta, cameras=2, max_push=1)
    assert multi.ring.n_slots == R

    def span(lo, hi):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        for f in range(lo, hi):
            assert [(c, i) for c, i, _ in multi.push({0: videos[0][f], 1: videos[1][f]})] == [(0, f - 1), (1, f - 1)]
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated()
    for f in range(R):
        multi.push({0: videos[0][f], 1: videos[1][f]})
    ptrs = [t.data_ptr() for t in multi.ring.tensors()]
    early = span(R, 2 * R)
    late = span(2 * R, 4 * R)
    print(f'peak bytes allocated: pushes R..2R {early}, pushes 2R..4R {late}')
    assert late <= early
    for f in range(4 * R, 4 * R + 2):
        multi.push({0: videos[0][f], 1: videos[1][f]})
    assert [t.data_ptr() for t in multi.ring.tensors()] == ptrs and len(ptrs) == 6


def test_a_failed_push_changes_nothing():
    from pavenet_amd.live import MultiLiveVideoPose
    m, meta = _model(3), _meta()
    multi = MultiLiveVideoPose(m, meta, cameras=2, max_push=2)
    good, wide = _rand(2, 3, 128, 160, seed=95), _rand(3, 128, 192, seed=96)
    with pytest.raises(ValueError, match='canvas'):      # the first push: the cameras disagree
        multi.push({0: good, 1: wide})
    assert multi.n_seen == [0, 0] and multi._canvas is None and multi.ring.memory is None
    assert [(c, i) for c, i, _ in multi.push({0: good[0], 1: good})] == [(1, 0)]
    seen, nxt, frames = list(multi.n_seen), list(multi.next_centre), list(multi.ring.n_frames)
    assert seen == [1, 2]
    for batch, match in (({0: good[0], 1: wide}, 'canvas'), ({0: good[0], 2: good[0]}, 'camera'),
                         ({0: good[0], -1: good[0]}, 'camera'), ({0: good[0], 1: _rand(3, 3, 128, 160)}, 'max_push'),
                         ({0: good[0], 1: torch.zeros(3, 128, 160)}, 'device'), ({}, 'dict'),
                         ({0: good[0], 1: good[0, 0]}, 'tensor'), (good, 'dict')):
        with pytest.raises(ValueError, match=match):
            multi.push(batch)
        assert multi.n_seen == seen and multi.next_centre == nxt and multi.ring.n_frames == frames
    with pytest.raises(ValueError, match='camera'):
        multi.flush(camera=2)
    # the object still works: camera 0's frame 1 completes its centre 0
    assert [(c, i) for c, i, _ in multi.push({0: good[1]})] == [(0, 0)]


@pytest.mark.parametrize('row_elems', [1028, 4])
def test_scatter_rows(row_elems, monkeypatch):
    """1028 elements per row are a multiple of 4 but not of a block's span (256 lanes x 4), 4 the smallest allowed."""
    from pavenet_amd import ops
    k, n, dst_rows, rows = 6, 5, 7, [6, 0, 3, 1, 5]
    shape = (row_elems // 4, 4)
    srcs = [_rand(n, *shape, seed=100 + t) for t in range(k)]
    kept = [s.clone() for s in srcs]
    dsts = [torch.full((dst_rows,) + shape, float('nan'), device='cuda') for _ in range(k)]
    launches = []
    real = ops._launch
    monkeypatch.setattr(ops, '_launch', lambda *a, **kw: (launches.append(a[0]), real(*a, **kw))[1])
    ops.scatter_rows(srcs, dsts, rows)
    assert launches == ['pave_scatter_rows_f32']
    for s, keep, d in zip(srcs, kept, dsts):
        assert torch.equal(d[rows], s) and torch.equal(s, keep), 'the named rows are the sources, which are unchanged'
        assert torch.isnan(d[[2, 4]]).all(), 'rows 2 and 4 were not written'
    # 70 rows: two launches
    del launches[:]
    g = torch.Generator().manual_seed(7)
    many = torch.randperm(80, generator=g)[:70].tolist()
    src, dst = _rand(70, *shape, seed=110), torch.full((80,) + shape, float('nan'), device='cuda')
    ops.scatter_rows([src], [dst], many)
    assert launches == ['pave_scatter_rows_f32'] * 2
    assert torch.equal(dst[many], src)
    assert torch.isnan(dst[sorted(set(range(80)) - set(many))]).all()
    # a non-default stream
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    dst2 = torch.full((dst_rows,) + shape, float('nan'), device='cuda')
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        ops.scatter_rows([srcs[0]], [dst2], rows)
    side.synchronize()
    assert torch.equal(dst2[rows], srcs[0]) and torch.isnan(dst2[[2, 4]]).all()


def _surface(H0, W0, pitch, g):
    """One [H0 * 3 // 2, pitch] NV12 surface on which every byte value occurs on every plane."""
    s = torch.randint(0, 256, (H0 * 3 // 2, pitch), dtype=torch.uint8, generator=g)

    def uniform(n):
        return (torch.arange(n) % 256)[torch.randperm(n, generator=g)].to(torch.uint8)
    s[:H0, :W0] = uniform(H0 * W0).view(H0, W0)
    s[H0:, 0:W0:2] = uniform(H0 * W0 // 4).view(H0 // 2, W0 // 2)
    s[H0:, 1:W0:2] = uniform(H0 * W0 // 4).view(H0 // 2, W0 // 2)
    for plane in (s[:H0, :W0], s[H0:, 0:W0:2], s[H0:, 1:W0:2]):
        assert len(plane.unique()) == 256, 'every byte value on every plane'
    return s


def test_preprocess_surfaces_nv12_equals_the_single_surface_kernel(monkeypatch):
    from pavenet_amd import preprocess
    from pavenet_amd.preprocess import preprocess_clip_nv12, preprocess_surfaces_nv12
    H0, W0, pitches = 36, 50, (64, 50, 72)
    settings = [('bt601', False), ('bt709', True), ('bt601', True)]
    g = torch.Generator().manual_seed(120)
    host = [_surface(H0, W0, p, g) for p in pitches]
    other = [s.clone() for s in host]
    for s, p in zip(other, pitches):          # what lies beyond the width must not matter
        s[:, W0:] = torch.randint(0, 256, (H0 * 3 // 2, p - W0), dtype=torch.uint8, generator=g)
    assert not torch.equal(other[0], host[0]) and not torch.equal(other[2], host[2])
    surfaces, beyond = [s.cuda() for s in host], [s.cuda() for s in other]      # separately allocated
    matrix, full_range = [m for m, _ in settings], [f for _, f in settings]
    for img_scale, divisor in (((80, 48), 32), ((30, 20), 1)):
        got, meta = preprocess_surfaces_nv12(surfaces, W0, img_scale, divisor, matrix=matrix, full_range=full_range)
        again, _ = preprocess_surfaces_nv12(beyond, W0, img_scale, divisor, matrix=matrix, full_range=full_range)
        for i, (m, f) in enumerate(settings):
            exp, exp_meta = preprocess_clip_nv12(surfaces[i][None], W0, img_scale, divisor, matrix=m, full_range=f)
            what = f'surface {i} {m} full_range={f} {img_scale} / {divisor}'
            assert got.shape == (3,) + exp.shape[2:] and torch.equal(got[i], exp[0, 0]), what
            assert torch.equal(again[i], exp[0, 0]), what + ': bytes beyond the width'
            assert meta == exp_meta, what
        # one value for all surfaces
        got, _ = preprocess_surfaces_nv12(surfaces, W0, img_scale, divisor, matrix='bt709', full_range=False)
        for i in range(3):
            exp, _ = preprocess_clip_nv12(surfaces[i][None], W0, img_scale, divisor, matrix='bt709')
            assert torch.equal(got[i], exp[0, 0])
    # mean, std and to_rgb go through unchanged
    kw = dict(mean=(1., 2., 3.), std=(4., 5., 6.), to_rgb=False)
    got, _ = preprocess_surfaces_nv12(surfaces, W0, (80, 48), 32, matrix=matrix, full_range=full_range, **kw)
    for i, (m, f) in enumerate(settings):
        exp, _ = preprocess_clip_nv12(surfaces[i][None], W0, (80, 48), 32, matrix=m, full_range=f, **kw)
        assert torch.equal(got[i], exp[0, 0])
    # 33 surfaces: two launches, equal surface by surface
    many = [surfaces[i % 3].roll(i, 1) for i in range(33)]       # 33 allocations, pitches 64, 50, 72 in turn
    many_set = [settings[(i + i // 3) % 3] for i in range(33)]
    launches = []
    real = preprocess._launch
    monkeypatch.setattr(preprocess, '_launch', lambda *a, **k: (launches.append(a[0]), real(*a, **k))[1])
    got, _ = preprocess_surfaces_nv12(many, W0, (80, 48), 32, matrix=[m for m, _ in many_set],
                                      full_range=[f for _, f in many_set])
    assert launches == ['pave_preprocess_surfaces_nv12'] * 2 and got.shape[0] == 33
    for i, (m, f) in enumerate(many_set):
        exp, _ = preprocess_clip_nv12(many[i][None], W0, (80, 48), 32, matrix=m, full_range=f)
        assert torch.equal(got[i], exp[0, 0]), f'surface {i} of 33'


def test_nv12_surfaces_of_three_cameras_into_live():
    from pavenet_amd.live import LiveVideoPose, MultiLiveVideoPose
    from pavenet_amd.preprocess import preprocess_clip_nv12, preprocess_surfaces_nv12
    g = torch.Generator().manual_seed(121)
    surfaces = [torch.randint(0, 256, (96 * 3 // 2, p), dtype=torch.uint8, generator=g).cuda() for p in (128, 120, 136)]
    img, meta = preprocess_surfaces_nv12(surfaces, 120, img_scale=(160, 128), size_divisor=32)
    assert img.shape == (3, 3, 128, 160) and meta['img_shape'] == (128, 160, 3) and meta['ori_shape'] == (96, 120, 3)
    multi = MultiLiveVideoPose(_model(3), meta, cameras=3, max_push=1, rescale=True)
    assert multi.push({0: img[0], 1: img[1], 2: img[2]}) == []
    got = multi.flush()
    assert [(c, i) for c, i, _ in got] == [(0, 0), (1, 0), (2, 0)]
    for c, _, (bboxes, labels, kpts) in got:
        n = bboxes.shape[0]
        assert n <= 12 and bboxes.shape == (n, 5) and labels.shape == (n,) and kpts.shape == (n, 15, 3)
        assert torch.isfinite(bboxes).all() and torch.isfinite(kpts).all()
        alone_img, alone_meta = preprocess_clip_nv12(surfaces[c][None], 120, img_scale=(160, 128), size_divisor=32)
        assert alone_meta == meta
        live = LiveVideoPose(_model(3), alone_meta, max_push=1, rescale=True)
        exp = live.push(alone_img[0]) + live.flush()
        assert [i for i, _ in exp] == [0]
        for x, y in zip((bboxes, labels, kpts), exp[0][1]):
            assert x.shape == y.shape and torch.equal(x, y), f'camera {c}'
