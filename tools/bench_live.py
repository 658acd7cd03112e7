"""Live video at full size (800x1344, R-50): latency of a `LiveVideoPose.push`, throughput of a live run against
`infer_video` on the same frames, the ring's resident bytes, and the NV12 ingest against the packed-BGR pipeline;
and the multi-camera leg: C = 2, 4, 8 cameras at max_push = 1 through one `MultiLiveVideoPose` against C
`LiveVideoPose` objects pushed in turn, the ingest of C surfaces in one launch against C launches, and the ring
write as one `ops.scatter_rows` launch against the `copy_` form.
python tools/bench_live.py [n_frames=56] [T=7] [legs=single,multi]"""
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pavenet_amd import ops  # noqa: E402
from pavenet_amd.live import LiveVideoPose, MultiLiveVideoPose  # noqa: E402
from pavenet_amd.models import build_model, videopose_r50_cfg  # noqa: E402
from pavenet_amd.preprocess import preprocess_clip, preprocess_clip_nv12, preprocess_surfaces_nv12  # noqa: E402
from pavenet_amd.streaming import VideoPoseStream  # noqa: E402
from pavenet_amd.weights import init_random_weights  # noqa: E402


def _live_run(live, video, step):
    """One video through push / flush -> (seconds per push, total seconds, results emitted)."""
    live.reset()
    per_push, emitted = [], 0
    torch.cuda.synchronize()
    t_all = time.perf_counter()
    for i in range(0, video.shape[0], step):
        t0 = time.perf_counter()
        emitted += len(live.push(video[i:i + step]))
        torch.cuda.synchronize()
        per_push.append(time.perf_counter() - t0)
    emitted += len(live.flush())
    torch.cuda.synchronize()
    return per_push, time.perf_counter() - t_all, emitted


def _time(fn, reps=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def single(m, meta, n, T):
    video = torch.randn(n, 3, 800, 1344, device='cuda')

    for max_push in (1, 4):
        live = LiveVideoPose(m, meta, max_push=max_push, decode_chunk=4)
        _live_run(live, video[:4 * T], max_push)             # warm-up: allocation, kernel selection
        per_push, total, emitted = _live_run(live, video, max_push)
        assert emitted == n
        steady = [t * 1e3 for t in per_push[T:]] or [t * 1e3 for t in per_push]   # (the first pushes emit less)
        print(f'live max_push={max_push}: push median {statistics.median(steady):.2f} ms, max {max(steady):.2f} ms '
              f'over {len(steady)} steady pushes; {n} frames in {total * 1e3:.1f} ms -> {n / total:.1f} frames/s; '
              f'ring {live.ring.n_slots} slots, {live.ring.resident_bytes()} bytes resident '
              f'({live.ring.resident_bytes() / 1e9:.2f} GB)')
        per_slot = live.ring.resident_bytes() // live.ring.n_slots
        del live

    stream = VideoPoseStream(m, meta, encode_chunk=8, decode_chunk=4)
    dt = _time(lambda: stream.infer_video(video), reps=2)
    print(f'infer_video (encode_chunk 8, decode_chunk 4): {n} frames in {dt * 1e3:.1f} ms -> {n / dt:.1f} frames/s; '
          f'its caches hold {n} frames = {n * per_slot / 1e9:.2f} GB')
    del stream, video
    torch.cuda.empty_cache()

    # ingest: 1080 x 1920 -> 800 x 1344 canvas (img_scale (1333, 800), size_divisor 32), Tn frames per launch
    Tn, H0, W0, pitch = 8, 1080, 1920, 2048
    surfaces = torch.randint(0, 256, (Tn, H0 * 3 // 2, pitch), dtype=torch.uint8, device='cuda')
    bgr = torch.randint(0, 256, (Tn, H0, W0, 3), dtype=torch.uint8, device='cuda')
    img, _ = preprocess_clip_nv12(surfaces, W0, size_divisor=32)
    t_nv12 = _time(lambda: preprocess_clip_nv12(surfaces, W0, size_divisor=32))
    t_bgr = _time(lambda: preprocess_clip(bgr, size_divisor=32))
    print(f'ingest {H0}x{W0} -> {tuple(img.shape[-2:])}, {Tn} frames per launch: NV12 (pitch {pitch}) '
          f'{t_nv12 / Tn * 1e6:.1f} us/frame, packed BGR uint8 {t_bgr / Tn * 1e6:.1f} us/frame')



def _pushes_ms(push, lo, hi):
    """Host-clock milliseconds of each of the pushes lo .. hi - 1, each ended by a device synchronise."""
    out = []
    for f in range(lo, hi):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        push(f)
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def multi(m, meta, n, T):
    """The multi-camera leg.  Both forms run in this process on the same frames, alternating in blocks of pushes,
    so that what else the host does falls on both alike."""
    block = 4
    for C in (2, 4, 8):
        videos = [torch.randn(n, 3, 800, 1344, device='cuda') for _ in range(min(C, 2))]   # cameras share two videos
        frames = [videos[c % 2] for c in range(C)]
        together = MultiLiveVideoPose(m, meta, cameras=C, max_push=1, decode_chunk=4)
        apart = [LiveVideoPose(m, meta, max_push=1, decode_chunk=4) for _ in range(C)]

        def push_together(f):
            return together.push({c: frames[c][f] for c in range(C)})

        def push_apart(f):
            return [live.push(frames[c][f]) for c, live in enumerate(apart)]
        warm = 2 * T
        for f in range(warm):                  # allocation, kernel selection, the first windows
            push_together(f)
            push_apart(f)
        t_together, t_apart = [], []
        for lo in range(warm, n, block):       # alternate: one block of pushes each
            t_together += _pushes_ms(push_together, lo, min(lo + block, n))
            t_apart += _pushes_ms(push_apart, lo, min(lo + block, n))
        a, b = statistics.median(t_together), statistics.median(t_apart)
        print(f'multi C={C}: one MultiLiveVideoPose push median {a:.2f} ms (min {min(t_together):.2f}, max '
              f'{max(t_together):.2f}) = {a / C:.2f} ms per camera; {C} LiveVideoPose pushed in turn median {b:.2f} ms '
              f'(min {min(t_apart):.2f}, max {max(t_apart):.2f}) = {b / C:.2f} ms per camera; ratio {a / b:.3f} over '
              f'{len(t_together)} pushes each; ring {together.ring.resident_bytes() / 1e9:.2f} GB against '
              f'{sum(x.ring.resident_bytes() for x in apart) / 1e9:.2f} GB')
        del together, apart, videos, frames
        torch.cuda.empty_cache()

    # ingest of C cameras' surfaces: one launch against C launches (1080 x 1920, pitch 2048, one allocation each)
    H0, W0, pitch = 1080, 1920, 2048
    for C in (2, 4, 8):
        surfaces = [torch.randint(0, 256, (H0 * 3 // 2, pitch), dtype=torch.uint8, device='cuda') for _ in range(C)]
        t_one = _time(lambda: preprocess_surfaces_nv12(surfaces, W0, size_divisor=32), reps=50)
        t_each = _time(lambda: [preprocess_clip_nv12(s[None], W0, size_divisor=32) for s in surfaces], reps=50)
        print(f'ingest C={C}: {C} surfaces in one launch {t_one * 1e6:.1f} us, in {C} launches {t_each * 1e6:.1f} us')

    # the ring write of one push: C frames into six [C * R, S, 256] tensors, S of the 800 x 1344 canvas
    S, R = sum((800 // s) * (1344 // s) for s in (8, 16, 32, 64)), T
    for C in (2, 4, 8):
        srcs = [torch.randn(C, S, 256, device='cuda') for _ in range(6)]
        dsts = [torch.empty(C * R, S, 256, device='cuda') for _ in range(6)]
        rows = [c * R + 3 for c in range(C)]

        def copies():
            for s, d in zip(srcs, dsts):
                for i, r in enumerate(rows):
                    d[r:r + 1].copy_(s[i:i + 1])
        t_scatter = _time(lambda: ops.scatter_rows(srcs, dsts, rows), reps=50)
        t_copy = _time(copies, reps=50)
        gb = 2 * 6 * C * S * 256 * 4 / 1e9
        print(f'ring write C={C}: scatter_rows (1 launch) {t_scatter * 1e6:.1f} us = {gb / t_scatter:.0f} GB/s read + '
              f'written; copy_ per tensor and camera ({6 * C} launches) {t_copy * 1e6:.1f} us')
        del srcs, dsts


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 56
    T = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    legs = (sys.argv[3] if len(sys.argv) > 3 else 'single,multi').split(',')
    torch.backends.cudnn.benchmark = True
    m = init_random_weights(build_model(videopose_r50_cfg(num_frames=T, max_per_img=20)), seed=0).cuda().eval()
    meta = dict(batch_input_shape=(800, 1344), img_shape=(800, 1344, 3), scale_factor=(1., 1., 1., 1.))
    if 'single' in legs:
        single(m, meta, n, T)
    if 'multi' in legs:
        multi(m, meta, n, T)


if __name__ == '__main__':
    main()
