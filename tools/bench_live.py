"""Live video at full size (800x1344, R-50): latency of a `LiveVideoPose.push`, throughput of a live run against
`infer_video` on the same frames, the ring's resident bytes, and the NV12 ingest against the packed-BGR pipeline.
python tools/bench_live.py [n_frames=56] [T=7]"""
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pavenet_amd.live import LiveVideoPose  # noqa: E402
from pavenet_amd.models import build_model, videopose_r50_cfg  # noqa: E402
from pavenet_amd.preprocess import preprocess_clip, preprocess_clip_nv12  # noqa: E402
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


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 56
    T = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    torch.backends.cudnn.benchmark = True
    m = init_random_weights(build_model(videopose_r50_cfg(num_frames=T, max_per_img=20)), seed=0).cuda().eval()
    meta = dict(batch_input_shape=(800, 1344), img_shape=(800, 1344, 3), scale_factor=(1., 1., 1., 1.))
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


if __name__ == '__main__':
    main()
