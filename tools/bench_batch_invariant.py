"""Cost of batch-invariant inference (bricks.set_batch_invariant): mode off and on, interleaved in one process, for
the configs[2] step (R-50, T = 7 x 4 clips, 800 x 1344), a one-clip step of the same model and streaming windows/s.
   python tools/bench_batch_invariant.py [reps=5] [stream_frames=14]"""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pavenet_amd.bricks import set_batch_invariant  # noqa: E402
from pavenet_amd.models import build_model, videopose_r50_cfg  # noqa: E402
from pavenet_amd.streaming import VideoPoseStream  # noqa: E402
from pavenet_amd.weights import init_random_weights  # noqa: E402


def _time(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    nf = int(sys.argv[2]) if len(sys.argv) > 2 else 14
    T = 7
    m = init_random_weights(build_model(videopose_r50_cfg(num_frames=T, max_per_img=20)), seed=0).cuda().eval()
    meta = dict(batch_input_shape=(800, 1344), img_shape=(800, 1344, 3), scale_factor=(1., 1., 1., 1.))
    g = torch.Generator(device='cuda').manual_seed(4321)
    img = torch.randn(4, T, 3, 800, 1344, device='cuda', generator=g)
    video = img[:2].reshape(2 * T, 3, 800, 1344)[:nf].contiguous()
    stream = VideoPoseStream(m, meta, encode_chunk=14, decode_chunk=14)
    work = [('configs[2] step (T=7 x 4 clips)', lambda: m.forward_device(img, [meta] * 4), 1),
            ('one-clip step (T=7 x 1 clip)', lambda: m.forward_device(img[:1], [meta]), 1),
            (f'streaming ({nf} frames = {nf} windows)', lambda: stream.infer_video(video), nf)]
    res = {name: {False: [], True: []} for name, _, _ in work}
    with torch.no_grad():
        for _ in range(3):                         # rounds of off / on, interleaved
            for flag in (False, True):
                set_batch_invariant(m, flag)
                for name, fn, _ in work:
                    res[name][flag].append(_time(fn, reps))
        set_batch_invariant(m, False)
    print('workload | mode off | mode on | on / off   (best of 3 interleaved rounds, ms per call; streaming: windows/s)')
    for name, _, per in work:
        off, on = min(res[name][False]), min(res[name][True])
        if per > 1:
            print(f'{name} | {per / off:.1f} win/s | {per / on:.1f} win/s | {off / on:.3f}x throughput')
        else:
            print(f'{name} | {off * 1e3:.1f} ms | {on * 1e3:.1f} ms | {on / off:.3f}')


if __name__ == '__main__':
    main()
