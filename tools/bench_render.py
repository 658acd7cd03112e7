"""Drawing poses into 1080p NV12 surfaces on the device (render.draw_poses_nv12): N = 20 and 100 poses, 1 and 8
surfaces, HIP events, warm-up, medians; beside each draw time two references on the same surfaces:
  (a) a device-to-device copy of the surfaces: the floor of touching every byte (the draw writes covered bytes only);
  (b) the pinned device -> host -> device round trip of the surfaces: the least a host renderer pays before it draws.
The poses are seeded figures of ~400 px spread over the picture, thickness = radius = 4, boxes on.  Beside every
plain draw, in the same run, the draw with track ids (pose p has id p + 1: a colour per id and a label at
label_scale 2 on every pose), on the same surfaces and poses.
python tools/bench_render.py [reps=50] [out=profiles/render_bench.txt]"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pavenet_amd.render import PoseStyle, TrackStyle, draw_poses_nv12  # noqa: E402

W, H, PITCH = 1920, 1080, 2048


def _poses(n, seed):
    g = torch.Generator().manual_seed(seed)
    centre = torch.rand(n, 1, 2, generator=g) * torch.tensor([W - 400.0, H - 400.0]) + 200.0
    kpts = torch.cat([centre + (torch.rand(n, 17, 2, generator=g) - 0.5) * 400.0, torch.rand(n, 17, 1, generator=g)], 2)
    lo, hi = kpts[..., :2].min(1)[0], kpts[..., :2].max(1)[0]
    bboxes = torch.cat([lo, hi, torch.full((n, 1), 0.9)], 1)
    return dict(bboxes=bboxes.cuda(), kpts=kpts.contiguous().cuda(), keep=torch.ones(n, dtype=torch.int32).cuda())


def _median_ms(fn, reps):
    """Median of `reps` event-timed calls after three warm-up calls."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times), min(times), max(times)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    out = sys.argv[2] if len(sys.argv) > 2 else None
    assert torch.cuda.is_available(), 'bench_render needs an MI355X'
    style = PoseStyle(17, thickness=4, radius=4, draw_boxes=True)
    track_style = TrackStyle(17, thickness=4, radius=4, draw_boxes=True, label_scale=2)
    lines = [f'draw_poses_nv12, {W} x {H} NV12 (pitch {PITCH}, {H * 3 // 2 * PITCH / 1e6:.2f} MB per surface), K = 17, '
             f'thickness = radius = 4, boxes on; median (min .. max) of {reps} event-timed calls, ms',
             f'{torch.cuda.get_device_name(0)}']
    for n_surf in (1, 8):
        surfaces = [torch.randint(0, 256, (H * 3 // 2, PITCH), dtype=torch.uint8).cuda() for _ in range(n_surf)]
        copies = [torch.empty_like(s) for s in surfaces]
        pinned = [torch.empty(s.shape, dtype=torch.uint8).pin_memory() for s in surfaces]

        def d2d():
            for s, c in zip(surfaces, copies):
                c.copy_(s)

        def round_trip():
            for s, p in zip(surfaces, pinned):
                p.copy_(s, non_blocking=True)
            for s, p in zip(surfaces, pinned):
                s.copy_(p, non_blocking=True)
        a, b = _median_ms(d2d, reps), _median_ms(round_trip, reps)
        lines.append(f'{n_surf} surface(s): (a) device-to-device copy {a[0]:.3f} ({a[1]:.3f} .. {a[2]:.3f}); '
                     f'(b) pinned D2H + H2D round trip {b[0]:.3f} ({b[1]:.3f} .. {b[2]:.3f})')
        for n in (20, 100):
            results = [_poses(n, 1000 * n_surf + i) for i in range(n_surf)]
            arg = (surfaces[0], results[0]) if n_surf == 1 else (surfaces, results)
            t = _median_ms(lambda: draw_poses_nv12(arg[0], W, arg[1], style=style), reps)
            verdict = 'slower than (b)' if t[0] > b[0] else f'{b[0] / t[0]:.1f} x faster than (b)'
            lines.append(f'  N = {n:3d} poses per surface: draw {t[0]:.3f} ({t[1]:.3f} .. {t[2]:.3f})  [{verdict}; '
                         f'{t[0] / a[0]:.2f} x (a)]')
            ids = [torch.arange(1, n + 1, dtype=torch.int32).cuda() for _ in range(n_surf)]
            ids = ids[0] if n_surf == 1 else ids
            u = _median_ms(lambda: draw_poses_nv12(arg[0], W, arg[1], style=track_style, ids=ids), reps)
            lines.append(f'                            with ids and labels (g = 2) {u[0]:.3f} ({u[1]:.3f} .. {u[2]:.3f})  '
                         f'[{u[0] / t[0]:.2f} x the plain draw]')
    text = '\n'.join(lines)
    print(text)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
