"""Hiding people in 1080p NV12 surfaces on the device (anonymize.anonymize_nv12): N = 20 and 100 poses, 1 and 8
surfaces, the 'head' and the 'person' region, both 'pixelate' at cell 16; HIP events, warm-up, medians; beside each
time two references on the same surfaces, in the same run:
  (a) a device-to-device copy of the surfaces: the floor of touching every byte (the call touches masked cells only);
  (b) the pinned device -> host -> device round trip of the surfaces: the least a host masker pays before it masks.
The poses are seeded K = 17 figures 400 px tall and 160 px wide spread over the picture, their five head key points
within 40 px at the top.  The share of the picture's cells each call masks is printed with its time (computed on the
host from the same poses by the rule's statement in tests/anon_ref.py).
python tools/bench_anonymize.py [reps=50] [out=profiles/anonymize_bench.txt]"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pavenet_amd.anonymize import PrivacyStyle, anonymize_nv12  # noqa: E402
from tests import anon_ref  # noqa: E402

W, H, PITCH = 1920, 1080, 2048


def _poses(n, seed):
    g = torch.Generator().manual_seed(seed)
    corner = torch.rand(n, 1, 2, generator=g) * torch.tensor([W - 160.0, H - 400.0])
    body = corner + torch.rand(n, 12, 2, generator=g) * torch.tensor([160.0, 340.0]) + torch.tensor([0.0, 60.0])
    head = corner + torch.tensor([60.0, 0.0]) + torch.rand(n, 5, 2, generator=g) * 40.0
    xy = torch.cat([head, body], 1)
    kpts = torch.cat([xy, torch.rand(n, 17, 1, generator=g) * 0.9 + 0.1], 2)
    bboxes = torch.cat([xy.min(1)[0], xy.max(1)[0], torch.full((n, 1), 0.9)], 1)
    return dict(bboxes=bboxes.cuda(), kpts=kpts.contiguous().cuda(), keep=torch.ones(n, dtype=torch.int32).cuda())


def _masked_share(results, style):
    """The share of the cells of the surfaces that the call masks."""
    masked = total = 0
    for r in results:
        regs = anon_ref.regions(r['kpts'].cpu().numpy(), r['bboxes'].cpu().numpy(), None, (1.0, 1.0), style)
        mask = anon_ref.cell_mask(W, H, style.cell, regs)
        masked, total = masked + int(mask.sum()), total + mask.size
    return masked / total


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
    assert torch.cuda.is_available(), 'bench_anonymize needs an MI355X'
    styles = [('head', PrivacyStyle(17, region='head', mode='pixelate', cell=16)),
              ('person', PrivacyStyle(17, region='person', mode='pixelate', cell=16))]
    lines = [f'anonymize_nv12, {W} x {H} NV12 (pitch {PITCH}, {H * 3 // 2 * PITCH / 1e6:.2f} MB per surface), K = 17, '
             f"'pixelate' at cell 16, the other defaults; median (min .. max) of {reps} event-timed calls, ms",
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
            for name, style in styles:
                t = _median_ms(lambda: anonymize_nv12(arg[0], W, arg[1], style=style), reps)
                verdict = f'{t[0] / b[0]:.2f} x SLOWER than (b)' if t[0] > b[0] else f'{b[0] / t[0]:.1f} x faster than (b)'
                lines.append(f'  N = {n:3d} poses per surface, {name:6s}: {t[0]:.3f} ({t[1]:.3f} .. {t[2]:.3f})  [{verdict}; '
                             f'{t[0] / a[0]:.2f} x (a); {100 * _masked_share(results, style):.1f} % of the cells masked]')
    lines.append('Kernel-only times: not measured (no trace run was taken); the times above include the host side of the '
                 'call.')
    text = '\n'.join(lines)
    print(text)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
