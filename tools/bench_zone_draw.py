"""Drawing zones, lines and counts into one 1080p NV12 surface on the device (overlay.draw_zones_nv12): 4 zones (one
concave, together about half the picture) and 2 lines with stems and labels, HIP events around the call, warm-up,
median and min .. max.  Beside it, in the same run and taking turns with it call by call:
  (a) draw_poses_nv12 at 20 poses on the same surface;
  (b) a device-to-device copy of the surface: the floor of touching every byte.
And the host alternative, wall clock around all of it: the surface and counts() copied to the host, the numpy
reference of the rule (tests/zone_draw_ref.py), the surface copied back.
python tools/bench_zone_draw.py [reps=50] [out=profiles/zone_draw_bench.txt]"""
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pavenet_amd.overlay import ZONE_FONT, ZoneStyle, draw_zones_nv12  # noqa: E402
from pavenet_amd.render import PoseStyle, draw_poses_nv12  # noqa: E402
from pavenet_amd.zones import ZoneMonitor  # noqa: E402
from tools.bench_render import _poses  # noqa: E402

W, H, PITCH = 1920, 1080, 2048
ZONES = [[(40, 60), (900, 60), (900, 520), (40, 520)],
         [(1100, 40), (1880, 40), (1880, 800), (1600, 800), (1600, 400), (1340, 400), (1340, 800), (1100, 800)],    # a U
         [(60, 600), (500, 560), (620, 900), (300, 1060), (80, 980)],
         [(1360, 450), (1580, 450), (1580, 780), (1360, 780)]]                                   # in the U's notch
LINES = [((960, 1060), (960, 20)), ((100, 540), (1800, 560))]


def _timed(fns, reps):
    """Event-timed calls of every function of `fns`, taking turns, after three warm-up rounds -> one list of ms each."""
    for _ in range(3):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(reps):
        for fn, t in zip(fns, times):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            t.append(a.elapsed_time(b))
    return times


def _row(t):
    return f'{statistics.median(t):.3f} ({min(t):.3f} .. {max(t):.3f})'


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    out = sys.argv[2] if len(sys.argv) > 2 else None
    assert torch.cuda.is_available(), 'bench_zone_draw needs an MI355X'
    mon = ZoneMonitor(17)
    mon.set_zones(0, ZONES, LINES, dwell_frames=[0, 30, 0, 0])
    counts = mon.counts(0)
    counts['occupancy'][:4] = torch.tensor([3, 0, 12, 1], dtype=torch.int32)
    counts['crossed'][:2] = torch.tensor([[128, 97], [5, 41]], dtype=torch.int32)
    style, pose_style = ZoneStyle(), PoseStyle(17, thickness=4, radius=4, draw_boxes=True)
    surface = torch.randint(0, 256, (H * 3 // 2, PITCH), dtype=torch.uint8).cuda()
    copy, result = torch.empty_like(surface), _poses(20, 7)
    zones, poses, d2d = _timed([lambda: draw_zones_nv12(surface, W, mon, style=style),
                                lambda: draw_poses_nv12(surface, W, result, style=pose_style),
                                lambda: copy.copy_(surface)], reps)
    from tests import zone_draw_ref as RD
    pinned = torch.empty(surface.shape, dtype=torch.uint8).pin_memory()
    host = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pinned.copy_(surface)
        to = lambda d: {k: v.cpu().numpy() for k, v in d.items()}
        drawn = RD.draw_nv12(pinned.numpy(), W, to(mon.geometry(0)), to(mon.counts(0)), to(mon.state(0)), style, ZONE_FONT)
        surface.copy_(torch.from_numpy(drawn))
        torch.cuda.synchronize()
        host.append((time.perf_counter() - t0) * 1e3)
    inside = sum(float(RD.fill_mask(W, H, [(8 * x, 8 * y) for x, y in z]).mean()) for z in ZONES)
    lines = [f'draw_zones_nv12, one {W} x {H} NV12 surface (pitch {PITCH}, {H * 3 // 2 * PITCH / 1e6:.2f} MB), 4 zones (one '
             f'concave; their areas add up to {inside:.2f} of the picture), 2 lines, default ZoneStyle; median (min .. max) of '
             f'{reps} event-timed calls taking turns, ms',
             f'{torch.cuda.get_device_name(0)}',
             f'draw_zones_nv12                          {_row(zones)}',
             f'(a) draw_poses_nv12, N = 20, boxes on    {_row(poses)}',
             f'(b) device-to-device copy of the surface {_row(d2d)}',
             f'host alternative (surface and counts to the host, the numpy reference, surface back), wall clock of 3 runs: '
             f'{_row(host)}']
    text = '\n'.join(lines)
    print(text)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
