"""Track trails on the device (trails.TrackTrails.update, draw_trails_nv12): HIP events around the call, warm-up,
median and min .. max, the rows of a table taking turns call by call in one run.
  update: TrackTrails.update (length 32) at 20 and at 100 poses that walk, beside ZoneMonitor.update (4 zones, 2 lines)
    on the same frames;
  draw: draw_trails_nv12 on one 1920 x 1080 surface with 20 and with 100 tracks of 32 points, beside draw_poses_nv12 at
    the same pose counts and a device-to-device copy of the surface;
  the draw kernel's own time: HIP events around a batch of launches queued behind a sleeping stream, so that the device
    and not the host sets the pace (the row says so if the host was slower than the sleep);
  the host alternative, wall clock around all of it: the result and the ids copied to the host, the numpy reference
    of the update rule (tests/trail_ref.py); and the surface and the state copied to the host, the numpy reference of
    the draw rule (tests/trail_draw_ref.py), the surface copied back.
python tools/bench_trails.py [reps=50] [out=profiles/trails_bench.txt]"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pavenet_amd.render import PoseStyle, draw_poses_nv12  # noqa: E402
from pavenet_amd.trails import TrackTrails, TrailStyle, draw_trails_nv12  # noqa: E402
from pavenet_amd.zones import ZoneMonitor  # noqa: E402
from tools.bench_render import _poses  # noqa: E402
from tools.bench_zone_draw import H, LINES, PITCH, W, ZONES, _row, _timed  # noqa: E402

LENGTH, WALK = 32, 40


def _walk(n, seed):
    """WALK frames of n people who walk 6 px a frame, each in a direction of their own, and turn round half way."""
    start = _poses(n, seed)
    g = torch.Generator().manual_seed(seed + 1)
    angle = torch.rand(n, generator=g) * 6.2832
    step = (torch.stack([angle.cos(), angle.sin()], 1) * 6.0).cuda()
    frames = []
    for f in range(WALK):
        d = f if f < WALK // 2 else WALK - f
        kpts, bboxes = start['kpts'].clone(), start['bboxes'].clone()
        kpts[..., :2] += step[:, None] * d
        bboxes[:, :2] += step * d
        bboxes[:, 2:4] += step * d
        frames.append(dict(bboxes=bboxes, kpts=kpts, keep=start['keep']))
    return frames, torch.arange(1, n + 1, dtype=torch.int32).cuda()


def _kernel_ms(fn, batch):
    """ms per launch of `batch` launches of fn queued behind a sleeping stream, and whether the host kept ahead."""
    a, b, c = (torch.cuda.Event(enable_timing=True) for _ in range(3))
    fn()
    torch.cuda.synchronize()
    c.record()
    torch.cuda._sleep(200_000_000)
    a.record()
    t0 = time.perf_counter()
    for _ in range(batch):
        fn()
    host = (time.perf_counter() - t0) * 1e3
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / batch, host < c.elapsed_time(a)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    out = sys.argv[2] if len(sys.argv) > 2 else None
    assert torch.cuda.is_available(), 'bench_trails needs an MI355X'
    walks = {n: _walk(n, 7 + n) for n in (20, 100)}
    trails = {n: TrackTrails(17, length=LENGTH) for n in walks}
    mons = {n: ZoneMonitor(17) for n in walks}
    for mon in mons.values():
        mon.set_zones(0, ZONES, LINES, dwell_frames=[0, 30, 0, 0])
    turn = {(kind, n): 0 for kind in 'tz' for n in walks}

    def one(kind, n):
        frames, ids = walks[n]
        f = turn[kind, n] = (turn[kind, n] + 1) % WALK
        (trails if kind == 't' else mons)[n].update(frames[f], ids)
    upd = _timed([lambda: one('t', 20), lambda: one('z', 20), lambda: one('t', 100), lambda: one('z', 100)], reps)

    # trails as a busy floor leaves them: every track with a full ring
    shown = {n: TrackTrails(17, length=LENGTH) for n in walks}
    for n, (frames, ids) in walks.items():
        for f in range(WALK):
            shown[n].update(frames[f], ids)
    points = {n: int(shown[n].state(0)['count'].sum()) for n in walks}
    style, pstyle = TrailStyle(), PoseStyle(17, thickness=4, radius=4)
    surface = torch.randint(0, 256, (H * 3 // 2, PITCH), dtype=torch.uint8).cuda()
    copy = torch.empty_like(surface)
    draw = _timed([lambda: draw_trails_nv12(surface, W, shown[20], style=style),
                   lambda: draw_poses_nv12(surface, W, walks[20][0][-1], style=pstyle),
                   lambda: draw_trails_nv12(surface, W, shown[100], style=style),
                   lambda: draw_poses_nv12(surface, W, walks[100][0][-1], style=pstyle), lambda: copy.copy_(surface)], reps)
    kernel = {n: _kernel_ms(lambda: draw_trails_nv12(surface, W, shown[n], style=style), 200) for n in walks}

    from tests import trail_draw_ref as DR
    from tests import trail_ref as TR
    host_upd, host_draw = [], []
    ref = TR.TrailRef(17, length=LENGTH)
    pinned = torch.empty(surface.shape, dtype=torch.uint8).pin_memory()
    for i in range(3):
        res, ids = walks[100][0][i], walks[100][1]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ref.update(res['kpts'].cpu().numpy(), res['bboxes'].cpu().numpy(), ids.cpu().numpy(), res['keep'].cpu().numpy())
        host_upd.append((time.perf_counter() - t0) * 1e3)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pinned.copy_(surface)
        st = {k: v[0].cpu().numpy() for k, v in shown[100].device_tensors().items()}
        surface.copy_(torch.from_numpy(DR.draw_nv12(pinned.numpy(), W, st, style)))
        torch.cuda.synchronize()
        host_draw.append((time.perf_counter() - t0) * 1e3)

    def own(n):
        ms, ahead = kernel[n]
        return f'{ms:.4f}' + ('' if ahead else ' (the host did not keep ahead of the device: an upper bound)')
    lines = [f'TrackTrails, length {LENGTH}, {W} x {H}; median (min .. max) of {reps} event-timed calls taking turns, ms',
             f'{torch.cuda.get_device_name(0)}',
             f'TrackTrails.update, N = 20                 {_row(upd[0])}',
             f'ZoneMonitor.update, N = 20 (4 zones, 2 lines) {_row(upd[1])}',
             f'TrackTrails.update, N = 100                {_row(upd[2])}',
             f'ZoneMonitor.update, N = 100                {_row(upd[3])}',
             f'draw_trails_nv12, one {W} x {H} NV12 surface (pitch {PITCH}), default TrailStyle:',
             f'draw_trails_nv12, 20 tracks ({points[20]} points)    {_row(draw[0])}',
             f'draw_poses_nv12, 20 poses                  {_row(draw[1])}',
             f'draw_trails_nv12, 100 tracks ({points[100]} points)  {_row(draw[2])}',
             f'draw_poses_nv12, 100 poses                 {_row(draw[3])}',
             f'device-to-device copy of the surface       {_row(draw[4])}',
             f'the draw kernel alone, 200 launches behind a sleeping stream, ms per launch: 20 tracks {own(20)}; 100 tracks '
             f'{own(100)}',
             f'host alternative of update at N = 100 (result and ids to the host, the numpy reference), wall clock of 3 '
             f'runs: {_row(host_upd)}',
             f'host alternative of draw at 100 tracks (surface and state to the host, the numpy reference, surface back), '
             f'wall clock of 3 runs: {_row(host_draw)}']
    text = '\n'.join(lines)
    print(text)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
