"""Footfall maps on the device (heatmap.FootfallMap.update, draw_heat_nv12): HIP events around the call, warm-up,
median and min .. max, the rows of a table taking turns call by call in one run.
  update: FootfallMap.update (1920 x 1080, cell 8, radius 1) at 20 and at 100 poses, beside ZoneMonitor.update (4 zones,
    2 lines) on the same frames;
  draw: draw_heat_nv12 on one 1920 x 1080 surface over a map with about a third of its cells warm, smooth on and off,
    beside draw_zones_nv12 and a device-to-device copy of the surface;
  the host alternative, wall clock around all of it: the result and the ids copied to the host, the numpy reference
    of the update rule (tests/heat_ref.py); and the surface and the map copied to the host, the numpy reference of the
    draw rule (tests/heat_draw_ref.py), the surface copied back.
python tools/bench_heat.py [reps=50] [out=profiles/heat_bench.txt]"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pavenet_amd.heatmap import FootfallMap, HeatStyle, draw_heat_nv12  # noqa: E402
from pavenet_amd.overlay import ZoneStyle, draw_zones_nv12  # noqa: E402
from pavenet_amd.zones import ZoneMonitor  # noqa: E402
from tools.bench_render import _poses  # noqa: E402
from tools.bench_zone_draw import H, LINES, PITCH, W, ZONES, _row, _timed  # noqa: E402


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    out = sys.argv[2] if len(sys.argv) > 2 else None
    assert torch.cuda.is_available(), 'bench_heat needs an MI355X'
    frames = {n: (_poses(n, 7 + n), torch.arange(1, n + 1, dtype=torch.int32).cuda()) for n in (20, 100)}
    fmaps = {n: FootfallMap(17, size=(W, H)) for n in frames}
    mons = {n: ZoneMonitor(17) for n in frames}
    for mon in mons.values():
        mon.set_zones(0, ZONES, LINES, dwell_frames=[0, 30, 0, 0])
    upd = _timed([lambda: fmaps[20].update(*frames[20]), lambda: mons[20].update(*frames[20]),
                  lambda: fmaps[100].update(*frames[100]), lambda: mons[100].update(*frames[100])], reps)

    # a map as a busy floor leaves it: blobs over about a third of the cells
    shown = FootfallMap(17, size=(W, H))
    shown.update(*frames[20])
    rng = np.random.default_rng(5)
    yy, xx = np.mgrid[0:shown.Gh, 0:shown.Gw]
    warm = sum(np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2.0 * s * s)) * a
               for cx, cy, s, a in zip(rng.uniform(0, shown.Gw, 14), rng.uniform(0, shown.Gh, 14), rng.uniform(6, 22, 14),
                                       rng.uniform(200, 4000, 14)))
    warm = np.where(warm > 150, warm, 0).astype(np.int32)
    shown.maps(0)['dwell'].copy_(torch.from_numpy(warm))
    shown.maps(0)['peak'][0] = int(warm.max())
    mon = mons[20]
    smooth, blocky, zstyle = HeatStyle(smooth=True), HeatStyle(smooth=False), ZoneStyle()
    surface = torch.randint(0, 256, (H * 3 // 2, PITCH), dtype=torch.uint8).cuda()
    copy = torch.empty_like(surface)
    draw = _timed([lambda: draw_heat_nv12(surface, W, shown, style=smooth),
                   lambda: draw_heat_nv12(surface, W, shown, style=blocky),
                   lambda: draw_zones_nv12(surface, W, mon, style=zstyle), lambda: copy.copy_(surface)], reps)

    from tests import heat_draw_ref as DR
    from tests import heat_ref as HR
    host_upd, host_draw = [], []
    ref = HR.HeatRef(17, size=(W, H))
    pinned = torch.empty(surface.shape, dtype=torch.uint8).pin_memory()
    for _ in range(3):
        res, ids = frames[100]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ref.update(res['kpts'].cpu().numpy(), res['bboxes'].cpu().numpy(), ids.cpu().numpy(), res['keep'].cpu().numpy())
        host_upd.append((time.perf_counter() - t0) * 1e3)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pinned.copy_(surface)
        maps = {k: v.cpu().numpy() for k, v in shown.maps(0).items()}
        surface.copy_(torch.from_numpy(DR.draw_nv12(pinned.numpy(), W, maps, shown.size, shown.cell, smooth)))
        torch.cuda.synchronize()
        host_draw.append((time.perf_counter() - t0) * 1e3)
    lines = [f'FootfallMap, {W} x {H}, cell 8 ({shown.Gw} x {shown.Gh} cells), radius 1; median (min .. max) of {reps} '
             f'event-timed calls taking turns, ms',
             f'{torch.cuda.get_device_name(0)}',
             f'FootfallMap.update, N = 20                 {_row(upd[0])}',
             f'ZoneMonitor.update, N = 20 (4 zones, 2 lines) {_row(upd[1])}',
             f'FootfallMap.update, N = 100                {_row(upd[2])}',
             f'ZoneMonitor.update, N = 100                {_row(upd[3])}',
             f'draw_heat_nv12, one {W} x {H} NV12 surface (pitch {PITCH}), {float((warm > 0).mean()):.2f} of the cells warm, '
             f'default HeatStyle:',
             f'draw_heat_nv12, smooth                     {_row(draw[0])}',
             f'draw_heat_nv12, smooth=False               {_row(draw[1])}',
             f'draw_zones_nv12 (4 zones, 2 lines)         {_row(draw[2])}',
             f'device-to-device copy of the surface       {_row(draw[3])}',
             f'host alternative of update at N = 100 (result and ids to the host, the numpy reference), wall clock of 3 '
             f'runs: {_row(host_upd)}',
             f'host alternative of draw (surface and map to the host, the numpy reference, surface back), wall clock of 3 '
             f'runs: {_row(host_draw)}']
    text = '\n'.join(lines)
    print(text)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
