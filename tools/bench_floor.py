"""The ground plane on the device (floor.GroundPlane.update): HIP events around the call, warm-up, median and min ..
max, the rows of a table taking turns call by call in one run.
  update: GroundPlane.update at 20 and at 100 poses that walk under a tilted camera, beside ZoneMonitor.update (4
    zones, 2 lines) on the same frames, and the ratio of the two medians;
  the kernel's own time: HIP events around a batch of launches queued behind a sleeping stream, so that the device and
    not the host sets the pace (the row says so if the host was slower than the sleep, and the time is then an upper
    bound and not the kernel's);
  the host alternative, wall clock around all of it: the result and the ids copied to the host and the numpy reference
    of the rule (tests/floor_ref.py).
python tools/bench_floor.py [reps=50] [out=profiles/floor_bench.txt]"""
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pavenet_amd.floor import GroundPlane  # noqa: E402
from pavenet_amd.zones import ZoneMonitor  # noqa: E402
from tools.bench_trails import WALK, _kernel_ms, _walk  # noqa: E402
from tools.bench_zone_draw import H, LINES, W, ZONES, _row, _timed  # noqa: E402


def _plane(tilt=55.0, height=3000.0, focal=1400.0):
    """pixels -> mm of a pinhole `height` mm above the floor that looks `tilt` degrees off the plumb line at the W x H
    picture: the horizon is 540 - 1400 tan(35 degrees) rows above the picture's top."""
    s, c = math.sin(math.radians(tilt)), math.cos(math.radians(tilt))
    R = np.asarray([[1.0, 0.0, 0.0], [0.0, -c, -s], [0.0, s, -c]])
    K = np.asarray([[focal, 0.0, W / 2], [0.0, focal, H / 2], [0.0, 0.0, 1.0]])
    M = np.linalg.inv(K @ np.stack([R[:, 0], R[:, 1], -R @ np.asarray([0.0, 0.0, height])], 1))
    return M if M[2, 2] > 0 else -M


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    out = sys.argv[2] if len(sys.argv) > 2 else None
    assert torch.cuda.is_available(), 'bench_floor needs an MI355X'
    walks = {n: _walk(n, 7 + n) for n in (20, 100)}
    planes = {n: GroundPlane(17, unit=50, origin=(-8000, 0)) for n in walks}
    mons = {n: ZoneMonitor(17) for n in walks}
    for n in walks:
        planes[n].set_plane(0, matrix=_plane())
        mons[n].set_zones(0, ZONES, LINES, dwell_frames=[0, 30, 0, 0])
    turn = {(kind, n): 0 for kind in 'fz' for n in walks}

    def one(kind, n):
        frames, ids = walks[n]
        f = turn[kind, n] = (turn[kind, n] + 1) % WALK
        return (planes if kind == 'f' else mons)[n].update(frames[f], ids)
    upd = _timed([lambda: one('f', 20), lambda: one('z', 20), lambda: one('f', 100), lambda: one('z', 100)], reps)
    placed = {n: int(one('f', n)['on'].sum()) for n in walks}
    kernel = {n: _kernel_ms(lambda: one('f', n), 200) for n in walks}

    from tests import floor_ref as FR
    host = []
    ref = FR.FloorRef(17, unit=50, origin=(-8000, 0))
    ref.set_plane(0, matrix=_plane())
    for i in range(3):
        res, ids = walks[100][0][i], walks[100][1]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ref.update(res['kpts'].cpu().numpy(), res['bboxes'].cpu().numpy(), ids.cpu().numpy(), res['keep'].cpu().numpy())
        host.append((time.perf_counter() - t0) * 1e3)

    def own(n):
        ms, ahead = kernel[n]
        return f'{ms:.4f}' + ('' if ahead else ' (the host did not keep ahead of the device: an upper bound, the '
                                             "kernel's own time was not separated)")

    def median(v):
        return sorted(v)[len(v) // 2]
    lines = [f'GroundPlane, {W} x {H}; median (min .. max) of {reps} event-timed calls taking turns, ms',
             f'{torch.cuda.get_device_name(0)}',
             f'GroundPlane.update, N = 20 ({placed[20]} placed)      {_row(upd[0])}',
             f'ZoneMonitor.update, N = 20 (4 zones, 2 lines) {_row(upd[1])}',
             f'GroundPlane.update, N = 100 ({placed[100]} placed)    {_row(upd[2])}',
             f'ZoneMonitor.update, N = 100                {_row(upd[3])}',
             f'GroundPlane.update / ZoneMonitor.update, medians of this run: N = 20 {median(upd[0]) / median(upd[1]):.2f}, '
             f'N = 100 {median(upd[2]) / median(upd[3]):.2f}',
             f'the kernel alone (an update launches nothing else), 200 calls queued behind a sleeping stream, ms per launch: N = 20 '
             f'{own(20)}; N = 100 {own(100)}',
             f'host alternative of update at N = 100 (result and ids to the host, the numpy reference), wall clock of 3 '
             f'runs: {_row(host)}']
    text = '\n'.join(lines)
    print(text)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
