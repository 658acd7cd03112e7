"""Postures and falls on the device (posture.PostureMonitor): microseconds per `update` at N = 20 and N = 100 poses
with as many live slots; HIP events, warm-up, medians.  Beside it, from the same run and on the same frames, taking
turns frame by frame: `ZoneMonitor.update` (bench_zones' 4 zones and 2 lines), the other per-track monitor of the
loop, and the host alternative: the result and its ids copied to the host (a synchronisation per frame), then the same
rule in numpy and Python (tests/posture_ref.py), wall clock.  K = 15, defaults; the people are bench_track's figure 100
px tall with a jitter of 1 px, shuffled on every frame, under ids 1 .. N; person d raises the hands in frames 5 .. 9
and turns to the floor over 8 frames from frame 10 + d % 20 on, so the frames carry every kind of event.  At the end
the device state and counters are compared with the oracle's.
python tools/bench_posture.py [reps=50] [out=profiles/posture_bench.txt]"""
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pavenet_amd.posture import PostureMonitor  # noqa: E402
from pavenet_amd.zones import ZoneMonitor  # noqa: E402
from tests import posture_ref as PR  # noqa: E402
from tools.bench_track import FIGURE, WARM, _device_us, _host_us  # noqa: E402
from tools.bench_zones import LINES, ZONES  # noqa: E402


def _turned(fig, degrees):
    a = math.radians(degrees)
    rot = np.asarray([[math.cos(a), -math.sin(a)], [math.sin(a), math.cos(a)]])
    return (fig - (.20, 1.0)) @ rot.T + (.20, 1.0)


def _frames(n, count, seed):
    """`count` frames of n people -> [((bboxes, labels, kpts), ids)] on the device."""
    rng = np.random.default_rng(seed)
    pos = np.stack([130.0 + 60.0 * (np.arange(n) % 16), 20.0 + 120.0 * (np.arange(n) // 16)], 1)
    raised = FIGURE.copy()
    raised[[7, 8], 1] = .05
    out = []
    for f in range(count):
        xy = np.empty((n, 15, 2))
        for d in range(n):
            turn = min(max(f - (10 + d % 20), 0), 8) / 8.0 * (90.0 if d % 2 else -90.0)
            xy[d] = _turned(raised if 5 <= f < 10 else FIGURE, turn) * 100.0 + pos[d]
        xy += rng.uniform(-1, 1, xy.shape)
        kpts = np.concatenate([xy, np.full((n, 15, 1), 0.9)], 2).astype(np.float32)
        bboxes = np.concatenate([xy.min(1), xy.max(1), np.full((n, 1), 0.8)], 1).astype(np.float32)
        order = rng.permutation(n)
        out.append(((torch.from_numpy(bboxes[order]).cuda(), torch.zeros(n, dtype=torch.int64).cuda(),
                     torch.from_numpy(kpts[order]).cuda()), torch.from_numpy((order + 1).astype(np.int32)).cuda()))
    return out


def _same(monitor, ref, camera):
    views = dict(monitor.state(camera), **monitor.counts(camera))
    exp = dict(ref.state(camera), **ref.counts(camera))
    return all(torch.equal(views[n].cpu(), torch.from_numpy(np.array(exp[n]))) for n in PR.STATE + PR.COUNTERS)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    out = sys.argv[2] if len(sys.argv) > 2 else None
    assert torch.cuda.is_available(), 'bench_posture needs an MI355X'
    lines = [f'PostureMonitor, K = 15, defaults (max_tracks 128, min_frames 3, lean 11, flat 11, squat 18, hand_up 4, '
             f'fall_window 30, down_frames 75, max_events 256); every frame has N poses in N live slots; median (min .. '
             f'max) of {reps} calls, microseconds; posture: HIP events around the call (its host part included); zones: '
             f'ZoneMonitor.update (defaults, 4 zones and 2 lines) on the same frames, the same way, taking turns with it; '
             f'host: result and ids copied to the host + tests/posture_ref.py, wall clock',
             f'{torch.cuda.get_device_name(0)}']

    def host_update(ref, res, ids):
        return ref.update(res[2].cpu().numpy(), res[0].cpu().numpy(), ids.cpu().numpy())
    for n in (20, 100):
        frames = _frames(n, reps + WARM, n)
        monitor, zones, ref = PostureMonitor(15), ZoneMonitor(15), PR.PostureRef(15)
        zones.set_zones(0, ZONES, LINES, dwell_frames=[10, 0, 20, 0])
        d, z = _device_us([lambda r=r, i=i: monitor.update(r, i) for r, i in frames],
                          [lambda r=r, i=i: zones.update(r, i) for r, i in frames])
        h = _host_us([lambda r=r, i=i: host_update(ref, r, i) for r, i in frames])
        same = _same(monitor, ref, 0) and int((ref.id[0] != 0).sum()) == n
        lines.append(f'update, N = {n:3d}: posture {d[0]:.1f} ({d[1]:.1f} .. {d[2]:.1f}); zones {z[0]:.1f} ({z[1]:.1f} .. '
                     f'{z[2]:.1f}) [posture / zones {d[0] / z[0]:.3f}]; host {h[0]:.1f} ({h[1]:.1f} .. {h[2]:.1f})  '
                     f'[{h[0] / d[0]:.1f} x; {n} slots, now {ref.now[0].tolist()}, {int(ref.falls[0])} falls, '
                     f'{int(ref.downs[0])} downs, device state and counters == host: {same}]')
    text = '\n'.join(lines)
    print(text)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
