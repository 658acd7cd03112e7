"""Zones and counting lines on the device (zones.ZoneMonitor): microseconds per `update` at N = 20 and N = 100 poses
with as many live slots, and per `update_many` of 8 cameras; HIP events, warm-up, medians.  Beside each, from the same
run and on the same frames, taking turns frame by frame: `PoseSmoother.smooth` (`smooth_many`), the other per-track
stage of the loop, and the host alternative: the result and its ids copied to the host (a synchronisation per
frame), then the same rule in numpy and Python (tests/zones_ref.py), wall clock.  K = 15, defaults, 4 zones (one
concave) and 2 lines over the walkers' paths; the people are bench_track's seeded figures 100 px tall that walk 2 px
per frame, shuffled on every frame; the ids are the tracker's own, made before the clock starts.  At the end the
device state and counters are compared with the oracle's.
python tools/bench_zones.py [reps=50] [out=profiles/zones_bench.txt]"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pavenet_amd.smoothing import PoseSmoother  # noqa: E402
from pavenet_amd.tracking import PoseTracker  # noqa: E402
from pavenet_amd.zones import ZoneMonitor  # noqa: E402
from tests import zones_ref as ZR  # noqa: E402
from tools.bench_track import WARM, _device_us, _frames, _host_us  # noqa: E402

ZONES = [[(0, 0), (520, 0), (520, 480), (0, 480)], [(520, 0), (1200, 0), (1200, 480), (520, 480)],
         [(0, 480), (1200, 480), (1200, 1100), (0, 1100)],
         [(100, 100), (900, 100), (900, 800), (700, 800), (700, 300), (300, 300), (300, 800), (100, 800)]]
LINES = [((520, 1100), (520, 0)), ((0, 480), (1200, 480))]
STATE = ('id', 'last', 'pos', 'inside', 'alerted', 'streak', 'since', 'frame', 'dropped')


def _same(monitor, ref, camera):
    views = dict(monitor.state(camera), **monitor.counts(camera))
    exp = dict(ref.state(camera), **ref.counts(camera))
    return all(torch.equal(views[n].cpu(), torch.from_numpy(np.array(exp[n])))
               for n in STATE + ZR.COUNTERS + ('crossed',))


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    out = sys.argv[2] if len(sys.argv) > 2 else None
    assert torch.cuda.is_available(), 'bench_zones needs an MI355X'
    lines = [f'ZoneMonitor, K = 15, defaults (max_tracks 128, anchor feet, min_frames 2, max_events 256), 4 zones (one '
             f'concave) and 2 lines; every frame has N poses in N live slots; median (min .. max) of {reps} calls, '
             f'microseconds; zones: HIP events around the call (its host part included); smooth: PoseSmoother.smooth '
             f'(defaults) on the same frames, the same way, taking turns with it; host: result and ids copied to the host '
             f'+ tests/zones_ref.py, wall clock',
             f'{torch.cuda.get_device_name(0)}']

    def host_update(ref, res, ids, camera=0):
        return ref.update(res[2].cpu().numpy(), res[0].cpu().numpy(), ids.cpu().numpy(), camera=camera)
    for n in (20, 100):
        frames = _frames(n, reps + WARM, n)
        ids = [t for t in PoseTracker(15).update_many([(0, r) for r in frames])]
        monitor, smoother, ref = ZoneMonitor(15), PoseSmoother(15), ZR.ZoneRef(15)
        monitor.set_zones(0, ZONES, LINES, dwell_frames=[10, 0, 20, 0])
        ref.set_zones(0, ZONES, LINES, dwell_frames=[10, 0, 20, 0])
        d, s = _device_us([lambda r=r, i=i: monitor.update(r, i) for r, i in zip(frames, ids)],
                          [lambda r=r, i=i: smoother.smooth(r, i) for r, i in zip(frames, ids)])
        h = _host_us([lambda r=r, i=i: host_update(ref, r, i) for r, i in zip(frames, ids)])
        same = _same(monitor, ref, 0) and int((ref.id[0] != 0).sum()) == n
        events = int(sum(int(ref.counts(0)[k].sum()) for k in ('entered', 'exited', 'appeared', 'vanished', 'crossed')))
        lines.append(f'update, N = {n:3d}: zones {d[0]:.1f} ({d[1]:.1f} .. {d[2]:.1f}); smooth {s[0]:.1f} ({s[1]:.1f} .. '
                     f'{s[2]:.1f}) [zones / smooth {d[0] / s[0]:.3f}]; host {h[0]:.1f} ({h[1]:.1f} .. {h[2]:.1f})  '
                     f'[{h[0] / d[0]:.1f} x; {n} slots, {events} counted events, device state and counters == host: {same}]')
        cams = [_frames(n, reps + WARM, 100 * n + c) for c in range(8)]
        cam_ids = [PoseTracker(15).update_many([(0, r) for r in cams[c]]) for c in range(8)]
        monitor, smoother, ref = ZoneMonitor(15, cameras=8), PoseSmoother(15, cameras=8), ZR.ZoneRef(15, cameras=8)
        for c in range(8):
            monitor.set_zones(c, ZONES, LINES, dwell_frames=[10, 0, 20, 0])
            ref.set_zones(c, ZONES, LINES, dwell_frames=[10, 0, 20, 0])
        d, s = _device_us([lambda f=f: monitor.update_many([(c, cams[c][f], cam_ids[c][f]) for c in range(8)])
                           for f in range(reps + WARM)],
                          [lambda f=f: smoother.smooth_many([(c, cams[c][f], cam_ids[c][f]) for c in range(8)])
                           for f in range(reps + WARM)])
        h = _host_us([lambda f=f: [host_update(ref, cams[c][f], cam_ids[c][f], c) for c in range(8)]
                      for f in range(reps + WARM)])
        same = all(_same(monitor, ref, c) for c in range(8))
        lines.append(f'update_many, 8 cameras x N = {n:3d}: zones {d[0]:.1f} ({d[1]:.1f} .. {d[2]:.1f}); smooth {s[0]:.1f} '
                     f'({s[1]:.1f} .. {s[2]:.1f}) [zones / smooth {d[0] / s[0]:.3f}]; host {h[0]:.1f} '
                     f'({h[1]:.1f} .. {h[2]:.1f})  [{h[0] / d[0]:.1f} x; device state and counters == host: {same}]')
    text = '\n'.join(lines)
    print(text)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
