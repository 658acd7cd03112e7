"""Steady poses on the device (smoothing.PoseSmoother): microseconds per `smooth` at N = 20 and N = 100 poses with as
many live slots, and per `smooth_many` of 8 cameras; HIP events, warm-up, medians.  Beside each, from the same run
and on the same frames, taking turns frame by frame: the tracker's `update` (`update_many`) that comes before it in
the loop, and the host alternative: the result and its ids copied to the host (a synchronisation per frame), then
the same rule in numpy (tests/smooth_ref.py), wall clock.  K = 15, defaults; the people are bench_track's seeded
figures 100 px tall that walk 2 px per frame, shuffled on every frame; the ids are the tracker's own, made before
the clock starts.
python tools/bench_smooth.py [reps=50] [out=profiles/smooth_bench.txt]"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pavenet_amd.smoothing import PoseSmoother  # noqa: E402
from pavenet_amd.tracking import PoseTracker  # noqa: E402
from tests import smooth_ref as SR  # noqa: E402
from tools.bench_track import WARM, _device_us, _frames, _host_us  # noqa: E402


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    out = sys.argv[2] if len(sys.argv) > 2 else None
    assert torch.cuda.is_available(), 'bench_smooth needs an MI355X'
    lines = [f'PoseSmoother, K = 15, defaults (max_tracks 128, alpha_min 32, beta 128, velocity_gain 3); every frame '
             f'filters N poses in N live slots; median (min .. max) of {reps} calls, microseconds; smooth: HIP events '
             f'around the call (its host part included); track: PoseTracker.update (defaults) on the same frames, the '
             f'same way, taking turns with it; host: result and ids copied to the host + tests/smooth_ref.py, wall clock',
             f'{torch.cuda.get_device_name(0)}']

    def host_smooth(ref, res, ids, camera=0):
        return ref.smooth(res[2].cpu().numpy(), res[0].cpu().numpy(), ids.cpu().numpy(), camera=camera)
    for n in (20, 100):
        frames = _frames(n, reps + WARM, n)
        ids = [t for t in PoseTracker(15).update_many([(0, r) for r in frames])]
        tracker, smoother, ref = PoseTracker(15), PoseSmoother(15), SR.SmoothRef(15)
        d, t = _device_us([lambda r=r, i=i: smoother.smooth(r, i) for r, i in zip(frames, ids)],
                          [lambda r=r: tracker.update(r) for r in frames])
        h = _host_us([lambda r=r, i=i: host_smooth(ref, r, i) for r, i in zip(frames, ids)])
        same = all(torch.equal(smoother.state(0)[name].cpu(), torch.from_numpy(ref.state(0)[name]))
                   for name in ('id', 'last', 'pos', 'vel')) and int((ref.id[0] != 0).sum()) == n
        lines.append(f'smooth, N = {n:3d}: smooth {d[0]:.1f} ({d[1]:.1f} .. {d[2]:.1f}); track {t[0]:.1f} ({t[1]:.1f} .. '
                     f'{t[2]:.1f}) [smooth / track {d[0] / t[0]:.3f}]; host {h[0]:.1f} ({h[1]:.1f} .. {h[2]:.1f})  '
                     f'[{h[0] / d[0]:.1f} x; {n} slots, device state == host state: {same}]')
        cams = [_frames(n, reps + WARM, 100 * n + c) for c in range(8)]
        cam_ids = [PoseTracker(15).update_many([(0, r) for r in cams[c]]) for c in range(8)]
        tracker, smoother, ref = PoseTracker(15, cameras=8), PoseSmoother(15, cameras=8), SR.SmoothRef(15, cameras=8)
        d, t = _device_us([lambda f=f: smoother.smooth_many([(c, cams[c][f], cam_ids[c][f]) for c in range(8)])
                           for f in range(reps + WARM)],
                          [lambda f=f: tracker.update_many([(c, cams[c][f]) for c in range(8)])
                           for f in range(reps + WARM)])
        h = _host_us([lambda f=f: [host_smooth(ref, cams[c][f], cam_ids[c][f], c) for c in range(8)]
                      for f in range(reps + WARM)])
        lines.append(f'smooth_many, 8 cameras x N = {n:3d}: smooth {d[0]:.1f} ({d[1]:.1f} .. {d[2]:.1f}); track {t[0]:.1f} '
                     f'({t[1]:.1f} .. {t[2]:.1f}) [smooth / track {d[0] / t[0]:.3f}]; host {h[0]:.1f} '
                     f'({h[1]:.1f} .. {h[2]:.1f})  [{h[0] / d[0]:.1f} x]')
    text = '\n'.join(lines)
    print(text)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
