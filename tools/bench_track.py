"""Track ids on the device (tracking.PoseTracker): microseconds per `update` at N = 20 and N = 100 poses with as many
live tracks, and per `update_many` of 8 cameras; HIP events, warm-up, medians.  Beside each, the host alternative
on the same frames: the results copied to the host (a synchronisation per frame), then the same rule in numpy
(tests/track_ref.py), wall clock.  K = 15, defaults; the people are seeded figures 100 px tall that walk 2 px per
frame, shuffled on every frame, so every frame is N matches.  Beside each device figure, from the same run and
on the same frames, the same call with motion='constant_velocity' (defaults): the kernel's MOTION = true form.
python tools/bench_track.py [reps=50] [out=profiles/track_bench.txt]"""
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pavenet_amd.tracking import PoseTracker  # noqa: E402
from tests import track_ref as TR  # noqa: E402

WARM = 3
# a standing figure in a box 0.4 wide and 1 high, PoseTrack order
FIGURE = np.asarray([(.20, .08), (.20, .14), (.20, .00), (.05, .20), (.35, .20), (.00, .36), (.40, .36), (.02, .50),
                     (.38, .50), (.10, .52), (.30, .52), (.09, .76), (.31, .76), (.08, 1.0), (.32, 1.0)])


def _frames(n, count, seed):
    """`count` frames of n walking people -> [(bboxes, labels, kpts)] on the device."""
    rng = np.random.default_rng(seed)
    pos = np.stack([30.0 + 60.0 * (np.arange(n) % 16), 20.0 + 120.0 * (np.arange(n) // 16)], 1)
    out = []
    for f in range(count):
        xy = FIGURE[None] * 100.0 + (pos + 2.0 * f)[:, None, :] + rng.uniform(-1, 1, (n, 15, 2))
        kpts = np.concatenate([xy, np.full((n, 15, 1), 0.9)], 2).astype(np.float32)
        bboxes = np.concatenate([pos + 2.0 * f, pos + 2.0 * f + (40.0, 100.0), np.full((n, 1), 0.8)], 1).astype(np.float32)
        order = rng.permutation(n)
        out.append((torch.from_numpy(bboxes[order]).cuda(), torch.zeros(n, dtype=torch.int64).cuda(),
                    torch.from_numpy(kpts[order]).cuda()))
    return out


def _stats(times):
    return statistics.median(times), min(times), max(times)


def _device_us(*legs):
    """legs: lists of one closure per frame; the first WARM of each are warm-up, the rest event-timed one by one,
    the legs taking turns frame by frame (what else the machine does then falls on all of them alike).  One
    (median, min, max) per leg."""
    for calls in legs:
        for fn in calls[:WARM]:
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in legs]
    for fns in zip(*(calls[WARM:] for calls in legs)):
        for out, fn in zip(times, fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            out.append(a.elapsed_time(b) * 1e3)
    return [_stats(t) for t in times]


def _host_us(calls):
    for fn in calls[:WARM]:
        fn()
    times = []
    for fn in calls[WARM:]:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e6)
    return _stats(times)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    out = sys.argv[2] if len(sys.argv) > 2 else None
    assert torch.cuda.is_available(), 'bench_track needs an MI355X'
    lines = [f'PoseTracker, K = 15, defaults (max_tracks 128); every frame links N poses to N live tracks; median '
             f'(min .. max) of {reps} calls, microseconds; device: HIP events around the call (its host part '
             f'included); motion: the same call of a tracker with motion=\'constant_velocity\' (gain 8, max_predict 30, '
             f'new_gate 4) on the same frames; host: copy to the host + tests/track_ref.py, wall clock',
             f'{torch.cuda.get_device_name(0)}']

    def host_update(ref, res, camera=0):
        return ref.update(res[2].cpu().numpy(), res[0].cpu().numpy(), camera=camera)
    for n in (20, 100):
        frames = _frames(n, reps + WARM, n)
        tracker, ref = PoseTracker(15), TR.TrackRef(15)
        moving = PoseTracker(15, motion='constant_velocity')
        d, m = _device_us([lambda r=r: tracker.update(r) for r in frames],
                          [lambda r=r: moving.update(r) for r in frames])
        h = _host_us([lambda r=r: host_update(ref, r) for r in frames])
        same = int(tracker.state(0)['next_id'].item()) == int(ref.next_id[0]) == n + 1 == \
            int(moving.state(0)['next_id'].item())
        lines.append(f'update, N = {n:3d}: device {d[0]:.1f} ({d[1]:.1f} .. {d[2]:.1f}); motion {m[0]:.1f} ({m[1]:.1f} .. '
                     f'{m[2]:.1f}) [{m[0] / d[0]:.3f} x]; host {h[0]:.1f} ({h[1]:.1f} .. '
                     f'{h[2]:.1f})  [{h[0] / d[0]:.1f} x; {n} ids on all three: {same}]')
        cams = [_frames(n, reps + WARM, 100 * n + c) for c in range(8)]
        tracker, ref = PoseTracker(15, cameras=8), TR.TrackRef(15, cameras=8)
        moving = PoseTracker(15, cameras=8, motion='constant_velocity')
        d, m = _device_us([lambda f=f: tracker.update_many([(c, cams[c][f]) for c in range(8)])
                           for f in range(reps + WARM)],
                          [lambda f=f: moving.update_many([(c, cams[c][f]) for c in range(8)])
                           for f in range(reps + WARM)])
        h = _host_us([lambda f=f: [host_update(ref, cams[c][f], c) for c in range(8)] for f in range(reps + WARM)])
        lines.append(f'update_many, 8 cameras x N = {n:3d}: device {d[0]:.1f} ({d[1]:.1f} .. {d[2]:.1f}); motion {m[0]:.1f} '
                     f'({m[1]:.1f} .. {m[2]:.1f}) [{m[0] / d[0]:.3f} x]; host {h[0]:.1f} '
                     f'({h[1]:.1f} .. {h[2]:.1f})  [{h[0] / d[0]:.1f} x]')
    text = '\n'.join(lines)
    print(text)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
