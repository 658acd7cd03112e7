"""Re-identification on the device (reid.PersonReID): microseconds per `update_nv12` on a 1080p NV12 surface at
N = 20 and N = 100 poses; HIP events, warm-up, medians.  Beside each, from the same run and on the same frames, taking
turns frame by frame: `PoseTracker.update`, the stage before it, and the host alternative: the surface, the result and
its ids copied to the host (a synchronisation per frame), then the same rule in numpy and Python (tests/reid_ref.py),
wall clock.  K = 15, defaults; the people are bench_track's seeded figures 100 px tall that walk 2 px per frame,
shuffled on every frame, over a surface of noise; the ids are the tracker's own, made before the clock starts.  A second
row per N gives every pose a new track id in every frame, the longest path of the link kernel (N x N pair scores, N
greedy rounds).  At the end the gallery on the device is compared with the oracle's.
python tools/bench_reid.py [reps=50] [out=profiles/reid_bench.txt]"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pavenet_amd import reid  # noqa: E402
from pavenet_amd.tracking import PoseTracker  # noqa: E402
from tests import reid_cases as RC  # noqa: E402
from tests import reid_ref as RR  # noqa: E402
from tools.bench_track import WARM, _device_us, _frames, _host_us  # noqa: E402

W, H = 1920, 1080
STATE = ('person', 'track', 'last', 'hits', 'hist', 'frame', 'next', 'dropped')


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    out = sys.argv[2] if len(sys.argv) > 2 else None
    assert torch.cuda.is_available(), 'bench_reid needs an MI355X'
    lines = [f'PersonReID.update_nv12, K = 15, defaults (max_people 128, match_thr {reid.DEFAULT_MATCH_THR}), one {W} x {H} '
             f'NV12 surface at pitch 2048; median (min .. max) of {reps} calls, microseconds; reid: HIP events around the '
             f'call (its host part included, two launches); track: PoseTracker.update (defaults) on the same frames, the '
             f'same way, taking turns with it; host: surface, result and ids copied to the host + tests/reid_ref.py, wall '
             f'clock', f'{torch.cuda.get_device_name(0)}']
    host_surface = RC.noise_nv12(H, W, 2048, 1)
    surface = torch.from_numpy(host_surface).cuda()
    for n in (20, 100):
        frames = _frames(n, reps + WARM, n)
        ids = [t for t in PoseTracker(15).update_many([(0, r) for r in frames])]
        gallery, tracker = reid.PersonReID(15), PoseTracker(15)
        ref = RR.ReIDRef(15, default_thr=reid.DEFAULT_MATCH_THR)

        def host_update(r, i):
            return ref.update('nv12', surface.cpu().numpy(), W, r[2].cpu().numpy(), r[0].cpu().numpy(), i.cpu().numpy())
        d, t = _device_us([lambda r=r, i=i: gallery.update_nv12(surface, W, r, i) for r, i in zip(frames, ids)],
                          [lambda r=r: tracker.update(r) for r in frames])
        h = _host_us([lambda r=r, i=i: host_update(r, i) for r, i in zip(frames, ids)])
        same = all(torch.equal(gallery.state(0)[k].cpu(), torch.from_numpy(np.array(ref.state(0)[k]))) for k in STATE)
        lines.append(f'update_nv12, N = {n:3d}: reid {d[0]:.1f} ({d[1]:.1f} .. {d[2]:.1f}); track {t[0]:.1f} ({t[1]:.1f} .. '
                     f'{t[2]:.1f}) [reid / track {d[0] / t[0]:.3f}]; host {h[0]:.1f} ({h[1]:.1f} .. {h[2]:.1f})  '
                     f'[{h[0] / d[0]:.1f} x; {int((ref.person[0] != 0).sum())} people, gallery on the device == host: {same}]')
        # the longest path: every track id is new in every frame, so all N poses are scored against all N slots and
        # taken back one greedy round each
        fresh = [torch.where(i > 0, i + 1000 * (f + 1), i) for f, i in enumerate(ids)]
        gallery, tracker = reid.PersonReID(15, min_hits=1), PoseTracker(15)
        ref = RR.ReIDRef(15, default_thr=reid.DEFAULT_MATCH_THR, min_hits=1)
        d, t = _device_us([lambda r=r, i=i: gallery.update_nv12(surface, W, r, i) for r, i in zip(frames, fresh)],
                          [lambda r=r: tracker.update(r) for r in frames])
        host = host_surface
        sims = 0
        for r, i in zip(frames, fresh):
            sims += int((ref.update('nv12', host, W, r[2].cpu().numpy(), r[0].cpu().numpy(), i.cpu().numpy())['sim'] > 0).sum())
        same = all(torch.equal(gallery.state(0)[k].cpu(), torch.from_numpy(np.array(ref.state(0)[k]))) for k in STATE)
        lines.append(f'update_nv12, N = {n:3d}, every track id new in every frame: reid {d[0]:.1f} ({d[1]:.1f} .. {d[2]:.1f}); '
                     f'track {t[0]:.1f} [reid / track {d[0] / t[0]:.3f}]  [{sims} poses re-identified in {len(frames)} '
                     f'frames, {int(ref.next[0]) - 1} person ids, gallery on the device == host: {same}]')
    text = '\n'.join(lines)
    print(text)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
