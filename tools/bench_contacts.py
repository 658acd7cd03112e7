"""Contacts and groups on the device (contacts.ContactMonitor.update): HIP events around the call, warm-up, median and
min .. max, the rows of a table taking turns call by call in one run.
  update: ContactMonitor.update (128 slots, radius 1500, release 1800) at 20 and at 100 placed poses that walk under a
    tilted camera, beside the GroundPlane.update that placed them, on the same frames, and the ratio of the medians;
  the kernel's own time: HIP events around a batch of launches queued behind a sleeping stream, so that the device and
    not the host sets the pace (the row says so if the host was slower than the sleep, and the time is then an upper
    bound and not the kernel's);
  the host alternative, wall clock around all of it: on, xy and the ids copied to the host and the numpy reference of
    the rule (tests/contact_ref.py).
python tools/bench_contacts.py [reps=50] [out=profiles/contacts_bench.txt]"""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pavenet_amd.contacts import ContactMonitor  # noqa: E402
from pavenet_amd.floor import GroundPlane  # noqa: E402
from tools.bench_floor import _plane  # noqa: E402
from tools.bench_trails import WALK, _kernel_ms, _walk  # noqa: E402
from tools.bench_zone_draw import H, W, _row, _timed  # noqa: E402

KW = dict(radius=1500, release=1800, min_frames=3, long_frames=25)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    out = sys.argv[2] if len(sys.argv) > 2 else None
    assert torch.cuda.is_available(), 'bench_contacts needs an MI355X'
    walks = {n: _walk(n, 7 + n) for n in (20, 100)}
    planes = {n: GroundPlane(17, unit=50, origin=(-8000, 0)) for n in walks}
    mons = {n: ContactMonitor(**KW) for n in walks}
    for n in walks:
        planes[n].set_plane(0, matrix=_plane())
    placed = {n: [planes[n].update(frame, walks[n][1]) for frame in walks[n][0]] for n in walks}
    turn = {(kind, n): 0 for kind in 'fc' for n in walks}

    def one(kind, n):
        frames, ids = walks[n]
        f = turn[kind, n] = (turn[kind, n] + 1) % WALK
        return planes[n].update(frames[f], ids) if kind == 'f' else mons[n].update(placed[n][f], ids)
    upd = _timed([lambda: one('c', 20), lambda: one('f', 20), lambda: one('c', 100), lambda: one('f', 100)], reps)
    on = {n: int(placed[n][0]['on'].sum()) for n in walks}
    seen = {n: {k: int(v) for k, v in mons[n].counts(0).items()} for n in walks}
    kernel = {n: _kernel_ms(lambda: one('c', n), 200) for n in walks}

    from tests import contact_ref as CR
    host = []
    ref = CR.ContactRef(**KW)
    for i in range(3):
        p, ids = placed[100][i], walks[100][1]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ref.update(p['on'].cpu().numpy(), p['xy'].cpu().numpy(), ids.cpu().numpy())
        host.append((time.perf_counter() - t0) * 1e3)

    def own(n):
        ms, ahead = kernel[n]
        return f'{ms:.4f}' + ('' if ahead else ' (the host did not keep ahead of the device: an upper bound, the '
                                             "kernel's own time was not separated)")

    def median(v):
        return sorted(v)[len(v) // 2]
    lines = [f'ContactMonitor, 128 slots, {W} x {H}; median (min .. max) of {reps} event-timed calls taking turns, ms',
             f'{torch.cuda.get_device_name(0)}',
             f'ContactMonitor.update, N = 20 ({on[20]} placed)     {_row(upd[0])}',
             f'GroundPlane.update, N = 20                     {_row(upd[1])}',
             f'ContactMonitor.update, N = 100 ({on[100]} placed)   {_row(upd[2])}',
             f'GroundPlane.update, N = 100                    {_row(upd[3])}',
             f'ContactMonitor.update / GroundPlane.update, medians of this run: N = 20 {median(upd[0]) / median(upd[1]):.2f}, '
             f'N = 100 {median(upd[2]) / median(upd[3]):.2f}',
             f'the counters after the timed calls: N = 20 {seen[20]}; N = 100 {seen[100]}',
             f'the kernel alone (an update launches nothing else), 200 calls queued behind a sleeping stream, ms per launch: N = 20 '
             f'{own(20)}; N = 100 {own(100)}',
             f'host alternative of update at N = 100 (on, xy and ids to the host, the numpy reference), wall clock of 3 '
             f'runs: {_row(host)}']
    text = '\n'.join(lines)
    print(text)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
