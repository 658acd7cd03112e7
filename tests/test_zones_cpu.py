"""Zones and counting lines, the parts that need no GPU: the edges of the rule of DESIGN section 17 as hand-worked
scripts on its numpy statement (tests/zones_cases.py on tests/zones_ref.py), what the rule gives on jittering walkers,
the plan's C layout, and every refusal of the C entry point and of the Python wrappers."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import zones_cases as ZC
from tests import zones_ref as ZR
from tests.test_track_cpu import walk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class OracleHarness:
    """tests/zones_cases.py's harness on the oracle alone."""

    def __init__(self, K, **kw):
        self.ref = ZR.ZoneRef(K, **kw)

    def set_zones(self, zones, lines, dwell_frames=None, camera=0):
        self.ref.set_zones(camera, zones, lines, dwell_frames)

    def frame(self, kpts, bboxes, ids, keep=None, camera=0):
        out = self.ref.update(kpts, bboxes, np.asarray(ids, np.int64).astype(np.int32),
                              None if keep is None else np.asarray(keep, np.int32), camera=camera)
        ZC.invariant(self.ref.state(camera), self.ref.counts(camera))
        return out

    def poke(self, field, index, value, camera=0):
        getattr(self.ref, field)[(camera,) + tuple(index)] = value

    def get(self, field, camera=0):
        return getattr(self.ref, field)[camera]


@pytest.mark.parametrize('script', ZC.SCRIPTS, ids=lambda s: s.__name__)
def test_hand_worked_scripts_on_the_oracle(script):
    script(OracleHarness)


PEOPLE = 6
ZONE_DEPTH = 150.0       # px a walker's zone extends past its line; every walk ends at most 144 px past it


def passages(height, step, min_frames, frames=None):
    """The walk of tests/test_track_cpu.py (1 % jitter on every coordinate, so at most 1 % of the height on the mean
    of the ankles) with person p under id p + 1.  Person p starts with the feet at x = 100 + 400 p + 0.2 height and
    walks `step` px per frame for D = step * frames px; line p stands upright at the middle of that walk, from y =
    2000 to y = 0 (its ends far from the feet, at y < 400; a walk to the right crosses it forward), and zone p is the
    150 px behind it.  D / 2 <= 144, so nobody reaches a zone's far side or another walker's geometry.  -> (the
    oracle, the ENTER + EXIT events, the crossings of either direction)."""
    frames = frames or (60 if step < 8 else 36)
    half = step * frames / 2.0
    ref = ZR.ZoneRef(15, min_frames=min_frames)
    mid = [100.0 + 400.0 * p + 0.2 * height + half for p in range(PEOPLE)]
    ref.set_zones(0, [[(m, 0), (m + ZONE_DEPTH, 0), (m + ZONE_DEPTH, 2000), (m, 2000)] for m in mid],
                  [((m, 2000), (m, 0)) for m in mid])
    assert half >= 10 * 0.01 * height and half <= 144
    flips = crossings = 0
    for kpts, bboxes, who in walk(height, step, frames=frames, people=PEOPLE, seed=int(height * 10 + step)):
        out = ref.update(kpts, bboxes, who + 1)
        ZC.invariant(ref.state(0), ref.counts(0))
        kinds = out['events'][:int(out['n_events']), 0]
        assert int(out['n_events']) <= ref.max_events
        flips += int(np.isin(kinds, (ZR.ENTER, ZR.EXIT)).sum())
        crossings += int(np.isin(kinds, (ZR.CROSS_FWD, ZR.CROSS_BACK)).sum())
        assert not np.isin(kinds, (ZR.APPEAR, ZR.VANISH, ZR.DWELL)).any()
    assert ref.dropped[0] == 0 and (ref.id[0] != 0).sum() == PEOPLE
    return ref, flips, crossings


@pytest.mark.parametrize('height', [40, 100, 300])
@pytest.mark.parametrize('step', [1, 2, 4, 8])
def test_walkers_are_counted_once(height, step):
    """What follows from the rule, whatever the jitter does on the way: a walker who starts on one side of a long
    line and ends on the other has a net count of 1 on it and 0 on every other line; a walker who has been deeper
    inside a zone than the jitter for min_frames frames is inside; a longer debounce never flips more often (a flip
    under min_frames 3 needs a change of the raw test since the flip before it, and every such change is a flip
    under min_frames 1)."""
    flips = {}
    for min_frames in (1, 2, 3):
        ref, flips[min_frames], crossings = passages(height, step, min_frames)
        net = ref.crossed[0, :, 0].astype(np.int64) - ref.crossed[0, :, 1]
        assert net.tolist() == [1] * PEOPLE + [0, 0]
        assert ref.occupancy[0].tolist() == [1] * PEOPLE + [0, 0]
        assert (ref.entered[0] - ref.exited[0]).tolist() == [1] * PEOPLE + [0, 0]
        print(f'height {height} step {step} min_frames {min_frames}: ENTER + EXIT per passage '
              f'{flips[min_frames] / PEOPLE:.2f}, crossings per passage {crossings / PEOPLE:.2f}')
    assert flips[3] <= flips[1]


def test_a_slow_walker_in_heavy_jitter_is_still_counted_once():
    """300 px tall at a quarter of a pixel per frame for 240 frames: the jitter (up to 3 px) is twelve times the step,
    so the raw test flickers for many frames around the line.  The same three properties hold; the debounce is what
    keeps the ENTER / EXIT events few (DESIGN section 17 has the figures this prints)."""
    flips = {}
    for min_frames in (1, 2, 3):
        ref, flips[min_frames], crossings = passages(300, 0.25, min_frames, frames=240)
        assert (ref.crossed[0, :, 0].astype(np.int64) - ref.crossed[0, :, 1]).tolist() == [1] * PEOPLE + [0, 0]
        assert ref.occupancy[0].tolist() == [1] * PEOPLE + [0, 0]
        print(f'height 300 step 0.25 min_frames {min_frames}: ENTER + EXIT per passage {flips[min_frames] / PEOPLE:.2f}, '
              f'crossings per passage {crossings / PEOPLE:.2f}')
    assert flips[3] <= flips[1]


def test_defaults_ranges_and_geometry():
    import pavenet_amd
    from pavenet_amd import zones
    from pavenet_amd.zones import ZoneMonitor
    assert pavenet_amd.ZoneMonitor is ZoneMonitor
    m = ZoneMonitor(15)
    assert (m.K, m.cameras, m.max_tracks, m.max_age, m.anchor, m.anchor_kpts, m.min_frames, m.max_events, m.score_thr,
            m.kpt_thr) == (15, 1, 128, 30, 'feet', (13, 14), 2, 256, 0.3, 0.0)
    r = ZR.ZoneRef(15)
    assert (r.S, r.max_age, r.anchor, r.anchor_kpts, r.min_frames, r.max_events, float(r.score_thr), float(r.kpt_thr)) == \
        (128, 30, 'feet', (13, 14), 2, 256, float(np.float32(0.3)), 0.0)
    assert ZoneMonitor(17).anchor_kpts == (15, 16) and ZoneMonitor(14).anchor_kpts == (10, 11)
    assert ZoneMonitor(5, anchor='box').anchor_kpts == () and ZoneMonitor(5, anchor_kpts=[4, 0, 1, 2]).anchor_kpts == (4, 0, 1, 2)
    assert (zones.ENTER, zones.EXIT, zones.DWELL, zones.APPEAR, zones.VANISH, zones.CROSS_FWD, zones.CROSS_BACK) == \
        (ZR.ENTER, ZR.EXIT, ZR.DWELL, ZR.APPEAR, ZR.VANISH, ZR.CROSS_FWD, ZR.CROSS_BACK) == (1, 2, 3, 4, 5, 6, 7)
    for kw in (dict(min_frames=1), dict(min_frames=255), dict(max_events=1), dict(max_events=4096), dict(max_tracks=1),
               dict(max_age=0), dict(cameras=4096), dict(anchor='centre'), dict(anchor_kpts=())):
        ZoneMonitor(15, **kw)
    for call, needle in ((lambda: ZoneMonitor(0), 'K is'),
                         (lambda: ZoneMonitor(33), 'K is'),
                         (lambda: ZoneMonitor(15, cameras=0), 'cameras'),
                         (lambda: ZoneMonitor(15, cameras=4097), 'cameras'),
                         (lambda: ZoneMonitor(15, max_tracks=0), 'max_tracks'),
                         (lambda: ZoneMonitor(15, max_tracks=129), 'max_tracks'),
                         (lambda: ZoneMonitor(15, max_age=-1), 'max_age'),
                         (lambda: ZoneMonitor(15, max_age=1.5), 'max_age'),
                         (lambda: ZoneMonitor(15, min_frames=0), 'min_frames'),
                         (lambda: ZoneMonitor(15, min_frames=256), 'min_frames'),
                         (lambda: ZoneMonitor(15, min_frames=2.0), 'min_frames'),
                         (lambda: ZoneMonitor(15, max_events=0), 'max_events'),
                         (lambda: ZoneMonitor(15, max_events=4097), 'max_events'),
                         (lambda: ZoneMonitor(15, max_events=True), 'max_events'),
                         (lambda: ZoneMonitor(15, anchor='head'), 'anchor is'),
                         (lambda: ZoneMonitor(16), 'needs anchor_kpts'),
                         (lambda: ZoneMonitor(15, anchor_kpts=(0, 1, 2, 3, 4)), 'at most 4'),
                         (lambda: ZoneMonitor(15, anchor_kpts=(15,)), 'anchor_kpts are'),
                         (lambda: ZoneMonitor(15, anchor_kpts=(-1,)), 'anchor_kpts are'),
                         (lambda: ZoneMonitor(15, anchor='box', anchor_kpts=(15,)), 'anchor_kpts are'),
                         (lambda: ZoneMonitor(15, anchor_kpts=(1.0,)), 'anchor_kpts are')):
        with pytest.raises(ValueError, match=needle):
            call()
    # the quantisation of set_zones: rint(8 x) in double, half to even
    tri = [(0, 0), (8191, 0.0625), (10.1875, 8191)]
    row = zones.quantise_geometry([tri, tri[::-1]], [((1, 2), (1.07, 2))], [0, 1 << 30])
    G = zones._G
    assert len(row) == G['WORDS'] == 306 and row[:2] == [2, 1] and row[G['NVERT']:G['NVERT'] + 3] == [3, 3, 0]
    assert row[G['DWELL']:G['DWELL'] + 2] == [0, 1 << 30]
    assert row[G['ZONES']:G['ZONES'] + 6] == [0, 0, 65528, 0, 82, 65528] and row[G['ZONES'] + 32:G['ZONES'] + 34] == [82, 65528]
    assert row[G['LINES']:G['LINES'] + 5] == [8, 16, 9, 16, 0]
    ref = ZR.ZoneRef(1)
    ref.set_zones(0, [tri, tri[::-1]], [((1, 2), (1.07, 2))], [0, 1 << 30])
    assert ref.zones[0, 0, :3].reshape(-1).tolist() == row[G['ZONES']:G['ZONES'] + 6]
    assert ref.lines[0, 0].reshape(-1).tolist() == [8, 16, 9, 16] and ref.dwell_frames[0, 1] == 1 << 30


def test_set_zones_refusals():
    """Every refusal of set_zones is raised by the host quantisation, before a device is looked for."""
    from pavenet_amd.zones import ZoneMonitor
    m = ZoneMonitor(15, cameras=2)
    sq = [(0, 0), (10, 0), (10, 10), (0, 10)]
    line = ((0, 0), (10, 10))
    for call, needle in (
            (lambda: m.set_zones(2, [sq]), 'camera'),
            (lambda: m.set_zones(0.5, [sq]), 'camera'),
            (lambda: m.set_zones(0, [sq[:2]]), 'zone 0 has 2 vertices'),
            (lambda: m.set_zones(0, [sq, [(i, i * i) for i in range(17)]]), 'zone 1 has 17 vertices'),
            (lambda: m.set_zones(0, [sq] * 9), 'at most 8 zones'),
            (lambda: m.set_zones(0, [], [line] * 9), 'at most 8 lines'),
            (lambda: m.set_zones(0, [[(0, 0), (10, float('nan')), (5, 5)]]), 'vertex 1 of zone 0'),
            (lambda: m.set_zones(0, [[(0, 0), (float('inf'), 0), (5, 5)]]), 'finite'),
            (lambda: m.set_zones(0, [[(0, 0), (-0.5, 0), (5, 5)]]), '0 .. 8191'),
            (lambda: m.set_zones(0, [[(0, 0), (8191.5, 0), (5, 5)]]), '0 .. 8191'),
            (lambda: m.set_zones(0, [[(0, 0), (1, 2, 3), (5, 5)]]), 'pair'),
            (lambda: m.set_zones(0, [], [((0, 0), (0, 8192))]), 'end B of line 0'),
            (lambda: m.set_zones(0, [], [((5, 5), (5.05, 5))]), 'one point'),
            (lambda: m.set_zones(0, [], [((5, 5),)]), 'line 0 is'),
            (lambda: m.set_zones(0, [sq], [], dwell_frames=[1, 2]), 'one integer per zone'),
            (lambda: m.set_zones(0, [sq], [], dwell_frames=[-1]), 'dwell_frames'),
            (lambda: m.set_zones(0, [sq], [], dwell_frames=[(1 << 30) + 1]), 'dwell_frames'),
            (lambda: m.set_zones(0, [sq], [], dwell_frames=[1.5]), 'dwell_frames')):
        with pytest.raises(ValueError, match=needle):
            call()
    assert m._state is None and m.state(0) is None and m.counts(1) is None and m.geometry(0) is None


def _lib():
    from pavenet_amd import native
    from pavenet_amd.build_native import build_native
    build_native()
    return native, native.load()


def test_zone_plan_layout_and_entry(tmp_path):
    """native.ZonePlan is the header's pave_zone_plan field for field, under the 4 KB kernel-argument limit, and the
    entry is in the header, the binding and both libraries at ABI 21."""
    native, lib = _lib()
    vp, ci = ctypes.c_void_p, ctypes.c_int
    assert native.FUNCTIONS['pave_zone_events'] == (ci, [vp, vp]) and 'pave_zone_events' in native.SIGNATURES
    assert hasattr(lib, 'pave_zone_events')
    for path in (native.LIB_PATH, native.DIAG_LIB_PATH):
        out = subprocess.run(['nm', '-D', '--defined-only', path], capture_output=True, text=True, check=True).stdout
        assert 'pave_zone_events' in {ln.split()[-1] for ln in out.splitlines()}
    assert native.ABI_VERSION == 21 and lib.pave_abi_version() == 21
    assert ctypes.sizeof(native.ZonePlan) == 2712 < 4096
    if not shutil.which('gcc'):
        pytest.skip('no gcc')
    fields = [f for f, _ in native.ZonePlan._fields_]
    src = tmp_path / 'layout.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pave_hip.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(pave_zone_plan));\n'
                   + ''.join(f'  printf(" %zu", offsetof(pave_zone_plan, {f}));\n' for f in fields)
                   + '  return 0;\n}\n')
    exe = tmp_path / 'layout'
    subprocess.run(['gcc', '-std=c99', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == ctypes.sizeof(native.ZonePlan) < 4096
    assert got[1:] == [getattr(native.ZonePlan, f).offset for f in fields]


STATE_FIELDS = ('slot_id', 'slot_last', 'slot_pos', 'slot_inside', 'slot_alerted', 'slot_streak', 'slot_since', 'frame',
                'dropped', 'counters')


def test_c_entry_refuses_bad_plans_before_any_device_call():
    """No GPU: every refusal is PAVE_E_ARG with a message (the addresses are never dereferenced)."""
    native, lib = _lib()
    host = (ctypes.c_ubyte * 64)()
    addr = ctypes.addressof(host)

    def plan(entries=2, n=3, K=15, S=8, cameras=2, camera=1, scale=(1.0, 1.0), max_age=30, min_frames=2, max_events=256,
             anchor=0, anchor_kpts=(13, 14), kpts=addr, bboxes=addr, ids=addr, keep=None, out_zones=addr,
             out_dwell=addr, out_events=addr, out_n_events=addr, geometry=addr, **state):
        p = native.ZonePlan()
        for i in range(min(max(entries, 0), 32)):
            p.kpts[i], p.bboxes[i], p.ids[i], p.keep[i] = kpts, bboxes, ids, keep
            p.out_zones[i], p.out_dwell[i], p.out_events[i], p.out_n_events[i] = out_zones, out_dwell, out_events, \
                out_n_events
            p.n[i], p.camera[i], p.scale[i][0], p.scale[i][1] = n, camera, scale[0], scale[1]
        for f in STATE_FIELDS:
            setattr(p, f, state.get(f, addr))
        p.geometry = geometry
        for i, k in enumerate(anchor_kpts[:4]):
            p.anchor_kpt[i] = k
        p.entries, p.cameras, p.S, p.K, p.max_age = entries, cameras, S, K, max_age
        p.anchor, p.n_anchor, p.min_frames, p.max_events = anchor, len(anchor_kpts), min_frames, max_events
        p.score_thr, p.kpt_thr = 0.3, 0.0
        return p

    def refused(p, needle):
        assert lib.pave_zone_events(ctypes.byref(p) if p is not None else None, None) == native.DEFINES['PAVE_E_ARG'] == -1
        assert needle in lib.pave_last_error().decode(), lib.pave_last_error()

    refused(None, 'null plan')
    refused(plan(entries=0), 'frames per launch')
    refused(plan(entries=33), 'frames per launch')
    refused(plan(kpts=None), 'null pose')
    refused(plan(bboxes=None), 'null pose')
    refused(plan(ids=None), 'null ids')
    refused(plan(out_zones=None), 'null output')
    refused(plan(out_dwell=None), 'null output')
    refused(plan(out_events=None), 'null events')
    refused(plan(out_n_events=None), 'null events')
    refused(plan(n=0, out_events=None), 'null events')
    for f in STATE_FIELDS:
        refused(plan(**{f: None}), 'null state')
    refused(plan(geometry=None), 'null geometry')
    refused(plan(n=-1), 'N outside')
    refused(plan(n=129), 'N outside')
    refused(plan(K=0), 'K outside')
    refused(plan(K=33), 'K outside')
    refused(plan(S=0), 'max_tracks')
    refused(plan(S=129), 'max_tracks')
    refused(plan(cameras=0), 'cameras outside')
    refused(plan(cameras=4097), 'cameras outside')
    refused(plan(camera=-1), 'camera index')
    refused(plan(camera=2), 'camera index')
    for bad in ((0.0, 1.0), (1.0, -1.0), (float('nan'), 1.0), (1.0, float('inf'))):
        refused(plan(scale=bad), 'scale')
    refused(plan(max_age=-1), 'max_age')
    refused(plan(min_frames=0), 'min_frames')
    refused(plan(min_frames=256), 'min_frames')
    refused(plan(max_events=0), 'max_events')
    refused(plan(max_events=4097), 'max_events')
    refused(plan(anchor=-1), 'anchor outside')
    refused(plan(anchor=3), 'anchor outside')
    refused(plan(anchor_kpts=(0, 1, 2, 3, 4)), 'n_anchor')
    p = plan()
    p.n_anchor = -1
    refused(p, 'n_anchor')
    refused(plan(anchor_kpts=(13, 15)), 'anchor key point')
    refused(plan(anchor_kpts=(-1,)), 'anchor key point')
    refused(plan(K=14), 'anchor key point')


def test_wrappers_raise_value_errors_on_host_tensors():
    """Shape, type and range checks, and the host-tensor check itself, are ValueErrors raised before anything is
    allocated on or asked of a device."""
    from pavenet_amd import native, ops, zones
    from pavenet_amd.zones import ZoneMonitor
    kp, bb, keep = torch.zeros(3, 15, 3), torch.zeros(3, 5), torch.ones(3, dtype=torch.int32)
    ids = torch.ones(3, dtype=torch.int32)
    res = (bb, None, kp)
    mon = ZoneMonitor(15, cameras=2)
    for call, needle in (
            (lambda: mon.update((bb, kp), ids), 'tuple'),
            (lambda: mon.update(dict(bboxes=bb), ids), 'bboxes and kpts'),
            (lambda: mon.update((bb.numpy(), None, kp), ids), 'tensor'),
            (lambda: mon.update((bb[:2], None, kp), ids), 'bboxes'),
            (lambda: mon.update((bb.double(), None, kp), ids), 'float32'),
            (lambda: mon.update(dict(bboxes=bb, kpts=kp, keep=keep.long()), ids), 'int32'),
            (lambda: mon.update((torch.zeros(129, 5), None, torch.zeros(129, 15, 3)), torch.zeros(129, dtype=torch.int32)),
             'at most 128'),
            (lambda: mon.update((bb, None, torch.zeros(3, 17, 3)), ids), 'K = 17'),
            (lambda: mon.update(res, ids.long()), 'ids of results'),
            (lambda: mon.update(res, ids[:2]), 'ids of results'),
            (lambda: mon.update(res, [1, 2, 3]), 'ids of results'),
            (lambda: mon.update(res, ids, camera=2), 'camera'),
            (lambda: mon.update(res, ids, camera=0.5), 'camera'),
            (lambda: mon.update(res, ids, scale_factor=0.0), 'positive'),
            (lambda: mon.update(res, ids, scale_factor=(1.0, float('nan'))), 'positive'),
            (lambda: mon.update_many([(0, res, ids), (1, res, ids)], scale_factor=[1.0, 1.0, 1.0]), 'scale_factor'),
            (lambda: mon.update_many([(0, res)]), 'triples'),
            (lambda: mon.update(res, ids), 'HIP device'),
            (lambda: mon.reset(camera=2), 'camera'),
            (lambda: mon.counts(2), 'camera'),
            (lambda: mon.geometry(-1), 'camera'),
            (lambda: mon.state(2), 'camera')):
        with pytest.raises(ValueError, match=needle):
            call()
    assert mon._state is None and mon.state(0) is None and mon.update_many([]) == []
    mon.reset()
    table = torch.tensor([[zones.APPEAR, 1, 7, 0, 3], [zones.VANISH, 0, 9, -1, 3], [0, 0, 0, 0, 0]], dtype=torch.int32)
    two = [dict(kind='appear', index=1, id=7, pose=0, frame=3), dict(kind='vanish', index=0, id=9, pose=-1, frame=3)]
    assert zones.events_to_list(dict(events=table, n_events=torch.tensor(2, dtype=torch.int32))) == two
    assert zones.events_to_list(dict(events=table[:2], n_events=torch.tensor(5, dtype=torch.int32))) == two   # 3 not stored
    assert zones.events_to_list(dict(events=table, n_events=torch.tensor(0, dtype=torch.int32))) == []

    def state(cameras=2, S=8, **over):
        z = dict(dtype=torch.int32)
        s = dict(id=torch.zeros(cameras, S, **z), last=torch.zeros(cameras, S, **z), pos=torch.zeros(cameras, S, 2, **z),
                 inside=torch.zeros(cameras, S, **z), alerted=torch.zeros(cameras, S, **z),
                 streak=torch.zeros(cameras, S, 8, **z), since=torch.zeros(cameras, S, 8, **z),
                 frame=torch.zeros(cameras, **z), dropped=torch.zeros(cameras, **z),
                 counters=torch.zeros(cameras, native.ZONE_COUNTER_WORDS, **z),
                 geometry=torch.zeros(cameras, native.ZONE_GEOM_WORDS, **z))
        s.update(over)
        return s

    def events(entries=((kp, bb, None, ids, 0, (1.0, 1.0)),), st=None, K=15, **kw):
        return ops.zone_events(entries, state() if st is None else st, K=K, **kw)
    for call, needle in (
            (lambda: events(st=dict(id=bb)), 'state holds'),
            (lambda: events(st=state(pos=torch.zeros(2, 8, 3, dtype=torch.int32))), 'state pos'),
            (lambda: events(st=state(S=129)), 'S in'),
            (lambda: events(K=33), 'K'),
            (lambda: events(K=15.0), 'K must be'),
            (lambda: events(st=state(streak=torch.zeros(2, 8, 8))), 'state streak'),
            (lambda: events(st=state(since=torch.zeros(2, 8, 7, dtype=torch.int32))), 'state since'),
            (lambda: events(st=state(frame=torch.zeros(3, dtype=torch.int32))), 'state frame'),
            (lambda: events(st=state(counters=torch.zeros(2, 55, dtype=torch.int32))), 'state counters'),
            (lambda: events(st=state(geometry=torch.zeros(2, 305, dtype=torch.int32))), 'state geometry'),
            (lambda: events(min_frames=0), 'min_frames'),
            (lambda: events(min_frames=256), 'min_frames'),
            (lambda: events(max_events=0), 'max_events'),
            (lambda: events(max_events=4097), 'max_events'),
            (lambda: events(max_events=2.0), 'max_events'),
            (lambda: events(max_age=-1), 'max_age'),
            (lambda: events(anchor='toes'), 'anchor must be'),
            (lambda: events(anchor_kpts=(0, 1, 2, 3, 4)), 'anchor_kpts'),
            (lambda: events(anchor_kpts=(15,)), 'anchor_kpts'),
            (lambda: events(entries=[(kp, bb, None, ids, 0)]), 'entry 0 is'),
            (lambda: events(entries=[(kp[:, :14], bb, None, ids, 0, (1, 1))]), 'kpts of entry 0'),
            (lambda: events(entries=[(kp, bb[:, :4], None, ids, 0, (1, 1))]), 'bboxes of entry 0'),
            (lambda: events(entries=[(kp, bb, keep.long(), ids, 0, (1, 1))]), 'keep of entry 0'),
            (lambda: events(entries=[(kp, bb, None, ids.long(), 0, (1, 1))]), 'ids of entry 0'),
            (lambda: events(entries=[(kp, bb, None, None, 0, (1, 1))]), 'ids of entry 0'),
            (lambda: events(entries=[(kp, bb, None, ids, 2, (1, 1))]), 'camera of entry 0'),
            (lambda: events(entries=[(kp, bb, None, ids, 0, (1, 1)), (kp, bb, None, ids, 0, (1, 0))]), 'scale of entry 1'),
            (lambda: events(entries=[(kp, bb, None, ids, 0, 1.0)]), 'scale of entry 0'),
            (lambda: events(entries=[(kp.transpose(0, 1).contiguous().transpose(0, 1), bb, None, ids, 0, (1, 1))]),
             'contiguous'),
            (lambda: events(), 'HIP device')):
        with pytest.raises(ValueError, match=needle):
            call()
