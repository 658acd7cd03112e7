"""Contacts and groups, the parts that need no GPU: the rule of DESIGN section 24 as hand-worked scripts on its numpy
statement (tests/contact_cases.py on tests/contact_ref.py), the plan's C layout, the entry in the header, the binding
and both libraries, every refusal of the C entry point and of the Python calls, the exports and the documents, and two
measurements on the numpy chain floor_ref -> contact_ref for the README and DESIGN section 24."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import contact_cases as CC
from tests import contact_ref as CR
from tests import floor_ref as FR
from tests.test_floor_cpu import camera_matrix
from tests.test_heat_cpu import layout
from tests.test_track_gpu import FIGURE15, poses


class OracleHarness:
    """tests/contact_cases.py's harness on the oracle alone."""

    def __init__(self, **kw):
        self.ref = CR.ContactRef(**kw)

    def frame(self, xy, ids, on=None, camera=0):
        xy = np.asarray(xy, np.int64).reshape(-1, 2).astype(np.int32)
        on = np.ones(len(xy), np.int32) if on is None else np.asarray(on, np.int32)
        return self.ref.update(on, xy, np.asarray(ids, np.int64).astype(np.int32), camera)

    def counts(self, camera=0):
        return self.ref.counts(camera)

    def get(self, field, camera=0):
        return self.ref.state(camera)[field]

    def pair(self, field, camera=0):
        return self.ref.pairs(camera)[field]


@pytest.mark.parametrize('script', CC.SCRIPTS, ids=lambda s: s.__name__)
def test_hand_worked_scripts_on_the_oracle(script):
    script(OracleHarness)


def test_the_oracle_on_random_frames_keeps_its_invariants():
    """40 random frames: contacts == meets - parts after every frame, a pair yields at most one event of the second
    section per frame, the events are ordered as the rule says, and every group is named by its smallest id."""
    rng = np.random.default_rng(251)
    ref = CR.ContactRef(max_tracks=24, max_age=2, radius=1500, release=1900, min_frames=2, long_frames=4, max_events=64)
    spots = rng.integers(-4000, 4000, (30, 2))
    seen_kinds = set()
    for f in range(40):
        n = int(rng.integers(0, 28))
        who = rng.integers(-1, 31, n)
        spots += rng.integers(-250, 251, spots.shape)
        out = ref.update((rng.uniform(size=n) < 0.9).astype(np.int32), spots[np.clip(who, 1, 30) - 1].astype(np.int32),
                         who.astype(np.int32))
        c = ref.counts(0)
        assert c['contacts'] == c['meets'] - c['parts'] and c['grouped'] >= 2 * c['groups'] and c['largest'] <= 24
        rows = out['events'][:int(out['n_events'])].tolist()
        later = [r for r in rows if not (r[0] == CR.PART and r[4] == -1 and r[5] == -1)]
        assert len({(r[1], r[2]) for r in later}) == len(later) and all(r[1] < r[2] and r[6] == f + 1 for r in rows)
        seen_kinds |= {r[0] for r in rows}
        taking = out['size'] > 0
        assert (out['group'][taking] <= who[taking]).all() and (out['group'][taking] >= 1).all()
    assert seen_kinds == {CR.MEET, CR.PART, CR.LONG} and ref.dropped[0] > 0


WALK_H = camera_matrix(55.0, 3000.0, 3000.0, size=4096)


def walkers(rng, where):
    """The floor tests' walking model: people of 1.7 m whose feet are at the floor points `where` [(X, Y) mm] under the
    tilted camera, as key points with 1 % jitter -> kpts, bboxes."""
    M = np.linalg.inv(WALK_H)
    kpts, bboxes = [], []
    for X, Y in where:
        feet, head = M @ [X, Y, 1.0], M @ [X, Y + 1.0, 1.0]
        feet, head = feet[:2] / feet[2], head[:2] / head[2]
        h = 1700.0 * np.hypot(*(head - feet))               # pixels per mm along the floor, times a person
        k, b = poses(rng, FIGURE15, [(feet[0] - 0.2 * h, feet[1] - h)], height=h)
        kpts.append(k)
        bboxes.append(b)
    return np.concatenate(kpts), np.concatenate(bboxes)


def test_six_walkers_one_couple_and_two_who_pass():
    """Six people at 1.4 m/s and 25 frames a second (56 mm a frame) for 100 frames under the tilted camera, key points
    with 1 % jitter, through floor_ref -> contact_ref (radius 1500, release 1800, min_frames 3, long_frames 50).  Ids 1
    and 2 walk side by side 600 mm apart: exactly one MEET, no PART, one LONG, one group of 2.  Ids 3 and 4 pass each
    other on lanes 5 m apart and never meet; nobody else does either."""
    rng = np.random.default_rng(252)
    plane = FR.FloorRef(15)
    plane.set_plane(0, matrix=WALK_H)
    mon = CR.ContactRef(radius=1500, release=1800, min_frames=3, long_frames=50)
    lanes = [(2500.0, 1), (3100.0, 1), (6000.0, -1), (11000.0, 1), (8500.0, 1), (13500.0, -1)]
    ids = np.arange(1, 7, dtype=np.int32)
    rows, closest = [], 1e9
    for f in range(100):
        where = [(way * (-2800.0 + 56.0 * f), Y) for Y, way in lanes]
        placed = plane.update(*walkers(rng, where), ids)
        assert placed['on'].all()
        out = mon.update(placed['on'], placed['xy'], ids)
        rows += out['events'][:int(out['n_events'])].tolist()
        closest = min(closest, float(np.hypot(*(placed['xy'][2] - placed['xy'][3]).tolist())))
        gap = float(np.hypot(*(placed['xy'][0] - placed['xy'][1]).tolist()))
        assert abs(gap - 600) < 300, gap
    assert [r[:3] for r in rows] == [[CR.MEET, 1, 2], [CR.LONG, 1, 2]], rows
    assert rows[0][6] == 3 and rows[1][3] == 50 and rows[1][6] == 53
    assert out['group'].tolist() == [1, 1, 3, 4, 5, 6] and out['size'].tolist() == [2, 2, 1, 1, 1, 1]
    assert out['partner'].tolist() == [2, 1, 0, 0, 0, 0] and out['together'][0] == 97
    c = mon.counts(0)
    assert (c['contacts'], c['meets'], c['parts'], c['longs'], c['groups'], c['grouped'], c['largest']) == (1, 1, 0, 1, 1, 2, 2)
    print(f'ids 3 and 4 came within {closest:.0f} mm of each other (radius 1500)')
    assert closest > 3000


FLIPS = {}


@pytest.mark.parametrize('min_frames', [1, 3])
@pytest.mark.parametrize('band', [0, 300])
def test_flips_of_a_pair_standing_exactly_at_the_radius(band, min_frames):
    """A measurement for the README and DESIGN section 24: two people standing exactly 1500 mm apart 2.5 m from the
    camera's foot for 200 frames, key points with 1 % jitter; how often the contact bit flips (MEETs + PARTs) at release
    = radius and radius + 300, min_frames 1 and 3.  What is asserted is what the table shows: without hysteresis the bit
    flickers and min_frames 3 thins it out, with a 300 mm band it is set once and stays."""
    rng = np.random.default_rng(253)
    plane = FR.FloorRef(15)
    plane.set_plane(0, matrix=WALK_H)
    mon = CR.ContactRef(radius=1500, release=1500 + band, min_frames=min_frames)
    ids = np.asarray([1, 2], np.int32)
    gaps = []
    for f in range(200):
        placed = plane.update(*walkers(rng, [(-750.0, 2500.0), (750.0, 2500.0)]), ids)
        mon.update(placed['on'], placed['xy'], ids)
        gaps.append(float(np.hypot(*(placed['xy'][0] - placed['xy'][1]).tolist())))
    c = mon.counts(0)
    flips = int(c['meets'] + c['parts'])
    FLIPS[band, min_frames] = flips
    print(f'release = radius + {band}, min_frames {min_frames}: {flips} flips in 200 frames; the measured distance was '
          f'{np.mean(gaps):.0f} mm, {min(gaps):.0f} .. {max(gaps):.0f}')
    if band == 300:
        assert flips == 1 and c['contacts'] == 1
    else:
        assert flips > 1
    if len(FLIPS) == 4:
        assert FLIPS[0, 3] < FLIPS[0, 1]


def _lib():
    from pavenet_amd import native
    from pavenet_amd.build_native import build_native
    build_native()
    return native, native.load()


def test_contact_plan_layout_and_entry(tmp_path):
    """native.ContactPlan is the header's pave_contact_plan field for field, under the 4 KB kernel-argument limit, and
    the entry is in the header, the binding and both libraries; the ABI number is the one it was."""
    native, lib = _lib()
    vp, ci = ctypes.c_void_p, ctypes.c_int
    assert native.FUNCTIONS['pave_contact_update'] == (ci, [vp, vp]) and 'pave_contact_update' in native.SIGNATURES
    for path in (native.LIB_PATH, native.DIAG_LIB_PATH):
        out = subprocess.run(['nm', '-D', '--defined-only', path], capture_output=True, text=True, check=True).stdout
        assert 'pave_contact_update' in {ln.split()[-1] for ln in out.splitlines()}
    assert native.ABI_VERSION == 21 and lib.pave_abi_version() == 21
    assert ctypes.sizeof(native.ContactPlan) == 1896 < 4096
    assert (native.CONTACT_OUT_WORDS, native.CONTACT_EVENT_WORDS, native.CONTACT_COUNTER_WORDS) == (5, 7, 8)
    assert (native.CONTACT_MAX_RADIUS, native.CONTACT_MAX_RELEASE, native.CONTACT_MAX_LONG, native.CONTACT_MAX_EVENTS) == \
        (2 ** 20, 2 ** 21, 2 ** 30, 4096)
    if shutil.which('gcc'):
        layout(tmp_path, native.ContactPlan, 'pave_contact_plan')


STATE_FIELDS = ('slot_id', 'slot_last', 'slot_pos', 'link', 'since', 'frame', 'dropped', 'counters')


def test_c_entry_refuses_bad_plans_before_any_device_call():
    """No GPU: every refusal is PAVE_E_ARG with a message (the addresses are never dereferenced)."""
    native, lib = _lib()
    host = (ctypes.c_ubyte * 64)()
    addr = ctypes.addressof(host)

    def plan(entries=2, n=3, S=8, cameras=2, camera=1, max_age=30, radius=1500, release=1500, min_frames=3, long_frames=0,
             max_events=16, **over):
        p = native.ContactPlan()
        for i in range(min(max(entries, 0), 32)):
            p.on[i], p.xy[i], p.ids[i] = over.get('on', addr), over.get('xy', addr), over.get('ids', addr)
            p.out[i], p.out_events[i] = over.get('out', addr), over.get('out_events', addr)
            p.out_n_events[i] = over.get('out_n_events', addr)
            p.n[i], p.camera[i] = n, camera
        for f in STATE_FIELDS:
            setattr(p, f, over.get(f, addr))
        p.entries, p.cameras, p.S, p.max_age = entries, cameras, S, max_age
        p.radius, p.release, p.min_frames, p.long_frames, p.max_events = radius, release, min_frames, long_frames, max_events
        return p

    def refused(p, needle):
        assert lib.pave_contact_update(ctypes.byref(p) if p is not None else None, None) == native.DEFINES['PAVE_E_ARG'] == -1
        assert needle in lib.pave_last_error().decode(), lib.pave_last_error()

    refused(None, 'null plan')
    refused(plan(entries=0), 'frames per launch')
    refused(plan(entries=33), 'frames per launch')
    refused(plan(on=None), 'null floor')
    refused(plan(xy=None), 'null floor')
    refused(plan(ids=None), 'null ids')
    for f in ('out', 'out_events', 'out_n_events'):
        refused(plan(**{f: None}), 'null output')
    refused(plan(n=0, out_events=None), 'null output')
    refused(plan(n=0, out_n_events=None), 'null output')
    for f in STATE_FIELDS:
        refused(plan(**{f: None}), 'null state')
    for kw, needle in ((dict(n=-1), 'N outside'), (dict(n=129), 'N outside'), (dict(S=0), 'max_tracks'), (dict(S=129), 'max_tracks'),
                       (dict(cameras=0), 'cameras outside'), (dict(cameras=4097), 'cameras outside'),
                       (dict(camera=-1), 'camera index'), (dict(camera=2), 'camera index'), (dict(max_age=-1), 'max_age'),
                       (dict(radius=-1, release=0), 'radius'), (dict(radius=2 ** 20 + 1, release=2 ** 20 + 1), 'radius'),
                       (dict(release=1499), 'release'), (dict(release=2 ** 21 + 1), 'release'),
                       (dict(min_frames=0), 'min_frames'), (dict(min_frames=256), 'min_frames'),
                       (dict(long_frames=-1), 'long_frames'), (dict(long_frames=2 ** 30 + 1), 'long_frames'),
                       (dict(max_events=0), 'max_events'), (dict(max_events=4097), 'max_events')):
        refused(plan(**kw), needle)


def test_defaults_ranges_and_exports():
    import pavenet_amd
    from pavenet_amd import ContactMonitor, contacts, native
    assert ContactMonitor is contacts.ContactMonitor and pavenet_amd.ContactMonitor is ContactMonitor
    assert (contacts.MEET, contacts.PART, contacts.LONG) == (CR.MEET, CR.PART, CR.LONG) == (CC.MEET, CC.PART, CC.LONG)
    m = ContactMonitor()
    assert (m.cameras, m.max_tracks, m.max_age, m.radius, m.release, m.min_frames, m.long_frames, m.max_events) == \
        (1, 128, 30, 1500, 1500, 3, 0, 256)
    assert ContactMonitor(radius=700).release == 700 and ContactMonitor(radius=700, release=900).release == 900
    assert m.state(0) is None and m.counts(0) is None and m.pairs(0) is None and m.update_many([]) == [] and m._state is None
    m.reset()
    assert ContactMonitor._RESET == ('id', 'frame', 'dropped', 'counters')
    assert native.CONTACT_MAX_RADIUS == 2 ** 20 and native.FLOOR_MAX_MM == CR.MAX_MM
    for kw in (dict(radius=0), dict(radius=2 ** 20), dict(radius=2 ** 20, release=2 ** 21), dict(min_frames=1), dict(min_frames=255),
               dict(long_frames=2 ** 30), dict(max_events=1), dict(max_events=4096), dict(max_tracks=1), dict(cameras=4096),
               dict(max_age=0)):
        ContactMonitor(**kw)
    for kw, needle in ((dict(cameras=0), 'cameras'), (dict(cameras=4097), 'cameras'), (dict(max_tracks=0), 'max_tracks'),
                       (dict(max_tracks=129), 'max_tracks'), (dict(max_age=-1), 'max_age'), (dict(radius=-1), 'radius'),
                       (dict(radius=2 ** 20 + 1), 'radius'), (dict(radius=1500.0), 'radius'), (dict(radius=True), 'radius'),
                       (dict(release=1499), 'release'), (dict(release=2 ** 21 + 1), 'release'), (dict(release=1600.0), 'release'),
                       (dict(min_frames=0), 'min_frames'), (dict(min_frames=256), 'min_frames'),
                       (dict(long_frames=-1), 'long_frames'), (dict(long_frames=2 ** 30 + 1), 'long_frames'),
                       (dict(max_events=0), 'max_events'), (dict(max_events=4097), 'max_events')):
        with pytest.raises(ValueError, match=needle):
            ContactMonitor(**kw)


def test_calls_raise_value_errors_on_host_tensors():
    """Shape, type and range checks, and the host-tensor check itself, are ValueErrors raised before anything is
    allocated on or asked of a device."""
    from pavenet_amd import ops
    from pavenet_amd.contacts import ContactMonitor
    on, xy, ids = torch.ones(3, dtype=torch.int32), torch.zeros(3, 2, dtype=torch.int32), torch.ones(3, dtype=torch.int32)
    placed = dict(on=on, xy=xy)
    m = ContactMonitor(cameras=2)
    big = dict(on=torch.ones(129, dtype=torch.int32), xy=torch.zeros(129, 2, dtype=torch.int32))
    for call, needle in (
            (lambda: m.update((on, xy), ids), 'on and xy'),
            (lambda: m.update(dict(on=on), ids), 'on and xy'),
            (lambda: m.update(dict(on=on.long(), xy=xy), ids), 'on of placed'),
            (lambda: m.update(dict(on=on[None], xy=xy), ids), 'on of placed'),
            (lambda: m.update(dict(on=on, xy=xy.float()), ids), 'xy of placed'),
            (lambda: m.update(dict(on=on, xy=xy[:2]), ids), 'xy of placed'),
            (lambda: m.update(big, torch.zeros(129, dtype=torch.int32)), 'at most 128'),
            (lambda: m.update(placed, ids.long()), 'ids of placed'),
            (lambda: m.update(placed, ids[:2]), 'ids of placed'),
            (lambda: m.update(placed, [1, 2, 3]), 'ids of placed'),
            (lambda: m.update(placed, ids, camera=2), 'camera'),
            (lambda: m.update(placed, ids, camera=True), 'camera'),
            (lambda: m.update_many([(0, placed)]), 'triples'),
            (lambda: m.update(placed, ids), 'HIP device tensors'),
            (lambda: m.reset(camera=2), 'camera'),
            (lambda: m.counts(2), 'camera'),
            (lambda: m.pairs(-1), 'camera'),
            (lambda: m.state(2), 'camera')):
        with pytest.raises(ValueError, match=needle):
            call()
    assert m._state is None

    def state(cameras=2, S=8, **over):
        z = dict(dtype=torch.int32)
        s = dict(id=torch.zeros(cameras, S, **z), last=torch.zeros(cameras, S, **z), pos=torch.zeros(cameras, S, 2, **z),
                 link=torch.zeros(cameras, S, S, **z), since=torch.zeros(cameras, S, S, **z), frame=torch.zeros(cameras, **z),
                 dropped=torch.zeros(cameras, **z), counters=torch.zeros(cameras, 8, **z))
        s.update(over)
        return s

    def update(entries=((on, xy, ids, 0),), st=None, **kw):
        return ops.contact_update(entries, state() if st is None else st, **kw)
    for call, needle in (
            (lambda: update(st=dict(id=on)), 'state holds'),
            (lambda: update(st=state(id=torch.zeros(2, dtype=torch.int32))), 'state id'),
            (lambda: update(st=state(S=129)), 'S in'),
            (lambda: update(st=state(pos=torch.zeros(2, 8, 2))), 'state pos'),
            (lambda: update(st=state(link=torch.zeros(2, 8, 7, dtype=torch.int32))), 'state link'),
            (lambda: update(st=state(since=torch.zeros(2, 8, dtype=torch.int32))), 'state since'),
            (lambda: update(st=state(counters=torch.zeros(2, 7, dtype=torch.int32))), 'state counters'),
            (lambda: update(st=state(frame=torch.zeros(3, dtype=torch.int32))), 'state frame'),
            (lambda: update(radius=-1), 'radius'),
            (lambda: update(radius=2 ** 20 + 1), 'radius'),
            (lambda: update(radius=1.5), 'radius'),
            (lambda: update(release=1499), 'release'),
            (lambda: update(release=2 ** 21 + 1), 'release'),
            (lambda: update(min_frames=0), 'min_frames'),
            (lambda: update(min_frames=256), 'min_frames'),
            (lambda: update(long_frames=-1), 'long_frames'),
            (lambda: update(max_events=0), 'max_events'),
            (lambda: update(max_events=4097), 'max_events'),
            (lambda: update(max_age=-1), 'max_age'),
            (lambda: update(entries=[(on, xy, ids)]), 'entry 0 is'),
            (lambda: update(entries=[(on.long(), xy, ids, 0)]), 'on of entry 0'),
            (lambda: update(entries=[(on, xy[:, :1], ids, 0)]), 'xy of entry 0'),
            (lambda: update(entries=[(on, xy, None, 0)]), 'ids of entry 0'),
            (lambda: update(entries=[(on, xy, ids, 2)]), 'camera of entry 0'),
            (lambda: update(entries=[(on, xy.t().contiguous().t(), ids, 0)]), 'contiguous'),
            (lambda: update(), 'HIP device')):
        with pytest.raises(ValueError, match=needle):
            call()


def test_the_documents_point_to_section_24():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    from pavenet_amd import contacts, floor
    docs = {}
    for name in ('README.md', 'DESIGN.md', 'INTEGRATION.md'):
        with open(os.path.join(root, name)) as f:
            docs[name] = f.read()
    assert '## 24. Contacts and groups' in docs['DESIGN.md'] and 'ContactMonitor' in docs['README.md']
    assert 'pave_contact_update' in docs['INTEGRATION.md'] and 'ContactMonitor' in floor.__doc__
    for word in ('across cameras', 'group-level events', 'drawing the links', 'per zone'):
        assert word in contacts.__doc__.lower() and word in docs['DESIGN.md'].lower(), word
