"""Postures and falls, the parts that need no GPU: the edges of the rule of DESIGN section 20 as hand-worked scripts
on its numpy statement (tests/posture_cases.py on tests/posture_ref.py), what the rule gives on painted figures that
stand, crouch, raise their hands, lie and fall under jitter, the plan's C layout, and every refusal of the C entry
point and of the Python wrappers."""
import ctypes
import math
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import posture_cases as PC
from tests import posture_ref as PR
from tests.test_track_cpu import FIGURE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class OracleHarness:
    """tests/posture_cases.py's harness on the oracle alone."""

    def __init__(self, K, **kw):
        self.ref = PR.PostureRef(K, **kw)

    def frame(self, kpts, bboxes, ids, keep=None, camera=0):
        out = self.ref.update(kpts, bboxes, np.asarray(ids, np.int64).astype(np.int32),
                              None if keep is None else np.asarray(keep, np.int32), camera=camera)
        PC.invariant(self.ref.state(camera), self.ref.counts(camera))
        return out

    def poke(self, field, index, value, camera=0):
        getattr(self.ref, field)[(camera,) + tuple(index)] = value

    def get(self, field, camera=0):
        return getattr(self.ref, field)[camera]


@pytest.mark.parametrize('script', PC.SCRIPTS, ids=lambda s: s.__name__)
def test_hand_worked_scripts_on_the_oracle(script):
    script(OracleHarness)


# ---- painted figures: tests/test_track_cpu.py's FIGURE (K = 15, PoseTrack order), 1 % jitter on every coordinate ----
HEIGHTS = [40, 100, 300]
ANKLES_AT = np.asarray([.20, 1.0])      # the middle of the figure's ankles: what a falling figure turns about


def standing():
    return FIGURE.copy()


def crouching():
    fig = FIGURE.copy()
    fig[[11, 12], 1], fig[[13, 14], 1] = .62, .72
    return fig


def hands_up():
    fig = FIGURE.copy()
    fig[[7, 8], 1] = .05
    return fig


def turned(fig, degrees):
    """The figure turned about its ankles, in the picture plane."""
    a = math.radians(degrees)
    rot = np.asarray([[math.cos(a), -math.sin(a)], [math.sin(a), math.cos(a)]])
    return (fig - ANKLES_AT) @ rot.T + ANKLES_AT


def paint(figs, height, seed):
    """One detection per frame: figs[f] * height at (600, 400) with a jitter of 1 % of the height on every
    coordinate -> (kpts [1, 15, 3], bboxes [1, 5]) per frame."""
    rng = np.random.default_rng(seed)
    for fig in figs:
        xy = fig * height + (600.0, 400.0)
        kpts = np.empty((1, 15, 3), np.float32)
        kpts[0, :, :2] = xy + rng.uniform(-0.01, 0.01, xy.shape) * height
        kpts[0, :, 2] = 0.9
        k = kpts[0]
        yield kpts, np.asarray([[k[:, 0].min(), k[:, 1].min(), k[:, 0].max(), k[:, 1].max(), 0.8]], np.float32)


def watch(figs, height, seed):
    """-> (the oracle, raw [F], hands [F], the events of all frames as tuples)."""
    ref = PR.PostureRef(15)
    raw, hands, events = [], [], []
    for kpts, bboxes in paint(figs, height, seed):
        out = ref.update(kpts, bboxes, np.asarray([1], np.int32))
        PC.invariant(ref.state(0), ref.counts(0))
        raw.append(int(out['raw'][0]))
        hands.append(int(out['hands'][0]))
        events += PC.ev(out)
    return ref, raw, hands, events


@pytest.mark.parametrize('height', HEIGHTS)
def test_painted_figures_are_classed_in_every_frame(height):
    """200 frames each under the defaults: standing is UPRIGHT with no hand, knees at .62 and ankles at .72 LOW,
    wrists at .05 UPRIGHT with both hands, and the figure turned by +-90 degrees about its ankles LYING -- in every
    frame, so there is no event at all."""
    for name, fig, want, want_hands in (('standing', standing(), PR.UPRIGHT, 0), ('crouching', crouching(), PR.LOW, 0),
                                        ('hands up', hands_up(), PR.UPRIGHT, 3),
                                        ('lying left', turned(standing(), -90), PR.LYING, 0),
                                        ('lying right', turned(standing(), 90), PR.LYING, 0)):
        ref, raw, hands, events = watch([fig] * 200, height, seed=height + len(name))
        assert set(raw) == {want} and set(hands) == {want_hands}, (name, sorted(set(raw)), sorted(set(hands)))
        assert [e for e in events if e[0] != PR.DOWN] == [], (name, events)
        assert ref.now[0].tolist() == [int(c == want) for c in range(5)]
        assert int(ref.downs[0]) == (1 if want == PR.LYING else 0)         # born lying, still there after 75 frames


def fall(T, sign):
    """20 frames upright, a turn of sign * 90 degrees linear over T frames, 100 frames lying."""
    return [standing()] * 20 + [turned(standing(), sign * 90.0 * i / T) for i in range(1, T + 1)] + \
        [turned(standing(), sign * 90.0)] * 100


def kinds(events):
    return [e[0] for e in events]


@pytest.mark.parametrize('height', HEIGHTS)
@pytest.mark.parametrize('T', [4, 8, 16, 32, 64])
def test_a_fall_is_reported_once(height, T):
    """A turn to the floor within 64 frames is exactly one FALL, one DOWN after it, and the track ends LYING."""
    for sign in (1, -1):
        ref, raw, _, events = watch(fall(T, sign), height, seed=1000 * T + height + sign)
        assert kinds(events).count(PR.FALL) == 1 and kinds(events).count(PR.DOWN) == 1, (sign, events)
        assert int(ref.posture[0, 0]) == PR.LYING and int(ref.falls[0]) == 1 and int(ref.downs[0]) == 1
        where = kinds(events)
        assert where.index(PR.FALL) < where.index(PR.DOWN)


@pytest.mark.parametrize('height', HEIGHTS)
@pytest.mark.parametrize('T', [240, 480])
def test_lying_down_slowly_is_no_fall(height, T):
    """A turn that takes 240 frames or more spends more than fall_window frames LEANING: no FALL, and still one DOWN
    once the person has been lying for down_frames frames."""
    for sign in (1, -1):
        ref, raw, _, events = watch(fall(T, sign), height, seed=1000 * T + height + sign)
        assert kinds(events).count(PR.FALL) == 0 and kinds(events).count(PR.DOWN) == 1, (sign, events)
        assert int(ref.posture[0, 0]) == PR.LYING and int(ref.falls[0]) == 0


def test_where_a_turn_stops_being_a_fall():
    """Prints where the changeover between a fall (T = 64) and lying down (T = 240) falls: the trunk is LEANING between
    about 35 and 55 degrees, 21 / 90 of the turn, and that must take no more than fall_window = 30 frames, so it is
    expected near T = 30 * 90 / 21 = 129 (DESIGN section 20 has the figures).  Nothing is asserted on it."""
    for height in HEIGHTS:
        falls = {T: sum(kinds(watch(fall(T, sign), height, seed=7 * T + height + sign)[3]).count(PR.FALL)
                        for sign in (1, -1)) for T in range(96, 161, 4)}
        last_fall = max([T for T, n in falls.items() if n == 2], default=None)
        first_none = min([T for T, n in falls.items() if n == 0], default=None)
        print(f'height {height}: both turns are a FALL up to T = {last_fall}, neither from T = {first_none}; FALLs of the '
              f'two turns by T: {falls}')


# ---- layout and refusals ----
def test_defaults_and_ranges():
    import pavenet_amd
    from pavenet_amd import posture
    from pavenet_amd.posture import PostureMonitor
    assert pavenet_amd.PostureMonitor is PostureMonitor
    m = PostureMonitor(15)
    assert (m.K, m.cameras, m.max_tracks, m.max_age, m.min_frames, m.lean, m.flat, m.squat, m.hand_up, m.fall_window,
            m.down_frames, m.max_events, m.score_thr, m.kpt_thr) == (15, 1, 128, 30, 3, 11, 11, 18, 4, 30, 75, 256, 0.3, 0.0)
    r = PR.PostureRef(15)
    assert (r.S, r.max_age, r.min_frames, r.lean, r.flat, r.squat, r.hand_up, r.fall_window, r.down_frames, r.max_events,
            float(r.score_thr), float(r.kpt_thr)) == (128, 30, 3, 11, 11, 18, 4, 30, 75, 256, float(np.float32(0.3)), 0.0)
    for K in (17, 15, 14):
        assert PostureMonitor(K).parts == posture.PARTS[K] == PR.PARTS[K] == PR.PostureRef(K).parts
    assert posture.PARTS[17] == dict(shoulders=(5, 6), hips=(11, 12), ankles=(15, 16), wrists=(9, 10))
    assert posture.PARTS[15] == dict(shoulders=(3, 4), hips=(9, 10), ankles=(13, 14), wrists=(7, 8))
    assert posture.PARTS[14] == dict(shoulders=(0, 1), hips=(6, 7), ankles=(10, 11), wrists=(4, 5))
    assert (posture.UNKNOWN, posture.UPRIGHT, posture.LOW, posture.LEANING, posture.LYING) == \
        (PR.UNKNOWN, PR.UPRIGHT, PR.LOW, PR.LEANING, PR.LYING) == (0, 1, 2, 3, 4)
    assert (posture.POSTURE, posture.FALL, posture.DOWN, posture.HANDS_UP, posture.HANDS_DOWN) == \
        (PR.POSTURE, PR.FALL, PR.DOWN, PR.HANDS_UP, PR.HANDS_DOWN) == (1, 2, 3, 4, 5)
    assert posture.KINDS == {1: 'posture', 2: 'fall', 3: 'down', 4: 'hands_up', 5: 'hands_down'}
    one = dict(shoulders=(0,), hips=[0], ankles=(), wrists=(0, 0, 0, 0))
    assert PostureMonitor(1, parts=one).parts == dict(shoulders=(0,), hips=(0,), ankles=(), wrists=(0, 0, 0, 0))
    for kw in (dict(min_frames=1), dict(min_frames=255), dict(max_events=1), dict(max_events=4096), dict(max_tracks=1),
               dict(max_age=0), dict(cameras=4096), dict(lean=1), dict(lean=255), dict(flat=1), dict(flat=255),
               dict(squat=0), dict(squat=255), dict(hand_up=0), dict(hand_up=255), dict(hand_up=None),
               dict(fall_window=0), dict(fall_window=1 << 30), dict(down_frames=0), dict(down_frames=1 << 30)):
        PostureMonitor(15, **kw)
    for call, needle in ((lambda: PostureMonitor(0), 'K is'),
                         (lambda: PostureMonitor(33), 'K is'),
                         (lambda: PostureMonitor(15, cameras=0), 'cameras'),
                         (lambda: PostureMonitor(15, cameras=4097), 'cameras'),
                         (lambda: PostureMonitor(15, max_tracks=0), 'max_tracks'),
                         (lambda: PostureMonitor(15, max_tracks=129), 'max_tracks'),
                         (lambda: PostureMonitor(15, max_age=-1), 'max_age'),
                         (lambda: PostureMonitor(15, max_age=1.5), 'max_age'),
                         (lambda: PostureMonitor(15, min_frames=0), 'min_frames'),
                         (lambda: PostureMonitor(15, min_frames=256), 'min_frames'),
                         (lambda: PostureMonitor(15, min_frames=2.0), 'min_frames'),
                         (lambda: PostureMonitor(15, max_events=0), 'max_events'),
                         (lambda: PostureMonitor(15, max_events=4097), 'max_events'),
                         (lambda: PostureMonitor(15, max_events=True), 'max_events'),
                         (lambda: PostureMonitor(15, lean=0), 'lean'),
                         (lambda: PostureMonitor(15, lean=256), 'lean'),
                         (lambda: PostureMonitor(15, lean=11.0), 'lean'),
                         (lambda: PostureMonitor(15, flat=0), 'flat'),
                         (lambda: PostureMonitor(15, flat=256), 'flat'),
                         (lambda: PostureMonitor(15, squat=-1), 'squat'),
                         (lambda: PostureMonitor(15, squat=256), 'squat'),
                         (lambda: PostureMonitor(15, hand_up=-1), 'hand_up'),
                         (lambda: PostureMonitor(15, hand_up=256), 'hand_up'),
                         (lambda: PostureMonitor(15, hand_up=False), 'hand_up'),
                         (lambda: PostureMonitor(15, fall_window=-1), 'fall_window'),
                         (lambda: PostureMonitor(15, fall_window=(1 << 30) + 1), 'fall_window'),
                         (lambda: PostureMonitor(15, down_frames=-1), 'down_frames'),
                         (lambda: PostureMonitor(15, down_frames=(1 << 30) + 1), 'down_frames'),
                         (lambda: PostureMonitor(15, down_frames=75.0), 'down_frames'),
                         (lambda: PostureMonitor(16), 'needs parts'),
                         (lambda: PostureMonitor(15, parts=[(3, 4), (9, 10), (13, 14), (7, 8)]), 'parts is a dict'),
                         (lambda: PostureMonitor(15, parts=dict(shoulders=(3, 4), hips=(9, 10), ankles=(13, 14))), 'parts is a dict'),
                         (lambda: PostureMonitor(15, parts=dict(one, knees=(1,))), 'parts is a dict'),
                         (lambda: PostureMonitor(15, parts=dict(one, hips=5)), 'sequence'),
                         (lambda: PostureMonitor(15, parts=dict(one, hips=(0, 1, 2, 3, 4))), 'at most 4'),
                         (lambda: PostureMonitor(15, parts=dict(one, ankles=(15,))), 'key points of ankles'),
                         (lambda: PostureMonitor(15, parts=dict(one, wrists=(-1,))), 'key points of wrists'),
                         (lambda: PostureMonitor(15, parts=dict(one, shoulders=(1.0,))), 'key points of shoulders')):
        with pytest.raises(ValueError, match=needle):
            call()


def _lib():
    from pavenet_amd import native
    from pavenet_amd.build_native import build_native
    build_native()
    return native, native.load()


def test_posture_plan_layout_and_entry(tmp_path):
    """native.PosturePlan is the header's pave_posture_plan field for field, under the 4 KB kernel-argument limit, and
    the entry is in the header, the binding and both libraries."""
    native, lib = _lib()
    vp, ci = ctypes.c_void_p, ctypes.c_int
    assert native.FUNCTIONS['pave_posture_events'] == (ci, [vp, vp]) and 'pave_posture_events' in native.SIGNATURES
    assert hasattr(lib, 'pave_posture_events')
    for path in (native.LIB_PATH, native.DIAG_LIB_PATH):
        out = subprocess.run(['nm', '-D', '--defined-only', path], capture_output=True, text=True, check=True).stdout
        assert 'pave_posture_events' in {ln.split()[-1] for ln in out.splitlines()}
    assert lib.pave_abi_version() == native.ABI_VERSION
    assert ctypes.sizeof(native.PosturePlan) == 3312 < 4096
    D = native.DEFINES
    assert [D['PAVE_POSTURE_' + n] for n in ('UNKNOWN', 'UPRIGHT', 'LOW', 'LEANING', 'LYING', 'CLASSES')] == [0, 1, 2, 3, 4, 5]
    assert [D['PAVE_POSTURE_EV_' + n] for n in ('POSTURE', 'FALL', 'DOWN', 'HANDS_UP', 'HANDS_DOWN')] == [1, 2, 3, 4, 5]
    assert [D['PAVE_POSTURE_PART_' + n] for n in ('SHOULDERS', 'HIPS', 'ANKLES', 'WRISTS')] == [0, 1, 2, 3]
    assert [D['PAVE_POSTURE_CNT_' + n] for n in ('NOW', 'HANDS_UP', 'FALLS', 'DOWNS')] == [0, 5, 6, 7]
    assert (D['PAVE_POSTURE_COUNTER_WORDS'], D['PAVE_POSTURE_PARTS'], D['PAVE_POSTURE_MAX_PART'], D['PAVE_POSTURE_MAX_EVENTS'],
            D['PAVE_POSTURE_EVENT_WORDS'], D['PAVE_POSTURE_MAX_SLOPE'], D['PAVE_POSTURE_MAX_WAIT'],
            D['PAVE_POSTURE_HANDS_OFF']) == (8, 4, 4, 4096, 5, 255, 1 << 30, -1)
    if not shutil.which('gcc'):
        pytest.skip('no gcc')
    fields = [f for f, _ in native.PosturePlan._fields_]
    src = tmp_path / 'layout.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pave_hip.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(pave_posture_plan));\n'
                   + ''.join(f'  printf(" %zu", offsetof(pave_posture_plan, {f}));\n' for f in fields)
                   + '  return 0;\n}\n')
    exe = tmp_path / 'layout'
    subprocess.run(['gcc', '-std=c99', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == ctypes.sizeof(native.PosturePlan) < 4096
    assert got[1:] == [getattr(native.PosturePlan, f).offset for f in fields]


STATE_FIELDS = ('slot_id', 'slot_last', 'slot_posture', 'slot_since', 'slot_upright', 'slot_streak', 'slot_alerted',
                'slot_hands', 'slot_hand_streak', 'frame', 'dropped', 'counters')
OUT_FIELDS = ('out_posture', 'out_raw', 'out_hands', 'out_since')


def test_c_entry_refuses_bad_plans_before_any_device_call():
    """No GPU: every refusal is PAVE_E_ARG with a message (the addresses are never dereferenced)."""
    native, lib = _lib()
    host = (ctypes.c_ubyte * 64)()
    addr = ctypes.addressof(host)

    def plan(entries=2, n=3, K=15, S=8, cameras=2, camera=1, scale=(1.0, 1.0), max_age=30, min_frames=3, max_events=256,
             lean=11, flat=11, squat=18, hand_up=4, fall_window=30, down_frames=75,
             parts=((3, 4), (9, 10), (13, 14), (7, 8)), kpts=addr, bboxes=addr, ids=addr, keep=None, out_events=addr,
             out_n_events=addr, **other):
        p = native.PosturePlan()
        for i in range(min(max(entries, 0), 32)):
            p.kpts[i], p.bboxes[i], p.ids[i], p.keep[i] = kpts, bboxes, ids, keep
            for f in OUT_FIELDS:
                getattr(p, f)[i] = other.get(f, addr)
            p.out_events[i], p.out_n_events[i] = out_events, out_n_events
            p.n[i], p.camera[i], p.scale[i][0], p.scale[i][1] = n, camera, scale[0], scale[1]
        for f in STATE_FIELDS:
            setattr(p, f, other.get(f, addr))
        for q, keys in enumerate(parts):
            p.n_part[q] = len(keys)
            for i, k in enumerate(keys[:4]):
                p.part[q][i] = k
        p.entries, p.cameras, p.S, p.K, p.max_age = entries, cameras, S, K, max_age
        p.min_frames, p.max_events, p.lean, p.flat, p.squat, p.hand_up = min_frames, max_events, lean, flat, squat, hand_up
        p.fall_window, p.down_frames = fall_window, down_frames
        p.score_thr, p.kpt_thr = 0.3, 0.0
        return p

    def refused(p, needle):
        assert lib.pave_posture_events(ctypes.byref(p) if p is not None else None, None) == native.DEFINES['PAVE_E_ARG'] == -1
        assert needle in lib.pave_last_error().decode(), lib.pave_last_error()

    refused(None, 'null plan')
    refused(plan(entries=0), 'frames per launch')
    refused(plan(entries=33), 'frames per launch')
    refused(plan(kpts=None), 'null pose')
    refused(plan(bboxes=None), 'null pose')
    refused(plan(ids=None), 'null ids')
    for f in OUT_FIELDS:
        refused(plan(**{f: None}), 'null output')
    refused(plan(out_events=None), 'null events')
    refused(plan(out_n_events=None), 'null events')
    refused(plan(n=0, out_events=None), 'null events')
    for f in STATE_FIELDS:
        refused(plan(**{f: None}), 'null state')
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
    refused(plan(lean=0), 'lean outside')
    refused(plan(lean=256), 'lean outside')
    refused(plan(flat=0), 'flat outside')
    refused(plan(flat=256), 'flat outside')
    refused(plan(squat=-1), 'squat outside')
    refused(plan(squat=256), 'squat outside')
    refused(plan(hand_up=-2), 'hand_up outside')
    refused(plan(hand_up=256), 'hand_up outside')
    refused(plan(fall_window=-1), 'fall_window outside')
    refused(plan(fall_window=(1 << 30) + 1), 'fall_window outside')
    refused(plan(down_frames=-1), 'down_frames outside')
    refused(plan(down_frames=(1 << 30) + 1), 'down_frames outside')
    for q in range(4):
        parts = [(3, 4), (9, 10), (13, 14), (7, 8)]
        parts[q] = (0, 1, 2, 3, 4)
        refused(plan(parts=parts), 'n_part')
        p = plan()
        p.n_part[q] = -1
        refused(p, 'n_part')
        parts[q] = (14, 15)
        refused(plan(parts=parts), 'part key point')
        parts[q] = (-1,)
        refused(plan(parts=parts), 'part key point')
    refused(plan(K=14), 'part key point')


def test_wrappers_raise_value_errors_on_host_tensors():
    """Shape, type and range checks, and the host-tensor check itself, are ValueErrors raised before anything is
    allocated on or asked of a device."""
    from pavenet_amd import native, ops, posture
    from pavenet_amd.posture import PostureMonitor
    kp, bb, keep = torch.zeros(3, 15, 3), torch.zeros(3, 5), torch.ones(3, dtype=torch.int32)
    ids = torch.ones(3, dtype=torch.int32)
    res = (bb, None, kp)
    mon = PostureMonitor(15, cameras=2)
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
            (lambda: mon.state(-1), 'camera')):
        with pytest.raises(ValueError, match=needle):
            call()
    assert mon._state is None and mon.state(0) is None and mon.counts(1) is None and mon.update_many([]) == []
    mon.reset()
    table = torch.tensor([[posture.POSTURE, 4, 7, 0, 3], [posture.FALL, 2, 7, 0, 3], [0, 0, 0, 0, 0]], dtype=torch.int32)
    two = [dict(kind='posture', index=4, id=7, pose=0, frame=3), dict(kind='fall', index=2, id=7, pose=0, frame=3)]
    assert posture.events_to_list(dict(events=table, n_events=torch.tensor(2, dtype=torch.int32))) == two
    assert posture.events_to_list(dict(events=table[:2], n_events=torch.tensor(5, dtype=torch.int32))) == two   # 3 not stored
    assert posture.events_to_list(dict(events=table, n_events=torch.tensor(0, dtype=torch.int32))) == []

    def state(cameras=2, S=8, **over):
        z = dict(dtype=torch.int32)
        s = {n: torch.zeros(cameras, S, **z) for n in PR.SLOTS}
        s.update(frame=torch.zeros(cameras, **z), dropped=torch.zeros(cameras, **z),
                 counters=torch.zeros(cameras, native.POSTURE_COUNTER_WORDS, **z))
        s.update(over)
        return s
    parts = [(3, 4), (9, 10), (13, 14), (7, 8)]

    def events(entries=((kp, bb, None, ids, 0, (1.0, 1.0)),), st=None, K=15, parts=parts, **kw):
        return ops.posture_events(entries, state() if st is None else st, K=K, parts=parts, **kw)
    for call, needle in (
            (lambda: events(st=dict(id=bb)), 'state holds'),
            (lambda: events(st=state(id=torch.zeros(2, 8, 2, dtype=torch.int32))), 'state id'),
            (lambda: events(st=state(S=129)), 'S in'),
            (lambda: events(K=33), 'K'),
            (lambda: events(K=15.0), 'K must be'),
            (lambda: events(st=state(streak=torch.zeros(2, 8))), 'state streak'),
            (lambda: events(st=state(upright=torch.zeros(2, 7, dtype=torch.int32))), 'state upright'),
            (lambda: events(st=state(frame=torch.zeros(3, dtype=torch.int32))), 'state frame'),
            (lambda: events(st=state(counters=torch.zeros(2, 7, dtype=torch.int32))), 'state counters'),
            (lambda: events(min_frames=0), 'min_frames'),
            (lambda: events(min_frames=256), 'min_frames'),
            (lambda: events(max_events=0), 'max_events'),
            (lambda: events(max_events=4097), 'max_events'),
            (lambda: events(max_events=2.0), 'max_events'),
            (lambda: events(max_age=-1), 'max_age'),
            (lambda: events(lean=0), 'lean'),
            (lambda: events(flat=256), 'flat'),
            (lambda: events(squat=-1), 'squat'),
            (lambda: events(hand_up=256), 'hand_up'),
            (lambda: events(fall_window=-1), 'fall_window'),
            (lambda: events(down_frames=(1 << 30) + 1), 'down_frames'),
            (lambda: events(parts=parts[:3]), 'parts are'),
            (lambda: events(parts=5), 'parts are'),
            (lambda: events(parts=parts[:3] + [(0, 1, 2, 3, 4)]), 'part wrists'),
            (lambda: events(parts=[(15,)] + parts[1:]), 'part shoulders'),
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
