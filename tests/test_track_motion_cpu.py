"""The constant-velocity motion model of the pose tracker, the parts that need no GPU: the rule of DESIGN section 14
"Motion" (tests/track_motion_ref.py) against the plain rule where the two must be equal, on people who walk fast, are
hidden or walk through each other, and at its arithmetic edges; the plan's C layout, every refusal of the C entry
point and of the Python wrappers."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import track_motion_cases as TC
from tests import track_ref as TR
from tests.test_track_cpu import C15, STATE_FIELDS, walk
from tests.track_motion_ref import TrackMotionRef

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHARED = ['id', 'last', 'kpts', 'vis', 'area', 'frame', 'next_id', 'dropped']
GAPS = {'no gap': (), '5-frame gap': range(15, 20), '10-frame gap': range(15, 25)}


def _same_shared_state(motion, plain, cameras, what):
    for c in cameras:
        got, exp = motion.state(c), plain.state(c)
        assert list(got) == SHARED + ['vel', 'hits'] and list(exp) == SHARED
        for name in SHARED:
            assert np.array_equal(got[name], exp[name]), f'{what}: camera {c} state {name}'


@pytest.mark.parametrize('height', [40, 100, 300])
@pytest.mark.parametrize('step', [1, 2, 4])
def test_degenerate_model_equals_the_plain_rule_on_walks(height, step):
    """max_predict = 0 and new_gate = 1: no shift and no wider test, so ids and shared state are the plain rule's
    (the velocities are still measured: they just go nowhere)."""
    motion, plain = TrackMotionRef(15, max_predict=0, new_gate=1), TR.TrackRef(15)
    for f, (kpts, bboxes, _) in enumerate(walk(height, step, seed=height * 10 + step)):
        assert np.array_equal(motion.update(kpts, bboxes), plain.update(kpts, bboxes)), f'frame {f}'
        _same_shared_state(motion, plain, [0], f'frame {f}')
    assert motion.next_id[0] == 7 and (motion.hits[0][:6] == 40).all()
    assert (motion.vel[0][:6, 0] != 0).any()


def test_degenerate_model_equals_the_plain_rule_with_absences_and_keep():
    """Two cameras, small M (drops and reuse), people who leave for longer and shorter than max_age, keep = 0 poses."""
    rng = np.random.default_rng(5)
    kw = dict(cameras=2, max_tracks=5, max_age=3)
    motion, plain = TrackMotionRef(15, max_predict=0, new_gate=1, **kw), TR.TrackRef(15, **kw)
    for f, (kpts, bboxes, who) in enumerate(walk(100, 3, frames=30, people=6, seed=11)):
        c = f % 2 if f < 20 else 0
        there = np.ones(6, bool)
        there[who == 1] = not 6 <= f < 10
        there[who == 2] = not 12 <= f < 24
        keep = (rng.uniform(size=6) > 0.2).astype(np.int32)
        args = (kpts[there], bboxes[there], keep[there], (0.694, 0.7), c)
        assert np.array_equal(motion.update(*args), plain.update(*args)), f'frame {f}'
        _same_shared_state(motion, plain, [0, 1], f'frame {f}')
    assert plain.dropped.sum() > 0 and plain.next_id[0] > 7


@pytest.mark.parametrize('height', [40, 100, 300])
@pytest.mark.parametrize('step', [0, 1, 2, 4, 8])
@pytest.mark.parametrize('gap', list(GAPS))
def test_links_survive_fast_walks_and_gaps(height, step, gap):
    """Six people for 40 frames, person 0 withheld for 5 or 10 frames: under the defaults (gain 8, max_predict =
    max_age = 30, new_gate 4) six ids, each person's constant.  The plain rule loses them in the cases named, so the
    comparison is not vacuous."""
    ref = TrackMotionRef(15)
    assert (ref.gain, ref.max_predict, ref.new_gate, ref.max_age) == (8, 30, 4, 30)
    seen = TC.ids_by_person(TC.walk_with_gap(height, step, GAPS[gap]), ref.update, 6)
    assert ref.next_id[0] == 7 and TC.constant_ids(seen)
    assert ((seen[:, 0] == -1) == np.isin(np.arange(40), list(GAPS[gap]))).all()
    if (height, step, gap) in ((40, 8, 'no gap'), (40, 1, '5-frame gap'), (100, 4, '5-frame gap'),
                               (300, 8, '5-frame gap')):
        plain = TR.TrackRef(15)
        lost = TC.ids_by_person(TC.walk_with_gap(height, step, GAPS[gap]), plain.update, 6)
        assert plain.next_id[0] > 7 and not TC.constant_ids(lost)


def test_the_limit_of_the_model():
    """A track born in one frame has no velocity in the next: it is linked only within sqrt(new_gate) = 2 times the
    OKS distance.  32 px per frame at 40 px height is beyond that, with or without a gap, so every frame is six births
    (16 px per frame at 40 px and 32 px at 100 px break too; 300 px tall people hold at 32 px per frame)."""
    for gap in GAPS.values():
        ref = TrackMotionRef(15)
        seen = TC.ids_by_person(TC.walk_with_gap(40, 32, gap), ref.update, 6)
        assert ref.next_id[0] > 7 and not TC.constant_ids(seen)


@pytest.mark.parametrize('height,step', [(100, 2), (100, 4), (100, 6), (300, 4), (300, 12), (40, 2), (40, 3)])
def test_crossing_people_keep_their_ids(height, step):
    """Two people walk through each other on one row: the model keeps both ids for all 60 frames, the plain rule
    swaps them."""
    ref, plain = TrackMotionRef(15), TR.TrackRef(15)
    seen = TC.ids_by_person(TC.crossing(height, step), ref.update, 2)
    assert ref.next_id[0] == 3 and TC.constant_ids(seen) and sorted(seen[0]) == [1, 2]
    lost = TC.ids_by_person(TC.crossing(height, step), plain.update, 2)
    assert not TC.constant_ids(lost)


@pytest.mark.parametrize('name', list(TC.edge_scripts()))
def test_arithmetic_edges(name):
    """Floor on negative sums and shifts, the prediction's clamps, the velocity's and the hit count's saturation, a gap
    above max_predict, the wider test of a track matched once: hand-worked values (tests/track_motion_cases.py)."""
    K, kw, steps = TC.edge_scripts()[name]
    ref = TrackMotionRef(K, **kw)

    def poke(slot, field, value):
        getattr(ref, field)[0, slot] = value
    TC.run_script(K, steps, ref.update, poke, lambda slot, field: getattr(ref, field)[0, slot])


def _lib():
    from pavenet_amd import native
    from pavenet_amd.build_native import build_native
    build_native()
    return native, native.load()


def test_motion_plan_layout_and_entry(tmp_path):
    """native.TrackMotionPlan is the header's pave_track_motion_plan field for field (its base pave_track_plan), fits
    the 4 KB kernel-argument limit, and the entry is in the header, the binding and both libraries at ABI 21."""
    native, lib = _lib()
    vp, ci = ctypes.c_void_p, ctypes.c_int
    assert native.FUNCTIONS['pave_track_poses_motion'] == (ci, [vp, vp])
    assert 'pave_track_poses_motion' in native.SIGNATURES and hasattr(lib, 'pave_track_poses_motion')
    for path in (native.LIB_PATH, native.DIAG_LIB_PATH):
        out = subprocess.run(['nm', '-D', '--defined-only', path], capture_output=True, text=True, check=True).stdout
        assert 'pave_track_poses_motion' in {ln.split()[-1] for ln in out.splitlines()}
    assert native.ABI_VERSION == 21 and lib.pave_abi_version() == 21
    assert ctypes.sizeof(native.TrackMotionPlan) <= 4096
    assert native.TrackMotionPlan._fields_[0] == ('base', native.TrackPlan) and native.TrackMotionPlan.base.offset == 0
    if not shutil.which('gcc'):
        pytest.skip('no gcc')
    fields = [f for f, _ in native.TrackMotionPlan._fields_]
    src = tmp_path / 'layout.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pave_hip.h"\nint main(void) {\n'
                   '  printf("%zu %zu", sizeof(pave_track_motion_plan), sizeof(pave_track_plan));\n'
                   + ''.join(f'  printf(" %zu", offsetof(pave_track_motion_plan, {f}));\n' for f in fields)
                   + '  return 0;\n}\n')
    exe = tmp_path / 'layout'
    subprocess.run(['gcc', '-std=c99', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == ctypes.sizeof(native.TrackMotionPlan) and got[1] == ctypes.sizeof(native.TrackPlan)
    assert got[2:] == [getattr(native.TrackMotionPlan, f).offset for f in fields]


def test_c_entry_refuses_bad_plans_before_any_device_call():
    """No GPU: every refusal is PAVE_E_ARG with a message (the addresses are never dereferenced): the base plan's,
    through the shared check, and the motion plan's own."""
    native, lib = _lib()
    host = (ctypes.c_ubyte * 64)()
    addr = ctypes.addressof(host)

    def plan(entries=2, n=3, K=15, M=8, cameras=2, camera=1, scale=(1.0, 1.0), C=1000, min_kpts=5, max_age=30,
             kpts=addr, bboxes=addr, ids=addr, keep=None, scratch=addr, track_vel=addr, track_hits=addr, gain=8,
             max_predict=30, new_gate=4, **state):
        full = native.TrackMotionPlan()
        p = full.base
        for i in range(min(max(entries, 0), 32)):
            p.kpts[i], p.bboxes[i], p.ids[i], p.keep[i] = kpts, bboxes, ids, keep
            p.n[i], p.camera[i], p.scale[i][0], p.scale[i][1] = n, camera, scale[0], scale[1]
        for f in STATE_FIELDS:
            setattr(p, f, state.get(f, addr))
        p.scratch = scratch
        for k in range(32):
            p.C[k] = C if k < max(K, 0) else 0
        p.entries, p.cameras, p.M, p.K, p.min_kpts, p.max_age = entries, cameras, M, K, min_kpts, max_age
        p.score_thr, p.kpt_thr = 0.3, 0.0
        full.track_vel, full.track_hits = track_vel, track_hits
        full.gain, full.max_predict, full.new_gate = gain, max_predict, new_gate
        return full

    def refused(p, needle):
        st = lib.pave_track_poses_motion(ctypes.byref(p) if p is not None else None, None)
        assert st == native.DEFINES['PAVE_E_ARG'] == -1
        assert needle in lib.pave_last_error().decode(), lib.pave_last_error()

    refused(None, 'null plan')
    refused(plan(entries=0), 'frames per launch')
    refused(plan(entries=33), 'frames per launch')
    refused(plan(kpts=None), 'null pose')
    refused(plan(bboxes=None), 'null pose')
    refused(plan(ids=None), 'null ids')
    for f in STATE_FIELDS:
        refused(plan(**{f: None}), 'null state')
    refused(plan(scratch=None), 'null scratch')
    refused(plan(n=-1), 'N outside')
    refused(plan(n=129), 'N outside')
    refused(plan(K=0), 'K outside')
    refused(plan(K=33), 'K outside')
    refused(plan(M=0), 'max_tracks')
    refused(plan(M=129), 'max_tracks')
    refused(plan(cameras=0), 'cameras outside')
    refused(plan(cameras=4097), 'cameras outside')
    refused(plan(camera=-1), 'camera index')
    refused(plan(camera=2), 'camera index')
    for bad in ((0.0, 1.0), (1.0, -1.0), (float('nan'), 1.0), (1.0, float('inf'))):
        refused(plan(scale=bad), 'scale')
    refused(plan(C=0), 'C[k]')
    refused(plan(C=1 << 24), 'C[k]')
    refused(plan(min_kpts=0), 'min_kpts')
    refused(plan(min_kpts=16), 'min_kpts')
    refused(plan(max_age=-1), 'max_age')
    refused(plan(track_vel=None), 'null velocity or hits')
    refused(plan(track_hits=None), 'null velocity or hits')
    refused(plan(gain=0), 'gain outside')
    refused(plan(gain=17), 'gain outside')
    refused(plan(max_predict=-1), 'max_predict outside')
    refused(plan(max_predict=256), 'max_predict outside')
    refused(plan(new_gate=0), 'new_gate outside')
    refused(plan(new_gate=17), 'new_gate outside')


def test_wrappers_raise_value_errors_on_host_tensors():
    from pavenet_amd import ops
    from pavenet_amd.tracking import PoseTracker
    cv = 'constant_velocity'
    t = PoseTracker(15, motion=cv)
    assert (t.motion, t.velocity_gain, t.max_predict, t.new_gate) == (cv, 8, 30, 4)
    assert PoseTracker(15, motion=cv, max_age=1000).max_predict == 255
    assert PoseTracker(15, motion=cv, max_age=0).max_predict == 0
    t = PoseTracker(15, motion=cv, velocity_gain=16, max_predict=255, new_gate=16)
    assert (t.velocity_gain, t.max_predict, t.new_gate) == (16, 255, 16)
    t = PoseTracker(15, motion=cv, velocity_gain=1, max_predict=0, new_gate=1)
    assert (t.velocity_gain, t.max_predict, t.new_gate) == (1, 0, 1)
    assert PoseTracker(15).motion is None
    for call, needle in ((lambda: PoseTracker(15, motion='kalman'), 'motion is None or'),
                         (lambda: PoseTracker(15, motion=True), 'motion is None or'),
                         (lambda: PoseTracker(15, velocity_gain=8), 'velocity_gain given with motion=None'),
                         (lambda: PoseTracker(15, max_predict=30), 'max_predict given with motion=None'),
                         (lambda: PoseTracker(15, new_gate=4), 'new_gate given with motion=None'),
                         (lambda: PoseTracker(15, motion=None, velocity_gain=8, new_gate=4), 'velocity_gain, new_gate'),
                         (lambda: PoseTracker(15, motion=cv, velocity_gain=0), 'velocity_gain is an integer'),
                         (lambda: PoseTracker(15, motion=cv, velocity_gain=17), 'velocity_gain is an integer'),
                         (lambda: PoseTracker(15, motion=cv, velocity_gain=8.0), 'velocity_gain is an integer'),
                         (lambda: PoseTracker(15, motion=cv, max_predict=-1), 'max_predict is an integer'),
                         (lambda: PoseTracker(15, motion=cv, max_predict=256), 'max_predict is an integer'),
                         (lambda: PoseTracker(15, motion=cv, new_gate=0), 'new_gate is an integer'),
                         (lambda: PoseTracker(15, motion=cv, new_gate=17), 'new_gate is an integer'),
                         (lambda: PoseTracker(15, motion=cv, new_gate=True), 'new_gate is an integer')):
        with pytest.raises(ValueError, match=needle):
            call()
    # the update's own checks come first, and nothing is allocated by a refused call
    kp, bb = torch.zeros(3, 15, 3), torch.zeros(3, 5)
    t = PoseTracker(15, motion=cv)
    with pytest.raises(ValueError, match='HIP device'):
        t.update((bb, None, kp))
    assert t._state is None and t.state(0) is None

    def state(cameras=2, M=8, K=15):
        z = dict(dtype=torch.int32)
        return dict(id=torch.zeros(cameras, M, **z), last=torch.zeros(cameras, M, **z), vis=torch.zeros(cameras, M, **z),
                    area=torch.zeros(cameras, M, **z), kpts=torch.zeros(cameras, M, K, 2, **z),
                    frame=torch.zeros(cameras, **z), next_id=torch.ones(cameras, **z), dropped=torch.zeros(cameras, **z))
    scratch = torch.empty((32, 128, 128), dtype=torch.int64)
    vel, hits = torch.zeros(2, 8, 2, dtype=torch.int32), torch.zeros(2, 8, dtype=torch.int32)

    def track(*motion, **named):
        if named:
            motion = dict(dict(vel=vel, hits=hits, gain=8, max_predict=30, new_gate=4), **named)
        return ops.track_poses([(kp, bb, None, 0, (1.0, 1.0))], state(), scratch, C15, min_kpts=5, motion=motion)
    for call, needle in (
            (lambda: track(vel, hits, 8, 30), 'motion is None or'),
            (lambda: ops.track_poses([], state(), scratch, C15, min_kpts=5, motion=dict(vel=vel, hits=hits)),
             'motion holds'),
            (lambda: ops.track_poses([], state(), scratch, C15, min_kpts=5, motion=7), 'motion is None or'),
            (lambda: track(vel=vel.numpy()), 'motion vel'),
            (lambda: track(vel=vel.long()), 'motion vel'),
            (lambda: track(vel=vel[:, :, :1]), 'motion vel'),
            (lambda: track(vel=torch.zeros(2, 2, 8, dtype=torch.int32).transpose(1, 2)), 'motion vel'),
            (lambda: track(vel=torch.zeros(2, 9, 2, dtype=torch.int32)), 'motion vel'),
            (lambda: track(hits=hits.float()), 'motion hits'),
            (lambda: track(hits=hits[:1]), 'motion hits'),
            (lambda: track(hits=None), 'motion hits'),
            (lambda: track(gain=0), 'motion gain'),
            (lambda: track(gain=17), 'motion gain'),
            (lambda: track(gain=8.5), 'motion gain'),
            (lambda: track(max_predict=-1), 'motion max_predict'),
            (lambda: track(max_predict=256), 'motion max_predict'),
            (lambda: track(new_gate=0), 'motion new_gate'),
            (lambda: track(new_gate=17), 'motion new_gate'),
            (lambda: track(vel, hits, 8, 30, 4), 'HIP device'),
            (lambda: track(gain=8), 'HIP device')):
        with pytest.raises(ValueError, match=needle):
            call()
