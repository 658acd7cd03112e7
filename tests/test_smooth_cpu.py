"""Steady poses, the parts that need no GPU: what the rule of DESIGN section 16 (tests/smooth_ref.py) buys on jittering
people, its arithmetic edges as hand-worked scripts (tests/smooth_cases.py), the plan's C layout, and every refusal
of the C entry point and of the Python wrappers."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import smooth_cases as SC
from tests import smooth_ref as SR
from tests.test_track_cpu import FIGURE, walk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rms_errors(height, step, frames=60, first=16, people=6):
    """The walk of tests/test_track_cpu.py (1 % jitter) with person p under id p + 1 through the oracle at its
    defaults -> (raw, smoothed): the RMS distance per coordinate of the key points from the noiseless figure over
    frames `first` .. `frames` (counted from 1), in per cent of the height."""
    ref = SR.SmoothRef(15)
    raw, smooth = [], []
    for f, (kpts, bboxes, who) in enumerate(walk(height, step, frames=frames, people=people, seed=height * 10 + step)):
        out, _ = ref.smooth(kpts, bboxes, who + 1)
        if f + 1 < first:
            continue
        truth = np.stack([FIGURE * height + (100.0 + 400.0 * p + step * f, 50.0 + 7.0 * p) for p in who])
        raw.append(kpts[..., :2].astype(np.float64) - truth)
        smooth.append(out[..., :2].astype(np.float64) - truth)
    assert ref.dropped[0] == 0 and (ref.id[0] != 0).sum() == people
    return tuple(100.0 * np.sqrt(np.mean(np.square(v))) / height for v in (raw, smooth))


@pytest.mark.parametrize('height', [40, 100, 300])
def test_a_standing_person_jitters_less_than_half_as_much(height):
    raw, smooth = rms_errors(height, 0)
    print(f'height {height} step 0: raw {raw:.3f} % smoothed {smooth:.3f} % ratio {smooth / raw:.3f}')
    assert smooth <= 0.5 * raw


@pytest.mark.parametrize('height', [40, 100, 300])
@pytest.mark.parametrize('step', [1, 2, 4, 8])
def test_a_walking_person_is_not_held_back(height, step):
    raw, smooth = rms_errors(height, step)
    print(f'height {height} step {step}: raw {raw:.3f} % smoothed {smooth:.3f} % ratio {smooth / raw:.3f}')
    assert smooth <= 1.1 * raw


class OracleHarness:
    """tests/smooth_cases.py's harness on the oracle alone."""

    def __init__(self, K, **kw):
        self.ref = SR.SmoothRef(K, **kw)

    def frame(self, kpts, bboxes, ids, keep=None):
        return self.ref.smooth(kpts, bboxes, np.asarray(ids, np.int32), None if keep is None else np.asarray(keep, np.int32))

    def poke(self, field, index, value):
        getattr(self.ref, field)[(0,) + tuple(index)] = value

    def get(self, field):
        return getattr(self.ref, field)[0]


@pytest.mark.parametrize('script', SC.SCRIPTS, ids=lambda s: s.__name__)
def test_hand_worked_scripts_on_the_oracle(script):
    script(OracleHarness)


def test_defaults_and_ranges():
    import pavenet_amd
    from pavenet_amd.smoothing import PoseSmoother
    assert pavenet_amd.PoseSmoother is PoseSmoother
    s = PoseSmoother(15)
    assert (s.K, s.cameras, s.max_tracks, s.max_age, s.alpha_min, s.beta, s.velocity_gain, s.score_thr, s.kpt_thr) == \
        (15, 1, 128, 30, 32, 128, 3, 0.3, 0.0)
    r = SR.SmoothRef(15)
    assert (r.S, r.max_age, r.alpha_min, r.beta, r.g, float(r.score_thr), float(r.kpt_thr)) == \
        (128, 30, 32, 128, 3, float(np.float32(0.3)), 0.0)
    for kw in (dict(alpha_min=1), dict(alpha_min=256), dict(beta=0), dict(beta=4096), dict(velocity_gain=1),
               dict(velocity_gain=16), dict(max_tracks=1), dict(max_age=0), dict(cameras=4096)):
        PoseSmoother(32, **kw)
    for call, needle in ((lambda: PoseSmoother(0), 'K is'),
                         (lambda: PoseSmoother(33), 'K is'),
                         (lambda: PoseSmoother(15, cameras=0), 'cameras'),
                         (lambda: PoseSmoother(15, cameras=4097), 'cameras'),
                         (lambda: PoseSmoother(15, max_tracks=0), 'max_tracks'),
                         (lambda: PoseSmoother(15, max_tracks=129), 'max_tracks'),
                         (lambda: PoseSmoother(15, max_age=-1), 'max_age'),
                         (lambda: PoseSmoother(15, max_age=1.5), 'max_age'),
                         (lambda: PoseSmoother(15, alpha_min=0), 'alpha_min'),
                         (lambda: PoseSmoother(15, alpha_min=257), 'alpha_min'),
                         (lambda: PoseSmoother(15, alpha_min=32.0), 'alpha_min'),
                         (lambda: PoseSmoother(15, beta=-1), 'beta'),
                         (lambda: PoseSmoother(15, beta=4097), 'beta'),
                         (lambda: PoseSmoother(15, velocity_gain=0), 'velocity_gain'),
                         (lambda: PoseSmoother(15, velocity_gain=17), 'velocity_gain'),
                         (lambda: PoseSmoother(15, velocity_gain=True), 'velocity_gain')):
        with pytest.raises(ValueError, match=needle):
            call()


def _lib():
    from pavenet_amd import native
    from pavenet_amd.build_native import build_native
    build_native()
    return native, native.load()


def test_smooth_plan_layout_and_entry(tmp_path):
    """native.SmoothPlan is the header's pave_smooth_plan field for field, 2136 bytes (under the 4 KB
    kernel-argument limit), and the entry is in the header, the binding and both libraries at ABI 21."""
    native, lib = _lib()
    vp, ci = ctypes.c_void_p, ctypes.c_int
    assert native.FUNCTIONS['pave_smooth_poses'] == (ci, [vp, vp]) and 'pave_smooth_poses' in native.SIGNATURES
    assert hasattr(lib, 'pave_smooth_poses')
    for path in (native.LIB_PATH, native.DIAG_LIB_PATH):
        out = subprocess.run(['nm', '-D', '--defined-only', path], capture_output=True, text=True, check=True).stdout
        assert 'pave_smooth_poses' in {ln.split()[-1] for ln in out.splitlines()}
    assert native.ABI_VERSION == 21 and lib.pave_abi_version() == 21
    assert ctypes.sizeof(native.SmoothPlan) == 2136 <= 4096
    if not shutil.which('gcc'):
        pytest.skip('no gcc')
    fields = [f for f, _ in native.SmoothPlan._fields_]
    src = tmp_path / 'layout.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pave_hip.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(pave_smooth_plan));\n'
                   + ''.join(f'  printf(" %zu", offsetof(pave_smooth_plan, {f}));\n' for f in fields)
                   + '  return 0;\n}\n')
    exe = tmp_path / 'layout'
    subprocess.run(['gcc', '-std=c99', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == ctypes.sizeof(native.SmoothPlan)
    assert got[1:] == [getattr(native.SmoothPlan, f).offset for f in fields]


STATE_FIELDS = ('slot_id', 'slot_last', 'slot_pos', 'slot_vel', 'frame', 'dropped')


def test_c_entry_refuses_bad_plans_before_any_device_call():
    """No GPU: every refusal is PAVE_E_ARG with a message (the addresses are never dereferenced)."""
    native, lib = _lib()
    host = (ctypes.c_ubyte * 64)()
    addr = ctypes.addressof(host)

    def plan(entries=2, n=3, K=15, S=8, cameras=2, camera=1, scale=(1.0, 1.0), alpha_min=32, beta=128,
             velocity_gain=3, max_age=30, kpts=addr, bboxes=addr, ids=addr, keep=None, out_kpts=addr, out_bboxes=addr,
             **state):
        p = native.SmoothPlan()
        for i in range(min(max(entries, 0), 32)):
            p.kpts[i], p.bboxes[i], p.ids[i], p.keep[i] = kpts, bboxes, ids, keep
            p.out_kpts[i], p.out_bboxes[i] = out_kpts, out_bboxes
            p.n[i], p.camera[i], p.scale[i][0], p.scale[i][1] = n, camera, scale[0], scale[1]
        for f in STATE_FIELDS:
            setattr(p, f, state.get(f, addr))
        p.entries, p.cameras, p.S, p.K, p.max_age = entries, cameras, S, K, max_age
        p.alpha_min, p.beta, p.velocity_gain = alpha_min, beta, velocity_gain
        p.score_thr, p.kpt_thr = 0.3, 0.0
        return p

    def refused(p, needle):
        assert lib.pave_smooth_poses(ctypes.byref(p) if p is not None else None, None) == native.DEFINES['PAVE_E_ARG'] == -1
        assert needle in lib.pave_last_error().decode(), lib.pave_last_error()

    refused(None, 'null plan')
    refused(plan(entries=0), 'frames per launch')
    refused(plan(entries=33), 'frames per launch')
    refused(plan(kpts=None), 'null pose')
    refused(plan(bboxes=None), 'null pose')
    refused(plan(ids=None), 'null ids')
    refused(plan(out_kpts=None), 'null output')
    refused(plan(out_bboxes=None), 'null output')
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
    refused(plan(alpha_min=0), 'alpha_min')
    refused(plan(alpha_min=257), 'alpha_min')
    refused(plan(beta=-1), 'beta')
    refused(plan(beta=4097), 'beta')
    refused(plan(velocity_gain=0), 'velocity_gain')
    refused(plan(velocity_gain=17), 'velocity_gain')
    refused(plan(max_age=-1), 'max_age')


def test_wrappers_raise_value_errors_on_host_tensors():
    """Shape, type and range checks, and the host-tensor check itself, are ValueErrors raised before anything is
    allocated on or asked of a device."""
    from pavenet_amd import ops
    from pavenet_amd.smoothing import PoseSmoother
    kp, bb, keep = torch.zeros(3, 15, 3), torch.zeros(3, 5), torch.ones(3, dtype=torch.int32)
    ids = torch.ones(3, dtype=torch.int32)
    res = (bb, None, kp)
    sm = PoseSmoother(15, cameras=2)
    for call, needle in (
            (lambda: sm.smooth((bb, kp), ids), 'tuple'),
            (lambda: sm.smooth(dict(bboxes=bb), ids), 'bboxes and kpts'),
            (lambda: sm.smooth((bb.numpy(), None, kp), ids), 'tensor'),
            (lambda: sm.smooth((bb[:2], None, kp), ids), 'bboxes'),
            (lambda: sm.smooth((bb.double(), None, kp), ids), 'float32'),
            (lambda: sm.smooth(dict(bboxes=bb, kpts=kp, keep=keep.long()), ids), 'int32'),
            (lambda: sm.smooth((torch.zeros(129, 5), None, torch.zeros(129, 15, 3)), torch.zeros(129, dtype=torch.int32)),
             'at most 128'),
            (lambda: sm.smooth((bb, None, torch.zeros(3, 17, 3)), ids), 'K = 17'),
            (lambda: sm.smooth(res, ids.long()), 'ids of results'),
            (lambda: sm.smooth(res, ids[:2]), 'ids of results'),
            (lambda: sm.smooth(res, [1, 2, 3]), 'ids of results'),
            (lambda: sm.smooth(res, ids, camera=2), 'camera'),
            (lambda: sm.smooth(res, ids, camera=0.5), 'camera'),
            (lambda: sm.smooth(res, ids, scale_factor=0.0), 'positive'),
            (lambda: sm.smooth(res, ids, scale_factor=(1.0, float('nan'))), 'positive'),
            (lambda: sm.smooth_many([(0, res, ids), (1, res, ids)], scale_factor=[1.0, 1.0, 1.0]), 'scale_factor'),
            (lambda: sm.smooth_many([(0, res)]), 'triples'),
            (lambda: sm.smooth(res, ids), 'HIP device'),
            (lambda: sm.reset(camera=2), 'camera'),
            (lambda: sm.state(2), 'camera')):
        with pytest.raises(ValueError, match=needle):
            call()
    assert sm._state is None and sm.state(0) is None and sm.smooth_many([]) == []
    sm.reset()

    def state(cameras=2, S=8, K=15, **over):
        z = dict(dtype=torch.int32)
        s = dict(id=torch.zeros(cameras, S, **z), last=torch.zeros(cameras, S, **z),
                 pos=torch.zeros(cameras, S, K + 2, 2, **z), vel=torch.zeros(cameras, S, K + 2, 2, **z),
                 frame=torch.zeros(cameras, **z), dropped=torch.zeros(cameras, **z))
        s.update(over)
        return s

    def smooth(entries=((kp, bb, None, ids, 0, (1.0, 1.0)),), st=None, **kw):
        return ops.smooth_poses(entries, state() if st is None else st, **kw)
    for call, needle in (
            (lambda: smooth(st=dict(id=bb)), 'state holds'),
            (lambda: smooth(st=state(pos=torch.zeros(2, 8, 17, 3, dtype=torch.int32))), 'state pos'),
            (lambda: smooth(st=state(S=129)), 'S in'),
            (lambda: smooth(st=state(K=33)), 'K'),
            (lambda: smooth(st=state(vel=torch.zeros(2, 8, 17, 2))), 'state vel'),
            (lambda: smooth(st=state(frame=torch.zeros(3, dtype=torch.int32))), 'state frame'),
            (lambda: smooth(alpha_min=0), 'alpha_min'),
            (lambda: smooth(alpha_min=257), 'alpha_min'),
            (lambda: smooth(beta=-1), 'beta'),
            (lambda: smooth(beta=4097), 'beta'),
            (lambda: smooth(beta=1.0), 'beta'),
            (lambda: smooth(velocity_gain=0), 'velocity_gain'),
            (lambda: smooth(velocity_gain=17), 'velocity_gain'),
            (lambda: smooth(max_age=-1), 'max_age'),
            (lambda: smooth(entries=[(kp, bb, None, ids, 0)]), 'entry 0 is'),
            (lambda: smooth(entries=[(kp[:, :14], bb, None, ids, 0, (1, 1))]), 'kpts of entry 0'),
            (lambda: smooth(entries=[(kp, bb[:, :4], None, ids, 0, (1, 1))]), 'bboxes of entry 0'),
            (lambda: smooth(entries=[(kp, bb, keep.long(), ids, 0, (1, 1))]), 'keep of entry 0'),
            (lambda: smooth(entries=[(kp, bb, None, ids.long(), 0, (1, 1))]), 'ids of entry 0'),
            (lambda: smooth(entries=[(kp, bb, None, None, 0, (1, 1))]), 'ids of entry 0'),
            (lambda: smooth(entries=[(kp, bb, None, ids, 2, (1, 1))]), 'camera of entry 0'),
            (lambda: smooth(entries=[(kp, bb, None, ids, 0, (1, 1)), (kp, bb, None, ids, 0, (1, 0))]), 'scale of entry 1'),
            (lambda: smooth(entries=[(kp, bb, None, ids, 0, 1.0)]), 'scale of entry 0'),
            (lambda: smooth(entries=[(kp.transpose(0, 1).contiguous().transpose(0, 1), bb, None, ids, 0, (1, 1))]),
             'contiguous'),
            (lambda: smooth(), 'HIP device')):
        with pytest.raises(ValueError, match=needle):
            call()
