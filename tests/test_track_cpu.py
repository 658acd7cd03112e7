"""Track ids, the parts that need no GPU: the rule of DESIGN section 14 (tests/track_ref.py) on walking people, the
host constants, the plan's C layout, every refusal of the C entry point and of the Python wrappers, and the PoseTrack
output format."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import track_ref as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C15 = [1965, 18144, 18144, 18144, 18144, 15071, 15071, 11176, 11176, 33285, 33285, 22005, 22005, 23028, 23028]

# a standing figure in a box 0.4 wide and 1 high, PoseTrack order (nose, head bottom, head top, then left / right
# shoulder, elbow, wrist, hip, knee, ankle)
FIGURE = np.asarray([(.20, .08), (.20, .14), (.20, .00), (.05, .20), (.35, .20), (.00, .36), (.40, .36), (.02, .50),
                     (.38, .50), (.10, .52), (.30, .52), (.09, .76), (.31, .76), (.08, 1.0), (.32, 1.0)], np.float64)


def walk(height, step, frames=40, people=6, seed=0):
    """`people` figures `height` px tall, 400 px apart, each walking `step` px per frame to the right with a jitter
    of 1 % of the height on every coordinate; the detections of every frame in a shuffled order.  Yields (kpts,
    bboxes, who): who[n] is the person detection n shows."""
    rng = np.random.default_rng(seed)
    for f in range(frames):
        kpts = np.empty((people, 15, 3), np.float32)
        for p in range(people):
            xy = FIGURE * height + (100.0 + 400.0 * p + step * f, 50.0 + 7.0 * p)
            kpts[p, :, :2] = xy + rng.uniform(-0.01, 0.01, xy.shape) * height
            kpts[p, :, 2] = 0.9
        who = rng.permutation(people)
        kpts = kpts[who]
        bboxes = np.concatenate([kpts[..., 0].min(1, keepdims=True), kpts[..., 1].min(1, keepdims=True),
                                 kpts[..., 0].max(1, keepdims=True), kpts[..., 1].max(1, keepdims=True),
                                 np.full((people, 1), 0.8, np.float32)], 1).astype(np.float32)
        yield kpts, bboxes, who


def run_walk(height, step):
    ref = TR.TrackRef(15)
    seen = []
    for kpts, bboxes, who in walk(height, step, seed=height * 10 + step):
        ids = ref.update(kpts, bboxes)
        by_person = np.empty(6, np.int64)
        by_person[who] = ids
        seen.append(by_person)
    return np.stack(seen), ref


@pytest.mark.parametrize('height', [40, 100, 300])
@pytest.mark.parametrize('step', [1, 2, 4])
def test_walking_people_keep_their_ids(height, step):
    """Six people, shuffled on every frame, keep six ids for 40 frames under the defaults."""
    seen, ref = run_walk(height, step)
    assert sorted(seen[0]) == [1, 2, 3, 4, 5, 6]
    assert (seen == seen[0]).all()
    assert ref.next_id[0] == 7 and ref.dropped[0] == 0 and ref.frame[0] == 40
    assert (ref.id[0] != 0).sum() == 6


def test_the_rule_is_not_vacuous():
    """8 px per frame at 40 px height: no key point stays within its OKS distance (the widest, sigma .107, allows
    about 6.4 px on this figure), so the links break, as OKS linking at 0.5 must."""
    seen, ref = run_walk(40, 8)
    assert ref.next_id[0] > 7
    assert not (seen == seen[0]).all()


def test_pair_constants_and_host_refusals():
    from pavenet_amd import native
    from pavenet_amd.heads import OKS_SIGMAS_POSETRACK15
    from pavenet_amd.tracking import SIGMAS, PoseTracker, pair_constants
    assert PoseTracker(15).C == C15 == TR.pair_constants(TR.POSETRACK_SIGMAS)
    assert np.allclose(SIGMAS[15], np.asarray(OKS_SIGMAS_POSETRACK15) / 10)
    for K in (14, 15, 17):
        t = PoseTracker(K)
        assert np.allclose(SIGMAS[K], TR.SIGMAS[K]) and t.C == TR.pair_constants(TR.SIGMAS[K]) and len(t.C) == K
        assert t.min_kpts == max(1, (K + 2) // 3) == TR.default_min_kpts(K)
        assert all(1 <= c < 1 << 24 for c in t.C)
    assert PoseTracker(15, match_thr=0.75).C == TR.pair_constants(TR.POSETRACK_SIGMAS, 0.75)
    assert PoseTracker(2, sigmas=[1e-6, 0.05]).C[0] == 1
    assert (native.TRACK_MAX_FRAMES, native.TRACK_MAX_POSES, native.TRACK_MAX_TRACKS, native.TRACK_MAX_K) == \
        (32, 128, 128, 32)
    for bad in (0.0, 1.0, -0.5, 1.5, float('nan')):
        with pytest.raises(ValueError, match='match_thr'):
            PoseTracker(15, match_thr=bad)
        with pytest.raises(ValueError, match='match_thr'):
            pair_constants([0.05], bad)
    for call, needle in ((lambda: PoseTracker(16), 'sigmas'),
                         (lambda: PoseTracker(0, sigmas=[]), 'K in'),
                         (lambda: PoseTracker(33, sigmas=[0.05] * 33), 'K in'),
                         (lambda: PoseTracker(15, sigmas=[0.05] * 14), 'one sigma'),
                         (lambda: PoseTracker(2, sigmas=[0.05, -1.0]), 'positive'),
                         (lambda: PoseTracker(2, sigmas=[0.05, 5.0], match_thr=0.01), '2\\^24'),
                         (lambda: PoseTracker(15, cameras=0), 'cameras'),
                         (lambda: PoseTracker(15, max_tracks=0), 'max_tracks'),
                         (lambda: PoseTracker(15, max_tracks=129), 'max_tracks'),
                         (lambda: PoseTracker(15, max_age=-1), 'max_age'),
                         (lambda: PoseTracker(15, min_kpts=0), 'min_kpts'),
                         (lambda: PoseTracker(15, min_kpts=16), 'min_kpts')):
        with pytest.raises(ValueError, match=needle):
            call()


def _lib():
    from pavenet_amd import native
    from pavenet_amd.build_native import build_native
    build_native()
    return native, native.load()


def test_track_plan_layout_and_entry(tmp_path):
    """native.TrackPlan is the header's pave_track_plan field for field, fits the 4 KB kernel-argument limit, and
    the entry is in the header, the binding and both libraries at ABI 21."""
    native, lib = _lib()
    vp, ci = ctypes.c_void_p, ctypes.c_int
    assert native.FUNCTIONS['pave_track_poses'] == (ci, [vp, vp]) and 'pave_track_poses' in native.SIGNATURES
    assert hasattr(lib, 'pave_track_poses')
    for path in (native.LIB_PATH, native.DIAG_LIB_PATH):
        out = subprocess.run(['nm', '-D', '--defined-only', path], capture_output=True, text=True, check=True).stdout
        assert 'pave_track_poses' in {ln.split()[-1] for ln in out.splitlines()}
    assert native.ABI_VERSION == 21 and lib.pave_abi_version() == 21
    assert ctypes.sizeof(native.TrackPlan) <= 4096
    if not shutil.which('gcc'):
        pytest.skip('no gcc')
    fields = [f for f, _ in native.TrackPlan._fields_]
    src = tmp_path / 'layout.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pave_hip.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(pave_track_plan));\n'
                   + ''.join(f'  printf(" %zu", offsetof(pave_track_plan, {f}));\n' for f in fields)
                   + '  return 0;\n}\n')
    exe = tmp_path / 'layout'
    subprocess.run(['gcc', '-std=c99', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == ctypes.sizeof(native.TrackPlan)
    assert got[1:] == [getattr(native.TrackPlan, f).offset for f in fields]


STATE_FIELDS = ('track_id', 'track_last', 'track_kpts', 'track_vis', 'track_area', 'frame', 'next_id', 'dropped')


def test_c_entry_refuses_bad_plans_before_any_device_call():
    """No GPU: every refusal is PAVE_E_ARG with a message (the addresses are never dereferenced)."""
    native, lib = _lib()
    host = (ctypes.c_ubyte * 64)()
    addr = ctypes.addressof(host)

    def plan(entries=2, n=3, K=15, M=8, cameras=2, camera=1, scale=(1.0, 1.0), C=1000, min_kpts=5, max_age=30,
             kpts=addr, bboxes=addr, ids=addr, keep=None, scratch=addr, **state):
        p = native.TrackPlan()
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
        return p

    def refused(p, needle):
        assert lib.pave_track_poses(ctypes.byref(p) if p is not None else None, None) == native.DEFINES['PAVE_E_ARG'] == -1
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


def test_wrappers_raise_value_errors_on_host_tensors():
    """Shape, type and range checks, and the host-tensor check itself, are ValueErrors raised before anything is
    allocated on or asked of a device."""
    import pavenet_amd
    from pavenet_amd import ops
    from pavenet_amd.tracking import PoseTracker
    assert pavenet_amd.PoseTracker is PoseTracker
    kp, bb, keep = torch.zeros(3, 15, 3), torch.zeros(3, 5), torch.ones(3, dtype=torch.int32)
    res = (bb, None, kp)
    tracker = PoseTracker(15, cameras=2)
    for call, needle in (
            (lambda: tracker.update((bb, kp)), 'tuple'),
            (lambda: tracker.update(dict(bboxes=bb)), 'bboxes and kpts'),
            (lambda: tracker.update((bb.numpy(), None, kp)), 'tensor'),
            (lambda: tracker.update((bb[:2], None, kp)), 'bboxes'),
            (lambda: tracker.update((bb, None, kp[..., :2])), 'kpts'),
            (lambda: tracker.update((bb.double(), None, kp)), 'float32'),
            (lambda: tracker.update(dict(bboxes=bb, kpts=kp, keep=keep.long())), 'int32'),
            (lambda: tracker.update(dict(bboxes=bb, kpts=kp, keep=keep[:2])), 'int32'),
            (lambda: tracker.update((torch.zeros(129, 5), None, torch.zeros(129, 15, 3))), 'at most 128'),
            (lambda: tracker.update((bb, None, torch.zeros(3, 17, 3))), 'K = 17'),
            (lambda: tracker.update(res, camera=2), 'camera'),
            (lambda: tracker.update(res, camera=-1), 'camera'),
            (lambda: tracker.update(res, camera=0.5), 'camera'),
            (lambda: tracker.update(res, scale_factor=0.0), 'positive'),
            (lambda: tracker.update(res, scale_factor=(1.0, 2.0, 3.0)), 'scale'),
            (lambda: tracker.update(res, scale_factor=(1.0, float('nan'))), 'positive'),
            (lambda: tracker.update_many([(0, res), (1, res)], scale_factor=[1.0, 1.0, 1.0]), 'scale_factor'),
            (lambda: tracker.update_many([res]), 'pairs'),
            (lambda: tracker.update(res), 'HIP device'),
            (lambda: tracker.update(dict(bboxes=bb[None], kpts=kp[None], keep=keep[None])), 'HIP device'),
            (lambda: tracker.reset(camera=2), 'camera'),
            (lambda: tracker.state(2), 'camera')):
        with pytest.raises(ValueError, match=needle):
            call()
    assert tracker._state is None and tracker.state(0) is None and tracker.update_many([]) == []
    tracker.reset()

    # ops.track_poses on a host state: everything but the device is checked first
    def state(cameras=2, M=8, K=15, **over):
        z = dict(dtype=torch.int32)
        s = dict(id=torch.zeros(cameras, M, **z), last=torch.zeros(cameras, M, **z), vis=torch.zeros(cameras, M, **z),
                 area=torch.zeros(cameras, M, **z), kpts=torch.zeros(cameras, M, K, 2, **z),
                 frame=torch.zeros(cameras, **z), next_id=torch.ones(cameras, **z), dropped=torch.zeros(cameras, **z))
        s.update(over)
        return s
    scratch = torch.empty(1).new_empty((32, 128, 128), dtype=torch.int64)

    def track(entries=((kp, bb, None, 0, (1.0, 1.0)),), st=None, scr=scratch, C=C15, min_kpts=5, **kw):
        return ops.track_poses(entries, state() if st is None else st, scr, C, min_kpts=min_kpts, **kw)
    for call, needle in (
            (lambda: track(st=dict(id=bb)), 'state holds'),
            (lambda: track(st=state(kpts=torch.zeros(2, 8, 15, 3, dtype=torch.int32))), 'state kpts'),
            (lambda: track(st=state(M=129)), 'M in'),
            (lambda: track(st=state(K=33), C=[5] * 33), 'K'),
            (lambda: track(st=state(vis=torch.zeros(2, 8))), 'state vis'),
            (lambda: track(st=state(frame=torch.zeros(3, dtype=torch.int32))), 'state frame'),
            (lambda: track(scr=scratch[:16]), 'scratch'),
            (lambda: track(scr=scratch.int()), 'scratch'),
            (lambda: track(C=C15[:14]), 'pair constants'),
            (lambda: track(C=[0] * 15), 'pair constants'),
            (lambda: track(C=[1 << 24] * 15), 'pair constants'),
            (lambda: track(min_kpts=0), 'min_kpts'),
            (lambda: track(min_kpts=16), 'min_kpts'),
            (lambda: track(max_age=-1), 'max_age'),
            (lambda: track(entries=[(kp, bb, None, 0)]), 'entry 0 is'),
            (lambda: track(entries=[(kp[:, :14], bb, None, 0, (1, 1))]), 'kpts of entry 0'),
            (lambda: track(entries=[(kp.double(), bb, None, 0, (1, 1))]), 'kpts of entry 0'),
            (lambda: track(entries=[(kp, bb[:, :4], None, 0, (1, 1))]), 'bboxes of entry 0'),
            (lambda: track(entries=[(kp, bb, keep.long(), 0, (1, 1))]), 'keep of entry 0'),
            (lambda: track(entries=[(torch.zeros(129, 15, 3), torch.zeros(129, 5), None, 0, (1, 1))]), 'at most 128'),
            (lambda: track(entries=[(kp, bb, None, 2, (1, 1))]), 'camera of entry 0'),
            (lambda: track(entries=[(kp, bb, None, 0, (1, 1)), (kp, bb, None, 0, (1, 0))]), 'scale of entry 1'),
            (lambda: track(entries=[(kp, bb, None, 0, (float('inf'), 1))]), 'scale of entry 0'),
            (lambda: track(entries=[(kp, bb, None, 0, 1.0)]), 'scale of entry 0'),
            (lambda: track(entries=[(kp.transpose(0, 1).contiguous().transpose(0, 1), bb, None, 0, (1, 1))]), 'contiguous'),
            (lambda: track(), 'HIP device')):
        with pytest.raises(ValueError, match=needle):
            call()


def test_posetrack_frame():
    from pavenet_amd.formats import posetrack_frame
    rng = np.random.default_rng(3)
    kp = torch.from_numpy(rng.uniform(0, 100, (4, 15, 3)).astype(np.float32))
    bb = torch.from_numpy(rng.uniform(0, 1, (4, 5)).astype(np.float32))
    ids = torch.tensor([7, 0, 2, 9], dtype=torch.int32)
    for result in ((bb, None, kp), dict(bboxes=bb[None], kpts=kp[None], keep=torch.ones(1, 4, dtype=torch.int32))):
        frame = posetrack_frame('images/val/000342_mpii_test/00000012.jpg', 12, result, ids)
        assert list(frame) == ['image', 'imgnum', 'annorect']
        assert frame['image'] == {'name': 'images/val/000342_mpii_test/00000012.jpg'} and frame['imgnum'] == [12]
        assert [r['track_id'] for r in frame['annorect']] == [[7], [2], [9]]
        for r, p in zip(frame['annorect'], (0, 2, 3)):
            assert list(r) == ['annopoints', 'score', 'track_id'] and r['score'] == [float(bb[p, 4])]
            assert len(r['annopoints']) == 1 and list(r['annopoints'][0]) == ['point']
            points = r['annopoints'][0]['point']
            assert len(points) == 15
            for k, pt in enumerate(points):
                assert list(pt) == ['id', 'x', 'y', 'score']
                assert pt == {'id': [k], 'x': [float(kp[p, k, 0])], 'y': [float(kp[p, k, 1])],
                              'score': [float(kp[p, k, 2])]}
    import json
    json.dumps(frame)
    assert posetrack_frame('a.jpg', 1, (bb, None, kp), [0, 0, 0, 0])['annorect'] == []
    with pytest.raises(ValueError, match='ids'):
        posetrack_frame('a.jpg', 1, (bb, None, kp), ids[:3])
