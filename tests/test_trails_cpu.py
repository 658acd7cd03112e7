"""Track trails, the parts that need no GPU: the edges of the update rule of DESIGN section 22 as hand-worked scripts on
its numpy statement (tests/trail_cases.py on tests/trail_ref.py), the committed points against section 17's pos, how
often a standing person commits, both plans' C layout, every refusal of the C entry points and of the Python calls,
and the exports."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import trail_cases as TC
from tests import trail_ref as TR
from tests.test_heat_cpu import layout
from tests.test_track_cpu import walk
from tests.zones_ref import ZoneRef


class OracleHarness:
    """tests/trail_cases.py's harness on the oracle alone."""

    def __init__(self, K, **kw):
        self.ref = TR.TrailRef(K, **kw)

    def frame(self, kpts, bboxes, ids, keep=None, camera=0):
        ids = np.asarray(ids, np.int64).astype(np.int32)
        out = self.ref.update(kpts, bboxes, ids, None if keep is None else np.asarray(keep, np.int32), camera=camera)
        TC.invariant(self.ref.drawn(camera), self.ref.L, self.ref.stride, self.ref.min_step, out, ids)
        return out

    def get(self, field, camera=0):
        return self.ref.drawn(camera)[field]


@pytest.mark.parametrize('script', TC.SCRIPTS, ids=lambda s: s.__name__)
def test_hand_worked_scripts_on_the_oracle(script):
    script(OracleHarness)


def test_committed_points_are_the_zone_monitors_pos():
    """min_step 0, stride 1, length 64: every frame commits, so after 64 frames of six walkers a slot's ring is, oldest
    first, the pos section 17's statement had for that slot in those frames."""
    ref, zone = TR.TrailRef(15, length=64, stride=1, min_step=0), ZoneRef(15)
    seen = []
    for kpts, bboxes, who in walk(100, 3, frames=64, people=6, seed=5):
        ref.update(kpts, bboxes, who + 1)
        zone.update(kpts, bboxes, who + 1)
        seen.append(zone.pos[0].copy())
    assert (ref.id[0] != 0).sum() == 6 and (ref.id[0] == zone.id[0]).all()
    for t in np.nonzero(ref.id[0])[0]:
        ring = TR.committed(ref.pts[0, t], ref.when[0, t], ref.head[0, t], ref.count[0, t])
        assert [p[:2] for p in ring] == [tuple(int(v) for v in s[t]) for s in seen]
        assert [p[2] for p in ring] == list(range(1, 65)) and ref.head[0, t] == 63


@pytest.mark.parametrize('height', [40, 100, 300])
def test_how_often_a_standing_person_commits(height):
    """A measurement, printed for DESIGN section 22 and not asserted beyond what the rule guarantees: six people
    standing for 100 frames with 1 % jitter on every coordinate; commits per person per 100 frames after the birth's.
    What the rule guarantees: min_step 0 commits every frame, and a larger min_step never commits more often."""
    per = []
    for min_step in (0, 8, 16, 32):
        ref = TR.TrailRef(15, length=64, min_step=min_step)
        commits = 0
        for kpts, bboxes, who in walk(height, 0, frames=100, people=6, seed=height):
            before = ref.when[0].copy(), ref.head[0].copy()
            ref.update(kpts, bboxes, who + 1)
            commits += int(((ref.when[0] != before[0]).any(1) | (ref.head[0] != before[1])).sum())
        per.append((commits - 6) / 6)
        print(f'height {height} min_step {min_step}: {per[-1]:.1f} commits per person per 100 frames')
    assert per[0] == 99 and per == sorted(per, reverse=True)


def test_defaults_ranges_and_exports():
    import pavenet_amd
    from pavenet_amd import TrackTrails, TrailStyle, draw_trails_bgr, draw_trails_nv12, native, render, trails
    assert TrackTrails is trails.TrackTrails and TrailStyle is trails.TrailStyle
    assert draw_trails_nv12 is trails.draw_trails_nv12 and draw_trails_bgr is trails.draw_trails_bgr
    assert pavenet_amd.TrackTrails is TrackTrails
    m = TrackTrails(17)
    assert (m.cameras, m.max_tracks, m.max_age, m.length, m.stride, m.min_step, m.anchor, m.anchor_kpts) == \
        (1, 128, 30, 32, 1, 16, 'feet', (15, 16))
    assert m.score_thr == pytest.approx(0.3) and m.kpt_thr == 0.0
    assert m.state(0) is None and m.points(0) is None and m.device_tensors() is None and m.update_many([]) == []
    m.reset()
    assert TrackTrails(15, anchor='box', anchor_kpts=(1, 2)).anchor_kpts == ()
    assert (native.TRAIL_MAX_POINTS, native.TRAIL_MAX_STRIDE, native.TRAIL_MAX_STEP) == (64, 255, 65535)
    for kw in (dict(length=1), dict(length=64), dict(stride=255), dict(min_step=0), dict(min_step=65535)):
        TrackTrails(15, **kw)
    for kw, needle in ((dict(K=0), 'K is'), (dict(K=33), 'K is'), (dict(cameras=0), 'cameras'), (dict(cameras=4097), 'cameras'),
                       (dict(max_tracks=0), 'max_tracks'), (dict(max_tracks=129), 'max_tracks'), (dict(max_age=-1), 'max_age'),
                       (dict(length=0), 'length'), (dict(length=65), 'length'), (dict(length=32.0), 'length'),
                       (dict(stride=0), 'stride'), (dict(stride=256), 'stride'), (dict(stride=True), 'stride'),
                       (dict(min_step=-1), 'min_step'), (dict(min_step=65536), 'min_step'), (dict(min_step=1.5), 'min_step'),
                       (dict(anchor='toes'), 'anchor'), (dict(K=5), 'anchor_kpts'),
                       (dict(anchor_kpts=(0, 1, 2, 3, 4)), 'at most 4'), (dict(anchor_kpts=(15,)), 'anchor_kpts')):
        args = dict(K=15)
        args.update(kw)
        with pytest.raises(ValueError, match=needle):
            TrackTrails(**args)
    s = TrailStyle()
    assert (s.thickness, s.thickness_tail, s.head_radius, s.tail_frames, s.linger) == (3, 1, 0, None, None)
    assert s.palette == [tuple(c) for c in render.TRACK_PALETTE]
    from tests.render_ref import bgr_to_yuv
    assert s.palette_bytes() == np.asarray(s.palette, np.uint8).tobytes() and len(s.palette_bytes()) == 96
    assert trails.MODES == [('bt601', False), ('bt601', True), ('bt709', False), ('bt709', True)]
    for matrix, full in trails.MODES:
        assert s.palette_bytes(matrix, full) == np.asarray([bgr_to_yuv(c, matrix, full) for c in s.palette], np.uint8).tobytes()
    for kw in (dict(thickness=32, thickness_tail=32), dict(head_radius=32), dict(tail_frames=1), dict(tail_frames=2 ** 30),
               dict(linger=0), dict(linger=2 ** 30)):
        TrailStyle(**kw)
    for kw, needle in ((dict(palette=[(0, 0, 0)] * 31), '32'), (dict(palette=7), '32'),
                       (dict(palette=[(0, 0, 256)] * 32), 'palette colour'), (dict(thickness=0), 'thickness'),
                       (dict(thickness=33), 'thickness'), (dict(thickness_tail=0), 'thickness_tail'),
                       (dict(thickness=2, thickness_tail=3), 'thickness_tail'), (dict(thickness=2.0), 'thickness'),
                       (dict(head_radius=-1), 'head_radius'), (dict(head_radius=33), 'head_radius'),
                       (dict(tail_frames=0), 'tail_frames'), (dict(tail_frames=2 ** 30 + 1), 'tail_frames'),
                       (dict(tail_frames=1.0), 'tail_frames'), (dict(linger=-1), 'linger'), (dict(linger=2 ** 30 + 1), 'linger')):
        with pytest.raises(ValueError, match=needle):
            TrailStyle(**kw)


def _lib():
    from pavenet_amd import native
    from pavenet_amd.build_native import build_native
    build_native()
    return native, native.load()


def test_trail_plan_layouts_and_entries(tmp_path):
    """native.TrailPlan and native.TrailDrawPlan are the header's structs field for field, under the 4 KB
    kernel-argument limit, and the entries are in the header, the binding and both libraries; the ABI number is the one
    it was."""
    native, lib = _lib()
    vp, ci = ctypes.c_void_p, ctypes.c_int
    names = ('pave_trail_update', 'pave_draw_trails_nv12', 'pave_draw_trails_bgr')
    for name in names:
        assert native.FUNCTIONS[name] == (ci, [vp, vp]) and name in native.SIGNATURES
    for path in (native.LIB_PATH, native.DIAG_LIB_PATH):
        out = subprocess.run(['nm', '-D', '--defined-only', path], capture_output=True, text=True, check=True).stdout
        assert set(names) <= {ln.split()[-1] for ln in out.splitlines()}
    assert native.ABI_VERSION == 21 and lib.pave_abi_version() == 21
    assert ctypes.sizeof(native.TrailPlan) == 2704 < 4096 and ctypes.sizeof(native.TrailDrawPlan) == 1296 < 4096
    if not shutil.which('gcc'):
        pytest.skip('no gcc')
    layout(tmp_path, native.TrailPlan, 'pave_trail_plan')
    layout(tmp_path, native.TrailDrawPlan, 'pave_trail_draw_plan')


STATE_FIELDS = ('slot_id', 'slot_last', 'slot_pos', 'slot_head', 'slot_count', 'slot_box', 'pts', 'when', 'frame')


def test_c_entries_refuse_bad_plans_before_any_device_call():
    """No GPU: every refusal is PAVE_E_ARG with a message (the addresses are never dereferenced)."""
    native, lib = _lib()
    host = (ctypes.c_ubyte * 64)()
    addr = ctypes.addressof(host)
    outs = ('out_count', 'out_span', 'out_dist', 'out_path')

    def plan(entries=2, n=3, K=15, S=8, L=32, cameras=2, camera=1, scale=(1.0, 1.0), max_age=30, anchor=0,
             anchor_kpts=(13, 14), stride=1, min_step=16, kpts=addr, bboxes=addr, ids=addr, keep=None, **over):
        p = native.TrailPlan()
        for i in range(min(max(entries, 0), 32)):
            p.kpts[i], p.bboxes[i], p.ids[i], p.keep[i] = kpts, bboxes, ids, keep
            for f in outs:
                getattr(p, f)[i] = over.get(f, addr)
            p.n[i], p.camera[i], p.scale[i][0], p.scale[i][1] = n, camera, scale[0], scale[1]
        for f in STATE_FIELDS + ('dropped',):
            setattr(p, f, over.get(f, addr))
        for i, k in enumerate(anchor_kpts[:4]):
            p.anchor_kpt[i] = k
        p.entries, p.cameras, p.S, p.K, p.L, p.max_age = entries, cameras, S, K, L, max_age
        p.anchor, p.n_anchor, p.stride, p.min_step = anchor, len(anchor_kpts), stride, min_step
        p.score_thr, p.kpt_thr = 0.3, 0.0
        return p

    def refused(p, needle, entry=lib.pave_trail_update):
        assert entry(ctypes.byref(p) if p is not None else None, None) == native.DEFINES['PAVE_E_ARG'] == -1
        assert needle in lib.pave_last_error().decode(), lib.pave_last_error()

    refused(None, 'null plan')
    refused(plan(entries=0), 'frames per launch')
    refused(plan(entries=33), 'frames per launch')
    refused(plan(kpts=None), 'null pose')
    refused(plan(bboxes=None), 'null pose')
    refused(plan(ids=None), 'null ids')
    for f in outs:
        refused(plan(**{f: None}), 'null output')
    for f in STATE_FIELDS + ('dropped',):
        refused(plan(**{f: None}), 'null state')
    for kw, needle in ((dict(n=-1), 'N outside'), (dict(n=129), 'N outside'), (dict(K=0), 'K outside'), (dict(K=33), 'K outside'),
                       (dict(S=0), 'max_tracks'), (dict(S=129), 'max_tracks'), (dict(cameras=0), 'cameras outside'),
                       (dict(cameras=4097), 'cameras outside'), (dict(camera=-1), 'camera index'), (dict(camera=2), 'camera index'),
                       (dict(max_age=-1), 'max_age'), (dict(L=0), 'length'), (dict(L=65), 'length'), (dict(stride=0), 'stride'),
                       (dict(stride=256), 'stride'), (dict(min_step=-1), 'min_step'), (dict(min_step=65536), 'min_step'),
                       (dict(anchor=-1), 'anchor outside'), (dict(anchor=3), 'anchor outside'),
                       (dict(anchor_kpts=(0, 1, 2, 3, 4)), 'n_anchor'), (dict(anchor_kpts=(13, 15)), 'anchor key point'),
                       (dict(K=14), 'anchor key point')):
        refused(plan(**kw), needle)
    for bad in ((0.0, 1.0), (1.0, -1.0), (float('nan'), 1.0), (1.0, float('inf'))):
        refused(plan(scale=bad), 'scale')

    def draw(n=2, width=64, height=48, pitch=192, table=0, camera=1, cameras=2, S=8, L=32, thickness=3, thickness_tail=1,
             head_radius=0, tail_frames=0, linger=-1, dst=addr, **over):
        p = native.TrailDrawPlan()
        for i in range(min(max(n, 0), 32)):
            p.dst[i], p.pitch[i], p.width[i], p.height[i], p.table[i], p.camera[i] = dst, pitch, width, height, table, camera
        for f in STATE_FIELDS:
            setattr(p, f, over.get(f, addr))
        p.n, p.cameras, p.S, p.L = n, cameras, S, L
        p.thickness, p.thickness_tail, p.head_radius, p.tail_frames, p.linger = thickness, thickness_tail, head_radius, \
            tail_frames, linger
        return p

    for entry, bpp in ((lib.pave_draw_trails_nv12, 1), (lib.pave_draw_trails_bgr, 3)):
        refused(None, 'null plan', entry)
        for kw, needle in ((dict(n=0), 'surfaces per launch'), (dict(n=33), 'surfaces per launch'), (dict(dst=None), 'null surface'),
                           (dict(width=0), 'width and height'), (dict(height=8193), 'width and height'),
                           (dict(pitch=bpp * 64 - 1), 'pitch'), (dict(table=4), 'table index'), (dict(camera=2), 'camera index'),
                           (dict(camera=-1), 'camera index'), (dict(cameras=0), 'cameras outside'), (dict(S=0), 'max_tracks'),
                           (dict(S=129), 'max_tracks'), (dict(L=0), 'length'), (dict(L=65), 'length'),
                           (dict(thickness=0), 'thickness'), (dict(thickness=33, thickness_tail=33), 'thickness'),
                           (dict(thickness_tail=0), 'thickness'), (dict(thickness=2, thickness_tail=3), 'thickness'),
                           (dict(head_radius=-1), 'head_radius'), (dict(head_radius=33), 'head_radius'),
                           (dict(tail_frames=-1), 'tail_frames'), (dict(tail_frames=2 ** 30 + 1), 'tail_frames'),
                           (dict(linger=-2), 'linger'), (dict(linger=2 ** 30 + 1), 'linger')):
            refused(draw(**kw), needle, entry)
        for f in STATE_FIELDS:
            refused(draw(**{f: None}), 'null state', entry)
    refused(draw(width=63), 'even', lib.pave_draw_trails_nv12)
    refused(draw(height=47), 'even', lib.pave_draw_trails_nv12)


def test_calls_raise_value_errors_on_host_tensors():
    """Shape, type and range checks, and the host-tensor check itself, are ValueErrors raised before anything is
    allocated on or asked of a device."""
    from pavenet_amd import ops
    from pavenet_amd.trails import TrackTrails, TrailStyle, draw_trails_bgr, draw_trails_nv12
    kp, bb, keep = torch.zeros(3, 15, 3), torch.zeros(3, 5), torch.ones(3, dtype=torch.int32)
    ids = torch.ones(3, dtype=torch.int32)
    res = (bb, None, kp)
    m = TrackTrails(15, cameras=2)
    nv, bgr = torch.zeros(72, 64, dtype=torch.uint8), torch.zeros(48, 64, 3, dtype=torch.uint8)
    for call, needle in (
            (lambda: m.update((bb, kp), ids), 'tuple'),
            (lambda: m.update(dict(bboxes=bb), ids), 'bboxes and kpts'),
            (lambda: m.update((bb[:2], None, kp), ids), 'bboxes'),
            (lambda: m.update((bb.double(), None, kp), ids), 'float32'),
            (lambda: m.update(dict(bboxes=bb, kpts=kp, keep=keep.long()), ids), 'int32'),
            (lambda: m.update((torch.zeros(129, 5), None, torch.zeros(129, 15, 3)), torch.zeros(129, dtype=torch.int32)),
             'at most 128'),
            (lambda: m.update((bb, None, torch.zeros(3, 17, 3)), ids), 'K = 17'),
            (lambda: m.update(res, ids.long()), 'ids of results'),
            (lambda: m.update(res, ids[:2]), 'ids of results'),
            (lambda: m.update(res, ids, camera=2), 'camera'),
            (lambda: m.update(res, ids, scale_factor=0.0), 'positive'),
            (lambda: m.update_many([(0, res, ids), (1, res, ids)], scale_factor=[1.0, 1.0, 1.0]), 'scale_factor'),
            (lambda: m.update_many([(0, res)]), 'triples'),
            (lambda: m.update(res, ids), 'HIP device'),
            (lambda: m.reset(camera=2), 'camera'),
            (lambda: m.points(2), 'camera'),
            (lambda: m.state(-1), 'camera'),
            (lambda: draw_trails_nv12(nv, 64, None), 'TrackTrails'),
            (lambda: draw_trails_nv12(nv, 64, m, style=7), 'TrailStyle'),
            (lambda: draw_trails_nv12(nv.float(), 64, m), 'uint8'),
            (lambda: draw_trails_nv12([], 64, m), 'uint8'),
            (lambda: draw_trails_nv12(nv, 64, m, camera=2), 'camera'),
            (lambda: draw_trails_nv12([nv, nv], [64], m), 'width'),
            (lambda: draw_trails_nv12(nv, 64, m, matrix='bt2020'), 'matrix'),
            (lambda: draw_trails_nv12(nv, 64, m), 'HIP device'),
            (lambda: draw_trails_bgr(bgr[..., :2], m), r'\[H, W, 3\]'),
            (lambda: draw_trails_bgr(bgr, m), 'HIP device')):
        with pytest.raises(ValueError, match=needle):
            call()
    assert m._state is None

    def state(cameras=2, S=8, L=4, **over):
        z = dict(dtype=torch.int32)
        s = dict(id=torch.zeros(cameras, S, **z), last=torch.zeros(cameras, S, **z), pos=torch.zeros(cameras, S, 2, **z),
                 head=torch.zeros(cameras, S, **z), count=torch.zeros(cameras, S, **z), box=torch.zeros(cameras, S, 4, **z),
                 pts=torch.zeros(cameras, S, L, 2, **z), when=torch.zeros(cameras, S, L, **z),
                 frame=torch.zeros(cameras, **z), dropped=torch.zeros(cameras, **z))
        s.update(over)
        return s

    def update(entries=((kp, bb, None, ids, 0, (1.0, 1.0)),), st=None, K=15, **kw):
        return ops.trail_update(entries, state() if st is None else st, K=K, **kw)

    def draw(kind='bgr', items=((bgr, None, 0, 0),), st=None, palettes=(bytes(96),), **kw):
        return ops.draw_trails(kind, items, state() if st is None else st, palettes, **kw)
    for call, needle in (
            (lambda: update(st=dict(id=bb)), 'state holds'),
            (lambda: update(st=state(when=torch.zeros(2, 8, dtype=torch.int32))), 'state when'),
            (lambda: update(st=state(S=129)), 'S in'),
            (lambda: update(st=state(L=65)), 'L in'),
            (lambda: update(K=33), 'K'),
            (lambda: update(K=15.0), 'K must be'),
            (lambda: update(st=state(pts=torch.zeros(2, 8, 4, 2))), 'state pts'),
            (lambda: update(st=state(pts=torch.zeros(2, 8, 5, 2, dtype=torch.int32))), 'state pts'),
            (lambda: update(st=state(box=torch.zeros(2, 8, 2, dtype=torch.int32))), 'state box'),
            (lambda: update(st=state(head=torch.zeros(2, 9, dtype=torch.int32))), 'state head'),
            (lambda: update(st=state(frame=torch.zeros(3, dtype=torch.int32))), 'state frame'),
            (lambda: update(stride=0), 'stride'),
            (lambda: update(stride=256), 'stride'),
            (lambda: update(min_step=65536), 'min_step'),
            (lambda: update(min_step=1.0), 'min_step'),
            (lambda: update(max_age=-1), 'max_age'),
            (lambda: update(anchor='toes'), 'anchor must be'),
            (lambda: update(anchor_kpts=(15,)), 'anchor_kpts'),
            (lambda: update(entries=[(kp, bb, None, ids, 0)]), 'entry 0 is'),
            (lambda: update(entries=[(kp[:, :14], bb, None, ids, 0, (1, 1))]), 'kpts of entry 0'),
            (lambda: update(entries=[(kp, bb[:, :4], None, ids, 0, (1, 1))]), 'bboxes of entry 0'),
            (lambda: update(entries=[(kp, bb, keep.long(), ids, 0, (1, 1))]), 'keep of entry 0'),
            (lambda: update(entries=[(kp, bb, None, None, 0, (1, 1))]), 'ids of entry 0'),
            (lambda: update(entries=[(kp, bb, None, ids, 2, (1, 1))]), 'camera of entry 0'),
            (lambda: update(entries=[(kp, bb, None, ids, 0, (1, 0))]), 'scale of entry 0'),
            (lambda: update(), 'HIP device'),
            (lambda: draw(kind='rgb'), 'kind'),
            (lambda: draw(items=()), 'no surface'),
            (lambda: draw(items=[(bgr, None, 0)]), 'an item is'),
            (lambda: draw(thickness=0), 'thickness'),
            (lambda: draw(thickness=2, thickness_tail=3), 'thickness_tail'),
            (lambda: draw(head_radius=33), 'head_radius'),
            (lambda: draw(tail_frames=0), 'tail_frames'),
            (lambda: draw(linger=-1), 'linger'),
            (lambda: draw(st=state(count=torch.zeros(2, 8))), 'state count'),
            (lambda: draw(palettes=()), 'palettes'),
            (lambda: draw(palettes=(bytes(95),)), 'palettes'),
            (lambda: draw(palettes=(bytes(96),) * 5), 'palettes'),
            (lambda: draw(items=[(bgr, None, 2, 0)]), 'camera of surface 0'),
            (lambda: draw(items=[(bgr, None, 0, 1)]), 'palette table'),
            (lambda: draw(kind='nv12', items=[(nv, 63, 0, 0)]), 'even'),
            (lambda: draw(kind='nv12', items=[(nv, 66, 0, 0)]), 'pitch'),
            (lambda: draw(), 'HIP device'),
            (lambda: TrailStyle(thickness=1, thickness_tail=2), 'thickness_tail')):
        with pytest.raises(ValueError, match=needle):
            call()


def test_not_built_sentences_no_longer_list_trails():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    from pavenet_amd import heatmap
    with open(os.path.join(root, 'README.md')) as f:
        readme = f.read()
    assert 'trails of single tracks' not in heatmap.__doc__ and 'trails of single tracks' not in readme
    assert 'Where they came from' in readme and 'draw_trails_nv12' in readme
