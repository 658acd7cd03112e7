"""Footfall maps, the parts that need no GPU: the edges of the update rule of DESIGN section 21 as hand-worked scripts
on its numpy statement (tests/heat_cases.py on tests/heat_ref.py), where the mass of jittering walkers lands, the
plan's C layout, every refusal of the C entry point and of the Python calls, and the exports."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import heat_cases as HC
from tests import heat_ref as HR
from tests.test_track_cpu import walk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class OracleHarness:
    """tests/heat_cases.py's harness on the oracle alone."""

    def __init__(self, K, **kw):
        self.ref = HR.HeatRef(K, **kw)

    def frame(self, kpts, bboxes, ids, entries, keep=None, camera=0):
        before = {k: v.copy() for k, v in self.ref.maps(camera).items()}
        out = self.ref.update(kpts, bboxes, np.asarray(ids, np.int64).astype(np.int32),
                              None if keep is None else np.asarray(keep, np.int32), camera=camera)
        frame, hl = int(self.ref.frame[camera]), self.ref.half_life
        HC.invariant(before, self.ref.maps(camera), out, self.ref.radius, hl > 0 and frame % hl == 0, entries)
        return out

    def get(self, field, camera=0):
        return dict(self.ref.state(camera), **self.ref.maps(camera))[field]


@pytest.mark.parametrize('script', HC.SCRIPTS, ids=lambda s: s.__name__)
def test_hand_worked_scripts_on_the_oracle(script):
    script(OracleHarness)


PEOPLE = 6


@pytest.mark.parametrize('height', [40, 100, 300])
def test_where_the_mass_of_walkers_lands(height):
    """A measurement, printed for DESIGN section 21 and not asserted beyond what the rule guarantees: the six walkers
    of tests/test_zones_cpu.py (1 % jitter on every coordinate), steps 1 .. 8 px per frame, cell 8, radius 1; the
    share of all dwell mass within radius + 1 cells (Chebyshev) of the cells a walker's true feet pass through.  What
    the rule guarantees: every frame adds (radius + 1)^4 per walker (nobody is near the border), and every walker's
    cells are visited."""
    for step in (1, 2, 4, 8):
        frames, radius, cell = (60 if step < 8 else 36), 1, 8
        ref = HR.HeatRef(15, size=(2816, 512), cell=cell, radius=radius)
        path = np.zeros((ref.Gh, ref.Gw), bool)
        for f, (kpts, bboxes, who) in enumerate(walk(height, step, frames=frames, people=PEOPLE, seed=int(height * 10 + step))):
            out = ref.update(kpts, bboxes, who + 1)
            assert (out['cell'] >= 0).all()
            for p in range(PEOPLE):
                x, y = 100.0 + 400.0 * p + step * f + 0.2 * height, 50.0 + 7.0 * p + height
                path[int(y) // cell, int(x) // cell] = True
        assert int(ref.dwell[0].sum()) == frames * PEOPLE * (radius + 1) ** 4 and ref.dropped[0] == 0
        near = np.zeros_like(path)
        ys, xs = np.nonzero(path)
        for y, x in zip(ys, xs):
            near[max(y - radius - 1, 0):y + radius + 2, max(x - radius - 1, 0):x + radius + 2] = True
        share = ref.dwell[0][near].sum() / ref.dwell[0].sum()
        assert int(ref.visits[0].sum()) >= PEOPLE and int(ref.peak[0, 0]) == int(ref.dwell[0].max())
        print(f'height {height} step {step}: {100 * share:.2f} % of the dwell mass within {radius + 1} cells of the true '
              f'paths; visits {int(ref.visits[0].sum())} over {int(path.sum())} path cells')


def test_defaults_ranges_and_exports():
    import pavenet_amd
    from pavenet_amd import FootfallMap, HeatStyle, draw_heat_bgr, draw_heat_nv12, heatmap, native
    assert FootfallMap is heatmap.FootfallMap and HeatStyle is heatmap.HeatStyle
    assert draw_heat_nv12 is heatmap.draw_heat_nv12 and draw_heat_bgr is heatmap.draw_heat_bgr
    assert pavenet_amd.FootfallMap is FootfallMap
    m = FootfallMap(17, size=(1920, 1080))
    assert (m.cell, m.cameras, m.max_tracks, m.max_age, m.anchor, m.anchor_kpts, m.radius, m.half_life) == \
        (8, 1, 128, 30, 'feet', (15, 16), 1, 0)
    assert (m.Gw, m.Gh) == (240, 135) and m.score_thr == pytest.approx(0.3) and m.kpt_thr == 0.0
    assert m.maps(0) is None and m.state(0) is None and m.device_tensors() is None and m.update_many([]) == []
    m.reset()
    assert (FootfallMap(15, size=(37, 19)).Gw, FootfallMap(15, size=(37, 19)).Gh) == (5, 3)
    assert (FootfallMap(14, size=(3, 2), cell=4).Gw, FootfallMap(14, size=(3, 2), cell=4).Gh) == (1, 1)
    assert FootfallMap(15, size=(8192, 8192), cell=16).Gw == 512 and FootfallMap(15, size=(2048, 4), cell=4).Gw == 512
    assert FootfallMap(15, size=(10, 10), anchor='box', anchor_kpts=(1, 2)).anchor_kpts == ()
    assert (native.HEAT_MAX_GRID, native.HEAT_MAX_RADIUS, native.HEAT_MAX_HALF_LIFE) == (512, 3, 2 ** 18)
    for kw, needle in ((dict(K=0), 'K is'), (dict(K=33), 'K is'), (dict(size=(0, 10)), 'size'), (dict(size=(10, 8193)), 'size'),
                       (dict(size=10), 'size'), (dict(size=(10.5, 10)), 'size'), (dict(cell=12), 'cell'), (dict(cell=2), 'cell'),
                       (dict(cell=128), 'cell'), (dict(size=(2049, 4), cell=4), 'grid'), (dict(size=(64, 8192), cell=8), 'grid'),
                       (dict(cameras=0), 'cameras'), (dict(cameras=4097), 'cameras'), (dict(max_tracks=0), 'max_tracks'),
                       (dict(max_tracks=129), 'max_tracks'), (dict(max_age=-1), 'max_age'), (dict(anchor='toes'), 'anchor'),
                       (dict(K=5), 'anchor_kpts'), (dict(anchor_kpts=(0, 1, 2, 3, 4)), 'at most 4'),
                       (dict(anchor_kpts=(15,)), 'anchor_kpts'), (dict(radius=-1), 'radius'), (dict(radius=4), 'radius'),
                       (dict(radius=1.0), 'radius'), (dict(half_life=-1), 'half_life'), (dict(half_life=2 ** 18 + 1), 'half_life')):
        args = dict(K=15, size=(64, 48))
        args.update(kw)
        with pytest.raises(ValueError, match=needle):
            FootfallMap(**args)
    s = HeatStyle()
    assert (s.source, s.full_scale, s.alpha_max, s.floor, s.smooth) == ('dwell', None, 160, 1, True)
    assert s.palette == [tuple(c) for c in heatmap.HEAT_PALETTE] and len(heatmap.HEAT_PALETTE) == 256
    assert heatmap.HEAT_PALETTE[0] == (48, 0, 0) and heatmap.HEAT_PALETTE[255] == (0, 0, 255) and heatmap.HEAT_PALETTE[51] == (255, 64, 0)
    tables = s.tables()
    assert tables.shape == (5, 256, 3) and tables.dtype == np.uint8
    from tests.heat_draw_ref import yuv_table
    assert (tables[0] == np.asarray(s.palette)).all() and heatmap.MODES[2] == ('bt709', False)
    assert (tables[3] == yuv_table(s.palette, 'bt709', False)).all()
    for kw, needle in ((dict(source='both'), 'source'), (dict(palette=[(0, 0, 0)] * 255), '256'),
                       (dict(palette=[(0, 0, 256)] * 256), 'palette colour'), (dict(palette=7), '256'),
                       (dict(full_scale=0), 'full_scale'), (dict(full_scale=2 ** 31), 'full_scale'),
                       (dict(full_scale=1.5), 'full_scale'), (dict(alpha_max=257), 'alpha_max'), (dict(alpha_max=-1), 'alpha_max'),
                       (dict(floor=256), 'floor'), (dict(floor=-1), 'floor')):
        with pytest.raises(ValueError, match=needle):
            HeatStyle(**kw)


def _lib():
    from pavenet_amd import native
    from pavenet_amd.build_native import build_native
    build_native()
    return native, native.load()


def layout(tmp_path, struct, name):
    fields = [f for f, _ in struct._fields_]
    src = tmp_path / 'layout.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pave_hip.h"\nint main(void) {\n'
                   f'  printf("%zu", sizeof({name}));\n'
                   + ''.join(f'  printf(" %zu", offsetof({name}, {f}));\n' for f in fields)
                   + '  return 0;\n}\n')
    exe = tmp_path / 'layout'
    subprocess.run(['gcc', '-std=c99', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == ctypes.sizeof(struct) < 4096
    assert got[1:] == [getattr(struct, f).offset for f in fields]


def test_heat_plan_layout_and_entry(tmp_path):
    """native.HeatPlan is the header's pave_heat_plan field for field, under the 4 KB kernel-argument limit, and the
    entry is in the header, the binding and both libraries; the ABI number is the one it was."""
    native, lib = _lib()
    vp, ci = ctypes.c_void_p, ctypes.c_int
    assert native.FUNCTIONS['pave_heat_update'] == (ci, [vp, vp]) and 'pave_heat_update' in native.SIGNATURES
    for path in (native.LIB_PATH, native.DIAG_LIB_PATH):
        out = subprocess.run(['nm', '-D', '--defined-only', path], capture_output=True, text=True, check=True).stdout
        assert 'pave_heat_update' in {ln.split()[-1] for ln in out.splitlines()}
    assert native.ABI_VERSION == 21 and lib.pave_abi_version() == 21
    assert ctypes.sizeof(native.HeatPlan) == 2440 < 4096
    if not shutil.which('gcc'):
        pytest.skip('no gcc')
    layout(tmp_path, native.HeatPlan, 'pave_heat_plan')


STATE_FIELDS = ('slot_id', 'slot_last', 'slot_cell', 'frame', 'dropped')
MAP_FIELDS = ('peak', 'dwell', 'visits')


def test_c_entry_refuses_bad_plans_before_any_device_call():
    """No GPU: every refusal is PAVE_E_ARG with a message (the addresses are never dereferenced)."""
    native, lib = _lib()
    host = (ctypes.c_ubyte * 64)()
    addr = ctypes.addressof(host)

    def plan(entries=2, n=3, K=15, S=8, cameras=2, camera=1, scale=(1.0, 1.0), max_age=30, anchor=0, anchor_kpts=(13, 14),
             width=64, height=48, cell=8, radius=1, half_life=0, kpts=addr, bboxes=addr, ids=addr, keep=None,
             out_cell=addr, out_dwell=addr, out_visits=addr, **state):
        p = native.HeatPlan()
        for i in range(min(max(entries, 0), 32)):
            p.kpts[i], p.bboxes[i], p.ids[i], p.keep[i] = kpts, bboxes, ids, keep
            p.out_cell[i], p.out_dwell[i], p.out_visits[i] = out_cell, out_dwell, out_visits
            p.n[i], p.camera[i], p.scale[i][0], p.scale[i][1] = n, camera, scale[0], scale[1]
        for f in STATE_FIELDS + MAP_FIELDS:
            setattr(p, f, state.get(f, addr))
        for i, k in enumerate(anchor_kpts[:4]):
            p.anchor_kpt[i] = k
        p.entries, p.cameras, p.S, p.K, p.max_age = entries, cameras, S, K, max_age
        p.anchor, p.n_anchor = anchor, len(anchor_kpts)
        p.width, p.height, p.cell, p.radius, p.half_life = width, height, cell, radius, half_life
        p.score_thr, p.kpt_thr = 0.3, 0.0
        return p

    def refused(p, needle):
        assert lib.pave_heat_update(ctypes.byref(p) if p is not None else None, None) == native.DEFINES['PAVE_E_ARG'] == -1
        assert needle in lib.pave_last_error().decode(), lib.pave_last_error()

    refused(None, 'null plan')
    refused(plan(entries=0), 'frames per launch')
    refused(plan(entries=33), 'frames per launch')
    refused(plan(kpts=None), 'null pose')
    refused(plan(bboxes=None), 'null pose')
    refused(plan(ids=None), 'null ids')
    for f in ('out_cell', 'out_dwell', 'out_visits'):
        refused(plan(**{f: None}), 'null output')
    for f in STATE_FIELDS:
        refused(plan(**{f: None}), 'null state')
    for f in MAP_FIELDS:
        refused(plan(**{f: None}), 'null map')
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
    for kw in (dict(width=0), dict(height=0), dict(width=8193), dict(height=8193), dict(cell=0), dict(cell=2), dict(cell=12),
               dict(cell=128), dict(cell=-8), dict(width=2049, cell=4), dict(height=4097, cell=8)):
        refused(plan(**kw), 'a map of')
    refused(plan(radius=-1), 'radius')
    refused(plan(radius=4), 'radius')
    refused(plan(half_life=-1), 'half_life')
    refused(plan(half_life=2 ** 18 + 1), 'half_life')
    refused(plan(anchor=-1), 'anchor outside')
    refused(plan(anchor=3), 'anchor outside')
    refused(plan(anchor_kpts=(0, 1, 2, 3, 4)), 'n_anchor')
    refused(plan(anchor_kpts=(13, 15)), 'anchor key point')
    refused(plan(K=14), 'anchor key point')


def test_calls_raise_value_errors_on_host_tensors():
    """Shape, type and range checks, and the host-tensor check itself, are ValueErrors raised before anything is
    allocated on or asked of a device."""
    from pavenet_amd import native, ops
    from pavenet_amd.heatmap import FootfallMap
    kp, bb, keep = torch.zeros(3, 15, 3), torch.zeros(3, 5), torch.ones(3, dtype=torch.int32)
    ids = torch.ones(3, dtype=torch.int32)
    res = (bb, None, kp)
    m = FootfallMap(15, size=(64, 48), cameras=2)
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
            (lambda: m.maps(2), 'camera'),
            (lambda: m.state(-1), 'camera')):
        with pytest.raises(ValueError, match=needle):
            call()
    assert m._state is None

    def state(cameras=2, S=8, Gh=6, Gw=8, **over):
        z = dict(dtype=torch.int32)
        s = dict(id=torch.zeros(cameras, S, **z), last=torch.zeros(cameras, S, **z), cell=torch.zeros(cameras, S, **z),
                 frame=torch.zeros(cameras, **z), dropped=torch.zeros(cameras, **z), peak=torch.zeros(cameras, 2, **z),
                 dwell=torch.zeros(cameras, Gh, Gw, **z), visits=torch.zeros(cameras, Gh, Gw, **z))
        s.update(over)
        return s

    def update(entries=((kp, bb, None, ids, 0, (1.0, 1.0)),), st=None, K=15, size=(64, 48), **kw):
        return ops.heat_update(entries, state() if st is None else st, K=K, size=size, **kw)
    for call, needle in (
            (lambda: update(st=dict(id=bb)), 'state holds'),
            (lambda: update(st=state(peak=torch.zeros(2, 3, dtype=torch.int32))), 'state peak'),
            (lambda: update(st=state(S=129)), 'S in'),
            (lambda: update(K=33), 'K'),
            (lambda: update(K=15.0), 'K must be'),
            (lambda: update(st=state(dwell=torch.zeros(2, 6, 8))), 'state dwell'),
            (lambda: update(st=state(visits=torch.zeros(2, 6, 7, dtype=torch.int32))), 'state visits'),
            (lambda: update(st=state(cell=torch.zeros(2, 9, dtype=torch.int32))), 'state cell'),
            (lambda: update(st=state(frame=torch.zeros(3, dtype=torch.int32))), 'state frame'),
            (lambda: update(size=(65, 48)), 'state dwell'),
            (lambda: update(size=(0, 48)), 'size'),
            (lambda: update(cell=3), 'cell'),
            (lambda: update(size=(4096, 48), cell=4), 'grid'),
            (lambda: update(radius=4), 'radius'),
            (lambda: update(half_life=2 ** 18 + 1), 'half_life'),
            (lambda: update(half_life=1.0), 'half_life'),
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
            (lambda: update(), 'HIP device')):
        with pytest.raises(ValueError, match=needle):
            call()
