"""The ground plane, the parts that need no GPU: the rule of DESIGN section 23 as hand-worked scripts on its numpy
statement (tests/floor_cases.py on tests/floor_ref.py), the calibration (the DLT, the quantisation, the package's
against the statement's), the integer projection against float64 on three calibrations, the square root, the bridge
into the statements of sections 17, 21 and 22, a measurement for the README, the plan's C layout, every refusal of the
C entry point and of the Python calls, and the exports."""
import ctypes
import math
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import floor_cases as FC
from tests import floor_ref as FR
from tests.heat_ref import HeatRef
from tests.test_heat_cpu import layout
from tests.test_track_gpu import FIGURE15, poses
from tests.trail_ref import TrailRef
from tests.zones_ref import ZoneRef


class OracleHarness:
    """tests/floor_cases.py's harness on the oracle alone."""

    def __init__(self, K, **kw):
        self.ref = FR.FloorRef(K, **kw)

    def set_plane(self, camera, **kw):
        self.ref.set_plane(camera, **kw)

    def frame(self, kpts, bboxes, ids, keep=None, camera=0):
        ids = np.asarray(ids, np.int64).astype(np.int32)
        return self.ref.update(kpts, bboxes, ids, None if keep is None else np.asarray(keep, np.int32), camera=camera)

    def get(self, field, camera=0):
        return self.ref.state(camera)[field]


@pytest.mark.parametrize('script', FC.SCRIPTS, ids=lambda s: s.__name__)
def test_hand_worked_scripts_on_the_oracle(script):
    script(OracleHarness)


def camera_matrix(tilt_deg, height_mm, focal, size=8192):
    """pixels -> floor mm for a pinhole `height_mm` above the floor whose axis is `tilt_deg` off the plumb line,
    principal point in the middle of a size x size picture; the third row is positive on the floor."""
    s, c = math.sin(math.radians(tilt_deg)), math.cos(math.radians(tilt_deg))
    R = np.asarray([[1.0, 0.0, 0.0], [0.0, -c, -s], [0.0, s, -c]])          # world -> camera: x, y (down the picture), z
    C = np.asarray([0.0, 0.0, height_mm])
    Kc = np.asarray([[focal, 0.0, size / 2], [0.0, focal, size / 2], [0.0, 0.0, 1.0]])
    M = Kc @ np.stack([R[:, 0], R[:, 1], -R @ C], 1)                         # floor (X, Y, 1) -> pixels
    H = np.linalg.inv(M)
    foot = M @ np.asarray([0.0, height_mm * math.tan(math.radians(tilt_deg)), 1.0])     # where the axis meets the floor
    foot = foot / foot[2]
    return H if H[2] @ foot > 0 else -H


FRONTO = np.asarray([[2.5, 0.0, -3000.0], [0.0, 2.5, -2000.0], [0.0, 0.0, 1.0]])
TILTED = camera_matrix(30.0, 3000.0, 6000.0)        # 30 + atan(4096 / 6000) = 64 degrees: the horizon is out of the picture
HORIZON = camera_matrix(60.0, 3000.0, 6000.0)       # the horizon is the row 4096 - 6000 tan(30) = 632
CALIBRATIONS = {'fronto': FRONTO, 'tilted': TILTED, 'horizon': HORIZON}


def to_floor(H, px, py):
    v = H @ np.asarray([px, py, 1.0])
    return v[0] / v[2], v[1] / v[2], v[2]


@pytest.mark.parametrize('pairs', [4, 9])
def test_the_dlt_recovers_a_known_matrix(pairs):
    """From 4 pairs (exactly determined) and 9 (least squares of exact data) the DLT returns the matrix the pairs were
    made with, up to scale, to 1e-9 of its largest entry; the package's solver and the statement's agree to the bit,
    and so do the words they quantise to."""
    from pavenet_amd import floor
    grid = [(x, y) for y in (1500.0, 4000.0, 7900.0) for x in (300.0, 4100.0, 7800.0)]
    pts = grid if pairs == 9 else [grid[0], grid[2], grid[6], grid[8]]
    for name, Ht in CALIBRATIONS.items():
        given = [((x, y), to_floor(Ht, x, y)[:2]) for x, y in pts]
        H, row = floor.calibrate(points=given)
        assert np.abs(H / H[2, 2] - Ht / Ht[2, 2]).max() <= 1e-9 * np.abs(Ht / Ht[2, 2]).max(), name
        ref = FR.dlt(given)
        assert np.array_equal(H, ref) and row[:9] == FR.quantise(ref), name
        assert row[9:] == [-FR.MAX_MM, -FR.MAX_MM, FR.MAX_MM, FR.MAX_MM, 1, 0, 0]
        at = np.mean([p for p, _ in given], 0)
        assert H[2] @ [at[0], at[1], 1.0] > 0, name


def test_the_quantisation_fills_61_bits_and_no_more():
    from pavenet_amd import floor
    rng = np.random.default_rng(231)
    for name, H in CALIBRATIONS.items():
        for scale in (1.0, 1e-30, 1e30, 2.0 ** -1000, 3.0):
            words = floor.quantise_plane(H * scale)
            assert words == FR.quantise(H * scale) and FR.row_ok(words), (name, scale)
            assert max((abs(words[3 * r]) + abs(words[3 * r + 1])) * 65535 + abs(words[3 * r + 2]) for r in range(3)) >= 1 << 59
    for _ in range(20):
        H = rng.normal(size=(3, 3)) * 10.0 ** rng.integers(-6, 6, (3, 3))
        if np.linalg.cond(H) < 1e12:
            assert floor.quantise_plane(H) == FR.quantise(H)
    assert floor.calibrate(matrix=FRONTO, bounds=(-5, 0, 7, 9))[1][9:13] == [-5, 0, 7, 9]


MEASURED = {}


@pytest.mark.parametrize('name', list(CALIBRATIONS))
def test_the_integer_projection_against_float64(name):
    """A 129 x 129 grid of anchors over an 8192 x 8192 picture.  Where float64 puts the point on the floor and more than
    1 mm inside the bounds, the integer rule does too and differs by at most 1 mm per axis (1/2 from the rounding, the
    rest from the quantisation of G); where float64 puts it above the horizon, the integer rule has it off the floor.
    The largest difference is printed for DESIGN section 23."""
    H = CALIBRATIONS[name]
    G = FR.quantise(H)
    bounds = (-FR.MAX_MM, -FR.MAX_MM, FR.MAX_MM, FR.MAX_MM)
    worst, on, above = 0.0, 0, 0
    for ay in np.linspace(0, 65534, 129).astype(np.int64):
        for ax in np.linspace(0, 65534, 129).astype(np.int64):
            x, y, w = to_floor(H, ax / 8.0, ay / 8.0)
            got = FR.project(G, bounds, int(ax), int(ay))
            if w > 0 and max(abs(x), abs(y)) < FR.MAX_MM - 1:
                assert got is not None, (name, ax, ay, x, y)
                worst = max(worst, abs(got[0] - x), abs(got[1] - y))
                on += 1
            elif w < 0:
                assert got is None, (name, ax, ay)
                above += 1
    MEASURED[name] = worst
    print(f'{name}: {on} anchors on the floor, {above} above the horizon, largest |integer - float64| = {worst:.6f} mm')
    assert worst <= 1.0 and on > 0
    assert (above > 0) == (name == 'horizon')


def test_floor_division_of_negative_numerators():
    """X = floor((2 nx + w) / (2 w)) at negative nx: -0.5 rounds to 0 and -0.51 to -1, where a truncating division
    gives 0 for both; and the half-way point goes up."""
    G, bounds = [4, 0, 0, 0, 4, 0, 0, 0, 8], (-100, -100, 100, 100)         # X = ax / 2
    assert FR.project(G, bounds, 3, 1) == (2, 1) and FR.project(G, bounds, 1, 0) == (1, 0)
    G = [-4, 0, 0, 0, -4, 0, 0, 0, 8]                                        # X = -ax / 2
    assert FR.project(G, bounds, 1, 3) == (0, -1) and FR.project(G, bounds, 2, 5) == (-1, -2)
    assert FR.project(G, bounds, 200, 0) == (-100, 0) and FR.project(G, bounds, 201, 0) == (-100, 0)
    assert FR.project(G, bounds, 202, 0) is None
    assert FR.project([4, 0, 0, 0, 4, 0, 0, 0, 0], bounds, 1, 1) is None     # w = 0
    assert FR.project([4, 0, 0, 0, 4, 0, 0, 0, -8], bounds, 1, 1) is None    # w < 0


def isqrt_by_double(v):
    """The kernel's way: the double square root, truncated, and a correction both ways."""
    r = int(np.sqrt(np.float64(v)))
    if r * r > v:
        r -= 1
    if (r + 1) * (r + 1) <= v:
        r += 1
    return r


def test_the_square_root_is_exact_where_a_double_is_not():
    """k^2 - 1, k^2 and k^2 + 1 for k around 2^17, 2^22 and 2^30 (the rule's operands reach 2^60): the corrected root
    is math.isqrt's; around 2^30 the uncorrected one is not, which is why the correction is there."""
    wrong = 0
    for centre in (1 << 17, 1 << 22, 1 << 30, (1 << 30) - 12345, 759250124):
        for k in range(centre - 64, centre + 65):
            for v in (k * k - 1, k * k, k * k + 1):
                assert isqrt_by_double(v) == math.isqrt(v), v
                wrong += int(np.sqrt(np.float64(v))) != math.isqrt(v)
    assert wrong > 0
    assert isqrt_by_double(0) == 0 and isqrt_by_double(1) == 1 and isqrt_by_double((1 << 60) - 1) == (1 << 30) - 1


@pytest.mark.parametrize('anchor', ['feet', 'box', 'centre'])
def test_the_bridge_stands_every_pose_at_2_px_2_py(anchor):
    """The statement's floor result pushed through the statements of sections 17, 21 and 22 with scale 1: whatever
    the consumer's anchor, a pose on the plan stands at exactly (2 Px, 2 Py) eighths, and a pose off it takes no part.
    Key-point scores around kpt_thr, so 'feet' uses two, one or no ankle."""
    rng = np.random.default_rng(232)
    kw = dict(anchor=anchor, max_tracks=16, kpt_thr=0.4)
    unit, origin = 30, (-4000, 1000)
    ref = FR.FloorRef(15, unit=unit, origin=origin, **kw)
    ref.set_plane(0, matrix=TILTED)
    zone, heat, trail = ZoneRef(15, **kw), HeatRef(15, (2048, 2048), **kw), TrailRef(15, min_step=0, **kw)
    stood = 0
    for f in range(6):
        pos = np.stack([rng.uniform(0, 7800, 12), rng.uniform(0, 7000, 12)], 1)
        kpts, bboxes = poses(rng, FIGURE15, pos, height=300.0, kpt_scores=rng.uniform(0.0, 1.0, (12, 15)).astype(np.float32))
        bboxes[10, 4] = 0.1
        ids = np.arange(1, 13, dtype=np.int32)
        out = ref.update(kpts, bboxes, ids)
        want = FR.plan_points(out, unit, origin)
        assert want[10] is None and sum(p is not None for p in want) >= 3
        zone.update(out['kpts'], out['bboxes'], ids)
        heat.update(out['kpts'], out['bboxes'], ids)
        trail.update(out['kpts'], out['bboxes'], ids)
        for d, p in enumerate(want):
            slots = np.nonzero((zone.id[0] == ids[d]) & (zone.last[0] == f + 1))[0]
            if p is None:
                assert len(slots) == 0 and heat.anchors[d].tolist() == [-1, -1]
                continue
            stood += 1
            assert zone.pos[0, slots[0]].tolist() == [2 * p[0], 2 * p[1]]
            assert heat.anchors[d].tolist() == [2 * p[0], 2 * p[1]]
            t = np.nonzero(trail.id[0] == ids[d])[0][0]
            assert trail.pos[0, t].tolist() == [2 * p[0], 2 * p[1]]
    assert stood >= 18


def test_six_walkers_near_and_far_a_measurement():
    """A measurement, printed for the README and DESIGN section 23 and not asserted beyond what the rule guarantees: six
    people walking 1.4 m/s at 25 frames a second (56 mm a frame) across the floor under the tilted camera, three 2.5 m
    from its foot and three 9 m, with 1 % jitter on every key point.  Speed from the floor (out['speed'] / 256 mm per
    frame) against 56, and a footfall map on the floor plan (200 mm cells) against one in the picture (32-pixel cells):
    the dwell mass a walker leaves per cell it touched.  What the rule guarantees: travel is at least the straight
    distance less one mm per move."""
    rng = np.random.default_rng(233)
    H = camera_matrix(55.0, 3000.0, 3000.0, size=4096)
    M = np.linalg.inv(H)
    plane = FR.FloorRef(15, unit=25, origin=(-6000, 0), velocity_gain=4)
    plane.set_plane(0, matrix=H)
    on_floor, in_picture = HeatRef(15, (480, 640), cell=8, radius=0), HeatRef(15, (4096, 4096), cell=32, radius=0)
    frames, step = 100, 56.0
    lanes = [2500.0, 2900.0, 3300.0, 9000.0, 9800.0, 10600.0]
    speeds, first, last = [[] for _ in lanes], {}, {}
    for f in range(frames):
        pos, heights = [], []
        for Y in lanes:
            feet = M @ [-2800.0 + step * f, Y, 1.0]
            head = M @ [-2800.0 + step * f, Y + 1.0, 1.0]
            feet, head = feet[:2] / feet[2], head[:2] / head[2]
            h = 1700.0 * np.hypot(*(head - feet))               # pixels per mm along the floor, times a person
            heights.append(h)
            pos.append((feet[0] - 0.2 * h, feet[1] - h))
        kpts = np.concatenate([poses(rng, FIGURE15, [p], height=h)[0] for p, h in zip(pos, heights)])
        bboxes = np.concatenate([poses(rng, FIGURE15, [p], height=h)[1] for p, h in zip(pos, heights)])
        ids = np.arange(1, 7, dtype=np.int32)
        out = plane.update(kpts, bboxes, ids)
        assert out['on'].all()
        on_floor.update(out['kpts'], out['bboxes'], ids)
        in_picture.update(kpts, bboxes, ids)
        for p in range(6):
            first.setdefault(p, out['xy'][p].copy())
            last[p] = out['xy'][p].copy()
            if f >= 20:
                speeds[p].append(out['speed'][p] / 256.0)
    for p in range(6):
        straight = math.hypot(*(last[p] - first[p]).tolist())
        assert out['travel'][p] >= straight - frames
    for name, group in (('near', range(3)), ('far', range(3, 6))):
        v = np.concatenate([speeds[p] for p in group])
        print(f'{name}: pixel height {np.mean([heights[p] for p in group]):.0f}, speed {v.mean():.1f} mm/frame (56 walked), '
              f'rms error {np.sqrt(((v - 56) ** 2).mean()):.1f}, travel {np.mean([out["travel"][p] for p in group]):.0f} mm '
              f'({step * (frames - 1):.0f} walked)')
    for name, m in (('floor plan', on_floor), ('picture', in_picture)):
        rows = m.dwell[0].shape[0]
        near, far = (m.dwell[0][rows // 2:], m.dwell[0][:rows // 2]) if name == 'picture' else \
            (m.dwell[0][:rows // 3], m.dwell[0][rows // 3:])
        print(f'{name}: dwell per touched cell near {near.sum() / max((near > 0).sum(), 1):.2f}, far '
              f'{far.sum() / max((far > 0).sum(), 1):.2f}; share of all mass in the far half {far.sum() / m.dwell[0].sum():.2f}')
    assert on_floor.dwell[0].sum() == 6 * frames


def test_defaults_ranges_and_exports():
    import pavenet_amd
    from pavenet_amd import GroundPlane, floor, native
    assert GroundPlane is floor.GroundPlane and pavenet_amd.GroundPlane is GroundPlane
    m = GroundPlane(17)
    assert (m.cameras, m.max_tracks, m.max_age, m.anchor, m.anchor_kpts, m.velocity_gain, m.near, m.unit, m.origin) == \
        (1, 128, 30, 'feet', (15, 16), 4, 1500, 10, (0, 0))
    assert m.score_thr == pytest.approx(0.3) and m.kpt_thr == 0.0 and m.H == [None]
    assert m.state(0) is None and m.calibration(0) is None and m.update_many([]) == []
    m.reset()
    assert GroundPlane(15, anchor='box', anchor_kpts=(1, 2)).anchor_kpts == ()
    assert (native.FLOOR_MAX_MM, native.FLOOR_MAX_NEAR, native.FLOOR_MAX_UNIT, native.FLOOR_MAX_GAIN) == \
        (2 ** 20 - 1, 2 ** 20, 1000, 16)
    for kw in (dict(velocity_gain=1), dict(velocity_gain=16), dict(near=0), dict(near=2 ** 20), dict(unit=1), dict(unit=1000),
               dict(origin=(-2 ** 20 + 1, 2 ** 20 - 1))):
        GroundPlane(15, **kw)
    for kw, needle in ((dict(K=0), 'K is'), (dict(K=33), 'K is'), (dict(cameras=0), 'cameras'), (dict(cameras=4097), 'cameras'),
                       (dict(max_tracks=0), 'max_tracks'), (dict(max_tracks=129), 'max_tracks'), (dict(max_age=-1), 'max_age'),
                       (dict(velocity_gain=0), 'velocity_gain'), (dict(velocity_gain=17), 'velocity_gain'),
                       (dict(velocity_gain=4.0), 'velocity_gain'), (dict(near=-1), 'near'), (dict(near=2 ** 20 + 1), 'near'),
                       (dict(near=True), 'near'), (dict(unit=0), 'unit'), (dict(unit=1001), 'unit'), (dict(unit=10.0), 'unit'),
                       (dict(origin=0), 'origin'), (dict(origin=(0, 0, 0)), 'origin'), (dict(origin=(0.5, 0)), 'origin'),
                       (dict(origin=(2 ** 20, 0)), 'origin'), (dict(anchor='toes'), 'anchor'), (dict(K=5), 'anchor_kpts'),
                       (dict(anchor_kpts=(0, 1, 2, 3, 4)), 'at most 4'), (dict(anchor_kpts=(15,)), 'anchor_kpts')):
        args = dict(K=15)
        args.update(kw)
        with pytest.raises(ValueError, match=needle):
            GroundPlane(**args)


def test_set_plane_refuses_before_anything_is_allocated():
    from pavenet_amd import GroundPlane
    m = GroundPlane(15, cameras=2)
    square = [((0, 0), (0, 0)), ((100, 0), (1000, 0)), ((100, 100), (1000, 1000)), ((0, 100), (0, 1000))]
    nan = float('nan')
    for kw, needle in (
            (dict(), 'points= or matrix='),
            (dict(points=square, matrix=FRONTO), 'points= or matrix='),
            (dict(points=square[:3]), 'at least 4'),
            (dict(points=[(0, 0)] * 4), 'pairs'),
            (dict(points=[7, 8, 9, 10]), 'pairs'),
            (dict(points=square[:3] + [((nan, 0), (5, 5))]), 'finite'),
            (dict(points=square[:3] + [((5, 5), (float('inf'), 5))]), 'finite'),
            (dict(points=[((i, 2 * i), (10 * i, i * i)) for i in range(5)]), 'picture points lie on one line'),
            (dict(points=[((i, i * i), (10 * i, 20 * i)) for i in range(5)]), 'floor points lie on one line'),
            (dict(points=[((0, 0), (0, 0)), ((50, 0), (500, 0)), ((100, 0), (1000, 0)), ((0, 100), (0, 1000))]), 'singular'),
            (dict(points=[((x, y), to_floor(HORIZON, x, y)[:2]) for x, y in ((100, 100), (8000, 100), (100, 8000), (8000, 8000))]),
             'horizon'),
            (dict(matrix=[[1, 0, 0], [0, 1, 0]]), '3 x 3'),
            (dict(matrix='plane'), '3 x 3'),
            (dict(matrix=[[1, 0, 0], [0, nan, 0], [0, 0, 1]]), 'finite'),
            (dict(matrix=[[1, 0, 0], [2, 0, 0], [0, 0, 1]]), 'singular'),
            (dict(matrix=np.zeros((3, 3))), 'positive at the picture point'),
            (dict(matrix=-FRONTO), 'positive at the picture point'),
            (dict(matrix=FRONTO, bounds=(0, 0, 10)), 'bounds'),
            (dict(matrix=FRONTO, bounds=7), 'bounds'),
            (dict(matrix=FRONTO, bounds=(0, 0, 10.5, 10)), 'bounds'),
            (dict(matrix=FRONTO, bounds=(10, 0, 0, 10)), 'bounds'),
            (dict(matrix=FRONTO, bounds=(0, 0, 2 ** 20, 10)), 'bounds')):
        with pytest.raises(ValueError, match=needle):
            m.set_plane(0, **kw)
    with pytest.raises(ValueError, match='camera'):
        m.set_plane(2, matrix=FRONTO)
    assert m._state is None and m._calib is None and m.H == [None, None]


def _lib():
    from pavenet_amd import native
    from pavenet_amd.build_native import build_native
    build_native()
    return native, native.load()


def test_floor_plan_layout_and_entry(tmp_path):
    """native.FloorPlan is the header's pave_floor_plan field for field, under the 4 KB kernel-argument limit, and the
    entry is in the header, the binding and both libraries; the ABI number is the one it was."""
    native, lib = _lib()
    vp, ci = ctypes.c_void_p, ctypes.c_int
    assert native.FUNCTIONS['pave_floor_update'] == (ci, [vp, vp]) and 'pave_floor_update' in native.SIGNATURES
    for path in (native.LIB_PATH, native.DIAG_LIB_PATH):
        out = subprocess.run(['nm', '-D', '--defined-only', path], capture_output=True, text=True, check=True).stdout
        assert 'pave_floor_update' in {ln.split()[-1] for ln in out.splitlines()}
    assert native.ABI_VERSION == 21 and lib.pave_abi_version() == 21
    assert ctypes.sizeof(native.FloorPlan) == 2192 < 4096
    if not shutil.which('gcc'):
        pytest.skip('no gcc')
    layout(tmp_path, native.FloorPlan, 'pave_floor_plan')


STATE_FIELDS = ('slot_id', 'slot_last', 'slot_hits', 'slot_pos', 'slot_vel', 'slot_travel', 'frame', 'dropped')


def test_c_entry_refuses_bad_plans_before_any_device_call():
    """No GPU: every refusal is PAVE_E_ARG with a message (the addresses are never dereferenced)."""
    native, lib = _lib()
    host = (ctypes.c_ubyte * 64)()
    addr = ctypes.addressof(host)

    def plan(entries=2, n=3, K=15, S=8, cameras=2, camera=1, scale=(1.0, 1.0), max_age=30, anchor=0, anchor_kpts=(13, 14),
             velocity_gain=4, near=1500, unit=10, origin=(0, 0), kpts=addr, bboxes=addr, ids=addr, keep=None, **over):
        p = native.FloorPlan()
        for i in range(min(max(entries, 0), 32)):
            p.kpts[i], p.bboxes[i], p.ids[i], p.keep[i] = kpts, bboxes, ids, keep
            p.out[i], p.out_floor[i] = over.get('out', addr), over.get('out_floor', addr)
            p.n[i], p.camera[i], p.scale[i][0], p.scale[i][1] = n, camera, scale[0], scale[1]
        for f in STATE_FIELDS + ('calib',):
            setattr(p, f, over.get(f, addr))
        for i, k in enumerate(anchor_kpts[:4]):
            p.anchor_kpt[i] = k
        p.entries, p.cameras, p.S, p.K, p.max_age = entries, cameras, S, K, max_age
        p.anchor, p.n_anchor = anchor, len(anchor_kpts)
        p.velocity_gain, p.near, p.unit, p.origin_x, p.origin_y = velocity_gain, near, unit, origin[0], origin[1]
        p.score_thr, p.kpt_thr = 0.3, 0.0
        return p

    def refused(p, needle):
        assert lib.pave_floor_update(ctypes.byref(p) if p is not None else None, None) == native.DEFINES['PAVE_E_ARG'] == -1
        assert needle in lib.pave_last_error().decode(), lib.pave_last_error()

    refused(None, 'null plan')
    refused(plan(entries=0), 'frames per launch')
    refused(plan(entries=33), 'frames per launch')
    refused(plan(kpts=None), 'null pose')
    refused(plan(bboxes=None), 'null pose')
    refused(plan(ids=None), 'null ids')
    refused(plan(out=None), 'null output')
    refused(plan(out_floor=None), 'null output')
    refused(plan(calib=None), 'null calibration')
    for f in STATE_FIELDS:
        refused(plan(**{f: None}), 'null state')
    for kw, needle in ((dict(n=-1), 'N outside'), (dict(n=129), 'N outside'), (dict(K=0), 'K outside'), (dict(K=33), 'K outside'),
                       (dict(S=0), 'max_tracks'), (dict(S=129), 'max_tracks'), (dict(cameras=0), 'cameras outside'),
                       (dict(cameras=4097), 'cameras outside'), (dict(camera=-1), 'camera index'), (dict(camera=2), 'camera index'),
                       (dict(max_age=-1), 'max_age'), (dict(velocity_gain=0), 'velocity_gain'), (dict(velocity_gain=17), 'velocity_gain'),
                       (dict(near=-1), 'near'), (dict(near=2 ** 20 + 1), 'near'), (dict(unit=0), 'unit'), (dict(unit=1001), 'unit'),
                       (dict(origin=(2 ** 20, 0)), 'origin'), (dict(origin=(0, -2 ** 20)), 'origin'),
                       (dict(anchor=-1), 'anchor outside'), (dict(anchor=3), 'anchor outside'),
                       (dict(anchor_kpts=(0, 1, 2, 3, 4)), 'n_anchor'), (dict(anchor_kpts=(13, 15)), 'anchor key point'),
                       (dict(K=14), 'anchor key point')):
        refused(plan(**kw), needle)
    for bad in ((0.0, 1.0), (1.0, -1.0), (float('nan'), 1.0), (1.0, float('inf'))):
        refused(plan(scale=bad), 'scale')


def test_calls_raise_value_errors_on_host_tensors():
    """Shape, type and range checks, and the host-tensor check itself, are ValueErrors raised before anything is
    allocated on or asked of a device."""
    from pavenet_amd import ops
    from pavenet_amd.floor import GroundPlane
    kp, bb, keep = torch.zeros(3, 15, 3), torch.zeros(3, 5), torch.ones(3, dtype=torch.int32)
    ids = torch.ones(3, dtype=torch.int32)
    res = (bb, None, kp)
    m = GroundPlane(15, cameras=2)
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
            (lambda: m.calibration(2), 'camera'),
            (lambda: m.state(-1), 'camera')):
        with pytest.raises(ValueError, match=needle):
            call()
    assert m._state is None

    def state(cameras=2, S=8, **over):
        z = dict(dtype=torch.int32)
        s = dict(id=torch.zeros(cameras, S, **z), last=torch.zeros(cameras, S, **z), hits=torch.zeros(cameras, S, **z),
                 pos=torch.zeros(cameras, S, 2, **z), vel=torch.zeros(cameras, S, 2, **z), travel=torch.zeros(cameras, S, **z),
                 frame=torch.zeros(cameras, **z), dropped=torch.zeros(cameras, **z))
        s.update(over)
        return s

    def update(entries=((kp, bb, None, ids, 0, (1.0, 1.0)),), st=None, calib=None, K=15, **kw):
        return ops.floor_update(entries, state() if st is None else st,
                                torch.zeros(2, 16, dtype=torch.int64) if calib is None else calib, K=K, **kw)
    for call, needle in (
            (lambda: update(st=dict(id=bb)), 'state holds'),
            (lambda: update(st=state(id=torch.zeros(2, dtype=torch.int32))), 'state id'),
            (lambda: update(st=state(S=129)), 'S in'),
            (lambda: update(K=33), 'K'),
            (lambda: update(K=15.0), 'K must be'),
            (lambda: update(st=state(pos=torch.zeros(2, 8, 2))), 'state pos'),
            (lambda: update(st=state(vel=torch.zeros(2, 8, dtype=torch.int32))), 'state vel'),
            (lambda: update(st=state(hits=torch.zeros(2, 9, dtype=torch.int32))), 'state hits'),
            (lambda: update(st=state(frame=torch.zeros(3, dtype=torch.int32))), 'state frame'),
            (lambda: update(calib=torch.zeros(2, 16, dtype=torch.int32)), 'calib'),
            (lambda: update(calib=torch.zeros(3, 16, dtype=torch.int64)), 'calib'),
            (lambda: update(calib=7), 'calib'),
            (lambda: update(velocity_gain=0), 'velocity_gain'),
            (lambda: update(velocity_gain=17), 'velocity_gain'),
            (lambda: update(near=2 ** 20 + 1), 'near'),
            (lambda: update(near=1.0), 'near'),
            (lambda: update(unit=0), 'unit'),
            (lambda: update(unit=1001), 'unit'),
            (lambda: update(origin=5), 'origin'),
            (lambda: update(origin=(0, 2 ** 20)), 'origin'),
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


def test_not_built_sentences_point_to_section_23():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    from pavenet_amd import floor, heatmap, trails
    with open(os.path.join(root, 'README.md')) as f:
        readme = f.read()
    with open(os.path.join(root, 'DESIGN.md')) as f:
        design = f.read()
    for doc in (heatmap.__doc__, trails.__doc__):
        assert 'GroundPlane' in doc
    assert '## 23. The ground plane' in design and 'On the floor' in readme and "out['floor']" in readme
    for word in ('lens distortion', 'vanishing points', 'across cameras'):
        assert word in floor.__doc__.lower() or word in floor.__doc__
