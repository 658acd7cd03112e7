"""Zones, lines and counts in the picture, the parts that need no GPU: the rule of DESIGN section 19 on its numpy
statement (tests/zone_draw_ref.py) with values worked out by hand, the fill tied pixel by pixel to the monitor's own
inside test (tests/zones_ref.py), the plan's C layout, and every refusal of the C entry points and of the Python
wrappers."""
import ctypes
import math
import os
import shutil
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import zone_draw_ref as RD
from tests import zones_cases as ZC
from tests import zones_ref as ZR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def font():
    from pavenet_amd.overlay import ZONE_FONT
    return ZONE_FONT


def style(**kw):
    """ZoneStyle's fields as plain data, every feature off unless asked for."""
    base = dict(zone_colors=[(10 * z + 5, 20 * z + 3, 200 - 9 * z) for z in range(8)],
                line_colors=[(250 - 7 * l, 11 * l + 40, 30 + 5 * l) for l in range(8)], alert_color=(36, 36, 242),
                label_color=(255, 255, 255), alpha=0, alpha_occupied=0, alpha_alert=0, outline=0, thickness=1, arrow=0,
                label_scale=0, zone_label='none', line_label='none')
    base.update(kw)
    return SimpleNamespace(**base)


def scene(zones=(), lines=(), S=4, **counters):
    """(geometry, counts, state) of one camera as the oracle's arrays; counters by name, e.g. occupancy=[1, 0]."""
    ref = ZR.ZoneRef(1, max_tracks=S)
    ref.set_zones(0, list(zones), list(lines))
    for name, values in counters.items():
        a = getattr(ref, name)[0]
        a.reshape(-1)[:np.asarray(values).size] = np.asarray(values, np.int64).astype(np.int32).reshape(-1)
    return ref.geometry(0), ref.counts(0), ref.state(0)


U_SHAPE = [(0, 0), (30, 0), (30, 30), (20, 30), (20, 10), (10, 10), (10, 30), (0, 30)]
RING = [(100 + 50 * math.cos(i * math.pi / 8), 100 + 50 * math.sin(i * math.pi / 8)) for i in range(16)]
SMALL_RING = [(20 + 11 * math.cos(i * math.pi / 8), 12 + 11 * math.sin(i * math.pi / 8)) for i in range(16)]
ODD = [(3.125, 2.375), (35.625, 5.875), (30.375, 21.125), (8.875, 18.625)]


@pytest.mark.parametrize('polygon', [ZC.SQUARE, U_SHAPE, RING, SMALL_RING, ODD],
                         ids=['square', 'concave_u', 'ring', 'small_ring', 'odd_eighths'])
def test_fill_is_the_monitors_inside_test(polygon):
    """A pixel is tinted iff an anchor standing on it would count: every pixel of a 40 x 24 picture against
    tests/zones_ref.py's own test at (8 px, 8 py)."""
    q = [tuple(ZR.quantise(p)) for p in polygon]
    mask = RD.fill_mask(40, 24, q)
    want = np.array([[ZR.inside((8 * px, 8 * py), q) for px in range(40)] for py in range(24)])
    assert np.array_equal(mask, want)
    if polygon is ZC.SQUARE:      # the left and top edges are in, the right and bottom edges out
        assert mask[10:20, 10:20].all() and mask.sum() == 100
    if polygon is U_SHAPE:
        assert mask[5, 15] and not mask[20, 15] and mask[20, 5] and mask[20, 25] and not mask[20, 10] and mask[20, 20]
    if polygon in (SMALL_RING, ODD):
        assert 0 < mask.sum() < mask.size


def test_blend_values_by_hand():
    assert RD.blend(255, 0, 128) == 128 and RD.blend(7, 200, 0) == 7 and RD.blend(7, 200, 256) == 200
    assert RD.blend(0, 255, 1) == 1 and RD.blend(100, 50, 48) == (100 * 208 + 50 * 48 + 128) >> 8 == 91
    img = np.full((24, 40, 3), 255, np.uint8)
    geo, cnt, st = scene([ZC.SQUARE])
    black = [(0, 0, 0)] * 8
    assert np.array_equal(RD.draw_bgr(img, geo, cnt, st, style(alpha=0, zone_colors=black), font()), img)   # a = 0: nothing
    out = RD.draw_bgr(img, geo, cnt, st, style(alpha=128, zone_colors=black), font())
    assert (out[10:20, 10:20] == 128).all() and (out == 128).sum() == 300 and (out[0] == 255).all()
    s = style(alpha=256)
    out = RD.draw_bgr(img, geo, cnt, st, s, font())
    assert (out[10:20, 10:20] == s.zone_colors[0]).all()                                   # a = 256: the colour
    # occupied: alpha_occupied instead of alpha
    geo, cnt, st = scene([ZC.SQUARE], occupancy=[2])
    out = RD.draw_bgr(img, geo, cnt, st, style(alpha=256, alpha_occupied=128, zone_colors=black), font())
    assert (out[10:20, 10:20] == 128).all()


def test_overlapping_zones_composite_in_ascending_index():
    a, b = [(0, 0), (6, 0), (6, 4), (0, 4)], [(3, 0), (8, 0), (8, 4), (3, 4)]
    img = np.full((4, 8, 3), 200, np.uint8)
    s = style(alpha=128, zone_colors=[(0, 0, 0), (255, 255, 255)] + [(9, 9, 9)] * 6)
    out = RD.draw_bgr(img, *scene([a, b]), s, font())
    first = RD.blend(200, 0, 128)
    assert first == 100 and (out[:, :3] == 100).all() and (out[:, 6:] == RD.blend(200, 255, 128)).all()
    assert (out[:, 3:6] == RD.blend(first, 255, 128)).all() and RD.blend(first, 255, 128) == 178
    swapped = RD.draw_bgr(img, *scene([b, a]), SimpleNamespace(**{**vars(s), 'zone_colors': s.zone_colors[1::-1] + s.zone_colors[2:]}),
                          font())
    assert (swapped[:, 3:6] == RD.blend(RD.blend(200, 255, 128), 0, 128)).all() and swapped[0, 4, 0] == 114
    assert not np.array_equal(out, swapped)


@pytest.mark.parametrize('n, polygon', [(1, [(0, 0), (1, 0), (1, 1), (0, 1)]), (2, [(0, 0), (2, 0), (2, 1), (0, 1)]),
                                        (3, [(0, 0), (2, 0), (2, 1), (1, 1), (1, 2), (0, 2)]),
                                        (4, [(0, 0), (2, 0), (2, 2), (0, 2)])])
def test_nv12_chroma_alpha_by_covered_luma_pixels(n, polygon):
    """a_c = (a n + 2) >> 2 for the n luma pixels of the sample inside the zone; pitch padding is never written."""
    from tests import render_ref as RR
    surf = np.full((6, 8), 60, np.uint8)            # 4 x 4 picture, pitch 8
    s = style(alpha=101)
    out = RD.draw_nv12(surf, 4, *scene([polygon]), s, font())
    y, u, v = RR.bgr_to_yuv(s.zone_colors[0], 'bt601', False)
    assert RD.fill_mask(4, 4, [tuple(ZR.quantise(p)) for p in polygon]).sum() == n
    assert (out[:4, :4] == RD.blend(60, y, 101)).sum() == n and (out[:4, :4] == 60).sum() == 16 - n
    ac = (101 * n + 2) >> 2
    assert ac == {1: 25, 2: 51, 3: 76, 4: 101}[n]
    assert out[4, 0] == RD.blend(60, u, ac) and out[4, 1] == RD.blend(60, v, ac)
    rest = out.copy()
    rest[:2, :2], rest[4, :2] = 60, 60
    assert (rest == 60).all()


def test_label_glyphs_plates_and_the_minus():
    assert font()[10] == (0, 0, 0, 31, 0, 0, 0) and len(font()) == 11
    line = [((8, 40), (8, 20))]                      # upwards: the stem points to the right
    for v, faces in ((0, [0]), (9, [9]), (10, [1, 0]), (99999, [9] * 5), (2 ** 31 - 1, [2, 1, 4, 7, 4, 8, 3, 6, 4, 7]),
                     (-1, [10, 1]), (-2 ** 31, [10, 2, 1, 4, 7, 4, 8, 3, 6, 4, 8])):
        assert RD.glyphs(v) == faces
        crossed = [v, 0] if v >= 0 else ([0, 1] if v == -1 else [-2 ** 31, 0])
        for g in (1, 3):
            _, labels = RD.primitives(*scene([], line, crossed=crossed), style(label_scale=g, line_label='net'))
            (plate, (ax, ay, Wp, Hp), got, row), = labels
            assert plate == 160 and got == faces and row == 8 and (Wp, Hp) == (g * (6 * len(faces) + 1), 9 * g)
            assert (ax, ay) == (max(8 - Wp // 2, 0), 30 - Hp // 2)       # no stem: centred on M = (8, 30)
    # the ink of -1 at g = 1: the minus bar in row 3 of the first cell, then the 1
    ids, rows = RD.id_map(40, 60, *scene([], line, crossed=[0, 1]), style(label_scale=1, line_label='net'), font())
    ax, ay = 8 - 13 // 2, 30 - 4
    ink = ids[ay + 1:ay + 8, ax + 1:ax + 12] == 161
    assert ink[3, :5].all() and ink[:, :5].sum() == 5 and not ink[:, 5].any() and ink[:, 6:11].sum() == 10
    assert rows[160] == 8 and rows[161] == RD.INK
    # zone labels: occupancy, or entered + appeared (wrapping as the counters do)
    z = [(8, 8), (24, 8), (24, 24), (8, 24)]
    sc = scene([z], occupancy=[7], entered=[2 ** 31 - 1], appeared=[1])
    assert RD.primitives(*sc, style(label_scale=2, zone_label='occupancy'))[1][0][2] == [7]
    assert RD.primitives(*sc, style(label_scale=2, zone_label='entered'))[1][0][2] == RD.glyphs(-2 ** 31)
    assert RD.primitives(*sc, style(label_scale=2, zone_label='occupancy'))[1][0][1] == (16 - 7, 16 - 9, 14, 18)
    assert RD.primitives(*sc, style(label_scale=0, zone_label='occupancy'))[1] == []
    for kind, want in (('forward', [5]), ('backward', [1, 2]), ('net', [10, 7])):
        assert RD.primitives(*scene([], line, crossed=[5, 12]), style(label_scale=1, line_label=kind))[1][0][2] == want


def test_plate_is_clamped_at_the_left_and_top_and_clipped_at_the_right_and_bottom():
    s = style(label_scale=2, zone_label='occupancy', alpha=0)
    img = np.zeros((20, 30, 3), np.uint8)
    corner = [(0, 0), (4, 0), (4, 4), (0, 4)]        # centre (2, 2): the corner would be (-5, -7)
    (_, plate, _, _), = RD.primitives(*scene([corner]), s)[1]
    assert plate == (0, 0, 14, 18)
    out = RD.draw_bgr(img, *scene([corner]), s, font())
    assert (out[:18, :14] != 0).any(axis=2).all() and not out[18:].any() and not out[:, 14:].any()
    far = [(26, 16), (30, 16), (30, 20), (26, 20)]   # centre (28, 18): corner (21, 9), 14 x 18: cut at 30 and 20
    (_, plate, _, _), = RD.primitives(*scene([far]), s)[1]
    assert plate == (21, 9, 14, 18)
    out = RD.draw_bgr(img, *scene([far]), s, font())
    assert (out[9:, 21:] != 0).any(axis=2).all() and not out[:9].any() and not out[:, :21].any()
    ids, _ = RD.id_map(30, 20, *scene([far]), s, font())
    assert (ids[9:, 21:] >= 144).all() and (ids == 145).sum() > 0


def test_stem_points_the_way_a_forward_crossing_goes():
    A, B = (10, 10), (30, 10)                         # to the right: forward is downwards (y grows)
    M, T, drawn = RD.stem_of(((80, 80), (240, 80)), 6)
    assert (M, T, drawn) == ((80, 40), (80, 64), True)
    # T is on the side where section 17's s is true and a point mirrored about the line is not: Q -> T crosses forward
    G = lambda q: (2 * q[0], 2 * q[1])
    a, b = tuple(ZR.quantise(A)), tuple(ZR.quantise(B))
    assert ZR.side(a, b, G(T)) and not ZR.side(a, b, G((80, 16))) and ZR.crossing(G((80, 16)), G(T), a, b) == ZR.CROSS_FWD
    # a slanted line: trunc towards zero on both signs, L = isqrt(d.d)
    M, T, drawn = RD.stem_of(((800, 800), (856, 888)), 10)  # Q: (400, 400) -> (428, 444); d.d = 2720, L = 52
    assert M == (414, 422) and T == (414 - (44 * 40) // 52, 422 + (28 * 40) // 52) == (414 - 33, 422 + 21) and drawn
    assert RD.stem_of(((0, 0), (56, 88)), 10)[1] == (0, 22 + 21)             # clamped at 0
    M, T, drawn = RD.stem_of(((400, 400), (400, 0)), 255)   # upwards: to the right, 1020 quarter pixels
    assert T == (200 + 1020, 100)
    assert RD.stem_of(((65535, 0), (65535, 65535)), 255)[1] == (32767 - 1020, 16383)
    assert RD.stem_of(((0, 0), (0, 65535)), 255)[1] == (0, 16383)          # clamped at 0
    assert RD.stem_of(((80, 80), (240, 80)), 0) == ((80, 40), (80, 40), False)   # arrow = 0
    # ends that are two points in 1/8 pixel and one in quarter pixels: no stem, the label on M
    geo, cnt, st = scene([], [((10, 10), (10.125, 10))])
    assert RD.stem_of(tuple(tuple(int(v) for v in p) for p in geo['lines'][0]), 24) == ((40, 40), (40, 40), False)
    caps, labels = RD.primitives(geo, cnt, st, style(arrow=24, label_scale=1, line_label='net', thickness=2))
    assert [c[0] for c in caps] == [128] and caps[0][1] == caps[0][2] == (40, 40) and caps[0][3] == 4
    assert labels[0][1][:2] == (10 - 3, 10 - 4)
    caps, labels = RD.primitives(*scene([], [(A, B)]), style(arrow=6, label_scale=1, line_label='net'))
    assert [c[0] for c in caps] == [128, 136] and caps[1][1:3] == ((80, 40), (80, 64)) and labels[0][1][:2] == (20 - 3, 16 - 4)


def test_painters_order():
    """Ink over plate over stem over line over outline over fill, at pixel (20, 12)."""
    zones = [[(4, 4), (36, 4), (36, 20), (4, 20)], [(20, 4), (36, 4), (36, 20), (20, 20)]]
    lines = [((4, 12), (36, 12))]
    full = dict(alpha=64, outline=1, thickness=1, arrow=1, label_scale=1, line_label='forward')
    at = lambda zs, ls, **kw: int(RD.id_map(40, 24, *scene(zs, ls, crossed=[1, 0]), style(**kw), font())[0][12, 20])
    assert at(zones, lines, **full) == 161                                       # the 1's middle column
    assert at(zones, lines, **{**full, 'line_label': 'backward'}) == 160         # a 0 has no ink there: the plate
    assert at(zones, lines, **{**full, 'label_scale': 0}) == 136
    assert at(zones, lines, **{**full, 'label_scale': 0, 'arrow': 0}) == 128
    assert at(zones, [], **full) == 16 + 3                                       # zone 1's left edge, vertex 3 -> 0
    assert at(zones, [], **{**full, 'outline': 0}) == -1
    img = np.full((24, 40, 3), 90, np.uint8)
    s = style(**{**full, 'outline': 0})
    out = RD.draw_bgr(img, *scene(zones, []), s, font())
    want = [RD.blend(RD.blend(90, s.zone_colors[0][c], 64), s.zone_colors[1][c], 64) for c in range(3)]
    assert out[12, 20].tolist() == want and out[12, 19].tolist() == [RD.blend(90, s.zone_colors[0][c], 64) for c in range(3)]
    out = RD.draw_bgr(img, *scene(zones, lines, crossed=[1, 0]), style(**full), font())
    assert out[12, 20].tolist() == [255, 255, 255] and out[12, 18].tolist() == list(style().line_colors[0])
    assert out[2, 2].tolist() == [90, 90, 90]
    # NV12: a chroma sample takes the largest id over its 2 x 2 luma pixels
    from tests import render_ref as RR
    surf = np.full((36, 40), 90, np.uint8)
    out = RD.draw_nv12(surf, 40, *scene(zones, lines, crossed=[1, 0]), style(**full), font(), 'bt709', True)
    assert out[12, 20] == 255 and out[24 + 6, 20:22].tolist() == list(RR.bgr_to_yuv((255, 255, 255), 'bt709', True)[1:])


def test_alert_needs_a_live_slot_with_both_bits():
    zones = [ZC.SQUARE, [(22, 10), (32, 10), (32, 20), (22, 20)]]
    img = np.full((24, 40, 3), 255, np.uint8)
    s = style(alpha=64, alpha_occupied=100, alpha_alert=256, outline=1)
    geo, cnt, st = scene(zones, occupancy=[1, 1])
    plain = RD.draw_bgr(img, geo, cnt, st, s, font())
    assert plain[15, 15].tolist() == [RD.blend(255, c, 100) for c in s.zone_colors[0]]
    for ident, inside, alerted, want in ((7, 2, 2, [False, True]), (7, 3, 1, [True, False]), (7, 1, 2, [False, False]),
                                         (0, 3, 3, [False, False]), (-5, 3, 3, [True, True])):
        st['id'][2], st['inside'][2], st['alerted'][2] = ident, inside, alerted
        got = [row == RD.ALERT for row, _ in RD.zone_states(2, cnt, st, s)]
        assert got == want, (ident, inside, alerted)
        out = RD.draw_bgr(img, geo, cnt, st, s, font())
        assert (out[15, 15].tolist() == list(s.alert_color)) == want[0]
        assert (out[15, 27].tolist() == list(s.alert_color)) == want[1]
        assert (out[10, 15].tolist() == list(s.alert_color)) == want[0]          # the outline takes the state's colour
        if not any(want):
            assert np.array_equal(out, plain)                                    # a free slot's bits change nothing


# ---- the library ----

def _lib():
    from pavenet_amd import native
    from pavenet_amd.build_native import build_native
    build_native()
    return native, native.load()


def test_zone_draw_plan_layout_and_entries(tmp_path):
    """native.ZoneDrawPlan is the header's pave_zone_draw_plan field for field, well under the 4 KB kernel-argument
    limit, and the two entries are in the header, the binding and both libraries at ABI 21."""
    native, lib = _lib()
    vp, ci = ctypes.c_void_p, ctypes.c_int
    for entry in ('pave_draw_zones_nv12', 'pave_draw_zones_bgr'):
        assert native.FUNCTIONS[entry] == (ci, [vp, vp]) and entry in native.SIGNATURES and hasattr(lib, entry)
        for path in (native.LIB_PATH, native.DIAG_LIB_PATH):
            out = subprocess.run(['nm', '-D', '--defined-only', path], capture_output=True, text=True, check=True).stdout
            assert entry in {ln.split()[-1] for ln in out.splitlines()}
    assert native.ABI_VERSION == 21 and lib.pave_abi_version() == 21
    assert ctypes.sizeof(native.ZoneDrawPlan) == 1184 < 2048
    if not shutil.which('gcc'):
        pytest.skip('no gcc')
    fields = [f for f, _ in native.ZoneDrawPlan._fields_]
    src = tmp_path / 'layout.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pave_hip.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(pave_zone_draw_plan));\n'
                   + ''.join(f'  printf(" %zu", offsetof(pave_zone_draw_plan, {f}));\n' for f in fields)
                   + '  return 0;\n}\n')
    exe = tmp_path / 'layout'
    subprocess.run(['gcc', '-std=c99', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == ctypes.sizeof(native.ZoneDrawPlan)
    assert got[1:] == [getattr(native.ZoneDrawPlan, f).offset for f in fields]


MONITOR_FIELDS = ('geometry', 'counters', 'slot_id', 'slot_alerted', 'slot_inside')


@pytest.mark.parametrize('entry, bpp', [('pave_draw_zones_nv12', 1), ('pave_draw_zones_bgr', 3)])
def test_c_entries_refuse_bad_plans_before_any_device_call(entry, bpp):
    """No GPU: every refusal is PAVE_E_ARG with a message (the addresses are never dereferenced)."""
    native, lib = _lib()
    host = (ctypes.c_ubyte * 64)()
    addr = ctypes.addressof(host)

    def plan(n=2, dst=addr, width=64, height=48, pitch=None, camera=1, table=0, cameras=2, S=8, font_bits=0, **kw):
        p = native.ZoneDrawPlan()
        for i in range(min(max(n, 0), 32)):
            p.dst[i], p.width[i], p.height[i], p.camera[i], p.table[i] = dst, width, height, camera, table
            p.pitch[i] = bpp * width if pitch is None else pitch
        for f in MONITOR_FIELDS:
            setattr(p, f, kw.pop(f, addr))
        p.n, p.cameras, p.S = n, cameras, S
        values = dict(alpha=48, alpha_occupied=96, alpha_alert=128, outline=2, thickness=3, arrow=24, label_scale=2,
                      zone_label=1, line_label=1)
        values.update(kw)
        for name, v in values.items():
            setattr(p, name, v)
        for d, face in enumerate(font()):
            for r, bits in enumerate(face):
                p.font[d][r] = bits
        p.font[10][6] |= font_bits
        return p

    def refused(p, needle):
        assert getattr(lib, entry)(ctypes.byref(p) if p is not None else None, None) == native.DEFINES['PAVE_E_ARG'] == -1
        assert needle in lib.pave_last_error().decode(), lib.pave_last_error()

    refused(None, 'null plan')
    refused(plan(n=0), 'surfaces per launch')
    refused(plan(n=33), 'surfaces per launch')
    refused(plan(dst=None), 'null surface')
    for f in MONITOR_FIELDS:
        refused(plan(**{f: None}), 'null monitor')
    for w, h in ((0, 48), (64, 0), (8193, 48), (64, 8193), (-2, 48)):
        refused(plan(width=w, height=h, pitch=1 << 20), 'width and height')
    if bpp == 1:
        refused(plan(width=63), 'must be even')
        refused(plan(height=47), 'must be even')
    refused(plan(pitch=bpp * 64 - 1), 'pitch below')
    refused(plan(table=4), 'table index')
    refused(plan(cameras=0), 'cameras outside')
    refused(plan(cameras=4097), 'cameras outside')
    refused(plan(camera=-1), 'camera index')
    refused(plan(camera=2), 'camera index')
    refused(plan(S=0), 'max_tracks')
    refused(plan(S=129), 'max_tracks')
    for name in ('alpha', 'alpha_occupied', 'alpha_alert'):
        refused(plan(**{name: -1}), 'alpha outside')
        refused(plan(**{name: 257}), 'alpha outside')
    for name, lo, hi in (('outline', 0, 32), ('thickness', 1, 32), ('arrow', 0, 255), ('label_scale', 0, 8),
                         ('zone_label', 0, 2), ('line_label', 0, 3)):
        refused(plan(**{name: lo - 1}), f'{name} outside')
        refused(plan(**{name: hi + 1}), f'{name} outside')
    refused(plan(font_bits=0x20), 'font row')
    refused(plan(font_bits=0x80), 'font row')


def test_wrappers_raise_value_errors_before_anything_is_asked_of_a_device():
    from pavenet_amd import ZoneStyle, draw_zones_bgr, draw_zones_nv12, native, ops
    from pavenet_amd.overlay import ZONE_COLORS, ZONE_FONT
    from pavenet_amd.zones import ZoneMonitor
    s = ZoneStyle()
    assert (s.alpha, s.alpha_occupied, s.alpha_alert, s.outline, s.thickness, s.arrow, s.label_scale) == (48, 96, 128, 2, 3, 24, 2)
    assert (s.zone_label, s.line_label, s.alert_color, s.label_color) == ('occupancy', 'net', (36, 36, 242), (255, 255, 255))
    assert len(s.table_bytes()) == len(s.table_bytes('bt709', True)) == 54 and s.table_bytes()[:3] == bytes(ZONE_COLORS[0])
    assert s.table_bytes('bt601') is s.table_bytes('bt601') and s.table_bytes('bt601') != s.table_bytes('bt709')
    for kw, needle in ((dict(zone_colors=ZONE_COLORS[:7]), 'zone_colors'), (dict(line_colors=None), 'line_colors'),
                       (dict(zone_colors=[(1, 2)] * 8), 'zone_colors'), (dict(line_colors=[(1, 2, 256)] * 8), 'line_colors'),
                       (dict(alert_color=(1, 2)), 'alert_color'), (dict(label_color='white'), 'label_color'),
                       (dict(alpha=-1), 'alpha'), (dict(alpha=257), 'alpha'), (dict(alpha=1.0), 'alpha'),
                       (dict(alpha_occupied=257), 'alpha_occupied'), (dict(alpha_alert=-1), 'alpha_alert'),
                       (dict(outline=33), 'outline'), (dict(outline=-1), 'outline'), (dict(thickness=0), 'thickness'),
                       (dict(thickness=33), 'thickness'), (dict(arrow=256), 'arrow'), (dict(arrow=-1), 'arrow'),
                       (dict(label_scale=9), 'label_scale'), (dict(label_scale=True), 'label_scale'),
                       (dict(zone_label='net'), 'zone_label'), (dict(line_label='occupancy'), 'line_label')):
        with pytest.raises(ValueError, match=needle):
            ZoneStyle(**kw)
    mon = ZoneMonitor(15, cameras=2)
    nv, bgr = torch.zeros(72, 64, dtype=torch.uint8), torch.zeros(48, 64, 3, dtype=torch.uint8)
    for call, needle in (
            (lambda: draw_zones_nv12(nv, 64, object()), 'ZoneMonitor'),
            (lambda: draw_zones_bgr(bgr, None), 'ZoneMonitor'),
            (lambda: draw_zones_nv12(nv, 64, mon, camera=2), 'camera'),
            (lambda: draw_zones_bgr(bgr, mon, camera=-1), 'camera'),
            (lambda: draw_zones_bgr([bgr, bgr], mon, camera=[0, 1, 0]), 'camera'),
            (lambda: draw_zones_nv12(nv, 64, mon, style=object()), 'ZoneStyle'),
            (lambda: draw_zones_nv12([], 64, mon), 'uint8 tensor'),
            (lambda: draw_zones_nv12(nv.float(), 64, mon), 'uint8 tensor'),
            (lambda: draw_zones_nv12(nv, 63, mon), 'even'),
            (lambda: draw_zones_nv12(torch.zeros(70, 64, dtype=torch.uint8), 64, mon), 'even height'),
            (lambda: draw_zones_nv12(nv, 66, mon), 'pitch'),
            (lambda: draw_zones_nv12(nv, [64, 64], mon), 'width'),
            (lambda: draw_zones_nv12(nv, 64, mon, matrix='bt2020'), 'matrix'),
            (lambda: draw_zones_nv12(bgr, 64, mon), 'pitch'),
            (lambda: draw_zones_bgr(nv, mon), r'\[H, W, 3\]'),
            (lambda: draw_zones_nv12(nv, 64, mon), 'HIP device'),
            (lambda: draw_zones_bgr(bgr, mon), 'HIP device')):
        with pytest.raises(ValueError, match=needle):
            call()
    assert mon._state is None and mon.device_tensors() is None

    def state(cameras=2, S=8, **over):
        z = dict(dtype=torch.int32)
        st = dict(geometry=torch.zeros(cameras, native.ZONE_GEOM_WORDS, **z), counters=torch.zeros(cameras, 56, **z),
                  id=torch.zeros(cameras, S, **z), alerted=torch.zeros(cameras, S, **z), inside=torch.zeros(cameras, S, **z))
        st.update(over)
        return st

    tables = [s.table_bytes()]

    def draw(kind='bgr', items=None, st=None, tabs=tables, face=ZONE_FONT, **kw):
        return ops.draw_zones(kind, [(bgr, None, 0, 0)] if items is None else items, state() if st is None else st, tabs,
                              face, **kw)
    for call, needle in (
            (lambda: draw('rgb'), 'kind'),
            (lambda: draw(items=[]), 'no surface'),
            (lambda: draw(items=[(bgr, None, 0)]), 'an item is'),
            (lambda: draw(alpha=257), 'alpha'), (lambda: draw(alpha_occupied=-1), 'alpha_occupied'),
            (lambda: draw(alpha_alert=2.0), 'alpha_alert'), (lambda: draw(outline=33), 'outline'),
            (lambda: draw(thickness=0), 'thickness'), (lambda: draw(arrow=256), 'arrow'),
            (lambda: draw(label_scale=9), 'label_scale'), (lambda: draw(zone_label='net'), 'zone_label'),
            (lambda: draw(line_label=1), 'line_label'),
            (lambda: draw(face=ZONE_FONT[:10]), 'font'),
            (lambda: draw(face=ZONE_FONT[:10] + ((32, 0, 0, 0, 0, 0, 0),)), 'font'),
            (lambda: draw(tabs=[]), 'tables'), (lambda: draw(tabs=[b'x' * 53]), 'tables'), (lambda: draw(tabs=tables * 5), 'tables'),
            (lambda: draw(st=dict(id=bgr)), 'state holds'),
            (lambda: draw(st=state(id=torch.zeros(2, 8, 1, dtype=torch.int32))), 'state id'),
            (lambda: draw(st=state(S=129)), 'S in'),
            (lambda: draw(st=state(geometry=torch.zeros(2, 305, dtype=torch.int32))), 'state geometry'),
            (lambda: draw(st=state(counters=torch.zeros(2, 56))), 'state counters'),
            (lambda: draw(st=state(alerted=torch.zeros(2, 7, dtype=torch.int32))), 'state alerted'),
            (lambda: draw(st=state(inside=torch.zeros(3, 8, dtype=torch.int32))), 'state inside'),
            (lambda: draw(items=[(bgr.float(), None, 0, 0)]), 'uint8'),
            (lambda: draw(items=[(nv, None, 0, 0)]), r'\[H, W, 3\]'),
            (lambda: draw('nv12', items=[(bgr, 64, 0, 0)]), 'pitch'),
            (lambda: draw('nv12', items=[(nv, 64.0, 0, 0)]), 'width'),
            (lambda: draw('nv12', items=[(nv, 62, 0, 0), (nv, 63, 0, 0)]), 'surface 1: width 63'),
            (lambda: draw('nv12', items=[(nv, 66, 0, 0)]), 'exceeds the pitch'),
            (lambda: draw('nv12', items=[(torch.zeros(70, 64, dtype=torch.uint8), 64, 0, 0)]), 'even height'),
            (lambda: draw(items=[(bgr[:, ::2], None, 0, 0)]), 'contiguous'),
            (lambda: draw(items=[(bgr, None, 2, 0)]), 'camera'), (lambda: draw(items=[(bgr, None, -1, 0)]), 'camera'),
            (lambda: draw(items=[(bgr, None, 0, 1)]), 'colour table'),
            (lambda: draw(), 'HIP device')):
        with pytest.raises(ValueError, match=needle):
            call()
