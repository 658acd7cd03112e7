"""The heat-map overlay, the parts that need no GPU: the draw rule of DESIGN section 21 worked by hand against its numpy
statement (tests/heat_draw_ref.py), the plan's C layout, and every refusal of the two C entries and of the Python
calls."""
import ctypes
import shutil

import numpy as np
import pytest
import torch

from tests import heat_draw_ref as DR
from tests.test_heat_cpu import _lib, layout


class Style:
    """What the oracle reads of a HeatStyle."""

    def __init__(self, source='dwell', palette=None, full_scale=None, alpha_max=160, floor=1, smooth=True):
        self.source, self.full_scale, self.alpha_max, self.floor, self.smooth = source, full_scale, alpha_max, floor, smooth
        self.palette = [(l, 255 - l, l // 2) for l in range(256)] if palette is None else palette


def maps(dwell, visits=None, peak=None):
    dwell = np.asarray(dwell, np.int32)
    visits = np.zeros_like(dwell) if visits is None else np.asarray(visits, np.int32)
    return dict(dwell=dwell, visits=visits,
                peak=np.asarray([dwell.max(), visits.max()] if peak is None else peak, np.int32))


def test_smooth_weights_along_a_three_cell_row():
    """cell 4, three cells: pixel 0 has u = 1, t = -3, i0 = -1, f = 5: both weights fall on cell 0 (the edge cell is
    replicated); pixel 5: u = 11, t = 7, i0 = 0, f = 7: 1 on cell 0 and 7 on cell 1; pixel 6: u = 13, t = 9, i0 = 1, f = 1;
    pixel 11: u = 23, t = 19, i0 = 2, f = 3: 5 and 3, both on cell 2."""
    a, b, w0, w1 = DR.axis_weights(2 * np.arange(12) + 1, 4, 3)
    rows = list(zip(a.tolist(), b.tolist(), w0.tolist(), w1.tolist()))
    assert rows[0] == (0, 0, 3, 5) and rows[5] == (0, 1, 1, 7) and rows[6] == (1, 2, 7, 1) and rows[11] == (2, 2, 5, 3)
    assert all(x + y == 8 for _, _, x, y in rows)
    # levels 0, 80, 240 in one row of cells: (8 (1 * 0 + 7 * 80) + 32) >> 6 = 70, (8 (7 * 80 + 240) + 32) >> 6 = 100
    lv = DR.sample(np.asarray([[0, 80, 240]], np.int64), 2 * np.arange(12) + 1, 2 * np.arange(4) + 1, 4, True)
    assert lv.shape == (4, 12) and (lv == lv[0]).all()
    assert lv[0].tolist() == [0, 0, 10, 30, 50, 70, 100, 140, 180, 220, 240, 240]
    # without smooth a pixel takes its cell
    assert DR.sample(np.asarray([[0, 80, 240]], np.int64), 2 * np.arange(12) + 1, [1], 4, False)[0].tolist() == \
        [0] * 4 + [80] * 4 + [240] * 4


@pytest.mark.parametrize('smooth', [False, True])
@pytest.mark.parametrize('cell', [4, 8, 16, 32, 64])
def test_a_constant_map_gives_a_constant_picture(cell, smooth):
    """Every cell 7 of a full scale of 10: level 178 everywhere, so one alpha and one colour: (160 * 178 + 128) >> 8 =
    111."""
    W, H = 3 * cell + 2, 2 * cell + 1
    m = maps(np.full((3, 4), 7))
    style = Style(full_scale=10, smooth=smooth)
    src = np.full((H, W, 3), 50, np.uint8)
    out = DR.draw_bgr(src, m, (W, H), cell, style)
    want = [(50 * (256 - 111) + c * 111 + 128) >> 8 for c in style.palette[178]]
    assert (out == np.asarray(want, np.uint8)).all()


def test_floor_and_the_ends_of_alpha():
    """Levels 0, 51, 255 in three cells without smooth.  alpha_max 0 writes nothing; alpha_max 256 gives a = level, so
    level 255 leaves 1 / 256 of the source; floor 52 leaves the level-51 cell alone and floor 51 does not."""
    m = maps([[0, 1, 5]])
    src = np.full((4, 12, 3), 200, np.uint8)
    assert (DR.draw_bgr(src, m, (12, 4), 4, Style(alpha_max=0, smooth=False)) == src).all()
    full = Style(alpha_max=256, floor=0, smooth=False)
    out = DR.draw_bgr(src, m, (12, 4), 4, full)
    assert (out[:, :4] == 200).all()                                   # level 0: a = 0
    assert out[0, 4].tolist() == [(200 * (256 - 51) + c * 51 + 128) >> 8 for c in full.palette[51]]
    assert out[0, 8].tolist() == [(200 + c * 255 + 128) >> 8 for c in full.palette[255]]
    assert (DR.draw_bgr(src, m, (12, 4), 4, Style(floor=52, smooth=False))[:, :8] == 200).all()
    assert (DR.draw_bgr(src, m, (12, 4), 4, Style(floor=51, smooth=False))[:, 4:8] != 200).any()
    assert DR.alpha_of(np.asarray([0, 1, 255]), Style(alpha_max=160, floor=0)).tolist() == [0, 1, 159]


def test_scale_saturation_and_negative_words():
    """full_scale 4 below a peak of 9: 255 * 9 / 4 saturates at 255; with None the peak scales: 255 * 3 / 9 = 85; a
    negative word reads as 0; a peak of 0 reads as 1."""
    assert DR.levels([[9, 4, 3, 1, -5]], 4).tolist() == [[255, 255, 191, 63, 0]]
    m = maps([[9, 3, -5]])
    src = np.zeros((4, 12, 3), np.uint8)
    style = Style(alpha_max=256, floor=0, smooth=False)
    out = DR.draw_bgr(src, m, (12, 4), 4, style)
    assert out[0, 4].tolist() == [(c * 85 + 128) >> 8 for c in style.palette[85]] and (out[:, 8:] == 0).all()
    assert DR.levels([[2 ** 31 - 1]], 1).tolist() == [[255]] and DR.levels([[2 ** 31 - 1]], 2 ** 31 - 1).tolist() == [[255]]
    zero = maps([[0, 0, 0]], peak=[0, 0])
    assert (DR.draw_bgr(src, zero, (12, 4), 4, style) == src).all()
    vis = maps([[0, 0, 0]], visits=[[0, 2, 1]])
    out = DR.draw_bgr(src, vis, (12, 4), 4, Style(source='visits', alpha_max=256, floor=0, smooth=False))
    assert (out[:, :4] == 0).all() and (out[:, 4:8] != 0).any() and (out[:, 8:] != out[:, 4:8]).any()


def test_nv12_chroma_of_a_block_with_four_levels():
    """cell 4, levels [[0, 64], [128, 255]] (full scale 255), the block at (2, 2).  Its pixels have f = 1 and 3 on
    either axis and its chroma sample (u = 6) f = 2, so with g(fx, fy) = ((8 - fy)((8 - fx) 0 + fx 64) + fy ((8 - fx) 128
    + fx 255) + 32) >> 6 the lumas are blended at levels g(1, 1) = 25, g(3, 1) = 43, g(1, 3) = 59, g(3, 3) = 81 and the
    chroma sample once at g(2, 2) = 52."""
    m = maps([[0, 64], [128, 255]], peak=[255, 0])
    style = Style(alpha_max=256, floor=0, palette=[(l, 0, 255 - l) for l in range(256)])
    src = np.full((12, 8), 100, np.uint8)
    out = DR.draw_nv12(src, 8, m, (8, 8), 4, style, 'bt709', True)
    yuv = DR.yuv_table(style.palette, 'bt709', True)
    mix = lambda l, ch: (100 * (256 - l) + int(yuv[l, ch]) * l + 128) >> 8
    assert [int(out[2, 2]), int(out[2, 3]), int(out[3, 2]), int(out[3, 3])] == [mix(25, 0), mix(43, 0), mix(59, 0), mix(81, 0)]
    assert [int(out[8 + 1, 2]), int(out[8 + 1, 3])] == [mix(52, 1), mix(52, 2)]
    assert len({25, 43, 59, 81, 52}) == 5 and yuv[52, 1] != yuv[43, 1]
    # without smooth the block lies in cell (0, 0): level 0, nothing written
    flat = DR.draw_nv12(src, 8, m, (8, 8), 4, Style(alpha_max=256, floor=0, smooth=False, palette=style.palette), 'bt709', True)
    assert (flat[:4, :4] == 100).all() and (flat[8:10, :4] == 100).all() and (flat[4:8, 4:8] != 100).all()


def test_pixels_beyond_the_map_are_untouched():
    """A 10 x 6 map (cell 4: 3 x 2 cells) on a 16 x 8 surface: columns from 10 and rows from 6 keep their bytes, luma and
    chroma; an odd map size writes the chroma sample of the block its last column starts."""
    m = maps(np.full((2, 3), 5))
    style = Style(alpha_max=256, floor=0)
    bgr = np.full((8, 16, 3), 9, np.uint8)
    out = DR.draw_bgr(bgr, m, (10, 6), 4, style)
    assert (out[:6, :10] != 9).all(axis=2).all() and (out[6:] == 9).all() and (out[:, 10:] == 9).all()
    nv = np.full((12, 16), 9, np.uint8)
    out = DR.draw_nv12(nv, 16, m, (10, 6), 4, style)
    assert (out[:6, :10] != 9).all() and (out[6:8] == 9).all() and (out[:8, 10:] == 9).all()
    assert (out[8:11, :10] != 9).all() and (out[11] == 9).all() and (out[8:, 10:] == 9).all()
    odd = DR.draw_nv12(nv, 16, m, (9, 5), 4, style)
    assert (odd[:5, :9] != 9).all() and (odd[:8, 9:] == 9).all() and (odd[5:8] == 9).all()
    assert (odd[8:11, :10] != 9).all() and (odd[8:, 10:] == 9).all()
    # a surface smaller than the map shows its top-left part
    small = DR.draw_bgr(np.full((3, 5, 3), 9, np.uint8), m, (10, 6), 4, style)
    assert (small == out_of(bgr, m, style)[:3, :5]).all()


def out_of(bgr, m, style):
    return DR.draw_bgr(bgr, m, (10, 6), 4, style)


def test_heat_draw_plan_layout_and_entries(tmp_path):
    native, lib = _lib()
    vp, ci = ctypes.c_void_p, ctypes.c_int
    for name in ('pave_draw_heat_nv12', 'pave_draw_heat_bgr'):
        assert native.FUNCTIONS[name] == (ci, [vp, vp]) and hasattr(lib, name)
    assert ctypes.sizeof(native.HeatDrawPlan) == 872 < 4096
    if not shutil.which('gcc'):
        pytest.skip('no gcc')
    layout(tmp_path, native.HeatDrawPlan, 'pave_heat_draw_plan')


def test_c_entries_refuse_bad_plans_before_any_device_call():
    native, lib = _lib()
    host = (ctypes.c_ubyte * 64)()
    addr = ctypes.addressof(host)

    def plan(n=2, width=64, height=48, pitch=256, camera=1, table=0, dst=addr, map=addr, peak=addr, palette=addr,
             cameras=2, tables=5, map_width=64, map_height=48, cell=8, source=0, full_scale=0, alpha_max=160, floor=1,
             smooth=1):
        p = native.HeatDrawPlan()
        for i in range(min(max(n, 0), 32)):
            p.dst[i], p.pitch[i], p.width[i], p.height[i], p.camera[i], p.table[i] = dst, pitch, width, height, camera, table
        p.map, p.peak, p.palette = map, peak, palette
        p.n, p.cameras, p.tables, p.map_width, p.map_height, p.cell = n, cameras, tables, map_width, map_height, cell
        p.source, p.full_scale, p.alpha_max, p.floor, p.smooth = source, full_scale, alpha_max, floor, smooth
        return p

    for entry, bpp in ((lib.pave_draw_heat_nv12, 1), (lib.pave_draw_heat_bgr, 3)):
        def refused(p, needle):
            assert entry(ctypes.byref(p) if p is not None else None, None) == native.DEFINES['PAVE_E_ARG'] == -1
            assert needle in lib.pave_last_error().decode(), lib.pave_last_error()
        refused(None, 'null plan')
        refused(plan(n=0), 'surfaces per launch')
        refused(plan(n=33), 'surfaces per launch')
        refused(plan(dst=None), 'null surface')
        refused(plan(map=None), 'null map')
        refused(plan(peak=None), 'null map')
        refused(plan(palette=None), 'null palette')
        refused(plan(tables=0), 'tables outside')
        refused(plan(tables=9), 'tables outside')
        refused(plan(table=5), 'table index')
        refused(plan(cameras=0), 'cameras outside')
        refused(plan(cameras=4097), 'cameras outside')
        refused(plan(camera=2), 'camera index')
        refused(plan(camera=-1), 'camera index')
        for kw in (dict(map_width=0), dict(map_height=8193), dict(cell=0), dict(cell=6), dict(cell=128),
                   dict(map_width=2052, cell=4)):
            refused(plan(**kw), 'a map of')
        refused(plan(source=-1), 'source')
        refused(plan(source=2), 'source')
        refused(plan(full_scale=-1), 'full_scale')
        refused(plan(alpha_max=-1), 'alpha_max')
        refused(plan(alpha_max=257), 'alpha_max')
        refused(plan(floor=-1), 'floor')
        refused(plan(floor=256), 'floor')
        refused(plan(smooth=2), 'smooth')
        refused(plan(width=0), 'width and height')
        refused(plan(height=8194), 'width and height')
        refused(plan(width=64, pitch=64 * bpp - 1), 'pitch')
        if bpp == 1:
            refused(plan(width=63), 'even')
            refused(plan(height=47), 'even')


def test_calls_raise_value_errors_on_host_tensors():
    from pavenet_amd import FootfallMap, HeatStyle, draw_heat_bgr, draw_heat_nv12, ops
    fmap = FootfallMap(15, size=(64, 48), cameras=2)
    nv, bgr = torch.zeros(72, 64, dtype=torch.uint8), torch.zeros(48, 64, 3, dtype=torch.uint8)
    for call, needle in (
            (lambda: draw_heat_nv12([], 64, fmap), 'non-empty'),
            (lambda: draw_heat_nv12(nv.float(), 64, fmap), 'uint8'),
            (lambda: draw_heat_nv12(nv, 64, object()), 'FootfallMap'),
            (lambda: draw_heat_nv12(nv, 64, fmap, style=object()), 'HeatStyle'),
            (lambda: draw_heat_nv12(nv, 64, fmap, camera=2), 'camera'),
            (lambda: draw_heat_nv12([nv, nv], 64, fmap, camera=[0]), 'camera'),
            (lambda: draw_heat_nv12(nv, 63, fmap), 'even'),
            (lambda: draw_heat_nv12(nv, 66, fmap), 'pitch'),
            (lambda: draw_heat_nv12(nv, 64.0, fmap), 'width'),
            (lambda: draw_heat_nv12(nv[:71], 64, fmap), 'rows'),
            (lambda: draw_heat_nv12(bgr, 64, fmap), 'pitch'),
            (lambda: draw_heat_nv12(nv, 64, fmap, matrix='bt2020'), 'matrix'),
            (lambda: draw_heat_nv12(nv, 64, fmap), 'HIP device'),
            (lambda: draw_heat_bgr(nv, fmap), r'\[H, W, 3\]'),
            (lambda: draw_heat_bgr(bgr, fmap, camera=-1), 'camera'),
            (lambda: draw_heat_bgr(bgr, fmap), 'HIP device')):
        with pytest.raises(ValueError, match=needle):
            call()
    assert fmap._state is None and HeatStyle()._device == {}

    z = dict(dtype=torch.int32)
    state = dict(peak=torch.zeros(2, 2, **z), dwell=torch.zeros(2, 6, 8, **z), visits=torch.zeros(2, 6, 8, **z))
    pal = torch.zeros(5, 256, 3, dtype=torch.uint8)

    def draw(kind='nv12', items=((nv, 64, 0, 1),), st=state, palette=pal, size=(64, 48), **kw):
        return ops.draw_heat(kind, items, st, palette, size=size, **kw)
    for call, needle in (
            (lambda: draw(kind='rgb'), 'kind'),
            (lambda: draw(items=()), 'no surface'),
            (lambda: draw(items=[(nv, 64, 0)]), 'an item is'),
            (lambda: draw(source='both'), 'source'),
            (lambda: draw(alpha_max=257), 'alpha_max'),
            (lambda: draw(floor=-1), 'floor'),
            (lambda: draw(full_scale=0), 'full_scale'),
            (lambda: draw(full_scale=2 ** 31), 'full_scale'),
            (lambda: draw(cell=5), 'cell'),
            (lambda: draw(size=(64, 0)), 'size'),
            (lambda: draw(size=(72, 48)), 'state dwell'),
            (lambda: draw(st=dict(peak=pal)), 'state holds'),
            (lambda: draw(st=dict(state, visits=torch.zeros(2, 6, 8))), 'state visits'),
            (lambda: draw(palette=pal[:, :255]), 'palette'),
            (lambda: draw(palette=pal.int()), 'palette'),
            (lambda: draw(palette=torch.zeros(9, 256, 3, dtype=torch.uint8)), 'palette'),
            (lambda: draw(items=[(nv, 64, 2, 1)]), 'camera of surface 0'),
            (lambda: draw(items=[(nv, 64, 0, 5)]), 'palette table'),
            (lambda: draw(items=[(nv, 62, 0, 1), (nv, 63, 0, 1)]), 'surface 1'),
            (lambda: draw(kind='bgr', items=[(nv, None, 0, 0)]), r'\[H, W, 3\]'),
            (lambda: draw(kind='bgr', items=[(bgr.transpose(0, 1), None, 0, 0)]), 'contiguous'),
            (lambda: draw(), 'HIP device')):
        with pytest.raises(ValueError, match=needle):
            call()
