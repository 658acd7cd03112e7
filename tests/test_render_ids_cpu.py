"""Track ids in the picture, the parts that need no GPU: the ids plan's C layout, the two entry points at ABI 21,
every refusal of the C entries and of the Python wrappers, the palette's conditions, and the oracle
(tests/render_ids_ref.py) on itself."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import render_ids_ref as IR
from tests import render_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from pavenet_amd import native
    from pavenet_amd.build_native import build_native
    build_native()
    return native, native.load()


def test_ids_plan_layout_and_entries(tmp_path):
    """native.DrawIdsPlan is the header's pave_draw_ids_plan field for field (its base a pave_draw_plan), fits the
    4 KB kernel-argument limit, and the two entries are in the header, the binding and both libraries at ABI 21."""
    native, lib = _lib()
    vp, ci = ctypes.c_void_p, ctypes.c_int
    names = ('pave_draw_tracks_nv12', 'pave_draw_tracks_bgr')
    for name in names:
        assert native.FUNCTIONS[name] == (ci, [vp, vp]) and name in native.SIGNATURES and hasattr(lib, name)
    for path in (native.LIB_PATH, native.DIAG_LIB_PATH):
        out = subprocess.run(['nm', '-D', '--defined-only', path], capture_output=True, text=True, check=True).stdout
        assert set(names) <= {ln.split()[-1] for ln in out.splitlines()}
    assert native.ABI_VERSION == 21 and lib.pave_abi_version() == 21
    assert native.DRAW_PALETTE == 32
    assert ctypes.sizeof(native.DrawIdsPlan) <= 4096
    assert native.DrawIdsPlan.base.offset == 0 and native.DrawIdsPlan.base.size == ctypes.sizeof(native.DrawPlan)
    if not shutil.which('gcc'):
        pytest.skip('no gcc')
    fields = [f for f, _ in native.DrawIdsPlan._fields_]
    src = tmp_path / 'layout.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pave_hip.h"\nint main(void) {\n'
                   '  printf("%zu %zu", sizeof(pave_draw_ids_plan), sizeof(pave_draw_plan));\n'
                   + ''.join(f'  printf(" %zu", offsetof(pave_draw_ids_plan, {f}));\n' for f in fields)
                   + '  return 0;\n}\n')
    exe = tmp_path / 'layout'
    subprocess.run(['gcc', '-std=c99', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == ctypes.sizeof(native.DrawIdsPlan) <= 4096 and got[1] == ctypes.sizeof(native.DrawPlan)
    assert got[2:] == [getattr(native.DrawIdsPlan, f).offset for f in fields]


def test_c_entries_refuse_bad_ids_plans_before_any_device_call():
    """No GPU: PAVE_E_ARG with a message for a bad label_scale, untracked_skip or font row, and for what the base plan
    gets wrong; the addresses are never dereferenced."""
    from pavenet_amd.render import DIGIT_FONT
    native, lib = _lib()
    host = (ctypes.c_ubyte * 64)()
    addr = ctypes.addressof(host)

    def plan(label_scale=2, untracked_skip=0, font=DIGIT_FONT, n=2, N=3, K=17, W=70, dst=addr):
        p = native.DrawIdsPlan()
        for i in range(n):
            p.base.dst[i], p.base.kpts[i], p.base.bboxes[i], p.ids[i] = dst, addr, addr, addr
            p.base.pitch[i], p.base.width[i], p.base.height[i], p.base.n_poses[i] = 256, W, 50, N
            p.base.scale[i][0], p.base.scale[i][1] = 1.0, 1.0
        p.base.n, p.base.K, p.base.E, p.base.thickness, p.base.radius = n, K, 0, 4, 4
        for d in range(10):
            for r in range(7):
                p.font[d][r] = font[d][r]
        p.label_scale, p.untracked_skip = label_scale, untracked_skip
        return p

    def refused(p, needle):
        for fn in (lib.pave_draw_tracks_nv12, lib.pave_draw_tracks_bgr):
            assert fn(ctypes.byref(p) if p is not None else None, None) == native.DEFINES['PAVE_E_ARG'] == -1
            assert needle in lib.pave_last_error().decode(), lib.pave_last_error()

    refused(None, 'null plan')
    for g in (-1, 9, 1 << 20):
        refused(plan(label_scale=g), 'label_scale')
    for skip in (-1, 2):
        refused(plan(untracked_skip=skip), 'untracked_skip')
    for d, r, bits in ((0, 0, 0x20), (9, 6, 0x80), (4, 3, 0xff)):
        font = [list(rows) for rows in DIGIT_FONT]
        font[d][r] = bits
        refused(plan(font=font), 'font row')
    # the base plan's refusals are draw_poses' own
    refused(plan(n=0), 'surfaces')
    refused(plan(K=33), 'K outside')
    refused(plan(N=4097), 'N outside')
    refused(plan(dst=None), 'null surface')
    refused(plan(W=8194), '8192')
    # nothing to draw: accepted, and nothing is launched
    assert lib.pave_draw_tracks_nv12(ctypes.byref(plan(N=0)), None) == 0
    assert lib.pave_draw_tracks_bgr(ctypes.byref(plan(N=0, label_scale=8, untracked_skip=1)), None) == 0


def test_wrappers_raise_value_errors_on_host_tensors():
    """Every ValueError of ops.draw_tracks, TrackStyle, ids= and style= on host tensors: before any device check."""
    import pavenet_amd
    from pavenet_amd import ops
    from pavenet_amd.render import DIGIT_FONT, PoseStyle, TrackStyle, draw_poses_bgr, draw_poses_nv12
    assert pavenet_amd.TrackStyle is TrackStyle and issubclass(TrackStyle, PoseStyle)
    surf, img = torch.zeros(75, 96, dtype=torch.uint8), torch.zeros(50, 70, 3, dtype=torch.uint8)
    kp, bb = torch.zeros(3, 17, 3), torch.zeros(3, 5)
    res, ids = (bb, None, kp), torch.ones(3, dtype=torch.int32)
    colors, pal, font = [[[0, 0, 0]] * 65], [[[0, 0, 0]] * 33], [list(r) for r in DIGIT_FONT]

    def item(ids=ids, surface=img, table=0):
        return (surface, None, kp, bb, None, (1, 1), table, ids)

    def tracks(items=None, colors=colors, palettes=pal, font=font, edges=(), K=17, kind='bgr', **kw):
        return ops.draw_tracks(kind, [item()] if items is None else items, colors, palettes, font, edges, K, **kw)
    bad_font = [list(r) for r in DIGIT_FONT]
    bad_font[3][2] = 32
    for call, needle in (
            (lambda: tracks(kind='rgb'), 'kind'),
            (lambda: tracks(items=[]), 'no surface'),
            (lambda: tracks(items=[item()[:7]]), 'an item is'),
            (lambda: tracks(label_scale=9), 'label_scale'),
            (lambda: tracks(label_scale=-1), 'label_scale'),
            (lambda: tracks(label_scale=1.5), 'label_scale'),
            (lambda: tracks(label_scale=True), 'label_scale'),
            (lambda: tracks(untracked='hide'), 'untracked'),
            (lambda: tracks(font=font[:9]), 'font'),
            (lambda: tracks(font=[r[:6] for r in font]), 'font'),
            (lambda: tracks(font=bad_font), 'font'),
            (lambda: tracks(font=5), 'font'),
            (lambda: tracks(palettes=[[[0, 0, 0]] * 32]), 'palettes'),
            (lambda: tracks(palettes=[]), 'palettes'),
            (lambda: tracks(palettes=pal * 2), 'one palette per colour table'),
            (lambda: tracks(colors=[[[0, 0, 0]] * 64]), 'tables'),
            (lambda: tracks(items=[item(table=1)]), 'colour table'),
            (lambda: tracks(edges=[(0, 17)]), 'edge'),
            (lambda: tracks(thickness=40), 'thickness'),
            (lambda: tracks(items=[item(surface=img.float())]), 'uint8'),
            (lambda: tracks(items=[item(ids=ids.long())]), 'ids of surface 0'),
            (lambda: tracks(items=[item(ids=ids[:2])]), 'ids of surface 0'),
            (lambda: tracks(items=[item(ids=[1, 2, 3])]), 'ids of surface 0'),
            (lambda: tracks(items=[item(), item(ids=torch.ones(6, dtype=torch.int32)[::2])]), 'surface 1 must be contiguous'),
            (lambda: tracks(items=[item(ids=ids.to('meta'))]), 'are on meta'),
            (lambda: TrackStyle(17, palette=[(0, 0, 0)] * 31), 'palette'),
            (lambda: TrackStyle(17, palette=5), 'palette'),
            (lambda: TrackStyle(17, palette=[(0, 0, 256)] * 32), '8-bit'),
            (lambda: TrackStyle(17, label_color='white'), '8-bit'),
            (lambda: TrackStyle(17, label_scale=9), 'label_scale'),
            (lambda: TrackStyle(17, label_scale=-1), 'label_scale'),
            (lambda: TrackStyle(17, label_scale=2.0), 'label_scale'),
            (lambda: TrackStyle(17, untracked='drop'), 'untracked'),
            (lambda: TrackStyle(16), 'built-in'),
            (lambda: TrackStyle(17, thickness=0), 'thickness'),
            (lambda: draw_poses_nv12(surf, 70, res, ids=ids, style=PoseStyle(17)), 'TrackStyle'),
            (lambda: draw_poses_bgr(img, res, ids=ids, style=PoseStyle(17)), 'TrackStyle'),
            (lambda: draw_poses_bgr(img, res, ids=ids, style='bright'), 'TrackStyle'),
            (lambda: draw_poses_bgr(img, res, ids=ids, style=TrackStyle(15)), 'K = 17'),
            (lambda: draw_poses_bgr(img, res, ids=[ids, ids]), 'ids is one tensor'),
            (lambda: draw_poses_bgr([img, img], [res, res], ids=ids), 'ids is one tensor'),
            (lambda: draw_poses_bgr([img, img], [res, res], ids=[ids]), 'ids is one tensor'),
            (lambda: draw_poses_bgr(img, res, ids=7), 'ids is one tensor'),
            (lambda: draw_poses_bgr([img], [res], ids=[[1, 2, 3]]), 'int32 tensor or None'),
            (lambda: draw_poses_bgr(img, res, ids=ids.long()), 'ids of surface 0'),
            (lambda: draw_poses_nv12(surf, 70, res, ids=ids[:2]), 'ids of surface 0'),
            (lambda: draw_poses_nv12(surf, 71, res, ids=ids), 'even')):
        with pytest.raises(ValueError, match=needle):
            call()
    # what is left is a valid call on host tensors: the device check speaks, and nothing was drawn
    for call in (tracks, lambda: draw_poses_nv12(surf, 70, res, ids=ids), lambda: draw_poses_bgr(img, res, ids=ids),
                 lambda: draw_poses_bgr([img, img], [res, res], ids=[None, ids], style=TrackStyle(17, untracked='skip')),
                 lambda: draw_poses_nv12([surf], 70, [res], ids=[None])):
        with pytest.raises(RuntimeError, match='HIP device tensor'):
            call()
    assert not surf.any() and not img.any()
    # a TrackStyle is a PoseStyle: the plain call takes it, and its tables are kept per (matrix, range)
    style = TrackStyle(17)
    assert (style.label_scale, style.label_color, style.untracked) == (2, (255, 255, 255), 'style')
    assert style.palette_bytes('bt709', True) is style.palette_bytes('bt709', True) and len(style.palette_bytes()) == 99
    assert style.palette_bytes() != style.palette_bytes('bt601') != style.palette_bytes('bt601', True)
    assert style.palette_bytes()[:3] == bytes(style.palette[0]) and style.palette_bytes()[96:] == bytes((255, 255, 255))
    assert len(style.table_bytes('bt601')) == 195


def test_palette_and_font_conditions():
    """32 distinct colours, each at least 64 of 255 in BT.601 luma from the default ink; ten distinct, non-empty
    5 x 7 faces."""
    from pavenet_amd.render import DIGIT_FONT, TRACK_PALETTE, TrackStyle
    assert len(TRACK_PALETTE) == 32 == len(set(TRACK_PALETTE))
    ink = TrackStyle(15).label_color

    def luma(bgr):
        return 0.299 * bgr[2] + 0.587 * bgr[1] + 0.114 * bgr[0]
    gaps = [abs(luma(ink) - luma(c)) for c in TRACK_PALETTE]
    print(f'luma distance to the ink: {min(gaps):.1f} .. {max(gaps):.1f}')
    assert all(len(c) == 3 and all(isinstance(v, int) and 0 <= v <= 255 for v in c) for c in TRACK_PALETTE)
    assert min(gaps) >= 64
    assert len(DIGIT_FONT) == 10 == len(set(DIGIT_FONT))
    assert all(len(rows) == 7 and all(0 <= r < 32 for r in rows) and any(rows) for rows in DIGIT_FONT)


def _scene(seed=3, n=4, W=96, H=64):
    rng = np.random.default_rng(seed)
    kpts = np.empty((n, 15, 3), np.float32)
    kpts[..., 0] = rng.uniform(8, W - 8, (n, 15))
    kpts[..., 1] = rng.uniform(24, H - 4, (n, 15))
    kpts[..., 2] = 0.9
    bboxes = np.concatenate([kpts[..., :2].min(1), kpts[..., :2].max(1), np.full((n, 1), 0.9)], 1).astype(np.float32)
    return kpts, bboxes


def test_oracle_on_itself():
    from pavenet_amd.render import DIGIT_FONT, TRACK_PALETTE, TrackStyle
    W, H = 96, 64
    kpts, bboxes = _scene()
    rng = np.random.default_rng(0)
    surface = rng.integers(0, 256, (H * 3 // 2, 128), dtype=np.uint8)
    image = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    style = TrackStyle(15, draw_boxes=True)
    # all ids 0 under 'style' (and a surface without ids) is section 13, bit for bit
    for ids in (np.zeros(4, np.int32), np.array([0, -5, 0, -2 ** 31], np.int32), None):
        got = IR.draw_nv12(surface, W, kpts, bboxes, None, ids, (1.0, 1.0), style, TRACK_PALETTE, DIGIT_FONT)
        assert np.array_equal(got, RR.draw_nv12(surface, W, kpts, bboxes, None, (1.0, 1.0), style))
        got = IR.draw_bgr(image, kpts, bboxes, None, ids, (1.0, 1.0), style, TRACK_PALETTE, DIGIT_FONT)
        assert np.array_equal(got, RR.draw_bgr(image, kpts, bboxes, None, (1.0, 1.0), style))
    # ... and under 'skip' nothing at all, except on a surface without ids
    skip = TrackStyle(15, draw_boxes=True, untracked='skip')
    assert np.array_equal(IR.draw_bgr(image, kpts, bboxes, None, np.zeros(4, np.int32), (1.0, 1.0), skip, TRACK_PALETTE,
                                      DIGIT_FONT), image)
    assert np.array_equal(IR.draw_bgr(image, kpts, bboxes, None, None, (1.0, 1.0), skip, TRACK_PALETTE, DIGIT_FONT),
                          RR.draw_bgr(image, kpts, bboxes, None, (1.0, 1.0), skip))
    # one pose, id 7, g = 1, no capsule anywhere near: exactly popcount(font[7]) ink pixels on a 7 x 9 plate
    one_k, one_b = kpts[:1].copy(), np.array([[40.0, 30.0, 60.0, 50.0, 0.9]], np.float32)
    one_k[..., 2] = 0.0                                  # no key point is visible: the label is all there is
    quiet = TrackStyle(15, label_scale=1, kpt_thr=0.5)
    id_of, colours = IR.id_map_and_colours(W, H, one_k, one_b, None, np.array([7], np.int32), (1.0, 1.0), quiet,
                                           TRACK_PALETTE, DIGIT_FONT)
    plate = 1 * (4 + 15 + 15)
    popcount = sum(bin(r).count('1') for r in DIGIT_FONT[7])
    assert int((id_of == plate + 1).sum()) == popcount == 11
    assert int((id_of >= plate).sum()) == 7 * 9 and int((id_of >= 0).sum()) == 7 * 9
    ys, xs = np.nonzero(id_of >= 0)
    assert (xs.min(), xs.max(), ys.min(), ys.max()) == (40, 46, 21, 29)
    assert colours[plate] == TRACK_PALETTE[6] and colours[plate + 1] == (255, 255, 255)
    # a plate is g (6 n + 1) x 9 g, for every digit count and scale that fits the picture
    for v, g in ((3, 1), (42, 2), (99999, 1), (2147483647, 1), (5, 8), (10, 3)):
        n = len(str(v))
        big = np.array([[2.0, 80.0, 90.0, 99.0, 0.9]], np.float32)
        id_of, _ = IR.id_map_and_colours(512, 128, one_k, big, None, np.array([v], np.int32), (1.0, 1.0),
                                         TrackStyle(15, label_scale=g, kpt_thr=0.5), TRACK_PALETTE, DIGIT_FONT)
        ys, xs = np.nonzero(id_of >= 0)
        assert (xs.max() - xs.min() + 1, ys.max() - ys.min() + 1) == (g * (6 * n + 1), 9 * g), (v, g)
        assert (xs.min(), ys.max()) == (2, 79) and len(xs) == g * (6 * n + 1) * 9 * g
        ink = sum(bin(r).count('1') for c in str(v) for r in DIGIT_FONT[int(c)]) * g * g
        assert int((id_of == plate + 1).sum()) == ink, (v, g)
    assert IR.label_geometry((2.0, 80.0, 90.0, 99.0), (1.0, 1.0), 2147483647, 8)[2:4] == (488, 72)
    # the box is used even when it is not drawn, ay clamps at 0, and the label is clipped at the borders
    ax, ay, Wp, Hp, digits = IR.label_geometry((90.0, 3.0, 60.0, 50.0), (1.0, 1.0), 120, 2)
    assert (ax, ay, Wp, Hp, digits) == (60, 0, 38, 18, [1, 2, 0])
    id_of, _ = IR.id_map_and_colours(W, H, one_k, np.array([[90.0, 3.0, 60.0, 50.0, 0.9]], np.float32), None,
                                     np.array([120], np.int32), (1.0, 1.0), TrackStyle(15, kpt_thr=0.5), TRACK_PALETTE,
                                     DIGIT_FONT)
    ys, xs = np.nonzero(id_of >= 0)
    assert (xs.min(), xs.max(), ys.min(), ys.max()) == (60, 95, 0, 17)
    # colours by id: 33 is the colour of 1; the discs keep the style's colours
    vis = _scene(seed=4, n=2)
    for a, b in ((1, 33), (32, 64)):
        ma, ca = IR.id_map_and_colours(W, H, *vis, None, np.array([a, 0], np.int32), (1.0, 1.0),
                                       TrackStyle(15, label_scale=0), TRACK_PALETTE, DIGIT_FONT)
        mb, cb = IR.id_map_and_colours(W, H, *vis, None, np.array([b, 0], np.int32), (1.0, 1.0),
                                       TrackStyle(15, label_scale=0), TRACK_PALETTE, DIGIT_FONT)
        assert np.array_equal(ma, mb) and ca == cb and ma.max() < 2 * 34
        assert ca[4] == TRACK_PALETTE[(a - 1) % 32] and ca[4 + 15] == style.kpt_colors[0]
        assert ca[34 + 4] == style.edge_colors[0]
