"""Drawing poses into frames, the parts that need no GPU: the integer rule of DESIGN section 13 (tests/render_ref.py)
against a float64 point-to-segment distance, its int64 head-room, the colour transform against the ingest conversion,
the plan's C layout, and every refusal of the C entry points and of the Python wrappers."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import render_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAND = 0.18   # quarter-pixel rounding moves an end by at most sqrt(2) / 8 = 0.177 px


def _random_poses(rng, n, K, W, H, scale):
    """n poses inside a W x H picture (a pixel away from its border: no clamp), in the coordinates of the scaled
    picture the network saw."""
    kpts = np.empty((n, K, 3), np.float32)
    kpts[..., 0] = rng.uniform(1, W - 2, (n, K)) * scale[0]
    kpts[..., 1] = rng.uniform(1, H - 2, (n, K)) * scale[1]
    kpts[..., 2] = 1.0
    bboxes = np.concatenate([kpts[..., 0].min(1, keepdims=True), kpts[..., 1].min(1, keepdims=True),
                             kpts[..., 0].max(1, keepdims=True), kpts[..., 1].max(1, keepdims=True),
                             np.full((n, 1), 0.9, np.float32)], 1).astype(np.float32)
    return kpts, bboxes


@pytest.mark.parametrize('W,H,scale', [(64, 48, (1.0, 1.0)), (70, 50, (0.694, 0.694)), (1920, 1080, (1.0, 1.0))])
def test_integer_rule_against_float64_distance(W, H, scale):
    """Per primitive, the integer coverage equals `distance <= radius` in float64 for every pixel whose distance is
    not within 0.18 px of the radius (the ends move by at most 0.177 px when they are rounded to quarter pixels),
    and that band is at most 20 % of the pixels within radius + 0.18 (16.6 - 18.0 % for these poses)."""
    from pavenet_amd.render import PoseStyle
    style = PoseStyle(17, thickness=4, radius=4)
    kpts, bboxes = _random_poses(np.random.default_rng(5), 3, 17, W, H, scale)
    prims = RR.primitives(kpts, bboxes, None, scale, style)
    assert len(prims) == 3 * (len(style.edges) + 17)
    ends = kpts[..., :2].astype(np.float64) / np.asarray(scale, np.float32).astype(np.float64)
    per_pose = 4 + len(style.edges) + 17
    left_out = near = 0
    for pid, A, B, r, (kind, i) in prims:
        p = pid // per_pose
        a, b = style.edges[i] if kind == 'limb' else (i, i)
        radius = style.thickness / 2 if kind == 'limb' else float(style.radius)
        assert r == 4 * radius
        lo_x, hi_x, lo_y, hi_y = RR.window(A, B, r, W, H, margin=2)
        xs, ys = np.meshgrid(np.arange(lo_x, hi_x + 1), np.arange(lo_y, hi_y + 1))
        got = RR.covered(A, B, r, 4 * xs.astype(np.int64), 4 * ys.astype(np.int64))
        pa, pb = ends[p, a], ends[p, b]
        d = pb - pa
        w = np.stack([xs - pa[0], ys - pa[1]], -1)
        L2 = float(d @ d)
        t = np.clip((w @ d) / L2, 0.0, 1.0) if L2 > 0 else np.zeros(xs.shape)
        dist = np.sqrt(((w - t[..., None] * d) ** 2).sum(-1))
        band = np.abs(dist - radius) <= BAND
        assert np.array_equal(got[~band], (dist <= radius)[~band]), (pid, kind, i)
        # outside the window nothing is covered by either statement
        edge = np.ones(xs.shape, bool)
        edge[1:-1, 1:-1] = False
        inner = (xs > 0) & (xs < W - 1) & (ys > 0) & (ys < H - 1)
        assert not got[edge & inner].any() and not (dist <= radius + BAND)[edge & inner].any()
        left_out += int(band.sum())
        near += int((dist <= radius + BAND).sum())
    share = left_out / near
    print(f'{W} x {H}: {left_out} of {near} pixels within radius + {BAND} are in the band ({100 * share:.1f} %)')
    assert share <= 0.20


def test_coverage_has_int64_headroom():
    """0 and 32767 corners, radius 128: the int64 rule equals the same rule in Python integers."""
    pts = [0, 4, 128, 16380, 32636, 32764]
    PX, PY = np.meshgrid(np.asarray(pts, np.int64), np.asarray(pts, np.int64))
    corners = [(0, 0), (32767, 0), (0, 32767), (32767, 32767), (16383, 16384)]
    for A in corners:
        for B in corners:
            got = RR.covered(A, B, 128, PX, PY)
            for iy, y in enumerate(pts):
                for ix, x in enumerate(pts):
                    dx, dy, wx, wy = B[0] - A[0], B[1] - A[1], x - A[0], y - A[1]
                    L2, t, r2 = dx * dx + dy * dy, wx * dx + wy * dy, 128 * 128
                    if t <= 0:
                        want = wx * wx + wy * wy <= r2
                    elif t >= L2:
                        want = (x - B[0]) ** 2 + (y - B[1]) ** 2 <= r2
                    else:
                        cross = wx * dy - wy * dx
                        assert abs(cross) <= 2 ** 31 and cross * cross < 2 ** 63 and r2 * L2 < 2 ** 63
                        want = cross * cross <= r2 * L2
                    assert bool(got[iy, ix]) == want, (A, B, x, y)


@pytest.mark.parametrize('matrix', ['bt601', 'bt709'])
@pytest.mark.parametrize('full_range', [False, True])
def test_bgr_to_yuv_round_trip_through_the_ingest_conversion(matrix, full_range):
    """bgr_to_yuv, then the conversion the ingest kernels make (DESIGN section 12, nv12_csc's coefficients, fp32):
    each colour comes back to within 2 per channel in limited range and 1 in full range."""
    from pavenet_amd.preprocess import nv12_csc
    from pavenet_amd.render import bgr_to_yuv
    rng = np.random.default_rng(11)
    cube = [[b, g, r] for b in (0, 255) for g in (0, 255) for r in (0, 255)]
    bgr = np.concatenate([rng.integers(0, 256, (20000, 3)), np.asarray(cube)], 0).astype(np.uint8)
    yuv = bgr_to_yuv(bgr, matrix, full_range)
    assert yuv.dtype == np.uint8 and yuv.shape == bgr.shape
    assert all(tuple(yuv[i]) == RR.bgr_to_yuv(bgr[i], matrix, full_range) for i in range(0, len(bgr), 97))
    yoff, cy, crv, cgu, cgv, cbu = (np.float32(c) for c in nv12_csc(matrix, full_range))
    Y, u, v = yuv[:, 0].astype(np.float32), yuv[:, 1].astype(np.float32) - 128, yuv[:, 2].astype(np.float32) - 128
    t = (Y - yoff) * cy
    back = np.stack([t + u * cbu, (t + u * cgu) + v * cgv, t + v * crv], -1)
    back = np.clip(np.rint(back), 0, 255).astype(np.int64)
    err = np.abs(back - bgr.astype(np.int64)).max()
    print(f'{matrix} full_range={full_range}: max |round trip - colour| = {err}')
    assert err <= (1 if full_range else 2)
    with pytest.raises(ValueError, match='matrix'):
        bgr_to_yuv(bgr, 'bt2020')


def _lib():
    from pavenet_amd import native
    from pavenet_amd.build_native import build_native
    build_native()
    return native, native.load()


def test_draw_plan_layout_and_entries(tmp_path):
    """native.DrawPlan is the header's pave_draw_plan field for field, fits the 4 KB kernel-argument limit, and the
    two entries are in the header, the binding and both libraries at ABI 21."""
    native, lib = _lib()
    vp, ci = ctypes.c_void_p, ctypes.c_int
    for name in ('pave_draw_poses_nv12', 'pave_draw_poses_bgr'):
        assert native.FUNCTIONS[name] == (ci, [vp, vp]) and name in native.SIGNATURES and hasattr(lib, name)
    for path in (native.LIB_PATH, native.DIAG_LIB_PATH):
        out = subprocess.run(['nm', '-D', '--defined-only', path], capture_output=True, text=True, check=True).stdout
        assert {'pave_draw_poses_nv12', 'pave_draw_poses_bgr'} <= {ln.split()[-1] for ln in out.splitlines()}
    assert native.ABI_VERSION == 21 and lib.pave_abi_version() == 21
    assert (native.DRAW_MAX_SURFACES, native.DRAW_MAX_K, native.DRAW_MAX_E, native.DRAW_MAX_TABLES, native.DRAW_COLORS,
            native.DRAW_MAX_POSES, native.DRAW_MAX_SIZE) == (32, 32, 32, 4, 65, 4096, 8192)
    assert ctypes.sizeof(native.DrawPlan) <= 4096
    if not shutil.which('gcc'):
        pytest.skip('no gcc')
    fields = [f for f, _ in native.DrawPlan._fields_]
    src = tmp_path / 'layout.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pave_hip.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(pave_draw_plan));\n'
                   + ''.join(f'  printf(" %zu", offsetof(pave_draw_plan, {f}));\n' for f in fields)
                   + '  return 0;\n}\n')
    exe = tmp_path / 'layout'
    subprocess.run(['gcc', '-std=c99', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == ctypes.sizeof(native.DrawPlan)
    assert got[1:] == [getattr(native.DrawPlan, f).offset for f in fields]


def test_c_entries_refuse_bad_plans_before_any_device_call():
    """No GPU: every refusal is PAVE_E_ARG with a message (the addresses are never dereferenced)."""
    native, lib = _lib()
    host = (ctypes.c_ubyte * 64)()
    addr = ctypes.addressof(host)

    def plan(n=2, W=70, H=50, pitch=256, N=3, K=17, E=2, edges=((0, 1), (1, 16)), thickness=4, radius=4,
             scale=(1.0, 1.0), table=0, dst=addr, kpts=addr, bboxes=addr):
        p = native.DrawPlan()
        for i in range(min(max(n, 0), 32)):
            p.dst[i], p.kpts[i], p.bboxes[i] = dst, kpts, bboxes
            p.pitch[i], p.width[i], p.height[i], p.n_poses[i] = pitch, W, H, N
            p.scale[i][0], p.scale[i][1], p.table[i] = scale[0], scale[1], table
        for e, (a, b) in enumerate(edges):
            p.edge[e][0], p.edge[e][1] = a, b
        p.n, p.K, p.E, p.thickness, p.radius = n, K, E, thickness, radius
        return p

    def refused(p, needle, entries=(lib.pave_draw_poses_nv12, lib.pave_draw_poses_bgr)):
        for fn in entries:
            assert fn(ctypes.byref(p) if p is not None else None, None) == native.DEFINES['PAVE_E_ARG'] == -1
            assert needle in lib.pave_last_error().decode(), lib.pave_last_error()

    nv12, bgr = (lib.pave_draw_poses_nv12,), (lib.pave_draw_poses_bgr,)
    refused(None, 'null plan')
    refused(plan(n=0), 'surfaces')
    refused(plan(n=33), 'surfaces')
    refused(plan(dst=None), 'null surface')
    refused(plan(kpts=None), 'null pose')
    refused(plan(bboxes=None), 'null pose')
    for bad in (dict(W=0), dict(H=0), dict(W=8194, pitch=8194 * 3), dict(H=8194)):
        refused(plan(**bad), '8192')
    refused(plan(W=69), 'even', nv12)
    refused(plan(H=49), 'even', nv12)
    refused(plan(pitch=68), 'pitch', nv12)
    refused(plan(pitch=209), 'pitch', bgr)
    refused(plan(N=-1), 'N outside')
    refused(plan(N=4097), 'N outside')
    refused(plan(K=0), 'K outside')
    refused(plan(K=33), 'K outside')
    refused(plan(E=-1), 'E outside')
    refused(plan(E=33), 'E outside')
    refused(plan(edges=((0, 1), (1, 17))), 'edge index')
    refused(plan(thickness=0), 'thickness')
    refused(plan(thickness=33), 'thickness')
    refused(plan(radius=-1), 'radius')
    refused(plan(radius=33), 'radius')
    for bad in ((0.0, 1.0), (1.0, -1.0), (float('nan'), 1.0), (1.0, float('inf'))):
        refused(plan(scale=bad), 'scale')
    refused(plan(table=4), 'table')
    # a plan with nothing to draw is accepted, and launches nothing
    assert lib.pave_draw_poses_nv12(ctypes.byref(plan(N=0, kpts=None, bboxes=None)), None) == 0
    assert lib.pave_draw_poses_bgr(ctypes.byref(plan(N=0, kpts=None, bboxes=None, pitch=210)), None) == 0


def test_wrappers_raise_value_errors_on_host_tensors():
    """Shape, type and range checks come before the device checks: every one of them on host tensors."""
    import pavenet_amd
    from pavenet_amd import ops
    from pavenet_amd.render import PoseStyle, draw_poses_bgr, draw_poses_nv12
    assert pavenet_amd.PoseStyle is PoseStyle and pavenet_amd.draw_poses_nv12 is draw_poses_nv12
    surf, img = torch.zeros(75, 96, dtype=torch.uint8), torch.zeros(50, 70, 3, dtype=torch.uint8)
    kp, bb, keep = torch.zeros(3, 17, 3), torch.zeros(3, 5), torch.ones(3, dtype=torch.int32)
    res = (bb, None, kp)

    def nv12(surfaces=surf, width=70, results=res, **kw):
        return draw_poses_nv12(surfaces, width, results, **kw)
    for call, needle in (
            (lambda: nv12(surfaces=surf.float()), 'uint8'),
            (lambda: nv12(surfaces=surf[None]), 'pitch'),
            (lambda: nv12(surfaces=torch.zeros(76, 96, dtype=torch.uint8)), 'rows'),
            (lambda: nv12(width=71), 'even'),
            (lambda: nv12(width=0), 'even'),
            (lambda: nv12(width=98), 'pitch'),
            (lambda: nv12(surfaces=torch.zeros(12300, 16, dtype=torch.uint8), width=16), '8192'),
            (lambda: nv12(surfaces=[]), 'non-empty'),
            (lambda: nv12(surfaces=[surf, surf], results=[res]), 'one result per surface'),
            (lambda: nv12(surfaces=[surf, surf], results=[res, res], width=[70]), 'width'),
            (lambda: nv12(surfaces=[surf, surf], results=[res, res], matrix=['bt601']), 'matrix'),
            (lambda: nv12(surfaces=[surf, surf], results=[res, res], full_range=[True]), 'full_range'),
            (lambda: nv12(surfaces=[surf, surf, surf], results=[res] * 3, scale_factor=[1.0, (1.0, 2.0)]), 'scale_factor'),
            (lambda: nv12(matrix='bt2020'), 'matrix'),
            (lambda: nv12(scale_factor=0.0), 'positive'),
            (lambda: nv12(scale_factor=(1.0, float('nan'))), 'positive'),
            (lambda: nv12(scale_factor=(1.0, 2.0, 3.0)), 'scale_factor'),
            (lambda: nv12(results=(bb, kp)), 'tuple'),
            (lambda: nv12(results=dict(bboxes=bb)), 'bboxes and kpts'),
            (lambda: nv12(results=(bb.numpy(), None, kp)), 'tensor'),
            (lambda: nv12(results=(bb[:2], None, kp)), 'bboxes'),
            (lambda: nv12(results=(bb, None, kp[..., :2])), 'kpts'),
            (lambda: nv12(results=(bb.double(), None, kp)), 'float32'),
            (lambda: nv12(results=dict(bboxes=bb, kpts=kp, keep=keep.long())), 'int32'),
            (lambda: nv12(results=dict(bboxes=bb, kpts=kp, keep=keep[:2])), 'int32'),
            (lambda: nv12(results=(torch.zeros(4097, 5), None, torch.zeros(4097, 17, 3))), '4096'),
            (lambda: nv12(style='thick'), 'PoseStyle'),
            (lambda: nv12(style=PoseStyle(15)), 'K = 17'),
            (lambda: nv12(results=(bb, None, torch.zeros(3, 16, 3))), 'built-in'),
            (lambda: draw_poses_bgr(img[..., :2], res), 'H, W, 3'),
            (lambda: draw_poses_bgr(img.float(), res), 'uint8'),
            (lambda: draw_poses_bgr([img, img], res), 'one result per surface'),
            (lambda: PoseStyle(16), 'built-in'),
            (lambda: PoseStyle(33, skeleton=([], [], [(0, 0, 0)] * 33)), 'K in'),
            (lambda: PoseStyle(3, skeleton=([(0, 3)], [(1, 2, 3)], [(0, 0, 0)] * 3)), 'edge index'),
            (lambda: PoseStyle(3, skeleton=([(0, 1)] * 33, [(1, 2, 3)] * 33, [(0, 0, 0)] * 3)), 'edges'),
            (lambda: PoseStyle(3, skeleton=([(0, 1)], [], [(0, 0, 0)] * 3)), 'one colour'),
            (lambda: PoseStyle(3, skeleton=([(0, 1)], [(1, 2, 3)], [(0, 0, 0)] * 2)), 'one colour'),
            (lambda: PoseStyle(3, skeleton=([(0, 1)], [(1, 2, 256)], [(0, 0, 0)] * 3)), '8-bit'),
            (lambda: PoseStyle(3, skeleton=([(0, 1)], [(1, 2)], [(0, 0, 0)] * 3)), '8-bit'),
            (lambda: PoseStyle(3, skeleton=(5, 6)), 'skeleton'),
            (lambda: PoseStyle(17, bbox_color='green'), '8-bit'),
            (lambda: PoseStyle(17, thickness=0), 'thickness'),
            (lambda: PoseStyle(17, thickness=33), 'thickness'),
            (lambda: PoseStyle(17, thickness=2.5), 'thickness'),
            (lambda: PoseStyle(17, radius=-1), 'radius'),
            (lambda: PoseStyle(17, radius=33), 'radius'),
            (lambda: ops.draw_poses('rgb', [], [], [], 17), 'kind'),
            (lambda: ops.draw_poses('bgr', [], [[[0, 0, 0]] * 65], [], 17), 'no surface'),
            (lambda: ops.draw_poses('bgr', [(img, None, kp, bb, None, (1, 1), 0)], [[[0, 0, 0]] * 64], [], 17), 'tables'),
            (lambda: ops.draw_poses('bgr', [(img, None, kp, bb, None, (1, 1), 1)], [[[0, 0, 0]] * 65], [], 17), 'colour table'),
            (lambda: ops.draw_poses('bgr', [(img, None, kp, bb, None, (1, 1), 0)], [[[0, 0, 0]] * 65], [(0, 17)], 17), 'edge'),
            (lambda: ops.draw_poses('bgr', [(img, None, kp, bb, None, (1, 1), 0)], [[[0, 0, 0]] * 65], [], 17,
                                    thickness=40), 'thickness')):
        with pytest.raises(ValueError, match=needle):
            call()
    # what is left is a valid call on host tensors: the device check speaks, and nothing was drawn
    for call in (nv12, lambda: nv12(results=dict(bboxes=bb[None], kpts=kp[None], keep=keep[None])),
                 lambda: draw_poses_bgr(img, res), lambda: draw_poses_bgr([img], [res], scale_factor=[(0.5, 0.5, 0.5, 0.5)])):
        with pytest.raises(RuntimeError, match='HIP device tensor'):
            call()
    assert not surf.any() and not img.any()


def test_builtin_skeletons_and_show_result_refusals():
    from pavenet_amd.detectors import VideoPoseV1
    from pavenet_amd.petr import PETR
    from pavenet_amd.render import SKELETONS, PoseStyle, show_result
    for K, E in ((17, 18), (15, 15), (14, 14)):
        edges, edge_colors, kpt_colors = SKELETONS[K]
        assert len(edges) == len(edge_colors) == E and len(kpt_colors) == K
        assert len({frozenset(e) for e in edges}) == E and all(0 <= a < K and 0 <= b < K and a != b for a, b in edges)
        # one connected figure that reaches every key point
        seen, grew = {edges[0][0]}, True
        while grew:
            grew = False
            for a, b in edges:
                if (a in seen) != (b in seen):
                    seen |= {a, b}
                    grew = True
        assert seen == set(range(K))
        table = PoseStyle(K).color_table()
        assert len(table) == 65 and table[0] == [72, 101, 241] and table[1] == list(edge_colors[0])
        assert table[33 + K - 1] == list(kpt_colors[-1]) and table[1 + E] == [0, 0, 0]
    assert VideoPoseV1.show_result is PETR.show_result

    class Head:
        num_keypoints = 17

    class Model:
        bbox_head = Head()
    img = np.zeros((8, 8, 3), np.uint8)
    with pytest.raises(NotImplementedError, match='display'):
        show_result(Model(), img, ([], []), show=True)
    with pytest.raises(NotImplementedError, match='display'):
        show_result(Model(), img, ([], []), out_file='x.png')
