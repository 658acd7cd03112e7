"""Hiding people in frames, the parts that need no GPU: every refusal of the Python layer and of the two C entry
points, the plan's C layout, the properties of the rule of DESIGN section 15 as tests/anon_ref.py states it, and the
claim that keeps the defaults honest: the default head region covers a head whose nose is visible."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import anon_ref as AR
from tests import render_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CELLS = (2, 4, 8, 16, 32, 64)
# the K = 15 figure of tests/test_track_cpu.py in units of its height: nose, head bottom, head top, then left / right
# shoulder, elbow, wrist, hip, knee, ankle
FIGURE = np.asarray([(.20, .08), (.20, .14), (.20, .00), (.05, .20), (.35, .20), (.00, .36), (.40, .36), (.02, .50),
                     (.38, .50), (.10, .52), (.30, .52), (.09, .76), (.31, .76), (.08, 1.0), (.32, 1.0)], np.float64)


def _lib():
    from pavenet_amd import native
    from pavenet_amd.build_native import build_native
    build_native()
    return native, native.load()


def test_plan_layout_and_entries(tmp_path):
    """native.AnonPlan is the header's pave_anon_plan field for field, fits the 4 KB kernel-argument limit, and the two
    entries are in the header, the binding and both libraries at ABI 21."""
    native, lib = _lib()
    vp, ci = ctypes.c_void_p, ctypes.c_int
    names = {'pave_anonymize_nv12', 'pave_anonymize_bgr'}
    for name in names:
        assert native.FUNCTIONS[name] == (ci, [vp, vp]) and name in native.SIGNATURES and hasattr(lib, name)
    for path in (native.LIB_PATH, native.DIAG_LIB_PATH):
        out = subprocess.run(['nm', '-D', '--defined-only', path], capture_output=True, text=True, check=True).stdout
        assert names <= {ln.split()[-1] for ln in out.splitlines()}
    assert native.ABI_VERSION == 21 and lib.pave_abi_version() == 21
    assert (native.ANON_MAX_HEAD, native.ANON_MAX_CELL, native.ANON_MAX_MARGIN, native.ANON_MAX_SIXTEENTHS) == (8, 64, 64, 32)
    assert ctypes.sizeof(native.AnonPlan) <= 4096
    if not shutil.which('gcc'):
        pytest.skip('no gcc')
    fields = [f for f, _ in native.AnonPlan._fields_]
    src = tmp_path / 'layout.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pave_hip.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(pave_anon_plan));\n'
                   + ''.join(f'  printf(" %zu", offsetof(pave_anon_plan, {f}));\n' for f in fields)
                   + '  return 0;\n}\n')
    exe = tmp_path / 'layout'
    subprocess.run(['gcc', '-std=c99', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == ctypes.sizeof(native.AnonPlan)
    assert got[1:] == [getattr(native.AnonPlan, f).offset for f in fields]


def test_c_entries_refuse_bad_plans_before_any_device_call():
    """No GPU: every refusal is PAVE_E_ARG with a message (the addresses are never dereferenced)."""
    native, lib = _lib()
    host = (ctypes.c_ubyte * 64)()
    addr = ctypes.addressof(host)

    def plan(n=2, W=70, H=50, pitch=256, N=3, K=17, head=(0, 1, 2, 3, 4), n_head=None, region=0, mode=0, fallback_skip=0,
             cell=16, margin=0, grow=2, head_scale=12, head_min=2, scale=(1.0, 1.0), table=0, dst=addr, kpts=addr,
             bboxes=addr):
        p = native.AnonPlan()
        for i in range(min(max(n, 0), 32)):
            p.dst[i], p.kpts[i], p.bboxes[i] = dst, kpts, bboxes
            p.pitch[i], p.width[i], p.height[i], p.n_poses[i] = pitch, W, H, N
            p.scale[i][0], p.scale[i][1], p.table[i] = scale[0], scale[1], table
        for h, k in enumerate(head[:8]):
            p.head[h] = k
        p.n, p.K, p.n_head = n, K, len(head) if n_head is None else n_head
        p.region, p.mode, p.fallback_skip, p.cell, p.margin = region, mode, fallback_skip, cell, margin
        p.grow, p.head_scale, p.head_min = grow, head_scale, head_min
        return p

    def refused(p, needle, entries=(lib.pave_anonymize_nv12, lib.pave_anonymize_bgr)):
        for fn in entries:
            assert fn(ctypes.byref(p) if p is not None else None, None) == native.DEFINES['PAVE_E_ARG'] == -1
            assert needle in lib.pave_last_error().decode(), lib.pave_last_error()

    nv12, bgr = (lib.pave_anonymize_nv12,), (lib.pave_anonymize_bgr,)
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
    refused(plan(head=(0, 17)), 'head index')
    refused(plan(K=3, head=(0, 1, 2, 3)), 'head index')
    refused(plan(n_head=9), 'n_head')
    refused(plan(n_head=-1), 'n_head')
    refused(plan(head=()), 'needs head indices')
    for bad in (0, 1, 3, 6, 24, 128, -16):
        refused(plan(cell=bad), 'cell')
    refused(plan(margin=-1), 'margin')
    refused(plan(margin=65), 'margin')
    for name in ('grow', 'head_scale', 'head_min'):
        refused(plan(**{name: -1}), name)
        refused(plan(**{name: 33}), name)
    for name in ('region', 'mode', 'fallback_skip'):
        refused(plan(**{name: -1}), name)
        refused(plan(**{name: 2}), name)
    for bad in ((0.0, 1.0), (1.0, -1.0), (float('nan'), 1.0), (1.0, float('inf'))):
        refused(plan(scale=bad), 'scale')
    refused(plan(table=4), 'table')
    # a plan with nobody to hide is accepted, and launches nothing; so is a person plan without head indices
    assert lib.pave_anonymize_nv12(ctypes.byref(plan(N=0, kpts=None, bboxes=None)), None) == 0
    assert lib.pave_anonymize_bgr(ctypes.byref(plan(N=0, kpts=None, bboxes=None, pitch=210, head=(), region=1)), None) == 0


def test_python_layer_raises_value_errors_on_host_tensors():
    """Shape, type and range checks come before the device checks: every one of them on host tensors."""
    import pavenet_amd
    from pavenet_amd import ops
    from pavenet_amd.anonymize import HEAD_KEYPOINTS, PrivacyStyle, anonymize_bgr, anonymize_nv12
    assert pavenet_amd.PrivacyStyle is PrivacyStyle and pavenet_amd.anonymize_nv12 is anonymize_nv12
    assert pavenet_amd.anonymize_bgr is anonymize_bgr
    assert HEAD_KEYPOINTS == {17: (0, 1, 2, 3, 4), 15: (0, 1, 2), 14: (12, 13)}
    assert all(PrivacyStyle(K).head == HEAD_KEYPOINTS[K] for K in HEAD_KEYPOINTS)
    style = PrivacyStyle(17)
    assert (style.region, style.mode, style.cell, style.fill_color, style.margin, style.grow, style.head_scale,
            style.head_min, style.fallback, style.score_thr, style.kpt_thr) == \
        ('head', 'pixelate', 16, (0, 0, 0), 0, 2, 12, 2, 'person', 0.3, 0.0)
    assert PrivacyStyle(20, region='person').head == () and PrivacyStyle(20, head=[19, 3]).head == (19, 3)
    surf, img = torch.zeros(75, 96, dtype=torch.uint8), torch.zeros(50, 70, 3, dtype=torch.uint8)
    kp, bb, keep = torch.zeros(3, 17, 3), torch.zeros(3, 5), torch.ones(3, dtype=torch.int32)
    res = (bb, None, kp)
    item = (img, None, kp, bb, None, (1, 1), 0)

    def nv12(surfaces=surf, width=70, results=res, **kw):
        return anonymize_nv12(surfaces, width, results, **kw)
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
            (lambda: nv12(style='blur'), 'PrivacyStyle'),
            (lambda: nv12(style=PrivacyStyle(15)), 'K = 17'),
            (lambda: nv12(results=(bb, None, torch.zeros(3, 16, 3))), 'built-in'),
            (lambda: anonymize_bgr(img[..., :2], res), 'H, W, 3'),
            (lambda: anonymize_bgr(img.float(), res), 'uint8'),
            (lambda: anonymize_bgr([img, img], res), 'one result per surface'),
            (lambda: PrivacyStyle(16), 'built-in'),
            (lambda: PrivacyStyle(0, region='person'), 'K'),
            (lambda: PrivacyStyle(33, region='person'), 'K'),
            (lambda: PrivacyStyle(17, region='face'), 'region'),
            (lambda: PrivacyStyle(17, mode='blur'), 'mode'),
            (lambda: PrivacyStyle(17, fallback='box'), 'fallback'),
            (lambda: PrivacyStyle(17, cell=0), 'cell'),
            (lambda: PrivacyStyle(17, cell=3), 'cell'),
            (lambda: PrivacyStyle(17, cell=128), 'cell'),
            (lambda: PrivacyStyle(17, cell=16.5), 'cell'),
            (lambda: PrivacyStyle(17, fill_color='black'), '8-bit'),
            (lambda: PrivacyStyle(17, fill_color=(0, 0, 256)), '8-bit'),
            (lambda: PrivacyStyle(17, margin=-1), 'margin'),
            (lambda: PrivacyStyle(17, margin=65), 'margin'),
            (lambda: PrivacyStyle(17, margin=1.5), 'margin'),
            (lambda: PrivacyStyle(17, grow=-1), 'grow'),
            (lambda: PrivacyStyle(17, grow=33), 'grow'),
            (lambda: PrivacyStyle(17, head_scale=-1), 'head_scale'),
            (lambda: PrivacyStyle(17, head_scale=33), 'head_scale'),
            (lambda: PrivacyStyle(17, head_min=-1), 'head_min'),
            (lambda: PrivacyStyle(17, head_min=33), 'head_min'),
            (lambda: PrivacyStyle(17, head_min=True), 'head_min'),
            (lambda: PrivacyStyle(17, head=[17]), 'head'),
            (lambda: PrivacyStyle(17, head=[-1]), 'head'),
            (lambda: PrivacyStyle(17, head=list(range(9))), 'head'),
            (lambda: PrivacyStyle(17, head=5), 'head'),
            (lambda: PrivacyStyle(17, head=[]), 'head'),
            (lambda: ops.anonymize('rgb', [item], [(0, 0, 0)], [0], 17), 'kind'),
            (lambda: ops.anonymize('bgr', [], [(0, 0, 0)], [0], 17), 'no surface'),
            (lambda: ops.anonymize('bgr', [item], [(0, 0, 0)], [0], 33), 'K in'),
            (lambda: ops.anonymize('bgr', [item], [(0, 0)], [0], 17), 'fills'),
            (lambda: ops.anonymize('bgr', [item], [(0, 0, 0)] * 5, [0], 17), 'fills'),
            (lambda: ops.anonymize('bgr', [item[:6] + (1,)], [(0, 0, 0)], [0], 17), 'fill 1 of 1'),
            (lambda: ops.anonymize('bgr', [item], [(0, 0, 0)], [17], 17), 'head'),
            (lambda: ops.anonymize('bgr', [item], [(0, 0, 0)], [], 17), 'head indices'),
            (lambda: ops.anonymize('bgr', [item], [(0, 0, 0)], [0], 17, cell=12), 'cell'),
            (lambda: ops.anonymize('bgr', [item], [(0, 0, 0)], [0], 17, region='face'), 'region'),
            (lambda: ops.anonymize('bgr', [item], [(0, 0, 0)], [0], 17, mode='blur'), 'mode'),
            (lambda: ops.anonymize('bgr', [item], [(0, 0, 0)], [0], 17, fallback='box'), 'fallback'),
            (lambda: ops.anonymize('bgr', [item], [(0, 0, 0)], [0], 17, margin=65), 'margin'),
            (lambda: ops.anonymize('bgr', [item], [(0, 0, 0)], [0], 17, grow=33), 'grow'),
            (lambda: ops.anonymize('bgr', [item], [(0, 0, 0)], [0], 17, head_scale=33), 'head_scale'),
            (lambda: ops.anonymize('bgr', [item], [(0, 0, 0)], [0], 17, head_min=-1), 'head_min')):
        with pytest.raises(ValueError, match=needle):
            call()
    # what is left is a valid call on host tensors: the device check speaks, and nothing was written
    for call in (nv12, lambda: nv12(results=dict(bboxes=bb[None], kpts=kp[None], keep=keep[None])),
                 lambda: nv12(style=PrivacyStyle(17, region='person', mode='fill', cell=64)),
                 lambda: anonymize_bgr(img, res), lambda: anonymize_bgr([img], [res], scale_factor=[(0.5, 0.5, 0.5, 0.5)])):
        with pytest.raises(RuntimeError, match='HIP device tensor'):
            call()
    assert not surf.any() and not img.any()


def _style(K=17, **kw):
    from pavenet_amd.anonymize import PrivacyStyle
    return PrivacyStyle(K, **kw)


def _three_figures():
    """Three overlapping K = 17 figures on a 70 x 50 picture: heads near (20, 10), (34, 14) and (50, 22)."""
    rng = np.random.default_rng(21)
    kpts = np.empty((3, 17, 3), np.float32)
    for p, (cx, cy) in enumerate(((20.0, 10.0), (34.0, 14.0), (50.0, 22.0))):
        kpts[p, :5, 0] = cx + rng.uniform(-3, 3, 5)
        kpts[p, :5, 1] = cy + rng.uniform(-3, 3, 5)
        kpts[p, 5:, 0] = cx + rng.uniform(-12, 12, 12)
        kpts[p, 5:, 1] = cy + rng.uniform(4, 26, 12)
        kpts[p, :, 2] = 0.9
    bboxes = np.stack([kpts[..., 0].min(1), kpts[..., 1].min(1), kpts[..., 0].max(1), kpts[..., 1].max(1),
                       np.full(3, 0.9)], 1).astype(np.float32)
    return kpts, bboxes


def _surface(H, W, pitch, seed=0, sentinel=0xA5):
    rng = np.random.default_rng(seed)
    s = np.full((H * 3 // 2, pitch), sentinel, np.uint8)
    s[:, :W] = rng.integers(0, 256, (H * 3 // 2, W), dtype=np.uint8)
    return s


@pytest.mark.parametrize('region', ['head', 'person'])
@pytest.mark.parametrize('cell', [2, 8, 16])
def test_oracle_properties(cell, region):
    """70 x 50 NV12 at pitch 96, three overlapping figures: twice equals once, the pose order does not matter, the
    pitch padding keeps its bytes, nothing outside the masked cells changes, and 'fill' writes the bgr_to_yuv triple."""
    from pavenet_amd.render import bgr_to_yuv
    W, H, pitch = 70, 50, 96
    kpts, bboxes = _three_figures()
    before = _surface(H, W, pitch, seed=cell)
    style = _style(cell=cell, region=region)
    regs = AR.regions(kpts, bboxes, None, (1.0, 1.0), style)
    assert len(regs) == 3
    pix = AR.pixel_mask(W, H, cell, regs)
    assert pix.any() and (region == 'person' or not pix.all())
    once = AR.anonymize_nv12(before, W, kpts, bboxes, None, (1.0, 1.0), style)
    assert (once != before).any()
    assert np.array_equal(AR.anonymize_nv12(once, W, kpts, bboxes, None, (1.0, 1.0), style), once)
    assert np.array_equal(AR.anonymize_nv12(before, W, kpts[::-1], bboxes[::-1], None, (1.0, 1.0), style), once)
    assert (once[:, W:] == 0xA5).all()
    assert np.array_equal(once[:H, :W][~pix], before[:H, :W][~pix])
    cpix = pix[::2, ::2]                      # a chroma sample's cell is its 2 x 2 block's cell: cells are even
    for c in (0, 1):
        assert np.array_equal(once[H:, c:W:2][~cpix], before[H:, c:W:2][~cpix])
    if cell == 2:                             # one chroma sample per cell: unchanged
        assert np.array_equal(once[H:], before[H:])
    # a cell's mean lies between its extremes, and is exact where the cell is flat
    flat = before.copy()
    flat[:H, :W] = 77
    assert (AR.anonymize_nv12(flat, W, kpts, bboxes, None, (1.0, 1.0), style)[:H, :W] == 77).all()
    for matrix, full_range in (('bt601', False), ('bt601', True), ('bt709', False), ('bt709', True)):
        fill = _style(cell=cell, region=region, mode='fill', fill_color=(200, 30, 90))
        got = AR.anonymize_nv12(before, W, kpts, bboxes, None, (1.0, 1.0), fill, matrix, full_range)
        y, u, v = (int(t) for t in bgr_to_yuv((200, 30, 90), matrix, full_range))
        assert (y, u, v) == RR.bgr_to_yuv((200, 30, 90), matrix, full_range)
        assert (got[:H, :W][pix] == y).all() and np.array_equal(got[:H, :W][~pix], before[:H, :W][~pix])
        assert (got[H:, 0:W:2][cpix] == u).all() and (got[H:, 1:W:2][cpix] == v).all()
        assert (got[:, W:] == 0xA5).all()


def test_rounded_mean_and_regions_by_hand():
    """The numbers of the rule on a case small enough to do by hand."""
    style = _style(15, cell=4, head_scale=0, head_min=0)
    kpts = np.zeros((1, 15, 3), np.float32)
    kpts[0, :, :2] = (5.0, 6.0)
    kpts[0, 0, 2] = 0.9                                   # the nose alone is visible
    bboxes = np.asarray([[9.0, 7.0, 1.0, 2.0, 0.9]], np.float32)     # corners swapped
    assert AR.regions(kpts, bboxes, None, (1.0, 1.0), style) == [(20, 24, 20, 24, 0)]
    mask = AR.cell_mask(12, 12, 4, [(20, 24, 20, 24, 0)])
    assert mask.sum() == 1 and mask[1, 1]                 # exactly the cell holding pixel (5, 6)
    person = _style(15, region='person', margin=3, grow=5)
    assert AR.regions(kpts, bboxes, None, (1.0, 1.0), person) == [(4, 8, 36, 28, 12 + ((32 * 5) >> 4))]
    none = _style(15, fallback='skip', kpt_thr=0.95)
    assert AR.regions(kpts, bboxes, None, (1.0, 1.0), none) == []
    fallback = _style(15, kpt_thr=0.95)
    assert AR.regions(kpts, bboxes, None, (1.0, 1.0), fallback) == [(4, 8, 36, 28, (32 * 2) >> 4)]
    img = np.zeros((4, 4, 3), np.uint8)
    img[..., 0] = np.arange(16).reshape(4, 4)             # sum 120, n 16: (240 + 16) // 32 = 8
    img[0, 0, 1] = 8                                      # sum 8: (16 + 16) // 32 = 1
    img[0, 0, 2] = 7                                      # sum 7: (14 + 16) // 32 = 0
    kpts[0, :, :2] = (1.0, 1.0)
    out = AR.anonymize_bgr(img, kpts, np.asarray([[0, 0, 3, 3, 0.9]], np.float32), None, (1.0, 1.0), style)
    assert (out[..., 0] == 8).all() and (out[..., 1] == 1).all() and (out[..., 2] == 0).all()


@pytest.mark.parametrize('height', [40, 100, 300])
def test_default_head_region_covers_the_head(height):
    """The K = 15 figure, `height` px tall, placed uniformly inside 640 x 480 with 1 % jitter, 20 seeded placements,
    every cell size, the default style: every pixel of the head's ellipse (centre (x0 + .20 h, y0 + .07 h), semi-axes
    .055 h x .07 h, float64) lies in a masked cell whenever the nose is among the visible head key points.  (With only
    head top or only head bottom visible the disc is centred on an end of the head and 190 of the 720 such cases cover
    84 - 99 % of the ellipse; head_min=3 covers all of them.  A documented limit of the defaults, not asserted.)"""
    W, H = 640, 480
    rng = np.random.default_rng(1000 + height)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    cases = 0
    for _ in range(20):
        x0, y0 = rng.uniform(0, W - 0.40 * height), rng.uniform(0, H - 1.0 * height)
        xy = FIGURE * height + (x0, y0)
        xy = xy + rng.uniform(-0.01, 0.01, xy.shape) * height
        ellipse = ((xs - (x0 + 0.20 * height)) / (0.055 * height)) ** 2 + ((ys - (y0 + 0.07 * height)) / (0.07 * height)) ** 2 <= 1.0
        assert ellipse.any()
        bbox = np.asarray([[xy[:, 0].min(), xy[:, 1].min(), xy[:, 0].max(), xy[:, 1].max(), 0.8]], np.float32)
        for visible in ((0, 1, 2), (0,), (0, 1), (0, 2)):
            kpts = np.zeros((1, 15, 3), np.float32)
            kpts[0, :, :2] = xy
            kpts[0, 3:, 2] = 0.9
            kpts[0, list(visible), 2] = 0.9
            for cell in CELLS:
                style = _style(15, cell=cell)
                regs = AR.regions(kpts, bbox, None, (1.0, 1.0), style)
                assert len(regs) == 1
                pix = AR.pixel_mask(W, H, cell, regs)
                missed = int((ellipse & ~pix).sum())
                assert missed == 0, (height, visible, cell, missed, int(ellipse.sum()))
                cases += 1
    assert cases == 20 * 4 * 6
