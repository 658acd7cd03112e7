"""Zones, lines and counts drawn on the device (csrc/pave_overlay.hip) against the rule of DESIGN section 19 in numpy
(tests/zone_draw_ref.py): torch.equal of the WHOLE allocation -- the picture is pre-filled with a pattern and the
pitch padding with a sentinel, so a byte written where the rule writes none fails.  The oracle reads the geometry,
the counters and the state from the monitor's own tensors, copied to the host.  Needs an MI355X."""
import math

import numpy as np
import pytest
import torch

from tests import render_ids_ref as IR
from tests import zone_draw_ref as RD
from tests import zones_cases as ZC

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
U_SHAPE = [(6, 6), (60, 6), (60, 44), (44, 44), (44, 20), (22, 20), (22, 44), (6, 44)]


def nv12_surface(H, W, pitch, seed=0):
    s = torch.full((H * 3 // 2, pitch), SENTINEL, dtype=torch.uint8)
    s[:, :W] = torch.from_numpy(np.random.default_rng(seed).integers(0, 256, (H * 3 // 2, W), dtype=np.uint8))
    return s


def bgr_buffer(H, W, pitch, seed=0):
    """[H, pitch] bytes: the picture in the first 3 W columns, the sentinel in the padding."""
    s = torch.full((H, pitch), SENTINEL, dtype=torch.uint8)
    s[:, :3 * W] = torch.from_numpy(np.random.default_rng(seed).integers(0, 256, (H, 3 * W), dtype=np.uint8))
    return s


def host(mon, camera):
    """(geometry, counts, state) of one camera as numpy: what the oracle draws from."""
    to = lambda d: {k: v.cpu().numpy() for k, v in d.items()}
    return to(mon.geometry(camera)), to(mon.counts(camera)), to(mon.state(camera))


def frozen(mon):
    return {k: v.clone() for k, v in mon._state.items()}


def unchanged(mon, before):
    assert sorted(mon._state) == sorted(before)
    for name, t in before.items():
        assert torch.equal(mon._state[name], t), f'the draw wrote into the monitor\'s {name}'


def same(got, want, what=''):
    got, want = got.cpu(), torch.from_numpy(want) if isinstance(want, np.ndarray) else want.cpu()
    diff = (got != want).nonzero()
    assert got.shape == want.shape and torch.equal(got, want), \
        f'{what}: {len(diff)} bytes differ, first at {diff[:5].tolist()}: {got[got != want][:5].tolist()} for ' \
        f'{want[got != want][:5].tolist()}'


def check_nv12(mon, H, W, pitch, style, camera=0, matrix='bt601', full_range=False, seed=0):
    from pavenet_amd import draw_zones_nv12
    before = nv12_surface(H, W, pitch, seed)
    dev, state = before.cuda(), frozen(mon)
    assert draw_zones_nv12(dev, W, mon, camera=camera, style=style, matrix=matrix, full_range=full_range) is dev
    want = RD.draw_nv12(before.numpy(), W, *host(mon, camera), style, font(), matrix, full_range)
    same(dev, want, f'nv12 {W} x {H}')
    unchanged(mon, state)
    return dev.cpu(), before


def check_bgr(mon, H, W, pitch, style, camera=0, seed=0):
    from pavenet_amd import draw_zones_bgr
    before = bgr_buffer(H, W, pitch, seed)
    dev, state = before.cuda(), frozen(mon)
    image = dev[:, :3 * W].unflatten(1, (W, 3))
    assert draw_zones_bgr(image, mon, camera=camera, style=style) is image
    want = before.numpy().copy()
    want[:, :3 * W] = RD.draw_bgr(before.numpy()[:, :3 * W].reshape(H, W, 3), *host(mon, camera), style, font()).reshape(H, 3 * W)
    same(dev, want, f'bgr {W} x {H}')
    unchanged(mon, state)
    return dev.cpu(), before


def font():
    from pavenet_amd.overlay import ZONE_FONT
    return ZONE_FONT


def monitor(zones, lines, cameras=1, K=1, dwell_frames=None, **kw):
    from pavenet_amd.zones import ZoneMonitor
    mon = ZoneMonitor(K, cameras=cameras, **({'anchor_kpts': (0,)} if K == 1 else {}), **kw)
    mon.set_zones(0, zones, lines, dwell_frames)
    return mon


def set_counts(mon, camera=0, **values):
    """Writes through the views of counts(): occupancy=[...], crossed=[[f, b], ...]."""
    views = mon.counts(camera)
    for name, v in values.items():
        t = torch.from_numpy(np.asarray(v, np.int64).astype(np.int32)).cuda()
        views[name][tuple(slice(0, n) for n in t.shape)] = t


def ring(cx, cy, r, phase=0.0, n=16):
    return [(cx + r * math.cos(phase + 2 * math.pi * i / n), cy + r * math.sin(phase + 2 * math.pi * i / n)) for i in range(n)]


def full_style(**kw):
    from pavenet_amd import ZoneStyle
    return ZoneStyle(**kw)


SMALL_ZONES = [[(0, 0), (40, 0), (40, 36), (0, 36)], [(1.5, 0.625), (33.125, 2), (20, 33.5)]]
SMALL_LINES = [((0, 1), (33, 30)), ((1, 0), (1, 1))]


@pytest.mark.parametrize('H, W, pitch', [(2, 2, 2), (34, 34, 34), (64, 96, 128)])
def test_nv12_small_and_ragged_sizes(H, W, pitch):
    mon = monitor(SMALL_ZONES, SMALL_LINES)
    set_counts(mon, occupancy=[3, 0], crossed=[[2, 14], [0, 0]])
    got, before = check_nv12(mon, H, W, pitch, full_style(label_scale=1), seed=H)
    assert (got != before).any() and torch.equal(got[:, W:], before[:, W:])


@pytest.mark.parametrize('H, W, pitch', [(1, 1, 3), (31, 33, 99), (50, 70, 240)])
def test_bgr_small_and_ragged_sizes(H, W, pitch):
    mon = monitor(SMALL_ZONES, SMALL_LINES)
    set_counts(mon, occupancy=[3, 0], crossed=[[2, 14], [0, 0]])
    got, before = check_bgr(mon, H, W, pitch, full_style(label_scale=1), seed=W)
    assert (got != before).any() and torch.equal(got[:, 3 * W:], before[:, 3 * W:])


@pytest.mark.parametrize('kind', ['nv12', 'bgr'])
def test_primitives_straddle_tile_edges_and_the_borders(kind):
    """70 x 50: tile boundaries at 32 and 64.  A zone over x = 32 and y = 32 that leaves the picture on the right and
    at the bottom, a line through both boundaries into the bottom-right corner with its stem and its plate over
    x = 64, and a zone plate about (32, 32)."""
    zones = [[(8, 8), (90, 8), (90, 70), (56, 56), (8, 56)], [(60, 40), (80, 40), (80, 60), (60, 60)]]
    lines = [((20, 10), (76, 48)), ((68, 2), (60, 30))]
    mon = monitor(zones, lines)
    set_counts(mon, occupancy=[12, 0], crossed=[[130, 7], [0, 25]])
    style = full_style(outline=3, thickness=2, arrow=20, label_scale=2)
    ids, _ = RD.id_map(70, 50, *host(mon, 0), style, font())
    # what shows: zone edges (the others are outside the picture or under something), both lines, stems and labels
    assert sorted(set(ids.reshape(-1).tolist())) == [-1, 0, 4, 16, 19, 128, 129, 136, 137, 144, 145, 146, 147, 160, 161, 162, 163]
    for pid in (128, 144, 160):     # on both sides of a tile boundary in x
        ys, xs = np.nonzero(ids >= pid) if pid >= 144 else np.nonzero(ids == pid)
        assert xs.min() < 32 <= xs.max() and ys.min() < 32 <= ys.max(), pid
    stem = [c for c in RD.primitives(*host(mon, 0), style)[0] if c[0] == 136][0]
    assert stem[1] == (192, 116) and stem[2] == (147, 182)          # from y = 29 over the boundary at 32 to y = 45.5
    assert (ids[:, 69] >= 0).any() and (ids[49] >= 0).any() and (ids[:, 64:] >= 144).any()
    if kind == 'nv12':
        check_nv12(mon, 50, 70, 96, style, matrix='bt709')
    else:
        check_bgr(mon, 50, 70, 3 * 70 + 5, style)


def eight_by_sixteen():
    zones = [ring(20 + 11 * z, 30 + 5 * (z % 3), 12 + 2 * z, phase=0.2 * z) for z in range(8)]
    lines = [((4 + 12 * l, 2 + 3 * l), (90 - 9 * l, 60 - 6 * l)) for l in range(8)]
    return zones, lines


@pytest.mark.parametrize('kind', ['nv12', 'bgr'])
def test_full_geometry(kind):
    """8 zones of 16 vertices and 8 lines, overlapping, every label shown, some zones occupied and one alerted."""
    mon = monitor(*eight_by_sixteen(), max_tracks=128)
    set_counts(mon, occupancy=[0, 1, 0, 25, 0, 0, 3, 0], entered=[5] * 8, appeared=[1, 2, 3, 4, 5, 6, 7, 8],
               crossed=[[l, 2 * l] for l in range(8)])
    st = mon.state(0)
    st['id'][127], st['inside'][127], st['alerted'][127] = 9, 0b101, 0b100      # zone 2 alerted, by the last slot
    for zone_label, line_label in (('occupancy', 'net'), ('entered', 'backward')):
        style = full_style(label_scale=1, zone_label=zone_label, line_label=line_label, arrow=9, thickness=1, outline=1)
        got, before = (check_nv12(mon, 64, 96, 128, style, full_range=True) if kind == 'nv12' else
                       check_bgr(mon, 64, 96, 3 * 96, style))
        assert (got != before).float().mean() > 0.3


@pytest.mark.parametrize('kind', ['nv12', 'bgr'])
def test_concave_u(kind):
    mon = monitor([U_SHAPE], [])
    style = full_style(alpha=200, outline=0, label_scale=0)
    got, before = check_nv12(mon, 48, 64, 64, style) if kind == 'nv12' else check_bgr(mon, 48, 64, 192, style)
    mask = RD.fill_mask(64, 48, [(8 * x, 8 * y) for x, y in U_SHAPE])
    assert not mask[30, 30] and mask[10, 30] and mask[30, 10] and mask[30, 50]      # the notch is outside
    step = 1 if kind == 'nv12' else 3
    changed = (got != before)[:48, :64 * step:step]
    assert not changed[~torch.from_numpy(mask)].any() and changed[torch.from_numpy(mask)].float().mean() > 0.9


def test_nothing_to_draw_leaves_the_buffer_bit_identical():
    """A camera without geometry, and a monitor that has no state yet."""
    from pavenet_amd import draw_zones_bgr, draw_zones_nv12
    from pavenet_amd.zones import ZoneMonitor
    mon = monitor(SMALL_ZONES, SMALL_LINES, cameras=2)
    for m in (mon, ZoneMonitor(15, cameras=2)):
        nv, bgr = nv12_surface(34, 34, 40).cuda(), bgr_buffer(31, 33, 99).cuda().view(31, 33, 3)
        was_nv, was_bgr = nv.clone(), bgr.clone()
        assert draw_zones_nv12(nv, 34, m, camera=1) is nv and draw_zones_bgr(bgr, m, camera=1) is bgr
        assert torch.equal(nv, was_nv) and torch.equal(bgr, was_bgr)
    assert ZoneMonitor(15)._state is None


def test_both_matrices_and_both_ranges_in_one_launch():
    from pavenet_amd import draw_zones_nv12
    mon = monitor(SMALL_ZONES, SMALL_LINES)
    set_counts(mon, occupancy=[1, 0])
    modes = [('bt601', False), ('bt601', True), ('bt709', False), ('bt709', True)]
    befores = [nv12_surface(34, 34, 48, seed=i) for i in range(4)]
    devs = [b.cuda() for b in befores]
    style = full_style(label_scale=1)
    out = draw_zones_nv12(devs, 34, mon, style=style, matrix=[m for m, _ in modes], full_range=[f for _, f in modes])
    assert out is devs
    wants = [RD.draw_nv12(b.numpy(), 34, *host(mon, 0), style, font(), m, f) for b, (m, f) in zip(befores, modes)]
    for i, (d, w) in enumerate(zip(devs, wants)):
        same(d, w, f'mode {modes[i]}')
    assert len({w.tobytes() for w in wants}) == 4


LABEL_VALUES = (0, 9, 10, 99999, 2 ** 31 - 1, -1, -2 ** 31)


def test_counters_from_a_real_run_then_poked():
    """Frames of tests/zones_cases.py's dwell script through a real ZoneMonitor: a person born inside the square stays
    past its dwell time (the zone turns to the alert colour), crosses the line and leaves.  Then the views of the
    counters and of the state are poked to the label values and the alert cases of the CPU tests."""
    mon = monitor([ZC.SQUARE, [(0, 0), (64, 0), (64, 40), (0, 40)]], [((24, 2), (24, 38))], dwell_frames=[2, 0],
                  min_frames=1, max_tracks=4)
    style = full_style(label_scale=1, arrow=6)
    seen = []
    for f, x in enumerate((15, 15, 15, 15, 30, 30, 15)):
        kp, bb = ZC.pts((x, 15))
        mon.update((torch.from_numpy(bb).cuda(), None, torch.from_numpy(kp).cuda()), torch.tensor([6], dtype=torch.int32).cuda())
        got, _ = check_nv12(mon, 40, 64, 64, style, seed=f)
        check_bgr(mon, 40, 64, 200, style, seed=f)
        geo, cnt, st = host(mon, 0)
        seen.append(([row for row, _ in RD.zone_states(2, cnt, st, style)], cnt['occupancy'][:2].tolist(), cnt['crossed'][0].tolist()))
    assert [s[0][0] for s in seen] == [0, 0, RD.ALERT, RD.ALERT, 0, 0, 0]        # alerted from frame 3 until it leaves
    assert seen[3][1] == [1, 1] and seen[4][1] == [0, 1] and seen[4][2] != seen[3][2] and seen[6][2] == [1, 1]
    # the label values, on the line ('net' = forward - backward wraps as the counters do) and on a zone
    for v in LABEL_VALUES:
        set_counts(mon, occupancy=[v, 0], crossed=[[v, 0]] if v >= 0 else [[0, 1]] if v == -1 else [[-2 ** 31, 0]])
        check_nv12(mon, 40, 64, 64, style, seed=3)
    set_counts(mon, occupancy=[1, 1], entered=[2 ** 31 - 1, 0], appeared=[1, 5], crossed=[[7, 7]])
    check_bgr(mon, 40, 64, 192, full_style(label_scale=2, zone_label='entered', line_label='forward'))
    # the alert cases: a live slot with both bits; one bit each; the same bits in a free slot
    st = mon.state(0)
    for ident, inside, alerted, want in ((7, 2, 2, [0, RD.ALERT]), (7, 3, 1, [RD.ALERT, 1]), (7, 1, 2, [0, 1]), (0, 3, 3, [0, 1]),
                                         (-5, 3, 3, [RD.ALERT, RD.ALERT])):
        st['id'][:] = 0
        st['id'][3], st['inside'][3], st['alerted'][3] = ident, inside, alerted
        geo, cnt, hs = host(mon, 0)
        assert [row for row, _ in RD.zone_states(2, cnt, hs, style)] == want
        check_nv12(mon, 40, 64, 64, style, seed=5)
        check_bgr(mon, 40, 64, 192, style, seed=5)


def test_33_surfaces_of_three_cameras_in_two_launches():
    from pavenet_amd import draw_zones_bgr, draw_zones_nv12
    from pavenet_amd.zones import ZoneMonitor
    mon = ZoneMonitor(1, cameras=3, anchor_kpts=(0,))
    mon.set_zones(0, SMALL_ZONES, SMALL_LINES)
    mon.set_zones(1, [U_SHAPE], [((50, 4), (10, 40))])
    mon.set_zones(2, *eight_by_sixteen())
    for c in range(3):
        set_counts(mon, c, occupancy=[c, 1], crossed=[[10 * c, 3]])
    style = full_style(label_scale=1, arrow=8)
    sizes = [(34 + 2 * (i % 5), 30 + 2 * (i % 7)) for i in range(33)]
    cams = [i % 3 for i in range(33)]
    state = frozen(mon)
    nv = [nv12_surface(H, W, W + (i % 3) * 6, seed=i).cuda() for i, (W, H) in enumerate(sizes)]
    singles = [s.clone() for s in nv]
    assert draw_zones_nv12(nv, [W for W, _ in sizes], mon, camera=cams, style=style, matrix='bt709') is nv
    for i, s in enumerate(singles):
        assert draw_zones_nv12(s, sizes[i][0], mon, camera=cams[i], style=style, matrix='bt709') is s
        assert torch.equal(nv[i], s), i
    for i in (0, 1, 32):
        want = RD.draw_nv12(nv12_surface(sizes[i][1], sizes[i][0], sizes[i][0] + (i % 3) * 6, seed=i).numpy(), sizes[i][0],
                            *host(mon, cams[i]), style, font(), 'bt709', False)
        same(nv[i], want, f'surface {i}')
    bgr = [bgr_buffer(H, W, 3 * W, seed=i).cuda().view(H, W, 3) for i, (W, H) in enumerate(sizes)]
    singles = [s.clone() for s in bgr]
    assert draw_zones_bgr(bgr, mon, camera=cams, style=style) is bgr
    for i, s in enumerate(singles):
        draw_zones_bgr(s, mon, camera=cams[i], style=style)
        assert torch.equal(bgr[i], s), i
    same(bgr[32], RD.draw_bgr(bgr_buffer(sizes[32][1], sizes[32][0], 3 * sizes[32][0], seed=32).view(sizes[32][1], sizes[32][0], 3).numpy(),
                              *host(mon, cams[32]), style, font()), 'bgr surface 32')
    unchanged(mon, state)


def test_drawing_twice_with_full_alphas_is_drawing_once():
    from pavenet_amd import draw_zones_bgr, draw_zones_nv12
    mon = monitor(*eight_by_sixteen())
    set_counts(mon, occupancy=[0, 1, 0, 2, 0, 0, 3, 0])
    style = full_style(alpha=256, alpha_occupied=256, alpha_alert=256, label_scale=1)
    nv, bgr = nv12_surface(64, 96, 100).cuda(), bgr_buffer(64, 96, 288).cuda().view(64, 96, 3)
    was = nv.clone()
    once_nv, once_bgr = draw_zones_nv12(nv, 96, mon, style=style).clone(), draw_zones_bgr(bgr, mon, style=style).clone()
    assert not torch.equal(once_nv, was)
    assert torch.equal(draw_zones_nv12(nv, 96, mon, style=style), once_nv)
    assert torch.equal(draw_zones_bgr(bgr, mon, style=style), once_bgr)


def test_chain_update_zones_poses():
    """ZoneMonitor.update -> draw_zones_nv12 -> draw_poses_nv12(ids=) on one surface against the two oracles in that
    order: skeletons lie over zones."""
    from pavenet_amd import TrackStyle, draw_poses_nv12, draw_zones_nv12
    from pavenet_amd.render import DIGIT_FONT
    from pavenet_amd.zones import ZoneMonitor
    from tests.test_track_gpu import FIGURE15, poses
    mon = ZoneMonitor(15, min_frames=1)
    mon.set_zones(0, [[(4, 30), (60, 30), (60, 62), (4, 62)], U_SHAPE], [((48, 2), (48, 62))], dwell_frames=[1, 0])
    kpts, bboxes = poses(np.random.default_rng(3), FIGURE15, [(10, 8), (52, 6)], height=44.0)
    ids = np.asarray([3, 12], np.int32)
    result = (torch.from_numpy(bboxes).cuda(), None, torch.from_numpy(kpts).cuda())
    dev_ids = torch.from_numpy(ids).cuda()
    for _ in range(3):
        out = mon.update(result, dev_ids)
    assert out['zones'].tolist()[0] & 1 and int(mon.counts(0)['occupancy'][0]) >= 1
    zstyle, pstyle = full_style(label_scale=1), TrackStyle(15, thickness=1, radius=1, label_scale=1)
    before = nv12_surface(64, 96, 128, seed=9)
    dev = before.cuda()
    draw_poses_nv12(draw_zones_nv12(dev, 96, mon, style=zstyle), 96, result, style=pstyle, ids=dev_ids)
    mid = RD.draw_nv12(before.numpy(), 96, *host(mon, 0), zstyle, font())
    want = IR.draw_nv12(mid, 96, kpts, bboxes, None, ids, (1.0, 1.0), pstyle, pstyle.palette, DIGIT_FONT, 'bt601', False)
    assert (mid != before.numpy()).any() and (want != mid).any()
    same(dev, want, 'chain')


def test_no_allocation_in_100_calls():
    from pavenet_amd import draw_zones_bgr, draw_zones_nv12
    mon = monitor(SMALL_ZONES, SMALL_LINES)
    style = full_style()
    nv, bgr = nv12_surface(64, 96, 128).cuda(), bgr_buffer(50, 70, 210).cuda().view(50, 70, 3)
    draw_zones_nv12(nv, 96, mon, style=style)
    draw_zones_bgr(bgr, mon, style=style)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    for _ in range(100):
        draw_zones_nv12(nv, 96, mon, style=style)
        draw_zones_bgr(bgr, mon, style=style)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() == base == torch.cuda.memory_allocated()
