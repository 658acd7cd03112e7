"""Footfall maps drawn on the device (csrc/pave_heat.hip, pave_draw_heat_nv12 / _bgr) against the draw rule of DESIGN
section 21 in numpy (tests/heat_draw_ref.py): torch.equal of the WHOLE allocation -- the picture is pre-filled with a
pattern and the pitch padding with a sentinel, so a byte written where the rule writes none fails.  The oracle reads the
maps and the peak from the map's own tensors, copied to the host.  Needs an MI355X."""
import numpy as np
import pytest
import torch

from tests import heat_draw_ref as DR
from tests.test_zone_draw_gpu import bgr_buffer, nv12_surface, same

pytestmark = pytest.mark.gpu


def heat_map(size, cell, cameras=1, seed=0, fill=None, **kw):
    """A FootfallMap whose maps are written here: random words, a third of them 0 and a few negative, or `fill`."""
    from pavenet_amd import FootfallMap
    fmap = FootfallMap(1, size=size, cell=cell, cameras=cameras, anchor_kpts=(0,), **kw)
    fmap._allocate(torch.device('cuda', torch.cuda.current_device()))
    rng = np.random.default_rng(seed)
    for c in range(cameras):
        for m, name in enumerate(('dwell', 'visits')):
            v = rng.integers(0, 1000, (fmap.Gh, fmap.Gw)).astype(np.int32)
            v[rng.random(v.shape) < 0.33] = 0
            v[rng.random(v.shape) < 0.05] = -7
            v[0, 0] = 500 + m                                    # (a grid of one cell still shows something)
            if fill is not None:
                v[:] = fill
            fmap.maps(c)[name].copy_(torch.from_numpy(v))
            fmap.maps(c)['peak'][m] = int(max(v.max(), 0))
    return fmap


def host(fmap, camera):
    return {k: v.cpu().numpy() for k, v in fmap.maps(camera).items()}


def frozen(fmap):
    return {k: v.clone() for k, v in fmap._state.items()}


def unchanged(fmap, before):
    for name, t in before.items():
        assert torch.equal(fmap._state[name], t), f'the draw wrote into the map\'s {name}'


def check_nv12(fmap, H, W, pitch, style, camera=0, matrix='bt601', full_range=False, seed=0):
    from pavenet_amd import draw_heat_nv12
    before = nv12_surface(H, W, pitch, seed)
    dev, state = before.cuda(), frozen(fmap)
    assert draw_heat_nv12(dev, W, fmap, camera=camera, style=style, matrix=matrix, full_range=full_range) is dev
    want = DR.draw_nv12(before.numpy(), W, host(fmap, camera), fmap.size, fmap.cell, style, matrix, full_range)
    same(dev, want, f'nv12 {W} x {H} cell {fmap.cell} smooth {style.smooth}')
    unchanged(fmap, state)
    return dev.cpu(), before


def check_bgr(fmap, H, W, pitch, style, camera=0, seed=0):
    from pavenet_amd import draw_heat_bgr
    before = bgr_buffer(H, W, pitch, seed)
    dev, state = before.cuda(), frozen(fmap)
    image = dev[:, :3 * W].unflatten(1, (W, 3))
    assert draw_heat_bgr(image, fmap, camera=camera, style=style) is image
    want = before.numpy().copy()
    want[:, :3 * W] = DR.draw_bgr(before.numpy()[:, :3 * W].reshape(H, W, 3), host(fmap, camera), fmap.size, fmap.cell,
                                  style).reshape(H, 3 * W)
    same(dev, want, f'bgr {W} x {H} cell {fmap.cell} smooth {style.smooth}')
    unchanged(fmap, state)
    return dev.cpu(), before


def styles(**kw):
    from pavenet_amd import HeatStyle
    return [HeatStyle(smooth=s, **kw) for s in (True, False)]


@pytest.mark.parametrize('H, W, pitch', [(2, 2, 2), (34, 34, 34), (64, 96, 128)])
def test_nv12_small_and_ragged_sizes(H, W, pitch):
    fmap = heat_map((W, H), 4, seed=H)
    for style in styles() + styles(source='visits', alpha_max=256, floor=40):
        got, before = check_nv12(fmap, H, W, pitch, style, seed=H)
        assert (got != before).any() and torch.equal(got[:, W:], before[:, W:])


@pytest.mark.parametrize('H, W, pitch', [(1, 1, 3), (31, 33, 99), (50, 70, 240)])
def test_bgr_small_and_ragged_sizes(H, W, pitch):
    """(the last one: rows of a wider buffer)"""
    fmap = heat_map((W, H), 4, seed=W)
    for style in styles() + styles(source='visits', full_scale=300):
        got, before = check_bgr(fmap, H, W, pitch, style, seed=W)
        assert (got != before).any() and torch.equal(got[:, 3 * W:], before[:, 3 * W:])


@pytest.mark.parametrize('cell', [4, 8, 16, 32, 64])
def test_every_cell_size_and_surfaces_larger_and_smaller_than_the_map(cell):
    """A 150 x 90 map (odd in cells at every cell size; an odd 75 x 45 one for NV12's chroma at the map's edge) under
    a surface larger than it -- the bytes beyond the map stay -- and under one smaller."""
    fmap, odd = heat_map((150, 90), cell, seed=cell), heat_map((75, 45), cell, seed=cell + 1)
    for style in styles(floor=0):
        got, before = check_nv12(fmap, 128, 192, 192, style)
        assert torch.equal(got[90:128], before[90:128]) and torch.equal(got[:128, 150:], before[:128, 150:])
        assert torch.equal(got[128 + 45:], before[128 + 45:]) and (got[:90, :150] != before[:90, :150]).any()
        check_nv12(odd, 64, 96, 128, style)
        check_nv12(fmap, 64, 96, 96, style)
        check_bgr(fmap, 100, 161, 500, style)
        check_bgr(odd, 100, 161, 483, style)
        check_bgr(fmap, 31, 33, 99, style)


@pytest.mark.parametrize('kind', ['nv12', 'bgr'])
def test_hot_cells_in_the_corners_and_on_a_tile_boundary(kind):
    """One hot cell in each corner and one on either side of the tile boundary at x = 32, the rest 0: with smooth the
    tint spreads up to the neighbouring cells' centres (x = 44 and x = 84), and nothing between them is written."""
    fmap = heat_map((96, 64), 8, fill=0)
    d = fmap.maps(0)['dwell']
    for gy, gx, v in ((0, 0, 9), (0, 11, 5), (7, 0, 3), (7, 11, 9), (3, 3, 7), (4, 4, 8)):
        d[gy, gx] = v
    fmap.maps(0)['peak'][0] = 9
    for style in styles():
        got, before = (check_nv12(fmap, 64, 96, 128, style) if kind == 'nv12' else check_bgr(fmap, 64, 96, 300, style))
        changed = (got != before)
        region = changed[:64, 48:80] if kind == 'nv12' else changed[:, 3 * 48:3 * 80]
        assert changed.any() and not region[16:48].any()


def test_an_all_zero_map_writes_nothing():
    from pavenet_amd import draw_heat_bgr, draw_heat_nv12
    fmap = heat_map((96, 64), 8, fill=0)
    for style in styles(floor=0, alpha_max=256):
        got, before = check_nv12(fmap, 64, 96, 128, style)
        assert torch.equal(got, before)
        got, before = check_bgr(fmap, 50, 70, 240, style)
        assert torch.equal(got, before)
    # and a map without state draws nothing and launches nothing
    from pavenet_amd import FootfallMap
    empty = FootfallMap(15, size=(96, 64))
    nv, bgr = nv12_surface(64, 96, 128).cuda(), bgr_buffer(50, 70, 210).cuda().view(50, 70, 3)
    keep = nv.clone(), bgr.clone()
    assert draw_heat_nv12(nv, 96, empty) is nv and draw_heat_bgr(bgr, empty) is bgr and empty._state is None
    assert torch.equal(nv, keep[0]) and torch.equal(bgr, keep[1])


def test_the_peak_is_read_on_the_device_with_no_new_upload():
    """full_scale=None: a real update changes the map and its peak on the device; the next draw follows it with the
    palette that was uploaded for the first."""
    from pavenet_amd import HeatStyle
    from tests.heat_cases import pts
    fmap = heat_map((96, 64), 8, fill=0, radius=2)
    style = HeatStyle(smooth=True)
    kp, bb = pts((20, 20), (70, 40))
    res = (torch.from_numpy(bb).cuda(), None, torch.from_numpy(kp).cuda())
    ids = torch.tensor([1, 2], dtype=torch.int32, device='cuda')
    fmap.update(res, ids)
    first, _ = check_nv12(fmap, 64, 96, 128, style)
    tables = dict(style._device)
    assert len(tables) == 1
    kp2, bb2 = pts((20, 20))
    for _ in range(3):
        fmap.update((torch.from_numpy(bb2).cuda(), None, torch.from_numpy(kp2).cuda()), ids[:1])
    assert fmap.maps(0)['peak'].tolist() == [36, 1]
    second, _ = check_nv12(fmap, 64, 96, 128, style)
    assert not torch.equal(first, second)                 # the second person's spot is now at a quarter of the scale
    assert list(style._device) == list(tables) and all(style._device[k] is tables[k] for k in tables)
    check_bgr(fmap, 64, 96, 288, style)
    assert list(style._device) == list(tables)


def test_both_matrices_and_both_ranges_in_one_launch():
    from pavenet_amd import HeatStyle, draw_heat_nv12
    fmap = heat_map((96, 64), 16, seed=5)
    style = HeatStyle()
    modes = [('bt601', False), ('bt709', True), ('bt709', False), ('bt601', True)]
    before = [nv12_surface(64, 96, 128, seed=i) for i in range(4)]
    dev = [b.cuda() for b in before]
    state = frozen(fmap)
    assert draw_heat_nv12(dev, 96, fmap, style=style, matrix=[m for m, _ in modes], full_range=[f for _, f in modes]) is dev
    wants = [DR.draw_nv12(b.numpy(), 96, host(fmap, 0), fmap.size, fmap.cell, style, m, f) for b, (m, f) in zip(before, modes)]
    for i, (d, w) in enumerate(zip(dev, wants)):
        same(d, w, f'surface {i}')
    assert (wants[0] != DR.draw_nv12(before[0].numpy(), 96, host(fmap, 0), fmap.size, fmap.cell, style, 'bt709', True)).any()
    unchanged(fmap, state)


def test_33_surfaces_of_three_cameras_in_two_launches():
    from pavenet_amd import HeatStyle, draw_heat_bgr, draw_heat_nv12
    fmap = heat_map((48, 32), 8, cameras=3, seed=7)
    style = HeatStyle(smooth=True, floor=30)
    sizes = [((2 + 2 * (i % 5)) * 4, (1 + i % 4) * 8) for i in range(33)]        # (W, H), all even
    cams = [i % 3 for i in range(33)]
    before = [nv12_surface(H, W, W + 2 * (i % 3), seed=i) for i, (W, H) in enumerate(sizes)]
    dev = [b.cuda() for b in before]
    draw_heat_nv12(dev, [W for W, _ in sizes], fmap, camera=cams, style=style)
    for i, (b, d, (W, H), c) in enumerate(zip(before, dev, sizes, cams)):
        same(d, DR.draw_nv12(b.numpy(), W, host(fmap, c), fmap.size, fmap.cell, style), f'surface {i}')
        one = b.cuda()
        draw_heat_nv12(one, W, fmap, camera=c, style=style)
        assert torch.equal(one, d)
    before = [torch.from_numpy(np.random.default_rng(i).integers(0, 256, (H, W, 3), dtype=np.uint8)) for i, (W, H) in enumerate(sizes)]
    dev = [b.cuda() for b in before]
    draw_heat_bgr(dev, fmap, camera=cams, style=style)
    for i, (b, d, c) in enumerate(zip(before, dev, cams)):
        same(d, DR.draw_bgr(b.numpy(), host(fmap, c), fmap.size, fmap.cell, style), f'image {i}')


def test_chain_update_heat_zones_poses():
    """FootfallMap.update and ZoneMonitor.update -> draw_heat_nv12 -> draw_zones_nv12 -> draw_poses_nv12(ids=) on one
    surface against the three oracles in that order: zones lie over the map, skeletons over both."""
    from pavenet_amd import FootfallMap, HeatStyle, TrackStyle, ZoneStyle, draw_heat_nv12, draw_poses_nv12, draw_zones_nv12
    from pavenet_amd.overlay import ZONE_FONT
    from pavenet_amd.render import DIGIT_FONT
    from pavenet_amd.zones import ZoneMonitor
    from tests import render_ids_ref as IR
    from tests import zone_draw_ref as RD
    from tests.test_track_gpu import FIGURE15, poses
    from tests.test_zone_draw_gpu import U_SHAPE
    from tests.test_zone_draw_gpu import host as zone_host
    mon, fmap = ZoneMonitor(15, min_frames=1), FootfallMap(15, size=(96, 64), cell=4, radius=2)
    mon.set_zones(0, [[(4, 30), (60, 30), (60, 62), (4, 62)], U_SHAPE], [((48, 2), (48, 62))], dwell_frames=[1, 0])
    ids = np.asarray([3, 12], np.int32)
    dev_ids = torch.from_numpy(ids).cuda()
    rng = np.random.default_rng(3)
    for f in range(3):
        kpts, bboxes = poses(rng, FIGURE15, [(10 + 3 * f, 8), (52, 6 + f)], height=44.0)
        result = (torch.from_numpy(bboxes).cuda(), None, torch.from_numpy(kpts).cuda())
        mon.update(result, dev_ids)
        out = fmap.update(result, dev_ids)
    assert (out['cell'] >= 0).all() and int(fmap.maps(0)['peak'][0]) >= 9
    hstyle, zstyle, pstyle = HeatStyle(), ZoneStyle(label_scale=1), TrackStyle(15, thickness=1, radius=1, label_scale=1)
    before = nv12_surface(64, 96, 128, seed=9)
    dev = before.cuda()
    draw_poses_nv12(draw_zones_nv12(draw_heat_nv12(dev, 96, fmap, style=hstyle), 96, mon, style=zstyle), 96, result,
                    style=pstyle, ids=dev_ids)
    heat = DR.draw_nv12(before.numpy(), 96, host(fmap, 0), fmap.size, fmap.cell, hstyle)
    mid = RD.draw_nv12(heat, 96, *zone_host(mon, 0), zstyle, ZONE_FONT)
    want = IR.draw_nv12(mid, 96, kpts, bboxes, None, ids, (1.0, 1.0), pstyle, pstyle.palette, DIGIT_FONT, 'bt601', False)
    assert (heat != before.numpy()).any() and (mid != heat).any() and (want != mid).any()
    same(dev, want, 'chain')


def test_no_allocation_in_100_calls():
    from pavenet_amd import HeatStyle, draw_heat_bgr, draw_heat_nv12
    fmap = heat_map((96, 64), 8, seed=11)
    style = HeatStyle()
    nv, bgr = nv12_surface(64, 96, 128).cuda(), bgr_buffer(50, 70, 210).cuda().view(50, 70, 3)
    draw_heat_nv12(nv, 96, fmap, style=style)
    draw_heat_bgr(bgr, fmap, style=style)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    for _ in range(100):
        draw_heat_nv12(nv, 96, fmap, style=style)
        draw_heat_bgr(bgr, fmap, style=style)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() == base == torch.cuda.memory_allocated()
