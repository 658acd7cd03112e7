"""Track trails drawn on the device (csrc/pave_trails.hip, pave_draw_trails_nv12 / _bgr) against the draw rule of DESIGN
section 22 in numpy (tests/trail_draw_ref.py): torch.equal of the WHOLE allocation -- the picture is pre-filled with a
pattern and the pitch padding with a sentinel, so a byte written where the rule writes none fails.  Every case first
asserts on the oracle alone that some bytes changed and some did not.  The oracle reads the state from the trails' own
tensors, copied to the host.  Needs an MI355X."""
import numpy as np
import pytest
import torch

from tests import trail_draw_ref as DR
from tests.heat_cases import pts
from tests.test_zone_draw_gpu import bgr_buffer, nv12_surface, same

pytestmark = pytest.mark.gpu


def style(**kw):
    from pavenet_amd import TrailStyle
    return TrailStyle(**kw)


def loaded(states, L, S=None):
    """A TrackTrails whose state is written here: one numpy state (DR.state_from) per camera."""
    from pavenet_amd import TrackTrails
    S = states[0]['id'].shape[0] if S is None else S
    trails = TrackTrails(1, cameras=len(states), max_tracks=S, length=L, anchor_kpts=(0,))
    trails._allocate(torch.device('cuda', torch.cuda.current_device()))
    for c, st in enumerate(states):
        for name, t in trails._state.items():
            t[c].copy_(torch.from_numpy(np.asarray(st[name])))
    return trails


def host(trails, camera):
    return {k: v[camera].cpu().numpy() for k, v in trails._state.items()}


def frozen(trails):
    return {k: v.clone() for k, v in trails._state.items()}


def unchanged(trails, before):
    assert sorted(trails._state) == sorted(before)
    for name, t in before.items():
        assert torch.equal(trails._state[name], t), f'the draw wrote into the trails\' {name}'


def check_nv12(trails, H, W, pitch, style, camera=0, matrix='bt601', full_range=False, seed=0, drawn=True):
    from pavenet_amd import draw_trails_nv12
    before = nv12_surface(H, W, pitch, seed)
    want = DR.draw_nv12(before.numpy(), W, host(trails, camera), style, matrix, full_range)
    assert (want != before.numpy()).any() == drawn and (want == before.numpy()).any()
    dev, state = before.cuda(), frozen(trails)
    assert draw_trails_nv12(dev, W, trails, camera=camera, style=style, matrix=matrix, full_range=full_range) is dev
    same(dev, want, f'nv12 {W} x {H}')
    unchanged(trails, state)
    return dev.cpu(), before


def check_bgr(trails, H, W, pitch, style, camera=0, seed=0, drawn=True):
    from pavenet_amd import draw_trails_bgr
    before = bgr_buffer(H, W, pitch, seed)
    want = before.numpy().copy()
    want[:, :3 * W] = DR.draw_bgr(before.numpy()[:, :3 * W].reshape(H, W, 3), host(trails, camera), style).reshape(H, 3 * W)
    assert (want != before.numpy()).any() == drawn and (want == before.numpy()).any()
    dev, state = before.cuda(), frozen(trails)
    image = dev[:, :3 * W].unflatten(1, (W, 3))
    assert draw_trails_bgr(image, trails, camera=camera, style=style) is image
    same(dev, want, f'bgr {W} x {H}')
    unchanged(trails, state)
    return dev.cpu(), before


BENT = [(5, 5), (20, 12), (34, 30), (50, 33), (60, 20)]           # crosses the tile corner (32, 32) of a 70 x 40 picture


def bent(frame=20, L=8, **kw):
    return DR.state_from([dict(slot=0, id=5, points=BENT, pos=(64, 10), **kw),
                          dict(slot=2, id=38, points=[(10, 35), (30, 20), (55, 6)], last=frame - 4,
                               when=[frame - 12, frame - 8, frame - 4]),
                          dict(slot=3, id=7, points=[(200, 200), (300, 220), (400, 90)])], S=4, L=L, frame=frame)


@pytest.mark.parametrize('H, W, pitch', [(1, 1, 5), (17, 33, 100), (40, 70, 240)])
def test_bgr_small_and_ragged_sizes(H, W, pitch):
    """A trail that starts on pixel (0, 0) and crosses the tile corners at 32; another wholly off the surface."""
    st = DR.state_from([dict(slot=0, id=5, points=[(0, 0), (20, 12), (34, 30), (50, 33), (60, 20)]),
                        dict(slot=1, id=9, points=[(200, 200), (300, 220)])], S=2, L=8, frame=9)
    trails = loaded([st], 8)
    for s in (style(), style(thickness=6, thickness_tail=2, head_radius=5)):
        got, before = check_bgr(trails, H, W, pitch, s, seed=W)
        assert torch.equal(got[:, 3 * W:], before[:, 3 * W:])


@pytest.mark.parametrize('H, W, pitch', [(2, 2, 2), (18, 34, 48), (40, 70, 80)])
def test_nv12_small_and_ragged_sizes(H, W, pitch):
    st = DR.state_from([dict(slot=0, id=5, points=[(0, 0), (20, 12), (34, 30), (50, 33), (60, 20)]),
                        dict(slot=1, id=9, points=[(200, 200), (300, 220)])], S=2, L=8, frame=9)
    trails = loaded([st], 8)
    for s in (style(thickness=1), style(thickness=6, thickness_tail=2, head_radius=5)):
        if (H, s.thickness) == (2, 6):
            continue                                             # (it covers all of a 2 x 2 surface)
        got, before = check_nv12(trails, H, W, pitch, s, seed=W)
        assert torch.equal(got[:, W:], before[:, W:])


def test_a_trail_wholly_off_the_surface_draws_nothing():
    st = DR.state_from([dict(slot=1, id=9, points=[(200, 200), (300, 220), (400, 90)])], S=2, L=8, frame=9)
    trails = loaded([st], 8)
    got, before = check_bgr(trails, 40, 70, 240, style(thickness=32, thickness_tail=32, head_radius=32), drawn=False)
    assert torch.equal(got, before)
    got, before = check_nv12(trails, 40, 70, 80, style(), drawn=False)
    assert torch.equal(got, before)


def test_state_filled_by_real_updates():
    """Two walkers through TrackTrails.update on the device, one with a gap; then both kinds of surface."""
    from pavenet_amd import TrackTrails
    trails = TrackTrails(1, anchor_kpts=(0,), length=6, max_tracks=4, min_step=8)
    for f in range(10):
        xy = [(4 + 6 * f, 6 + 3 * f), (66 - 5 * f, 30 - 2 * (f % 3))] if f not in (4, 5) else [(4 + 6 * f, 6 + 3 * f)]
        kp, bb = pts(*xy)
        ids = torch.tensor([3, 12][:len(xy)], dtype=torch.int32, device='cuda')
        trails.update((torch.from_numpy(bb).cuda(), None, torch.from_numpy(kp).cuda()), ids)
    assert trails.state(0)['count'][:2].tolist() == [6, 6] and int(trails.state(0)['frame']) == 10
    for s in (style(), style(head_radius=4, tail_frames=3), style(linger=0)):
        check_bgr(trails, 40, 70, 240, s)
        check_nv12(trails, 40, 70, 80, s)


@pytest.mark.parametrize('L', [5, 8])
def test_hostile_head_and_count_draw_what_the_reduced_values_give(L):
    """head negative and >= L, count <= 0 and > L, written straight into the state (the box is left to cover every
    point of the ring, as the rings are full): the picture is the one of (unsigned)head % L and count clamped to 1 ..
    L, which the oracle states; L = 5 is where the unsigned and the signed remainder of a negative head differ."""
    ring = [(6 + 11 * j, 8 + (7 * j) % 27) for j in range(L)]
    st = DR.state_from([dict(slot=t, id=4 + t, points=[(x, y + 2 * t) for x, y in ring]) for t in range(4)], S=4, L=L, frame=30)
    st['head'][:] = [-1, L + 3, -2 ** 31, 2 ** 31 - 1]
    st['count'][:] = [L + 1, -5, 0, 2 ** 31 - 1]
    trails = loaded([st], L)
    assert trails.state(0)['head'].tolist() == st['head'].tolist()
    for s in (style(), style(head_radius=3, thickness=5)):
        check_bgr(trails, 40, 70, 240, s)
        check_nv12(trails, 40, 70, 80, s)


def test_two_trails_cross_and_the_larger_id_is_on_top():
    """ids 5 and 37 share palette row 4; 38 has row 5.  Whatever the slot order, the larger id is on top."""
    a, b, c = [(5, 20), (60, 20)], [(30, 4), (30, 36)], [(8, 6), (62, 34)]
    s = style(thickness=4, thickness_tail=2)
    pictures = []
    for slots in ((0, 1, 2), (2, 0, 1), (1, 2, 0)):
        st = DR.state_from([dict(slot=slots[0], id=5, points=a), dict(slot=slots[1], id=37, points=b),
                            dict(slot=slots[2], id=38, points=c)], S=3, L=4, frame=7)
        got, _ = check_bgr(loaded([st], 4), 40, 70, 240, s)
        check_nv12(loaded([st], 4), 40, 70, 80, s)
        pictures.append(got)
    assert torch.equal(pictures[0], pictures[1]) and torch.equal(pictures[0], pictures[2])
    image = pictures[0][:, :210].reshape(40, 70, 3)
    assert tuple(image[20, 10].tolist()) == s.palette[4] == tuple(image[6, 30].tolist())
    assert tuple(image[20, 35].tolist()) == s.palette[5]                 # (38 over 5 and 37 where all three meet)


def test_a_wrapped_ring_of_64():
    """64 committed points of a spiral, the newest at ring index 20: the walk wraps at the ring's end."""
    a = np.arange(64) * 0.21
    spiral = [(35 + (4 + 0.4 * j) * np.cos(v), 20 + (3 + 0.25 * j) * np.sin(v)) for j, v in enumerate(a)]
    st = DR.state_from([dict(slot=1, id=11, points=spiral, head=20)], S=2, L=64, frame=100)
    trails = loaded([st], 64)
    assert int(trails.state(0)['head'][1]) == 20 and int(trails.state(0)['count'][1]) == 64
    for s in (style(thickness=2), style(thickness=3, tail_frames=40, head_radius=2)):
        check_bgr(trails, 40, 70, 240, s)
        check_nv12(trails, 40, 70, 80, s)


def test_128_tracks_of_64_points_under_one_tile():
    """The worst case of the round count: 128 slots x 65 primitives on the 32 x 32 tile at the origin, 33 rounds of
    256; the surface has a second tile that nothing touches."""
    rng = np.random.default_rng(231)
    tracks = [dict(slot=t, id=1000 - 7 * t, points=[tuple(p) for p in rng.uniform(1, 30, (64, 2))], head=int(rng.integers(64)))
              for t in range(128)]
    st = DR.state_from(tracks, S=128, L=64, frame=500)
    trails = loaded([st], 64)
    s = style(thickness=1, head_radius=1)
    got, before = check_bgr(trails, 34, 66, 200, s)
    assert torch.equal(got[:, 3 * 36:], before[:, 3 * 36:])
    check_nv12(trails, 34, 66, 66, s)


def test_tail_frames_linger_and_head_radius_on_and_off():
    trails = loaded([bent()], 8)
    seen = {}
    for name, kw in (('plain', {}), ('tail', dict(tail_frames=2)), ('linger', dict(linger=0)), ('head', dict(head_radius=6)),
                     ('all', dict(tail_frames=2, linger=0, head_radius=6))):
        seen[name], before = check_bgr(trails, 40, 70, 240, style(**kw))
        check_nv12(trails, 40, 70, 80, style(**kw))
    changed = {k: int((v != before).sum()) for k, v in seen.items()}
    assert changed['tail'] < changed['plain'] and changed['linger'] < changed['plain'] < changed['head']
    assert len({v.numpy().tobytes() for v in seen.values()}) == 5


def test_both_matrices_and_both_ranges_in_one_launch():
    from pavenet_amd import draw_trails_nv12
    trails = loaded([bent()], 8)
    s = style(head_radius=3)
    modes = [('bt601', False), ('bt709', True), ('bt709', False), ('bt601', True)]
    before = [nv12_surface(40, 70, 80, seed=i) for i in range(4)]
    wants = [DR.draw_nv12(b.numpy(), 70, host(trails, 0), s, m, f) for b, (m, f) in zip(before, modes)]
    assert all((w != b.numpy()).any() and (w == b.numpy()).any() for w, b in zip(wants, before))
    assert (wants[0] != DR.draw_nv12(before[0].numpy(), 70, host(trails, 0), s, 'bt709', True)).any()
    dev, state = [b.cuda() for b in before], frozen(trails)
    assert draw_trails_nv12(dev, 70, trails, style=s, matrix=[m for m, _ in modes], full_range=[f for _, f in modes]) is dev
    for i, (d, w) in enumerate(zip(dev, wants)):
        same(d, w, f'surface {i}')
    unchanged(trails, state)


def test_33_surfaces_of_two_cameras_in_two_launches():
    from pavenet_amd import draw_trails_bgr, draw_trails_nv12
    other = DR.state_from([dict(slot=1, id=21, points=[(2, 2), (12, 9), (30, 4), (38, 14)])], S=4, L=8, frame=3)
    trails = loaded([bent(), other], 8)
    s = style(head_radius=2)
    sizes = [((2 + 2 * (i % 5)) * 4, (1 + i % 4) * 8) for i in range(33)]        # (W, H), all even
    cams = [i % 2 for i in range(33)]
    before = [nv12_surface(H, W, W + 2 * (i % 3), seed=i) for i, (W, H) in enumerate(sizes)]
    wants = [DR.draw_nv12(b.numpy(), W, host(trails, c), s) for b, (W, H), c in zip(before, sizes, cams)]
    assert all((w != b.numpy()).any() and (w == b.numpy()).any() for w, b in zip(wants, before))
    dev, state = [b.cuda() for b in before], frozen(trails)
    draw_trails_nv12(dev, [W for W, _ in sizes], trails, camera=cams, style=s)
    for i, (b, d, w, (W, H), c) in enumerate(zip(before, dev, wants, sizes, cams)):
        same(d, w, f'surface {i}')
        one = b.cuda()
        draw_trails_nv12(one, W, trails, camera=c, style=s)
        assert torch.equal(one, d)
    before = [torch.from_numpy(np.random.default_rng(i).integers(0, 256, (H, W, 3), dtype=np.uint8)) for i, (W, H) in enumerate(sizes)]
    wants = [DR.draw_bgr(b.numpy(), host(trails, c), s) for b, c in zip(before, cams)]
    assert all((w != b.numpy()).any() and (w == b.numpy()).any() for w, b in zip(wants, before))
    dev = [b.cuda() for b in before]
    draw_trails_bgr(dev, trails, camera=cams, style=s)
    for i, (d, w) in enumerate(zip(dev, wants)):
        same(d, w, f'image {i}')
    unchanged(trails, state)


def test_trails_without_state_leave_the_surface_untouched():
    from pavenet_amd import TrackTrails, draw_trails_bgr, draw_trails_nv12
    empty = TrackTrails(15)
    nv, bgr = nv12_surface(64, 96, 128).cuda(), bgr_buffer(50, 70, 210).cuda().view(50, 70, 3)
    keep = nv.clone(), bgr.clone()
    assert draw_trails_nv12(nv, 96, empty) is nv and draw_trails_bgr(bgr, empty) is bgr and empty._state is None
    assert torch.equal(nv, keep[0]) and torch.equal(bgr, keep[1])
    # and with state but no live slot
    trails = loaded([DR.state_from([], S=4, L=8, frame=0)], 8)
    assert draw_trails_nv12(nv, 96, trails) is nv and torch.equal(nv, keep[0])


def test_no_allocation_in_100_calls():
    from pavenet_amd import draw_trails_bgr, draw_trails_nv12
    trails = loaded([bent()], 8)
    s = style()
    nv, bgr = nv12_surface(64, 96, 128).cuda(), bgr_buffer(50, 70, 210).cuda().view(50, 70, 3)
    draw_trails_nv12(nv, 96, trails, style=s)
    draw_trails_bgr(bgr, trails, style=s)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    for _ in range(100):
        draw_trails_nv12(nv, 96, trails, style=s)
        draw_trails_bgr(bgr, trails, style=s)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() == base == torch.cuda.memory_allocated()
