"""The trail draw rule of DESIGN section 22 on its numpy statement alone (tests/trail_draw_ref.py): properties the rule
must have whatever draws it.  No GPU."""
import numpy as np
import pytest

from tests import trail_draw_ref as DR


def style(**kw):
    from pavenet_amd.trails import TrailStyle
    return TrailStyle(**kw)


def picture(H=40, W=70, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def surface(H=40, W=70, pitch=80, seed=0):
    s = np.full((H * 3 // 2, pitch), 0xA5, np.uint8)
    s[:, :W] = np.random.default_rng(seed).integers(0, 256, (H * 3 // 2, W), dtype=np.uint8)
    return s


def two_tracks(frame=20):
    """A bent trail of five points and a straight one of three that crosses it; the second was last seen 4 frames ago."""
    return DR.state_from([dict(slot=0, id=5, points=[(5, 5), (20, 12), (34, 30), (50, 33), (60, 20)], pos=(64, 10)),
                          dict(slot=3, id=38, points=[(10, 35), (30, 20), (55, 6)], last=frame - 4,
                               when=[frame - 12, frame - 8, frame - 4])], S=4, L=8, frame=frame)


def test_drawing_twice_is_drawing_once():
    st, s = two_tracks(), style(head_radius=3)
    once = DR.draw_bgr(picture(), st, s)
    assert (once != picture()).any() and (once == picture()).any()
    assert (DR.draw_bgr(once, st, s) == once).all()
    nv = DR.draw_nv12(surface(), 70, st, s)
    assert (nv != surface()).any() and (nv[:, 70:] == 0xA5).all()
    assert (DR.draw_nv12(nv, 70, st, s) == nv).all()


@pytest.mark.parametrize('kw', [dict(tail_frames=1), dict(tail_frames=3), dict(tail_frames=9), dict(linger=0), dict(linger=3),
                                dict(linger=4), dict(tail_frames=5, linger=0)])
def test_tail_frames_and_linger_only_remove_pixels(kw):
    """A pixel drawn with a limit is drawn without it; where both draw, a removed primitive may show the one below."""
    st, before = two_tracks(), picture()
    full, part = DR.draw_bgr(before, st, style()), DR.draw_bgr(before, st, style(**kw))
    drawn_full, drawn_part = (full != before).any(-1), (part != before).any(-1)
    assert not (drawn_part & ~drawn_full).any()
    if kw.get('linger') == 4 and 'tail_frames' not in kw:
        assert (part == full).all()                                   # (frame - last = 4 <= 4: both slots are drawn)
    else:
        assert drawn_part.sum() < drawn_full.sum()
    keys_full = DR.key_map(70, 40, DR.primitives(st, style()))[0]
    keys_part = DR.key_map(70, 40, DR.primitives(st, style(**kw)))[0]
    assert (keys_part <= keys_full).all() and set(np.unique(keys_part)) <= set(np.unique(keys_full))


@pytest.mark.parametrize('T', [1, 3, 8])
def test_a_one_point_trail_is_a_disc_of_radius_2T(T):
    """count 1, pos on the point, head_radius 0: the one capsule has both ends on the point and radius 2 T quarter
    pixels: pixel (x, y) is drawn iff (4 x - X)^2 + (4 y - Y)^2 <= 4 T^2."""
    st = DR.state_from([dict(slot=1, id=9, points=[(20.25, 17.25)])], S=2, L=4, frame=3)
    keys, _ = DR.key_map(70, 40, DR.primitives(st, style(thickness=T, thickness_tail=1)))
    yy, xx = np.mgrid[0:40, 0:70]
    disc = (4 * xx - 81) ** 2 + (4 * yy - 69) ** 2 <= (2 * T) ** 2
    assert ((keys != DR.NONE) == disc).all() and disc.any() and (keys[disc] == 9 * 128).all()


def test_taper_radii():
    assert DR.radii(1, 3, 1) == [6] and DR.radii(2, 3, 1) == [4, 6] and DR.radii(1, 1, 1) == [2]
    r = DR.radii(64, 32, 1)
    assert r[0] == 2 and r[-1] == 64 and r == sorted(r) and len(r) == 64 and r[31] == 2 + 31
    assert DR.radii(64, 3, 1) == [2 + (j + 1) // 16 for j in range(64)]
    assert DR.radii(5, 4, 4) == [8] * 5 and DR.radii(3, 32, 32) == [64] * 3


def test_the_larger_key_is_on_top_whatever_the_slot_order():
    """Two trails that cross, ids 5 and 38 (palette rows 4 and 5): the crossing takes the larger id's colour in either
    slot order, and within a trail the newer segment covers the older one's end."""
    a = dict(id=5, points=[(5, 20), (60, 20)])
    b = dict(id=38, points=[(30, 4), (30, 36)])
    s = style(thickness=4, thickness_tail=4)
    one = DR.draw_bgr(picture(), DR.state_from([dict(slot=0, **a), dict(slot=1, **b)], 2, 4, 7), s)
    two = DR.draw_bgr(picture(), DR.state_from([dict(slot=1, **a), dict(slot=0, **b)], 2, 4, 7), s)
    assert (one == two).all() and tuple(one[20, 30]) == s.palette[5] and tuple(one[20, 10]) == s.palette[4]
    keys, _ = DR.key_map(70, 40, DR.primitives(DR.state_from([dict(slot=0, id=2, points=[(5, 5), (30, 5), (30, 30)])], 1, 4, 7), s))
    assert keys[5, 10] == 2 * 128 and keys[5, 30] == 2 * 128 + 1 and keys[20, 30] == 2 * 128 + 1        # the corner: j = 1
    assert keys[30, 30] == 2 * 128 + 2                                  # pos lies on the newest point: capsule 2 is a disc


def test_hostile_head_and_count_are_reduced():
    """head and count outside their ranges draw what (unsigned)head % L and count clamped to 1 .. L give."""
    st = two_tracks()
    ok = DR.draw_bgr(picture(), st, style())
    st['head'][0] += 8 * 5                        # L = 8
    assert (DR.draw_bgr(picture(), st, style()) == ok).all()
    st['head'][0] -= 8 * 6                        # negative: (head + 2^32) % 8 is still the head it was
    assert st['head'][0] < 0 and (DR.draw_bgr(picture(), st, style()) == ok).all()
    assert DR.committed(np.zeros((5, 2), np.int32), np.arange(5), -1, 1) == [(0, 0, 0)]      # (2^32 - 1) % 5 = 0, not 4
    low, high = {k: v.copy() for k, v in st.items()}, {k: v.copy() for k, v in st.items()}
    low['count'][3], high['count'][3] = -7, 1000
    one, all8 = {k: v.copy() for k, v in st.items()}, {k: v.copy() for k, v in st.items()}
    one['count'][3], all8['count'][3] = 1, 8
    assert (DR.draw_bgr(picture(), low, style()) == DR.draw_bgr(picture(), one, style())).all()
    assert (DR.draw_bgr(picture(), high, style()) == DR.draw_bgr(picture(), all8, style())).all()
