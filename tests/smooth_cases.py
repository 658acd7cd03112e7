"""Scenarios for the smoothing rule of DESIGN section 16 that the CPU and the GPU tests share: the arithmetic edges of
the rule as small scripts with values worked out by hand.  A script drives a harness `make(K, **arguments)` with
  h.frame(kpts, bboxes, ids, keep=None) -> (out_kpts, out_bboxes) as numpy float32
  h.poke(field, index, value)               a write into camera 0's state
  h.get(field)                              camera 0's state tensor as numpy
The CPU harness is the oracle alone; the GPU harness runs the device beside it and compares everything after every
frame, so the hand-worked values below hold for both.

Coordinates are quarter pixels at scale 1, so a pixel coordinate q / 4 is exact in fp32; a state position is 16 q."""
import numpy as np

NAN_BITS = 0x7fc00000


def det(points, box, score=0.9, box_score=0.8):
    """points: K (X, Y) quarter-pixel pairs; box: (X1, Y1, X2, Y2) quarter pixels -> kpts [1, K, 3], bboxes [1, 5]."""
    kp = np.asarray([[(x / 4.0, y / 4.0, score) for x, y in points]], np.float32)
    bb = np.asarray([[v / 4.0 for v in box] + [box_score]], np.float32)
    return kp, bb


def stack(*dets):
    return np.concatenate([d[0] for d in dets]), np.concatenate([d[1] for d in dets])


def empty(K):
    return np.zeros((0, K, 3), np.float32), np.zeros((0, 5), np.float32), np.zeros(0, np.int32)


def q64(out):
    """Output coordinates -> the integers they are 1/64 of."""
    v = np.asarray(out, np.float64) * 64
    assert (v == np.rint(v)).all()
    return v.astype(np.int64)


BOX100 = (0, 0, 100, 100)     # s = 100


def _one_step(make, pos, vel, Z, gaps=1, box=BOX100, **kw):
    """K = 1: id 7 is born, its key point's state is overwritten with pos / vel, `gaps` - 1 frames pass without it,
    then it is detected at Z (quarter pixels * 16 given as state units, multiples of 16) -> (h, out_kpts)."""
    h = make(1, **kw)
    h.frame(*det([(Z[0] // 16, Z[1] // 16)], box), [7])
    h.poke('pos', (0, 0), pos)
    h.poke('vel', (0, 0), vel)
    for _ in range(gaps - 1):
        h.frame(*empty(1))
    out, _ = h.frame(*det([(Z[0] // 16, Z[1] // 16)], box), [7])
    return h, out


def negative_odd_error(make):
    """e = (-11, 8), gap 1: r = e; vel = (-33 + 8) >> 4 = -2 (C's / gives -1), (24 + 8) >> 4 = 2; speed 4, s = 100:
    u = 256 / 100 = 2, alpha = 32 + (256 >> 4) = 48; pos x += (-528 + 128) >> 8 = -2 (truncation: -1), pos y +=
    512 >> 8 = 2."""
    h, out = _one_step(make, (1003, 1000), (0, 0), (992, 1008))
    assert h.get('vel')[0, 0].tolist() == [-2, 2]
    assert h.get('pos')[0, 0].tolist() == [1001, 1002]
    assert q64(out[0, 0, :2]).tolist() == [1001, 1002]
    assert h.get('last')[0] == 2 and h.get('frame') == 2


def gap_division_and_negative_velocity(make):
    """gap 3, e = (-11, 8): r = floor(-19 / 6) = -4 (C: -3), floor(19 / 6) = 3; vel (-7, 5) -> (-12 - 91 + 8) >> 4
    = -95 >> 4 = -6 (C: -5), (9 + 65 + 8) >> 4 = 5; speed 11: u = 704 / 100 = 7, alpha = 32 + (896 >> 4) = 88; pos x
    += (-968 + 128) >> 8 = -4, pos y += 832 >> 8 = 3."""
    h, out = _one_step(make, (1003, 1000), (-7, 5), (992, 1008), gaps=3)
    assert h.get('vel')[0, 0].tolist() == [-6, 5]
    assert h.get('pos')[0, 0].tolist() == [999, 1003]
    assert q64(out[0, 0, :2]).tolist() == [999, 1003]
    assert h.get('last')[0] == 4


def alpha_at_256_and_below(make):
    """velocity_gain 16: vel = r = e = (280, 0); s = 640: u = 280 * 64 / 640 = 28; alpha_min 32: alpha = 32 + 224 =
    256 exactly and pos = Z; alpha_min 31: alpha = 255 and pos x += (71400 + 128) >> 8 = 279, one short of Z;
    alpha_min 40: 264 is cut to 256."""
    for alpha_min, px in ((32, 1600), (31, 1599), (40, 1600)):
        h, out = _one_step(make, (1320, 1600), (0, 0), (1600, 1600), box=(0, 0, 640, 10), velocity_gain=16,
                           alpha_min=alpha_min)
        assert h.get('vel')[0, 0].tolist() == [280, 0]
        assert h.get('pos')[0, 0].tolist() == [px, 1600], alpha_min
        assert q64(out[0, 0, :2]).tolist() == [px, 1600]


def size_one(make):
    """A box of no extent has s = 1: vel = (16, 0), u = 16 * 64 = 1024, beta 1: alpha = 32 + (1024 >> 4) = 96, pos x
    += (1536 + 128) >> 8 = 6."""
    h, out = _one_step(make, (1584, 1600), (0, 0), (1600, 1600), box=(5, 5, 5, 5), velocity_gain=16, beta=1)
    assert h.get('vel')[0, 0].tolist() == [16, 0]
    assert h.get('pos')[0, 0].tolist() == [1590, 1600]
    assert q64(out[0, 0, :2]).tolist() == [1590, 1600]


def beta_zero(make):
    """beta 0 is a fixed exponential filter, however fast the point is: alpha_min 64, e = 400: pos += 25728 >> 8 =
    100; then e = 300: pos += 19328 >> 8 = 75.  The velocity is still kept: 1208 >> 4 = 75, (900 + 975 + 8) >> 4 =
    117."""
    h, out = _one_step(make, (1200, 1600), (0, 0), (1600, 1600), beta=0, alpha_min=64)
    assert h.get('pos')[0, 0].tolist() == [1300, 1600] and h.get('vel')[0, 0].tolist() == [75, 0]
    out, _ = h.frame(*det([(100, 100)], BOX100), [7])
    assert h.get('pos')[0, 0].tolist() == [1375, 1600] and h.get('vel')[0, 0].tolist() == [117, 0]
    assert q64(out[0, 0, :2]).tolist() == [1375, 1600]


def alpha_min_256_is_the_pass_through(make):
    """alpha = 256 at every point: every output is the quantised detection, 16 X / 64 = X / 4."""
    rng = np.random.default_rng(5)
    h = make(3, alpha_min=256)
    for f in range(6):
        kp = rng.uniform(0, 500, (4, 3, 3)).astype(np.float32)
        bb = rng.uniform(0, 500, (4, 5)).astype(np.float32)
        kp[..., 2], bb[:, 4] = 0.9, 0.8
        out_k, out_b = h.frame(kp, bb, [3, 1, 0, 2])
        with np.errstate(all='ignore'):
            assert (out_k[..., :2] == np.rint(kp[..., :2] * np.float32(4)) / np.float32(4)).all()
            assert (out_b[:, :4] == np.rint(bb[:, :4] * np.float32(4)) / np.float32(4)).all()
        assert (out_k[..., 2] == kp[..., 2]).all() and (out_b[:, 4] == bb[:, 4]).all()
    assert sorted(h.get('id')[:4].tolist()) == [0, 1, 2, 3]


def invisible_point(make):
    """K = 2, kpt_thr 0: a score of 0 is not visible.  The point's pos x becomes -1 and nothing else of it changes,
    its output is the detection; seen again it starts at the detection with vel 0, whatever it held before."""
    h = make(2, velocity_gain=16)
    h.frame(*det([(100, 100), (200, 200)], BOX100), [4])
    h.frame(*det([(110, 100), (210, 200)], BOX100), [4])
    assert h.get('vel')[0, 1].tolist() == [160, 0]
    pos_y = int(h.get('pos')[0, 1, 1])
    kp, bb = det([(110, 100), (300, 300)], BOX100)
    kp[0, 1, 2] = 0.0
    out, _ = h.frame(kp, bb, [4])
    assert h.get('pos')[0, 1].tolist() == [-1, pos_y] and h.get('vel')[0, 1].tolist() == [160, 0]
    assert q64(out[0, 1, :2]).tolist() == [4800, 4800] and out[0, 1, 2] == 0.0
    out, _ = h.frame(*det([(110, 100), (400, 404)], BOX100), [4])
    assert h.get('pos')[0, 1].tolist() == [6400, 6464] and h.get('vel')[0, 1].tolist() == [0, 0]
    assert q64(out[0, 1, :2]).tolist() == [6400, 6464]
    # born invisible: only pos x is written
    h = make(2)
    h.poke('pos', (0, 1), (55, 66))
    h.poke('vel', (0, 1), (77, 88))
    kp, bb = det([(110, 100), (300, 300)], BOX100)
    kp[0, 1, 2] = -1.0
    h.frame(kp, bb, [9])
    assert h.get('pos')[0, 1].tolist() == [-1, 66] and h.get('vel')[0, 1].tolist() == [77, 88]
    assert h.get('id')[0] == 9


def duplicate_and_unusable_ids(make):
    """Of two valid poses with one id the first is filtered and the second passes through; a pose that is not valid
    does not count as the first; ids <= 0 pass through and take no slot."""
    h = make(1, alpha_min=128, beta=0)
    a, b = det([(100, 100)], BOX100), det([(300, 300)], BOX100)
    h.frame(*stack(a, b), [7, 7])
    assert h.get('id')[:2].tolist() == [7, 0] and h.get('pos')[0, 0].tolist() == [1600, 1600]
    a2, b2 = det([(132, 100)], BOX100), det([(332, 300)], BOX100)
    out, _ = h.frame(*stack(b2, a2), [7, 7])          # the first of the frame is b2 now: e = 5312 - 1600
    assert q64(out[:, 0, 0]).tolist() == [1600 + ((128 * 3712 + 128) >> 8), 2112]
    out, _ = h.frame(*stack(a, b, a), [7, 7, 5], keep=[0, 1, 1])
    assert h.get('id')[:3].tolist() == [7, 5, 0]
    assert q64(out[0, 0, :2]).tolist() == [1600, 1600]        # not kept: passes through
    assert q64(out[1, 0, 0]) != 4800                          # filtered towards b
    h = make(1)
    out, _ = h.frame(*stack(a, b, a), [0, -3, -(2 ** 31)])
    assert not h.get('id').any() and h.get('dropped') == 0 and h.get('frame') == 1
    assert q64(out[:, 0, 0]).tolist() == [1600, 4800, 1600]


def expiry(make):
    """frame - last == max_age keeps the slot, max_age + 1 frees it: the id is born again, at the detection (with
    max_age 0 on every frame).  A kept point moves by (128 * 512 + 128) >> 8 = 256 whatever the gap."""
    for max_age, idle, kept in ((2, 1, True), (2, 2, False), (1, 0, True), (1, 1, False), (0, 0, False)):
        h = make(1, max_age=max_age, alpha_min=128, beta=0)
        h.frame(*det([(100, 100)], BOX100), [3])
        for _ in range(idle):
            h.frame(*empty(1))
        out, _ = h.frame(*det([(132, 100)], BOX100), [3])
        assert h.get('id')[0] == 3 and h.get('last')[0] == idle + 2
        assert q64(out[0, 0, 0]) == (1600 + 256 if kept else 2112), (max_age, idle)
        assert h.get('vel')[0, 0, 0] == ((3 * ((2 * 512 + idle + 1) // (2 * (idle + 1))) + 8) >> 4 if kept else 0)


def two_slots(make):
    """S = 2: a third id is dropped and passes through; an expired slot is taken again, the lowest first."""
    h = make(1, max_tracks=2, max_age=1, alpha_min=128, beta=0)
    a, b, c = det([(100, 100)], BOX100), det([(300, 300)], BOX100), det([(500, 500)], BOX100)
    h.frame(*stack(a, b, c), [11, 12, 13])
    assert h.get('id').tolist() == [11, 12] and h.get('dropped') == 1
    c2 = det([(532, 500)], BOX100)
    out, _ = h.frame(*stack(c2, b), [13, 12])        # 11 is away but not yet expired: 13 finds no slot
    assert h.get('id').tolist() == [11, 12] and h.get('dropped') == 2
    assert q64(out[0, 0, 0]) == 8512
    out, _ = h.frame(*stack(c2, b), [13, 12])        # slot 0 is free now
    assert h.get('id').tolist() == [13, 12] and h.get('dropped') == 2 and h.get('last').tolist() == [3, 3]
    h.frame(*empty(1))
    h.frame(*empty(1))
    h.frame(*stack(b, a), [12, 11])                  # both expired: born in ascending pose index
    assert h.get('id').tolist() == [12, 11] and h.get('pos')[:, 0, 0].tolist() == [4800, 1600]


def garbage_is_never_read(make):
    """Whatever free slots and uninitialised points hold, the outputs and the live state are the same."""
    results = []
    for garbage in (False, True):
        h = make(2, max_tracks=3)
        kp, bb = det([(100, 100), (200, 200)], BOX100)
        kp[0, 1, 2] = 0.0
        if garbage:
            for t in range(3):
                h.poke('pos', (t,), np.full((4, 2), -2 ** 31, np.int64))
                h.poke('vel', (t,), np.full((4, 2), 2 ** 31 - 1, np.int64))
                h.poke('last', (t,), -2 ** 31)
        h.frame(kp, bb, [2 ** 31 - 1])
        if garbage:
            h.poke('pos', (0, 1, 1), 2 ** 31 - 1)          # the y of an uninitialised point
            h.poke('vel', (0, 1), (-2 ** 31, 2 ** 31 - 1))
        outs = [h.frame(*det([(104, 100), (204, 200)], BOX100), [2 ** 31 - 1]),
                h.frame(*det([(108, 100), (208, 200)], BOX100), [2 ** 31 - 1])]
        results.append((outs, h.get('pos')[0].copy(), h.get('vel')[0].copy(), h.get('id').copy()))
    for (ok, ob), (gk, gb) in zip(results[0][0], results[1][0]):
        assert ok.tobytes() == gk.tobytes() and ob.tobytes() == gb.tobytes()
    assert all((a == b).all() for a, b in zip(results[0][1:], results[1][1:]))
    assert results[0][3].tolist() == [2 ** 31 - 1, 0, 0]


def unusable_pose(make):
    """A coordinate that is not finite makes every coordinate of the pose the quiet NaN 0x7fc00000; its scores, a
    NaN with a payload among them, are copied bit for bit.  It takes no slot."""
    h = make(2)
    for where in ('kpt', 'box'):
        kp, bb = stack(det([(100, 100), (200, 200)], BOX100), det([(300, 300), (400, 400)], BOX100))
        if where == 'kpt':
            kp[1, 1, 1] = np.inf
        else:
            bb[1, 2] = np.nan
        kp[1, 0, 2:3].view(np.uint32)[:] = 0x7fc12345
        bb[1, 4:5].view(np.uint32)[:] = 0xffc00001
        out_k, out_b = h.frame(kp, bb, [1, 2])
        assert (out_k[1, :, :2].view(np.uint32) == NAN_BITS).all() and (out_b[1, :4].view(np.uint32) == NAN_BITS).all()
        assert out_k[1, :, 2].view(np.uint32).tolist() == [0x7fc12345, kp[1, 1, 2:3].view(np.uint32)[0]]
        assert out_b[1, 4:5].view(np.uint32)[0] == 0xffc00001
        assert q64(out_k[0, :, :2]).tolist() == [[1600, 1600], [3200, 3200]]
        assert h.get('id')[:2].tolist() == [1, 0]


def score_at_the_threshold(make):
    """bboxes[:, 4] > score_thr: a score equal to the threshold passes through and takes no slot."""
    h = make(1, score_thr=0.3)
    thr = float(np.float32(0.3))
    h.frame(*det([(100, 100)], BOX100, box_score=thr), [5])
    assert not h.get('id').any()
    above = float(np.nextafter(np.float32(0.3), np.float32(1)))
    h.frame(*det([(100, 100)], BOX100, box_score=above), [5])
    assert h.get('id')[0] == 5
    # the same for a key point's score and kpt_thr
    h = make(1, kpt_thr=0.5)
    h.frame(*det([(100, 100)], BOX100, score=0.5), [5])
    assert h.get('pos')[0, 0, 0] == -1 and h.get('pos')[0, 1].tolist() == [0, 0]
    h.frame(*det([(100, 100)], BOX100, score=float(np.nextafter(np.float32(0.5), np.float32(1)))), [5])
    assert h.get('pos')[0, 0].tolist() == [1600, 1600]


SCRIPTS = [negative_odd_error, gap_division_and_negative_velocity, alpha_at_256_and_below, size_one, beta_zero,
           alpha_min_256_is_the_pass_through, invisible_point, duplicate_and_unusable_ids, expiry, two_slots,
           garbage_is_never_read, unusable_pose, score_at_the_threshold]
