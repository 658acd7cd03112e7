"""Scenarios for the motion model of DESIGN section 14 that the CPU and the GPU tests share: walking people with one
withheld, two people who walk through each other, and the arithmetic edges of the rule as small scripts of frames,
writes into the state ("poke") and expected values ("check")."""
import math

import numpy as np

from tests.test_track_cpu import FIGURE, walk


def walk_with_gap(height, step, hidden=(), frames=40):
    """tests.test_track_cpu.walk with person 0 withheld on the 0-based frames `hidden` (their jitter is still
    drawn).  Yields (kpts, bboxes, who)."""
    for f, (kpts, bboxes, who) in enumerate(walk(height, step, frames=frames, people=6, seed=height * 10 + step)):
        if f in hidden:
            there = who != 0
            kpts, bboxes, who = kpts[there], bboxes[there], who[there]
        yield kpts, bboxes, who


def crossing(height, step, frames=60):
    """Two figures on one row that start step * 59 px apart and walk towards and through each other, `step` px per
    frame each, jitter 1 % of the height, shuffled on every frame.  Yields (kpts, bboxes, who)."""
    rng = np.random.default_rng(1)
    for f in range(frames):
        kpts = np.empty((2, 15, 3), np.float32)
        for p, x in enumerate((100.0 + step * f, 100.0 + step * 59 - step * f)):
            xy = FIGURE * height + (x, 50.0)
            kpts[p, :, :2] = xy + rng.uniform(-0.01, 0.01, xy.shape) * height
            kpts[p, :, 2] = 0.9
        who = rng.permutation(2)
        kpts = kpts[who]
        bboxes = np.concatenate([kpts[..., 0].min(1, keepdims=True), kpts[..., 1].min(1, keepdims=True),
                                 kpts[..., 0].max(1, keepdims=True), kpts[..., 1].max(1, keepdims=True),
                                 np.full((2, 1), 0.8, np.float32)], 1).astype(np.float32)
        yield kpts, bboxes, who


def ids_by_person(frames, update, people):
    """Runs `update(kpts, bboxes)` over frames of (kpts, bboxes, who) -> [frames, people] ids, -1 where absent."""
    seen = []
    for kpts, bboxes, who in frames:
        row = np.full(people, -1, np.int64)
        row[who] = update(kpts, bboxes)
        seen.append(row)
    return np.stack(seen)


def constant_ids(seen):
    """Every person has one id, not 0, on all the frames they are present."""
    return all(len(set(col[col >= 0].tolist())) == 1 and col[col >= 0][0] > 0 for col in seen.T)


# ---- the arithmetic edges: quarter pixels at scale 1, so a pixel coordinate q / 4 is exact in fp32 ----
def _det(points, box):
    """points: K (X, Y) quarter-pixel pairs; box: (X1, Y1, X2, Y2) quarter pixels -> kpts [1, K, 3], bboxes [1, 5]."""
    kp = np.asarray([[(x / 4.0, y / 4.0, 0.9) for x, y in points]], np.float32)
    bb = np.asarray([[v / 4.0 for v in box] + [0.8]], np.float32)
    return kp, bb


def _empty(K):
    return np.zeros((0, K, 3), np.float32), np.zeros((0, 5), np.float32)


TIGHT = dict(sigmas=[0.5], match_thr=math.exp(-1.0), min_kpts=1)    # K = 1, C = 2^20: agrees iff d2 <= G (area sum)
WIDE2 = dict(sigmas=[0.5, 0.5], min_kpts=1)                        # K = 2, C = 726817
HUGE = dict(sigmas=[1.9], match_thr=math.exp(-1.0), min_kpts=1)     # K = 1, C = 15141437 < 2^24
BOX8, BOX9 = (0, 0, 2, 4), (0, 0, 3, 3)                            # areas 8 and 9
BIG = (0, 0, 400, 400)


def edge_scripts():
    """name -> (K, tracker arguments, steps).  A step is ('frame', kpts, bboxes, ids expected), ('poke', slot,
    {field: value}) or ('check', slot, {field: value}); the expected values are worked out by hand from the rule."""
    out = {}
    # floor, not truncation, on a negative odd sum: S = (-3, 0), n = 2, gap = 1: m = floor(-94 / 4) = -24 (C: -23)
    # and floor(2 / 4) = 0; then hits == 2, the slot is missed for two frames and S = (-5, 3), n = 2, gap = 3:
    # m = floor(-154 / 12) = -13 (C: -12), floor(102 / 12) = 8; v = (8 m + 8 vel + 8) >> 4 = -288 >> 4 = -18, 72 >> 4 = 4
    out['negative odd S'] = (2, dict(WIDE2), [
        ('frame', *_det([(400, 400), (440, 400)], BIG), [1]),
        ('check', 0, dict(vel=(0, 0), hits=1)),
        ('frame', *_det([(399, 400), (438, 400)], BIG), [1]),
        ('check', 0, dict(vel=(-24, 0), hits=2)),
        ('frame', *_empty(2), []),
        ('frame', *_empty(2), []),
        ('frame', *_det([(396, 401), (436, 402)], BIG), [1]),
        ('check', 0, dict(vel=(-18, 4), hits=3, last=5)),
    ])
    # n = 1 of K = 2 (the second key point is not visible in the detection): S = (-1, -1): floor(-31 / 2) = -16
    kp, bb = _det([(399, 399), (0, 0)], BIG)
    kp[0, 1, 2] = 0.0
    out['one co-visible point'] = (2, dict(WIDE2, kpt_thr=0.5), [
        ('frame', *_det([(400, 400), (440, 400)], BIG), [1]),
        ('frame', kp, bb, [1]),
        ('check', 0, dict(vel=(-16, -16), hits=2, vis=1)),
    ])
    # (v g + 8) >> 4 on negative v: vel (-9, -25), g = 1: shifts -1 and -2 (C: 0 and -1).  The slot (40, 40) is
    # predicted at (39, 38); the detection (35, 37) is at d2 = 17 <= 17 from there, 29 from (40, 39), 34 from (40, 40)
    # then m = floor(-159 / 2) = -80, floor(-95 / 2) = -48; v = (-640 - 72 + 8) >> 4 = -44, (-384 - 200 + 8) >> 4 = -36
    out['negative shift'] = (1, dict(TIGHT), [
        ('frame', *_det([(40, 40)], BOX9), [1]),
        ('poke', 0, dict(vel=(-9, -25), hits=2)),
        ('frame', *_det([(35, 37)], BOX8), [1]),
        ('check', 0, dict(vel=(-44, -36), hits=3)),
    ])
    # the same detection without the floor's help: vel (-7, -23) shifts by 0 and -1: (40, 39), d2 = 29 > 17
    out['negative shift, other side'] = (1, dict(TIGHT), [
        ('frame', *_det([(40, 40)], BOX9), [1]),
        ('poke', 0, dict(vel=(-7, -23), hits=2)),
        ('frame', *_det([(35, 37)], BOX8), [2]),
        ('check', 0, dict(vel=(-7, -23), hits=2, last=1)),
        ('check', 1, dict(vel=(0, 0), hits=1, last=2)),
    ])
    # the prediction clamped at 32767 and at 0: (32000, 40) + (2048, -2048) -> (32767, 0); a detection exactly there
    # agrees under d2 <= 17, one at the unclamped place could not exist.  m = floor(24545 / 2) = 12272,
    # floor(-1279 / 2) = -640; v = (98176 + 262136 + 8) >> 4 = 22520, (-5120 - 262144 + 8) >> 4 = -16704
    out['prediction clamped'] = (1, dict(TIGHT), [
        ('frame', *_det([(32000, 40)], BOX9), [1]),
        ('poke', 0, dict(vel=(32767, -32768), hits=2)),
        ('frame', *_det([(32767, 0)], BOX8), [1]),
        ('check', 0, dict(vel=(22520, -16704), hits=3)),
    ])
    # and the other two corners
    out['prediction clamped, other corner'] = (1, dict(TIGHT), [
        ('frame', *_det([(40, 32000)], BOX9), [1]),
        ('poke', 0, dict(vel=(-32768, 32767), hits=2)),
        ('frame', *_det([(0, 32767)], BOX8), [1]),
        ('check', 0, dict(vel=(-16704, 22520), hits=3)),
    ])
    # vel saturates at both ends, by a first measurement (hits == 1: v = m = +-512000) and by the smoothed form
    # ((8 (+-512000) + 8 (+-32767) + 8) >> 4); hits saturates at 32767.  Area 2 x 32000^2, C ~ 14.44 x 2^20: every
    # d2 below 2^31 agrees.
    far = (0, 0, 32000, 32000)
    out['velocity saturates'] = (1, dict(HUGE), [
        ('frame', *_det([(40, 32000)], far), [1]),
        ('frame', *_det([(32040, 0)], far), [1]),
        ('check', 0, dict(vel=(32767, -32768), hits=2)),
        ('poke', 0, dict(hits=32766)),
        ('frame', *_det([(40, 32000)], far), [1]),
        ('check', 0, dict(vel=(-32768, 32767), hits=32767)),
        ('frame', *_det([(40, 32000)], far), [1]),
        ('check', 0, dict(vel=(-16384, 16384), hits=32767)),
        ('poke', 0, dict(vel=(32767, -32768))),
        ('frame', *_det([(32040, 0)], far), [1]),
        ('check', 0, dict(vel=(32767, -32768), hits=32767)),
    ])
    # gap > max_predict: vel (160, 0), gap = 5, max_predict = 2: the shift is (320 + 8) >> 4 = 20, not 50; the
    # velocity is measured over the whole gap: m = floor((640 + 5) / 10) = 64, v = (512 + 1280 + 8) >> 4 = 112
    gap = [('frame', *_det([(40, 40)], BOX9), [1]), ('poke', 0, dict(vel=(160, 0), hits=3))] + \
          [('frame', *_empty(1), [])] * 4
    out['gap above max_predict'] = (1, dict(TIGHT, max_predict=2), gap + [
        ('frame', *_det([(60, 40)], BOX8), [1]),
        ('check', 0, dict(vel=(112, 0), hits=4, last=6)),
    ])
    out['gap above max_predict, uncapped place'] = (1, dict(TIGHT, max_predict=2), gap + [
        ('frame', *_det([(90, 40)], BOX8), [2]),
    ])
    out['gap below max_predict'] = (1, dict(TIGHT, max_predict=5), gap + [
        ('frame', *_det([(90, 40)], BOX8), [1]),
        ('check', 0, dict(vel=(160, 0), hits=4)),
    ])
    # max_predict = 0: no shift at all
    out['max_predict 0'] = (1, dict(TIGHT, max_predict=0), gap + [
        ('frame', *_det([(40, 40)], BOX8), [1]),
        ('check', 0, dict(vel=(80, 0), hits=4)),
    ])
    # hits == 1 widens the test by new_gate = 4: d2 = 68 <= 4 x 17 agrees; then hits == 2, vel = (128, 32): the slot
    # (48, 42) is predicted at (56, 44), and d2 = 17 agrees, d2 = 20 <= 68 does not
    out['new_gate at hits 1'] = (1, dict(TIGHT, new_gate=4), [
        ('frame', *_det([(40, 40)], BOX8), [1]),
        ('frame', *_det([(48, 42)], BOX9), [1]),
        ('check', 0, dict(vel=(128, 32), hits=2)),
        ('frame', *_det([(60, 45)], BOX8), [1]),
        ('check', 0, dict(hits=3)),
    ])
    out['no new_gate at hits 2'] = (1, dict(TIGHT, new_gate=4), [
        ('frame', *_det([(40, 40)], BOX8), [1]),
        ('frame', *_det([(48, 42)], BOX9), [1]),
        ('frame', *_det([(60, 46)], BOX8), [2]),
        ('check', 0, dict(vel=(128, 32), hits=2)),
    ])
    out['new_gate is inclusive'] = (1, dict(TIGHT, new_gate=4), [
        ('frame', *_det([(40, 40)], BOX8), [1]),
        ('frame', *_det([(46, 46)], BOX9), [2]),           # d2 = 72 > 68
    ])
    out['new_gate 1'] = (1, dict(TIGHT, new_gate=1), [
        ('frame', *_det([(40, 40)], BOX8), [1]),
        ('frame', *_det([(48, 42)], BOX9), [2]),
    ])
    out['new_gate 16, gain 16'] = (1, dict(TIGHT, new_gate=16, velocity_gain=16), [
        ('frame', *_det([(40, 40)], BOX8), [1]),
        ('frame', *_det([(56, 44)], BOX9), [1]),           # d2 = 272 = 16 x 17
        ('check', 0, dict(vel=(256, 64), hits=2)),
        ('frame', *_det([(70, 48)], BOX8), [1]),           # predicted (72, 48): d2 = 4; v = m = (224, 64)
        ('check', 0, dict(vel=(224, 64), hits=3)),
    ])
    out['gain 1'] = (1, dict(TIGHT, velocity_gain=1), [
        ('frame', *_det([(40, 40)], BOX8), [1]),
        ('poke', 0, dict(vel=(-100, 100), hits=2)),
        ('frame', *_det([(36, 44)], BOX9), [1]),           # predicted (34, 46): d2 = 8; m = (-64, 64)
        ('check', 0, dict(vel=(-98, 98), hits=3)),         # (-64 - 1500 + 8) >> 4 = -98 (C: -97); (64 + 1500 + 8) >> 4
    ])
    return out


def run_script(K, steps, update, poke, peek):
    """update(kpts, bboxes) -> ids; poke(slot, field, value) writes the state; peek(slot, field) reads it."""
    for i, step in enumerate(steps):
        if step[0] == 'frame':
            got = [int(v) for v in update(step[1], step[2])]
            assert got == step[3], f'step {i}: ids {got}, expected {step[3]}'
        elif step[0] == 'poke':
            for field, value in step[2].items():
                poke(step[1], field, value)
        else:
            for field, value in step[2].items():
                got = np.asarray(peek(step[1], field)).tolist()
                assert got == (list(value) if isinstance(value, tuple) else value), \
                    f'step {i}: slot {step[1]} {field} {got}, expected {value}'
