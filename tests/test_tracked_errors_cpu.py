"""The messages of the six updates that follow track ids, word for word: every malformed input of one table goes
through `ops.smooth_poses`, `zone_events`, `posture_events`, `heat_update`, `trail_update` and `floor_update`, and
through `PoseSmoother`, `ZoneMonitor`, `PostureMonitor`, `FootfallMap`, `TrackTrails` and `GroundPlane`.  Where two
checks could both fire the case names the one that does.  Everything here is raised before a device is asked for
anything, so host tensors do."""
import pytest
import torch

K, CAMERAS, S = 17, 2, 4
I32 = dict(dtype=torch.int32)


def _state(**shapes):
    return {name: torch.zeros(shape, **I32) for name, shape in shapes.items()}


def _smooth(entries, **kw):
    from pavenet_amd import ops
    st = _state(id=(CAMERAS, S), last=(CAMERAS, S), pos=(CAMERAS, S, K + 2, 2), vel=(CAMERAS, S, K + 2, 2),
                frame=(CAMERAS,), dropped=(CAMERAS,))
    return ops.smooth_poses(entries, st, **kw)


def _zones(entries, **kw):
    from pavenet_amd import native, ops
    st = _state(id=(CAMERAS, S), last=(CAMERAS, S), pos=(CAMERAS, S, 2), inside=(CAMERAS, S), alerted=(CAMERAS, S),
                streak=(CAMERAS, S, 8), since=(CAMERAS, S, 8), frame=(CAMERAS,), dropped=(CAMERAS,),
                counters=(CAMERAS, native.ZONE_COUNTER_WORDS), geometry=(CAMERAS, native.ZONE_GEOM_WORDS))
    return ops.zone_events(entries, st, K=K, **kw)


def _posture(entries, **kw):
    from pavenet_amd import native, ops
    st = _state(frame=(CAMERAS,), dropped=(CAMERAS,), counters=(CAMERAS, native.POSTURE_COUNTER_WORDS),
                **{n: (CAMERAS, S) for n in ('id', 'last', 'posture', 'since', 'upright', 'streak', 'alerted', 'hands',
                                             'hand_streak')})
    return ops.posture_events(entries, st, K=K, parts=[[5, 6], [11, 12], [15, 16], [9, 10]], **kw)


def _heat(entries, **kw):
    from pavenet_amd import ops
    st = _state(id=(CAMERAS, S), last=(CAMERAS, S), cell=(CAMERAS, S), frame=(CAMERAS,), dropped=(CAMERAS,),
                peak=(CAMERAS, 2), dwell=(CAMERAS, 6, 8), visits=(CAMERAS, 6, 8))
    return ops.heat_update(entries, st, K=K, size=(64, 48), cell=8, **kw)


def _trails(entries, **kw):
    from pavenet_amd import ops
    st = _state(id=(CAMERAS, S), last=(CAMERAS, S), pos=(CAMERAS, S, 2), head=(CAMERAS, S), count=(CAMERAS, S),
                box=(CAMERAS, S, 4), pts=(CAMERAS, S, 4, 2), when=(CAMERAS, S, 4), frame=(CAMERAS,),
                dropped=(CAMERAS,))
    return ops.trail_update(entries, st, K=K, **kw)


def _floor(entries, **kw):
    from pavenet_amd import native, ops
    st = _state(id=(CAMERAS, S), last=(CAMERAS, S), hits=(CAMERAS, S), pos=(CAMERAS, S, 2), vel=(CAMERAS, S, 2),
                travel=(CAMERAS, S), frame=(CAMERAS,), dropped=(CAMERAS,))
    calib = torch.zeros(CAMERAS, native.FLOOR_CALIB_WORDS, dtype=torch.int64)
    return ops.floor_update(entries, st, calib, K=K, **kw)


OPS = dict(smooth_poses=_smooth, zone_events=_zones, posture_events=_posture, heat_update=_heat, trail_update=_trails,
           floor_update=_floor)
ANCHORED = ('zone_events', 'heat_update', 'trail_update', 'floor_update')


def _entry(n=3, **over):
    e = dict(kpts=torch.zeros(n, K, 3), bboxes=torch.zeros(n, 5), keep=None, ids=torch.ones(n, **I32), camera=0,
             scale=(1.0, 1.0))
    e.update(over)
    return tuple(e[k] for k in ('kpts', 'bboxes', 'keep', 'ids', 'camera', 'scale'))


GOOD = _entry()
# name, entries, keywords, the message after f'{who}: ', the entry points it applies to (None: all six)
OPS_CASES = [
    ('five fields', [GOOD[:5]], {}, 'entry 0 is (kpts, bboxes, keep, ids, camera, (sx, sy))', None),
    ('a dict', [dict(kpts=GOOD[0])], {}, 'entry 0 is (kpts, bboxes, keep, ids, camera, (sx, sy))', None),
    ('the second entry', [GOOD, GOOD + (0,)], {}, 'entry 1 is (kpts, bboxes, keep, ids, camera, (sx, sy))', None),
    ('kpts float64', [_entry(kpts=torch.zeros(3, K, 3, dtype=torch.float64))], {},
     f'kpts of entry 0 must be a [N, {K}, 3] float32 tensor', None),
    ('kpts rank 2', [_entry(kpts=torch.zeros(3, K * 3))], {}, f'kpts of entry 0 must be a [N, {K}, 3] float32 tensor',
     None),
    ('kpts K', [_entry(kpts=torch.zeros(3, 15, 3))], {}, f'kpts of entry 0 must be a [N, {K}, 3] float32 tensor', None),
    ('kpts not a tensor', [_entry(kpts=[[0.0] * 3] * K)], {}, f'kpts of entry 0 must be a [N, {K}, 3] float32 tensor',
     None),
    ('bboxes columns', [_entry(bboxes=torch.zeros(3, 4))], {}, 'bboxes of entry 0 must be a [3, 5] float32 tensor', None),
    ('bboxes rows', [GOOD, _entry(bboxes=torch.zeros(2, 5))], {}, 'bboxes of entry 1 must be a [3, 5] float32 tensor',
     None),
    ('keep int64', [_entry(keep=torch.ones(3, dtype=torch.int64))], {}, 'keep of entry 0 must be a [3] int32 tensor',
     None),
    ('keep bool', [_entry(keep=torch.ones(3, dtype=torch.bool))], {}, 'keep of entry 0 must be a [3] int32 tensor', None),
    ('ids shape', [_entry(ids=torch.ones(2, **I32))], {}, 'ids of entry 0 must be a [3] int32 tensor', None),
    ('ids None', [_entry(ids=None)], {}, 'ids of entry 0 must be a [3] int32 tensor', None),
    ('ids int64', [_entry(ids=torch.ones(3, dtype=torch.int64))], {}, 'ids of entry 0 must be a [3] int32 tensor', None),
    ('129 poses', [_entry(n=129)], {}, 'entry 0 has 129 poses, at most 128', None),
    ('camera 2', [_entry(camera=2)], {}, f'the camera of entry 0 must be an integer in [0, {CAMERAS}), got 2', None),
    ('camera -1', [_entry(camera=-1)], {}, f'the camera of entry 0 must be an integer in [0, {CAMERAS}), got -1', None),
    ('camera True', [_entry(camera=True)], {}, f'the camera of entry 0 must be an integer in [0, {CAMERAS}), got True',
     None),
    ('camera 0.5', [_entry(camera=0.5)], {}, f'the camera of entry 0 must be an integer in [0, {CAMERAS}), got 0.5', None),
    ('scale a number', [_entry(scale=1.0)], {}, 'the scale of entry 0 is (sx, sy)', None),
    ('scale of three', [_entry(scale=(1.0, 1.0, 1.0))], {}, 'the scale of entry 0 is (sx, sy)', None),
    ('scale of words', [_entry(scale=('a', 'b'))], {}, 'the scale of entry 0 is (sx, sy)', None),
    ('scale zero', [_entry(scale=(1, 0))], {}, 'the scale of entry 0 must be positive and finite, got (1.0, 0.0)', None),
    ('scale negative', [_entry(scale=(-2.0, 1.0))], {},
     'the scale of entry 0 must be positive and finite, got (-2.0, 1.0)', None),
    ('scale inf', [_entry(scale=(1.0, float('inf')))], {},
     'the scale of entry 0 must be positive and finite, got (1.0, inf)', None),
    ('scale nan', [_entry(scale=(float('nan'), 1.0))], {},
     'the scale of entry 0 must be positive and finite, got (nan, 1.0)', None),
    ('kpts not contiguous', [_entry(kpts=torch.zeros(3, K, 6)[:, :, ::2])], {},
     'the tensors of entry 0 must be contiguous', None),
    ('ids not contiguous', [GOOD, _entry(ids=torch.ones(6, **I32)[::2])], {}, 'the tensors of entry 1 must be contiguous',
     None),
    ('a host state', [GOOD], {}, 'the state must be on a HIP device (pavenet_amd has no CPU path), got cpu', None),
    ('a host state and no entry', [], {}, 'the state must be on a HIP device (pavenet_amd has no CPU path), got cpu',
     None),
    ('max_age -1', [GOOD], dict(max_age=-1), 'max_age must be an integer >= 0, got -1', None),
    ('max_age 1.5', [GOOD], dict(max_age=1.5), 'max_age must be an integer >= 0, got 1.5', None),
    ('max_age True', [GOOD], dict(max_age=True), 'max_age must be an integer >= 0, got True', None),
    ('anchor', [GOOD], dict(anchor='toes'), "anchor must be one of feet, box, centre, got 'toes'", ANCHORED),
    ('five anchor_kpts', [GOOD], dict(anchor_kpts=(0, 1, 2, 3, 4)),
     f'anchor_kpts holds at most 4 integers in [0, {K}), got [0, 1, 2, 3, 4]', ANCHORED),
    ('anchor_kpts K', [GOOD], dict(anchor_kpts=(K,)), f'anchor_kpts holds at most 4 integers in [0, {K}), got [{K}]',
     ANCHORED),
    ('anchor_kpts True', [GOOD], dict(anchor_kpts=(True,)),
     f'anchor_kpts holds at most 4 integers in [0, {K}), got [True]', ANCHORED),
    # two defects: the one that is reported
    ('max_age before the anchor', [GOOD], dict(max_age=-1, anchor='toes'), 'max_age must be an integer >= 0, got -1',
     ANCHORED),
    ('the anchor before its key points', [GOOD], dict(anchor='toes', anchor_kpts=(K,)),
     "anchor must be one of feet, box, centre, got 'toes'", ANCHORED),
    ('max_age before an entry', [GOOD[:5]], dict(max_age=-1), 'max_age must be an integer >= 0, got -1', None),
    ('anchor_kpts before an entry', [GOOD[:5]], dict(anchor_kpts=(K,)),
     f'anchor_kpts holds at most 4 integers in [0, {K}), got [{K}]', ANCHORED),
    ('kpts before bboxes', [_entry(kpts=torch.zeros(3, 15, 3), bboxes=torch.zeros(3, 4))], {},
     f'kpts of entry 0 must be a [N, {K}, 3] float32 tensor', None),
    ('ids before the pose count', [_entry(n=129, ids=torch.ones(128, **I32))], {},
     'ids of entry 0 must be a [129] int32 tensor', None),
    ('the pose count before the camera', [_entry(n=129, camera=2)], {}, 'entry 0 has 129 poses, at most 128', None),
    ('the camera before the scale', [_entry(camera=2, scale=(0, 0))], {},
     f'the camera of entry 0 must be an integer in [0, {CAMERAS}), got 2', None),
    ('the scale before contiguity', [_entry(kpts=torch.zeros(3, K, 6)[:, :, ::2], scale=(0, 1))], {},
     'the scale of entry 0 must be positive and finite, got (0.0, 1.0)', None),
    ('entry 0 before entry 1', [_entry(camera=2), GOOD[:5]], {},
     f'the camera of entry 0 must be an integer in [0, {CAMERAS}), got 2', None),
]


@pytest.mark.parametrize('who', list(OPS))
def test_ops_messages(who):
    ran = 0
    for name, entries, kw, message, only in OPS_CASES:
        if only is not None and who not in only:
            continue
        with pytest.raises(ValueError) as err:
            OPS[who](entries, **kw)
        assert str(err.value) == f'{who}: {message}', name
        ran += 1
    assert ran == (len(OPS_CASES) if who in ANCHORED else sum(1 for c in OPS_CASES if c[4] is None))


def _classes():
    from pavenet_amd.floor import GroundPlane
    from pavenet_amd.heatmap import FootfallMap
    from pavenet_amd.posture import PostureMonitor
    from pavenet_amd.smoothing import PoseSmoother
    from pavenet_amd.trails import TrackTrails
    from pavenet_amd.zones import ZoneMonitor
    # the class, its extra positional arguments, the `who` of its update, "the X" of its K, "the X's" of its state
    return dict(PoseSmoother=(PoseSmoother, (), 'PoseSmoother.smooth', 'the smoother'),
                ZoneMonitor=(ZoneMonitor, (), 'ZoneMonitor.update', 'the monitor'),
                PostureMonitor=(PostureMonitor, (), 'PostureMonitor.update', 'the monitor'),
                FootfallMap=(FootfallMap, ((64, 48),), 'FootfallMap.update', 'the map'),
                TrackTrails=(TrackTrails, (), 'TrackTrails.update', 'the trails'),
                GroundPlane=(GroundPlane, (), 'GroundPlane.update', 'the plane'))


CLASSES = ('PoseSmoother', 'ZoneMonitor', 'PostureMonitor', 'FootfallMap', 'TrackTrails', 'GroundPlane')
CLASS_ANCHORED = ('ZoneMonitor', 'FootfallMap', 'TrackTrails', 'GroundPlane')


@pytest.mark.parametrize('name', CLASSES)
def test_class_messages(name):
    cls, extra, who, noun = _classes()[name]
    m = cls(K, *extra, cameras=CAMERAS, max_tracks=S)
    many = m.smooth_many if name == 'PoseSmoother' else m.update_many
    one = m.smooth if name == 'PoseSmoother' else m.update
    kp, bb, ids = torch.zeros(3, K, 3), torch.zeros(3, 5), torch.ones(3, **I32)
    res = (bb, None, kp)
    big = (torch.zeros(129, 5), None, torch.zeros(129, K, 3))
    triples = f'{who}: items are (camera, result, ids) triples'
    camera = f'camera must be an integer in [0, {CAMERAS}), got'
    host = f'{who}: results[0] and its ids must be HIP device tensors (pavenet_amd has no CPU path)'
    for label, call, message in (
            ('a pair', lambda: many([(0, res)]), triples),
            ('four fields', lambda: many([(0, res, ids), (0, res, ids, 1.0)]), triples),
            ('not a sequence', lambda: many([7]), triples),
            ('camera 2', lambda: one(res, ids, camera=2), f'{who}: {camera} 2'),
            ('camera True', lambda: one(res, ids, camera=True), f'{who}: {camera} True'),
            ('camera -1', lambda: many([(0, res, ids), (-1, res, ids)]), f'{who}: {camera} -1'),
            ('a pair as the result', lambda: one((bb, kp), ids),
             f'{who}: results[0] is a (bboxes, labels, kpts) tuple or a dict(bboxes=, kpts=, keep=)'),
            ('a dict without kpts', lambda: one(dict(bboxes=bb), ids), f'{who}: results[0] needs bboxes and kpts'),
            ('kpts float64', lambda: one((bb, None, kp.double()), ids),
             f'{who}: kpts and bboxes of results[0] must be float32'),
            ('kpts rank 2', lambda: one((bb, None, kp.view(3, -1)), ids),
             f'{who}: results[0] needs kpts [N, K, 3] and bboxes [N, 5], got (3, {3 * K}) and (3, 5)'),
            ('bboxes columns', lambda: many([(0, res, ids), (0, (bb[:, :4], None, kp), ids)]),
             f'{who}: results[1] needs kpts [N, K, 3] and bboxes [N, 5], got (3, {K}, 3) and (3, 4)'),
            ('keep int64', lambda: one(dict(bboxes=bb, kpts=kp, keep=ids.long()), ids),
             f'{who}: keep of results[0] must be int32 [3]'),
            ('three scales for two', lambda: many([(0, res, ids), (1, res, ids)], scale_factor=[1.0, 1.0, 1.0]),
             f'{who}: scale_factor is one value or one per surface (2), got 3'),
            ('scale zero', lambda: one(res, ids, scale_factor=0.0), f'{who}: a scale factor must be positive and finite'),
            ('scale inf', lambda: one(res, ids, scale_factor=(1.0, float('inf'))),
             f'{who}: a scale factor must be positive and finite'),
            ('K', lambda: one((bb, None, torch.zeros(3, 15, 3)), ids), f'{who}: results[0] has K = 15, {noun} K = {K}'),
            ('129 poses', lambda: one(big, torch.ones(129, **I32)), f'{who}: results[0] has 129 poses, at most 128'),
            ('ids int64', lambda: one(res, ids.long()), f'{who}: ids of results[0] must be an int32 [3] tensor'),
            ('ids shape', lambda: one(res, ids[:2]), f'{who}: ids of results[0] must be an int32 [3] tensor'),
            ('ids None', lambda: one(res, None), f'{who}: ids of results[0] must be an int32 [3] tensor'),
            ('host tensors', lambda: one(res, ids), host),
            # two defects: the one that is reported
            ('the triples before a camera', lambda: many([(2, res, ids), (0, res)]), triples),
            ('the camera before the result', lambda: one((bb, kp), ids, camera=2), f'{who}: {camera} 2'),
            ('the result before the scale', lambda: one((bb, kp), ids, scale_factor=0.0),
             f'{who}: results[0] is a (bboxes, labels, kpts) tuple or a dict(bboxes=, kpts=, keep=)'),
            ('the scale before K', lambda: one((bb, None, torch.zeros(3, 15, 3)), ids, scale_factor=0.0),
             f'{who}: a scale factor must be positive and finite'),
            ('K before the pose count', lambda: one((big[0], None, torch.zeros(129, 15, 3)), torch.ones(129, **I32)),
             f'{who}: results[0] has K = 15, {noun} K = {K}'),
            ('the pose count before the ids', lambda: one(big, ids), f'{who}: results[0] has 129 poses, at most 128'),
            ('the first result before the second', lambda: many([(0, res, ids), (1, res, ids[:2])]), host),
            ('reset', lambda: m.reset(camera=CAMERAS), f'{name}.reset: {camera} {CAMERAS}'),
            ('reset True', lambda: m.reset(True), f'{name}.reset: {camera} True'),
            ('state', lambda: m.state(-1), f'{name}.state: {camera} -1'),
            ('max_age -1', lambda: cls(K, *extra, max_age=-1), f'{name}: max_age is an integer >= 0, got -1'),
            ('max_age 1.5', lambda: cls(K, *extra, max_age=1.5), f'{name}: max_age is an integer >= 0, got 1.5')):
        with pytest.raises(ValueError) as err:
            call()
        assert str(err.value) == message, label
    if name in CLASS_ANCHORED:
        for label, call, message in (
                ('anchor', lambda: cls(K, *extra, anchor='toes'), f"{name}: anchor is 'feet', 'box' or 'centre', got 'toes'"),
                ('five anchor_kpts', lambda: cls(K, *extra, anchor_kpts=(0, 1, 2, 3, 4)),
                 f'{name}: at most 4 anchor_kpts, got 5'),
                ('anchor_kpts K', lambda: cls(K, *extra, anchor_kpts=(K,)),
                 f'{name}: anchor_kpts are integers in [0, {K}), got [{K}]'),
                ('max_age before the anchor', lambda: cls(K, *extra, max_age=-1, anchor='toes'),
                 f'{name}: max_age is an integer >= 0, got -1')):
            with pytest.raises(ValueError) as err:
                call()
            assert str(err.value) == message, label
    assert many([]) == [] and m._state is None and m.state() is None and m.reset() is None
