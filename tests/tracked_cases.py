"""One script of frames for the rule every analytic that follows track ids shares (who takes
part, expiry, find a slot, births, dropped), made to go wrong wherever that rule can: K = 17, two cameras interleaved,
N from 0 to 6, `MAX_AGE` = 2, for S = 2 and S = 4.  `script()` is a list of steps; a step is a list of (camera, kpts
[N, 17, 3], bboxes [N, 5], ids [N], keep [N] or None) frames in numpy.  A step of one frame is one `update`; the last
step is one `update_many` of 33 frames, so that camera 0's frames straddle the 32-entry launch split.

Per camera, with f its clock (the hand-made frames; S = 2 drops what S = 4 still takes):
  camera 0
    f1  ids 1 (score 0.1), 1, 2, 0, -1      a duplicate id whose first copy is invalid: the second takes part; 0 and -1
    f2  ids 3, 4, 5 (score == score_thr), 6 (keep 0)       two births: S = 2 has no free slot, dropped + 2
    f3  ids 1, 7 (a NaN key point), 8 (an infinite box corner)    id 1 at exactly max_age: the same slot, no birth
    f4  ids 2, 3, 5, 6, 7, 8                id 2 at max_age + 1: expired and born again; more births than free slots
    f5  no pose
    f6  ids 9, 9                            both copies valid: the first takes part
  camera 1
    f1  ids 5, 5 (keep 0), 6
    f2  no pose
    f3  ids 6                               at exactly max_age
    f4  ids 5, 7, 8, 9, 10                  id 5 at max_age + 1; S = 2: dropped moves
then 33 seeded random frames, cameras alternating, ids -1 .. 6, keep on and off, a NaN or an infinity now and then."""
import numpy as np

K, CAMERAS, MAX_AGE, SCORE_THR = 17, 2, 2, 0.3
SIZE = (256, 256)        # every box and key point lies inside: the picture of the footfall map


def _pose(i, score=0.9, nan=False, inf=False):
    """Pose number i of a frame: a box and 17 key points inside it, all in [8, 232)."""
    x, y, w, h = 8.0 + 31.0 * (i % 6), 16.0 + 23.0 * (i % 5), 20.0 + 3.0 * i, 40.0 + 2.0 * i
    bbox = np.array([x, y, x + w, y + h, score], np.float32)
    kpts = np.empty((K, 3), np.float32)
    kpts[:, 0] = x + w * (0.25 + 0.5 * (np.arange(K) % 2))
    kpts[:, 1] = y + h * np.arange(K) / (K - 1)
    kpts[:, 2] = 0.8
    if nan:
        kpts[3, 1] = np.nan
    if inf:
        bbox[2] = np.inf
    return kpts, bbox


def _frame(camera, poses, keep=None):
    """poses: (id, keywords of _pose) pairs."""
    made = [_pose(i, **kw) for i, (_, kw) in enumerate(poses)]
    kpts = np.stack([m[0] for m in made]) if made else np.zeros((0, K, 3), np.float32)
    bboxes = np.stack([m[1] for m in made]) if made else np.zeros((0, 5), np.float32)
    ids = np.array([ident for ident, _ in poses], np.int32)
    return camera, kpts, bboxes, ids, None if keep is None else np.array(keep, np.int32)


def script():
    ok = {}
    cam0 = [_frame(0, [(1, dict(score=0.1)), (1, ok), (2, ok), (0, ok), (-1, ok)]),
            _frame(0, [(3, ok), (4, ok), (5, dict(score=SCORE_THR)), (6, ok)], keep=[1, 1, 1, 0]),
            _frame(0, [(1, ok), (7, dict(nan=True)), (8, dict(inf=True))]),
            _frame(0, [(2, ok), (3, ok), (5, ok), (6, ok), (7, ok), (8, ok)]),
            _frame(0, []),
            _frame(0, [(9, ok), (9, ok)])]
    cam1 = [_frame(1, [(5, ok), (5, ok), (6, ok)], keep=[1, 0, 1]),
            _frame(1, []),
            _frame(1, [(6, ok)]),
            _frame(1, [(5, ok), (7, ok), (8, ok), (9, ok), (10, ok)])]
    steps = []
    for i in range(len(cam0)):      # interleaved, one frame per step
        steps.append([cam0[i]])
        if i < len(cam1):
            steps.append([cam1[i]])
    rng = np.random.RandomState(1709)
    many = []
    for i in range(33):
        n = int(rng.randint(0, 7))
        poses = [(int(rng.randint(-1, 7)), dict(score=float(rng.choice([0.9, 0.9, 0.9, 0.1])),
                                                nan=bool(rng.rand() < 0.08), inf=bool(rng.rand() < 0.08)))
                 for _ in range(n)]
        keep = [int(rng.rand() < 0.85) for _ in range(n)] if i % 3 else None
        many.append(_frame(i % 2, poses, keep))
    steps.append(many)
    return steps


def references(S):
    """The six numpy references at the script's settings, each as (name, object, the name of its update method)."""
    from tests.floor_ref import FloorRef
    from tests.heat_ref import HeatRef
    from tests.posture_ref import PostureRef
    from tests.smooth_ref import SmoothRef
    from tests.trail_ref import TrailRef
    from tests.zones_ref import ZoneRef
    kw = dict(cameras=CAMERAS, max_tracks=S, max_age=MAX_AGE, score_thr=SCORE_THR)
    floor = FloorRef(K, **kw)
    for c in range(CAMERAS):
        floor.set_plane(c, matrix=np.eye(3))      # a pixel is a millimetre; the bounds are the whole range
    return [('SmoothRef', SmoothRef(K, **kw), 'smooth'), ('ZoneRef', ZoneRef(K, **kw), 'update'),
            ('PostureRef', PostureRef(K, **kw), 'update'), ('HeatRef', HeatRef(K, SIZE, **kw), 'update'),
            ('TrailRef', TrailRef(K, length=4, **kw), 'update'), ('FloorRef', floor, 'update')]


def shared(state):
    """What the rule fixes of one camera's state (numpy or torch): id, frame, dropped, and last where a slot is live."""
    ident, last = state['id'], state['last']
    return dict(id=ident, frame=state['frame'], dropped=state['dropped'], last=last * (ident != 0))
