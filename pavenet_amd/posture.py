"""Postures and falls for the live path (``csrc/pave_posture.hip``): whether a tracked person is
upright, low (crouching or sitting), leaning or lying, who fell, who stays down and who raised their hands, per track
id, on the device, by an integer-exact rule on the key points of the trunk, the legs and the wrists.
``PostureMonitor.update`` sits where ``ZoneMonitor.update`` sits -- after ``PoseTracker.update`` (or after
``PoseSmoother.smooth``, with ``scale_factor=None``) -- and takes the same arguments: a result in either form and the
frame's track ids.  It returns a posture per pose and the frame's events as a fixed-shape table and keeps running
counters, without reading a device value on the host.

The class is read from the trunk in the picture, so it knows what a camera from the side knows: see "Not built".

Not built: a person lying along the camera's axis (the trunk is foreshortened, not flat; a box-aspect test would be
the next step), sitting versus crouching, drawing postures or alerts into the picture, per-zone posture rules, any
learned classifier.
"""
import torch

from . import native, ops
from .tracked import Tracked

UNKNOWN, UPRIGHT, LOW, LEANING, LYING = (
    native.DEFINES['PAVE_POSTURE_' + n] for n in ('UNKNOWN', 'UPRIGHT', 'LOW', 'LEANING', 'LYING'))
POSTURES = {UNKNOWN: 'unknown', UPRIGHT: 'upright', LOW: 'low', LEANING: 'leaning', LYING: 'lying'}
POSTURE, FALL, DOWN, HANDS_UP, HANDS_DOWN = (
    native.DEFINES['PAVE_POSTURE_EV_' + n] for n in ('POSTURE', 'FALL', 'DOWN', 'HANDS_UP', 'HANDS_DOWN'))
KINDS = {POSTURE: 'posture', FALL: 'fall', DOWN: 'down', HANDS_UP: 'hands_up', HANDS_DOWN: 'hands_down'}
PART_NAMES = ops.POSTURE_PARTS                        # shoulders, hips, ankles, wrists
MAX_PART, MAX_SLOPE, MAX_WAIT = native.POSTURE_MAX_PART, native.POSTURE_MAX_SLOPE, native.POSTURE_MAX_WAIT
PARTS = {17: dict(shoulders=(5, 6), hips=(11, 12), ankles=(15, 16), wrists=(9, 10)),      # COCO
         15: dict(shoulders=(3, 4), hips=(9, 10), ankles=(13, 14), wrists=(7, 8)),        # PoseTrack
         14: dict(shoulders=(0, 1), hips=(6, 7), ankles=(10, 11), wrists=(4, 5))}         # CrowdPose
_C = {n: native.DEFINES['PAVE_POSTURE_CNT_' + n] for n in ('NOW', 'HANDS_UP', 'FALLS', 'DOWNS')}
_SLOTS = ('id', 'last', 'posture', 'since', 'upright', 'streak', 'alerted', 'hands', 'hand_streak')
_STATE = _SLOTS + ('frame', 'dropped')


class PostureMonitor(Tracked):
    """Classes the tracked poses of `cameras` cameras by the slope of the trunk: one slot per track id (`max_tracks`,
    1 .. 128; a slot not seen for more than `max_age` frames is freed).  A pose takes part iff its box score is >
    `score_thr` (and keep, and finite coordinates), its id is >= 1 and no pose before it in the frame has the same id.

    `parts` names the key points of the shoulders, hips, ankles and wrists (at most 4 each, visible iff their score
    is > `kpt_thr`); those of the 17-, 15- and 14-point skeletons are built in.  With (dx, dy) from the shoulders to
    the hips a pose is LYING iff 16 |dy| <= `flat` |dx|, else UPRIGHT iff dy > 0 and 16 |dx| <= `lean` dy -- LOW
    instead iff the ankles are less than `squat` / 16 trunk heights below the hips (0: never) -- and LEANING
    otherwise; a wrist is raised iff it is `hand_up` / 16 trunk heights above the shoulders of an UPRIGHT or LOW
    pose (None: no hands).  A track's posture follows the raw class, and its hand bit the raw one, once it has
    disagreed `min_frames` (1 .. 255) frames in a row.  LYING within `fall_window` frames of UPRIGHT is a fall, and
    `down_frames` frames of LYING are reported once per stay (0: never).  `max_events` (1 .. 4096) rows of events
    are stored per frame, and all of them are counted."""
    _NOUN, _NOUNS = 'the monitor', "the monitor's"
    _RESET = ('id', 'frame', 'dropped', 'counters')

    def __init__(self, K, cameras=1, max_tracks=128, max_age=30, parts=None, min_frames=3, lean=11, flat=11, squat=18,
                 hand_up=4, fall_window=30, down_frames=75, max_events=256, score_thr=0.3, kpt_thr=0.):
        who = 'PostureMonitor'
        if isinstance(K, bool) or int(K) != K or not 1 <= K <= native.TRACK_MAX_K:
            raise ValueError(f'{who}: K is an integer in 1 .. {native.TRACK_MAX_K}, got {K!r}')
        for name, v, lo, hi in (('cameras', cameras, 1, native.TRACK_MAX_CAMERAS),
                                ('max_tracks', max_tracks, 1, native.TRACK_MAX_TRACKS),
                                ('min_frames', min_frames, 1, 255), ('lean', lean, 1, MAX_SLOPE),
                                ('flat', flat, 1, MAX_SLOPE), ('squat', squat, 0, MAX_SLOPE),
                                ('hand_up', 0 if hand_up is None else hand_up, 0, MAX_SLOPE),
                                ('fall_window', fall_window, 0, MAX_WAIT), ('down_frames', down_frames, 0, MAX_WAIT),
                                ('max_events', max_events, 1, native.POSTURE_MAX_EVENTS)):
            if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
                raise ValueError(f'{who}: {name} is an integer in {lo} .. {hi}, got {v!r}')
        if isinstance(max_age, bool) or int(max_age) != max_age or max_age < 0:
            raise ValueError(f'{who}: max_age is an integer >= 0, got {max_age!r}')
        K = int(K)
        if parts is None:
            if K not in PARTS:
                raise ValueError(f'{who}: the parts of K = 17, 15 and 14 are built in; K = {K} needs parts=dict('
                                 f'{", ".join(n + "=" for n in PART_NAMES)})')
            parts = PARTS[K]
        if not isinstance(parts, dict) or sorted(parts) != sorted(PART_NAMES):
            raise ValueError(f'{who}: parts is a dict of {", ".join(PART_NAMES)}, got {parts!r}')
        try:
            parts = {n: tuple(parts[n]) for n in PART_NAMES}
        except TypeError:
            raise ValueError(f'{who}: every part is a sequence of key points, got {parts!r}') from None
        for n, p in parts.items():
            if len(p) > MAX_PART:
                raise ValueError(f'{who}: at most {MAX_PART} key points in a part, {n} has {len(p)}')
            if any(isinstance(k, bool) or not isinstance(k, int) or not 0 <= k < K for k in p):
                raise ValueError(f'{who}: the key points of {n} are integers in [0, {K}), got {p!r}')
        self.K, self.cameras, self.max_tracks, self.max_age = K, cameras, max_tracks, int(max_age)
        self.parts, self.min_frames = parts, min_frames
        self.lean, self.flat, self.squat, self.hand_up = lean, flat, squat, hand_up
        self.fall_window, self.down_frames, self.max_events = fall_window, down_frames, max_events
        self.score_thr, self.kpt_thr = float(score_thr), float(kpt_thr)
        self._state = None

    def _allocate(self, dev):
        C, S = self.cameras, self.max_tracks
        z = dict(dtype=torch.int32, device=dev)
        self._state = {name: torch.zeros((C, S), **z) for name in _SLOTS}
        self._state.update(frame=torch.zeros((C,), **z), dropped=torch.zeros((C,), **z),
                           counters=torch.zeros((C, native.POSTURE_COUNTER_WORDS), **z))

    def update_many(self, items, scale_factor=None):
        """items: (camera, result, ids) triples, the entries of one camera in time order -> one dict per item of new
        int32 device tensors: posture [N] (the debounced posture of the pose's track, UNKNOWN .. LYING; -1: the pose
        takes no part), raw [N] (this frame's class, or -1), hands [N] (this frame's raised wrists as bits), since [N]
        (frames in the current posture), events [max_events, 5] (rows (kind, index, id, pose, frame) in the rule's
        order; zero past the count) and n_events (0-d: all events of the frame, stored or not).  result, ids and
        scale_factor are what `ZoneMonitor.update_many` takes.  One launch per 32 items."""
        items = list(items)
        entries = self._entries(items, scale_factor, 'PostureMonitor.update')
        if not entries:
            return []
        return ops.posture_events(entries, self._state, K=self.K, parts=[self.parts[n] for n in PART_NAMES],
                                  max_age=self.max_age, min_frames=self.min_frames, lean=self.lean, flat=self.flat,
                                  squat=self.squat, hand_up=self.hand_up, fall_window=self.fall_window,
                                  down_frames=self.down_frames, max_events=self.max_events, score_thr=self.score_thr,
                                  kpt_thr=self.kpt_thr)

    def update(self, result, ids, scale_factor=None, camera=0):
        """One frame of `camera` with its track ids -> dict(posture=, raw=, hands=, since=, events=, n_events=)."""
        return self.update_many([(camera, result, ids)], scale_factor)[0]

    def reset(self, camera=None):
        """Frees the slots of `camera` (None: of every camera) without events; its frame count, drop count and
        counters restart at 0.  The state tensors stay where they are (a birth writes a slot, and a free slot is
        never read)."""
        self._reset(camera)

    def counts(self, camera=0):
        """Views of one camera's running counters on the device: now [5] (the live slots per posture, UNKNOWN ..
        LYING; their sum is the live slots), hands_up (the live slots with a raised hand), falls and downs (0-d
        running totals).  None before the first call."""
        camera = self._camera(camera, 'PostureMonitor.counts')
        if self._state is None:
            return None
        row = self._state['counters'][camera]
        return dict(now=row[_C['NOW']:_C['NOW'] + native.POSTURE_CLASSES], hands_up=row[_C['HANDS_UP']],
                    falls=row[_C['FALLS']], downs=row[_C['DOWNS']])

    def state(self, camera=0):
        """Views of one camera's state on the device: id, last, posture, since, upright, streak, alerted, hands,
        hand_streak [S] (id 0 = free slot; its other fields mean nothing), frame, dropped (0-d).  None before the
        first call."""
        return self._views(camera, 'state', _STATE)


def events_to_list(out):
    """The events of one `update` as a list of dict(kind=, index=, id=, pose=, frame=) on the host, kind one of
    'posture', 'fall', 'down', 'hands_up', 'hands_down', index the new class ('posture'), the frames since the track
    was upright ('fall'), the frames lying ('down') or the raised wrists as bits, pose the row of the result.  THE host
    copy of this module: it reads n_events and the table from the device, which waits for the stream.  Only the rows
    that were stored are listed (`out['n_events']` may be larger)."""
    n = min(int(out['n_events']), out['events'].shape[0])
    return [dict(kind=KINDS[k], index=i, id=t, pose=p, frame=f) for k, i, t, p, f in out['events'][:n].tolist()]
