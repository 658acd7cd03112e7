"""Contacts and groups on the floor for the live path (``csrc/pave_contacts.hip``): who stands with
whom.  ``GroundPlane.update`` says per frame how far everybody's nearest neighbour is; ``ContactMonitor.update`` sits
directly behind it, takes the dict it returned and the frame's track ids, and keeps what lasts: a contact bit per pair
of tracks, debounced and with hysteresis (a pair meets within `radius` and parts beyond `release`), since when the two
have been together, the parties they form -- the connected components of the contact graph -- and the frame's MEET,
PART and LONG events as a fixed-shape table, with running counters.  The rule is integer-exact and nothing is read on
the host.

    plane, mon = GroundPlane(K), ContactMonitor(radius=1500, release=1800, long_frames=250)
    plane.set_plane(0, points=[...])
    for result, ids in frames:
        placed = plane.update(result, ids, scale_factor)
        out = mon.update(placed, ids)            # group, size, contacts, partner, together [N]; events; n_events
    contacts.events_to_list(out)                 # THE host copy

Not built: contacts across cameras; group-level events (a group formed, was joined or split); drawing the links into
the picture; rules per zone.
"""
import torch

from . import native, ops
from .tracked import Tracked

MEET, PART, LONG = (native.DEFINES['PAVE_CONTACT_' + n] for n in ('MEET', 'PART', 'LONG'))
KINDS = {MEET: 'meet', PART: 'part', LONG: 'long'}
_C = {n.lower(): native.DEFINES['PAVE_CONTACT_CNT_' + n] for n in ('CONTACTS', 'MEETS', 'PARTS', 'LONGS', 'GROUPS', 'GROUPED',
                                                                   'LARGEST')}
_STATE = ('id', 'last', 'pos', 'frame', 'dropped')


class ContactMonitor(Tracked):
    """The contacts among the tracks of each of `cameras` cameras, one slot per track id (`max_tracks`, 1 .. 128; a
    slot not seen for more than `max_age` frames is freed, and its contacts part).  A pose takes part iff it is on the
    floor, its id is >= 1 and no such pose before it in the frame has the same id.  Two tracks that are not in contact
    are near within `radius` mm (0 .. 2^20), two that are within `release` mm (`radius` .. 2^21; None: `radius`); the
    contact bit flips once that test has disagreed with it `min_frames` (1 .. 255) frames in a row in which both were
    seen.  A contact that has lasted `long_frames` (0 .. 2^30; 0: never) frames is reported once.  `max_events` (1 ..
    4096) rows of events are stored per frame, and all of them are counted.

    Memory: two int32 words per pair of slots, `cameras` x `max_tracks`^2 x 8 bytes (128 KiB a camera at 128 tracks),
    beside the slot arrays; allocated on the first call and never again."""
    _NOUN, _NOUNS = 'the monitor', "the monitor's"
    _RESET = ('id', 'frame', 'dropped', 'counters')

    def __init__(self, cameras=1, max_tracks=128, max_age=30, radius=1500, release=None, min_frames=3, long_frames=0,
                 max_events=256):
        who = 'ContactMonitor'
        for name, v, lo, hi in (('cameras', cameras, 1, native.TRACK_MAX_CAMERAS),
                                ('max_tracks', max_tracks, 1, native.TRACK_MAX_TRACKS),
                                ('radius', radius, 0, native.CONTACT_MAX_RADIUS),
                                ('release', radius if release is None else release, radius, native.CONTACT_MAX_RELEASE),
                                ('min_frames', min_frames, 1, 255),
                                ('long_frames', long_frames, 0, native.CONTACT_MAX_LONG),
                                ('max_events', max_events, 1, native.CONTACT_MAX_EVENTS)):
            if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:   # (radius is checked before release)
                raise ValueError(f'{who}: {name} is an integer in {lo} .. {hi}, got {v!r}')
        if isinstance(max_age, bool) or int(max_age) != max_age or max_age < 0:
            raise ValueError(f'{who}: max_age is an integer >= 0, got {max_age!r}')
        self.cameras, self.max_tracks, self.max_age = cameras, max_tracks, int(max_age)
        self.radius, self.release = radius, radius if release is None else release
        self.min_frames, self.long_frames, self.max_events = min_frames, long_frames, max_events
        self._state = None

    def _allocate(self, dev):
        C, S = self.cameras, self.max_tracks
        z = dict(dtype=torch.int32, device=dev)
        self._state = dict(id=torch.zeros((C, S), **z), last=torch.zeros((C, S), **z), pos=torch.zeros((C, S, 2), **z),
                           link=torch.zeros((C, S, S), **z), since=torch.zeros((C, S, S), **z),
                           frame=torch.zeros((C,), **z), dropped=torch.zeros((C,), **z),
                           counters=torch.zeros((C, native.CONTACT_COUNTER_WORDS), **z))

    def _items(self, items, who):
        """The (on, xy, ids, camera) entries of (camera, placed, ids) items, with the state allocated on their device;
        [] for no items.  The items are not results, so this is not `Tracked._entries`."""
        if any(not (isinstance(it, (tuple, list)) and len(it) == 3) for it in items):
            raise ValueError(f'{who}: items are (camera, placed, ids) triples')
        if not items:
            return []
        entries = []
        for i, (camera, placed, ids) in enumerate(items):
            camera = self._camera(camera, who)
            if not (isinstance(placed, dict) and isinstance(placed.get('on'), torch.Tensor)
                    and isinstance(placed.get('xy'), torch.Tensor)):
                raise ValueError(f"{who}: placed[{i}] is the dict GroundPlane.update returned: it holds the tensors on and xy")
            on, xy = placed['on'], placed['xy']
            if on.dtype != torch.int32 or on.dim() != 1:
                raise ValueError(f'{who}: on of placed[{i}] must be an int32 [N] tensor')
            N = on.shape[0]
            if xy.dtype != torch.int32 or tuple(xy.shape) != (N, 2):
                raise ValueError(f'{who}: xy of placed[{i}] must be an int32 [{N}, 2] tensor')
            if N > native.TRACK_MAX_POSES:
                raise ValueError(f'{who}: placed[{i}] has {N} poses, at most {native.TRACK_MAX_POSES}')
            if not (isinstance(ids, torch.Tensor) and ids.dtype == torch.int32 and tuple(ids.shape) == (N,)):
                raise ValueError(f'{who}: ids of placed[{i}] must be an int32 [{N}] tensor')
            if not (on.is_cuda and xy.is_cuda and ids.is_cuda):
                raise ValueError(f'{who}: placed[{i}] and its ids must be HIP device tensors (pavenet_amd has no CPU '
                                 'path)')
            entries.append((on.contiguous(), xy.contiguous(), ids.contiguous(), camera))
        dev = entries[0][0].device
        if self._state is not None and self._state['id'].device != dev:
            raise ValueError(f"{who}: {self._NOUNS} state is on {self._state['id'].device}, placed[0] on {dev}")
        if self._state is None:
            self._allocate(dev)
        return entries

    def update_many(self, items):
        """items: (camera, placed, ids) triples, the entries of one camera in time order; placed is the dict
        `GroundPlane.update` returned (only its `on` [N] and `xy` [N, 2] int32 device tensors are read), ids the
        tracker's [N] int32 -> one dict per item of new int32 device tensors: group [N] (the smallest track id of the
        pose's party), size [N] (the tracks in it; 1 alone), contacts [N] (how many it is in contact with), partner [N]
        (the id of its oldest contact, the lower slot on a tie, or 0), together [N] (frames since that contact began,
        or 0) -- all 0 for a pose without a slot -- events [max_events, 7] (rows (kind, a, b, frames, pose_a, pose_b,
        frame), a < b the two ids, pose_* their rows in this frame or -1; zero past the count) and n_events (0-d: all
        events of the frame, stored or not).  One launch per 32 items on the current stream; no host copy, no sync."""
        entries = self._items(list(items), 'ContactMonitor.update')
        if not entries:
            return []
        return ops.contact_update(entries, self._state, radius=self.radius, release=self.release,
                                  min_frames=self.min_frames, long_frames=self.long_frames,
                                  max_events=self.max_events, max_age=self.max_age)

    def update(self, placed, ids, camera=0):
        """One frame of `camera` -> dict(group=, size=, contacts=, partner=, together=, events=, n_events=)."""
        return self.update_many([(camera, placed, ids)])[0]

    def reset(self, camera=None):
        """Frees the slots of `camera` (None: of every camera) without events; its frame count, drop count and counters
        restart at 0.  The state tensors stay where they are: a birth zeroes the pair words of its slot, and the words
        of a free slot are never read."""
        self._reset(camera)

    def counts(self, camera=0):
        """Views of one camera's counters on the device (0-d): contacts (the pairs in contact now = meets - parts),
        meets, parts, longs (running), groups (the parties of two or more), grouped (the tracks in them), largest (the
        largest party, 1 when everybody is alone, 0 with nobody there).  None before the first call."""
        camera = self._camera(camera, 'ContactMonitor.counts')
        if self._state is None:
            return None
        row = self._state['counters'][camera]
        return {name: row[at] for name, at in _C.items()}

    def pairs(self, camera=0):
        """Views of one camera's pair words on the device, [S, S], the pair of slots s < t at [s, t]: link (bit 0: in
        contact, bits 8 ..: the frames in a row the distance test has disagreed with it) and since (the frame the
        contact began, 0 without one).  A word means something only while both slots are live.  None before the first
        call."""
        return self._views(camera, 'pairs', ('link', 'since'))

    def state(self, camera=0):
        """Views of one camera's slots on the device: id, last [S] (id 0 = free slot; its other fields mean nothing),
        pos [S, 2] (mm), frame, dropped (0-d).  None before the first call."""
        return self._views(camera, 'state', _STATE)


def events_to_list(out):
    """The events of one `update` as a list of dict(kind=, a=, b=, frames=, pose_a=, pose_b=, frame=) on the host, kind
    one of 'meet', 'part', 'long', a < b the two track ids, frames how long the contact has lasted, pose_* the rows of
    the two in this frame (-1 where a track was not seen).  THE host copy of this module: it reads n_events and the
    table from the device, which waits for the stream.  Only the rows that were stored are listed (`out['n_events']`
    may be larger)."""
    n = min(int(out['n_events']), out['events'].shape[0])
    return [dict(kind=KINDS[k], a=a, b=b, frames=fr, pose_a=pa, pose_b=pb, frame=f)
            for k, a, b, fr, pa, pb, f in out['events'][:n].tolist()]
