"""Contacts and groups on the device (csrc/pave_contacts.hip, pave_contact_update) against the rule of DESIGN section 24
in numpy (tests/contact_ref.py): after every frame every output, every counter, the slot state (live slots), the pair
words (pairs of two live slots) are compared with the oracle by torch.equal, and the inputs with what they were.  Needs
an MI355X."""
import numpy as np
import pytest
import torch

from tests import contact_cases as CC
from tests import contact_ref as CR
from tests import floor_ref as FR

pytestmark = pytest.mark.gpu


class Pair:
    """A ContactMonitor and the oracle, configured alike."""

    def __init__(self, **kw):
        from pavenet_amd import ContactMonitor
        self.mon, self.ref = ContactMonitor(**kw), CR.ContactRef(**kw)


def same(got, exp, what):
    g, e = got.detach().cpu(), torch.from_numpy(np.array(exp))
    assert g.dtype == torch.int32 and e.dtype == torch.int32 and g.shape == e.shape, (what, g.dtype, tuple(g.shape), tuple(e.shape))
    assert torch.equal(g, e), f'{what}: {int((g != e).sum())} words differ, first at {(g != e).nonzero()[:4].tolist()}: ' \
                              f'{g[g != e][:4].tolist()} for {e[g != e][:4].tolist()}'


def same_outputs(got, exp, what):
    assert sorted(got) == sorted(CR.OUTPUTS)
    for name in CR.OUTPUTS:
        assert got[name].is_cuda
        same(got[name], exp[name], f'{what}: {name}')


def same_all(p, cameras, what):
    """The slots of the oracle that are live and the words of the pairs of two of them; the counters whole."""
    for c in cameras:
        got, exp = p.mon.state(c), p.ref.state(c)
        assert list(got) == list(CR.STATE)
        live = exp['id'] != 0
        for name in CR.STATE:
            g, e = got[name], np.asarray(exp[name])
            if e.ndim >= 1 and name != 'id':
                g, e = g[torch.from_numpy(live).to(g.device)], e[live]
            same(g, e, f'{what}: camera {c} state {name}')
        both = np.triu(live[:, None] & live[None, :], 1)
        got, exp = p.mon.pairs(c), p.ref.pairs(c)
        assert list(got) == list(CR.PAIRS)
        for name in CR.PAIRS:
            same(got[name][torch.from_numpy(both).to(got[name].device)], exp[name][both], f'{what}: camera {c} pairs {name}')
        got, exp = p.mon.counts(c), p.ref.counts(c)
        assert list(got) == list(CR.COUNTS)
        for name in CR.COUNTS:
            same(got[name], exp[name], f'{what}: camera {c} counter {name}')
        assert int(exp['contacts']) == int(exp['meets']) - int(exp['parts'])


def device(on, xy, ids):
    return (dict(on=torch.from_numpy(np.ascontiguousarray(on, np.int32)).cuda(),
                 xy=torch.from_numpy(np.ascontiguousarray(xy, np.int32).reshape(-1, 2)).cuda()),
            torch.from_numpy(np.ascontiguousarray(ids, np.int32)).cuda())


def step(p, xy, ids, what, on=None, camera=0):
    """One frame through the device and the reference; everything compared, the inputs included.  Returns the oracle's
    outputs and the device's."""
    xy = np.asarray(xy, np.int64).reshape(-1, 2).astype(np.int32)
    ids = np.asarray(ids, np.int64).astype(np.int32)
    on = np.ones(len(xy), np.int32) if on is None else np.asarray(on, np.int32)
    exp = p.ref.update(on, xy, ids, camera)
    placed, dev_ids = device(on, xy, ids)
    before = [t.clone() for t in (placed['on'], placed['xy'], dev_ids)]
    got = p.mon.update(placed, dev_ids, camera=camera)
    same_outputs(got, exp, what)
    same_all(p, [camera], what)
    for t, b in zip((placed['on'], placed['xy'], dev_ids), before):
        assert torch.equal(t, b), f'{what}: an input changed'
    return exp, got


@pytest.mark.parametrize('script', CC.SCRIPTS, ids=lambda s: s.__name__)
def test_hand_worked_scripts_on_the_device(script):
    class Harness:
        def __init__(self, **kw):
            self.p = Pair(**kw)
            self.frames = 0

        def frame(self, xy, ids, on=None, camera=0):
            self.frames += 1
            _, got = step(self.p, xy, ids, f'{script.__name__} frame {self.frames}', on, camera)
            return {name: got[name].cpu().numpy() for name in CR.OUTPUTS}

        def counts(self, camera=0):
            return {k: int(v) for k, v in self.p.mon.counts(camera).items()}

        def get(self, field, camera=0):
            return self.p.mon.state(camera)[field].cpu().numpy()

        def pair(self, field, camera=0):
            return self.p.mon.pairs(camera)[field].cpu().numpy()
    script(Harness)


@pytest.mark.parametrize('max_tracks', [1, 2, 128])
def test_no_pose_one_two_and_128_poses_with_drops(max_tracks):
    """N = 0 (the clock still runs), 1, 2 and then 128 poses with 128 ids on a 16 x 8 grid of 1 m for three frames:
    max_tracks 1 (no pair exists) and 2 drop all but the first ids, 128 holds them all; 129 poses are refused."""
    rng = np.random.default_rng(261)
    p = Pair(max_tracks=max_tracks, radius=1000, min_frames=2, max_events=512)
    exp, _ = step(p, [], [], 'N = 0')
    assert exp['group'].shape == (0,) and p.ref.frame[0] == 1 and int(p.mon.state(0)['frame']) == 1
    step(p, [(100, 100)], [9], 'N = 1')
    step(p, [(100, 100), (600, 100)], [9, 3], 'N = 2')
    grid = np.stack([1000 * (np.arange(128) % 16), 1000 * (np.arange(128) // 16)], 1)
    for f in range(3):
        order = rng.permutation(128)
        exp, _ = step(p, grid[order] + 5 * f, np.arange(1, 129)[order], f'N = 128 frame {f}')
    assert (p.ref.id[0] != 0).sum() == max_tracks and (p.ref.dropped[0] > 0) == (max_tracks < 128)
    if max_tracks == 128:      # the 15 x 8 + 16 x 7 edges of the grid met in the second of these frames
        assert p.ref.counts(0)['meets'] == 232 and p.ref.counts(0)['largest'] == 128
    if max_tracks == 1:
        assert p.ref.counts(0)['meets'] == 0 and p.ref.counts(0)['largest'] == 1
    placed, ids = device(np.ones(129), np.zeros((129, 2)), np.arange(129))
    with pytest.raises(ValueError, match='at most 128'):
        p.mon.update(placed, ids)


def test_a_chain_of_128_whose_smallest_id_is_in_the_last_slot():
    """Pose i has id 128 - i and stands at x = 1000 i: 127 contacts in a row, one component of 128 whose name, id 1,
    sits in slot 127 and has to travel 127 hops.  max_events 100 < 127: the table is full and n_events says so."""
    p = Pair(radius=1000, min_frames=1, max_events=100)
    xy = np.stack([1000 * np.arange(128), np.zeros(128, np.int64)], 1)
    exp, _ = step(p, xy, 128 - np.arange(128), 'the chain')
    assert int(exp['n_events']) == 127 and (exp['events'][:, 0] == CR.MEET).all()
    assert (exp['group'] == 1).all() and (exp['size'] == 128).all() and exp['contacts'].tolist() == [1] + [2] * 126 + [1]
    c = p.ref.counts(0)
    assert (c['contacts'], c['groups'], c['grouped'], c['largest']) == (127, 1, 128, 128)
    xy[64, 1] = 5000                       # the middle steps out: two chains of 64 and 63
    exp, _ = step(p, xy, 128 - np.arange(128), 'the chain cut')
    assert int(exp['n_events']) == 2 and sorted(set(exp['size'].tolist())) == [1, 63, 64]
    assert exp['group'][:64].tolist() == [65] * 64 and exp['group'][65:].tolist() == [1] * 63 and exp['group'][64] == 64


def test_the_release_threshold_is_its_own():
    """radius 1000, release 1500, min_frames 1: met at 1000; (900, 1200) apart is still near, (901, 1200) is not."""
    p = Pair(radius=1000, release=1500, min_frames=1)
    exp, _ = step(p, [(0, 0), (600, 800), (9000, 0), (9600, 801)], [1, 2, 3, 4], 'meet')
    assert exp['events'][:int(exp['n_events']), :3].tolist() == [[CR.MEET, 1, 2]]
    exp, _ = step(p, [(0, 0), (900, 1200), (9000, 0), (9600, 800)], [1, 2, 3, 4], 'on release')
    assert exp['events'][:int(exp['n_events']), :3].tolist() == [[CR.MEET, 3, 4]]
    exp, _ = step(p, [(0, 0), (901, 1200), (9000, 0), (9900, 1200)], [1, 2, 3, 4], 'past release')
    assert exp['events'][:int(exp['n_events']), :4].tolist() == [[CR.PART, 1, 2, 2]]


def frames_for(rng, cams):
    spots = rng.integers(-2000, 2000, (8, 2))
    frames = []
    for cam in cams:
        n = int(rng.integers(3, 8))
        spots += rng.integers(-300, 301, spots.shape)
        who = rng.permutation(8)[:n]                             # an id of 0 among them now and then
        frames.append((cam, (rng.uniform(size=n) < 0.9).astype(np.int32), spots[who].astype(np.int32), who.astype(np.int32)))
    return frames


def test_three_cameras_in_33_entries_of_two_launches():
    """update_many with 33 entries: camera 0 five times, cameras 1 and 2 fourteen times each, interleaved.  Against the
    same frames in single calls on a second object; the oracle runs beside both."""
    from pavenet_amd import ContactMonitor
    rng = np.random.default_rng(262)
    kw = dict(cameras=3, max_age=1, max_tracks=6, radius=1500, release=2000, min_frames=1, long_frames=2, max_events=8)
    many, single = Pair(**kw), ContactMonitor(**kw)
    cams = [0 if i % 7 == 0 else 1 + i % 2 for i in range(33)]
    frames = frames_for(rng, cams)
    items = [(cam,) + device(on, xy, ids) for cam, on, xy, ids in frames]
    outs = many.mon.update_many(items)
    assert len(outs) == 33
    kinds = set()
    for i, ((cam, on, xy, ids), item, out) in enumerate(zip(frames, items, outs)):
        exp = many.ref.update(on, xy, ids, cam)
        same_outputs(out, exp, f'entry {i}')
        same_outputs(single.update(item[1], item[2], camera=cam), exp, f'entry {i} alone')
        kinds |= set(exp['events'][:, 0].tolist())
    same_all(many, [0, 1, 2], 'after 33 entries')
    assert many.ref.frame.tolist() == [5, 14, 14] and kinds == {0, CR.MEET, CR.PART, CR.LONG}
    for cam in range(3):
        for name in CR.COUNTS:
            assert torch.equal(many.mon.counts(cam)[name], single.counts(cam)[name]), name
        assert torch.equal(many.mon.state(cam)['id'], single.state(cam)['id'])


def test_reset_of_one_camera_and_a_side_stream():
    """reset(camera=1) frees camera 1's slots and zeroes its counters, and leaves camera 0's tensors and every data_ptr
    as they were; the stale pair words of camera 1 do no harm, since a birth zeroes them; frames on a side stream are
    counted on that stream."""
    p = Pair(cameras=2, max_tracks=4, radius=1500, min_frames=1)
    for cam in (0, 1):
        for f in range(2):
            step(p, [(0, 0), (1000, 0), (2000, 50 * f)], [1, 2, 3], f'camera {cam} frame {f}', camera=cam)
    assert p.ref.counts(1)['contacts'] == 2
    ptrs = {k: v.data_ptr() for k, v in p.mon._state.items()}
    zero = {k: v[0].clone() for k, v in p.mon._state.items()}
    p.mon.reset(camera=1)
    p.ref.reset(1)
    assert {k: v.data_ptr() for k, v in p.mon._state.items()} == ptrs
    for k, v in zero.items():
        assert torch.equal(p.mon._state[k][0], v), k
    for k in ('id', 'frame', 'dropped', 'counters'):
        assert not p.mon._state[k][1].any(), k
    assert p.mon._state['link'][1].any()               # (stale, and never read)
    same_all(p, [0, 1], 'after reset(1)')
    exp, _ = step(p, [(0, 0), (5000, 0), (9000, 0)], [1, 2, 3], 'camera 1 after its reset: far apart', camera=1)
    assert int(exp['n_events']) == 0 and p.ref.counts(1)['contacts'] == 0
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for f in range(3):
            step(p, [(0, 0), (1000 + 400 * f, 0)], [1, 2], f'side stream frame {f}', camera=0)
    torch.cuda.current_stream().wait_stream(side)
    assert p.ref.frame.tolist() == [5, 1] and p.ref.counts(0)['parts'] >= 1
    p.mon.reset()
    p.ref.reset()
    same_all(p, [0, 1], 'after reset()')


def test_forty_random_frames():
    """0 .. 128 poses a frame for 40 frames: ids drawn from 1 .. 140 with repeats, zeros and negatives, on flags at
    random, positions past the floor now and then, 96 slots so that some poses drop, a short max_age so that contacts
    expire, a table that overflows."""
    rng = np.random.default_rng(263)
    p = Pair(max_tracks=96, max_age=2, radius=900, release=1200, min_frames=2, long_frames=5, max_events=6)
    walkers = rng.integers(-4000, 4000, (140, 2))
    events, over, kinds, biggest = 0, 0, set(), 0
    for f in range(40):
        n = int(rng.integers(0, 129)) if f % 8 else (0, 128, 1, 127, 2)[f // 8]
        who = rng.integers(-2, 141, n)
        walkers += rng.integers(-150, 151, walkers.shape)
        xy = walkers[np.clip(who, 1, 140) - 1].copy()
        xy[rng.uniform(size=n) < 0.03] *= 400                    # out of the floor: clamped
        exp, _ = step(p, xy, who, f'frame {f}', on=(rng.uniform(size=n) < 0.9).astype(np.int32))
        events += int(exp['n_events'])
        over += int(exp['n_events']) > 6
        kinds |= set(exp['events'][:, 0].tolist())
        biggest = max(biggest, int(exp['size'].max(initial=0)))
    c = p.ref.counts(0)
    assert events > 200 and over > 5 and kinds == {0, CR.MEET, CR.PART, CR.LONG} and p.ref.dropped[0] > 0
    assert c['meets'] > 50 and c['parts'] > 20 and c['longs'] > 0 and biggest >= 5


def test_a_ground_plane_on_the_device_feeds_the_monitor():
    """GroundPlane.update -> ContactMonitor.update on the device equals floor_ref -> contact_ref: twelve people walking
    under the tilted camera, six of them in pairs."""
    from pavenet_amd import GroundPlane, contacts
    from tests.test_floor_cpu import TILTED
    from tests.test_floor_gpu import marks, people
    from tests.test_track_gpu import result
    rng = np.random.default_rng(264)
    plane, plane_ref = GroundPlane(15, max_tracks=16), FR.FloorRef(15, max_tracks=16)
    plane.set_plane(0, points=marks(TILTED))
    plane_ref.set_plane(0, points=marks(TILTED))
    p = Pair(max_tracks=16, radius=300, release=400, min_frames=2, long_frames=4)
    start = np.stack([600.0 + 1100.0 * (np.arange(12) // 2) + 160.0 * (np.arange(12) % 2), 2500.0 + 700.0 * (np.arange(12) // 2)], 1)
    drift = np.repeat(rng.uniform(-25, 25, (6, 2)), 2, 0)
    drift[6:] = rng.uniform(-60, 60, (6, 2))                     # the last three pairs walk apart
    ids = np.arange(1, 13, dtype=np.int32)
    listed = []
    for f in range(10):
        kpts, bboxes = people(rng, start + drift * f)
        placed_ref = plane_ref.update(kpts, bboxes, ids)
        exp = p.ref.update(placed_ref['on'], placed_ref['xy'], ids)
        dev_ids = torch.from_numpy(ids).cuda()
        placed = plane.update(result(kpts, bboxes), dev_ids)
        same(placed['xy'], placed_ref['xy'], f'frame {f}: xy')
        got = p.mon.update(placed, dev_ids)
        same_outputs(got, exp, f'frame {f}')
        same_all(p, [0], f'frame {f}')
        listed += contacts.events_to_list(got)
    assert len(listed) == p.ref.counts(0)['meets'] + p.ref.counts(0)['parts'] + p.ref.counts(0)['longs'] >= 4
    assert {e['kind'] for e in listed} >= {'meet', 'long'} and all(e['a'] < e['b'] for e in listed)
    assert p.ref.counts(0)['groups'] >= 2


def test_updates_allocate_no_growing_memory():
    from pavenet_amd import ContactMonitor
    mon = ContactMonitor(max_events=16, min_frames=1)
    placed, ids = device([1, 1], [(0, 0), (1000, 0)], [1, 2])
    mon.update(placed, ids)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    for _ in range(100):
        out = mon.update(placed, ids)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - base <= 8 * 512     # (the one small output of a call or two)
    assert int(mon.state(0)['frame']) == 101 and out['together'].tolist() == [100, 100] and int(mon.counts(0)['meets']) == 1
