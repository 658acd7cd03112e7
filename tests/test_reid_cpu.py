"""Re-identification without a GPU: the rule of DESIGN section 18 in numpy (tests/reid_ref.py) measured on painted
scenes -- the measurement that sets the default match_thr -- its arithmetic, the plan layouts and every refusal of
the C entries and of the Python wrappers."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import reid_cases as RC
from tests import reid_ref as RR
from tests import track_ref as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEIGHTS = (40, 100, 300)
PEOPLE = 20
# What `measure` gives (the assertions below hold the numbers in place): per height the lowest score between two
# sightings of one person and the highest between two different people.
MEASURED = {40: (43913, 11860), 100: (49030, 12364), 300: (49663, 10331)}


def pair_score(qa, ca, qb, cb):
    """The rule's score of a pose (qb, cb) against a slot that holds the descriptors of one sighting (qa, ca)."""
    if ca[0] == 0 or cb[0] == 0:
        return None
    s = RR.similarity(qa[0], qb[0])
    if ca[1] > 0 and cb[1] > 0:
        s = (s + RR.similarity(qa[1], qb[1])) >> 1
    return s


def sightings(height, seed):
    """PEOPLE people of one height, seen twice: other places, other noise, a brightness shift of up to +-SHIFT and a
    tint of up to +-TINT between the two -> two dicts of describe()."""
    rng = np.random.default_rng(seed)
    shirts, trousers = RC.colours(PEOPLE, seed)
    step = int(0.4 * height) + 24
    W, H = (PEOPLE * step + 32) // 2 * 2, (height + 48) // 2 * 2
    out = []
    for sight in range(2):
        order = rng.permutation(PEOPLE)
        pos = np.stack([8.0 + step * np.argsort(order) + rng.uniform(0, 8, PEOPLE), rng.uniform(4, 40, PEOPLE)], 1)
        people = [(pos[i, 0], pos[i, 1], height, shirts[i], trousers[i]) for i in range(PEOPLE)]
        shift = 0 if sight == 0 else int(rng.choice([-RC.SHIFT, RC.SHIFT]))
        tint = (0, 0) if sight == 0 else tuple(int(v) for v in rng.choice([-RC.TINT, RC.TINT], 2))
        surface = RC.paint_nv12(rng, W, H, W + 6, people, shift, tint)
        kpts, bboxes = RC.poses15(rng, pos, height)
        out.append(RR.describe('nv12', surface, W, kpts, bboxes, K=15))
    return out


def measure(height, seeds=(1, 2, 3)):
    same, diff, legs = [], [], 0
    for seed in seeds:
        a, b = sightings(height, 1000 * height + seed)
        assert (a['count'][:, 0] > 0).all() and (b['count'][:, 0] > 0).all()
        legs += int((a['count'][:, 1] > 0).sum())
        for i in range(PEOPLE):
            for j in range(PEOPLE):
                s = pair_score(a['hist'][i], a['count'][i], b['hist'][j], b['count'][j])
                (same if i == j else diff).append(s)
    return min(same), max(diff), legs


@pytest.fixture(scope='module')
def measured():
    return {h: measure(h) for h in HEIGHTS}


def test_the_default_threshold_is_the_measured_midpoint(measured):
    """20 people x 3 seeds per height, shirts and trousers at least 32 apart in U or V, noise sigma 10 / 5, a
    brightness shift of 12 and a tint of 3: the same-person scores and the different-person scores are disjoint at
    every height, and the default is the midpoint between the lowest of the first and the highest of the second."""
    from pavenet_amd import reid
    for h in HEIGHTS:
        lo_same, hi_diff, legs = measured[h]
        print(f'height {h}: lowest same-person score {lo_same}, highest different-person score {hi_diff}, '
              f'{legs} of {3 * PEOPLE} first sightings with valid legs')
        assert (lo_same, hi_diff) == MEASURED[h]
        assert hi_diff < reid.DEFAULT_MATCH_THR <= lo_same
    lo, hi = min(m[0] for m in measured.values()), max(m[1] for m in measured.values())
    assert lo > hi
    assert reid.DEFAULT_MATCH_THR == (lo + hi) // 2


def frames_of(script, height, seed, W=960, H=400):
    """script: per frame a list of (person, x, y) -> per frame (surface, kpts, bboxes): painted NV12 frames with
    their poses, a new brightness shift and tint every frame."""
    rng = np.random.default_rng(seed)
    shirts, trousers = RC.colours(4, seed)
    for there in script:
        pos = np.asarray([(x, y) for _, x, y in there], np.float64).reshape(-1, 2)
        people = [(x, y, height, shirts[p], trousers[p]) for p, x, y in there]
        shift, tint = int(rng.integers(-RC.SHIFT, RC.SHIFT + 1)), tuple(int(v) for v in rng.integers(-RC.TINT, RC.TINT + 1, 2))
        kpts, bboxes = RC.poses15(rng, pos, height)
        yield RC.paint_nv12(rng, W, H, W, people, shift, tint), kpts, bboxes


def run(script, height, seed, **kw):
    """The numpy tracker (plain, max_age 30) and the numpy gallery over a script -> per frame (track ids, person ids)."""
    from pavenet_amd import reid
    tracker = TR.TrackRef(15, max_age=30)
    gallery = RR.ReIDRef(15, default_thr=reid.DEFAULT_MATCH_THR, **kw)
    out = []
    for surface, kpts, bboxes in frames_of(script, height, seed):
        ids = tracker.update(kpts, bboxes)
        out.append((ids.copy(), gallery.update('nv12', surface, 960, kpts, bboxes, ids)['ids']))
    return out


GAP = 30 + 10      # the tracker's max_age and ten frames more


@pytest.mark.parametrize('height', HEIGHTS)
def test_a_hidden_person_comes_back_under_the_same_person_id(height):
    """Person 0 walks, is hidden for max_age + 10 frames and comes back somewhere else, while person 1 stands by: a
    new track id and the same person id, in 3 of 3 seeded cases per height."""
    for seed in (1, 2, 3):
        script = [[(0, 100 + 4 * f, 20), (1, 600, 30)] for f in range(6)] + [[(1, 600, 30)]] * GAP + \
                 [[(0, 400 + 4 * f, 40), (1, 600, 30)] for f in range(4)]
        out = run(script, height, seed)
        (t0, p0), (t1, p1) = out[5], out[-1]
        assert t1[0] != t0[0] and t1[0] >= 1 and p1[0] == p0[0] >= 1, (height, seed, t0, t1, p0, p1)
        assert t1[1] == t0[1] and p1[1] == p0[1] != p0[0]
        assert all(len(set(p.tolist())) == len(p) for _, p in out)


@pytest.mark.parametrize('height', HEIGHTS)
def test_two_people_who_return_in_the_other_order_keep_their_ids(height):
    """Two people in different colours leave; they come back in each other's places, the second first: both get
    new track ids in the other order and each keeps its own person id, in 3 of 3 seeded cases per height."""
    for seed in (1, 2, 3):
        script = [[(0, 100, 20), (1, 500, 30)] for f in range(6)] + [[]] * GAP + [[(1, 100, 20)]] * 3 + \
                 [[(1, 100, 20), (0, 500, 30)]] * 3
        out = run(script, height, seed)
        (t0, p0), (t1, p1) = out[5], out[-1]
        assert sorted(t1) == [3, 4] and sorted(t0) == [1, 2]
        assert p1[0] == p0[1] and p1[1] == p0[0] and p0[0] != p0[1], (height, seed, p0, p1)


def test_the_limit_people_dressed_alike_merge():
    """Stated, not hidden: a second person in the first one's colours takes the first one's person id once the first
    has left."""
    rng = np.random.default_rng(5)
    shirts, trousers = RC.colours(1, 5)
    from pavenet_amd import reid
    tracker, gallery = TR.TrackRef(15, max_age=2), RR.ReIDRef(15, default_thr=reid.DEFAULT_MATCH_THR)
    seen = []
    for f in range(12):
        x = 100 if f < 5 else 500
        there = [] if 5 <= f < 9 else [(x, 20, 100, shirts[0], trousers[0])]
        kpts, bboxes = RC.poses15(rng, [(x, 20)] if there else np.zeros((0, 2)), 100)
        ids = tracker.update(kpts, bboxes)
        seen.append((ids.tolist(), gallery.update('nv12', RC.paint_nv12(rng, 960, 200, 960, there), 960, kpts, bboxes, ids)['ids'].tolist()))
    assert seen[4] == ([1], [1]) and seen[-1] == ([2], [1])


def test_soft_bin_weights_sum_to_8_on_every_axis():
    c = np.arange(256)
    for n in (4, 8):
        b0, b1, w0, w1 = RR.soft_bins(c, n)
        assert ((w0 + w1) == 8).all() and (w0 >= 0).all() and (w1 >= 0).all()
        assert (b0 >= 0).all() and (b1 < n).all() and ((b1 - b0) <= 1).all()
        assert ((w1 == 0) | (b1 > b0)).all()           # the last bin is never voted for twice
        centre = 256 // n // 2
        assert w1[centre] == 0 and b0[centre] == 0 and w0[0] == 8 and w0[255] == 8 and b0[255] == n - 1


def test_a_descriptor_sums_to_almost_65536():
    rng = np.random.default_rng(3)
    for n in (16, 17, 100, 999, 1024):
        Y, U, V = (rng.integers(0, 256, n) for _ in range(3))
        h = RR.histogram(Y, U, V)
        assert h.sum() == 512 * n
        q = RR.normalise(h, n)
        assert 65536 - 256 < q.sum() <= 65536
    assert RR.stride_of(32, 32) == 1 and RR.stride_of(33, 32) == 2 and RR.stride_of(4096, 4096) == 128
    assert RR.CAP * 512 * 128 < 2 ** 31


def _gallery_scene(frames, n_people=5, seed=7, height=100, **kw):
    rng = np.random.default_rng(seed)
    shirts, trousers = RC.colours(n_people, seed)
    g = RR.ReIDRef(15, **kw)
    for there, ids in frames:
        pos = [(40 + 90 * p, 20) for p in there]
        people = [(x, y, height, shirts[p], trousers[p]) for p, (x, y) in zip(there, pos)]
        kpts, bboxes = RC.poses15(rng, pos if pos else np.zeros((0, 2)), height)
        yield g, g.update('nv12', RC.paint_nv12(rng, 512, 160, 512, people), 512, kpts, bboxes, np.asarray(ids, np.int32))


def test_a_threshold_that_never_matches_relabels_the_track_ids():
    """match_thr = 65537: track id <-> person id is a bijection, whatever the colours are."""
    frames = [([0, 1, 2], [1, 2, 3])] * 4 + [([0, 2], [1, 3])] * 2 + [([0, 1, 2], [1, 4, 3])] * 3 + [([1, 0], [4, 5])] * 2
    seen = {}
    for (there, ids), (g, out) in zip(frames, _gallery_scene(frames, match_thr=RR.NEVER)):
        assert (out['sim'] == 0).all()
        for t, p in zip(ids, out['ids'].tolist()):
            assert seen.setdefault(t, p) == p
    assert sorted(seen) == [1, 2, 3, 4, 5] and sorted(seen.values()) == [1, 2, 3, 4, 5]


def test_person_ids_are_never_reused_after_eviction_and_reset():
    frames = [([0, 1], [1, 2])] * 2 + [([2, 3], [3, 4])] * 2 + [([4], [5])]
    handed = []
    for g, out in _gallery_scene(frames, max_people=2, match_thr=RR.NEVER):
        handed.append(out['ids'].tolist())
    assert handed == [[1, 2], [1, 2], [3, 4], [3, 4], [5]]          # the lost slots were evicted, oldest first
    assert g.person[0].tolist() == [5, 4] and g.next[0] == 6
    g.reset(0)
    assert g.person[0].tolist() == [0, 0] and g.frame[0] == 0 and g.next[0] == 6
    rng = np.random.default_rng(1)
    kpts, bboxes = RC.poses15(rng, [(40, 20)], 100)
    out = g.update('nv12', RC.paint_nv12(rng, 512, 160, 512, []), 512, kpts, bboxes, [9])
    assert out['ids'].tolist() == [6]
    # all slots live: the third pose is dropped
    kpts, bboxes = RC.poses15(rng, [(40, 20), (140, 20), (240, 20)], 100)
    out = g.update('nv12', RC.paint_nv12(rng, 512, 160, 512, []), 512, kpts, bboxes, [9, 10, 11])
    assert out['ids'].tolist() == [6, 7, 0] and g.dropped[0] == 1


def test_the_class_is_exported():
    import pavenet_amd
    from pavenet_amd import reid
    assert pavenet_amd.PersonReID is reid.PersonReID
    assert reid.TORSO == RR.TORSO and reid.LEGS == RR.LEGS and reid.NEVER == RR.NEVER == 65537
    from pavenet_amd import native
    assert (native.REID_CAP, native.REID_MIN_SAMPLES, native.REID_MAX_HITS) == (RR.CAP, RR.MIN_SAMPLES, RR.MAX_HITS)


def _lib():
    from pavenet_amd import native
    from pavenet_amd.build_native import build_native
    build_native()
    return native, native.load()


ENTRIES = ('pave_reid_describe_nv12', 'pave_reid_describe_bgr', 'pave_reid_update_nv12', 'pave_reid_update_bgr')


def test_plan_layouts_and_entries(tmp_path):
    """native.ReidDescribePlan and native.ReidPlan are the header's structs field for field, under the 4 KB
    kernel-argument limit, and the entries are in the header, the binding and both libraries."""
    native, lib = _lib()
    vp, ci = ctypes.c_void_p, ctypes.c_int
    for name in ENTRIES:
        assert native.FUNCTIONS[name] == (ci, [vp, vp]) and name in native.SIGNATURES and hasattr(lib, name)
    for path in (native.LIB_PATH, native.DIAG_LIB_PATH):
        out = subprocess.run(['nm', '-D', '--defined-only', path], capture_output=True, text=True, check=True).stdout
        assert set(ENTRIES) <= {ln.split()[-1] for ln in out.splitlines()}
    assert ctypes.sizeof(native.ReidDescribePlan) == 2400 and ctypes.sizeof(native.ReidPlan) == 3392 < 4096
    assert native.ReidPlan.d.offset == 0
    if not shutil.which('gcc'):
        pytest.skip('no gcc')
    for struct, cls in (('pave_reid_describe_plan', native.ReidDescribePlan), ('pave_reid_plan', native.ReidPlan)):
        fields = [f for f, _ in cls._fields_]
        src = tmp_path / f'{struct}.c'
        src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pave_hip.h"\nint main(void) {\n'
                       f'  printf("%zu", sizeof({struct}));\n'
                       + ''.join(f'  printf(" %zu", offsetof({struct}, {f}));\n' for f in fields)
                       + '  return 0;\n}\n')
        exe = tmp_path / struct
        subprocess.run(['gcc', '-std=c99', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
        got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
        assert got[0] == ctypes.sizeof(cls)
        assert got[1:] == [getattr(cls, f).offset for f in fields]


GALLERY = ('person', 'track', 'last', 'hits', 'hist', 'frame', 'next', 'dropped')


def test_c_entries_refuse_bad_plans_before_any_device_call():
    """No GPU: every refusal is PAVE_E_ARG with a message (the addresses are never dereferenced)."""
    native, lib = _lib()
    host = (ctypes.c_ubyte * 64)()
    addr = ctypes.addressof(host)

    def plan(entries=2, n=3, K=15, W=64, H=48, pitch=None, scale=(1.0, 1.0), src=addr, kpts=addr, bboxes=addr, d_hist=addr,
             count=addr, torso=((3, 4), (9, 10)), ids=addr, out_ids=addr, out_sim=addr, camera=1, cameras=2, S=8,
             max_lost=900, match_thr=30000, min_hits=3, gain=2, pairs=addr, bgr=False, **state):
        p = native.ReidPlan()
        for i in range(min(max(entries, 0), 32)):
            p.d.src[i], p.d.kpts[i], p.d.bboxes[i], p.d.hist[i], p.d.count[i] = src, kpts, bboxes, d_hist, count
            p.d.pitch[i] = (3 * W if bgr else W) if pitch is None else pitch
            p.d.width[i], p.d.height[i], p.d.n[i], p.d.scale[i][0], p.d.scale[i][1] = W, H, n, scale[0], scale[1]
            p.ids[i], p.out_ids[i], p.out_sim[i], p.camera[i] = ids, out_ids, out_sim, camera
        for r, region in enumerate((torso, ((9, 10), (11, 12)))):
            for h, half in enumerate(region):
                p.d.n_part[r][h] = len(half)
                for i, k in enumerate(half[:4]):
                    p.d.part[r][h][i] = k
        p.d.entries, p.d.K, p.d.score_thr, p.d.kpt_thr = entries, K, 0.3, 0.0
        for f in GALLERY:
            setattr(p, f, state.get(f, addr))
        p.pairs, p.cameras, p.S, p.max_lost, p.match_thr, p.min_hits, p.gain = pairs, cameras, S, max_lost, match_thr, \
            min_hits, gain
        return p

    def refused(needle, update_only=False, bgr=False, **kw):
        p = plan(bgr=bgr, **kw)
        calls = [(lib.pave_reid_update_bgr if bgr else lib.pave_reid_update_nv12, ctypes.byref(p))]
        if not update_only:
            calls.append((lib.pave_reid_describe_bgr if bgr else lib.pave_reid_describe_nv12, ctypes.byref(p.d)))
        for fn, arg in calls:
            assert fn(arg, None) == native.DEFINES['PAVE_E_ARG'] == -1
            assert needle in lib.pave_last_error().decode(), lib.pave_last_error()

    for name in ENTRIES:
        assert getattr(lib, name)(None, None) == -1 and 'null plan' in lib.pave_last_error().decode()
    for bgr in (False, True):
        refused('entries per launch', bgr=bgr, entries=0)
        refused('entries per launch', bgr=bgr, entries=33)
        refused('K outside', bgr=bgr, K=0)
        refused('K outside', bgr=bgr, K=33)
        refused('null surface', bgr=bgr, src=None)
        refused('null hist or count', bgr=bgr, d_hist=None)
        refused('null hist or count', bgr=bgr, count=None)
        refused('null pose', bgr=bgr, kpts=None)
        refused('null pose', bgr=bgr, bboxes=None)
        refused('N outside', bgr=bgr, n=-1)
        refused('N outside', bgr=bgr, n=129)
        refused('width or height', bgr=bgr, W=0)
        refused('width or height', bgr=bgr, W=8194)
        refused('width or height', bgr=bgr, H=0)
        refused('width or height', bgr=bgr, H=8194)
        refused('pitch', bgr=bgr, pitch=63)
        for bad in ((0.0, 1.0), (1.0, -1.0), (float('nan'), 1.0), (1.0, float('inf'))):
            refused('scale', bgr=bgr, scale=bad)
        refused('n_part', bgr=bgr, torso=((0, 1, 2, 3, 4), (9,)))
        refused('part key point', bgr=bgr, torso=((3, 15), (9,)))
        refused('part key point', bgr=bgr, torso=((3,), (-1,)))
        refused('part key point', bgr=bgr, K=10)
        for f in GALLERY:
            refused('null gallery', True, bgr=bgr, **{f: None})
        refused('null pairs', True, bgr=bgr, pairs=None)
        refused('null ids or output', True, bgr=bgr, ids=None)
        refused('null ids or output', True, bgr=bgr, out_ids=None)
        refused('null ids or output', True, bgr=bgr, out_sim=None)
        refused('max_people', True, bgr=bgr, S=0)
        refused('max_people', True, bgr=bgr, S=129)
        refused('cameras outside', True, bgr=bgr, cameras=0)
        refused('cameras outside', True, bgr=bgr, cameras=4097)
        refused('camera index', True, bgr=bgr, camera=-1)
        refused('camera index', True, bgr=bgr, camera=2)
        refused('max_lost', True, bgr=bgr, max_lost=-1)
        refused('match_thr', True, bgr=bgr, match_thr=-1)
        refused('match_thr', True, bgr=bgr, match_thr=65538)
        refused('min_hits', True, bgr=bgr, min_hits=0)
        refused('min_hits', True, bgr=bgr, min_hits=32768)
        refused('gain', True, bgr=bgr, gain=0)
        refused('gain', True, bgr=bgr, gain=17)
    refused('odd NV12', W=63)
    refused('odd NV12', H=47)
    refused('pitch', bgr=True, pitch=200)      # a BGR picture is dense


def test_constructor_refusals():
    from pavenet_amd.reid import PersonReID
    for kw, needle in ((dict(K=0), 'K is'), (dict(K=33), 'K is'), (dict(K=True), 'K is'), (dict(cameras=0), 'cameras'),
                       (dict(cameras=4097), 'cameras'), (dict(max_people=0), 'max_people'), (dict(max_people=129), 'max_people'),
                       (dict(max_people=8.0), 'max_people'), (dict(max_lost=-1), 'max_lost'), (dict(max_lost=1.5), 'max_lost'),
                       (dict(match_thr=-1), 'match_thr'), (dict(match_thr=65538), 'match_thr'), (dict(match_thr=0.5), 'match_thr'),
                       (dict(min_hits=0), 'min_hits'), (dict(min_hits=32768), 'min_hits'), (dict(gain=0), 'gain'),
                       (dict(gain=17), 'gain'), (dict(K=5), 'needs torso= and legs='),
                       (dict(K=5, torso=((0,), (1,))), 'needs torso= and legs='),
                       (dict(torso=(0, 1)), 'torso is an'), (dict(torso=((0,), (1,), (2,))), 'torso is an'),
                       (dict(torso=((), (1,))), 'a part of torso'), (dict(legs=((0, 1, 2, 3, 4), (1,))), 'a part of legs'),
                       (dict(legs=((0,), (15,))), 'key points of legs'), (dict(legs=((0,), (1.0,))), 'key points of legs')):
        args = dict(K=15)
        args.update(kw)
        with pytest.raises(ValueError, match=needle):
            PersonReID(**args)
    r = PersonReID(5, torso=((0, 1), (2,)), legs=((2,), (3, 4)))
    assert r.torso == ((0, 1), (2,)) and r.legs == ((2,), (3, 4)) and r.match_thr == PersonReID(17).match_thr


def test_wrappers_raise_value_errors_on_host_tensors():
    """Shape, type and range checks, and the host-tensor check itself, are ValueErrors raised before anything is
    allocated on or asked of a device."""
    from pavenet_amd import native, ops
    from pavenet_amd.reid import PersonReID
    kp, bb, keep = torch.zeros(3, 15, 3), torch.zeros(3, 5), torch.ones(3, dtype=torch.int32)
    ids = torch.ones(3, dtype=torch.int32)
    res = (bb, None, kp)
    surf, img = torch.zeros(72, 64, dtype=torch.uint8), torch.zeros(48, 64, 3, dtype=torch.uint8)
    g = PersonReID(15, cameras=2)
    for call, needle in (
            (lambda: g.update_nv12(surf, 64, (bb, kp), ids), 'tuple'),
            (lambda: g.update_nv12(surf, 64, dict(bboxes=bb), ids), 'bboxes and kpts'),
            (lambda: g.update_nv12(surf, 64, (bb[:2], None, kp), ids), 'bboxes'),
            (lambda: g.update_nv12(surf, 64, (bb.double(), None, kp), ids), 'float32'),
            (lambda: g.update_nv12(surf, 64, dict(bboxes=bb, kpts=kp, keep=keep.long()), ids), 'int32'),
            (lambda: g.update_nv12(surf, 64, (torch.zeros(129, 5), None, torch.zeros(129, 15, 3)),
                                   torch.zeros(129, dtype=torch.int32)), 'at most 128'),
            (lambda: g.update_nv12(surf, 64, (bb, None, torch.zeros(3, 17, 3)), ids), 'K = 17'),
            (lambda: g.update_nv12(surf, 64, res, ids.long()), 'ids of results'),
            (lambda: g.update_nv12(surf, 64, res, ids[:2]), 'ids of results'),
            (lambda: g.update_nv12(surf, 64, res, [1, 2, 3]), 'ids of results'),
            (lambda: g.update_nv12(surf, 64, res, ids, camera=2), 'camera'),
            (lambda: g.update_nv12(surf, 64, res, ids, camera=0.5), 'camera'),
            (lambda: g.update_nv12(surf, 64, res, ids, scale_factor=0.0), 'positive'),
            (lambda: g.update_nv12(surf, 64.0, res, ids), 'width is an integer'),
            (lambda: g.update_nv12(surf.numpy(), 64, res, ids), 'uint8 tensor'),
            (lambda: g.update_many_nv12([(0, surf, 64, res, ids)] * 2, scale_factor=[1.0, 1.0, 1.0]), 'scale_factor'),
            (lambda: g.update_many_nv12([(0, surf, 64, res)]), 'tuples'),
            (lambda: g.update_many_bgr([(0, img, 64, res, ids)]), 'tuples'),
            (lambda: g.update_nv12(surf, 64, res, ids), 'HIP device'),
            (lambda: g.update_bgr(img, res, ids), 'HIP device'),
            (lambda: g.describe_nv12(surf, 64, res), 'HIP device'),
            (lambda: g.describe_bgr(img, res), 'HIP device'),
            (lambda: g.describe_nv12([surf, surf], 64, [res]), 'one result per surface'),
            (lambda: g.describe_nv12([], 64, []), 'non-empty'),
            (lambda: g.describe_nv12([surf, surf], [64], [res, res]), 'width'),
            (lambda: g.reset(camera=2), 'camera'),
            (lambda: g.state(2), 'camera')):
        with pytest.raises(ValueError, match=needle):
            call()
    assert g._state is None and g.state(0) is None and g.update_many_nv12([]) == [] and g.kind is None
    g.reset()
    g.kind = 'bgr'                               # a gallery that has seen BGR pictures
    with pytest.raises(ValueError, match='one kind'):
        g.update_nv12(surf, 64, res, ids)
    g.kind = 'nv12'
    with pytest.raises(ValueError, match='one kind'):
        g.update_bgr(img, res, ids)

    parts = ((3, 4), (9, 10)), ((9, 10), (11, 12))

    def state(cameras=2, S=8, **over):
        z = dict(dtype=torch.int32)
        s = dict(person=torch.zeros(cameras, S, **z), track=torch.zeros(cameras, S, **z), last=torch.zeros(cameras, S, **z),
                 hits=torch.zeros(cameras, S, 2, **z), hist=torch.zeros(cameras, S, 2, 256, **z),
                 frame=torch.zeros(cameras, **z), next=torch.ones(cameras, **z), dropped=torch.zeros(cameras, **z))
        s.update(over)
        return s
    scratch = ops.reid_scratch('meta')

    def update(entries=((surf, 64, kp, bb, None, (1.0, 1.0), ids, 0),), st=None, kind='nv12', K=15, parts=parts, sc=scratch,
               match_thr=30000, **kw):
        return ops.reid_update(kind, entries, state() if st is None else st, sc, K, parts, match_thr=match_thr, **kw)

    def entry(**over):
        e = dict(surface=surf, width=64, kpts=kp, bboxes=bb, keep=None, scale=(1.0, 1.0), ids=ids, camera=0)
        e.update(over)
        return [tuple(e.values())]
    for call, needle in (
            (lambda: update(st=dict(person=bb)), 'state holds'),
            (lambda: update(st=state(person=torch.zeros(2, 8, 1, dtype=torch.int32))), 'state person'),
            (lambda: update(st=state(S=129)), 'S in'),
            (lambda: update(st=state(hits=torch.zeros(2, 8, 2))), 'state hits'),
            (lambda: update(st=state(hist=torch.zeros(2, 8, 2, 255, dtype=torch.int32))), 'state hist'),
            (lambda: update(st=state(next=torch.zeros(3, dtype=torch.int32))), 'state next'),
            (lambda: update(match_thr=65538), 'match_thr'),
            (lambda: update(match_thr=0.5), 'match_thr'),
            (lambda: update(min_hits=0), 'min_hits'),
            (lambda: update(gain=17), 'gain'),
            (lambda: update(max_lost=-1), 'max_lost'),
            (lambda: update(kind='rgb'), 'kind'),
            (lambda: update(K=33), 'K must be'),
            (lambda: update(K=15.0), 'K must be'),
            (lambda: update(parts=(parts[0],)), 'parts is'),
            (lambda: update(parts=(((0, 1, 2, 3, 4), (9,)), parts[1])), 'a part holds'),
            (lambda: update(parts=(((3,), (15,)), parts[1])), 'a part holds'),
            (lambda: update(entries=[(surf, 64, kp, bb, None, (1.0, 1.0), ids)]), 'an entry is'),
            (lambda: update(entries=entry(surface=surf.float())), 'surface 0 must be a uint8'),
            (lambda: update(entries=entry(surface=surf[:71])), 'rows'),
            (lambda: update(entries=entry(width=63)), 'even'),
            (lambda: update(entries=entry(width=66)), 'exceeds the pitch'),
            (lambda: update(entries=entry(surface=img)), r'\[H \* 3 // 2, pitch\]'),
            (lambda: update(kind='bgr', entries=entry(surface=surf)), r'\[H, W, 3\]'),
            (lambda: update(entries=entry(kpts=kp[:, :14])), 'kpts of surface 0'),
            (lambda: update(entries=entry(bboxes=bb[:, :4])), 'bboxes of surface 0'),
            (lambda: update(entries=entry(keep=keep.long())), 'keep of surface 0'),
            (lambda: update(entries=entry(scale=(1.0, 0.0))), 'scale of surface 0'),
            (lambda: update(entries=entry(kpts=torch.zeros(129, 15, 3), bboxes=torch.zeros(129, 5),
                                          ids=torch.zeros(129, dtype=torch.int32))), 'at most 128'),
            (lambda: update(entries=entry(ids=ids.long())), 'ids of entry 0'),
            (lambda: update(entries=entry(ids=None)), 'ids of entry 0'),
            (lambda: update(entries=entry(camera=2)), 'camera of entry 0'),
            (lambda: update(sc=dict(hist=scratch['hist'])), 'scratch is'),
            (lambda: update(), 'HIP device'),
            (lambda: ops.reid_describe('nv12', [(surf, 64, kp, bb, None, (1.0, 1.0))], 15, parts), 'HIP device'),
            (lambda: ops.reid_describe('nv12', [], 15, parts), 'no surface')):
        with pytest.raises(ValueError, match=needle):
            call()
