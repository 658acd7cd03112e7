"""Multi-camera live video, the parts that need no GPU: the schedule of MultiLiveVideoPose replayed against row
ownership, CameraRing on host tensors, the two new entry points in header / library / binding, their host-side
refusals through the loaded library, and the Python wrappers' argument checks."""
import ctypes
import itertools

import pytest
import torch

MAX_PUSH = 3
CAMERAS = 3


def _lengths(T):
    return [1, T, 4 * T + 1]


def _push_patterns(T):
    """Lists of {camera: n} that deliver _lengths(T): every camera one frame at a time in lockstep, and a mixed
    pattern in which a camera is skipped every third round and the counts cycle through 1 .. MAX_PUSH."""
    lengths = _lengths(T)
    left = list(lengths)
    lockstep = []
    while any(left):
        lockstep.append({c: 1 for c in range(CAMERAS) if left[c]})
        left = [max(v - 1, 0) for v in left]
    yield lockstep
    left, mixed = list(lengths), []
    counts = itertools.cycle([1, MAX_PUSH, 2, MAX_PUSH, 1, 2])
    for rnd in itertools.count():
        if not any(left):
            break
        push = {}
        for c in range(CAMERAS):
            if left[c] and (rnd + c) % 3 != 2:
                push[c] = min(next(counts), left[c])
                left[c] -= push[c]
        if push:
            mixed.append(push)
    yield mixed


@pytest.mark.parametrize('T', [3, 5, 7])
def test_schedule_replayed_against_row_ownership(T):
    from pavenet_amd.live import LiveVideoPose, MultiLiveVideoPose
    from pavenet_amd.streaming import VideoPoseStream
    R, h, lengths = T - 1 + MAX_PUSH, T // 2, _lengths(T)
    patterns = list(_push_patterns(T))
    assert any(len(p) < CAMERAS for p in patterns[1]) and {n for p in patterns[1] for n in p.values()} == {1, 2, 3}
    for pushes in patterns:
        assert [sum(p.get(c, 0) for p in pushes) for c in range(CAMERAS)] == lengths
        plan = MultiLiveVideoPose.schedule(T, CAMERAS, MAX_PUSH, pushes)
        assert len(plan) == len(pushes) + 1
        owner, seen = {}, [0] * CAMERAS
        centres, windows = [[] for _ in range(CAMERAS)], [[] for _ in range(CAMERAS)]
        for step, items in enumerate(plan):
            before = list(seen)
            if step < len(pushes):
                for c, n in pushes[step].items():           # the push writes its frames first
                    for f in range(seen[c], seen[c] + n):
                        owner[c * R + f % R] = (c, f)
                    seen[c] += n
            assert [(c, ctr) for c, ctr, _, _ in items] == sorted((c, ctr) for c, ctr, _, _ in items)
            for c, ctr, fw, rw in items:
                if step < len(pushes):
                    assert c in pushes[step] and before[c] <= ctr + h < seen[c], 'the latency rule'
                assert len(fw) == len(rw) == T
                for f, r in zip(fw, rw):
                    assert r == c * R + f % R and c * R <= r < (c + 1) * R, 'a row of this camera'
                    assert owner.get(r) == (c, f), (T, pushes, step, c, ctr, fw, rw)
                centres[c].append(ctr)
                windows[c].append(fw)
        for c in range(CAMERAS):
            assert centres[c] == list(range(lengths[c])), 'every centre once, in order'
            assert windows[c] == VideoPoseStream.window_indices(lengths[c], T)
            # per camera: LiveVideoPose.schedule of that camera's pushes, rows offset by c * R
            own = [p[c] for p in pushes if c in p]
            alone = LiveVideoPose.schedule(lengths[c], T, own, max_push=MAX_PUSH)
            steps = [s for s, p in enumerate(pushes) if c in p] + [len(pushes)]
            assert len(alone) == len(steps)
            for s, (cs, frames, slots) in zip(steps, alone):
                mine = [it for it in plan[s] if it[0] == c]
                assert [it[1] for it in mine] == cs and [it[2] for it in mine] == frames
                assert [it[3] for it in mine] == [[c * R + v for v in w] for w in slots]
            for s in set(range(len(pushes))) - set(steps):
                assert not [it for it in plan[s] if it[0] == c], 'a camera that was not pushed emits nothing'
    for bad in ([{3: 1}], [{0: 4}], [{}], [{0: 0}]):
        with pytest.raises(ValueError):
            MultiLiveVideoPose.schedule(T, CAMERAS, MAX_PUSH, bad)


def test_camera_ring_on_host_tensors():
    """Writes land in row c * R + f % R across the wrap, in place; covers() answers per camera; reset(camera) keeps
    the tensors and the other cameras' counters; a chunk smaller than the plan consumes its share of it."""
    from pavenet_amd.live import CameraRing
    cams, R, S, C, n_pose = 3, 4, 5, 3, 3
    ring = CameraRing(cams, R)
    assert len(ring) == 0 and not ring.covers([0])

    def code(c, f):
        return float(1000 * c + f)

    def mem(entries):
        return torch.stack([torch.full((S, C), code(c, f)) for c, f in entries])

    def vals(entries):
        return [torch.stack([torch.full((S, 8, 2), code(c, f) + 0.125 * (l + 1)) for c, f in entries])
                for l in range(5)]
    seen, ptrs = [0] * cams, None
    pushes = [{0: 1, 1: 2, 2: 1}, {1: 2}, {0: 2, 2: 1}, {1: 2, 2: 2}, {0: 1, 1: 1}, {1: 2, 2: 2}, {1: 2}, {1: 1, 2: 2}]
    for step, push in enumerate(pushes):
        entries = [(c, seen[c] + j) for c in sorted(push) for j in range(push[c])]
        ring.plan(entries)
        chunk = 2 if step % 2 else len(entries)            # an encode chunk smaller than the push
        for i in range(0, len(entries), chunk):
            ring._append_memory(mem(entries[i:i + chunk]))
            assert not ring.covers([ring.row(*entries[i])]), 'memory without its values is not covered'
            ring._append_values(vals(entries[i:i + chunk]), n_pose, 0)
        ring.commit()
        for c, n in push.items():
            seen[c] += n
        assert ring.n_frames == seen and ring.n_cached == seen
        ptrs = ptrs or [t.data_ptr() for t in ring.tensors()]
        assert [t.data_ptr() for t in ring.tensors()] == ptrs and len(ptrs) == 6 and len(ring) == cams * R
        assert ring.memory.shape == (cams * R, S, C)
        for c in range(cams):
            for f in range(max(0, seen[c] - R), seen[c]):
                r = c * R + f % R
                assert (ring[r] == code(c, f)).all() and ring[r].data_ptr() == ring.memory[r].data_ptr()
                for l, v in enumerate(ring.values[0] + ring.values[1]):
                    assert v.shape == (cams * R, S, 8, 2) and (v[r] == code(c, f) + 0.125 * (l + 1)).all()
            live = [c * R + s for s in range(min(seen[c], R))]
            assert not live or ring.covers(live)
            if seen[c] < R:     # the camera's next row holds none of its frames yet, whatever its neighbours hold
                assert not ring.covers([c * R + seen[c]]) and not ring.covers(live + [c * R + seen[c]])
    assert seen[1] > 2 * R, 'camera 1 wrapped more than twice'
    assert not ring.covers([-1]) and not ring.covers([cams * R])
    assert len(ring.values[0]) == n_pose and len(ring.values[1]) == 2
    assert ring.resident_bytes() == cams * R * (S * C * 4 + 5 * S * 8 * 2 * 4)
    # reset(camera) touches that camera only
    ring.reset(1)
    assert ring.n_frames == [seen[0], 0, seen[2]] and ring.n_cached == [seen[0], 0, seen[2]]
    assert not ring.covers([R]) and ring.covers([0]) and ring.covers([2 * R])
    assert [t.data_ptr() for t in ring.tensors()] == ptrs
    ring.plan([(1, 0)])
    ring._append_memory(mem([(1, 0)]))
    ring._append_values(vals([(1, 0)]), n_pose, 0)
    assert (ring[R] == code(1, 0)).all() and ring.covers([R, 0]) and not ring.covers([R, R + 1])
    # memory only (padded metas): the write is made by commit(), and nothing is covered
    ring.plan([(0, seen[0])])
    ring._append_memory(mem([(0, seen[0])]))
    ring.values, ring.n_cached = None, 0                    # what `_encode` does after a chunk without values
    ring.commit()
    assert (ring[seen[0] % R] == code(0, seen[0])).all() and not ring.covers([R])
    assert ring.n_cached == [0, 0, 0]
    ring.reset()
    assert ring.n_frames == [0, 0, 0] and len(ring.tensors()) == 1
    # a frame that is not its camera's next, or more frames than planned, is a programming error
    ring.plan([(0, 1)])
    with pytest.raises(AssertionError):
        ring._append_memory(mem([(0, 1)]))


NEW = ('pave_scatter_rows_f32', 'pave_preprocess_surfaces_nv12')


def test_entry_points_in_header_library_and_binding():
    import subprocess
    from pavenet_amd import native
    from pavenet_amd.build_native import build_native
    build_native()
    header = open(native.HEADER_PATH).read()
    vp, ci = ctypes.c_void_p, ctypes.c_int
    assert native.FUNCTIONS['pave_scatter_rows_f32'] == (ci, [vp, vp])
    assert native.FUNCTIONS['pave_preprocess_surfaces_nv12'] == (ci, [vp, vp] + [ci] * 6 + [vp, vp, ci, vp])
    for name in NEW:
        assert name in header and name in native.SIGNATURES and name in native.EXPORTED
        assert hasattr(native.load(), name)
    for path in (native.LIB_PATH, native.DIAG_LIB_PATH):
        out = subprocess.run(['nm', '-D', '--defined-only', path], capture_output=True, text=True, check=True).stdout
        assert set(NEW) <= {ln.split()[-1] for ln in out.splitlines() if ' T ' in ln}, path
    assert native.ABI_VERSION == 21 and native.load().pave_abi_version() == 21
    # the ctypes structures have the header's capacities and the C layout
    assert (native.SCATTER_MAX_ROWS, native.SCATTER_MAX_TENSORS, native.INGEST_MAX_SURFACES) == (64, 8, 32)
    for define, value in (('PAVE_SCATTER_MAX_ROWS', 64), ('PAVE_SCATTER_MAX_TENSORS', 8),
                          ('PAVE_INGEST_MAX_SURFACES', 32)):
        assert native.DEFINES[define] == value and f'#define {define} {value}' in header
    sp, ip = native.ScatterPlan(), native.IngestPlan()
    assert (len(sp.src), len(sp.dst), len(sp.row)) == (8, 8, 64)
    assert (len(ip.src), len(ip.pitch), len(ip.csc), len(ip.csc[0])) == (32, 32, 32, 6)
    assert ctypes.sizeof(native.ScatterPlan) == 8 * 8 * 2 + 64 * 4 + 3 * 4 + 4 + 8
    assert native.ScatterPlan.row_elems.offset == 8 * 8 * 2 + 64 * 4 + 16
    assert ctypes.sizeof(native.IngestPlan) == 32 * 8 + 32 * 4 + 32 * 6 * 4 + 8 and native.IngestPlan.n.offset == 1152


def _lib():
    from pavenet_amd import native
    from pavenet_amd.build_native import build_native
    build_native()
    return native, native.load()


def _refused(native, lib, status, needle):
    assert status == native.DEFINES['PAVE_E_ARG'] == -1
    msg = lib.pave_last_error().decode()
    assert needle in msg, msg


def test_scatter_rows_host_side_refusals():
    """No GPU: every refusal is made before any device call, with PAVE_E_ARG and a message."""
    native, lib = _lib()
    # (the addresses are never dereferenced: these plans do not reach a launch)
    host = (ctypes.c_float * 1024)()
    base = (ctypes.addressof(host) + 15) & ~15

    def plan(rows=(2, 0, 1), dst_rows=3, row_elems=8, k=2, n=None, src=base, dst=base + 2048):
        p = native.ScatterPlan()
        for t in range(k if 0 < k <= 8 else 0):
            p.src[t], p.dst[t] = src, dst
        for i, r in enumerate(rows):
            p.row[i] = r
        p.n, p.k, p.dst_rows, p.row_elems = len(rows) if n is None else n, k, dst_rows, row_elems
        return p

    def call(p):
        return lib.pave_scatter_rows_f32(ctypes.byref(p), None)
    _refused(native, lib, call(plan(rows=(2, 0, 2))), 'duplicate')
    _refused(native, lib, call(plan(rows=(2, 0, 3))), 'outside')
    _refused(native, lib, call(plan(rows=(-1, 0, 1))), 'outside')
    _refused(native, lib, call(plan(row_elems=6)), 'multiple of 4')
    _refused(native, lib, call(plan(src=base + 4)), '16-byte')
    _refused(native, lib, call(plan(dst=base + 2048 + 4)), '16-byte')
    _refused(native, lib, call(plan(rows=())), 'scatter_rows')
    _refused(native, lib, call(plan(rows=tuple(range(64)), n=65, dst_rows=65)), 'scatter_rows')
    _refused(native, lib, call(plan(k=0)), 'scatter_rows')
    _refused(native, lib, call(plan(k=9)), 'scatter_rows')
    _refused(native, lib, call(plan(dst_rows=0)), 'scatter_rows')
    _refused(native, lib, call(plan(row_elems=0)), 'scatter_rows')
    p = plan()
    p.dst[1] = None
    _refused(native, lib, call(p), 'null')
    _refused(native, lib, lib.pave_scatter_rows_f32(None, None), 'null')


def test_preprocess_surfaces_host_side_refusals():
    native, lib = _lib()
    host = (ctypes.c_ubyte * 64)()
    mean, std = (ctypes.c_float * 3)(1, 2, 3), (ctypes.c_float * 3)(4, 5, 6)
    mp, sp = ctypes.cast(mean, ctypes.c_void_p), ctypes.cast(std, ctypes.c_void_p)
    dst = ctypes.addressof(host)

    def plan(n=2, pitch=64):
        p = native.IngestPlan()
        for i in range(min(max(n, 0), 32)):
            p.src[i], p.pitch[i] = ctypes.addressof(host), pitch
        p.n = n
        return p

    def call(p, H0=36, W0=50, Hn=48, Wn=67, Hp=64, Wp=96, d=dst):
        return lib.pave_preprocess_surfaces_nv12(ctypes.byref(p), d, H0, W0, Hn, Wn, Hp, Wp, mp, sp, 1, None)
    _refused(native, lib, call(plan(n=0)), 'surfaces')
    _refused(native, lib, call(plan(n=33)), 'surfaces')
    _refused(native, lib, call(plan(), W0=49), 'even')
    _refused(native, lib, call(plan(), H0=35), 'even')
    _refused(native, lib, call(plan(pitch=48)), 'pitch')
    _refused(native, lib, call(plan(), Hp=40), 'sizes')
    _refused(native, lib, call(plan(), d=None), 'null')
    p = plan()
    p.src[1] = None
    _refused(native, lib, call(p), 'null')


def test_wrapper_argument_errors_come_before_any_device_call(monkeypatch):
    from pavenet_amd import ops, preprocess

    def no_launch(*a, **k):
        raise AssertionError('a device call was made')
    monkeypatch.setattr(preprocess, '_launch', no_launch)
    monkeypatch.setattr(ops, '_launch', no_launch)
    ok = [torch.zeros(54, 64, dtype=torch.uint8), torch.zeros(54, 50, dtype=torch.uint8)]
    for surfaces, width, kw in (([], 50, {}), (ok[0], 50, {}), ([ok[0][None]], 50, {}), ([ok[0].float()], 50, {}),
                                ([torch.zeros(52, 64, dtype=torch.uint8)], 50, {}),
                                ([torch.zeros(56, 64, dtype=torch.uint8)], 50, {}),
                                ([ok[0], torch.zeros(57, 64, dtype=torch.uint8)], 50, {}),   # another source size
                                (ok, 49, {}), (ok, 52, {}),                                   # odd; beyond a pitch
                                (ok, 50, dict(matrix='bt2020')), (ok, 50, dict(matrix=['bt601'])),
                                (ok, 50, dict(full_range=[True, False, True]))):
        with pytest.raises(ValueError):
            preprocess.preprocess_surfaces_nv12(surfaces, width, **kw)
    with pytest.raises(RuntimeError, match='device'):          # host tensors with good sizes: refused, no launch
        preprocess.preprocess_surfaces_nv12(ok, 50, matrix=['bt601', 'bt709'], full_range=[False, True])

    src, dst = torch.zeros(3, 2, 4), torch.zeros(5, 2, 4)
    for srcs, dsts, rows in (([src], [dst], [0, 1, 1]), ([src], [dst], [0, 1, 5]), ([src], [dst], [0, 1, -1]),
                             ([src], [dst], [0, 1]), ([src], [dst], []), ([], [], [0]), ([src], [dst, dst], [0, 1, 2]),
                             ([src] * 9, [dst] * 9, [0, 1, 2]), ([src.double()], [dst], [0, 1, 2]),
                             ([torch.zeros(3, 6)], [torch.zeros(5, 6)], [0, 1, 2]),             # row_elems = 6
                             ([src], [torch.zeros(5, 2, 8)], [0, 1, 2]),                        # another row size
                             ([src], [torch.zeros(6 * 8 + 1)[1:].view(6, 2, 4)[:5]], [0, 1, 2])):   # address % 16 = 4
        with pytest.raises(ValueError):
            ops.scatter_rows(srcs, dsts, rows)
    with pytest.raises(RuntimeError, match='device'):
        ops.scatter_rows([src], [dst], [4, 0, 2])


def test_multi_live_video_pose_is_exported_from_the_package():
    import pavenet_amd
    from pavenet_amd.live import CameraRing, MultiLiveVideoPose
    assert pavenet_amd.MultiLiveVideoPose is MultiLiveVideoPose and pavenet_amd.CameraRing is CameraRing
