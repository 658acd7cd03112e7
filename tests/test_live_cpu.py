"""Live video, the parts that need no GPU: the ring schedule of LiveVideoPose, the NV12 colour coefficients, the
new entry point in header / library / binding, and preprocess_clip_nv12's argument checks."""
import itertools

import pytest
import torch


def _push_patterns(n_frames, max_push):
    """Pushes of one frame, and a mixed pattern 1, max_push, 2, ... cut to n_frames."""
    yield [1] * n_frames
    mixed, left = [], n_frames
    for p in itertools.cycle([1, max_push, 2, max_push, max_push, 1]):
        if left == 0:
            break
        mixed.append(min(p, left))
        left -= mixed[-1]
    yield mixed


@pytest.mark.parametrize('T', [3, 5, 7])
def test_schedule_emits_every_window_once_from_live_slots(T):
    """Centres 0 .. N - 1 once and in order, windows equal to window_indices(N, T), centre c emitted by the push
    that delivers frame c + T // 2, and no window reads a slot that was overwritten after its frame was written."""
    from pavenet_amd.live import LiveVideoPose
    from pavenet_amd.streaming import VideoPoseStream
    max_push = 3
    R = T - 1 + max_push
    for N in (1, 2, T, 4 * T + 1):
        for pushes in _push_patterns(N, max_push):
            assert sum(pushes) == N and max(pushes) <= max_push
            plan = LiveVideoPose.schedule(N, T, pushes, max_push=max_push)
            assert len(plan) == len(pushes) + 1
            owner, seen, centres, windows = {}, 0, [], []
            for step, (cs, frames, slots) in enumerate(plan):
                if step < len(pushes):
                    for f in range(seen, seen + pushes[step]):   # the push writes its frames first
                        owner[f % R] = f
                    seen += pushes[step]
                    assert all(seen - pushes[step] <= c + T // 2 < seen for c in cs), 'the latency rule'
                assert len(cs) == len(frames) == len(slots)
                for fw, sw in zip(frames, slots):
                    assert len(fw) == len(sw) == T
                    for f, s in zip(fw, sw):
                        assert s == f % R and owner.get(s) == f, (N, T, pushes, step, fw, sw)
                centres += cs
                windows += frames
            assert centres == list(range(N))
            assert windows == VideoPoseStream.window_indices(N, T)
    # the default ring is as large as the largest push needs
    assert LiveVideoPose.schedule(5, 3, [2, 2, 1])[0][2] == [[0, 0, 1]]
    with pytest.raises(ValueError):
        LiveVideoPose.schedule(5, 3, [2, 2])
    with pytest.raises(ValueError):
        LiveVideoPose.schedule(4, 3, [4], max_push=3)


def test_live_video_pose_is_exported_from_the_package():
    import pavenet_amd
    from pavenet_amd.live import LiveVideoPose
    assert pavenet_amd.LiveVideoPose is LiveVideoPose


def test_nv12_csc_coefficients():
    """BT.601 limited range: the six values agree with the usual five-decimal figures 16, 1.16438, 1.59603,
    -0.39176, -0.81297, 2.01723 in every digit those give, and to 1e-6 with the same quantities written out to ten
    digits (the five-decimal figures themselves are up to 4e-6 away from 255/219 etc., so 1e-6 is asked of the
    longer ones)."""
    from pavenet_amd.preprocess import nv12_csc
    got = nv12_csc('bt601', False)
    assert [round(v, 5) for v in got] == [16, 1.16438, 1.59603, -0.39176, -0.81297, 2.01723]
    exact = (16.0, 1.1643835616, 1.5960267857, -0.3917622901, -0.8129676472, 2.0172321429)
    assert len(got) == 6 and all(abs(g - e) < 1e-6 for g, e in zip(got, exact)), got
    assert nv12_csc() == got
    full = nv12_csc('bt601', True)
    assert full[0] == 0 and full[1] == 1
    assert all(abs(g - e) < 1e-6 for g, e in zip(full[2:], (1.402, -0.3441362862, -0.7141362862, 1.772)))
    # BT.709: Kr = 0.2126, Kb = 0.0722
    hd = nv12_csc('bt709', True)
    assert all(abs(g - e) < 1e-6 for g, e in zip(hd, (0, 1, 1.5748, -0.1873242729, -0.4681242729, 1.8556)))
    lim = nv12_csc('bt709', False)
    assert lim[0] == 16 and abs(lim[1] - 255 / 219) < 1e-12
    assert all(abs(a - b * 255 / 224) < 1e-12 for a, b in zip(lim[2:], hd[2:]))
    with pytest.raises(ValueError):
        nv12_csc('bt2020')


def test_nv12_entry_point_in_header_library_and_binding():
    import ctypes
    import subprocess
    from pavenet_amd import native
    from pavenet_amd.build_native import build_native
    build_native()
    name = 'pave_preprocess_frames_nv12'
    assert name in open(native.HEADER_PATH).read()
    vp, ci, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    assert native.FUNCTIONS[name] == (ci, [vp, ll, ci, vp] + [ci] * 7 + [vp, vp, vp, ci, vp])
    assert name in native.SIGNATURES and name in native.EXPORTED
    for path in (native.LIB_PATH, native.DIAG_LIB_PATH):
        out = subprocess.run(['nm', '-D', '--defined-only', path], capture_output=True, text=True, check=True).stdout
        assert name in {ln.split()[-1] for ln in out.splitlines() if ' T ' in ln}, path
    assert hasattr(native.load(), name)
    assert native.ABI_VERSION == 21 and native.load().pave_abi_version() == 21


def test_preprocess_clip_nv12_argument_errors_come_before_any_device_call(monkeypatch):
    from pavenet_amd import preprocess

    def no_launch(*a, **k):
        raise AssertionError('a device call was made')
    monkeypatch.setattr(preprocess, '_launch', no_launch)
    ok = torch.zeros(2, 54, 64, dtype=torch.uint8)            # 36 rows of Y + 18 of UV, pitch 64
    # (an even height has 3 * H0 / 2 rows, a multiple of 3: 35 x 3 / 2 and 37 x 3 / 2 are no whole numbers)
    for surfaces, width in ((torch.zeros(2, 52, 64, dtype=torch.uint8), 50),    # H0 = 35 rounded down
                            (torch.zeros(2, 55, 64, dtype=torch.uint8), 50),    # H0 = 37 rounded down
                            (torch.zeros(2, 56, 64, dtype=torch.uint8), 50),
                            (ok, 49),                                           # odd width
                            (ok, 66),                                           # width > pitch
                            (ok.float(), 50), (ok[0], 50)):
        with pytest.raises(ValueError):
            preprocess.preprocess_clip_nv12(surfaces, width)
    with pytest.raises(ValueError, match='matrix'):
        preprocess.preprocess_clip_nv12(ok, 50, matrix='bt2020')
    with pytest.raises(RuntimeError, match='device'):          # a host tensor with good sizes: refused, no launch
        preprocess.preprocess_clip_nv12(ok, 50)


def test_ring_slabs_write_frames_to_their_slots():
    """RingSlabs on host tensors: frame f's memory and values land in slot f mod R across the wrap, in place;
    covers() answers for resident slots only; reset() keeps the tensors."""
    from pavenet_amd.live import RingSlabs
    R, S, C, n_pose = 4, 5, 3, 3
    ring = RingSlabs(R)
    assert len(ring) == 0 and not ring.covers([0])

    def mem(f0, n):
        return torch.stack([torch.full((S, C), float(f)) for f in range(f0, f0 + n)])

    def vals(f0, n):
        return [torch.stack([torch.full((S, 8, 2), float(10 * f + l)) for f in range(f0, f0 + n)]) for l in range(5)]
    f, ptrs = 0, None
    for n in (1, 2, 2, 1, 2, 2, 2):           # 12 frames through 4 slots, chunks that straddle the wrap
        ring._append_memory(mem(f, n))
        assert not ring.covers([f % R]), 'memory without its values is not covered'
        ring._append_values(vals(f, n), n_pose, 0)
        f += n
        ptrs = ptrs or [t.data_ptr() for t in ring.tensors()]
        assert [t.data_ptr() for t in ring.tensors()] == ptrs and len(ptrs) == 6 and len(ring) == R
        for g in range(max(0, f - R), f):
            assert (ring[g % R] == g).all() and ring[g % R].data_ptr() == ring.memory[g % R].data_ptr()
            for l, c in enumerate(ring.values[0] + ring.values[1]):
                assert c.shape == (R, S, 8, 2) and (c[g % R] == 10 * g + l).all()
        assert ring.covers(list(range(min(f, R)))) and not ring.covers([min(f, R)]) and not ring.covers([-1])
    assert len(ring.values[0]) == n_pose and len(ring.values[1]) == 2
    assert ring.resident_bytes() == R * S * C * 4 + 5 * R * S * 8 * 2 * 4
    ring.reset()
    assert not ring.covers([0]) and [t.data_ptr() for t in ring.tensors()] == ptrs
    ring._append_memory(mem(100, 1))
    ring._append_values(vals(100, 1), n_pose, 0)
    assert (ring[0] == 100).all() and ring.covers([0]) and not ring.covers([0, 1])
    with pytest.raises(AssertionError):
        ring._append_memory(mem(0, R + 1))
