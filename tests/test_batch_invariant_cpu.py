"""Batch-invariant inference, host side: the form plan of the GEMM / convolution dispatchers
(pave_form_plan) is a function of (K, N, kind) alone under form policies 1 and 2, and reproduces
the selection by row count under policy 0; the Python switches refuse what they do not cover."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ops():
    from pavenet_amd import ops
    return ops


def test_form_policy_abi_is_declared_exported_and_typed():
    """The three entry points are in the header, the library and native.py, and the three agree on the ABI version
    (they are additions: no existing signature changed, and a library without them fails native.load())."""
    from pavenet_amd import native
    header = open(os.path.join(ROOT, 'include', 'pave_hip.h')).read()
    lib = native.load()
    assert lib.pave_abi_version() == native.ABI_VERSION == int(
        re.search(r'#define PAVE_ABI_VERSION (\d+)', header).group(1))
    assert 'pave_form_plan' in native.SIGNATURES and 'pave_set_form_policy' in native.SIGNATURES
    for name in ('pave_set_form_policy', 'pave_get_form_policy', 'pave_form_plan'):
        assert name in native.EXPORTED and re.search(r'\b' + name + r'\s*\(', header)
        assert getattr(lib, name) is not None


def _sweep_rows():
    """1 .. 2^20 with every threshold of the dispatchers +- 1: the K-split form's 2 048 rows and its 4 096 / 1 280
    32 x 32 tiles, the small-row form's 8 192 rows and 64 tiles, the split-K tile classes 16 / 128 / 200 (x 128 rows),
    the wide form's 400 tiles, the LayerNorm wide form's 512 row tiles and its 2^22-row identity-buffer limit."""
    ms = {1 << e for e in range(21)}
    bases = [2048, 8192, 16 * 128, 128 * 128, 200 * 128, 400 * 128, 512 * 128, 64 * 128]
    bases += [4096 * 32 // c for c in (1, 2, 4, 8, 16, 32, 64)] + [1280 * 32 // c for c in (1, 2, 4, 8, 16, 32)]
    bases += [400 * 128 // c for c in (1, 2, 4, 8)] + [200 * 128 // c for c in (1, 2, 4, 8)]
    for b in bases:
        ms.update((b - 1, b, b + 1))
    ms.update(range(1, 40))
    ms.update((300, 600, 1200, 2100, 2400, 3150, 7350, 22323, 89292, 156261, 625044))
    ms.update(((1 << 22) - 1, 1 << 22, (1 << 22) + 1))
    return sorted(m for m in ms if 1 <= m <= (1 << 22) + 1)


def _r50_t7_shapes():
    """Every (K, N, kind) the R-50 T = 7 PAVE-Net launches (ResNet-50 bottlenecks, ChannelMapper, deformable
    encoder, pose / joint decoders, heads)."""
    o = _ops()
    s = set()
    for cin, mid, cout in ((64, 64, 256), (256, 64, 256), (256, 128, 512), (512, 128, 512), (512, 256, 1024),
                           (1024, 256, 1024), (1024, 512, 2048), (2048, 512, 2048)):
        s.add((cin, mid, o.FORM_ROWS_SPLITK))           # conv1
        s.add((9 * mid, mid, o.FORM_CONV3X3))           # conv2
        s.add((mid, cout, o.FORM_ROWS_SPLITK))          # conv3 + identity
        s.add((mid + cin, cout, o.FORM_ROWS_TILE))      # conv3 | downsample (two sources)
        s.add((cin, cout, o.FORM_CONV1X1S))             # stride-2 downsample
        s.add((cin, cout, o.FORM_ROWS_SPLITK))
    for cin in (512, 1024, 2048):
        s.add((cin, 256, o.FORM_ROWS_SPLITK))           # ChannelMapper laterals
    s.add((9 * 2048, 256, o.FORM_CONV3X3))             # its extra level
    s.add((256, 256, o.FORM_ENCPROJ))
    for k, n in ((256, 256), (256, 512), (256, 1024), (1024, 256), (256, 384), (256, 768), (256, 2688),
                 (512, 512), (256, 30), (256, 2), (256, 1), (512, 30), (512, 34), (256, 64), (256, 128)):
        s.add((k, n, o.FORM_ROWS))
        s.add((k, n, o.FORM_ROWS_SPLITK))
        s.add((k, n, o.FORM_ROWS_TILE))
    for k in (64, 128, 256, 1024):
        s.add((k, 256, o.FORM_LN))
    return sorted(s)


@pytest.mark.parametrize('policy', [1, 2])
def test_plan_is_independent_of_the_row_count(policy):
    o = _ops()
    ms = _sweep_rows()
    for planes in (3, o.PLANES_FP16):
        for k, n, kind in _r50_t7_shapes():
            plans = {o.form_plan(m, k, n, kind, policy=policy, planes=planes) for m in ms}
            assert len(plans) == 1, (k, n, kind, policy, planes, plans)
            order, parts = plans.pop()
            assert parts == 1 and order != o.ORDER_SPLITK
            if policy == 1:
                assert order == o.ORDER_TILE
            elif kind == o.FORM_LN:
                assert order == (o.ORDER_KSPLIT_LNPASS if k >= 256 else o.ORDER_TILE)
            elif kind in (o.FORM_ROWS, o.FORM_ROWS_SPLITK):
                assert order == (o.ORDER_KSPLIT if (k >= 512 or (k >= 256 and n <= 512)) else o.ORDER_TILE)
            else:
                assert order == o.ORDER_TILE


def test_policy_0_keeps_the_selection_by_row_count():
    o = _ops()
    plan = lambda *a: o.form_plan(*a, policy=0)   # noqa: E731
    # the decoders' FFN2: K-split form up to 2 048 rows, the tile kernels above
    assert plan(1200, 1024, 256) == (o.ORDER_KSPLIT, 1)
    assert plan(2048, 1024, 256) == (o.ORDER_KSPLIT, 1)
    assert plan(2400, 1024, 256) == (o.ORDER_TILE, 1)
    assert plan(1200, 1024, 256, o.FORM_LN) == (o.ORDER_KSPLIT_LNPASS, 1)
    assert plan(2400, 1024, 256, o.FORM_LN) == (o.ORDER_TILE_LNPASS, 1)
    assert plan(31 * 128, 64, 256, o.FORM_LN) == (o.ORDER_TILE_LNPASS, 1)     # (fewer than 64 128 x 128 tiles)
    # ... then the fused epilogue: the 8-wave block below 512 row tiles, the wide form from there on, the 8-wave block
    # again from 2^22 rows (the wide form's identity buffer) -- three orders of one LayerNorm GEMM by row count
    assert plan(31 * 128 + 1, 1024, 256, o.FORM_LN) == (o.ORDER_TILE_LN8, 1)
    assert plan(511 * 128, 1024, 256, o.FORM_LN) == (o.ORDER_TILE_LN8, 1)
    assert plan(511 * 128 + 1, 1024, 256, o.FORM_LN) == (o.ORDER_TILE, 1)
    assert plan((1 << 22) - 1, 256, 256, o.FORM_LN) == (o.ORDER_TILE, 1)
    assert plan(1 << 22, 256, 256, o.FORM_LN) == (o.ORDER_TILE_LN8, 1)
    # one-clip T = 7 layer4 at 800 x 1344 (25 x 42 pixels per frame): split-K parts for the 3x3 and the 1x1
    # reduction; the 4-clip bench batch takes the tile kernels
    assert plan(7350, 9 * 512, 512, o.FORM_CONV3X3) == (o.ORDER_SPLITK, 4)
    assert plan(7350, 2048, 512, o.FORM_ROWS_SPLITK) == (o.ORDER_SPLITK, 4)
    assert plan(4 * 7350, 9 * 512, 512, o.FORM_CONV3X3) == (o.ORDER_TILE, 1)
    assert plan(4 * 7350, 2048, 512, o.FORM_ROWS_SPLITK) == (o.ORDER_TILE, 1)
    # the ChannelMapper's extra level of a one-clip batch (819 pixels, K = 18 432): 32 parts
    assert plan(819, 9 * 2048, 256, o.FORM_CONV3X3)[0] == o.ORDER_SPLITK
    assert plan(819, 9 * 2048, 256, o.FORM_CONV3X3)[1] >= 8
    for kind in (o.FORM_ROWS_TILE, o.FORM_CONV1X1S, o.FORM_ENCPROJ):
        assert plan(300, 1024, 256, kind) == (o.ORDER_TILE, 1)
    # the same answers as the library's own split-K plan (workspace sizes)
    lib = __import__('pavenet_amd.native', fromlist=['load']).load()
    for m in (819, 3150, 7350, 29400):
        parts = plan(m, 2048, 512, o.FORM_ROWS_SPLITK)[1]
        assert lib.pave_gemm_splitk_workspace_bytes(m, 2048, 512) == (parts * m * 512 * 4 if parts > 1 else 0)


def test_split_k_workspaces_follow_the_policy():
    o = _ops()
    lib = __import__('pavenet_amd.native', fromlist=['load']).load()
    assert lib.pave_conv3x3_splitk_workspace_bytes(1, 25, 42, 512, 512, 1) > 0
    assert lib.pave_gemm_splitk_workspace_bytes(1050, 2048, 512) > 0
    for p in (1, 2):
        with o.form_policy(p):
            assert lib.pave_get_form_policy() == p
            assert lib.pave_conv3x3_splitk_workspace_bytes(1, 25, 42, 512, 512, 1) == 0
            assert lib.pave_gemm_splitk_workspace_bytes(1050, 2048, 512) == 0
    assert lib.pave_get_form_policy() == 0


def test_form_policy_restores_on_exit_and_on_exception():
    o = _ops()
    lib = __import__('pavenet_amd.native', fromlist=['load']).load()
    with o.form_policy(1):
        with o.form_policy(2):
            assert lib.pave_get_form_policy() == 2 and o.current_form_policy() == 2
        assert lib.pave_get_form_policy() == 1 and o.current_form_policy() == 1
        with pytest.raises(KeyError):
            with o.form_policy(2):
                raise KeyError('boom')
        assert lib.pave_get_form_policy() == 1
    assert lib.pave_get_form_policy() == 0 and o.current_form_policy() == 0
    with pytest.raises(RuntimeError):
        with o.form_policy(3):
            pass
    assert lib.pave_set_form_policy(3) != 0 and lib.pave_get_form_policy() == 0
    with pytest.raises(RuntimeError):
        o.form_plan(100, 256, 256, kind=7)


def test_set_batch_invariant_scope_checks():
    from pavenet_amd import bricks
    from pavenet_amd.models import build_model, petr_r50_cfg, videopose_r50_cfg
    m = build_model(videopose_r50_cfg(num_frames=3, max_per_img=4))
    assert m.batch_invariant is False
    old = bricks.get_gemm_mode()
    try:
        for mode in ('native', 'fp16', 'bf16'):
            bricks.set_gemm_mode(mode)
            with pytest.raises(ValueError):
                bricks.set_batch_invariant(m)
            assert m.batch_invariant is False
        bricks.set_gemm_mode('bf16x3')
        assert bricks.set_batch_invariant(m) is m and m.batch_invariant is True
        bricks.set_gemm_mode('native')            # a mode switched after the flag: refused at forward time
        with pytest.raises(ValueError):
            bricks.batch_invariant_scope(m)
        bricks.set_batch_invariant(m, False)       # leaving the mode is always allowed
        assert m.batch_invariant is False
        bricks.set_gemm_mode('bf16x3')
        with pytest.raises(NotImplementedError):
            bricks.set_batch_invariant(build_model(petr_r50_cfg(max_per_img=4)))
    finally:
        bricks.set_gemm_mode(old)


def test_form_policy_is_per_thread():
    """A batch-invariant block on one Python thread leaves another thread's policy (and what it reads of it) at 0."""
    import threading
    o = _ops()
    inside, done = threading.Event(), threading.Event()
    seen = []

    def worker():
        with o.form_policy(1):
            seen.append(o.current_form_policy())
            inside.set()
            done.wait(30)
        seen.append(o.current_form_policy())

    t = threading.Thread(target=worker)
    t.start()
    assert inside.wait(30)
    try:
        assert o.current_form_policy() == 0
        from pavenet_amd import bricks
        assert isinstance(bricks.query_rows_scope(), __import__('contextlib').nullcontext)
    finally:
        done.set()
        t.join(30)
    assert seen == [1, 0]


def test_library_without_the_form_policy_entries_is_refused(tmp_path):
    """The entry points were added without a signature change (ABI version kept): a library built from older sources
    lacks them and is refused with the rebuild message, not a bare ctypes error."""
    import subprocess
    from pavenet_amd import native
    src = tmp_path / 'stale.c'
    src.write_text('int pave_abi_version(void) { return %d; }\n'
                   'const char* pave_last_error(void) { return ""; }\n' % native.ABI_VERSION)
    so = tmp_path / 'libstale.so'
    subprocess.check_call(['gcc', '-shared', '-fPIC', '-o', str(so), str(src)])
    with pytest.raises(native.NativeLibraryError, match='pave_form_plan'):
        native._open(str(so))
