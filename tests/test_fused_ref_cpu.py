"""tests/fused_ref.py (the fp64 reference of the fused T-frame samplers) pinned to what the project already
trusts: the oracle composition of tests/fused_expected.py run in fp64.  No GPU."""
import numpy as np
import pytest
import torch

from oracle.seeded import seeded_array
from tests.fused_expected import grid_expected, pose_expected
from tests.fused_ref import grid_ref64, pose_ref64
from tests.msda_ref import contiguous_lsi, msda_ref

LEVELS = [(12, 20), (6, 10), (3, 5), (2, 3)]


def _t64(name, shape, scale=1.0):
    return torch.from_numpy(seeded_array(name, shape, scale)).double()


def _close(got, exp, rel=1e-12):
    """`rel` relative to the size of the expected numbers (an element that cancels to ~0 is not asked for
    1e-12 of ITSELF: both sides sum the same ~100 products in a different order)."""
    exp = exp.numpy()
    np.testing.assert_allclose(got.numpy(), exp, rtol=rel, atol=rel * np.abs(exp).max())


def _slabs(unit_clip, T):
    return unit_clip.long()[:, None] * T + torch.arange(T)[None]


@pytest.mark.parametrize('T', [1, 3])
def test_grid_reference_equals_the_oracle_composition_in_fp64(T):
    shapes = torch.as_tensor(LEVELS)
    lsi = contiguous_lsi(shapes)
    S, U, clips = int(shapes.prod(1).sum()), 13, 2
    value = _t64(f'fr.g.value.{T}', (clips * T, S, 8, 32))
    proj = _t64(f'fr.g.proj.{T}', (U, T * 8 * 16 * 3))
    proj[:, :T * 8 * 16 * 2] *= 2.0
    ref = _t64(f'fr.g.ref.{T}', (T, U, 4, 2), 0.35) + 0.5
    unit_clip = (torch.arange(U) * 5 % 3 % clips).long()          # not monotone
    exp = grid_expected(value, shapes, lsi, proj, ref, T, unit_clip)
    out, mx, sm = grid_ref64(value, shapes, lsi, proj, ref, T, _slabs(unit_clip, T))
    assert out.dtype == torch.float64 and exp.dtype == torch.float64
    _close(out, exp)
    lg = proj[:, T * 8 * 16 * 2:].view(U, T, 8, 16).permute(0, 2, 1, 3).reshape(U, 8, -1)
    assert torch.equal(mx, lg.max(-1)[0])
    _close(sm, torch.exp(lg - lg.max(-1, keepdim=True)[0]).sum(-1))


@pytest.mark.parametrize('T', [1, 3])
@pytest.mark.parametrize('L,K', [(1, 7), (2, 16), (3, 17), (4, 15)])
def test_pose_reference_equals_the_oracle_composition_in_fp64(L, K, T):
    shapes = torch.as_tensor(LEVELS[:L])
    lsi = contiguous_lsi(shapes)
    S, clips, Q = int(shapes.prod(1).sum()), 2, 3
    value = _t64(f'fr.p.value.{L}.{T}', (clips * T, S, 8, 32))
    proj = _t64(f'fr.p.proj.{L}.{T}', (clips * Q, T * 8 * L * K * 3))
    ref = torch.sigmoid(_t64(f'fr.p.ref.{L}.{T}', (clips, T * Q, L, 2 * K)))
    exp = pose_expected(value, shapes, lsi, proj, ref, T, clips, Q, K)
    out, mx, sm = pose_ref64(value, shapes, lsi, proj, ref, T, clips, Q, K,
                             _slabs(torch.arange(clips * Q) // Q, T))
    _close(out, exp)
    lg = proj[:, T * 8 * L * K * 2:].view(clips * Q, T, 8, L * K).permute(0, 2, 1, 3).reshape(clips * Q, 8, -1)
    assert torch.equal(mx, lg.max(-1)[0])
    _close(sm, torch.exp(lg - lg.max(-1, keepdim=True)[0]).sum(-1))


def test_reference_softmax_is_shift_invariant():
    """+200 on every logit overflows an un-stabilised fp32 exp; the reference is unmoved.  The shift is made in
    fp64, where 200 + x keeps x to 2.8e-14: the weights move by ~1e-13 relative, 1e-11 is asked."""
    shapes = torch.as_tensor(LEVELS)
    lsi = contiguous_lsi(shapes)
    S, T, U, K, Q = int(shapes.prod(1).sum()), 3, 6, 5, 3
    value = _t64('fr.s.value', (2 * T, S, 8, 32))
    proj = _t64('fr.s.proj', (U, T * 8 * 16 * 3))
    ref = _t64('fr.s.ref', (T, U, 4, 2), 0.3) + 0.5
    slabs = _slabs(torch.arange(U) % 2, T)
    a, amx, asm = grid_ref64(value, shapes, lsi, proj, ref, T, slabs)
    hot = proj.clone()
    hot[:, T * 8 * 16 * 2:] += 200.0
    b, bmx, bsm = grid_ref64(value, shapes, lsi, hot, ref, T, slabs)
    assert torch.isfinite(b).all()
    _close(b, a, 1e-11)
    _close(bmx, amx + 200.0, 1e-15)
    _close(bsm, asm, 1e-11)
    pproj = _t64('fr.s.pproj', (2 * Q, T * 8 * 4 * K * 3))
    pref = torch.sigmoid(_t64('fr.s.pref', (2, T * Q, 4, 2 * K)))
    pslabs = _slabs(torch.arange(2 * Q) // Q, T)
    a = pose_ref64(value, shapes, lsi, pproj, pref, T, 2, Q, K, pslabs)[0]
    hot = pproj.clone()
    hot[:, T * 8 * 4 * K * 2:] += 200.0
    b = pose_ref64(value, shapes, lsi, hot, pref, T, 2, Q, K, pslabs)[0]
    _close(b, a, 1e-11)


def test_pose_clamp_engages_for_coincident_key_points():
    """A query whose K key points coincide has extent 0 on both axes: the offsets are scaled by the 1e-4 floor
    (a 5e-5 step per unit offset), not by 0 -- the output is that of points at ref + offset * 5e-5, and it is
    NOT the output of all points sitting on the key point."""
    shapes = torch.as_tensor(LEVELS)
    lsi = contiguous_lsi(shapes)
    S, T, Q, K, L = int(shapes.prod(1).sum()), 1, 2, 6, 4
    value = _t64('fr.c.value', (1, S, 8, 32))
    proj = _t64('fr.c.proj', (Q, 8 * L * K * 3))
    proj[:, :8 * L * K * 2] *= 20.0                # 20 * 5e-5 * 20 px: a thousandth of a pixel and more
    ref = torch.sigmoid(_t64('fr.c.ref', (1, Q, L, 2 * K)))
    point = torch.tensor([0.37, 0.61], dtype=torch.float64)
    ref[0, 0] = point.repeat(K)                    # query 0: every key point of every level at one place
    out = pose_ref64(value, shapes, lsi, proj, ref, T, 1, Q, K, torch.zeros(Q, 1, dtype=torch.long))[0]
    off = proj[:1, :8 * L * K * 2].view(1, 1, 8, L, K, 2)
    w = proj[:1, 8 * L * K * 2:].view(1, 1, 8, L * K).softmax(-1).view(1, 1, 8, L, K)
    moved = msda_ref(value, shapes, lsi, point + off * 1e-4 * 0.5, w)[0, 0]
    still = msda_ref(value, shapes, lsi, point + off * 0.0, w)[0, 0]
    _close(out[0], moved)
    assert (out[0] - still).abs().max() > 1e-6 * still.abs().max()
    # query 1 has spread key points and is the oracle's
    _close(out, pose_expected(value, shapes, lsi, proj, ref, T, 1, Q, K))
