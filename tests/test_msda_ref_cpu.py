"""The gather reference of the sampler (tests/msda_ref.py) against the oracle's formulations, on the host."""
import numpy as np
import pytest
import torch

from oracle import pavenet_ref as R
from tests.msda_ref import contiguous_lsi, msda_ref

CASES = [  # (bs, M, D, levels, Lq, P)
    (1, 1, 1, [(1, 1)], 7, 1),
    (2, 3, 5, [(3, 2), (2, 1)], 6, 2),
    (3, 8, 4, [(1, 9), (7, 3), (1, 1)], 5, 4),
    (1, 2, 3, [(5, 4), (1, 6), (4, 1), (2, 2), (3, 3), (1, 1), (6, 2), (2, 5)], 4, 3),
]


def _inputs(bs, M, D, levels, Lq, P, seed):
    g = torch.Generator().manual_seed(seed)
    shapes = torch.as_tensor(levels, dtype=torch.long)
    S, L = int(shapes.prod(1).sum()), len(levels)
    value = torch.rand(bs, S, M, D, generator=g, dtype=torch.float64) * 2 - 1
    loc = torch.rand(bs, Lq, M, L, P, 2, generator=g, dtype=torch.float64) * 1.3 - 0.15
    aw = torch.rand(bs, Lq, M, L, P, generator=g, dtype=torch.float64) + 0.05
    return shapes, value, loc, aw / aw.sum((-1, -2), keepdim=True)


@pytest.mark.parametrize('case', range(len(CASES)))
def test_ref_equals_grid_sample_formulation_and_its_gradients(case):
    shapes, value, loc, aw = _inputs(*CASES[case], seed=case)
    lsi = contiguous_lsi(shapes)
    a = [t.clone().requires_grad_(True) for t in (value, loc, aw)]
    b = [t.clone().requires_grad_(True) for t in (value, loc, aw)]
    out_a = msda_ref(a[0], shapes, lsi, a[1], a[2])
    out_b = R.msda_forward_torch(b[0], shapes, b[1], b[2])
    np.testing.assert_allclose(out_a.detach().numpy(), out_b.detach().numpy(), rtol=1e-12, atol=1e-13)
    gout = torch.rand(out_a.shape, generator=torch.Generator().manual_seed(100 + case), dtype=torch.float64)
    out_a.backward(gout)
    out_b.backward(gout)
    for x, y in zip(a, b):
        np.testing.assert_allclose(x.grad.numpy(), y.grad.numpy(), rtol=1e-11, atol=1e-12)


def test_ref_on_a_query_subset_equals_the_same_rows_of_the_full_call():
    shapes, value, loc, aw = _inputs(*CASES[2], seed=7)
    lsi = contiguous_lsi(shapes)
    full = msda_ref(value, shapes, lsi, loc, aw)
    q = torch.tensor([4, 0, 2])
    assert torch.equal(msda_ref(value, shapes, lsi, loc, aw, queries=q), full[:, q])


def test_ref_honours_level_start_index_and_the_range_test():
    """Levels stored in reverse order with unused rows between them give the same result as the contiguous
    layout, and the C restatement of mmcv's kernel (which reads lsi) agrees, NaN / inf locations included."""
    shapes, value, loc, aw = _inputs(*CASES[3], seed=3)
    sizes = shapes.prod(1).tolist()
    lsi = contiguous_lsi(shapes)
    gap = 5
    S2 = sum(sizes) + gap
    lsi2 = torch.zeros_like(lsi)
    pos = 0
    for l in reversed(range(len(sizes))):
        lsi2[l] = pos
        pos += sizes[l] + (gap if l == 4 else 0)
    v2 = torch.full((value.shape[0], S2) + tuple(value.shape[2:]), 1e3, dtype=torch.float64)
    for l in range(len(sizes)):
        v2[:, lsi2[l]:lsi2[l] + sizes[l]] = value[:, lsi[l]:lsi[l] + sizes[l]]
    loc.view(-1)[::11] = torch.tensor([float('nan'), float('inf'), -float('inf'), 1e30, -1e30]).repeat(
        loc.numel())[:loc.view(-1)[::11].numel()]
    assert torch.equal(msda_ref(v2, shapes, lsi2, loc, aw), msda_ref(value, shapes, lsi, loc, aw))
    np.testing.assert_allclose(msda_ref(v2, shapes, lsi2, loc, aw).numpy(),
                               R.msda_forward_c(v2.numpy(), shapes.numpy(), lsi2.numpy(), loc.numpy(),
                                                aw.numpy()), rtol=1e-13, atol=1e-14)
