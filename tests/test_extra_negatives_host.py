"""The closed form of the in-batch softmax with shared extra negatives (tests/_xneg_reference.py) against torch autograd, on the CPU.

1. loss, dN, dC, dX of the closed form equal autograd's of the masked_fill + logsumexp loss on the concatenated row logits to 1e-12
   relative -- with and without the logQ correction and the mask.
2. With Wx removed the form is tests/_mask_reference.reference.
"""
import numpy as np
import pytest
import torch

import _mask_reference as MR
import _xneg_reference as XR


def _unit_rows(R, D, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(R, D, generator=g, dtype=torch.float64)
    return (x / x.norm(dim=1, keepdim=True)).float()


def _lq(R, seed):
    v = np.random.default_rng(seed).uniform(-30.0, 0.0, R)
    if R >= 3:
        v[0], v[1], v[2] = 0.0, -40.0, -55.0
    return torch.tensor(v, dtype=torch.float32)


def _x_ids(ent_c, M, seed):
    """extras' company ids: some repeat a batch row's company (tile-edge rows among them), the rest are new"""
    B = ent_c.shape[0]
    g = np.random.default_rng(seed)
    ex = np.arange(M, dtype=np.int64) + 100 * B + 1000
    for j, a in enumerate((0, 31, 32, B - 1)):
        if j < M and 0 <= a < B:
            ex[(5 * j) % M] = int(ent_c[a])
    hit = g.permutation(M)[:max(M // 4, 1)]
    ex[hit] = ent_c.numpy()[g.integers(0, B, len(hit))]
    return torch.tensor(ex, dtype=torch.int32)


def _nrel(x, ref):
    return float((x - ref).norm() / max(float(ref.norm()), 1e-300))


CASES = [(5, 3, 4), (70, 33, 16), (40, 97, 8)]


@pytest.mark.parametrize("B,M,D", CASES)
@pytest.mark.parametrize("with_lq", [False, True])
@pytest.mark.parametrize("pattern", [None, "tile_edge", "groups"])
def test_closed_form_equals_autograd(B, M, D, with_lq, pattern):
    inv_t = 1.0 / 0.5
    n, c, x = _unit_rows(B, D, 1), _unit_rows(B, D, 2), _unit_rows(M, D, 3)
    ent_n = ent_c = ent_x = None
    if pattern is not None:
        ent_n, ent_c = MR.ids(B, pattern, seed=4)
        ent_x = _x_ids(ent_c, M, 5)
    lq_n, lq_c, lq_x = (_lq(B, 6), _lq(B, 7), _lq(M, 8)) if with_lq else (None, None, None)
    loss, dN, dC, dX = XR.reference(n, c, x, inv_t, "fp32", ent_n, ent_c, ent_x, lq_n, lq_c, lq_x)
    # autograd on the same f64 operands
    A, Bm, Xm = (t.double().clone().requires_grad_(True) for t in (n, c, x))
    S, Z = (A @ Bm.T) * inv_t, (A @ Xm.T) * inv_t
    Min = MR.mask_matrix(ent_n, ent_c) if pattern is not None else torch.zeros((B, B), dtype=torch.bool)
    Mx = XR.x_mask(ent_c, ent_x, B, M, "cpu")
    if pattern is not None:
        assert Mx.any() and not Mx.all()
    la = XR.xneg_loss(S, Z, Min, Mx, lq_n, lq_c, lq_x)
    la.backward()
    assert abs(loss - la.item()) <= 1e-12 * abs(la.item())
    for got, ref in ((dN, A.grad), (dC, Bm.grad), (dX, Xm.grad)):
        assert _nrel(got, ref) <= 1e-12, _nrel(got, ref)
    # the extras change the loss
    assert abs(loss - MR.reference(n, c, inv_t, *(MR.ids(B, "distinct") if pattern is None else (ent_n, ent_c)), "fp32", lq_n, lq_c)[0]) > 1e-6


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("with_lq", [False, True])
@pytest.mark.parametrize("pattern", ["distinct", "groups"])
def test_without_wx_is_the_mask_reference(mode, with_lq, pattern):
    B, M, D, inv_t = 70, 33, 16, 1.0
    n, c, x = _unit_rows(B, D, 11), _unit_rows(B, D, 12), _unit_rows(M, D, 13)
    ent_n, ent_c = MR.ids(B, pattern, seed=14)
    ent_x = _x_ids(ent_c, M, 15)
    lq_n, lq_c, lq_x = (_lq(B, 16), _lq(B, 17), _lq(M, 18)) if with_lq else (None, None, None)
    loss, dN, dC, dX = XR.reference(n, c, x, inv_t, mode, ent_n, ent_c, ent_x, lq_n, lq_c, lq_x, with_wx=False)
    rl, rN, rC = MR.reference(n, c, inv_t, ent_n, ent_c, mode, lq_n, lq_c)
    assert abs(loss - rl) <= 1e-14 * abs(rl)
    assert _nrel(dN, rN) <= 1e-14 and _nrel(dC, rC) <= 1e-14
    assert float(dX.abs().max()) == 0.0
