"""The composed f64 oracle of a step with shared extra negatives (tests/_xneg_step_reference.py) against torch f64 autograd, on the CPU.

The same step is built a second way: oracle_torch._tower for both sides (the company side over the concatenated B + M rows), then
tests/_xneg_reference.xneg_loss on the two score blocks, then autograd.  Loss, every dense gradient, every table's dense gradient
and the BatchNorm running statistics must agree to 1e-10 norm-wise per tensor -- plain and with logQ plus entity ids, at
(B, M) = (5, 3) and (9, 20).  The sparse row list scattered into the fused row space must be the same gradient; with the notice
rows dropped from that list (what a store that keeps one pending side leaves the optimiser) it is far outside the bar.
"""
import numpy as np
import pytest
import torch

import oracle_np as O
import oracle_torch as OT
from params_init import init_state_numpy
import _mask_reference as MR
import _xneg_reference as XR
import _xneg_step_reference as SR

BAR = 1e-10
KN, KC, VN, VC = ["na", "nb"], ["ca", "cb"], [9, 6], [7, 11]
E, DIN_N, DIN_C, HIDDEN, D, T = 4, 6, 5, [8, 7], 6, 0.5


def _state(seed):
    shapes = {}
    for pre, keys, vocab, din in ((O.NT, KN, VN, DIN_N), (O.CT, KC, VC, DIN_C)):
        for k, v in zip(keys, vocab):
            shapes[f"{pre}categorical_embedder.embeddings.{k}.weight"] = (v, E)
        shapes[pre + "dense_projection.weight"], shapes[pre + "dense_projection.bias"] = (HIDDEN[0], din), (HIDDEN[0],)
        kx = HIDDEN[0] + len(keys) * E
        shapes[pre + "mlp.0.weight"], shapes[pre + "mlp.0.bias"] = (HIDDEN[1], kx), (HIDDEN[1],)
        for n in ("weight", "bias", "running_mean", "running_var"):
            shapes[f"{pre}mlp.2.{n}"] = (HIDDEN[1],)
        shapes[pre + "mlp.2.num_batches_tracked"] = ()
        shapes[pre + "mlp.4.weight"], shapes[pre + "mlp.4.bias"] = (D, HIDDEN[1]), (D,)
    return {k: (v.astype(np.float64) if v.dtype.kind == "f" else v) for k, v in init_state_numpy(shapes, 5 + seed).items()}


def _err(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-300))


@pytest.mark.parametrize("B,M", [(5, 3), (9, 20)])
@pytest.mark.parametrize("decorated", [False, True])
def test_composed_oracle_equals_autograd(B, M, decorated):
    state = _state(B)
    b = SR.make_batch(B, M, VN, VC, DIN_N, DIN_C, 3 + M, decorated)
    ref = SR.xneg_step(state, b, KN, KC, VN, VC, T, "fp32")
    # the same step in torch f64 autograd
    st = OT.make_state(state)
    f = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64))
    dense_c, ids_c = SR.company_side(b)
    n = OT._tower(st, OT.NT, KN, VN, f(b["notice_dense"]), torch.from_numpy(b["notice_ids"]).reshape(-1), True)
    cx = OT._tower(st, OT.CT, KC, VC, f(dense_c), torch.from_numpy(ids_c).reshape(-1), True)
    c, x = cx[:B], cx[B:]
    g = lambda k: None if b.get(k) is None else torch.from_numpy(b[k])
    Min = MR.mask_matrix(g("ent_n"), g("ent_c")) if decorated else torch.zeros((B, B), dtype=torch.bool)
    Mx = XR.x_mask(g("ent_c"), g("ent_x"), B, M, "cpu")
    if decorated:
        assert Min.any() and Mx.any() and not Mx.all()
    loss = XR.xneg_loss((n @ c.T) / T, (n @ x.T) / T, Min, Mx, g("lq_n"), g("lq_c"), g("lq_x"))
    loss.backward()
    assert abs(ref["loss"] - loss.item()) <= BAR * abs(loss.item())
    for name, got in (("N", n), ("C", c), ("X", x)):
        assert _err(ref[name], got.detach().numpy()) <= BAR, name
    params = {k: v for k, v in st.items() if v.requires_grad}
    assert set(ref["grads"]) == set(params)
    for k, p in params.items():
        assert _err(ref["grads"][k], p.grad.numpy()) <= BAR, (k, _err(ref["grads"][k], p.grad.numpy()))
    for k, v in ref["bn_updates"].items():                   # F.batch_norm updated the running statistics in place, over B + M rows
        assert _err(v, st[k].detach().numpy()) <= BAR, k
    # the sparse row list is the same gradient in the fused row space (notice keys, then company keys) ...
    tables = [params[f"{pre}categorical_embedder.embeddings.{k}.weight"].grad.numpy() for pre, keys in ((O.NT, KN), (O.CT, KC)) for k in keys]
    fused = np.concatenate(tables, 0)
    rn, gn, rc, gc = ref["rows"]
    assert rn.max() < sum(VN) <= rc.min()
    assert _err(SR.scatter_rows(np.concatenate([rn, rc]), np.concatenate([gn, gc]), fused.shape[0]), fused) <= BAR
    # ... and one that lost the notice side's rows is not: the comparison can fail
    assert _err(SR.scatter_rows(rc, gc, fused.shape[0]), fused) > 0.1
    # the ids carry every case: a company row only an extra carries, rows nobody carries, repeats
    only_extra = sum(VN) + VC[0] - 2
    assert only_extra in rc and VC[0] - 2 not in b["company_ids"][:, 0]
    assert sum(VN) + VC[0] - 1 not in rc and VN[0] - 1 not in rn
    assert len(rn) < B * len(KN) and len(rc) < (B + M) * len(KC)
