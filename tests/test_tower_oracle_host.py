"""The tower oracle checked before it judges: oracle_np.tower_fwd / tower_bwd (q = None, f64) against torch float64 autograd of the
reference's layer stack -- nn.Linear projection and the concatenation with the looked-up rows, [Linear, ReLU, BatchNorm1d,
Dropout(p = 0)] blocks, Linear, F.normalize -- at every shape of test_gpu_tower_parity's case table (B capped).  CPU only."""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import oracle_np as O
from test_gpu_tower_parity import CASES, _keys_vocabs

B_CAP = 1024
TOL = 1e-12
TOL_TWO_ROWS = 1e-10     # BatchNorm over two rows: the gradients in front of it are O(1) terms cancelling to f64 noise (~1e-16)


def _state(c, rng):
    """random tower state (prefix-free keys) for the notice side of case c"""
    kn, _, vn, _ = _keys_vocabs(c)
    E, din, hidden, D = c["E"], c["din"][0], c["hidden"], c["D"]
    st = {f"categorical_embedder.embeddings.{k}.weight": rng.standard_normal((v, E)) for k, v in zip(kn, vn)}
    st["dense_projection.weight"] = rng.standard_normal((hidden[0], din)) / np.sqrt(din)
    st["dense_projection.bias"] = 0.1 * rng.standard_normal(hidden[0])
    w_in = hidden[0] + len(kn) * E
    for i, h in enumerate(hidden[1:]):
        st[f"mlp.{4 * i}.weight"] = rng.standard_normal((h, w_in)) / np.sqrt(w_in)
        st[f"mlp.{4 * i}.bias"] = 0.1 * rng.standard_normal(h)
        st[f"mlp.{4 * i + 2}.weight"] = 1 + 0.1 * rng.standard_normal(h)
        st[f"mlp.{4 * i + 2}.bias"] = 0.1 * rng.standard_normal(h)
        st[f"mlp.{4 * i + 2}.running_mean"] = 0.2 * rng.standard_normal(h)
        st[f"mlp.{4 * i + 2}.running_var"] = 0.5 + rng.random(h)
        st[f"mlp.{4 * i + 2}.num_batches_tracked"] = np.asarray(3, dtype=np.int64)
        w_in = h
    st[f"mlp.{4 * (len(hidden) - 1)}.weight"] = rng.standard_normal((D, w_in)) / np.sqrt(w_in)
    st[f"mlp.{4 * (len(hidden) - 1)}.bias"] = 0.1 * rng.standard_normal(D)
    return st, kn, vn


def _torch_tower(st, keys, hidden, D, dense, ids, d_emb, train):
    """the reference's layer stack in torch float64: returns (emb, {key: grad}, {key: updated BN buffer})"""
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
    tables = [t(st[f"categorical_embedder.embeddings.{k}.weight"]).requires_grad_() for k in keys]
    proj = nn.Linear(*st["dense_projection.weight"].shape[::-1]).double()
    layers = []
    w_in = hidden[0] + sum(tb.shape[1] for tb in tables)
    for h in hidden[1:]:
        layers += [nn.Linear(w_in, h), nn.ReLU(), nn.BatchNorm1d(h), nn.Dropout(0.0)]
        w_in = h
    layers.append(nn.Linear(w_in, D))
    mlp = nn.Sequential(*layers).double()
    with torch.no_grad():
        for name, prm in list(proj.named_parameters()):
            prm.copy_(t(st["dense_projection." + name]))
        for name, v in mlp.state_dict().items():
            v.copy_(t(st["mlp." + name]))
    mlp.train(train)
    x = torch.cat([proj(t(dense))] + [tb[torch.from_numpy(ids[:, k])] for k, tb in enumerate(tables)], dim=1)
    emb = F.normalize(mlp(x), p=2, dim=1)
    if train:
        torch.autograd.backward(emb, t(d_emb))
    grads = {"dense_projection." + n: p.grad.numpy() for n, p in proj.named_parameters()} if train else {}
    grads.update({"mlp." + n: p.grad.numpy() for n, p in mlp.named_parameters() if p.grad is not None})
    grads.update({f"categorical_embedder.embeddings.{k}.weight": tb.grad.numpy() for k, tb in zip(keys, tables) if tb.grad is not None})
    bufs = {"mlp." + n: b.numpy() for n, b in mlp.named_buffers()}
    return emb.detach().numpy(), grads, bufs


def _err(got, ref):
    """max-abs error relative to the reference's largest element; absolute where the reference is zero up to rounding (D = 1: a
    unit row of one element has no tangent space, every gradient vanishes -- autograd leaves ~1e-14, the oracle exact zeros)"""
    ref = np.asarray(ref, dtype=np.float64)
    scale = np.abs(ref).max() if ref.size else 0.0
    return float(np.abs(np.asarray(got, dtype=np.float64) - ref).max(initial=0.0) / (scale if scale > 1e-9 else 1.0))


@pytest.mark.parametrize("c", CASES)
def test_tower_oracle_vs_torch_autograd(c):
    B = min(c["B"], B_CAP)
    rng = np.random.default_rng(B * 31 + c["D"])
    st, keys, vocab = _state(c, rng)
    dense = rng.standard_normal((B, c["din"][0]))
    ids = np.stack([rng.integers(0, v + 3, B) for v in vocab], axis=1)          # a few ids past the table: clamped
    ids_c = O.unpack_clamp_ids(ids.reshape(-1), vocab)
    d_emb = rng.standard_normal((B, c["D"]))
    for train in ((False,) if c["mode"] == "eval" else (True, False)):
        emb, cache, bn_up = O.tower_fwd(st, "", keys, vocab, dense, ids.reshape(-1), train, np.float64)
        t_emb, t_grads, t_bufs = _torch_tower(st, keys, c["hidden"], c["D"], dense, ids_c, d_emb, train)
        assert _err(emb, t_emb) <= TOL, ("emb", train)
        if not train:
            continue
        for k, v in bn_up.items():
            if k.endswith("num_batches_tracked"):
                assert int(v) == int(t_bufs[k]), k
            else:
                assert _err(v, t_bufs[k]) <= TOL, k
        g = O.tower_bwd(cache, d_emb, "", keys, vocab, "dense", "direct")
        gf = O.tower_bwd(cache, d_emb, "", keys, vocab, "dense", "factored")
        names = [k for k in g if not k.startswith("_")]
        assert sorted(names) == sorted(t_grads), (sorted(names), sorted(t_grads))
        tol = TOL_TWO_ROWS if B == 2 else TOL
        for k in names:
            assert _err(g[k], t_grads[k]) <= tol, k
            assert _err(gf[k], g[k]) <= tol, ("factored", k)
