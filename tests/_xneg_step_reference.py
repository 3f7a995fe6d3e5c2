"""float64 reference of ONE training step whose batch carries shared extra negatives: the two tower sides
have different row counts -- the notice tower runs over B rows, the company tower over the B batch companies followed by the M
extras.  Nothing new is derived here; the step is composed from pieces that are pinned elsewhere:

    towers    oracle_np.tower_fwd / tower_bwd, the company side over the CONCATENATED B + M rows (train-mode BatchNorm batch
              statistics and running-statistic updates therefore cover B + M rows); C = rows [:B], X = rows [B:] of its output
    score     tests/_xneg_reference.reference on the f64 embeddings: loss, dN, dC, dX (mode "fp32", or "bf16" together with
              rounding="bf16" in the towers)
    tables    oracle_np.embed_grad_dense per key, and oracle_np.embed_grad_sparse over the fused row space (notice keys, then
              company keys: the offsets of test_gpu_parity.test_bf16_step_vs_rounded_oracle)
    optimiser oracle_np.adam_step / sparse_adam_rows at step 1 with the f32 hyper-parameters the kernels see

batch: numpy arrays notice_dense [B, Dn], notice_ids [B, Kn], company_dense [B, Dc], company_ids [B, Kc], neg_dense [M, Dc],
neg_ids [M, Kc] and optionally lq_n / lq_c [B], lq_x [M] (f32) and ent_n / ent_c [B], ent_x [M] (int32).
"""
import numpy as np
import torch

import oracle_np as O
import _xneg_reference as XR

B1, B2, EPS = 0.9, 0.999, 1e-8


def f32(x):
    return float(np.float32(x))


def fused_offsets(vocab_n, vocab_c):
    """first fused row of every notice key, then of every company key (the store holds the notice tower's tables first)"""
    return np.cumsum([0] + list(vocab_n[:-1])), sum(vocab_n) + np.cumsum([0] + list(vocab_c[:-1]))


def company_side(batch):
    """the company tower's input of the step: the batch's companies, then the extras"""
    return (np.concatenate([batch["company_dense"], batch["neg_dense"]], 0),
            np.concatenate([np.asarray(batch["company_ids"]), np.asarray(batch["neg_ids"])], 0))


def make_batch(B, M, vocab_n, vocab_c, din_n, din_c, seed, decorated=False):
    """A batch with extras whose ids exercise every way a table row can be carried.  Per company key of V rows: the batch and the
    extras draw from [0, V - 3) (V small against B: batch companies repeat each other, extras repeat batch companies), batch row 1
    is a copy of batch row 0, the first extra (M >= 2) a copy of batch row 0, the last extra a copy of batch row 1 but for its first
    key, whose row V - 2 it alone carries; row V - 1 of every key, and V - 3, are carried by nobody.  Notice keys draw from [0, V - 2),
    rows 3 and 4 alike.  decorated: logQ on the three sides, and entity ids -- the companies' and the extras' are their first key's
    id, so an extra that repeats a batch company is masked for that company's rows; notices 3 and 4 are one entity."""
    r = np.random.default_rng(seed)
    assert B >= 5 and M >= 1 and min(vocab_c) >= 5 and min(vocab_n) >= 4
    ids_n = np.stack([r.integers(0, v - 2, B) for v in vocab_n], axis=1).astype(np.int64)
    ids_c = np.stack([r.integers(0, v - 3, B) for v in vocab_c], axis=1).astype(np.int64)
    ids_x = np.stack([r.integers(0, v - 3, M) for v in vocab_c], axis=1).astype(np.int64)
    ids_n[4], ids_c[1] = ids_n[3], ids_c[0]
    if M >= 2:
        ids_x[0] = ids_c[0]
    ids_x[M - 1] = ids_c[1]
    ids_x[M - 1, 0] = vocab_c[0] - 2
    b = {"notice_ids": ids_n, "company_ids": ids_c, "neg_ids": ids_x,
         "notice_dense": r.standard_normal((B, din_n)).astype(np.float32),
         "company_dense": r.standard_normal((B, din_c)).astype(np.float32),
         "neg_dense": r.standard_normal((M, din_c)).astype(np.float32)}
    if decorated:
        b.update(lq_n=r.uniform(-6.0, 0.0, B).astype(np.float32), lq_c=r.uniform(-6.0, 0.0, B).astype(np.float32),
                 lq_x=r.uniform(-6.0, 0.0, M).astype(np.float32), ent_n=np.arange(B, dtype=np.int32),
                 ent_c=ids_c[:, 0].astype(np.int32), ent_x=ids_x[:, 0].astype(np.int32))
        b["ent_n"][4] = b["ent_n"][3]
    return b


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a))


def xneg_step(state, batch, keys_n, keys_c, vocab_n, vocab_c, temperature=1.0, mode="fp32", rounding=None, dropout=None,
              proj_grad="direct"):
    """One forward + backward in train mode.  mode: the score arithmetic ("fp32" | "bf16"); rounding: the towers' (None | "bf16");
    dropout: (p, {(tower prefix, block): keep}) as oracle_np.tower_fwd takes it, the company side's masks over B + M rows.
    Returns loss, the embedding blocks N / C / X, grads {state key: array} (tables dense), bn_updates, the caches of both towers
    and the sparse table gradient (rows_n, grad_n, rows_c, grad_c) over the fused row space."""
    if rounding not in (None, "bf16"):
        raise ValueError(f"rounding must be None or 'bf16', got {rounding!r}")
    q = O.q_bf16 if rounding == "bf16" else None
    B = batch["notice_dense"].shape[0]
    dense_c, ids_c = company_side(batch)
    ne, cn, bn_n = O.tower_fwd(state, O.NT, keys_n, vocab_n, batch["notice_dense"], np.asarray(batch["notice_ids"]).reshape(-1), True,
                               np.float64, q, dropout)
    cx, cc, bn_c = O.tower_fwd(state, O.CT, keys_c, vocab_c, dense_c, ids_c.reshape(-1), True, np.float64, q, dropout)
    loss, dN, dC, dX = XR.reference(_t(ne), _t(cx[:B]), _t(cx[B:]), 1.0 / float(temperature), mode, _t(batch.get("ent_n")),
                                    _t(batch.get("ent_c")), _t(batch.get("ent_x")), _t(batch.get("lq_n")), _t(batch.get("lq_c")),
                                    _t(batch.get("lq_x")))
    g = O.tower_bwd(cn, dN.numpy(), O.NT, keys_n, vocab_n, "dense", proj_grad)
    g2 = O.tower_bwd(cc, np.concatenate([dC.numpy(), dX.numpy()], 0), O.CT, keys_c, vocab_c, "dense", proj_grad)
    dcat_n, dcat_c = g.pop("_d_concat"), g2.pop("_d_concat")
    offs_n, offs_c = fused_offsets(vocab_n, vocab_c)
    E = cn["E"]
    rn, gn = O.embed_grad_sparse(dcat_n, cn["ids"], offs_n, E)
    rc, gc = O.embed_grad_sparse(dcat_c, cc["ids"], offs_c, E)
    return {"loss": loss, "N": ne, "C": cx[:B], "X": cx[B:], "grads": {**g, **g2}, "bn_updates": {**bn_n, **bn_c},
            "cache_n": cn, "cache_c": cc, "rows": (rn, gn, rc, gc)}


def block_stats(cache):
    """per hidden block (mean, rstd) of the BatchNorm batch statistics of an oracle_np.tower_fwd cache"""
    return [(np.maximum(blk["pre"], 0).mean(axis=0), blk["rstd"]) for blk in cache["blocks"]]


def scatter_rows(rows, grad_rows, R):
    """dense [R, E] image of a sparse gradient: what a row list that misses rows leaves at zero"""
    out = np.zeros((R, grad_rows.shape[1]), dtype=np.float64)
    out[np.asarray(rows, dtype=np.int64)] = grad_rows
    return out


def adam_first_step(p0, g, lr, wd):
    """f64 Adam at step 1 from zero moments with the f32 hyper-parameters the kernels see; returns (p, m, v)"""
    p = np.asarray(p0, dtype=np.float64).copy()
    m, v = np.zeros_like(p), np.zeros_like(p)
    O.adam_step(p, np.asarray(g, dtype=np.float64), m, v, 1, f32(lr), f32(B1), f32(B2), f32(EPS), f32(wd))
    return p, m, v


def sparse_adam_first_step(table0, rows, grad_rows, lr, wd):
    """row-sparse Adam at step 1 over the fused table [R, E] from zero moments; returns (table, m, v) in f64"""
    t = np.asarray(table0, dtype=np.float64).copy()
    m, v = np.zeros_like(t), np.zeros_like(t)
    O.sparse_adam_rows(t, m, v, 1, rows, np.asarray(grad_rows, dtype=np.float64), f32(lr), f32(B1), f32(B2), f32(EPS), f32(wd))
    return t, m, v

