"""numpy f64 reference of the pooled multi-valued lookup (embedding bags) and of its scatter backward.

Wire format (sample-major, as the KJT): lengths[b*K + k] is the length of bag (b, k), ids the concatenation of all bags in that
slot order.  Key k owns rows [key_offsets[k], key_offsets[k] + vocabs[k]) of one fused table; ids are clamped into [0, V_k - 1]
(src/towers/cat_embed.py:117).  pooling[k] is "sum" or "mean"; an empty bag pools to zeros.
"""
import numpy as np

import oracle_np as O


def positions(ids, lengths, key_offsets, vocabs):
    """Per position p of `ids`: (slot of its bag, fused row).  Ids the lengths leave over are dropped."""
    lengths = np.asarray(lengths, dtype=np.int64).reshape(-1)
    K = len(vocabs)
    slots = np.repeat(np.arange(lengths.size, dtype=np.int64), lengths)
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)[:slots.size]
    k = slots % K
    hi = np.asarray(vocabs, dtype=np.int64)[k] - 1
    rows = np.asarray(key_offsets, dtype=np.int64)[k] + np.minimum(np.maximum(ids, 0), hi)
    return slots, rows


def slot_weights(lengths, pooling):
    """f64 weight of every slot's contributions: 1 for sum, 1 / length for mean (1 for an empty bag: nothing uses it)."""
    lengths = np.asarray(lengths, dtype=np.int64).reshape(-1)
    K = len(pooling)
    mean = np.tile(np.array([p == "mean" for p in pooling]), lengths.size // K)
    return np.where(mean & (lengths > 0), 1.0 / np.maximum(lengths, 1), 1.0)


def bag_forward(table, ids, lengths, key_offsets, vocabs, pooling):
    """table [R, E] -> (pooled [B, K*E] f64, sum of |x| / divisor [B, K*E] f64 -- the error scale of a bag --, slots, rows)."""
    table = np.asarray(table, dtype=np.float64)
    lengths = np.asarray(lengths, dtype=np.int64).reshape(-1)
    K, E = len(vocabs), table.shape[1]
    slots, rows = positions(ids, lengths, key_offsets, vocabs)
    x = table[rows]
    out = np.zeros((lengths.size, E))
    mag = np.zeros((lengths.size, E))
    np.add.at(out, slots, x)
    np.add.at(mag, slots, np.abs(x))
    w = slot_weights(lengths, pooling)[:, None]
    B = lengths.size // K
    return (out * w).reshape(B, K * E), (mag * w).reshape(B, K * E), slots, rows


def bag_backward(d_out, ids, lengths, key_offsets, vocabs, pooling, weights=None):
    """d_out [B, K*E] -> per distinct fused row (ascending): (rows [U], gradient [U, E] f64, sum of |w x| [U, E], count [U]).
    weights: the per-slot weights to use instead of the exact 1 / length (the f32 values a kernel was handed)."""
    lengths = np.asarray(lengths, dtype=np.int64).reshape(-1)
    K = len(vocabs)
    E = d_out.shape[1] // K
    slots, rows = positions(ids, lengths, key_offsets, vocabs)
    w = slot_weights(lengths, pooling) if weights is None else np.asarray(weights, dtype=np.float64).reshape(-1)
    vals = np.asarray(d_out, dtype=np.float64).reshape(lengths.size, E)[slots] * w[slots, None]
    if rows.size == 0:
        return rows, np.zeros((0, E)), np.zeros((0, E)), np.zeros(0, np.int64)
    return O.row_sums_f64(rows, vals)


def dense_grad(table_rows, E, uniq, sums):
    g = np.zeros((table_rows, E))
    g[uniq] = sums
    return g
