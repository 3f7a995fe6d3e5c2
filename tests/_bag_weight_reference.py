"""numpy f64 reference of the WEIGHTED pooled lookup (one f32 weight per id) and of its row gradient.

The wire format and the id decoding are tests/_bag_reference.py's.  weights: f32 [nnz] in the order of ids -- the values a kernel
was handed, taken to f64 exactly.  Bag (b, k) over positions p0 < p1 < ... of length L:
  sum   out = w_p0 * row_p0 + w_p1 * row_p1 + ...
  mean  that sum / L  (the divisor is the NUMBER of ids, not the sum of the weights)
and the row of position P receives c_P * d_out[slot of P], c_P = w_P * (1 / L for a mean key, else 1).  inv_len: the f32 per-slot
values a kernel was handed instead of the exact 1 / L (then c_P = w_P * inv_len[slot], the product exact in f64).
"""
import numpy as np

import _bag_reference as R
import oracle_np as O


def _weights(weights, n):
    w = np.asarray(weights, dtype=np.float32).reshape(-1)[:n].astype(np.float64)
    assert w.size == n, f"{w.size} weights for {n} covered positions"
    return w


def weighted_forward(table, ids, lengths, key_offsets, vocabs, pooling, weights):
    """table [R, E] -> (pooled [B, K*E] f64, sum of |w x| / divisor [B, K*E] f64 -- the error scale of a bag --, slots, rows)."""
    table = np.asarray(table, dtype=np.float64)
    lengths = np.asarray(lengths, dtype=np.int64).reshape(-1)
    K, E = len(vocabs), table.shape[1]
    slots, rows = R.positions(ids, lengths, key_offsets, vocabs)
    x = table[rows] * _weights(weights, slots.size)[:, None]
    out = np.zeros((lengths.size, E))
    mag = np.zeros((lengths.size, E))
    np.add.at(out, slots, x)
    np.add.at(mag, slots, np.abs(x))
    w = R.slot_weights(lengths, pooling)[:, None]
    B = lengths.size // K
    return (out * w).reshape(B, K * E), (mag * w).reshape(B, K * E), slots, rows


def weighted_backward(d_out, ids, lengths, key_offsets, vocabs, pooling, weights, inv_len=None):
    """d_out [B, K*E] -> per distinct fused row (ascending): (rows [U], gradient [U, E] f64, sum of |c x| [U, E], count [U])."""
    lengths = np.asarray(lengths, dtype=np.int64).reshape(-1)
    K = len(vocabs)
    E = d_out.shape[1] // K
    rows, vals = contributions(d_out, ids, lengths, key_offsets, vocabs, pooling, weights, inv_len)
    if rows.size == 0:
        return rows, np.zeros((0, E)), np.zeros((0, E)), np.zeros(0, np.int64)
    return O.row_sums_f64(rows, vals)


def contributions(d_out, ids, lengths, key_offsets, vocabs, pooling, weights, inv_len=None):
    """(fused row, c_P * d_out[slot of P]) of every covered position, in position order: what several sides concatenate before
    oracle_np.row_sums_f64"""
    lengths = np.asarray(lengths, dtype=np.int64).reshape(-1)
    E = d_out.shape[1] // len(vocabs)
    slots, rows = R.positions(ids, lengths, key_offsets, vocabs)
    sw = R.slot_weights(lengths, pooling) if inv_len is None else np.asarray(inv_len, dtype=np.float32).reshape(-1).astype(np.float64)
    c = _weights(weights, slots.size) * sw[slots]
    return rows, np.asarray(d_out, dtype=np.float64).reshape(lengths.size, E)[slots] * c[:, None]
