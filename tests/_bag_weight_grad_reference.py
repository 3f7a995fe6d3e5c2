"""numpy f64 references of the gradient FOR a pooled lookup's per-id weights and of learned position weights.

The wire format and the id decoding are tests/_bag_reference.py's.  For position P of bag (b, k), slot = b*K + k:

  g[P] = c * sum_e d_out[slot, e] * table[row_P, e],   c = 1 / L for a mean key (or the f32 inv_len a kernel was handed), else 1

-- the derivative of sum(d_out * pooled) with respect to w_P in pooled = c * sum_P w_P * row_P: the forward weight is no factor.
Position weights: position j of a bag of key k reads param[pw_offset[k] + min(j, pw_len[k] - 1)] (positions at or beyond max_len
share the last element; pw_offset -1: the key has none, its ids weigh 1), and the parameter's gradient sums g over its readers.
"""
import numpy as np

import _bag_reference as R


def weight_grad(table, d_out, ids, lengths, key_offsets, vocabs, pooling, inv_len=None):
    """-> (g f64 [covered positions], |c| * sum_e |d_e x_e| f64 [covered positions]: the error scale of a position)"""
    lengths = np.asarray(lengths, dtype=np.int64).reshape(-1)
    E = np.asarray(table).shape[1]
    slots, rows = R.positions(ids, lengths, key_offsets, vocabs)
    x = np.asarray(table, dtype=np.float64)[rows]
    d = np.asarray(d_out, dtype=np.float64).reshape(lengths.size, E)[slots]
    c = R.slot_weights(lengths, pooling) if inv_len is None else np.asarray(inv_len, dtype=np.float32).reshape(-1).astype(np.float64)
    c = c[slots]
    return c * (d * x).sum(axis=1), np.abs(c) * np.abs(d * x).sum(axis=1)


def position_index(lengths, K, pw_offset, pw_len):
    """per covered position: the parameter element it reads, -1 for a key without position weights"""
    lengths = np.asarray(lengths, dtype=np.int64).reshape(-1)
    slots = np.repeat(np.arange(lengths.size, dtype=np.int64), lengths)
    starts = np.concatenate([[0], np.cumsum(lengths)])[:-1]
    j = np.arange(slots.size, dtype=np.int64) - starts[slots]
    off = np.asarray(pw_offset, dtype=np.int64)[slots % K]
    ln = np.asarray(pw_len, dtype=np.int64)[slots % K]
    return np.where(off >= 0, off + np.minimum(j, np.maximum(ln, 1) - 1), -1)


def expand(param, index):
    """the weight of every covered position: a copy of its element (dtype kept), 1 where index is -1"""
    param = np.asarray(param)
    return np.where(index >= 0, param[np.maximum(index, 0)], param.dtype.type(1))


def reduce(g, index, n_param):
    """-> (sum of g f64 [n_param], sum of |g| [n_param], contributions [n_param]) over the positions that read each element"""
    g = np.asarray(g, dtype=np.float64).reshape(-1)[:index.size]
    live = index >= 0
    out, mag, cnt = np.zeros(n_param), np.zeros(n_param), np.zeros(n_param, np.int64)
    np.add.at(out, index[live], g[live])
    np.add.at(mag, index[live], np.abs(g[live]))
    np.add.at(cnt, index[live], 1)
    return out, mag, cnt
