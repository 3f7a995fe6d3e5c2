"""numpy model of the duplicate-row plans over a pooled lookup's positions (tt_dedup_plan / tt_dedup_plan_pad) and of the ordered
f32 sums the gradient forms from them.

A plan over `rows` (one fused row per position): sorted_src = the positions in a STABLE ascending sort by row, unique_rows the
distinct rows ascending, seg_offsets[u] where row u's run starts in sorted_src (seg_offsets[U] its end), n_unique = U.  The
padded plan takes keys in [0, pad_row]: the key pad_row sorts last, stays in unique_rows / seg_offsets behind the real rows and
is not counted, so seg_offsets[n_unique] is still the end of the last real row.
"""
import numpy as np


def plan(rows):
    rows = np.asarray(rows, dtype=np.int64).reshape(-1)
    sorted_src = np.argsort(rows, kind="stable")
    keys = rows[sorted_src]
    heads = np.flatnonzero(np.concatenate([[True], keys[1:] != keys[:-1]])) if rows.size else np.zeros(0, np.int64)
    return sorted_src, keys[heads], np.concatenate([heads, [rows.size]]).astype(np.int64), int(heads.size)


def padded_plan(rows, pad_row):
    """plan() over keys in [0, pad_row] with the pad key left out of n_unique"""
    rows = np.asarray(rows, dtype=np.int64).reshape(-1)
    assert rows.size == 0 or (rows.min() >= 0 and rows.max() <= pad_row)
    sorted_src, uniq, seg, n = plan(rows)
    if n and uniq[-1] == pad_row:
        n -= 1
    return sorted_src, uniq, seg, n


def ordered_sums(sorted_src, seg, n_unique, contrib):
    """per distinct row the f32 sum of contrib[position] in the plan's order, one rounding per addition: [n_unique, E]"""
    contrib = np.asarray(contrib, dtype=np.float32)
    out = np.zeros((n_unique, contrib.shape[1]), np.float32)
    for u in range(n_unique):
        acc = np.zeros(contrib.shape[1], np.float32)
        for p in sorted_src[seg[u]:seg[u + 1]]:
            acc = (acc + contrib[p]).astype(np.float32)
        out[u] = acc
    return out


def with_pads(rows, pad_row, capacity_layout):
    """`rows` (the live positions of all sides, side after side) laid out in capacity space.  capacity_layout: per side
    (live count, capacity).  Returns (rows in capacity space with pad_row at the pads, live position -> capacity position)."""
    out, where, at, base = [], [], 0, 0
    for n, cap in capacity_layout:
        assert cap >= n
        out += [np.asarray(rows[at:at + n], dtype=np.int64), np.full(cap - n, pad_row, np.int64)]
        where.append(base + np.arange(n))
        at, base = at + n, base + cap
    return np.concatenate(out), np.concatenate(where) if where else np.zeros(0, np.int64)
