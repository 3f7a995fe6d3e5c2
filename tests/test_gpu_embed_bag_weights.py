"""Weighted bags on the MI355X: tt_embed_bag_fwd_w / tt_embed_bag_fwd_cap_w / tt_embed_bag_grad_bwd_w (one f32 weight per id)
through ops, against the unweighted entries and the f64 reference of tests/_bag_weight_reference.py.

Shapes are tests/test_gpu_embed_bag.py's (its Case is reused): B = 37, two sides of K = 3 and K = 2 keys, E in {4, 32, 48},
vocabularies of 50 to 300 rows, outputs that are column-offset views of NaN-filled padded buffers.

1  Ones are the unweighted path: 1 * x = x (a -0 included) and fma(1, x, acc) = acc + x, so weights of 1.0 -- on both sides, or
   on one side with NULL on the other -- give the bits of the unweighted entries in both directions.
2  Exact grid: table rows and gradients are multiples of 2^-4 with |x| <= 3/16 (oracle_np.exact_grid_values), weights come from
   {0, +-0.25, 0.5, 1, 2}: every product is a multiple of 2^-6 and at most 3/8 in magnitude, a 200-term sum stays below 2^7,
   so every partial sum is exact in f32 in any order and the kernels must equal f64 BIT FOR BIT.  Mean pooling stays exact on
   power-of-two lengths (the divisor, and inv_len = 2^-k with k <= 7 in the backward's coefficient w * inv_len, only shift).
3  Rounding, random normal tables and weights, against f64 over the same f32 weights, gamma_k = k u / (1 - k u), u = 2^-24:
     forward   |got - ref| <= gamma_(L+1) * sum|w x| / divisor    one rounding per multiply or multiply-add (L), one of the division
     backward  |got - ref| <= gamma_(n+1) * sum|c x|              one rounding in the coefficient product c = fl(w * inv_len), and
                                                                   every contribution passes through at most n roundings of the
                                                                   sum (chunked rows add partial sums: fewer per term, never more);
                                                                   the reference takes the f32 inv_len the kernel was handed
   and norm-wise under RANDN_NORM_BOUND = 1.6e-6, the bar of the unweighted bag tests.
4  The capacity form: garbage ids and NaN weights behind the live ones, w_out pre-filled with NaN.
5  Refusals before any launch.
"""
import ctypes

import numpy as np
import pytest
import torch

import _bag_reference as R
import _bag_weight_reference as W
import oracle_np as O
from test_gpu_embed_bag import (B, EDGE_COUNTS, EDGE_KEY, ES, KS, MEAN, MIXED, MIXED_EDGE, POW2_LENGTHS, RANDN_NORM_BOUND, SUM, U24,  # noqa: F401
                                VOCABS, Case, _bits, _launches, _srcs, edge_case)
from test_gpu_parity import DEV, tt  # noqa: F401  (tt: the module fixture)

from jodalrob_twotower_amd import _lib as _L

pytestmark = pytest.mark.gpu

FWD_LENGTHS = [0, 1, 2, 3, 5, 7, 8, 9, 63, 64, 65, 200]          # the 8-id trip and its edges
GRID_WEIGHTS = np.array([0.0, 0.25, -0.25, 0.5, 1.0, 2.0], dtype=np.float32)
GARBAGE = [1 << 40, -7, (1 << 62) + 5, -(1 << 50)]               # what a capacity id buffer's tail holds


def gamma(k):
    ku = np.asarray(k, dtype=np.float64) * U24
    return ku / (1 - ku)


def _weights(c, how):
    """per side f32 [nnz]: "grid" (GRID_WEIGHTS), "randn", or "ones\""""
    if how == "ones":
        return [np.ones(n, np.float32) for n in c.nnz]
    if how == "grid":
        return [c.rng.choice(GRID_WEIGHTS, n).astype(np.float32) for n in c.nnz]
    return [c.rng.standard_normal(n).astype(np.float32) for n in c.nnz]


def _with_weights(sides, ws):
    for s, w in zip(sides, ws):
        s.weights = None if w is None else torch.from_numpy(w).to(DEV)
    return sides


def _forward(c, ops, ws, out_dtype=torch.float32):
    sides, bufs = c.sides(ops, out_dtype)
    bag = ops.embed_bag_lookup(torch.from_numpy(c.table).to(DEV), _with_weights(sides, ws), B, want_rows=True)
    torch.cuda.synchronize()
    return sides, bufs, bag


def _reference(c, ws):
    """per side (pooled, magnitude, global slots, fused rows) of the weighted forward"""
    out, base = [], 0
    for si in range(2):
        o, m, sl, rows = W.weighted_forward(c.table, c.ids[si], c.lengths[si], c.offs[si], VOCABS[si], c.pooling[si], ws[si])
        out.append((o, m, sl + base, rows))
        base += B * KS[si]
    return out


def _grad_reference(c, vals, ws, inv_len=None):
    """(uniq, sums, abs_sums, counts) over both sides; inv_len: the f32 per-slot values the kernel was handed, all sides"""
    rows, contrib, base = [], [], 0
    for si in range(2):
        inv = None if inv_len is None else inv_len[base:base + B * KS[si]]
        r, v = W.contributions(vals[si], c.ids[si], c.lengths[si], c.offs[si], VOCABS[si], c.pooling[si], ws[si], inv)
        rows.append(r)
        contrib.append(v)
        base += B * KS[si]
    return O.row_sums_f64(np.concatenate(rows), np.concatenate(contrib))


def _view(buf, K, E, h0=8):
    return buf[:, h0:h0 + K * E]


# ------------------------------------------------------------------------------------------- 1: ones are the unweighted path
@pytest.mark.parametrize("E", ES)
@pytest.mark.parametrize("which", ["both", "side0-only", "side1-only"])
def test_ones_give_the_bits_of_the_unweighted_entries(tt, E, which):
    from jodalrob_twotower_amd import ops
    c = edge_case(1100 + E, E, MIXED_EDGE, False)                               # mean bags of any length: rounded 1 / L, rounded sums
    c.table = c.rng.standard_normal(c.table.shape).astype(np.float32)
    # a row of -0.0 pooled alone (a bag of one id, weight 1) must stay -0.0
    ls0 = c.lengths[0]
    slot = int(np.flatnonzero((ls0 == 1) & (np.arange(ls0.size) % KS[0] != EDGE_KEY))[0])
    sl, rows = R.positions(c.ids[0], ls0, c.offs[0], VOCABS[0])
    zero_row = int(rows[sl == slot][0])
    c.table[zero_row] = -0.0
    ones = _weights(c, "ones")
    ws = {"both": ones, "side0-only": [ones[0], None], "side1-only": [None, ones[1]]}[which]
    for out_dtype in (torch.float32, torch.bfloat16):
        _, bufs0, bag0 = _forward(c, ops, [None, None], out_dtype)
        assert bag0.pos_w is None                                               # no side has weights: the entries of before
        _, bufs1, bag1 = _forward(c, ops, ws, out_dtype)
        for a, b in zip(bufs0, bufs1):
            assert np.array_equal(_bits(a), _bits(b))                           # NaN padding included
        assert torch.equal(bag0.rows, bag1.rows) and torch.equal(bag0.bag_of, bag1.bag_of)
        assert np.array_equal(_bits(bag0.inv_len), _bits(bag1.inv_len))
        assert bag1.pos_w is not None and bag1.pos_w.numel() == sum(c.nnz) and bool((bag1.pos_w == 1.0).all())
        b, k = divmod(slot, KS[0])
        got = _view(bufs1[0], KS[0], E)[b, k * E:(k + 1) * E].float().cpu().numpy()
        assert (got == 0).all() and np.signbit(got).all()
    plan = ops.dedup_plan(bag0.rows, c.table_rows)
    for src_dtype in (torch.float32, torch.bfloat16):
        srcs, _ = _srcs(c, exact=False, dtype=src_dtype)
        for mode in (ops.TT_GRAD_SPARSE, ops.TT_GRAD_DENSE_SET, ops.TT_GRAD_DENSE_ACC):
            n = bag0.nnz if mode == ops.TT_GRAD_SPARSE else c.table_rows
            prior = torch.randn((n, E), device=DEV)
            a, b2 = prior.clone(), prior.clone()
            ops.embed_bag_grad(plan, bag0, srcs, B, E, mode, a)
            ops.embed_bag_grad(plan, bag1, srcs, B, E, mode, b2)
            assert np.array_equal(_bits(a), _bits(b2)), (src_dtype, mode)
            if mode != ops.TT_GRAD_DENSE_ACC:                                   # ... and with every key summing (inv_len NULL)
                a, b2 = prior.clone(), prior.clone()
                ops.embed_bag_grad(plan, bag0._replace(inv_len=None), srcs, B, E, mode, a)
                ops.embed_bag_grad(plan, bag1._replace(inv_len=None), srcs, B, E, mode, b2)
                assert np.array_equal(_bits(a), _bits(b2)), (src_dtype, mode, "no inv_len")


# ------------------------------------------------------------------------------------------- 2: exact grid
def _check_index_arrays(c, bag, ref, ws):
    assert bag.nnz == sum(c.nnz)
    assert np.array_equal(bag.rows.cpu().numpy(), np.concatenate([r[3] for r in ref]).astype(np.int32))
    assert np.array_equal(bag.bag_of.cpu().numpy(), np.concatenate([r[2] for r in ref]).astype(np.int32))
    want = np.concatenate([np.ones(n, np.float32) if w is None else w for w, n in zip(ws, c.nnz)])
    assert np.array_equal(bag.pos_w.cpu().numpy().view(np.uint32), want.view(np.uint32))      # w_out: the weights, verbatim


def _check_padding(bufs, E, h0=8):
    for buf, K in zip(bufs, KS):
        f = buf.float()
        assert bool(torch.isnan(f[:, :h0]).all()) and bool(torch.isnan(f[:, h0 + K * E:]).all())
        assert not bool(torch.isnan(f[:, h0:h0 + K * E]).any())


@pytest.mark.parametrize("E", ES)
@pytest.mark.parametrize("pooling,lengths", [(SUM, FWD_LENGTHS), (MIXED, POW2_LENGTHS)], ids=["sum", "mean-pow2"])
def test_forward_exact_grid(tt, E, pooling, lengths):
    from jodalrob_twotower_amd import ops
    c = Case(1200 + E + len(lengths), E, pooling, lengths)                      # (out-of-range and negative ids; one id repeated in a bag)
    for ls in c.lengths:
        assert set(lengths) <= set(ls.tolist())
    ws = _weights(c, "grid")
    if pooling is SUM:                                                          # the repeated id carries different weights
        for si in range(2):
            p0 = int(np.cumsum(c.lengths[si])[np.flatnonzero(c.lengths[si] == 5)[0]] - 5)
            assert len(set(c.ids[si][p0:p0 + 5])) == 1
            ws[si][p0:p0 + 5] = [2.0, -0.25, 0.5, 0.0, 1.0]
    ref = _reference(c, ws)
    assert all(float(m.max()) < 2.0 ** 7 for _, m, _, _ in ref)
    _, bufs, bag = _forward(c, ops, ws)
    for si, (buf, K) in enumerate(zip(bufs, KS)):
        got = _view(buf, K, E).cpu().numpy()
        assert np.array_equal(got.astype(np.float64), ref[si][0])
        empty = np.repeat(c.lengths[si].reshape(B, K) == 0, E, axis=1)
        assert empty.any() and not got[empty].any()                             # empty bags are zeros
    _check_padding(bufs, E)
    _check_index_arrays(c, bag, ref, ws)
    # one side without weights (NULL): its ids weigh 1
    half = [ws[0], None]
    ref_h = _reference(c, [ws[0], np.ones(c.nnz[1], np.float32)])
    _, bufs_h, bag_h = _forward(c, ops, half)
    for si, (buf, K) in enumerate(zip(bufs_h, KS)):
        assert np.array_equal(_view(buf, K, E).cpu().numpy().astype(np.float64), ref_h[si][0])
    _check_index_arrays(c, bag_h, ref_h, half)
    # bf16 output: the RNE rounding of the exact sums; a second call gives the same bits
    _, bufs16, _ = _forward(c, ops, ws, torch.bfloat16)
    _, bufs16b, _ = _forward(c, ops, ws, torch.bfloat16)
    for si, (buf, K) in enumerate(zip(bufs16, KS)):
        want = torch.from_numpy(ref[si][0].astype(np.float32)).to(torch.bfloat16)
        assert torch.equal(_view(buf, K, E).cpu(), want)
        assert np.array_equal(_bits(buf), _bits(bufs16b[si]))
    _check_padding(bufs16, E)


def _check_backward(c, ops, ws, srcs, vals, exact):
    _, _, bag = _forward(c, ops, ws)
    plan = ops.dedup_plan(bag.rows, c.table_rows)
    U = int(plan.n_unique.item())
    inv = None if bag.inv_len is None else bag.inv_len.cpu().numpy()
    uniq, sums, abs_sums, counts = _grad_reference(c, vals, ws, inv)
    assert U == len(uniq) and np.array_equal(plan.unique_rows[:U].cpu().numpy(), uniq)
    assert np.array_equal(np.diff(plan.seg_offsets[:U + 1].cpu().numpy()), counts)
    E, nnz = c.E, bag.nnz
    rigorous = gamma(counts + 1)[:, None] * abs_sums

    def compare(got, want, what):
        if exact:
            bad = got.astype(np.float64) != want
            assert not bad.any(), (what, int(bad.any(1).sum()), "rows differ; counts", np.unique(counts[bad.any(1)])[:10])
            return
        err = np.abs(got.astype(np.float64) - want)
        norm = float(np.linalg.norm(err) / np.linalg.norm(want))
        print(f"\n[embed_bag_w bwd randn E={E} {what}] norm {norm:.3e} worst err / bound {float((err / np.maximum(rigorous, 1e-300)).max()):.3f}")
        assert (err <= rigorous).all(), what
        assert norm <= RANDN_NORM_BOUND, (what, norm)

    out = torch.full((nnz, E), float("nan"), device=DEV)
    assert _launches(lambda: ops.embed_bag_grad(plan, bag, srcs, B, E, ops.TT_GRAD_SPARSE, out)) == 4      # the launches of the unweighted entry
    g = out.cpu().numpy()
    assert np.isnan(g[U:]).all()
    compare(g[:U], sums, "sparse")
    prior = O.exact_grid_values(c.rng, (c.table_rows, E)) if exact else c.rng.standard_normal((c.table_rows, E)).astype(np.float32)
    untouched = np.ones(c.table_rows, bool)
    untouched[uniq] = False
    assert untouched.any()
    for mode, what in ((ops.TT_GRAD_DENSE_SET, "set"), (ops.TT_GRAD_DENSE_ACC, "acc")):
        dense = torch.from_numpy(prior).to(DEV)
        ops.embed_bag_grad(plan, bag, srcs, B, E, mode, dense)
        gd = dense.cpu().numpy()
        assert np.array_equal(gd[untouched].view(np.uint32), prior[untouched].view(np.uint32))
        if what == "set":
            compare(gd[uniq], sums, what)
        elif exact:
            compare(gd[uniq], sums + prior[uniq], what)
        else:
            assert np.array_equal(gd[uniq], (g[:U] + prior[uniq]).astype(np.float32))
    again = torch.full((nnz, E), float("nan"), device=DEV)                      # reproducible
    ops.embed_bag_grad(plan, bag, srcs, B, E, ops.TT_GRAD_SPARSE, again)
    assert np.array_equal(_bits(again[:U]), _bits(out[:U]))
    return counts, uniq


def _assert_edge_counts(c, counts, uniq):
    at = np.searchsorted(uniq, int(c.offs[0][1]) + np.arange(len(EDGE_COUNTS)))
    assert counts[at].tolist() == EDGE_COUNTS


@pytest.mark.parametrize("E", ES)
@pytest.mark.parametrize("pooling,pow2", [(SUM, False), (MIXED_EDGE, True)], ids=["sum", "mean-pow2"])
@pytest.mark.parametrize("src_dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_backward_exact_grid(tt, E, pooling, pow2, src_dtype):
    """the EDGE_COUNTS rows (1 .. 129 contributions; in the mean case on a mean key with power-of-two bag lengths): the weighted
    multiply-add meets every trip and chunk boundary and the long-row finish"""
    from jodalrob_twotower_amd import ops
    c = edge_case(1300 + E + pow2, E, pooling, pow2)
    ws = _weights(c, "grid")
    srcs, vals = _srcs(c, exact=True, dtype=src_dtype)
    counts, uniq = _check_backward(c, ops, ws, srcs, vals, exact=True)
    _assert_edge_counts(c, counts, uniq)


# ------------------------------------------------------------------------------------------- 3: rounding
@pytest.mark.parametrize("E", ES)
def test_forward_random_normal_within_the_rounding_bound(tt, E):
    from jodalrob_twotower_amd import ops
    c = Case(1400 + E, E, MIXED, FWD_LENGTHS, exact_table=False)
    ws = _weights(c, "randn")
    ref = _reference(c, ws)
    _, bufs, bag = _forward(c, ops, ws)
    _, bufs16, _ = _forward(c, ops, ws, torch.bfloat16)
    err2 = ref2 = 0.0
    for si, K in enumerate(KS):
        L = np.repeat(c.lengths[si].reshape(B, K), E, axis=1).astype(np.float64)
        bound = gamma(L + 1) * ref[si][1]
        got = _view(bufs[si], K, E).cpu().numpy().astype(np.float64)
        err = np.abs(got - ref[si][0])
        print(f"\n[embed_bag_w fwd randn E={E} side={si}] worst err / bound = {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
        assert (err <= bound).all()
        err2 += float((err ** 2).sum())
        ref2 += float((ref[si][0] ** 2).sum())
        g16 = _view(bufs16[si], K, E).float().cpu().numpy()
        assert np.array_equal(g16, torch.from_numpy(got.astype(np.float32)).to(torch.bfloat16).float().numpy())
    norm = (err2 / ref2) ** 0.5
    print(f"[embed_bag_w fwd randn E={E}] norm {norm:.3e}")
    assert norm <= RANDN_NORM_BOUND
    _check_index_arrays(c, bag, ref, ws)


@pytest.mark.parametrize("E", ES)
@pytest.mark.parametrize("pooling", [SUM, MEAN], ids=["sum", "mean-any-length"])
def test_backward_random_normal_within_the_rounding_bound(tt, E, pooling):
    from jodalrob_twotower_amd import ops
    c = edge_case(1500 + E + (pooling is MEAN), E, pooling, False)
    c.table = c.rng.standard_normal(c.table.shape).astype(np.float32)
    ws = _weights(c, "randn")
    srcs, vals = _srcs(c, exact=False)
    counts, uniq = _check_backward(c, ops, ws, srcs, vals, exact=False)
    _assert_edge_counts(c, counts, uniq)


# ------------------------------------------------------------------------------------------- 4: the capacity form
def _cap_forward(c, ops, ws, caps, lengths=None):
    """tt_bag_prepare + tt_embed_bag_fwd_cap_w called on buffers this test owns: id tails of out-of-range garbage, weight tails of
    NaN, w_out pre-filled with NaN.  -> (output buffers, ops.BagPlan)"""
    lib, dev = _L.load(), torch.device(DEV)
    table = torch.from_numpy(c.table).to(DEV)
    sides, bufs = c.sides(ops)
    keep = []
    for si, s in enumerate(sides):
        tail = np.resize(np.asarray(GARBAGE, dtype=np.int64), max(caps[si] - c.nnz[si], 0))
        s.ids = torch.from_numpy(np.concatenate([c.ids[si], tail])[:caps[si]]).to(DEV)
        if lengths is not None:
            s.lengths = torch.from_numpy(lengths[si]).to(DEV)
        if ws[si] is not None:
            s.weights = torch.from_numpy(np.concatenate([ws[si], np.full(max(caps[si] - c.nnz[si], 0), np.nan, np.float32)])[:caps[si]]).to(DEV)
        s.capacity = caps[si]
    offs, inv_len = ops.bag_prepare([s.lengths for s in sides], [s.key_pool for s in sides], KS, B, caps)
    arr = (_L.BagSide * 2)()
    for i, (s, off) in enumerate(zip(sides, offs)):
        arr[i] = _L.BagSide(_L.ptr(s.ids), _L.ptr(off), _L.ptr(s.key_row_offset), _L.ptr(s.key_vocab), _L.ptr(s.key_pool), _L.ptr(s.out),
                            s.out.stride(0), caps[i], s.K, _L.TT_F32)
    cap = sum(caps)
    idx = torch.empty((2, max(cap, 1)), dtype=torch.int32, device=DEV)
    w_out = torch.full((max(cap, 1),), float("nan"), device=DEV)
    warr = (_L.vp * 2)(*[_L.ptr(s.weights) for s in sides])
    _L.check(lib.tt_embed_bag_fwd_cap_w(_L.ctx(dev), _L.ptr(table), table.shape[0], c.E, arr, 2, B, _L.ptr(idx[0]), _L.ptr(idx[1]), warr,
                                        _L.ptr(w_out), _L.stream(dev)), "tt_embed_bag_fwd_cap_w")
    torch.cuda.synchronize()
    keep += [offs, sides]
    return bufs, ops.BagPlan(idx[0, :cap], idx[1, :cap], inv_len, cap, table.shape[0], w_out[:cap])


@pytest.mark.parametrize("name", ["cap=nnz", "cap=4nnz", "one-side-without-ids", "one-side-without-weights"])
def test_capacity_form_equals_the_plain_weighted_form(tt, name):
    from jodalrob_twotower_amd import ops
    dev = torch.device(DEV)
    E = 32
    c = Case(1600 + len(name), E, MIXED, [0, 1, 2, 3, 5, 9], exact_table=False)
    if name == "one-side-without-ids":
        c.lengths[1][:] = 0
        c.ids[1] = np.zeros(0, np.int64)
        c.nnz[1] = 0
    ws = _weights(c, "randn")
    if name == "one-side-without-weights":
        ws[1] = None
    caps = {"cap=nnz": list(c.nnz), "cap=4nnz": [4 * n for n in c.nnz]}.get(name, [c.nnz[0] + 33, c.nnz[1] + 17])
    _L.check_device_errors(dev)                                                 # start clean
    _, bufs0, bag0 = _forward(c, ops, ws)
    bufs1, bag1 = _cap_forward(c, ops, ws, caps)
    _L.check_device_errors(dev)                                                 # nothing of the garbage tails was decoded
    for a, b in zip(bufs0, bufs1):
        assert np.array_equal(_bits(a), _bits(b))                               # pooled outputs, NaN padding around the views included
        assert bool(torch.isfinite(a[:, 8:-4]).all())                           # ... finite: no NaN weight of a tail was read
    # w_out: the weights on the covered positions, still NaN exactly on the pads
    w1, of1 = bag1.pos_w.cpu().numpy(), bag1.bag_of.cpu().numpy()
    live = np.zeros(sum(caps), bool)
    live[:c.nnz[0]] = True
    live[caps[0]:caps[0] + c.nnz[1]] = True
    assert np.array_equal(np.isnan(w1), ~live) and np.array_equal(of1 < 0, ~live)
    assert np.array_equal(w1[live].view(np.uint32), bag0.pos_w.cpu().numpy().view(np.uint32))
    assert np.array_equal(bag1.rows.cpu().numpy()[live], bag0.rows.cpu().numpy()) and bool((bag1.rows.cpu().numpy()[~live] == c.table_rows).all())
    # the gradient over the padded plan: the bits of the plain weighted form
    plan0, plan1 = ops.dedup_plan(bag0.rows, c.table_rows), ops.bag_dedup_plan(bag1, c.table_rows)
    U = int(plan0.n_unique.item())
    assert int(plan1.n_unique.item()) == U
    srcs, _ = _srcs(c, exact=False)
    for mode in (ops.TT_GRAD_SPARSE, ops.TT_GRAD_DENSE_SET, ops.TT_GRAD_DENSE_ACC):
        prior = torch.randn((c.table_rows, E), device=DEV)
        a = prior.clone() if mode != ops.TT_GRAD_SPARSE else torch.zeros((bag0.nnz, E), device=DEV)
        b = prior.clone() if mode != ops.TT_GRAD_SPARSE else torch.zeros((bag1.nnz, E), device=DEV)
        ops.embed_bag_grad(plan0, bag0, srcs, B, E, mode, a)
        ops.embed_bag_grad(plan1, bag1, srcs, B, E, mode, b)
        n = U if mode == ops.TT_GRAD_SPARSE else c.table_rows
        assert np.array_equal(_bits(a[:n]), _bits(b[:n])), mode
        assert bool(torch.isfinite(b[:n]).all())
    _L.check_device_errors(dev)


def test_capacity_form_refused_offsets_read_nothing_through_the_side(tt):
    """side 0's lengths total more than its capacity: tt_bag_prepare raises TT_DEVERR_BAG_OFFSETS and zeroes the side's offsets --
    its bags pool to zeros, none of its positions is covered (w_out stays NaN, bag_of -1) and nothing is read through it; side 1
    is whole."""
    from jodalrob_twotower_amd import ops
    dev = torch.device(DEV)
    E = 32
    c = Case(1700, E, SUM, [0, 1, 2, 3, 5], exact_table=False)
    ws = _weights(c, "randn")
    _, bufs0, bag0 = _forward(c, ops, ws)
    caps = [c.nnz[0] + 8, c.nnz[1] + 8]
    lengths = [c.lengths[0].copy(), c.lengths[1]]
    lengths[0][3] += 9                                                          # the total is one above the capacity
    _L.check_device_errors(dev)
    bufs1, bag1 = _cap_forward(c, ops, ws, caps, lengths)
    with pytest.raises(_L.TwoTowerHipError, match=r"status -5\).*device error word 0x8:.*bag offsets"):
        _L.check_device_errors(dev)
    assert not bool(_view(bufs1[0], KS[0], E).any())                            # every bag of the side counts as empty
    assert np.array_equal(_bits(bufs0[1]), _bits(bufs1[1]))
    w1, of1 = bag1.pos_w.cpu().numpy(), bag1.bag_of.cpu().numpy()
    assert np.isnan(w1[:caps[0]]).all() and (of1[:caps[0]] == -1).all() and bool((bag1.rows[:caps[0]] == c.table_rows).all())
    assert np.array_equal(w1[caps[0]:caps[0] + c.nnz[1]].view(np.uint32), ws[1].view(np.uint32)) and np.isnan(w1[caps[0] + c.nnz[1]:]).all()
    _L.check_device_errors(dev)                                                 # the word was cleared


# ------------------------------------------------------------------------------------------- 5: refusals before any launch
def test_bad_weights_are_refused_before_any_launch(tt):
    from jodalrob_twotower_amd import ops
    lib, dev = _L.load(), torch.device(DEV)
    c = Case(1800, 32, SUM, [0, 1, 2, 3, 5])
    table = torch.from_numpy(c.table).to(DEV)
    ws = _weights(c, "grid")
    bad = {"dtype": torch.from_numpy(ws[0]).to(DEV).double(), "length": torch.from_numpy(ws[0][:-1].copy()).to(DEV),
           "device": torch.from_numpy(ws[0]), "contiguous": torch.from_numpy(np.repeat(ws[0], 2)).to(DEV)[::2]}
    torch.cuda.synchronize()
    n0 = lib.tt_launch_count()
    for what, w in bad.items():
        sides, _ = c.sides(ops)
        sides[0].weights = w
        with pytest.raises(ValueError, match="bag weights must be a contiguous float32"):
            ops.embed_bag_lookup(table, sides, B, want_rows=True)
        sides[0].capacity, sides[1].capacity = c.nnz                             # ... and in the capacity form
        with pytest.raises(ValueError, match="bag weights must be a contiguous float32"):
            ops.embed_bag_lookup(table, sides, B, want_rows=False)
    # the entry itself: rows_out with a weighted side and no w_out
    sides, _ = c.sides(ops)
    _with_weights(sides, ws)
    offs = []
    arr = (_L.BagSide * 2)()
    for i, s in enumerate(sides):
        off = torch.zeros(B * s.K + 1, dtype=torch.int64, device=DEV)
        offs.append(off)
        arr[i] = _L.BagSide(_L.ptr(s.ids), _L.ptr(off), _L.ptr(s.key_row_offset), _L.ptr(s.key_vocab), _L.ptr(s.key_pool), _L.ptr(s.out),
                            s.out.stride(0), s.ids.numel(), s.K, _L.TT_F32)
    idx = torch.zeros((2, sum(c.nnz)), dtype=torch.int32, device=DEV)
    warr = (_L.vp * 2)(*[_L.ptr(s.weights) for s in sides])
    for entry in (lib.tt_embed_bag_fwd_w, lib.tt_embed_bag_fwd_cap_w):
        with pytest.raises(_L.TwoTowerHipError, match=r"status -1\).*needs w_out"):
            _L.check(entry(_L.ctx(dev), _L.ptr(table), table.shape[0], 32, arr, 2, B, _L.ptr(idx[0]), _L.ptr(idx[1]), warr, None, _L.stream(dev)), "fwd_w")
        with pytest.raises(_L.TwoTowerHipError, match=r"status -1\).*NULL weights array"):
            _L.check(entry(_L.ctx(dev), _L.ptr(table), table.shape[0], 32, arr, 2, B, None, None, None, None, _L.stream(dev)), "fwd_w")
    # what the unweighted entries refuse the weighted ones refuse too
    for E, h0, what in ((6, 8, "multiple of 4"), (32, 2, "4-element aligned")):
        c2 = Case(1800 + E, E, SUM, [0, 1, 2, 3, 5])
        sides, _ = c2.sides(ops, h0=h0)
        with pytest.raises(_L.TwoTowerHipError, match=rf"status -4\).*{what}"):
            ops.embed_bag_lookup(torch.from_numpy(c2.table).to(DEV), _with_weights(sides, _weights(c2, "grid")), B, want_rows=True)
    torch.cuda.synchronize()
    assert lib.tt_launch_count() == n0
    # the gradient: a pos_w of another size than the plan's positions
    _, _, bag = _forward(c, ops, ws)
    plan = ops.dedup_plan(bag.rows, c.table_rows)
    srcs, _ = _srcs(c, exact=True)
    out = torch.zeros((bag.nnz, 32), device=DEV)
    torch.cuda.synchronize()
    n0 = lib.tt_launch_count()
    with pytest.raises(ValueError, match="pos_w must hold one float32 per position"):
        ops.embed_bag_grad(plan, bag._replace(pos_w=bag.pos_w[:-1]), srcs, B, 32, ops.TT_GRAD_SPARSE, out)
    with pytest.raises(_L.TwoTowerHipError, match=r"status -4\).*4-element aligned"):
        ops.embed_bag_grad(plan, bag, _srcs(c, exact=True, pad=2)[0], B, 32, ops.TT_GRAD_SPARSE, out)
    assert lib.tt_launch_count() == n0
