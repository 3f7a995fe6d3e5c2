"""tt_embed_bag_fwd / tt_embed_bag_grad_bwd (pooled multi-valued lookups) against the f64 reference of tests/_bag_reference.py.

Shapes are small on purpose: B = 37 samples, two sides of K = 3 and K = 2 keys, E in {4, 32, 48} (lane groups of 1, 8 and 16
lanes, the last with idle lanes), vocabularies of 50 to 300 rows.  The exact cases draw table rows and gradients from
oracle_np.exact_grid_values (multiples of 2^-4, |x| <= 3/16): every partial sum is then exact in f32 whatever the order, so the
kernels must equal f64 BIT FOR BIT -- one dropped, doubled or misattributed position fails.  Mean pooling stays exact while the
bag lengths are powers of two: the weights 2^-k (k <= 8) make every product a multiple of 2^-12 and every sum stays far below
2^12, i.e. inside f32's 24 bits.  The random-normal cases check the rounding:
  forward   |got - f64| <= L * 2^-24 * sum|x| / divisor   (L - 1 roundings of the ordered sum, one of the division)
  backward  |got - f64| <= gamma_(n-1) * sum|w x|, gamma_k = k u / (1 - k u), u = 2^-24, for a row of n contributions whose
            products w x are exact (w = 1, or 2^-k for mean bags of 2^k ids): the first fused multiply-add then adds an exact
            product to zero and each later one rounds once.  A mean bag of any other length has a rounded weight w = fl(1 / L)
            and a product that is not exact: against the f64 sum over the SAME f32 weights that is one rounding more, gamma_n
            (test_backward_mean_any_length; the weight's own rounding is the caller's, not the kernel's).
  norm-wise under RANDN_NORM_BOUND = 1.6e-6, the bar tests/test_gpu_embed_grad_parity.py measured for the plain reduction.
"""
import numpy as np
import pytest
import torch

import _bag_reference as R
import oracle_np as O
from test_gpu_parity import DEV, tt  # noqa: F401  (tt: the module fixture)

from jodalrob_twotower_amd import _lib as _L

pytestmark = pytest.mark.gpu

B = 37
KS = [3, 2]
VOCABS = [[50, 300, 120], [200, 75]]
ES = [4, 32, 48]
U24 = 2.0 ** -24
RANDN_NORM_BOUND = 1.6e-6
FWD_LENGTHS = [0, 1, 2, 3, 5, 63, 64, 65, 200]
POW2_LENGTHS = [0, 1, 2, 4, 8, 64]
EDGE_COUNTS = [1, 15, 16, 17, 63, 64, 65, 128, 129]          # contributions per row: the 8-load trip and the 64-position chunk
# 14 power-of-two bag lengths that hold the 498 edge contributions (the other bags of that key are empty)
EDGE_POW2 = [128, 128, 64, 64, 32, 32, 16, 16, 8, 4, 2, 2, 1, 1]
assert sum(EDGE_POW2) == sum(EDGE_COUNTS) == 498


class Case:
    """Two sides of ragged bags over one fused table.  edge: key 1 of side 0 holds exactly EDGE_COUNTS contributions on its rows
    0..8 (spread over bags of random lengths, or of EDGE_POW2 lengths when pow2)."""

    def __init__(self, seed, E, pooling, length_set, edge=False, pow2=False, exact_table=True):
        rng = np.random.default_rng(seed)
        self.E, self.pooling = E, pooling
        self.offs, self.ids, self.lengths = [], [], []
        off = 0
        for si, (K, vs) in enumerate(zip(KS, VOCABS)):
            self.offs.append(off + np.concatenate([[0], np.cumsum(vs)[:-1]]).astype(np.int64))
            off += sum(vs)
            n = B * K
            # every value of the set occurs once per side; the other slots draw from its four smallest (keeps nnz small)
            ls = rng.choice(sorted(length_set)[:4], n).astype(np.int64)
            ls[rng.permutation(n)[:len(length_set)]] = length_set
            ls2 = ls.reshape(B, K)
            if edge and si == 0:
                if pow2:
                    ls2[:, 1] = rng.permutation(np.array(EDGE_POW2 + [0] * (B - len(EDGE_POW2))))
                else:
                    cuts = np.sort(rng.integers(0, 499, B - 1))
                    ls2[:, 1] = np.diff(np.concatenate([[0], cuts, [498]]))
            bags = []
            edge_ids = rng.permutation(np.repeat(np.arange(len(EDGE_COUNTS)), EDGE_COUNTS))
            taken = 0
            for b in range(B):
                for k in range(K):
                    L = int(ls2[b, k])
                    if edge and si == 0 and k == 1:
                        bags.append(edge_ids[taken:taken + L])
                        taken += L
                    else:
                        bags.append(rng.integers(-3, vs[k] + 3, L))              # out-of-range and negative ids included
            if not edge and len(length_set) > 4:
                five =np.flatnonzero(ls2.reshape(-1) == sorted(length_set)[4])[0]
                bags[five][:] = bags[five][0]                                   # one id repeated inside a bag
            self.lengths.append(ls2.reshape(-1))
            self.ids.append(np.concatenate(bags).astype(np.int64) if bags else np.zeros(0, np.int64))
        self.table_rows = off
        self.table = (O.exact_grid_values(rng, (off, E)) if exact_table else rng.standard_normal((off, E)).astype(np.float32))
        self.nnz = [len(i) for i in self.ids]
        self.rng = rng

    def reference(self):
        """per side (pooled, magnitude, global slots, fused rows)"""
        out, base = [], 0
        for si in range(2):
            o, m, sl, rows = R.bag_forward(self.table, self.ids[si], self.lengths[si], self.offs[si], VOCABS[si], self.pooling[si])
            out.append((o, m, sl + base, rows))
            base += B * KS[si]
        return out

    def sides(self, ops, out_dtype=torch.float32, h0=8, pad=4, fill=float("nan")):
        """ops.BagSide per side; the outputs are column-offset views into wider NaN-filled buffers with a padded row stride"""
        bufs, sides = [], []
        for si, K in enumerate(KS):
            buf = torch.full((B, h0 + K * self.E + pad), fill, dtype=out_dtype, device=DEV)
            pool = torch.tensor([ops.POOL_MODES[p] for p in self.pooling[si]], dtype=torch.int32, device=DEV)
            sides.append(ops.BagSide(torch.from_numpy(self.ids[si]).to(DEV), torch.from_numpy(self.lengths[si]).to(DEV),
                                     torch.from_numpy(self.offs[si]).to(DEV), torch.tensor(VOCABS[si], dtype=torch.int64, device=DEV),
                                     pool, buf[:, h0:h0 + K * self.E], K, any(p == "mean" for p in self.pooling[si])))
            bufs.append(buf)
        return sides, bufs

    def grad_reference(self, d_outs, weights=None):
        """(uniq, sums, abs_sums, counts) over both sides; d_outs: per side [B, K*E] f32 arrays"""
        rows, vals, base = [], [], 0
        for si in range(2):
            sl, r = R.positions(self.ids[si], self.lengths[si], self.offs[si], VOCABS[si])
            w = R.slot_weights(self.lengths[si], self.pooling[si]) if weights is None else weights[base:base + B * KS[si]].astype(np.float64)
            vals.append(d_outs[si].astype(np.float64).reshape(B * KS[si], self.E)[sl] * w[sl, None])
            rows.append(r)
            base += B * KS[si]
        return O.row_sums_f64(np.concatenate(rows), np.concatenate(vals))


SUM = [["sum"] * 3, ["sum"] * 2]
MEAN = [["mean"] * 3, ["mean"] * 2]
MIXED = [["mean", "sum", "mean"], ["sum", "mean"]]
# the backward's mean cases: EDGE_KEY, the key that holds the edge rows (1 .. 129 contributions), is a MEAN key, so the weighted
# multiply-add meets every trip and chunk boundary and the long-row finish
EDGE_KEY = 1                                                       # of side 0
MIXED_EDGE = [["sum", "mean", "mean"], ["sum", "mean"]]
assert MIXED_EDGE[0][EDGE_KEY] == "mean"


def _launches(fn):
    lib = _L.load()
    torch.cuda.synchronize()
    n0 = lib.tt_launch_count()
    fn()
    torch.cuda.synchronize()
    return int(lib.tt_launch_count() - n0)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).numpy()


def _srcs(c, exact, dtype=torch.float32, pad=4):
    """gradient sources per side: ([B, K*E] view of a padded buffer, K) and what they hold as f32 numpy"""
    srcs, vals = [], []
    for K in KS:
        d = O.exact_grid_values(c.rng, (B, K * c.E + pad)) if exact else c.rng.standard_normal((B, K * c.E + pad)).astype(np.float32)
        t = torch.from_numpy(d).to(DEV).to(dtype)
        srcs.append((t[:, :K * c.E], K))
        vals.append(t[:, :K * c.E].float().cpu().numpy())
    return srcs, vals


# ------------------------------------------------------------------------------------------- 1: degenerate bags
@pytest.mark.parametrize("E", ES)
@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_length_one_bags_equal_the_plain_lookup_and_gradient(tt, E, out_dtype):
    from jodalrob_twotower_amd import ops
    c = Case(100 + E, E, MIXED, [1])
    assert all((ls == 1).all() for ls in c.lengths)
    sides, bufs = c.sides(ops, out_dtype)
    assert _launches(lambda: None) == 0
    bag = None

    def fwd():
        nonlocal bag
        bag = ops.embed_bag_lookup(torch.from_numpy(c.table).to(DEV), sides, B, want_rows=True)
    assert _launches(fwd) == 1                                                 # one launch
    plain_bufs = [torch.full_like(b, float("nan")) for b in bufs]
    plain = [ops.LookupSide(s.ids, s.key_row_offset, s.key_vocab, pb[:, 8:8 + s.K * E], s.K) for s, pb in zip(sides, plain_bufs)]
    rows = ops.embed_lookup(torch.from_numpy(c.table).to(DEV), plain, B, want_rows=True)
    for got, want in zip(bufs, plain_bufs):
        assert np.array_equal(_bits(got), _bits(want))                         # NaN padding included
    assert torch.equal(bag.rows, rows)
    assert torch.equal(bag.bag_of, torch.arange(B * sum(KS), dtype=torch.int32, device=DEV))
    assert bag.inv_len is not None and bool((bag.inv_len == 1).all())
    if out_dtype == torch.bfloat16:
        return
    plan = ops.dedup_plan(rows, c.table_rows)
    bplan = ops.dedup_plan(bag.rows, c.table_rows)
    for src_dtype in (torch.float32, torch.bfloat16):
        srcs, _ = _srcs(c, exact=False, dtype=src_dtype)
        for mode in (ops.TT_GRAD_SPARSE, ops.TT_GRAD_DENSE_SET, ops.TT_GRAD_DENSE_ACC):
            n = rows.numel() if mode == ops.TT_GRAD_SPARSE else c.table_rows
            prior = torch.randn((n, E), device=DEV)
            a, b = prior.clone(), prior.clone()
            ops.embed_grad(plan, srcs, B, E, mode, a)
            ops.embed_bag_grad(bplan, bag, srcs, B, E, mode, b)
            assert np.array_equal(_bits(a), _bits(b)), (src_dtype, mode)
            b2 = prior.clone()
            ops.embed_bag_grad(bplan, bag._replace(inv_len=None), srcs, B, E, mode, b2)      # every key sums: no weights
            assert np.array_equal(_bits(a), _bits(b2)), (src_dtype, mode)


# ------------------------------------------------------------------------------------------- 2, 3: forward
def _forward(c, ops, out_dtype=torch.float32):
    sides, bufs = c.sides(ops, out_dtype)
    bag = ops.embed_bag_lookup(torch.from_numpy(c.table).to(DEV), sides, B, want_rows=True)
    torch.cuda.synchronize()
    return sides, bufs, bag


def _check_index_arrays(c, bag, ref):
    assert bag.nnz == sum(c.nnz)
    assert np.array_equal(bag.rows.cpu().numpy(), np.concatenate([r[3] for r in ref]).astype(np.int32))
    assert np.array_equal(bag.bag_of.cpu().numpy(), np.concatenate([r[2] for r in ref]).astype(np.int32))


def _check_padding(bufs, E, h0=8):
    for buf, K in zip(bufs, KS):
        f = buf.float()
        assert bool(torch.isnan(f[:, :h0]).all()) and bool(torch.isnan(f[:, h0 + K * E:]).all())      # every byte outside the view
        assert not bool(torch.isnan(f[:, h0:h0 + K * E]).any())


@pytest.mark.parametrize("E", ES)
def test_forward_sum_exact_grid(tt, E):
    from jodalrob_twotower_amd import ops
    c = Case(200 + E, E, SUM, FWD_LENGTHS)
    for ls in c.lengths:
        assert set(FWD_LENGTHS) <= set(ls.tolist())
    ref = c.reference()
    assert all(O.exact_sum_precondition(m) for _, m, _, _ in ref)
    sides, bufs, bag = _forward(c, ops)
    for si, (buf, K) in enumerate(zip(bufs, KS)):
        got = buf[:, 8:8 + K * E].cpu().numpy()
        assert np.array_equal(got.astype(np.float64), ref[si][0])
        empty = np.repeat(c.lengths[si].reshape(B, K) == 0, E, axis=1)
        assert empty.any() and not got[empty].any()                                                  # empty bags are zeros
    _check_padding(bufs, E)
    _check_index_arrays(c, bag, ref)
    # bf16 output: the RNE rounding of the exact sums; a second call gives the same bits
    _, bufs16, _ = _forward(c, ops, torch.bfloat16)
    _, bufs16b, _ = _forward(c, ops, torch.bfloat16)
    for si, (buf, K) in enumerate(zip(bufs16, KS)):
        want = torch.from_numpy(ref[si][0].astype(np.float32)).to(torch.bfloat16)
        assert torch.equal(buf[:, 8:8 + K * E].cpu(), want)
        assert np.array_equal(_bits(buf), _bits(bufs16b[si]))
    _check_padding(bufs16, E)


@pytest.mark.parametrize("E", ES)
def test_forward_mean_power_of_two_lengths_exact(tt, E):
    from jodalrob_twotower_amd import ops
    c = Case(300 + E, E, MIXED, POW2_LENGTHS)
    ref = c.reference()
    sides, bufs, bag = _forward(c, ops)
    for si, (buf, K) in enumerate(zip(bufs, KS)):
        assert np.array_equal(buf[:, 8:8 + K * E].cpu().numpy().astype(np.float64), ref[si][0])
    _check_padding(bufs, E)
    _check_index_arrays(c, bag, ref)
    w = np.concatenate([R.slot_weights(c.lengths[si], c.pooling[si]) for si in range(2)])
    assert np.array_equal(bag.inv_len.cpu().numpy().astype(np.float64), w)


@pytest.mark.parametrize("E", ES)
def test_forward_mean_random_normal_within_the_rounding_bound(tt, E):
    from jodalrob_twotower_amd import ops
    c = Case(400 + E, E, MIXED, FWD_LENGTHS, exact_table=False)
    ref = c.reference()
    _, bufs, _ = _forward(c, ops)
    _, bufs16, _ = _forward(c, ops, torch.bfloat16)
    worst = 0.0
    for si, K in enumerate(KS):
        L = np.repeat(c.lengths[si].reshape(B, K), E, axis=1).astype(np.float64)
        bound = L * U24 * ref[si][1]
        got = bufs[si][:, 8:8 + K * E].cpu().numpy().astype(np.float64)
        err = np.abs(got - ref[si][0])
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        print(f"\n[embed_bag fwd randn E={E} side={si}] worst err / bound = {worst:.3f}")
        assert (err <= bound).all()
        # bf16: the RNE rounding of some value inside the bound (rounding is monotone: between the roundings of the bound's ends)
        lo = torch.from_numpy((ref[si][0] - bound).astype(np.float32)).to(torch.bfloat16).float().numpy()
        hi = torch.from_numpy((ref[si][0] + bound).astype(np.float32)).to(torch.bfloat16).float().numpy()
        g16 = bufs16[si][:, 8:8 + K * E].float().cpu().numpy()
        assert ((lo <= g16) & (g16 <= hi)).all()
        assert np.array_equal(g16, torch.from_numpy(got.astype(np.float32)).to(torch.bfloat16).float().numpy())


# ------------------------------------------------------------------------------------------- 4, 5: backward
def _check_backward(c, ops, srcs, vals, exact, weights=None, extra_rounding=0):
    sides, bufs, bag = _forward(c, ops)
    plan = ops.dedup_plan(bag.rows, c.table_rows)
    U = int(plan.n_unique.item())
    if weights is not None:
        weights = bag.inv_len.cpu().numpy()
    uniq, sums, abs_sums, counts = c.grad_reference(vals, weights)
    assert U == len(uniq) and np.array_equal(plan.unique_rows[:U].cpu().numpy(), uniq)               # the distinct-row set
    assert np.array_equal(np.diff(plan.seg_offsets[:U + 1].cpu().numpy()), counts)
    E, nnz = c.E, bag.nnz
    ku = np.maximum(counts - 1 + extra_rounding, 0)[:, None] * U24
    rigorous = ku / (1 - ku) * abs_sums

    def compare(got, want, what):
        if exact:
            bad = got.astype(np.float64) != want
            assert not bad.any(), (what, int(bad.any(1).sum()), "rows differ; counts", np.unique(counts[bad.any(1)])[:10])
            return
        err = np.abs(got.astype(np.float64) - want)
        norm = float(np.linalg.norm(err) / np.linalg.norm(want))
        print(f"\n[embed_bag bwd randn E={E} {what}] norm {norm:.3e} worst err / rigorous {float((err / np.maximum(rigorous, 1e-300)).max()):.3f}")
        assert (err <= rigorous).all(), what
        assert norm <= RANDN_NORM_BOUND, (what, norm)

    out = torch.full((nnz, E), float("nan"), device=DEV)
    assert _launches(lambda: ops.embed_bag_grad(plan, bag, srcs, B, E, ops.TT_GRAD_SPARSE, out)) == 4
    g = out.cpu().numpy()
    assert np.isnan(g[U:]).all()                                                                      # rows >= U keep their sentinel
    compare(g[:U], sums, "sparse")
    sparse_bits = _bits(out[:U])
    prior = O.exact_grid_values(c.rng, (c.table_rows, E)) if exact else c.rng.standard_normal((c.table_rows, E)).astype(np.float32)
    untouched = np.ones(c.table_rows, bool)
    untouched[uniq] = False
    assert untouched.any()
    for mode, what in ((ops.TT_GRAD_DENSE_SET, "set"), (ops.TT_GRAD_DENSE_ACC, "acc")):
        dense = torch.from_numpy(prior).to(DEV)
        ops.embed_bag_grad(plan, bag, srcs, B, E, mode, dense)
        gd = dense.cpu().numpy()
        assert np.array_equal(gd[untouched].view(np.uint32), prior[untouched].view(np.uint32))       # untouched rows keep their bits
        if what == "set":
            compare(gd[uniq], sums, what)
        elif exact:
            assert O.exact_sum_precondition(abs_sums + np.abs(prior[uniq]))
            compare(gd[uniq], sums + prior[uniq], what)
        else:                                                        # f32(prior + f32 sum): the sparse result plus one rounding
            assert np.array_equal(gd[uniq], (g[:U] + prior[uniq]).astype(np.float32))
    again = torch.full((nnz, E), float("nan"), device=DEV)                                             # 5: reproducible
    ops.embed_bag_grad(plan, bag, srcs, B, E, ops.TT_GRAD_SPARSE, again)
    assert np.array_equal(_bits(again[:U]), sparse_bits)
    return counts


def edge_case(seed, E, pooling, pow2):
    """The backward's case: the edge rows sit on key EDGE_KEY of side 0.  In the mean cases that key pools by MEAN and its
    contributions carry the weights 1 / L of bags of 1 .. 128 ids -- asserted here, so that a sum key cannot stand in for it."""
    c = Case(seed, E, pooling, POW2_LENGTHS if pow2 else [0, 1, 2, 3, 5], edge=True, pow2=pow2)
    if pooling is not SUM:
        assert pooling[0][EDGE_KEY] == "mean"
        w = R.slot_weights(c.lengths[0], pooling[0]).reshape(B, KS[0])[:, EDGE_KEY]
        L = c.lengths[0].reshape(B, KS[0])[:, EDGE_KEY]
        assert L.sum() == sum(EDGE_COUNTS) and (L > 1).any() and (w[L > 1] < 1).all()
        if pow2:
            assert sorted(L[L > 0].tolist(), reverse=True) == EDGE_POW2 and set(w.tolist()) <= {2.0 ** -k for k in range(8)}
    return c


@pytest.mark.parametrize("E", ES)
@pytest.mark.parametrize("pooling,pow2", [(SUM, False), (MIXED_EDGE, True)], ids=["sum", "mean-pow2"])
@pytest.mark.parametrize("src_dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_backward_exact_grid(tt, E, pooling, pow2, src_dtype):
    from jodalrob_twotower_amd import ops
    c = edge_case(500 + E + pow2, E, pooling, pow2)
    srcs, vals = _srcs(c, exact=True, dtype=src_dtype)
    counts = _check_backward(c, ops, srcs, vals, exact=True)
    edge_rows = int(c.offs[0][1])
    uniq = np.unique(np.concatenate([R.positions(c.ids[si], c.lengths[si], c.offs[si], VOCABS[si])[1] for si in range(2)]))
    at = np.searchsorted(uniq, edge_rows + np.arange(len(EDGE_COUNTS)))
    assert counts[at].tolist() == EDGE_COUNTS


@pytest.mark.parametrize("E", ES)
@pytest.mark.parametrize("pooling,pow2", [(SUM, False), (MIXED_EDGE, True)], ids=["sum", "mean-pow2"])
def test_backward_random_normal_within_the_rounding_bound(tt, E, pooling, pow2):
    from jodalrob_twotower_amd import ops
    c = edge_case(600 + E + pow2, E, pooling, pow2)
    srcs, vals = _srcs(c, exact=False)
    _check_backward(c, ops, srcs, vals, exact=False)


@pytest.mark.parametrize("E", ES)
def test_backward_mean_any_length(tt, E):
    """Mean bags of lengths that are no power of two: the weights fl(1 / L) are rounded and the products are not exact, so every
    contribution rounds once -- gamma_n against the f64 sum over the same f32 weights (the module docstring derives it)."""
    from jodalrob_twotower_amd import ops
    c = edge_case(700 + E, E, MEAN, False)
    srcs, vals = _srcs(c, exact=False)
    _check_backward(c, ops, srcs, vals, exact=False, weights=True, extra_rounding=1)


# ------------------------------------------------------------------------------------------- 6: argument and device errors
def test_unsupported_shapes_are_refused_before_any_launch(tt):
    from jodalrob_twotower_amd import ops
    lib = _L.load()
    for E, h0, what in ((6, 8, "multiple of 4"), (260, 8, "multiple of 4"), (32, 2, "4-element aligned")):
        c = Case(800 + E, E, SUM, [0, 1, 2, 3, 5])
        sides, bufs = c.sides(ops, h0=h0)
        torch.cuda.synchronize()
        n0 = lib.tt_launch_count()
        with pytest.raises(_L.TwoTowerHipError, match=rf"status -4\).*{what}"):
            ops.embed_bag_lookup(torch.from_numpy(c.table).to(DEV), sides, B, want_rows=True)
        assert lib.tt_launch_count() == n0
    c = Case(801, 32, SUM, [0, 1, 2, 3, 5])
    sides, bufs, bag = _forward(c, ops)
    plan = ops.dedup_plan(bag.rows, c.table_rows)
    srcs, _ = _srcs(c, exact=True, pad=2)                                       # ld % 4 != 0
    out = torch.zeros((bag.nnz, 32), device=DEV)
    torch.cuda.synchronize()
    n0 = lib.tt_launch_count()
    with pytest.raises(_L.TwoTowerHipError, match=r"status -4\).*4-element aligned"):
        ops.embed_bag_grad(plan, bag, srcs, B, 32, ops.TT_GRAD_SPARSE, out)
    with pytest.raises(_L.TwoTowerHipError, match=r"status -1\).*bad mode"):
        ops.embed_bag_grad(plan, bag, _srcs(c, exact=True)[0], B, 32, ops.TT_GRAD_SPARSE | _L.TT_GRAD_PLANNED, out)
    assert lib.tt_launch_count() == n0


@pytest.mark.parametrize("how", ["decreasing", "beyond-nnz"])
def test_bad_offsets_raise_the_device_error_word(tt, how):
    """Offsets are a device array: the host cannot check them without a synchronisation.  A bag whose offsets decrease, or end
    beyond nnz, raises TT_DEVERR_BAG_OFFSETS, is treated as empty and reads nothing; the launch finishes normally, the bags in
    front of it are right, and the check then clears the word."""
    from jodalrob_twotower_amd import ops
    dev = torch.device(DEV)
    c = Case(900, 32, SUM, [0, 1, 2, 3, 5])
    ref = c.reference()
    bad_slot = 40
    if how == "decreasing":
        c.lengths[0][bad_slot] = -2                      # offsets[bad_slot + 1] < offsets[bad_slot]
    else:
        c.lengths[0][-1] += 1000                         # the last bag ends beyond nnz
        bad_slot = B * KS[0] - 1
    _L.check_device_errors(dev)                          # start clean
    sides, bufs, bag = _forward(c, ops)
    with pytest.raises(_L.TwoTowerHipError, match=r"status -5\).*device error word 0x8:.*bag offsets"):
        _L.check_device_errors(dev)
    got = bufs[0][:, 8:8 + KS[0] * 32].cpu().numpy().reshape(B * KS[0], 32)
    want = ref[0][0].reshape(B * KS[0], 32)
    assert np.array_equal(got[:bad_slot].astype(np.float64), want[:bad_slot]) and not got[bad_slot].any()
    assert np.array_equal(bufs[1][:, 8:8 + KS[1] * 32].cpu().numpy().astype(np.float64), ref[1][0])   # the other side is whole
    _L.check_device_errors(dev)                          # the word was cleared
