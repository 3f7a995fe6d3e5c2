"""tt_embed_bag_weight_grad on the MI355X through ops.bag_weight_grad: the gradient for a pooled lookup's per-id weights,

    g[P] = c(slot of P) * < d_out[slot of P, :], table[row of P, :] >,

against the f64 reference of tests/_bag_weight_grad_reference.py over the SAME f32 / bf16 inputs and the f32 inv_len the lookup
formed.  Inputs are standard normal (magnitude about 1: no product underflows).

Bound: |g - g64| <= gamma(E + 2) * |c| * sum_e |d_e x_e|, gamma(k) = k u / (1 - k u), u = 2^-24.  The kernel forms E products
and adds them -- each lane one multiply and three fused multiply-adds over its 16-byte piece, then a tree over the lane group --
so every term passes through at most E roundings whatever the order (a fused multiply-add rounds once, fewer than the multiply
and the add the bound allows), and the product with c rounds once more: E + 1 <= E + 2.

Shapes: E in {4, 12, 64, 256} -- one lane, a lane group of 3 lanes in 4, 16 lanes, a whole wave; B in {5, 67}; two sides of K = 3
keys pooled sum / mean / sum; lengths from {0, 1, 2, 3, 8, 9} plus one bag of 300 ids (which the flat walk spreads over lane
groups); ids out of range on both ends (clamped by the lookup); an id repeated inside a bag; ids behind the last bag (trailing);
sources f32 and bf16, column views of wider buffers (row stride > K*E).
"""
import numpy as np
import pytest
import torch

import _bag_weight_grad_reference as G
from test_gpu_embed_bag import U24
from test_gpu_parity import DEV, tt  # noqa: F401  (tt: the module fixture)

from jodalrob_twotower_amd import _lib as _L

pytestmark = pytest.mark.gpu

ES = [4, 12, 64, 256]
BS = [5, 67]
K = 3
POOLING = ["sum", "mean", "sum"]
VOCABS = [[40, 97, 23], [31, 64, 150]]
LENGTHS = [0, 1, 2, 3, 8, 9]
LONG = 300
TRAILING = 5
H0 = 8                                                         # the sources start at column 8 of buffers 4 columns wider still
GARBAGE = [1 << 40, -7, (1 << 62) + 5, -(1 << 50)]


def gamma(k):
    ku = np.asarray(k, dtype=np.float64) * U24
    return ku / (1 - ku)


class Case:
    def __init__(self, B, E, seed):
        rng = np.random.default_rng(seed)
        self.B, self.E, self.rng = B, E, rng
        self.offs, base = [], 0
        for v in VOCABS:
            self.offs.append(base + np.concatenate([[0], np.cumsum(v)[:-1]]).astype(np.int64))
            base += sum(v)
        self.table = rng.standard_normal((base, E)).astype(np.float32)
        self.lengths, self.ids = [], []
        for si in range(2):
            ln = rng.choice(LENGTHS, B * K).astype(np.int64)
            ln[0], ln[1] = 2, 3                                                  # (the repeated id below needs a bag of two)
            ln[K + 1 - si] = LONG                                                # side 0: a mean key's bag; side 1: a sum key's
            ids = np.concatenate([rng.integers(-3, VOCABS[si][s % K] + 3, int(n)) for s, n in enumerate(ln)]).astype(np.int64)
            ids[1] = ids[0]                                                      # an id repeated inside a bag
            ids[2], ids[3] = -5, VOCABS[si][1] + 7                               # out of range on both ends
            if si == 0:
                ids = np.concatenate([ids, rng.integers(0, 20, TRAILING)])        # ids behind the last bag: no bag covers them
            self.lengths.append(ln)
            self.ids.append(ids)
        self.nnz = [i.size for i in self.ids]
        self.live = [int(l.sum()) for l in self.lengths]

    def dev(self, a, dtype=None):
        t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
        return t if dtype is None else t.to(dtype)

    def sides(self, ops, capacity=False, pad=0):
        """ops.BagSide per side (capacity: the capacity form, `pad` stale garbage ids behind each side's ids)"""
        out = []
        for si in range(2):
            ids = self.ids[si]
            if capacity:
                ids = np.concatenate([ids[:self.live[si]], np.resize(np.array(GARBAGE, dtype=np.int64), pad)])
            buf = torch.full((self.B, H0 + K * self.E + 4), float("nan"), device=DEV)
            out.append(ops.BagSide(self.dev(ids), self.dev(self.lengths[si]), self.dev(self.offs[si]), self.dev(np.array(VOCABS[si], np.int64)),
                                   self.dev(np.array([ops.POOL_MODES[m] for m in POOLING], np.int32)), buf[:, H0:H0 + K * self.E], K,
                                   True, ids.size if capacity else None))
        return out

    def sources(self, dtype):
        """per side (d_out view [B, K*E] of a wider buffer, K) and the values as f32 numpy (bf16: what the kernel widens)"""
        srcs, vals = [], []
        for _ in range(2):
            buf = torch.from_numpy(self.rng.standard_normal((self.B, H0 + K * self.E + 4)).astype(np.float32)).to(DEV).to(dtype)
            view = buf[:, H0:H0 + K * self.E]
            assert view.stride(0) > K * self.E
            srcs.append((view, K))
            vals.append(view.float().cpu().numpy())
        return srcs, vals

    def reference(self, vals, inv_len):
        """per side (g64, scale) over the covered positions; inv_len: f32 [all slots] as the lookup formed it"""
        out = []
        for si in range(2):
            inv = inv_len[si * self.B * K:(si + 1) * self.B * K]
            out.append(G.weight_grad(self.table, vals[si], self.ids[si], self.lengths[si], self.offs[si], VOCABS[si], POOLING, inv_len=inv))
        return out


def _check(c, got, ref, si, covered, total):
    """the bound on the covered positions, exact zeros behind them"""
    g = got.cpu().numpy()
    assert g.dtype == np.float32 and g.shape == (total,)
    g64, scale = ref[si]
    assert g64.size == covered
    err = np.abs(g[:covered].astype(np.float64) - g64)
    bound = gamma(c.E + 2) * scale
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print(f"\n[bag_weight_grad] E={c.E} B={c.B} side {si}: max err / bound = {worst:.3f}, max |g| = {np.abs(g64).max():.3f}")
    assert (err <= bound).all()
    assert np.abs(g64).max() > 0.5                                               # (the check is not vacuous)
    assert not g[covered:].any() and not np.signbit(g[covered:]).any()           # exactly +0.0 where no bag covers


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("E", ES)
def test_weight_gradient_against_f64(tt, E, B, dtype):
    from jodalrob_twotower_amd import ops
    dev = torch.device(DEV)
    _L.check_device_errors(dev)
    c = Case(B, E, 4000 + 10 * E + B)
    table = c.dev(c.table)
    bag = ops.embed_bag_lookup(table, c.sides(ops), B, want_rows=True)
    assert bag.side_nnz == tuple(c.nnz) and bag.inv_len is not None
    srcs, vals = c.sources(dtype)
    ref = c.reference(vals, bag.inv_len.cpu().numpy())
    both = ops.bag_weight_grad(table, bag, srcs, B, [True, True])
    for si in range(2):
        _check(c, both[si], ref, si, c.live[si], c.nnz[si])
    assert c.nnz[0] == c.live[0] + TRAILING                                       # side 0's trailing ids were among the zeros
    again = ops.bag_weight_grad(table, bag, srcs, B, [True, True])
    for a, b in zip(both, again):
        assert np.array_equal(a.cpu().numpy().view(np.uint32), b.cpu().numpy().view(np.uint32))      # two runs: equal bits
    # one side asked for: the other's entry is None, and the requested one has the bits of the joint call
    only0 = ops.bag_weight_grad(table, bag, srcs, B, [True, False])
    only1 = ops.bag_weight_grad(table, bag, [(None, K), srcs[1]], B, [False, True])      # (a skipped side's source is not looked at)
    assert only0[1] is None and only1[0] is None
    assert torch.equal(only0[0], both[0]) and torch.equal(only1[1], both[1])
    assert ops.bag_weight_grad(table, bag, srcs, B, [False, False]) == [None, None]
    # every key summing (inv_len NULL): c = 1
    bag1 = bag._replace(inv_len=None)
    ref1 = c.reference(vals, np.ones(2 * B * K, np.float32))
    for si, g in enumerate(ops.bag_weight_grad(table, bag1, srcs, B, [True, True])):
        _check(c, g, ref1, si, c.live[si], c.nnz[si])
    torch.cuda.synchronize()
    _L.check_device_errors(dev)


@pytest.mark.parametrize("E", [12, 256])
def test_null_side_is_not_touched(tt, E):
    """The entry called directly: the second side's pointer NULL.  Both sides' outputs are parts of ONE guard-filled buffer, so an
    overrun of side 0's output, or any write for side 1, would land in the guard."""
    from jodalrob_twotower_amd import ops
    dev = torch.device(DEV)
    B = 67
    c = Case(B, E, 4500 + E)
    table = c.dev(c.table)
    bag = ops.embed_bag_lookup(table, c.sides(ops), B, want_rows=True)
    srcs, vals = c.sources(torch.float32)
    ref = c.reference(vals, bag.inv_len.cpu().numpy())
    guard = np.float32(-1234.5)
    buf = torch.full((c.nnz[0] + c.nnz[1] + 16,), float(guard), device=DEV)
    arr = (_L.GradSrc * 2)()
    for i, (d, k) in enumerate(srcs):
        arr[i] = _L.GradSrc(_L.ptr(d) if i == 0 else None, d.stride(0), k, _L.TT_F32)      # the skipped side: no source either
    nn = (_L.i64 * 2)(*c.nnz)
    garr = (_L.vp * 2)(_L.ptr(buf), None)
    _L.check(_L.load().tt_embed_bag_weight_grad(_L.ctx(dev), _L.ptr(table), table.shape[0], E, arr, 2, B, _L.ptr(bag.rows), _L.ptr(bag.bag_of),
                                                _L.ptr(bag.inv_len), nn, garr, _L.stream(dev)), "tt_embed_bag_weight_grad")
    torch.cuda.synchronize()
    _check(c, buf[:c.nnz[0]], ref, 0, c.live[0], c.nnz[0])
    assert bool((buf[c.nnz[0]:] == float(guard)).all())
    _L.check_device_errors(dev)


@pytest.mark.parametrize("E", [4, 64])
def test_capacity_form_pads_are_zero_and_live_ids_keep_their_bits(tt, E):
    """A capacity-form plan (ops._embed_bag_lookup_cap): live ids below the capacity, a stale tail of huge ids behind them.  The
    pads name the row one past the table: they get 0.0 and nothing is read through them.  The live positions run the arithmetic
    of the plain form on the same values (tt_bag_prepare's inv_len is the plain form's, bit for bit): equal bits."""
    from jodalrob_twotower_amd import ops
    dev = torch.device(DEV)
    _L.check_device_errors(dev)
    B, pad = 67, 37
    c = Case(B, E, 4700 + E)
    table = c.dev(c.table)
    plain = ops.embed_bag_lookup(table, c.sides(ops), B, want_rows=True)
    cap = ops.embed_bag_lookup(table, c.sides(ops, capacity=True, pad=pad), B, want_rows=True)
    caps = tuple(n + pad for n in c.live)
    assert cap.pad_row == table.shape[0] and cap.side_nnz == caps and cap.nnz == sum(caps)
    assert np.array_equal(plain.inv_len.cpu().numpy().view(np.uint32), cap.inv_len.cpu().numpy().view(np.uint32))
    at = 0
    for si in range(2):                                                            # the plan itself: pads behind the live positions
        rows, of = cap.rows[at:at + caps[si]].cpu().numpy(), cap.bag_of[at:at + caps[si]].cpu().numpy()
        assert (of[:c.live[si]] >= 0).all() and (of[c.live[si]:] == -1).all() and (rows[c.live[si]:] == table.shape[0]).all()
        at += caps[si]
    srcs, vals = c.sources(torch.bfloat16 if E == 64 else torch.float32)
    ref = c.reference(vals, cap.inv_len.cpu().numpy())
    g_plain = ops.bag_weight_grad(table, plain, srcs, B, [True, True])
    g_cap = ops.bag_weight_grad(table, cap, srcs, B, [True, True])
    for si in range(2):
        _check(c, g_cap[si], ref, si, c.live[si], caps[si])
        assert torch.equal(g_cap[si][:c.live[si]], g_plain[si][:c.live[si]])
    torch.cuda.synchronize()
    _L.check_device_errors(dev)


def test_refusals_before_any_launch(tt):
    from jodalrob_twotower_amd import ops
    B, E = 5, 12
    c = Case(B, E, 4900)
    table = c.dev(c.table)
    bag = ops.embed_bag_lookup(table, c.sides(ops), B, want_rows=True)
    srcs, _ = c.sources(torch.float32)
    with pytest.raises(ValueError, match="sources and"):
        ops.bag_weight_grad(table, bag, srcs[:1], B, [True])
    with pytest.raises(ValueError, match="sources and"):
        ops.bag_weight_grad(table, bag, srcs, B, [True])
    with pytest.raises(ValueError, match=r"\[B, K\*E\] view"):
        ops.bag_weight_grad(table, bag, [(srcs[0][0][:, :-4], K), srcs[1]], B, [True, True])
    with pytest.raises(ValueError, match="inv_len"):
        ops.bag_weight_grad(table, bag._replace(inv_len=bag.inv_len[:-1]), srcs, B, [True, True])
    with pytest.raises(ValueError, match="pad row"):
        ops.bag_weight_grad(table, bag._replace(pad_row=3), srcs, B, [True, True])
    # widths the bag kernels do not serve: TT_ERR_UNSUPPORTED from the entry itself
    for bad_e in (6, 260):
        t = torch.zeros((8, bad_e), device=DEV)
        one = ops.BagPlan(torch.zeros(4, dtype=torch.int32, device=DEV), torch.zeros(4, dtype=torch.int32, device=DEV), None, 4)
        with pytest.raises(_L.TwoTowerHipError, match=r"multiple of 4 in \[4, 256\]"):
            ops.bag_weight_grad(t, one, [(torch.zeros((1, bad_e), device=DEV), 1)], 1, [True])
