"""The capacity form of the pooled lookup on the MI355X -- tt_bag_prepare, tt_embed_bag_fwd_cap, tt_dedup_plan_pad and the gradient
over them -- against today's exact entries (tt_embed_bag_fwd, tt_dedup_plan, tt_embed_bag_grad_bwd) on the live ids alone.

Everything is compared BIT FOR BIT: the capacity form only adds positions nobody reads (the pad row sorts last, is not counted
in n_unique, and the gradient and the optimiser visit the first n_unique rows), so the pooled outputs, n_unique, unique_rows[:U]
and every gradient must not change by one bit; tables and gradients are random normal, so a changed order of a row's sum shows.
Every capacity buffer's tail (behind the live ids) holds out-of-range garbage: reading one id of it would raise the row-range bit of
the device error word, which every test checks to be clean.

Shapes: B = 37 samples, two sides of 3 and 2 keys, E = 16 (the lookup's lane-group forms are tests/test_gpu_embed_bag.py's), small
vocabularies -- each case is one where the capacity form can go wrong (the parameter ids say which).
"""
import numpy as np
import pytest
import torch

import _bag_plan_reference as P
from test_gpu_parity import DEV, tt  # noqa: F401  (tt: the module fixture)

from jodalrob_twotower_amd import _lib as _L

pytestmark = pytest.mark.gpu

B, E = 37, 16
KS = [3, 2]
VOCABS = [[50, 300, 120], [200, 75]]
POOLING = [["mean", "sum", "mean"], ["sum", "mean"]]
GARBAGE = [1 << 40, -7, (1 << 62) + 5, -(1 << 50)]                # what a capacity buffer's tail holds


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).numpy()


class Case:
    """Two sides of ragged bags over one fused table; extra[i] = capacity of side i beyond its live ids"""

    def __init__(self, seed, extra, lengths=(0, 1, 2, 3, 5), vocabs=VOCABS, tail_empty=0, last_row=False):
        rng = np.random.default_rng(seed)
        self.vocabs, self.extra = vocabs, list(extra)
        self.offs, self.ids, self.lengths = [], [], []
        off = 0
        for si, (K, vs) in enumerate(zip(KS, vocabs)):
            self.offs.append(off + np.concatenate([[0], np.cumsum(vs)[:-1]]).astype(np.int64))
            off += sum(vs)
            ls = rng.choice(np.asarray(lengths), B * K).astype(np.int64)
            if tail_empty:
                ls[-tail_empty:] = 0                                   # empty bags at the end of the side
            v = np.asarray(vs, dtype=np.int64)[np.repeat(np.arange(B * K), ls) % K]
            ids = (rng.random(v.size) * (v + 4)).astype(np.int64) - 2     # a few negative and too large ids: clamped
            if last_row and ids.size:
                k = np.repeat(np.arange(B * K), ls) % K
                ids[k == K - 1] = np.where(rng.random(int((k == K - 1).sum())) < 0.5, vs[-1] - 1, ids[k == K - 1])
            self.lengths.append(ls)
            self.ids.append(ids)
        self.table_rows = off
        self.table = torch.from_numpy(rng.standard_normal((off, E)).astype(np.float32)).to(DEV)
        self.nnz = [len(i) for i in self.ids]
        self.caps = [n + x for n, x in zip(self.nnz, self.extra)]
        self.d = [torch.from_numpy(rng.standard_normal((B, K * E)).astype(np.float32)).to(DEV) for K in KS]

    def sides(self, ops, capacity, out_dtype=torch.float32, counts="right"):
        """ops.BagSide per side (exact: the live ids; capacity: buffers of self.caps ids with garbage tails) and the output buffers"""
        bufs, sides = [], []
        for si, K in enumerate(KS):
            buf = torch.full((B, 8 + K * E + 4), float("nan"), dtype=out_dtype, device=DEV)
            ids = self.ids[si]
            kw = {}
            if capacity:
                tail = np.resize(np.asarray(GARBAGE, dtype=np.int64), max(self.caps[si] - self.nnz[si], 0))
                ids = np.concatenate([ids, tail])[:self.caps[si]]
                n = self.nnz[si] if counts == "right" else counts[si]
                kw = dict(capacity=self.caps[si], count=None if n is None else torch.tensor([n], dtype=torch.int32, device=DEV))
            pool = torch.tensor([ops.POOL_MODES[p] for p in POOLING[si]], dtype=torch.int32, device=DEV)
            sides.append(ops.BagSide(torch.from_numpy(ids).to(DEV), torch.from_numpy(self.lengths[si]).to(DEV),
                                     torch.from_numpy(self.offs[si]).to(DEV), torch.tensor(self.vocabs[si], dtype=torch.int64, device=DEV),
                                     pool, buf[:, 8:8 + K * E], K, True, **kw))
            bufs.append(buf)
        return sides, bufs

    def srcs(self, dtype=torch.float32):
        return [(d.to(dtype), K) for d, K in zip(self.d, KS)]


CASES = {
    "cap=nnz": dict(extra=(0, 0)),
    "cap=nnz+1": dict(extra=(1, 1)),
    "cap=nnz+5000": dict(extra=(5000, 5000)),                          # the pads cross a 4096-element sort tile and a head tile
    "all-bags-empty": dict(extra=(64, 9), lengths=(0,)),               # the plan is all pads: n_unique = 0
    "empty-bags-at-the-end": dict(extra=(300, 40), tail_empty=20),
    "two-capacities": dict(extra=(777, 3)),                            # side 0's pads sit in the middle of position space
    "long-rows": dict(extra=(130, 70), lengths=(3, 4, 5), vocabs=[[50, 1, 120], [2, 75]]),      # rows of > 64 and > 128 contributions
    "table-of-256-rows": dict(extra=(100, 50), vocabs=[[100, 40, 20], [60, 36]], last_row=True),   # the pad key is the 9th bit
    "table-of-2048-rows": dict(extra=(100, 50), vocabs=[[1000, 400, 100], [500, 48]], last_row=True),   # ... the 12th
    "table-of-255-rows": dict(extra=(100, 50), vocabs=[[100, 40, 20], [60, 35]], last_row=True),   # the pad key is value 255 of 8 bits
}


def _run(c, ops, capacity, out_dtype=torch.float32):
    sides, bufs = c.sides(ops, capacity, out_dtype)
    bag = ops.embed_bag_lookup(c.table, sides, B, want_rows=True)
    plan = ops.bag_dedup_plan(bag, c.table_rows) if bag.nnz else None     # (no ids at all: the towers build no plan either)
    return sides, bufs, bag, plan


def _grads(c, ops, bag, plan, dtype):
    """sparse rows, the dense-set gradient, the dense-accumulate gradient over a random prior"""
    srcs = c.srcs(dtype)
    g = torch.Generator(device=DEV).manual_seed(5)
    sparse = torch.full((max(plan.M if plan else 0, 1), E), float("nan"), device=DEV)
    dense_set = torch.zeros((c.table_rows, E), device=DEV)
    dense_acc = torch.randn((c.table_rows, E), device=DEV, generator=g)
    if plan is not None:
        ops.embed_bag_grad(plan, bag, srcs, B, E, ops.TT_GRAD_SPARSE, sparse)
        ops.embed_bag_grad(plan, bag, srcs, B, E, ops.TT_GRAD_DENSE_SET, dense_set)
        ops.embed_bag_grad(plan, bag, srcs, B, E, ops.TT_GRAD_DENSE_ACC, dense_acc)
    return sparse, dense_set, dense_acc


@pytest.mark.parametrize("name", list(CASES))
def test_capacity_form_equals_the_exact_entries_on_the_live_ids(tt, name):
    from jodalrob_twotower_amd import ops
    dev = torch.device(DEV)
    c = Case(sum(map(ord, name)), **CASES[name])
    assert c.table_rows == {"table-of-256-rows": 256, "table-of-2048-rows": 2048, "table-of-255-rows": 255}.get(name, c.table_rows)
    _L.check_device_errors(dev)                                       # start clean
    _, bufs0, bag0, plan0 = _run(c, ops, False)
    _, bufs1, bag1, plan1 = _run(c, ops, True)
    torch.cuda.synchronize()
    _L.check_device_errors(dev)                                       # nothing of the garbage tails was decoded
    assert bag0.pad_row is None and bag1.pad_row == c.table_rows and bag1.nnz == plan1.M == sum(c.caps) and bag0.nnz == sum(c.nnz)
    for a, b in zip(bufs0, bufs1):
        assert np.array_equal(_bits(a), _bits(b))                      # pooled outputs, NaN padding around the views included
    for dt in (torch.bfloat16,):
        _, a16, _, _ = _run(c, ops, False, dt)
        _, b16, _, _ = _run(c, ops, True, dt)
        for a, b in zip(a16, b16):
            assert np.array_equal(_bits(a), _bits(b))
    # rows_out / bag_of: the covered positions as the exact entry writes them, every pad position (table_rows, -1)
    rows1, of1 = bag1.rows.cpu().numpy(), bag1.bag_of.cpu().numpy()
    want_rows, where = P.with_pads(bag0.rows.cpu().numpy(), c.table_rows, list(zip(c.nnz, c.caps)))
    want_of, _ = P.with_pads(bag0.bag_of.cpu().numpy(), -1, list(zip(c.nnz, c.caps)))
    assert np.array_equal(rows1, want_rows) and np.array_equal(of1, want_of)
    if name.startswith("table-of"):
        assert (bag0.rows == c.table_rows - 1).any()                   # the last row is in use, next to the pad key
    assert bag0.inv_len is not None and bag1.inv_len is not None
    if sum(c.nnz):
        assert np.array_equal(_bits(bag0.inv_len), _bits(bag1.inv_len))
    # the plan: n_unique, unique_rows[:U], the real rows' runs as runs of live positions; the numpy model agrees
    U0, U1 = int(plan0.n_unique.item()) if plan0 else 0, int(plan1.n_unique.item())
    assert U0 == U1 and (U1 > 0) == (sum(c.nnz) > 0) and (plan0 is None) == (name == "all-bags-empty")
    if plan0:
        assert torch.equal(plan0.unique_rows[:U0], plan1.unique_rows[:U1]) and torch.equal(plan0.seg_offsets[:U0 + 1], plan1.seg_offsets[:U1 + 1])
    src_m, uniq_m, seg_m, n_m = P.padded_plan(rows1, c.table_rows)
    assert n_m == U1 and np.array_equal(plan1.sorted_src.cpu().numpy(), src_m)
    assert np.array_equal(plan1.unique_rows[:len(uniq_m)].cpu().numpy(), uniq_m)
    assert np.array_equal(plan1.seg_offsets[:len(seg_m)].cpu().numpy(), seg_m)
    back = np.full(sum(c.caps), -1, np.int64)
    back[where] = np.arange(sum(c.nnz))
    end = int(plan1.seg_offsets[U1].item()) if sum(c.caps) else 0
    if plan0:
        assert end == sum(c.nnz) and np.array_equal(back[plan1.sorted_src[:end].cpu().numpy()], plan0.sorted_src.cpu().numpy())
    if name == "long-rows":
        seg = plan1.seg_offsets[:U1 + 1].cpu().numpy()
        assert (np.diff(seg) > 128).any() and (np.diff(seg) > 64).sum() >= 2      # the chunk path and the finish run, pads present
    # the gradients
    for dt in (torch.float32, torch.bfloat16):
        g0, g1 = _grads(c, ops, bag0, plan0, dt), _grads(c, ops, bag1, plan1, dt)
        assert np.array_equal(_bits(g0[0][:U0]), _bits(g1[0][:U1])), dt          # the sparse rows [:U]
        assert np.array_equal(_bits(g0[1]), _bits(g1[1])) and np.array_equal(_bits(g0[2]), _bits(g1[2])), dt
        if U1:
            assert not torch.isnan(g1[0][:U1]).any() and bool(torch.isnan(g1[0][U1:]).all())      # nothing behind the real rows is written
    torch.cuda.synchronize()
    _L.check_device_errors(dev)


@pytest.mark.parametrize("slots_b", [37, 1500], ids=["111+74-slots", "4500+3000-slots"])
def test_prepare_equals_the_torch_formulas(tt, slots_b):
    """offsets and inv_len of tt_bag_prepare against torch.cumsum and the one f32 division ops.embed_bag_lookup forms, bit for bit:
    lengths 0, 1, powers of two and others up to 300, slot counts that are no multiple of a thread's 8 or a tile's 2048 (4500 slots:
    three tiles, so the tile totals and the scan across them are exercised)."""
    from jodalrob_twotower_amd import ops
    dev = torch.device(DEV)
    g = torch.Generator().manual_seed(slots_b)
    lengths, pools = [], []
    for K in KS:
        ln = torch.randint(0, 12, (slots_b * K,), generator=g)
        ln[torch.randint(0, ln.numel(), (9,), generator=g)] = torch.tensor([0, 1, 3, 7, 64, 100, 255, 256, 300])
        lengths.append(ln.to(DEV))
        pools.append(torch.tensor([1, 0, 1][:K], dtype=torch.int32, device=DEV))
    totals = [int(ln.sum()) for ln in lengths]
    counts = [torch.tensor([t], dtype=torch.int32, device=DEV) for t in totals]
    _L.check_device_errors(dev)
    offs, inv = ops.bag_prepare(lengths, pools, KS, slots_b, [totals[0], totals[1] + 11], counts)
    want_inv = []
    for ln, pool, K, off, tot in zip(lengths, pools, KS, offs, totals):
        want = torch.zeros(ln.numel() + 1, dtype=torch.int64, device=DEV)
        torch.cumsum(ln, 0, out=want[1:])
        assert off.dtype == torch.int64 and torch.equal(off, want) and int(off[-1]) == tot
        lf = ln.to(torch.float32)
        mean = (pool != 0).repeat(slots_b) & (ln > 0)
        one = torch.ones_like(lf)
        want_inv.append(torch.where(mean, one / lf.clamp(min=1.0), one))
    assert np.array_equal(_bits(inv), _bits(torch.cat(want_inv)))
    assert ops.bag_prepare(lengths, pools, KS, slots_b, totals, None, want_inv_len=False)[1] is None
    torch.cuda.synchronize()
    _L.check_device_errors(dev)


@pytest.mark.parametrize("how", ["count-differs", "total-above-capacity", "negative-length"])
def test_refused_totals_raise_the_device_error_word(tt, how):
    """The lengths and the handed-over count are device data: a count that differs from the lengths' total, a total above the
    capacity or a negative length raises TT_DEVERR_BAG_OFFSETS (the sticky word tests/test_gpu_embed_bag.py exercises -- no fault).
    The launches complete, the side's bags count as empty (zeros pooled, every position a pad: nothing is read through them), the
    other side is whole, and the next correct call is clean."""
    from jodalrob_twotower_amd import ops
    dev = torch.device(DEV)
    c = Case(77, (40, 40), lengths=(1, 2, 3))
    _, good, bag_good, _ = _run(c, ops, True)
    counts = [c.nnz[0], c.nnz[1]]
    if how == "count-differs":
        counts[0] += 1
    elif how == "total-above-capacity":
        c.caps[0] = c.nnz[0] - 1                                       # (the id buffer is cut to it)
        counts[0] = None
    else:
        c.lengths[0][5] = -1
        counts[0] = None
    _L.check_device_errors(dev)
    sides, bufs = c.sides(ops, True, counts=counts)
    bag = ops.embed_bag_lookup(c.table, sides, B, want_rows=True)
    plan = ops.bag_dedup_plan(bag, c.table_rows)
    sparse = torch.zeros((plan.M, E), device=DEV)
    ops.embed_bag_grad(plan, bag, c.srcs(), B, E, ops.TT_GRAD_SPARSE, sparse)
    torch.cuda.synchronize()
    with pytest.raises(_L.TwoTowerHipError, match=r"status -5\).*device error word 0x8:.*bag offsets"):
        _L.check_device_errors(dev)
    assert not bufs[0][:, 8:8 + KS[0] * E].any()                       # side 0: every bag empty
    assert bool((bag.rows[:c.caps[0]] == c.table_rows).all()) and bool((bag.bag_of[:c.caps[0]] == -1).all())
    assert np.array_equal(_bits(bufs[1]), _bits(good[1]))              # side 1 is whole
    assert torch.equal(bag.rows[c.caps[0]:], bag_good.rows[c.nnz[0] + 40:]) and int(plan.n_unique.item()) > 0
    c2 = Case(77, (40, 40), lengths=(1, 2, 3))                         # the next correct call is clean
    _, again, _, _ = _run(c2, ops, True)
    torch.cuda.synchronize()
    _L.check_device_errors(dev)
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(again, good))
