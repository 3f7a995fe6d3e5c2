"""Learned position weights inside the captured bag-mode step on the MI355X: the pooled lookup's position-weight source
(tt_embed_bag_fwd_posw / tt_embed_bag_fwd_cap_posw) and GraphedTrainStep(learned_weights=True).

Shapes: B = 37, K = 3 keys per tower, E = 8 (C = 2 chunks, LG = 2) and E = 24 (C = 6, LG = 8: two dead lanes per group), bag lengths
0 .. 19 (empty bags, more than one 8-id trip, bags longer than max_len); per key max_len 4 (the clamp to a shared last weight), 32
(elements nobody reads) and none (pw_offset = -1); one mean key, two sum keys; the parameter drawn from U(0.5, 1.5).

What is bit for bit and why: the source reads the very f32 element tt_bag_position_weights_fwd copies into the per-id array (one
shared index function), and hands it to the multiply / fused-multiply-add chain of the weighted lookup; the captured backward runs
the eager launches (tt_embed_bag_weight_grad, tt_bag_position_weights_bwd) over the capacity, where uncovered positions hold a
gradient of 0 that the offsets never reach.  The f64 check uses the weighted lookup's own bound (tests/test_gpu_embed_bag_weights.py):
|got - ref| <= gamma_(L+1) * sum|w x| / divisor.
"""
import numpy as np
import pytest
import torch

import _bag_weight_reference as W
from test_gpu_embed_bag import U24
from test_gpu_embed_bag_capture import _assert_same_state, _eager, _task
from test_gpu_parity import DEV, tt  # noqa: F401  (tt: the module fixture)

from jodalrob_twotower_amd import _lib as _L

pytestmark = pytest.mark.gpu

B, K = 37, 3
VOCABS = [11, 23, 17]
POOLING = ["mean", "sum", "sum"]
PW_OFF, PW_LEN, N_PARAM = [0, 4, -1], [4, 32, 0], 36
GARBAGE = [1 << 40, -7, (1 << 62) + 5, -(1 << 50)]


@pytest.fixture(autouse=True)
def _device_errors_clean():
    yield
    torch.cuda.synchronize()
    _L.check_device_errors(torch.device(DEV))


def gamma(k):
    ku = np.asarray(k, dtype=np.float64) * U24
    return ku / (1 - ku)


class Case:
    """one side's bags, table and parameter (numpy), and their device copies"""

    def __init__(self, seed, E):
        r = np.random.default_rng(seed)
        self.E = E
        self.lengths = r.integers(0, 20, B * K).astype(np.int64)
        self.lengths[:6] = [0, 19, 1, 8, 9, 0]                      # every edge present whatever the draw
        self.key_off = np.concatenate([[0], np.cumsum(VOCABS)[:-1]]).astype(np.int64)
        key = np.repeat(np.arange(B * K) % K, self.lengths)
        self.ids = np.array([r.integers(-2, VOCABS[k] + 2) for k in key], dtype=np.int64)      # a few out of range: the clamp
        self.nnz = int(self.lengths.sum())
        self.table = r.standard_normal((sum(VOCABS), E)).astype(np.float32)
        self.param = r.uniform(0.5, 1.5, N_PARAM).astype(np.float32)
        j = np.concatenate([np.arange(n) for n in self.lengths]) if self.nnz else np.zeros(0, np.int64)
        off, ln = np.asarray(PW_OFF)[key], np.asarray(PW_LEN)[key]
        self.w_ref = np.where(off >= 0, self.param[np.clip(off + np.minimum(j, ln - 1), 0, N_PARAM - 1)], np.float32(1.0)).astype(np.float32)
        dev = DEV
        self.t_table = torch.from_numpy(self.table).to(dev)
        self.t_param = torch.from_numpy(self.param).to(dev)
        self.t_lengths = torch.from_numpy(self.lengths).to(dev)
        self.t_off = torch.tensor(PW_OFF, dtype=torch.int32, device=dev)
        self.t_len = torch.tensor(PW_LEN, dtype=torch.int32, device=dev)
        self.dir = (torch.from_numpy(self.key_off).to(dev), torch.tensor(VOCABS, dtype=torch.int64, device=dev),
                    torch.tensor([1 if p == "mean" else 0 for p in POOLING], dtype=torch.int32, device=dev))

    def side(self, ops, out_dtype, capacity=None, weights=None, source=False):
        ids, w = self.ids, weights
        if capacity is not None:                                    # a static buffer: garbage ids and NaN weights behind the live ones
            ids = np.concatenate([ids, np.resize(np.asarray(GARBAGE, dtype=np.int64), capacity - self.nnz)])
            if w is not None:
                w = torch.cat([w, torch.full((capacity - self.nnz,), float("nan"), device=DEV)])
        out = torch.zeros((B, K * self.E), dtype=out_dtype, device=DEV)
        pw = ops.BagPosWeights(self.t_param, self.t_off, self.t_len) if source else None
        return ops.BagSide(torch.from_numpy(ids).to(DEV), self.t_lengths, *self.dir, out, K, True, capacity, None, w, pw)

    def expanded(self, ops):
        """the per-id weights tt_bag_position_weights_fwd forms (the eager path's launch)"""
        (w,) = ops.bag_position_weights(self.t_param, [ops.PosWeightSide(self.t_lengths, self.t_off, self.t_len, self.nnz, K)], B)
        return w


def _same(a_sides, a, b_sides, b):
    """out of every side, rows, bag_of everywhere, pos_w at the positions a bag covers"""
    for sa, sb in zip(a_sides, b_sides):
        assert torch.equal(sa.out, sb.out)
    assert torch.equal(a.rows, b.rows) and torch.equal(a.bag_of, b.bag_of)
    cov = a.bag_of >= 0
    assert int(cov.sum()) > 0 and torch.equal(a.pos_w[cov], b.pos_w[cov])
    assert a.pad_row == b.pad_row and a.side_nnz == b.side_nnz
    return cov


@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("E", [8, 24])
@pytest.mark.parametrize("form", ["plain", "cap=nnz", "cap=2nnz+5"])
def test_source_lookup_equals_expansion_plus_weighted_lookup(tt, E, out_dtype, form):
    from jodalrob_twotower_amd import ops
    c = Case(4100 + E, E)
    assert c.lengths.min() == 0 and c.lengths.max() == 19 and c.nnz > 8 * B
    cap = None if form == "plain" else (c.nnz if form == "cap=nnz" else 2 * c.nnz + 5)
    w = c.expanded(ops)
    assert np.array_equal(w.cpu().numpy().view(np.uint32), c.w_ref.view(np.uint32))      # (the expansion is the numpy index)
    assert len(np.unique(c.w_ref)) > 10
    ref_sides = [c.side(ops, out_dtype, cap, weights=w)]
    ref = ops.embed_bag_lookup(c.t_table, ref_sides, B, want_rows=True)
    got_sides = [c.side(ops, out_dtype, cap, source=True)]
    n0 = _L.load().tt_launch_count()
    got = ops.embed_bag_lookup(c.t_table, got_sides, B, want_rows=True)
    assert _L.load().tt_launch_count() - n0 == (1 if cap is None else 3)                 # the lookup (+ tt_bag_prepare's two): no expansion
    torch.cuda.synchronize()
    cov = _same(got_sides, got, ref_sides, ref)
    assert int(cov.sum()) == c.nnz
    if cap is not None:
        assert bool((got.rows[~cov] == c.table.shape[0]).all()) and bool((got.bag_of[~cov] == -1).all())
        assert got.offsets is not None and int(got.offsets[0][-1]) == c.nnz
    # without rows: the pooled block alone, the same bits
    only = [c.side(ops, out_dtype, cap, source=True)]
    assert ops.embed_bag_lookup(c.t_table, only, B, want_rows=False) is None
    assert torch.equal(only[0].out, ref_sides[0].out)


@pytest.mark.parametrize("other", ["data-weights", "none"])
@pytest.mark.parametrize("form", ["plain", "cap"])
def test_two_sides_of_different_sources_share_one_launch(tt, other, form):
    from jodalrob_twotower_amd import ops
    E = 24
    a, b = Case(4200, E), Case(4201, E)
    b.t_table = a.t_table                                           # one store: both sides read one table (b's rows are a's)
    caps = (None, None) if form == "plain" else (2 * a.nnz + 5, b.nnz)
    wb = torch.from_numpy(np.random.default_rng(3).standard_normal(b.nnz).astype(np.float32)).to(DEV) if other == "data-weights" else None
    for order in ((0, 1), (1, 0)):                                  # the parameter side first, and second
        ref_sides = [a.side(ops, torch.float32, caps[0], weights=a.expanded(ops)), b.side(ops, torch.float32, caps[1], weights=wb)]
        got_sides = [a.side(ops, torch.float32, caps[0], source=True), b.side(ops, torch.float32, caps[1], weights=wb)]
        ref_sides, got_sides = [ref_sides[i] for i in order], [got_sides[i] for i in order]
        ref = ops.embed_bag_lookup(a.t_table, ref_sides, B, want_rows=True)
        n0 = _L.load().tt_launch_count()
        got = ops.embed_bag_lookup(a.t_table, got_sides, B, want_rows=True)
        assert _L.load().tt_launch_count() - n0 == (1 if form == "plain" else 3)
        torch.cuda.synchronize()
        cov = _same(got_sides, got, ref_sides, ref)
        assert int(cov.sum()) == a.nnz + b.nnz
        if other == "none":                                         # the side without a source weighs 1 in w_out
            lo = 0 if order[0] == 1 else got.side_nnz[0]
            assert bool((got.pos_w[lo:lo + b.nnz] == 1.0).all())


def test_source_lookup_within_the_weighted_lookups_bound_of_f64(tt):
    from jodalrob_twotower_amd import ops
    E = 24
    c = Case(4300, E)
    sides = [c.side(ops, torch.float32, source=True)]
    ops.embed_bag_lookup(c.t_table, sides, B, want_rows=False)
    torch.cuda.synchronize()
    ref, mag, _, _ = W.weighted_forward(c.table, c.ids, c.lengths, c.key_off, VOCABS, POOLING, c.w_ref)
    L = np.repeat(c.lengths.reshape(B, K), E, axis=1).astype(np.float64)
    bound = gamma(L + 1) * mag
    err = np.abs(sides[0].out.cpu().numpy().astype(np.float64) - ref)
    print(f"\n[embed_bag_pw fwd E={E}] worst err / bound = {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
    assert (err <= bound).all() and np.abs(ref).max() > 1


def test_bad_sources_are_refused_before_any_launch(tt):
    from jodalrob_twotower_amd import ops
    c = Case(4400, 8)
    n0 = _L.load().tt_launch_count()
    both = c.side(ops, torch.float32, weights=torch.ones(c.nnz, device=DEV), source=True)
    with pytest.raises(ValueError, match="one source of weights per side"):
        ops.embed_bag_lookup(c.t_table, [both], B, want_rows=True)
    for bad, what in ((ops.BagPosWeights(c.t_param.double(), c.t_off, c.t_len), "float32 vector"),
                      (ops.BagPosWeights(c.t_param.cpu(), c.t_off, c.t_len), "float32 vector"),
                      (ops.BagPosWeights(c.t_param[:0], c.t_off, c.t_len), "non-empty"),
                      (ops.BagPosWeights(c.t_param, c.t_off[:2], c.t_len), "pw_offset"),
                      (ops.BagPosWeights(c.t_param, c.t_off, c.t_len.long()), "pw_len")):
        s = c.side(ops, torch.float32)
        s.pos_weights = bad
        with pytest.raises(ValueError, match=what):
            ops.embed_bag_lookup(c.t_table, [s], B, want_rows=True)
    assert _L.load().tt_launch_count() == n0


# ------------------------------------------------------------------------------------------- the captured step
F32 = dict(embedding_grad="sparse", mlp_dtype="fp32", score_dtype="fp32")
BF16 = dict(embedding_grad="sparse", mlp_dtype="bf16", score_dtype="bf16")
SIDES = (("notice", "notice_tower", "n"), ("company", "company_tower", "c"))


def _cfg(manifest, E):
    """three pooled keys per tower (the company tower's third key is not in the metadata: the default vocabulary of 1000 ids)"""
    return dict(manifest["cases"]["wide_b40"], B=B, E=E, keys_n=["nc", "nd", "ne"], vocab_n=[27, 50, 1000], keys_c=["ca", "cb", "cz"],
                vocab_c=[13, 60, 1000])


POOL = {"nc": "mean", "nd": "sum", "ne": "sum", "ca": "sum", "cb": "mean", "cz": "sum"}
PW = {"nc": 4, "nd": 32, "cb": 4, "ca": 32}                      # ne, cz: none


def _pw_task(tt, cfg, modes, pw=PW):
    task = _task(tt, cfg, POOL, **({} if pw is None else dict(categorical_position_weights=pw)), **modes)
    if pw is not None:
        g = torch.Generator().manual_seed(11)
        with torch.no_grad():
            for _, tower, _ in SIDES:
                p = getattr(task.two_tower_model, tower).categorical_embedder.position_weight
                p.copy_((torch.rand(p.shape, generator=g) + 0.5).to(p.device))
    return task


def _batch(tt, cfg, seed, top=20):
    r = np.random.default_rng(seed)
    out = {}
    for side, _, s in SIDES:
        keys, vocabs = cfg[f"keys_{s}"], cfg[f"vocab_{s}"]
        lengths = r.integers(0, top, B * K).astype(np.int64)
        lengths[:4] = [0, top - 1, 1, min(9, top - 1)]
        key = np.repeat(np.arange(B * K) % K, lengths)
        ids = np.array([r.integers(0, vocabs[k]) for k in key], dtype=np.int64)
        out[side] = {"dense": torch.from_numpy(r.standard_normal((B, cfg[f"din_{s}"])).astype(np.float32)).to(DEV),
                     "kjt": tt.build_bag_kjt(keys, values=torch.from_numpy(ids), lengths=torch.from_numpy(lengths), device=DEV)}
    return out


def _nnz(b):
    return {side: b[side]["kjt"].values().numel() for side, _, _ in SIDES}


def _params(task):
    return [getattr(task.two_tower_model, tower).categorical_embedder.position_weight for _, tower, _ in SIDES]


@pytest.mark.parametrize("E", [8, 24])
@pytest.mark.parametrize("mlp", ["f32", "bf16"])
def test_captured_step_equals_the_eager_step(tt, manifest, monkeypatch, E, mlp):
    from jodalrob_twotower_amd import config as _config
    from jodalrob_twotower_amd.graph import GraphedTrainStep
    from jodalrob_twotower_amd.optim import FusedAdam
    if mlp == "bf16":                                               # the pooled block and d_x in bf16: the sources of both gradients
        monkeypatch.setattr(_config.settings, "tower_io_dtype", "both")
    cfg, modes = _cfg(manifest, E), (F32 if mlp == "f32" else BF16)
    te, tg = _pw_task(tt, cfg, modes), _pw_task(tt, cfg, modes)
    oe, og = (FusedAdam.for_task(t, lr=1e-2) for t in (te, tg))
    start = [p.detach().clone() for p in _params(tg)]
    assert all(bool((p != 1).all()) for p in start)
    batches = [_batch(tt, cfg, 800 + i, top) for i, top in enumerate((20, 7, 20, 12))]
    counts = [_nnz(b) for b in batches]
    assert all(len({c[side] for c in counts}) == 4 for side, _, _ in SIDES), counts      # four different id counts
    caps = {side: max(c[side] for c in counts) + 17 for side, _, _ in SIDES}
    gs = GraphedTrainStep(tg, og, batches[0], warmup=2, bag_capacity=caps, learned_weights=True)
    try:
        for p, s in zip(_params(tg), start):                        # the warm-up's steps were put back, the parameter included
            assert torch.equal(p.detach(), s)
            st = og.state.get(p)
            assert not st or not (bool(st["exp_avg"].any()) or bool(st["exp_avg_sq"].any()))      # ... with its moments
        for i, b in enumerate(batches):
            le = _eager(te, oe, b)
            lg = gs.step(b)["loss"].detach().clone()
            assert torch.equal(le, lg), (i, float(le), float(lg))
            torch.cuda.synchronize()
            _assert_same_state(te, oe, tg, og)                      # every parameter (both position_weights) and every moment
        for p, s in zip(_params(tg), start):
            read = (p.detach() - s).abs() > 0                       # elements some bag position reads moved; the others did not
            assert int(read.sum()) == 4 + 19                        # max_len 4: all four; max_len 32: positions 0 .. 18 of bags of <= 19 ids
            assert len(torch.unique(p.detach()[read])) > 8 and bool((p.detach()[read] != 1).all())
            assert any(p is q for grp in og.param_groups for q in grp["params"])
    finally:
        gs.close()


def _stores(tt, cfg, seed=90, N=96):
    from jodalrob_twotower_amd.data_loader import DeviceBagFeatureStore
    r = np.random.default_rng(seed)
    out = {}
    for side, _, s in SIDES:
        keys, vocabs = cfg[f"keys_{s}"], cfg[f"vocab_{s}"]
        lengths = r.integers(0, 20, N * K).astype(np.int64)
        lengths[:3] = [0, 19, 9]
        key = np.repeat(np.arange(N * K) % K, lengths)
        ids = np.array([r.integers(0, vocabs[k]) for k in key], dtype=np.int64)
        out[side] = DeviceBagFeatureStore({"dense_projected": torch.from_numpy(r.standard_normal((N, cfg[f"din_{s}"])).astype(np.float32)),
                                           "categorical_offsets": torch.from_numpy(np.concatenate([[0], np.cumsum(lengths)])),
                                           "categorical_values": torch.from_numpy(ids)}, keys, DEV)
    return out


def test_store_fed_step_equals_the_step_on_the_gathered_batch(tt, manifest):
    from jodalrob_twotower_amd.graph import GraphedTrainStep
    from jodalrob_twotower_amd.optim import FusedAdam
    cfg = _cfg(manifest, 24)
    ta, tb = _pw_task(tt, cfg, F32), _pw_task(tt, cfg, F32)
    oa, ob = (FusedAdam.for_task(t, lr=1e-2) for t in (ta, tb))
    stores = _stores(tt, cfg)
    g = torch.Generator().manual_seed(6)
    steps = 3
    pairs = torch.randint(0, 96, (steps * B, 2), generator=g).to(DEV)
    gathered = [{"notice": stores["notice"].gather(pairs[i * B:(i + 1) * B, 0]), "company": stores["company"].gather(pairs[i * B:(i + 1) * B, 1])}
                for i in range(steps)]
    counts = [_nnz(b) for b in gathered]
    caps = {side: max(c[side] for c in counts) + 9 for side, _, _ in SIDES}
    ga = GraphedTrainStep(ta, oa, gathered[0], warmup=1, bag_capacity=caps, learned_weights=True)
    gb = GraphedTrainStep(tb, ob, gathered[0], warmup=1, bag_capacity=caps, learned_weights=True)
    try:
        for i in range(steps):
            la = ga.step(gathered[i])["loss"].detach().clone()
            lb = gb.step_from_store(stores["notice"], stores["company"], pairs, None, i * B,
                                    bag_ids=None if i == steps - 1 else counts[i])["loss"].detach().clone()
            assert torch.equal(la, lb), (i, float(la), float(lb))
        torch.cuda.synchronize()
        _assert_same_state(ta, oa, tb, ob)
    finally:
        ga.close()
        gb.close()


def test_an_epoch_through_the_loader_with_one_batch_over_the_capacity(tt, manifest):
    """DevicePairLoader(bag stores).step_batches(captured with learned_weights, eager) == the eager loop over the loader's batches:
    batch B on 3 B + 5 pairs (a ragged last batch: the eager step), the fullest full batch forced over the capacity (the eager step
    with its position weights expanded, counted); bit for bit, both position_weights and their moments included."""
    from jodalrob_twotower_amd.data_loader import DevicePairLoader
    from jodalrob_twotower_amd.graph import GraphedTrainStep
    from jodalrob_twotower_amd.optim import FusedAdam
    cfg = _cfg(manifest, 8)
    te, tg = _pw_task(tt, cfg, F32), _pw_task(tt, cfg, F32)
    oe, og = (FusedAdam.for_task(t, lr=1e-2) for t in (te, tg))
    stores = _stores(tt, cfg)
    pairs = np.random.default_rng(4).integers(0, 96, (3 * B + 5, 2))
    le_, lg_ = (DevicePairLoader(stores["notice"], stores["company"], pairs, B, shuffle=True, seed=9) for _ in range(2))
    state = lg_._gen.get_state()
    order = lg_.epoch_order()                                       # a look at the epoch the loader is about to run
    lg_._gen.set_state(state)
    counts = lg_.epoch_bag_ids(order)
    full = counts["company"][:3]
    assert len(counts["company"]) == 4 and len(set(full.tolist())) == 3
    caps = {"notice": int(counts["notice"].max()) + 10, "company": int(sorted(full)[-2])}       # the fullest full batch does not fit
    k0 = int(np.argmin(full))
    gs = GraphedTrainStep(tg, og, lg_.batch(order, B * k0, bag_ids=counts), warmup=1, bag_capacity=caps, learned_weights=True)
    try:
        want = [_eager(te, oe, b) for b in le_]
        with pytest.warns(UserWarning, match=r"ids on the company side.*bag_capacity"):
            got = [r["loss"].detach().clone() for r in lg_.step_batches(gs, eager_step=lambda b: {"loss": _eager(tg, og, b)})]
        assert lg_.eager_bag_batches == 1 and len(got) == len(want) == 4
        for i, (a, b) in enumerate(zip(want, got)):
            assert torch.equal(a, b), (i, float(a), float(b))
        torch.cuda.synchronize()
        _assert_same_state(te, oe, tg, og)
    finally:
        gs.close()


def test_at_initialisation_the_first_captured_loss_is_the_unweighted_one(tt, manifest):
    from jodalrob_twotower_amd.graph import GraphedTrainStep
    from jodalrob_twotower_amd.optim import FusedAdam
    cfg = _cfg(manifest, 8)
    tp, tu = _pw_task(tt, cfg, F32), _pw_task(tt, cfg, F32, pw=None)
    with torch.no_grad():
        for p in _params(tp):
            p.fill_(1.0)
    b = _batch(tt, cfg, 820)
    caps = {side: n + 5 for side, n in _nnz(b).items()}
    gp = GraphedTrainStep(tp, FusedAdam.for_task(tp, lr=1e-2), b, warmup=1, bag_capacity=caps, learned_weights=True)
    gu = GraphedTrainStep(tu, FusedAdam.for_task(tu, lr=1e-2), b, warmup=1, bag_capacity=caps)
    try:
        assert torch.equal(gp.step(b)["loss"], gu.step(b)["loss"])
    finally:
        gp.close()
        gu.close()


def test_refusals_change_nothing(tt, manifest):
    from jodalrob_twotower_amd.data_loader import DeviceBagFeatureStore
    from jodalrob_twotower_amd.graph import GraphedTrainStep
    from jodalrob_twotower_amd.optim import FusedAdam
    from jodalrob_twotower_amd.segmented import SegmentedTrainStep
    from jodalrob_twotower_amd.unrolled import UnrolledTrainStep
    cfg = _cfg(manifest, 8)
    task, plain = _pw_task(tt, cfg, F32), _pw_task(tt, cfg, F32, pw=None)
    opt, popt = FusedAdam.for_task(task, lr=1e-2), FusedAdam.for_task(plain, lr=1e-2)
    b = _batch(tt, cfg, 830)
    caps = {side: n + 5 for side, n in _nnz(b).items()}

    def weighted(batch, grad=False):
        out = dict(batch)
        k = batch["company"]["kjt"]
        w = torch.ones(k.values().numel(), device=DEV, requires_grad=grad)
        out["company"] = dict(batch["company"], kjt=tt.KeyedJaggedTensor(k.keys(), k.values(), k.lengths(), w))
        return out

    towers = (task.two_tower_model.notice_tower, task.two_tower_model.company_tower)
    state = {k: v.detach().clone() for k, v in task.state_dict().items()}
    launches = _L.load().tt_launch_count()
    kw = dict(warmup=1, bag_capacity=caps, learned_weights=True)
    with pytest.raises(ValueError, match="no embedder of the model learns position weights"):
        GraphedTrainStep(plain, popt, b, **kw)
    with pytest.raises(ValueError, match="learned_weights=True.* needs bag_capacity"):
        GraphedTrainStep(task, opt, b, warmup=1, learned_weights=True)
    with pytest.raises(ValueError, match="one source of weights per embedder"):
        GraphedTrainStep(task, opt, weighted(b), **kw)
    with pytest.raises(ValueError, match="does not support per-id weights that require grad"):
        GraphedTrainStep(plain, popt, weighted(b, grad=True), warmup=1, bag_capacity=caps)
    with pytest.raises(ValueError, match="UnrolledTrainStep.learned_weights=True.*refuse them"):
        UnrolledTrainStep(task, opt, b, unroll=2, **kw)
    with pytest.raises(ValueError, match="SegmentedTrainStep.learned_weights=True.*refuse them"):
        SegmentedTrainStep(task, opt, b, **kw)
    task.exchange = object()                                        # what marks a row-wise sharded task (distributed.py)
    try:
        with pytest.raises(ValueError, match=r"GraphedTrainStep\(learned_weights=True\).*unsharded task alone.*sharded steps refuse them"):
            GraphedTrainStep(task, opt, b, **kw)
    finally:
        del task.exchange
    with pytest.raises(ValueError, match="GraphedTrainStep does not support learned position weights.*eager step"):
        GraphedTrainStep(task, opt, b, warmup=1, bag_capacity=caps)                       # the default stands
    assert _L.load().tt_launch_count() == launches
    assert all(torch.equal(v, state[k]) for k, v in task.state_dict().items())
    assert all(t._seed_dev is None for t in towers)
    # a captured step: a batch, and a store, with per-id weights on a position-weighted side
    gs = GraphedTrainStep(task, opt, b, **kw)
    try:
        gs.step(b)
        torch.cuda.synchronize()
        state = {k: v.detach().clone() for k, v in task.state_dict().items()}
        launches = _L.load().tt_launch_count()
        seeds = [(t._seed_dev, None if t._seed_dev is None else t._seed_dev.clone()) for t in towers]

        def unchanged():
            assert _L.load().tt_launch_count() == launches
            assert all(torch.equal(v, state[k]) for k, v in task.state_dict().items())
            for t, (ref, val) in zip(towers, seeds):
                assert t._seed_dev is ref and (val is None or torch.equal(t._seed_dev, val))
            assert torch.equal(gs._seed_dev, seed_word)
        seed_word = gs._seed_dev.clone()
        with pytest.raises(ValueError, match="one source of weights per embedder"):
            gs.step(weighted(b))
        unchanged()
        stores = _stores(tt, cfg)
        cs = stores["company"]
        wstore = DeviceBagFeatureStore({"dense_projected": cs.dense, "categorical_offsets": cs.offsets, "categorical_values": cs.values,
                                        "categorical_weights": torch.ones(cs.values.numel())}, cfg["keys_c"], DEV)
        pairs = torch.zeros((B, 2), dtype=torch.int64, device=DEV)
        with pytest.raises(ValueError, match="one source of weights per embedder"):
            gs.step_from_store(stores["notice"], wstore, pairs, None, 0, bag_ids={"notice": 0, "company": 0})
        unchanged()
    finally:
        gs.close()
