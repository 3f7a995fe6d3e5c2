"""The captured bag-mode step fed from WEIGHTED device-resident bag stores on the MI355X: DevicePairLoader.step_batches ->
GraphedTrainStep.step_from_store (tt_bag_store_gather_w fills the static id AND weight buffers) against the captured step(batch) on
store.gather batches and against the eager step on the same batches.

Schema of the bag tests (manifest case wide_b40: 5 + 2 keys, E = 16, towers [32, 24] -> 16) at B = 320 (two scan tiles), two pooled
keys per tower (one summed, one averaged), dropout 0.1, fp32 modes.  Everything is bit for bit: the gather copies ids and weights,
so a store-fed step sees the very static buffers a step(batch) fills, and a captured bag step runs its eager twin's kernels on the
same values in the same order (tests/test_gpu_embed_bag_capture.py).  Dropout: a captured step adds a per-step device word to the
seed baked at capture; the eager legs run on base + that word (as tests/test_gpu_pair_weights.py does)."""
import numpy as np
import pytest
import torch

import _bag_store_weight_reference as RW
from test_gpu_embed_bag_capture import _assert_same_state, _cfg, _eager, _task
from test_gpu_parity import DEV, tt, to_batch  # noqa: F401

from jodalrob_twotower_amd import _lib as _L

pytestmark = pytest.mark.gpu

B, N, STEPS = 320, 150, 3
M64, BASE = (1 << 64) - 1, 0x5DEECE66D
KW = dict(embedding_grad="sparse", mlp_dtype="fp32", score_dtype="fp32", dropout_rate=0.1)


def _pool(cfg, sides):
    """two pooled keys per tower of `sides`: one sum, one mean"""
    out = {}
    if "notice" in sides:
        out.update({cfg["keys_n"][3]: "sum", cfg["keys_n"][4]: "mean"})
    if "company" in sides:
        out.update({cfg["keys_c"][0]: "sum", cfg["keys_c"][1]: "mean"})
    return out


def _stores(tt, cfg, sides, weights="uniform", mean=3.0, seed=70):
    """{side: store} over N entities: a DeviceBagFeatureStore for the bag-mode `sides` (the pooled keys ragged bags, the others one id;
    weights: None | "uniform" | "ones"), a plain DeviceFeatureStore for the others"""
    from jodalrob_twotower_amd import synthetic
    from jodalrob_twotower_amd.data_loader import DeviceBagFeatureStore, DeviceFeatureStore
    from params_init import synth_batch_numpy
    b = to_batch(tt, synth_batch_numpy(N, cfg["vocab_n"], cfg["vocab_c"], cfg["din_n"], cfg["din_c"], seed, oob=False), cfg["keys_n"], cfg["keys_c"])
    out = {}
    for side in ("notice", "company"):
        keys, vocabs = cfg[f"keys_{side[0]}"], cfg[f"vocab_{side[0]}"]
        plain = DeviceFeatureStore({"dense_projected": b[side]["dense"], "categorical": b[side]["kjt"].values().view(N, -1)}, keys, DEV)
        if side not in sides:
            out[side] = plain
            continue
        st = synthetic.bag_store(plain, vocabs, _pool(cfg, [side]), mean, seed=seed + len(side), weights=None if weights is None else "uniform")
        if weights == "ones":
            st = DeviceBagFeatureStore({"dense_projected": st.dense, "categorical_offsets": st.offsets, "categorical_values": st.values,
                                        "categorical_weights": torch.ones_like(st.weights)}, keys, DEV)
        out[side] = st
    return out


def _loader(stores, pairs, seed=9):
    from jodalrob_twotower_amd.data_loader import DevicePairLoader
    return DevicePairLoader(stores["notice"], stores["company"], pairs, B, shuffle=True, seed=seed)


def _peek_counts(loader):
    """(order, id counts per batch) of the epoch the loader is about to run"""
    state = loader._gen.get_state()
    order = loader.epoch_order()
    loader._gen.set_state(state)
    return order, loader.epoch_bag_ids(order)


def _towers(task):
    return (task.two_tower_model.notice_tower, task.two_tower_model.company_tower)


def _seed(task, word=None):
    for tw in _towers(task):
        tw._seed_override = BASE if word is None else (BASE + word) & M64


def _captured(task, opt, example, caps):
    from jodalrob_twotower_amd.graph import GraphedTrainStep
    _seed(task)
    torch.manual_seed(99)                                  # the replays' device seed words draw from it
    return GraphedTrainStep(task, opt, example, warmup=1, bag_capacity=caps)


def _pairs(n_batches=STEPS, seed=3):
    return np.random.default_rng(seed).integers(0, N, (n_batches * B, 2))


@pytest.mark.parametrize("sides", [("notice", "company"), ("company",)], ids=["both-weighted", "company-weighted-notice-plain"])
def test_three_legs_agree_bit_for_bit(tt, manifest, sides):
    from jodalrob_twotower_amd.optim import FusedAdam
    cfg, dev = _cfg(manifest), torch.device(DEV)
    te, ta, tb = (_task(tt, cfg, _pool(cfg, sides), **KW) for _ in range(3))
    oe, oa, ob = (FusedAdam.for_task(t, lr=1e-2) for t in (te, ta, tb))
    stores = _stores(tt, cfg, sides)
    for side in ("notice", "company"):
        assert (getattr(stores[side], "weights", None) is not None) == (side in sides)
    pairs = _pairs()
    le_, la_, lb_ = (_loader(stores, pairs) for _ in range(3))
    order, counts = _peek_counts(lb_)
    assert sorted(counts) == sorted(sides) and all(len(c) == STEPS for c in counts.values())
    caps = {side: int(c.max()) + 17 for side, c in counts.items()}
    example = lb_.batch(order, 0, bag_ids=counts)
    for side in sides:
        k = example[side]["kjt"]
        assert k.weights().numel() == k.values().numel() == int(counts[side][0]) and float(k.weights().min()) < 1.0 < float(k.weights().max())
    _L.check_device_errors(dev)
    ga, gb = _captured(ta, oa, example, caps), _captured(tb, ob, example, caps)
    try:
        assert ga._bag_w == gb._bag_w == frozenset(sides)
        loss_a, loss_b, words_a, words_b = [], [], [], []
        torch.manual_seed(7)                               # (the replays draw their seed words from torch's generator: both legs the same)
        for b in la_:                                      # the captured step(batch) on store.gather batches
            loss_a.append(ga.step(b)["loss"].detach().clone())
            words_a.append(int(ga._seed_dev.item()) & M64)
        torch.manual_seed(7)
        for r in lb_.step_batches(gb, eager_step=None):    # the store-fed hand-over
            loss_b.append(r["loss"].detach().clone())
            words_b.append(int(gb._seed_dev.item()) & M64)
            for side in sides:                             # the count word the hand-over carried
                assert int(gb.static[side]["kjt"].bag_count) == int(counts[side][len(loss_b) - 1])
        assert lb_.eager_bag_batches == 0 and len(loss_a) == len(loss_b) == STEPS and words_a == words_b and len(set(words_a)) == STEPS
        loss_e = []
        for i, b in enumerate(le_):                        # the eager step on the same batches, on the captured steps' seeds
            _seed(te, words_a[i])
            loss_e.append(_eager(te, oe, b))
        for i in range(STEPS):
            assert torch.equal(loss_a[i], loss_b[i]) and torch.equal(loss_e[i], loss_b[i]), (i, float(loss_e[i]), float(loss_a[i]), float(loss_b[i]))
        for side in sides:                                 # after the last step both captured steps hold the same ids and weights
            n = int(counts[side][-1])
            sa, sb = ga.static[side]["kjt"], gb.static[side]["kjt"]
            assert torch.equal(sa.values()[:n], sb.values()[:n]) and torch.equal(RW.bits(sa.weights()[:n]), RW.bits(sb.weights()[:n]))
            assert torch.equal(sa.lengths(), sb.lengths())
        torch.cuda.synchronize()
        _L.check_device_errors(dev)
        _assert_same_state(ta, oa, tb, ob)
        _assert_same_state(te, oe, tb, ob)
    finally:
        ga.close()
        gb.close()


def test_unit_weights_are_the_weightless_store(tt, manifest):
    from jodalrob_twotower_amd.optim import FusedAdam
    cfg, dev, sides = _cfg(manifest), torch.device(DEV), ("notice", "company")
    ta, tb = (_task(tt, cfg, _pool(cfg, sides), **KW) for _ in range(2))
    oa, ob = (FusedAdam.for_task(t, lr=1e-2) for t in (ta, tb))
    plain, ones = _stores(tt, cfg, sides, weights=None), _stores(tt, cfg, sides, weights="ones")
    for side in sides:
        assert plain[side].weights is None and bool((ones[side].weights == 1).all()) and torch.equal(plain[side].values, ones[side].values)
    pairs = _pairs()
    la_, lb_ = _loader(plain, pairs), _loader(ones, pairs)
    order, counts = _peek_counts(la_)
    caps = {side: int(c.max()) + 17 for side, c in counts.items()}
    _L.check_device_errors(dev)
    ga = _captured(ta, oa, la_.batch(order, 0, bag_ids=counts), caps)
    gb = _captured(tb, ob, lb_.batch(order, 0, bag_ids=counts), caps)
    try:
        assert ga._bag_w == frozenset() and gb._bag_w == frozenset(sides)
        torch.manual_seed(7)                               # (the replays draw their seed words from torch's generator: both runs the same)
        la = [r["loss"].detach().clone() for r in la_.step_batches(ga, eager_step=None)]
        torch.manual_seed(7)
        lb = [r["loss"].detach().clone() for r in lb_.step_batches(gb, eager_step=None)]
        assert len(la) == len(lb) == STEPS and all(torch.equal(a, b) for a, b in zip(la, lb)), ([float(x) for x in la], [float(x) for x in lb])
        # each step refuses the other's stores: weights nobody captured would be dropped, weights somebody captured are missing
        with pytest.raises(ValueError, match="store carries per-id weights, but the step was captured without them"):
            ga.step_from_store(ones["notice"], ones["company"], la_.pairs, order, 0)
        with pytest.raises(ValueError, match="step_from_store: the step was captured with per-id weights"):
            gb.step_from_store(plain["notice"], plain["company"], lb_.pairs, order, 0)
        torch.cuda.synchronize()
        _L.check_device_errors(dev)
        _assert_same_state(ta, oa, tb, ob)
    finally:
        ga.close()
        gb.close()


def test_a_batch_over_the_capacity_takes_the_eager_step_with_its_weights(tt, manifest):
    from jodalrob_twotower_amd.optim import FusedAdam
    cfg, dev, sides = _cfg(manifest), torch.device(DEV), ("notice", "company")
    te, tg = (_task(tt, cfg, _pool(cfg, sides), **KW) for _ in range(2))
    oe, og = (FusedAdam.for_task(t, lr=1e-2) for t in (te, tg))
    stores = _stores(tt, cfg, sides)
    pairs = _pairs(4)
    le_, lg_ = _loader(stores, pairs), _loader(stores, pairs)
    order, counts = _peek_counts(lg_)
    full = counts["company"]
    assert len(full) == 4 and sorted(full)[-1] > sorted(full)[-2]
    caps = {"notice": int(counts["notice"].max()) + 10, "company": int(sorted(full)[-2])}        # the fullest batch does not fit
    k0 = int(np.argmin(full))
    _L.check_device_errors(dev)
    gs = _captured(tg, og, lg_.batch(order, B * k0, bag_ids=counts), caps)
    try:
        words, got, fell = [], [], []

        def eager_step(b):
            assert all(b[s]["kjt"].weights().numel() == b[s]["kjt"].values().numel() for s in sides)     # the batch gather() built carries them
            fell.append(len(got))
            _seed(tg)
            return {"loss": _eager(tg, og, b)}
        with pytest.warns(UserWarning, match=r"ids on the company side.*bag_capacity"):
            for r in lg_.step_batches(gs, eager_step=eager_step):
                words.append(None if fell and fell[-1] == len(got) else int(gs._seed_dev.item()) & M64)
                got.append(r["loss"].detach().clone())
        assert lg_.eager_bag_batches == 1 and fell == [int(np.argmax(full))] and len(got) == 4
        for i, b in enumerate(le_):                        # the all-eager run, on the same seeds
            _seed(te, words[i])
            assert torch.equal(_eager(te, oe, b), got[i]), i
        torch.cuda.synchronize()
        _L.check_device_errors(dev)
        _assert_same_state(te, oe, tg, og)
    finally:
        gs.close()


def test_a_catalogue_from_a_weighted_store(tt, manifest):
    """CatalogIndex.from_store reads the entities through store.gather, weights included: the index of a weighted company store is the
    index of the same entities' host-built weighted batch, and not the weightless store's."""
    from jodalrob_twotower_amd.retrieval import CatalogIndex
    cfg = _cfg(manifest)
    task = _task(tt, cfg, _pool(cfg, ["company"]), **KW)
    cs = _stores(tt, cfg, ["company"])["company"]
    bare = _stores(tt, cfg, ["company"], weights=None)["company"]
    index = CatalogIndex.from_store(task, cs, chunk=len(cs))
    assert task.training
    host = tt.build_bag_kjt(cs.keys, values=cs.values.cpu(), lengths=(cs.offsets[1:] - cs.offsets[:-1]).cpu(), weights=cs.weights.cpu(), device=DEV)
    task.eval()
    with torch.no_grad():
        emb = task.two_tower_model.get_company_embeddings({"dense": cs.dense, "kjt": host})
    task.train()
    want = CatalogIndex.from_embeddings(emb, task.temperature, task.score_dtype)
    assert index.size == want.size == N and torch.equal(index.data, want.data)
    q = torch.nn.functional.normalize(torch.randn(16, emb.shape[1], generator=torch.Generator().manual_seed(1)), dim=1).to(DEV)
    (va, ia), (vb, ib) = index.search(q, k=10), want.search(q, k=10)
    assert torch.equal(va, vb) and torch.equal(ia, ib) and ia.shape == (16, 10)
    assert not torch.equal(CatalogIndex.from_store(task, bare, chunk=len(bare)).data, index.data)
