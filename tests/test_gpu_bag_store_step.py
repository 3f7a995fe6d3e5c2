"""The store-fed hand-over of the captured bag-mode step on the MI355X: GraphedTrainStep.step_from_store fed from
DeviceBagFeatureStore objects (tt_bag_store_gather) against the same step fed hand-built batches, and both against an eager twin.
Schema and helpers of tests/test_gpu_embed_bag_capture.py (manifest case wide_b40, B = 64, dropout 0).

Everything here is bit for bit: the gather moves integers and copies f32, so a store-fed step sees the very static buffers a
step(batch) on store.gather(...) fills, and a captured bag step equals its eager twin (test_gpu_embed_bag_capture.py)."""
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from test_gpu_parity import DEV, tt, to_batch  # noqa: F401
from test_gpu_embed_bag_capture import B, MEANS, VARIANTS, _assert_same_state, _bag_sides, _cfg, _eager, _task

from jodalrob_twotower_amd import _lib as _L

pytestmark = pytest.mark.gpu

GROUP = 48                                                  # entities per group; group g's bags have mean length MEANS[g]


def _stores(tt, cfg, sides, seed=70):
    """{side: store} over len(MEANS) * GROUP entities: a DeviceBagFeatureStore for the bag-mode `sides` -- every key a ragged bag, the
    entities of group g drawn with mean length MEANS[g] -- and a plain DeviceFeatureStore for the others"""
    from jodalrob_twotower_amd import synthetic
    from jodalrob_twotower_amd.data_loader import DeviceBagFeatureStore, DeviceFeatureStore
    from params_init import synth_batch_numpy
    N = len(MEANS) * GROUP
    b = to_batch(tt, synth_batch_numpy(N, cfg["vocab_n"], cfg["vocab_c"], cfg["din_n"], cfg["din_c"], seed, oob=False), cfg["keys_n"], cfg["keys_c"])
    out = {}
    for side in ("notice", "company"):
        keys, vocabs = cfg[f"keys_{side[0]}"], cfg[f"vocab_{side[0]}"]
        plain = DeviceFeatureStore({"dense_projected": b[side]["dense"], "categorical": b[side]["kjt"].values().view(N, -1)}, keys, DEV)
        if side not in sides:
            out[side] = plain
            continue
        parts = []
        for g, mean in enumerate(MEANS):
            grp = DeviceFeatureStore({"dense_projected": plain.dense[g * GROUP:(g + 1) * GROUP],
                                      "categorical": plain.categorical[g * GROUP:(g + 1) * GROUP]}, keys, DEV)
            parts.append(synthetic.bag_store(grp, vocabs, keys, mean, seed=seed + 10 * g + len(side)))
        lengths = torch.cat([p.offsets[1:] - p.offsets[:-1] for p in parts])
        out[side] = DeviceBagFeatureStore({"dense_projected": plain.dense, "categorical_offsets": torch.cat([lengths.new_zeros(1), torch.cumsum(lengths, 0)]),
                                           "categorical_values": torch.cat([p.values for p in parts])}, keys, DEV)
    return out


def _pair_table(seed=5):
    """(pairs int64 [P, 2] on the device, order, [(notice entities, company entities)] per batch): batch i is pairs[order[64 i : 64 i + 64]],
    its entities drawn (with repeats) from group i"""
    g = torch.Generator().manual_seed(seed)
    P = len(MEANS) * B
    rows = torch.cat([i * GROUP + torch.randint(0, GROUP, (B, 2), generator=g) for i in range(len(MEANS))])
    order = torch.randperm(P, generator=g)
    pairs = torch.empty((P, 2), dtype=torch.int64)
    pairs[order] = rows
    return pairs.to(DEV), order.to(DEV), [(rows[i * B:(i + 1) * B, 0].to(DEV), rows[i * B:(i + 1) * B, 1].to(DEV)) for i in range(len(MEANS))]


def _counts(stores, sides, ents):
    return [{side: int(stores[side].run_lengths[e[0 if side == "notice" else 1]].sum()) for side in sides} for e in ents]


def _terms(i):
    g = torch.Generator().manual_seed(40 + i)
    return {s: {"log_q": (torch.rand(B, generator=g) * -3.0).to(DEV), "entity": torch.randint(0, B // 2, (B,), generator=g).to(torch.int32).to(DEV)}
            for s in ("notice", "company")}


def _batch(stores, e, terms=None):
    b = {"notice": stores["notice"].gather(e[0]), "company": stores["company"].gather(e[1])}
    if terms is not None:
        for s in b:
            b[s].update(terms[s])
    return b


@pytest.mark.parametrize("name", ["f32-sparse", "bf16-sparse", "company-only", "logq-entity"])
def test_store_fed_step_equals_the_hand_built_step_and_the_eager_twin(tt, manifest, name):
    from jodalrob_twotower_amd.graph import GraphedTrainStep
    from jodalrob_twotower_amd.optim import FusedAdam
    v, cfg, dev = VARIANTS[name], _cfg(manifest), torch.device(DEV)
    ta, tb, te = (_task(tt, cfg, v["pool"], **v["kw"]) for _ in range(3))
    sides = _bag_sides(ta)
    assert sides == (["company"] if name == "company-only" else ["notice", "company"])
    oa, ob, oe = (FusedAdam.for_task(t, lr=1e-2, **v.get("opt", {})) for t in (ta, tb, te))
    stores = _stores(tt, cfg, sides)
    pairs, order, ents = _pair_table()
    counts = _counts(stores, sides, ents)
    for side in sides:
        n = [c[side] for c in counts]
        assert n[0] < n[1] > n[2] > n[3] < n[4], n                     # rises, falls, rises again
    caps = {side: max(c[side] for c in counts) + 17 for side in sides}
    terms = [_terms(i) if v.get("terms") else None for i in range(len(ents))]
    _L.check_device_errors(dev)
    ga = GraphedTrainStep(ta, oa, _batch(stores, ents[0], terms[0]), warmup=2, bag_capacity=caps)
    gb = GraphedTrainStep(tb, ob, _batch(stores, ents[0], terms[0]), warmup=2, bag_capacity=caps)
    try:
        for i, e in enumerate(ents):
            batch = _batch(stores, e, terms[i])
            for side in sides:
                assert batch[side]["kjt"].values().numel() == counts[i][side]
            le = _eager(te, oe, batch)
            la = ga.step(batch)["loss"].detach().clone()
            kw = {} if terms[i] is None else {k: (terms[i]["notice"][k], terms[i]["company"][k]) for k in ("log_q", "entity")}
            # the last batch without bag_ids: the counts are summed from run_lengths and read back
            lb = gb.step_from_store(stores["notice"], stores["company"], pairs, order, i * B,
                                    bag_ids=None if i == len(ents) - 1 else counts[i], **kw)["loss"].detach().clone()
            assert torch.equal(la, lb) and torch.equal(le, lb), (i, float(le), float(la), float(lb))
            for side in ("notice", "company"):                         # the static buffers the two hand-overs filled
                sa, sb = ga.static[side], gb.static[side]
                n = counts[i].get(side, sa["kjt"].values().numel())
                assert torch.equal(sa["dense"], sb["dense"]) and torch.equal(sa["kjt"].values()[:n], sb["kjt"].values()[:n])
                assert torch.equal(sa["kjt"].lengths(), sb["kjt"].lengths())
                if side in sides:
                    assert int(sb["kjt"].bag_count) == n
        torch.cuda.synchronize()
        _L.check_device_errors(dev)
        _assert_same_state(ta, oa, tb, ob)
        _assert_same_state(te, oe, tb, ob)
    finally:
        ga.close()
        gb.close()


def test_over_the_capacity_is_refused_before_anything_is_launched(tt, manifest):
    from jodalrob_twotower_amd.data_loader import DeviceBagFeatureStore
    from jodalrob_twotower_amd.graph import GraphedTrainStep
    from jodalrob_twotower_amd.optim import FusedAdam
    cfg, dev = _cfg(manifest), torch.device(DEV)
    kw = dict(embedding_grad="sparse", mlp_dtype="fp32", score_dtype="fp32")
    te, tg = _task(tt, cfg, {"company": "mean"}, **kw), _task(tt, cfg, {"company": "mean"}, **kw)
    oe, og = (FusedAdam.for_task(t, lr=1e-2) for t in (te, tg))
    stores = _stores(tt, cfg, ["company"])
    pairs, order, ents = _pair_table()
    counts = _counts(stores, ["company"], ents)
    small, big, nxt = 2, 1, 3                                          # mean lengths 1.5, 5 and 0.3
    cap = counts[small]["company"] + 5
    assert counts[big]["company"] > cap >= counts[nxt]["company"]
    gs = GraphedTrainStep(tg, og, _batch(stores, ents[small]), warmup=1, bag_capacity=cap)
    ns, cs = stores["notice"], stores["company"]
    try:
        assert torch.equal(_eager(te, oe, _batch(stores, ents[small])), gs.step_from_store(ns, cs, pairs, order, small * B, bag_ids=counts[small])["loss"])
        held = lambda: [t.clone() for s in ("notice", "company") for t in (gs.static[s]["dense"], gs.static[s]["kjt"].values(), gs.static[s]["kjt"].lengths())] \
            + [gs.static["company"]["kjt"].bag_count.clone()]
        before = held()
        for ids in (counts[big], None):                                # the count given, and the count read back
            with pytest.raises(ValueError, match=rf"company: {counts[big]['company']} ids, the step was captured with bag_capacity = {cap}"):
                gs.step_from_store(ns, cs, pairs, order, big * B, bag_ids=ids)
        with pytest.raises(ValueError, match="step_from_store does not support bag mode"):       # a plain store on the bag-mode side
            gs.step_from_store(ns, ns, pairs, order, 0)
        with pytest.raises(ValueError, match="notice side is fed from a DeviceBagFeatureStore, but that side's embedder does not pool"):
            gs.step_from_store(DeviceBagFeatureStore.from_single(ns), cs, pairs, order, 0, bag_ids=counts[small])
        with pytest.raises(ValueError, match="bag_ids names"):
            gs.step_from_store(ns, cs, pairs, order, 0, bag_ids={"notice": 3, "company": 3})
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(before, held()))
        assert torch.equal(_eager(te, oe, _batch(stores, ents[nxt])), gs.step_from_store(ns, cs, pairs, order, nxt * B, bag_ids=counts[nxt])["loss"])
        torch.cuda.synchronize()
        _L.check_device_errors(dev)
        _assert_same_state(te, oe, tg, og)
    finally:
        gs.close()


def test_an_epoch_through_the_loader(tt, manifest):
    """DevicePairLoader(bag stores).step_batches(captured, eager) == for b in loader: eager(b): batch 16 on 70 pairs (a ragged last
    batch, through the eager step), one full batch forced over the capacity (eager too, counted)."""
    from jodalrob_twotower_amd.data_loader import DevicePairLoader
    from jodalrob_twotower_amd.graph import GraphedTrainStep
    from jodalrob_twotower_amd.optim import FusedAdam
    cfg, dev = _cfg(manifest), torch.device(DEV)
    pool, kw = {"notice": "sum", "company": "mean"}, dict(embedding_grad="sparse", mlp_dtype="fp32", score_dtype="fp32")
    te, tg = _task(tt, cfg, pool, **kw), _task(tt, cfg, pool, **kw)
    oe, og = (FusedAdam.for_task(t, lr=1e-2) for t in (te, tg))
    stores = _stores(tt, cfg, ["notice", "company"])
    N, Bl = len(stores["notice"]), 16
    pairs = np.random.default_rng(3).integers(0, N, (70, 2))
    le_, lg_ = (DevicePairLoader(stores["notice"], stores["company"], pairs, Bl, shuffle=True, seed=9) for _ in range(2))
    state = lg_._gen.get_state()
    order = lg_.epoch_order()                                          # a look at the epoch the loader is about to run
    lg_._gen.set_state(state)
    counts = lg_.epoch_bag_ids(order)
    full = counts["company"][:4]
    assert len(counts["company"]) == 5 and len(set(full.tolist())) == 4
    caps = {"notice": int(counts["notice"].max()) + 10, "company": int(sorted(full)[-2])}       # the fullest full batch does not fit
    k0 = int(np.argmin(full))
    gs = GraphedTrainStep(tg, og, lg_.batch(order, Bl * k0, bag_ids=counts), warmup=1, bag_capacity=caps)
    try:
        want = [_eager(te, oe, b) for b in le_]
        with pytest.warns(UserWarning, match=r"ids on the company side.*bag_capacity"):
            got = [r["loss"].detach().clone() for r in lg_.step_batches(gs, eager_step=lambda b: {"loss": _eager(tg, og, b)})]
        assert lg_.eager_bag_batches == 1 and len(got) == len(want) == 5
        for i, (a, b) in enumerate(zip(want, got)):
            assert torch.equal(a, b), (i, float(a), float(b))
        torch.cuda.synchronize()
        _L.check_device_errors(dev)
        _assert_same_state(te, oe, tg, og)
    finally:
        gs.close()


def test_a_catalogue_from_a_bag_store(tt, manifest):
    """Downstream use through gather's duck type: CatalogIndex.from_store over a bag company store indexes the rows
    get_company_embeddings(store.gather(every entity)) gives."""
    from jodalrob_twotower_amd.retrieval import CatalogIndex
    cfg = _cfg(manifest)
    task = _task(tt, cfg, {"company": "mean"}, embedding_grad="sparse", mlp_dtype="fp32", score_dtype="fp32")
    cs = _stores(tt, cfg, ["company"])["company"]
    index = CatalogIndex.from_store(task, cs, chunk=len(cs))
    assert task.training                                               # (the mode is put back)
    task.eval()
    with torch.no_grad():
        want = task.two_tower_model.get_company_embeddings(cs.gather(torch.arange(len(cs), device=DEV)))
    task.train()
    assert index.size == len(cs) and index.score_dtype == "fp32" and torch.equal(index.data, want.float())


def test_train_driver_feeds_the_pooled_loop_from_bag_stores(tt, tmp_path):
    """scripts/train.py --pool ... --pool-store: training and evaluation read per-entity bag stores; with --fast the epoch runs through
    step_batches on a step captured with a capacity, and prints the per-step losses of the same command without --fast.  Both runs
    seed torch and switch dropout off (the captured step draws its dropout seed with the step's scalars, the eager one per tower)."""
    def run(extra):
        cmd = [sys.executable, str(ROOT / "scripts" / "train.py"), "--results-csv", str(tmp_path / "r.csv"), "--output-dir", str(tmp_path / "m"),
               "--pairs", "3000", "--entities", "600", "--steps", "6", "--pool", "rgncd=mean", "cntrynm=sum", "ntceinsttcd=mean",
               "--pool-length", "3", "--seed", "11", "--dropout-rate", "0", "--log-interval", "1", "--pool-store"] + extra
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert "done: 6 steps" in r.stdout
        steps = [ln for ln in r.stdout.splitlines() if ln.startswith("step ")]
        assert len(steps) == 6
        return steps, r.stdout
    eager, _ = run([])
    fast, out = run(["--fast", "--pool-capture", "2"])
    assert "--pool-store: captured with bag_capacity" in out
    assert "--pool-store: 6 captured steps, 0 batches took the eager step" in out
    assert eager == fast
    r = subprocess.run([sys.executable, str(ROOT / "scripts" / "train.py"), "--pool-store"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 2 and "--pool-store needs --pool" in r.stderr
