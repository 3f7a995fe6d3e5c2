"""Host-side checks of per-id weights in the device-resident bag store (DeviceBagFeatureStore(... "categorical_weights")) and of what
is built on them: the constructor's refusals and the three construction forms, the weighted torch reference against a Python loop,
ops.bag_store_gather's argument checks (raised before the library is loaded), GraphedTrainStep.step_from_store's two refusals on a
stand-in step, the routing of DevicePairLoader.step_batches with weighted stores, the train driver's parser and the C ABI.  No GPU:
the stores live on the CPU and nothing here launches a kernel."""
import ctypes
import re
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _bag_store_weight_reference as RW
from conftest import ROOT

from jodalrob_twotower_amd import _lib, ops, synthetic
from jodalrob_twotower_amd.data_loader import DeviceBagFeatureStore, DeviceFeatureStore, DevicePairLoader
from jodalrob_twotower_amd.graph import GraphedTrainStep

KEYS = ["a", "b", "c"]


def _bags(rng, N, K, lengths_from=(0, 0, 1, 1, 2, 5)):
    bags = [[[int(i) for i in rng.integers(-3, 50, int(rng.choice(lengths_from)))] for _ in range(K)] for _ in range(N)]
    weights = [[[float(np.float32(w)) for w in rng.random(len(bag)) * 4 - 2] for bag in row] for row in bags]
    return bags, weights


def _store(seed=0, N=17, K=3):
    rng = np.random.default_rng(seed)
    dense = rng.standard_normal((N, 4)).astype(np.float32)
    bags, weights = _bags(rng, N, K)
    return DeviceBagFeatureStore.from_bags(dense, bags, KEYS[:K], "cpu", weights=weights), dense, bags, weights


def test_constructor_takes_and_refuses_weights():
    dense = np.zeros((2, 3), np.float32)
    ok = {"dense_projected": dense, "categorical_offsets": np.array([0, 1, 1, 4, 4, 5, 6]), "categorical_values": np.arange(6)}
    assert DeviceBagFeatureStore(ok, KEYS, "cpu").weights is None
    odd = np.array([1.0, -0.0, np.nan, np.inf, 1e-42, -3.5], np.float32)        # kept verbatim: no finiteness check
    st = DeviceBagFeatureStore(dict(ok, categorical_weights=odd), KEYS, "cpu")
    assert st.weights.dtype == torch.float32 and st.weights.is_contiguous() and st.weights.shape == (6,)
    assert torch.equal(RW.bits(st.weights), torch.from_numpy(odd.view(np.int32)))
    assert st.run_lengths.tolist() == [4, 2] and torch.equal(st.values, torch.arange(6))
    strided = torch.arange(12, dtype=torch.float64)[::2]                        # another dtype, not contiguous: converted, 6 entries
    assert DeviceBagFeatureStore(dict(ok, categorical_weights=strided), KEYS, "cpu").weights.tolist() == [0.0, 2.0, 4.0, 6.0, 8.0, 10.0]
    for bad in (odd[:5], np.concatenate([odd, odd[:1]]), odd.reshape(2, 3), odd.reshape(6, 1), np.float32(1.0), torch.tensor(1.0),
                torch.zeros(0), torch.zeros(1, 6)):
        with pytest.raises(ValueError, match=r"categorical_weights: shape .* holds 6 ids"):
            DeviceBagFeatureStore(dict(ok, categorical_weights=bad), KEYS, "cpu")
    one = dict(ok, dense_projected=dense[:1], categorical_offsets=np.array([0, 0, 1, 1]), categorical_values=np.arange(1))
    with pytest.raises(ValueError, match="categorical_weights"):                # a 0-d weight is not reshaped into the one id's
        DeviceBagFeatureStore(dict(one, categorical_weights=torch.tensor(2.0)), KEYS, "cpu")
    assert DeviceBagFeatureStore(dict(one, categorical_weights=[2.0]), KEYS, "cpu").weights.tolist() == [2.0]
    # from_bags: a nested list shaped exactly like the bags
    bags = [[[1], [], [2, 3, 4]], [[], [5], [6]]]
    good = [[[0.5], [], [1.0, 2.0, 3.0]], [[], [4.0], [5.0]]]
    assert DeviceBagFeatureStore.from_bags(dense, bags, KEYS, "cpu", weights=good).weights.tolist() == [0.5, 1.0, 2.0, 3.0, 4.0, 5.0]
    assert DeviceBagFeatureStore.from_bags(dense, bags, KEYS, "cpu").weights is None
    for bad, what in ((good[:1], "per entity"), ([good[0], good[1][:2]], "per entity"), ([good[0], [[], [4.0], 5.0]], "one weight per id"),
                      ([[[0.5], [], [1.0, 2.0]], good[1]], "one weight per id"), ([[[0.5], [9.0], [1.0, 2.0, 3.0]], good[1]], "one weight per id")):
        with pytest.raises(ValueError, match=what):
            DeviceBagFeatureStore.from_bags(dense, bags, KEYS, "cpu", weights=bad)


def test_the_three_construction_forms_agree():
    st, dense, bags, weights = _store(1)
    lengths = [len(b) for row in bags for b in row]
    flat_w = [w for row in weights for wb in row for w in wb]
    as_dict = DeviceBagFeatureStore({"dense_projected": torch.from_numpy(dense), "categorical_offsets": np.concatenate([[0], np.cumsum(lengths)]),
                                     "categorical_values": torch.tensor([i for row in bags for b in row for i in b]),
                                     "categorical_weights": torch.tensor(flat_w, dtype=torch.float32)}, KEYS, "cpu")
    for a, b in ((st.dense, as_dict.dense), (st.offsets, as_dict.offsets), (st.values, as_dict.values), (st.run_lengths, as_dict.run_lengths)):
        assert torch.equal(a, b)
    assert torch.equal(RW.bits(st.weights), RW.bits(as_dict.weights)) and st.weights.tolist() == flat_w and min(flat_w) < 0
    # synthetic.bag_store(weights="uniform"): the ids of the unweighted store of the same seed, the weights ragged_bags draws
    cat = np.random.default_rng(2).integers(0, 9, (40, 3))
    plain = DeviceFeatureStore({"dense_projected": np.zeros((40, 4), np.float32), "categorical": cat}, KEYS, "cpu")
    a = synthetic.bag_store(plain, [9, 9, 9], ["a", "c"], 2.5, seed=5)
    b = synthetic.bag_store(plain, [9, 9, 9], ["a", "c"], 2.5, seed=5, weights="uniform")
    assert a.weights is None and torch.equal(a.values, b.values) and torch.equal(a.offsets, b.offsets)
    kjt = synthetic.ragged_bags(tt_kjt(plain), [9, 9, 9], ["a", "c"], 2.5, 5, "uniform")
    assert torch.equal(RW.bits(b.weights), RW.bits(kjt.weights())) and b.weights.numel() == b.values.numel() > 40 * 3
    assert float(b.weights.min()) >= 0.5 and float(b.weights.max()) < 1.5 and len(set(b.weights.tolist())) > 10
    again = DeviceBagFeatureStore({"dense_projected": b.dense, "categorical_offsets": b.offsets, "categorical_values": b.values,
                                   "categorical_weights": b.weights}, KEYS, "cpu")
    assert torch.equal(RW.bits(again.weights), RW.bits(b.weights))
    with pytest.raises(ValueError, match="weights must be None or 'uniform'"):
        synthetic.bag_store(plain, [9, 9, 9], ["a"], 2.5, seed=5, weights="normal")
    assert DeviceBagFeatureStore.from_single(plain).weights is None              # from_single stays weightless


def tt_kjt(plain):
    from jodalrob_twotower_amd.kjt import KeyedJaggedTensor
    return KeyedJaggedTensor(list(plain.keys), plain.categorical.reshape(-1))


@pytest.mark.parametrize("K", [1, 3])
def test_weighted_reference_agrees_with_a_python_loop(K):
    st, _, _, _ = _store(3 + K, N=23, K=K)
    st.weights[:4] = torch.tensor([0x7FC01234, 0xFF800001 - (1 << 32), -(1 << 31), 0x00000007], dtype=torch.int32).view(torch.float32)
    rng = np.random.default_rng(9)
    for ent in ([0], [22], [5, 5, 5], rng.integers(0, 23, 40).tolist(), [-4, 99, 0]):          # repeats; indices outside the store are clamped
        e = torch.tensor(ent)
        got = RW.gather(st.dense, st.offsets, st.values, st.weights, K, e)
        want = RW.gather_loop(st.dense, st.offsets, st.values, st.weights, K, e)
        for a, b in zip(got[:3], want[:3]):
            assert a.dtype == b.dtype and torch.equal(a, b)
        assert got[3].dtype == torch.float32 and torch.equal(RW.bits(got[3]), RW.bits(want[3]))
        assert got[1].numel() == len(ent) * K and got[2].numel() == got[3].numel() == int(got[1].sum())


def test_ops_gather_checks_the_weight_arguments_before_the_library(monkeypatch):
    def no_library():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", no_library)
    st, _, _, _ = _store(2)
    B, K = 4, 3
    ent = torch.arange(B)
    outs = lambda: (torch.zeros(B, 4), torch.zeros(B * K, dtype=torch.int64), torch.zeros(30, dtype=torch.int64))
    side = lambda w, wo, ids_n=30: ops.BagStoreSide(ent, 1, st.dense, st.offsets, st.values, K, *outs()[:2], torch.zeros(ids_n, dtype=torch.int64), -1, w, wo)
    w, wo = st.weights, torch.zeros(30)
    assert ops.BagStoreSide(ent, 1, st.dense, st.offsets, st.values, K, *outs()).weights is None                # the defaults: ids alone
    for s, what in ((side(w, None), "weights alone was given"), (side(None, wo), "weights_out alone was given"),
                    (side(w[:-1], wo), rf"{w.numel() - 1} weights for {w.numel()} ids"), (side(w, wo[:29]), "weights_out holds 29 entries, ids_out 30"),
                    (side(w, torch.zeros(31)), "weights_out holds 31 entries"), (side(w.double(), wo), "weights must be a contiguous 1-D float32"),
                    (side(w, wo.to(torch.int32)), "weights_out must be a contiguous 1-D float32"),
                    (side(torch.zeros(2 * w.numel())[::2], wo), "weights must be a contiguous"), (side(w, torch.zeros(60)[::2]), "weights_out must be a contiguous"),
                    (side(w.reshape(1, -1), wo), "weights must be a contiguous 1-D"), (side(w.to("meta"), wo), "weights must be a contiguous 1-D float32 tensor on cpu")):
        with pytest.raises(ValueError, match="bag_store_gather: side 0: .*" + what):
            ops.bag_store_gather([], [s], B)
        with pytest.raises(ValueError, match="bag_store_gather: side 1: "):     # the second side of a call, beside an unweighted one
            ops.bag_store_gather([], [side(None, None), s], B)
    with pytest.raises(AssertionError, match="the library was loaded"):         # well-formed sides get as far as the library
        ops.bag_store_gather([], [side(w, wo)], B)
    with pytest.raises(AssertionError, match="the library was loaded"):
        ops.bag_store_gather([], [side(None, None)], B)


def _fake_step(bag, bag_w):
    return SimpleNamespace(_terms=frozenset(), _bag=bag, _bag_w=frozenset(bag_w))


def test_step_from_store_refuses_weights_that_do_not_match_the_capture():
    weighted, _, _, _ = _store(4)
    plain_bags = DeviceBagFeatureStore({"dense_projected": weighted.dense, "categorical_offsets": weighted.offsets,
                                        "categorical_values": weighted.values}, KEYS, "cpu")
    single = DeviceFeatureStore({"dense_projected": np.zeros((17, 4), np.float32), "categorical": np.zeros((17, 3), np.int64)}, KEYS, "cpu")
    pairs = torch.zeros((8, 2), dtype=torch.int64)
    prefix = "step_from_store: the step was captured with per-id weights"
    # captured WITH weights: every such side needs a bag store that carries them
    step = _fake_step({"notice": 50, "company": 50}, {"notice", "company"})
    for ns, cs, side in ((None, None, "company"), (weighted, plain_bags, "company"), (plain_bags, weighted, "notice"), (weighted, single, "company"),
                         (single, weighted, "notice")):
        with pytest.raises(ValueError, match=rf"{prefix} on \['company', 'notice'\], and the {side} store carries none"):
            GraphedTrainStep.step_from_store(step, ns, cs, pairs)
    one = _fake_step({"company": 50}, {"company"})
    with pytest.raises(ValueError, match=rf"{prefix} on \['company'\], and the company store"):
        GraphedTrainStep.step_from_store(one, single, plain_bags, pairs)
    # captured WITHOUT them on a bag-mode side: a weighted store's weights would be dropped silently
    for step, ns, cs, side in ((_fake_step({"notice": 50, "company": 50}, ()), plain_bags, weighted, "company"),
                               (_fake_step({"notice": 50, "company": 50}, {"company"}), weighted, weighted, "notice"),
                               (_fake_step({"company": 50}, ()), single, weighted, "company")):
        with pytest.raises(ValueError, match=rf"step_from_store: the {side} store carries per-id weights, but the step was captured without them"):
            GraphedTrainStep.step_from_store(step, ns, cs, pairs)


class _Step:
    """a stand-in for a captured bag-mode step: records what step_from_store is handed"""

    def __init__(self, caps, rows):
        self.bag_capacity, self.static, self.calls = caps, {"notice": {"dense": torch.zeros(rows, 1)}}, []

    def step_from_store(self, ns, cs, pairs, order, lo, bag_ids=None, **kw):
        assert all(n <= self.bag_capacity[s] for s, n in bag_ids.items()) and not kw
        self.calls.append((lo, dict(bag_ids), ns, cs))
        return "store"


@pytest.mark.parametrize("company", ["weighted", "plain"])
def test_step_batches_routes_weighted_stores_by_the_id_counts(company):
    """the loader counts ids, whatever else the stores hold: a weighted notice store beside a weighted bag store or a plain store"""
    rng = np.random.default_rng(6)
    nN, nC, P, B = 25, 40, 70, 16
    bags, weights = _bags(rng, nN, 2)
    ns = DeviceBagFeatureStore.from_bags(np.zeros((nN, 2), np.float32), bags, ["a", "b"], "cpu", weights=weights)
    if company == "weighted":
        cbags, cw = _bags(rng, nC, 1, (0, 3, 9))
        cs = DeviceBagFeatureStore.from_bags(np.zeros((nC, 2), np.float32), cbags, ["x"], "cpu", weights=cw)
    else:
        cs = DeviceFeatureStore({"dense_projected": np.zeros((nC, 2), np.float32), "categorical": np.zeros((nC, 1), np.int64)}, ["x"], "cpu")
    pr = np.random.default_rng(60)                                             # (a stream of its own: the same pairs in both cases)
    pairs = np.stack([pr.integers(0, nN, P), pr.integers(0, nC, P)], 1)
    loader = DevicePairLoader(ns, cs, pairs, B, shuffle=False)
    counts = loader.epoch_bag_ids(None)
    assert sorted(counts) == (["company", "notice"] if company == "weighted" else ["notice"])
    unweighted = DeviceBagFeatureStore({"dense_projected": ns.dense, "categorical_offsets": ns.offsets, "categorical_values": ns.values}, ["a", "b"], "cpu")
    assert counts["notice"].tolist() == DevicePairLoader(unweighted, cs, pairs, B, shuffle=False).epoch_bag_ids(None)["notice"].tolist()
    full_n = counts["notice"][:4]
    cap = int(sorted(full_n)[2])                                                # the fullest of the four full batches does not fit
    over = [int(c) > cap for c in full_n]
    assert sum(over) == 1
    seen = []
    loader.batch = lambda order, lo, neg=None, cells=None, bag_ids=None: seen.append(lo) or ("batch", lo)
    full = _Step({"notice": cap, "company": 10 ** 6}, B)
    with pytest.warns(UserWarning, match=rf"{max(full_n)} ids on the notice side.*room for {cap} \(bag_capacity\)"):
        out = list(loader.step_batches(full, eager_step=lambda b: b))
    assert out == [("batch", 16 * k) if over[k] else "store" for k in range(4)] + [("batch", 64)]
    assert loader.eager_bag_batches == 1 and seen == [16 * over.index(True), 64]
    assert [c[0] for c in full.calls] == [16 * k for k in range(4) if not over[k]]
    assert all(c[2] is ns and c[3] is cs and c[2].weights is not None for c in full.calls)         # the stores travel as they are
    assert all(c[1] == {side: int(counts[side][c[0] // B]) for side in counts} for c in full.calls)


def test_train_driver_parser():
    base = [sys.executable, str(ROOT / "scripts" / "train.py"), "--pool-store-weights"]
    for extra in ([], ["--pool", "rgncd=mean"]):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 2 and "--pool-store-weights needs --pool ... --pool-store" in r.stderr, r.stderr[-500:]
    r = subprocess.run([sys.executable, str(ROOT / "scripts" / "train.py"), "--pool-weights", "--pool", "rgncd=mean", "--pool-store"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "--pool-weights: not with --pool-store" in r.stderr and "--pool-store-weights" in r.stderr


def test_c_abi_declares_and_binds_the_weighted_gather():
    header = (ROOT / "include" / "twotower.h").read_text()
    assert len(re.findall(r"^int tt_bag_store_gather_w\(", header, flags=re.M)) == 1 and "tt_bag_store_gather_w" in _lib.SIGNATURES
    fields = lambda name: re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", re.search(rf"typedef struct {name} \{{(.*?)\}} {name};", header,
                                                                                   flags=re.S).group(1), flags=re.S))
    plain, w = fields("tt_bag_store_side"), fields("tt_bag_store_side_w")
    assert w == plain + ["weights", "weights_out"]                              # tt_bag_store_side's fields, then the weights
    assert w == [f[0] for f in _lib.BagStoreSideW._fields_] and plain == [f[0] for f in _lib.BagStoreSide._fields_]
    assert [f[1] for f in _lib.BagStoreSideW._fields_[:len(plain)]] == [f[1] for f in _lib.BagStoreSide._fields_]
    assert ctypes.sizeof(_lib.BagStoreSideW) == ctypes.sizeof(_lib.BagStoreSide) + 16 == 8 * 8 + 3 * 8 + 4 * 4 + 2 * 8
    assert _lib.SIGNATURES["tt_bag_store_gather_w"][1][5] == ctypes.POINTER(_lib.BagStoreSideW)
    assert _lib.SIGNATURES["tt_bag_store_gather_w"][1][:5] == _lib.SIGNATURES["tt_bag_store_gather"][1][:5]
    assert _lib.SIGNATURES["tt_bag_store_gather_w"][1][6:] == _lib.SIGNATURES["tt_bag_store_gather"][1][6:]
    assert hasattr(_lib.load(), "tt_bag_store_gather_w")                        # the built library exports it
