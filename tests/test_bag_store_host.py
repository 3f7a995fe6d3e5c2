"""Host-side checks of the device-resident bag store (DeviceBagFeatureStore) and of what the loader builds on it: the constructor's
validations, the three construction forms, the torch reference of the gather against a Python loop, the per-batch id counts against
brute force, the routing of DevicePairLoader.step_batches with stand-ins for the captured steps, and the refusal that stays.  No GPU:
the stores live on the CPU and nothing here launches a kernel."""
import ctypes
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _bag_store_reference as R
from conftest import GOLD, ROOT

import jodalrob_twotower_amd as tt
from jodalrob_twotower_amd import _lib
from jodalrob_twotower_amd.data_loader import DeviceBagFeatureStore, DeviceFeatureStore, DevicePairLoader, batch_id_counts

KEYS = ["a", "b", "c"]


def _bags(rng, N, K, lengths_from=(0, 0, 1, 1, 2, 5)):
    return [[[int(i) for i in rng.integers(-3, 50, int(rng.choice(lengths_from)))] for _ in range(K)] for _ in range(N)]


def _store(seed=0, N=17, K=3):
    rng = np.random.default_rng(seed)
    dense = rng.standard_normal((N, 4)).astype(np.float32)
    bags = _bags(rng, N, K)
    return DeviceBagFeatureStore.from_bags(dense, bags, KEYS[:K], "cpu"), dense, bags


def test_constructor_validates_once():
    dense = np.zeros((2, 3), np.float32)
    ok = {"dense_projected": dense, "categorical_offsets": np.array([0, 1, 1, 4, 4, 5, 6]), "categorical_values": np.arange(6)}
    st = DeviceBagFeatureStore(ok, KEYS, "cpu")
    assert len(st) == 2 and st.keys == KEYS and st.run_lengths.tolist() == [4, 2] and st.run_lengths.dtype == torch.int64
    assert st.offsets.dtype == torch.int64 and st.values.dtype == torch.int64 and st.dense.dtype == torch.float32
    for bad, what in (([1, 1, 1, 4, 4, 5, 6], "start at 0"), ([0, 1, 0, 4, 4, 5, 6], "must not decrease"), ([0, 1, 1, 4, 4, 5, 7], "end at 7"),
                      ([0, 1, 1, 4, 4, 5], r"N\*K \+ 1 = 7"), ([0, 1, 1, 4, 4, 5, 6, 6, 6, 6], r"N\*K \+ 1 = 7")):
        with pytest.raises(ValueError, match=what):
            DeviceBagFeatureStore(dict(ok, categorical_offsets=np.array(bad)), KEYS, "cpu")
    with pytest.raises(ValueError, match=r"N\*K \+ 1 = 10"):                   # dense and offsets disagree on N
        DeviceBagFeatureStore(dict(ok, dense_projected=np.zeros((3, 3), np.float32)), KEYS, "cpu")
    with pytest.raises(ValueError, match="one id list per key"):
        DeviceBagFeatureStore.from_bags(dense, [[[1], [2]], [[3], [4], [5]]], KEYS, "cpu")


def test_the_three_construction_forms_agree():
    st, dense, bags = _store(1)
    lengths = [len(b) for row in bags for b in row]
    values = [i for row in bags for b in row for i in b]
    as_dict = DeviceBagFeatureStore({"dense_projected": torch.from_numpy(dense), "categorical_offsets": np.concatenate([[0], np.cumsum(lengths)]),
                                     "categorical_values": torch.tensor(values)}, KEYS, "cpu")
    for a, b in ((st.dense, as_dict.dense), (st.offsets, as_dict.offsets), (st.values, as_dict.values), (st.run_lengths, as_dict.run_lengths)):
        assert torch.equal(a, b)
    assert st.values.tolist() == values and min(values) < 0                     # ids are stored verbatim
    assert any(len(b) == 0 for row in bags for b in row)                        # empty bags included
    # from_single: every bag one id, the plain store's ids in its order
    cat = np.random.default_rng(2).integers(0, 9, (5, 3))
    plain = DeviceFeatureStore({"dense_projected": dense[:5], "categorical": cat}, KEYS, "cpu")
    single = DeviceBagFeatureStore.from_single(plain)
    want = DeviceBagFeatureStore.from_bags(dense[:5], [[[int(i)] for i in row] for row in cat], KEYS, "cpu")
    for a, b in ((single.dense, want.dense), (single.offsets, want.offsets), (single.values, want.values)):
        assert torch.equal(a, b)
    assert single.run_lengths.tolist() == [3] * 5 and single.keys == KEYS


@pytest.mark.parametrize("K", [1, 3])
def test_reference_gather_agrees_with_a_python_loop(K):
    st, _, _ = _store(3 + K, N=23, K=K)
    rng = np.random.default_rng(9)
    for ent in ([0], [22], [5, 5, 5], rng.integers(0, 23, 40).tolist(), [-4, 99, 0]):          # repeats; indices outside the store are clamped
        e = torch.tensor(ent)
        got, want = R.gather(st.dense, st.offsets, st.values, K, e), R.gather_loop(st.dense, st.offsets, st.values, K, e)
        for a, b in zip(got, want):
            assert a.dtype == b.dtype and torch.equal(a, b)
        assert got[1].numel() == len(ent) * K and got[2].numel() == int(got[1].sum())


def _world(seed, nN=25, nC=40, P=70):
    rng = np.random.default_rng(seed)
    ns = DeviceBagFeatureStore.from_bags(np.zeros((nN, 2), np.float32), _bags(rng, nN, 2), ["a", "b"], "cpu")
    cs = DeviceBagFeatureStore.from_bags(np.zeros((nC, 2), np.float32), _bags(rng, nC, 1, (0, 3, 9)), ["x"], "cpu")
    return ns, cs, np.stack([rng.integers(0, nN, P), rng.integers(0, nC, P)], 1)


@pytest.mark.parametrize("shuffle", [False, True])
def test_epoch_bag_ids_equal_brute_force(shuffle):
    ns, cs, pairs = _world(5)
    B = 16                                                                      # 70 pairs: four full batches and a ragged one of 6
    loader = DevicePairLoader(ns, cs, pairs, B, shuffle=shuffle, seed=4)
    if shuffle:
        with pytest.raises(ValueError, match="needs this epoch's order"):
            loader.epoch_bag_ids(None)
    order = loader.epoch_order()
    got = loader.epoch_bag_ids(order)
    sel = pairs if order is None else pairs[order.numpy()]
    for col, (side, st) in enumerate((("notice", ns), ("company", cs))):
        want = [sum(int(st.run_lengths[e]) for e in sel[lo:lo + B, col]) for lo in range(0, len(sel), B)]
        assert got[side].tolist() == want and len(want) == 5 and got[side].dtype == np.int64
        assert torch.equal(batch_id_counts(st.run_lengths, torch.as_tensor(sel[:, col]), B), torch.tensor(want))
    # a loader of plain stores has none; a mixed one counts its bag side only
    plain = DeviceFeatureStore({"dense_projected": np.zeros((25, 2), np.float32), "categorical": np.zeros((25, 2), np.int64)}, ["a", "b"], "cpu")
    assert DevicePairLoader(plain, plain, pairs[:, :1].repeat(2, 1), B, shuffle=False).epoch_bag_ids(None) is None
    assert list(DevicePairLoader(plain, cs, pairs, B, shuffle=False).epoch_bag_ids(None)) == ["company"]


class _Step:
    """a stand-in for a captured bag-mode step: records what step_from_store is handed"""

    def __init__(self, caps, rows):
        self.bag_capacity, self.static, self.calls = caps, {"notice": {"dense": torch.zeros(rows, 1)}}, []

    def step_from_store(self, ns, cs, pairs, order, lo, bag_ids=None, **kw):
        assert all(n <= self.bag_capacity[s] for s, n in bag_ids.items()) and not kw
        self.calls.append((lo, dict(bag_ids)))
        return "store"


@pytest.mark.parametrize("ragged", ["ragged_step", "eager", "over"])
def test_step_batches_routes_by_the_id_counts(ragged):
    ns, cs, pairs = _world(6)
    B = 16
    loader = DevicePairLoader(ns, cs, pairs, B, shuffle=False)
    loader.batch = lambda order, lo, neg=None, cells=None, bag_ids=None: ("batch", lo, int(bag_ids["company"][lo // B]))
    counts = loader.epoch_bag_ids(None)
    full_c = counts["company"][:4]
    cap = int(sorted(full_c)[2])                                                # one of the four full batches does not fit
    over = [int(c) > cap for c in full_c]
    assert sum(over) == 1
    full = _Step({"notice": 10 ** 6, "company": cap}, B)
    rag = None if ragged == "eager" else _Step({"notice": 10 ** 6, "company": 0 if ragged == "over" else 10 ** 6}, 70 - 4 * B)
    with pytest.warns(UserWarning, match=rf"{max(full_c)} ids on the company side.*room for {cap} \(bag_capacity\)"):
        out = list(loader.step_batches(full, eager_step=lambda b: b, ragged_step=rag))
    want = [("batch", 16 * k, int(full_c[k])) if over[k] else "store" for k in range(4)]
    want.append("store" if ragged == "ragged_step" else ("batch", 64, int(counts["company"][4])))
    assert out == want
    assert loader.eager_bag_batches == 1 + (ragged == "over" and counts["company"][4] > 0)
    assert full.calls == [(16 * k, {"notice": int(counts["notice"][k]), "company": int(full_c[k])}) for k in range(4) if not over[k]]
    if ragged == "ragged_step":
        assert rag.calls == [(64, {"notice": int(counts["notice"][4]), "company": int(counts["company"][4])})]
    # without an eager step nothing is skipped silently: the captured step gets the batch and refuses it itself
    full.calls.clear()
    with pytest.raises(AssertionError):
        list(loader.step_batches(full, eager_step=None))


def _cpu_task(pool):
    import json
    syn = json.loads((GOLD / "schema_synthetic.json").read_text())
    return tt.create_two_tower_train_task(syn["notice"]["categorical"], syn["company"]["categorical"], metadata_path=str(GOLD / "synthetic_metadata.csv"),
                                          categorical_embedding_dim=4, notice_dense_input_dim=3, company_dense_input_dim=2,
                                          tower_hidden_dims=[8, 4], final_embedding_dim=4, device="cpu", categorical_pooling=pool)


def test_a_plain_store_under_a_bag_mode_task_is_still_refused():
    ns, cs, pairs = _world(7)
    plain = DeviceFeatureStore({"dense_projected": np.zeros((40, 2), np.float32), "categorical": np.zeros((40, 1), np.int64)}, ["x"], "cpu")
    step = SimpleNamespace(task=_cpu_task({"company": "mean"}), bag_capacity={"company": 10 ** 6})
    msg = r"DevicePairLoader\.step_batches does not support bag mode \(categorical_pooling / CategoricalEmbedder\(pooling=\.\.\.\)\)"
    with pytest.raises(ValueError, match=msg):                                  # the company side pools, its store holds single ids
        next(DevicePairLoader(ns, plain, pairs, 16, shuffle=False).step_batches(step))
    both = SimpleNamespace(task=_cpu_task("mean"), bag_capacity={})
    with pytest.raises(ValueError, match=msg):                                  # both pool, only the company store holds bags
        next(DevicePairLoader(DeviceFeatureStore({"dense_projected": np.zeros((25, 2), np.float32), "categorical": np.zeros((25, 2), np.int64)},
                                                 ["a", "b"], "cpu"), cs, pairs, 16, shuffle=False).step_batches(both))
    with pytest.raises(ValueError, match=r"DevicePairLoader\.eval_batches does not support bag mode"):       # evaluation keeps refusing
        DevicePairLoader(ns, cs, pairs, 16, shuffle=False).eval_batches(step)


def test_every_piece_of_the_id_copy_on_the_host(tmp_path):
    """The integer code that places the gather's 16-byte pieces (csrc/tt_bag_store_piece.h) compiles without hipcc: a host program
    walks every piece of tiles of random runs under the address and undefined-behaviour sanitizers -- each position written once,
    from the right id, every index inside its array (tests/bag_store_piece_check.cpp)."""
    import subprocess
    exe = tmp_path / "piece_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", str(ROOT / "jodalrob-twotower_amd" / "csrc"), str(ROOT / "tests" / "bag_store_piece_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout[-500:] + r.stderr[-2000:]


def test_c_abi_declares_and_binds_the_gather():
    header = (ROOT / "include" / "twotower.h").read_text()
    for name in ("tt_bag_store_gather", "tt_bag_store_gather_workspace_bytes", "tt_bag_store_tile"):
        assert len(re.findall(rf"^(?:size_t|int) {name}\(", header, flags=re.M)) == 1, name
        assert name in _lib.SIGNATURES
    lib = _lib.load()
    from jodalrob_twotower_amd import ops
    assert lib.tt_bag_store_tile() == ops.BAG_STORE_TILE
    assert lib.tt_bag_store_gather_workspace_bytes(1, 1) == 8 and lib.tt_bag_store_gather_workspace_bytes(ops.BAG_STORE_TILE + 1, 2) == 32
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct tt_bag_store_side \{(.*?)\} tt_bag_store_side;", header, flags=re.S).group(1),
                  flags=re.S)
    assert re.findall(r"(\w+);", body) == [f[0] for f in _lib.BagStoreSide._fields_]
    assert ctypes.sizeof(_lib.BagStoreSide) == 8 * 8 + 3 * 8 + 4 * 4
