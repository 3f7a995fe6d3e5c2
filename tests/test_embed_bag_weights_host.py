"""Weighted bags (one f32 weight per id): what can be checked without a GPU -- the f64 reference of tests/_bag_weight_reference.py
against the unweighted reference and against torch's embedding_bag(per_sample_weights=) in float64, the KJT plumbing (weights(),
to / pin_memory, concat_kjt, build_bag_kjt's validation, synthetic.ragged_bags(weights="uniform")), the new C-ABI entries, and the
refusals that are raised before anything touches a device."""
import re

import numpy as np
import pytest
import torch

import _bag_reference as R
import _bag_weight_reference as W
from conftest import GOLD, ROOT

import jodalrob_twotower_amd as tt
from jodalrob_twotower_amd import _lib, synthetic

VOCABS = [50, 300, 120]
OFFS = np.array([0, 50, 350], dtype=np.int64)
POOLING = ["mean", "sum", "mean"]
B, K, E = 11, 3, 5


def _case(seed):
    rng = np.random.default_rng(seed)
    lengths = rng.choice([0, 1, 2, 3, 5, 9], B * K).astype(np.int64)
    nnz = int(lengths.sum())
    ids = np.concatenate([rng.integers(-3, VOCABS[s % K] + 3, int(n)) for s, n in enumerate(lengths)]).astype(np.int64)
    table = rng.standard_normal((sum(VOCABS), E))
    weights = rng.uniform(-2, 2, nnz).astype(np.float32)
    d_out = rng.standard_normal((B, K * E))
    return rng, lengths, ids, table, weights, d_out


def test_symbols_in_header_and_library():
    header = (ROOT / "include" / "twotower.h").read_text()
    lib = _lib.load()
    for name in ("tt_embed_bag_fwd_w", "tt_embed_bag_fwd_cap_w", "tt_embed_bag_grad_bwd_w"):
        assert re.search(rf"^\s*int\s+{name}\s*\(", header, flags=re.M), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    S = _lib.SIGNATURES
    # the unweighted entries' arguments plus (weights, w_out) in front of the stream / pos_w behind inv_len
    assert S["tt_embed_bag_fwd_w"][1][:9] == S["tt_embed_bag_fwd"][1][:9] and len(S["tt_embed_bag_fwd_w"][1]) == len(S["tt_embed_bag_fwd"][1]) + 2
    assert S["tt_embed_bag_fwd_cap_w"] == S["tt_embed_bag_fwd_w"]
    assert len(S["tt_embed_bag_grad_bwd_w"][1]) == len(S["tt_embed_bag_grad_bwd"][1]) + 1
    assert re.search(r"#define TT_ABI_VERSION 2\b", header)                        # entries were added, none changed


@pytest.mark.parametrize("seed", range(3))
def test_ones_are_the_unweighted_reference(seed):
    _, lengths, ids, table, _, d_out = _case(seed)
    ones = np.ones(ids.size, np.float32)
    a = R.bag_forward(table, ids, lengths, OFFS, VOCABS, POOLING)
    b = W.weighted_forward(table, ids, lengths, OFFS, VOCABS, POOLING, ones)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    a = R.bag_backward(d_out, ids, lengths, OFFS, VOCABS, POOLING)
    b = W.weighted_backward(d_out, ids, lengths, OFFS, VOCABS, POOLING, ones)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


def torch_weighted_bags(table, ids, lengths, weights):
    """The float64 torch expression of the weighted pooling over the clamped fused rows: embedding_bag(mode="sum",
    per_sample_weights=) and, for the mean keys, that sum divided by the bag's length.  table: a float64 tensor (may require grad)."""
    slots, rows = R.positions(ids, lengths, OFFS, VOCABS)
    offsets = torch.from_numpy(np.concatenate([[0], np.cumsum(lengths)[:-1]]).astype(np.int64))
    pooled = torch.nn.functional.embedding_bag(torch.from_numpy(rows), table, offsets, mode="sum",
                                               per_sample_weights=torch.from_numpy(weights[:rows.size].astype(np.float64)))
    mean = torch.from_numpy(np.tile(np.array([p == "mean" for p in POOLING]), B))
    div = torch.where(mean & torch.from_numpy(lengths > 0), torch.from_numpy(np.maximum(lengths, 1)).to(torch.float64),
                      torch.ones(lengths.size, dtype=torch.float64))
    return (pooled / div[:, None]).reshape(B, K * E)


@pytest.mark.parametrize("seed", range(3))
def test_reference_equals_torch_embedding_bag_in_f64(seed):
    _, lengths, ids, table, weights, d_out = _case(10 + seed)
    t = torch.from_numpy(table).requires_grad_(True)
    want = torch_weighted_bags(t, ids, lengths, weights)
    got, mag, _, _ = W.weighted_forward(table, ids, lengths, OFFS, VOCABS, POOLING, weights)
    assert np.allclose(got, want.detach().numpy(), rtol=1e-12, atol=1e-12 * float(mag.max()))
    empty = np.repeat(lengths.reshape(B, K) == 0, E, axis=1)
    assert empty.any() and not got[empty].any()
    # the table gradient: torch's autograd gradient of the same expression
    want.backward(torch.from_numpy(d_out))
    uniq, sums, abs_sums, _ = W.weighted_backward(d_out, ids, lengths, OFFS, VOCABS, POOLING, weights)
    dense = R.dense_grad(sum(VOCABS), E, uniq, sums)
    g = t.grad.numpy()
    assert np.abs(dense - g).max() <= 1e-12 * np.abs(g).max()
    # handing over the f32 1 / L of a kernel instead of the exact one moves the gradient by that rounding alone
    inv = R.slot_weights(lengths, POOLING).astype(np.float32)
    _, sums32, _, _ = W.weighted_backward(d_out, ids, lengths, OFFS, VOCABS, POOLING, weights, inv_len=inv)
    assert (np.abs(sums32 - sums) <= 2.0 ** -24 * abs_sums * (1 + 1e-6)).all()


def test_kjt_carries_weights():
    keys = ["a", "b"]
    v, ln, w = torch.arange(5), torch.tensor([2, 0, 1, 2]), torch.tensor([0.5, 1.0, 2.0, -1.0, 0.0])
    plain = tt.KeyedJaggedTensor(keys, v, ln)
    assert plain.weights_or_none() is None
    with pytest.raises(ValueError, match="carries no weights"):
        plain.weights()
    k = tt.KeyedJaggedTensor(keys, v, ln, w)
    assert k.weights() is w and k.weights_or_none() is w
    moved = k.to("cpu")
    assert torch.equal(moved.weights(), w) and torch.equal(moved.values(), v) and torch.equal(moved.lengths(), ln)
    assert plain.to("cpu").weights_or_none() is None
    if torch.cuda.is_available():                                                 # (pinning needs an accelerator runtime)
        pinned = k.pin_memory()
        assert pinned.weights().is_pinned() and torch.equal(pinned.weights(), w) and plain.pin_memory().weights_or_none() is None


def test_concat_kjt_three_cases():
    keys = ["a", "b"]
    a = tt.KeyedJaggedTensor(keys, torch.tensor([1, 2, 3]), torch.tensor([2, 1]), torch.tensor([0.5, 2.0, 3.0]))
    b = tt.KeyedJaggedTensor(keys, torch.tensor([7]), torch.tensor([0, 1]), torch.tensor([4.0]))
    plain_a = tt.KeyedJaggedTensor(keys, a.values(), a.lengths())
    plain_b = tt.KeyedJaggedTensor(keys, b.values(), b.lengths())
    both = tt.concat_kjt(a, b)
    assert both.values().tolist() == [1, 2, 3, 7] and both.lengths().tolist() == [2, 1, 0, 1]
    assert both.weights().tolist() == [0.5, 2.0, 3.0, 4.0] and both.weights().dtype == torch.float32
    assert tt.concat_kjt(a, plain_b).weights().tolist() == [0.5, 2.0, 3.0, 1.0]      # the side without weights: ones
    assert tt.concat_kjt(plain_a, b).weights().tolist() == [1.0, 1.0, 1.0, 4.0]
    assert tt.concat_kjt(plain_a, plain_b).weights_or_none() is None               # ... and none stay none


def test_build_bag_kjt_weights_and_validation():
    keys = ["a", "b"]
    bags = [[[3, 4], []], [[5], [6, 7, 8]]]
    wts = [[[0.5, 2.0], []], [[1.0], [0.25, 0.0, -1.0]]]
    k = tt.build_bag_kjt(keys, bags=bags, weights=wts)
    assert k.values().tolist() == [3, 4, 5, 6, 7, 8] and k.lengths().tolist() == [2, 0, 1, 3]
    assert k.weights().tolist() == [0.5, 2.0, 1.0, 0.25, 0.0, -1.0] and k.weights().dtype == torch.float32
    t = tt.build_bag_kjt(keys, bags=bags, weights=torch.arange(6, dtype=torch.float64))
    assert t.weights().dtype == torch.float32 and t.weights().tolist() == [0, 1, 2, 3, 4, 5]
    v = tt.build_bag_kjt(keys, values=k.values(), lengths=k.lengths(), weights=k.weights())
    assert torch.equal(v.weights(), k.weights())
    assert tt.build_bag_kjt(keys, bags=bags).weights_or_none() is None
    with pytest.raises(ValueError, match="5 weights for 6 ids"):                  # wrong count
        tt.build_bag_kjt(keys, values=k.values(), lengths=k.lengths(), weights=torch.ones(5))
    with pytest.raises(ValueError, match="5 weights for 6 ids"):
        tt.build_bag_kjt(keys, bags=bags, weights=torch.ones(5))
    with pytest.raises(ValueError, match="does not have its bag's length"):
        tt.build_bag_kjt(keys, bags=bags, weights=[[[0.5], []], [[1.0], [0.25, 0.0, -1.0]]])
    with pytest.raises(ValueError, match="one weight per id"):                    # wrong nesting: floats where a bag's list belongs
        tt.build_bag_kjt(keys, bags=bags, weights=[[0.5, 2.0], [1.0, 0.25]])
    with pytest.raises(ValueError, match="one weight list per key"):              # ... a flat list
        tt.build_bag_kjt(keys, bags=bags, weights=[0.5, 2.0, 1.0, 0.25, 0.0, -1.0])
    with pytest.raises(ValueError, match="one weight list per key"):
        tt.build_bag_kjt(keys, bags=bags, weights=[[[0.5, 2.0], []]])
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="non-finite"):
            tt.build_bag_kjt(keys, bags=bags, weights=[[[0.5, bad], []], [[1.0], [0.25, 0.0, -1.0]]])
    with pytest.raises(ValueError, match="tensor"):
        tt.build_bag_kjt(keys, values=k.values(), lengths=k.lengths(), weights=[0.5] * 6)


def test_ragged_bags_uniform_weights():
    keys, vocabs = ["a", "b", "c"], [40, 50, 60]
    base = tt.KeyedJaggedTensor(keys, torch.arange(64 * 3) % 40)
    plain = synthetic.ragged_bags(base, vocabs, {"a", "c"}, 4.0, seed=5)
    k = synthetic.ragged_bags(base, vocabs, {"a", "c"}, 4.0, seed=5, weights="uniform")
    assert plain.weights_or_none() is None
    assert torch.equal(k.values(), plain.values()) and torch.equal(k.lengths(), plain.lengths())      # the ids are the unweighted draw's
    w = k.weights()
    assert w.dtype == torch.float32 and w.shape == k.values().shape
    assert bool((w >= 0.5).all()) and bool((w < 1.5).all())
    ln = k.lengths()
    starts = (torch.cumsum(ln, 0) - ln)[ln > 0]
    assert bool((w[starts] == 1.0).all())                                          # a bag's first id weighs 1
    rest = torch.ones_like(w, dtype=torch.bool)
    rest[starts] = False
    assert rest.any() and w[rest].unique().numel() > rest.sum() // 2               # the others are drawn
    again = synthetic.ragged_bags(base, vocabs, {"a", "c"}, 4.0, seed=5, weights="uniform")
    other = synthetic.ragged_bags(base, vocabs, {"a", "c"}, 4.0, seed=6, weights="uniform")
    assert torch.equal(again.weights(), w)
    assert other.weights().shape != w.shape or not torch.equal(other.weights(), w)
    with pytest.raises(ValueError, match="None or 'uniform'"):
        synthetic.ragged_bags(base, vocabs, {"a"}, 4.0, seed=5, weights="normal")


def test_refusals_that_need_no_device(schema_syn):
    """A weighted KJT into an embedder that is not in bag mode, and an example batch whose weights do not match its ids: raised
    before anything touches a device (the modules live on the CPU)."""
    from jodalrob_twotower_amd.cat_embed import CategoricalEmbedder
    from jodalrob_twotower_amd.graph import GraphedTrainStep
    from jodalrob_twotower_amd.optim import FusedAdam
    kn, kc = schema_syn["notice"]["categorical"], schema_syn["company"]["categorical"]
    meta = str(GOLD / "synthetic_metadata.csv")
    emb = CategoricalEmbedder(kc, meta, "company", embedding_dim=4, device="cpu")
    n = 2 * len(kc)
    weighted = tt.KeyedJaggedTensor(kc, torch.zeros(n, dtype=torch.long), torch.ones(n, dtype=torch.long), torch.ones(n))
    with pytest.raises(ValueError, match="not in bag mode"):
        emb(weighted)
    task = tt.create_two_tower_train_task(kn, kc, metadata_path=meta, categorical_embedding_dim=4, notice_dense_input_dim=3,
                                          company_dense_input_dim=2, tower_hidden_dims=[8, 4], final_embedding_dim=4, device="cpu",
                                          categorical_pooling={"company": "mean"})
    Bn = 4
    lengths = torch.tensor([2, 0, 1, 3] * len(kc))[:Bn * len(kc)]
    nnz = int(lengths.sum())
    bad = tt.KeyedJaggedTensor(kc, torch.zeros(nnz, dtype=torch.long), lengths, torch.ones(nnz - 1))
    batch = {"notice": {"dense": torch.zeros(Bn, 3), "kjt": tt.build_batch_kjt(torch.zeros((Bn, len(kn)), dtype=torch.long), kn)},
             "company": {"dense": torch.zeros(Bn, 2), "kjt": bad}}
    with pytest.raises(ValueError, match=rf"company: the example batch carries {nnz - 1} weights for {nnz} ids"):
        GraphedTrainStep(task, FusedAdam.for_task(task, lr=1e-2), batch, bag_capacity=64)
    # weights on the plain (notice) side of a towers pass are refused as well, not dropped
    wn = tt.KeyedJaggedTensor(kn, torch.zeros(Bn * len(kn), dtype=torch.long), None, torch.ones(Bn * len(kn)))
    good = tt.build_bag_kjt(kc, values=torch.zeros(nnz, dtype=torch.long), lengths=lengths, weights=torch.ones(nnz))
    from jodalrob_twotower_amd.towers import run_towers
    model = task.two_tower_model
    with pytest.raises(ValueError, match="not in bag mode"):
        run_towers([model.notice_tower, model.company_tower], [{"dense": torch.zeros(Bn, 3), "kjt": wn}, {"dense": torch.zeros(Bn, 2), "kjt": good}])


def test_train_driver_refuses_pool_weights_with_pool_store():
    """scripts/train.py --pool-weights: refused by the argument parser with --pool-store (the bag stores hold ids alone) and without
    --pool, before anything is built"""
    import subprocess
    import sys
    base = [sys.executable, str(ROOT / "scripts" / "train.py"), "--pool-weights"]
    r = subprocess.run(base + ["--pool", "rgncd=mean", "--pool-store"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "--pool-weights: not with --pool-store" in r.stderr
    r = subprocess.run(base, capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "--pool-weights needs --pool" in r.stderr
