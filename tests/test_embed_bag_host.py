"""Host-side checks of the pooled multi-valued lookup (embedding bags): the f64 reference of tests/_bag_reference.py against
torch.nn.functional.embedding_bag, the KJT helpers, the C ABI declarations and the unchanged length-one interface.  No GPU."""
import inspect
import re

import numpy as np
import pytest
import torch

import _bag_reference as R
import oracle_np as O
from conftest import GOLD, ROOT

import jodalrob_twotower_amd as tt
from jodalrob_twotower_amd import _lib


def _ragged(rng, B, vocabs, lengths_from, lo=0, hi=0):
    """ids / lengths of B samples over len(vocabs) keys; ids in [-lo, V + hi)"""
    K = len(vocabs)
    lengths = rng.choice(lengths_from, B * K).astype(np.int64)
    ids = np.concatenate([rng.integers(-lo, vocabs[s % K] + hi, int(L)) for s, L in enumerate(lengths)] + [np.zeros(0, np.int64)])
    return ids.astype(np.int64), lengths


@pytest.mark.parametrize("pooling", [["sum", "sum", "sum"], ["mean", "mean", "mean"], ["mean", "sum", "mean"]])
def test_reference_agrees_with_torch_embedding_bag(pooling):
    """Per key, in f64: forward and the autograd gradient of the table; empty bags included."""
    rng = np.random.default_rng(3)
    B, E, vocabs = 23, 5, [7, 40, 13]
    K = len(vocabs)
    offs = np.concatenate([[0], np.cumsum(vocabs)[:-1]]).astype(np.int64)
    table = rng.standard_normal((sum(vocabs), E))
    ids, lengths = _ragged(rng, B, vocabs, [0, 1, 2, 3, 7])
    assert (lengths == 0).any()
    d_out = rng.standard_normal((B, K * E))
    out, _, slots, rows = R.bag_forward(table, ids, lengths, offs, vocabs, pooling)
    uniq, sums, _, counts = R.bag_backward(d_out, ids, lengths, offs, vocabs, pooling)
    grad = R.dense_grad(sum(vocabs), E, uniq, sums)
    starts = np.concatenate([[0], np.cumsum(lengths)])
    for k in range(K):
        w = torch.tensor(table[offs[k]:offs[k] + vocabs[k]], dtype=torch.float64, requires_grad=True)
        sel = np.arange(B) * K + k
        kid = np.concatenate([ids[starts[s]:starts[s + 1]] for s in sel] + [np.zeros(0, np.int64)])
        koff = np.concatenate([[0], np.cumsum(lengths[sel])[:-1]])
        got = torch.nn.functional.embedding_bag(torch.from_numpy(kid), w, torch.from_numpy(koff), mode=pooling[k])
        np.testing.assert_allclose(out[:, k * E:(k + 1) * E], got.detach().numpy(), rtol=1e-13, atol=1e-14)
        assert not out[lengths[sel] == 0, k * E:(k + 1) * E].any()
        got.backward(torch.from_numpy(d_out[:, k * E:(k + 1) * E].copy()))
        np.testing.assert_allclose(grad[offs[k]:offs[k] + vocabs[k]], w.grad.numpy(), rtol=1e-13, atol=1e-14)
    assert counts.sum() == lengths.sum() and np.array_equal(np.repeat(np.arange(B * K), lengths), slots)


def test_reference_clamps_out_of_range_and_negative_ids():
    rng = np.random.default_rng(4)
    vocabs, B = [5, 9], 11
    offs = np.array([0, 5], np.int64)
    ids, lengths = _ragged(rng, B, vocabs, [1, 2, 4], lo=6, hi=6)
    assert (ids < 0).any() and (ids >= 9).any()
    slots, rows = R.positions(ids, lengths, offs, vocabs)
    k = slots % 2
    want = offs[k] + np.clip(ids, 0, np.array(vocabs)[k] - 1)
    assert np.array_equal(rows, want) and rows.min() >= 0 and (rows[k == 0] < 5).all() and (rows[k == 1] < 14).all()
    assert np.array_equal(np.clip(ids[:4], 0, None), O.unpack_clamp_ids(ids[:4], [10 ** 9] * 2).reshape(-1))


def test_kjt_helper_and_concat_round_trip():
    keys = ["a", "b"]
    bags = [[[3], [1, 2, 2]], [[], [7]], [[5, 6], []]]
    k = tt.build_bag_kjt(keys, bags=bags)
    assert k.keys() == keys and k.lengths().tolist() == [1, 3, 0, 1, 2, 0] and k.values().tolist() == [3, 1, 2, 2, 7, 5, 6]
    k2 = tt.build_bag_kjt(keys, values=k.values(), lengths=k.lengths())
    assert torch.equal(k2.values(), k.values()) and torch.equal(k2.lengths(), k.lengths())
    # rebuild the per-slot lists from (values, lengths)
    off = np.concatenate([[0], np.cumsum(k.lengths().numpy())])
    back = [[k.values()[off[b * 2 + j]:off[b * 2 + j + 1]].tolist() for j in range(2)] for b in range(3)]
    assert back == bags
    both = tt.concat_kjt(k, tt.build_bag_kjt(keys, bags=[[[9, 9], [4]]]))
    assert both.lengths().tolist() == [1, 3, 0, 1, 2, 0, 2, 1] and both.values().tolist() == [3, 1, 2, 2, 7, 5, 6, 9, 9, 4]
    # all lengths one: exactly build_batch_kjt's wire format
    ids = torch.arange(8).view(4, 2)
    one = tt.build_bag_kjt(keys, bags=[[[int(v)] for v in row] for row in ids])
    plain = tt.build_batch_kjt(ids, keys)
    assert torch.equal(one.values(), plain.values()) and torch.equal(one.lengths(), plain.lengths())
    with pytest.raises(ValueError):
        tt.concat_kjt(k, tt.build_bag_kjt(["a", "c"], bags=[[[1], [2]]]))
    with pytest.raises(ValueError):
        tt.build_bag_kjt(keys, bags=[[[1]]])
    with pytest.raises(ValueError):
        tt.build_bag_kjt(keys, values=torch.zeros(3, dtype=torch.long), lengths=torch.ones(3, dtype=torch.long))


def test_synthetic_ragged_bags():
    """synthetic.make_batch(bag_keys=...): the named keys become ragged bags that keep the plain batch's id in front; the other
    keys, the dense features and the plain batch itself are as without the option."""
    from jodalrob_twotower_amd import synthetic
    vn, vc, kn, kc, B = [12, 40, 7], [9, 5], ["a", "b", "c"], ["d", "e"], 33
    plain = synthetic.make_batch(B, vn, vc, kn, kc, 3, 2, "cpu", seed=5)
    bags = synthetic.make_batch(B, vn, vc, kn, kc, 3, 2, "cpu", seed=5, bag_keys={"b", "e"}, mean_bag_length=3.0)
    again = synthetic.make_batch(B, vn, vc, kn, kc, 3, 2, "cpu", seed=5, bag_keys={"b", "e"}, mean_bag_length=3.0)
    for side, keys, vocabs in (("notice", kn, vn), ("company", kc, vc)):
        K = len(keys)
        k, p = bags[side]["kjt"], plain[side]["kjt"]
        assert torch.equal(bags[side]["dense"], plain[side]["dense"]) and torch.equal(p.lengths(), torch.ones(B * K, dtype=torch.long))
        assert torch.equal(k.values(), again[side]["kjt"].values()) and torch.equal(k.lengths(), again[side]["kjt"].lengths())
        L = k.lengths().view(B, K)
        assert int(k.lengths().sum()) == k.values().numel()
        chosen = [key in ("b", "e") for key in keys]
        for j in range(K):
            if not chosen[j]:
                assert bool((L[:, j] == 1).all())
        assert bool((L[:, chosen.index(True)] == 0).any()) and int(L[:, chosen.index(True)].max()) > 3
        off = torch.cumsum(k.lengths(), 0) - k.lengths()
        has = k.lengths() > 0
        assert torch.equal(k.values()[off[has]], p.values()[has])                  # the entity's own id leads its bag
        v = torch.tensor(vocabs)[torch.repeat_interleave(torch.arange(B * K), k.lengths()) % K]
        assert bool((k.values() >= 0).all()) and bool((k.values() < v).all())


def test_c_abi_declares_and_binds_the_bag_entries():
    header = (ROOT / "include" / "twotower.h").read_text()
    assert re.search(r"#define TT_ABI_VERSION 2\b", header)
    lib = _lib.load()
    assert lib.tt_abi_version() == 2
    for name in ("tt_embed_bag_fwd", "tt_embed_bag_grad_bwd", "tt_embed_bag_grad_workspace_bytes"):
        assert re.search(rf"^\s*(?:int|size_t)\s+{name}\s*\(", header, flags=re.M), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert re.search(r"#define TT_DEVERR_BAG_OFFSETS 8u", header) and _lib.TT_DEVERR_BAG_OFFSETS == 8
    assert lib.tt_embed_bag_grad_workspace_bytes(1000, 32) == lib.tt_embed_grad_workspace_bytes(1000, 32) > 0
    # the ctypes side struct has the C layout: 6 pointers, two int64, two int32
    import ctypes
    assert ctypes.sizeof(_lib.BagSide) == 6 * 8 + 2 * 8 + 2 * 4
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct tt_bag_side \{(.*?)\} tt_bag_side;", header, flags=re.S).group(1), flags=re.S)
    assert re.findall(r"(\w+);", body) == [f[0] for f in _lib.BagSide._fields_]


def test_pooling_none_leaves_the_embedder_interface_as_it_was(schema_syn):
    from jodalrob_twotower_amd.cat_embed import CategoricalEmbedder
    names = list(inspect.signature(CategoricalEmbedder.__init__).parameters)
    assert names == ["self", "keys", "metadata_path", "table_name", "embedding_dim", "device", "safety_margin", "embedding_grad",
                     "materialize", "pooling"]
    p = inspect.signature(CategoricalEmbedder.__init__).parameters
    assert (p["embedding_dim"].default, p["device"].default, p["safety_margin"].default, p["embedding_grad"].default,
            p["materialize"].default, p["pooling"].default) == (64, "cuda:0", 10, None, True, None)
    kc = schema_syn["company"]["categorical"]
    meta = str(GOLD / "synthetic_metadata.csv")
    plain = CategoricalEmbedder(kc, meta, "company", embedding_dim=4, device="cpu")
    assert plain.pooling is None and not plain.bag_mode and not hasattr(plain, "_key_pool")
    bag = CategoricalEmbedder(kc, meta, "company", embedding_dim=4, device="cpu", pooling={kc[0]: "mean"})
    assert bag.bag_mode and bag.pooling == ["mean"] + ["sum"] * (len(kc) - 1) and bag._key_pool.tolist() == [1] + [0] * (len(kc) - 1)
    assert list(bag.state_dict()) == list(plain.state_dict())                      # no new persistent state
    for bad in ("max", {"nope": "sum"}, {kc[0]: "max"}, 3):
        with pytest.raises((ValueError, TypeError)):
            CategoricalEmbedder(kc, meta, "company", embedding_dim=4, device="cpu", pooling=bad)
    # the factories pass categorical_pooling through, per tower
    task = tt.create_two_tower_train_task(schema_syn["notice"]["categorical"], kc, metadata_path=meta, categorical_embedding_dim=4,
                                          notice_dense_input_dim=3, company_dense_input_dim=2, tower_hidden_dims=[8, 4],
                                          final_embedding_dim=4, device="cpu", categorical_pooling={"company": "mean"})
    m = task.two_tower_model
    assert not m.notice_tower.categorical_embedder.bag_mode and m.company_tower.categorical_embedder.pooling == ["mean"] * len(kc)
    for f in (tt.create_two_tower_model, tt.create_two_tower_train_task, tt.BaseTower.__init__, tt.NoticeTower.__init__, tt.CompanyTower.__init__):
        sig = inspect.signature(f).parameters
        assert list(sig)[-1] == "categorical_pooling" and sig["categorical_pooling"].default is None


def test_refusals_name_bag_mode_without_a_gpu(schema_syn):
    from jodalrob_twotower_amd.cat_embed import refuse_bag_mode
    kn, kc = schema_syn["notice"]["categorical"], schema_syn["company"]["categorical"]
    meta = str(GOLD / "synthetic_metadata.csv")
    mk = lambda pool: tt.create_two_tower_train_task(kn, kc, metadata_path=meta, categorical_embedding_dim=4, notice_dense_input_dim=3,
                                                     company_dense_input_dim=2, tower_hidden_dims=[8, 4], final_embedding_dim=4,
                                                     device="cpu", categorical_pooling=pool)
    refuse_bag_mode(mk(None), "x")                                                  # a plain model passes
    with pytest.raises(ValueError, match="bag mode.*company_tower"):
        refuse_bag_mode(mk({"company": "sum"}), "GraphedTrainStep")


def test_sharded_paths_and_unaligned_shapes_refuse_bag_mode(schema_syn):
    """The sharded exchange step refuses a bag-mode model when it is built, and a bag-mode tower refuses an exchange in its
    forward (both before anything touches a device); shapes the pooled lookup's 16-byte pieces cannot serve are refused when the
    embedder / tower is built, not at the first step."""
    from jodalrob_twotower_amd.cat_embed import CategoricalEmbedder
    from jodalrob_twotower_amd.distributed import DistributedTwoTowerTrainTask
    kn, kc = schema_syn["notice"]["categorical"], schema_syn["company"]["categorical"]
    meta = str(GOLD / "synthetic_metadata.csv")
    mk = lambda **kw: tt.create_two_tower_model(kn, kc, metadata_path=meta, notice_dense_input_dim=3, company_dense_input_dim=2,
                                                final_embedding_dim=4, device="cpu",
                                                **{"categorical_embedding_dim": 4, "tower_hidden_dims": [8, 4], **kw})
    model = mk(categorical_pooling={"company": "mean"})
    with pytest.raises(ValueError, match=r"sharded exchange step \(DistributedTwoTowerTrainTask\) does not support bag mode.*company_tower"):
        DistributedTwoTowerTrainTask(model, None)
    tower = model.company_tower
    tower.exchange = object()
    B, K = 3, len(kc)
    kjt = tt.build_bag_kjt(kc, values=torch.zeros(2 * B * K, dtype=torch.long), lengths=torch.full((B * K,), 2))
    with pytest.raises(ValueError, match="bag mode.*sharded table exchange"):
        tower({"dense": torch.zeros(B, 2), "kjt": kjt})
    tower.exchange = None
    with pytest.raises(ValueError, match=r"bag mode: the kjt must carry B\*K"):
        tower({"dense": torch.zeros(B + 1, 2), "kjt": kjt})
    for E in (6, 2, 260):
        with pytest.raises(ValueError, match="bag mode.*embedding_dim.*multiple of 4"):
            CategoricalEmbedder(kc, meta, "company", embedding_dim=E, device="cpu", pooling="sum")
    CategoricalEmbedder(kc, meta, "company", embedding_dim=6, device="cpu")                    # the plain path takes any width
    with pytest.raises(ValueError, match=r"bag mode.*tower_hidden_dims\[0\].*multiple of 4"):
        mk(categorical_pooling="mean", tower_hidden_dims=[6, 4])
    mk(tower_hidden_dims=[6, 4])
    # the pooling modes belong to the key directory: they are where it is after the stores were fused
    emb = model.company_tower.categorical_embedder
    assert emb._key_pool.device == emb._key_row_offset.device == emb._key_vocab.device and emb._key_pool.tolist() == [1] * K


def test_exact_grid_inputs_of_the_gpu_tests_keep_sums_exact():
    """The GPU tests' exact cases: every pooled bag and every gradient row keeps its sum of |x| below 2^20 (oracle_np's limit for
    grid values), so the kernels' f32 sums are exact in any order."""
    import test_gpu_embed_bag as G
    for E in G.ES:
        c = G.Case(200 + E, E, G.SUM, G.FWD_LENGTHS)
        assert all(O.exact_sum_precondition(m) for _, m, _, _ in c.reference())
        for pooling, pow2 in ((G.SUM, False), (G.MIXED_EDGE, True)):
            c = G.edge_case(500 + E + pow2, E, pooling, pow2)     # (asserts that the edge key is a mean key with weights < 1)
            d = [O.exact_grid_values(c.rng, (G.B, K * E)) for K in G.KS]
            uniq, sums, abs_sums, counts = c.grad_reference(d)
            assert O.exact_sum_precondition(abs_sums) and abs_sums.max() < 2.0 ** 20
            at = np.searchsorted(uniq, int(c.offs[0][1]) + np.arange(len(G.EDGE_COUNTS)))
            assert counts[at].tolist() == G.EDGE_COUNTS
            if pow2:        # mean weights 2^-k, k <= 7: every product is a multiple of 2^-11 and every sum < 2^13 -- 24 bits hold it
                w = np.concatenate([R.slot_weights(c.lengths[si], c.pooling[si]) for si in range(2)])
                assert set(np.unique(w)) <= {2.0 ** -k for k in range(8)}
