"""Gradients for per-id bag weights and learned position weights: what can be checked without a GPU -- the new C-ABI entries,
the f64 references of tests/_bag_weight_grad_reference.py against torch's float64 autograd, the refusals raised while an
embedder, a tower or the train driver's arguments are built, and the parameter's place in state_dict and among the parameters."""
import ctypes
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import _bag_reference as R
import _bag_weight_grad_reference as G
from conftest import GOLD, ROOT

import jodalrob_twotower_amd as tt
from jodalrob_twotower_amd import _lib
from jodalrob_twotower_amd.cat_embed import CategoricalEmbedder, position_weighted_embedders, refuse_learned_weights

VOCABS = [50, 300, 120]
OFFS = np.array([0, 50, 350], dtype=np.int64)
POOLING = ["mean", "sum", "mean"]
B, K, E = 11, 3, 8
META = str(GOLD / "synthetic_metadata.csv")


def _case(seed):
    rng = np.random.default_rng(seed)
    lengths = rng.choice([0, 1, 2, 3, 5, 9], B * K).astype(np.int64)
    ids = np.concatenate([rng.integers(-3, VOCABS[s % K] + 3, int(n)) for s, n in enumerate(lengths)]).astype(np.int64)
    table = rng.standard_normal((sum(VOCABS), E))
    d_out = rng.standard_normal((B, K * E))
    return rng, lengths, ids, table, d_out


def test_symbols_in_header_and_library():
    header = (ROOT / "include" / "twotower.h").read_text()
    lib = _lib.load()
    for name in ("tt_embed_bag_weight_grad", "tt_bag_position_weights_fwd", "tt_bag_position_weights_bwd"):
        assert re.search(rf"^\s*int\s+{name}\s*\(", header, flags=re.M), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert re.search(r"#define TT_ABI_VERSION 2\b", header)                        # entries were added, none changed
    assert _lib.SIGNATURES["tt_bag_position_weights_fwd"] == _lib.SIGNATURES["tt_bag_position_weights_bwd"]
    # the ctypes side struct has the C layout
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct tt_bag_pw_side \{(.*?)\} tt_bag_pw_side;", header, flags=re.S).group(1), flags=re.S)
    assert re.findall(r"(\w+);", body) == [f[0] for f in _lib.BagPwSide._fields_]
    assert ctypes.sizeof(_lib.BagPwSide) == 4 * 8 + 8 + 2 * 4


@pytest.mark.parametrize("seed", range(3))
def test_weight_gradient_reference_is_float64_autograd(seed):
    """g = d(sum(d_out * pooled)) / dw with pooled = sum_P w_P * row_P (mean: / L) and w a leaf -- at any w: it is no factor"""
    rng, lengths, ids, table, d_out = _case(seed)
    slots, rows = R.positions(ids, lengths, OFFS, VOCABS)
    w = torch.from_numpy(rng.uniform(-2, 2, slots.size)).requires_grad_(True)
    x = torch.from_numpy(table)[torch.from_numpy(rows)] * w[:, None]
    pooled = torch.zeros(B * K, E, dtype=torch.float64).index_add(0, torch.from_numpy(slots), x)
    mean = np.tile(np.array([p == "mean" for p in POOLING]), B)
    pooled = pooled / torch.from_numpy(np.where(mean, np.maximum(lengths, 1), 1).astype(np.float64))[:, None]
    (pooled.reshape(B, K * E) * torch.from_numpy(d_out)).sum().backward()
    g, mag = G.weight_grad(table, d_out, ids, lengths, OFFS, VOCABS, POOLING)
    np.testing.assert_allclose(g, w.grad.numpy(), rtol=1e-12, atol=1e-300)
    assert g.shape == mag.shape == (int(lengths.sum()),) and (np.abs(g) <= mag * (1 + 1e-12)).all() and np.abs(g).max() > 0.1
    # inv_len given: the f32 values instead of the exact 1 / L
    inv = np.where(mean & (lengths > 0), np.float32(1) / np.maximum(lengths, 1).astype(np.float32), np.float32(1))
    g32, _ = G.weight_grad(table, d_out, ids, lengths, OFFS, VOCABS, POOLING, inv_len=inv)
    np.testing.assert_allclose(g32, g, rtol=2.0 ** -23)
    assert not np.array_equal(g32, g)                                              # (lengths 3, 5, 9: 1 / L rounds)


@pytest.mark.parametrize("seed", range(3))
def test_position_weight_references_are_indexing_and_its_autograd(seed):
    rng, lengths, _, _, _ = _case(seed)
    pw_offset, pw_len = [0, -1, 4], [4, 0, 2]                                       # key 1 has none; bags of 5 and 9 pass both max_len
    idx = G.position_index(lengths, K, pw_offset, pw_len)
    assert idx.size == lengths.sum() and idx.max() == 5 and (idx[np.repeat(np.arange(B * K) % K, lengths) == 1] == -1).all()
    starts = np.concatenate([[0], np.cumsum(lengths)])
    for s in range(B * K):                                                         # the definition, position by position
        for j in range(int(lengths[s])):
            k = s % K
            assert idx[starts[s] + j] == (-1 if pw_offset[k] < 0 else pw_offset[k] + min(j, pw_len[k] - 1))
    param = torch.from_numpy(rng.standard_normal(6)).requires_grad_(True)
    g = rng.standard_normal(idx.size)
    live = torch.from_numpy(idx >= 0)
    w = torch.where(live, param[torch.from_numpy(np.maximum(idx, 0))], torch.ones((), dtype=torch.float64))
    assert np.array_equal(w.detach().numpy(), G.expand(param.detach().numpy(), idx))
    (w * torch.from_numpy(g)).sum().backward()
    total, mag, cnt = G.reduce(g, idx, 6)
    np.testing.assert_allclose(total, param.grad.numpy(), rtol=1e-12, atol=1e-300)
    assert cnt.sum() == (idx >= 0).sum() and (np.abs(total) <= mag * (1 + 1e-12)).all()
    f32 = np.arange(6, dtype=np.float32)
    assert G.expand(f32, idx).dtype == np.float32                                  # a copy: the dtype (and the bits) kept


def test_embedder_refusals_and_parameter(schema_syn):
    kc = schema_syn["company"]["categorical"]
    mk = lambda **kw: CategoricalEmbedder(kc, META, "company", embedding_dim=4, device="cpu", **kw)
    with pytest.raises(ValueError, match="need bag mode.*without pooling"):
        mk().add_position_weights({kc[0]: 3})
    for bad, what in (({"nope": 3}, "does not have"), ({kc[0]: 0}, "max_len"), ({kc[0]: -2}, "max_len"), ({kc[0]: 2.5}, "max_len"),
                      ({kc[0]: True}, "max_len"), ({}, "non-empty"), ([kc[0]], "non-empty")):
        with pytest.raises(ValueError, match=what):
            mk(pooling="sum").add_position_weights(bad)
    plain = mk(pooling="sum")
    assert plain.position_weights is None and "position_weight" not in plain.state_dict() and not position_weighted_embedders(plain)
    emb = mk(pooling={kc[0]: "mean"}).add_position_weights({kc[-1]: 3, kc[0]: 5})
    with pytest.raises(ValueError, match="already has position weights"):
        emb.add_position_weights({kc[0]: 2})
    p = emb.position_weight
    assert isinstance(p, torch.nn.Parameter) and p.shape == (8,) and p.dtype == torch.float32 and bool((p == 1).all()) and p.requires_grad
    assert emb._pw_offset.tolist() == [0] + [-1] * (len(kc) - 2) + [5] and emb._pw_len.tolist() == [5] + [0] * (len(kc) - 2) + [3]
    assert emb._pw_offset.dtype == emb._pw_len.dtype == torch.int32
    assert dict(emb.named_parameters())["position_weight"] is p and all(p is not t for t in emb.table_parameters())
    assert list(emb.state_dict()) == ["position_weight"] + list(plain.state_dict())      # persistent; the key directory is not
    # a state_dict round trip restores it; moving the module keeps the Parameter's identity
    with torch.no_grad():
        p.copy_(torch.arange(8.0))
    other = mk(pooling={kc[0]: "mean"}).add_position_weights({kc[-1]: 3, kc[0]: 5})
    other.load_state_dict(emb.state_dict())
    assert torch.equal(other.position_weight, p) and other.position_weight is not p
    assert emb.to("cpu").position_weight is p and emb._pw_offset.device == p.device
    with pytest.raises(TypeError, match="float32"):                                # as the tables: the kernels read f32
        emb.double()
    # one source of weights per embedder: a KJT with data weights is refused before any lookup
    n = 2 * len(kc)
    kjt = tt.build_bag_kjt(kc, values=torch.zeros(n, dtype=torch.long), lengths=torch.ones(n, dtype=torch.long), weights=torch.ones(n))
    with pytest.raises(ValueError, match="one source of weights per embedder"):
        emb(kjt)
    with pytest.raises(ValueError, match="one source of weights per embedder"):
        emb.bag_weights(kjt)
    assert plain.bag_weights(kjt) is kjt.weights()                                 # without position weights: the KJT's own, as before


def test_towers_and_factories_take_position_weights(schema_syn):
    import inspect
    kn, kc = schema_syn["notice"]["categorical"], schema_syn["company"]["categorical"]
    mk = lambda **kw: tt.create_two_tower_train_task(kn, kc, metadata_path=META, categorical_embedding_dim=4, notice_dense_input_dim=3,
                                                     company_dense_input_dim=2, tower_hidden_dims=[8, 4], final_embedding_dim=4,
                                                     device="cpu", **kw)
    for f in (tt.create_two_tower_model, tt.create_two_tower_train_task, tt.BaseTower.__init__, tt.NoticeTower.__init__, tt.CompanyTower.__init__):
        assert inspect.signature(f).parameters["categorical_position_weights"].default is None
    task = mk(categorical_pooling={kc[0]: "mean", kn[1]: "sum"}, categorical_position_weights={kc[0]: 4, kn[1]: 2, kn[0]: 3})
    m = task.two_tower_model
    assert m.company_tower.categorical_embedder.position_weights == {kc[0]: 4}
    assert m.notice_tower.categorical_embedder.position_weights == {kn[0]: 3, kn[1]: 2}      # every key of a bag-mode embedder pools
    names = [n for n, _ in task.named_parameters() if n.endswith("position_weight")]
    assert names == ["two_tower_model.notice_tower.categorical_embedder.position_weight",
                     "two_tower_model.company_tower.categorical_embedder.position_weight"]
    assert set(names) <= set(task.state_dict())
    assert position_weighted_embedders(task) == [n.rsplit(".", 1)[0] for n in names]
    per_tower = mk(categorical_pooling="sum", categorical_position_weights={"company": {kc[1]: 2}})
    assert per_tower.two_tower_model.notice_tower.categorical_embedder.position_weights is None
    assert per_tower.two_tower_model.company_tower.categorical_embedder.position_weights == {kc[1]: 2}
    # refused while the model is built: no pooling at all, a key of a tower that does not pool, unknown keys, max_len < 1
    with pytest.raises(ValueError, match="need bag mode"):
        mk(categorical_position_weights={kc[0]: 4})
    with pytest.raises(ValueError, match="need bag mode"):
        mk(categorical_pooling={"company": "sum"}, categorical_position_weights={kn[0]: 4})
    with pytest.raises(ValueError, match="neither tower has"):
        mk(categorical_pooling="sum", categorical_position_weights={"nope": 4})
    with pytest.raises(ValueError, match="max_len"):
        mk(categorical_pooling="sum", categorical_position_weights={kc[0]: 0})
    # the captured steps' refusal, as a function: position weights, and example weights that require grad
    with pytest.raises(ValueError, match="GraphedTrainStep does not support learned position weights.*company_tower.*eager step"):
        refuse_learned_weights(per_tower, "GraphedTrainStep")
    plain = mk(categorical_pooling="sum")
    n = 2 * len(kc)
    w = torch.ones(n, requires_grad=True)
    kjt = tt.build_bag_kjt(kc, values=torch.zeros(n, dtype=torch.long), lengths=torch.ones(n, dtype=torch.long), weights=w)
    assert kjt.weights().requires_grad
    with pytest.raises(ValueError, match="weights that require grad.*eager step"):
        refuse_learned_weights(plain, "GraphedTrainStep", [None, kjt])
    data = tt.build_bag_kjt(kc, values=torch.zeros(n, dtype=torch.long), lengths=torch.ones(n, dtype=torch.long), weights=w.detach())
    refuse_learned_weights(plain, "GraphedTrainStep", [None, data])                # data weights pass, as before


def test_train_driver_refuses_position_weights_beside_other_weights_and_captured_steps():
    base = [sys.executable, str(ROOT / "scripts" / "train.py"), "--pool-position-weights", "4"]
    pool = ["--pool", "rgncd=mean"]
    for extra, what in ((["--pool-weights"], "not with --pool-weights"), (["--pool-capture"], "not with --pool-capture"),
                        (["--pool-store", "--fast"], "not with --pool-store --fast")):
        r = subprocess.run(base + pool + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 2 and f"--pool-position-weights: {what}" in r.stderr, (extra, r.stderr[-400:])
    r = subprocess.run(base, capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "--pool-position-weights needs --pool" in r.stderr
