"""Bag mode (pooled multi-valued categorical features) through the Python layers on the MI355X: the stand-alone embedder, the
towers inside the eager training step, extra negatives, and the paths that refuse it.  B = 64, the small synthetic schema
(manifest case wide_b40: 5 + 2 keys, E = 16, towers [32, 24] -> 16), fp32 modes.

The equivalence tests feed a bag-mode company tower (mean pooling) bags that are one id or the same id twice: (x + x) / 2 = x
exactly, so the pooled input equals the plain lookup's bit for bit and so does everything the towers and the loss compute from it
(loss, tower outputs, dense-parameter gradients).  The table gradients re-associate -- a doubled id contributes d/2 + d/2 where
the plain step contributes d -- and agree norm-wise within RANDN_NORM_BOUND, the bar of tests/test_gpu_embed_grad_parity.py.

Bounds of the stand-alone embedder: tests/test_gpu_embed_bag.py's (its docstring derives them); the mean keys' bags have
power-of-two lengths so that the weights 1 / L are exact in f32, as the backward bound needs.
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _bag_reference as R
from conftest import GOLD
from test_gpu_parity import DEV, tt, make_task, to_batch, load_state  # noqa: F401
from test_gpu_embed_bag import RANDN_NORM_BOUND, U24

pytestmark = pytest.mark.gpu

B = 64


def _cfg(manifest):
    return dict(manifest["cases"]["wide_b40"], B=B)


# ------------------------------------------------------------------------------------------- 1: stand-alone embedder
def _embedder(cfg, grad_mode, pooling, state=None):
    from jodalrob_twotower_amd.cat_embed import CategoricalEmbedder
    emb = CategoricalEmbedder(cfg["keys_n"], str(GOLD / "synthetic_metadata.csv"), "notice", embedding_dim=cfg["E"], device=DEV,
                              embedding_grad=grad_mode, pooling=pooling)
    if state is not None:
        emb.load_state_dict(state)
    return emb


@pytest.mark.parametrize("mean_lengths", [[0, 1, 2, 4, 8], [0, 1, 2, 3, 5, 7, 11]], ids=["mean-pow2", "mean-ragged"])
def test_standalone_embedder_matches_f64_embedding_bag(tt, manifest, mean_lengths):
    """mean-pow2: the mean keys' weights 1 / L are exact, the backward bound is gamma_(n-1).  mean-ragged: the ordinary case --
    lengths of any size, so the weights are fl(1 / L) as ops.embed_bag_lookup forms them on the device (one correctly rounded
    f32 division, formed here the same way) and every contribution rounds once: gamma_n against the f64 sum over those weights
    (tests/test_gpu_embed_bag.py derives both).  The forward bound holds for any length."""
    exact_w = all(L & (L - 1) == 0 for L in mean_lengths)
    cfg = _cfg(manifest)
    keys, E = cfg["keys_n"], cfg["E"]
    K = len(keys)
    pooling = {keys[0]: "mean", keys[2]: "mean", keys[4]: "sum"}                   # the keys left out sum
    dense = _embedder(cfg, "dense", pooling)
    modes = dense.pooling
    assert modes == ["mean", "sum", "mean", "sum", "sum"]
    vocabs = [dense.vocab_sizes[k] for k in keys]
    offs = dense._key_row_offset.cpu().numpy()
    rng = np.random.default_rng(12)
    lengths = np.stack([rng.choice(mean_lengths if m == "mean" else [0, 1, 2, 3, 5, 7], B) for m in modes], axis=1).reshape(-1)
    ids = np.concatenate([rng.integers(-2, vocabs[s % K] + 2, int(L)) for s, L in enumerate(lengths)]).astype(np.int64)
    kjt = tt.build_bag_kjt(keys, values=torch.from_numpy(ids), lengths=torch.from_numpy(lengths), device=DEV)
    g = rng.standard_normal((B, K * E)).astype(np.float32)
    gt = torch.from_numpy(g).to(DEV)
    out = dense(kjt, return_dict=False)
    (out * gt).sum().backward()
    table = dense.store.weight.detach().cpu().numpy()
    ref, mag, _, _ = R.bag_forward(table, ids, lengths, offs, vocabs, modes)
    # the f64 reference IS torch's embedding_bag, key by key
    starts = np.concatenate([[0], np.cumsum(lengths)])
    for k in range(K):
        sel = np.arange(B) * K + k
        kid = np.concatenate([ids[starts[s]:starts[s + 1]] for s in sel]).clip(0, vocabs[k] - 1)
        koff = np.concatenate([[0], np.cumsum(lengths[sel])[:-1]])
        w = torch.from_numpy(table[offs[k]:offs[k] + vocabs[k]].astype(np.float64))
        eb = torch.nn.functional.embedding_bag(torch.from_numpy(kid), w, torch.from_numpy(koff), mode=modes[k]).numpy()
        np.testing.assert_allclose(ref[:, k * E:(k + 1) * E], eb, rtol=1e-13, atol=1e-14)
    L = np.repeat(lengths.reshape(B, K), E, axis=1).astype(np.float64)
    err = np.abs(out.detach().cpu().numpy().astype(np.float64) - ref)
    assert (err <= L * U24 * mag).all()                                            # the forward bound
    d = dense(kjt)                                                                 # the dict form: the same columns
    assert all(torch.equal(d[k], out[:, i * E:(i + 1) * E]) for i, k in enumerate(keys))
    w32 = np.where(np.tile(np.array([m == "mean" for m in modes]), B) & (lengths > 0),
                   np.float32(1) / np.maximum(lengths, 1).astype(np.float32), np.float32(1))
    if exact_w:
        assert np.array_equal(w32.astype(np.float64), R.slot_weights(lengths, modes))
    uniq, sums, abs_sums, counts = R.bag_backward(g, ids, lengths, offs, vocabs, modes, weights=w32)
    ku = np.maximum(counts - (1 if exact_w else 0), 0)[:, None] * U24
    got = dense.store.grad.cpu().numpy()
    assert (np.abs(got[uniq].astype(np.float64) - sums) <= ku / (1 - ku) * abs_sums).all()      # the backward bound
    rest = np.ones(len(got), bool)
    rest[uniq] = False
    assert not got[rest].any()
    for k in keys:                                                                 # dense .grad views, as the plain path binds them
        p = dense.embeddings[k].weight
        assert p.grad is not None and p.grad.data_ptr() == dense.store.grad[dense._key_row_offset[keys.index(k)]:].data_ptr()
    # sparse mode files (plan, grad_rows) that reproduce the dense gradient's non-zero rows bit for bit
    sparse = _embedder(cfg, "sparse", pooling, dense.state_dict())
    (sparse(kjt, return_dict=False) * gt).sum().backward()
    plan, grad_rows = sparse.store.sparse_grad
    U = int(plan.n_unique.item())
    assert plan.M == len(ids) and np.array_equal(plan.unique_rows[:U].cpu().numpy(), uniq)
    assert np.array_equal(grad_rows[:U].cpu().numpy().view(np.uint32), got[uniq].view(np.uint32))
    assert got[uniq].any(1).all()


# ------------------------------------------------------------------------------------------- 2, 3: the eager step
def _tasks(tt, manifest, **kw):
    """(plain task, bag task with a mean-pooling company tower) on the same weights, dropout 0, sparse tables; the batch"""
    from params_init import init_state_numpy, synth_batch_numpy
    cfg = _cfg(manifest)
    tasks = []
    for pool in (None, {"company": "mean"}):
        task = make_task(tt, cfg, embedding_grad="sparse", mlp_dtype="fp32", score_dtype="fp32", categorical_pooling=pool, **kw)
        load_state(task, init_state_numpy({k: tuple(v.shape) for k, v in task.state_dict().items()}, 77))
        task.train()
        task._pair_check_done = True
        tasks.append(task)
    nb = synth_batch_numpy(B, cfg["vocab_n"], cfg["vocab_c"], cfg["din_n"], cfg["din_c"], 610, oob=False)
    return tasks[0], tasks[1], to_batch(tt, nb, cfg["keys_n"], cfg["keys_c"]), cfg


def _doubled(tt, kjt, seed):
    """the same bags as the length-one `kjt`, every other one (at random) holding its id twice"""
    g = torch.Generator().manual_seed(seed)
    v = kjt.values().cpu()
    lengths = torch.randint(1, 3, (v.numel(),), generator=g)
    assert bool((lengths == 1).any()) and bool((lengths == 2).any())
    return tt.build_bag_kjt(list(kjt.keys()), values=torch.repeat_interleave(v, lengths), lengths=lengths, device=DEV)


def _table_grad(task):
    """the pending sparse gradients as one dense [R, E] array, and the rows they touch"""
    store = task.two_tower_model.embedding_store
    g = np.zeros((store.rows, store.E), np.float32)
    touched = np.zeros(store.rows, bool)
    for plan, rows in store.sparse_grads():
        U = int(plan.n_unique.item())
        u = plan.unique_rows[:U].cpu().numpy()
        assert not touched[u].any()
        g[u] = rows[:U].cpu().numpy()
        touched[u] = True
    return g, touched


def _step(task, batch):
    task.zero_grad(set_to_none=True)
    res = task(batch, return_metrics=True)
    res["loss"].backward()
    torch.cuda.synchronize()
    dense = {k: p.grad.clone() for k, p in task.named_parameters() if p.grad is not None and "embeddings." not in k}
    return res, dense


def _compare_steps(plain, bag, b_plain, b_bag, company_rows):
    from jodalrob_twotower_amd.optim import FusedAdam
    rp, dp = _step(plain, b_plain)
    rb, db = _step(bag, b_bag)
    assert torch.equal(rp["loss"], rb["loss"])                                     # bit for bit
    for k in ("notice_embeddings", "company_embeddings"):
        if k in rp:
            assert torch.equal(rp[k], rb[k]), k
    assert dp.keys() == db.keys() and len(dp) >= 12
    for k in dp:
        assert torch.equal(dp[k], db[k]), k
    gp, tp = _table_grad(plain)
    gb, tb = _table_grad(bag)
    assert np.array_equal(tp, tb)
    assert np.array_equal(gp[~company_rows].view(np.uint32), gb[~company_rows].view(np.uint32))        # the plain side: bit for bit
    norm = float(np.linalg.norm(gp.astype(np.float64) - gb) / np.linalg.norm(gp.astype(np.float64)))
    print(f"\n[embed_bag step] table gradient: norm-wise {norm:.3e}")
    assert norm <= RANDN_NORM_BOUND
    # one FusedAdam step (sparse tables, Adam)
    before = plain.two_tower_model.embedding_store.weight.detach().cpu().numpy().copy()
    for task in (plain, bag):
        FusedAdam.for_task(task, lr=1e-2).step()
    torch.cuda.synchronize()
    wp = plain.two_tower_model.embedding_store.weight.detach().cpu().numpy()
    wb = bag.two_tower_model.embedding_store.weight.detach().cpu().numpy()
    assert np.array_equal(wp[~tp].view(np.uint32), before[~tp].view(np.uint32)) and np.array_equal(wb[~tp].view(np.uint32), before[~tp].view(np.uint32))
    assert not np.array_equal(wp[tp], before[tp])
    wnorm = float(np.linalg.norm(wp.astype(np.float64) - wb) / np.linalg.norm(wp.astype(np.float64)))
    print(f"[embed_bag step] tables after one Adam step: norm-wise {wnorm:.3e}")
    assert wnorm <= RANDN_NORM_BOUND
    for (k, a), (_, c) in zip(plain.named_parameters(), bag.named_parameters()):
        if "embeddings." not in k:
            assert torch.equal(a, c), k                                            # the towers stepped on identical gradients


def _company_rows(task):
    emb = task.two_tower_model.company_tower.categorical_embedder
    rows = np.zeros(task.two_tower_model.embedding_store.rows, bool)
    rows[emb.row_base:emb.row_base + emb.total_rows] = True
    return rows


def _forward_outputs(task, batch):
    with torch.no_grad():
        n, c = task.two_tower_model(batch["notice"], batch["company"])
    return n.clone(), c.clone()


def test_mean_pooled_company_tower_equals_the_plain_step(tt, manifest):
    plain, bag, b, cfg = _tasks(tt, manifest)
    assert bag.two_tower_model.company_tower.categorical_embedder.bag_mode and not bag.two_tower_model.notice_tower.categorical_embedder.bag_mode
    bb = {"notice": b["notice"], "company": dict(b["company"], kjt=_doubled(tt, b["company"]["kjt"], 5))}
    for t in (plain, bag):
        t.eval()
    (np_, cp), (nb_, cb) = _forward_outputs(plain, b), _forward_outputs(bag, bb)
    assert torch.equal(np_, nb_) and torch.equal(cp, cb)                          # tower outputs, bit for bit
    for t in (plain, bag):
        t.train()
    _compare_steps(plain, bag, b, bb, _company_rows(plain))


def test_extra_negatives_with_a_bag_mode_company_tower(tt, manifest):
    from jodalrob_twotower_amd.kjt import KeyedJaggedTensor
    plain, bag, b, cfg = _tasks(tt, manifest)
    M, K = 9, len(cfg["keys_c"])
    g = torch.Generator(device=DEV).manual_seed(3)
    pick = torch.randint(0, B, (M,), generator=g, device=DEV)
    neg_ids = b["company"]["kjt"].values().view(B, K)[pick].reshape(-1)
    neg = {"dense": b["company"]["dense"][pick] + 0.25, "kjt": KeyedJaggedTensor(cfg["keys_c"], neg_ids)}
    b_plain = dict(b, negatives=neg)
    b_bag = {"notice": b["notice"], "company": dict(b["company"], kjt=_doubled(tt, b["company"]["kjt"], 6)),
             "negatives": dict(neg, kjt=_doubled(tt, neg["kjt"], 7))}
    with torch.no_grad():
        assert float(plain(b_plain)) != float(plain(b))                            # the extras take part
    _compare_steps(plain, bag, b_plain, b_bag, _company_rows(plain))


# ------------------------------------------------------------------------------------------- 4: refusals
def test_static_id_buffer_paths_refuse_bag_mode(tt, manifest):
    from jodalrob_twotower_amd.data_loader import DeviceFeatureStore, DevicePairLoader
    from jodalrob_twotower_amd.graph import GraphedEvalStep, GraphedTrainStep
    from jodalrob_twotower_amd.optim import FusedAdam
    from jodalrob_twotower_amd.segmented import SegmentedTrainStep
    from jodalrob_twotower_amd.unrolled import UnrolledTrainStep
    plain, bag, b, cfg = _tasks(tt, manifest)
    opt = FusedAdam.for_task(bag, lr=1e-2)
    for cls in (GraphedTrainStep, UnrolledTrainStep, SegmentedTrainStep):
        with pytest.raises(ValueError, match=rf"{cls.__name__} does not support bag mode"):
            cls(bag, opt, b)
    with pytest.raises(ValueError, match="GraphedEvalStep does not support bag mode"):
        GraphedEvalStep(bag, b)
    stores = [DeviceFeatureStore({"dense_projected": b[s]["dense"], "categorical": b[s]["kjt"].values().view(B, -1)}, cfg[f"keys_{s[0]}"], DEV)
              for s in ("notice", "company")]
    loader = DevicePairLoader(stores[0], stores[1], np.stack([np.arange(B), np.arange(B)], axis=1), 16, shuffle=False)
    fake = SimpleNamespace(task=bag)                                               # (no captured step of a bag-mode task can exist)
    with pytest.raises(ValueError, match="DevicePairLoader.step_batches does not support bag mode"):
        next(loader.step_batches(fake))
    with pytest.raises(ValueError, match="DevicePairLoader.eval_batches does not support bag mode"):
        loader.eval_batches(fake)
    assert torch.isfinite(bag(next(iter(loader))))                                 # its plain batches still train eagerly: bags of one id
    # the evaluator captures its pass where it can: for a bag-mode model it falls back to the batch-by-batch loop instead
    ev = tt.TwoTowerEvaluator(device=DEV)
    m = ev.evaluate_comprehensive(bag, loader, verbose=False)
    assert m["num_batches"] == 4 and np.isfinite(m["loss"]) and not ev.__dict__.get("_eval_graphs")
    ev.close()


def test_pooling_none_ignores_lengths_as_before(tt, manifest):
    plain, bag, b, cfg = _tasks(tt, manifest)
    want = plain(b)
    kjt = b["company"]["kjt"]
    odd = tt.KeyedJaggedTensor(kjt.keys(), kjt.values(), torch.full_like(kjt.values(), 3))      # non-unit lengths, B*K ids
    got = plain({"notice": b["notice"], "company": dict(b["company"], kjt=odd)})
    assert torch.equal(want, got)                                                  # lengths are not looked at
    short = tt.KeyedJaggedTensor(kjt.keys(), kjt.values()[:-1], torch.ones(kjt.values().numel() - 1, dtype=torch.long, device=DEV))
    with pytest.raises(ValueError, match=r"ids but the batch needs B\*K"):         # the towers' B*K check is unchanged
        plain({"notice": b["notice"], "company": dict(b["company"], kjt=short)})
    with pytest.raises(ValueError, match="bag mode: the kjt must carry"):          # bag mode checks the lengths instead
        bag({"notice": b["notice"], "company": dict(b["company"], kjt=short)})
    from jodalrob_twotower_amd.cat_embed import CategoricalEmbedder
    emb = CategoricalEmbedder(cfg["keys_c"], str(GOLD / "synthetic_metadata.csv"), "company", embedding_dim=cfg["E"], device=DEV)
    assert torch.equal(emb(kjt, return_dict=False), emb(odd, return_dict=False))


# ------------------------------------------------------------------------------------------- 5: the driver
def test_train_driver_pools_ragged_bags(tt, tmp_path):
    """scripts/train.py --pool KEY=MODE: a few eager steps on ragged bags of keys of both towers, the evaluation (batch by batch:
    no captured pass for a bag-mode model) and the checkpoints; --pool with --fast is refused by the argument parser."""
    import subprocess
    import sys
    from conftest import ROOT
    base = [sys.executable, str(ROOT / "scripts" / "train.py"), "--results-csv", str(tmp_path / "r.csv"), "--output-dir", str(tmp_path / "m"),
            "--pairs", "3000", "--entities", "600", "--steps", "6", "--pool", "rgncd=mean", "cntrynm=sum", "ntceinsttcd=mean", "--pool-length", "3"]
    r = subprocess.run(base, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "done: 6 steps" in r.stdout and (tmp_path / "m" / "final_model.pt").exists()
    losses = [float(ln.split("Loss:")[1].split(",")[0]) for ln in r.stdout.splitlines() if ln.startswith(("Train -", "Val   -"))]
    assert len(losses) == 2 and all(np.isfinite(losses))
    r = subprocess.run(base + ["--fast"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 2 and "--pool needs the eager loop" in r.stderr
