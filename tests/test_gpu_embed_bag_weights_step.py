"""Weighted bags (a KJT's weights(): one f32 per id) through the Python layers on the MI355X: the stand-alone embedder, the towers
inside the eager training step, extra negatives, and the captured step GraphedTrainStep(bag_capacity=...) with its refusals.

The small synthetic schema of the bag tests (manifest case wide_b40: 5 + 2 keys, E = 16, towers [32, 24] -> 16) at B = 64, dropout
0, fp32 modes, two pooled keys per tower -- one summed, one averaged; the embedders' other keys keep bags of one id.

What is bit for bit and why:
  * weights of 1.0 are the unweighted step: 1 * x = x and fma(1, x, acc) = acc + x in both kernels;
  * under sum pooling an id listed twice is the id once at weight 2.0: x + x = 2 x exactly, in the pooled input and -- for a table
    row that one bag alone touches, which is every row of that test's batch -- in the row's gradient (fma(1, d, fma(1, d, 0)) =
    fma(2, d, 0));
  * the captured step runs the eager step's kernels on the same values in the same order (tests/test_gpu_embed_bag_capture.py).
The stand-alone embedder is held to the derived rounding bounds of tests/test_gpu_embed_bag_weights.py (case 3).
"""
from unittest import mock

import numpy as np
import pytest
import torch

import _bag_weight_reference as W
from conftest import GOLD
from test_gpu_embed_bag import U24
from test_gpu_embed_bag_capture import _assert_same_state, _cfg, _eager, _task
from test_gpu_embed_bag_step import _forward_outputs, _step, _table_grad
from test_gpu_parity import DEV, tt, make_task, to_batch, load_state  # noqa: F401

from jodalrob_twotower_amd import _lib as _L

pytestmark = pytest.mark.gpu

B = 64
F32 = dict(embedding_grad="sparse", mlp_dtype="fp32", score_dtype="fp32")


def gamma(k):
    ku = np.asarray(k, dtype=np.float64) * U24
    return ku / (1 - ku)


def _pool(cfg):
    """two pooled keys per tower: one sum, one mean"""
    return {cfg["keys_n"][3]: "sum", cfg["keys_n"][4]: "mean", cfg["keys_c"][0]: "sum", cfg["keys_c"][1]: "mean"}


def _batch(tt, cfg, mean, seed, weights="uniform", sides=("notice", "company"), n=B):
    """the plain synthetic batch with the pooled keys of `sides` turned into ragged bags of about `mean` ids (weights: None | "uniform" |
    "ones")"""
    from jodalrob_twotower_amd import synthetic
    from params_init import synth_batch_numpy
    b = to_batch(tt, synth_batch_numpy(n, cfg["vocab_n"], cfg["vocab_c"], cfg["din_n"], cfg["din_c"], seed, oob=False), cfg["keys_n"], cfg["keys_c"])
    pool = _pool(cfg)
    for side in sides:
        vocabs = cfg[f"vocab_{side[0]}"]
        kjt = synthetic.ragged_bags(b[side]["kjt"], vocabs, pool, mean, seed=seed + len(side), weights=None if weights is None else "uniform")
        if weights == "ones":
            kjt = tt.KeyedJaggedTensor(kjt.keys(), kjt.values(), kjt.lengths(), torch.ones_like(kjt.weights()))
        b[side] = dict(b[side], kjt=kjt)
    return b


def _without_weights(tt, b):
    out = dict(b)
    for side in ("notice", "company", "negatives"):
        if side in b:
            k = b[side]["kjt"]
            out[side] = dict(b[side], kjt=tt.KeyedJaggedTensor(k.keys(), k.values(), k.lengths()))
    return out


def _adam_step_and_compare(ta, tb):
    from jodalrob_twotower_amd.optim import FusedAdam
    for t in (ta, tb):
        FusedAdam.for_task(t, lr=1e-2).step()
    torch.cuda.synchronize()
    for (k, a), (_, b) in zip(ta.named_parameters(), tb.named_parameters()):
        assert torch.equal(a, b), k
    assert torch.equal(ta.two_tower_model.embedding_store.weight, tb.two_tower_model.embedding_store.weight)


def _compare_steps_bitwise(ta, ba, tb, bb):
    """loss, every dense gradient, the touched table rows and their gradients, the parameters after one optimiser step"""
    ra, da = _step(ta, ba)
    rb, db = _step(tb, bb)
    assert torch.equal(ra["loss"], rb["loss"])
    assert da.keys() == db.keys() and len(da) >= 12
    for k in da:
        assert torch.equal(da[k], db[k]), k
    ga, touched_a = _table_grad(ta)
    gb, touched_b = _table_grad(tb)
    assert np.array_equal(touched_a, touched_b) and touched_a.any()
    assert np.array_equal(ga.view(np.uint32), gb.view(np.uint32))
    _adam_step_and_compare(ta, tb)


# ------------------------------------------------------------------------------------------- the eager step
def test_eager_step_with_ones_is_the_unweighted_step(tt, manifest):
    from jodalrob_twotower_amd import ops
    cfg = _cfg(manifest)
    ta, tb = _task(tt, cfg, _pool(cfg), **F32), _task(tt, cfg, _pool(cfg), **F32)
    bw = _batch(tt, cfg, 3.0, 610, weights="ones")
    assert all(bool((bw[s]["kjt"].weights() == 1).all()) and int(bw[s]["kjt"].lengths().max()) > 2 for s in ("notice", "company"))
    with mock.patch.object(ops, "_bag_weight_args", wraps=ops._bag_weight_args) as spy:
        _compare_steps_bitwise(ta, _without_weights(tt, bw), tb, bw)
    assert spy.call_count >= 1                                                   # the weighted batch took the _w entries


def test_an_id_listed_twice_is_the_id_once_at_weight_two(tt, manifest):
    cfg = dict(_cfg(manifest), B=12)
    n, keys, K = 12, cfg["keys_c"], len(cfg["keys_c"])
    assert min(cfg["vocab_c"]) >= n
    pool = {"company": "sum"}
    ta, tb = _task(tt, cfg, pool, **F32), _task(tt, cfg, pool, **F32)
    base = _batch(tt, cfg, 1.0, 611, weights=None, sides=(), n=n)
    g = torch.Generator().manual_seed(8)
    # every (sample, key) its own id: a table row is touched by one bag alone
    ids = torch.stack([torch.randperm(v, generator=g)[:n] for v in cfg["vocab_c"]], dim=1).reshape(-1)
    twice = torch.randint(0, 2, (n * K,), generator=g).bool()
    assert bool(twice.any()) and not bool(twice.all())
    lengths = torch.where(twice, 2, 1)
    listed = tt.build_bag_kjt(keys, values=torch.repeat_interleave(ids, lengths), lengths=lengths, device=DEV)
    weighted = tt.build_bag_kjt(keys, values=ids, lengths=torch.ones(n * K, dtype=torch.long), device=DEV,
                                weights=torch.where(twice, 2.0, 1.0))
    ba = {"notice": base["notice"], "company": dict(base["company"], kjt=listed)}
    bb = {"notice": base["notice"], "company": dict(base["company"], kjt=weighted)}
    for t in (ta, tb):
        t.eval()
    (na, ca), (nb, cb) = _forward_outputs(ta, ba), _forward_outputs(tb, bb)
    assert torch.equal(na, nb) and torch.equal(ca, cb)                           # the pooled inputs, hence the towers' outputs
    for t in (ta, tb):
        t.train()
    _compare_steps_bitwise(ta, ba, tb, bb)


def test_extra_negatives_ride_along_with_their_weights(tt, manifest):
    """company + negatives go through concat_kjt: weights of 1.0 -- on both, or on the batch's companies alone (the negatives then
    get ones) -- give the unweighted step with the same extras, bit for bit"""
    cfg = _cfg(manifest)
    pool = {"company": "mean"}
    M = 9
    bw = _batch(tt, cfg, 3.0, 612, weights="ones", sides=("company",))
    negs = _batch(tt, cfg, 2.0, 613, weights="ones", sides=("company",), n=M)["company"]
    bw["negatives"] = {"dense": negs["dense"] + 0.25, "kjt": negs["kjt"]}
    plain = _without_weights(tt, bw)
    half = dict(bw, negatives=plain["negatives"])
    for weighted in (bw, half):
        ta, tb = _task(tt, cfg, pool, **F32), _task(tt, cfg, pool, **F32)
        with torch.no_grad():                                                    # the extras take part (both tasks run the same passes)
            assert float(ta(plain)) != float(ta({k: v for k, v in plain.items() if k != "negatives"}))
            assert float(tb(weighted)) != float(tb({k: v for k, v in weighted.items() if k != "negatives"}))
        _compare_steps_bitwise(ta, plain, tb, weighted)


# ------------------------------------------------------------------------------------------- the stand-alone embedder
def test_standalone_embedder_matches_f64_embedding_bag(tt, manifest):
    from jodalrob_twotower_amd.cat_embed import CategoricalEmbedder
    cfg = _cfg(manifest)
    keys, E = cfg["keys_n"], cfg["E"]
    K = len(keys)
    pooling = {keys[0]: "mean", keys[2]: "mean", keys[4]: "sum"}
    emb = CategoricalEmbedder(keys, str(GOLD / "synthetic_metadata.csv"), "notice", embedding_dim=E, device=DEV, embedding_grad="dense",
                              pooling=pooling)
    modes = emb.pooling
    vocabs = [emb.vocab_sizes[k] for k in keys]
    offs = emb._key_row_offset.cpu().numpy()
    rng = np.random.default_rng(14)
    lengths = rng.choice([0, 1, 2, 3, 5, 7, 11], B * K).astype(np.int64)
    ids = np.concatenate([rng.integers(-2, vocabs[s % K] + 2, int(n)) for s, n in enumerate(lengths)]).astype(np.int64)
    w = rng.standard_normal(ids.size).astype(np.float32)
    kjt = tt.build_bag_kjt(keys, values=torch.from_numpy(ids), lengths=torch.from_numpy(lengths), weights=torch.from_numpy(w), device=DEV)
    g = rng.standard_normal((B, K * E)).astype(np.float32)
    out = emb(kjt, return_dict=False)
    (out * torch.from_numpy(g).to(DEV)).sum().backward()
    table = emb.store.weight.detach().cpu().numpy()
    ref, mag, _, _ = W.weighted_forward(table, ids, lengths, offs, vocabs, modes, w)
    # the f64 reference IS torch's embedding_bag(mode="sum", per_sample_weights=), key by key; a mean key: that sum / L
    starts = np.concatenate([[0], np.cumsum(lengths)])
    t64 = torch.from_numpy(table.astype(np.float64)).requires_grad_(True)
    cols = []
    for k in range(K):
        sel = np.arange(B) * K + k
        pos = np.concatenate([np.arange(starts[s], starts[s + 1]) for s in sel]).astype(np.int64)
        rows = offs[k] + ids[pos].clip(0, vocabs[k] - 1)
        koff = np.concatenate([[0], np.cumsum(lengths[sel])[:-1]])
        eb = torch.nn.functional.embedding_bag(torch.from_numpy(rows), t64, torch.from_numpy(koff), mode="sum",
                                               per_sample_weights=torch.from_numpy(w[pos].astype(np.float64)))
        if modes[k] == "mean":
            eb = eb / torch.from_numpy(np.maximum(lengths[sel], 1).astype(np.float64))[:, None]
        cols.append(eb)
    want = torch.cat(cols, dim=1)
    np.testing.assert_allclose(ref, want.detach().numpy(), rtol=1e-13, atol=1e-14)
    L = np.repeat(lengths.reshape(B, K), E, axis=1).astype(np.float64)
    err = np.abs(out.detach().cpu().numpy().astype(np.float64) - ref)
    assert (err <= gamma(L + 1) * mag).all()                                     # the forward bound
    # backward: against f64 over the f32 1 / L the lookup forms (one correctly rounded division), within gamma_(n+1)
    inv = np.where(np.tile(np.array([m == "mean" for m in modes]), B) & (lengths > 0),
                   np.float32(1) / np.maximum(lengths, 1).astype(np.float32), np.float32(1))
    uniq, sums, abs_sums, counts = W.weighted_backward(g, ids, lengths, offs, vocabs, modes, w, inv_len=inv)
    got = emb.store.grad.cpu().numpy()
    assert (np.abs(got[uniq].astype(np.float64) - sums) <= gamma(counts + 1)[:, None] * abs_sums).all()
    rest = np.ones(len(got), bool)
    rest[uniq] = False
    assert not got[rest].any()
    # ... and torch's autograd gradient of the float64 expression agrees with that reference up to the rounding of 1 / L
    want.backward(torch.from_numpy(g.astype(np.float64)))
    assert (np.abs(t64.grad.numpy()[uniq] - sums) <= U24 * abs_sums * (1 + 1e-6)).all()
    assert kjt.weights().grad is None and not kjt.weights().requires_grad       # no gradient flows to the weights


def test_weights_into_an_embedder_that_does_not_pool_are_refused(tt, manifest):
    from jodalrob_twotower_amd.cat_embed import CategoricalEmbedder
    cfg = _cfg(manifest)
    keys = cfg["keys_c"]
    emb = CategoricalEmbedder(keys, str(GOLD / "synthetic_metadata.csv"), "company", embedding_dim=cfg["E"], device=DEV)
    n = B * len(keys)
    plain = tt.KeyedJaggedTensor(keys, torch.zeros(n, dtype=torch.long, device=DEV))
    weighted = tt.KeyedJaggedTensor(keys, plain.values(), None, torch.ones(n, device=DEV))
    assert emb(plain, return_dict=False).shape == (B, len(keys) * cfg["E"])
    with pytest.raises(ValueError, match="not in bag mode"):
        emb(weighted)
    task = _task(tt, cfg, None, **F32)                                           # ... and through the towers of a plain task
    b = _batch(tt, cfg, 1.0, 614, weights=None, sides=())
    with pytest.raises(ValueError, match="not in bag mode"):
        task({"notice": b["notice"], "company": dict(b["company"], kjt=tt.KeyedJaggedTensor(keys, b["company"]["kjt"].values(), None,
                                                                                           torch.ones(n, device=DEV)))})


# ------------------------------------------------------------------------------------------- the captured step
def _nnz(b, side):
    return b[side]["kjt"].values().numel()


def _capture_setup(tt, manifest, example_weights="uniform"):
    from jodalrob_twotower_amd.graph import GraphedTrainStep
    from jodalrob_twotower_amd.optim import FusedAdam
    cfg = _cfg(manifest)
    te, tg = _task(tt, cfg, _pool(cfg), **F32), _task(tt, cfg, _pool(cfg), **F32)
    oe, og = (FusedAdam.for_task(t, lr=1e-2) for t in (te, tg))
    # the id counts: at the capacity, far below it, in between (a batch after a shorter one, stale weights of the first behind both)
    batches = [_batch(tt, cfg, m, 620 + i, weights=example_weights) for i, m in enumerate((5.0, 0.3, 2.0))]
    caps = {}
    for side in ("notice", "company"):
        n = [_nnz(b, side) for b in batches]
        assert n[0] > n[2] > n[1] and 2 * n[1] < n[0], n
        caps[side] = n[0]                                                        # batch 0 is exactly at the capacity
    gs = GraphedTrainStep(tg, og, batches[0], warmup=2, bag_capacity=caps)
    return cfg, te, tg, oe, og, batches, gs


def test_captured_weighted_step_equals_the_eager_step(tt, manifest):
    from jodalrob_twotower_amd import ops
    dev = torch.device(DEV)
    _L.check_device_errors(dev)
    cfg, te, tg, oe, og, batches, gs = _capture_setup(tt, manifest)
    try:
        for side in ("notice", "company"):
            st = gs.static[side]["kjt"]
            assert st.weights().dtype == torch.float32 and st.weights().numel() == st.values().numel() == gs.bag_capacity[side]
        with mock.patch.object(ops, "_bag_weight_args", wraps=ops._bag_weight_args) as spy:
            for i, b in enumerate(batches):
                le = _eager(te, oe, b)
                eager_calls = spy.call_count
                lg = gs.step(b)["loss"].detach().clone()
                assert spy.call_count == eager_calls                             # a replay: no lookup is issued from Python
                assert torch.equal(le, lg), (i, float(le), float(lg))
        assert spy.call_count >= len(batches)                                    # the eager steps took the _w entries
        torch.cuda.synchronize()
        _L.check_device_errors(dev)
        _assert_same_state(te, oe, tg, og)
    finally:
        gs.close()


def test_captured_step_refusals_change_nothing(tt, manifest):
    dev = torch.device(DEV)
    _L.check_device_errors(dev)
    for captured_with in ("uniform", None):
        cfg, te, tg, oe, og, batches, gs = _capture_setup(tt, manifest, captured_with)
        try:
            assert torch.equal(_eager(te, oe, batches[0]), gs.step(batches[0])["loss"])
            other = _batch(tt, cfg, 2.0, 630, weights=None if captured_with else "uniform")
            bad = [(other, "captured with them" if captured_with else "captured without them")]
            if captured_with:
                k = batches[2]["company"]["kjt"]
                short = tt.KeyedJaggedTensor(k.keys(), k.values(), k.lengths(), k.weights()[:-1])
                bad.append((dict(batches[2], company=dict(batches[2]["company"], kjt=short)), "weights for"))
            for b, what in bad:
                with pytest.raises(ValueError, match=what):
                    gs.step(b)
            if captured_with:
                with pytest.raises(ValueError, match="step_from_store: the step was captured with per-id weights"):
                    gs.step_from_store(None, None, torch.zeros((B, 2), dtype=torch.int64, device=DEV))
            for b in batches[1:]:                                                # the next valid steps are still the eager ones
                assert torch.equal(_eager(te, oe, b), gs.step(b)["loss"])
            torch.cuda.synchronize()
            _L.check_device_errors(dev)
            _assert_same_state(te, oe, tg, og)
        finally:
            gs.close()
