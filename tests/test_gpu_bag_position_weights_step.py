"""Learned position weights and differentiable per-id weights through the eager training step on the MI355X.

The small synthetic schema of the bag step tests (manifest case wide_b40: 5 + 2 keys, E = 16, towers [32, 24] -> 16) at B = 64,
dropout 0, fp32 modes; helpers of tests/test_gpu_embed_bag_weights_step.py and the files it builds on.

What is bit for bit and why:
  * every position weight 1.0 is the unweighted step: the expanded weights are copies of 1.0, and 1 * x = x, fma(1, x, acc) = acc + x
    in the weighted lookup and the weighted table gradient;
  * a task with position weights and a task fed explicit leaf weights equal to the expanded parameter run the same launches on the
    same values, so the backward entry over the second's weights.grad reproduces the first's position_weight.grad.
The towers hand the per-id gradient the slice of d_x the table gradient reads: with bags of one id, each row its own, sum pooling
and weights of 1.0 a touched row's gradient IS that slice (fl(1 * d) = d), so g must be the dot product of the row's gradient with the
row, within gamma(E + 2) * sum |d x| (tests/test_gpu_bag_weight_grad.py derives it; c = 1).
"""
import numpy as np
import pytest
import torch

from test_gpu_embed_bag import U24
from test_gpu_embed_bag_capture import _cfg, _task
from test_gpu_embed_bag_step import _step, _table_grad
from test_gpu_embed_bag_weights_step import F32, _batch, _pool, gamma
from test_gpu_parity import DEV, tt, make_task, to_batch, load_state  # noqa: F401

from jodalrob_twotower_amd import _lib as _L

pytestmark = pytest.mark.gpu

SIDES = (("notice", "notice_tower", "n"), ("company", "company_tower", "c"))


def _pw(cfg):
    """position weights on both towers' pooled keys (tests/test_gpu_embed_bag_weights_step.py: _pool); max_len 1 .. 3 against bags
    of about 3 ids: bags pass it"""
    return {cfg["keys_n"][3]: 3, cfg["keys_n"][4]: 2, cfg["keys_c"][0]: 3, cfg["keys_c"][1]: 1}


def _embedder(task, tower):
    return getattr(task.two_tower_model, tower).categorical_embedder


def _set_ones(task):
    with torch.no_grad():
        for _, tower, _ in SIDES:
            _embedder(task, tower).position_weight.fill_(1.0)


def _with_leaf_weights(tt, b, weights):
    """the batch with explicit per-id weights {side: leaf tensor that requires grad}"""
    out = dict(b)
    for side, w in weights.items():
        k = b[side]["kjt"]
        out[side] = dict(b[side], kjt=tt.KeyedJaggedTensor(k.keys(), k.values(), k.lengths(), w))
    return out


def test_at_initialisation_the_step_is_the_unweighted_step(tt, manifest):
    from jodalrob_twotower_amd import ops
    from unittest import mock
    cfg = _cfg(manifest)
    ta, tb = _task(tt, cfg, _pool(cfg), **F32), _task(tt, cfg, _pool(cfg), categorical_position_weights=_pw(cfg), **F32)
    _set_ones(tb)
    b = _batch(tt, cfg, 3.0, 710, weights=None)
    assert all(int(b[s]["kjt"].lengths().max()) > 3 for s, _, _ in SIDES)
    with mock.patch.object(ops, "bag_weight_grad", wraps=ops.bag_weight_grad) as spy:
        ra, da = _step(ta, b)
        assert spy.call_count == 0                                                # nobody differentiates weights: no new launch
        rb, db = _step(tb, b)
        assert spy.call_count == 1                                                # both towers' sides in one launch
    assert torch.equal(ra["loss"], rb["loss"])
    extra = sorted(set(db) - set(da))
    assert extra == sorted(f"two_tower_model.{t}.categorical_embedder.position_weight" for _, t, _ in SIDES) and len(da) >= 12
    for k in da:
        assert torch.equal(da[k], db[k]), k
    ga, touched_a = _table_grad(ta)
    gb, touched_b = _table_grad(tb)
    assert np.array_equal(touched_a, touched_b) and touched_a.any()
    assert np.array_equal(ga.view(np.uint32), gb.view(np.uint32))
    for k in extra:
        assert bool((db[k] != 0).all()) and bool(torch.isfinite(db[k]).all()), k


@pytest.mark.parametrize("mlp", ["fp32", "bf16"])
def test_the_towers_hand_over_the_slice_the_table_gradient_reads(tt, manifest, monkeypatch, mlp):
    from jodalrob_twotower_amd import config as _config
    cfg = dict(_cfg(manifest), B=12)
    n, E = 12, cfg["E"]
    modes = F32
    if mlp == "bf16":      # d_x stored as bf16: the source of both the table gradient and the weights' gradient is bf16
        monkeypatch.setattr(_config.settings, "tower_io_dtype", "both")
        modes = dict(embedding_grad="sparse", mlp_dtype="bf16", score_dtype="bf16")
    task = _task(tt, cfg, "sum", **modes)
    assert all(getattr(task.two_tower_model, t).dx_dtype == (torch.bfloat16 if mlp == "bf16" else torch.float32) for _, t, _ in SIDES)
    base = _batch(tt, cfg, 1.0, 711, weights=None, sides=(), n=n)
    g = torch.Generator().manual_seed(9)
    leaves, batch, ids = {}, dict(base), {}
    for side, tower, s in SIDES:
        keys, vocabs = cfg[f"keys_{s}"], cfg[f"vocab_{s}"]
        assert min(vocabs) >= n
        # every (sample, key) its own id: a table row is touched by one bag of one id alone
        ids[side] = torch.stack([torch.randperm(v, generator=g)[:n] for v in vocabs], dim=1).reshape(-1)
        leaves[side] = torch.ones(n * len(keys), device=DEV, requires_grad=True)
        kjt = tt.build_bag_kjt(keys, values=ids[side], lengths=torch.ones(n * len(keys), dtype=torch.long), device=DEV)
        batch[side] = dict(base[side], kjt=tt.KeyedJaggedTensor(keys, kjt.values(), kjt.lengths(), leaves[side]))
    table = task.two_tower_model.embedding_store.weight.detach().cpu().numpy().astype(np.float64)      # before the step
    _step(task, batch)
    grad, touched = _table_grad(task)
    for side, tower, s in SIDES:
        emb = _embedder(task, tower)
        K = len(emb.keys)
        rows = (emb._key_row_offset.cpu()[torch.arange(n * K) % K] + ids[side]).numpy()
        assert touched[rows].all() and len(set(rows.tolist())) == n * K
        d = grad[rows].astype(np.float64)                                         # fl(1 * d) = d: the slice the table gradient read
        if mlp == "bf16":
            assert not (grad[rows].view(np.uint32) & 0xFFFF).any()               # (bf16 values, widened)
        want, scale = (d * table[rows]).sum(1), np.abs(d * table[rows]).sum(1)
        got = leaves[side].grad
        assert got is not None and got.shape == (n * K,)
        err = np.abs(got.cpu().numpy().astype(np.float64) - want)
        print(f"\n[{mlp}] {side}: max err / bound = {float((err / (gamma(E + 2) * scale)).max()):.3f}, max |g| = {np.abs(want).max():.3e}")
        assert (err <= gamma(E + 2) * scale).all() and np.abs(want).max() > 0
    _L.check_device_errors(torch.device(DEV))


def test_position_weights_are_the_reduction_of_the_per_id_gradient(tt, manifest):
    from jodalrob_twotower_amd import ops
    cfg = _cfg(manifest)
    ta = _task(tt, cfg, _pool(cfg), categorical_position_weights=_pw(cfg), **F32)
    tb = _task(tt, cfg, _pool(cfg), **F32)
    b = _batch(tt, cfg, 3.0, 712, weights=None)
    leaves, sides = {}, {}
    for side, tower, _ in SIDES:
        emb = _embedder(ta, tower)
        p = emb.position_weight.detach()
        assert not bool((p == 1).any())                                           # (the loaded state: 1 + 0.1 * randn)
        kjt = b[side]["kjt"]
        sides[side] = ops.PosWeightSide(kjt.lengths(), emb._pw_offset, emb._pw_len, kjt.values().numel(), len(emb.keys))
        (w,) = ops.bag_position_weights(p, [sides[side]], cfg["B"])
        leaves[side] = w.clone().requires_grad_(True)
    ra, da = _step(ta, b)
    rb, db = _step(tb, _with_leaf_weights(tt, b, leaves))
    assert torch.equal(ra["loss"], rb["loss"])
    for k in db:
        assert torch.equal(da[k], db[k]), k
    for side, tower, _ in SIDES:
        emb = _embedder(ta, tower)
        want = ops.bag_position_weights_bwd(emb.position_weight.detach(), [sides[side]], cfg["B"], [leaves[side].grad])
        assert torch.equal(emb.position_weight.grad, want), side
        assert bool((want != 0).all())
    _L.check_device_errors(torch.device(DEV))


def test_optimizer_steps_the_parameter_and_state_dict_carries_it(tt, manifest):
    from jodalrob_twotower_amd.optim import FusedAdam
    cfg = _cfg(manifest)
    task = _task(tt, cfg, _pool(cfg), categorical_position_weights=_pw(cfg), **F32)
    names = [f"two_tower_model.{t}.categorical_embedder.position_weight" for _, t, _ in SIDES]
    params = dict(task.named_parameters())
    # FusedAdam.for_task: an ordinary non-table parameter -- in the towers' Adam group when the tables take another optimiser
    opt2 = FusedAdam.for_task(task, lr=1e-2, table_optimizer="rowwise_adagrad")
    towers_group, table_group = opt2.param_groups
    assert table_group.get("table_optimizer") == "rowwise_adagrad"
    for k in names:
        assert any(p is params[k] for p in towers_group["params"]) and not any(p is params[k] for p in table_group["params"])
    opt = FusedAdam.for_task(task, lr=1e-2)
    assert all(any(p is params[k] for grp in opt.param_groups for p in grp["params"]) for k in names)
    before = {k: params[k].detach().clone() for k in names}
    saved = {k: v.detach().clone() for k, v in task.state_dict().items()}
    assert set(names) <= set(saved)
    _step(task, _batch(tt, cfg, 3.0, 713, weights=None))
    opt.step()
    torch.cuda.synchronize()
    for k in names:
        moved = (params[k].detach() - before[k]).abs()
        assert bool((moved > 0).all()) and float(moved.max()) <= 1.01e-2, k       # Adam's first step: lr in magnitude
    # a state_dict round trip restores it (and everything else)
    task.load_state_dict(saved)
    for k in names:
        assert torch.equal(params[k].detach(), before[k]), k
    fresh = _task(tt, cfg, _pool(cfg), categorical_position_weights=_pw(cfg), **F32)
    with torch.no_grad():
        for k in names:
            dict(fresh.named_parameters())[k].zero_()
    fresh.load_state_dict(saved)
    for k in names:
        assert torch.equal(dict(fresh.named_parameters())[k].detach(), before[k]), k
    _L.check_device_errors(torch.device(DEV))


def test_captured_steps_refuse_learned_weights_and_change_nothing(tt, manifest):
    from jodalrob_twotower_amd.graph import GraphedTrainStep
    from jodalrob_twotower_amd.optim import FusedAdam
    cfg = _cfg(manifest)
    b = _batch(tt, cfg, 3.0, 714, weights=None)
    caps = {side: 2 * b[side]["kjt"].values().numel() for side, _, _ in SIDES}
    # an embedder with position weights
    task = _task(tt, cfg, _pool(cfg), categorical_position_weights=_pw(cfg), **F32)
    opt = FusedAdam.for_task(task, lr=1e-2)
    state = {k: v.detach().clone() for k, v in task.state_dict().items()}
    launches = _L.load().tt_launch_count()
    for kw in (dict(bag_capacity=caps), dict()):
        with pytest.raises(ValueError, match="GraphedTrainStep does not support learned position weights.*eager step"):
            GraphedTrainStep(task, opt, b, warmup=1, **kw)
    # example weights that require grad
    plain = _task(tt, cfg, _pool(cfg), **F32)
    popt = FusedAdam.for_task(plain, lr=1e-2)
    leaves = {side: torch.ones(b[side]["kjt"].values().numel(), device=DEV, requires_grad=True) for side, _, _ in SIDES}
    with pytest.raises(ValueError, match="GraphedTrainStep does not support per-id weights that require grad.*eager step"):
        GraphedTrainStep(plain, popt, _with_leaf_weights(tt, b, {"company": leaves["company"]}), warmup=1, bag_capacity=caps)
    assert _L.load().tt_launch_count() == launches                                # refused before anything ran, let alone a capture
    assert all(torch.equal(v, state[k]) for k, v in task.state_dict().items())
    assert all(t._seed_dev is None for t in (task.two_tower_model.notice_tower, task.two_tower_model.company_tower))
    # ... and the eager step of both still runs
    _step(task, b)
    _step(plain, _with_leaf_weights(tt, b, leaves))
    assert all(leaves[s].grad is not None and bool(leaves[s].grad.abs().sum() > 0) for s in leaves)
    # data weights (no grad) are captured as before
    data = _with_leaf_weights(tt, b, {s: w.detach() for s, w in leaves.items()})
    fresh = _task(tt, cfg, _pool(cfg), **F32)
    gs = GraphedTrainStep(fresh, FusedAdam.for_task(fresh, lr=1e-2), data, warmup=1, bag_capacity=caps)
    try:
        assert bool(torch.isfinite(gs.step(data)["loss"]))
    finally:
        gs.close()
    _L.check_device_errors(torch.device(DEV))
