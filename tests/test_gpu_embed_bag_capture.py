"""GraphedTrainStep(bag_capacity=...) on the MI355X: a bag-mode model's captured step against its eager step.  The small synthetic
schema of the bag tests (manifest case wide_b40: 5 + 2 keys, E = 16, towers [32, 24] -> 16) at B = 64, dropout 0.

Captured equals eager BIT FOR BIT: two tasks on the same weights, each with its own FusedAdam, train on the same five bag batches
whose id count rises, falls and rises again (one batch with many empty bags) -- stale ids of a longer batch sit behind a shorter
one in the static buffer.  The captured step runs the same kernels on the same values in the same order: tt_bag_prepare forms the
integers and the one division ops.embed_bag_lookup forms with torch, the capacity lookup adds pads nobody reads, and the padded
plan's real rows list their positions in the exact plan's order (tests/test_gpu_embed_bag_capacity.py pins each).  The launches a
captured step defers into other launches are bit-identical to their separate forms.  So torch.equal on the
loss of every step and, at the end, on every dense parameter, the whole fused table and every optimiser state tensor.
"""
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from test_gpu_parity import DEV, tt, make_task, to_batch, load_state  # noqa: F401

from jodalrob_twotower_amd import _lib as _L

pytestmark = pytest.mark.gpu

B = 64
MEANS = [3.0, 5.0, 1.5, 0.3, 4.0]                                 # mean bag lengths of the five batches: up, down (many empty), up


def _cfg(manifest):
    return dict(manifest["cases"]["wide_b40"], B=B)


def _task(tt, cfg, pool, **kw):
    from params_init import init_state_numpy
    task = make_task(tt, cfg, categorical_pooling=pool, **kw)
    load_state(task, init_state_numpy({k: tuple(v.shape) for k, v in task.state_dict().items()}, 77))
    task.train()
    task._pair_check_done = True
    return task


def _bag_sides(task):
    m = task.two_tower_model
    return [s for s, t in (("notice", m.notice_tower), ("company", m.company_tower)) if t.categorical_embedder.bag_mode]


def _batches(tt, cfg, sides, means=MEANS, avoid=None, terms=False):
    """one bag batch per mean length: the plain synthetic batch with every key of the bag-mode `sides` turned into ragged bags.
    avoid: {side: (first row's id, last row's id)} ids the batches must not use (the pad test)"""
    from jodalrob_twotower_amd import synthetic
    from params_init import synth_batch_numpy
    out = []
    for i, mean in enumerate(means):
        nb = synth_batch_numpy(B, cfg["vocab_n"], cfg["vocab_c"], cfg["din_n"], cfg["din_c"], 610 + i, oob=False)
        b = to_batch(tt, nb, cfg["keys_n"], cfg["keys_c"])
        for side in sides:
            keys, vocabs = cfg[f"keys_{side[0]}"], cfg[f"vocab_{side[0]}"]
            kjt = synthetic.ragged_bags(b[side]["kjt"], vocabs, keys, mean, seed=900 + 10 * i + len(side))
            if avoid is not None:
                K = len(keys)
                key = torch.repeat_interleave(torch.arange(kjt.lengths().numel(), device=DEV) % K, kjt.lengths())
                v = kjt.values().clone()
                first, last = avoid[side]
                if first:
                    v[(key == 0) & (v == 0)] = 1
                if last:
                    v[(key == K - 1) & (v >= vocabs[-1] - 1)] = vocabs[-1] - 2
                kjt = tt.KeyedJaggedTensor(keys, v, kjt.lengths())
            b[side] = dict(b[side], kjt=kjt)
        if terms:
            g = torch.Generator().manual_seed(40 + i)
            for s in ("notice", "company"):
                b[s]["log_q"] = (torch.rand(B, generator=g) * -3.0).to(DEV)
                b[s]["entity"] = torch.randint(0, B // 2, (B,), generator=g).to(torch.int32).to(DEV)
        out.append(b)
    return out


def _nnz(batches, side):
    return [b[side]["kjt"].values().numel() for b in batches]


def _eager(task, opt, batch):
    opt.zero_grad()
    res = task(batch, return_metrics=True)
    res["loss"].backward()
    opt.step()
    return res["loss"].detach().clone()


def _state_tensors(opt):
    """every optimiser state tensor: the dense parameters' Adam moments and the stores' moments / Adagrad sums"""
    opt._flush_pending()
    out = []
    for group in opt.param_groups:
        for p in group["params"]:
            st = opt.state.get(p) or {}
            out += [st[k] for k in ("exp_avg", "exp_avg_sq", "sum") if k in st]
    for store in opt._stores:
        st = opt._state_of(store)
        out += [st[k] for k in ("m", "v", "sum") if k in st]
    return out


def _assert_same_state(ta, oa, tb, ob):
    for (k, a), (_, b) in zip(ta.named_parameters(), tb.named_parameters()):
        assert torch.equal(a, b), k                                    # every dense parameter and every table view
    assert torch.equal(ta.two_tower_model.embedding_store.weight, tb.two_tower_model.embedding_store.weight)      # the whole fused table
    sa, sb = _state_tensors(oa), _state_tensors(ob)
    assert len(sa) == len(sb) and len(sa) >= 20
    for a, b in zip(sa, sb):
        assert torch.equal(a, b)
    assert oa.current_step() == ob.current_step()


VARIANTS = {
    "f32-sparse": dict(pool={"notice": "sum", "company": "mean"}, kw=dict(embedding_grad="sparse", mlp_dtype="fp32", score_dtype="fp32")),
    "bf16-sparse": dict(pool={"notice": "mean", "company": "mean"}, kw=dict(embedding_grad="sparse", mlp_dtype="bf16", score_dtype="bf16")),
    "dense-grad": dict(pool={"notice": "mean", "company": "sum"}, kw=dict(embedding_grad="dense", mlp_dtype="fp32", score_dtype="fp32")),
    "rowwise-adagrad": dict(pool={"notice": "mean", "company": "mean"}, kw=dict(embedding_grad="sparse", mlp_dtype="fp32", score_dtype="fp32"),
                            opt=dict(table_optimizer="rowwise_adagrad", table_lr=5e-2)),
    "company-only": dict(pool={"company": "mean"}, kw=dict(embedding_grad="sparse", mlp_dtype="fp32", score_dtype="fp32")),
    "logq-entity": dict(pool={"notice": "mean", "company": "mean"}, kw=dict(embedding_grad="sparse", mlp_dtype="bf16", score_dtype="bf16"),
                        terms=True),
}


@pytest.mark.parametrize("name", list(VARIANTS))
def test_captured_bag_step_equals_the_eager_step(tt, manifest, name):
    from jodalrob_twotower_amd.graph import GraphedTrainStep
    from jodalrob_twotower_amd.optim import FusedAdam
    v, cfg, dev = VARIANTS[name], _cfg(manifest), torch.device(DEV)
    te, tg = _task(tt, cfg, v["pool"], **v["kw"]), _task(tt, cfg, v["pool"], **v["kw"])
    sides = _bag_sides(te)
    assert sides == (["company"] if name == "company-only" else ["notice", "company"])
    if name == "bf16-sparse":
        assert tg.two_tower_model.company_tower.x_dtype == torch.bfloat16      # the pooled block is written as bf16
    oe, og = (FusedAdam.for_task(t, lr=1e-2, **v.get("opt", {})) for t in (te, tg))
    batches = _batches(tt, cfg, sides, terms=v.get("terms", False))
    for side in sides:
        n = _nnz(batches, side)
        assert n[0] < n[1] > n[2] > n[3] < n[4], n                     # rises, falls, rises again
        assert int((batches[3][side]["kjt"].lengths() == 0).sum()) > B            # many empty bags
    caps = {side: max(_nnz(batches, side)) + 17 for side in sides}
    _L.check_device_errors(dev)
    from unittest import mock
    from jodalrob_twotower_amd import ops
    with mock.patch.object(ops, "_embed_bag_lookup_cap", wraps=ops._embed_bag_lookup_cap) as spy:
        gs = GraphedTrainStep(tg, og, batches[0], warmup=2, bag_capacity=caps)
    assert spy.call_count == 3                                         # two warm-up steps and the capture ran the capacity form
    assert gs.bag_capacity == caps and gs._ingest is None
    try:
        for i, b in enumerate(batches):
            le = _eager(te, oe, b)
            lg = gs.step(b)["loss"].detach().clone()
            assert torch.equal(le, lg), (i, float(le), float(lg))
        torch.cuda.synchronize()
        _L.check_device_errors(dev)                                    # no refused offsets, no decoded stale id
        _assert_same_state(te, oe, tg, og)
    finally:
        gs.close()


def test_pads_touch_neither_row_0_nor_the_last_row(tt, manifest):
    """The pad positions name the row one past the table and are not counted in n_unique: with batches that use neither the table's
    row 0 nor its last row, those rows' weights and Adam moments are bitwise unchanged after the captured steps (a zero-gradient
    visit under Adam would decay the moments and, with weight decay, move the weight)."""
    from jodalrob_twotower_amd.graph import GraphedTrainStep
    from jodalrob_twotower_amd.optim import FusedAdam
    cfg = _cfg(manifest)
    task = _task(tt, cfg, {"notice": "mean", "company": "mean"}, embedding_grad="sparse", mlp_dtype="fp32", score_dtype="fp32")
    store = task.two_tower_model.embedding_store
    first_side = "notice" if task.two_tower_model.notice_tower.categorical_embedder.row_base == 0 else "company"
    last_side = "company" if first_side == "notice" else "notice"
    batches = _batches(tt, cfg, ["notice", "company"], avoid={first_side: (True, False), last_side: (False, True)})
    opt = FusedAdam.for_task(task, lr=1e-2, weight_decay=1e-2)
    _eager(task, opt, _batches(tt, cfg, ["notice", "company"], means=[2.0])[0])      # moments exist, and rows 0 / last have some
    st = opt._state_of(store)
    st["m"][[0, -1]] = 0.25
    st["v"][[0, -1]] = 0.5
    before = [t[[0, -1]].clone() for t in (store.weight, st["m"], st["v"])]
    gs = GraphedTrainStep(task, opt, batches[0], warmup=2, bag_capacity="auto")
    assert all(c >= 1024 for c in gs.bag_capacity.values())            # far more pads than ids
    try:
        w0 = store.weight.clone()
        for b in batches:
            gs.step(b)
        torch.cuda.synchronize()
        assert not torch.equal(w0, store.weight)
        for t, was in zip((store.weight, st["m"], st["v"]), before):
            assert torch.equal(t[[0, -1]], was)
    finally:
        gs.close()


@pytest.mark.parametrize("grad_mode,table_opt", [("sparse", "adam"), ("dense", "adam"), ("sparse", "rowwise_adagrad")])
def test_preserve_state_leaves_no_trace_of_the_warm_up(tt, manifest, grad_mode, table_opt):
    from jodalrob_twotower_amd.graph import GraphedTrainStep
    from jodalrob_twotower_amd.optim import FusedAdam
    cfg = _cfg(manifest)
    task = _task(tt, cfg, {"notice": "sum", "company": "mean"}, embedding_grad=grad_mode, mlp_dtype="fp32", score_dtype="fp32")
    opt = FusedAdam.for_task(task, lr=1e-2, table_optimizer=table_opt)
    batches = _batches(tt, cfg, ["notice", "company"], means=[2.0, 3.0])
    _eager(task, opt, batches[1])                                      # a step before: moments, step counts and running statistics exist
    snap = lambda: ([p.detach().clone() for p in task.parameters()] + [b.detach().clone() for b in task.buffers()] +
                    [t.clone() for t in _state_tensors(opt)] + [task.two_tower_model.embedding_store.weight.clone()])
    before, step0 = snap(), opt.current_step()
    gs = GraphedTrainStep(task, opt, batches[0], warmup=3, bag_capacity=2000)
    try:
        after = snap()
        assert len(before) == len(after) and all(torch.equal(a, b) for a, b in zip(before, after))
        assert opt.current_step() == step0 and sum(b.numel() for b in task.buffers()) > 0
        gs.step(batches[0])
        torch.cuda.synchronize()
        assert opt.current_step() == step0 + 1 and not all(torch.equal(a, b) for a, b in zip(before, snap()))
    finally:
        gs.close()


def test_a_batch_over_the_capacity_is_refused_and_changes_nothing(tt, manifest):
    from jodalrob_twotower_amd.graph import GraphedTrainStep
    from jodalrob_twotower_amd.optim import FusedAdam
    cfg, dev = _cfg(manifest), torch.device(DEV)
    kw = dict(embedding_grad="sparse", mlp_dtype="fp32", score_dtype="fp32")
    te, tg = _task(tt, cfg, {"company": "mean"}, **kw), _task(tt, cfg, {"company": "mean"}, **kw)
    oe, og = (FusedAdam.for_task(t, lr=1e-2) for t in (te, tg))
    small, big, nxt = _batches(tt, cfg, ["company"], means=[2.0, 6.0, 1.0])
    n = _nnz([small, big, nxt], "company")
    cap = n[0] + 5
    assert n[1] > cap >= n[2]
    gs = GraphedTrainStep(tg, og, small, warmup=1, bag_capacity=cap)
    try:
        assert torch.equal(_eager(te, oe, small), gs.step(small)["loss"])
        held = [t.clone() for s in ("notice", "company") for t in (gs.static[s]["dense"], gs.static[s]["kjt"].values(), gs.static[s]["kjt"].lengths())]
        count = gs.static["company"]["kjt"].bag_count.clone()
        with pytest.raises(ValueError, match=rf"company: {n[1]} ids, the step was captured with bag_capacity = {cap}"):
            gs.step(big)
        short = dict(nxt, company=dict(nxt["company"], kjt=tt.KeyedJaggedTensor(cfg["keys_c"], nxt["company"]["kjt"].values(),
                                                                              nxt["company"]["kjt"].lengths()[:-1])))
        with pytest.raises(ValueError, match=r"company: \d+ bag lengths, the captured step holds B\*K"):
            gs.step(short)
        now = [t for s in ("notice", "company") for t in (gs.static[s]["dense"], gs.static[s]["kjt"].values(), gs.static[s]["kjt"].lengths())]
        assert all(torch.equal(a, b) for a, b in zip(held, now)) and torch.equal(count, gs.static["company"]["kjt"].bag_count)
        assert torch.equal(_eager(te, oe, nxt), gs.step(nxt)["loss"])  # the next fitting batch: bit for bit as the eager twin
        torch.cuda.synchronize()
        _L.check_device_errors(dev)
        _assert_same_state(te, oe, tg, og)
    finally:
        gs.close()


def test_refusals_that_stay(tt, manifest):
    from jodalrob_twotower_amd.data_loader import DeviceFeatureStore
    from jodalrob_twotower_amd.graph import GraphedTrainStep
    from jodalrob_twotower_amd.optim import FusedAdam
    from jodalrob_twotower_amd.segmented import SegmentedTrainStep
    from jodalrob_twotower_amd.unrolled import UnrolledTrainStep
    cfg = _cfg(manifest)
    kw = dict(embedding_grad="sparse", mlp_dtype="fp32", score_dtype="fp32")
    bag, plain = _task(tt, cfg, {"company": "mean"}, **kw), _task(tt, cfg, None, **kw)
    b = _batches(tt, cfg, ["company"], means=[2.0])[0]
    opt = FusedAdam.for_task(bag, lr=1e-2)
    with pytest.raises(ValueError, match="GraphedTrainStep does not support bag mode"):       # the refusal the existing test pins
        GraphedTrainStep(bag, opt, b)
    for cls in (UnrolledTrainStep, SegmentedTrainStep):
        with pytest.raises(ValueError, match=rf"{cls.__name__} does not support bag mode"):
            cls(bag, opt, b, bag_capacity=4096)
    M, K = 5, len(cfg["keys_c"])
    neg = {"dense": b["company"]["dense"][:M] + 0.5,
           "kjt": tt.build_bag_kjt(cfg["keys_c"], values=torch.zeros(M * K, dtype=torch.long), lengths=torch.ones(M * K, dtype=torch.long), device=DEV)}
    with pytest.raises(NotImplementedError, match="extra negatives"):
        GraphedTrainStep(bag, opt, dict(b, negatives=neg), bag_capacity=4096)
    plain_b = _batches(tt, cfg, [], means=[1.0])[0]
    with pytest.raises(ValueError, match="bag_capacity: the model has no bag-mode embedder"):
        GraphedTrainStep(plain, FusedAdam.for_task(plain, lr=1e-2), plain_b, bag_capacity=4096)
    with pytest.raises(ValueError, match="bag_capacity = 3 for 'company'"):
        GraphedTrainStep(bag, opt, b, bag_capacity=3)
    gs = GraphedTrainStep(bag, opt, b, warmup=1, bag_capacity=4096)
    try:
        stores = [DeviceFeatureStore({"dense_projected": plain_b[s]["dense"], "categorical": plain_b[s]["kjt"].values().view(B, -1)},
                                     cfg[f"keys_{s[0]}"], DEV) for s in ("notice", "company")]
        pairs = torch.stack([torch.arange(B), torch.arange(B)], 1).to(DEV)
        with pytest.raises(ValueError, match="step_from_store does not support bag mode"):
            gs.step_from_store(stores[0], stores[1], pairs)
    finally:
        gs.close()


def test_train_driver_captures_the_pooled_loop(tt, tmp_path):
    """scripts/train.py --pool ... --pool-capture 2: the pooled loop through GraphedTrainStep.step(batch); its per-step losses (and
    the epoch's mean) equal those of the same command without --pool-capture.  Both runs seed torch and switch dropout off: the
    captured step draws its dropout seed with the step's scalars, the eager one per tower."""
    def run(extra):
        cmd = [sys.executable, str(ROOT / "scripts" / "train.py"), "--results-csv", str(tmp_path / "r.csv"), "--output-dir", str(tmp_path / "m"),
               "--pairs", "3000", "--entities", "600", "--steps", "6", "--pool", "rgncd=mean", "cntrynm=sum", "ntceinsttcd=mean",
               "--pool-length", "3", "--seed", "11", "--dropout-rate", "0", "--log-interval", "1"] + extra
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert "done: 6 steps" in r.stdout
        steps = [ln for ln in r.stdout.splitlines() if ln.startswith("step ")]
        assert len(steps) == 6
        return steps + [ln for ln in r.stdout.splitlines() if ln.startswith(("Train -", "Val   -"))], r.stdout
    eager, _ = run([])
    captured, out = run(["--pool-capture", "2"])
    assert "--pool-capture: captured with bag_capacity" in out
    assert f"--pool-capture: 6 captured steps, 0 batches took the eager step" in out
    assert eager == captured and len(eager) == 8
    r = subprocess.run([sys.executable, str(ROOT / "scripts" / "train.py"), "--pool-capture", "2"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 2 and "--pool-capture needs --pool" in r.stderr
