"""Row-wise Adagrad for the embedding tables (FusedAdam.for_task(table_optimizer="rowwise_adagrad")) on the MI355X: the
kernels against an f64 restatement of the update, the fused launch against the separate entries, dense against sparse grad
mode, the task step against the oracle, graph replay against eager steps, checkpoints, and the sharded store."""
import io
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import oracle_np as O
from conftest import GOLD
from params_init import init_state_numpy, synth_batch_numpy
from test_gpu_parity import DEV, load_state, make_task, to_batch, tt  # noqa: F401  (tt: the module fixture)

pytestmark = pytest.mark.gpu


def rowwise_adagrad_f64(w, g, s, lr, eps, wd):
    """One row-wise Adagrad step on rows w [n, E] (f64 in place) with gradients g and accumulators s [n]."""
    g = g + wd * w if wd != 0 else g
    s += (g * g).sum(axis=1) / w.shape[1]
    w -= (lr / (np.sqrt(s) + eps))[:, None] * g


def _plan_rows(rng, n, R, pads, long_rows):
    """n slot ids over [0, R + pads): pads >= R are routing pads; `long_rows` ids repeat more than 64 times."""
    ids = rng.integers(0, R + pads, n)
    hot = rng.integers(0, R, long_rows)
    for i, h in enumerate(hot):
        ids[i * 100:(i + 1) * 100] = h
    return torch.from_numpy(rng.permutation(ids).astype(np.int32)).to(DEV)


@pytest.mark.parametrize("E", [32, 64, 7, 256])
@pytest.mark.parametrize("wd", [0.0, 1e-4])
def test_sparse_kernel_matches_f64(tt, E, wd):
    from jodalrob_twotower_amd import ops
    rng = np.random.default_rng(E * 10 + int(wd > 0))
    R, pads, lr, eps = 3000, 40, 0.05, 1e-8
    w0 = rng.standard_normal((R, E)).astype(np.float32)
    table = torch.from_numpy(w0).to(DEV)
    acc = torch.zeros(R, dtype=torch.float32, device=DEV)
    # M = 0: nothing runs, nothing changes
    z = torch.zeros(1, dtype=torch.int32, device=DEV)
    empty = ops.DedupPlan(z, z, z, z, 0)
    ops.rowwise_adagrad_sparse(table, acc, empty, torch.zeros(0, E, device=DEV), lr, eps, wd)
    torch.cuda.synchronize()
    assert np.array_equal(table.cpu().numpy(), w0) and not acc.any()
    w, s = w0.astype(np.float64), np.zeros(R)
    touched = np.zeros(R, bool)
    for step in range(4):
        plan = ops.dedup_plan(_plan_rows(rng, 4000, R, pads, 3), R + pads)
        grad = torch.from_numpy(rng.standard_normal((plan.M, E)).astype(np.float32)).to(DEV)
        before = table.cpu().numpy(), acc.cpu().numpy()
        ops.rowwise_adagrad_sparse(table, acc, plan, grad, lr, eps, wd)
        U = int(plan.n_unique.item())
        u = plan.unique_rows[:U].cpu().numpy().astype(np.int64)
        assert (u >= R).any() and (u < R).any()
        keep = u < R
        rows, g = u[keep], grad[:U].cpu().numpy().astype(np.float64)[keep]
        ws, ss = w[rows], s[rows]
        rowwise_adagrad_f64(ws, g, ss, lr, eps, wd)
        w[rows], s[rows] = ws, ss
        touched[rows] = True
        out_w, out_s = table.cpu().numpy(), acc.cpu().numpy()
        np.testing.assert_allclose(out_w, w, rtol=1e-5, atol=1e-6, err_msg=f"step {step}")
        np.testing.assert_allclose(out_s, s, rtol=1e-5, atol=0, err_msg=f"step {step}")
        untouched = np.ones(R, bool)
        untouched[rows] = False
        assert np.array_equal(out_w[untouched], before[0][untouched]) and np.array_equal(out_s[untouched], before[1][untouched])
    assert touched.sum() > 100
    # the same inputs twice: the same bits (fixed reduction order)
    again_t, again_a = torch.from_numpy(w0).to(DEV), torch.zeros(R, device=DEV)
    first_t, first_a = torch.from_numpy(w0).to(DEV), torch.zeros(R, device=DEV)
    plan = ops.dedup_plan(_plan_rows(rng, 4000, R, pads, 3), R + pads)
    grad = torch.from_numpy(rng.standard_normal((plan.M, E)).astype(np.float32)).to(DEV)
    ops.rowwise_adagrad_sparse(first_t, first_a, plan, grad, lr, eps, wd)
    ops.rowwise_adagrad_sparse(again_t, again_a, plan, grad, lr, eps, wd)
    assert torch.equal(first_t, again_t) and torch.equal(first_a, again_a)


@pytest.mark.parametrize("E", [32, 7, 256])
def test_dense_kernel_matches_f64_and_sparse_at_wd0(tt, E):
    from jodalrob_twotower_amd import ops
    rng = np.random.default_rng(400 + E)
    R, lr, eps = 2000, 0.05, 1e-8
    w0 = rng.standard_normal((R, E)).astype(np.float32)
    for wd in (0.0, 1e-4):
        table, acc = torch.from_numpy(w0).to(DEV), torch.zeros(R, device=DEV)
        w, s = w0.astype(np.float64), np.zeros(R)
        for step in range(3):
            g = rng.standard_normal((R, E)).astype(np.float32)
            g[rng.random(R) < 0.5] = 0                                  # rows without gradient
            ops.rowwise_adagrad_dense(table, acc, torch.from_numpy(g).to(DEV), lr, eps, wd)
            rowwise_adagrad_f64(w, g.astype(np.float64), s, lr, eps, wd)
            np.testing.assert_allclose(table.cpu().numpy(), w, rtol=1e-5, atol=1e-6, err_msg=f"wd {wd} step {step}")
            np.testing.assert_allclose(acc.cpu().numpy(), s, rtol=1e-5, atol=0)
            if wd == 0 and step == 0:                                   # a row without gradient does not move
                zero = ~g.any(axis=1)
                assert np.array_equal(table.cpu().numpy()[zero], w0[zero])
    # wd = 0: the sparse form over the rows with a gradient IS the dense update
    g = np.zeros((R, E), np.float32)
    ids = _plan_rows(rng, 3000, R, 0, 2)
    plan = ops.dedup_plan(ids, R)
    U = int(plan.n_unique.item())
    u = plan.unique_rows[:U].cpu().numpy().astype(np.int64)
    grad_rows = torch.from_numpy(rng.standard_normal((plan.M, E)).astype(np.float32)).to(DEV)
    g[u] = grad_rows[:U].cpu().numpy()
    td, ad = torch.from_numpy(w0).to(DEV), torch.zeros(R, device=DEV)
    tsp, asp = torch.from_numpy(w0).to(DEV), torch.zeros(R, device=DEV)
    ops.rowwise_adagrad_dense(td, ad, torch.from_numpy(g).to(DEV), lr, eps, 0.0)
    ops.rowwise_adagrad_sparse(tsp, asp, plan, grad_rows, lr, eps, 0.0)
    assert torch.equal(td, tsp) and torch.equal(ad, asp)


@pytest.mark.parametrize("E", [32, 64, 7, 256])
def test_fused_plain_equals_separate_entries(tt, E):
    from jodalrob_twotower_amd import ops
    rng = np.random.default_rng(700 + E)
    R, lr, eps, wd, t_lr, t_eps, t_wd = 2500, 1e-2, 1e-8, 1e-5, 0.05, 1e-7, 1e-4
    shapes = [(300, 40), (40,), (64, 300), (5,)]
    towers0 = [rng.standard_normal(s).astype(np.float32) for s in shapes]
    grads = [torch.from_numpy(rng.standard_normal(s).astype(np.float32)).to(DEV) for s in shapes]
    w0 = rng.standard_normal((R, E)).astype(np.float32)
    plan = ops.dedup_plan(_plan_rows(rng, 5000, R, 30, 3), R + 30)
    grad_rows = torch.from_numpy(rng.standard_normal((plan.M, E)).astype(np.float32)).to(DEV)
    outs = []
    for fused in (False, True):
        ps = [torch.from_numpy(t).to(DEV) for t in towers0]
        ms = [torch.full_like(p, 0.01) for p in ps]
        vs = [torch.full_like(p, 0.02) for p in ps]
        table, acc = torch.from_numpy(w0).to(DEV), torch.full((R,), 0.5, device=DEV)
        items = list(zip(ps, grads, ms, vs))
        for step in (1, 2):
            if fused:
                ops.adam_rowwise_adagrad_fused(items, step, lr, 0.9, 0.999, eps, wd, None, table, acc, plan, grad_rows, t_lr, t_eps, t_wd)
            else:
                ops.adam_multi(items, step, lr, 0.9, 0.999, eps, wd)
                ops.rowwise_adagrad_sparse(table, acc, plan, grad_rows, t_lr, t_eps, t_wd)
        outs.append([t.cpu() for t in ps + ms + vs + [table, acc]])
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def _real_task(tt, manifest, schema_real):
    cfg = dict(manifest["cases"]["real_schema"])
    kn, kc = schema_real["notice"]["categorical"], schema_real["company"]["categorical"]
    cfg.update(keys_n=kn, keys_c=kc)
    return cfg, kn, kc


@pytest.mark.parametrize("B", [2048, 777])
def test_fused_finish_equals_separate_entries(tt, manifest, schema_real, monkeypatch, B):
    """TT_GRAD_DEFER_FINISH + the fused _finish launch (long rows of thousands of slots, finished and updated inside it) ==
    the plain fused launch == tower Adam then the sparse Adagrad entry after the reduction's own finish, bit for bit:
    gradient rows, table, accumulator and every dense weight after two steps.  Real 32 + 6 key schema."""
    from jodalrob_twotower_amd.optim import FusedAdam
    cfg, kn, kc = _real_task(tt, manifest, schema_real)
    vn, vc = schema_real["notice"]["vocab_sizes"], schema_real["company"]["vocab_sizes"]
    batches = [synth_batch_numpy(B, vn, vc, cfg["din_n"], cfg["din_c"], 650 + i, oob=True) for i in range(2)]
    from jodalrob_twotower_amd import ops
    fused_calls = []
    real = ops.adam_rowwise_adagrad_fused
    monkeypatch.setattr(ops, "adam_rowwise_adagrad_fused", lambda *a, **k: (fused_calls.append(1), real(*a, **k)))
    outs, state = {}, None
    for variant in ("separate", "fused", "fused_finish"):
        fused_calls.clear()
        task = make_task(tt, cfg, meta=GOLD / "real_vocab_metadata.csv", embedding_grad="sparse", mlp_dtype="bf16", score_dtype="bf16")
        if state is None:
            state = init_state_numpy({k: tuple(v.shape) for k, v in task.state_dict().items()}, 651)
        load_state(task, state)
        task.train()
        opt = FusedAdam.for_task(task, table_optimizer="rowwise_adagrad", lr=1e-2, weight_decay=1e-5, table_lr=0.05,
                                 table_weight_decay=1e-4)
        store = task.two_tower_model.embedding_store
        store = store() if callable(store) else store
        if variant == "separate":
            opt._fusable_store = lambda *a, **k: None
        grads = []
        for b in batches:
            opt.zero_grad()
            store.defer_long_finish = variant == "fused_finish"
            task(to_batch(tt, b, kn, kc), return_metrics=True)["loss"].backward()
            store.defer_long_finish = False
            plan, rows = store.sparse_grad
            assert (plan.finish_deferred is not None) == (variant == "fused_finish")
            opt.step()
            assert plan.finish_deferred is None and store.sparse_grad is None
            U = int(plan.n_unique.item())
            grads.append((plan.unique_rows[:U].cpu().numpy(), rows[:U].cpu().numpy()))
        assert len(fused_calls) == (0 if variant == "separate" else len(batches)), variant
        st = opt._state_of(store)
        outs[variant] = (grads, store.weight.cpu().numpy(), st["sum"].cpu().numpy(),
                         {k: v.detach().cpu().numpy() for k, v in task.state_dict().items()})
    ref = outs["separate"]
    assert ref[2].any()
    for variant in ("fused", "fused_finish"):
        for (u0, g0), (u1, g1) in zip(ref[0], outs[variant][0]):
            assert np.array_equal(u0, u1) and np.array_equal(g0, g1), variant
        assert np.array_equal(ref[1], outs[variant][1]), variant
        assert np.array_equal(ref[2], outs[variant][2]), variant
        for k, v in ref[3].items():
            assert np.array_equal(v, outs[variant][3][k]), (variant, k)


def test_task_step_matches_oracle(tt, manifest):
    """3 steps of FusedAdam.for_task(table_optimizer="rowwise_adagrad") == Adam on the towers and the f64 row-wise update on
    the tables (O.task_step gradients), sparse and dense grad modes; after step 1 the towers equal an Adam-tables run."""
    from jodalrob_twotower_amd.optim import FusedAdam
    cfg = dict(manifest["cases"]["wide_b40"])
    lr, wd, t_lr, t_wd = 1e-2, 1e-4, 0.05, 1e-4
    finals = {}
    for mode in ("dense", "sparse"):
        task = make_task(tt, cfg, embedding_grad=mode)
        shapes = {k: tuple(v.shape) for k, v in task.state_dict().items()}
        state = init_state_numpy(shapes, 31)
        load_state(task, state)
        opt = FusedAdam.for_task(task, table_optimizer="rowwise_adagrad", lr=lr, weight_decay=wd, table_lr=t_lr,
                                 table_weight_decay=t_wd)
        pk = [k for k in state if "running" not in k and "num_batches" not in k]
        m = {k: np.zeros_like(state[k]) for k in pk}
        v = {k: np.zeros_like(state[k]) for k in pk}
        acc = {k: np.zeros(state[k].shape[0]) for k in pk if "embeddings" in k}
        st = {k: np.array(val, copy=True) for k, val in state.items()}
        task.train()
        for s in range(3):
            b = synth_batch_numpy(cfg["B"], cfg["vocab_n"], cfg["vocab_c"], cfg["din_n"], cfg["din_c"], 50 + s, oob=False)
            opt.zero_grad()
            task(to_batch(tt, b, cfg["keys_n"], cfg["keys_c"])).backward()
            opt.step()
            ref = O.task_step(st, b, cfg["keys_n"], cfg["keys_c"], cfg["vocab_n"], cfg["vocab_c"], cfg["T"], True)
            for k in pk:
                g = ref["grads"][k]
                if "embeddings" in k:
                    rows = np.flatnonzero(np.abs(g).sum(1) > 0) if mode == "sparse" else np.arange(g.shape[0])
                    w64, s64 = st[k][rows].astype(np.float64), acc[k][rows]
                    rowwise_adagrad_f64(w64, g[rows].astype(np.float64), s64, t_lr, 1e-8, t_wd)
                    st[k][rows], acc[k][rows] = w64, s64
                else:
                    O.adam_step(st[k], g, m[k], v[k], s + 1, lr, wd=wd)
            st.update(ref["bn_updates"])
            if s == 0 and mode == "sparse":               # towers after step 1 == a table_optimizer="adam" run from the same state
                other = make_task(tt, cfg, embedding_grad=mode)
                load_state(other, state)
                other.train()
                oa = FusedAdam.for_task(other, lr=lr, weight_decay=wd)
                other(to_batch(tt, b, cfg["keys_n"], cfg["keys_c"])).backward()
                oa.step()
                theirs = dict(other.named_parameters())
                for n, p in task.named_parameters():
                    if "embeddings" not in n:
                        assert torch.equal(p, theirs[n]), n
        for k, val in task.state_dict().items():
            np.testing.assert_allclose(val.cpu().numpy(), st[k], rtol=2e-4, atol=2e-6, err_msg=f"{mode}:{k}")
        params = dict(task.named_parameters())
        for k, a in acc.items():
            np.testing.assert_allclose(opt.state[params[k]]["sum"].cpu().numpy(), a, rtol=2e-4, atol=1e-9, err_msg=f"{mode}:{k}")
        finals[mode] = {k: v.detach().cpu().numpy().copy() for k, v in task.state_dict().items()}
    assert finals["dense"].keys() == finals["sparse"].keys()


def test_sparse_mode_equals_dense_mode_at_wd0(tt, manifest):
    """weight_decay = 0: the row-sparse update is the exact sparse form of the dense one (no bias correction, a row without
    gradient does not move)."""
    from jodalrob_twotower_amd.optim import FusedAdam
    cfg = dict(manifest["cases"]["wide_b40"])
    finals = {}
    for mode in ("dense", "sparse"):
        task = make_task(tt, cfg, embedding_grad=mode)
        load_state(task, init_state_numpy({k: tuple(v.shape) for k, v in task.state_dict().items()}, 32))
        opt = FusedAdam.for_task(task, table_optimizer="rowwise_adagrad", lr=1e-2, table_lr=0.05)
        task.train()
        for s in range(3):
            b = synth_batch_numpy(cfg["B"], cfg["vocab_n"], cfg["vocab_c"], cfg["din_n"], cfg["din_c"], 60 + s, oob=False)
            opt.zero_grad()
            task(to_batch(tt, b, cfg["keys_n"], cfg["keys_c"])).backward()
            opt.step()
        finals[mode] = {n: p.detach().cpu().numpy().copy() for n, p in task.named_parameters()}
        finals[mode + "_sum"] = {n: opt.state[p]["sum"].cpu().numpy().copy() for n, p in task.named_parameters() if "embeddings" in n}
    for n, v in finals["dense"].items():
        np.testing.assert_allclose(finals["sparse"][n], v, rtol=1e-5, atol=1e-7, err_msg=n)
    for n, v in finals["dense_sum"].items():
        np.testing.assert_allclose(finals["sparse_sum"][n], v, rtol=1e-5, atol=1e-12, err_msg=n)


def test_graphed_step_equals_eager(tt, manifest):
    """GraphedTrainStep == eager steps, bit for bit, with LambdaLR changing both groups' lr; the warm-up leaves the
    accumulator untouched; the captured step has as many launches as the Adam-tables step with the same options."""
    from jodalrob_twotower_amd.graph import GraphedTrainStep
    from jodalrob_twotower_amd.optim import FusedAdam
    cfg = dict(manifest["cases"]["wide_b40"])
    cfg["B"] = 256
    batches = [synth_batch_numpy(cfg["B"], cfg["vocab_n"], cfg["vocab_c"], cfg["din_n"], cfg["din_c"], 910 + i, oob=False) for i in range(6)]
    finals, launches = {}, {}
    for mode in ("eager", "graph", "graph_adam"):
        task = make_task(tt, cfg, embedding_grad="sparse", score_dtype="bf16")
        shapes = {k: tuple(v.shape) for k, v in task.state_dict().items()}
        load_state(task, init_state_numpy(shapes, 56))
        task.train()
        task._pair_check_done = True
        kind = "adam" if mode == "graph_adam" else "rowwise_adagrad"
        kw = {} if kind == "adam" else dict(table_optimizer=kind, table_lr=0.05, table_weight_decay=1e-5)
        opt = FusedAdam.for_task(task, lr=1e-2, weight_decay=1e-5, **kw)
        sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda s: (s + 1) / 4 if s < 3 else 1.0)
        tb = [to_batch(tt, b, cfg["keys_n"], cfg["keys_c"]) for b in batches]
        losses = []
        if mode == "eager":
            for b in tb:
                opt.zero_grad()
                r = task(b, return_metrics=True)
                r["loss"].backward()
                opt.step(); sched.step()
                losses.append(r["loss"].item())
        else:
            w_before = {n: p.detach().clone() for n, p in task.named_parameters()}
            gs = GraphedTrainStep(task, opt, tb[0], warmup=3)
            launches[mode] = gs.library_launches
            if mode == "graph_adam":
                continue
            store = task.two_tower_model.embedding_store
            store = store() if callable(store) else store
            assert not opt._state_of(store)["sum"].any()              # the warm-up left no trace
            for n, p in task.named_parameters():
                assert torch.equal(p, w_before[n]), n
            for b in tb:
                r = gs.step(b)
                sched.step()
                losses.append(r["loss"].item())
            assert opt.current_step() == len(tb)
        finals[mode] = (losses, {k: v.detach().cpu().numpy().copy() for k, v in task.state_dict().items()})
    assert launches["graph"] == launches["graph_adam"], launches
    assert finals["eager"][0] == finals["graph"][0]
    for k, v in finals["eager"][1].items():
        assert np.array_equal(v, finals["graph"][1][k]), k


def test_checkpoint_round_trip_and_mismatch(tt, manifest):
    from jodalrob_twotower_amd.optim import FusedAdam
    cfg = dict(manifest["cases"]["wide_b40"])
    batches = [synth_batch_numpy(cfg["B"], cfg["vocab_n"], cfg["vocab_c"], cfg["din_n"], cfg["din_c"], 70 + i, oob=False) for i in range(4)]
    kw = dict(table_optimizer="rowwise_adagrad", lr=1e-2, weight_decay=1e-5, table_lr=0.05)

    def run(task, opt, bs):
        task.train()
        for b in bs:
            opt.zero_grad()
            task(to_batch(tt, b, cfg["keys_n"], cfg["keys_c"])).backward()
            opt.step()

    task = make_task(tt, cfg, embedding_grad="sparse")
    state = init_state_numpy({k: tuple(v.shape) for k, v in task.state_dict().items()}, 71)
    load_state(task, state)
    opt = FusedAdam.for_task(task, **kw)
    run(task, opt, batches[:2])
    buf = io.BytesIO()
    torch.save({"model": task.state_dict(), "optim": opt.state_dict()}, buf)
    sd = opt.state_dict()
    for n, p in task.named_parameters():
        if "embeddings" in n:
            s = opt.state[p]
            assert set(s) == {"step", "sum"} and tuple(s["sum"].shape) == (p.shape[0],), n
    tables = [i for g in sd["param_groups"] if g.get("table_optimizer") == "rowwise_adagrad" for i in g["params"]]
    assert tables and all(set(sd["state"][i]) == {"step", "sum"} for i in tables)
    run(task, opt, batches[2:])
    # a fresh task + optimiser from the checkpoint continues bit for bit
    buf.seek(0)
    ck = torch.load(buf, weights_only=False)
    task2 = make_task(tt, cfg, embedding_grad="sparse")
    task2.load_state_dict(ck["model"])
    opt2 = FusedAdam.for_task(task2, **kw)
    opt2.load_state_dict(ck["optim"])
    run(task2, opt2, batches[2:])
    for (n, p), (n2, p2) in zip(task.named_parameters(), task2.named_parameters()):
        assert torch.equal(p, p2), n
        if "embeddings" in n:
            assert torch.equal(opt.state[p]["sum"], opt2.state[p2]["sum"]), n
    # a state of the other table optimiser is refused, in both directions
    adam_task = make_task(tt, cfg, embedding_grad="sparse")
    load_state(adam_task, state)
    adam = FusedAdam.for_task(adam_task, lr=1e-2)
    run(adam_task, adam, batches[:1])
    with pytest.raises(ValueError, match="table_optimizer"):
        FusedAdam.for_task(make_task(tt, cfg, embedding_grad="sparse"), **kw).load_state_dict(adam.state_dict())
    with pytest.raises(ValueError, match="table_optimizer"):
        FusedAdam.for_task(make_task(tt, cfg, embedding_grad="sparse"), lr=1e-2).load_state_dict(opt.state_dict())


def test_sharded_world1_subprocess(tt):
    """Sharded store (world 1, exact and fixed-capacity exchange) == unsharded store under row-wise Adagrad; the exchange's
    pads leave the accumulator untouched; a sharded checkpoint continues bit for bit.  Own process: own process group."""
    worker = Path(__file__).resolve().parent / "_rowwise_adagrad_world1_worker.py"
    r = subprocess.run([sys.executable, str(worker)], capture_output=True, text=True, timeout=300)
    assert "ROWWISE_WORLD1_OK" in r.stdout and r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
