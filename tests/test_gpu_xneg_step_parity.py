"""One training step with shared extra negatives against the f64 oracle of tests/_xneg_step_reference.py.

A batch with batch["negatives"] is the one step whose tower sides have different row counts (notice B, company B + M), so it runs
code nothing else does: one lookup and one general duplicate-row plan per side, one tower call per side (its own dropout seed, its
own BatchNorm), company statistics over B + M rows, and a table gradient reduced once per side into the ONE store both towers
share.  test_gpu_extra_negatives.py pins the score node; here the whole step is held to the oracle: forward, one backward, one
optimiser step.

Per case (one JSON report line, visible with -s, then the assertions):
  forward    loss; the embedding blocks N, C, X; both towers' per-block BatchNorm mean / rstd (the company tower's over B + M rows,
             read through towers._DEBUG_KEEP); both towers' running statistics after the step; num_batches_tracked + 1 per tower
  gradients  every dense parameter of both towers; the tables -- dense mode: each table's .grad; sparse mode: the union of what is
             pending on the store after backward(): its row set BIT FOR BIT the oracle's (notice rows, then company rows, the row
             only an extra carries among them), its values within the bound
  optimiser  after one FusedAdam.for_task(task, lr=1e-2, weight_decay=1e-5).step(): every dense tensor and every table row (and
             their moments) against the oracle's Adam at step 1; sparse mode: rows nobody carries bitwise unchanged, EVERY touched
             notice row changed, the store's step counter 1 (not 2).  One case with table_optimizer="rowwise_adagrad".
The optimiser's reference is the oracle's update (oracle_np.adam_step / sparse_adam_rows, f32 hyper-parameters) applied to the
kernels' own gradient of this step, which the lines above have already held to the oracle's: that is the convention of
test_gpu_table_adam_parity.py, whose bounds these are.  (Fed the oracle's gradient instead, Adam's first step -lr g / (|g| + eps)
turns a gradient element whose sign differs within the gradient bound into a full 2 lr difference: a figure about the gradient,
not about the update.)  The ROWS the update is applied to are the oracle's, so a row the pending gradient misses fails here too.

Other routes to the same store: the two towers called separately (get_notice_embeddings / get_company_embeddings, two autograd
nodes, equal sides) against oracle_np.task_step; GraphedTrainStep.step with extras against the eager step bit for bit, the touched
notice rows moved; two backward passes without a step (sparse mode keeps the latest: INTEGRATION.md).

Bounds are the project's: test_gpu_logq.BOUNDS / LOSS_ATOL for the loss, test_gpu_tower_parity.TOWER_BOUNDS for everything in the
towers (bn_running_* for the running statistics, "table" for the table gradients in both layouts), test_gpu_table_adam_parity's
TRAJ_BOUNDS (one step) and ADAGRAD_FINISH_BOUND for the optimiser.
"""
import json

import numpy as np
import pytest
import torch

import oracle_np as O
from params_init import init_state_numpy
from test_gpu_dropout_parity import SEED_C, SEED_N
from test_gpu_extra_negatives import _small_task, _with_negatives
from test_gpu_logq import BOUNDS, LOSS_ATOL
from test_gpu_parity import DEV, load_state, make_task, to_batch, tt  # noqa: F401
from test_gpu_rowwise_adagrad import rowwise_adagrad_f64
from test_gpu_table_adam_parity import ADAGRAD_FINISH_BOUND, TRAJ_BOUNDS
from test_gpu_tower_parity import TOWER_BOUNDS, _acts_view, _err
import _xneg_step_reference as SR

pytestmark = pytest.mark.gpu

LR, WD = 1e-2, 1e-5
# name: (B, M, E, keys (notice, company), din, hidden, D, T) -- the smallest shapes that cross the edges of the unequal-sides path;
# "fixture" is the golden manifest's wide_b40 towers (test_gpu_mask_repeats._small_task), B + M = 103 of "ragged" is off every tile
# grid, "m_gt_b" runs the company side at 10 x the notice side, "one_extra" a single extra behind 257 rows
SHAPES = {"fixture": (64, 37, None, None, None, None, None, None),
          "ragged": (70, 33, 8, (3, 2), (100, 37), [48, 40], 33, 0.5),
          "m_gt_b": (33, 300, 32, (3, 1), (64, 128), [32, 17], 64, 1.0),
          "one_extra": (257, 1, 8, (2, 3), (50, 64), [24, 33], 64, 1.0)}
MODES = [("fp32", "fp32", "dense"), ("fp32", "fp32", "sparse"), ("bf16", "bf16", "sparse")]      # (mlp, score, embedding_grad)
SPARSE = [m for m in MODES if m[2] == "sparse"]
CASES = [(s, m, "plain", "adam") for s in SHAPES for m in MODES] + \
        [(s, m, "lq_ent", "adam") for s in ("fixture", "ragged") for m in MODES] + \
        [("ragged", m, "dropout", "adam") for m in SPARSE] + \
        [("fixture", MODES[2], "plain", "rowwise_adagrad")]
P_DROP = 0.1


def _build(tt, manifest, tmp_path, shape, mode, p=0.0, **kw):
    """(task, keys / vocabularies, state as numpy, (B, M, din)): the towers of `shape` in `mode`, parameters from
    params_init.init_state_numpy (BatchNorm scale / shift, biases and running statistics away from their symmetric spots)"""
    from jodalrob_twotower_amd import synthetic
    B, M, E, keys, din, hidden, D, T = SHAPES[shape]
    mlp, score, eg = mode
    if shape == "fixture":
        cfg = manifest["cases"]["wide_b40"]
        kn, kc, vn, vc, din, T = cfg["keys_n"], cfg["keys_c"], cfg["vocab_n"], cfg["vocab_c"], (cfg["din_n"], cfg["din_c"]), cfg["T"]
        task = make_task(tt, cfg, embedding_grad=eg, mlp_dtype=mlp, score_dtype=score, dropout_rate=p, **kw)
    else:
        kn, kc = [f"n{i}" for i in range(keys[0])], [f"c{i}" for i in range(keys[1])]
        vn, vc = [20 + 3 * i for i in range(len(kn))], [17 + 5 * i for i in range(len(kc))]
        meta = synthetic.write_metadata(tmp_path / "m.csv", {"notice": dict(zip(kn, vn)), "company": dict(zip(kc, vc))})
        task = tt.create_two_tower_train_task(kn, kc, metadata_path=str(meta), categorical_embedding_dim=E, notice_dense_input_dim=din[0],
                                              company_dense_input_dim=din[1], tower_hidden_dims=hidden, final_embedding_dim=D,
                                              dropout_rate=p, temperature=T, device=DEV, embedding_grad=eg, score_dtype=score,
                                              mlp_dtype=mlp, **kw)
    state = init_state_numpy({k: tuple(v.shape) for k, v in task.state_dict().items()}, 77)
    load_state(task, state)
    task.train()
    task._pair_check_done = True
    tn, tc = task.two_tower_model.notice_tower, task.two_tower_model.company_tower
    tn._seed_override, tc._seed_override = SEED_N, SEED_C
    return task, (kn, kc, vn, vc), state, (B, M, din, T)


def _device_batch(tt, b, kn, kc):
    """the numpy batch of _xneg_step_reference.make_batch as the task takes it"""
    t = lambda a: torch.from_numpy(a).to(DEV)
    out = to_batch(tt, b, kn, kc)
    out["negatives"] = {"dense": t(b["neg_dense"]), "kjt": tt.build_batch_kjt(torch.from_numpy(b["neg_ids"]), kc).to(DEV)}
    if "lq_n" in b:
        out["notice"].update(log_q=t(b["lq_n"]), entity=t(b["ent_n"]))
        out["company"].update(log_q=t(b["lq_c"]), entity=t(b["ent_c"]))
        out["negatives"].update(log_q=t(b["lq_x"]), entity=t(b["ent_x"]))
    return out


def _pending(store):
    """everything pending on a sparse-mode store after backward(): (rows int64 [U], gradient rows [U, E]), the entries in the
    store's order -- by their embedders' first row: the notice side's rows, then the company side's"""
    from jodalrob_twotower_amd import ops
    rows, vals = [], []
    for plan, grad_rows in store.sparse_grads():
        ops.embed_grad_finish(plan)
        U = int(plan.n_unique.item())
        rows.append(plan.unique_rows[:U].cpu().numpy().astype(np.int64))
        vals.append(grad_rows[:U].cpu().numpy())
    if not rows:
        return np.zeros(0, np.int64), np.zeros((0, store.E), np.float32)
    return np.concatenate(rows), np.concatenate(vals)


def _np(t):
    return t.detach().cpu().numpy().copy()


def _table_keys(kn, kc):
    return [f"{pre}categorical_embedder.embeddings.{k}.weight" for pre, keys in ((O.NT, kn), (O.CT, kc)) for k in keys]


def _check_adam_dense(opt, task, before, grads, report, checks, skip):
    """every dense tensor (and its moments) after the step against f64 Adam at step 1 on the kernels' gradient"""
    worst = {"p_norm": 0.0, "m_norm": 0.0, "v_norm": 0.0}
    for name, prm in task.named_parameters():
        if name in skip:
            continue
        p, m, v = SR.adam_first_step(before[name], grads[name], LR, WD)
        st = opt.state[prm]
        for k, got, ref in (("p_norm", prm, p), ("m_norm", st["exp_avg"], m), ("v_norm", st["exp_avg_sq"], v)):
            e = _err(_np(got), ref)
            worst[k] = max(worst[k], e)
            checks.append((f"adam.{name}.{k}", e <= TRAJ_BOUNDS[k]))
        checks.append((f"adam.{name}.step", float(st["step"]) == 1.0))
    report["adam_dense"] = worst


@pytest.mark.parametrize("shape,mode,variant,table_opt", CASES,
                         ids=[f"{s}-{m[0]}-{m[1]}-{m[2]}-{v}" + ("" if t == "adam" else "-" + t) for s, m, v, t in CASES])
def test_xneg_step_vs_f64_oracle(tt, manifest, tmp_path, shape, mode, variant, table_opt):
    from jodalrob_twotower_amd import towers as TW
    from jodalrob_twotower_amd.optim import FusedAdam
    mlp, score, eg = mode
    p = P_DROP if variant == "dropout" else 0.0
    task, (kn, kc, vn, vc), state, (B, M, din, T) = _build(tt, manifest, tmp_path, shape, mode, p)
    tn, tc = task.two_tower_model.notice_tower, task.two_tower_model.company_tower
    store = task.two_tower_model.embedding_store
    b = SR.make_batch(B, M, vn, vc, din[0], din[1], 610 + B + M, decorated=variant == "lq_ent")
    batch = _device_batch(tt, b, kn, kc)
    opt = FusedAdam.for_task(task, table_optimizer=table_opt, lr=LR, weight_decay=WD)
    opt.zero_grad()
    TW._DEBUG_KEEP = []
    try:
        res = task(batch, return_metrics=True)
        res["loss"].backward()
        torch.cuda.synchronize()
        keep = TW._DEBUG_KEEP
    finally:
        TW._DEBUG_KEEP = None
    assert [k["B"] for k in keep] == [B, B + M]                 # one tower pass per side, the company side over B + M rows

    # ---- the oracle: each side launched alone takes its own seed in slot 0, the company side's masks over B + M rows
    hid = tn.tower_hidden_dims[1:]
    drop = None
    if p > 0:
        drop = (p, {(pre, i): O.dropout_keep(seed, 0, i, rows, H, p) for pre, seed, rows in ((O.NT, SEED_N, B), (O.CT, SEED_C, B + M))
                    for i, H in enumerate(hid)})
    ref = SR.xneg_step(state, b, kn, kc, vn, vc, T, score, "bf16" if mlp == "bf16" else None, drop)
    bd = TOWER_BOUNDS[mlp]
    report = {"shape": shape, "B": B, "M": M, "mode": list(mode), "variant": variant, "table_optimizer": table_opt}
    checks = []

    def chk(tag, e, bound):
        report[tag] = e
        checks.append((tag, e <= bound))

    # ---- forward
    loss = res["loss"].item()
    report["loss"] = abs(loss - ref["loss"]) / abs(ref["loss"])
    checks.append(("loss", abs(loss - ref["loss"]) <= BOUNDS[score][0] * abs(ref["loss"]) + LOSS_ATOL))
    cx = _np(keep[1]["emb"])
    for name, got in (("N", _np(keep[0]["emb"])), ("C", cx[:B]), ("X", cx[B:])):
        e = (_err(got, ref[name]), float(np.abs(got - ref[name]).max()))
        report["emb." + name] = e
        checks.append(("emb." + name, e[0] <= bd["emb_norm"] and e[1] <= bd["emb_maxabs"]))
    for side, tw, k, cache in (("notice", tn, keep[0], ref["cache_n"]), ("company", tc, keep[1], ref["cache_c"])):
        view = _acts_view(tw, k)
        for i, (mean, rstd) in enumerate(SR.block_stats(cache)):
            chk(f"{side}.block{i}.mean", _err(view["blocks"][i]["mean"], mean), bd["mean"])
            chk(f"{side}.block{i}.rstd", _err(view["blocks"][i]["rstd"], rstd), bd["rstd"])
    after_bwd = {k: _np(v) for k, v in task.state_dict().items()}
    assert len(ref["bn_updates"]) == 6 * len(hid)
    for k, want in ref["bn_updates"].items():
        if k.endswith("num_batches_tracked"):
            checks.append((k, int(after_bwd[k]) == int(state[k]) + 1 == int(want)))
        else:
            chk(k, _err(after_bwd[k], want), bd["bn_" + k.rsplit(".", 1)[1]])

    # ---- gradients
    tables = _table_keys(kn, kc)
    grads = {}
    for name, prm in task.named_parameters():
        if name in tables:
            continue
        grads[name] = _np(prm.grad)
        chk("grad." + name, _err(grads[name], ref["grads"][name]), bd["grad_matrix" if prm.ndim > 1 else "grad_vector"])
    rn, gn, rc, gc = ref["rows"]
    want_rows = np.concatenate([rn, rc])
    R = sum(vn) + sum(vc)
    only_extra, nobody = sum(vn) + vc[0] - 2, np.setdiff1d(np.arange(R), want_rows)
    assert only_extra in rc and vc[0] - 2 not in b["company_ids"][:, 0] and len(rn) >= 2 and len(nobody) >= 3
    assert len(rc) < (B + M) * len(kc)                          # companies repeat each other / extras repeat batch companies
    if eg == "dense":
        for name in tables:
            grads[name] = _np(dict(task.named_parameters())[name].grad)
            chk("grad." + name, _err(grads[name], ref["grads"][name]), bd["table"])
    else:
        got_rows, got_vals = _pending(store)
        report["rows_equal"] = bool(np.array_equal(got_rows, want_rows))
        report["pending_rows"] = [int(len(got_rows)), int(len(want_rows)), int(len(rn))]
        checks.append(("rows_equal", report["rows_equal"]))
        if report["rows_equal"]:
            chk("table.notice_rows", _err(got_vals[:len(rn)], gn), bd["table"])
            chk("table.company_rows", _err(got_vals[len(rn):], gc), bd["table"])
        # the gradient the optimiser's reference is fed: the kernels' own wherever the pending entries hold the row
        fed = np.concatenate([gn, gc])
        at = {int(r): i for i, r in enumerate(got_rows)}
        for i, r in enumerate(want_rows):
            if int(r) in at:
                fed[i] = got_vals[at[int(r)]]

    # ---- one optimiser step
    table0 = _np(store.weight)
    opt.step()
    torch.cuda.synchronize()
    _check_adam_dense(opt, task, state, grads, report, checks, set(tables) if (eg == "sparse" or table_opt != "adam") else set())
    table1 = _np(store.weight)
    sst = opt._store_state[id(store)]
    report["store_step"] = int(sst["step"])
    checks.append(("store_step", int(sst["step"]) == 1))
    checks += [("table_param_step." + n, float(opt.state[dict(task.named_parameters())[n]]["step"]) == 1.0) for n in tables]
    if eg == "sparse":
        rows = want_rows
        if table_opt == "adam":
            t, m, v = SR.sparse_adam_first_step(table0, rows, fed, LR, WD)
            for k, got, want in (("p_norm", table1, t), ("m_norm", _np(sst["m"]), m), ("v_norm", _np(sst["v"]), v)):
                chk("adam_rows." + k, _err(got[rows], want[rows]), TRAJ_BOUNDS[k])
        else:
            w, s = table0[rows].astype(np.float64), np.zeros(len(rows))
            gp = fed + SR.f32(WD) * w
            rowwise_adagrad_f64(w, fed.astype(np.float64), s, SR.f32(LR), SR.f32(1e-8), SR.f32(WD))
            size = np.abs(SR.f32(LR) / (np.sqrt(s) + SR.f32(1e-8)))[:, None] * np.abs(gp)
            chk("adagrad_rows.w", float((np.abs(table1[rows] - w) / (np.abs(w) + size)).max()), ADAGRAD_FINISH_BOUND)
            chk("adagrad_rows.s", float((np.abs(_np(sst["sum"])[rows] - s) / s).max()), ADAGRAD_FINISH_BOUND)
        report["rows_nobody_unchanged"] = bool(np.array_equal(table1[nobody].view(np.uint32), table0[nobody].view(np.uint32)))
        moved = np.any(table1[rn] != table0[rn], axis=1)
        report["notice_rows_moved"] = [int(moved.sum()), int(len(rn))]
        report["only_extra_row_moved"] = bool(np.any(table1[only_extra] != table0[only_extra]))
        checks += [("rows_nobody_unchanged", report["rows_nobody_unchanged"]), ("notice_rows_moved", bool(moved.all())),
                   ("only_extra_row_moved", report["only_extra_row_moved"])]
    print("\n[xneg step vs f64 oracle]", json.dumps(report))
    bad = [tag for tag, ok in checks if not ok]
    assert not bad, (bad, report)


@pytest.mark.parametrize("mode", SPARSE, ids=lambda m: f"{m[0]}-{m[1]}")
def test_separate_tower_calls_reach_the_optimiser(tt, manifest, tmp_path, mode):
    """get_notice_embeddings and get_company_embeddings called separately (two autograd nodes on the one store), equal sides, then
    the score node and ONE backward: table gradients and one Adam step against plain oracle_np.task_step"""
    from jodalrob_twotower_amd.optim import FusedAdam
    from jodalrob_twotower_amd.two_tower_train_task import _ScoreCEFn
    mlp, score, eg = mode
    task, (kn, kc, vn, vc), state, (B, M, din, T) = _build(tt, manifest, tmp_path, "fixture", mode)
    model, store = task.two_tower_model, task.two_tower_model.embedding_store
    b = SR.make_batch(B, M, vn, vc, din[0], din[1], 611)
    batch = to_batch(tt, b, kn, kc)
    opt = FusedAdam.for_task(task, lr=LR, weight_decay=WD)
    opt.zero_grad()
    ne, ce = model.get_notice_embeddings(batch["notice"]), model.get_company_embeddings(batch["company"])
    loss, _, _ = _ScoreCEFn.apply(ne, ce, 1.0 / float(T), score, False, False)
    loss.backward()
    torch.cuda.synchronize()
    ref = O.task_step(state, b, kn, kc, vn, vc, T, True, dtype=np.float64, rounding="bf16" if mlp == "bf16" else None, table_grads="none")
    offs_n, offs_c = SR.fused_offsets(vn, vc)
    E = store.E
    rn, gn = O.embed_grad_sparse(ref["d_concat_notice"], ref["ids_notice"], offs_n, E)
    rc, gc = O.embed_grad_sparse(ref["d_concat_company"], ref["ids_company"], offs_c, E)
    want_rows, bd = np.concatenate([rn, rc]), TOWER_BOUNDS[mlp]
    got_rows, got_vals = _pending(store)
    report = {"mode": list(mode), "loss": abs(loss.item() - ref["loss"]) / abs(ref["loss"]),
              "rows_equal": bool(np.array_equal(got_rows, want_rows)), "pending_rows": [int(len(got_rows)), int(len(want_rows)), int(len(rn))]}
    checks = [("loss", abs(loss.item() - ref["loss"]) <= BOUNDS[score][0] * abs(ref["loss"]) + LOSS_ATOL), ("rows_equal", report["rows_equal"])]
    grads = {}
    for name, prm in task.named_parameters():
        if "categorical_embedder" not in name:
            grads[name] = _np(prm.grad)
            report["grad." + name] = _err(grads[name], ref["grads"][name])
            checks.append(("grad." + name, report["grad." + name] <= bd["grad_matrix" if prm.ndim > 1 else "grad_vector"]))
    fed = np.concatenate([gn, gc])
    if report["rows_equal"]:
        report["table.notice_rows"], report["table.company_rows"] = _err(got_vals[:len(rn)], gn), _err(got_vals[len(rn):], gc)
        checks += [("table.notice_rows", report["table.notice_rows"] <= bd["table"]), ("table.company_rows", report["table.company_rows"] <= bd["table"])]
        fed = got_vals
    table0 = _np(store.weight)
    opt.step()
    torch.cuda.synchronize()
    _check_adam_dense(opt, task, state, grads, report, checks, set(_table_keys(kn, kc)))
    table1, sst = _np(store.weight), opt._store_state[id(store)]
    t, m, v = SR.sparse_adam_first_step(table0, want_rows, fed, LR, WD)
    for k, got, want in (("p_norm", table1, t), ("m_norm", _np(sst["m"]), m), ("v_norm", _np(sst["v"]), v)):
        report["adam_rows." + k] = _err(got[want_rows], want[want_rows])
        checks.append(("adam_rows." + k, report["adam_rows." + k] <= TRAJ_BOUNDS[k]))
    nobody = np.setdiff1d(np.arange(table0.shape[0]), want_rows)
    moved = np.any(table1[rn] != table0[rn], axis=1)
    report["notice_rows_moved"] = [int(moved.sum()), int(len(rn))]
    checks += [("store_step", int(sst["step"]) == 1), ("notice_rows_moved", bool(moved.all())),
               ("rows_nobody_unchanged", bool(np.array_equal(table1[nobody].view(np.uint32), table0[nobody].view(np.uint32))))]
    print("\n[separate tower calls vs f64 oracle]", json.dumps(report))
    bad = [tag for tag, ok in checks if not ok]
    assert not bad, (bad, report)


def test_xneg_graphed_step_moves_the_notice_rows(tt, manifest):
    """GraphedTrainStep.step with extras, sparse tables: after two steps every table row equals the eager run's bit for bit AND the
    notice rows the batches carry differ from their initial values"""
    from jodalrob_twotower_amd.graph import GraphedTrainStep
    from jodalrob_twotower_amd.optim import FusedAdam
    finals = {}
    for leg in ("eager", "graph"):
        task, b, B = _small_task(tt, manifest, score_dtype="bf16")
        emb = task.two_tower_model.notice_tower.categorical_embedder
        store = task.two_tower_model.embedding_store
        K = len(emb.keys)
        carried = torch.unique((b["notice"]["kjt"].values().view(B, K).clamp(min=0).minimum(emb._key_vocab - 1) + emb._key_row_offset).reshape(-1))
        before = store.weight.detach().clone()
        bs = [_with_negatives(b, 37, 30 + k) for k in range(2)]
        opt = FusedAdam.for_task(task, lr=LR, weight_decay=WD)
        gs = GraphedTrainStep(task, opt, bs[0], warmup=1) if leg == "graph" else None
        assert torch.equal(store.weight, before)                 # (the warm-up leaves no trace)
        for bk in bs:
            if gs is None:
                opt.zero_grad()
                task(bk).backward()
                opt.step()
            else:
                gs.step(bk)
        torch.cuda.synchronize()
        if gs is not None:
            gs.close()
        after = store.weight.detach().clone()
        assert len(carried) >= 2 and bool((after[carried] != before[carried]).any(dim=1).all()), leg
        assert opt.current_step() == 2
        finals[leg] = after
    assert torch.equal(finals["eager"], finals["graph"])


def test_sparse_store_keeps_the_latest_backward(tt, manifest):
    """two backward passes without a step, sparse tables, equal sides: the pending gradient is the second batch's, for both towers
    (sparse mode does not accumulate across backward passes: INTEGRATION.md)"""
    task, b, B = _small_task(tt, manifest, score_dtype="bf16")
    store = task.two_tower_model.embedding_store
    g = torch.Generator(device=DEV).manual_seed(5)
    perm = torch.randperm(B, generator=g, device=DEV)
    from jodalrob_twotower_amd.kjt import KeyedJaggedTensor
    b2 = {}
    for side in ("notice", "company"):
        K = len(b[side]["kjt"].keys())
        ids2 = b[side]["kjt"].values().view(B, K)[perm].clone()
        ids2[0] = ids2[1]                                        # (another row set than b's, not only another order)
        b2[side] = {"dense": b[side]["dense"][perm] + 0.5, "kjt": KeyedJaggedTensor(b[side]["kjt"].keys(), ids2.reshape(-1))}
    task(b).backward()
    first = _pending(store)
    task(b2).backward()
    torch.cuda.synchronize()
    assert len(store.sparse_grads()) == 1 and store.sparse_grad is not None
    both = _pending(store)
    task.zero_grad(set_to_none=True)
    store.sparse_grad = None
    task(b2).backward()
    torch.cuda.synchronize()
    alone = _pending(store)
    n_rows = task.two_tower_model.company_tower.categorical_embedder.row_base
    assert (both[0] < n_rows).any() and (both[0] >= n_rows).any()            # both towers' rows
    assert np.array_equal(both[0], alone[0]) and np.array_equal(both[1].view(np.uint32), alone[1].view(np.uint32))
    assert not (np.array_equal(first[0], both[0]) and np.array_equal(first[1], both[1]))
