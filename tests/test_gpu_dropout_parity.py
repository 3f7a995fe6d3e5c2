"""The training step with dropout on -- bench.py's and scripts/train.py's setting (dropout_rate = 0.1) -- against the f64 oracle
that models the kernels' mask (oracle_np.dropout_keep: the counter-based hash of csrc/tt_common.h over (seed, salt + row * H +
column), salt = ((i + 1) << 40) ^ (t << 52) + rng_row_offset * H).  The mask is never stored: every forward and backward kernel
rebuilds it, so these tests read it off the kernels' outputs and check it against the restatement, then feed the restated masks
to the oracle.

a. Mask pin: each hidden block's activation buffer of a dropout step against the same batch at p = 0, bit for bit.
b. One step against the f64 oracle with the kernels' masks: loss, embeddings, metrics, every dense gradient, the sparse rows,
   the BatchNorm running statistics -- on every tower path (front + fused tail, wide tail, general bf16, fp32, two blocks).
c. Captured steps: each replay's masks are the eager step's at seed = host seed + that replay's device word.
d. Eval mode with dropout_rate > 0 against the oracle's eval forward on the kernels' running statistics.

Which tower slot and seed a block's mask uses follows the launch: both towers in one batched call (same batch size, block count
and dropout setting) share the notice tower's seed, notice in slot t = 0 and company in t = 1; a tower launched alone uses its own
seed in slot 0.  The towers here get different seeds, so the pin would fail if a shape took the other form than predicted.

Each case prints one JSON report line (visible with -s), then asserts.  Bounds quote what an MI355X measured.
"""
import json

import numpy as np
import pytest
import torch

import oracle_np as O
from params_init import init_state_numpy, synth_batch_numpy
from test_gpu_parity import BF16_VS_REFERENCE_BOUNDS, DEV, _rel, load_state, make_task, to_batch, tt  # noqa: F401

pytestmark = pytest.mark.gpu

SEED_N, SEED_C = 0x5DEECE66D, 0xB5297A4D3F    # notice / company tower seeds (different: see the module docstring)
M64 = (1 << 64) - 1

# Bounds of the dropout step against the f64 oracle fed the kernels' masks (bf16: rounding="bf16"; fp32: rounding=None), each at
# most 4x the worst figure an MI355X measured over CASES (in brackets).  bf16: the two-block towers ([128, 128, 64]) carry the
# largest figures -- one more rounded Linear than the p = 0 table (test_gpu_parity.BF16_STEP_BOUNDS) was measured on.
DROPOUT_STEP_BOUNDS = {
    "bf16": {"loss_rtol": 1e-6,                      # (2.5e-7, two blocks)
             "emb_norm": 4e-4, "emb_maxabs": 3e-3,   # (1.2e-4 / 9.2e-4, two blocks)
             "metric_atol": 5e-6,                    # (1.3e-6)
             "dense_grad_matrix_norm": 3e-3,         # (9.2e-4)
             "dense_grad_vector_norm": 3e-3,         # (9.2e-4)
             "row_grad_norm": 2.5e-3,                # (7.4e-4); row SET bit-exact
             "bn_running_mean": 6e-6,                # norm-wise per tensor (1.6e-6)
             "bn_running_var": 2.5e-7},              # (6.3e-8)
    "fp32": {"loss_rtol": 4e-7,                      # (1.2e-7, B = 8192)
             "emb_norm": 3.5e-6, "emb_maxabs": 3.4e-6,   # (9.4e-7 / 8.6e-7)
             "metric_atol": 6e-9,                    # (1.7e-9)
             "dense_grad_matrix_norm": 7e-6,         # (1.9e-6)
             "dense_grad_vector_norm": 3e-5,         # (7.6e-6)
             "table_grad_norm": 7e-6,                # (1.8e-6)
             "bn_running_mean": 3.5e-7,              # (8.9e-8)
             "bn_running_var": 1.4e-7},              # (3.7e-8)
}
# bf16 at the bench shape against the UNROUNDED oracle (the reference's arithmetic): test_gpu_parity.BF16_VS_REFERENCE_BOUNDS holds
# (measured: loss 8.6e-7; embeddings 3.7e-3 / 2.8e-3; metrics 3.2e-5; weights 4.4e-2; vectors 9.3e-2; rows 4.4e-2)
PIN_KEPT_MAXREL = 3.5e-7       # blocks behind a dropped block: kept values against f32 BN output x scale (9.4e-8)
EVAL_BOUNDS = {"bf16": {"emb_norm": 7e-5, "emb_maxabs": 5e-4},    # (1.9e-5 / 1.2e-4, two blocks)
               "fp32": {"emb_norm": 1.5e-6, "emb_maxabs": 9e-7}}  # (4.0e-7 / 2.5e-7)


def _print(tag, report):
    print(f"\n[{tag}]", json.dumps(report))


def _towers(task):
    return task.two_tower_model.notice_tower, task.two_tower_model.company_tower


def _rng_slots(task, B):
    """{tower prefix: (seed, slot t)} as the launch takes them (towers.py _TowersFn: one batched call when the towers agree on the
    batch size, the number of hidden blocks and (train, p); else one call per tower with its own seed in slot 0)"""
    tn, tc = _towers(task)
    batched = tn.n_hidden == tc.n_hidden and tn.training == tc.training and tn.dropout_rate == tc.dropout_rate
    if batched:
        return {O.NT: (tn._seed_override, 0), O.CT: (tn._seed_override, 1)}, True
    return {O.NT: (tn._seed_override, 0), O.CT: (tc._seed_override, 0)}, False


def _masks(task, B, p, word=0):
    slots, _ = _rng_slots(task, B)
    hid = task.two_tower_model.notice_tower.tower_hidden_dims[1:]
    return {(pre, i): O.dropout_keep((seed + word) & M64, t, i, B, H, p) for pre, (seed, t) in slots.items() for i, H in enumerate(hid)}


def _build(tt, schema_real, tmp_path, rows_per_tower, hidden, D, T, mlp, p):
    from jodalrob_twotower_amd import synthetic
    kn, kc = schema_real["notice"]["categorical"], schema_real["company"]["categorical"]
    vn, vc = schema_real["notice"]["vocab_sizes"], schema_real["company"]["vocab_sizes"]
    if rows_per_tower:
        vn, vc = synthetic.scale_vocabs(vn, rows_per_tower), synthetic.scale_vocabs(vc, rows_per_tower)
    meta = synthetic.write_metadata(tmp_path / "m.csv", {"notice": dict(zip(kn, vn)), "company": dict(zip(kc, vc))})
    torch.manual_seed(2718)
    task = tt.create_two_tower_train_task(kn, kc, metadata_path=str(meta), categorical_embedding_dim=32, notice_dense_input_dim=256,
                                          company_dense_input_dim=128, tower_hidden_dims=hidden, final_embedding_dim=D,
                                          dropout_rate=p, temperature=T, device=DEV, embedding_grad="sparse",
                                          score_dtype="bf16" if mlp == "bf16" else "fp32", mlp_dtype=mlp)
    task.train()
    task._pair_check_done = True
    with torch.no_grad():                       # BN scale / shift and biases away from the init's symmetric spots
        g = torch.Generator(device=DEV).manual_seed(79)
        for prm in task.parameters():
            if prm.ndim == 1:
                prm.add_(0.1 * torch.randn(prm.shape, generator=g, device=DEV))
    tn, tc = _towers(task)
    tn._seed_override, tc._seed_override = SEED_N, SEED_C
    return task, (kn, kc, vn, vc)


def _run(task, batch):
    """one step (forward + backward); returns the per-tower buffers: emb [B, D] and, per hidden block, pre / act [B, H] and
    mean / rstd [H] (the flat activation buffer of towers.py: x | (pre_i, act_i)* | (mean_i, rstd_i)* | y)"""
    from jodalrob_twotower_amd import towers as TW
    TW._DEBUG_KEEP = []
    try:
        res = task(batch, return_metrics=True)
        res["loss"].backward()
        torch.cuda.synchronize()
        keep = TW._DEBUG_KEEP
    finally:
        TW._DEBUG_KEEP = None
    assert len(keep) == 2
    out = {}
    for pre, tw, k in zip((O.NT, O.CT), _towers(task), keep):
        B, hid = k["B"], list(k["hidden"])
        sizes = [TW._al(B * tw.x_width) if tw.x_dtype == torch.float32 else 0] + [TW._al(B * h) for h in hid for _ in (0, 1)] + \
            [TW._al(h) for h in hid for _ in (0, 1)]
        offs = np.concatenate([[0], np.cumsum(sizes)])
        nh = len(hid)
        buf = k["acts"].detach().cpu().numpy()
        blocks = []
        for i, H in enumerate(hid):
            blocks.append({"pre": buf[offs[1 + 2 * i]:offs[1 + 2 * i] + B * H].reshape(B, H),
                           "act": buf[offs[2 + 2 * i]:offs[2 + 2 * i] + B * H].reshape(B, H),
                           "mean": buf[offs[1 + 2 * nh + 2 * i]:offs[1 + 2 * nh + 2 * i] + H],
                           "rstd": buf[offs[2 + 2 * nh + 2 * i]:offs[2 + 2 * nh + 2 * i] + H]})
        out[pre] = {"emb": k["emb"].detach().cpu().numpy().copy(), "blocks": blocks}
    return res, out


def _np_batch(batch, B, kn, kc):
    return {"notice_ids": batch["notice"]["kjt"].values().cpu().numpy().reshape(B, len(kn)),
            "company_ids": batch["company"]["kjt"].values().cpu().numpy().reshape(B, len(kc)),
            "notice_dense": batch["notice"]["dense"].cpu().numpy(), "company_dense": batch["company"]["dense"].cpu().numpy()}


# (rows per tower, mlp, hidden, D, B, p, T, the tower path): hidden lists the projection width first (the reference's convention)
CASES = [
    (1_000_000, "bf16", [128, 64], 64, 8192, 0.1, 1.0, "front+fused tail (bench step)"),
    (None, "bf16", [128, 64], 64, 1000, 0.3, 0.5, "front+fused tail, ragged"),
    (None, "bf16", [512, 256], 128, 2240, 0.1, 1.0, "wide tail"),
    (None, "bf16", [256, 128], 256, 4097, 0.1, 0.7, "general bf16"),
    (None, "bf16", [128, 128, 64], 64, 2048, 0.2, 1.0, "bn_apply block + fused tail"),
    (1_000_000, "fp32", [128, 64], 64, 8192, 0.1, 1.0, "fp32 (bench shape)"),
    (None, "fp32", [256, 128, 96], 64, 4097, 0.5, 0.5, "fp32, two blocks, ragged"),
]
IDS = [f"{c[1]}-{'-'.join(map(str, c[2]))}-{c[3]}-B{c[4]}-p{c[5]}" for c in CASES]


@pytest.mark.parametrize("rows_per_tower,mlp,hidden,D,B,p,T,path", CASES, ids=IDS)
def test_dropout_mask_pin(tt, schema_real, tmp_path, rows_per_tower, mlp, hidden, D, B, p, T, path):
    """a. The first hidden block sees the same input at p and at p = 0, so its BN statistics agree and, bit for bit,
    act_p == where(keep, f32(act_0 * scale), 0) with keep the restated mask and scale = f32(1) / (f32(1) - f32(p)).  Deeper
    blocks see dropped inputs: there the zero pattern of act_p is exactly ~keep and the kept values are the BN output of the
    dropout run's own statistics times the scale."""
    from jodalrob_twotower_amd import synthetic
    task, (kn, kc, vn, vc) = _build(tt, schema_real, tmp_path, rows_per_tower, hidden, D, T, mlp, p)
    batch = synthetic.make_batch(B, vn, vc, kn, kc, 256, 128, torch.device(DEV), seed=B + 11)
    _, got_p = _run(task, batch)
    for tw in _towers(task):
        tw.dropout_rate = 0.0
    _, got_0 = _run(task, batch)
    state = {k: v.detach().cpu().numpy() for k, v in task.state_dict().items()}
    masks = _masks(task, B, p)             # (the slots of the dropout call: dropout_rate is the same on both towers either way)
    _, batched = _rng_slots(task, B)
    scale = O.dropout_scale(p)
    report = {"path": path, "mlp": mlp, "hidden": hidden, "B": B, "p": p, "batched": batched}
    checks = []
    for pre in (O.NT, O.CT):
        for i, blk in enumerate(got_p[pre]["blocks"]):
            keep, a_p = masks[(pre, i)], blk["act"]
            tag = f"{'notice' if pre == O.NT else 'company'}.{i}"
            report[tag + ".kept"] = round(float(keep.mean()), 5)
            if i == 0:
                b0 = got_0[pre]["blocks"][0]
                assert np.array_equal(blk["mean"], b0["mean"]) and np.array_equal(blk["rstd"], b0["rstd"]), tag
                want = b0["act"] * np.where(keep, scale, np.float32(0))          # f32(y * s): a dropped negative y is -0
                assert want.dtype == np.float32
                bad = int(np.count_nonzero(a_p.view(np.uint32) != want.view(np.uint32)))
                report[tag + ".bits_differ"] = bad
                checks.append((tag, bad == 0))
            else:
                g, b = state[f"{pre}mlp.{4 * i + 2}.weight"], state[f"{pre}mlp.{4 * i + 2}.bias"]
                y = ((np.maximum(blk["pre"], 0) - blk["mean"]) * blk["rstd"] * g + b).astype(np.float32)
                assert np.all(y != 0), tag
                zeros_ok = bool(np.array_equal(a_p == 0, ~keep))
                err = float(np.abs(a_p[keep] - y[keep] * scale).max() / np.abs(y[keep] * scale).max())
                report[tag + ".zeros_exact"], report[tag + ".kept_maxrel"] = zeros_ok, err
                checks.append((tag, zeros_ok and err <= PIN_KEPT_MAXREL))
    _print("dropout mask pin", report)
    for tag, ok in checks:
        assert ok, (tag, report)


def _bn_report(task, ref, report):
    worst = {"running_mean": 0.0, "running_var": 0.0}
    for k, v in task.state_dict().items():
        if k in ref["bn_updates"]:
            got, want = v.cpu().numpy(), ref["bn_updates"][k]
            if k.endswith("num_batches_tracked"):
                assert int(got) == int(want), k
            else:
                kind = k.rsplit(".", 1)[1]
                worst[kind] = max(worst[kind], _rel(got, want))
    report["bn_running_mean"], report["bn_running_var"] = worst["running_mean"], worst["running_var"]


def _step_report(task, res, got, ref, B, vn, vc, report):
    report["loss"] = abs(res["loss"].item() - ref["loss"]) / abs(ref["loss"])
    for name, pre in (("notice_emb", O.NT), ("company_emb", O.CT)):
        report[name] = (_rel(got[pre]["emb"], ref[name]), float(np.abs(got[pre]["emb"] - ref[name]).max()))
    for k in ("positive_similarity_mean", "negative_similarity_mean", "similarity_gap", "accuracy"):
        report[k] = abs(res[k].item() - float(ref[k]))
    mat, vec = [], []
    for n_, prm in task.named_parameters():
        if "categorical_embedder" not in n_:
            report[n_] = _rel(prm.grad.cpu().numpy(), ref["grads"][n_])
            (vec if prm.ndim == 1 else mat).append(n_)
    store = task.two_tower_model.embedding_store
    store = store() if callable(store) else store
    plan, grad_rows = store.sparse_grad
    U = int(plan.n_unique.item())
    got_rows, got_grad = plan.unique_rows[:U].cpu().numpy().astype(np.int64), grad_rows[:U].cpu().numpy()
    offs_n = np.cumsum([0] + list(vn[:-1]))
    offs_c = sum(vn) + np.cumsum([0] + list(vc[:-1]))
    rn, gn = O.embed_grad_sparse(ref["d_concat_notice"], ref["ids_notice"], offs_n, 32)
    rc, gc = O.embed_grad_sparse(ref["d_concat_company"], ref["ids_company"], offs_c, 32)
    report["table_rows_exact"] = bool(np.array_equal(got_rows, np.concatenate([rn, rc])))
    report["table_grads"] = _rel(got_grad, np.concatenate([gn, gc])) if report["table_rows_exact"] else float("inf")
    return mat, vec


def _assert_report(report, mat, vec, B, bd):
    assert report["loss"] <= bd["loss_rtol"], report
    for name in ("notice_emb", "company_emb"):
        assert report[name][0] <= bd["emb_norm"] and report[name][1] <= bd["emb_maxabs"], (name, report[name])
    for k in ("positive_similarity_mean", "negative_similarity_mean", "similarity_gap"):
        assert report[k] <= bd["metric_atol"], (k, report[k])
    assert report["accuracy"] <= 2.0 / B, report["accuracy"]
    for n_ in mat:
        assert report[n_] <= bd["dense_grad_matrix_norm"], (n_, report[n_])
    for n_ in vec:
        assert report[n_] <= bd["dense_grad_vector_norm"], (n_, report[n_])
    assert report["table_rows_exact"], report
    assert report["table_grads"] <= bd.get("row_grad_norm", bd.get("table_grad_norm")), report["table_grads"]


@pytest.mark.parametrize("rows_per_tower,mlp,hidden,D,B,p,T,path", CASES, ids=IDS)
def test_dropout_step_vs_f64_oracle(tt, schema_real, tmp_path, rows_per_tower, mlp, hidden, D, B, p, T, path):
    """b. One dropout step against the f64 oracle fed the restated masks (pinned by test_dropout_mask_pin): loss, both towers'
    embeddings, the metrics, every dense gradient, the sparse row set (bit-exact) and row gradients, and the BatchNorm running
    mean / variance / num_batches_tracked (statistics before dropout).  bf16 against rounding="bf16"; its distance from the
    unrounded oracle (the reference's arithmetic) is printed too, and bounded at the bench shape."""
    from jodalrob_twotower_amd import synthetic
    task, (kn, kc, vn, vc) = _build(tt, schema_real, tmp_path, rows_per_tower, hidden, D, T, mlp, p)
    state = {k: v.detach().cpu().numpy().copy() for k, v in task.state_dict().items()}
    batch = synthetic.make_batch(B, vn, vc, kn, kc, 256, 128, torch.device(DEV), seed=B + 13)
    res, got = _run(task, batch)
    b = _np_batch(batch, B, kn, kc)
    masks = _masks(task, B, p)
    rounding = "bf16" if mlp == "bf16" else None
    # the one-launch first-block backward (B a multiple of 64, narrow first block) forms the projection gradients factored
    proj = "factored" if (mlp == "bf16" and B % 64 == 0 and (hidden[1] // 64) * hidden[0] <= 256) else "direct"
    ref = O.task_step(state, b, kn, kc, vn, vc, T, True, dtype=np.float64, rounding=rounding, table_grads="none", keep_sim=False,
                      proj_grad=proj, dropout=(p, masks))
    report = {"path": path, "mlp": mlp, "hidden": hidden, "D": D, "B": B, "p": p}
    mat, vec = _step_report(task, res, got, ref, B, vn, vc, report)
    _bn_report(task, ref, report)
    _print(f"dropout step vs f64 oracle ({'rounded' if rounding else 'unrounded'})", report)
    plain = None
    if mlp == "bf16":
        ref0 = O.task_step(state, b, kn, kc, vn, vc, T, True, dtype=np.float64, rounding=None, table_grads="none", keep_sim=False,
                           dropout=(p, masks))
        plain = {"path": path, "B": B}
        _step_report(task, res, got, ref0, B, vn, vc, plain)
        _print("dropout step vs unrounded f64 oracle", plain)
    bd = DROPOUT_STEP_BOUNDS[mlp]
    _assert_report(report, mat, vec, B, bd)
    assert report["bn_running_mean"] <= bd["bn_running_mean"], report
    assert report["bn_running_var"] <= bd["bn_running_var"], report
    if plain is not None and rows_per_tower:
        _assert_report(plain, mat, vec, B, BF16_VS_REFERENCE_BOUNDS)


def test_dropout_graph_replays_use_seed_word(tt, manifest):
    """c. GraphedTrainStep (FusedAdam, bf16, p = 0.1; towers [64, 64, 32] -> 32: block 0 on bn_apply / colsum_partial /
    bn_bwd_apply inside the graph, block 1 on the fused tail): after each of 3 replays, the same step run eagerly on a twin task
    whose seed is the captured host seed plus the replay's device word (mod 2^64) gives the same loss and the same parameters
    and Adam moments, bit for bit; consecutive replays draw different masks."""
    from jodalrob_twotower_amd.graph import GraphedTrainStep
    from jodalrob_twotower_amd.optim import FusedAdam
    cfg = dict(manifest["cases"]["wide_b40"])
    cfg.update(hidden=[64, 64, 32], D=32, B=256)
    base = (1 << 64) - 12345                           # a host seed near 2^64: seed + word wraps
    batches = [synth_batch_numpy(cfg["B"], cfg["vocab_n"], cfg["vocab_c"], cfg["din_n"], cfg["din_c"], 3100 + i, oob=True) for i in range(3)]
    tasks, opts = [], []
    for _ in range(2):
        task = make_task(tt, cfg, embedding_grad="sparse", score_dtype="bf16", mlp_dtype="bf16", dropout_rate=0.1)
        load_state(task, init_state_numpy({k: tuple(v.shape) for k, v in task.state_dict().items()}, 58))
        task.train()
        task._pair_check_done = True
        for tw in _towers(task):
            tw._seed_override = base
        tasks.append(task)
        opts.append(FusedAdam.for_task(task, lr=1e-2, weight_decay=1e-5))
    tb = [to_batch(tt, b, cfg["keys_n"], cfg["keys_c"]) for b in batches]
    gs = GraphedTrainStep(tasks[0], opts[0], tb[0], warmup=2)
    twin, topt = tasks[1], opts[1]
    words, report = [], {"replays": []}
    try:
        for i, b in enumerate(tb):
            torch.manual_seed(500 + i)
            lg = gs.step(b)["loss"].item()
            torch.cuda.synchronize()
            word = int(gs._seed_dev.item()) & M64
            words.append(word)
            for tw in _towers(twin):
                tw._seed_override = (base + word) & M64
            topt.zero_grad()
            r = twin(b, return_metrics=True)
            r["loss"].backward()
            topt.step()
            torch.cuda.synchronize()
            le = r["loss"].item()
            sd_g, sd_e = tasks[0].state_dict(), twin.state_dict()
            diff = [k for k in sd_g if not torch.equal(sd_g[k], sd_e[k])]
            for (pg, pe) in zip(tasks[0].parameters(), twin.parameters()):
                sg, se = opts[0].state.get(pg) or {}, topt.state.get(pe) or {}
                for key in ("exp_avg", "exp_avg_sq"):
                    if key in sg and not torch.equal(sg[key], se[key]):
                        diff.append(key)
            for sg_, se_ in zip(opts[0]._stores, topt._stores):
                a, c = opts[0]._state_of(sg_), topt._state_of(se_)
                for key in ("m", "v"):
                    if not torch.equal(a[key], c[key]):
                        diff.append("store." + key)
            report["replays"].append({"word": hex(word), "loss_graph": lg, "loss_eager": le, "differ": diff[:8]})
            assert lg == le and not diff, report
    finally:
        gs.close()
    _print("dropout graph replays", report)
    assert len(set(words)) == 3
    masks = [O.dropout_keep((base + w) & M64, 0, 0, cfg["B"], 64, 0.1) for w in words]
    assert not np.array_equal(masks[0], masks[1]) and not np.array_equal(masks[1], masks[2])


@pytest.mark.parametrize("mlp,hidden,D", [("bf16", [128, 64], 64), ("bf16", [128, 128, 64], 64), ("fp32", [256, 128, 96], 64)])
def test_dropout_eval_forward(tt, schema_real, tmp_path, mlp, hidden, D):
    """d. After a dropout training step, eval() with dropout_rate = 0.1 (in bf16 the general kernels: the fused tails are
    train-only) matches the oracle's eval forward on the kernels' updated running statistics, and is bit-identical to the same
    eval forward at dropout_rate = 0: no element is dropped."""
    from jodalrob_twotower_amd import synthetic
    B, p = 1000, 0.1
    task, (kn, kc, vn, vc) = _build(tt, schema_real, tmp_path, None, hidden, D, 1.0, mlp, p)
    batch = synthetic.make_batch(B, vn, vc, kn, kc, 256, 128, torch.device(DEV), seed=17)
    _run(task, batch)
    task.eval()
    with torch.no_grad():
        ne, ce = [x.cpu().numpy() for x in task.two_tower_model(batch["notice"], batch["company"])]
        for tw in _towers(task):
            tw.dropout_rate = 0.0
        ne0, ce0 = [x.cpu().numpy() for x in task.two_tower_model(batch["notice"], batch["company"])]
    state = {k: v.detach().cpu().numpy() for k, v in task.state_dict().items()}
    b = _np_batch(batch, B, kn, kc)
    q = O.q_bf16 if mlp == "bf16" else None
    report = {"mlp": mlp, "hidden": hidden, "B": B}
    for name, pre, keys, vocab, got, got0 in (("notice_emb", O.NT, kn, vn, ne, ne0), ("company_emb", O.CT, kc, vc, ce, ce0)):
        want, _, _ = O.tower_fwd(state, pre, keys, vocab, b[name.split("_")[0] + "_dense"], b[name.split("_")[0] + "_ids"].reshape(-1),
                                 False, np.float64, q)
        report[name] = (_rel(got, want), float(np.abs(got - want).max()))
        report[name + ".same_as_p0"] = bool(np.array_equal(got, got0))
    _print("dropout eval forward vs f64 oracle", report)
    bd = EVAL_BOUNDS[mlp]
    for name in ("notice_emb", "company_emb"):
        assert report[name + ".same_as_p0"], report
        assert report[name][0] <= bd["emb_norm"] and report[name][1] <= bd["emb_maxabs"], (name, report)
