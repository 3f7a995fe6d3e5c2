"""score_dtype = "bf16x3": split-bf16 operands (x = hi + lo, three bf16 MFMAs per product) against the f64 oracle.

1. The pack: the hi half is tt_score_pack2_bf16's image bit for bit, the lo half is bf16(scale x - hi) in the same layout.
2. The score node (tt_score_fwd_sym_bf16x3 / tt_score_fwd_bf16x3 / tt_score_bwd_bf16x3) over B 1 .. 8192, D 1 .. 256, T 0.025 .. 2:
   an analytic bound on the diagonal; every figure no worse than the reference's own TF32 arithmetic (the f64 oracle fed operands
   rounded to 11 significant bits) and clearly better than the bf16 mode; ranks bracketed by f64 counts; planted ties exact.
3. Reproducibility and the two forward forms against each other.
4. Training steps against oracle_np.task_step(rounding=None) at the four shapes of test_f32_step_vs_f64_oracle.
5. The captured step (GraphedTrainStep) equals the eager loop bit for bit.

Every case prints one JSON report line (visible with -s).  The fixed bounds are at most 4x the worst figure an MI355X measured (in
brackets); DESIGN.md section 4 quotes them too.
"""
import numpy as np
import pytest
import torch

import oracle_np as O
from _score_forms import rank_bracket as _rank_bracket
from params_init import init_state_numpy, synth_batch_numpy
from test_gpu_parity import DEV, _rel, tt, make_task, to_batch, load_state, BF16_VS_REFERENCE_BOUNDS  # noqa: F401
from test_gpu_f32_parity import _tied_pair, _maxrel, _print, _step_vs_oracle, _assert_step

pytestmark = pytest.mark.gpu

EPS32 = 2.0 ** -23


def _tf32(x):
    """x rounded to 11 significant bits (TF32's 10 stored + the implicit one), round-to-nearest-even, in f64"""
    x = np.asarray(x, dtype=np.float64)
    m, e = np.frexp(x)                        # x = m 2^e, 0.5 <= |m| < 1
    return np.ldexp(np.rint(m * 2.0 ** 11) / 2.0 ** 11, e)


def _bf16_host(t):
    return t.to(torch.bfloat16).to(torch.float32)


# ------------------------------------------------------------------------------------------------ 1. the pack
@pytest.mark.parametrize("R", [1, 63, 65, 4097])
@pytest.mark.parametrize("D", [1, 3, 64, 129, 256])
def test_pack_bf16x3_images(tt, R, D):
    from jodalrob_twotower_amd import ops
    from jodalrob_twotower_amd import _lib as L
    rng = np.random.default_rng(17 * R + D)
    x = torch.from_numpy(rng.standard_normal((R, D)).astype(np.float32)).to(DEV)
    half = L.load().tt_score_pack_bytes(R, D)
    for sc in (1.0, ops.score_unit_scale(1.0 / 0.07)):
        p3, _ = ops.score_pack2_bf16x3(x, x, sc, 1.0)
        assert p3.numel() == 2 * half
        hi_ref, _ = ops.score_pack2_bf16(x, x, sc, 1.0)
        p = x * torch.tensor(sc, dtype=torch.float32, device=DEV)          # the f32 product, as the kernel forms it
        lo = (p - _bf16_host(p)).to(torch.bfloat16).to(torch.float32)     # bf16(scale x - hi), RNE
        lo_ref, _ = ops.score_pack2_bf16(lo, lo, 1.0, 1.0)                 # exact in bf16: the same layout, zero padding
        assert torch.equal(p3[:half], hi_ref), (R, D, sc)
        assert torch.equal(p3[half:], lo_ref), (R, D, sc)
        assert bool(lo.abs().max() > 0) or D * R < 4                       # (a zero lo half would pass the layout check trivially)


# ------------------------------------------------------------------------------------------------ 2. the score node
# Each bound is at most 4x the worst figure an MI355X measured over X3_CASES (in brackets); metric bounds are in units of 1 / T.
X3_SCORE_BOUNDS = {
    "loss_rtol": 1.5e-6,         # |loss - ref| / ref, B > 1                  (3.9e-7 at B = 63, D = 129, T = 0.05)
    "pos_atol": 1.1e-6,          # positive similarity mean, times T          (3.0e-7 at B = 65, D = 3)
    "neg_atol": 1.3e-6,          # negative similarity mean, times T          (3.3e-7 at B = 2, D = 256)
    "grad_norm": 4e-5,           # dN, dC norm-wise                           (1.1e-5 at B = 4097, D = 3, T = 0.05)
    "grad_maxrel": 8e-5,         # dN, dC max-abs over max |ref|              (2.1e-5 at B = 4097, D = 3, T = 0.05)
    "sum_rtol": 9e-6,            # sym vs directional forward: row / column exp-sums, max relative difference   (2.4e-6 at B = 4097, D = 129)
    "b1_loss_ulps": 0.8,         # B = 1: |loss| in f32 spacings of 2 / T     (0.22 at T = 1)
    "b1_grad_eps": 1.8,          # B = 1: max |grad| * T in units of 2^-23    (0.47 at T = 0.025)
}

X3_CASES = [  # (B, D, T)
    (1, 64, 1.0), (1, 3, 0.025),
    (2, 1, 1.0), (2, 256, 2.0),
    (63, 129, 0.05), (63, 1, 0.025),
    (65, 192, 2.0), (65, 64, 0.025), (65, 3, 1.0),
    (97, 96, 1.0),                                        # the 65..128 class of D, ragged B
    (4097, 192, 1.0), (4097, 129, 0.025), (4097, 3, 0.05),
    (8192, 256, 0.025), (8192, 64, 1.0), (8192, 129, 0.05),
]


def _node_errors(loss, o8, gn, gc, ref):
    ref_loss, met, dN, dC = ref
    r = {"loss": abs(float(loss) - ref_loss) / abs(ref_loss),
         "pos": abs(float(o8[2]) - met["positive_similarity_mean"]),
         "neg": abs(float(o8[3]) - met["negative_similarity_mean"])}
    r["dN"] = (_rel(gn, dN), _maxrel(gn, dN))
    r["dC"] = (_rel(gc, dC), _maxrel(gc, dC))
    return r


def _flat(r):
    return {"loss": r["loss"], "pos": r["pos"], "neg": r["neg"], "dN_norm": r["dN"][0], "dN_maxrel": r["dN"][1],
            "dC_norm": r["dC"][0], "dC_maxrel": r["dC"][1]}


def _run_autograd(n, c, inv_t, dtype, *flags):
    from jodalrob_twotower_amd.two_tower_train_task import _ScoreCEFn
    tn, tc = torch.from_numpy(n).to(DEV).requires_grad_(), torch.from_numpy(c).to(DEV).requires_grad_()
    loss, out8, _ = _ScoreCEFn.apply(tn, tc, inv_t, dtype, *flags)
    loss.backward()
    return float(loss.item()), out8.cpu().numpy(), tn.grad.cpu().numpy(), tc.grad.cpu().numpy()


def _x3_node(n, c, inv_t, sym):
    """the x3 node through ops: (loss, out8, dN, dC, diag, rowsum, colsum[, full row rank, col rank, top-1 flags])"""
    from jodalrob_twotower_amd import ops
    B, D = n.shape
    shift = abs(inv_t)
    tn, tc = torch.from_numpy(n).to(DEV), torch.from_numpy(c).to(DEV)
    sn = 1.0                                       # as the task: unscaled images (two_tower_train_task._ScoreCEFn)
    Np, Cp = ops.score_pack2_bf16x3(tn, tc, sn, 1.0)
    extra = ()
    if sym:
        rs, cs, dg, rk, inv, out8, loss = ops.score_fwd_sym(Np, Cp, B, D, inv_t, shift, sn, True, x3=True)
    else:
        rs, cs, dg, rk, ck, ss, inv = ops.score_fwd_bf16(Np, Cp, B, D, inv_t, shift, True, True, sn, with_inv=True, x3=True)
        flag = ops.score_fwd_bf16(Np, Cp, B, D, inv_t, shift, False, False, sn, with_inv=True, x3=True)[3]
        out8, loss = ops.score_loss_finish(B, shift, rs, cs, dg, rk, ck, ss)
        extra = (rk.cpu().numpy(), ck.cpu().numpy(), flag.cpu().numpy())
    dl = torch.ones(1, dtype=torch.float32, device=DEV)
    dN, dC = ops.score_bwd_bf16(Np, Cp, B, D, inv_t, shift, rs, cs, dl, inv_t / (2.0 * B), sn, inv, x3=True)
    torch.cuda.synchronize()
    return (float(loss.item()), out8.cpu().numpy(), dN.cpu().numpy(), dC.cpu().numpy(), dg.cpu().numpy(), rs.cpu().numpy(),
            cs.cpu().numpy()) + extra


@pytest.mark.parametrize("B,D,T", X3_CASES)
def test_x3_score_node_vs_f64(tt, B, D, T):
    rng = np.random.default_rng(1000 * B + D + 7)
    n, c = _tied_pair(rng, B, D)
    n64, c64 = n.astype(np.float64), c.astype(np.float64)
    inv_t = 1.0 / T
    ref_loss, met, S, lse = O.score_ce_fwd(n64, c64, T)
    dN, dC = O.score_ce_bwd(n64, c64, S, lse, T)
    ref = (ref_loss, met, dN, dC)
    # the reference's arithmetic: TF32 operands for S and for the gradient products, TF32-rounded softmax weights
    nt, ct = _tf32(n64), _tf32(c64)
    t_loss, t_met, St, lset = O.score_ce_fwd(nt, ct, T)
    t_dN, t_dC = O.score_ce_bwd(nt, ct, St, lset, T, q=_tf32)
    del St, lset
    sym = _x3_node(n, c, inv_t, True)
    dirf = _x3_node(n, c, inv_t, False)
    f32 = _run_autograd(n, c, inv_t, "fp32")
    b16 = _run_autograd(n, c, inv_t, "bf16", False, False)
    report = {"B": B, "D": D, "T": T}
    # analytic bound on the diagonal: |T diag - (n_i . c_i)_64| <= 2^-13 sum_k |n_ik c_ik|
    dot = (n64 * c64).sum(1)
    bnd = 2.0 ** -13 * np.abs(n64 * c64).sum(1)
    for tag, res in (("sym", sym), ("dir", dirf)):
        err = np.abs(T * res[4].astype(np.float64) - dot)
        report[f"{tag}_diag_over_bound"] = float((err / np.maximum(bnd, 1e-300)).max())
    if B == 1:
        report["loss"] = [sym[0], dirf[0]]
        report["grad_maxabs"] = float(max(np.abs(x).max() for r in (sym, dirf) for x in (r[2], r[3])))
        _print("bf16x3 score node vs f64", report)
        bd = X3_SCORE_BOUNDS
        for r in (sym, dirf):
            assert abs(r[0]) <= bd["b1_loss_ulps"] * float(np.spacing(np.float32(2.0 / T))), report
            assert np.all(np.isfinite(r[2])) and np.all(np.isfinite(r[3]))
            assert max(np.abs(r[2]).max(), np.abs(r[3]).max()) * T <= bd["b1_grad_eps"] * EPS32, report
            assert np.all(np.abs(T * r[4].astype(np.float64) - dot) <= bnd), report
        return
    e_sym = _flat(_node_errors(sym[0], sym[1], sym[2], sym[3], ref))
    e_dir = _flat(_node_errors(dirf[0], dirf[1], dirf[2], dirf[3], ref))
    e_f32 = _flat(_node_errors(f32[0], f32[1], f32[2], f32[3], ref))
    e_b16 = _flat(_node_errors(b16[0], b16[1], b16[2], b16[3], ref))
    e_tf = _flat({"loss": abs(t_loss - ref_loss) / abs(ref_loss),
                  "pos": abs(t_met["positive_similarity_mean"] - met["positive_similarity_mean"]),
                  "neg": abs(t_met["negative_similarity_mean"] - met["negative_similarity_mean"]),
                  "dN": (_rel(t_dN, dN), _maxrel(t_dN, dN)), "dC": (_rel(t_dC, dC), _maxrel(t_dC, dC))})
    # the floor: 4 f32 spacings of the reference value (relative figures: 4 * 2^-23)
    floor = {"loss": 4 * EPS32, "pos": 4 * float(np.spacing(np.float32(abs(met["positive_similarity_mean"])))),
             "neg": 4 * float(np.spacing(np.float32(abs(met["negative_similarity_mean"])))),
             **{k: 4 * EPS32 for k in ("dN_norm", "dN_maxrel", "dC_norm", "dC_maxrel")}}
    report.update({"x3_sym": e_sym, "x3_dir": e_dir, "fp32": e_f32, "tf32": e_tf, "bf16": e_b16,
                   "tf32_over_x3": {k: e_tf[k] / max(e_sym[k], 1e-300) for k in e_sym}})
    # the two forward forms: the same sums up to order (the sym kernel adds the tiles of a row in another order)
    report["sym_vs_dir_sums"] = float(max(np.abs(sym[5] / dirf[5] - 1).max(), np.abs(sym[6] / dirf[6] - 1).max()))
    # ranks: the full rank of every row (and column) inside the f64 bracket; planted ties exact; top-1 flags == (rank == 0)
    delta = 2.0 * 2.0 ** -13 * np.linalg.norm(n64, axis=1) * np.linalg.norm(c64, axis=1).max() / T
    lo, hi = _rank_bracket(S, c, delta)
    delta_c = 2.0 * 2.0 ** -13 * np.linalg.norm(c64, axis=1) * np.linalg.norm(n64, axis=1).max() / T
    lo_c, hi_c = _rank_bracket(np.ascontiguousarray(S.T), n, delta_c)
    rk, ck, flag = dirf[7], dirf[8], dirf[9]
    report["rank_outside"] = int(((rk < lo) | (rk > hi)).sum())
    report["col_rank_outside"] = int(((ck < lo_c) | (ck > hi_c)).sum())
    report["top1_flag_mismatch"] = int(((flag == 0) != (rk == 0)).sum())
    _print("bf16x3 score node vs f64", report)

    bd = X3_SCORE_BOUNDS
    for tag in ("sym", "dir"):
        assert report[f"{tag}_diag_over_bound"] <= 1.0, report
    assert report["rank_outside"] == 0 and report["col_rank_outside"] == 0 and report["top1_flag_mismatch"] == 0, report
    if B >= 4:                                                       # the planted ties (tests/test_gpu_f32_parity._tied_pair)
        assert rk[B - 1] >= 1 and flag[B - 1] == 1, report           # row B-1's company row equals row 1's: the earlier one wins
        assert ck[B - 2] >= 1, report                                # column B-2's notice row equals row 0's
    assert report["sym_vs_dir_sums"] <= bd["sum_rtol"], report
    for e in (e_sym, e_dir):
        for k in e:
            assert e[k] <= max(e_tf[k], 2 * e_f32[k], floor[k]), (k, e[k], e_tf[k], e_f32[k], report)
            if k not in ("pos", "neg"):
                assert e[k] <= max(e_b16[k] / 16, floor[k]), (k, e[k], e_b16[k], report)
        assert e["loss"] <= bd["loss_rtol"], report
        assert e["pos"] * T <= bd["pos_atol"] and e["neg"] * T <= bd["neg_atol"], report
        for k in ("dN", "dC"):
            assert e[f"{k}_norm"] <= bd["grad_norm"] and e[f"{k}_maxrel"] <= bd["grad_maxrel"], (k, report)


# ------------------------------------------------------------------------------------------------ 3. reproducibility
@pytest.mark.parametrize("B,D", [(4097, 64), (8192, 256)])
def test_x3_node_bitwise_reproducible(tt, B, D):
    rng = np.random.default_rng(B + D)
    n, c = _tied_pair(rng, B, D)
    for sym in (True, False):
        a, b = _x3_node(n, c, 2.0, sym), _x3_node(n, c, 2.0, sym)
        assert a[0] == b[0] and np.array_equal(a[1], b[1]), sym
        assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]), sym


# ------------------------------------------------------------------------------------------------ 4. the training step
# One step with score_dtype = "bf16x3", mlp_dtype = "fp32" against oracle_np.task_step(rounding=None) in f64.  Each bound is at most
# 4x the worst figure an MI355X measured over the four cases (in brackets), and at most 1/10 of BF16_VS_REFERENCE_BOUNDS' entry.
X3_STEP_BOUNDS = {
    "loss_rtol": 2e-7,                # |loss - ref| / ref                  (6.8e-8 at B = 8192)
    "emb_norm": 3.2e-6, "emb_maxabs": 2.6e-6,    # unit rows [B, D]         (8.5e-7 / 6.6e-7)
    "metric_atol": 8e-8,              # positive / negative means, gap       (2.1e-8 at B = 4097, T = 0.07)
    "dense_grad_matrix_norm": 1.6e-5, # Linear weights, norm-wise per tensor (4.0e-6 at B = 1000)
    "dense_grad_vector_norm": 8.5e-5, # biases, BN scale / shift             (2.2e-5 at B = 8192)
    "table_grad_norm": 1.4e-5,        # sparse rows (row set bit-exact) or the full dense tables   (3.6e-6 at B = 1000)
}


def test_x3_step_bounds_below_a_tenth_of_bf16():
    ref = dict(BF16_VS_REFERENCE_BOUNDS, table_grad_norm=BF16_VS_REFERENCE_BOUNDS["row_grad_norm"])
    for k, v in X3_STEP_BOUNDS.items():
        assert v <= ref[k] / 10, k


def _x3_task(tt, schema_real, tmp_path, rows_per_tower, hidden, D, T, grad, score_dtype="bf16x3", mlp_dtype="fp32"):
    """test_gpu_f32_parity._real_task with the given precisions"""
    from jodalrob_twotower_amd import synthetic
    kn, kc = schema_real["notice"]["categorical"], schema_real["company"]["categorical"]
    vn, vc = schema_real["notice"]["vocab_sizes"], schema_real["company"]["vocab_sizes"]
    if rows_per_tower:
        vn, vc = synthetic.scale_vocabs(vn, rows_per_tower), synthetic.scale_vocabs(vc, rows_per_tower)
    meta = synthetic.write_metadata(tmp_path / "m.csv", {"notice": dict(zip(kn, vn)), "company": dict(zip(kc, vc))})
    torch.manual_seed(4321)
    task = tt.create_two_tower_train_task(kn, kc, metadata_path=str(meta), categorical_embedding_dim=32, notice_dense_input_dim=256,
                                          company_dense_input_dim=128, tower_hidden_dims=hidden, final_embedding_dim=D,
                                          dropout_rate=0.0, temperature=T, device=DEV, embedding_grad=grad, score_dtype=score_dtype,
                                          mlp_dtype=mlp_dtype)
    task.train()
    task._pair_check_done = True
    with torch.no_grad():
        g = torch.Generator(device=DEV).manual_seed(78)
        for p in task.parameters():
            if p.ndim == 1:
                p.add_(0.1 * torch.randn(p.shape, generator=g, device=DEV))
    return task, (kn, kc, vn, vc)


def _summary(report, mat, vec):
    return {"loss": report["loss"], "dense_matrix_max": max(report[k] for k in mat), "dense_vector_max": max(report[k] for k in vec),
            "table": report["table_grads"], "metric_max": max(report[k] for k in ("positive_similarity_mean", "negative_similarity_mean",
                                                                                    "similarity_gap"))}


@pytest.mark.parametrize("rows_per_tower,B,T,hidden,D,grad", [(1_000_000, 8192, 1.0, [128, 64], 64, "sparse"),
                                                              (None, 1000, 0.5, [128, 64], 64, "dense"),
                                                              (None, 2240, 1.0, [512, 256], 128, "sparse"),
                                                              (None, 4097, 0.07, [256, 128], 256, "sparse")])
def test_x3_step_vs_f64_oracle(tt, schema_real, tmp_path, rows_per_tower, B, T, hidden, D, grad):
    task, schema = _x3_task(tt, schema_real, tmp_path, rows_per_tower, hidden, D, T, grad)
    report, ref_metric, mat, vec = _step_vs_oracle(task, schema, B, T, grad, seed=2468)
    _print("bf16x3 step vs f64 oracle", report)
    _assert_step(report, ref_metric, mat, vec, B, X3_STEP_BOUNDS)


def test_x3_score_share_of_bf16_step_error(tt, schema_real, tmp_path):
    """mlp_dtype = "bf16" with score_dtype = "bf16x3" next to the all-bf16 mode, both against the unrounded f64 oracle at configs[1]'s
    shapes: what is left with the score near f32 is the MLP's share of the bf16 mode's error (figures in DESIGN.md section 4)."""
    out = {}
    for sd in ("bf16x3", "bf16"):
        task, schema = _x3_task(tt, schema_real, tmp_path, 1_000_000, [128, 64], 64, 1.0, "sparse", score_dtype=sd, mlp_dtype="bf16")
        report, _, mat, vec = _step_vs_oracle(task, schema, 8192, 1.0, "sparse", seed=2468)
        out[sd] = _summary(report, mat, vec)
        assert report["table_rows_exact"], report
        assert all(np.isfinite(v) for v in out[sd].values()), out
        del task
    _print("score share of the bf16 step error (mlp bf16)", out)
    bd = BF16_VS_REFERENCE_BOUNDS
    assert out["bf16x3"]["dense_matrix_max"] <= bd["dense_grad_matrix_norm"], out
    assert out["bf16x3"]["dense_vector_max"] <= bd["dense_grad_vector_norm"], out


# ------------------------------------------------------------------------------------------------ 5. the captured step
def test_x3_graphed_step_equals_eager(tt, manifest):
    """test_gpu_parity.test_graphed_step_equals_eager with score_dtype = "bf16x3": HIP-graph replay == the eager loop, bit for bit
    (losses, weights, Adam moments)."""
    from jodalrob_twotower_amd.graph import GraphedTrainStep
    from jodalrob_twotower_amd.optim import FusedAdam
    cfg = dict(manifest["cases"]["wide_b40"])
    cfg["B"] = 256
    batches = [synth_batch_numpy(cfg["B"], cfg["vocab_n"], cfg["vocab_c"], cfg["din_n"], cfg["din_c"], 930 + i, oob=False) for i in range(3)]
    finals = {}
    for mode in ("eager", "graph"):
        task = make_task(tt, cfg, embedding_grad="sparse", score_dtype="bf16x3", mlp_dtype="fp32")
        shapes = {k: tuple(v.shape) for k, v in task.state_dict().items()}
        load_state(task, init_state_numpy(shapes, 56))
        task.train()
        task._pair_check_done = True
        opt = FusedAdam.for_task(task, lr=1e-2, weight_decay=1e-5)
        tb = [to_batch(tt, b, cfg["keys_n"], cfg["keys_c"]) for b in batches]
        losses = []
        if mode == "eager":
            for b in tb:
                opt.zero_grad()
                r = task(b, return_metrics=True)
                r["loss"].backward()
                opt.step()
                losses.append(r["loss"].item())
        else:
            gs = GraphedTrainStep(task, opt, tb[0], warmup=3)
            for b in tb:
                r = gs.step(b)
                losses.append(r["loss"].item())
        moments = {}                                  # torch.optim.Adam layout: exp_avg / exp_avg_sq per parameter, in order
        for i, p in enumerate(task.parameters()):
            for k, v in opt.state.get(p, {}).items():
                if torch.is_tensor(v) and v.numel() > 1:
                    moments[f"{i}.{k}"] = v.detach().cpu().numpy().copy()
        assert moments
        finals[mode] = (losses, {k: v.detach().cpu().numpy().copy() for k, v in task.state_dict().items()}, moments)
    assert finals["eager"][0] == finals["graph"][0]
    for k, v in finals["eager"][1].items():
        assert np.array_equal(v, finals["graph"][1][k]), k
    for k, v in finals["eager"][2].items():
        assert np.array_equal(v, finals["graph"][2][k]), k
