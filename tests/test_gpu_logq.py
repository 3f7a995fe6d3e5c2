"""logQ sampling-bias correction of the in-batch softmax on the MI355X (include/twotower.h *_lq entries).

1. The score node (_ScoreCEFn with lq_n / lq_c) against a float64 reference of the corrected loss written here, fed the kernels'
   own operand rounding: bf16, bf16x3 and fp32, ragged shapes, every backward form, extreme and Zipf-like log q.
2. Invariances: a constant log q gives the uncorrected loss and gradients; log q below -40 is clamped; runs are bitwise
   reproducible; metrics are bitwise the uncorrected entry's.
3. The temperature limit of the corrected entries (2/T <= 40).
4. Training: the eager step and GraphedTrainStep.step(batch) with log q are bit-identical (dropout off); with dropout on two
   captured runs agree bit for bit, and the corrected run moves the weights differently from an uncorrected one.
"""
import numpy as np
import pytest
import torch

from params_init import init_state_numpy, synth_batch_numpy
from test_gpu_parity import DEV, tt, ctx_option, make_task, to_batch, load_state  # noqa: F401

pytestmark = pytest.mark.gpu

L_CLAMP = 40.0


def _lq(B, kind, seed):
    g = np.random.default_rng(seed)
    if kind == "random":
        v = g.uniform(-30.0, 0.0, B)
        if B >= 3:
            v[0], v[1], v[2] = 0.0, -40.0, -55.0          # planted extremes (the last one clamps to -40)
    elif kind == "zipf":                                     # log of a Zipf(1.1) share, ranks shuffled
        r = g.permutation(B) + 1.0
        p = r ** -1.1
        v = np.log(p / p.sum())
    else:
        v = np.full(B, float(kind))
    return torch.tensor(v, dtype=torch.float32, device=DEV)


def _unit_rows(B, D, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(B, D, generator=g, device=DEV)
    return x / x.norm(dim=1, keepdim=True)


def _bf16(x):
    return x.to(torch.bfloat16).to(torch.float64)


def _operands(n, c, inv_t, mode):
    """(A, Bm, s_scale): the f64 operands the kernels multiply and the factor that turns A Bm^T into s = <n, c> / T"""
    from jodalrob_twotower_amd import ops
    if mode == "bf16":
        sn = ops.score_unit_scale(inv_t)
        return _bf16(torch.tensor(sn, dtype=torch.float32, device=DEV) * n), _bf16(c), inv_t / sn
    if mode == "bf16x3":
        def split(x):
            hi = x.to(torch.bfloat16).float()
            return hi.double() + (x - hi).to(torch.bfloat16).double()
        return split(n), split(c), inv_t
    return n.double(), c.double(), inv_t


def _reference(n, c, inv_t, lq_n, lq_c, mode):
    """f64 corrected loss and (dN, dC) for d_loss = 1 on the kernels' operands (bf16: the softmax weights rounded to bf16 and
    the gradient products on the bf16 images, as the kernels form them)."""
    A, Bm, k = _operands(n, c, inv_t, mode)
    B = A.shape[0]
    S = (A @ Bm.T) * k
    qn = lq_n.double().clamp(-L_CLAMP, 0.0)
    qc = lq_c.double().clamp(-L_CLAMP, 0.0)
    R = S - qc[None, :]                                      # row direction: s_ab - lqC[b]
    C = S - qn[:, None]                                      # column direction: s_ab - lqN[a]
    eye = torch.eye(B, dtype=torch.float64, device=DEV)
    loss = 0.5 * ((torch.logsumexp(R, 1) - R.diagonal()).mean() + (torch.logsumexp(C, 0) - C.diagonal()).mean())
    W = torch.softmax(R, 1) + torch.softmax(C, 0) - 2.0 * eye
    if mode == "bf16":
        W = _bf16(W.float())
    g = inv_t / (2.0 * B)
    if mode == "bf16":
        Ag = A * (k / inv_t)                                 # the notice image carries the unit scale: dC divides it out
        return loss.item(), g * (W @ Bm), g * (W.T @ Ag)
    return loss.item(), g * (W @ Bm), g * (W.T @ A)


def _run(n, c, inv_t, mode, lq_n=None, lq_c=None, first_call=False, with_rank=False):
    from jodalrob_twotower_amd.two_tower_train_task import _ScoreCEFn
    n = n.clone().requires_grad_(True)
    c = c.clone().requires_grad_(True)
    loss, out8, rank = _ScoreCEFn.apply(n, c, inv_t, mode, first_call, False, None, None, None, lq_n, lq_c)
    loss.backward()
    torch.cuda.synchronize()
    r = (loss.detach().clone(), out8.detach().clone(), n.grad.detach().clone(), c.grad.detach().clone())
    return r + (rank.clone(),) if with_rank else r


def _ref_sums(n, c, inv_t, lq_n, lq_c, mode):
    """f64 corrected per-row sums as the entries return them: rowsum[a] = sum_b exp(s_ab - 1/T) exp(-40 - lqC[b]), colsum likewise"""
    A, Bm, k = _operands(n, c, inv_t, mode)
    E = torch.exp((A @ Bm.T) * k - abs(inv_t))
    wn = torch.exp(-L_CLAMP - lq_n.double().clamp(-L_CLAMP, 0.0))
    wc = torch.exp(-L_CLAMP - lq_c.double().clamp(-L_CLAMP, 0.0))
    return E @ wc, E.T @ wn


def _sums(n, c, inv_t, lq_n, lq_c, mode):
    """the entries' corrected per-row sums (the forward _ScoreCEFn runs, called directly)"""
    from jodalrob_twotower_amd import ops
    B, D = n.shape
    if mode == "fp32":
        return ops.score_dir_fwd_lq(n, c, inv_t, abs(inv_t), lq_c)[0], ops.score_dir_fwd_lq(c, n, inv_t, abs(inv_t), lq_n)[0]
    x3 = mode == "bf16x3"
    sn = 1.0 if x3 else ops.score_unit_scale(inv_t)
    Np, Cp = (ops.score_pack2_bf16x3 if x3 else ops.score_pack2_bf16)(n, c, sn, 1.0)
    r = ops.score_fwd_sym_lq(Np, Cp, B, D, inv_t, abs(inv_t), lq_n, lq_c, sn, True, x3=x3)
    return r[0], r[1]


def _nrel(x, ref, floor=1e-3):
    """norm-wise relative error; the floor keeps B = 1 (a zero gradient) meaningful"""
    return float((x.double() - ref).norm() / max(ref.norm().item(), floor))


# loss rtol / gradient norm-wise bounds per mode: those the existing tests hold the UNCORRECTED node of the same mode to
# (test_gpu_parity / test_gpu_score_bf16x3 / test_gpu_f32_parity; bf16: the reference rounds the softmax weights as the kernels
# do).  Stated margin: the corrected per-row loss term adds and subtracts log terms of size up to ~40 + 1/T, so its absolute
# rounding is one f32 ulp of 64 (2^-18 = 3.8e-6) where the plain one's is an ulp of ~log B -- LOSS_ATOL.
BOUNDS = {"bf16": (2e-6, 3e-4), "bf16x3": (1.5e-6, 4e-5), "fp32": (3e-6, 7e-6)}
LOSS_ATOL = 2.0 ** -18
SUM_RTOL = {"bf16": 2e-5, "bf16x3": 2e-6, "fp32": 2e-6}     # per-row corrected sums against f64 on the same operands


def _sum_rtol(mode, inv_t):
    """stated margin: a term's f32 exponent argument s - 1/T - 40 - lq reaches 2/T + 40 in magnitude, and one rounding of it is a
    relative error of that times 2^-24 in the term (4 such roundings allowed); at T = 1 the per-mode bound holds alone"""
    return max(SUM_RTOL[mode], 4 * 2.0 ** -24 * (2 * abs(inv_t) + L_CLAMP))
SHAPES = [(1, 32, 1.0), (33, 1, 0.5), (257, 200, 2.0), (257, 64, 0.05), (2048, 128, 1.0), (2048, 256, 0.5),
          (8192, 64, 1.0), (8192, 128, 0.05), (33, 256, 1.0), (2048, 32, 2.0),
          (97, 96, 1.0)]                              # (the 65..128 class of D at a ragged B: four tiles, the last one partial)


# (the f32 parity path at B = 8192 runs at D = 64 only)
NODE_CASES = [(m, B, D, T) for m in ("bf16", "bf16x3", "fp32") for (B, D, T) in SHAPES if not (m == "fp32" and B == 8192 and D == 128)]


@pytest.mark.parametrize("mode,B,D,T", NODE_CASES)
@pytest.mark.parametrize("kind", ["random", "zipf"])
def test_logq_score_node_vs_f64(tt, mode, B, D, T, kind):
    inv_t = 1.0 / T
    n, c = _unit_rows(B, D, 11 + B + D), _unit_rows(B, D, 29 + B + D)
    lq_n, lq_c = _lq(B, kind, 3 + B), _lq(B, kind, 5 + D)
    loss, out8, gn, gc, rank = _run(n, c, inv_t, mode, lq_n, lq_c, with_rank=True)
    ref_loss, ref_gn, ref_gc = _reference(n, c, inv_t, lq_n, lq_c, mode)
    lb, gb = BOUNDS[mode]
    assert abs(loss.item() - ref_loss) <= lb * abs(ref_loss) + LOSS_ATOL, (loss.item(), ref_loss)
    fl = inv_t / (2.0 * B)                                   # one unit row's full gradient weight: the floor at B = 1 (zero gradient)
    assert _nrel(gn, ref_gn, fl) <= gb, _nrel(gn, ref_gn, fl)
    assert _nrel(gc, ref_gc, fl) <= gb, _nrel(gc, ref_gc, fl)
    # the corrected per-row sums
    rs, cs = _sums(n, c, inv_t, lq_n, lq_c, mode)
    ref_rs, ref_cs = _ref_sums(n, c, inv_t, lq_n, lq_c, mode)
    for got, ref in ((rs, ref_rs), (cs, ref_cs)):
        err = float(((got.double() - ref).abs() / ref).max())
        assert err <= _sum_rtol(mode, inv_t), err
    # metrics (all of out8 but the loss) and the row ranks are the raw scores': bitwise the uncorrected entry's
    _, out8_plain, _, _, rank_plain = _run(n, c, inv_t, mode, with_rank=True)
    torch.testing.assert_close(out8[1:], out8_plain[1:], rtol=0, atol=0, equal_nan=True)     # (B = 1: the negative mean is nan)
    assert torch.equal(rank, rank_plain)


@pytest.mark.parametrize("mode", ["bf16", "bf16x3"])
@pytest.mark.parametrize("B,D", [(2048, 64), (4100, 128), (2048, 256)])
def test_logq_workgroup_staged_backward(tt, ctx_option, mode, B, D):
    """TT_OPT_SCORE_BWD_ROWS_MIN forced low: the bf16 backward takes its workgroup-staged form (weights staged beside the
    reciprocals) and still meets the f64 reference."""
    from jodalrob_twotower_amd import _lib as L
    ctx_option(L.TT_OPT_SCORE_BWD_ROWS_MIN, 64, 32768)
    n, c = _unit_rows(B, D, 71), _unit_rows(B, D, 73)
    lq_n, lq_c = _lq(B, "random", 1), _lq(B, "zipf", 2)
    loss, _, gn, gc = _run(n, c, 1.0, mode, lq_n, lq_c)
    ref_loss, ref_gn, ref_gc = _reference(n, c, 1.0, lq_n, lq_c, mode)
    lb, gb = BOUNDS[mode]
    assert abs(loss.item() - ref_loss) <= lb * abs(ref_loss) + LOSS_ATOL
    assert _nrel(gn, ref_gn) <= gb and _nrel(gc, ref_gc) <= gb, (_nrel(gn, ref_gn), _nrel(gc, ref_gc))


@pytest.mark.parametrize("mode", ["bf16", "bf16x3", "fp32"])
def test_logq_constant_is_uncorrected_and_clamped_and_reproducible(tt, mode):
    B, D, inv_t = 1000, 64, 1.0
    n, c = _unit_rows(B, D, 5), _unit_rows(B, D, 6)
    const = _lq(B, -7.25, 0)
    loss_c, _, gn_c, gc_c = _run(n, c, inv_t, mode, const, const)
    loss_p, _, gn_p, gc_p = _run(n, c, inv_t, mode)
    assert abs(loss_c.item() - loss_p.item()) <= 1e-5 * abs(loss_p.item())          # softmax shift invariance
    assert _nrel(gn_c, gn_p.double()) <= 2e-4 and _nrel(gc_c, gc_p.double()) <= 2e-4
    # below -40 counts as -40: the same bits
    lo = _lq(B, "random", 9)
    r40 = _run(n, c, inv_t, mode, lo.clamp(min=-40.0), lo.clamp(min=-40.0))
    r99 = _run(n, c, inv_t, mode, torch.where(lo <= -40.0, torch.full_like(lo, -99.0), lo), torch.where(lo <= -40.0, -1e4 + 0 * lo, lo))
    for a, b in zip(r40, r99):
        assert torch.equal(a, b)
    # bitwise reproducible
    again = _run(n, c, inv_t, mode, lo, lo)
    first = _run(n, c, inv_t, mode, lo, lo)
    for a, b in zip(first, again):
        assert torch.equal(a, b)


@pytest.mark.parametrize("mode", ["bf16", "bf16x3", "fp32"])
def test_logq_first_call_diagnostic(tt, mode):
    """The task's first call (want_col_rank: the pair-alignment diagnostic): the loss and gradients are the corrected ones,
    out8[5] (the column top-1 rate) is the uncorrected first call's."""
    B, D = 1000, 64
    n, c = _unit_rows(B, D, 15), _unit_rows(B, D, 16)
    lq_n, lq_c = _lq(B, "random", 17), _lq(B, "zipf", 18)
    first = _run(n, c, 1.0, mode, lq_n, lq_c, first_call=True)
    later = _run(n, c, 1.0, mode, lq_n, lq_c)
    for a, b in zip(first[:1] + first[2:], later[:1] + later[2:]):
        assert torch.equal(a, b)
    # metrics: those of the corrected steady-state call (the symmetric forward); the row and column top-1 rates those of the plain
    # first call (whose means come from the two-direction kernel: equal up to summation order, not compared bitwise)
    torch.testing.assert_close(first[1][1:5], later[1][1:5], rtol=0, atol=0)
    plain_first = _run(n, c, 1.0, mode, first_call=True)
    assert first[1][5].item() == plain_first[1][5].item() and first[1][5].item() > 0.0
    assert first[1][1].item() == plain_first[1][1].item()


def test_logq_temperature_limit(tt):
    from jodalrob_twotower_amd import ops
    B, D = 64, 32
    n, c = _unit_rows(B, D, 1), _unit_rows(B, D, 2)
    lq = _lq(B, "random", 3)
    for mode in ("bf16", "bf16x3", "fp32"):
        with pytest.raises(ValueError, match="2/T"):
            _run(n, c, 1.0 / 0.049, mode, lq, lq)
    # the C entry itself: TT_ERR_UNSUPPORTED
    Np, Cp = ops.score_pack2_bf16(n, c, 1.0, 1.0)
    with pytest.raises(Exception, match="2/T"):
        ops.score_fwd_sym_lq(Np, Cp, B, D, 1.0 / 0.049, 1.0 / 0.049, lq, lq)
    with pytest.raises(Exception, match="2/T"):
        ops.score_dir_fwd_lq(n, c, 1.0 / 0.049, 1.0 / 0.049, lq)
    # the backward entries refuse it too
    d_loss = torch.ones(1, device=DEV)
    with pytest.raises(Exception, match="2/T"):
        ops.score_dir_bwd_lq(n, c, 1.0 / 0.049, 1.0 / 0.049, 0, lq, lq, torch.ones(B, device=DEV), torch.ones(B, device=DEV), d_loss, 1.0)
    rs, cs, _, _, inv, w, _, _ = ops.score_fwd_sym_lq(Np, Cp, B, D, 20.0, 20.0, lq, lq)
    with pytest.raises(Exception, match="2/T"):
        ops.score_bwd_bf16_lq(Np, Cp, B, D, 1.0 / 0.049, 1.0 / 0.049, rs, cs, d_loss, 1.0, w, inv=inv)
    _run(n, c, 1.0 / 0.05, "bf16", lq, lq)                       # 2/T = 40 is supported


def _train(tt, manifest, with_lq, score_dtype, steps=5):
    from jodalrob_twotower_amd.graph import GraphedTrainStep
    from jodalrob_twotower_amd.optim import FusedAdam
    cfg = dict(manifest["cases"]["wide_b40"])
    cfg["B"] = 256
    batches = [synth_batch_numpy(cfg["B"], cfg["vocab_n"], cfg["vocab_c"], cfg["din_n"], cfg["din_c"], 610 + i, oob=False)
               for i in range(steps)]
    torch.manual_seed(2024)                                  # the towers draw their dropout seeds from torch's CPU generator
    task = make_task(tt, cfg, embedding_grad="sparse", score_dtype=score_dtype, mlp_dtype="fp32", dropout_rate=0.2)
    shapes = {k: tuple(v.shape) for k, v in task.state_dict().items()}
    load_state(task, init_state_numpy(shapes, 77))
    task.train()
    task._pair_check_done = True
    opt = FusedAdam.for_task(task, lr=1e-2, weight_decay=1e-5)
    tb = [to_batch(tt, b, cfg["keys_n"], cfg["keys_c"]) for b in batches]
    if with_lq:
        for i, b in enumerate(tb):
            b["notice"]["log_q"] = _lq(cfg["B"], "random", 40 + i)
            b["company"]["log_q"] = _lq(cfg["B"], "zipf", 50 + i)
    gs = GraphedTrainStep(task, opt, tb[0], warmup=3)
    losses = [gs.step(b)["loss"].item() for b in tb]
    return losses, {k: v.detach().cpu().numpy().copy() for k, v in task.state_dict().items()}


@pytest.mark.parametrize("score_dtype", ["bf16", "fp32"])
def test_logq_graphed_dropout_reproducible_and_correction_is_wired(tt, manifest, score_dtype):
    """Dropout on: two captured runs with log q (two more copy segments of the one hand-over launch) agree bit for bit, and the
    corrected run's losses and weights differ from an uncorrected run's."""
    g_losses, g_state = _train(tt, manifest, True, score_dtype)
    g2_losses, g2_state = _train(tt, manifest, True, score_dtype)
    assert g_losses == g2_losses
    for k, v in g_state.items():
        assert np.array_equal(v, g2_state[k]), k
    p_losses, p_state = _train(tt, manifest, False, score_dtype)
    assert g_losses != p_losses
    assert any(not np.array_equal(v, p_state[k]) for k, v in g_state.items() if v.dtype.kind == "f")


def test_logq_eager_equals_graphed_without_dropout(tt, manifest):
    """dropout off: the eager and captured steps consume no seeds, so the two loops must match bit for bit"""
    from jodalrob_twotower_amd.graph import GraphedTrainStep
    from jodalrob_twotower_amd.optim import FusedAdam
    cfg = dict(manifest["cases"]["wide_b40"])
    cfg["B"] = 256
    batches = [synth_batch_numpy(cfg["B"], cfg["vocab_n"], cfg["vocab_c"], cfg["din_n"], cfg["din_c"], 700 + i, oob=False) for i in range(5)]
    finals = {}
    for mode in ("eager", "graph"):
        task = make_task(tt, cfg, embedding_grad="sparse", score_dtype="bf16", mlp_dtype="fp32")
        shapes = {k: tuple(v.shape) for k, v in task.state_dict().items()}
        load_state(task, init_state_numpy(shapes, 56))
        task.train()
        task._pair_check_done = True
        opt = FusedAdam.for_task(task, lr=1e-2, weight_decay=1e-5)
        tb = [to_batch(tt, b, cfg["keys_n"], cfg["keys_c"]) for b in batches]
        for i, b in enumerate(tb):
            b["notice"]["log_q"] = _lq(cfg["B"], "random", 80 + i)
            b["company"]["log_q"] = _lq(cfg["B"], "zipf", 90 + i)
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
                losses.append(gs.step(b)["loss"].item())
            with pytest.raises(ValueError, match="log_q mismatch"):
                gs.step({s: {k: v for k, v in tb[0][s].items() if k != "log_q"} for s in ("notice", "company")})
        finals[mode] = (losses, {k: v.detach().cpu().numpy().copy() for k, v in task.state_dict().items()})
    assert finals["eager"][0] == finals["graph"][0]
    for k, v in finals["eager"][1].items():
        assert np.array_equal(v, finals["graph"][1][k]), k


def _pair_world(tt, tmp_path, n_pairs):
    """test_gpu_next_rows' synthetic stores: metadata, schema and a SyntheticSource of n_pairs pairs"""
    from jodalrob_twotower_amd import synthetic
    vn, vc = [12, 400, 7, 90], [9, 50]
    meta = synthetic.write_metadata(tmp_path / "metadata.csv", {"notice": {f"n{i}": v for i, v in enumerate(vn)},
                                                                 "company": {f"c{i}": v for i, v in enumerate(vc)}})
    with open(meta, "a", encoding="utf-8") as f:
        f.write("notice,bidntceno,text,Y,,,,0,,Y,Y,,\nnotice,bidntceord,text,Y,,,,0,,Y,Y,,\ncompany,bizno,text,Y,,,,0,,Y,Y,,\n"
                "notice,amount,numeric,Y,,,,0,,,,,\ncompany,size,numeric,Y,,,,0,,,,,\n")
    schema = tt.build_torchrec_schema_from_meta(notice_table="notice", company_table="company", pair_table="bid_two_tower",
                                                pair_notice_id_cols=["bidntceno", "bidntceord"], pair_company_id_cols=["bizno"],
                                                metadata_path=str(meta))
    return meta, schema, lambda: synthetic.SyntheticSource(900, 700, n_pairs, vn, vc, pair_zipf_alpha=1.1)


def test_logq_eager_vs_step_vs_step_from_store(tt, tmp_path):
    """Dropout on, 1203 pairs (not a multiple of 4) in batches of 254 (not a multiple of 4 either): 4 full batches + a ragged one
    of 187, two epochs, the loader attaching log q (DevicePairLoader(log_q=...)).  Three legs, bit for bit -- per-step losses,
    final weights: (a) every batch through the eager step, (b) full batches through GraphedTrainStep.step(batch) (log q as two
    more copy segments of the hand-over), (c) the epoch through DevicePairLoader.step_batches -> step_from_store (log q slices of
    the per-epoch array inside tt_batch_ingest_store's copy list).  The ragged batch goes through the eager step in every leg.
    Dropout seeds: the captured steps' host seed plus each replay's device word; the eager leg replays those words."""
    from jodalrob_twotower_amd.data_loader import create_unified_bid_dataloaders
    from jodalrob_twotower_amd.graph import GraphedTrainStep
    from jodalrob_twotower_amd.optim import FusedAdam
    from jodalrob_twotower_amd.sampling_bias import log_sampling_probs
    M64 = (1 << 64) - 1
    base = 0x5DEECE66D
    P, B = 1203, 254
    meta, schema, source = _pair_world(tt, tmp_path, P)
    finals, words_of = {}, {}
    for mode in ("tensors", "store", "eager"):
        torch.manual_seed(123)
        train_loader, _ = create_unified_bid_dataloaders(source(), schema, batch_size=B, test_split=0.0, shuffle_seed=7,
                                                         test_mode=True, pair_limit=P, device=DEV)
        tp = train_loader.pairs
        train_loader.set_log_q((log_sampling_probs(tp[:, 0], len(train_loader.notice)),
                                log_sampling_probs(tp[:, 1], len(train_loader.company))))
        assert len(train_loader) == 5 and tp.shape[0] == P
        first = next(iter(train_loader))
        assert first["notice"]["log_q"].shape == (B,) and first["company"]["log_q"].std() > 0
        train_loader._gen.manual_seed(7)
        task = tt.create_two_tower_train_task(schema.notice.categorical, schema.company.categorical, metadata_path=str(meta),
                                              categorical_embedding_dim=16, notice_dense_input_dim=first["notice"]["dense"].shape[1],
                                              company_dense_input_dim=first["company"]["dense"].shape[1], tower_hidden_dims=[64, 32],
                                              final_embedding_dim=32, dropout_rate=0.1, device=DEV, embedding_grad="sparse",
                                              score_dtype="bf16", mlp_dtype="bf16")
        torch.manual_seed(0)
        with torch.no_grad():
            for p in task.parameters():
                p.copy_(0.05 * torch.randn(p.shape, device=DEV))
        task.train()
        task._pair_check_done = True
        towers = (task.two_tower_model.notice_tower, task.two_tower_model.company_tower)
        for tw in towers:
            tw._seed_override = base
        opt = FusedAdam.for_task(task, lr=1e-2, weight_decay=1e-5)
        torch.manual_seed(99)                                            # the replays' device seed words draw from it
        gs = GraphedTrainStep(task, opt, first, warmup=1) if mode != "eager" else None

        def eager(b, word=None):
            for tw in towers:
                tw._seed_override = base if word is None else (base + word) & M64
            opt.zero_grad()
            r = task(b, return_metrics=True)
            r["loss"].backward()
            opt.step()
            return r
        losses, words = [], []
        for ep in range(2):
            if mode == "store":
                for r in train_loader.step_batches(gs, eager):
                    losses.append(r["loss"].item())
                    if r is gs.result:
                        words.append(int(gs._seed_dev.item()) & M64)
            else:
                for b in train_loader:
                    full = b["notice"]["dense"].shape[0] == B
                    if mode == "tensors" and full:
                        r = gs.step(b)
                        losses.append(r["loss"].item())
                        words.append(int(gs._seed_dev.item()) & M64)
                    elif mode == "eager" and full:
                        w = words_of["tensors"][len(words)]
                        losses.append(eager(b, w)["loss"].item())
                        words.append(w)
                    else:
                        losses.append(eager(b)["loss"].item())
        torch.cuda.synchronize()
        assert len(losses) == 10 and len(words) == 8
        words_of[mode] = words
        finals[mode] = (losses, {k: v.detach().cpu().clone() for k, v in task.state_dict().items()})
        if gs is not None:
            gs.close()
    assert words_of["tensors"] == words_of["store"] and len(set(words_of["tensors"])) == 8
    for mode in ("store", "eager"):
        assert finals[mode][0] == finals["tensors"][0], (mode, finals[mode][0], finals["tensors"][0])
        for k, v in finals["tensors"][1].items():
            assert torch.equal(v, finals[mode][1][k]), (mode, k)


def test_logq_epoch_array_slices_are_aligned(tt, tmp_path):
    """DevicePairLoader.epoch_log_q: every batch's two slices start 16-byte aligned and hold the loader's own batches' log q."""
    from jodalrob_twotower_amd.data_loader import create_unified_bid_dataloaders
    from jodalrob_twotower_amd.sampling_bias import log_sampling_probs
    meta, schema, source = _pair_world(tt, tmp_path, 1001)
    loader, _ = create_unified_bid_dataloaders(source(), schema, batch_size=99, test_split=0.0, shuffle_seed=3, test_mode=True,
                                               pair_limit=1001, device=DEV)
    tp = loader.pairs
    loader.set_log_q((log_sampling_probs(tp[:, 0], len(loader.notice)), log_sampling_probs(tp[:, 1], len(loader.company))))
    order = loader.epoch_order()
    lq = loader.epoch_log_q(order)
    for k, lo in enumerate(range(0, 1001, 99)):
        m = min(99, 1001 - lo)
        b = loader.batch(order, lo)
        for side, s in (("notice", 0), ("company", 1)):
            sl = lq[k, s, :m]
            assert sl.data_ptr() % 16 == 0 and torch.equal(sl, b[side]["log_q"])
