"""Shared extra negatives of the in-batch softmax on the MI355X (include/twotower.h *_xneg entries).

1. The score node (_ScoreCEFn with x) against the float64 closed form of tests/_xneg_reference.py on the kernels' operands: bf16 and
   fp32, at the smallest shapes that cross every edge of the kernels -- one ragged extras tile; D padded to 256 and two tiles; the
   256-row J group on both sides; 513 rows; M > B -- plain, with logQ, with the mask, with both.  Loss, row sums (extras included),
   dN, dC, dX within the bounds tests/test_gpu_logq.py holds the mode to (dX under dC's: the extras add positive terms of the same
   kind to the same sums); colsum, diag and the positive / negative means BITWISE those of the call without extras.
2. Accuracy: an extra that is a bit copy of a row's positive does not cost the row its hit; one strictly closer does.
3. Two runs are bitwise equal.
4. Wiring: the eager task with batch["negatives"] is the node on the tower outputs, bit for bit; the loss differs from the batch
   without extras; the extras' table rows are trained; GraphedTrainStep.step equals the eager step bit for bit, the other captured
   steps refuse; the loader draws deterministically, keeps the pair order, and __iter__ / step_batches yield the same batches.
5. Refusals.
"""
import numpy as np
import pytest
import torch

from test_gpu_parity import DEV, tt, ctx_option, make_task, to_batch, load_state  # noqa: F401
from test_gpu_logq import BOUNDS, LOSS_ATOL, _sum_rtol, _nrel, _lq, _unit_rows, _pair_world
from test_gpu_mask_repeats import _small_task
from _mask_reference import ids
import _xneg_reference as XR

pytestmark = pytest.mark.gpu

# (B, M, D, T): what each crosses is in the module docstring; the temperatures are test_gpu_logq.SHAPES'
SHAPES = [(70, 1, 32, 1.0), (70, 33, 200, 0.5), (300, 263, 64, 2.0), (513, 32, 128, 0.05), (96, 300, 64, 1.0)]
VARIANTS = [("plain", None), ("lq", None), ("mask", "tile_edge"), ("mask", "groups"), ("mask", "heavy"), ("both", "tile_edge"),
            ("both", "groups")]


def _x_ids(ent_c, M, seed):
    """extras' company ids: the companies of tile-edge rows and of the batch's two ends, a random quarter repeating batch rows, the
    rest new"""
    B = ent_c.shape[0]
    g = np.random.default_rng(seed)
    ec = ent_c.cpu().numpy()
    ex = np.arange(M, dtype=np.int64) + 100 * B + 1000
    hit = g.permutation(M)[:max(M // 4, 1)]
    ex[hit] = ec[g.integers(0, B, len(hit))]
    for j, a in enumerate((0, 31, 32, 63, 64, 255, 256, B - 1)):
        if a < B:
            ex[(7 * j) % M] = ec[a]                          # (M = 1: the last one, row B - 1's company)
    return torch.tensor(ex, dtype=torch.int32, device=DEV)


def _case(B, M, D, variant, pattern):
    n, c, x = _unit_rows(B, D, 11 + B + D), _unit_rows(B, D, 29 + B + D), _unit_rows(M, D, 41 + M + D)
    ent = (None, None, None)
    if variant in ("mask", "both"):
        en, ec = ids(B, pattern, seed=B, device=DEV)
        ent = (en, ec, _x_ids(ec, M, M))
    lq = (None, None, None)
    if variant in ("lq", "both"):
        lq = (_lq(B, "random", 3 + B), _lq(B, "zipf", 5 + D), _lq(M, "random", 7 + M))
    return n, c, x, ent, lq


def _run(n, c, x, inv_t, mode, ent=(None, None, None), lq=(None, None, None), first_call=False, pair_w=None):
    from jodalrob_twotower_amd.two_tower_train_task import _ScoreCEFn
    n, c = n.clone().requires_grad_(True), c.clone().requires_grad_(True)
    x = None if x is None else x.clone().requires_grad_(True)
    loss, out8, rank = _ScoreCEFn.apply(n, c, inv_t, mode, first_call, False, None, None, None, lq[0], lq[1], ent[0], ent[1], pair_w, x,
                                        lq[2], ent[2])
    loss.backward()
    torch.cuda.synchronize()
    return (loss.detach().clone(), out8.detach().clone(), rank.clone(), n.grad.clone(), c.grad.clone(), None if x is None else x.grad.clone())


def _sums(n, c, x, inv_t, mode, ent, lq):
    """(rowsum, colsum, diag) of the entries with the extras and (colsum, diag) of the same call without them"""
    from jodalrob_twotower_amd import ops
    B, D = n.shape
    M = x.shape[0]
    e2 = ops.score_mask_ids(ent[0], ent[1], B, n.device) if ent[0] is not None else None
    ex = ops.score_xneg_ids(ent[2], M, n.device) if ent[2] is not None else None
    if mode == "fp32":
        rs, dg, rk, _ = ops.score_dir_fwd(n, c, inv_t, abs(inv_t), 0, True, lq_b=lq[1], ent=e2)
        cs = ops.score_dir_fwd(c, n, inv_t, abs(inv_t), 0, False, lq_b=lq[0], ent=e2)[0]
        dg0, cs0 = dg.clone(), cs.clone()
        ops.score_dir_fwd_xneg(n, x, inv_t, abs(inv_t), dg, rs, rk, lq_x=lq[2], ent_c=e2[1] if ex is not None else None, ent_x=ex)
        return rs, cs, dg, cs0, dg0
    sn = ops.score_unit_scale(inv_t)
    Np, Cp = ops.score_pack2_bf16(n, c, sn, 1.0)
    Xp = ops.score_pack_bf16(x, 1.0)
    r = ops.score_fwd_sym_xneg(Np, Cp, Xp, B, M, D, inv_t, abs(inv_t), e2, ex, lq[0], lq[1], lq[2], sn, True)
    r0 = ops._fwd_sym(Np, Cp, B, D, inv_t, abs(inv_t), sn, True, False, False, lq[0], lq[1], e2)
    return r[0].clone(), r[1].clone(), r[2].clone(), r0[1].clone(), r0[2].clone()


# ---- 1. the node against the reference ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["bf16", "fp32"])
@pytest.mark.parametrize("B,M,D,T", SHAPES)
@pytest.mark.parametrize("variant,pattern", VARIANTS)
def test_xneg_score_node_vs_f64(tt, mode, B, M, D, T, variant, pattern):
    inv_t = 1.0 / T
    n, c, x, ent, lq = _case(B, M, D, variant, pattern)
    loss, out8, rank, gn, gc, gx = _run(n, c, x, inv_t, mode, ent, lq)
    ref_loss, ref_gn, ref_gc, ref_gx = XR.reference(n, c, x, inv_t, mode, *ent, *lq)
    lb, gb = BOUNDS[mode]
    fl = inv_t / (2.0 * B)
    figs = dict(loss=abs(loss.item() - ref_loss) / abs(ref_loss), dN=_nrel(gn, ref_gn, fl), dC=_nrel(gc, ref_gc, fl), dX=_nrel(gx, ref_gx, fl))
    rs, cs, dg, cs0, dg0 = _sums(n, c, x, inv_t, mode, ent, lq)
    ref_rs = XR.ref_rowsum(n, c, x, inv_t, mode, *ent, *lq)
    figs["rowsum"] = float(((rs.double() - ref_rs).abs() / ref_rs).max())
    print(mode, (B, M, D, T), variant, pattern, figs)
    assert abs(loss.item() - ref_loss) <= lb * abs(ref_loss) + LOSS_ATOL, (loss.item(), ref_loss)
    assert figs["rowsum"] <= _sum_rtol(mode, inv_t), figs
    assert figs["dN"] <= gb and figs["dC"] <= gb and figs["dX"] <= gb, figs
    # what the extras do not enter is bit for bit the call's without them
    assert torch.equal(cs, cs0) and torch.equal(dg, dg0)
    loss0, out8_0, rank0, _, _, _ = _run(n, c, None, inv_t, mode, ent, lq)
    assert loss.item() != loss0.item()
    for k in (2, 3, 4, 6):
        assert out8[k].item() == out8_0[k].item(), (k, out8, out8_0)
    # the extras can only take hits away
    assert bool(((rank != 0) | (rank0 == 0)).all())
    if variant in ("mask", "both"):                          # the mask bites: some extra is some row's own company
        assert bool((ent[1][:, None] == ent[2][None, :]).any())


# ---- 2. accuracy semantics ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["bf16", "fp32"])
@pytest.mark.parametrize("B,M,D", [(70, 33, 32), (300, 40, 200)])
def test_xneg_accuracy_ties_and_closer_extras(tt, mode, B, M, D):
    n = _unit_rows(B, D, 3)
    c = n + 0.3 * _unit_rows(B, D, 4)                        # every row scores a hit in the batch
    c = c / c.norm(dim=1, keepdim=True)
    x = _unit_rows(M, D, 5)
    _, out8_0, rank0, _, _, _ = _run(n, c, None, 1.0, mode)
    assert out8_0[1].item() == 1.0 and int(rank0.abs().sum()) == 0
    rows = [0, 31, 32, B - 1]
    xt = x.clone()
    for j, a in enumerate(rows):
        xt[(j * 9) % M] = c[a]                               # bit copies of positives: ties, and an extra sits behind the positive
    _, out8, rank, _, _, _ = _run(n, c, xt, 1.0, mode)
    assert out8[1].item() == 1.0 and int(rank.abs().sum()) == 0
    xc = x.clone()
    xc[M - 1] = n[rows[1]]                                   # strictly closer than the positive: <n, n> = 1 > <n, c>
    xc[0] = n[rows[3]]
    _, out8, rank, _, _, _ = _run(n, c, xc, 1.0, mode)
    lost = torch.zeros(B, dtype=torch.bool, device=DEV)
    lost[[rows[1], rows[3]]] = True
    assert torch.equal(rank != 0, lost)
    assert out8[1].item() == np.float32(B - 2) / np.float32(B)
    for k in (2, 3, 4, 6):
        assert out8[k].item() == out8_0[k].item()


# ---- 3. reproducibility ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["bf16", "fp32"])
def test_xneg_runs_are_bit_identical(tt, mode):
    B, M, D, T = SHAPES[2]
    n, c, x, ent, lq = _case(B, M, D, "both", "groups")
    a = _run(n, c, x, 1.0 / T, mode, ent, lq)
    b = _run(n, c, x, 1.0 / T, mode, ent, lq)
    for u, v in zip(a, b):
        assert torch.equal(u, v)


# ---- 4. wiring ---------------------------------------------------------------------------------------------------------------------
def _with_negatives(b, M, seed, log_q=False, entity=False):
    """batch b plus M extras: company rows drawn from b's own company side (features and ids), as a loader's would be"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    B = b["company"]["dense"].shape[0]
    K = len(b["company"]["kjt"].keys())
    pick = torch.randint(0, B, (M,), generator=g, device=DEV)
    from jodalrob_twotower_amd.kjt import KeyedJaggedTensor
    neg = {"dense": b["company"]["dense"][pick] + 0.25, "kjt": KeyedJaggedTensor(b["company"]["kjt"].keys(),
                                                                                 b["company"]["kjt"].values().view(B, K)[pick].reshape(-1))}
    if log_q:
        neg["log_q"] = -6.0 * torch.rand(M, generator=g, device=DEV)
    if entity:
        neg["entity"] = pick.to(torch.int32)
    return dict(b, negatives=neg)


@pytest.mark.parametrize("score_dtype", ["bf16", "fp32"])
def test_xneg_eager_task_is_the_node_on_the_tower_outputs(tt, manifest, score_dtype):
    from jodalrob_twotower_amd.towers import run_towers
    from jodalrob_twotower_amd.kjt import KeyedJaggedTensor
    task, b, B = _small_task(tt, manifest, score_dtype=score_dtype)
    M = 37
    g = torch.Generator(device=DEV).manual_seed(1)
    b = {"notice": dict(b["notice"], log_q=-5.0 * torch.rand(B, generator=g, device=DEV)),
         "company": dict(b["company"], log_q=-5.0 * torch.rand(B, generator=g, device=DEV), entity=torch.arange(B, dtype=torch.int32, device=DEV))}
    bn = _with_negatives(b, M, 2, log_q=True, entity=True)
    res = task(bn, return_metrics=True)
    res["loss"].backward()
    grads = {k: p.grad.clone() for k, p in task.named_parameters() if p.grad is not None}
    # the same towers by hand: ONE company pass over the B + M rows, then the node
    task.zero_grad(set_to_none=True)
    model = task.two_tower_model
    both = {"dense": torch.cat([b["company"]["dense"], bn["negatives"]["dense"]], 0),
            "kjt": KeyedJaggedTensor(b["company"]["kjt"].keys(), torch.cat([b["company"]["kjt"].values(), bn["negatives"]["kjt"].values()], 0))}
    ne, cx = run_towers([model.notice_tower, model.company_tower], [b["notice"], both])
    from jodalrob_twotower_amd.two_tower_train_task import _ScoreCEFn
    loss, out8, _ = _ScoreCEFn.apply(ne, cx[:B], 1.0 / float(task.temperature), score_dtype, False, False, None, None, None,
                                     b["notice"]["log_q"], b["company"]["log_q"], None, b["company"]["entity"], None, cx[B:],
                                     bn["negatives"]["log_q"], bn["negatives"]["entity"])
    loss.backward()
    assert torch.equal(loss, res["loss"]) and torch.equal(out8[1], res["accuracy"])
    for k, p in task.named_parameters():
        if p.grad is not None:
            assert torch.equal(p.grad, grads[k]), k
    # and the extras matter
    with torch.no_grad():
        assert task(bn).item() != task(b).item()


def test_xneg_trains_the_extras_table_rows(tt, manifest):
    """a company id that only an extra carries: its embedding row moves in an eager step, a row nobody carries does not; on the notice
    side of the same store a row the batch carries moves too, and one nobody carries does not"""
    from jodalrob_twotower_amd.optim import FusedAdam
    from jodalrob_twotower_amd.kjt import KeyedJaggedTensor
    task, b, B = _small_task(tt, manifest, score_dtype="bf16")
    emb = task.two_tower_model.company_tower.categorical_embedder
    key0 = emb.keys[0]
    K = len(emb.keys)
    V = emb.embeddings[key0].weight.shape[0]
    assert V >= 3
    only_extra, nobody = V - 2, V - 1
    vb = b["company"]["kjt"].values().clone().view(B, K)
    vb[:, 0] %= V - 2                                        # the batch's companies keep off the two rows
    b = dict(b, company=dict(b["company"], kjt=KeyedJaggedTensor(b["company"]["kjt"].keys(), vb.reshape(-1))))
    bn = _with_negatives(b, 5, 3)
    v = bn["negatives"]["kjt"].values().clone().view(5, K)
    v[2, 0] = only_extra
    bn["negatives"]["kjt"] = KeyedJaggedTensor(b["company"]["kjt"].keys(), v.reshape(-1))
    before = emb.embeddings[key0].weight.detach().clone()
    # the notice side of the same store: an id the batch carries, and one nobody carries
    nemb = task.two_tower_model.notice_tower.categorical_embedder
    nkey, Kn = nemb.keys[-1], len(nemb.keys)
    n_ids = bn["notice"]["kjt"].values().view(B, Kn)[:, -1]
    Vn = nemb.embeddings[nkey].weight.shape[0]
    n_carried = int(n_ids[0])
    n_nobody = next(i for i in range(Vn) if not bool((n_ids == i).any()))
    assert 0 <= n_carried < Vn
    n_before = nemb.embeddings[nkey].weight.detach().clone()
    opt = FusedAdam.for_task(task, lr=1e-2, weight_decay=0.0)
    opt.zero_grad()
    task(bn).backward()
    opt.step()
    torch.cuda.synchronize()
    after = emb.embeddings[key0].weight.detach()
    assert not torch.equal(after[only_extra], before[only_extra])
    assert torch.equal(after[nobody], before[nobody])
    n_after = nemb.embeddings[nkey].weight.detach()
    assert not torch.equal(n_after[n_carried], n_before[n_carried])
    assert torch.equal(n_after[n_nobody], n_before[n_nobody])


def _decorated(b, B, seed):
    """b with log q on both sides and company ids: the extras then carry both too"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    return {"notice": dict(b["notice"], log_q=-5.0 * torch.rand(B, generator=g, device=DEV)),
            "company": dict(b["company"], log_q=-5.0 * torch.rand(B, generator=g, device=DEV),
                            entity=torch.randint(0, B // 2, (B,), generator=g, device=DEV, dtype=torch.int32))}


def _three_steps(tt, manifest, mode, M, decorated, B=64, both_ids=False, after=None):
    """(per-step (loss, accuracy), the final state) of three FusedAdam steps on batches whose extras differ: eager, or
    GraphedTrainStep.step(batch); after(gs, b, bs): called on the captured step before it is closed"""
    from jodalrob_twotower_amd.graph import GraphedTrainStep
    from jodalrob_twotower_amd.optim import FusedAdam
    task, b, B = _small_task(tt, manifest, B=B, score_dtype="bf16")
    if decorated:
        b = _decorated(b, B, 11)
    if both_ids:
        b["notice"]["entity"] = torch.randint(0, B // 2, (B,), generator=torch.Generator(device=DEV).manual_seed(12), device=DEV, dtype=torch.int32)
    bs = [_with_negatives(b, M, 20 + k, log_q=decorated, entity=decorated) for k in range(3)]
    opt = FusedAdam.for_task(task, lr=1e-2, weight_decay=1e-5)
    gs = GraphedTrainStep(task, opt, bs[0], warmup=1) if mode == "graph" else None
    losses = []
    for bk in bs:
        if gs is None:
            opt.zero_grad()
            r = task(bk, return_metrics=True)
            r["loss"].backward()
            opt.step()
        else:
            r = gs.step(bk)
        losses.append((r["loss"].item(), r["accuracy"].item()))
    torch.cuda.synchronize()
    state = {k: v.detach().cpu().clone() for k, v in task.state_dict().items()}
    if gs is not None:
        if after is not None:
            after(gs, b, bs)
        gs.close()
    return losses, state


def _assert_graph_is_eager(finals):
    assert finals["graph"][0] == finals["eager"][0], (finals["graph"][0], finals["eager"][0])
    assert len(set(finals["eager"][0])) == 3
    for k, v in finals["eager"][1].items():
        assert torch.equal(v, finals["graph"][1][k]), k


@pytest.mark.parametrize("decorated", [False, True])
def test_xneg_graphed_step_equals_eager(tt, manifest, decorated):
    """three steps on batches whose extras differ, FusedAdam: GraphedTrainStep.step(batch) (static M-row buffers, the plain-copy
    hand-over) against the eager step, bit for bit -- per-step losses and accuracies, every weight and table row after them"""
    M = 37

    def refusals(gs, b, bs):
        # a step captured with extras refuses a batch without them, another M, and the store-fed hand-over
        with pytest.raises(ValueError, match="negatives mismatch"):
            gs.step(b)
        with pytest.raises(ValueError, match="one M"):
            gs.step(_with_negatives(b, M + 1, 5, log_q=decorated, entity=decorated))
        with pytest.raises(NotImplementedError, match="negatives"):
            gs.step_from_store(None, None, None)
    _assert_graph_is_eager({mode: _three_steps(tt, manifest, mode, M, decorated, after=refusals) for mode in ("eager", "graph")})


WIDEST_LAUNCHES = 64               # GraphedTrainStep.library_launches of the case below, read off the commit before the hand-over's
                                   # host code was folded into one table walk


def test_xneg_widest_handover_is_two_copy_launches(tt, manifest, monkeypatch):
    """the widest hand-over -- extras that carry log_q and entity, log_q and entity on BOTH sides: 13 copy segments (4 of the extras, 2
    + 2 of the sides' terms, 4 of the sides, the scalars), more than one tt_copy_multi launch takes -- at B = 40, M = 24 (neither a
    multiple of the 32-wide tiles): bit for bit the eager steps, two copy launches per step(), and as many library launches per step
    as before"""
    from jodalrob_twotower_amd import ops
    calls, seen = [], {}
    real = ops.copy_multi

    def counting(pairs):
        calls.append(len(pairs))
        return real(pairs)

    def widest(gs, b, bs):
        monkeypatch.setattr(ops, "copy_multi", counting)
        gs.step(bs[0])
        monkeypatch.setattr(ops, "copy_multi", real)
        seen["launches"] = gs.library_launches
    finals = {mode: _three_steps(tt, manifest, mode, 24, True, B=40, both_ids=True, after=widest) for mode in ("eager", "graph")}
    print(f"widest hand-over: copy_multi segments per launch {calls}, library_launches {seen['launches']}")
    _assert_graph_is_eager(finals)
    assert calls == [8, 5]
    assert seen["launches"] == WIDEST_LAUNCHES


def test_xneg_other_captured_steps_refuse(tt, manifest):
    from jodalrob_twotower_amd.graph import GraphedTrainStep
    from jodalrob_twotower_amd.unrolled import UnrolledTrainStep
    from jodalrob_twotower_amd.segmented import SegmentedTrainStep
    from jodalrob_twotower_amd.optim import FusedAdam
    task, b, B = _small_task(tt, manifest, score_dtype="bf16")
    bn = _with_negatives(b, 8, 4)
    opt = FusedAdam.for_task(task, lr=1e-2)
    for cls in (UnrolledTrainStep, SegmentedTrainStep):
        with pytest.raises(NotImplementedError, match="negatives"):
            cls(task, opt, bn)
    gs = GraphedTrainStep(task, opt, b, warmup=1)            # captured without extras: refuses a batch that carries them
    with pytest.raises(ValueError, match="negatives mismatch"):
        gs.step(bn)
    gs.step(b)
    gs.close()


def test_xneg_loader_draws_deterministically_and_keeps_the_pair_order(tt, tmp_path):
    from jodalrob_twotower_amd.data_loader import create_unified_bid_dataloaders, DevicePairLoader
    from jodalrob_twotower_amd.sampling_bias import log_sampling_probs
    P, B, M = 333, 64, 10
    meta, schema, source = _pair_world(tt, tmp_path, P)
    base, _ = create_unified_bid_dataloaders(source(), schema, batch_size=B, test_split=0.0, shuffle_seed=7, test_mode=True, pair_limit=P,
                                             device=DEV)
    pairs = base.pairs.cpu().numpy()
    lq = (log_sampling_probs(base.pairs[:, 0], len(base.notice)), log_sampling_probs(base.pairs[:, 1], len(base.company)))

    def loader(M, pool=None):
        return DevicePairLoader(base.notice, base.company, pairs, B, shuffle=True, seed=7, log_q=lq, mask_repeats=True, extra_negatives=M,
                                negative_pool=pool)
    plain, a, a2 = list(loader(0)), list(loader(M)), list(loader(M))
    assert len(a) == len(plain) == 6
    for p, u, v in zip(plain, a, a2):
        for side in ("notice", "company"):                  # the pair order is the one without extras
            assert torch.equal(p[side]["entity"], u[side]["entity"]) and torch.equal(p[side]["dense"], u[side]["dense"])
        assert "negatives" not in p
        nu, nv = u["negatives"], v["negatives"]
        assert nu["dense"].shape == (M, p["company"]["dense"].shape[1]) and nu["entity"].dtype == torch.int32
        assert torch.equal(nu["entity"], nv["entity"]) and torch.equal(nu["dense"], nv["dense"])            # the same seed: the same draw
        assert torch.equal(nu["kjt"].values(), nv["kjt"].values())
        assert torch.equal(nu["dense"], base.company.dense[nu["entity"].long()])
        assert torch.equal(nu["log_q"], torch.full((M,), -float(np.log(len(base.company))), dtype=torch.float32, device=DEV))
    assert not torch.equal(a[0]["negatives"]["entity"], a[1]["negatives"]["entity"])
    # a pool: every extra comes from it, log q = log(1 / pool size)
    pool = torch.tensor([3, 5, 8, 13, 21], dtype=torch.int64, device=DEV)
    for u in loader(M, pool):
        assert bool(torch.isin(u["negatives"]["entity"].long(), pool).all())
        assert torch.equal(u["negatives"]["log_q"], torch.full((M,), -float(np.log(5)), dtype=torch.float32, device=DEV))
    # __iter__ and step_batches yield the same batches (no captured step: every batch through the eager callable)
    it, sb = list(loader(M)), list(loader(M).step_batches(None, eager_step=lambda b: b))
    assert len(it) == len(sb)
    for u, v in zip(it, sb):
        for side in ("notice", "company", "negatives"):
            assert torch.equal(u[side]["dense"], v[side]["dense"]) and torch.equal(u[side]["entity"], v[side]["entity"])
            assert torch.equal(u[side]["kjt"].values(), v[side]["kjt"].values()) and torch.equal(u[side]["log_q"], v[side]["log_q"])
    with pytest.raises(ValueError, match="int64"):
        loader(M, pool.int())
    with pytest.raises(KeyError):
        loader(M, torch.tensor([len(base.company)], device=DEV))
    with pytest.raises(ValueError, match=">= 0"):
        loader(-1)
    with pytest.raises(ValueError, match="pair_weight"):
        DevicePairLoader(base.notice, base.company, pairs, B, shuffle=True, pair_weight=torch.ones(P), extra_negatives=M)


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------
def test_xneg_refusals(tt, manifest):
    from jodalrob_twotower_amd import ops
    B, M, D = 64, 9, 32
    n, c, x = _unit_rows(B, D, 1), _unit_rows(B, D, 2), _unit_rows(M, D, 3)
    en, ec = ids(B, "groups", device=DEV)
    ex = _x_ids(ec, M, 1)
    for mode in ("fp8", "bf16x3"):
        with pytest.raises(ValueError, match=mode):
            _run(n, c, x, 1.0, mode)
    with pytest.raises(ValueError, match="pair weights"):
        _run(n, c, x, 1.0, "bf16", pair_w=torch.ones(B, device=DEV))
    with pytest.raises(ValueError, match="M >= 1"):
        _run(n, c, x[:0], 1.0, "bf16")
    with pytest.raises(ValueError, match=f"{D}"):
        _run(n, c, _unit_rows(M, D + 1, 4), 1.0, "bf16")
    with pytest.raises(TypeError, match="int32"):
        _run(n, c, x, 1.0, "bf16", (en, ec, ex.long()))
    with pytest.raises(ValueError, match="shape"):
        _run(n, c, x, 1.0, "bf16", (en, ec, ex[:-1]))
    with pytest.raises(ValueError, match="ent_c"):
        _run(n, c, x, 1.0, "bf16", (en, None, ex))
    lq = _lq(B, "random", 3)
    with pytest.raises(TypeError, match="float32"):
        _run(n, c, x, 1.0, "bf16", lq=(lq, lq, _lq(M, "random", 4).double()))
    with pytest.raises(ValueError, match="shape"):
        _run(n, c, x, 1.0, "fp32", lq=(lq, lq, _lq(M + 1, "random", 4)))
    with pytest.raises(ValueError, match="not corrected"):
        _run(n, c, x, 1.0, "bf16", lq=(None, None, _lq(M, "random", 4)))
    with pytest.raises(ValueError, match="2/T"):
        _run(n, c, x, 1.0 / 0.049, "bf16", lq=(lq, lq, None))
    _run(n, c, x, 1.0 / 0.049, "bf16")                       # without logQ the plain limit (2/T <= 80) holds
    Np, Cp = ops.score_pack2_bf16(n, c, 1.0, 1.0)
    with pytest.raises(ValueError, match="M must be"):
        ops.score_fwd_sym_xneg(Np, Cp, Np, B, 0, D, 1.0, 1.0)
    # the task
    task, b, Bt = _small_task(tt, manifest, score_dtype="bf16")
    bn = _with_negatives(b, 6, 5)
    for sd in ("fp8", "bf16x3"):
        task.score_dtype = sd
        with pytest.raises(ValueError, match=sd):
            task(bn)
    task.score_dtype = "bf16"
    for dense in (tt.TwoTowerTrainTask(task.two_tower_model, label_smoothing=0.1, score_dtype="bf16"),
                  tt.TwoTowerTrainTask(task.two_tower_model, loss_type="cosine_embedding", score_dtype="bf16")):
        with pytest.raises(ValueError, match="dense loss"):
            dense(bn)
    with pytest.raises(ValueError, match="pair_weight"):
        task(dict(bn, pair_weight=torch.ones(Bt, device=DEV)))
    with pytest.raises(ValueError, match="negatives"):
        task.forward_with_ranks(bn)

    def neg(**kw):
        return dict(b, negatives=dict(bn["negatives"], **kw))
    with pytest.raises(ValueError, match="M >= 1"):
        task(neg(dense=bn["negatives"]["dense"][:0]))
    with pytest.raises(ValueError, match="company-side input"):
        task(neg(dense=bn["negatives"]["dense"][:, :-1]))
    with pytest.raises(ValueError, match="company-side input"):
        task(neg(dense=bn["negatives"]["dense"].double()))
    with pytest.raises(ValueError, match="is on cpu"):
        task(neg(dense=bn["negatives"]["dense"].cpu()))
    with pytest.raises(ValueError, match="keys"):
        task(neg(kjt=b["notice"]["kjt"]))
    with pytest.raises(ValueError, match="needs batch"):
        task(neg(log_q=torch.zeros(6, device=DEV)))          # the batch is not corrected
    with pytest.raises(ValueError, match="needs batch"):
        task(neg(entity=torch.zeros(6, dtype=torch.int32, device=DEV)))
    bl = {"notice": b["notice"], "company": dict(b["company"], log_q=torch.zeros(Bt, device=DEV), entity=torch.arange(Bt, dtype=torch.int32, device=DEV)),
          "negatives": bn["negatives"]}
    with pytest.raises(ValueError, match="float32"):
        task(dict(bl, negatives=dict(bn["negatives"], log_q=torch.zeros(6, dtype=torch.float64, device=DEV))))
    with pytest.raises(ValueError, match="shape"):
        task(dict(bl, negatives=dict(bn["negatives"], entity=torch.zeros(7, dtype=torch.int32, device=DEV))))
    with pytest.raises(ValueError, match="is on cpu"):
        task(dict(bl, negatives=dict(bn["negatives"], entity=torch.zeros(6, dtype=torch.int32))))
    assert torch.isfinite(task(bl))                          # a corrected, masked batch whose extras carry neither: served
