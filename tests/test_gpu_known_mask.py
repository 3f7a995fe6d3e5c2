"""Masked cells of the in-batch softmax -- the known-pair mask -- on the MI355X (include/twotower.h *_cells entries).

1. The score node (_ScoreCEFn with cells) against the float64 closed form of tests/_known_mask_reference.py on the kernels' operands,
   at shapes that cross every edge -- one ragged tile, 513 rows, D padded to 256, M = 1, the 256-row J group on both sides, M > B --
   plain and with logQ, three cell patterns (tile edges, a random 3 %, a row and a column fully listed).  Loss, row sums, dN, dC, dX
   within the bounds tests/test_gpu_logq.py holds bf16 to; the cells bite.
2. Cleaning: duplicates, diagonal cells and cells out of range change no bit.  The plan itself against a host bucketing.
3. An empty list: loss, sums and diag bit for bit the call's without the entry at every shape; the gradients bit for bit where that
   call takes the b-split backward too (D <= 32 and D > 128 below the large-batch threshold).  At D in (32, 128] the plain entry takes
   its transposing form, whose sums run in another order: there dN / dC are bit for bit those of the plain b-split launch (the
   repeated-entity entry on all-distinct ids), within the node's bound of the plain call's, and dX bit for bit.
4. Two runs, and a permuted list, are bit identical.
5. Wiring: the eager task is the node on the tower outputs; GraphedTrainStep.step equals the eager step bit for bit over three steps
   with FusedAdam and extras while L varies (0 and the capacity included); capacity + 1 cells and every refusal raise; the loader's
   cells equal brute force and __iter__ / step_batches yield the same batches.
"""
import numpy as np
import pytest
import torch

from test_gpu_parity import DEV, tt, ctx_option, make_task, to_batch, load_state  # noqa: F401
from test_gpu_logq import BOUNDS, LOSS_ATOL, _sum_rtol, _nrel, _lq, _unit_rows, _pair_world
from test_gpu_mask_repeats import _small_task
from test_gpu_extra_negatives import _with_negatives
import _known_mask_reference as KR

pytestmark = pytest.mark.gpu

SHAPES = [(70, 0, 32, 1.0), (513, 0, 128, 0.05), (70, 1, 32, 1.0), (70, 33, 200, 0.5), (300, 263, 64, 2.0), (96, 300, 64, 1.0),
          # every class of D with and without extras at a ragged B (four tiles, the last one partial)
          (97, 0, 64, 1.0), (97, 0, 200, 1.0), (97, 40, 96, 1.0)]
PATTERNS = ["edges", "random", "heavy"]


def _cells(B, M, pattern, seed=0):
    """int64 numpy [L, 2] of the named pattern (may hold the diagonal: the entries ignore it)"""
    if pattern == "edges":
        pts = sorted({p for p in (0, 31, 32, 63, 64, B - 1) if 0 <= p < B})
        cols = pts + sorted({B + q for q in (0, 31, 32, M - 1) if 0 <= q < M})
        return np.array([(a, j) for a in pts for j in cols], dtype=np.int64)
    if pattern == "random":
        g = np.random.default_rng(seed + B + M)
        L = max(int(0.03 * B * (B + M)), 4)
        return np.stack([g.integers(0, B, L), g.integers(0, B + M, L)], 1)
    if pattern == "heavy":                                     # row 33 loses every negative, column 5 every row but its own
        return np.array([(33, j) for j in range(B + M)] + [(a, 5) for a in range(B)], dtype=np.int64)
    raise ValueError(pattern)


def _dev_cells(cells):
    return torch.as_tensor(np.asarray(cells, dtype=np.int64).reshape(-1, 2), dtype=torch.int32, device=DEV)


def _case(B, M, D, lq, kinds=("random", "zipf", "random")):
    """kinds: the log q of the notices, the companies and the extras (tests/test_gpu_logq.py's _lq).  "random" spreads the sampling
    weights over e^30 and plants both clamps: a few columns then carry a row's whole sum, and a sparse pattern that misses them moves
    no f32 bit of the loss -- the few-cell pattern takes "zipf" (a spread of e^7) on every side, so that each of its cells counts"""
    n, c = _unit_rows(B, D, 11 + B + D), _unit_rows(B, D, 29 + B + D)
    x = _unit_rows(M, D, 41 + M + D) if M else None
    q = (_lq(B, kinds[0], 3 + B), _lq(B, kinds[1], 5 + D), _lq(M, kinds[2], 7 + M) if M else None) if lq else (None, None, None)
    return n, c, x, q


def _run(n, c, x, inv_t, cells, lq=(None, None, None), mode="bf16", count=None, ent=(None, None), pair_w=None):
    from jodalrob_twotower_amd.two_tower_train_task import _ScoreCEFn
    n, c = n.clone().requires_grad_(True), c.clone().requires_grad_(True)
    x = None if x is None else x.clone().requires_grad_(True)
    loss, out8, rank = _ScoreCEFn.apply(n, c, inv_t, mode, False, False, None, None, None, lq[0], lq[1], ent[0], ent[1], pair_w, x, lq[2],
                                        None, cells, count)
    loss.backward()
    torch.cuda.synchronize()
    return (loss.detach().clone(), out8.detach().clone(), rank.clone(), n.grad.clone(), c.grad.clone(), None if x is None else x.grad.clone())


def _sums(n, c, x, inv_t, cells, lq):
    """(rowsum, colsum, diag) of the forward entry with cells"""
    from jodalrob_twotower_amd import ops
    B, D = n.shape
    M = 0 if x is None else x.shape[0]
    sn = ops.score_unit_scale(inv_t)
    Np, Cp = ops.score_pack2_bf16(n, c, sn, 1.0)
    Xp = ops.score_pack_bf16(x, 1.0) if M else None
    plan = ops.score_cells_plan(cells, B, M)
    r = ops.score_fwd_sym_cells(Np, Cp, B, D, inv_t, abs(inv_t), plan, Xp, M, lq[0], lq[1], lq[2], sn, True)
    return r[0].clone(), r[1].clone(), r[2].clone()


def _sums_without(n, c, x, inv_t, lq):
    """(rowsum, colsum, diag) of the same call without the entry"""
    from jodalrob_twotower_amd import ops
    B, D = n.shape
    sn = ops.score_unit_scale(inv_t)
    Np, Cp = ops.score_pack2_bf16(n, c, sn, 1.0)
    if x is None:
        r = ops._fwd_sym(Np, Cp, B, D, inv_t, abs(inv_t), sn, True, False, False, lq[0], lq[1])
    else:
        r = ops.score_fwd_sym_xneg(Np, Cp, ops.score_pack_bf16(x, 1.0), B, x.shape[0], D, inv_t, abs(inv_t), None, None, lq[0], lq[1], lq[2], sn, True)
    return r[0].clone(), r[1].clone(), r[2].clone()


# ---- 1. the node against the reference -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,M,D,T", SHAPES)
@pytest.mark.parametrize("variant", ["plain", "lq"])
@pytest.mark.parametrize("pattern", PATTERNS)
def test_cells_score_node_vs_f64(tt, B, M, D, T, variant, pattern):
    inv_t = 1.0 / T
    n, c, x, lq = _case(B, M, D, variant == "lq", ("zipf",) * 3 if pattern == "edges" else ("random", "zipf", "random"))
    cells = _cells(B, M, pattern)
    om = KR.clean_cells(cells, B, M)
    assert len(om) > 0 and (M == 0 or bool((om[:, 1] >= B).any()))          # the cells bite: some survive, some on the extras
    dc = _dev_cells(cells)
    loss, out8, rank, gn, gc, gx = _run(n, c, x, inv_t, dc, lq)
    ref_loss, ref_gn, ref_gc, ref_gx = KR.reference(n, c, x, cells, inv_t, "bf16", *lq)
    lb, gb = BOUNDS["bf16"]
    fl = inv_t / (2.0 * B)
    figs = dict(loss=abs(loss.item() - ref_loss) / abs(ref_loss), dN=_nrel(gn, ref_gn, fl), dC=_nrel(gc, ref_gc, fl))
    if M:
        figs["dX"] = _nrel(gx, ref_gx, fl)
    rs, cs, dg = _sums(n, c, x, inv_t, dc, lq)
    ref_rs = KR.ref_rowsum(n, c, x, cells, inv_t, "bf16", *lq)
    figs["rowsum"] = float(((rs.double() - ref_rs).abs() / ref_rs).max())
    print((B, M, D, T), variant, pattern, len(om), figs)
    assert np.isfinite(loss.item())
    assert abs(loss.item() - ref_loss) <= lb * abs(ref_loss) + LOSS_ATOL, (loss.item(), ref_loss)
    assert figs["rowsum"] <= _sum_rtol("bf16", inv_t), figs
    assert all(figs[k] <= gb for k in figs if k.startswith("d")), figs
    # metrics stay on the raw scores; the loss moves
    loss0, out8_0, rank0, _, _, _ = _run(n, c, x, inv_t, None, lq)
    assert loss.item() != loss0.item()
    assert torch.equal(out8[1:5], out8_0[1:5]) and out8[6].item() == out8_0[6].item() and torch.equal(rank, rank0)
    assert torch.equal(dg, _sums_without(n, c, x, inv_t, lq)[2])


# ---- 2. cleaning, and the plan ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,M,D,T", [SHAPES[0], SHAPES[3], SHAPES[4]])
def test_cells_cleaning_changes_no_bit(tt, B, M, D, T):
    n, c, x, lq = _case(B, M, D, True)
    om = KR.clean_cells(_cells(B, M, "random"), B, M)
    g = np.random.default_rng(1)
    junk = np.array([[0, 0], [B - 1, B - 1], [31, 31], [-1, 3], [3, -1], [B, 0], [0, B + M], [2 ** 31 - 1, 1], [1, 2 ** 31 - 1], [-2 ** 31, 0]])
    dirty = np.concatenate([om, junk, om[g.integers(0, len(om), 40)]], 0)
    dirty = dirty[g.permutation(len(dirty))]
    a = _run(n, c, x, 1.0 / T, _dev_cells(om), lq)
    b = _run(n, c, x, 1.0 / T, _dev_cells(dirty), lq)
    for u, v in zip(a, b):
        assert (u is None and v is None) or torch.equal(u, v)


@pytest.mark.parametrize("B,M", [(70, 0), (70, 33), (300, 263), (96, 300)])
def test_cells_plan_equals_host_bucketing(tt, B, M):
    from jodalrob_twotower_amd import ops
    cells = np.concatenate([_cells(B, M, "random"), _cells(B, M, "edges"), [[0, 0], [-1, 2], [2, B + M]]], 0)
    cap = len(cells) + 50
    buf = torch.zeros((cap, 2), dtype=torch.int32, device=DEV)
    buf[:len(cells)] = _dev_cells(cells)
    buf[len(cells):] = 1                                       # (beyond the count: never read -- (1, 1) is a diagonal cell anyway)
    count = torch.tensor([len(cells)], dtype=torch.int32, device=DEV)
    off, codes = ops.score_cells_unpack(ops.score_cells_plan(buf, B, M, count=count), B, M)
    nT, nTx = (B + 31) // 32, (M + 31) // 32
    c = np.asarray(cells, dtype=np.int64)
    ok = (c[:, 0] >= 0) & (c[:, 0] < B) & (c[:, 1] >= 0) & (c[:, 1] < B + M) & (c[:, 1] != c[:, 0])
    c = c[ok]                                                  # duplicates stay: the plan keeps them
    jl = np.where(c[:, 1] < B, c[:, 1], c[:, 1] - B)
    pair = (c[:, 0] // 32) * (nT + nTx) + np.where(c[:, 1] < B, 0, nT) + jl // 32
    code = (c[:, 0] % 32) * 32 + jl % 32
    want_off = np.concatenate([[0], np.cumsum(np.bincount(pair, minlength=nT * (nT + nTx)))])
    assert off.tolist() == want_off.tolist()
    for p in np.unique(pair):
        assert sorted(codes[off[p]:off[p + 1]].tolist()) == sorted(code[pair == p].tolist()), p
    # the count is read on the device: a smaller one drops the tail
    count.fill_(7)
    off7, _ = ops.score_cells_unpack(ops.score_cells_plan(buf, B, M, count=count), B, M)
    assert int(off7[-1]) == int(ok[:7].sum())


# ---- 3. an empty list ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,M,D,T", SHAPES)
@pytest.mark.parametrize("variant", ["plain", "lq"])
def test_cells_empty_list_is_the_call_without_the_entry(tt, B, M, D, T, variant):
    n, c, x, lq = _case(B, M, D, variant == "lq")
    empty = torch.zeros((0, 2), dtype=torch.int32, device=DEV)
    a = _run(n, c, x, 1.0 / T, empty, lq)
    b = _run(n, c, x, 1.0 / T, None, lq)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])          # loss, metrics, ranks
    for u, v in zip(_sums(n, c, x, 1.0 / T, empty, lq), _sums_without(n, c, x, 1.0 / T, lq)):       # rowsum, colsum, diag
        assert torch.equal(u, v)
    if D <= 32 or D > 128:                                     # the plain entry's backward is the b-split form here too
        for u, v in zip(a[3:], b[3:]):
            assert (u is None and v is None) or torch.equal(u, v)
    else:
        # D in (32, 128]: the plain entry takes its transposing backward, whose sums over b run in another order than the b-split
        # form the issue asks of this entry at every shape -- the two calls' dN / dC cannot share their bits.  Held instead, so that no
        # shape goes without an assertion: (1) bit for bit the gradients of the plain B-SPLIT launch of these shapes -- the
        # repeated-entity entry on all-distinct ids, which masks nothing and runs the same tiles; (2) the plain call's gradients under
        # the bound the node is held to against f64 (each of the two is within it of the reference, so twice it); dX, whose launch
        # has one form, bit for bit
        ids = (torch.arange(B, dtype=torch.int32, device=DEV), torch.arange(B, dtype=torch.int32, device=DEV) + 7 * B)
        m = _run(n, c, x, 1.0 / T, None, lq, ent=ids)
        assert torch.equal(a[0], m[0]) and torch.equal(a[3], m[3]) and torch.equal(a[4], m[4])
        fl, gb = (1.0 / T) / (2.0 * B), BOUNDS["bf16"][1]
        figs = dict(dN=_nrel(a[3], b[3].double(), fl), dC=_nrel(a[4], b[4].double(), fl))
        print((B, M, D, T), variant, "empty list against the plain call", figs)
        assert figs["dN"] <= 2 * gb and figs["dC"] <= 2 * gb, figs
        if M:
            assert torch.equal(a[5], b[5]) and torch.equal(a[5], m[5])
    # a count of zero over a full buffer is the empty list as well
    full = _dev_cells(_cells(B, M, "random"))
    z = _run(n, c, x, 1.0 / T, full, lq, count=torch.zeros(1, dtype=torch.int32, device=DEV))
    for u, v in zip(a, z):
        assert (u is None and v is None) or torch.equal(u, v)


# ---- 4. reproducibility ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,M,D,T", [SHAPES[1], SHAPES[4]])
def test_cells_runs_and_permuted_lists_are_bit_identical(tt, B, M, D, T):
    n, c, x, lq = _case(B, M, D, True)
    cells = np.concatenate([_cells(B, M, "random"), _cells(B, M, "heavy")], 0)
    a = _run(n, c, x, 1.0 / T, _dev_cells(cells), lq)
    b = _run(n, c, x, 1.0 / T, _dev_cells(cells), lq)
    p = _run(n, c, x, 1.0 / T, _dev_cells(cells[np.random.default_rng(2).permutation(len(cells))]), lq)
    for u, v, w in zip(a, b, p):
        assert (u is None and v is None and w is None) or (torch.equal(u, v) and torch.equal(u, w))


# ---- 5. wiring -------------------------------------------------------------------------------------------------------------------------
def _batch_cells(B, M, L, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.stack([torch.randint(0, B, (L,), generator=g, device=DEV), torch.randint(0, B + M, (L,), generator=g, device=DEV)], 1).to(torch.int32)


def test_cells_eager_task_is_the_node_on_the_tower_outputs(tt, manifest):
    from jodalrob_twotower_amd.towers import run_towers
    from jodalrob_twotower_amd.kjt import KeyedJaggedTensor
    from jodalrob_twotower_amd.two_tower_train_task import _ScoreCEFn
    task, b, B = _small_task(tt, manifest, score_dtype="bf16")
    M = 37
    g = torch.Generator(device=DEV).manual_seed(1)
    b = {"notice": dict(b["notice"], log_q=-5.0 * torch.rand(B, generator=g, device=DEV)),
         "company": dict(b["company"], log_q=-5.0 * torch.rand(B, generator=g, device=DEV))}
    bn = dict(_with_negatives(b, M, 2, log_q=True), masked_cells=_batch_cells(B, M, 300, 3))
    res = task(bn, return_metrics=True)
    res["loss"].backward()
    grads = {k: p.grad.clone() for k, p in task.named_parameters() if p.grad is not None}
    task.zero_grad(set_to_none=True)
    model = task.two_tower_model
    both = {"dense": torch.cat([b["company"]["dense"], bn["negatives"]["dense"]], 0),
            "kjt": KeyedJaggedTensor(b["company"]["kjt"].keys(), torch.cat([b["company"]["kjt"].values(), bn["negatives"]["kjt"].values()], 0))}
    ne, cx = run_towers([model.notice_tower, model.company_tower], [b["notice"], both])
    loss, out8, _ = _ScoreCEFn.apply(ne, cx[:B], 1.0 / float(task.temperature), "bf16", False, False, None, None, None, b["notice"]["log_q"],
                                     b["company"]["log_q"], None, None, None, cx[B:], bn["negatives"]["log_q"], None, bn["masked_cells"])
    loss.backward()
    assert torch.equal(loss, res["loss"]) and torch.equal(out8[1], res["accuracy"])
    for k, p in task.named_parameters():
        if p.grad is not None:
            assert torch.equal(p.grad, grads[k]), k
    with torch.no_grad():                                      # the cells matter; without extras the task serves them too
        assert task(bn).item() != task({k: v for k, v in bn.items() if k != "masked_cells"}).item()
        plain = dict(b, masked_cells=_batch_cells(B, 0, 200, 4))
        assert task(plain).item() != task(b).item()


@pytest.mark.parametrize("log_q", [True, False])
def test_cells_graphed_step_equals_eager(tt, manifest, log_q):
    """three steps with FusedAdam and extras while the cell count varies -- L = 0, an odd L (a copy segment with a tail) and L = the
    capacity: GraphedTrainStep.step(batch) against the eager step, bit for bit"""
    from jodalrob_twotower_amd.graph import GraphedTrainStep
    from jodalrob_twotower_amd.optim import FusedAdam
    M, cap, finals = 37, 1100, {}
    for mode in ("eager", "graph"):
        task, b, B = _small_task(tt, manifest, score_dtype="bf16")
        if log_q:
            g = torch.Generator(device=DEV).manual_seed(11)
            b = {"notice": dict(b["notice"], log_q=-5.0 * torch.rand(B, generator=g, device=DEV)),
                 "company": dict(b["company"], log_q=-5.0 * torch.rand(B, generator=g, device=DEV))}
        bs = [dict(_with_negatives(b, M, 20 + k, log_q=log_q), masked_cells=_batch_cells(B, M, L, 30 + k)) for k, L in enumerate((301, 0, cap))]
        opt = FusedAdam.for_task(task, lr=1e-2, weight_decay=1e-5)
        gs = GraphedTrainStep(task, opt, bs[0], warmup=1, cell_capacity=cap) if mode == "graph" else None
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
        finals[mode] = (losses, {k: v.detach().cpu().clone() for k, v in task.state_dict().items()})
        if gs is not None:
            assert gs.cell_capacity == cap
            before = {k: v.detach().clone() for k, v in task.state_dict().items()}
            with pytest.raises(ValueError, match="cell_capacity"):
                gs.step(dict(bs[0], masked_cells=_batch_cells(B, M, cap + 1, 5)))
            with pytest.raises(ValueError, match="masked_cells mismatch"):
                gs.step({k: v for k, v in bs[0].items() if k != "masked_cells"})
            with pytest.raises(NotImplementedError, match="masked cells"):
                gs.step_from_store(None, None, None)
            torch.cuda.synchronize()
            for k, v in task.state_dict().items():             # a refused batch copied nothing and stepped nothing
                assert torch.equal(v, before[k]), k
            gs.close()
    assert finals["graph"][0] == finals["eager"][0], (finals["graph"][0], finals["eager"][0])
    assert len(set(finals["eager"][0])) == 3
    for k, v in finals["eager"][1].items():
        assert torch.equal(v, finals["graph"][1][k]), k


def test_cells_refusals(tt, manifest):
    from jodalrob_twotower_amd.graph import GraphedTrainStep
    from jodalrob_twotower_amd.unrolled import UnrolledTrainStep
    from jodalrob_twotower_amd.segmented import SegmentedTrainStep
    from jodalrob_twotower_amd.optim import FusedAdam
    from _mask_reference import ids
    B, M, D = 64, 9, 32
    n, c, x = _unit_rows(B, D, 1), _unit_rows(B, D, 2), _unit_rows(M, D, 3)
    cells = _batch_cells(B, M, 50, 1)
    en, ec = ids(B, "groups", device=DEV)
    for mode in ("fp32", "fp8", "bf16x3"):
        with pytest.raises(ValueError, match=mode):
            _run(n, c, x, 1.0, cells, mode=mode)
    with pytest.raises(ValueError, match="repeated-entity"):
        _run(n, c, None, 1.0, cells, ent=(en, ec))
    with pytest.raises(ValueError, match="pair weights"):
        _run(n, c, None, 1.0, cells, pair_w=torch.ones(B, device=DEV))
    with pytest.raises(TypeError, match="int32"):
        _run(n, c, None, 1.0, cells.long())
    with pytest.raises(ValueError, match="shape"):
        _run(n, c, None, 1.0, cells[:, 0])
    with pytest.raises(ValueError, match="is on cpu"):
        _run(n, c, None, 1.0, cells.cpu())
    # the task
    task, b, Bt = _small_task(tt, manifest, score_dtype="bf16")
    bc = dict(b, masked_cells=_batch_cells(Bt, 0, 40, 2))
    assert torch.isfinite(task(bc))
    with pytest.raises(ValueError, match="entity"):
        task({"notice": b["notice"], "company": dict(b["company"], entity=torch.arange(Bt, dtype=torch.int32, device=DEV)),
              "masked_cells": bc["masked_cells"]})
    with pytest.raises(ValueError, match="pair_weight"):
        task(dict(bc, pair_weight=torch.ones(Bt, device=DEV)))
    with pytest.raises(ValueError, match="masked_cells"):
        task.forward_with_ranks(bc)
    for sd in ("fp32", "fp8", "bf16x3"):
        task.score_dtype = sd
        with pytest.raises(ValueError, match=sd):
            task(bc)
    task.score_dtype = "bf16"
    for dense in (tt.TwoTowerTrainTask(task.two_tower_model, label_smoothing=0.1, score_dtype="bf16"),
                  tt.TwoTowerTrainTask(task.two_tower_model, loss_type="cosine_embedding", score_dtype="bf16")):
        with pytest.raises(ValueError, match="dense loss"):
            dense(bc)
    for bad in (bc["masked_cells"].long(), bc["masked_cells"][:, :1], bc["masked_cells"].cpu()):
        with pytest.raises(ValueError, match="masked_cells"):
            task(dict(b, masked_cells=bad))
    # the captured steps
    opt = FusedAdam.for_task(task, lr=1e-2)
    for cls in (UnrolledTrainStep, SegmentedTrainStep):
        with pytest.raises(NotImplementedError, match="masked cells"):
            cls(task, opt, bc)
    with pytest.raises(ValueError, match="cell_capacity"):
        GraphedTrainStep(task, opt, b, warmup=1, cell_capacity=64)          # no cells in the example
    with pytest.raises(ValueError, match="cell_capacity"):
        GraphedTrainStep(task, opt, bc, warmup=1, cell_capacity=39)         # fewer rows than the example's cells
    gs = GraphedTrainStep(task, opt, b, warmup=1)              # captured without cells: refuses a batch that carries them
    with pytest.raises(ValueError, match="masked_cells mismatch"):
        gs.step(bc)
    gs.step(b)
    gs.close()
    gs = GraphedTrainStep(task, opt, bc, warmup=1)             # the default capacity: four times the example's, at least 1024
    assert gs.cell_capacity == 1024
    gs.close()


def test_cells_loader_equals_brute_force_and_step_batches_equals_iter(tt, tmp_path):
    from jodalrob_twotower_amd.data_loader import create_unified_bid_dataloaders, DevicePairLoader
    from jodalrob_twotower_amd.sampling_bias import log_sampling_probs
    P, B, M = 333, 64, 24
    meta, schema, source = _pair_world(tt, tmp_path, P)
    base, _ = create_unified_bid_dataloaders(source(), schema, batch_size=B, test_split=0.0, shuffle_seed=7, test_mode=True, pair_limit=P,
                                             device=DEV)
    pairs = base.pairs.cpu().numpy()
    lq = (log_sampling_probs(base.pairs[:, 0], len(base.notice)), log_sampling_probs(base.pairs[:, 1], len(base.company)))
    # "mined" rows: each notice's table holds known companies of OTHER notices and some of its own (what a ceiling would let through)
    rng = np.random.default_rng(5)
    table = torch.as_tensor(pairs[rng.integers(0, P, (len(base.notice), 4)), 1].astype(np.int32), device=DEV)
    known = set(map(tuple, pairs.tolist()))

    def loader(mk=True):
        return DevicePairLoader(base.notice, base.company, pairs, B, shuffle=True, seed=7, log_q=lq, extra_negatives=M, mined=table,
                                hard_fraction=0.75, mask_known=mk)
    on, off = list(loader()), list(loader(False))
    assert len(on) == len(off) == 6
    n_in = n_x = 0
    order = loader().epoch_order().cpu().numpy()
    for k, (u, v) in enumerate(zip(on, off)):
        assert "masked_cells" not in v and torch.equal(u["notice"]["dense"], v["notice"]["dense"])      # the pair order and the draw stay
        rows = u["negatives"]["kjt"].values()
        assert torch.equal(rows, v["negatives"]["kjt"].values())
        sel = pairs[order[k * B:(k + 1) * B]]
        got =[tuple(r) for r in u["masked_cells"].cpu().tolist()]
        want_cols = _extras_rows(loader, k)
        want = KR.brute_cells(sel, want_cols, known, len(sel))
        assert got == want, k
        n_in += sum(1 for a, j in want if j < len(sel))
        n_x += sum(1 for a, j in want if j >= len(sel))
        assert u["masked_cells"].dtype == torch.int32 and u["masked_cells"].device.type == "cuda"
    assert n_in > 0 and n_x > 0
    # __iter__ and step_batches yield the same batches (no captured step: every batch through the eager callable)
    sb = list(loader().step_batches(None, eager_step=lambda b: b))
    assert len(sb) == len(on)
    for u, v in zip(on, sb):
        assert torch.equal(u["masked_cells"], v["masked_cells"]) and torch.equal(u["notice"]["dense"], v["notice"]["dense"])
        assert torch.equal(u["negatives"]["dense"], v["negatives"]["dense"])


def _extras_rows(loader, k):
    """the company rows of batch k's extras, from a fresh loader's own epoch draw (the same seed: the same draw)"""
    ld = loader()
    order = ld.epoch_order()
    return ld.epoch_negatives(order)[k].cpu().numpy()
