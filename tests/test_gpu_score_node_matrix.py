"""Every term combination the score node (_ScoreCEFn) accepts, run against ONE float64 model of the whole node
(tests/_score_node_reference.py), and every combination it refuses, on the MI355X.

The matrix is tests/test_score_terms_host.py's (DTYPES x every subset of TERMS x the extras' riders), imported so that the files cannot
drift.  Inputs are the term files' generators, composed by tests/_score_node_inputs.py (tests/test_score_node_reference_host.py checks
on the same function that every term and rider of every accepted combination moves the reference loss by 100 loss bounds at least).

1. Accepted combinations (42 per shape): loss, dN, dC, dX within the bounds tests/test_gpu_logq.py holds the uncorrected node of the
   mode to (fp8: tests/test_gpu_parity.py's rounded-oracle bounds at T >= 0.5), the sums within its _sum_rtol; what a term does not enter
   -- diag, out8[2, 3, 4, 6], with extras colsum -- bit for bit; accuracy within 2 / B.
2. Refused combinations: ValueError with exactly the table's text, no launch.  Unequal row counts: refused by the node, no launch.
3. The first call (want_col_rank=True) at the widest combination of each dtype and at the plain call.
4. One-sided ids, alone and with extras.

Shapes (B, M, D, T), the smallest that cross the sweep's edges (argued in tests/test_gpu_extra_negatives.py and test_gpu_known_mask.py):
(70, 33, 200, 0.5) -- ragged row tile, ragged extras tile, D padded to 256; (300, 263, 64, 2.0) -- the 256-row J group on both sides,
more than one extras tile.  M counts only where extras are present.
"""
import contextlib
import functools
import time

import numpy as np
import pytest
import torch

import oracle_np as O
import test_gpu_logq as GL
from test_gpu_parity import tt, _rel  # noqa: F401
from test_gpu_logq import BOUNDS, LOSS_ATOL, _nrel, _sum_rtol
import _score_node_reference as NR
from _score_node_inputs import (ACCEPTED, DROPS, DTYPES, FP8_BOUNDS, ONE_SIDED, REFUSED, RIDERS, SHAPES, TERMS, _expected, _inputs, _name, _ref_kw,
                                loss_bound, teeth)

pytestmark = pytest.mark.gpu

# ---- running the node ------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _recorded(n):
    """The diag the node's forward formed (no output carries it), taken where the forward gets it: ops._sym_fwd's SymOut.diag, or on the
    f32 path the second result of the ops.score_dir_fwd call whose first operand is the node's own n (the row direction; the column
    direction's call has c there).  This leans on how forward is written: if it stops calling either function, no diag is recorded and
    _run's asserts say so."""
    from jodalrob_twotower_amd import ops
    rec = {}
    sym, dirf = ops._sym_fwd, ops.score_dir_fwd

    def sym_(*a, **k):
        o = sym(*a, **k)
        assert "diag" not in rec
        rec["diag"] = o.diag
        return o

    def dir_(A, *a, **k):
        o = dirf(A, *a, **k)
        if A.data_ptr() == n.data_ptr():
            assert "diag" not in rec
            rec["diag"] = o[1]
        return o
    ops._sym_fwd, ops.score_dir_fwd = sym_, dir_
    try:
        yield rec
    finally:
        ops._sym_fwd, ops.score_dir_fwd = sym, dirf


def _run(kw, inv_t, dtype, want_col_rank=False, backward=True):
    """dict: loss, out8, rank, rowsum, colsum, diag[, dN, dC, dX]"""
    from jodalrob_twotower_amd.two_tower_train_task import _ScoreCEFn
    n, c = kw["n"].clone().requires_grad_(True), kw["c"].clone().requires_grad_(True)
    x = None if kw["x"] is None else kw["x"].clone().requires_grad_(True)
    B = n.shape[0]
    with _recorded(n) as rec:
        loss, out8, rank = _ScoreCEFn.apply(n, c, inv_t, dtype, want_col_rank, False, None, None, None, kw["lq_n"], kw["lq_c"], kw["ent_n"],
                                            kw["ent_c"], kw["pair_w"], x, kw["lq_x"], kw["ent_x"], kw["cells"])
    # forward saves (n, c, rowsum, colsum[, x]) in this order: the first two are checked to BE n and c, the sums by their shape
    saved = loss.grad_fn.saved_tensors
    assert saved[0].data_ptr() == n.data_ptr() and saved[1].data_ptr() == c.data_ptr() and len(saved) == (4 if x is None else 5)
    assert saved[2].shape == saved[3].shape == (B,) and saved[2].data_ptr() != saved[3].data_ptr()
    plain_first = want_col_rank and dtype in ("bf16", "bf16x3") and not any(v is not None for k, v in kw.items() if k not in ("n", "c"))
    assert ("diag" in rec) != plain_first                   # (the plain bf16 / bf16x3 first call takes the two-direction kernel)
    r = dict(loss=loss.detach().clone(), out8=out8.detach().clone(), rank=rank.clone(), rowsum=saved[2].clone(), colsum=saved[3].clone(),
             diag=rec["diag"].clone() if "diag" in rec else None)
    assert r["diag"] is None or r["diag"].shape == (B,)
    if backward:
        loss.backward()
        r.update(dN=n.grad.clone(), dC=c.grad.clone(), dX=None if x is None else x.grad.clone())
    torch.cuda.synchronize()
    return r


@functools.lru_cache(maxsize=None)
def _forward_of(dtype, terms, shape, drop=None):
    """the forward of a combination, run once and shared (never written to): the plain call, or -- drop="extras" -- the same inputs
    without the extras (the same cell list: its cells on the extras are then out of range, which the plan ignores)"""
    B, M, D, T = shape
    kw = _inputs(terms, B, M, D)
    return _run(dict(kw, **dict.fromkeys(DROPS[drop])) if drop else kw, 1.0 / T, dtype, backward=False)


def _launches():
    from jodalrob_twotower_amd import _lib
    return int(_lib.load().tt_launch_count())


def _fp8_reference(kw, T):
    """(loss, dN, dC, accuracy) of the f64 oracle on the e4m3-rounded operands, the gradient products as the fp8 kernels form them"""
    n, c = kw["n"].cpu().numpy().astype(np.float64), kw["c"].cpu().numpy().astype(np.float64)
    n8, c8 = O.score_operands_fp8(n, c, T)
    ref_loss, met, S, lse = O.score_ce_fwd(n8, c8, T)
    rN, rC = O.score_ce_bwd(n8, c8, S, lse, T, q=O.q_bf16, prod_operands=O.score_operands_bf16(n, c, T), block_fp8=True)
    return float(ref_loss), rN, rC, float(met["accuracy"])


def _check_against_reference(dtype, terms, shape):
    B, M, D, T = shape
    inv_t = 1.0 / T
    kw = _inputs(terms, B, M, D)
    t0 = time.perf_counter()
    got = _run(kw, inv_t, dtype)
    t_node = time.perf_counter() - t0
    fl = inv_t / (2.0 * B)
    figs = {}
    if dtype == "fp8":
        ref_loss, rN, rC, ref_acc = _fp8_reference(kw, T)
        gb = FP8_BOUNDS[1]
        figs.update(dN=_rel(got["dN"].cpu().numpy(), rN), dC=_rel(got["dC"].cpu().numpy(), rC))
    else:
        ref_loss, rN, rC, rX, ref_rs, ref_cs = NR.reference(kw["n"], kw["c"], inv_t, dtype, **_ref_kw(kw))
        ref_acc = NR.accuracy(kw["n"], kw["c"], inv_t, dtype, kw["x"])
        gb = BOUNDS[dtype][1]
        figs.update(dN=_nrel(got["dN"], rN, fl), dC=_nrel(got["dC"], rC, fl))
        if kw["x"] is not None:
            figs["dX"] = _nrel(got["dX"], rX, fl)
        figs["rowsum"] = float(((got["rowsum"].double() - ref_rs).abs() / ref_rs).max())
        figs["colsum"] = float(((got["colsum"].double() - ref_cs).abs() / ref_cs).max())
    figs["loss"] = abs(got["loss"].item() - ref_loss)
    figs["accuracy"] = abs(got["out8"][1].item() - ref_acc)
    print(f"{dtype} {shape} {_name(terms)}: loss {got['loss'].item():.9g} ref {ref_loss:.9g} (bound {loss_bound(dtype, ref_loss):.3g}) "
          + " ".join(f"{k} {v:.3g}" for k, v in figs.items()) + f" (gradient bound {gb:g}) node {1e3 * t_node:.1f} ms")
    assert np.isfinite(got["loss"].item())
    assert figs["loss"] <= loss_bound(dtype, ref_loss), (got["loss"].item(), ref_loss)
    assert all(figs[k] <= gb for k in ("dN", "dC", "dX") if k in figs), figs
    if dtype != "fp8":
        assert figs["rowsum"] <= _sum_rtol(dtype, inv_t) and figs["colsum"] <= _sum_rtol(dtype, inv_t), figs
    assert figs["accuracy"] <= 2.0 / B, figs
    # what a term does not enter is bit for bit the plain call's of the same dtype on the same n, c
    plain = _forward_of(dtype, frozenset(), shape)
    assert torch.equal(got["diag"], plain["diag"])
    for k in (2, 3, 4, 6):
        assert got["out8"][k].item() == plain["out8"][k].item(), (k, got["out8"], plain["out8"])
    if "extras" in terms:                                    # the extras stand in no column sum
        assert torch.equal(got["colsum"], _forward_of(dtype, terms, shape, "extras")["colsum"])
    return got


# ---- 1. accepted combinations ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype,terms", ACCEPTED, ids=lambda v: v if isinstance(v, str) else _name(v))
def test_accepted_combination_vs_f64(tt, dtype, terms, shape):
    _check_against_reference(dtype, terms, shape)


def _widest(dtype):
    return max((t for d, t in ACCEPTED if d == dtype), key=lambda t: (len(t), sorted(t)))


def test_the_matrix_is_the_tables(tt):
    assert len(ACCEPTED) == 42 and len(ACCEPTED) + len(REFUSED) == 320
    assert all(t <= set(TERMS) | set(RIDERS) and set(DROPS) >= (t - {"ent"}) for d, t in ACCEPTED)
    assert {d for d, t in ACCEPTED if t} == {"fp32", "bf16", "bf16x3"} and ("fp8", frozenset()) in ACCEPTED
    assert _widest("bf16") == _widest("fp32") == frozenset({"lq", "ent", "extras", "ent_x", "lq_x"}) and _widest("bf16x3") == {"lq"}


# ---- 2. refused combinations -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_refused_combinations_launch_nothing(tt, dtype):
    B, M, D, T = SHAPES[0]
    seen = 0
    for d, terms in REFUSED:
        if d != dtype:
            continue
        kw = _inputs(terms, B, M, D)
        torch.cuda.synchronize()
        before = _launches()
        with pytest.raises(ValueError) as e:
            _run(kw, 1.0 / T, dtype)
        assert str(e.value) == _expected(dtype, terms), (dtype, sorted(terms))
        assert _launches() == before, (dtype, sorted(terms))
        seen += 1
    assert seen == {"fp32": 80 - 17, "bf16": 80 - 22, "bf16x3": 80 - 2, "fp8": 80 - 1}[dtype]


@pytest.mark.parametrize("dtype", DTYPES)
def test_unequal_row_counts_launch_nothing(tt, dtype):
    from jodalrob_twotower_amd.two_tower_train_task import _ScoreCEFn
    n, c = GL._unit_rows(4, 8, 1), GL._unit_rows(3, 8, 2)
    torch.cuda.synchronize()
    before = _launches()
    for a, b in ((n, c), (c, n)):
        with pytest.raises(ValueError, match="4.*3|3.*4"):
            _ScoreCEFn.apply(a, b, 1.0, dtype)
    assert _launches() == before


# ---- 3. the first call -------------------------------------------------------------------------------------------------------------------
FIRST_CALLS = [(d, _widest(d)) for d in ("fp32", "bf16", "bf16x3")] + [("bf16", frozenset({"cells", "extras", "lq", "lq_x"}))] \
    + [(d, frozenset()) for d in DTYPES]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype,terms", FIRST_CALLS, ids=lambda v: v if isinstance(v, str) else _name(v))
def test_first_call_diagnostic(tt, dtype, terms, shape):
    """want_col_rank=True: everything but the column top-1 rate is the steady-state call's, bit for bit; out8[5] is the column top-1 rate
    of the plain two-direction kernel on the same packed operands (fp32: of the plain column-direction sweep; fp8: the node has the
    symmetric forward only, which writes no rate -- out8[5] is then only held equal to the steady-state call's).

    The plain call of bf16 and bf16x3 is the one first call that is NOT the steady-state forward plus a second launch: with no term to
    correct, the node takes sums, means and reciprocals from the two-direction launch that ranks the columns (tt_score_fwd_bf16, then
    tt_score_loss_finish).  That launch adds the row sums and the diagonal in another order than the symmetric sweep, and it forms the
    sum of all scores by adding them, where the sweep forms (sum_a n_a) . (sum_b c_b): out8[3:5] and, through the reciprocals, the
    bf16x3 gradients cannot share their bits (measured: the negative mean apart by 1.2e-10 / 8.1e-10, bf16x3 gradients by 5.8e-8).
    Held there, so that nothing goes without an assertion:
      1. bit for bit against the steady-state call, as everywhere else: loss, row ranks, out8[:3] (loss, accuracy, the positive mean),
         and in bf16 the gradients -- only the negative mean, the gap formed from it and the bf16x3 gradients are left to 3 and 4;
      2. bit for bit against the entries called directly (score_fwd_bf16 -> score_loss_finish -> the backward on those sums): loss, ranks,
         all of out8[:6] and both gradients -- what the node hands on is what those launches computed;
      3. against f64 on the kernels' operands: loss and gradients under the mode's bounds, the positive and negative means of BOTH calls
         under the bounds tests/test_gpu_parity.py::test_score_fp8_vs_rounded_oracle holds these two metrics to;
      4. the two calls against each other, by the triangle inequality on 3 (as tests/test_gpu_known_mask.py argues for its transposing
         backward): the means within twice their bound, the bf16x3 gradients within twice the mode's."""
    from jodalrob_twotower_amd import ops
    B, M, D, T = shape
    inv_t = 1.0 / T
    kw = _inputs(terms, B, M, D)
    # the companies lean on their notices, so that the rates are neither 0 nor 1 (independent rows: 1 / B) and the column rate, over B
    # rows, is not the row rate, over B + M columns: 2.8 / sqrt(D) puts the positive near the largest of B scores of spread 1 / sqrt(D)
    c = kw["c"] + (2.8 / D ** 0.5) * kw["n"]
    kw["c"] = c / c.norm(dim=1, keepdim=True)
    n, c = kw["n"], kw["c"]
    first, later = _run(kw, inv_t, dtype, want_col_rank=True), _run(kw, inv_t, dtype)
    fp8, x3 = dtype == "fp8", dtype == "bf16x3"
    two_direction = not terms and dtype in ("bf16", "bf16x3")
    if dtype != "fp32":
        sn = 1.0 if x3 else ops.score_unit_scale(inv_t)
        Np, Cp = (ops.score_pack2_fp8 if fp8 else ops.score_pack2_bf16x3 if x3 else ops.score_pack2_bf16)(n, c, sn, 1.0)
    if not two_direction:
        for k in ("loss", "rank", "dN", "dC", "dX"):
            assert (first[k] is None and later[k] is None) or torch.equal(first[k], later[k]), k
        assert torch.equal(first["out8"][:5], later["out8"][:5]), (first["out8"], later["out8"])
        if fp8:
            assert first["out8"][5].item() == later["out8"][5].item()
            return
        col_rank = ops.score_dir_fwd(c, n, inv_t, abs(inv_t), 0, False)[2] if dtype == "fp32" else \
            ops.score_fwd_bf16(Np, Cp, B, D, inv_t, abs(inv_t), True, False, sn, x3=x3)[4]
    else:
        # 1.
        assert torch.equal(first["loss"], later["loss"]) and torch.equal(first["rank"], later["rank"])
        assert torch.equal(first["out8"][:3], later["out8"][:3]), (first["out8"], later["out8"])
        if dtype == "bf16":
            assert torch.equal(first["dN"], later["dN"]) and torch.equal(first["dC"], later["dC"])
        # 2.
        rs, cs, dg, rr, col_rank, ss, inv = ops.score_fwd_bf16(Np, Cp, B, D, inv_t, abs(inv_t), True, False, sn, with_inv=True, x3=x3)
        out8_d, loss_d = ops.score_loss_finish(B, abs(inv_t), rs, cs, dg, rr, col_rank, ss)
        dN_d, dC_d, _ = ops._bwd_sym(Np, Cp, B, D, inv_t, abs(inv_t), rs, cs, torch.ones((), device=n.device), inv_t / (2.0 * B), sn, inv, dtype,
                                     None, ops.ScoreTerms())
        assert torch.equal(first["loss"], loss_d) and torch.equal(first["rank"], rr) and torch.equal(first["out8"][:6], out8_d[:6])
        assert torch.equal(first["dN"], dN_d) and torch.equal(first["dC"], dC_d)
        # 3.
        ref_loss, rN, rC = NR.reference(n, c, inv_t, dtype)[:3]
        A, Bm, _, k = NR.node_operands(n, c, None, inv_t, dtype)
        S = (A @ Bm.T) * k
        pos = float(S.diagonal().mean())
        neg = float((S.sum() - S.diagonal().sum()) / (B * B - B))
        b_pos, b_neg = 1e-4 * abs(pos) + 1e-6, 2e-3 * abs(neg) + 2e-6
        fl, (lb, gb) = inv_t / (2.0 * B), BOUNDS[dtype]
        figs = dict(loss=abs(first["loss"].item() - ref_loss), dN=_nrel(first["dN"], rN, fl), dC=_nrel(first["dC"], rC, fl),
                    pos_first=abs(first["out8"][2].item() - pos), pos_later=abs(later["out8"][2].item() - pos),
                    neg_first=abs(first["out8"][3].item() - neg), neg_later=abs(later["out8"][3].item() - neg),
                    first_vs_later_dN=_nrel(first["dN"], later["dN"].double(), fl), first_vs_later_dC=_nrel(first["dC"], later["dC"].double(), fl),
                    first_vs_later_means=[abs(first["out8"][j].item() - later["out8"][j].item()) for j in (2, 3, 4)])
        print(dtype, shape, "plain first call (the two-direction kernel)", figs, "bounds: means", b_pos, b_neg, "gradients", gb)
        assert figs["loss"] <= lb * abs(ref_loss) + LOSS_ATOL and figs["dN"] <= gb and figs["dC"] <= gb, figs
        assert figs["pos_first"] <= b_pos and figs["pos_later"] <= b_pos and figs["neg_first"] <= b_neg and figs["neg_later"] <= b_neg, figs
        for call in (first, later):                          # (the gap is formed from the two means, exactly)
            assert call["out8"][4].item() == (call["out8"][2] - call["out8"][3]).item()
        # 4.
        dm = figs["first_vs_later_means"]
        assert dm[0] <= 2 * b_pos and dm[1] <= 2 * b_neg and dm[2] <= 2 * (b_pos + b_neg), figs
        assert figs["first_vs_later_dN"] <= 2 * gb and figs["first_vs_later_dC"] <= 2 * gb, figs
    # out8[5]: hits / B as an f32 quotient.  With a term on packed operands the node forms it as torch's mean over the second launch's
    # ranks: the same expression here, exactly.  On a plain first call and on the f32 path the finish kernel divides, and may round the other way (126 / 300: 0.42 - 1.3e-8
    # against torch's 0.42 + 1.7e-8): there the hit count read back from the rate is the kernel's, exactly, and the rate is within one
    # f32 ulp of hits / B (bf16 / bf16x3: item 2 above holds it to the finish kernel's own bits besides)
    hits = int((col_rank == 0).sum())
    got5 = first["out8"][5].item()
    ref = NR.accuracy(n, c, inv_t, dtype, columns=True)
    print(dtype, shape, _name(terms), "column top-1 rate", got5, "kernel hits", hits, "of", B, "f64", ref)
    if terms and dtype != "fp32":                            # (the f32 path has no second launch: its finish kernel divides there too)
        assert got5 == (col_rank == 0).float().mean().item()
    else:
        assert round(got5 * B) == hits and abs(got5 - hits / B) <= 2.0 ** -23 * hits / B
    assert abs(hits / B - ref) <= 2.0 / B and 0.1 <= ref <= 0.9
    if kw["x"] is not None:
        assert got5 != first["out8"][1].item()


# ---- 4. one-sided ids --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("terms", ONE_SIDED, ids=_name)
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_one_sided_ids_vs_f64(tt, dtype, terms, shape):
    """ids on one side only: the other side is all-distinct (the reference's mask_matrix with None)"""
    B, M, D, T = shape
    kw = _inputs(terms, B, M, D)
    assert (kw["ent_n"] is None) != (kw["ent_c"] is None)
    _check_against_reference(dtype, terms, shape)


# ---- the inputs above, on the device's own rows ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_inputs_have_teeth_on_the_device(tt, shape):
    """tests/test_score_node_reference_host.py's condition, on the rows the device's generator draws"""
    for dtype, terms in ACCEPTED + [(d, t) for d in ("fp32", "bf16") for t in ONE_SIDED]:
        if dtype == "fp8":
            continue                                         # (the plain call only: nothing to take away)
        for term, ratio in teeth(dtype, terms, *shape).items():
            assert ratio >= 100.0, (dtype, sorted(terms), term, ratio)
