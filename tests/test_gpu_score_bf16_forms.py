"""score_dtype = "bf16": every form of tt_score_fwd_bf16 / tt_score_bwd_bf16 against f64 at the smallest shapes at which it can go
wrong (shapes, operands, dispatch mirror and bars: tests/_score_forms.py; the bars on the CPU: tests/test_score_bf16_forms_host.py).

A. Backward: the seven kernels of bwd_bf16() x {unit, non-unit} x {reciprocals from the forward, NULL}, square and rectangular
   (Ra != Rb, diag_offset no multiple of 32, positives ending in the ragged last tile, fewer b tiles than waves), one or two
   directions, two directions with different Ra.  TT_OPT_SCORE_BWD_ROWS_MIN forces the rows form or keeps it away; every call is
   exactly one launch.  Bar, per element, derived (nothing measured): with e_ab = exp(s_ab - shift),
   w_ab = e_ab (1 / sum_a + 1 / sum_b) - 2 [b is a's positive], k = scale, Dp = padded D,

       |dA - k (W B)_f64|[a, d] <= rho k sum_b (|e_ab (1 / sum_a + 1 / sum_b)| + 2 [b is a's positive]) |B_bd|
       rho = 2^-8 + 2 Dp 2^-24 / T + (Rb + 16) 2^-24

   2^-8: the round-to-nearest bf16 rounding of the weight (the gradient MFMA's operand; the reference's W is not rounded).  bf16
   keeps 8 significant bits: neighbours in [1, 2) are 2^-7 apart, so a value just above 1 moves by up to 2^-8 of itself.  (The
   plan for this suite said 2^-9, which holds only at the top of a binade.  The f32 + bf16 emulation of the host test leaves a
   2^-9 bar by 6 % at B = 33, D = 33, T = 0.07: a row whose positive has one exact copy has ONE weight that matters, 1.089, and
   bf16(1.089) = 1.0859 is 3.6e-3 of it away.)
   2 Dp 2^-24 / T: the f32 accumulation of the exponent's argument, once in the recompute and once in the forward's sums
   (|n . c| <= 1 for unit rows).   (Rb + 16) 2^-24: the f32 accumulation over b, plus exp2, rcp, add and multiply.
   The positive's 2 is counted by magnitude: at B = 1 the weight cancels (1 + 1 - 2) and the bar must not.
   The reference is O.score_dir_terms on the kernels' operands (O.score_operands_bf16 for the unit form, q_bf16 of both sides
   for scale 1) and the kernels' own forward sums, which section B checks.
   Between forms on the same operands and sums: the rows form against its b-split / transposing counterpart differs in the
   order of the sum over b only: per element <= 2 (Rb + 16) 2^-24 (the same magnitude sum).  Reciprocals given against taken in
   the kernel: the f32 weights differ in their last bits (4 2^-24), and a weight that sits on a bf16 rounding boundary may flip
   to the neighbour, 2^-7 of itself away: counted for the weights whose f64 value lies within the f32 error of the weight
   (2 Dp 2^-24 / T + 16 2^-24 of its magnitude) of a boundary.  A second identical call gives the same bits.
B. Forward, tt_score_fwd_bf16: four tiles x {unit, non-unit} x rank mode {none, top-1, full}, with and without diag, sumscore and
   inv_sumexp, square and rectangular: sumexp relative Dp 2^-24 / T + (Rb + 8) 2^-24; diag absolute Dp 2^-24 / T; sumscore
   (Rb + Dp) 2^-24 sum_b |s_ab|; inv_sumexp * sumexp = the unit factor to 3 f32 spacings; full ranks inside the f64 bracket,
   planted ties exact; top-1 flag == (full rank != 0); unit and non-unit form (the same image times 2) agree on ranks and flags.
C. Padding contracts: the pack (and the towers' tail) writes every padding row and column of both images as +0 whatever the
   buffer held; the entries of sumexp_b / inv_b past Rb may hold any finite non-zero value.
D. Refusals launch nothing.

Every case prints its largest fraction of the bar (visible with -s); DESIGN.md section 4 quotes them.
"""
import functools
import json
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import oracle_np as O
import _score_forms as F
from conftest import GOLD
from params_init import init_state_numpy, synth_batch_numpy
from test_gpu_parity import DEV, ctx_option, tt, make_task, to_batch, load_state  # noqa: F401  (tt, ctx_option: fixtures)

from jodalrob_twotower_amd import _lib as L

pytestmark = pytest.mark.gpu

FLT_MAX = float(np.finfo(np.float32).max)


def _dev():
    return torch.device(DEV)


def _pad(n, m=64):
    return (n + m - 1) // m * m


def _f32(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(DEV)


def _np(t):
    return t.detach().cpu().numpy()


def _report(**kw):
    print(json.dumps(kw))


# ---- the two entries through ctypes: any number of directions, any shapes -----------------------------------------------------
def _fwd(dirs, D, inv_t, expect_rc_ok=True):
    """tt_score_fwd_bf16 over dirs = [dict(A, B, Ra, Rb, off, ab, mode, diag, ss, inv)] (mode: None, 1 = top-1 flag, 2 = full rank;
    diag / ss / inv: whether to ask for that output).  Exactly one launch.  Per direction a namespace of the outputs; the
    per-row arrays are padded to 64 rows with ones (tt_score_bwd_dir reads whole tiles)."""
    arr = (L.ScoreFwdDir * 2)()
    outs = []
    for i, d in enumerate(dirs):
        Ra = d["Ra"]
        o = SimpleNamespace(
            sumexp=torch.ones(_pad(Ra), dtype=torch.float32, device=DEV),
            diag=torch.full((Ra,), float("nan"), dtype=torch.float32, device=DEV) if d.get("diag") else None,
            rank=torch.full((Ra,), -7, dtype=torch.int32, device=DEV) if d.get("mode") else None,
            ss=torch.full((Ra,), float("nan"), dtype=torch.float32, device=DEV) if d.get("ss") else None,
            inv=torch.ones(_pad(Ra), dtype=torch.float32, device=DEV) if d.get("inv") else None)
        arr[i] = L.ScoreFwdDir(L.ptr(d["A"]), L.ptr(d["B"]), Ra, d["Rb"], d["off"], L.ptr(o.sumexp), L.ptr(o.diag), L.ptr(o.rank),
                               L.ptr(o.ss), d.get("mode") or 0, d["ab"], L.ptr(o.inv))
        outs.append(o)
    lib = L.load()
    n0 = lib.tt_launch_count()
    L.check(lib.tt_score_fwd_bf16(L.ctx(_dev()), arr, len(dirs), D, inv_t, abs(inv_t), L.stream(_dev())), "tt_score_fwd_bf16")
    assert lib.tt_launch_count() == n0 + 1
    return outs


def _bwd_raw(dirs, n_dirs, D, inv_t, scale, d_loss):
    """tt_score_bwd_bf16's status, no check: dirs = [dict(A, B, Ra, Rb, off, sa, sb, ab, bs, ia, ib, dA)]"""
    arr = (L.ScoreBwdDir * 2)()
    for i, d in enumerate(dirs):
        arr[i] = L.ScoreBwdDir(L.ptr(d["A"]), L.ptr(d["B"]), d["Ra"], d["Rb"], d["off"], L.ptr(d["sa"]), L.ptr(d["sb"]), L.ptr(d["dA"]),
                               d["ab"], d["bs"], L.ptr(d.get("ia")), L.ptr(d.get("ib")))
    return L.load().tt_score_bwd_bf16(L.ctx(_dev()), arr, n_dirs, D, inv_t, abs(inv_t), L.ptr(d_loss), scale, L.stream(_dev()))


def _bwd(dirs, D, inv_t, scale):
    """tt_score_bwd_bf16 over the directions: exactly one launch; returns [dA] (NaN where the kernel wrote nothing)"""
    one = torch.ones(1, dtype=torch.float32, device=DEV)
    for d in dirs:
        d["dA"] = torch.full((d["Ra"], D), float("nan"), dtype=torch.float32, device=DEV)
    lib = L.load()
    n0 = lib.tt_launch_count()
    L.check(_bwd_raw(dirs, len(dirs), D, inv_t, scale, one), "tt_score_bwd_bf16")
    assert lib.tt_launch_count() == n0 + 1, "tt_score_bwd_bf16 must be one launch"
    return [d["dA"] for d in dirs]


# ---- one group's operands, forward results and references, computed once ------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _state(g):
    from jodalrob_twotower_amd import ops
    p = F.make_problem(g)
    st = SimpleNamespace(g=g, p=p, inv_t=1.0 / g.T)
    st.sn = F.unit_scale(g.T) if g.unit else 1.0
    if g.unit:
        assert st.sn == ops.score_unit_scale(st.inv_t)                 # exactly: or the kernels would take their non-unit form
    st.k = float(np.float32(st.inv_t / (2.0 * g.Rb)))                   # scale, as the entry receives it
    s = slice(g.off, g.off + g.Ra)
    tn, tc = _f32(p.n), _f32(p.c)
    st.tn, st.tc = tn, tc
    st.Np, st.Cp = ops.score_pack2_bf16(tn, tc, st.sn, 1.0)
    square = g.Ra == g.Rb and g.off == 0
    st.Npl, st.Cpl = (st.Np, st.Cp) if square else ops.score_pack2_bf16(tn[s].contiguous(), tc[s].contiguous(), st.sn, 1.0)
    full = dict(ab=st.sn, mode=2, diag=True, ss=True, inv=True)
    st.fwd_all = [dict(A=st.Np, B=st.Cp, Ra=g.Rb, Rb=g.Rb, off=0, **full), dict(A=st.Cp, B=st.Np, Ra=g.Rb, Rb=g.Rb, off=0, **full)]
    st.fwd_own = [dict(A=st.Npl, B=st.Cp, Ra=g.Ra, Rb=g.Rb, off=g.off, **full), dict(A=st.Cpl, B=st.Np, Ra=g.Ra, Rb=g.Rb, off=g.off, **full)]
    st.all = _fwd(st.fwd_all, g.D, st.inv_t)                            # everybody's rows: the sums of the b rows
    st.own = st.all if square else _fwd(st.fwd_own, g.D, st.inv_t)
    nb, cb = F.operands(p)
    st.ops64 = F.directions(p, nb, cb)
    st.ref = []
    for d, (A, Bm) in enumerate(st.ops64):
        sa, sb = _np(st.own[d].sumexp)[:g.Ra], _np(st.all[1 - d].sumexp)[:g.Rb]
        st.ref.append(F.grad_reference(g, A, Bm, sa, sb, st.k) + (sa, sb))
    torch.cuda.synchronize()
    return st


def _bwd_dirs(st, inv, pad_value=None):
    """the two directions of the group's backward; inv: with the forward's reciprocals; pad_value: what the entries of the b rows'
    arrays past Rb hold (default: what the forward call left there, ones)"""
    g = st.g
    out = []
    for d in (0, 1):
        own, oth = st.own[d], st.all[1 - d]
        sb, ib = oth.sumexp, oth.inv
        if pad_value is not None:
            sb, ib = sb.clone(), ib.clone()
            sb[g.Rb:] = pad_value
            ib[g.Rb:] = pad_value
        out.append(dict(A=st.Npl if d == 0 else st.Cpl, B=st.Cp if d == 0 else st.Np, Ra=g.Ra, Rb=g.Rb, off=g.off, sa=own.sumexp, sb=sb,
                        ab=st.sn, bs=1.0 if d == 0 else st.sn, ia=own.inv if inv else None, ib=ib if inv else None))
    return out


def _flip_allowance(g, A, Bm, sa, sb, k):
    """k sum_b [w_ab within its f32 error of a bf16 rounding boundary] 2^-7 mag_ab |B_bd|: what the weights that may round to the
    other neighbour when their last f32 bits change can move an element by (module docstring, A)"""
    W, mag = O.score_dir_terms(A, Bm, g.T, g.off, sa.astype(np.float64), sb.astype(np.float64))
    w = np.abs(W)
    _, e = np.frexp(np.where(w > 0, w, 1.0))
    ulp = np.ldexp(1.0, e - 8)                                        # bf16 spacing at w
    x = w / ulp
    dist = np.abs(x - np.floor(x) - 0.5) * ulp                        # to the nearest midpoint between two bf16 values
    eps = (2 * F.padded_d(g.D) * F.U24 / g.T + 16 * F.U24) * mag
    return k * ((np.where(dist <= eps, 2.0 ** -7, 0.0) * mag) @ np.abs(Bm))


# ---- A. backward ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", F.GROUPS, ids=F.group_id)
def test_backward_forms_vs_f64(tt, ctx_option, g):
    st = _state(g)
    ctx_option(L.TT_OPT_FUSE_SCORE_TAIL, 0, 0)
    got, fractions = {}, {}
    for rows_min, inv in F.bwd_variants(g):
        ctx_option(L.TT_OPT_SCORE_BWD_ROWS_MIN, rows_min, F.ROWS_MIN_DEFAULT)
        kernel = F.bwd_kernel(g.D, g.Ra, rows_min, g.unit)
        assert (kernel[0] in F.BWD_ROWS.values()) == (rows_min == F.ROWS_ALWAYS)
        dA = _bwd(_bwd_dirs(st, inv), g.D, st.inv_t, st.k)
        again = _bwd(_bwd_dirs(st, inv), g.D, st.inv_t, st.k)
        got[(rows_min, inv)] = [_np(x).astype(np.float64) for x in dA]
        for d in (0, 1):
            assert torch.equal(dA[d], again[d]), (kernel, inv, d)                         # (NaN anywhere fails this too)
            ref, magsum = st.ref[d][:2]
            fractions[f"{kernel[0]} {'unit' if g.unit else 'nonunit'} {'inv' if inv else 'rcp'} dir{d}"] = \
                F.bound_fraction(got[(rows_min, inv)][d], ref, magsum, F.rho(g))
    _report(group=F.group_id(g), rho=F.rho(g), fraction_of_bar=fractions)
    assert all(f <= 1.0 for f in fractions.values()), fractions
    # between forms, on identical operands and sums
    order = 2 * (g.Rb + 16) * F.U24
    cross = {}
    for d, (A, Bm) in enumerate(st.ops64):
        ref, magsum, sa, sb = st.ref[d]
        if F.padded_d(g.D) >= 64:
            for inv in (True, False):
                cross[f"rows_vs_small inv={inv} dir{d}"] = F.bound_fraction(got[(F.ROWS_ALWAYS, inv)][d], got[(F.ROWS_NEVER, inv)][d], magsum, order)
        flips = _flip_allowance(g, A, Bm, sa, sb, st.k)
        for rows_min in {rm for rm, _ in got}:
            err = np.abs(got[(rows_min, True)][d] - got[(rows_min, False)][d])
            lim = (order + 4 * F.U24) * magsum + flips
            cross[f"inv_vs_rcp rows_min={rows_min} dir{d}"] = float((err / np.where(lim > 0, lim, 1.0)).max()) if (lim > 0).all() else float(err.max() > 0)
    _report(group=F.group_id(g), between_forms=cross)
    assert all(f <= 1.0 for f in cross.values()), cross


@pytest.mark.parametrize("D,rows_min", [(8, F.ROWS_NEVER), (64, F.ROWS_NEVER), (64, F.ROWS_ALWAYS), (128, F.ROWS_NEVER), (129, F.ROWS_ALWAYS),
                                        (200, F.ROWS_NEVER), (65, F.ROWS_ALWAYS)])
def test_backward_one_direction_and_two_row_counts(tt, ctx_option, D, rows_min):
    """n_dirs = 1, and two directions with Ra = 70 and Ra = 33 (two problems in one call: the grid is sized by the larger, the
    workgroups past the smaller Ra return per direction): each direction inside the bar, and the same bits whether a direction is
    launched alone or beside the other."""
    ctx_option(L.TT_OPT_FUSE_SCORE_TAIL, 0, 0)
    ctx_option(L.TT_OPT_SCORE_BWD_ROWS_MIN, rows_min, F.ROWS_MIN_DEFAULT)
    g70, g33 = F.Group(70, 70, 0, D, 0.5, True), F.Group(33, 33, 0, D, 0.5, True)
    s70, s33 = _state(g70), _state(g33)
    d70, d33 = _bwd_dirs(s70, True)[0], _bwd_dirs(s33, True)[1]          # dN of the 70-row problem, dC of the 33-row problem
    both = _bwd([d70, d33], D, s70.inv_t, s70.k)
    alone70 = _bwd([dict(d70)], D, s70.inv_t, s70.k)[0]
    alone33 = _bwd([dict(d33)], D, s70.inv_t, s70.k)[0]
    assert torch.equal(both[0], alone70) and torch.equal(both[1], alone33)
    swapped = _bwd([dict(d33), dict(d70)], D, s70.inv_t, s70.k)          # the larger Ra second
    assert torch.equal(swapped[0], alone33) and torch.equal(swapped[1], alone70)
    fr = {}
    for name, st, d, x in (("Ra70", s70, 0, alone70), ("Ra33", s33, 1, alone33)):
        A, Bm = st.ops64[d]
        ref, magsum = F.grad_reference(st.g, A, Bm, st.ref[d][2], st.ref[d][3], s70.k)      # (the call's scale: the 70-row problem's)
        fr[name] = F.bound_fraction(_np(x), ref, magsum, F.rho(st.g))
    _report(D=D, rows_min=rows_min, fraction_of_bar=fr)
    assert all(f <= 1.0 for f in fr.values()), fr


# ---- B. forward -----------------------------------------------------------------------------------------------------------------
def _fwd_checks(g, o, A, Bm, M_cols, tie, tag):
    """one direction's outputs (full rank, diag, sumscore, inv_sumexp) against f64 on the same operands"""
    Ra, Rb, off = g.Ra, g.Rb, g.off
    S = (A @ Bm.T) / g.T
    E = np.exp(S - 1.0 / g.T)
    rows, pos = np.arange(Ra), np.arange(Ra) + off
    sumexp, diag, ss, inv, rank = (_np(o.sumexp)[:Ra].astype(np.float64), _np(o.diag).astype(np.float64), _np(o.ss).astype(np.float64),
                                   _np(o.inv)[:Ra].astype(np.float64), _np(o.rank))
    fr = {"sumexp": float((np.abs(sumexp - E.sum(1)) / E.sum(1)).max() / F.sumexp_rtol(g)),
          "diag": float(np.abs(diag - S[rows, pos]).max() / F.diag_atol(g)),
          "sumscore": float((np.abs(ss - S.sum(1)) / (F.sumscore_factor(g) * np.abs(S).sum(1))).max())}
    c2 = np.float32(-np.float32(1.0 / g.T)) * np.float32(O.LOG2E)                     # the library's exponent offset, in f32
    kexp = float(np.exp2(np.float64(c2))) if g.unit else 1.0
    fr["inv_x_sumexp_spacings"] = float((np.abs(inv * sumexp - kexp) / np.spacing(np.float32(kexp))).max()) / 3.0
    lo, hi = F.rank_bracket(S, M_cols, np.full(Ra, F.diag_atol(g)), off)
    outside = int(((rank < lo) | (rank > hi - 1)).sum())                              # (hi counts the positive itself)
    _report(group=F.group_id(g), direction=tag, forward_fraction_of_bar=fr, rank_outside=outside, rank_undecided=int((hi - 1 > lo).sum()))
    assert all(v <= 1.0 for v in fr.values()), (tag, fr)
    assert outside == 0, (tag, rank, lo, hi)
    if tie is not None:
        a, p, copies = tie
        before = sum(j < p for j in copies)
        assert rank[a] >= before and rank[a] <= hi[a] - 1
        if g.D >= 8:                # the positive is the row's clear maximum: only its exact copies in front of it count
            assert lo[a] == hi[a] - 1 == before and rank[a] == before, (tag, a, p, copies, rank[a], lo[a], hi[a])
    return rank


@pytest.mark.parametrize("g", F.GROUPS, ids=F.group_id)
def test_forward_forms_vs_f64(tt, g):
    from jodalrob_twotower_amd import ops
    st = _state(g)
    kernel = F.fwd_kernel(g.D, g.unit)
    assert kernel[0] in F.FWD_KERNELS.values()
    M = (st.p.c, st.p.n)
    ranks = [_fwd_checks(g, st.own[d], *st.ops64[d], M[d], st.p.ties.get(d), f"dir{d}") for d in (0, 1)]
    # rank mode and optional outputs: the same sums bit for bit; the top-1 flag is (full rank != 0)
    top1 = _fwd([dict(d, mode=1, diag=False, ss=False, inv=False) for d in st.fwd_own], g.D, st.inv_t)
    none = _fwd([dict(d, mode=None, diag=(i == 0), ss=(i == 1), inv=(i == 1)) for i, d in enumerate(st.fwd_own)], g.D, st.inv_t)
    again = _fwd(st.fwd_own, g.D, st.inv_t)
    for d in (0, 1):
        full = st.own[d]
        assert torch.equal(top1[d].sumexp, full.sumexp) and torch.equal(none[d].sumexp, full.sumexp) and torch.equal(again[d].sumexp, full.sumexp)
        assert torch.equal(top1[d].rank, (full.rank != 0).to(torch.int32)), d
        assert torch.equal(again[d].rank, full.rank) and torch.equal(again[d].diag, full.diag) and torch.equal(again[d].ss, full.ss)
    assert torch.equal(none[0].diag, st.own[0].diag) and torch.equal(none[1].ss, st.own[1].ss) and torch.equal(none[1].inv, st.own[1].inv)
    # one direction alone: the same bits
    for d in (0, 1):
        alone = _fwd([st.fwd_own[d]], g.D, st.inv_t)[0]
        assert torch.equal(alone.sumexp, st.own[d].sumexp) and torch.equal(alone.rank, st.own[d].rank) and torch.equal(alone.diag, st.own[d].diag)
    if g.unit:
        # the non-unit form on the same image times 2 (exact in bf16: every product doubles, comparisons are unchanged)
        s = slice(g.off, g.off + g.Ra)
        Np2, _ = ops.score_pack2_bf16(st.tn, st.tc, 2.0 * st.sn, 1.0)
        Npl2, _ = ops.score_pack2_bf16(st.tn[s].contiguous(), st.tc[s].contiguous(), 2.0 * st.sn, 1.0)
        twin = [dict(st.fwd_own[0], A=Npl2, ab=2.0 * st.sn), dict(st.fwd_own[1], B=Np2, ab=2.0 * st.sn)]
        assert 2.0 * st.sn != ops.score_unit_scale(st.inv_t)
        t_full = _fwd(twin, g.D, st.inv_t)
        t_top1 = _fwd([dict(d, mode=1) for d in twin], g.D, st.inv_t)
        for d in (0, 1):
            assert torch.equal(t_full[d].rank, st.own[d].rank) and torch.equal(t_top1[d].rank, top1[d].rank), d
            np.testing.assert_allclose(_np(t_full[d].diag), _np(st.own[d].diag), rtol=2 ** -22, atol=0)
            np.testing.assert_allclose(_np(t_full[d].sumexp)[:g.Ra], _np(st.own[d].sumexp)[:g.Ra], rtol=2 * F.sumexp_rtol(g), atol=0)


# ---- C. padding contracts -------------------------------------------------------------------------------------------------------
def _unpack_images(buf, R, D):
    """(rows image, fragment image) of a tt_score_pack_bf16 buffer as int16 bit patterns [Rp, Dp]: rows image
    [tile][k-step][half][row in tile][8], fragment image [tile][s][h][d][8] with element j of a chunk = row
    32 t + 16 s + 8 (j >> 2) + 4 h + (j & 3), column d"""
    Rp, Dp = _pad(R), F.padded_d(D)
    raw = buf.view(torch.int16).cpu().numpy()
    assert raw.size == 2 * Rp * Dp
    rows = raw[:Rp * Dp].reshape(Rp // 32, Dp // 16, 2, 32, 8).transpose(0, 3, 1, 2, 4).reshape(Rp, Dp)
    frag = raw[Rp * Dp:].reshape(Rp // 32, 2, 2, Dp, 2, 4).transpose(0, 1, 4, 2, 5, 3).reshape(Rp, Dp)
    return rows, frag


def _assert_images(buf, x, scale, who):
    """both images hold bf16(scale x) where there is a row and a column, +0 everywhere else"""
    R, D = x.shape
    want = np.zeros((_pad(R), F.padded_d(D)), dtype=np.int16)
    want[:R, :D] = (x * torch.tensor(scale, dtype=torch.float32, device=x.device)).to(torch.bfloat16).view(torch.int16).cpu().numpy()
    rows, frag = _unpack_images(buf, R, D)
    assert np.array_equal(rows, want), who
    assert np.array_equal(frag, want), who


@pytest.mark.parametrize("R,D", [(1, 1), (31, 8), (65, 33), (300, 200), (129, 256), (64, 64)])
def test_pack_writes_its_padding(tt, R, D):
    """tt_score_pack2_bf16 into buffers full of 0xFF bytes (every bf16 a NaN): the same bytes as into zeroed buffers, every
    padding row and column +0 -- what lets the kernels multiply zero weights with the padding rows."""
    lib = L.load()
    rng = np.random.default_rng(R * 1000 + D)
    x0, x1 = _f32(rng.standard_normal((R, D))), _f32(rng.standard_normal((R, D)))
    sc = F.unit_scale(0.07)
    bufs = []
    for fill in (0xFF, 0x00):
        b0 = torch.full((lib.tt_score_pack_bytes(R, D),), fill, dtype=torch.uint8, device=DEV)
        b1 = torch.full((lib.tt_score_pack_bytes(R, D),), fill, dtype=torch.uint8, device=DEV)
        L.check(lib.tt_score_pack2_bf16(L.ctx(_dev()), L.ptr(x0), R, L.ptr(b0), L.ptr(x1), R, L.ptr(b1), D, sc, 1.0, L.stream(_dev())),
                "tt_score_pack2_bf16")
        bufs.append((b0, b1))
    assert torch.equal(bufs[0][0], bufs[1][0]) and torch.equal(bufs[0][1], bufs[1][1])
    _assert_images(bufs[0][0], x0, sc, "scaled operand")
    _assert_images(bufs[0][1], x1, 1.0, "unscaled operand")


@pytest.mark.parametrize("g", [g for g in F.GROUPS if g.Rb % 32], ids=F.group_id)
def test_poisoned_buffers_and_tile_padding_leave_the_bits(tt, ctx_option, g):
    """Forward and backward on operands packed into 0xFF-filled buffers, and the backward with the entries of sumexp_b / inv_b past
    Rb holding 1, FLT_MAX, 2^-126 and -3 (finite and non-zero, as include/twotower.h asks): bit-identical, in every backward form."""
    lib = L.load()
    st = _state(g)
    s = slice(g.off, g.off + g.Ra)
    packs = []
    for x0, x1 in ((st.tn, st.tc), (st.tn[s].contiguous(), st.tc[s].contiguous())):
        R = x0.shape[0]
        b0 = torch.full((lib.tt_score_pack_bytes(R, g.D),), 0xFF, dtype=torch.uint8, device=DEV)
        b1 = torch.full((lib.tt_score_pack_bytes(R, g.D),), 0xFF, dtype=torch.uint8, device=DEV)
        L.check(lib.tt_score_pack2_bf16(L.ctx(_dev()), L.ptr(x0), R, L.ptr(b0), L.ptr(x1), R, L.ptr(b1), g.D, st.sn, 1.0, L.stream(_dev())),
                "tt_score_pack2_bf16")
        packs.append((b0, b1))
    (Np, Cp), (Npl, Cpl) = packs
    assert torch.equal(Np, st.Np) and torch.equal(Cp, st.Cp) and torch.equal(Npl, st.Npl) and torch.equal(Cpl, st.Cpl)
    own = _fwd([dict(st.fwd_own[0], A=Npl, B=Cp), dict(st.fwd_own[1], A=Cpl, B=Np)], g.D, st.inv_t)
    for d in (0, 1):
        for name in ("sumexp", "diag", "rank", "ss", "inv"):
            assert torch.equal(getattr(own[d], name), getattr(st.own[d], name)), (d, name)
    ctx_option(L.TT_OPT_FUSE_SCORE_TAIL, 0, 0)
    for rows_min, inv in F.bwd_variants(g):
        ctx_option(L.TT_OPT_SCORE_BWD_ROWS_MIN, rows_min, F.ROWS_MIN_DEFAULT)
        base = _bwd(_bwd_dirs(st, inv), g.D, st.inv_t, st.k)
        poisoned = _bwd_dirs(st, inv)
        poisoned[0].update(A=Npl, B=Cp)
        poisoned[1].update(A=Cpl, B=Np)
        for x, y in zip(_bwd(poisoned, g.D, st.inv_t, st.k), base):
            assert torch.equal(x, y), (rows_min, inv)
        for pad_value in (1.0, FLT_MAX, 2.0 ** -126, -3.0):
            for x, y in zip(_bwd(_bwd_dirs(st, inv, pad_value), g.D, st.inv_t, st.k), base):
                assert torch.equal(x, y), (rows_min, inv, pad_value)


@pytest.mark.parametrize("B", [65, 300])
def test_tower_tail_writes_its_padding(tt, manifest, monkeypatch, B):
    """The images the towers' fused tail emits (tt_tower_acts.emb_packed) into a buffer full of 0xFF bytes: the images
    tt_score_pack2_bf16 makes of the emitted rows, padding rows and columns +0."""
    from jodalrob_twotower_amd import ops
    cfg = dict(manifest["cases"]["wide_b40"])
    z = np.load(GOLD / "case_wide_b40.npz")
    shapes = {k[6:]: z[k].shape for k in z.files if k.startswith("state.")}
    state = init_state_numpy(shapes, 151)
    b = synth_batch_numpy(B, cfg["vocab_n"], cfg["vocab_c"], cfg["din_n"], cfg["din_c"], 152, oob=False)
    task = make_task(tt, cfg, mlp_dtype="bf16", score_dtype="bf16")
    load_state(task, state)
    task.train()
    assert task.two_tower_model.notice_tower.pack_for_score
    real_empty = torch.empty

    def poisoned_empty(*args, **kw):
        t = real_empty(*args, **kw)
        return t.fill_(0xFF) if t.dtype == torch.uint8 else t
    tb = to_batch(tt, b, cfg["keys_n"], cfg["keys_c"])
    monkeypatch.setattr(torch, "empty", poisoned_empty)
    n, c = task.two_tower_model(tb["notice"], tb["company"])
    monkeypatch.setattr(torch, "empty", real_empty)
    (pn, sn), (pc, sc) = n._tt_packed, c._tt_packed
    D = n.shape[1]
    assert n.shape[0] == B and pn.numel() == L.load().tt_score_pack_bytes(B, D)
    _assert_images(pn, n.detach(), sn, "notice tower")
    _assert_images(pc, c.detach(), sc, "company tower")
    rn, rc = ops.score_pack2_bf16(n.detach().contiguous(), c.detach().contiguous(), sn, sc)
    assert torch.equal(pn, rn) and torch.equal(pc, rc)


# ---- D. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(tt, ctx_option):
    ctx_option(L.TT_OPT_FUSE_SCORE_TAIL, 0, 0)
    lib = L.load()
    st = _state(F.Group(33, 33, 0, 64, 1.0, True))
    one = torch.ones(1, dtype=torch.float32, device=DEV)

    def bwd(n_dirs=2, D=64, **change):
        dirs = _bwd_dirs(st, True)
        for d in dirs:
            d["dA"] = torch.zeros((33, 64), dtype=torch.float32, device=DEV)
            d.update(change)
        return _bwd_raw(dirs, n_dirs, D, st.inv_t, st.k, one)

    def fwd(n_dirs=2, D=64, **change):
        arr = (L.ScoreFwdDir * 2)()
        keep = []
        for i, d in enumerate(st.fwd_own):
            d = dict(d, **change)
            sums = torch.ones(64, dtype=torch.float32, device=DEV)
            keep.append(sums)
            arr[i] = L.ScoreFwdDir(L.ptr(d["A"]), L.ptr(d["B"]), d["Ra"], d["Rb"], d["off"], L.ptr(sums), None, None, None, 0, d["ab"], None)
        return lib.tt_score_fwd_bf16(L.ctx(_dev()), arr, n_dirs, D, st.inv_t, abs(st.inv_t), L.stream(_dev()))

    sb, ib = st.all[0].sumexp, st.all[0].inv
    torch.cuda.synchronize()
    n0 = lib.tt_launch_count()
    assert bwd(D=0) != 0 and bwd(D=257) != 0 and bwd(n_dirs=3) != 0 and bwd(n_dirs=0) != 0 and bwd(Ra=0) != 0 and bwd(Rb=0) != 0
    assert bwd(sb=sb[1:]) != 0 and bwd(ib=ib[1:]) != 0                   # 4 bytes off a 16-byte boundary
    assert fwd(D=0) != 0 and fwd(D=257) != 0 and fwd(n_dirs=3) != 0 and fwd(n_dirs=0) != 0 and fwd(Ra=0) != 0 and fwd(Rb=0) != 0
    assert lib.tt_launch_count() == n0, "a refused call launched something"
    assert bwd() == 0 and lib.tt_launch_count() == n0 + 1                # (the same arguments unchanged are taken)
