"""Shared by tests/test_gpu_score_bf16_forms.py (GPU) and tests/test_score_bf16_forms_host.py (CPU): the shapes, the operands with
their planted ties and edge negatives, a mirror of the dispatch of bwd_bf16() / fwd_bf16() (csrc/tt_score_bf16.hip), the
per-element bar on the gradient, and an f32 + bf16 emulation of the kernels' arithmetic that shows the bar can pass and can fail.

A "group" is one problem (Ra, Rb, off, D, T, unit): Rb notice rows and Rb company rows, of which the Ra rows off .. off + Ra - 1
are the caller's own (global in-batch negatives; Ra == Rb, off == 0 is the square problem).  Direction 0 is A = own notices
against B = all companies, direction 1 is A = own companies against B = all notices; the positive of own row a is column a + off.
"""
from collections import namedtuple

import numpy as np

import oracle_np as O

U24 = 2.0 ** -24

Group = namedtuple("Group", "Ra Rb off D T unit")

# square B, D, T, unit form: every B of {1, 31, 32, 33, 63, 64, 65, 127, 129, 257, 300}, 127 / 129 / 255 / 257 rows either side of the
# rows forms' workgroups (128 rows at padded D = 256, 256 rows below), every D of {1, 8, 32 | 33, 64 | 65, 128 | 129, 200, 256}
SQUARE = [(1, 1, 1.0, True), (31, 8, 0.5, False), (32, 32, 2.0, True), (33, 33, 0.07, False), (63, 64, 0.025, True),
          (64, 65, 1.0, False), (65, 128, 0.5, True), (127, 129, 2.0, False), (129, 200, 0.07, True), (257, 256, 0.025, False),
          (300, 64, 1.0, True), (255, 64, 0.5, False), (257, 128, 2.0, False), (255, 65, 0.07, True), (129, 33, 0.025, False),
          (127, 256, 1.0, True), (300, 8, 0.07, False), (65, 32, 0.025, True), (1, 200, 0.5, False)]
# (Ra, Rb, off): offsets that are no multiple of 32 (70, 90, 37, 1953); positives that end in the ragged last tile ((45, 135, 90),
# (96, 2049, 1953), (33, 65, 32)); fewer b tiles than waves ((33, 65, 32): 3 tiles, 8 or 4 waves)
RECT_SHAPES = [(70, 210, 70), (45, 135, 90), (64, 1000, 37), (96, 2049, 1953), (33, 65, 32)]
RECT = [((70, 210, 70), 64, 1.0, True), ((70, 210, 70), 256, 0.5, False), ((45, 135, 90), 32, 0.07, False),
        ((45, 135, 90), 128, 2.0, True), ((64, 1000, 37), 128, 0.025, False), ((64, 1000, 37), 8, 1.0, True),
        ((96, 2049, 1953), 200, 0.07, True), ((96, 2049, 1953), 33, 0.5, False), ((33, 65, 32), 65, 0.025, True),
        ((33, 65, 32), 1, 2.0, False)]
GROUPS = [Group(B, B, 0, D, T, u) for B, D, T, u in SQUARE] + [Group(*s, D, T, u) for s, D, T, u in RECT]

ROWS_MIN_DEFAULT = 32768
ROWS_ALWAYS, ROWS_NEVER = 1, 1000000000          # TT_OPT_SCORE_BWD_ROWS_MIN: the rows form from one row up / never


def group_id(g):
    return f"Ra{g.Ra}-Rb{g.Rb}-off{g.off}-D{g.D}-T{g.T}-{'unit' if g.unit else 'nonunit'}"


def padded_d(D):
    return 32 if D <= 32 else (64 if D <= 64 else (128 if D <= 128 else 256))


# ---- the dispatch, as csrc/tt_score_bf16.hip has it ---------------------------------------------------------------------------
FWD_KERNELS = {32: "score_fwd_bf16_kernel<2,2,8>", 64: "score_fwd_bf16_kernel<4,1,8>", 128: "score_fwd_bf16_kernel<8,2,8>",
               256: "score_fwd_bf16_kernel<16,1,8>"}
BWD_SMALL = {32: "score_bwd_bf16_kernel<2,2,8>", 64: "score_bwd_tr_kernel<4,2>", 128: "score_bwd_tr_kernel<8,1>",
             256: "score_bwd_bf16_kernel<16,1,4>"}
BWD_ROWS = {64: "score_bwd_rows_kernel<4,.,2,4>", 128: "score_bwd_rows_kernel<8,.,2,4>", 256: "score_bwd_rows_kernel<16,.,1,4>"}
BWD_WAVES = {"score_bwd_bf16_kernel<2,2,8>": 8, "score_bwd_tr_kernel<4,2>": 8, "score_bwd_tr_kernel<8,1>": 8,
             "score_bwd_bf16_kernel<16,1,4>": 4}


def fwd_kernel(D, unit):
    """(kernel, unit form) fwd_bf16() launches"""
    return FWD_KERNELS[padded_d(D)], bool(unit)


def bwd_kernel(D, max_ra, rows_min, unit):
    """(kernel, unit form) bwd_bf16() launches for padded D and the larger Ra of the call at TT_OPT_SCORE_BWD_ROWS_MIN = rows_min
    (TT_OPT_FUSE_SCORE_TAIL = 0)"""
    Dp = padded_d(D)
    if max_ra >= rows_min and Dp >= 64:
        return BWD_ROWS[Dp], bool(unit)
    return BWD_SMALL[Dp], bool(unit)


def bwd_variants(g):
    """the backward calls of a group: (rows_min, reciprocals given) -- padded D = 32 has no rows form"""
    forms = (ROWS_NEVER, ROWS_ALWAYS) if padded_d(g.D) >= 64 else (ROWS_NEVER,)
    return [(rm, inv) for rm in forms for inv in (True, False)]


# ---- operands -----------------------------------------------------------------------------------------------------------------
def _unit(x):
    return (x / np.linalg.norm(x, axis=-1, keepdims=True)).astype(np.float32)


def _near(rng, row):
    """the row plus 5 % noise, renormalised"""
    g = rng.standard_normal(row.shape)
    return _unit(row.astype(np.float64) + 0.05 * g / np.linalg.norm(g))


Problem = namedtuple("Problem", "g n c edges ties")


def make_problem(g, seed=None):
    """Unit rows n, c [Rb, D] f32 (c correlated with n) with, in this order,
    - hard negatives at the ragged edges of b: rows Rb - 1, Rb - 2 and 32 * floor((Rb - 1) / 32) of c are own notice rows plus 5 %
      noise, the same rows of n own company rows plus 5 % noise (never the a-row's own positive: a-rows are taken off the edges);
    - ties: for one own notice a1 (positive p1 = a1 + off, made the row's clear maximum) the company rows p1 - 35 (before the
      positive), p1 + 37 (after it) and p1 ^ 1 (inside the positive's tile) are copies of row p1, as far as they exist; the same
      with -38 / +41 / ^ 1 in n for one own company a2.
    edges: the planted edge rows; ties: {direction: (own row a, positive p, [copies])}."""
    Ra, Rb, off, D = g.Ra, g.Rb, g.off, g.D
    rng = np.random.default_rng(seed if seed is not None else 1000003 * Rb + 1009 * Ra + 31 * D + off)
    n = rng.standard_normal((Rb, D))
    c = 0.5 * n + rng.standard_normal((Rb, D))
    n, c = _unit(n), _unit(c)
    edge_rows = sorted({r for r in (Rb - 1, Rb - 2, 32 * ((Rb - 1) // 32)) if r >= 0})
    used = set(edge_rows)                                             # rows that are planted or that a planting leans on
    cand = [a for a in range(Ra) if a + off not in used]
    edges = []
    if cand:
        for i, e in enumerate(edge_rows):
            a0, a1 = cand[i % len(cand)], cand[(i + 1) % len(cand)]
            c[e] = _near(rng, n[off + a0])
            n[e] = _near(rng, c[off + a1])
            used.update((off + a0, off + a1))
            edges.append(e)
    ties = {}
    for direction, (d_before, d_after) in enumerate(((35, 37), (38, 41))):
        free = [a for a in range(Ra) if a + off not in used]
        if not free:
            continue
        mid = free[len(free) // 2]                                       # the free row nearest the middle whose tile mate is free too
        mated = [a for a in sorted(free, key=lambda a: abs(a - mid)) if (a + off) ^ 1 < Rb and (a + off) ^ 1 not in used]
        a = mated[0] if mated else mid
        p = a + off
        dst, src = (c, n) if direction == 0 else (n, c)
        copies = [j for j in (p - d_before, p + d_after, p ^ 1) if 0 <= j < Rb and j not in used and j != p]
        dst[p] = _near(rng, src[p])
        for j in copies:
            dst[j] = dst[p]
        used.update([p] + copies)
        ties[direction] = (a, p, copies)
    return Problem(g, n, c, edges, ties)


def unit_scale(T):
    """tt_score_unit_scale(1 / T) = f32(1 / T) * f32(log2 e), in f32"""
    return float(np.float32(np.float32(1.0 / T) * np.float32(O.LOG2E)))


def operands(p):
    """(nb, cb) f64 [Rb, D]: the values the kernels' MFMAs see, unscaled -- O.score_operands_bf16 for the unit form (the notice
    image is packed times tt_score_unit_scale), q_bf16 of both sides for scale 1"""
    n64, c64 = p.n.astype(np.float64), p.c.astype(np.float64)
    return O.score_operands_bf16(n64, c64, p.g.T) if p.g.unit else (O.q_bf16(n64), O.q_bf16(c64))


def directions(p, nb, cb):
    """per direction (A [Ra, D], B [Rb, D]) of the f64 operands"""
    s = slice(p.g.off, p.g.off + p.g.Ra)
    return (nb[s], cb), (cb[s], nb)


# ---- the bar ------------------------------------------------------------------------------------------------------------------
def rho(g):
    """2^-8: the round-to-nearest bf16 rounding of the weight, the gradient MFMA's operand (the reference's W is not rounded).
    bf16 keeps 8 significant bits, so neighbours in [1, 2) are 2^-7 apart and a value just above 1 moves by up to 2^-8 of itself
    -- not 2^-9, which holds only at the top of a binade: one weight of 1.089 (a row whose positive has one exact copy: e / sum_a
    = 1/2 twice) rounds to 1.0859, 3.6e-3 of itself, and such a row's gradient is that one term;
    2 Dp 2^-24 / T: the f32 accumulation of the exponent's argument, once in the recompute and once in the forward's sums
    (|n . c| <= 1 for unit rows); (Rb + 16) 2^-24: the f32 accumulation over b, plus exp2, rcp, add and multiply."""
    return 2.0 ** -8 + 2 * padded_d(g.D) * U24 / g.T + (g.Rb + 16) * U24


def grad_reference(g, A, Bm, sum_a, sum_b, k):
    """(k W B, k mag |B|) in f64 for one direction, W and mag from O.score_dir_terms on the kernels' operands and sums"""
    W, mag = O.score_dir_terms(A, Bm, g.T, g.off, np.asarray(sum_a, dtype=np.float64), np.asarray(sum_b, dtype=np.float64))
    return k * (W @ Bm), k * (mag @ np.abs(Bm))


def bound_fraction(got, ref, magsum, factor):
    """max over the elements of |got - ref| / (factor * magsum): <= 1 is inside the bar.  (An element whose magnitude sum is 0
    -- an all-zero column of B -- must be exact.)"""
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    lim = factor * magsum
    frac = np.where(lim > 0, err / np.where(lim > 0, lim, 1.0), np.where(err > 0, np.inf, 0.0))
    return float(frac.max())


# forward bars (test_gpu_score_bf16_forms.py, section B)
def sumexp_rtol(g):
    return padded_d(g.D) * U24 / g.T + (g.Rb + 8) * U24


def diag_atol(g):
    return padded_d(g.D) * U24 / g.T


def sumscore_factor(g):
    return (g.Rb + padded_d(g.D)) * U24


def rank_bracket(S, M_cols, delta, off=0):
    """per row i of S [Ra, Rb] (positive at column i + off): f64 counts #{j : s_ij > s_ip + d_i} and #{j : s_ij >= s_ip - d_i}, with
    exact ties (bitwise equal operand rows M_cols[j] == M_cols[i + off]: equal scores in every arithmetic) placed by the lower-index
    rule.  The second count includes the positive itself."""
    Ra = S.shape[0]
    d = S[np.arange(Ra), np.arange(Ra) + off][:, None]
    lo = (S > d + delta[:, None]).sum(1)
    hi = (S >= d - delta[:, None]).sum(1)
    groups = {}
    for j, row in enumerate(M_cols):
        groups.setdefault(row.tobytes(), []).append(j)
    for js in groups.values():
        for j in js:
            i = j - off
            if 0 <= i < Ra:
                lo[i] += sum(jj < j for jj in js)      # an exact tie before the positive counts ...
                hi[i] -= sum(jj > j for jj in js)      # ... one after it does not
    return lo, hi


# ---- f32 + bf16 emulation of the kernels' arithmetic ----------------------------------------------------------------------------
def _q32(x):
    return O.q_bf16(np.asarray(x, dtype=np.float32))


def emulate(p, fault=None):
    """The backward of both directions as the kernels compute it, in numpy f32 with bf16-rounded operands and weights: products
    accumulated in f32, exp2 of the accumulator (unit form) or of fma(acc, c1, c2), f32 sums and reciprocals, the weight
    e (1 / sum_a + 1 / sum_b) - 2 [positive] rounded to bf16, the gradient product accumulated in f32.  (numpy's summation order is
    not the kernels': the emulation shows what the arithmetic costs, not the kernels' bits.)
    fault = "drop_last": the weight of b = Rb - 1 is masked away (an off-by-one in the ragged last tile's mask);
    fault = "shift_pos": the -2 of the positive lands one column to the right (to the left from the last column; nowhere at Rb = 1).
    Returns per direction (dA f32 [Ra, D], sum_a f32 [Ra], sum_b f32 [Rb], k): the sums as the forward stores them."""
    g = p.g
    f32 = np.float32
    inv_t = f32(1.0 / g.T)
    sn = f32(unit_scale(g.T)) if g.unit else f32(1.0)
    PN, PC = _q32(p.n * sn), _q32(p.c)
    acc = PN @ PC.T                                                   # [notice, company], f32
    c2 = f32(-inv_t * f32(O.LOG2E))
    if g.unit:
        E = np.exp2(acc)
        kexp = np.exp2(c2)
    else:
        E = np.exp2(acc * f32(inv_t * f32(O.LOG2E)) + c2)
        kexp = f32(1.0)
    raw_r, raw_c = E.sum(1, dtype=f32), E.sum(0, dtype=f32)
    rs, cs = raw_r * kexp, raw_c * kexp                               # as stored
    ir, ic = f32(1.0) / raw_r, f32(1.0) / raw_c
    k = f32(inv_t / f32(2 * g.Rb))
    s = slice(g.off, g.off + g.Ra)
    out = []
    for direction in (0, 1):
        Ed = E[s, :] if direction == 0 else E.T[s, :]
        ia, ib = (ir[s], ic) if direction == 0 else (ic[s], ir)
        sa, sb = (rs[s], cs) if direction == 0 else (cs[s], rs)
        Bimg, bscale = (PC, f32(1.0)) if direction == 0 else (PN, sn)
        w = (Ed * (ia[:, None] + ib[None, :])).astype(f32)
        if fault == "drop_last":
            w[:, g.Rb - 1] = 0
        pos = np.arange(g.Ra) + g.off
        if fault == "shift_pos":
            pos = np.where(pos + 1 < g.Rb, pos + 1, pos - 1)
        ok = (pos >= 0) & (pos < g.Rb)
        w[np.arange(g.Ra)[ok], pos[ok]] -= f32(2.0)
        dA = (_q32(w) @ Bimg) * f32(k / bscale)
        out.append((dA, sa, sb, float(k)))
    return out


def emulation_fraction(p, fault=None):
    """largest fraction of the bar over both directions of the emulated backward"""
    nb, cb = operands(p)
    worst = 0.0
    for (A, Bm), (dA, sa, sb, k) in zip(directions(p, nb, cb), emulate(p, fault)):
        ref, magsum = grad_reference(p.g, A, Bm, sa, sb, k)
        worst = max(worst, bound_fraction(dA, ref, magsum, rho(p.g)))
    return worst
