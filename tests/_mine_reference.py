"""The f64 reference of hard-negative mining: masked scores, the score ceiling, top-k under the index tie rule, the miner's
selection and the loader's draw rule -- and the shared inputs of the host and the GPU tests (made on the CPU, so that both see
the same numbers).  Everything here is torch on whatever device its inputs live on; nothing calls the library."""
import numpy as np
import torch

NEG_INF = -float("inf")

# (nQ, nC, D, k, inv_t): ragged tiles, a ragged query tile, every KS (D = 6 / 64 / 128 / 200), the scalar f32 tile (D = 6), and
# both sweep forms (k <= 64 and k > 64)
CASES = [
    (1, 33, 6, 1, 1.0),
    (33, 1000, 200, 64, 1.0),
    (300, 1000, 6, 10, 0.05),
    (33, 65537, 64, 10, 0.05),
    (33, 65537, 64, 65, 1.0),
    (7, 4099, 128, 200, 1.0),
]


def tolerance(bf16, inv_t):
    """the score tolerance of test_gpu_retrieval_exclude.py"""
    return (1e-5 if bf16 else 2e-6) * max(1.0, inv_t) + 1e-6


def unit_rows(n, d, g):
    x = torch.randn((n, d), generator=g, dtype=torch.float32)
    return x / x.norm(dim=1, keepdim=True)


def make_case(nQ, nC, D, k):
    """(Q, Cm) f32 unit rows on the CPU, and (off, rows) numpy exclusion lists: ascending, up to nC // 8 rows per query, with
    duplicates and rows outside [0, nC)."""
    g = torch.Generator().manual_seed(nQ * 5 + nC + D + k)
    rng = np.random.default_rng(nQ + nC + D + k)
    Q, Cm = unit_rows(nQ, D, g), unit_rows(nC, D, g)
    lens = rng.integers(0, min(300, nC // 8) + 1, nQ)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    rows = np.concatenate([np.sort(rng.integers(-2, nC + 2, n)) for n in lens] + [np.zeros(0, np.int64)]).astype(np.int32)
    return Q, Cm, off, rows


def ref_scores(Q, Cm, inv_t, bf16):
    """f64 scores of the operands as the library rounds them (bf16: queries unscaled, catalogue times inv_t, both rounded)"""
    if bf16:
        return Q.float().to(torch.bfloat16).double() @ (Cm * inv_t).to(torch.bfloat16).double().T
    return (Q.double() @ Cm.double().T) * inv_t


def mask_scores(S, off, rows):
    """-inf at every (q, excluded row in range)"""
    M = S.clone()
    off, rows = np.asarray(off), np.asarray(rows)
    q = np.repeat(np.arange(S.shape[0]), np.diff(off))
    ok = (rows >= 0) & (rows < S.shape[1])
    M[torch.as_tensor(q[ok], device=S.device), torch.as_tensor(rows[ok].astype(np.int64), device=S.device)] = NEG_INF
    return M


def apply_ceiling(M, ceil):
    """-inf where M >= ceil[q] (a NaN ceiling compares false and removes nothing)"""
    return torch.where(M >= ceil.to(M.dtype)[:, None], torch.full_like(M, NEG_INF), M)


def topk_index_rule(M, k):
    """(vals, idx): per row the k best, value descending, ties to the lower index; (-inf, -1) where no finite entry is left"""
    order = torch.sort(-M, dim=1, stable=True).indices[:, :k]            # stable: equal values keep their index order
    vals = torch.gather(M, 1, order)
    return vals, torch.where(torch.isfinite(vals), order, torch.full_like(order, -1))


def gap_ceilings(M, tol):
    """Per query the midpoint of the widest gap among its reference scores at ranks 3 to 12 (0-based, descending), and ok [nQ]:
    the gap is at least 8 tol wide, so every reference score lies 4 tol or more from the ceiling.  Queries with fewer than 13
    finite scores, or without such a gap, are not ok (their ceiling is +inf)."""
    nQ, nC = M.shape
    ceil = torch.full((nQ,), float("inf"), dtype=torch.float64, device=M.device)
    ok = torch.zeros(nQ, dtype=torch.bool, device=M.device)
    if nC < 13:
        return ceil.float(), ok
    top = torch.topk(M, 13, dim=1).values[:, 3:]                          # ranks 3 .. 12
    gap = top[:, :-1] - top[:, 1:]
    w, j = gap.max(dim=1)
    mid = (torch.gather(top, 1, j[:, None]) + torch.gather(top, 1, j[:, None] + 1))[:, 0] / 2
    ok = torch.isfinite(top[:, -1]) & (w >= 8 * tol)
    c32 = mid.float()                                                    # the ceiling the library gets; still 4 tol from every score?
    ok &= (M - c32.double()[:, None]).abs().min(dim=1).values >= 4 * tol
    return torch.where(ok, c32, torch.full_like(c32, float("inf"))), ok


def check_topk(M, vals, idx, k, tol, rows=None):
    """The library's (vals, idx) against the masked (and ceiled) f64 reference M, for the queries `rows` (default: all): as
    test_gpu_retrieval_exclude's check -- the first n_eligible slots hold eligible rows, their values within tol, none worse than
    the reference's k-th best by more than tol, distinct, in order; the rest are -inf / -1."""
    if rows is not None:
        M, vals, idx = M[rows], vals[rows], idx[rows]
    nQ = M.shape[0]
    assert vals.shape == idx.shape == (nQ, k)
    if nQ == 0:
        return
    elig = torch.isfinite(M).sum(1).clamp(max=k)
    slot = torch.arange(k, device=M.device)[None, :]
    real = slot < elig[:, None]
    assert bool((idx[~real] == -1).all()) and bool((vals[~real] == NEG_INF).all())
    assert bool((idx[real] >= 0).all()) and bool((idx[real] < M.shape[1]).all())
    got = torch.gather(M, 1, idx.clamp(min=0))
    assert bool(torch.isfinite(got[real]).all())                         # never an excluded row or one at / above the ceiling
    err = (got[real] - vals[real].double()).abs()
    assert err.numel() == 0 or float(err.max()) <= tol
    kth = torch.gather(torch.topk(M, k, dim=1).values, 1, (elig - 1).clamp(min=0)[:, None])
    assert bool((got[real] >= (kth.expand(-1, k)[real] - tol)).all())
    srt = torch.sort(torch.where(real, idx, -1 - slot), dim=1).values
    assert bool((srt[:, 1:] != srt[:, :-1]).all())
    dv = vals[:, 1:] - vals[:, :-1]
    both = real[:, 1:]
    assert bool((dv[both] <= 0).all())
    assert bool(((dv < 0) | (idx[:, 1:] > idx[:, :-1]))[both].all())


# ---- mining ----------------------------------------------------------------------------------------------------------------------
def mine_reference(S, pairs, n_notices, k, per_notice, ceiling):
    """The miner's rule on a score matrix S [n_notices, nC] (numpy, any float type; the comparisons are exact in it).  Returns
    (table int32 [n_notices, per_notice], cand: notice -> its up-to-k rows in order, ceil: notice -> its ceiling or None).
    Per notice with pairs: known = its companies; s_min = the lowest score of them; ceil = f32(alpha) * s_min + f32(beta) in f32;
    eligible = rows outside known with S < ceil; order = value descending, lower row first; table row = the first per_notice."""
    S = np.asarray(S)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    table = np.full((n_notices, per_notice), -1, dtype=np.int32)
    cand, ceils = {}, {}
    for n in np.unique(pairs[:, 0]):
        known = np.unique(pairs[pairs[:, 0] == n, 1])
        s = S[n]
        c = None
        ok = np.ones(s.shape[0], dtype=bool)
        ok[known] = False
        if ceiling is not None:
            s_min = np.float32(s[known].min())
            c = np.float32(np.float32(np.float32(ceiling[0]) * s_min) + np.float32(ceiling[1]))
            ok &= ~(s >= c)
        rows = np.nonzero(ok)[0]
        rows = rows[np.lexsort((rows, -s[rows].astype(np.float64)))][:k]
        cand[int(n)], ceils[int(n)] = rows, c
        table[n, :min(per_notice, len(rows))] = rows[:per_notice]
    return table, cand, ceils


# ---- the loader's draw --------------------------------------------------------------------------------------------------------------
def batch_candidates(table, notice_rows):
    """The proposal of a batch's mined slots: the valid (>= 0) entries of table[notice rows of the batch], one table row per pair of
    the batch, in pair order then slot order.  A mined slot is a uniform draw (with replacement) from this list, and carries
    log q = -log(len(list)); an empty list means the batch falls back to the uniform draw over the store."""
    t = np.asarray(table)[np.asarray(notice_rows, dtype=np.int64)].reshape(-1)
    return t[t >= 0]


def draw_from(cands, u):
    """the entry a uniform u in [0, 1) selects"""
    return cands[min(int(u * len(cands)), len(cands) - 1)]
