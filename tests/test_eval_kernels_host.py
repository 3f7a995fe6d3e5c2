"""The references and bars of tests/test_gpu_eval_kernels.py, shown sound without a GPU: the derived f32 GEMM bar against an f32
emulation in two summation orders, the top-k and rank references against brute-force loops (ties, +-0, +-inf, NaN, the -1 and
(-inf, -1) conventions), and the evaluator's R > C formulae against a numpy transcription of the reference's topk comparison."""
import json

import numpy as np
import pytest
import torch

import oracle_np as O

U = 2.0 ** -24          # unit roundoff of f32

# (M, N, K) of the tt_linear_fwd cases: every M of {0, 1, 2, 63, 65, 130}, N of {1, 33, 64, 65, 200} and K of
# {1, 3, 16, 17, 64, 130, 768} at least once, the corners (1, 1, 1) and (130, 200, 768), and (130, 200, K) at a vector K, a
# scalar K and a long K for the position checks
TRIPLES = [(1, 1, 1), (130, 200, 768), (130, 200, 64), (130, 200, 17), (0, 33, 16), (2, 64, 3), (63, 65, 130), (65, 33, 16),
           (65, 64, 64), (1, 200, 17), (2, 1, 768), (63, 33, 1), (130, 65, 3), (65, 200, 130), (63, 64, 768)]


# ---- references (shared with tests/test_gpu_eval_kernels.py) ------------------------------------------------------------------------
def gemm_problem(seed, M, N, K):
    """f32 x [M, K], w [N, K], b [N], zero-mean: about half of the pre-activations x w^T + b are negative."""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((M, K)).astype(np.float32), rng.standard_normal((N, K)).astype(np.float32),
            rng.standard_normal(N).astype(np.float32))


def gemm_ref(x, w, b=None, alpha=1.0, relu=False, extra=4):
    """(y64, bar) of y = alpha * sum_k x_k w_k + b on f32 inputs: the float64 value and the per-element gamma bound
    (K + extra) * 2^-24 * (|alpha| sum_k |x_k w_k| + |b|) of ANY f32 accumulation order -- K product roundings and K - 1 additions
    sit on every term at most, one more each for alpha and the bias; (K + 2) u / (1 - (K + 2) u) <= (K + 4) u while
    (K + 2)(K + 4) u <= 2, i.e. up to K of a few thousand.  ReLU is 1-Lipschitz: the same bar."""
    x64, w64 = np.asarray(x, np.float64), np.asarray(w, np.float64)
    K = x64.shape[1]
    y = alpha * (x64 @ w64.T)
    mag = abs(alpha) * (np.abs(x64) @ np.abs(w64).T)
    if b is not None:
        y = y + np.asarray(b, np.float64)[None, :]
        mag = mag + np.abs(np.asarray(b, np.float64))[None, :]
    if relu:
        y = np.maximum(y, 0.0)
    return y, (K + extra) * U * mag


def bar_fraction(got, y64, bar):
    """largest |got - y64| / bar (0 for an empty problem; an element with a zero bar must be exact)"""
    got = np.asarray(got, np.float64)
    assert got.shape == y64.shape, (got.shape, y64.shape)
    if got.size == 0:
        return 0.0
    err = np.abs(got - y64)
    assert np.all(np.isfinite(got))
    assert np.all(err[bar == 0] == 0)
    return float(np.max(np.where(bar > 0, err / np.where(bar > 0, bar, 1.0), 0.0)))


def ref_topk_rows(S, k):
    """tt_topk_rows: per row the k best entries, value descending, ties (+0 == -0 among them) to the lower column -- the stable
    rule of oracle_np.topk_rows; a NaN is never selected, and slots beyond the row's non-NaN entries are (-inf, -1).  vals are the
    selected ELEMENTS (f32, their own bits)."""
    S = np.asarray(S, np.float32)
    R = S.shape[0]
    vals = np.full((R, k), -np.inf, np.float32)
    idx = np.full((R, k), -1, np.int64)
    for r in range(R):
        order = np.argsort(-S[r], kind="stable")            # numpy sorts NaN behind everything
        order = order[~np.isnan(S[r][order])][:k]
        vals[r, :order.size] = S[r][order]
        idx[r, :order.size] = order
    return vals, idx


def ref_diag_rank(S, off=0):
    """tt_diag_rank_rows: #{c : s > s_p} + #{c < p : s == s_p} with p = r + off; -1 where p is outside [0, C)."""
    S = np.asarray(S)
    R, C = S.shape
    out = np.full(R, -1, np.int64)
    for r in range(R):
        p = r + off
        if 0 <= p < C:
            out[r] = int((S[r] > S[r, p]).sum() + (S[r, :p] == S[r, p]).sum())
    return out


def recall_at_k_formula(S, k):
    """The reference's Recall@K (src/evaluation/evaluator.py:20-43) written out in numpy: the top min(k, C) columns of every
    row compared with the row's own index; a row whose index is no column (R > C) can never match: a miss."""
    S = np.asarray(S)
    R, C = S.shape
    top = np.argsort(-S, axis=1, kind="stable")[:, :min(k, C)]
    return float(np.mean((top == np.arange(R)[:, None]).any(axis=1).astype(np.float32)))


def mrr_formula(S):
    """The reference's MRR (:45-71): the position of column i in row i's descending order; where there is no such column the
    reference's `.nonzero().item()` fails on an empty match -- ValueError here."""
    S = np.asarray(S)
    order = np.argsort(-S, axis=1, kind="stable")
    rr = []
    for i in range(S.shape[0]):
        pos = np.nonzero(order[i] == i)[0]
        if pos.size != 1:
            raise ValueError(f"row {i}: no column {i}")
        rr.append(1.0 / (pos[0] + 1))
    return float(np.mean(np.asarray(rr, np.float32)))


def special_rows():
    """Rows over 9 columns with ties, +-0, +-inf and NaN (for k up to 9)."""
    inf, nan = np.inf, np.nan
    return np.array([[1.0, 3.0, 3.0, 2.0, 3.0, -1.0, 2.0, 0.5, 3.0],
                     [0.0, -0.0, 0.0, -0.0, -1.0, 1.0, -0.0, 0.0, -2.0],
                     [-0.0, 0.0, -inf, inf, -inf, 5.0, inf, -0.0, -inf],
                     [-inf, -inf, -inf, -inf, -inf, -inf, -inf, -inf, -inf],
                     [nan, 1.0, nan, 1.0, -inf, nan, 2.0, nan, -0.0],
                     [nan, nan, nan, nan, nan, nan, nan, nan, nan],
                     [nan, nan, nan, nan, -inf, nan, nan, nan, nan],
                     [7.0, 7.0, 7.0, 7.0, 7.0, 7.0, 7.0, 7.0, 7.0]], np.float32)


# ---- the bar -----------------------------------------------------------------------------------------------------------------------
def _f32_gemm(x, w, b, alpha, relu, reverse):
    """y = alpha * sum_k x_k w_k + b with every product and every partial sum rounded to f32, k ascending or descending"""
    acc = np.zeros((x.shape[0], w.shape[0]), np.float32)
    ks = range(x.shape[1] - 1, -1, -1) if reverse else range(x.shape[1])
    for k in ks:
        acc = (acc + (x[:, k, None] * w[None, :, k]).astype(np.float32)).astype(np.float32)
    y = (acc * np.float32(alpha)).astype(np.float32)
    if b is not None:
        y = (y + b[None, :]).astype(np.float32)
    return np.maximum(y, np.float32(0)) if relu else y


@pytest.mark.parametrize("M,N,K", TRIPLES)
def test_gamma_bar_holds_for_an_f32_gemm_in_either_order(M, N, K):
    x, w, b = gemm_problem(1000 + 7 * M + 3 * N + K, M, N, K)
    worst = {}
    for bias, relu, alpha in ((True, False, 1.0), (False, True, 1.0), (True, True, 1.0), (False, False, 20.0)):
        y64, bar = gemm_ref(x, w, b if bias else None, alpha, relu)
        for reverse in (False, True):
            f = bar_fraction(_f32_gemm(x, w, b if bias else None, alpha, relu, reverse), y64, bar)
            worst["rev" if reverse else "fwd"] = max(worst.get("rev" if reverse else "fwd", 0.0), f)
    print("\n[gamma-bar-host]", json.dumps({"M": M, "N": N, "K": K, **worst}))
    assert max(worst.values()) <= 1.0, worst


def test_bar_is_not_vacuous():
    """operands rounded to bf16 on the way in (the towers' other compute mode) miss the bar by orders of magnitude"""
    x, w, b = gemm_problem(5, 65, 33, 16)
    y64, bar = gemm_ref(x, w, b)
    xb = torch.from_numpy(x).bfloat16().float().numpy()
    assert bar_fraction(_f32_gemm(x, w, b, 1.0, False, False), y64, bar) <= 1.0
    assert bar_fraction(_f32_gemm(xb, w, b, 1.0, False, False), y64, bar) > 50.0


# ---- top-k and rank references against brute force -----------------------------------------------------------------------------------
def _brute_topk(row, k):
    """k selection passes in plain Python: the best not-yet-taken non-NaN entry, the lower column among equals"""
    taken, vals, idx = set(), [], []
    for _ in range(k):
        best = None
        for c, v in enumerate(row):
            if c in taken or v != v:
                continue
            if best is None or v > row[best]:
                best = c
        if best is None:
            vals.append(np.float32(-np.inf))
            idx.append(-1)
        else:
            taken.add(best)
            vals.append(row[best])
            idx.append(best)
    return vals, idx


def _brute_rank(row, p):
    if not 0 <= p < len(row):
        return -1
    n = 0
    for c, v in enumerate(row):
        if v > row[p] or (v == row[p] and c < p):
            n += 1
    return n


def _tie_rows(rng, R, C):
    return rng.choice(np.array([-1.5, 0.25, 0.25, 2.0], np.float32), size=(R, C))


@pytest.mark.parametrize("k", [1, 4, 9])
def test_topk_reference_equals_brute_force(k):
    rng = np.random.default_rng(11)
    S = np.concatenate([special_rows(), _tie_rows(rng, 6, 9), rng.standard_normal((4, 9)).astype(np.float32)])
    vals, idx = ref_topk_rows(S, k)
    for r in range(S.shape[0]):
        bv, bi = _brute_topk(S[r], k)
        assert idx[r].tolist() == bi, r
        assert vals[r].view(np.int32).tolist() == np.asarray(bv, np.float32).view(np.int32).tolist(), r    # the element's own sign of zero
    # the stable rule of oracle_np.topk_rows wherever no NaN is involved
    clean = ~np.isnan(S).any(axis=1)
    ov, oi = O.topk_rows(S[clean], k)
    assert np.array_equal(oi, idx[clean]) and np.array_equal(ov.view(np.int32), vals[clean].view(np.int32))


def test_topk_reference_conventions():
    vals, idx = ref_topk_rows(special_rows(), 9)
    assert idx[0].tolist() == [1, 2, 4, 8, 3, 6, 0, 7, 5]
    assert idx[1].tolist() == [5, 0, 1, 2, 3, 6, 7, 4, 8]                       # +-0 are equal: column order
    assert np.signbit(vals[1, 1:7]).tolist() == [False, True, False, True, True, False]
    assert idx[2].tolist() == [3, 6, 5, 0, 1, 7, 2, 4, 8]                       # -inf entries keep their own columns
    assert idx[3].tolist() == list(range(9))
    assert idx[4].tolist() == [6, 1, 3, 8, 4, -1, -1, -1, -1]                   # a NaN is never selected
    assert np.all(np.isneginf(vals[4, 4:]))
    assert idx[5].tolist() == [-1] * 9 and np.all(np.isneginf(vals[5]))
    assert idx[6].tolist() == [4] + [-1] * 8
    assert idx[7].tolist() == list(range(9))


@pytest.mark.parametrize("off", [0, 3, -2, 8, -8, 9, -9])
def test_rank_reference_equals_brute_force(off):
    rng = np.random.default_rng(12)
    S = np.concatenate([special_rows(), _tie_rows(rng, 6, 9)])
    got = ref_diag_rank(S, off)
    assert got.tolist() == [_brute_rank(S[r], r + off) for r in range(S.shape[0])]
    outside = [not 0 <= r + off < 9 for r in range(S.shape[0])]
    assert (got == -1).tolist() == outside                                      # -1 exactly where there is no positive


def test_rank_reference_agrees_with_the_retrieval_and_oracle_rules():
    from test_retrieval_host import ref_rank
    rng = np.random.default_rng(13)
    S = _tie_rows(rng, 9, 9)
    assert ref_diag_rank(S).tolist() == ref_rank(S, np.arange(9)).tolist() == O.diag_rank_stable(S).tolist()


# ---- the evaluator on R != C --------------------------------------------------------------------------------------------------------
def _recall_from_ranks(S, k):
    """what TwoTowerEvaluator.compute_recall_at_k forms from tt_diag_rank_rows's ranks"""
    rank = ref_diag_rank(S)
    return float(np.mean(((rank >= 0) & (rank < min(k, S.shape[1]))).astype(np.float32)))


@pytest.mark.parametrize("R,C", [(70, 33), (33, 70), (33, 33)])
def test_rank_formulae_equal_the_references_topk_comparison(R, C):
    rng = np.random.default_rng(14)
    S = rng.standard_normal((R, C)).astype(np.float32)
    S[np.arange(min(R, C)), np.arange(min(R, C))] += np.float32(1.0)            # some hits
    S[1, :4] = S[1, 1]                                                          # ties around a positive: the stable order on both sides
    for k in (1, 5, 10, 200):
        assert _recall_from_ranks(S, k) == recall_at_k_formula(S, k), k
    if R > C:
        assert round(recall_at_k_formula(S, 5) * R) <= C                        # rows C.. are misses ...
        as_hits = np.where(ref_diag_rank(S) < 0, 0, ref_diag_rank(S))           # (rank 0 there would count them as hits)
        assert float(np.mean((as_hits < 5).astype(np.float32))) > recall_at_k_formula(S, 5)
        with pytest.raises(ValueError):                                         # ... and have no reciprocal rank
            mrr_formula(S)
    else:
        mrr = float(np.mean((1.0 / (ref_diag_rank(S) + 1.0)).astype(np.float32)))
        assert mrr == pytest.approx(mrr_formula(S), rel=1e-6)


def test_evaluator_refuses_mrr_without_positives_before_any_launch():
    """compute_mrr / compute_comprehensive_metrics on R > C raise from the shapes: on a CPU tensor nothing else could."""
    import jodalrob_twotower_amd as tt
    ev = tt.TwoTowerEvaluator(device="cpu")
    S = torch.zeros(70, 33)
    with pytest.raises(ValueError, match="no positive column"):
        ev.compute_mrr(S)
    with pytest.raises(ValueError, match="no positive column"):
        ev.compute_comprehensive_metrics(S, {})
