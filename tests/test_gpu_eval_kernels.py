"""The dense evaluation kernels and the similarity autograd node against f64 at ragged shapes: tt_linear_fwd (FeatureProjector),
tt_score_matrix, _SimilarityFn forward / backward (TwoTowerModel.compute_similarity), tt_topk_rows (predict_batch) and
tt_diag_rank_rows (TwoTowerEvaluator).

The bar of the f32 GEMM entries is derived, not measured (tests/test_eval_kernels_host.py: gemm_ref): for
y = alpha sum_k x_k w_k + b accumulated in f32 in any order, |y - y64| <= (K + 4) 2^-24 (|alpha| sum_k |x_k w_k| + |b|) per element,
y64 = numpy float64 on the same f32 inputs.  Every case prints one JSON line with its largest fraction of that bar, then asserts.
Selection and ranks compare exactly; staging forms, positions, repeats and padding compare bit for bit."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from conftest import load_case, split_prefix
from test_eval_kernels_host import (TRIPLES, bar_fraction, gemm_problem, gemm_ref, mrr_formula, recall_at_k_formula, ref_diag_rank,
                                    ref_topk_rows, special_rows)
from test_gpu_f32_parity import _misaligned
from test_gpu_parity import DEV, load_state, make_task, to_batch, tt  # noqa: F401  (tt: the module fixture)

from jodalrob_twotower_amd import _lib as L

pytestmark = pytest.mark.gpu

NAN_FILL = 0x7FC0BEEF          # a quiet-NaN bit pattern no kernel produces


def _report(tag, **kw):
    print(f"\n[{tag}]", json.dumps(kw))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _launches():
    return int(L.load().tt_launch_count())


def _nan_filled(rows, cols):
    return torch.full((rows, cols), NAN_FILL, dtype=torch.int32, device=DEV).view(torch.float32)


def _column_slice(x, lead, width):
    """x as the column slice wide[:, lead : lead + K] of a [M, width] tensor whose other columns hold NaN"""
    wide = _nan_filled(x.shape[0], width)
    v = wide[:, lead:lead + x.shape[1]]
    v.copy_(x)
    return v


# ---- A. tt_linear_fwd ---------------------------------------------------------------------------------------------------------------
def _linear_raw(X, ldx, W, bias, Y, ldy, M, N, K, relu=0):
    """the entry itself; X / W / bias / Y are tensors, integers (addresses that a refused call never reads) or None"""
    p = lambda t: L.ptr(t) if (t is None or torch.is_tensor(t)) else L.vp(t)
    return L.load().tt_linear_fwd(L.ctx(torch.device(DEV)), p(X), ldx, p(W), p(bias), p(Y), ldy, M, N, K, relu, L.stream(torch.device(DEV)))


@pytest.mark.parametrize("M,N,K", [t for t in TRIPLES if t[0] > 0])
def test_linear_fwd_against_f64_in_every_staging_form(tt, M, N, K):
    from jodalrob_twotower_amd import ops
    x, w, b = gemm_problem(2000 + 7 * M + 3 * N + K, M, N, K)
    X, W, Bv = _dev(x), _dev(w), _dev(b)
    wide4 = (K + 8 + 3) // 4 * 4
    forms = {"ldx": lambda: _column_slice(X, 4, wide4),               # 16-byte base, ldx % 4 == 0 > K: the vector form where K % 4 == 0
             "ldx_odd": lambda: _column_slice(X, 4, wide4 + 1),       # ldx = 4 j + 1: the scalar form through ldx
             "base": lambda: _column_slice(X, 1, wide4)}              # base one float past 16 bytes: the scalar form through the base
    worst, negative = 0.0, None
    for bias, relu in ((True, False), (True, True), (False, True), (False, False)):
        bt = Bv if bias else None
        y = ops.linear_fwd(X, W, bt, relu=relu)
        y64, bar = gemm_ref(x, w, b if bias else None, 1.0, relu)
        worst = max(worst, bar_fraction(y.cpu().numpy(), y64, bar))
        if not relu and bias:
            negative = float((y < 0).float().mean().item())
        for name, make in forms.items():
            assert _same_bits(ops.linear_fwd(make(), W, bt, relu=relu), y), (name, bias, relu)
        assert _same_bits(ops.linear_fwd(X, _misaligned(W), bt, relu=relu), y), ("w_base", bias, relu)
        assert _same_bits(ops.linear_fwd(X, W, bt, relu=relu), y), ("repeat", bias, relu)
        if (M, N) == (130, 200):                                       # an element depends on its own row of X, its own row of W and K only
            assert _same_bits(ops.linear_fwd(X[129:130], W, bt, relu=relu), y[129:130]), ("row 129", bias, relu)
            one = ops.linear_fwd(X, W[199:200].contiguous(), bt[199:200].contiguous() if bias else None, relu=relu)
            assert _same_bits(one, y[:, 199:200]), ("column 199", bias, relu)
    _report("linear_fwd", M=M, N=N, K=K, fraction=worst, negative_share=negative)
    assert worst <= 1.0
    if M * N >= 1000:
        assert 0.3 < negative < 0.7                                    # ReLU sees both signs


@pytest.mark.parametrize("M,N,K", [(1, 1, 1), (65, 33, 16), (63, 65, 130), (130, 200, 64)])
def test_linear_fwd_leaves_the_padding_of_y_alone(tt, M, N, K):
    from jodalrob_twotower_amd import ops
    x, w, b = gemm_problem(2100 + M, M, N, K)
    X, W, Bv = _dev(x), _dev(w), _dev(b)
    ldy = N + 3
    for relu in (0, 1):
        Y = _nan_filled(M + 2, ldy)
        assert _linear_raw(X, K, W, Bv, Y, ldy, M, N, K, relu) == 0
        assert _same_bits(Y[:M, :N], ops.linear_fwd(X, W, Bv, relu=bool(relu)))
        assert bool((_bits(Y[:, N:]) == NAN_FILL).all()) and bool((_bits(Y[M:]) == NAN_FILL).all())


def test_linear_fwd_empty_and_refusals_launch_nothing(tt):
    from jodalrob_twotower_amd import ops
    W, Bv = _dev(np.ones((33, 16), np.float32)), _dev(np.ones(33, np.float32))
    before = _launches()
    y = ops.linear_fwd(torch.empty((0, 16), dtype=torch.float32, device=DEV), W, Bv, relu=True)
    assert y.shape == (0, 33) and y.dtype == torch.float32
    odd = torch.empty_strided((0, 16), (0, 0), dtype=torch.float32, device=DEV)        # what an empty numpy array becomes: contiguous, strides 0
    assert odd.is_contiguous() and ops.linear_fwd(odd, W, None).shape == (0, 33)
    assert _linear_raw(None, 16, None, None, None, 33, 0, 33, 16) == 0                # M = 0 asks for no pointer
    X, Y = _dev(np.ones((4, 16), np.float32)), _nan_filled(4, 33)                     # (real buffers; a refused call reads none of them)
    refused = {"N=0": (X, 16, W, Bv, Y, 33, 4, 0, 16), "K=0": (X, 16, W, Bv, Y, 33, 4, 33, 0), "ldx<K": (X, 15, W, Bv, Y, 33, 4, 33, 16),
               "ldy<N": (X, 16, W, Bv, Y, 32, 4, 33, 16), "X=NULL": (None, 16, W, Bv, Y, 33, 4, 33, 16), "M<0": (X, 16, W, Bv, Y, 33, -1, 33, 16)}
    for name, args in refused.items():
        assert _linear_raw(*args) != 0, name
        assert L.load().tt_last_error_string().decode().startswith("tt_linear_fwd"), name
    assert _launches() == before and bool((_bits(Y) == NAN_FILL).all())


@pytest.mark.parametrize("M", [0, 1, 65])
@pytest.mark.parametrize("num_dim", [1, 3, 37])
def test_feature_projector_layer_by_layer(tt, M, num_dim):
    from jodalrob_twotower_amd import ops
    torch.manual_seed(300 + num_dim)
    proj = tt.FeatureProjector(num_dim, 768).to(DEV)
    rng = np.random.default_rng(310 + M + num_dim)
    dense = _dev(rng.standard_normal((M, num_dim)).astype(np.float32))
    text = {"title": _dev(rng.standard_normal((M, 768)).astype(np.float32)), "none": torch.empty((0, 768), dtype=torch.float32, device=DEV)}
    got_dense, got_text = proj(dense, text)
    assert list(got_text) == ["title", "none"] and got_text["none"].shape == (0, 128) and got_dense.shape == (M, 128)
    worst = [0.0, 0.0]
    for seq, x, got in ((proj.num_proj, dense, got_dense), (proj.text_proj, text["title"], got_text["title"])):
        w0, b0, w2, b2 = (p.detach() for p in (seq[0].weight, seq[0].bias, seq[2].weight, seq[2].bias))
        h = ops.linear_fwd(x, w0.contiguous(), b0, relu=True)                           # the forward's own first layer, bit for bit
        y64, bar = gemm_ref(x.cpu().numpy(), w0.cpu().numpy(), b0.cpu().numpy(), 1.0, True)
        worst[0] = max(worst[0], bar_fraction(h.cpu().numpy(), y64, bar))
        y64, bar = gemm_ref(h.cpu().numpy(), w2.cpu().numpy(), b2.cpu().numpy(), 1.0, False)    # fed the kernel's own first layer
        worst[1] = max(worst[1], bar_fraction(got.cpu().numpy(), y64, bar))
    _report("feature_projector", M=M, num_dim=num_dim, fraction_layer1=worst[0], fraction_layer2=worst[1])
    assert max(worst) <= 1.0
    assert proj(None, {})[0] is None


# ---- B. tt_score_matrix -------------------------------------------------------------------------------------------------------------
def _score_raw(A, Bm, Ra, Rb, D, inv_t, S, lds):
    dev = torch.device(DEV)
    return L.load().tt_score_matrix(L.ctx(dev), L.ptr(A), L.ptr(Bm), Ra, Rb, D, inv_t, L.ptr(S), lds, L.stream(dev))


@pytest.mark.parametrize("inv_t", [1.0, 20.0])
@pytest.mark.parametrize("Ra,Rb,D", [(1, 1, 1), (65, 33, 3), (33, 130, 17), (130, 65, 64), (63, 64, 200)])
def test_score_matrix_against_f64(tt, Ra, Rb, D, inv_t):
    from jodalrob_twotower_amd import ops
    a, b, _ = gemm_problem(400 + Ra + Rb + D, Ra, Rb, D)
    A, Bm = _dev(a), _dev(b)
    S = ops.score_matrix(A, Bm, inv_t)
    y64, bar = gemm_ref(a, b, None, inv_t, False)
    frac = bar_fraction(S.cpu().numpy(), y64, bar)
    _report("score_matrix", Ra=Ra, Rb=Rb, D=D, inv_t=inv_t, fraction=frac)
    assert frac <= 1.0
    assert _same_bits(ops.score_matrix(_misaligned(A), Bm, inv_t), S)                  # scalar staging form: the same values
    assert _same_bits(ops.score_matrix(A, _misaligned(Bm), inv_t), S)
    assert _same_bits(ops.score_matrix(_misaligned(A), _misaligned(Bm), inv_t), S)
    lds = Rb + 3                                                                       # padded rows of S: the padding keeps its fill
    Sp = _nan_filled(Ra + 1, lds)
    assert _score_raw(A, Bm, Ra, Rb, D, inv_t, Sp, lds) == 0
    assert _same_bits(Sp[:Ra, :Rb], S)
    assert bool((_bits(Sp[:, Rb:]) == NAN_FILL).all()) and bool((_bits(Sp[Ra:]) == NAN_FILL).all())


def test_score_matrix_empty_sides_and_refusals_launch_nothing(tt):
    from jodalrob_twotower_amd import ops
    A, Bm = _dev(np.ones((5, 8), np.float32)), _dev(np.ones((7, 8), np.float32))
    S = _nan_filled(5, 7)
    before = _launches()
    assert _score_raw(A, Bm, 0, 7, 8, 1.0, S, 7) == 0 and _score_raw(A, Bm, 5, 0, 8, 1.0, S, 7) == 0
    assert _score_raw(None, Bm, 0, 7, 8, 1.0, None, 7) == 0 and _score_raw(A, None, 5, 0, 8, 1.0, None, 0) == 0
    empty = torch.empty((0, 8), dtype=torch.float32, device=DEV)
    assert ops.score_matrix(empty, Bm, 1.0).shape == (0, 7) and ops.score_matrix(A, empty, 1.0).shape == (5, 0)
    assert bool((_bits(S) == NAN_FILL).all())
    for name, args in {"D=0": (A, Bm, 5, 7, 0, 1.0, S, 7), "lds<Rb": (A, Bm, 5, 7, 8, 1.0, S, 6), "A=NULL": (None, Bm, 5, 7, 8, 1.0, S, 7),
                       "S=NULL": (A, Bm, 5, 7, 8, 1.0, None, 7), "Ra<0": (A, Bm, -1, 7, 8, 1.0, S, 7)}.items():
        assert _score_raw(*args) != 0, name
    assert _launches() == before


# ---- C. _SimilarityFn (TwoTowerModel.compute_similarity) ------------------------------------------------------------------------------
def _unit_rows(rng, R, D):
    x = rng.standard_normal((R, D)).astype(np.float32)
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def _similarity_grads(n, c, inv_t, G, transposed=False, only=None):
    """(S, dN, dC) of loss = (S * G).sum() -- with `transposed`, (S.t() * G.t()).sum(): the same loss, dS arrives non-contiguous"""
    from jodalrob_twotower_amd.two_tower_model import _SimilarityFn
    tn = n.detach().clone().requires_grad_(only in (None, "n"))
    tc = c.detach().clone().requires_grad_(only in (None, "c"))
    S = _SimilarityFn.apply(tn, tc, inv_t)
    loss = (S.t() * G.t().contiguous()).sum() if transposed else (S * G).sum()
    loss.backward()
    return S.detach(), tn.grad, tc.grad


@pytest.mark.parametrize("T", [1.0, 0.05])
@pytest.mark.parametrize("Ra,Rb,D", [(1, 1, 1), (2, 2, 3), (65, 65, 33), (33, 130, 64), (130, 63, 129)])
def test_similarity_forward_and_backward_against_f64(tt, Ra, Rb, D, T):
    from jodalrob_twotower_amd import ops
    from jodalrob_twotower_amd.two_tower_model import _SimilarityFn
    rng = np.random.default_rng(500 + Ra + Rb + D)
    n, c = _unit_rows(rng, Ra, D), _unit_rows(rng, Rb, D)
    g = rng.standard_normal((Ra, Rb)).astype(np.float32)                               # non-symmetric upstream gradient
    N, Cm, G = _dev(n), _dev(c), _dev(g)
    inv_t = 1.0 / T
    S, dN, dC = _similarity_grads(N, Cm, inv_t, G)
    assert _same_bits(S, ops.score_matrix(N, Cm, inv_t))
    # dN = (G c) / T over K = Rb, dC = (G^T n) / T over K = Ra; one unit more for the separate * inv_t
    g64 = g.astype(np.float64)
    n64, c64 = (g64 @ c.astype(np.float64)) / T, (g64.T @ n.astype(np.float64)) / T
    bar_n, bar_c = gemm_ref(g, c.T, None, inv_t, False, extra=5)[1], gemm_ref(g.T, n.T, None, inv_t, False, extra=5)[1]
    fn, fc = bar_fraction(dN.cpu().numpy(), n64, bar_n), bar_fraction(dC.cpu().numpy(), c64, bar_c)
    _report("similarity_bwd", Ra=Ra, Rb=Rb, D=D, T=T, fraction_dN=fn, fraction_dC=fc)
    assert fn <= 1.0 and fc <= 1.0
    # a second identical call, and dS arriving non-contiguous: the same bits
    for kw in ({}, {"transposed": True}):
        S2, dN2, dC2 = _similarity_grads(N, Cm, inv_t, G, **kw)
        assert _same_bits(S2, S) and _same_bits(dN2, dN) and _same_bits(dC2, dC), kw
    # one side alone asks for a gradient: the other one is simply unused
    _, dN1, none_c = _similarity_grads(N, Cm, inv_t, G, only="n")
    _, none_n, dC1 = _similarity_grads(N, Cm, inv_t, G, only="c")
    assert none_c is None and none_n is None and _same_bits(dN1, dN) and _same_bits(dC1, dC)
    # a non-contiguous view and a bf16 input: made contiguous f32 by the node, gradients in the inputs' own shape and type
    base = N.t().contiguous().requires_grad_()                                         # [D, Ra]
    view = base.t()
    cb = Cm.bfloat16().requires_grad_()
    Sv = _SimilarityFn.apply(view, cb, inv_t)
    assert _same_bits(Sv, ops.score_matrix(N, cb.detach().float(), inv_t))
    gv, gb = torch.autograd.grad((Sv * G).sum(), [view, cb])
    _, dNb, dCb = _similarity_grads(N, cb.detach().float(), inv_t, G)
    assert gv.shape == view.shape and gv.dtype == torch.float32 and _same_bits(gv, dNb)
    assert gb.shape == cb.shape and gb.dtype == torch.bfloat16 and torch.equal(gb, dCb.bfloat16())
    if Ra > 1:
        assert not view.is_contiguous()


# ---- D. tt_topk_rows -----------------------------------------------------------------------------------------------------------------
def _topk_raw(S, R, Cc, lds, k, vals, idx):
    dev = torch.device(DEV)
    p = lambda t: L.ptr(t) if (t is None or torch.is_tensor(t)) else L.vp(t)
    return L.load().tt_topk_rows(L.ctx(dev), p(S), R, Cc, lds, k, p(vals), p(idx), L.stream(dev))


def _poisoned_view(s, extra=5):
    """s as wide[:, :C] of a matrix whose remaining columns hold +inf: nothing past C may reach a result"""
    wide = torch.full((s.shape[0], s.shape[1] + extra), float("inf"), dtype=torch.float32, device=DEV)
    v = wide[:, :s.shape[1]]
    v.copy_(_dev(s))
    return v


def _assert_topk(ops, s, k, tag):
    ev, ei = ref_topk_rows(s, k)
    for name, S in (("contiguous", _dev(s)), ("lds>C", _poisoned_view(s))):
        vals, idx = ops.topk_rows(S, k)
        assert np.array_equal(idx.cpu().numpy(), ei), (tag, name)
        assert np.array_equal(vals.cpu().numpy().view(np.int32), ev.view(np.int32)), (tag, name)    # bits: the selected element's own zero
    return vals, idx


@pytest.mark.parametrize("R,C,k", [(1, 1, 1), (3, 7, 7), (5, 63, 5), (4, 64, 64), (130, 65, 64), (7, 129, 63), (9, 1000, 1)])
def test_topk_rows_exact(tt, R, C, k):
    from jodalrob_twotower_amd import ops
    rng = np.random.default_rng(600 + R + C + k)
    s = rng.standard_normal((R, C)).astype(np.float32)
    vals, idx = _assert_topk(ops, s, k, "random")
    three = rng.choice(np.array([-1.5, 0.25, 2.0], np.float32), size=(R, C))          # heavy ties across the 64-lane stride
    three[R - 1] = np.float32(0.25)                                                   # one all-equal row: columns 0 .. k-1
    tv, ti = _assert_topk(ops, three, k, "three values")
    assert ti[R - 1].tolist() == list(range(k))
    # row r of the R-row call == the one-row call on that row
    for r in sorted({0, R // 2, R - 1}):
        v1, i1 = ops.topk_rows(_dev(s[r:r + 1]), k)
        assert _same_bits(v1, vals[r:r + 1]) and torch.equal(i1, idx[r:r + 1]), r
    _report("topk_rows", R=R, C=C, k=k, exact=True)


@pytest.mark.parametrize("k", [1, 4, 9])
def test_topk_rows_special_values(tt, k):
    from jodalrob_twotower_amd import ops
    s = special_rows()
    _, idx = _assert_topk(ops, s, k, "specials")
    if k == 9:
        assert idx[1].tolist() == [5, 0, 1, 2, 3, 6, 7, 4, 8]                          # +-0 are equal: the lower column first
        assert idx[2].tolist() == [3, 6, 5, 0, 1, 7, 2, 4, 8]                          # -inf selected with its own column
        assert idx[4].tolist() == [6, 1, 3, 8, 4, -1, -1, -1, -1]                      # NaN never; then (-inf, -1)
    # the same rows spread over more than one 64-lane stride, specials on both sides of it
    rng = np.random.default_rng(61)
    widev = rng.standard_normal((s.shape[0], 130)).astype(np.float32)
    widev[:, 60:69] = s
    widev[4, :] = np.nan
    widev[4, [3, 64, 129]] = [np.float32(-0.0), np.float32(0.0), -np.inf]
    _assert_topk(ops, widev, k, "specials across strides")


def test_topk_rows_empty_and_refusals_launch_nothing(tt):
    S = _dev(np.zeros((4, 70), np.float32))
    V = _nan_filled(4, 65)                                                             # (real buffers; a refused call touches none of them)
    I = torch.full((4, 65), 77, dtype=torch.int64, device=DEV)
    before = _launches()
    assert _topk_raw(None, 0, 70, 70, 5, None, None) == 0                              # R = 0
    for name, args in {"k=0": (S, 4, 70, 70, 0, V, I), "k=65": (S, 4, 70, 70, 65, V, I), "k>C": (S, 4, 3, 70, 4, V, I),
                       "lds<C": (S, 4, 70, 69, 5, V, I), "S=NULL": (None, 4, 70, 70, 5, V, I), "R<0": (S, -1, 70, 70, 5, V, I)}.items():
        assert _topk_raw(*args) != 0, name
        assert L.load().tt_last_error_string().decode().startswith("tt_topk_rows"), name
    assert _launches() == before and bool((_bits(V) == NAN_FILL).all()) and bool((I == 77).all())


def test_predict_batch_top_k_edges(tt, manifest):
    cfg = manifest["cases"]["tiny_eval"]
    g = load_case("tiny_eval")
    task = make_task(tt, cfg)
    load_state(task, split_prefix(g, "state."))
    batch = to_batch(tt, split_prefix(g, "in."), cfg["keys_n"], cfg["keys_c"])
    B = cfg["B"]
    task.predict_batch(batch, top_k=B)                                                 # (first call: one-off set-up launches)
    l0 = _launches()
    pr = task.predict_batch(batch, top_k=B)
    ok_launches = _launches() - l0
    sim = pr["all_similarities"].cpu().numpy()
    ev, ei = ref_topk_rows(sim, B)
    assert np.array_equal(pr["top_indices"].cpu().numpy(), ei)
    assert np.array_equal(pr["top_similarities"].cpu().numpy().view(np.int32), ev.view(np.int32))
    unique_max = (sim == sim.max(axis=1, keepdims=True)).sum(axis=1) == 1
    assert unique_max.any()
    assert np.array_equal(pr["top_indices"][:, 0].cpu().numpy()[unique_max], sim.argmax(axis=1)[unique_max])
    for bad in (B + 1, 65, 0):
        l0 = _launches()
        with pytest.raises(L.TwoTowerHipError, match="tt_topk_rows"):
            task.predict_batch(batch, top_k=bad)
        # the towers and the score matrix in front of it ran as before; the refused selection itself launched nothing
        assert _launches() - l0 == ok_launches - 1, bad


# ---- E. tt_diag_rank_rows and the evaluator on top of it ---------------------------------------------------------------------------------
def _rank_case(rng, R, C, off):
    """random rows with exact ties planted on both sides of every in-range positive"""
    s = rng.standard_normal((R, C)).astype(np.float32)
    for r in range(R):
        p = r + off
        if 0 <= p < C:
            for c in (p - 1, p + 1, p - 64, p + 64, 0, C - 1):
                if 0 <= c < C and (r + c) % 3:
                    s[r, c] = s[r, p]
    return s


@pytest.mark.parametrize("R,C,off", [(1, 1, 0), (5, 5, 0), (130, 130, 0), (33, 100, 40), (33, 100, 67), (33, 100, 90), (10, 40, -3),
                                     (70, 33, 0)])
def test_diag_rank_rows_exact(tt, R, C, off):
    from jodalrob_twotower_amd import ops
    s = _rank_case(np.random.default_rng(700 + R + C + off), R, C, off)
    want = ref_diag_rank(s, off)
    outside = int((want < 0).sum())
    assert outside == {(33, 100, 90): 23, (10, 40, -3): 3, (70, 33, 0): 37}.get((R, C, off), 0)
    for name, S in (("contiguous", _dev(s)), ("lds>C", _poisoned_view(s))):
        got = ops.diag_rank_rows(S, off).cpu().numpy()
        _report("diag_rank_rows", R=R, C=C, off=off, form=name, outside=outside, mismatches=int((got != want).sum()),
                rank_of_first_outside_row=(int(got[want < 0][0]) if outside else None))
        assert np.array_equal(got, want), name


def test_diag_rank_rows_empty_and_refusals_launch_nothing(tt):
    dev = torch.device(DEV)
    S = _dev(np.zeros((4, 8), np.float32))
    rank = torch.full((4,), 77, dtype=torch.int32, device=DEV)
    fn = L.load().tt_diag_rank_rows
    before = _launches()
    assert fn(L.ctx(dev), None, 0, 8, 8, 0, None, L.stream(dev)) == 0                  # R = 0
    assert fn(L.ctx(dev), L.ptr(S), 4, 8, 7, 0, L.ptr(rank), L.stream(dev)) != 0       # lds < C
    assert fn(L.ctx(dev), L.ptr(S), 4, 0, 8, 0, L.ptr(rank), L.stream(dev)) != 0       # C = 0
    assert fn(L.ctx(dev), None, 4, 8, 8, 0, L.ptr(rank), L.stream(dev)) != 0           # NULL S
    assert _launches() == before and rank.tolist() == [77] * 4


@pytest.mark.parametrize("R,C", [(70, 33), (33, 70)])
def test_evaluator_on_rectangular_matrices(tt, R, C):
    """[70, 33]: rows 33.. have no positive -- misses for Recall@K as in the reference's topk comparison, and no MRR at all;
    [33, 70]: every row has one, the reference's formulae as they are."""
    ev = tt.TwoTowerEvaluator(device=DEV)
    rng = np.random.default_rng(800 + R)
    s = rng.standard_normal((R, C)).astype(np.float32)
    d = np.arange(min(R, C))
    s[d[::2], d[::2]] += np.float32(2.0)                                               # a good share of hits among the rows that can hit
    S = _dev(s)
    for k in (1, 5, 10, 200):
        got = ev.compute_recall_at_k(S, k).item()
        want = recall_at_k_formula(s, k)
        _report("evaluator_recall", R=R, C=C, k=k, got=got, want=want)
        assert got == pytest.approx(want, abs=1e-7), k
    assert 0.0 < recall_at_k_formula(s, 5) <= min(R, C) / R
    if R > C:
        before = _launches()
        with pytest.raises(ValueError):
            ev.compute_mrr(S)
        with pytest.raises(ValueError):
            ev.compute_comprehensive_metrics(S, {"loss": 1.0})
        with pytest.raises(ValueError):
            mrr_formula(s)
        assert _launches() == before
    else:
        assert ev.compute_mrr(S).item() == pytest.approx(mrr_formula(s), rel=1e-6)
        m = ev.compute_comprehensive_metrics(S, {"loss": 1.0})
        assert m["recall@5"] == pytest.approx(recall_at_k_formula(s, 5), abs=1e-7)
        assert m["recall@10"] == pytest.approx(recall_at_k_formula(s, 10), abs=1e-7)
        assert m["mrr"] == pytest.approx(mrr_formula(s), rel=1e-6) and m["batch_size"] == R
