"""CPU side of tests/test_gpu_score_bf16_forms.py: the directional oracle against the square one, the case table against the
dispatch it has to reach, and the per-element bar shown able to pass (an f32 + bf16 emulation of the kernels' arithmetic stays
inside it at every shape) and able to fail (two planted errors leave it at every shape)."""
import numpy as np
import pytest

import oracle_np as O
import _score_forms as F


@pytest.fixture(scope="module")
def problems():
    return {g: F.make_problem(g) for g in F.GROUPS}


@pytest.mark.parametrize("B,D,T", [(1, 3, 1.0), (33, 8, 0.5), (70, 64, 0.07), (129, 200, 2.0)])
def test_score_dir_terms_equals_square_oracle(B, D, T):
    rng = np.random.default_rng(B + D)
    n = rng.standard_normal((B, D))
    c = 0.5 * n + rng.standard_normal((B, D))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    loss, met, S, lse = O.score_ce_fwd(n, c, T)
    dN, dC = O.score_ce_bwd(n, c, S, lse, T)
    shift = 1.0 / T
    rs, cs = np.exp(lse[0] - shift), np.exp(lse[1] - shift)
    k = 1.0 / (2 * B * T)
    W, mag = O.score_dir_terms(n, c, T, 0, rs, cs)
    np.testing.assert_allclose(k * (W @ c), dN, rtol=1e-14, atol=1e-14 * np.abs(dN).max())
    W1, mag1 = O.score_dir_terms(c, n, T, 0, cs, rs)
    np.testing.assert_allclose(k * (W1 @ n), dC, rtol=1e-14, atol=1e-14 * np.abs(dC).max())
    np.testing.assert_allclose(W1, W.T, rtol=1e-14, atol=1e-14)
    idx = np.arange(B)
    np.testing.assert_allclose(mag[idx, idx], np.abs(W[idx, idx] + 2) + 2, rtol=1e-14)   # the positive, counted by magnitude
    off_diag = ~np.eye(B, dtype=bool)
    assert np.array_equal(mag[off_diag], np.abs(W[off_diag]))
    # a window of the same problem: rows 5 .. of a rectangular direction are the square problem's rows
    if B > 8:
        Wr, _ = O.score_dir_terms(n[5:9], c, T, 5, rs[5:9], cs)
        np.testing.assert_allclose(Wr, W[5:9], rtol=1e-14, atol=1e-14)


def test_case_table_reaches_every_form():
    """every backward kernel of bwd_bf16() in both unit forms, with and without reciprocals, and every forward tile in both unit
    forms, each by a square and by a rectangular group; every shape, D and T of the plan appears"""
    bwd, fwd = {}, {}
    for g in F.GROUPS:
        kind = "square" if g.Ra == g.Rb and g.off == 0 else "rect"
        fwd.setdefault(F.fwd_kernel(g.D, g.unit), set()).add(kind)
        for rows_min, inv in F.bwd_variants(g):
            bwd.setdefault(F.bwd_kernel(g.D, g.Ra, rows_min, g.unit) + (inv,), set()).add(kind)
    names = set(F.BWD_SMALL.values()) | set(F.BWD_ROWS.values())
    assert len(names) == 7
    assert set(bwd) == {(k, u, i) for k in names for u in (True, False) for i in (True, False)}
    assert set(fwd) == {(k, u) for k in F.FWD_KERNELS.values() for u in (True, False)}
    assert all(v == {"square", "rect"} for v in bwd.values()), bwd
    assert all(v == {"square", "rect"} for v in fwd.values()), fwd
    assert {g.Rb for g in F.GROUPS if g.Ra == g.Rb} >= {1, 31, 32, 33, 63, 64, 65, 127, 129, 257, 300}
    assert {g.D for g in F.GROUPS} == {1, 8, 32, 33, 64, 65, 128, 129, 200, 256}
    assert {g.T for g in F.GROUPS} == {1.0, 0.5, 2.0, 0.07, 0.025}
    assert {(g.Ra, g.Rb, g.off) for g in F.GROUPS if g.Ra != g.Rb} == set(F.RECT_SHAPES)
    # the rows forms' workgroups (256 rows; 128 at padded D = 256) with Ra either side
    for Dp, edge in ((64, (255, 300)), (128, (255, 257)), (256, (127, 129))):
        assert set(edge) <= {g.Ra for g in F.GROUPS if F.padded_d(g.D) == Dp}, Dp
    # with the default threshold none of these shapes takes the rows form: the tests have to force it
    assert all(F.bwd_kernel(g.D, g.Ra, F.ROWS_MIN_DEFAULT, g.unit)[0] in F.BWD_SMALL.values() for g in F.GROUPS)
    # fewer b tiles than the b-split's waves
    assert any((g.Rb + 31) // 32 < F.BWD_WAVES[F.bwd_kernel(g.D, g.Ra, F.ROWS_NEVER, g.unit)[0]] for g in F.GROUPS if g.Ra != g.Rb)


def test_planted_operands(problems):
    for g, p in problems.items():
        for x in (p.n, p.c):
            np.testing.assert_allclose(np.linalg.norm(x.astype(np.float64), axis=1), 1.0, atol=1e-6)
        if g.Rb >= 8:
            assert len(p.edges) == len({g.Rb - 1, g.Rb - 2, 32 * ((g.Rb - 1) // 32)}), g
        for direction, (a, pos, copies) in p.ties.items():
            M = p.c if direction == 0 else p.n
            assert pos == a + g.off and pos not in p.edges and not set(copies) & set(p.edges)
            assert all(np.array_equal(M[j], M[pos]) for j in copies)
        if g.Ra >= 8:
            assert all(len(p.ties[d][2]) >= 1 for d in (0, 1)), g
        if g.Ra >= 127:                                                # a copy before, one after, one inside the positive's tile
            a, pos, copies = p.ties[0]
            assert any(j < pos and j // 32 != pos // 32 for j in copies) and any(j > pos and j // 32 != pos // 32 for j in copies)
            assert any(j // 32 == pos // 32 for j in copies)


def test_emulation_inside_the_bar_and_planted_errors_outside(problems):
    """The bar (_score_forms.rho times the magnitude sum) against the emulated kernel arithmetic: inside it as computed, outside it
    with the last b row masked away and with the positive's -2 one column off -- at every group's shape."""
    worst = 0.0
    for g, p in problems.items():
        f = F.emulation_fraction(p)
        assert f <= 1.0, (g, f)
        worst = max(worst, f)
        f_drop = F.emulation_fraction(p, "drop_last")
        assert f_drop > 1.0, (g, f_drop)
        f_shift = F.emulation_fraction(p, "shift_pos")
        assert f_shift > 1.0, (g, f_shift)
    print(f"emulation: largest fraction of the bar {worst:.3f}")
