"""Host checks of the f64 references the embedding-gradient and table-Adam parity files stand on (no GPU): oracle_np.adam_step
and sparse_adam_rows against torch.optim.Adam in f64, and the exactly summable gradient grid (oracle_np.exact_grid_values)
whose sums must come out of any f32 summation order bit for bit."""
import numpy as np
import pytest
import torch

import oracle_np as O


@pytest.mark.parametrize("wd", [0.0, 1e-2])
def test_adam_step_matches_torch_adam_f64(wd):
    rng = np.random.default_rng(5)
    p0 = rng.standard_normal((7, 5))
    grads = [rng.standard_normal((7, 5)) for _ in range(6)]
    tp = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.Adam([tp], lr=3e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)
    p, m, v = p0.copy(), np.zeros_like(p0), np.zeros_like(p0)
    for t, g in enumerate(grads, start=1):
        tp.grad = torch.from_numpy(g.copy())
        opt.step()
        O.adam_step(p, g, m, v, t, 3e-3, 0.9, 0.999, 1e-8, wd)
        np.testing.assert_allclose(p, tp.detach().numpy(), rtol=1e-12, atol=1e-12)
        st = opt.state[tp]
        np.testing.assert_allclose(m, st["exp_avg"].numpy(), rtol=1e-12, atol=1e-15)
        np.testing.assert_allclose(v, st["exp_avg_sq"].numpy(), rtol=1e-12, atol=1e-15)


def test_sparse_adam_rows_uses_the_global_step():
    """Rows looked up in some steps only are corrected with the optimiser's step count, not their own."""
    rng = np.random.default_rng(6)
    R, E = 9, 4
    table, m, v = rng.standard_normal((R, E)), np.zeros((R, E)), np.zeros((R, E))
    ref = [table.copy(), m.copy(), v.copy()]
    for step, rows in ((1, [0, 3, 4]), (2, [3, 8]), (3, [0, 8, 5])):
        g = rng.standard_normal((len(rows), E))
        O.sparse_adam_rows(table, m, v, step, rows, g, 1e-2, wd=1e-2)
        for r, gr in zip(rows, g):
            O.adam_step(ref[0][r], gr, ref[1][r], ref[2][r], step, 1e-2, wd=1e-2)
        assert np.array_equal(table, ref[0]) and np.array_equal(m, ref[1]) and np.array_equal(v, ref[2])
    assert np.array_equal(table[[1, 2, 6, 7]], ref[0][[1, 2, 6, 7]]) and not m[[1, 2, 6, 7]].any()


def test_exact_grid_values_are_exact_in_bf16_and_any_f32_order():
    rng = np.random.default_rng(7)
    x = O.exact_grid_values(rng, (4096, 3))
    assert np.array_equal(x * 16, np.round(x * 16)) and np.abs(x).max() <= 3 / 16 and len(np.unique(x)) == 7
    assert torch.equal(torch.from_numpy(x).to(torch.bfloat16).float(), torch.from_numpy(x))
    # one long row at the bound's edge: 2^20 / (3/16) slots of |x| = 3/16 would reach 2^20; stay one slot below it
    n = int(O.EXACT_ABS_LIMIT / (3 / 16)) - 1
    vals = np.full((n, 1), 3 / 16, np.float32)
    vals[::2] *= -1
    vals[: n // 3] = np.float32(3 / 16)
    rows = np.zeros(n, np.int32)
    uniq, s, a, cnt = O.row_sums_f64(rows, vals)
    assert O.exact_sum_precondition(a) and cnt[0] == n
    for order in (np.arange(n), rng.permutation(n)):
        acc = np.cumsum(vals[order, 0], dtype=np.float32)[-1]                   # strictly sequential f32 adds
        assert float(acc) == float(s[0, 0])
        blocks = np.add.reduceat(vals[order, 0], np.arange(0, n, 64)).astype(np.float32)   # 64-slot chunk partials, then their sum
        assert float(np.cumsum(blocks, dtype=np.float32)[-1]) == float(s[0, 0])
    assert not O.exact_sum_precondition(a + 1.0)


def test_row_sums_f64_matches_add_at():
    rng = np.random.default_rng(8)
    rows = rng.integers(0, 50, 3000).astype(np.int32)
    vals = O.exact_grid_values(rng, (3000, 6))
    uniq, s, a, cnt = O.row_sums_f64(rows, vals)
    ref = np.zeros((50, 6))
    np.add.at(ref, rows, vals.astype(np.float64))
    refa = np.zeros((50, 6))
    np.add.at(refa, rows, np.abs(vals.astype(np.float64)))
    assert np.array_equal(uniq, np.unique(rows)) and np.array_equal(s, ref[uniq]) and np.array_equal(a, refa[uniq])
    assert np.array_equal(cnt, np.bincount(rows, minlength=50)[uniq])
