"""The Adam entries against f64 (oracle_np.adam_step, torch.optim.Adam's update with the optimiser's GLOBAL step count).

Per step: the f64 update is computed from the kernel's OWN previous p, m, v (and the f32 hyper-parameters the kernel sees), so
what is left is one update's rounding, measured in units of 2^-24 times the magnitude of the terms that form each result
(m: |b1 m| + |(1 - b1) g'|; v: b2 v + (1 - b2) g'^2; p: |p| + lr / bc1 * (|b1 m| + |(1 - b1) g'| + |m'|) / denom).  Over a 20-step trajectory the f64 run
is independent.  Host scalars and the device copy from ops.adam_hparams (what a captured graph reads) give the same bits, also
when the device scalars change between steps.  Routing-pad rows, untouched rows and their moments keep their bits; gradient rows
past U are NaN and must not leak.  The LONG blocks of tt_adam_fused_step_finish are fed by a real deferred reduction of exactly
summable rows (test_gpu_embed_grad_parity.Case): their completed gradient rows must equal the f64 sums bit for bit.
Bounds quote what an MI355X measured (in brackets; each bound <= 4x); DESIGN.md section 4 quotes them too.
"""
import json

import numpy as np
import pytest
import torch

import oracle_np as O
from test_gpu_embed_grad_parity import Case, _launches, _plan
from test_gpu_parity import DEV, tt  # noqa: F401  (tt: the module fixture)
from test_gpu_rowwise_adagrad import rowwise_adagrad_f64

pytestmark = pytest.mark.gpu

B1, B2, EPS, LR = 0.9, 0.999, 1e-8, 1e-2
ADAM_ULP_BOUNDS = {"p": 9.0, "m": 10.0, "v": 16.0}      # (p 2.3, m 2.6, v 4.0 over every entry, step and width)
TRAJ_BOUNDS = {"p_norm": 4.4e-7, "m_norm": 2.6e-7, "v_norm": 2.9e-7}   # (1.1e-7, 6.7e-8, 7.3e-8 after 20 steps, n = 50,000)
ADAGRAD_FINISH_BOUND = 6.5e-7  # (1.7e-7 w, 1.6e-7 s) max |w - w64| / (|w64| + |lr / (sqrt(s) + eps) * g'|) over the table
STEPS = (1, 2, 10, 10_000)


def _f32(x):
    return float(np.float32(x))


def _ref_step(p, g, m, v, step, wd):
    """f64 Adam from f32 state with the kernel's f32 hyper-parameters; returns (p, m, v, scales) in f64."""
    p, g, m, v = (np.asarray(a, np.float64).copy() for a in (p, g, m, v))
    b1, b2, lr, eps, wd = _f32(B1), _f32(B2), _f32(LR), _f32(EPS), _f32(wd)
    gp = g + wd * p if wd else g
    sm = np.abs(b1 * m) + np.abs((1 - b1) * gp)
    sv = b2 * v + (1 - b2) * gp * gp
    p0 = p.copy()
    O.adam_step(p, g, m, v, step, lr, b1, b2, eps, wd)
    # p: |p| plus the update's size with m replaced by the magnitude of its terms (a cancelling m carries their rounding)
    denom = np.sqrt(v) / np.sqrt(1 - b2 ** step) + eps
    return p, m, v, {"p": np.abs(p0) + lr / (1 - b1 ** step) * (sm + np.abs(m)) / denom, "m": sm, "v": sv}


def _ulps(got, want, scale):
    return float((np.abs(np.asarray(got, np.float64) - want) / (np.maximum(scale, 1e-30) * 2.0 ** -24)).max(initial=0.0))


def _hp(step, wd):
    from jodalrob_twotower_amd import ops
    return torch.tensor(ops.adam_hparams(step, LR, B1, B2, EPS, wd), dtype=torch.float32, device=DEV)


def _state(rng, shape):
    return (rng.standard_normal(shape).astype(np.float32), (0.1 * rng.standard_normal(shape)).astype(np.float32),
            (0.01 * np.abs(rng.standard_normal(shape))).astype(np.float32))


def _check(report, got, tag):
    for k, (a, b, s) in got.items():
        report[f"{tag}{k}"] = max(report.get(f"{tag}{k}", 0.0), _ulps(a, b, s))
    for k in got:
        assert report[f"{tag}{k}"] <= ADAM_ULP_BOUNDS[k], (tag, k, report)


@pytest.mark.parametrize("n,misaligned", [(3_000_004, False), (3_000_003, False), (100_000, True)])
@pytest.mark.parametrize("wd", [0.0, 1e-2])
def test_adam_dense_step_vs_f64(tt, n, misaligned, wd):
    """tt_adam_dense_step: vec4 past num_cus * 8 workgroups (grid-stride), scalar by n % 4 != 0 and by a misaligned base."""
    from jodalrob_twotower_amd import ops
    rng = np.random.default_rng(n + int(wd * 100))
    p0, m0, v0 = _state(rng, n)
    off = 1 if misaligned else 0

    def dev(a):
        buf = torch.empty(n + off, device=DEV)
        buf[off:] = torch.from_numpy(a)
        return buf[off:]
    a = [dev(x) for x in (p0, m0, v0)]
    b = [dev(x) for x in (p0, m0, v0)]
    report = {"n": n, "wd": wd}
    for step in STEPS:
        g = rng.standard_normal(n).astype(np.float32)
        tg = dev(g)
        before = [x.cpu().numpy() for x in a]
        ops.adam_dense(*a[:1], tg, *a[1:], step, LR, B1, B2, EPS, wd)
        ops.adam_dense(*b[:1], tg, *b[1:], step, LR, B1, B2, EPS, wd, hp_dev=_hp(step, wd))
        got = [x.cpu().numpy() for x in a]
        for x, y in zip(a, b):
            assert torch.equal(x, y), step                     # host scalars == device scalars, bitwise
        rp, rm, rv, sc = _ref_step(*before[:1], g, *before[1:], step, wd)
        _check(report, {"p": (got[0], rp, sc["p"]), "m": (got[1], rm, sc["m"]), "v": (got[2], rv, sc["v"])}, "")
    print("\n[adam dense per step]", json.dumps(report))


def test_adam_multi_two_launches_vs_f64(tt):
    """tt_adam_multi_step over 40 tensors (two launches of 32 + 8), empty ones among them, one past 64 workgroups (grid-stride);
    device scalars that change every step (a schedule) == host scalars, bitwise."""
    from jodalrob_twotower_amd import ops
    rng = np.random.default_rng(3)
    sizes = [0, 5, 70_001, 0, 3, 4096, 1] + [int(s) for s in rng.integers(0, 3000, 33)]
    st = [_state(rng, s) for s in sizes]
    A = [[torch.from_numpy(x.copy()).to(DEV) for x in t] for t in st]
    Bt = [[torch.from_numpy(x.copy()).to(DEV) for x in t] for t in st]
    report = {}
    for i, step in enumerate(STEPS):
        wd = (0.0, 1e-2)[i % 2]
        gs = [torch.from_numpy(rng.standard_normal(s).astype(np.float32)).to(DEV) for s in sizes]
        before = [[x.cpu().numpy() for x in t] for t in A]
        n = _launches(lambda: ops.adam_multi([(t[0], g, t[1], t[2]) for t, g in zip(A, gs)], step, LR, B1, B2, EPS, wd))
        assert n == 2
        ops.adam_multi([(t[0], g, t[1], t[2]) for t, g in zip(Bt, gs)], step, LR, B1, B2, EPS, wd, hp_dev=_hp(step, wd))
        for t, u, bf, g in zip(A, Bt, before, gs):
            for x, y in zip(t, u):
                assert torch.equal(x, y)
            rp, rm, rv, sc = _ref_step(bf[0], g.cpu().numpy(), bf[1], bf[2], step, wd)
            _check(report, {"p": (t[0].cpu().numpy(), rp, sc["p"]), "m": (t[1].cpu().numpy(), rm, sc["m"]),
                            "v": (t[2].cpu().numpy(), rv, sc["v"])}, "")
    print("\n[adam multi per step]", json.dumps(report))


def _sparse_plan(rng, R, U, pads, M):
    """unique_rows: U distinct rows of [0, R) and `pads` routing pads >= R, shuffled; n_unique = U + pads."""
    from jodalrob_twotower_amd import ops
    rows = np.concatenate([rng.choice(R, U, replace=False), R + np.arange(pads)])
    rows = rng.permutation(rows).astype(np.int32)
    ur = torch.full((M,), -7, dtype=torch.int32, device=DEV)
    ur[:len(rows)] = torch.from_numpy(rows)
    z = torch.zeros(1, dtype=torch.int32, device=DEV)
    return ops.DedupPlan(z, ur, z, torch.tensor([len(rows)], dtype=torch.int32, device=DEV), M), rows


@pytest.mark.parametrize("E", [1, 7, 32, 256, 1024])
@pytest.mark.parametrize("entry", ["sparse", "fused"])
def test_sparse_and_fused_adam_vs_f64(tt, E, entry):
    """tt_sparse_adam_step / tt_adam_fused_step (plus three tower tensors in the fused launch): looked-up rows against f64 per
    step, routing pads and untouched rows (and their moments) bit-unchanged, gradient rows past U (NaN) never read."""
    from jodalrob_twotower_amd import ops
    rng = np.random.default_rng(E + (entry == "fused"))
    R = max(64, 40_000 // E)
    U, pads = R // 3, 5
    M = U + pads + 17
    tab = [torch.from_numpy(x).to(DEV) for x in _state(rng, (R, E))]
    twin = [x.clone() for x in tab]
    dense_shapes = [(300, 40), (7,), (70_001,)]
    towers = [[torch.from_numpy(x).to(DEV) for x in _state(rng, s)] for s in dense_shapes]
    report = {"E": E, "entry": entry}
    for i, step in enumerate(STEPS):
        wd = (1e-2, 0.0)[i % 2]
        plan, rows = _sparse_plan(rng, R, U, pads, M)
        g = np.full((M, E), np.nan, np.float32)
        g[:U + pads] = rng.standard_normal((U + pads, E))
        tg = torch.from_numpy(g).to(DEV)
        before = [x.cpu().numpy() for x in tab]
        tb = [[x.cpu().numpy() for x in t] for t in towers]
        gt = [torch.from_numpy(rng.standard_normal(s).astype(np.float32)).to(DEV) for s in dense_shapes]
        if entry == "sparse":
            ops.adam_sparse(*tab, plan, tg, step, LR, B1, B2, EPS, wd)
            ops.adam_sparse(*twin, plan, tg, step, LR, B1, B2, EPS, wd, hp_dev=_hp(step, wd))
        else:
            items = [(t[0], gg, t[1], t[2]) for t, gg in zip(towers, gt)]
            ops.adam_fused(items, *tab, plan, tg, step, LR, B1, B2, EPS, wd)
            ops.adam_sparse(*twin, plan, tg, step, LR, B1, B2, EPS, wd, hp_dev=_hp(step, wd))
            for t, bf, gg in zip(towers, tb, gt):
                rp, rm, rv, sc = _ref_step(bf[0], gg.cpu().numpy(), bf[1], bf[2], step, wd)
                _check(report, {"p": (t[0].cpu().numpy(), rp, sc["p"]), "m": (t[1].cpu().numpy(), rm, sc["m"]),
                                "v": (t[2].cpu().numpy(), rv, sc["v"])}, "dense_")
        got = [x.cpu().numpy() for x in tab]
        for x, y in zip(tab, twin):
            assert torch.equal(x, y), step                     # fused == sparse entry; host == device scalars
        real = rows < R
        r = rows[real].astype(np.int64)
        rp, rm, rv, sc = _ref_step(before[0][r], g[:U + pads][real], before[1][r], before[2][r], step, wd)
        _check(report, {"p": (got[0][r], rp, sc["p"]), "m": (got[1][r], rm, sc["m"]), "v": (got[2][r], rv, sc["v"])}, "")
        untouched = np.ones(R, bool)
        untouched[r] = False
        for a, b in zip(got, before):
            assert np.array_equal(a[untouched].view(np.uint32), b[untouched].view(np.uint32))
            assert np.isfinite(a).all()
    print("\n[adam sparse/fused per step]", json.dumps(report))


def test_adam_trajectory_20_steps_vs_f64(tt):
    """20 steps of tt_adam_dense_step against an independent f64 trajectory (global step count, wd = 1e-2)."""
    from jodalrob_twotower_amd import ops
    rng = np.random.default_rng(20)
    n, wd = 50_000, 1e-2
    p0, m0, v0 = _state(rng, n)
    m0[:], v0[:] = 0, 0
    p, m, v = (torch.from_numpy(x.copy()).to(DEV) for x in (p0, m0, v0))
    rp, rm, rv = (x.astype(np.float64) for x in (p0, m0, v0))
    for step in range(1, 21):
        g = rng.standard_normal(n).astype(np.float32)
        ops.adam_dense(p, torch.from_numpy(g).to(DEV), m, v, step, LR, B1, B2, EPS, wd)
        O.adam_step(rp, g.astype(np.float64), rm, rv, step, _f32(LR), _f32(B1), _f32(B2), _f32(EPS), _f32(wd))
    rel = {k: float(np.linalg.norm(t.cpu().numpy() - r) / np.linalg.norm(r)) for k, t, r in (("p_norm", p, rp), ("m_norm", m, rm),
                                                                                            ("v_norm", v, rv))}
    rel["p_change_norm"] = float(np.linalg.norm(p.cpu().numpy() - rp) / np.linalg.norm(rp - p0))
    print("\n[adam trajectory]", json.dumps(rel))
    for k, b in TRAJ_BOUNDS.items():
        assert rel[k] <= b, (k, rel)


@pytest.mark.parametrize("E,km", [(32, False), (8, True), (7, False)])
def test_fused_finish_long_rows_vs_f64(tt, monkeypatch, E, km):
    """tt_adam_fused_step_finish on a real deferred reduction (keyed plan with E > 0, exact inputs): the LONG blocks' completed
    gradient rows equal the f64 sums bit for bit, and every touched row (long ones by the LONG blocks, the rest by the row blocks)
    follows f64 Adam with wd = 1e-2; the three tower tensors in the same launch as well."""
    from jodalrob_twotower_amd import ops
    c = Case(90 + E, 8192, [4, 2], E, "edge")
    plan = _plan(c, "keyed_long_km" if km else "keyed_long", monkeypatch)
    U = int(plan.n_unique.item())
    assert (c.counts > 64).sum() >= 4 and U == len(c.uniq)
    rng = np.random.default_rng(E)
    tab = [torch.from_numpy(x).to(DEV) for x in _state(rng, (c.table_rows, E))]
    towers = [[torch.from_numpy(x).to(DEV) for x in _state(rng, s)] for s in [(64, 33), (5,)]]
    gt = [torch.from_numpy(rng.standard_normal(t[0].shape).astype(np.float32)).to(DEV) for t in towers]
    before = [x.cpu().numpy() for x in tab]
    tb = [[x.cpu().numpy() for x in t] for t in towers]
    grad_rows = torch.full((c.M, E), float("nan"), device=DEV)
    step, wd = 3, 1e-2
    n = _launches(lambda: (ops.embed_grad(plan, c.srcs, c.B, E, ops.TT_GRAD_SPARSE, grad_rows, defer_finish=True),
                           ops.adam_fused([(t[0], g, t[1], t[2]) for t, g in zip(towers, gt)], *tab, plan, grad_rows, step, LR, B1,
                                          B2, EPS, wd)))
    assert n == 3 and plan.finish_deferred is None         # the deferred reduction (2 counted, see FORM_LAUNCHES) + the optimiser
    gr = grad_rows.cpu().numpy()
    assert np.array_equal(gr[:U].astype(np.float64), c.sums) and np.isnan(gr[U:]).all()
    got = [x.cpu().numpy() for x in tab]
    r = c.uniq.astype(np.int64)
    report = {"E": E, "long_rows": int((c.counts > 64).sum())}
    rp, rm, rv, sc = _ref_step(before[0][r], c.sums, before[1][r], before[2][r], step, wd)
    _check(report, {"p": (got[0][r], rp, sc["p"]), "m": (got[1][r], rm, sc["m"]), "v": (got[2][r], rv, sc["v"])}, "")
    for t, bf, g in zip(towers, tb, gt):
        rp, rm, rv, sc = _ref_step(bf[0], g.cpu().numpy(), bf[1], bf[2], step, wd)
        _check(report, {"p": (t[0].cpu().numpy(), rp, sc["p"]), "m": (t[1].cpu().numpy(), rm, sc["m"]),
                        "v": (t[2].cpu().numpy(), rv, sc["v"])}, "dense_")
    untouched = np.ones(c.table_rows, bool)
    untouched[r] = False
    for a, b in zip(got, before):
        assert np.array_equal(a[untouched].view(np.uint32), b[untouched].view(np.uint32))
    print("\n[adam fused finish]", json.dumps(report))


@pytest.mark.parametrize("E", [32, 7])
def test_rowwise_adagrad_fused_finish_vs_f64(tt, monkeypatch, E):
    """adam_rowwise_adagrad_fused in its deferred-finish form (long rows completed and updated inside the optimiser's launch)
    against the f64 restatement of row-wise Adagrad (test_gpu_rowwise_adagrad.rowwise_adagrad_f64) on exact gradient rows."""
    from jodalrob_twotower_amd import ops
    c = Case(95 + E, 8192, [3, 2], E, "edge")
    plan = _plan(c, "keyed_long", monkeypatch)
    U = int(plan.n_unique.item())
    rng = np.random.default_rng(50 + E)
    w0 = rng.standard_normal((c.table_rows, E)).astype(np.float32)
    s0 = np.abs(rng.standard_normal(c.table_rows)).astype(np.float32)
    table, acc = torch.from_numpy(w0).to(DEV), torch.from_numpy(s0).to(DEV)
    towers = [[torch.from_numpy(x).to(DEV) for x in _state(rng, (300,))]]
    g = torch.from_numpy(rng.standard_normal(300).astype(np.float32)).to(DEV)
    grad_rows = torch.full((c.M, E), float("nan"), device=DEV)
    t_lr, t_eps, t_wd = 0.05, 1e-7, 1e-2
    ops.embed_grad(plan, c.srcs, c.B, E, ops.TT_GRAD_SPARSE, grad_rows, defer_finish=True)
    ops.adam_rowwise_adagrad_fused([(towers[0][0], g, towers[0][1], towers[0][2])], 1, LR, B1, B2, EPS, 0.0, None, table, acc, plan,
                                   grad_rows, t_lr, t_eps, t_wd)
    assert plan.finish_deferred is None
    gr = grad_rows.cpu().numpy()
    assert np.array_equal(gr[:U].astype(np.float64), c.sums) and np.isnan(gr[U:]).all()
    r = c.uniq.astype(np.int64)
    w, s = w0[r].astype(np.float64), s0[r].astype(np.float64)
    gp = c.sums + _f32(t_wd) * w
    rowwise_adagrad_f64(w, c.sums, s, _f32(t_lr), _f32(t_eps), _f32(t_wd))
    got_w, got_s = table.cpu().numpy(), acc.cpu().numpy()
    step = np.abs(_f32(t_lr) / (np.sqrt(s) + _f32(t_eps)))[:, None] * np.abs(gp)
    rel_w = float((np.abs(got_w[r] - w) / (np.abs(w) + step)).max())
    rel_s = float((np.abs(got_s[r] - s) / s).max())
    print("\n[rowwise adagrad fused finish]", json.dumps({"E": E, "w": rel_w, "s": rel_s}))
    assert rel_w <= ADAGRAD_FINISH_BOUND and rel_s <= ADAGRAD_FINISH_BOUND
    untouched = np.ones(c.table_rows, bool)
    untouched[r] = False
    assert np.array_equal(got_w[untouched], w0[untouched]) and np.array_equal(got_s[untouched], s0[untouched])
