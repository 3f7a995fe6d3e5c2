"""tt_embed_grad_bwd and the duplicate-row plans it consumes against f64 at skewed row counts.

The core cases draw every gradient value from oracle_np.exact_grid_values (multiples of 2^-4, |x| <= 3/16) and keep every row's
sum of |x| below 2^20: every partial sum is then exact in f32 whatever the order and the chunking, so the kernel's rows must
equal the f64 reference BIT FOR BIT -- one dropped, doubled or misattributed slot, column, side or chunk boundary fails.  Each
case names its plan and its launch form (unplanned, short segments, planned, planned + deferred finish), and the form is
confirmed by the library's launch count.  A random-normal pass over some of the shapes checks the rounding: norm-wise against
f64, and element-wise inside the rigorous gamma_(n_row - 1) * sum|x| with gamma_k = k u / (1 - k u), u = 2^-24.

Invariants in every case: the distinct-row set is bit-exact, sparse rows >= U keep their NaN sentinel, untouched dense rows keep
their prior bits, and a second call gives the same bits.  test_second_reduction_over_one_planned_plan is the regression for the
planned long-row counters that the first reduction's finish used to zero (a second reduction over the same plan lost every row
of more than 64 slots).  The bound quotes what an MI355X measured; DESIGN.md section 4 quotes it too.
"""
import json

import numpy as np
import pytest
import torch

import oracle_np as O
from test_gpu_parity import DEV, tt  # noqa: F401  (tt: the module fixture)

from jodalrob_twotower_amd import _lib as _L
from jodalrob_twotower_amd import config as _cfg

pytestmark = pytest.mark.gpu

LONG = 64                     # kLongSeg: rows of more slots are summed in 64-slot chunks
EDGE_COUNTS = [1, 15, 16, 17, 63, 64, 65, 127, 128, 129]     # the kBatch = 16 trip and kLongSeg = 64 chunk boundaries
# random-normal pass, norm-wise |got - ref| / |ref| over all rows (the worst an MI355X measured over RANDN_CASES in brackets)
RANDN_NORM_BOUND = 1.6e-6      # (4.2e-7: 300,000 slots on one row; 1.6e-7 Zipf 1.05 planned; 4.9e-8 / 9.6e-8 edge rows)
# launches per form: unplanned = zeroing + row pass + chunk pass + finish; short = the row pass alone; planned = rows and chunks
# in one launch + finish; deferred = that launch, then tt_embed_grad_finish
# (tt_launch_count counts launch checks: tt_embed_grad_bwd's closing check counts once more in the short and deferred forms)
FORM_LAUNCHES = {"unplanned": 4, "short": 2, "planned": 2, "deferred": 3}


def _ids_for_key(rng, B, v, dist):
    """B ids in [0, v) for one key: "uniform", "edge" (rows of exactly EDGE_COUNTS slots while they fit, the rest in rows of
    1-3 slots), "one" (every slot on row 0) or a Zipf exponent."""
    if dist == "uniform":
        return rng.integers(0, v, B)
    if dist == "one":
        return np.zeros(B, np.int64)
    if dist == "edge":
        counts, left = [], B
        for n in EDGE_COUNTS:
            if n > left:
                break
            counts.append(n)
            left -= n
        while left > 0:
            counts.append(min(left, 1 + len(counts) % 3))
            left -= counts[-1]
        assert len(counts) <= v, (len(counts), v)
        return rng.permutation(np.repeat(np.arange(len(counts)), counts))
    return np.minimum(rng.zipf(float(dist), B) - 1, v - 1)


class Case:
    """Sides of K_i keys over B samples; slot = side_base + b * K_i + k; row = key offset + id (a key-partitioned row space, as
    the keyed plans need).  Gradient sources [B, ld_i] of which the first K_i * E columns are read."""

    def __init__(self, seed, B, Ks, E, dist, vocab=5000, src_dtype="f32", pad_ld=0, exact=True, ids=None, vocabs=None):
        rng = np.random.default_rng(seed)
        self.B, self.Ks, self.E = B, list(Ks), E
        rows, vals, self.srcs, off = [], [], [], 0
        for i, K in enumerate(Ks):
            vs = vocabs[i] if vocabs else [vocab] * K
            offs = off + np.concatenate([[0], np.cumsum(vs)[:-1]]).astype(np.int64)
            idk = ids[i] if ids is not None else np.stack([_ids_for_key(rng, B, v, dist) for v in vs], axis=1)
            rows.append((idk + offs[None, :]).reshape(-1))
            off += int(sum(vs))
            ld = K * E + pad_ld
            d = O.exact_grid_values(rng, (B, ld)) if exact else rng.standard_normal((B, ld)).astype(np.float32)
            td = torch.from_numpy(d).to(DEV)
            if src_dtype == "bf16":
                td = td.to(torch.bfloat16)
                d = td.float().cpu().numpy()
            self.srcs.append((td[:, :K * E], K))
            vals.append(d[:, :K * E].reshape(B * K, E))
        self.table_rows = off
        self.rows = np.concatenate(rows).astype(np.int32)
        self.vals = np.concatenate(vals)
        self.M = len(self.rows)
        self.uniq, self.sums, self.abs_sums, self.counts = O.row_sums_f64(self.rows, self.vals)
        self.rows_dev = torch.from_numpy(self.rows).to(DEV)

    def rows_key_major(self):
        parts, base = [], 0
        for K in self.Ks:
            parts.append(self.rows[base:base + self.B * K].reshape(self.B, K).T.reshape(-1))
            base += self.B * K
        return torch.from_numpy(np.ascontiguousarray(np.concatenate(parts))).to(DEV)


def _plan(c, kind, monkeypatch):
    from jodalrob_twotower_amd import ops
    if kind == "general":
        return ops.dedup_plan(c.rows_dev, c.table_rows)
    monkeypatch.setattr(_cfg.settings, "grad_planned", True)
    if kind == "keyed":
        return ops.dedup_plan_keyed(c.rows_dev, c.Ks, c.B)
    if kind == "keyed_long":
        return ops.dedup_plan_keyed(c.rows_dev, c.Ks, c.B, E=c.E)
    assert kind == "keyed_long_km", kind
    return ops.dedup_plan_keyed(c.rows_key_major(), c.Ks, c.B, key_major=True, E=c.E)


def _launches(fn):
    lib = _L.load()
    torch.cuda.synchronize()
    n0 = lib.tt_launch_count()
    fn()
    torch.cuda.synchronize()
    return int(lib.tt_launch_count() - n0)


def _run(c, plan, form, mode, out):
    """One reduction in launch form `form`; returns its launch count."""
    from jodalrob_twotower_amd import ops

    def go():
        if form == "deferred":
            ops.embed_grad(plan, c.srcs, c.B, c.E, mode, out, defer_finish=True)
            assert plan.finish_deferred is not None
            ops.embed_grad_finish(plan)
        else:
            ops.embed_grad(plan, c.srcs, c.B, c.E, mode, out, short_segments=form == "short")
    return _launches(go)


def _out(rows, E, misaligned, fill):
    """[rows, E] f32 on the device; misaligned: its base one float past a 16-byte boundary (the scalar path)"""
    buf = torch.full((rows * E + 1,), fill, device=DEV)
    out = (buf[1:] if misaligned else buf[:-1]).view(rows, E)
    assert out.data_ptr() % 16 == (4 if misaligned else 0)
    return out


def _check_case(c, plan, form, misaligned=False):
    """SPARSE, DENSE_SET and DENSE_ACC (onto a nonzero grid prior) on one plan, each bit for bit against f64 (exact inputs),
    with the invariants; returns a small report."""
    from jodalrob_twotower_amd import ops
    E = c.E
    U = int(plan.n_unique.item())
    uniq = plan.unique_rows[:U].cpu().numpy()
    assert U == len(c.uniq) and np.array_equal(uniq, c.uniq)
    assert np.array_equal(np.diff(plan.seg_offsets[:U + 1].cpu().numpy()), c.counts)
    assert O.exact_sum_precondition(c.abs_sums)
    rng = np.random.default_rng(U + E)
    sparse = None
    for mode in (["sparse"] if form == "deferred" else ["sparse", "set", "acc"]):
        if mode == "sparse":
            out = _out(c.M, E, misaligned, float("nan"))
            n = _run(c, plan, form, ops.TT_GRAD_SPARSE, out)
            g = out.cpu().numpy()
            assert np.isnan(g[U:]).all()
            got, want = g[:U], c.sums
            sparse = got
        else:
            prior = (O.exact_grid_values(rng, (c.table_rows, E)) if mode == "acc"
                     else rng.standard_normal((c.table_rows, E)).astype(np.float32))
            out = _out(c.table_rows, E, misaligned, 0.0)
            out.copy_(torch.from_numpy(prior))
            n = _run(c, plan, form, ops.TT_GRAD_DENSE_ACC if mode == "acc" else ops.TT_GRAD_DENSE_SET, out)
            g = out.cpu().numpy()
            untouched = np.ones(c.table_rows, bool)
            untouched[uniq] = False
            assert np.array_equal(g[untouched].view(np.uint32), prior[untouched].view(np.uint32))
            got, want = g[uniq], c.sums
            if mode == "acc":
                want = want + prior[uniq]
                assert O.exact_sum_precondition(c.abs_sums + np.abs(prior[uniq]))
        assert n == FORM_LAUNCHES[form], (form, mode, n)
        bad = got.astype(np.float64) != want
        assert not bad.any(), (form, mode, int(bad.any(1).sum()), "rows differ; counts", np.unique(c.counts[bad.any(1)])[:10])
    out = _out(c.M, E, misaligned, float("nan"))
    _run(c, plan, form, ops.TT_GRAD_SPARSE, out)
    assert np.array_equal(out[:U].cpu().numpy().view(np.uint32), sparse.view(np.uint32))
    return {"U": U, "long_rows": int((c.counts > LONG).sum()), "max_count": int(c.counts.max())}


# (id, seed, B, Ks, E, dist, plan, form, extra)
EXACT_CASES = [
    # widths: vec4 lane groups of 4 / 8 / 16 (E = 16 / 32 / 64), the generic group (E = 96, 256, 1024), scalar (E = 1, 3, 255)
    ("w1-general", 1, 8192, [2], 1, "edge", "general", "unplanned", {}),
    ("w3-general-bf16", 2, 2000, [3, 1], 3, "edge", "general", "unplanned", {"src_dtype": "bf16"}),
    ("w4-keyed", 3, 8192, [2, 1], 4, "edge", "keyed", "unplanned", {}),
    ("w8-keyed-long", 4, 8192, [3, 1, 2, 1], 8, "edge", "keyed_long", "planned", {}),
    ("w16-keyed-long-km", 5, 4097, [2, 2], 16, "edge", "keyed_long_km", "planned", {}),
    ("w32-keyed-long-deferred", 6, 8192, [4, 1], 32, "edge", "keyed_long", "deferred", {}),
    ("w64-keyed-long-bf16", 7, 2048, [2, 1], 64, "edge", "keyed_long", "planned", {"src_dtype": "bf16"}),
    ("w96-general-short", 8, 1000, [2, 1], 96, "edge", "general", "short", {}),
    ("w255-general", 9, 700, [1, 2], 255, "edge", "general", "unplanned", {}),
    ("w256-keyed-long-deferred", 10, 1500, [2], 256, "edge", "keyed_long", "deferred", {}),
    ("w1024-general", 11, 300, [1, 1], 1024, "edge", "general", "unplanned", {}),
    ("w1024-keyed-long", 12, 300, [1, 1], 1024, "edge", "keyed_long", "planned", {}),
    # the scalar path at widths that are otherwise vec4: a misaligned out, a source with ld % 4 != 0
    ("w32-misaligned-out", 13, 4096, [2, 1], 32, "edge", "keyed_long", "planned", {"misaligned": True}),
    ("w1024-misaligned-general", 14, 200, [1], 1024, "edge", "general", "unplanned", {"misaligned": True}),
    ("w16-ld-odd", 15, 4096, [2, 3], 16, "edge", "general", "unplanned", {"pad_ld": 1}),
    ("w8-ld-odd-bf16-planned", 16, 4096, [1, 2], 8, "edge", "keyed_long", "planned", {"pad_ld": 3, "src_dtype": "bf16"}),
    # the planned launch with no slab items on the scalar path: two rows of ~65 slots per key (either side of kLongSeg in one
    # plan; counts 62 / 68 / 70 / 60 and 66 / 64 / 76 / 54), fewer chunk workgroups than kChunkFirst
    ("w3-keyed-long-vocab2", 33, 130, [1, 1], 3, "uniform", "keyed_long", "planned", {"vocab": 2}),
    ("w3-keyed-long-vocab2-bf16", 34, 130, [1, 1], 3, "uniform", "keyed_long", "planned", {"vocab": 2, "src_dtype": "bf16"}),
    # sides: up to four of unequal K with K = 1 (the magic = 2^32 - 1 fix-up) and padded rows; batches at the edges
    ("sides4-B1", 17, 1, [3, 1, 5, 2], 8, "uniform", "keyed_long", "planned", {"pad_ld": 4}),
    ("sides4-B63", 18, 63, [1, 4, 1, 2], 4, "uniform", "keyed", "unplanned", {"pad_ld": 4}),
    ("sides4-B64", 19, 64, [2, 1, 3, 1], 12, "1.2", "general", "unplanned", {"pad_ld": 8}),
    ("sides4-B65", 20, 65, [1, 1, 1, 1], 32, "uniform", "keyed_long_km", "planned", {"pad_ld": 4}),
    ("sides4-B8192", 21, 8192, [5, 1, 2, 1], 8, "1.05", "keyed_long", "deferred", {"pad_ld": 4}),
    ("sides2-B8193", 22, 8193, [3, 1], 16, "1.2", "general", "unplanned", {"pad_ld": 4}),
    ("sides3-B65536-short", 23, 65536, [1, 2, 1], 4, "2.0", "general", "short", {}),
    ("sides1-K1-B65536", 24, 65536, [1], 8, "1.05", "general", "unplanned", {"pad_ld": 8}),
    # skew: Zipf 1.05 / 1.2 / 2.0 through the keyed plans' forms
    ("zipf1.05-keyed-long", 25, 8192, [6, 2], 32, "1.05", "keyed_long", "planned", {}),
    ("zipf1.2-keyed-long-km-deferred", 26, 8192, [4], 16, "1.2", "keyed_long_km", "deferred", {}),
    ("zipf2.0-keyed-short", 27, 8192, [3, 1], 32, "2.0", "keyed", "short", {}),
    ("zipf2.0-general-bf16", 28, 20000, [2], 8, "2.0", "general", "unplanned", {"src_dtype": "bf16"}),
    # ~2,400 rows of ~109 slots: more long rows than the finish has workgroups (num_cus * 8), so each of them loops
    ("many-long-rows-B65536", 29, 65536, [4], 8, "uniform", "general", "unplanned", {"vocab": 600}),
    ("many-long-rows-B8192-planned", 32, 8192, [40], 4, "uniform", "keyed_long", "planned", {"vocab": 80}),
]


@pytest.mark.parametrize("seed,B,Ks,E,dist,plan_kind,form,extra", [c[1:] for c in EXACT_CASES], ids=[c[0] for c in EXACT_CASES])
def test_exact_inputs_bit_exact(tt, monkeypatch, seed, B, Ks, E, dist, plan_kind, form, extra):
    extra = dict(extra)
    misaligned = extra.pop("misaligned", False)
    c = Case(seed, B, Ks, E, dist, **extra)
    plan = _plan(c, plan_kind, monkeypatch)
    assert (plan.grad_ws is not None) == plan_kind.startswith("keyed_long")
    rep = _check_case(c, plan, form, misaligned)
    print("\n[embed_grad exact]", json.dumps({"B": B, "Ks": Ks, "E": E, "form": form, **rep}))


def test_one_row_holds_every_slot(tt, monkeypatch):
    """M = 2.5 M slots on one row: ~39k chunk partials added by one finish workgroup (E = 4: the vec4 lane group of 4)."""
    c = Case(30, 2_500_000, [1], 4, "one", vocab=3)
    assert c.counts.tolist() == [2_500_000]
    rep = _check_case(c, _plan(c, "general", monkeypatch), "unplanned")
    print("\n[embed_grad exact one row]", json.dumps(rep))


def _real_ids(schema_real, B, seed):
    from jodalrob_twotower_amd import synthetic
    kn, kc = schema_real["notice"]["categorical"], schema_real["company"]["categorical"]
    vn, vc = schema_real["notice"]["vocab_sizes"], schema_real["company"]["vocab_sizes"]
    b = synthetic.make_batch(B, vn, vc, kn, kc, 4, 4, torch.device(DEV), seed=seed)
    ids = [b["notice"]["kjt"].values().cpu().numpy().reshape(B, len(kn)), b["company"]["kjt"].values().cpu().numpy().reshape(B, len(kc))]
    return ids, [list(vn), list(vc)]


@pytest.mark.parametrize("B,plan_kind,form", [(65536, "general", "unplanned"), (8192, "keyed_long", "planned"),
                                               (8192, "keyed_long_km", "deferred")])
def test_real_schema_ids(tt, monkeypatch, schema_real, B, plan_kind, form):
    """The real 32 + 6 key schema's ids from synthetic.make_batch.  B = 65536 is configs[4]'s distribution (2.5 M slots, the
    general radix plan; ~1,500 rows of more than 64 slots, the largest ~5,600)."""
    ids, vocabs = _real_ids(schema_real, B, seed=17)
    c = Case(31 + B, B, [len(v) for v in vocabs], 8, None, ids=ids, vocabs=vocabs)
    rep = _check_case(c, _plan(c, plan_kind, monkeypatch), form)
    if B == 65536:
        assert rep["long_rows"] > 1000 and rep["max_count"] > 4096, rep
    print(f"\n[embed_grad exact real B={B}]", json.dumps(rep))


def test_dedup_plan_runs_with_routing_pads(tt):
    """dedup_plan_runs with row_limit: ids >= row_limit (routing pads) are grouped last and left out of n_unique; the reduction
    never writes them (sparse rows >= U keep NaN, the dense pad rows stay zero) and the rows below are exact."""
    from jodalrob_twotower_amd import ops
    rng = np.random.default_rng(40)
    G, C, R, E = 8, 3000, 1000, 16
    runs = [np.sort(np.where(rng.random(C) < 0.05, R, np.minimum(rng.zipf(1.3, C) - 1, R - 1))) for _ in range(G)]   # one pad value
    rows = np.concatenate(runs).astype(np.int32)
    d = O.exact_grid_values(rng, (G * C, E))
    src = torch.from_numpy(d).to(DEV)
    plan = ops.dedup_plan_runs(torch.from_numpy(rows).to(DEV), G, C, row_limit=R)
    U = int(plan.n_unique.item())
    uniq, sums, _, counts = O.row_sums_f64(rows, d)
    keep = uniq < R
    assert U == int(keep.sum()) and np.array_equal(plan.unique_rows[:U].cpu().numpy(), uniq[keep])
    assert (counts[keep] > LONG).sum() >= 3
    out = torch.full((G * C, E), float("nan"), device=DEV)
    assert _launches(lambda: ops.embed_grad(plan, [(src, 1)], G * C, E, ops.TT_GRAD_SPARSE, out)) == FORM_LAUNCHES["unplanned"]
    g = out.cpu().numpy()
    assert np.array_equal(g[:U].astype(np.float64), sums[keep]) and np.isnan(g[U:]).all()
    dense = torch.zeros((R + 1, E), device=DEV)
    ops.embed_grad(plan, [(src, 1)], G * C, E, ops.TT_GRAD_DENSE_SET, dense)
    gd = dense.cpu().numpy()
    assert np.array_equal(gd[uniq[keep]].astype(np.float64), sums[keep]) and not gd[R:].any()


RANDN_CASES = [("keyed-long-zipf1.05", 50, 8192, [6, 2], 32, "1.05", "keyed_long", "planned"),
               ("general-one-row", 51, 300_000, [1], 4, "one", "general", "unplanned"),
               ("general-edge-scalar", 52, 8192, [2, 1], 3, "edge", "general", "unplanned"),
               ("keyed-long-deferred-w256", 53, 1500, [2], 256, "edge", "keyed_long", "deferred")]


@pytest.mark.parametrize("seed,B,Ks,E,dist,plan_kind,form", [c[1:] for c in RANDN_CASES], ids=[c[0] for c in RANDN_CASES])
def test_random_normal_rounding(tt, monkeypatch, seed, B, Ks, E, dist, plan_kind, form):
    from jodalrob_twotower_amd import ops
    c = Case(seed, B, Ks, E, dist, exact=False)
    plan = _plan(c, plan_kind, monkeypatch)
    U = int(plan.n_unique.item())
    assert U == len(c.uniq)
    out = torch.full((c.M, E), float("nan"), device=DEV)
    _run(c, plan, form, ops.TT_GRAD_SPARSE, out)
    err = np.abs(out[:U].cpu().numpy().astype(np.float64) - c.sums)
    ku = np.maximum(c.counts - 1, 0)[:, None] * 2.0 ** -24
    rigorous = ku / (1 - ku) * c.abs_sums
    norm = float(np.linalg.norm(err) / np.linalg.norm(c.sums))
    rep = {"norm": norm, "worst_over_rigorous": float((err / np.maximum(rigorous, 1e-300)).max()), "max_count": int(c.counts.max())}
    print(f"\n[embed_grad randn B={B} E={E} {form}]", json.dumps(rep))
    assert (err <= rigorous).all(), rep
    assert norm <= RANDN_NORM_BOUND, rep


def test_e_too_wide_refused_before_any_launch(tt):
    """E = 1025 is past the long-row finish's LDS: TT_ERR_UNSUPPORTED, and not one launch first (not even the zeroing)."""
    from jodalrob_twotower_amd import ops
    c = Case(60, 64, [2], 1025, "uniform", vocab=10)
    plan = ops.dedup_plan(c.rows_dev, c.table_rows)
    out = torch.empty((c.M, 1025), device=DEV)
    torch.cuda.synchronize()
    lib = _L.load()
    n0 = lib.tt_launch_count()
    with pytest.raises(_L.TwoTowerHipError, match=r"status -4\).*too wide"):
        ops.embed_grad(plan, c.srcs, c.B, 1025, ops.TT_GRAD_SPARSE, out)
    assert lib.tt_launch_count() == n0


@pytest.mark.parametrize("km", [False, True])
def test_second_reduction_over_one_planned_plan(tt, monkeypatch, km):
    """Regression: a keyed plan built with E > 0 keeps the long-row list and its counters in its gradient workspace.  The first
    reduction's finish used to zero those counters, so a second reduction over the same plan (several backward passes over one
    forward: TT_GRAD_DENSE_SET, then TT_GRAD_DENSE_ACC) silently skipped every row of more than 64 slots."""
    from jodalrob_twotower_amd import ops
    c = Case(70 + km, 8192, [4, 2], 32, "edge", exact=False)
    plan = _plan(c, "keyed_long_km" if km else "keyed_long", monkeypatch)
    assert plan.grad_ws is not None
    U = int(plan.n_unique.item())
    n_long = int((c.counts > LONG).sum())
    assert n_long >= 4
    first = torch.full((c.M, c.E), float("nan"), device=DEV)
    second = torch.full((c.M, c.E), float("nan"), device=DEV)
    ops.embed_grad(plan, c.srcs, c.B, c.E, ops.TT_GRAD_SPARSE, first)
    ops.embed_grad(plan, c.srcs, c.B, c.E, ops.TT_GRAD_SPARSE, second)
    a, b = first[:U].cpu().numpy(), second[:U].cpu().numpy()
    assert np.isfinite(a).all()
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"{int((a != b).any(1).sum())} of {n_long} long rows differ"
    for _ in range(2):                                       # the deferred form and its finish, twice over the same plan
        third = torch.full((c.M, c.E), float("nan"), device=DEV)
        ops.embed_grad(plan, c.srcs, c.B, c.E, ops.TT_GRAD_SPARSE, third, defer_finish=True)
        ops.embed_grad_finish(plan)
        assert np.array_equal(third[:U].cpu().numpy().view(np.uint32), a.view(np.uint32))
    dense = torch.zeros((c.table_rows, c.E), device=DEV)
    ops.embed_grad(plan, c.srcs, c.B, c.E, ops.TT_GRAD_DENSE_SET, dense)
    once = dense.clone()
    ops.embed_grad(plan, c.srcs, c.B, c.E, ops.TT_GRAD_DENSE_ACC, dense)
    assert np.array_equal(once.cpu().numpy()[plan.unique_rows[:U].cpu().numpy()], a)
    twice = (dense != 2 * once).any(1)
    assert not bool(twice.any()), f"{int(twice.sum())} rows are not twice the first pass ({n_long} long rows)"
