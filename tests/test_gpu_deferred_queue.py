"""The queue discipline of the step's queued launches (csrc/tt_deferred.h) on the bare entries, for the slots that
test_gpu_score_tail_fused.py::test_queued_score_backward_runs_exactly_once does not cover: the keyed plan's sort and compaction, the
symmetric score forward's loss reduction, what a second queueing call displaces, and one whole eager step under every combination
of the three options.  Launches are counted with tt_launch_count(), results compared with torch.equal against the same call with
the option off.

Shapes.  Plan: two sides of 3 and 2 keys, B = 200 (a ragged last 64-row tile), one row of the first key drawn 101 times (more than
kPlanLongSeg = 64: the compaction builds the long-row list, E = 32), TT_OPT_KEYED_PARTS 1 and 2.  Score forward: B = 192, D = 64.
Whole step: B = 192, dropout 0.1, towers [128, 64] -> 64 (the fused narrow tail hosts everything) and [512, 256] -> 128 (it hosts
nothing: every queued slot leaves through a flush).

The stream rule (a slot runs stand-alone on the stream it was queued on and is hosted only by a call on that stream) cannot be made
to fail from here without racing on purpose; it is checked by reading tt_deferred_flush and tt_deferred_host."""
import numpy as np
import pytest
import torch

from _eager_step import DEV, _batch, _compare, _one_step
from jodalrob_twotower_amd import config as _cfg

pytestmark = pytest.mark.gpu

KS, B_PLAN, E = [3, 2], 200, 32
B_SYM, D_SYM, INV_T = 192, 64, 20.0


@pytest.fixture(scope="module")
def tt():
    import jodalrob_twotower_amd as m
    from jodalrob_twotower_amd import _lib
    _lib.load()
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return m


@pytest.fixture()
def L(tt, monkeypatch):
    """the library module, the plan's long-row list on, and every queueing option off again afterwards"""
    from jodalrob_twotower_amd import _lib
    monkeypatch.setattr(_cfg.settings, "grad_planned", True)
    dev = torch.device(DEV)
    assert _lib.load().tt_deferred_pending(_lib.ctx(dev)) == 0
    yield _lib
    _lib.set_defer_riders(dev, False)
    _lib.set_option(dev, _lib.TT_OPT_KEYED_PARTS, 0)


def _rows(seed):
    """slot rows [side][sample][key] of the two sides; key 0 of side 0 repeats one row 101 times"""
    rng = np.random.default_rng(seed)
    sides, off = [], 0
    for K in KS:
        v = rng.choice([7, 40, 300, 70000], size=K)
        offs = off + np.concatenate([[0], np.cumsum(v)[:-1]])
        ids = np.stack([rng.integers(0, vk, B_PLAN) for vk in v], axis=1)
        if off == 0:
            ids[rng.permutation(B_PLAN)[:101], 0] = 3
        sides.append((ids + offs[None, :]).reshape(-1))
        off += int(v.sum())
    return torch.from_numpy(np.concatenate(sides).astype(np.int32)).to(DEV)


def _plan_out(plan):
    U = int(plan.n_unique.item())
    return {"n_unique": plan.n_unique.cpu().clone(), "unique_rows": plan.unique_rows[:U].cpu().clone(),
            "seg_offsets": plan.seg_offsets[:U + 1].cpu().clone(), "sorted_src": plan.sorted_src.cpu().clone()}


def _same(ref, got):
    assert set(ref) == set(got)
    for k, v in ref.items():
        assert torch.equal(v, got[k]), k


@pytest.fixture(scope="module")
def plan_refs(tt):
    """the two plans of these tests with nothing queued: computed once"""
    from jodalrob_twotower_amd import ops
    old = _cfg.settings.grad_planned
    _cfg.settings.grad_planned = True
    try:
        refs = {}
        for seed in (1, 2):
            rows = _rows(seed)
            refs[seed] = (rows, _plan_out(ops.dedup_plan_keyed(rows, KS, B_PLAN, E=E)))
    finally:
        _cfg.settings.grad_planned = old
    U = int(refs[1][1]["n_unique"])
    seg = refs[1][1]["seg_offsets"]
    assert int((seg[1:] - seg[:-1]).max()) > 64 and 0 < U < B_PLAN * sum(KS)
    return refs


def _sym_inputs(seed):
    from jodalrob_twotower_amd import ops
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    n = torch.nn.functional.normalize(torch.randn(B_SYM, D_SYM, generator=g, device=DEV), dim=1)
    c = torch.nn.functional.normalize(torch.randn(B_SYM, D_SYM, generator=g, device=DEV), dim=1)
    scale_n = ops.score_unit_scale(INV_T)
    Np, Cp = ops.score_pack2_bf16(n, c, scale_n, 1.0)
    return Np, Cp, scale_n


def _sym(inputs):
    from jodalrob_twotower_amd import ops
    Np, Cp, scale_n = inputs
    r = ops.score_fwd_sym(Np, Cp, B_SYM, D_SYM, INV_T, INV_T, scale_n)
    return r[5], r[6]


@pytest.fixture(scope="module")
def sym_refs(tt):
    refs = {}
    for seed in (11, 12):
        inp = _sym_inputs(seed)
        out8, loss = _sym(inp)
        torch.cuda.synchronize()
        refs[seed] = (inp, out8.cpu().clone(), loss.cpu().clone())
        assert torch.isfinite(refs[seed][1]).all() and float(refs[seed][2]) > 0
    assert not torch.equal(refs[11][1], refs[12][1])
    return refs


@pytest.mark.parametrize("parts", [1, 2])
def test_queued_plan_runs_exactly_once(L, plan_refs, parts):
    """With TT_OPT_DEFER_RIDERS the plan call launches nothing (bit 1 of tt_deferred_pending); tt_flush_deferred launches the sort, then
    the compaction -- exactly 2 -- and the plan equals the one built with the option off; a second flush launches nothing."""
    from jodalrob_twotower_amd import ops
    dev = torch.device(DEV)
    lib, ctx = L.load(), L.ctx(dev)
    rows, ref = plan_refs[1]
    L.set_option(dev, L.TT_OPT_KEYED_PARTS, parts)
    L.set_defer_riders(dev, True)
    n0 = lib.tt_launch_count()
    plan = ops.dedup_plan_keyed(rows, KS, B_PLAN, E=E)
    assert lib.tt_launch_count() == n0 and lib.tt_deferred_pending(ctx) == 2
    L.flush_deferred(dev)
    assert lib.tt_launch_count() == n0 + 2 and lib.tt_deferred_pending(ctx) == 0
    L.flush_deferred(dev)
    assert lib.tt_launch_count() == n0 + 2
    torch.cuda.synchronize()
    _same(ref, _plan_out(plan))


def test_queued_plan_and_loss_reduction_leave_in_two_launches(L, plan_refs, sym_refs):
    """Plan and symmetric score forward both queued: one flush launches the sort, then ONE launch that carries the compaction and
    the loss reduction; out8, the loss and the plan equal their references."""
    from jodalrob_twotower_amd import ops
    dev = torch.device(DEV)
    lib, ctx = L.load(), L.ctx(dev)
    rows, ref = plan_refs[1]
    inp, ref8, ref_loss = sym_refs[11]
    L.set_defer_riders(dev, True)
    n0 = lib.tt_launch_count()
    plan = ops.dedup_plan_keyed(rows, KS, B_PLAN, E=E)
    assert lib.tt_launch_count() == n0
    out8, loss = _sym(inp)
    n1 = lib.tt_launch_count()
    assert lib.tt_deferred_pending(ctx) == 2
    L.flush_deferred(dev)
    assert lib.tt_launch_count() == n1 + 2 and lib.tt_deferred_pending(ctx) == 0
    L.flush_deferred(dev)
    assert lib.tt_launch_count() == n1 + 2
    torch.cuda.synchronize()
    assert torch.equal(out8.cpu(), ref8) and torch.equal(loss.cpu(), ref_loss)
    _same(ref, _plan_out(plan))


def test_second_plan_displaces_the_first(L, plan_refs):
    """Two plans in a row with the option on: the second call launches exactly the first plan's sort and compaction and leaves itself
    queued; both plans equal their references after the final flush."""
    from jodalrob_twotower_amd import ops
    dev = torch.device(DEV)
    lib, ctx = L.load(), L.ctx(dev)
    L.set_defer_riders(dev, True)
    n0 = lib.tt_launch_count()
    p1 = ops.dedup_plan_keyed(plan_refs[1][0], KS, B_PLAN, E=E)
    assert lib.tt_launch_count() == n0
    p2 = ops.dedup_plan_keyed(plan_refs[2][0], KS, B_PLAN, E=E)
    assert lib.tt_launch_count() == n0 + 2 and lib.tt_deferred_pending(ctx) == 2
    L.flush_deferred(dev)
    assert lib.tt_launch_count() == n0 + 4 and lib.tt_deferred_pending(ctx) == 0
    torch.cuda.synchronize()
    _same(plan_refs[1][1], _plan_out(p1))
    _same(plan_refs[2][1], _plan_out(p2))


def test_second_score_forward_displaces_the_first(L, sym_refs):
    """Two symmetric score forwards in a row: the second call launches the first one's loss reduction -- after a synchronise, without
    a flush, the first call's out8 and loss already equal their references -- and leaves its own queued."""
    dev = torch.device(DEV)
    lib, ctx = L.load(), L.ctx(dev)
    L.set_defer_riders(dev, True)
    a8, a_loss = _sym(sym_refs[11][0])
    assert lib.tt_deferred_pending(ctx) == 2
    b8, b_loss = _sym(sym_refs[12][0])
    assert lib.tt_deferred_pending(ctx) == 2
    torch.cuda.synchronize()
    assert torch.equal(a8.cpu(), sym_refs[11][1]) and torch.equal(a_loss.cpu(), sym_refs[11][2])
    n0 = lib.tt_launch_count()
    L.flush_deferred(dev)
    assert lib.tt_launch_count() == n0 + 1 and lib.tt_deferred_pending(ctx) == 0
    torch.cuda.synchronize()
    assert torch.equal(b8.cpu(), sym_refs[12][1]) and torch.equal(b_loss.cpu(), sym_refs[12][2])


# Launches one whole eager step (forward, backward, FusedAdam) saves per (slabs, riders, fuse) against the all-off step.  Narrow
# towers: what include/twotower.h documents -- 1 for the slab reduction (it rides in the embedding gradient's launch), 2 for the
# riders (compaction in tail_fwd, loss reduction in tail_bwd / tail_bwd_apply), 1 for the score backward.  Wide towers host nothing
# and queue neither slabs (first block wider than 256: the general backward) nor the score backward (D = 128): the plan and the loss
# reduction leave through tt_embed_grad_bwd's flush, where compaction and loss reduction share ONE launch -- sort, compaction,
# reduction as 2 launches instead of 3, so riders save 1.  (Derived from the launch sites; profiles/NOTES.md has the status of the
# measurement on the commit before the queue became one.)
NARROW = ([128, 64], 64)
WIDE = ([512, 256], 128)
COMBOS = [(s, r, f) for s in (False, True) for r in (False, True) for f in (False, True)]
SAVED = {
    "narrow": {c: int(c[0]) + 2 * int(c[1]) + int(c[2]) for c in COMBOS},
    "wide": {c: int(c[1]) for c in COMBOS},
}


@pytest.fixture(scope="module")
def step_refs(tt, schema_real):
    """the all-off step of either tower shape: computed once"""
    refs = {}
    for name, (hidden, D) in (("narrow", NARROW), ("wide", WIDE)):
        batch = _batch(schema_real, 192, 1100)
        state = {}
        out, n, pend = _one_step(tt, schema_real, state, batch, hidden, D, 0.1, fuse=False, pending_at="optimiser")
        assert pend == 0
        refs[name] = (batch, state, out, n)
    return refs


@pytest.mark.parametrize("slabs,riders,fuse", COMBOS[1:], ids=lambda v: str(int(v)))
@pytest.mark.parametrize("shape", ["narrow", "wide"])
def test_whole_step_under_every_option_combination(tt, schema_real, step_refs, shape, slabs, riders, fuse):
    """One whole eager step with any of the three options on == the all-off step bit for bit; nothing stays queued behind the
    optimiser; the launch count is the all-off count minus what the table above says."""
    from jodalrob_twotower_amd import _lib
    hidden, D = NARROW if shape == "narrow" else WIDE
    batch, state, ref, n_ref = step_refs[shape]
    got, n_got, pend = _one_step(tt, schema_real, state, batch, hidden, D, 0.1, fuse=fuse, riders=riders, slabs=slabs, pending_at="optimiser")
    print(f"[launches] {shape} slabs={int(slabs)} riders={int(riders)} fuse={int(fuse)}: {n_got} (all off: {n_ref})")
    _compare(ref, got)
    assert pend == 0 and _lib.load().tt_deferred_pending(_lib.ctx(torch.device(DEV))) == 0
    assert n_got == n_ref - SAVED[shape][(slabs, riders, fuse)], (n_got, n_ref)
