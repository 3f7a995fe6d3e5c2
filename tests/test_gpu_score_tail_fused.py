"""The towers' backward head run inside the score backward's launch (TT_OPT_FUSE_SCORE_TAIL: tt_score_bwd_bf16 leaves its launch queued,
tt_towers_mlp_bwd issues score_bwd_tr_kernel<4, 2, UNIT, false, true> in place of tail_bwd_kernel) against the two-launch path of
the same build, bit for bit: the head is one device function with two hosts (csrc/tt_tail_bwd.h), the sweep and the cross-wave tree
are the same code.

Shapes.  The fusion needs 64-row chunks numbered like the score backward's 64-row tiles (chunks_for: min(128, cdiv(B, 64)) chunks of
cdiv(B, chunks) rows), two towers with H = D = 64, no logQ, bf16 score operands:
  fuse:      B = 64 one workgroup per direction; 127 two chunks, last row missing (ragged last b tile of the sweep, ragged last chunk
             of the head); 192; 1024.
  fall back: B = 185 (three chunks of 62), 1000 (chunks of 63); final dim 32 and 128; H = 40; the wide tail [512, 256] -> 128; logQ;
             score_dtype bf16x3.
The launch counter tells which path ran: one launch fewer where the fusion applies, the same number where it does not."""
import numpy as np
import pytest
import torch

from _eager_step import DEV, _batch, _compare, _one_step, _task

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tt():
    import jodalrob_twotower_amd as m
    from jodalrob_twotower_amd import _lib
    _lib.load()
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return m


FUSE = [(64, 0.0, None), (127, 0.1, None), (127, 0.0, None), (192, 0.1, None), (1024, 0.0, None), (1024, 0.1, 1.2)]


@pytest.mark.parametrize("B,p,zipf", FUSE)
@pytest.mark.parametrize("riders", [False, True])
def test_fused_step_equals_two_launch_step(tt, schema_real, B, p, zipf, riders):
    """One whole step, towers [128, 64] -> 64, with the head in the score backward's launch == the same step with two launches: d_emb
    of both towers, the loss, every parameter gradient (w_out / b_out come from the head's slabs, the BN gradients from its S1 / S2,
    everything below from its d_act), running BN buffers, the table.  One launch fewer; nothing stays queued behind the backward.
    riders: the queued loss reduction rides tail_bwd_apply's extra grid row instead of tail_bwd's."""
    batch = _batch(schema_real, B, 900 + B, zipf)
    state = {}
    ref, n_ref, pend_ref = _one_step(tt, schema_real, state, batch, [128, 64], 64, p, fuse=False, riders=riders)
    got, n_got, pend_got = _one_step(tt, schema_real, state, batch, [128, 64], 64, p, fuse=True, riders=riders)
    _compare(ref, got)
    assert pend_ref & 4 == 0 and pend_got & 4 == 0
    assert n_got == n_ref - 1, (n_got, n_ref)


FALLBACK = [(185, [128, 64], 64, {}), (1000, [128, 64], 64, {}), (192, [128, 64], 32, {}), (192, [128, 64], 128, {}),
            (192, [128, 40], 64, {}), (192, [512, 256], 128, {}), (192, [128, 64], 64, {"log_q": True}),
            (192, [128, 64], 64, {"score_dtype": "bf16x3"})]


@pytest.mark.parametrize("B,hidden,D,kw", FALLBACK, ids=lambda v: str(v).replace(" ", ""))
def test_shapes_that_do_not_fuse_equal_the_option_off_step(tt, schema_real, B, hidden, D, kw):
    """Chunks that are not 64 rows, other widths, the wide tail, logQ, bf16x3 operands: with the option set the step takes the two
    launches it takes without it (a queued score backward is launched in front of the towers' backward; the other score entries
    never queue) -- same results, same number of launches."""
    batch = _batch(schema_real, B, 700 + B, log_q=kw.get("log_q", False))
    sd = kw.get("score_dtype", "bf16")
    state = {}
    ref, n_ref, _ = _one_step(tt, schema_real, state, batch, hidden, D, 0.1, fuse=False, score_dtype=sd)
    got, n_got, pend = _one_step(tt, schema_real, state, batch, hidden, D, 0.1, fuse=True, score_dtype=sd)
    _compare(ref, got)
    assert pend & 4 == 0 and n_got == n_ref, (n_got, n_ref)


def test_dense_gradient_mode_equals_the_option_off_step(tt, schema_real):
    """embedding_grad="dense" (no plan, no tt_embed_grad_bwd behind the towers: the optimiser entries are the next flush point) at a
    shape whose towers can host the score backward: the step equals the option-off step and nothing stays queued behind it."""
    from jodalrob_twotower_amd import _lib as L
    batch = _batch(schema_real, 192, 31)
    state = {}
    ref, n_ref, _ = _one_step(tt, schema_real, state, batch, [128, 64], 64, 0.1, fuse=False, embedding_grad="dense")
    got, n_got, pend = _one_step(tt, schema_real, state, batch, [128, 64], 64, 0.1, fuse=True, embedding_grad="dense")
    _compare(ref, got)
    assert pend & 4 == 0 and n_ref - n_got in (0, 1)
    assert L.load().tt_deferred_pending(L.ctx(torch.device(DEV))) == 0


@pytest.mark.parametrize("how", ["flush", "clear"])
@pytest.mark.parametrize("B", [127, 256])
def test_queued_score_backward_runs_exactly_once(tt, how, B):
    """Queue discipline on the bare entry: with the option set tt_score_bwd_bf16 launches nothing (bit 2 of tt_deferred_pending);
    tt_flush_deferred alone / clearing the option alone then yields the stand-alone call's d_emb with exactly one launch, and
    nothing stays queued (a second flush launches nothing)."""
    from jodalrob_twotower_amd import _lib as L
    from jodalrob_twotower_amd import ops
    dev = torch.device(DEV)
    D, inv_t = 64, 20.0
    g = torch.Generator(device=DEV)
    g.manual_seed(5 + B)
    n = torch.nn.functional.normalize(torch.randn(B, D, generator=g, device=DEV), dim=1)
    c = torch.nn.functional.normalize(torch.randn(B, D, generator=g, device=DEV), dim=1)
    scale_n = ops.score_unit_scale(inv_t)
    Np, Cp = ops.score_pack2_bf16(n, c, scale_n, 1.0)
    rowsum, colsum, _, _, _, _, inv = ops.score_fwd_bf16(Np, Cp, B, D, inv_t, inv_t, False, False, scale_n, with_inv=True)
    d_loss = torch.ones(1, device=DEV)
    args = (Np, Cp, B, D, inv_t, inv_t, rowsum, colsum, d_loss, inv_t / (2.0 * B), scale_n, inv)
    lib, ctx = L.load(), L.ctx(dev)
    refN, refC = ops.score_bwd_bf16(*args)
    torch.cuda.synchronize()
    assert lib.tt_deferred_pending(ctx) == 0
    L.set_fuse_score_tail(dev, True)
    try:
        n0 = lib.tt_launch_count()
        dN, dC = ops.score_bwd_bf16(*args)
        assert lib.tt_launch_count() == n0 and lib.tt_deferred_pending(ctx) == 4
        if how == "flush":
            L.flush_deferred(dev)
        else:
            L.set_fuse_score_tail(dev, False)
        assert lib.tt_launch_count() == n0 + 1 and lib.tt_deferred_pending(ctx) == 0
        L.flush_deferred(dev)
        L.set_fuse_score_tail(dev, False)
        assert lib.tt_launch_count() == n0 + 1
        torch.cuda.synchronize()
        assert torch.equal(dN, refN) and torch.equal(dC, refC) and torch.isfinite(refN).all() and refN.abs().max() > 0
    finally:
        L.set_fuse_score_tail(dev, False)


@pytest.mark.parametrize("B", [1024, 127])
@pytest.mark.parametrize("riders", [True, False])
def test_replayed_fused_step_equals_unfused_and_eager(tt, schema_real, B, riders):
    """Three replays of GraphedTrainStep with the option on == three replays with it off == three eager steps (p = 0): losses and the
    final state_dict bit for bit; the captured step has one library launch fewer.  riders on and off: the loss reduction's new
    host (tail_bwd_apply's extra row) and the plain launch."""
    from jodalrob_twotower_amd.graph import GraphedTrainStep
    from jodalrob_twotower_amd.optim import FusedAdam
    batches = [_batch(schema_real, B, 500 + i) for i in range(4)]
    finals, state, launches = {}, None, {}
    for mode in ("fused", "unfused", "eager"):
        task = _task(tt, schema_real, [128, 64], 64, 0.0)
        if state is None:
            state = {k: v.detach().clone() for k, v in task.state_dict().items()}
        task.load_state_dict(state)
        opt = FusedAdam.for_task(task, lr=1e-2, weight_decay=1e-5)
        losses = []
        if mode == "eager":
            for b in batches[1:]:
                opt.zero_grad()
                r = task(b, return_metrics=True)
                r["loss"].backward()
                opt.step()
                losses.append(r["loss"].item())
        else:
            gs = GraphedTrainStep(task, opt, batches[0], warmup=1, defer_riders=riders, fuse_score_tail=mode == "fused")
            launches[mode] = gs.library_launches
            for b in batches[1:]:
                losses.append(gs.step(b)["loss"].item())
            torch.cuda.synchronize()
            gs.close()
        finals[mode] = (losses, {k: v.detach().cpu().clone() for k, v in task.state_dict().items()})
    for m in ("unfused", "eager"):
        assert finals["fused"][0] == finals[m][0], m
        for k, v in finals["fused"][1].items():
            assert torch.equal(v, finals[m][1][k]), (m, k)
    assert launches["fused"] == launches["unfused"] - 1, launches
    assert len(set(finals["fused"][0])) == 3 and np.isfinite(finals["fused"][0]).all()


def test_replayed_step_that_cannot_fuse_keeps_its_launches(tt, schema_real):
    """B = 1000 (chunks of 63 rows), dropout on: the captured step with the option on replays the launches of the step with it off,
    with the same losses and final state."""
    from jodalrob_twotower_amd.graph import GraphedTrainStep
    from jodalrob_twotower_amd.optim import FusedAdam
    batches = [_batch(schema_real, 1000, 600 + i) for i in range(4)]
    finals, state, launches = {}, None, {}
    for mode in ("fused", "unfused"):
        task = _task(tt, schema_real, [128, 64], 64, 0.1)
        if state is None:
            state = {k: v.detach().clone() for k, v in task.state_dict().items()}
        task.load_state_dict(state)
        opt = FusedAdam.for_task(task, lr=1e-2, weight_decay=1e-5)
        gs = GraphedTrainStep(task, opt, batches[0], warmup=1, fuse_score_tail=mode == "fused")
        launches[mode] = gs.library_launches
        losses = [gs.step(b)["loss"].item() for b in batches[1:]]
        torch.cuda.synchronize()
        gs.close()
        finals[mode] = (losses, {k: v.detach().cpu().clone() for k, v in task.state_dict().items()})
    assert finals["fused"][0] == finals["unfused"][0] and launches["fused"] == launches["unfused"], launches
    for k, v in finals["fused"][1].items():
        assert torch.equal(v, finals["unfused"][1][k]), k
