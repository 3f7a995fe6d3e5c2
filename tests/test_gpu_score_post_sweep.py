"""What the score backward's workgroups do behind their sweep when they host the towers' backward head
(score_bwd_tr_kernel<4, 2, UNIT, false, true>, csrc/tt_score_bf16.hip), and where the symmetric forward's loss reduction rides then.

The head is hosted when its row chunks are the score backward's 64-row tiles: cdiv(B, chunks) == 64 with chunks = min(128,
cdiv(B, 64)) -- B = 64 k - j with j < k (64; 127, 128; 190 .. 192; ...).  Every other B takes the two launches whatever the option
says; the launch counter tells which path ran (one launch fewer when hosted).

A. The flat final reduction.  Behind round one of the cross-wave tree the hosted form adds the four slabs as (s0 + s2) + (s1 + s3) in
   the thread that normalises the row in the head -- the tree's own association -- and hands d_emb on in registers.  One whole eager step
   with TT_OPT_FUSE_SCORE_TAIL on == the same step with it off (tail_bwd_kernel reading d_emb from memory behind the tree of the sweep-only
   form), bit for bit: d_emb, the loss, every dense gradient, the table-gradient rows, the state behind the optimiser.  Towers
   [128, 64] -> 64; unit and non-unit score form (the notice image packed times 2 instead of inv_t log2 e); dropout off and 0.1 with
   a fixed seed.  Batch sizes (test_gpu_score_tail_fused.py has 64 with dropout off, 127, 192 and 1024):
     64    hosted.  Two b tiles: waves 2 .. 7 sweep nothing and must contribute exact zeros to the flat sum (dropout on; non-unit)
     512   hosted.  16 b tiles: both buffers of every wave used exactly once
     190   hosted.  Three chunks, the last with 62 live rows; six b tiles, the last ragged: waves 6 and 7 sweep nothing
     568   hosted.  Nine chunks, the last with 56 live rows; 18 b tiles, the last ragged: waves 0 and 1 take a third tile
     2, 65, 70, 544   NOT hosted (chunks of 2, 33, 35 and 61 rows): a chunk of one or six live rows and a 17-tile sweep cannot meet
           the hosted form, whose last chunk has at least 65 - chunks rows; the option-on step is the option-off step, launch for launch
   The launch counter is checked in every case; test_launch_count_shows_the_hosted_path states it for one B of either kind.

B. The loss reduction (slot TT_DQ_LOSS of csrc/tt_deferred.h, Finish2Rider) rides gemm_back_kernel's launch when the score backward
   hosts the head: finish2_body on 256 threads, every thread running the four (j, q) items it stands in for in the 1024-thread
   order.  Loss and out8 of a forward + backward with riders and the hosted head on == those of the same forward with NO backward
   behind it, whose queued reduction leaves through tt_flush_deferred as a 1024-thread launch of its own -- bit for bit, and the
   backward launches nothing for it (as many launches as with the riders off, less the two the riders save).
     64    one partial record; hosted, gemm_back takes the rider
     128   two records; hosted, gemm_back
     2112  33 records: the second trip of the record loop; hosted, gemm_back
     127   two records; hosted, but B is no multiple of 64: the pass has no gemm_back launch and tail_bwd_apply's extra row takes it
     70    two records; towers that do not host the head: tail_bwd_kernel's extra row takes it
     185   three records; the same"""
import pytest
import torch

import _eager_step
from _eager_step import DEV, _batch, _compare, _one_step

pytestmark = pytest.mark.gpu

HIDDEN, D = [128, 64], 64


@pytest.fixture(scope="module")
def tt():
    import jodalrob_twotower_amd as m
    from jodalrob_twotower_amd import _lib
    _lib.load()
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return m


@pytest.fixture()
def form(request, monkeypatch):
    """unit: the task as it is.  nonunit: the notice image is packed times 2, so the score kernels take their general form"""
    if request.param == "nonunit":
        make = _eager_step._task

        def task(*a, **k):
            t = make(*a, **k)
            t.two_tower_model.notice_tower.pack_scale = 2.0
            return t
        monkeypatch.setattr(_eager_step, "_task", task)
    return request.param


def _hosts(B):
    chunks = min(128, -(-B // 64))
    return -(-B // chunks) == 64


# (B, dropout p, form) -- every B in both forms and with dropout on and off
HOSTED = [(B, p, f) for B in (2, 64, 65, 70, 190, 512, 544, 568) for p, f in ((0.0, "unit"), (0.1, "nonunit"))]
HOSTED = [(B, 0.1 - p if B in (64, 70, 544) else p, f) for B, p, f in HOSTED]        # (64 with dropout off and unit: the other file)


@pytest.mark.parametrize("B,p,form", HOSTED, indirect=["form"])
def test_hosted_step_equals_two_launch_step(tt, schema_real, B, p, form):
    batch = _batch(schema_real, B, 1300 + B)
    state = {}
    ref, n_ref, pend_ref = _one_step(tt, schema_real, state, batch, HIDDEN, D, p, fuse=False)
    got, n_got, pend_got = _one_step(tt, schema_real, state, batch, HIDDEN, D, p, fuse=True)
    _compare(ref, got)
    assert ref["d_emb0"].abs().max() > 0 and ref["d_emb1"].abs().max() > 0
    assert pend_ref & 4 == 0 and pend_got & 4 == 0
    assert n_got == n_ref - int(_hosts(B)), (n_got, n_ref)


@pytest.mark.parametrize("form", ["unit"], indirect=True)
def test_launch_count_shows_the_hosted_path(tt, schema_real, form):
    """B = 128 hosts (two 64-row chunks numbered like the score backward's tiles): one launch fewer than the option-off step.  B = 185
    (three chunks of 62 rows) cannot: the same number of launches.  Both equal their option-off step."""
    assert _hosts(128) and not _hosts(185)
    for B, saved in ((128, 1), (185, 0)):
        batch = _batch(schema_real, B, 1400 + B)
        state = {}
        ref, n_ref, _ = _one_step(tt, schema_real, state, batch, HIDDEN, D, 0.0, fuse=False)
        got, n_got, _ = _one_step(tt, schema_real, state, batch, HIDDEN, D, 0.0, fuse=True)
        _compare(ref, got)
        assert n_got == n_ref - saved, (B, n_got, n_ref)


def _forward(tt, schema_real, state, batch, riders, backward):
    """forward (+ backward) of the task at dropout 0.1 with the hosted head on; riders: TT_OPT_DEFER_RIDERS around it.  Without a
    backward, what stays queued leaves through tt_flush_deferred.  Returns (loss, out8), the library's launches, and
    tt_deferred_pending right behind the last call."""
    from jodalrob_twotower_amd import _lib as L
    dev = torch.device(DEV)
    task = _eager_step._task(tt, schema_real, HIDDEN, D, 0.1)
    if state:
        task.load_state_dict(state)
    else:
        state.update({k: v.detach().clone() for k, v in task.state_dict().items()})
    lib = L.load()
    n0 = lib.tt_launch_count()
    try:
        L.set_fuse_score_tail(dev, True)
        if riders:
            L.set_defer_riders(dev, True)
        res = task(batch, return_metrics=True)
        if backward:
            res["loss"].backward()
        pending = lib.tt_deferred_pending(L.ctx(dev))
        L.flush_deferred(dev)
        torch.cuda.synchronize()
        out = (res["loss"].detach().cpu().clone(), res.out8.detach().cpu().clone())
    finally:
        L.set_defer_riders(dev, False)
        L.set_fuse_score_tail(dev, False)
    return out, lib.tt_launch_count() - n0, pending


@pytest.mark.parametrize("B", [64, 70, 127, 128, 185, 2112])
def test_loss_rider_equals_the_flushed_reduction(tt, schema_real, B):
    batch = _batch(schema_real, B, 1500 + B)
    state = {}
    # no backward behind the forward: the loss reduction is still queued (bit 1 of tt_deferred_pending) and the flush delivers it
    (loss_f, out8_f), _, pend_f = _forward(tt, schema_real, state, batch, riders=True, backward=False)
    assert pend_f & 2 and torch.isfinite(out8_f).all() and float(loss_f) > 0 and loss_f == out8_f[0]
    # the reduction launched at once by the forward (riders off): the same
    (loss_0, out8_0), n_0, _ = _forward(tt, schema_real, state, batch, riders=False, backward=True)
    assert torch.equal(loss_0, loss_f) and torch.equal(out8_0, out8_f)
    # riding in the backward: gemm_back's first workgroup / tail_bwd_apply's row / tail_bwd's row (see the list above)
    (loss_r, out8_r), n_r, pend_r = _forward(tt, schema_real, state, batch, riders=True, backward=True)
    assert torch.equal(loss_r, loss_f) and torch.equal(out8_r, out8_f)
    assert pend_r & 2 == 0 and n_r == n_0 - 2, (n_r, n_0)
