"""The towers' BatchNorm batch statistics finished once per tower by a rider workgroup in the keyed sort's launch (tt_riders.h:
BnFinishRider; tail_fwd_kernel<true> reads the finished pair) against the in-tail finish of the same build (every tail workgroup
merges the chunk partials itself: tail_fwd_kernel<false>), bit for bit -- the merge order is one device function with two hosts.

The rider path is taken whenever TT_OPT_DEFER_RIDERS queues the keyed plan (what GraphedTrainStep replays) and towers with the
fused narrow tail follow; it needs no graph, so the step-level cases set the option around eager steps.  Batch sizes follow the
chunking of the statistics (chunks_for: min(128, cdiv(B, 64)) chunks of cdiv(B, chunks) rows for H <= 64):
B = 64 one chunk, 65 two chunks (33 + 32 rows), 200 four chunks, 700 eleven chunks (no multiple of 4 or of kSubChain = 8, ragged
last one), 8192 the 128-chunk maximum (once).  The Zipf batch sends hot keys of the plan to the LSD fallback of the sort."""
import numpy as np
import pytest
import torch

from conftest import GOLD

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def tt():
    import jodalrob_twotower_amd as m
    from jodalrob_twotower_amd import _lib
    _lib.load()
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return m


def _task(tt, schema_real, hidden, D, p, embedding_grad="sparse"):
    kn, kc = schema_real["notice"]["categorical"], schema_real["company"]["categorical"]
    torch.manual_seed(9)
    task = tt.create_two_tower_train_task(kn, kc, metadata_path=str(GOLD / "real_vocab_metadata.csv"), categorical_embedding_dim=32,
                                          notice_dense_input_dim=256, company_dense_input_dim=128, tower_hidden_dims=hidden,
                                          final_embedding_dim=D, dropout_rate=p, device=DEV, embedding_grad=embedding_grad,
                                          score_dtype="bf16", mlp_dtype="bf16")
    task._pair_check_done = True
    task.train()
    for tw in (task.two_tower_model.notice_tower, task.two_tower_model.company_tower):
        tw._seed_override = 77
    return task


def _batch(schema_real, B, seed, zipf=None):
    from jodalrob_twotower_amd import synthetic
    kn, kc = schema_real["notice"]["categorical"], schema_real["company"]["categorical"]
    vn, vc = schema_real["notice"]["vocab_sizes"], schema_real["company"]["vocab_sizes"]
    return synthetic.make_batch(B, vn, vc, kn, kc, 256, 128, torch.device(DEV), seed=seed, zipf_alpha=zipf)


def _sides_of(loss):
    """the towers' autograd node of this step (towers.py keeps its per-side buffers on it)"""
    seen, todo = set(), [loss.grad_fn]
    while todo:
        fn = todo.pop()
        if fn is None or id(fn) in seen:
            continue
        seen.add(id(fn))
        if hasattr(fn, "sides") and hasattr(fn, "plans"):
            return fn.sides
        todo.extend(f for f, _ in fn.next_functions)
    raise AssertionError("no tower node under the loss")


def _side_tensors(s):
    """pre / act / mean / rstd of every block and y out of the side's flat activation buffer (the gaps between them are padding)"""
    from jodalrob_twotower_amd.towers import _al
    tw, B = s.tower, s.B
    hid, D = list(tw.tower_hidden_dims[1:]), tw.final_embedding_dim
    names = [f"{n}{i}" for i in range(len(hid)) for n in ("pre", "act")] + [f"{n}{i}" for i in range(len(hid)) for n in ("mean", "rstd")] + ["y"]
    lens = [B * h for h in hid for _ in (0, 1)] + [h for h in hid for _ in (0, 1)] + [B * D]
    off = s.buf.numel() - sum(_al(z) for z in lens)
    out = {}
    for n, z in zip(names, lens):
        out[n] = s.buf[off:off + z].detach().cpu().clone()
        off += _al(z)
    out["emb"] = s.emb.detach().cpu().clone()
    if s.packed is not None:
        out["packed"] = s.packed.detach().cpu().clone()
    return out


def _one_step(tt, schema_real, state, batch, hidden, D, p, riders):
    """one whole eager step; riders: TT_OPT_DEFER_RIDERS around it, as the captured step has it"""
    from jodalrob_twotower_amd import _lib as L
    from jodalrob_twotower_amd.optim import FusedAdam
    dev = torch.device(DEV)
    task = _task(tt, schema_real, hidden, D, p)
    if state:
        task.load_state_dict(state)
    else:
        state.update({k: v.detach().clone() for k, v in task.state_dict().items()})
    opt = FusedAdam.for_task(task, lr=1e-2, weight_decay=1e-5)
    launches = L.load().tt_launch_count()
    try:
        if riders:
            L.set_defer_riders(dev, True)
        res = task(batch, return_metrics=True)
        fwd_pending = L.load().tt_deferred_pending(L.ctx(dev))
        out = {}
        for i, s in enumerate(_sides_of(res["loss"])):      # (read before the backward reuses any of them)
            out.update({f"side{i}.{k}": v for k, v in _side_tensors(s).items()})
        res["loss"].backward()
        out["loss"] = res["loss"].detach().cpu().clone()    # (a riding loss reduction writes it in tail_bwd's launch)
        for n_, p_ in task.named_parameters():
            if p_.grad is not None:
                out["grad." + n_] = p_.grad.detach().cpu().clone()
        store = opt._stores[0]
        plan, rows = store.sparse_grad
        L.flush_deferred(dev)
        U = int(plan.n_unique.item())
        out.update({"plan.sorted_src": plan.sorted_src.cpu().clone(), "plan.unique_rows": plan.unique_rows[:U].cpu().clone(),
                    "plan.seg_offsets": plan.seg_offsets[:U + 1].cpu().clone(), "plan.grad_rows": rows[:U].cpu().clone()})
        opt.step()
        torch.cuda.synchronize()
    finally:
        if riders:
            L.set_defer_riders(dev, False)
    launches = L.load().tt_launch_count() - launches
    out.update({"state." + k: v.detach().cpu().clone() for k, v in task.state_dict().items()})     # (running BN buffers and the table among them)
    st = opt._state_of(store)
    out.update({"opt.m": st["m"].cpu().clone(), "opt.v": st["v"].cpu().clone()})
    return out, launches, fwd_pending


CASES = [(64, [128, 64], 64, 0.0, None), (65, [128, 64], 64, 0.1, None), (200, [128, 40], 32, 0.1, None), (200, [128, 40], 32, 0.0, None),
         (700, [128, 64], 64, 0.1, None), (2048, [128, 64], 64, 0.1, 1.2), (8192, [128, 64], 64, 0.1, None)]


@pytest.mark.parametrize("B,hidden,D,p,zipf", CASES)
def test_step_with_statistics_rider_equals_in_tail_finish(tt, schema_real, B, hidden, D, p, zipf):
    """One whole step (forward, backward, FusedAdam) with the keyed sort issued behind tower_front and the statistics riders in
    its grid == the same step with the sort in front and the finish in every tail workgroup: pre, act, saved mean / rstd, y, emb,
    both packed operand images, the loss, every parameter gradient, the dedup plan (sorted_src, unique rows, segment offsets; the
    long-row list through the gradient rows it produces), running BN buffers, num_batches_tracked, the table and its Adam state.
    The notice tower reads 256 dense columns, the company tower 128.  The riders' form takes two launches fewer (compaction and loss reduction ride):
    the sort is one launch in either place."""
    batch = _batch(schema_real, B, 400 + B, zipf)
    state = {}
    ref, n_ref, pend_ref = _one_step(tt, schema_real, state, batch, hidden, D, p, riders=False)
    got, n_got, pend_got = _one_step(tt, schema_real, state, batch, hidden, D, p, riders=True)
    assert set(ref) == set(got)
    for k, v in ref.items():
        assert torch.equal(v, got[k]), k
    assert torch.isfinite(ref["loss"]).all() and any(k.endswith(".packed") for k in ref)
    assert pend_ref & 2 == 0 and pend_got & 2 == 2          # (the loss reduction waits for tail_bwd; the sort and the compaction were hosted:
    #                                                          the pair of them would otherwise show as two more launches)
    assert n_got == n_ref - 2                                # compaction and loss reduction ride; the sort is one launch in either place


def test_queued_sort_without_a_host_is_flushed(tt, schema_real):
    """Towers that do not take the fused narrow tail ([512, 256] -> 128: the wide tail) leave the queued sort and its compaction to
    the flush in front of the embedding gradient: the sort runs without riders (bf_wg = 0) and the step is the unqueued one's."""
    batch = _batch(schema_real, 300, 77)
    state = {}
    ref, _, _ = _one_step(tt, schema_real, state, batch, [512, 256], 128, 0.1, riders=False)
    got, _, pend = _one_step(tt, schema_real, state, batch, [512, 256], 128, 0.1, riders=True)
    assert pend & 2 == 2
    for k, v in ref.items():
        assert torch.equal(v, got[k]), k


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_replayed_rider_step_equals_eager_and_fallbacks(tt, schema_real, p):
    """Three replays of the captured step (statistics riders in the sort's launch) == three eager steps (in-tail finish) == three
    replays with the riders off (the parent's launches), and the dense-gradient mode (no plan, hence no sort to ride in) replayed ==
    eager: losses and final state bit for bit.  B = 1000: ragged last tile and chunk.  (With dropout the eager steps draw their own
    seeds, so the eager leg runs at p = 0 only; the two captured forms share the seed override.)"""
    from jodalrob_twotower_amd.graph import GraphedTrainStep
    from jodalrob_twotower_amd.optim import FusedAdam
    B = 1000
    batches = [_batch(schema_real, B, 500 + i) for i in range(4)]
    for grad in ("sparse", "dense"):
        finals, state, launches = {}, None, {}
        modes = ("riders", "no_riders") + (("eager",) if p == 0.0 else ())
        for mode in modes if grad == "sparse" else (("riders", "eager") if p == 0.0 else ()):
            task = _task(tt, schema_real, [128, 64], 64, p, embedding_grad=grad)
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
                gs = GraphedTrainStep(task, opt, batches[0], warmup=1, defer_riders=mode == "riders")
                launches[mode] = gs.library_launches
                for b in batches[1:]:
                    losses.append(gs.step(b)["loss"].item())
                torch.cuda.synchronize()
                gs.close()
            finals[mode] = (losses, {k: v.detach().cpu().clone() for k, v in task.state_dict().items()})
        names = list(finals)
        for m in names[1:]:
            assert finals[names[0]][0] == finals[m][0], (grad, m)
            for k, v in finals[names[0]][1].items():
                assert torch.equal(v, finals[m][1][k]), (grad, m, k)
        if "no_riders" in launches:                          # compaction and loss reduction ride; the sort is one launch in either place
            assert launches["riders"] == launches["no_riders"] - 2, launches
        if names:
            assert len(set(finals[names[0]][0])) == 3 and np.isfinite(finals[names[0]][0]).all()
