"""One whole eager training step of the two-tower task on the real 32 + 6 key schema, with the context options that queue launches
(TT_OPT_FUSE_SCORE_TAIL, TT_OPT_DEFER_RIDERS, TT_OPT_DEFER_SLAB_REDUCE) set around it as the captured step sets them: shared by the
tests that compare such steps bit for bit and count their launches."""
import torch

from conftest import GOLD

DEV = "cuda:0"


def _task(tt, schema_real, hidden, D, p, embedding_grad="sparse", score_dtype="bf16"):
    kn, kc = schema_real["notice"]["categorical"], schema_real["company"]["categorical"]
    torch.manual_seed(9)
    task = tt.create_two_tower_train_task(kn, kc, metadata_path=str(GOLD / "real_vocab_metadata.csv"), categorical_embedding_dim=32,
                                          notice_dense_input_dim=256, company_dense_input_dim=128, tower_hidden_dims=hidden,
                                          final_embedding_dim=D, dropout_rate=p, device=DEV, embedding_grad=embedding_grad,
                                          score_dtype=score_dtype, mlp_dtype="bf16")
    task._pair_check_done = True
    task.train()
    for tw in (task.two_tower_model.notice_tower, task.two_tower_model.company_tower):
        tw._seed_override = 77
    return task


def _batch(schema_real, B, seed, zipf=None, log_q=False):
    from jodalrob_twotower_amd import synthetic
    kn, kc = schema_real["notice"]["categorical"], schema_real["company"]["categorical"]
    vn, vc = schema_real["notice"]["vocab_sizes"], schema_real["company"]["vocab_sizes"]
    b = synthetic.make_batch(B, vn, vc, kn, kc, 256, 128, torch.device(DEV), seed=seed, zipf_alpha=zipf)
    if log_q:
        g = torch.Generator(device=DEV)
        g.manual_seed(seed + 1)
        for side in ("notice", "company"):
            b[side]["log_q"] = -8.0 * torch.rand(B, generator=g, device=DEV, dtype=torch.float32)
    return b


def _one_step(tt, schema_real, state, batch, hidden, D, p, fuse, riders=False, embedding_grad="sparse", score_dtype="bf16", slabs=False,
              pending_at="backward"):
    """one whole eager step (forward, backward, FusedAdam); fuse / riders: the context options around it, slabs: around the backward
    only, as the captured step has them.  Returns (everything the step produced, library launches, tt_deferred_pending right after
    the backward -- pending_at="optimiser": right after the optimiser step, the options still set)."""
    from jodalrob_twotower_amd import _lib as L
    from jodalrob_twotower_amd import towers
    from jodalrob_twotower_amd.optim import FusedAdam
    dev = torch.device(DEV)
    task = _task(tt, schema_real, hidden, D, p, embedding_grad, score_dtype)
    if state:
        task.load_state_dict(state)
    else:
        state.update({k: v.detach().clone() for k, v in task.state_dict().items()})
    opt = FusedAdam.for_task(task, lr=1e-2, weight_decay=1e-5)
    launches = L.load().tt_launch_count()
    towers._DEBUG_KEEP = keep = []
    try:
        if fuse:
            L.set_fuse_score_tail(dev, True)
        if riders:
            L.set_defer_riders(dev, True)
        res = task(batch, return_metrics=True)
        if slabs:
            L.set_defer_slab_reduce(dev, True)
        try:
            res["loss"].backward()
        finally:
            if slabs:
                L.set_defer_slab_reduce(dev, False)      # (flushes)
        pending = L.load().tt_deferred_pending(L.ctx(dev))
        out = {f"d_emb{i}": k["d_emb"].detach().cpu().clone() for i, k in enumerate(keep)}
        out["loss"] = res["loss"].detach().cpu().clone()
        for n_, p_ in task.named_parameters():
            if p_.grad is not None:
                g = p_.grad
                out["grad." + n_] = (g.to_dense() if g.is_sparse else g).detach().cpu().clone()
        opt.step()
        if pending_at == "optimiser":
            pending = L.load().tt_deferred_pending(L.ctx(dev))
        torch.cuda.synchronize()
    finally:
        towers._DEBUG_KEEP = None
        if riders:
            L.set_defer_riders(dev, False)
        if fuse:
            L.set_fuse_score_tail(dev, False)
    launches = L.load().tt_launch_count() - launches
    out.update({"state." + k: v.detach().cpu().clone() for k, v in task.state_dict().items()})
    return out, launches, pending


def _compare(ref, got):
    assert set(ref) == set(got)
    for k, v in ref.items():
        assert torch.equal(v, got[k]), k
    assert torch.isfinite(ref["loss"]).all() and "d_emb0" in ref and "d_emb1" in ref
