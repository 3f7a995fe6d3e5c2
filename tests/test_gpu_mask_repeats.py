"""Repeated-entity mask of the in-batch softmax on the MI355X (include/twotower.h *_mask entries).

1. The score node (_ScoreCEFn with ent_n / ent_c) against the float64 reference of tests/_mask_reference.py, fed the kernels' own
   operand rounding: bf16 and fp32, ragged shapes, five id patterns; the masked per-row sums; metrics and ranks bitwise the plain call's.
2. Mask and logQ correction together.
3. An inert mask (all ids distinct) is bit-identical to the plain entry wherever the masked dispatch picks the plain one's kernel form.
4. Runs are bitwise reproducible.
5. Wiring: eager task, GraphedTrainStep.step and step_from_store fed by DevicePairLoader(mask_repeats=True) agree bit for bit; the mask
   changes the loss; a captured step refuses a batch whose entity ids do not match its capture.
6. Refusals: fp8, bf16x3, the dense loss, wrong dtype / shape / device, rectangular problems, the temperature limit with logQ.

Bounds: those tests/test_gpu_logq.py holds the same mode to (imported).  They carry over: the masked sums are sub-sums of the same
positive terms -- every kept term has the relative error it has in the unmasked sum and a masked one contributes exactly zero on both
sides, so a per-term relative bound bounds the sub-sum; the softmax weights are the same terms over those sums.
"""
import functools

import numpy as np
import pytest
import torch

from test_gpu_parity import DEV, tt, ctx_option, make_task, to_batch, load_state  # noqa: F401
from test_gpu_logq import BOUNDS, LOSS_ATOL, _sum_rtol, _nrel, _lq, _unit_rows, _pair_world
from _mask_reference import ids, reference, ref_sums, unit_scale

pytestmark = pytest.mark.gpu

SHAPES = [(1, 32, 1.0), (33, 1, 0.5), (65, 64, 0.05), (257, 200, 2.0), (257, 64, 0.05), (2048, 128, 1.0),
          (97, 96, 1.0)]                              # (the 65..128 class of D at a ragged B: four tiles, the last one partial)
PATTERNS = ["distinct", "one_notice", "tile_edge", "groups", "heavy"]
MODES = ["bf16", "fp32"]


@functools.lru_cache(maxsize=None)
def _inputs(B, D):
    return _unit_rows(B, D, 11 + B + D), _unit_rows(B, D, 29 + B + D)


@functools.lru_cache(maxsize=None)
def _ids(B, pattern):
    return ids(B, pattern, seed=B, device=DEV)


@functools.lru_cache(maxsize=None)
def _lqs(B, D, kind):
    return (None, None) if kind is None else (_lq(B, kind, 3 + B), _lq(B, kind, 5 + D))


@functools.lru_cache(maxsize=None)
def _ref(B, D, T, pattern, mode, kind=None):
    """(loss, dN, dC, rowsum, colsum) in f64: computed once per case, shared, never written to"""
    n, c = _inputs(B, D)
    en, ec = _ids(B, pattern)
    lq_n, lq_c = _lqs(B, D, kind)
    return reference(n, c, 1.0 / T, en, ec, mode, lq_n, lq_c) + ref_sums(n, c, 1.0 / T, en, ec, mode, lq_n, lq_c)


def _run(n, c, inv_t, mode, ent=(None, None), lq=(None, None), first_call=False):
    from jodalrob_twotower_amd.two_tower_train_task import _ScoreCEFn
    n = n.clone().requires_grad_(True)
    c = c.clone().requires_grad_(True)
    loss, out8, rank = _ScoreCEFn.apply(n, c, inv_t, mode, first_call, False, None, None, None, lq[0], lq[1], ent[0], ent[1])
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().clone(), out8.detach().clone(), n.grad.detach().clone(), c.grad.detach().clone(), rank.clone()


def _sums(n, c, inv_t, mode, ent, lq=(None, None)):
    """the entries' masked per-row sums (the forward _ScoreCEFn runs, called directly)"""
    from jodalrob_twotower_amd import ops
    B, D = n.shape
    e = ops.score_mask_ids(ent[0], ent[1], B, n.device)
    if mode == "fp32":
        return (ops.score_dir_fwd(n, c, inv_t, abs(inv_t), lq_b=lq[1], ent=e)[0], ops.score_dir_fwd(c, n, inv_t, abs(inv_t), lq_b=lq[0], ent=e)[0])
    sn = ops.score_unit_scale(inv_t)
    assert sn == unit_scale(inv_t)                           # the reference's operand scale is the library's
    Np, Cp = ops.score_pack2_bf16(n, c, sn, 1.0)
    r = ops.score_fwd_sym_mask(Np, Cp, B, D, inv_t, abs(inv_t), e, lq[0], lq[1], sn)
    return r[0], r[1]


def _check(B, D, T, pattern, mode, kind=None):
    inv_t = 1.0 / T
    n, c = _inputs(B, D)
    ent, lq = _ids(B, pattern), _lqs(B, D, kind)
    loss, out8, gn, gc, rank = _run(n, c, inv_t, mode, ent, lq)
    ref_loss, ref_gn, ref_gc, ref_rs, ref_cs = _ref(B, D, T, pattern, mode, kind)
    lb, gb = BOUNDS[mode]
    fl = inv_t / (2.0 * B)                                   # one unit row's full gradient weight: the floor where the gradient is ~0
    rs, cs = _sums(n, c, inv_t, mode, ent, lq)
    errs = [float(((got.double() - ref).abs() / ref).max()) for got, ref in ((rs, ref_rs), (cs, ref_cs))]
    print(f"mask {mode} B={B} D={D} T={T} {pattern} lq={kind}: loss {loss.item():.9g} ref {ref_loss:.9g}  nrel dN {_nrel(gn, ref_gn, fl):.3g} "
          f"dC {_nrel(gc, ref_gc, fl):.3g} (bound {gb:g})  sums {errs[0]:.3g} {errs[1]:.3g} (bound {_sum_rtol(mode, inv_t):.3g})")
    assert torch.isfinite(loss) and torch.isfinite(gn).all() and torch.isfinite(gc).all()
    assert abs(loss.item() - ref_loss) <= lb * abs(ref_loss) + LOSS_ATOL, (loss.item(), ref_loss)
    assert _nrel(gn, ref_gn, fl) <= gb, _nrel(gn, ref_gn, fl)
    assert _nrel(gc, ref_gc, fl) <= gb, _nrel(gc, ref_gc, fl)
    assert max(errs) <= _sum_rtol(mode, inv_t), errs
    # metrics (all of out8 but the loss) and the row ranks are the raw scores': bitwise the plain entry's
    _, out8_plain, _, _, rank_plain = _run(n, c, inv_t, mode)
    torch.testing.assert_close(out8[1:], out8_plain[1:], rtol=0, atol=0, equal_nan=True)     # (B = 1: the negative mean is nan)
    assert torch.equal(rank, rank_plain)
    return loss, gn, gc


# ---- 1. the node against f64 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("B,D,T", SHAPES)
@pytest.mark.parametrize("pattern", PATTERNS)
def test_mask_score_node_vs_f64(tt, mode, B, D, T, pattern):
    """(one_notice: every negative is masked -- the reference's loss and gradients are 0, and the bounds' absolute parts, LOSS_ATOL and
    the _nrel floor inv_t / 2B, are what the finite results are held to)"""
    _check(B, D, T, pattern, mode)


# ---- 2. mask and logQ together ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("B,D,T", [(33, 1, 0.5), (257, 64, 0.05), (2048, 128, 1.0)])
@pytest.mark.parametrize("pattern", ["groups", "tile_edge"])
@pytest.mark.parametrize("kind", ["random", "zipf"])
def test_mask_with_logq_vs_f64(tt, mode, B, D, T, pattern, kind):
    _check(B, D, T, pattern, mode, kind)


# ---- 3. the inert mask -----------------------------------------------------------------------------------------------------------
# The masked symmetric forward is the plain sweep with one more select per element, so the forward's outputs are the plain entry's
# bits at every shape.  The masked bf16 backward is always the b-split kernel on four waves: the plain dispatch picks that form (same
# waves, same tile order) at padded D = 256 only -- (257, 200, 2.0) -- and the transposing form or eight waves elsewhere (another
# summation tree: there test 1's f64 bounds apply).  The fp32 path has one form: identical at every shape.
INERT_BITWISE_GRADS = {("bf16", (257, 200, 2.0))} | {("fp32", s) for s in SHAPES}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("B,D,T", SHAPES)
def test_inert_mask_is_the_plain_entry(tt, mode, B, D, T):
    n, c = _inputs(B, D)
    masked = _run(n, c, 1.0 / T, mode, _ids(B, "distinct"))
    plain = _run(n, c, 1.0 / T, mode)
    assert torch.equal(masked[0], plain[0]) and torch.equal(masked[4], plain[4])
    torch.testing.assert_close(masked[1], plain[1], rtol=0, atol=0, equal_nan=True)
    if (mode, (B, D, T)) in INERT_BITWISE_GRADS:
        assert torch.equal(masked[2], plain[2]) and torch.equal(masked[3], plain[3])
    else:
        _, ref_gn, ref_gc, _, _ = _ref(B, D, T, "distinct", mode)
        fl = (1.0 / T) / (2.0 * B)
        assert _nrel(masked[2], ref_gn, fl) <= BOUNDS[mode][1] and _nrel(masked[3], ref_gc, fl) <= BOUNDS[mode][1]
    # one side alone: the other counts as all-distinct
    en, ec = _ids(B, "distinct")
    for ent in ((en, None), (None, ec)):
        one = _run(n, c, 1.0 / T, mode, ent)
        for a, b in zip(one, masked):
            torch.testing.assert_close(a, b, rtol=0, atol=0, equal_nan=True)


# ---- 4. reproducibility ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("B,D,T", [(257, 64, 0.05), (2048, 128, 1.0)])
def test_mask_runs_are_bit_identical(tt, mode, B, D, T):
    n, c = _inputs(B, D)
    for lq in ((None, None), _lqs(B, D, "zipf")):
        first = _run(n, c, 1.0 / T, mode, _ids(B, "groups"), lq)
        again = _run(n, c, 1.0 / T, mode, _ids(B, "groups"), lq)
        for a, b in zip(first, again):
            assert torch.equal(a, b)


def test_mask_first_call_diagnostic(tt):
    """The task's first call (want_col_rank): loss and gradients are the masked ones, out8[5] the plain first call's column top-1 rate"""
    B, D = 257, 64
    n, c = _inputs(B, D)
    for mode in MODES:
        first = _run(n, c, 1.0, mode, _ids(B, "groups"), first_call=True)
        later = _run(n, c, 1.0, mode, _ids(B, "groups"))
        for k in (0, 2, 3, 4):
            assert torch.equal(first[k], later[k])
        plain_first = _run(n, c, 1.0, mode, first_call=True)
        assert first[1][5].item() == plain_first[1][5].item() and first[1][1].item() == plain_first[1][1].item()


# ---- 5. wiring -------------------------------------------------------------------------------------------------------------------
def test_mask_eager_vs_step_vs_step_from_store(tt, tmp_path):
    """Dropout on, 1203 pairs in batches of 254 (4 full batches + a ragged one of 187), the loader attaching the entity ids
    (DevicePairLoader mask_repeats).  Three legs, bit for bit -- per-step losses, final weights -- as the logQ counterpart
    (test_gpu_logq.test_logq_eager_vs_step_vs_step_from_store): (a) the eager step, (b) GraphedTrainStep.step(batch), (c)
    DevicePairLoader.step_batches -> step_from_store.  The ragged batch goes through the eager step in every leg."""
    from jodalrob_twotower_amd.data_loader import create_unified_bid_dataloaders
    from jodalrob_twotower_amd.graph import GraphedTrainStep
    from jodalrob_twotower_amd.optim import FusedAdam
    M64 = (1 << 64) - 1
    base = 0x5DEECE66D
    P, B = 1203, 254
    meta, schema, source = _pair_world(tt, tmp_path, P)
    finals, words_of = {}, {}
    for mode in ("tensors", "store", "eager"):
        torch.manual_seed(123)
        train_loader, _ = create_unified_bid_dataloaders(source(), schema, batch_size=B, test_split=0.0, shuffle_seed=7,
                                                         test_mode=True, pair_limit=P, device=DEV)
        train_loader.set_mask_repeats(True)
        first = next(iter(train_loader))
        # the batches' entity ids are the pair table's columns, and this world repeats notices inside a batch
        order = train_loader.epoch_order()
        ent = train_loader.epoch_entity(order)
        for k, lo in enumerate(range(0, P, B)):
            m = min(B, P - lo)
            b = train_loader.batch(order, lo)
            sel = train_loader.pairs[order[lo:lo + m]]
            for side, s in (("notice", 0), ("company", 1)):
                assert b[side]["entity"].dtype == torch.int32 and torch.equal(b[side]["entity"], sel[:, s].to(torch.int32))
                assert torch.equal(ent[k, s, :m], b[side]["entity"]) and ent[k, s, :m].data_ptr() % 16 == 0
        assert first["notice"]["entity"].unique().numel() < B
        train_loader._gen.manual_seed(7)
        task = tt.create_two_tower_train_task(schema.notice.categorical, schema.company.categorical, metadata_path=str(meta),
                                              categorical_embedding_dim=16, notice_dense_input_dim=first["notice"]["dense"].shape[1],
                                              company_dense_input_dim=first["company"]["dense"].shape[1], tower_hidden_dims=[64, 32],
                                              final_embedding_dim=32, dropout_rate=0.1, device=DEV, embedding_grad="sparse",
                                              score_dtype="bf16", mlp_dtype="bf16")
        torch.manual_seed(0)
        with torch.no_grad():
            for p in task.parameters():
                p.copy_(0.05 * torch.randn(p.shape, device=DEV))
        task.train()
        task._pair_check_done = True
        towers = (task.two_tower_model.notice_tower, task.two_tower_model.company_tower)
        for tw in towers:
            tw._seed_override = base
        opt = FusedAdam.for_task(task, lr=1e-2, weight_decay=1e-5)
        torch.manual_seed(99)                                            # the replays' device seed words draw from it
        gs = GraphedTrainStep(task, opt, first, warmup=1) if mode != "eager" else None

        def eager(b, word=None):
            for tw in towers:
                tw._seed_override = base if word is None else (base + word) & M64
            opt.zero_grad()
            r = task(b, return_metrics=True)
            r["loss"].backward()
            opt.step()
            return r
        losses, words = [], []
        if mode == "store":
            for r in train_loader.step_batches(gs, eager):
                losses.append(r["loss"].item())
                if r is gs.result:
                    words.append(int(gs._seed_dev.item()) & M64)
        else:
            for b in train_loader:
                full = b["notice"]["dense"].shape[0] == B
                if mode == "tensors" and full:
                    r = gs.step(b)
                    losses.append(r["loss"].item())
                    words.append(int(gs._seed_dev.item()) & M64)
                elif mode == "eager" and full:
                    w = words_of["tensors"][len(words)]
                    losses.append(eager(b, w)["loss"].item())
                    words.append(w)
                else:
                    losses.append(eager(b)["loss"].item())
        torch.cuda.synchronize()
        assert len(losses) == 5 and len(words) == 4
        words_of[mode] = words
        finals[mode] = (losses, {k: v.detach().cpu().clone() for k, v in task.state_dict().items()})
        if mode == "eager":
            # on the same batch the masked loss differs from the unmasked one
            task.eval()
            with torch.no_grad():
                plain = {s: {k: v for k, v in first[s].items() if k != "entity"} for s in ("notice", "company")}
                assert task(first).item() != task(plain).item()
        if gs is not None:
            # a step captured with entity ids refuses a batch (or a store step) without them
            with pytest.raises(ValueError, match="entity mismatch"):
                gs.step({s: {k: v for k, v in first[s].items() if k != "entity"} for s in ("notice", "company")})
            with pytest.raises(ValueError, match="entity mismatch"):
                gs.step_from_store(train_loader.notice, train_loader.company, train_loader.pairs, None, 0)
            gs.close()
    assert words_of["tensors"] == words_of["store"]
    for mode in ("store", "eager"):
        assert finals[mode][0] == finals["tensors"][0], (mode, finals[mode][0], finals["tensors"][0])
        for k, v in finals["tensors"][1].items():
            assert torch.equal(v, finals[mode][1][k]), (mode, k)


def _small_task(tt, manifest, B=64, **kw):
    from params_init import init_state_numpy, synth_batch_numpy
    cfg = dict(manifest["cases"]["wide_b40"])
    cfg["B"] = B
    task = make_task(tt, cfg, embedding_grad="sparse", mlp_dtype="fp32", **kw)
    shapes = {k: tuple(v.shape) for k, v in task.state_dict().items()}
    load_state(task, init_state_numpy(shapes, 77))
    task.train()
    task._pair_check_done = True
    b = to_batch(tt, synth_batch_numpy(cfg["B"], cfg["vocab_n"], cfg["vocab_c"], cfg["din_n"], cfg["din_c"], 610, oob=False),
                 cfg["keys_n"], cfg["keys_c"])
    return task, b, cfg["B"]


def test_step_captured_without_entity_refuses_a_batch_with_it(tt, manifest):
    from jodalrob_twotower_amd.graph import GraphedTrainStep
    from jodalrob_twotower_amd.optim import FusedAdam
    task, b, B = _small_task(tt, manifest, score_dtype="bf16")
    gs = GraphedTrainStep(task, FusedAdam.for_task(task, lr=1e-2), b, warmup=1)
    ent = ids(B, "groups", device=DEV)
    with_ent = {"notice": dict(b["notice"], entity=ent[0]), "company": dict(b["company"], entity=ent[1])}
    with pytest.raises(ValueError, match="entity mismatch"):
        gs.step(with_ent)
    gs.step(b)
    gs.close()


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------
def test_mask_refusals(tt, manifest):
    from jodalrob_twotower_amd import ops
    B, D = 64, 32
    n, c = _unit_rows(B, D, 1), _unit_rows(B, D, 2)
    ent = ids(B, "groups", device=DEV)
    for mode in ("fp8", "bf16x3"):
        with pytest.raises(ValueError, match=mode):
            _run(n, c, 1.0, mode, ent)
    # the task: score dtypes, the dense loss path, dtype / shape / device of the arrays
    task, b, Bt = _small_task(tt, manifest, score_dtype="bf16")
    e = ids(Bt, "groups", device=DEV)

    def batch(en, ec):
        return {"notice": dict(b["notice"], entity=en), "company": dict(b["company"], entity=ec)}
    for sd in ("fp8", "bf16x3"):
        task.score_dtype = sd
        with pytest.raises(ValueError, match=sd):
            task(batch(*e))
    task.score_dtype = "bf16"
    for dense in (tt.TwoTowerTrainTask(task.two_tower_model, label_smoothing=0.1, score_dtype="bf16"),
                  tt.TwoTowerTrainTask(task.two_tower_model, loss_type="cosine_embedding", score_dtype="bf16")):
        with pytest.raises(ValueError, match="dense loss"):
            dense(batch(*e))
    with pytest.raises(ValueError, match="int32"):
        task(batch(e[0].long(), e[1]))
    with pytest.raises(ValueError, match="int32"):
        task(batch(e[0], e[1].float()))
    with pytest.raises(ValueError, match="shape"):
        task(batch(e[0][:-1], e[1]))
    with pytest.raises(ValueError, match="shape"):
        task(batch(e[0], e[1].reshape(Bt, 1)))
    with pytest.raises(ValueError, match="is on cpu"):
        task(batch(e[0].cpu(), e[1]))
    assert torch.isfinite(task(batch(e[0], None)))            # one side alone is served
    # the C entries: square problems only, the logQ temperature limit carries over
    e64 = ops.score_mask_ids(ent[0], ent[1], B, n.device)
    with pytest.raises(Exception, match="square"):
        ops.score_dir_fwd(n, c[:48].contiguous(), 1.0, 1.0, ent=e64)
    with pytest.raises(Exception, match="square"):
        ops.score_dir_fwd(n, c, 1.0, 1.0, diag_offset=1, ent=e64)
    lq = _lq(B, "random", 3)
    with pytest.raises(ValueError, match="2/T"):
        _run(n, c, 1.0 / 0.049, "bf16", ent, (lq, lq))
    Np, Cp = ops.score_pack2_bf16(n, c, 1.0, 1.0)
    with pytest.raises(Exception, match="2/T"):
        ops.score_fwd_sym_mask(Np, Cp, B, D, 1.0 / 0.049, 1.0 / 0.049, e64, lq, lq)
    with pytest.raises(Exception, match="2/T"):
        ops.score_dir_fwd(n, c, 1.0 / 0.049, 1.0 / 0.049, lq_b=lq, ent=e64)
    _run(n, c, 1.0 / 0.049, "bf16", ent)                     # without logQ the plain limit (2/T <= 80) holds
    _run(n, c, 1.0 / 0.05, "bf16", ent, (lq, lq))            # 2/T = 40 with logQ is supported
