"""Per-pair sample weights of the in-batch softmax on the MI355X (include/twotower.h *_pw entries).

1. The score node (_ScoreCEFn with pair_w) against the float64 reference of tests/_pair_weight_reference.py, fed the kernels' own
   operand rounding: bf16 and fp32, ragged shapes, six weight patterns; the folded reciprocals g / sum and the unweighted sums;
   metrics and ranks bitwise the plain call's.
2. Weights with the logQ correction and with the repeated-entity mask.
3. All-ones weights: loss, sums and metrics are the plain entry's bits.  All-zero weights: loss and gradients exactly 0.
4. Scaling every weight by a power of two changes no bit; runs are bitwise reproducible.
5. Wiring: eager task, GraphedTrainStep.step and step_from_store fed by DevicePairLoader(pair_weight=) agree bit for bit over three
   steps with different weights; a captured step refuses a batch whose pair weights do not match its capture.
6. Refusals: fp8, bf16x3, the dense loss, wrong dtype / shape / device, rectangular problems, missing folded reciprocals.

Bounds: those tests/test_gpu_logq.py holds the same mode to (imported), as tests/test_gpu_mask_repeats.py does.  They carry over: g is
B / sum(w') times w', three f32 roundings and a fixed-order sum of positive terms away from the f64 value (relative error at most
(ceil(B / 1024) + 24) * 2^-24 = 1.6e-6 at B = 2048, far inside the gradients' bounds; in the loss it multiplies every pair's term, so
the weighted mean moves by at most that fraction of itself, inside the loss bound's 2e-6 + 2^-18).  The sums are the unweighted ones, so
_sum_rtol holds as it stands.  The one quantity with no bound of its own yet is the folded reciprocal g_i / sum_i: the sum's bound
plus g's rounding above plus the reciprocal's and the product's roundings -- _inv_rtol, derived here and in DESIGN.md 8e, measured
against the f64 reference.
"""
import functools
import math

import pytest
import torch

from test_gpu_parity import DEV, tt, ctx_option, make_task, to_batch, load_state  # noqa: F401
from test_gpu_logq import BOUNDS, LOSS_ATOL, _sum_rtol, _nrel, _lq, _unit_rows, _pair_world
from _mask_reference import ids, unit_scale
from _pair_weight_reference import PATTERNS, normalise, reference, ref_sums, weights

pytestmark = pytest.mark.gpu

SHAPES = [(1, 32, 1.0), (33, 1, 0.5), (65, 64, 0.05), (257, 200, 2.0), (257, 64, 0.05), (2048, 128, 1.0),
          (97, 96, 1.0)]                              # (the 65..128 class of D at a ragged B: four tiles, the last one partial)
COMBO_SHAPES = [(33, 1, 0.5), (257, 64, 0.05), (2048, 128, 1.0)]
MODES = ["bf16", "fp32"]


def _inv_rtol(mode, inv_t, B):
    """folded reciprocal g_i / sum_i against f64: the sum's own bound, plus g = w' * (B / total) -- the total's fixed-order sum of
    positive terms (ceil(B / 1024) adds per thread, 6 butterfly rounds, 16 wave sums: each a relative 2^-24 at most), the division
    and the product -- plus the reciprocal 1 / sum and the product g * (1 / sum): (ceil(B / 1024) + 26) roundings of 2^-24"""
    return _sum_rtol(mode, inv_t) + (math.ceil(B / 1024) + 26) * 2.0 ** -24


@functools.lru_cache(maxsize=None)
def _inputs(B, D):
    return _unit_rows(B, D, 11 + B + D), _unit_rows(B, D, 29 + B + D)


@functools.lru_cache(maxsize=None)
def _w(B, pattern):
    return weights(B, pattern, seed=B, device=DEV)


@functools.lru_cache(maxsize=None)
def _ids(B, idp):
    return (None, None) if idp is None else ids(B, idp, seed=B, device=DEV)


@functools.lru_cache(maxsize=None)
def _lqs(B, D, kind):
    return (None, None) if kind is None else (_lq(B, kind, 3 + B), _lq(B, kind, 5 + D))


@functools.lru_cache(maxsize=None)
def _ref(B, D, T, pattern, mode, kind=None, idp=None):
    """(loss, dN, dC, rowsum, colsum, g) in f64: computed once per case, shared, never written to"""
    n, c = _inputs(B, D)
    en, ec = _ids(B, idp)
    lq_n, lq_c = _lqs(B, D, kind)
    return reference(n, c, 1.0 / T, _w(B, pattern), mode, en, ec, lq_n, lq_c) + ref_sums(n, c, 1.0 / T, mode, en, ec, lq_n, lq_c) \
        + (normalise(_w(B, pattern)),)


def _run(n, c, inv_t, mode, w=None, ent=(None, None), lq=(None, None), first_call=False):
    from jodalrob_twotower_amd.two_tower_train_task import _ScoreCEFn
    n = n.clone().requires_grad_(True)
    c = c.clone().requires_grad_(True)
    loss, out8, rank = _ScoreCEFn.apply(n, c, inv_t, mode, first_call, False, None, None, None, lq[0], lq[1], ent[0], ent[1], w)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().clone(), out8.detach().clone(), n.grad.detach().clone(), c.grad.detach().clone(), rank.clone()


def _fwd(n, c, inv_t, mode, w, ent=(None, None), lq=(None, None)):
    """(rowsum, colsum, inv or None, g): the forward _ScoreCEFn runs, called directly.  fp32: the unchanged directional forwards (the
    sums are unweighted) -- that path has no reciprocal arrays."""
    from jodalrob_twotower_amd import ops
    B, D = n.shape
    g = ops.score_pair_weights(w, B, n.device)
    e = None if ent[0] is None and ent[1] is None else ops.score_mask_ids(ent[0], ent[1], B, n.device)
    if mode == "fp32":
        return (ops.score_dir_fwd(n, c, inv_t, abs(inv_t), lq_b=lq[1], ent=e)[0], ops.score_dir_fwd(c, n, inv_t, abs(inv_t), lq_b=lq[0], ent=e)[0],
                None, g)
    sn = ops.score_unit_scale(inv_t)
    assert sn == unit_scale(inv_t)                           # the reference's operand scale is the library's
    Np, Cp = ops.score_pack2_bf16(n, c, sn, 1.0)
    r = ops.score_fwd_sym_pw(Np, Cp, B, D, inv_t, abs(inv_t), g, e, lq[0], lq[1], sn)
    return r[0], r[1], r[4], g


def _check(B, D, T, pattern, mode, kind=None, idp=None):
    inv_t = 1.0 / T
    n, c = _inputs(B, D)
    w, ent, lq = _w(B, pattern), _ids(B, idp), _lqs(B, D, kind)
    loss, out8, gn, gc, rank = _run(n, c, inv_t, mode, w, ent, lq)
    ref_loss, ref_gn, ref_gc, ref_rs, ref_cs, ref_g = _ref(B, D, T, pattern, mode, kind, idp)
    lb, gb = BOUNDS[mode]
    fl = inv_t / (2.0 * B)                                   # one unit row's full gradient weight: the floor where the gradient is ~0
    rs, cs, inv, g = _fwd(n, c, inv_t, mode, w, ent, lq)
    errs = [float(((got.double() - ref).abs() / ref).max()) for got, ref in ((rs, ref_rs), (cs, ref_cs))]
    # g: [round_up(B, 64)], zero past B, zero exactly where the reference's is, a few roundings from it elsewhere
    assert g.shape[0] == (B + 63) // 64 * 64 and not g[B:].any()
    nz = ref_g > 0
    assert torch.equal(g[:B] > 0, nz)
    g_err = float(((g[:B].double() - ref_g).abs()[nz] / ref_g[nz]).max()) if nz.any() else 0.0
    inv_err = 0.0
    if inv is not None:
        # the stored reciprocals are of the sums as accumulated: the returned sums carry the factor exp(-1/T) (unit-scaled operands)
        for got, ref_sum in ((inv[0], ref_rs), (inv[1], ref_cs)):
            ref_inv = ref_g / (ref_sum * math.exp(abs(inv_t)))
            assert torch.equal(got > 0, nz) and not got[~nz].any()
            if nz.any():
                inv_err = max(inv_err, float(((got.double() - ref_inv).abs()[nz] / ref_inv[nz]).max()))
    print(f"pw {mode} B={B} D={D} T={T} {pattern} lq={kind} ids={idp}: loss {loss.item():.9g} ref {ref_loss:.9g}  nrel dN {_nrel(gn, ref_gn, fl):.3g} "
          f"dC {_nrel(gc, ref_gc, fl):.3g} (bound {gb:g})  sums {errs[0]:.3g} {errs[1]:.3g} (bound {_sum_rtol(mode, inv_t):.3g})  "
          f"g {g_err:.3g}  inv {inv_err:.3g} (bound {_inv_rtol(mode, inv_t, B):.3g})")
    assert torch.isfinite(loss) and torch.isfinite(gn).all() and torch.isfinite(gc).all()
    assert abs(loss.item() - ref_loss) <= lb * abs(ref_loss) + LOSS_ATOL, (loss.item(), ref_loss)
    assert _nrel(gn, ref_gn, fl) <= gb, _nrel(gn, ref_gn, fl)
    assert _nrel(gc, ref_gc, fl) <= gb, _nrel(gc, ref_gc, fl)
    assert max(errs) <= _sum_rtol(mode, inv_t), errs
    assert g_err <= (math.ceil(B / 1024) + 24) * 2.0 ** -24, g_err
    assert inv_err <= _inv_rtol(mode, inv_t, B), inv_err
    # metrics (all of out8 but the loss) and the row ranks are the raw scores': bitwise the plain entry's
    _, out8_plain, _, _, rank_plain = _run(n, c, inv_t, mode)
    torch.testing.assert_close(out8[1:], out8_plain[1:], rtol=0, atol=0, equal_nan=True)     # (B = 1: the negative mean is nan)
    assert torch.equal(rank, rank_plain)
    if not nz.any():                                         # no positive weight at all: exactly nothing
        assert loss.item() == 0.0 and not gn.any() and not gc.any()
    return loss, gn, gc


# ---- 1. the node against f64 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("B,D,T", SHAPES)
@pytest.mark.parametrize("pattern", PATTERNS)
def test_pw_score_node_vs_f64(tt, mode, B, D, T, pattern):
    _check(B, D, T, pattern, mode)


# ---- 2. with the logQ correction and the repeated-entity mask --------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("B,D,T", COMBO_SHAPES)
@pytest.mark.parametrize("kind,idp", [("random", None), ("zipf", None), (None, "groups"), (None, "tile_edge"), ("random", "groups"),
                                      ("zipf", "tile_edge"), ("random", "tile_edge"), ("zipf", "groups")])
@pytest.mark.parametrize("pattern", ["random", "edge_zeros"])
def test_pw_with_logq_and_mask_vs_f64(tt, mode, B, D, T, kind, idp, pattern):
    _check(B, D, T, pattern, mode, kind, idp)


# ---- 3. all-ones and all-zero weights --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("B,D,T", SHAPES)
def test_ones_are_the_plain_entry(tt, mode, B, D, T):
    """g = 1 exactly (B / B), and every product with it is exact: loss, sums and metrics are the plain entry's bits.  The gradients are
    held to the mode's f64 bound: the plain entry may run another backward form (another summation tree)."""
    from jodalrob_twotower_amd import ops
    inv_t = 1.0 / T
    n, c = _inputs(B, D)
    ones = _w(B, "ones")
    got = _run(n, c, inv_t, mode, ones)
    plain = _run(n, c, inv_t, mode)
    assert torch.equal(got[0], plain[0]) and torch.equal(got[4], plain[4])
    torch.testing.assert_close(got[1], plain[1], rtol=0, atol=0, equal_nan=True)
    rs, cs, inv, g = _fwd(n, c, inv_t, mode, ones)
    assert torch.equal(g[:B], torch.ones(B, device=DEV))
    if mode == "bf16":
        sn = ops.score_unit_scale(inv_t)
        Np, Cp = ops.score_pack2_bf16(n, c, sn, 1.0)
        p = ops.score_fwd_sym(Np, Cp, B, D, inv_t, abs(inv_t), sn)
        assert torch.equal(rs, p[0]) and torch.equal(cs, p[1]) and torch.equal(inv[0], p[4][0]) and torch.equal(inv[1], p[4][1])
    _, ref_gn, ref_gc, _, _, _ = _ref(B, D, T, "ones", mode)
    fl = inv_t / (2.0 * B)
    assert _nrel(got[2], ref_gn, fl) <= BOUNDS[mode][1] and _nrel(got[3], ref_gc, fl) <= BOUNDS[mode][1]
    # the same with the mask and the logQ correction on: the masked / corrected entries' loss and metrics
    if (B, D, T) in COMBO_SHAPES:
        ent, lq = _ids(B, "groups"), _lqs(B, D, "zipf")
        a, b = _run(n, c, inv_t, mode, ones, ent, lq), _run(n, c, inv_t, mode, None, ent, lq)
        assert torch.equal(a[0], b[0]) and torch.equal(a[4], b[4])
        torch.testing.assert_close(a[1], b[1], rtol=0, atol=0, equal_nan=True)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("B,D,T", SHAPES)
def test_all_zero_weights_give_exactly_nothing(tt, mode, B, D, T):
    n, c = _inputs(B, D)
    for ent, lq in (((None, None), (None, None)), (_ids(B, "groups"), _lqs(B, D, "random"))):
        if lq[0] is not None and 2.0 / T > 40.0:
            continue
        loss, out8, gn, gc, _ = _run(n, c, 1.0 / T, mode, _w(B, "all_zero"), ent, lq)
        assert loss.item() == 0.0 and out8[0].item() == 0.0
        assert not gn.any() and not gc.any()


# ---- 4. power-of-two scaling, reproducibility --------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("B,D,T", [(65, 64, 0.05), (257, 64, 0.05), (2048, 128, 1.0)])
@pytest.mark.parametrize("pattern", ["random", "dirty"])
def test_power_of_two_scaling_changes_no_bit(tt, mode, B, D, T, pattern):
    """the sum is taken in one fixed order and B / sum scales exactly: g itself is bit-identical, and with it every output"""
    from jodalrob_twotower_amd import ops
    n, c = _inputs(B, D)
    w = _w(B, pattern)
    for ent, lq in (((None, None), (None, None)), (_ids(B, "groups"), _lqs(B, D, "zipf"))):
        first = _run(n, c, 1.0 / T, mode, w, ent, lq)
        for k in (8.0, 0.25, 1.0):                           # (1.0: the same call again)
            assert torch.equal(ops.score_pair_weights(w * k, B, n.device), ops.score_pair_weights(w, B, n.device))
            again = _run(n, c, 1.0 / T, mode, w * k, ent, lq)
            for a, b in zip(first, again):
                torch.testing.assert_close(a, b, rtol=0, atol=0, equal_nan=True)


def test_pw_first_call_diagnostic(tt):
    """The task's first call (want_col_rank): loss and gradients are the weighted ones, out8[5] the plain first call's column top-1 rate"""
    B, D = 257, 64
    n, c = _inputs(B, D)
    for mode in MODES:
        first = _run(n, c, 1.0, mode, _w(B, "random"), first_call=True)
        later = _run(n, c, 1.0, mode, _w(B, "random"))
        for k in (0, 2, 3, 4):
            assert torch.equal(first[k], later[k])
        plain_first = _run(n, c, 1.0, mode, first_call=True)
        assert first[1][5].item() == plain_first[1][5].item() and first[1][1].item() == plain_first[1][1].item()


# ---- 5. wiring -------------------------------------------------------------------------------------------------------------------
def _adam_state(task, opt):
    """the moments by parameter name (the optimiser creates its state entries in the order it first meets the gradients)"""
    return {f"{name}.{key}": v.detach().cpu().clone() for name, p in task.named_parameters() if p in opt.state
            for key, v in opt.state[p].items() if key != "step" and torch.is_tensor(v)}


def test_pw_eager_vs_step_vs_step_from_store(tt, tmp_path):
    """Dropout on, 762 pairs in three full batches of 254, the loader attaching each batch's slice of a per-pair weight table (so every
    step has other weights), with the repeated-entity mask on as train.py combines them.  Three legs, bit for bit -- per-step out8, final
    weights, Adam state -- as test_gpu_mask_repeats.test_mask_eager_vs_step_vs_step_from_store: (a) the eager step, (b)
    GraphedTrainStep.step(batch), (c) DevicePairLoader.step_batches -> step_from_store."""
    from jodalrob_twotower_amd.data_loader import create_unified_bid_dataloaders
    from jodalrob_twotower_amd.graph import GraphedTrainStep
    from jodalrob_twotower_amd.optim import FusedAdam
    from jodalrob_twotower_amd.pair_weights import inverse_count_weights
    M64 = (1 << 64) - 1
    base = 0x5DEECE66D
    P, B = 762, 254
    meta, schema, source = _pair_world(tt, tmp_path, P)
    finals, words_of = {}, {}
    for mode in ("tensors", "store", "eager"):
        torch.manual_seed(123)
        train_loader, _ = create_unified_bid_dataloaders(source(), schema, batch_size=B, test_split=0.0, shuffle_seed=7,
                                                         test_mode=True, pair_limit=P, device=DEV)
        train_loader.set_mask_repeats(True)
        pw = (inverse_count_weights(train_loader.pairs) * weights(P, "edge_zeros", seed=5, device=DEV)).contiguous()
        train_loader.set_pair_weight(pw)
        first = next(iter(train_loader))
        # the batches' weights are the table's rows of the batch's pairs; the per-epoch array's slices are 16-byte aligned
        order = train_loader.epoch_order()
        arr = train_loader.epoch_pair_weight(order)
        for k, lo in enumerate(range(0, P, B)):
            b = train_loader.batch(order, lo)
            assert b["pair_weight"].dtype == torch.float32 and torch.equal(b["pair_weight"], pw[order[lo:lo + B]])
            assert torch.equal(arr[k, :B], b["pair_weight"]) and arr[k, :B].data_ptr() % 16 == 0
        assert not torch.equal(arr[0], arr[1]) and (first["pair_weight"] == 0).any()
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
        outs, words = [], []
        if mode == "store":
            for r in train_loader.step_batches(gs, eager):
                outs.append(r.out8.detach().cpu().clone())
                words.append(int(gs._seed_dev.item()) & M64)
        else:
            for b in train_loader:
                if mode == "tensors":
                    outs.append(gs.step(b).out8.detach().cpu().clone())
                    words.append(int(gs._seed_dev.item()) & M64)
                else:
                    w = words_of["tensors"][len(words)]
                    outs.append(eager(b, w).out8.detach().cpu().clone())
                    words.append(w)
        torch.cuda.synchronize()
        assert len(outs) == 3 and len(words) == 3
        words_of[mode] = words
        finals[mode] = (outs, {k: v.detach().cpu().clone() for k, v in task.state_dict().items()}, _adam_state(task, opt))
        if mode == "eager":
            # on the same batch the weighted loss differs from the unweighted one
            task.eval()
            with torch.no_grad():
                assert task(first).item() != task({k: v for k, v in first.items() if k != "pair_weight"}).item()
        if gs is not None:
            # a step captured with pair weights refuses a batch (or a store step) without them
            ent = (first["notice"]["entity"], first["company"]["entity"])
            with pytest.raises(ValueError, match="pair_weight mismatch"):
                gs.step({k: v for k, v in first.items() if k != "pair_weight"})
            with pytest.raises(ValueError, match="pair_weight mismatch"):
                gs.step_from_store(train_loader.notice, train_loader.company, train_loader.pairs, None, 0, entity=ent)
            gs.close()
    assert words_of["tensors"] == words_of["store"]
    for mode in ("store", "eager"):
        for a, b in zip(finals[mode][0], finals["tensors"][0]):
            assert torch.equal(a, b), (mode, a, b)
        for k, v in finals["tensors"][1].items():
            assert torch.equal(v, finals[mode][1][k]), (mode, k)
        assert finals[mode][2].keys() == finals["tensors"][2].keys() and len(finals[mode][2]) > 0
        for k, v in finals["tensors"][2].items():
            assert torch.equal(v, finals[mode][2][k]), (mode, k)


def _small_task(tt, manifest, **kw):
    from params_init import init_state_numpy, synth_batch_numpy
    cfg = dict(manifest["cases"]["wide_b40"])
    cfg["B"] = 64
    task = make_task(tt, cfg, embedding_grad="sparse", mlp_dtype="fp32", **kw)
    shapes = {k: tuple(v.shape) for k, v in task.state_dict().items()}
    load_state(task, init_state_numpy(shapes, 77))
    task.train()
    task._pair_check_done = True
    b = to_batch(tt, synth_batch_numpy(cfg["B"], cfg["vocab_n"], cfg["vocab_c"], cfg["din_n"], cfg["din_c"], 610, oob=False),
                 cfg["keys_n"], cfg["keys_c"])
    return task, b, cfg["B"]


def test_step_captured_without_pair_weight_refuses_a_batch_with_it(tt, manifest):
    from jodalrob_twotower_amd.graph import GraphedTrainStep
    from jodalrob_twotower_amd.optim import FusedAdam
    task, b, B = _small_task(tt, manifest, score_dtype="bf16")
    gs = GraphedTrainStep(task, FusedAdam.for_task(task, lr=1e-2), b, warmup=1)
    with pytest.raises(ValueError, match="pair_weight mismatch"):
        gs.step(dict(b, pair_weight=_w(B, "random")))
    gs.step(b)
    gs.close()


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------
def test_pw_refusals(tt, manifest):
    from jodalrob_twotower_amd import ops
    B, D = 64, 32
    n, c = _unit_rows(B, D, 1), _unit_rows(B, D, 2)
    w = _w(B, "random")
    for mode in ("fp8", "bf16x3"):
        with pytest.raises(ValueError, match=mode):
            _run(n, c, 1.0, mode, w)
    # the task: score dtypes, the dense loss path, dtype / shape / device of the array; forward_with_ranks
    task, b, Bt = _small_task(tt, manifest, score_dtype="bf16")
    wt = _w(Bt, "random")
    for sd in ("fp8", "bf16x3"):
        task.score_dtype = sd
        with pytest.raises(ValueError, match=sd):
            task(dict(b, pair_weight=wt))
    task.score_dtype = "bf16"
    for dense in (tt.TwoTowerTrainTask(task.two_tower_model, label_smoothing=0.1, score_dtype="bf16"),
                  tt.TwoTowerTrainTask(task.two_tower_model, loss_type="cosine_embedding", score_dtype="bf16")):
        with pytest.raises(ValueError, match="dense loss"):
            dense(dict(b, pair_weight=wt))
    with pytest.raises(ValueError, match="float32"):
        task(dict(b, pair_weight=wt.double()))
    with pytest.raises(ValueError, match="shape"):
        task(dict(b, pair_weight=wt[:-1]))
    with pytest.raises(ValueError, match="shape"):
        task(dict(b, pair_weight=wt.reshape(Bt, 1)))
    with pytest.raises(ValueError, match="is on cpu"):
        task(dict(b, pair_weight=wt.cpu()))
    with pytest.raises(ValueError, match="pair_weight"):
        task.forward_with_ranks(dict(b, pair_weight=wt))
    assert torch.isfinite(task(dict(b, pair_weight=wt)))
    # the C entries: square problems only, the folded reciprocals are required, the logQ temperature limit carries over
    g = ops.score_pair_weights(w, B, n.device)
    ones = torch.ones(B, device=DEV)
    d1 = torch.ones(1, device=DEV)
    with pytest.raises(Exception, match="square"):
        ops.score_dir_bwd(n, c[:48].contiguous(), 1.0, 1.0, 0, ones, ones[:48].contiguous(), d1, 1.0, pw=g)
    with pytest.raises(Exception, match="square"):
        ops.score_dir_bwd(n, c, 1.0, 1.0, 1, ones, ones, d1, 1.0, pw=g)
    Np, Cp = ops.score_pack2_bf16(n, c, 1.0, 1.0)
    r = ops.score_fwd_sym_pw(Np, Cp, B, D, 1.0, 1.0, g)
    with pytest.raises(ValueError, match="folded reciprocals"):
        ops.score_bwd_bf16(Np, Cp, B, D, 1.0, 1.0, r[0], r[1], d1, 1.0, pw=g)
    lq = _lq(B, "random", 3)
    with pytest.raises(ValueError, match="2/T"):
        _run(n, c, 1.0 / 0.049, "bf16", w, lq=(lq, lq))
    with pytest.raises(Exception, match="2/T"):
        ops.score_fwd_sym_pw(Np, Cp, B, D, 1.0 / 0.049, 1.0 / 0.049, g, None, lq, lq)
    _run(n, c, 1.0 / 0.049, "bf16", w)                       # without logQ the plain limit (2/T <= 80) holds
    _run(n, c, 1.0 / 0.05, "bf16", w, lq=(lq, lq))           # 2/T = 40 with logQ is supported
