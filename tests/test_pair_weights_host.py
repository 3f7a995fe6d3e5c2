"""Host-side tests of the per-pair sample weights: the f64 reference (tests/_pair_weight_reference.py) against autograd of the weighted
mean sum(w' l) / sum(w'), the C entries declared, bound and exported, DevicePairLoader's weight arrays, inverse_count_weights, and
the refusals that need no device."""
import ctypes
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import ROOT
from jodalrob_twotower_amd import _lib
from _mask_reference import ids
from _pair_weight_reference import PATTERNS, _mask, normalise, reference, weighted_mean_loss, weights

PW_SYMBOLS = ("tt_score_prepare_pw", "tt_score_fwd_sym_bf16_pw", "tt_score_bwd_bf16_pw", "tt_score_loss_finish_pw", "tt_score_dir_bwd_pw")


def _unit_rows(B, D, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, D, generator=g)
    return x / x.norm(dim=1, keepdim=True)


@pytest.mark.parametrize("B", [1, 33, 65])
@pytest.mark.parametrize("with_lq", [False, True])
@pytest.mark.parametrize("with_mask", [False, True])
@pytest.mark.parametrize("pattern", PATTERNS)
def test_reference_equals_autograd(B, with_lq, with_mask, pattern):
    """the closed form (loss, W C, W^T N) against autograd of the weighted mean of the pairs' terms in f64: 1e-12"""
    D, inv_t = 16, 1.0 / 0.3
    n, c = _unit_rows(B, D, 3 + B), _unit_rows(B, D, 5 + B)
    ent_n, ent_c = ids(B, "groups", seed=B) if with_mask else (None, None)
    g = torch.Generator().manual_seed(9)
    lq_n = (-45.0 * torch.rand(B, generator=g)) if with_lq else None          # (some below the clamp)
    lq_c = (-45.0 * torch.rand(B, generator=g)) if with_lq else None
    w = weights(B, pattern, seed=B)
    loss, dN, dC = reference(n, c, inv_t, w, "fp32", ent_n, ent_c, lq_n, lq_c)
    A = n.double().requires_grad_(True)
    Bm = c.double().requires_grad_(True)
    auto = weighted_mean_loss((A @ Bm.T) * inv_t, _mask(B, ent_n, ent_c, A.device), w, lq_n, lq_c)
    auto.backward()
    assert abs(loss - auto.item()) <= 1e-12 * max(1.0, abs(auto.item()))
    assert (dN - A.grad).abs().max().item() <= 1e-12 and (dC - Bm.grad).abs().max().item() <= 1e-12
    assert torch.isfinite(dN).all() and torch.isfinite(dC).all() and np.isfinite(loss)
    gw = normalise(w)
    if gw.sum().item() == 0:                                 # all_zero, or dirty at B = 1: exactly nothing
        assert loss == 0.0 and dN.abs().max().item() == 0.0 and dC.abs().max().item() == 0.0
    else:
        assert abs(gw.sum().item() - B) <= 1e-12 * B


def test_normalise_definition():
    w = torch.tensor([2.0, -1.0, float("nan"), float("inf"), 0.0, 6.0, -float("inf")], dtype=torch.float32)
    g = normalise(w)
    assert torch.equal(g, torch.tensor([7 * 2.0 / 8.0, 0, 0, 0, 0, 7 * 6.0 / 8.0, 0], dtype=torch.float64))
    assert torch.equal(normalise(torch.zeros(5)), torch.zeros(5, dtype=torch.float64))
    assert torch.equal(normalise(8.0 * w), g) and torch.equal(normalise(0.25 * w), g)
    # all-ones weights are the plain loss
    B = 33
    n, c = _unit_rows(B, 8, 1), _unit_rows(B, 8, 2)
    from _mask_reference import reference as mask_reference
    en, ec = ids(B, "groups", seed=B)
    a = reference(n, c, 2.0, torch.ones(B), "fp32", en, ec)
    b = mask_reference(n, c, 2.0, en, ec, "fp32")
    assert abs(a[0] - b[0]) <= 1e-14 and (a[1] - b[1]).abs().max().item() <= 1e-15 and (a[2] - b[2]).abs().max().item() <= 1e-15


def test_pw_entries_declared_bound_exported():
    header = (ROOT / "include" / "twotower.h").read_text()
    declared = set(re.findall(r"\b(tt_\w+_pw)\s*\(", header))
    assert declared == set(PW_SYMBOLS)
    assert re.search(r"#define\s+TT_ABI_VERSION\s+2\b", header)
    lib = _lib.load()
    assert lib.tt_abi_version() == 2
    for name in PW_SYMBOLS:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    sig, vp = _lib.SIGNATURES, _lib.vp
    # the masked entries with g in front of the ids; the finish is the logQ one with g in front of the logQ vectors
    m = sig["tt_score_fwd_sym_bf16_mask"][1]
    assert sig["tt_score_fwd_sym_bf16_pw"][1] == m[:9] + [vp] + m[9:]
    m = sig["tt_score_bwd_bf16_mask"][1]
    assert sig["tt_score_bwd_bf16_pw"][1] == m[:2] + [vp] + m[2:]
    assert m[4] == ctypes.POINTER(_lib.ScoreBwdLq)
    m = sig["tt_score_dir_bwd_mask"][1]
    assert sig["tt_score_dir_bwd_pw"][1] == m[:9] + [vp] + m[9:]
    m = sig["tt_score_loss_finish_lq"][1]
    assert sig["tt_score_loss_finish_pw"][1] == m[:3] + [vp] + m[3:]
    assert sig["tt_score_prepare_pw"][1] == [vp, vp, _lib.i64, vp, vp]


class _FakeStore:
    def __init__(self, n):
        self.n, self.device = n, torch.device("cpu")

    def __len__(self):
        return self.n


def _loader(n_pairs=10, batch=3, **kw):
    from jodalrob_twotower_amd.data_loader import DevicePairLoader
    pairs = np.stack([np.arange(n_pairs) % 5, (np.arange(n_pairs) * 2) % 3], axis=1)
    return DevicePairLoader(_FakeStore(5), _FakeStore(3), pairs, batch, shuffle=False, **kw)


def test_loader_pair_weight_arrays():
    assert _loader().pair_weight is None and _loader().epoch_pair_weight(None) is None
    w = torch.arange(1, 11, dtype=torch.float32)
    ld = _loader(pair_weight=w)
    assert torch.equal(ld.pair_weight, w)
    arr = ld.epoch_pair_weight(None)
    assert arr.shape == (4, 4) and arr.dtype == torch.float32
    order = torch.tensor([9, 0, 4, 3, 2, 1, 8, 7, 6, 5])
    arr_o = ld.epoch_pair_weight(order)
    for k, lo in enumerate(range(0, 10, 3)):
        m = min(3, 10 - lo)
        assert torch.equal(arr[k, :m], w[lo:lo + m]) and torch.equal(arr_o[k, :m], w[order[lo:lo + m]])
        assert arr[k, :m].data_ptr() % 16 == arr.data_ptr() % 16
        assert not arr[k, m:].any()
    ld.set_pair_weight(None)
    assert ld.pair_weight is None and ld.epoch_pair_weight(None) is None
    for bad, what in ((w[:-1], "shape"), (w.double(), "float32"), (w.reshape(10, 1), "shape"), (list(range(10)), "float32")):
        with pytest.raises(ValueError, match=what):
            _loader(pair_weight=bad)
    with pytest.raises(NotImplementedError, match="unrolled"):
        next(_loader(pair_weight=w).step_batches(SimpleNamespace(unroll=2)))


def test_inverse_count_weights():
    from jodalrob_twotower_amd.pair_weights import inverse_count_weights
    pairs = np.array([[3, 0], [3, 1], [5, 1], [3, 2], [9, 1], [5, 0]], dtype=np.int64)
    wn = inverse_count_weights(pairs)
    assert wn.dtype == torch.float32 and wn.device.type == "cpu"
    assert torch.equal(wn, torch.tensor([1 / 3, 1 / 3, 1 / 2, 1 / 3, 1.0, 1 / 2], dtype=torch.float32))
    wc = inverse_count_weights(torch.from_numpy(pairs), side="company")
    assert torch.equal(wc, torch.tensor([1 / 2, 1 / 3, 1 / 3, 1.0, 1 / 3, 1 / 2], dtype=torch.float32))
    # every notice counts once: the weights of a notice's pairs sum to 1
    assert abs(float(wn.sum()) - 3.0) < 1e-6
    with pytest.raises(ValueError, match="side"):
        inverse_count_weights(pairs, side="both")
    with pytest.raises(ValueError, match="shape"):
        inverse_count_weights(pairs[:, 0])
    with pytest.raises(TypeError, match="integers"):
        inverse_count_weights(pairs.astype(np.float32))
    # the loader takes them as they are
    ld = _loader(n_pairs=6, pair_weight=inverse_count_weights(_loader(n_pairs=6).pairs))
    assert ld.pair_weight.shape == (6,)


def _fake_task(score_dtype="bf16", dense=False):
    return SimpleNamespace(score_dtype=score_dtype, _dense_loss=dense, _refused=frozenset())


def _batch(B, w):
    b = {"notice": {"dense": torch.zeros(B, 3)}, "company": {"dense": torch.zeros(B, 3)}}
    if w is not None:
        b["pair_weight"] = w
    return b


def test_task_refuses_pair_weights_it_does_not_cover():
    from jodalrob_twotower_amd.two_tower_train_task import TwoTowerTrainTask
    from jodalrob_twotower_amd.distributed import DistributedTwoTowerTrainTask
    B = 8
    w = torch.ones(B)
    def f(task, batch, B):
        return TwoTowerTrainTask._batch_terms(task, batch, B).pw
    assert f(_fake_task(), _batch(B, None), B) is None
    assert f(_fake_task("fp32"), _batch(B, w), B) is w
    for dt in ("fp8", "bf16x3"):
        with pytest.raises(ValueError, match=dt):
            f(_fake_task(dt), _batch(B, w), B)
    with pytest.raises(ValueError, match="dense loss"):
        f(_fake_task(dense=True), _batch(B, w), B)
    with pytest.raises(ValueError, match="shape"):
        f(_fake_task(), _batch(B, torch.ones(B + 1)), B)
    with pytest.raises(ValueError, match="shape"):
        f(_fake_task(), _batch(B, torch.ones(B, 1)), B)
    with pytest.raises(ValueError, match="float32"):
        f(_fake_task(), _batch(B, w.double()), B)
    with pytest.raises(ValueError, match="float32"):
        f(_fake_task(), _batch(B, [1.0] * B), B)
    with pytest.raises(ValueError, match="is on meta"):
        f(_fake_task(), _batch(B, torch.ones(B, device="meta")), B)
    with pytest.raises(ValueError, match="pair_weight"):
        TwoTowerTrainTask.forward_with_ranks(None, _batch(B, w))
    with pytest.raises(NotImplementedError, match="sharded"):
        DistributedTwoTowerTrainTask._score_ce(None, None, None, 1.0, False, pair_weight=w)


def test_unrolled_segmented_and_sharded_steps_refuse_pair_weights():
    from jodalrob_twotower_amd.graph import GraphedTrainStep
    from jodalrob_twotower_amd.segmented import SegmentedTrainStep
    from jodalrob_twotower_amd.unrolled import UnrolledTrainStep
    assert "pair_weight" in GraphedTrainStep._accepts and "pair_weight" not in UnrolledTrainStep._accepts
    assert "pair_weight" not in SegmentedTrainStep._accepts
    ex = {"notice": {"dense": torch.zeros(4, 2)}, "company": {"dense": torch.zeros(4, 2)}, "pair_weight": torch.ones(4)}
    with pytest.raises(NotImplementedError, match="UnrolledTrainStep"):
        UnrolledTrainStep(None, None, ex, unroll=2)
    with pytest.raises(NotImplementedError, match="SegmentedTrainStep"):
        SegmentedTrainStep(None, None, ex)
    with pytest.raises(NotImplementedError, match="sharded"):
        GraphedTrainStep(SimpleNamespace(exchange=object()), None, ex)
    # a captured step's with / without check (no device needed: the check comes first)
    step = SimpleNamespace(_terms=frozenset())
    assert GraphedTrainStep._term_pairs(step, "pair_weight", None, "the batch") == []
    with pytest.raises(ValueError, match="pair_weight mismatch"):
        GraphedTrainStep._term_pairs(step, "pair_weight", torch.ones(4), "the batch")
    step = SimpleNamespace(_terms=frozenset({"pair_weight"}), static={"pair_weight": torch.zeros(4)})
    with pytest.raises(ValueError, match="pair_weight mismatch"):
        GraphedTrainStep._term_pairs(step, "pair_weight", None, "step_from_store")
    with pytest.raises(ValueError, match="shape"):
        GraphedTrainStep._term_pairs(step, "pair_weight", torch.ones(5), "the batch")
    (dst, src), = GraphedTrainStep._term_pairs(step, "pair_weight", torch.ones(4), "the batch")
    assert dst is step.static["pair_weight"] and src.data_ptr() % 16 == 0
