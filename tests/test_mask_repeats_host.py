"""Host-side tests of the repeated-entity mask: the f64 reference (tests/_mask_reference.py) against autograd of masked_fill(-inf) +
logsumexp, the C entries declared, bound and exported, DevicePairLoader's entity arrays, and the refusals that need no device."""
import ctypes
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import ROOT
from jodalrob_twotower_amd import _lib
from _mask_reference import ids, mask_matrix, masked_loss, reference

MASK_SYMBOLS = ("tt_score_fwd_sym_bf16_mask", "tt_score_bwd_bf16_mask", "tt_score_dir_fwd_mask", "tt_score_dir_bwd_mask")


def _unit_rows(B, D, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, D, generator=g)
    return x / x.norm(dim=1, keepdim=True)


@pytest.mark.parametrize("B", [1, 33, 65])
@pytest.mark.parametrize("with_lq", [False, True])
@pytest.mark.parametrize("pattern", ["distinct", "one_notice", "tile_edge", "groups", "heavy"])
def test_reference_equals_autograd(B, with_lq, pattern):
    """the closed form (loss, W C, W^T N) against autograd of the masked logsumexp in f64: 1e-12"""
    D, inv_t = 16, 1.0 / 0.3
    n, c = _unit_rows(B, D, 3 + B), _unit_rows(B, D, 5 + B)
    ent_n, ent_c = ids(B, pattern, seed=B)
    g = torch.Generator().manual_seed(9)
    lq_n = (-45.0 * torch.rand(B, generator=g)) if with_lq else None          # (some below the clamp)
    lq_c = (-45.0 * torch.rand(B, generator=g)) if with_lq else None
    loss, dN, dC = reference(n, c, inv_t, ent_n, ent_c, "fp32", lq_n, lq_c)
    A = n.double().requires_grad_(True)
    Bm = c.double().requires_grad_(True)
    auto = masked_loss((A @ Bm.T) * inv_t, mask_matrix(ent_n, ent_c), lq_n, lq_c)
    auto.backward()
    assert abs(loss - auto.item()) <= 1e-12 * max(1.0, abs(auto.item()))
    assert (dN - A.grad).abs().max().item() <= 1e-12 and (dC - Bm.grad).abs().max().item() <= 1e-12
    assert torch.isfinite(dN).all() and torch.isfinite(dC).all() and np.isfinite(loss)
    if pattern == "one_notice":                              # every negative masked: the positive term alone, loss 0, no gradient
        assert abs(loss) <= 1e-12 and dN.abs().max().item() <= 1e-12


def test_mask_matrix_definition():
    en = torch.tensor([1, 1, 2, 3, 3], dtype=torch.int32)
    ec = torch.tensor([9, 8, 8, 7, 6], dtype=torch.int32)
    M = mask_matrix(en, ec)
    want = torch.zeros(5, 5, dtype=torch.bool)
    for a, b in ((0, 1), (1, 2), (3, 4)):
        want[a, b] = want[b, a] = True
    assert torch.equal(M, want) and torch.equal(M, M.T) and not M.diagonal().any()
    assert torch.equal(mask_matrix(en, None), mask_matrix(en, torch.arange(5, dtype=torch.int32)))


def test_mask_entries_declared_bound_exported():
    header = (ROOT / "include" / "twotower.h").read_text()
    declared = set(re.findall(r"\b(tt_\w+_mask)\s*\(", header))
    assert declared == set(MASK_SYMBOLS)
    lib = _lib.load()
    for name in MASK_SYMBOLS:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    sig, vp = _lib.SIGNATURES, _lib.vp
    # each is the _lq entry plus the two id arrays in front of the (optional) logQ arguments
    lq = sig["tt_score_fwd_sym_bf16_lq"][1]
    assert sig["tt_score_fwd_sym_bf16_mask"][1] == lq[:9] + [vp] * 2 + lq[9:]
    lq = sig["tt_score_bwd_bf16_lq"][1]
    assert sig["tt_score_bwd_bf16_mask"][1] == lq[:2] + [vp] * 2 + lq[2:]
    assert lq[2] == ctypes.POINTER(_lib.ScoreBwdLq)
    assert sig["tt_score_dir_fwd_mask"][1] == sig["tt_score_dir_fwd_lq"][1][:9] + [vp] * 2 + sig["tt_score_dir_fwd_lq"][1][9:]
    assert sig["tt_score_dir_bwd_mask"][1] == sig["tt_score_dir_bwd_lq"][1][:9] + [vp] * 2 + sig["tt_score_dir_bwd_lq"][1][9:]


class _FakeStore:
    def __init__(self, n):
        self.n, self.device = n, torch.device("cpu")

    def __len__(self):
        return self.n


def _loader(n_pairs=10, batch=3, **kw):
    from jodalrob_twotower_amd.data_loader import DevicePairLoader
    pairs = np.stack([np.arange(n_pairs) % 5, (np.arange(n_pairs) * 2) % 3], axis=1)
    return DevicePairLoader(_FakeStore(5), _FakeStore(3), pairs, batch, shuffle=False, **kw)


def test_loader_entity_arrays_are_the_pair_columns():
    assert _loader().entity is None and _loader().epoch_entity(None) is None
    ld = _loader(mask_repeats=True)
    assert ld.entity.dtype == torch.int32 and torch.equal(ld.entity, ld.pairs.t().to(torch.int32))
    arr = ld.epoch_entity(None)
    assert arr.shape == (4, 2, 4) and arr.dtype == torch.int32
    order = torch.tensor([9, 0, 4, 3, 2, 1, 8, 7, 6, 5])
    arr_o = ld.epoch_entity(order)
    for k, lo in enumerate(range(0, 10, 3)):
        m = min(3, 10 - lo)
        for s in (0, 1):
            assert torch.equal(arr[k, s, :m], ld.pairs[lo:lo + m, s].to(torch.int32))
            assert torch.equal(arr_o[k, s, :m], ld.pairs[order[lo:lo + m], s].to(torch.int32))
            assert arr[k, s, :m].data_ptr() % 16 == arr.data_ptr() % 16
    ld.set_mask_repeats(False)
    assert ld.entity is None
    with pytest.raises(NotImplementedError, match="unrolled"):
        next(_loader(mask_repeats=True).step_batches(SimpleNamespace(unroll=2)))


def test_loader_refuses_an_index_beyond_int32():
    from jodalrob_twotower_amd.data_loader import DevicePairLoader
    big = 1 << 31
    pairs = np.array([[0, big]], dtype=np.int64)
    DevicePairLoader(_FakeStore(1), _FakeStore(big + 1), pairs, 1, shuffle=False)
    with pytest.raises(ValueError, match="int32"):
        DevicePairLoader(_FakeStore(1), _FakeStore(big + 1), pairs, 1, shuffle=False, mask_repeats=True)


def _fake_task(score_dtype="bf16", dense=False):
    return SimpleNamespace(score_dtype=score_dtype, _dense_loss=dense, _refused=frozenset())


def _side(B, ent):
    d = {"dense": torch.zeros(B, 3)}
    if ent is not None:
        d["entity"] = ent
    return d


def test_task_refuses_entity_ids_it_does_not_cover():
    from jodalrob_twotower_amd.two_tower_train_task import TwoTowerTrainTask
    from jodalrob_twotower_amd.distributed import DistributedTwoTowerTrainTask
    B = 8
    ent = torch.arange(B, dtype=torch.int32)
    def f(task, notice, company, B):
        return TwoTowerTrainTask._batch_terms(task, {"notice": notice, "company": company}, B).ent
    assert f(_fake_task(), _side(B, None), _side(B, None), B) is None
    for dt in ("fp8", "bf16x3"):
        with pytest.raises(ValueError, match=dt):
            f(_fake_task(dt), _side(B, ent), _side(B, None), B)
    with pytest.raises(ValueError, match="dense loss"):
        f(_fake_task(dense=True), _side(B, None), _side(B, ent), B)
    with pytest.raises(ValueError, match="shape"):
        f(_fake_task(), _side(B, torch.zeros(B + 1, dtype=torch.int32)), _side(B, None), B)
    with pytest.raises(ValueError, match="int32"):
        f(_fake_task(), _side(B, ent.long()), _side(B, None), B)
    n, c = f(_fake_task("fp32"), _side(B, None), _side(B, ent), B)           # a missing side counts as all-distinct
    assert n is None and torch.equal(c, ent)
    with pytest.raises(NotImplementedError, match="sharded"):
        DistributedTwoTowerTrainTask._score_ce(None, None, None, 1.0, False, entity=(ent, ent))


def test_unrolled_segmented_and_sharded_steps_refuse_entity_ids():
    from jodalrob_twotower_amd.graph import GraphedTrainStep
    from jodalrob_twotower_amd.segmented import SegmentedTrainStep
    from jodalrob_twotower_amd.unrolled import UnrolledTrainStep
    assert "entity" in GraphedTrainStep._accepts and "entity" not in UnrolledTrainStep._accepts and "entity" not in SegmentedTrainStep._accepts
    ex = {"notice": {"dense": torch.zeros(4, 2), "entity": torch.zeros(4, dtype=torch.int32)}, "company": {"dense": torch.zeros(4, 2)}}
    with pytest.raises(NotImplementedError, match="UnrolledTrainStep"):
        UnrolledTrainStep(None, None, ex, unroll=2)
    with pytest.raises(NotImplementedError, match="SegmentedTrainStep"):
        SegmentedTrainStep(None, None, ex)
    with pytest.raises(NotImplementedError, match="sharded"):
        GraphedTrainStep(SimpleNamespace(exchange=object()), None, ex)
