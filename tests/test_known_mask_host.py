"""Host-side checks of the known-pair mask (masked cells of the in-batch softmax; include/twotower.h *_cells entries): the f64 reference
of tests/_known_mask_reference.py against autograd and against the repeated-entity references, the loader's epoch_cells against a
brute-force set-membership loop, the C ABI of the new symbols, and the refusals that need no GPU."""
import re

import numpy as np
import pytest
import torch

import _known_mask_reference as KR
import _mask_reference as MR
import _xneg_reference as XR
from conftest import ROOT

NEW_SYMBOLS = ("tt_score_cells_plan_bytes", "tt_score_cells_plan_workspace_bytes", "tt_score_cells_plan", "tt_score_fwd_sym_bf16_cells",
               "tt_score_bwd_bf16_cells")


def _rows(R, D, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(R, D, generator=g)
    return x / x.norm(dim=1, keepdim=True)


def _random_cells(B, M, frac, seed, junk=True):
    g = np.random.default_rng(seed)
    L = max(int(frac * B * (B + M)), 1)
    cells = np.stack([g.integers(0, B, L), g.integers(0, B + M, L)], 1)
    if junk:                                                   # duplicates, diagonal cells and cells outside the ranges
        cells = np.concatenate([cells, cells[:3], [[1, 1], [B - 1, B - 1], [-1, 0], [0, -1], [B, 0], [0, B + M], [2**30, 3]]], 0)
    return cells


# ---- 1. the reference ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,M,D,T", [(9, 0, 5, 1.0), (37, 0, 16, 0.5), (12, 7, 8, 2.0), (33, 40, 12, 0.25)])
@pytest.mark.parametrize("lq", [False, True])
def test_reference_equals_f64_autograd(B, M, D, T, lq):
    n, c = _rows(B, D, 1 + B), _rows(B, D, 2 + B)
    x = _rows(M, D, 3 + M) if M else None
    g = torch.Generator().manual_seed(5)
    q = (-45.0 * torch.rand(B, generator=g), -6.0 * torch.rand(B, generator=g), -6.0 * torch.rand(M, generator=g) if M else None) if lq \
        else (None, None, None)
    cells = _random_cells(B, M, 0.2, B + M)
    om = KR.clean_cells(cells, B, M)
    assert len(om) and (om[:, 0] != om[:, 1]).all() and om[:, 1].max() < B + M and (M == 0 or (om[:, 1] >= B).any())
    loss, dN, dC, dX = KR.reference(n, c, x, cells, 1.0 / T, "fp32", *q)
    a_loss, a_dN, a_dC, a_dX = KR.autograd_reference(n, c, x, cells, 1.0 / T, *q)
    assert abs(loss - a_loss) <= 1e-12 * max(abs(a_loss), 1.0)
    assert float((dN - a_dN).abs().max()) <= 1e-12 and float((dC - a_dC).abs().max()) <= 1e-12
    if M:
        assert float((dX - a_dX).abs().max()) <= 1e-12
    else:
        assert dX is None and a_dX is None
    # the cleaned list gives the same numbers; a heavy row (everything but its positive masked) stays finite
    assert KR.reference(n, c, x, om, 1.0 / T, "fp32", *q)[0] == loss
    heavy = np.array([[2, j] for j in range(B + M)] + [[a, 4] for a in range(B)])
    hl = KR.reference(n, c, x, heavy, 1.0 / T, "fp32", *q)
    assert np.isfinite(hl[0]) and bool(torch.isfinite(hl[1]).all())


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("pattern", ["tile_edge", "groups", "heavy", "one_notice"])
@pytest.mark.parametrize("lq", [False, True])
def test_reference_with_entity_cells_is_the_entity_mask(mode, pattern, lq):
    B, M, D, inv_t = 70, 21, 16, 2.0
    n, c, x = _rows(B, D, 1), _rows(B, D, 2), _rows(M, D, 3)
    en, ec = MR.ids(B, pattern, seed=B)
    g = np.random.default_rng(4)
    ex = torch.tensor(np.where(g.random(M) < 0.5, ec.numpy()[g.integers(0, B, M)], 10 ** 6 + np.arange(M)), dtype=torch.int32)
    tg = torch.Generator().manual_seed(6)
    q = (-5.0 * torch.rand(B, generator=tg), -5.0 * torch.rand(B, generator=tg), -5.0 * torch.rand(M, generator=tg)) if lq else (None,) * 3
    # in-batch only: tests/_mask_reference.py
    got = KR.reference(n, c, None, KR.entity_cells(en, ec), inv_t, mode, q[0], q[1])
    want = MR.reference(n, c, inv_t, en, ec, mode, q[0], q[1])
    assert abs(got[0] - want[0]) <= 1e-12 and float((got[1] - want[1]).abs().max()) <= 1e-12 and float((got[2] - want[2]).abs().max()) <= 1e-12
    # with extras: tests/_xneg_reference.py's masked form
    got = KR.reference(n, c, x, KR.entity_cells(en, ec, ex), inv_t, mode, *q)
    want = XR.reference(n, c, x, inv_t, mode, en, ec, ex, *q)
    assert abs(got[0] - want[0]) <= 1e-12
    for u, v in zip(got[1:], want[1:]):
        assert float((u - v).abs().max()) <= 1e-12


# ---- 2. the loader's cells ---------------------------------------------------------------------------------------------------------
def _cpu_world(seed, nN=25, nC=60, P=150):
    from jodalrob_twotower_amd.data_loader import DeviceFeatureStore
    rng = np.random.default_rng(seed)
    ns = DeviceFeatureStore({"dense_projected": np.zeros((nN, 2), np.float32), "categorical": np.zeros((nN, 1), np.int64)}, ["a"], "cpu")
    cs = DeviceFeatureStore({"dense_projected": np.zeros((nC, 2), np.float32), "categorical": np.zeros((nC, 1), np.int64)}, ["b"], "cpu")
    # few notices and a skewed company draw: repeated notices, repeated companies and repeated pairs inside every batch
    pairs = np.stack([rng.integers(0, nN, P), np.minimum(rng.geometric(0.08, P) - 1, nC - 1)], 1)
    return ns, cs, pairs


def _epoch(loader):
    order = loader.epoch_order()
    neg = loader.epoch_negatives(order)
    return order, neg, loader.epoch_cells(order, neg)


@pytest.mark.parametrize("shuffle", [False, True])
@pytest.mark.parametrize("M", [0, 13])
@pytest.mark.parametrize("extra_known", [False, True])
def test_epoch_cells_equal_brute_force(shuffle, M, extra_known):
    from jodalrob_twotower_amd.data_loader import DevicePairLoader
    ns, cs, pairs = _cpu_world(7)
    B = 32                                                     # 150 pairs: four full batches and a ragged one of 22
    known_pairs = None
    if extra_known:                                            # train plus "validation" pairs
        rng = np.random.default_rng(8)
        known_pairs = np.concatenate([pairs, np.stack([rng.integers(0, 25, 80), rng.integers(0, 60, 80)], 1)], 0)
    # the extras' pool: the companies of the pair table, so that extras ARE known companies of other rows' notices
    pool = torch.as_tensor(np.unique(pairs[:, 1]))
    loader = DevicePairLoader(ns, cs, pairs, B, shuffle=shuffle, seed=3, extra_negatives=M, negative_pool=pool if M else None,
                              mask_known=True, known_pairs=known_pairs)
    known = set(map(tuple, (pairs if known_pairs is None else known_pairs).tolist()))
    for epoch in range(2):
        order, neg, (cells, bounds) = _epoch(loader)
        assert cells.dtype == torch.int32 and cells.shape[1] == 2 and len(bounds) == len(loader)
        assert all(lo % 2 == 0 and lo <= hi for lo, hi in bounds) and bounds[-1][1] <= cells.shape[0]      # 16-byte aligned slices
        sel_all = pairs if order is None else pairs[order.numpy()]
        n_x = n_in = worst = 0
        for k in range(len(loader)):
            sel = sel_all[k * B:(k + 1) * B]
            m = len(sel)
            want = KR.brute_cells(sel, None if neg is None else neg[k].numpy(), known, m)
            got = [tuple(r) for r in cells[bounds[k][0]:bounds[k][1]].tolist()]
            assert got == want, (epoch, k)
            n_in += sum(1 for a, j in want if j < m)
            n_x += sum(1 for a, j in want if j >= m)
            worst = max(worst, len(want))
            # superset of the repeated-entity mask's cells (in-batch)
            ent = KR.entity_cells(torch.as_tensor(sel[:, 0]), torch.as_tensor(sel[:, 1]))
            assert set(map(tuple, ent.tolist())) <= set(want)
        assert loader.max_cells == worst
        assert n_in > 0 and (M == 0 or n_x > 0)
        assert len(sel_all) % B != 0                           # the ragged batch was covered


def test_epoch_cells_do_not_depend_on_the_chunk_size():
    from jodalrob_twotower_amd.data_loader import DevicePairLoader
    ns, cs, pairs = _cpu_world(7)
    pool = torch.as_tensor(np.unique(pairs[:, 1]))
    got = []
    for chunk in (1, 2, 8):
        loader = DevicePairLoader(ns, cs, pairs, 32, shuffle=True, seed=3, extra_negatives=13, negative_pool=pool, mask_known=True)
        loader.CELLS_CHUNK_BATCHES = chunk
        got.append(_epoch(loader)[2])
    for cells, bounds in got[1:]:
        assert torch.equal(cells, got[0][0]) and bounds == got[0][1]


def test_step_batches_counts_batches_over_the_capacity():
    """no GPU: stand-ins for the captured steps -- a batch with more cells than the step it would take has room for goes through the
    eager callable, is counted and warned about once; the others go through .step"""
    from jodalrob_twotower_amd.data_loader import DevicePairLoader
    ns, cs, pairs = _cpu_world(7)
    loader = DevicePairLoader(ns, cs, pairs, 32, shuffle=False, mask_known=True)
    loader.batch = lambda order, lo, neg=None, cells=None: {"masked_cells": cells[0][cells[1][lo // 32][0]:cells[1][lo // 32][1]]}
    _, bounds = loader.epoch_cells(None, None)
    sizes = [hi - lo for lo, hi in bounds]

    class Step:
        def __init__(self, cap, rows):
            self.cell_capacity, self.static, self.seen = cap, {"notice": {"dense": torch.zeros(rows, 1)}}, 0

        def step(self, b):
            assert b["masked_cells"].shape[0] <= self.cell_capacity
            self.seen += 1
            return "step"
    cap = sorted(sizes[:4])[1]                                  # two of the four full batches fit
    full, ragged = Step(cap, 32), Step(10 ** 6, 150 - 4 * 32)
    with pytest.warns(UserWarning, match="cell_capacity"):
        out = list(loader.step_batches(full, eager_step=lambda b: "eager", ragged_step=ragged))
    want = ["step" if s_ <= cap else "eager" for s_ in sizes[:4]] + ["step"]
    assert out == want and loader.eager_cell_batches == want.count("eager") >= 1 and full.seen == want.count("step") - 1 and ragged.seen == 1


def test_loader_refusals_and_off_by_default():
    from jodalrob_twotower_amd.data_loader import DevicePairLoader
    ns, cs, pairs = _cpu_world(9)
    plain = DevicePairLoader(ns, cs, pairs, 32, shuffle=False)
    assert plain.known is None and plain.epoch_cells(None, None) is None
    with pytest.raises(ValueError):
        DevicePairLoader(ns, cs, pairs, 32, shuffle=False, mask_repeats=True, mask_known=True)
    with pytest.raises(ValueError):
        DevicePairLoader(ns, cs, pairs, 32, shuffle=False, pair_weight=torch.ones(len(pairs)), mask_known=True)
    on = DevicePairLoader(ns, cs, pairs, 32, shuffle=True, mask_known=True)
    with pytest.raises(ValueError):
        on.set_mask_repeats(True)
    with pytest.raises(ValueError):
        on.set_pair_weight(torch.ones(len(pairs)))
    with pytest.raises(ValueError):
        on.epoch_cells(None, None)                             # shuffling: needs the order
    with pytest.raises(KeyError):
        on.set_mask_known(True, known_pairs=np.array([[0, 60]]))
    with pytest.raises(KeyError):
        on.set_mask_known(True, known_pairs=np.array([[25, 0]]))
    on.set_mask_known(False)
    assert on.known is None


# ---- 3. the C ABI and the refusals that need no GPU ----------------------------------------------------------------------------------
def test_new_symbols_are_declared_once_and_bound():
    from jodalrob_twotower_amd import _lib
    header = (ROOT / "include" / "twotower.h").read_text()
    for name in NEW_SYMBOLS:
        assert len(re.findall(r"^(?:size_t|int) %s\(" % name, header, flags=re.M)) == 1, name
        assert name in _lib.SIGNATURES
    lib = _lib.load()
    # the plan's size: offsets over the nT x (nT + nTx) tile pairs plus one, padded to 16 bytes, then one code per slot
    assert lib.tt_score_cells_plan_bytes(70, 33, 100) == 4 * ((3 * 5 + 1 + 3) // 4 * 4 + 100)
    assert lib.tt_score_cells_plan_bytes(64, 0, 1) == 4 * (8 + 1)
    assert lib.tt_score_cells_plan_bytes(0, 0, 1) == 0 and lib.tt_score_cells_plan_bytes(64, 0, 0) == 0
    assert lib.tt_score_cells_plan_workspace_bytes(70, 33) >= 4 * 15


def _cpu_task(**kw):
    import jodalrob_twotower_amd as tt
    gold = ROOT / "tests" / "golden"
    schema = tt.build_torchrec_schema_from_meta(metadata_path=gold / "synthetic_metadata.csv", notice_table="notice", company_table="company",
                                                pair_table="bid_two_tower", pair_notice_id_cols=["bidntceno", "bidntceord"],
                                                pair_company_id_cols=["bizno"])
    return tt.create_two_tower_train_task(schema.notice.categorical, schema.company.categorical, metadata_path=str(gold / "synthetic_metadata.csv"),
                                          categorical_embedding_dim=4, notice_dense_input_dim=8, company_dense_input_dim=8,
                                          tower_hidden_dims=[8, 8], final_embedding_dim=8, device="cpu", **kw)


def _cpu_batch(B=6, **extra):
    b = {"notice": {"dense": torch.zeros(B, 8)}, "company": {"dense": torch.zeros(B, 8)}}
    b.update(extra)
    return b


def test_task_refusals_without_a_gpu():
    cells = torch.zeros((3, 2), dtype=torch.int32)
    task = _cpu_task(score_dtype="bf16")
    for bad in (cells.long(), cells[:, 0], torch.zeros((3, 3), dtype=torch.int32), [[0, 1]]):
        with pytest.raises(ValueError):
            task._batch_terms(_cpu_batch(masked_cells=bad), 6)
    with pytest.raises(ValueError):
        task._batch_terms(_cpu_batch(masked_cells=cells, masked_cells_count=torch.zeros(1)), 6)
    with pytest.raises(ValueError):                            # with the repeated-entity mask
        b = _cpu_batch(masked_cells=cells)
        b["notice"]["entity"] = torch.zeros(6, dtype=torch.int32)
        task._batch_terms(b, 6)
    with pytest.raises(ValueError):                            # with pair weights
        task._batch_terms(_cpu_batch(masked_cells=cells, pair_weight=torch.ones(6)), 6)
    assert task._batch_terms(_cpu_batch(), 6).cells is None
    got = task._batch_terms(_cpu_batch(masked_cells=cells), 6).cells
    assert got[0] is cells and got[1] is None
    for dt in ("fp32", "fp8", "bf16x3"):
        with pytest.raises(ValueError):
            _cpu_task(score_dtype=dt)._batch_terms(_cpu_batch(masked_cells=cells), 6)
    dense = _cpu_task(score_dtype="bf16")
    dense._dense_loss = True
    with pytest.raises(ValueError):
        dense._batch_terms(_cpu_batch(masked_cells=cells), 6)
    with pytest.raises(ValueError):
        task.forward_with_ranks(_cpu_batch(masked_cells=cells))
    task._refused = frozenset({"masked_cells"})                # what the sharded task declares
    with pytest.raises(NotImplementedError):
        task._batch_terms(_cpu_batch(masked_cells=cells), 6)
    from jodalrob_twotower_amd.distributed import DistributedTwoTowerTrainTask
    assert "masked_cells" in DistributedTwoTowerTrainTask._refused


def test_score_node_signature_keeps_positional_calls():
    import inspect
    from jodalrob_twotower_amd.two_tower_train_task import _ScoreCEFn
    names = list(inspect.signature(_ScoreCEFn.forward).parameters)
    assert names[-5:] == ["x", "lq_x", "ent_x", "cells", "cell_count"]
    sig = inspect.signature(_ScoreCEFn.forward)
    assert sig.parameters["cells"].default is None and sig.parameters["cell_count"].default is None
