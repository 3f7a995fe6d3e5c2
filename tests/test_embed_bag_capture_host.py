"""The capacity form of the pooled lookup and the captured bag-mode step: what can be checked without a GPU -- the C ABI's new
entries, the numpy model of the padded plan (tests/_bag_plan_reference.py), and the argument checks of
GraphedTrainStep(bag_capacity=...) that run before anything touches a device."""
import ctypes
import re

import numpy as np
import pytest
import torch

import _bag_plan_reference as P
from conftest import GOLD, ROOT

import jodalrob_twotower_amd as tt
from jodalrob_twotower_amd import _lib

SYMBOLS = ("tt_embed_bag_fwd_cap", "tt_bag_prepare", "tt_bag_prepare_workspace_bytes", "tt_dedup_plan_pad")


def test_symbols_in_header_and_library():
    header = (ROOT / "include" / "twotower.h").read_text()
    lib = _lib.load()
    for name in SYMBOLS:
        assert re.search(rf"^\s*(?:int|size_t)\s+{name}\s*\(", header, flags=re.M), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    # the existing entries are declared as they were
    for name in ("tt_embed_bag_fwd", "tt_embed_bag_grad_bwd", "tt_dedup_plan"):
        assert re.search(rf"^\s*int\s+{name}\s*\(", header, flags=re.M) and name in _lib.SIGNATURES
    assert _lib.SIGNATURES["tt_embed_bag_fwd_cap"] == _lib.SIGNATURES["tt_embed_bag_fwd"]
    assert _lib.SIGNATURES["tt_dedup_plan_pad"] == _lib.SIGNATURES["tt_dedup_plan"]
    # the ctypes lengths struct has the C layout: 4 pointers, one int64, one int32 (+ padding)
    assert ctypes.sizeof(_lib.BagLengths) == 4 * 8 + 8 + 8
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct tt_bag_lengths \{(.*?)\} tt_bag_lengths;", header, flags=re.S).group(1), flags=re.S)
    assert re.findall(r"(\w+);", body) == [f[0] for f in _lib.BagLengths._fields_]
    # one int64 of workspace per 2048-slot tile of a side
    slots = (ctypes.c_int64 * 2)(2048, 2049)
    assert lib.tt_bag_prepare_workspace_bytes(slots, 2) == 8 * 3
    assert lib.tt_bag_prepare_workspace_bytes(slots, 1) == 8


@pytest.mark.parametrize("seed", range(6))
def test_padded_plan_model_equals_the_plan_of_the_live_positions(seed):
    """Positions with the pad row appended anywhere -- behind every side, so in the middle of position space too -- give the same
    unique_rows[:U], the same segments (as runs of LIVE positions) and the same ordered f32 sums as the live positions alone."""
    rng = np.random.default_rng(seed)
    R, E = 40, 3
    live = [int(rng.integers(0, 60)) for _ in range(3)]
    if seed == 0:
        live = [0, 0, 0]                                               # nothing live: the plan is all pads, n_unique = 0
    caps = [n + int(rng.integers(0, 30)) for n in live]
    if seed == 1:
        caps = list(live)                                              # no pad at all
    rows = rng.integers(0, R, sum(live))
    if rows.size:
        rows[rng.integers(0, rows.size, 3)] = R - 1                    # the last real row, next to the pad key
    contrib = rng.standard_normal((sum(live), E)).astype(np.float32)
    src0, uniq0, seg0, n0 = P.plan(rows)
    padded, where = P.with_pads(rows, R, list(zip(live, caps)))
    assert padded.size == sum(caps) and (padded[where] == rows).all() and (np.delete(padded, where) == R).all()
    src1, uniq1, seg1, n1 = P.padded_plan(padded, R)
    assert n1 == n0 and np.array_equal(uniq1[:n1], uniq0[:n0]) and np.array_equal(seg1[:n1 + 1], seg0[:n0 + 1])
    # the real rows' runs list the same live positions in the same order
    back = np.full(sum(caps), -1, np.int64)
    back[where] = np.arange(sum(live))
    assert np.array_equal(back[src1[:seg1[n1]]], src0[:seg0[n0]])
    # behind them: the pad run, every pad position once, ascending
    assert np.array_equal(src1[seg1[n1]:], np.delete(np.arange(sum(caps)), where))
    if sum(caps) > sum(live):
        assert uniq1[n1] == R and seg1[n1 + 1] == sum(caps) and len(uniq1) == n1 + 1
    in_cap = np.zeros((sum(caps), E), np.float32)
    in_cap[where] = contrib
    a, b = P.ordered_sums(src0, seg0, n0, contrib), P.ordered_sums(src1, seg1, n1, in_cap)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_resolve_bag_capacity():
    from jodalrob_twotower_amd.graph import resolve_bag_capacity as r
    nnz = {"notice": 300, "company": 90}
    assert r(500, nnz) == {"notice": 500, "company": 500}
    assert r({"notice": 300, "company": 1000}, nnz) == {"notice": 300, "company": 1000}
    assert r("auto", nnz) == {"notice": 1200, "company": 1024}                     # four times the example's, at least 1024
    assert r(7, {"company": 0}) == {"company": 7} and r("auto", {}) == {}
    for bad, what in ((299, "example batch carries 300 ids"), ({"notice": 400}, "no capacity for the bag-mode side 'company'"),
                      ({"notice": 400, "company": 89}, "carries 90 ids"), ({"notice": 400, "company": 90, "x": 1}, "not in bag mode"),
                      ("big", "'auto'"), (3.5, "must be an int"), (True, "must be an int"), (0, "at least 1")):
        with pytest.raises(ValueError, match=what):
            r(bad, nnz if bad != 0 else {"company": 0})


def test_bag_capacity_refusals_need_no_device(schema_syn):
    """bag_capacity on a plain model, the refusal without it, the steps that keep refusing, a capacity below the example's ids and
    an example with extra negatives: all raised before the constructor touches a device (the tasks live on the CPU)."""
    from jodalrob_twotower_amd.graph import GraphedTrainStep
    from jodalrob_twotower_amd.optim import FusedAdam
    from jodalrob_twotower_amd.segmented import SegmentedTrainStep
    from jodalrob_twotower_amd.unrolled import UnrolledTrainStep
    kn, kc = schema_syn["notice"]["categorical"], schema_syn["company"]["categorical"]
    meta = str(GOLD / "synthetic_metadata.csv")
    mk = lambda pool: tt.create_two_tower_train_task(kn, kc, metadata_path=meta, categorical_embedding_dim=4, notice_dense_input_dim=3,
                                                     company_dense_input_dim=2, tower_hidden_dims=[8, 4], final_embedding_dim=4,
                                                     device="cpu", categorical_pooling=pool)
    B = 4
    lengths = torch.tensor([2, 0, 1, 3] * len(kc))[:B * len(kc)]
    batch = {"notice": {"dense": torch.zeros(B, 3), "kjt": tt.build_batch_kjt(torch.zeros((B, len(kn)), dtype=torch.long), kn)},
             "company": {"dense": torch.zeros(B, 2),
                         "kjt": tt.build_bag_kjt(kc, values=torch.zeros(int(lengths.sum()), dtype=torch.long), lengths=lengths)}}
    nnz = int(lengths.sum())
    plain, bag = mk(None), mk({"company": "mean"})
    with pytest.raises(ValueError, match="bag_capacity: the model has no bag-mode embedder"):
        GraphedTrainStep(plain, FusedAdam.for_task(plain, lr=1e-2), batch, bag_capacity=64)
    opt = FusedAdam.for_task(bag, lr=1e-2)
    with pytest.raises(ValueError, match="GraphedTrainStep does not support bag mode"):
        GraphedTrainStep(bag, opt, batch)
    for cls in (UnrolledTrainStep, SegmentedTrainStep):                            # with or without a capacity
        for kw in ({}, {"bag_capacity": 64}):
            with pytest.raises(ValueError, match=rf"{cls.__name__} does not support bag mode"):
                cls(bag, opt, batch, **kw)
    with pytest.raises(ValueError, match=rf"bag_capacity = {nnz - 1} for 'company': the example batch carries {nnz} ids"):
        GraphedTrainStep(bag, opt, batch, bag_capacity=nnz - 1)
    with pytest.raises(ValueError, match="names sides that are not in bag mode"):
        GraphedTrainStep(bag, opt, batch, bag_capacity={"notice": 64, "company": 64})
    neg = {"dense": torch.zeros(2, 2), "kjt": tt.build_bag_kjt(kc, values=torch.zeros(2 * len(kc), dtype=torch.long),
                                                             lengths=torch.ones(2 * len(kc), dtype=torch.long))}
    with pytest.raises(NotImplementedError, match="extra negatives.*captured bag-mode step"):
        GraphedTrainStep(bag, opt, dict(batch, negatives=neg), bag_capacity=64)
