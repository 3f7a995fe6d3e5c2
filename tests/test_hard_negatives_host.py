"""Host-side tests of hard-negative mining (tt_ceil_retrieve_topk_*, tt_pair_scores_*, CatalogIndex max_score= / pair_scores,
hard_negatives.mine_hard_negatives, DevicePairLoader mined=): the f64 reference of tests/_mine_reference.py against brute force,
the ceilings the GPU tests place (every reference score 4 tol away, at most 1 % of a case's queries left out), the C ABI of the
four new symbols, the argument errors that need no GPU, and the loader's draw on the CPU."""
import math
import re

import numpy as np
import pytest
import torch

import _mine_reference as R
from conftest import ROOT

NEW_SYMBOLS = ("tt_ceil_retrieve_topk_bf16", "tt_ceil_retrieve_topk_f32", "tt_pair_scores_bf16", "tt_pair_scores_f32")


# ---- the reference against brute force ------------------------------------------------------------------------------------------
def test_reference_topk_under_a_ceiling_matches_brute_force():
    rng = np.random.default_rng(0)
    for trial in range(20):
        nQ, nC, k = int(rng.integers(1, 6)), int(rng.integers(3, 30)), int(rng.integers(1, 8))
        k = min(k, nC)
        S = torch.as_tensor(rng.integers(-4, 5, (nQ, nC)) / 4.0)           # few distinct values: ties everywhere
        lens = rng.integers(0, 5, nQ)
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        rows = np.concatenate([np.sort(rng.integers(-1, nC + 1, n)) for n in lens] + [np.zeros(0, np.int64)]).astype(np.int32)
        ceil = torch.as_tensor(rng.choice([-1.0, -0.25, 0.0, 0.5, 1.0, np.inf, -np.inf, np.nan], nQ), dtype=torch.float32)
        vals, idx = R.topk_index_rule(R.apply_ceiling(R.mask_scores(S, off, rows), ceil), k)
        for q in range(nQ):
            ex = set(rows[off[q]:off[q + 1]].tolist())
            c = float(ceil[q])
            elig = [(-float(S[q, j]), j) for j in range(nC) if j not in ex and not float(S[q, j]) >= c]
            want = sorted(elig)[:k]
            want_idx = [j for _, j in want] + [-1] * (k - len(want))
            want_val = [-v for v, _ in want] + [-math.inf] * (k - len(want))
            assert idx[q].tolist() == want_idx and vals[q].tolist() == want_val, (trial, q)


def test_reference_mining_matches_brute_force():
    rng = np.random.default_rng(1)
    nN, nC, k, per = 12, 40, 6, 3
    S = (rng.integers(-8, 9, (nN, nC)) / 8.0).astype(np.float32)
    pairs = np.stack([rng.integers(0, nN - 2, 30), rng.integers(0, nC, 30)], 1)     # the last two notices have no pairs
    for ceiling in (None, (0.5, 0.0), (1.0, -0.125)):
        table, cand, ceils = R.mine_reference(S, pairs, nN, k, per, ceiling)
        for n in range(nN):
            known = {int(c) for a, c in pairs if a == n}
            if not known:
                assert (table[n] == -1).all() and n not in cand
                continue
            lim = math.inf if ceiling is None else ceiling[0] * min(float(S[n, c]) for c in known) + ceiling[1]
            elig = sorted((-float(S[n, c]), c) for c in range(nC) if c not in known and float(S[n, c]) < lim)
            want = [c for _, c in elig][:per]
            assert table[n].tolist() == want + [-1] * (per - len(want))
            assert cand[n].tolist() == [c for _, c in elig][:k]


def test_reference_draw_rule():
    table = np.array([[5, 7, -1], [-1, -1, -1], [7, 9, 11]], dtype=np.int32)
    c = R.batch_candidates(table, [2, 0, 0, 1])
    assert c.tolist() == [7, 9, 11, 5, 7, 5, 7]
    assert R.batch_candidates(table, [1, 1]).size == 0
    assert [R.draw_from(c, u) for u in (0.0, 0.15, 0.5, 0.999999)] == [7, 9, 5, 7]


# ---- the ceilings the GPU tests place --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bf16", [True, False])
@pytest.mark.parametrize("nQ,nC,D,k,inv_t", R.CASES)
def test_gap_ceilings_are_unambiguous_and_leave_out_at_most_one_percent(bf16, nQ, nC, D, k, inv_t):
    Q, Cm, off, rows = R.make_case(nQ, nC, D, k)
    tol = R.tolerance(bf16, inv_t)
    S = R.ref_scores(Q, Cm, inv_t, bf16)
    for M in (S, R.mask_scores(S, off, rows)):
        ceil, ok = R.gap_ceilings(M, tol)
        assert int((~ok).sum()) <= nQ // 100
        assert ceil.dtype == torch.float32 and bool(torch.isfinite(ceil[ok]).all())
        dist = (M[ok] - ceil[ok].double()[:, None]).abs().min(dim=1).values
        assert bool((dist >= 4 * tol).all())
        below = (M[ok] < ceil[ok].double()[:, None]).sum(1)
        above = (M[ok] >= ceil[ok].double()[:, None]).sum(1)
        assert bool((above >= 4).all()) and bool((above <= 12).all()) and bool((below >= 1).all())


# ---- C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_header_lib_and_exports_of_the_new_symbols():
    from jodalrob_twotower_amd import _lib
    header = (ROOT / "include" / "twotower.h").read_text()
    declared = set(re.findall(r"^\s*int\s+(tt_ceil_retrieve\w+|tt_pair_scores\w+)\s*\(", header, flags=re.M))
    assert declared == set(NEW_SYMBOLS)
    lib = _lib.load()
    sig = _lib.SIGNATURES
    for name in NEW_SYMBOLS:
        assert name in sig and hasattr(lib, name), name
    for t in ("bf16", "f32"):                                            # the exclusion entry's arguments with `ceil` after excl_rows
        excl, ceil = sig[f"tt_excl_retrieve_topk_{t}"][1], sig[f"tt_ceil_retrieve_topk_{t}"][1]
        assert ceil == excl[:-3] + [_lib.vp] + excl[-3:]
    assert len(sig["tt_pair_scores_f32"][1]) == len(sig["tt_pair_scores_bf16"][1]) + 1       # inv_t
    assert not [n for n in NEW_SYMBOLS if n.startswith(("tt_retrieve", "tt_excl_retrieve", "tt_filt_retrieve"))]
    assert lib.tt_abi_version() == 2


# ---- argument errors -----------------------------------------------------------------------------------------------------------
def test_max_score_argument_errors():
    from jodalrob_twotower_amd.retrieval import CatalogIndex
    g = torch.Generator().manual_seed(0)
    Cm, Q = R.unit_rows(50, 8, g), R.unit_rows(4, 8, g)
    index = CatalogIndex.from_embeddings(Cm, score_dtype="fp32", tags=torch.ones(50, dtype=torch.int32))
    good = torch.zeros(4)
    for bad in (good.double(), good.long(), torch.zeros(5), torch.zeros(4, 1), [0.0] * 4, good.to("meta")):
        with pytest.raises(ValueError):
            index.search(Q, 3, max_score=bad)
        with pytest.raises(ValueError):
            index.search_with_rank(Q, 3, torch.zeros(4, dtype=torch.int64), max_score=bad)
    ones = torch.ones(4, dtype=torch.int32)
    for kw in ({"allow": ones}, {"require": ones}, {"allow": ones, "require": ones}):
        with pytest.raises(ValueError, match="max_score"):
            index.search(Q, 3, max_score=good, **kw)
        with pytest.raises(ValueError, match="max_score"):
            index.search_with_rank(Q, 3, torch.zeros(4, dtype=torch.int64), max_score=good, **kw)


def test_mine_argument_errors():
    from jodalrob_twotower_amd.hard_negatives import mine_hard_negatives, select_mined

    class Store(list):
        device = "cpu"
    ns, cs = Store(range(5)), Store(range(10))
    pairs = np.array([[0, 1]])
    for kw in ({"select": "best"}, {"k": 0}, {"k": 11}, {"k": 513}, {"per_notice": 0}, {"k": 4, "per_notice": 5}, {"chunk": 0},
               {"ceiling": 0.95}, {"ceiling": (1.0,)}):
        with pytest.raises(ValueError):
            mine_hard_negatives(None, ns, cs, pairs, **{"k": 8, "per_notice": 2, **kw})
    idx = torch.tensor([[4, 9, 2, -1, -1], [7, 1, 3, 5, 6], [-1, -1, -1, -1, -1]])
    assert select_mined(idx, 2, "top").tolist() == [[4, 9], [7, 1], [-1, -1]]
    g = torch.Generator().manual_seed(3)
    a = select_mined(idx, 4, "uniform", g)
    assert a.dtype == torch.int32 and sorted(a[0].tolist()) == [-1, 2, 4, 9] and a[0, 3] == -1
    assert set(a[1].tolist()) <= {7, 1, 3, 5, 6} and len(set(a[1].tolist())) == 4 and a[2].tolist() == [-1] * 4
    assert torch.equal(a, select_mined(idx, 4, "uniform", torch.Generator().manual_seed(3)))


# ---- the loader's draw, on the CPU ------------------------------------------------------------------------------------------------
def _cpu_loader(shuffle, **kw):
    from jodalrob_twotower_amd.data_loader import DeviceFeatureStore, DevicePairLoader
    rng = np.random.default_rng(4)
    nN, nC, P = 40, 200, 90
    ns = DeviceFeatureStore({"dense_projected": np.zeros((nN, 2), np.float32), "categorical": np.zeros((nN, 1), np.int64)}, ["a"], "cpu")
    cs = DeviceFeatureStore({"dense_projected": np.zeros((nC, 2), np.float32), "categorical": np.zeros((nC, 1), np.int64)}, ["b"], "cpu")
    pairs = np.stack([rng.integers(0, nN, P), rng.integers(0, nC, P)], 1)
    pairs[16:32, 0] = 39                                                   # batch 1 (unshuffled): one notice, nothing mined for it
    table = torch.as_tensor(rng.integers(0, nC, (nN, 3)), dtype=torch.int32)
    table[rng.random(nN) < 0.3] = -1
    table[:, 2] = -1
    table[39] = -1
    return DevicePairLoader(ns, cs, pairs, 16, shuffle=shuffle, seed=11, **kw), pairs, table


def test_loader_argument_errors():
    loader, pairs, table = _cpu_loader(True)
    with pytest.raises(ValueError):
        loader.set_extra_negatives(0, mined=table)
    with pytest.raises(ValueError):
        loader.set_extra_negatives(8, negative_pool=torch.arange(5), mined=table)
    for f in (0.0, -0.5, 1.5):
        with pytest.raises(ValueError):
            loader.set_extra_negatives(8, mined=table, hard_fraction=f)
    for bad in (table.long(), table[:-1], table[:, 0], table.tolist()):
        with pytest.raises(ValueError):
            loader.set_extra_negatives(8, mined=bad)
    with pytest.raises(KeyError):
        loader.set_extra_negatives(8, mined=torch.full_like(table, 200))
    loader.set_extra_negatives(8, mined=table)
    with pytest.raises(ValueError, match="order"):
        loader.epoch_negatives()                                           # shuffling: never draw for the wrong batches


@pytest.mark.parametrize("shuffle", [False, True])
@pytest.mark.parametrize("frac", [1.0, 0.5, 0.3])
def test_loader_draw_on_the_cpu(shuffle, frac):
    from jodalrob_twotower_amd.hard_negatives import MinedNegatives
    M = 10
    plain, pairs, table = _cpu_loader(shuffle, extra_negatives=M)
    loader, _, _ = _cpu_loader(shuffle, extra_negatives=M, mined=MinedNegatives(table, 8, 3, None, "top", 0), hard_fraction=frac)
    bare, _, _ = _cpu_loader(shuffle)
    H = int(round(frac * M))
    assert loader.hard_slots == H
    for epoch in range(2):
        order = loader.epoch_order()
        assert (order is None) == (not shuffle)
        if shuffle:
            assert torch.equal(order, bare.epoch_order())                  # a seed's pair order: that of a loader without extras
            plain.epoch_order()
        neg = loader.epoch_negatives(order)
        uni = plain.epoch_negatives()                                      # the same generator state: the uniform slots' bits
        assert neg.shape == (len(loader), M) and neg.dtype == torch.int64
        sel = pairs if order is None else pairs[order.numpy()]
        fell_back = 0
        for b in range(len(loader)):
            cands = R.batch_candidates(table.numpy(), sel[16 * b:16 * b + 16, 0])
            assert int(loader._epoch_cand[b]) == len(cands)
            if epoch == 0:                                                 # (later epochs: the mined draw has advanced the generator)
                assert torch.equal(neg[b, H:], uni[b, H:])
            if len(cands) == 0:
                fell_back += 1
                assert epoch > 0 or torch.equal(neg[b], uni[b])
            else:
                assert set(neg[b, :H].tolist()) <= set(cands.tolist())
            assert bool(((neg[b] >= 0) & (neg[b] < 200)).all())
        assert shuffle or fell_back == 1
