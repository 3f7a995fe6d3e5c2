"""Host-side tests of per-query exclusion lists in catalogue-wide retrieval: retrieval.exclusions_from_pairs against a dict
reference, CatalogIndex's checks of `exclude` (refused before any device call), the masked reference of the top-k order and
the rank rule next to exact ties, and the two C entries being declared, exported and bound."""
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from jodalrob_twotower_amd import _lib
from test_retrieval_host import ref_rank, ref_topk

EXCL_SYMBOLS = ("tt_excl_retrieve_topk_bf16", "tt_excl_retrieve_topk_f32")


# ---- masked numpy reference (shared with tests/test_gpu_retrieval_exclude.py) ---------------------------------------------------
def masked_scores(S, offsets, rows):
    """S with every query's excluded rows set to -inf (rows outside [0, nC) match nothing)."""
    S = np.array(S, dtype=np.float64, copy=True)
    offsets, rows = np.asarray(offsets), np.asarray(rows)
    for q in range(S.shape[0]):
        r = rows[offsets[q]:offsets[q + 1]]
        r = r[(r >= 0) & (r < S.shape[1])]
        S[q, r] = -np.inf
    return S


def ref_topk_excl(S, k, offsets, rows):
    """(idx, n_eligible): idx as ref_topk over the eligible rows, -1 past the eligible ones."""
    M = masked_scores(S, offsets, rows)
    idx = ref_topk(M, k)
    elig = np.isfinite(M).sum(1)
    idx = np.where(np.arange(k)[None, :] < elig[:, None], idx, -1)
    return idx, elig


def ref_rank_excl(S, positives, offsets, rows):
    """#{c not in E : s > s_p} + #{c not in E, c < p : s == s_p}: ref_rank on the masked scores with s_p from the unmasked
    ones (p never counts against itself, in E or not)."""
    S = np.asarray(S, dtype=np.float64)
    M = masked_scores(S, offsets, rows)
    out = np.empty(S.shape[0], dtype=np.int64)
    for i, p in enumerate(positives):
        sp = S[i, p]
        row = M[i]
        out[i] = int((row > sp).sum() + (row[:p] == sp).sum())
    return out


def test_masked_reference_with_ties_next_to_excluded_rows():
    S = np.array([[1.0, 3.0, 3.0, 2.0, 3.0],
                  [1.0, 3.0, 3.0, 2.0, 3.0],
                  [0.0, 0.0, 0.0, 0.0, 0.0]])
    off = np.array([0, 1, 3, 7])
    rows = np.array([2, 1, 4, 0, 1, 2, 3])                   # q0 {2}; q1 {1, 4}; q2 all but row 4
    idx, elig = ref_topk_excl(S, 3, off, rows)
    assert idx.tolist() == [[1, 4, 3], [2, 3, 0], [4, -1, -1]] and elig.tolist() == [4, 3, 1]
    # no exclusions: the plain reference
    assert np.array_equal(ref_topk_excl(S, 3, np.zeros(4, int), np.zeros(0, int))[0], ref_topk(S, 3))
    assert np.array_equal(ref_rank_excl(S, [2, 3, 4], np.zeros(4, int), np.zeros(0, int)), ref_rank(S, [2, 3, 4]))
    # q0, p = 4: ties before it at 1 (counts) and 2 (excluded) -> 1; q1, p = 2: tie at 1 excluded, 4 after p -> 0;
    # q2, p = 4: rows 0..3 tie before p but are excluded -> 0
    assert ref_rank_excl(S, [4, 2, 4], off, rows).tolist() == [1, 0, 0]
    # p in its own list changes nothing: q0 p = 2 (in {2}), q1 p = 1 (in {1, 4}), q2 p = 0 (in {0, 1, 2, 3})
    assert ref_rank_excl(S, [2, 1, 0], off, rows).tolist() == [1, 0, 0]
    assert ref_rank_excl(S, [2, 1, 0], [0, 0, 1, 4], [4, 1, 2, 3]).tolist() == [1, 0, 0]
    # out-of-range rows match nothing
    assert np.array_equal(ref_topk_excl(S, 3, [0, 2, 2, 3], [-1, 5, 99])[0], ref_topk(S, 3))


# ---- exclusions_from_pairs ------------------------------------------------------------------------------------------------------
def _dict_reference(keys, pairs):
    known = {}
    for n, c in pairs:
        known.setdefault(int(n), set()).add(int(c))
    lists = [sorted(known.get(int(k), ())) for k in keys]
    off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    return off, np.array([c for x in lists for c in x], dtype=np.int32)


def test_exclusions_from_pairs_matches_dict_reference():
    from jodalrob_twotower_amd.retrieval import exclusions_from_pairs
    rng = np.random.default_rng(0)
    pairs = np.stack([rng.integers(0, 40, 500), rng.integers(0, 100, 500)], 1)
    pairs = np.concatenate([pairs, pairs[:50], pairs[::-7]])          # duplicate pairs, unsorted
    keys = np.concatenate([rng.integers(0, 50, 60), [3, 3, 45, 49]])   # repeated keys, keys without pairs (>= 40)
    off, rows = exclusions_from_pairs(torch.as_tensor(keys), torch.as_tensor(pairs), 100)
    want_off, want_rows = _dict_reference(keys, pairs)
    assert off.dtype == torch.int64 and rows.dtype == torch.int32
    assert np.array_equal(off.numpy(), want_off) and np.array_equal(rows.numpy(), want_rows)
    assert (np.diff(want_off) == 0).any()                             # some queries have empty lists


def test_exclusions_from_pairs_edges():
    from jodalrob_twotower_amd.retrieval import exclusions_from_pairs
    off, rows = exclusions_from_pairs(torch.tensor([1, 2]), torch.zeros((0, 2), dtype=torch.int64), 10)
    assert off.tolist() == [0, 0, 0] and rows.numel() == 0
    off, rows = exclusions_from_pairs(torch.tensor([7]), torch.tensor([[7, 9], [7, 0], [7, 9], [8, 3]]), 10)
    assert off.tolist() == [0, 2] and rows.tolist() == [0, 9]
    with pytest.raises(ValueError, match=r"\[0, 10\)"):
        exclusions_from_pairs(torch.tensor([1]), torch.tensor([[1, 10]]), 10)
    with pytest.raises(ValueError, match=r"\[0, 10\)"):
        exclusions_from_pairs(torch.tensor([1]), torch.tensor([[1, -1]]), 10)
    with pytest.raises(ValueError, match="pairs"):
        exclusions_from_pairs(torch.tensor([1]), torch.zeros((3, 3), dtype=torch.int64), 10)


# ---- CatalogIndex: refused before any device call -------------------------------------------------------------------------------
def test_catalog_index_rejects_bad_exclusions():
    from jodalrob_twotower_amd.retrieval import CatalogIndex
    index = CatalogIndex.from_embeddings(torch.randn(20, 16), score_dtype="fp32")
    Q = torch.randn(3, 16)
    pos = torch.zeros(3, dtype=torch.int64)
    good_rows = torch.tensor([1, 2], dtype=torch.int32)
    bad = [
        (torch.tensor([0, 1, 2], dtype=torch.int64), good_rows),          # offsets shape (nQ,) not (nQ + 1,)
        (torch.tensor([[0, 1, 2, 2]], dtype=torch.int64), good_rows),     # 2-D offsets
        (torch.tensor([0, 1, 2, 2], dtype=torch.int32), good_rows),       # int32 offsets
        (torch.tensor([0, 1, 2, 2], dtype=torch.int64), good_rows.float()),  # float rows
        (torch.tensor([0, 1, 2, 2], dtype=torch.int64), good_rows[None]),  # 2-D rows
        (torch.tensor([0, 1, 2, 2], dtype=torch.int64), good_rows, None),  # not a pair
    ]
    for ex in bad:
        for call in (lambda: index.search(Q, 5, exclude=ex), lambda: index.rank(Q, pos, exclude=ex),
                     lambda: index.search_with_rank(Q, 5, pos, exclude=ex)):
            with pytest.raises(ValueError, match="exclude"):
                call()
    # device mismatch: a meta-device tensor stands in for "not the catalogue's device"
    with pytest.raises(ValueError, match="catalogue on"):
        index.search(Q, 5, exclude=(torch.zeros(4, dtype=torch.int64, device="meta"), good_rows))
    with pytest.raises(ValueError, match="catalogue on"):
        index.search(Q, 5, exclude=(torch.zeros(4, dtype=torch.int64), good_rows.to("meta")))


def test_catalog_index_canonicalises_caller_lists():
    from jodalrob_twotower_amd.retrieval import CatalogIndex
    index = CatalogIndex.from_embeddings(torch.randn(20, 16), score_dtype="fp32")
    off = torch.tensor([0, 3, 3, 6], dtype=torch.int64)
    rows = torch.tensor([9, 2, 5, 19, 0, 7], dtype=torch.int64)
    o, r = index._check_exclude((off, rows), 3)
    assert torch.equal(o, off) and r.dtype == torch.int32 and r.tolist() == [2, 5, 9, 0, 7, 19]
    # int64 rows beyond int32 stay outside [0, nC) instead of wrapping into it
    o, r = index._check_exclude((torch.tensor([0, 2], dtype=torch.int64), torch.tensor([(1 << 32) + 3, -(1 << 40)])), 1)
    assert r.tolist() == [-1, 20]


def test_evaluate_catalog_rejects_bad_filter_pairs():
    import jodalrob_twotower_amd as tt
    from conftest import GOLD
    from jodalrob_twotower_amd.retrieval import CatalogIndex
    kw = dict(notice_table="notice", company_table="company", pair_table="p", pair_notice_id_cols=["a"],
              pair_company_id_cols=["b"])
    schema = tt.build_torchrec_schema_from_meta(metadata_path=GOLD / "synthetic_metadata.csv", **kw)
    task = tt.create_two_tower_train_task(schema.notice.categorical, schema.company.categorical,
                                          metadata_path=str(GOLD / "synthetic_metadata.csv"), categorical_embedding_dim=4,
                                          notice_dense_input_dim=8, company_dense_input_dim=8, tower_hidden_dims=[8, 8],
                                          final_embedding_dim=8, device="cpu")
    ev = tt.TwoTowerEvaluator(device="cpu")
    good = CatalogIndex.from_embeddings(torch.randn(30, 8), score_dtype="fp32")

    class NoStore:
        def gather(self, *_):
            raise AssertionError("the store was touched before the arguments were checked")

    with pytest.raises(ValueError, match="filter_pairs"):
        ev.evaluate_catalog(task, NoStore(), good, np.array([[0, 1]]), filter_pairs=np.zeros((3, 3), np.int64))


# ---- C ABI ----------------------------------------------------------------------------------------------------------------------
def test_exclusion_symbols_declared_exported_and_bound():
    header = (ROOT / "include" / "twotower.h").read_text()
    declared = set(re.findall(r"^\s*int\s+(tt_excl_retrieve\w+)\s*\(", header, flags=re.M))
    assert declared == set(EXCL_SYMBOLS)
    lib = _lib.load()
    for name in EXCL_SYMBOLS:
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        args = _lib.SIGNATURES[name][1]
        plain = _lib.SIGNATURES[name.replace("tt_excl_retrieve", "tt_retrieve")][1]
        assert args == plain[:-3] + [_lib.vp, _lib.vp] + plain[-3:]     # excl_offsets, excl_rows after rank
    assert lib.tt_abi_version() == 2
