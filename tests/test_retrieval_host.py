"""Host-side tests of catalogue-wide retrieval (tt_retrieve_*, retrieval.CatalogIndex, TwoTowerEvaluator.evaluate_catalog):
the C ABI is declared and exported, the workspace size behaves, bad arguments are refused before any device call, and this
file's own numpy reference of the top-k order and the rank rule (which the GPU tests use) gives the expected answers."""
import re

import numpy as np
import pytest
import torch

from conftest import GOLD, ROOT
from jodalrob_twotower_amd import _lib

RETRIEVE_SYMBOLS = ("tt_retrieve_workspace_bytes", "tt_retrieve_topk_bf16", "tt_retrieve_topk_f32")


# ---- numpy reference (shared with tests/test_gpu_retrieval.py) ------------------------------------------------------------------
def ref_topk(S, k):
    """Per row: indices of the k best scores, value descending, ties to the lower index (tt_topk_rows's order)."""
    S = np.asarray(S)
    cols = np.arange(S.shape[1])
    return np.stack([np.lexsort((cols, -row))[:k] for row in S])


def ref_rank(S, positives):
    """#{c : s > s_p} + #{c < p : s == s_p} per row (tt_diag_rank_rows's rule)."""
    S = np.asarray(S)
    out = np.empty(S.shape[0], dtype=np.int64)
    for i, (row, p) in enumerate(zip(S, positives)):
        sp = row[p]
        out[i] = int((row > sp).sum() + (row[:p] == sp).sum())
    return out


def test_reference_topk_order_with_ties():
    S = np.array([[1.0, 3.0, 3.0, 2.0, 3.0],
                  [0.0, 0.0, 0.0, 0.0, 0.0],
                  [-1.0, 5.0, -1.0, 4.0, 5.0]])
    assert ref_topk(S, 3).tolist() == [[1, 2, 4], [0, 1, 2], [1, 4, 3]]
    assert ref_topk(S, 5)[2].tolist() == [1, 4, 3, 0, 2]


def test_reference_rank_rule_with_ties():
    S = np.array([[1.0, 3.0, 3.0, 2.0, 3.0],
                  [1.0, 3.0, 3.0, 2.0, 3.0],
                  [1.0, 3.0, 3.0, 2.0, 3.0],
                  [0.0, 0.0, 0.0, 0.0, 0.0]])
    # p = 2: one tie before it (col 1) counts, the tie after (col 4) does not; p = 3: three larger; p = 0: four larger
    assert ref_rank(S, [2, 3, 0, 4]).tolist() == [1, 3, 4, 4]
    assert ref_rank(S[:1], [1]).tolist() == [0]


# ---- C ABI ------------------------------------------------------------------------------------------------------------------------
def test_retrieve_symbols_declared_exported_and_bound():
    header = (ROOT / "include" / "twotower.h").read_text()
    declared = set(re.findall(r"^\s*(?:int|size_t)\s+(tt_retrieve\w+)\s*\(", header, flags=re.M))
    assert declared == set(RETRIEVE_SYMBOLS)
    lib = _lib.load()
    for name in RETRIEVE_SYMBOLS:
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert re.search(r"#define TT_OPT_RETRIEVE_SPLITS 9\b", header) and _lib.TT_OPT_RETRIEVE_SPLITS == 9
    assert lib.tt_abi_version() == 2


def test_workspace_bytes_positive_and_monotone():
    ws = _lib.load().tt_retrieve_workspace_bytes
    base = ws(300, 1000, 64, 10)
    assert base > 0 and ws(1, 1, 1, 0) > 0
    for nQ in (1, 7, 300, 8192, 100000):
        for nC in (1, 31, 33, 1000, 65537, 1 << 20):
            prev = 0
            for k in (0, 1, 10, 64):
                if k > nC:
                    continue
                b = ws(nQ, nC, 64, k)
                assert b > 0 and b >= prev, (nQ, nC, k)
                prev = b
    assert ws(301, 1000, 64, 10) >= base and ws(300, 1001, 64, 10) >= base and ws(300, 1000, 64, 11) >= base
    assert ws(300, 1 << 20, 64, 64) >= ws(300, 1 << 16, 64, 64) >= ws(300, 1000, 64, 64)
    # invalid shapes: 0
    assert ws(0, 10, 64, 1) == 0 and ws(10, 0, 64, 1) == 0 and ws(10, 10, 0, 1) == 0 and ws(10, 10, 257, 1) == 0
    assert ws(10, 10, 64, 65) == 0 and ws(10, 5, 64, 6) == 0 and ws(10, 10, 64, -1) == 0 and ws(10, 1 << 31, 64, 1) == 0


# ---- Python layer: refused before any device call (CPU tensors; the fp32 index keeps its rows as they are) --------------------
def test_catalog_index_rejects_bad_arguments():
    from jodalrob_twotower_amd.retrieval import CatalogIndex
    C = torch.randn(20, 16)
    idx = CatalogIndex.from_embeddings(C, temperature=0.5, score_dtype="fp32")
    assert len(idx) == 20 and idx.dim == 16 and idx.inv_t == 2.0
    Q = torch.randn(3, 16)
    for k in (0, -1, 65, 21):
        with pytest.raises(ValueError, match="k must be"):
            idx.search(Q, k)
    with pytest.raises(ValueError, match="dimension"):
        idx.search(torch.randn(3, 15), 5)
    with pytest.raises(ValueError, match="dimension"):
        idx.rank(torch.randn(3, 17), torch.zeros(3, dtype=torch.int64))
    with pytest.raises(ValueError, match="positives"):
        idx.rank(Q, torch.zeros(4, dtype=torch.int64))
    with pytest.raises(ValueError):
        CatalogIndex.from_embeddings(torch.randn(20, 300), score_dtype="fp32")
    with pytest.raises(ValueError):
        CatalogIndex.from_embeddings(torch.randn(0, 16), score_dtype="fp32")
    with pytest.raises(ValueError, match="score_dtype"):
        CatalogIndex.from_embeddings(C, score_dtype="int8")
    with pytest.raises(ValueError, match="temperature"):
        CatalogIndex.from_embeddings(C, temperature=0.0, score_dtype="fp32")


def test_fp8_index_falls_back_to_bf16():
    from jodalrob_twotower_amd.retrieval import CatalogIndex
    assert "falls back to bf16" in CatalogIndex.__doc__
    assert "fp8" in CatalogIndex.from_embeddings.__doc__


def test_evaluate_catalog_rejects_bad_arguments():
    import jodalrob_twotower_amd as tt
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
    wrong_d = CatalogIndex.from_embeddings(torch.randn(30, 16), score_dtype="fp32")
    pairs = np.array([[0, 1], [1, 2]])

    class NoStore:                                  # any use of the store would be a device call
        def gather(self, *_):
            raise AssertionError("the store was touched before the arguments were checked")

    with pytest.raises(ValueError, match="dimension"):
        ev.evaluate_catalog(task, NoStore(), wrong_d, pairs)
    with pytest.raises(ValueError, match="ks"):
        ev.evaluate_catalog(task, NoStore(), good, pairs, ks=(0, 5))
    with pytest.raises(ValueError, match="pairs"):
        ev.evaluate_catalog(task, NoStore(), good, np.zeros((3, 3), np.int64))
    with pytest.raises(ValueError, match="company rows"):
        ev.evaluate_catalog(task, NoStore(), good, np.array([[0, 30]]))
    with pytest.raises(TypeError):
        ev.evaluate_catalog(task, NoStore(), torch.randn(30, 8), pairs)
    with pytest.raises(ValueError, match="k must be"):
        task.predict_catalog({"dense": torch.zeros(2, 8)}, good, top_k=65)
    with pytest.raises(ValueError, match="dimension"):
        task.predict_catalog({"dense": torch.zeros(2, 8)}, wrong_d, top_k=5)
