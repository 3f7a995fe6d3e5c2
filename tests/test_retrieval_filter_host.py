"""Host-side tests of per-query attribute filters in catalogue-wide retrieval (tt_filt_retrieve_topk_*, CatalogIndex tags= /
allow= / require=): the two C entries declared, exported and bound, this file's numpy reference of eligibility and of the
masked top-k and rank (which the GPU tests use), the onehot_bits / equality_bits helpers against plain loops, and the Python
layer refusing bad tags and masks before any device call."""
import re

import numpy as np
import pytest
import torch

from conftest import GOLD, ROOT
from jodalrob_twotower_amd import _lib
from test_retrieval_host import ref_rank, ref_topk

FILT_SYMBOLS = ("tt_filt_retrieve_topk_bf16", "tt_filt_retrieve_topk_f32")


# ---- numpy reference (shared with tests/test_gpu_retrieval_filter.py) -----------------------------------------------------------
def ref_eligible(tags, any_mask=None, all_mask=None):
    """bool [nQ, nC]: row c is eligible for query q when it shares a bit with a non-zero any[q] and holds every bit of all[q].
    tags [nC, W], masks [nQ, W] (or None: always true), any integer dtype; only the low 32 bits of a word count."""
    tags = np.asarray(tags).astype(np.int64) & 0xFFFFFFFF
    nQ = len(any_mask if any_mask is not None else all_mask)
    ok = np.ones((nQ, tags.shape[0]), dtype=bool)
    if any_mask is not None:
        a = np.asarray(any_mask).astype(np.int64) & 0xFFFFFFFF
        shares = ((tags[None, :, :] & a[:, None, :]) != 0).any(2)
        ok &= shares | (a == 0).all(1)[:, None]
    if all_mask is not None:
        r = np.asarray(all_mask).astype(np.int64) & 0xFFFFFFFF
        ok &= ((tags[None, :, :] & r[:, None, :]) == r[:, None, :]).all(2)
    return ok


def ref_topk_masked(S, elig, k):
    """ref_topk over the eligible rows only: indices [nQ, k], -1 in the slots beyond a query's eligible rows."""
    S = np.asarray(S, dtype=np.float64)
    idx = ref_topk(np.where(elig, S, -np.inf), k)
    n = elig.sum(1)
    return np.where(np.arange(k)[None, :] < n[:, None], idx, -1)


def ref_rank_masked(S, elig, positives):
    """#{eligible c : s > s_p} + #{eligible c < p : s == s_p}; the positive never counts, eligible or not."""
    S = np.asarray(S, dtype=np.float64)
    out = np.empty(S.shape[0], dtype=np.int64)
    for i, (row, p) in enumerate(zip(S, positives)):
        m = np.where(elig[i], row, -np.inf)
        m[p] = row[p]                                   # (p counts in neither term; keep s_p where ref_rank reads it)
        out[i] = ref_rank(m[None, :], [p])[0]
    return out


def test_reference_on_a_hand_made_case():
    #           c: 0     1     2     3     4     5
    tags = np.array([[0b001], [0b011], [0b010], [0b100], [0b111], [0b000]])
    S = np.array([[3.0, 3.0, 2.0, 3.0, 3.0, 9.0]] * 5)
    any_m = np.array([[0b000], [0b001], [0b110], [0b000], [0b1000]])
    all_m = np.array([[0b000], [0b000], [0b010], [0b101], [0b000]])
    e = ref_eligible(tags, any_m, all_m)
    assert e.astype(int).tolist() == [[1, 1, 1, 1, 1, 1],      # no restriction
                                      [1, 1, 0, 0, 1, 0],      # shares bit 0
                                      [0, 1, 1, 0, 1, 0],      # shares bit 1 or 2, and holds bit 1
                                      [0, 0, 0, 0, 1, 0],      # holds bits 0 and 2
                                      [0, 0, 0, 0, 0, 0]]      # shares a bit nobody has: no eligible row
    assert ref_eligible(tags, any_m, None)[2].astype(int).tolist() == [0, 1, 1, 1, 1, 0]
    assert ref_eligible(tags, None, all_m)[2].astype(int).tolist() == [0, 1, 1, 0, 1, 0]
    # top-k: exact ties (3.0 at c = 0, 1, 3, 4) next to ineligible rows go to the lower index; -1 beyond the eligible rows
    assert ref_topk_masked(S, e, 3).tolist() == [[5, 0, 1], [0, 1, 4], [1, 4, 2], [4, -1, -1], [-1, -1, -1]]
    # rank of p = 4 (s_p = 3): the eligible ties before it count, the ineligible ones and the ineligible 9.0 do not
    assert ref_rank_masked(S, e, [4] * 5).tolist() == [4, 2, 1, 0, 0]
    # an ineligible positive is ranked all the same: p = 3 for query 1 -> ties at 0 and 1 before it
    assert ref_rank_masked(S, e, [3] * 5).tolist() == [3, 2, 1, 0, 0]
    # only the low 32 bits of a word count, whatever the dtype
    assert ref_eligible(np.array([[-1]], np.int32), np.array([[1 << 31]], np.int64), None).tolist() == [[True]]


# ---- C ABI ------------------------------------------------------------------------------------------------------------------------
def test_filter_symbols_declared_exported_and_bound():
    header = (ROOT / "include" / "twotower.h").read_text()
    declared = set(re.findall(r"^\s*int\s+(tt_filt_retrieve\w+)\s*\(", header, flags=re.M))
    assert declared == set(FILT_SYMBOLS)
    lib = _lib.load()
    for name in FILT_SYMBOLS:
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        args = _lib.SIGNATURES[name][1]
        excl = _lib.SIGNATURES[name.replace("tt_filt_retrieve", "tt_excl_retrieve")][1]
        assert args[:-7] == excl[:-3] and args[-3:] == excl[-3:]    # the exclusion entry's, with tags, W, q_any, q_all after
        assert args[-7:-3] == [_lib.vp, _lib.i32, _lib.vp, _lib.vp]   # excl_rows
    assert "tags[c,w] & any[q,w] != 0" in header and "tags[c,w] & all[q,w] == all[q,w]" in header
    assert lib.tt_abi_version() == 2


# ---- onehot_bits / equality_bits against plain loops ----------------------------------------------------------------------------
def loop_onehot(codes, n_values, first_bit, W):
    out = np.zeros((len(codes), W), dtype=np.uint32)
    for i, c in enumerate(codes):
        if c >= 0:
            b = first_bit + int(c)
            out[i, b // 32] |= np.uint32(1 << (b % 32))
    return out


def loop_equality(codes, n_values, first_bit, W):
    nb = max(1, int(np.ceil(np.log2(n_values)))) if n_values > 1 else 1
    out = np.zeros((len(codes), W), dtype=np.uint32)
    for i, c in enumerate(codes):
        if c < 0:
            continue
        for j in range(nb):
            b = first_bit + (j if (int(c) >> j) & 1 else nb + j)
            out[i, b // 32] |= np.uint32(1 << (b % 32))
    return out


def _u32(t):
    return t.numpy().view(np.uint32)


@pytest.mark.parametrize("V", [1, 2, 3, 315, 3680])
def test_bit_helpers_match_plain_loops(V):
    from jodalrob_twotower_amd.retrieval import equality_bits, onehot_bits
    rng = np.random.default_rng(V)
    codes = np.concatenate([[0, V - 1, -1, -7], rng.integers(-2, V, 200)])
    t = torch.as_tensor(codes)
    nb = 2 * max(1, (V - 1).bit_length())
    for first in (0, 5, 27, 31, 60):
        W = (first + nb + 31) // 32
        got = equality_bits(t, V, first_bit=first)
        assert got.dtype == torch.int32 and got.shape == (len(codes), W) and got.is_contiguous()
        assert np.array_equal(_u32(got), loop_equality(codes, V, first, W))
        assert np.array_equal(_u32(equality_bits(t.to(torch.int32), V, first_bit=first, words=4)), loop_equality(codes, V, first, 4))
        if first + V <= 128:
            W1 = (first + V + 31) // 32
            one = onehot_bits(t, V, first_bit=first)
            assert one.dtype == torch.int32 and one.shape == (len(codes), W1)
            assert np.array_equal(_u32(one), loop_onehot(codes, V, first, W1))
            assert np.array_equal(_u32(onehot_bits(t, V, first_bit=first, words=4)), loop_onehot(codes, V, first, 4))
    assert not _u32(equality_bits(torch.tensor([-1, -5]), V)).any()         # negative: zero bits
    assert not _u32(onehot_bits(torch.tensor([-1, -5]), min(V, 128))).any()


def test_bit_helpers_cross_a_word_boundary_and_combine():
    from jodalrob_twotower_amd.retrieval import equality_bits, onehot_bits
    one = onehot_bits(torch.tensor([0, 3, 4]), 8, first_bit=28)              # bits 28 .. 35
    assert _u32(one).tolist() == [[1 << 28, 0], [1 << 31, 0], [0, 1]]
    eq = equality_bits(torch.tensor([5]), 6, first_bit=30)                   # 3 digits: bits 30, 31, 32; complements 33, 34, 35
    assert _u32(eq).tolist() == [[1 << 30, 0b0101]]                          # 5 = 101b: digits 0 and 2 set, complement of digit 1
    both = equality_bits(torch.tensor([2, 1]), 4, first_bit=0, words=2) | onehot_bits(torch.tensor([1, 0]), 40, first_bit=4, words=2)
    assert _u32(both).tolist() == [[0b0110 | (1 << 5), 0], [0b1001 | (1 << 4), 0]]


def test_bit_helpers_refuse_bad_codes_and_overflow():
    from jodalrob_twotower_amd.retrieval import equality_bits, onehot_bits
    for fn in (onehot_bits, equality_bits):
        with pytest.raises(ValueError, match="n_values"):
            fn(torch.tensor([0, 5]), 5)                                      # code >= n_values
        with pytest.raises(ValueError, match="fit"):
            fn(torch.tensor([0]), 40, first_bit=120)                         # past 128 bits
        with pytest.raises(ValueError, match="fit"):
            fn(torch.tensor([0]), 40, first_bit=30, words=1)                 # past the words asked for
        with pytest.raises(ValueError, match="fit"):
            fn(torch.tensor([0]), 4, words=5)
        with pytest.raises(ValueError, match="integer"):
            fn(torch.tensor([0.5]), 4)
        with pytest.raises(ValueError):
            fn(torch.tensor([0]), 0)
    with pytest.raises(ValueError, match="fit"):
        onehot_bits(torch.tensor([0]), 129)
    assert onehot_bits(torch.tensor([127]), 128).shape == (1, 4)
    assert equality_bits(torch.tensor([3679]), 3680, first_bit=104).shape == (1, 4)       # 24 bits end at bit 128
    with pytest.raises(ValueError, match="fit"):
        equality_bits(torch.tensor([3679]), 3680, first_bit=105)


def test_equality_bits_all_match_is_exactly_code_equality():
    from jodalrob_twotower_amd.retrieval import equality_bits
    V = 37
    codes = torch.arange(V)
    for first in (0, 26):                                                    # the second field crosses a word boundary
        enc = equality_bits(codes, V, first_bit=first)
        e = ref_eligible(enc.numpy(), None, enc.numpy())
        assert np.array_equal(e, np.eye(V, dtype=bool))
    # a "don't care" query matches every row; a row without bits matches only "don't care"
    q = equality_bits(torch.tensor([-1, 4]), V)
    rows = equality_bits(torch.tensor([4, -1, 5]), V)
    assert ref_eligible(rows.numpy(), None, q.numpy()).tolist() == [[True, True, True], [True, False, False]]


# ---- Python layer: refused before any device call ---------------------------------------------------------------------------------
def test_catalog_index_rejects_bad_tags_and_masks():
    from jodalrob_twotower_amd.retrieval import CatalogIndex
    C = torch.randn(20, 16)
    for bad in (torch.zeros(19, dtype=torch.int32), torch.zeros((20, 5), dtype=torch.int32), torch.zeros((20, 0), dtype=torch.int32),
                torch.zeros(20), torch.zeros((20, 1, 1), dtype=torch.int32), [0] * 20, torch.zeros(20, dtype=torch.bool)):
        with pytest.raises(ValueError, match="tags"):
            CatalogIndex.from_embeddings(C, score_dtype="fp32", tags=bad)
    plain = CatalogIndex.from_embeddings(C, score_dtype="fp32")
    assert plain.tags is None and plain.tag_words == 0
    idx = CatalogIndex.from_embeddings(C, score_dtype="fp32", tags=torch.arange(40).reshape(20, 2))
    assert idx.tags.dtype == torch.int32 and idx.tags.shape == (20, 2) and idx.tags.is_contiguous() and idx.tag_words == 2
    one = CatalogIndex(C, 1.0, "fp32", tags=torch.tensor([2 ** 32 - 1] * 20))
    assert one.tags.shape == (20, 1) and bool((one.tags == -1).all())        # the bit pattern is kept
    Q, pos = torch.randn(3, 16), torch.zeros(3, dtype=torch.int64)
    ok = torch.zeros((3, 2), dtype=torch.int32)
    with pytest.raises(ValueError, match="tags="):
        plain.search(Q, 5, allow=ok)
    with pytest.raises(ValueError, match="tags="):
        plain.rank(Q, pos, require=ok)
    for bad in (torch.zeros((4, 2), dtype=torch.int32), torch.zeros((3, 1), dtype=torch.int32), torch.zeros(3, dtype=torch.int32),
                torch.zeros((3, 2)), torch.zeros((3, 2), dtype=torch.bool), [[0, 0]] * 3):
        with pytest.raises(ValueError, match="allow"):
            idx.search(Q, 5, allow=bad)
        with pytest.raises(ValueError, match="require"):
            idx.search_with_rank(Q, 5, pos, require=bad)
        with pytest.raises(ValueError, match="require"):
            idx.rank(Q, pos, allow=ok, require=bad)
    filt = idx._check_filter(None, torch.tensor([[1, 2 ** 32 - 1]] * 3), 3)
    assert filt[0] is idx.tags and filt[1] == 2 and filt[2] is None and filt[3].tolist() == [[1, -1]] * 3
    assert idx._check_filter(None, None, 3) is None
    assert one._check_filter(torch.tensor([1, 2, 3]), None, 3)[2].shape == (3, 1)        # [nQ] masks for W = 1


def test_evaluate_catalog_and_predict_catalog_reject_bad_masks():
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
    untagged = CatalogIndex.from_embeddings(torch.randn(30, 8), score_dtype="fp32")
    tagged = CatalogIndex.from_embeddings(torch.randn(30, 8), score_dtype="fp32", tags=torch.arange(30))
    pairs = np.array([[0, 1], [1, 2]])
    good, short = torch.zeros(2, dtype=torch.int64), torch.zeros(3, dtype=torch.int64)

    class NoStore:                                  # any use of the store would be a device call
        def gather(self, *_):
            raise AssertionError("the store was touched before the arguments were checked")

    class NoTower(dict):                            # any use of the batch would run the tower
        def __getitem__(self, key):
            raise AssertionError("the batch was touched before the arguments were checked")

    with pytest.raises(ValueError, match="tags="):
        ev.evaluate_catalog(task, NoStore(), untagged, pairs, require=good)
    with pytest.raises(ValueError, match="allow"):
        ev.evaluate_catalog(task, NoStore(), tagged, pairs, allow=short)
    with pytest.raises(ValueError, match="require"):
        ev.evaluate_catalog(task, NoStore(), tagged, pairs, allow=good, require=torch.zeros((2, 2), dtype=torch.int32))
    with pytest.raises(ValueError, match="tags="):
        task.predict_catalog(NoTower(dense=None), untagged, top_k=5, allow=good)
    with pytest.raises(ValueError, match="require"):
        task.predict_catalog(NoTower(dense=None), tagged, top_k=5, require=torch.zeros(2))
    with pytest.raises(ValueError, match="allow"):
        task.predict_catalog(NoTower(dense=None), tagged, top_k=5, allow=torch.zeros((2, 3), dtype=torch.int32))
