"""Host-side tests of catalogue-wide retrieval for 64 < k <= 512: CatalogIndex's argument checks take the wider range, and the
workspace of a k > 64 call exists and never exceeds the k = 64 one of the same shape (the split cap S k <= 2048)."""
import pytest
import torch

from jodalrob_twotower_amd import _lib

LARGE_K = (65, 128, 200, 512)


def test_catalog_index_accepts_k_up_to_512_as_far_as_argument_checks_go():
    from jodalrob_twotower_amd import retrieval
    from jodalrob_twotower_amd.retrieval import CatalogIndex
    assert retrieval.MAX_K == 512
    idx = CatalogIndex.from_embeddings(torch.randn(600, 16), temperature=0.5, score_dtype="fp32")
    for k in (65, 512):
        assert idx._check_k(k) == k
    Q = torch.randn(3, 16)
    for k in (513, 601, 1000):
        with pytest.raises(ValueError, match="k must be"):
            idx.search(Q, k)
        with pytest.raises(ValueError, match="k must be"):
            idx.search_with_rank(Q, k, torch.zeros(3, dtype=torch.int64))
    small = CatalogIndex.from_embeddings(torch.randn(100, 16), score_dtype="fp32")
    assert small._check_k(100) == 100
    with pytest.raises(ValueError, match="k must be"):                        # k > size below the cap
        small.search(Q, 101)


def test_workspace_bytes_positive_up_to_512():
    ws = _lib.load().tt_retrieve_workspace_bytes
    for k in LARGE_K:
        for nC in (k, k + 1, 1000, 1 << 20):
            assert ws(300, nC, 64, k) > 0, (nC, k)
    assert ws(300, 1000, 64, 513) == 0 and ws(300, 1 << 20, 64, 513) == 0 and ws(300, 1 << 20, 64, 1 << 20) == 0
    assert ws(300, 511, 64, 512) == 0 and ws(10, 10, 64, 65) == 0                 # k > nC stays invalid


def test_workspace_of_large_k_never_exceeds_the_k64_one():
    """S k <= 2048 = 32 x 64 for k > 64, so the partial lists of a call are never larger than those of the same call at k = 64
    (nQ S k 8 bytes would otherwise reach 1 GB at nQ = 8192, nC = 1 M, k = 512)."""
    ws = _lib.load().tt_retrieve_workspace_bytes
    for nQ in (1, 7, 300, 8192, 100000):
        for nC in (1000, 65537, 1 << 20):                                        # the monotonicity grid's nC >= 512
            base = ws(nQ, nC, 64, 64)
            assert base > 0
            for k in LARGE_K:
                b = ws(nQ, nC, 64, k)
                assert 0 < b <= base, (nQ, nC, k, b, base)
    # between 512 and 1023 rows a k = 64 call has fewer than 32 splits: the cap follows it
    for nC in (512, 600, 777, 1023):
        for k in LARGE_K:
            assert 0 < ws(300, nC, 64, k) <= ws(300, nC, 64, 64), (nC, k)
    assert ws(8192, 1 << 20, 64, 512) <= 8192 * 2048 * 8 + 8192 * 33 * 4 + 4 * 256
