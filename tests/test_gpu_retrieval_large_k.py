"""GPU tests of catalogue-wide retrieval for 64 < k <= 512 (the sweep's and the merge's large-k forms): top-k against the f64
reference with the bars of test_gpu_retrieval.py, the first 64 columns of a k = 512 search bitwise the k = 64 search, index
tie-breaks more than 64 deep, bitwise determinism across runs and forced split counts with the rank of a k = 0 call, exclusion
lists and attribute filters at k = 128, graph capture, and the k = 513 error path."""
import numpy as np
import pytest
import torch

from test_gpu_retrieval import _check_topk, _ref_scores, _run, _unit
from test_gpu_retrieval_exclude import _check_rank_masked, _check_topk_masked, _dev, _mask
from test_gpu_retrieval_filter import _elig_mask, _random_filter
from test_gpu_retrieval_filter import _run as _run_masked
from test_retrieval_filter_host import ref_eligible

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def tt():
    import jodalrob_twotower_amd as m
    return m


@pytest.fixture(autouse=True)
def _auto_splits():
    yield
    from jodalrob_twotower_amd import _lib as L
    L.set_option(torch.device(DEV), L.TT_OPT_RETRIEVE_SPLITS, 0)


def _tol(bf16, inv_t):
    """test_gpu_retrieval.py's bars for the same tile routines."""
    return 1e-5 * max(1.0, inv_t) + 1e-6 if bf16 else 2e-6 * max(1.0, inv_t)


def _bits(a, b):
    return torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])


CASES = [  # nQ, nC, D, k, inv_t
    (1, 65, 32, 65, 1.0),          # nC == k == 65: the smallest large-k call
    (7, 129, 6, 128, 1.0),
    (7, 513, 100, 512, 0.05),
    (300, 1000, 64, 512, 0.05),    # more than half the catalogue
    (300, 1000, 256, 200, 1.0),
    (33, 65537, 64, 512, 1.0),
    (2100, 1000, 64, 128, 1.0),    # many query tiles (bf16 only)
]


@pytest.mark.parametrize("nQ,nC,D,k,inv_t,bf16", [c + (True,) for c in CASES] + [c + (False,) for c in CASES if c[0] != 2100])
def test_topk_vs_reference(tt, nQ, nC, D, k, inv_t, bf16):
    g = torch.Generator(device=DEV).manual_seed(nQ * 7 + nC + D + k)
    Q, Cm = _unit(nQ, D, g), _unit(nC, D, g)
    vals, idx = _run(tt, Q, Cm, k, inv_t, bf16)
    _check_topk(_ref_scores(Q, Cm, inv_t, bf16), vals, idx, k, _tol(bf16, inv_t))


@pytest.mark.parametrize("bf16", [True, False])
def test_first_64_columns_of_k512_are_bitwise_the_k64_search(tt, bf16):
    g = torch.Generator(device=DEV).manual_seed(12)
    Q, Cm = _unit(300, 64, g), _unit(20000, 64, g)
    small = _run(tt, Q, Cm, 64, 1.0, bf16)
    big = _run(tt, Q, Cm, 512, 1.0, bf16)
    assert big[0].shape == (300, 512)
    assert _bits((big[0][:, :64].contiguous(), big[1][:, :64].contiguous()), small)
    _check_topk(_ref_scores(Q, Cm, 1.0, bf16), big[0], big[1], 512, _tol(bf16, 1.0))


@pytest.mark.parametrize("bf16", [True, False])
def test_ties_deeper_than_64_come_in_ascending_index_order(tt, bf16):
    """Three base rows over 1000 catalogue rows (125, 375 and 500 copies), k = 200: a query's list is its best base row's copies in
    ascending index, then the next one's -- 125 + 75 where the best row is the rare one, else 200 copies of one row, so the index
    tie-break among equal keys has to place up to 200 of 375 or 500."""
    g = torch.Generator(device=DEV).manual_seed(3)
    base = _unit(3, 64, g)
    j = torch.arange(1000, device=DEV)
    which = torch.where(j % 8 == 0, 0, torch.where(j % 8 <= 3, 1, 2))
    Cm = base[which].contiguous()
    Q = _unit(50, 64, g)
    vals, idx = _run(tt, Q, Cm, 200, 1.0, bf16)
    B = _ref_scores(Q, base, 1.0, bf16)                                          # [50, 3]
    order = torch.argsort(B, dim=1, descending=True)
    srt = torch.gather(B, 1, order)
    clear = (srt[:, :-1] - srt[:, 1:]).min(dim=1).values > 10 * _tol(bf16, 1.0)  # the base rows' order is not in doubt
    assert float(clear.float().mean()) > 0.9
    copies = [torch.nonzero(which == b).flatten() for b in range(3)]
    seen_rare_first = False
    for q in torch.nonzero(clear).flatten().tolist():
        want = torch.cat([copies[b] for b in order[q].tolist()])[:200]
        assert torch.equal(idx[q], want), q
        n0 = min(200, copies[int(order[q, 0])].numel())
        assert bool((vals[q, :n0] == vals[q, 0]).all()) and (n0 == 200 or float(vals[q, n0]) < float(vals[q, 0]))
        seen_rare_first |= n0 < 200
    assert seen_rare_first
    _check_topk(_ref_scores(Q, Cm, 1.0, bf16), vals, idx, 200, _tol(bf16, 1.0))


@pytest.mark.parametrize("bf16", [True, False])
def test_bitwise_identical_across_runs_and_forced_splits(tt, bf16):
    from jodalrob_twotower_amd import _lib as L
    g = torch.Generator(device=DEV).manual_seed(5)
    Q, Cm = _unit(300, 64, g), _unit(20000, 64, g)
    Cm[5000:5300] = Cm[100:400]                                          # exact ties across splits, deeper than 64
    pos = torch.randint(0, 20000, (300,), generator=g, device=DEV)
    outs = []
    for s in (0, 0, 1, 2, 7, 32, 1000):                                  # (above 2048 / 200 = 10: clamped)
        L.set_option(torch.device(DEV), L.TT_OPT_RETRIEVE_SPLITS, s)
        outs.append(_run(tt, Q, Cm, 200, 1.0, bf16, positives=pos))
    for o in outs[1:]:
        assert _bits(o, outs[0]) and torch.equal(o[2], outs[0][2])
    L.set_option(torch.device(DEV), L.TT_OPT_RETRIEVE_SPLITS, 0)
    assert torch.equal(_run(tt, Q, Cm, 0, 1.0, bf16, positives=pos), outs[0][2])
    _check_topk(_ref_scores(Q, Cm, 1.0, bf16), outs[0][0], outs[0][1], 200, _tol(bf16, 1.0))


@pytest.mark.parametrize("bf16", [True, False])
def test_k128_lists_that_leave_fewer_than_k_rows(tt, bf16):
    g = torch.Generator(device=DEV).manual_seed(8)
    nQ, nC, k = 40, 1000, 128
    Q, Cm = _unit(nQ, 32, g), _unit(nC, 32, g)
    rng = np.random.default_rng(3)
    left = [(q * 13) % k for q in range(nQ)]                             # 0 .. 127 rows left, above and below 64
    assert min(left) == 0 and max(left) > 100
    keep = [np.sort(rng.choice(nC, j, replace=False)) for j in left]
    lists = [np.setdiff1d(np.arange(nC), kp) for kp in keep]
    off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    rows = np.concatenate(lists).astype(np.int32)
    vals, idx, _ = _run_masked(Q, Cm, k, 1.0, bf16, exclude=_dev(off, rows))
    for q in range(nQ):
        j = left[q]
        assert sorted(idx[q, :j].cpu().tolist()) == keep[q].tolist(), q
        assert bool((idx[q, j:] == -1).all()) and bool((vals[q, j:] == -float("inf")).all()), q
    _check_topk_masked(_mask(_ref_scores(Q, Cm, 1.0, bf16), off, rows), vals, idx, k, _tol(bf16, 1.0))


@pytest.mark.parametrize("score_dtype", ["bf16", "fp32"])
def test_k128_empty_exclusion_lists_are_bitwise_the_plain_search(tt, score_dtype):
    from jodalrob_twotower_amd.retrieval import CatalogIndex
    g = torch.Generator(device=DEV).manual_seed(9)
    Q, Cm = _unit(70, 64, g), _unit(1000, 64, g)
    index = CatalogIndex.from_embeddings(Cm, temperature=0.5, score_dtype=score_dtype)
    plain = index.search(Q, 128)
    empty = (torch.zeros(71, dtype=torch.int64, device=DEV), torch.zeros(0, dtype=torch.int32, device=DEV))
    assert _bits(index.search(Q, 128, exclude=empty), plain)
    _check_topk(_ref_scores(Q, Cm, 2.0, score_dtype == "bf16"), plain[0], plain[1], 128, _tol(score_dtype == "bf16", 2.0))


@pytest.mark.parametrize("bf16", [True, False])
@pytest.mark.parametrize("W", [1, 3])
def test_k128_filters_vs_masked_reference(tt, bf16, W):
    nQ, nC, k = 70, 1000, 128
    g = torch.Generator(device=DEV).manual_seed(20 + W)
    rng = np.random.default_rng(W)
    Q, Cm = _unit(nQ, 64, g), _unit(nC, 64, g)
    tags, any_m, all_m = _random_filter(nQ, nC, W, rng)
    any_m[1], all_m[1] = 0, tags[5]                                      # row 5 and hardly another: a list of -inf / -1
    any_m[2], all_m[2] = 0, 0xFFFFFFFF                                   # no eligible row
    pos = torch.as_tensor(rng.integers(0, nC, nQ), device=DEV)
    vals, idx, rank = _run_masked(Q, Cm, k, 1.0, bf16, positives=pos, filt=(tags, any_m, all_m))
    elig = ref_eligible(tags, any_m, all_m)
    assert 1 <= elig[1].sum() < 4 and elig[2].sum() == 0 and (elig[3:].sum(1) > k).mean() > 0.5
    S = _ref_scores(Q, Cm, 1.0, bf16)
    M = _elig_mask(S, elig)
    tol = _tol(bf16, 1.0)
    _check_topk_masked(M, vals, idx, k, tol)
    _check_rank_masked(S, M, pos, rank, tol)
    assert torch.equal(_run_masked(Q, Cm, 0, 1.0, bf16, positives=pos, filt=(tags, any_m, all_m))[2], rank)
    # through CatalogIndex: allow= / require= at k = 128 are the same call
    from jodalrob_twotower_amd.retrieval import CatalogIndex
    from test_gpu_retrieval_filter import _words
    index = CatalogIndex.from_embeddings(Cm, score_dtype="bf16" if bf16 else "fp32", tags=_words(tags))
    v2, i2 = index.search(Q, k, allow=_words(any_m), require=_words(all_m))
    assert _bits((v2, i2), (vals, idx))


def test_k128_search_can_be_captured_in_a_graph(tt):
    from jodalrob_twotower_amd.retrieval import CatalogIndex
    g = torch.Generator(device=DEV).manual_seed(4)
    Q, Cm = _unit(100, 64, g), _unit(5000, 64, g)
    index = CatalogIndex.from_embeddings(Cm, temperature=0.5, score_dtype="bf16")
    want = index.search(Q, 128)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        index.search(Q, 128)                                            # workspace of this stream exists before capture
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            got = index.search(Q, 128)
    torch.cuda.current_stream().wait_stream(s)
    graph.replay()
    torch.cuda.synchronize()
    assert _bits(got, want)


def test_k513_returns_nonzero_and_launches_nothing(tt):
    from jodalrob_twotower_amd import _lib as L
    lib, dev = L.load(), torch.device(DEV)
    ctx, st = L.ctx(dev), L.stream(dev)
    g = torch.Generator(device=DEV).manual_seed(1)
    Q, Cm = _unit(8, 32, g), _unit(1000, 32, g)
    assert lib.tt_retrieve_workspace_bytes(8, 1000, 32, 513) == 0
    ws = torch.empty(lib.tt_retrieve_workspace_bytes(8, 1000, 32, 512), dtype=torch.uint8, device=DEV)
    vals = torch.empty((8, 513), device=DEV)
    idx = torch.empty((8, 513), dtype=torch.int64, device=DEV)
    p = L.ptr
    from jodalrob_twotower_amd import ops
    q, c = ops.score_pack_bf16(Q, 1.0), ops.score_pack_bf16(Cm, 1.0)

    def f32(k):
        return lib.tt_retrieve_topk_f32(ctx, p(Q), 8, p(Cm), 1000, 32, 1.0, k, None, 1, p(vals), p(idx), None, p(ws), ws.numel(), st)

    assert f32(512) == 0, lib.tt_last_error_string()
    torch.cuda.synchronize()
    n0 = lib.tt_launch_count()
    assert f32(513) != 0
    assert lib.tt_retrieve_topk_bf16(ctx, p(q), 8, p(c), 1000, 32, 513, None, 0, p(vals), p(idx), None, p(ws), ws.numel(), st) != 0
    assert lib.tt_launch_count() == n0
