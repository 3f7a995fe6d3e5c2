"""GPU tests of hard-negative mining: the sweep's per-query score ceiling (tt_ceil_retrieve_topk_bf16 / _f32) against the masked
f64 reference of tests/_mine_reference.py and bit for bit against the plain entry, its edge ceilings, the untouched rank, split
counts, tt_pair_scores_*, graph capture and the error paths; then mine_hard_negatives end to end, the loader's mined extras, and
the captured step on such batches against the eager one."""
import numpy as np
import pytest
import torch

import _mine_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INF, NAN = float("inf"), float("nan")


@pytest.fixture(scope="module")
def tt():
    import jodalrob_twotower_amd as m
    return m


@pytest.fixture(autouse=True)
def _auto_splits():
    yield
    from jodalrob_twotower_amd import _lib as L
    L.set_option(torch.device(DEV), L.TT_OPT_RETRIEVE_SPLITS, 0)


def _unit(n, d, g):
    x = torch.randn((n, d), generator=g, device=DEV, dtype=torch.float32)
    return x / x.norm(dim=1, keepdim=True)


def _run(Q, Cm, k, inv_t, bf16, positives=None, exclude=None, ceil=None):
    """(vals, idx, rank) from one ops-level call; ceil=None runs the plain / exclusion entry"""
    from jodalrob_twotower_amd import ops
    nQ, D = Q.shape
    nC = Cm.shape[0]
    if bf16:
        q, c = ops.score_pack_bf16(Q, 1.0), ops.score_pack_bf16(Cm, inv_t)
        out = ops._retrieve(q, nQ, c, nC, D, k, 1.0, True, positives, None, exclude, None, ceil)
    else:
        out = ops._retrieve(Q, nQ, Cm, nC, D, k, inv_t, False, positives, None, exclude, None, ceil)
    torch.cuda.synchronize()
    return out


def _dev(off, rows):
    return torch.as_tensor(off, device=DEV), torch.as_tensor(rows, device=DEV)


def _same(a, b):
    """bitwise equal (vals, idx[, rank]) results"""
    ranks = len(a) > 2 and len(b) > 2 and a[2] is not None and b[2] is not None
    return (torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])
            and (not ranks or torch.equal(a[2], b[2])))


# ---- 1. against the masked f64 reference -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lists", [False, True])
@pytest.mark.parametrize("bf16", [True, False])
@pytest.mark.parametrize("nQ,nC,D,k,inv_t", R.CASES)
def test_ceiling_topk_vs_masked_reference(tt, bf16, lists, nQ, nC, D, k, inv_t):
    Q, Cm, off, rows = R.make_case(nQ, nC, D, k)
    Q, Cm = Q.to(DEV), Cm.to(DEV)
    tol = R.tolerance(bf16, inv_t)
    S = R.ref_scores(Q, Cm, inv_t, bf16)
    M = R.mask_scores(S, off, rows) if lists else S
    ceil, ok = R.gap_ceilings(M, tol)
    assert int((~ok).sum()) <= nQ // 100                                   # (test_hard_negatives_host.py: holds for these inputs)
    vals, idx, _ = _run(Q, Cm, k, inv_t, bf16, exclude=_dev(off, rows) if lists else None, ceil=ceil)
    R.check_topk(R.apply_ceiling(M, ceil), vals, idx, k, tol, rows=ok)
    assert bool((vals[ok] < ceil[ok][:, None]).all())
    assert bool((idx[ok][:, 0] >= 0).all())                                # the ceiling sits at ranks 3 .. 12: rows remain below it


# ---- 2. bit for bit the plain entry with the entries >= ceil dropped ---------------------------------------------------------------
@pytest.mark.parametrize("bf16", [True, False])
@pytest.mark.parametrize("k", [10, 65])
def test_ceiling_is_the_plain_search_with_the_top_dropped(tt, bf16, k):
    g = torch.Generator(device=DEV).manual_seed(3)
    nQ, nC, D = 70, 3001, 64
    Q, Cm = _unit(nQ, D, g), _unit(nC, D, g)
    Cm[1500:1600] = Cm[0:100]                                              # duplicated rows: exact ties, also with the ceiling
    Cm[2900:2950] = Cm[0:50]
    Q[:35] = Cm[:35] + 0.3 * Q[:35]                                        # ... and at the top of these queries' lists
    K2 = 2 * k + 16
    big = _run(Q, Cm, K2, 1.0, bf16)
    plain = _run(Q, Cm, k, 1.0, bf16)
    tied = 0
    for j in (0, 3, k - 1):
        ceil = plain[0][:, j].contiguous()
        keep = big[0] < ceil[:, None]
        assert bool((keep.sum(1) >= k).all())
        order = torch.sort((~keep).to(torch.int8), dim=1, stable=True).indices[:, :k]
        want = (torch.gather(big[0], 1, order), torch.gather(big[1], 1, order), None)
        got = _run(Q, Cm, k, 1.0, bf16, ceil=ceil)
        assert _same(got, want), j
        tied += int(((big[0] == ceil[:, None]).sum(1) > 1).sum())
        assert not bool((got[0] >= ceil[:, None]).any())
    assert tied > 0                                                        # ties with the ceiling existed, and all went


# ---- 3. edge ceilings ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bf16", [True, False])
@pytest.mark.parametrize("k", [10, 100])
def test_edge_ceilings(tt, bf16, k):
    g = torch.Generator(device=DEV).manual_seed(8)
    nQ, nC = 70, 5003
    Q, Cm = _unit(nQ, 64, g), _unit(nC, 64, g)
    pos = torch.randint(0, nC, (nQ,), generator=g, device=DEV)
    _, _, off, rows = R.make_case(nQ, nC, 64, k)
    mixed = torch.full((nQ,), INF, device=DEV)
    mixed[::2] = NAN
    for ex in (None, _dev(off, rows)):
        want = _run(Q, Cm, k, 1.0, bf16, positives=pos, exclude=ex)
        for ceil in (torch.full((nQ,), INF, device=DEV), torch.full((nQ,), NAN, device=DEV), mixed):
            assert _same(_run(Q, Cm, k, 1.0, bf16, positives=pos, exclude=ex, ceil=ceil), want)
        none = _run(Q, Cm, k, 1.0, bf16, positives=pos, exclude=ex, ceil=torch.full((nQ,), -INF, device=DEV))
        assert bool((none[1] == -1).all()) and bool((none[0] == -INF).all())
        assert torch.equal(none[2], want[2])
        some = mixed.clone()                                               # per query: -inf for one, untouched neighbours
        some[5] = -INF
        got = _run(Q, Cm, k, 1.0, bf16, exclude=ex, ceil=some)
        assert bool((got[1][5] == -1).all()) and torch.equal(got[1][:5], want[1][:5]) and torch.equal(got[1][6:], want[1][6:])


# ---- 4. the rank never sees the ceiling ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("score_dtype", ["bf16", "fp32"])
def test_rank_is_that_of_the_call_without_a_ceiling(tt, score_dtype):
    from jodalrob_twotower_amd.retrieval import CatalogIndex
    g = torch.Generator(device=DEV).manual_seed(9)
    nQ, nC = 100, 5003
    Q, Cm = _unit(nQ, 64, g), _unit(nC, 64, g)
    index = CatalogIndex.from_embeddings(Cm, temperature=0.5, score_dtype=score_dtype)
    pos = torch.randint(0, nC, (nQ,), generator=g, device=DEV)
    _, _, off, rows = R.make_case(nQ, nC, 64, 10)
    for ex in (None, _dev(off, rows)):
        for k in (10, 100):
            v0, i0, r0 = index.search_with_rank(Q, k, pos, exclude=ex)
            ceil = v0[:, 4].contiguous()                                   # removes five or more rows of every query
            v1, i1, r1 = index.search_with_rank(Q, k, pos, exclude=ex, max_score=ceil)
            assert torch.equal(r1, r0) and torch.equal(r0, index.rank(Q, pos, exclude=ex))
            assert torch.equal(i1[:, :k - 5], i0[:, 5:]) and torch.equal(v1[:, :k - 5].view(torch.int32), v0[:, 5:].view(torch.int32))
            s = index.search(Q, k, exclude=ex, max_score=ceil)
            assert _same(s, (v1, i1))


# ---- 5. split counts ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bf16", [True, False])
@pytest.mark.parametrize("k", [64, 100])
def test_bitwise_identical_across_split_counts(tt, bf16, k):
    from jodalrob_twotower_amd import _lib as L
    g = torch.Generator(device=DEV).manual_seed(5)
    nQ, nC = 100, 20000 - 7
    Q, Cm = _unit(nQ, 64, g), _unit(nC, 64, g)
    Cm[5000:5100] = Cm[100:200]                                            # exact ties across splits
    pos = torch.randint(0, nC, (nQ,), generator=g, device=DEV)
    _, _, off, rows = R.make_case(nQ, nC, 64, k)
    ex = _dev(off, rows)
    ceil = _run(Q, Cm, k, 1.0, bf16, exclude=ex)[0][:, 7].contiguous()
    outs = []
    for s in (0, 0, 1, 2, 7):
        L.set_option(torch.device(DEV), L.TT_OPT_RETRIEVE_SPLITS, s)
        outs.append(_run(Q, Cm, k, 1.0, bf16, positives=pos, exclude=ex, ceil=ceil))
    for o in outs[1:]:
        assert _same(o, outs[0])
    assert not bool((outs[0][0] >= ceil[:, None]).any()) and bool((outs[0][1] >= 0).all())


# ---- 6. pair_scores ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("score_dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("nQ,nC,D", [(70, 3001, 64), (33, 1000, 200), (300, 1000, 6), (7, 4099, 128), (1, 33, 30)])
def test_pair_scores_are_the_sweeps_bits(tt, score_dtype, nQ, nC, D):
    from jodalrob_twotower_amd.retrieval import CatalogIndex
    g = torch.Generator(device=DEV).manual_seed(nQ + D)
    Q, Cm = _unit(nQ, D, g), _unit(nC, D, g)
    index = CatalogIndex.from_embeddings(Cm, temperature=0.5, score_dtype=score_dtype)
    vals, idx = index.search(Q, 10)
    for j in (0, 4, 9):
        got = index.pair_scores(Q, idx[:, j])
        assert got.dtype == torch.float32 and got.shape == (nQ,)
        assert torch.equal(got.view(torch.int32), vals[:, j].contiguous().view(torch.int32)), j
        assert torch.equal(index.pair_scores(Q, idx[:, j].to(torch.int32)).view(torch.int32), got.view(torch.int32))
    rows = torch.randint(0, nC, (nQ,), generator=g, device=DEV)             # any row, not only the best: against f64
    S = R.ref_scores(Q, Cm, 2.0, score_dtype == "bf16")
    err = (index.pair_scores(Q, rows).double() - S.gather(1, rows[:, None])[:, 0]).abs().max()
    assert float(err) <= R.tolerance(score_dtype == "bf16", 2.0)
    bad = rows.clone()
    bad[0] = -1
    bad[nQ - 1] = nC if nQ > 1 else -5
    out = index.pair_scores(Q, bad)
    assert bool(torch.isnan(out[0])) and bool(torch.isnan(out[nQ - 1])) and not bool(torch.isnan(out[1:nQ - 1]).any())


# ---- 7. graph capture ----------------------------------------------------------------------------------------------------------------
def test_search_with_a_ceiling_can_be_captured_in_a_graph(tt):
    from jodalrob_twotower_amd.retrieval import CatalogIndex
    g = torch.Generator(device=DEV).manual_seed(4)
    Q, Cm = _unit(100, 64, g), _unit(5000, 64, g)
    index = CatalogIndex.from_embeddings(Cm, temperature=0.5, score_dtype="bf16")
    _, _, off, rows = R.make_case(100, 5000, 64, 10)
    ex = _dev(off, rows)
    ceil = index.search(Q, 10, exclude=ex)[0][:, 3].contiguous()
    want = index.search(Q, 10, exclude=ex, max_score=ceil)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        index.search(Q, 10, exclude=ex, max_score=ceil)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            got = index.search(Q, 10, exclude=ex, max_score=ceil)
    torch.cuda.current_stream().wait_stream(s)
    graph.replay()
    torch.cuda.synchronize()
    assert _same(got, want) and not bool((got[0] >= ceil[:, None]).any())


# ---- 8. error paths --------------------------------------------------------------------------------------------------------------------
def test_error_paths(tt):
    from jodalrob_twotower_amd import _lib as L
    from jodalrob_twotower_amd.retrieval import CatalogIndex
    g = torch.Generator(device=DEV).manual_seed(1)
    Q, Cm = _unit(8, 32, g), _unit(50, 32, g)
    index = CatalogIndex.from_embeddings(Cm, score_dtype="fp32", tags=torch.ones(50, dtype=torch.int32, device=DEV))
    good = torch.zeros(8, device=DEV)
    pos = torch.zeros(8, dtype=torch.int64, device=DEV)
    for bad in (good.double(), good.long(), torch.zeros(9, device=DEV), torch.zeros((8, 1), device=DEV), good.cpu(), [0.0] * 8):
        with pytest.raises(ValueError):
            index.search(Q, 3, max_score=bad)
        with pytest.raises(ValueError):
            index.search_with_rank(Q, 3, pos, max_score=bad)
    ones = torch.ones(8, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="max_score"):
        index.search(Q, 3, max_score=good, allow=ones)
    with pytest.raises(ValueError, match="max_score"):
        index.search_with_rank(Q, 3, pos, max_score=good, require=ones)
    # the C entries
    lib, dev = L.load(), torch.device(DEV)
    ctx, st, p = L.ctx(dev), L.stream(dev), L.ptr
    ws = torch.empty(lib.tt_retrieve_workspace_bytes(8, 50, 32, 10), dtype=torch.uint8, device=DEV)
    vals = torch.empty((8, 10), device=DEV)
    idx = torch.empty((8, 10), dtype=torch.int64, device=DEV)
    off = torch.zeros(9, dtype=torch.int64, device=DEV)
    rows = torch.zeros(4, dtype=torch.int32, device=DEV)
    ceil = torch.zeros(9, device=DEV)
    qb = torch.empty(lib.tt_score_pack_bytes(8, 32), dtype=torch.uint8, device=DEV)
    cb = torch.empty(lib.tt_score_pack_bytes(50, 32), dtype=torch.uint8, device=DEV)
    out = torch.empty(8, device=DEV)

    def f32(op, rp, cl, wsz=ws.numel()):
        return lib.tt_ceil_retrieve_topk_f32(ctx, p(Q), 8, p(Cm), 50, 32, 1.0, 10, None, 0, p(vals), p(idx), None, op, rp, cl, p(ws), wsz, st)

    def bf16(op, rp, cl, wsz=ws.numel()):
        return lib.tt_ceil_retrieve_topk_bf16(ctx, p(qb), 8, p(cb), 50, 32, 10, None, 0, p(vals), p(idx), None, op, rp, cl, p(ws), wsz, st)

    assert f32(p(off), p(rows), p(ceil)) == 0, lib.tt_last_error_string()
    assert f32(None, None, p(ceil)) == 0, lib.tt_last_error_string()      # the exclusion pair: both NULL is fine
    torch.cuda.synchronize()
    n0 = lib.tt_launch_count()
    mis = L.vp(ceil.data_ptr() + 2)
    bad = []
    for fn in (f32, bf16):
        bad += [fn(p(off), p(rows), None),                                 # NULL ceiling
                fn(None, None, None),
                fn(p(off), p(rows), mis),                                  # not 4-byte aligned
                fn(None, p(rows), p(ceil)),                                # one of the exclusion pair
                fn(p(off), None, p(ceil)),
                fn(p(off), p(rows), p(ceil), 64)]                          # workspace too small
    bad += [lib.tt_pair_scores_f32(ctx, p(Q), 8, p(Cm), 50, 32, 1.0, None, 1, p(out), st),
            lib.tt_pair_scores_f32(ctx, p(Q), 8, p(Cm), 50, 32, 1.0, p(off), 1, None, st),
            lib.tt_pair_scores_f32(ctx, p(Q), 8, p(Cm), 50, 257, 1.0, p(off), 1, p(out), st),
            lib.tt_pair_scores_f32(None, p(Q), 8, p(Cm), 50, 32, 1.0, p(off), 1, p(out), st),
            lib.tt_pair_scores_bf16(ctx, None, 8, p(cb), 50, 32, p(off), 1, p(out), st),
            lib.tt_pair_scores_bf16(ctx, p(qb), 8, p(cb), 50, 32, None, 0, p(out), st)]
    assert all(rc == -1 for rc in bad), bad                                # TT_ERR_INVALID_ARG
    assert lib.tt_launch_count() == n0


# ---- 9. mining end to end -------------------------------------------------------------------------------------------------------------
N_NOTICE, N_COMPANY, N_PAIRS, CHUNK = 300, 400, 1200, 128


def _world(tt, manifest, score_dtype="bf16"):
    """the golden wide_b40 towers (test_gpu_mask_repeats._small_task), stores of a few hundred entities, ~4 companies per notice;
    the last 20 notices have no pairs"""
    from jodalrob_twotower_amd.data_loader import DeviceFeatureStore
    from test_gpu_mask_repeats import _small_task
    task, _, _ = _small_task(tt, manifest, score_dtype=score_dtype)
    cfg = manifest["cases"]["wide_b40"]
    rng = np.random.default_rng(0)
    ns = {"dense_projected": rng.standard_normal((N_NOTICE, cfg["din_n"])).astype(np.float32),
          "categorical": np.stack([rng.integers(0, v, N_NOTICE) for v in cfg["vocab_n"]], 1)}
    cs = {"dense_projected": rng.standard_normal((N_COMPANY, cfg["din_c"])).astype(np.float32),
          "categorical": np.stack([rng.integers(0, v, N_COMPANY) for v in cfg["vocab_c"]], 1)}
    pairs = np.stack([rng.integers(0, N_NOTICE - 20, N_PAIRS), rng.integers(0, N_COMPANY, N_PAIRS)], 1)
    return task, DeviceFeatureStore(ns, cfg["keys_n"], DEV), DeviceFeatureStore(cs, cfg["keys_c"], DEV), pairs


def _sweep_scores(task, nstore, index, pairs):
    """[N_NOTICE, N_COMPANY] f32: every (notice, company) score bit for bit as the sweep forms it (pair_scores, pinned in section 6),
    the notices embedded as the miner embeds them: eval mode, the unique notices of the pairs CHUNK at a time"""
    uniq = torch.as_tensor(np.unique(pairs[:, 0]), device=DEV)
    modes = [(m, m.training) for m in task.modules()]
    task.eval()
    S = torch.full((N_NOTICE, N_COMPANY), NAN, device=DEV)
    with torch.no_grad():
        for s in range(0, uniq.numel(), CHUNK):
            keys = uniq[s:s + CHUNK]
            Q = task.two_tower_model.get_notice_embeddings(nstore.gather(keys.contiguous())).detach().float()
            rows = torch.arange(N_COMPANY, device=DEV).repeat(keys.numel())
            S[keys] = index.pair_scores(Q.repeat_interleave(N_COMPANY, 0), rows).view(keys.numel(), N_COMPANY)
    for m, was in modes:
        m.training = was
    return S


@pytest.mark.parametrize("score_dtype", ["bf16", "fp32"])
def test_mining_end_to_end(tt, manifest, score_dtype):
    from jodalrob_twotower_amd.hard_negatives import MinedNegatives, mine_hard_negatives
    from jodalrob_twotower_amd.retrieval import CatalogIndex
    task, nstore, cstore, pairs = _world(tt, manifest, score_dtype)
    task.train()
    task.two_tower_model.company_tower.eval()                              # a mixed state: restored exactly, not "all train"
    flags = [m.training for m in task.modules()]
    index = CatalogIndex.from_store(task, cstore, chunk=CHUNK)            # (embedded in the chunks the miner's own index uses)
    assert index.score_dtype == ("bf16" if score_dtype == "bf16" else "fp32")
    S = _sweep_scores(task, nstore, index, pairs)
    Sn = S.cpu().numpy()
    known = {n: set(pairs[pairs[:, 0] == n, 1].tolist()) for n in range(N_NOTICE)}
    k, per = 16, 4
    for ceiling in ((0.95, 0.0), (1.0, -0.5), None):
        want, cand, ceils = R.mine_reference(Sn, pairs, N_NOTICE, k, per, ceiling)
        mined = mine_hard_negatives(task, nstore, cstore, pairs, k=k, per_notice=per, ceiling=ceiling, chunk=CHUNK, index=index)
        assert isinstance(mined, MinedNegatives) and (mined.k, mined.per_notice, mined.ceiling, mined.select) == (k, per, ceiling, "top")
        table = mined.table.cpu().numpy()
        assert mined.table.dtype == torch.int32 and table.shape == (N_NOTICE, per)
        assert np.array_equal(table, want)                                 # the reference's ranking, -1 exactly where it has none
        assert (table[N_NOTICE - 20:] == -1).all()
        for n in range(N_NOTICE):
            got = table[n][table[n] >= 0]
            assert not set(got.tolist()) & known[n]
            if ceiling is not None and len(got):
                assert (Sn[n, got] < ceils[n]).all()
        # uniform: a subset of the k valid rows, reproducible per seed
        u1 = mine_hard_negatives(task, nstore, cstore, pairs, k=k, per_notice=per, ceiling=ceiling, select="uniform", chunk=CHUNK, seed=5,
                                 index=index).table.cpu().numpy()
        u2 = mine_hard_negatives(task, nstore, cstore, pairs, k=k, per_notice=per, ceiling=ceiling, select="uniform", chunk=CHUNK, seed=5,
                                 index=index).table.cpu().numpy()
        u3 = mine_hard_negatives(task, nstore, cstore, pairs, k=k, per_notice=per, ceiling=ceiling, select="uniform", chunk=CHUNK, seed=6,
                                 index=index).table.cpu().numpy()
        assert np.array_equal(u1, u2) and not np.array_equal(u1, u3)
        for n in range(N_NOTICE):
            got = u1[n][u1[n] >= 0]
            have = cand.get(n, np.zeros(0, np.int64))
            assert len(got) == min(per, len(have)) == len(set(got.tolist())) and set(got.tolist()) <= set(have.tolist())
        assert not np.array_equal(u1, table)
    assert [m.training for m in task.modules()] == flags
    # the index built inside, and one chunk for everything: the same table
    again = mine_hard_negatives(task, nstore, cstore, pairs, k=k, per_notice=per, ceiling=(0.95, 0.0), chunk=CHUNK)
    assert [m.training for m in task.modules()] == flags
    assert np.array_equal(again.table.cpu().numpy(), R.mine_reference(Sn, pairs, N_NOTICE, k, per, (0.95, 0.0))[0])


# ---- 10. the loader ----------------------------------------------------------------------------------------------------------------
def _entity_batches(it):
    return [{s: {f: (v.values() if f == "kjt" else v).clone() for f, v in b[s].items()} for s in ("notice", "company", "negatives") if s in b}
            for b in it]


@pytest.mark.parametrize("frac", [1.0, 0.4])
def test_loader_draws_a_batchs_extras_from_its_own_mined_rows(tt, manifest, frac):
    from jodalrob_twotower_amd.data_loader import DevicePairLoader
    from jodalrob_twotower_amd.sampling_bias import log_sampling_probs
    _, nstore, cstore, pairs = _world(tt, manifest)
    rng = np.random.default_rng(3)
    table = rng.integers(0, N_COMPANY, (N_NOTICE, 4)).astype(np.int32)
    table[rng.random(N_NOTICE) < 0.9] = -1                                 # few notices have mined rows: some batches have none
    table[:, 3] = -1
    B, M = 16, 10
    H = int(round(frac * M))
    pt = torch.as_tensor(pairs, device=DEV)
    lq = (log_sampling_probs(pt[:, 0], N_NOTICE), log_sampling_probs(pt[:, 1], N_COMPANY))

    def loader(M, **kw):
        return DevicePairLoader(nstore, cstore, pairs, B, shuffle=True, seed=7, log_q=lq, mask_repeats=True, extra_negatives=M, **kw)
    mk = dict(mined=torch.as_tensor(table, device=DEV), hard_fraction=frac)
    plain, uni, got = _entity_batches(loader(0)), _entity_batches(loader(M)), _entity_batches(loader(M, **mk))
    assert len(got) == len(plain) == N_PAIRS // B
    uni_lq = torch.full((M,), -float(np.log(N_COMPANY)), dtype=torch.float32, device=DEV)
    fell_back = drew = 0
    for p, u, b in zip(plain, uni, got):
        for side in ("notice", "company"):                                 # the pair order of a loader without extras
            assert torch.equal(p[side]["entity"], b[side]["entity"]) and torch.equal(p[side]["dense"], b[side]["dense"])
        neg = b["negatives"]
        ent = neg["entity"].cpu().numpy()
        assert ent.shape == (M,) and ((ent >= 0) & (ent < N_COMPANY)).all()
        assert torch.equal(neg["dense"], cstore.dense[neg["entity"].long()])
        assert torch.equal(neg["entity"][H:], u["negatives"]["entity"][H:])           # the uniform slots: the uniform loader's bits
        cands = R.batch_candidates(table, b["notice"]["entity"].cpu().numpy())
        want_lq = uni_lq.clone()
        if len(cands):
            drew += 1
            assert set(ent[:H].tolist()) <= set(cands.tolist())
            want_lq[:H] = -float(np.log(len(cands)))
        else:
            fell_back += 1
            assert torch.equal(neg["entity"], u["negatives"]["entity"])
        assert torch.allclose(neg["log_q"], want_lq, rtol=1e-6, atol=0) and neg["log_q"].dtype == torch.float32
        assert float(neg["log_q"].max()) < 0.0                             # never 0: that would drop the row from the softmax
    assert fell_back > 0 and drew > fell_back
    assert any(not torch.equal(a["negatives"]["entity"], b["negatives"]["entity"]) for a, b in zip(uni, got))
    # the same seed: the same draw; __iter__ and step_batches see the same batches
    again = _entity_batches(loader(M, **mk))
    sb = _entity_batches(loader(M, **mk).step_batches(None, eager_step=lambda b: b))
    for a, b, c in zip(got, again, sb):
        for side in ("notice", "company", "negatives"):
            for f in ("dense", "entity", "log_q", "kjt"):
                assert torch.equal(a[side][f], b[side][f]) and torch.equal(a[side][f], c[side][f]), (side, f)
    ld = loader(M, **mk)
    order = ld.epoch_order()
    with pytest.raises(ValueError, match="order"):
        ld.epoch_negatives()
    assert ld.epoch_negatives(order).shape == (len(ld), M)
    ordered = DevicePairLoader(nstore, cstore, pairs, B, shuffle=False, extra_negatives=M, **mk)
    assert ordered.epoch_negatives().shape == (len(ordered), M)           # not shuffling: the pair list's own order


# ---- 11. the captured step on mined batches ---------------------------------------------------------------------------------------------
def test_captured_step_on_mined_batches_equals_eager(tt, manifest):
    from jodalrob_twotower_amd.data_loader import DevicePairLoader
    from jodalrob_twotower_amd.graph import GraphedTrainStep
    from jodalrob_twotower_amd.hard_negatives import mine_hard_negatives
    from jodalrob_twotower_amd.optim import FusedAdam
    from jodalrob_twotower_amd.sampling_bias import log_sampling_probs
    B, M, finals, tables = 64, 24, {}, []
    for mode in ("eager", "graph"):
        task, nstore, cstore, pairs = _world(tt, manifest)
        pairs = pairs[:3 * B]
        mined = mine_hard_negatives(task, nstore, cstore, pairs, k=16, per_notice=4)
        tables.append(mined.table.cpu())
        pt = torch.as_tensor(pairs, device=DEV)
        lq = (log_sampling_probs(pt[:, 0], N_NOTICE), log_sampling_probs(pt[:, 1], N_COMPANY))
        loader = DevicePairLoader(nstore, cstore, pairs, B, shuffle=True, seed=3, log_q=lq, mask_repeats=True, extra_negatives=M,
                                  mined=mined, hard_fraction=0.75)
        bs = list(loader)[:2]
        assert bool((bs[0]["negatives"]["log_q"][:18] > bs[0]["negatives"]["log_q"][18:].max()).all())      # mined slots, their own log q
        task.train()
        opt = FusedAdam.for_task(task, lr=1e-2, weight_decay=1e-5)
        gs = GraphedTrainStep(task, opt, bs[0], warmup=1) if mode == "graph" else None
        losses = []
        for bk in bs:
            if gs is None:
                opt.zero_grad()
                r = task(bk, return_metrics=True)
                r["loss"].backward()
                opt.step()
            else:
                r = gs.step(bk)
            losses.append(r["loss"].item())
        torch.cuda.synchronize()
        finals[mode] = (losses, {k: v.detach().cpu().clone() for k, v in task.state_dict().items()})
        if gs is not None:
            gs.close()
    assert torch.equal(tables[0], tables[1]) and int((tables[0] >= 0).sum()) > 0
    assert finals["graph"][0] == finals["eager"][0] and len(set(finals["eager"][0])) == 2
    for k, v in finals["eager"][1].items():
        assert torch.equal(v, finals["graph"][1][k]), k
