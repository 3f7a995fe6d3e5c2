"""GPU tests of per-query exclusion lists in catalogue-wide retrieval (tt_excl_retrieve_topk_bf16 / _f32): top-k and rank
against a masked f64 reference of the same rounded operands, bitwise equality with the plain entry for empty lists, bitwise
determinism across split counts, exact identities against the plain entry (excluding the top-k gives the next k; the rank drops
by the excluded rows that outrank p), short eligible sets, graph capture, the error paths, and the filtered evaluation end to
end on a trained task."""
import numpy as np
import pytest
import torch

from conftest import GOLD

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


def _unit(n, d, g):
    x = torch.randn((n, d), generator=g, device=DEV, dtype=torch.float32)
    return x / x.norm(dim=1, keepdim=True)


def _ref_scores(Q, Cm, inv_t, bf16):
    if bf16:
        return Q.float().to(torch.bfloat16).double() @ (Cm * inv_t).to(torch.bfloat16).double().T
    return (Q.double() @ Cm.double().T) * inv_t


def _run(Q, Cm, k, inv_t, bf16, positives=None, exclude=None):
    """(vals, idx, rank) from one ops-level call; exclude = (offsets, rows) device tensors, or None for the plain entry."""
    from jodalrob_twotower_amd import ops
    nQ, D = Q.shape
    nC = Cm.shape[0]
    if bf16:
        q, c = ops.score_pack_bf16(Q, 1.0), ops.score_pack_bf16(Cm, inv_t)
        out = ops._retrieve(q, nQ, c, nC, D, k, 1.0, True, positives, None, exclude)
    else:
        out = ops._retrieve(Q, nQ, Cm, nC, D, k, inv_t, False, positives, None, exclude)
    torch.cuda.synchronize()
    return out


def _random_lists(nQ, nC, max_len, rng, lo=-2, hi_extra=2):
    """Ascending lists of 0 .. max_len rows per query, duplicates and out-of-range rows included."""
    lens = rng.integers(0, max_len + 1, nQ)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    rows = np.concatenate([np.sort(rng.integers(lo, nC + hi_extra, n)) for n in lens] + [np.zeros(0, np.int64)])
    return off, rows.astype(np.int32)


def _dev(off, rows):
    return torch.as_tensor(off, device=DEV), torch.as_tensor(rows, device=DEV)


def _mask(S, off, rows):
    """-inf at every (q, excluded row in range) of the f64 reference."""
    M = S.clone()
    off, rows = np.asarray(off), np.asarray(rows)
    q = np.repeat(np.arange(S.shape[0]), np.diff(off))
    ok = (rows >= 0) & (rows < S.shape[1])
    M[torch.as_tensor(q[ok], device=DEV), torch.as_tensor(rows[ok].astype(np.int64), device=DEV)] = -float("inf")
    return M


def _check_topk_masked(M, vals, idx, k, tol):
    """M: masked f64 reference.  The first n_eligible slots as _check_topk of test_gpu_retrieval checks them, the rest -inf / -1."""
    nQ = M.shape[0]
    elig = torch.isfinite(M).sum(1).clamp(max=k)
    slot = torch.arange(k, device=DEV)[None, :]
    real = slot < elig[:, None]
    assert vals.shape == idx.shape == (nQ, k)
    assert bool((idx[~real] == -1).all()) and bool((vals[~real] == -float("inf")).all())
    assert bool((idx[real] >= 0).all()) and bool((idx[real] < M.shape[1]).all())
    got = torch.gather(M, 1, idx.clamp(min=0))
    assert bool(torch.isfinite(got[real]).all())                      # never an excluded row
    err = (got[real] - vals[real].double()).abs()
    assert err.numel() == 0 or float(err.max()) <= tol
    kth = torch.gather(torch.topk(M, k, dim=1).values, 1, (elig - 1).clamp(min=0)[:, None])
    assert bool((got[real] >= (kth.expand(-1, k)[real] - tol)).all())
    srt = torch.sort(torch.where(real, idx, -1 - slot), dim=1).values
    assert bool((srt[:, 1:] != srt[:, :-1]).all())
    dv = vals[:, 1:] - vals[:, :-1]
    both = real[:, 1:]
    assert bool((dv[both] <= 0).all())
    assert bool(((dv < 0) | (idx[:, 1:] > idx[:, :-1]))[both].all())


def _check_rank_masked(S, M, pos, r, tol):
    """Rank between the bounds of the masked reference with tol, and equal to the rule where there is no near-tie."""
    sp = torch.gather(S, 1, pos[:, None])
    Mp = M.clone()
    Mp.scatter_(1, pos[:, None], -float("inf"))                       # p never counts against itself
    lo = (Mp > sp + tol).sum(1)
    hi = (Mp >= sp - tol).sum(1)
    r = r.long()
    assert bool(((r >= lo) & (r <= hi)).all())
    exact = lo == hi
    cols = torch.arange(S.shape[1], device=DEV)[None, :]
    want = (Mp > sp).sum(1) + ((Mp == sp) & (cols < pos[:, None])).sum(1)
    assert torch.equal(r[exact], want[exact])
    return exact


CASES = [  # nQ, nC, D, k, inv_t
    (1, 33, 6, 1, 1.0),
    (33, 33, 64, 10, 0.05),
    (300, 33, 200, 10, 1.0),
    (33, 1000, 200, 64, 1.0),
    (300, 1000, 6, 10, 0.05),
    (1, 1000, 64, 64, 1.0),
    (33, 65537, 64, 10, 0.05),
    (300, 65537, 200, 1, 1.0),
    (1, 65537, 6, 64, 1.0),
]


@pytest.mark.parametrize("bf16", [True, False])
@pytest.mark.parametrize("nQ,nC,D,k,inv_t", CASES)
def test_topk_and_rank_vs_masked_reference(tt, bf16, nQ, nC, D, k, inv_t):
    g = torch.Generator(device=DEV).manual_seed(nQ * 5 + nC + D + k)
    rng = np.random.default_rng(nQ + nC + D + k)
    Q, Cm = _unit(nQ, D, g), _unit(nC, D, g)
    off, rows = _random_lists(nQ, nC, 300, rng)
    pos = torch.as_tensor(rng.integers(0, nC, nQ), device=DEV)
    vals, idx, rank = _run(Q, Cm, k, inv_t, bf16, positives=pos, exclude=_dev(off, rows))
    S = _ref_scores(Q, Cm, inv_t, bf16)
    M = _mask(S, off, rows)
    tol = (1e-5 if bf16 else 2e-6) * max(1.0, inv_t) + 1e-6
    _check_topk_masked(M, vals, idx, k, tol)
    exact = _check_rank_masked(S, M, pos, rank, tol)
    if nC <= 1000:
        assert float(exact.float().mean()) > 0.5
    r_only = _run(Q, Cm, 0, inv_t, bf16, positives=pos.to(torch.int32), exclude=_dev(off, rows))[2]
    assert torch.equal(r_only, rank)                                   # k = 0 and k > 0, int32 and int64 positives


@pytest.mark.parametrize("bf16", [True, False])
def test_empty_and_out_of_range_lists_are_bitwise_the_plain_entry(tt, bf16):
    g = torch.Generator(device=DEV).manual_seed(7)
    nQ, nC = 300, 20011
    Q, Cm = _unit(nQ, 64, g), _unit(nC, 64, g)
    pos = torch.randint(0, nC, (nQ,), generator=g, device=DEV)
    pos[:3] = torch.tensor([-1, nC, nC + 5], device=DEV)
    plain = _run(Q, Cm, 64, 1.0, bf16, positives=pos)
    empty = (torch.zeros(nQ + 1, dtype=torch.int64, device=DEV), torch.zeros(0, dtype=torch.int32, device=DEV))
    rng = np.random.default_rng(1)
    lens = rng.integers(0, 40, nQ)
    lens[::3] = 0
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    rows = np.concatenate([np.sort(np.where(rng.random(n) < 0.5, rng.integers(-1000, 0, n), rng.integers(nC, nC + 1000, n)))
                           for n in lens]).astype(np.int32)
    for ex in (empty, _dev(off, rows)):
        got = _run(Q, Cm, 64, 1.0, bf16, positives=pos, exclude=ex)
        assert torch.equal(got[0].view(torch.int32), plain[0].view(torch.int32))
        assert torch.equal(got[1], plain[1]) and torch.equal(got[2], plain[2])
    r_plain = _run(Q, Cm, 0, 1.0, bf16, positives=pos)[2]
    assert torch.equal(_run(Q, Cm, 0, 1.0, bf16, positives=pos, exclude=empty)[2], r_plain)


@pytest.mark.parametrize("bf16", [True, False])
def test_bitwise_identical_across_split_counts(tt, bf16):
    from jodalrob_twotower_amd import _lib as L
    g = torch.Generator(device=DEV).manual_seed(5)
    nQ, nC = 300, 20000 - 7                                            # ragged last tile
    Q, Cm = _unit(nQ, 64, g), _unit(nC, 64, g)
    Cm[5000:5100] = Cm[100:200]                                        # exact ties across splits
    pos = torch.randint(0, nC, (nQ,), generator=g, device=DEV)
    rng = np.random.default_rng(2)
    nT = (nC + 31) // 32
    bounds = sorted({32 * (nT * s // S) for S in (2, 7, 32) for s in range(1, S)})
    lists = []
    for q in range(nQ):
        r = list(rng.integers(0, nC, rng.integers(0, 120)))
        for b in rng.choice(bounds, 3):                                # runs straddling split (and tile) boundaries
            r += list(range(b - rng.integers(1, 40), b + rng.integers(1, 40)))
        r += list(range(nC - 20, nC + 3))                              # the ragged last tile, past its end too
        r += list(range(100, 100 + (q % 50)))                          # tied rows
        lists.append(np.sort(np.array(r)))
    off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    ex = _dev(off, np.concatenate(lists).astype(np.int32))
    outs = []
    for s in (0, 0, 1, 2, 7, 32):
        L.set_option(torch.device(DEV), L.TT_OPT_RETRIEVE_SPLITS, s)
        outs.append(_run(Q, Cm, 64, 1.0, bf16, positives=pos, exclude=ex))
    for o in outs[1:]:
        assert torch.equal(o[0].view(torch.int32), outs[0][0].view(torch.int32))
        assert torch.equal(o[1], outs[0][1]) and torch.equal(o[2], outs[0][2])
    _check_topk_masked(_mask(_ref_scores(Q, Cm, 1.0, bf16), off, np.concatenate(lists)), outs[0][0], outs[0][1], 64,
                       2e-5 if bf16 else 3e-6)


@pytest.mark.parametrize("bf16", [True, False])
@pytest.mark.parametrize("k", [10, 32])
def test_excluding_the_top_k_gives_the_next_k(tt, bf16, k):
    g = torch.Generator(device=DEV).manual_seed(k)
    Q, Cm = _unit(100, 64, g), _unit(30000, 64, g)
    Cm[20000:20200] = Cm[:200]                                         # exact ties
    v2, i2, _ = _run(Q, Cm, 2 * k, 1.0, bf16)
    top = torch.sort(i2[:, :k], dim=1).values
    off = torch.arange(101, dtype=torch.int64, device=DEV) * k
    v, i, _ = _run(Q, Cm, k, 1.0, bf16, exclude=(off, top.reshape(-1).to(torch.int32).contiguous()))
    assert torch.equal(v.view(torch.int32), v2[:, k:].contiguous().view(torch.int32)) and torch.equal(i, i2[:, k:])


@pytest.mark.parametrize("bf16", [True, False])
def test_fewer_eligible_rows_than_k(tt, bf16):
    g = torch.Generator(device=DEV).manual_seed(8)
    nQ, nC, k = 40, 300, 10
    Q, Cm = _unit(nQ, 32, g), _unit(nC, 32, g)
    rng = np.random.default_rng(3)
    keep = [np.sort(rng.choice(nC, q % k, replace=False)) for q in range(nQ)]        # j = 0 .. 9 rows left
    lists = [np.setdiff1d(np.arange(nC), kp) for kp in keep]
    off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    vals, idx, rank = _run(Q, Cm, k, 1.0, bf16, positives=torch.zeros(nQ, dtype=torch.int64, device=DEV),
                           exclude=_dev(off, np.concatenate(lists).astype(np.int32)))
    S = _ref_scores(Q, Cm, 1.0, bf16)
    for q in range(nQ):
        j = len(keep[q])
        got = idx[q].cpu().numpy()
        assert sorted(got[:j].tolist()) == keep[q].tolist(), q
        assert (got[j:] == -1).all() and bool((vals[q, j:] == -float("inf")).all())
        assert bool((vals[q, 1:j] <= vals[q, :j - 1]).all()) if j > 1 else True
        # rank of row 0 counts only the kept rows that outrank it
        sp = S[q, 0]
        kp = torch.as_tensor(keep[q][keep[q] != 0], device=DEV, dtype=torch.int64)
        assert int(rank[q]) == int((S[q, kp] > sp).sum()), q
    _check_topk_masked(_mask(S, off, np.concatenate(lists)), vals, idx, k, 2e-5)


@pytest.mark.parametrize("bf16", [True, False])
def test_rank_drops_by_the_excluded_rows_that_outrank_p(tt, bf16):
    g = torch.Generator(device=DEV).manual_seed(12)
    nQ, nC, L = 64, 5000, 40
    Q, Cm = _unit(nQ, 64, g), _unit(nC, 64, g)
    Cm[4000:4100] = Cm[:100]                                           # exact ties
    rng = np.random.default_rng(4)
    pos = rng.integers(0, nC, nQ)
    lists = []
    for q in range(nQ):
        r = set(rng.choice(nC, L, replace=False).tolist()) | {int(pos[q]) % 100, int(pos[q]) % 100 + 4000}
        lists.append(np.array(sorted(r)))
    with_p = [np.union1d(x, [pos[q]]) for q, x in enumerate(lists)]
    without_p = [np.setdiff1d(x, [pos[q]]) for q, x in enumerate(lists)]
    pos_t = torch.as_tensor(pos, device=DEV)

    def csr(ls):
        off = np.concatenate([[0], np.cumsum([len(x) for x in ls])]).astype(np.int64)
        return _dev(off, np.concatenate(ls).astype(np.int32))

    r_with = _run(Q, Cm, 0, 1.0, bf16, positives=pos_t, exclude=csr(with_p))[2]
    r_without = _run(Q, Cm, 0, 1.0, bf16, positives=pos_t, exclude=csr(without_p))[2]
    assert torch.equal(r_with, r_without)
    # plain ranks are positions in the total order: c outranks p  <=>  plain rank of c < plain rank of p
    r_plain = _run(Q, Cm, 0, 1.0, bf16, positives=pos_t)[2].long()
    qs = np.concatenate([np.full(len(x), q) for q, x in enumerate(without_p)])
    cs = np.concatenate(without_p)
    r_c = _run(Q[torch.as_tensor(qs, device=DEV)].contiguous(), Cm, 0, 1.0, bf16, positives=torch.as_tensor(cs, device=DEV))[2]
    outr = torch.zeros(nQ, dtype=torch.int64, device=DEV)
    outr.index_add_(0, torch.as_tensor(qs, device=DEV), (r_c.long() < r_plain[torch.as_tensor(qs, device=DEV)]).long())
    assert torch.equal(r_with.long(), r_plain - outr)
    assert int(outr.sum()) > 0


def test_search_with_exclusion_can_be_captured_in_a_graph(tt):
    from jodalrob_twotower_amd.retrieval import CatalogIndex
    g = torch.Generator(device=DEV).manual_seed(4)
    Q, Cm = _unit(100, 64, g), _unit(5000, 64, g)
    index = CatalogIndex.from_embeddings(Cm, temperature=0.5, score_dtype="bf16")
    rng = np.random.default_rng(5)
    off, rows = _random_lists(100, 5000, 200, rng)
    for q in range(100):                                               # unsorted caller lists: the index sorts each one
        rows[off[q]:off[q + 1]] = rng.permutation(rows[off[q]:off[q + 1]])
    ex = _dev(off, rows)
    want = index.search(Q, 10, exclude=ex)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        index.search(Q, 10, exclude=ex)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            got = index.search(Q, 10, exclude=ex)
    torch.cuda.current_stream().wait_stream(s)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(got[0].view(torch.int32), want[0].view(torch.int32)) and torch.equal(got[1], want[1])
    # the unsorted lists mean the same as the sorted ones
    srt = np.concatenate([np.sort(rows[off[q]:off[q + 1]]) for q in range(100)]).astype(np.int32)
    ref = index.search(Q, 10, exclude=_dev(off, srt))
    assert torch.equal(ref[1], want[1])


def test_error_paths_return_nonzero_and_launch_nothing(tt):
    from jodalrob_twotower_amd import _lib as L
    lib, dev = L.load(), torch.device(DEV)
    ctx, st = L.ctx(dev), L.stream(dev)
    g = torch.Generator(device=DEV).manual_seed(1)
    Q, Cm = _unit(8, 32, g), _unit(50, 32, g)
    ws = torch.empty(lib.tt_retrieve_workspace_bytes(8, 50, 32, 10), dtype=torch.uint8, device=DEV)
    vals = torch.empty((8, 10), device=DEV)
    idx = torch.empty((8, 10), dtype=torch.int64, device=DEV)
    off = torch.zeros(9 + 1, dtype=torch.int64, device=DEV)            # one spare element for the misaligned view
    rows = torch.zeros(4, dtype=torch.int32, device=DEV)
    p = L.ptr
    qp, cp = p(Q), p(Cm)
    packed_q = L.load().tt_score_pack_bytes(8, 32)
    qb = torch.empty(packed_q, dtype=torch.uint8, device=DEV)
    cb = torch.empty(L.load().tt_score_pack_bytes(50, 32), dtype=torch.uint8, device=DEV)

    def f32(op, rp, wsz):
        return lib.tt_excl_retrieve_topk_f32(ctx, qp, 8, cp, 50, 32, 1.0, 10, None, 0, p(vals), p(idx), None, op, rp, p(ws), wsz, st)

    def bf16(op, rp, wsz):
        return lib.tt_excl_retrieve_topk_bf16(ctx, p(qb), 8, p(cb), 50, 32, 10, None, 0, p(vals), p(idx), None, op, rp, p(ws), wsz,
                                              st)

    ok = f32(p(off), p(rows), ws.numel())
    assert ok == 0, lib.tt_last_error_string()
    torch.cuda.synchronize()
    n0 = lib.tt_launch_count()
    mis_off = L.vp(off.data_ptr() + 4)
    mis_rows = L.vp(rows.data_ptr() + 2)
    bad = []
    for fn in (f32, bf16):
        bad += [fn(None, p(rows), ws.numel()),                         # NULL offsets
                fn(p(off), None, ws.numel()),                          # NULL rows
                fn(mis_off, p(rows), ws.numel()),                      # offsets not 8-byte aligned
                fn(p(off), mis_rows, ws.numel()),                      # rows not 4-byte aligned
                fn(p(off), p(rows), 64)]                               # workspace too small
    assert all(rc == -1 for rc in bad), bad                            # TT_ERR_INVALID_ARG
    assert lib.tt_launch_count() == n0


# ---- end to end on a trained task ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trained(tt, manifest):
    from jodalrob_twotower_amd.data_loader import DeviceFeatureStore, DevicePairLoader
    cfg = manifest["cases"]["tiny_train"]
    torch.manual_seed(0)
    task = tt.create_two_tower_train_task(cfg["keys_n"], cfg["keys_c"], metadata_path=str(GOLD / "synthetic_metadata.csv"),
                                          categorical_embedding_dim=cfg["E"], notice_dense_input_dim=cfg["din_n"],
                                          company_dense_input_dim=cfg["din_c"], tower_hidden_dims=[32, 32],
                                          final_embedding_dim=32, dropout_rate=0.1, temperature=0.5, device=DEV, score_dtype="fp32")
    rng = np.random.default_rng(0)
    nN, nC = 300, 1500
    ns = {"dense_projected": rng.standard_normal((nN, cfg["din_n"])).astype(np.float32),
          "categorical": np.stack([rng.integers(0, v, nN) for v in cfg["vocab_n"]], 1)}
    cs = {"dense_projected": rng.standard_normal((nC, cfg["din_c"])).astype(np.float32),
          "categorical": np.stack([rng.integers(0, v, nC) for v in cfg["vocab_c"]], 1)}
    pairs = np.stack([rng.integers(0, nN, 3000), rng.integers(0, nC, 3000)], 1)        # ~10 companies per notice
    nstore, cstore = DeviceFeatureStore(ns, cfg["keys_n"], DEV), DeviceFeatureStore(cs, cfg["keys_c"], DEV)
    loader = DevicePairLoader(nstore, cstore, pairs, 256, shuffle=False)
    opt = torch.optim.SGD(task.parameters(), lr=0.05)
    task.train()
    for i, b in enumerate(loader):
        if i == 4:
            break
        opt.zero_grad()
        task(b).backward()
        opt.step()
    torch.cuda.synchronize()
    return task, nstore, cstore, loader, pairs


def _state(task):
    return {k: v.detach().clone() for k, v in task.state_dict().items()}


def _same_state(a, b):
    return a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)


def test_filtered_evaluate_catalog_and_predict_catalog(tt, trained):
    from jodalrob_twotower_amd.retrieval import CatalogIndex, exclusions_from_pairs
    task, nstore, cstore, loader, pairs = trained
    ev = tt.TwoTowerEvaluator(device=DEV)
    index = CatalogIndex.from_store(task, cstore)
    task.train()
    before = _state(task)
    sub = pairs[:1000]
    raw = ev.evaluate_catalog(task, nstore, index, sub, batch_size=300)
    assert ev.evaluate_catalog(task, nstore, index, sub, batch_size=300, filter_pairs=None) == raw
    filt = ev.evaluate_catalog(task, nstore, index, sub, batch_size=300, filter_pairs=pairs)
    assert filt.keys() == raw.keys() and filt["num_queries"] == 1000 and filt["catalog_size"] == 1500
    for key in ("recall@5", "recall@10", "mrr"):
        assert filt[key] >= raw[key], key
    assert filt["mrr"] > raw["mrr"]
    # the f64 dense masked reference
    task.eval()
    with torch.no_grad():
        q = task.two_tower_model.get_notice_embeddings(nstore.gather(torch.as_tensor(sub[:, 0], device=DEV)))
    task.train()
    S = (q.double() @ index.data.double().T) * index.inv_t
    off, rows = exclusions_from_pairs(torch.as_tensor(sub[:, 0], device=DEV), torch.as_tensor(pairs, device=DEV), 1500)
    M = _mask(S, off.cpu().numpy(), rows.cpu().numpy())
    pos = torch.as_tensor(sub[:, 1], device=DEV)
    r = index.rank(q, pos, exclude=(off, rows))
    exact = _check_rank_masked(S, M, pos, r, 1e-5)
    assert float(exact.float().mean()) > 0.95
    for k in (5, 10):
        assert filt[f"recall@{k}"] == pytest.approx(float((r < k).float().mean()), abs=1e-6)
    assert filt["mrr"] == pytest.approx(float((1.0 / (r.double() + 1.0)).mean()), rel=1e-5)
    # predict_catalog never returns an excluded row
    batch = loader.batch(None, 0)
    keys = torch.as_tensor(pairs[:batch["notice"]["dense"].shape[0], 0], device=DEV)     # (shuffle=False: batch 0 = pairs[:B])
    ex = exclusions_from_pairs(keys, torch.as_tensor(pairs, device=DEV), 1500)
    pred = task.predict_catalog(batch["notice"], index, top_k=64, exclude=ex)
    o, rw = ex[0].cpu().numpy(), ex[1].cpu().numpy()
    got = pred["top_indices"].cpu().numpy()
    assert sum(o[i + 1] - o[i] for i in range(len(o) - 1)) > 0
    for i in range(got.shape[0]):
        assert not set(got[i].tolist()) & set(rw[o[i]:o[i + 1]].tolist()), i
    assert task.training and _same_state(before, _state(task))
