"""GPU tests of catalogue-wide retrieval: tt_retrieve_topk_bf16 / tt_retrieve_topk_f32 against an f64 reference, the top-k
order and tie rule, bitwise determinism across runs and split counts, the rank rule (also against the in-batch
tt_diag_rank_rows), the error paths, and CatalogIndex / predict_catalog / evaluate_catalog end to end on a trained task."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import GOLD
from test_retrieval_host import ref_rank

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


def _bf16_round(x: torch.Tensor) -> torch.Tensor:
    """f32 -> nearest-even bf16, back as f32 (what tt_score_pack_bf16 stores)."""
    return x.float().to(torch.bfloat16).float()


def _unit(n, d, g):
    x = torch.randn((n, d), generator=g, device=DEV, dtype=torch.float32)
    return x / x.norm(dim=1, keepdim=True)


def _run(tt, Q, Cm, k, inv_t, bf16, positives=None):
    from jodalrob_twotower_amd import ops
    nQ, D = Q.shape
    nC = Cm.shape[0]
    if bf16:
        q, c = ops.score_pack_bf16(Q, 1.0), ops.score_pack_bf16(Cm, inv_t)
        out = ops.retrieve_topk(q, nQ, c, nC, D, k, bf16=True, positives=positives) if k else \
            ops.retrieve_rank(q, nQ, c, nC, D, positives, bf16=True)
    else:
        out = ops.retrieve_topk(Q, nQ, Cm, nC, D, k, inv_t=inv_t, positives=positives) if k else \
            ops.retrieve_rank(Q, nQ, Cm, nC, D, positives, inv_t=inv_t)
    torch.cuda.synchronize()
    return out


def _ref_scores(Q, Cm, inv_t, bf16):
    if bf16:
        return _bf16_round(Q).double() @ _bf16_round(Cm * inv_t).double().T
    return (Q.double() @ Cm.double().T) * inv_t


def _check_topk(S, vals, idx, k, tol):
    """S: f64 reference [nQ, nC] (device).  Values near the reference score of the index returned, every returned score at least
    the reference k-th minus tol, indices distinct and in range, order non-increasing with ties in ascending index."""
    nC = S.shape[1]
    assert vals.shape == idx.shape == (S.shape[0], k)
    assert int(idx.min()) >= 0 and int(idx.max()) < nC
    got = torch.gather(S, 1, idx)
    assert float((got - vals.double()).abs().max()) <= tol
    kth = torch.topk(S, k, dim=1).values[:, -1:]
    assert bool((got >= kth - tol).all())
    srt = torch.sort(idx, dim=1).values
    assert bool((srt[:, 1:] != srt[:, :-1]).all())
    dv = vals[:, 1:] - vals[:, :-1]
    assert bool((dv <= 0).all())
    assert bool(((dv < 0) | (idx[:, 1:] > idx[:, :-1])).all())


CASES = [  # nQ, nC, D, k, inv_t
    (1, 10, 32, 10, 1.0),          # nC == k
    (1, 64, 256, 64, 1.0),         # nC == k == 64
    (7, 31, 6, 10, 1.0),
    (7, 33, 100, 10, 0.05),
    (300, 33, 32, 1, 1.0),
    (300, 1000, 64, 64, 0.05),
    (300, 1000, 6, 10, 1.0),
    (7, 65537, 100, 1, 0.05),
    (300, 65537, 256, 64, 1.0),
    (300, 65537, 64, 10, 0.05),
    (8192, 1000, 64, 10, 1.0),
    (8192, 1000, 256, 64, 0.05),
]


@pytest.mark.parametrize("nQ,nC,D,k,inv_t", CASES)
def test_bf16_topk_vs_rounded_reference(tt, nQ, nC, D, k, inv_t):
    g = torch.Generator(device=DEV).manual_seed(nQ * 7 + nC + D + k)
    Q, Cm = _unit(nQ, D, g), _unit(nC, D, g)
    vals, idx = _run(tt, Q, Cm, k, inv_t, True)
    tol = 1e-5 * max(1.0, inv_t) + 1e-6
    _check_topk(_ref_scores(Q, Cm, inv_t, True), vals, idx, k, tol)


def test_bf16_topk_one_million_rows(tt):
    g = torch.Generator(device=DEV).manual_seed(11)
    Q, Cm = _unit(7, 64, g), _unit(1 << 20, 64, g)
    for k in (10, 64):
        vals, idx = _run(tt, Q, Cm, k, 1.0, True)
        _check_topk(_ref_scores(Q, Cm, 1.0, True), vals, idx, k, 2e-5)


@pytest.mark.parametrize("nQ,nC,D,k,inv_t", [(7, 33, 100, 10, 0.05), (300, 1000, 64, 64, 1.0), (300, 65537, 32, 10, 0.05),
                                             (33, 1000, 6, 64, 1.0), (8192, 1000, 256, 10, 1.0)])
def test_f32_topk_vs_reference_and_dense_path(tt, nQ, nC, D, k, inv_t):
    from jodalrob_twotower_amd import ops
    g = torch.Generator(device=DEV).manual_seed(nQ + nC + D + k)
    Q, Cm = _unit(nQ, D, g), _unit(nC, D, g)
    vals, idx = _run(tt, Q, Cm, k, inv_t, False)
    S = _ref_scores(Q, Cm, inv_t, False)
    tol = 2e-6 * max(1.0, inv_t)
    _check_topk(S, vals, idx, k, tol)
    # rows without near-ties around their k best: the same indices as the dense tt_score_matrix + tt_topk_rows path
    dv, di = ops.topk_rows(ops.score_matrix(Q, Cm, inv_t), k)
    top = torch.topk(S, k + 1, dim=1).values                              # (nC > k in these cases)
    gaps = top[:, :-1] - top[:, 1:]
    edge = gaps[:, -1] > 10 * tol                                          # a clear k-th / (k+1)-th boundary: same index set
    assert float(edge.float().mean()) > 0.5
    assert torch.equal(torch.sort(idx[edge], 1).values, torch.sort(di[edge], 1).values)
    clear = gaps.min(dim=1).values > 10 * tol                              # no near-tie anywhere in the k best: same order
    assert torch.equal(idx[clear], di[clear])
    assert float((vals - dv).abs().max()) <= tol


@pytest.mark.parametrize("bf16", [True, False])
def test_duplicated_rows_come_in_ascending_index_order(tt, bf16):
    g = torch.Generator(device=DEV).manual_seed(3)
    base = _unit(40, 64, g)
    Cm = base[torch.arange(1000, device=DEV) % 40].contiguous()         # row j duplicates row j % 40
    Q = _unit(50, 64, g)
    vals, idx = _run(tt, Q, Cm, 64, 1.0, bf16)
    dv = vals[:, 1:] - vals[:, :-1]
    assert bool(((dv < 0) | (idx[:, 1:] > idx[:, :-1])).all())
    # the best base row's 25 copies come first, in ascending order, then the next base row's ...
    best = torch.argmax(_ref_scores(Q, base, 1.0, bf16), dim=1)
    assert torch.equal(idx[:, :25], best[:, None] + 40 * torch.arange(25, device=DEV)[None, :])
    assert bool((vals[:, :25] == vals[:, :1]).all())
    # every returned copy's lower-index copies are returned too
    for row in idx.cpu().numpy().tolist():
        assert all(j - 40 in set(row) for j in row if j >= 40)


@pytest.mark.parametrize("bf16", [True, False])
def test_bitwise_identical_across_runs_and_split_counts(tt, bf16):
    from jodalrob_twotower_amd import _lib as L
    g = torch.Generator(device=DEV).manual_seed(5)
    Q, Cm = _unit(300, 64, g), _unit(20000, 64, g)
    Cm[5000:5100] = Cm[100:200]                                          # exact ties across splits
    pos = torch.randint(0, 20000, (300,), generator=g, device=DEV)
    outs = []
    for s in (0, 0, 1, 2, 7, 32, 1000):
        L.set_option(torch.device(DEV), L.TT_OPT_RETRIEVE_SPLITS, s)
        outs.append(_run(tt, Q, Cm, 64, 1.0, bf16, positives=pos))
    for o in outs[1:]:
        assert torch.equal(o[0].view(torch.int32), outs[0][0].view(torch.int32))
        assert torch.equal(o[1], outs[0][1]) and torch.equal(o[2], outs[0][2])


@pytest.mark.parametrize("bf16", [True, False])
@pytest.mark.parametrize("nQ,nC,D", [(300, 1000, 64), (7, 65537, 100), (64, 33, 6)])
def test_rank_matches_reference_rule(tt, bf16, nQ, nC, D):
    g = torch.Generator(device=DEV).manual_seed(nQ + nC)
    Q, Cm = _unit(nQ, D, g), _unit(nC, D, g)
    pos64 = torch.randint(0, nC, (nQ,), generator=g, device=DEV)
    S = _ref_scores(Q, Cm, 1.0, bf16)
    r_only = _run(tt, Q, Cm, 0, 1.0, bf16, positives=pos64.to(torch.int32))
    _, _, r_k = _run(tt, Q, Cm, min(10, nC), 1.0, bf16, positives=pos64)
    assert torch.equal(r_only, r_k)                                      # k = 0 and k > 0, int32 and int64 positives
    tol = 4e-6
    sp = torch.gather(S, 1, pos64[:, None])
    lo = (S > sp + tol).sum(dim=1)
    hi = (S >= sp - tol).sum(dim=1) - 1
    r = r_only.long()
    assert bool(((r >= lo) & (r <= hi)).all())
    exact = lo == hi                                                    # no near-ties: the rule's value itself
    if nC <= 1000:                                                      # (65537 scores in [-1, 1]: near-ties are the rule)
        assert float(exact.float().mean()) > 0.5
    want = ref_rank(S.cpu().numpy(), pos64.cpu().numpy())
    assert np.array_equal(r.cpu().numpy()[exact.cpu().numpy()], want[exact.cpu().numpy()])


def test_rank_of_exact_ties_and_out_of_range_positives(tt):
    g = torch.Generator(device=DEV).manual_seed(9)
    base = _unit(10, 32, g)
    Cm = base[torch.arange(200, device=DEV) % 10].contiguous()
    Q = _unit(20, 32, g)
    pos = torch.randint(0, 200, (20,), generator=g, device=DEV)
    pos[3], pos[4] = -1, 200
    for bf16 in (True, False):
        r = _run(tt, Q, Cm, 0, 1.0, bf16, positives=pos).long().cpu()
        assert r[3] == -1 and r[4] == -1
        # the kernel's own scores are exact copies across duplicates: rank = (#better base rows) * 20 + copies before p
        B = (_bf16_round(Q).double() @ _bf16_round(base).double().T) if bf16 else (Q.double() @ base.double().T)
        for i in (0, 1, 2, 5, 6, 7):
            p = int(pos[i])
            better = int((B[i] > B[i, p % 10]).sum())
            assert int(r[i]) == better * 20 + p // 10


def test_rank_in_batch_equals_dense_diag_rank(tt):
    from jodalrob_twotower_amd import ops
    g = torch.Generator(device=DEV).manual_seed(21)
    N, Cm = _unit(512, 32, g), _unit(512, 32, g)
    inv_t = 2.0
    dense = ops.diag_rank_rows(ops.score_matrix(N, Cm, inv_t))
    r = _run(tt, N, Cm, 0, inv_t, False, positives=torch.arange(512, device=DEV))
    S = _ref_scores(N, Cm, inv_t, False)
    sp = torch.diagonal(S)[:, None]
    clear = ((S - sp).abs() > 1e-5).sum(dim=1) == 511                    # rows without a near-tie to the positive
    assert float(clear.float().mean()) > 0.95
    assert torch.equal(r[clear], dense[clear])
    _, _, r2 = _run(tt, N, Cm, 10, inv_t, False, positives=torch.arange(512, device=DEV))
    assert torch.equal(r, r2)


def test_error_paths_return_nonzero_and_launch_nothing(tt):
    from jodalrob_twotower_amd import _lib as L
    lib, dev = L.load(), torch.device(DEV)
    ctx, st = L.ctx(dev), L.stream(dev)
    g = torch.Generator(device=DEV).manual_seed(1)
    Q, Cm = _unit(8, 32, g), _unit(50, 32, g)
    assert lib.tt_retrieve_workspace_bytes(8, 50, 32, 64) == 0                     # k > nC: no valid size
    ws = torch.empty(lib.tt_retrieve_workspace_bytes(8, 50, 32, 50), dtype=torch.uint8, device=DEV)
    vals = torch.empty((8, 64), device=DEV)
    idx = torch.empty((8, 64), dtype=torch.int64, device=DEV)
    rank = torch.empty(8, dtype=torch.int32, device=DEV)
    pos = torch.zeros(8, dtype=torch.int64, device=DEV)
    p = L.ptr

    def f32(Qp, nC, k, vp, ip, pp, rp, wsz):
        return lib.tt_retrieve_topk_f32(ctx, Qp, 8, p(Cm), nC, 32, 1.0, k, pp, 1, vp, ip, rp, p(ws), wsz, st)

    ok = f32(p(Q), 50, 10, p(vals), p(idx), None, None, ws.numel())
    assert ok == 0, lib.tt_last_error_string()
    torch.cuda.synchronize()
    n0 = lib.tt_launch_count()
    bad = [f32(None, 50, 10, p(vals), p(idx), None, None, ws.numel()),          # NULL queries
           f32(p(Q), 50, 10, None, p(idx), None, None, ws.numel()),            # NULL vals
           f32(p(Q), 50, 10, p(vals), None, None, None, ws.numel()),           # NULL idx
           f32(p(Q), 50, 0, None, None, None, None, ws.numel()),               # k = 0 without positives
           f32(p(Q), 50, 65, p(vals), p(idx), None, None, ws.numel()),         # k = 65
           f32(p(Q), 20, 30, p(vals), p(idx), None, None, ws.numel()),         # k > nC
           f32(p(Q), 50, 10, p(vals), p(idx), p(pos), None, ws.numel()),       # positives without rank
           f32(p(Q), 50, 10, p(vals), p(idx), None, None, 64),                 # workspace too small
           lib.tt_retrieve_topk_f32(ctx, p(Q), 8, p(Cm), 50, 32, 1.0, 10, None, 0, p(vals), p(idx), None, None, ws.numel(), st),
           lib.tt_retrieve_topk_f32(ctx, p(Q), 8, p(Cm), 50, 257, 1.0, 10, None, 0, p(vals), p(idx), None, p(ws), ws.numel(), st),
           lib.tt_retrieve_topk_bf16(ctx, None, 8, p(Cm), 50, 32, 10, None, 0, p(vals), p(idx), None, p(ws), ws.numel(), st),
           lib.tt_retrieve_topk_bf16(None, p(Q), 8, p(Cm), 50, 32, 10, None, 0, p(vals), p(idx), None, p(ws), ws.numel(), st)]
    assert all(rc != 0 for rc in bad), bad
    assert lib.tt_launch_count() == n0


def test_search_can_be_captured_in_a_graph(tt):
    from jodalrob_twotower_amd.retrieval import CatalogIndex
    g = torch.Generator(device=DEV).manual_seed(4)
    Q, Cm = _unit(100, 64, g), _unit(5000, 64, g)
    index = CatalogIndex.from_embeddings(Cm, temperature=0.5, score_dtype="bf16")
    want = index.search(Q, 10)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        index.search(Q, 10)                                             # workspace of this stream exists before capture
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            got = index.search(Q, 10)
    torch.cuda.current_stream().wait_stream(s)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


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
    nN, nC = 700, 1500
    ns = {"dense_projected": rng.standard_normal((nN, cfg["din_n"])).astype(np.float32),
          "categorical": np.stack([rng.integers(0, v, nN) for v in cfg["vocab_n"]], 1)}
    cs = {"dense_projected": rng.standard_normal((nC, cfg["din_c"])).astype(np.float32),
          "categorical": np.stack([rng.integers(0, v, nC) for v in cfg["vocab_c"]], 1)}
    pairs = np.stack([rng.integers(0, nN, 3000), rng.integers(0, nC, 3000)], 1)
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


def test_from_store_rows_are_eval_company_embeddings(tt, trained):
    from jodalrob_twotower_amd.retrieval import CatalogIndex
    task, _, cstore, _, _ = trained
    task.train()
    before = _state(task)
    index = CatalogIndex.from_store(task, cstore, chunk=512)              # 3 chunks, the last one ragged
    assert task.training and all(m.training for m in task.modules()) and _same_state(before, _state(task))
    assert index.score_dtype == "fp32" and len(index) == len(cstore) and index.inv_t == 2.0
    ent = torch.tensor([0, 5, 511, 512, 1499, 77], device=DEV)
    task.eval()
    with torch.no_grad():
        want = task.two_tower_model.get_company_embeddings(cstore.gather(ent))
    task.train()
    torch.testing.assert_close(index.data[ent], want, rtol=1e-5, atol=1e-6)


def test_evaluate_catalog_and_predict_catalog(tt, trained):
    from jodalrob_twotower_amd.retrieval import CatalogIndex
    task, nstore, cstore, loader, pairs = trained
    ev = tt.TwoTowerEvaluator(device=DEV)
    index = CatalogIndex.from_store(task, cstore)
    task.train()
    before = _state(task)
    sub = pairs[:1000]
    m = ev.evaluate_catalog(task, nstore, index, sub, batch_size=1000)
    m300 = ev.evaluate_catalog(task, nstore, index, sub, batch_size=300)
    assert m300["num_queries"] == 1000 and abs(m300["mrr"] - m["mrr"]) < 0.01
    assert m["catalog_size"] == 1500 and m["num_queries"] == 1000
    task.eval()
    with torch.no_grad():
        q = task.two_tower_model.get_notice_embeddings(nstore.gather(torch.as_tensor(sub[:, 0], device=DEV)))
    task.train()
    r = index.rank(q, torch.as_tensor(sub[:, 1], device=DEV)).cpu().numpy()
    for k in (5, 10):
        assert m[f"recall@{k}"] == pytest.approx(float((r < k).mean()), abs=1e-6)
    assert m["mrr"] == pytest.approx(float((1.0 / (r + 1.0)).mean()), rel=1e-5)
    # predict_catalog = search on the eval-mode notice embeddings
    batch = loader.batch(None, 0)
    pred = task.predict_catalog(batch["notice"], index, top_k=10)
    task.eval()
    with torch.no_grad():
        qb = task.two_tower_model.get_notice_embeddings(batch["notice"])
    task.train()
    vals, idx = index.search(qb, 10)
    assert torch.equal(pred["top_indices"], idx) and torch.equal(pred["top_similarities"], vals)
    assert task.training and _same_state(before, _state(task))


def test_catalog_of_one_batch_matches_in_batch_metrics(tt, trained):
    from jodalrob_twotower_amd.retrieval import CatalogIndex
    task, nstore, _, loader, pairs = trained
    ev = tt.TwoTowerEvaluator(device=DEV)
    batch = loader.batch(None, 0)
    B = batch["company"]["dense"].shape[0]
    task.eval()
    with torch.no_grad():
        comp = task.two_tower_model.get_company_embeddings(batch["company"])
    index = CatalogIndex.from_embeddings(comp, temperature=task.temperature, score_dtype="fp32")
    inb = ev.evaluate_single_batch(task, batch, verbose=False)
    task.train()
    cat = ev.evaluate_catalog(task, nstore, index, np.stack([pairs[:B, 0], np.arange(B)], 1))
    for key in ("recall@5", "recall@10", "mrr"):
        assert cat[key] == pytest.approx(inb[key], abs=1.0 / B), key
    assert cat["catalog_size"] == B and cat["num_queries"] == B
