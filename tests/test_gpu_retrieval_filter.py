"""GPU tests of per-query attribute filters in catalogue-wide retrieval (tt_filt_retrieve_topk_bf16 / _f32): top-k and rank
against a masked f64 reference of the same rounded operands, bitwise equality with the plain and the exclusion entries for
neutral masks, bitwise determinism across split counts with eligibility flipping at tile and split boundaries, a restricted
search against a plain search over the compacted catalogue, filter plus exclusion lists, the rank identity against the plain
entry, short eligible sets, graph capture, the error paths, and the restricted evaluation end to end on a trained task."""
import numpy as np
import pytest
import torch

from conftest import GOLD
from test_gpu_retrieval_exclude import (CASES, _check_rank_masked, _check_topk_masked, _dev, _mask, _random_lists, _ref_scores,
                                        _same_state, _state, _unit)
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


def _words(x):
    """numpy integer words (values in [0, 2^32)) -> int32 device tensor of the same bit patterns."""
    return torch.as_tensor(np.ascontiguousarray(np.asarray(x).astype(np.uint32).view(np.int32)), device=DEV)


def _run(Q, Cm, k, inv_t, bf16, positives=None, exclude=None, filt=None):
    """(vals, idx, rank) from one ops-level call; filt = (tags, any, all) numpy words or device int32 tensors (masks may be None)."""
    from jodalrob_twotower_amd import ops
    nQ, D = Q.shape
    nC = Cm.shape[0]
    if filt is not None:
        t, a, r = [x if x is None or torch.is_tensor(x) else _words(x) for x in filt]
        filt = (t, t.shape[1], a, r)
    if bf16:
        q, c = ops.score_pack_bf16(Q, 1.0), ops.score_pack_bf16(Cm, inv_t)
        out = ops._retrieve(q, nQ, c, nC, D, k, 1.0, True, positives, None, exclude, filt)
    else:
        out = ops._retrieve(Q, nQ, Cm, nC, D, k, inv_t, False, positives, None, exclude, filt)
    torch.cuda.synchronize()
    return out


def _random_filter(nQ, nC, W, rng):
    """Tags: the AND of two random words (each bit set with probability 1/4).  any: a random 4-bit mask, zero for every third
    query.  all: sparse (0, 0, 1 or 2 bits).  About 45 % of the pairs are eligible."""
    tags = rng.integers(0, 1 << 32, (nC, W), dtype=np.uint64) & rng.integers(0, 1 << 32, (nC, W), dtype=np.uint64)
    any_m = np.zeros((nQ, W), dtype=np.uint64)
    all_m = np.zeros((nQ, W), dtype=np.uint64)
    for q in range(nQ):
        if q % 3:
            for b in rng.integers(0, 32 * W, 4):
                any_m[q, b // 32] |= np.uint64(1 << (b % 32))
        for b in rng.integers(0, 32 * W, rng.choice([0, 0, 1, 2])):
            all_m[q, b // 32] |= np.uint64(1 << (b % 32))
    return tags, any_m, all_m


def _elig_mask(S, elig):
    M = S.clone()
    M[~torch.as_tensor(elig, device=DEV)] = -float("inf")
    return M


def _bits_equal(a, b):
    return torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1]) and \
        (a[2] is None and b[2] is None or torch.equal(a[2], b[2]))


@pytest.mark.parametrize("bf16", [True, False])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_topk_and_rank_vs_masked_reference(tt, bf16, case):
    nQ, nC, D, k, inv_t = CASES[case]
    W = (1, 2, 4)[case % 3]
    g = torch.Generator(device=DEV).manual_seed(nQ * 5 + nC + D + k)
    rng = np.random.default_rng(nQ + nC + D + k)
    Q, Cm = _unit(nQ, D, g), _unit(nC, D, g)
    tags, any_m, all_m = _random_filter(nQ, nC, W, rng)
    if nQ > 2 and nC <= 1000:
        any_m[1], all_m[1] = 0, tags[5]                                # row 5 and hardly another hold all of its bits
        any_m[2], all_m[2] = 0, 0xFFFFFFFF                             # no eligible row
    pos = torch.as_tensor(rng.integers(0, nC, nQ), device=DEV)
    vals, idx, rank = _run(Q, Cm, k, inv_t, bf16, positives=pos, filt=(tags, any_m, all_m))
    elig = ref_eligible(tags, any_m, all_m)
    if nQ > 2 and nC <= 1000:
        assert 1 <= elig[1].sum() < 4 and elig[2].sum() == 0
        assert 0.35 < elig[3:].mean() < 0.55
    S = _ref_scores(Q, Cm, inv_t, bf16)
    M = _elig_mask(S, elig)
    tol = (1e-5 if bf16 else 2e-6) * max(1.0, inv_t) + 1e-6
    _check_topk_masked(M, vals, idx, k, tol)
    exact = _check_rank_masked(S, M, pos, rank, tol)
    if nC <= 1000:
        assert float(exact.float().mean()) > 0.5
    r_only = _run(Q, Cm, 0, inv_t, bf16, positives=pos.to(torch.int32), filt=(tags, any_m, all_m))[2]
    assert torch.equal(r_only, rank)                                   # k = 0 and k > 0, int32 and int64 positives
    # one mask at a time: the other pointer NULL
    for a, r in ((any_m, None), (None, all_m)):
        v1, i1, r1 = _run(Q, Cm, k, inv_t, bf16, positives=pos, filt=(tags, a, r))
        M1 = _elig_mask(S, ref_eligible(tags, a, r))
        _check_topk_masked(M1, v1, i1, k, tol)
        _check_rank_masked(S, M1, pos, r1, tol)


@pytest.mark.parametrize("bf16", [True, False])
@pytest.mark.parametrize("W", [1, 3])
def test_neutral_masks_are_bitwise_the_plain_and_the_exclusion_entry(tt, bf16, W):
    g = torch.Generator(device=DEV).manual_seed(7)
    nQ, nC = 300, 20011
    Q, Cm = _unit(nQ, 64, g), _unit(nC, 64, g)
    pos = torch.randint(0, nC, (nQ,), generator=g, device=DEV)
    pos[:3] = torch.tensor([-1, nC, nC + 5], device=DEV)
    rng = np.random.default_rng(1)
    tags = rng.integers(0, 1 << 32, (nC, W), dtype=np.uint64)
    zero = np.zeros((nQ, W), dtype=np.uint64)
    plain = _run(Q, Cm, 64, 1.0, bf16, positives=pos)
    for filt in ((tags, zero, zero), (tags, zero, None), (tags, None, zero)):
        assert _bits_equal(_run(Q, Cm, 64, 1.0, bf16, positives=pos, filt=filt), plain)
    ex = _dev(*_random_lists(nQ, nC, 300, rng))
    excl = _run(Q, Cm, 64, 1.0, bf16, positives=pos, exclude=ex)
    assert not torch.equal(excl[1], plain[1])
    assert _bits_equal(_run(Q, Cm, 64, 1.0, bf16, positives=pos, exclude=ex, filt=(tags, zero, zero)), excl)
    r_plain = _run(Q, Cm, 0, 1.0, bf16, positives=pos)[2]
    assert torch.equal(_run(Q, Cm, 0, 1.0, bf16, positives=pos, filt=(tags, zero, zero))[2], r_plain)


@pytest.mark.parametrize("bf16", [True, False])
@pytest.mark.parametrize("W", [1, 2, 3, 4])
def test_bitwise_identical_across_split_counts(tt, bf16, W):
    from jodalrob_twotower_amd import _lib as L
    g = torch.Generator(device=DEV).manual_seed(5)
    nQ, nC = 70, 20011                                                 # ragged last tile (11 rows)
    Q, Cm = _unit(nQ, 64, g), _unit(nC, 64, g)
    Cm[5000:5100] = Cm[100:200]                                        # exact ties across splits
    pos = torch.randint(0, nC, (nQ,), generator=g, device=DEV)
    nT = (nC + 31) // 32
    bounds = sorted({32 * (nT * s // S) for S in (2, 7, 32) for s in range(1, S)})
    # bit b of word b // 32: eligibility of the rows flips exactly at every tile boundary (bit 0), at every split boundary (bit
    # 33 % (32 W)), row by row in the ragged last tile (bit 2), and on one of each pair of tied rows (bit 3)
    rows = np.arange(nC)
    bit = np.zeros((nC, 32 * W), dtype=bool)
    bit[:, 0] = (rows // 32) % 2 == 0
    bit[:, 33 % (32 * W)] = np.searchsorted(bounds, rows, side="right") % 2 == 0
    bit[:, 2] = (rows >= nC - 11) & (rows % 2 == 1)
    bit[:, 3] = rows < 5050
    bit[:, 32 * W - 1] = rows % 3 == 0
    tags = np.zeros((nC, W), dtype=np.uint64)
    for b in range(32 * W):
        tags[:, b // 32] |= bit[:, b].astype(np.uint64) << np.uint64(b % 32)
    any_m = np.zeros((nQ, W), dtype=np.uint64)
    all_m = np.zeros((nQ, W), dtype=np.uint64)
    for q in range(nQ):
        for m, sel in ((any_m, q % 5), (all_m, q // 5 % 5)):
            for b in {0: [], 1: [0], 2: [33 % (32 * W)], 3: [2, 3], 4: [32 * W - 1, 0]}[sel]:
                m[q, b // 32] |= np.uint64(1 << (b % 32))
    filt = (_words(tags), _words(any_m), _words(all_m))
    outs = []
    for s in (0, 0, 1, 2, 7, 32):
        L.set_option(torch.device(DEV), L.TT_OPT_RETRIEVE_SPLITS, s)
        outs.append(_run(Q, Cm, 64, 1.0, bf16, positives=pos, filt=filt))
    for o in outs[1:]:
        assert _bits_equal(o, outs[0])
    S = _ref_scores(Q, Cm, 1.0, bf16)
    M = _elig_mask(S, ref_eligible(tags, any_m, all_m))
    _check_topk_masked(M, outs[0][0], outs[0][1], 64, 2e-5 if bf16 else 3e-6)
    _check_rank_masked(S, M, pos, outs[0][2], 2e-5 if bf16 else 3e-6)


@pytest.mark.parametrize("bf16", [True, False])
@pytest.mark.parametrize("share", [0.5, 0.03])
def test_subset_search_equals_plain_search_of_the_compacted_catalogue(tt, bf16, share):
    g = torch.Generator(device=DEV).manual_seed(21)
    rng = np.random.default_rng(6)
    nQ, nC, k = 100, 30000, 32
    Q, Cm = _unit(nQ, 64, g), _unit(nC, 64, g)
    Cm[20000:20200] = Cm[:200]                                         # exact ties: the order by index survives compaction
    member = rng.random(nC) < share
    tags = np.where(member, 1 << 9, 1 << 8).astype(np.uint64)[:, None] | rng.integers(0, 256, (nC, 1), dtype=np.uint64)
    keep = torch.as_tensor(np.nonzero(member)[0], device=DEV)
    want_v, want_i, _ = _run(Q, Cm[keep].contiguous(), k, 1.0, bf16)
    for filt in ((tags, np.full((nQ, 1), 1 << 9), None), (tags, None, np.full((nQ, 1), 1 << 9))):
        v, i, _ = _run(Q, Cm, k, 1.0, bf16, filt=filt)
        assert torch.equal(v.view(torch.int32), want_v.view(torch.int32))
        assert torch.equal(i, keep[want_i])


@pytest.mark.parametrize("bf16", [True, False])
@pytest.mark.parametrize("nQ,nC,D,k,W", [(33, 1000, 200, 64, 2), (300, 65537, 64, 10, 4)])
def test_filter_and_exclusion_lists_together(tt, bf16, nQ, nC, D, k, W):
    g = torch.Generator(device=DEV).manual_seed(nQ + W)
    rng = np.random.default_rng(nC + W)
    Q, Cm = _unit(nQ, D, g), _unit(nC, D, g)
    tags, any_m, all_m = _random_filter(nQ, nC, W, rng)
    off, rows = _random_lists(nQ, nC, 300, rng)
    pos = torch.as_tensor(rng.integers(0, nC, nQ), device=DEV)
    vals, idx, rank = _run(Q, Cm, k, 1.0, bf16, positives=pos, exclude=_dev(off, rows), filt=(tags, any_m, all_m))
    S = _ref_scores(Q, Cm, 1.0, bf16)
    M = _mask(_elig_mask(S, ref_eligible(tags, any_m, all_m)), off, rows)
    tol = (1e-5 if bf16 else 2e-6) + 1e-6
    _check_topk_masked(M, vals, idx, k, tol)
    _check_rank_masked(S, M, pos, rank, tol)
    only_f = _run(Q, Cm, k, 1.0, bf16, positives=pos, filt=(tags, any_m, all_m))
    only_x = _run(Q, Cm, k, 1.0, bf16, positives=pos, exclude=_dev(off, rows))
    assert not torch.equal(idx, only_f[1]) and not torch.equal(idx, only_x[1])
    assert bool((rank <= only_f[2]).all()) and bool((rank <= only_x[2]).all())


@pytest.mark.parametrize("bf16", [True, False])
def test_rank_drops_by_the_ineligible_rows_that_outrank_p(tt, bf16):
    g = torch.Generator(device=DEV).manual_seed(12)
    nQ, nC, W = 64, 5000, 2
    Q, Cm = _unit(nQ, 64, g), _unit(nC, 64, g)
    Cm[4000:4100] = Cm[:100]                                           # exact ties
    rng = np.random.default_rng(4)
    pos = rng.integers(0, nC, nQ)
    pos[:8] = np.arange(8) + 4000                                      # positives among the tied rows
    tags, any_m, all_m = _random_filter(nQ, nC, W, rng)
    elig = ref_eligible(tags, any_m, all_m)
    pos_t = torch.as_tensor(pos, device=DEV)
    r_plain = _run(Q, Cm, 0, 1.0, bf16, positives=pos_t)[2].long()
    r_filt = _run(Q, Cm, 0, 1.0, bf16, positives=pos_t, filt=(tags, any_m, all_m))[2].long()
    p_ok = torch.as_tensor(elig[np.arange(nQ), pos], device=DEV)
    assert int(p_ok.sum()) > 10 and int((~p_ok).sum()) > 10
    assert bool((r_filt <= r_plain).all())                             # (eligible positive or not: rows only leave)
    # the ineligible rows that outrank p under the rule, from the f64 reference where it has no near-tie
    S = _ref_scores(Q, Cm, 1.0, bf16)
    sp = torch.gather(S, 1, pos_t[:, None])
    cols = torch.arange(nC, device=DEV)[None, :]
    inel = ~torch.as_tensor(elig, device=DEV) & (cols != pos_t[:, None])
    tol = 2e-5 if bf16 else 3e-6
    near = (((S - sp).abs() <= tol) & (S != sp) & (cols != pos_t[:, None])).any(1)
    outr = (inel & ((S > sp) | ((S == sp) & (cols < pos_t[:, None])))).sum(1)
    assert int((~near).sum()) > nQ // 2 and int(outr.sum()) > 0
    assert torch.equal(r_filt[~near], (r_plain - outr)[~near])


@pytest.mark.parametrize("bf16", [True, False])
def test_fewer_eligible_rows_than_k(tt, bf16):
    g = torch.Generator(device=DEV).manual_seed(8)
    nQ, nC, k = 40, 300, 10
    Q, Cm = _unit(nQ, 32, g), _unit(nC, 32, g)
    rng = np.random.default_rng(3)
    # row c holds bit c % 10 of word 1 and 25 rows also bit 20 of word 0: query q requires bit 20 and allows q % 10 residues
    tags = np.zeros((nC, 2), dtype=np.uint64)
    tags[:, 1] = 1 << (np.arange(nC) % 10)
    special = rng.choice(nC, 25, replace=False)
    tags[special, 0] = 1 << 20
    any_m = np.zeros((nQ, 2), dtype=np.uint64)
    all_m = np.zeros((nQ, 2), dtype=np.uint64)
    all_m[:, 0] = 1 << 20
    for q in range(nQ):
        any_m[q, 1] = (1 << (q % 10)) - 1 if q % 10 else 1 << 15      # residues 0 .. q % 10 - 1; bit 15: nobody
    elig = ref_eligible(tags, any_m, all_m)
    n_el = elig.sum(1)
    assert (n_el[::10] == 0).all() and (n_el < k).sum() >= 12 and (n_el >= k).sum() >= 8
    vals, idx, rank = _run(Q, Cm, k, 1.0, bf16, positives=torch.zeros(nQ, dtype=torch.int64, device=DEV),
                           filt=(tags, any_m, all_m))
    S = _ref_scores(Q, Cm, 1.0, bf16)
    for q in range(nQ):
        j = min(int(n_el[q]), k)
        got = idx[q].cpu().numpy()
        if j < k:
            assert sorted(got[:j].tolist()) == np.nonzero(elig[q])[0].tolist(), q
        assert (got[j:] == -1).all() and bool((vals[q, j:] == -float("inf")).all())
        kp = torch.as_tensor(np.nonzero(elig[q] & (np.arange(nC) != 0))[0], device=DEV, dtype=torch.int64)
        assert int(rank[q]) == int((S[q, kp] > S[q, 0]).sum()), q
        if n_el[q] == 0:
            assert int(rank[q]) == 0
    _check_topk_masked(_elig_mask(S, elig), vals, idx, k, 2e-5)


def test_filtered_search_can_be_captured_in_a_graph(tt):
    from jodalrob_twotower_amd.retrieval import CatalogIndex, onehot_bits
    g = torch.Generator(device=DEV).manual_seed(4)
    Q, Cm = _unit(100, 64, g), _unit(5000, 64, g)
    rng = np.random.default_rng(5)
    region = torch.as_tensor(rng.integers(0, 40, 5000), device=DEV)
    index = CatalogIndex.from_embeddings(Cm, temperature=0.5, score_dtype="bf16", tags=onehot_bits(region, 40))
    assert index.tag_words == 2
    allow = onehot_bits(torch.as_tensor(rng.integers(0, 40, 100), device=DEV), 40)
    other = onehot_bits(torch.as_tensor(rng.integers(-1, 40, 100), device=DEV), 40) | allow.roll(1, 0)
    want = index.search(Q, 10, allow=allow)
    want_other = index.search(Q, 10, allow=other)
    assert not torch.equal(want[1], want_other[1])
    buf = allow.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        index.search(Q, 10, allow=buf)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            got = index.search(Q, 10, allow=buf)
    torch.cuda.current_stream().wait_stream(s)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(got[0].view(torch.int32), want[0].view(torch.int32)) and torch.equal(got[1], want[1])
    buf.copy_(other)                                                   # the masks changed in place: the replay sees them
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(got[0].view(torch.int32), want_other[0].view(torch.int32)) and torch.equal(got[1], want_other[1])
    reg = region.cpu().numpy()
    al = other.cpu().numpy().view(np.uint32)
    for q in range(100):                                               # only allowed regions come back
        for c in got[1][q].tolist():
            assert c == -1 or (al[q, reg[c] // 32] >> (reg[c] % 32)) & 1, (q, c)


def test_error_paths_return_nonzero_and_launch_nothing(tt):
    from jodalrob_twotower_amd import _lib as L
    lib, dev = L.load(), torch.device(DEV)
    ctx, st = L.ctx(dev), L.stream(dev)
    g = torch.Generator(device=DEV).manual_seed(1)
    Q, Cm = _unit(8, 32, g), _unit(50, 32, g)
    ws = torch.empty(lib.tt_retrieve_workspace_bytes(8, 50, 32, 10), dtype=torch.uint8, device=DEV)
    vals = torch.full((8, 10), 7.0, device=DEV)
    idx = torch.full((8, 10), 7, dtype=torch.int64, device=DEV)
    off = torch.zeros(9, dtype=torch.int64, device=DEV)
    rows = torch.zeros(4, dtype=torch.int32, device=DEV)
    tags = torch.zeros(50 * 5 + 4, dtype=torch.int32, device=DEV)      # spare elements for W = 5 and the misaligned view
    qa = torch.zeros(8 * 5, dtype=torch.int32, device=DEV)
    ql = torch.zeros(8 * 5, dtype=torch.int32, device=DEV)
    p = L.ptr
    qb = torch.zeros(lib.tt_score_pack_bytes(8, 32), dtype=torch.uint8, device=DEV)
    cb = torch.zeros(lib.tt_score_pack_bytes(50, 32), dtype=torch.uint8, device=DEV)

    def f32(op, rp, tp, W, ap, lp, wsz=ws.numel()):
        return lib.tt_filt_retrieve_topk_f32(ctx, p(Q), 8, p(Cm), 50, 32, 1.0, 10, None, 0, p(vals), p(idx), None, op, rp, tp, W,
                                             ap, lp, p(ws), wsz, st)

    def bf16(op, rp, tp, W, ap, lp, wsz=ws.numel()):
        return lib.tt_filt_retrieve_topk_bf16(ctx, p(qb), 8, p(cb), 50, 32, 10, None, 0, p(vals), p(idx), None, op, rp, tp, W, ap,
                                              lp, p(ws), wsz, st)

    torch.cuda.synchronize()
    n0 = lib.tt_launch_count()
    mis_tags = L.vp(tags.data_ptr() + 4)
    mis_mask = L.vp(qa.data_ptr() + 2)
    bad = []
    for fn in (f32, bf16):
        bad += [fn(None, None, p(tags), 0, p(qa), p(ql)),              # W = 0
                fn(None, None, p(tags), 5, p(qa), p(ql)),              # W = 5
                fn(None, None, p(tags), 1, None, None),                # both masks NULL
                fn(p(off), None, p(tags), 1, p(qa), p(ql)),            # half an exclusion pair
                fn(None, p(rows), p(tags), 1, p(qa), p(ql)),
                fn(None, None, mis_tags, 1, p(qa), p(ql)),             # tags not 16-byte aligned
                fn(None, None, None, 1, p(qa), p(ql)),                 # NULL tags
                fn(None, None, p(tags), 1, mis_mask, None),            # mask not 4-byte aligned
                fn(None, None, p(tags), 1, p(qa), p(ql), 64)]          # workspace too small
    assert all(rc == -1 for rc in bad), bad                            # TT_ERR_INVALID_ARG
    assert lib.tt_launch_count() == n0
    torch.cuda.synchronize()
    assert bool((vals == 7.0).all()) and bool((idx == 7).all())        # the pre-filled outputs are untouched
    for W in (1, 4):                                                   # the same calls with good arguments run
        assert f32(None, None, p(tags), W, p(qa), None) == 0, lib.tt_last_error_string()
        assert f32(p(off), p(rows), p(tags), W, None, p(ql)) == 0, lib.tt_last_error_string()
    torch.cuda.synchronize()
    assert lib.tt_launch_count() == n0 + 4 * 2                         # sweep and merge (no positives: no pos launch)
    assert bool((idx >= 0).all())


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


def test_restricted_evaluate_catalog_and_predict_catalog(tt, trained):
    from jodalrob_twotower_amd.retrieval import CatalogIndex, equality_bits, onehot_bits
    task, nstore, cstore, loader, pairs = trained
    ev = tt.TwoTowerEvaluator(device=DEV)
    rng = np.random.default_rng(9)
    V = 37
    region = torch.as_tensor(rng.integers(0, V, 1500), device=DEV)      # a "region code" per company
    licence = torch.as_tensor(rng.integers(0, 5, 1500), device=DEV)
    tags = equality_bits(region, V, words=2) | onehot_bits(licence, 5, first_bit=40, words=2)
    task.train()
    before = _state(task)
    index = CatalogIndex.from_store(task, cstore, tags=tags)
    assert index.tag_words == 2 and torch.equal(index.tags, tags)
    sub = pairs[:1000]
    pos = torch.as_tensor(sub[:, 1], device=DEV)
    require = equality_bits(region[pos], V, words=2)                    # every query: the region of its own positive
    allow = onehot_bits(licence[pos], 5, first_bit=40, words=2) | onehot_bits((licence[pos] + 1) % 5, 5, first_bit=40, words=2)
    raw = ev.evaluate_catalog(task, nstore, index, sub, batch_size=300)
    assert ev.evaluate_catalog(task, nstore, index, sub, batch_size=300, allow=None, require=None) == raw
    res = ev.evaluate_catalog(task, nstore, index, sub, batch_size=300, allow=allow, require=require)
    assert res.keys() == raw.keys() and res["num_queries"] == 1000 and res["catalog_size"] == 1500
    for key in ("recall@5", "recall@10", "mrr"):
        assert res[key] >= raw[key], key                               # every positive is eligible: rows only leave
    assert res["mrr"] > raw["mrr"]
    # the f64 dense masked reference
    task.eval()
    with torch.no_grad():
        q = task.two_tower_model.get_notice_embeddings(nstore.gather(torch.as_tensor(sub[:, 0], device=DEV)))
    task.train()
    S = (q.double() @ index.data.double().T) * index.inv_t
    lic = licence[None, :]
    elig = (region[None, :] == region[pos][:, None]) & ((lic == licence[pos][:, None]) | (lic == (licence[pos][:, None] + 1) % 5))
    assert np.array_equal(ref_eligible(tags.cpu().numpy(), allow.cpu().numpy(), require.cpu().numpy()), elig.cpu().numpy())
    M = S.clone()
    M[~elig] = -float("inf")
    r = index.rank(q, pos, allow=allow, require=require)
    exact = _check_rank_masked(S, M, pos, r, 1e-5)
    assert float(exact.float().mean()) > 0.95
    for k in (5, 10):
        assert res[f"recall@{k}"] == pytest.approx(float((r < k).float().mean()), abs=1e-6)
    assert res["mrr"] == pytest.approx(float((1.0 / (r.double() + 1.0)).mean()), rel=1e-5)
    # predict_catalog never returns an ineligible company
    batch = loader.batch(None, 0)
    B = batch["notice"]["dense"].shape[0]                              # (shuffle=False: batch 0 = pairs[:B])
    pred = task.predict_catalog(batch["notice"], index, top_k=64, allow=allow[:B], require=require[:B])
    got = pred["top_indices"]
    ok = torch.gather(elig[:B], 1, got.clamp(min=0))
    assert bool((ok | (got < 0)).all()) and bool((got < 0).any()) and bool((got >= 0).any())
    n_el = elig[:B].sum(1).clamp(max=64)
    assert torch.equal((got >= 0).sum(1), n_el)
    assert task.training and _same_state(before, _state(task))
