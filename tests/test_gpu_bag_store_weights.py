"""tt_bag_store_gather_w on the MI355X: the batch gather out of a bag store that keeps one f32 weight per id, against the torch
reference of tests/_bag_store_weight_reference.py.  The gather copies, so every comparison is bit for bit (weights through their
int32 patterns: NaN payloads, -0.0 and denormals count).

The store: N = 37 entities, run lengths from {0, 1, 2, 7} (several entities wholly empty), one entity with 3000 ids -- one run that
spans lanes, trips and the workgroups that share a tile.  Its id and weight arrays start with 1 or 3 dummy entries the offsets skip,
which puts the sources at odd offsets (ids 8 mod 16; weights 4 / 12 mod 16).  The destinations are views into larger buffers
prefilled with a sentinel pattern: ids_out at 0 / 8 mod 16, weights_out at 0 / 4 / 8 / 12 mod 16, guard words on both sides."""
import numpy as np
import pytest
import torch

import _bag_store_reference as R
import _bag_store_weight_reference as RW
from test_gpu_parity import DEV, tt  # noqa: F401

from jodalrob_twotower_amd import _lib as _L
from jodalrob_twotower_amd import ops

pytestmark = pytest.mark.gpu

N, LONG, DIN = 37, 20, 8
EMPTY = (3, 11, 12, 30)                                  # entities without any id
SENT = -0x5A5A5A5A5A5A5A5A                               # the id buffers' sentinel
WSENT = 0x7FA5A5A5                                       # the weight buffers': a NaN pattern no store weight carries
SIZES = [1, 255, 256, 257, 513]
GUARD = 4                                                # elements in front of every view: a whole number of 16-byte pieces
ERR = r"status -5\).*device error word 0x8:.*bag offsets"


def _host_store(K, prefix, seed=0):
    """(dense, offsets, values, weights) on the host; offsets[0] = prefix: the first `prefix` ids and weights belong to nobody"""
    rng = np.random.default_rng(100 * K + prefix + seed)
    lengths = np.zeros((N, K), dtype=np.int64)
    for e in range(N):
        run = 3000 if e == LONG else (0 if e in EMPTY else (2 if e == N - 1 else int(rng.choice([0, 1, 2, 7]))))      # (B = 1 names entity N - 1)
        for _ in range(run):                              # the run's ids spread over the entity's K bags
            lengths[e, rng.integers(0, K)] += 1
    nnz = int(lengths.sum())
    offsets = torch.from_numpy(prefix + np.concatenate([[0], np.cumsum(lengths.reshape(-1))]).astype(np.int64))
    values = torch.from_numpy(np.concatenate([np.full(prefix, -77), rng.integers(-5, 2 ** 33, nnz)]).astype(np.int64))
    weights = torch.from_numpy(np.concatenate([np.full(prefix, 77.0), rng.standard_normal(nnz)]).astype(np.float32))
    dense = torch.from_numpy(rng.standard_normal((N, DIN)).astype(np.float32))
    assert int((lengths.sum(1) == 0).sum()) >= len(EMPTY) and offsets[-1] == values.numel() == weights.numel()
    return dense, offsets, values, weights


@pytest.fixture(scope="module")
def stores():
    """{(K, prefix): (host tensors, the same on the device)} and, under "plain", the unweighted second side (K = 2)"""
    out = {(K, p): _host_store(K, p) for K in (1, 3) for p in (1, 3)}
    out["plain"] = _host_store(2, 0, seed=50)[:3]
    return {k: (v, tuple(t.to(DEV) for t in v)) for k, v in out.items()}


def _entities(B, seed, tile_edge=False):
    """B entity indices: repeats, the long run, empty entities, indices outside the store (clamped into it)"""
    rng = np.random.default_rng(seed)
    e = rng.integers(0, N, B)
    if tile_edge:                                         # B = 513: a tile of empty samples between two full ones
        full = np.array([i for i in range(N) if i not in EMPTY and i != LONG])
        e = np.concatenate([full[rng.integers(0, len(full), 256)], np.array(EMPTY)[rng.integers(0, len(EMPTY), 256)], [LONG]])
    elif B >= 8:
        e[:7] = [0, LONG, EMPTY[0], -3, N + 5, e[7], e[7]]
    e[-1] = N - 1 if not tile_edge else e[-1]
    return torch.from_numpy(e.astype(np.int64))


@pytest.fixture(scope="module")
def references(stores):
    """{(B, K, prefix): (entities per side, weighted reference, the plain side's reference)}, computed once on the host"""
    out = {}
    for B in SIZES:
        for (K, p) in [k for k in stores if k != "plain"]:
            ents = [_entities(B, 1000 * B + 10 * K + p + i) for i in range(2)]
            out[B, K, p] = (ents, RW.gather(*stores[K, p][0], K, ents[0]), R.gather(*stores["plain"][0], 2, ents[1]))
    return out


def _view(total_len, shift, dtype, fill):
    """(buffer, view of total_len elements starting GUARD + shift elements in): guard words on both sides of the view"""
    buf = torch.empty(GUARD + shift + total_len + 16, dtype=dtype, device=DEV)
    (buf.view(torch.int32) if dtype == torch.float32 else buf).fill_(fill)
    return buf, buf[GUARD + shift:GUARD + shift + total_len]


def _untouched(buf, lo, hi, fill):
    """everything of `buf` outside [lo, hi) still holds the sentinel"""
    b = (buf.view(torch.int32) if buf.dtype == torch.float32 else buf).cpu()
    return bool((b[:lo] == fill).all()) and bool((b[hi:] == fill).all())


def _pair_list(ents, use_order, seed):
    B = ents[0].numel()
    g = torch.Generator().manual_seed(seed)
    P, off = B + 11, 5
    pairs = torch.randint(0, N, (P, 2), generator=g)
    batch = torch.stack(ents, 1)
    if use_order:
        order = torch.randperm(P, generator=g)
        pairs[order[off:off + B]] = batch
        return pairs.to(DEV), order.to(DEV), off
    pairs[off:off + B] = batch
    return pairs.to(DEV), None, off


def _side(store_dev, K, flat, col, B, ids_out, expect, w_out=None, weighted=True):
    dense, offsets, values = store_dev[:3]
    d = torch.full((B, DIN), float("nan"), device=DEV)
    ln = torch.full((B * K,), SENT, dtype=torch.int64, device=DEV)
    w = store_dev[3] if weighted and len(store_dev) > 3 else None
    return ops.BagStoreSide(flat[col:], 2, dense, offsets, values, K, d, ln, ids_out, expect, w, w_out if w is not None else None)


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("B", SIZES)
def test_weighted_gather_equals_the_reference_at_every_alignment(tt, stores, references, B, K):
    dev = torch.device(DEV)
    _L.check_device_errors(dev)
    seen = set()
    for prefix in (1, 3):
        ents, (rd, rl, ri, rw), (pd, pl, pi) = references[B, K, prefix]
        n, n_plain = ri.numel(), pi.numel()
        if B >= 8:
            assert n > 3000 and int((rl.view(B, K).sum(1) == 0).sum()) > 0
        for use_order in (True, False):
            pairs, order, off = _pair_list(ents, use_order, B + prefix)
            flat, base = pairs.view(-1), (0 if use_order else 2 * off)
            slack = 0 if use_order else 17                # with order: capacity == total, no expect; without: 17 spare, the count given
            for ishift in (0, 1):
                for wshift in (0, 1, 2, 3):
                    ibuf, iv = _view(n + slack, ishift, torch.int64, SENT)
                    wbuf, wv = _view(n + slack, wshift, torch.float32, WSENT)
                    pbuf, pv = _view(n_plain + slack, ishift ^ 1, torch.int64, SENT)
                    assert iv.data_ptr() % 16 == 8 * ishift and wv.data_ptr() % 16 == 4 * wshift
                    seen.add((iv.data_ptr() % 16, wv.data_ptr() % 16))
                    sides = [_side(stores[K, prefix][1], K, flat, base, B, iv, n if slack else -1, wv),
                             _side(stores["plain"][1], 2, flat, base + 1, B, pv, n_plain if slack else -1)]      # one weighted, one not
                    ops.bag_store_gather([], sides, B, order, off if use_order else 0)
                    what = (prefix, use_order, ishift, wshift)
                    assert torch.equal(sides[0].dense_out.cpu(), rd) and torch.equal(sides[0].lengths_out.cpu(), rl), what
                    assert torch.equal(iv[:n].cpu(), ri), what
                    assert torch.equal(RW.bits(wv[:n]).cpu(), RW.bits(rw)), what
                    assert _untouched(ibuf, GUARD + ishift, GUARD + ishift + n, SENT), what            # [total, capacity) and the guards
                    assert _untouched(wbuf, GUARD + wshift, GUARD + wshift + n, WSENT), what
                    assert torch.equal(sides[1].dense_out.cpu(), pd) and torch.equal(sides[1].lengths_out.cpu(), pl), what
                    assert torch.equal(pv[:n_plain].cpu(), pi) and _untouched(pbuf, GUARD + (ishift ^ 1), GUARD + (ishift ^ 1) + n_plain, SENT), what
    assert len(seen) == 8                                 # ids_out 0 / 8 mod 16 x weights_out 0 / 4 / 8 / 12 mod 16
    _L.check_device_errors(dev)                           # clean


def test_a_tile_of_empty_samples_between_two_full_ones(tt, stores):
    dev, B, K, prefix = torch.device(DEV), 513, 3, 1
    host, on_dev = stores[K, prefix]
    e = _entities(B, 5, tile_edge=True)
    rd, rl, ri, rw = RW.gather(*host, K, e)
    assert int(rl.view(B, K)[256:512].sum()) == 0 and int(rl.view(B, K)[:256].sum()) > 256 and int(rl.view(B, K)[512].sum()) == 3000
    n = ri.numel()
    _L.check_device_errors(dev)
    for ishift, wshift in ((0, 0), (1, 1), (0, 3), (1, 2)):
        ibuf, iv = _view(n, ishift, torch.int64, SENT)
        wbuf, wv = _view(n, wshift, torch.float32, WSENT)
        side = _side(on_dev, K, torch.stack([e, e], 1).to(DEV).view(-1), 0, B, iv, n, wv)
        ops.bag_store_gather([], [side], B)
        assert torch.equal(side.lengths_out.cpu(), rl) and torch.equal(side.dense_out.cpu(), rd)
        assert torch.equal(iv.cpu(), ri) and torch.equal(RW.bits(wv).cpu(), RW.bits(rw))
        assert _untouched(ibuf, GUARD + ishift, GUARD + ishift + n, SENT) and _untouched(wbuf, GUARD + wshift, GUARD + wshift + n, WSENT)
    _L.check_device_errors(dev)


@pytest.mark.parametrize("why", ["over-capacity", "expect"])
def test_a_refused_side_gets_neither_ids_nor_weights(tt, stores, references, why):
    """The device-side refusal: a bounded, designed outcome signalled through the error word.  capacity = total - 1, or expect =
    total + 1: the id and weight buffers are wholly untouched, lengths and dense rows are written, TT_DEVERR_BAG_OFFSETS once."""
    dev, B, K, prefix = torch.device(DEV), 257, 3, 3
    ents, (rd, rl, ri, rw), (pd, pl, pi) = references[B, K, prefix]
    n, n_plain = ri.numel(), pi.numel()
    cap, expect = (n - 1, -1) if why == "over-capacity" else (n + 9, n + 1)
    pairs, order, off = _pair_list(ents, True, 3)
    ibuf, iv = _view(cap, 1, torch.int64, SENT)
    wbuf, wv = _view(cap, 1, torch.float32, WSENT)
    pbuf, pv = _view(n_plain, 0, torch.int64, SENT)
    _L.check_device_errors(dev)
    sides = [_side(stores[K, prefix][1], K, pairs.view(-1), 0, B, iv, expect, wv), _side(stores["plain"][1], 2, pairs.view(-1), 1, B, pv, n_plain)]
    ops.bag_store_gather([], sides, B, order, off)
    torch.cuda.synchronize()
    assert _untouched(ibuf, 0, 0, SENT) and _untouched(wbuf, 0, 0, WSENT)       # no id, no weight, nothing beside them
    assert torch.equal(pv.cpu(), pi)                                            # the other side of the call is served
    assert torch.equal(sides[0].dense_out.cpu(), rd) and torch.equal(sides[0].lengths_out.cpu(), rl)
    assert torch.equal(sides[1].dense_out.cpu(), pd) and torch.equal(sides[1].lengths_out.cpu(), pl)
    with pytest.raises(_L.TwoTowerHipError, match=ERR):
        _L.check_device_errors(dev)
    _L.check_device_errors(dev)                                                 # once: clean after


def test_special_values_arrive_with_their_bits(tt, stores):
    dev, B, K, prefix = torch.device(DEV), 256, 1, 1
    (dense, offsets, values, _), on_dev = stores[K, prefix]
    special = np.array([0x7FC00000, 0x7FC01234, 0xFFC00001, 0x7F800001, 0xFFBFFFFF, 0x7F800000, 0xFF800000, 0x80000000, 0x00000000,
                        0x00000001, 0x807FFFFF, 0x00400000, 0x3F800000, 0xBF800000, 0x7F7FFFFF, 0x00800000], dtype=np.uint32)
    patt = np.random.default_rng(4).integers(0, 2 ** 32, values.numel(), dtype=np.uint64).astype(np.uint32)
    patt[:values.numel() // 2] = special[np.arange(values.numel() // 2) % len(special)]
    patt[patt == WSENT] = 0
    w = torch.from_numpy(patt.view(np.int32).copy()).view(torch.float32)
    e = _entities(B, 9)
    rd, rl, ri, rw = RW.gather(dense, offsets, values, w, K, e)
    n = ri.numel()
    got_bits = set(RW.bits(rw).numpy().view(np.uint32).tolist())
    assert set(special.tolist()) <= got_bits and bool(torch.isnan(rw).any()) and n > 3000
    _L.check_device_errors(dev)
    for wshift in (0, 1, 2, 3):
        wbuf, wv = _view(n, wshift, torch.float32, WSENT)
        ids = torch.empty(n, dtype=torch.int64, device=DEV)
        side = _side(on_dev[:3] + (w.to(DEV),), K, torch.stack([e, e], 1).to(DEV).view(-1), 0, B, ids, n, wv)
        ops.bag_store_gather([], [side], B)
        assert torch.equal(RW.bits(wv).cpu(), RW.bits(rw)) and torch.equal(ids.cpu(), ri)
        assert _untouched(wbuf, GUARD + wshift, GUARD + wshift + n, WSENT)
    _L.check_device_errors(dev)


def _raw_gather_w(sides, B):
    """tt_bag_store_gather_w called directly: the sides' weights as given, NULL included (ops.bag_store_gather takes the unweighted
    entry when no side has weights)"""
    dev = torch.device(DEV)
    arr = (_L.BagStoreSideW * len(sides))()
    for i, t in enumerate(sides):
        Ns, dd = t.dense_store.shape
        arr[i] = _L.BagStoreSideW(_L.ptr(t.entity), t.entity_stride, _L.ptr(t.dense_store), _L.ptr(t.offsets), _L.ptr(t.values), _L.ptr(t.dense_out),
                                  _L.ptr(t.lengths_out), _L.ptr(t.ids_out), t.values.numel(), t.ids_out.numel(), int(t.expect), dd, Ns, t.K, 0,
                                  _L.ptr(t.weights), _L.ptr(t.weights_out))
    lib = _L.load()
    ws = _L.workspace(dev, lib.tt_bag_store_gather_workspace_bytes(B, len(sides)))
    return lib.tt_bag_store_gather_w(_L.ctx(dev), 0, None, None, None, arr, len(sides), B, _L.vp(0), _L.ptr(ws), ws.numel(), _L.stream(dev))


@pytest.mark.parametrize("B", [257, 513])
def test_the_unweighted_entry_gives_the_same_ids(tt, stores, references, B):
    dev, K, prefix = torch.device(DEV), 3, 1
    ents, (rd, rl, ri, rw), _ = references[B, K, prefix]
    n = ri.numel()
    flat = torch.stack([ents[0], ents[0]], 1).to(DEV).view(-1)
    _L.check_device_errors(dev)
    got = {}
    for form in ("weighted", "unweighted", "raw-null"):
        ibuf, iv = _view(n + 5, 1, torch.int64, SENT)
        wbuf, wv = _view(n + 5, 1, torch.float32, WSENT)
        side = _side(stores[K, prefix][1], K, flat, 0, B, iv, n, wv, weighted=form == "weighted")
        if form == "raw-null":
            assert side.weights is None and _raw_gather_w([side], B) == 0
        else:
            ops.bag_store_gather([], [side], B)
        got[form] = (side.dense_out.cpu(), side.lengths_out.cpu(), ibuf.cpu())
        assert _untouched(wbuf, GUARD + 1, GUARD + 1 + (n if form == "weighted" else 0), WSENT), form       # ids alone: no weight is written
    for form in ("unweighted", "raw-null"):
        for a, b in zip(got["weighted"], got[form]):
            assert torch.equal(a, b), form
    assert torch.equal(got["weighted"][2][GUARD + 1:GUARD + 1 + n], ri) and torch.equal(got["weighted"][1], rl)
    # the entry's own argument check, before any launch: weights without weights_out, and the reverse
    ibuf, iv = _view(n, 0, torch.int64, SENT)
    wbuf, wv = _view(n, 0, torch.float32, WSENT)
    side = _side(stores[K, prefix][1], K, flat, 0, B, iv, n, wv)
    for w, wo in ((side.weights, None), (None, side.weights_out)):
        side.weights, side.weights_out = w, wo
        assert _raw_gather_w([side], B) != 0
    torch.cuda.synchronize()
    assert _untouched(ibuf, 0, 0, SENT) and _untouched(wbuf, 0, 0, WSENT) and bool(torch.isnan(side.dense_out).all())
    _L.check_device_errors(dev)


@pytest.mark.parametrize("B", [1, 4])
def test_a_batch_of_only_empty_entities(tt, stores, B):
    """A batch without a single id -- one empty entity, a catalogue chunk of empty ones: values() and weights() are empty tensors
    (a NULL weights_out beside a NULL ids_out at capacity 0), a weighted store serves it as the weightless one does, nothing is
    refused; with room in the buffers nothing is written into them."""
    from jodalrob_twotower_amd.data_loader import DeviceBagFeatureStore
    dev, K, prefix = torch.device(DEV), 3, 1
    (dense, offsets, values, weights), on_dev = stores[K, prefix]
    d = {"dense_projected": dense, "categorical_offsets": offsets - prefix, "categorical_values": values[prefix:]}
    weighted = DeviceBagFeatureStore(dict(d, categorical_weights=weights[prefix:]), list("abc"), DEV)
    bare = DeviceBagFeatureStore(d, list("abc"), DEV)
    e = torch.tensor(EMPTY[:B])
    assert int(weighted.run_lengths[e.to(DEV)].sum()) == 0 and weighted.weights.numel() == weighted.values.numel() > 3000
    _L.check_device_errors(dev)
    for st in (weighted, bare):
        for n_ids in (None, 0):
            got = st.gather(e.to(DEV), n_ids)
            k = got["kjt"]
            assert torch.equal(got["dense"].cpu(), dense[e]) and torch.equal(k.lengths().cpu(), torch.zeros(B * K, dtype=torch.int64))
            assert k.values().shape == (0,) and k.values().dtype == torch.int64
            if st is weighted:
                assert k.weights().shape == (0,) and k.weights().dtype == torch.float32
            else:
                assert k.weights_or_none() is None
    flat = torch.stack([e, e], 1).to(DEV).view(-1)
    for cap in (0, 5):                                    # through ops: capacity 0 (empty views), and room nobody uses
        ibuf, iv = _view(cap, 1, torch.int64, SENT)
        wbuf, wv = _view(cap, 3, torch.float32, WSENT)
        side = _side(on_dev, K, flat, 0, B, iv, 0, wv)
        ops.bag_store_gather([], [side], B)
        assert torch.equal(side.dense_out.cpu(), dense[e]) and not bool(side.lengths_out.any())
        assert _untouched(ibuf, 0, 0, SENT) and _untouched(wbuf, 0, 0, WSENT)
    # the entry itself: weights without weights_out is fine where capacity == 0 (as ids_out == NULL is) and refused where it is not
    side = _side(on_dev, K, flat, 0, B, torch.empty(0, dtype=torch.int64, device=DEV), 0, torch.empty(0, device=DEV))
    assert side.weights_out.data_ptr() == 0 and side.weights.data_ptr() != 0 and _raw_gather_w([side], B) == 0
    assert torch.equal(side.dense_out.cpu(), dense[e]) and not bool(side.lengths_out.any())
    torch.cuda.synchronize()
    _L.check_device_errors(dev)


@pytest.mark.parametrize("mode", ["mean", "sum"])
def test_store_gather_returns_a_weighted_kjt_the_embedder_pools(tt, manifest, mode):
    """DeviceBagFeatureStore.gather on a weighted store: weights() beside values(), and a bag-mode embedder pools the result to the
    bits of the same KJT built on the host by build_bag_kjt(..., weights=)."""
    from conftest import GOLD
    from jodalrob_twotower_amd.cat_embed import CategoricalEmbedder
    from jodalrob_twotower_amd.data_loader import DeviceBagFeatureStore
    dev = torch.device(DEV)
    cfg = manifest["cases"]["wide_b40"]
    keys, vocabs = cfg["keys_c"], cfg["vocab_c"]
    K = len(keys)
    rng = np.random.default_rng(21)
    bags = [[[int(i) for i in rng.integers(-1, vocabs[k] + 1, 0 if e in EMPTY else int(rng.choice([0, 1, 2, 7])))] for k in range(K)] for e in range(N)]
    weights = [[[float(np.float32(w)) for w in rng.uniform(-2, 2, len(bag))] for bag in row] for row in bags]
    dense = rng.standard_normal((N, DIN)).astype(np.float32)
    st = DeviceBagFeatureStore.from_bags(dense, bags, keys, DEV, weights=weights)
    unweighted = DeviceBagFeatureStore.from_bags(dense, bags, keys, DEV)
    e = _entities(300, 2).clamp(0, N - 1)
    rd, rl, ri, rw = RW.gather(st.dense.cpu(), st.offsets.cpu(), st.values.cpu(), st.weights.cpu(), K, e)
    _L.check_device_errors(dev)
    for n_ids in (None, ri.numel()):
        got = st.gather(e.to(DEV), n_ids)
        k = got["kjt"]
        assert torch.equal(got["dense"].cpu(), rd) and torch.equal(k.lengths().cpu(), rl) and torch.equal(k.values().cpu(), ri)
        assert k.weights().dtype == torch.float32 and torch.equal(RW.bits(k.weights()).cpu(), RW.bits(rw)) and k.keys() == keys
    plain = unweighted.gather(e.to(DEV))["kjt"]                                 # a weightless store: today's call and result
    assert plain.weights_or_none() is None and torch.equal(plain.values().cpu(), ri)
    host = tt.build_bag_kjt(keys, bags=[bags[i] for i in e.tolist()], weights=[weights[i] for i in e.tolist()], device=DEV)
    assert torch.equal(host.values().cpu(), ri) and torch.equal(RW.bits(host.weights()).cpu(), RW.bits(rw))
    emb = CategoricalEmbedder(keys, str(GOLD / "synthetic_metadata.csv"), "company", embedding_dim=cfg["E"], device=DEV, pooling=mode)
    with torch.no_grad():
        a, b, c = emb(k, return_dict=False), emb(host, return_dict=False), emb(plain, return_dict=False)
    assert torch.equal(a, b) and not torch.equal(a, c) and bool(torch.isfinite(a).all())
    _L.check_device_errors(dev)
