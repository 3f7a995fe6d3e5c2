"""tt_bag_store_gather on the MI355X, through ops.bag_store_gather alone: B entity indices of two sides -> dense rows, [B*K] lengths
and the samples' id runs packed behind one another, against the torch reference of tests/_bag_store_reference.py.  The gather moves
integers and copies f32, so every comparison is torch.equal.

Two stores of N = 97 entities, K = 5 and K = 2, one call with both sides.  Their bags hold: an entity with no ids at all, empty bags
at the first and the last key, one entity whose only bag has 3000 ids (one trip of one workgroup copies 2048), negative ids and ids
at or above 2^31; every batch names entity 0 and entity N - 1 (the store's last offset is read) and repeats entities.  Batch sizes
1, 63, 64, 300 and the scan tile + 3 (a second tile whose start is the first tile's total), each with `order` + offset and without
`order` at a non-zero offset into the interleaved [P, 2] pair list."""
import numpy as np
import pytest
import torch

import _bag_store_reference as R
from test_gpu_parity import DEV, tt  # noqa: F401

from jodalrob_twotower_amd import _lib as _L
from jodalrob_twotower_amd import ops

pytestmark = pytest.mark.gpu

N, LONG, NONE, EDGES = 97, 50, 3, 4            # entities; the one with the 3000-id bag, the one without ids, the one with empty end bags
SENT = -0x5A5A5A5A5A5A5A5A
SIZES = [1, 63, 64, 300, ops.BAG_STORE_TILE + 3]


def _ids(rng, n):
    """n ids: a fifth negative, the others small or at / above 2^31 (the store keeps them verbatim)"""
    u = rng.random(n)
    return [int(i) for i in np.where(u < 0.2, rng.integers(-5, 0, n), np.where(u < 0.6, rng.integers(0, 50, n), rng.integers(2 ** 31, 2 ** 33, n)))]


def _host_store(seed, K, din):
    rng = np.random.default_rng(seed)
    bags = []
    for e in range(N):
        row = [_ids(rng, int(rng.choice([0, 1, 1, 2, 3, 7]))) for _ in range(K)]
        if e == NONE:
            row = [[] for _ in range(K)]
        if e == EDGES:
            row[0], row[K - 1] = [], []
            if K > 2:
                row[1] = [7, -1, 2 ** 31]
        if e == LONG:
            row = [[] for _ in range(K)]
            row[K - 1] = _ids(rng, 3000)
        bags.append(row)
    lengths = np.array([len(b) for row in bags for b in row], dtype=np.int64)
    values = torch.tensor([i for row in bags for b in row for i in b], dtype=torch.int64)
    offsets = torch.from_numpy(np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64))
    dense = torch.from_numpy(rng.standard_normal((N, din)).astype(np.float32))
    assert int((values < 0).sum()) > 0 and int((values >= 2 ** 31).sum()) > 0
    return dense, offsets, values


@pytest.fixture(scope="module")
def stores():
    """[(K, host (dense, offsets, values), the same on the device)] of the two sides (din 8: the dense rows move in 16-byte pieces)"""
    out = []
    for seed, K, din in ((1, 5, 8), (2, 2, 8)):
        host = _host_store(seed, K, din)
        out.append((K, host, tuple(t.to(DEV) for t in host)))
    return out


def _entities(B, seed):
    rng = np.random.default_rng(seed)
    e = rng.integers(0, N, B)
    e[-1] = N - 1
    if B >= 8:
        e[:6] = [0, LONG, NONE, EDGES, e[7], e[7]]             # entity 0, the long bag, no ids, empty end bags, one entity three times
    return torch.from_numpy(e.astype(np.int64))


def _pair_list(ents, use_order, seed):
    """(pairs int64 [P, 2] on the device, order or None, offset): the batch is pairs[order[offset : offset + B]] / pairs[offset : offset + B]"""
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


def _sides(stores, pairs, order, off, B, ids_out, expect):
    flat = pairs.view(-1)
    base = 0 if order is not None else 2 * off
    sides, outs = [], []
    for i, (K, _, (dense, offsets, values)) in enumerate(stores):
        d = torch.full((B, dense.shape[1]), float("nan"), device=DEV)
        ln = torch.full((B * K,), SENT, dtype=torch.int64, device=DEV)
        sides.append(ops.BagStoreSide(flat[base + i:], 2, dense, offsets, values, K, d, ln, ids_out[i], expect[i]))
        outs.append((d, ln))
    return sides, outs


@pytest.fixture(scope="module")
def references(stores):
    """{(B, use_order): (entities per side, reference (dense, lengths, ids) per side)}, computed once on the host"""
    out = {}
    for B in SIZES:
        for use_order in (True, False):
            ents = [_entities(B, 100 * B + 10 * use_order + i) for i in range(2)]
            out[B, use_order] = (ents, [R.gather(*host, K, e) for (K, host, _), e in zip(stores, ents)])
    return out


@pytest.mark.parametrize("use_order", [True, False], ids=["order", "offset"])
@pytest.mark.parametrize("B", SIZES)
def test_gather_equals_the_reference(tt, stores, references, B, use_order):
    dev = torch.device(DEV)
    ents, refs = references[B, use_order]
    pairs, order, off = _pair_list(ents, use_order, B)
    n = [r[2].numel() for r in refs]
    if B >= 8:
        assert all(c > 3000 for c in n) and all(int((r[1] == 0).sum()) > 0 for r in refs)
    _L.check_device_errors(dev)
    scalars_src, scalars_dst = torch.arange(20, dtype=torch.float32, device=DEV), torch.zeros(20, device=DEV)
    # capacity == n, capacity == n + 17, and a destination at an odd element (8 mod 16): the narrow copy path
    for slack, shift in ((0, 0), (17, 0), (17, 1), (0, 1)):
        bufs = [torch.full((c + slack + 64 + shift,), SENT, dtype=torch.int64, device=DEV) for c in n]
        ids_out = [b[shift:shift + c + slack] for b, c in zip(bufs, n)]
        assert all(v.data_ptr() % 16 == 8 * shift for v in ids_out)
        sides, outs = _sides(stores, pairs, order, off, B, ids_out, n if slack else [-1, -1])
        scalars_dst.zero_()
        ops.bag_store_gather([(scalars_dst, scalars_src)], sides, B, order, off if order is not None else 0)
        for (d, ln), buf, (rd, rl, ri), c in zip(outs, bufs, refs, n):
            assert torch.equal(d.cpu(), rd) and torch.equal(ln.cpu(), rl)
            got = buf.cpu()
            assert torch.equal(got[shift:shift + c], ri), (slack, shift)
            assert bool((got[:shift] == SENT).all()) and bool((got[shift + c:] == SENT).all())      # nothing beside the batch's ids
        assert torch.equal(scalars_dst, scalars_src)
    _L.check_device_errors(dev)                                                 # clean


def test_store_gather_through_the_store(tt, stores, references):
    """DeviceBagFeatureStore.gather: the same wire format, with the id count given and read back"""
    from jodalrob_twotower_amd.data_loader import DeviceBagFeatureStore
    dev = torch.device(DEV)
    K, host, _ = stores[0]
    st = DeviceBagFeatureStore({"dense_projected": host[0], "categorical_offsets": host[1], "categorical_values": host[2]}, list("abcde"), DEV)
    ents, refs = references[300, True]
    rd, rl, ri = refs[0]
    for n_ids in (None, ri.numel()):
        got = st.gather(ents[0].to(DEV), n_ids)
        assert torch.equal(got["dense"].cpu(), rd) and torch.equal(got["kjt"].lengths().cpu(), rl) and torch.equal(got["kjt"].values().cpu(), ri)
        assert got["kjt"].keys() == list("abcde")
    assert torch.equal(st.run_lengths.cpu(), host[1][K::K] - host[1][:-1:K])
    # six dense features: no 16-byte pieces, the rows move float by float
    narrow = DeviceBagFeatureStore({"dense_projected": host[0][:, :6], "categorical_offsets": host[1], "categorical_values": host[2]}, list("abcde"), DEV)
    got = narrow.gather(ents[0].to(DEV), ri.numel())
    assert torch.equal(got["dense"].cpu(), rd[:, :6]) and torch.equal(got["kjt"].values().cpu(), ri)
    _L.check_device_errors(dev)


@pytest.mark.parametrize("why", ["over-capacity", "expect"])
def test_a_total_that_does_not_fit_writes_no_id(tt, stores, references, why):
    """The device-side refusal: a bounded, designed outcome signalled through the error word.  The total is above the capacity (or is
    not the count the host believes): nothing at or beyond ids_out[capacity] is written, no id is written at all, lengths and dense
    rows are, and check_device_errors reports TT_DEVERR_BAG_OFFSETS once."""
    dev = torch.device(DEV)
    B = ops.BAG_STORE_TILE + 3
    ents, refs = references[B, True]
    pairs, order, off = _pair_list(ents, True, B)
    n = [r[2].numel() for r in refs]
    cap = [n[0] - 5, n[1] + 9] if why == "over-capacity" else [n[0] + 9, n[1] + 9]
    expect = [-1, -1] if why == "over-capacity" else [n[0] + 1, n[1]]           # side 0 is refused, side 1 is fine
    bufs = [torch.full((c + 64,), SENT, dtype=torch.int64, device=DEV) for c in cap]
    _L.check_device_errors(dev)
    sides, outs = _sides(stores, pairs, order, off, B, [b[:c] for b, c in zip(bufs, cap)], expect)
    ops.bag_store_gather([], sides, B, order, off)
    torch.cuda.synchronize()
    assert bool((bufs[0] == SENT).all())                                        # no id, and nothing at or beyond the capacity
    assert torch.equal(bufs[1][:n[1]].cpu(), refs[1][2]) and bool((bufs[1][n[1]:] == SENT).all())
    for (d, ln), (rd, rl, _) in zip(outs, refs):
        assert torch.equal(d.cpu(), rd) and torch.equal(ln.cpu(), rl)           # lengths and dense rows are written all the same
    with pytest.raises(_L.TwoTowerHipError, match=r"status -5\).*device error word 0x8:.*bag offsets"):
        _L.check_device_errors(dev)
    _L.check_device_errors(dev)                                                 # once: clean after
