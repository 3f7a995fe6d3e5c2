"""Learned position weights on the MI355X: tt_bag_position_weights_fwd / _bwd through ops, and a stand-alone embedder whose
KJT weights are a leaf that requires grad.

Forward: w[p] is a COPY of the parameter element position p reads (tests/_bag_weight_grad_reference.py: position_index) -- equal
bits, 1.0 for a key without position weights and for ids no bag covers.
Backward: element e sums the per-id gradient of the n_e positions that read it; whatever the order, every term passes through at
most n_e - 1 <= n_e roundings: |got - ref| <= gamma(n_e) * sum |g_P|.  Elements nobody reads are exactly 0; two runs: equal bits.
B = 67, K = 3, max_len {1, 4, 7}.
"""
import numpy as np
import pytest
import torch

import _bag_weight_grad_reference as G
import _bag_weight_reference as W
from conftest import GOLD
from test_gpu_embed_bag import U24
from test_gpu_embed_bag_capture import _cfg
from test_gpu_parity import DEV, tt  # noqa: F401  (tt: the module fixture)

from jodalrob_twotower_amd import _lib as _L

pytestmark = pytest.mark.gpu

B, K = 67, 3
# per key: (max_len, the lengths its bags are drawn from).  Key 0: max_len 1 -- every position reads the one element.  Key 1: bags
# longer than max_len 4 (and empty ones).  Key 2: no bag reaches position 3, so elements 3 .. 6 of its 7 are read by nobody.
KEYS = [(1, [0, 1, 2, 5]), (4, [0, 1, 3, 4, 5, 9, 12]), (7, [0, 1, 2, 3])]
TRAILING = 4


def gamma(k):
    ku = np.asarray(k, dtype=np.float64) * U24
    return ku / (1 - ku)


def _case(seed, without=None):
    """(lengths, pw_offset, pw_len, n_param, nnz); without: a key that gets pw_offset = -1"""
    rng = np.random.default_rng(seed)
    lengths = np.stack([rng.choice(ls, B) for _, ls in KEYS], axis=1).reshape(-1).astype(np.int64)
    off, ln, total = [], [], 0
    for k, (m, _) in enumerate(KEYS):
        off.append(-1 if k == without else total)
        ln.append(0 if k == without else m)
        total += 0 if k == without else m
    return rng, lengths, off, ln, total, int(lengths.sum()) + TRAILING


def _side(ops, lengths, off, ln, nnz):
    t = lambda a, dt: torch.from_numpy(np.asarray(a)).to(device=DEV, dtype=dt)
    return ops.PosWeightSide(t(lengths, torch.int64), t(off, torch.int32), t(ln, torch.int32), nnz, K)


@pytest.mark.parametrize("without", [None, 1], ids=["all-keys", "key1-without"])
def test_forward_is_the_indexed_parameter_and_backward_its_sum(tt, without):
    from jodalrob_twotower_amd import ops
    dev = torch.device(DEV)
    _L.check_device_errors(dev)
    rng, lengths, off, ln, n_param, nnz = _case(50 + (without or 0), without)
    assert n_param == (12 if without is None else 8) and (lengths == 0).any() and lengths.max() == 12
    param = rng.standard_normal(n_param).astype(np.float32)
    idx = G.position_index(lengths, K, off, ln)
    side = _side(ops, lengths, off, ln, nnz)
    pt = torch.from_numpy(param).to(DEV)
    (w,) = ops.bag_position_weights(pt, [side], B)
    want = np.concatenate([G.expand(param, idx), np.ones(TRAILING, np.float32)])    # ids behind the last bag weigh 1
    assert w.dtype == torch.float32 and w.shape == (nnz,)
    assert torch.equal(w.cpu(), torch.from_numpy(want))
    assert np.array_equal(w.cpu().numpy().view(np.uint32), want.view(np.uint32))
    if without is not None:
        key = np.repeat(np.arange(B * K) % K, lengths)
        assert (want[:idx.size][key == without] == 1).all() and (idx[key == without] == -1).all()
    # backward
    g = rng.standard_normal(nnz).astype(np.float32)
    gt = torch.from_numpy(g).to(DEV)
    d = ops.bag_position_weights_bwd(pt, [side], B, [gt])
    ref, mag, cnt = G.reduce(g, idx, n_param)
    got = d.cpu().numpy()
    assert got.shape == (n_param,) and got.dtype == np.float32
    err = np.abs(got.astype(np.float64) - ref)
    print(f"\n[position weights] contributions per element {cnt.tolist()}, max err / bound = "
          f"{float((err[cnt > 0] / (gamma(cnt) * mag)[cnt > 0]).max()):.3f}")
    assert (err <= gamma(cnt) * mag).all()
    assert cnt.max() > 100 and (cnt == 0).sum() >= 4                             # key 2's elements 3 .. 6
    assert not got[cnt == 0].any() and not np.signbit(got[cnt == 0]).any()       # exactly 0 where nobody reads
    d2 = ops.bag_position_weights_bwd(pt, [side], B, [gt])
    assert np.array_equal(got.view(np.uint32), d2.cpu().numpy().view(np.uint32))      # two runs: equal bits
    assert bool((ops.bag_position_weights_bwd(pt, [side], B, [None]) == 0).all())     # a side without a gradient contributes nothing
    torch.cuda.synchronize()
    _L.check_device_errors(dev)


def test_max_len_one_and_empty_bags(tt):
    """every key with max_len 1: each id of a key copies that key's one element, however long the bag; a batch of empty bags"""
    from jodalrob_twotower_amd import ops
    rng = np.random.default_rng(7)
    lengths = rng.choice([0, 1, 6], B * K).astype(np.int64)
    param = np.array([0.5, -2.0, 3.25], np.float32)
    side = _side(ops, lengths, [0, 1, 2], [1, 1, 1], int(lengths.sum()))
    pt = torch.from_numpy(param).to(DEV)
    (w,) = ops.bag_position_weights(pt, [side], B)
    key = np.repeat(np.arange(B * K) % K, lengths)
    assert torch.equal(w.cpu(), torch.from_numpy(param[key]))
    g = torch.ones(int(lengths.sum()), device=DEV)
    d = ops.bag_position_weights_bwd(pt, [side], B, [g]).cpu().numpy()
    assert d.tolist() == [float((key == k).sum()) for k in range(K)]             # small integers: exact
    empty = _side(ops, np.zeros(B * K, np.int64), [0, 1, 2], [1, 1, 1], 0)
    (w0,) = ops.bag_position_weights(pt, [empty], B)
    assert w0.numel() == 0
    assert bool((ops.bag_position_weights_bwd(pt, [empty], B, [w0]) == 0).all())
    _L.check_device_errors(torch.device(DEV))


def test_standalone_embedder_gives_leaf_weights_their_gradient(tt, manifest):
    """The schema and shapes of test_standalone_embedder_matches_f64_embedding_bag (tests/test_gpu_embed_bag_weights_step.py), the KJT's
    weights a leaf that requires grad: .grad within the ops-level bound gamma(E + 2) * |c| * sum |d x| of the float64 autograd
    gradient built here; the output and the table gradient keep that test's bounds."""
    from jodalrob_twotower_amd.cat_embed import CategoricalEmbedder
    cfg = _cfg(manifest)
    Bn = cfg["B"]
    keys, E = cfg["keys_n"], cfg["E"]
    Kn = len(keys)
    pooling = {keys[0]: "mean", keys[2]: "mean", keys[4]: "sum"}
    emb = CategoricalEmbedder(keys, str(GOLD / "synthetic_metadata.csv"), "notice", embedding_dim=E, device=DEV, embedding_grad="dense",
                              pooling=pooling)
    modes = emb.pooling
    vocabs = [emb.vocab_sizes[k] for k in keys]
    offs = emb._key_row_offset.cpu().numpy()
    rng = np.random.default_rng(14)
    lengths = rng.choice([0, 1, 2, 3, 5, 7, 11], Bn * Kn).astype(np.int64)
    ids = np.concatenate([rng.integers(-2, vocabs[s % Kn] + 2, int(n)) for s, n in enumerate(lengths)]).astype(np.int64)
    w = rng.standard_normal(ids.size).astype(np.float32)
    wt = torch.from_numpy(w).to(DEV).requires_grad_(True)
    kjt = tt.KeyedJaggedTensor(keys, torch.from_numpy(ids).to(DEV), torch.from_numpy(lengths).to(DEV), wt)
    assert kjt.weights() is wt
    g = rng.standard_normal((Bn, Kn * E)).astype(np.float32)
    out = emb(kjt, return_dict=False)
    (out * torch.from_numpy(g).to(DEV)).sum().backward()
    torch.cuda.synchronize()
    table = emb.store.weight.detach().cpu().numpy()
    # the float64 autograd reference: embedding_bag(per_sample_weights=) key by key, the weights a leaf
    starts = np.concatenate([[0], np.cumsum(lengths)])
    t64 = torch.from_numpy(table.astype(np.float64)).requires_grad_(True)
    w64 = torch.from_numpy(w.astype(np.float64)).requires_grad_(True)
    cols = []
    for k in range(Kn):
        sel = np.arange(Bn) * Kn + k
        pos = np.concatenate([np.arange(starts[s], starts[s + 1]) for s in sel]).astype(np.int64)
        rows = offs[k] + ids[pos].clip(0, vocabs[k] - 1)
        koff = np.concatenate([[0], np.cumsum(lengths[sel])[:-1]])
        eb = torch.nn.functional.embedding_bag(torch.from_numpy(rows), t64, torch.from_numpy(koff), mode="sum",
                                               per_sample_weights=w64[torch.from_numpy(pos)])
        if modes[k] == "mean":
            eb = eb / torch.from_numpy(np.maximum(lengths[sel], 1).astype(np.float64))[:, None]
        cols.append(eb)
    want = torch.cat(cols, dim=1)
    want.backward(torch.from_numpy(g.astype(np.float64)))
    # the output: that test's forward bound
    ref, mag, _, _ = W.weighted_forward(table, ids, lengths, offs, vocabs, modes, w)
    np.testing.assert_allclose(ref, want.detach().numpy(), rtol=1e-13, atol=1e-14)
    L = np.repeat(lengths.reshape(Bn, Kn), E, axis=1).astype(np.float64)
    assert (np.abs(out.detach().cpu().numpy().astype(np.float64) - ref) <= gamma(L + 1) * mag).all()
    # the weights' gradient.  The kernel multiplies by the f32 inv_len the lookup formed; the autograd reference divides by L
    # exactly: the reference over that inv_len is the one the bound is about, and autograd agrees with it up to the rounding of 1 / L
    inv = np.where(np.tile(np.array([m == "mean" for m in modes]), Bn) & (lengths > 0),
                   np.float32(1) / np.maximum(lengths, 1).astype(np.float32), np.float32(1))
    g64, scale = G.weight_grad(table, g, ids, lengths, offs, vocabs, modes, inv_len=inv)
    assert (np.abs(w64.grad.numpy() - g64) <= U24 * scale * (1 + 1e-6)).all()
    assert wt.grad is not None and wt.grad.shape == wt.shape and wt.grad.dtype == torch.float32
    err = np.abs(wt.grad.cpu().numpy().astype(np.float64) - g64)
    print(f"\n[embedder] weights.grad: max err / bound = {float((err / np.maximum(gamma(E + 2) * scale, 1e-300)).max()):.3f}")
    assert (err <= gamma(E + 2) * scale).all() and np.abs(g64).max() > 1
    # the table gradient: that test's backward bound
    uniq, sums, abs_sums, counts = W.weighted_backward(g, ids, lengths, offs, vocabs, modes, w, inv_len=inv)
    got = emb.store.grad.cpu().numpy()
    assert (np.abs(got[uniq].astype(np.float64) - sums) <= gamma(counts + 1)[:, None] * abs_sums).all()
    rest = np.ones(len(got), bool)
    rest[uniq] = False
    assert not got[rest].any()
    _L.check_device_errors(torch.device(DEV))


def test_standalone_embedder_with_position_weights(tt, manifest):
    """at 1.0 the pooled output is the unweighted embedder's, bit for bit; position_weight.grad is the reduction of the per-id
    gradient; a KJT with data weights is refused"""
    from jodalrob_twotower_amd import ops
    from jodalrob_twotower_amd.cat_embed import CategoricalEmbedder
    cfg = _cfg(manifest)
    Bn, keys, E = cfg["B"], cfg["keys_n"], cfg["E"]
    Kn = len(keys)
    mk = lambda: CategoricalEmbedder(keys, str(GOLD / "synthetic_metadata.csv"), "notice", embedding_dim=E, device=DEV, embedding_grad="dense",
                                     pooling={keys[0]: "mean"})
    plain, emb = mk(), mk().add_position_weights({keys[0]: 3, keys[3]: 2})
    emb.load_state_dict(plain.state_dict(), strict=False)
    assert emb.position_weight.device.type == "cuda" and emb._pw_offset.device.type == "cuda"
    vocabs = [emb.vocab_sizes[k] for k in keys]
    rng = np.random.default_rng(15)
    lengths = rng.choice([0, 1, 2, 3, 5, 7], Bn * Kn).astype(np.int64)
    ids = np.concatenate([rng.integers(0, vocabs[s % Kn], int(n)) for s, n in enumerate(lengths)]).astype(np.int64)
    kjt = tt.build_bag_kjt(keys, values=torch.from_numpy(ids), lengths=torch.from_numpy(lengths), device=DEV)
    g = torch.from_numpy(rng.standard_normal((Bn, Kn * E)).astype(np.float32)).to(DEV)
    out_p, out_w = plain(kjt, return_dict=False), emb(kjt, return_dict=False)
    assert torch.equal(out_p, out_w)
    (out_p * g).sum().backward()
    (out_w * g).sum().backward()
    torch.cuda.synchronize()
    assert torch.equal(plain.store.grad, emb.store.grad)                         # weights of 1.0: the unweighted table gradient
    # the parameter's gradient: the per-id gradient of a leaf of ones, reduced by the backward entry -- the same two launches
    leaf = torch.ones(ids.size, device=DEV, requires_grad=True)
    twin = mk()
    twin.load_state_dict(plain.state_dict())
    (twin(tt.KeyedJaggedTensor(keys, kjt.values(), kjt.lengths(), leaf), return_dict=False) * g).sum().backward()
    side = ops.PosWeightSide(kjt.lengths(), emb._pw_offset, emb._pw_len, ids.size, Kn)
    want = ops.bag_position_weights_bwd(emb.position_weight.detach(), [side], Bn, [leaf.grad])
    assert emb.position_weight.grad is not None and torch.equal(emb.position_weight.grad, want) and bool(want.abs().min() > 0)
    with pytest.raises(ValueError, match="one source of weights per embedder"):
        emb(tt.KeyedJaggedTensor(keys, kjt.values(), kjt.lengths(), leaf.detach()))
    _L.check_device_errors(torch.device(DEV))
