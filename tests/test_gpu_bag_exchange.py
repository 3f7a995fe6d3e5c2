"""Pooled multi-valued features across the row-wise sharded exchange, on the GPU.

(a) ops.embed_bag_rows (tt_embed_bag_rows[_w], the rows-only instantiation of the pooled lookup's kernel) against
    ops.embed_bag_lookup(want_rows=True) on the same sides: rows, bag_of, pos_w, inv_len, offsets bit for bit; the device error words.
(b) PaddedRowExchange.forward_bags / backward with the REAL HIP steps for G = 2 and 3 virtual ranks (threads on one GPU,
    test_gpu_parity._ThreadComm): pooled blocks == ops.embed_bag_lookup on the unsharded table, bit for bit; owners' row sums == the f64
    reference bit for bit on exact data (power-of-two lengths on mean keys, weights in {0.5, 1, 2}: every sum is exact in f32, so
    neither the rank order nor the split into per-rank sums can matter) and norm-wise under RANDN_NORM_BOUND on random normal data;
    a capacity that is too small raises the flag and pools ZERO rows, never another row.
(c) the sharded bag-mode training step at RCCL world 1, in a subprocess (tests/_bag_dist_world1_worker.py).
"""
import threading

import numpy as np
import pytest
import torch

import _bag_weight_reference as RW
import oracle_np as O
from test_gpu_embed_bag import RANDN_NORM_BOUND
from test_gpu_parity import DEV, _ThreadComm, tt  # noqa: F401  (tt: the module fixture)

from jodalrob_twotower_amd import _lib as _L

pytestmark = pytest.mark.gpu

B = 37
VOCABS = [[50, 300, 120, 9], [200, 75]]            # two sides, K = 4 and 2
POOLING = [["mean", "sum", "mean", "sum"], ["sum", "mean"]]
R_ROWS = sum(map(sum, VOCABS))


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).numpy()


def _desc(seed, weighted, pow2=False, exact_w=False, plain_second=False, trailing=3):
    """numpy description of one rank's two sides: per side (ids, lengths, key offsets, vocab, pooling, weights or None)"""
    rng = np.random.default_rng(seed)
    out, base = [], 0
    for si, v in enumerate(VOCABS):
        K = len(v)
        off = (np.concatenate([[0], np.cumsum(v)[:-1]]) + base).astype(np.int64)
        base += sum(v)
        if plain_second and si == 1:
            ids = np.stack([rng.integers(-2, vk + 2, B) for vk in v], axis=1).astype(np.int64).reshape(-1)
            out.append((ids, np.ones(B * K, np.int64), off, v, ["sum"] * K, None))
            continue
        lengths = rng.choice([0, 1, 2, 4, 8] if pow2 else np.arange(12), B * K).astype(np.int64)
        lengths[rng.integers(0, B * K, 3)] = 0                                           # empty bags for certain
        ids = np.concatenate([rng.integers(-2, v[s % K] + 2, int(n)) for s, n in enumerate(lengths)] +
                             [rng.integers(0, 5, trailing if si == 0 else 0)]).astype(np.int64)      # ids behind the last bag
        w = None
        if weighted and si == 0:                                                         # one weighted side beside an unweighted one
            w = (rng.choice([0.5, 1.0, 2.0], ids.size) if exact_w else rng.uniform(0.5, 1.5, ids.size)).astype(np.float32)
        out.append((ids, lengths, off, v, POOLING[si], w))
    return out


def _sides(ops, desc, E, out_dtype=torch.float32, h0=8):
    """ops.BagSide per side; outputs are column-offset views into wider NaN-filled buffers, as the towers' x"""
    sides, bufs = [], []
    for ids, lengths, off, v, pooling, w in desc:
        K = len(v)
        buf = torch.full((B, h0 + K * E + 4), float("nan"), dtype=out_dtype, device=DEV)
        pool = torch.tensor([ops.POOL_MODES[p] for p in pooling], dtype=torch.int32, device=DEV)
        sides.append(ops.BagSide(torch.from_numpy(ids).to(DEV), torch.from_numpy(lengths).to(DEV), torch.from_numpy(off).to(DEV),
                                 torch.tensor(v, dtype=torch.int64, device=DEV), pool, buf[:, h0:h0 + K * E], K,
                                 any(p == "mean" for p in pooling), weights=None if w is None else torch.from_numpy(w).to(DEV)))
        bufs.append(buf)
    return sides, bufs


# ------------------------------------------------------------------------------------------------ (a) the rows-only form
@pytest.mark.parametrize("E", [4, 32])
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
def test_embed_bag_rows_equals_the_lookups_index_arrays(tt, E, weighted):
    from jodalrob_twotower_amd import ops
    lib = _L.load()
    desc = _desc(70 + E, weighted)
    assert any((d[1] == 0).any() for d in desc) and any(d[1].max() == 11 for d in desc) and desc[0][0].size > desc[0][1].sum()
    assert any((d[0] < 0).any() and (d[0] > max(d[3])).any() for d in desc)
    table = torch.from_numpy(np.random.default_rng(1).standard_normal((R_ROWS, E)).astype(np.float32)).to(DEV)
    sides, _ = _sides(ops, desc, E)
    ref = ops.embed_bag_lookup(table, sides, B, want_rows=True)
    sides2, bufs2 = _sides(ops, desc, E)
    torch.cuda.synchronize()
    n0 = lib.tt_launch_count()
    got = ops.embed_bag_rows(sides2, B, R_ROWS)
    torch.cuda.synchronize()
    assert lib.tt_launch_count() - n0 == 1                                               # one launch
    assert all(torch.isnan(b).all() for b in bufs2)                                      # no pooled output is written
    assert got.nnz == ref.nnz and got.side_nnz == ref.side_nnz and got.pad_row is None
    assert np.array_equal(_bits(got.rows), _bits(ref.rows)) and np.array_equal(_bits(got.bag_of), _bits(ref.bag_of))
    assert (ref.bag_of.cpu().numpy() < 0).sum() == 3 and np.array_equal(_bits(got.inv_len), _bits(ref.inv_len))
    assert len(got.offsets) == len(ref.offsets) and all(torch.equal(a, b) for a, b in zip(got.offsets, ref.offsets))
    if weighted:
        covered = ref.bag_of.cpu().numpy() >= 0                                          # (w_out is not written where no bag covers)
        assert np.array_equal(_bits(got.pos_w)[covered], _bits(ref.pos_w)[covered])
    else:
        assert got.pos_w is None and ref.pos_w is None
    got_noout = ops.embed_bag_rows([ops.BagSide(**{**s.__dict__, "out": None}) for s in sides2], B, R_ROWS)      # no output at all
    assert torch.equal(got_noout.rows, ref.rows) and torch.equal(got_noout.bag_of, ref.bag_of)
    with pytest.raises(ValueError, match="position-weight source"):
        pw = ops.BagPosWeights(torch.ones(4, device=DEV), torch.zeros(4, dtype=torch.int32, device=DEV), torch.ones(4, dtype=torch.int32, device=DEV))
        ops.embed_bag_rows([ops.BagSide(**{**sides2[0].__dict__, "weights": None, "pos_weights": pw})], B, R_ROWS)


@pytest.mark.parametrize("how", ["decreasing", "beyond-nnz", "row-range"])
def test_embed_bag_rows_raises_the_device_error_words(tt, how):
    """A refused offset pair raises TT_DEVERR_BAG_OFFSETS and counts as an empty bag; a row beyond table_rows raises
    TT_DEVERR_ROW_RANGE and is stored as the last row -- the words and the arrays of the lookup itself."""
    from jodalrob_twotower_amd import ops
    dev = torch.device(DEV)
    E = 32
    desc = _desc(90, False)
    rows_limit = R_ROWS
    if how == "decreasing":
        desc[0][1][40] = -2
    elif how == "beyond-nnz":
        desc[0][1][-1] += 1000
    else:
        rows_limit = R_ROWS - 60                                                         # side 1's last key reaches beyond the table
    table = torch.from_numpy(np.random.default_rng(1).standard_normal((rows_limit, E)).astype(np.float32)).to(DEV)
    _L.check_device_errors(dev)
    sides, _ = _sides(ops, desc, E)
    ref = ops.embed_bag_lookup(table, sides, B, want_rows=True)
    word = r"0x2:" if how == "row-range" else r"0x8:.*bag offsets"
    with pytest.raises(_L.TwoTowerHipError, match=r"status -5\).*device error word " + word):
        _L.check_device_errors(dev)
    got = ops.embed_bag_rows(sides, B, rows_limit)
    with pytest.raises(_L.TwoTowerHipError, match=r"status -5\).*device error word " + word):
        _L.check_device_errors(dev)
    assert torch.equal(got.rows, ref.rows) and torch.equal(got.bag_of, ref.bag_of)
    if how == "row-range":
        assert int(got.rows.max()) == rows_limit - 1
    _L.check_device_errors(dev)


# ------------------------------------------------------------------------------------------------ (b) G virtual ranks on one GPU
class _TurnComm(_ThreadComm):
    """_ThreadComm for virtual ranks that all work on the DEFAULT stream, one at a time: a rank holds `turn` while it launches and
    gives it up only inside a collective, after its launches have finished (the base class synchronises first).  A stream of its own
    per rank would cost a slice of the library's plan-chain pool (16 slices, one per stream it has seen, never handed back) in every
    test, and the tests that run after this file count their launches."""

    def __init__(self, world, rank, shared, turn):
        super().__init__(world, rank, shared)
        self.turn = turn

    def _exchange(self, t):
        torch.cuda.current_stream().synchronize()
        self.turn.release()
        try:
            return super()._exchange(t)
        finally:
            self.turn.acquire()


def _run_ranks(G, E, rank_fn, capacity=None):
    from jodalrob_twotower_amd.distributed import PaddedRowExchange, ShardedStore
    table = torch.from_numpy(np.random.default_rng(11).standard_normal((R_ROWS, E)).astype(np.float32))
    shared = {"slots": [None] * G, "bar": threading.Barrier(G)}
    results, errors = [None] * G, []
    turn = threading.Lock()

    def run(rank):
        try:
            with turn:
                store = ShardedStore(E, R_ROWS, rank, G, DEV, "sparse")
                store.load_global(table)
                ex = PaddedRowExchange(store, comm=_TurnComm(G, rank, shared, turn), capacity=capacity)
                results[rank] = rank_fn(rank, ex, store, table)
                torch.cuda.current_stream().synchronize()
        except Exception:                                       # pragma: no cover
            import traceback
            errors.append(traceback.format_exc())
            shared["bar"].abort()

    threads = [threading.Thread(target=run, args=(r,)) for r in range(G)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    assert not errors, errors[0]
    return results, table


@pytest.mark.parametrize("G,x_dtype,weighted,plain_second", [(2, torch.float32, False, False), (3, torch.float32, True, True),
                                                             (3, torch.bfloat16, False, True), (2, torch.bfloat16, True, False)])
def test_padded_bag_exchange_forward_equals_the_unsharded_lookup(tt, G, x_dtype, weighted, plain_second):
    from jodalrob_twotower_amd import ops
    E = 32

    def rank_fn(rank, ex, store, table):
        desc = _desc(500 + rank, weighted, plain_second=plain_second)
        sides, bufs = _sides(ops, desc, E, x_dtype)
        ref_sides, ref_bufs = _sides(ops, desc, E, x_dtype)
        ops.embed_bag_lookup(table.to(DEV), ref_sides, B, want_rows=False)
        assert ex.forward_bags(sides, B, False) is None
        same = all(np.array_equal(_bits(s.out), _bits(r.out)) for s, r in zip(sides, ref_sides))
        pad_ok = all(bool(torch.isnan(b[:, :8].float()).all()) and bool(torch.isnan(b[:, -4:].float()).all()) for b in bufs)
        return dict(same=same, pad_ok=pad_ok, overflow=ex.overflowed(), C=ex.C, buf_dtype=ex._place_buf.dtype)

    results, _ = _run_ranks(G, E, rank_fn)
    for r in results:
        assert r["same"] and r["pad_ok"] and not r["overflow"] and r["C"] >= 256
        assert r["buf_dtype"] == torch.float32                   # pooled rows travel as f32 whatever the tower input dtype is


def _backward(G, E, exact, src_dtype=torch.float32):
    """owners' summed rows (dense [R, E] f32, assembled from every rank's sparse gradient) and the f64 reference"""
    from jodalrob_twotower_amd import ops

    def rank_fn(rank, ex, store, table):
        desc = _desc(700 + rank, True, pow2=exact, exact_w=exact)
        sides, _ = _sides(ops, desc, E)
        state = ex.forward_bags(sides, B, True)
        rng = np.random.default_rng(900 + rank)
        srcs, rows, vals = [], [], []
        inv = state["bag"].inv_len.cpu().numpy()
        base = 0
        for s, (ids, lengths, off, v, pooling, w) in zip(sides, desc):
            d = O.exact_grid_values(rng, (B, s.K * E + 4)) if exact else rng.standard_normal((B, s.K * E + 4)).astype(np.float32)
            t = torch.from_numpy(d).to(DEV).to(src_dtype)
            srcs.append((t[:, :s.K * E], s.K))
            rws, vls = RW.contributions(t[:, :s.K * E].float().cpu().numpy(), ids, lengths, off, v, pooling,
                                        np.ones(ids.size, np.float32) if w is None else w, inv_len=inv[base:base + B * s.K])
            rows.append(rws); vals.append(vls)
            base += B * s.K
        ex.backward(state, srcs, B)
        plan, grad_rows = store.sparse_grad
        torch.cuda.current_stream().synchronize()
        U = int(plan.n_unique.item())
        return dict(rows=np.concatenate(rows), vals=np.concatenate(vals), uniq=plan.unique_rows[:U].cpu().numpy(),
                    grads=grad_rows[:U].cpu().numpy(), local_rows=store.local_rows, overflow=ex.overflowed())

    results, _ = _run_ranks(G, E, rank_fn)
    ref = np.zeros((R_ROWS, E), np.float64)
    mag = np.zeros((R_ROWS, E), np.float64)
    got = np.zeros((R_ROWS, E), np.float32)
    for r in results:
        assert not r["overflow"]
        np.add.at(ref, r["rows"], r["vals"])
        np.add.at(mag, r["rows"], np.abs(r["vals"]))
    for rank, r in enumerate(results):
        real = r["uniq"] < r["local_rows"]
        assert (~real).sum() <= 1                                  # the last distinct "row" is the bucket pad
        got[r["uniq"][real] * G + rank] = r["grads"][real]
        touched = np.flatnonzero(np.abs(ref[rank::G]).sum(1) > 0)
        assert set(touched.tolist()) <= set(r["uniq"][real].tolist())
    return got, ref, mag


@pytest.mark.parametrize("G", [2, 3])
@pytest.mark.parametrize("src_dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_padded_bag_exchange_backward_exact_grid(tt, G, src_dtype):
    got, ref, mag = _backward(G, 32, exact=True, src_dtype=src_dtype)
    assert O.exact_sum_precondition(mag)                           # every partial sum is exact in f32: no order can matter
    assert np.abs(ref).sum() > 0
    bad = got.astype(np.float64) != ref
    assert not bad.any(), (int(bad.any(1).sum()), "rows differ")


@pytest.mark.parametrize("G", [2, 3])
def test_padded_bag_exchange_backward_random_normal(tt, G):
    got, ref, _ = _backward(G, 32, exact=False)
    norm = float(np.linalg.norm(got.astype(np.float64) - ref) / np.linalg.norm(ref))
    print(f"\n[bag exchange bwd randn G={G}] norm-wise error {norm:.3e} (bound {RANDN_NORM_BOUND:.1e})")
    assert norm <= RANDN_NORM_BOUND, norm


@pytest.mark.parametrize("G", [2, 3])
def test_padded_bag_exchange_overflow_pools_zero_rows(tt, G):
    """capacity = 16: a bucket holds the 16 smallest distinct rows of its owner; the flag rises, check_overflow raises, and every
    position whose row did not fit pools the ZERO row -- the pooled blocks are the unsharded lookup's on a table whose rows that
    did not fit are zeroed, bit for bit (adding a zero row changes no bits of a sum)."""
    from jodalrob_twotower_amd import ops
    from jodalrob_twotower_amd.distributed import ExchangeOverflowError
    E, C = 32, 16

    def rank_fn(rank, ex, store, table):
        desc = _desc(500 + rank, True)
        sides, _ = _sides(ops, desc, E)
        ref_sides, _ = _sides(ops, desc, E)
        bag = ops.embed_bag_rows(sides, B, R_ROWS)
        distinct = np.unique(bag.rows.cpu().numpy())
        cut = table.clone()
        dropped = 0
        for g in range(G):
            mine = distinct[distinct % G == g]
            cut[torch.from_numpy(mine[C:].astype(np.int64))] = 0.0
            dropped += max(len(mine) - C, 0)
        ops.embed_bag_lookup(cut.to(DEV), ref_sides, B, want_rows=False)
        ex.forward_bags(sides, B, False)
        same = all(np.array_equal(_bits(s.out), _bits(r.out)) for s, r in zip(sides, ref_sides))
        raised = False
        try:
            ex.check_overflow()
        except ExchangeOverflowError:
            raised = True
        return dict(same=same, dropped=dropped, overflow=ex.overflowed(), raised=raised)

    results, _ = _run_ranks(G, E, rank_fn, capacity=C)
    for r in results:
        assert r["dropped"] > 0 and r["overflow"] and r["raised"] and r["same"]


# ------------------------------------------------------------------------------------------------ (c) RCCL world 1
def test_sharded_bag_step_world1_subprocess(tt):
    """The sharded bag-mode training step (exact and padded exchanges) against the unsharded bag-mode step: one GPU process with its
    own process group and the ordinary teardown; the return code must be 0."""
    import subprocess
    import sys
    from pathlib import Path
    worker = Path(__file__).resolve().parent / "_bag_dist_world1_worker.py"
    r = subprocess.run([sys.executable, str(worker)], capture_output=True, text=True, timeout=240)
    assert "BAG_DIST_WORLD1_OK" in r.stdout, (r.stdout.splitlines()[-4:], [ln for ln in r.stderr.splitlines() if "rror" in ln or "what()" in ln][-8:])
    assert r.returncode == 0, (r.returncode, r.stderr.splitlines()[-8:])
