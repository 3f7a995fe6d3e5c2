"""gloo tests (CPU, worlds 2 and 3) of the POOLED routing of the row-wise sharded step -- RowExchange.forward_bags and
PaddedRowExchange.forward_bags -- with a checker backend (numpy pooling) in the place of the HIP steps, against
tests/_bag_reference.py / _bag_weight_reference.py on the unsharded table; the refusals of the sharded bag-mode task; and the
random-normal bar the GPU test of the same routing uses, pinned against f64.  No GPU."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import _bag_reference as R
import _bag_weight_reference as RW
from conftest import GOLD
from test_distributed_gloo import CheckerBackend, _free_port

RANDN_NORM_BOUND = 1.6e-6           # tests/test_gpu_embed_bag.py's bar (not imported here: that module needs a GPU session's fixtures)


class BagCheckerBackend(CheckerBackend):
    """CheckerBackend plus the pooled steps of HipBackend (bag_rows, pool_rows, collect_bag_grads, bag_local_plan,
    reduce_bags_into_buckets): the same contracts, plain numpy."""

    def bag_rows(self, sides, B, table_rows):
        from jodalrob_twotower_amd import ops
        rows, bag_of, inv, pos_w, offs, base = [], [], [], [], [], 0
        weighted = any(s.weights is not None for s in sides)
        for s in sides:
            assert s.pos_weights is None and s.capacity is None
            ln = s.lengths.numpy().reshape(-1)
            sl, r = R.positions(s.ids.numpy(), ln, s.key_row_offset.numpy(), s.key_vocab.numpy().tolist())
            n = s.ids.numel()
            rr, bb = np.zeros(n, np.int32), np.full(n, -1, np.int32)          # positions behind the last bag: (0, -1)
            rr[:sl.size], bb[:sl.size] = r, sl + base
            rows.append(rr); bag_of.append(bb)
            mean = np.tile(s.key_pool.numpy() != 0, B) & (ln > 0)
            inv.append(np.where(mean, np.float32(1) / np.maximum(ln, 1).astype(np.float32), np.float32(1)).astype(np.float32))
            pos_w.append(s.weights.numpy() if s.weights is not None else np.ones(n, np.float32))
            offs.append(torch.from_numpy(np.concatenate([[0], np.cumsum(ln)]).astype(np.int64)))
            base += B * s.K
        t = lambda a: torch.from_numpy(np.concatenate(a))
        nnz = sum(s.ids.numel() for s in sides)
        return ops.BagPlan(t(rows), t(bag_of), t(inv) if any(s.any_mean for s in sides) else None, nnz, None,
                           t(pos_w) if weighted else None, tuple(s.ids.numel() for s in sides), tuple(offs))

    def pool_rows(self, received, idx, sides, B):
        base, M = 0, received.shape[0]
        E = received.shape[1]
        for s in sides:
            n = s.ids.numel()
            pooling = ["mean" if p else "sum" for p in s.key_pool.tolist()]
            w = s.weights.numpy() if s.weights is not None else np.ones(n, np.float32)
            out, _, _, _ = RW.weighted_forward(received.numpy(), idx[base:base + n].numpy(), s.lengths.numpy(), np.zeros(s.K, np.int64),
                                               [M] * s.K, pooling, w)
            s.out.copy_(torch.from_numpy(out.astype(np.float32)).view(B, s.K * E))
            base += n

    def _contrib(self, srcs, bag, B, E):
        flat = torch.cat([d.reshape(B * K, E) for d, K in srcs]).numpy().astype(np.float64)
        slot = bag.bag_of.numpy()
        c = np.ones(bag.nnz) if bag.pos_w is None else bag.pos_w.numpy().astype(np.float64)
        if bag.inv_len is not None:
            c = c * bag.inv_len.numpy().astype(np.float64)[np.maximum(slot, 0)]
        return np.where(slot[:, None] >= 0, flat[np.maximum(slot, 0)] * c[:, None], 0.0)

    def collect_bag_grads(self, srcs, order, bag, B, E):
        return torch.from_numpy(self._contrib(srcs, bag, B, E)[order.long().numpy()].astype(np.float32))

    def bag_local_plan(self, bag, table_rows):
        return self.local_plan(bag.rows, None, 0, table_rows)

    def reduce_bags_into_buckets(self, plan, pos_u, bag, srcs, B, E, out):
        vals = self._contrib(srcs, bag, B, E)
        for u in range(int(plan.n_unique)):
            sl = plan.sorted_src[int(plan.seg_offsets[u]):int(plan.seg_offsets[u + 1])].long().numpy()
            out[int(pos_u[u])] = torch.from_numpy(vals[sl].sum(0).astype(np.float32))
        return out


VOCABS = [[5, 11, 3], [7, 2]]
POOLING = [["mean", "sum", "mean"], ["sum", "mean"]]
E, B = 4, 9


def _rank_sides(ops, rank, weighted, plain_second):
    """this rank's two sides (ragged bags with empty bags, trailing ids and out-of-range ids; the second side optionally a plain
    one riding along as length-one sum bags) and what the reference needs of them"""
    r2 = np.random.default_rng(1000 + rank)
    sides, outs, desc, base = [], [], [], 0
    for si, v in enumerate(VOCABS):
        K = len(v)
        off = (np.concatenate([[0], np.cumsum(v)[:-1]]) + base).astype(np.int64)
        base += sum(v)
        out = torch.full((B, K * E), 7.0)
        if plain_second and si == 1:
            ids = np.stack([r2.integers(-2, vk + 2, B) for vk in v], axis=1).astype(np.int64).reshape(-1)
            sides.append(ops.bag_side_from_lookup(ops.LookupSide(torch.from_numpy(ids), torch.from_numpy(off), torch.tensor(v, dtype=torch.int64),
                                                                 out, K), B))
            desc.append((ids, np.ones(B * K, np.int64), off, v, ["sum"] * K, np.ones(ids.size, np.float32)))
        else:
            lengths = r2.choice([0, 1, 2, 3, 11], B * K).astype(np.int64)
            ids = np.concatenate([r2.integers(-2, v[s % K] + 2, int(L)) for s, L in enumerate(lengths)] + [r2.integers(0, 2, 3)]).astype(np.int64)
            w = r2.uniform(0.5, 1.5, ids.size).astype(np.float32) if (weighted and si == 0) else None      # one weighted side, one not
            pool = torch.tensor([ops.POOL_MODES[p] for p in POOLING[si]], dtype=torch.int32)
            sides.append(ops.BagSide(torch.from_numpy(ids), torch.from_numpy(lengths), torch.from_numpy(off), torch.tensor(v, dtype=torch.int64),
                                     pool, out, K, True, weights=None if w is None else torch.from_numpy(w)))
            desc.append((ids, lengths, off, v, POOLING[si], np.ones(ids.size, np.float32) if w is None else w))
        outs.append(out)
    return sides, outs, desc, r2


def _worker(rank, world, port, q, kind, weighted, plain_second):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from jodalrob_twotower_amd import ops
        from jodalrob_twotower_amd.distributed import PaddedRowExchange, RowExchange, ShardedStore
        Rr = sum(map(sum, VOCABS))
        table = torch.from_numpy(np.random.default_rng(123).standard_normal((Rr, E)).astype(np.float32))      # same on every rank
        store = ShardedStore(E, Rr, rank, world, "cpu", "dense" if kind == "exact" else "sparse")
        store.load_global(table)
        be = BagCheckerBackend()
        ex = RowExchange(store, backend=be) if kind == "exact" else PaddedRowExchange(store, backend=be)
        sides, outs, desc, r2 = _rank_sides(ops, rank, weighted, plain_second)
        state = ex.forward_bags(sides, B, True)
        for out, (ids, lengths, off, v, pooling, w) in zip(outs, desc):
            ref, _, _, _ = RW.weighted_forward(table.numpy(), ids, lengths, off, v, pooling, w)
            assert np.array_equal(out.numpy(), ref.astype(np.float32)), "pooled block != the reference pooled from the unsharded table"
        rows_all, vals_all, srcs = [], [], []
        for s, (ids, lengths, off, v, pooling, w) in zip(sides, desc):
            d = torch.from_numpy(r2.standard_normal((B, s.K * E)).astype(np.float32))
            srcs.append((d, s.K))
            rws, vls = RW.contributions(d.numpy(), ids, lengths, off, v, pooling, w)
            rows_all.append(rws); vals_all.append(vls)
        ex.backward(state, srcs, B)
        gathered = [None] * world
        dist.all_gather_object(gathered, (np.concatenate(rows_all), np.concatenate(vals_all)))
        ref = np.zeros((Rr, E), np.float64)
        for rws, vls in gathered:
            np.add.at(ref, rws, vls)
        mine = ref[rank::world]
        np.testing.assert_allclose(be.dense_grad.numpy()[:mine.shape[0]], mine, rtol=1e-5, atol=1e-6)
        if kind == "padded":
            from jodalrob_twotower_amd.distributed import ExchangeOverflowError
            assert not ex.overflowed() and ex.C >= 256
            ex2 = PaddedRowExchange(store, backend=be, capacity=1)
            ex2.forward_bags(sides, B, False)
            assert ex2.overflowed()
            with pytest.raises(ExchangeOverflowError):
                ex2.check_overflow()
            assert ex.forward_bags(sides, B, False) is None               # eval-mode forward: no state
        # a position-weight source is refused before anything is routed
        bad = ops.BagSide(**{**sides[0].__dict__, "weights": None,
                             "pos_weights": ops.BagPosWeights(torch.ones(2), torch.zeros(sides[0].K, dtype=torch.int32),
                                                              torch.ones(sides[0].K, dtype=torch.int32))})
        with pytest.raises(ValueError, match="position weights"):
            ex.forward_bags([bad], B, False)
        q.put((rank, "ok"))
    except Exception:                                       # pragma: no cover
        import traceback
        q.put((rank, traceback.format_exc()))
    finally:
        dist.destroy_process_group()


def _run(target, world, *args):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=target, args=(r, world, port, q, *args)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=180) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    for rank, msg in res:
        assert msg == "ok", f"rank {rank}: {msg}"


@pytest.mark.parametrize("world,kind,weighted,plain_second", [(2, "exact", False, False), (3, "exact", True, True), (2, "padded", True, False),
                                                              (3, "padded", False, True)])
def test_bag_exchange_gloo(world, kind, weighted, plain_second):
    """Every rank's pooled block == the reference pooled from the unsharded table; every owner's summed row gradient == the global
    scatter-add of all ranks' contributions restricted to its rows."""
    _run(_worker, world, kind, weighted, plain_second)


# ------------------------------------------------------------------------------------------------ refusals
def _model(tt, schema_syn, **kw):
    kn, kc = schema_syn["notice"]["categorical"], schema_syn["company"]["categorical"]
    return tt.create_two_tower_model(kn, kc, metadata_path=str(GOLD / "synthetic_metadata.csv"), notice_dense_input_dim=3,
                                     company_dense_input_dim=2, final_embedding_dim=4, device="cpu", categorical_embedding_dim=4,
                                     tower_hidden_dims=[8, 4], **kw), kn, kc


def test_default_constructor_and_position_weights_are_refused(schema_syn):
    """pooled_exchange defaults to False: today's refusal, word for word; True refuses learned position weights -- both when the
    task is built, before any process group or device is touched."""
    import jodalrob_twotower_amd as tt
    from jodalrob_twotower_amd.distributed import DistributedTwoTowerTrainTask
    model, kn, kc = _model(tt, schema_syn, categorical_pooling={"company": "mean"})
    with pytest.raises(ValueError, match=r"sharded exchange step \(DistributedTwoTowerTrainTask\) does not support bag mode.*company_tower"):
        DistributedTwoTowerTrainTask(model, None)
    with pytest.raises(ValueError, match=r"sharded exchange step \(DistributedTwoTowerTrainTask\) does not support bag mode"):
        DistributedTwoTowerTrainTask(model, None, pooled_exchange=False)
    model, kn, kc = _model(tt, schema_syn, categorical_pooling={"company": "mean"}, categorical_position_weights={kc[0]: 3})
    with pytest.raises(ValueError, match=r"sharded exchange step .* does not support learned position weights.*company_tower"):
        DistributedTwoTowerTrainTask(model, None, pooled_exchange=True)


def _refusal_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import json
        import jodalrob_twotower_amd as tt
        from jodalrob_twotower_amd.distributed import create_distributed_train_task
        from jodalrob_twotower_amd.graph import GraphedTrainStep
        from jodalrob_twotower_amd.optim import FusedAdam
        from jodalrob_twotower_amd.segmented import SegmentedTrainStep
        from jodalrob_twotower_amd.unrolled import UnrolledTrainStep
        schema = json.loads((GOLD / "schema_synthetic.json").read_text())
        kn, kc = schema["notice"]["categorical"], schema["company"]["categorical"]
        task = create_distributed_train_task(kn, kc, metadata_path=str(GOLD / "synthetic_metadata.csv"), categorical_embedding_dim=4,
                                             notice_dense_input_dim=3, company_dense_input_dim=2, tower_hidden_dims=[8, 4],
                                             final_embedding_dim=4, device="cpu", backend=BagCheckerBackend(), exchange="exact",
                                             embedding_grad="dense", categorical_pooling={"company": "mean"})
        assert task.pooled_exchange and task.two_tower_model.company_tower.categorical_embedder.bag_mode
        assert not task.two_tower_model.notice_tower.categorical_embedder.bag_mode
        Bq, Kn, Kc = 3, len(kn), len(kc)
        w = torch.ones(2 * Bq * Kc, requires_grad=True)
        batch = {"notice": {"dense": torch.zeros(Bq, 3), "kjt": tt.build_batch_kjt(torch.zeros(Bq, Kn, dtype=torch.long), kn)},
                 "company": {"dense": torch.zeros(Bq, 2),
                             "kjt": tt.build_bag_kjt(kc, values=torch.zeros(2 * Bq * Kc, dtype=torch.long), lengths=torch.full((Bq * Kc,), 2),
                                                     weights=w)}}
        with pytest.raises(ValueError, match="per-id weights that require grad are not supported with the sharded table exchange"):
            task(batch)
        batch["company"]["kjt"] = tt.build_bag_kjt(kc, values=torch.zeros(2 * Bq * Kc, dtype=torch.long), lengths=torch.full((Bq * Kc,), 2))
        opt = FusedAdam.for_task(task)
        for cls in (GraphedTrainStep, SegmentedTrainStep, UnrolledTrainStep):
            with pytest.raises(ValueError, match=cls.__name__ + " does not support bag mode"):
                cls(task, opt, batch)
            with pytest.raises(ValueError, match="does not support bag mode|bag_capacity"):
                cls(task, opt, batch, bag_capacity="auto")
        q.put((rank, "ok"))
    except Exception:                                       # pragma: no cover
        import traceback
        q.put((rank, traceback.format_exc()))
    finally:
        dist.destroy_process_group()


def test_weights_requiring_grad_and_captured_steps_are_refused():
    """On a sharded bag-mode task (gloo world 1, CPU): KJT weights that require grad are refused in the towers' forward before any
    launch or collective; the captured, segmented and unrolled steps keep refusing bag mode."""
    _run(_refusal_worker, 1)


# ------------------------------------------------------------------------------------------------ the random-normal bar
def test_rank_order_f32_reduction_stays_under_the_random_normal_bar():
    """The sharded backward adds a row's contributions per rank (f32, position order) and the owner adds the ranks' sums in rank
    order (f32).  Against f64 that stays under RANDN_NORM_BOUND norm-wise -- over the whole matrix and for every single row: G = 3,
    Zipf rows, lengths 1..11, weights in U[0.5, 1.5), 20 seeds."""
    G, Rr, Ew, Bq = 3, 400, 8, 37
    worst_all = worst_row = 0.0
    for seed in range(20):
        rng = np.random.default_rng(seed)
        got = np.zeros((Rr, Ew), np.float32)
        ref = np.zeros((Rr, Ew), np.float64)
        for g in range(G):
            lengths = rng.integers(1, 12, Bq)
            rows = np.minimum(rng.zipf(1.3, int(lengths.sum())) - 1, Rr - 1)
            slot = np.repeat(np.arange(Bq), lengths)
            w = rng.uniform(0.5, 1.5, rows.size).astype(np.float32)
            inv = (np.float32(1) / lengths.astype(np.float32)).astype(np.float32)
            d = rng.standard_normal((Bq, Ew)).astype(np.float32)
            c = (w * inv[slot]).astype(np.float32)                       # one f32 product, as the kernel forms it
            part = np.zeros((Rr, Ew), np.float32)
            for p in range(rows.size):                                   # f32, position order (fma's single rounding is no worse)
                part[rows[p]] = (part[rows[p]] + c[p] * d[slot[p]]).astype(np.float32)
            got = (got + part).astype(np.float32)                        # the owner: rank order
            np.add.at(ref, rows, c[:, None].astype(np.float64) * d[slot].astype(np.float64))
        worst_all = max(worst_all, np.linalg.norm(got - ref) / np.linalg.norm(ref))
        nz = np.linalg.norm(ref, axis=1) > 0
        worst_row = max(worst_row, float((np.linalg.norm(got - ref, axis=1)[nz] / np.linalg.norm(ref, axis=1)[nz]).max()))
    print(f"worst norm-wise error: matrix {worst_all:.2e}, single row {worst_row:.2e}")
    assert worst_all <= RANDN_NORM_BOUND and worst_row <= RANDN_NORM_BOUND, (worst_all, worst_row)
