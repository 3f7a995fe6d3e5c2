#!/usr/bin/env python3
"""Bag-mode training fed from device-resident bag stores, on one MI355X at the bench shape: B = 8192, E = 32, the real schema's
32 + 6 keys on --rows table rows per tower, bf16 towers and score operands, row-sparse tables, FusedAdam.  The first --pool-keys
keys of each tower hold per-entity bags of Poisson(mean) ids (mean pooling, synthetic.bag_store), the others one id, for mean bag
lengths 1 / 4 / 16.  Per mean length, in THREE fresh processes (run one after the other):

  (a) gather_us        the two launches of tt_bag_store_gather alone (both towers, into buffers of the step's capacity), and
      gather_GBps      the bytes the shapes imply over that time -- per side B pair entries, B dense rows in and out, B*(K+1)
                       offsets in, B*K lengths out and the batch's ids in and out (gather_bytes, computed here);
  (b) store_fed_ms     GraphedTrainStep.step_from_store(bag stores, ..., bag_ids=...) per step: the gather, then the replay;
  (c) prebuilt_ms      the captured step(batch) of the same capacity on PREBUILT device batches (the same batches, gathered before the
                       clock starts): a floor no real loop reaches, somebody has to build those batches;
      eager_ms         the eager bag step on the same prebuilt batches: what a bag-mode user with real data runs today.
      (b) and the two of (c) alternate, --rounds times each, inside one process; each figure is the mean over its rounds.

Times: device events around --steps steps (every shape warmed up first), per step / per call.  The parent process collects the
children's lines, prints a summary per mean length -- (b) over the prebuilt floor, (b) against the FASTEST of the three eager runs,
and the run-to-run spread of (b) -- and writes everything to --out (default profiles/bag_store_bench.json).

--weighted: the stores also keep one f32 weight per id (synthetic.bag_store(weights="uniform")): (a) is tt_bag_store_gather_w moving ids
and weights (12 bytes per id each way instead of 8), (b) the store-fed step of a step captured with weights, (c) the weighted captured
and eager steps on prebuilt weighted batches.  Default --out: profiles/bag_store_weights_bench.json."""
import argparse
import contextlib
import io
import json
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=8192)
ap.add_argument("--rows", type=int, default=1_000_000, help="table rows per tower")
ap.add_argument("--entities", type=int, default=200_000, help="entities per store")
ap.add_argument("--hidden", default="128,64")
ap.add_argument("--final-dim", type=int, default=128)
ap.add_argument("--lengths", type=float, nargs="+", default=[1, 4, 16])
ap.add_argument("--pool-keys", type=int, default=2, help="pooled keys per tower (the first ones of its key list)")
ap.add_argument("--factor", type=float, default=2.0, help="bag_capacity over the pair table's mean ids per batch (the driver's default)")
ap.add_argument("--steps", type=int, default=60)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--batches", type=int, default=8, help="batches the steps rotate through")
ap.add_argument("--iters", type=int, default=200, help="calls of the gather alone")
ap.add_argument("--processes", type=int, default=3)
ap.add_argument("--child", type=int, default=None, help=argparse.SUPPRESS)
ap.add_argument("--weighted", action="store_true", help="stores with per-id weights: the weighted gather and the weighted steps")
ap.add_argument("--out", default=None)
a = ap.parse_args()
if a.out is None:
    a.out = str(ROOT / "profiles" / ("bag_store_weights_bench.json" if a.weighted else "bag_store_bench.json"))


def gather_bytes(B, sides, weighted=False):
    """bytes tt_bag_store_gather(_w) must move for one batch; sides: [(Din, K, ids of the batch)]"""
    total = 0
    for din, K, n in sides:
        total += 8 * B                      # the pair list's entity indices
        total += 2 * 4 * B * din            # dense rows, in and out
        total += 8 * B * (K + 1)            # a sample's K + 1 offsets
        total += 8 * B * K                  # lengths out
        total += 2 * 8 * n                  # ids, in and out
        total += 2 * 4 * n if weighted else 0      # their weights, in and out
    return total


def child():
    import math

    import numpy as np
    import torch
    sys.path.insert(0, str(ROOT))
    import jodalrob_twotower_amd as tt
    from jodalrob_twotower_amd import ops, synthetic
    from jodalrob_twotower_amd.data_loader import DeviceFeatureStore, DevicePairLoader
    from jodalrob_twotower_amd.graph import GraphedTrainStep
    from jodalrob_twotower_amd.optim import FusedAdam
    dev = torch.device("cuda:0")
    B, E, N = a.batch, 32, a.entities
    schema = synthetic.load_real_schema(ROOT / "jodalrob-twotower_amd" / "schema_real.json")
    keys = {"notice": schema["notice"]["categorical"], "company": schema["company"]["categorical"]}
    din = {"notice": 256, "company": 128}
    vocabs = {s: synthetic.scale_vocabs(schema[s]["vocab_sizes"], a.rows) for s in keys}
    pooled = {s: keys[s][:a.pool_keys] for s in keys}
    pooling = {k: "mean" for s in keys for k in pooled[s]}
    meta = synthetic.write_metadata(Path(tempfile.mkdtemp(prefix="tt_bagstore_")) / "metadata.csv",
                                    {s: dict(zip(keys[s], vocabs[s])) for s in keys})

    def make_task():
        torch.manual_seed(1234)
        with contextlib.redirect_stdout(io.StringIO()):
            task = tt.create_two_tower_train_task(keys["notice"], keys["company"], metadata_path=str(meta), categorical_embedding_dim=E,
                                                  notice_dense_input_dim=din["notice"], company_dense_input_dim=din["company"],
                                                  tower_hidden_dims=[int(h) for h in a.hidden.split(",")], final_embedding_dim=a.final_dim,
                                                  dropout_rate=0.1, temperature=1.0, device=dev, embedding_grad="sparse", score_dtype="bf16",
                                                  mlp_dtype="bf16", categorical_pooling=pooling)
        task.train()
        task._pair_check_done = True
        return task, FusedAdam.for_task(task, lr=1e-3, weight_decay=1e-5)

    def events(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(n):
            fn(i)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n                     # ms per call

    g = torch.Generator(device=dev)
    g.manual_seed(99)
    plain = {s: DeviceFeatureStore({"dense_projected": torch.randn((N, din[s]), generator=g, device=dev),
                                    "categorical": torch.stack([torch.randint(0, v, (N,), generator=g, device=dev) for v in vocabs[s]], 1)},
                                   keys[s], dev) for s in keys}
    P = a.batches * B
    pairs = torch.randint(0, N, (P, 2), generator=g, device=dev).cpu().numpy()
    for mean in a.lengths:
        stores = {s: synthetic.bag_store(plain[s], vocabs[s], pooled[s], mean, seed=7 + i, **({"weights": "uniform"} if a.weighted else {}))
                  for i, s in enumerate(keys)}
        loader = DevicePairLoader(stores["notice"], stores["company"], pairs, B, shuffle=True, seed=5)
        order = loader.epoch_order()
        counts = loader.epoch_bag_ids(order)
        ids = [{s: int(counts[s][k]) for s in keys} for k in range(a.batches)]
        caps = {s: max(math.ceil(a.factor * float(counts[s].mean())), int(counts[s].max())) for s in keys}
        prebuilt = [loader.batch(order, k * B, bag_ids=counts) for k in range(a.batches)]
        r = {"process": a.child, "weighted": a.weighted, "mean_bag_length": mean, "B": B, "E": E, "pooled_keys_per_tower": a.pool_keys, "rows_per_tower": a.rows,
             "entities": N, "ids_per_batch": {s: float(counts[s].mean()) for s in keys}, "capacity": caps, "steps": a.steps, "rounds": a.rounds}
        # (a) the gather alone, into buffers of the step's capacity
        bufs = {s: (torch.empty((B, din[s]), device=dev), torch.empty(B * len(keys[s]), dtype=torch.int64, device=dev),
                    torch.empty(caps[s], dtype=torch.int64, device=dev)) for s in keys}
        flat = loader.pairs.view(-1)
        wargs = {s: (stores[s].weights, torch.empty(caps[s], dtype=torch.float32, device=dev)) if a.weighted else () for s in keys}

        def gather(i):
            k = i % a.batches
            ops.bag_store_gather([], [ops.BagStoreSide(flat[j:], 2, stores[s].dense, stores[s].offsets, stores[s].values, len(keys[s]), *bufs[s], ids[k][s],
                                                       *wargs[s]) for j, s in enumerate(keys)], B, order, k * B)
        events(gather, 2 * a.batches)
        r["gather_us"] = round(events(gather, a.iters) * 1e3, 2)
        r["gather_bytes"] = int(np.mean([gather_bytes(B, [(din[s], len(keys[s]), ids[k][s]) for s in keys], a.weighted) for k in range(a.batches)]))
        r["gather_GBps"] = round(r["gather_bytes"] / (r["gather_us"] * 1e-6) / 1e9, 1)
        # (b), (c): three tasks on the same weights
        (tb, ob), (tc, oc), (te, oe) = make_task(), make_task(), make_task()
        gb = GraphedTrainStep(tb, ob, prebuilt[0], warmup=2, bag_capacity=caps)
        gc = GraphedTrainStep(tc, oc, prebuilt[0], warmup=2, bag_capacity=caps)

        def store_fed(i):
            k = i % a.batches
            gb.step_from_store(stores["notice"], stores["company"], loader.pairs, order, k * B, bag_ids=ids[k])

        def prebuilt_step(i):
            gc.step(prebuilt[i % a.batches])

        def eager(i):
            oe.zero_grad()
            res = te(prebuilt[i % a.batches], return_metrics=True)
            res["loss"].backward()
            oe.step()
        legs = {"store_fed_ms": store_fed, "prebuilt_ms": prebuilt_step, "eager_ms": eager}
        for fn in legs.values():
            events(fn, a.warmup)
        got = {name: [] for name in legs}
        for _ in range(a.rounds):
            for name, fn in legs.items():
                got[name].append(events(fn, a.steps))
        for name, v in got.items():
            r[name] = round(sum(v) / len(v), 4)
            r[name.replace("_ms", "_rounds_ms")] = [round(x, 4) for x in v]
        from jodalrob_twotower_amd import _lib
        _lib.check_device_errors(dev)
        gb.close()
        gc.close()
        del tb, ob, tc, oc, te, oe, gb, gc, stores, loader, prebuilt, bufs, wargs
        print("RESULT " + json.dumps(r), flush=True)


def parent():
    lines = []
    for p in range(a.processes):                           # fresh processes, one after the other
        cmd = [sys.executable, str(Path(__file__).resolve()), "--child", str(p)] + [x for x in sys.argv[1:]]
        out = subprocess.run(cmd, capture_output=True, text=True)
        if out.returncode != 0:
            sys.stderr.write(out.stdout[-2000:] + out.stderr[-4000:])
            raise SystemExit(f"process {p} failed with status {out.returncode}")
        got = [json.loads(ln[7:]) for ln in out.stdout.splitlines() if ln.startswith("RESULT ")]
        for r in got:
            print(json.dumps(r), flush=True)
        lines += got
    summary = []
    for mean in a.lengths:
        runs = [r for r in lines if r["mean_bag_length"] == mean]
        b, c, e = [r["store_fed_ms"] for r in runs], [r["prebuilt_ms"] for r in runs], [r["eager_ms"] for r in runs]
        s = {"mean_bag_length": mean, "weighted": a.weighted, "store_fed_ms": b, "prebuilt_ms": c, "eager_ms": e, "gather_us": [r["gather_us"] for r in runs],
             "gather_GBps": [r["gather_GBps"] for r in runs], "store_fed_over_prebuilt": round(sorted(b)[len(b) // 2] / sorted(c)[len(c) // 2], 3),
             "store_fed_spread_ms": round(max(b) - min(b), 4), "fastest_eager_ms": min(e), "slowest_store_fed_ms": max(b),
             "eager_minus_store_fed_ms": round(min(e) - max(b), 4), "store_fed_below_fastest_eager": max(b) < min(e)}
        summary.append(s)
        print("SUMMARY " + json.dumps(s), flush=True)
    p = Path(a.out)
    p.parent.mkdir(parents=True, exist_ok=True)
    p.write_text(json.dumps({"runs": lines, "summary": summary}, indent=1) + "\n")


if __name__ == "__main__":
    child() if a.child is not None else parent()
