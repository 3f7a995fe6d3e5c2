#!/usr/bin/env python3
"""The eager row-wise SHARDED bag-mode step (fixed-capacity exchange, forward_bags) beside the eager UNSHARDED bag-mode step and
the eager sharded PLAIN step, in one process at RCCL world 1: B = 8192, E = 32, the real schema's 32 + 6 keys on --rows table rows
per tower, bf16 towers and score operands, row-sparse tables, FusedAdam.  The first --pool-keys keys of each tower hold ragged
bags of Poisson(mean) ids (mean pooling), the others one id, for mean bag lengths 1 / 4 / 16 (the shapes of
tools/bench_embed_bag_step.py).  Per mean length one JSON line:

  * sharded_bag_ms      DistributedTwoTowerTrainTask(pooled_exchange=True), exchange "padded": forward, backward, optimiser step;
  * unsharded_bag_ms    the same model unsharded (create_two_tower_train_task(categorical_pooling=...));
  * sharded_plain_ms    the sharded step of the plain model on one id per key (the same for every mean length: measured once).

All three are eager steps launched one call at a time from Python: host clock around --steps steps that end in a device
synchronise, after --warmup steps, ms per step.  Nothing with more than one rank runs here: at world 1 every all-to-all is a
copy onto the rank itself, so the figures price the launches and the host work of the route, not the wire.  Run it several
times (fresh processes) for a spread; --out appends the lines to a JSON list."""
import argparse
import contextlib
import io
import json
import os
import socket
import sys
import tempfile
import time
from pathlib import Path

import torch
import torch.distributed as dist

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import jodalrob_twotower_amd as tt  # noqa: E402
from jodalrob_twotower_amd import synthetic  # noqa: E402
from jodalrob_twotower_amd.distributed import create_distributed_train_task  # noqa: E402
from jodalrob_twotower_amd.optim import FusedAdam  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=8192)
ap.add_argument("--rows", type=int, default=1_000_000, help="table rows per tower")
ap.add_argument("--hidden", default="128,64")
ap.add_argument("--final-dim", type=int, default=128)
ap.add_argument("--lengths", type=float, nargs="+", default=[1, 4, 16])
ap.add_argument("--pool-keys", type=int, default=2, help="pooled keys per tower (the first ones of its key list)")
ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--pool", type=int, default=4, help="batches the steps rotate through")
ap.add_argument("--tag", default="", help="copied into every result line (e.g. the run number)")
ap.add_argument("--out", default=None)
a = ap.parse_args()

dev = torch.device("cuda:0")
sk = socket.socket(); sk.bind(("127.0.0.1", 0)); port = sk.getsockname()[1]; sk.close()
os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)

B, E = a.batch, 32
schema = synthetic.load_real_schema(ROOT / "jodalrob-twotower_amd" / "schema_real.json")
keys = {"notice": schema["notice"]["categorical"], "company": schema["company"]["categorical"]}
vocabs = {s: synthetic.scale_vocabs(schema[s]["vocab_sizes"], a.rows) for s in keys}
pooled = {s: keys[s][:a.pool_keys] for s in keys}
meta = synthetic.write_metadata(Path(tempfile.mkdtemp(prefix="tt_bagexch_")) / "metadata.csv",
                                {s: dict(zip(keys[s], vocabs[s])) for s in keys})
common = dict(metadata_path=str(meta), categorical_embedding_dim=E, notice_dense_input_dim=256, company_dense_input_dim=128,
              tower_hidden_dims=[int(h) for h in a.hidden.split(",")], final_embedding_dim=a.final_dim, dropout_rate=0.1, temperature=1.0,
              device=dev, embedding_grad="sparse", score_dtype="bf16", mlp_dtype="bf16")


def make_task(sharded, pooling):
    torch.manual_seed(1234)
    with contextlib.redirect_stdout(io.StringIO()):
        if sharded:
            task = create_distributed_train_task(keys["notice"], keys["company"], exchange="padded", categorical_pooling=pooling, **common)
        else:
            task = tt.create_two_tower_train_task(keys["notice"], keys["company"], categorical_pooling=pooling, **common)
    task.train()
    task._pair_check_done = True
    return task, FusedAdam.for_task(task, lr=1e-3, weight_decay=1e-5)


def batches(mean, n):
    bag_keys = set(pooled["notice"]) | set(pooled["company"])
    return [synthetic.make_batch(B, vocabs["notice"], vocabs["company"], keys["notice"], keys["company"], 256, 128, dev, seed=1234 + 7919 * i,
                                 **({} if mean is None else dict(bag_keys=bag_keys, mean_bag_length=mean))) for i in range(n)]


def clock(sharded, pooling, pool):
    task, opt = make_task(sharded, pooling)

    def step(b):
        opt.zero_grad()
        res = task(b, return_metrics=True)
        res["loss"].backward()
        opt.step()
    for i in range(a.warmup):
        step(pool[i % len(pool)])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(a.steps):
        step(pool[i % len(pool)])
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / a.steps
    if sharded:
        task.exchange.check_overflow()
    cap = getattr(getattr(task, "exchange", None), "C", None)
    del task, opt
    return round(ms, 4), cap


plain_ms, plain_cap = clock(True, None, batches(None, a.pool))
results = []
for mean in a.lengths:
    pool = batches(mean, a.pool)
    pooling = {k: "mean" for s in keys for k in pooled[s]}
    r = {"tag": a.tag, "mean_bag_length": mean, "B": B, "E": E, "keys": sum(len(k) for k in keys.values()), "pooled_keys_per_tower": a.pool_keys,
         "rows_per_tower": a.rows, "world": 1, "nnz": {s: max(b[s]["kjt"].values().numel() for b in pool) for s in keys}, "steps": a.steps}
    r["sharded_bag_ms"], r["bucket_capacity"] = clock(True, pooling, pool)
    r["unsharded_bag_ms"], _ = clock(False, pooling, pool)
    r["sharded_plain_ms"], r["plain_bucket_capacity"] = plain_ms, plain_cap
    results.append(r)
    print(json.dumps(r), flush=True)
if a.out:
    p = Path(a.out)
    p.parent.mkdir(parents=True, exist_ok=True)
    old = json.loads(p.read_text()) if p.exists() else []
    p.write_text(json.dumps(old + results, indent=1) + "\n")
torch.cuda.synchronize()
dist.destroy_process_group()
