#!/usr/bin/env python3
"""The bag-mode training step, eager against captured (GraphedTrainStep(bag_capacity=...)), at the bench shape: B = 8192, E = 32,
the real schema's 32 + 6 keys on --rows table rows per tower, bf16 towers and score operands, row-sparse tables, FusedAdam.  The
first --pool-keys keys of each tower hold ragged bags of Poisson(mean) ids (mean pooling), the others one id, for mean bag lengths
1 / 4 / 16.  Per mean length:

  * eager_ms            the eager step (task forward, backward, optimiser step; launched one call at a time from Python);
  * captured_ms[f]      the captured step at a capacity of f times the batch's ids per bag-mode side, f in --factors, each fed a
                        rotating pool of batches through step(batch) (hand-over launch + one graph replay);
  * prepare_us / torch_prepare_us   tt_bag_prepare alone against the torch ops it replaces on a captured chain (the zero-filled
                        offsets, cumsum, and the mean weights' compare / convert / clamp / divide / select chain), device events;
  * lookup_cap_us[f], plan_pad_us[f]   the capacity lookup and the padded plan alone at each capacity, beside the exact entries'
                        lookup_us / plan_us on the live ids (what the pads cost);
  * plain_captured_launches         library_launches of the PLAIN model's captured step at this shape (this path must not change).

Step times: a host clock around --steps steps that end in a device synchronise, after --warmup steps, in ms per step.  Run it
several times (fresh processes) for a spread: every run prints one JSON line per mean length; --out appends them to a JSON list.
--weighted: every id of the bag-mode sides carries an f32 weight (synthetic.ragged_bags(weights="uniform")): the eager and the
captured step then run the weighted entries (tt_embed_bag_fwd_w / _cap_w / tt_embed_bag_grad_bwd_w), and so do the launch-level figures.
--position-weights MAXLEN: the pooled keys of both towers learn MAXLEN position weights each (categorical_position_weights): the
eager step then also expands the parameter, forms the per-id weight gradient and reduces it; the captured leg is
GraphedTrainStep(learned_weights=True): the pooled lookup reads the parameter by position and the gradient chain runs over the
capacity inside the graph.  Not with --weighted (one source of weights per embedder); the launch-level figures are left out.  Its
yardsticks are the eager step of the same model and the captured --weighted step.
--captured-only: no eager leg (eager_ms is null).  --steps-only: no launch-level figures."""
import argparse
import contextlib
import io
import json
import sys
import tempfile
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import jodalrob_twotower_amd as tt  # noqa: E402
from jodalrob_twotower_amd import ops, synthetic  # noqa: E402
from jodalrob_twotower_amd.graph import GraphedTrainStep  # noqa: E402
from jodalrob_twotower_amd.optim import FusedAdam  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=8192)
ap.add_argument("--rows", type=int, default=1_000_000, help="table rows per tower")
ap.add_argument("--hidden", default="128,64")
ap.add_argument("--final-dim", type=int, default=128)
ap.add_argument("--lengths", type=float, nargs="+", default=[1, 4, 16])
ap.add_argument("--factors", type=float, nargs="+", default=[1.0, 1.25, 2.0, 4.0])
ap.add_argument("--pool-keys", type=int, default=2, help="pooled keys per tower (the first ones of its key list)")
ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--pool", type=int, default=4, help="batches the steps rotate through")
ap.add_argument("--iters", type=int, default=50, help="calls per launch-level figure")
ap.add_argument("--tag", default="", help="copied into every result line (e.g. the run number, or 'parent')")
ap.add_argument("--weighted", action="store_true", help="per-id weights on the bag-mode sides: the weighted entries")
ap.add_argument("--position-weights", type=int, default=None, metavar="MAXLEN", help="learned position weights on the pooled keys of both towers")
ap.add_argument("--captured-only", action="store_true", help="skip the eager leg")
ap.add_argument("--steps-only", action="store_true", help="skip the launch-level figures (a kernel trace then holds the steps' launches alone)")
ap.add_argument("--eager-only", action="store_true", help="the eager step only (a checkout without bag_capacity)")
ap.add_argument("--out", default=None)
a = ap.parse_args()
if a.position_weights is not None:
    if a.weighted:
        ap.error("--position-weights: not with --weighted (one source of weights per embedder)")
dev = torch.device("cuda:0")
B, E = a.batch, 32
schema = synthetic.load_real_schema(ROOT / "jodalrob-twotower_amd" / "schema_real.json")
keys = {"notice": schema["notice"]["categorical"], "company": schema["company"]["categorical"]}
vocabs = {s: synthetic.scale_vocabs(schema[s]["vocab_sizes"], a.rows) for s in keys}
pooled = {s: keys[s][:a.pool_keys] for s in keys}
meta = synthetic.write_metadata(Path(tempfile.mkdtemp(prefix="tt_bagstep_")) / "metadata.csv",
                                {s: dict(zip(keys[s], vocabs[s])) for s in keys})


def make_task(pooling):
    torch.manual_seed(1234)
    with contextlib.redirect_stdout(io.StringIO()):
        task = tt.create_two_tower_train_task(keys["notice"], keys["company"], metadata_path=str(meta), categorical_embedding_dim=E,
                                              notice_dense_input_dim=256, company_dense_input_dim=128,
                                              tower_hidden_dims=[int(h) for h in a.hidden.split(",")], final_embedding_dim=a.final_dim,
                                              dropout_rate=0.1, temperature=1.0, device=dev, embedding_grad="sparse", score_dtype="bf16",
                                              mlp_dtype="bf16", categorical_pooling=pooling,
                                              **({} if a.position_weights is None or pooling is None else
                                                 dict(categorical_position_weights={k: a.position_weights for k in pooling})))
    task.train()
    task._pair_check_done = True
    return task, FusedAdam.for_task(task, lr=1e-3, weight_decay=1e-5)


def batches(mean, n):
    bag_keys = set(pooled["notice"]) | set(pooled["company"])
    return [synthetic.make_batch(B, vocabs["notice"], vocabs["company"], keys["notice"], keys["company"], 256, 128, dev, seed=1234 + 7919 * i,
                                 **({} if mean is None else dict(bag_keys=bag_keys, mean_bag_length=mean)),
                                 **(dict(bag_weights="uniform") if a.weighted and mean is not None else {})) for i in range(n)]


def clock(step, pool):
    for i in range(a.warmup):
        step(pool[i % len(pool)])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(a.steps):
        step(pool[i % len(pool)])
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / a.steps


def events(fn):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / a.iters          # us per call


def torch_prepare(lengths, pools):
    """what ops.embed_bag_lookup forms with torch ops per side"""
    out = []
    for ln, pool in zip(lengths, pools):
        off = torch.zeros(ln.numel() + 1, dtype=torch.int64, device=dev)
        torch.cumsum(ln, 0, out=off[1:])
        lf = ln.to(torch.float32)
        mean = (pool != 0).repeat(B) & (ln > 0)
        one = torch.ones_like(lf)
        out.append((off, torch.where(mean, one / lf.clamp(min=1.0), one)))
    return out


plain_launches = None
if not a.eager_only:
    task, opt = make_task(None)
    g = GraphedTrainStep(task, opt, batches(None, 1)[0], warmup=2)
    plain_launches = g.library_launches
    g.close()
    del task, opt, g

results = []
for mean in a.lengths:
    pool = batches(mean, a.pool)
    nnz = {s: max(b[s]["kjt"].values().numel() for b in pool) for s in keys}
    r = {"tag": a.tag, "weighted": a.weighted, "position_weights": a.position_weights, "mean_bag_length": mean, "B": B, "E": E, "keys": sum(len(k) for k in keys.values()), "pooled_keys_per_tower": a.pool_keys,
         "rows_per_tower": a.rows, "nnz": nnz, "steps": a.steps, "plain_captured_launches": plain_launches}
    pooling = {k: "mean" for s in keys for k in pooled[s]}
    r["eager_ms"] = None
    if not a.captured_only:
        task, opt = make_task(pooling)

        def eager(b):
            opt.zero_grad()
            res = task(b, return_metrics=True)
            res["loss"].backward()
            opt.step()
        r["eager_ms"] = round(clock(eager, pool), 4)
        del task, opt
    if not a.eager_only:
        r["captured_ms"], r["captured_launches"], r["capacity"] = {}, {}, {}
        for f in a.factors:
            task, opt = make_task(pooling)
            caps = {s: int(-(-nnz[s] * f // 1)) for s in keys}
            g = GraphedTrainStep(task, opt, pool[0], warmup=2, bag_capacity=caps,
                                 **(dict(learned_weights=True) if a.position_weights is not None else {}))
            r["captured_ms"][str(f)] = round(clock(g.step, pool), 4)
            r["captured_launches"][str(f)] = g.library_launches
            r["capacity"][str(f)] = caps
            g.close()
            del task, opt, g
    if not a.eager_only and a.position_weights is None and not a.steps_only:
        # the launches alone, on pool[0]
        task, _ = make_task(pooling)
        m = task.two_tower_model
        embs = [m.notice_tower.categorical_embedder, m.company_tower.categorical_embedder]
        b = pool[0]
        lengths = [b[s]["kjt"].lengths() for s in keys]
        ids = [b[s]["kjt"].values() for s in keys]
        Ks = [len(keys[s]) for s in keys]
        pools = [e._key_pool for e in embs]
        live = [v.numel() for v in ids]
        wts = [b[s]["kjt"].weights_or_none() for s in keys]
        r["torch_prepare_us"] = round(events(lambda: torch_prepare(lengths, pools)), 2)
        r["prepare_us"] = round(events(lambda: ops.bag_prepare(lengths, pools, Ks, B, live, None)), 2)
        table = embs[0].store.weight
        outs = [torch.empty((B, K * E), dtype=torch.bfloat16, device=dev) for K in Ks]
        exact = [e.bag_side(v, ln, o, weights=w) for e, v, ln, o, w in zip(embs, ids, lengths, outs, wts)]
        bag = ops.embed_bag_lookup(table, exact, B, want_rows=True)
        r["lookup_us"] = round(events(lambda: ops.embed_bag_lookup(table, exact, B, want_rows=True)), 2)
        r["plan_us"] = round(events(lambda: ops.dedup_plan(bag.rows, table.shape[0])), 2)
        r["lookup_cap_us"], r["plan_pad_us"] = {}, {}
        for f in a.factors:
            caps = [int(-(-n * f // 1)) for n in live]
            bufs = [torch.cat([v, torch.full((c - v.numel(),), 1 << 40, dtype=torch.int64, device=dev)]) for v, c in zip(ids, caps)]
            counts = [torch.tensor([n], dtype=torch.int32, device=dev) for n in live]
            wbufs = [None if w is None else torch.cat([w, torch.zeros(c - w.numel(), device=dev)]) for w, c in zip(wts, caps)]
            cap_sides = [e.bag_side(v, ln, o, cnt, w) for e, v, ln, o, cnt, w in zip(embs, bufs, lengths, outs, counts, wbufs)]
            bagc = ops.embed_bag_lookup(table, cap_sides, B, want_rows=True)
            r["lookup_cap_us"][str(f)] = round(events(lambda: ops.embed_bag_lookup(table, cap_sides, B, want_rows=True)), 2)   # (prepare included)
            r["plan_pad_us"][str(f)] = round(events(lambda: ops.bag_dedup_plan(bagc, table.shape[0])), 2)
        del task
    results.append(r)
    print(json.dumps(r), flush=True)
if a.out:
    p = Path(a.out)
    p.parent.mkdir(parents=True, exist_ok=True)
    old = json.loads(p.read_text()) if p.exists() else []
    p.write_text(json.dumps(old + results, indent=1) + "\n")
