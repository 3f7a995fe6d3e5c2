#!/usr/bin/env python3
"""Micro-benchmark of the pooled multi-valued lookup (tt_embed_bag_fwd) and its table gradient (tt_embed_bag_grad_bwd) at the
bench shape: B = 8192, E = 32, the real schema's 32 + 6 keys on 1 M + 1 M rows, every key a bag of Poisson(mean) ids for mean bag
lengths 1 (all bags exactly one id), 4 and 16.  Beside each, the plain lookup (tt_embed_lookup_fwd) and the plain gradient
(tt_embed_grad_bwd over the general plan, as the bags use) over the SAME number of gathered rows: a batch of nnz / 38 samples.

Times are device events around the C-ABI call alone (ops.KernelTimer), after warm-up, mean over --iters calls; "GB/s" is
ALGORITHMIC: the bytes the operation has to move by its definition over that time --
  lookup    read  nnz * (E * 4 + 8)  [rows + ids]  + slots * 8 [offsets];  write slots * E * out_bytes + nnz * 8 [rows_out, bag_of]
  plain     read  M * (E * 4 + 8);                                          write M * E * out_bytes + M * 4 [rows_out]
  gradient  read  nnz * (E * 4 + 8)  [the bag's d_out row, sorted_src, bag_of];  write U * E * 4
  plain     read  M * (E * 4 + 4);                                          write U * E * 4
(the gradient's d_out rows are re-read once per id of the bag, so its algorithmic bytes count each read).
--weighted: every id carries an f32 weight ~ U[0.5, 1.5) (tt_embed_bag_fwd_w / tt_embed_bag_grad_bwd_w): the lookup reads nnz * 4 more
bytes and writes nnz * 4 more (w_out), the gradient reads nnz * 4 more (pos_w); the plain figures beside it are unchanged.
--weight-grad (implies --weighted): also the gradient FOR the per-id weights (tt_embed_bag_weight_grad, both sides asked for, f32
sources) beside the weighted lookup on the same batch in the same process -- it gathers the same nnz table rows, which makes the
lookup its yardstick:
  weight gradient  read  nnz * (E * 4 + 8)  [rows + rows_out, bag_of]  + nnz * E * 4 [the bag's d_out row, once per id] + nnz * 4 [inv_len];
                   write nnz * 4
One JSON line per mean length; --out writes them as a JSON list too."""
import argparse
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import jodalrob_twotower_amd  # noqa: E402,F401
from jodalrob_twotower_amd import ops, synthetic  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=8192)
ap.add_argument("--rows", type=int, default=1_000_000, help="table rows per tower")
ap.add_argument("--iters", type=int, default=50)
ap.add_argument("--lengths", type=float, nargs="+", default=[1, 4, 16])
ap.add_argument("--out-dtype", choices=["f32", "bf16"], default="bf16", help="element type of the lookup output (the bench's x is bf16)")
ap.add_argument("--weighted", action="store_true", help="per-id weights: the _w entries (lookup and gradient)")
ap.add_argument("--weight-grad", action="store_true", help="also time tt_embed_bag_weight_grad beside the weighted lookup (implies --weighted)")
ap.add_argument("--tag", default="", help="copied into every result line (e.g. the run number, or 'parent')")
ap.add_argument("--out", default=None)
a = ap.parse_args()
a.weighted = a.weighted or a.weight_grad
dev = torch.device("cuda:0")
B, E = a.batch, 32
odt = torch.bfloat16 if a.out_dtype == "bf16" else torch.float32
osz = 2 if a.out_dtype == "bf16" else 4
schema = synthetic.load_real_schema(ROOT / "jodalrob-twotower_amd" / "schema_real.json")
keys = [schema["notice"]["categorical"], schema["company"]["categorical"]]
vocabs = [synthetic.scale_vocabs(schema["notice"]["vocab_sizes"], a.rows), synthetic.scale_vocabs(schema["company"]["vocab_sizes"], a.rows)]
Ks = [len(v) for v in vocabs]
offs, total = [], 0
for v in vocabs:
    o = []
    for x in v:
        o.append(total)
        total += x
    offs.append(torch.tensor(o, dtype=torch.int64, device=dev))
voc = [torch.tensor(v, dtype=torch.int64, device=dev) for v in vocabs]
table = torch.randn(total, E, device=dev)
pool = [torch.ones(K, dtype=torch.int32, device=dev) for K in Ks]           # mean pooling on every key (the weighted gradient)


def timed(names, fn, iters):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    t = ops.KernelTimer(names)
    ops.set_timer(t)
    try:
        for _ in range(iters):
            fn()
        s = t.summary()
    finally:
        ops.set_timer(None)
    return {n: s[n][1] * 1e3 for n in names}            # us


results = []
for mean in a.lengths:
    if mean == 1:
        batch = synthetic.make_batch(B, vocabs[0], vocabs[1], keys[0], keys[1], 4, 4, dev, 7)
    else:
        batch = synthetic.make_batch(B, vocabs[0], vocabs[1], keys[0], keys[1], 4, 4, dev, 7, bag_keys=set(keys[0]) | set(keys[1]),
                                     mean_bag_length=mean)
    outs = [torch.empty((B, K * E), dtype=odt, device=dev) for K in Ks]
    sides = [ops.BagSide(batch[s]["kjt"].values(), batch[s]["kjt"].lengths(), offs[i], voc[i], pool[i], outs[i], Ks[i], True)
             for i, s in enumerate(("notice", "company"))]
    if a.weighted:
        gw = torch.Generator(device=dev).manual_seed(11)
        for s in sides:
            s.weights = torch.rand(s.ids.numel(), generator=gw, device=dev) + 0.5
    nnz, slots = sum(int(s.ids.numel()) for s in sides), B * sum(Ks)
    wb = nnz * 4 if a.weighted else 0
    bag = ops.embed_bag_lookup(table, sides, B, want_rows=True)
    plan = ops.dedup_plan(bag.rows, total)
    U = int(plan.n_unique.item())
    srcs = [(torch.randn(B, K * E, device=dev), K) for K in Ks]
    grad = torch.empty((nnz, E), device=dev)
    t_bag = timed(["tt_embed_bag_fwd"], lambda: ops.embed_bag_lookup(table, sides, B, want_rows=True), a.iters)["tt_embed_bag_fwd"]
    t_bgrad = timed(["tt_embed_bag_grad_bwd"], lambda: ops.embed_bag_grad(plan, bag, srcs, B, E, ops.TT_GRAD_SPARSE, grad),
                    a.iters)["tt_embed_bag_grad_bwd"]
    # the plain path over as many gathered rows: nnz / 38 samples of one id per key
    Bp = max(1, round(nnz / sum(Ks)))
    pb = synthetic.make_batch(Bp, vocabs[0], vocabs[1], keys[0], keys[1], 4, 4, dev, 8)
    pouts = [torch.empty((Bp, K * E), dtype=odt, device=dev) for K in Ks]
    psides = [ops.LookupSide(pb[s]["kjt"].values(), offs[i], voc[i], pouts[i], Ks[i]) for i, s in enumerate(("notice", "company"))]
    prow = ops.embed_lookup(table, psides, Bp, want_rows=True)
    pplan = ops.dedup_plan(prow, total)
    pU, M = int(pplan.n_unique.item()), Bp * sum(Ks)
    psrcs = [(torch.randn(Bp, K * E, device=dev), K) for K in Ks]
    pgrad = torch.empty((M, E), device=dev)
    t_plain = timed(["tt_embed_lookup_fwd"], lambda: ops.embed_lookup(table, psides, Bp, want_rows=True), a.iters)["tt_embed_lookup_fwd"]
    t_pgrad = timed(["tt_embed_grad_bwd"], lambda: ops.embed_grad(pplan, psrcs, Bp, E, ops.TT_GRAD_SPARSE, pgrad), a.iters)["tt_embed_grad_bwd"]
    gbs = lambda nbytes, us: round(nbytes / (us * 1e-6) / 1e9, 1)
    r = {"tag": a.tag, "weighted": a.weighted, "mean_bag_length": mean, "B": B, "E": E, "keys": sum(Ks), "nnz": nnz, "unique_rows": U, "out_dtype": a.out_dtype,
         "bag_lookup_us": round(t_bag, 2), "bag_lookup_GBps": gbs(nnz * (E * 4 + 8) + slots * 8 + slots * E * osz + nnz * 8 + 2 * wb, t_bag),
         "plain_lookup_rows": M, "plain_lookup_us": round(t_plain, 2), "plain_lookup_GBps": gbs(M * (E * 4 + 8) + M * E * osz + M * 4, t_plain),
         "bag_over_plain_lookup_time_at_equal_rows": round(t_bag / t_plain * M / nnz, 3),
         "bag_grad_us": round(t_bgrad, 2), "bag_grad_GBps": gbs(nnz * (E * 4 + 8) + U * E * 4 + wb, t_bgrad),
         "plain_grad_us": round(t_pgrad, 2), "plain_grad_unique_rows": pU, "plain_grad_GBps": gbs(M * (E * 4 + 4) + pU * E * 4, t_pgrad),
         "bag_over_plain_grad_time_at_equal_rows": round(t_bgrad / t_pgrad * M / nnz, 3)}
    if a.weight_grad:
        t_wg = timed(["tt_embed_bag_weight_grad"], lambda: ops.bag_weight_grad(table, bag, srcs, B, [True, True]), a.iters)["tt_embed_bag_weight_grad"]
        r.update({"weight_grad_us": round(t_wg, 2), "weight_grad_GBps": gbs(nnz * (E * 4 + 8) + nnz * E * 4 + nnz * 4 + nnz * 4, t_wg),
                  "weight_grad_over_weighted_lookup_time": round(t_wg / t_bag, 3)})
    results.append(r)
    print(json.dumps(r), flush=True)
if a.out:
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    old = json.loads(Path(a.out).read_text()) if a.tag and Path(a.out).exists() else []      # (tagged runs append: one file per spread)
    Path(a.out).write_text(json.dumps(old + results, indent=1) + "\n")
