#!/usr/bin/env python3
"""Cost of per-pair sample weights at BASELINE configs[1]'s shapes (B = 8192, 32 + 6 real keys, 1 M + 1 M table rows, E = 32,
towers [128, 64] -> 64, bf16 score and MLP operands, sparse table gradients, T = 1), measured two ways in ONE process, plain and
weighted alternating:

  * the captured training step (GraphedTrainStep.step on a batch with / without "pair_weight"), medians of --reps blocks of --steps;
  * the score node alone (_ScoreCEFn: weight preparation + symmetric forward + backward) at D = 64 and D = 128.

The weights are those of a synthetic pair table with repeated notices: each batch's pairs draw their notice from a Zipf(1.1) law over
50 000 notices, and a pair weighs 1 / (the batch's pairs of its notice) -- pair_weights.inverse_count_weights on the batch.

Writes --out (default profiles/pair_weight_bench.json).  --only plain|weighted times just that captured step (for a `rocprofv3
--kernel-trace --stats` run of each, taken separately).
"""
import argparse
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import jodalrob_twotower_amd as tt  # noqa: E402
from jodalrob_twotower_amd import ops, synthetic  # noqa: E402
from jodalrob_twotower_amd.graph import GraphedTrainStep  # noqa: E402
from jodalrob_twotower_amd.optim import FusedAdam  # noqa: E402
from jodalrob_twotower_amd.pair_weights import inverse_count_weights  # noqa: E402
from jodalrob_twotower_amd.two_tower_train_task import _ScoreCEFn  # noqa: E402

DEV = torch.device("cuda:0")


def _median(v):
    return sorted(v)[len(v) // 2]


def _task(meta, kn, kc):
    torch.manual_seed(1)
    task = tt.create_two_tower_train_task(kn, kc, metadata_path=str(meta), categorical_embedding_dim=32, notice_dense_input_dim=256,
                                          company_dense_input_dim=128, tower_hidden_dims=[128, 64], final_embedding_dim=64,
                                          dropout_rate=0.2, temperature=1.0, device=DEV, embedding_grad="sparse", score_dtype="bf16",
                                          mlp_dtype="bf16")
    task.train()
    task._pair_check_done = True
    return task, FusedAdam.for_task(task, lr=1e-3, weight_decay=1e-5)


def _weights(B, seed):
    """f32 [B]: 1 / (pairs of the row's notice in this batch), notices drawn from a Zipf(1.1) law over 50 000"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    p = torch.arange(1, 50_001, dtype=torch.float32, device=DEV) ** -1.1
    en = torch.multinomial(p, B, replacement=True, generator=g)
    return inverse_count_weights(torch.stack([en, torch.zeros_like(en)], 1)).contiguous()


def steps(args, tmp):
    real = synthetic.load_real_schema(ROOT / "jodalrob-twotower_amd" / "schema_real.json")
    kn, kc = real["notice"]["categorical"], real["company"]["categorical"]
    vn = synthetic.scale_vocabs(real["notice"]["vocab_sizes"], 1_000_000)
    vc = synthetic.scale_vocabs(real["company"]["vocab_sizes"], 1_000_000)
    meta = synthetic.write_metadata(tmp / "pw_bench_metadata.csv", {"notice": dict(zip(kn, vn)), "company": dict(zip(kc, vc))})
    B = args.batch
    batches = [synthetic.make_batch(B, vn, vc, kn, kc, 256, 128, DEV, seed=100 + i) for i in range(8)]
    pw_batches = [dict(b, pair_weight=_weights(B, 5 + i)) for i, b in enumerate(batches)]
    modes = [args.only] if args.only else ["plain", "weighted"]
    runs = {}
    for m in modes:
        task, opt = _task(meta, kn, kc)
        bs = batches if m == "plain" else pw_batches
        runs[m] = (GraphedTrainStep(task, opt, bs[0], warmup=3, return_metrics=False), bs)
    for m, (gs, bs) in runs.items():
        for i in range(20):
            gs.step(bs[i % len(bs)])
    torch.cuda.synchronize()
    t = {m: [] for m in runs}
    for _ in range(args.reps):
        for m, (gs, bs) in runs.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for i in range(args.steps):
                gs.step(bs[i % len(bs)])
            e.record()
            torch.cuda.synchronize()
            t[m].append(s.elapsed_time(e) / args.steps)
    for gs, _ in runs.values():
        gs.close()
    out = {f"{m}_ms_per_step": _median(v) for m, v in t.items()}
    out.update({f"{m}_ms_per_step_all": v for m, v in t.items()})
    if len(t) == 2:
        out["ratio"] = out["weighted_ms_per_step"] / out["plain_ms_per_step"]
    return out


def score_node(args):
    out = {}
    for D in (64, 128):
        B = args.batch
        g = torch.Generator(device=DEV).manual_seed(1)
        n = torch.randn(B, D, generator=g, device=DEV)
        n /= n.norm(dim=1, keepdim=True)
        c = torch.randn(B, D, generator=g, device=DEV)
        c /= c.norm(dim=1, keepdim=True)
        w = _weights(B, 9)
        sn = ops.score_unit_scale(1.0)
        Np, Cp = ops.score_pack2_bf16(n, c, sn, 1.0)

        def step(with_pw):
            a, b = n.detach().requires_grad_(True), c.detach().requires_grad_(True)
            loss, _, _ = _ScoreCEFn.apply(a, b, 1.0, "bf16", False, False, Np, Cp, sn, None, None, None, None, w if with_pw else None)
            loss.backward()
        for _ in range(20):
            step(False)
            step(True)
        t = {False: [], True: []}
        for _ in range(args.reps):
            for k in (False, True):
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                for _ in range(50):
                    step(k)
                e.record()
                torch.cuda.synchronize()
                t[k].append(s.elapsed_time(e) / 50 * 1000)
        out[f"D{D}"] = {"plain_us": _median(t[False]), "weighted_us": _median(t[True]), "ratio": _median(t[True]) / _median(t[False])}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", choices=["plain", "weighted"], default=None)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "pair_weight_bench.json"))
    args = ap.parse_args()
    tmp = Path(args.out).resolve().parent
    tmp.mkdir(parents=True, exist_ok=True)
    res = {"workload": "configs[1] shapes: B = %d, 32+6 real keys, 1M + 1M rows, E=32, towers [128,64] -> 64, bf16, sparse, T = 1, "
                       "dropout 0.2; pair weights: 1 / (the batch's pairs of the row's notice), notices Zipf(1.1) over 50 000" % args.batch,
           "step": steps(args, tmp)}
    if not args.only:
        res["score_node"] = score_node(args)
    (tmp / "pw_bench_metadata.csv").unlink(missing_ok=True)
    print(json.dumps(res))
    if not args.only:
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
