#!/usr/bin/env python3
"""Cost of shared extra negatives at BASELINE configs[1]'s shapes (B = 8192, 32 + 6 real keys, 1 M + 1 M table rows, E = 32, towers
[128, 64] -> 64, bf16 score and MLP operands, sparse table gradients, T = 1) with M = 1024 and M = 8192 extras, against the plain step
in ONE process, the two alternating, best of --reps blocks:

  * the eager training step (forward, backward, FusedAdam) on a batch with / without "negatives" -- the company tower runs over
    B + M rows, the score node packs N, C and X and runs the extended sweep, the square backward and the extras' launch;
  * the captured step (GraphedTrainStep.step(batch) on a batch with / without "negatives": with them the plain-copy hand-over, without
    them the key-major one);
  * the score node alone (_ScoreCEFn: packs + symmetric forward + backward(s)).

Writes --out (default profiles/extra_negatives_bench.json).
"""
import argparse
import json
import sys
import tempfile
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import jodalrob_twotower_amd as tt  # noqa: E402
from jodalrob_twotower_amd import synthetic  # noqa: E402
from jodalrob_twotower_amd.graph import GraphedTrainStep  # noqa: E402
from jodalrob_twotower_amd.optim import FusedAdam  # noqa: E402
from jodalrob_twotower_amd.two_tower_train_task import _ScoreCEFn  # noqa: E402

DEV = torch.device("cuda:0")


def _timed(fn, n):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for i in range(n):
        fn(i)
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / n


def _alternate(fns, steps, reps):
    """best-of-reps ms per call of each named callable, the callables alternating block by block"""
    for fn in fns.values():
        for i in range(5):
            fn(i)
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            t[k].append(_timed(fn, steps))
    return {k: min(v) for k, v in t.items()}, t


def _world(args, tmp):
    real = synthetic.load_real_schema(ROOT / "jodalrob-twotower_amd" / "schema_real.json")
    kn, kc = real["notice"]["categorical"], real["company"]["categorical"]
    vn = synthetic.scale_vocabs(real["notice"]["vocab_sizes"], 1_000_000)
    vc = synthetic.scale_vocabs(real["company"]["vocab_sizes"], 1_000_000)
    meta = synthetic.write_metadata(tmp / "xneg_bench_metadata.csv", {"notice": dict(zip(kn, vn)), "company": dict(zip(kc, vc))})
    B = args.batch
    batches = [synthetic.make_batch(B, vn, vc, kn, kc, 256, 128, DEV, seed=100 + i) for i in range(4)]

    def make_task():
        torch.manual_seed(1)
        task = tt.create_two_tower_train_task(kn, kc, metadata_path=str(meta), categorical_embedding_dim=32, notice_dense_input_dim=256,
                                              company_dense_input_dim=128, tower_hidden_dims=[128, 64], final_embedding_dim=64,
                                              dropout_rate=0.2, temperature=1.0, device=DEV, embedding_grad="sparse", score_dtype="bf16",
                                              mlp_dtype="bf16")
        task.train()
        task._pair_check_done = True
        return task, FusedAdam.for_task(task, lr=1e-3, weight_decay=1e-5)

    def with_neg(M):
        out = []
        for i, b in enumerate(batches):
            other = synthetic.make_batch(M, vn, vc, kn, kc, 256, 128, DEV, seed=500 + i)["company"]
            out.append(dict(b, negatives=other))
        return out
    return make_task, {"plain": batches, **{f"M{M}": with_neg(M) for M in args.extras}}


def _ratios(args, best, every, unit):
    out = {f"{k}_{unit}": v for k, v in best.items()}
    out.update({f"{k}_{unit}_all": v for k, v in every.items()})
    for M in args.extras:
        out[f"M{M}_ratio"] = best[f"M{M}"] / best["plain"]
    return out


def captured_steps(args, make_task, sets):
    steps = {}
    for k, bs in sets.items():
        task, opt = make_task()
        steps[k] = (GraphedTrainStep(task, opt, bs[0], warmup=3, return_metrics=False), bs)
    best, every = _alternate({k: (lambda i, gs=gs, bs=bs: gs.step(bs[i % len(bs)])) for k, (gs, bs) in steps.items()}, args.steps, args.reps)
    for gs, _ in steps.values():
        gs.close()
    return _ratios(args, best, every, "ms_per_step")


def eager_steps(args, make_task, sets):
    task, opt = make_task()

    def step_on(bs):
        def f(i):
            opt.zero_grad()
            task(bs[i % len(bs)]).backward()
            opt.step()
        return f
    best, every = _alternate({k: step_on(bs) for k, bs in sets.items()}, args.steps, args.reps)
    return _ratios(args, best, every, "ms_per_step")


def score_node(args):
    B, D = args.batch, 64
    g = torch.Generator(device=DEV).manual_seed(1)

    def unit(R):
        x = torch.randn(R, D, generator=g, device=DEV)
        return x / x.norm(dim=1, keepdim=True)
    n, c = unit(B), unit(B)
    xs = {M: unit(M) for M in args.extras}

    def node(x):
        def f(_):
            a, b = n.detach().requires_grad_(True), c.detach().requires_grad_(True)
            xx = None if x is None else x.detach().requires_grad_(True)
            loss, _, _ = _ScoreCEFn.apply(a, b, 1.0, "bf16", False, False, None, None, None, None, None, None, None, None, xx)
            loss.backward()
        return f
    best, _ = _alternate({"plain": node(None), **{f"M{M}": node(x) for M, x in xs.items()}}, 50, args.reps)
    out = {f"{k}_us": 1000 * v for k, v in best.items()}
    for M in args.extras:
        out[f"M{M}_ratio"] = best[f"M{M}"] / best["plain"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--extras", type=int, nargs="+", default=[1024, 8192])
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "extra_negatives_bench.json"))
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as d:
        make_task, sets = _world(args, Path(d))
        res = {"device": torch.cuda.get_device_name(0), "batch": args.batch, "D": 64, "extras": args.extras, "reps": args.reps,
               "timing": "best of reps, the variants alternating in one process",
               "eager_step": eager_steps(args, make_task, sets), "captured_step": captured_steps(args, make_task, sets),
               "score_node": score_node(args)}
    Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
