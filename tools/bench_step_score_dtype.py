#!/usr/bin/env python3
"""Graphed training step per score_dtype at configs[1] shapes (bench.py's single-GPU leg: B = 8192, 1 M + 1 M rows, towers
[128, 64] -> 64, dropout 0.1, mlp_dtype bf16), in ALTERNATED runs: round r runs every score_dtype once, each in a fresh process,
so drift of the box is shared by all of them.  bench.py's --score-dtype choices stay as they are: a child process builds
bench.py's arguments and sets score_dtype itself (which is how 'bf16x3' gets in).

    python tools/bench_step_score_dtype.py --rounds 3 --steps 200 --warmup 50 [--dtypes fp32,bf16,bf16x3] [--out FILE]

Prints one JSON line: per score_dtype the ms_per_step of every round, their median, and each median's speed-up over fp32."""
import argparse
import json
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]


def child(dtype, steps, warmup):
    sys.path.insert(0, str(ROOT))
    import bench
    args = bench.parse(["--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--mlp-dtype", "bf16", "--no-cpu-baseline",
                        "--no-extra-legs", "--no-h2d", "--no-lookup-profile"])
    args.score_dtype = dtype
    bench.run(args)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--dtypes", default="fp32,bf16,bf16x3")
    ap.add_argument("--timeout", type=float, default=600.0, help="seconds per child run")
    ap.add_argument("--out", default=None, help="also write the JSON result here")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a.child, a.steps, a.warmup)
        return
    dtypes = a.dtypes.split(",")
    runs = {d: [] for d in dtypes}
    loss = {}
    for r in range(a.rounds):
        order = dtypes if r % 2 == 0 else dtypes[::-1]
        for d in order:
            p = subprocess.run([sys.executable, __file__, "--child", d, "--steps", str(a.steps), "--warmup", str(a.warmup)],
                               cwd=ROOT, capture_output=True, text=True, timeout=a.timeout)
            if p.returncode != 0:
                sys.stderr.write(p.stdout[-4000:] + p.stderr[-4000:])
                raise SystemExit(f"score_dtype={d}, round {r}: exit status {p.returncode}")
            res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
            runs[d].append(res["ms_per_step"])
            loss[d] = res.get("final_loss")
            print(f"[round {r}] {d}: {res['ms_per_step']:.4f} ms/step", file=sys.stderr, flush=True)
    med = {d: statistics.median(v) for d, v in runs.items()}
    out = {"config": "configs[1]: B 8192, 1M + 1M rows, towers [128, 64] -> 64, dropout 0.1, mlp_dtype bf16, graphed, fused_sparse",
           "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds,
           "ms_per_step": runs, "median_ms": med, "final_loss": loss,
           "speedup_vs_fp32": {d: med["fp32"] / m for d, m in med.items()} if "fp32" in med else None}
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
