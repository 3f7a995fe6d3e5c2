#!/usr/bin/env python3
"""Graphed training step per table optimiser (Adam, row-wise Adagrad) at bench.py's single-GPU leg, in ALTERNATED runs:
round r runs every (rows, optimiser) once, each in a fresh process, so drift of the box is shared by both optimisers.
bench.py is not changed: a child process builds bench.py's arguments, wraps FusedAdam.for_task to pass table_optimizer,
runs bench.run and prints torch.cuda.max_memory_allocated() after it, and torch.cuda.memory_allocated() with the optimiser
(hence the task's parameters and the optimiser state) still alive: what stays resident for training.

    python tools/bench_table_optimizer.py --rounds 2 --steps 200 --warmup 50 [--rows 1m,100m] [--out FILE]
    python tools/bench_table_optimizer.py --profile --steps 100 --warmup 20 [--rows 1m,100m] [--out FILE]

--rows: 1m = configs[1] (1 M + 1 M rows); 100m = one GPU with --rows-notice 100000000 --rows-company 10000000.
--profile: one run per (rows, optimiser) under `rocprofv3 --kernel-trace --stats`, reporting the optimiser launch's
average time (fused_step_kernel<AdamRows, ...> / fused_step_kernel<AdagradRows, ...>) instead of the step time.
Prints one JSON line: per rows setting and optimiser the ms/step and pairs/s of every round, their medians, the peak memory."""
import argparse
import csv
import json
import re
import statistics
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
ROWS = {"1m": [], "100m": ["--rows-notice", "100000000", "--rows-company", "10000000"]}
OPTS = ("adam", "rowwise_adagrad")
LAUNCH = {"adam": r"fused_step_kernel<[^>]*AdamRows,", "rowwise_adagrad": r"fused_step_kernel<[^>]*AdagradRows,"}


def child(opt, rows, steps, warmup):
    sys.path.insert(0, str(ROOT))
    import torch
    import bench
    from jodalrob_twotower_amd.optim import FusedAdam
    args = bench.parse(["--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--no-cpu-baseline", "--no-extra-legs",
                        "--no-h2d", "--no-lookup-profile", *ROWS[rows]])
    plain = FusedAdam.for_task.__func__
    kept = []

    def for_task(cls, task, **kw):
        if opt != "adam":                                  # the towers keep bench.py's Adam hyper-parameters; the tables inherit them
            kw["table_optimizer"] = opt
        kept.append(plain(cls, task, **kw))
        return kept[-1]
    FusedAdam.for_task = classmethod(for_task)
    bench.run(args)
    torch.cuda.synchronize()
    print(json.dumps({"max_memory_allocated": torch.cuda.max_memory_allocated(), "memory_allocated": torch.cuda.memory_allocated()}),
          flush=True)


def _json_lines(text):
    return [json.loads(ln) for ln in text.splitlines() if ln.startswith("{")]


def launch_us(stats_csv: Path, pattern: str):
    for r in csv.DictReader(open(stats_csv)):
        if re.search(pattern, r["Name"]):
            return {"kernel": re.search(r"\w+_kernel<[^>]*>", r["Name"]).group(0), "calls": int(r["Calls"]), "avg_us": float(r["AverageNs"]) / 1e3,
                    "min_us": float(r["MinNs"]) / 1e3}
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--rows", default="1m,100m")
    ap.add_argument("--profile", action="store_true", help="optimiser-launch time under rocprofv3 --kernel-trace --stats")
    ap.add_argument("--timeout", type=float, default=900.0, help="seconds per child run")
    ap.add_argument("--out", default=None, help="also write the JSON result here")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--child-rows", default="1m", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a.child, a.child_rows, a.steps, a.warmup)
        return
    rows_list = a.rows.split(",")
    out = {"measured": True, "steps": a.steps, "warmup": a.warmup,
           "configs": {"1m": "configs[1]: B 8192, 1 M + 1 M rows, E 32, towers [128, 64] -> 64, graphed, fused_sparse",
                       "100m": "one GPU, 100 M + 10 M rows, otherwise configs[1]"}}
    for rows in rows_list:
        res = {o: {"ms_per_step": [], "pairs_per_s": [], "max_memory_allocated": [], "memory_allocated_after_run": []} for o in OPTS}
        rounds = 1 if a.profile else a.rounds
        for r in range(rounds):
            for o in (OPTS if r % 2 == 0 else OPTS[::-1]):
                cmd = [sys.executable, __file__, "--child", o, "--child-rows", rows, "--steps", str(a.steps), "--warmup", str(a.warmup)]
                tmp = None
                if a.profile:
                    tmp = Path(tempfile.mkdtemp(prefix="tabopt_prof_"))
                    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", str(tmp), "-o", "run", "--output-format", "csv", "--"] + cmd
                p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=a.timeout)
                if p.returncode != 0:
                    sys.stderr.write(p.stdout[-4000:] + p.stderr[-4000:])
                    raise SystemExit(f"{rows} {o}, round {r}: exit status {p.returncode}")
                lines = _json_lines(p.stdout)
                bl = [d for d in lines if "ms_per_step" in d][-1]
                mems = [d for d in lines if "max_memory_allocated" in d][-1]
                mem = mems["max_memory_allocated"]
                res[o]["ms_per_step"].append(bl["ms_per_step"])
                res[o]["pairs_per_s"].append(bl["value"])
                res[o]["max_memory_allocated"].append(mem)
                res[o]["memory_allocated_after_run"].append(mems["memory_allocated"])
                if a.profile:
                    stats = sorted(tmp.rglob("*kernel_stats.csv"))
                    res[o]["optimizer_launch"] = launch_us(stats[0], LAUNCH[o]) if stats else None
                print(f"[{rows} round {r}] {o}: {bl['ms_per_step']:.4f} ms/step, peak {mem / 2**30:.2f} GiB", file=sys.stderr, flush=True)
        for o in OPTS:
            res[o]["median_ms_per_step"] = statistics.median(res[o]["ms_per_step"])
            res[o]["median_pairs_per_s"] = statistics.median(res[o]["pairs_per_s"])
            res[o]["peak_memory_gib"] = max(res[o]["max_memory_allocated"]) / 2**30
            res[o]["allocated_after_run_gib"] = max(res[o]["memory_allocated_after_run"]) / 2**30
        res["step_time_ratio_rowwise_over_adam"] = res["rowwise_adagrad"]["median_ms_per_step"] / res["adam"]["median_ms_per_step"]
        out[rows] = res
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
