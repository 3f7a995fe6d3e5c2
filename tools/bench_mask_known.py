#!/usr/bin/env python3
"""Cost of the known-pair mask (masked cells) on the captured training step, at BASELINE configs[1]'s shapes (B = 8192, the real
schema's 32 + 6 keys, E = 32, towers [128, 64] -> 64, bf16 score and MLP operands, sparse table gradients, T = 1).

    python tools/bench_mask_known.py [--entities 100000] [--pairs 200000] [--zipf 0 1.1] [--extras 0 1024] [--steps 50] [--reps 7]
                                     [--out profiles/mask_known_bench.json]

The worlds are the driver's (scripts/train.py): its default pair table (companies drawn uniformly: few shared bidders) and one whose
companies follow a Zipf law (--zipf A, the driver's --pair-zipf; 0 = uniform), where a few companies bid everywhere.  Per world and
M in --extras (0: none; otherwise M extras per batch, the first three quarters drawn from rows mined with the untrained task), two
loaders over the same pairs and seed -- one with mask_known, one without -- yield the same batches; a captured step of each
(GraphedTrainStep.step(batch), the plain-copy hand-over in both) runs the epoch's full batches, alternating block by block in ONE
process, medians of --reps blocks of --steps.  The cells are the loader's real ones: cells per batch (mean, maximum) are reported.
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
from jodalrob_twotower_amd.data_loader import DevicePairLoader, create_unified_bid_dataloaders  # noqa: E402
from jodalrob_twotower_amd.graph import GraphedTrainStep  # noqa: E402
from jodalrob_twotower_amd.hard_negatives import mine_hard_negatives  # noqa: E402
from jodalrob_twotower_amd.optim import FusedAdam  # noqa: E402

DEV = torch.device("cuda:0")


def _median(v):
    return sorted(v)[len(v) // 2]


def _world(args, zipf):
    real = synthetic.load_real_schema(ROOT / "jodalrob-twotower_amd" / "schema_real.json")
    rows = [synthetic.META_HEADER]
    for side in ("notice", "company"):
        rows += [f"{side},{c},text,Y,,,,0,,Y,Y,," for c in real[side]["pk_cols"]]
        rows += [f"{side},{c},numeric,Y,,,,0,,,,," for c in real[side]["numeric"]]
        rows += [f"{side},{c},text,Y,,Y,{v - 10},0,,,,," for c, v in zip(real[side]["categorical"], real[side]["vocab_sizes"])]
        rows += [f"{side},{c},text,Y,,N,,0,,,,," for c in real[side]["text"]]
    meta = Path(tempfile.mkdtemp(prefix="tt_mask_known_")) / "metadata.csv"
    meta.write_text("\n".join(rows) + "\n", encoding="utf-8")
    schema = tt.build_torchrec_schema_from_meta(notice_table="notice", company_table="company", pair_table="bid_two_tower",
                                                pair_notice_id_cols=["bidntceno", "bidntceord"], pair_company_id_cols=["bizno"],
                                                metadata_path=str(meta))
    source = synthetic.SyntheticSource(args.entities, args.entities, args.pairs, real["notice"]["vocab_sizes"], real["company"]["vocab_sizes"],
                                       pair_zipf_alpha=zipf if zipf > 0 else None)
    loader, _ = create_unified_bid_dataloaders(source, schema, batch_size=args.batch, test_split=0.2, shuffle_seed=42, test_mode=True,
                                               pair_limit=args.pairs, device=DEV)
    return meta, schema, loader


def _task(meta, schema):
    torch.manual_seed(1)
    task = tt.create_two_tower_train_task(schema.notice.categorical, schema.company.categorical, metadata_path=str(meta),
                                          categorical_embedding_dim=32, notice_dense_input_dim=256, company_dense_input_dim=128,
                                          tower_hidden_dims=[128, 64], final_embedding_dim=64, dropout_rate=0.2, temperature=1.0, device=DEV,
                                          embedding_grad="sparse", score_dtype="bf16", mlp_dtype="bf16")
    task.train()
    task._pair_check_done = True
    return task, FusedAdam.for_task(task, lr=1e-3, weight_decay=1e-5)


def case(args, meta, schema, base, M):
    pairs = base.pairs.cpu().numpy()
    kw = {}
    if M:
        task0, _ = _task(meta, schema)
        kw = dict(extra_negatives=M, mined=mine_hard_negatives(task0, base.notice, base.company, base.pairs, k=64, per_notice=8), hard_fraction=0.75)
        del task0
    runs, counts = {}, None
    for mode in ("plain", "cells"):
        loader = DevicePairLoader(base.notice, base.company, pairs, args.batch, shuffle=True, seed=42, mask_known=mode == "cells", **kw)
        bs = [b for b in loader if b["notice"]["dense"].shape[0] == args.batch][:8]
        if mode == "cells":
            counts = [int(b["masked_cells"].shape[0]) for b in bs]
            extras = [int((b["masked_cells"][:, 1] >= args.batch).sum()) for b in bs]
        task, opt = _task(meta, schema)
        cap = {"cell_capacity": max(1024, 2 * loader.max_cells)} if mode == "cells" else {}
        runs[mode] = (GraphedTrainStep(task, opt, bs[0], warmup=3, return_metrics=False, **cap), bs)
    for gs, bs in runs.values():
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
    launches = {m: gs.library_launches for m, (gs, _) in runs.items()}
    for gs, _ in runs.values():
        gs.close()
    out = {"M": M, "batches_timed": len(counts), **{f"{m}_ms_per_step": _median(v) for m, v in t.items()},
           **{f"{m}_ms_per_step_all": v for m, v in t.items()}, "ratio": _median(t["cells"]) / _median(t["plain"]),
           "library_launches": launches, "cells_per_batch_mean": sum(counts) / len(counts), "cells_per_batch_max": max(counts),
           "cells_on_extras_per_batch_mean": sum(extras) / len(extras), "cell_capacity": cap.get("cell_capacity")}
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--entities", type=int, default=100_000)
    ap.add_argument("--pairs", type=int, default=200_000)
    ap.add_argument("--zipf", type=float, nargs="+", default=[0.0, 1.1],
                    help="per world: Zipf exponent of the pairs' companies (the driver's --pair-zipf); 0 = uniform, the driver's default")
    ap.add_argument("--extras", type=int, nargs="+", default=[0, 1024])
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "mask_known_bench.json"))
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0),
           "workload": "configs[1] shapes: B = %d, 32+6 real keys, E = 32, towers [128,64] -> 64, bf16, sparse, T = 1, dropout 0.2; the driver's "
                       "synthetic world: %d notices, %d companies, %d pairs (80 %% train)" % (args.batch, args.entities, args.entities, args.pairs),
           "cases": []}
    for z in args.zipf:
        meta, schema, base = _world(args, z)
        for M in args.extras:
            res["cases"].append({"companies": "Zipf(%g)" % z if z > 0 else "uniform", **case(args, meta, schema, base, M)})
        del base
        torch.cuda.empty_cache()
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
