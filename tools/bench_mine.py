"""Hard-negative mining: what the sweep's score ceiling costs, and how long one whole mining pass takes.

    python tools/bench_mine.py [--nq 8192] [--nc 1048576] [--d 64] [--k 64 256] [--dtypes bf16] [--exclude 16] [--reps 5]
                               [--entities 100000] [--pairs 200000] [--out profiles/mine_bench.json]

Sweep: per (dtype, k), four searches on the same queries and catalogue in one process, alternating rep by rep, best of --reps:
the plain search, the exclusion search (--exclude random rows per query: the parent code path mining would otherwise run), the
ceiling search with the same lists, and the ceiling search without lists.  Each query's ceiling is 0.95 times its score against the
row at rank 5 of its plain list (CatalogIndex.pair_scores) -- a positive that ranks high, as a trained one does -- so the ceiling
removes the handful of rows above it and the running threshold settles a little lower than in the plain search.  One JSON line
per case with the four times and the ratios ceil+excl / excl and ceil / plain.

Pass: a synthetic world as scripts/train.py builds it (--entities notices and companies, --pairs pairs, the real schema's
columns), an untrained bf16 task; mine_hard_negatives over the train pairs, timed once with the catalogue index built inside and
once with a ready index (k = 64, per_notice = 8, ceiling (0.95, 0)).
"""
from __future__ import annotations

import argparse
import json
import sys
import tempfile
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from bench_retrieve import _time, random_exclusions  # noqa: E402  (tools/ is this script's directory)


def sweep_rows(args, dev):
    from jodalrob_twotower_amd import ops
    from jodalrob_twotower_amd.retrieval import CatalogIndex
    g = torch.Generator(device=dev).manual_seed(0)
    nq, nc, d = args.nq, args.nc, args.d
    Q = torch.randn((nq, d), generator=g, device=dev)
    Q /= Q.norm(dim=1, keepdim=True)
    Cm = torch.randn((nc, d), generator=g, device=dev)
    Cm /= Cm.norm(dim=1, keepdim=True)
    out = []
    for dt in args.dtypes:
        index = CatalogIndex.from_embeddings(Cm, temperature=0.05, score_dtype=dt)
        bf16 = index.score_dtype == "bf16"
        q = ops.score_pack_bf16(Q, 1.0) if bf16 else Q
        ex = random_exclusions(nq, nc, args.exclude, g, dev)
        pos = index.search(Q, 10)[1][:, 5].contiguous()
        ceil = (0.95 * index.pair_scores(Q, pos)).contiguous()
        for k in args.k:
            ws = index._workspace(nq, k)
            run = lambda e, c: (lambda: ops._retrieve(q, nq, index.data, nc, d, k, index.inv_t, bf16, None, ws, e, None, c))
            forms = {"plain": run(None, None), "excl": run(ex, None), "ceil_excl": run(ex, ceil), "ceil": run(None, ceil)}
            ms = {name: [] for name in forms}
            for _ in range(args.reps):                                # alternating, so all see the same clocks and caches
                for name, fn in forms.items():
                    ms[name].append(_time(fn, 1)[0])
            vals, idx = index.search(Q, k, exclude=ex, max_score=ceil)
            plain_idx = index.search(Q, k)[1]
            row = {"nq": nq, "nc": nc, "d": d, "k": k, "dtype": dt, "exclude_L": args.exclude,
                   **{f"{name}_ms": round(min(v), 4) for name, v in ms.items()},
                   "ceil_excl_over_excl": round(min(ms["ceil_excl"]) / min(ms["excl"]), 4),
                   "ceil_over_plain": round(min(ms["ceil"]) / min(ms["plain"]), 4),
                   **{f"{name}_ms_all": [round(x, 4) for x in v] for name, v in ms.items()},
                   "rows_at_or_above_ceiling_returned": int((vals >= ceil[:, None]).sum()),
                   "slots_filled_frac": float((idx >= 0).float().mean()),
                   "slots_shared_with_plain_frac": float((idx[:, :, None] == plain_idx[:, None, :k]).any(2).float().mean())
                   if k <= 64 else None}
            print(json.dumps(row), flush=True)
            out.append(row)
        del index
        torch.cuda.empty_cache()
    return out


def pass_row(args, dev):
    import jodalrob_twotower_amd as tt
    from jodalrob_twotower_amd import synthetic
    from jodalrob_twotower_amd.data_loader import create_unified_bid_dataloaders
    from jodalrob_twotower_amd.hard_negatives import mine_hard_negatives
    from jodalrob_twotower_amd.retrieval import CatalogIndex
    real = synthetic.load_real_schema(ROOT / "jodalrob-twotower_amd" / "schema_real.json")
    meta_rows = [synthetic.META_HEADER]
    for side in ("notice", "company"):
        for c in real[side]["pk_cols"]:
            meta_rows.append(f"{side},{c},text,Y,,,,0,,Y,Y,,")
        for c in real[side]["numeric"]:
            meta_rows.append(f"{side},{c},numeric,Y,,,,0,,,,,")
        for c, v in zip(real[side]["categorical"], real[side]["vocab_sizes"]):
            meta_rows.append(f"{side},{c},text,Y,,Y,{v - 10},0,,,,,")
        for c in real[side]["text"]:
            meta_rows.append(f"{side},{c},text,Y,,N,,0,,,,,")
    meta = Path(tempfile.mkdtemp(prefix="tt_mine_")) / "metadata.csv"
    meta.write_text("\n".join(meta_rows) + "\n", encoding="utf-8")
    schema = tt.build_torchrec_schema_from_meta(notice_table="notice", company_table="company", pair_table="bid_two_tower",
                                                pair_notice_id_cols=["bidntceno", "bidntceord"], pair_company_id_cols=["bizno"],
                                                metadata_path=str(meta))
    source = synthetic.SyntheticSource(args.entities, args.entities, args.pairs, real["notice"]["vocab_sizes"], real["company"]["vocab_sizes"])
    loader, _ = create_unified_bid_dataloaders(source, schema, batch_size=8192, test_split=0.2, shuffle_seed=42, test_mode=True,
                                               pair_limit=args.pairs, device=dev)
    task = tt.create_two_tower_train_task(schema.notice.categorical, schema.company.categorical, metadata_path=str(meta),
                                          categorical_embedding_dim=32, notice_dense_input_dim=256, company_dense_input_dim=128,
                                          tower_hidden_dims=[128, 64], final_embedding_dim=64, dropout_rate=0.1, temperature=1.0,
                                          loss_type="cross_entropy", device=dev, embedding_grad="sparse", score_dtype="bf16", mlp_dtype="bf16")
    kw = dict(k=64, per_notice=8, ceiling=(0.95, 0.0))

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return r, (time.perf_counter() - t) * 1e3

    mine_hard_negatives(task, loader.notice, loader.company, loader.pairs, **kw)              # warm: allocations, first launches
    mined, whole = timed(lambda: mine_hard_negatives(task, loader.notice, loader.company, loader.pairs, **kw))
    index, build = timed(lambda: CatalogIndex.from_store(task, loader.company))
    _, search = timed(lambda: mine_hard_negatives(task, loader.notice, loader.company, loader.pairs, index=index, **kw))
    t = mined.table
    row = {"pass": "mine_hard_negatives", "notices": len(loader.notice), "companies": len(loader.company), "pairs": int(loader.pairs.shape[0]),
           "notices_with_pairs": int(torch.unique(loader.pairs[:, 0]).numel()), **{k: list(v) if isinstance(v, tuple) else v for k, v in kw.items()},
           "whole_pass_ms": round(whole, 2), "index_build_ms": round(build, 2), "pass_with_ready_index_ms": round(search, 2),
           "slots_filled_frac_of_mined_notices": float((t[t[:, 0] >= 0] >= 0).float().mean()) if bool((t[:, 0] >= 0).any()) else 0.0}
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nq", type=int, default=8192)
    ap.add_argument("--nc", type=int, default=1 << 20)
    ap.add_argument("--d", type=int, default=64)
    ap.add_argument("--k", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--dtypes", nargs="+", default=["bf16"])
    ap.add_argument("--exclude", type=int, default=16, help="exclusion list length per query")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--entities", type=int, default=100_000)
    ap.add_argument("--pairs", type=int, default=200_000)
    ap.add_argument("--no-pass", action="store_true", help="the sweep comparison only")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    def write(rows):
        if args.out:
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            Path(args.out).write_text(json.dumps({"device": torch.cuda.get_device_name(0), "rows": rows}, indent=1) + "\n")

    rows = sweep_rows(args, dev)
    write(rows)
    if not args.no_pass:
        rows.append(pass_row(args, dev))
        write(rows)


if __name__ == "__main__":
    main()
