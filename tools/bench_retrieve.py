"""Catalogue-wide top-k retrieval: the fused score + select kernels (tt_retrieve_topk_bf16 / _f32) against chunked
torch.mm + torch.topk on the same inputs.

    python tools/bench_retrieve.py [--nq 8192] [--nc 65536 1048576] [--d 64 256] [--k 10 64] [--dtypes bf16 fp32]
                                   [--reps 3] [--out profiles/retrieve_bench.json] [--exclude 0 16 256]
                                   [--filter 1 4 --eligible 1.0 0.1]

One JSON line per case: kernel ms per search and scores/s, the MFMA fraction of 2.5 PF dense bf16 (2 nQ nC D flops), the
catalogue read rate (bytes of the catalogue operand per search) against 8 TB/s, and the baseline's ms and how many rows'
index sets agree with the kernel's.  The baseline keeps at most 1 GiB of f32 scores alive per chunk (bf16: torch.mm of the two
bf16 images, bf16 scores; fp32: f32 scores), takes the chunk's top-k and merges it into the running top-k.  --k takes every k the
index does (1 .. 512; k > 64 runs the sweep's large-k form), and the baseline runs for each of them.

--exclude L [L ...] (no baseline then): per case and L, every query gets L random distinct catalogue rows as its exclusion
list, and the exclusion search (tt_excl_retrieve_topk_*) is timed against the plain search in the same process, the two
alternating rep by rep; one JSON line per (case, L) with both times and their ratio.

--filter W [W ...] with --eligible P [P ...] (no baseline then): per case, W and P, every catalogue row gets W random tag words
whose last word has each bit set with probability P, and query q requires bit q % 32 of that word, so a share P of the rows is
eligible per query.  The filtered search (tt_filt_retrieve_topk_*) is timed against the plain search in the same process, the
two alternating, best of --reps (use 5); one JSON line per (case, W, P) with both times and their ratio.
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

PEAK_BF16 = 2.5e15
PEAK_HBM = 8.0e12


def _time(fn, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return min(ms), sum(ms) / len(ms)


def baseline(Q, Cm, k, inv_t, bf16):
    nQ, nC = Q.shape[0], Cm.shape[0]
    chunk = max(k, min(nC, (1 << 28) // nQ))                   # <= 1 GiB of f32 scores
    q = Q.to(torch.bfloat16) if bf16 else Q
    best_v = best_i = None
    for s in range(0, nC, chunk):
        c = Cm[s:s + chunk]
        S = (q @ (c * inv_t).to(torch.bfloat16).T).float() if bf16 else (q @ c.T) * inv_t
        v, i = torch.topk(S, min(k, S.shape[1]), dim=1)
        i = i + s
        if best_v is None:
            best_v, best_i = v, i
        else:
            v2, j = torch.topk(torch.cat([best_v, v], 1), k, dim=1)
            best_i = torch.gather(torch.cat([best_i, i], 1), 1, j)
            best_v = v2
    return best_v, best_i


def random_exclusions(nq, nc, L, g, dev):
    """L distinct rows per query, ascending: a sorted draw from [0, nc - L] plus 0 .. L-1."""
    off = torch.arange(nq + 1, dtype=torch.int64, device=dev) * L
    if L == 0:
        return off, torch.zeros(0, dtype=torch.int32, device=dev)
    r = torch.sort(torch.randint(0, nc - L + 1, (nq, L), generator=g, device=dev), dim=1).values
    r += torch.arange(L, device=dev)
    return off, r.reshape(-1).to(torch.int32).contiguous()


def exclude_rows(index, Q, k, nc, d, dt, args):
    from jodalrob_twotower_amd import ops
    dev = Q.device
    g = torch.Generator(device=dev).manual_seed(1)
    nq = Q.shape[0]
    ws = index._workspace(nq, k)
    q = ops.score_pack_bf16(Q, 1.0) if index.score_dtype == "bf16" else Q
    bf16 = index.score_dtype == "bf16"
    out = []
    for L in args.exclude:
        ex = random_exclusions(nq, nc, L, g, dev)

        def plain():
            ops._retrieve(q, nq, index.data, nc, d, k, index.inv_t, bf16, None, ws)

        def excl():
            ops._retrieve(q, nq, index.data, nc, d, k, index.inv_t, bf16, None, ws, ex)

        pm, xm = [], []
        for _ in range(args.reps):                               # alternating, so both see the same clocks and caches
            pm.append(_time(plain, 1)[0])
            xm.append(_time(excl, 1)[0])
        vals, idx = index.search(Q, k, exclude=ex)
        hit = 0
        if L:
            lists = ex[1].view(nq, L).long()
            hit = int((idx[:, :, None] == lists[:, None, :]).any(2).sum())
        row = {"nq": nq, "nc": nc, "d": d, "k": k, "dtype": dt, "exclude_L": L, "plain_ms": round(min(pm), 4),
               "excl_ms": round(min(xm), 4), "excl_over_plain": round(min(xm) / min(pm), 4),
               "plain_ms_all": [round(x, 4) for x in pm], "excl_ms_all": [round(x, 4) for x in xm],
               "excluded_rows_returned": hit}
        print(json.dumps(row), flush=True)
        out.append(row)
    return out


def filter_rows(index, Q, k, nc, d, dt, args):
    from jodalrob_twotower_amd import ops
    dev = Q.device
    g = torch.Generator(device=dev).manual_seed(2)
    nq = Q.shape[0]
    ws = index._workspace(nq, k)
    bf16 = index.score_dtype == "bf16"
    q = ops.score_pack_bf16(Q, 1.0) if bf16 else Q
    out = []
    for W in args.filter:
        for P in args.eligible:
            tags = torch.randint(-2 ** 31, 2 ** 31, (nc, W), generator=g, device=dev, dtype=torch.int64)
            last = torch.zeros(nc, dtype=torch.int64, device=dev)
            for b in range(32):
                last |= (torch.rand(nc, generator=g, device=dev) < P).long() << b
            tags[:, W - 1] = torch.where(last >= 2 ** 31, last - 2 ** 32, last)
            tags = tags.to(torch.int32).contiguous()
            bit = torch.arange(nq, device=dev) % 32
            need = torch.zeros((nq, W), dtype=torch.int64, device=dev)
            need[:, W - 1] = torch.where(bit == 31, torch.full_like(bit, -2 ** 31), 1 << bit)
            need = need.to(torch.int32).contiguous()
            filt = (tags, W, None, need)

            def plain():
                ops._retrieve(q, nq, index.data, nc, d, k, index.inv_t, bf16, None, ws)

            def filtered():
                ops._retrieve(q, nq, index.data, nc, d, k, index.inv_t, bf16, None, ws, None, filt)

            pm, fm = [], []
            for _ in range(args.reps):                           # alternating, so both see the same clocks and caches
                pm.append(_time(plain, 1)[0])
                fm.append(_time(filtered, 1)[0])
            vals, idx, _ = ops._retrieve(q, nq, index.data, nc, d, k, index.inv_t, bf16, None, ws, None, filt)
            got = tags[idx.clamp(min=0), W - 1]                   # [nq, k]: the returned rows' last tag word
            ineligible = int((((got >> bit[:, None]) & 1) == 0)[idx >= 0].sum())
            share = float(((tags[:, W - 1][None, :4096] >> bit[:64, None]) & 1).float().mean())
            row = {"nq": nq, "nc": nc, "d": d, "k": k, "dtype": dt, "filter_W": W, "eligible_P": P,
                   "eligible_share_measured": round(share, 4), "plain_ms": round(min(pm), 4), "filt_ms": round(min(fm), 4),
                   "filt_over_plain": round(min(fm) / min(pm), 4), "plain_ms_all": [round(x, 4) for x in pm],
                   "filt_ms_all": [round(x, 4) for x in fm], "ineligible_rows_returned": ineligible}
            print(json.dumps(row), flush=True)
            out.append(row)
            del tags, need
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nq", type=int, default=8192)
    ap.add_argument("--nc", type=int, nargs="+", default=[65536, 1 << 20])
    ap.add_argument("--d", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--k", type=int, nargs="+", default=[10, 64], help="1 .. 512 each (retrieval.MAX_K)")
    ap.add_argument("--dtypes", nargs="+", default=["bf16", "fp32"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--exclude", type=int, nargs="+", action="extend", default=None,
                    help="exclusion list lengths L to time against the plain search (repeatable)")
    ap.add_argument("--filter", type=int, nargs="+", default=None, help="tag words W (1 .. 4) to time against the plain search")
    ap.add_argument("--eligible", type=float, nargs="+", default=[1.0, 0.1], help="share of rows eligible per query (--filter)")
    args = ap.parse_args()

    from jodalrob_twotower_amd.retrieval import CatalogIndex
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    rows = []
    for nc in args.nc:
        for d in args.d:
            Q = torch.randn((args.nq, d), generator=g, device=dev)
            Q /= Q.norm(dim=1, keepdim=True)
            Cm = torch.randn((nc, d), generator=g, device=dev)
            Cm /= Cm.norm(dim=1, keepdim=True)
            for dt in args.dtypes:
                index = CatalogIndex.from_embeddings(Cm, temperature=0.05, score_dtype=dt)
                for k in args.k:
                    if args.filter is not None:
                        rows.extend(filter_rows(index, Q, k, nc, d, dt, args))
                        continue
                    if args.exclude is not None:
                        rows.extend(exclude_rows(index, Q, k, nc, d, dt, args))
                        continue
                    best, mean = _time(lambda: index.search(Q, k), args.reps)
                    vals, idx = index.search(Q, k)
                    flops = 2.0 * args.nq * nc * d
                    cat_bytes = nc * (2 * (32 if d <= 32 else 64 if d <= 64 else 128 if d <= 128 else 256) if dt == "bf16" else 4 * d)
                    row = {"nq": args.nq, "nc": nc, "d": d, "k": k, "dtype": dt, "ms": round(best, 4), "ms_mean": round(mean, 4),
                           "scores_per_s": args.nq * nc / (best * 1e-3),
                           "mfma_frac_of_2.5PF": flops / (best * 1e-3) / PEAK_BF16,
                           "catalog_read_frac_of_8TBs": cat_bytes / (best * 1e-3) / PEAK_HBM}
                    if not args.no_baseline:
                        bms, _ = _time(lambda: baseline(Q, Cm, k, index.inv_t, dt == "bf16"), max(1, args.reps - 1))
                        bv, bi = baseline(Q, Cm, k, index.inv_t, dt == "bf16")
                        same = (torch.sort(bi, 1).values == torch.sort(idx, 1).values).all(1)
                        row.update({"torch_ms": round(bms, 4), "speedup_vs_torch": bms / best,
                                    "index_sets_agree_frac": float(same.float().mean()),
                                    "max_abs_val_diff": float((bv - vals).abs().max())})
                        del bv, bi
                    print(json.dumps(row), flush=True)
                    rows.append(row)
                del index
                torch.cuda.empty_cache()
            del Q, Cm
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps({"device": torch.cuda.get_device_name(0), "rows": rows}, indent=1) + "\n")


if __name__ == "__main__":
    main()
