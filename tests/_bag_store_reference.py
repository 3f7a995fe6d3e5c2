"""A torch-only reference of the bag store's batch gather (tt_bag_store_gather / DeviceBagFeatureStore.gather): index,
repeat_interleave, cumulative sums.  Runs on whatever device its arguments live on; the tests run it on the host."""
import torch


def gather(dense, offsets, values, K, entities):
    """(dense [B, Din], lengths int64 [B*K], ids int64 [n]) of the entities `entities` (int64 [B]; an index outside the store is
    clamped into it): the sample-major bag wire format -- lengths[b*K + k] = the length of bag (b, k), ids = the samples' runs
    values[offsets[e*K] : offsets[(e+1)*K]] behind one another."""
    N = dense.shape[0]
    e = entities.to(torch.int64).clamp(0, N - 1)
    B = e.numel()
    slots = (e[:, None] * K + torch.arange(K, device=e.device)[None, :]).reshape(-1)
    lengths = offsets[slots + 1] - offsets[slots]
    first = offsets[e * K]
    run = offsets[(e + 1) * K] - first
    start = torch.cumsum(run, 0) - run
    b = torch.repeat_interleave(torch.arange(B, device=e.device), run)
    ids = values[first[b] + (torch.arange(b.numel(), device=e.device) - start[b])]
    return dense[e], lengths, ids


def gather_loop(dense, offsets, values, K, entities):
    """the same by a plain Python loop over samples, keys and ids"""
    N = dense.shape[0]
    rows, lengths, ids = [], [], []
    for e in entities.tolist():
        e = min(max(int(e), 0), N - 1)
        rows.append(dense[e])
        for k in range(K):
            lo, hi = int(offsets[e * K + k]), int(offsets[e * K + k + 1])
            lengths.append(hi - lo)
            ids += [int(values[p]) for p in range(lo, hi)]
    return torch.stack(rows), torch.tensor(lengths, dtype=torch.int64), torch.tensor(ids, dtype=torch.int64)
