"""A torch-only reference of the WEIGHTED bag store's batch gather (tt_bag_store_gather_w / DeviceBagFeatureStore.gather on a store
with weights): plain indexing, repeat_interleave and cumulative sums.  Runs on whatever device its arguments live on; the tests run
it on the host.  The weights are a copy, so the tests compare them through bits(): NaN payloads and -0.0 count."""
import torch


def bits(w):
    """f32 -> its int32 bit patterns (what the weighted gather must reproduce)"""
    return w.contiguous().view(torch.int32)


def gather(dense, offsets, values, weights, K, entities):
    """(dense [B, Din], lengths int64 [B*K], ids int64 [n], weights f32 [n]) of the entities `entities` (int64 [B]; an index outside
    the store is clamped into it): the sample-major bag wire format -- lengths[b*K + k] = the length of bag (b, k), ids / weights =
    the samples' runs values / weights[offsets[e*K] : offsets[(e+1)*K]] behind one another."""
    N = dense.shape[0]
    e = entities.to(torch.int64).clamp(0, N - 1)
    B = e.numel()
    slots = (e[:, None] * K + torch.arange(K, device=e.device)[None, :]).reshape(-1)
    lengths = offsets[slots + 1] - offsets[slots]
    first = offsets[e * K]
    run = offsets[(e + 1) * K] - first
    start = torch.cumsum(run, 0) - run
    b = torch.repeat_interleave(torch.arange(B, device=e.device), run)
    src = first[b] + (torch.arange(b.numel(), device=e.device) - start[b])
    return dense[e], lengths, values[src], bits(weights)[src].view(torch.float32)


def gather_loop(dense, offsets, values, weights, K, entities):
    """the same by a plain Python loop over samples, keys and ids"""
    N = dense.shape[0]
    wb = bits(weights)
    rows, lengths, ids, w = [], [], [], []
    for e in entities.tolist():
        e = min(max(int(e), 0), N - 1)
        rows.append(dense[e])
        for k in range(K):
            lo, hi = int(offsets[e * K + k]), int(offsets[e * K + k + 1])
            lengths.append(hi - lo)
            ids += [int(values[p]) for p in range(lo, hi)]
            w += [int(wb[p]) for p in range(lo, hi)]
    return (torch.stack(rows), torch.tensor(lengths, dtype=torch.int64), torch.tensor(ids, dtype=torch.int64),
            torch.tensor(w, dtype=torch.int32).view(torch.float32))
