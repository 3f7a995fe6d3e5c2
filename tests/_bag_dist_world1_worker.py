"""Worker of test_gpu_bag_exchange.py::test_sharded_bag_step_world1_subprocess (not collected by pytest: no test_ prefix).

The row-wise sharded BAG-MODE step at RCCL world 1 (one GPU process, its own process group on a free port, the ordinary teardown
of _dist_world1_worker.py), B = 64 on the manifest's wide_b40 schema, two models: the company tower pooled (mean) with the notice
tower riding along as length-one bags, then both towers pooled (sum, per-id weights on both KJTs).

  A. `exact` exchange, dense table gradients, against the UNSHARDED bag-mode task from the same state: equal loss, every dense
     gradient torch.equal, shard gradient torch.equal to the fused table gradient.
  B. `padded` against `exact`, row-sparse FusedAdam, one warm-up step + four steps: equal losses, final full_state_dict within
     rtol 1e-6 / atol 1e-7 (_dist_world1_worker.py's own); an eval-mode step of the sharded task == the unsharded one's loss.

Why the bags have power-of-two lengths and the weights lie in {0.5, 1, 2}: the unsharded gradient adds a position's contribution
with ONE fused multiply-add, acc = fma(c * w, d, acc); the exact exchange forms the contribution (c * w) * d where the position
lives, rounds it to f32 for the wire, and the owner adds it.  The two agree bit for bit exactly when the product is exact in f32,
which power-of-two coefficients make it; in general they differ by one rounding per contribution (the random-normal test of
test_gpu_bag_exchange.py bounds that)."""
import json
import os
import sys
from pathlib import Path

import numpy as np
import torch
import torch.distributed as dist

ROOT = Path(__file__).resolve().parents[1]
for p in (ROOT, ROOT / "tests", ROOT / "oracle"):
    sys.path.insert(0, str(p))
import jodalrob_twotower_amd as tt  # noqa: E402
from jodalrob_twotower_amd.distributed import create_distributed_train_task  # noqa: E402
from jodalrob_twotower_amd.optim import FusedAdam  # noqa: E402
from params_init import init_state_numpy  # noqa: E402

DEV = "cuda:0"
GOLD = ROOT / "tests" / "golden"
B = 64


def bag_batch(cfg, seed, pooled, weighted):
    """pooled: the sides whose KJT carries ragged bags (lengths in {0, 1, 2, 4, 8}); the other side one id per key"""
    rng = np.random.default_rng(seed)
    out = {}
    for side, keys, vocab, din in (("notice", cfg["keys_n"], cfg["vocab_n"], cfg["din_n"]), ("company", cfg["keys_c"], cfg["vocab_c"], cfg["din_c"])):
        K = len(keys)
        dense = torch.from_numpy(rng.standard_normal((B, din)).astype(np.float32)).to(DEV)
        if side in pooled:
            lengths = rng.choice([0, 1, 2, 4, 8], B * K).astype(np.int64)
            ids = np.concatenate([rng.integers(-1, vocab[s % K] + 1, int(n)) for s, n in enumerate(lengths)] + [np.zeros(0, np.int64)])
            w = torch.from_numpy(rng.choice([0.5, 1.0, 2.0], ids.size).astype(np.float32)) if weighted else None
            kjt = tt.build_bag_kjt(keys, values=torch.from_numpy(ids.astype(np.int64)), lengths=torch.from_numpy(lengths), weights=w)
        else:
            kjt = tt.build_batch_kjt(torch.from_numpy(np.stack([rng.integers(-1, v + 1, B) for v in vocab], axis=1)), keys)
        out[side] = {"dense": dense, "kjt": kjt.to(DEV)}
    return out


def run_model(cfg, pooling, pooled, weighted):
    common = dict(metadata_path=str(GOLD / "synthetic_metadata.csv"), categorical_embedding_dim=cfg["E"], notice_dense_input_dim=cfg["din_n"],
                  company_dense_input_dim=cfg["din_c"], tower_hidden_dims=list(cfg["hidden"]), final_embedding_dim=cfg["D"], dropout_rate=0.0,
                  temperature=cfg["T"], device=DEV, categorical_pooling=pooling)
    batches = [bag_batch(cfg, 4100 + i, pooled, weighted) for i in range(5)]
    # ---- A: exact exchange, dense table gradients, against the unsharded bag-mode task
    single = tt.create_two_tower_train_task(cfg["keys_n"], cfg["keys_c"], embedding_grad="dense", **common)
    state = init_state_numpy({k: tuple(v.shape) for k, v in single.state_dict().items()}, 4242)
    single.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in state.items()})
    dtask = create_distributed_train_task(cfg["keys_n"], cfg["keys_c"], embedding_grad="dense", exchange="exact", **common)
    assert dtask.pooled_exchange
    dtask.load_full_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in state.items()})
    single.train(); dtask.train()
    r1, r2 = single(batches[0], return_metrics=True), dtask(batches[0], return_metrics=True)
    assert r1["loss"].item() == r2["loss"].item(), (r1["loss"].item(), r2["loss"].item())
    r1["loss"].backward(); r2["loss"].backward()
    g1 = {n: p.grad for n, p in single.named_parameters()}
    for n, p in dtask.named_parameters():
        if n != "embedding_shard":
            assert torch.equal(p.grad, g1[n]), n
    fused = torch.cat([g1[name] for name, _, _ in dtask.key_directory()])
    assert fused.abs().sum().item() > 0
    assert torch.equal(dtask.embedding_shard.grad[:fused.shape[0]], fused), float((dtask.embedding_shard.grad[:fused.shape[0]] - fused).abs().max())
    # ---- eval-mode forward (want_grad False) == the unsharded one's loss
    single.eval(); dtask.eval()
    with torch.no_grad():
        e1, e2 = single(batches[1], return_metrics=True)["loss"].item(), dtask(batches[1], return_metrics=True)["loss"].item()
    assert e1 == e2, (e1, e2)
    del single, dtask
    # ---- B: padded against exact, row-sparse FusedAdam
    finals = {}
    for mode in ("exact", "padded"):
        t = create_distributed_train_task(cfg["keys_n"], cfg["keys_c"], embedding_grad="sparse", exchange=mode, **common)
        t.load_full_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in state.items()})
        t.train()
        o = FusedAdam.for_task(t, lr=1e-2, weight_decay=1e-5)
        losses = []
        for i, bt in enumerate(batches):                                  # batches[0]: the warm-up step (calibrates the bucket capacity)
            o.zero_grad()
            r = t(bt, return_metrics=True)
            r["loss"].backward()
            o.step()
            if i:
                losses.append(r["loss"].item())
        if mode == "padded":
            t.exchange.check_overflow()
        finals[mode] = (losses, {k: v.detach().cpu().numpy().copy() for k, v in t.full_state_dict().items()})
        del o, t
    assert finals["padded"][0] == finals["exact"][0], (finals["padded"][0], finals["exact"][0])
    moved = 0.0
    for k, v in finals["exact"][1].items():
        np.testing.assert_allclose(finals["padded"][1][k], v, rtol=1e-6, atol=1e-7, err_msg=k)
        if "embeddings" in k:
            moved += float(np.abs(v - state[k]).sum())
    assert moved > 0                                                       # the tables trained


def main():
    import socket
    sk = socket.socket(); sk.bind(("127.0.0.1", 0)); port = sk.getsockname()[1]; sk.close()
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)     # never the parent's rendezvous port
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device(DEV))
    cfg = dict(json.load(open(GOLD / "manifest.json"))["cases"]["wide_b40"])
    run_model(cfg, {"company": "mean"}, ("company",), False)
    print("[bag world1] company tower pooled (mean), notice tower riding along: ok", flush=True)
    run_model(cfg, "sum", ("notice", "company"), True)
    print("[bag world1] both towers pooled (sum, weighted): ok", flush=True)
    import gc
    gc.collect()
    torch.cuda.synchronize()
    dist.destroy_process_group()
    print("BAG_DIST_WORLD1_OK", flush=True)


if __name__ == "__main__":
    try:
        main()
    except BaseException:
        import traceback
        traceback.print_exc()
        sys.stdout.flush(); sys.stderr.flush()
        os._exit(1)
    sys.stdout.flush()
