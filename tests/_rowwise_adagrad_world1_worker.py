"""Worker of test_gpu_rowwise_adagrad.py::test_sharded_world1_subprocess (not collected by pytest: no test_ prefix).

Row-wise Adagrad on the sharded store (world 1, exact and fixed-capacity exchange) == the unsharded store over 3 steps:
weights and accumulators to 1e-6; rows no step looked up keep a zero accumulator (the fixed-capacity exchange's pads,
ids >= table_rows, are skipped); a sharded run resumed from (full_state_dict, FusedAdam.state_dict()) continues bit for bit."""
import io
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
from params_init import init_state_numpy, synth_batch_numpy  # noqa: E402

DEV = "cuda:0"
GOLD = ROOT / "tests" / "golden"
KW = dict(table_optimizer="rowwise_adagrad", lr=1e-2, weight_decay=1e-5, table_lr=0.05, table_weight_decay=1e-4)


def main():
    import socket
    sk = socket.socket(); sk.bind(("127.0.0.1", 0)); port = sk.getsockname()[1]; sk.close()
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device(DEV))
    cfg = dict(json.load(open(GOLD / "manifest.json"))["cases"]["wide_b40"])
    cfg["B"] = 256
    common = dict(metadata_path=str(GOLD / "synthetic_metadata.csv"), categorical_embedding_dim=cfg["E"],
                  notice_dense_input_dim=cfg["din_n"], company_dense_input_dim=cfg["din_c"], tower_hidden_dims=list(cfg["hidden"]),
                  final_embedding_dim=cfg["D"], dropout_rate=0.0, temperature=cfg["T"], device=DEV, embedding_grad="sparse")

    def to_batch(b):
        return {"notice": {"dense": torch.from_numpy(b["notice_dense"]).to(DEV),
                           "kjt": tt.build_batch_kjt(torch.from_numpy(b["notice_ids"]), cfg["keys_n"]).to(DEV)},
                "company": {"dense": torch.from_numpy(b["company_dense"]).to(DEV),
                            "kjt": tt.build_batch_kjt(torch.from_numpy(b["company_ids"]), cfg["keys_c"]).to(DEV)}}

    batches = [to_batch(synth_batch_numpy(cfg["B"], cfg["vocab_n"], cfg["vocab_c"], cfg["din_n"], cfg["din_c"], 820 + i, oob=True))
               for i in range(4)]

    def run(task, opt, bs):
        task.train()
        for b in bs:
            opt.zero_grad()
            task(b).backward()
            opt.step()

    single = tt.create_two_tower_train_task(cfg["keys_n"], cfg["keys_c"], **common)
    state = {k: torch.from_numpy(np.asarray(v))
             for k, v in init_state_numpy({k: tuple(v.shape) for k, v in single.state_dict().items()}, 821).items()}
    single.load_state_dict(state)
    sopt = FusedAdam.for_task(single, **KW)
    run(single, sopt, batches[:3])
    sparams = dict(single.named_parameters())
    ref = {k: v.detach().cpu().numpy() for k, v in single.state_dict().items()}
    for exchange in ("exact", "padded"):
        t = create_distributed_train_task(cfg["keys_n"], cfg["keys_c"], exchange=exchange, **common)
        t.load_full_state_dict(state)
        opt = FusedAdam.for_task(t, **KW)
        run(t, opt, batches[:3])
        for k, v in t.full_state_dict().items():
            np.testing.assert_allclose(v.detach().cpu().numpy(), ref[k], rtol=1e-6, atol=1e-7, err_msg=f"{exchange}:{k}")
        acc = opt.state[t.embedding_shard]["sum"]
        assert tuple(acc.shape) == (t.embedding_shard.shape[0],)
        acc = acc.cpu().numpy()
        n = 0
        for name, base, v in t.key_directory():
            want = sopt.state[sparams[name]]["sum"].cpu().numpy()
            np.testing.assert_allclose(acc[base:base + v], want, rtol=1e-6, atol=1e-12, err_msg=f"{exchange}:{name}")
            assert np.array_equal(acc[base:base + v] == 0, want == 0), f"{exchange}:{name}"
            n = base + v
        assert not acc[n:].any(), exchange                                  # rows past the table: never written
        # resume from a checkpoint: continues bit for bit
        buf = io.BytesIO()
        torch.save({"model": t.full_state_dict(), "optim": opt.state_dict()}, buf)
        buf.seek(0)
        ck = torch.load(buf, weights_only=False)
        t2 = create_distributed_train_task(cfg["keys_n"], cfg["keys_c"], exchange=exchange, **common)
        t2.load_full_state_dict(ck["model"])
        opt2 = FusedAdam.for_task(t2, **KW)
        opt2.load_state_dict(ck["optim"])
        run(t, opt, batches[3:])
        run(t2, opt2, batches[3:])
        assert torch.equal(t.embedding_shard, t2.embedding_shard), exchange
        assert torch.equal(opt.state[t.embedding_shard]["sum"], opt2.state[t2.embedding_shard]["sum"]), exchange
        for (k, a), (_, b) in zip(t.named_parameters(), t2.named_parameters()):
            assert torch.equal(a, b), (exchange, k)
        del t, t2, opt, opt2
    torch.cuda.synchronize()
    dist.destroy_process_group()
    print("ROWWISE_WORLD1_OK", flush=True)


if __name__ == "__main__":
    main()
