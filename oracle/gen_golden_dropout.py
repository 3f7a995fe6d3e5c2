#!/usr/bin/env python3
"""Golden vectors for a training step with dropout on (base_tower.py:88-93: Linear, ReLU, BatchNorm1d, Dropout per hidden
block).  Same harness as gen_golden.py (the reference's own modules run on CPU with numpy-generated parameters and inputs);
writes tests/golden/case_dropout_train.npz and dropout_cases.json and touches no other fixture.  TEST INFRASTRUCTURE ONLY;
runs only where /root/reference exists.

The reference draws its masks from torch's generator; forward hooks on every nn.Dropout record them as output != 0 (the
hook asserts that no input element is exactly 0, so a zero output means a dropped element), and the oracle is then fed the
recorded masks.  Also frozen: inputs, loss, metrics, both towers' embeddings (hooks on the towers: a second forward would
draw new masks), every gradient and the BatchNorm running statistics after the step.

Usage:  python oracle/gen_golden_dropout.py
"""
from __future__ import annotations

import json
import os
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "oracle"))
import gen_golden as G  # noqa: E402
from params_init import init_state_numpy, synth_batch_numpy  # noqa: E402

CASE = "dropout_train"
CFG = dict(E=4, din_n=10, din_c=5, hidden=(16, 12, 8), D=6, T=0.5, B=24, seed=900, p=0.3)


def main():
    assert G.REF.is_dir(), f"reference not found at {G.REF}"
    G._install_standins()
    sys.path.insert(0, str(G.REF))
    os.chdir(G.REF)
    with G.quiet():
        from src.towers.two_tower_train_task import create_two_tower_train_task
        from src.towers.pairs.unified_bid_data_loader import _build_batch_kjt
    torch.manual_seed(0)
    torch.set_num_threads(4)
    syn = json.loads((G.GOLD / "schema_synthetic.json").read_text())
    kn, kc = syn["notice"]["categorical"], syn["company"]["categorical"]
    vn, vc = syn["notice"]["vocab_sizes"], syn["company"]["vocab_sizes"]
    c = CFG
    with G.quiet():
        task = create_two_tower_train_task(kn, kc, metadata_path=str(G.GOLD / "synthetic_metadata.csv"), categorical_embedding_dim=c["E"],
                                           notice_dense_input_dim=c["din_n"], company_dense_input_dim=c["din_c"],
                                           tower_hidden_dims=list(c["hidden"]), final_embedding_dim=c["D"], dropout_rate=c["p"],
                                           temperature=c["T"], loss_type="cross_entropy", device=torch.device("cpu"))
    shapes = {k: tuple(v.shape) for k, v in task.state_dict().items()}
    state = init_state_numpy(shapes, c["seed"])
    G.load_numpy_state(task, state)
    b = synth_batch_numpy(c["B"], vn, vc, c["din_n"], c["din_c"], c["seed"] + 1, oob=True)

    out = {"in." + k: v for k, v in b.items()}
    out.update({"state." + k: np.asarray(v) for k, v in state.items()})
    hooks, n_drop = [], 0
    for name, mod in task.named_modules():
        if isinstance(mod, torch.nn.Dropout):
            # "two_tower_model.notice_tower.mlp.3" -> prefix "two_tower_model.notice_tower.", block 3 // 4 = 0
            prefix, idx = name.split("mlp.")
            key = f"mask.{prefix}{int(idx) // 4}"

            def rec(m, inp, outp, key=key):
                x = inp[0].detach()
                assert not (x == 0).any(), f"{key}: an input element is exactly 0 (its mask bit cannot be read off the output)"
                keep = (outp.detach() != 0)
                torch.testing.assert_close(outp.detach()[keep], x[keep] / (1 - m.p), rtol=1e-6, atol=0)
                out[key] = keep.numpy().copy()
            hooks.append(mod.register_forward_hook(rec))
            n_drop += 1
    for side in ("notice", "company"):
        hooks.append(getattr(task.two_tower_model, f"{side}_tower").register_forward_hook(
            lambda m, inp, outp, side=side: out.__setitem__(f"out.{side}_emb", outp.detach().numpy().copy())))
    task.train(True)
    with G.quiet():
        res = task(G.make_batch(_build_batch_kjt, kn, kc, b), return_metrics=True)
    res["loss"].backward()
    for h in hooks:
        h.remove()
    assert n_drop == 2 * (len(c["hidden"]) - 1) and sum(k.startswith("mask.") for k in out) == n_drop
    for n, p in task.named_parameters():
        out["grad." + n] = p.grad.detach().numpy().copy()
    out["sim"] = res["similarity_matrix"].detach().numpy().copy()
    for k in ("loss", "accuracy", "positive_similarity_mean", "negative_similarity_mean", "similarity_gap"):
        out["out." + k] = np.asarray(res[k].detach().numpy())
    out.update({"state_after." + k: v for k, v in G.sd_to_np(task.state_dict()).items() if "running" in k or "num_batches" in k})
    np.savez_compressed(G.GOLD / f"case_{CASE}.npz", **out)
    kept = [float(v.mean()) for k, v in out.items() if k.startswith("mask.")]
    manifest = {"torch": torch.__version__, "cases": {CASE: {**{k: (list(v) if isinstance(v, tuple) else v) for k, v in c.items()},
                                                             "keys_n": kn, "keys_c": kc, "vocab_n": vn, "vocab_c": vc,
                                                             "loss": float(res["loss"].detach())}}}
    (G.GOLD / "dropout_cases.json").write_text(json.dumps(manifest, indent=1))
    print(CASE, res["loss"].item(), "kept fractions", [round(x, 3) for x in kept])


if __name__ == "__main__":
    main()
