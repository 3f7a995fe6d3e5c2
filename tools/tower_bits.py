#!/usr/bin/env python3
"""The bits of the tower passes: for a fixed list of tiny problems, one line per case -- the case id and, per tower, the SHA-256 of
what tt_towers_mlp_fwd / _bwd (or tt_tower_mlp_*) wrote.  tests/golden/tower_bits.json holds the output of the build that last
changed the arithmetic on purpose; tests/test_gpu_tower_bits.py recomputes the digests and compares case by case.

    python tools/tower_bits.py                                   # the lines
    python tools/tower_bits.py --out FILE --commit ID            # the JSON file (header: commit, ROCm, device)

Every case runs towers.run_towers and, in training mode, a backward on seeded random d_emb.  Hashed per tower, in this order: the
unit rows, the packed score operand images (every tower emits them: pack_for_score), every dense gradient in dense_parameters()
order, the embedding columns d_x[:, h0:] (read through towers._DEBUG_KEEP; the projection's columns are not materialised on the
one-launch first-block backward), and each block's BatchNorm running_mean / running_var / num_batches_tracked.  State, batch and
d_emb come from numpy generators (oracle/params_init.py), so the digests depend on the library alone.

The widths are rows of tests/test_gpu_tower_parity.CASES, B cut to the smallest batch the path takes that still has a ragged last
64-row chunk (65, 130, 300) or to the predicate's own minimum (64 for the one-launch first-block backward, 2 and 1 where the row
says so).  The paths of csrc/tt_tower.hip they reach:
  front/...        one-launch front + narrow tail, B = 65 and B = 2; front-back: + the one-launch first-block backward at B = 64
  tail/...         narrow tail behind the separate GEMMs: split-K slabs finished by tail_head_kernel (B = 128), direct (B = 300),
                   three hidden blocks
  wide/...         wide tail (H 65 / D 100 / B 63, H 256 / D 128 / B 2), wide tail + first-block backward (B = 64)
  general/...      separate kernels (H 300 / D 130 / B 128)
  nohidden/...     projection + output Linear alone, bf16 and fp32
  fp32/2blk, eval/B1, dropout/narrow, dropout/wide
  solo/...         ONE tower (tt_tower_mlp_fwd / _bwd);  mixedB/...  two towers of different B (towers.py's per-tower calls)
  sync/...         the SyncBN two-phase pass with a one-rank communicator, dropout on, B = 130: narrow tail behind the front and
                   behind the separate GEMMs, wide tail, separate kernels
A case that names the first-block backward must take fewer launches than with tower_unfused_back, or its digest is refused.
The rider and hosted-score-backward variants need a captured step: tests/test_gpu_bn_finish_rider.py, test_gpu_score_tail_fused.py,
test_gpu_score_bwd_bits.py."""
import argparse
import hashlib
import json
import sys
import tempfile
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
for p in (ROOT, ROOT / "oracle"):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))

DEV = "cuda:0"
SEEDS = (1234567, 7654321)       # dropout seeds (notice, company)


def _c(name, mlp, hidden, D, B, E=32, keys=(3, 1), din=(64, 128), p=0.0, mode="train", back=False, sync=False):
    """hidden lists the projection width first; keys / din: (notice, company); B: one batch size or (notice, company)"""
    return dict(name=name, mlp=mlp, hidden=list(hidden), D=D, B=B, E=E, keys=keys, din=din, p=p, mode=mode, back=back, sync=sync)


CASES = [
    _c("front/h32-H17-D33-B65", "bf16", [32, 17], 33, 65),
    _c("front/h32-H1-D64-B2", "bf16", [32, 1], 64, 2, din=(64, 64)),
    _c("front-back/h128-H64-D33-B64", "bf16", [128, 64], 33, 64, keys=(4, 2), din=(256, 128), back=True),
    _c("tail/splitk-B128", "bf16", [48, 64], 32, 128, keys=(32, 20), din=(64, 64)),
    _c("tail/h48-din100-37-B300", "bf16", [48, 40], 33, 300, E=8, keys=(3, 2), din=(100, 37)),
    _c("tail/3blk-odd-B300", "bf16", [24, 33, 65, 31], 64, 300, E=8, keys=(2, 3), din=(50, 64)),
    _c("wide/H65-D100-B63", "bf16", [64, 65], 100, 63, keys=(2, 1)),
    _c("wide/H256-D128-B2", "bf16", [128, 256], 128, 2, keys=(2, 1)),
    _c("wide-back/h64-H256-D64-B64", "bf16", [64, 256], 64, 64, keys=(2, 4), din=(128, 64), back=True),
    _c("general/H300-D130-B128", "bf16", [64, 300], 130, 128, E=8, keys=(3, 2), din=(100, 64)),
    _c("nohidden/bf16-h37-D70-B65", "bf16", [37], 70, 65, E=6, keys=(3, 2), din=(37, 64)),
    _c("nohidden/fp32-h37-D70-B65", "fp32", [37], 70, 65, E=6, keys=(3, 2), din=(37, 64)),
    _c("fp32/2blk-B65", "fp32", [33, 17, 40], 9, 65, E=6, keys=(3, 2), din=(37, 20)),
    _c("eval/bf16-B1", "bf16", [64, 100], 70, 1, keys=(2, 1), mode="eval"),
    _c("dropout/narrow-B130", "bf16", [48, 40], 33, 130, E=8, keys=(3, 2), din=(100, 37), p=0.2),
    _c("dropout/wide-2blk-B130", "bf16", [40, 70, 129], 100, 130, E=6, keys=(3, 2), din=(37, 64), p=0.2),
    _c("solo/front-h32-H17-D33-B65", "bf16", [32, 17], 33, (65, 0)),
    _c("solo/general-H300-D130-B128", "bf16", [64, 300], 130, (0, 128), E=8, keys=(3, 2), din=(100, 64), p=0.2),
    _c("mixedB/front-h32-H17-D33-B65-B40", "bf16", [32, 17], 33, (65, 40), p=0.2),
    _c("sync/front-h32-H17-D33-B130", "bf16", [32, 17], 33, 130, p=0.2, sync=True),
    _c("sync/tail-h48-din100-37-B130", "bf16", [48, 40], 33, 130, E=8, keys=(3, 2), din=(100, 37), p=0.2, sync=True),
    _c("sync/wide-H65-D100-B130", "bf16", [64, 65], 100, 130, keys=(2, 1), p=0.2, sync=True),
    _c("sync/general-H300-D130-B130", "bf16", [64, 300], 130, 130, E=8, keys=(3, 2), din=(100, 64), p=0.2, sync=True),
    _c("sync/fp32-h33-H40-D9-B130", "fp32", [33, 40], 9, 130, E=6, keys=(3, 2), din=(37, 20), p=0.2, sync=True),
]


class Solo:
    """a one-rank communicator: the all-gather hands back the rank's own statistics"""
    world, rank = 1, 0

    def all_gather(self, t):
        return t.clone()


def _run(tt, TW, c, tmp, lib):
    from jodalrob_twotower_amd import synthetic
    from params_init import init_state_numpy, synth_batch_numpy
    kn, kc = [f"n{i}" for i in range(c["keys"][0])], [f"c{i}" for i in range(c["keys"][1])]
    vn, vc = [20 + 3 * i for i in range(len(kn))], [17 + 5 * i for i in range(len(kc))]
    meta = synthetic.write_metadata(Path(tmp) / "m.csv", {"notice": dict(zip(kn, vn)), "company": dict(zip(kc, vc))})
    task = tt.create_two_tower_train_task(kn, kc, metadata_path=str(meta), categorical_embedding_dim=c["E"], notice_dense_input_dim=c["din"][0],
                                          company_dense_input_dim=c["din"][1], tower_hidden_dims=c["hidden"], final_embedding_dim=c["D"],
                                          dropout_rate=c["p"], temperature=1.0, device=DEV, embedding_grad="dense", score_dtype="fp32",
                                          mlp_dtype=c["mlp"])
    state = init_state_numpy({k: tuple(v.shape) for k, v in task.state_dict().items()}, 4242)
    snap = {k: torch.from_numpy(np.asarray(v)) for k, v in state.items()}
    Bs = c["B"] if isinstance(c["B"], tuple) else (c["B"], c["B"])
    train = c["mode"] == "train"
    towers, inputs, d_embs = [], [], []
    for t, (tw, keys, side) in enumerate(((task.two_tower_model.notice_tower, kn, "notice"), (task.two_tower_model.company_tower, kc, "company"))):
        if Bs[t] == 0:
            continue
        b = synth_batch_numpy(Bs[t], vn, vc, c["din"][0], c["din"][1], 29 + Bs[t])
        tw._seed_override, tw.pack_for_score = SEEDS[t], True
        tw.sync_comm = Solo() if c["sync"] else None
        towers.append(tw)
        inputs.append({"dense": torch.from_numpy(b[side + "_dense"]).to(DEV),
                       "kjt": tt.build_batch_kjt(torch.from_numpy(b[side + "_ids"]), keys).to(DEV)})
        d_embs.append(torch.from_numpy(np.random.default_rng([7 * Bs[t] + c["D"], t]).standard_normal((Bs[t], c["D"])).astype(np.float32)).to(DEV))

    def once(**attrs):
        task.load_state_dict(snap)
        for prm in task.parameters():
            prm.grad = None
        for tw in towers:
            tw.train(train)
            for a, v in attrs.items():
                setattr(tw, a, v)
        TW._DEBUG_KEEP = []
        try:
            torch.cuda.synchronize()
            n0 = lib.tt_launch_count()
            if train:
                outs = TW.run_towers(towers, inputs)
                torch.autograd.backward(outs, d_embs)
            else:
                with torch.no_grad():
                    outs = TW.run_towers(towers, inputs)
            torch.cuda.synchronize()
            return outs, TW._DEBUG_KEEP, int(lib.tt_launch_count() - n0)
        finally:
            TW._DEBUG_KEEP = None

    if c["back"]:
        _, _, n_apart = once(unfused_back=True)
    outs, keep, launches = once(unfused_back=False)
    if c["back"] and launches >= n_apart:
        raise RuntimeError(f"{c['name']}: the one-launch first-block backward did not run: {launches} launches against {n_apart}")
    shas = []
    for t, (tw, o) in enumerate(zip(towers, outs)):
        h = hashlib.sha256()

        def add(tag, x):
            h.update(tag.encode())
            h.update(np.ascontiguousarray(x.detach().cpu().numpy() if x.dtype != torch.bfloat16 else x.detach().view(torch.int16).cpu().numpy()).tobytes())

        add("emb", o)
        pk = getattr(o, "_tt_packed", None)
        if pk is not None:
            add("packed", pk[0])
        if train:
            for i, prm in enumerate(tw.dense_parameters()):
                add(f"grad{i}", prm.grad)
            k = keep[t]
            nd, B, xw, h0 = k["n_dense"], k["B"], tw.x_width, tw.tower_hidden_dims[0]
            add("d_x", k["buf"][k["offs"][nd]:k["offs"][nd] + B * xw].view(B, xw)[:, h0:])
        for i in range(tw.n_hidden):
            bn = tw.mlp[4 * i + 2]
            add(f"rm{i}", bn.running_mean)
            add(f"rv{i}", bn.running_var)
            add(f"nbt{i}", bn.num_batches_tracked)
        shas.append(h.hexdigest())
    return shas


def digests():
    """{case id: [sha256 of each tower's outputs]}"""
    import jodalrob_twotower_amd as tt
    from jodalrob_twotower_amd import _lib
    from jodalrob_twotower_amd import towers as TW
    lib = _lib.load()
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for c in CASES:
            out[c["name"]] = _run(tt, TW, c, tmp, lib)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="write the JSON file (tests/golden/tower_bits.json) instead of printing the lines alone")
    ap.add_argument("--commit", default="unknown", help="the commit the library was built from (header of the JSON file)")
    a = ap.parse_args()
    d = digests()
    for k, v in d.items():
        print(k, *v)
    if a.out:
        head = {"commit": a.commit, "rocm": torch.version.hip, "device": torch.cuda.get_device_name(0),
                "note": "digests of the build named here; a change that alters the arithmetic on purpose regenerates this file and says so"}
        Path(a.out).write_text(json.dumps({"header": head, "cases": d}, indent=1) + "\n")
