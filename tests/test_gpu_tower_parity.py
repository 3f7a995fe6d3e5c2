"""The tower MLP (tt_towers_mlp_fwd / _bwd) against the f64 oracle (oracle_np.tower_fwd / tower_bwd) at shapes off the tile grid.

Both towers of a task run as in training -- ONE batched call of towers.run_towers, different din and key counts per tower -- and
autograd.backward feeds them seeded random embedding gradients, so neither the score kernels nor a unit tangent hide anything.
bf16 MLP against the oracle with the kernels' operand rounding (q = q_bf16), fp32 against the unrounded oracle.  Checked per case:
the embeddings, each hidden block's pre-activation and BatchNorm mean / rstd (read through towers._DEBUG_KEEP), every dense
gradient, the tables' dense gradients, the BatchNorm running statistics, and the eval forward on the updated statistics.  Then
stage by stage (_stage_checks): each stage against the oracle's arithmetic fed the kernels' own input to that stage, which pins
every kernel's arithmetic at any depth, where the end-to-end figures also carry bf16 rounding flips from upstream.

Every case names the path it is written to cover, and the launch counts confirm it: a case on the one-launch front, a fused
(narrow or wide) tail or the one-launch first-block backward launches fewer kernels than the same pass with the matching
tower_unfused_* switch; a case that falls back launches the same number.  The projection gradients' oracle form (proj_grad) is
read off the same count.  At every case also: bf16 weight shadows (tower._w16, as GraphedTrainStep sets them) change no bit,
a bf16 tower input (tower_io_dtype "x") equals an f32 one ("none") bit for bit, and the packed score operand images the pass
emits equal ops.score_pack2_bf16 of the returned rows bit for bit.

Each case prints one JSON report line (visible with -s), then asserts.  Bounds quote what an MI355X measured.
"""
import json

import numpy as np
import pytest
import torch

import oracle_np as O
from test_gpu_dropout_parity import SEED_C, SEED_N, _masks
from test_gpu_parity import DEV, tt  # noqa: F401

pytestmark = pytest.mark.gpu

# Bounds against the f64 oracle, each at most 4x the worst figure an MI355X measured over CASES (in brackets).  Norm-wise per tensor
# unless named max-abs; "matrix" = Linear weights, "vector" = biases and BatchNorm scale / shift (column sums over the batch),
# "table" = the tables' dense gradients; pre / mean / rstd per hidden block.  DESIGN.md section 4 quotes these tables.
#
# End to end.  bf16 against the oracle with the kernels' operand rounding: what is left is f32 accumulation order and the element
# whose f32 value (kernels) and f64 value (oracle) straddle a bf16 rounding boundary -- the two then round apart by 2^-8 of it, and
# that one flipped operand moves everything downstream.  Flips of the projection's output x (a wide kx against few hidden columns)
# reach the first block's gradients through the BatchNorm backward, whose batch sums cancel: so the vectors and the tables sit up to
# 5.5x above test_gpu_parity.BF16_STEP_BOUNDS' on-grid 5.6e-4 (worst: wide-H200-D128-B8300, a 64-wide x over 8300 rows).  The
# kernels' own arithmetic at those tensors is pinned to <= 3.4e-7 by STAGE_BOUNDS.
TOWER_BOUNDS = {
    "bf16": {"emb_norm": 2.9e-4, "emb_maxabs": 3.8e-3,          # (7.3e-5 / 9.6e-4)
             "pre": 1.2e-4, "mean": 4.4e-6, "rstd": 5.8e-6,     # (3.1e-5: a second block behind flipped x; 1.1e-6 / 1.5e-6)
             "grad_matrix": 7e-3, "grad_vector": 1.2e-2,        # (1.8e-3 / 3.1e-3)
             "table": 7.5e-3,                                   # (1.9e-3)
             "bn_running_mean": 4.9e-7, "bn_running_var": 1.8e-7},   # (1.2e-7 / 4.6e-8)
    "fp32": {"emb_norm": 5.7e-6, "emb_maxabs": 9.6e-6,          # (1.4e-6 / 2.4e-6, eight blocks)
             "pre": 4.2e-6, "mean": 2.5e-6, "rstd": 4e-6,       # (1.1e-6; 6.5e-7 / 1.0e-6 at B = 2)
             "grad_matrix": 6e-6, "grad_vector": 6.6e-6,        # (1.5e-6 / 1.7e-6)
             "table": 5.6e-6,                                   # (1.4e-6)
             "bn_running_mean": 4e-7, "bn_running_var": 1.8e-7},     # (1.0e-7 / 4.6e-8)
}
# bf16 towers deeper than three hidden blocks, end to end: every block's BN output is rounded to bf16 for the next Linear, so the
# flips above recur at every block and each perturbs the next block's pre-activations, which moves more values across boundaries
# there: the forward error grows about 3x per block from the third on (blocks 0 / 1 at 4e-8, block 7 at 1.2e-3) and the backward
# sees the grown forward error through the BatchNorm backward's cancellations.  Not a kernel error: _stage_checks holds every stage
# of the same passes to <= 3.4e-7 (STAGE_BOUNDS), and an fp32 tower of the same depth (no rounding points) stays at 1.5e-6.
DEEP_BF16_BOUNDS = dict(TOWER_BOUNDS["bf16"], emb_norm=8e-3, emb_maxabs=1.1e-2,     # (2.2e-3 / 2.9e-3)
                        pre=4.5e-3, mean=1.6e-3, rstd=1e-3,                     # (1.2e-3 / 4.1e-4 / 2.6e-4, block 7)
                        grad_matrix=0.14, grad_vector=0.25, table=0.13,         # (3.6e-2 / 6.4e-2 / 3.4e-2)
                        bn_running_mean=1.9e-4, bn_running_var=2.3e-5)          # (4.8e-5 / 5.7e-6)
# Stage by stage: each stage against the oracle's arithmetic fed the kernels' OWN input to it (_stage_checks) -- no flips, so this
# is one stage's f32 accumulation order alone, at every depth.  "grad" covers d_y, d_pre and every gradient formed from them.
STAGE_BOUNDS = {"bf16": {"pre": 3.6e-7, "bn": 6.6e-7, "act": 2e-7, "grad": 1.3e-6},     # (9.1e-8 / 1.7e-7 / 5.1e-8 / 3.4e-7)
                "fp32": {"pre": 8.3e-7, "bn": 3.1e-7, "act": 2.2e-7, "grad": 1.6e-6}}   # (2.1e-7 / 8.0e-8 / 5.5e-8 / 4.1e-7)
# BatchNorm over two rows: xhat = +-1 up to eps, so the BN backward's terms cancel to rounding noise and every gradient in front of
# the last BatchNorm is noise about a (near) zero reference: bounded by norm(got - ref) <= atol + rtol * norm(ref) instead, rtol the
# matrix bound (the forward and the gradients behind the last BatchNorm keep TOWER_BOUNDS).  End to end: atol (7.8e-5, bf16);
# stage by stage, d_pre against the BN backward of the kernels' own upstream gradient: dpre_atol (3.3e-6 bf16 / 1.1e-6 fp32).
TWO_ROW_BOUNDS = {"atol": 3e-4, "dpre_atol": {"bf16": 1.3e-5, "fp32": 4.3e-6}}
# D = 1: every unit row is +-1 and its tangent space is empty, so every reference gradient is exactly 0 -- and so is every gradient
# the kernels return (measured: exactly 0)
EVAL_BOUNDS = {"bf16": {"emb_norm": 4.5e-4, "emb_maxabs": 2.8e-3},     # (1.1e-4 / 7.0e-4)
               "fp32": {"emb_norm": 1e-6, "emb_maxabs": 1.1e-6}}       # (2.6e-7 / 2.8e-7)


def _case(name, mlp, hidden, D, B, E=32, keys=(3, 1), din=(64, 128), p=0.0, front=False, tail=None, back=False, mode="train"):
    """hidden lists the projection width first (the reference's convention); keys / din: (notice, company).  The path claims:
    front = tower_front_kernel; tail = "narrow" (tail_*_kernel) | "wide" (tail_*_wide_kernel) | None (separate kernels);
    back = gemm_back_kernel (one-launch first-block backward).  The launch counts confirm a fused tail; which of the two it is
    follows from the widths (tail_shape_ok: last hidden width and D at most 64), checked here so that a row cannot name the other."""
    if tail is not None:
        assert (tail == "narrow") == (len(hidden) > 1 and hidden[-1] <= 64 and D <= 64), name
    return pytest.param(dict(name=name, mlp=mlp, hidden=list(hidden), D=D, B=B, E=E, keys=keys, din=din, p=p, front=front, tail=tail,
                             back=back, mode=mode), id=name)


DEEP = [40, 33, 70, 17, 129, 65, 50, 90, 48]         # TT_MAX_HIDDEN = 8 blocks behind the projection, last <= 64
DEEP_WIDE = [32, 65, 17, 90, 33, 48, 129, 40, 100]    # ... last > 64

CASES = [
    # front + narrow fused tail: h0 a multiple of 32 (<= 128), din and kx = h0 + keys * E multiples of 64
    _case("front-h32-H17-D33-B65", "bf16", [32, 17], 33, 65, keys=(3, 1), din=(64, 128), front=True, tail="narrow"),
    _case("front-h96-H63-D1-B4097", "bf16", [96, 63], 1, 4097, keys=(5, 1), din=(192, 64), front=True, tail="narrow"),
    _case("front-h128-H64-D64-B8191", "bf16", [128, 64], 64, 8191, E=16, keys=(8, 4), din=(256, 128), front=True, tail="narrow"),
    _case("front-h32-H1-D64-B2", "bf16", [32, 1], 64, 2, keys=(3, 1), din=(64, 64), front=True, tail="narrow"),
    _case("front-back-h128-H64-D33-B8192", "bf16", [128, 64], 33, 8192, keys=(4, 2), din=(256, 128), front=True, tail="narrow",
          back=True),
    # narrow fused tail behind the separate projection / block GEMMs (h0 or din off the front's grid)
    _case("tail-h48-din100-37", "bf16", [48, 40], 33, 1000, E=8, keys=(3, 2), din=(100, 37), tail="narrow"),
    _case("tail-2blk-odd", "bf16", [40, 72, 50], 17, 4097, E=6, keys=(5, 3), din=(37, 100), tail="narrow"),
    _case("tail-3blk-odd", "bf16", [24, 33, 65, 31], 64, 300, E=8, keys=(2, 3), din=(50, 64), tail="narrow"),
    # wide tail: H not a multiple of 16 (the Hp padding) and the limit 256, D up to 128 (Dp = 128)
    _case("wide-H65-D100-B63", "bf16", [64, 65], 100, 63, keys=(2, 1), din=(64, 128), tail="wide"),
    _case("wide-H129-D65-B4097", "bf16", [96, 129], 65, 4097, E=16, keys=(3, 5), din=(192, 100), tail="wide"),
    _case("wide-H200-D128-B8300", "bf16", [32, 200], 128, 8300, E=8, keys=(4, 2), din=(64, 37), tail="wide"),
    _case("wide-H256-D128-B2", "bf16", [128, 256], 128, 2, keys=(2, 1), din=(64, 128), tail="wide"),
    # general bf16 path: H > 256 or D > 128 (l2norm generic at D = 130, fast at 192 / 256)
    _case("general-H300-D130", "bf16", [64, 300], 130, 1000, E=8, keys=(3, 2), din=(100, 64)),
    _case("general-H96-D192-B4097", "bf16", [128, 96], 192, 4097, keys=(2, 3), din=(128, 64)),
    _case("general-back-H64-D256-B2048", "bf16", [64, 64], 256, 2048, keys=(2, 4), din=(128, 64), back=True),
    # no hidden block: projection, concatenation, output Linear, L2 normalise
    _case("nohidden-bf16-h37-D70", "bf16", [37], 70, 300, E=6, keys=(3, 2), din=(37, 64)),
    _case("nohidden-bf16-h128-D1", "bf16", [128], 1, 65, keys=(2, 1), din=(64, 128)),
    _case("nohidden-fp32-h37-D70", "fp32", [37], 70, 4097, E=6, keys=(3, 2), din=(37, 64)),
    _case("nohidden-fp32-h128-D1", "fp32", [128], 1, 2, keys=(2, 1), din=(64, 128)),
    # deep: eight hidden blocks of mixed odd widths
    _case("deep8-narrow", "bf16", DEEP, 40, 1000, E=6, keys=(3, 2), din=(37, 64), tail="narrow"),
    _case("deep8-wide", "bf16", DEEP_WIDE, 64, 513, E=6, keys=(3, 2), din=(37, 64), tail="wide"),
    # one-launch first-block backward: B % 64 = 0, H in {64, 128, 256}, (H / 64) * h0 <= 256; each next to a neighbour just off
    # its predicate (B = 4095, h0 = 96, din = 200), which takes the separate GEMMs
    _case("back-h64-H256-B4096", "bf16", [64, 256], 64, 4096, keys=(2, 4), din=(128, 64), tail="wide", back=True),
    _case("back-off-h64-H256-B4095", "bf16", [64, 256], 64, 4095, keys=(2, 4), din=(128, 64), tail="wide"),
    _case("back-h128-H128-B2048", "bf16", [128, 128], 48, 2048, keys=(2, 4), din=(128, 64), tail="wide", back=True),
    _case("back-off-h96-H128-B2048", "bf16", [96, 128], 48, 2048, keys=(1, 3), din=(128, 64), tail="wide"),
    _case("back-k64-h256-H64-B1024", "bf16", [256, 64], 64, 1024, keys=(2, 4), din=(128, 256), tail="narrow", back=True),
    _case("back-off-k64-h256-din200", "bf16", [256, 64], 64, 1024, keys=(2, 4), din=(200, 256), tail="narrow"),
    # split-K: a small batch against a wide tower input -- 4 / 20 output tiles in the block GEMM's launch, so nt_splits =
    # min(kx / 128, 16) = 8 / 5 and 5 / 8 (the narrow tail's tail_head_kernel finishes the slabs, the general path's
    # slab_reduce_kernel); kx = 1072 / 688 and 680 / 1064 are not multiples of BK16 = 32
    _case("splitk-tail-B128", "bf16", [48, 64], 32, 128, keys=(32, 20), din=(64, 64), tail="narrow"),
    _case("splitk-general-B128", "bf16", [40, 300], 100, 128, keys=(20, 32), din=(64, 100)),
    # fp32: gemm_kernel, vec (every row 16-byte aligned) and non-vec (din odd, E = 6)
    _case("fp32-nonvec-B4097", "fp32", [37, 45], 33, 4097, E=6, keys=(3, 5), din=(101, 37)),
    _case("fp32-vec-B8300", "fp32", [64, 128], 64, 8300, E=8, keys=(4, 2), din=(128, 64)),
    _case("fp32-3blk-B2", "fp32", [33, 17, 40], 9, 2, E=6, keys=(3, 2), din=(37, 20)),
    _case("fp32-deep8", "fp32", DEEP, 40, 300, E=6, keys=(3, 2), din=(37, 64)),
    # eval forward at B = 1 (bn_eval_prepare + bn_apply; the fused tails are train-only)
    _case("eval-bf16-B1", "bf16", [64, 100], 70, 1, keys=(2, 1), din=(64, 128), mode="eval"),
    _case("eval-nohidden-bf16-B1", "bf16", [37], 70, 1, E=6, keys=(3, 2), din=(37, 64), mode="eval"),
    _case("eval-fp32-B1", "fp32", [37, 45], 33, 1, E=6, keys=(3, 5), din=(101, 37), mode="eval"),
    # dropout on, off the tile grid (the masks restated by test_gpu_dropout_parity)
    _case("dropout-narrow-B1000", "bf16", [48, 40], 33, 1000, E=8, keys=(3, 2), din=(100, 37), p=0.2, tail="narrow"),
    _case("dropout-wide-2blk-B4097", "bf16", [40, 70, 129], 100, 4097, E=6, keys=(3, 2), din=(37, 64), p=0.1, tail="wide"),
]


def _keys_vocabs(c):
    kn = [f"n{i}" for i in range(c["keys"][0])]
    kc = [f"c{i}" for i in range(c["keys"][1])]
    return kn, kc, [20 + 3 * i for i in range(len(kn))], [17 + 5 * i for i in range(len(kc))]


def _build(tt, tmp_path, c):
    from jodalrob_twotower_amd import synthetic
    kn, kc, vn, vc = _keys_vocabs(c)
    meta = synthetic.write_metadata(tmp_path / "m.csv", {"notice": dict(zip(kn, vn)), "company": dict(zip(kc, vc))})
    torch.manual_seed(4242)
    task = tt.create_two_tower_train_task(kn, kc, metadata_path=str(meta), categorical_embedding_dim=c["E"], notice_dense_input_dim=c["din"][0],
                                          company_dense_input_dim=c["din"][1], tower_hidden_dims=c["hidden"], final_embedding_dim=c["D"],
                                          dropout_rate=c["p"], temperature=1.0, device=DEV, embedding_grad="dense", score_dtype="fp32",
                                          mlp_dtype=c["mlp"])
    with torch.no_grad():                       # BN scale / shift and biases away from the init's symmetric spots
        g = torch.Generator(device=DEV).manual_seed(83)
        for prm in task.parameters():
            if prm.ndim == 1:
                prm.add_(0.1 * torch.randn(prm.shape, generator=g, device=DEV))
        for name, buf in task.named_buffers():  # running statistics away from (0, 1): the eval forward then reads real values
            if name.endswith("running_mean"):
                buf.copy_(0.2 * torch.randn(buf.shape, generator=g, device=DEV))
            elif name.endswith("running_var"):
                buf.copy_(0.5 + torch.rand(buf.shape, generator=g, device=DEV))
    tn, tc = task.two_tower_model.notice_tower, task.two_tower_model.company_tower
    tn._seed_override, tc._seed_override = SEED_N, SEED_C
    for tw in (tn, tc):
        tw.pack_for_score = True
    batch = synthetic.make_batch(c["B"], vn, vc, kn, kc, c["din"][0], c["din"][1], torch.device(DEV), seed=c["B"] + 29)
    return task, (tn, tc), batch, (kn, kc, vn, vc)


def _acts_view(tw, k):
    """the kernels' intermediates of one tower: per hidden block pre / act [B, H], mean / rstd [H] and the gradient d_pre [B, H]
    (the backward's scratch, BN-backward applied in place), the output Linear's y and d_y [B, D] -- out of the flat activation
    buffer x | (pre_i, act_i)* | (mean_i, rstd_i)* | y and the backward buffer (towers.py _TowersFn)"""
    from jodalrob_twotower_amd import towers as TW
    B, hid, D = k["B"], list(k["hidden"]), tw.final_embedding_dim
    sizes = [TW._al(B * tw.x_width) if tw.x_dtype == torch.float32 else 0] + [TW._al(B * h) for h in hid for _ in (0, 1)] + \
        [TW._al(h) for h in hid for _ in (0, 1)]
    offs = np.concatenate([[0], np.cumsum(sizes)])
    nh = len(hid)
    buf = k["acts"].detach().cpu().numpy()
    gbuf, goffs, nd = k["buf"].detach().cpu().numpy(), k["offs"], k["n_dense"]
    blocks = [{"pre": buf[offs[1 + 2 * i]:offs[1 + 2 * i] + B * H].reshape(B, H),
               "act": buf[offs[2 + 2 * i]:offs[2 + 2 * i] + B * H].reshape(B, H),
               "mean": buf[offs[1 + 2 * nh + 2 * i]:offs[1 + 2 * nh + 2 * i] + H].copy(),
               "rstd": buf[offs[2 + 2 * nh + 2 * i]:offs[2 + 2 * nh + 2 * i] + H].copy(),
               "dpre": gbuf[goffs[nd + 1 + i]:goffs[nd + 1 + i] + B * H].reshape(B, H)} for i, H in enumerate(hid)]
    y = buf[offs[1 + 4 * nh]:offs[1 + 4 * nh] + B * D].reshape(B, D)
    dy = gbuf[goffs[nd + 1 + nh]:goffs[nd + 1 + nh] + B * D].reshape(B, D)
    return {"blocks": blocks, "y": y, "dy": dy}


class _Runner:
    """Runs the two towers' pass from one saved state: every pass starts from the same parameters and running statistics."""

    def __init__(self, task, towers, batch, c):
        from jodalrob_twotower_amd import _lib
        self.task, self.towers, self.c = task, towers, c
        self.inputs = [batch["notice"], batch["company"]]
        self.snap = {k: v.detach().clone() for k, v in task.state_dict().items()}
        g = torch.Generator(device=DEV).manual_seed(c["B"] * 7 + c["D"])
        self.d_embs = [torch.randn(c["B"], c["D"], generator=g, device=DEV) for _ in towers]
        self.lib = _lib.load()

    def run(self, train=True, keep=False, **attrs):
        from jodalrob_twotower_amd import towers as TW
        self.task.load_state_dict(self.snap)
        for p in self.task.parameters():
            p.grad = None
        saved = [{a: getattr(tw, a) for a in attrs} for tw in self.towers]
        for tw in self.towers:
            tw.train(train)
            for a, v in attrs.items():
                setattr(tw, a, v(tw) if callable(v) else v)
        TW._DEBUG_KEEP = [] if keep else None
        try:
            torch.cuda.synchronize()
            n0 = self.lib.tt_launch_count()
            if train:
                outs = TW.run_towers(list(self.towers), self.inputs)
                torch.autograd.backward(outs, self.d_embs)
            else:
                with torch.no_grad():
                    outs = TW.run_towers(list(self.towers), self.inputs)
            torch.cuda.synchronize()
            launches = int(self.lib.tt_launch_count() - n0)
            k = TW._DEBUG_KEEP
        finally:
            TW._DEBUG_KEEP = None
            for tw, s in zip(self.towers, saved):
                for a, v in s.items():
                    setattr(tw, a, v)
        res = {"launches": launches, "emb": [o.detach().cpu().numpy().copy() for o in outs],
               "packed": [getattr(o, "_tt_packed", None) for o in outs]}
        if train:
            res["grads"] = {n: p.grad.detach().cpu().numpy().copy() for n, p in self.task.named_parameters() if p.grad is not None}
            res["state"] = {k_: v.detach().cpu().numpy().copy() for k_, v in self.task.state_dict().items()
                            if "running" in k_ or "num_batches" in k_}
        if keep:
            res["inter"] = [_acts_view(tw, kk) for tw, kk in zip(self.towers, k)]
        return res


def _shadows(tw):
    """bf16 shadows of the projection and block weights, as GraphedTrainStep's hand-over launch leaves them"""
    ws = [tw.dense_projection.weight] + [tw.mlp[4 * i].weight for i in range(tw.n_hidden)]
    sh = [w.detach().to(torch.bfloat16).contiguous() for w in ws]
    return (sh[0], sh[1:])


def _err(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-300))


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a["emb"], b["emb"])) and \
        all(np.array_equal(a["grads"][k], b["grads"][k]) for k in a["grads"]) and \
        all(np.array_equal(a["state"][k], b["state"][k]) for k in a["state"])


def _stage_checks(st, pre, c, kv, emb_k, grads_k, dE, q, keeps, side, report, checks):
    """Each stage of the pass against the f64 oracle's arithmetic fed the kernels' OWN input to that stage (their act, pre, mean,
    rstd, y, d_y, d_pre): what is left is that one stage's f32 accumulation, however many rounded Linears came before it.  Forward:
    block i >= 1's pre from act[i - 1]; mean / rstd from pre; act from (pre, mean, rstd) [* keep * scale]; y from the last act;
    emb from y.  Backward: d_y from (y, emb, d_emb); the output layer's gradients from d_y; per block, top down, d_pre from the
    gradient above it through the BatchNorm backward (on the kernels' statistics), the block's BN and (i >= 1) Linear gradients
    from d_pre."""
    q = q or (lambda a: a)
    f = lambda a: np.asarray(a, dtype=np.float64)
    bd = STAGE_BOUNDS[c["mlp"]]
    B, D, nh = c["B"], c["D"], len(c["hidden"]) - 1
    scale = f(O.dropout_scale(c["p"])) if keeps else None
    blocks = kv["blocks"]

    def chk(tag, got, ref, kind):
        e = _err(got, ref)
        report[f"{side}.stage.{tag}"] = e
        checks.append((f"{side}.stage.{tag}", e <= bd[kind]))

    for i, kb in enumerate(blocks):
        W, b_ = f(st[f"{pre}mlp.{4 * i}.weight"]), f(st[f"{pre}mlp.{4 * i}.bias"])
        g, be = f(st[f"{pre}mlp.{4 * i + 2}.weight"]), f(st[f"{pre}mlp.{4 * i + 2}.bias"])
        if i >= 1:
            chk(f"block{i}.pre", kb["pre"], q(f(blocks[i - 1]["act"])) @ q(W).T + b_, "pre")
        a = np.maximum(f(kb["pre"]), 0)
        chk(f"block{i}.mean", kb["mean"], a.mean(axis=0), "bn")
        chk(f"block{i}.rstd", kb["rstd"], 1.0 / np.sqrt(a.var(axis=0) + O.BN_EPS), "bn")
        act = (a - f(kb["mean"])) * f(kb["rstd"]) * g + be
        if keeps and keeps[i] is not None:
            act = act * np.where(keeps[i], scale, 0.0)
        chk(f"block{i}.act", kb["act"], act, "act")
    fin = 4 * nh
    Wf = f(st[f"{pre}mlp.{fin}.weight"])
    y = f(kv["y"])
    if nh:
        chk("y", y, q(f(blocks[-1]["act"])) @ q(Wf).T + f(st[f"{pre}mlp.{fin}.bias"]), "pre")
    nrm = np.sqrt((y * y).sum(axis=1, keepdims=True))
    chk("emb", emb_k, y / np.maximum(nrm, O.NORM_EPS), "act")
    if D == 1:                              # (the tangent space is empty: the backward is pinned by the zero-reference check)
        return
    e = f(emb_k)
    dot = (e * dE).sum(axis=1, keepdims=True)
    chk("dy", kv["dy"], np.where(nrm > O.NORM_EPS, (dE - e * dot) / np.maximum(nrm, O.NORM_EPS), dE / O.NORM_EPS), "grad")
    dnext, Wn = f(kv["dy"]), Wf
    if nh:
        chk(f"mlp.{fin}.weight", grads_k[f"{pre}mlp.{fin}.weight"], q(dnext).T @ q(f(blocks[-1]["act"])), "grad")
    chk(f"mlp.{fin}.bias", grads_k[f"{pre}mlp.{fin}.bias"], dnext.sum(axis=0), "grad")
    for i in reversed(range(nh)):
        kb = blocks[i]
        dh = q(dnext) @ q(Wn)
        if keeps and keeps[i] is not None:
            dh = dh * np.where(keeps[i], scale, 0.0)
        pre_k = f(kb["pre"])
        xhat = (np.maximum(pre_k, 0) - f(kb["mean"])) * f(kb["rstd"])
        g = f(st[f"{pre}mlp.{4 * i + 2}.weight"])
        chk(f"mlp.{4 * i + 2}.weight", grads_k[f"{pre}mlp.{4 * i + 2}.weight"], (dh * xhat).sum(axis=0), "grad")
        chk(f"mlp.{4 * i + 2}.bias", grads_k[f"{pre}mlp.{4 * i + 2}.bias"], dh.sum(axis=0), "grad")
        dxh = dh * g
        dpre = f(kb["rstd"]) * (dxh - dxh.mean(axis=0) - xhat * (dxh * xhat).mean(axis=0)) * (pre_k > 0)
        if B == 2:                          # BatchNorm over two rows: d_pre is noise about zero (TWO_ROW_BOUNDS)
            err = float(np.linalg.norm(f(kb["dpre"]) - dpre))
            report[f"{side}.stage.block{i}.dpre"] = err
            checks.append((f"{side}.stage.block{i}.dpre",
                           err <= TWO_ROW_BOUNDS["dpre_atol"][c["mlp"]] + bd["grad"] * float(np.linalg.norm(dpre))))
        else:
            chk(f"block{i}.dpre", kb["dpre"], dpre, "grad")
        dnext, Wn = f(kb["dpre"]), f(st[f"{pre}mlp.{4 * i}.weight"])
        if i >= 1:
            chk(f"mlp.{4 * i}.weight", grads_k[f"{pre}mlp.{4 * i}.weight"], q(dnext).T @ q(f(blocks[i - 1]["act"])), "grad")
        chk(f"mlp.{4 * i}.bias", grads_k[f"{pre}mlp.{4 * i}.bias"], dnext.sum(axis=0), "grad")


@pytest.mark.parametrize("c", CASES)
def test_tower_pass_vs_f64_oracle(tt, tmp_path, c):
    from jodalrob_twotower_amd import ops
    task, towers, batch, (kn, kc, vn, vc) = _build(tt, tmp_path, c)
    B, D, mlp, train = c["B"], c["D"], c["mlp"], c["mode"] == "train"
    R = _Runner(task, towers, batch, c)
    state0 = {k: v.cpu().numpy() for k, v in R.snap.items()}
    R.run(train=train)                                          # first-call paths
    base = R.run(train=train, keep=train)
    report = {"case": c["name"], "mlp": mlp, "hidden": c["hidden"], "D": D, "B": B, "p": c["p"], "launches": base["launches"]}

    # ---- the path the case names, by launch counts against the matching unfused switch
    claims = {}
    unf = {}
    for sw, attr in (("front", "unfused_front"), ("tail", "unfused_tail"), ("back", "unfused_back")):
        unf[sw] = R.run(train=train, **{attr: True})
        report[f"launches_{attr}"] = unf[sw]["launches"]
        claims[sw] = unf[sw]["launches"] > base["launches"]
    want = {"front": c["front"], "tail": c["tail"] is not None, "back": c["back"]}
    proj = "factored" if claims["back"] else "direct"

    # ---- claim checks: shadows, bf16 vs f32 tower input, packed operand images
    if train and mlp == "bf16":
        report["shadows_bit_identical"] = _same(R.run(_w16=_shadows), base)
        arm = unf["front"] if c["front"] else base      # (the one-launch front needs a bf16 x: both arms without it)
        f32x = R.run(unfused_front=True, x_dtype=torch.float32)
        report["io_x_equals_none"] = _same(arm, f32x)
    pk = ops.score_pack2_bf16(torch.from_numpy(base["emb"][0]).to(DEV), torch.from_numpy(base["emb"][1]).to(DEV), 1.0, 1.0)
    report["packed_bit_identical"] = all(p is not None and p[1] == 1.0 and torch.equal(p[0], q) for p, q in zip(base["packed"], pk))

    # ---- the f64 oracle
    b = {"notice_ids": batch["notice"]["kjt"].values().cpu().numpy(), "company_ids": batch["company"]["kjt"].values().cpu().numpy(),
         "notice_dense": batch["notice"]["dense"].cpu().numpy(), "company_dense": batch["company"]["dense"].cpu().numpy()}
    q = O.q_bf16 if mlp == "bf16" else None
    drop = (c["p"], _masks(task, B, c["p"])) if (train and c["p"] > 0) else None
    bd = DEEP_BF16_BOUNDS if (mlp == "bf16" and len(c["hidden"]) - 1 > 3) else TOWER_BOUNDS[mlp]
    two_rows = train and B == 2
    checks = []
    for t, (pre, side, keys, vocab) in enumerate(((O.NT, "notice", kn, vn), (O.CT, "company", kc, vc))):
        dE = R.d_embs[t].cpu().numpy().astype(np.float64)
        emb, cache, bn_up = O.tower_fwd(state0, pre, keys, vocab, b[side + "_dense"], b[side + "_ids"], train, np.float64, q, drop)
        got = base["emb"][t]
        report[side + ".emb"] = (_err(got, emb), float(np.abs(got - emb).max()))
        eb = bd if train else EVAL_BOUNDS[mlp]
        checks.append((side + ".emb", report[side + ".emb"][0] <= eb["emb_norm"] and report[side + ".emb"][1] <= eb["emb_maxabs"]))
        if not train:
            continue
        for i, blk in enumerate(cache["blocks"]):
            kb = base["inter"][t]["blocks"][i]
            ref = {"pre": blk["pre"], "mean": np.maximum(blk["pre"], 0).mean(axis=0), "rstd": blk["rstd"]}
            for stage in ("pre", "mean", "rstd"):
                e = _err(kb[stage], ref[stage])
                report[f"{side}.block{i}.{stage}"] = e
                checks.append((f"{side}.block{i}.{stage}", e <= bd[stage]))
        g = O.tower_bwd(cache, dE, pre, keys, vocab, "dense", proj)
        _stage_checks(state0, pre, c, base["inter"][t], base["emb"][t], base["grads"], dE, q,
                      [drop[1].get((pre, i)) for i in range(len(c["hidden"]) - 1)] if drop else None, side, report, checks)
        zero_ref = D == 1
        # in front of the last BatchNorm over two rows: noise about a zero reference
        last_bn = 4 * (len(c["hidden"]) - 2) + 2
        for name, ref in g.items():
            if name.startswith("_"):
                continue
            gk = base["grads"][name]
            short = name[len(pre):]
            kind = "table" if "categorical_embedder" in name else ("grad_matrix" if gk.ndim > 1 else "grad_vector")
            if zero_ref:
                assert not np.any(ref), name
                e = float(np.abs(gk).max())
                ok = e == 0.0
            elif two_rows and len(c["hidden"]) > 1 and not (short.startswith("mlp.") and int(short.split(".")[1]) >= last_bn):
                e = float(np.linalg.norm(gk - ref))
                ok = e <= TWO_ROW_BOUNDS["atol"] + bd["grad_matrix"] * float(np.linalg.norm(ref))
            else:
                e = _err(gk, ref)
                ok = e <= bd[kind]
            report[f"{side}.{short}"] = e
            checks.append((f"{side}.{short}", ok))
        for k, ref in bn_up.items():
            gk = base["state"][k]
            if k.endswith("num_batches_tracked"):
                checks.append((k, int(gk) == int(ref)))
                continue
            kind = "bn_" + k.rsplit(".", 1)[1]
            e = _err(gk, ref)
            report[f"{side}.{k[len(pre):]}"] = e
            checks.append((k, e <= bd[kind]))
    # ---- eval forward on the running statistics this pass left (train cases; eval cases were checked above)
    if train:
        st1 = dict(state0)
        st1.update(base["state"])
        R.snap = {k: torch.from_numpy(np.asarray(v)).to(DEV) for k, v in st1.items()}
        ev = R.run(train=False)
        for t, (pre, side, keys, vocab) in enumerate(((O.NT, "notice", kn, vn), (O.CT, "company", kc, vc))):
            emb, _, _ = O.tower_fwd(st1, pre, keys, vocab, b[side + "_dense"], b[side + "_ids"], False, np.float64, q)
            e = (_err(ev["emb"][t], emb), float(np.abs(ev["emb"][t] - emb).max()))
            report[side + ".eval_emb"] = e
            checks.append((side + ".eval_emb", e[0] <= EVAL_BOUNDS[mlp]["emb_norm"] and e[1] <= EVAL_BOUNDS[mlp]["emb_maxabs"]))
    report.update({"claims": claims, "want": want, "proj_grad": proj})
    print(f"\n[tower pass vs f64 oracle]", json.dumps(report))
    for sw in claims:
        assert claims[sw] == (want[sw] if train else False), (sw, claims, want, report)
    for key in ("shadows_bit_identical", "io_x_equals_none", "packed_bit_identical"):
        if key in report:
            assert report[key], (key, report)
    bad = [tag for tag, ok in checks if not ok]
    assert not bad, (bad, report)
