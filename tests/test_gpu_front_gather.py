"""The towers' one-launch front gathering the embedding rows itself (tower_front_kernel's GATHER form, tt_tower_acts.gather_*)
against the two launches it replaces -- tt_embed_lookup_rows_fwd + the front reading x -- on the same build.  Every comparison is
array_equal: the gathered pieces are rounded and packed as the lookup's store does, and no sum changes its order.

  kernel level    x whole (projection columns included), pre, the chunk partials (the whole tower workspace), and everything the tail
                  makes of them, over batch sizes 64 / 65 / 190 / 300 (chunks of 64, 64 + 1, 64 and 60 rows) and 8257 (chunks of 65
                  rows: a second block with one live row per workgroup), two towers of different K in one launch, K = 1, E = 8 / 16 /
                  32 / 64, h0 = 32 / 64 / 128, kx = 64 (narrower than one stage) and 448 (into the stage loop's padding), rows that hit
                  table row 0 and the last row of a table that ends its buffer, all samples on one row
  refusals        E = 12, f32 x, din % 64 != 0, two hidden blocks: tt_towers_fwd_gathers answers 0 and the two launches run
  captured step   GraphedTrainStep / UnrolledTrainStep(unroll=2) with settings.front_gather on and off: losses and state_dict equal
                  bit for bit, library_launches apart by exactly one
"""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import GOLD
from params_init import init_state_numpy, synth_batch_numpy

from jodalrob_twotower_amd import _lib as L
from jodalrob_twotower_amd import config as _cfg
from jodalrob_twotower_amd import ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
D_OUT = 64


def _tower(g, K, E, h0, din, hidden, x_dtype):
    """One tower's parameters (f32 + bf16 shadows), seeded"""
    dev = torch.device(DEV)
    rnd = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).to(dev)     # noqa: E731
    widths = [h0 + K * E] + list(hidden)
    t = {"w_proj": rnd(h0, din, scale=din ** -0.5), "b_proj": rnd(h0, scale=0.1),
         "w": [rnd(h, k, scale=k ** -0.5) for h, k in zip(hidden, widths)], "b": [rnd(h, scale=0.1) for h in hidden],
         "bn_w": [1.0 + rnd(h, scale=0.1) for h in hidden], "bn_b": [rnd(h, scale=0.1) for h in hidden],
         "w_out": rnd(D_OUT, widths[-1], scale=widths[-1] ** -0.5), "b_out": rnd(D_OUT, scale=0.1),
         "K": K, "h0": h0, "din": din, "hidden": list(hidden), "x_dtype": x_dtype}
    t["w_proj16"] = t["w_proj"].to(torch.bfloat16)
    t["w16"] = [w.to(torch.bfloat16) for w in t["w"]]
    return t


def _run(towers, table, rows, dense, B, E, gather, flags=0, ids_lookup=False):
    """One training forward of the towers side by side: gather=False looks the rows up in a launch of its own.  Returns the
    predicate's answer and every output as numpy arrays (x as raw 16-bit / 32-bit words)."""
    dev = torch.device(DEV)
    params, acts, keep, outs, sides = [], [], [], [], []
    base = 0
    for t, dn in zip(towers, dense):
        K, h0, hid = t["K"], t["h0"], t["hidden"]
        kx = h0 + K * E
        bf = t["x_dtype"] == torch.bfloat16
        rm = [torch.zeros(h, device=dev) for h in hid]
        rv = [torch.ones(h, device=dev) for h in hid]
        nbt = [torch.zeros((), dtype=torch.int64, device=dev) for _ in hid]
        p = ops.tower_params_struct(t["din"], h0, K * E, hid, D_OUT, t["w_proj"], t["b_proj"], t["w"], t["b"], t["bn_w"], t["bn_b"], rm, rv,
                                    t["w_out"], t["b_out"], bn_nbt=nbt, compute_dtype=ops.TT_BF16,
                                    x_dtype=ops.TT_BF16 if bf else ops.TT_F32, flags=flags, w_proj_bf16=t["w_proj16"], w_bf16=t["w16"])
        x = torch.full((B, kx), -1, dtype=torch.int16 if bf else torch.int32, device=dev)     # NaN patterns: every element must be written
        o = {"x": x, "pre": [torch.full((B, h), float("nan"), device=dev) for h in hid], "act": [torch.empty(B, h, device=dev) for h in hid],
             "mean": [torch.empty(h, device=dev) for h in hid], "rstd": [torch.empty(h, device=dev) for h in hid],
             "y": torch.empty(B, D_OUT, device=dev), "emb": torch.empty(B, D_OUT, device=dev), "rm": rm, "rv": rv}
        a = L.TowerActs()
        a.dense, a.x, a.y, a.emb = dn.data_ptr(), x.data_ptr(), o["y"].data_ptr(), o["emb"].data_ptr()
        for i in range(len(hid)):
            a.pre[i], a.act[i], a.mean[i], a.rstd[i] = o["pre"][i].data_ptr(), o["act"][i].data_ptr(), o["mean"][i].data_ptr(), o["rstd"][i].data_ptr()
        if gather:
            a.gather_table, a.gather_rows, a.gather_K, a.gather_E = table.data_ptr(), rows.data_ptr() + 4 * base, K, E
        xv = x.view(torch.bfloat16 if bf else torch.float32)[:, h0:]
        ids = rows[base:base + B * K].to(torch.int64) if ids_lookup else None
        sides.append(ops.LookupSide(ids, torch.zeros(K, dtype=torch.int64, device=dev) if ids_lookup else None,
                                    torch.full((K,), table.shape[0], dtype=torch.int64, device=dev) if ids_lookup else None, xv, K))
        base += B * K
        params.append(p); acts.append(a); outs.append(o); keep.append((rm, rv, nbt))
    says = ops.towers_fwd_gathers(params, acts, B, True)
    if gather and not says:
        return says, None
    ws, _, _ = ops._tower_workspaces(params, B, dev)
    ws.zero_()
    if not gather:
        if ids_lookup:
            ops.embed_lookup(table, sides, B, want_rows=False)
        else:
            ops.embed_lookup_rows(table, rows, sides, B)
    ops.towers_fwd(params, acts, B, True, 0.1, 77, dev)
    torch.cuda.synchronize()
    res = {"ws": ws.cpu().numpy().copy()}
    for n, o in enumerate(outs):
        for k, v in o.items():
            for i, u in enumerate(v if isinstance(v, list) else [v]):
                res[f"{n}.{k}.{i}"] = u.cpu().numpy().copy()
    return says, res


def _inputs(g, towers, B, E, R, pattern):
    """A table that is the tail of its buffer, slot-order fused rows of all towers, dense features"""
    dev = torch.device(DEV)
    table = torch.randn(R * E + 512, generator=g).to(dev)[512:].view(R, E)
    n = sum(B * t["K"] for t in towers)
    rows = torch.randint(0, R, (n,), generator=g, dtype=torch.int64)
    rows[::7], rows[3::11] = 0, R - 1                                   # the table's first row and its last
    rows[0], rows[-1] = R - 1, R - 1
    if pattern == "one_row":
        rows[:] = R - 4
    dense = [torch.randn(B, t["din"], generator=g).to(dev) for t in towers]
    return table, rows.to(torch.int32).to(dev), dense


#                 B     E   towers (K, h0, din, H)                      rows
CASES = [
    pytest.param(64, 32, [(32, 128, 256, 64), (6, 128, 128, 64)], "random", id="B64-E32-K32+K6-h128"),
    pytest.param(65, 32, [(32, 128, 256, 64), (6, 128, 128, 64)], "random", id="B65-E32-K32+K6-h128"),
    pytest.param(190, 8, [(4, 32, 64, 64), (12, 32, 128, 33)], "random", id="B190-E8-kx64+kx128-h32"),
    pytest.param(300, 16, [(6, 32, 64, 64), (26, 32, 192, 40)], "random", id="B300-E16-kx128+kx448-h32"),
    pytest.param(190, 64, [(1, 64, 64, 64), (5, 128, 256, 64)], "random", id="B190-E64-K1+kx448-h64+h128"),
    pytest.param(300, 32, [(1, 32, 64, 48), (13, 32, 192, 64)], "one_row", id="B300-E32-K1-kx64+kx448-onerow"),
    pytest.param(65, 32, [(3, 96, 128, 64)], "one_row", id="B65-E32-one-tower-h96"),
    pytest.param(8257, 32, [(6, 128, 64, 64), (1, 32, 64, 17)], "random", id="B8257-two-blocks-per-chunk"),
]


@pytest.mark.parametrize("B,E,specs,pattern", CASES)
def test_front_gather_equals_lookup_then_front(B, E, specs, pattern):
    """The gathering front == tt_embed_lookup_rows_fwd + the front reading x: x whole, pre, the chunk partials (the tower
    workspace, zeroed before either run) and all the tail makes of them, bit for bit."""
    g = torch.Generator().manual_seed(1000 + B + E)
    towers = [_tower(g, K, E, h0, din, [H], torch.bfloat16) for K, h0, din, H in specs]
    table, rows, dense = _inputs(g, towers, B, E, 997, pattern)
    no, two = _run(towers, table, rows, dense, B, E, gather=False)
    yes, one = _run(towers, table, rows, dense, B, E, gather=True)
    assert not no and yes                       # (without the fields there is nothing to gather; with them these shapes qualify)
    assert set(one) == set(two)
    for k in two:
        assert np.array_equal(one[k], two[k]), k
    for n in range(len(towers)):                # every element of pre was written, and x holds the table's rows
        assert not np.isnan(one[f"{n}.pre.0"]).any() and np.isfinite(one[f"{n}.emb.0"]).all()
    K0, h0 = specs[0][0], specs[0][1]
    ref = table[rows[:B * K0].long()].view(B, K0 * E).to(torch.bfloat16).cpu()
    assert torch.equal(torch.from_numpy(one["0.x.0"]).view(torch.bfloat16)[:, h0:], ref)


def test_front_gather_escape_hatch():
    """TT_TOWER_UNFUSED_GATHER: the predicate answers 0 for shapes it otherwise takes"""
    g = torch.Generator().manual_seed(5)
    towers = [_tower(g, 6, 32, 128, 64, [64], torch.bfloat16)]
    table, rows, dense = _inputs(g, towers, 64, 32, 101, "random")
    says, res = _run(towers, table, rows, dense, 64, 32, gather=True, flags=L.TT_TOWER_UNFUSED_GATHER)
    assert not says and res is None


@pytest.mark.parametrize("E,K,h0,din,hidden,x_dtype", [
    pytest.param(12, 8, 32, 64, [64], torch.bfloat16, id="E12"),
    pytest.param(32, 6, 128, 64, [64], torch.float32, id="f32-x"),
    pytest.param(32, 6, 128, 96, [64], torch.bfloat16, id="din96"),
    pytest.param(32, 6, 128, 64, [64, 64], torch.bfloat16, id="two-hidden-blocks"),
])
def test_front_gather_refusals(E, K, h0, din, hidden, x_dtype):
    """Shapes the gathering front does not take: the predicate says so, and the two launches run as they always did"""
    B = 130
    g = torch.Generator().manual_seed(9)
    towers = [_tower(g, K, E, h0, din, hidden, x_dtype)]
    table, rows, dense = _inputs(g, towers, B, E, 101, "random")
    says, res = _run(towers, table, rows, dense, B, E, gather=True)
    assert not says and res is None
    says, res = _run(towers, table, rows, dense, B, E, gather=False, ids_lookup=True)
    assert not says
    ref = table[rows.long()].view(B, K * E).to(x_dtype).cpu()
    assert torch.equal(torch.from_numpy(res["0.x.0"]).view(x_dtype)[:, h0:], ref)
    assert np.isfinite(res["0.emb.0"]).all()


# ---------------------------------------------------------------------------------------------- the whole captured step
def _make_task(tt, cfg, meta, **kw):
    return tt.create_two_tower_train_task(
        cfg["keys_n"], cfg["keys_c"], metadata_path=str(meta), categorical_embedding_dim=cfg["E"], notice_dense_input_dim=cfg["din_n"],
        company_dense_input_dim=cfg["din_c"], tower_hidden_dims=list(cfg["hidden"]), final_embedding_dim=cfg["D"],
        dropout_rate=kw.pop("dropout_rate", 0.0), temperature=cfg["T"], device=DEV, **kw)


def _to_batch(tt, b, keys_n, keys_c):
    return {"notice": {"dense": torch.from_numpy(b["notice_dense"]).to(DEV), "kjt": tt.build_batch_kjt(torch.from_numpy(b["notice_ids"]), keys_n).to(DEV)},
            "company": {"dense": torch.from_numpy(b["company_dense"]).to(DEV), "kjt": tt.build_batch_kjt(torch.from_numpy(b["company_ids"]), keys_c).to(DEV)}}


def _steps(tt, cfg, batches, state, on, unroll, monkeypatch):
    from jodalrob_twotower_amd.graph import GraphedTrainStep
    from jodalrob_twotower_amd.optim import FusedAdam
    from jodalrob_twotower_amd.unrolled import UnrolledTrainStep
    monkeypatch.setattr(_cfg.settings, "front_gather", on)
    task = _make_task(tt, cfg, GOLD / "real_vocab_metadata.csv", embedding_grad="sparse", score_dtype="bf16", mlp_dtype="bf16", dropout_rate=0.1)
    task.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in state.items()})
    task.train()
    task._pair_check_done = True
    for tw in (task.two_tower_model.notice_tower, task.two_tower_model.company_tower):
        tw._seed_override = 4242                 # (a capture bakes a host seed, to which the ring's per-step word is added)
    opt = FusedAdam.for_task(task, lr=1e-2)
    tb = [_to_batch(tt, b, cfg["keys_n"], cfg["keys_c"]) for b in batches]
    seen, plain = [], ops.embed_lookup_rows
    monkeypatch.setattr(ops, "embed_lookup_rows", lambda *a, **k: (seen.append(1), plain(*a, **k))[1])
    losses = []
    if unroll == 1:
        gs = GraphedTrainStep(task, opt, tb[0], warmup=1)
        for i, b in enumerate(tb):
            torch.manual_seed(1000 + i)          # the ring draws the step's dropout seed from torch's CPU generator
            losses.append(gs.step(b)["loss"].item())
    else:
        gs = UnrolledTrainStep(task, opt, tb[0], unroll=unroll, warmup=1)
        nxt = [0]

        def after_each():
            nxt[0] += 1
            torch.manual_seed(1000 + nxt[0])
        for i in range(0, len(tb), unroll):
            torch.manual_seed(1000 + i)
            nxt[0] = i
            losses += [r["loss"].item() for r in gs.step_many(tb[i:i + unroll], after_each=after_each)]
    torch.cuda.synchronize()
    monkeypatch.setattr(ops, "embed_lookup_rows", plain)
    out = (losses, {k: v.detach().cpu().numpy().copy() for k, v in task.state_dict().items()}, gs.library_launches, len(seen))
    gs.close()
    return out


@pytest.mark.parametrize("B,unroll", [(128, 1), (190, 1), (190, 2)])
def test_captured_step_front_gather_on_equals_off(manifest, schema_real, monkeypatch, B, unroll):
    """Replayed training steps (real 32 + 6 key layout, dropout 0.1) with settings.front_gather on == off: losses and the whole
    state_dict bit for bit, one library launch fewer per step, and no lookup launch made with the setting on."""
    import jodalrob_twotower_amd as tt
    cfg = dict(manifest["cases"]["real_schema"])
    cfg.update(keys_n=schema_real["notice"]["categorical"], keys_c=schema_real["company"]["categorical"])
    vn, vc = schema_real["notice"]["vocab_sizes"], schema_real["company"]["vocab_sizes"]
    n_steps = 3 if unroll == 1 else 4
    batches = [synth_batch_numpy(B, vn, vc, cfg["din_n"], cfg["din_c"], 1200 + i, oob=True) for i in range(n_steps)]
    state = init_state_numpy({k: tuple(v) for k, v in manifest["state_dict_keys_real"].items()}, 1201)
    off = _steps(tt, cfg, batches, state, False, unroll, monkeypatch)
    on = _steps(tt, cfg, batches, state, True, unroll, monkeypatch)
    assert len(set(off[0])) == n_steps and off[0] == on[0], (off[0], on[0])
    for k, v in off[1].items():
        assert np.array_equal(v, on[1][k], equal_nan=True), k
    assert off[3] > 0 and on[3] == 0
    assert on[2] == off[2] - 1, (on[2], off[2])
