"""Row-wise Adagrad for the tables, host side (no GPU): FusedAdam.for_task's parameter groups, hyper-parameter validation,
and the new C-ABI symbols in the header, the ctypes table and the cross-compiled library."""
import re
from pathlib import Path

import pytest
import torch

import jodalrob_twotower_amd as tt
from jodalrob_twotower_amd import _lib
from jodalrob_twotower_amd.optim import FusedAdam, find_stores

ROOT = Path(__file__).resolve().parents[1]
GOLD = ROOT / "tests" / "golden"
SYMBOLS = ("tt_rowwise_adagrad_sparse_step", "tt_rowwise_adagrad_dense_step", "tt_adam_rowwise_adagrad_fused_step",
           "tt_adam_rowwise_adagrad_fused_step_finish")


def _task():
    return tt.create_two_tower_train_task(["a", "b"], ["c"], metadata_path=str(GOLD / "synthetic_metadata.csv"),
                                          categorical_embedding_dim=8, notice_dense_input_dim=4, company_dense_input_dim=3,
                                          tower_hidden_dims=[16], final_embedding_dim=8, device="cpu")


def test_for_task_groups():
    task = _task()
    table_ids = {id(p) for s in find_stores(task) for p in s.optim_parameters()}
    assert len(table_ids) == 3
    adam = FusedAdam.for_task(task, lr=0.1)
    assert len(adam.param_groups) == 1 and "table_optimizer" not in adam.param_groups[0]
    opt = FusedAdam.for_task(task, table_optimizer="rowwise_adagrad", lr=0.1, weight_decay=1e-5, eps=1e-7)
    towers, tables = opt.param_groups
    assert "table_optimizer" not in towers and tables["table_optimizer"] == "rowwise_adagrad"
    assert {id(p) for p in tables["params"]} == table_ids and not table_ids & {id(p) for p in towers["params"]}
    assert len(towers["params"]) + len(tables["params"]) == len(list(task.parameters()))
    assert (tables["lr"], tables["eps"], tables["weight_decay"]) == (0.1, 1e-8, 1e-5)           # None inherits; eps its own
    assert (towers["lr"], towers["eps"], towers["weight_decay"]) == (0.1, 1e-7, 1e-5)
    opt = FusedAdam.for_task(task, table_optimizer="rowwise_adagrad", lr=0.1, table_lr=0.5, table_eps=1e-6, table_weight_decay=0.0,
                             weight_decay=1e-4)
    assert (opt.param_groups[1]["lr"], opt.param_groups[1]["eps"], opt.param_groups[1]["weight_decay"]) == (0.5, 1e-6, 0.0)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda s: 0.25)                   # scales both groups
    assert [g["lr"] for g in opt.param_groups] == [0.025, 0.125]
    del sched


def test_state_layout_before_a_step():
    task = _task()
    opt = FusedAdam.for_task(task, table_optimizer="rowwise_adagrad", lr=0.1)
    store = find_stores(task)[0]
    st = opt._state_of(store)
    assert set(st) == {"sum", "step"} and tuple(st["sum"].shape) == (store.weight.shape[0],)
    for p in store.optim_parameters():
        assert set(opt.state[p]) == {"step", "sum"} and tuple(opt.state[p]["sum"].shape) == (p.shape[0],)
        assert opt.state[p]["sum"].untyped_storage().data_ptr() == st["sum"].untyped_storage().data_ptr()   # views of one buffer


@pytest.mark.parametrize("kw,msg", [
    (dict(table_optimizer="sgd"), "table_optimizer"),
    (dict(table_optimizer="rowwise_adagrad", table_lr=-1.0), "row-wise Adagrad"),
    (dict(table_optimizer="rowwise_adagrad", table_eps=0.0), "row-wise Adagrad"),
    (dict(table_optimizer="rowwise_adagrad", table_weight_decay=-1e-3), "row-wise Adagrad"),
    (dict(table_lr=0.1), "rowwise_adagrad"),
    (dict(table_weight_decay=0.1), "rowwise_adagrad"),
])
def test_hyper_parameter_validation(kw, msg):
    with pytest.raises(ValueError, match=msg):
        FusedAdam.for_task(_task(), lr=0.1, **kw)


def test_group_mismatch_on_load_raises():
    task = _task()
    adam = FusedAdam.for_task(task, lr=0.1)
    rw = FusedAdam.for_task(task, table_optimizer="rowwise_adagrad", lr=0.1)
    with pytest.raises(ValueError, match="table_optimizer"):
        rw.load_state_dict(adam.state_dict())
    with pytest.raises(ValueError, match="table_optimizer"):
        adam.load_state_dict(rw.state_dict())


def test_symbols_in_header_and_library():
    header = (ROOT / "include" / "twotower.h").read_text()
    lib = _lib.load()
    for name in SYMBOLS:
        assert re.search(rf"\bint {name}\(", header), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
