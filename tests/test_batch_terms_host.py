"""Host-side checks of the batch entries that change the loss (batch_terms.TABLE: log_q, entity, pair_weight, negatives, masked_cells)
as the task's one validator and the captured steps decide on them -- no device.  Every refusal is held to its exception type and its
whole text; the texts stand here as written out, not as the table forms them."""
import re
from types import SimpleNamespace

import pytest
import torch

from test_known_mask_host import _cpu_batch, _cpu_task

B, M = 6, 3
KEYS = ("log_q", "entity", "pair_weight", "negatives", "masked_cells")
SAY = {"log_q": "the logQ correction (a batch with 'log_q') is", "entity": "the repeated-entity mask (a batch with 'entity') is",
       "pair_weight": "pair weights (a batch with 'pair_weight') are", "negatives": "extra negatives (a batch with 'negatives') are",
       "masked_cells": "masked cells (a batch with 'masked_cells') are"}
NO_FORM = {"log_q": ("fp8",), "entity": ("fp8", "bf16x3"), "pair_weight": ("fp8", "bf16x3"), "negatives": ("fp8", "bf16x3"),
           "masked_cells": ("fp32", "fp8", "bf16x3")}
# the arrays: (name in the task's texts, name in the captured step's, "a <dtype>", dtype, a wrong dtype, shape in the texts)
ARRAYS = {"log_q": ("batch['notice']['log_q']", "notice log_q", "a float32", torch.float32, torch.float64, "[6]"),
          "entity": ("batch['notice']['entity']", "notice entity", "an int32", torch.int32, torch.int64, "[6]"),
          "pair_weight": ("batch['pair_weight']", "pair_weight", "a float32", torch.float32, torch.float64, "[6]"),
          "negatives": ("batch['negatives']['log_q']", None, "a float32", torch.float32, torch.float64, "[3]"),
          "masked_cells": ("batch['masked_cells']", "masked_cells", "an int32", torch.int32, torch.int64, "[L, 2]")}
CLASHES = {("masked_cells", "entity"): "masked cells (a batch with 'masked_cells') do not combine with 'entity': cells built from the pair table "
                                       "already hold every repeat",
           ("masked_cells", "pair_weight"): "masked cells (a batch with 'masked_cells') do not combine with 'pair_weight'",
           ("negatives", "pair_weight"): "extra negatives (a batch with 'negatives') do not combine with 'pair_weight'"}
MISMATCH = {"log_q": ("log_q mismatch: the step was captured with a log_q, the batch has none",
                      "log_q mismatch: the step was captured without a log_q, the batch carries one"),
            "entity": ("entity mismatch: the step was captured with entity ids, the batch has none",
                       "entity mismatch: the step was captured without entity ids, the batch carries them"),
            "pair_weight": ("pair_weight mismatch: the step was captured with pair weights, the batch has none",
                            "pair_weight mismatch: the step was captured without pair weights, the batch carries them"),
            "negatives": ("negatives mismatch: the step was captured with extra negatives, the batch has none",
                          "negatives mismatch: the step was captured without extra negatives, the batch carries them"),
            "masked_cells": ("masked_cells mismatch: the step was captured with masked cells, the batch has none",
                             "masked_cells mismatch: the step was captured without masked cells, the batch carries them")}
STORE_MISMATCH = {"log_q": ("log_q mismatch: the step was captured with a log_q, step_from_store got none",
                            "log_q mismatch: the step was captured without a log_q, step_from_store got one"),
                  "entity": ("entity mismatch: the step was captured with entity ids, step_from_store got none",
                             "entity mismatch: the step was captured without entity ids, step_from_store got them"),
                  "pair_weight": ("pair_weight mismatch: the step was captured with pair weights, step_from_store has none",
                                  "pair_weight mismatch: the step was captured without pair weights, step_from_store carries them")}
NO_STORE = {"negatives": "extra negatives: no store-fed hand-over -- a step captured with 'negatives' takes step(batch)",
            "masked_cells": "masked cells: no store-fed hand-over -- a step captured with 'masked_cells' takes step(batch)"}
DENSE = " not supported by the dense loss path (label_smoothing != 0 or loss_type='cosine_embedding')"

_TASKS = {}


def _task(score_dtype="bf16"):
    if score_dtype not in _TASKS:
        _TASKS[score_dtype] = _cpu_task(score_dtype=score_dtype)
    return _TASKS[score_dtype]


def _good(key, n=B):
    dt = ARRAYS[key][3]
    return torch.zeros((4, 2), dtype=dt) if key == "masked_cells" else torch.zeros(M if key == "negatives" else n, dtype=dt)


def _bad_arrays(key, n):
    """(array, what the text says it got): a wrong dtype, a wrong rank, a wrong length, no tensor"""
    dt, wrong = ARRAYS[key][3:5]
    if key == "masked_cells":
        return [(torch.zeros((4, 2), dtype=wrong), "torch.int64 [4, 2]"), (torch.zeros(4, dtype=dt), "torch.int32 [4]"),
                (torch.zeros((4, 3), dtype=dt), "torch.int32 [4, 3]"), ([[0, 1]], "list []")]
    return [(torch.zeros(n, dtype=wrong), f"{wrong} [{n}]"), (torch.zeros((n, 1), dtype=dt), f"{dt} [{n}, 1]"),
            (torch.zeros(n + 1, dtype=dt), f"{dt} [{n + 1}]"), ([0] * n, "list []")]


def _batch(**entries):
    """a CPU batch of B rows with the entries under their keys; a value of ... stands for a valid one.  Per-side entries go to the notice
    side; "negatives": a valid company-side input of M rows -- a value other than ...: its "log_q" (the batch's own log_q rides along)"""
    from jodalrob_twotower_amd.kjt import KeyedJaggedTensor
    b = _cpu_batch(B)
    for key, v in entries.items():
        v = _good(key) if v is ... else v
        if key in ("log_q", "entity"):
            b["notice"][key] = v
        elif key == "negatives":
            keys = list(_task().two_tower_model.company_tower.categorical_embedder.keys)
            b["company"]["kjt"] = KeyedJaggedTensor(keys, torch.zeros(B * len(keys), dtype=torch.int64))
            b[key] = {"dense": torch.zeros(M, 8), "kjt": KeyedJaggedTensor(keys, torch.zeros(M * len(keys), dtype=torch.int64))}
            if entries[key] is not ...:
                b["company"]["log_q"], b[key]["log_q"] = torch.zeros(B), v
        else:
            b[key] = v
    return b


def _raises(exc, text):
    return pytest.raises(exc, match="^" + re.escape(text) + "$")


def test_the_table_is_these_five_in_this_order():
    from jodalrob_twotower_amd import batch_terms as T
    from jodalrob_twotower_amd import two_tower_train_task as task_module
    assert tuple(row.key for row in T.TABLE) == KEYS and [row.term for row in T.TABLE] == ["lq", "ent", "pw", "extras", "cells"]
    assert task_module._TERM_FORMS is T._TERM_FORMS and task_module._TERM_CLASHES is T._TERM_CLASHES and task_module._terms_clash is T._terms_clash
    assert T.present(_cpu_batch(B)) == frozenset()
    for key in KEYS:
        assert T.present(_batch(**{key: ...})) >= {key}


# ---- the task's validator ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", KEYS)
def test_task_array_checks(key):
    name, _, a_dtype, _, _, shape = ARRAYS[key]
    good = _good(key)
    for bad, got in _bad_arrays(key, M if key == "negatives" else B):
        with _raises(ValueError, f"{name} must be {a_dtype} tensor of shape {shape}, got {got}"):
            _task()._batch_terms(_batch(**{key: bad}), B)
    with _raises(ValueError, f"{name} is on meta, the batch on cpu"):
        _task()._batch_terms(_batch(**{key: good.to("meta")}), B)
    got = _task()._batch_terms(_batch(**{key: good}), B)
    assert [f for f in got._fields if getattr(got, f) is not None] == \
        {"log_q": ["lq"], "entity": ["ent"], "pair_weight": ["pw"], "negatives": ["lq", "neg"], "masked_cells": ["cells"]}[key]


def test_task_array_checks_of_the_extras_entity_ids():
    b = _batch(negatives=...)
    b["company"]["entity"] = torch.zeros(B, dtype=torch.int32)
    b["negatives"]["entity"] = torch.zeros(M, dtype=torch.int64)
    with _raises(ValueError, "batch['negatives']['entity'] must be a int32 tensor of shape [3], got torch.int64 [3]"):
        _task()._batch_terms(b, B)
    b["negatives"]["entity"] = torch.zeros(M, dtype=torch.int32)
    del b["company"]["entity"]
    with _raises(ValueError, "batch['negatives']['entity'] needs batch['company']['entity']: the extras' entity has nothing to be compared with"):
        _task()._batch_terms(b, B)
    with _raises(ValueError, "batch['masked_cells_count'] must be an int32 tensor of one element on cpu"):
        _task()._batch_terms(dict(_batch(masked_cells=...), masked_cells_count=torch.zeros(1)), B)


def test_task_values_are_what_the_node_takes():
    lq, ent, w = torch.ones(B), torch.arange(B, dtype=torch.int32), torch.ones(B)
    b = _cpu_batch(B, pair_weight=w)
    b["company"]["log_q"], b["company"]["entity"] = lq, ent
    t = _task()._batch_terms(b, B)
    assert torch.equal(t.lq[0], torch.zeros(B)) and t.lq[1] is lq                 # a missing side's log q: zeros
    assert t.ent[0] is None and t.ent[1] is ent                                   # a missing side's ids: None (all-distinct)
    assert t.pw is w and t.neg is None and t.cells is None
    count = torch.zeros(1, dtype=torch.int32)
    cells = _good("masked_cells")
    assert _task()._batch_terms(dict(_batch(masked_cells=cells), masked_cells_count=count), B).cells == (cells, count)


@pytest.mark.parametrize("key", KEYS)
def test_task_refuses_dense_loss_missing_forms_and_what_it_does_not_take(key):
    dense = _cpu_task(score_dtype="bf16")
    dense._dense_loss = True
    with _raises(ValueError, SAY[key] + DENSE):
        dense._batch_terms(_batch(**{key: ...}), B)
    for dt in NO_FORM[key]:
        with _raises(ValueError, f"{SAY[key]} not supported for score_dtype='{dt}'"):
            _task(dt)._batch_terms(_batch(**{key: ...}), B)
    for dt in {"fp32", "bf16", "bf16x3", "fp8"} - set(NO_FORM[key]):
        _task(dt)._batch_terms(_batch(**{key: ...}), B)
    refusing = _cpu_task(score_dtype="bf16")
    refusing._refused = frozenset({key})
    with _raises(NotImplementedError, f"{SAY[key]} not supported by TwoTowerTrainTask"):
        refusing._batch_terms(_batch(**{key: ...}), B)
    dense._refused = frozenset({key})                              # "may this task take it" comes before the dense loss
    with _raises(NotImplementedError, f"{SAY[key]} not supported by TwoTowerTrainTask"):
        dense._batch_terms(_batch(**{key: ...}), B)


@pytest.mark.parametrize("pair", sorted(CLASHES))
def test_task_refuses_each_clash(pair):
    from jodalrob_twotower_amd import batch_terms as T
    assert {frozenset(T.ROWS[k].term for k in p) for p in CLASHES} == set(T._TERM_CLASHES)
    with _raises(ValueError, CLASHES[pair]):
        _task()._batch_terms(_batch(**{k: ... for k in pair}), B)
    if pair[0] == "masked_cells":                                  # the clash comes before the score_dtype's form
        with _raises(ValueError, CLASHES[pair]):
            _task("fp32")._batch_terms(_batch(**{k: ... for k in pair}), B)


def test_task_with_two_refusable_entries_raises_the_first_decided():
    """the entries are decided in the table's order, each to its end"""
    with _raises(ValueError, SAY["log_q"] + " not supported for score_dtype='fp8'"):
        _task("fp8")._batch_terms(_batch(log_q=..., entity=...), B)
    with _raises(ValueError, SAY["entity"] + " not supported for score_dtype='bf16x3'"):
        _task("bf16x3")._batch_terms(_batch(log_q=..., entity=..., pair_weight=...), B)
    with _raises(ValueError, "batch['pair_weight'] must be a float32 tensor of shape [6], got torch.float64 [6]"):
        _task()._batch_terms(_batch(pair_weight=torch.zeros(B, dtype=torch.float64), masked_cells=...), B)
    with _raises(ValueError, SAY["negatives"] + " not supported for score_dtype='fp8'"):
        _task("fp8")._batch_terms(_batch(negatives=..., masked_cells=...), B)
    with _raises(ValueError, SAY["masked_cells"] + " not supported for score_dtype='fp32'"):
        _task("fp32")._batch_terms(_batch(negatives=..., masked_cells=...), B)
    with _raises(ValueError, "batch['negatives']['log_q'] must be a float32 tensor of shape [3], got torch.float64 [3]"):
        _task()._batch_terms(_batch(negatives=torch.zeros(M, dtype=torch.float64), masked_cells=torch.zeros(3)), B)
    sharded = _cpu_task(score_dtype="bf16")
    sharded._refused = frozenset({"negatives", "masked_cells"})
    with _raises(NotImplementedError, SAY["negatives"] + " not supported by TwoTowerTrainTask"):
        sharded._batch_terms(_batch(negatives=..., masked_cells=...), B)
    with _raises(ValueError, "batch['notice']['log_q'] must be a float32 tensor of shape [6], got torch.float64 [6]"):
        sharded._batch_terms(_batch(log_q=torch.zeros(B, dtype=torch.float64), masked_cells=...), B)


def test_sharded_task_and_evaluation_refusals():
    from jodalrob_twotower_amd.distributed import DistributedTwoTowerTrainTask
    from jodalrob_twotower_amd.two_tower_train_task import TwoTowerTrainTask
    assert TwoTowerTrainTask._refused == frozenset() and DistributedTwoTowerTrainTask._refused == {"negatives", "masked_cells"}
    given = {"log_q": (torch.zeros(B), torch.zeros(B)), "entity": (torch.zeros(B, dtype=torch.int32), None), "pair_weight": torch.ones(B)}
    for key, kw in (("log_q", "log_q"), ("entity", "entity"), ("pair_weight", "pair_weight")):
        with _raises(NotImplementedError, f"{SAY[key]} not supported by the sharded task"):
            DistributedTwoTowerTrainTask._score_ce(None, None, None, 1.0, False, **{kw: given[key]})
    with _raises(NotImplementedError, SAY["pair_weight"] + " not supported by the sharded task"):      # pair_weight, log_q, entity
        DistributedTwoTowerTrainTask._score_ce(None, None, None, 1.0, False, **given)
    with _raises(NotImplementedError, SAY["log_q"] + " not supported by the sharded task"):
        DistributedTwoTowerTrainTask._score_ce(None, None, None, 1.0, False, log_q=given["log_q"], entity=given["entity"])
    why = {"pair_weight": "evaluation is unweighted", "negatives": "evaluation ranks the batch's own companies",
           "masked_cells": "evaluation filters with exclusion lists"}
    for key, text in why.items():
        with _raises(ValueError, f"forward_with_ranks does not take a batch with '{key}' ({text})"):
            TwoTowerTrainTask.forward_with_ranks(None, _cpu_batch(B, **{key: _good(key)}))
    with _raises(ValueError, "forward_with_ranks does not take a batch with 'pair_weight' (evaluation is unweighted)"):
        TwoTowerTrainTask.forward_with_ranks(None, _cpu_batch(B, masked_cells=_good("masked_cells"), negatives={}, pair_weight=torch.ones(B)))


# ---- the captured steps --------------------------------------------------------------------------------------------------------------
def _example(key):
    ex = {"notice": {"dense": torch.zeros(4, 2)}, "company": {"dense": torch.zeros(4, 2)}}
    if key is None:
        return ex
    if key in ("log_q", "entity"):
        ex["company"][key] = _good(key, 4)
    else:
        ex[key] = {"dense": torch.zeros(M, 2)} if key == "negatives" else _good(key, 4)
    return ex


@pytest.mark.parametrize("key", KEYS)
def test_step_constructors_refuse(key):
    from jodalrob_twotower_amd.graph import GraphedTrainStep
    from jodalrob_twotower_amd.segmented import SegmentedTrainStep
    from jodalrob_twotower_amd.unrolled import UnrolledTrainStep
    assert key in GraphedTrainStep._accepts and UnrolledTrainStep._accepts == frozenset() == SegmentedTrainStep._accepts
    sharded = SimpleNamespace(exchange=object())
    for task in (None, sharded):                                   # "not by this class" comes before "not by the sharded task"
        with _raises(NotImplementedError, f"{SAY[key]} not supported by UnrolledTrainStep"):
            UnrolledTrainStep(task, None, _example(key), unroll=2)
        with _raises(NotImplementedError, f"{SAY[key]} not supported by SegmentedTrainStep"):
            SegmentedTrainStep(task, None, _example(key))
    with _raises(NotImplementedError, f"{SAY[key]} not supported by the sharded task"):
        GraphedTrainStep(sharded, None, _example(key))
    if key != "masked_cells":
        with _raises(ValueError, "cell_capacity: the example batch carries no 'masked_cells'"):
            GraphedTrainStep(None, None, _example(key), cell_capacity=8)


def test_step_constructors_refuse_the_first_entry_in_the_tables_order():
    from jodalrob_twotower_amd.graph import GraphedTrainStep
    from jodalrob_twotower_amd.unrolled import UnrolledTrainStep
    ex = dict(_example("masked_cells"), negatives={"dense": torch.zeros(M, 2)}, pair_weight=torch.ones(4))
    with _raises(NotImplementedError, SAY["pair_weight"] + " not supported by UnrolledTrainStep"):
        UnrolledTrainStep(None, None, ex, unroll=2)
    del ex["pair_weight"]
    with _raises(NotImplementedError, SAY["negatives"] + " not supported by the sharded task"):
        GraphedTrainStep(SimpleNamespace(exchange=object()), None, ex)
    ex["company"]["entity"] = _good("entity", 4)
    with _raises(NotImplementedError, SAY["entity"] + " not supported by the sharded task"):
        GraphedTrainStep(SimpleNamespace(exchange=object()), None, ex)


def _step(terms=()):
    """a captured step's stand-in: the entries it was captured with; nothing of the device"""
    from jodalrob_twotower_amd.graph import GraphedTrainStep
    step = object.__new__(GraphedTrainStep)
    step._terms = frozenset(terms)
    step.static = {"notice": {"log_q": torch.zeros(4), "entity": torch.zeros(4, dtype=torch.int32)},
                   "company": {"log_q": torch.zeros(4), "entity": torch.zeros(4, dtype=torch.int32)}, "pair_weight": torch.zeros(4)}
    step._fill = {"log_q": torch.zeros(4), "entity": torch.arange(4, dtype=torch.int32)}
    return step


@pytest.mark.parametrize("key", KEYS)
def test_step_with_without_mismatch_both_ways_on_both_paths(key):
    with_it, without_it = MISMATCH[key]
    with _raises(ValueError, with_it):
        _step([key]).step(_example(None))
    with _raises(ValueError, without_it):
        _step().step(_example(key))
    if key in NO_STORE:
        with _raises(NotImplementedError, NO_STORE[key]):
            _step([key]).step_from_store(None, None, None)
        return
    value = (None, _good(key, 4)) if key in ("log_q", "entity") else _good(key, 4)
    with_it, without_it = STORE_MISMATCH[key]
    with _raises(ValueError, with_it):
        _step([key]).step_from_store(None, None, None)
    with _raises(ValueError, without_it):
        _step().step_from_store(None, None, None, **{key: value})


def test_step_decides_cells_first_then_extras_then_the_tables_order():
    ex = dict(_example("masked_cells"), negatives={"dense": torch.zeros(M, 2)}, pair_weight=torch.ones(4))
    ex["notice"]["log_q"] = torch.zeros(4)
    with _raises(ValueError, MISMATCH["masked_cells"][1]):
        _step().step(ex)
    del ex["masked_cells"]
    with _raises(ValueError, MISMATCH["negatives"][1]):
        _step().step(ex)
    del ex["negatives"]
    with _raises(ValueError, MISMATCH["log_q"][1]):
        _step().step(ex)
    with _raises(ValueError, MISMATCH["pair_weight"][1]):
        _step(["log_q"]).step(ex)
    with _raises(NotImplementedError, NO_STORE["masked_cells"]):
        _step(["masked_cells", "negatives"]).step_from_store(None, None, None, log_q=(None, None))
    with _raises(ValueError, STORE_MISMATCH["log_q"][1]):
        _step().step_from_store(None, None, None, log_q=(None, None), entity=(None, None), pair_weight=torch.ones(4))


@pytest.mark.parametrize("key", ["log_q", "entity", "pair_weight", "masked_cells"])
def test_step_array_checks(key):
    from jodalrob_twotower_amd.graph import GraphedTrainStep
    _, name, a_dtype, dt, _, shape = ARRAYS[key]
    shape = shape.replace("6", "4")
    good = _good(key, 4)

    def run(t):
        if key == "masked_cells":
            return GraphedTrainStep._check_cells(t, torch.device("cpu"), 8)
        return _step([key])._term_pairs(key, (t, None) if key != "pair_weight" else t, "the batch")
    for t, got in _bad_arrays(key, 4):
        with _raises(ValueError, f"{name} must be {a_dtype} tensor of shape {shape}, got {got}"):
            run(t)
    with _raises(ValueError, f"{name} is on meta, the captured step on cpu"):
        run(good.to("meta"))
    if key == "masked_cells":
        with _raises(ValueError, "masked_cells: 9 cells, the step was captured with cell_capacity = 8"):
            run(torch.zeros((9, 2), dtype=dt))
        assert run(good) is good
    else:
        pairs = run(good)
        assert len(pairs) == (1 if key == "pair_weight" else 2) and pairs[0][1] is good and all(dst.dtype == dt for dst, _ in pairs)


def test_missing_side_of_a_captured_entry_is_its_fill():
    step = _step(["log_q", "entity"])
    lq = torch.ones(4)
    (d0, s0), (d1, s1) = step._term_pairs("log_q", (None, lq), "step_from_store")
    assert d0 is step.static["notice"]["log_q"] and s0 is step._fill["log_q"] and d1 is step.static["company"]["log_q"] and s1 is lq
    (_, s0), (_, s1) = step._term_pairs("entity", (None, None), "the batch")
    assert s0 is step._fill["entity"] and s1 is step._fill["entity"] and torch.equal(s0, torch.arange(4, dtype=torch.int32))


def test_aligned_arrays_are_segments_and_misaligned_ones_are_copied_at_once():
    """the copy launch moves 16-byte pieces: a [B] float array sliced at offset 1 is copied at once and is no segment; an aligned one
    is the segment (static buffer, the tensor passed)"""
    from jodalrob_twotower_amd import batch_terms as T
    base = torch.arange(12, dtype=torch.float32)
    assert base.data_ptr() % 16 == 0
    dst = torch.zeros(4)
    off = base[1:5]
    assert off.data_ptr() % 16 == 4 and T.segment(dst, off) == [] and torch.equal(dst, off)
    (d, s), = T.segment(dst, base[4:8])
    assert d is dst and s.data_ptr() == base[4:8].data_ptr() and torch.equal(dst, off)      # (nothing copied yet)
    whole = torch.ones(4)
    (d, s), = T.segment(dst, whole)
    assert d is dst and s is whole
    # through the captured step's path
    step = _step(["pair_weight"])
    assert step._term_pairs("pair_weight", off, "the batch") == [] and torch.equal(step.static["pair_weight"], off)
    (d, s), = step._term_pairs("pair_weight", whole, "the batch")
    assert d is step.static["pair_weight"] and s is whole
