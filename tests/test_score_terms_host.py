"""The score node's one rule table (two_tower_train_task._score_terms_check) over the full matrix score_dtype x every subset of the
optional terms {lq, ent, pw, extras, cells} x {ent_x, lq_x} where extras are present: the accepted combinations and every refusal's
type and text are those of the three forwards the node had before they were folded (plain / extras / cells).  The expectation below
is data, written from that code: per path, its refusals in the order it decided them -- the first row that matches a combination names
its message, a combination no row matches is accepted.  No device, no tensors."""
import itertools

import pytest

DTYPES = ("fp32", "bf16", "bf16x3", "fp8")
TERMS = ("lq", "ent", "pw", "extras", "cells")

CELLS_ENT = "masked cells do not combine with the repeated-entity mask (cells built from the pair table hold every repeat)"
LQX = "the extras carry log_q but the batch is not corrected"
ENTX = "the extras' entity ids are compared with the batch's company ids: ent_c is missing"
HINT2 = " (score_dtype 'bf16' or 'fp32')"

# (all of these present, none of these present, any of these present or None, the score_dtypes the row covers, message; {d}: the dtype)
REFUSALS = (
    # a call with cells (the cells forward)
    ({"cells"}, set(), {"ent", "ent_x"}, DTYPES, CELLS_ENT),
    ({"cells"}, set(), None, ("fp32", "bf16x3", "fp8"), "masked cells have no {d} form (score_dtype 'bf16')"),
    ({"cells", "pw"}, set(), None, DTYPES, "masked cells do not combine with pair weights"),
    ({"cells", "lq_x"}, {"lq"}, None, DTYPES, LQX),
    # a call with extras and no cells (the extras forward)
    ({"extras"}, {"cells"}, None, ("bf16x3", "fp8"), "extra negatives have no {d} form" + HINT2),
    ({"extras", "pw"}, {"cells"}, None, DTYPES, "extra negatives do not combine with pair weights"),
    ({"extras", "ent_x"}, {"cells", "ent"}, None, DTYPES, ENTX),
    ({"extras", "lq_x"}, {"cells", "lq"}, None, DTYPES, LQX),
    # neither (the plain forward): the mask, then pair weights, then logQ
    ({"ent"}, {"cells", "extras"}, None, ("bf16x3", "fp8"), "the repeated-entity mask has no {d} form" + HINT2),
    ({"pw"}, {"cells", "extras"}, None, ("bf16x3", "fp8"), "pair weights have no {d} form" + HINT2),
    ({"lq"}, {"cells", "extras"}, None, ("fp8",), "the logQ correction has no fp8 form"),
)
N_COMBINATIONS = 4 * (16 + 16 * 4)         # per dtype: 16 subsets without extras, 16 with, those x {ent_x} x {lq_x}
N_ACCEPTED = 17 + (17 + 5) + 2 + 1         # fp32; bf16 without / with cells; bf16x3: {} and {lq}; fp8: {}

# the square rule, per term that has it (logQ has none in the node): non-square shapes of an otherwise accepted call
NOT_SQUARE = (
    ("bf16", {"cells"}, "masked cells need as many notice rows as company rows"),
    ("bf16", {"cells", "extras", "lq"}, "masked cells need as many notice rows as company rows"),
    ("fp32", {"extras"}, "extra negatives need as many notice rows as company rows"),
    ("bf16", {"extras", "ent", "ent_x"}, "extra negatives need as many notice rows as company rows"),
    ("bf16", {"ent"}, "the repeated-entity mask needs as many notice rows as company rows"),
    ("fp32", {"ent", "pw", "lq"}, "the repeated-entity mask needs as many notice rows as company rows"),
    ("bf16", {"pw", "lq"}, "pair weights need as many notice rows as company rows"),
    ("bf16x3", {"lq"}, None),
    ("bf16", set(), None),
)


def _expected(dtype, present):
    for need, absent, any_of, dtypes, msg in REFUSALS:
        if need <= present and not (absent & present) and (any_of is None or any_of & present) and dtype in dtypes:
            return msg.format(d=dtype)
    return None


def _matrix():
    for dtype in DTYPES:
        for r in range(len(TERMS) + 1):
            for sub in itertools.combinations(TERMS, r):
                riders = [()] if "extras" not in sub else [(), ("ent_x",), ("lq_x",), ("ent_x", "lq_x")]
                for extra in riders:
                    yield dtype, frozenset(sub + extra)


def _present(terms):
    """the node's names: 'ent' in the matrix stands for both sides' ids"""
    return frozenset(terms | ({"ent_c"} if "ent" in terms else set()))


def test_terms_matrix():
    from jodalrob_twotower_amd.two_tower_train_task import _score_terms_check
    cases = list(_matrix())
    assert len(cases) == len(set(cases)) == N_COMBINATIONS
    accepted = 0
    for dtype, terms in cases:
        want = _expected(dtype, terms)
        if want is None:
            _score_terms_check(dtype, True, _present(terms))
            accepted += 1
            continue
        with pytest.raises(ValueError) as e:
            _score_terms_check(dtype, True, _present(terms))
        assert str(e.value) == want, (dtype, sorted(terms))
    assert accepted == N_ACCEPTED


def test_expectation_spot_checks():
    """the table above read back at combinations written out in full"""
    f = lambda d, *t: _expected(d, frozenset(t))
    assert f("fp8") is None and f("bf16x3", "lq") is None and f("fp32", "lq", "ent", "pw") is None
    assert f("bf16", "cells", "extras", "lq", "lq_x") is None and f("fp32", "extras", "ent", "lq", "ent_x", "lq_x") is None
    assert f("fp8", "lq") == "the logQ correction has no fp8 form"
    assert f("fp8", "lq", "ent", "pw") == "the repeated-entity mask has no fp8 form (score_dtype 'bf16' or 'fp32')"
    assert f("bf16x3", "pw", "lq") == "pair weights have no bf16x3 form (score_dtype 'bf16' or 'fp32')"
    assert f("fp32", "cells") == "masked cells have no fp32 form (score_dtype 'bf16')"
    assert f("fp32", "cells", "ent", "pw") == CELLS_ENT and f("bf16", "cells", "extras", "ent_x") == CELLS_ENT
    assert f("bf16", "cells", "pw") == "masked cells do not combine with pair weights"
    assert f("fp8", "extras", "pw") == "extra negatives have no fp8 form (score_dtype 'bf16' or 'fp32')"
    assert f("bf16", "extras", "pw", "ent") == "extra negatives do not combine with pair weights"
    assert f("bf16", "extras", "ent_x", "lq_x") == ENTX and f("bf16", "extras", "ent", "ent_x", "lq_x") == LQX
    assert f("bf16", "cells", "extras", "lq_x") == LQX


@pytest.mark.parametrize("dtype,terms,want", NOT_SQUARE)
def test_square_rule(dtype, terms, want):
    from jodalrob_twotower_amd.two_tower_train_task import _score_terms_check
    _score_terms_check(dtype, True, _present(terms))
    if want is None:
        _score_terms_check(dtype, False, _present(terms))
        return
    with pytest.raises(ValueError) as e:
        _score_terms_check(dtype, False, _present(terms))
    assert str(e.value) == want


def test_validators_share_the_table():
    """the task's batch validators decide with the node's table: a term the node has a form of is one a batch may carry"""
    from jodalrob_twotower_amd import two_tower_train_task as T
    assert {t: set(d) for t, d in T._TERM_FORMS.items()} == {
        "cells": {"bf16"}, "extras": {"fp32", "bf16"}, "ent": {"fp32", "bf16"}, "pw": {"fp32", "bf16"}, "lq": {"fp32", "bf16", "bf16x3"}}
    clashes = {(a, b) for a in TERMS for b in TERMS if a < b and T._terms_clash(a, b)}
    assert clashes == {("cells", "ent"), ("cells", "pw"), ("extras", "pw")}


@pytest.mark.parametrize("dtype", DTYPES)
def test_node_refuses_unequal_row_counts(dtype):
    """the node's own refusal (the table above answers for the terms only: a plain call passes it at any shape) -- on CPU tensors,
    before anything is packed or launched: the library is not even loaded"""
    import torch
    from jodalrob_twotower_amd import _lib
    from jodalrob_twotower_amd.two_tower_train_task import _ScoreCEFn
    loaded = _lib._lib
    for rows_n, rows_c in ((4, 3), (3, 4)):
        with pytest.raises(ValueError) as e:
            _ScoreCEFn.apply(torch.zeros(rows_n, 8), torch.zeros(rows_c, 8), 1.0, dtype)
        assert str(e.value) == f"the score node needs as many notice rows as company rows, got {rows_n} and {rows_c}"
    assert _lib._lib is loaded
