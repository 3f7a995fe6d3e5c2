"""The inputs tests/test_gpu_score_node_matrix.py feeds the score node, and the condition they are held to; shared with
tests/test_score_node_reference_host.py, which checks that condition on the CPU.  No test lives here and nothing here needs a device.

The matrix is tests/test_score_terms_host.py's (DTYPES x every subset of TERMS x the extras' riders), imported so that the files cannot
drift.  The generators are the term files' own; they draw on their module's DEV, so `_inputs(..., device=)` points the three modules at
another device for the duration of one call (numpy draws the log q, ids, cells and weights: the same values on every device; the unit
rows come from torch's generator of the device: on the CPU they are other draws of the same law, which is why the GPU file repeats the
condition on the device's own rows).
"""
import contextlib

import numpy as np
import torch

import test_gpu_extra_negatives as GX
import test_gpu_known_mask as GK
import test_gpu_logq as GL
from test_gpu_logq import BOUNDS, LOSS_ATOL
from test_score_terms_host import DTYPES, TERMS, _expected, _matrix  # noqa: F401
from _mask_reference import ids
from _pair_weight_reference import weights
import _score_node_reference as NR

SHAPES = [(70, 33, 200, 0.5), (300, 263, 64, 2.0)]
FP8_BOUNDS = (2e-6, 1e-4)                                     # test_score_fp8_vs_rounded_oracle at T >= 0.5: loss rtol, gradients norm-wise
RIDERS = ("ent_x", "lq_x")
ACCEPTED = [(d, t) for d, t in _matrix() if _expected(d, t) is None]
REFUSED = [(d, t) for d, t in _matrix() if _expected(d, t) is not None]
# one-sided ids: 'ent_n' / 'ent_c' name the one side that carries ids ('ent' in the matrix stands for both)
ONE_SIDED = [frozenset(t) for t in (("ent_n",), ("ent_c",), ("ent_n", "extras"), ("ent_c", "extras", "ent_x"))]
N_COMPANIES, LQ_SCALE, HEAVY_PAIRS = 4, 0.4, 8               # _inputs' three departures from the term files' generators, argued there


def _name(terms):
    return "+".join(sorted(terms)) or "plain"


@contextlib.contextmanager
def _generators_on(device):
    """the term files' generators draw on `device` inside the block (None: where they always draw)"""
    mods = (GL, GX, GK) if device is not None else ()
    old = [m.DEV for m in mods]
    for m in mods:
        m.DEV = device
    try:
        yield
    finally:
        for m, d in zip(mods, old):
            m.DEV = d


def _inputs(terms, B, M, D, device=None):
    """The node's inputs of one combination as keyword arguments (n, c and the terms' arrays; None: absent), on the generators' device
    or on `device`.
    terms: the matrix's names ('ent': both sides' ids) or ONE_SIDED's.
      rows     test_gpu_logq._unit_rows, the term files' seeds
      log q    LQ_SCALE times test_gpu_logq._lq "zipf", shifted so that its largest entry is 0.  Why not "random": it hands a row's
               whole sum to the two planted -40s, and no mask that misses them moves the loss.  Why shifted and scaled: log q is clamped
               to [-40, 0], so extras without a log q of their own (zeros) weigh 1 against in-batch weights of 1 / q >= 1 -- under the
               unscaled law (weights up to B^1.1) they hold less than 1e-3 of a row's sum, and neither they nor their ids move the loss;
               at 0.4 of the spread they hold a sixth of it and the correction itself still moves the loss
      ids      _mask_reference.ids "groups", the companies folded to N_COMPANIES ids: an extra's id then masks a quarter of the rows, not
               three of them (the extras' ids must move the loss on their own); the extras' ids from test_gpu_extra_negatives._x_ids
      cells    test_gpu_known_mask._cells: "random" (3 %), "heavy" (row 33 and column 5 fully listed) and "edges" together
      weights  _pair_weight_reference.weights "random", the HEAVY_PAIRS pairs whose positives score lowest B / HEAVY_PAIRS heavier: the
               weighted mean differs from the plain one by the covariance of weight and term, which for weights drawn apart from the
               rows is noise around 0 (measured: 35 loss bounds at B = 300, T = 2); leaning on the pairs with the largest terms gives
               it a sign
    """
    with _generators_on(device):
        return _draw(terms, B, M, D)


def _draw(terms, B, M, D):
    dev = GL.DEV
    kw = dict.fromkeys(("lq_n", "lq_c", "ent_n", "ent_c", "pair_w", "x", "lq_x", "ent_x", "cells"))
    kw["n"], kw["c"] = GL._unit_rows(B, D, 11 + B + D), GL._unit_rows(B, D, 29 + B + D)
    extras = "extras" in terms
    if extras:
        kw["x"] = GL._unit_rows(M, D, 41 + M + D)
    def lq(R, seed):
        q = GL._lq(R, "zipf", seed)
        return LQ_SCALE * (q - q.max())
    if "lq" in terms:
        kw["lq_n"], kw["lq_c"] = lq(B, 3 + B), lq(B, 5 + D)
    if "lq_x" in terms:
        kw["lq_x"] = lq(M, 7 + M)
    if terms & {"ent", "ent_n", "ent_c", "ent_x"}:
        en, ec = ids(B, "groups", seed=B, device=dev)
        ec = ec % N_COMPANIES
        if terms & {"ent", "ent_n"}:
            kw["ent_n"] = en
        if terms & {"ent", "ent_c"}:
            kw["ent_c"] = ec
        if "ent_x" in terms:                                 # (without the companies' ids: a refused call)
            kw["ent_x"] = GX._x_ids(ec, M, M)
    if "cells" in terms:
        m = M if extras else 0
        cells = np.concatenate([GK._cells(B, m, p) for p in ("random", "heavy", "edges")], 0)
        kw["cells"] = torch.as_tensor(cells, dtype=torch.int32, device=dev)
    if "pw" in terms:
        w = weights(B, "random", seed=B, device=dev)
        w[torch.argsort((kw["n"] * kw["c"]).sum(1))[:HEAVY_PAIRS]] += B / HEAVY_PAIRS
        kw["pair_w"] = w
    return kw


def _ref_kw(kw):
    return {k: v for k, v in kw.items() if k not in ("n", "c")}


def loss_bound(mode, ref_loss):
    """the loss bound test_accepted_combination_vs_f64 applies to the mode"""
    return FP8_BOUNDS[0] * abs(ref_loss) if mode == "fp8" else BOUNDS[mode][0] * abs(ref_loss) + LOSS_ATOL


# what leaves the call with each term or rider (each side's ids count on their own; the extras' ids need the companies')
DROPS = {"lq": ("lq_n", "lq_c", "lq_x"), "lq_x": ("lq_x",), "ent_n": ("ent_n",), "ent_c": ("ent_c", "ent_x"), "ent_x": ("ent_x",),
         "cells": ("cells",), "pw": ("pair_w",), "extras": ("x", "lq_x", "ent_x")}


def teeth(mode, terms, B, M, D, T, device=None):
    """{term: |reference loss with it - reference loss of the same inputs without it| / the mode's loss bound} over every term and
    rider present"""
    kw = _inputs(terms, B, M, D, device)
    full = NR.reference(kw["n"], kw["c"], 1.0 / T, mode, **_ref_kw(kw))[0]
    out = {}
    for term in sorted((set(terms) - {"ent"}) | ({"ent_n", "ent_c"} if "ent" in terms else set())):
        less = dict(kw, **dict.fromkeys(DROPS[term]))
        out[term] = abs(full - NR.reference(kw["n"], kw["c"], 1.0 / T, mode, **_ref_kw(less))[0]) / loss_bound(mode, full)
    return out
