"""The f64 reference of the whole score node (tests/_score_node_reference.py) on the CPU, and the inputs tests/test_gpu_score_node_matrix.py
feeds the node.  No device, no library.

1. Anchoring: at every combination one of the term references covers (tests/_mask_reference.py, _pair_weight_reference.py,
   _xneg_reference.py, _known_mask_reference.py), the unified reference equals that reference's reference(...) -- loss and every gradient
   to 1e-12 relative, modes "fp32" and "bf16", B = 70, M = 33, D = 32.
2. Closed form == f64 autograd (mode "fp32") to 1e-10 over every combination the table accepts for fp32 and bf16, and the one-sided ids.
3. The inputs have teeth: for every accepted combination at both of the GPU file's shapes, every term and rider present moves the
   reference loss by at least 100 times the loss bound the GPU file applies to the mode.

The inputs are tests/_score_node_inputs.py's -- the term files' generators, the ones the GPU file feeds the node -- drawn on the CPU
(device="cpu"; what that means for the unit rows is said there).
"""
import pytest
import torch

import _known_mask_reference as KR
import _mask_reference as MR
import _pair_weight_reference as PW
import _score_node_reference as NR
import _xneg_reference as XR
import _score_node_inputs as GM

B0, M0, D0, INV_T0 = 70, 33, 32, 2.0
TERM_SETS = sorted({t for d, t in GM.ACCEPTED if d in ("fp32", "bf16")}, key=lambda t: (len(t), sorted(t)))      # bf16's 22 hold fp32's 17
ALL_SETS = TERM_SETS + GM.ONE_SIDED


def _close(got, ref, tol):
    if ref is None:
        return got is None
    if not isinstance(ref, torch.Tensor):
        return abs(got - ref) <= tol * abs(ref)
    return float((got - ref).abs().max()) <= tol * float(ref.abs().max())


def _term_references(terms, kw, mode):
    """[(name, (loss, dN, dC[, dX]))] of every term reference that covers the combination"""
    n, c, q = kw["n"], kw["c"], (kw["lq_n"], kw["lq_c"])
    ent = (kw["ent_n"], kw["ent_c"])
    has_ent = ent[0] is not None or ent[1] is not None
    out = []
    if not terms & {"pw", "extras", "cells"}:
        out.append(("mask", MR.reference(n, c, INV_T0, *(ent if has_ent else MR.ids(B0, "distinct")), mode, *q)))
    if "pw" in terms:
        out.append(("pair weights", PW.reference(n, c, INV_T0, kw["pair_w"], mode, *ent, *q)))
    if "extras" in terms and "cells" not in terms:
        out.append(("extras", XR.reference(n, c, kw["x"], INV_T0, mode, *ent, kw["ent_x"], *q, kw["lq_x"])))
    if "cells" in terms:
        out.append(("cells", KR.reference(n, c, kw["x"], kw["cells"], INV_T0, mode, *q, kw["lq_x"])))
    return out


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("terms", ALL_SETS, ids=GM._name)
def test_anchored_to_the_term_references(terms, mode):
    kw = GM._inputs(terms, B0, M0, D0, "cpu")
    got = NR.reference(kw["n"], kw["c"], INV_T0, mode, **GM._ref_kw(kw))
    refs = _term_references(terms, kw, mode)
    assert refs, sorted(terms)
    for name, ref in refs:
        ref = tuple(ref) + (None,) * (4 - len(ref))          # (the references without extras return no dX)
        for k, what in enumerate(("loss", "dN", "dC", "dX")):
            assert _close(got[k], ref[k], 1e-12), (name, what)


def test_every_term_reference_anchors_something():
    seen = set()
    for terms in ALL_SETS:
        seen |= {name for name, _ in _term_references(terms, GM._inputs(terms, B0, M0, D0, "cpu"), "fp32")}
    assert seen == {"mask", "pair weights", "extras", "cells"}
    # extras and weights together, which no term reference and no kernel covers: the weights ride on the extras' softmax weights too
    kw = GM._inputs(frozenset({"extras", "pw", "lq", "lq_x"}), B0, M0, D0, "cpu")
    for u, v in zip(NR.reference(kw["n"], kw["c"], INV_T0, "fp32", **GM._ref_kw(kw)), NR.autograd_reference(kw["n"], kw["c"], INV_T0, **GM._ref_kw(kw))):
        assert _close(u, v, 1e-10)


@pytest.mark.parametrize("terms", ALL_SETS, ids=GM._name)
def test_closed_form_equals_autograd(terms):
    kw = GM._inputs(terms, B0, M0, D0, "cpu")
    got = NR.reference(kw["n"], kw["c"], INV_T0, "fp32", **GM._ref_kw(kw))
    ref = NR.autograd_reference(kw["n"], kw["c"], INV_T0, **GM._ref_kw(kw))
    for k, what in enumerate(("loss", "dN", "dC", "dX", "rowsum", "colsum")):
        assert _close(got[k], ref[k], 1e-10), what
    assert (got[3] is None) == ("extras" not in terms)


@pytest.mark.parametrize("shape", GM.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_the_inputs_have_teeth(shape):
    """every term and rider of every accepted combination (each side's ids on their own) moves the reference loss by 100 loss bounds of
    the mode at least: a term that the node dropped, or read from another term's slot, cannot pass the GPU file's loss check"""
    cases = [(d, t) for d, t in GM.ACCEPTED if t] + [(d, t) for d in ("fp32", "bf16") for t in GM.ONE_SIDED]
    worst = {}
    for dtype, terms in cases:
        figs = GM.teeth(dtype, terms, *shape, device="cpu")
        assert set(figs) >= (set(terms) - {"ent"}), (dtype, sorted(terms), figs)
        for term, ratio in figs.items():
            worst[term] = min(worst.get(term, ratio), ratio)
            assert ratio >= 100.0, (dtype, sorted(terms), term, ratio)
    print(shape, {k: round(v) for k, v in worst.items()})
    assert set(worst) == {"lq", "lq_x", "ent_n", "ent_c", "ent_x", "cells", "pw", "extras"}
