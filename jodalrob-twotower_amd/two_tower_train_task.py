"""TwoTowerTrainTask -- drop-in for src/towers/two_tower_train_task.py:9-293 on the HIP path.

forward(batch, return_metrics) -> loss, or a dict with loss / accuracy / positive_similarity_mean /
negative_similarity_mean / similarity_gap / similarity_matrix (same keys as :89-95).

The B x B score matrix is never materialised on the training path: tt_score_dir_fwd sweeps it tile
by tile on MFMA for both softmax directions, tt_score_loss_finish forms loss and metrics, and
tt_score_dir_bwd recomputes the tiles for the gradients.  `similarity_matrix` is produced on demand
(eagerly for small batches, lazily above LAZY_SIM_BATCH) by tt_score_matrix.
"""
from __future__ import annotations

from typing import Dict, NamedTuple, Optional, Union

import torch
from ._lib import no_dynamo as _no_dynamo
import torch.nn as nn

from . import batch_terms as T
from . import ops
from .batch_terms import _CLASH_WHY, _TERM_CLASHES, _TERM_FORMS, _terms_clash       # (what combines: the node decides with it; also imported from here)
from .config import settings
from .cat_embed import kjt_weights, refuse_weights
from .kjt import KeyedJaggedTensor, concat_kjt
from .towers import run_towers
from .two_tower_model import TwoTowerModel, create_two_tower_model

LAZY_SIM_BATCH = 2048


class _DenseLossFn(torch.autograd.Function):
    """The loss variants the fused kernels do not cover, on the materialised score matrix (tt_score_dense_fwd / _bwd):
    loss_type 0 = cross-entropy with label smoothing (:114-133), 1 = cosine-embedding loss (:135-158).  O(B^2) memory."""

    @staticmethod
    def forward(ctx, n, c, inv_t, loss_type, label_smoothing):
        n, c = n.contiguous().float(), c.contiguous().float()
        S, stats, out8, loss = ops.score_dense_fwd(n, c, inv_t, loss_type, label_smoothing)
        ctx.save_for_backward(n, c, S, stats)
        ctx.cfg = (inv_t, loss_type, label_smoothing)
        ctx.mark_non_differentiable(out8)
        return loss.reshape(()), out8

    @staticmethod
    def backward(ctx, d_loss, _d_out8):
        n, c, S, stats = ctx.saved_tensors
        inv_t, loss_type, label_smoothing = ctx.cfg
        # tt_score_dense_bwd overwrites its S argument with dS through a raw pointer (no version counter sees it): work on a copy,
        # so a second backward over the same graph (retain_graph=True) starts from the scores again
        dN, dC = ops.score_dense_bwd(n, c, inv_t, loss_type, label_smoothing, S.clone(), stats, d_loss.reshape(1).contiguous().float())
        return dN, dC, None, None, None


class _ScoreCEFn(torch.autograd.Function):
    """loss = 0.5 * [CE(S, diag) + CE(S^T, diag)],  S = N C^T / T   (:99-134); out8 carries the metrics.
    score_dtype 'fp32': exact-f32 MFMA path (parity); 'bf16': bf16-operand MFMA fast path; 'bf16x3': split-bf16 operands
    (hi + lo, three bf16 MFMAs per product: near-f32 products on the bf16 pipe).
    lq_n / lq_c (f32 [B], both or neither): logQ sampling-bias correction (include/twotower.h *_lq entries) -- the loss and the
    gradients of the corrected softmax, metrics on the raw scores.
    ent_n / ent_c (int32 [B], either or both; a missing side counts as all-distinct): the repeated-entity mask (include/twotower.h
    *_mask entries) -- pairs a != b whose rows share a notice or a company leave both softmax sums; score_dtype 'bf16' and 'fp32'
    only; combines with lq_n / lq_c; metrics on the raw scores.
    pair_w (f32 [B] raw per-pair sample weights): the weighted mean of the pairs' terms (include/twotower.h *_pw entries) -- entries
    that are not positive finite numbers count as 0; score_dtype 'bf16' and 'fp32' only; combines with lq_* and ent_*; the sums and
    the metrics are the unweighted ones.
    x (f32 [M, D] unit rows, with optional lq_x f32 [M] / ent_x int32 [M]): shared extra negatives (include/twotower.h *_xneg
    entries) -- M more columns of every notice's row-direction softmax, no positive, no column sum; an extra is masked for row a iff
    ent_x[m] == ent_c[a]; score_dtype 'bf16' and 'fp32' only; combines with lq_* and ent_*, not with pair_w.  The node packs N, C and
    X itself.  accuracy / row_rank are over the B + M scores, the other metrics the in-batch ones.
    cells (int32 [L, 2] rows (a, j), a < B, j < B + M; with optional cell_count int32 [1] on the device: only the first cell_count rows
    count): masked cells (include/twotower.h *_cells entries) -- the listed pairs leave the row softmax (in-batch columns and extras)
    and, for j < B, the column softmax; the diagonal and cells out of range are ignored; score_dtype 'bf16' only; combines with lq_*
    and x (with lq_x), not with ent_* or pair_w; metrics on the raw scores."""

    @staticmethod
    def forward(ctx, n, c, inv_t, score_dtype, want_col_rank=True, full_rank=True, packed_n=None, packed_c=None, scale_n=None,
                lq_n=None, lq_c=None, ent_n=None, ent_c=None, pair_w=None, x=None, lq_x=None, ent_x=None, cells=None, cell_count=None):
        if n.shape[0] != c.shape[0]:                         # every path below sweeps a square problem of n's row count
            raise ValueError(f"the score node needs as many notice rows as company rows, got {n.shape[0]} and {c.shape[0]}")
        n, c = n.contiguous().float(), c.contiguous().float()
        B, D = n.shape
        dev, shift = n.device, abs(inv_t)                    # unit rows: |s| <= 1/T
        lq = lq_n is not None
        fp8, x3 = score_dtype == "fp8", score_dtype == "bf16x3"
        present = frozenset(k for k, v in (("lq", lq_n), ("ent", ent_n), ("ent", ent_c), ("ent_c", ent_c), ("pw", pair_w), ("extras", x),
                                           ("cells", cells), ("ent_x", ent_x), ("lq_x", lq_x)) if v is not None)
        _score_terms_check(score_dtype, c.shape == n.shape, present)
        if lq:
            ops._lq_check_t(inv_t)
        # the terms' arrays as the entries read them
        M = 0
        if x is not None:
            if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.shape[1] != D or x.shape[0] < 1 or x.device != dev:
                raise ValueError(f"the extra negatives must be a [M >= 1, {D}] tensor on {dev}")
            x = x.contiguous().float()
            M = x.shape[0]
            if lq and lq_x is None:                          # a missing log_q on the extras counts as zeros
                lq_x = torch.zeros(M, dtype=torch.float32, device=dev)
            packed_n = packed_c = scale_n = None             # with extras the node packs N, C and X itself
        if cells is not None:
            cells = ops.score_cells_check(cells, dev)
        ent = ops.score_mask_ids(ent_n, ent_c, B, dev) if "ent" in present else None
        exs = ops.score_xneg_ids(ent_x, M, dev) if x is not None and ent_x is not None else None
        pw = ops.score_pair_weights(pair_w, B, dev) if pair_w is not None else None
        # the operands, once per mode
        Np = Cp = Xp = None
        if fp8:
            # e4m3 operands for the S products (v_mfma_scale_f32_32x32x64_f8f6f4: twice the bf16 MFMA rate), everything else as
            # the bf16 path; always the single-pass forward and the workgroup-staged backward (BASELINE configs[4])
            scale_n = ops.score_unit_scale(inv_t)
            Np, Cp = ops.score_pack2_fp8(n, c, scale_n, 1.0)
        elif x3:
            # as bf16 on [hi | lo] images (tt_score_pack2_bf16x3); the towers' fused tail emits bf16 images only, so the pack is
            # always its own launch.  Both images unscaled: the split of inv_t * log2(e) * n (the "unit" form) would carry the
            # scale's rounding into every operand -- one multiply-add more per score keeps operands that are exact in bf16 exact
            # here (D = 1: every product exact, as in fp32).
            scale_n = 1.0
            Np, Cp = ops.score_pack2_bf16x3(n, c, scale_n, 1.0)
        elif score_dtype == "bf16":
            # scale_n: the notice image holds bf16(scale_n * n) -- with scale_n = inv_t * log2(e) the exponent scale of the
            # softmax rides in the MFMA and the kernels skip a multiply-add per score (results are scale-free).
            # The towers' fused tail can emit the packed operand images itself (tt_tower_acts.emb_packed): one launch fewer.
            if packed_n is not None and packed_c is not None:
                Np, Cp = packed_n, packed_c
                scale_n = 1.0 if scale_n is None else scale_n
            else:
                scale_n = ops.score_unit_scale(inv_t) if scale_n is None else scale_n
                Np, Cp = ops.score_pack2_bf16(n, c, scale_n, 1.0)
            if x is not None:
                Xp = ops.score_pack_bf16(x, 1.0)
        # the kernel form, once.  Symmetric: ONE sweep of the B x B tiles serves both softmax directions -- the steady state of
        # training, and always for fp8 and for every optional term (their row ranks and metrics are the raw scores').  Otherwise the
        # first call's diagnostics (column / full ranks) on the two-direction kernel, or the f32 path's two directional sweeps (plus
        # the extras' rectangular one).
        any_term = bool(present & _TERM_FORMS.keys())
        terms = ops.ScoreTerms(ent=ent, pw=pw)
        inv = w = w_x = None
        if Np is not None and (fp8 or any_term or not (want_col_rank or full_rank)):
            plan = ops.score_cells_plan(cells, B, M, count=cell_count) if cells is not None else None
            terms = ops.ScoreTerms((lq_n, lq_c) if lq else None, ent, pw, (Xp, M, lq_x, exs) if x is not None else None, plan)
            rowsum, colsum, diag, row_rank, inv, w, w_x, out8, loss = ops._sym_fwd(Np, Cp, B, D, inv_t, shift, scale_n, True, score_dtype, terms)
            if any_term and want_col_rank:
                # the first call's column top-1 rate (a diagnostic only) from the uncorrected two-direction kernel
                col_rank = ops.score_fwd_bf16(Np, Cp, B, D, inv_t, shift, True, False, scale_n, x3=x3)[4]
                out8 = out8.clone()
                out8[5] = (col_rank == 0).float().mean()
        else:
            if Np is not None:
                rowsum, colsum, diag, row_rank, col_rank, sumscore, inv = ops.score_fwd_bf16(Np, Cp, B, D, inv_t, shift, want_col_rank,
                                                                                             full_rank, scale_n, with_inv=True, x3=x3)
                if not want_col_rank:
                    col_rank = row_rank                  # placeholder: column top-1 rate is only a first-call diagnostic
            else:
                rowsum, diag, row_rank, sumscore = ops.score_dir_fwd(n, c, inv_t, shift, 0, True, lq_b=lq_c, ent=ent)
                colsum, _, col_rank, _ = ops.score_dir_fwd(c, n, inv_t, shift, 0, False, lq_b=lq_n, ent=ent)
                if x is not None:
                    terms = terms._replace(extras=(None, M, lq_x, exs))
                    ops.score_dir_fwd_xneg(n, x, inv_t, shift, diag, rowsum, row_rank, lq_x=lq_x, ent_c=ent[1] if exs is not None else None,
                                           ent_x=exs)
                if lq:
                    w = (lq_n.contiguous(), lq_c.contiguous())
            out8, loss = ops.score_loss_finish(B, shift, rowsum, colsum, diag, row_rank, col_rank, sumscore, lq_n=lq_n, lq_c=lq_c, pw=pw)
        ctx.rec = _Saved(inv_t, shift, score_dtype, None if Np is None else (Np, Cp, scale_n, inv), w, w_x, terms)
        ctx.save_for_backward(n, c, rowsum, colsum, *(() if x is None else (x,)))
        ctx.mark_non_differentiable(out8, row_rank)
        ctx.set_materialize_grads(False)                     # else autograd zero-fills grads for out8 / row_rank every step
        return loss, out8, row_rank

    @staticmethod
    def backward(ctx, d_loss, _d_out8, _d_rank):
        """the square backward on the forward's sums (which include the extras), then the extras' two rectangular directions: dN +=
        and dX, in this order (one launch with masked cells)"""
        if d_loss is None:
            return _node_grads()
        n, c, rowsum, colsum = ctx.saved_tensors[:4]
        B, D = n.shape
        if d_loss.dtype != torch.float32 or not d_loss.is_contiguous():
            d_loss = d_loss.contiguous().float()
        r = ctx.rec
        scale = r.inv_t / (2.0 * B)
        if r.packed is not None:
            Np, Cp, scale_n, inv = r.packed
            dN, dC, dX = ops._bwd_sym(Np, Cp, B, D, r.inv_t, r.shift, rowsum, colsum, d_loss, scale, scale_n, inv, r.operands, r.w, r.terms, r.w_x)
        else:
            ent, pw = r.terms.ent, r.terms.pw
            lqn, lqc = r.w if r.w is not None else (None, None)
            dN = ops.score_dir_bwd(n, c, r.inv_t, r.shift, 0, rowsum, colsum, d_loss, scale, lq_a=lqn, lq_b=lqc, ent=ent, pw=pw)
            dC = ops.score_dir_bwd(c, n, r.inv_t, r.shift, 0, colsum, rowsum, d_loss, scale, lq_a=lqc, lq_b=lqn, ent=ent, pw=pw)
            dX = None
            if r.terms.extras is not None:
                x, (_, _, lq_x, exs) = ctx.saved_tensors[4], r.terms.extras
                ec = ent[1] if exs is not None else None
                ops.score_dir_bwd_xneg(n, x, r.inv_t, r.shift, True, rowsum, d_loss, scale, lq_x=lq_x, ent_a=ec, ent_b=exs, out=dN)
                dX = ops.score_dir_bwd_xneg(x, n, r.inv_t, r.shift, False, rowsum, d_loss, scale, lq_x=lq_x, ent_a=exs, ent_b=ec)
        return _node_grads(n=dN, c=dC, x=dX)


class _Saved(NamedTuple):
    """what _ScoreCEFn.forward leaves for its backward: packed = (Np, Cp, scale_n, inv) or None on the f32 path; w = the forward's
    sampling weights (the f32 path: the log q vectors); terms as the backward entries take them"""
    inv_t: float
    shift: float
    operands: str
    packed: Optional[tuple]
    w: Optional[tuple]
    w_x: Optional[torch.Tensor]
    terms: "ops.ScoreTerms"


class _BatchTerms(NamedTuple):
    """what TwoTowerTrainTask._batch_terms makes of a batch: lq (lq_n, lq_c); ent (ent_n, ent_c), a side may be None; pw; neg the
    "negatives" dict; cells (cells, count or None) -- each None when the batch carries none"""
    lq: Optional[tuple] = None
    ent: Optional[tuple] = None
    pw: Optional[torch.Tensor] = None
    neg: Optional[dict] = None
    cells: Optional[tuple] = None


_NO_TERMS = _BatchTerms()
_NODE_INPUTS = _ScoreCEFn.forward.__code__.co_varnames[1:_ScoreCEFn.forward.__code__.co_argcount]
_NODE_SLOT = {name: i for i, name in enumerate(_NODE_INPUTS)}


def _node_grads(**grads):
    """_ScoreCEFn.backward's return: one slot per forward input, filled by parameter name"""
    out = [None] * len(_NODE_INPUTS)
    for name, g in grads.items():
        out[_NODE_SLOT[name]] = g
    return tuple(out)


def _need_form(term, score_dtype, name, hint=" (score_dtype 'bf16' or 'fp32')"):
    if score_dtype not in _TERM_FORMS[term]:
        raise ValueError(f"{name} no {score_dtype} form{hint}")


def _need_square(square, name):
    if not square:
        raise ValueError(f"{name} as many notice rows as company rows")


def _score_terms_check(score_dtype, square, present):
    """Refuses what the score node does not cover; no device, no tensors.  present: the names of what the call carries, of 'lq', 'ent'
    (either side's ids; 'ent_c' the companies'), 'pw', 'extras' (with 'ent_x' / 'lq_x'), 'cells'.  square: as many notice rows as
    company rows.  The refusals in the order they are decided."""
    if not present:
        return
    has = present.__contains__
    cells, extras = has("cells"), has("extras")
    if cells:
        if (has("ent") or has("ent_x")) and _terms_clash("cells", "ent"):      # (ids on the extras are the mask's too)
            raise ValueError("masked cells do not combine with the repeated-entity mask (cells built from the pair table hold every repeat)")
        _need_form("cells", score_dtype, "masked cells have", " (score_dtype 'bf16')")
        if has("pw") and _terms_clash("cells", "pw"):
            raise ValueError("masked cells do not combine with pair weights")
        _need_square(square, "masked cells need")
    if extras:
        _need_form("extras", score_dtype, "extra negatives have")
        if has("pw") and _terms_clash("extras", "pw"):
            raise ValueError("extra negatives do not combine with pair weights")
        _need_square(square, "extra negatives need")
        if has("ent_x") and not has("ent_c"):
            raise ValueError("the extras' entity ids are compared with the batch's company ids: ent_c is missing")
    if (cells or extras) and has("lq_x"):
        if not has("lq"):
            raise ValueError("the extras carry log_q but the batch is not corrected")
        if not extras:
            raise ValueError("masked cells: lq_x needs lq_n / lq_c and the extras")
    if has("ent"):
        _need_form("ent", score_dtype, "the repeated-entity mask has")
        _need_square(square, "the repeated-entity mask needs")
    if has("pw"):
        _need_form("pw", score_dtype, "pair weights have")
        _need_square(square, "pair weights need")
    if has("lq"):
        _need_form("lq", score_dtype, "the logQ correction has", "")


class _Result(dict):
    """Result dict whose 'similarity_matrix' entry is computed on first access (large batches)."""

    def __init__(self, *a, sim_thunk=None, out8=None, **k):
        super().__init__(*a, **k)
        self._sim_thunk = sim_thunk
        self.out8 = out8          # the finish kernel's 8 floats (loss, accuracy, pos, neg, gap, ...): the entries above are views of it

    def _materialise(self):
        if self._sim_thunk is not None and not dict.__contains__(self, "similarity_matrix"):
            dict.__setitem__(self, "similarity_matrix", self._sim_thunk())
            self._sim_thunk = None

    def __missing__(self, key):
        if key == "similarity_matrix" and self._sim_thunk is not None:
            self._materialise()
            return dict.__getitem__(self, key)
        raise KeyError(key)

    def __contains__(self, key):
        return dict.__contains__(self, key) or (key == "similarity_matrix" and self._sim_thunk is not None)

    def get(self, key, default=None):
        if key == "similarity_matrix":
            self._materialise()
        return dict.get(self, key, default)

    def keys(self):
        self._materialise()
        return dict.keys(self)

    def items(self):
        self._materialise()
        return dict.items(self)

    def values(self):
        self._materialise()
        return dict.values(self)


class TwoTowerTrainTask(nn.Module):
    def __init__(self, two_tower_model: TwoTowerModel, temperature: float = 1.0, loss_type: str = "cross_entropy",
                 label_smoothing: float = 0.0, score_dtype: str = None):
        super().__init__()
        self.score_dtype = score_dtype or settings.score_dtype
        if self.score_dtype not in ("fp32", "bf16", "bf16x3", "fp8"):
            raise ValueError(f"score_dtype must be 'fp32', 'bf16', 'bf16x3' or 'fp8', got {self.score_dtype!r}")
        if self.score_dtype == "bf16" and settings.tower_pack:       # (settings.tower_pack = False: separate pack launch; tests)
            for tw in (two_tower_model.notice_tower, two_tower_model.company_tower):
                tw.pack_for_score = True
            # the notice image carries the softmax's exponent scale (see _ScoreCEFn)
            two_tower_model.notice_tower.pack_scale = ops.score_unit_scale(1.0 / float(temperature))
        self.two_tower_model = two_tower_model
        self.temperature = temperature
        self.loss_type = loss_type
        self.label_smoothing = label_smoothing
        if loss_type not in ["cross_entropy", "cosine_embedding"]:
            raise ValueError(f"Unsupported loss_type: {loss_type}")                         # :37-38
        if not 0.0 <= float(label_smoothing) <= 1.0:
            raise ValueError(f"label_smoothing must be in [0, 1], got {label_smoothing}")
        # cosine-embedding loss (:135-158) and label smoothing (never set by the reference's factory or driver) run on the
        # dense path: the score matrix is materialised (O(B^2) memory), f32 throughout -- see _DenseLossFn
        self._dense_loss = loss_type != "cross_entropy" or float(label_smoothing) != 0.0

    # ---- forward: :40-97 ----------------------------------------------------------------------------
    @_no_dynamo
    def forward(self, batch, return_metrics: bool = False):
        notice_input, company_input = batch["notice"], batch["company"]
        nb, cb = notice_input["dense"].size(0), company_input["dense"].size(0)
        if nb != cb:                                                                         # :64-67
            raise ValueError(f"Notice와 Company 배치 크기가 다릅니다: {nb} vs {cb}")
        t = self._batch_terms(batch, nb)
        if t.neg is not None:
            notice_embeddings, company_embeddings, loss, out8 = self._forward_negatives(notice_input, company_input, t.neg, nb, t.lq, t.ent, t.cells)
        else:
            notice_embeddings, company_embeddings = self.two_tower_model(notice_input, company_input)
            loss, out8, _ = self._score_ce(notice_embeddings, company_embeddings, 1.0 / float(self.temperature),
                                           not hasattr(self, "_pair_check_done"), log_q=t.lq, entity=t.ent, pair_weight=t.pw, cells=t.cells)
        if not hasattr(self, "_pair_check_done"):                                            # :82-84
            self._verify_positive_pair_alignment(out8)
            self._pair_check_done = True
        if not return_metrics:
            return loss
        n_det, c_det, inv_t = notice_embeddings.detach(), company_embeddings.detach(), 1.0 / float(self.temperature)
        res = _Result({"loss": loss, "accuracy": out8[1], "positive_similarity_mean": out8[2],
                       "negative_similarity_mean": out8[3], "similarity_gap": out8[4]},
                      sim_thunk=lambda: ops.score_matrix(n_det, c_det, inv_t), out8=out8)
        if nb <= LAZY_SIM_BATCH:
            res._materialise()
        return res

    def forward_with_ranks(self, batch):
        """(result dict as forward(batch, return_metrics=True), 0-based rank of each positive in its row) from ONE pass
        through the towers -- what the evaluator needs per batch (src/evaluation/evaluator.py:123-155 calls the model once
        and ranks its similarity matrix).  Ranks come from the exact-f32 score sweep, as diagonal_ranks()."""
        for row in T.TABLE:
            if row.eval_why is not None and batch.get(row.key) is not None:
                raise ValueError(f"forward_with_ranks does not take a batch with '{row.key}' ({row.eval_why})")
        with torch.no_grad():
            n, c = self.two_tower_model(batch["notice"], batch["company"])
            if n.size(0) != c.size(0):
                raise ValueError(f"Notice와 Company 배치 크기가 다릅니다: {n.size(0)} vs {c.size(0)}")
            inv_t = 1.0 / float(self.temperature)
            loss, out8, _ = self._score_ce(n, c, inv_t, False)
            _, _, rank, _ = ops.score_dir_fwd(n.contiguous(), c.contiguous(), inv_t, abs(inv_t), 0, False)
            n_det, c_det = n.detach(), c.detach()
            res = _Result({"loss": loss, "accuracy": out8[1], "positive_similarity_mean": out8[2],
                           "negative_similarity_mean": out8[3], "similarity_gap": out8[4]},
                          sim_thunk=lambda: ops.score_matrix(n_det, c_det, inv_t))
            return res, rank

    _refused = frozenset()         # the batch entries (keys of batch_terms.TABLE) this task does not take; the sharded task has some

    def _batch_terms(self, batch, B):
        """The batch's optional entries, validated, as the score node takes them (_BatchTerms).  One walk of batch_terms.TABLE; per
        entry, in this order: may this task take it, what it does not combine with, the dense loss, the score_dtype's form, its
        arrays.  Refuses what the loss does not cover -- never ignores an entry."""
        have = T.present(batch)
        if not have:
            return _NO_TERMS
        dev, out = batch["notice"]["dense"].device, {}
        for row in T.TABLE:
            if row.key not in have:
                continue
            if row.key in self._refused:
                raise NotImplementedError(f"{row.phrase} {row.verb} not supported by {type(self).__name__}")
            for other in T.TABLE:                              # (what it clashes with has been decided: it stands above in the table)
                if other.term in out and _terms_clash(row.term, other.term):
                    raise ValueError(f"{row.phrase} do not combine with '{other.key}'" + _CLASH_WHY.get(frozenset({row.term, other.term}), ""))
            if self._dense_loss:
                raise ValueError(f"{row.phrase} {row.verb} not supported by the dense loss path "
                                 "(label_smoothing != 0 or loss_type='cosine_embedding')")
            if self.score_dtype not in _TERM_FORMS[row.term]:
                raise ValueError(f"{row.phrase} {row.verb} not supported for score_dtype={self.score_dtype!r}")
            if row.where == "nested":
                out[row.term] = self._check_negatives(batch, out.get("lq"), out.get("ent"))
                continue
            v = [t if t is None else T.check(t, name, row.dtype, row.dims(B), dev, "the batch")
                 for name, t in zip(row.names("the batch"), row.of(batch) if row.where == "side" else (batch[row.key],))]
            if row.missing == "zeros":                         # (a missing side's ids stay None: all-distinct to the node)
                v = [row.fill(B, dev) if t is None else t.contiguous() for t in v]
            out[row.term] = tuple(v) if row.where == "side" else v[0]
        if "cells" in out:             # the optional device count of the rows in use (static buffers)
            n = batch.get("masked_cells_count")
            if n is not None and not (isinstance(n, torch.Tensor) and n.dtype == torch.int32 and n.numel() == 1 and n.device == dev):
                raise ValueError(f"batch['masked_cells_count'] must be an int32 tensor of one element on {dev}")
            out["cells"] = (out["cells"], n)
        return _BatchTerms(out.get("lq"), out.get("ent"), out.get("pw"), out.get("extras"), out.get("cells"))

    def _forward_negatives(self, notice_input, company_input, neg, B, lq, ent, cells=None):
        """(notice embeddings, company embeddings, loss, out8) of a batch with shared extra negatives: the M rows ride behind the batch's
        companies through ONE company-tower pass (in train mode its BatchNorm batch statistics run over the B + M rows), the output is
        split into C and X, and the score node takes X as M more columns of every notice's row-direction softmax"""
        if self.two_tower_model.company_tower.categorical_embedder.bag_mode:      # ragged bags: the lengths ride along
            kjt = concat_kjt(company_input["kjt"], neg["kjt"])
        else:
            for k in (company_input["kjt"], neg["kjt"]):
                refuse_weights(kjt_weights(k), "the company tower")
            kjt = KeyedJaggedTensor(company_input["kjt"].keys(), torch.cat([company_input["kjt"].values(), neg["kjt"].values()], 0))
        both = {"dense": torch.cat([company_input["dense"], neg["dense"]], 0), "kjt": kjt}
        n_emb, cx = run_towers([self.two_tower_model.notice_tower, self.two_tower_model.company_tower], [notice_input, both])
        c_emb, x_emb = cx[:B], cx[B:]
        lqs, ents = lq if lq is not None else (None, None), ent if ent is not None else (None, None)
        loss, out8, _ = _ScoreCEFn.apply(n_emb, c_emb, 1.0 / float(self.temperature), self.score_dtype, not hasattr(self, "_pair_check_done"),
                                         False, None, None, None, lqs[0], lqs[1], ents[0], ents[1], None, x_emb, neg.get("log_q"),
                                         neg.get("entity"), *(cells if cells is not None else (None, None)))
        return n_emb, c_emb, loss, out8

    def _check_negatives(self, batch, lq, ent):
        """batch["negatives"]'s structure -- {"dense" [M, Dc], "kjt"} with optional "log_q" f32 [M] and "entity" int32 [M], M >= 1 company
        rows every notice of the batch is contrasted with besides the in-batch ones; lq / ent: the batch's own, validated"""
        neg, company_input = batch["negatives"], batch["company"]
        ref = company_input["dense"]
        d = neg.get("dense") if isinstance(neg, dict) else None
        if not isinstance(d, torch.Tensor) or d.dim() != 2 or d.shape[1] != ref.shape[1] or d.dtype != ref.dtype or "kjt" not in neg:
            raise ValueError(f"batch['negatives'] must be a company-side input {{'dense' [M, {ref.shape[1]}] {ref.dtype}, 'kjt'}}")
        M = d.shape[0]
        if M < 1:
            raise ValueError("batch['negatives'] must hold at least one row (M >= 1)")
        if d.device != ref.device:
            raise ValueError(f"batch['negatives']['dense'] is on {d.device}, the batch on {ref.device}")
        K = len(company_input["kjt"].keys())
        v = neg["kjt"].values()
        # (a bag-mode company tower reads M * K bag lengths; the number of ids is then free)
        n_slots = neg["kjt"].lengths().numel() if self.two_tower_model.company_tower.categorical_embedder.bag_mode else v.numel()
        if list(neg["kjt"].keys()) != list(company_input["kjt"].keys()) or n_slots != M * K or v.device != ref.device:
            raise ValueError(f"batch['negatives']['kjt'] must carry the company side's {K} keys for {M} rows on {ref.device}")
        for name, given in (("log_q", lq is not None), ("entity", ent is not None and ent[1] is not None)):
            if neg.get(name) is None:
                continue
            T.check(neg[name], f"batch['negatives']['{name}']", T.ROWS[name].dtype, (M,), ref.device, "the batch", a="a")
            if not given:
                raise ValueError(f"batch['negatives']['{name}'] needs batch['company']['{name}']: the extras' {name} has nothing to be "
                                 "compared with")
        return neg

    def _score_ce(self, n, c, inv_t, first_call, log_q=None, entity=None, pair_weight=None, cells=None):
        """(loss, out8, row_rank) of the symmetric in-batch-negative softmax-CE (:99-134); the sharded task overrides it.
        log_q: (lq_n, lq_c) -- the logQ-corrected loss (_ScoreCEFn).  entity: (ent_n, ent_c) -- the repeated-entity mask.
        pair_weight: f32 [B] -- per-pair sample weights; combines with both.  cells: (cells, count) -- masked cells."""
        for given, term, what, s in ((pair_weight, "pw", "pair weights", ""), (entity, "ent", "the repeated-entity mask", "s"),
                                     (log_q, "lq", "the logQ correction", "s")):
            if given is None:
                continue
            if self._dense_loss or self.score_dtype not in _TERM_FORMS[term]:
                raise ValueError(f"{what} cover{s} the fused cross-entropy with score_dtype {' / '.join(_TERM_FORMS[term])} only")
            if n.shape != c.shape:
                raise ValueError(f"{what} need{s} as many notice rows as company rows")
        if self._dense_loss:
            if n.shape != c.shape:
                raise ValueError("the dense loss path needs as many notice rows as company rows")
            loss, out8 = _DenseLossFn.apply(n, c, inv_t, 0 if self.loss_type == "cross_entropy" else 1, float(self.label_smoothing))
            return loss, out8, None
        lqs, ents, kp = log_q or (None, None), entity or (None, None), cells or (None, None)
        pn, pc = getattr(n, "_tt_packed", None), getattr(c, "_tt_packed", None)     # (buffer, scale) emitted by the towers
        if self.score_dtype != "bf16" or n.shape != c.shape or pn is None or pc is None or pc[1] != 1.0:
            pn, pc = (None, None), (None, None)
        return _ScoreCEFn.apply(n, c, inv_t, self.score_dtype, first_call, False, pn[0], pc[0], pn[1], lqs[0], lqs[1], ents[0], ents[1],
                                pair_weight, None, None, None, kp[0], kp[1])

    def _compute_similarity_matrix(self, notice_embeddings, company_embeddings):                # :99-112
        return self.two_tower_model.compute_similarity(notice_embeddings, company_embeddings, self.temperature)

    def _verify_positive_pair_alignment(self, out8: torch.Tensor):                               # :253-290
        row_hit, col_hit = float(out8[1]), float(out8[5])
        print("🔍 [Positive Pair Alignment Check]")
        print(f"   📊 Notice→Company Top-1 정확도: {row_hit:.3f}")
        print(f"   📊 Company→Notice Top-1 정확도: {col_hit:.3f}")
        print(f"   🎯 대각선이 row-max인 비율: {row_hit:.3f}")
        if row_hit < 0.05 and col_hit < 0.05:
            print("   🚨 CRITICAL: Positive pair 정합성 실패!")
            print("   → DataLoader에서 notice/company 순서가 어긋남")
            print("   → 동일한 샘플러/인덱스로 페어를 구성하세요")
        elif row_hit < 0.3 or col_hit < 0.3:
            print("   ⚠️  WARNING: Positive pair 정합성 부족")
            print("   → 배치 내 positive 비율 확인 필요")
        else:
            print("   ✅ Positive pair 정합성 양호")
        print()

    # ---- predict_batch: :181-207 ----------------------------------------------------------------------
    @_no_dynamo
    def predict_batch(self, batch, top_k: int = 10) -> Dict[str, torch.Tensor]:
        self.eval()
        with torch.no_grad():
            n, c = self.two_tower_model(batch["notice"], batch["company"])
            sim = ops.score_matrix(n.contiguous(), c.contiguous(), 1.0 / float(self.temperature))
            vals, idx = ops.topk_rows(sim, top_k)
            return {"top_similarities": vals, "top_indices": idx, "all_similarities": sim}

    @_no_dynamo
    def predict_catalog(self, notice_batch, index, top_k: int = 10, exclude=None, allow=None,
                        require=None) -> Dict[str, torch.Tensor]:
        """Top-k companies of the whole catalogue `index` (a retrieval.CatalogIndex) for every notice of `notice_batch` (the
        notice side's {"dense", "kjt"}, or a full batch with a "notice" entry): {"top_similarities" f32 [B, top_k],
        "top_indices" int64 [B, top_k]} -- index rows, value descending, ties to the lower index; 1 <= top_k <= min(512, catalogue
        size) (retrieval.MAX_K).  The notice tower runs in
        eval mode; the task's train()/eval() state is restored afterwards.  (predict_batch ranks within one batch.)
        exclude=(offsets, rows): per-notice exclusion lists (CatalogIndex.search), e.g. companies that already bid on it
        (retrieval.exclusions_from_pairs).  allow / require: per-notice attribute masks for an index built with tags=
        (CatalogIndex.search): only eligible companies are returned."""
        from .retrieval import CatalogIndex
        if not isinstance(index, CatalogIndex):
            raise TypeError("index must be a CatalogIndex")
        index._check_k(top_k)
        if index.dim != self.two_tower_model.final_embedding_dim:
            raise ValueError(f"catalogue dimension {index.dim} != the towers' {self.two_tower_model.final_embedding_dim}")
        notice = notice_batch["notice"] if "notice" in notice_batch else notice_batch
        if allow is not None or require is not None:                  # refused here, before the tower runs
            n = allow if allow is not None else require
            index._check_filter(allow, require, int(n.shape[0]) if torch.is_tensor(n) and n.dim() >= 1 else -1)
        modes = [(m, m.training) for m in self.modules()]
        self.eval()
        try:
            with torch.no_grad():
                q = self.two_tower_model.get_notice_embeddings(notice)
                vals, idx = index.search(q, top_k, exclude=exclude, allow=allow, require=require)
        finally:
            for m, was in modes:
                m.training = was
        return {"top_similarities": vals, "top_indices": idx}

    def diagonal_ranks(self, batch):
        """0-based rank of each positive in its row (count of strictly larger scores, ties before the
        diagonal counted) -- the quantity Recall@K / MRR need, without the B x B matrix."""
        with torch.no_grad():
            n, c = self.two_tower_model(batch["notice"], batch["company"])
            inv_t = 1.0 / float(self.temperature)
            _, _, rank, _ = ops.score_dir_fwd(n.contiguous(), c.contiguous(), inv_t, abs(inv_t), 0, False)
            return rank


def create_two_tower_train_task(notice_categorical_keys, company_categorical_keys, metadata_path: str = "meta/metadata.csv",
                                categorical_embedding_dim: int = 64, notice_dense_input_dim: int = 256,
                                company_dense_input_dim: int = 128, tower_hidden_dims=None, final_embedding_dim: int = 128,
                                dropout_rate: float = 0.2, temperature: float = 1.0, loss_type: str = "cross_entropy",
                                device="cuda:0", embedding_grad=None, score_dtype=None, mlp_dtype=None,
                                categorical_position_weights=None, categorical_pooling=None) -> TwoTowerTrainTask:
    model = create_two_tower_model(notice_categorical_keys=notice_categorical_keys,
                                   company_categorical_keys=company_categorical_keys, metadata_path=metadata_path,
                                   categorical_embedding_dim=categorical_embedding_dim,
                                   notice_dense_input_dim=notice_dense_input_dim,
                                   company_dense_input_dim=company_dense_input_dim, tower_hidden_dims=tower_hidden_dims,
                                   final_embedding_dim=final_embedding_dim, dropout_rate=dropout_rate, device=device,
                                   embedding_grad=embedding_grad, mlp_dtype=mlp_dtype,
                                   categorical_position_weights=categorical_position_weights, categorical_pooling=categorical_pooling)
    return TwoTowerTrainTask(two_tower_model=model, temperature=temperature, loss_type=loss_type, score_dtype=score_dtype)
