"""BaseTower / NoticeTower / CompanyTower on the HIP path.

Drop-in for src/towers/tower/{base_tower,notice_tower,company_tower}.py: same constructor arguments,
same sub-module names and therefore the same state-dict keys and shapes
(`categorical_embedder.embeddings.<key>.weight`, `dense_projection.{weight,bias}`,
`mlp.{4i}.{weight,bias}`, `mlp.{4i+2}.{weight,bias,running_mean,running_var,num_batches_tracked}`,
`mlp.{4n}.{weight,bias}`), same forward contract: {"dense": [B,Din] f32, "kjt": KJT} -> unit rows [B,D].

The torch modules below (nn.Linear / nn.BatchNorm1d / ...) are PARAMETER CONTAINERS only -- they give
the reference's initialisation and key names; their forward is never called.  The arithmetic runs in
libtwotower_hip.so: tt_embed_lookup_fwd writes the embedding rows straight into the MLP input buffer
(no torch.cat), tt_tower_mlp_fwd/_bwd run the MLP, tt_dedup_plan + tt_embed_grad_bwd produce the
table gradients.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence

import torch
from ._lib import no_dynamo as _no_dynamo
import torch.nn as nn

from . import _lib as L
from . import ops
from .config import settings
from .cat_embed import CategoricalEmbedder, EmbeddingStore, kjt_weights, refuse_weights, weights_need_grad


_DEBUG_KEEP = None   # set to a list by debugging tools


def _sync_comm(sides):
    """The communicator for SyncBN if it applies to this pass: every tower asks for it, trains, shares one batch size and
    dropout setting (the C side then checks the shape conditions of the fused tail), else None."""
    if not sides:
        return None
    comms = [getattr(s.tower, "sync_comm", None) for s in sides]
    if any(c is None for c in comms) or not all(s.train for s in sides):
        return None
    if len({s.B for s in sides}) != 1 or len({s.p_drop for s in sides}) != 1:
        raise ValueError("SyncBN needs one batch size and one dropout rate for all towers of a pass")
    return comms[0]


def _al(n: int) -> int:
    return (n + 63) // 64 * 64


def _one_call(sides, key) -> bool:
    """Several towers that share B, depth and key(side) run as one fused call (_run_pass)"""
    return len(sides) > 1 and len({(s.B, s.tower.n_hidden) + key(s) for s in sides}) == 1


def _fwd_key(s):
    """What the towers of one fused forward call must share, besides B and depth"""
    return (s.train, s.p_drop)


def _front_gathers(group, live, store, sm, B) -> bool:
    """The towers' forward gathers the embedding rows of this store's sides inside its one-launch front, from the hand-over
    launch's slot-order rows `sm`: when settings.front_gather is on, the sides are exactly the towers of ONE forward call and
    the library says it will (tt_towers_fwd_gathers -- the shapes are its business).  Fills the gather fields of the sides'
    activation structs; the caller then launches no lookup."""
    sides = [g[0] for g in group]
    if not all(s.tower.front_gather for s in sides) or any(g[2] for g in group) or len(sides) != len(live) or any(a is not b for a, b in zip(sides, live)):
        return False
    if _sync_comm(live) is not None or not (len(live) == 1 or _one_call(live, _fwd_key)):
        return False
    Ks = [len(s.tower.categorical_embedder.keys) for s in sides]
    if sm.dtype != torch.int32 or not sm.is_contiguous() or sm.numel() != B * sum(Ks) or sm.device != store.weight.device or not store.weight.is_contiguous():
        return False
    base = 0
    for s, K in zip(sides, Ks):
        a = s.acts_struct
        a.gather_table, a.gather_rows, a.gather_K, a.gather_E = store.weight.data_ptr(), sm.data_ptr() + 4 * base, K, store.weight.shape[1]
        base += B * K
    if ops.towers_fwd_gathers([s.tower._params() for s in sides], [s.acts_struct for s in sides], B, sides[0].train):
        return True
    for s in sides:
        a = s.acts_struct
        a.gather_table, a.gather_rows, a.gather_K, a.gather_E = None, None, 0, 0
    return False


def _run_pass(items, one, many, key, sync):
    """The dispatch of a tower pass, forward or backward, over items = (side, *that side's arguments of the C call): SyncBN in
    two calls around ONE all-gather (twotower.h: sync_phase); one fused call (horizontal fusion: one launch per layer step covers
    every tower) when the towers share B, depth and key(side); else one call per tower.  one / many: ops.tower_* / ops.towers_*.
    sync = (position in an item of the struct that holds the SyncBN pointers, its field for this rank's buffer, for the gathered
    one, for the gathered one's stride, floats per hidden column: forward 3 -- (n, mean, M2) -- backward 2 -- (S1, S2), added in
    rank order).  A batched call runs on the first side's seed, which every side then takes.  Returns the SyncBN buffers or None."""
    sides = [it[0] for it in items]
    comm = _sync_comm(sides)
    if comm is None and not _one_call(sides, key):
        for s, *args in items:
            one(s.tower._params(), *args, s.B, s.train, s.p_drop, s.seed, s.emb.device, s.tower._seed_dev)
        return None
    s0 = sides[0]
    params = [s.tower._params() for s in sides]
    args = [list(col) for col in zip(*(it[1:] for it in items))]
    call = lambda: many(params, *args, s0.B, s0.train, s0.p_drop, s0.seed, s0.emb.device, s0.tower._seed_dev)
    keep = None
    if comm is None:
        call()
    else:
        at, local, gathered, stride, per = sync
        widths = [per * s.tower.tower_hidden_dims[1] for s in sides]
        loc = torch.empty(sum(widths), dtype=torch.float32, device=s0.emb.device)
        where = [(it[at], p, 4 * sum(widths[:k])) for k, (it, p) in enumerate(zip(items, params))]
        for s, (holder, p, off) in zip(sides, where):
            setattr(holder, local, loc.data_ptr() + off)
            p.sync_phase, p.sync_ranks, p.rng_row_offset = 1, comm.world, comm.rank * s.B
        try:
            call()                                  # stops at the local statistics / column sums
            allg = comm.all_gather(loc)
            for holder, p, off in where:
                setattr(holder, gathered, allg.data_ptr() + off)
                setattr(holder, stride, loc.numel())
                p.sync_phase = 2
            call()                                  # merges every rank's share in rank order
        finally:
            for p in params:
                p.sync_phase = 0
        keep = (loc, allg)
    for s in sides:
        s.seed = s0.seed
    return keep


class BaseTower(nn.Module):
    def __init__(self, categorical_keys: List[str], metadata_path: str = "meta/metadata.csv", table_name: str = "notice",
                 categorical_embedding_dim: int = 64, dense_input_dim: int = 256,
                 tower_hidden_dims: Optional[List[int]] = None, final_embedding_dim: int = 128, dropout_rate: float = 0.2,
                 device="cuda:0", embedding_grad: Optional[str] = None, materialize_tables: bool = True,
                 mlp_dtype: Optional[str] = None, categorical_position_weights=None, categorical_pooling=None):
        super().__init__()
        if tower_hidden_dims is None:
            tower_hidden_dims = [256, 128]
        if categorical_pooling is not None and tower_hidden_dims[0] % 4 != 0:
            # the pooled block starts at column tower_hidden_dims[0] of the tower input and is written in 16-byte pieces (the pooled
            # lookup has no scalar form, unlike the plain one); the embedder checks embedding_dim itself
            raise ValueError(f"bag mode (categorical_pooling=...) needs tower_hidden_dims[0] to be a multiple of 4, got {tower_hidden_dims[0]}")
        self.mlp_dtype = mlp_dtype or settings.mlp_dtype
        if self.mlp_dtype not in ("fp32", "bf16"):
            raise ValueError(f"mlp_dtype must be 'fp32' or 'bf16', got {self.mlp_dtype!r}")
        # bf16 MLP: the tower input x = [projection | embedding rows] lives in bf16 -- bit-identical results (the GEMMs
        # that read x round it to bf16 anyway) at half the bytes: lookup 15.7 -> 9.2 us, step -7 us at B = 8192.
        # A bf16 d_x (settings.tower_io_dtype = dx | both) is implemented but measures no faster (0.354 vs 0.352 ms per step: the
        # segmented reduction is bound by its dependent trips, not by bytes, and the data-gradient GEMM stores 2-byte
        # pieces) and rounds the per-slot row gradients, so it stays off.
        io = settings.tower_io_dtype if self.mlp_dtype == "bf16" else "none"
        if io not in ("none", "x", "dx", "both"):
            raise ValueError(f"settings.tower_io_dtype must be none|x|dx|both, got {io!r}")
        self.x_dtype = torch.bfloat16 if io in ("x", "both") else torch.float32
        self.dx_dtype = torch.bfloat16 if io in ("dx", "both") else torch.float32
        # the fused launches against the separate kernels they replaced (tests): config.Settings
        self.unfused_tail, self.unfused_front, self.unfused_back = settings.tower_unfused_tail, settings.tower_unfused_front, settings.tower_unfused_back
        self.front_gather = settings.front_gather    # a captured step's forward gathers the embedding rows in its front launch (_front_gathers)
        self.categorical_keys = list(categorical_keys)
        self.exchange = None            # set by the distributed task: sharded-table row exchange
        self.sync_comm = None           # set by the distributed task (sync_bn=True): BN statistics over all ranks' rows
        self.pack_for_score = False     # set by the train task (score_dtype='bf16'): also emit the score kernels' operand images
        self._last_packed = None
        self.pack_scale = 1.0           # the images hold bf16(pack_scale * emb)
        self._seed_dev = None           # set by GraphedTrainStep: device word added to the dropout seed
        self._w16 = None                # set by GraphedTrainStep while its step runs: (bf16 shadow of w_proj, [bf16 shadows of the blocks' weights])
        self._seed_override = None      # tests: a fixed dropout seed instead of one drawn from torch's CPU generator
        self.device = device
        self.tower_hidden_dims = list(tower_hidden_dims)
        self.final_embedding_dim = final_embedding_dim
        self.dropout_rate = float(dropout_rate)
        self.dense_input_dim = dense_input_dim
        dev = torch.device(device)
        self.categorical_embedder = CategoricalEmbedder(keys=self.categorical_keys, metadata_path=metadata_path,
                                                        table_name=table_name, embedding_dim=categorical_embedding_dim,
                                                        device=str(dev), embedding_grad=embedding_grad,
                                                        materialize=materialize_tables, pooling=categorical_pooling)
        if categorical_position_weights is not None:      # {key: max_len}: learned position weights of the pooled keys (refusals: there)
            self.categorical_embedder.add_position_weights(categorical_position_weights)
        self.dense_projection = nn.Linear(dense_input_dim, tower_hidden_dims[0])
        self._build_mlp(categorical_embedding_dim, tower_hidden_dims, final_embedding_dim, dropout_rate)
        self._struct_key = None
        self._params_struct = None
        self.to(dev)                    # (the reference hard-codes cuda:0 here: base_tower.py:69)

    def _build_mlp(self, categorical_embedding_dim, tower_hidden_dims, final_embedding_dim, dropout_rate):
        in_dim = tower_hidden_dims[0] + len(self.categorical_keys) * categorical_embedding_dim
        layers = []
        for h in tower_hidden_dims[1:]:
            layers += [nn.Linear(in_dim, h), nn.ReLU(), nn.BatchNorm1d(h), nn.Dropout(dropout_rate)]
            in_dim = h
        layers.append(nn.Linear(in_dim, final_embedding_dim))
        self.mlp = nn.Sequential(*layers)

    # ---- parameter plumbing ----------------------------------------------------------------------
    @property
    def n_hidden(self) -> int:
        return len(self.tower_hidden_dims) - 1

    def dense_parameters(self) -> List[torch.Tensor]:
        """Order = order of the gradients tt_tower_mlp_bwd returns."""
        ps = [self.dense_projection.weight, self.dense_projection.bias]
        for i in range(self.n_hidden):
            lin, bn = self.mlp[4 * i], self.mlp[4 * i + 2]
            ps += [lin.weight, lin.bias, bn.weight, bn.bias]
        ps += [self.mlp[4 * self.n_hidden].weight, self.mlp[4 * self.n_hidden].bias]
        return ps

    def _params(self):
        nh = self.n_hidden
        lins = [self.mlp[4 * i] for i in range(nh)]
        bns = [self.mlp[4 * i + 2] for i in range(nh)]
        out = self.mlp[4 * nh]
        tensors = [self.dense_projection.weight, self.dense_projection.bias, out.weight, out.bias]
        for lin, bn in zip(lins, bns):
            tensors += [lin.weight, lin.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var]
        w16 = self._w16
        key = tuple(t.data_ptr() for t in tensors) + tuple(b.num_batches_tracked.data_ptr() for b in bns) + (self.mlp_dtype, self.x_dtype, self.dx_dtype, self.unfused_tail, self.unfused_front, self.unfused_back, self.front_gather) + \
            ((w16[0].data_ptr(),) + tuple(w.data_ptr() for w in w16[1]) if w16 is not None else ())
        if key != self._struct_key:
            for t in tensors:
                if t.dtype != torch.float32 or not t.is_contiguous():
                    raise TypeError("tower parameters must be contiguous float32")
            E = self.categorical_embedder.embedding_dim
            self._params_struct = ops.tower_params_struct(
                self.dense_input_dim, self.tower_hidden_dims[0], len(self.categorical_keys) * E, self.tower_hidden_dims[1:],
                self.final_embedding_dim, self.dense_projection.weight, self.dense_projection.bias,
                [l.weight for l in lins], [l.bias for l in lins], [b.weight for b in bns], [b.bias for b in bns],
                [b.running_mean for b in bns], [b.running_var for b in bns], out.weight, out.bias,
                bn_nbt=[b.num_batches_tracked for b in bns],
                compute_dtype=ops.TT_BF16 if self.mlp_dtype == "bf16" else ops.TT_F32,
                x_dtype=ops.TT_BF16 if self.x_dtype == torch.bfloat16 else ops.TT_F32,
                dx_dtype=ops.TT_BF16 if self.dx_dtype == torch.bfloat16 else ops.TT_F32,
                flags=(ops.L.TT_TOWER_UNFUSED_TAIL if self.unfused_tail else 0) | (ops.L.TT_TOWER_UNFUSED_FRONT if self.unfused_front else 0) | (ops.L.TT_TOWER_UNFUSED_BACK if self.unfused_back else 0) | (0 if self.front_gather else ops.L.TT_TOWER_UNFUSED_GATHER),
                w_proj_bf16=None if w16 is None else w16[0], w_bf16=() if w16 is None else w16[1])
            self._struct_key = key
        return self._params_struct

    @property
    def x_width(self) -> int:
        return self.tower_hidden_dims[0] + len(self.categorical_keys) * self.categorical_embedder.embedding_dim

    # ---- forward: src/towers/tower/base_tower.py:101-147 ------------------------------------------
    @_no_dynamo
    def forward(self, tower_input: Dict[str, torch.Tensor]) -> torch.Tensor:
        return run_towers([self], [tower_input])[0]


class NoticeTower(BaseTower):
    def __init__(self, categorical_keys: List[str], metadata_path: str = "meta/metadata.csv",
                 categorical_embedding_dim: int = 64, dense_input_dim: int = 256,
                 tower_hidden_dims: Optional[List[int]] = None, final_embedding_dim: int = 128, dropout_rate: float = 0.2,
                 device="cuda:0", embedding_grad: Optional[str] = None, materialize_tables: bool = True,
                 mlp_dtype: Optional[str] = None, categorical_position_weights=None, categorical_pooling=None):
        super().__init__(categorical_keys=categorical_keys, metadata_path=metadata_path, table_name="notice",
                         categorical_embedding_dim=categorical_embedding_dim, dense_input_dim=dense_input_dim,
                         tower_hidden_dims=tower_hidden_dims, final_embedding_dim=final_embedding_dim,
                         dropout_rate=dropout_rate, device=device, embedding_grad=embedding_grad,
                         materialize_tables=materialize_tables, mlp_dtype=mlp_dtype,
                         categorical_position_weights=categorical_position_weights, categorical_pooling=categorical_pooling)


class CompanyTower(BaseTower):
    def __init__(self, categorical_keys: List[str], metadata_path: str = "meta/metadata.csv",
                 categorical_embedding_dim: int = 64, dense_input_dim: int = 128,
                 tower_hidden_dims: Optional[List[int]] = None, final_embedding_dim: int = 128, dropout_rate: float = 0.2,
                 device="cuda:0", embedding_grad: Optional[str] = None, materialize_tables: bool = True,
                 mlp_dtype: Optional[str] = None, categorical_position_weights=None, categorical_pooling=None):
        super().__init__(categorical_keys=categorical_keys, metadata_path=metadata_path, table_name="company",
                         categorical_embedding_dim=categorical_embedding_dim, dense_input_dim=dense_input_dim,
                         tower_hidden_dims=tower_hidden_dims, final_embedding_dim=final_embedding_dim,
                         dropout_rate=dropout_rate, device=device, embedding_grad=embedding_grad,
                         materialize_tables=materialize_tables, mlp_dtype=mlp_dtype,
                         categorical_position_weights=categorical_position_weights, categorical_pooling=categorical_pooling)


# --------------------------------------------------------------------------------------------------
# one autograd node for >= 1 towers (lookup and table gradient fused across towers that share a store)
# --------------------------------------------------------------------------------------------------
def run_towers(towers: Sequence[BaseTower], inputs: Sequence[Dict]) -> List[torch.Tensor]:
    flat, bag_lengths, w_inputs = [], [], []
    for tw, inp in zip(towers, inputs):
        dev = tw.categorical_embedder.store.device
        dense = inp["dense"].to(dev)
        kjt = inp["kjt"]
        kjt = kjt.to(dev) if hasattr(kjt, "to") else kjt
        values = kjt.values()
        # a bag-mode embedder also reads the bags' lengths; any other reads the values only, as before
        # (a captured step's static KJT: values() is a buffer of a fixed capacity and bag_count the device word with the id count the
        # host handed over -- the pair says "capacity form": ops.BagSide)
        # a KJT with weights: (lengths, count or None, weights) -- the pooled lookup's weighted form
        count = getattr(kjt, "bag_count", None)
        if not tw.categorical_embedder.bag_mode:
            weights = kjt_weights(kjt)
            refuse_weights(weights, type(tw).__name__)
        else:                                     # the KJT's own weights, or the embedder's position weights expanded over its bags
            weights = tw.categorical_embedder.bag_weights(kjt)
        lengths = kjt.lengths() if tw.categorical_embedder.bag_mode else None
        if isinstance(weights, ops.BagPosWeights):
            # a static KJT of an embedder with position weights: the lookup reads the parameter by position.  With autograd on the
            # parameter is a tensor input of the node (its gradient: the backward's capacity-form chain); otherwise it is data
            if weights.param.requires_grad and torch.is_grad_enabled():
                bag_lengths.append((lengths, count, _WeightInput(len(w_inputs), weights)))
                w_inputs.append(weights.param)
            else:
                bag_lengths.append((lengths, count, weights))
        elif lengths is not None and weights_need_grad(weights):
            # weights somebody differentiates: tensor inputs of the node, behind every tower's own (the entry names which)
            bag_lengths.append((lengths, count, _WeightInput(len(w_inputs))))
            w_inputs.append(weights)
        elif lengths is not None and weights is not None:
            bag_lengths.append((lengths, count, weights))
        else:
            bag_lengths.append(lengths if count is None or lengths is None else (lengths, count))
        flat += [dense, values] + tw.dense_parameters() + tw.categorical_embedder.table_parameters()
    outs = _TowersFn.apply(tuple(towers), tuple(bag_lengths), *flat, *w_inputs)
    outs = list(outs) if isinstance(outs, tuple) else [outs]
    for tw, o in zip(towers, outs):                      # hand the packed images to the score step with the rows they belong to
        if tw._last_packed is not None:
            o._tt_packed, tw._last_packed = tw._last_packed, None
    return outs


class _Side:
    __slots__ = ("tower", "B", "acts", "acts_struct", "buf", "x", "emb", "train", "seed", "p_drop", "sync_keep", "packed", "values",
                 "lengths", "count", "weights", "w_flat", "pos_weights")


class _WeightInput:
    """In the place of a side's weights in _TowersFn's bag_lengths: they are tensor input `index` behind the towers' own inputs,
    and the backward returns their gradient.  source: the input is a position-weight PARAMETER (ops.BagPosWeights, whose directory
    says how the lookup reads it), not one weight per id."""
    __slots__ = ("index", "source")

    def __init__(self, index: int, source=None):
        self.index = index
        self.source = source


class _TowersFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, towers, bag_lengths, *flat):
        """bag_lengths: per tower, the KJT's lengths() for a bag-mode embedder -- or (lengths, count) for the capacity form, or
        (lengths, count or None, weights) for a KJT with per-id weights -- None for any other (its lengths are not read).  weights a
        _WeightInput: differentiable weights, passed behind the towers' inputs in `flat`"""
        if len(bag_lengths) != len(towers):
            raise ValueError(f"{len(towers)} towers but {len(bag_lengths)} bag-length entries")
        sides: List[_Side] = []
        pos = 0
        grad_on = any(ctx.needs_input_grad)       # (grad mode is always off inside Function.forward)
        spans = []
        lookups: Dict[int, list] = {}
        bag_lookups: Dict[tuple, list] = {}      # (store, batch size) -> [(side, ops.BagSide)]
        w_base = len(flat) - sum(isinstance(l, tuple) and isinstance(l[-1], _WeightInput) for l in bag_lengths)
        for tw, lengths in zip(towers, bag_lengths):
            emb = tw.categorical_embedder
            nd, nt = len(tw.dense_parameters()), len(emb.table_parameters())
            dense, values = flat[pos], flat[pos + 1]
            spans.append((pos, nd, nt))
            pos += 2 + nd + nt
            dev = emb.store.device
            if dense.dim() != 2 or dense.shape[1] != tw.dense_input_dim:
                raise ValueError(f"dense input must be [B, {tw.dense_input_dim}], got {tuple(dense.shape)}")
            dense = dense.to(dtype=torch.float32).contiguous()
            values = values.to(dtype=torch.int64).contiguous()
            B, K, E = dense.shape[0], len(emb.keys), emb.embedding_dim
            count = weights = None
            if isinstance(lengths, tuple):      # (lengths, count): the capacity form; (lengths, count, weights): weighted bags
                lengths, count, weights = lengths if len(lengths) == 3 else (*lengths, None)
            w_ref = weights.index if isinstance(weights, _WeightInput) else None
            pos_weights = weights.source if w_ref is not None else (weights if isinstance(weights, ops.BagPosWeights) else None)
            if w_ref is not None:
                w_ref += w_base
                weights = flat[w_ref]
                w_like = (weights.shape, weights.dtype, weights.device)
            if pos_weights is not None:         # the parameter as the lookup's source (its data: autograd sees the node's input)
                pos_weights, weights = ops.BagPosWeights(pos_weights.param.detach(), pos_weights.pw_offset, pos_weights.pw_len), None
            if emb.bag_mode:
                if lengths is None or lengths.numel() != B * K:
                    raise ValueError(f"bag mode: the kjt must carry B*K = {B}*{K} bag lengths, got "
                                     f"{'none' if lengths is None else lengths.numel()}")
                if tw.exchange is not None:         # the sharded step pools across the exchange's forward_bags -- or refuses, before any launch
                    if not hasattr(tw.exchange, "forward_bags"):
                        raise ValueError("bag mode (categorical_pooling) is not supported with the sharded table exchange")
                    if pos_weights is not None:
                        raise ValueError("learned position weights are not supported with the sharded table exchange: the weight "
                                         "gradient does not cross it (per-id data weights on the KJT are)")
                    if w_ref is not None:
                        raise ValueError("per-id weights that require grad are not supported with the sharded table exchange: it forms "
                                         "no gradient for them -- detach them")
                    if count is not None:
                        raise ValueError("the sharded table exchange has no capacity form of the pooled lookup (a static KJT with "
                                         "bag_count): run the eager step on an ordinary KJT")
                lengths = lengths.to(device=dev, dtype=torch.int64).contiguous()
                if weights is not None:
                    weights = weights.to(device=dev, dtype=torch.float32).contiguous()
            elif values.numel() != B * K:
                raise ValueError(f"kjt carries {values.numel()} ids but the batch needs B*K = {B}*{K}")
            s = _Side()
            s.lengths = lengths if emb.bag_mode else None
            s.count = count if emb.bag_mode else None
            s.weights = weights if emb.bag_mode else None
            s.pos_weights = pos_weights if emb.bag_mode else None
            s.w_flat = None if w_ref is None else (w_ref, *w_like)      # where the weights' gradient goes, and what it must look like
            s.tower, s.B, s.train = tw, B, tw.training
            s.p_drop = tw.dropout_rate if tw.training else 0.0
            s.seed = 0 if s.p_drop <= 0 else (tw._seed_override if tw._seed_override is not None else
                                              int(torch.empty((), dtype=torch.int64).random_().item()))
            s.values = values
            s.acts = (dense,)
            sides.append(s)
        # a graph-replayed step's hand-over launch may ALREADY have looked the rows up into persistent input buffers
        # (ops.batch_ingest(table=...): tt_batch_ingest_lookup): then x is that buffer and no lookup launch follows
        pre = {}
        if towers[0].exchange is None and grad_on:
            by_store: Dict[int, list] = {}
            for s in sides:
                emb = s.tower.categorical_embedder
                if s.B and len(emb.keys) and not emb.bag_mode:
                    by_store.setdefault(id(emb.store), []).append(s)
            for group in by_store.values():
                st = group[0].tower.categorical_embedder.store
                xs = st.x_for([g.values for g in group], [(g.B, g.tower.x_width, g.tower.x_dtype) for g in group])
                if xs is not None:
                    for g, x in zip(group, xs):
                        pre[id(g)] = x
        for s in sides:
            tw, B, dense, values = s.tower, s.B, s.acts[0], s.values
            emb = tw.categorical_embedder
            K, E = len(emb.keys), emb.embedding_dim
            dev = emb.store.device
            # one flat activation buffer: x | (pre_i, act_i)* | (mean_i, rstd_i)* | y
            hid = tw.tower_hidden_dims[1:]
            px = pre.get(id(s))
            x_f32 = tw.x_dtype == torch.float32 and px is None
            sizes = [_al(B * tw.x_width) if x_f32 else 0] + [_al(B * h) for h in hid for _ in (0, 1)] + \
                    [_al(h) for h in hid for _ in (0, 1)] + [_al(B * tw.final_embedding_dim)]
            s.buf = torch.empty(sum(sizes), dtype=torch.float32, device=dev)
            offs = [0]
            for z in sizes:
                offs.append(offs[-1] + z)
            s.x = px if px is not None else (s.buf[:B * tw.x_width].view(B, tw.x_width) if x_f32 else
                                             torch.empty((B, tw.x_width), dtype=tw.x_dtype, device=dev))
            s.emb = torch.empty((B, tw.final_embedding_dim), dtype=torch.float32, device=dev)
            a = L.TowerActs()
            base, esz = s.buf.data_ptr(), 4
            a.dense, a.x, a.emb = dense.data_ptr(), s.x.data_ptr(), s.emb.data_ptr()
            nh = len(hid)
            for i in range(nh):
                a.pre[i] = base + esz * offs[1 + 2 * i]
                a.act[i] = base + esz * offs[2 + 2 * i]
                a.mean[i] = base + esz * offs[1 + 2 * nh + 2 * i]
                a.rstd[i] = base + esz * offs[2 + 2 * nh + 2 * i]
            a.y = base + esz * offs[1 + 4 * nh]
            s.packed = None
            if tw.pack_for_score and B:
                # the score kernels' bf16 operand images of the unit rows, written by the tower pass itself (tt_tower_acts.emb_packed)
                s.packed = torch.empty(L.load().tt_score_pack_bytes(B, tw.final_embedding_dim), dtype=torch.uint8, device=dev)
                a.emb_packed, a.emb_pack_scale = s.packed.data_ptr(), float(tw.pack_scale)
            s.acts_struct = a
            if K and B and emb.bag_mode:     # pooled bags: launches and plans of their own, beside the plain sides of the store
                bag_lookups.setdefault((id(emb.store), B), []).append((s, emb.bag_side(values, s.lengths, s.x[:, tw.tower_hidden_dims[0]:], s.count, s.weights, s.pos_weights)))
            elif K and B:
                lookups.setdefault(id(emb.store), []).append((s, emb.lookup_side(values, s.x[:, tw.tower_hidden_dims[0]:]), px is not None))
        # fused lookup (+ duplicate-row plan when a backward will follow) per store
        plans = []
        live = [s for s in sides if s.B]
        exch = towers[0].exchange
        ctx.exch, ctx.exch_state = exch, None
        if exch is not None:            # sharded table: ids -> owners, pooled rows <- owners (distributed.py)
            group = [g for grp in lookups.values() for g in grp]
            bags = [g for grp in bag_lookups.values() for g in grp]
            if bags:
                # at least one tower pools: every side goes through ONE pooled route (one plan, one set of all-to-alls per step) --
                # a plain side as sum bags of length one, bit-exact copies of its rows
                Bx = bags[0][0].B
                both = bags + [(g[0], ops.bag_side_from_lookup(g[1], g[0].B)) for g in group]
                if any(g[0].B != Bx for g in both):
                    raise ValueError("the sharded table exchange pools the towers of one step together: they must share one batch size")
                both.sort(key=lambda g: live.index(g[0]))                 # tower order: the order the backward hands d_x over in
                ctx.exch_state = exch.forward_bags([g[1] for g in both], Bx, grad_on)
                ctx.exch_sides = [g[0] for g in both]
            elif group:
                ctx.exch_state = exch.forward([g[1] for g in group], group[0][0].B, grad_on)
                ctx.exch_sides = [g[0] for g in group]
            lookups, bag_lookups = {}, {}
        for group in lookups.values():
            store: EmbeddingStore = group[0][0].tower.categorical_embedder.store
            B = group[0][0].B
            if any(g[0].B != B for g in group):
                # different batch sizes cannot share one launch: fall back to one launch per side
                for g in group:
                    rows = ops.embed_lookup(store.weight, [g[1]], g[0].B, want_rows=grad_on)
                    plans.append([store, [g[0]], ops.dedup_plan(rows, store.rows) if grad_on else None])
                continue
            # a graph-replayed step hands the batch over with ops.batch_ingest, which leaves the fused rows of exactly these id
            # tensors in key-major order: the plan sorts those, the lookup need not write its slot-major copy
            km = store.rows_km_for([g[1].ids for g in group]) if (grad_on and 0 < B <= ops.KEYED_MAX_B) else None
            sm = store.rows_sm_for([g[1].ids for g in group]) if km is not None else None
            if all(g[2] for g in group) and km is not None:
                rows = None                             # the hand-over launch has filled x already (tt_batch_ingest_lookup)
            elif sm is not None and store.weight.shape[1] % 4 == 0 and all(g[1].out.stride(0) % 4 == 0 for g in group):
                rows = None                             # ... or left the clamped fused rows in slot order: no id decoding here,
                if not _front_gathers(group, live, store, sm, B):     # and no launch where the towers' front gathers from them itself
                    ops.embed_lookup_rows(store.weight, sm, [g[1] for g in group], B)
            else:
                rows = ops.embed_lookup(store.weight, [g[1] for g in group], B, want_rows=grad_on and km is None)
            plans.append([store, [g[0] for g in group], None, rows if km is None else km, grad_on, km is not None])
        # pooled bags: one launch per (store, batch size) writes the pooled block straight into x[:, h0:]; the general plan over the
        # positions' rows (M = nnz: the keyed plans sort B ids per key, a bag-mode key holds any number)
        bag_plans = []
        for group in bag_lookups.values():
            store = group[0][0].tower.categorical_embedder.store
            bag = ops.embed_bag_lookup(store.weight, [g[1] for g in group], group[0][0].B, want_rows=grad_on)
            if bag is not None and bag.nnz:
                bag_plans.append((store, [g[0] for g in group], ops.bag_dedup_plan(bag, store.rows), bag))
        ctx.bag_plans = bag_plans
        # duplicate-row plans: depend on ids only, first needed in the backward.  In line on the launch stream (a side stream
        # overlapped the sort with the score kernels, but a captured graph with two streams is replayed node by node with
        # cross-queue signals: 4-6 us gaps in front of eight kernels -- as much as the overlap saved), and BEFORE the towers'
        # forward: with TT_OPT_DEFER_RIDERS the plan's compaction then rides in the towers' tail launch, and the sort itself is
        # queued by this call and issued by the towers' forward between its front and tail kernels (it hosts the workgroups that
        # finish the BatchNorm statistics once per tower: tt_riders.h)
        for pl in plans:
            if len(pl) == 6:
                store, psides, _, rows, want_plan, key_major = pl
                plan = None
                if want_plan:
                    Bs = psides[0].B
                    if 0 < Bs <= ops.KEYED_MAX_B:       # per-key LDS sorts (2 launches)
                        plan = ops.dedup_plan_keyed(rows, [len(q.tower.categorical_embedder.keys) for q in psides], Bs, key_major,
                                                    E=int(store.E))
                    else:
                        plan = ops.dedup_plan(rows, store.rows)
                    plan.keep = rows                    # keep the sort input alive until it has run
                pl[:] = [store, psides, plan]
        keep = _run_pass([(s, s.acts_struct) for s in live], ops.tower_fwd, ops.towers_fwd, _fwd_key,
                         (1, "bn_sync_local", "bn_sync_all", "bn_sync_stride", 3))
        for s in live if keep else ():
            s.sync_keep = keep
        for s in sides:
            s.tower._last_packed = None if s.packed is None else (s.packed, float(s.tower.pack_scale))
        ctx.sides, ctx.plans, ctx.spans, ctx.n_flat = sides, plans, spans, len(flat)
        # hand out aliases: keeping the returned objects themselves on ctx would form a reference cycle
        outs = tuple(s.emb.view(s.emb.shape) for s in sides)
        ctx.mark_non_differentiable(*[o for o, s in zip(outs, sides) if s.B == 0])
        return outs

    @staticmethod
    def backward(ctx, *d_embs):
        grads = [None] * ctx.n_flat
        dxs = {}
        exch = ctx.exch
        if exch is not None and exch.world > 1:            # global objective = mean over ranks of the local losses
            d_embs = [None if d is None else d * (1.0 / exch.world) for d in d_embs]
        flat_grads = []
        work = [(s, d, sp) for s, d, sp in zip(ctx.sides, d_embs, ctx.spans) if s.B and d is not None]
        prepared = []
        # one buffer for the whole pass: [dense gradients of every tower | per-tower scratch] -- the dense part is ONE
        # contiguous range, so the data-parallel sum is a single all-reduce however many towers there are
        side_sizes = []
        for s, _, _ in work:
            tw = s.tower
            side_sizes.append(([_al(p.numel()) for p in tw.dense_parameters()],
                               [_al(s.B * tw.x_width) if tw.dx_dtype == torch.float32 else 0] +
                               [_al(s.B * h) for h in tw.tower_hidden_dims[1:]] + [_al(s.B * tw.final_embedding_dim)]))
        dense_total = sum(sum(d) for d, _ in side_sizes)
        buf = torch.empty(dense_total + sum(sum(r) for _, r in side_sizes), dtype=torch.float32, device=work[0][0].emb.device) if work else None
        dense_at, scratch_at = 0, dense_total
        for (s, d_emb, (pos, nd, nt)), (dsz, rsz) in zip(work, side_sizes):
            tw = s.tower
            dev = s.emb.device
            d_emb = d_emb.to(dtype=torch.float32).contiguous()
            dps = tw.dense_parameters()
            hid = tw.tower_hidden_dims[1:]
            B = s.B
            dx_f32 = tw.dx_dtype == torch.float32
            offs = [dense_at]                                   # absolute offsets in buf: dense entries, then this tower's scratch
            for z in dsz[:-1]:
                offs.append(offs[-1] + z)
            dense_at += sum(dsz)
            offs.append(scratch_at)
            for z in rsz:
                offs.append(offs[-1] + z)
            scratch_at += sum(rsz)
            base = buf.data_ptr()
            views = [buf[offs[i]:offs[i] + p.numel()].view(p.shape) for i, p in enumerate(dps)]
            g = L.TowerGrads()
            g.w_proj, g.b_proj = base + 4 * offs[0], base + 4 * offs[1]
            for i in range(len(hid)):
                g.w[i], g.b[i] = base + 4 * offs[2 + 4 * i], base + 4 * offs[3 + 4 * i]
                g.bn_w[i], g.bn_b[i] = base + 4 * offs[4 + 4 * i], base + 4 * offs[5 + 4 * i]
                g.scratch[i] = base + 4 * offs[len(dps) + 1 + i]
            g.w_out, g.b_out = base + 4 * offs[len(dps) - 2], base + 4 * offs[len(dps) - 1]
            d_x = buf[offs[len(dps)]:offs[len(dps)] + B * tw.x_width].view(B, tw.x_width) if dx_f32 else \
                torch.empty((B, tw.x_width), dtype=tw.dx_dtype, device=dev)
            g.d_x = d_x.data_ptr()
            g.d_y = base + 4 * offs[len(dps) + 1 + len(hid)]
            prepared.append((s, d_emb, g))
            if _DEBUG_KEEP is not None:      # tests/debug/tail_diff.py: keep the backward scratch for inspection
                _DEBUG_KEEP.append({"buf": buf, "offs": offs, "n_dense": len(dps), "hidden": hid, "B": B, "acts": s.buf, "emb": s.emb,
                                    "d_emb": d_emb})
            for i, v in enumerate(views):
                grads[pos + 2 + i] = v
            dxs[id(s)] = d_x[:, tw.tower_hidden_dims[0]:]
        _run_pass([(s, s.acts_struct, d, g) for s, d, g in prepared], ops.tower_bwd, ops.towers_bwd, lambda s: (s.train, s.p_drop, s.seed),
                  (3, "s_sync_local", "s_sync_all", "s_sync_stride", 2))
        if exch is not None:
            # the exchange's backward first: its local reduction is the launch that hosts a queued (deferred) slab reduction
            if ctx.exch_state is not None:
                srcs = []
                for s in ctx.exch_sides:
                    K = len(s.tower.categorical_embedder.keys)
                    d = dxs.get(id(s))
                    if d is None:
                        d = torch.zeros((s.B, K * exch.E), dtype=s.tower.dx_dtype, device=s.emb.device)
                    srcs.append((d, K))
                exch.backward(ctx.exch_state, srcs, ctx.exch_sides[0].B)
            if buf is not None and dense_total:
                flat_grads.append(buf[:dense_total])
                # a slab reduction that is STILL queued owes w[0] / b[0] / w_proj / b_proj of this buffer: it must have run before
                # anything outside the library reads the dense gradients (GraphedTrainStep sets the deferral)
                L.flush_deferred(buf.device)
            exch.all_reduce_dense(flat_grads)
        # table gradients: one fused segmented reduction per store
        for store, plan_sides, plan in ctx.plans:
            if plan is None:
                continue
            srcs = []
            for s in plan_sides:
                K = len(s.tower.categorical_embedder.keys)
                d = dxs.get(id(s))
                if d is None:       # this tower received no gradient: contribute zeros
                    d = torch.zeros((s.B, K * store.E), dtype=s.tower.dx_dtype, device=store.device)
                srcs.append((d, K))
            # (filed under the sides' embedders: the per-side plans of a pass with unequal batch sizes, or of two passes over one
            # store, each keep their gradient until the optimiser steps)
            store.accumulate_grad(plan, srcs, plan_sides[0].B, members=[s.tower.categorical_embedder for s in plan_sides])
        for store, plan_sides, plan, bag in ctx.bag_plans:      # the bag-mode sides: reduced from d_x[:, h0:] in dx_dtype through bag_of
            srcs = []
            for s in plan_sides:
                K = len(s.tower.categorical_embedder.keys)
                d = dxs.get(id(s))
                if d is None:
                    d = torch.zeros((s.B, K * store.E), dtype=s.tower.dx_dtype, device=store.device)
                srcs.append((d, K))
            store.accumulate_grad(plan, srcs, plan_sides[0].B, members=[s.tower.categorical_embedder for s in plan_sides], bag=bag)
            # the gradient for differentiable per-id weights, from the same views; no side asks: no launch
            want = [s.w_flat is not None and ctx.needs_input_grad[2 + s.w_flat[0]] for s in plan_sides]
            if any(want):
                gs = ops.bag_weight_grad(store.weight, bag, srcs, plan_sides[0].B, want)
                for i, (s, g) in enumerate(zip(plan_sides, gs)):
                    if g is None:
                        continue
                    at, shape, dtype, wdev = s.w_flat
                    if s.pos_weights is not None:
                        # the parameter's gradient: the per-id gradient over the side's whole capacity (0 where no bag covers) summed
                        # through the offsets tt_bag_prepare formed -- no launch here depends on how many ids are live
                        pw, K = s.pos_weights, len(s.tower.categorical_embedder.keys)
                        side = ops.PosWeightSide(s.lengths, pw.pw_offset, pw.pw_len, g.numel(), K, offsets=bag.offsets[i])
                        g = ops.bag_position_weights_bwd(pw.param, [side], s.B, [g])
                    grads[at] = g.reshape(shape).to(device=wdev, dtype=dtype)
        return (None, None, *grads)


def tower_dense_param_names(n_hidden: int) -> List[str]:
    names = ["dense_projection.weight", "dense_projection.bias"]
    for i in range(n_hidden):
        names += [f"mlp.{4 * i}.weight", f"mlp.{4 * i}.bias", f"mlp.{4 * i + 2}.weight", f"mlp.{4 * i + 2}.bias"]
    names += [f"mlp.{4 * n_hidden}.weight", f"mlp.{4 * n_hidden}.bias"]
    return names
