"""CategoricalEmbedder on one fused HBM-resident table.

Drop-in for the reference class of the same name (src/towers/cat_embed.py:11-190): same constructor,
same vocab rule (metadata category count + 10, 1000 when unknown: :50-85), same forward contract
(kjt -> dict of [B,E] or concatenated [B,K*E]; clamp to [0,V-1]; kjt None -> zeros of batch 1), same
state-dict keys (`embeddings.<key>.weight`, shape [V_k, E]).

Layout: all per-key tables of one store are rows of ONE [R, E] f32 tensor (key k owns rows
[off_k, off_k+V_k)); the per-key nn.Parameters are views into it, so optimisers, state_dict and
checkpoints see the reference's tensors while the lookup / gradient kernels see one row space.
"""
from __future__ import annotations

from pathlib import Path
from typing import Dict, List, Optional, Union

import torch
from ._lib import no_dynamo as _no_dynamo
import torch.nn as nn

from . import ops
from .config import settings
from .schema import category_counts


class EmbeddingStore:
    """One fused row space [R, E] (+ its gradient / optimiser state), shared by >= 1 embedders."""

    def __init__(self, E: int, device, grad_mode: str = "dense"):
        if grad_mode not in ("dense", "sparse"):
            raise ValueError(f"embedding_grad must be 'dense' or 'sparse', got {grad_mode!r}")
        self.E = E
        self.device = torch.device(device)
        self.grad_mode = grad_mode
        self.weight: Optional[torch.Tensor] = None      # [R, E] f32
        self.grad: Optional[torch.Tensor] = None        # dense mode: [R, E]
        # sparse mode: the gradients waiting for the optimiser, [(member embedders or None = the whole store, DedupPlan, grad_rows
        # [M, E])].  Entries over disjoint embedders coexist (towers passes of different batch sizes, or two autograd nodes, file one
        # per side): their rows are disjoint.  A new entry replaces every entry it overlaps: the latest backward wins (file_sparse_grad)
        self._sparse_pending: list = []
        self.defer_long_finish = False                  # GraphedTrainStep: the optimiser's launch finishes the long rows
        self.members: List["CategoricalEmbedder"] = []
        self.version = 0
        self._grad_counters = None                      # 4 int32 words the gradient reduction keeps zero between calls
        # set by GraphedTrainStep: (static id tensors per side, their _version at the last hand-over, rows_km[, x buffers]) -- the
        # fused rows of exactly those id tensors in key-major order, written by ops.batch_ingest.  A pass over other tensors, or
        # over these after anybody else wrote to them, does not see it (rows_km_for).  With the fused hand-over + lookup launch the
        # fourth entry holds, per side, the tower input x whose embedding columns that launch has ALREADY filled (x_for): valid for
        # one pass (`ingest_x_fresh`), because an optimiser step in between changes the table rows they were copied from.
        self.ingest = None
        self.ingest_x_fresh = False

    # ---- sparse mode: the pending gradients ------------------------------------------------------
    def sparse_grads(self) -> list:
        """Every pending (DedupPlan, grad_rows [M, E]), in the order of their embedders' first row (whichever order autograd ran
        the nodes in).  The optimiser applies each with the same step number: disjoint rows, so that is exactly one step."""
        key = lambda e: min((m.row_base for m in e[0]), default=0) if e[0] is not None else 0
        return [(plan, rows) for _, plan, rows in sorted(self._sparse_pending, key=key)]

    @property
    def sparse_grad(self):
        """The pending (DedupPlan, grad_rows) of a step that filed ONE gradient (every towers pass whose sides share a batch size
        does), None when nothing is pending.  With several pending entries there is no single pair: read sparse_grads()."""
        if len(self._sparse_pending) > 1:
            raise RuntimeError(f"{len(self._sparse_pending)} sparse gradients are pending on this store: read sparse_grads()")
        return self._sparse_pending[0][1:] if self._sparse_pending else None

    @sparse_grad.setter
    def sparse_grad(self, pair):
        self._sparse_pending = [] if pair is None else [(None, pair[0], pair[1])]

    def file_sparse_grad(self, plan, grad_rows, members=None):
        """File a gradient over the rows of `members` (embedders of this store; None: the whole store).  It replaces every pending
        entry that covers one of them -- sparse mode does not accumulate across backward passes -- and joins the others."""
        ids = None if members is None else {id(m) for m in members}
        keep = [e for e in self._sparse_pending if ids is not None and e[0] is not None and ids.isdisjoint(id(m) for m in e[0])]
        self._sparse_pending = keep + [(None if members is None else tuple(members), plan, grad_rows)]

    def rows_km_for(self, id_tensors) -> Optional[torch.Tensor]:
        """The key-major rows of ops.batch_ingest if they describe exactly `id_tensors` as they are now, else None."""
        reg = self.ingest
        if reg is None or len(reg[0]) != len(id_tensors):
            return None
        for t, r, v in zip(id_tensors, reg[0], reg[1]):
            if t.data_ptr() != r.data_ptr() or t.numel() != r.numel() or r._version != v:
                return None
        return reg[2]

    def rows_sm_for(self, id_tensors) -> Optional[torch.Tensor]:
        """The slot-order fused rows the hand-over launch left for exactly `id_tensors` (as they are now), or None."""
        reg = self.ingest
        if reg is None or len(reg) < 5 or reg[4] is None or self.rows_km_for(id_tensors) is None:
            return None
        return reg[4]

    def x_for(self, id_tensors, shapes) -> Optional[list]:
        """The towers' input buffers whose embedding columns the hand-over launch has already filled for exactly `id_tensors` (as
        they are now), or None: then the lookup runs as its own launch.  shapes: per side (B, x_width, dtype).  One pass only."""
        reg = self.ingest
        if reg is None or len(reg) < 4 or reg[3] is None or not self.ingest_x_fresh or self.rows_km_for(id_tensors) is None:
            return None
        xs = reg[3]
        if len(xs) != len(shapes) or any(tuple(x.shape) != (b, w) or x.dtype != dt for x, (b, w, dt) in zip(xs, shapes)):
            return None
        self.ingest_x_fresh = False
        return xs

    def grad_counters(self) -> Optional[torch.Tensor]:
        """Allocated on first use OUTSIDE a graph capture (a zero-fill inside one would become a memset node: DESIGN.md section 6);
        while capturing without them, the reduction falls back to its own zeroing launch."""
        if self._grad_counters is None or self._grad_counters.device != self.device:
            if self.device.type != "cuda" or torch.cuda.is_current_stream_capturing():
                return None
            self._grad_counters = torch.zeros(4, dtype=torch.int32, device=self.device)
        return self._grad_counters

    @property
    def rows(self) -> int:
        return 0 if self.weight is None else self.weight.shape[0]

    def append_rows(self, n: int) -> int:
        new = torch.empty((n, self.E), dtype=torch.float32, device=self.device)
        nn.init.normal_(new)                             # nn.Embedding default init N(0,1)
        base = self.rows
        self.weight = new if self.weight is None else torch.cat([self.weight, new])
        self.grad, self.sparse_grad = None, None
        self.version += 1
        return base

    def apply(self, fn):
        new = fn(self.weight)
        if new is not self.weight:
            if new.dtype != torch.float32:
                raise TypeError("embedding tables are kept in float32")
            self.weight = new
            self.device = new.device
            self.grad = None if self.grad is None else fn(self.grad)
            self.sparse_grad = None
            self.version += 1

    @staticmethod
    def fuse(stores: List["EmbeddingStore"]) -> "EmbeddingStore":
        """Concatenate several stores into one row space and rebind their embedders."""
        uniq = []
        for s in stores:
            if all(s is not u for u in uniq):
                uniq.append(s)
        if len(uniq) == 1:
            return uniq[0]
        first = uniq[0]
        if any(s.E != first.E for s in uniq):
            raise ValueError("cannot fuse embedding stores of different embedding_dim")
        fused = EmbeddingStore(first.E, first.device, first.grad_mode)
        fused.weight = torch.cat([s.weight.to(first.device) for s in uniq])
        base = 0
        for s in uniq:
            for m in s.members:
                m._rebind(fused, m.row_base + base)
            base += s.rows
        return fused

    def optim_parameters(self):
        """The nn.Parameters an optimiser sees for this row space (per-key views)."""
        return [p for m in self.members for p in m.table_parameters()]

    def bind_grads(self):
        for m in self.members:
            m._bind_grads()

    # ---- gradient bookkeeping (called from the autograd backward) ------------------------------
    def accumulate_grad(self, plan: ops.DedupPlan, srcs, B: int, short_segments: bool = False, members=None, bag=None):
        """srcs: [(d_out view [B, K*E], K)] in slot order of `plan`.  members: the embedders whose rows `plan` covers (None: the
        whole store) -- sparse mode files the gradient under them (file_sparse_grad).  bag: the ops.BagPlan of a pooled lookup --
        `plan` then covers its positions (M = nnz) and the reduction is ops.embed_bag_grad; filing and the dense views are the same."""
        if bag is not None:
            reduce = lambda mode, out: ops.embed_bag_grad(plan, bag, srcs, B, self.E, mode, out)
        if self.grad_mode == "sparse":
            grad_rows = torch.empty((max(plan.M, 1), self.E), dtype=torch.float32, device=self.device)
            if bag is not None:
                reduce(ops.TT_GRAD_SPARSE, grad_rows)
            else:
                ops.embed_grad(plan, srcs, B, self.E, ops.TT_GRAD_SPARSE, grad_rows, short_segments, self.grad_counters(),
                               defer_finish=self.defer_long_finish)
            self.file_sparse_grad(plan, grad_rows, members)
            return
        params = self.optim_parameters()
        fresh = any(p.grad is None for p in params) or self.grad is None
        if self.grad is None:
            self.grad = torch.empty_like(self.weight)
        if fresh:
            self.grad.zero_()                            # reference semantics: dense [V_k, E] grads
            if bag is not None:
                reduce(ops.TT_GRAD_DENSE_SET, self.grad)
            else:
                ops.embed_grad(plan, srcs, B, self.E, ops.TT_GRAD_DENSE_SET, self.grad, counters=self.grad_counters())
            self.bind_grads()
        elif bag is not None:
            reduce(ops.TT_GRAD_DENSE_ACC, self.grad)
        else:
            ops.embed_grad(plan, srcs, B, self.E, ops.TT_GRAD_DENSE_ACC, self.grad, counters=self.grad_counters())


class _Table(nn.Module):
    """Holds the per-key Parameter (a view into the fused store); name parity with nn.Embedding."""

    def __init__(self, view: torch.Tensor):
        super().__init__()
        self.weight = nn.Parameter(view)

    @property
    def num_embeddings(self):
        return self.weight.shape[0]

    @property
    def embedding_dim(self):
        return self.weight.shape[1]


class CategoricalEmbedder(nn.Module):
    def __init__(self, keys: List[str], metadata_path: Union[str, Path], table_name: str, embedding_dim: int = 64,
                 device: Optional[str] = "cuda:0", safety_margin: int = 10, embedding_grad: Optional[str] = None,
                 materialize: bool = True, pooling=None):
        super().__init__()
        self.keys = list(keys)
        self.pooling = self._pooling_modes(pooling, self.keys)     # None: every bag has length one (lengths are not read)
        if self.pooling is not None and not (embedding_dim % 4 == 0 and 4 <= embedding_dim <= 256):
            raise ValueError(f"bag mode (pooling=...) needs embedding_dim to be a multiple of 4 in [4, 256], got {embedding_dim}: the "
                             "pooled lookup moves rows in 16-byte pieces and has no scalar form")
        self.materialize = materialize
        self.embedding_dim = embedding_dim
        self.device_str = str(device or "cuda:0")
        self.safety_margin = safety_margin
        self.vocab_sizes = self._extract_vocab_sizes(metadata_path, table_name, self.keys)
        print(f"[CategoricalEmbedder] Initializing with {len(self.keys)} features")
        mode = embedding_grad or settings.embedding_grad
        self.store = EmbeddingStore(embedding_dim, torch.device(self.device_str), mode)
        self.embeddings = nn.ModuleDict()
        offs = []
        if materialize:
            self.row_base = self.store.append_rows(sum(self.vocab_sizes[k] for k in self.keys)) if self.keys else 0
            self.store.members.append(self)
            off = self.row_base
            for k in self.keys:
                v = self.vocab_sizes[k]
                self.embeddings[k] = _Table(self.store.weight[off:off + v])
                offs.append(off)
                off += v
        else:       # rows live in a sharded store owned by the distributed task; only the key directory is kept
            self.row_base, off = 0, 0
            for k in self.keys:
                offs.append(off)
                off += self.vocab_sizes[k]
        dev = self.store.device
        self.register_buffer("_key_row_offset", torch.tensor(offs, dtype=torch.int64, device=dev), persistent=False)
        self.register_buffer("_key_vocab", torch.tensor([self.vocab_sizes[k] for k in self.keys], dtype=torch.int64,
                                                        device=dev), persistent=False)
        if self.pooling is not None:
            self.register_buffer("_key_pool", torch.tensor([ops.POOL_MODES[m] for m in self.pooling], dtype=torch.int32, device=dev),
                                 persistent=False)
        self._bound_version = self.store.version
        self.position_weights: Optional[Dict[str, int]] = None     # {key: max_len} once add_position_weights has run

    def add_position_weights(self, position_weights: Dict[str, int]) -> "CategoricalEmbedder":
        """Learned position weights (torchrec's PositionWeightedModule): position j of a bag of `key` weighs
        position_weight[offset(key) + min(j, max_len - 1)], one f32 nn.Parameter over all the keys named here, initialised to 1.0 --
        at initialisation the pooled lookup is the unweighted one, bit for bit.  Positions at or beyond max_len SHARE the key's last
        weight (torchrec would index out of range there).  The parameter is an ordinary non-table parameter: named
        `position_weight`, in state_dict, trained by the towers' optimiser group.  A key left out weighs 1 at every position.
        Part of building the embedder -- BaseTower(categorical_position_weights=...) calls it: ValueError without pooling, for keys this
        embedder does not have (in bag mode every key of the embedder is pooled: no other key can be), for max_len < 1, and when
        called twice."""
        if not isinstance(position_weights, dict) or not position_weights:
            raise ValueError(f"position_weights must be a non-empty {{key: max_len}} dict, got {position_weights!r}")
        if self.pooling is None:
            raise ValueError("position_weights need bag mode: this embedder was built without pooling=..., so none of its keys is "
                             f"pooled (got position weights for {sorted(position_weights)})")
        if self.position_weights is not None:
            raise ValueError("this embedder already has position weights")
        unknown = [k for k in position_weights if k not in self.keys]
        if unknown:
            raise ValueError(f"position_weights names keys this embedder does not have: {unknown}")
        bad = {k: n for k, n in position_weights.items() if isinstance(n, bool) or not isinstance(n, int) or n < 1}
        if bad:
            raise ValueError(f"position_weights: max_len must be an integer >= 1, got {bad}")
        offs, lens, total = [], [], 0
        for k in self.keys:
            n = position_weights.get(k)
            offs.append(-1 if n is None else total)
            lens.append(0 if n is None else n)
            total += n or 0
        dev = self.store.device
        self.position_weights = {k: position_weights[k] for k in self.keys if k in position_weights}
        self.position_weight = nn.Parameter(torch.ones(total, dtype=torch.float32, device=dev))
        self.register_buffer("_pw_offset", torch.tensor(offs, dtype=torch.int32, device=dev), persistent=False)
        self.register_buffer("_pw_len", torch.tensor(lens, dtype=torch.int32, device=dev), persistent=False)
        return self

    def bag_weights(self, kjt) -> Optional[torch.Tensor]:
        """(bag mode) the per-id weights the pooled lookup takes for `kjt`: the KJT's own, or with position weights the parameter
        expanded over the bags' positions (differentiable: _PosWeightFn) -- never both: one source of weights per embedder.  On a
        captured step's static id buffers (the KJT carries bag_count) the parameter is not expanded: the answer is an
        ops.BagPosWeights source, which the towers' pooled lookup reads by position itself (towers.run_towers)."""
        weights = kjt_weights(kjt)
        if self.position_weights is None:
            return weights
        if weights is not None:
            raise ValueError("this embedder learns position weights (position_weights=...), and the KJT carries per-id weights of its "
                             "own: one source of weights per embedder -- hand the ids over without weights")
        if getattr(kjt, "bag_count", None) is not None:
            return ops.BagPosWeights(self.position_weight, self._pw_offset, self._pw_len)
        return _PosWeightFn.apply(self, kjt.lengths(), int(kjt.values().numel()), self.position_weight)

    @staticmethod
    def _pooling_modes(pooling, keys):
        """pooling: None | "sum" | "mean" | {key: "sum" | "mean"} (keys the dict leaves out sum) -> per-key modes, or None"""
        if pooling is None:
            return None
        if isinstance(pooling, str):
            modes = [pooling] * len(keys)
        elif isinstance(pooling, dict):
            unknown = [k for k in pooling if k not in keys]
            if unknown:
                raise ValueError(f"pooling names keys this embedder does not have: {unknown}")
            modes = [pooling.get(k, "sum") for k in keys]
        else:
            raise TypeError(f"pooling must be None, 'sum', 'mean' or a dict of them, got {type(pooling).__name__}")
        bad = [m for m in modes if m not in ops.POOL_MODES]
        if bad:
            raise ValueError(f"pooling modes must be 'sum' or 'mean', got {bad[0]!r}")
        return modes

    @property
    def bag_mode(self) -> bool:
        return self.pooling is not None

    def bag_side(self, values: torch.Tensor, lengths: torch.Tensor, out_view: torch.Tensor, count: Optional[torch.Tensor] = None,
                 weights: Optional[torch.Tensor] = None, pos_weights: Optional[ops.BagPosWeights] = None) -> ops.BagSide:
        """count: the device word of a captured step's static id buffer -- `values` is then that buffer, its size the capacity.
        weights: the KJT's weights (one f32 per id, in the order of `values`), or None: every id weighs 1.  pos_weights: the
        position-weight source in their place (bag_weights on a static KJT)"""
        return ops.BagSide(values, lengths, self._key_row_offset, self._key_vocab, self._key_pool, out_view, len(self.keys),
                           any(m == "mean" for m in self.pooling), None if count is None else values.numel(), count, weights, pos_weights)

    # ---- vocab sizes: src/towers/cat_embed.py:50-85 -------------------------------------------
    def _extract_vocab_sizes(self, metadata_path, table_name: str, keys: List[str]) -> Dict[str, int]:
        try:
            counts = category_counts(table_name, metadata_path)
        except Exception as e:                                            # whole-file failure: :82-85
            print(f"[ERROR] Failed to extract vocab_sizes from metadata: {e}")
            print("[FALLBACK] Using default vocab_size=1000 for all keys")
            return {k: 1000 for k in keys}
        out = {}
        for k in keys:
            if k not in counts:
                print(f"[WARNING] Column '{k}' not found in metadata, using default vocab_size=1000")
                out[k] = 1000
            elif counts[k] is None:
                print(f"[WARNING] No category count info for '{k}', using default vocab_size=1000")
                out[k] = 1000
            else:
                out[k] = int(counts[k]) + self.safety_margin
        return out

    # ---- store plumbing -------------------------------------------------------------------------
    def table_parameters(self):
        return [self.embeddings[k].weight for k in self.keys] if self.materialize else []

    @property
    def total_rows(self) -> int:
        return sum(self.vocab_sizes[k] for k in self.keys)

    def set_row_base(self, base: int):
        """(non-materialised embedders) place this embedder's keys at `base` of a global row space."""
        off, offs = base, []
        for k in self.keys:
            offs.append(off)
            off += self.vocab_sizes[k]
        self.row_base = base
        self._key_row_offset = torch.tensor(offs, dtype=torch.int64, device=self._key_row_offset.device)

    def _rebind(self, store: Optional[EmbeddingStore] = None, row_base: Optional[int] = None):
        if store is not None and store is not self.store:
            self.store = store
            if self not in store.members:
                store.members.append(self)
        if row_base is not None:
            self.row_base = row_base
        off = self.row_base
        offs = []
        for k in self.keys:
            v = self.vocab_sizes[k]
            self.embeddings[k].weight.data = self.store.weight[off:off + v]
            self.embeddings[k].weight.grad = None
            offs.append(off)
            off += v
        dev = self.store.device
        self._key_row_offset = torch.tensor(offs, dtype=torch.int64, device=dev)
        self._key_vocab = self._key_vocab.to(dev)
        self._move_key_pool(dev)
        self._bound_version = self.store.version
        if self.store.grad is not None:
            self._bind_grads()

    def _bind_grads(self):
        off = self.row_base
        for k in self.keys:
            v = self.vocab_sizes[k]
            self.embeddings[k].weight.grad = self.store.grad[off:off + v]
            off += v

    def _apply(self, fn, recurse=True):
        if not self.materialize:
            dev = fn(torch.empty(0, device=self._key_vocab.device)).device
            self._key_row_offset, self._key_vocab = self._key_row_offset.to(dev), self._key_vocab.to(dev)
            self._move_key_pool(dev)
            self._move_position_weights(fn, dev)
            self.store.device = dev
            return self
        # move the fused storage ONCE, then re-point the per-key views (keeps Parameter identity, so
        # optimisers built before .to(device) stay valid)
        self.store.apply(fn)
        for s_member in self.store.members:
            if s_member._bound_version != s_member.store.version:
                s_member._rebind()
        self._key_row_offset = self._key_row_offset.to(self.store.device)
        self._key_vocab = self._key_vocab.to(self.store.device)
        self._move_key_pool(self.store.device)
        self._move_position_weights(fn, self.store.device)
        return self

    def _move_position_weights(self, fn, dev):
        """the position-weight parameter is no view of the store: it moves like any module parameter (identity kept)"""
        if getattr(self, "position_weights", None) is not None:
            p = self.position_weight
            if fn(p.data).dtype != torch.float32:
                raise TypeError("position weights are kept in float32")
            p.data = fn(p.data)
            if p.grad is not None:
                p.grad.data = fn(p.grad.data)
            self._pw_offset, self._pw_len = self._pw_offset.to(dev), self._pw_len.to(dev)

    def _move_key_pool(self, dev):
        """(bag mode) the per-key pooling modes are part of the key directory: they move with it"""
        if self.pooling is not None:
            self._key_pool = self._key_pool.to(dev)

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        return super().load_state_dict(state_dict, strict=strict, assign=False)   # copy through the views

    # ---- forward: src/towers/cat_embed.py:126-190 ------------------------------------------------
    def lookup_side(self, values: torch.Tensor, out_view: torch.Tensor) -> ops.LookupSide:
        return ops.LookupSide(values, self._key_row_offset, self._key_vocab, out_view, len(self.keys))

    @_no_dynamo
    def forward(self, kjt, return_dict: bool = True):
        K, E = len(self.keys), self.embedding_dim
        if kjt is None:                                                    # :143-150
            dev = self.store.device
            if return_dict:
                return {k: torch.zeros(1, E, device=dev) for k in self.keys}
            return torch.zeros(1, K * E, device=dev)
        values = kjt.values()
        weights = self.bag_weights(kjt) if self.bag_mode else kjt_weights(kjt)
        if isinstance(weights, ops.BagPosWeights):
            raise ValueError("position weights on a captured step's static id buffers run through the towers (GraphedTrainStep("
                             "learned_weights=True)), not through a stand-alone embedder call")
        if self.bag_mode and weights_need_grad(weights):      # a tensor input of the node: its backward returns their gradient
            cat = _LookupFn.apply(self, (values, kjt.lengths(), _WEIGHTS_FIRST), weights, *self.table_parameters())
        elif self.bag_mode:
            cat = _LookupFn.apply(self, (values, kjt.lengths(), weights), *self.table_parameters())
        else:
            refuse_weights(weights, "CategoricalEmbedder")
            cat = _LookupFn.apply(self, values, *self.table_parameters())
        if not return_dict:
            return cat
        return {k: cat[:, i * E:(i + 1) * E] for i, k in enumerate(self.keys)}


class _LookupFn(torch.autograd.Function):
    """Stand-alone differentiable lookup (used when the embedder is called outside a tower)."""

    @staticmethod
    def forward(ctx, emb: CategoricalEmbedder, values, *tables):
        K, E = len(emb.keys), emb.embedding_dim
        ctx.bag = None
        ctx.w_grad = False
        if emb.bag_mode:                                                  # (values, lengths[, weights]): pooled bags
            values, lengths, weights = values if len(values) == 3 else (*values, None)
            if weights is _WEIGHTS_FIRST:                                 # differentiable weights: the first tensor input
                weights, tables, ctx.w_grad = tables[0], tables[1:], True
                ctx.w_shape, ctx.w_dtype, ctx.w_device = weights.shape, weights.dtype, weights.device
            dev = emb.store.device
            values = values.to(device=dev, dtype=torch.int64).contiguous()
            lengths = lengths.to(device=dev, dtype=torch.int64).contiguous()
            if weights is not None:
                weights = weights.detach().to(device=dev, dtype=torch.float32).contiguous()      # data: no gradient flows to them
            B = lengths.numel() // max(K, 1)
            out = torch.empty((B, K * E), dtype=torch.float32, device=dev)
            need_grad = any(ctx.needs_input_grad)
            ctx.emb, ctx.B, ctx.plan = emb, B, None
            if K and B:
                bag = ops.embed_bag_lookup(emb.store.weight, [emb.bag_side(values, lengths[:B * K], out, weights=weights)], B, want_rows=need_grad)
                if bag is not None and bag.nnz:
                    ctx.bag, ctx.plan = bag, ops.dedup_plan(bag.rows, emb.store.rows)
            return out
        values = values.to(device=emb.store.device, dtype=torch.int64).contiguous()
        B = values.numel() // max(K, 1)                                   # :98
        out = torch.empty((B, K * E), dtype=torch.float32, device=emb.store.device)
        need_grad = any(ctx.needs_input_grad)
        rows = ops.embed_lookup(emb.store.weight, [emb.lookup_side(values[:B * K], out)], B, want_rows=need_grad) \
            if K and B else None
        ctx.emb, ctx.B = emb, B
        ctx.plan = ops.dedup_plan(rows, emb.store.rows) if rows is not None else None
        return out

    @staticmethod
    def backward(ctx, d_out):
        emb = ctx.emb
        g_w = ()
        if ctx.plan is not None:
            d_out = d_out.contiguous()
            emb.store.accumulate_grad(ctx.plan, [(d_out, len(emb.keys))], ctx.B, members=[emb], bag=ctx.bag)
        if ctx.w_grad:
            g = None
            if ctx.bag is not None and ctx.needs_input_grad[2]:           # from the d_out the table gradient read
                g = ops.bag_weight_grad(emb.store.weight, ctx.bag, [(d_out, len(emb.keys))], ctx.B, [True])[0]
                g = g.reshape(ctx.w_shape).to(device=ctx.w_device, dtype=ctx.w_dtype)
            g_w = (g,)
        return (None, None) + g_w + (None,) * len(emb.keys)


class _PosWeightFn(torch.autograd.Function):
    """The position-weight parameter expanded over a KJT's bags (tt_bag_position_weights_fwd), and the sum of the per-id gradient
    back into it (tt_bag_position_weights_bwd)."""

    @staticmethod
    def forward(ctx, emb: CategoricalEmbedder, lengths, nnz: int, param):
        K = len(emb.keys)
        dev = param.device
        lengths = lengths.to(device=dev, dtype=torch.int64).contiguous()
        B = lengths.numel() // max(K, 1)
        ctx.side = ops.PosWeightSide(lengths[:B * K], emb._pw_offset, emb._pw_len, nnz, K)
        ctx.B = B
        ctx.save_for_backward(param)
        if not (K and B):
            return torch.ones(nnz, dtype=torch.float32, device=dev)
        return ops.bag_position_weights(param.detach(), [ctx.side], B)[0]

    @staticmethod
    def backward(ctx, g):
        (param,) = ctx.saved_tensors
        if not (ctx.side.K and ctx.B):
            return None, None, None, torch.zeros_like(param)
        g = g.to(dtype=torch.float32).contiguous()
        return None, None, None, ops.bag_position_weights_bwd(param.detach(), [ctx.side], ctx.B, [g])


_WEIGHTS_FIRST = object()      # _LookupFn: in the place of the weights -- "they are the first tensor input"


def weights_need_grad(weights) -> bool:
    """Per-id weights somebody wants a gradient for (a leaf that requires grad, or the expanded position weights) while autograd
    records; any other weights are data, handed over exactly as before."""
    return weights is not None and weights.requires_grad and torch.is_grad_enabled()


def position_weighted_embedders(module) -> List[str]:
    """Names of the embedders under `module` that learn position weights"""
    if not isinstance(module, nn.Module):
        return []
    return [n or "embedder" for n, m in module.named_modules() if isinstance(m, CategoricalEmbedder) and m.position_weights is not None]


def refuse_learned_weights(module, who: str, kjts=(), learned: bool = False) -> None:
    """The captured steps call this before they capture anything: ValueError when an embedder under `module` learns position weights
    or one of the example KJTs carries weights that require grad -- the gradient for per-id weights runs in the eager step only.
    learned: the caller captures position weights (GraphedTrainStep(learned_weights=True)): those pass, and a model without any is
    refused; weights that require grad stay refused."""
    names = position_weighted_embedders(module)
    if learned and not names:
        raise ValueError(f"{who}(learned_weights=True): no embedder of the model learns position weights (categorical_position_weights "
                         "/ add_position_weights)")
    if names and not learned:
        raise ValueError(f"{who} does not support learned position weights (categorical_position_weights / add_position_weights) yet: "
                         f"{', '.join(names)} would need the per-id weight gradient inside the captured step -- run such a model "
                         "through the eager step")
    for kjt in kjts:
        w = kjt_weights(kjt) if kjt is not None else None
        if w is not None and w.requires_grad:
            raise ValueError(f"{who} does not support per-id weights that require grad yet: the captured step forms no gradient for "
                             "them -- detach them, or run the eager step")


def kjt_weights(kjt) -> Optional[torch.Tensor]:
    """The per-id weights a KJT carries (ours or torchrec's: both answer weights_or_none()), or None"""
    get = getattr(kjt, "weights_or_none", None)
    return get() if get is not None else None


def refuse_weights(weights, who: str) -> None:
    """Weights mean something to a pooled lookup alone: an embedder that is not in bag mode raises instead of dropping them."""
    if weights is not None:
        raise ValueError(f"{who}: the KJT carries per-id weights, but this embedder is not in bag mode (pooling=None reads one id per "
                         "key and no weights) -- build it with pooling='sum' / 'mean', or hand the ids over without weights")


def bag_mode_embedders(module) -> List[str]:
    """Names of the embedders under `module` that pool ragged bags (empty: none, or `module` is no nn.Module)"""
    if not isinstance(module, nn.Module):
        return []
    return [n or "embedder" for n, m in module.named_modules() if isinstance(m, CategoricalEmbedder) and m.bag_mode]


def refuse_bag_mode(module: nn.Module, who: str) -> None:
    """The paths that keep a step's ids in static B*K buffers (captured, unrolled, segmented and sharded steps, the store-fed
    hand-over) call this: ValueError when an embedder under `module` pools ragged bags."""
    names = bag_mode_embedders(module)
    if names:
        raise ValueError(f"{who} does not support bag mode (categorical_pooling / CategoricalEmbedder(pooling=...)): its static id "
                         f"buffers hold exactly B*K ids, and {', '.join(names)} pool{'s' if len(names) == 1 else ''} bags of any "
                         "length -- run such a model through the eager step")


def create_categorical_embedder(keys: List[str], metadata_path="meta/metadata.csv", table_name: str = "notice",
                                embedding_dim: int = 64, device: Optional[str] = "cuda:0") -> CategoricalEmbedder:
    return CategoricalEmbedder(keys=keys, metadata_path=metadata_path, table_name=table_name,
                               embedding_dim=embedding_dim, device=device)
