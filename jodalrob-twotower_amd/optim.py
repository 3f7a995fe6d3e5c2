"""FusedAdam -- torch.optim.Adam semantics (scripts/train.py:231: lr, betas=(0.9,0.999), eps=1e-8,
coupled weight_decay) on the HIP path, usable wherever the reference builds `optim.Adam(
train_task.parameters(), ...)` (works with LambdaLR warm-up: lr is read from param_groups each step).

  * tower weights            : one tt_adam_multi_step launch per 32 tensors (exact dense Adam)
  * embedding tables, dense  : ONE tt_adam_dense_step over the fused [R, E] store (exact: identical to
    grad mode                  per-key Adam since the update is elementwise)
  * embedding tables, sparse : tt_sparse_adam_step over the rows looked up in this step only.  Rows that
    grad mode                  were not looked up keep weight / exp_avg / exp_avg_sq untouched (the
                               reference's dense Adam would decay their moments and apply weight decay);
                               bias correction uses the global step.  See DESIGN.md "optimiser semantics".

State layout matches torch.optim.Adam ('step', 'exp_avg', 'exp_avg_sq' per parameter; for table
parameters these are views into store-level buffers), so optimizer.state_dict() round-trips through
the reference's checkpoint format (scripts/train.py:506-511).

Row-wise Adagrad for the tables (FBGEMM's EXACT_ROWWISE_ADAGRAD; for_task(table_optimizer="rowwise_adagrad")):
the table parameters sit in a parameter group of their own carrying table_optimizer="rowwise_adagrad", and
their state is {'step', 'sum'} -- 'sum' a [num_embeddings] view into one store-level [R] f32 accumulator, so
the optimiser state is R floats instead of Adam's 2 x R x E.  Per looked-up row:
    g' = g + weight_decay * w;   sum += mean_j(g'_j^2);   w -= lr / (sqrt(sum) + eps) * g'
  * sparse grad mode : tt_rowwise_adagrad_sparse_step over the step's rows (exactly the dense update when
                       weight_decay = 0: a row with no gradient does not move)
  * dense grad mode  : tt_rowwise_adagrad_dense_step over all R rows
  * tower Adam + the looked-up rows: one tt_adam_rowwise_adagrad_fused_step launch
"""
from __future__ import annotations

from typing import Dict, List

import torch

from . import ops
from .cat_embed import EmbeddingStore


TABLE_OPTIMIZERS = ("adam", "rowwise_adagrad")


def _kind(group) -> str:
    return group.get("table_optimizer", "adam")


class FusedAdam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, stores: List[EmbeddingStore] = ()):
        if lr < 0 or eps < 0 or weight_decay < 0 or not (0 <= betas[0] < 1) or not (0 <= betas[1] < 1):
            raise ValueError("invalid Adam hyper-parameters")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self._stores: List[EmbeddingStore] = list(stores)
        self._store_state: Dict[int, dict] = {}
        self._hp_dev = None             # [n_groups, 8] device floats while a captured graph owns the step
        self._step_cache = None         # current_step() as of the last eager change (peek_step)

    @classmethod
    def for_task(cls, task, table_optimizer: str = "adam", table_lr=None, table_eps: float = 1e-8, table_weight_decay=None, **kw):
        """Collect the embedding stores of a TwoTowerTrainTask / TwoTowerModel / tower automatically.

        table_optimizer="rowwise_adagrad": the tables go in a parameter group of their own (table_optimizer="rowwise_adagrad",
        lr=table_lr, eps=table_eps, weight_decay=table_weight_decay; None inherits the towers' value), updated by row-wise
        Adagrad; the towers keep Adam.  A scheduler such as LambdaLR scales both groups' lr."""
        if table_optimizer not in TABLE_OPTIMIZERS:
            raise ValueError(f"table_optimizer must be one of {TABLE_OPTIMIZERS}, got {table_optimizer!r}")
        stores = find_stores(task)
        if table_optimizer == "adam":
            if table_lr is not None or table_weight_decay is not None:
                raise ValueError("table_lr / table_weight_decay apply to table_optimizer='rowwise_adagrad' only")
            return cls(task.parameters(), stores=stores, **kw)
        table_ids = {id(p) for s in stores for p in s.optim_parameters()}
        params = list(task.parameters())
        towers = [p for p in params if id(p) not in table_ids]
        tables = [p for p in params if id(p) in table_ids]
        if not tables:
            raise ValueError("table_optimizer='rowwise_adagrad': the task has no embedding tables")
        lr = kw.get("lr", 1e-3)
        table_group = {"params": tables, "table_optimizer": "rowwise_adagrad", "lr": lr if table_lr is None else table_lr,
                       "eps": table_eps, "weight_decay": kw.get("weight_decay", 0.0) if table_weight_decay is None else table_weight_decay}
        groups = ([{"params": towers}] if towers else []) + [table_group]
        return cls(groups, stores=stores, **kw)

    def add_param_group(self, param_group):
        kind = param_group.get("table_optimizer", "adam")
        if kind not in TABLE_OPTIMIZERS:
            raise ValueError(f"table_optimizer must be one of {TABLE_OPTIMIZERS}, got {kind!r}")
        if kind == "rowwise_adagrad":
            lr, eps, wd = (param_group.get(k, self.defaults[k]) for k in ("lr", "eps", "weight_decay"))
            if not (lr >= 0 and eps > 0 and wd >= 0):
                raise ValueError(f"invalid row-wise Adagrad hyper-parameters (lr={lr}, eps={eps}, weight_decay={wd}): "
                                 "lr >= 0, eps > 0, weight_decay >= 0")
        super().add_param_group(param_group)

    # ---- store-level state --------------------------------------------------------------------------
    def _group_of_store(self, store: EmbeddingStore):
        members = store.optim_parameters()
        if members:
            for group in self.param_groups:
                if any(members[0] is p for p in group["params"]):
                    return group
        return None

    def _state_of(self, store: EmbeddingStore) -> dict:
        group = self._group_of_store(store)
        if group is not None and _kind(group) == "rowwise_adagrad":
            return self._rowwise_state_of(store)
        st = self._store_state.get(id(store))
        if st is None or "m" not in st or st["m"].shape != store.weight.shape or st["m"].device != store.weight.device:
            st = {"m": torch.zeros_like(store.weight), "v": torch.zeros_like(store.weight), "step": 0}
            self._store_state[id(store)] = st
            shard = getattr(store, "shard_param", None)
            if shard is not None:                            # sharded store: one parameter = the local rows
                self.state[shard] = {"step": torch.tensor(0.0), "exp_avg": st["m"], "exp_avg_sq": st["v"]}
            for emb in ([] if shard is not None else store.members):   # per-parameter views, torch.optim.Adam layout
                off = emb.row_base
                for k in emb.keys:
                    n = emb.vocab_sizes[k]
                    p = emb.embeddings[k].weight
                    self.state[p] = {"step": torch.tensor(0.0), "exp_avg": st["m"][off:off + n],
                                     "exp_avg_sq": st["v"][off:off + n]}
                    off += n
        return st

    def _rowwise_state_of(self, store: EmbeddingStore) -> dict:
        st = self._store_state.get(id(store))
        if st is None or "sum" not in st or st["sum"].shape[0] != store.weight.shape[0] or st["sum"].device != store.weight.device:
            st = {"sum": torch.zeros(store.weight.shape[0], dtype=torch.float32, device=store.weight.device), "step": 0}
            self._store_state[id(store)] = st
            shard = getattr(store, "shard_param", None)
            if shard is not None:                            # sharded store: one parameter = the local rows, one [local_rows] buffer
                self.state[shard] = {"step": torch.tensor(0.0), "sum": st["sum"]}
            for emb in ([] if shard is not None else store.members):   # per-parameter [num_embeddings] views
                off = emb.row_base
                for k in emb.keys:
                    n = emb.vocab_sizes[k]
                    self.state[emb.embeddings[k].weight] = {"step": torch.tensor(0.0), "sum": st["sum"][off:off + n]}
                    off += n
        return st

    def _table_param_ids(self):
        return {id(p) for s in self._stores for p in s.optim_parameters()}

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._flush_pending()
        self._step_cache = None
        table_ids = self._table_param_ids()
        group_of = {}
        for group in self.param_groups:
            for p in group["params"]:
                group_of[id(p)] = group
        # ---- tower weights ----
        for gi, group in enumerate(self.param_groups):
            b1, b2 = group["betas"]
            hp = None if self._hp_dev is None else self._hp_dev[gi]
            items = []
            step_no = None
            for p in group["params"]:
                if id(p) in table_ids or p.grad is None:
                    continue
                if _kind(group) != "adam":
                    raise ValueError("a table_optimizer='rowwise_adagrad' parameter group holds embedding-table parameters only")
                st = self.state[p]
                if not st:
                    st["step"] = torch.tensor(0.0)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["step"] += 1
                step_no = int(st["step"].item())
                g = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
                items.append((p, g, st["exp_avg"], st["exp_avg_sq"], step_no))
            by_step: Dict[int, list] = {}
            for it in items:
                by_step.setdefault(it[4], []).append(it[:4])
            for s_no, its in by_step.items():
                fuse = self._fusable_store(group, s_no, len(its), len(by_step))
                if fuse is None:
                    ops.adam_multi(its, s_no, group["lr"], b1, b2, group["eps"], group["weight_decay"], hp)
                    continue
                store, st, tgroup = fuse          # tower weights + the looked-up rows of that store: one launch
                plan, grad_rows = store.sparse_grad
                st["step"] += 1
                if _kind(tgroup) == "rowwise_adagrad":   # (another group's table, its own hyper-parameters)
                    thp = None if self._hp_dev is None else self._hp_dev[self.param_groups.index(tgroup)]
                    ops.adam_rowwise_adagrad_fused(its, s_no, group["lr"], b1, b2, group["eps"], group["weight_decay"], hp,
                                                   store.weight, st["sum"], plan, grad_rows, tgroup["lr"], tgroup["eps"],
                                                   tgroup["weight_decay"], thp)
                else:
                    ops.adam_fused(its, store.weight, st["m"], st["v"], plan, grad_rows, s_no, group["lr"], b1, b2,
                                   group["eps"], group["weight_decay"], hp)
                store.sparse_grad = None
                self._write_step(store, st)
        # ---- embedding stores ----
        for store in self._stores:
            members = store.optim_parameters()
            if not members:
                continue
            group = group_of.get(id(members[0]))
            if group is None:
                continue                                     # tables not handed to this optimiser
            b1, b2 = group["betas"]
            hp = None if self._hp_dev is None else self._hp_dev[self.param_groups.index(group)]
            st = self._state_of(store)
            sparse, rowwise = store.grad_mode == "sparse", _kind(group) == "rowwise_adagrad"
            if sparse:
                entries = store.sparse_grads()               # (empty also once a fused launch above has applied the one entry)
                pending = bool(entries)
            else:
                pending = store.grad is not None and all(p.grad is not None for p in members)
            if not pending:
                continue
            st["step"] += 1
            lr, eps, wd = group["lr"], group["eps"], group["weight_decay"]
            if sparse:
                # several entries (one per side of a pass with unequal batch sizes, one per autograd node): disjoint rows, each
                # applied at the SAME step number -- one step of the store
                for plan, grad_rows in entries:
                    if rowwise:
                        ops.rowwise_adagrad_sparse(store.weight, st["sum"], plan, grad_rows, lr, eps, wd, hp)
                    else:
                        ops.adam_sparse(store.weight, st["m"], st["v"], plan, grad_rows, st["step"], lr, b1, b2, eps, wd, hp)
                store.sparse_grad = None
            elif rowwise:
                ops.rowwise_adagrad_dense(store.weight, st["sum"], store.grad, lr, eps, wd, hp)
            else:
                ops.adam_dense(store.weight, store.grad, st["m"], st["v"], st["step"], lr, b1, b2, eps, wd, hp)
            self._write_step(store, st)
        return loss

    def _write_step(self, store, st):
        for p in store.optim_parameters():
            self.state[p]["step"] = torch.tensor(float(st["step"]))

    def _fusable_store(self, group, s_no: int, n_items: int, n_buckets: int):
        """(store, state, the store's group) of the one store whose pending sparse gradient can ride in the launch that steps
        `group`'s tower tensors to s_no: `group`'s own Adam store when its next step is s_no, or, when `group` has no store, the
        one row-wise Adagrad store of another group; else None."""
        if n_buckets != 1 or not (1 <= n_items <= 32) or _kind(group) != "adam":
            return None
        own = [s for s in self._stores if self._group_of_store(s) is group]
        if own:
            cands = [(s, group) for s in own]
        else:
            cands = [(s, g) for s in self._stores for g in [self._group_of_store(s)] if g is not None and _kind(g) == "rowwise_adagrad"]
        if len(cands) != 1:
            return None
        store, tgroup = cands[0]
        pending = store.sparse_grads() if store.grad_mode == "sparse" else []
        if len(pending) != 1 or pending[0][0].M < 1:          # (several pending entries: the per-store branch applies each)
            return None
        st = self._state_of(store)
        return (store, st, tgroup) if tgroup is not group or st["step"] + 1 == s_no else None

    def advance_steps(self, n: int):
        """Account for `n` optimiser steps executed by graph replays (step counters live on the host;
        folded into the per-parameter state lazily)."""
        self._pending_steps = getattr(self, "_pending_steps", 0) + n

    def _flush_pending(self):
        n = getattr(self, "_pending_steps", 0)
        if n:
            self._pending_steps = 0
            if self._step_cache is not None:
                self._step_cache += n
            for st in self._store_state.values():
                st["step"] += n
            for st in self.state.values():
                if "step" in st:
                    st["step"] = st["step"] + float(n)

    def current_step(self) -> int:
        self._flush_pending()
        steps = [int(float(st["step"])) for st in self.state.values() if "step" in st]
        return max(steps) if steps else 0

    def peek_step(self) -> int:
        """Number of optimiser steps taken so far -- eager step() calls AND graph replays accounted through advance_steps() --
        without walking the per-parameter state on every call: a captured step asks for it at every hand-over (its bias
        corrections must follow the optimiser's own count when eager steps and replays interleave: GraphedTrainStep._fill_slot)."""
        if self._step_cache is None:
            self._step_cache = self.current_step()                 # (flushes the pending replays into the state)
        return self._step_cache + getattr(self, "_pending_steps", 0)

    def state_dict(self):
        self._flush_pending()
        return super().state_dict()

    def zero_grad(self, set_to_none: bool = True):
        super().zero_grad(set_to_none=set_to_none)
        for store in self._stores:
            store.sparse_grad = None

    def _check_table_state(self, state_dict):
        """Refuses a state whose table optimiser differs from this one's (an Adam state into a row-wise group, or the reverse)."""
        saved = state_dict.get("param_groups", [])
        if len(saved) != len(self.param_groups):
            kinds, skinds = {_kind(g) for g in self.param_groups}, {g.get("table_optimizer", "adam") for g in saved}
            if kinds != skinds:
                raise ValueError(f"load_state_dict: the state was saved with table_optimizer {sorted(skinds)}, this optimiser uses "
                                 f"{sorted(kinds)}")
            return                                                   # torch's own check reports it
        table_ids = self._table_param_ids()
        for group, sg in zip(self.param_groups, saved):
            kind, skind = _kind(group), sg.get("table_optimizer", "adam")
            if kind != skind:
                raise ValueError(f"load_state_dict: the state was saved with table_optimizer={skind!r}, this optimiser's group uses "
                                 f"{kind!r}")
            for p, idx in zip(group["params"], sg["params"]):
                s = state_dict["state"].get(idx)
                if id(p) not in table_ids or not s:
                    continue
                if (kind == "rowwise_adagrad" and "exp_avg" in s) or (kind == "adam" and "sum" in s):
                    raise ValueError(f"load_state_dict: a table parameter's saved state {sorted(s)} does not belong to "
                                     f"table_optimizer={kind!r}")

    def _load_rowwise(self, store):
        """After torch's load: copy the loaded per-parameter 'sum' into fresh store-level buffers (the kernels update those)."""
        shard = getattr(store, "shard_param", None)
        params = [shard] if shard is not None else [emb.embeddings[k].weight for emb in store.members for k in emb.keys]
        loaded = {id(p): dict(self.state[p]) for p in params if p in self.state and "sum" in self.state[p]}
        self._store_state.pop(id(store), None)
        if not loaded:
            return
        st = self._rowwise_state_of(store)
        for p in params:
            old = loaded.get(id(p))
            if old is not None:
                self.state[p]["sum"].copy_(old["sum"].to(self.state[p]["sum"].device))
                st["step"] = max(st["step"], int(float(old["step"])))
        for p in params:
            self.state[p]["step"] = torch.tensor(float(st["step"]))

    def load_state_dict(self, state_dict):
        self._check_table_state(state_dict)
        super().load_state_dict(state_dict)
        self._step_cache = None
        # re-point the table parameters' moments at store-level buffers (the kernels update those; self.state holds views)
        for store in self._stores:
            group = self._group_of_store(store)
            if group is not None and _kind(group) == "rowwise_adagrad":
                self._load_rowwise(store)
                continue
            shard = getattr(store, "shard_param", None)
            if shard is not None:
                # row-wise sharded store: ONE parameter = this rank's rows, its moments are the store-level buffers themselves
                old = dict(self.state[shard]) if shard in self.state and "exp_avg" in self.state[shard] else None
                self._store_state.pop(id(store), None)
                if old is None:
                    continue
                st = self._state_of(store)                     # fresh zero buffers, aliased into self.state[shard]
                st["m"].copy_(old["exp_avg"].to(st["m"].device))
                st["v"].copy_(old["exp_avg_sq"].to(st["v"].device))
                st["step"] = int(float(old["step"]))
                self.state[shard]["step"] = torch.tensor(float(st["step"]))
                continue
            loaded = {}
            for emb in store.members:
                for k in emb.keys:
                    p = emb.embeddings[k].weight
                    if p in self.state and "exp_avg" in self.state[p]:
                        loaded[id(p)] = dict(self.state[p])
            self._store_state.pop(id(store), None)
            if not loaded:
                continue
            st = self._state_of(store)
            for emb in store.members:
                for k in emb.keys:
                    p = emb.embeddings[k].weight
                    old = loaded.get(id(p))
                    if old is not None:
                        self.state[p]["exp_avg"].copy_(old["exp_avg"])
                        self.state[p]["exp_avg_sq"].copy_(old["exp_avg_sq"])
                        st["step"] = max(st["step"], int(float(old["step"])))
                        self.state[p]["step"] = torch.tensor(float(st["step"]))


def find_stores(module) -> List[EmbeddingStore]:
    from .cat_embed import CategoricalEmbedder
    out = []
    for m in module.modules():
        if hasattr(m, "embedding_stores"):
            out += [s for s in m.embedding_stores() if all(s is not o for o in out)]
        if isinstance(m, CategoricalEmbedder) and m.materialize and all(m.store is not s for s in out):
            out.append(m.store)
    return out
