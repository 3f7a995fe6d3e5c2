"""GraphedTrainStep: the whole training step (forward + backward + FusedAdam) captured ONCE into a HIP
graph and replayed per batch -- the MI355X counterpart of the reference's optional
torch.compile(train_task, mode="reduce-overhead") (scripts/train.py:223-225, off by default there).

Why: at batch 8192 the step is ~75 short kernels (0.9 ms of GPU time); launched one by one from Python the
host needs ~1.5 ms, so the GPU idles 40 % of the time.  A replay costs one launch.

What makes the capture replayable with NEW data every step:
  * the batch is copied into static input buffers before the replay -- one launch (`ops.batch_ingest`) that also leaves the
    fused table rows of the batch's ids in key-major order for the duplicate-row plan (the plan's own strided load of one
    key's rows is 6.5 of a sort workgroup's 18 us);
  * Adam's per-step scalars (lr from the scheduler, the bias corrections) and the dropout seed live in
    device memory (`hparams_dev` / `seed_dev` arguments of the C ABI) and are refreshed by one small
    pinned-memory copy before each replay;
  * every buffer the step allocates comes from the graph's private pool, so addresses are stable.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch

from . import _lib as L
from . import batch_terms as T
from . import ops
from .cat_embed import bag_mode_embedders, kjt_weights, refuse_bag_mode, refuse_learned_weights
from .config import settings
from .data_loader import DeviceBagFeatureStore
from .kjt import KeyedJaggedTensor
from .optim import FusedAdam


_MAX_COPIES = 8                    # copy segments per tt_copy_multi launch (include/twotower.h: TT_MAX_COPIES)
_STEP = "the captured step"        # whose device the array checks name
_CELLS, _NEGATIVES = T.ROWS["masked_cells"], T.ROWS["negatives"]


def resolve_bag_capacity(bag_capacity, nnz: Dict[str, int]) -> Dict[str, int]:
    """The capacity in ids of every bag-mode side's static id buffer.  bag_capacity: an int (every side), a {side: int} dict, or
    "auto" (four times the example batch's ids, at least 1024, as cell_capacity); nnz: {side: ids of the example batch} of the
    bag-mode sides.  ValueError for anything else, for a side the dict leaves out and for a capacity below the example's ids."""
    out = {}
    for side, n in nnz.items():
        if isinstance(bag_capacity, str):
            if bag_capacity != "auto":
                raise ValueError(f"bag_capacity must be an int, a dict of ints per side or 'auto', got {bag_capacity!r}")
            cap = max(4 * n, 1024)
        elif isinstance(bag_capacity, dict):
            unknown = [k for k in bag_capacity if k not in nnz]
            if unknown:
                raise ValueError(f"bag_capacity names sides that are not in bag mode: {unknown} (bag mode: {list(nnz)})")
            if side not in bag_capacity:
                raise ValueError(f"bag_capacity gives no capacity for the bag-mode side '{side}'")
            cap = bag_capacity[side]
        else:
            cap = bag_capacity
        if isinstance(cap, bool) or not isinstance(cap, int):
            raise ValueError(f"bag_capacity must be an int, a dict of ints per side or 'auto', got {cap!r} for '{side}'")
        if cap < max(n, 1):
            raise ValueError(f"bag_capacity = {cap} for '{side}': the example batch carries {n} ids there (and at least 1)")
        out[side] = cap
    return out


def _holders(static, row):
    """the dicts of the static buffers that hold `row`'s arrays under its key: one per side, or the top level"""
    return [static[side] for side in T.SIDES] if row.where == "side" else [static]


class GraphedTrainStep:
    _steps_per_replay = 1          # (unrolled.UnrolledTrainStep: several steps, hand-overs included, per graph launch)
    _bag_capture = True            # bag_capacity is honoured (the unrolled / segmented steps keep refusing bag mode)
    _bag: Dict[str, int] = {}      # {side: capacity} of the bag-mode sides (none: a plain model)
    _bag_w: frozenset = frozenset()   # the bag-mode sides captured WITH per-id weights (the example KJT carried them)
    _bag_pw: frozenset = frozenset()  # the bag-mode sides whose embedder learns position weights (learned_weights=True)
    _accepts = frozenset(T.ROWS)   # the batch entries that change the loss (batch_terms.TABLE) an example batch may carry; the
                                   # unrolled / segmented steps take none

    def __init__(self, task, optimizer: FusedAdam, example_batch: Dict, return_metrics: bool = True, warmup: int = 3,
                 defer_long: bool = True, defer_slabs: bool = True, defer_riders: bool = True, preserve_state: bool = True,
                 accumulate_metrics: bool = False, metric_sums: Optional[torch.Tensor] = None, fuse_score_tail: bool = True,
                 cell_capacity: Optional[int] = None, bag_capacity=None, learned_weights: bool = False):
        """defer_long / defer_slabs: the long rows' finish rides in the optimiser's launch and the towers' slab reduction in the
        embedding gradient's (both bit-identical to the separate launches; the arguments exist for that comparison).
        fuse_score_tail: the score backward waits for the towers' backward, which launches it with its own first kernel's work in
        the epilogue (one launch fewer where the shapes allow it, bit-identical; independent of defer_riders; not for a sharded task).
        preserve_state: the eager warm-up steps (allocator + first-call paths) are REAL steps on the example batch; with this flag
        everything they change -- weights, Adam moments and step counts, BatchNorm running statistics -- is put back before the
        capture, so a captured loop starts from the state an eager loop starts from (row-sparse tables: only the example batch's
        rows move and only those are saved; dense-gradient tables are saved whole).
        accumulate_metrics: `metric_sums` (device, 8 floats: loss, accuracy, positive mean, negative mean, gap, ...: twotower.h
        tt_score_loss_finish) += the step's figures inside the replay -- an epoch's mean loss / accuracy (the reference driver's
        avg_train_loss: scripts/train.py:357-358) without a host sync per step.  metric_sums: add into THIS tensor (another captured
        step's sums: the two then share one epoch total; what it holds survives this object's warm-up).
        cell_capacity: rows of the static masked-cells buffer of a step captured on a batch with "masked_cells" (default: four times
        the example's, at least 1024); a later batch with more cells is refused.
        bag_capacity: None -- a bag-mode model (categorical_pooling) is refused; an int, a {"notice": n, "company": n} dict or "auto"
        (four times the example batch's ids, at least 1024) -- the capacity in ids of every bag-mode side's static id buffer: the
        captured step then runs the pooled lookup's capacity form, a later batch with more ids is refused.
        learned_weights: False -- a model whose embedders learn position weights (categorical_position_weights) is refused; True (with
        bag_capacity) -- it is captured: the pooled lookup reads the parameter by position, the backward forms its gradient over the
        capacity and FusedAdam steps it inside the graph.  Per-id data weights on such a side, weights that
        require grad, and the unrolled / segmented / sharded steps stay refused."""
        # the example batch's entries that change the loss (batch_terms.TABLE): each gets static buffers -- [B] per side (a side the
        # batch does not carry: zeros / its row indices) or one [B]; the extras' M rows with whichever of log_q / entity they carry; an
        # int32 [capacity, 2] buffer of cells and a device count, one more word of the step's scalars -- filled at every hand-over by more
        # copy segments of its launch(es); the captured forward reads the buffers, and the launches that prepare them (the weights', the
        # cells' plan: their grids depend on the capacity alone) are nodes of the graph.  With extras the hand-over is the plain-copy one
        self._terms = T.present(example_batch)
        for row in T.TABLE:
            if row.key not in self._terms:
                continue
            if row.key not in self._accepts:
                raise NotImplementedError(f"{row.phrase} {row.verb} not supported by {type(self).__name__}")
            if getattr(task, "exchange", None) is not None:
                raise NotImplementedError(f"{row.phrase} {row.verb} not supported by the sharded task")
        if cell_capacity is not None and _CELLS.key not in self._terms:
            raise ValueError("cell_capacity: the example batch carries no 'masked_cells'")
        if not isinstance(optimizer, FusedAdam):
            raise TypeError("GraphedTrainStep needs jodalrob_twotower_amd.optim.FusedAdam (device-side hyper-parameters)")
        # learned position weights need the per-id weight gradient, which the captured step runs on request alone
        # (learned_weights=True); per-id weights that require grad it never does: refused before anything is built or captured
        who = type(self).__name__
        if learned_weights:
            if not self._bag_capture or getattr(task, "exchange", None) is not None:
                raise ValueError(f"{who}(learned_weights=True): learned position weights are captured by GraphedTrainStep on an unsharded "
                                 "task alone -- the unrolled, segmented and sharded steps refuse them; run the eager step")
            if bag_capacity is None:
                raise ValueError(f"{who}(learned_weights=True) needs bag_capacity: position weights belong to pooled keys, and a captured "
                                 "bag-mode step runs on static id buffers of a fixed capacity")
        refuse_learned_weights(task, who, [example_batch[side].get("kjt") for side in T.SIDES if side in example_batch],
                               learned=bool(learned_weights))
        # the static id buffers hold B*K ids: no ragged bags in a captured step -- refused here, once, so that step() and
        # step_from_store() of a bag-mode model cannot be reached (and pay no check per step)
        self._bag = self._bag_sides(task, example_batch, bag_capacity, bool(learned_weights))    # {side: capacity} of the bag-mode sides
        self.bag_capacity = dict(self._bag) or None
        self.task, self.opt, self.return_metrics = task, optimizer, return_metrics
        self._defer_long, self._defer_slabs, self._defer_riders = bool(defer_long), bool(defer_slabs), bool(defer_riders)
        self._fuse_score_tail = bool(fuse_score_tail)
        dev = example_batch["notice"]["dense"].device
        self.static = {side: {"dense": example_batch[side]["dense"].clone(), "kjt": self._static_kjt(example_batch[side]["kjt"], side, dev)}
                       for side in ("notice", "company")}
        B, self._fill = example_batch["notice"]["dense"].shape[0], {}
        for row in T.B_TERMS:
            if row.key not in self._terms:
                continue
            if row.missing:
                self._fill[row.key] = row.fill(B, dev)
            given = row.of(example_batch)
            for holder, name, t in zip(_holders(self.static, row), row.names(_STEP), given if row.where == "side" else (given,)):
                holder[row.key] = (self._fill[row.key] if t is None else T.check(t, name, row.dtype, (B,), dev, _STEP).contiguous()).clone()
        if _NEGATIVES.key in self._terms:
            neg = example_batch["negatives"]
            self.static["negatives"] = {"dense": neg["dense"].clone(), "kjt": KeyedJaggedTensor(neg["kjt"].keys(), neg["kjt"].values().clone())}
            for k in ("log_q", "entity"):
                if neg.get(k) is not None:
                    self.static["negatives"][k] = neg[k].clone()
        ng = len(optimizer.param_groups)
        # per-step scalars (Adam step sizes, dropout seed, the masked cells' count) travel through a RING of pinned host slots: the copy
        # kernel reads the slot when it executes, and the host may be many steps ahead of the GPU by then
        self._bag_word = ng * 8 + 2 + (2 if _CELLS.key in self._terms else 0)     # a bag-mode side's id count: one word each
        self._n_scalar = self._bag_word + len(self._bag)
        self._slot_len = (self._n_scalar + 3) // 4 * 4                 # 16-byte slots
        self._ring = 64
        self._host_ring = torch.zeros(self._ring, self._slot_len, dtype=torch.float32).pin_memory()
        self._slot_events = [None] * self._ring
        self._slot = 0
        self._unmarked = []                                            # ring slots filled since the last _mark_slot
        self._host = self._host_ring[0, :self._n_scalar]
        self._dev = torch.zeros(self._n_scalar, dtype=torch.float32, device=dev)
        self._hp_dev = self._dev[:ng * 8].view(ng, 8)
        self._seed_dev = self._dev[ng * 8:ng * 8 + 2].view(torch.int64)          # 2 floats = one 64-bit word
        if _CELLS.key in self._terms:
            ex = self._check_cells(example_batch["masked_cells"], dev, None)
            cap = max(4 * ex.shape[0], 1024) if cell_capacity is None else int(cell_capacity)
            if cap < max(ex.shape[0], 1):
                raise ValueError(f"cell_capacity = {cap}: the example batch carries {ex.shape[0]} cells (and at least 1)")
            self.cell_capacity, self._cells_n = cap, ex.shape[0]
            self.static["masked_cells"] = torch.zeros((cap, 2), dtype=torch.int32, device=dev)
            self.static["masked_cells"][:ex.shape[0]] = ex
            self.static["masked_cells_count"] = self._dev[ng * 8 + 2:ng * 8 + 3].view(torch.int32)      # (the scalars' copy fills it)
        for i, side in enumerate(self._bag):       # the count word rides with the step's scalars; the warm-up reads the example's
            word = self._dev[self._bag_word + i:self._bag_word + i + 1].view(torch.int32)
            word.fill_(self._bag_n[side])
            self.static[side]["kjt"].bag_count = word
        self._ones = torch.ones((), dtype=torch.float32, device=dev)
        self._towers = [m for m in task.modules() if hasattr(m, "_seed_dev") and hasattr(m, "dense_parameters")]
        self.metric_sums = torch.zeros(8, dtype=torch.float32, device=dev) if (accumulate_metrics and return_metrics) else None
        sums_before = None
        if metric_sums is not None and self.metric_sums is not None:
            self.metric_sums, sums_before = metric_sums, metric_sums.clone()
        self._ingest = self._setup_ingest()
        self._shadows = self._setup_shadows()
        if self._ingest is not None:
            self._run_ingest([], None)                           # rows_km of the example batch: warm-up and capture see it
        # eager warm-up on a side stream (allocator + first-call paths), then capture
        snap = self._snapshot_state() if (preserve_state and warmup > 0) else None
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(warmup):
                self._eager_once()
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        if snap is not None:
            self._restore_state(snap)
        if self.metric_sums is not None:
            self.metric_sums.zero_() if sums_before is None else self.metric_sums.copy_(sums_before)
        if self._ingest is not None:
            self._run_ingest([], None)
        self._push_scalars()
        for t in self._towers:
            t._seed_dev = self._seed_dev
        optimizer._hp_dev = self._hp_dev
        self.graph = None
        # With a process group alive, its watchdog thread polls events while we capture; under the default "global" capture
        # mode that poll is an error ("operation not permitted when stream is capturing") that aborts the process --
        # now and then, depending on timing.  "thread_local" restricts the check to the capturing thread.
        import torch.distributed as _dist
        mode = "thread_local" if (_dist.is_available() and _dist.is_initialized()) else "global"
        n0 = L.load().tt_launch_count()
        try:
            self._capture(mode)
        finally:
            self.library_launches = int(L.load().tt_launch_count() - n0) + 1       # (+ the hand-over launch in front of every replay)
            optimizer._hp_dev = None
            for t in self._towers:
                t._seed_dev = None
        # the capture itself ran the host-side bookkeeping of one optimiser step (per captured body) without executing it
        optimizer.advance_steps(-self._steps_per_replay)

    def _bag_sides(self, task, example_batch, bag_capacity, learned_weights: bool = False) -> Dict[str, int]:
        """{side: capacity} of the sides whose embedder pools bags, after the refusals (no device work)"""
        self._bag_n, self._bag_w, self._bag_pw = {}, frozenset(), frozenset()
        if not bag_mode_embedders(task):
            if bag_capacity is not None:
                raise ValueError("bag_capacity: the model has no bag-mode embedder (categorical_pooling)")
            return {}
        # the static id buffers hold B*K ids: without a capacity no ragged bags in a captured step -- refused here, once, so that
        # step() and step_from_store() of such a model cannot be reached (and pay no check per step)
        if bag_capacity is None or not self._bag_capture:
            refuse_bag_mode(task, type(self).__name__)
        if _NEGATIVES.key in self._terms:          # (the company side would splice two padded id buffers)
            raise NotImplementedError(f"{_NEGATIVES.phrase} {_NEGATIVES.verb} not supported by a captured bag-mode step")
        model = getattr(task, "two_tower_model", None)
        sides = {side: example_batch[side]["kjt"].values().numel() for side, name in (("notice", "notice_tower"), ("company", "company_tower"))
                 if getattr(getattr(getattr(model, name, None), "categorical_embedder", None), "bag_mode", False)}
        if not sides or getattr(task, "exchange", None) is not None:
            refuse_bag_mode(task, type(self).__name__)
        self._bag_n = dict(sides)                  # ids the static buffer holds now (the count word of the next hand-over)
        self._bag_w = frozenset(side for side in sides if kjt_weights(example_batch[side]["kjt"]) is not None)
        if learned_weights:
            self._bag_pw = frozenset(side for side in sides
                                     if getattr(model, f"{side}_tower").categorical_embedder.position_weights is not None)
            for side in sorted(self._bag_pw & self._bag_w):
                raise ValueError(f"{side}: the example batch carries per-id weights, and the side's embedder learns position weights: "
                                 "one source of weights per embedder -- hand the ids over without weights")
        for side in self._bag_w:
            w, v = kjt_weights(example_batch[side]["kjt"]), example_batch[side]["kjt"].values()
            if w.numel() != v.numel():
                raise ValueError(f"{side}: the example batch carries {w.numel()} weights for {v.numel()} ids")
        return resolve_bag_capacity(bag_capacity, sides)

    def _static_kjt(self, kjt, side, dev):
        """the static KJT of a side: its ids; a bag-mode side: an id buffer of the capacity (the example's ids at its head) and the
        [B*K] lengths (its count word is attached once the scalars exist); a side captured with weights: also an f32 weight buffer of
        the capacity, zero-initialised, the example's weights at its head -- the towers then take the capacity form's weighted entry"""
        if side not in self._bag:
            return KeyedJaggedTensor(kjt.keys(), kjt.values().clone())
        v = kjt.values().to(device=dev, dtype=torch.int64).reshape(-1)
        buf = torch.zeros(self._bag[side], dtype=torch.int64, device=dev)
        buf[:v.numel()] = v
        wbuf = None
        if side in self._bag_w:
            wbuf = torch.zeros(self._bag[side], dtype=torch.float32, device=dev)
            wbuf[:v.numel()] = kjt_weights(kjt).to(device=dev, dtype=torch.float32).reshape(-1)
        return KeyedJaggedTensor(kjt.keys(), buf, kjt.lengths().to(device=dev, dtype=torch.int64).reshape(-1).clone(), wbuf)

    def _bag_check(self, batch):
        """a bag-mode side's ids fit the capacity, its lengths are B*K and it carries weights (one per id) exactly when the side was
        captured with them -- before anything is copied"""
        if batch is None:
            return
        for side, cap in self._bag.items():
            kjt, st = batch[side]["kjt"], self.static[side]["kjt"]
            if kjt.values().numel() > cap:
                raise ValueError(f"{side}: {kjt.values().numel()} ids, the step was captured with bag_capacity = {cap}")
            if kjt.lengths().numel() != st.lengths().numel():
                raise ValueError(f"{side}: {kjt.lengths().numel()} bag lengths, the captured step holds B*K = {st.lengths().numel()}")
            w = kjt_weights(kjt)
            if w is not None and side in self._bag_pw:
                raise ValueError(f"{side}: the batch carries per-id weights, and the side's embedder learns position weights: one source "
                                 "of weights per embedder -- hand the ids over without weights")
            if (w is not None) != (side in self._bag_w):
                raise ValueError(f"{side}: the batch carries {'per-id weights' if w is not None else 'no weights'}, the step was captured "
                                 f"{'with' if side in self._bag_w else 'without'} them (the example batch decides)")
            if w is not None and w.numel() != kjt.values().numel():
                raise ValueError(f"{side}: {w.numel()} weights for {kjt.values().numel()} ids")

    def _bag_pairs(self, side, kjt):
        """copy segments of a bag-mode side's ids (into the head of the static buffer), lengths and -- a side captured with them --
        weights (into the head of the static weight buffer, beside the ids); the count goes with the scalars"""
        st = self.static[side]["kjt"]
        v, ln = kjt.values().reshape(-1), kjt.lengths().reshape(-1)
        sv, sl = st.values(), st.lengths()
        n = v.numel()
        self._bag_n[side] = n
        out = []
        segs = [(sv[:n], v), (sl, ln)]
        if side in self._bag_w:
            segs.insert(1, (st.weights()[:n], kjt_weights(kjt).reshape(-1)))
        for dst, src in segs:
            if not dst.numel():
                continue
            if src.device == dst.device and src.dtype == dst.dtype:
                out += T.segment(dst, src)
            else:
                dst.copy_(src, non_blocking=True)
        return out

    def _capture(self, mode: str):
        """Captures self._body() into self.graph (ONE graph; segmented.SegmentedTrainStep cuts it at the collectives instead)."""
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph, capture_error_mode=mode):
            self.result = self._body()

    def _replay_graph(self):
        self.graph.replay()

    def _setup_ingest(self):
        """Key-major row hand-over (ops.batch_ingest) when the step looks the static ids up in ONE local fused table with the
        per-key plan: returns (store, embedders, rows_km, static id tensors, B) or None (then the batch is handed over by plain
        copies and the plan gathers its rows out of the lookup's slot-major array)."""
        self._x_static, self._rows_sm = None, None
        if not settings.graph_ingest or _NEGATIVES.key in self._terms or self._bag:     # (extras: the company side is B + M rows;
            return None                                                                  # bags: a side holds any number of ids)
        model = getattr(self.task, "two_tower_model", None)
        towers = [getattr(model, n, None) for n in ("notice_tower", "company_tower")]
        if model is None or any(t is None for t in towers):
            return None
        embs = [t.categorical_embedder for t in towers]
        ex = getattr(self.task, "exchange", None)
        if ex is not None:
            # row-wise sharded tables: the key-major rows are GLOBAL fused rows (the embedders' offsets span the global row space);
            # the fixed-capacity exchange sorts them in place of its rows-only lookup
            store = getattr(ex, "store", None)
            ids = [self.static[side]["kjt"].values() for side in ("notice", "company")]
            B = self.static["notice"]["dense"].shape[0]
            if store is None or not hasattr(ex, "poll_overflow") or not (0 < B <= ops.KEYED_MAX_B) or \
                    any(len(e.keys) == 0 or len(e.keys) > 64 or v.dtype != torch.int64 or not v.is_contiguous() for e, v in zip(embs, ids)):
                return None
            rows_km = torch.empty(sum(v.numel() for v in ids), dtype=torch.int32, device=ids[0].device)
            return store, embs, rows_km, ids, B
        store = embs[0].store
        ids = [self.static[side]["kjt"].values() for side in ("notice", "company")]
        B = self.static["notice"]["dense"].shape[0]
        if any(e.store is not store for e in embs) or store.weight is None or not (0 < B <= ops.KEYED_MAX_B):
            return None
        if any(len(e.keys) == 0 or len(e.keys) > 64 or v.dtype != torch.int64 or not v.is_contiguous() or v.numel() != B * len(e.keys)
               for e, v in zip(embs, ids)):
            return None
        rows_km = torch.empty(sum(v.numel() for v in ids), dtype=torch.int32, device=ids[0].device)
        # persistent tower inputs x = [projection | embedding rows]: the hand-over launch looks the batch's rows up straight into
        # their embedding columns (tt_batch_ingest_lookup), the captured forward finds them filled and has no lookup launch
        if settings.graph_ingest_lookup:
            xs = [torch.zeros((B, t.x_width), dtype=t.x_dtype, device=ids[0].device) for t in towers]
            outs = [ops.LookupSide(v, e._key_row_offset, e._key_vocab, x[:, t.tower_hidden_dims[0]:], len(e.keys))
                    for e, v, x, t in zip(embs, ids, xs, towers)]
            if ops.ingest_lookup_supported(store.weight, outs):
                self._x_static = xs
        # the same rows in slot order: the captured lookup reads them instead of decoding the ids again (tt_embed_lookup_rows_fwd)
        if self._x_static is None and settings.graph_ingest_rows and store.weight.shape[1] % 4 == 0:
            self._rows_sm = torch.empty_like(rows_km)
        return store, embs, rows_km, ids, B

    def _setup_shadows(self):
        """bf16 shadows of the towers' projection and block weights (bf16 towers): [(tower, w_proj16, [w16 per block])].  The hand-over
        launch converts the f32 weights into them at EVERY step (ops.batch_ingest(cvt=...)), so whoever updated the weights since
        the last hand-over -- the replayed Adam, an eager step, load_state_dict -- the replay reads current values; the towers see the
        shadows only while this object's step runs (_body)."""
        if not settings.graph_weight_shadows or self._ingest is None:
            return []
        out = []
        for t in self._towers:
            if getattr(t, "mlp_dtype", None) != "bf16" or t.n_hidden < 1:
                continue
            lins = [t.mlp[4 * i] for i in range(t.n_hidden)]
            ws = [t.dense_projection.weight] + [l.weight for l in lins]
            if any(w.dtype != torch.float32 or not w.is_contiguous() or w.numel() % 8 for w in ws):
                continue
            sh = [torch.empty(w.shape, dtype=torch.bfloat16, device=w.device) for w in ws]
            out.append((t, ws, sh))
        n = sum(len(ws) for _, ws, _ in out)
        return out if 0 < n <= L.TT_MAX_CVT else []

    def _cvt(self):
        return [(s_, w) for _, ws, sh in self._shadows for w, s_ in zip(ws, sh)]

    def _lookup_outs(self):
        towers = [self.task.two_tower_model.notice_tower, self.task.two_tower_model.company_tower]
        return [x[:, t.tower_hidden_dims[0]:] for x, t in zip(self._x_static, towers)]

    def _register(self, store, ids, rows_km):
        xs = getattr(self, "_x_static", None)
        store.ingest = (ids, [v._version for v in ids], rows_km, xs, getattr(self, "_rows_sm", None))
        store.ingest_x_fresh = xs is not None

    @staticmethod
    def _table_rows(store) -> int:
        """Size of the row space the hand-over's fused rows index: the fused table, or the GLOBAL row space of row-wise sharded tables."""
        g = getattr(store, "global_rows", None)
        return int(g) if g is not None else int(store.weight.shape[0])

    def _run_ingest(self, pairs, src_ids):
        """One launch: the copy segments + the key-major rows of `src_ids` (default: the static id buffers themselves) (+ the
        lookup of those rows into the persistent tower inputs)."""
        store, embs, rows_km, ids, B = self._ingest
        src = ids if src_ids is None else src_ids
        xs = getattr(self, "_x_static", None)
        if xs is not None:
            sides = [ops.LookupSide(v, e._key_row_offset, e._key_vocab, o, len(e.keys)) for e, v, o in zip(embs, src, self._lookup_outs())]
            ops.batch_ingest(pairs, sides, B, rows_km, table=store.weight, cvt=self._cvt())
        else:
            sides = [ops.LookupSide(v, e._key_row_offset, e._key_vocab, None, len(e.keys)) for e, v in zip(embs, src)]
            ops.batch_ingest(pairs, sides, B, rows_km, rows_sm=getattr(self, "_rows_sm", None), cvt=self._cvt(), table_rows=self._table_rows(store))
        self._register(store, ids, rows_km)

    def _body(self):
        self.opt.zero_grad(set_to_none=True)
        # backward and optimiser step are one unit here: the gradient reduction leaves its long rows to the optimiser's launch
        # (FusedAdam finishes them whichever of its paths it takes) -- one launch fewer in the dependent chain
        defer = self._defer_long
        stores = list(getattr(self.opt, "_stores", ()))
        for st in stores:
            st.defer_long_finish = defer
        # likewise the slab reduction of the towers' weight gradients rides in the embedding gradient's launch (the two do not
        # depend on each other); whatever is still queued after the backward is launched on its own
        dev = self._dev.device
        # (a sharded task's dense-gradient all-reduce comes BEHIND the exchange's backward, whose first launch hosts the queue, and
        # flushes whatever is still queued before it reads the gradients: towers.py)
        ex = getattr(self.task, "exchange", None)
        slabs = self._defer_slabs
        # the keyed plan's compaction and the score forward's loss reduction ride in the towers' tail launches (two launches fewer
        # in the chain).  A sharded task's exchange reads the plan at once: only the loss reduction rides there (and not under SyncBN,
        # whose tail kernels run in two phases with a collective between them)
        riders = self._defer_riders and self._ingest is not None and (ex is None or not getattr(self.task, "sync_bn", False))
        # the score backward waits in the context for the towers' backward (TT_OPT_FUSE_SCORE_TAIL): nothing but the library touches
        # d_emb between the two.  A sharded task scales d_emb by 1 / world in between and its score backward is rectangular: off
        fuse = self._fuse_score_tail and ex is None
        for t, _, sh in self._shadows:                 # the hand-over launch in front of this step has refreshed them
            t._w16 = (sh[0], sh[1:])
        try:
            if fuse:
                L.set_fuse_score_tail(dev, True)
            if riders:
                L.set_defer_riders(dev, True, loss_only=ex is not None)
            res = self.task(self.static, return_metrics=self.return_metrics)
            loss = res["loss"] if isinstance(res, dict) else res
            if slabs:
                L.set_defer_slab_reduce(dev, True)
            try:
                loss.backward(self._ones)              # preallocated seed gradient: no fill kernel per step
            finally:
                if slabs:
                    L.set_defer_slab_reduce(dev, False)      # (flushes)
            self.opt.step()
            for st in stores:                          # a store this optimiser did not step: nobody else will finish its gradient
                for plan, _ in st.sparse_grads():
                    ops.embed_grad_finish(plan)
            if self.metric_sums is not None:           # (behind the backward: a riding loss reduction has written out8 by now)
                self.metric_sums.add_(res.out8)
        finally:
            for t, _, _ in self._shadows:
                t._w16 = None
            if fuse:
                L.set_fuse_score_tail(dev, False)      # (launches a score backward nobody hosted: a backward that never reached the towers)
            if riders:
                L.set_defer_riders(dev, False)         # (launches what nobody hosted: e.g. the loss reduction of a forward-only pass)
            for st in stores:
                st.defer_long_finish = False
        return res

    def _eager_once(self):
        if self._ingest is not None:
            self._run_ingest([], None)          # (an optimiser step has changed the rows since the last hand-over filled x)
        self._body()

    # ---- warm-up without side effects ---------------------------------------------------------------------------------
    def _touched_rows(self, store):
        """Fused rows (sorted, distinct) the example batch looks up in `store`, or None when they cannot be told from here
        (row-wise sharded tables: the rows this rank updates come from every rank's batch)."""
        model = getattr(self.task, "two_tower_model", None)
        if model is None or getattr(self.task, "exchange", None) is not None:
            return None
        rows = []
        for name, side in (("notice_tower", "notice"), ("company_tower", "company")):
            tw = getattr(model, name, None)
            if tw is None:
                return None
            e = tw.categorical_embedder
            if e.store is not store or not e.keys:
                continue
            if side in self._bag:                  # the key of a position follows from the lengths (a synchronisation: construction only)
                kjt, K = self.static[side]["kjt"], len(e.keys)
                key = torch.repeat_interleave(torch.arange(kjt.lengths().numel(), device=kjt.lengths().device) % K, kjt.lengths())
                ids = kjt.values()[:self._bag_n[side]][:key.numel()]
                rows.append(ids.clamp(min=0).minimum(e._key_vocab[key] - 1) + e._key_row_offset[key])
                continue
            ids = self.static[side]["kjt"].values().view(-1, len(e.keys))
            if side == "company" and _NEGATIVES.key in self._terms:     # the extras go through the company tower too
                ids = torch.cat([ids, self.static["negatives"]["kjt"].values().view(-1, len(e.keys))], 0)
            rows.append((ids.clamp(min=0).minimum(e._key_vocab - 1) + e._key_row_offset).reshape(-1))      # cat_embed.py:114-117
        return torch.unique(torch.cat(rows)) if rows else None

    def _snapshot_state(self):
        opt = self.opt
        opt._flush_pending()
        table_ids = opt._table_param_ids()
        snap = {"buffers": [(b, b.detach().clone()) for b in self.task.buffers()], "dense": [], "stores": [], "steps": []}
        for group in opt.param_groups:
            for p in group["params"]:
                if id(p) in table_ids:
                    continue
                st = opt.state.get(p) or {}
                snap["dense"].append((p, p.detach().clone(), None if "exp_avg" not in st else
                                      (st["exp_avg"].clone(), st["exp_avg_sq"].clone(), st["step"].clone())))
        for store in getattr(opt, "_stores", ()):
            if store.weight is None or not store.optim_parameters():
                continue
            st = opt._state_of(store)
            keys = ("sum",) if "sum" in st else ("m", "v")                 # row-wise Adagrad: one [R] accumulator; Adam: two [R, E] moments
            rows = self._touched_rows(store) if store.grad_mode == "sparse" else None
            if rows is None and (store.weight.numel() + sum(st[k].numel() for k in keys)) * 4 > (8 << 30):
                rows = torch.empty(0, dtype=torch.int64, device=store.weight.device)     # too large to copy whole: left as the warm-up leaves it
            pick = (lambda t: t[rows].clone()) if rows is not None else (lambda t: t.clone())
            snap["stores"].append((store, rows, pick(store.weight), {k: pick(st[k]) for k in keys}, st["step"]))
        snap["steps"] = [(st, st["step"].clone()) for st in opt.state.values() if "step" in st]
        return snap

    @torch.no_grad()
    def _restore_state(self, snap):
        opt = self.opt
        opt._flush_pending()
        for b, saved in snap["buffers"]:
            b.copy_(saved)
        for p, w, st0 in snap["dense"]:
            p.copy_(w)
            st = opt.state.get(p)
            if st and "exp_avg" in st:
                if st0 is None:                        # the state came into being during the warm-up: back to Adam's initial state
                    st["exp_avg"].zero_(); st["exp_avg_sq"].zero_(); st["step"] = torch.tensor(0.0)
                else:
                    st["exp_avg"].copy_(st0[0]); st["exp_avg_sq"].copy_(st0[1]); st["step"] = st0[2].clone()
        for store, rows, w, saved, step in snap["stores"]:
            st = opt._state_of(store)
            if rows is None:
                store.weight.copy_(w)
                for k, t in saved.items():
                    st[k].copy_(t)
            elif rows.numel():
                store.weight[rows] = w
                for k, t in saved.items():
                    st[k][rows] = t
            st["step"] = step
        known = {id(st): val for st, val in snap["steps"]}
        for st in opt.state.values():
            if "step" in st:
                st["step"] = known[id(st)].clone() if id(st) in known else torch.tensor(0.0)
        opt._step_cache = None
        opt.zero_grad(set_to_none=True)

    def _fill_slot(self, ahead: int = 0):
        """Writes the scalars of the step `ahead` steps after the next one into the next ring slot; returns the (dst, src) copy pair."""
        self._slot = (self._slot + 1) % self._ring
        self._unmarked.append(self._slot)
        ev = self._slot_events[self._slot]
        if ev is not None:
            ev.synchronize()                                        # the copy that last read this slot has run
        host = self._host_ring[self._slot, :self._n_scalar]
        ng = len(self.opt.param_groups)
        # the optimiser's own count: eager steps taken between replays (a ragged last batch, another captured step sharing
        # the optimiser) advance the bias corrections exactly as they do in an all-eager loop
        step = self.opt.peek_step() + 1 + ahead
        for gi, g in enumerate(self.opt.param_groups):
            if g.get("table_optimizer", "adam") == "rowwise_adagrad":        # the row-wise Adagrad entries read [lr, eps, weight_decay]
                host[gi * 8: gi * 8 + 3] = torch.tensor([float(g["lr"]), g["eps"], g["weight_decay"]])
                continue
            hp = ops.adam_hparams(step, float(g["lr"]), g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"])
            host[gi * 8: gi * 8 + 6] = torch.tensor(hp)
        host[ng * 8:ng * 8 + 2].view(torch.int64).random_()
        if _CELLS.key in self._terms:
            host[ng * 8 + 2:ng * 8 + 4].view(torch.int32)[0] = self._cells_n
        for i, side in enumerate(self._bag):
            host[self._bag_word + i:self._bag_word + i + 1].view(torch.int32)[0] = self._bag_n[side]
        return (self._dev, host)

    def _mark_slot(self):
        """One event behind the launch(es) that read the slots filled since the last mark: a slot is refilled only after it."""
        slots, self._unmarked = self._unmarked, []
        if not slots:
            return
        ev = self._slot_events[slots[0]]
        if ev is None or len(slots) > 1:
            ev = torch.cuda.Event()
        ev.record()
        for sl in slots:
            self._slot_events[sl] = ev

    def _push_scalars(self):
        ops.copy_multi([self._fill_slot()])
        self._mark_slot()

    @staticmethod
    def _check_cells(t, dev, capacity):
        """t as a contiguous int32 [L, 2] on dev, L <= capacity (L is the tensor's shape: no synchronisation)"""
        T.check(t, _CELLS.key, _CELLS.dtype, _CELLS.shape, dev, _STEP)
        if capacity is not None and t.shape[0] > capacity:
            raise ValueError(f"masked_cells: {t.shape[0]} cells, the step was captured with cell_capacity = {capacity}")
        return t.contiguous()

    def _cells_check(self, batch):
        """this step's cells after the with / without and the capacity checks -- before anything is copied"""
        cells, captured = None if batch is None else batch.get(_CELLS.key), _CELLS.key in self._terms
        if batch is not None and (cells is not None) != captured:
            raise ValueError(T.mismatch(_CELLS, captured))
        return None if cells is None else self._check_cells(cells, self._dev.device, self.cell_capacity)

    def _cells_pairs(self, cells):
        """the copy segment of this step's cells into the head of the static buffer; their count goes with the step's scalars"""
        if cells is None:
            return []
        self._cells_n = n = cells.shape[0]
        return T.segment(self.static[_CELLS.key][:n], cells) if n else []

    def _term_pairs(self, key, value, who):
        """copy segments of this step's arrays of a [B] entry -- `value`: per side (notice, company) or the one array, a side given
        as None: what it stands for -- into the static buffers, after the with / without check; who hands it over: "the batch" or
        "step_from_store" (the mismatch sentence names it)"""
        row, captured = T.ROWS[key], key in self._terms
        if (value is not None) != captured:
            raise ValueError(T.mismatch(row, captured, who))
        out = []
        if value is not None:
            for holder, name, t in zip(_holders(self.static, row), row.names(_STEP), value if row.where == "side" else (value,)):
                dst = holder[key]
                out += T.segment(dst, self._fill[key] if t is None else T.check(t, name, row.dtype, dst.shape, dst.device, _STEP))
        return out

    def _negatives_pairs(self, neg):
        """copy segments of this step's extra negatives into the static M-row buffers, after the with / without check (the task
        validates what the buffers then hold)"""
        captured = _NEGATIVES.key in self._terms
        if (neg is not None) != captured:
            raise ValueError(T.mismatch(_NEGATIVES, captured))
        if neg is None:
            return []
        sn = self.static["negatives"]
        if {k for k in ("log_q", "entity") if neg.get(k) is not None} != {k for k in ("log_q", "entity") if k in sn}:
            raise ValueError("negatives mismatch: the batch's extras carry other optional entries (log_q / entity) than the captured ones")
        out = []
        for name, dst, src in [("dense", sn["dense"], neg["dense"]), ("kjt", sn["kjt"].values(), neg["kjt"].values())] + \
                [(k, sn[k], neg[k]) for k in ("log_q", "entity") if k in sn]:
            if not isinstance(src, torch.Tensor) or src.shape != dst.shape or src.dtype != dst.dtype or src.device != dst.device:
                raise ValueError(f"negatives['{name}'] must be a {dst.dtype} tensor of shape {list(dst.shape)} on {dst.device} "
                                 "(the captured step has one M)")
            out += T.segment(dst, src)
        return out

    def _handover_pairs(self, batch: Optional[Dict]):
        """(copy segments, per-side id sources) that hand `batch` over into the static buffers (None: nothing to copy)."""
        pairs, src_ids = [], []                                 # src_ids per side: where this step's ids are read from
        if batch is None:
            return pairs, None
        pairs += self._negatives_pairs(batch.get("negatives"))
        for row in T.B_TERMS:
            pairs += self._term_pairs(row.key, row.of(batch), "the batch")
        for side in ("notice", "company"):
            d, v = batch[side]["dense"], batch[side]["kjt"].values()
            sd, sv = self.static[side]["dense"], self.static[side]["kjt"].values()
            if side in self._bag:
                if d.device == sd.device and d.dtype == sd.dtype and d.is_contiguous():
                    pairs += [(sd, d)]
                else:
                    sd.copy_(d, non_blocking=True)
                pairs += self._bag_pairs(side, batch[side]["kjt"])
                src_ids.append(sv)
                continue
            if d.device == sd.device and d.dtype == sd.dtype and v.dtype == sv.dtype and d.is_contiguous() and v.is_contiguous():
                pairs += [(sd, d), (sv, v)]
                src_ids.append(v)
            else:                                               # host batch / other dtype: ordinary copies
                sd.copy_(d, non_blocking=True)
                sv.copy_(v, non_blocking=True)
                src_ids.append(sv)
        return pairs, src_ids

    def step(self, batch: Optional[Dict] = None):
        """Train on `batch` (or on whatever the static buffers hold); returns the static result."""
        cells = self._cells_check(batch)
        self._bag_check(batch)
        pairs, src_ids = self._handover_pairs(batch)
        pairs += self._cells_pairs(cells)
        if self._ingest is not None:
            # ONE launch: the four batch buffers + the scalars + the key-major rows of this step's ids -- also when nobody handed a
            # batch over: the static id buffers may have been written to by means no version counter sees (`.data`), and the
            # replayed plan sorts whatever rows_km holds
            self._run_ingest(pairs + [self._fill_slot()], src_ids)
            self._mark_slot()
        else:
            segs = pairs + [self._fill_slot()]                  # ONE launch: the four batch buffers + the scalars (extras with
            for i in range(0, len(segs), _MAX_COPIES):          # log_q and entity on every side: 13 segments, two launches)
                ops.copy_multi(segs[i:i + _MAX_COPIES])
            self._mark_slot()
        return self._replay()

    def _replay(self):
        self._replay_graph()
        self.opt.advance_steps(self._steps_per_replay)
        ex = getattr(self.task, "exchange", None)
        if ex is not None and hasattr(ex, "poll_overflow"):
            ex.poll_overflow()                                  # sharded tables: a bucket overflow rejects the step (non-blocking)
        return self.result

    def step_from_store(self, notice_store, company_store, pairs: torch.Tensor, order: Optional[torch.Tensor] = None, offset: int = 0,
                        log_q=None, entity=None, pair_weight=None, bag_ids=None):
        """Train on the B pairs `pairs[order[offset : offset + B]]` (order None: `pairs[offset : offset + B]`) gathered straight
        out of the device-resident feature stores into the static buffers -- ONE launch (tt_batch_ingest_store: dense rows, ids,
        key-major fused rows, the step scalars) and the replay; nothing per step crosses PCIe and no batch tensors are built
        (the reference assembles the batch on the host and copies it over: unified_bid_data_loader.py:461-504, :630-684;
        scripts/train.py:261-273).  `pairs`: int64 [P, 2] on the device, (notice row, company row) per pair; the stores are
        data_loader.DeviceFeatureStore objects (`.dense` f32 [N, D], `.categorical` int64 [N, K]).
        log_q: (notice, company) f32 [B] of this step's pairs for a step captured with a log_q (DevicePairLoader.step_batches passes
        slices of its per-epoch array): two more copy segments of the same launch.
        entity: (notice, company) int32 [B] ids of this step's pairs for a step captured with entity ids (the repeated-entity mask;
        DevicePairLoader(mask_repeats=True).step_batches passes slices of its per-epoch array): likewise.
        pair_weight: f32 [B] weights of this step's pairs for a step captured with pair weights: one more copy segment.
        A step captured with bag_capacity: every bag-mode side takes a data_loader.DeviceBagFeatureStore, and tt_bag_store_gather (two
        launches, which also carry the copy segments) fills the side's static dense buffer, its [B*K] lengths and the head of its static
        id buffer; a side that is not in bag mode keeps its DeviceFeatureStore and goes through tt_batch_ingest_store alone.
        A side captured with per-id weights takes a store that carries them (DeviceBagFeatureStore(... "categorical_weights")): the same
        two launches fill the head of its static weight buffer beside the ids.  A weighted step on a store without weights, and a
        weighted store on a side captured without them, are refused before anything is launched.
        bag_ids: {side: this batch's id count} of the bag-mode sides (DevicePairLoader.epoch_bag_ids) -- it goes into the count word
        with the step's scalars, as step(batch)'s; a count above the capacity is refused before anything is launched, one that is not
        the batch's raises the device error word and the captured step runs the side's bags as empty.  Without bag_ids the counts are
        summed from the stores' run_lengths and READ BACK from the device: correct, and a host synchronisation per step."""
        for row in (_CELLS, _NEGATIVES):
            if row.key in self._terms:
                raise NotImplementedError(f"{row.noun}: no store-fed hand-over -- a step captured with '{row.key}' takes step(batch)")
        stores = {"notice": notice_store, "company": company_store}
        for side in sorted(self._bag_w):      # (the weights come out of the store: its gather fills the static weight buffer)
            if not isinstance(stores[side], DeviceBagFeatureStore) or getattr(stores[side], "weights", None) is None:
                raise ValueError(f"step_from_store: the step was captured with per-id weights on {sorted(self._bag_w)}, and the {side} store "
                                 "carries none -- it takes a DeviceBagFeatureStore with categorical_weights, or step(batch)")
        for side in sorted(getattr(self, "_bag_pw", ())):
            if getattr(stores[side], "weights", None) is not None:
                raise ValueError(f"step_from_store: the {side} store carries per-id weights, and the side's embedder learns position weights: "
                                 "one source of weights per embedder -- it takes a plain DeviceBagFeatureStore")
        for side in self._bag:
            if side not in self._bag_w and getattr(stores[side], "weights", None) is not None:
                raise ValueError(f"step_from_store: the {side} store carries per-id weights, but the step was captured without them on that "
                                 "side (the example batch decides): they would be dropped silently")
        if any(not isinstance(stores[side], DeviceBagFeatureStore) for side in self._bag):      # (a DeviceFeatureStore holds one id per key)
            refuse_bag_mode(self.task, "step_from_store")
        for side, fs in stores.items():
            if isinstance(fs, DeviceBagFeatureStore) and side not in self._bag:
                raise ValueError(f"step_from_store: the {side} side is fed from a DeviceBagFeatureStore, but that side's embedder does not pool bags "
                                 "(categorical_pooling): its static id buffer holds exactly B*K ids")
        counts = self._bag_counts(stores, pairs, order, offset, bag_ids) if self._bag else None
        given, extra = {"log_q": log_q, "entity": entity, "pair_weight": pair_weight}, []
        for row in T.B_TERMS:
            extra += self._term_pairs(row.key, given[row.key], "step_from_store")
        if self._bag:
            self._ingest_from_bag_stores(stores, pairs, order, offset, counts, extra)
        else:
            self._ingest_from_store(notice_store, company_store, pairs, order, offset, extra=extra or None)
        self._mark_slot()
        return self._replay()

    def _store_pairs(self, pairs: torch.Tensor, order: Optional[torch.Tensor], offset: int):
        """(the flat pair list, the first element of this batch's first pair) after the checks every store-fed hand-over makes"""
        B = self.static["notice"]["dense"].shape[0]
        if pairs.dtype != torch.int64 or pairs.dim() != 2 or pairs.shape[1] != 2 or not pairs.is_contiguous():
            raise ValueError("step_from_store: pairs must be a contiguous int64 [P, 2] tensor")
        if order is None and (offset < 0 or offset + B > pairs.shape[0]):
            raise ValueError("step_from_store: the batch runs past the pair list")
        return pairs.view(-1), (0 if order is not None else 2 * offset)

    def _bag_counts(self, stores, pairs, order, offset, bag_ids) -> Dict[str, int]:
        """{side: ids of this batch} of the bag-mode sides, each within the side's capacity -- nothing is launched or changed before"""
        B = self.static["notice"]["dense"].shape[0]
        if bag_ids is None:
            self._store_pairs(pairs, order, offset)
            if order is not None and (offset < 0 or offset + B > order.numel()):
                raise ValueError("step_from_store: the batch runs past the order")
            sel = pairs[offset:offset + B] if order is None else pairs[order[offset:offset + B]]
            sums = torch.stack([stores[side].run_lengths[sel[:, 0 if side == "notice" else 1]].sum() for side in self._bag]).tolist()
            bag_ids = dict(zip(self._bag, sums))              # (the one device read of this form)
        if set(bag_ids) != set(self._bag):
            raise ValueError(f"step_from_store: bag_ids names {sorted(bag_ids)}, the step's bag-mode sides are {sorted(self._bag)}")
        counts = {side: int(bag_ids[side]) for side in self._bag}
        for side, n in counts.items():
            if n > self._bag[side]:
                raise ValueError(f"{side}: {n} ids, the step was captured with bag_capacity = {self._bag[side]}")
            if n < 0:
                raise ValueError(f"step_from_store: bag_ids['{side}'] = {n}")
        return counts

    def _ingest_from_bag_stores(self, stores, pairs, order, offset, counts, extra):
        """The hand-over launches of a bag-mode step_from_store: tt_batch_ingest_store for the sides that are not in bag mode (none:
        no launch), then tt_bag_store_gather for the bag-mode sides with the copy segments `extra` and the step's scalars."""
        B = self.static["notice"]["dense"].shape[0]
        flat, base = self._store_pairs(pairs, order, offset)
        model = self.task.two_tower_model
        embs = {"notice": model.notice_tower.categorical_embedder, "company": model.company_tower.categorical_embedder}
        bags, lookups, plains = [], [], []
        for i, side in enumerate(("notice", "company")):
            fs, e, sd, kjt = stores[side], embs[side], self.static[side]["dense"], self.static[side]["kjt"]
            if side in self._bag:
                if len(fs.keys) != len(e.keys):
                    raise ValueError(f"step_from_store: the {side} store holds {len(fs.keys)} keys, the embedder {len(e.keys)}")
                w = side in self._bag_w                      # (the static weight buffer beside the id buffer: the same capacity)
                bags.append(ops.BagStoreSide(flat[base + i:], 2, fs.dense, fs.offsets, fs.values, len(e.keys), sd, kjt.lengths(), kjt.values(),
                                             counts[side], fs.weights if w else None, kjt.weights() if w else None))
            else:
                lookups.append(ops.LookupSide(None, e._key_row_offset, e._key_vocab, None, len(e.keys)))
                plains.append(ops.StoreSide(flat[base + i:], 2, fs.dense, fs.categorical, sd, kjt.values()))
        off = offset if order is not None else 0
        if plains:
            ops.batch_ingest_store([], lookups, plains, B, order, None, off)
        self._bag_n.update(counts)                              # (the count word of this hand-over: _fill_slot reads it)
        ops.bag_store_gather(extra + [self._fill_slot()], bags, B, order, off)

    def _ingest_from_store(self, notice_store, company_store, pairs: torch.Tensor, order: Optional[torch.Tensor], offset: int, ahead: int = 0,
                           extra=None):
        """The hand-over launch of step_from_store (tt_batch_ingest_store) into the static buffers; `ahead`: _fill_slot; `extra`:
        more copy segments for the same launch."""
        B = self.static["notice"]["dense"].shape[0]
        flat, base = self._store_pairs(pairs, order, offset)
        model = self.task.two_tower_model
        embs = [model.notice_tower.categorical_embedder, model.company_tower.categorical_embedder]
        sides, stores = [], []
        xs = getattr(self, "_x_static", None) if self._ingest is not None else None
        outs = self._lookup_outs() if xs is not None else [None, None]
        for i, (side, fs, e) in enumerate(zip(("notice", "company"), (notice_store, company_store), embs)):
            sd, sv = self.static[side]["dense"], self.static[side]["kjt"].values()
            sides.append(ops.LookupSide(None, e._key_row_offset, e._key_vocab, outs[i], len(e.keys)))
            stores.append(ops.StoreSide(flat[base + i:], 2, fs.dense, fs.categorical, sd, sv))
        rows_km = self._ingest[2] if self._ingest is not None else None
        ops.batch_ingest_store((extra or []) + [self._fill_slot(ahead)], sides, stores, B, order, rows_km, offset if order is not None else 0,
                               table=self._ingest[0].weight if xs is not None else None,
                               rows_sm=getattr(self, "_rows_sm", None) if (self._ingest is not None and xs is None) else None,
                               cvt=self._cvt(), table_rows=self._table_rows(self._ingest[0]) if self._ingest is not None else 0)
        if self._ingest is not None:
            store, _, _, ids, _ = self._ingest
            self._register(store, ids, rows_km)

    def close(self):
        """Final (synchronous) overflow check, then drop the captured graph and its private pool.  With a process group
        alive this must happen BEFORE `destroy_process_group()`: the graph's nodes reference the communicator's buffers
        and streams, and tearing the communicator down first aborts inside RCCL."""
        dev = self._dev.device
        torch.cuda.synchronize(dev)
        ex = getattr(self.task, "exchange", None)
        try:
            L.check_device_errors(dev)                          # (a chained plan launch that gave up: the steps since the last check are invalid)
            if ex is not None and hasattr(ex, "check_overflow"):
                ex.check_overflow()
        finally:
            self.result = None
            if self._ingest is not None:
                self._ingest[0].ingest = None                   # the key-major rows belonged to this object's static buffers
                self._ingest = None
            if self.graph is not None:
                self.graph.reset()
                self.graph = None
            import gc
            gc.collect()
            torch.cuda.synchronize(dev)


class GraphedEvalStep:
    """The evaluation pass of one batch -- towers in eval mode, loss and metrics, the rank of every positive in its row, and from
    the ranks Recall@5 / Recall@10 / MRR (src/evaluation/evaluator.py:20-71, :123-155) -- captured once and replayed per batch,
    fed like GraphedTrainStep.step_from_store from the device-resident feature stores.  Per batch the eager evaluator costs ~30
    launches from Python and a dozen `.item()` round trips; here it is one hand-over launch, one replay and NO host sync: the
    eight per-batch figures are added into a device accumulator, read once at the end (`means()`).
    metrics order: loss, accuracy, similarity_gap, positive_similarity_mean, negative_similarity_mean, recall@5, recall@10, mrr."""

    KEYS = ("loss", "accuracy", "similarity_gap", "positive_similarity_mean", "negative_similarity_mean", "recall@5", "recall@10", "mrr")

    def __init__(self, task, example_batch: Dict, warmup: int = 2):
        refuse_bag_mode(task, type(self).__name__)
        self.task = task
        dev = example_batch["notice"]["dense"].device
        self.static = {side: {"dense": example_batch[side]["dense"].clone(),
                              "kjt": KeyedJaggedTensor(example_batch[side]["kjt"].keys(), example_batch[side]["kjt"].values().clone())}
                       for side in ("notice", "company")}
        self.B = self.static["notice"]["dense"].shape[0]
        self.acc = torch.zeros(8, dtype=torch.float32, device=dev)
        self.batches = 0
        was_training = task.training
        task.eval()
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side), torch.no_grad():
            for _ in range(warmup):
                self._body()
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        self.acc.zero_()
        self.graph = torch.cuda.CUDAGraph()
        import torch.distributed as _dist
        mode = "thread_local" if (_dist.is_available() and _dist.is_initialized()) else "global"
        with torch.no_grad(), torch.cuda.graph(self.graph, capture_error_mode=mode):
            self._body()
        task.train(was_training)

    def _body(self):
        res, ranks = self.task.forward_with_ranks(self.static)
        k5, k10 = min(5, self.B), min(10, self.B)
        r = ranks.float()
        per = torch.stack([res["loss"].reshape(()), res["accuracy"].reshape(()), res["similarity_gap"].reshape(()),
                           res["positive_similarity_mean"].reshape(()), res["negative_similarity_mean"].reshape(()),
                           (ranks < k5).float().mean(), (ranks < k10).float().mean(), (1.0 / (r + 1.0)).mean()])
        self.acc.add_(per)

    def reset(self):
        self.acc.zero_()
        self.batches = 0

    def step_from_store(self, notice_store, company_store, pairs: torch.Tensor, order: Optional[torch.Tensor] = None, offset: int = 0):
        flat = pairs.view(-1)
        base = 0 if order is not None else 2 * offset
        model = self.task.two_tower_model
        embs = [model.notice_tower.categorical_embedder, model.company_tower.categorical_embedder]
        sides, stores = [], []
        for i, (side, fs, e) in enumerate(zip(("notice", "company"), (notice_store, company_store), embs)):
            sides.append(ops.LookupSide(None, e._key_row_offset, e._key_vocab, None, len(e.keys)))
            stores.append(ops.StoreSide(flat[base + i:], 2, fs.dense, fs.categorical, self.static[side]["dense"], self.static[side]["kjt"].values()))
        ops.batch_ingest_store([], sides, stores, self.B, order, None, offset if order is not None else 0)
        self.graph.replay()
        self.batches += 1

    def add_eager(self, metrics: Dict):
        """A batch evaluated outside the graph (the ragged last one) joins the sums."""
        self.acc.add_(torch.tensor([float(metrics[k]) for k in self.KEYS], dtype=torch.float32, device=self.acc.device))
        self.batches += 1

    def means(self) -> Dict[str, float]:
        vals = (self.acc / max(self.batches, 1)).cpu().tolist()          # the one host sync of the evaluation
        return dict(zip(self.KEYS, vals))

    def close(self):
        torch.cuda.synchronize(self.acc.device)
        if self.graph is not None:
            self.graph.reset()
            self.graph = None
