"""Device-resident feature store + pair loader -- the MI355X replacement for UnifiedBidDataset.__getitem__
and create_collate_fn (src/towers/pairs/unified_bid_data_loader.py:461-504, :630-684): the reference keeps
`dense_projected` / `categorical` in host numpy arrays, gathers them per batch with fancy indexing on a
2-thread pool, wraps the ids in a KJT (:827-841) and copies the batch to the GPU (scripts/train.py:261-273)
-- the README names this loader as the training bottleneck (23 it/s at 40 % GPU utilisation).

Here both stores live in HBM and a batch is assembled by tt_batch_gather from the pair indices: the only
per-step host->device traffic is 16 bytes per pair.  Batches have the reference's format
{"notice": {"dense", "kjt"}, "company": {"dense", "kjt"}} with sample-major ids.
"""
from __future__ import annotations

from typing import Dict, Iterator, Optional, Tuple

import numpy as np
import torch

from . import ops
from .feature_preprocessor import FeaturePreprocessor
from .kjt import KeyedJaggedTensor
from .schema import TorchRecSchema


class DeviceFeatureStore:
    """dense_projected f32 [N, Din] and categorical i64 [N, K] of one tower, resident on the device."""

    def __init__(self, store: Dict, categorical_keys, device):
        self.device = torch.device(device)
        self.keys = list(categorical_keys)
        def resident(x, dtype):            # host arrays (the reference's stores: feature_store.py:76-79) or tensors already on a device
            t = x if torch.is_tensor(x) else torch.as_tensor(np.ascontiguousarray(x))
            return t.to(device=self.device, dtype=dtype).contiguous()
        self.dense = resident(store["dense_projected"], torch.float32)
        self.categorical = resident(store["categorical"], torch.int64)
        if self.dense.shape[0] != self.categorical.shape[0]:
            raise ValueError("dense_projected and categorical must have one row per entity")

    def __len__(self):
        return self.dense.shape[0]

    def gather(self, entity_idx: torch.Tensor) -> Dict:
        dense, ids = ops.batch_gather(entity_idx, self.dense, self.categorical)
        return {"dense": dense, "kjt": KeyedJaggedTensor(self.keys, ids)}


class DeviceBagFeatureStore:
    """One tower's entities with MULTI-VALUED categorical features, resident on the device: dense f32 [N, Din] and the bags as CSR
    over (entity, key) slots -- offsets int64 [N*K + 1], values int64 [nnz]; the bag of entity e, key k is
    values[offsets[e*K + k] : offsets[e*K + k + 1]].  An entity's K bags are one contiguous run, so a batch's values() in the
    sample-major wire format (kjt.build_bag_kjt: slot b*K + k) is the concatenation of its entities' runs: what
    ops.bag_store_gather packs without a host round trip.  Ids are stored verbatim; the lookup clamps them as ever.
    Optional per-id weights (an entity's share per industry code, a confidence per licence): `weights` f32 [nnz], entry p the weight
    of values[p], stored verbatim as the ids are; gather() then returns a KJT with weights().  None: the store holds ids alone."""

    def __init__(self, store: Dict, categorical_keys, device):
        """store: {"dense_projected", "categorical_offsets", "categorical_values"} and optionally "categorical_weights", host arrays
        or tensors.  ValueError -- checked here, once -- unless the offsets start at 0, never decrease, end at len(values) and number
        N*K + 1 for dense's N, and the weights (when given) are exactly len(values) entries in one dimension."""
        self.device = torch.device(device)
        self.keys = list(categorical_keys)
        def resident(x, dtype):
            t = x if torch.is_tensor(x) else torch.as_tensor(np.ascontiguousarray(x))
            return t.to(device=self.device, dtype=dtype).contiguous()
        self.dense = resident(store["dense_projected"], torch.float32)
        self.offsets = resident(store["categorical_offsets"], torch.int64).reshape(-1)
        self.values = resident(store["categorical_values"], torch.int64).reshape(-1)
        if self.dense.dim() != 2:
            raise ValueError("dense_projected must be [N, Din]")
        N, K = self.dense.shape[0], len(self.keys)
        if self.offsets.numel() != N * K + 1:
            raise ValueError(f"categorical_offsets: {self.offsets.numel()} entries, {N} entities of {K} keys need N*K + 1 = {N * K + 1}")
        if int(self.offsets[0]) != 0:
            raise ValueError("categorical_offsets must start at 0")
        if N * K and bool((self.offsets[1:] < self.offsets[:-1]).any()):
            raise ValueError("categorical_offsets must not decrease")
        if int(self.offsets[-1]) != self.values.numel():
            raise ValueError(f"categorical_offsets end at {int(self.offsets[-1])}, categorical_values holds {self.values.numel()} ids")
        ends = self.offsets[::K] if K else self.offsets.new_zeros(N + 1)
        self.run_lengths = (ends[1:] - ends[:-1]).contiguous()            # int64 [N]: the ids per entity
        self.weights = None
        w = store.get("categorical_weights")
        if w is not None:
            w = w if torch.is_tensor(w) else torch.as_tensor(np.asarray(w))
            if w.dim() != 1 or w.numel() != self.values.numel():             # (refused, not reshaped)
                raise ValueError(f"categorical_weights: shape {list(w.shape)}, categorical_values holds {self.values.numel()} ids "
                                 f"(one weight per id: [{self.values.numel()}])")
            self.weights = w.to(device=self.device, dtype=torch.float32).contiguous()

    @classmethod
    def from_bags(cls, dense, bags, categorical_keys, device, weights=None):
        """bags[e][k]: the list of ids of entity e, key k; weights[e][k][i]: the weight of bags[e][k][i] (a nested list shaped exactly
        like `bags`), or None"""
        K = len(categorical_keys)
        if any(len(row) != K for row in bags):
            raise ValueError(f"every entity needs one id list per key ({K} keys)")
        lengths = np.array([len(bag) for row in bags for bag in row], dtype=np.int64)
        values = np.array([int(i) for row in bags for bag in row for i in bag], dtype=np.int64)
        offsets = np.concatenate([np.zeros(1, dtype=np.int64), np.cumsum(lengths)])
        store = {"dense_projected": dense, "categorical_offsets": offsets, "categorical_values": values}
        if weights is not None:
            if len(weights) != len(bags) or any(not isinstance(wr, (list, tuple)) or len(wr) != K for wr in weights):
                raise ValueError(f"weights must list, per entity, one weight list per key ({len(bags)} entities, {K} keys)")
            if any(not isinstance(wb, (list, tuple)) or len(wb) != len(bag) for row, wr in zip(bags, weights) for bag, wb in zip(row, wr)):
                raise ValueError("every bag needs one weight per id: a weight list does not have its bag's length")
            store["categorical_weights"] = np.array([float(w) for wr in weights for wb in wr for w in wb], dtype=np.float32)
        return cls(store, categorical_keys, device)

    @classmethod
    def from_single(cls, store: DeviceFeatureStore):
        """the plain store's entities, every bag of length one"""
        n = store.categorical.numel()
        return cls({"dense_projected": store.dense, "categorical_offsets": torch.arange(n + 1, dtype=torch.int64, device=store.device),
                    "categorical_values": store.categorical.reshape(-1)}, store.keys, store.device)

    def __len__(self):
        return self.dense.shape[0]

    def gather(self, entity_idx: torch.Tensor, n_ids: Optional[int] = None) -> Dict:
        """{"dense", "kjt"} of the entities `entity_idx` (int64 [B]; an index outside the store is clamped into it), the kjt in the
        bag wire format -- DeviceFeatureStore.gather's duck type.  n_ids: the batch's id count, when the caller knows it
        (DevicePairLoader.epoch_bag_ids); without it this call reads ONE word back from the device to size values() -- a host
        synchronisation per call.  A wrong n_ids writes no ids and raises the device error word (_lib.check_device_errors).
        A store with weights: the kjt carries weights() f32 [n_ids], position for position beside the ids, from the same launches."""
        B, K = entity_idx.numel(), len(self.keys)
        idx = entity_idx.to(torch.int64).reshape(-1).contiguous()
        if n_ids is None:
            n_ids = int(self.run_lengths[idx.clamp(0, max(len(self) - 1, 0))].sum()) if B and len(self) else 0
        dense = torch.empty((B, self.dense.shape[1]), dtype=torch.float32, device=self.device)
        lengths = torch.empty(B * K, dtype=torch.int64, device=self.device)
        ids = torch.empty(int(n_ids), dtype=torch.int64, device=self.device)
        if self.weights is None:
            if B:
                ops.bag_store_gather([], [ops.BagStoreSide(idx, 1, self.dense, self.offsets, self.values, K, dense, lengths, ids, int(n_ids))], B)
            return {"dense": dense, "kjt": KeyedJaggedTensor(self.keys, ids, lengths)}
        w = torch.empty(int(n_ids), dtype=torch.float32, device=self.device)
        if B:
            ops.bag_store_gather([], [ops.BagStoreSide(idx, 1, self.dense, self.offsets, self.values, K, dense, lengths, ids, int(n_ids),
                                                       self.weights, w)], B)
        return {"dense": dense, "kjt": KeyedJaggedTensor(self.keys, ids, lengths, w)}


def batch_id_counts(run_lengths: torch.Tensor, entities: torch.Tensor, batch_size: int) -> torch.Tensor:
    """int64 [n_batches]: the ids of every batch of `entities` (int64 [n], in epoch order; the last batch may be ragged) --
    run_lengths[entities] summed per batch.  Plain torch on whatever device the arguments live on."""
    n = entities.numel()
    nb = (n + batch_size - 1) // batch_size
    runs = torch.zeros(nb * batch_size, dtype=torch.int64, device=entities.device)
    runs[:n] = run_lengths[entities]
    return runs.view(nb, batch_size).sum(1)


NEGATIVE_SEED_OFFSET = 0x5851F42D                  # the extras' generator: the loader's seed plus this


def _refuse_bag_mode_step(step, who: str, stores=None) -> None:
    """The store-fed hand-over of plain stores writes B*K ids per side into a captured step's static buffers: a step whose task pools
    ragged bags (bag mode) is refused before the epoch starts (once per epoch, not per batch) -- unless every side that pools is fed
    from a DeviceBagFeatureStore (`stores`: the (notice, company) stores of a loader that may hold some)."""
    task = getattr(step, "task", None)
    if isinstance(task, torch.nn.Module):
        from .cat_embed import refuse_bag_mode
        model = getattr(task, "two_tower_model", None)
        towers = [getattr(model, name, None) for name in ("notice_tower", "company_tower")]
        if stores is not None and all(isinstance(st, DeviceBagFeatureStore) or
                                      not getattr(getattr(tw, "categorical_embedder", None), "bag_mode", True)
                                      for st, tw in zip(stores, towers)):
            return
        refuse_bag_mode(task, who)


class DevicePairLoader:
    """Iterates over (notice_idx, company_idx) pairs in batches; len() = number of batches (drop_last=False,
    as torch's DataLoader default used by the reference: unified_bid_data_loader.py:1090-1110)."""

    def __init__(self, notice, company, pairs: np.ndarray, batch_size: int,
                 shuffle: bool, seed: int = 42, log_q=None, mask_repeats: bool = False, pair_weight=None, extra_negatives: int = 0,
                 negative_pool=None, mined=None, hard_fraction: float = 1.0, mask_known: bool = False, known_pairs=None):
        """notice / company: a DeviceFeatureStore or, for multi-valued features, a DeviceBagFeatureStore (either side, or both).
        mask_repeats: every batch carries "entity" [B] int32 on both sides -- the pair's notice and company indices -- and the train
        task masks the in-batch negatives that repeat a row's notice or company (the repeated-entity mask).
        log_q: optional (notice [Nn], company [Nc]) f32 log sampling probabilities per entity (sampling_bias.log_sampling_probs):
        every batch then carries "log_q" [B] on both sides and the train task applies the logQ correction.
        pair_weight: optional f32 [P], one raw sample weight per row of `pairs` (pair_weights.inverse_count_weights): every batch
        then carries "pair_weight" [B] and the train task takes the weighted mean of the pairs' loss terms.
        extra_negatives: M > 0: every batch carries "negatives", M company rows drawn uniformly (with replacement) from the company
        store -- or from negative_pool, an int64 tensor of company rows such as mined hard negatives -- which the train task contrasts
        with every notice of the batch besides the in-batch companies.  They carry "log_q" = log(1 / pool size) when the loader
        corrects and "entity" = the company row when mask_repeats is on.  Drawn per epoch from a generator of their own: a seed's pair
        order is the same with and without extras.
        mined: a hard_negatives.MinedNegatives (or its int32 table [len(notice), per_notice], -1 = empty): the first
        H = round(hard_fraction * M) extras of a batch are drawn, uniformly with replacement, from the rows mined for THAT batch's
        notices; the other M - H, and all of a batch whose notices have no mined row, are drawn from the store as above.  A mined
        slot's "log_q" is -log(number of candidates of its batch), its proposal's.  Not together with negative_pool.
        mask_known: every batch carries "masked_cells" int32 [L, 2]: the cells (row a, column j) whose column -- an in-batch company
        (j < B) or an extra (j >= B) -- is a KNOWN company of row a's notice, the positive itself left out; the train task takes them
        out of both softmax directions.  known_pairs: [P', 2] entity rows (notice index, company index), default the loader's own pair
        table (a caller may pass train plus validation pairs).  Not together with mask_repeats (these cells hold every repeat) or
        pair_weight."""
        self.notice, self.company, self.batch_size, self.shuffle = notice, company, batch_size, shuffle
        pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
        if len(pairs) and (pairs[:, 0].max() >= len(notice) or pairs[:, 1].max() >= len(company) or pairs.min() < 0):
            raise KeyError("pair refers to an entity that is not in the feature store")      # reference raises KeyError: :495-498
        self.pairs = torch.from_numpy(pairs).to(notice.device)
        self.entity = None
        self.set_mask_repeats(mask_repeats)
        # the epoch permutation is drawn where it is used: a host randperm of 1.6 M pairs + its upload cost ~20 ms per epoch,
        # a third of a 68-ms epoch at batch 8192 (profiles/NOTES.md, round 4)
        self._gen = torch.Generator(device=self.pairs.device)
        self._gen.manual_seed(seed)
        self.log_q = None
        self.set_log_q(log_q)
        self.pair_weight = None
        self.set_pair_weight(pair_weight)
        self._neg_gen = torch.Generator(device=self.pairs.device)
        self._neg_gen.manual_seed((int(seed) + NEGATIVE_SEED_OFFSET) & ((1 << 63) - 1))
        self.extra_negatives, self.negative_pool = 0, None
        self.mined, self.hard_slots, self._epoch_cand = None, 0, None
        self.set_extra_negatives(extra_negatives, negative_pool, mined, hard_fraction)
        self.known, self.max_cells, self.eager_cell_batches = None, 0, 0
        self.set_mask_known(mask_known, known_pairs)
        self.eager_bag_batches = 0         # step_batches: batches with more ids than the captured step's bag_capacity

    def set_mask_known(self, mask_known: bool, known_pairs=None) -> None:
        """Turns the known-pair mask on / off for every batch this loader produces from now on.  known_pairs: [P', 2] (notice index,
        company index) rows, default the loader's pair table.  Keeps the per-notice lists of known companies (CSR, as
        retrieval.exclusions_from_pairs builds them)."""
        self.known, self.max_cells = None, 0
        if not mask_known:
            return
        if self.entity is not None:
            raise ValueError("mask_known does not combine with mask_repeats: the known pairs' cells hold every repeat")
        if self.pair_weight is not None:
            raise ValueError("mask_known does not combine with pair_weight")
        from .retrieval import exclusions_from_pairs
        dev = self.pairs.device
        kp = self.pairs if known_pairs is None else torch.as_tensor(np.asarray(known_pairs, dtype=np.int64).reshape(-1, 2)).to(dev)
        if kp.numel() and (int(kp[:, 0].min()) < 0 or int(kp[:, 0].max()) >= len(self.notice)):
            raise KeyError("known_pairs refers to a notice that is not in the feature store")
        if len(self.company) - 1 > np.iinfo(np.int32).max:
            raise ValueError("mask_known: a company row does not fit int32")
        try:
            off, rows = exclusions_from_pairs(torch.arange(len(self.notice), device=dev), kp, len(self.company))
        except ValueError as e:
            raise KeyError("known_pairs refers to a company that is not in the feature store") from e
        self.known = (off, rows.to(torch.int64))

    CELLS_CHUNK_BATCHES = 8            # batches joined at a time by epoch_cells: what bounds its transient memory

    def epoch_cells(self, order: Optional[torch.Tensor] = None, negatives: Optional[torch.Tensor] = None):
        """This epoch's masked cells, or None without mask_known: (cells int32 [T, 2], bounds) -- batch k's cells are
        cells[bounds[k][0]:bounds[k][1]] (bounds: a host list of n_batches (lo, hi) pairs; every lo is even, so every batch's slice
        starts 16 bytes aligned and a captured step takes it as one copy segment of its hand-over -- an odd batch is followed by one
        unused row), rows (a, j) local to the batch: a the row, j < m an in-batch column, j >= m extra j - m (m = the batch's size;
        the ragged last batch has its own).  A cell is listed when column j's company is a known company of row a's notice and
        j != a; each (a, j) once, rows ascending.  order / negatives: this epoch's epoch_order() and epoch_negatives().
        Vectorised device passes over CELLS_CHUNK_BATCHES batches at a time and ONE read of the per-batch counts at the end (their
        largest is kept as self.max_cells).  Memory: the result, 8 bytes per cell of the epoch, plus the join's transient arrays --
        about ten int64 arrays over the (row, known company) keys and the hits of ONE chunk, i.e. some 100 bytes per cell of the
        chunk's batches (a pair table in which a few companies bid everywhere lists a few per cent of B * (B + M) cells per batch)."""
        if self.known is None:
            return None
        if self.shuffle and order is None:
            raise ValueError("epoch_cells(): a shuffling loader needs this epoch's order")
        if (negatives is not None) != bool(self.extra_negatives):
            raise ValueError("epoch_cells(): a loader with extra_negatives needs this epoch's epoch_negatives(), one without takes none")
        n, B, dev = self.pairs.shape[0], self.batch_size, self.pairs.device
        nb = len(self)
        sel = self.pairs if order is None else self.pairs[order]
        parts = [self._chunk_cells(sel, negatives, b0, min(b0 + self.CELLS_CHUNK_BATCHES, nb))
                 for b0 in range(0, nb, self.CELLS_CHUNK_BATCHES)]
        k = torch.cat([p[0] for p in parts]) if parts else torch.zeros(0, dtype=torch.int64, device=dev)
        aj = torch.cat([p[1] for p in parts]) if parts else torch.zeros((0, 2), dtype=torch.int32, device=dev)
        counts = torch.bincount(k, minlength=nb)
        padded = (counts + 1) // 2 * 2                                     # every batch starts on an even row
        start = torch.cumsum(padded, 0) - padded
        first = torch.cumsum(counts, 0) - counts
        host = torch.stack([start, counts]).tolist()                      # the epoch's one read of the counts
        cells = torch.zeros((int(sum(host[1])) + int(sum(c & 1 for c in host[1])), 2), dtype=torch.int32, device=dev)
        cells[start[k] + (torch.arange(k.shape[0], dtype=torch.int64, device=dev) - first[k])] = aj
        bounds = [(lo, lo + c) for lo, c in zip(host[0], host[1])]
        self.max_cells = max(host[1], default=0)
        return cells, bounds

    def _chunk_cells(self, sel, negatives, b0, b1):
        """(batch index int64 [T], (a, j) int32 [T, 2]) of the batches b0 .. b1 - 1, sorted by batch, row, column"""
        n, B, M, dev = self.pairs.shape[0], self.batch_size, self.extra_negatives, self.pairs.device
        Nc, nbc = len(self.company), b1 - b0
        koff, krows = self.known
        r0, r1 = b0 * B, min(b1 * B, n)
        sub = sel[r0:r1]
        # the columns of every batch: its companies, then its extras; a slot past the ragged batch's end never matches
        cols = torch.full((nbc * B,), -1, dtype=torch.int64, device=dev)
        cols[:r1 - r0] = sub[:, 1]
        cols = cols.view(nbc, B)
        if M:
            cols = torch.cat([cols, negatives[b0:b1].to(torch.int64)], 1)
        bk = torch.arange(nbc, dtype=torch.int64, device=dev)[:, None]
        ckey, cperm = torch.sort(torch.where(cols >= 0, bk * Nc + cols, torch.full_like(cols, -1)).view(-1), stable=True)
        # every (row, known company of its notice): the row's batch and that company as one key, looked up among the columns' keys
        deg = koff[sub[:, 0] + 1] - koff[sub[:, 0]]
        row = torch.repeat_interleave(torch.arange(r1 - r0, dtype=torch.int64, device=dev), deg)
        first = torch.cumsum(deg, 0) - deg
        comp = krows[koff[sub[row, 0]] + (torch.arange(row.shape[0], dtype=torch.int64, device=dev) - first[row])]
        key = (row // B) * Nc + comp
        lo = torch.searchsorted(ckey, key, right=False)
        cnt = torch.searchsorted(ckey, key, right=True) - lo
        hit = torch.repeat_interleave(torch.arange(key.shape[0], dtype=torch.int64, device=dev), cnt)   # a company met twice: both columns
        cfirst = torch.cumsum(cnt, 0) - cnt
        pos = cperm[lo[hit] + (torch.arange(hit.shape[0], dtype=torch.int64, device=dev) - cfirst[hit])] % (B + M)
        a = row[hit] % B
        kb = row[hit] // B
        size = torch.clamp(n - (kb + b0) * B, max=B)                      # the batch's own row count: where its extras' columns start
        j = torch.where(pos < B, pos, pos - B + size)
        keep = j != a
        kb, a, j = kb[keep], a[keep], j[keep]
        srt = torch.argsort((kb * B + a) * (B + M) + j)                    # by batch, row, column
        return kb[srt] + b0, torch.stack([a[srt], j[srt]], 1).to(torch.int32)

    def set_extra_negatives(self, extra_negatives: int, negative_pool=None, mined=None, hard_fraction: float = 1.0) -> None:
        """M >= 0 shared extra negatives per batch (0: none), drawn from the whole company store or from `negative_pool` (int64 [n >= 1]
        company rows) -- or, with `mined` (a MinedNegatives or its table), the first round(hard_fraction * M) of them from the rows
        mined for the batch's own notices"""
        M = int(extra_negatives)
        if M < 0:
            raise ValueError(f"extra_negatives must be >= 0, got {M}")
        table, H = None, 0
        hard_fraction = float(hard_fraction)
        if not 0.0 < hard_fraction <= 1.0:
            raise ValueError(f"hard_fraction must be in (0, 1], got {hard_fraction}")
        if mined is not None:
            if M == 0:
                raise ValueError("mined negatives need extra_negatives > 0")
            if negative_pool is not None:
                raise ValueError("mined negatives do not combine with negative_pool")
            t = getattr(mined, "table", mined)
            if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.dim() != 2 or t.shape[0] != len(self.notice) \
                    or t.shape[1] < 1:
                raise ValueError(f"mined: need an int32 table of shape [{len(self.notice)}, per_notice >= 1], got "
                                 f"{getattr(t, 'dtype', type(t).__name__)} {list(getattr(t, 'shape', []))}")
            if int(t.max()) >= len(self.company):
                raise KeyError("mined refers to a company that is not in the feature store")
            table, H = t.to(self.pairs.device).contiguous(), int(round(hard_fraction * M))
        if M > 0 and self.pair_weight is not None:
            raise ValueError("extra_negatives do not combine with pair_weight")
        pool = None
        if negative_pool is not None:
            t = negative_pool
            if not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or t.dim() != 1 or t.shape[0] < 1:
                raise ValueError(f"negative_pool: need an int64 tensor of shape [n >= 1], got "
                                 f"{getattr(t, 'dtype', type(t).__name__)} {list(getattr(t, 'shape', []))}")
            if int(t.min()) < 0 or int(t.max()) >= len(self.company):
                raise KeyError("negative_pool refers to a company that is not in the feature store")
            pool = t.to(self.pairs.device).contiguous()
        if M > 0 and pool is None and len(self.company) < 1:
            raise ValueError("extra_negatives: the company store is empty")
        if M > 0 and len(self.company) - 1 > np.iinfo(np.int32).max:
            raise ValueError("extra_negatives: a company row does not fit int32")
        self.extra_negatives, self.negative_pool = M, pool
        self.mined, self.hard_slots, self._epoch_cand = table, H, None

    def epoch_negatives(self, order: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
        """int64 [n_batches, M]: this epoch's extra negatives, batch k's company rows at [k] -- ONE draw per epoch from the extras' own
        seeded generator (the pair order's generator is not touched).  None without extras.
        order: this epoch's epoch_order().  A loader with mined negatives draws a batch's first H slots from the rows mined for that
        batch's notices, so a shuffling one needs the order and raises without it."""
        if not self.extra_negatives:
            return None
        n_pool = self.negative_pool.shape[0] if self.negative_pool is not None else len(self.company)
        idx = torch.randint(0, n_pool, (len(self), self.extra_negatives), generator=self._neg_gen, device=self.pairs.device)
        if self.mined is not None:
            return self._draw_mined(idx, order)
        return self.negative_pool[idx] if self.negative_pool is not None else idx

    def _draw_mined(self, idx: torch.Tensor, order: Optional[torch.Tensor]) -> torch.Tensor:
        """idx [n_batches, M], the uniform draw, with the first H slots of every batch that has candidates replaced by a uniform draw
        (with replacement) among them: the valid entries of the mined table's rows of the batch's notices, one entry per pair of the
        batch.  One vectorised pass; the candidates' count per batch is kept for the slots' log q."""
        if self.shuffle and order is None:
            raise ValueError("epoch_negatives(): a shuffling loader with mined negatives needs this epoch's order")
        n, B, H, dev = self.pairs.shape[0], self.batch_size, self.hard_slots, self.pairs.device
        nb = len(self)
        rows_n = torch.full((nb * B,), -1, dtype=torch.int64, device=dev)
        rows_n[:n] = self.pairs[:, 0] if order is None else self.pairs[order, 0]
        cand = torch.where(rows_n[:, None] >= 0, self.mined[rows_n.clamp(min=0)].to(torch.int64), rows_n[:, None]).view(nb, -1)
        upto = torch.cumsum((cand >= 0).to(torch.int64), 1)                 # [nb, B * per_notice]: valid entries up to each
        count = upto[:, -1]
        self._epoch_cand = count
        if H == 0 or nb == 0:
            return idx
        u = torch.rand((nb, H), generator=self._neg_gen, device=dev, dtype=torch.float64)
        j = (u * count[:, None]).to(torch.int64).clamp(max=(count[:, None] - 1).clamp(min=0))       # the j-th valid entry
        at = torch.searchsorted(upto, j + 1).clamp(max=cand.shape[1] - 1)
        hard = cand.gather(1, at)
        idx[:, :H] = torch.where(count[:, None] > 0, hard, idx[:, :H])
        return idx

    def negatives(self, rows: torch.Tensor, n_cand: Optional[torch.Tensor] = None) -> Dict:
        """the batch entry "negatives" of the company rows `rows` (int64 [M]).  n_cand (mined negatives): the 0-d count of the batch's
        mined candidates -- the first H slots were drawn from that many rows (0: the batch fell back to the store)."""
        out = self.company.gather(rows.contiguous())
        if self.log_q is not None:
            n_pool = self.negative_pool.shape[0] if self.negative_pool is not None else len(self.company)
            out["log_q"] = torch.full((rows.shape[0],), -float(np.log(n_pool)), dtype=torch.float32, device=rows.device)
            if n_cand is not None and self.hard_slots:
                lq = -torch.log(n_cand.clamp(min=1).to(torch.float32))
                out["log_q"][:self.hard_slots] = torch.where(n_cand > 0, lq, out["log_q"][0])
        if self.entity is not None:
            out["entity"] = rows.to(torch.int32)
        return out

    def set_pair_weight(self, pair_weight) -> None:
        """f32 [P] raw sample weights, one per row of the pair table, or None: turns pair weights on / off for every batch this
        loader produces from now on."""
        if pair_weight is None:
            self.pair_weight = None
            return
        if getattr(self, "extra_negatives", 0):
            raise ValueError("pair_weight does not combine with extra_negatives")
        if getattr(self, "known", None) is not None:
            raise ValueError("pair_weight does not combine with mask_known")
        P = self.pairs.shape[0]
        t = pair_weight
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 1 or t.shape[0] != P:
            raise ValueError(f"pair_weight: need a float32 tensor of shape [{P}], got "
                             f"{getattr(t, 'dtype', type(t).__name__)} {list(getattr(t, 'shape', []))}")
        self.pair_weight = t.to(self.pairs.device).contiguous()

    def set_mask_repeats(self, mask_repeats: bool) -> None:
        """Turns the repeated-entity mask on / off for every batch this loader produces from now on: with it `entity` holds the pair
        table's columns as int32 [2, P] (notice indices, company indices)."""
        self.entity = None
        if mask_repeats and getattr(self, "known", None) is not None:
            raise ValueError("mask_repeats does not combine with mask_known: the known pairs' cells hold every repeat")
        if mask_repeats:
            if self.pairs.numel() and int(self.pairs.max()) > np.iinfo(np.int32).max:
                raise ValueError("mask_repeats: an entity index does not fit int32")
            self.entity = self.pairs.t().to(torch.int32).contiguous()

    def set_log_q(self, log_q) -> None:
        """(notice [Nn], company [Nc]) f32 log sampling probabilities per entity, or None: turns the logQ correction on / off for
        every batch this loader produces from now on."""
        if log_q is None:
            self.log_q = None
            return
        if not isinstance(log_q, (tuple, list)) or len(log_q) != 2:
            raise ValueError("log_q must be a (notice, company) pair of per-entity f32 tensors")
        out = []
        for name, t, n in (("notice", log_q[0], len(self.notice)), ("company", log_q[1], len(self.company))):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 1 or t.shape[0] != n:
                raise ValueError(f"log_q {name}: need a float32 tensor of shape [{n}], got "
                                 f"{getattr(t, 'dtype', type(t).__name__)} {list(getattr(t, 'shape', []))}")
            out.append(t.to(self.pairs.device).contiguous())
        self.log_q = tuple(out)

    def __len__(self) -> int:
        return (self.pairs.shape[0] + self.batch_size - 1) // self.batch_size

    def epoch_order(self) -> Optional[torch.Tensor]:
        """This epoch's permutation of the pair list on the device (None when not shuffling); drawn from the loader's seeded
        generator, so an epoch iterated through __iter__ and one driven through step_batches() see the same batches."""
        n = self.pairs.shape[0]
        return torch.randperm(n, generator=self._gen, device=self.pairs.device) if self.shuffle else None

    def bag_stores(self):
        """[(side, store, column of the pair table)] of the sides fed from a DeviceBagFeatureStore"""
        return [(side, st, col) for side, st, col in (("notice", self.notice, 0), ("company", self.company, 1))
                if isinstance(st, DeviceBagFeatureStore)]

    def epoch_bag_ids(self, order: Optional[torch.Tensor] = None) -> Optional[Dict[str, np.ndarray]]:
        """{side: int64 host array [n_batches]} -- the id count of every batch of this epoch on each side fed from a bag store (None:
        no such side).  Summed on the device from run_lengths[pairs[order]] (batch_id_counts) and read back ONCE per epoch: with it
        neither batch() nor the store-fed hand-over synchronises per batch.  order: this epoch's epoch_order()."""
        sides = self.bag_stores()
        if not sides:
            return None
        if self.shuffle and order is None:
            raise ValueError("epoch_bag_ids(): a shuffling loader needs this epoch's order")
        sel = self.pairs if order is None else self.pairs[order]
        counts = torch.stack([batch_id_counts(st.run_lengths, sel[:, col], self.batch_size) for _, st, col in sides]).cpu().numpy()
        return {side: counts[i] for i, (side, _, _) in enumerate(sides)}

    def _gather(self, side: str, idx: torch.Tensor, bag_ids, k: int) -> Dict:
        st = self.notice if side == "notice" else self.company
        if isinstance(st, DeviceBagFeatureStore):
            return st.gather(idx, None if bag_ids is None else int(bag_ids[side][k]))
        return st.gather(idx)

    def batch(self, order: Optional[torch.Tensor], lo: int, negatives: Optional[torch.Tensor] = None, cells=None, bag_ids=None) -> Dict:
        """negatives: this batch's row of epoch_negatives() (a loader with extras: required); cells: epoch_cells()'s result (a loader
        with mask_known: required); bag_ids: epoch_bag_ids()'s result (a loader with bag stores: optional -- without it every bag
        store's gather reads its id count back from the device)"""
        if (negatives is not None) != bool(self.extra_negatives):
            raise ValueError("batch(): a loader with extra_negatives needs this batch's row of epoch_negatives(), one without takes none")
        if (cells is not None) != (self.known is not None):
            raise ValueError("batch(): a loader with mask_known needs this epoch's epoch_cells(), one without takes none")
        sel = self.pairs[lo:lo + self.batch_size] if order is None else self.pairs[order[lo:lo + self.batch_size]]
        k = lo // self.batch_size
        out = {"notice": self._gather("notice", sel[:, 0].contiguous(), bag_ids, k),
               "company": self._gather("company", sel[:, 1].contiguous(), bag_ids, k)}
        if self.pair_weight is not None:
            w = self.pair_weight
            out["pair_weight"] = w[lo:lo + self.batch_size].clone() if order is None else w[order[lo:lo + self.batch_size]]
        if self.log_q is not None:
            out["notice"]["log_q"] = self.log_q[0][sel[:, 0]]
            out["company"]["log_q"] = self.log_q[1][sel[:, 1]]
        if self.entity is not None:
            out["notice"]["entity"] = sel[:, 0].to(torch.int32)
            out["company"]["entity"] = sel[:, 1].to(torch.int32)
        if negatives is not None:
            mined = self.mined is not None and self._epoch_cand is not None
            out["negatives"] = self.negatives(negatives, self._epoch_cand[lo // self.batch_size] if mined else None)
        if cells is not None:
            k = lo // self.batch_size
            out["masked_cells"] = cells[0][cells[1][k][0]:cells[1][k][1]]
        return out

    def epoch_entity(self, order: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
        """int32 [n_batches, 2, Bp] (Bp = batch_size rounded up to 4): the pairs' (notice index, company index) in this epoch's order,
        laid out as epoch_log_q's array -- ONE gather per epoch, every slice 16 bytes aligned.  None without mask_repeats."""
        if self.entity is None:
            return None
        n, B = self.pairs.shape[0], self.batch_size
        ent = self.entity if order is None else self.entity[:, order]
        nb, Bp = (n + B - 1) // B, (B + 3) // 4 * 4
        flat = torch.zeros((2, nb * B), dtype=torch.int32, device=self.pairs.device)
        flat[:, :n] = ent
        out = torch.zeros((nb, 2, Bp), dtype=torch.int32, device=self.pairs.device)
        out[:, :, :B] = flat.view(2, nb, B).transpose(0, 1)
        return out

    def epoch_pair_weight(self, order: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
        """f32 [n_batches, Bp] (Bp = batch_size rounded up to 4): the pairs' raw weights in this epoch's order, batch k's at [k, :m],
        every slice 16 bytes aligned as epoch_log_q's -- ONE gather per epoch.  None without pair_weight."""
        if self.pair_weight is None:
            return None
        n, B = self.pairs.shape[0], self.batch_size
        nb, Bp = (n + B - 1) // B, (B + 3) // 4 * 4
        flat = torch.zeros(nb * B, dtype=torch.float32, device=self.pairs.device)
        flat[:n] = self.pair_weight if order is None else self.pair_weight[order]
        out = torch.zeros((nb, Bp), dtype=torch.float32, device=self.pairs.device)
        out[:, :B] = flat.view(nb, B)
        return out

    def epoch_log_q(self, order: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
        """f32 [n_batches, 2, Bp] (Bp = batch_size rounded up to 4): the pairs' log q (notice row, company row) in this epoch's order,
        batch k's two sides at [k, 0, :m] / [k, 1, :m] -- ONE gather per epoch.  Every slice starts 16 bytes aligned, as the hand-over
        launch's copy segments must (a [2, P] array's slices would not whenever P or the batch size is not a multiple of 4).
        None without log_q."""
        if self.log_q is None:
            return None
        n, B = self.pairs.shape[0], self.batch_size
        sel = self.pairs if order is None else self.pairs[order]
        nb, Bp = (n + B - 1) // B, (B + 3) // 4 * 4
        flat = torch.zeros((2, nb * B), dtype=torch.float32, device=self.pairs.device)
        flat[0, :n] = self.log_q[0][sel[:, 0]]
        flat[1, :n] = self.log_q[1][sel[:, 1]]
        out = torch.zeros((nb, 2, Bp), dtype=torch.float32, device=self.pairs.device)
        out[:, :, :B] = flat.view(2, nb, B).transpose(0, 1)
        return out

    def __iter__(self) -> Iterator[Dict]:
        order = self.epoch_order()
        neg = self.epoch_negatives(order)
        cells = self.epoch_cells(order, neg)
        bag = self.epoch_bag_ids(order)
        for k, lo in enumerate(range(0, self.pairs.shape[0], self.batch_size)):
            yield self.batch(order, lo, None if neg is None else neg[k], cells, **({} if bag is None else {"bag_ids": bag}))

    def eval_batches(self, graphed_eval, eager_eval=None, max_batches: Optional[int] = None) -> int:
        """One pass over the pairs in order (no shuffling is applied here: the reference's test loader does not shuffle) through a
        GraphedEvalStep: full batches from the stores, the ragged last one through `eager_eval(batch) -> metrics dict` (skipped
        when None).  Returns the number of batches evaluated; the sums sit in `graphed_eval`."""
        _refuse_bag_mode_step(graphed_eval, "DevicePairLoader.eval_batches")
        n, B, done = self.pairs.shape[0], self.batch_size, 0
        order = self.epoch_order()
        for lo in range(0, n, B):
            if max_batches is not None and done >= max_batches:
                break
            if lo + B <= n:
                graphed_eval.step_from_store(self.notice, self.company, self.pairs, order, lo)
            elif eager_eval is not None:
                graphed_eval.add_eager(eager_eval(self._plain_batch(order, lo)))
            else:
                continue
            done += 1
        return done

    def step_batches(self, graphed_step, eager_step=None, ragged_step=None):
        """One epoch on the fast path: every full batch is gathered out of the stores by the captured step's own hand-over launch
        (GraphedTrainStep.step_from_store) and replayed; the ragged last batch -- a captured step has one batch size -- goes
        through `ragged_step` (a second GraphedTrainStep captured at the remainder's size, sharing task and optimiser) or, without
        one, through `eager_step(batch)` (skipped when None).  Yields the step's result dict per batch (an unrolled step's U results
        arrive together, after its one launch: read them before the next launch overwrites them)."""
        for st in (graphed_step, ragged_step):
            _refuse_bag_mode_step(st, "DevicePairLoader.step_batches", (self.notice, self.company))
        order = self.epoch_order()
        n, B = self.pairs.shape[0], self.batch_size
        U = int(getattr(graphed_step, "unroll", 1))
        neg = self.epoch_negatives(order)
        cells = self.epoch_cells(order, neg)
        bag = self.epoch_bag_ids(order)
        if bag is not None and neg is None and cells is None:
            yield from self._step_bag_batches(graphed_step, eager_step, ragged_step, order, bag)
            return
        if neg is not None or cells is not None:
            # extra negatives / masked cells: no store-fed hand-over -- the batches __iter__ yields, through the captured step's plain-copy
            # hand-over step(batch) (a step captured on a batch with the same M), the ragged one through ragged_step or the eager callable
            if U > 1:
                raise NotImplementedError("extra negatives and masked cells are not supported by the unrolled step")
            for k, lo in enumerate(range(0, n, B)):
                b = self.batch(order, lo, None if neg is None else neg[k], cells, **({} if bag is None else {"bag_ids": bag}))
                if cells is not None and eager_step is not None:
                    # the captured step this batch would take; with more cells than it has room for (.step would raise) the batch goes
                    # through the eager step instead -- counted in self.eager_cell_batches and warned about once per loader
                    g = graphed_step if lo + B <= n else (ragged_step if ragged_step is not None and
                                                          ragged_step.static["notice"]["dense"].shape[0] == n - lo else None)
                    if g is not None and b["masked_cells"].shape[0] > getattr(g, "cell_capacity", 0):
                        self.eager_cell_batches += 1
                        if self.eager_cell_batches == 1:
                            import warnings
                            warnings.warn(f"a batch carries {b['masked_cells'].shape[0]} masked cells, the captured step has room for "
                                          f"{g.cell_capacity} (cell_capacity): such batches run through the eager step "
                                          "(DevicePairLoader.eager_cell_batches counts them)")
                        yield eager_step(b)
                        continue
                if lo + B <= n and graphed_step is not None:
                    yield graphed_step.step(b)
                elif ragged_step is not None and lo + B > n and ragged_step.static["notice"]["dense"].shape[0] == n - lo:
                    yield ragged_step.step(b)
                elif eager_step is not None:
                    yield eager_step(b)
            return
        lq = self.epoch_log_q(order)
        if lq is not None and U > 1:
            raise NotImplementedError("the logQ correction is not supported by the unrolled step")
        ent = self.epoch_entity(order)
        if ent is not None and U > 1:
            raise NotImplementedError("the repeated-entity mask is not supported by the unrolled step")
        pw = self.epoch_pair_weight(order)
        if pw is not None and U > 1:
            raise NotImplementedError("pair weights are not supported by the unrolled step")
        kw = lambda lo, m: {**({} if lq is None else {"log_q": (lq[lo // B, 0, :m], lq[lo // B, 1, :m])}),
                            **({} if ent is None else {"entity": (ent[lo // B, 0, :m], ent[lo // B, 1, :m])}),
                            **({} if pw is None else {"pair_weight": pw[lo // B, :m]})}
        lo = 0
        while U > 1 and lo + U * B <= n:                      # unrolled.UnrolledTrainStep: U full batches per graph launch
            for r in graphed_step.steps_from_store(self.notice, self.company, self.pairs, order, [lo + j * B for j in range(U)]):
                yield r
            lo += U * B
        for lo in range(lo, n, B):
            if lo + B <= n:
                yield graphed_step.step_from_store(self.notice, self.company, self.pairs, order, lo, **kw(lo, B))
            elif ragged_step is not None and ragged_step.static["notice"]["dense"].shape[0] == n - lo:
                yield ragged_step.step_from_store(self.notice, self.company, self.pairs, order, lo, **kw(lo, n - lo))
            elif eager_step is not None:
                yield eager_step(self.batch(order, lo))

    def _step_bag_batches(self, graphed_step, eager_step, ragged_step, order, bag):
        """step_batches of a loader with bag stores (no extras, no masked cells): a batch whose id counts fit the captured step's
        bag_capacity goes through its store-fed hand-over (GraphedTrainStep.step_from_store(..., bag_ids=...): no host
        synchronisation, the counts come from epoch_bag_ids); one over the capacity goes through `eager_step` -- counted in
        self.eager_bag_batches and warned about once per loader; the ragged last batch through `ragged_step` or `eager_step` as ever."""
        n, B = self.pairs.shape[0], self.batch_size
        if int(getattr(graphed_step, "unroll", 1)) > 1:
            raise NotImplementedError("bag stores are not supported by the unrolled step")
        lq, ent, pw = self.epoch_log_q(order), self.epoch_entity(order), self.epoch_pair_weight(order)
        for k, lo in enumerate(range(0, n, B)):
            m = min(B, n - lo)
            g = graphed_step if m == B else (ragged_step if ragged_step is not None and
                                             ragged_step.static["notice"]["dense"].shape[0] == m else None)
            ids = {side: int(c[k]) for side, c in bag.items()}
            cap = (getattr(g, "bag_capacity", None) or {}) if g is not None else {}
            over = {side: c for side, c in ids.items() if side in cap and c > cap[side]}
            if g is not None and over and eager_step is not None:
                self.eager_bag_batches += 1
                if self.eager_bag_batches == 1:
                    import warnings
                    side, c = next(iter(over.items()))
                    warnings.warn(f"a batch carries {c} ids on the {side} side, the captured step has room for {cap[side]} "
                                  "(bag_capacity): such batches run through the eager step (DevicePairLoader.eager_bag_batches counts them)")
                g = None
            if g is not None:
                kw = {**({} if lq is None else {"log_q": (lq[k, 0, :m], lq[k, 1, :m])}),
                      **({} if ent is None else {"entity": (ent[k, 0, :m], ent[k, 1, :m])}),
                      **({} if pw is None else {"pair_weight": pw[k, :m]})}
                yield g.step_from_store(self.notice, self.company, self.pairs, order, lo, bag_ids=ids, **kw)
            elif eager_step is not None:
                yield eager_step(self.batch(order, lo, bag_ids=bag))

    def _plain_batch(self, order: Optional[torch.Tensor], lo: int) -> Dict:
        """batch(order, lo) without extras or masked cells, whatever the loader draws for training (evaluation ranks the batch's own
        companies)"""
        M, self.extra_negatives = self.extra_negatives, 0
        known, self.known = self.known, None
        try:
            return self.batch(order, lo)
        finally:
            self.extra_negatives, self.known = M, known

    def ragged_example(self) -> Optional[Dict]:
        """A batch of the remainder's size (pairs % batch_size), or None when the epoch has no ragged batch: the example a second
        captured step is built from."""
        n, B = self.pairs.shape[0], self.batch_size
        r = n % B
        if r == 0 or n < B:
            return None
        return self._head(r)

    def _head(self, r: int) -> Dict:
        sel = self.pairs[:r]
        out = {"notice": self.notice.gather(sel[:, 0].contiguous()), "company": self.company.gather(sel[:, 1].contiguous())}
        if self.log_q is not None:
            out["notice"]["log_q"] = self.log_q[0][sel[:, 0]]
            out["company"]["log_q"] = self.log_q[1][sel[:, 1]]
        if self.entity is not None:
            out["notice"]["entity"] = sel[:, 0].to(torch.int32)
            out["company"]["entity"] = sel[:, 1].to(torch.int32)
        if self.pair_weight is not None:
            out["pair_weight"] = self.pair_weight[:r].clone()
        if self.extra_negatives:                              # (an example of the right shapes: the extras' generator is not touched)
            n_pool = self.negative_pool.shape[0] if self.negative_pool is not None else len(self.company)
            idx = torch.arange(self.extra_negatives, device=self.pairs.device) % n_pool
            out["negatives"] = self.negatives(self.negative_pool[idx] if self.negative_pool is not None else idx)
        if self.known is not None:                            # (an example of the right form: an empty list)
            out["masked_cells"] = torch.zeros((0, 2), dtype=torch.int32, device=self.pairs.device)
        return out


def sklearn_split_indices(n: int, test_size: float, seed: int) -> Tuple[np.ndarray, np.ndarray]:
    """(train, test) index arrays -- membership AND order -- of `sklearn.model_selection.train_test_split(range(n),
    test_size=test_size, random_state=seed)`, which is how the reference's test-mode loader splits its pair list
    (unified_bid_data_loader.py:1222-1226; scripts/train.py: test_split 0.2, shuffle_seed 42).  scikit-learn's ShuffleSplit draws
    `RandomState(seed).permutation(n)`, takes the first n_test = ceil(test_size * n) entries as the test set and the following
    n - n_test as the training set.  Index work: bit-exact against tests/golden/split_indices.json (generated with scikit-learn
    itself by oracle/gen_split_fixture.py); scikit-learn is not needed at run time."""
    if not (0.0 < test_size < 1.0):
        return np.arange(n, dtype=np.int64), np.empty(0, dtype=np.int64)        # reference: test_split == 0 keeps every pair (:1227-1228)
    n_test = int(np.ceil(test_size * n))
    n_train = n - n_test
    if n_train <= 0:
        raise ValueError(f"With n_samples={n}, test_size={test_size} the resulting train set will be empty")     # sklearn's ValueError
    perm = np.random.RandomState(seed).permutation(n)
    return perm[n_test:n_test + n_train].astype(np.int64), perm[:n_test].astype(np.int64)


def create_unified_bid_dataloaders(db_engine, schema: TorchRecSchema, batch_size: int = 32, limit: Optional[int] = None,
                                   test_split: float = 0.1, shuffle_seed: int = 42, num_workers: int = 4, pin_memory: bool = False,
                                   prefetch_factor: int = 2, persistent_workers: bool = False, streaming: bool = False,
                                   chunk_size: int = 1000, load_all_features: bool = True, feature_chunksize: int = 5000,
                                   feature_limit: Optional[int] = None, use_preprocessor: bool = True, test_mode: bool = False,
                                   pair_limit: Optional[int] = None, device="cuda:0") -> Tuple[DevicePairLoader, DevicePairLoader]:
    """Same signature as the reference factory (:971-990); `db_engine` is a feature/pair source object
    (see FeaturePreprocessor) offering additionally `load_pairs(pair_schema, limit)` -> list of
    ((bidntceno, bidntceord), bizno).  Worker / pinning / streaming knobs are accepted and ignored: there is
    no host-side batch assembly left to parallelise."""
    pre = FeaturePreprocessor(schema, device=str(device))
    stores = pre.preprocess_all(db_engine, feature_chunksize=feature_chunksize, feature_limit=feature_limit, show_progress=False)
    n2i, c2i = pre.build_id_mappings(stores)
    raw = db_engine.load_pairs(schema.pair, pair_limit if test_mode else limit)
    idx = np.empty((len(raw), 2), dtype=np.int64)
    for i, (nk, ck) in enumerate(raw):
        if tuple(nk) not in n2i:
            raise KeyError(f"Notice ID not found in features: {tuple(nk)}")
        if str(ck) not in c2i:
            raise KeyError(f"Company ID not found in features: {ck}")
        idx[i] = (n2i[tuple(nk)], c2i[str(ck)])
    train_sel, test_sel = sklearn_split_indices(len(idx), test_split, shuffle_seed)
    test_idx, train_idx = idx[test_sel], idx[train_sel]
    ns = DeviceFeatureStore(stores["notice"], schema.notice.categorical, device)
    cs = DeviceFeatureStore(stores["company"], schema.company.categorical, device)
    return (DevicePairLoader(ns, cs, train_idx, batch_size, shuffle=True, seed=shuffle_seed),
            DevicePairLoader(ns, cs, test_idx, batch_size, shuffle=False, seed=shuffle_seed))
