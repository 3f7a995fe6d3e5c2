"""CatalogIndex -- catalogue-wide retrieval with the trained towers.

The training step ranks a notice against the companies of its own batch.  A user of the model searches the whole company
catalogue: the catalogue is embedded once (company tower, eval mode) and packed once, and every search streams it past the
queries in one fused score + select sweep (tt_retrieve_topk_bf16 / tt_retrieve_topk_f32) that never writes the nQ x nC score
matrix to memory.

    index = CatalogIndex.from_store(model, company_store)         # row i of the index = entity i of the store
    vals, idx = index.search(notice_embeddings, k=10)             # s = <q, c> / T, value descending, ties -> lower index
    ranks = index.rank(notice_embeddings, positives)              # #{c : s > s_p} + #{c < p : s == s_p}

k goes up to MAX_K = 512 (candidates for a re-ranker, hard negatives past the near-duplicates): the same exact order, filler rule
and bitwise reproducibility at every k; k > 64 runs the sweep's large-k form (one wave per workgroup).

Every search also takes exclude=(offsets, rows), per-query exclusion lists in CSR form: query i's rows
rows[offsets[i]:offsets[i+1]] are left out of its top-k and its rank, inside the same sweep
(tt_excl_retrieve_topk_bf16 / _f32).  exclusions_from_pairs builds them from known (query key, row) pairs -- the filtered
ranking of link-prediction evaluation, or the companies that already bid on a notice when serving.

An index built with tags= (up to 128 attribute bits per row) also takes allow= / require=, per-query masks: a row is eligible
for query i when it shares a bit with allow[i] (unless allow[i] is zero) and holds every bit of require[i] -- again inside the
sweep (tt_filt_retrieve_topk_bf16 / _f32), and combinable with exclude=.  onehot_bits and equality_bits build tags and masks:

    tags = equality_bits(region_code, 315) | onehot_bits(licence_class, 12, first_bit=18)      # fields: disjoint bit ranges
    index = CatalogIndex.from_store(model, company_store, tags=tags)
    index.search(q, 10, require=equality_bits(wanted_region, 315))                             # -1: don't care

search and search_with_rank also take max_score=, an f32 [nQ] score ceiling per query: only rows that score BELOW max_score[i]
enter query i's top-k, inside the sweep (tt_ceil_retrieve_topk_bf16 / _f32), so that all k slots go to rows under the ceiling;
the rank never sees it.  It combines with exclude= and is refused together with allow= / require=.  pair_scores gives the score
of a (query, row) pair bit for bit as the sweep forms it -- what a ceiling relative to a known positive is derived from
(hard_negatives.mine_hard_negatives).
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import ops
from .config import settings

MAX_K = 512


def exclusions_from_pairs(query_keys, pairs, nC: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """Canonical exclusion lists (offsets int64 [nQ + 1], rows int32 [offsets[-1]]) on query_keys' device: query i's list
    holds every c with (query_keys[i], c) a row of `pairs` [P, 2], ascending, without duplicates.  Repeated keys get the same
    list; a key without pairs gets an empty one.  Raises ValueError for a pair row outside [0, nC)."""
    keys = torch.as_tensor(query_keys)
    dev = keys.device
    keys = keys.to(torch.int64).reshape(-1).contiguous()
    pairs = torch.as_tensor(pairs).to(device=dev, dtype=torch.int64)
    if pairs.dim() != 2 or pairs.shape[1] != 2:
        raise ValueError("pairs must be a [P, 2] array of (query key, catalogue row) rows")
    if pairs.shape[0]:
        lo, hi = int(pairs[:, 1].min()), int(pairs[:, 1].max())
        if lo < 0 or hi >= nC:
            raise ValueError(f"pair catalogue rows must be in [0, {nC}), got [{lo}, {hi}]")
    up = torch.unique(pairs, dim=0) if pairs.shape[0] else pairs          # sorted by (key, row), duplicates removed
    pk, pc = up[:, 0].contiguous(), up[:, 1].contiguous()
    first = torch.searchsorted(pk, keys, right=False)
    count = torch.searchsorted(pk, keys, right=True) - first
    offsets = torch.zeros(keys.numel() + 1, dtype=torch.int64, device=dev)
    offsets[1:] = torch.cumsum(count, 0)
    n = int(offsets[-1])
    j = torch.arange(n, dtype=torch.int64, device=dev)
    q = torch.searchsorted(offsets[1:], j, right=True)                  # the query entry j belongs to
    rows = pc[first[q] + (j - offsets[q])].to(torch.int32)
    return offsets, rows


MAX_TAG_WORDS = 4


def _field(codes, n_values: int, first_bit: int, n_bits: int, words):
    codes = torch.as_tensor(codes)
    if codes.dim() != 1 or codes.dtype.is_floating_point or codes.dtype in (torch.bool, torch.complex64, torch.complex128):
        raise ValueError("codes must be a 1-D integer tensor")
    n_values, first_bit = int(n_values), int(first_bit)
    if n_values < 1 or first_bit < 0:
        raise ValueError(f"n_values must be >= 1 and first_bit >= 0, got {n_values} and {first_bit}")
    need = -(-(first_bit + n_bits) // 32)
    W = max(need, 1) if words is None else int(words)
    if not 1 <= W <= MAX_TAG_WORDS or need > W:
        raise ValueError(f"a field of {n_bits} bits at bit {first_bit} does not fit in {32 * min(max(W, 1), MAX_TAG_WORDS)} bits "
                         f"(words = {words}, at most {MAX_TAG_WORDS})")
    codes = codes.to(torch.int64)
    if codes.numel() and int(codes.max()) >= n_values:
        raise ValueError(f"codes must be < n_values = {n_values} (negative: no bits), got {int(codes.max())}")
    return codes, W


def _set_bits(out, rows_on, bit):
    """ORs bit `bit` [n] (a position in the 32 W bit row) into out int64 [n, W] where rows_on."""
    word = (bit // 32).clamp(0, out.shape[1] - 1)
    val = torch.where(rows_on, torch.ones_like(bit) << (bit % 32), torch.zeros_like(bit))
    out.scatter_(1, word[:, None], out.gather(1, word[:, None]) | val[:, None])


def _as_words(out):
    """int64 words in [0, 2^32) -> the same bit patterns as int32."""
    return torch.where(out >= 2 ** 31, out - 2 ** 32, out).to(torch.int32).contiguous()


def onehot_bits(codes, n_values: int, first_bit: int = 0, words: Optional[int] = None) -> torch.Tensor:
    """int32 [n, W] with bit first_bit + codes[i] set in row i (bit b is bit b % 32 of word b // 32); a negative code sets
    nothing.  As a catalogue tag under `allow`, "the row's value is one of the query's"; rows and queries use the same call.
    W = words, or as many words as the field's n_values bits at first_bit need.  Raises ValueError for a code >= n_values or
    a field that does not fit in 32 W bits (W <= 4).  Fields are combined by | over disjoint bit ranges."""
    codes, W = _field(codes, n_values, first_bit, int(n_values), words)
    out = torch.zeros((codes.numel(), W), dtype=torch.int64, device=codes.device)
    on = codes >= 0
    _set_bits(out, on, torch.where(on, codes, torch.zeros_like(codes)) + int(first_bit))
    return _as_words(out)


def equality_bits(codes, n_values: int, first_bit: int = 0, words: Optional[int] = None) -> torch.Tensor:
    """int32 [n, W]: the binary-plus-complement encoding of codes[i] in 2 b bits at first_bit, b = ceil(log2 n_values) (at least
    1): bit first_bit + j is binary digit j of the code, bit first_bit + b + j its complement.  With the same call on the
    catalogue side (tags) and on the query side (`require`), a row holds every required bit exactly when the two codes are
    equal.  A negative code gives zero bits: "don't care" for a query, and a catalogue row that satisfies no requirement.
    Raises ValueError like onehot_bits."""
    b = max(1, (int(n_values) - 1).bit_length())
    codes, W = _field(codes, n_values, first_bit, 2 * b, words)
    out = torch.zeros((codes.numel(), W), dtype=torch.int64, device=codes.device)
    on = codes >= 0
    for j in range(b):
        digit = ((codes >> j) & 1) == 1
        pos = torch.where(digit, torch.full_like(codes, int(first_bit) + j), torch.full_like(codes, int(first_bit) + b + j))
        _set_bits(out, on, pos)
    return _as_words(out)


def _check_words(x, n: int, what: str, device, W: Optional[int] = None) -> torch.Tensor:
    """An integer tensor [n] or [n, W] as contiguous int32 [n, W] (bit patterns kept; no host synchronisation)."""
    if not torch.is_tensor(x) or x.dtype not in (torch.int32, torch.int64, torch.uint8, torch.int16, torch.int8):
        raise ValueError(f"{what} must be an integer tensor")
    if x.dim() == 1:
        x = x[:, None]
    if x.dim() != 2 or x.shape[0] != n or not 1 <= x.shape[1] <= MAX_TAG_WORDS or (W is not None and x.shape[1] != W):
        want = f"({n},) or ({n}, W <= {MAX_TAG_WORDS})" if W is None else f"({n}, {W})" + (f" or ({n},)" if W == 1 else "")
        raise ValueError(f"{what} must have shape {want}, got {tuple(x.shape)}")
    if x.device != device:
        raise ValueError(f"{what} on {x.device}, catalogue on {device}")
    if x.dtype == torch.int64:                                             # values in [0, 2^32) keep their low 32 bits
        x = torch.where(x >= 2 ** 31, x - 2 ** 32, x)
    return x.to(torch.int32).contiguous()


class CatalogIndex:
    """A packed catalogue of nC rows of dimension D.  score_dtype 'bf16' keeps the tt_score_pack_bf16 image of C / T (queries
    are packed unscaled, so the score is <bf16(q), bf16(c / T)> in f32); 'fp32' keeps C as it is and scores with an f32 FMA
    chain times 1 / T.  'fp8' (a training-time mode) falls back to bf16 here: the index has no fp8 images.  'bf16x3' (also a
    training-time mode: near-f32 products) falls back to the exact 'fp32' sweep -- the fallback that keeps its precision.
    tags: an integer tensor [nC] or [nC, W <= 4] on the catalogue's device, W 32-bit tag words per row (onehot_bits,
    equality_bits), kept as contiguous int32 [nC, W]; the searches of an index with tags take allow= / require=."""

    def __init__(self, C: torch.Tensor, temperature: float = 1.0, score_dtype: Optional[str] = None, tags=None):
        if not torch.is_tensor(C) or C.dim() != 2 or C.shape[0] < 1 or not 1 <= C.shape[1] <= 256:
            raise ValueError("the catalogue must be a [nC >= 1, 1 <= D <= 256] tensor")
        if C.shape[0] >= 2 ** 31:
            raise ValueError("the catalogue holds at most 2^31 - 1 rows")
        score_dtype = score_dtype or settings.score_dtype
        if score_dtype not in ("fp32", "bf16", "bf16x3", "fp8"):
            raise ValueError(f"score_dtype must be 'fp32', 'bf16', 'bf16x3' or 'fp8', got {score_dtype!r}")
        if float(temperature) <= 0.0:
            raise ValueError(f"temperature must be > 0, got {temperature}")
        self.score_dtype = "fp32" if score_dtype in ("fp32", "bf16x3") else "bf16"
        self.temperature = float(temperature)
        self.inv_t = 1.0 / self.temperature
        self.device = C.device
        self.size, self.dim = int(C.shape[0]), int(C.shape[1])
        self.tags = None if tags is None else _check_words(tags, self.size, "tags", self.device)
        self.tag_words = 0 if self.tags is None else int(self.tags.shape[1])
        C = C.detach().to(torch.float32).contiguous()
        if self.score_dtype == "bf16":
            self.data = ops.score_pack_bf16(C, self.inv_t)
        else:
            self.data = C
        self._ws = {}

    @classmethod
    def from_embeddings(cls, C: torch.Tensor, temperature: float = 1.0, score_dtype: Optional[str] = None,
                        tags=None) -> "CatalogIndex":
        """Index of ready embeddings C [nC, D] (the towers' outputs are L2-normalised; nothing is normalised here).
        score_dtype: 'fp32' | 'bf16' | 'bf16x3' (-> fp32) | 'fp8' (-> bf16); default: the package's score_dtype setting (TT_SCORE_DTYPE).
        tags: the rows' attribute tag words, [nC] or [nC, W] integers (see the class)."""
        return cls(C, temperature, score_dtype, tags)

    @classmethod
    @torch.no_grad()
    def from_store(cls, model, company_store, chunk: int = 8192, score_dtype: Optional[str] = None, tags=None) -> "CatalogIndex":
        """Embeds every entity of a DeviceFeatureStore through the company tower, `chunk` rows at a time, in eval mode (running
        BatchNorm statistics, no dropout), and indexes the result: row i of the index is entity i of the store.  `model` is a
        TwoTowerTrainTask (its temperature and score_dtype are used) or a TwoTowerModel (temperature 1).  The model's
        train()/eval() state is restored afterwards.  tags: one row of attribute tag words per entity of the store."""
        if chunk < 1:
            raise ValueError("chunk must be >= 1")
        task = model if hasattr(model, "two_tower_model") else None
        tower_model = task.two_tower_model if task is not None else model
        temperature = float(task.temperature) if task is not None else 1.0
        if score_dtype is None and task is not None:
            score_dtype = task.score_dtype
        n = len(company_store)
        if n < 1:
            raise ValueError("the company store is empty")
        if tags is not None:
            tags = _check_words(tags, n, "tags", torch.device(company_store.device))
        modes = [(m, m.training) for m in model.modules()]
        model.eval()
        try:
            dev = company_store.device
            parts = []
            for s in range(0, n, chunk):
                ent = torch.arange(s, min(s + chunk, n), dtype=torch.int64, device=dev)
                emb = tower_model.get_company_embeddings(company_store.gather(ent))
                parts.append(emb.detach().float())
            C = torch.cat(parts, 0) if len(parts) > 1 else parts[0]
        finally:
            for m, was in modes:
                m.training = was
        return cls(C, temperature, score_dtype, tags)

    # ---- queries ------------------------------------------------------------------------------------------------------
    def _check_queries(self, Q: torch.Tensor) -> torch.Tensor:
        if not torch.is_tensor(Q) or Q.dim() != 2 or Q.shape[0] < 1:
            raise ValueError("queries must be a [nQ >= 1, D] tensor")
        if Q.shape[1] != self.dim:
            raise ValueError(f"query dimension {Q.shape[1]} != catalogue dimension {self.dim}")
        if Q.device != self.device:
            raise ValueError(f"queries on {Q.device}, catalogue on {self.device}")
        return Q.detach().to(torch.float32).contiguous()

    def _check_k(self, k: int) -> int:
        k = int(k)
        if not 1 <= k <= min(MAX_K, self.size):
            raise ValueError(f"k must be in [1, min({MAX_K}, catalogue size {self.size})], got {k}")
        return k

    def _check_positives(self, positives, nQ: int) -> torch.Tensor:
        if not torch.is_tensor(positives) or positives.shape != (nQ,):
            raise ValueError(f"positives must be a tensor of shape ({nQ},)")
        if positives.dtype not in (torch.int32, torch.int64):
            positives = positives.to(torch.int64)
        return positives.to(self.device).contiguous()

    def _check_exclude(self, exclude, nQ: int):
        """(offsets int64 [nQ + 1], rows int32) with every query's list sorted ascending, from a caller's CSR pair.  Rows may
        be int32 or int64 (converted) and in any order within a list; rows outside [0, nC) match nothing.  The offsets are
        used clamped to [0, len(rows)] and non-decreasing (no host synchronisation here: a search stays capturable)."""
        if not isinstance(exclude, (tuple, list)) or len(exclude) != 2:
            raise ValueError("exclude must be an (offsets, rows) pair")
        off, rows = exclude
        if not torch.is_tensor(off) or off.dtype != torch.int64 or off.shape != (nQ + 1,):
            raise ValueError(f"exclude offsets must be an int64 tensor of shape ({nQ + 1},)")
        if not torch.is_tensor(rows) or rows.dtype not in (torch.int32, torch.int64) or rows.dim() != 1:
            raise ValueError("exclude rows must be a 1-D int32 or int64 tensor")
        if off.device != self.device or rows.device != self.device:
            raise ValueError(f"exclude on {off.device} / {rows.device}, catalogue on {self.device}")
        n = rows.numel()
        off = torch.cummax(off.clamp(0, n), 0).values.contiguous()
        seg = torch.searchsorted(off, torch.arange(n, dtype=torch.int64, device=self.device), right=True)
        rows = rows.to(torch.int64).clamp(-1, self.size)                   # (outside [0, nC) either way: int32 without wrapping)
        order = torch.argsort(seg * (1 << 32) + rows)                       # (list, row): sorts within each list only
        return off, rows[order].to(torch.int32).contiguous()

    def _check_filter(self, allow, require, nQ: int):
        """None without masks, else the filt argument of ops._retrieve: (tags, W, allow, require) with the masks as contiguous
        int32 [nQ, W] (a [nQ] mask for W = 1).  No host synchronisation: a filtered search stays capturable."""
        if allow is None and require is None:
            return None
        if self.tags is None:
            raise ValueError("allow= / require= need an index built with tags=")
        a = None if allow is None else _check_words(allow, nQ, "allow", self.device, self.tag_words)
        r = None if require is None else _check_words(require, nQ, "require", self.device, self.tag_words)
        return self.tags, self.tag_words, a, r

    def _workspace(self, nQ: int, k: int) -> torch.Tensor:
        need = ops.retrieve_workspace_bytes(nQ, self.size, self.dim, k)
        key = torch.cuda.current_stream(self.device).cuda_stream
        ws = self._ws.get(key)
        if ws is None or ws.numel() < need:
            ws = torch.empty(max(need, 1), dtype=torch.uint8, device=self.device)
            self._ws[key] = ws
        return ws

    def _check_max_score(self, max_score, filt, nQ: int):
        """None, or the ceilings as a contiguous f32 [nQ] tensor.  No host synchronisation: a search with a ceiling stays
        capturable."""
        if max_score is None:
            return None
        if filt is not None:
            raise ValueError("max_score= does not combine with allow= / require=")
        if not torch.is_tensor(max_score) or max_score.dtype != torch.float32:
            raise ValueError("max_score must be a float32 tensor")
        if max_score.shape != (nQ,):
            raise ValueError(f"max_score must have shape ({nQ},), got {tuple(max_score.shape)}")
        if max_score.device != self.device:
            raise ValueError(f"max_score on {max_score.device}, catalogue on {self.device}")
        return max_score.detach().contiguous()

    def _call(self, Q: torch.Tensor, k: int, positives, exclude=None, filt=None, ceil=None):
        nQ = Q.shape[0]
        ws = self._workspace(nQ, k)
        if self.score_dtype == "bf16":
            q = ops.score_pack_bf16(Q, 1.0)
            return ops._retrieve(q, nQ, self.data, self.size, self.dim, k, self.inv_t, True, positives, ws, exclude, filt, ceil)
        return ops._retrieve(Q, nQ, self.data, self.size, self.dim, k, self.inv_t, False, positives, ws, exclude, filt, ceil)

    def pair_scores(self, Q: torch.Tensor, rows) -> torch.Tensor:
        """f32 [nQ]: the score of query i against catalogue row rows[i] (an integer tensor [nQ]), bit for bit the value a search
        computes for that pair -- for a bf16 index the queries are packed as search packs them.  NaN where rows[i] is outside
        [0, nC)."""
        Q = self._check_queries(Q)
        rows = self._check_positives(rows, Q.shape[0])
        nQ = Q.shape[0]
        if self.score_dtype == "bf16":
            return ops.pair_scores(ops.score_pack_bf16(Q, 1.0), nQ, self.data, self.size, self.dim, rows, self.inv_t, True)
        return ops.pair_scores(Q, nQ, self.data, self.size, self.dim, rows, self.inv_t, False)

    def search(self, Q: torch.Tensor, k: int = 10, exclude=None, allow=None, require=None,
               max_score=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """(vals f32 [nQ, k], idx int64 [nQ, k]): every query's k best catalogue rows, value descending, ties to the lower
        index.  1 <= k <= min(512, catalogue size).  exclude=(offsets int64 [nQ + 1], rows): query i's rows
        rows[offsets[i]:offsets[i+1]] are left out; if fewer than k rows remain, the last slots are -inf / -1.
        allow / require (an index with tags only): integer masks [nQ] or [nQ, W]; only rows that share a bit with a non-zero
        allow[i] and hold every bit of require[i] are eligible for query i.  They combine with exclude.
        max_score: f32 [nQ] on the index's device: only rows with a score below max_score[i] are kept for query i (a tie with
        the ceiling goes; NaN or +inf keeps every row, -inf none).  Combines with exclude; ValueError with allow / require."""
        k = self._check_k(k)
        Q = self._check_queries(Q)
        ex = None if exclude is None else self._check_exclude(exclude, Q.shape[0])
        filt = self._check_filter(allow, require, Q.shape[0])
        vals, idx, _ = self._call(Q, k, None, ex, filt, self._check_max_score(max_score, filt, Q.shape[0]))
        return vals, idx

    def search_with_rank(self, Q: torch.Tensor, k: int, positives, exclude=None, allow=None,
                         require=None, max_score=None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """search() and rank() from one sweep over the catalogue (the same exclusion lists and masks for both);
        1 <= k <= min(512, catalogue size).  max_score bounds the top-k only: the rank is that of the call without it."""
        k = self._check_k(k)
        Q = self._check_queries(Q)
        pos = self._check_positives(positives, Q.shape[0])
        ex = None if exclude is None else self._check_exclude(exclude, Q.shape[0])
        filt = self._check_filter(allow, require, Q.shape[0])
        return self._call(Q, k, pos, ex, filt, self._check_max_score(max_score, filt, Q.shape[0]))

    def rank(self, Q: torch.Tensor, positives, exclude=None, allow=None, require=None) -> torch.Tensor:
        """int32 [nQ]: 0-based rank of catalogue row positives[i] for query i among ALL catalogue rows,
        #{c : s > s_p} + #{c < p : s == s_p} (tt_diag_rank_rows's rule); -1 where the positive is outside [0, nC).
        exclude=(offsets, rows): only rows outside query i's list count -- the filtered rank.  The positive never counts
        against itself, so it may be in its own list.  allow / require: only eligible rows count (see search); whether the
        positive itself is eligible makes no difference."""
        Q = self._check_queries(Q)
        pos = self._check_positives(positives, Q.shape[0])
        ex = None if exclude is None else self._check_exclude(exclude, Q.shape[0])
        return self._call(Q, 0, pos, ex, self._check_filter(allow, require, Q.shape[0]))[2]

    def __len__(self) -> int:
        return self.size

    def __repr__(self) -> str:
        tags = f", tag_words={self.tag_words}" if self.tags is not None else ""
        return (f"CatalogIndex(size={self.size}, dim={self.dim}, score_dtype={self.score_dtype!r}, "
                f"temperature={self.temperature}{tags})")

