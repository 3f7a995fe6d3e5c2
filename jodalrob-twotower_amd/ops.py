"""Thin Python wrappers over the C ABI (one per entry point of include/twotower.h).  They only
translate torch tensors to pointers/sizes and allocate outputs; no arithmetic happens here."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import List, NamedTuple, Optional, Sequence

import torch

from . import _lib as L
from .config import settings
from ._lib import TT_BF16, TT_F32, TT_GRAD_DENSE_ACC, TT_GRAD_DENSE_SET, TT_GRAD_SPARSE  # noqa: F401


class KernelTimer:
    """HIP-event timing of C-ABI calls on the stream they are enqueued on (bench.py: roofline legs)."""

    def __init__(self, names=None):
        self.names = set(names) if names else None
        self.records = {}

    def wants(self, name):
        return self.names is None or name in self.names

    def summary(self):
        """name -> (launches, mean ms); synchronises."""
        torch.cuda.synchronize()
        return {n: (len(ev), sum(a.elapsed_time(b) for a, b in ev) / max(len(ev), 1)) for n, ev in self.records.items()}


_TIMER: Optional[KernelTimer] = None
_SYNC_DEBUG = settings.sync_debug


def set_timer(t: Optional[KernelTimer]):
    global _TIMER
    _TIMER = t


class _timed:
    __slots__ = ("name", "a")

    def __init__(self, name):
        self.name = name
        self.a = None

    def __enter__(self):
        if _TIMER is not None and _TIMER.wants(self.name):
            self.a = torch.cuda.Event(enable_timing=True)
            self.a.record()
        return self

    def __exit__(self, *exc):
        if _SYNC_DEBUG and not torch.cuda.is_current_stream_capturing():     # TT_SYNC_DEBUG=1: name every C-ABI call and wait for it (fault hunting)
            import sys
            print(f"[tt] {self.name} ...", end="", file=sys.stderr, flush=True)
            torch.cuda.synchronize()
            print(" done", file=sys.stderr, flush=True)
        if self.a is not None:
            b = torch.cuda.Event(enable_timing=True)
            b.record()
            _TIMER.records.setdefault(self.name, []).append((self.a, b))
        return False


def _dt(t: torch.Tensor) -> int:
    if t.dtype == torch.float32:
        return TT_F32
    if t.dtype == torch.bfloat16:
        return TT_BF16
    raise TypeError(f"unsupported dtype {t.dtype}")


# ---------------------------------------------------------------------------------------------- lookup
@dataclass
class LookupSide:
    ids: torch.Tensor             # int64 [B*K] sample-major
    key_row_offset: torch.Tensor  # int64 [K] (device)
    key_vocab: torch.Tensor       # int64 [K] (device)
    out: torch.Tensor             # 2-D view [B, K*E] inside the destination buffer (row stride = ld)
    K: int


def embed_lookup(table: Optional[torch.Tensor], sides: Sequence[LookupSide], B: int, want_rows: bool, E: int = 0,
                 table_rows: int = 0, tag: str = "") -> Optional[torch.Tensor]:
    """table None => rows-only mode (E and table_rows then describe the row space)."""
    dev = table.device if table is not None else sides[0].ids.device
    E = table.shape[1] if table is not None else E
    table_rows = table.shape[0] if table is not None else table_rows
    arr = (L.EmbedSide * len(sides))()
    M = 0
    for i, s in enumerate(sides):
        if s.ids.dtype != torch.int64 or not s.ids.is_contiguous() or s.ids.device != dev:
            raise ValueError("ids must be a contiguous int64 tensor on the table's device")
        if s.ids.numel() != B * s.K:
            raise ValueError(f"side {i}: {s.ids.numel()} ids for B={B}, K={s.K}")
        if s.out is not None:
            assert s.out.stride(1) == 1
            arr[i] = L.EmbedSide(L.ptr(s.ids), L.ptr(s.key_row_offset), L.ptr(s.key_vocab), L.ptr(s.out),
                                 s.out.stride(0), s.K, _dt(s.out))
        else:
            arr[i] = L.EmbedSide(L.ptr(s.ids), L.ptr(s.key_row_offset), L.ptr(s.key_vocab), None, s.K * E, s.K, TT_F32)
        M += B * s.K
    rows = torch.empty(M, dtype=torch.int32, device=dev) if want_rows else None
    with _timed("tt_embed_lookup_fwd" + tag):
        L.check(L.load().tt_embed_lookup_fwd(L.ctx(dev), L.ptr(table), table_rows, E, arr, len(sides), B,
                                             L.ptr(rows), L.stream(dev)), "tt_embed_lookup_fwd")
    return rows


def embed_lookup_rows(table: torch.Tensor, rows: torch.Tensor, sides: Sequence[LookupSide], B: int):
    """tt_embed_lookup_rows_fwd: the lookup from precomputed fused rows (int32, slot order: the hand-over launch's `rows_sm`)."""
    dev, E = table.device, table.shape[1]
    arr = (L.EmbedSide * len(sides))()
    M = 0
    for i, s in enumerate(sides):
        assert s.out is not None and s.out.stride(1) == 1
        arr[i] = L.EmbedSide(None, None, None, L.ptr(s.out), s.out.stride(0), s.K, _dt(s.out))
        M += B * s.K
    if rows.dtype != torch.int32 or rows.numel() != M or not rows.is_contiguous() or rows.device != dev:
        raise ValueError("embed_lookup_rows: rows must be a contiguous int32 tensor of sum(B*K) elements on the table's device")
    with _timed("tt_embed_lookup_fwd"):
        L.check(L.load().tt_embed_lookup_rows_fwd(L.ctx(dev), L.ptr(table), table.shape[0], E, arr, len(sides), B, L.ptr(rows), L.stream(dev)),
                "tt_embed_lookup_rows_fwd")


class LookupProfile:
    """Device-clock stamps of the lookup kernel, one block of per-workgroup pairs per launch (works inside captured graphs,
    needs no host synchronisation and no extra launch while measuring; reduced on the host afterwards)."""

    MAX_WG = 8192

    def __init__(self, device, n_slots: int = 256):
        self.device, self.n = torch.device(device), n_slots
        self.ring = torch.zeros(self.MAX_WG + n_slots * self.MAX_WG * 2, dtype=torch.int64, device=self.device)
        L.check(L.load().tt_embed_lookup_set_profile(L.ctx(self.device), L.ptr(self.ring), n_slots), "tt_embed_lookup_set_profile")

    def reset(self):
        self.ring.zero_()

    def durations_us(self, first_wg: int = 0, last_wg: Optional[int] = None):
        """Kernel durations (us) of the (last n_slots) launches since the last reset(), oldest first; synchronises.
        first_wg / last_wg: only the workgroups [first_wg, last_wg) (the fused hand-over + lookup launch: its tiles -- the gather
        phase -- are the first workgroups, the copy roles follow)."""
        torch.cuda.synchronize(self.device)
        r = self.ring.cpu()
        launches = int(r[0])
        pairs = r[self.MAX_WG:].view(self.n, self.MAX_WG, 2)
        same = r[:self.MAX_WG] == launches          # workgroups that took part in every launch (grids of one size)
        if first_wg or last_wg is not None:
            sel = torch.zeros_like(same)
            sel[first_wg:last_wg] = True
            same = same & sel
        out = []
        for n in range(max(0, launches - self.n), launches):
            blk = pairs[n % self.n]
            live = (blk[:, 1] > 0) & same
            if bool(live.any()):
                out.append(float(blk[live, 1].max() - blk[live, 0].min()) * 0.01)   # 100 MHz clock
        return out

    def close(self):
        L.check(L.load().tt_embed_lookup_set_profile(L.ctx(self.device), None, 0), "tt_embed_lookup_set_profile")

    def reopen(self):
        L.check(L.load().tt_embed_lookup_set_profile(L.ctx(self.device), L.ptr(self.ring), self.n), "tt_embed_lookup_set_profile")


@dataclass
class DedupPlan:
    sorted_src: torch.Tensor
    unique_rows: torch.Tensor
    seg_offsets: torch.Tensor
    n_unique: torch.Tensor        # int32 [1] on device
    M: int
    keep: object = None           # tensors that must outlive the plan's kernels
    staging: object = None        # the keyed sort's staging arrays when the compaction is deferred (TT_OPT_DEFER_RIDERS)
    grad_ws: object = None        # (uint8 workspace, E): the gradient reduction's workspace with the long-row list already in it
    finish_deferred: object = None  # grad_rows whose long rows embed_grad left unfinished (adam_fused / embed_grad_finish complete them)


def dedup_plan(rows: torch.Tensor, table_rows: int) -> DedupPlan:
    dev, M = rows.device, rows.numel()
    buf = torch.empty(3 * M + 2, dtype=torch.int32, device=dev)
    plan = DedupPlan(buf[:M], buf[M:2 * M], buf[2 * M:3 * M + 1], buf[3 * M + 1:], M)
    lib = L.load()
    nb = lib.tt_dedup_workspace_bytes(M)
    ws = L.workspace(dev, nb)
    with _timed("tt_dedup_plan"):
        L.check(lib.tt_dedup_plan(L.ctx(dev), L.ptr(rows), M, table_rows, L.ptr(plan.sorted_src), L.ptr(plan.unique_rows),
                                  L.ptr(plan.seg_offsets), L.ptr(plan.n_unique), L.ptr(ws), ws.numel(), L.stream(dev)),
                "tt_dedup_plan")
    return plan


def dedup_plan_runs(rows: torch.Tensor, G: int, C: int, row_limit: int = 0) -> DedupPlan:
    """Plan of G ascending runs of C ids (stable merge; same outputs as dedup_plan on the concatenation).  row_limit > 0:
    ids >= row_limit are pads, grouped last and left out of n_unique."""
    dev, M = rows.device, G * C
    assert rows.numel() == M and rows.dtype == torch.int32
    buf = torch.empty(3 * M + 2, dtype=torch.int32, device=dev)
    plan = DedupPlan(buf[:M], buf[M:2 * M], buf[2 * M:3 * M + 1], buf[3 * M + 1:], M)
    lib = L.load()
    ws = L.workspace(dev, lib.tt_dedup_workspace_bytes(M))
    with _timed("tt_dedup_plan_runs"):
        L.check(lib.tt_dedup_plan_runs(L.ctx(dev), L.ptr(rows), G, C, row_limit, L.ptr(plan.sorted_src), L.ptr(plan.unique_rows),
                                       L.ptr(plan.seg_offsets), L.ptr(plan.n_unique), L.ptr(ws), ws.numel(), L.stream(dev)),
                "tt_dedup_plan_runs")
    return plan


KEYED_MAX_B = 8192


def dedup_plan_keyed(rows: torch.Tensor, side_K: Sequence[int], B: int, key_major: bool = False, E: int = 0) -> DedupPlan:
    """Plan for slot rows straight from embed_lookup (slot = side_base + b*K + k): per-key LDS sorts, 2 launches.
    key_major: `rows` is batch_ingest's [key][sample] array instead (rows[side_base + k*B + b]); same plan.
    E > 0: the plan also prepares embed_grad's long-row list for rows of E floats (tt_dedup_plan_keyed_long): its own gradient
    workspace travels with the plan, and embed_grad then runs its row and chunk passes as one launch."""
    dev, M = rows.device, rows.numel()
    assert M == B * sum(side_K)
    buf = torch.empty(3 * M + 2, dtype=torch.int32, device=dev)
    plan = DedupPlan(buf[:M], buf[M:2 * M], buf[2 * M:3 * M + 1], buf[3 * M + 1:], M)
    lib = L.load()
    nk = sum(side_K)
    if L.riders_deferred(dev, 1):    # the compaction runs later, inside the towers' launch: its staging arrays must outlive whatever
        ws = torch.empty(lib.tt_dedup_keyed_workspace_bytes(M, nk), dtype=torch.uint8, device=dev)      # takes the shared scratch meanwhile
    else:
        ws = L.workspace(dev, lib.tt_dedup_keyed_workspace_bytes(M, nk))
    plan.staging = ws
    ks = (L.i32 * len(side_K))(*side_K)
    if E > 0 and settings.grad_planned:
        gws = torch.empty(lib.tt_embed_grad_workspace_bytes(M, E), dtype=torch.uint8, device=dev)
        with _timed("tt_dedup_plan_keyed"):
            L.check(lib.tt_dedup_plan_keyed_long(L.ctx(dev), L.ptr(rows), int(key_major), ks, len(side_K), B, E, L.ptr(plan.sorted_src),
                                                 L.ptr(plan.unique_rows), L.ptr(plan.seg_offsets), L.ptr(plan.n_unique), L.ptr(gws),
                                                 gws.numel(), L.ptr(ws), ws.numel(), L.stream(dev)), "tt_dedup_plan_keyed_long")
        plan.grad_ws = (gws, E)
        return plan
    fn = lib.tt_dedup_plan_keyed_km if key_major else lib.tt_dedup_plan_keyed
    with _timed("tt_dedup_plan_keyed"):
        L.check(fn(L.ctx(dev), L.ptr(rows), ks, len(side_K), B, L.ptr(plan.sorted_src), L.ptr(plan.unique_rows),
                   L.ptr(plan.seg_offsets), L.ptr(plan.n_unique), L.ptr(ws), ws.numel(), L.stream(dev)),
                "tt_dedup_plan_keyed")
    return plan


def embed_grad(plan: DedupPlan, srcs: Sequence[tuple], B: int, E: int, mode: int, out: torch.Tensor, short_segments: bool = False,
               counters: Optional[torch.Tensor] = None, defer_finish: bool = False):
    """srcs: [(d_out 2-D view [B, K*E], K)].  short_segments: the caller knows no row has many contributions (skips the
    chunk passes; results do not depend on it).  counters: >= 3 int32 words the caller keeps ZERO between calls (allocated
    once, outside any graph capture): the reduction re-zeroes them itself and needs no zeroing launch in front.
    defer_finish (sparse mode, planned workspace; ignored otherwise): the long rows of `out` are left for adam_fused /
    embed_grad_finish -- plan.finish_deferred then holds `out` until one of them has run."""
    if short_segments:
        mode |= L.TT_GRAD_SHORT_SEGMENTS
    dev = out.device
    arr = (L.GradSrc * len(srcs))()
    for i, (d, K) in enumerate(srcs):
        assert d.stride(1) == 1
        arr[i] = L.GradSrc(L.ptr(d), d.stride(0), K, _dt(d))
    lib = L.load()
    nb = lib.tt_embed_grad_workspace_bytes(plan.M, E)
    if plan.grad_ws is not None and plan.grad_ws[1] == E and not short_segments:
        ws = plan.grad_ws[0]                                # the plan left the long-row list in its own workspace
        deferred = defer_finish and mode == L.TT_GRAD_SPARSE and plan.M >= 1
        mode |= L.TT_GRAD_PLANNED | (L.TT_GRAD_DEFER_FINISH if deferred else 0)
    else:
        ws = L.workspace(dev, nb)
        deferred = False
    with _timed("tt_embed_grad_bwd"):
        L.check(lib.tt_embed_grad_bwd(L.ctx(dev), arr, len(srcs), B, E, L.ptr(plan.sorted_src), L.ptr(plan.seg_offsets),
                                      L.ptr(plan.unique_rows), L.ptr(plan.n_unique), plan.M, mode, L.ptr(out),
                                      L.ptr(counters), L.ptr(ws), ws.numel(), L.stream(dev)), "tt_embed_grad_bwd")
    plan.finish_deferred = out if deferred else None


def embed_grad_finish(plan: DedupPlan):
    """Complete a gradient whose long-row finish was deferred (no-op otherwise)."""
    out = plan.finish_deferred
    if out is None:
        return
    ws, E = plan.grad_ws
    dev = out.device
    with _timed("tt_embed_grad_finish"):
        L.check(L.load().tt_embed_grad_finish(L.ctx(dev), E, L.ptr(plan.seg_offsets), plan.M, L.ptr(out), L.ptr(ws), ws.numel(),
                                              L.stream(dev)), "tt_embed_grad_finish")
    plan.finish_deferred = None


# ---------------------------------------------------------------------------------------------- embedding bags
POOL_MODES = {"sum": L.TT_POOL_SUM, "mean": L.TT_POOL_MEAN}


@dataclass
class BagPosWeights:
    """A pooled side's position-weight SOURCE: the lookup reads position j of a bag of key k from
    param[pw_offset[k] + min(j, pw_len[k] - 1)] itself (1.0 for a key with pw_offset < 0) instead of taking one weight per id."""
    param: torch.Tensor           # f32 [n_param] (device), contiguous: the learned parameter
    pw_offset: torch.Tensor       # int32 [K] (device): first element of key k in param, -1: the key has no position weights
    pw_len: torch.Tensor          # int32 [K] (device): max_len of key k


@dataclass
class BagSide:
    ids: torch.Tensor             # int64 [nnz]: the bags' ids, concatenated in slot order (slot = b*K + k)
    lengths: torch.Tensor         # int64 [B*K] (device): length of bag (b, k); 0 allowed
    key_row_offset: torch.Tensor  # int64 [K] (device)
    key_vocab: torch.Tensor       # int64 [K] (device)
    key_pool: torch.Tensor        # int32 [K] (device): TT_POOL_SUM / TT_POOL_MEAN
    out: torch.Tensor             # 2-D view [B, K*E] inside the destination buffer (row stride = ld)
    K: int
    any_mean: bool = True         # host copy of (key_pool == mean).any(): with no mean key the gradient needs no weights
    capacity: Optional[int] = None   # the CAPACITY form (a captured step's static buffers): ids holds `capacity` ids, of which the
                                     # first sum(lengths) are live -- device data; the tail is stale and never read
    count: Optional[torch.Tensor] = None   # (capacity form) int32 [1] on the device: the id count the host handed over, compared
                                           # with sum(lengths) on the device; None: not compared
    weights: Optional[torch.Tensor] = None # f32 [nnz] ([capacity] in the capacity form): one weight per id; None: every id weighs 1
    pos_weights: Optional[BagPosWeights] = None   # the weights come out of a position-weight parameter; never beside `weights`


class BagPlan(NamedTuple):
    """What embed_bag_lookup leaves for embed_bag_grad: rows / bag_of per position (int32 [nnz]), inv_len per slot (f32, None when
    every key sums), nnz.  The capacity form: nnz is the sides' total capacity and pad_row (= table rows) what `rows` holds where no
    bag covers -- the plan over such rows is bag_dedup_plan's padded one.  pos_w: the weighted form's weight per position (f32
    [nnz], valid where a bag covers), None when no side carried weights.  side_nnz: the positions of each side (they lie behind one
    another in rows / bag_of), what bag_weight_grad splits its result by; None on a plan built by hand: one side of nnz positions.  offsets:
    (capacity form) per side the int64 [B*K + 1] offsets tt_bag_prepare formed -- what bag_position_weights_bwd walks."""
    rows: torch.Tensor
    bag_of: torch.Tensor
    inv_len: Optional[torch.Tensor]
    nnz: int
    pad_row: Optional[int] = None
    pos_w: Optional[torch.Tensor] = None
    side_nnz: Optional[tuple] = None
    offsets: Optional[tuple] = None


def _check_bag_side(i: int, s: BagSide, B: int, E: int, dev, check_out: bool = True):
    if s.ids.dtype != torch.int64 or not s.ids.is_contiguous() or s.ids.device != dev:
        raise ValueError("bag ids must be a contiguous int64 tensor on the table's device")
    if s.lengths.numel() != B * s.K or s.lengths.device != dev:
        raise ValueError(f"side {i}: {s.lengths.numel()} bag lengths for B={B}, K={s.K} (on the table's device)")
    w = s.weights
    if w is not None and (w.dtype != torch.float32 or not w.is_contiguous() or w.device != dev or w.numel() != s.ids.numel()):
        raise ValueError(f"side {i}: bag weights must be a contiguous float32 tensor of ids.numel() = {s.ids.numel()} elements on the "
                         f"table's device, got {w.dtype} x {w.numel()} on {w.device}")
    pw = s.pos_weights
    if pw is not None:
        if w is not None:
            raise ValueError(f"side {i}: per-id weights and a position-weight source on one side -- one source of weights per side")
        if pw.param.dtype != torch.float32 or not pw.param.is_contiguous() or pw.param.device != dev or pw.param.dim() != 1 or \
                pw.param.numel() < 1:
            raise ValueError(f"side {i}: the position weights must be a contiguous, non-empty float32 vector on the table's device, got "
                             f"{pw.param.dtype} x {tuple(pw.param.shape)} on {pw.param.device}")
        for name, t in (("pw_offset", pw.pw_offset), ("pw_len", pw.pw_len)):
            if t.dtype != torch.int32 or t.numel() != s.K or t.device != dev or not t.is_contiguous():
                raise ValueError(f"side {i}: {name} must be a contiguous int32 tensor of {s.K} elements on the table's device")
    for name, t, dt, n in (("key_row_offset", s.key_row_offset, torch.int64, s.K), ("key_vocab", s.key_vocab, torch.int64, s.K),
                           ("key_pool", s.key_pool, torch.int32, s.K)):
        if t.device != dev or t.dtype != dt or t.numel() != n or not t.is_contiguous():
            raise ValueError(f"side {i}: {name} must be a contiguous {dt} tensor of {n} elements on the table's device")
    if not check_out:          # (embed_bag_rows without an output: nothing is written through the side)
        return
    if s.out.device != dev or s.out.dim() != 2 or s.out.shape[0] != B or s.out.shape[1] != s.K * E:
        raise ValueError(f"side {i}: out must be a [B, K*E] = [{B}, {s.K * E}] view on the table's device")
    assert s.out.stride(1) == 1


def bag_prepare(lengths: Sequence[torch.Tensor], key_pools: Sequence[torch.Tensor], Ks: Sequence[int], B: int, capacities: Sequence[int],
                counts: Optional[Sequence[Optional[torch.Tensor]]] = None, want_inv_len: bool = True):
    """tt_bag_prepare: per side the offsets (int64 [B*K + 1], exclusive prefix sum of the int64 `lengths`) and, for all sides, inv_len
    (f32 per slot: 1 / length for a mean key's non-empty bag, 1 otherwise) -- the values embed_bag_lookup's torch formulas give.  A side
    whose total exceeds its capacity or differs from its count word (int32 [1], device) raises the device error word and gets
    offsets all zero.  Returns (offsets per side, inv_len or None)."""
    dev, n = lengths[0].device, len(lengths)
    arr = (L.BagLengths * n)()
    offs, slots = [], (L.i64 * n)()
    for i, (ln, pool, K, cap) in enumerate(zip(lengths, key_pools, Ks, capacities)):
        if ln.dtype != torch.int64 or not ln.is_contiguous() or ln.numel() != B * K or ln.device != dev:
            raise ValueError(f"side {i}: lengths must be a contiguous int64 tensor of B*K = {B * K} elements on one device")
        if pool.dtype != torch.int32 or pool.numel() != K or pool.device != dev or not pool.is_contiguous():
            raise ValueError(f"side {i}: key_pool must be a contiguous int32 tensor of {K} elements on the lengths' device")
        cnt = None if counts is None else counts[i]
        if cnt is not None and (cnt.dtype != torch.int32 or cnt.numel() != 1 or cnt.device != dev):
            raise ValueError(f"side {i}: the count must be one int32 word on the lengths' device")
        off = torch.empty(B * K + 1, dtype=torch.int64, device=dev)
        offs.append(off)
        slots[i] = B * K
        arr[i] = L.BagLengths(L.ptr(ln), L.ptr(pool), L.ptr(cnt), L.ptr(off), int(cap), K)
    inv_len = torch.empty(sum(B * K for K in Ks), dtype=torch.float32, device=dev) if want_inv_len else None
    lib = L.load()
    ws = torch.empty(lib.tt_bag_prepare_workspace_bytes(slots, n) // 8, dtype=torch.int64, device=dev)
    with _timed("tt_bag_prepare"):
        L.check(lib.tt_bag_prepare(L.ctx(dev), arr, n, B, L.ptr(inv_len), L.ptr(ws), ws.numel() * 8, L.stream(dev)), "tt_bag_prepare")
    return offs, inv_len


def _bag_weight_args(sides: Sequence[BagSide], positions: int, want_rows: bool, dev):
    """(host array of the sides' weight pointers, w_out or None) for the _w entries"""
    arr = (L.vp * len(sides))(*[L.ptr(s.weights) for s in sides])
    return arr, (torch.empty(max(positions, 1), dtype=torch.float32, device=dev) if want_rows else None)


def _bag_source_args(sides: Sequence[BagSide], positions: int, want_rows: bool, dev):
    """(host array of the sides' weight sources, w_out or None) for the _posw entries"""
    arr = (L.BagWeightSrc * len(sides))()
    for i, s in enumerate(sides):
        pw = s.pos_weights
        arr[i] = L.BagWeightSrc(L.ptr(s.weights), None, None, None, 0) if pw is None else \
            L.BagWeightSrc(None, L.ptr(pw.param), L.ptr(pw.pw_offset), L.ptr(pw.pw_len), pw.param.numel())
    return arr, (torch.empty(max(positions, 1), dtype=torch.float32, device=dev) if want_rows else None)


def _embed_bag_lookup_cap(table: torch.Tensor, sides: Sequence[BagSide], B: int, want_rows: bool) -> Optional[BagPlan]:
    """The capacity form of embed_bag_lookup: tt_bag_prepare + tt_embed_bag_fwd_cap.  No launch here depends on how many ids are live."""
    dev, E = table.device, table.shape[1]
    for i, s in enumerate(sides):
        _check_bag_side(i, s, B, E, dev)
        if s.capacity is None or s.capacity != s.ids.numel():
            raise ValueError(f"side {i}: the capacity form takes every side with capacity = ids.numel() (got {s.capacity}, {s.ids.numel()} ids)")
    any_mean = any(s.any_mean for s in sides)
    offs, inv_len = bag_prepare([s.lengths.reshape(-1) for s in sides], [s.key_pool for s in sides], [s.K for s in sides], B,
                                [s.capacity for s in sides], [s.count for s in sides], want_inv_len=want_rows and any_mean)
    arr = (L.BagSide * len(sides))()
    for i, (s, off) in enumerate(zip(sides, offs)):
        arr[i] = L.BagSide(L.ptr(s.ids), L.ptr(off), L.ptr(s.key_row_offset), L.ptr(s.key_vocab), L.ptr(s.key_pool), L.ptr(s.out),
                           s.out.stride(0), s.capacity, s.K, _dt(s.out))
    cap = sum(s.capacity for s in sides)
    idx = torch.empty((2, max(cap, 1)), dtype=torch.int32, device=dev) if want_rows else None      # (the launch writes every position)
    pos_w = None
    with _timed("tt_embed_bag_fwd"):
        if any(s.pos_weights is not None for s in sides):
            sarr, pos_w = _bag_source_args(sides, cap, want_rows, dev)
            L.check(L.load().tt_embed_bag_fwd_cap_posw(L.ctx(dev), L.ptr(table), table.shape[0], E, arr, len(sides), B,
                                                     L.ptr(idx[0]) if want_rows else None, L.ptr(idx[1]) if want_rows else None,
                                                     sarr, L.ptr(pos_w), L.stream(dev)), "tt_embed_bag_fwd_cap_posw")
        elif any(s.weights is not None for s in sides):
            warr, pos_w = _bag_weight_args(sides, cap, want_rows, dev)
            L.check(L.load().tt_embed_bag_fwd_cap_w(L.ctx(dev), L.ptr(table), table.shape[0], E, arr, len(sides), B,
                                                    L.ptr(idx[0]) if want_rows else None, L.ptr(idx[1]) if want_rows else None,
                                                    warr, L.ptr(pos_w), L.stream(dev)), "tt_embed_bag_fwd_cap_w")
        else:
            L.check(L.load().tt_embed_bag_fwd_cap(L.ctx(dev), L.ptr(table), table.shape[0], E, arr, len(sides), B,
                                                  L.ptr(idx[0]) if want_rows else None, L.ptr(idx[1]) if want_rows else None, L.stream(dev)),
                    "tt_embed_bag_fwd_cap")
    if not want_rows:
        return None
    return BagPlan(idx[0, :cap], idx[1, :cap], inv_len, cap, table.shape[0], None if pos_w is None else pos_w[:cap],
                   tuple(s.capacity for s in sides), tuple(offs))


def bag_dedup_plan(bag: BagPlan, table_rows: int) -> DedupPlan:
    """The duplicate-row plan over a pooled lookup's positions: dedup_plan, or for the capacity form tt_dedup_plan_pad (M = the
    capacity; the pad row sorts last and is not counted in n_unique)."""
    if bag.pad_row is None:
        return dedup_plan(bag.rows, table_rows)
    if bag.pad_row != table_rows:
        raise ValueError(f"the bags' pad row is {bag.pad_row}, the table has {table_rows} rows")
    rows = bag.rows
    dev, M = rows.device, rows.numel()
    buf = torch.empty(3 * M + 2, dtype=torch.int32, device=dev)
    plan = DedupPlan(buf[:M], buf[M:2 * M], buf[2 * M:3 * M + 1], buf[3 * M + 1:], M)
    lib = L.load()
    ws = L.workspace(dev, lib.tt_dedup_workspace_bytes(M))
    with _timed("tt_dedup_plan"):
        L.check(lib.tt_dedup_plan_pad(L.ctx(dev), L.ptr(rows), M, table_rows, L.ptr(plan.sorted_src), L.ptr(plan.unique_rows),
                                      L.ptr(plan.seg_offsets), L.ptr(plan.n_unique), L.ptr(ws), ws.numel(), L.stream(dev)),
                "tt_dedup_plan_pad")
    return plan


def embed_bag_lookup(table: torch.Tensor, sides: Sequence[BagSide], B: int, want_rows: bool) -> Optional[BagPlan]:
    """tt_embed_bag_fwd: pooled lookup of every side's bags into side.out.  The offsets are torch.cumsum of the lengths and the
    mean weights 1 / length, both formed on the device: no host synchronisation.  sum(lengths) must equal ids.numel() (ids the
    lengths leave over belong to no bag; lengths that ask for more raise the context's device error word).  Sides with a
    `capacity` take the capacity form (every side then): tt_bag_prepare + tt_embed_bag_fwd_cap, the same pooled bits."""
    dev, E = table.device, table.shape[1]
    if table.dtype != torch.float32 or not table.is_contiguous():
        raise ValueError("the table must be a contiguous float32 [rows, E] tensor")
    if any(s.capacity is not None for s in sides):
        return _embed_bag_lookup_cap(table, sides, B, want_rows)
    arr = (L.BagSide * len(sides))()
    keep, nnz, inv = [], 0, []
    for i, s in enumerate(sides):
        _check_bag_side(i, s, B, E, dev)
        lengths = s.lengths.to(torch.int64).reshape(-1)
        off = torch.zeros(B * s.K + 1, dtype=torch.int64, device=dev)
        torch.cumsum(lengths, 0, out=off[1:])
        keep.append(off)
        arr[i] = L.BagSide(L.ptr(s.ids), L.ptr(off), L.ptr(s.key_row_offset), L.ptr(s.key_vocab), L.ptr(s.key_pool), L.ptr(s.out),
                           s.out.stride(0), s.ids.numel(), s.K, _dt(s.out))
        nnz += s.ids.numel()
        if want_rows:
            lf = lengths.to(torch.float32)
            mean = (s.key_pool != 0).repeat(B) & (lengths > 0)
            one = torch.ones_like(lf)
            inv.append(torch.where(mean, one / lf.clamp(min=1.0), one))        # fl(1 / L): one correctly rounded f32 division
    # zero-filled: a position no bag covers (offsets the kernel refused) then names row 0 / slot 0 instead of stale memory
    idx = torch.zeros((2, max(nnz, 1)), dtype=torch.int32, device=dev) if want_rows else None
    pos_w = None
    with _timed("tt_embed_bag_fwd"):
        if any(s.pos_weights is not None for s in sides):
            sarr, pos_w = _bag_source_args(sides, nnz, want_rows, dev)
            L.check(L.load().tt_embed_bag_fwd_posw(L.ctx(dev), L.ptr(table), table.shape[0], E, arr, len(sides), B,
                                                 L.ptr(idx[0]) if want_rows else None, L.ptr(idx[1]) if want_rows else None,
                                                 sarr, L.ptr(pos_w), L.stream(dev)), "tt_embed_bag_fwd_posw")
        elif any(s.weights is not None for s in sides):
            warr, pos_w = _bag_weight_args(sides, nnz, want_rows, dev)
            L.check(L.load().tt_embed_bag_fwd_w(L.ctx(dev), L.ptr(table), table.shape[0], E, arr, len(sides), B,
                                                L.ptr(idx[0]) if want_rows else None, L.ptr(idx[1]) if want_rows else None,
                                                warr, L.ptr(pos_w), L.stream(dev)), "tt_embed_bag_fwd_w")
        else:
            L.check(L.load().tt_embed_bag_fwd(L.ctx(dev), L.ptr(table), table.shape[0], E, arr, len(sides), B,
                                              L.ptr(idx[0]) if want_rows else None, L.ptr(idx[1]) if want_rows else None, L.stream(dev)),
                    "tt_embed_bag_fwd")
    if not want_rows:
        return None
    inv_len = torch.cat(inv) if any(s.any_mean for s in sides) else None
    return BagPlan(idx[0, :nnz], idx[1, :nnz], inv_len, nnz, None, None if pos_w is None else pos_w[:nnz],
                   tuple(s.ids.numel() for s in sides), tuple(keep))


_UNIT_BAGS: dict = {}


def bag_side_from_lookup(side: LookupSide, B: int) -> BagSide:
    """A plain side as sum bags of length one (a bag of one id is a bit-exact copy of its row in the pooled lookup): what lets a
    plain tower ride along when the other tower pools across the sharded exchange.  The constant lengths / modes are cached."""
    dev = side.ids.device
    key = (str(dev), B, side.K)
    c = _UNIT_BAGS.get(key)
    if c is None:
        c = _UNIT_BAGS[key] = (torch.ones(B * side.K, dtype=torch.int64, device=dev), torch.zeros(side.K, dtype=torch.int32, device=dev))
    return BagSide(side.ids, c[0], side.key_row_offset, side.key_vocab, c[1], side.out, side.K, any_mean=False)


def embed_bag_rows(sides: Sequence[BagSide], B: int, table_rows: int) -> BagPlan:
    """tt_embed_bag_rows[_w]: the plan embed_bag_lookup(..., want_rows=True) returns for these sides -- rows, bag_of, inv_len, nnz, pos_w,
    side_nnz, offsets, bit for bit -- without a table: no row is read and no side's `out` written (it may be None; one that is given
    is checked as the lookup checks it, against E = its width / K).  table_rows: the GLOBAL row count of the row space the sides'
    key_row_offset live in.  What a rank of the row-wise sharded step runs before it routes the rows to their owners.  Offsets and
    inv_len are the lookup's torch formulas: no host synchronisation.  Position-weight sources and the capacity form: ValueError."""
    if not sides:
        raise ValueError("embed_bag_rows: no sides")
    dev = sides[0].ids.device
    if not (1 <= int(table_rows) <= 2 ** 31 - 1):
        raise ValueError(f"embed_bag_rows: table_rows must lie in [1, 2^31), got {table_rows}")
    arr = (L.BagSide * len(sides))()
    keep, nnz, inv = [], 0, []
    for i, s in enumerate(sides):
        if s.pos_weights is not None:
            raise ValueError(f"side {i}: embed_bag_rows takes no position-weight source (the sharded step does not carry learned position "
                             "weights across the exchange)")
        if s.capacity is not None:
            raise ValueError(f"side {i}: embed_bag_rows has no capacity form")
        _check_bag_side(i, s, B, s.out.shape[1] // max(s.K, 1) if s.out is not None and s.out.dim() == 2 else 0, dev,
                        check_out=s.out is not None)
        lengths = s.lengths.to(torch.int64).reshape(-1)
        off = torch.zeros(B * s.K + 1, dtype=torch.int64, device=dev)
        torch.cumsum(lengths, 0, out=off[1:])
        keep.append(off)
        arr[i] = L.BagSide(L.ptr(s.ids), L.ptr(off), L.ptr(s.key_row_offset), L.ptr(s.key_vocab), L.ptr(s.key_pool), None, 0,
                           s.ids.numel(), s.K, TT_F32)
        nnz += s.ids.numel()
        lf = lengths.to(torch.float32)
        mean = (s.key_pool != 0).repeat(B) & (lengths > 0)
        one = torch.ones_like(lf)
        inv.append(torch.where(mean, one / lf.clamp(min=1.0), one))
    idx = torch.zeros((2, max(nnz, 1)), dtype=torch.int32, device=dev)
    pos_w = None
    with _timed("tt_embed_bag_rows"):
        if any(s.weights is not None for s in sides):
            warr, pos_w = _bag_weight_args(sides, nnz, True, dev)
            L.check(L.load().tt_embed_bag_rows_w(L.ctx(dev), int(table_rows), arr, len(sides), B, L.ptr(idx[0]), L.ptr(idx[1]), warr,
                                                 L.ptr(pos_w), L.stream(dev)), "tt_embed_bag_rows_w")
        else:
            L.check(L.load().tt_embed_bag_rows(L.ctx(dev), int(table_rows), arr, len(sides), B, L.ptr(idx[0]), L.ptr(idx[1]),
                                               L.stream(dev)), "tt_embed_bag_rows")
    inv_len = torch.cat(inv) if any(s.any_mean for s in sides) else None
    return BagPlan(idx[0, :nnz], idx[1, :nnz], inv_len, nnz, None, None if pos_w is None else pos_w[:nnz],
                   tuple(s.ids.numel() for s in sides), tuple(keep))


def embed_bag_grad(plan: DedupPlan, bag: BagPlan, srcs: Sequence[tuple], B: int, E: int, mode: int, out: torch.Tensor):
    """tt_embed_bag_grad_bwd.  plan: dedup_plan(bag.rows, table_rows) (M = nnz); srcs: [(d_out 2-D view [B, K*E], K)] in the
    sides' order; mode: TT_GRAD_SPARSE / TT_GRAD_DENSE_SET / TT_GRAD_DENSE_ACC."""
    dev = out.device
    if plan.M != bag.nnz:
        raise ValueError(f"the plan covers {plan.M} positions, the bags {bag.nnz}")
    slots = sum(B * K for _, K in srcs)
    if bag.inv_len is not None and (bag.inv_len.numel() != slots or bag.inv_len.dtype != torch.float32 or bag.inv_len.device != dev):
        raise ValueError(f"inv_len must hold one float32 per slot ({slots}) on the output's device")
    pw = bag.pos_w
    if pw is not None and (pw.numel() != bag.nnz or pw.dtype != torch.float32 or pw.device != dev or not pw.is_contiguous()):
        raise ValueError(f"pos_w must hold one float32 per position ({bag.nnz}) on the output's device")
    if out.dim() != 2 or out.shape[1] != E or out.dtype != torch.float32 or not out.is_contiguous() or \
            (mode == TT_GRAD_SPARSE and out.shape[0] < max(bag.nnz, 1)):
        raise ValueError("out must be a contiguous float32 [rows, E] tensor (sparse mode: room for nnz rows)")
    for d, K in srcs:
        if d.device != dev or d.dim() != 2 or d.shape[0] != B or d.shape[1] != K * E:
            raise ValueError(f"every source must be a [B, K*E] view on the output's device, got {tuple(d.shape)} for K={K}")
    arr = (L.GradSrc * len(srcs))()
    for i, (d, K) in enumerate(srcs):
        assert d.stride(1) == 1
        arr[i] = L.GradSrc(L.ptr(d), d.stride(0), K, _dt(d))
    lib = L.load()
    ws = L.workspace(dev, lib.tt_embed_bag_grad_workspace_bytes(bag.nnz, E))
    with _timed("tt_embed_bag_grad_bwd"):
        if pw is not None:
            L.check(lib.tt_embed_bag_grad_bwd_w(L.ctx(dev), arr, len(srcs), B, E, L.ptr(bag.bag_of), L.ptr(bag.inv_len), L.ptr(pw),
                                                L.ptr(plan.sorted_src), L.ptr(plan.seg_offsets), L.ptr(plan.unique_rows), L.ptr(plan.n_unique),
                                                bag.nnz, mode, L.ptr(out), L.ptr(ws), ws.numel(), L.stream(dev)), "tt_embed_bag_grad_bwd_w")
            return
        L.check(lib.tt_embed_bag_grad_bwd(L.ctx(dev), arr, len(srcs), B, E, L.ptr(bag.bag_of), L.ptr(bag.inv_len), L.ptr(plan.sorted_src),
                                          L.ptr(plan.seg_offsets), L.ptr(plan.unique_rows), L.ptr(plan.n_unique), bag.nnz, mode,
                                          L.ptr(out), L.ptr(ws), ws.numel(), L.stream(dev)), "tt_embed_bag_grad_bwd")


def bag_weight_grad(table: torch.Tensor, bag: BagPlan, srcs: Sequence[tuple], B: int, want: Sequence[bool]) -> List[Optional[torch.Tensor]]:
    """tt_embed_bag_weight_grad: the gradient for the per-id weights of a pooled lookup, per side f32 [side positions] (None where
    `want` is False: nothing of such a side is read or written).  g[p] = c * <d_out[slot of p], table[row of p]>, c the mean
    weight of the slot (bag.inv_len) or 1; 0.0 where no bag covers p.  bag: the plan of embed_bag_lookup, plain or capacity form;
    srcs: [(d_out 2-D view [B, K*E], K)] in the sides' order, as embed_bag_grad takes them."""
    dev, E = table.device, table.shape[1]
    if table.dtype != torch.float32 or not table.is_contiguous() or table.dim() != 2:
        raise ValueError("the table must be a contiguous float32 [rows, E] tensor")
    side_nnz = bag.side_nnz if bag.side_nnz is not None else (bag.nnz,)
    if len(srcs) != len(side_nnz) or len(want) != len(srcs) or sum(side_nnz) != bag.nnz:
        raise ValueError(f"{len(srcs)} sources and {len(want)} requests for a plan of {len(side_nnz)} sides ({sum(side_nnz)} of {bag.nnz} positions)")
    for name, t in (("rows", bag.rows), ("bag_of", bag.bag_of)):
        if t.dtype != torch.int32 or t.numel() != bag.nnz or t.device != dev or not t.is_contiguous():
            raise ValueError(f"the plan's {name} must be a contiguous int32 tensor of nnz = {bag.nnz} elements on the table's device")
    if bag.pad_row is not None and bag.pad_row != table.shape[0]:
        raise ValueError(f"the bags' pad row is {bag.pad_row}, the table has {table.shape[0]} rows")
    slots = sum(B * K for _, K in srcs)
    if bag.inv_len is not None and (bag.inv_len.numel() != slots or bag.inv_len.dtype != torch.float32 or bag.inv_len.device != dev):
        raise ValueError(f"inv_len must hold one float32 per slot ({slots}) on the table's device")
    arr = (L.GradSrc * len(srcs))()
    for i, (d, K) in enumerate(srcs):
        if not want[i]:
            arr[i] = L.GradSrc(None, 0, K, TT_F32)
            continue
        if d.device != dev or d.dim() != 2 or d.shape[0] != B or d.shape[1] != K * E:
            raise ValueError(f"every source must be a [B, K*E] view on the table's device, got {tuple(d.shape)} for K={K}")
        assert d.stride(1) == 1
        arr[i] = L.GradSrc(L.ptr(d), d.stride(0), K, _dt(d))
    outs = [torch.empty(max(n, 1), dtype=torch.float32, device=dev)[:n] if w else None for n, w in zip(side_nnz, want)]
    if not any(want):
        return outs
    nn_arr = (L.i64 * len(srcs))(*[int(n) for n in side_nnz])
    garr = (L.vp * len(srcs))(*[L.ptr(o) for o in outs])
    with _timed("tt_embed_bag_weight_grad"):
        L.check(L.load().tt_embed_bag_weight_grad(L.ctx(dev), L.ptr(table), table.shape[0], E, arr, len(srcs), B, L.ptr(bag.rows),
                                                  L.ptr(bag.bag_of), L.ptr(bag.inv_len), nn_arr, garr, L.stream(dev)),
                "tt_embed_bag_weight_grad")
    return outs


@dataclass
class PosWeightSide:
    lengths: torch.Tensor         # int64 [B*K] (device): length of bag (b, k)
    pw_offset: torch.Tensor       # int32 [K] (device): first element of key k in the parameter, -1: the key has no position weights
    pw_len: torch.Tensor          # int32 [K] (device): max_len of key k
    nnz: int                      # ids of the side (sum(lengths), or more: the rest belongs to no bag)
    K: int
    offsets: Optional[torch.Tensor] = None   # int64 [B*K + 1]: formed from the lengths on first use, kept for the backward


def _pos_weight_sides(param: torch.Tensor, sides: Sequence[PosWeightSide], B: int, bufs: Sequence[Optional[torch.Tensor]]):
    dev = param.device
    if param.dtype != torch.float32 or not param.is_contiguous() or param.dim() != 1 or param.numel() < 1:
        raise ValueError("the position weights must be a contiguous, non-empty float32 vector")
    arr = (L.BagPwSide * len(sides))()
    for i, (s, w) in enumerate(zip(sides, bufs)):
        if s.lengths.dtype != torch.int64 or s.lengths.numel() != B * s.K or s.lengths.device != dev:
            raise ValueError(f"side {i}: {s.lengths.numel()} int64 bag lengths for B={B}, K={s.K} (on the parameter's device)")
        for name, t in (("pw_offset", s.pw_offset), ("pw_len", s.pw_len)):
            if t.dtype != torch.int32 or t.numel() != s.K or t.device != dev or not t.is_contiguous():
                raise ValueError(f"side {i}: {name} must be a contiguous int32 tensor of {s.K} elements on the parameter's device")
        if w is not None and (w.dtype != torch.float32 or w.numel() != s.nnz or w.device != dev or not w.is_contiguous()):
            raise ValueError(f"side {i}: one contiguous float32 per id ({s.nnz}) on the parameter's device")
        if s.offsets is None:
            s.offsets = torch.zeros(B * s.K + 1, dtype=torch.int64, device=dev)
            torch.cumsum(s.lengths.reshape(-1), 0, out=s.offsets[1:])
        arr[i] = L.BagPwSide(L.ptr(s.offsets), L.ptr(s.pw_offset), L.ptr(s.pw_len), L.ptr(w), s.nnz, s.K, 0)
    return arr


def bag_position_weights(param: torch.Tensor, sides: Sequence[PosWeightSide], B: int) -> List[torch.Tensor]:
    """tt_bag_position_weights_fwd: per side the f32 weight of every id, w[p] = param[pw_offset[k] + min(j, pw_len[k] - 1)] for
    position j of bag (b, k) -- a copy, bit for bit; 1.0 for a key without position weights and for ids no bag covers.  Positions
    at or beyond a key's max_len share its last weight."""
    dev = param.device
    outs = [torch.empty(max(s.nnz, 1), dtype=torch.float32, device=dev)[:s.nnz] for s in sides]
    arr = _pos_weight_sides(param, sides, B, outs)
    with _timed("tt_bag_position_weights_fwd"):
        L.check(L.load().tt_bag_position_weights_fwd(L.ctx(dev), L.ptr(param), param.numel(), arr, len(sides), B, L.stream(dev)),
                "tt_bag_position_weights_fwd")
    return outs


def bag_position_weights_bwd(param: torch.Tensor, sides: Sequence[PosWeightSide], B: int, gs: Sequence[Optional[torch.Tensor]]) -> torch.Tensor:
    """tt_bag_position_weights_bwd: the gradient of `param` (f32, its shape) from the per-id gradients gs (per side f32 [nnz], None: the
    side contributes nothing): each element sums the ids that read it, in an order the shapes alone fix; 0 where nobody reads."""
    dev = param.device
    arr = _pos_weight_sides(param, sides, B, gs)
    out = torch.empty_like(param)
    with _timed("tt_bag_position_weights_bwd"):
        L.check(L.load().tt_bag_position_weights_bwd(L.ctx(dev), L.ptr(out), param.numel(), arr, len(sides), B, L.stream(dev)),
                "tt_bag_position_weights_bwd")
    return out


# ---------------------------------------------------------------------------------------------- Adam
def adam_dense(p, g, m, v, step, lr, b1, b2, eps, wd, hp_dev=None):
    dev = p.device
    with _timed("tt_adam_dense_step"):
        L.check(L.load().tt_adam_dense_step(L.ctx(dev), L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), p.numel(), step, lr, b1, b2,
                                            eps, wd, L.ptr(hp_dev), L.stream(dev)), "tt_adam_dense_step")


def _adam_tensors(items):
    """items: [(p, g, m, v)] float32 contiguous tensors on one device -> the tt_adam_tensor array of the optimiser entries."""
    arr = (L.AdamTensor * len(items))()
    for i, (p, g, m, v) in enumerate(items):
        arr[i] = L.AdamTensor(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel())
    return arr


def _fused_step(who, entry, head, plan: "DedupPlan", grad_rows, tail):
    """One fused optimiser call `entry`(*head, *tail) -- or, when the plan's long-row finish is deferred, `entry`_finish with the
    plan's (seg_offsets, workspace, workspace_bytes) between head and tail, which completes grad_rows on the way."""
    fin = ()
    if plan.finish_deferred is not None:
        if plan.finish_deferred.data_ptr() != grad_rows.data_ptr():
            raise RuntimeError(f"{who}: the plan's deferred gradient is not the one handed to the optimiser")
        ws = plan.grad_ws[0]
        fin = (L.ptr(plan.seg_offsets), L.ptr(ws), ws.numel())
    name = entry + "_finish" if fin else entry
    with _timed(entry):
        L.check(getattr(L.load(), name)(*head, *fin, *tail), name)
    plan.finish_deferred = None


def adam_multi(items, step, lr, b1, b2, eps, wd, hp_dev=None):
    """items: [(p, g, m, v)] float32 contiguous tensors on one device."""
    if not items:
        return
    dev = items[0][0].device
    with _timed("tt_adam_multi_step"):
        L.check(L.load().tt_adam_multi_step(L.ctx(dev), _adam_tensors(items), len(items), step, lr, b1, b2, eps, wd, L.ptr(hp_dev),
                                            L.stream(dev)), "tt_adam_multi_step")


def adam_sparse(table, m, v, plan: DedupPlan, grad_rows, step, lr, b1, b2, eps, wd, hp_dev=None):
    dev = table.device
    embed_grad_finish(plan)
    with _timed("tt_sparse_adam_step"):
        L.check(L.load().tt_sparse_adam_step(L.ctx(dev), L.ptr(table), L.ptr(m), L.ptr(v), table.shape[0], table.shape[1],
                                             L.ptr(plan.unique_rows), L.ptr(grad_rows), L.ptr(plan.n_unique), plan.M, step,
                                             lr, b1, b2, eps, wd, L.ptr(hp_dev), L.stream(dev)), "tt_sparse_adam_step")


def adam_fused(items, table, m, v, plan: DedupPlan, grad_rows, step, lr, b1, b2, eps, wd, hp_dev=None):
    """adam_multi(items) + adam_sparse(table rows) with one set of hyper-parameters, one launch."""
    dev = table.device
    head = (L.ctx(dev), _adam_tensors(items), len(items), L.ptr(table), L.ptr(m), L.ptr(v), table.shape[0], table.shape[1],
            L.ptr(plan.unique_rows), L.ptr(grad_rows), L.ptr(plan.n_unique), plan.M)
    tail = (step, lr, b1, b2, eps, wd, L.ptr(hp_dev), L.stream(dev))
    _fused_step("adam_fused", "tt_adam_fused_step", head, plan, grad_rows, tail)


# ---------------------------------------------------------------------------------------------- row-wise Adagrad (tables)
# hp_dev: NULL or device floats [lr, eps, weight_decay] read instead of the host scalars (graph replay)
def rowwise_adagrad_sparse(table, acc, plan: DedupPlan, grad_rows, lr, eps, wd, hp_dev=None):
    """Row-wise Adagrad over the plan's rows of `table` [R, E]; acc: the [R] per-row accumulator."""
    dev = table.device
    embed_grad_finish(plan)
    with _timed("tt_rowwise_adagrad_sparse_step"):
        L.check(L.load().tt_rowwise_adagrad_sparse_step(L.ctx(dev), L.ptr(table), L.ptr(acc), table.shape[0], table.shape[1],
                                                        L.ptr(plan.unique_rows), L.ptr(grad_rows), L.ptr(plan.n_unique), plan.M,
                                                        lr, eps, wd, L.ptr(hp_dev), L.stream(dev)), "tt_rowwise_adagrad_sparse_step")


def rowwise_adagrad_dense(table, acc, grad, lr, eps, wd, hp_dev=None):
    """Row-wise Adagrad over every row of `table` [R, E] with a dense [R, E] gradient."""
    dev = table.device
    with _timed("tt_rowwise_adagrad_dense_step"):
        L.check(L.load().tt_rowwise_adagrad_dense_step(L.ctx(dev), L.ptr(table), L.ptr(acc), L.ptr(grad), table.shape[0], table.shape[1],
                                                       lr, eps, wd, L.ptr(hp_dev), L.stream(dev)), "tt_rowwise_adagrad_dense_step")


def adam_rowwise_adagrad_fused(items, step, lr, b1, b2, eps, wd, hp_dev, table, acc, plan: DedupPlan, grad_rows, t_lr, t_eps, t_wd,
                               t_hp_dev=None):
    """adam_multi(items) with the towers' hyper-parameters + rowwise_adagrad_sparse(table rows) with the table's, one launch."""
    dev = table.device
    head = (L.ctx(dev), _adam_tensors(items), len(items), step, lr, b1, b2, eps, wd, L.ptr(hp_dev), L.ptr(table), L.ptr(acc),
            table.shape[0], table.shape[1], L.ptr(plan.unique_rows), L.ptr(grad_rows), L.ptr(plan.n_unique), plan.M)
    tail = (t_lr, t_eps, t_wd, L.ptr(t_hp_dev), L.stream(dev))
    _fused_step("adam_rowwise_adagrad_fused", "tt_adam_rowwise_adagrad_fused_step", head, plan, grad_rows, tail)


# ---------------------------------------------------------------------------------------------- tower MLP
def _fill(arr, tensors):
    for i, t in enumerate(tensors):
        arr[i] = t.data_ptr() if t is not None else 0


def tower_params_struct(din, h0, kcat_e, hidden, d_out, w_proj, b_proj, ws, bs, bn_w, bn_b, bn_rm, bn_rv, w_out, b_out,
                        bn_nbt=(), compute_dtype=TT_F32, x_dtype=TT_F32, dx_dtype=TT_F32, flags=0, w_proj_bf16=None, w_bf16=()):
    if len(hidden) > L.TT_MAX_HIDDEN:
        raise ValueError(f"at most {L.TT_MAX_HIDDEN} hidden blocks per tower are supported")
    p = L.TowerParams()
    p.din, p.h0, p.kcat_e, p.n_hidden, p.d_out = din, h0, kcat_e, len(hidden), d_out
    for i, h in enumerate(hidden):
        p.hidden[i] = h
    p.w_proj, p.b_proj, p.w_out, p.b_out = w_proj.data_ptr(), b_proj.data_ptr(), w_out.data_ptr(), b_out.data_ptr()
    _fill(p.w, ws); _fill(p.b, bs); _fill(p.bn_w, bn_w); _fill(p.bn_b, bn_b); _fill(p.bn_rm, bn_rm); _fill(p.bn_rv, bn_rv)
    _fill(p.bn_nbt, bn_nbt)
    p.compute_dtype, p.x_dtype, p.dx_dtype, p.flags = compute_dtype, x_dtype, dx_dtype, flags
    p.w_proj_bf16 = w_proj_bf16.data_ptr() if w_proj_bf16 is not None else 0      # bf16 shadows (tt_tower_params.w_proj_bf16 / w_bf16)
    _fill(p.w_bf16, w_bf16)
    return p


def adam_hparams(step, lr, b1, b2, eps, wd):
    out = (L.f32 * 6)()
    L.load().tt_adam_hparams(step, lr, b1, b2, eps, wd, C.byref(out))
    return list(out)


def tower_workspace(params, B, dev):
    nb = L.load().tt_tower_workspace_bytes(C.byref(params), B)
    return L.workspace(dev, nb)


def tower_fwd(params, acts, B, train, p_drop, seed, dev, seed_dev=None):
    ws = tower_workspace(params, B, dev)
    with _timed("tt_tower_mlp_fwd"):
        L.check(L.load().tt_tower_mlp_fwd(L.ctx(dev), C.byref(params), C.byref(acts), B, int(train), p_drop, seed, L.ptr(seed_dev), L.ptr(ws),
                                          ws.numel(), L.stream(dev)), "tt_tower_mlp_fwd")


def tower_bwd(params, acts, d_emb, grads, B, train, p_drop, seed, dev, seed_dev=None):
    ws = tower_workspace(params, B, dev)
    with _timed("tt_tower_mlp_bwd"):
        L.check(L.load().tt_tower_mlp_bwd(L.ctx(dev), C.byref(params), C.byref(acts), L.ptr(d_emb), C.byref(grads), B,
                                          int(train), p_drop, seed, L.ptr(seed_dev), L.ptr(ws), ws.numel(), L.stream(dev)), "tt_tower_mlp_bwd")


def _tower_workspaces(params_list, B, dev):
    """One growable buffer per (device, stream), carved into per-tower regions."""
    lib = L.load()
    sizes = [(lib.tt_tower_workspace_bytes(C.byref(p), B) + 255) // 256 * 256 for p in params_list]
    buf = L.workspace(dev, sum(sizes))
    ptrs, off = (L.vp * len(sizes))(), 0
    for i, z in enumerate(sizes):
        ptrs[i] = buf.data_ptr() + off
        off += z
    return buf, ptrs, (L.sz * len(sizes))(*sizes)


def towers_fwd(params_list, acts_list, B, train, p_drop, seed, dev, seed_dev=None):
    """All towers in one launch per layer step (tt_towers_mlp_fwd)."""
    n = len(params_list)
    _, wptrs, wsizes = _tower_workspaces(params_list, B, dev)
    P = (C.POINTER(L.TowerParams) * n)(*[C.pointer(p) for p in params_list])
    A = (C.POINTER(L.TowerActs) * n)(*[C.pointer(a) for a in acts_list])
    with _timed("tt_towers_mlp_fwd"):
        L.check(L.load().tt_towers_mlp_fwd(L.ctx(dev), n, P, A, B, int(train), p_drop, seed, L.ptr(seed_dev), wptrs, wsizes,
                                           L.stream(dev)), "tt_towers_mlp_fwd")


def towers_fwd_gathers(params_list, acts_list, B, train) -> bool:
    """tt_towers_fwd_gathers: will towers_fwd / tower_fwd on these arguments (gather fields filled) gather the embedding rows itself?"""
    n = len(params_list)
    P = (C.POINTER(L.TowerParams) * n)(*[C.pointer(p) for p in params_list])
    A = (C.POINTER(L.TowerActs) * n)(*[C.pointer(a) for a in acts_list])
    return bool(L.load().tt_towers_fwd_gathers(n, P, A, B, int(train)))


def towers_bwd(params_list, acts_list, d_embs, grads_list, B, train, p_drop, seed, dev, seed_dev=None):
    n = len(params_list)
    _, wptrs, wsizes = _tower_workspaces(params_list, B, dev)
    P = (C.POINTER(L.TowerParams) * n)(*[C.pointer(p) for p in params_list])
    A = (C.POINTER(L.TowerActs) * n)(*[C.pointer(a) for a in acts_list])
    G = (C.POINTER(L.TowerGrads) * n)(*[C.pointer(g) for g in grads_list])
    D = (L.vp * n)(*[d.data_ptr() for d in d_embs])
    with _timed("tt_towers_mlp_bwd"):
        L.check(L.load().tt_towers_mlp_bwd(L.ctx(dev), n, P, A, D, G, B, int(train), p_drop, seed, L.ptr(seed_dev), wptrs, wsizes,
                                           L.stream(dev)), "tt_towers_mlp_bwd")


# ---------------------------------------------------------------------------------------------- score / loss
# logQ sampling-bias correction (the *_lq entries of include/twotower.h): the score wrappers take the log sampling
# probabilities as optional arguments and call the _lq entry when they are given
LQ_MAX_TWO_INV_T = 40.0      # the *_lq entries support 2/T <= 40 (T >= 0.05)


def _lq_vec(lq, B, dev, name):
    """f32 [B] log sampling probabilities, contiguous on `dev` (validated: no device sync)"""
    if not isinstance(lq, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor, got {type(lq).__name__}")
    if lq.dtype != torch.float32:
        raise TypeError(f"{name} must be float32, got {lq.dtype}")
    if lq.dim() != 1 or lq.shape[0] != B:
        raise ValueError(f"{name} must have shape [{B}], got {list(lq.shape)}")
    if lq.device != dev:
        raise ValueError(f"{name} is on {lq.device}, the scores on {dev}")
    return lq.contiguous()


def _lq_check_t(inv_t):
    if 2.0 * abs(inv_t) > LQ_MAX_TWO_INV_T:
        raise ValueError(f"logQ correction needs 2/T <= {LQ_MAX_TWO_INV_T:g} (T >= 0.05), got 1/T = {inv_t:g}")


def _lq_pair(a, b, Ra, Rb, dev, names):
    """() without logQ, else the two validated vectors (the caller holds them for the duration of the call)"""
    return () if a is None else (_lq_vec(a, Ra, dev, names[0]), _lq_vec(b, Rb, dev, names[1]))


# repeated-entity mask (the *_mask entries of include/twotower.h): the score wrappers take the rows' notice / company ids as
# optional arguments `ent=(ent_n, ent_c)` and call the _mask entry when they are given
def _ent_vec(e, B, dev, name):
    """int32 [B] entity ids on `dev` (validated: no device sync)"""
    if not isinstance(e, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor, got {type(e).__name__}")
    if e.dtype != torch.int32:
        raise TypeError(f"{name} must be int32, got {e.dtype}")
    if e.dim() != 1 or e.shape[0] != B:
        raise ValueError(f"{name} must have shape [{B}], got {list(e.shape)}")
    if e.device != dev:
        raise ValueError(f"{name} is on {e.device}, the scores on {dev}")
    return e


def score_mask_ids(ent_n, ent_c, B, dev):
    """(ent_n, ent_c) as the *_mask entries read them: ONE int32 [2, round_up(B, 64)] array (rows 16-byte aligned, the entries past
    B zero and ignored); a side given as None counts as all-distinct (its row index)."""
    Bp = (B + 63) // 64 * 64
    if B == Bp and ent_n is not None and ent_c is not None:          # whole tiles: the arrays as they are (no copy, no launch)
        en, ec = _ent_vec(ent_n, B, dev, "ent_n"), _ent_vec(ent_c, B, dev, "ent_c")
        if en.is_contiguous() and ec.is_contiguous() and en.data_ptr() % 16 == 0 and ec.data_ptr() % 16 == 0:
            return en, ec
    out = torch.zeros((2, Bp), dtype=torch.int32, device=dev)
    for k, (e, name) in enumerate(((ent_n, "ent_n"), (ent_c, "ent_c"))):
        if e is None:
            out[k, :B] = torch.arange(B, dtype=torch.int32, device=dev)
        else:
            out[k, :B] = _ent_vec(e, B, dev, name)
    return out[0], out[1]


def _mask_args(ent, lq, n_lq):
    """the _mask entries' (ent_n, ent_c, lq...) arguments: NULL where the call has no logQ vectors"""
    return (L.ptr(ent[0]), L.ptr(ent[1])) + (tuple(map(L.ptr, lq)) if lq else (None,) * n_lq)


# per-pair sample weights (the *_pw entries of include/twotower.h): the score wrappers take the normalised weights `pw` =
# score_pair_weights(w, B, dev) as an optional argument and call the _pw entry when it is given; ent / lq combine with it
def score_pair_weights(w, B, dev):
    """g = w' B / sum(w') as the *_pw entries read it (tt_score_prepare_pw, one launch): f32 [round_up(B, 64)], 0 past B; w' = the raw
    weights w (f32 [B] on `dev`) with every entry that is not a positive finite number set to 0; all 0 when the sum is 0."""
    if not isinstance(w, torch.Tensor):
        raise TypeError(f"pair_weight must be a torch.Tensor, got {type(w).__name__}")
    if w.dtype != torch.float32:
        raise TypeError(f"pair_weight must be float32, got {w.dtype}")
    if w.dim() != 1 or w.shape[0] != B:
        raise ValueError(f"pair_weight must have shape [{B}], got {list(w.shape)}")
    if w.device != torch.device(dev):
        raise ValueError(f"pair_weight is on {w.device}, the scores on {dev}")
    w = w.contiguous()
    g = torch.empty((B + 63) // 64 * 64, dtype=torch.float32, device=w.device)
    with _timed("tt_score_prepare_pw"):
        L.check(L.load().tt_score_prepare_pw(L.ctx(w.device), L.ptr(w), B, L.ptr(g), L.stream(w.device)), "tt_score_prepare_pw")
    return g


def _pw_args(pw, ent, lq, n_lq):
    """the _pw entries' (g, ent_n, ent_c, lq...) arguments: NULL where the call has no ids / no logQ vectors"""
    return (L.ptr(pw),) + ((L.ptr(ent[0]), L.ptr(ent[1])) if ent is not None else (None, None)) \
        + (tuple(map(L.ptr, lq)) if lq else (None,) * n_lq)


def score_dir_fwd(A, Bm, inv_t, shift, diag_offset=0, want_sumscore=True, lq_b=None, ent=None):
    """lq_b: the B rows' log sampling probabilities [Rb] (tt_score_dir_fwd_lq).
    ent: (ent_n, ent_c) from score_mask_ids -- the repeated-entity mask (tt_score_dir_fwd_mask, square problems)."""
    dev, Ra, Rb, D = A.device, A.shape[0], Bm.shape[0], A.shape[1]
    lq = () if lq_b is None else (_lq_vec(lq_b, Rb, dev, "lq_b"),)
    f = torch.empty((3, Ra), dtype=torch.float32, device=dev)       # sumexp, diag, sumscore
    rank = torch.empty(Ra, dtype=torch.int32, device=dev)
    if ent is not None:
        name = "tt_score_dir_fwd_mask"
        with _timed(name):
            L.check(getattr(L.load(), name)(L.ctx(dev), L.ptr(A), L.ptr(Bm), Ra, Rb, D, inv_t, shift, diag_offset, *_mask_args(ent, lq, 1),
                                            L.ptr(f[0]), L.ptr(f[1]), L.ptr(rank), L.ptr(f[2]) if want_sumscore else None, L.stream(dev)),
                    name)
        return f[0], f[1], rank, f[2]
    name = "tt_score_dir_fwd_lq" if lq else "tt_score_dir_fwd"
    with _timed(name):
        L.check(getattr(L.load(), name)(L.ctx(dev), L.ptr(A), L.ptr(Bm), Ra, Rb, D, inv_t, shift, diag_offset, *map(L.ptr, lq),
                                        L.ptr(f[0]), L.ptr(f[1]), L.ptr(rank), L.ptr(f[2]) if want_sumscore else None, L.stream(dev)),
                name)
    return f[0], f[1], rank, f[2]


def score_loss_finish(B, shift, rowsum, colsum, diag, row_rank, col_rank, sumscore, lq_n=None, lq_c=None, pw=None):
    """Returns (out8, loss): the loss is its own 0-dim tensor so that autograd sees a plain output.
    lq_n / lq_c (both or neither): the corrected positives (tt_score_loss_finish_lq).
    pw: score_pair_weights' g -- the weighted loss (tt_score_loss_finish_pw)."""
    dev = rowsum.device
    lq = _lq_pair(lq_n, lq_c, B, B, dev, ("lq_n", "lq_c"))
    out = torch.empty(8, dtype=torch.float32, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    if pw is not None:
        name = "tt_score_loss_finish_pw"
        with _timed(name):
            L.check(getattr(L.load(), name)(L.ctx(dev), B, shift, L.ptr(pw), *(map(L.ptr, lq) if lq else (None, None)), L.ptr(rowsum),
                                            L.ptr(colsum), L.ptr(diag), L.ptr(row_rank), L.ptr(col_rank), L.ptr(sumscore), L.ptr(out),
                                            L.ptr(loss), L.stream(dev)), name)
        return out, loss
    name = "tt_score_loss_finish_lq" if lq else "tt_score_loss_finish"
    with _timed(name):
        L.check(getattr(L.load(), name)(L.ctx(dev), B, shift, *map(L.ptr, lq), L.ptr(rowsum), L.ptr(colsum), L.ptr(diag),
                                        L.ptr(row_rank), L.ptr(col_rank), L.ptr(sumscore), L.ptr(out), L.ptr(loss), L.stream(dev)),
                name)
    return out, loss


def score_dir_bwd(A, Bm, inv_t, shift, diag_offset, sumexp_a, sumexp_b, d_loss, scale, lq_a=None, lq_b=None, ent=None, pw=None):
    """lq_a / lq_b (both or neither): the log sampling probabilities of the A rows [Ra] and the B rows [Rb] (tt_score_dir_bwd_lq).
    ent: (ent_n, ent_c) from score_mask_ids -- the repeated-entity mask (tt_score_dir_bwd_mask, square problems).
    pw: score_pair_weights' g -- the weighted gradient (tt_score_dir_bwd_pw, square problems; ent / lq optional)."""
    dev, Ra, Rb, D = A.device, A.shape[0], Bm.shape[0], A.shape[1]
    lq = _lq_pair(lq_a, lq_b, Ra, Rb, dev, ("lq_a", "lq_b"))
    dA = torch.empty_like(A)
    if pw is not None:
        name = "tt_score_dir_bwd_pw"
        with _timed(name):
            L.check(getattr(L.load(), name)(L.ctx(dev), L.ptr(A), L.ptr(Bm), Ra, Rb, D, inv_t, shift, diag_offset, *_pw_args(pw, ent, lq, 2),
                                            L.ptr(sumexp_a), L.ptr(sumexp_b), L.ptr(d_loss), scale, L.ptr(dA), L.stream(dev)), name)
        return dA
    if ent is not None:
        name = "tt_score_dir_bwd_mask"
        with _timed(name):
            L.check(getattr(L.load(), name)(L.ctx(dev), L.ptr(A), L.ptr(Bm), Ra, Rb, D, inv_t, shift, diag_offset, *_mask_args(ent, lq, 2),
                                            L.ptr(sumexp_a), L.ptr(sumexp_b), L.ptr(d_loss), scale, L.ptr(dA), L.stream(dev)), name)
        return dA
    name = "tt_score_dir_bwd_lq" if lq else "tt_score_dir_bwd"
    with _timed(name):
        L.check(getattr(L.load(), name)(L.ctx(dev), L.ptr(A), L.ptr(Bm), Ra, Rb, D, inv_t, shift, diag_offset, *map(L.ptr, lq),
                                        L.ptr(sumexp_a), L.ptr(sumexp_b), L.ptr(d_loss), scale, L.ptr(dA), L.stream(dev)), name)
    return dA


def score_pack_bf16(X, scale: float = 1.0):
    """f32 [R, D] -> packed bf16 operand images of scale * X (uint8 buffer)."""
    dev, R, D = X.device, X.shape[0], X.shape[1]
    lib = L.load()
    buf = torch.empty(lib.tt_score_pack_bytes(R, D), dtype=torch.uint8, device=dev)
    with _timed("tt_score_pack_bf16"):
        L.check(lib.tt_score_pack_bf16(L.ctx(dev), L.ptr(X), R, D, scale, L.ptr(buf), L.stream(dev)), "tt_score_pack_bf16")
    return buf


def score_unit_scale(inv_t: float) -> float:
    """inv_t * log2(e) exactly as the library computes it: packing ONE tower's operand images with it lets the score
    kernels drop the exponent's multiply-add (tt_score_fwd_dir.ab_scale)."""
    return float(L.load().tt_score_unit_scale(inv_t))


def score_pack2_bf16(X0, X1, scale0: float = 1.0, scale1: float = 1.0):
    """Both operands of a step in one launch (images of scale * X)."""
    dev, D = X0.device, X0.shape[1]
    lib = L.load()
    b0 = torch.empty(lib.tt_score_pack_bytes(X0.shape[0], D), dtype=torch.uint8, device=dev)
    b1 = torch.empty(lib.tt_score_pack_bytes(X1.shape[0], D), dtype=torch.uint8, device=dev)
    with _timed("tt_score_pack_bf16"):
        L.check(lib.tt_score_pack2_bf16(L.ctx(dev), L.ptr(X0), X0.shape[0], L.ptr(b0), L.ptr(X1), X1.shape[0], L.ptr(b1), D,
                                        scale0, scale1, L.stream(dev)), "tt_score_pack2_bf16")
    return b0, b1


def score_pack2_bf16x3(X0, X1, scale0: float = 1.0, scale1: float = 1.0):
    """Both operands of a step as split-bf16 images [hi | lo] of scale * X (tt_score_pack2_bf16x3): the x3= operands of
    score_fwd_bf16 / score_fwd_sym / score_bwd_bf16."""
    dev, D = X0.device, X0.shape[1]
    lib = L.load()
    b0 = torch.empty(lib.tt_score_pack_x3_bytes(X0.shape[0], D), dtype=torch.uint8, device=dev)
    b1 = torch.empty(lib.tt_score_pack_x3_bytes(X1.shape[0], D), dtype=torch.uint8, device=dev)
    with _timed("tt_score_pack2_bf16x3"):
        L.check(lib.tt_score_pack2_bf16x3(L.ctx(dev), L.ptr(X0), X0.shape[0], L.ptr(b0), L.ptr(X1), X1.shape[0], L.ptr(b1), D,
                                          scale0, scale1, L.stream(dev)), "tt_score_pack2_bf16x3")
    return b0, b1


def score_fwd_bf16(Np, Cp, B, D, inv_t, shift, want_col_rank=True, full_rank=True, scale_n: float = 1.0, with_inv: bool = False,
                   x3: bool = False):
    """Both softmax directions of the square in-batch problem in one launch.  scale_n: the scale Np was packed with.
    with_inv: also return (inv_row, inv_col), the reciprocals score_bwd_bf16 can take instead of computing its own.
    x3: Np / Cp are score_pack2_bf16x3 images (tt_score_fwd_bf16x3)."""
    dev = Np.device
    Bp = (B + 63) // 64 * 64                                           # tt_score_bwd_bf16 reads its per-row arrays a 32-row tile at a time
    f = (torch.empty if B == Bp else torch.ones)((6, Bp), dtype=torch.float32, device=dev)    # rowsum, colsum, diag, sumscore, 1/rowsum', 1/colsum'
    ranks = torch.empty((2, B), dtype=torch.int32, device=dev)
    arr = (L.ScoreFwdDir * 2)()
    rm = 2 if full_rank else 1
    arr[0] = L.ScoreFwdDir(L.ptr(Np), L.ptr(Cp), B, B, 0, L.ptr(f[0]), L.ptr(f[2]), L.ptr(ranks[0]), L.ptr(f[3]), rm, scale_n,
                           L.ptr(f[4]) if with_inv else None)
    arr[1] = L.ScoreFwdDir(L.ptr(Cp), L.ptr(Np), B, B, 0, L.ptr(f[1]), None, L.ptr(ranks[1]) if want_col_rank else None, None, rm, scale_n,
                           L.ptr(f[5]) if with_inv else None)
    name = "tt_score_fwd_bf16x3" if x3 else "tt_score_fwd_bf16"
    with _timed(name):
        L.check(getattr(L.load(), name)(L.ctx(dev), arr, 2, D, inv_t, shift, L.stream(dev)), name)
    out = (f[0][:B], f[1][:B], f[2][:B], ranks[0], ranks[1], f[3][:B])
    return out + ((f[4][:B], f[5][:B]),) if with_inv else out


def score_pack2_fp8(X0, X1, scale0: float = 1.0, scale1: float = 1.0):
    """Both operands of a step as [fp8 rows image | bf16 fragment image] (tt_score_pack2_fp8)."""
    dev, D = X0.device, X0.shape[1]
    lib = L.load()
    b0 = torch.empty(lib.tt_score_pack_fp8_bytes(X0.shape[0], D), dtype=torch.uint8, device=dev)
    b1 = torch.empty(lib.tt_score_pack_fp8_bytes(X1.shape[0], D), dtype=torch.uint8, device=dev)
    with _timed("tt_score_pack2_fp8"):
        L.check(lib.tt_score_pack2_fp8(L.ctx(dev), L.ptr(X0), X0.shape[0], L.ptr(b0), L.ptr(X1), X1.shape[0], L.ptr(b1), D,
                                       scale0, scale1, L.stream(dev)), "tt_score_pack2_fp8")
    return b0, b1


class ScoreTerms(NamedTuple):
    """The optional terms of the in-batch softmax as the score entries take them; None: the term is absent."""
    lq: Optional[tuple] = None        # (lq_n, lq_c) f32 [B]: logQ sampling-bias correction
    ent: Optional[tuple] = None       # score_mask_ids' (ent_n, ent_c): the repeated-entity mask
    pw: Optional[torch.Tensor] = None   # score_pair_weights' g: per-pair sample weights
    extras: Optional[tuple] = None    # (Xp, M, lq_x, ent_x): shared extra negatives -- score_pack_bf16(X), lq_x f32 [M] / score_xneg_ids or None
    plan: Optional[torch.Tensor] = None   # score_cells_plan's plan: masked cells


class SymOut(NamedTuple):
    """What the symmetric forward leaves: inv = (inv_row, inv_col); w = (w_n, w_c) with logQ, w_x [round_up(M, 64)] with extras, else None."""
    rowsum: torch.Tensor
    colsum: torch.Tensor
    diag: torch.Tensor
    row_rank: torch.Tensor
    inv: tuple
    w: Optional[tuple]
    w_x: Optional[torch.Tensor]
    out8: torch.Tensor
    loss: torch.Tensor


_NO_TERMS = ScoreTerms()
_SYM_ENTRY = {"bf16": "tt_score_fwd_sym_bf16", "bf16x3": "tt_score_fwd_sym_bf16x3", "fp8": "tt_score_fwd_sym_fp8"}
_BWD_ENTRY = {"bf16": "tt_score_bwd_bf16", "bf16x3": "tt_score_bwd_bf16x3", "fp8": "tt_score_bwd_fp8"}


def _operands(fp8, x3):
    return "fp8" if fp8 else ("bf16x3" if x3 else "bf16")


def _sym_fwd(Np, Cp, B, D, inv_t, shift, scale_n, want_rank, operands, terms: ScoreTerms) -> SymOut:
    """The symmetric forward of every form (the tt_score_fwd_sym_* entries): operands 'bf16', 'bf16x3' or 'fp8', the packing of Np / Cp."""
    dev = Np.device
    other = operands != "bf16"
    if terms.pw is not None and other:
        raise ValueError("the weighted symmetric forward takes bf16 operands only")
    if terms.lq is not None and operands == "fp8":
        raise ValueError("the logQ-corrected symmetric forward has no fp8 form")
    if terms.ent is not None and other:
        raise ValueError("the masked symmetric forward takes bf16 operands only")
    lq = _lq_pair(*(terms.lq or (None, None)), B, B, dev, ("lq_n", "lq_c"))
    Xp, M, lq_x, ent_x = terms.extras or (None, 0, None, None)
    ent, pw, plan = terms.ent, terms.pw, terms.plan
    if plan is not None:
        if (Xp is None) != (M == 0):
            raise ValueError("masked cells: the extras' image Xp and M >= 1 go together")
        if lq_x is not None and (not lq or Xp is None):
            raise ValueError("masked cells: lq_x needs lq_n / lq_c and the extras")
    elif terms.extras is not None:
        _xneg_check(B, M, ent, ent_x, lq, lq_x)
    if lq and (plan is not None or terms.extras is not None):
        _lq_check_t(inv_t)
    lqx = None if lq_x is None else _lq_vec(lq_x, M, dev, "lq_x")
    Bp, Mp = (B + 63) // 64 * 64, (M + 63) // 64 * 64            # the kernel fills the entries past B (read by tt_score_bwd_bf16)
    f = torch.empty((7 if lq else 5, Bp), dtype=torch.float32, device=dev)    # rowsum, colsum, diag, 1/rowsum', 1/colsum'[, w_n, w_c]
    w_x = torch.empty(Mp, dtype=torch.float32, device=dev) if M else None
    rank = torch.empty(B, dtype=torch.int32, device=dev)
    out8 = torch.empty(8, dtype=torch.float32, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    lib = L.load()
    nbytes = lib.tt_score_fwd_sym_xneg_workspace_bytes(B, M, D) if M else lib.tt_score_fwd_sym_workspace_bytes(B, D)
    if L.riders_deferred(dev, 2):    # the last reduction runs later (inside the towers' backward launch): its partial records must
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)         # outlive the shared scratch's next user
        out8._tt_keep = ws
    else:
        ws = L.workspace(dev, nbytes)
    # the entry of the terms present and its argument order: (name, operands' head, terms before the sums, weights behind them)
    lqp = tuple(map(L.ptr, lq)) or (None, None)
    entp = (L.ptr(ent[0]), L.ptr(ent[1])) if ent is not None else (None, None)
    wp = (L.ptr(f[5]), L.ptr(f[6])) if lq else (None, None)
    head = (L.ptr(Np), L.ptr(Cp), B, D) if Xp is None and plan is None else (L.ptr(Np), L.ptr(Cp), L.ptr(Xp), B, M, D)
    if plan is not None:
        name, pre, wout = "tt_score_fwd_sym_bf16_cells", (L.ptr(plan), int(plan._tt_cap), *lqp, L.ptr(lqx)), wp + (L.ptr(w_x),)
    elif terms.extras is not None:
        name, pre, wout = "tt_score_fwd_sym_bf16_xneg", (*entp, L.ptr(ent_x), *lqp, L.ptr(lqx)), wp + (L.ptr(w_x),)
    elif pw is not None:
        name, pre, wout = "tt_score_fwd_sym_bf16_pw", (L.ptr(pw), *entp, *lqp), wp
    elif ent is not None:
        name, pre, wout = "tt_score_fwd_sym_bf16_mask", (*entp, *lqp), wp
    else:
        name, pre, wout = _SYM_ENTRY[operands] + ("_lq" if lq else ""), (lqp if lq else ()), (wp if lq else ())
    with _timed(name):
        L.check(getattr(lib, name)(L.ctx(dev), *head, inv_t, shift, scale_n, int(want_rank), *pre, L.ptr(f[0]), L.ptr(f[1]), L.ptr(f[3]),
                                   L.ptr(f[4]), *wout, L.ptr(f[2]), L.ptr(rank), L.ptr(out8), L.ptr(loss), L.ptr(ws), ws.numel(),
                                   L.stream(dev)), name)
    return SymOut(f[0][:B], f[1][:B], f[2][:B], rank, (f[3][:B], f[4][:B]), (f[5][:B], f[6][:B]) if lq else None, w_x, out8, loss)


def _lq_terms(lq_n, lq_c):
    return None if lq_n is None else (lq_n, lq_c)


def _sym8(o: SymOut):
    """the documented tuple of score_fwd_sym_lq / _mask / _pw"""
    return o.rowsum, o.colsum, o.diag, o.row_rank, o.inv, o.w, o.out8, o.loss


def _fwd_sym(Np, Cp, B, D, inv_t, shift, scale_n: float = 1.0, want_rank: bool = True, fp8: bool = False, x3: bool = False,
             lq_n=None, lq_c=None, ent=None, pw=None):
    """_sym_fwd by flags: (rowsum, colsum, diag, row_rank, (inv_row, inv_col), out8, loss, w)"""
    o = _sym_fwd(Np, Cp, B, D, inv_t, shift, scale_n, want_rank, _operands(fp8, x3), ScoreTerms(_lq_terms(lq_n, lq_c), ent, pw))
    return o.rowsum, o.colsum, o.diag, o.row_rank, o.inv, o.out8, o.loss, o.w


def score_fwd_sym(Np, Cp, B, D, inv_t, shift, scale_n: float = 1.0, want_rank: bool = True, fp8: bool = False, x3: bool = False):
    """Single-pass symmetric forward of the square problem (tt_score_fwd_sym_bf16 / _fp8 / _bf16x3): returns (rowsum, colsum, diag,
    row_rank, (inv_row, inv_col), out8, loss) -- loss its own 0-dim tensor so that autograd sees a plain output."""
    o = _sym_fwd(Np, Cp, B, D, inv_t, shift, scale_n, want_rank, _operands(fp8, x3), _NO_TERMS)
    return o.rowsum, o.colsum, o.diag, o.row_rank, o.inv, o.out8, o.loss


def score_fwd_sym_lq(Np, Cp, B, D, inv_t, shift, lq_n, lq_c, scale_n: float = 1.0, want_rank: bool = True, x3: bool = False):
    """logQ-corrected score_fwd_sym (tt_score_fwd_sym_bf16_lq / _bf16x3_lq): lq_n / lq_c f32 [B] log sampling probabilities of
    the batch's notices / companies.  Returns (rowsum, colsum, diag, row_rank, (inv_row, inv_col), (w_n, w_c), out8, loss):
    (w_n, w_c) are the sampling weights score_bwd_bf16(..., w=) takes."""
    return _sym8(_sym_fwd(Np, Cp, B, D, inv_t, shift, scale_n, want_rank, _operands(False, x3), ScoreTerms(_lq_terms(lq_n, lq_c))))


def score_fwd_sym_mask(Np, Cp, B, D, inv_t, shift, ent, lq_n=None, lq_c=None, scale_n: float = 1.0, want_rank: bool = True):
    """score_fwd_sym with the repeated-entity mask (tt_score_fwd_sym_bf16_mask): ent = score_mask_ids(ent_n, ent_c, B, dev); lq_n /
    lq_c optional (both or neither).  Returns (rowsum, colsum, diag, row_rank, (inv_row, inv_col), w, out8, loss), w = (w_n, w_c)
    with logQ, else None -- what score_bwd_bf16(..., w=, ent=) takes."""
    return _sym8(_sym_fwd(Np, Cp, B, D, inv_t, shift, scale_n, want_rank, "bf16", ScoreTerms(_lq_terms(lq_n, lq_c), ent)))


def score_fwd_sym_pw(Np, Cp, B, D, inv_t, shift, pw, ent=None, lq_n=None, lq_c=None, scale_n: float = 1.0, want_rank: bool = True):
    """score_fwd_sym with per-pair sample weights (tt_score_fwd_sym_bf16_pw): pw = score_pair_weights(w, B, dev); ent (from
    score_mask_ids) and lq_n / lq_c optional.  Returns as score_fwd_sym_mask; (inv_row, inv_col) are the folded g / rowsum, g / colsum
    that score_bwd_bf16(..., pw=) requires, rowsum / colsum the unweighted sums."""
    return _sym8(_sym_fwd(Np, Cp, B, D, inv_t, shift, scale_n, want_rank, "bf16", ScoreTerms(_lq_terms(lq_n, lq_c), ent, pw)))


def _bwd_sym(Np, Cp, B, D, inv_t, shift, rowsum, colsum, d_loss, scale, scale_n, inv, operands, w, terms: ScoreTerms, w_x=None):
    """The backward of every form on _sym_fwd's sums (the tt_score_bwd_* entries): (dN, dC, dX), dX None without extras.  w / w_x / inv:
    that forward's.  Extras without a plan: the square backward, then their two rectangular directions (score_bwd_bf16_xneg)."""
    dev = Np.device
    other = operands != "bf16"
    ent, pw, plan = terms.ent, terms.pw, terms.plan
    Xp, M, _, ent_x = terms.extras or (None, 0, None, None)
    if w is not None and operands == "fp8":
        raise ValueError("the logQ-corrected backward has no fp8 form")
    if ent is not None and other:
        raise ValueError("the masked backward takes bf16 operands only")
    if pw is not None and other:
        raise ValueError("the weighted backward takes bf16 operands only")
    if pw is not None and inv is None:
        raise ValueError("the weighted backward needs inv, the weighted forward's folded reciprocals")
    if plan is not None:
        if (Xp is None) != (M == 0) or (Xp is None) != (w_x is None):
            raise ValueError("masked cells: the extras' image Xp, M >= 1 and w_x go together")
        if Xp is not None and inv is None:
            raise ValueError("masked cells: the extras' backward needs inv, the forward's reciprocals")
    dN = torch.empty((B, D), dtype=torch.float32, device=dev)
    dC = torch.empty((B, D), dtype=torch.float32, device=dev)
    dX = None
    arr = (L.ScoreBwdDir * 2)()
    ir, ic = (L.ptr(inv[0]), L.ptr(inv[1])) if inv is not None else (None, None)
    arr[0] = L.ScoreBwdDir(L.ptr(Np), L.ptr(Cp), B, B, 0, L.ptr(rowsum), L.ptr(colsum), L.ptr(dN), scale_n, 1.0, ir, ic)   # B = company: unscaled
    arr[1] = L.ScoreBwdDir(L.ptr(Cp), L.ptr(Np), B, B, 0, L.ptr(colsum), L.ptr(rowsum), L.ptr(dC), scale_n, scale_n, ic, ir)  # B = notice image
    lq = None
    if w is not None:                                                  # (w_n / w_c are views of arrays padded to 64 rows, as the kernels read them)
        lq = (L.ScoreBwdLq * 2)()
        lq[0] = L.ScoreBwdLq(L.ptr(w[0]), L.ptr(w[1]))                 # direction (N, C): A = notices, B = companies
        lq[1] = L.ScoreBwdLq(L.ptr(w[1]), L.ptr(w[0]))
    entp = (L.ptr(ent[0]), L.ptr(ent[1])) if ent is not None else (None, None)
    tail = (D, inv_t, shift, L.ptr(d_loss), scale, L.stream(dev))
    if plan is not None:
        dX = torch.empty((M, D), dtype=torch.float32, device=dev) if M else None
        name, args = "tt_score_bwd_bf16_cells", (L.ptr(plan), int(plan._tt_cap), lq, L.ptr(Xp), M, ir, L.ptr(w_x), L.ptr(dX))
    elif pw is not None:                                               # (pw: score_pair_weights' g, with the weighted forward's inv)
        name, args = "tt_score_bwd_bf16_pw", (L.ptr(pw), *entp, lq, 2)
    elif ent is not None:                                              # (ent: score_mask_ids' padded arrays, with the masked forward's sums)
        name, args = "tt_score_bwd_bf16_mask", (*entp, lq, 2)
    else:
        name, args = _BWD_ENTRY[operands] + ("_lq" if lq else ""), ((lq, 2) if lq else (2,))
    with _timed(name):
        L.check(getattr(L.load(), name)(L.ctx(dev), arr, *args, *tail), name)
    if plan is None and terms.extras is not None:
        dX = score_bwd_bf16_xneg(Np, Xp, B, M, D, inv_t, shift, inv[0], w_x, d_loss, scale, dN, scale_n,
                                 ent_c=ent[1] if ent_x is not None else None, ent_x=ent_x)
    return dN, dC, dX


def score_bwd_bf16(Np, Cp, B, D, inv_t, shift, rowsum, colsum, d_loss, scale, scale_n: float = 1.0, inv=None, fp8: bool = False,
                   x3: bool = False, w=None, ent=None, pw=None):
    """inv: (inv_row, inv_col) from score_fwd_bf16(..., with_inv=True) with the same scale_n (optional).
    fp8: the operands are tt_score_pack2_fp8 buffers (tt_score_bwd_fp8); x3: score_pack2_bf16x3 buffers (tt_score_bwd_bf16x3).
    w: (w_n, w_c) from score_fwd_sym_lq, with its rowsum / colsum / inv: the logQ-corrected backward (tt_score_bwd_bf16_lq / _bf16x3_lq).
    ent / pw: as score_fwd_sym_mask / _pw took them (tt_score_bwd_bf16_mask / _pw); pw requires inv."""
    return _bwd_sym(Np, Cp, B, D, inv_t, shift, rowsum, colsum, d_loss, scale, scale_n, inv, _operands(fp8, x3), w,
                    ScoreTerms(ent=ent, pw=pw))[:2]


def score_bwd_bf16_lq(Np, Cp, B, D, inv_t, shift, rowsum, colsum, d_loss, scale, w, scale_n: float = 1.0, inv=None, x3: bool = False):
    """score_bwd_bf16(..., w=w): the logQ-corrected backward."""
    return score_bwd_bf16(Np, Cp, B, D, inv_t, shift, rowsum, colsum, d_loss, scale, scale_n, inv, x3=x3, w=w)


# shared extra negatives (the *_xneg entries of include/twotower.h): M extra company rows X enter every notice's row-direction softmax
def score_xneg_ids(ent_x, M, dev):
    """the extras' company ids as the *_xneg entries read them: int32 [round_up(M, 64)], 16-byte aligned, zero (ignored) past M"""
    e = _ent_vec(ent_x, M, dev, "ent_x")
    Mp = (M + 63) // 64 * 64
    if M == Mp and e.is_contiguous() and e.data_ptr() % 16 == 0:
        return e
    out = torch.zeros(Mp, dtype=torch.int32, device=dev)
    out[:M] = e
    return out


def _xneg_check(B, M, ent, ent_x, lq, lq_x):
    if M < 1:
        raise ValueError(f"extra negatives: M must be >= 1, got {M}")
    if ent_x is not None and ent is None:
        raise ValueError("extra negatives: ent_x needs the batch's ids (ent)")
    if lq_x is not None and not lq:
        raise ValueError("extra negatives: lq_x needs lq_n / lq_c")


def score_fwd_sym_xneg(Np, Cp, Xp, B, M, D, inv_t, shift, ent=None, ent_x=None, lq_n=None, lq_c=None, lq_x=None, scale_n: float = 1.0,
                       want_rank: bool = True):
    """score_fwd_sym (/_lq /_mask) with M shared extra negatives (tt_score_fwd_sym_bf16_xneg): Xp = score_pack_bf16(X) (scale 1), ent =
    score_mask_ids(...) or None, ent_x = score_xneg_ids(...) or None (never masked), lq_x f32 [M] or None (log q = 0).  Returns
    (rowsum, colsum, diag, row_rank, (inv_row, inv_col), w, w_x, out8, loss): rowsum / inv_row include the extras, w = (w_n, w_c) with
    logQ else None, w_x [round_up(M, 64)] the extras' weights -- what score_bwd_bf16_xneg takes."""
    return tuple(_sym_fwd(Np, Cp, B, D, inv_t, shift, scale_n, want_rank, "bf16",
                          ScoreTerms(_lq_terms(lq_n, lq_c), ent, extras=(Xp, M, lq_x, ent_x))))


def score_bwd_bf16_xneg(Np, Xp, B, M, D, inv_t, shift, inv_row, w_x, d_loss, scale, dN, scale_n: float = 1.0, ent_c=None, ent_x=None):
    """The extras' share of the backward (tt_score_bwd_bf16_xneg), AFTER score_bwd_bf16 on the same forward's sums: adds (1/T)/(2B) Wx X
    to dN in place and returns dX [M, D].  inv_row / w_x: score_fwd_sym_xneg's (views of its padded arrays); ent_c = the ent[1] of
    score_mask_ids and ent_x = score_xneg_ids(...), both or neither."""
    dev = Np.device
    if (ent_c is None) != (ent_x is None):
        raise ValueError("extra negatives: ent_c and ent_x go together")
    if not (dN.is_contiguous() and dN.dtype == torch.float32 and tuple(dN.shape) == (B, D)):
        raise ValueError(f"dN must be a contiguous float32 [{B}, {D}] tensor")
    dX = torch.empty((M, D), dtype=torch.float32, device=dev)
    name = "tt_score_bwd_bf16_xneg"
    with _timed(name):
        L.check(getattr(L.load(), name)(L.ctx(dev), L.ptr(Np), L.ptr(Xp), B, M, D, inv_t, shift, scale_n, L.ptr(inv_row), L.ptr(w_x),
                                        L.ptr(ent_c) if ent_c is not None else None, L.ptr(ent_x) if ent_x is not None else None,
                                        L.ptr(d_loss), scale, L.ptr(dN), L.ptr(dX), L.stream(dev)), name)
    return dX


def score_dir_fwd_xneg(n, x, inv_t, shift, diag, sumexp, rank, lq_x=None, ent_c=None, ent_x=None):
    """f32 parity path (tt_score_dir_fwd_xneg): adds the extras x [M, D] to the row direction of score_dir_fwd(n, c, ...) IN PLACE --
    sumexp[a] += sum_m e_am w_m, rank[a] += #{m: s_am > diag[a]}.  ent_c / ent_x (both or neither): the company-only mask."""
    dev, B, M, D = n.device, n.shape[0], x.shape[0], n.shape[1]
    if (ent_c is None) != (ent_x is None):
        raise ValueError("extra negatives: ent_c and ent_x go together")
    lqx = None if lq_x is None else _lq_vec(lq_x, M, dev, "lq_x")
    name = "tt_score_dir_fwd_xneg"
    with _timed(name):
        L.check(getattr(L.load(), name)(L.ctx(dev), L.ptr(n), L.ptr(x), B, M, D, inv_t, shift, L.ptr(ent_c) if ent_c is not None else None,
                                        L.ptr(ent_x) if ent_x is not None else None, L.ptr(lqx) if lqx is not None else None,
                                        L.ptr(diag), L.ptr(sumexp), L.ptr(rank), L.stream(dev)), name)


def score_dir_bwd_xneg(A, Bm, inv_t, shift, x_is_b, rowsum, d_loss, scale, lq_x=None, ent_a=None, ent_b=None, out=None):
    """f32 parity path (tt_score_dir_bwd_xneg), one rectangular direction of the extras: x_is_b: A = N, Bm = X -> dN's extra term, added
    to `out` (the square backward's dN); else A = X, Bm = N -> dX (returned).  rowsum: the notice rows' sums with the extras."""
    dev, Ra, Rb, D = A.device, A.shape[0], Bm.shape[0], A.shape[1]
    if (ent_a is None) != (ent_b is None):
        raise ValueError("extra negatives: ent_a and ent_b go together")
    lqx = None if lq_x is None else _lq_vec(lq_x, Rb if x_is_b else Ra, dev, "lq_x")
    dA = out if out is not None else torch.empty_like(A)
    name = "tt_score_dir_bwd_xneg"
    with _timed(name):
        L.check(getattr(L.load(), name)(L.ctx(dev), L.ptr(A), L.ptr(Bm), Ra, Rb, D, inv_t, shift, int(bool(x_is_b)),
                                        L.ptr(ent_a) if ent_a is not None else None, L.ptr(ent_b) if ent_b is not None else None,
                                        L.ptr(lqx) if lqx is not None else None, L.ptr(rowsum), L.ptr(d_loss), scale,
                                        int(out is not None), L.ptr(dA), L.stream(dev)), name)
    return dA


# masked cells (the *_cells entries of include/twotower.h): a sparse per-step list of (row, column) pairs that are never negatives
def score_cells_check(cells, dev, name="masked_cells"):
    """int32 [L, 2] on `dev`, L >= 0 (validated: no device sync); returns it contiguous"""
    if not isinstance(cells, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor, got {type(cells).__name__}")
    if cells.dtype != torch.int32:
        raise TypeError(f"{name} must be int32, got {cells.dtype}")
    if cells.dim() != 2 or cells.shape[1] != 2:
        raise ValueError(f"{name} must have shape [L, 2], got {list(cells.shape)}")
    if cells.device != torch.device(dev):
        raise ValueError(f"{name} is on {cells.device}, the scores on {dev}")
    return cells.contiguous()


def score_cells_plan(cells, B, M=0, count=None, out=None):
    """The masked cells bucketed by 32 x 32 tile pair (tt_score_cells_plan), what score_fwd_sym_cells / score_bwd_bf16_cells take.
    cells int32 [capacity, 2] rows (a, j), a in [0, B), j in [0, B + M) (j >= B: extra j - B); cells on the diagonal or outside the
    ranges are dropped, duplicates and order are free.  count: int32 [1] on the device -- only the first min(count, capacity) rows are
    read (None: all of them); the launches' grids depend on the capacity alone, so the call can be captured with a static `cells` buffer
    and a device count.  out: a plan buffer of an earlier call with the same B, M and capacity, refilled in place."""
    dev = cells.device
    cells = score_cells_check(cells, dev)
    L_ = cells.shape[0]
    cap = max(L_, 1)
    if L_ == 0:                                                        # (the entry wants one slot; the count says it is unused)
        cells = torch.zeros((1, 2), dtype=torch.int32, device=dev)
        count = torch.zeros(1, dtype=torch.int32, device=dev) if count is None else count
    if count is None:
        count = torch.full((1,), L_, dtype=torch.int32, device=dev)
    elif not (isinstance(count, torch.Tensor) and count.dtype == torch.int32 and count.numel() == 1 and count.device == dev):
        raise ValueError(f"count must be an int32 tensor of one element on {dev}")
    lib = L.load()
    n = lib.tt_score_cells_plan_bytes(B, M, cap) // 4
    if n == 0:
        raise ValueError(f"masked cells: bad shape B={B} M={M} capacity={cap}")
    plan = out if out is not None else torch.empty(n, dtype=torch.int32, device=dev)
    if plan.dtype != torch.int32 or plan.numel() < n or plan.device != dev or not plan.is_contiguous():
        raise ValueError(f"out must be a contiguous int32 tensor of at least {n} elements on {dev}")
    # the tile pairs' counters: memory of this call's own, kept with the plan (not the stream's shared scratch)
    ws = torch.empty(lib.tt_score_cells_plan_workspace_bytes(B, M), dtype=torch.uint8, device=dev)
    with _timed("tt_score_cells_plan"):
        L.check(lib.tt_score_cells_plan(L.ctx(dev), L.ptr(cells), L.ptr(count), cap, B, M, L.ptr(plan), plan.numel() * 4, L.ptr(ws),
                                        ws.numel(), L.stream(dev)), "tt_score_cells_plan")
    plan._tt_keep = (cells, count, ws)
    plan._tt_cap = cap
    return plan


def score_cells_unpack(plan, B, M=0):
    """(offsets int64 [nT * (nT + nTx) + 1], codes int32 [offsets[-1]]) of a plan, on the host -- a debugging / test aid (synchronises)"""
    nT, nTx = (B + 31) // 32, (M + 31) // 32
    n_pairs = nT * (nT + nTx)
    at = (n_pairs + 1 + 3) // 4 * 4
    p = plan.cpu()
    off = p[:n_pairs + 1].long()
    return off, p[at:at + int(off[-1])]


def score_fwd_sym_cells(Np, Cp, B, D, inv_t, shift, plan, Xp=None, M=0, lq_n=None, lq_c=None, lq_x=None, scale_n: float = 1.0,
                        want_rank: bool = True):
    """score_fwd_sym (/_lq, /_xneg without ids) on the masked cells of `plan` = score_cells_plan(cells, B, M)
    (tt_score_fwd_sym_bf16_cells).  Returns as score_fwd_sym_xneg: (rowsum, colsum, diag, row_rank, (inv_row, inv_col), w, w_x, out8,
    loss), w_x None without extras."""
    return tuple(_sym_fwd(Np, Cp, B, D, inv_t, shift, scale_n, want_rank, "bf16",
                          ScoreTerms(_lq_terms(lq_n, lq_c), extras=(Xp, M, lq_x, None), plan=plan)))


def score_bwd_bf16_cells(Np, Cp, B, D, inv_t, shift, rowsum, colsum, d_loss, scale, plan, scale_n: float = 1.0, inv=None, w=None,
                         Xp=None, M=0, w_x=None):
    """The backward on score_fwd_sym_cells' sums (tt_score_bwd_bf16_cells): returns (dN, dC, dX), dX None without extras.  inv / w: that
    forward's (views of its padded arrays); with extras (Xp, M, w_x) inv is required -- its inv_row is the extras' row factor."""
    return _bwd_sym(Np, Cp, B, D, inv_t, shift, rowsum, colsum, d_loss, scale, scale_n, inv, "bf16", w,
                    ScoreTerms(extras=(Xp, M, None, None), plan=plan), w_x)


def score_dir_fwd_lq(A, Bm, inv_t, shift, lq_b, diag_offset=0, want_sumscore=True):
    """score_dir_fwd(..., lq_b=lq_b)"""
    return score_dir_fwd(A, Bm, inv_t, shift, diag_offset, want_sumscore, lq_b=lq_b)


def score_dir_bwd_lq(A, Bm, inv_t, shift, diag_offset, lq_a, lq_b, sumexp_a, sumexp_b, d_loss, scale):
    """score_dir_bwd(..., lq_a=lq_a, lq_b=lq_b)"""
    return score_dir_bwd(A, Bm, inv_t, shift, diag_offset, sumexp_a, sumexp_b, d_loss, scale, lq_a=lq_a, lq_b=lq_b)


def score_fwd_bf16_rect(Ap0, Bp0, Ap1, Bp1, Ra, Rb, off, D, inv_t, shift, full_rank=True):
    """Rectangular form (global in-batch negatives): direction 0 = rows of A0 [Ra] against all rows of B0 [Rb], direction 1 =
    rows of A1 [Ra] against B1 [Rb]; the positive of local row a sits at column a + off.  Returns (sumexp0, sumexp1, diag,
    rank0, rank1, sumscore0)."""
    dev = Ap0.device
    Rp = (Ra + 3) // 4 * 4
    f = torch.empty((4, Rp), dtype=torch.float32, device=dev)
    ranks = torch.empty((2, Ra), dtype=torch.int32, device=dev)
    arr = (L.ScoreFwdDir * 2)()
    rm = 2 if full_rank else 1
    arr[0] = L.ScoreFwdDir(L.ptr(Ap0), L.ptr(Bp0), Ra, Rb, off, L.ptr(f[0]), L.ptr(f[2]), L.ptr(ranks[0]), L.ptr(f[3]), rm)
    arr[1] = L.ScoreFwdDir(L.ptr(Ap1), L.ptr(Bp1), Ra, Rb, off, L.ptr(f[1]), None, L.ptr(ranks[1]), None, rm)
    with _timed("tt_score_fwd_bf16"):
        L.check(L.load().tt_score_fwd_bf16(L.ctx(dev), arr, 2, D, inv_t, shift, L.stream(dev)), "tt_score_fwd_bf16")
    return f[0][:Ra], f[1][:Ra], f[2][:Ra], ranks[0], ranks[1], f[3][:Ra]


def _tile_padded(t: torch.Tensor) -> torch.Tensor:
    """per-row float array readable a whole 32-row tile at a time (tt_score_bwd_dir): ragged sizes get a padded copy"""
    n = t.numel()
    if n % 32 == 0 and t.is_contiguous():
        return t
    out = torch.ones((n + 31) // 32 * 32, dtype=t.dtype, device=t.device)
    out[:n] = t
    return out


def score_bwd_bf16_rect(Ap0, Bp0, Ap1, Bp1, Ra, Rb, off, D, inv_t, shift, sa0, sb0, sa1, sb1, d_loss, scale):
    """dA0 [Ra, D], dA1 [Ra, D]: sa* = sum-exp of the A rows (this direction), sb* = sum-exp of the B rows in the OTHER
    direction (all Rb of them: gathered from their owners)."""
    dev = Ap0.device
    sb0, sb1 = _tile_padded(sb0), _tile_padded(sb1)
    d0 = torch.empty((Ra, D), dtype=torch.float32, device=dev)
    d1 = torch.empty((Ra, D), dtype=torch.float32, device=dev)
    arr = (L.ScoreBwdDir * 2)()
    arr[0] = L.ScoreBwdDir(L.ptr(Ap0), L.ptr(Bp0), Ra, Rb, off, L.ptr(sa0), L.ptr(sb0), L.ptr(d0))
    arr[1] = L.ScoreBwdDir(L.ptr(Ap1), L.ptr(Bp1), Ra, Rb, off, L.ptr(sa1), L.ptr(sb1), L.ptr(d1))
    with _timed("tt_score_bwd_bf16"):
        L.check(L.load().tt_score_bwd_bf16(L.ctx(dev), arr, 2, D, inv_t, shift, L.ptr(d_loss), scale, L.stream(dev)),
                "tt_score_bwd_bf16")
    return d0, d1


def score_matrix(A, Bm, inv_t):
    dev, Ra, Rb, D = A.device, A.shape[0], Bm.shape[0], A.shape[1]
    S = torch.empty((Ra, Rb), dtype=torch.float32, device=dev)
    with _timed("tt_score_matrix"):
        L.check(L.load().tt_score_matrix(L.ctx(dev), L.ptr(A), L.ptr(Bm), Ra, Rb, D, inv_t, L.ptr(S), Rb, L.stream(dev)),
                "tt_score_matrix")
    return S


def score_dense_fwd(n, c, inv_t: float, loss_type: int, label_smoothing: float, hit=None):
    """Dense loss path (tt_score_dense_fwd): returns (S [B, B], stats, out8, loss[1]) -- S and stats feed score_dense_bwd.
    hit (optional int32 [2 B]): receives the per-row / per-column top-1 flags (first argmax == diagonal)."""
    dev, B, D = n.device, n.shape[0], n.shape[1]
    S = torch.empty((B, B), dtype=torch.float32, device=dev)
    stats = torch.empty(6 * B, dtype=torch.float32, device=dev)
    if hit is None:
        hit = torch.empty(2 * B, dtype=torch.int32, device=dev)
    assert hit.dtype == torch.int32 and hit.is_contiguous() and hit.numel() >= 2 * B
    out8 = torch.empty(8, dtype=torch.float32, device=dev)
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    with _timed("tt_score_dense_fwd"):
        L.check(L.load().tt_score_dense_fwd(L.ctx(dev), L.ptr(n), L.ptr(c), B, D, inv_t, loss_type, label_smoothing, L.ptr(S), L.ptr(stats),
                                            L.ptr(hit), L.ptr(out8), L.ptr(loss), L.stream(dev)), "tt_score_dense_fwd")
    return S, stats, out8, loss


def score_dense_bwd(n, c, inv_t: float, loss_type: int, label_smoothing: float, S, stats, d_loss):
    """(dN, dC) of the dense loss path; S is overwritten by d loss / d (N C^T)."""
    dev, B, D = n.device, n.shape[0], n.shape[1]
    dN, dC = torch.empty_like(n), torch.empty_like(c)
    ws = torch.empty(L.load().tt_score_dense_workspace_bytes(B, D), dtype=torch.uint8, device=dev)
    with _timed("tt_score_dense_bwd"):
        L.check(L.load().tt_score_dense_bwd(L.ctx(dev), L.ptr(n), L.ptr(c), B, D, inv_t, loss_type, label_smoothing, L.ptr(S), L.ptr(stats),
                                            L.ptr(d_loss), L.ptr(dN), L.ptr(dC), L.ptr(ws), ws.numel(), L.stream(dev)), "tt_score_dense_bwd")
    return dN, dC


def diag_rank_rows(S, diag_offset=0):
    dev, R, Cc = S.device, S.shape[0], S.shape[1]
    assert S.stride(1) == 1 and S.dtype == torch.float32
    rank = torch.empty(R, dtype=torch.int32, device=dev)
    L.check(L.load().tt_diag_rank_rows(L.ctx(dev), L.ptr(S), R, Cc, S.stride(0), diag_offset, L.ptr(rank), L.stream(dev)),
            "tt_diag_rank_rows")
    return rank


def topk_rows(S, k):
    dev, R, Cc = S.device, S.shape[0], S.shape[1]
    assert S.stride(1) == 1
    vals = torch.empty((R, k), dtype=torch.float32, device=dev)
    idx = torch.empty((R, k), dtype=torch.int64, device=dev)
    with _timed("tt_topk_rows"):
        L.check(L.load().tt_topk_rows(L.ctx(dev), L.ptr(S), R, Cc, S.stride(0), k, L.ptr(vals), L.ptr(idx), L.stream(dev)),
                "tt_topk_rows")
    return vals, idx


def retrieve_workspace_bytes(nQ: int, nC: int, D: int, k: int) -> int:
    return int(L.load().tt_retrieve_workspace_bytes(int(nQ), int(nC), int(D), int(k)))


def _retrieve(Q, nQ, C, nC, D, k, inv_t, bf16, positives, workspace, exclude=None, filt=None, ceil=None):
    """One tt_retrieve_topk_* call: Q / C are packed bf16 images (bf16=True) or f32 [n, D] rows.  Returns (vals, idx, rank);
    vals / idx are None for k = 0, rank is None without positives.  exclude=(offsets int64 [nQ + 1], rows int32): per-query
    exclusion lists in CSR form, each list ascending (tt_excl_retrieve_topk_*).  filt=(tags int32 [nC, W], W, any, all):
    attribute filter (tt_filt_retrieve_topk_*, with or without exclude); any / all are int32 [nQ, W] masks or None, not
    both None.  ceil: f32 [nQ] per-query score ceilings of the top-k (tt_ceil_retrieve_topk_*, with or without exclude, never with
    filt)."""
    dev = C.device
    lib = L.load()
    vals = torch.empty((nQ, k), dtype=torch.float32, device=dev) if k else None
    idx = torch.empty((nQ, k), dtype=torch.int64, device=dev) if k else None
    rank = None
    if positives is not None:
        if positives.dtype not in (torch.int32, torch.int64) or positives.shape != (nQ,) or not positives.is_contiguous():
            raise ValueError(f"positives must be a contiguous int32/int64 tensor of shape ({nQ},)")
        rank = torch.empty(nQ, dtype=torch.int32, device=dev)
    if exclude is not None:
        off, rows = exclude
        if off.dtype != torch.int64 or off.shape != (nQ + 1,) or not off.is_contiguous() or off.device != dev:
            raise ValueError(f"exclusion offsets must be a contiguous int64 tensor of shape ({nQ + 1},) on {dev}")
        if rows.dtype != torch.int32 or rows.dim() != 1 or not rows.is_contiguous() or rows.device != dev:
            raise ValueError(f"exclusion rows must be a contiguous 1-D int32 tensor on {dev}")
        if rows.numel() == 0:                                     # (the entry wants a pointer even for empty lists)
            rows = torch.zeros(1, dtype=torch.int32, device=dev)
    need = lib.tt_retrieve_workspace_bytes(nQ, nC, D, k)
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
    pos_i64 = 1 if positives is not None and positives.dtype == torch.int64 else 0
    if ceil is not None:
        if filt is not None:
            raise ValueError("a score ceiling does not combine with an attribute filter")
        if ceil.dtype != torch.float32 or ceil.shape != (nQ,) or not ceil.is_contiguous() or ceil.device != dev:
            raise ValueError(f"the score ceilings must be a contiguous float32 tensor of shape ({nQ},) on {dev}")
        off, rows = (off, rows) if exclude is not None else (None, None)
        name = "tt_ceil_retrieve_topk_bf16" if bf16 else "tt_ceil_retrieve_topk_f32"
        with _timed(name):
            if bf16:
                rc = lib.tt_ceil_retrieve_topk_bf16(L.ctx(dev), L.ptr(Q), nQ, L.ptr(C), nC, D, k, L.ptr(positives), pos_i64,
                                                    L.ptr(vals), L.ptr(idx), L.ptr(rank), L.ptr(off), L.ptr(rows), L.ptr(ceil),
                                                    L.ptr(workspace), workspace.numel(), L.stream(dev))
            else:
                rc = lib.tt_ceil_retrieve_topk_f32(L.ctx(dev), L.ptr(Q), nQ, L.ptr(C), nC, D, inv_t, k, L.ptr(positives), pos_i64,
                                                   L.ptr(vals), L.ptr(idx), L.ptr(rank), L.ptr(off), L.ptr(rows), L.ptr(ceil),
                                                   L.ptr(workspace), workspace.numel(), L.stream(dev))
            L.check(rc, name)
        return vals, idx, rank
    if filt is not None:
        tags, W, m_any, m_all = filt
        W = int(W)
        if tags.dtype != torch.int32 or tags.shape != (nC, W) or not tags.is_contiguous() or tags.device != dev:
            raise ValueError(f"tags must be a contiguous int32 tensor of shape ({nC}, {W}) on {dev}")
        for what, m in (("any", m_any), ("all", m_all)):
            if m is not None and (m.dtype != torch.int32 or m.shape != (nQ, W) or not m.is_contiguous() or m.device != dev):
                raise ValueError(f"the {what} mask must be a contiguous int32 tensor of shape ({nQ}, {W}) on {dev}")
        off, rows = (off, rows) if exclude is not None else (None, None)
        name = "tt_filt_retrieve_topk_bf16" if bf16 else "tt_filt_retrieve_topk_f32"
        with _timed(name):
            if bf16:
                rc = lib.tt_filt_retrieve_topk_bf16(L.ctx(dev), L.ptr(Q), nQ, L.ptr(C), nC, D, k, L.ptr(positives), pos_i64,
                                                    L.ptr(vals), L.ptr(idx), L.ptr(rank), L.ptr(off), L.ptr(rows), L.ptr(tags), W,
                                                    L.ptr(m_any), L.ptr(m_all), L.ptr(workspace), workspace.numel(), L.stream(dev))
            else:
                rc = lib.tt_filt_retrieve_topk_f32(L.ctx(dev), L.ptr(Q), nQ, L.ptr(C), nC, D, inv_t, k, L.ptr(positives), pos_i64,
                                                   L.ptr(vals), L.ptr(idx), L.ptr(rank), L.ptr(off), L.ptr(rows), L.ptr(tags), W,
                                                   L.ptr(m_any), L.ptr(m_all), L.ptr(workspace), workspace.numel(), L.stream(dev))
            L.check(rc, name)
        return vals, idx, rank
    if exclude is None:
        name = "tt_retrieve_topk_bf16" if bf16 else "tt_retrieve_topk_f32"
        with _timed(name):
            if bf16:
                rc = lib.tt_retrieve_topk_bf16(L.ctx(dev), L.ptr(Q), nQ, L.ptr(C), nC, D, k, L.ptr(positives), pos_i64, L.ptr(vals),
                                               L.ptr(idx), L.ptr(rank), L.ptr(workspace), workspace.numel(), L.stream(dev))
            else:
                rc = lib.tt_retrieve_topk_f32(L.ctx(dev), L.ptr(Q), nQ, L.ptr(C), nC, D, inv_t, k, L.ptr(positives), pos_i64,
                                              L.ptr(vals), L.ptr(idx), L.ptr(rank), L.ptr(workspace), workspace.numel(), L.stream(dev))
            L.check(rc, name)
        return vals, idx, rank
    name = "tt_excl_retrieve_topk_bf16" if bf16 else "tt_excl_retrieve_topk_f32"
    with _timed(name):
        if bf16:
            rc = lib.tt_excl_retrieve_topk_bf16(L.ctx(dev), L.ptr(Q), nQ, L.ptr(C), nC, D, k, L.ptr(positives), pos_i64, L.ptr(vals),
                                                L.ptr(idx), L.ptr(rank), L.ptr(off), L.ptr(rows), L.ptr(workspace), workspace.numel(),
                                                L.stream(dev))
        else:
            rc = lib.tt_excl_retrieve_topk_f32(L.ctx(dev), L.ptr(Q), nQ, L.ptr(C), nC, D, inv_t, k, L.ptr(positives), pos_i64,
                                               L.ptr(vals), L.ptr(idx), L.ptr(rank), L.ptr(off), L.ptr(rows), L.ptr(workspace),
                                               workspace.numel(), L.stream(dev))
        L.check(rc, name)
    return vals, idx, rank


def retrieve_topk(Q, nQ, C, nC, D, k, inv_t=1.0, bf16=False, positives=None, workspace=None, exclude=None, filt=None, ceil=None):
    """Top-k of every query over the whole catalogue (tt_retrieve_topk_bf16 / _f32): (vals f32 [nQ, k], idx int64 [nQ, k]),
    value descending, ties to the lower index.  With positives, (vals, idx, rank) from the same sweep.  exclude=(offsets,
    rows): query q's rows rows[offsets[q]:offsets[q+1]] (ascending) are left out of its top-k and rank
    (tt_excl_retrieve_topk_*).  filt=(tags, W, any, all): only rows eligible under the query's masks (tt_filt_retrieve_topk_*).
    ceil: f32 [nQ]: only rows that score below ceil[q] enter query q's top-k; the rank is unchanged (tt_ceil_retrieve_topk_*)."""
    vals, idx, rank = _retrieve(Q, nQ, C, nC, D, k, inv_t, bf16, positives, workspace, exclude, filt, ceil)
    return (vals, idx) if positives is None else (vals, idx, rank)


def retrieve_rank(Q, nQ, C, nC, D, positives, inv_t=1.0, bf16=False, workspace=None, exclude=None, filt=None):
    """Rank of each query's positive among all catalogue rows (k = 0 call): int32 [nQ],
    #{c : s > s_p} + #{c < p : s == s_p}, -1 for a positive outside [0, nC).  With exclude=(offsets, rows), only rows outside
    the query's list count; with filt=(tags, W, any, all), only eligible rows."""
    return _retrieve(Q, nQ, C, nC, D, 0, inv_t, bf16, positives, workspace, exclude, filt)[2]


def pair_scores(Q, nQ, C, nC, D, rows, inv_t=1.0, bf16=False):
    """f32 [nQ]: the score of query q against catalogue row rows[q] (int32 / int64 [nQ]), bit for bit what the retrieval sweep
    computes for that pair (tt_pair_scores_bf16 / _f32; operands as retrieve_topk's); NaN for a row outside [0, nC)."""
    dev = C.device
    if rows.dtype not in (torch.int32, torch.int64) or rows.shape != (nQ,) or not rows.is_contiguous() or rows.device != dev:
        raise ValueError(f"rows must be a contiguous int32/int64 tensor of shape ({nQ},) on {dev}")
    lib = L.load()
    out = torch.empty(nQ, dtype=torch.float32, device=dev)
    i64 = 1 if rows.dtype == torch.int64 else 0
    name = "tt_pair_scores_bf16" if bf16 else "tt_pair_scores_f32"
    with _timed(name):
        if bf16:
            rc = lib.tt_pair_scores_bf16(L.ctx(dev), L.ptr(Q), nQ, L.ptr(C), nC, D, L.ptr(rows), i64, L.ptr(out), L.stream(dev))
        else:
            rc = lib.tt_pair_scores_f32(L.ctx(dev), L.ptr(Q), nQ, L.ptr(C), nC, D, inv_t, L.ptr(rows), i64, L.ptr(out), L.stream(dev))
        L.check(rc, name)
    return out


# ---------------------------------------------------------------------------------------------- misc
def linear_fwd(X, W, bias, relu=False):
    dev, M, K, N = X.device, X.shape[0], X.shape[1], W.shape[0]
    assert (M == 0 or X.stride(1) == 1) and W.is_contiguous()
    Y = torch.empty((M, N), dtype=torch.float32, device=dev)
    ldx = X.stride(0) if M else K                                 # (an empty tensor's strides say nothing: they may be 0)
    L.check(L.load().tt_linear_fwd(L.ctx(dev), L.ptr(X), ldx, L.ptr(W), L.ptr(bias), L.ptr(Y), N, M, N, K, int(relu),
                                   L.stream(dev)), "tt_linear_fwd")
    return Y


def _copy_segments(pairs, who):
    """[(dst, src)] contiguous same-sized tensors -> (n, dst, src, nb): the ctypes arrays of one launch's copy segments."""
    for d, s_ in pairs:
        if d.numel() * d.element_size() != s_.numel() * s_.element_size() or not d.is_contiguous() or not s_.is_contiguous():
            raise ValueError(f"{who}: segments must be contiguous and equally sized")
    n = len(pairs)
    dst = (L.vp * max(n, 1))(*[d.data_ptr() for d, _ in pairs])
    src = (L.vp * max(n, 1))(*[s_.data_ptr() for _, s_ in pairs])
    nb = (L.i64 * max(n, 1))(*[d.numel() * d.element_size() for d, _ in pairs])
    return n, dst, src, nb


def copy_multi(pairs):
    """pairs: [(dst, src)] contiguous same-sized tensors on one device -> one launch."""
    if not pairs:
        return
    dev = pairs[0][0].device
    n, dst, src, nb = _copy_segments(pairs, "copy_multi")
    with _timed("tt_copy_multi"):
        L.check(L.load().tt_copy_multi(L.ctx(dev), n, dst, src, nb, L.stream(dev)), "tt_copy_multi")


def ingest_lookup_supported(table: Optional[torch.Tensor], sides: Sequence[LookupSide]) -> bool:
    """Shapes the fused hand-over + lookup launch takes (tt_batch_ingest_lookup): E in {8, 16, 32, 64}, 8-element aligned outputs."""
    if table is None or table.dtype != torch.float32 or table.dim() != 2 or table.shape[1] not in (8, 16, 32, 64) or table.data_ptr() % 16:
        return False
    for s_ in sides:
        o = s_.out
        if o is None or o.dtype not in (torch.float32, torch.bfloat16) or o.stride(1) != 1 or o.stride(0) % 8 or \
                o.data_ptr() % (8 * o.element_size()) or not (1 <= s_.K <= 64):
            return False
    return True


def ingest_lookup_tiles(B: int, side_K: Sequence[int]) -> int:
    """Tile workgroups of the fused hand-over + lookup launch (csrc/tt_embed.hip fill_lookup_part: TS = 64 samples, halved until
    TS * K <= 512 slots, not below 8)."""
    n = 0
    for K in side_K:
        sh = 6
        while sh > 3 and (K << sh) > 512:
            sh -= 1
        n += (B + (1 << sh) - 1) >> sh
    return n


def _cvt_list(cvt):
    """[(dst bf16, src f32)] -> ctypes tt_cvt_list pointer (or None): conversions that ride in the hand-over launch."""
    if not cvt:
        return None
    if len(cvt) > L.TT_MAX_CVT:
        raise ValueError(f"at most {L.TT_MAX_CVT} conversions per hand-over launch")
    c = L.CvtList()
    c.n = len(cvt)
    for i, (d, s_) in enumerate(cvt):
        if d.dtype != torch.bfloat16 or s_.dtype != torch.float32 or d.numel() != s_.numel() or not d.is_contiguous() or not s_.is_contiguous() \
                or d.device != s_.device:
            raise ValueError("cvt: (bf16 destination, f32 source) pairs of contiguous tensors of one size on one device")
        c.src[i], c.dst[i], c.count[i] = s_.data_ptr(), d.data_ptr(), s_.numel()
    return C.byref(c)


def _lookup_part(table: torch.Tensor):
    return L.IngestLookup(L.ptr(table), table.shape[0], table.shape[1], 0)


def _embed_sides(sides, B, dev, who, with_ids: bool, with_out: bool):
    """sides -> (tt_embed_side array, sum(B*K)).  with_ids: the sides' own ids (False: the hand-over reads them from the stores);
    with_out: the sides' output views (the fused hand-over + lookup)."""
    arr = (L.EmbedSide * len(sides))()
    M = 0
    for i, s in enumerate(sides):
        if with_ids and (s.ids.dtype != torch.int64 or not s.ids.is_contiguous() or s.ids.device != dev or s.ids.numel() != B * s.K):
            raise ValueError(f"{who}: side {i} needs {B}*{s.K} contiguous int64 ids on {dev}")
        if with_out:
            if s.out.shape[0] != B or s.out.shape[1] < s.K or s.out.device != dev:
                raise ValueError(f"{who}: side {i}: output view must be [B, K*E] on {dev}")
            arr[i] = L.EmbedSide(L.ptr(s.ids) if with_ids else None, L.ptr(s.key_row_offset), L.ptr(s.key_vocab), L.ptr(s.out), s.out.stride(0),
                                 s.K, _dt(s.out))
        else:
            arr[i] = L.EmbedSide(L.ptr(s.ids) if with_ids else None, L.ptr(s.key_row_offset), L.ptr(s.key_vocab), None, 0, s.K, TT_F32)
        M += B * s.K
    return arr, M


def _check_rows(rows, M, who, name):
    if rows is not None and (rows.dtype != torch.int32 or rows.numel() != M or not rows.is_contiguous()):
        raise ValueError(f"{who}: {name} must be a contiguous int32 tensor of sum(B*K) elements")


def batch_ingest(pairs, sides: Sequence[LookupSide], B: int, rows_km: Optional[torch.Tensor], table: Optional[torch.Tensor] = None,
                 rows_sm: Optional[torch.Tensor] = None, cvt=None, table_rows: int = 0):
    """copy_multi's segments plus, per side, the fused rows of the side's ids in key-major order (tt_batch_ingest): the batch
    hand-over of a graph-replayed step in one launch.  sides[i].ids is the id source (the incoming batch or the static buffer).
    table given (and sides[i].out set): the same launch also looks the rows up and writes them into sides[i].out -- the towers'
    input (tt_batch_ingest_lookup); rows_km may then be None.  rows_sm (without `table`): the same fused rows also in slot order,
    the input of embed_lookup_rows.  table_rows (without `table`): the size of the row space the fused rows index -- a row outside
    it is stored as the last row and raises the device error word (_lib.check_device_errors), so neither embed_lookup_rows nor the
    plan's consumers touch memory outside the table; 0 = unchecked."""
    dev = table.device if table is not None else rows_km.device
    n, dst, src, nb = _copy_segments(pairs, "batch_ingest")
    arr, M = _embed_sides(sides, B, dev, "batch_ingest", True, table is not None)
    _check_rows(rows_km, M, "batch_ingest", "rows_km")
    if table is not None:
        lk = _lookup_part(table)
        with _timed("tt_batch_ingest_lookup"):
            L.check(L.load().tt_batch_ingest_lookup(L.ctx(dev), n, dst, src, nb, arr, len(sides), B, L.ptr(rows_km), C.byref(lk), _cvt_list(cvt),
                                                    L.stream(dev)), "tt_batch_ingest_lookup")
        return
    _check_rows(rows_sm, M, "batch_ingest", "rows_sm")
    with _timed("tt_batch_ingest"):
        L.check(L.load().tt_batch_ingest(L.ctx(dev), n, dst, src, nb, arr, len(sides), B, L.ptr(rows_km), L.ptr(rows_sm), int(table_rows),
                                         _cvt_list(cvt), L.stream(dev)), "tt_batch_ingest")


@dataclass
class StoreSide:
    """One tower's device-resident feature store as the source of a batch (tt_store_side)."""
    entity: torch.Tensor          # int64: entity index per pair, element [o * entity_stride] (a column of the [P, 2] pair list)
    entity_stride: int
    dense_store: torch.Tensor     # f32 [N, dense_dim]
    cat_store: torch.Tensor       # int64 [N, K]
    dense_out: torch.Tensor       # f32 [B, dense_dim]  (the step's static dense buffer)
    ids_out: torch.Tensor         # int64 [B * K]       (the step's static id buffer)


def batch_ingest_store(pairs, sides: Sequence[LookupSide], stores: Sequence[StoreSide], B: int, order: Optional[torch.Tensor],
                       rows_km: Optional[torch.Tensor], order_offset: int = 0, table: Optional[torch.Tensor] = None,
                       rows_sm: Optional[torch.Tensor] = None, cvt=None, table_rows: int = 0):
    """tt_batch_ingest_store: the batch `order[order_offset : order_offset + B]` of the pair list gathered out of the device
    stores straight into the step's static buffers (+ key-major fused rows, + the copy segments `pairs`), one launch.
    table given (and sides[i].out set): the launch also looks the batch's rows up into sides[i].out (tt_batch_ingest_store_lookup).
    Without `order` the entity view must hold the batch (B entries at its stride); a pair list or offset that does not is a
    ValueError here, not an out-of-bounds read on the device (the reference raises IndexError / KeyError:
    unified_bid_data_loader.py:495-498); entity indices are clamped into the store by the kernel (tt_store_side.n_rows)."""
    dev = stores[0].dense_out.device
    for i, t in enumerate(stores):
        if t.entity.dtype != torch.int64 or t.entity.dim() != 1 or t.entity_stride < 1 or t.entity.device != dev:
            raise ValueError(f"batch_ingest_store: store {i}: entity must be a 1-D int64 view on {dev}")
        need = (B - 1) * t.entity_stride + 1 if order is None else 1
        if t.entity.numel() < need:
            raise ValueError(f"batch_ingest_store: store {i}: the batch runs past the pair list ({t.entity.numel()} entries, {need} needed)")
    n, dst, src, nb = _copy_segments(pairs, "batch_ingest_store")
    arr, M = _embed_sides(sides, B, dev, "batch_ingest_store", False, table is not None)
    st = (L.StoreSide * len(sides))()
    for i, (s, t) in enumerate(zip(sides, stores)):
        dd = t.dense_store.shape[1]
        if t.cat_store.dtype != torch.int64 or t.cat_store.shape[1] != s.K or not t.cat_store.is_contiguous() or \
                t.dense_store.dtype != torch.float32 or not t.dense_store.is_contiguous() or t.entity.dtype != torch.int64:
            raise ValueError(f"batch_ingest_store: store {i}: need contiguous f32 [N, D] features and int64 [N, {s.K}] ids")
        if t.dense_out.shape != (B, dd) or not t.dense_out.is_contiguous() or t.dense_out.dtype != torch.float32 or \
                t.ids_out.numel() != B * s.K or t.ids_out.dtype != torch.int64 or not t.ids_out.is_contiguous():
            raise ValueError(f"batch_ingest_store: side {i}: static buffers must be contiguous f32 [{B}, {dd}] and int64 [{B * s.K}]")
        st[i] = L.StoreSide(L.ptr(t.entity), t.entity_stride, L.ptr(t.dense_store), L.ptr(t.cat_store), L.ptr(t.dense_out), L.ptr(t.ids_out), dd,
                            min(int(t.dense_store.shape[0]), 2 ** 31 - 1))
    _check_rows(rows_km, M, "batch_ingest_store", "rows_km")
    if order is not None:
        if order.dtype != torch.int64 or not order.is_contiguous() or order_offset < 0 or order_offset + B > order.numel():
            raise ValueError("batch_ingest_store: order must be a contiguous int64 tensor holding the batch's B entries")
        order_ptr = L.vp(order.data_ptr() + 8 * order_offset)
    else:
        order_ptr = L.vp(0)
    if table is not None:
        lk = _lookup_part(table)
        with _timed("tt_batch_ingest_lookup"):
            L.check(L.load().tt_batch_ingest_store_lookup(L.ctx(dev), n, dst, src, nb, arr, st, len(sides), B, order_ptr, L.ptr(rows_km),
                                                          C.byref(lk), _cvt_list(cvt), L.stream(dev)), "tt_batch_ingest_store_lookup")
        return
    _check_rows(rows_sm, M, "batch_ingest_store", "rows_sm")
    with _timed("tt_batch_ingest_store"):
        L.check(L.load().tt_batch_ingest_store(L.ctx(dev), n, dst, src, nb, arr, st, len(sides), B, order_ptr, L.ptr(rows_km), L.ptr(rows_sm),
                                               int(table_rows), _cvt_list(cvt), L.stream(dev)), "tt_batch_ingest_store")


BAG_STORE_TILE = 256          # samples per scan tile of tt_bag_store_gather (tt_bag_store_tile(): the kernel's kStoreTile)


@dataclass
class BagStoreSide:
    """One tower's device-resident bag store as the source of a batch (tt_bag_store_side)."""
    entity: torch.Tensor          # int64: entity index per pair, element [o * entity_stride]
    entity_stride: int
    dense_store: torch.Tensor     # f32 [N, dense_dim]
    offsets: torch.Tensor         # int64 [N*K + 1]
    values: torch.Tensor          # int64 [nnz]
    K: int
    dense_out: torch.Tensor       # f32 [B, dense_dim]
    lengths_out: torch.Tensor     # int64 [B*K]
    ids_out: torch.Tensor         # int64 [capacity]: the run total fills its head, the rest keeps what it held
    expect: int = -1              # the id count the host believes, or -1
    weights: Optional[torch.Tensor] = None        # f32 [nnz]: one weight per entry of `values` (None: the side moves ids alone)
    weights_out: Optional[torch.Tensor] = None    # f32 [capacity]: position for position beside ids_out


def _check_bag_store_weights(i: int, t: BagStoreSide, dev) -> None:
    """ValueError unless side i's weights / weights_out are both absent, or both contiguous f32 on `dev` with one entry per id"""
    if (t.weights is None) != (t.weights_out is None):
        raise ValueError(f"bag_store_gather: side {i}: weights and weights_out go together, "
                         f"{'weights_out' if t.weights is None else 'weights'} alone was given")
    if t.weights is None:
        return
    for name, x in (("weights", t.weights), ("weights_out", t.weights_out)):
        if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.dim() != 1 or not x.is_contiguous() or x.device != dev:
            raise ValueError(f"bag_store_gather: side {i}: {name} must be a contiguous 1-D float32 tensor on {dev}")
    if t.weights.numel() != t.values.numel():
        raise ValueError(f"bag_store_gather: side {i}: {t.weights.numel()} weights for {t.values.numel()} ids of the store")
    if t.weights_out.numel() != t.ids_out.numel():
        raise ValueError(f"bag_store_gather: side {i}: weights_out holds {t.weights_out.numel()} entries, ids_out {t.ids_out.numel()}")


def bag_store_gather(pairs, sides: Sequence[BagStoreSide], B: int, order: Optional[torch.Tensor] = None, order_offset: int = 0):
    """tt_bag_store_gather: the batch `order[order_offset : order_offset + B]` of the pair list gathered out of device-resident bag
    stores into the sample-major bag wire format (+ the copy segments `pairs`), two launches and no host round trip.  A side whose
    ids do not fit ids_out, or do not number `expect`, gets no ids and raises the device error word (_lib.check_device_errors).
    A side with `weights` also gets weights_out[p] = the weight of the id at ids_out[p], bit for bit, from the same two launches
    (tt_bag_store_gather_w; a refused side gets neither); without any such side this is the unweighted entry with its arguments."""
    dev = sides[0].dense_out.device
    weighted = False
    for i, t in enumerate(sides):
        if t.weights is not None or t.weights_out is not None:
            _check_bag_store_weights(i, t, dev)
            weighted = True
    arr = ((L.BagStoreSideW if weighted else L.BagStoreSide) * len(sides))()
    for i, t in enumerate(sides):
        if t.entity.dtype != torch.int64 or t.entity.dim() != 1 or t.entity_stride < 1 or t.entity.device != dev:
            raise ValueError(f"bag_store_gather: side {i}: entity must be a 1-D int64 view on {dev}")
        need = (B - 1) * t.entity_stride + 1 if order is None else 1
        if t.entity.numel() < need:
            raise ValueError(f"bag_store_gather: side {i}: the batch runs past the pair list ({t.entity.numel()} entries, {need} needed)")
        N, dd = t.dense_store.shape
        if t.dense_store.dtype != torch.float32 or not t.dense_store.is_contiguous() or N < 1 or \
                any(x.dtype != torch.int64 or x.dim() != 1 or not x.is_contiguous() or x.device != dev for x in (t.offsets, t.values)) or \
                t.offsets.numel() != N * t.K + 1:
            raise ValueError(f"bag_store_gather: side {i}: need contiguous f32 [N, D] features, int64 [N*{t.K} + 1] offsets and int64 ids")
        if t.dense_out.shape != (B, dd) or not t.dense_out.is_contiguous() or t.dense_out.dtype != torch.float32 or \
                t.lengths_out.numel() != B * t.K or t.lengths_out.dtype != torch.int64 or not t.lengths_out.is_contiguous() or \
                t.ids_out.dim() != 1 or t.ids_out.dtype != torch.int64 or not t.ids_out.is_contiguous():
            raise ValueError(f"bag_store_gather: side {i}: outputs must be contiguous f32 [{B}, {dd}], int64 [{B * t.K}] and a 1-D int64 id buffer")
        if weighted:
            arr[i] = L.BagStoreSideW(L.ptr(t.entity), t.entity_stride, L.ptr(t.dense_store), L.ptr(t.offsets), L.ptr(t.values), L.ptr(t.dense_out),
                                     L.ptr(t.lengths_out), L.ptr(t.ids_out), t.values.numel(), t.ids_out.numel(), int(t.expect), dd,
                                     min(int(N), 2 ** 31 - 1), t.K, 0, L.ptr(t.weights), L.ptr(t.weights_out))
            continue
        arr[i] = L.BagStoreSide(L.ptr(t.entity), t.entity_stride, L.ptr(t.dense_store), L.ptr(t.offsets), L.ptr(t.values), L.ptr(t.dense_out),
                                L.ptr(t.lengths_out), L.ptr(t.ids_out), t.values.numel(), t.ids_out.numel(), int(t.expect), dd,
                                min(int(N), 2 ** 31 - 1), t.K, 0)
    n, dst, src, nb = _copy_segments(pairs, "bag_store_gather")
    if order is not None:
        if order.dtype != torch.int64 or not order.is_contiguous() or order_offset < 0 or order_offset + B > order.numel():
            raise ValueError("bag_store_gather: order must be a contiguous int64 tensor holding the batch's B entries")
        order_ptr = L.vp(order.data_ptr() + 8 * order_offset)
    else:
        order_ptr = L.vp(0)
    lib = L.load()
    ws = L.workspace(dev, lib.tt_bag_store_gather_workspace_bytes(B, len(sides)))
    if weighted:
        with _timed("tt_bag_store_gather_w"):
            L.check(lib.tt_bag_store_gather_w(L.ctx(dev), n, dst, src, nb, arr, len(sides), B, order_ptr, L.ptr(ws), ws.numel(), L.stream(dev)),
                    "tt_bag_store_gather_w")
        return
    with _timed("tt_bag_store_gather"):
        L.check(lib.tt_bag_store_gather(L.ctx(dev), n, dst, src, nb, arr, len(sides), B, order_ptr, L.ptr(ws), ws.numel(), L.stream(dev)),
                "tt_bag_store_gather")


# ---------------------------------------------------------------------------------------------- multi-GPU routing
def route_bucket(plan: DedupPlan, G: int, C: int, pad_id: Sequence[int], pad_u: int, overflow: torch.Tensor, expand: bool = False):
    """Distinct rows of `plan` -> fixed-capacity owner buckets.  Returns (send_ids [G*C] i32, send_u [G*C] i32,
    pos_u [M] i32, counts [G] i32) -- all on the device, no host sync; `overflow` (int32 [1], caller-owned, sticky)
    is set to 1 when a bucket needed more than C entries.  expand: also idx_slot [M] int64 = pos_u[u(slot)] as a fifth
    result (tt_route_bucket_expand: route_expand's output from the same launch)."""
    dev, M = plan.unique_rows.device, plan.M
    buf = torch.empty(2 * G * C + M + G, dtype=torch.int32, device=dev)
    send_ids, send_u = buf[:G * C], buf[G * C:2 * G * C]
    pos_u, counts = buf[2 * G * C:2 * G * C + M], buf[2 * G * C + M:]
    lib = L.load()
    ws = L.workspace(dev, lib.tt_route_workspace_bytes(M, G))
    pads = (L.i32 * G)(*[int(p) for p in pad_id])
    if expand:
        idx = torch.empty(M, dtype=torch.int64, device=dev)
        with _timed("tt_route_bucket_expand"):
            L.check(lib.tt_route_bucket_expand(L.ctx(dev), L.ptr(plan.unique_rows), L.ptr(plan.n_unique), M, G, C, pads, pad_u, L.ptr(send_ids),
                                               L.ptr(send_u), L.ptr(pos_u), L.ptr(counts), L.ptr(overflow), L.ptr(ws), ws.numel(),
                                               L.ptr(plan.sorted_src), L.ptr(plan.seg_offsets), L.ptr(idx), L.stream(dev)),
                    "tt_route_bucket_expand")
        return send_ids, send_u, pos_u, counts, idx
    with _timed("tt_route_bucket"):
        L.check(lib.tt_route_bucket(L.ctx(dev), L.ptr(plan.unique_rows), L.ptr(plan.n_unique), M, G, C, pads, pad_u, L.ptr(send_ids),
                                    L.ptr(send_u), L.ptr(pos_u), L.ptr(counts), L.ptr(overflow), L.ptr(ws), ws.numel(), L.stream(dev)),
                "tt_route_bucket")
    return send_ids, send_u, pos_u, counts


def gather_rows(table: torch.Tensor, rows: torch.Tensor, out_dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """out[i] = 0 if rows[i] < 0 else table[min(rows[i], R - 1)]  (rows int32; out_dtype float32 or bfloat16)."""
    dev, n, E = table.device, rows.numel(), table.shape[1]
    out = torch.empty((n, E), dtype=out_dtype, device=dev)
    with _timed("tt_gather_rows"):
        L.check(L.load().tt_gather_rows(L.ctx(dev), L.ptr(table), table.shape[0], E, L.ptr(rows), n, L.ptr(out), _dt(out),
                                        L.stream(dev)), "tt_gather_rows")
    return out


def route_expand(plan: DedupPlan, pos_u: torch.Tensor) -> torch.Tensor:
    """idx_slot [M] int64 = pos_u[u(slot)]."""
    dev = pos_u.device
    idx = torch.empty(plan.M, dtype=torch.int64, device=dev)
    with _timed("tt_route_expand"):
        L.check(L.load().tt_route_expand(L.ctx(dev), L.ptr(plan.sorted_src), L.ptr(plan.seg_offsets), L.ptr(plan.n_unique), L.ptr(pos_u),
                                         plan.M, L.ptr(idx), L.stream(dev)), "tt_route_expand")
    return idx


def batch_gather(entity, dense_store, cat_store):
    dev, B = entity.device, entity.numel()
    dd = dense_store.shape[1] if dense_store is not None else 0
    K = cat_store.shape[1] if cat_store is not None else 0
    dense = torch.empty((B, dd), dtype=torch.float32, device=dev)
    ids = torch.empty(B * K, dtype=torch.int64, device=dev)
    L.check(L.load().tt_batch_gather(L.ctx(dev), L.ptr(entity), B, L.ptr(dense_store), dd, L.ptr(cat_store), K, L.ptr(dense),
                                     L.ptr(ids), L.stream(dev)), "tt_batch_gather")
    return dense, ids
