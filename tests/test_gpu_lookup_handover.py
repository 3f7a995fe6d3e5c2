"""The byte movers at the front of the step -- lookup from ids, lookup from precomputed rows, tt_gather_rows, the batch hand-over, the
fused hand-over + lookup and the bf16 conversion ride -- bit for bit against numpy / torch-CPU at every dispatch branch.

The expected values come from numpy and torch-CPU only: `table[rows]` by fancy index with rows from `oracle_np.unpack_clamp_ids`
plus the key offsets, `tensor.to(torch.bfloat16)` on the CPU for RNE.  No kernel path is compared with another.  Every comparison is
`np.array_equal` on integer views; where the expected bf16 value is a NaN only NaN-ness is compared.  Every output buffer the tests
hand in is pre-filled with the byte 0x5A and compared WHOLE against a CPU image of itself (sentinel everywhere, the reference where
the kernel must write), so projection columns in front of the embeddings, the gap between K*E and ld, guard rows after the last
sample and guard elements behind a conversion or copy destination are all part of every assert.

Which case runs which kernel (csrc/tt_embed.hip lookup_fwd_impl / TT_INGEST_LOOKUP_FN / batch_ingest*_kernel, csrc/tt_route.hip):

  lookup_wave_kernel<C, 64, W, ROWS>, C = E/4 (h0 = leading projection columns: 16 -> 8-element aligned, 4 -> 4-element aligned)
    <1, 64, 1, false>                       test_lookup_ids_dispatch[E=4, h0 in {16, 4}]; capped grid: test_lookup_capped_wave[4-...]
    <C, 64, 2, false>, C = 2 4 8 16 32 64   test_lookup_ids_dispatch[E = 8 16 32 64 128 256, h0=16]; capped: test_lookup_capped_wave[16-bf16-16-ids]
    <C, 64, 1, false>, C = 2 4 8 16 32 64   test_lookup_ids_dispatch[E = 8 .. 256, h0=4]; test_lookup_sides[mixed-16-4] (the weaker side
                                            decides); capped: test_lookup_capped_wave[16-bf16-4-ids]
    <1, 64, 1, true>                        test_lookup_rows_dispatch[E=4, h0 in {16, 4}]
    <C, 64, 2, true>,  C = 2 .. 64          test_lookup_rows_dispatch[E = 8 .. 256, h0=16]; capped: test_lookup_capped_wave[16-bf16-16-rows]
    <C, 64, 1, true>,  C = 2 .. 64          test_lookup_rows_dispatch[E = 8 .. 256, h0=4]
  lookup_kernel<4, 4>                       test_lookup_ids_dispatch[E in {12, 24, 260}, h0 in {16, 4}]; test_lookup_sides[.., E=12];
                                            capped: test_lookup_capped_tasks[12]
  lookup_kernel<1, 4>                       test_lookup_ids_dispatch[E in {6, 5}, any h0] and [any E, h0=3] (misalignment);
                                            test_lookup_sides[mixed-16-3]; rows-only mode (table=None): test_lookup_rows_only;
                                            capped: test_lookup_capped_tasks[6]
  tt_embed_lookup_rows_fwd refusals         test_lookup_rows_refused (E = 12, E = 260, unaligned output: error code, no launch)
  gather_rows_kernel<false> / <true>        test_gather_rows_matrix[f32 / bf16]; capped grid: test_gather_rows_capped
  batch_ingest_kernel                       test_cvt_ride_*[batch], test_handover_beside_real_work[batch]
  batch_ingest_store_kernel<true>           test_cvt_ride_*[store], test_fused_dense_widths[dims=(0, 8)] (its no-table launch)
  batch_ingest_store_kernel<false>          test_fused_dense_widths[dims=(7, 5)] (its no-table launch)
  ingest_lookup_kernel<LPR, false, true>    LPR = E/8: 1 and 8 test_fused_k_boundaries[E = 8 / 64]; 2 and 4 test_fused_dense_widths[E = 16 / 32]
  ingest_lookup_kernel<LPR, true, true>     1 and 8 test_fused_k_boundaries; 1 2 4 8 test_fused_dense_widths[dims=(0, 8), E = 8 16 32 64]
  ingest_lookup_kernel<LPR, true, false>    1 2 4 8 test_fused_dense_widths[dims=(7, 5), E = 8 16 32 64]
  cvt_role                                  test_cvt_ride_counts (scalar tail, zero count, capped body), _eight_segments, _refused,
                                            test_handover_beside_real_work; special values: test_bf16_rounding_special_values
  dense_rows_role / copy_segment_role strided over a capped grid:  test_fused_capped_dense_rows
  store_entity clamp, three and four sides: test_fused_entity_clamp

Measured on an MI355X: the whole file, 352 cases, takes 5.7 s; no case takes longer than 0.2 s (the capped-grid ones 0.02 - 0.07 s).
"""
import numpy as np
import pytest
import torch

import oracle_np as O

from jodalrob_twotower_amd import _lib as _L
from test_gpu_parity import DEV, ctx_option, tt  # noqa: F401  (tt: the module fixture)

pytestmark = pytest.mark.gpu

GUARD = 3                      # guard rows behind the last sample
SENT = 0x5A                    # every byte of an output buffer before the launch
I64_MIN, I64_MAX = int(np.iinfo(np.int64).min), int(np.iinfo(np.int64).max)
I32_MIN, I32_MAX = int(np.iinfo(np.int32).min), int(np.iinfo(np.int32).max)
BF16, F32 = torch.bfloat16, torch.float32
_INT_VIEW = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def _esz(dtype):
    return torch.empty(0, dtype=dtype).element_size()


def _sent(shape, dtype, device):
    n = int(np.prod(shape)) if len(shape) else 1
    return torch.full((n * _esz(dtype),), SENT, dtype=torch.uint8, device=device).view(dtype).view(*shape)


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(_INT_VIEW[t.element_size()]).numpy()


def _assert_same(got, exp, what=""):
    """bitwise; where the expected bf16 value is a NaN, any NaN"""
    got = got.detach().cpu()
    assert got.shape == exp.shape and got.dtype == exp.dtype, what
    g, e = _bits(got), _bits(exp)
    if exp.dtype == BF16:
        nan = torch.isnan(exp).numpy()
        if nan.any():
            assert torch.isnan(got).numpy()[nan].all(), f"{what}: a NaN did not stay a NaN"
            g, e = np.where(nan, 0, g), np.where(nan, 0, e)
    if not np.array_equal(g, e):
        bad = np.argwhere(g != e)
        i = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {g.size} elements differ, first at {i}: got {int(g[i]):#x}, want {int(e[i]):#x}")


class _Buf:
    """an output buffer full of sentinel bytes on the device and its expected image on the CPU"""

    def __init__(self, shape, dtype):
        self.dev = _sent(shape, dtype, DEV)
        self.exp = _sent(shape, dtype, "cpu")

    def check(self, what):
        _assert_same(self.dev, self.exp, what)

    def untouched(self):
        return bool((_bits(self.dev).view(np.uint8) == SENT).all())


def _ld(h0, ke):
    """row stride with at least one gap element behind K*E, in the alignment class of h0: 8-element, 4-element only, or odd"""
    m, r = (8, 0) if h0 % 8 == 0 else ((8, 4) if h0 % 4 == 0 else (2, 1))
    ld = h0 + ke + 1
    while ld % m != r:
        ld += 1
    return ld


def _offsets(vocabs):
    offs, rows = [], 0
    for v in vocabs:
        offs.append((np.concatenate([[0], np.cumsum(v)[:-1]]) + rows).astype(np.int64) if len(v) else np.zeros(0, np.int64))
        rows += int(sum(v))
    return offs, max(rows, 1)


def _ids(rng, vocab, B):
    """uniform in [-3, vocab + 3) with 0, vocab - 1, vocab, -1, INT64_MIN and INT64_MAX planted per key"""
    if len(vocab) == 0:
        return np.zeros((B, 0), np.int64)
    ids = np.stack([rng.integers(-3, v + 3, B) for v in vocab], axis=1).astype(np.int64)
    j = 0
    for k, v in enumerate(vocab):
        for s in (0, v - 1, v, -1, I64_MIN, I64_MAX):
            ids[j % B, k] = s
            j += 1
    return ids


def _rows(ids, vocab, off):
    if len(vocab) == 0:
        return np.zeros((ids.shape[0], 0), np.int64)
    return O.unpack_clamp_ids(ids.reshape(-1), vocab) + off[None, :]


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


# ============================================================================================== 1 + 2: the lookup
def _lookup_case(ops, E, specs, B, seed, mode="ids", table_np=None, ids_list=None):
    """specs: [(vocab, h0, out dtype)] per side.  mode: ids (tt_embed_lookup_fwd, rows returned) / rows (tt_embed_lookup_rows_fwd, the
    rows from the reference)."""
    rng = np.random.default_rng(seed)
    vocabs = [s[0] for s in specs]
    offs, R = _offsets(vocabs)
    if table_np is None:
        table_np = rng.standard_normal((R, E)).astype(np.float32)
    table = _dev(table_np)
    sides, bufs, rows_all = [], [], []
    for i, ((vocab, h0, dt), off) in enumerate(zip(specs, offs)):
        K = len(vocab)
        ids = ids_list[i] if ids_list is not None else _ids(rng, vocab, B)
        rows = _rows(ids, vocab, off)
        rows_all.append(rows.reshape(-1))
        buf = _Buf((B + GUARD, _ld(h0, K * E)), dt)
        if K:
            buf.exp[:B, h0:h0 + K * E] = torch.from_numpy(table_np[rows.reshape(-1)].reshape(B, K * E)).to(dt)
        bufs.append(buf)
        out = buf.dev[:B, h0:h0 + K * E]
        if mode == "ids":
            sides.append(ops.LookupSide(_dev(ids.reshape(-1)), _dev(off), _dev(np.asarray(vocab, np.int64)), out, K))
        else:
            sides.append(ops.LookupSide(None, None, None, out, K))
    exp_rows = np.concatenate(rows_all).astype(np.int32)
    if mode == "ids":
        got_rows = ops.embed_lookup(table, sides, B, want_rows=True)
        assert np.array_equal(got_rows.cpu().numpy(), exp_rows), "returned rows"
    else:
        ops.embed_lookup_rows(table, _dev(exp_rows), sides, B)
    torch.cuda.synchronize()
    for i, b in enumerate(bufs):
        b.check(f"side {i}")
    _L.check_device_errors(torch.device(DEV))                  # every row lay in the table: the error word stays clear
    return exp_rows


_V2 = [[12, 300, 7], [1, 64, 5, 9, 33]]                        # two sides, K = 3 and 5, one key with vocab = 1
_DT = {"f32": F32, "bf16": BF16}


@pytest.mark.parametrize("h0", [16, 4, 3])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("E", [4, 8, 16, 32, 64, 128, 256, 12, 24, 260, 6, 5])
def test_lookup_ids_dispatch(tt, E, dt, h0):
    """B = 67: 536 slots = 8 whole 64-slot chunks and a partial ninth, the side boundary at slot 201 inside a chunk."""
    from jodalrob_twotower_amd import ops
    _lookup_case(ops, E, [(v, h0, _DT[dt]) for v in _V2], 67, seed=E * 100 + h0)


@pytest.mark.parametrize("h0", [16, 4])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("E", [4, 8, 16, 32, 64, 128, 256])
def test_lookup_rows_dispatch(tt, E, dt, h0):
    from jodalrob_twotower_amd import ops
    _lookup_case(ops, E, [(v, h0, _DT[dt]) for v in _V2], 67, seed=E * 100 + h0 + 1, mode="rows")


_SIDES = {
    "one": [([9, 4, 700], 16, BF16)],
    "two-K1": [([40], 16, F32), ([3, 17], 16, BF16)],                                      # a K = 1 side; f32 beside bf16
    "four": [([5, 11, 2], 16, BF16), ([], 16, F32), ([90], 16, F32), ([6, 1, 8, 3, 21, 4, 2], 16, BF16)],   # TT_MAX_SIDES, a K = 0 side
    "four-4al": [([5, 11, 2], 4, BF16), ([], 4, F32), ([90], 4, F32), ([6, 1, 8, 3, 21, 4, 2], 4, BF16)],
    "mixed-16-4": [([12, 300, 7], 16, BF16), ([64, 5], 4, BF16)],                          # the weaker side decides: W = 1 for both
    "mixed-4-16": [([12, 300, 7], 4, F32), ([64, 5], 16, BF16)],
    "mixed-16-3": [([12, 300, 7], 16, F32), ([64, 5], 3, BF16)],                           # ... the scalar kernel for both
}


# every side set from ids at a wave width, at lookup_kernel<4>'s and at lookup_kernel<1>'s; from precomputed rows where that entry takes the shape
_SIDE_CASES = [(n, E, "ids") for n in _SIDES for E in (16, 12, 6)] + [(n, 16, "rows") for n in _SIDES if n != "mixed-16-3"]


@pytest.mark.parametrize("name,E,mode", _SIDE_CASES)
def test_lookup_sides(tt, name, E, mode):
    from jodalrob_twotower_amd import ops
    _lookup_case(ops, E, _SIDES[name], 70, seed=E + len(name), mode=mode)


@pytest.mark.parametrize("K", [1, 3, 7])
@pytest.mark.parametrize("B", [1, 63, 65, 257])
@pytest.mark.parametrize("E,dt,h0", [(4, "f32", 4), (32, "bf16", 16), (8, "bf16", 4), (12, "f32", 16), (6, "bf16", 3)])
def test_lookup_small_shapes(tt, E, dt, h0, B, K):
    """a partial first chunk, a partial last one, and (second side, K = 3) a chunk that straddles two sides"""
    from jodalrob_twotower_amd import ops
    vocab = [17, 1, 250, 9, 4, 33, 1000][:K]
    _lookup_case(ops, E, [(vocab, h0, _DT[dt]), ([5, 64, 2], h0, _DT[dt])], B, seed=B * 10 + K)


@pytest.mark.parametrize("B,vocabs", [(65, [[12, 300, 7], [1, 64]]), (300, [[9], [5, 5, 5, 800]])])
def test_lookup_rows_only(tt, B, vocabs):
    """table=None: the rows alone (lookup_kernel<1, 4> without a table)"""
    from jodalrob_twotower_amd import ops
    rng = np.random.default_rng(B)
    offs, R = _offsets(vocabs)
    sides, exp = [], []
    for v, off in zip(vocabs, offs):
        ids = _ids(rng, v, B)
        exp.append(_rows(ids, v, off).reshape(-1))
        sides.append(ops.LookupSide(_dev(ids.reshape(-1)), _dev(off), _dev(np.asarray(v, np.int64)), None, len(v)))
    got = ops.embed_lookup(None, sides, B, want_rows=True, E=32, table_rows=R)
    assert np.array_equal(got.cpu().numpy(), np.concatenate(exp).astype(np.int32))


@pytest.mark.parametrize("E,dt,h0,mode", [(4, "f32", 16, "ids"), (16, "bf16", 16, "ids"), (16, "bf16", 4, "ids"), (16, "bf16", 16, "rows")])
def test_lookup_capped_wave(tt, E, dt, h0, mode):
    """More 64-slot chunks than the capped grid has waves (num_cus * 16 workgroups of 4), a quarter of them more, and a ragged last
    chunk: a wave goes round its chunk loop twice and reuses its LDS records."""
    from jodalrob_twotower_amd import ops
    cap_slots = _L.num_cus(torch.device(DEV)) * 16 * 4 * 64
    B = ((cap_slots * 5 // 4) // 4) | 1                        # 4 slots per sample (K = 3 + 1), 4 * B not a multiple of 64
    assert 4 * B > cap_slots and (4 * B) % 64 != 0
    _lookup_case(ops, E, [([5000, 7, 300], h0, _DT[dt]), ([64], h0, _DT[dt])], B, seed=E, mode=mode)


@pytest.mark.parametrize("E", [6, 12])
def test_lookup_capped_tasks(tt, E):
    """lookup_kernel<1> (E = 6) / lookup_kernel<4> (E = 12): more (slot, chunk) tasks than num_cus * 8 * 256 threads x 4 tasks, so a
    thread goes round `base += stride * U` twice; ragged count."""
    from jodalrob_twotower_amd import ops
    cap_tasks = _L.num_cus(torch.device(DEV)) * 8 * 256 * 4
    C = E if E == 6 else E // 4
    B = ((cap_tasks * 5 // 4) // C // 4) | 1
    assert 4 * B * C > cap_tasks + 1024
    _lookup_case(ops, E, [([5000, 7, 300], 3 if E == 6 else 4, BF16), ([64], 3 if E == 6 else 4, BF16)], B, seed=E)


def test_lookup_rows_refused(tt):
    """tt_embed_lookup_rows_fwd refuses E = 12, E = 260 and an output that is not 4-element aligned: an error code and no launch"""
    from jodalrob_twotower_amd import ops
    lib = _L.load()
    B, vocab = 9, [5, 7]
    for E, h0 in ((12, 16), (260, 16), (8, 3)):
        table = torch.zeros((12, E), device=DEV)
        buf = _Buf((B + GUARD, _ld(h0, 2 * E)), F32)
        rows = torch.zeros(B * 2, dtype=torch.int32, device=DEV)
        torch.cuda.synchronize()
        n0 = lib.tt_launch_count()
        with pytest.raises(_L.TwoTowerHipError):
            ops.embed_lookup_rows(table, rows, [ops.LookupSide(None, None, None, buf.dev[:B, h0:h0 + 2 * E], 2)], B)
        assert lib.tt_launch_count() == n0, (E, h0)
        torch.cuda.synchronize()
        assert buf.untouched(), (E, h0)


# ============================================================================================== 3: tt_gather_rows
def _gather(table_np, idx_np, odt):
    """tt_gather_rows through the C ABI into a sentinel buffer with guard rows; reference: zero row for a negative index, else
    table[min(index, R - 1)]"""
    dev = torch.device(DEV)
    R, E = table_np.shape
    n = idx_np.size
    table, idx = _dev(table_np), _dev(idx_np.astype(np.int32))
    buf = _Buf((n + GUARD, E), odt)
    exp = table_np[np.clip(idx_np.astype(np.int64), 0, R - 1)]
    exp[idx_np < 0] = 0.0
    buf.exp[:n] = torch.from_numpy(exp).to(odt)
    _L.check(_L.load().tt_gather_rows(_L.ctx(dev), _L.ptr(table), R, E, _L.ptr(idx), n, _L.ptr(buf.dev), _L.TT_BF16 if odt == BF16 else _L.TT_F32,
                                      _L.stream(dev)), "tt_gather_rows")
    torch.cuda.synchronize()
    buf.check(f"gather E={E} n={n}")


def _gather_idx(rng, n, R):
    idx = rng.integers(-5, R + 5, n).astype(np.int64)
    for j, s in enumerate((-1, I32_MIN, R - 1, R, I32_MAX)):
        if j < n:
            idx[(j * 7919) % n] = s
    return idx


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("E", [4, 12, 32, 260])
def test_gather_rows_matrix(tt, E, dt):
    rng = np.random.default_rng(E)
    R = 1000
    table = rng.standard_normal((R, E)).astype(np.float32)
    for s in (-1, I32_MIN, R - 1, R, I32_MAX, 0):              # n = 1, each edge index on its own
        _gather(table, np.array([s], np.int64), _DT[dt])
    _gather(table, _gather_idx(rng, 4097, R), _DT[dt])


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_gather_rows_capped(tt, dt):
    """more 16-byte pieces than grid_for's num_cus * 8 * 256 threads: the grid-stride loop goes round twice, ragged"""
    rng = np.random.default_rng(11)
    n = _L.num_cus(torch.device(DEV)) * 8 * 256 * 5 // 4 + 37
    table = rng.standard_normal((777, 4)).astype(np.float32)
    _gather(table, _gather_idx(rng, n, 777), _DT[dt])


# ============================================================================================== 4 + 5: the hand-over
ENTRIES = {"batch": (False, False), "batch+lookup": (False, True), "store": (True, False), "store+lookup": (True, True)}


def _handover(ops, *, store, with_table, Ks, B, E=8, odt=BF16, dims=None, h0=16, copy_bytes=(), cvt_counts=(), cvt_align=0, want_km=True,
              use_order=True, bad_entities=False, seed=0, vocabs=None, table_np=None, cvt_src=None, refused=None):
    """One hand-over launch through ops.batch_ingest / ops.batch_ingest_store (with_table: the fused hand-over + lookup) checked
    against numpy: x, rows_km (and rows_sm without the table), the static ids and dense buffers from the stores, the copies, the
    conversions.  refused: the exception the call must raise -- then nothing may be launched and every buffer keeps its sentinel."""
    rng = np.random.default_rng(seed)
    dev = torch.device(DEV)
    n = len(Ks)
    vocabs = vocabs or [[int(v) for v in rng.integers(1, 500, K)] for K in Ks]
    offs, R = _offsets(vocabs)
    dims = dims or tuple(4 * (i + 1) for i in range(n))
    bufs = []

    def buf(shape, dtype, what):
        b = _Buf(shape, dtype)
        bufs.append((what, b))
        return b

    table = None
    if with_table:
        if table_np is None:
            table_np = rng.standard_normal((R, E)).astype(np.float32)
        table = _dev(table_np)
    # ---- the batch: ids from the caller, or entity rows of the stores through the pair list
    stores, order_t, lo = [], None, B + 3
    if store:
        N = [137 + 11 * i for i in range(n)]
        cat = [np.stack([rng.integers(-3, v + 3, N[i]) for v in vocabs[i]], axis=1).astype(np.int64) for i in range(n)]
        for i in range(n):
            cat[i][0, 0], cat[i][1, 0] = I64_MIN, I64_MAX
        dense = [rng.standard_normal((N[i], dims[i])).astype(np.float32) for i in range(n)]
        P = 3 * B + 17
        pairs = np.stack([rng.integers(0, N[i], P) for i in range(n)], axis=1).astype(np.int64)
        order = rng.permutation(P).astype(np.int64) if use_order else None
        sel = order[lo:lo + B] if use_order else np.arange(lo, lo + B)
        if bad_entities:                                        # outside the store: clamped by store_entity, as the reference index is here
            for i in range(n):
                pairs[sel[0], i] = -1 if i % 2 == 0 else N[i] + 5
                pairs[sel[-1], i] = N[i] + 5 if i % 2 == 0 else -1
        ent = [np.clip(pairs[sel, i], 0, N[i] - 1) for i in range(n)]
        ids = [cat[i][ent[i]] for i in range(n)]
        flat = _dev(pairs).view(-1)
        order_t = _dev(order) if use_order else None
        base_el = 0 if use_order else n * lo
        for i in range(n):
            d_out = buf((B + GUARD, dims[i]), F32, f"dense_out {i}")
            d_out.exp[:B] = torch.from_numpy(dense[i][ent[i]])
            i_out = buf((B * Ks[i] + GUARD,), torch.int64, f"ids_out {i}")
            i_out.exp[:B * Ks[i]] = torch.from_numpy(ids[i].reshape(-1))
            stores.append(ops.StoreSide(flat[base_el + i:], n, _dev(dense[i]), _dev(cat[i]), d_out.dev[:B], i_out.dev[:B * Ks[i]]))
    else:
        ids = [_ids(rng, vocabs[i], B) for i in range(n)]
    rows = [_rows(ids[i], vocabs[i], offs[i]) for i in range(n)]
    M = B * sum(Ks)
    # ---- outputs and what they must hold
    sides = []
    for i in range(n):
        out = None
        if with_table:
            x = buf((B + GUARD, _ld(h0, Ks[i] * E)), odt, f"x {i}")
            x.exp[:B, h0:h0 + Ks[i] * E] = torch.from_numpy(table_np[rows[i].reshape(-1)].reshape(B, Ks[i] * E)).to(odt)
            out = x.dev[:B, h0:h0 + Ks[i] * E]
        sides.append(ops.LookupSide(None if store else _dev(ids[i].reshape(-1)), _dev(offs[i]), _dev(np.asarray(vocabs[i], np.int64)), out, Ks[i]))
    want_km = want_km or (not store and not with_table)         # tt_batch_ingest always writes the key-major rows
    km = sm = None
    if want_km:
        km = buf((M + GUARD,), torch.int32, "rows_km")
        km.exp[:M] = torch.from_numpy(np.concatenate([r.T.reshape(-1) for r in rows]).astype(np.int32))     # [side][key][sample]
    if not with_table:
        sm = buf((M + GUARD,), torch.int32, "rows_sm")
        sm.exp[:M] = torch.from_numpy(np.concatenate([r.reshape(-1) for r in rows]).astype(np.int32))       # [side][sample][key]
    copies = []
    for j, nb in enumerate(copy_bytes):
        src = rng.integers(0, 256, nb, dtype=np.uint8)
        c = buf((nb + 16 * GUARD,), torch.uint8, f"copy {j}")
        c.exp[:nb] = torch.from_numpy(src)
        copies.append((c.dev[:nb], _dev(src)))
    cvts = []
    for j, cnt in enumerate(cvt_counts):
        src = cvt_src[j] if cvt_src is not None else rng.standard_normal(cnt).astype(np.float32)
        assert src.size == cnt
        c = buf((cvt_align + cnt + 16,), BF16, f"cvt {j} (count {cnt})")
        if refused is None:
            c.exp[cvt_align:cvt_align + cnt] = torch.from_numpy(src).to(BF16)
        cvts.append((c.dev[cvt_align:cvt_align + cnt], _dev(src)))
    kw = dict(table=table, cvt=cvts or None)
    if not with_table:
        kw.update(rows_sm=sm.dev[:M], table_rows=R)

    def call():
        if store:
            ops.batch_ingest_store(copies, sides, stores, B, order_t, km.dev[:M] if km else None, lo if use_order else 0, **kw)
        else:
            ops.batch_ingest(copies, sides, B, km.dev[:M] if km else None, **kw)

    if refused is not None:
        torch.cuda.synchronize()
        n0 = _L.load().tt_launch_count()
        with pytest.raises(refused):
            call()
        assert _L.load().tt_launch_count() == n0, "a refused hand-over launched something"
        torch.cuda.synchronize()
        assert all(b.untouched() for _, b in bufs)
        return None
    call()
    torch.cuda.synchronize()
    for what, b in bufs:
        b.check(what)
    _L.check_device_errors(dev)
    return rows


_CVT_BIG = "capped"


@pytest.mark.parametrize("align", [0, 4])                      # destination 16-byte aligned / 8- but not 16-byte aligned (legal)
@pytest.mark.parametrize("count", [0, 1, 3, 4, 5, 4099, _CVT_BIG])
@pytest.mark.parametrize("entry", list(ENTRIES))
def test_cvt_ride_counts(tt, entry, count, align):
    """The conversion beside the smallest legal hand-over (one side, B = 1, K = 1): the scalar tail (counts 1, 3, 5, 4099), no body
    (1, 3), no tail (4), nothing (0), and a count above the capped grid's reach, where the body strides."""
    from jodalrob_twotower_amd import ops
    store, with_table = ENTRIES[entry]
    if count == _CVT_BIG:
        count = _L.num_cus(torch.device(DEV)) * 8 * 256 * 4 + 3
    _handover(ops, store=store, with_table=with_table, Ks=[1], B=1, cvt_counts=[count], cvt_align=align, seed=count % 1000 + align)


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_cvt_ride_eight_segments(tt, entry):
    """TT_MAX_CVT segments of different counts in one list"""
    from jodalrob_twotower_amd import ops
    store, with_table = ENTRIES[entry]
    assert _L.TT_MAX_CVT == 8
    _handover(ops, store=store, with_table=with_table, Ks=[1], B=1, cvt_counts=[5, 0, 4099, 1, 1024, 3, 7, 258], cvt_align=4, seed=8)


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_cvt_ride_refused(tt, entry):
    """nine segments (refused on the host) and a 4-byte-misaligned destination (refused by the entry): no launch"""
    from jodalrob_twotower_amd import ops
    store, with_table = ENTRIES[entry]
    _handover(ops, store=store, with_table=with_table, Ks=[1], B=1, cvt_counts=[4] * 9, refused=ValueError)
    _handover(ops, store=store, with_table=with_table, Ks=[1], B=1, cvt_counts=[8], cvt_align=2, refused=_L.TwoTowerHipError)


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_handover_beside_real_work(tt, entry):
    """the same conversions beside copy segments (odd byte tails) and a many-tile hand-over, B = 300 with K = [5, 2]"""
    from jodalrob_twotower_amd import ops
    store, with_table = ENTRIES[entry]
    _handover(ops, store=store, with_table=with_table, Ks=[5, 2], B=300, E=16, dims=(24, 8), copy_bytes=(4096 + 13, 48, 100001, 7),
              cvt_counts=[5, 0, 4099, 1, 1024, 3, 7, 258], seed=300)


def _tile_samples(ops, K):
    """TS of the fused launch for a side of K keys, from ops.ingest_lookup_tiles (one tile holds up to TS samples)"""
    return max(ts for ts in (8, 16, 32, 64) if ops.ingest_lookup_tiles(ts, [K]) == 1)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("E", [8, 64])
@pytest.mark.parametrize("K", [1, 7, 8, 9, 16, 17, 32, 33, 63, 64])
def test_fused_k_boundaries(tt, K, E, dt):
    """K either side of the tile-size steps (TS = 64 for K <= 8, 32 for K <= 16, 16 for K <= 32, else 8): B = 1, 9, 65 and 2 TS + 1,
    from batch tensors and from the stores; a second side (K = 2) keeps the tile bases apart"""
    from jodalrob_twotower_amd import ops
    ts = _tile_samples(ops, K)
    assert ts == (64 if K <= 8 else 32 if K <= 16 else 16 if K <= 32 else 8)
    for B in (1, 9, 65, 2 * ts + 1):
        for store in (False, True):
            _handover(ops, store=store, with_table=True, Ks=[K, 2], B=B, E=E, odt=_DT[dt], dims=(24, 8), seed=K * 1000 + B)


@pytest.mark.parametrize("E", [8, 16, 32, 64])
@pytest.mark.parametrize("dims", [(7, 5), (0, 8)])
def test_fused_dense_widths(tt, dims, E):
    """from the stores with dense widths (7, 5) -- floats, VEC = false -- and (0, 8) -- a side without dense features -- with and
    without the lookup; the launch from batch tensors at the same row width beside them"""
    from jodalrob_twotower_amd import ops
    for store, with_table in ((True, True), (True, False), (False, True)):
        _handover(ops, store=store, with_table=with_table, Ks=[6, 3], B=131, E=E, odt=BF16 if E in (8, 32) else F32, dims=dims,
                  copy_bytes=(48,), use_order=(E != 16), seed=E + dims[0])


@pytest.mark.parametrize("entry", ["batch+lookup", "store+lookup", "store"])
def test_fused_without_rows_km(tt, entry):
    from jodalrob_twotower_amd import ops
    store, with_table = ENTRIES[entry]
    _handover(ops, store=store, with_table=with_table, Ks=[9, 2], B=77, E=32, want_km=False, seed=77)


@pytest.mark.parametrize("nt", [0, 1])
@pytest.mark.parametrize("entry", ["batch+lookup", "store+lookup"])
def test_fused_lookup_nt(tt, ctx_option, entry, nt):
    """TT_OPT_LOOKUP_NT: the bf16 rows leave by non-temporal stores or not -- the same bits as the reference either way"""
    from jodalrob_twotower_amd import ops
    ctx_option(_L.TT_OPT_LOOKUP_NT, nt, 0)
    store, with_table = ENTRIES[entry]
    for E in (8, 32):
        _handover(ops, store=store, with_table=with_table, Ks=[5, 2], B=300, E=E, odt=BF16, seed=E + nt)


@pytest.mark.parametrize("with_table", [True, False])
@pytest.mark.parametrize("Ks", [[3, 1, 9], [2, 33, 1, 5]])
def test_fused_entity_clamp(tt, Ks, with_table):
    """three and four sides in one launch, from the stores; entity indices -1 and N + 5 in the pair list are clamped into the store
    (store_entity) -- the documented clamp, the reference index is clamped the same way"""
    from jodalrob_twotower_amd import ops
    for B, use_order in ((1, True), (70, True), (70, False)):
        _handover(ops, store=True, with_table=with_table, Ks=Ks, B=B, E=16, bad_entities=True, use_order=use_order, seed=len(Ks) * B)


@pytest.mark.parametrize("with_table", [True, False])
def test_fused_capped_dense_rows(tt, with_table):
    """from the stores, dense width 260: more 16-byte pieces than num_cus * 8 * 256 threads, so the dense-row role strides; in the
    same launch a copy segment of more than num_cus * 8 * 256 * 16 bytes with an odd byte tail strides too"""
    from jodalrob_twotower_amd import ops
    cus = _L.num_cus(torch.device(DEV))
    B = cus * 8 * 256 * 4 // 260 + 131
    assert B * 260 // 4 > cus * 8 * 256
    _handover(ops, store=True, with_table=with_table, Ks=[2, 1], B=B, E=8, dims=(260, 4), copy_bytes=(cus * 8 * 256 * 16 + 4096 * 16 + 13,), seed=260)


# ============================================================================================== 6: bf16 rounding on special values
_SPECIAL_BITS = [
    0x3F808000, 0x3F818000,                                    # exact ties: kept mantissa even (down), odd (up)
    0x3F807FFF, 0x3F808001, 0x3F817FFF, 0x3F818001,            # one ulp either side of each tie
    0x3FFFFFFF, 0x3FFF8000,                                    # mantissa all ones / a tie at the top of the binade: up into the next binade
    0x7F7FFFFF, 0xFF7FFFFF,                                    # +-FLT_MAX: rounds to infinity
    0x7F7F7FFF, 0x7F7F8000,                                    # the largest value that stays finite; the tie above it (to infinity)
    0x00000000, 0x80000000,                                    # +-0
    0x7F800000, 0xFF800000,                                    # +-inf
    0x7FC00000, 0x7F800001,                                    # a quiet NaN; a NaN whose payload lies in the dropped bits only
    0x00000001, 0x007FFFFF, 0x00800000,                        # smallest and largest f32 denormal, smallest normal
    0x00010000, 0x80010000, 0x807FFFFF,                        # denormals that bf16 holds exactly; the negative denormal of largest magnitude
]


def _special_table(E):
    """24 rows x E: row r, column c holds special (r + c) % 24 -- every column position sees every value"""
    s = np.array(_SPECIAL_BITS, np.uint32)
    assert s.size == 24
    return s[(np.arange(24)[:, None] + np.arange(E)[None, :]) % 24].view(np.float32)


def test_special_value_reference_is_what_it_claims():
    """the CPU conversion on the planted patterns (no GPU involved): ties to even, the binade step, overflow to infinity, NaN"""
    got = torch.from_numpy(np.array(_SPECIAL_BITS[:12], np.uint32).view(np.float32)).to(BF16).view(torch.int16).numpy().view(np.uint16)
    assert list(got) == [0x3F80, 0x3F82, 0x3F80, 0x3F81, 0x3F81, 0x3F82, 0x4000, 0x4000, 0x7F80, 0xFF80, 0x7F7F, 0x7F80]
    assert torch.isnan(torch.from_numpy(np.array(_SPECIAL_BITS[16:18], np.uint32).view(np.float32)).to(BF16)).all()


@pytest.mark.parametrize("path", ["wave-W2", "wave-W1", "wave-C1", "vec4", "scalar", "scalar-unaligned", "rows-W2", "gather"])
def test_bf16_rounding_special_values_lookup(tt, path):
    from jodalrob_twotower_amd import ops
    E, h0, mode = {"wave-W2": (8, 16, "ids"), "wave-W1": (8, 4, "ids"), "wave-C1": (4, 16, "ids"), "vec4": (12, 16, "ids"), "scalar": (6, 16, "ids"),
                   "scalar-unaligned": (8, 3, "ids"), "rows-W2": (32, 16, "rows"), "gather": (4, 0, None)}[path]
    table = _special_table(E)
    if path == "gather":
        for odt in (BF16, F32):
            _gather(table, np.arange(-1, 25, dtype=np.int64), odt)
        return
    ids = [np.arange(24, dtype=np.int64).reshape(24, 1)]
    for odt in (BF16, F32):                                    # (f32: the copy keeps every bit, NaN payloads and denormals included)
        rows = _lookup_case(ops, E, [([24], h0, odt)], 24, seed=1, mode=mode, table_np=table, ids_list=ids)
        assert np.array_equal(rows, np.arange(24))


@pytest.mark.parametrize("nt", [0, 1])
@pytest.mark.parametrize("entry", ["batch+lookup", "store+lookup"])
def test_bf16_rounding_special_values_fused(tt, ctx_option, entry, nt):
    from jodalrob_twotower_amd import ops
    ctx_option(_L.TT_OPT_LOOKUP_NT, nt, 0)
    store, with_table = ENTRIES[entry]
    for E in (8, 32):
        rows = _handover(ops, store=store, with_table=with_table, Ks=[2], B=200, E=E, odt=BF16, vocabs=[[12, 12]], table_np=_special_table(E), seed=E)
        assert len(np.unique(rows[0])) == 24                   # every row of the table was looked up


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_bf16_rounding_special_values_cvt(tt, entry):
    """every special value through cvt_role's 16-byte body (one segment of 24) and through its scalar tail (eight segments of 3)"""
    from jodalrob_twotower_amd import ops
    store, with_table = ENTRIES[entry]
    s = np.array(_SPECIAL_BITS, np.uint32).view(np.float32)
    _handover(ops, store=store, with_table=with_table, Ks=[1], B=1, cvt_counts=[24], cvt_src=[s.copy()])
    _handover(ops, store=store, with_table=with_table, Ks=[1], B=1, cvt_counts=[3] * 8, cvt_src=[s[3 * j:3 * j + 3].copy() for j in range(8)])
