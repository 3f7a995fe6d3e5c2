// The batch gather out of a device-resident store of per-entity bags (tt_bag_store_gather) on gfx950: B entity indices -> the
// sample-major bag wire format (dense rows, [B*K] lengths, the samples' id runs packed behind one another) without a host round
// trip.  A store keeps an entity's K bags as ONE contiguous run of ids (CSR over (entity, key) slots), so a batch's values() is
// the concatenation of its entities' runs at the exclusive prefix sum of the runs' lengths -- the offsets tt_bag_prepare forms
// again inside the captured graph.  Two launches, no workgroup waits on another (as tt_bag_prepare): the first writes the
// lengths, the dense rows, the copy segments and one total per tile of kStoreTile samples; every workgroup of the second adds up
// its side's earlier totals, scans its own tile and copies its share of the tile's ids.  tt_bag_store_gather_w: a store that keeps
// one f32 weight per id; the second launch's weighted instantiation moves the weights with the ids, bit for bit.
#include "tt_common.h"
#include "tt_embed_slots.h"
#include "tt_copy_role.h"
#include "tt_bag_store_piece.h"

namespace {

static_assert(kStoreTile == kThreads, "one sample per thread (kStoreTile: tt_bag_store_piece.h)");
constexpr int kStoreTrip = 4;                         // 16-byte pieces per thread and trip: all their loads before the first store
constexpr int kStoreMaxSplit = 16;                    // workgroups that share one tile's ids, at most
constexpr int64_t kStoreBad = (int64_t)1 << 62;       // a tile that met a run outside [0, nnz]: larger than any sum of real runs

struct BagStoreSide {
  const int64_t* entity;
  int64_t entity_stride;
  const float* dense_store;
  const int64_t* offs;
  const int64_t* values;
  float* dense_out;
  int64_t* lengths_out;
  int64_t* ids_out;
  int64_t nnz;
  int64_t capacity;
  int64_t expect;
  int32_t dense_dim;
  int32_t n_rows;
  int32_t K;
  uint32_t tile_base;        // first tile of this side
};

struct BagStoreArgs {
  CopyArgs c;
  BagStoreSide s[TT_MAX_SIDES];
  const int64_t* order;
  int64_t* tile_sum;         // [tiles]
  uint32_t* dev_err;
  int32_t n_copy, n_sides, B;
  uint32_t tiles;
};

// the weighted pack kernel's second argument: the sides' per-id weights (NULL: this side moves ids alone).  A record of its own,
// so the unweighted kernels keep their one argument as it was.
struct BagStoreWeights {
  const uint32_t* w[TT_MAX_SIDES];       // [nnz] f32, moved as 32-bit words: bit for bit
  uint32_t* w_out[TT_MAX_SIDES];         // [capacity]
};

__device__ __forceinline__ int store_side_of(const BagStoreArgs& a, uint32_t tile) {
  int si = 0;
#pragma unroll
  for (int i = 1; i < TT_MAX_SIDES; ++i)
    if (i < a.n_sides && tile >= a.s[i].tile_base) si = i;
  return si;
}

// the store row of sample b: clamped into the store, as tt_batch_ingest_store's
__device__ __forceinline__ int64_t store_row(const BagStoreArgs& a, const BagStoreSide& s, int b) {
  const int64_t o = a.order ? a.order[b] : b;
  const int64_t e = s.entity[o * s.entity_stride];
  return e < 0 ? 0 : (e >= s.n_rows ? (int64_t)s.n_rows - 1 : e);
}

// sum over the workgroup (every thread gets it); sh: 4 words, free again on return
__device__ __forceinline__ int64_t store_block_sum(int64_t v, int64_t* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  const int64_t t = sh[0] + sh[1] + sh[2] + sh[3];
  __syncthreads();
  return t;
}

// the dense feature rows of one side: 16-byte pieces (VEC) or floats, a row's pieces on consecutive lanes
template <bool VEC>
__device__ __forceinline__ void store_dense_rows_role(const BagStoreArgs& a, const BagStoreSide& s) {
  const int dd = s.dense_dim;
  if (dd == 0) return;
  const int per = VEC ? dd / 4 : dd;
  const int64_t total = (int64_t)a.B * per, stride = (int64_t)gridDim.x * role_threads();
  for (int64_t t = (int64_t)blockIdx.x * role_threads() + threadIdx.x; t < total; t += stride) {
    const int b = (int)(t / per), j = (int)(t - (int64_t)b * per);
    const int64_t e = store_row(a, s, b);
    if (VEC) reinterpret_cast<float4*>(s.dense_out + (int64_t)b * dd)[j] = reinterpret_cast<const float4*>(s.dense_store + e * dd)[j];
    else s.dense_out[(int64_t)b * dd + j] = s.dense_store[e * dd + j];
  }
}

// Launch 1.  Grid rows: 0 = every side's tiles (lengths and the tile's total), 1 .. n_sides = the dense rows of side y - 1, then
// one row per copy segment.
template <bool VEC>
__global__ __launch_bounds__(kThreads) void bag_store_lengths_kernel(BagStoreArgs a) {
  if ((int)blockIdx.y > a.n_sides) { copy_segment_role(a.c, blockIdx.y - 1 - a.n_sides); return; }
  if (blockIdx.y >= 1) { store_dense_rows_role<VEC>(a, a.s[blockIdx.y - 1]); return; }
  if (blockIdx.x >= a.tiles) return;
  __shared__ int64_t s_ent[kStoreTile];
  __shared__ int64_t sh[4];
  const BagStoreSide& s = a.s[store_side_of(a, blockIdx.x)];
  const int K = s.K;
  const int b0 = (int)(blockIdx.x - s.tile_base) * kStoreTile;
  const int nb = min(kStoreTile, a.B - b0);
  int64_t run = 0, bad = 0;
  if ((int)threadIdx.x < nb) {
    const int64_t e = store_row(a, s, b0 + threadIdx.x);
    s_ent[threadIdx.x] = e;
    const int64_t o0 = s.offs[e * K], o1 = s.offs[(e + 1) * K];
    bad = (o0 < 0 || o1 < o0 || o1 > s.nnz) ? 1 : 0;       // nothing is read through such a run (the constructor refuses such a store)
    run = bad ? 0 : o1 - o0;
  }
  __syncthreads();
  // lengths_out[b*K + k] = offsets[e*K + k + 1] - offsets[e*K + k]: a trip's loads before its first store
  const int n = nb * K;
  for (int i0 = threadIdx.x; i0 < n; i0 += kStoreTrip * kThreads) {
    int64_t lo[kStoreTrip], hi[kStoreTrip];
#pragma unroll
    for (int j = 0; j < kStoreTrip; ++j) {
      const int i = i0 + j * kThreads;
      lo[j] = hi[j] = 0;
      if (i < n) {
        const int bl = i / K;
        const int64_t at = s_ent[bl] * K + (i - bl * K);
        lo[j] = s.offs[at];
        hi[j] = s.offs[at + 1];
      }
    }
#pragma unroll
    for (int j = 0; j < kStoreTrip; ++j) {
      const int i = i0 + j * kThreads;
      if (i < n) s.lengths_out[(int64_t)b0 * K + i] = hi[j] - lo[j];
    }
  }
  const int64_t tot = store_block_sum(run, sh);
  const int64_t anybad = store_block_sum(bad, sh);
  if (threadIdx.x == 0) a.tile_sum[blockIdx.x] = anybad ? kStoreBad : tot;
}

// Launch 2.  blockIdx.x = tile, blockIdx.y = which share of the tile's ids.  The ids move in 16-byte pieces laid on the
// DESTINATION's 16-byte grid: a piece whose two ids lie in the tile is one 16-byte store, fed by one 16-byte load when its ids are
// neighbours in the store at a 16-byte aligned address and by two 8-byte loads otherwise; a piece at the tile's edge moves 8 bytes.
// A position is found in the tile's runs by bisection, so a long run spreads over lanes and workgroups like any other.
// W: the side's per-id weights ride with the ids -- the thread that owns piece q also moves the two floats of its positions, one
// 8-byte load when the sources are neighbours at an 8-byte aligned address, one 8-byte store when both positions are live and the
// destination is 8-byte aligned, 4-byte accesses otherwise (weights and weights_out are 4-byte aligned, whatever ids_out is).
// (Wt: BagStoreWeights for W, nothing otherwise -- the unweighted instantiation takes the one argument it always took)
template <bool W, class... Wt>
__global__ __launch_bounds__(kThreads) void bag_store_pack_kernel(BagStoreArgs a, Wt... wt) {
  static_assert(sizeof...(Wt) == (W ? 1 : 0), "the weighted form takes one BagStoreWeights");
  __shared__ int64_t s_start[kStoreTile + 1];
  __shared__ int64_t s_src[kStoreTile];
  __shared__ int64_t sh[4];
  __shared__ int64_t wsum[4];
  const int si = store_side_of(a, blockIdx.x);
  const BagStoreSide& s = a.s[si];
  const uint32_t ntile = (si + 1 < a.n_sides ? a.s[si + 1].tile_base : a.tiles) - s.tile_base, tile = blockIdx.x - s.tile_base;
  // the side's total and this tile's start: integer sums, any order gives the same bits
  int64_t before = 0, all = 0, bad = 0;
  for (uint32_t t = threadIdx.x; t < ntile; t += kThreads) {
    const int64_t v = a.tile_sum[s.tile_base + t];
    bad |= v >= kStoreBad ? 1 : 0;
    all += v >= kStoreBad ? 0 : v;
    if (t < tile) before += v >= kStoreBad ? 0 : v;
  }
  before = store_block_sum(before, sh);
  all = store_block_sum(all, sh);
  bad = store_block_sum(bad, sh);
  // refused: more ids than the buffer holds, or another total than the host believes -- no id is written, the error word says so
  // (the captured tt_bag_prepare then refuses the side through its own count check)
  if (bad != 0 || all > s.capacity || (s.expect >= 0 && all != s.expect)) {
    if (tile == 0 && blockIdx.y == 0 && threadIdx.x == 0 && a.dev_err) atomicOr(a.dev_err, TT_DEVERR_BAG_OFFSETS);
    return;
  }
  const int K = s.K;
  const int b0 = (int)tile * kStoreTile;
  const int nb = min(kStoreTile, a.B - b0);
  int64_t run = 0, src = 0;
  if ((int)threadIdx.x < nb) {
    const int64_t e = store_row(a, s, b0 + threadIdx.x);
    const int64_t o0 = s.offs[e * K], o1 = s.offs[(e + 1) * K];
    src = o0;
    run = o1 - o0;
  }
  int64_t x = run;                                             // inclusive scan of the samples' runs
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int64_t y = __shfl_up(x, o);
    if (lane >= (uint32_t)o) x += y;
  }
  if (lane == 63) wsum[wave] = x;
  __syncthreads();
  int64_t start = before + x - run;
  for (uint32_t w = 0; w < wave; ++w) start += wsum[w];
  s_start[threadIdx.x] = start;
  s_src[threadIdx.x] = src;
  if (threadIdx.x == kThreads - 1) s_start[kStoreTile] = start + run;
  __syncthreads();
  const int64_t ts = s_start[0];
  const int64_t te = s_start[kStoreTile] < s.capacity ? s_start[kStoreTile] : s.capacity;      // (a total that fits ends inside the buffer)
  if (te <= ts) return;
  const int64_t A = (int64_t)((reinterpret_cast<uintptr_t>(s.ids_out) >> 3) & 1);              // ids_out is 8 mod 16: piece q holds ids 2q - 1, 2q
  const int64_t q_hi = (te - 1 + A) >> 1;
  const int64_t stride = (int64_t)gridDim.y * kThreads;
  [[maybe_unused]] const uint32_t* wsrc = nullptr;
  [[maybe_unused]] uint32_t* wdst = nullptr;
  if constexpr (W) {
    const BagStoreWeights& aw = (wt, ...);
    wsrc = aw.w[si];
    wdst = aw.w_out[si];
  }
  for (int64_t q0 = ((ts + A) >> 1) + (int64_t)blockIdx.y * kThreads + threadIdx.x; q0 <= q_hi; q0 += kStoreTrip * stride) {
    longlong2 v[kStoreTrip];
    uint2 wv[W ? kStoreTrip : 1];
    int live[kStoreTrip];
#pragma unroll
    for (int j = 0; j < kStoreTrip; ++j) {
      const int64_t q = q0 + j * stride;
      live[j] = 0;
      v[j] = make_longlong2(0, 0);
      if (q > q_hi) continue;
      int64_t p0, i0, i1;
      int lv = store_piece(s_start, s_src, ts, te, A, q, &p0, &i0, &i1);
      // (a source index outside the store cannot come out of validated runs; it is not read, and the error word says so)
      const bool in0 = (uint64_t)i0 < (uint64_t)s.nnz, in1 = (uint64_t)i1 < (uint64_t)s.nnz;
      if (((lv & 1) && !in0) || ((lv & 2) && !in1)) {
        if (a.dev_err) atomicOr(a.dev_err, TT_DEVERR_BAG_OFFSETS);
        lv = 0;
      }
      if (lv == 3 && i1 == i0 + 1 && (reinterpret_cast<uintptr_t>(s.values + i0) & 15) == 0) {
        v[j] = *reinterpret_cast<const longlong2*>(s.values + i0);
      } else {
        if (lv & 1) v[j].x = s.values[i0];
        if (lv & 2) v[j].y = s.values[i1];
      }
      if constexpr (W) {
        wv[j] = make_uint2(0, 0);
        if (wsrc) {                                                  // (lv == 0 where a source index left the store: nothing is read)
          if (lv == 3 && i1 == i0 + 1 && (reinterpret_cast<uintptr_t>(wsrc + i0) & 7) == 0) {
            wv[j] = *reinterpret_cast<const uint2*>(wsrc + i0);
          } else {
            if (lv & 1) wv[j].x = wsrc[i0];
            if (lv & 2) wv[j].y = wsrc[i1];
          }
        }
      }
      live[j] = lv;
    }
#pragma unroll
    for (int j = 0; j < kStoreTrip; ++j) {
      const int64_t p0 = 2 * (q0 + j * stride) - A;
      if (live[j] == 3) *reinterpret_cast<longlong2*>(s.ids_out + p0) = v[j];
      else if (live[j] == 1) s.ids_out[p0] = v[j].x;
      else if (live[j] == 2) s.ids_out[p0 + 1] = v[j].y;
      if constexpr (W) {
        if (wdst) {
          if (live[j] == 3 && (reinterpret_cast<uintptr_t>(wdst + p0) & 7) == 0) *reinterpret_cast<uint2*>(wdst + p0) = wv[j];
          else {
            if (live[j] & 1) wdst[p0] = wv[j].x;
            if (live[j] & 2) wdst[p0 + 1] = wv[j].y;
          }
        }
      }
    }
  }
}

// both entries: Side = tt_bag_store_side (ids alone: the kernels and arguments of old) or tt_bag_store_side_w
template <class Side>
int bag_store_gather_impl(tt_ctx* ctx, int32_t n, void* const* dst, const void* const* src, const int64_t* bytes, const Side* sides,
                          int32_t n_sides, int64_t B, const int64_t* order, void* workspace, size_t workspace_bytes, tt_stream stream) {
  constexpr bool kW = std::is_same<Side, tt_bag_store_side_w>::value;
  TT_CHECK_ARG(ctx && n >= 0 && n <= TT_MAX_COPIES && (n == 0 || (dst && src && bytes)), "tt_bag_store_gather: bad copy arguments");
  TT_CHECK_ARG(sides && workspace && n_sides >= 1 && n_sides <= TT_MAX_SIDES && B >= 1 && B < ((int64_t)1 << 31),
               "tt_bag_store_gather: bad side arguments");
  if (!tt_aligned(workspace, 8)) {
    tt_set_error("tt_bag_store_gather: the workspace must be 8-byte aligned");
    return TT_ERR_UNSUPPORTED;
  }
  if (workspace_bytes < tt_bag_store_gather_workspace_bytes(B, n_sides)) {
    tt_set_error("tt_bag_store_gather: workspace %zu < required %zu", workspace_bytes, tt_bag_store_gather_workspace_bytes(B, n_sides));
    return TT_ERR_WORKSPACE;
  }
  BagStoreArgs a{};
  BagStoreWeights aw{};
  bool weighted = false;
  int64_t mx = 0, dense_pieces = 0, tiles = 0;
  for (int i = 0; i < n; ++i) {
    TT_CHECK_ARG(bytes[i] >= 0 && (bytes[i] == 0 || (dst[i] && src[i])), "tt_bag_store_gather: segment %d NULL", i);
    TT_CHECK_ARG(tt_aligned(dst[i], 16) && tt_aligned(src[i], 16), "tt_bag_store_gather: segment %d not 16-byte aligned", i);
    a.c.dst[i] = reinterpret_cast<char*>(dst[i]);
    a.c.src[i] = reinterpret_cast<const char*>(src[i]);
    a.c.bytes[i] = bytes[i];
    mx = bytes[i] > mx ? bytes[i] : mx;
  }
  bool vec = true;
  for (int i = 0; i < n_sides; ++i) {
    const Side& t = sides[i];
    if constexpr (kW) {
      // weights and weights_out go together; as ids_out, weights_out may be NULL where capacity == 0 (and weights where nnz == 0):
      // such a side has nowhere to put a weight, or none to move, and runs as a side without weights
      const float* w = t.weights;
      float* wo = t.weights_out;
      TT_CHECK_ARG(wo || !w || t.nnz <= 0 || t.capacity == 0, "tt_bag_store_gather_w: side %d: weights without weights_out (capacity=%lld)", i,
                   (long long)t.capacity);
      TT_CHECK_ARG(w || !wo || t.nnz <= 0, "tt_bag_store_gather_w: side %d: weights_out without weights (nnz=%lld)", i, (long long)t.nnz);
      TT_CHECK_ARG(tt_aligned(w, 4) && tt_aligned(wo, 4), "tt_bag_store_gather_w: side %d weights not 4-byte aligned", i);
      if (w && wo) {
        aw.w[i] = reinterpret_cast<const uint32_t*>(w);
        aw.w_out[i] = reinterpret_cast<uint32_t*>(wo);
        weighted = true;
      }
    }
    TT_CHECK_ARG(t.K >= 1 && t.n_rows >= 1 && t.entity && t.entity_stride >= 1 && t.offsets && t.lengths_out && t.dense_dim >= 0 &&
                 (t.dense_dim == 0 || (t.dense_store && t.dense_out)), "tt_bag_store_gather: side %d NULL / bad shape", i);
    TT_CHECK_ARG(t.nnz >= 0 && t.capacity >= 0 && t.capacity < ((int64_t)1 << 31) && (t.values || t.nnz == 0) && (t.ids_out || t.capacity == 0),
                 "tt_bag_store_gather: side %d has nnz=%lld capacity=%lld", i, (long long)t.nnz, (long long)t.capacity);
    TT_CHECK_ARG(tt_aligned(t.values, 8) && tt_aligned(t.ids_out, 8) && tt_aligned(t.offsets, 8) && tt_aligned(t.lengths_out, 8),
                 "tt_bag_store_gather: side %d arrays not 8-byte aligned", i);
    TT_CHECK_ARG(B * t.K < ((int64_t)1 << 31), "tt_bag_store_gather: side %d: %lld bags exceed the 2^31 index range", i, (long long)(B * t.K));
    a.s[i] = BagStoreSide{t.entity, t.entity_stride, t.dense_store, t.offsets, t.values, t.dense_out, t.lengths_out, t.ids_out,
                          t.nnz, t.capacity, t.expect, t.dense_dim, t.n_rows, t.K, (uint32_t)tiles};
    tiles += tt_cdiv(B, kStoreTile);
    vec = vec && t.dense_dim % 4 == 0 && tt_aligned(t.dense_store, 16) && tt_aligned(t.dense_out, 16);
    const int64_t p = B * (int64_t)t.dense_dim;
    dense_pieces = p > dense_pieces ? p : dense_pieces;
  }
  a.order = order;
  a.tile_sum = reinterpret_cast<int64_t*>(workspace);
  a.dev_err = ctx->dev_err;
  a.n_copy = n;
  a.n_sides = n_sides;
  a.B = (int32_t)B;
  a.tiles = (uint32_t)tiles;
  // launch 1: the copy and dense rows stride over their work (at most 8 workgroups per CU, as tt_batch_ingest_store); row 0 holds every tile
  int64_t gx = tt_cdiv(mx / 16 + 1, kThreads);
  const int64_t rows_wg = tt_cdiv(vec ? dense_pieces / 4 : dense_pieces, kThreads);
  if (rows_wg > gx) gx = rows_wg;
  const int64_t cap = (int64_t)ctx->num_cus * 8;
  if (gx > cap) gx = cap;
  if (tiles > gx) gx = tiles;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const dim3 g1((unsigned)gx, (unsigned)(1 + n_sides + n));
  if (vec) bag_store_lengths_kernel<true><<<g1, kThreads, 0, st>>>(a);
  else bag_store_lengths_kernel<false><<<g1, kThreads, 0, st>>>(a);
  TT_LAUNCH_CHECK();
  // launch 2: the tiles' ids, every tile shared by enough workgroups to put two on each CU
  int64_t split = tt_cdiv((int64_t)ctx->num_cus * 2, tiles);
  split = split < 1 ? 1 : (split > kStoreMaxSplit ? kStoreMaxSplit : split);
  const dim3 g2((unsigned)tiles, (unsigned)split);
  if (weighted) bag_store_pack_kernel<true><<<g2, kThreads, 0, st>>>(a, aw);
  else bag_store_pack_kernel<false><<<g2, kThreads, 0, st>>>(a);
  TT_LAUNCH_CHECK();
  return TT_OK;
}

}  // namespace

extern "C" {

int tt_bag_store_tile(void) { return kStoreTile; }

size_t tt_bag_store_gather_workspace_bytes(int64_t B, int32_t n_sides) {
  const int64_t tiles = tt_cdiv(B > 0 ? B : 1, kStoreTile) * (n_sides > 0 ? n_sides : 1);
  return sizeof(int64_t) * (size_t)tiles;
}

int tt_bag_store_gather(tt_ctx* ctx, int32_t n, void* const* dst, const void* const* src, const int64_t* bytes,
                        const tt_bag_store_side* sides, int32_t n_sides, int64_t B, const int64_t* order, void* workspace,
                        size_t workspace_bytes, tt_stream stream) {
  return bag_store_gather_impl(ctx, n, dst, src, bytes, sides, n_sides, B, order, workspace, workspace_bytes, stream);
}

int tt_bag_store_gather_w(tt_ctx* ctx, int32_t n, void* const* dst, const void* const* src, const int64_t* bytes,
                          const tt_bag_store_side_w* sides, int32_t n_sides, int64_t B, const int64_t* order, void* workspace,
                          size_t workspace_bytes, tt_stream stream) {
  return bag_store_gather_impl(ctx, n, dst, src, bytes, sides, n_sides, B, order, workspace, workspace_bytes, stream);
}

}  // extern "C"
