// Table lookup and batch hand-over on gfx950: the fused multi-table lookup, the device-side batch assembly (gather, copies,
// conversions, id ingest) and the launch that does both (ingest_lookup_kernel).  All kernels are HBM-bound byte movers: 64-wide
// waves, 16-byte lanes, grids capped at 8 workgroups per CU with grid-stride loops.  The rest of the embedding path: tt_plan.hip
// (duplicate-row plans), tt_grad.hip (gradient reduction), tt_optim.hip (optimisers), tt_route.hip (sharded row routing).
#include "tt_common.h"
#include "tt_deferred.h"
#include "tt_embed_slots.h"
#include "tt_copy_role.h"

#include <stdlib.h>
#include <type_traits>

namespace {

// ------------------------------------------------------------------------------------------------
// a4 + a5: lookup.  Task = (slot, chunk); consecutive lanes take consecutive chunks of one row, so
// an E=32 f32 row is one 128-B line read by 8 lanes and a wave-instruction gathers 8 rows.
// U independent tasks per thread are issued before any store to keep >= U*16 B per lane in flight.
// ------------------------------------------------------------------------------------------------
template <int VEC, int U>
__global__ __launch_bounds__(kThreads) void lookup_kernel(SideSet a, const float* __restrict__ table,
                                                          int32_t* __restrict__ rows_out) {
  const uint32_t total = a.total_slots * a.C;
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t base = blockIdx.x * blockDim.x + threadIdx.x; base < total; base += stride * U) {
    float v[U][VEC];
    char* dst[U];
    int dt[U];
    bool ok[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t task = base + u * stride;
      ok[u] = task < total;
      if (ok[u]) {
        const uint32_t slot = task / a.C;
        const uint32_t chunk = task - slot * a.C;
        const int si = side_of(a, slot);
        const SideDev& s = a.s[si];
        const uint32_t local = slot - s.slot_base;
        const uint32_t b = local / (uint32_t)s.K;
        const uint32_t k = local - b * (uint32_t)s.K;
        int64_t id = s.ids[local];
        const int64_t hi = s.vocab[k] - 1;
        id = id < 0 ? 0 : (id > hi ? hi : id);                 // clamp: cat_embed.py:117
        const int64_t row = row_in_table(s.off[k] + id, a.table_rows, a.dev_err);
        if (chunk == 0 && rows_out) rows_out[slot] = (int32_t)row;
        if (table == nullptr) { ok[u] = false; continue; }      // rows-only mode (wave-uniform)
        const float* src = table + row * a.E + chunk * VEC;
        if (VEC == 4) {
          const float4 t = *reinterpret_cast<const float4*>(src);
          v[u][0] = t.x; v[u][1 % VEC] = t.y; v[u][2 % VEC] = t.z; v[u][3 % VEC] = t.w;
        } else {
          v[u][0] = src[0];
        }
        dt[u] = s.dtype;
        const int64_t col = (int64_t)b * s.ld + (int64_t)k * a.E + chunk * VEC;
        dst[u] = s.out + col * (s.dtype == TT_BF16 ? 2 : 4);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (!ok[u]) continue;
      if (dt[u] == TT_F32) {
        if (VEC == 4) {
          *reinterpret_cast<float4*>(dst[u]) = make_float4(v[u][0], v[u][1 % VEC], v[u][2 % VEC], v[u][3 % VEC]);
        } else {
          *reinterpret_cast<float*>(dst[u]) = v[u][0];
        }
      } else {
        if (VEC == 4) {
          ushort4 o;
          o.x = tt_f2bf(v[u][0]); o.y = tt_f2bf(v[u][1 % VEC]); o.z = tt_f2bf(v[u][2 % VEC]); o.w = tt_f2bf(v[u][3 % VEC]);
          *reinterpret_cast<ushort4*>(dst[u]) = o;
        } else {
          *reinterpret_cast<uint16_t*>(dst[u]) = tt_f2bf(v[u][0]);
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------
// a4 + a5, wave-chunk form (16-byte lanes, E % 4 == 0, E/4 a power of two <= 64).  A wave owns 64
// consecutive slots: lane l decodes slot l ONCE (coalesced 512-B id read, clamp, row, destination) and
// parks {source, destination} in a wave-private LDS table; the wave then walks the chunk 64/C rows at a
// time (C = E/4 lanes per row), issuing ALL row loads of the chunk before the first store, so every lane
// keeps C x 16 B in flight and a wave-instruction still reads whole 128-B lines.
// ------------------------------------------------------------------------------------------------
constexpr int kProfileMaxWg = 8192;
struct SlotRec {
  const float* src;
  char* dst;
};
using f32x4n = __attribute__((ext_vector_type(4))) float;

// W = 16-byte pieces per lane (round 4: with W = 2 a lane moves 32 B of a row -- two loads, ONE 16-byte bf16 store: half the
// store instructions, 3 % faster on tables in and out of the caches);  ROWS = the fused rows come precomputed (int32, slot
// order: the hand-over launch of a captured step has decoded and clamped the ids already -- tt_embed_lookup_rows_fwd) instead
// of being decoded from int64 ids, key offsets and vocabularies: no gathered offset / vocabulary loads, no 64-bit clamp, half
// the index bytes (lab, tools/probe/lookup_lab.hip: 9.2 -> 8.5 us back to back, 14.3 -> 11.9 us behind a cache-evicting copy).
template <int C, int SPW, int W, bool ROWS>   // C 16-byte chunks per row, SPW slots per wave pass
__global__ __launch_bounds__(kThreads) void lookup_wave_kernel(SideSet a, const float* __restrict__ table,
                                                              int32_t* __restrict__ rows_out, const int32_t* __restrict__ rows_in,
                                                              unsigned long long* __restrict__ ring, int ring_slots) {
  // measurement only: per-workgroup start/end stamps.  Workgroup b keeps its OWN launch counter (ring[b]) and writes the pair
  // of launch n into slot n % ring_slots of its column: no cross-workgroup traffic, no extra launch; the host reduces afterwards
  const bool stamp = ring && blockIdx.x < kProfileMaxWg && threadIdx.x == 0;
  unsigned long long t_start = 0, n_launch = 0;
  if (stamp) {
    t_start = __builtin_amdgcn_s_memrealtime();
    n_launch = ring[blockIdx.x];
  }
  __shared__ SlotRec recs[kThreads / 64][SPW];
  __shared__ int dts[kThreads / 64][SPW];
  static_assert(C % W == 0, "W pieces per lane must divide the row");
  constexpr int LPR = C / W;                        // lanes per row
  constexpr int RPI = 64 / LPR;                     // rows per wave-instruction
  constexpr int NIT = SPW / RPI;                    // wave-instructions per pass
  static_assert(SPW % RPI == 0 && NIT >= 1, "SPW must be a multiple of the rows per wave-instruction");
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t nchunks = (a.total_slots + SPW - 1) / SPW;
  const uint32_t wstride = gridDim.x * (kThreads / 64);
  for (uint32_t chunk = blockIdx.x * (kThreads / 64) + wave; chunk < nchunks; chunk += wstride) {
    const uint32_t slot = chunk * SPW + lane;
    SlotRec rec{nullptr, nullptr};
    int dt = TT_F32;
    if (lane < SPW && slot < a.total_slots) {
      const int si = side_of(a, slot);
      const SideDev& s = a.s[si];
      const uint32_t local = slot - s.slot_base;
      const uint32_t b = local / (uint32_t)s.K;
      const uint32_t k = local - b * (uint32_t)s.K;
      int64_t row;
      if (ROWS) {
        row = rows_in[slot];                               // checked where they were formed (tt_batch_ingest*: table_rows), not here
      } else {
        int64_t id = s.ids[local];
        const int64_t hi = s.vocab[k] - 1;
        id = id < 0 ? 0 : (id > hi ? hi : id);             // clamp: cat_embed.py:117
        row = row_in_table(s.off[k] + id, a.table_rows, a.dev_err);
        if (rows_out) rows_out[slot] = (int32_t)row;
      }
      rec.src = table + row * a.E;
      dt = s.dtype;
      rec.dst = s.out + ((int64_t)b * s.ld + (int64_t)k * a.E) * (dt == TT_BF16 ? 2 : 4);
    }
    if (lane < SPW) {
      recs[wave][lane] = rec;
      dts[wave][lane] = dt;
    }
    __builtin_amdgcn_wave_barrier();
    float4 v[NIT][W];
    const uint32_t sub = lane / LPR, part = lane % LPR;
#pragma unroll
    for (int j = 0; j < NIT; ++j) {
      const SlotRec r = recs[wave][j * RPI + sub];
#pragma unroll
      for (int w = 0; w < W; ++w) {
        v[j][w] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r.src != nullptr) v[j][w] = *reinterpret_cast<const float4*>(r.src + (part * W + w) * 4);
      }
    }
#pragma unroll
    for (int j = 0; j < NIT; ++j) {
      const SlotRec r = recs[wave][j * RPI + sub];
      if (r.dst == nullptr) continue;
      if (dts[wave][j * RPI + sub] == TT_F32) {            // non-temporal: the rows are read next by another kernel, not this one
#pragma unroll
        for (int w = 0; w < W; ++w) {
          f32x4n t;
          t[0] = v[j][w].x; t[1] = v[j][w].y; t[2] = v[j][w].z; t[3] = v[j][w].w;
          __builtin_nontemporal_store(t, reinterpret_cast<f32x4n*>(r.dst + (part * W + w) * 16));
        }
      } else if (W == 2) {
        uint4 o;
        o.x = (uint32_t)tt_f2bf(v[j][0].x) | ((uint32_t)tt_f2bf(v[j][0].y) << 16);
        o.y = (uint32_t)tt_f2bf(v[j][0].z) | ((uint32_t)tt_f2bf(v[j][0].w) << 16);
        o.z = (uint32_t)tt_f2bf(v[j][W - 1].x) | ((uint32_t)tt_f2bf(v[j][W - 1].y) << 16);
        o.w = (uint32_t)tt_f2bf(v[j][W - 1].z) | ((uint32_t)tt_f2bf(v[j][W - 1].w) << 16);
        *reinterpret_cast<uint4*>(r.dst + part * 16) = o;
      } else {
        ushort4 o;
        o.x = tt_f2bf(v[j][0].x); o.y = tt_f2bf(v[j][0].y); o.z = tt_f2bf(v[j][0].z); o.w = tt_f2bf(v[j][0].w);
        *reinterpret_cast<ushort4*>(r.dst + part * 8) = o;
      }
    }
    __builtin_amdgcn_wave_barrier();
  }
  if (ring) {                                            // measurement only: wait for this workgroup's stores
    __builtin_amdgcn_s_waitcnt(0);
    __syncthreads();
    if (stamp) {
      unsigned long long* pair = ring + kProfileMaxWg + ((n_launch % (unsigned long long)ring_slots) * kProfileMaxWg + blockIdx.x) * 2;
      pair[0] = t_start;
      pair[1] = __builtin_amdgcn_s_memrealtime();
      ring[blockIdx.x] = n_launch + 1;
    }
  }
}

// ------------------------------------------------------------------------------------------------
// a1/a2: device-side batch assembly
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void batch_gather_kernel(const int64_t* __restrict__ entity, uint32_t B,
                                                               const float* __restrict__ dense_store, uint32_t dense_dim,
                                                               const int64_t* __restrict__ cat_store, uint32_t K,
                                                               float* __restrict__ dense_out, int64_t* __restrict__ ids_out) {
  const uint32_t per = dense_dim + K;
  const uint32_t total = B * per;
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
    const uint32_t b = t / per, j = t - b * per;
    const int64_t e = entity[b];
    if (j < dense_dim) dense_out[(int64_t)b * dense_dim + j] = dense_store[e * dense_dim + j];
    else ids_out[(int64_t)b * K + (j - dense_dim)] = cat_store[e * K + (j - dense_dim)];
  }
}

// (CopyArgs and copy_segment_role: tt_copy_role.h)
__global__ __launch_bounds__(kThreads) void copy_multi_kernel(CopyArgs a) { copy_segment_role(a, blockIdx.y); }

// Batch hand-over of a graph-replayed step (tt_batch_ingest*): the copy segments of copy_multi_kernel plus, per side, the fused
// row of every id in KEY-MAJOR order (key_major_tile_role).  Grid rows of the launch: row 0 = every side's tiles (dispatched
// first: the few tile workgroups must not queue behind the thousands of copy workgroups); from the stores only, rows
// 1 .. n_sides = the dense feature rows of side y - 1 (dense_rows_role); then one row per copy segment; last, when the launch
// carries conversions, the cvt row.
constexpr int kIngestMaxK = 64;
// f32 -> bf16 (RNE) copies riding in the hand-over launch (tt_cvt_list): the towers' bf16 weight shadows, refreshed every step
struct CvtDev {
  const float* src[TT_MAX_CVT];
  uint16_t* dst[TT_MAX_CVT];
  int64_t count[TT_MAX_CVT];
  int32_t n;
};
__device__ __forceinline__ void cvt_role(const CvtDev& v) {
  for (int seg = 0; seg < v.n; ++seg) {
    const int64_t n4 = v.count[seg] / 4, stride = (int64_t)gridDim.x * blockDim.x;
    const float4* __restrict__ s = reinterpret_cast<const float4*>(v.src[seg]);
    ushort4* __restrict__ d = reinterpret_cast<ushort4*>(v.dst[seg]);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
      const float4 x = s[i];
      ushort4 o;
      o.x = tt_f2bf(x.x); o.y = tt_f2bf(x.y); o.z = tt_f2bf(x.z); o.w = tt_f2bf(x.w);
      d[i] = o;
    }
    if (blockIdx.x == 0)
      for (int64_t i = 4 * n4 + threadIdx.x; i < v.count[seg]; i += blockDim.x) v.dst[seg][i] = tt_f2bf(v.src[seg][i]);
  }
}
struct IngestArgs {
  CopyArgs c;
  CvtDev v;
  int32_t n_copy, n_sides, B;
  const int64_t* ids[TT_MAX_SIDES];
  const int64_t* off[TT_MAX_SIDES];
  const int64_t* vocab[TT_MAX_SIDES];
  int32_t K[TT_MAX_SIDES];
  int32_t side_base[TT_MAX_SIDES];
  int32_t* rows_km;
  int32_t* rows_sm;    // optional: the same fused rows in SLOT order (side_base + b * K + k) for tt_embed_lookup_rows_fwd
  int32_t table_rows;  // > 0: the rows are checked against this table size where they are formed (row_in_table)
  uint32_t* dev_err;
};

// The hand-over straight from the device-resident feature stores (tt_batch_ingest_store*): the batch's ids and dense features
// come out of the stores through the pair list instead of from a staged batch.
struct StoreIngestArgs {
  IngestArgs g;                                  // ids[] unused
  const int64_t* order;
  const int64_t* entity[TT_MAX_SIDES];
  int64_t entity_stride[TT_MAX_SIDES];
  const float* dense_store[TT_MAX_SIDES];
  const int64_t* cat_store[TT_MAX_SIDES];
  float* dense_out[TT_MAX_SIDES];
  int64_t* ids_out[TT_MAX_SIDES];
  int32_t dense_dim[TT_MAX_SIDES];
  int32_t n_rows[TT_MAX_SIDES];                  // entity rows of the store (0 = unchecked): indices are clamped into [0, n_rows)
};

// the store row of sample b of side si
__device__ __forceinline__ int64_t store_entity(const StoreIngestArgs& a, int si, int b) {
  const int64_t o = a.order ? a.order[b] : b;
  int64_t e = a.entity[si][o * a.entity_stride[si]];
  const int64_t nr = a.n_rows[si];
  if (nr > 0) e = e < 0 ? 0 : (e >= nr ? nr - 1 : e);
  return e;
}

// the dense feature rows of side si: 16-byte pieces (VEC) or floats, a row's pieces on consecutive lanes
template <bool VEC>
__device__ __forceinline__ void dense_rows_role(const StoreIngestArgs& __restrict__ a, int si) {
  const int dd = a.dense_dim[si];
  if (dd == 0) return;
  const int per = VEC ? dd / 4 : dd;                           // pieces per row
  const int64_t total = (int64_t)a.g.B * per, stride = (int64_t)gridDim.x * role_threads();
  for (int64_t t = (int64_t)blockIdx.x * role_threads() + threadIdx.x; t < total; t += stride) {
    const int b = (int)(t / per), j = (int)(t - (int64_t)b * per);
    const int64_t e = store_entity(a, si, b);
    if (VEC) reinterpret_cast<float4*>(a.dense_out[si] + (int64_t)b * dd)[j] = reinterpret_cast<const float4*>(a.dense_store[si] + e * dd)[j];
    else a.dense_out[si][(int64_t)b * dd + j] = a.dense_store[si][e * dd + j];
  }
}

__device__ __forceinline__ const IngestArgs& ingest_part(const IngestArgs& a) { return a; }
__device__ __forceinline__ const IngestArgs& ingest_part(const StoreIngestArgs& a) { return a.g; }
__device__ __forceinline__ const int64_t* id_source(const IngestArgs& a, int si) { return a.ids[si]; }
__device__ __forceinline__ const int64_t* id_source(const StoreIngestArgs& a, int si) { return a.cat_store[si]; }

// Grid row 0 of the hand-over without the lookup: every side's 64-sample tiles side by side (an own grid row per side meant a
// thousand empty workgroups each).  A tile writes the fused row of each of its ids in KEY-MAJOR order
// (rows_km[side_base + k * B + b] = key_row_offset[k] + clamp(ids[b * K + k])) -- the input tt_dedup_plan_keyed_km sorts.  A key's
// rows sit one per K * 4 bytes in the lookup's sample-major array: gathered by the sort itself that is a 128-byte line per lane
// (6.5 of a share's 18 us); here a workgroup reads 64 samples' ids as one run, turns the tile in LDS and writes 256-byte runs
// per key.  A = IngestArgs: the ids are the sample-major ids[]; A = StoreIngestArgs: they come from the stores (order ->
// entity -> cat_store) and are also written to ids_out, and the key-major rows are optional.
template <class A>
__device__ __forceinline__ void key_major_tile_role(const A& __restrict__ a) {
  constexpr bool FROM_STORE = std::is_same<A, StoreIngestArgs>::value;
  const IngestArgs& g = ingest_part(a);
  const int B = g.B, tiles = (B + 63) / 64;
  const int si = (int)blockIdx.x / tiles, tile = (int)blockIdx.x % tiles;
  if (si >= g.n_sides) return;
  const int K = g.K[si];
  __shared__ int32_t tl[kIngestMaxK][65];
  __shared__ int64_t s_off[kIngestMaxK], s_hi[kIngestMaxK], s_ent[64];
  const int64_t* __restrict__ ids = id_source(a, si);           // sample-major ids, or the store's id rows
  const int b0 = tile * 64;
  const int nb = min(64, B - b0), n = nb * K;
  if ((int)threadIdx.x < K) {
    s_off[threadIdx.x] = g.off[si][threadIdx.x];
    s_hi[threadIdx.x] = g.vocab[si][threadIdx.x] - 1;
  }
  if constexpr (FROM_STORE)
    if ((int)threadIdx.x >= 64 && (int)threadIdx.x < 64 + nb) s_ent[threadIdx.x - 64] = store_entity(a, si, b0 + threadIdx.x - 64);
  __syncthreads();
  constexpr int PER = kIngestMaxK * 64 / kThreads;            // ids per thread and tile: all loads issued before the first use
  int64_t idv[PER];
#pragma unroll
  for (int u = 0; u < PER; ++u) {                             // the tile's ids (a sample's: of its entity row) are one contiguous run
    const int e = threadIdx.x + u * kThreads;
    const int ec = e < n ? e : 0;
    if constexpr (FROM_STORE) {
      const int bl = ec / K, k = ec - bl * K;
      idv[u] = ids[s_ent[bl] * K + k];
    } else {
      idv[u] = ids[(int64_t)b0 * K + ec];
    }
  }
#pragma unroll
  for (int u = 0; u < PER; ++u) {
    const int e = threadIdx.x + u * kThreads;
    if (e < n) {
      const int bl = e / K, k = e - bl * K;
      int64_t id = idv[u];
      if constexpr (FROM_STORE) a.ids_out[si][(int64_t)b0 * K + e] = id;  // sample-major: the KJT values() of the batch
      id = id < 0 ? 0 : (id > s_hi[k] ? s_hi[k] : id);        // clamp: cat_embed.py:117 (as the lookup)
      tl[k][bl] = (int32_t)row_in_table(s_off[k] + id, g.table_rows, g.dev_err);
      if (g.rows_sm) g.rows_sm[g.side_base[si] + (int64_t)b0 * K + e] = tl[k][bl];
    }
  }
  if (FROM_STORE && g.rows_km == nullptr) return;
  __syncthreads();
  for (int e = threadIdx.x; e < K * 64; e += kThreads) {
    const int k = e >> 6, bl = e & 63;
    if (bl < nb) g.rows_km[g.side_base[si] + (int64_t)k * B + b0 + bl] = tl[k][bl];
  }
}

__global__ __launch_bounds__(kThreads) void batch_ingest_kernel(IngestArgs a) {
  if ((int)blockIdx.y == a.n_copy + 1) { cvt_role(a.v); return; }        // (last grid row, present when a.v.n > 0)
  if (blockIdx.y >= 1) { copy_segment_role(a.c, blockIdx.y - 1); return; }
  key_major_tile_role(a);
}

template <bool VEC>
__global__ __launch_bounds__(kThreads) void batch_ingest_store_kernel(StoreIngestArgs a) {
  if ((int)blockIdx.y == 1 + a.g.n_sides + a.g.n_copy) { cvt_role(a.g.v); return; }
  if ((int)blockIdx.y > a.g.n_sides) { copy_segment_role(a.g.c, blockIdx.y - 1 - a.g.n_sides); return; }
  if (blockIdx.y >= 1) { dense_rows_role<VEC>(a, blockIdx.y - 1); return; }
  key_major_tile_role(a);
}

// ------------------------------------------------------------------------------------------------
// Hand-over AND lookup in one launch (tt_batch_ingest_lookup / tt_batch_ingest_store_lookup; round 4).  The hand-over's tile
// workgroups already hold the batch's clamped fused rows in LDS; here they gather the table rows themselves and write them
// into the towers' input x (cat_embed.py:157-178 + base_tower.py:139), so the separate lookup launch -- its boundary, its
// re-read of the ids and its dispatch ramp -- is gone, and the copies of the dense features run beside the gathers.
//   tile = TS samples of one side, TS = 2^ts_shift chosen so that TS * K <= 512 slots: a 256-thread workgroup decodes two
//   slots per thread, a wave gathers up to two 64-slot chunks (every load issued before the first store: 16 x 16 B per lane
//   in flight, the standalone kernel's 19 waves per CU x 8 become ~10 x 16);
//   a lane moves 32 B of a row (LPR = E / 8 lanes per row): two 16-B loads, one 16-B bf16 store (two for f32 rows).
// Grid row 0 = every side's tiles (dispatched first); then, from the stores, one row per side for the dense features; then
// the copy segments.  Bit-identical to the hand-over followed by tt_embed_lookup_fwd (test).
// ------------------------------------------------------------------------------------------------
struct LookupPart {
  const float* table;
  char* out[TT_MAX_SIDES];
  int64_t ld[TT_MAX_SIDES];          // elements
  int32_t dtype[TT_MAX_SIDES];
  int32_t ts_shift[TT_MAX_SIDES];
  int32_t tile_base[TT_MAX_SIDES + 1];
  int32_t E;
  unsigned long long* ring;          // measurement: per-workgroup stamps of the tile role (tt_embed_lookup_set_profile)
  int32_t ring_slots;
  int32_t nt;                        // TT_OPT_LOOKUP_NT: bf16 rows leave by non-temporal stores
  int32_t table_rows;                // row_in_table
  uint32_t* dev_err;
};
constexpr int kTileSlots = 512;

template <int LPR, bool FROM_STORE, bool VEC>
__device__ __forceinline__ void ingest_lookup_body(const StoreIngestArgs& a, const LookupPart& lp) {
  const int B = a.g.B;
  const int first_copy_row = 1 + (FROM_STORE ? a.g.n_sides : 0);
  if ((int)blockIdx.y == first_copy_row + a.g.n_copy) { cvt_role(a.g.v); return; }
  if ((int)blockIdx.y >= first_copy_row) { copy_segment_role(a.g.c, blockIdx.y - first_copy_row); return; }
  if (FROM_STORE && blockIdx.y >= 1) { dense_rows_role<VEC>(a, blockIdx.y - 1); return; }
  // ---- row 0: tiles ----
  int si = 0;
#pragma unroll
  for (int i = 1; i < TT_MAX_SIDES; ++i)
    if (i < a.g.n_sides && (int)blockIdx.x >= lp.tile_base[i]) si = i;
  if ((int)blockIdx.x >= lp.tile_base[a.g.n_sides]) return;
  const int tile = (int)blockIdx.x - lp.tile_base[si];
  const int K = a.g.K[si], KP = K | 1, sh = lp.ts_shift[si], TS = 1 << sh;
  const int b0 = tile << sh;
  const int nb = min(TS, B - b0), n = nb * K;                  // <= kTileSlots
  // A wave works alone up to its gathers: it decodes its two 64-slot chunks (w and w + 4) itself -- id, key offset and vocabulary
  // straight from memory, like the stand-alone lookup -- parks {row, destination} in wave-private LDS and issues every row load;
  // only the key-major read-out of the tile's rows (tl) needs the other waves, and by then the rows are in flight.
  __shared__ int32_t rows_w[kThreads / 64][2][64];             // fused row of the wave's slot (the gather's order)
  __shared__ int64_t dst_w[kThreads / 64][2][64];              // byte offset of the slot's destination row in x (-1: no slot)
  __shared__ int32_t tl[kTileSlots + 64];                      // the tile's rows at bl * KP + k (odd stride: the key-major read-out)
  const int esz = lp.dtype[si] == TT_BF16 ? 2 : 4;
  constexpr int RPI = 64 / LPR;                                  // rows per wave-instruction
  constexpr int NIT = LPR;                                       // wave-instructions per chunk
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sub = lane / LPR, part = lane % LPR;
  const int64_t* __restrict__ offp = a.g.off[si];
  const int64_t* __restrict__ vocp = a.g.vocab[si];
  float4 v[2][NIT][2];
  int64_t dv[2][NIT];
  // decode both chunks first (their id loads are independent and issued together), then every row load of both
  int64_t idv[2], hiv[2], ofv[2];
  int blv[2], kv[2];
#pragma unroll
  for (int cc = 0; cc < 2; ++cc) {
    const int e = (wave + cc * (kThreads / 64)) * 64 + lane;
    const int ec = e < n ? e : 0;
    const int bl = ec / K, k = ec - bl * K;
    blv[cc] = bl; kv[cc] = k;
    if (FROM_STORE) {
      idv[cc] = a.cat_store[si][store_entity(a, si, b0 + bl) * K + k];
    } else {
      idv[cc] = a.g.ids[si][(int64_t)b0 * K + ec];
    }
    hiv[cc] = vocp[k] - 1;
    ofv[cc] = offp[k];
  }
#pragma unroll
  for (int cc = 0; cc < 2; ++cc) {
    const int e = (wave + cc * (kThreads / 64)) * 64 + lane;
    int32_t row = 0;
    int64_t dst = -1;
    if (e < n) {
      int64_t id = idv[cc];
      if (FROM_STORE) a.ids_out[si][(int64_t)b0 * K + e] = id;  // sample-major: the KJT values() of the batch
      id = id < 0 ? 0 : (id > hiv[cc] ? hiv[cc] : id);           // clamp: cat_embed.py:117
      row = (int32_t)row_in_table(ofv[cc] + id, lp.table_rows, lp.dev_err);
      dst = ((int64_t)(b0 + blv[cc]) * lp.ld[si] + (int64_t)kv[cc] * lp.E) * esz;
      tl[blv[cc] * KP + kv[cc]] = row;
    }
    rows_w[wave][cc][lane] = row;
    dst_w[wave][cc][lane] = dst;
  }
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int cc = 0; cc < 2; ++cc) {
#pragma unroll
    for (int j = 0; j < NIT; ++j) {
      const int sl = j * RPI + sub;
      dv[cc][j] = dst_w[wave][cc][sl];
      v[cc][j][0] = v[cc][j][1] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (dv[cc][j] >= 0) {
        const float* src = lp.table + (int64_t)rows_w[wave][cc][sl] * lp.E + part * 8;
        v[cc][j][0] = *reinterpret_cast<const float4*>(src);
        v[cc][j][1] = *reinterpret_cast<const float4*>(src + 4);
      }
    }
  }
  // while the rows fly: the key-major rows for the duplicate-row plan
  if (a.g.rows_km != nullptr) {
    __syncthreads();
    for (int e = threadIdx.x; e < (K << sh); e += kThreads) {
      const int k = e >> sh, bl = e & (TS - 1);
      if (bl < nb) a.g.rows_km[a.g.side_base[si] + (int64_t)k * B + b0 + bl] = tl[bl * KP + k];
    }
  }
  char* __restrict__ out = lp.out[si];
#pragma unroll
  for (int cc = 0; cc < 2; ++cc) {
#pragma unroll
    for (int j = 0; j < NIT; ++j) {
      if (dv[cc][j] < 0) continue;
      if (esz == 4) {                                          // non-temporal: the rows are read next by another kernel
        f32x4n t0, t1;
        t0[0] = v[cc][j][0].x; t0[1] = v[cc][j][0].y; t0[2] = v[cc][j][0].z; t0[3] = v[cc][j][0].w;
        t1[0] = v[cc][j][1].x; t1[1] = v[cc][j][1].y; t1[2] = v[cc][j][1].z; t1[3] = v[cc][j][1].w;
        f32x4n* d = reinterpret_cast<f32x4n*>(out + dv[cc][j] + part * 32);
        __builtin_nontemporal_store(t0, d);
        __builtin_nontemporal_store(t1, d + 1);
      } else {
        uint4 o;
        o.x = (uint32_t)tt_f2bf(v[cc][j][0].x) | ((uint32_t)tt_f2bf(v[cc][j][0].y) << 16);
        o.y = (uint32_t)tt_f2bf(v[cc][j][0].z) | ((uint32_t)tt_f2bf(v[cc][j][0].w) << 16);
        o.z = (uint32_t)tt_f2bf(v[cc][j][1].x) | ((uint32_t)tt_f2bf(v[cc][j][1].y) << 16);
        o.w = (uint32_t)tt_f2bf(v[cc][j][1].z) | ((uint32_t)tt_f2bf(v[cc][j][1].w) << 16);
        if (lp.nt) {
          using u32x4n = __attribute__((ext_vector_type(4))) unsigned int;
          u32x4n t; t[0] = o.x; t[1] = o.y; t[2] = o.z; t[3] = o.w;
          __builtin_nontemporal_store(t, reinterpret_cast<u32x4n*>(out + dv[cc][j] + part * 16));
        } else {
          *reinterpret_cast<uint4*>(out + dv[cc][j] + part * 16) = o;
        }
      }
    }
  }
}

template <int LPR, bool FROM_STORE, bool VEC>
__global__ __launch_bounds__(kThreads) void ingest_lookup_kernel(StoreIngestArgs a, LookupPart lp) {
  // measurement only (tt_embed_lookup_set_profile): start / end stamps of EVERY workgroup, column = its linear index -- the tiles
  // (gather phase) come first, the copy roles after them; the host reduces either set
  const uint32_t wg = blockIdx.y * gridDim.x + blockIdx.x;
  const bool stamp = lp.ring && wg < (uint32_t)kProfileMaxWg && threadIdx.x == 0;
  unsigned long long t_start = 0, n_launch = 0;
  if (stamp) {
    t_start = __builtin_amdgcn_s_memrealtime();
    n_launch = lp.ring[wg];
  }
  ingest_lookup_body<LPR, FROM_STORE, VEC>(a, lp);
  if (lp.ring) {                                               // wait for this workgroup's stores
    __builtin_amdgcn_s_waitcnt(0);
    __syncthreads();
    if (stamp) {
      unsigned long long* pair = lp.ring + kProfileMaxWg + ((n_launch % (unsigned long long)lp.ring_slots) * kProfileMaxWg + wg) * 2;
      pair[0] = t_start;
      pair[1] = __builtin_amdgcn_s_memrealtime();
      lp.ring[wg] = n_launch + 1;
    }
  }
}

// ------------------------------------------------------------------------------------------------
// host helpers
// ------------------------------------------------------------------------------------------------
// checks a tt_cvt_list and fills the device form; returns the number of extra grid rows (0 or 1) or < 0
static int fill_cvt(const char* who, const tt_cvt_list* cvt, CvtDev* v, int64_t* widest) {
  v->n = 0;
  if (!cvt || cvt->n == 0) return 0;
  if (cvt->n < 0 || cvt->n > TT_MAX_CVT) {
    tt_set_error("%s: cvt->n = %d not in [0, %d]", who, cvt->n, TT_MAX_CVT);
    return TT_ERR_INVALID_ARG;
  }
  for (int i = 0; i < cvt->n; ++i) {
    if (!(cvt->count[i] >= 0 && (cvt->count[i] == 0 || (cvt->src[i] && cvt->dst[i]))) || !tt_aligned(cvt->src[i], 16) || !tt_aligned(cvt->dst[i], 8)) {
      tt_set_error("%s: conversion %d NULL / misaligned (f32 source 16-byte, bf16 destination 8-byte aligned)", who, i);
      return TT_ERR_INVALID_ARG;
    }
    v->src[i] = cvt->src[i];
    v->dst[i] = reinterpret_cast<uint16_t*>(cvt->dst[i]);
    v->count[i] = cvt->count[i];
    if (cvt->count[i] * 4 > *widest) *widest = cvt->count[i] * 4;       // (bytes of f32 read: sizes the grid like a copy segment)
  }
  v->n = cvt->n;
  return 1;
}

}  // namespace

extern "C" {

int tt_embed_lookup_set_profile(tt_ctx* ctx, uint64_t* ring_dev, int32_t n_slots) {
  TT_CHECK_ARG(ctx, "tt_embed_lookup_set_profile: ctx NULL");
  TT_CHECK_ARG(ring_dev == nullptr || n_slots >= 1, "tt_embed_lookup_set_profile: n_slots must be >= 1");
  ctx->lookup_stamps = reinterpret_cast<unsigned long long*>(ring_dev);
  ctx->lookup_stamp_slots = ring_dev ? n_slots : 0;
  return TT_OK;
}

static int lookup_fwd_impl(tt_ctx* ctx, const float* table, int64_t table_rows, int32_t E, const tt_embed_side* sides, int32_t n_sides, int64_t B,
                           int32_t* rows_out, const int32_t* rows_in, tt_stream stream);

int tt_embed_lookup_fwd(tt_ctx* ctx, const float* table, int64_t table_rows, int32_t E, const tt_embed_side* sides,
                        int32_t n_sides, int64_t B, int32_t* rows_out, tt_stream stream) {
  return lookup_fwd_impl(ctx, table, table_rows, E, sides, n_sides, B, rows_out, nullptr, stream);
}

int tt_embed_lookup_rows_fwd(tt_ctx* ctx, const float* table, int64_t table_rows, int32_t E, const tt_embed_side* sides,
                             int32_t n_sides, int64_t B, const int32_t* rows, tt_stream stream) {
  TT_CHECK_ARG(table && rows, "tt_embed_lookup_rows_fwd: NULL table / rows");
  TT_CHECK_ARG(E % 4 == 0 && E / 4 <= 64 && ((E / 4) & (E / 4 - 1)) == 0 && tt_aligned(table, 16),
               "tt_embed_lookup_rows_fwd: E=%d must be 4 x a power of two <= 256 and the table 16-byte aligned", E);
  return lookup_fwd_impl(ctx, table, table_rows, E, sides, n_sides, B, nullptr, rows, stream);
}

static int lookup_fwd_impl(tt_ctx* ctx, const float* table, int64_t table_rows, int32_t E, const tt_embed_side* sides, int32_t n_sides, int64_t B,
                           int32_t* rows_out, const int32_t* rows_in, tt_stream stream) {
  TT_CHECK_ARG(ctx && sides && (table || rows_out), "tt_embed_lookup_fwd: NULL argument");
  TT_CHECK_ARG(n_sides >= 1 && n_sides <= TT_MAX_SIDES, "tt_embed_lookup_fwd: n_sides=%d not in [1,%d]", n_sides, TT_MAX_SIDES);
  TT_CHECK_ARG(E >= 1 && B >= 0 && table_rows >= 1, "tt_embed_lookup_fwd: bad E=%d B=%lld rows=%lld", E, (long long)B, (long long)table_rows);
  TT_CHECK_ARG(table_rows <= INT32_MAX, "tt_embed_lookup_fwd: table_rows %lld exceeds int32 row index", (long long)table_rows);
  SideSet a{};
  a.n = n_sides;
  a.E = E;
  bool vec4 = (E % 4 == 0) && tt_aligned(table, 16);
  int64_t slots = 0;
  for (int i = 0; i < n_sides; ++i) {
    const tt_embed_side& s = sides[i];
    TT_CHECK_ARG(s.K >= 0 && (s.K == 0 || (((s.ids && s.key_row_offset && s.key_vocab) || rows_in) && (s.out || !table))), "tt_embed_lookup_fwd: side %d has NULL pointers", i);
    TT_CHECK_ARG(s.out_dtype == TT_F32 || s.out_dtype == TT_BF16, "tt_embed_lookup_fwd: side %d bad out_dtype %d", i, s.out_dtype);
    TT_CHECK_ARG(s.ld_out >= (int64_t)s.K * E, "tt_embed_lookup_fwd: side %d ld_out %lld < K*E", i, (long long)s.ld_out);
    a.s[i] = SideDev{s.ids, s.key_row_offset, s.key_vocab, reinterpret_cast<char*>(s.out), s.ld_out, (uint32_t)slots, s.K, s.out_dtype, 0u};
    const size_t esz = s.out_dtype == TT_BF16 ? 2 : 4;
    vec4 = vec4 && (s.ld_out % 4 == 0) && tt_aligned(s.out, 4 * esz);
    slots += B * s.K;
  }
  const int64_t C = table ? (vec4 ? E / 4 : E) : 1;
  TT_CHECK_ARG(slots * C < (int64_t)1 << 31, "tt_embed_lookup_fwd: %lld slots x %lld chunks exceeds 2^31 tasks", (long long)slots, (long long)C);
  if (slots == 0) return TT_OK;
  a.C = (uint32_t)C;
  a.total_slots = (uint32_t)slots;
  a.table_rows = (int32_t)table_rows;
  a.dev_err = ctx->dev_err;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  constexpr int U = 4;
  const bool pow2c = vec4 && table && C <= 64 && (C & (C - 1)) == 0;
  if (pow2c) {
    const int spw = 64;                                    // slots per wave pass (32 and 16 measured slower at every C)
    int64_t wg = tt_cdiv(tt_cdiv(slots, spw), kThreads / 64);
    const int64_t cap = (int64_t)ctx->num_cus * 16;
    const int grid = (int)(wg < cap ? wg : cap);
    // two 16-byte pieces per lane when the rows and the outputs allow 32-byte lanes
    bool wide = C >= 2;
    for (int i = 0; i < n_sides; ++i) {
      const size_t esz = sides[i].out_dtype == TT_BF16 ? 2 : 4;
      wide = wide && (sides[i].ld_out % 8 == 0) && tt_aligned(sides[i].out, 8 * esz);
    }
    auto launch = [&](auto kernel) {
      kernel<<<grid, kThreads, 0, st>>>(a, table, rows_out, rows_in, ctx->lookup_stamps, ctx->lookup_stamp_slots);
    };
#define TT_LK1(CV, WV) do { if (rows_in) launch(lookup_wave_kernel<CV, spw, WV, true>); else launch(lookup_wave_kernel<CV, spw, WV, false>); } while (0)
#define TT_LK(CV) do { if (wide) TT_LK1(CV, (CV >= 2 ? 2 : 1)); else TT_LK1(CV, 1); } while (0)
    switch (C) {
      case 1: TT_LK1(1, 1); break;
      case 2: TT_LK(2); break;
      case 4: TT_LK(4); break;
      case 8: TT_LK(8); break;
      case 16: TT_LK(16); break;
      case 32: TT_LK(32); break;
      default: TT_LK(64); break;
    }
#undef TT_LK
#undef TT_LK1
    TT_LAUNCH_CHECK();
    return TT_OK;
  }
  if (rows_in) {
    tt_set_error("tt_embed_lookup_rows_fwd: outputs must be 4-element aligned (ld_out and base) for the precomputed-row form");
    return TT_ERR_UNSUPPORTED;
  }
  const int grid = grid_for(ctx, tt_cdiv(slots * C, U));
  if (vec4 && table) lookup_kernel<4, U><<<grid, kThreads, 0, st>>>(a, table, rows_out);
  else lookup_kernel<1, U><<<grid, kThreads, 0, st>>>(a, table, rows_out);
  TT_LAUNCH_CHECK();
  return TT_OK;
}

int tt_copy_multi(tt_ctx* ctx, int32_t n, void* const* dst, const void* const* src, const int64_t* bytes, tt_stream stream) {
  TT_CHECK_ARG(ctx && n >= 0 && n <= TT_MAX_COPIES && (n == 0 || (dst && src && bytes)), "tt_copy_multi: bad arguments");
  if (n == 0) return TT_OK;
  CopyArgs a{};
  int64_t mx = 0;
  for (int i = 0; i < n; ++i) {
    TT_CHECK_ARG(bytes[i] >= 0 && (bytes[i] == 0 || (dst[i] && src[i])), "tt_copy_multi: segment %d NULL", i);
    TT_CHECK_ARG(tt_aligned(dst[i], 16) && tt_aligned(src[i], 16), "tt_copy_multi: segment %d not 16-byte aligned", i);
    a.dst[i] = reinterpret_cast<char*>(dst[i]);
    a.src[i] = reinterpret_cast<const char*>(src[i]);
    a.bytes[i] = bytes[i];
    mx = bytes[i] > mx ? bytes[i] : mx;
  }
  int64_t gx = tt_cdiv(mx / 16 + 1, kThreads);
  const int64_t cap = (int64_t)ctx->num_cus * 4;
  if (gx > cap) gx = cap;
  copy_multi_kernel<<<dim3((unsigned)gx, (unsigned)n), kThreads, 0, reinterpret_cast<hipStream_t>(stream)>>>(a);
  TT_LAUNCH_CHECK();
  return TT_OK;
}

// The hand-over kernels leave by this door: an ordinary launch -- remembering, when the stream is being captured, the graph node the
// launch became -- or, while the context is retargeting (tt_handover_retarget), no launch at all: the node of the executable graph
// is re-pointed at this call's function, grid and arguments (hipGraphExecKernelNodeSetParams; launches of the graph already in flight
// keep the arguments they were enqueued with: tools/probe/graph_setparams.hip).
static int handover_launch(tt_ctx* ctx, const void* fn, dim3 grid, void** args, hipStream_t st) {
  if (ctx->ho_exec) {
    hipKernelNodeParams p{};
    p.func = const_cast<void*>(fn);
    p.gridDim = grid;
    p.blockDim = dim3(kThreads);
    p.kernelParams = args;
    TT_HIP(hipGraphExecKernelNodeSetParams(reinterpret_cast<hipGraphExec_t>(ctx->ho_exec), reinterpret_cast<hipGraphNode_t>(ctx->ho_node), &p));
    return TT_OK;
  }
  TT_HIP(hipLaunchKernel(fn, grid, dim3(kThreads), args, 0, st));
  TT_LAUNCH_CHECK();
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  const hipGraphNode_t* deps = nullptr;
  size_t n_deps = 0;
  if (hipStreamGetCaptureInfo_v2(st, &cs, nullptr, nullptr, &deps, &n_deps) == hipSuccess && cs == hipStreamCaptureStatusActive && n_deps == 1)
    ctx->ho_last = const_cast<void*>(reinterpret_cast<const void*>(deps[0]));
  else
    (void)hipGetLastError();
  return TT_OK;
}

// shared by the two fused hand-over + lookup entries: checks the lookup half and fills LookupPart; returns the tile count or < 0
static int64_t fill_lookup_part(tt_ctx* ctx, const char* who, const tt_embed_side* sides, int32_t n_sides, int64_t B, const tt_ingest_lookup* lk,
                                LookupPart* lp) {
  if (!(lk && lk->table && lk->table_rows >= 1 && lk->table_rows <= INT32_MAX)) {
    tt_set_error("%s: lookup part NULL / bad table", who);
    return TT_ERR_INVALID_ARG;
  }
  const int E = lk->E;
  if (!(E == 8 || E == 16 || E == 32 || E == 64) || !tt_aligned(lk->table, 16)) {
    tt_set_error("%s: E=%d not in {8, 16, 32, 64} or table not 16-byte aligned (use the separate hand-over and tt_embed_lookup_fwd)", who, E);
    return TT_ERR_UNSUPPORTED;
  }
  lp->table = lk->table;
  lp->E = E;
  lp->ring = ctx->lookup_stamps;
  lp->ring_slots = ctx->lookup_stamp_slots;
  lp->nt = ctx->lookup_nt;
  lp->table_rows = (int32_t)lk->table_rows;
  lp->dev_err = ctx->dev_err;
  int64_t tiles = 0;
  for (int i = 0; i < n_sides; ++i) {
    const tt_embed_side& s = sides[i];
    if (!(s.out && (s.out_dtype == TT_F32 || s.out_dtype == TT_BF16) && s.ld_out >= (int64_t)s.K * E)) {
      tt_set_error("%s: side %d needs an output (out, ld_out >= K*E, out_dtype f32 | bf16)", who, i);
      return TT_ERR_INVALID_ARG;
    }
    const size_t esz = s.out_dtype == TT_BF16 ? 2 : 4;
    if (!tt_aligned(s.out, 8 * esz) || (s.ld_out * esz) % (8 * esz) != 0) {
      tt_set_error("%s: side %d output not aligned to 8 elements", who, i);
      return TT_ERR_UNSUPPORTED;
    }
    int sh = 6;                                              // TS = 64 samples, halved until TS * K <= 512 slots (K <= 64: TS >= 8)
    while (sh > 3 && ((int64_t)s.K << sh) > kTileSlots) --sh;
    lp->out[i] = reinterpret_cast<char*>(s.out);
    lp->ld[i] = s.ld_out;
    lp->dtype[i] = s.out_dtype;
    lp->ts_shift[i] = sh;
    lp->tile_base[i] = (int32_t)tiles;
    tiles += tt_cdiv(B, (int64_t)1 << sh);
  }
  lp->tile_base[n_sides] = (int32_t)tiles;
  for (int i = n_sides + 1; i <= TT_MAX_SIDES; ++i) lp->tile_base[i] = (int32_t)tiles;
  if (tiles >= ((int64_t)1 << 30)) {
    tt_set_error("%s: too many tiles", who);
    return TT_ERR_INVALID_ARG;
  }
  return tiles;
}

// Everything the four hand-over entries share.  stores != nullptr: the ids and dense features come from the device stores
// (StoreIngestArgs); lk != nullptr: the launch also looks the rows up (LookupPart).  Checks the arguments -- error strings
// carry the entry's name `who` -- and fills the kernel arguments and the grid.
struct Handover {
  StoreIngestArgs a;
  LookupPart lp;
  dim3 grid;
  bool vec;            // store forms: every side's dense rows move in 16-byte pieces
};
static int build_handover(tt_ctx* ctx, const char* who, int32_t n, void* const* dst, const void* const* src, const int64_t* bytes,
                          const tt_embed_side* sides, const tt_store_side* stores, int32_t n_sides, int64_t B, const int64_t* order,
                          int32_t* rows_km, int32_t* rows_sm, int64_t table_rows, const tt_cvt_list* cvt, const tt_ingest_lookup* lk,
                          Handover* h) {
  TT_CHECK_ARG(ctx && n >= 0 && n <= TT_MAX_COPIES && (n == 0 || (dst && src && bytes)), "%s: bad copy arguments", who);
  TT_CHECK_ARG(sides && n_sides >= 1 && n_sides <= TT_MAX_SIDES && B >= 1, "%s: bad side arguments", who);
  TT_CHECK_ARG(table_rows >= 0 && table_rows <= INT32_MAX, "%s: table_rows %lld out of range", who, (long long)table_rows);
  *h = Handover{};
  StoreIngestArgs& a = h->a;
  int64_t mx = 0, slots = 0, dense_pieces = 0;
  for (int i = 0; i < n; ++i) {
    TT_CHECK_ARG(bytes[i] >= 0 && (bytes[i] == 0 || (dst[i] && src[i])), "%s: segment %d NULL", who, i);
    TT_CHECK_ARG(tt_aligned(dst[i], 16) && tt_aligned(src[i], 16), "%s: segment %d not 16-byte aligned", who, i);
    a.g.c.dst[i] = reinterpret_cast<char*>(dst[i]);
    a.g.c.src[i] = reinterpret_cast<const char*>(src[i]);
    a.g.c.bytes[i] = bytes[i];
    mx = bytes[i] > mx ? bytes[i] : mx;
  }
  a.g.n_copy = n;
  a.g.n_sides = n_sides;
  a.g.B = (int32_t)B;
  a.g.rows_km = rows_km;
  a.g.rows_sm = rows_sm;
  a.g.table_rows = (int32_t)table_rows;
  a.g.dev_err = ctx->dev_err;
  a.order = order;
  h->vec = true;
  for (int i = 0; i < n_sides; ++i) {
    const tt_embed_side& s = sides[i];
    TT_CHECK_ARG(s.K >= 1 && (stores || s.ids) && s.key_row_offset && s.key_vocab, "%s: side %d NULL / no keys", who, i);
    if (s.K > kIngestMaxK) {
      tt_set_error("%s: side %d has %d keys (max %d)", who, i, s.K, kIngestMaxK);
      return TT_ERR_UNSUPPORTED;
    }
    a.g.ids[i] = stores ? nullptr : s.ids; a.g.off[i] = s.key_row_offset; a.g.vocab[i] = s.key_vocab; a.g.K[i] = s.K;
    a.g.side_base[i] = (int32_t)slots;
    slots += B * s.K;
    if (!stores) continue;
    const tt_store_side& t = stores[i];
    TT_CHECK_ARG(t.entity && t.entity_stride >= 1 && t.cat_store && t.ids_out && t.dense_dim >= 0 && t.n_rows >= 0 &&
                 (t.dense_dim == 0 || (t.dense_store && t.dense_out)), "%s: store %d NULL / bad shape", who, i);
    a.entity[i] = t.entity; a.entity_stride[i] = t.entity_stride; a.dense_store[i] = t.dense_store; a.cat_store[i] = t.cat_store;
    a.dense_out[i] = t.dense_out; a.ids_out[i] = t.ids_out; a.dense_dim[i] = t.dense_dim;
    a.n_rows[i] = t.n_rows;
    h->vec = h->vec && t.dense_dim % 4 == 0 && tt_aligned(t.dense_store, 16) && tt_aligned(t.dense_out, 16);
    const int64_t p = B * (int64_t)t.dense_dim;
    dense_pieces = p > dense_pieces ? p : dense_pieces;
  }
  TT_CHECK_ARG(slots < ((int64_t)1 << 31), "%s: too many slots", who);
  int64_t tiles = tt_cdiv(B, 64) * n_sides;                // row 0 holds every tile (the other rows stride over their work)
  if (lk) {
    tiles = fill_lookup_part(ctx, who, sides, n_sides, B, lk, &h->lp);
    if (tiles < 0) return (int)tiles;
  }
  const int cvt_rows = fill_cvt(who, cvt, &a.g.v, &mx);
  if (cvt_rows < 0) return cvt_rows;
  int64_t gx = tt_cdiv(mx / 16 + 1, kThreads);
  const int64_t rows_wg = tt_cdiv(h->vec ? dense_pieces / 4 : dense_pieces, kThreads);
  if (rows_wg > gx) gx = rows_wg;
  // workgroups per CU the copy and dense rows stride with: the forms from a staged batch keep copy_multi's 4, the store forms
  // take 8 (as written with the dense-feature rows; no measurement of either choice is recorded)
  const int64_t cap = (int64_t)ctx->num_cus * (stores ? 8 : 4);
  if (gx > cap) gx = cap;
  if (tiles > gx) gx = tiles;
  h->grid = dim3((unsigned)gx, (unsigned)(1 + (stores ? n_sides : 0) + n + cvt_rows));
  return TT_OK;
}

#define TT_INGEST_LOOKUP_FN(FROM_STORE, VEC)                                                                              \
  (h.lp.E == 8 ? reinterpret_cast<const void*>(ingest_lookup_kernel<1, FROM_STORE, VEC>)                                  \
   : h.lp.E == 16 ? reinterpret_cast<const void*>(ingest_lookup_kernel<2, FROM_STORE, VEC>)                               \
   : h.lp.E == 32 ? reinterpret_cast<const void*>(ingest_lookup_kernel<4, FROM_STORE, VEC>)                               \
                  : reinterpret_cast<const void*>(ingest_lookup_kernel<8, FROM_STORE, VEC>))

int tt_batch_ingest(tt_ctx* ctx, int32_t n, void* const* dst, const void* const* src, const int64_t* bytes, const tt_embed_side* sides,
                    int32_t n_sides, int64_t B, int32_t* rows_km, int32_t* rows_sm, int64_t table_rows, const tt_cvt_list* cvt, tt_stream stream) {
  TT_CHECK_ARG(rows_km, "tt_batch_ingest: bad side arguments");      // (this form's tiles always write the key-major rows)
  Handover h;
  const int rc = build_handover(ctx, "tt_batch_ingest", n, dst, src, bytes, sides, nullptr, n_sides, B, nullptr, rows_km, rows_sm,
                                table_rows, cvt, nullptr, &h);
  if (rc != TT_OK) return rc;
  void* args[] = {&h.a.g};
  return handover_launch(ctx, reinterpret_cast<const void*>(batch_ingest_kernel), h.grid, args, reinterpret_cast<hipStream_t>(stream));
}

int tt_batch_ingest_store(tt_ctx* ctx, int32_t n, void* const* dst, const void* const* src, const int64_t* bytes, const tt_embed_side* sides,
                          const tt_store_side* stores, int32_t n_sides, int64_t B, const int64_t* order, int32_t* rows_km, int32_t* rows_sm,
                          int64_t table_rows, const tt_cvt_list* cvt, tt_stream stream) {
  TT_CHECK_ARG(stores, "tt_batch_ingest_store: bad side arguments");
  Handover h;
  const int rc = build_handover(ctx, "tt_batch_ingest_store", n, dst, src, bytes, sides, stores, n_sides, B, order, rows_km, rows_sm,
                                table_rows, cvt, nullptr, &h);
  if (rc != TT_OK) return rc;
  void* args[] = {&h.a};
  return handover_launch(ctx, h.vec ? reinterpret_cast<const void*>(batch_ingest_store_kernel<true>) : reinterpret_cast<const void*>(batch_ingest_store_kernel<false>),
                         h.grid, args, reinterpret_cast<hipStream_t>(stream));
}

int tt_batch_ingest_lookup(tt_ctx* ctx, int32_t n, void* const* dst, const void* const* src, const int64_t* bytes, const tt_embed_side* sides,
                           int32_t n_sides, int64_t B, int32_t* rows_km, const tt_ingest_lookup* lk, const tt_cvt_list* cvt, tt_stream stream) {
  Handover h;
  const int rc = build_handover(ctx, "tt_batch_ingest_lookup", n, dst, src, bytes, sides, nullptr, n_sides, B, nullptr, rows_km, nullptr, 0,
                                cvt, lk, &h);
  if (rc != TT_OK) return rc;
  void* args[] = {&h.a, &h.lp};
  return handover_launch(ctx, TT_INGEST_LOOKUP_FN(false, true), h.grid, args, reinterpret_cast<hipStream_t>(stream));
}

int tt_batch_ingest_store_lookup(tt_ctx* ctx, int32_t n, void* const* dst, const void* const* src, const int64_t* bytes,
                                 const tt_embed_side* sides, const tt_store_side* stores, int32_t n_sides, int64_t B, const int64_t* order,
                                 int32_t* rows_km, const tt_ingest_lookup* lk, const tt_cvt_list* cvt, tt_stream stream) {
  TT_CHECK_ARG(stores, "tt_batch_ingest_store_lookup: bad side arguments");
  Handover h;
  const int rc = build_handover(ctx, "tt_batch_ingest_store_lookup", n, dst, src, bytes, sides, stores, n_sides, B, order, rows_km, nullptr,
                                0, cvt, lk, &h);
  if (rc != TT_OK) return rc;
  void* args[] = {&h.a, &h.lp};
  return handover_launch(ctx, h.vec ? TT_INGEST_LOOKUP_FN(true, true) : TT_INGEST_LOOKUP_FN(true, false), h.grid, args,
                         reinterpret_cast<hipStream_t>(stream));
}

int tt_batch_gather(tt_ctx* ctx, const int64_t* entity, int64_t B, const float* dense_store, int32_t dense_dim,
                    const int64_t* cat_store, int32_t K, float* dense_out, int64_t* ids_out, tt_stream stream) {
  TT_CHECK_ARG(ctx && entity, "tt_batch_gather: NULL argument");
  TT_CHECK_ARG(B >= 0 && dense_dim >= 0 && K >= 0, "tt_batch_gather: negative size");
  TT_CHECK_ARG(dense_dim == 0 || (dense_store && dense_out), "tt_batch_gather: NULL dense buffers");
  TT_CHECK_ARG(K == 0 || (cat_store && ids_out), "tt_batch_gather: NULL id buffers");
  const int64_t total = B * ((int64_t)dense_dim + K);
  TT_CHECK_ARG(total < ((int64_t)1 << 31), "tt_batch_gather: too many elements");
  if (total == 0) return TT_OK;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  batch_gather_kernel<<<grid_for(ctx, total), kThreads, 0, st>>>(entity, (uint32_t)B, dense_store, (uint32_t)dense_dim, cat_store,
                                                                  (uint32_t)K, dense_out, ids_out);
  TT_LAUNCH_CHECK();
  return TT_OK;
}

}  // extern "C"
