// Pooled multi-valued categorical features (embedding bags) on gfx950: the pooled lookup and its table gradient.  A bag is the
// run ids[offsets[slot] .. offsets[slot + 1]) of one (sample, key) slot.  Forward: one lane group of E/4 lanes per bag gathers
// the bag's rows with 16-byte loads and adds them in position order.  Backward: the lookup's duplicate-row plan over the
// POSITIONS' rows (tt_plan.hip, unchanged), reduced like tt_grad.hip's rows -- same chunking, same workspace, the same long-row
// finish body (tt_grad_ws.h) -- with the contribution of a position read through bag_of (its slot) and weighted for mean pooling.
// The weighted form (one f32 weight per id: the _w entries) is a template parameter of the same kernels, not a copy of them; so is
// the forward's position-weight source (the _posw entries: a side's weights read out of a learned parameter by position in the bag).
#include "tt_bag_pw.h"
#include "tt_common.h"
#include "tt_deferred.h"
#include "tt_embed_slots.h"
#include "tt_grad_ws.h"

namespace {

struct BagSideDev {
  const int64_t* ids;
  const int64_t* offs;
  const int64_t* off;
  const int64_t* vocab;
  const int32_t* pool;
  char* out;
  int64_t ld;
  int64_t nnz;
  uint32_t slot_base;  // first slot of this side
  uint32_t pos_base;   // first position of this side in rows_out / bag_of
  int32_t K;
  int32_t dtype;
};

struct BagSet {
  BagSideDev s[TT_MAX_SIDES];
  int32_t n;
  int32_t E;
  uint32_t C;            // 16-byte chunks per row
  uint32_t LG;           // lanes per bag: the power of two >= C
  uint32_t total_slots;
  int32_t table_rows;
  uint32_t* dev_err;
  int32_t* rows_out;
  int32_t* bag_of;
  int32_t pad_row;       // < 0: tt_embed_bag_fwd.  >= 0 (table_rows): the capacity form -- every position no bag covers gets (pad_row, -1)
  uint32_t total_pos;    // (capacity form) all sides' capacities
};

// ------------------------------------------------------------------------------------------------
// forward.  A lane group owns one bag at a time; 64 / LG bags share a wave.  Per trip the group reads kBagBatch ids (every lane
// the same words), decodes them and issues all their row loads before the first add; the adds stay in position order.
// ------------------------------------------------------------------------------------------------
constexpr int kBagBatch = 8;

// the kernel's argument.  The weighted form (W) adds the per-id weights: one f32 per position of a side (NULL: the side's ids all
// weigh 1) and the place the gradient reads them back from, laid out like rows_out / bag_of.  The unweighted instantiation takes
// BagSet as it is: its kernel-argument layout, like its code, does not change.
// W is the forward's weight form: 0 none, 1 per-id arrays, 2 per side a per-id array, a position-weight parameter or nothing.
// 3 and 4 are the ROWS-ONLY forms of 0 and 1 (tt_embed_bag_rows[_w]): the same walk over the bags and the same words in rows_out /
// bag_of / w_out, but no table is read and no pooled output written -- what a rank of the sharded step runs, whose table is not local.
constexpr bool bag_weighted(int W) { return W == 1 || W == 2 || W == 4; }
constexpr bool bag_rows_only(int W) { return W >= 3; }
template <int W>
struct BagFwdArgs : BagSet {};
template <>
struct BagFwdArgs<1> : BagSet {
  const float* w[TT_MAX_SIDES];
  float* w_out;
};
// the _posw entries: per side a position-weight parameter (NULL: the side takes w[si], or weighs 1) and its key directory
template <>
struct BagFwdArgs<4> : BagFwdArgs<1> {};
template <>
struct BagFwdArgs<2> : BagFwdArgs<1> {
  const float* pw_param[TT_MAX_SIDES];
  const int32_t* pw_off[TT_MAX_SIDES];
  const int32_t* pw_len[TT_MAX_SIDES];
  int64_t pw_n[TT_MAX_SIDES];
};

// W: acc = w * x for a bag's first position, acc = fma(w, x, acc) for every later one.  With every weight 1 these are the bits of
// the unweighted form (1 * x = x, a -0 included; fma(1, x, acc) = acc + x).
// W == 2: a side with a parameter reads position j of a bag of key k from param[pw_index_at(off[k], len[k], j)] (tt_bag_pw.h), 1
// for a key without; the value takes the place of the per-id weight in the same chain and in w_out.  The sides of one launch may
// differ: parameter, per-id array, none.
// Rows-only forms: the lane group is kBagBatch lanes wide (lane j writes position j of a trip) and `table` is NULL.
template <int W>
__global__ __launch_bounds__(kThreads) void bag_fwd_kernel(BagFwdArgs<W> a, const float* __restrict__ table) {
  const uint32_t LG = a.LG;
  const uint32_t gthread = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t lig = gthread & (LG - 1);
  const uint32_t ngroups = gridDim.x * blockDim.x / LG;
  [[maybe_unused]] const bool live = lig < a.C;
  for (uint32_t slot = gthread / LG; slot < a.total_slots; slot += ngroups) {
    int si = 0;
#pragma unroll
    for (int i = 1; i < TT_MAX_SIDES; ++i)
      if (i < a.n && slot >= a.s[i].slot_base) si = i;
    const BagSideDev& s = a.s[si];
    const uint32_t local = slot - s.slot_base;
    [[maybe_unused]] const uint32_t b = local / (uint32_t)s.K;
    const uint32_t k = local - b * (uint32_t)s.K;
    int64_t o0 = s.offs[local], o1 = s.offs[local + 1];
    if (o0 < 0 || o1 < o0 || o1 > s.nnz) {                   // nothing is read through such a pair: the bag counts as empty
      if (lig == 0 && a.dev_err) atomicOr(a.dev_err, TT_DEVERR_BAG_OFFSETS);
      o0 = o1 = 0;
    }
    const int64_t hi = s.vocab[k] - 1, base = s.off[k];
    const float* sw = nullptr;
    if constexpr (bag_weighted(W)) sw = a.w[si];
    const float* pp = nullptr;                                 // (W == 2) the side's parameter and this bag's key entry
    int32_t poff = -1, plen = 0;
    int64_t pn = 0;
    if constexpr (W == 2) {
      pp = a.pw_param[si];
      if (pp) {
        poff = a.pw_off[si][k]; plen = a.pw_len[si][k];
        pn = a.pw_n[si];
      }
    }
    [[maybe_unused]] float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int64_t p = o0; p < o1; p += kBagBatch) {
      int64_t id[kBagBatch];
#pragma unroll
      for (int j = 0; j < kBagBatch; ++j) id[j] = p + j < o1 ? s.ids[p + j] : 0;
      float wj[kBagBatch];                                     // (W) the trip's weights, loaded next to its ids: no new dependent level
      if constexpr (W == 2) {
#pragma unroll
        for (int j = 0; j < kBagBatch; ++j) {
          wj[j] = 1.f;
          if (p + j >= o1) continue;
          if (pp) {
            const int64_t e = pw_index_at(poff, plen, p + j - o0, pn);
            if (e >= 0) wj[j] = pp[e];
          } else if (sw) {
            wj[j] = sw[p + j];
          }
        }
      } else if constexpr (bag_weighted(W)) {
#pragma unroll
        for (int j = 0; j < kBagBatch; ++j) wj[j] = (sw && p + j < o1) ? sw[p + j] : 1.f;
      }
      [[maybe_unused]] float4 v[kBagBatch];
#pragma unroll
      for (int j = 0; j < kBagBatch; ++j) {
        if constexpr (!bag_rows_only(W)) v[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (p + j < o1) {
          const int64_t idc = id[j] < 0 ? 0 : (id[j] > hi ? hi : id[j]);             // clamp: cat_embed.py:117 (as the lookup)
          const int64_t row = row_in_table(base + idc, a.table_rows, a.dev_err);
          if (lig == ((uint32_t)j & (LG - 1))) {
            if (a.rows_out) a.rows_out[s.pos_base + (p + j)] = (int32_t)row;
            if (a.bag_of) a.bag_of[s.pos_base + (p + j)] = (int32_t)slot;
            if constexpr (bag_weighted(W)) {
              if (a.w_out) a.w_out[s.pos_base + (p + j)] = wj[j];
            }
          }
          if constexpr (!bag_rows_only(W)) {
            if (live) v[j] = *reinterpret_cast<const float4*>(table + row * a.E + lig * 4);
          }
        }
      }
#pragma unroll
      for (int j = 0; j < kBagBatch; ++j) {
        if (bag_rows_only(W) || p + j >= o1) continue;
        if constexpr (bag_weighted(W)) {
          if (p + j == o0) {
            acc.x = __fmul_rn(wj[j], v[j].x); acc.y = __fmul_rn(wj[j], v[j].y);
            acc.z = __fmul_rn(wj[j], v[j].z); acc.w = __fmul_rn(wj[j], v[j].w);
          } else {
            acc.x = __fmaf_rn(wj[j], v[j].x, acc.x); acc.y = __fmaf_rn(wj[j], v[j].y, acc.y);
            acc.z = __fmaf_rn(wj[j], v[j].z, acc.z); acc.w = __fmaf_rn(wj[j], v[j].w, acc.w);
          }
        } else if (p + j == o0) {                            // the first row as it is: a bag of one id is a bit-exact copy
          acc = v[j];
        } else {
          acc.x += v[j].x; acc.y += v[j].y; acc.z += v[j].z; acc.w += v[j].w;
        }
      }
    }
    const int64_t len = o1 - o0;
    if (!bag_rows_only(W) && len > 1 && s.pool[k] == TT_POOL_MEAN) {
      const float l = (float)len;
      acc.x /= l; acc.y /= l; acc.z /= l; acc.w /= l;
    }
    if (!bag_rows_only(W) && live) {
      const int64_t col = (int64_t)b * s.ld + (int64_t)k * a.E + lig * 4;
      if (s.dtype == TT_F32) {
        *reinterpret_cast<float4*>(s.out + col * 4) = acc;
      } else {
        ushort4 o;
        o.x = tt_f2bf(acc.x); o.y = tt_f2bf(acc.y); o.z = tt_f2bf(acc.z); o.w = tt_f2bf(acc.w);
        *reinterpret_cast<ushort4*>(s.out + col * 2) = o;
      }
    }
    // positions behind the side's last bag belong to no bag: row 0, bag -1 (the gradient skips them)
    if (a.pad_row < 0 && slot + 1 == (si + 1 < a.n ? a.s[si + 1].slot_base : a.total_slots)) {
      const int64_t t0 = s.offs[local + 1];
      if (t0 >= 0 && t0 <= s.nnz)
        for (int64_t p = t0 + lig; p < s.nnz; p += LG) {
          if (a.rows_out) a.rows_out[s.pos_base + p] = 0;
          if (a.bag_of) a.bag_of[s.pos_base + p] = -1;
        }
    }
  }
  if (a.pad_row < 0) return;
  // capacity form: nnz is the CAPACITY of a static id buffer and the live count offs[B*K] is device data.  The whole grid walks
  // position space (the sides lie behind one another: side 1 starts at side 0's capacity) and writes (pad_row, -1) wherever no
  // bag covers: [live, capacity), and a position below `live` whose bag was refused above.  Nothing is read from ids here.
  for (uint32_t P = gthread; P < a.total_pos; P += gridDim.x * blockDim.x) {
    int si = 0;
#pragma unroll
    for (int i = 1; i < TT_MAX_SIDES; ++i)
      if (i < a.n && P >= a.s[i].pos_base) si = i;
    const BagSideDev& s = a.s[si];
    const int64_t p = (int64_t)(P - s.pos_base);
    const uint32_t S = (si + 1 < a.n ? a.s[si + 1].slot_base : a.total_slots) - s.slot_base;
    const int64_t live = s.offs[S];
    bool covered = false;
    if (p < live) {
      // the bag that holds p: the last slot whose offset is <= p (offsets ascend; where they do not, a pair was refused and
      // the error word is up -- the search still stays inside [0, S])
      uint32_t lo = 0, hi = S;                                 // first slot in (lo, hi] whose offset is > p
      while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (s.offs[mid + 1] > p) hi = mid; else lo = mid + 1;
      }
      if (lo < S) {
        const int64_t o0 = s.offs[lo], o1 = s.offs[lo + 1];
        covered = o0 >= 0 && o0 <= p && p < o1 && o1 <= s.nnz;
      }
    }
    if (!covered) {
      if (a.rows_out) a.rows_out[P] = a.pad_row;
      if (a.bag_of) a.bag_of[P] = -1;
    }
  }
}

// ------------------------------------------------------------------------------------------------
// tt_bag_prepare: offsets (exclusive prefix sum of the lengths) and mean weights of every side, grid-wide in two launches with no
// wait between workgroups: tile totals, then every tile adds up its side's earlier totals (<= 2048 words) and scans its own part.
// ------------------------------------------------------------------------------------------------
constexpr int kPrepPer = 8;                           // slots per thread: 64 bytes of lengths
constexpr int kPrepTile = kThreads * kPrepPer;

struct PrepSide {
  const int64_t* lengths;
  const int32_t* pool;
  const int32_t* count;      // the id count the host handed over (device word), or NULL
  int64_t* offs;
  int64_t capacity;
  uint32_t slots;            // B*K
  uint32_t slot_base;
  uint32_t tile_base;
  int32_t K;
};
struct PrepSet {
  PrepSide s[TT_MAX_SIDES];
  int32_t n;
  uint32_t tiles;
  float* inv_len;            // [total slots] or NULL
  int64_t* tile_sum;         // [tiles]; a tile with a negative length reports kPrepBad
  uint32_t* dev_err;
};
constexpr int64_t kPrepBad = (int64_t)1 << 62;         // larger than any sum of 2^31 lengths that could fit a buffer

__device__ __forceinline__ int prep_side_of(const PrepSet& a, uint32_t tile) {
  int si = 0;
#pragma unroll
  for (int i = 1; i < TT_MAX_SIDES; ++i)
    if (i < a.n && tile >= a.s[i].tile_base) si = i;
  return si;
}

// the thread's kPrepPer lengths (0 behind the side's end): 16-byte loads where the whole run lies inside
__device__ __forceinline__ void prep_load(const PrepSide& s, uint32_t first, int64_t (&len)[kPrepPer]) {
  if (first + kPrepPer <= s.slots && (reinterpret_cast<uintptr_t>(s.lengths) & 15) == 0) {
    const longlong2* q = reinterpret_cast<const longlong2*>(s.lengths + first);
#pragma unroll
    for (int j = 0; j < kPrepPer / 2; ++j) {
      const longlong2 t = q[j];
      len[2 * j] = t.x; len[2 * j + 1] = t.y;
    }
  } else {
#pragma unroll
    for (int j = 0; j < kPrepPer; ++j) len[j] = first + j < s.slots ? s.lengths[first + j] : 0;
  }
}

// sum over the workgroup (every thread gets it); sh: 2 * 4 words
__device__ __forceinline__ int64_t prep_block_sum(int64_t v, int64_t* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return sh[0] + sh[1] + sh[2] + sh[3];
}

__global__ __launch_bounds__(kThreads) void bag_prep_reduce_kernel(PrepSet a) {
  __shared__ int64_t sh[8];
  const PrepSide& s = a.s[prep_side_of(a, blockIdx.x)];
  const uint32_t first = (blockIdx.x - s.tile_base) * kPrepTile + threadIdx.x * kPrepPer;
  int64_t len[kPrepPer], t = 0, bad = 0;
  prep_load(s, first, len);
#pragma unroll
  for (int j = 0; j < kPrepPer; ++j) {
    bad |= (len[j] < 0 || len[j] > s.capacity) ? 1 : 0;      // (also keeps the sums far from overflow)
    t += len[j];
  }
  const int64_t tot = prep_block_sum(t, sh);
  const int64_t anybad = prep_block_sum(bad, sh + 4);
  if (threadIdx.x == 0) a.tile_sum[blockIdx.x] = anybad ? kPrepBad : tot;
}

__global__ __launch_bounds__(kThreads) void bag_prep_scan_kernel(PrepSet a) {
  __shared__ int64_t sh[8];
  __shared__ int64_t wsum[4];
  const int si = prep_side_of(a, blockIdx.x);
  const PrepSide& s = a.s[si];
  const uint32_t ntile = (si + 1 < a.n ? a.s[si + 1].tile_base : a.tiles) - s.tile_base, tile = blockIdx.x - s.tile_base;
  // the side's total and this tile's start: integer sums, any order gives the same bits
  int64_t before = 0, all = 0, bad = 0;
  for (uint32_t b = threadIdx.x; b < ntile; b += kThreads) {
    const int64_t v = a.tile_sum[s.tile_base + b];
    bad |= v >= kPrepBad ? 1 : 0;
    all += v >= kPrepBad ? 0 : v;
    if (b < tile) before += v >= kPrepBad ? 0 : v;
  }
  before = prep_block_sum(before, sh);
  all = prep_block_sum(all, sh + 4);
  __syncthreads();
  bad = prep_block_sum(bad, sh);
  // refused: a negative length, a total above the capacity, or another total than the host handed over -- the side's bags then all
  // count as empty (offsets all zero: every position of the side is a pad) and the context's error word says so
  const bool refused = bad != 0 || all > s.capacity || (s.count && (int64_t)*s.count != all);
  if (refused && tile == 0 && threadIdx.x == 0 && a.dev_err) atomicOr(a.dev_err, TT_DEVERR_BAG_OFFSETS);
  const uint32_t first = tile * kPrepTile + threadIdx.x * kPrepPer;
  int64_t len[kPrepPer], t = 0;
  prep_load(s, first, len);
#pragma unroll
  for (int j = 0; j < kPrepPer; ++j) t += len[j];
  int64_t x = t;                                             // inclusive scan of the threads' sums
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int64_t y = __shfl_up(x, o);
    if (lane >= (uint32_t)o) x += y;
  }
  __syncthreads();
  if (lane == 63) wsum[wave] = x;
  __syncthreads();
  int64_t run = before + x - t;
  for (uint32_t w = 0; w < wave; ++w) run += wsum[w];
  // offs[i] = sum of the lengths before slot i (16-byte stores where the run is whole); the side's last slot also writes offs[slots]
  int64_t o[kPrepPer + 1];
#pragma unroll
  for (int j = 0; j <= kPrepPer; ++j) {
    o[j] = refused ? 0 : run;
    if (j < kPrepPer) run += len[j];
  }
  if (first + kPrepPer <= s.slots && (reinterpret_cast<uintptr_t>(s.offs) & 15) == 0) {
    longlong2* q = reinterpret_cast<longlong2*>(s.offs + first);
#pragma unroll
    for (int j = 0; j < kPrepPer / 2; ++j) q[j] = make_longlong2(o[2 * j], o[2 * j + 1]);
    if (first + kPrepPer == s.slots) s.offs[s.slots] = o[kPrepPer];
  } else {
#pragma unroll
    for (int j = 0; j < kPrepPer; ++j)
      if (first + j < s.slots) {
        s.offs[first + j] = o[j];
        if (first + j + 1 == s.slots) s.offs[s.slots] = o[j + 1];
      }
  }
  if (a.inv_len) {
#pragma unroll
    for (int j = 0; j < kPrepPer; ++j)
      if (first + j < s.slots) {
        const uint32_t k = (first + j) % (uint32_t)s.K;
        a.inv_len[s.slot_base + first + j] = (s.pool[k] != TT_POOL_SUM && len[j] > 0) ? __fdiv_rn(1.0f, (float)len[j]) : 1.0f;
      }
  }
}

// ------------------------------------------------------------------------------------------------
// backward
// ------------------------------------------------------------------------------------------------
struct BagGradSet {
  const char* d[TT_MAX_SIDES];
  int64_t ld[TT_MAX_SIDES];
  uint32_t slot_base[TT_MAX_SIDES];
  uint32_t K[TT_MAX_SIDES];
  int32_t n;
  int32_t E;
  uint32_t C;
  uint32_t total_slots;
  const int32_t* bag_of;
  const float* inv_len;
};
// (weighted form) + the weight of every position; the unweighted instantiations take BagGradSet as it is
template <bool W>
struct BagGradArgs : BagGradSet {};
template <>
struct BagGradArgs<true> : BagGradSet {
  const float* pos_w;
};

__global__ void bag_zero_words_kernel(int32_t* __restrict__ p, int n) {
  if ((int)threadIdx.x < n) p[threadIdx.x] = 0;
}

// ordered sum over positions sorted_src[lo..hi) for one 16-byte column piece: acc = fma(w, x, acc) in that order, kBagBatch
// gradient loads in flight.  The side's fields are picked with selects on kernel-argument scalars, as tt_grad.hip's grad_addr does.
// W: the coefficient of position P is pos_w[P], times inv_len[slot] (one f32 product) where inv_len is given; pos_w[P] is loaded at
// the level of bag_of[P] -- both hang off sorted_src[i].
template <int DT, bool W>
__device__ __forceinline__ void bag_sum_range(const BagGradArgs<W>& a, const int32_t* __restrict__ sorted_src, int32_t lo, int32_t hi,
                                              uint32_t chunk, Acc<4>& acc) {
  constexpr int ESZ = DT == TT_F32 ? 4 : 2;
  for (int32_t i = lo; i < hi; i += kBagBatch) {
    int32_t slot[kBagBatch];
    float pw[kBagBatch];
    if constexpr (W) {
#pragma unroll
      for (int j = 0; j < kBagBatch; ++j) {
        const int32_t P = i + j < hi ? sorted_src[i + j] : -1;
        slot[j] = P >= 0 ? a.bag_of[P] : -1;
        pw[j] = P >= 0 ? a.pos_w[P] : 0.f;
      }
    } else {
#pragma unroll
      for (int j = 0; j < kBagBatch; ++j) slot[j] = i + j < hi ? a.bag_of[sorted_src[i + j]] : -1;
    }
    float w[kBagBatch];
    float x[kBagBatch][4];
#pragma unroll
    for (int j = 0; j < kBagBatch; ++j) {
      w[j] = 0.f;
      x[j][0] = x[j][1] = x[j][2] = x[j][3] = 0.f;
      if (slot[j] < 0) continue;
      const uint32_t sl = (uint32_t)slot[j] < a.total_slots ? (uint32_t)slot[j] : a.total_slots - 1;
      const char* base = a.d[0];
      int64_t ld = a.ld[0];
      uint32_t sb = 0, K = a.K[0];
#pragma unroll
      for (int t = 1; t < TT_MAX_SIDES; ++t) {
        const bool sel = t < a.n && sl >= a.slot_base[t];
        base = sel ? a.d[t] : base;
        ld = sel ? a.ld[t] : ld;
        sb = sel ? a.slot_base[t] : sb;
        K = sel ? a.K[t] : K;
      }
      const uint32_t local = sl - sb;
      const uint32_t b = local / K, k = local - b * K;
      const char* p = base + ((int64_t)b * ld + (int64_t)(k * (uint32_t)a.E + chunk * 4)) * ESZ;
      if constexpr (W) w[j] = a.inv_len ? __fmul_rn(pw[j], a.inv_len[sl]) : pw[j];
      else w[j] = a.inv_len ? a.inv_len[sl] : 1.f;
      if (DT == TT_F32) {
        const float4 t4 = *reinterpret_cast<const float4*>(p);
        x[j][0] = t4.x; x[j][1] = t4.y; x[j][2] = t4.z; x[j][3] = t4.w;
      } else {
        const ushort4 t4 = *reinterpret_cast<const ushort4*>(p);
        x[j][0] = tt_bf2f(t4.x); x[j][1] = tt_bf2f(t4.y); x[j][2] = tt_bf2f(t4.z); x[j][3] = tt_bf2f(t4.w);
      }
    }
#pragma unroll
    for (int j = 0; j < kBagBatch; ++j)
      if (slot[j] >= 0) {
#pragma unroll
        for (int e = 0; e < 4; ++e) acc.v[e] = __fmaf_rn(w[j], x[j][e], acc.v[e]);
      }
  }
}

__device__ __forceinline__ void bag_write_row(float* __restrict__ out, int64_t row, int32_t E, uint32_t chunk, const Acc<4>& acc,
                                              bool accumulate) {
  float* p = out + row * E + chunk * 4;
  float4 t = make_float4(acc.v[0], acc.v[1], acc.v[2], acc.v[3]);
  if (accumulate) {
    const float4 q = *reinterpret_cast<float4*>(p);
    t.x += q.x; t.y += q.y; t.z += q.z; t.w += q.w;
  }
  *reinterpret_cast<float4*>(p) = t;
}

// one lane group per distinct row; rows of more than kLongSeg positions are registered in the workspace's lists (as
// tt_grad.hip's unplanned row pass registers them) and summed chunk by chunk by bag_chunk_kernel
template <int DT, bool W>
__global__ __launch_bounds__(kThreads) void bag_reduce_kernel(BagGradArgs<W> a, const int32_t* __restrict__ sorted_src,
                                                             const int32_t* __restrict__ seg, const int32_t* __restrict__ unique_rows,
                                                             const int32_t* __restrict__ n_unique, int32_t mode, float* __restrict__ out,
                                                             GradWs ws, uint32_t LG) {
  const uint32_t U = (uint32_t)*n_unique;
  const uint32_t gthread = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t lig = gthread % LG;
  const uint32_t ngroups = gridDim.x * blockDim.x / LG;
  for (uint32_t u = gthread / LG; u < U; u += ngroups) {
    const int32_t s0 = seg[u], s1 = seg[u + 1];
    if (s1 - s0 > kLongSeg) {
      register_long_row(ws, u, s0, s1, lig, LG);
      continue;
    }
    const int64_t orow = mode == TT_GRAD_SPARSE ? (int64_t)u : (int64_t)unique_rows[u];
    if (lig < a.C) {
      Acc<4> acc;
      acc.zero();
      bag_sum_range<DT, W>(a, sorted_src, s0, s1, lig, acc);
      bag_write_row(out, orow, a.E, lig, acc, mode == TT_GRAD_DENSE_ACC);
    }
  }
}

template <int DT, bool W>
__global__ __launch_bounds__(kThreads) void bag_chunk_kernel(BagGradArgs<W> a, const int32_t* __restrict__ sorted_src, GradWs ws, uint32_t LG) {
  const uint32_t nchunks = (uint32_t)ws.counters[0];
  if (blockIdx.x == 0 && threadIdx.x == 0) ws.counters[2] = ws.counters[1];      // snapshot for the finish
  const uint32_t gthread = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t lig = gthread % LG;
  const uint32_t ngroups = gridDim.x * blockDim.x / LG;
  for (uint32_t c = gthread / LG; c < nchunks; c += ngroups) {
    if (lig >= a.C) continue;
    Acc<4> acc;
    acc.zero();
    bag_sum_range<DT, W>(a, sorted_src, ws.chunk_lo[c], ws.chunk_hi[c], lig, acc);
    bag_write_row(ws.chunk_partial, (int64_t)c, a.E, lig, acc, false);
  }
}

__global__ __launch_bounds__(kThreads) void bag_long_finish_kernel(int32_t E, uint32_t C, const int32_t* __restrict__ seg,
                                                                  const int32_t* __restrict__ unique_rows, int32_t mode,
                                                                  float* __restrict__ out, GradWs ws, uint32_t LG) {
  __shared__ float part[kFinishMaxFloats];
  long_rows_finish_into<4>(E, C, seg, unique_rows, mode, out, ws, LG, part);
}

static int bag_unsupported(const char* who, const char* what) {
  tt_set_error("%s: %s", who, what);
  return TT_ERR_UNSUPPORTED;
}

}  // namespace

// tt_embed_bag_fwd (cap false) and its capacity form (cap true: nnz is each side's capacity, uncovered positions get table_rows / -1)
static int bag_fwd_impl(tt_ctx* ctx, const float* table, int64_t table_rows, int32_t E, const tt_bag_side* sides, int32_t n_sides,
                        int64_t B, int32_t* rows_out, int32_t* bag_of, tt_stream stream, bool cap, bool weighted = false,
                        const float* const* weights = nullptr, float* w_out = nullptr, const tt_bag_weight_src* wsrc = nullptr) {
  TT_CHECK_ARG(ctx && table && sides, "tt_embed_bag_fwd: NULL argument");
  TT_CHECK_ARG(n_sides >= 1 && n_sides <= TT_MAX_SIDES, "tt_embed_bag_fwd: n_sides=%d not in [1,%d]", n_sides, TT_MAX_SIDES);
  TT_CHECK_ARG(B >= 0 && table_rows >= 1 && table_rows <= INT32_MAX, "tt_embed_bag_fwd: bad B=%lld rows=%lld", (long long)B, (long long)table_rows);
  if (E % 4 != 0 || E < 4 || E > 256) return bag_unsupported("tt_embed_bag_fwd", "E must be a multiple of 4 in [4, 256]");
  if (!tt_aligned(table, 16)) return bag_unsupported("tt_embed_bag_fwd", "the table must be 16-byte aligned");
  BagFwdArgs<2> a{};         // (the per-id launch passes its BagFwdArgs<1> part, the unweighted one its BagSet part)
  bool any_pw = false;
  a.n = n_sides;
  a.E = E;
  a.C = (uint32_t)(E / 4);
  a.LG = pow2_at_least(a.C);
  int64_t slots = 0, positions = 0;
  for (int i = 0; i < n_sides; ++i) {
    const tt_bag_side& s = sides[i];
    a.w[i] = weighted && weights ? weights[i] : nullptr;
    if (wsrc) {                                                // the _posw entries: one source per side, or none
      const tt_bag_weight_src& ws = wsrc[i];
      TT_CHECK_ARG(!(ws.weights && ws.param), "tt_embed_bag_fwd_posw: side %d has both per-id weights and a position-weight parameter", i);
      a.w[i] = ws.weights;
      if (ws.param) {
        TT_CHECK_ARG(ws.pw_offset && ws.pw_len, "tt_embed_bag_fwd_posw: side %d has a parameter without pw_offset / pw_len", i);
        TT_CHECK_ARG(ws.n_param >= 1 && ws.n_param < ((int64_t)1 << 31), "tt_embed_bag_fwd_posw: side %d bad n_param=%lld", i, (long long)ws.n_param);
        if (!tt_aligned(ws.param, 4) || !tt_aligned(ws.pw_offset, 4) || !tt_aligned(ws.pw_len, 4))
          return bag_unsupported("tt_embed_bag_fwd_posw", "the parameter and its key directory must be 4-byte aligned");
        a.pw_param[i] = ws.param; a.pw_off[i] = ws.pw_offset; a.pw_len[i] = ws.pw_len; a.pw_n[i] = ws.n_param;
        any_pw = true;
      }
    }
    TT_CHECK_ARG(!(rows_out && (a.w[i] || a.pw_param[i]) && !w_out), "%s: rows_out with weights on side %d needs w_out",
                 wsrc ? "tt_embed_bag_fwd_posw" : "tt_embed_bag_fwd_w", i);
    if (!tt_aligned(a.w[i], 4) || !tt_aligned(w_out, 4)) return bag_unsupported("tt_embed_bag_fwd_w", "weights and w_out must be 4-byte aligned");
    TT_CHECK_ARG(s.K >= 1 && s.nnz >= 0, "tt_embed_bag_fwd: side %d has K=%d nnz=%lld", i, s.K, (long long)s.nnz);
    TT_CHECK_ARG(s.offsets && s.key_row_offset && s.key_vocab && s.key_pool && s.out && (s.ids || s.nnz == 0), "tt_embed_bag_fwd: side %d has NULL pointers", i);
    TT_CHECK_ARG(s.out_dtype == TT_F32 || s.out_dtype == TT_BF16, "tt_embed_bag_fwd: side %d bad out_dtype %d", i, s.out_dtype);
    TT_CHECK_ARG(s.ld_out >= (int64_t)s.K * E, "tt_embed_bag_fwd: side %d ld_out %lld < K*E", i, (long long)s.ld_out);
    const size_t esz = s.out_dtype == TT_BF16 ? 2 : 4;
    if (s.ld_out % 4 != 0 || !tt_aligned(s.out, 4 * esz)) return bag_unsupported("tt_embed_bag_fwd", "outputs must be 4-element aligned (base and ld_out)");
    a.s[i] = BagSideDev{s.ids, s.offsets, s.key_row_offset, s.key_vocab, s.key_pool, reinterpret_cast<char*>(s.out), s.ld_out, s.nnz,
                        (uint32_t)slots, (uint32_t)positions, s.K, s.out_dtype};
    slots += B * s.K;
    positions += s.nnz;
  }
  TT_CHECK_ARG(slots * a.LG < ((int64_t)1 << 31) && positions < ((int64_t)1 << 31), "tt_embed_bag_fwd: %lld bags / %lld ids exceed the 2^31 index range",
               (long long)slots, (long long)positions);
  if (slots == 0) return TT_OK;
  a.total_slots = (uint32_t)slots;
  a.table_rows = (int32_t)table_rows;
  a.dev_err = ctx->dev_err;
  a.rows_out = rows_out;
  a.bag_of = bag_of;
  a.pad_row = cap ? (int32_t)table_rows : -1;
  a.total_pos = (uint32_t)positions;
  // (capacity form: the grid is sized by the bags and the capacities, never by the live count)
  const int64_t threads = cap && positions > slots * a.LG ? positions : slots * a.LG;
  a.w_out = w_out;
  if (any_pw) {
    bag_fwd_kernel<2><<<grid_for(ctx, threads), kThreads, 0, reinterpret_cast<hipStream_t>(stream)>>>(a, table);
  } else if (weighted) {
    bag_fwd_kernel<1><<<grid_for(ctx, threads), kThreads, 0, reinterpret_cast<hipStream_t>(stream)>>>(static_cast<const BagFwdArgs<1>&>(a), table);
  } else {
    BagFwdArgs<0> u{};
    static_cast<BagSet&>(u) = a;
    bag_fwd_kernel<0><<<grid_for(ctx, threads), kThreads, 0, reinterpret_cast<hipStream_t>(stream)>>>(u, table);
  }
  TT_LAUNCH_CHECK();
  return TT_OK;
}

// tt_embed_bag_rows[_w]: the rows-only launch.  No table, no E, no outputs: a side's `out` fields are not looked at.
static int bag_rows_impl(tt_ctx* ctx, int64_t table_rows, const tt_bag_side* sides, int32_t n_sides, int64_t B, int32_t* rows_out,
                         int32_t* bag_of, const float* const* weights, float* w_out, tt_stream stream, const char* who) {
  TT_CHECK_ARG(ctx && sides, "%s: NULL argument", who);
  TT_CHECK_ARG(n_sides >= 1 && n_sides <= TT_MAX_SIDES, "%s: n_sides=%d not in [1,%d]", who, n_sides, TT_MAX_SIDES);
  TT_CHECK_ARG(B >= 0 && table_rows >= 1 && table_rows <= INT32_MAX, "%s: bad B=%lld rows=%lld", who, (long long)B, (long long)table_rows);
  BagFwdArgs<4> a{};         // (the unweighted launch passes its BagSet part)
  a.n = n_sides;
  a.C = a.LG = kBagBatch;
  int64_t slots = 0, positions = 0;
  for (int i = 0; i < n_sides; ++i) {
    const tt_bag_side& s = sides[i];
    a.w[i] = weights ? weights[i] : nullptr;
    TT_CHECK_ARG(!(rows_out && a.w[i] && !w_out), "%s: rows_out with weights on side %d needs w_out", who, i);
    if (!tt_aligned(a.w[i], 4) || !tt_aligned(w_out, 4)) return bag_unsupported(who, "weights and w_out must be 4-byte aligned");
    TT_CHECK_ARG(s.K >= 1 && s.nnz >= 0, "%s: side %d has K=%d nnz=%lld", who, i, s.K, (long long)s.nnz);
    TT_CHECK_ARG(s.offsets && s.key_row_offset && s.key_vocab && (s.ids || s.nnz == 0), "%s: side %d has NULL pointers", who, i);
    a.s[i] = BagSideDev{s.ids, s.offsets, s.key_row_offset, s.key_vocab, s.key_pool, nullptr, 0, s.nnz, (uint32_t)slots, (uint32_t)positions,
                        s.K, TT_F32};
    slots += B * s.K;
    positions += s.nnz;
  }
  TT_CHECK_ARG(slots * a.LG < ((int64_t)1 << 31) && positions < ((int64_t)1 << 31), "%s: %lld bags / %lld ids exceed the 2^31 index range", who,
               (long long)slots, (long long)positions);
  if (slots == 0) return TT_OK;
  a.total_slots = (uint32_t)slots;
  a.table_rows = (int32_t)table_rows;
  a.dev_err = ctx->dev_err;
  a.rows_out = rows_out;
  a.bag_of = bag_of;
  a.pad_row = -1;
  a.total_pos = (uint32_t)positions;
  a.w_out = w_out;
  if (weights) {
    bag_fwd_kernel<4><<<grid_for(ctx, slots * a.LG), kThreads, 0, reinterpret_cast<hipStream_t>(stream)>>>(a, nullptr);
  } else {
    BagFwdArgs<3> u{};
    static_cast<BagSet&>(u) = a;
    bag_fwd_kernel<3><<<grid_for(ctx, slots * a.LG), kThreads, 0, reinterpret_cast<hipStream_t>(stream)>>>(u, nullptr);
  }
  TT_LAUNCH_CHECK();
  return TT_OK;
}

extern "C" {

int tt_embed_bag_rows(tt_ctx* ctx, int64_t table_rows, const tt_bag_side* sides, int32_t n_sides, int64_t B, int32_t* rows_out,
                      int32_t* bag_of, tt_stream stream) {
  return bag_rows_impl(ctx, table_rows, sides, n_sides, B, rows_out, bag_of, nullptr, nullptr, stream, "tt_embed_bag_rows");
}

int tt_embed_bag_rows_w(tt_ctx* ctx, int64_t table_rows, const tt_bag_side* sides, int32_t n_sides, int64_t B, int32_t* rows_out,
                        int32_t* bag_of, const float* const* weights, float* w_out, tt_stream stream) {
  TT_CHECK_ARG(weights, "tt_embed_bag_rows_w: NULL weights array (a side without weights has a NULL entry)");
  return bag_rows_impl(ctx, table_rows, sides, n_sides, B, rows_out, bag_of, weights, w_out, stream, "tt_embed_bag_rows_w");
}

int tt_embed_bag_fwd(tt_ctx* ctx, const float* table, int64_t table_rows, int32_t E, const tt_bag_side* sides, int32_t n_sides,
                     int64_t B, int32_t* rows_out, int32_t* bag_of, tt_stream stream) {
  return bag_fwd_impl(ctx, table, table_rows, E, sides, n_sides, B, rows_out, bag_of, stream, false);
}

int tt_embed_bag_fwd_cap(tt_ctx* ctx, const float* table, int64_t table_rows, int32_t E, const tt_bag_side* sides, int32_t n_sides,
                         int64_t B, int32_t* rows_out, int32_t* bag_of, tt_stream stream) {
  TT_CHECK_ARG(table_rows < INT32_MAX, "tt_embed_bag_fwd_cap: no room for the pad row behind %lld rows", (long long)table_rows);
  return bag_fwd_impl(ctx, table, table_rows, E, sides, n_sides, B, rows_out, bag_of, stream, true);
}

int tt_embed_bag_fwd_w(tt_ctx* ctx, const float* table, int64_t table_rows, int32_t E, const tt_bag_side* sides, int32_t n_sides,
                       int64_t B, int32_t* rows_out, int32_t* bag_of, const float* const* weights, float* w_out, tt_stream stream) {
  TT_CHECK_ARG(weights, "tt_embed_bag_fwd_w: NULL weights array (a side without weights has a NULL entry)");
  return bag_fwd_impl(ctx, table, table_rows, E, sides, n_sides, B, rows_out, bag_of, stream, false, true, weights, w_out);
}

int tt_embed_bag_fwd_cap_w(tt_ctx* ctx, const float* table, int64_t table_rows, int32_t E, const tt_bag_side* sides, int32_t n_sides,
                           int64_t B, int32_t* rows_out, int32_t* bag_of, const float* const* weights, float* w_out, tt_stream stream) {
  TT_CHECK_ARG(weights, "tt_embed_bag_fwd_cap_w: NULL weights array (a side without weights has a NULL entry)");
  TT_CHECK_ARG(table_rows < INT32_MAX, "tt_embed_bag_fwd_cap_w: no room for the pad row behind %lld rows", (long long)table_rows);
  return bag_fwd_impl(ctx, table, table_rows, E, sides, n_sides, B, rows_out, bag_of, stream, true, true, weights, w_out);
}

// a call whose sides all lack a parameter launches the _w kernel (with per-id weights or none: its bits)
int tt_embed_bag_fwd_posw(tt_ctx* ctx, const float* table, int64_t table_rows, int32_t E, const tt_bag_side* sides, int32_t n_sides,
                        int64_t B, int32_t* rows_out, int32_t* bag_of, const tt_bag_weight_src* srcs, float* w_out, tt_stream stream) {
  TT_CHECK_ARG(srcs, "tt_embed_bag_fwd_posw: NULL weight sources (a side without weights has an all-NULL entry)");
  return bag_fwd_impl(ctx, table, table_rows, E, sides, n_sides, B, rows_out, bag_of, stream, false, true, nullptr, w_out, srcs);
}

int tt_embed_bag_fwd_cap_posw(tt_ctx* ctx, const float* table, int64_t table_rows, int32_t E, const tt_bag_side* sides, int32_t n_sides,
                            int64_t B, int32_t* rows_out, int32_t* bag_of, const tt_bag_weight_src* srcs, float* w_out, tt_stream stream) {
  TT_CHECK_ARG(srcs, "tt_embed_bag_fwd_cap_posw: NULL weight sources (a side without weights has an all-NULL entry)");
  TT_CHECK_ARG(table_rows < INT32_MAX, "tt_embed_bag_fwd_cap_posw: no room for the pad row behind %lld rows", (long long)table_rows);
  return bag_fwd_impl(ctx, table, table_rows, E, sides, n_sides, B, rows_out, bag_of, stream, true, true, nullptr, w_out, srcs);
}

size_t tt_bag_prepare_workspace_bytes(const int64_t* side_slots, int32_t n_sides) {
  size_t tiles = 0;
  for (int i = 0; side_slots && i < n_sides; ++i) tiles += (size_t)tt_cdiv(side_slots[i] > 0 ? side_slots[i] : 1, kPrepTile);
  return sizeof(int64_t) * (tiles > 0 ? tiles : 1);
}

int tt_bag_prepare(tt_ctx* ctx, const tt_bag_lengths* sides, int32_t n_sides, int64_t B, float* inv_len, void* workspace,
                   size_t workspace_bytes, tt_stream stream) {
  TT_CHECK_ARG(ctx && sides && workspace, "tt_bag_prepare: NULL argument");
  TT_CHECK_ARG(n_sides >= 1 && n_sides <= TT_MAX_SIDES && B >= 0, "tt_bag_prepare: n_sides=%d B=%lld", n_sides, (long long)B);
  if (!tt_aligned(workspace, 8)) return bag_unsupported("tt_bag_prepare", "the workspace must be 8-byte aligned");
  PrepSet a{};
  a.n = n_sides;
  int64_t slots = 0, tiles = 0, per_side[TT_MAX_SIDES];
  for (int i = 0; i < n_sides; ++i) {
    const tt_bag_lengths& s = sides[i];
    TT_CHECK_ARG(s.K >= 1 && s.capacity >= 0 && s.capacity < ((int64_t)1 << 31), "tt_bag_prepare: side %d has K=%d capacity=%lld", i, s.K,
                 (long long)s.capacity);
    TT_CHECK_ARG(s.lengths && s.offsets && (s.key_pool || !inv_len), "tt_bag_prepare: side %d has NULL pointers", i);
    per_side[i] = B * s.K;
    a.s[i] = PrepSide{s.lengths, s.key_pool, s.count, s.offsets, s.capacity, (uint32_t)per_side[i], (uint32_t)slots, (uint32_t)tiles, s.K};
    slots += per_side[i];
    tiles += tt_cdiv(per_side[i] > 0 ? per_side[i] : 1, kPrepTile);
  }
  TT_CHECK_ARG(slots < ((int64_t)1 << 31), "tt_bag_prepare: %lld bags exceed the 2^31 index range", (long long)slots);
  if (slots == 0) return TT_OK;
  if (workspace_bytes < tt_bag_prepare_workspace_bytes(per_side, n_sides)) {
    tt_set_error("tt_bag_prepare: workspace %zu < required %zu", workspace_bytes, tt_bag_prepare_workspace_bytes(per_side, n_sides));
    return TT_ERR_WORKSPACE;
  }
  a.tiles = (uint32_t)tiles;
  a.inv_len = inv_len;
  a.tile_sum = reinterpret_cast<int64_t*>(workspace);
  a.dev_err = ctx->dev_err;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  bag_prep_reduce_kernel<<<(int)tiles, kThreads, 0, st>>>(a);
  TT_LAUNCH_CHECK();
  bag_prep_scan_kernel<<<(int)tiles, kThreads, 0, st>>>(a);
  TT_LAUNCH_CHECK();
  return TT_OK;
}

size_t tt_embed_bag_grad_workspace_bytes(int64_t nnz, int32_t E) { return grad_layout(nullptr, nnz > 0 ? nnz : 1, E > 0 ? E : 1).bytes; }

int tt_embed_bag_grad_bwd(tt_ctx* ctx, const tt_grad_src* srcs, int32_t n_srcs, int64_t B, int32_t E, const int32_t* bag_of,
                          const float* inv_len, const int32_t* sorted_src, const int32_t* seg_offsets, const int32_t* unique_rows,
                          const int32_t* n_unique, int64_t nnz, int32_t mode, float* out, void* workspace, size_t workspace_bytes,
                          tt_stream stream) {
  return tt_embed_bag_grad_bwd_w(ctx, srcs, n_srcs, B, E, bag_of, inv_len, nullptr, sorted_src, seg_offsets, unique_rows, n_unique, nnz, mode,
                                 out, workspace, workspace_bytes, stream);
}

// pos_w NULL: the unweighted kernels, launched as tt_embed_bag_grad_bwd always launched them
int tt_embed_bag_grad_bwd_w(tt_ctx* ctx, const tt_grad_src* srcs, int32_t n_srcs, int64_t B, int32_t E, const int32_t* bag_of,
                            const float* inv_len, const float* pos_w, const int32_t* sorted_src, const int32_t* seg_offsets,
                            const int32_t* unique_rows, const int32_t* n_unique, int64_t nnz, int32_t mode, float* out, void* workspace,
                            size_t workspace_bytes, tt_stream stream) {
  TT_CHECK_ARG(ctx && srcs && out, "tt_embed_bag_grad_bwd: NULL argument");
  TT_CHECK_ARG(n_srcs >= 1 && n_srcs <= TT_MAX_SIDES, "tt_embed_bag_grad_bwd: n_srcs=%d", n_srcs);
  TT_CHECK_ARG(mode >= TT_GRAD_SPARSE && mode <= TT_GRAD_DENSE_ACC, "tt_embed_bag_grad_bwd: bad mode %d (the PLANNED / DEFER_FINISH / SHORT forms are not offered)", mode);
  TT_CHECK_ARG(B >= 0 && nnz >= 0 && nnz < ((int64_t)1 << 31), "tt_embed_bag_grad_bwd: bad B / nnz");
  if (E % 4 != 0 || E < 4 || E > 256) return bag_unsupported("tt_embed_bag_grad_bwd", "E must be a multiple of 4 in [4, 256]");
  if (!tt_aligned(out, 16)) return bag_unsupported("tt_embed_bag_grad_bwd", "out must be 16-byte aligned");
  BagGradArgs<true> a{};      // (the unweighted launches pass its BagGradSet part)
  a.n = n_srcs;
  a.E = E;
  int64_t slots = 0;
  for (int i = 0; i < n_srcs; ++i) {
    const tt_grad_src& s = srcs[i];
    TT_CHECK_ARG(s.K >= 1 && s.d_out, "tt_embed_bag_grad_bwd: src %d NULL / no keys", i);
    TT_CHECK_ARG(s.dtype == TT_F32 || s.dtype == TT_BF16, "tt_embed_bag_grad_bwd: src %d bad dtype", i);
    TT_CHECK_ARG(s.dtype == srcs[0].dtype, "tt_embed_bag_grad_bwd: all sources must share one dtype (src %d differs)", i);
    TT_CHECK_ARG(s.ld >= (int64_t)s.K * E, "tt_embed_bag_grad_bwd: src %d ld %lld < K*E", i, (long long)s.ld);
    const size_t esz = s.dtype == TT_BF16 ? 2 : 4;
    if (s.ld % 4 != 0 || !tt_aligned(s.d_out, 4 * esz)) return bag_unsupported("tt_embed_bag_grad_bwd", "sources must be 4-element aligned (base and ld)");
    a.d[i] = reinterpret_cast<const char*>(s.d_out);
    a.ld[i] = s.ld;
    a.slot_base[i] = (uint32_t)slots;
    a.K[i] = (uint32_t)s.K;
    slots += B * s.K;
  }
  TT_CHECK_ARG(slots < ((int64_t)1 << 31), "tt_embed_bag_grad_bwd: too many slots");
  if (nnz == 0 || slots == 0) return TT_OK;
  TT_CHECK_ARG(bag_of && sorted_src && seg_offsets && unique_rows && n_unique && workspace, "tt_embed_bag_grad_bwd: NULL plan / bag_of / workspace");
  if (workspace_bytes < tt_embed_bag_grad_workspace_bytes(nnz, E)) {
    tt_set_error("tt_embed_bag_grad_bwd: workspace %zu < required %zu", workspace_bytes, tt_embed_bag_grad_workspace_bytes(nnz, E));
    return TT_ERR_WORKSPACE;
  }
  uint32_t LG;
  row_mapping(E, true, &a.C, &LG);
  if (!finish_fits(E, LG)) return bag_unsupported("tt_embed_bag_grad_bwd", "E too wide for the long-row finish");      // (E <= 256 fits: 1024 floats at most)
  a.total_slots = (uint32_t)slots;
  a.bag_of = bag_of;
  a.inv_len = inv_len;
  a.pos_w = pos_w;
  const GradLayout gl = grad_layout(reinterpret_cast<char*>(workspace), nnz, E);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (int rc = tt_deferred_flush(ctx, TT_DQ_ALL)) return rc;      // the sources may be the products of a launch still queued
  const int g1 = grid_for(ctx, nnz * LG), g2 = grid_for(ctx, gl.max_chunks * LG), g3 = long_row_blocks(ctx, gl);
  const int dt = srcs[0].dtype;
  bag_zero_words_kernel<<<1, 64, 0, st>>>(gl.ws.counters, 2);
  TT_LAUNCH_CHECK();
  BagGradArgs<false> u{};
  static_cast<BagGradSet&>(u) = a;
#define TT_BAG_REDUCE(DT, W, A) bag_reduce_kernel<DT, W><<<g1, kThreads, 0, st>>>(A, sorted_src, seg_offsets, unique_rows, n_unique, mode, out, gl.ws, LG)
#define TT_BAG_CHUNK(DT, W, A) bag_chunk_kernel<DT, W><<<g2, kThreads, 0, st>>>(A, sorted_src, gl.ws, LG)
  if (pos_w) { if (dt == TT_F32) TT_BAG_REDUCE(TT_F32, true, a); else TT_BAG_REDUCE(TT_BF16, true, a); }
  else { if (dt == TT_F32) TT_BAG_REDUCE(TT_F32, false, u); else TT_BAG_REDUCE(TT_BF16, false, u); }
  TT_LAUNCH_CHECK();
  if (pos_w) { if (dt == TT_F32) TT_BAG_CHUNK(TT_F32, true, a); else TT_BAG_CHUNK(TT_BF16, true, a); }
  else { if (dt == TT_F32) TT_BAG_CHUNK(TT_F32, false, u); else TT_BAG_CHUNK(TT_BF16, false, u); }
  TT_LAUNCH_CHECK();
#undef TT_BAG_REDUCE
#undef TT_BAG_CHUNK
  bag_long_finish_kernel<<<g3, kThreads, 0, st>>>(E, a.C, seg_offsets, unique_rows, mode, out, gl.ws, LG);
  TT_LAUNCH_CHECK();
  return TT_OK;
}

}  // extern "C"
