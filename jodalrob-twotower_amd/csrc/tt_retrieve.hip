// Catalogue-wide top-k retrieval and rank (tt_retrieve_topk_bf16 / tt_retrieve_topk_f32): the catalogue streams past the
// queries in 32-row tiles, every query keeps its best k, and no score is ever written to memory.
//
// Three launches on the caller's stream, no host synchronisation:
//   pos   (rank only)  the positive's score s_p of every query, computed by the SAME tile routine as the sweep, so that the
//                      sweep's comparisons against it are bit-for-bit;
//   sweep              grid (query tile of 32 x catalogue split).  A wave owns 32 queries and the split's tiles; per tile it forms
//                      the 32 x 32 score block X[row][query] with lane (c, h) holding query c and rows rowmap(r, h) (as in
//                      tt_score_bf16.hip).  Each query has a running threshold (its k-th best so far): one v_max3 chain and one
//                      compare on the accumulators reject a tile in the common case.  Scores that pass go into the query's LDS
//                      candidate region; when a region is nearly full the wave selects the k best of it (binary search for
//                      the k-th largest order key, index tie break) and raises the threshold.  The split's k best (unsorted)
//                      and its rank counts go to the workspace;
//   merge              one wave per query: the k best of the S partial lists, sorted, and the summed rank.
// Order: value descending, then lower catalogue index (tt_topk_rows).  Rank: #{c : s > s_p} + #{c < p : s == s_p}
// (tt_diag_rank_rows).  Every score comes from one instruction sequence whichever wave or split computes it, and the selection
// is exact under a total order, so results are bitwise identical across runs and split counts.
//
// Exclusion lists (tt_excl_retrieve_topk_*: the sweep's EXCL = true instantiation): query q's ascending CSR list of catalogue
// rows is removed before the k-th-best filter and the rank counts see them.  Each lane holds a cursor into its query's list
// (binary-searched to the split's first row) and the next excluded row in a register: a tile without excluded rows costs one
// compare and one __any; otherwise the wave walks the tile's entries and sets the matching scores to -inf, which neither the
// filter (threshold >= -inf, strict compare) nor the rank counts (strict compare against a finite s_p) ever take.
//
// Attribute filters (tt_filt_retrieve_topk_*: the sweep's FILT = true instantiations): catalogue row c carries W tag words, query
// q an `any` and an `all` mask of W words; rows that fail (tags & any) != 0 (unless any == 0) or (tags & all) == all get -inf at
// the same point as the excluded ones.  A tile's 32 W tag words are contiguous: the wave reads them with one coalesced load
// (W > 2: two, 16 rows each) a tile ahead, one word per lane, and every lane fetches the words of its 16 rows with ds_bpermute.
//
// Score ceilings (tt_ceil_retrieve_topk_*: the sweep's CEIL = true instantiations): query q's scores at or above ceil[q] leave its
// top-k -- after the rank counts, which never see the ceiling, and before the k-th-best filter, so that the k slots go to the best
// rows BELOW the ceiling (hard-negative mining under a positive-aware ceiling).  One register and one compare per score; a NaN
// ceiling compares false and removes nothing.  tt_pair_scores_* is the pos launch alone, writing to the caller: the score of a
// (query, row) pair exactly as the sweep forms it, which is what such a ceiling is derived from.
//
// k up to 512 (the sweep's and the merge's BIGK = true instantiations, k > 64): the same sweep with one wave per workgroup and
// a region of ret_big_slots(k) slots per query, up to the CU's whole 160 KB of LDS at k > 256; the splits are capped so that
// S k <= 2048, which keeps the merge's selection and the workspace of the k = 64 call.  k <= 64 runs the code it always ran.
#include "tt_score_bf16.h"

#include <math.h>

namespace {

using namespace ttscore;

constexpr int kRetWaves = 2;        // waves per sweep workgroup, k <= 64 (each its own 32 queries; <= 64 KB of LDS at k = 64)
constexpr int kRetCap = 64;         // candidate slots per query beyond the k kept ones (>= 32: room for one whole tile)
constexpr int kRetMaxSplits = 32;
constexpr int kRetSmallK = 64;      // k above this runs the large-k sweep (BIGK: one wave per workgroup) and the strided merge
constexpr int kRetMaxK = 512;
constexpr size_t kRetBigLds = 640 * 32 * 8;                    // a CU's whole LDS (160 KB): 640 slots of 32 queries x (key, index)

// Slots of a query's region in the large-k sweep (one wave per workgroup).  The CU's 640 slots go evenly to as many waves, at
// most four, as leave every region k + kRetCap slots or more: 4 waves for k <= 96, 3 for k <= 146, 2 for k <= 256, else 1.  What
// a region holds beyond k is spare room, so a select() comes every slots - k - 32 candidates or more, not every 32.  (210, not
// 213: every size is a whole number of 1280-byte LDS allocation granules.)
__host__ __device__ constexpr int ret_big_slots(int k) { return k <= 96 ? 160 : k <= 146 ? 210 : k <= 256 ? 320 : 640; }
static_assert(ret_big_slots(kRetSmallK + 1) >= kRetSmallK + 1 + kRetCap && ret_big_slots(96) >= 96 + kRetCap &&
              ret_big_slots(146) >= 146 + kRetCap && ret_big_slots(256) >= 256 + kRetCap && ret_big_slots(kRetMaxK) >= kRetMaxK + kRetCap &&
              (size_t)ret_big_slots(kRetMaxK) * 256 <= kRetBigLds, "a region holds k + kRetCap slots and fits the CU");
constexpr int32_t kSentIdx = 0x7fffffff;   // index of an empty list entry (order key 0: below every score)

// order-preserving key of a score: larger float <=> larger key; -0 and +0 share one key
__device__ __forceinline__ uint32_t okey(float x) {
  const uint32_t u = __float_as_uint(x + 0.f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float okey_val(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// largest float below x (x >= s_p  <=>  x > below(s_p) for the rank's "tie before the positive" rows)
__device__ __forceinline__ float below(float x) {
  if (x != x || x == -INFINITY) return x;
  if (x == 0.f) return -__uint_as_float(1u);
  const uint32_t u = __float_as_uint(x);
  return __uint_as_float(x > 0.f ? u - 1 : u + 1);
}

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// ---- score tiles: acc[r] = s(query 32 qt + c, catalogue row 32 t + rowmap(r, h)) ----------------------------------------------
template <int KS>
struct TileBf16 {             // packed images (tt_score_pack_bf16): s = <Q, C> times the scales the images carry
  const __bf16* q_rows;
  const __bf16* c_rows;
  bf16x8 qf[KS];
  struct Frag { bf16x8 v[KS]; };
  __device__ __forceinline__ void load_queries(int64_t qt, int c, int h, int64_t) { load_bfrag<KS>(q_rows, qt, c, h, qf); }
  __device__ __forceinline__ void load(int64_t t, int c, int h, Frag& f) const { load_bfrag<KS>(c_rows, t, c, h, f.v); }
  __device__ __forceinline__ void score(const Frag& f, int64_t, int, int, f32x16& acc) const {
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
    for (int s = 0; s < KS; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.v[s], qf[s], acc, 0, 0, 0);
  }
};

template <bool VEC>
struct TileF32 {              // plain f32 rows: s = inv_t * (f32 FMA chain over k = 0 .. D-1)
  const float* Q;
  const float* Cm;
  int64_t nQ, nC;
  int D;
  float inv_t;
  const float* qrow;
  struct Frag {};
  __device__ __forceinline__ void load_queries(int64_t qt, int c, int, int64_t) {
    const int64_t q = 32 * qt + c;
    qrow = Q + (q < nQ ? q : nQ - 1) * D;
  }
  __device__ __forceinline__ void load(int64_t, int, int, Frag&) const {}
  __device__ __forceinline__ void score(const Frag&, int64_t t, int, int h, f32x16& acc) const {
    const float* rp[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t row = 32 * t + rowmap(r, h);
      rp[r] = Cm + (row < nC ? row : nC - 1) * D;
      acc[r] = 0.f;
    }
    if (VEC) {
      for (int k = 0; k < D; k += 4) {
        const float4 q = *reinterpret_cast<const float4*>(qrow + k);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float4 v = *reinterpret_cast<const float4*>(rp[r] + k);
          acc[r] = fmaf(q.w, v.w, fmaf(q.z, v.z, fmaf(q.y, v.y, fmaf(q.x, v.x, acc[r]))));
        }
      }
    } else {
      for (int k = 0; k < D; ++k) {
        const float q = qrow[k];
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = fmaf(q, rp[r][k], acc[r]);
      }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] *= inv_t;
  }
};

struct RetArgs {
  int64_t nQ, nC;
  int k, S;
  const int32_t* pos32;       // positives (one of the two, or both NULL)
  const int64_t* pos64;
  float* sp;                  // [nQ] positive scores (NaN: positive out of range)
  int32_t* part_rank;         // [nQ][S] or NULL
  uint32_t* part_key;         // [nQ][S][k] order keys (0 = empty)
  int32_t* part_idx;          // [nQ][S][k]
  float* vals;                // [nQ][k] out
  int64_t* idx;               // [nQ][k] out
  int32_t* rank;              // [nQ] out or NULL
  const int64_t* excl_off;    // [nQ + 1] CSR offsets of the exclusion lists (EXCL sweep only)
  const int32_t* excl_rows;   // [excl_off[nQ]] ascending catalogue rows per query
  const uint32_t* tags;       // [nC][W] tag words of the catalogue rows (FILT sweep only)
  const uint32_t* q_any;      // [nQ][W] or NULL: a row must share a bit with a non-zero mask
  const uint32_t* q_all;      // [nQ][W] or NULL: a row must hold every bit of the mask
  int W;                      // 1 .. 4
  const float* ceil;          // [nQ] score ceilings (CEIL sweep only): s >= ceil[q] never enters query q's top-k
};

__device__ __forceinline__ int64_t positive_of(const RetArgs& a, int64_t q) { return a.pos64 ? a.pos64[q] : (int64_t)a.pos32[q]; }

// ---- pos: s_p per query ---------------------------------------------------------------------------------------------------------
template <class Tile>
__global__ __launch_bounds__(64) void retrieve_pos_kernel(Tile tile, RetArgs a) {
  const int lane = threadIdx.x, c = lane & 31, h = lane >> 5;
  const int64_t qt = blockIdx.x, q0 = 32 * qt;
  tile.load_queries(qt, c, h, a.nQ);
  for (int i = 0; i < 32 && q0 + i < a.nQ; ++i) {
    const int64_t p = positive_of(a, q0 + i);                 // wave-uniform
    if (p < 0 || p >= a.nC) {
      if (lane == 0) a.sp[q0 + i] = __uint_as_float(0x7fc00000u);
      continue;
    }
    typename Tile::Frag f;
    f32x16 acc;
    tile.load(p / 32, c, h, f);
    tile.score(f, p / 32, c, h, acc);
    float v = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r)
      if (rowmap(r, h) == (int)(p & 31)) v = acc[r];
    if (c == i && h == (int)((p >> 2) & 1)) a.sp[q0 + i] = v;
  }
}

// attribute filter of one tile: -inf for the rows whose tags miss a required bit (mall) or share none with a non-zero many.
// tg0 / tg1: the tile's tag words as the sweep loads them; the word of row rowmap(r, h) sits in lane (row - R j) WW + w of tg[j].
template <int WW>
__device__ __forceinline__ void filter_tile(f32x16& acc, int h, uint32_t tg0, uint32_t tg1, const uint32_t (&many)[4],
                                            const uint32_t (&mall)[4], uint32_t hit0) {
  constexpr int R = WW <= 2 ? 32 : 16;
  int base = 16 * h * WW;                                       // byte address of lane 4 h WW
  asm volatile("" : "+v"(base));                                // opaque per tile: base + constant folds into the offset field
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = rowmap(r, 0), j = row / R;
    uint32_t bad = 0u, hit = hit0;
#pragma unroll
    for (int w = 0; w < WW; ++w) {
      const uint32_t x = (uint32_t)__builtin_amdgcn_ds_bpermute(base + 4 * ((row - R * j) * WW + w), (int)(j ? tg1 : tg0));
      bad |= mall[w] & ~x;
      hit |= many[w] & x;
    }
    if (bad != 0u || hit == 0u) acc[r] = -INFINITY;
  }
}

// ---- sweep ------------------------------------------------------------------------------------------------------------------
// BIGK (64 < k <= 512): one wave per workgroup and ret_big_slots(k) slots per query, up to the CU's whole 160 KB; select() skips
// the key bits its bounds share.  Everything else -- tiles, EXCL / FILT steps, the filter, the rank counts -- is the k <= 64 form's.
// CEIL: the per-query score ceiling of the top-k (built without FILT only).
template <class Tile, bool EXCL, bool FILT, bool BIGK, bool CEIL = false>
__global__ __launch_bounds__((BIGK ? 1 : kRetWaves) * 64) void retrieve_sweep_kernel(Tile tile, RetArgs a) {
  constexpr int NW = BIGK ? 1 : kRetWaves;
  extern __shared__ uint32_t ret_lds[];
  const int lane = threadIdx.x & 63, c = lane & 31, h = lane >> 5;
  const int wave = BIGK ? 0 : threadIdx.x >> 6;
  const int64_t qt = (int64_t)blockIdx.x * NW + wave, q0 = 32 * qt;
  if (q0 >= a.nQ) return;                                       // (no workgroup barriers below: the waves are independent)
  const int s = blockIdx.y, S = a.S, k = a.k;
  const int64_t nT = (a.nC + 31) / 32, tb = nT * s / S, te = nT * (s + 1) / S;
  const int slots = BIGK ? ret_big_slots(k) : k + kRetCap;
  uint32_t* keys = ret_lds + (size_t)wave * slots * 64;         // [slot][query c]
  int32_t* ids = reinterpret_cast<int32_t*>(keys + slots * 32);
  const int64_t q = q0 + c;
  const bool qok = q < a.nQ;
  tile.load_queries(qt, c, h, a.nQ);

  const bool want_rank = a.part_rank != nullptr, want_topk = k > 0;
  int64_t p = -1, tp = -1;
  float sp = 0.f, sp_lo = 0.f;
  if (want_rank && qok) {
    p = positive_of(a, q);
    sp = a.sp[q];
    tp = p >= 0 ? p / 32 : -1;
    sp_lo = below(sp);
  }
  // exclusion cursor: e indexes query q's list, nxt is the excluded row it points at (INT32_MAX: none left in this split)
  int64_t e = 0, ee = 0;
  int32_t nxt = INT32_MAX;
  if (EXCL && qok) {
    const int64_t tot = a.excl_off[a.nQ];
    int64_t lo = a.excl_off[q], hi = a.excl_off[q + 1];
    lo = lo < 0 ? 0 : lo;
    hi = hi < tot ? hi : tot;
    hi = hi > lo ? hi : lo;
    ee = hi;
    const int64_t first = 32 * tb;                              // first entry >= the split's first row
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if ((int64_t)a.excl_rows[mid] < first) lo = mid + 1;
      else hi = mid;
    }
    e = lo;
    nxt = e < ee ? a.excl_rows[e] : INT32_MAX;
  }
  // attribute filter: the query's masks (hit0: an all-zero `any` is satisfied from the start) and the tile's tag words.  tg[j]
  // holds the words of rows 32 t + R j .. + R - 1 (R = 32 for W <= 2, else 16), word i of them in lane i
  const int W = FILT ? a.W : 0;
  uint32_t many[4] = {0u, 0u, 0u, 0u}, mall[4] = {0u, 0u, 0u, 0u};
  uint32_t hit0 = 1u, tg[2] = {0u, 0u};
  auto load_tags = [&](int64_t t) {                             // clamped: no word at or past tags[nC W] is read
    const int64_t last = a.nC * W - 1, i0 = 32 * t * W + lane, i1 = i0 + 16 * W;
    tg[0] = a.tags[i0 < last ? i0 : last];
    if (W > 2) tg[1] = a.tags[i1 < last ? i1 : last];
  };
  if (FILT) {
    if (qok) {
      uint32_t o = 0u;
#pragma unroll
      for (int w = 0; w < 4; ++w)
        if (w < W) {
          many[w] = a.q_any ? a.q_any[q * W + w] : 0u;
          mall[w] = a.q_all ? a.q_all[q * W + w] : 0u;
          o |= many[w];
        }
      hit0 = o == 0u ? 1u : 0u;
    }
    load_tags(tb);
  }
  float cl = INFINITY;                                          // CEIL: the query's ceiling (a lane past nQ keeps nothing)
  if constexpr (CEIL) cl = qok ? a.ceil[q] : -INFINITY;
  int rcnt = 0;
  float thr = -INFINITY;                                       // the query's k-th best so far (both lanes of a query agree)
  int cnt = 0;                                                  // filled slots of the query's region
  float top = -INFINITY;                                        // BIGK: no score this lane put into the region exceeds it

  // the k best of slots [0, cnt) of every query whose region holds more than k; region [0, k) afterwards
  auto select = [&]() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    const bool act = cnt > k;
    const int n = act ? cnt : 0;
    uint32_t K = 0;                                             // k-th largest key
    int btop = 31;
    if constexpr (BIGK) {
      // Every key of the region lies in [okey(thr), okey(top)], so the k-th largest shares the leading bits the two bounds
      // share: the search starts below them (the wave at its queries' highest differing bit; a bit above a query's own is
      // set already or fails its test, so K is what the full search finds).  Typically 9 or more of the 32 passes go.
      const uint32_t lo = okey(thr), hi = okey(fmaxf(top, __shfl_xor(top, 32)));
      const uint32_t d = hi >= lo ? lo ^ hi : 0xffffffffu;       // (hi < lo cannot be: the full search then)
      btop = !act ? -1 : d ? 31 - __clz(d) : -1;                 // the query's highest differing bit
      K = btop >= 0 ? hi & ~((2u << btop) - 1u) : hi;            // (2u << 31 wraps to 0: no bits kept)
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) {
        const int x = __shfl_xor(btop, o);
        btop = x > btop ? x : btop;
      }
    }
    for (int b = btop; b >= 0; --b) {
      const uint32_t tr = K | (1u << b);
      int ge = 0, i = h;
      if constexpr (BIGK)                                       // eight reads in flight: at most four waves share the CU's LDS
        for (; i + 14 < n; i += 16) {
          uint32_t x[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) x[j] = keys[(i + 2 * j) * 32 + c];
#pragma unroll
          for (int j = 0; j < 8; ++j) ge += x[j] >= tr ? 1 : 0;
        }
      for (; i < n; i += 2) ge += keys[i * 32 + c] >= tr ? 1 : 0;
      ge += __shfl_xor(ge, 32);
      if (ge >= k) K = tr;
    }
    int gt = 0, eq = 0;
    for (int i = h; i < n; i += 2) {
      const uint32_t x = keys[i * 32 + c];
      gt += x > K ? 1 : 0;
      eq += x == K ? 1 : 0;
    }
    gt += __shfl_xor(gt, 32);
    eq += __shfl_xor(eq, 32);
    const int need = k - gt;                                    // >= 1
    const bool tie = act && eq > need;
    int32_t I = kSentIdx;                                       // the need-th smallest index among key == K
    if (__any(tie)) {
      int32_t J = 0;
      for (int b = 30; b >= 0; --b) {
        const int32_t cand = J | (1 << b);
        int lt = 0;
        if (tie)
          for (int i = h; i < n; i += 2) lt += (keys[i * 32 + c] == K && ids[i * 32 + c] < cand) ? 1 : 0;
        lt += __shfl_xor(lt, 32);
        if (lt < need) J = cand;
      }
      if (tie) I = J;
    }
    if (act && h == 0) {                                        // in-place compaction, 8 slots read ahead of the writes
      int w = 0;
      for (int i0 = 0; i0 < n; i0 += 8) {
        uint32_t kk[8];
        int32_t ii[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          kk[j] = i0 + j < n ? keys[(i0 + j) * 32 + c] : 0u;
          ii[j] = i0 + j < n ? ids[(i0 + j) * 32 + c] : kSentIdx;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (i0 + j < n && (kk[j] > K || (kk[j] == K && ii[j] <= I))) {
            keys[w * 32 + c] = kk[j];
            ids[w * 32 + c] = ii[j];
            ++w;
          }
      }
    }
    if (act) {
      cnt = k;
      thr = okey_val(K);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  };

  typename Tile::Frag f;
  tile.load(tb, c, h, f);
  for (int64_t t = tb; t < te; ++t) {
    f32x16 acc;
    tile.score(f, t, c, h, acc);
    if (t + 1 < te) tile.load(t + 1, c, h, f);                 // next tile's operands fly while this one is filtered
    const uint32_t tg0 = tg[0], tg1 = tg[1];
    if (FILT && t + 1 < te) load_tags(t + 1);
    const int64_t r0 = 32 * t;
    if (r0 + 32 > a.nC) {                                       // ragged last tile: rows past the catalogue never count
#pragma unroll
      for (int r = 0; r < 16; ++r)
        if (r0 + rowmap(r, h) >= a.nC) acc[r] = -INFINITY;
    }
    if (EXCL) {                                                 // nxt >= r0 here: every entry below the tile is consumed
      const int64_t lim = r0 + 32;
      if (__any(nxt < lim)) {
        uint32_t xm = 0;                                        // bit j: row r0 + j is excluded for this lane's query
        do {                                                    // wave-uniform: ends with every lane past the tile
          if (nxt < lim) {
            xm |= 1u << (uint32_t)(nxt - r0);
            ++e;
            nxt = e < ee ? a.excl_rows[e] : INT32_MAX;
          }
        } while (__any(nxt < lim));
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if ((xm >> rowmap(r, h)) & 1u) acc[r] = -INFINITY;
      }
    }
    if (FILT) {                                                 // (W is wave-uniform: one of four straight-line copies)
      if (W == 1) filter_tile<1>(acc, h, tg0, tg1, many, mall, hit0);
      else if (W == 2) filter_tile<2>(acc, h, tg0, tg1, many, mall, hit0);
      else if (W == 3) filter_tile<3>(acc, h, tg0, tg1, many, mall, hit0);
      else filter_tile<4>(acc, h, tg0, tg1, many, mall, hit0);
    }
    if (want_rank) {
      if (!__any(t == tp)) {                                    // whole tile before (ties count) or after (they do not) p
        const float th = t < tp ? sp_lo : sp;
#pragma unroll
        for (int r = 0; r < 16; ++r) rcnt += acc[r] > th ? 1 : 0;
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int64_t row = r0 + rowmap(r, h);
          rcnt += (acc[r] > sp || (acc[r] == sp && row < p)) ? 1 : 0;
        }
      }
    }
    if constexpr (CEIL) {                                       // after the rank counts: the rank is among all eligible rows
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = acc[r] >= cl ? -INFINITY : acc[r];   // (a NaN ceiling: false, nothing goes)
    }
    if (want_topk) {
      float m = max3_asm(acc[0], acc[1], acc[2]);
#pragma unroll
      for (int r = 3; r < 15; r += 2) m = max3_asm(m, acc[r], acc[r + 1]);
      m = fmaxf(m, acc[15]);
      if (__any(m > thr)) {
        int mine = 0;
#pragma unroll
        for (int r = 0; r < 16; ++r) mine += acc[r] > thr ? 1 : 0;
        const int other = __shfl_xor(mine, 32);
        int w = cnt + (h ? other : 0);                          // half 0's candidates first, then half 1's
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (acc[r] > thr) {
            keys[w * 32 + c] = okey(acc[r]);
            ids[w * 32 + c] = (int32_t)(r0 + rowmap(r, h));
            ++w;
          }
        cnt += mine + other;
        if constexpr (BIGK) top = fmaxf(top, m);
        if (__any(cnt > slots - 32)) select();
      }
    }
  }
  if (want_topk) {
    if (__any(cnt > k)) select();
    if (qok) {
      uint32_t* pk = a.part_key + (q * S + s) * k;
      int32_t* pi = a.part_idx + (q * S + s) * k;
      for (int i = h; i < k; i += 2) {
        pk[i] = i < cnt ? keys[i * 32 + c] : 0u;
        pi[i] = i < cnt ? ids[i * 32 + c] : kSentIdx;
      }
    }
  }
  if (want_rank) {
    rcnt += __shfl_xor(rcnt, 32);
    if (qok && h == 0) a.part_rank[q * S + s] = rcnt;
  }
}

// ---- merge: one wave per query ------------------------------------------------------------------------------------------------
// (BIGK: k up to 512 -- the staging arrays hold kRetMaxK entries and a lane places every 64th of them)
template <int PER, bool BIGK>
__global__ __launch_bounds__(64) void retrieve_merge_kernel(RetArgs a) {
  constexpr int KM = BIGK ? kRetMaxK : kRetSmallK;
  const int lane = threadIdx.x;
  const int64_t q = blockIdx.x;
  const int S = a.S, k = a.k;
  if (a.rank && lane == 0) {
    const int64_t p = positive_of(a, q);
    int r = 0;
    for (int s = 0; s < S; ++s) r += a.part_rank[q * S + s];
    a.rank[q] = (p >= 0 && p < a.nC) ? r : -1;
  }
  if (k == 0) return;
  const int n = S * k;
  const uint32_t* pk = a.part_key + q * n;
  const int32_t* pi = a.part_idx + q * n;
  uint32_t kk[PER];
  int32_t ii[PER];
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int i = lane + 64 * j;
    kk[j] = i < n ? pk[i] : 0u;
    ii[j] = i < n ? pi[i] : kSentIdx;
    if (kk[j] == 0u) ii[j] = kSentIdx - i;                      // empty entries: distinct, after every real index
  }
  uint32_t K = 0;
  for (int b = 31; b >= 0; --b) {
    const uint32_t tr = K | (1u << b);
    int ge = 0;
#pragma unroll
    for (int j = 0; j < PER; ++j) ge += kk[j] >= tr ? 1 : 0;
    if (wave_sum(ge) >= k) K = tr;
  }
  int gt = 0, eq = 0;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    gt += kk[j] > K ? 1 : 0;
    eq += kk[j] == K ? 1 : 0;
  }
  gt = wave_sum(gt);
  eq = wave_sum(eq);
  const int need = k - gt;
  int32_t I = kSentIdx;
  if (eq > need) {                                              // wave-uniform
    int32_t J = 0;
    for (int b = 30; b >= 0; --b) {
      const int32_t cand = J | (1 << b);
      int lt = 0;
#pragma unroll
      for (int j = 0; j < PER; ++j) lt += (kk[j] == K && ii[j] < cand) ? 1 : 0;
      if (wave_sum(lt) < need) J = cand;
    }
    I = J;
  }
  __shared__ uint32_t sk[KM];
  __shared__ int32_t si[KM];
  int base = 0;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const bool sel = kk[j] > K || (kk[j] == K && ii[j] <= I);
    const uint64_t m = __ballot(sel);
    const int at = base + __popcll(m & ((1ull << lane) - 1));
    if (sel && at < KM) {                                       // (exactly k <= KM are selected)
      sk[at] = kk[j];
      si[at] = ii[j];
    }
    base += __popcll(m);
  }
  __syncthreads();
  if constexpr (!BIGK) {
    if (lane < k) {
      const uint32_t mk = sk[lane];
      const int32_t mi = si[lane];
      int pos = 0;
      for (int j = 0; j < k; ++j) pos += (sk[j] > mk || (sk[j] == mk && si[j] < mi)) ? 1 : 0;
      const bool empty = mk == 0u;
      a.vals[q * k + pos] = empty ? -INFINITY : okey_val(mk);
      a.idx[q * k + pos] = empty ? -1 : (int64_t)mi;
    }
  } else {
    for (int i = lane; i < k; i += 64) {
      const uint32_t mk = sk[i];
      const int32_t mi = si[i];
      int pos = 0;
      for (int j = 0; j < k; ++j) pos += (sk[j] > mk || (sk[j] == mk && si[j] < mi)) ? 1 : 0;
      const bool empty = mk == 0u;
      a.vals[q * k + pos] = empty ? -INFINITY : okey_val(mk);
      a.idx[q * k + pos] = empty ? -1 : (int64_t)mi;
    }
  }
}

// Most splits of a call.  k > 64: as many as keep S k within what the same catalogue's k = 64 call has (at most 32 x 64 = 2048
// entries), so that the merge's selection over 2048 entries holds and the workspace never exceeds the k = 64 one.
int ret_max_splits(int64_t nC, int k) {
  const int64_t nT = (nC + 31) / 32;
  const int64_t S = nT < kRetMaxSplits ? nT : kRetMaxSplits;
  if (k <= kRetSmallK) return (int)S;
  const int64_t cap = S * kRetSmallK / k;                       // S = 32: 2048 / k.  (k <= nC <= 32 nT, so never below 2)
  return (int)(cap > 1 ? cap : 1);
}

struct RetLayout {
  size_t sp, rank, key, idx, total;
};
RetLayout ret_layout(int64_t nQ, int64_t nC, int k) {
  const int64_t S = ret_max_splits(nC, k);
  RetLayout L;
  L.sp = 0;
  L.rank = L.sp + (size_t)rup(nQ * 4, 256);
  L.key = L.rank + (size_t)rup(nQ * S * 4, 256);
  L.idx = L.key + (size_t)rup(nQ * S * k * 4, 256);
  L.total = L.idx + (size_t)rup(nQ * S * k * 4, 256);
  return L;
}

bool ret_shape_ok(int64_t nQ, int64_t nC, int D, int k) {
  return nQ >= 1 && nC >= 1 && nC < (int64_t(1) << 31) && D >= 1 && D <= 256 && k >= 0 && k <= kRetMaxK && k <= nC;
}

struct RetFilt {              // attribute filter of a call (tags == NULL: none), or its score ceilings (ceil == NULL: none)
  const uint32_t* tags;
  int32_t W;
  const uint32_t* q_any;
  const uint32_t* q_all;
  const float* ceil;
};
constexpr RetFilt kNoFilt{nullptr, 0, nullptr, nullptr, nullptr};

template <class Tile>
int ret_launch(tt_ctx* ctx, const Tile& tile, int64_t nQ, int64_t nC, int32_t k, const void* positives,
               int32_t positives_i64, float* vals, int64_t* idx, int32_t* rank, const int64_t* excl_off,
               const int32_t* excl_rows, const RetFilt& flt, void* workspace, hipStream_t st) {
  const int64_t nT = tt_cdiv(nC, 32), nQt = tt_cdiv(nQ, 32);
  const int cap = ret_max_splits(nC, k);
  int64_t S;
  if (ctx->retrieve_splits > 0) {
    S = ctx->retrieve_splits;
  } else {                                                      // ~8 waves per CU, at least 16 tiles per split
    S = tt_cdiv(8 * (int64_t)ctx->num_cus, nQt);
    const int64_t lim = nT / 16 > 1 ? nT / 16 : 1;
    S = S < lim ? S : lim;
  }
  S = S < cap ? S : cap;
  S = S > 1 ? S : 1;
  const RetLayout lay = ret_layout(nQ, nC, k);
  char* ws = reinterpret_cast<char*>(workspace);
  RetArgs a{};
  a.nQ = nQ;
  a.nC = nC;
  a.k = k;
  a.S = (int)S;
  a.pos32 = positives && !positives_i64 ? reinterpret_cast<const int32_t*>(positives) : nullptr;
  a.pos64 = positives && positives_i64 ? reinterpret_cast<const int64_t*>(positives) : nullptr;
  a.sp = reinterpret_cast<float*>(ws + lay.sp);
  a.part_rank = positives ? reinterpret_cast<int32_t*>(ws + lay.rank) : nullptr;
  a.part_key = reinterpret_cast<uint32_t*>(ws + lay.key);
  a.part_idx = reinterpret_cast<int32_t*>(ws + lay.idx);
  a.vals = vals;
  a.idx = idx;
  a.rank = positives ? rank : nullptr;
  a.excl_off = excl_off;
  a.excl_rows = excl_rows;
  a.tags = flt.tags;
  a.q_any = flt.q_any;
  a.q_all = flt.q_all;
  a.W = flt.W;
  a.ceil = flt.ceil;
  if (positives) {
    retrieve_pos_kernel<Tile><<<(unsigned)nQt, 64, 0, st>>>(tile, a);
    TT_LAUNCH_CHECK();
  }
  const int64_t n = S * k;
  if (k > kRetSmallK) {                                         // large-k form: one wave per workgroup, up to the CU's whole LDS
    const size_t lds = (size_t)ret_big_slots(k) * 32 * 8;
    const dim3 grid((unsigned)nQt, (unsigned)S);
#define TT_RET_BIG(E, ...)                                                               \
  do {                                                                                   \
    TT_LDS_ONCE(kRetBigLds, &retrieve_sweep_kernel<Tile, E, __VA_ARGS__>);               \
    retrieve_sweep_kernel<Tile, E, __VA_ARGS__><<<grid, 64, lds, st>>>(tile, a);         \
  } while (0)
    if (flt.ceil) {
      if (excl_off) TT_RET_BIG(true, false, true, true);
      else TT_RET_BIG(false, false, true, true);
    } else if (flt.tags) {
      if (excl_off) TT_RET_BIG(true, true, true);
      else TT_RET_BIG(false, true, true);
    } else if (excl_off) {
      TT_RET_BIG(true, false, true);
    } else {
      TT_RET_BIG(false, false, true);
    }
#undef TT_RET_BIG
    TT_LAUNCH_CHECK();
    if (n <= 128) retrieve_merge_kernel<2, true><<<(unsigned)nQ, 64, 0, st>>>(a);
    else if (n <= 512) retrieve_merge_kernel<8, true><<<(unsigned)nQ, 64, 0, st>>>(a);
    else retrieve_merge_kernel<kRetMaxSplits, true><<<(unsigned)nQ, 64, 0, st>>>(a);
    TT_LAUNCH_CHECK();
    return TT_OK;
  }
  const size_t lds = (size_t)kRetWaves * (k + kRetCap) * 32 * 8;
  const dim3 grid((unsigned)tt_cdiv(nQt, kRetWaves), (unsigned)S);
  if (flt.ceil) {
    if (excl_off) retrieve_sweep_kernel<Tile, true, false, false, true><<<grid, kRetWaves * 64, lds, st>>>(tile, a);
    else retrieve_sweep_kernel<Tile, false, false, false, true><<<grid, kRetWaves * 64, lds, st>>>(tile, a);
  } else if (flt.tags) {
    if (excl_off) retrieve_sweep_kernel<Tile, true, true, false><<<grid, kRetWaves * 64, lds, st>>>(tile, a);
    else retrieve_sweep_kernel<Tile, false, true, false><<<grid, kRetWaves * 64, lds, st>>>(tile, a);
  } else if (excl_off) {
    retrieve_sweep_kernel<Tile, true, false, false><<<grid, kRetWaves * 64, lds, st>>>(tile, a);
  } else {
    retrieve_sweep_kernel<Tile, false, false, false><<<grid, kRetWaves * 64, lds, st>>>(tile, a);
  }
  TT_LAUNCH_CHECK();
  if (n <= 128) retrieve_merge_kernel<2, false><<<(unsigned)nQ, 64, 0, st>>>(a);
  else if (n <= 512) retrieve_merge_kernel<8, false><<<(unsigned)nQ, 64, 0, st>>>(a);
  else retrieve_merge_kernel<kRetMaxSplits, false><<<(unsigned)nQ, 64, 0, st>>>(a);
  TT_LAUNCH_CHECK();
  return TT_OK;
}

#define TT_RET_CHECK_COMMON(NAME)                                                                                                 \
  TT_CHECK_ARG(ctx != nullptr, NAME ": NULL context");                                                                           \
  TT_CHECK_ARG(ret_shape_ok(nQ, nC, D, k), NAME ": bad shape nQ=%lld nC=%lld D=%d k=%d (need nQ >= 1, 1 <= nC < 2^31, "         \
               "1 <= D <= 256, 0 <= k <= min(512, nC))", (long long)nQ, (long long)nC, D, k);                                    \
  TT_CHECK_ARG(k > 0 || positives != nullptr, NAME ": k = 0 asks for nothing (pass positives and rank, or k >= 1)");             \
  TT_CHECK_ARG(k == 0 || (vals != nullptr && idx != nullptr), NAME ": k = %d needs vals and idx", k);                           \
  TT_CHECK_ARG((positives == nullptr) == (rank == nullptr), NAME ": positives and rank go together (both or neither)");          \
  TT_CHECK_ARG(workspace != nullptr && tt_aligned(workspace, 16), NAME ": workspace NULL or not 16-byte aligned");            \
  TT_CHECK_ARG(workspace_bytes >= ret_layout(nQ, nC, k).total, NAME ": workspace of %zu bytes < %zu (tt_retrieve_workspace_bytes)", \
               workspace_bytes, ret_layout(nQ, nC, k).total)

#define TT_RET_CHECK_BF16(NAME)                                                                                                   \
  TT_CHECK_ARG(Q_packed && C_packed && tt_aligned(Q_packed, 16) && tt_aligned(C_packed, 16),                                     \
               NAME ": packed images NULL or not 16-byte aligned")

#define TT_RET_CHECK_EXCL(NAME)                                                                                                   \
  TT_CHECK_ARG(excl_offsets != nullptr && tt_aligned(excl_offsets, 8), NAME ": excl_offsets NULL or not 8-byte aligned");       \
  TT_CHECK_ARG(excl_rows != nullptr && tt_aligned(excl_rows, 4), NAME ": excl_rows NULL or not 4-byte aligned")

// filter entries: tags with 1 <= W <= 4 and at least one mask; the exclusion pair both given or both NULL
#define TT_RET_CHECK_FILT(NAME)                                                                                                   \
  TT_CHECK_ARG(W >= 1 && W <= 4, NAME ": W = %d tag words (need 1 <= W <= 4)", W);                                               \
  TT_CHECK_ARG(tags != nullptr && tt_aligned(tags, 16), NAME ": tags NULL or not 16-byte aligned");                              \
  TT_CHECK_ARG(q_any != nullptr || q_all != nullptr, NAME ": q_any and q_all both NULL (use the plain or the exclusion entry)"); \
  TT_CHECK_ARG(tt_aligned(q_any, 4) && tt_aligned(q_all, 4), NAME ": q_any or q_all not 4-byte aligned");                        \
  TT_CHECK_ARG((excl_offsets == nullptr) == (excl_rows == nullptr), NAME ": excl_offsets and excl_rows go together");            \
  TT_CHECK_ARG(tt_aligned(excl_offsets, 8) && tt_aligned(excl_rows, 4), NAME ": excl_offsets not 8- or excl_rows not 4-byte aligned")

// (arguments checked by the caller; excl_off == NULL launches the sweep without lists, flt.tags == NULL the one without filter)
int ret_bf16(tt_ctx* ctx, const void* Q_packed, int64_t nQ, const void* C_packed, int64_t nC, int32_t D, int32_t k,
             const void* positives, int32_t positives_i64, float* vals, int64_t* idx, int32_t* rank, const int64_t* excl_off,
             const int32_t* excl_rows, const RetFilt& flt, void* workspace, hipStream_t st) {
  const int Dp = padded_d(D);
#define TT_RET_BF16(KS)                                                                                                 \
  do {                                                                                                                  \
    TileBf16<KS> tile{};                                                                                                \
    tile.q_rows = view(Q_packed, nQ, D).rows;                                                                           \
    tile.c_rows = view(C_packed, nC, D).rows;                                                                           \
    return ret_launch(ctx, tile, nQ, nC, k, positives, positives_i64, vals, idx, rank, excl_off, excl_rows, flt, workspace, st); \
  } while (0)
  if (Dp == 32) TT_RET_BF16(2);
  if (Dp == 64) TT_RET_BF16(4);
  if (Dp == 128) TT_RET_BF16(8);
  TT_RET_BF16(16);
#undef TT_RET_BF16
}

int ret_f32(tt_ctx* ctx, const float* Q, int64_t nQ, const float* Cm, int64_t nC, int32_t D, float inv_t, int32_t k,
            const void* positives, int32_t positives_i64, float* vals, int64_t* idx, int32_t* rank, const int64_t* excl_off,
            const int32_t* excl_rows, const RetFilt& flt, void* workspace, hipStream_t st) {
  if (D % 4 == 0 && tt_aligned(Q, 16) && tt_aligned(Cm, 16)) {
    TileF32<true> tile{Q, Cm, nQ, nC, D, inv_t, nullptr};
    return ret_launch(ctx, tile, nQ, nC, k, positives, positives_i64, vals, idx, rank, excl_off, excl_rows, flt, workspace, st);
  }
  TileF32<false> tile{Q, Cm, nQ, nC, D, inv_t, nullptr};
  return ret_launch(ctx, tile, nQ, nC, k, positives, positives_i64, vals, idx, rank, excl_off, excl_rows, flt, workspace, st);
}

// tt_pair_scores_*: the pos launch with the caller's rows as positives and the caller's array as sp
template <int KS>
TileBf16<KS> pair_tile_bf16(const void* Q_packed, int64_t nQ, const void* C_packed, int64_t nC, int32_t D) {
  TileBf16<KS> tile{};
  tile.q_rows = view(Q_packed, nQ, D).rows;
  tile.c_rows = view(C_packed, nC, D).rows;
  return tile;
}

template <class Tile>
int pair_launch(const Tile& tile, int64_t nQ, int64_t nC, const void* rows, int32_t rows_i64, float* out, hipStream_t st) {
  RetArgs a{};
  a.nQ = nQ;
  a.nC = nC;
  a.pos32 = rows_i64 ? nullptr : reinterpret_cast<const int32_t*>(rows);
  a.pos64 = rows_i64 ? reinterpret_cast<const int64_t*>(rows) : nullptr;
  a.sp = out;
  retrieve_pos_kernel<Tile><<<(unsigned)tt_cdiv(nQ, 32), 64, 0, st>>>(tile, a);
  TT_LAUNCH_CHECK();
  return TT_OK;
}

}  // namespace

extern "C" {

size_t tt_retrieve_workspace_bytes(int64_t nQ, int64_t nC, int32_t D, int32_t k) {
  if (!ret_shape_ok(nQ, nC, D, k)) return 0;
  return ret_layout(nQ, nC, k).total;
}

int tt_retrieve_topk_bf16(tt_ctx* ctx, const void* Q_packed, int64_t nQ, const void* C_packed, int64_t nC, int32_t D, int32_t k,
                          const void* positives, int32_t positives_i64, float* vals, int64_t* idx, int32_t* rank, void* workspace,
                          size_t workspace_bytes, tt_stream stream) {
  TT_RET_CHECK_COMMON("tt_retrieve_topk_bf16");
  TT_RET_CHECK_BF16("tt_retrieve_topk_bf16");
  return ret_bf16(ctx, Q_packed, nQ, C_packed, nC, D, k, positives, positives_i64, vals, idx, rank, nullptr, nullptr, kNoFilt, workspace,
                  reinterpret_cast<hipStream_t>(stream));
}

int tt_retrieve_topk_f32(tt_ctx* ctx, const float* Q, int64_t nQ, const float* Cm, int64_t nC, int32_t D, float inv_t, int32_t k,
                         const void* positives, int32_t positives_i64, float* vals, int64_t* idx, int32_t* rank, void* workspace,
                         size_t workspace_bytes, tt_stream stream) {
  TT_RET_CHECK_COMMON("tt_retrieve_topk_f32");
  TT_CHECK_ARG(Q && Cm, "tt_retrieve_topk_f32: NULL embeddings");
  return ret_f32(ctx, Q, nQ, Cm, nC, D, inv_t, k, positives, positives_i64, vals, idx, rank, nullptr, nullptr, kNoFilt, workspace,
                 reinterpret_cast<hipStream_t>(stream));
}

int tt_excl_retrieve_topk_bf16(tt_ctx* ctx, const void* Q_packed, int64_t nQ, const void* C_packed, int64_t nC, int32_t D,
                               int32_t k, const void* positives, int32_t positives_i64, float* vals, int64_t* idx, int32_t* rank,
                               const int64_t* excl_offsets, const int32_t* excl_rows, void* workspace, size_t workspace_bytes,
                               tt_stream stream) {
  TT_RET_CHECK_COMMON("tt_excl_retrieve_topk_bf16");
  TT_RET_CHECK_BF16("tt_excl_retrieve_topk_bf16");
  TT_RET_CHECK_EXCL("tt_excl_retrieve_topk_bf16");
  return ret_bf16(ctx, Q_packed, nQ, C_packed, nC, D, k, positives, positives_i64, vals, idx, rank, excl_offsets, excl_rows,
                  kNoFilt, workspace, reinterpret_cast<hipStream_t>(stream));
}

int tt_excl_retrieve_topk_f32(tt_ctx* ctx, const float* Q, int64_t nQ, const float* Cm, int64_t nC, int32_t D, float inv_t,
                              int32_t k, const void* positives, int32_t positives_i64, float* vals, int64_t* idx, int32_t* rank,
                              const int64_t* excl_offsets, const int32_t* excl_rows, void* workspace, size_t workspace_bytes,
                              tt_stream stream) {
  TT_RET_CHECK_COMMON("tt_excl_retrieve_topk_f32");
  TT_CHECK_ARG(Q && Cm, "tt_excl_retrieve_topk_f32: NULL embeddings");
  TT_RET_CHECK_EXCL("tt_excl_retrieve_topk_f32");
  return ret_f32(ctx, Q, nQ, Cm, nC, D, inv_t, k, positives, positives_i64, vals, idx, rank, excl_offsets, excl_rows, kNoFilt,
                 workspace, reinterpret_cast<hipStream_t>(stream));
}

int tt_filt_retrieve_topk_bf16(tt_ctx* ctx, const void* Q_packed, int64_t nQ, const void* C_packed, int64_t nC, int32_t D,
                               int32_t k, const void* positives, int32_t positives_i64, float* vals, int64_t* idx, int32_t* rank,
                               const int64_t* excl_offsets, const int32_t* excl_rows, const uint32_t* tags, int32_t W,
                               const uint32_t* q_any, const uint32_t* q_all, void* workspace, size_t workspace_bytes,
                               tt_stream stream) {
  TT_RET_CHECK_COMMON("tt_filt_retrieve_topk_bf16");
  TT_RET_CHECK_BF16("tt_filt_retrieve_topk_bf16");
  TT_RET_CHECK_FILT("tt_filt_retrieve_topk_bf16");
  return ret_bf16(ctx, Q_packed, nQ, C_packed, nC, D, k, positives, positives_i64, vals, idx, rank, excl_offsets, excl_rows,
                  RetFilt{tags, W, q_any, q_all, nullptr}, workspace, reinterpret_cast<hipStream_t>(stream));
}

int tt_filt_retrieve_topk_f32(tt_ctx* ctx, const float* Q, int64_t nQ, const float* Cm, int64_t nC, int32_t D, float inv_t,
                              int32_t k, const void* positives, int32_t positives_i64, float* vals, int64_t* idx, int32_t* rank,
                              const int64_t* excl_offsets, const int32_t* excl_rows, const uint32_t* tags, int32_t W,
                              const uint32_t* q_any, const uint32_t* q_all, void* workspace, size_t workspace_bytes,
                              tt_stream stream) {
  TT_RET_CHECK_COMMON("tt_filt_retrieve_topk_f32");
  TT_CHECK_ARG(Q && Cm, "tt_filt_retrieve_topk_f32: NULL embeddings");
  TT_RET_CHECK_FILT("tt_filt_retrieve_topk_f32");
  return ret_f32(ctx, Q, nQ, Cm, nC, D, inv_t, k, positives, positives_i64, vals, idx, rank, excl_offsets, excl_rows,
                 RetFilt{tags, W, q_any, q_all, nullptr}, workspace, reinterpret_cast<hipStream_t>(stream));
}

// ceiling entries: the exclusion pair both given or both NULL, the ceilings required
#define TT_RET_CHECK_CEIL(NAME)                                                                                                   \
  TT_CHECK_ARG(ceil != nullptr && tt_aligned(ceil, 4), NAME ": ceil NULL or not 4-byte aligned");                                \
  TT_CHECK_ARG((excl_offsets == nullptr) == (excl_rows == nullptr), NAME ": excl_offsets and excl_rows go together");            \
  TT_CHECK_ARG(tt_aligned(excl_offsets, 8) && tt_aligned(excl_rows, 4), NAME ": excl_offsets not 8- or excl_rows not 4-byte aligned")

int tt_ceil_retrieve_topk_bf16(tt_ctx* ctx, const void* Q_packed, int64_t nQ, const void* C_packed, int64_t nC, int32_t D,
                               int32_t k, const void* positives, int32_t positives_i64, float* vals, int64_t* idx, int32_t* rank,
                               const int64_t* excl_offsets, const int32_t* excl_rows, const float* ceil, void* workspace,
                               size_t workspace_bytes, tt_stream stream) {
  TT_RET_CHECK_COMMON("tt_ceil_retrieve_topk_bf16");
  TT_RET_CHECK_BF16("tt_ceil_retrieve_topk_bf16");
  TT_RET_CHECK_CEIL("tt_ceil_retrieve_topk_bf16");
  return ret_bf16(ctx, Q_packed, nQ, C_packed, nC, D, k, positives, positives_i64, vals, idx, rank, excl_offsets, excl_rows,
                  RetFilt{nullptr, 0, nullptr, nullptr, ceil}, workspace, reinterpret_cast<hipStream_t>(stream));
}

int tt_ceil_retrieve_topk_f32(tt_ctx* ctx, const float* Q, int64_t nQ, const float* Cm, int64_t nC, int32_t D, float inv_t,
                              int32_t k, const void* positives, int32_t positives_i64, float* vals, int64_t* idx, int32_t* rank,
                              const int64_t* excl_offsets, const int32_t* excl_rows, const float* ceil, void* workspace,
                              size_t workspace_bytes, tt_stream stream) {
  TT_RET_CHECK_COMMON("tt_ceil_retrieve_topk_f32");
  TT_CHECK_ARG(Q && Cm, "tt_ceil_retrieve_topk_f32: NULL embeddings");
  TT_RET_CHECK_CEIL("tt_ceil_retrieve_topk_f32");
  return ret_f32(ctx, Q, nQ, Cm, nC, D, inv_t, k, positives, positives_i64, vals, idx, rank, excl_offsets, excl_rows,
                 RetFilt{nullptr, 0, nullptr, nullptr, ceil}, workspace, reinterpret_cast<hipStream_t>(stream));
}

#define TT_PAIR_CHECK(NAME)                                                                                                       \
  TT_CHECK_ARG(ctx != nullptr, NAME ": NULL context");                                                                           \
  TT_CHECK_ARG(ret_shape_ok(nQ, nC, D, 0), NAME ": bad shape nQ=%lld nC=%lld D=%d (need nQ >= 1, 1 <= nC < 2^31, "               \
               "1 <= D <= 256)", (long long)nQ, (long long)nC, D);                                                               \
  TT_CHECK_ARG(rows != nullptr && tt_aligned(rows, rows_i64 ? 8 : 4), NAME ": rows NULL or misaligned");                         \
  TT_CHECK_ARG(out != nullptr && tt_aligned(out, 4), NAME ": out NULL or not 4-byte aligned")

int tt_pair_scores_bf16(tt_ctx* ctx, const void* Q_packed, int64_t nQ, const void* C_packed, int64_t nC, int32_t D,
                        const void* rows, int32_t rows_i64, float* out, tt_stream stream) {
  TT_PAIR_CHECK("tt_pair_scores_bf16");
  TT_RET_CHECK_BF16("tt_pair_scores_bf16");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int Dp = padded_d(D);
  if (Dp == 32) return pair_launch(pair_tile_bf16<2>(Q_packed, nQ, C_packed, nC, D), nQ, nC, rows, rows_i64, out, st);
  if (Dp == 64) return pair_launch(pair_tile_bf16<4>(Q_packed, nQ, C_packed, nC, D), nQ, nC, rows, rows_i64, out, st);
  if (Dp == 128) return pair_launch(pair_tile_bf16<8>(Q_packed, nQ, C_packed, nC, D), nQ, nC, rows, rows_i64, out, st);
  return pair_launch(pair_tile_bf16<16>(Q_packed, nQ, C_packed, nC, D), nQ, nC, rows, rows_i64, out, st);
}

int tt_pair_scores_f32(tt_ctx* ctx, const float* Q, int64_t nQ, const float* Cm, int64_t nC, int32_t D, float inv_t,
                       const void* rows, int32_t rows_i64, float* out, tt_stream stream) {
  TT_PAIR_CHECK("tt_pair_scores_f32");
  TT_CHECK_ARG(Q && Cm, "tt_pair_scores_f32: NULL embeddings");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (D % 4 == 0 && tt_aligned(Q, 16) && tt_aligned(Cm, 16))                    // the sweep's own choice of tile
    return pair_launch(TileF32<true>{Q, Cm, nQ, nC, D, inv_t, nullptr}, nQ, nC, rows, rows_i64, out, st);
  return pair_launch(TileF32<false>{Q, Cm, nQ, nC, D, inv_t, nullptr}, nQ, nC, rows, rows_i64, out, st);
}

}  // extern "C"
