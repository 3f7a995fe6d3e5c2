// The duplicate-row plans of the embedding gradient on gfx950: which slots of the batch hit the same table row.  Two builders
// -- an LSD radix sort of (row, slot) pairs with segment heads, and a keyed sort that gives every (side, key) one workgroup
// and sorts its rows in LDS -- both ending in (sorted_src, unique_rows, seg_offsets, n_unique).  The keyed plan's compaction
// (tt_riders.h) also fills the long-row lists of the reduction's workspace (tt_grad_ws.h).
#include "tt_common.h"
#include "tt_deferred.h"
#include "tt_embed_slots.h"
#include "tt_grad_ws.h"

namespace {

// ------------------------------------------------------------------------------------------------
// Dedup plan: LSD radix sort (BITS per pass) of (row, slot) pairs.
//   hist    : per-tile digit histogram        -> hist[digit * nblk + tile]
//   scan    : exclusive scan of that array (one workgroup)
//   scatter : stable ranking by wave ballots (no sorting network, no atomics on the output side)
// ------------------------------------------------------------------------------------------------
constexpr int kSortTile = 4096;                 // elements per workgroup
constexpr int kWaveSpan = kSortTile / 4;        // contiguous elements per wave

template <int BITS>
__global__ __launch_bounds__(kThreads) void sort_hist_kernel(const uint32_t* __restrict__ keys, uint32_t M, int shift,
                                                            uint32_t* __restrict__ hist, uint32_t nblk) {
  constexpr uint32_t R = 1u << BITS;
  __shared__ uint32_t h[R];
  for (uint32_t d = threadIdx.x; d < R; d += kThreads) h[d] = 0;
  __syncthreads();
  const uint32_t base = blockIdx.x * kSortTile;
  for (uint32_t i = threadIdx.x; i < kSortTile; i += kThreads) {
    const uint32_t idx = base + i;
    if (idx < M) atomicAdd(&h[(keys[idx] >> shift) & (R - 1)], 1u);
  }
  __syncthreads();
  for (uint32_t d = threadIdx.x; d < R; d += kThreads) hist[blockIdx.x * R + d] = h[d];
}

// per digit: exclusive scan over the tiles (hist[tile][digit], in place) and the digit total.
// grid = R/64 workgroups; thread = (digit, one of kScanSeg tile segments).  Round 4: 16 segments (1024 threads) instead of 4 -- at
// configs[4] (608 tiles) a thread walked 152 tiles twice and the launch took 42 us on 32 CUs; now 38 tiles: the same sums in the same
// order per segment, segment totals added in segment order (integers: any order gives the same bits)
constexpr int kScanSeg = 16;
template <int BITS>
__global__ __launch_bounds__(64 * kScanSeg) void sort_colscan_kernel(uint32_t* __restrict__ hist, uint32_t nblk, uint32_t* __restrict__ total) {
  constexpr uint32_t R = 1u << BITS;
  __shared__ uint32_t sh[kScanSeg][64];
  const uint32_t d = blockIdx.x * 64 + (threadIdx.x & 63), seg = threadIdx.x >> 6;
  const uint32_t per = (nblk + kScanSeg - 1) / kScanSeg;
  const uint32_t lo = seg * per < nblk ? seg * per : nblk;
  const uint32_t hi = lo + per < nblk ? lo + per : nblk;
  uint32_t s = 0;
  for (uint32_t b = lo; b < hi; ++b) s += hist[b * R + d];
  sh[seg][threadIdx.x & 63] = s;
  __syncthreads();
  uint32_t run = 0;
  for (uint32_t g = 0; g < seg; ++g) run += sh[g][threadIdx.x & 63];
  for (uint32_t b = lo; b < hi; ++b) {
    const uint32_t t = hist[b * R + d];
    hist[b * R + d] = run;
    run += t;
  }
  if (seg == kScanSeg - 1) total[d] = run;
}

template <int BITS>
__global__ __launch_bounds__(kThreads) void sort_scatter_kernel(const uint32_t* __restrict__ keys_in,
                                                               const uint32_t* __restrict__ vals_in,
                                                               uint32_t* __restrict__ keys_out,
                                                               uint32_t* __restrict__ vals_out, uint32_t M, int shift,
                                                               const uint32_t* __restrict__ hist_scanned,
                                                               const uint32_t* __restrict__ total) {
  constexpr uint32_t R = 1u << BITS;
  constexpr uint32_t PER = R / kThreads;              // digits per thread in the digit-base scan
  __shared__ uint32_t woff_s[4][R];
  __shared__ uint32_t dbase[R];
  __shared__ uint32_t wsum[4];
  volatile uint32_t(*woff)[R] = woff_s;
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (uint32_t d = tid; d < 4 * R; d += kThreads) (&woff_s[0][0])[d] = 0;
  __syncthreads();
  const uint32_t wbase = blockIdx.x * kSortTile + wave * kWaveSpan;
  // phase 1: per-wave digit counts
  for (uint32_t it = 0; it < kWaveSpan / 64; ++it) {
    const uint32_t idx = wbase + it * 64 + lane;
    if (idx < M) atomicAdd(&woff_s[wave][(keys_in[idx] >> shift) & (R - 1)], 1u);
  }
  __syncthreads();
  // digit bases: exclusive scan of the digit totals (R <= 2048 values) inside the workgroup
  {
    uint32_t loc[PER], c = 0;
#pragma unroll
    for (uint32_t j = 0; j < PER; ++j) { loc[j] = total[tid * PER + j]; c += loc[j]; }
    uint32_t x = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t y = __shfl_up(x, o);
      if (lane >= (uint32_t)o) x += y;
    }
    if (lane == 63) wsum[wave] = x;
    __syncthreads();
    uint32_t run = x - c;
    for (uint32_t w = 0; w < wave; ++w) run += wsum[w];
#pragma unroll
    for (uint32_t j = 0; j < PER; ++j) { dbase[tid * PER + j] = run; run += loc[j]; }
  }
  __syncthreads();
  // phase 2: counts -> starting output offset of (wave, digit)
  for (uint32_t d = tid; d < R; d += kThreads) {
    uint32_t base = dbase[d] + hist_scanned[blockIdx.x * R + d];
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const uint32_t c = woff_s[w][d];
      woff_s[w][d] = base;
      base += c;
    }
  }
  __syncthreads();
  // phase 3: stable rank inside each 64-element batch from ballots, running offsets in LDS
  const uint64_t lt_mask = (1ull << lane) - 1ull;
  for (uint32_t it = 0; it < kWaveSpan / 64; ++it) {
    const uint32_t idx = wbase + it * 64 + lane;
    const bool valid = idx < M;
    const uint32_t key = valid ? keys_in[idx] : 0u;
    const uint32_t val = valid ? (vals_in ? vals_in[idx] : idx) : 0u;
    const uint32_t d = (key >> shift) & (R - 1);
    uint64_t peers = __ballot(valid);
#pragma unroll
    for (int bit = 0; bit < BITS; ++bit) {
      const bool one = (d >> bit) & 1u;
      const uint64_t bm = __ballot(one);
      peers &= one ? bm : ~bm;
    }
    uint32_t pos = 0;
    const uint32_t rank = (uint32_t)__popcll(peers & lt_mask);
    if (valid) pos = woff[wave][d] + rank;
    __builtin_amdgcn_wave_barrier();
    if (valid && rank == 0) woff[wave][d] = pos + (uint32_t)__popcll(peers);
    __builtin_amdgcn_wave_barrier();
    if (valid) {
      keys_out[pos] = key;
      vals_out[pos] = val;
    }
  }
}

// stable merge of G ascending runs of length C (the owner's received buckets: every source sends its distinct rows in
// ascending order, pads = the largest value at the end): the position of an element is its own index plus, per other
// run, the number of elements that sort before it (<= for lower runs, < for higher ones) -- binary searches in L2,
// no radix passes (80 -> 30 us for 98 k ids; at G = 1 the run is already the answer)
__global__ __launch_bounds__(kThreads) void merge_runs_kernel(const int32_t* __restrict__ rows, uint32_t G, uint32_t C,
                                                             uint32_t* __restrict__ keys_out, int32_t* __restrict__ sorted_src) {
  const uint32_t total = G * C;
  for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
    const uint32_t r = e / C, i = e - r * C;
    const uint32_t x = (uint32_t)rows[e];
    uint32_t pos = i;
    for (uint32_t q = 0; q < G; ++q) {
      if (q == r) continue;
      const int32_t* run = rows + (size_t)q * C;
      uint32_t lo = 0, hi = C;                          // first index whose value is > x (q < r) or >= x (q > r)
      while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        const uint32_t v = (uint32_t)run[mid];
        const bool before = q < r ? v <= x : v < x;
        if (before) lo = mid + 1; else hi = mid;
      }
      pos += lo;
    }
    keys_out[pos] = x;
    sorted_src[pos] = (int32_t)e;
  }
}

// segment heads -------------------------------------------------------------------------------
__device__ __forceinline__ bool is_head(const uint32_t* keys, uint32_t i) { return i == 0 || keys[i] != keys[i - 1]; }

__global__ __launch_bounds__(kThreads) void head_count_kernel(const uint32_t* __restrict__ keys, uint32_t M,
                                                             uint32_t* __restrict__ blockcount) {
  __shared__ uint32_t cnt;
  if (threadIdx.x == 0) cnt = 0;
  __syncthreads();
  const uint32_t base = blockIdx.x * kSortTile;
  uint32_t c = 0;
  for (uint32_t i = threadIdx.x; i < kSortTile; i += kThreads) {
    const uint32_t idx = base + i;
    if (idx < M && is_head(keys, idx)) ++c;
  }
  atomicAdd(&cnt, c);
  __syncthreads();
  if (threadIdx.x == 0) blockcount[blockIdx.x] = cnt;
}

__global__ __launch_bounds__(kThreads) void head_write_kernel(const uint32_t* __restrict__ keys, uint32_t M,
                                                             const uint32_t* __restrict__ blockcount,
                                                             int32_t* __restrict__ n_unique,
                                                             int32_t* __restrict__ unique_rows,
                                                             int32_t* __restrict__ seg_offsets, uint32_t drop_from = 0xFFFFFFFFu) {
  __shared__ uint32_t wsum[4], wbefore[4], wall[4];
  constexpr uint32_t PER = kSortTile / kThreads;   // 16 contiguous elements per thread
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t lo = blockIdx.x * kSortTile + tid * PER;
  uint32_t flags = 0, c = 0;
#pragma unroll
  for (uint32_t j = 0; j < PER; ++j) {
    const uint32_t idx = lo + j;
    if (idx < M && is_head(keys, idx)) { flags |= 1u << j; ++c; }
  }
  uint32_t x = c;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t y = __shfl_up(x, o);
    if (lane >= (uint32_t)o) x += y;
  }
  if (lane == 63) wsum[wave] = x;
  // offset of this tile = sum of the head counts of the tiles before it (block 0 also forms the total)
  uint32_t before = 0, all = 0;
  const uint32_t nblk = gridDim.x;
  for (uint32_t b = tid; b < nblk; b += kThreads) {
    const uint32_t v = blockcount[b];
    all += v;
    if (b < blockIdx.x) before += v;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { before += __shfl_xor(before, o); all += __shfl_xor(all, o); }
  if (lane == 0) { wbefore[wave] = before; wall[wave] = all; }
  __syncthreads();
  before = wbefore[0] + wbefore[1] + wbefore[2] + wbefore[3];
  all = wall[0] + wall[1] + wall[2] + wall[3];
  uint32_t u = before + x - c;
  for (uint32_t w = 0; w < wave; ++w) u += wsum[w];
#pragma unroll
  for (uint32_t j = 0; j < PER; ++j) {
    if (flags & (1u << j)) {
      unique_rows[u] = (int32_t)keys[lo + j];
      seg_offsets[u] = (int32_t)(lo + j);
      ++u;
    }
  }
  if (blockIdx.x == 0 && tid == 0) {
    // drop_from: the largest key is a pad value (>= drop_from) that the plan's consumers must not see as a row: it stays
    // in unique_rows / seg_offsets (seg_offsets[n_unique] is still the end of the last real row) but is not counted
    n_unique[0] = (int32_t)(all - ((M > 0 && keys[M - 1] >= drop_from) ? 1u : 0u));
    seg_offsets[all] = (int32_t)M;
  }
}

// chained aggregates (tt_common.h: tt_ctx::chain): a workgroup's value with the ready bit; a reader polls until the bit shows.
// All workgroups of these grids are resident at once (<= 2048 of 256 threads) and dispatched in index order, so a predecessor is
// always running or done; the poll is bounded all the same -- a buffer left dirty by an aborted launch must not hang the device
// (`stuck` then leaves an EMPTY plan, n_unique = 0: wrong results, but no consumer indexes anything with it).
// (relaxed agent-scope atomics: the word itself is all that travels, and nothing else has to become visible with it -- an acquire
//  load per poll invalidates the XCD's caches every time: 72 us for 608 tiles against 24 us for the two launches it replaced)
__device__ __forceinline__ void chain_publish(uint32_t* slot, uint32_t v) {
  __hip_atomic_store(slot, v | kChainReady, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint32_t chain_wait(const uint32_t* slot, bool& stuck, int max_spin) {
  for (int spin = 0; spin < max_spin; ++spin) {
    const uint32_t v = __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (v & kChainReady) return v & ~kChainReady;
    __builtin_amdgcn_s_sleep(1);
  }
  stuck = true;
  return 0u;
}

// head_count_kernel + head_write_kernel as ONE launch: a tile publishes its head count in chain[1 + tile] and adds up the tiles before
// it; the last tile also writes the totals.  chain[0] counts the tiles that are through with their reads: the last one clears.
__global__ __launch_bounds__(kThreads) void head_chained_kernel(const uint32_t* __restrict__ keys, uint32_t M, uint32_t* __restrict__ chain,
                                                               int32_t* __restrict__ n_unique, int32_t* __restrict__ unique_rows,
                                                               int32_t* __restrict__ seg_offsets, uint32_t drop_from, uint32_t* __restrict__ dev_err,
                                                               int max_spin) {
  __shared__ uint32_t wsum[4], wbefore[4];
  __shared__ uint32_t s_stuck, s_last;
  constexpr uint32_t PER = kSortTile / kThreads;
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nblk = gridDim.x;
  const uint32_t lo = blockIdx.x * kSortTile + tid * PER;
  if (tid == 0) s_stuck = 0;
  uint32_t flags = 0, c = 0;
#pragma unroll
  for (uint32_t j = 0; j < PER; ++j) {
    const uint32_t idx = lo + j;
    if (idx < M && is_head(keys, idx)) { flags |= 1u << j; ++c; }
  }
  uint32_t x = c;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t y = __shfl_up(x, o);
    if (lane >= (uint32_t)o) x += y;
  }
  if (lane == 63) wsum[wave] = x;
  __syncthreads();
  const uint32_t total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
  if (tid == 0) chain_publish(chain + 1 + blockIdx.x, total);
  uint32_t before = 0;
  bool stuck = false;
  for (uint32_t b = tid; b < blockIdx.x; b += kThreads) before += chain_wait(chain + 1 + b, stuck, max_spin);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) before += __shfl_xor(before, o);
  if (lane == 0) wbefore[wave] = before;
  if (stuck) {
    s_stuck = 1;
    // ANY tile whose wait expired raises the context's sticky device error word: the last tile only knows about
    // itself, and a plan with a middle tile's prefix missing is corrupt, not empty.  tt_ctx_check_device_errors reports it, clears
    // it and zeroes the chain buffers (a half-run launch leaves ready bits behind)
    atomicOr(dev_err, TT_DEVERR_CHAIN_TIMEOUT);
  }
  __syncthreads();
  before = wbefore[0] + wbefore[1] + wbefore[2] + wbefore[3];
  uint32_t u = before + x - c;
  for (uint32_t w = 0; w < wave; ++w) u += wsum[w];
#pragma unroll
  for (uint32_t j = 0; j < PER; ++j) {
    if (flags & (1u << j)) {
      unique_rows[u] = (int32_t)keys[lo + j];
      seg_offsets[u] = (int32_t)(lo + j);
      ++u;
    }
  }
  if (blockIdx.x == nblk - 1 && tid == 0) {              // (drop_from: see head_write_kernel)
    const uint32_t all = before + total;
    n_unique[0] = s_stuck ? 0 : (int32_t)(all - ((M > 0 && keys[M - 1] >= drop_from) ? 1u : 0u));   // (stuck: an empty plan reads nothing)
    seg_offsets[all] = (int32_t)M;
  }
  // everybody's reads of the chain are done once every tile has been here: the last one leaves the buffer all-zero
  if (tid == 0) s_last = atomicAdd(chain, 1u) == nblk - 1 ? 1u : 0u;
  __syncthreads();
  if (s_last) {
    for (uint32_t b = tid; b < nblk; b += kThreads) chain[1 + b] = 0u;
    if (tid == 0) chain[0] = 0u;
  }
}

// ------------------------------------------------------------------------------------------------
// Keyed dedup plan: one 1024-thread workgroup per (side, key) sorts that key's B slot rows in LDS.
// ------------------------------------------------------------------------------------------------
constexpr int kKeyedB = 8192;          // max ids per key (LDS: 2 x 32 KB keys + 2 x 16 KB values + 16 KB histograms + 32 KB lane sets)
constexpr int kKeyedThreads = 1024;

static_assert(kKeyedThreads == kRiderThreads, "the statistics riders run in the sort's workgroups");
constexpr int kKeyedMaxParts = 8;
// (KeyedArgs; PlanLong, the long-row list the compaction builds for the gradient reduction: tt_riders.h)
// (bf_wg > 0: the FIRST bf_wg workgroups -- dispatched first, so they start at once even when the sort fills every CU -- finish the
// towers' BatchNorm statistics, one tower each, and return: tt_riders.h.  They use the head of `keys` for their 12 KB of triples.  The
// sort's workgroups follow; bf_wg == 0 is the kernel as it was.)

__global__ __launch_bounds__(kKeyedThreads) void keyed_sort_kernel(KeyedArgs a, const int32_t* __restrict__ rows,
                                                                  int32_t* __restrict__ sorted_src, int32_t* __restrict__ uniq_stage,
                                                                  int32_t* __restrict__ seg_stage, int32_t* __restrict__ ucount,
                                                                  int32_t* __restrict__ ubase, int32_t* __restrict__ uend, bool key_major,
                                                                  int32_t* __restrict__ long_counters, BnFinishRiders bf, int bf_wg) {
  __shared__ uint32_t keys[2][kKeyedB];
  __shared__ uint16_t vals[2][kKeyedB];
  __shared__ uint32_t whist[16][256];
  __shared__ unsigned long long peers_mask[16][256];   // lane sets per (wave, digit); all zero between batches
  __shared__ uint32_t red[32];
  static_assert(sizeof(Wf) * 16 * 64 <= sizeof(keys), "the statistics rider's triples live in keys");
  if ((int)blockIdx.x < bf_wg) {
    bn_finish_body(bf.r[blockIdx.x], reinterpret_cast<Wf(*)[64]>(&keys[0][0]));
    return;
  }
  const int wg = (int)blockIdx.x - bf_wg;                // the sort's own workgroup index
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // `parts` workgroups per key: every one loads the key's B rows and builds the same bucket histogram, then scatters, ranks and
  // writes only the buckets of ITS share of the key's row range (whole rows: a row never straddles two shares) -- the sorted
  // positions follow from the common prefix, so there is nothing to merge.  Every workgroup of a key reaches the same decision
  // about the LSD fallback (same histogram); share 0 then sorts the whole key alone.
  const int P = a.parts, ki = wg / P, part = wg % P, B = a.B;
  if (long_counters && wg == 0 && tid < 2) long_counters[tid] = 0;      // the compaction (next launch) counts from zero
  for (int d = tid; d < 16 * 256; d += kKeyedThreads) (&peers_mask[0][0])[d] = 0ull;
  int side = 0;
#pragma unroll
  for (int i = 1; i < TT_MAX_SIDES; ++i)
    if (i < a.n_sides && ki >= a.key_base[i]) side = i;
  const int K = a.K[side], k = ki - a.key_base[side], sbase = a.side_base[side];
  // load this key's ids (stride K in the slot-major array) and find the row range
  uint32_t lo = 0xFFFFFFFFu, hi = 0;
  {
    // stride-K gather (one id per 4*K-byte step): all loads of a thread are issued before the first LDS store
    // (every key of a side reads the same 4*K-byte-strided lines, one dword of each: the workgroups start at different
    // samples so that they do not all ask for the same line at the same moment: 10.5 -> 7.9 us for the 32 notice keys)
    constexpr int PERL = kKeyedB / kKeyedThreads;
    uint32_t r[PERL];
    // key_major: the rows arrive as [key][sample] (tt_batch_ingest) -- this key's B rows are one contiguous run: 6.5 -> 2 us
    const int rot = key_major ? 0 : (int)(((unsigned)k * 264u) % (unsigned)B);
#pragma unroll
    for (int j = 0; j < PERL; ++j) {
      int b = tid + j * kKeyedThreads + rot;
      b = b >= B ? b - B : b;
      r[j] = tid + j * kKeyedThreads < B ? (uint32_t)rows[key_major ? sbase + k * B + b : sbase + b * K + k] : 0u;
    }
#pragma unroll
    for (int j = 0; j < PERL; ++j) {
      int b = tid + j * kKeyedThreads + rot;
      b = b >= B ? b - B : b;
      if (tid + j * kKeyedThreads < B) {
        keys[0][b] = r[j];
        vals[0][b] = (uint16_t)b;
        lo = r[j] < lo ? r[j] : lo;
        hi = r[j] > hi ? r[j] : hi;
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t l2 = __shfl_xor(lo, o), h2 = __shfl_xor(hi, o);
    lo = l2 < lo ? l2 : lo;
    hi = h2 > hi ? h2 : hi;
  }
  if (lane == 0) { red[wave] = lo; red[16 + wave] = hi; }
  __syncthreads();
  lo = red[0]; hi = red[16];
  for (int w = 1; w < 16; ++w) { lo = red[w] < lo ? red[w] : lo; hi = red[16 + w] > hi ? red[16 + w] : hi; }
  int bits = 0;
  while (bits < 32 && ((hi - lo) >> bits) != 0) ++bits;
  const int passes = (bits + 7) / 8;
  // digits of equal width (a 9-bit range as 5 + 4 bits, not 8 + 1: a 1-bit digit sends all 64 lanes of a batch
  // to two LDS words and that pass ran 2x longer than an 8-bit one)
  const int dbits = passes > 0 ? (bits + passes - 1) / passes : 8;
  const uint32_t dmask = (1u << dbits) - 1u;
  // every wave owns a contiguous span of the array: stable LSD passes with per-wave digit histograms
  const int span = (B + 15) / 16;
  const int wlo = wave * span < B ? wave * span : B, whi = wlo + span < B ? wlo + span : B;
  const uint64_t lt_mask = (1ull << lane) - 1ull;
  int cur = 0;
  volatile uint32_t(*wh)[256] = whist;
  volatile unsigned long long(*pm)[256] = peers_mask;
  constexpr int NB = kKeyedB / 16 / 64;                // batches of 64 lanes per wave span
  // ---- bucket + rank instead of the LSD passes (~12 us each) -----------------------------------------------------------
  // The (row, slot) pairs are all different, so the sorted order is unique and the algorithm need not be stable: distribute
  // the pairs over buckets that are monotone in (row, slot) with plain LDS atomics (whatever order they are served in), scan,
  // scatter, then every element ranks itself inside its bucket by comparing (row, slot) with the bucket's other members.
  // (buckets of ~2 members: with 1024 buckets of 8 the ranking step's LDS reads -- members^2 per bucket -- took longer than
  // the passes they replace.)
  // A bucket with more than kBucketCap members (hot rows: Zipf ids) sends the whole key to the LSD passes below, which
  // produce the same unique order.
  bool sorted_by_buckets = false;
  const uint32_t range = hi - lo + 1u;
  int e_lo = 0, e_hi = B;                              // this workgroup's share of the sorted positions
  if (B > 64) {
    constexpr uint32_t kBucketCap = 32;
    // bucket = leading part of the pair (row - lo, slot), <= 4096 buckets, monotone in (row, slot):
    //   range <= 4096 : (row, slot >> sh) with 4096 / range (rounded down to a power of two) sub-buckets per row
    //   wider         : row scaled to [0, 4096) by one 32 x 32 -> 64 multiply
    // Up to 19 bits of row range the pair travels as ONE word (row - lo) * 8192 + slot (half the LDS reads of the ranking
    // step); wider keys keep two arrays.
    const bool fine = range <= 4096u, one_word = range <= (1u << 19);
    int sub_log = 0;
    while (sub_log < 13 && (range << (sub_log + 1)) <= 4096u) ++sub_log;
    const int sh = 13 - sub_log;
    const int nbk = fine ? (int)(range << sub_log) : 4096;
    const uint32_t M = fine ? 0u : (uint32_t)((4096ull << 32) / (uint64_t)range);
    auto bucket_of = [&](uint32_t rl, uint32_t slot) -> uint32_t {
      return fine ? (rl << sub_log) | (slot >> sh) : (uint32_t)(((uint64_t)rl * M) >> 32);
    };
    uint32_t* cnt = &whist[0][0];                                             // [4096]
    uint32_t* start = reinterpret_cast<uint32_t*>(&peers_mask[0][0]);         // [4096] (the lane sets are zeroed again below)
    uint32_t* w1 = &keys[1][0];                                               // scattered: composite, or row - lo ...
    uint16_t* s1 = &vals[1][0];                                               // ... and slot (two-array form)
#pragma unroll
    for (int q = 0; q < 4; ++q) cnt[tid * 4 + q] = 0;
    __syncthreads();
    constexpr int PERL = kKeyedB / kKeyedThreads;
    uint32_t kk[PERL], pp[PERL];
#pragma unroll
    for (int j = 0; j < PERL; ++j) {
      const int b = tid + j * kKeyedThreads;
      kk[j] = b < B ? keys[0][b] - lo : 0u;
      pp[j] = 0;
      if (b < B) pp[j] = atomicAdd(&cnt[bucket_of(kk[j], (uint32_t)b)], 1u);
    }
    __syncthreads();
    uint32_t c4[4], tot = 0, mx = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      c4[q] = tid * 4 + q < nbk ? cnt[tid * 4 + q] : 0u;
      tot += c4[q];
      mx = c4[q] > mx ? c4[q] : mx;
    }
    if (!__syncthreads_or(mx > kBucketCap)) {
      uint32_t x = tot;                                 // exclusive scan: thread = 4 consecutive buckets
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(x, o);
        if (lane >= o) x += y;
      }
      if (lane == 63) red[wave] = x;
      __syncthreads();
      uint32_t run = x - tot;
      for (int w = 0; w < wave; ++w) run += red[w];
#pragma unroll
      for (int q = 0; q < 4; ++q) { start[tid * 4 + q] = run; run += c4[q]; }
      __syncthreads();
      // this share's buckets: rows [r_lo, r_hi) of the key's range (fine: a row owns 2^sub_log buckets; wider: a row owns one)
      uint32_t bk_lo, bk_hi;
      if (fine) {
        const uint32_t per = (range + (uint32_t)P - 1u) / (uint32_t)P;
        const uint32_t r_lo = min((uint32_t)part * per, range), r_hi = min(r_lo + per, range);
        bk_lo = r_lo << sub_log; bk_hi = r_hi << sub_log;
      } else {
        bk_lo = (uint32_t)part * 4096u / (uint32_t)P; bk_hi = (uint32_t)(part + 1) * 4096u / (uint32_t)P;
      }
      e_lo = bk_lo < (uint32_t)nbk ? (int)start[bk_lo] : B;
      e_hi = bk_hi < (uint32_t)nbk ? (int)start[bk_hi] : B;
#pragma unroll
      for (int j = 0; j < PERL; ++j) {
        const int b = tid + j * kKeyedThreads;
        if (b < B) {
          const uint32_t bk = bucket_of(kk[j], (uint32_t)b);
          if (bk >= bk_lo && bk < bk_hi) {
            const uint32_t pos = start[bk] + pp[j];
            w1[pos] = one_word ? (kk[j] << 13) | (uint32_t)b : kk[j];
            if (!one_word) s1[pos] = (uint16_t)b;
          }
        }
      }
      __syncthreads();
      // the thread's PERL elements rank themselves side by side: one loop to the longest of their buckets with PERL
      // independent LDS reads per trip (element by element the reads were one dependent chain each)
      uint32_t ek[PERL], ev[PERL], es[PERL], el[PERL], rk[PERL], maxlen = 0;
#pragma unroll
      for (int j = 0; j < PERL; ++j) {
        const int q = e_lo + tid + j * kKeyedThreads;
        const bool on = q < e_hi;
        const uint32_t w = on ? w1[q] : 0u;
        ek[j] = one_word ? w >> 13 : w;                 // row - lo
        ev[j] = one_word ? (w & 8191u) : (on ? (uint32_t)s1[q] : 0u);
        const uint32_t bk = on ? bucket_of(ek[j], ev[j]) : 0u;
        es[j] = on ? start[bk] : 0u;
        el[j] = on ? cnt[bk] : 0u;
        rk[j] = 0;
        maxlen = el[j] > maxlen ? el[j] : maxlen;
      }
      if (one_word) {
        for (uint32_t i = 0; i < maxlen; ++i) {
#pragma unroll
          for (int j = 0; j < PERL; ++j)
            rk[j] += (i < el[j] && w1[es[j] + (i < el[j] ? i : 0u)] < ((ek[j] << 13) | ev[j])) ? 1u : 0u;
        }
      } else {
        for (uint32_t i = 0; i < maxlen; ++i) {
#pragma unroll
          for (int j = 0; j < PERL; ++j) {
            const uint32_t at = es[j] + (i < el[j] ? i : 0u);
            const uint32_t ki = w1[at], vi = s1[at];
            rk[j] += (i < el[j] && (ki < ek[j] || (ki == ek[j] && vi < ev[j]))) ? 1u : 0u;
          }
        }
      }
#pragma unroll
      for (int j = 0; j < PERL; ++j)
        if (e_lo + tid + j * kKeyedThreads < e_hi) {
          keys[0][es[j] + rk[j]] = ek[j] + lo;
          vals[0][es[j] + rk[j]] = (uint16_t)ev[j];
        }
      sorted_by_buckets = true;
    }
    __syncthreads();
    for (int d = tid; d < 16 * 256; d += kKeyedThreads) (&peers_mask[0][0])[d] = 0ull;     // `start` lived there
    __syncthreads();
  }
  if (!sorted_by_buckets) {                            // LSD passes: share 0 sorts the whole key, the others have nothing
    e_lo = 0;
    e_hi = part == 0 ? B : 0;
    if (part != 0) {
      if (tid == 0) { ucount[wg] = 0; ubase[wg] = ki * B; uend[wg] = ki * B; }
      return;
    }
  }
  for (int p = 0; p < (sorted_by_buckets ? 0 : passes); ++p) {
    const int shift = dbits * p;
    for (int d = tid; d < 16 * 256; d += kKeyedThreads) (&whist[0][0])[d] = 0;
    uint32_t kreg[NB];
    uint16_t vreg[NB];
#pragma unroll
    for (int q = 0; q < NB; ++q) {                      // the span's elements up front: one LDS round trip, not NB
      const int i = wlo + q * 64 + lane;
      kreg[q] = i < whi ? keys[cur][i] : 0u;
      vreg[q] = i < whi ? vals[cur][i] : (uint16_t)0;
    }
    // phase 1 -- who shares my digit in my batch: every lane ORs its bit into a per-(wave, digit) LDS word (the
    // result of an OR does not depend on the order the lanes are served in), reads the word back and clears it.
    // One 64-bit LDS atomic + one read per batch instead of eight ballots with per-lane 64-bit selects (that
    // loop was VALU-bound), and nothing in batch q+1 waits for batch q: the NB batches pipeline in the LDS queue.
    uint64_t peers[NB];
#pragma unroll
    for (int q = 0; q < NB; ++q) {
      const bool valid = wlo + q * 64 + lane < whi;
      const uint32_t d = ((kreg[q] - lo) >> shift) & dmask;
      if (valid) __hip_atomic_fetch_or(const_cast<unsigned long long*>(&pm[wave][d]), 1ull << lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
      __builtin_amdgcn_wave_barrier();
      peers[q] = valid ? pm[wave][d] : 0ull;
      __builtin_amdgcn_wave_barrier();
      if (valid) pm[wave][d] = 0ull;                    // every peer writes the same zero: no leader needed yet
      __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();                                    // whist zeroed by everyone
    // per-(wave, digit) counts: one lane per distinct digit of a batch adds the batch's count
#pragma unroll
    for (int q = 0; q < NB; ++q) {
      const uint32_t d = ((kreg[q] - lo) >> shift) & dmask;
      const bool leader = peers[q] != 0ull && (peers[q] & lt_mask) == 0ull;
      if (leader) atomicAdd(&whist[wave][d], (uint32_t)__popcll(peers[q]));
    }
    __syncthreads();
    {
      // exclusive prefix over the 4096 (digit, wave) counters in digit-major order: thread t owns digit t/4,
      // waves 4*(t%4) .. +3; wave-level scan of the thread sums, then the 16 wave totals
      const int d = tid >> 2, w0 = (tid & 3) * 4;
      uint32_t c4[4], tot = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) { c4[j] = whist[w0 + j][d]; tot += c4[j]; }
      uint32_t x = tot;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(x, o);
        if (lane >= o) x += y;
      }
      if (lane == 63) red[wave] = x;
      __syncthreads();
      uint32_t run = x - tot;
      for (int w = 0; w < wave; ++w) run += red[w];
#pragma unroll
      for (int j = 0; j < 4; ++j) { whist[w0 + j][d] = run; run += c4[j]; }
    }
    __syncthreads();
    // phase 2 -- positions: the batch's leader of a digit takes the running offset (one lane per address and
    // instruction, batches in program order => deterministic) and hands it to its peers with a bpermute
    uint32_t base[NB];
#pragma unroll
    for (int q = 0; q < NB; ++q) {
      const uint32_t d = ((kreg[q] - lo) >> shift) & dmask;
      const bool leader = peers[q] != 0ull && (peers[q] & lt_mask) == 0ull;
      base[q] = 0;
      if (leader) base[q] = atomicAdd(const_cast<uint32_t*>(&wh[wave][d]), (uint32_t)__popcll(peers[q]));
    }
#pragma unroll
    for (int q = 0; q < NB; ++q) {
      const bool valid = peers[q] != 0ull;
      const int leader_lane = valid ? (int)__builtin_ctzll(peers[q]) : lane;
      const uint32_t b0 = (uint32_t)__builtin_amdgcn_ds_bpermute(leader_lane << 2, (int)base[q]);
      if (valid) {
        const uint32_t pos = b0 + (uint32_t)__popcll(peers[q] & lt_mask);
        keys[cur ^ 1][pos] = kreg[q];
        vals[cur ^ 1][pos] = vreg[q];
      }
    }
    __syncthreads();
    cur ^= 1;
  }
  // outputs: sorted slots, then the heads of this key (staged; compacted across keys by the second kernel)
  const int64_t gbase = (int64_t)ki * B;
  constexpr int PER = kKeyedB / kKeyedThreads;        // 8 contiguous elements per thread
  const int i_lo = e_lo + tid * PER;
  uint32_t flags = 0, c = 0;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int i = i_lo + j;
    if (i < e_hi) {
      sorted_src[gbase + i] = sbase + (int)vals[cur][i] * K + k;
      if (i == e_lo || keys[cur][i] != keys[cur][i - 1]) { flags |= 1u << j; ++c; }   // (a share starts at a row boundary)
    }
  }
  uint32_t x = c;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t y = __shfl_up(x, o);
    if (lane >= o) x += y;
  }
  __syncthreads();
  if (lane == 63) red[wave] = x;
  __syncthreads();
  uint32_t u = x - c;
  for (int w = 0; w < wave; ++w) u += red[w];
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    if (flags & (1u << j)) {                            // staged at the share's own positions: it has at most e_hi - e_lo heads
      uniq_stage[gbase + e_lo + u] = (int32_t)keys[cur][i_lo + j];
      seg_stage[gbase + e_lo + u] = (int32_t)(gbase + i_lo + j);
      ++u;
    }
  }
  if (tid == kKeyedThreads - 1) {
    ucount[wg] = (int32_t)u;
    ubase[wg] = (int32_t)(gbase + e_lo);
    uend[wg] = (int32_t)(gbase + e_hi);           // where the share's last segment ends
  }
}

__global__ __launch_bounds__(kKeyedThreads) void keyed_compact_kernel(CompactRider cr) { compact_body(cr, blockIdx.x); }

// two single words at unrelated addresses (an empty plan's n_unique and seg_offsets[0]) in ONE launch -- never a pair of
// hipMemsetAsync calls: captured into a graph, two memset nodes are the pattern that faulted on replay
__global__ void zero_two_words_kernel(int32_t* __restrict__ a, int32_t* __restrict__ b) {
  if (threadIdx.x == 0) a[0] = 0;
  if (threadIdx.x == 1) b[0] = 0;
}

// ------------------------------------------------------------------------------------------------
// host helpers
// ------------------------------------------------------------------------------------------------
struct DedupWs {
  uint32_t *keysA, *keysB, *valsB, *hist, *total, *blockcount;
  size_t bytes;
};

inline DedupWs dedup_layout(char* base, int64_t M) {
  DedupWs w;
  const uint32_t nblk = (uint32_t)tt_cdiv(M > 0 ? M : 1, kSortTile);
  size_t o = 0;
  auto take = [&](size_t n) { char* p = base ? base + o : nullptr; o += align256(n); return p; };
  w.keysA = reinterpret_cast<uint32_t*>(take(sizeof(uint32_t) * (size_t)(M + 1)));
  w.keysB = reinterpret_cast<uint32_t*>(take(sizeof(uint32_t) * (size_t)(M + 1)));
  w.valsB = reinterpret_cast<uint32_t*>(take(sizeof(uint32_t) * (size_t)(M + 1)));
  w.hist = reinterpret_cast<uint32_t*>(take(sizeof(uint32_t) * (size_t)2048 * nblk));
  w.total = reinterpret_cast<uint32_t*>(take(sizeof(uint32_t) * (size_t)2048));
  w.blockcount = reinterpret_cast<uint32_t*>(take(sizeof(uint32_t) * (size_t)(nblk + 1)));
  w.bytes = o;
  return w;
}

// segment heads of the sorted keys: unique rows, segment offsets, their number -- one chained launch, or count + write
static int launch_heads(tt_ctx* ctx, hipStream_t st, const DedupWs& w, int64_t M, uint32_t nblk, int32_t* n_unique, int32_t* unique_rows,
                        int32_t* seg_offsets, uint32_t drop_from) {
  uint32_t* chain = (int64_t)nblk + 1 <= ctx->chain_words && nblk <= 2048 ? tt_chain_for(ctx, st) : nullptr;
  if (chain) {
    head_chained_kernel<<<nblk, kThreads, 0, st>>>(w.keysA, (uint32_t)M, chain, n_unique, unique_rows, seg_offsets, drop_from, ctx->dev_err,
                                                   ctx->chain_spin);
    TT_LAUNCH_CHECK();
    return TT_OK;
  }
  head_count_kernel<<<nblk, kThreads, 0, st>>>(w.keysA, (uint32_t)M, w.blockcount);
  TT_LAUNCH_CHECK();
  head_write_kernel<<<nblk, kThreads, 0, st>>>(w.keysA, (uint32_t)M, w.blockcount, n_unique, unique_rows, seg_offsets, drop_from);
  TT_LAUNCH_CHECK();
  return TT_OK;
}

template <int BITS>
int sort_pass(hipStream_t st, const uint32_t* kin, const uint32_t* vin, uint32_t* kout, uint32_t* vout, uint32_t M, int shift,
              uint32_t* hist, uint32_t* total, uint32_t nblk) {
  sort_hist_kernel<BITS><<<nblk, kThreads, 0, st>>>(kin, M, shift, hist, nblk);
  TT_LAUNCH_CHECK();
  sort_colscan_kernel<BITS><<<(1u << BITS) / 64, 64 * kScanSeg, 0, st>>>(hist, nblk, total);
  TT_LAUNCH_CHECK();
  sort_scatter_kernel<BITS><<<nblk, kThreads, 0, st>>>(kin, vin, kout, vout, M, shift, hist, total);
  TT_LAUNCH_CHECK();
  return TT_OK;
}

}  // namespace

int tt_keyed_sort_run(const KeyedSortQueued& q, hipStream_t st, const BnFinishRiders* bf, int bf_wg) {
  if (!bf || bf_wg < 0 || bf_wg > TT_MAX_SIDES) bf_wg = 0;
  keyed_sort_kernel<<<bf_wg + q.grid, kKeyedThreads, 0, st>>>(q.a, q.rows, q.sorted_src, q.uniq_stage, q.seg_stage, q.ucount, q.ubase, q.uend,
                                                              q.key_major, q.long_counters, bf_wg > 0 ? *bf : BnFinishRiders{}, bf_wg);
  TT_LAUNCH_CHECK();
  return TT_OK;
}

extern "C" {

size_t tt_dedup_workspace_bytes(int64_t M) { return dedup_layout(nullptr, M).bytes; }

// tt_dedup_plan (pad false) and tt_dedup_plan_pad (pad true: keys in [0, table_rows], the key table_rows a pad that sorts last and is
// not counted -- one more key value for the digit plan, drop_from for the heads)
static int dedup_plan_impl(tt_ctx* ctx, const int32_t* rows, int64_t M, int64_t table_rows, int32_t* sorted_src, int32_t* unique_rows,
                           int32_t* seg_offsets, int32_t* n_unique, void* workspace, size_t workspace_bytes, tt_stream stream, bool pad) {
  TT_CHECK_ARG(ctx && sorted_src && unique_rows && seg_offsets && n_unique, "tt_dedup_plan: NULL output");
  TT_CHECK_ARG(M >= 0 && M < ((int64_t)1 << 31) - kSortTile, "tt_dedup_plan: M=%lld out of range", (long long)M);
  TT_CHECK_ARG(table_rows >= 1 && table_rows <= INT32_MAX, "tt_dedup_plan: table_rows=%lld out of range", (long long)table_rows);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (M == 0) {
    zero_two_words_kernel<<<1, 64, 0, st>>>(n_unique, seg_offsets);
    TT_LAUNCH_CHECK();
    return TT_OK;
  }
  TT_CHECK_ARG(rows && workspace, "tt_dedup_plan: NULL rows/workspace");
  if (workspace_bytes < tt_dedup_workspace_bytes(M)) {
    tt_set_error("tt_dedup_plan: workspace %zu < required %zu", workspace_bytes, tt_dedup_workspace_bytes(M));
    return TT_ERR_WORKSPACE;
  }
  DedupWs w = dedup_layout(reinterpret_cast<char*>(workspace), M);
  const uint32_t nblk = (uint32_t)tt_cdiv(M, kSortTile);
  int bits = 1;
  while (((int64_t)1 << bits) < table_rows + (pad ? 1 : 0)) ++bits;
  // digit plan: fewest passes with 8- or 11-bit digits
  int digit = 8, passes = (bits + 7) / 8;
  if ((bits + 10) / 11 < passes) { digit = 11; passes = (bits + 10) / 11; }
  // ping-pong so that the LAST pass lands values in sorted_src and keys in keysA
  const uint32_t* kin = reinterpret_cast<const uint32_t*>(rows);
  const uint32_t* vin = nullptr;
  for (int p = 0; p < passes; ++p) {
    const bool last_to_A = ((passes - 1 - p) % 2) == 0;
    uint32_t* kout = last_to_A ? w.keysA : w.keysB;
    uint32_t* vout = last_to_A ? reinterpret_cast<uint32_t*>(sorted_src) : w.valsB;
    int rc = digit == 8 ? sort_pass<8>(st, kin, vin, kout, vout, (uint32_t)M, p * digit, w.hist, w.total, nblk)
                        : sort_pass<11>(st, kin, vin, kout, vout, (uint32_t)M, p * digit, w.hist, w.total, nblk);
    if (rc != TT_OK) return rc;
    kin = kout;
    vin = vout;
  }
  return launch_heads(ctx, st, w, M, nblk, n_unique, unique_rows, seg_offsets, pad ? (uint32_t)table_rows : 0xFFFFFFFFu);
}

int tt_dedup_plan(tt_ctx* ctx, const int32_t* rows, int64_t M, int64_t table_rows, int32_t* sorted_src, int32_t* unique_rows,
                  int32_t* seg_offsets, int32_t* n_unique, void* workspace, size_t workspace_bytes, tt_stream stream) {
  return dedup_plan_impl(ctx, rows, M, table_rows, sorted_src, unique_rows, seg_offsets, n_unique, workspace, workspace_bytes, stream, false);
}

int tt_dedup_plan_pad(tt_ctx* ctx, const int32_t* rows, int64_t M, int64_t table_rows, int32_t* sorted_src, int32_t* unique_rows,
                      int32_t* seg_offsets, int32_t* n_unique, void* workspace, size_t workspace_bytes, tt_stream stream) {
  TT_CHECK_ARG(table_rows < INT32_MAX, "tt_dedup_plan_pad: no room for the pad key behind %lld rows", (long long)table_rows);
  return dedup_plan_impl(ctx, rows, M, table_rows, sorted_src, unique_rows, seg_offsets, n_unique, workspace, workspace_bytes, stream, true);
}

int tt_dedup_plan_runs(tt_ctx* ctx, const int32_t* rows, int32_t G, int64_t C, int64_t row_limit, int32_t* sorted_src,
                       int32_t* unique_rows, int32_t* seg_offsets, int32_t* n_unique, void* workspace, size_t workspace_bytes,
                       tt_stream stream) {
  TT_CHECK_ARG(ctx && rows && sorted_src && unique_rows && seg_offsets && n_unique && workspace, "tt_dedup_plan_runs: NULL argument");
  TT_CHECK_ARG(G >= 1 && G <= TT_MAX_RANKS && C >= 1 && (int64_t)G * C < ((int64_t)1 << 31) - kSortTile, "tt_dedup_plan_runs: bad G / C");
  const int64_t M = (int64_t)G * C;
  if (workspace_bytes < tt_dedup_workspace_bytes(M)) {
    tt_set_error("tt_dedup_plan_runs: workspace %zu < required %zu", workspace_bytes, tt_dedup_workspace_bytes(M));
    return TT_ERR_WORKSPACE;
  }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  DedupWs w = dedup_layout(reinterpret_cast<char*>(workspace), M);
  const uint32_t nblk = (uint32_t)tt_cdiv(M, kSortTile);
  merge_runs_kernel<<<grid_for(ctx, M), kThreads, 0, st>>>(rows, (uint32_t)G, (uint32_t)C, w.keysA, sorted_src);
  TT_LAUNCH_CHECK();
  return launch_heads(ctx, st, w, M, nblk, n_unique, unique_rows, seg_offsets,
                      row_limit > 0 && row_limit < (int64_t)0xFFFFFFFFll ? (uint32_t)row_limit : 0xFFFFFFFFu);
}

size_t tt_dedup_keyed_workspace_bytes(int64_t M, int32_t n_keys) {
  return align256(sizeof(int32_t) * (size_t)(M > 0 ? M : 1)) * 2 +
         3 * align256(sizeof(int32_t) * (size_t)(n_keys > 0 ? n_keys : 1) * kKeyedMaxParts);      // + head counts, stage bases and ends per (key, share)
}

static int dedup_plan_keyed_impl(tt_ctx* ctx, const int32_t* rows, const int32_t* side_K, int32_t n_sides, int64_t B, int32_t* sorted_src,
                                 int32_t* unique_rows, int32_t* seg_offsets, int32_t* n_unique, void* workspace, size_t workspace_bytes,
                                 tt_stream stream, bool key_major, int32_t E = 0, void* grad_ws = nullptr, size_t grad_ws_bytes = 0) {
  TT_CHECK_ARG(ctx && rows && side_K && sorted_src && unique_rows && seg_offsets && n_unique && workspace, "tt_dedup_plan_keyed: NULL argument");
  TT_CHECK_ARG(n_sides >= 1 && n_sides <= TT_MAX_SIDES, "tt_dedup_plan_keyed: n_sides=%d", n_sides);
  if (B < 1 || B > kKeyedB) {
    tt_set_error("tt_dedup_plan_keyed: B=%lld not in [1, %d]; use tt_dedup_plan", (long long)B, kKeyedB);
    return TT_ERR_UNSUPPORTED;
  }
  KeyedArgs a{};
  a.n_sides = n_sides;
  a.B = (int32_t)B;
  int n_keys = 0;
  int64_t slots = 0;
  for (int i = 0; i < n_sides; ++i) {
    TT_CHECK_ARG(side_K[i] >= 0, "tt_dedup_plan_keyed: negative K");
    a.side_base[i] = (int32_t)slots;
    a.key_base[i] = n_keys;
    a.K[i] = side_K[i];
    n_keys += side_K[i];
    slots += B * side_K[i];
  }
  a.side_base[n_sides] = (int32_t)slots;
  a.key_base[n_sides] = n_keys;
  TT_CHECK_ARG(slots < ((int64_t)1 << 31), "tt_dedup_plan_keyed: too many slots");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (n_keys == 0) {
    zero_two_words_kernel<<<1, 64, 0, st>>>(n_unique, seg_offsets);
    TT_LAUNCH_CHECK();
    return TT_OK;
  }
  if (workspace_bytes < tt_dedup_keyed_workspace_bytes(slots, n_keys)) {
    tt_set_error("tt_dedup_plan_keyed: workspace %zu < required %zu", workspace_bytes, tt_dedup_keyed_workspace_bytes(slots, n_keys));
    return TT_ERR_WORKSPACE;
  }
  char* w = reinterpret_cast<char*>(workspace);
  int32_t* uniq_stage = reinterpret_cast<int32_t*>(w);
  int32_t* seg_stage = reinterpret_cast<int32_t*>(w + align256(sizeof(int32_t) * (size_t)slots));
  int32_t* ucount = reinterpret_cast<int32_t*>(w + 2 * align256(sizeof(int32_t) * (size_t)slots));
  int32_t* ubase = reinterpret_cast<int32_t*>(w + 2 * align256(sizeof(int32_t) * (size_t)slots) +
                                              align256(sizeof(int32_t) * (size_t)n_keys * kKeyedMaxParts));
  int32_t* uend = reinterpret_cast<int32_t*>(w + 2 * align256(sizeof(int32_t) * (size_t)slots) +
                                             2 * align256(sizeof(int32_t) * (size_t)n_keys * kKeyedMaxParts));
  PlanLong pl{};
  if (grad_ws) {                                         // the gradient reduction's own workspace layout: its lists are filled here
    if (E < 1 || grad_ws_bytes < tt_embed_grad_workspace_bytes(slots, E)) {
      tt_set_error("tt_dedup_plan_keyed_long: gradient workspace %zu < required %zu", grad_ws_bytes, tt_embed_grad_workspace_bytes(slots, E));
      return TT_ERR_WORKSPACE;
    }
    const GradLayout gl = grad_layout(reinterpret_cast<char*>(grad_ws), slots, E);
    pl = PlanLong{gl.ws.counters, gl.ws.long_row, gl.ws.long_base, gl.ws.chunk_lo, gl.ws.chunk_hi};
  }
  // workgroups per key (TT_OPT_KEYED_PARTS overrides): the sort's scatter, ranking and output phases split P ways, the load and
  // histogram phases are repeated by every share; small batches are launch-bound anyway
  int parts = ctx->keyed_parts > 0 ? ctx->keyed_parts : (B >= 2048 ? 6 : 1);                        // (38 keys: 4 shares 17.9 us, 5: 17.4, 6: 17.2)
  if (parts > kKeyedMaxParts) parts = kKeyedMaxParts;
  while (parts > 1 && (int64_t)n_keys * parts > (int64_t)ctx->num_cus) --parts;        // a workgroup needs a CU of its own (144 KB of LDS)
  a.parts = parts;
  const KeyedSortQueued sq{a, rows, sorted_src, uniq_stage, seg_stage, ucount, ubase, uend, key_major, pl.counters, n_keys * parts};
  const CompactRider cr{uniq_stage, seg_stage, ucount, ubase, uend, pl, n_keys * parts, slots, unique_rows, seg_offsets, n_unique};
  // TT_OPT_DEFER_RIDERS: the compaction rides beside the towers' tail_fwd, and the sort itself waits for the towers' forward, which
  // issues it behind its front kernel with the BatchNorm statistics riders in its grid (nothing reads the plan before the compaction)
  if (ctx->dq->defer_riders & 1) return tt_deferred_queue_plan(ctx, st, sq, cr, n_keys * parts);
  if (int rc = tt_keyed_sort_run(sq, st, nullptr, 0)) return rc;
  keyed_compact_kernel<<<n_keys * parts, kKeyedThreads, 0, st>>>(cr);
  TT_LAUNCH_CHECK();
  return TT_OK;
}

int tt_dedup_plan_keyed(tt_ctx* ctx, const int32_t* rows, const int32_t* side_K, int32_t n_sides, int64_t B, int32_t* sorted_src,
                        int32_t* unique_rows, int32_t* seg_offsets, int32_t* n_unique, void* workspace, size_t workspace_bytes,
                        tt_stream stream) {
  return dedup_plan_keyed_impl(ctx, rows, side_K, n_sides, B, sorted_src, unique_rows, seg_offsets, n_unique, workspace, workspace_bytes,
                               stream, false);
}

int tt_dedup_plan_keyed_long(tt_ctx* ctx, const int32_t* rows, int32_t rows_key_major, const int32_t* side_K, int32_t n_sides, int64_t B,
                             int32_t E, int32_t* sorted_src, int32_t* unique_rows, int32_t* seg_offsets, int32_t* n_unique,
                             void* grad_workspace, size_t grad_workspace_bytes, void* workspace, size_t workspace_bytes, tt_stream stream) {
  TT_CHECK_ARG(grad_workspace, "tt_dedup_plan_keyed_long: NULL gradient workspace");
  return dedup_plan_keyed_impl(ctx, rows, side_K, n_sides, B, sorted_src, unique_rows, seg_offsets, n_unique, workspace, workspace_bytes,
                               stream, rows_key_major != 0, E, grad_workspace, grad_workspace_bytes);
}

int tt_dedup_plan_keyed_km(tt_ctx* ctx, const int32_t* rows_km, const int32_t* side_K, int32_t n_sides, int64_t B, int32_t* sorted_src,
                           int32_t* unique_rows, int32_t* seg_offsets, int32_t* n_unique, void* workspace, size_t workspace_bytes,
                           tt_stream stream) {
  return dedup_plan_keyed_impl(ctx, rows_km, side_K, n_sides, B, sorted_src, unique_rows, seg_offsets, n_unique, workspace, workspace_bytes,
                               stream, true);
}

}  // extern "C"
