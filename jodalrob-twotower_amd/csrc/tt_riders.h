// "Riders": small roles of the training step that depend on nothing the launches around them produce and are worth one launch
// each in the step's dependent chain (~5 us + a boundary) -- the compaction of the keyed duplicate-row plan (needs every sort
// workgroup's head count; first consumer: tt_embed_grad_bwd), the last reduction of the symmetric score forward (loss + metrics:
// read by the host only) and the finish of the towers' BatchNorm batch statistics.  This header holds their argument structs and
// their device bodies, which the stand-alone kernels and the host kernels (the towers' fused tails, 1024-thread workgroups like
// every role here; the keyed plan's sort; gemm_back_kernel, whose 256 threads run the loss reduction in the 1024-thread order) share,
// so results are bit-identical (test).  How they are queued, hosted and flushed: tt_deferred.h.
#pragma once
#include "tt_common.h"

constexpr int kRiderThreads = 1024;
// the long-row list of the segmented gradient reduction (rows with more than kPlanLongSeg slots are summed chunk by chunk), built
// by the plan's compaction instead of by the reduction itself: the reduction's row and chunk passes then run as ONE launch
constexpr int kPlanLongSeg = 64;
struct PlanLong {
  int32_t* counters;     // [0] chunks, [1] long rows (zeroed by keyed_sort_kernel, filled by the compaction)
  int32_t* long_row; int32_t* long_base; int32_t* chunk_lo; int32_t* chunk_hi;
};
struct CompactRider {
  const int32_t* uniq_stage; const int32_t* seg_stage; const int32_t* ucount; const int32_t* ubase; const int32_t* uend;
  PlanLong pl;
  int n_keys; int64_t M;
  int32_t* unique_rows; int32_t* seg_offsets; int32_t* n_unique;
};
struct Finish2Rider {
  const float* part; int n_wg, Dp; float fb, unscale; float* out; float* loss_out;
};
// The towers' BatchNorm batch statistics, finished ONCE per tower instead of by every tail workgroup: the chunk partials that
// tower_front / tail_head leave behind are merged by one workgroup per tower riding in front of the keyed plan's sort (its grid
// leaves CUs idle and it depends on nothing the towers produce), and the kernel boundary behind the sort hands (mean, rstd) to
// every workgroup of tail_fwd.  What the in-tail finish does once per tower -- the saved statistics of the backward, the running
// estimates, num_batches_tracked -- happens here instead, never in both places.
struct BnFinishRider {
  const float* partial; int64_t pstride; int nchunks, H;          // as BnStatArgs (pstride: floats between chunks, never 0 here)
  float* mean; float* rstd; float* rm; float* rv; int64_t* nbt;
  float* out;                                                     // [2][H]: mean, rstd (context-owned: tt_ctx::bn_fin)
};
struct BnFinishRiders { BnFinishRider r[TT_MAX_SIDES]; };
constexpr int kBnFinStride = 2 * 64;                              // floats per tower in tt_ctx::bn_fin (the narrow tail: H <= 64)

// the keyed plan's sort (keyed_sort_kernel, tt_plan.hip): argument block, and the whole launch (while it is held back: tt_deferred.h)
struct KeyedArgs {
  int32_t side_base[TT_MAX_SIDES + 1];   // first slot of side i
  int32_t key_base[TT_MAX_SIDES + 1];    // first key instance of side i
  int32_t K[TT_MAX_SIDES];
  int32_t n_sides;
  int32_t B;
  int32_t parts;                         // workgroups per key (range partition of the key's rows)
};
struct KeyedSortQueued {
  KeyedArgs a; const int32_t* rows; int32_t* sorted_src; int32_t* uniq_stage; int32_t* seg_stage; int32_t* ucount; int32_t* ubase;
  int32_t* uend; bool key_major; int32_t* long_counters; int grid;
};
// argument block of the two grid-row riders' stand-alone launch (riders_kernel, tt_ctx.hip): c_wg workgroups compact, one more reduces
struct tt_riders {
  CompactRider c; int c_wg;
  Finish2Rider f;
};

#ifdef __HIPCC__
// ---- column statistics of relu(pre): Welford per thread, Chan combine ------------------------
constexpr float kBnEps = 1e-5f, kBnMomentum = 0.1f;
constexpr int kMaxChunks = 128;  // row chunks of the two-stage column reductions
struct Wf {
  float n, mean, m2;
};
__device__ __forceinline__ Wf wf_combine(Wf a, Wf b) {
  if (b.n == 0.f) return a;
  if (a.n == 0.f) return b;
  Wf o;
  o.n = a.n + b.n;
  const float d = b.mean - a.mean, w = b.n / o.n;      // one division per combine (the chains of 32 are latency-bound)
  o.mean = a.mean + d * w;
  o.m2 = a.m2 + b.m2 + d * d * (a.n * w);
  return o;
}

// Canonical merge order of the chunk statistics (round 4; every finish -- bn_stats_finish_kernel, the fused tails, the SyncBN hand-over,
// the statistics rider -- uses it, so their results stay bit-identical to each other).  Chunk lane jl owns chunks jl, jl + 4, jl + 8, ...
// in four SUB-CHAINS of kMaxChunks / 16 chunks each:   lane(jl) = ((C0 + C1) + C2) + C3,  C_s = ((v[8 s] + v[8 s + 1]) + ...) + v[8 s + 7];
// the four lanes then merge as (lane0 + lane1) + (lane2 + lane3).  Sub-chains exist so that a 1024-thread workgroup can give each one to
// its own thread (16 per column: 8 triples in flight per thread instead of 32 -- 52 registers, two workgroups per CU) without changing
// the association; before, a lane was one chain of 32.
constexpr int kSubChain = kMaxChunks / 16;
__device__ __forceinline__ Wf wf_lane_merge(const Wf* v /* [kMaxChunks / 4] */) {
  Wf o{0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    Wf cs{0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < kSubChain; ++i) cs = wf_combine(cs, v[kSubChain * s + i]);
    o = wf_combine(o, cs);
  }
  return o;
}

// The finish as a 1024-thread workgroup runs it (the fused forward tail, or the statistics rider: ONE order, two hosts), in two steps
// around a barrier.  Step 1, thread (c, rq) = (t & 63, t >> 6): sub-chain rq >> 2 of chunk lane rq & 3 of column c -> sh[rq][c].
__device__ __forceinline__ Wf bn_finish_subchain(const float* __restrict__ partial, int64_t ps, int nchunks, int H, int c, int rq) {
  Wf cs{0.f, 0.f, 0.f};
  if (c < H) {
    const int jl = rq & 3, sc = rq >> 2;
    Wf v[kSubChain];
#pragma unroll
    for (int i = 0; i < kSubChain; ++i) {
      const int k = jl + 4 * (kSubChain * sc + i);
      const float* q = partial + (int64_t)min(k, nchunks - 1) * ps;      // (clamped address, no branch around the loads)
      const float x0 = q[c], x1 = q[H + c], x2 = q[2 * H + c];
      v[i] = k < nchunks ? Wf{x0, x1, x2} : Wf{0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int i = 0; i < kSubChain; ++i) cs = wf_combine(cs, v[i]);
  }
  return cs;
}
// Step 2, one thread per column c < H: the sub-chains of every lane, the four lanes, variance and rstd.  `once`: this thread also
// does what happens once per tower and pass (saved statistics, running estimates as nn.BatchNorm1d -- momentum 0.1, unbiased
// variance --, num_batches_tracked).
__device__ __forceinline__ void bn_finish_column(const Wf (*sh)[64], int c, bool once, float* mean_out, float* rstd_out, float* rm,
                                                 float* rv, int64_t* nbt, float& mean, float& rstd) {
  Wf ln[4];
#pragma unroll
  for (int jl = 0; jl < 4; ++jl) {                       // lane(jl) = ((C0 + C1) + C2) + C3, starting from the empty statistic
    Wf o{0.f, 0.f, 0.f};
#pragma unroll
    for (int sc = 0; sc < 4; ++sc) o = wf_combine(o, sh[4 * sc + jl][c]);
    ln[jl] = o;
  }
  const Wf o = wf_combine(wf_combine(ln[0], ln[1]), wf_combine(ln[2], ln[3]));
  const float var = o.n > 0.f ? o.m2 / o.n : 0.f;
  mean = o.mean;
  rstd = 1.f / sqrtf(var + kBnEps);
  if (once) {
    mean_out[c] = o.mean;
    rstd_out[c] = rstd;
    if (rm) {
      rm[c] = (1.f - kBnMomentum) * rm[c] + kBnMomentum * o.mean;
      rv[c] = (1.f - kBnMomentum) * rv[c] + kBnMomentum * (o.n > 1.f ? o.m2 / (o.n - 1.f) : var);
    }
    if (nbt && c == 0) nbt[0] += 1;
  }
}
// the statistics rider's workgroup (kRiderThreads threads); sh: 16 x 64 triples of the host kernel's LDS
__device__ __forceinline__ void bn_finish_body(const BnFinishRider& r, Wf (*sh)[64]) {
  const int t = threadIdx.x, c = t & 63, rq = t >> 6;
  sh[rq][c] = bn_finish_subchain(r.partial, r.pstride, r.nchunks, r.H, c, rq);
  __syncthreads();
  if (t < 64 && c < r.H) {
    float mean, rstd;
    bn_finish_column(sh, c, true, r.mean, r.rstd, r.rm, r.rv, r.nbt, mean, rstd);
    r.out[c] = mean;
    r.out[r.H + c] = rstd;
  }
}

// workgroup ki of the keyed plan's compaction (kRiderThreads threads)
__device__ __forceinline__ void compact_body(const CompactRider& cr, int ki) {
  const int32_t* __restrict__ uniq_stage = cr.uniq_stage;
  const int32_t* __restrict__ seg_stage = cr.seg_stage;
  const int32_t* __restrict__ ucount = cr.ucount;
  const int32_t* __restrict__ ubase = cr.ubase;
  const int32_t* __restrict__ uend = cr.uend;
  const PlanLong pl = cr.pl;
  const int n_keys = cr.n_keys;
  const int64_t M = cr.M;
  int32_t* __restrict__ unique_rows = cr.unique_rows;
  int32_t* __restrict__ seg_offsets = cr.seg_offsets;
  int32_t* __restrict__ n_unique = cr.n_unique;
  constexpr int kKeyedThreads = kRiderThreads;

  // head counts of all (key, share) pairs -- a few dozen to a few hundred -- added up in parallel (integer sums: any order)
  __shared__ int sred[2][kKeyedThreads / 64];
  int before = 0, all = 0;
  for (int q = threadIdx.x; q < n_keys; q += kKeyedThreads) {
    const int v = ucount[q];
    all += v;
    if (q < ki) before += v;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    before += __shfl_xor(before, o);
    all += __shfl_xor(all, o);
  }
  if ((threadIdx.x & 63) == 0) { sred[0][threadIdx.x >> 6] = before; sred[1][threadIdx.x >> 6] = all; }
  __syncthreads();
  before = 0; all = 0;
#pragma unroll
  for (int w = 0; w < kKeyedThreads / 64; ++w) { before += sred[0][w]; all += sred[1][w]; }
  const int U = ucount[ki];
  const int64_t gbase = ubase[ki];
  for (int u = threadIdx.x; u < U; u += kKeyedThreads) {
    unique_rows[before + u] = uniq_stage[gbase + u];
    const int32_t s0 = seg_stage[gbase + u];
    seg_offsets[before + u] = s0;
    if (pl.counters) {                                   // long rows -> chunk list (what seg_reduce_kernel registers otherwise)
      const int32_t s1 = u + 1 < U ? seg_stage[gbase + u + 1] : uend[ki];
      if (s1 - s0 > kPlanLongSeg) {
        const int32_t nch = (s1 - s0 + kPlanLongSeg - 1) / kPlanLongSeg;
        const int32_t cb = atomicAdd(&pl.counters[0], nch);
        const int32_t li = atomicAdd(&pl.counters[1], 1);
        pl.long_row[li] = before + u;
        pl.long_base[li] = cb;
        for (int32_t c = 0; c < nch; ++c) {
          pl.chunk_lo[cb + c] = s0 + c * kPlanLongSeg;
          pl.chunk_hi[cb + c] = min(s1, s0 + (c + 1) * kPlanLongSeg);
        }
      }
    }
  }
  if (ki == 0 && threadIdx.x == 0) {
    n_unique[0] = all;
    seg_offsets[all] = (int32_t)M;
  }
}

// the one workgroup that adds the symmetric forward's partial records in a fixed order (item (j, q): records q, q + 4, ... of entry
// j, the four partial sums in order); loss and metrics (out8 as tt_score_loss_finish).  The order is the one of a kRiderThreads
// workgroup whose thread i runs item (i & 255, i >> 8); a host with NT threads (a power of two, 256 at least) lets thread t stand in
// for the threads t, t + NT, ... of that workgroup, each item summed in its own order with the items' loads in flight together:
// the same sums, the same results.  lds: kFinish2Lds floats.
constexpr int kFinish2Lds = 4 * (4 + 2 * 256) + 256;
template <int NT>
__device__ __forceinline__ void finish2_body(const Finish2Rider& fr, float* lds) {
  static_assert(NT >= 256 && kRiderThreads % NT == 0, "thread t stands in for the threads t + NT i of a kRiderThreads workgroup");
  constexpr int NI = kRiderThreads / NT;
  const float* __restrict__ part = fr.part;
  const int n_wg = fr.n_wg, Dp = fr.Dp;
  const float fb = fr.fb, unscale = fr.unscale;
  float* __restrict__ out = fr.out;
  float* __restrict__ loss_out = fr.loss_out;

  float (*red)[4 + 2 * 256] = reinterpret_cast<float (*)[4 + 2 * 256]>(lds);
  float* prod = lds + 4 * (4 + 2 * 256);
  const int t = threadIdx.x, q0 = t >> 8, j0 = t & 255, stride = 4 + 2 * Dp;
  for (int j = j0; j < stride; j += 256) {
    float s[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) s[i] = 0.f;
    for (int w0 = q0; w0 < n_wg; w0 += 32) {               // (item i: q = q0 + (NT / 256) i, its records q + 32 m + 4 k)
      float v[NI][8];
#pragma unroll
      for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const int w = w0 + (NT / 256) * i + 4 * k;
          v[i][k] = w < n_wg ? part[w * stride + j] : 0.f;       // (32-bit: n_wg * stride is a few thousand)
        }
#pragma unroll
      for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int k = 0; k < 8; ++k) s[i] += v[i][k];
    }
#pragma unroll
    for (int i = 0; i < NI; ++i) red[q0 + (NT / 256) * i][j] = s[i];
  }
  __syncthreads();
  if (t < 256) {
    float p = 0.f;
    if (t < Dp) {
      const float u = (red[0][4 + t] + red[1][4 + t]) + (red[2][4 + t] + red[3][4 + t]);
      const float v = (red[0][4 + Dp + t] + red[1][4 + Dp + t]) + (red[2][4 + Dp + t] + red[3][4 + Dp + t]);
      p = u * v;
    }
    prod[t] = p;
  }
  __syncthreads();
  if (t < 64) {
    float p = (prod[t] + prod[t + 64]) + (prod[t + 128] + prod[t + 192]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) p += __shfl_xor(p, o);
    if (t == 0) {
      const float tot = p * unscale;                       // sum of all s_ab / T = (sum_a n_a) . (sum_b c_b) / T
      const float l = (red[0][0] + red[1][0]) + (red[2][0] + red[3][0]);
      const float hit = (red[0][1] + red[1][1]) + (red[2][1] + red[3][1]);
      const float dsum = (red[0][2] + red[1][2]) + (red[2][2] + red[3][2]);
      const float pos = dsum / fb;
      const float neg = (tot - dsum) / (fb * fb - fb);     // mean over the off-diagonal (nan for B == 1, as torch)
      out[0] = 0.5f * l / fb;
      out[1] = hit / fb;
      out[2] = pos;
      out[3] = neg;
      out[4] = pos - neg;
      out[5] = 0.f;                                        // column-direction top-1 rate: first-call diagnostic only (two-direction kernel)
      out[6] = tot;
      out[7] = 0.f;
      if (loss_out) loss_out[0] = out[0];
    }
  }
}
// as a kRiderThreads workgroup of its own runs it (the stand-alone kernels, the tails' extra grid row)
__device__ __forceinline__ void finish2_body(const Finish2Rider& fr) {
  __shared__ float lds[kFinish2Lds];
  finish2_body<kRiderThreads>(fr, lds);
}
#endif
