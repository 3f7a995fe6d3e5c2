// The embedding gradient on gfx950: an atomic-free segmented reduction of the towers' input gradients over a duplicate-row
// plan (tt_plan.hip), one row of the table's gradient per distinct row.  Long rows are cut into chunks summed by lane groups
// of their own and added up by a finish pass; the workspace and that finish body are shared with the plan and the fused
// optimiser launch (tt_grad_ws.h).  The hosted kernel also runs a queued slab reduction of the towers (tt_deferred.h).
#include "tt_common.h"
#include "tt_deferred.h"
#include "tt_embed_slots.h"
#include "tt_grad_ws.h"

namespace {

// ------------------------------------------------------------------------------------------------
// a16: segmented gradient reduction.  A lane-group of LG lanes owns one distinct row and walks its
// segment in ascending slot order (4 independent loads in flight, added in order).
// ------------------------------------------------------------------------------------------------
__global__ void zero_words_kernel(int32_t* __restrict__ p, int n) {
  if ((int)threadIdx.x < n) p[threadIdx.x] = 0;
}

// Gradient source address of (slot, chunk).  Branch-free on purpose: the side's fields are picked with selects
// on kernel-argument scalars (indexing a.s[] with a per-lane index turns every field into a dependent memory
// load) and the element type is a template parameter (a per-slot dtype branch keeps the compiler from batching
// the loads of a trip: 0.4 us PER SLOT measured, 26 us for one 64-slot chunk).
template <int VEC, int ESZ>
__device__ __forceinline__ const char* grad_addr(const SideSet& a, uint32_t slot, uint32_t chunk) {
  const char* base = a.s[0].out;
  int64_t ld = a.s[0].ld;
  uint32_t sb = 0, K = (uint32_t)a.s[0].K, magic = a.s[0].magic;
#pragma unroll
  for (int i = 1; i < TT_MAX_SIDES; ++i) {
    const bool sel = i < a.n && slot >= a.s[i].slot_base;
    base = sel ? a.s[i].out : base;
    ld = sel ? a.s[i].ld : ld;
    sb = sel ? a.s[i].slot_base : sb;
    K = sel ? (uint32_t)a.s[i].K : K;
    magic = sel ? a.s[i].magic : magic;
  }
  const uint32_t local = slot - sb;
  uint32_t b = __umulhi(local, magic);       // floor(local / K) or one less (magic = floor(2^32 / K))
  uint32_t k = local - b * K;
  if (k >= K) { k -= K; ++b; }
  return base + ((int64_t)b * ld + (int64_t)(k * (uint32_t)a.E + chunk * VEC)) * ESZ;
}

template <int VEC, int DT>
__device__ __forceinline__ void load_grad_chunk(const SideSet& a, uint32_t slot, uint32_t chunk, float* o) {
  if (DT == TT_F32) {
    const float* p = reinterpret_cast<const float*>(grad_addr<VEC, 4>(a, slot, chunk));
    if (VEC == 4) {
      const float4 t = *reinterpret_cast<const float4*>(p);
      o[0] = t.x; o[1 % VEC] = t.y; o[2 % VEC] = t.z; o[3 % VEC] = t.w;
    } else {
      o[0] = p[0];
    }
  } else {
    const uint16_t* p = reinterpret_cast<const uint16_t*>(grad_addr<VEC, 2>(a, slot, chunk));
    if (VEC == 4) {
      const ushort4 t = *reinterpret_cast<const ushort4*>(p);
      o[0] = tt_bf2f(t.x); o[1 % VEC] = tt_bf2f(t.y); o[2 % VEC] = tt_bf2f(t.z); o[3 % VEC] = tt_bf2f(t.w);
    } else {
      o[0] = tt_bf2f(p[0]);
    }
  }
}

// ordered sum of slots sorted_src[lo..hi) for one chunk column.  The walk is a dependent chain of trips
// (index load -> decode -> gradient load), so the trip count and the instructions per trip -- not bandwidth --
// set the kernel time.  kBatch gradient loads are in flight per trip.
//   LGT > 0 (lane group of LGT = 4, 8 or 16 lanes, all active): the lanes split the trip's index loads and
//   decodes (kBatch / LGT each) and hand the addresses round with ds_bpermute, instead of all decoding all.
//   LGT == 0: every lane decodes every slot (any group width).
constexpr int kBatch = 16;
#define TT_GLOBAL __attribute__((address_space(1)))
using tt_u32x4 = __attribute__((ext_vector_type(4))) uint32_t;
using tt_u32x2 = __attribute__((ext_vector_type(2))) uint32_t;

__device__ __forceinline__ uint64_t shfl_u64(uint64_t v, int src, int width) {
  const uint32_t lo = __shfl((uint32_t)v, src, width), hi = __shfl((uint32_t)(v >> 32), src, width);
  return ((uint64_t)hi << 32) | lo;
}

template <int VEC, int DT, int LGT>
__device__ __forceinline__ void sum_range(const SideSet& a, const int32_t* __restrict__ sorted_src, int32_t lo, int32_t hi,
                                          uint32_t chunk, uint32_t lig, Acc<VEC>& acc) {
  constexpr int ESZ = DT == TT_F32 ? 4 : 2;
  if (LGT > 0) {
    constexpr int PER = LGT > 0 ? kBatch / (LGT > 0 ? LGT : 1) : 1;
    int32_t idx[PER];
#pragma unroll
    for (int p = 0; p < PER; ++p) {
      const int32_t s = lo + p * LGT + (int32_t)lig;
      idx[p] = s < hi ? sorted_src[s] : 0;
    }
    for (int32_t i = lo; i < hi; i += kBatch) {
      const int32_t n = hi - i;                                   // group-uniform
      uint64_t mine[PER];
#pragma unroll
      for (int p = 0; p < PER; ++p) mine[p] = reinterpret_cast<uint64_t>(grad_addr<VEC, ESZ>(a, (uint32_t)idx[p], 0));
#pragma unroll
      for (int p = 0; p < PER; ++p) {                             // next trip's indices under this trip's loads
        const int32_t s = i + kBatch + p * LGT + (int32_t)lig;
        idx[p] = s < hi ? sorted_src[s] : 0;
      }
      // raw bits first, decode after the last load: a bf16 -> f32 convert inside the `j < n` branch makes the
      // compiler wait for each load where it stands (vmcnt(0) per slot: 27 us against 14 for the kernel)
      constexpr int RW = VEC * ESZ >= 4 ? VEC * ESZ / 4 : 1;
      uint32_t raw[kBatch][RW];
#pragma unroll
      for (int j = 0; j < kBatch; ++j) {
        const uint64_t ptr = shfl_u64(mine[j / LGT], j % LGT, LGT) + (uint64_t)chunk * VEC * ESZ;
        if (j < n) {
          if (RW == 4) {
            const tt_u32x4 q = *reinterpret_cast<const TT_GLOBAL tt_u32x4*>(ptr);
            raw[j][0] = q.x; raw[j][1 % RW] = q.y; raw[j][2 % RW] = q.z; raw[j][3 % RW] = q.w;
          } else if (RW == 2) {
            const tt_u32x2 q = *reinterpret_cast<const TT_GLOBAL tt_u32x2*>(ptr);
            raw[j][0] = q.x; raw[j][1 % RW] = q.y;
          } else if (ESZ == 4) {
            raw[j][0] = *reinterpret_cast<const TT_GLOBAL uint32_t*>(ptr);
          } else {
            raw[j][0] = *reinterpret_cast<const TT_GLOBAL uint16_t*>(ptr);
          }
        } else {
#pragma unroll
          for (int e = 0; e < RW; ++e) raw[j][e] = 0u;
        }
      }
#pragma unroll
      for (int j = 0; j < kBatch; ++j)
        if (j < n) {
#pragma unroll
          for (int e = 0; e < VEC; ++e) {
            float f;
            if (DT == TT_F32) f = __uint_as_float(raw[j][e % RW]);
            else f = __uint_as_float((e & 1) ? (raw[j][(e / 2) % RW] & 0xffff0000u) : (raw[j][(e / 2) % RW] << 16));
            acc.v[e] += f;
          }
        }
    }
    return;
  }
  int32_t i = lo;
  if (i + kBatch <= hi) {
    int32_t idx[kBatch];
#pragma unroll
    for (int j = 0; j < kBatch; ++j) idx[j] = sorted_src[i + j];
    for (; i + kBatch <= hi; i += kBatch) {
      float t[kBatch][VEC];
#pragma unroll
      for (int j = 0; j < kBatch; ++j) load_grad_chunk<VEC, DT>(a, (uint32_t)idx[j], chunk, t[j]);
      if (i + 2 * kBatch <= hi) {
#pragma unroll
        for (int j = 0; j < kBatch; ++j) idx[j] = sorted_src[i + kBatch + j];
      }
#pragma unroll
      for (int j = 0; j < kBatch; ++j)
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc.v[e] += t[j][e];
    }
  }
  for (; i + 4 <= hi; i += 4) {
    float t[4][VEC];
#pragma unroll
    for (int j = 0; j < 4; ++j) load_grad_chunk<VEC, DT>(a, (uint32_t)sorted_src[i + j], chunk, t[j]);
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int e = 0; e < VEC; ++e) acc.v[e] += t[j][e];
  }
  for (; i < hi; ++i) {
    float t[VEC];
    load_grad_chunk<VEC, DT>(a, (uint32_t)sorted_src[i], chunk, t);
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc.v[e] += t[e];
  }
}

template <int VEC>
__device__ __forceinline__ void write_row(float* __restrict__ out, int64_t row, int32_t E, uint32_t chunk, const Acc<VEC>& acc,
                                          bool accumulate) {
  float* p = out + row * E + chunk * VEC;
  if (VEC == 4) {
    float4 t = make_float4(acc.v[0], acc.v[1 % VEC], acc.v[2 % VEC], acc.v[3 % VEC]);
    if (accumulate) {
      const float4 q = *reinterpret_cast<float4*>(p);
      t.x += q.x; t.y += q.y; t.z += q.z; t.w += q.w;
    }
    *reinterpret_cast<float4*>(p) = t;
  } else {
    p[0] = accumulate ? p[0] + acc.v[0] : acc.v[0];
  }
}

// PLANNED: the long rows are already in the workspace's lists (built by the plan's compaction): nothing to register here.
// all_short (unplanned only): the caller knows no row is long, so every row is summed here whatever its length
template <int VEC, int DT, int LGT, bool PLANNED>
__device__ __forceinline__ void seg_reduce_body(const SideSet& a, const int32_t* __restrict__ sorted_src,
                                                const int32_t* __restrict__ seg, const int32_t* __restrict__ unique_rows,
                                                const int32_t* __restrict__ n_unique, int32_t mode,
                                                float* __restrict__ out, const GradWs& ws, uint32_t LG, bool all_short,
                                                uint32_t bid, uint32_t nblocks) {
  const uint32_t U = (uint32_t)*n_unique;
  const uint32_t gthread = bid * blockDim.x + threadIdx.x;
  const uint32_t lig = gthread % LG;
  const uint32_t ngroups = nblocks * blockDim.x / LG;
  for (uint32_t u = gthread / LG; u < U; u += ngroups) {
    const int32_t s0 = seg[u], s1 = seg[u + 1];
    if (PLANNED && s1 - s0 > kLongSeg) continue;
    if (!PLANNED && !all_short && s1 - s0 > kLongSeg) {
      register_long_row(ws, u, s0, s1, lig, LG);
      continue;
    }
    const int64_t orow = mode == TT_GRAD_SPARSE ? (int64_t)u : (int64_t)unique_rows[u];
    for (uint32_t chunk = lig; chunk < a.C; chunk += LG) {
      Acc<VEC> acc;
      acc.zero();
      sum_range<VEC, DT, LGT>(a, sorted_src, s0, s1, chunk, lig, acc);
      write_row<VEC>(out, orow, a.E, chunk, acc, mode == TT_GRAD_DENSE_ACC);
    }
  }
}

template <int VEC, int DT, int LGT>
__global__ __launch_bounds__(kThreads) void seg_reduce_kernel(SideSet a, const int32_t* __restrict__ sorted_src,
                                                             const int32_t* __restrict__ seg, const int32_t* __restrict__ unique_rows,
                                                             const int32_t* __restrict__ n_unique, int32_t mode,
                                                             float* __restrict__ out, GradWs ws, uint32_t LG, bool all_short) {
  seg_reduce_body<VEC, DT, LGT, false>(a, sorted_src, seg, unique_rows, n_unique, mode, out, ws, LG, all_short, blockIdx.x, gridDim.x);
}

template <int VEC, int DT, int LGT>
__device__ __forceinline__ void seg_chunk_body(const SideSet& a, const int32_t* __restrict__ sorted_src, const GradWs& ws, uint32_t LG,
                                               uint32_t bid, uint32_t nblocks) {
  const uint32_t nchunks = (uint32_t)ws.counters[0];
  if (bid == 0 && threadIdx.x == 0) ws.counters[2] = ws.counters[1];      // snapshot for seg_long_finish_kernel
  const uint32_t gthread = bid * blockDim.x + threadIdx.x;
  const uint32_t lig = gthread % LG;
  const uint32_t ngroups = nblocks * blockDim.x / LG;
  for (uint32_t c = gthread / LG; c < nchunks; c += ngroups) {
    for (uint32_t chunk = lig; chunk < a.C; chunk += LG) {
      Acc<VEC> acc;
      acc.zero();
      sum_range<VEC, DT, LGT>(a, sorted_src, ws.chunk_lo[c], ws.chunk_hi[c], chunk, lig, acc);
      write_row<VEC>(ws.chunk_partial, (int64_t)c, a.E, chunk, acc, false);
    }
  }
}

template <int VEC, int DT, int LGT>
__global__ __launch_bounds__(kThreads) void seg_chunk_kernel(SideSet a, const int32_t* __restrict__ sorted_src, GradWs ws, uint32_t LG) {
  seg_chunk_body<VEC, DT, LGT>(a, sorted_src, ws, LG, blockIdx.x, gridDim.x);
}

// measurement aid, compiled in with -DTT_SEG_STAMPS only (tools/r04_seg_stamps.py): start / end stamps and role of every workgroup
#ifdef TT_SEG_STAMPS
__device__ unsigned long long g_seg_stamps[4096 * 4];
#define TT_SEG_STAMP(i, role) do { __builtin_amdgcn_s_waitcnt(0); __syncthreads(); if (threadIdx.x == 0 && blockIdx.x < 4096) { \
  g_seg_stamps[blockIdx.x * 4 + (i)] = __builtin_amdgcn_s_memrealtime(); g_seg_stamps[blockIdx.x * 4 + 2] = (role) + 1; } } while (0)
#else
#define TT_SEG_STAMP(i, role) do { } while (0)
#endif

// The planned form: rows and chunks in ONE launch, because the plan's compaction has already built the long-row list -- the chunk
// pass no longer waits for the row pass to register the long rows -- and, in the same grid, the ns workgroups of a slab reduction
// tt_towers_mlp_bwd left queued in the context (TT_OPT_DEFER_SLAB_REDUCE; ns = 0: none): the weight gradients' split-K slabs and
// this reduction do not depend on each other.
// Order of the roles in the flat grid (round 4, from per-workgroup stamps: tools/r04_seg_stamps.py).  The machine holds ~1800 of these
// workgroups at a time and hands them out in index order: what comes first starts at once, what comes last starts when slots free up.
//   [the first kChunkFirst chunk workgroups: the long rows' chunks, four dependent trips of gathers (9 us) -- they used to be dispatched
//    last, started 10 us in and ended the launch]
//   [the slab items: 2-4 us each on the still empty machine; ONE workgroup per projection-bias item instead of a row of idle ones]
//   [the rows: 3.5 us each, the plan's small-vocabulary keys (33-64-slot rows: 11 us) first]
//   [the remaining chunk workgroups: idle unless the batch is skewed]
// Rows (all, or half of them) in front of the slab items measured slower (profiles/NOTES.md: 20.3-20.9 against 18.5-19.4 us);
// 512-thread workgroups and a cap of 4 or 5 waves per SIMD made no difference (same entry).
constexpr uint32_t kChunkFirst = 8;
template <int VEC, int DT, int LGT>
__global__ __launch_bounds__(kThreads) void seg_reduce_chunk_slab_kernel(SideSet a, const int32_t* __restrict__ sorted_src,
                                                                        const int32_t* __restrict__ seg, const int32_t* __restrict__ unique_rows,
                                                                        const int32_t* __restrict__ n_unique, int32_t mode,
                                                                        float* __restrict__ out, GradWs ws, uint32_t LG, uint32_t g1,
                                                                        SlabBatch sb, uint32_t nsx, uint32_t n_items, uint32_t ns) {
  const uint32_t g2 = gridDim.x - g1 - ns;
  const uint32_t gc = g2 < kChunkFirst ? g2 : kChunkFirst;
  // the workgroup's role (0 slabs, 1 rows, 2 chunks) and its index b among the role's workgroups
  uint32_t b = blockIdx.x;
  int role = 2;
  if (b >= gc) {
    b -= gc;
    if (b < ns) role = 0;
    else if (b - ns < g1) { role = 1; b -= ns; }
    else b -= ns + g1 - gc;
  }
  TT_SEG_STAMP(0, role);
  if (role == 0) {
    int item, bx;
    if (slab_role_locate(sb, (int)n_items, (int)nsx, (int)b, item, bx)) slab_reduce_block(sb, bx, (int)nsx, item);
  } else if (role == 1) {
    seg_reduce_body<VEC, DT, LGT, true>(a, sorted_src, seg, unique_rows, n_unique, mode, out, ws, LG, false, b, g1);
  } else {
    seg_chunk_body<VEC, DT, LGT>(a, sorted_src, ws, LG, b, g2);
  }
  TT_SEG_STAMP(1, role);
}

// RESET: the words [0] / [1] were counted up by this reduction's row pass (unplanned).  Planned, they are the PLAN's: its
// compaction counted them and every reduction over that plan reads them again, so they are left as they are (a graph replay
// rebuilds the plan, and keyed_sort_kernel zeroes them in front of its compaction).
template <int VEC, bool RESET = true>
__global__ __launch_bounds__(kThreads) void seg_long_finish_kernel(int32_t E, uint32_t C, const int32_t* __restrict__ seg,
                                                                  const int32_t* __restrict__ unique_rows, int32_t mode,
                                                                  float* __restrict__ out, GradWs ws, uint32_t LG) {
  __shared__ float part[kFinishMaxFloats];
  // nobody reads the live words [0] / [1] any more (counters[2] holds the snapshot), so one thread zeroes them here for the
  // next call -- a caller that keeps the words between calls needs no zeroing launch
  // (a "last workgroup done" atomic instead cost 35 us: 2048 same-address atomics with return serialise at ~17 ns each)
  if (RESET && blockIdx.x == 0 && threadIdx.x == 0) { ws.counters[0] = 0; ws.counters[1] = 0; }
  long_rows_finish_into<VEC>(E, C, seg, unique_rows, mode, out, ws, LG, part);
}

// ------------------------------------------------------------------------------------------------
// host helpers
// ------------------------------------------------------------------------------------------------
// one call of tt_embed_grad_bwd, checked and laid out: the kernels' common arguments, the grids of the row pass (g1), the chunk
// pass (g2) and the long-row finish (g3), and the form
struct SegCall {
  tt_ctx* ctx;
  hipStream_t st;
  SideSet a;
  const int32_t *sorted_src, *seg, *unique_rows, *n_unique;
  int32_t mode;
  float* out;
  GradWs ws;
  uint32_t LG;
  int g1, g2, g3;
  bool all_short, planned, defer;
  const TnPending* slabs;      // planned: the queued slab reduction this launch hosts (NULL: none)
};

// The launches of one reduction.  The caller's closing check is the finish's (and counts once more where the form has no finish).
//   planned   : rows, chunks and the hosted slab items in one launch, then the finish unless it is deferred
//   unplanned : the row pass registers the long rows, so the chunk pass is a launch of its own behind it; then the finish
//   short     : the unplanned row pass alone
template <int VEC, int DT, int LGT>
int seg_launch(const SegCall& c) {
  if (c.planned) {
    const int nsx = c.slabs ? tt_slab_role_blocks_x(c.slabs) : 0;
    const int ns = c.slabs ? tt_slab_role_blocks(c.slabs, nsx) : 0;
    seg_reduce_chunk_slab_kernel<VEC, DT, LGT><<<ns + c.g1 + c.g2, kThreads, 0, c.st>>>(
        c.a, c.sorted_src, c.seg, c.unique_rows, c.n_unique, c.mode, c.out, c.ws, c.LG, (uint32_t)c.g1, c.slabs ? c.slabs->sb : SlabBatch{},
        (uint32_t)nsx, (uint32_t)(c.slabs ? c.slabs->n : 0), (uint32_t)ns);
    TT_LAUNCH_CHECK();
    if (c.slabs) tt_deferred_taken(c.ctx, TT_DQ_SLABS);
    if (!c.defer) seg_long_finish_kernel<VEC, false><<<c.g3, kThreads, 0, c.st>>>(c.a.E, c.a.C, c.seg, c.unique_rows, c.mode, c.out, c.ws, c.LG);
    return TT_OK;
  }
  seg_reduce_kernel<VEC, DT, LGT><<<c.g1, kThreads, 0, c.st>>>(c.a, c.sorted_src, c.seg, c.unique_rows, c.n_unique, c.mode, c.out, c.ws, c.LG,
                                                               c.all_short);
  TT_LAUNCH_CHECK();
  if (c.all_short) return TT_OK;
  seg_chunk_kernel<VEC, DT, LGT><<<c.g2, kThreads, 0, c.st>>>(c.a, c.sorted_src, c.ws, c.LG);
  TT_LAUNCH_CHECK();
  seg_long_finish_kernel<VEC><<<c.g3, kThreads, 0, c.st>>>(c.a.E, c.a.C, c.seg, c.unique_rows, c.mode, c.out, c.ws, c.LG);
  return TT_OK;
}

template <int VEC, int DT>
int seg_launch_lgt(const SegCall& c, int lgt) {
  return lgt == 8 ? seg_launch<VEC, DT, 8>(c) : lgt == 16 ? seg_launch<VEC, DT, 16>(c) : lgt == 4 ? seg_launch<VEC, DT, 4>(c)
                                                                                                  : seg_launch<VEC, DT, 0>(c);
}

}  // namespace

extern "C" {

#ifdef TT_SEG_STAMPS
int tt_debug_seg_stamps(int clear, unsigned long long* host_out) {
  if (clear) {
    static unsigned long long zeros[4096 * 4];
    return hipMemcpyToSymbol(HIP_SYMBOL(g_seg_stamps), zeros, sizeof(zeros)) == hipSuccess ? 0 : 1;
  }
  return hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_seg_stamps), sizeof(unsigned long long) * 4096 * 4) == hipSuccess ? 0 : 1;
}
#endif

size_t tt_embed_grad_workspace_bytes(int64_t M, int32_t E) { return grad_layout(nullptr, M > 0 ? M : 1, E > 0 ? E : 1).bytes; }

int tt_embed_grad_bwd(tt_ctx* ctx, const tt_grad_src* srcs, int32_t n_srcs, int64_t B, int32_t E, const int32_t* sorted_src,
                      const int32_t* seg_offsets, const int32_t* unique_rows, const int32_t* n_unique, int64_t M, int32_t mode,
                      float* out, int32_t* counters, void* workspace, size_t workspace_bytes, tt_stream stream) {
  TT_CHECK_ARG(ctx && srcs && out, "tt_embed_grad_bwd: NULL argument");
  TT_CHECK_ARG(n_srcs >= 1 && n_srcs <= TT_MAX_SIDES, "tt_embed_grad_bwd: n_srcs=%d", n_srcs);
  // TT_GRAD_SHORT_SEGMENTS: every segment is summed by its own lane group whatever its length -- the right choice (and
  // three launches fewer) when the caller knows no segment is long, e.g. the owner side of the row exchange, where a
  // row arrives at most once per rank.  Results do not depend on the flag.
  const bool all_short = (mode & TT_GRAD_SHORT_SEGMENTS) != 0;
  const bool planned = (mode & TT_GRAD_PLANNED) != 0 && !all_short;      // the workspace holds the plan's long-row list and counters
  // TT_GRAD_DEFER_FINISH: the long rows' chunk partials are left unadded -- tt_adam_fused_step_finish (or tt_embed_grad_finish)
  // on the same workspace completes `out`; sparse mode on a planned workspace only
  const bool defer = (mode & TT_GRAD_DEFER_FINISH) != 0;
  mode &= ~(TT_GRAD_SHORT_SEGMENTS | TT_GRAD_PLANNED | TT_GRAD_DEFER_FINISH);
  TT_CHECK_ARG(!defer || (planned && mode == TT_GRAD_SPARSE), "tt_embed_grad_bwd: TT_GRAD_DEFER_FINISH needs TT_GRAD_PLANNED | TT_GRAD_SPARSE");
  TT_CHECK_ARG(mode >= TT_GRAD_SPARSE && mode <= TT_GRAD_DENSE_ACC, "tt_embed_grad_bwd: bad mode %d", mode);
  TT_CHECK_ARG(E >= 1 && B >= 0, "tt_embed_grad_bwd: bad E/B");
  if (M == 0) return TT_OK;
  TT_CHECK_ARG(sorted_src && seg_offsets && unique_rows && n_unique && workspace, "tt_embed_grad_bwd: NULL plan/workspace");
  if (workspace_bytes < tt_embed_grad_workspace_bytes(M, E)) {
    tt_set_error("tt_embed_grad_bwd: workspace %zu < required %zu", workspace_bytes, tt_embed_grad_workspace_bytes(M, E));
    return TT_ERR_WORKSPACE;
  }
  SideSet a{};
  a.n = n_srcs;
  a.E = E;
  bool vec4 = (E % 4 == 0) && tt_aligned(out, 16);
  int64_t slots = 0;
  for (int i = 0; i < n_srcs; ++i) {
    const tt_grad_src& s = srcs[i];
    TT_CHECK_ARG(s.K == 0 || s.d_out, "tt_embed_grad_bwd: src %d NULL", i);
    TT_CHECK_ARG(s.dtype == TT_F32 || s.dtype == TT_BF16, "tt_embed_grad_bwd: src %d bad dtype", i);
    TT_CHECK_ARG(s.dtype == srcs[0].dtype, "tt_embed_grad_bwd: all sources must share one dtype (src %d differs)", i);
    a.s[i] = SideDev{nullptr, nullptr, nullptr, const_cast<char*>(reinterpret_cast<const char*>(s.d_out)), s.ld, (uint32_t)slots, s.K, s.dtype, s.K > 1 ? (uint32_t)(0x100000000ull / (uint64_t)s.K) : 0xFFFFFFFFu};   // K = 1: 2^32 - 1, the fix-up step covers it
    const size_t esz = s.dtype == TT_BF16 ? 2 : 4;
    vec4 = vec4 && (s.ld % 4 == 0) && tt_aligned(s.d_out, 4 * esz);
    slots += B * s.K;
  }
  TT_CHECK_ARG(slots == M, "tt_embed_grad_bwd: sum(B*K)=%lld != M=%lld", (long long)slots, (long long)M);
  uint32_t LG;
  row_mapping(E, vec4, &a.C, &LG);
  a.total_slots = (uint32_t)slots;
  const int dt = srcs[0].dtype;
  // (before any launch: a refused call leaves the caller's counters and the plan's workspace as they were)
  if (!finish_fits(E, LG)) {
    tt_set_error("tt_embed_grad_bwd: E=%d too wide for the long-row finish (max %d)", E, kFinishMaxFloats * (int)LG / kThreads);
    return TT_ERR_UNSUPPORTED;
  }
  GradLayout gl = grad_layout(reinterpret_cast<char*>(workspace), M, E);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (int rc = tt_deferred_flush(ctx, TT_DQ_ALL & ~TT_DQ_SLABS)) return rc;      // nobody hosted them: this reduction reads the plan (and d_emb's products)
  if (planned) {
    // counters and lists were written into THIS workspace by tt_dedup_plan_keyed_long: nothing to zero, nothing to register
  } else if (counters) {
    gl.ws.counters = counters;      // caller-kept, zero on entry: the finish kernel re-zeroes them (one launch fewer per step)
  } else if (!all_short) {
    zero_words_kernel<<<1, 64, 0, st>>>(gl.ws.counters, 2);    // (a kernel, not a memset node: see graph notes in DESIGN.md)
    TT_LAUNCH_CHECK();
  }
  // a slab reduction the tower backward left in the context: inside this launch when the workspace is the plan's own (nothing
  // here then writes the shared scratch the slabs live in), launched on its own first otherwise
  int host_slabs = 0;
  if (int rc = planned ? tt_deferred_host(ctx, TT_DQ_SLABS, st, &host_slabs) : tt_deferred_flush(ctx, TT_DQ_SLABS)) return rc;
  const SegCall c{ctx, st, a, sorted_src, seg_offsets, unique_rows, n_unique, mode, out, gl.ws, LG, grid_for(ctx, M * LG),
                  grid_for(ctx, gl.max_chunks * LG), long_row_blocks(ctx, gl), all_short, planned, defer,
                  host_slabs ? &ctx->dq->slabs : nullptr};
  // all sources share one element type (checked above): it is a template parameter of the kernels, and so is
  // the lane-group width when every lane of a group owns exactly one chunk (shared decode, see sum_range)
  const int lgt = (vec4 && a.C == LG && (LG == 4 || LG == 8 || LG == 16)) ? (int)LG : 0;
  int rc;
  if (vec4 && dt == TT_F32) rc = seg_launch_lgt<4, TT_F32>(c, lgt);
  else if (vec4) rc = seg_launch_lgt<4, TT_BF16>(c, lgt);
  else if (dt == TT_F32) rc = seg_launch<1, TT_F32, 0>(c);
  else rc = seg_launch<1, TT_BF16, 0>(c);
  if (rc != TT_OK) return rc;
  TT_LAUNCH_CHECK();
  return TT_OK;
}

int tt_embed_grad_finish(tt_ctx* ctx, int32_t E, const int32_t* seg_offsets, int64_t M, float* out, void* workspace,
                         size_t workspace_bytes, tt_stream stream) {
  TT_CHECK_ARG(ctx && seg_offsets && out && workspace, "tt_embed_grad_finish: NULL argument");
  TT_CHECK_ARG(E >= 1 && M >= 1, "tt_embed_grad_finish: bad E/M");
  if (workspace_bytes < tt_embed_grad_workspace_bytes(M, E)) {
    tt_set_error("tt_embed_grad_finish: workspace %zu < required %zu", workspace_bytes, tt_embed_grad_workspace_bytes(M, E));
    return TT_ERR_WORKSPACE;
  }
  const bool vec4 = (E % 4 == 0) && tt_aligned(out, 16);
  uint32_t C, LG;
  row_mapping(E, vec4, &C, &LG);
  const GradLayout gl = grad_layout(reinterpret_cast<char*>(workspace), M, E);
  const int g3 = long_row_blocks(ctx, gl);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  // (deferred only from a planned reduction: the counters are the plan's)
  if (vec4) seg_long_finish_kernel<4, false><<<g3, kThreads, 0, st>>>(E, C, seg_offsets, nullptr, TT_GRAD_SPARSE, out, gl.ws, LG);
  else seg_long_finish_kernel<1, false><<<g3, kThreads, 0, st>>>(E, C, seg_offsets, nullptr, TT_GRAD_SPARSE, out, gl.ws, LG);
  TT_LAUNCH_CHECK();
  return TT_OK;
}

}  // extern "C"
