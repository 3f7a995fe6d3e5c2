// The segmented gradient reduction's workspace (tt_grad.hip): the long rows' chunk lists and partials.  The keyed plan's
// compaction fills the lists (tt_plan.hip), the reduction sums the chunks, and either its own finish kernel or the fused
// optimiser launch (tt_optim.hip) adds a long row's partials up through long_rows_finish -- one body, so the same bits.
#pragma once
#include "tt_embed_slots.h"
#include "tt_riders.h"

namespace {

// segments longer than this are split into kLongSeg-slot chunks (4 trips each) summed by their own lane groups.
// (16 = one trip per chunk was tried: at the bench's 6,200 rows of 17-64 slots the two same-address atomics per long
//  row and a workgroup-per-row finish cost more than the serial trips save: 25 + 8 + 11 us against 14 + 9 + 5.)
constexpr int kLongSeg = 64;
static_assert(kPlanLongSeg == kLongSeg, "the plan's compaction and the reduction must cut long rows into the same chunks");

struct GradWs {
  int32_t* counters;     // [0] chunks allocated, [1] long rows
  int32_t* long_row;     // [maxLong]   distinct-row index u
  int32_t* long_base;    // [maxLong]   first chunk of that row
  int32_t* chunk_lo;     // [maxChunks]
  int32_t* chunk_hi;
  float* chunk_partial;  // [maxChunks, E]
};

struct GradLayout {
  GradWs ws;
  size_t bytes;
  int64_t max_long, max_chunks;
};

inline GradLayout grad_layout(char* base, int64_t M, int32_t E) {
  GradLayout g;
  g.max_long = M / kLongSeg + 1;
  g.max_chunks = M / kLongSeg + g.max_long + 1;
  size_t o = 0;
  auto take = [&](size_t n) { char* p = base ? base + o : nullptr; o += align256(n); return p; };
  g.ws.counters = reinterpret_cast<int32_t*>(take(sizeof(int32_t) * 3));     // chunks allocated, long rows, snapshot of the long-row count
  g.ws.long_row = reinterpret_cast<int32_t*>(take(sizeof(int32_t) * (size_t)g.max_long));
  g.ws.long_base = reinterpret_cast<int32_t*>(take(sizeof(int32_t) * (size_t)g.max_long));
  g.ws.chunk_lo = reinterpret_cast<int32_t*>(take(sizeof(int32_t) * (size_t)g.max_chunks));
  g.ws.chunk_hi = reinterpret_cast<int32_t*>(take(sizeof(int32_t) * (size_t)g.max_chunks));
  g.ws.chunk_partial = reinterpret_cast<float*>(take(sizeof(float) * (size_t)g.max_chunks * (size_t)E));
  g.bytes = o;
  return g;
}

// workgroups of a long-row finish: one per long row the workspace can list, at most eight per CU
inline int long_row_blocks(const tt_ctx* ctx, const GradLayout& gl) {
  const int64_t cap = (int64_t)ctx->num_cus * 8;
  return (int)(gl.max_long < cap ? gl.max_long : cap);
}

template <int VEC>
struct Acc {
  float v[VEC];
  __device__ __forceinline__ void zero() {
#pragma unroll
    for (int i = 0; i < VEC; ++i) v[i] = 0.f;
  }
};

// A row of more than kLongSeg slots met by an unplanned row pass (tt_grad.hip's, tt_embed_bag.hip's): the row's lane group
// enters it into the workspace's lists -- its chunks [s0 + c * kLongSeg, ...) are summed by a chunk pass, added up by
// long_rows_finish.  Called by every lane of the group (lig = its lane in the group of LG).
__device__ __forceinline__ void register_long_row(const GradWs& ws, uint32_t u, int32_t s0, int32_t s1, uint32_t lig, uint32_t LG) {
  const int32_t nch = (s1 - s0 + kLongSeg - 1) / kLongSeg;
  int32_t base = 0;
  if (lig == 0) {
    base = atomicAdd(&ws.counters[0], nch);
    const int32_t li = atomicAdd(&ws.counters[1], 1);
    ws.long_row[li] = (int32_t)u;
    ws.long_base[li] = base;
  }
  base = __shfl(base, 0, (int)LG);                     // the group's lanes write the chunk list together
  for (int32_t c = (int32_t)lig; c < nch; c += (int32_t)LG) {
    ws.chunk_lo[base + c] = s0 + c * kLongSeg;
    ws.chunk_hi[base + c] = min(s1, s0 + (c + 1) * kLongSeg);
  }
}

// one WORKGROUP per long row: its lane groups sum contiguous ranges of the row's chunk partials (8 loads in flight,
// chunk order), the group sums are added in group order through LDS -- one or two trips however long the row is
// (a binary key at B = 8192 has ~4096-slot rows = 256 partials)
constexpr int kFinishMaxFloats = 4096;     // (kThreads / LG) * E floats of LDS
// emit(u, col, total): called once per (long row, column) by the thread that added the group sums
// done(u): called by every thread of the workgroup once all of row u's emits have happened and are visible to the workgroup
struct NoRowDone {
  __device__ void operator()(int32_t) const {}
};
template <int VEC, typename EMIT, typename DONE = NoRowDone>
__device__ __forceinline__ void long_rows_finish(int32_t E, uint32_t C, const int32_t* __restrict__ seg, const GradWs& ws, uint32_t LG,
                                                 uint32_t bid, uint32_t nblocks, float* __restrict__ part, EMIT&& emit,
                                                 DONE&& done = DONE{}) {
  const uint32_t nlong = (uint32_t)ws.counters[2];        // the long-row count as seg_chunk_body saw it
  const uint32_t grp = threadIdx.x / LG, lig = threadIdx.x % LG, ngrp = blockDim.x / LG;
  for (uint32_t li = bid; li < nlong; li += nblocks) {
    const int32_t u = ws.long_row[li], base = ws.long_base[li];
    const int32_t nch = (seg[u + 1] - seg[u] + kLongSeg - 1) / kLongSeg;
    const int32_t per = (nch + (int32_t)ngrp - 1) / (int32_t)ngrp;
    const int32_t c0 = min(nch, (int32_t)grp * per), c1 = min(nch, c0 + per);
    for (uint32_t chunk = lig; chunk < C; chunk += LG) {
      Acc<VEC> acc;
      acc.zero();
      const float* p0 = ws.chunk_partial + (int64_t)base * E + chunk * VEC;
      int32_t c = c0;
      for (; c + 8 <= c1; c += 8) {
        float t[8][VEC];
#pragma unroll
        for (int j = 0; j < 8; ++j)
#pragma unroll
          for (int e = 0; e < VEC; ++e) t[j][e] = p0[(int64_t)(c + j) * E + e];
#pragma unroll
        for (int j = 0; j < 8; ++j)
#pragma unroll
          for (int e = 0; e < VEC; ++e) acc.v[e] += t[j][e];
      }
      for (; c < c1; ++c) {
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc.v[e] += p0[(int64_t)c * E + e];
      }
#pragma unroll
      for (int e = 0; e < VEC; ++e) part[grp * E + chunk * VEC + e] = acc.v[e];
    }
    __syncthreads();
    for (int32_t col = threadIdx.x; col < E; col += blockDim.x) {
      float tot = 0.f;
      for (uint32_t g = 0; g < ngrp; ++g) tot += part[g * E + col];
      emit(u, col, tot);
    }
    __syncthreads();
    done(u);     // (whatever it reads was written before the barrier above; the next row's emits follow the next barrier)
  }
}

// The finish kernels' body (tt_grad.hip's, tt_embed_bag.hip's): every long row's total into `out` in `mode` (TT_GRAD_*).
// part: kFinishMaxFloats floats of LDS.
template <int VEC>
__device__ __forceinline__ void long_rows_finish_into(int32_t E, uint32_t C, const int32_t* __restrict__ seg,
                                                      const int32_t* __restrict__ unique_rows, int32_t mode, float* __restrict__ out,
                                                      const GradWs& ws, uint32_t LG, float* __restrict__ part) {
  long_rows_finish<VEC>(E, C, seg, ws, LG, blockIdx.x, gridDim.x, part, [&](int32_t u, int32_t col, float tot) {
    const int64_t orow = mode == TT_GRAD_SPARSE ? (int64_t)u : (int64_t)unique_rows[u];
    float* o = out + orow * E + col;
    *o = mode == TT_GRAD_DENSE_ACC ? *o + tot : tot;
  });
}

// the widest row the finish's LDS holds for lane groups of LG: (kThreads / LG) * E floats
inline bool finish_fits(int32_t E, uint32_t LG) { return (int64_t)(kThreads / LG) * E <= kFinishMaxFloats; }

}  // namespace
