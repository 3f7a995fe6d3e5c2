// Row routing of the sharded step on gfx950: the plan's distinct rows go into fixed-capacity buckets per owner rank (stable, no
// host synchronisation), the owner gathers its rows, and the slots learn where their row's embedding arrives.  Shares only the
// slot helpers (tt_embed_slots.h).
#include "tt_common.h"
#include "tt_embed_slots.h"

namespace {

// ------------------------------------------------------------------------------------------------
// multi-GPU routing: distinct rows -> fixed-capacity owner buckets (stable, no host sync)
//   a workgroup of 4 waves covers 2048 consecutive plan rows, a wave 512 of them in 8 batches of 64
// ------------------------------------------------------------------------------------------------
constexpr int kRouteChunk = 2048, kRouteWaves = 4;

struct RoutePads { int32_t id[TT_MAX_RANKS]; };

__global__ __launch_bounds__(kThreads) void route_count_kernel(const int32_t* __restrict__ unique_rows, const int32_t* __restrict__ n_unique,
                                                              uint32_t G, uint32_t* __restrict__ seg_counts) {
  __shared__ uint32_t cnt[kRouteWaves][TT_MAX_RANKS];
  const uint32_t U = (uint32_t)*n_unique, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane < G) cnt[wave][lane] = 0;
  __builtin_amdgcn_wave_barrier();
  const uint32_t u0 = blockIdx.x * kRouteChunk + wave * (kRouteChunk / kRouteWaves);
#pragma unroll
  for (int q = 0; q < kRouteChunk / kRouteWaves / 64; ++q) {
    const uint32_t u = u0 + q * 64 + lane;
    if (u < U) atomicAdd(&cnt[wave][(uint32_t)unique_rows[u] % G], 1u);
  }
  __builtin_amdgcn_wave_barrier();
  if (lane < G) seg_counts[((size_t)blockIdx.x * kRouteWaves + wave) * G + lane] = cnt[wave][lane];
}

// Every workgroup adds up the (block, wave) segment counts itself -- all of them for the totals (pads, counts, overflow flag), those
// in front of its own block for its starting offsets: nseg * G words from L2 per workgroup instead of a one-workgroup scan launch
// between the two passes (round 3: 6.4 us of the sharded step for 152 x 4 numbers).  Chaining the three passes through a ready-flag
// buffer in ONE launch was measured too: 19.7 us against 19.0 for the three -- the last workgroup's serial tail ate the launches saved.
__global__ __launch_bounds__(kThreads) void route_scatter_kernel(const int32_t* __restrict__ unique_rows, const int32_t* __restrict__ n_unique,
                                                                uint32_t G, uint32_t C, const uint32_t* __restrict__ seg_counts,
                                                                int32_t* __restrict__ counts, int32_t* __restrict__ overflow, RoutePads pads,
                                                                int32_t pad_u, int32_t* __restrict__ send_ids, int32_t* __restrict__ send_u,
                                                                int32_t* __restrict__ pos_u) {
  __shared__ uint32_t tot[TT_MAX_RANKS], pre[TT_MAX_RANKS];
  __shared__ uint32_t off[kRouteWaves][TT_MAX_RANKS];
  __shared__ unsigned long long pm[kRouteWaves][TT_MAX_RANKS];
  const uint32_t U = (uint32_t)*n_unique, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t nseg = gridDim.x * kRouteWaves, my_first = blockIdx.x * kRouteWaves;
  if (threadIdx.x < G) { tot[threadIdx.x] = 0; pre[threadIdx.x] = 0; }
  __syncthreads();
  for (uint32_t e = threadIdx.x; e < nseg * G; e += kThreads) {
    const uint32_t v = seg_counts[e];
    if (v) {
      atomicAdd(&tot[e % G], v);
      if (e / G < my_first) atomicAdd(&pre[e % G], v);
    }
  }
  __syncthreads();
  if (blockIdx.x == 0 && threadIdx.x < G) {
    counts[threadIdx.x] = (int32_t)tot[threadIdx.x];
    if (tot[threadIdx.x] > C) overflow[0] = 1;          // sticky: the caller owns (and clears) the flag
  }
  // unused tail of every bucket: pad entries, written by the whole grid
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < G * C; i += gridDim.x * blockDim.x) {
    const uint32_t g = i / C, p = i - g * C;
    if (p >= tot[g]) { send_ids[i] = pads.id[g]; send_u[i] = pad_u; }
  }
  if (lane < G) {
    uint32_t o = pre[lane];
    for (uint32_t w = 0; w < wave; ++w) o += seg_counts[((size_t)my_first + w) * G + lane];
    off[wave][lane] = o;
    pm[wave][lane] = 0ull;
  }
  __builtin_amdgcn_wave_barrier();
  volatile uint32_t(*vo)[TT_MAX_RANKS] = off;
  volatile unsigned long long(*vp)[TT_MAX_RANKS] = pm;
  const uint64_t lt_mask = (1ull << lane) - 1ull;
  const uint32_t u0 = blockIdx.x * kRouteChunk + wave * (kRouteChunk / kRouteWaves);
#pragma unroll 1
  for (int q = 0; q < kRouteChunk / kRouteWaves / 64; ++q) {
    const uint32_t u = u0 + q * 64 + lane;
    const bool valid = u < U;
    const uint32_t row = valid ? (uint32_t)unique_rows[u] : 0u;
    const uint32_t g = row % G;
    // rank among the lanes of this batch with the same owner: OR-ed lane set (order-independent), as in the keyed sort
    if (valid) __hip_atomic_fetch_or(const_cast<unsigned long long*>(&vp[wave][g]), 1ull << lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    __builtin_amdgcn_wave_barrier();
    const uint64_t peers = valid ? vp[wave][g] : 0ull;
    __builtin_amdgcn_wave_barrier();
    if (valid) vp[wave][g] = 0ull;
    __builtin_amdgcn_wave_barrier();
    const uint32_t rank = (uint32_t)__popcll(peers & lt_mask);
    uint32_t pos = 0;
    if (valid) pos = vo[wave][g] + rank;
    __builtin_amdgcn_wave_barrier();
    if (valid && rank == 0) vo[wave][g] = pos + (uint32_t)__popcll(peers);
    __builtin_amdgcn_wave_barrier();
    if (valid) {
      if (pos < C) {
        send_ids[(size_t)g * C + pos] = (int32_t)(row / G);
        send_u[(size_t)g * C + pos] = (int32_t)u;
        pos_u[u] = (int32_t)(g * C + pos);
      } else {
        pos_u[u] = (int32_t)(G * C);                    // did not fit (flagged in the prologue): the row AFTER the buckets,
      }                                                 // which the caller keeps all-zero -- never another row's embedding
    }
  }
}

// out[i, :] = rows[i] < 0 ? 0 : table[min(rows[i], R - 1), :]   (16-byte lanes; the owner-side gather / gradient hand-over)
// OUT_BF16: rows leave as bf16 (RNE) -- what the bf16 tower input would round them to anyway, at half the wire bytes
template <bool OUT_BF16>
__global__ __launch_bounds__(kThreads) void gather_rows_kernel(const float* __restrict__ table, const int32_t* __restrict__ rows, uint32_t n,
                                                              int32_t R, uint32_t C4, void* __restrict__ out) {
  const uint64_t total = (uint64_t)n * C4;
  for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t i = (uint32_t)(t / C4), c = (uint32_t)(t - (uint64_t)i * C4);
    int32_t r = rows[i];
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);                  // negative index: a zero row (unused bucket entries)
    if (r >= 0) v = reinterpret_cast<const float4*>(table)[(uint64_t)(r >= R ? R - 1 : r) * C4 + c];
    if (OUT_BF16) {
      ushort4 o;
      o.x = tt_f2bf(v.x); o.y = tt_f2bf(v.y); o.z = tt_f2bf(v.z); o.w = tt_f2bf(v.w);
      reinterpret_cast<ushort4*>(out)[(uint64_t)i * C4 + c] = o;
    } else {
      reinterpret_cast<float4*>(out)[(uint64_t)i * C4 + c] = v;
    }
  }
}

// idx_slot[slot] = pos_u[u] for the slots of plan row u: an 8-lane group per row
__global__ __launch_bounds__(kThreads) void route_expand_kernel(const int32_t* __restrict__ sorted_src, const int32_t* __restrict__ seg,
                                                               const int32_t* __restrict__ n_unique, const int32_t* __restrict__ pos_u,
                                                               int64_t* __restrict__ idx_slot) {
  const uint32_t U = (uint32_t)*n_unique;
  const uint32_t gthread = blockIdx.x * blockDim.x + threadIdx.x, lig = gthread & 7u;
  const uint32_t ngroups = gridDim.x * blockDim.x / 8;
  for (uint32_t u = gthread / 8; u < U; u += ngroups) {
    const int64_t v = pos_u[u];
    for (int32_t p = seg[u] + (int32_t)lig; p < seg[u + 1]; p += 8) idx_slot[sorted_src[p]] = v;
  }
}

}  // namespace

extern "C" {

size_t tt_route_workspace_bytes(int64_t M, int32_t G) {
  const int64_t nb = tt_cdiv(M > 0 ? M : 1, kRouteChunk);
  return align256(sizeof(uint32_t) * (size_t)nb * kRouteWaves * (size_t)(G > 0 ? G : 1));
}

static int route_bucket_impl(tt_ctx* ctx, const int32_t* unique_rows, const int32_t* n_unique, int64_t M, int32_t G, int32_t C,
                             const int32_t* pad_id, int32_t pad_u, int32_t* send_ids, int32_t* send_u, int32_t* pos_u, int32_t* counts,
                             int32_t* overflow, void* workspace, size_t workspace_bytes, const int32_t* sorted_src,
                             const int32_t* seg_offsets, int64_t* idx_slot, tt_stream stream) {
  TT_CHECK_ARG(ctx && unique_rows && n_unique && pad_id && send_ids && send_u && pos_u && counts && overflow && workspace,
               "tt_route_bucket: NULL argument");
  TT_CHECK_ARG(M >= 1 && M < ((int64_t)1 << 31) && G >= 1 && G <= TT_MAX_RANKS && C >= 1 && (int64_t)G * C < ((int64_t)1 << 31),
               "tt_route_bucket: bad M / G / C");
  TT_CHECK_ARG(idx_slot == nullptr || (sorted_src && seg_offsets), "tt_route_bucket_expand: NULL plan arrays");
  if (workspace_bytes < tt_route_workspace_bytes(M, G)) {
    tt_set_error("tt_route_bucket: workspace %zu < required %zu", workspace_bytes, tt_route_workspace_bytes(M, G));
    return TT_ERR_WORKSPACE;
  }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const unsigned nb = (unsigned)tt_cdiv(M, kRouteChunk);
  uint32_t* seg = reinterpret_cast<uint32_t*>(workspace);
  RoutePads pads{};
  for (int g = 0; g < G; ++g) pads.id[g] = pad_id[g];
  route_count_kernel<<<nb, kThreads, 0, st>>>(unique_rows, n_unique, (uint32_t)G, seg);
  TT_LAUNCH_CHECK();
  route_scatter_kernel<<<nb, kThreads, 0, st>>>(unique_rows, n_unique, (uint32_t)G, (uint32_t)C, seg, counts, overflow, pads, pad_u, send_ids,
                                                send_u, pos_u);
  TT_LAUNCH_CHECK();
  if (idx_slot != nullptr) {
    route_expand_kernel<<<grid_for(ctx, M * 8), kThreads, 0, st>>>(sorted_src, seg_offsets, n_unique, pos_u, idx_slot);
    TT_LAUNCH_CHECK();
  }
  return TT_OK;
}

int tt_route_bucket(tt_ctx* ctx, const int32_t* unique_rows, const int32_t* n_unique, int64_t M, int32_t G, int32_t C,
                    const int32_t* pad_id, int32_t pad_u, int32_t* send_ids, int32_t* send_u, int32_t* pos_u, int32_t* counts,
                    int32_t* overflow, void* workspace, size_t workspace_bytes, tt_stream stream) {
  return route_bucket_impl(ctx, unique_rows, n_unique, M, G, C, pad_id, pad_u, send_ids, send_u, pos_u, counts, overflow, workspace,
                           workspace_bytes, nullptr, nullptr, nullptr, stream);
}

int tt_route_bucket_expand(tt_ctx* ctx, const int32_t* unique_rows, const int32_t* n_unique, int64_t M, int32_t G, int32_t C,
                           const int32_t* pad_id, int32_t pad_u, int32_t* send_ids, int32_t* send_u, int32_t* pos_u, int32_t* counts,
                           int32_t* overflow, void* workspace, size_t workspace_bytes, const int32_t* sorted_src,
                           const int32_t* seg_offsets, int64_t* idx_slot, tt_stream stream) {
  TT_CHECK_ARG(idx_slot != nullptr, "tt_route_bucket_expand: NULL idx_slot");
  return route_bucket_impl(ctx, unique_rows, n_unique, M, G, C, pad_id, pad_u, send_ids, send_u, pos_u, counts, overflow, workspace,
                           workspace_bytes, sorted_src, seg_offsets, idx_slot, stream);
}

int tt_gather_rows(tt_ctx* ctx, const float* table, int64_t table_rows, int32_t E, const int32_t* rows, int64_t n, void* out,
                   int32_t out_dtype, tt_stream stream) {
  TT_CHECK_ARG(ctx && table && rows && out, "tt_gather_rows: NULL argument");
  TT_CHECK_ARG(table_rows >= 1 && table_rows <= INT32_MAX && n >= 0 && n < ((int64_t)1 << 31) && E >= 4 && E % 4 == 0,
               "tt_gather_rows: bad shape (E must be a multiple of 4)");
  TT_CHECK_ARG(out_dtype == TT_F32 || out_dtype == TT_BF16, "tt_gather_rows: bad out_dtype");
  TT_CHECK_ARG(tt_aligned(table, 16) && tt_aligned(out, out_dtype == TT_BF16 ? 8 : 16), "tt_gather_rows: table / out alignment");
  if (n == 0) return TT_OK;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int grid = grid_for(ctx, n * (E / 4));
  if (out_dtype == TT_BF16) gather_rows_kernel<true><<<grid, kThreads, 0, st>>>(table, rows, (uint32_t)n, (int32_t)table_rows, (uint32_t)(E / 4), out);
  else gather_rows_kernel<false><<<grid, kThreads, 0, st>>>(table, rows, (uint32_t)n, (int32_t)table_rows, (uint32_t)(E / 4), out);
  TT_LAUNCH_CHECK();
  return TT_OK;
}

int tt_route_expand(tt_ctx* ctx, const int32_t* sorted_src, const int32_t* seg_offsets, const int32_t* n_unique, const int32_t* pos_u,
                    int64_t M, int64_t* idx_slot, tt_stream stream) {
  TT_CHECK_ARG(ctx && sorted_src && seg_offsets && n_unique && pos_u && idx_slot, "tt_route_expand: NULL argument");
  TT_CHECK_ARG(M >= 1, "tt_route_expand: M < 1");
  route_expand_kernel<<<grid_for(ctx, M * 8), kThreads, 0, reinterpret_cast<hipStream_t>(stream)>>>(sorted_src, seg_offsets, n_unique, pos_u,
                                                                                                      idx_slot);
  TT_LAUNCH_CHECK();
  return TT_OK;
}

}  // extern "C"
