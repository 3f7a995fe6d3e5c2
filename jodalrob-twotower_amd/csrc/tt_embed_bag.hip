// Pooled multi-valued categorical features (embedding bags) on gfx950: the pooled lookup and its table gradient.  A bag is the
// run ids[offsets[slot] .. offsets[slot + 1]) of one (sample, key) slot.  Forward: one lane group of E/4 lanes per bag gathers
// the bag's rows with 16-byte loads and adds them in position order.  Backward: the lookup's duplicate-row plan over the
// POSITIONS' rows (tt_plan.hip, unchanged), reduced like tt_grad.hip's rows -- same chunking, same workspace, the same long-row
// finish body (tt_grad_ws.h) -- with the contribution of a position read through bag_of (its slot) and weighted for mean pooling.
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
};

// ------------------------------------------------------------------------------------------------
// forward.  A lane group owns one bag at a time; 64 / LG bags share a wave.  Per trip the group reads kBagBatch ids (every lane
// the same words), decodes them and issues all their row loads before the first add; the adds stay in position order.
// ------------------------------------------------------------------------------------------------
constexpr int kBagBatch = 8;

__global__ __launch_bounds__(kThreads) void bag_fwd_kernel(BagSet a, const float* __restrict__ table) {
  const uint32_t LG = a.LG;
  const uint32_t gthread = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t lig = gthread & (LG - 1);
  const uint32_t ngroups = gridDim.x * blockDim.x / LG;
  const bool live = lig < a.C;
  for (uint32_t slot = gthread / LG; slot < a.total_slots; slot += ngroups) {
    int si = 0;
#pragma unroll
    for (int i = 1; i < TT_MAX_SIDES; ++i)
      if (i < a.n && slot >= a.s[i].slot_base) si = i;
    const BagSideDev& s = a.s[si];
    const uint32_t local = slot - s.slot_base;
    const uint32_t b = local / (uint32_t)s.K;
    const uint32_t k = local - b * (uint32_t)s.K;
    int64_t o0 = s.offs[local], o1 = s.offs[local + 1];
    if (o0 < 0 || o1 < o0 || o1 > s.nnz) {                   // nothing is read through such a pair: the bag counts as empty
      if (lig == 0 && a.dev_err) atomicOr(a.dev_err, TT_DEVERR_BAG_OFFSETS);
      o0 = o1 = 0;
    }
    const int64_t hi = s.vocab[k] - 1, base = s.off[k];
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int64_t p = o0; p < o1; p += kBagBatch) {
      int64_t id[kBagBatch];
#pragma unroll
      for (int j = 0; j < kBagBatch; ++j) id[j] = p + j < o1 ? s.ids[p + j] : 0;
      float4 v[kBagBatch];
#pragma unroll
      for (int j = 0; j < kBagBatch; ++j) {
        v[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (p + j < o1) {
          const int64_t idc = id[j] < 0 ? 0 : (id[j] > hi ? hi : id[j]);             // clamp: cat_embed.py:117 (as the lookup)
          const int64_t row = row_in_table(base + idc, a.table_rows, a.dev_err);
          if (lig == ((uint32_t)j & (LG - 1))) {
            if (a.rows_out) a.rows_out[s.pos_base + (p + j)] = (int32_t)row;
            if (a.bag_of) a.bag_of[s.pos_base + (p + j)] = (int32_t)slot;
          }
          if (live) v[j] = *reinterpret_cast<const float4*>(table + row * a.E + lig * 4);
        }
      }
#pragma unroll
      for (int j = 0; j < kBagBatch; ++j) {
        if (p + j >= o1) continue;
        if (p + j == o0) {                                   // the first row as it is: a bag of one id is a bit-exact copy
          acc = v[j];
        } else {
          acc.x += v[j].x; acc.y += v[j].y; acc.z += v[j].z; acc.w += v[j].w;
        }
      }
    }
    const int64_t len = o1 - o0;
    if (len > 1 && s.pool[k] == TT_POOL_MEAN) {
      const float l = (float)len;
      acc.x /= l; acc.y /= l; acc.z /= l; acc.w /= l;
    }
    if (live) {
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
    if (slot + 1 == (si + 1 < a.n ? a.s[si + 1].slot_base : a.total_slots)) {
      const int64_t t0 = s.offs[local + 1];
      if (t0 >= 0 && t0 <= s.nnz)
        for (int64_t p = t0 + lig; p < s.nnz; p += LG) {
          if (a.rows_out) a.rows_out[s.pos_base + p] = 0;
          if (a.bag_of) a.bag_of[s.pos_base + p] = -1;
        }
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

__global__ void bag_zero_words_kernel(int32_t* __restrict__ p, int n) {
  if ((int)threadIdx.x < n) p[threadIdx.x] = 0;
}

// ordered sum over positions sorted_src[lo..hi) for one 16-byte column piece: acc = fma(w, x, acc) in that order, kBagBatch
// gradient loads in flight.  The side's fields are picked with selects on kernel-argument scalars, as tt_grad.hip's grad_addr does.
template <int DT>
__device__ __forceinline__ void bag_sum_range(const BagGradSet& a, const int32_t* __restrict__ sorted_src, int32_t lo, int32_t hi,
                                              uint32_t chunk, Acc<4>& acc) {
  constexpr int ESZ = DT == TT_F32 ? 4 : 2;
  for (int32_t i = lo; i < hi; i += kBagBatch) {
    int32_t slot[kBagBatch];
#pragma unroll
    for (int j = 0; j < kBagBatch; ++j) slot[j] = i + j < hi ? a.bag_of[sorted_src[i + j]] : -1;
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
      w[j] = a.inv_len ? a.inv_len[sl] : 1.f;
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
template <int DT>
__global__ __launch_bounds__(kThreads) void bag_reduce_kernel(BagGradSet a, const int32_t* __restrict__ sorted_src,
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
      bag_sum_range<DT>(a, sorted_src, s0, s1, lig, acc);
      bag_write_row(out, orow, a.E, lig, acc, mode == TT_GRAD_DENSE_ACC);
    }
  }
}

template <int DT>
__global__ __launch_bounds__(kThreads) void bag_chunk_kernel(BagGradSet a, const int32_t* __restrict__ sorted_src, GradWs ws, uint32_t LG) {
  const uint32_t nchunks = (uint32_t)ws.counters[0];
  if (blockIdx.x == 0 && threadIdx.x == 0) ws.counters[2] = ws.counters[1];      // snapshot for the finish
  const uint32_t gthread = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t lig = gthread % LG;
  const uint32_t ngroups = gridDim.x * blockDim.x / LG;
  for (uint32_t c = gthread / LG; c < nchunks; c += ngroups) {
    if (lig >= a.C) continue;
    Acc<4> acc;
    acc.zero();
    bag_sum_range<DT>(a, sorted_src, ws.chunk_lo[c], ws.chunk_hi[c], lig, acc);
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

extern "C" {

int tt_embed_bag_fwd(tt_ctx* ctx, const float* table, int64_t table_rows, int32_t E, const tt_bag_side* sides, int32_t n_sides,
                     int64_t B, int32_t* rows_out, int32_t* bag_of, tt_stream stream) {
  TT_CHECK_ARG(ctx && table && sides, "tt_embed_bag_fwd: NULL argument");
  TT_CHECK_ARG(n_sides >= 1 && n_sides <= TT_MAX_SIDES, "tt_embed_bag_fwd: n_sides=%d not in [1,%d]", n_sides, TT_MAX_SIDES);
  TT_CHECK_ARG(B >= 0 && table_rows >= 1 && table_rows <= INT32_MAX, "tt_embed_bag_fwd: bad B=%lld rows=%lld", (long long)B, (long long)table_rows);
  if (E % 4 != 0 || E < 4 || E > 256) return bag_unsupported("tt_embed_bag_fwd", "E must be a multiple of 4 in [4, 256]");
  if (!tt_aligned(table, 16)) return bag_unsupported("tt_embed_bag_fwd", "the table must be 16-byte aligned");
  BagSet a{};
  a.n = n_sides;
  a.E = E;
  a.C = (uint32_t)(E / 4);
  a.LG = pow2_at_least(a.C);
  int64_t slots = 0, positions = 0;
  for (int i = 0; i < n_sides; ++i) {
    const tt_bag_side& s = sides[i];
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
  bag_fwd_kernel<<<grid_for(ctx, slots * a.LG), kThreads, 0, reinterpret_cast<hipStream_t>(stream)>>>(a, table);
  TT_LAUNCH_CHECK();
  return TT_OK;
}

size_t tt_embed_bag_grad_workspace_bytes(int64_t nnz, int32_t E) { return grad_layout(nullptr, nnz > 0 ? nnz : 1, E > 0 ? E : 1).bytes; }

int tt_embed_bag_grad_bwd(tt_ctx* ctx, const tt_grad_src* srcs, int32_t n_srcs, int64_t B, int32_t E, const int32_t* bag_of,
                          const float* inv_len, const int32_t* sorted_src, const int32_t* seg_offsets, const int32_t* unique_rows,
                          const int32_t* n_unique, int64_t nnz, int32_t mode, float* out, void* workspace, size_t workspace_bytes,
                          tt_stream stream) {
  TT_CHECK_ARG(ctx && srcs && out, "tt_embed_bag_grad_bwd: NULL argument");
  TT_CHECK_ARG(n_srcs >= 1 && n_srcs <= TT_MAX_SIDES, "tt_embed_bag_grad_bwd: n_srcs=%d", n_srcs);
  TT_CHECK_ARG(mode >= TT_GRAD_SPARSE && mode <= TT_GRAD_DENSE_ACC, "tt_embed_bag_grad_bwd: bad mode %d (the PLANNED / DEFER_FINISH / SHORT forms are not offered)", mode);
  TT_CHECK_ARG(B >= 0 && nnz >= 0 && nnz < ((int64_t)1 << 31), "tt_embed_bag_grad_bwd: bad B / nnz");
  if (E % 4 != 0 || E < 4 || E > 256) return bag_unsupported("tt_embed_bag_grad_bwd", "E must be a multiple of 4 in [4, 256]");
  if (!tt_aligned(out, 16)) return bag_unsupported("tt_embed_bag_grad_bwd", "out must be 16-byte aligned");
  BagGradSet a{};
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
  const GradLayout gl = grad_layout(reinterpret_cast<char*>(workspace), nnz, E);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (int rc = tt_deferred_flush(ctx, TT_DQ_ALL)) return rc;      // the sources may be the products of a launch still queued
  const int g1 = grid_for(ctx, nnz * LG), g2 = grid_for(ctx, gl.max_chunks * LG), g3 = long_row_blocks(ctx, gl);
  const int dt = srcs[0].dtype;
  bag_zero_words_kernel<<<1, 64, 0, st>>>(gl.ws.counters, 2);
  TT_LAUNCH_CHECK();
  if (dt == TT_F32) bag_reduce_kernel<TT_F32><<<g1, kThreads, 0, st>>>(a, sorted_src, seg_offsets, unique_rows, n_unique, mode, out, gl.ws, LG);
  else bag_reduce_kernel<TT_BF16><<<g1, kThreads, 0, st>>>(a, sorted_src, seg_offsets, unique_rows, n_unique, mode, out, gl.ws, LG);
  TT_LAUNCH_CHECK();
  if (dt == TT_F32) bag_chunk_kernel<TT_F32><<<g2, kThreads, 0, st>>>(a, sorted_src, gl.ws, LG);
  else bag_chunk_kernel<TT_BF16><<<g2, kThreads, 0, st>>>(a, sorted_src, gl.ws, LG);
  TT_LAUNCH_CHECK();
  bag_long_finish_kernel<<<g3, kThreads, 0, st>>>(E, a.C, seg_offsets, unique_rows, mode, out, gl.ws, LG);
  TT_LAUNCH_CHECK();
  return TT_OK;
}

}  // extern "C"
