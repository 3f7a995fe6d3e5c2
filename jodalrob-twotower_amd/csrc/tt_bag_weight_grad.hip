// Gradients for the pooled lookup's per-id weights on gfx950, and learned position weights over them.
//   tt_embed_bag_weight_grad:   g[P] = c(slot of P) * < d_out[slot of P, :], table[row of P, :] >  for every position P of a bag plan
//   tt_bag_position_weights_*:  w[P] = param[pw_offset[k] + min(j, pw_len[k] - 1)] for position j of bag (b, k), and the sum of g
//                               over the positions that read each parameter element
// The kernels of tt_embed_bag.hip are not touched: these read what its forward left (rows, bag_of, inv_len) and write f32 per position.
#include "tt_bag_pw.h"
#include "tt_common.h"
#include "tt_deferred.h"
#include "tt_embed_slots.h"

namespace {

// ------------------------------------------------------------------------------------------------
// the per-id weight gradient.  Position space is walked flat: one lane group of LG lanes (the power of two >= E/4, as the pooled
// forward's) owns kWgBatch positions per trip, issues all their row and source loads, forms the lanes' partial dot products and
// then reduces each over the group with a fixed xor tree.  No atomics, no LDS.
// ------------------------------------------------------------------------------------------------
constexpr int kWgBatch = 4;

struct WGradSet {
  const char* d[TT_MAX_SIDES];
  float* g[TT_MAX_SIDES];          // NULL: the side is skipped -- nothing of it is read or written
  int64_t ld[TT_MAX_SIDES];
  uint32_t slot_base[TT_MAX_SIDES];
  uint32_t slots[TT_MAX_SIDES];    // B*K of the side
  uint32_t pos_base[TT_MAX_SIDES];
  uint32_t K[TT_MAX_SIDES];
  int32_t n;
  int32_t E;
  uint32_t C;
  uint32_t LG;
  uint32_t total_pos;
  int32_t table_rows;
  const int32_t* rows;
  const int32_t* bag_of;
  const float* inv_len;
};

template <int DT>
__global__ __launch_bounds__(kThreads) void bag_weight_grad_kernel(WGradSet a, const float* __restrict__ table) {
  constexpr int ESZ = DT == TT_F32 ? 4 : 2;
  const uint32_t LG = a.LG;
  const uint32_t gthread = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t lig = gthread & (LG - 1);
  const uint32_t ngroups = gridDim.x * blockDim.x / LG;
  const bool live = lig < a.C;
  // (uint64: base + the stride may pass 2^32 where total_pos is close to 2^31 * 2)
  for (uint64_t base = (uint64_t)(gthread / LG) * kWgBatch; base < a.total_pos; base += (uint64_t)ngroups * kWgBatch) {
    float* dst[kWgBatch];
    float c[kWgBatch];
    const float* xp[kWgBatch];
    const char* dp[kWgBatch];
#pragma unroll
    for (int j = 0; j < kWgBatch; ++j) {
      dst[j] = nullptr;
      xp[j] = nullptr;
      dp[j] = nullptr;
      c[j] = 0.f;
      const uint64_t P64 = base + j;
      if (P64 >= a.total_pos) continue;
      const uint32_t P = (uint32_t)P64;
      const char* sd = a.d[0];
      float* sg = a.g[0];
      int64_t ld = a.ld[0];
      uint32_t sb = a.slot_base[0], ns = a.slots[0], pb = 0, K = a.K[0];
#pragma unroll
      for (int t = 1; t < TT_MAX_SIDES; ++t) {
        const bool sel = t < a.n && P >= a.pos_base[t];
        sd = sel ? a.d[t] : sd;
        sg = sel ? a.g[t] : sg;
        ld = sel ? a.ld[t] : ld;
        sb = sel ? a.slot_base[t] : sb;
        ns = sel ? a.slots[t] : ns;
        pb = sel ? a.pos_base[t] : pb;
        K = sel ? a.K[t] : K;
      }
      if (!sg) continue;                                       // a side nobody asked for
      dst[j] = sg + (P - pb);
      const int32_t slot = a.bag_of[P];
      if (slot < 0) continue;                                  // no bag covers P: g = 0, nothing is read through rows[P]
      const uint32_t local = (uint32_t)slot - sb;              // (a slot of another side wraps to a huge value)
      const int32_t row = a.rows[P];
      if (local >= ns || (uint32_t)row >= (uint32_t)a.table_rows) continue;      // a plan that is not this call's: treated as uncovered
      const uint32_t b = local / K, k = local - b * K;
      c[j] = a.inv_len ? a.inv_len[slot] : 1.f;
      xp[j] = table + (int64_t)row * a.E + lig * 4;
      dp[j] = sd + ((int64_t)b * ld + (int64_t)(k * (uint32_t)a.E + lig * 4)) * ESZ;
    }
    float4 x[kWgBatch], d[kWgBatch];
#pragma unroll
    for (int j = 0; j < kWgBatch; ++j) {
      x[j] = make_float4(0.f, 0.f, 0.f, 0.f);
      d[j] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (live && xp[j]) {
        x[j] = *reinterpret_cast<const float4*>(xp[j]);
        if (DT == TT_F32) {
          d[j] = *reinterpret_cast<const float4*>(dp[j]);
        } else {
          const ushort4 t4 = *reinterpret_cast<const ushort4*>(dp[j]);
          d[j] = make_float4(tt_bf2f(t4.x), tt_bf2f(t4.y), tt_bf2f(t4.z), tt_bf2f(t4.w));
        }
      }
    }
    float p[kWgBatch];
#pragma unroll
    for (int j = 0; j < kWgBatch; ++j) {
      p[j] = __fmul_rn(d[j].x, x[j].x);
      p[j] = __fmaf_rn(d[j].y, x[j].y, p[j]);
      p[j] = __fmaf_rn(d[j].z, x[j].z, p[j]);
      p[j] = __fmaf_rn(d[j].w, x[j].w, p[j]);
    }
    // the group's sum: a fixed tree (lane l adds lane l ^ o for o = LG/2 .. 1; the lanes of a group run together)
    for (uint32_t o = LG >> 1; o > 0; o >>= 1) {
#pragma unroll
      for (int j = 0; j < kWgBatch; ++j) p[j] += __shfl_xor(p[j], (int)o);
    }
    if (lig == 0) {
#pragma unroll
      for (int j = 0; j < kWgBatch; ++j)
        if (dst[j]) *dst[j] = xp[j] ? __fmul_rn(c[j], p[j]) : 0.0f;
    }
  }
}

// ------------------------------------------------------------------------------------------------
// position weights
// ------------------------------------------------------------------------------------------------
struct PwSideDev {
  const int64_t* offs;
  const int32_t* pw_off;
  const int32_t* pw_len;
  float* w;                 // forward: the weights written; backward: the per-id gradient read
  int64_t nnz;
  uint32_t pos_base;
  uint32_t slots;
  int32_t K;
};
struct PwSet {
  PwSideDev s[TT_MAX_SIDES];
  int32_t n;
  uint32_t total_pos;
  int64_t n_param;
};

__global__ __launch_bounds__(kThreads) void bag_pw_fwd_kernel(PwSet a, const float* __restrict__ param) {
  for (uint32_t P = blockIdx.x * blockDim.x + threadIdx.x; P < a.total_pos; P += gridDim.x * blockDim.x) {
    int si = 0;
#pragma unroll
    for (int i = 1; i < TT_MAX_SIDES; ++i)
      if (i < a.n && P >= a.s[i].pos_base) si = i;
    const PwSideDev& s = a.s[si];
    const int64_t p = (int64_t)(P - s.pos_base);
    const uint32_t S = s.slots;
    float w = 1.0f;                                            // a position no bag covers, or a key without position weights
    uint32_t lo = 0, hi = S;                                   // the first slot whose end lies behind p
    while (lo < hi) {
      const uint32_t mid = (lo + hi) >> 1;
      if (s.offs[mid + 1] > p) hi = mid; else lo = mid + 1;
    }
    if (lo < S) {
      const int64_t o0 = s.offs[lo], o1 = s.offs[lo + 1];
      if (o0 >= 0 && o0 <= p && p < o1 && o1 <= s.nnz) {
        const int64_t e = pw_index(s.pw_off, s.pw_len, lo % (uint32_t)s.K, p - o0, a.n_param);      // (tt_bag_pw.h)
        if (e >= 0) w = param[e];
      }
    }
    s.w[p] = w;
  }
}

// one workgroup per parameter element: its threads stride over the samples of every key that reads the element, each adds its
// positions in ascending order, then a fixed tree over the workgroup.  The launch and the order depend on the shapes alone.
__global__ __launch_bounds__(kThreads) void bag_pw_bwd_kernel(PwSet a, float* __restrict__ d_param, uint32_t B) {
  __shared__ float sh[kThreads];
  const int64_t e = blockIdx.x;
  float acc = 0.f;
  for (int si = 0; si < a.n; ++si) {
    const PwSideDev& s = a.s[si];
    if (!s.w) continue;
    for (uint32_t k = 0; k < (uint32_t)s.K; ++k) {
      const int32_t off = s.pw_off[k], len = s.pw_len[k];
      if (off < 0 || len < 1 || e < off || e >= (int64_t)off + len) continue;
      const int64_t j = e - off;
      for (uint32_t b = threadIdx.x; b < B; b += kThreads) {
        const uint32_t slot = b * (uint32_t)s.K + k;
        const int64_t o0 = s.offs[slot], o1 = s.offs[slot + 1];
        if (o0 < 0 || o1 < o0 || o1 > s.nnz) continue;         // a pair the lookup refused
        // the element's positions: j alone, or for the key's last element every position from j on
        const int64_t q1 = j < len - 1 ? (o0 + j + 1 < o1 ? o0 + j + 1 : o1) : o1;
        for (int64_t q = o0 + j; q < q1; ++q) acc += s.w[q];
      }
    }
  }
  sh[threadIdx.x] = acc;
  __syncthreads();
#pragma unroll
  for (int o = kThreads / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) d_param[e] = sh[0];
}

static int wg_unsupported(const char* who, const char* what) {
  tt_set_error("%s: %s", who, what);
  return TT_ERR_UNSUPPORTED;
}

static int pw_args(const char* who, const tt_bag_pw_side* sides, int32_t n_sides, int64_t B, int64_t n_param, bool fwd, PwSet* out) {
  TT_CHECK_ARG(sides, "%s: NULL argument", who);
  TT_CHECK_ARG(n_sides >= 1 && n_sides <= TT_MAX_SIDES, "%s: n_sides=%d not in [1,%d]", who, n_sides, TT_MAX_SIDES);
  TT_CHECK_ARG(B >= 0 && n_param >= 1 && n_param < ((int64_t)1 << 31), "%s: bad B=%lld n_param=%lld", who, (long long)B, (long long)n_param);
  PwSet a{};
  a.n = n_sides;
  a.n_param = n_param;
  int64_t positions = 0;
  for (int i = 0; i < n_sides; ++i) {
    const tt_bag_pw_side& s = sides[i];
    TT_CHECK_ARG(s.K >= 1 && s.nnz >= 0 && B * s.K < ((int64_t)1 << 31), "%s: side %d has K=%d nnz=%lld", who, i, s.K, (long long)s.nnz);
    TT_CHECK_ARG(s.offsets && s.pw_offset && s.pw_len, "%s: side %d has NULL pointers", who, i);
    TT_CHECK_ARG(s.w || (!fwd) || s.nnz == 0, "%s: side %d has no output", who, i);
    if (!tt_aligned(s.w, 4)) return wg_unsupported(who, "the per-position buffers must be 4-byte aligned");
    a.s[i] = PwSideDev{s.offsets, s.pw_offset, s.pw_len, s.w, s.nnz, (uint32_t)positions, (uint32_t)(B * s.K), s.K};
    positions += s.nnz;
  }
  TT_CHECK_ARG(positions < ((int64_t)1 << 31), "%s: %lld ids exceed the 2^31 index range", who, (long long)positions);
  a.total_pos = (uint32_t)positions;
  *out = a;
  return TT_OK;
}

}  // namespace

extern "C" {

int tt_embed_bag_weight_grad(tt_ctx* ctx, const float* table, int64_t table_rows, int32_t E, const tt_grad_src* srcs, int32_t n_sides,
                             int64_t B, const int32_t* rows, const int32_t* bag_of, const float* inv_len, const int64_t* side_nnz,
                             float* const* g_out, tt_stream stream) {
  TT_CHECK_ARG(ctx && table && srcs && side_nnz && g_out, "tt_embed_bag_weight_grad: NULL argument");
  TT_CHECK_ARG(n_sides >= 1 && n_sides <= TT_MAX_SIDES, "tt_embed_bag_weight_grad: n_sides=%d not in [1,%d]", n_sides, TT_MAX_SIDES);
  TT_CHECK_ARG(B >= 0 && table_rows >= 1 && table_rows <= INT32_MAX, "tt_embed_bag_weight_grad: bad B=%lld rows=%lld", (long long)B,
               (long long)table_rows);
  if (E % 4 != 0 || E < 4 || E > 256) return wg_unsupported("tt_embed_bag_weight_grad", "E must be a multiple of 4 in [4, 256]");
  if (!tt_aligned(table, 16)) return wg_unsupported("tt_embed_bag_weight_grad", "the table must be 16-byte aligned");
  WGradSet a{};
  a.n = n_sides;
  a.E = E;
  a.C = (uint32_t)(E / 4);
  a.LG = pow2_at_least(a.C);
  int64_t slots = 0, positions = 0;
  int dt = -1;                                                 // the requested sides' source dtype
  for (int i = 0; i < n_sides; ++i) {
    const tt_grad_src& s = srcs[i];
    TT_CHECK_ARG(s.K >= 1 && side_nnz[i] >= 0, "tt_embed_bag_weight_grad: side %d has K=%d nnz=%lld", i, s.K, (long long)side_nnz[i]);
    a.g[i] = side_nnz[i] > 0 ? g_out[i] : nullptr;
    if (a.g[i]) {                                              // (a skipped side's source is not looked at)
      TT_CHECK_ARG(s.d_out, "tt_embed_bag_weight_grad: side %d has no source", i);
      TT_CHECK_ARG(s.dtype == TT_F32 || s.dtype == TT_BF16, "tt_embed_bag_weight_grad: side %d bad dtype", i);
      TT_CHECK_ARG(dt < 0 || s.dtype == dt, "tt_embed_bag_weight_grad: all sources must share one dtype (side %d differs)", i);
      TT_CHECK_ARG(s.ld >= (int64_t)s.K * E, "tt_embed_bag_weight_grad: side %d ld %lld < K*E", i, (long long)s.ld);
      const size_t esz = s.dtype == TT_BF16 ? 2 : 4;
      if (s.ld % 4 != 0 || !tt_aligned(s.d_out, 4 * esz)) return wg_unsupported("tt_embed_bag_weight_grad", "sources must be 4-element aligned (base and ld)");
      if (!tt_aligned(a.g[i], 4)) return wg_unsupported("tt_embed_bag_weight_grad", "the outputs must be 4-byte aligned");
      dt = s.dtype;
    }
    a.d[i] = reinterpret_cast<const char*>(s.d_out);
    a.ld[i] = s.ld;
    a.K[i] = (uint32_t)s.K;
    a.slots[i] = (uint32_t)(B * s.K);
    a.slot_base[i] = (uint32_t)slots;
    a.pos_base[i] = (uint32_t)positions;
    slots += B * s.K;
    positions += side_nnz[i];
    TT_CHECK_ARG(slots < ((int64_t)1 << 31) && positions < ((int64_t)1 << 31), "tt_embed_bag_weight_grad: too many slots / ids");
  }
  if (dt < 0 || positions == 0 || slots == 0) return TT_OK;
  TT_CHECK_ARG(rows && bag_of, "tt_embed_bag_weight_grad: NULL rows / bag_of");
  a.total_pos = (uint32_t)positions;
  a.table_rows = (int32_t)table_rows;
  a.rows = rows;
  a.bag_of = bag_of;
  a.inv_len = inv_len;
  if (int rc = tt_deferred_flush(ctx, TT_DQ_ALL)) return rc;      // the sources may be the products of a launch still queued
  const int grid = grid_for(ctx, tt_cdiv(positions, kWgBatch) * a.LG);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (dt == TT_F32) bag_weight_grad_kernel<TT_F32><<<grid, kThreads, 0, st>>>(a, table);
  else bag_weight_grad_kernel<TT_BF16><<<grid, kThreads, 0, st>>>(a, table);
  TT_LAUNCH_CHECK();
  return TT_OK;
}

int tt_bag_position_weights_fwd(tt_ctx* ctx, const float* param, int64_t n_param, const tt_bag_pw_side* sides, int32_t n_sides, int64_t B,
                                tt_stream stream) {
  TT_CHECK_ARG(ctx && param, "tt_bag_position_weights_fwd: NULL argument");
  PwSet a;
  if (int rc = pw_args("tt_bag_position_weights_fwd", sides, n_sides, B, n_param, true, &a)) return rc;
  if (a.total_pos == 0) return TT_OK;
  bag_pw_fwd_kernel<<<grid_for(ctx, a.total_pos), kThreads, 0, reinterpret_cast<hipStream_t>(stream)>>>(a, param);
  TT_LAUNCH_CHECK();
  return TT_OK;
}

int tt_bag_position_weights_bwd(tt_ctx* ctx, float* d_param, int64_t n_param, const tt_bag_pw_side* sides, int32_t n_sides, int64_t B,
                                tt_stream stream) {
  TT_CHECK_ARG(ctx && d_param, "tt_bag_position_weights_bwd: NULL argument");
  PwSet a;
  if (int rc = pw_args("tt_bag_position_weights_bwd", sides, n_sides, B, n_param, false, &a)) return rc;
  bag_pw_bwd_kernel<<<(int)n_param, kThreads, 0, reinterpret_cast<hipStream_t>(stream)>>>(a, d_param, (uint32_t)B);
  TT_LAUNCH_CHECK();
  return TT_OK;
}

}  // extern "C"
