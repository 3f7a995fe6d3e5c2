// The optimisers on gfx950: Adam over dense tensors, Adam and row-wise Adagrad over the looked-up table rows, and the fused
// launch that runs the towers' Adam, a row rule and -- when the gradient reduction deferred it -- the long rows' finish in one
// grid.  Shares the row mapping (tt_embed_slots.h) and the reduction's workspace and finish body (tt_grad_ws.h).
#include "tt_common.h"
#include "tt_deferred.h"
#include "tt_embed_slots.h"
#include "tt_grad_ws.h"

namespace {

// ------------------------------------------------------------------------------------------------
// a17: Adam
// ------------------------------------------------------------------------------------------------
struct AdamK {
  float lr_over_bc1, inv_sqrt_bc2, b1, b2, eps, wd;
  const float* dev;   // optional device copy of the six scalars above (graph replay)
};

__device__ __forceinline__ AdamK adam_resolve(const AdamK& k) {
  if (k.dev == nullptr) return k;
  AdamK r;
  r.lr_over_bc1 = k.dev[0]; r.inv_sqrt_bc2 = k.dev[1]; r.b1 = k.dev[2]; r.b2 = k.dev[3]; r.eps = k.dev[4]; r.wd = k.dev[5];
  r.dev = nullptr;
  return r;
}

__device__ __forceinline__ void adam1(float& p, float g, float& m, float& v, const AdamK& k) {
  // explicit fused multiply-adds: left to the compiler, the contraction of a * b + c * d differs from one inlining context
  // to the next (the float4 row path and the scalar long-row path of the fused launch disagreed in the last bit)
  g = k.wd != 0.f ? __builtin_fmaf(k.wd, p, g) : g;
  m = __builtin_fmaf(k.b1, m, (1.f - k.b1) * g);
  v = __builtin_fmaf(k.b2, v, (1.f - k.b2) * g * g);
  const float denom = __builtin_fmaf(sqrtf(v), k.inv_sqrt_bc2, k.eps);
  p = __builtin_fmaf(-k.lr_over_bc1, m / denom, p);
}

__global__ __launch_bounds__(kThreads) void adam_dense_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                             float* __restrict__ m, float* __restrict__ v, int64_t n, AdamK k0) {
  const AdamK k = adam_resolve(k0);
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    float pp = p[i], mm = m[i], vv = v[i];
    adam1(pp, g[i], mm, vv, k);
    p[i] = pp; m[i] = mm; v[i] = vv;
  }
}

__global__ __launch_bounds__(kThreads) void adam_dense_vec4_kernel(float4* __restrict__ p, const float4* __restrict__ g,
                                                                  float4* __restrict__ m, float4* __restrict__ v, int64_t n4, AdamK k0) {
  const AdamK k = adam_resolve(k0);
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    float4 pp = p[i], mm = m[i], vv = v[i];
    const float4 gg = g[i];
    adam1(pp.x, gg.x, mm.x, vv.x, k); adam1(pp.y, gg.y, mm.y, vv.y, k);
    adam1(pp.z, gg.z, mm.z, vv.z, k); adam1(pp.w, gg.w, mm.w, vv.w, k);
    p[i] = pp; m[i] = mm; v[i] = vv;
  }
}

constexpr int kAdamMulti = 32;
struct AdamMultiArgs {
  tt_adam_tensor t[kAdamMulti];
};

__global__ __launch_bounds__(kThreads) void adam_multi_kernel(AdamMultiArgs a, AdamK k0) {
  const AdamK k = adam_resolve(k0);
  const tt_adam_tensor& t = a.t[blockIdx.y];
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < t.n; i += stride) {
    float pp = t.p[i], mm = t.m[i], vv = t.v[i];
    adam1(pp, t.g[i], mm, vv, k);
    t.p[i] = pp; t.m[i] = mm; t.v[i] = vv;
  }
}

// the update of one table row by its LG lanes (lig = lane in group); g: the row's gradient; w / m / v: the [R, E] weights and
// moments, the row starts at element `off` of each (one offset for the three, as they share a layout)
template <int VEC>
__device__ __forceinline__ void adam_row(float* __restrict__ w, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                         int64_t off, uint32_t C, uint32_t LG, uint32_t lig, const AdamK& k) {
  for (uint32_t chunk = lig; chunk < C; chunk += LG) {
    const int64_t o = off + chunk * VEC;
    if constexpr (VEC == 4) {
      float4 pp = *reinterpret_cast<float4*>(w + o), mm = *reinterpret_cast<float4*>(m + o), vv = *reinterpret_cast<float4*>(v + o);
      const float4 gg = *reinterpret_cast<const float4*>(g + chunk * VEC);
      adam1(pp.x, gg.x, mm.x, vv.x, k); adam1(pp.y, gg.y, mm.y, vv.y, k);
      adam1(pp.z, gg.z, mm.z, vv.z, k); adam1(pp.w, gg.w, mm.w, vv.w, k);
      *reinterpret_cast<float4*>(w + o) = pp;
      *reinterpret_cast<float4*>(m + o) = mm;
      *reinterpret_cast<float4*>(v + o) = vv;
    } else {
      float pp = w[o], mm = m[o], vv = v[o];
      adam1(pp, g[chunk], mm, vv, k);
      w[o] = pp; m[o] = mm; v[o] = vv;
    }
  }
}

// dense tensors + the looked-up table rows in ONE launch: blocks [0, nd) walk the dense tensors (prefix table),
// the rest are the row-sparse update (every small launch in the step's dependent chain costs ~5 us)
struct AdamFusedArgs {
  tt_adam_tensor t[kAdamMulti];
  int32_t blk0[kAdamMulti + 1];   // first block of dense tensor i; blk0[n] = nd
  int32_t n;
};

// the dense-tensor role of block `bid` < nd: find its tensor in the prefix table, stride over it with the tensor's blocks
__device__ __forceinline__ void adam_dense_role(const AdamFusedArgs& a, int bid, const AdamK& k) {
  int ti = 0;
  for (int i = 1; i < a.n; ++i)
    if (bid >= a.blk0[i]) ti = i;
  const tt_adam_tensor t = a.t[ti];
  const int64_t nb = a.blk0[ti + 1] - a.blk0[ti];
  const int64_t stride = nb * role_threads();
  for (int64_t i = (int64_t)(bid - a.blk0[ti]) * role_threads() + threadIdx.x; i < t.n; i += stride) {
    float pp = t.p[i], mm = t.m[i], vv = t.v[i];
    adam1(pp, t.g[i], mm, vv, k);
    t.p[i] = pp; t.m[i] = mm; t.v[i] = vv;
  }
}

// ------------------------------------------------------------------------------------------------
// a17b: row-wise Adagrad (one f32 accumulator per table row)
//   g' = g + wd * w;  s += sum_j g'_j^2 / E;  w -= lr / (sqrt(s) + eps) * g'
// A row is owned by LG lanes of one wave (LG a power of two <= 64, the adam_sparse_kernel mapping); each lane holds its
// chunks of g' in registers, the row's sum of squares is formed lane-locally in chunk order and then by an xor butterfly
// over the LG lanes (no LDS, no atomics).  Every lane of the group ends with the same bits, so any lane may write s.
// ------------------------------------------------------------------------------------------------
struct AdagradK {
  float lr, eps, wd;
  const float* dev;   // optional device copy of the three scalars above (graph replay): [0] lr [1] eps [2] wd
};

__device__ __forceinline__ AdagradK adagrad_resolve(const AdagradK& k) {
  if (k.dev == nullptr) return k;
  AdagradK r;
  r.lr = k.dev[0]; r.eps = k.dev[1]; r.wd = k.dev[2];
  r.dev = nullptr;
  return r;
}

constexpr int kAdagradMaxChunks = 4;   // chunks of one row per lane: E <= 4 * 64 * VEC

// the update of one table row by its LG lanes (lig = lane in group); g: the row's gradient, w: its weights, s: its accumulator
template <int VEC>
__device__ __forceinline__ void adagrad_row(float* __restrict__ w, const float* __restrict__ g, float* __restrict__ s, int32_t E,
                                            uint32_t C, uint32_t LG, uint32_t lig, const AdagradK& k) {
  float gp[kAdagradMaxChunks][VEC], wp[kAdagradMaxChunks][VEC];
  float sq = 0.f;
#pragma unroll
  for (int c = 0; c < kAdagradMaxChunks; ++c) {
    const uint32_t chunk = lig + (uint32_t)c * LG;
    if (chunk < C) {
      if constexpr (VEC == 4) {
        const float4 gg = *reinterpret_cast<const float4*>(g + chunk * 4);
        const float4 ww = *reinterpret_cast<const float4*>(w + chunk * 4);
        gp[c][0] = gg.x; gp[c][1] = gg.y; gp[c][2] = gg.z; gp[c][3] = gg.w;
        wp[c][0] = ww.x; wp[c][1] = ww.y; wp[c][2] = ww.z; wp[c][3] = ww.w;
      } else {
        gp[c][0] = g[chunk];
        wp[c][0] = w[chunk];
      }
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        gp[c][e] = k.wd != 0.f ? __builtin_fmaf(k.wd, wp[c][e], gp[c][e]) : gp[c][e];
        sq = __builtin_fmaf(gp[c][e], gp[c][e], sq);
      }
    }
  }
  for (uint32_t off = LG >> 1; off >= 1; off >>= 1) sq += __shfl_xor(sq, (int)off, 64);
  const float snew = *s + sq / (float)E;
  const float step = k.lr / (sqrtf(snew) + k.eps);
#pragma unroll
  for (int c = 0; c < kAdagradMaxChunks; ++c) {
    const uint32_t chunk = lig + (uint32_t)c * LG;
    if (chunk < C) {
#pragma unroll
      for (int e = 0; e < VEC; ++e) wp[c][e] = __builtin_fmaf(-step, gp[c][e], wp[c][e]);
      if constexpr (VEC == 4) *reinterpret_cast<float4*>(w + chunk * 4) = make_float4(wp[c][0], wp[c][1], wp[c][2], wp[c][3]);
      else w[chunk] = wp[c][0];
    }
  }
  if (lig == 0) *s = snew;
}

// ------------------------------------------------------------------------------------------------
// a17c: the row rules and the launches built from them
// A row rule is what an optimiser does to one looked-up table row: its state, its hyper-parameters (resolve() once per
// thread, before anything else; it is handed the towers' Adam set), row() for a row whose gradient is complete in grad_rows,
// and the two long_rows_finish hooks for a row whose gradient the long-row blocks are still adding up (long_col: EMIT, one
// finished column, already stored to grad_rows; long_done: DONE; `row` may be a routing pad there: >= table_rows).
// The rule types are plain structs, not templates: tools/bench_table_optimizer.py reads them out of the kernel names.
// ------------------------------------------------------------------------------------------------
struct AdamRows {
  float* m;   // [R, E] moments
  float* v;
  AdamK k;    // the towers' set: the fused Adam launch has one (the host leaves it empty)
  __device__ __forceinline__ void resolve(const AdamK& towers) { k = adam_resolve(towers); }
  template <int VEC>
  __device__ __forceinline__ void row(float* __restrict__ table, int64_t row, const float* __restrict__ g, int32_t E, uint32_t C,
                                      uint32_t LG, uint32_t lig) const {
    adam_row<VEC>(table, g, m, v, row * E, C, LG, lig, k);
  }
  // EMIT: each column is applied by the thread that finished it
  __device__ __forceinline__ void long_col(float* __restrict__ table, int64_t row, int64_t table_rows, int32_t E, int32_t col,
                                           float tot) const {
    if (row >= table_rows) return;
    const int64_t o = row * E + col;
    float pp = table[o], mm = m[o], vv = v[o];
    adam1(pp, tot, mm, vv, k);
    table[o] = pp; m[o] = mm; v[o] = vv;
  }
  // DONE: nothing left to do (NoRowDone)
  template <int VEC>
  __device__ __forceinline__ void long_done(float*, int64_t, int64_t, int32_t, uint32_t, uint32_t) const {}
};

struct AdagradRows {
  float* sum;   // [R] accumulators
  AdagradK k;
  __device__ __forceinline__ void resolve(const AdamK&) { k = adagrad_resolve(k); }
  template <int VEC>
  __device__ __forceinline__ void row(float* __restrict__ table, int64_t row, const float* __restrict__ g, int32_t E, uint32_t C,
                                      uint32_t LG, uint32_t lig) const {
    adagrad_row<VEC>(table + row * E, g, sum + row, E, C, LG, lig, k);
  }
  // the long row's gradient as the workgroup finishes it (only launches that call the hooks carry it)
  static __device__ __forceinline__ float* row_copy() {
    __shared__ __attribute__((aligned(16))) float rowg[kFinishMaxFloats / 4];   // E <= kFinishMaxFloats * LG / kThreads <= 1024
    return rowg;
  }
  // EMIT: the column goes into the LDS copy of the row
  __device__ __forceinline__ void long_col(float*, int64_t, int64_t, int32_t, int32_t col, float tot) const { row_copy()[col] = tot; }
  // DONE: all E columns exist: the block's first LG lanes apply adagrad_row from the copy -- the same values and the same
  // reduction order as the row blocks
  template <int VEC>
  __device__ __forceinline__ void long_done(float* __restrict__ table, int64_t row, int64_t table_rows, int32_t E, uint32_t C,
                                            uint32_t LG) const {
    if (threadIdx.x < LG && row < table_rows) adagrad_row<VEC>(table + row * E, row_copy(), sum + row, E, C, LG, threadIdx.x, k);
  }
};

// the row-sparse update over the looked-up rows; LONG_SKIP: rows whose segment is longer than kLongSeg are left to the
// long-row workgroups of the fused finish launch.  `first` blocks of the grid belong to other roles.
template <int VEC, bool LONG_SKIP, typename RULE>
__device__ __forceinline__ void sparse_rows(const RULE& r, float* __restrict__ table, int32_t E, uint32_t C,
                                            const int32_t* __restrict__ unique_rows, const float* __restrict__ grad_rows,
                                            const int32_t* __restrict__ n_unique, uint32_t LG, int64_t table_rows,
                                            const int32_t* __restrict__ seg, uint32_t first) {
  const uint32_t U = (uint32_t)*n_unique;
  const uint32_t gthread = (blockIdx.x - first) * role_threads() + threadIdx.x;
  const uint32_t lig = gthread % LG;
  const uint32_t ngroups = (gridDim.x - first) * role_threads() / LG;
  for (uint32_t u = gthread / LG; u < U; u += ngroups) {
    const int64_t row = unique_rows[u];
    if (row >= table_rows) continue;                   // routing pad (multi-GPU fixed-capacity buckets)
    if (LONG_SKIP && seg[u + 1] - seg[u] > kLongSeg) continue;   // finished and applied by the long-row blocks
    r.template row<VEC>(table, row, grad_rows + (int64_t)u * E, E, C, LG, lig);
  }
}

template <int VEC>
__global__ __launch_bounds__(kThreads) void adam_sparse_kernel(float* __restrict__ table, float* __restrict__ m, float* __restrict__ v,
                                                              int32_t E, uint32_t C, const int32_t* __restrict__ unique_rows,
                                                              const float* __restrict__ grad_rows, const int32_t* __restrict__ n_unique,
                                                              AdamK k0, uint32_t LG, int64_t table_rows) {
  const AdamRows r{m, v, adam_resolve(k0)};
  sparse_rows<VEC, false>(r, table, E, C, unique_rows, grad_rows, n_unique, LG, table_rows, nullptr, 0);
}

template <int VEC>
__global__ __launch_bounds__(kThreads) void adagrad_sparse_kernel(float* __restrict__ table, float* __restrict__ sum, int32_t E, uint32_t C,
                                                                 const int32_t* __restrict__ unique_rows,
                                                                 const float* __restrict__ grad_rows, const int32_t* __restrict__ n_unique,
                                                                 AdagradK k0, uint32_t LG, int64_t table_rows) {
  const AdagradRows r{sum, adagrad_resolve(k0)};
  sparse_rows<VEC, false>(r, table, E, C, unique_rows, grad_rows, n_unique, LG, table_rows, nullptr, 0);
}

// dense gradient mode: every row of the [R, E] store
template <int VEC>
__global__ __launch_bounds__(kThreads) void adagrad_dense_kernel(float* __restrict__ table, float* __restrict__ sum,
                                                                const float* __restrict__ grad, int64_t R, int32_t E, uint32_t C,
                                                                AdagradK k0, uint32_t LG) {
  const AdagradK k = adagrad_resolve(k0);
  const uint64_t gthread = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t lig = (uint32_t)(gthread % LG);
  const uint64_t ngroups = (uint64_t)gridDim.x * blockDim.x / LG;
  for (uint64_t r = gthread / LG; r < (uint64_t)R; r += ngroups)
    adagrad_row<VEC>(table + (int64_t)r * E, grad + (int64_t)r * E, sum + r, E, C, LG, lig, k);
}

// the towers' Adam + the looked-up table rows under RULE in ONE launch (AdagradRows brings a hyper-parameter set of its own; a
// block resolves the one set its role needs: two device-scalar reads in a row are two memory latencies).  Blocks [0, nd): the dense tensors.  LONG: the gradient reduction left its long rows unfinished
// (TT_GRAD_DEFER_FINISH): blocks [nd, nd + nlb) add a long row's chunk partials exactly as seg_long_finish_kernel does, store
// the sum into grad_rows and update that table row through the rule's hooks; the row blocks behind them skip those rows.  One
// launch fewer in the step's dependent chain, the same values as the separate entries.
template <typename RULE, int VEC, bool LONG>
__global__ __launch_bounds__(kThreads) void fused_step_kernel(AdamFusedArgs a, AdamK ak0, RULE r, float* __restrict__ table, int32_t E,
                                                             uint32_t C, const int32_t* __restrict__ unique_rows,
                                                             float* __restrict__ grad_rows, const int32_t* __restrict__ n_unique,
                                                             uint32_t LG, int64_t table_rows, const int32_t* __restrict__ seg, GradWs ws,
                                                             int nlb) {
  const int nd = a.blk0[a.n];
  if ((int)blockIdx.x < nd) {
    adam_dense_role(a, (int)blockIdx.x, adam_resolve(ak0));
    return;
  }
  r.resolve(ak0);
  const int first = nd + (LONG ? nlb : 0);
  if (LONG && (int)blockIdx.x < first) {
    __shared__ float part[kFinishMaxFloats];
    long_rows_finish<VEC>(E, C, seg, ws, LG, blockIdx.x - nd, (uint32_t)nlb, part, [&](int32_t u, int32_t col, float tot) {
      grad_rows[(int64_t)u * E + col] = tot;
      r.long_col(table, unique_rows[u], table_rows, E, col, tot);
    }, [&](int32_t u) { r.template long_done<VEC>(table, unique_rows[u], table_rows, E, C, LG); });
    return;
  }
  sparse_rows<VEC, LONG>(r, table, E, C, unique_rows, grad_rows, n_unique, LG, table_rows, seg, (uint32_t)first);
}

// ------------------------------------------------------------------------------------------------
// host helpers
// ------------------------------------------------------------------------------------------------
AdamK make_adam(int64_t step, float lr, float b1, float b2, float eps, float wd, const float* dev) {
  const double bc1 = 1.0 - pow((double)b1, (double)step);
  const double bc2 = 1.0 - pow((double)b2, (double)step);
  AdamK k;
  k.lr_over_bc1 = (float)((double)lr / bc1);
  k.inv_sqrt_bc2 = (float)(1.0 / sqrt(bc2));
  k.b1 = b1; k.b2 = b2; k.eps = eps; k.wd = wd;
  k.dev = dev;
  return k;
}

// ---- optimiser launches ----
// (every optimiser entry starts with tt_deferred_flush(ctx, TT_DQ_ALL), before it looks at its arguments: a queued compaction's rows
// are read here, and the gradients are not complete before a queued score backward and slab reduction)
AdagradK make_adagrad(float lr, float eps, float wd, const float* dev) {
  AdagradK k;
  k.lr = lr; k.eps = eps; k.wd = wd;
  k.dev = dev;
  return k;
}

// adagrad_row holds a lane's chunks of the row in registers: false (error set) when a lane would own more than it holds
bool adagrad_fits(const char* who, int32_t E, uint32_t C, uint32_t LG) {
  if (C > (uint32_t)kAdagradMaxChunks * LG) {
    tt_set_error("%s: E=%d too wide (max %d, or %d when E %% 4 != 0)", who, E, kAdagradMaxChunks * 64 * 4, kAdagradMaxChunks * 64);
    return false;
  }
  return true;
}

// ---- the towers' Adam + the looked-up rows under a row rule, one launch ----
// what the host asks of a rule: is its state there, does it allow float4 rows, does the row fit its row()
bool rule_state(const AdamRows& r) { return r.m && r.v; }
bool rule_state(const AdagradRows& r) { return r.sum != nullptr; }
bool rule_vec4(const AdamRows& r) { return tt_aligned(r.m, 16) && tt_aligned(r.v, 16); }
bool rule_vec4(const AdagradRows&) { return true; }      // (one accumulator per row: no vector access to it)
bool rule_fits(const AdamRows&, const char*, int32_t, uint32_t, uint32_t) { return true; }
bool rule_fits(const AdagradRows&, const char* who, int32_t E, uint32_t C, uint32_t LG) { return adagrad_fits(who, E, C, LG); }

// grad_workspace != NULL: the reduction's deferred finish (tt_embed_grad_bwd with TT_GRAD_DEFER_FINISH) rides in this launch
template <typename RULE>
int fused_step_impl(tt_ctx* ctx, const char* who, const tt_adam_tensor* tensors, int32_t n_tensors, int64_t step, const AdamK& ak,
                           const RULE& rule, float* table, int64_t table_rows, int32_t E, const int32_t* unique_rows, float* grad_rows,
                           const int32_t* n_unique, int64_t M, const int32_t* seg_offsets, void* grad_workspace,
                           size_t grad_workspace_bytes, tt_stream stream) {
  if (int rc = tt_deferred_flush(ctx, TT_DQ_ALL)) return rc;
  TT_CHECK_ARG(ctx && tensors && table && rule_state(rule) && unique_rows && grad_rows && n_unique, "%s: NULL argument", who);
  TT_CHECK_ARG(n_tensors >= 1 && n_tensors <= kAdamMulti, "%s: n_tensors=%d not in [1,%d]", who, n_tensors, kAdamMulti);
  TT_CHECK_ARG(step >= 1 && E >= 1 && M >= 1 && table_rows >= 1, "%s: bad step/E/M/table_rows", who);
  AdamFusedArgs a{};
  a.n = n_tensors;
  int nd = 0;
  for (int i = 0; i < n_tensors; ++i) {
    const tt_adam_tensor& t = tensors[i];
    TT_CHECK_ARG(t.n >= 0 && (t.n == 0 || (t.p && t.g && t.m && t.v)), "%s: tensor %d has NULL pointers", who, i);
    a.t[i] = t;
    a.blk0[i] = nd;
    int64_t nb = tt_cdiv(t.n > 0 ? t.n : 1, kThreads);
    nd += (int)(nb > 64 ? 64 : nb);
  }
  a.blk0[n_tensors] = nd;
  const bool vec4 = (E % 4 == 0) && tt_aligned(table, 16) && rule_vec4(rule) && tt_aligned(grad_rows, 16);
  uint32_t C, LG;
  row_mapping(E, vec4, &C, &LG);
  if (!rule_fits(rule, who, E, C, LG)) return TT_ERR_UNSUPPORTED;
  GradWs ws{};
  int nlb = 0;
  if (grad_workspace) {
    TT_CHECK_ARG(seg_offsets, "%s: NULL seg_offsets", who);
    if (grad_workspace_bytes < tt_embed_grad_workspace_bytes(M, E)) {
      tt_set_error("%s: gradient workspace %zu < required %zu", who, grad_workspace_bytes, tt_embed_grad_workspace_bytes(M, E));
      return TT_ERR_WORKSPACE;
    }
    if ((int64_t)(kThreads / LG) * E > kFinishMaxFloats) {
      tt_set_error("%s: E=%d too wide for the long-row finish (max %d)", who, E, kFinishMaxFloats * (int)LG / kThreads);
      return TT_ERR_UNSUPPORTED;
    }
    const GradLayout gl = grad_layout(reinterpret_cast<char*>(grad_workspace), M, E);
    ws = gl.ws;
    nlb = long_row_blocks(ctx, gl);
  }
  const int grid = nd + nlb + grid_for(ctx, M * LG);
  auto launch = [&](auto kernel) {
    kernel<<<grid, kThreads, 0, reinterpret_cast<hipStream_t>(stream)>>>(a, ak, rule, table, E, C, unique_rows, grad_rows, n_unique, LG,
                                                                         table_rows, seg_offsets, ws, nlb);
  };
  if (grad_workspace) vec4 ? launch(fused_step_kernel<RULE, 4, true>) : launch(fused_step_kernel<RULE, 1, true>);
  else vec4 ? launch(fused_step_kernel<RULE, 4, false>) : launch(fused_step_kernel<RULE, 1, false>);
  TT_LAUNCH_CHECK();
  return TT_OK;
}

}  // namespace

extern "C" {

void tt_adam_hparams(int64_t step, float lr, float beta1, float beta2, float eps, float weight_decay, float out6[6]) {
  const AdamK k = make_adam(step < 1 ? 1 : step, lr, beta1, beta2, eps, weight_decay, nullptr);
  out6[0] = k.lr_over_bc1; out6[1] = k.inv_sqrt_bc2; out6[2] = k.b1; out6[3] = k.b2; out6[4] = k.eps; out6[5] = k.wd;
}

int tt_adam_dense_step(tt_ctx* ctx, float* p, const float* g, float* m, float* v, int64_t n, int64_t step, float lr, float beta1,
                       float beta2, float eps, float weight_decay, const float* hparams_dev, tt_stream stream) {
  if (int rc = tt_deferred_flush(ctx, TT_DQ_ALL)) return rc;
  TT_CHECK_ARG(ctx && (n == 0 || (p && g && m && v)), "tt_adam_dense_step: NULL argument");
  TT_CHECK_ARG(step >= 1 && n >= 0, "tt_adam_dense_step: step must be >= 1");
  if (n == 0) return TT_OK;
  const AdamK k = make_adam(step, lr, beta1, beta2, eps, weight_decay, hparams_dev);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (n % 4 == 0 && tt_aligned(p, 16) && tt_aligned(g, 16) && tt_aligned(m, 16) && tt_aligned(v, 16)) {
    adam_dense_vec4_kernel<<<grid_for(ctx, n / 4), kThreads, 0, st>>>(reinterpret_cast<float4*>(p), reinterpret_cast<const float4*>(g),
                                                                      reinterpret_cast<float4*>(m), reinterpret_cast<float4*>(v), n / 4, k);
  } else {
    adam_dense_kernel<<<grid_for(ctx, n), kThreads, 0, st>>>(p, g, m, v, n, k);
  }
  TT_LAUNCH_CHECK();
  return TT_OK;
}

int tt_adam_multi_step(tt_ctx* ctx, const tt_adam_tensor* tensors, int32_t n_tensors, int64_t step, float lr, float beta1,
                       float beta2, float eps, float weight_decay, const float* hparams_dev, tt_stream stream) {
  if (int rc = tt_deferred_flush(ctx, TT_DQ_ALL)) return rc;
  TT_CHECK_ARG(ctx && (n_tensors == 0 || tensors), "tt_adam_multi_step: NULL argument");
  TT_CHECK_ARG(step >= 1 && n_tensors >= 0, "tt_adam_multi_step: step must be >= 1");
  const AdamK k = make_adam(step, lr, beta1, beta2, eps, weight_decay, hparams_dev);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  for (int base = 0; base < n_tensors; base += kAdamMulti) {
    AdamMultiArgs a{};
    const int cnt = n_tensors - base < kAdamMulti ? n_tensors - base : kAdamMulti;
    int64_t nmax = 1;
    for (int i = 0; i < cnt; ++i) {
      const tt_adam_tensor& t = tensors[base + i];
      TT_CHECK_ARG(t.n >= 0 && (t.n == 0 || (t.p && t.g && t.m && t.v)), "tt_adam_multi_step: tensor %d has NULL pointers", base + i);
      a.t[i] = t;
      nmax = t.n > nmax ? t.n : nmax;
    }
    int64_t gx = tt_cdiv(nmax, kThreads);
    if (gx > 64) gx = 64;
    adam_multi_kernel<<<dim3((unsigned)gx, (unsigned)cnt), kThreads, 0, st>>>(a, k);
    TT_LAUNCH_CHECK();
  }
  return TT_OK;
}

int tt_sparse_adam_step(tt_ctx* ctx, float* table, float* m, float* v, int64_t table_rows, int32_t E, const int32_t* unique_rows,
                        const float* grad_rows, const int32_t* n_unique, int64_t M, int64_t step, float lr, float beta1, float beta2, float eps,
                        float weight_decay, const float* hparams_dev, tt_stream stream) {
  if (int rc = tt_deferred_flush(ctx, TT_DQ_ALL)) return rc;
  TT_CHECK_ARG(ctx && table && m && v, "tt_sparse_adam_step: NULL state");
  TT_CHECK_ARG(step >= 1 && E >= 1 && M >= 0 && table_rows >= 1, "tt_sparse_adam_step: bad step/E/M/table_rows");
  if (M == 0) return TT_OK;
  TT_CHECK_ARG(unique_rows && grad_rows && n_unique, "tt_sparse_adam_step: NULL plan");
  const AdamK k = make_adam(step, lr, beta1, beta2, eps, weight_decay, hparams_dev);
  const bool vec4 = (E % 4 == 0) && tt_aligned(table, 16) && tt_aligned(m, 16) && tt_aligned(v, 16) && tt_aligned(grad_rows, 16);
  uint32_t C, LG;
  row_mapping(E, vec4, &C, &LG);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int grid = grid_for(ctx, M * LG);
  if (vec4) adam_sparse_kernel<4><<<grid, kThreads, 0, st>>>(table, m, v, E, C, unique_rows, grad_rows, n_unique, k, LG, table_rows);
  else adam_sparse_kernel<1><<<grid, kThreads, 0, st>>>(table, m, v, E, C, unique_rows, grad_rows, n_unique, k, LG, table_rows);
  TT_LAUNCH_CHECK();
  return TT_OK;
}

int tt_rowwise_adagrad_sparse_step(tt_ctx* ctx, float* table, float* sum, int64_t table_rows, int32_t E, const int32_t* unique_rows,
                                   const float* grad_rows, const int32_t* n_unique, int64_t M, float lr, float eps, float weight_decay,
                                   const float* hparams_dev, tt_stream stream) {
  if (int rc = tt_deferred_flush(ctx, TT_DQ_ALL)) return rc;
  TT_CHECK_ARG(ctx && table && sum, "tt_rowwise_adagrad_sparse_step: NULL state");
  TT_CHECK_ARG(E >= 1 && M >= 0 && table_rows >= 1, "tt_rowwise_adagrad_sparse_step: bad E/M/table_rows");
  if (M == 0) return TT_OK;
  TT_CHECK_ARG(unique_rows && grad_rows && n_unique, "tt_rowwise_adagrad_sparse_step: NULL plan");
  const AdagradK k = make_adagrad(lr, eps, weight_decay, hparams_dev);
  const bool vec4 = (E % 4 == 0) && tt_aligned(table, 16) && tt_aligned(grad_rows, 16);
  uint32_t C, LG;
  row_mapping(E, vec4, &C, &LG);
  if (!adagrad_fits("tt_rowwise_adagrad_sparse_step", E, C, LG)) return TT_ERR_UNSUPPORTED;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int grid = grid_for(ctx, M * LG);
  if (vec4) adagrad_sparse_kernel<4><<<grid, kThreads, 0, st>>>(table, sum, E, C, unique_rows, grad_rows, n_unique, k, LG, table_rows);
  else adagrad_sparse_kernel<1><<<grid, kThreads, 0, st>>>(table, sum, E, C, unique_rows, grad_rows, n_unique, k, LG, table_rows);
  TT_LAUNCH_CHECK();
  return TT_OK;
}

int tt_rowwise_adagrad_dense_step(tt_ctx* ctx, float* table, float* sum, const float* grad, int64_t table_rows, int32_t E, float lr,
                                  float eps, float weight_decay, const float* hparams_dev, tt_stream stream) {
  if (int rc = tt_deferred_flush(ctx, TT_DQ_ALL)) return rc;
  TT_CHECK_ARG(ctx && table && sum && grad, "tt_rowwise_adagrad_dense_step: NULL state");
  TT_CHECK_ARG(E >= 1 && table_rows >= 1, "tt_rowwise_adagrad_dense_step: bad E/table_rows");
  const AdagradK k = make_adagrad(lr, eps, weight_decay, hparams_dev);
  const bool vec4 = (E % 4 == 0) && tt_aligned(table, 16) && tt_aligned(grad, 16);
  uint32_t C, LG;
  row_mapping(E, vec4, &C, &LG);
  if (!adagrad_fits("tt_rowwise_adagrad_dense_step", E, C, LG)) return TT_ERR_UNSUPPORTED;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int grid = grid_for(ctx, table_rows * LG);
  if (vec4) adagrad_dense_kernel<4><<<grid, kThreads, 0, st>>>(table, sum, grad, table_rows, E, C, k, LG);
  else adagrad_dense_kernel<1><<<grid, kThreads, 0, st>>>(table, sum, grad, table_rows, E, C, k, LG);
  TT_LAUNCH_CHECK();
  return TT_OK;
}

int tt_adam_fused_step(tt_ctx* ctx, const tt_adam_tensor* tensors, int32_t n_tensors, float* table, float* m, float* v, int64_t table_rows,
                       int32_t E,
                       const int32_t* unique_rows, const float* grad_rows, const int32_t* n_unique, int64_t M, int64_t step, float lr,
                       float beta1, float beta2, float eps, float weight_decay, const float* hparams_dev, tt_stream stream) {
  const AdamK k = make_adam(step, lr, beta1, beta2, eps, weight_decay, hparams_dev);
  return fused_step_impl(ctx, "tt_adam_fused_step", tensors, n_tensors, step, k, AdamRows{m, v, {}}, table, table_rows, E, unique_rows,
                         const_cast<float*>(grad_rows), n_unique, M, nullptr, nullptr, 0, stream);
}

int tt_adam_fused_step_finish(tt_ctx* ctx, const tt_adam_tensor* tensors, int32_t n_tensors, float* table, float* m, float* v,
                              int64_t table_rows, int32_t E, const int32_t* unique_rows, float* grad_rows, const int32_t* n_unique,
                              int64_t M, const int32_t* seg_offsets, void* grad_workspace, size_t grad_workspace_bytes, int64_t step,
                              float lr, float beta1, float beta2, float eps, float weight_decay, const float* hparams_dev,
                              tt_stream stream) {
  TT_CHECK_ARG(grad_workspace, "tt_adam_fused_step_finish: NULL gradient workspace");
  const AdamK k = make_adam(step, lr, beta1, beta2, eps, weight_decay, hparams_dev);
  return fused_step_impl(ctx, "tt_adam_fused_step_finish", tensors, n_tensors, step, k, AdamRows{m, v, {}}, table, table_rows, E,
                         unique_rows, grad_rows, n_unique, M, seg_offsets, grad_workspace, grad_workspace_bytes, stream);
}

int tt_adam_rowwise_adagrad_fused_step(tt_ctx* ctx, const tt_adam_tensor* tensors, int32_t n_tensors, int64_t step, float lr,
                                       float beta1, float beta2, float eps, float weight_decay, const float* hparams_dev, float* table,
                                       float* sum, int64_t table_rows, int32_t E, const int32_t* unique_rows, const float* grad_rows,
                                       const int32_t* n_unique, int64_t M, float table_lr, float table_eps, float table_weight_decay,
                                       const float* table_hparams_dev, tt_stream stream) {
  return fused_step_impl(ctx, "tt_adam_rowwise_adagrad_fused_step", tensors, n_tensors, step,
                         make_adam(step, lr, beta1, beta2, eps, weight_decay, hparams_dev),
                         AdagradRows{sum, make_adagrad(table_lr, table_eps, table_weight_decay, table_hparams_dev)}, table, table_rows, E,
                         unique_rows, const_cast<float*>(grad_rows), n_unique, M, nullptr, nullptr, 0, stream);
}

int tt_adam_rowwise_adagrad_fused_step_finish(tt_ctx* ctx, const tt_adam_tensor* tensors, int32_t n_tensors, int64_t step, float lr,
                                              float beta1, float beta2, float eps, float weight_decay, const float* hparams_dev,
                                              float* table, float* sum, int64_t table_rows, int32_t E, const int32_t* unique_rows,
                                              float* grad_rows, const int32_t* n_unique, int64_t M, const int32_t* seg_offsets,
                                              void* grad_workspace, size_t grad_workspace_bytes, float table_lr, float table_eps,
                                              float table_weight_decay, const float* table_hparams_dev, tt_stream stream) {
  TT_CHECK_ARG(grad_workspace, "tt_adam_rowwise_adagrad_fused_step_finish: NULL gradient workspace");
  return fused_step_impl(ctx, "tt_adam_rowwise_adagrad_fused_step_finish", tensors, n_tensors, step,
                         make_adam(step, lr, beta1, beta2, eps, weight_decay, hparams_dev),
                         AdagradRows{sum, make_adagrad(table_lr, table_eps, table_weight_decay, table_hparams_dev)}, table, table_rows, E,
                         unique_rows, grad_rows, n_unique, M, seg_offsets, grad_workspace, grad_workspace_bytes, stream);
}

}  // extern "C"
