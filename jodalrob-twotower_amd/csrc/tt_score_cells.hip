// tt_score_cells_plan: the per-step list of masked (row, column) cells of the in-batch softmax, cleaned and bucketed by 32 x 32 tile
// pair for the *_cells score kernels (tt_score_cells.h).  A counting sort in four small launches (zero, count, scan, fill), every grid fixed
// by the list's CAPACITY -- the number of cells in use is read from device memory, so the launches can be nodes of a captured graph:
//   count:  cell i < min(*count, capacity), cleaned (ranges, the diagonal), adds one to its tile pair's counter (integer atomics:
//           the counts do not depend on the order)
//   scan:   ONE workgroup turns the counters into offsets (thread t owns a contiguous run of tile pairs; a fixed-order scan of the
//           1024 run totals) and leaves a copy in the counters as the fill's cursors
//   fill:   cell i takes the next slot of its tile pair (atomic cursor) and writes its local code there -- the order inside a
//           tile pair depends on the atomics' order, which no reader cares about: masking a cell twice or in another order is the same
//   zero:   in front of them, the counters' own launch
// Behind the plan: the masked-cells (KP) instantiations of the b-split backward kernels (tt_score_bwd_bsplit.h) and their launches.
// The plan costs a lane one register, so the square launch keeps the plain entry's b-split tiles where that entry has them (D <= 32:
// eight waves; D > 128: four) -- there an empty list gives the plain entry's bits -- and the masked launches' tiles between (there it
// gives the masked entry's bits on all-distinct ids); the extras' launch keeps tt_score_bwd_bf16_xneg's.  No KP instantiation uses
// scratch (profiles/NOTES.md, "masked cells"): D = 256 keeps one b tile in flight.
#include "tt_score_cells.h"
#include "tt_score_bwd_bsplit.h"

#include <string.h>

namespace {

constexpr int kScanThreads = 1024;

struct CellsArgs {
  const int32_t* cells;    // [capacity][2]
  const int32_t* count;    // device: cells in use
  int capacity, B, M, nT, nTJ;
  int n_pairs;
  int32_t* cnt;            // [n_pairs] counters, then cursors
  int32_t* off;            // [n_pairs + 1]
  int32_t* codes;          // [capacity]
  uint32_t* dev_err;       // the context's sticky error word (TT_DEVERR_CELLS_PLAN)
};

// the tile pair of cell i, or -1 (dropped); code = its local code
__device__ __forceinline__ int cell_pair(const CellsArgs& g, int i, int& code) {
  const int a = g.cells[2 * i], j = g.cells[2 * i + 1];
  if (a < 0 || a >= g.B || j < 0 || j >= g.B + g.M || j == a) return -1;
  const int jl = j < g.B ? j : j - g.B;                    // the extras' tiles start on their own boundary
  const int Jg = (j < g.B ? 0 : g.nT) + jl / 32;
  code = (a & 31) * 32 + (jl & 31);
  return (a / 32) * g.nTJ + Jg;
}

__global__ __launch_bounds__(256) void cells_zero_kernel(CellsArgs g) {
  for (int p = (int)blockIdx.x * 256 + (int)threadIdx.x; p < g.n_pairs; p += (int)gridDim.x * 256) g.cnt[p] = 0;
}

__global__ __launch_bounds__(256) void cells_count_kernel(CellsArgs g) {
  const int n = min(max(g.count[0], 0), g.capacity);
  for (int i = (int)blockIdx.x * 256 + (int)threadIdx.x; i < n; i += (int)gridDim.x * 256) {
    int code;
    const int p = cell_pair(g, i, code);
    if (p >= 0) atomicAdd(g.cnt + p, 1);
  }
}

__global__ __launch_bounds__(kScanThreads) void cells_scan_kernel(CellsArgs g) {
  __shared__ int tot[kScanThreads];
  const int t = threadIdx.x;
  const int per = (g.n_pairs + kScanThreads - 1) / kScanThreads;
  const int p0 = min(t * per, g.n_pairs), p1 = min(p0 + per, g.n_pairs);
  int s = 0;
  for (int p = p0; p < p1; ++p) s += g.cnt[p];
  tot[t] = s;
  __syncthreads();
  for (int o = 1; o < kScanThreads; o <<= 1) {             // inclusive scan of the run totals (integers: any order gives these bits)
    const int v = t >= o ? tot[t - o] : 0;
    __syncthreads();
    tot[t] += v;
    __syncthreads();
  }
  int at = tot[t] - s;
  for (int p = p0; p < p1; ++p) {
    const int n = g.cnt[p];
    g.off[p] = at;
    g.cnt[p] = at;
    at += n;
  }
  if (t == kScanThreads - 1) {
    g.off[g.n_pairs] = tot[t];
    // the counts are those of at most `capacity` cells; a larger total means somebody else wrote the counters.  Nobody reads or writes
    // past the codes array for it (the fill checks its slot, the readers clamp their spans), and the step is reported invalid
    if ((tot[t] < 0 || tot[t] > g.capacity) && g.dev_err) atomicOr(g.dev_err, TT_DEVERR_CELLS_PLAN);
  }
}

__global__ __launch_bounds__(256) void cells_fill_kernel(CellsArgs g) {
  const int n = min(max(g.count[0], 0), g.capacity);
  for (int i = (int)blockIdx.x * 256 + (int)threadIdx.x; i < n; i += (int)gridDim.x * 256) {
    int code;
    const int p = cell_pair(g, i, code);
    if (p < 0) continue;
    const int at = atomicAdd(g.cnt + p, 1);                // < off[n_pairs] <= capacity by construction (else: the scan's error bit)
    if (at >= 0 && at < g.capacity) g.codes[at] = code;
  }
}

inline bool cells_shape_ok(int64_t B, int64_t M, int64_t capacity) {
  return B >= 1 && B < ((int64_t)1 << 30) && M >= 0 && M < ((int64_t)1 << 30) && capacity >= 1 && capacity < ((int64_t)1 << 30) &&
         tt_cells_pairs(B, M) < ((int64_t)1 << 30);
}

}  // namespace

int tt_score_bwd_cells_square(const void* args, size_t args_bytes, int64_t maxRa, bool unit, bool lq, int32_t D, const int32_t* plan,
                              int64_t capacity, int64_t B, int64_t M, hipStream_t st) {
  TT_CHECK_ARG(args && args_bytes == sizeof(BwdArgs), "tt_score_bwd_cells_square: bad arguments");
  BwdArgsKP a{};
  memcpy(static_cast<BwdArgs*>(&a), args, sizeof(BwdArgs));
  a.kp = tt_cells_view(plan, B, M, capacity);
  const auto sq = [&](auto ks, auto at, auto nw) {
    const dim3 grid((unsigned)tt_cdiv(maxRa, 32 * at), 2);
    tt_dispatch([&](auto u, auto l) { score_bwd_bf16_kernel<ks, at, nw, u, false, l, false, false, true><<<grid, nw * 64, 0, st>>>(a); }, unit, lq);
  };
  switch (padded_d(D)) {
    case 32: sq(tt_c<2>, tt_c<2>, tt_c<8>); break;
    case 64: sq(tt_c<4>, tt_c<2>, tt_c<4>); break;
    case 128: sq(tt_c<8>, tt_c<1>, tt_c<4>); break;
    default: sq(tt_c<16>, tt_c<1>, tt_c<4>); break;
  }
  TT_LAUNCH_CHECK();
  return TT_OK;
}

int tt_score_bwd_cells_xneg(const void* args, size_t args_bytes, bool unit, int32_t D, const int32_t* plan, int64_t capacity, int64_t B,
                            int64_t M, hipStream_t st) {
  TT_CHECK_ARG(args && args_bytes == sizeof(XnegArgs), "tt_score_bwd_cells_xneg: bad arguments");
  XnegArgsKP a{};
  memcpy(static_cast<XnegArgs*>(&a), args, sizeof(XnegArgs));
  a.kp = tt_cells_view(plan, B, M, capacity);
  a.nT = (int)tt_cdiv(B, 32);
  const int64_t maxRa = B > M ? B : M;
  const auto go = [&](auto ks, auto at) {
    const dim3 grid((unsigned)tt_cdiv(maxRa, 32 * at), 2);
    tt_dispatch([&](auto u) { score_bwd_xneg_kernel<ks, at, 4, u, false, true><<<grid, 4 * 64, 0, st>>>(a); }, unit);
  };
  switch (padded_d(D)) {
    case 32: go(tt_c<2>, tt_c<2>); break;
    case 64: go(tt_c<4>, tt_c<2>); break;
    case 128: go(tt_c<8>, tt_c<1>); break;
    default: go(tt_c<16>, tt_c<1>); break;
  }
  TT_LAUNCH_CHECK();
  return TT_OK;
}

extern "C" {

size_t tt_score_cells_plan_bytes(int64_t B, int64_t M, int64_t capacity) {
  if (!cells_shape_ok(B, M, capacity)) return 0;
  return sizeof(int32_t) * (size_t)(tt_cells_codes_at(B, M) + capacity);
}

size_t tt_score_cells_plan_workspace_bytes(int64_t B, int64_t M) {
  if (!cells_shape_ok(B, M, 1)) return 0;
  return sizeof(int32_t) * (size_t)tt_cells_pairs(B, M) + 256;
}

int tt_score_cells_plan(tt_ctx* ctx, const int32_t* cells, const int32_t* count, int64_t capacity, int64_t B, int64_t M, int32_t* plan,
                        size_t plan_bytes, void* workspace, size_t workspace_bytes, tt_stream stream) {
  TT_CHECK_ARG(ctx && cells && count && plan && workspace, "tt_score_cells_plan: NULL argument");
  TT_CHECK_ARG(cells_shape_ok(B, M, capacity), "tt_score_cells_plan: bad shape B=%lld M=%lld capacity=%lld", (long long)B, (long long)M,
               (long long)capacity);
  TT_CHECK_ARG(tt_aligned(plan, 16), "tt_score_cells_plan: plan must be 16-byte aligned");
  TT_CHECK_ARG(plan_bytes >= tt_score_cells_plan_bytes(B, M, capacity), "tt_score_cells_plan: plan %zu < required %zu bytes", plan_bytes,
               tt_score_cells_plan_bytes(B, M, capacity));
  if (workspace_bytes < tt_score_cells_plan_workspace_bytes(B, M)) {
    tt_set_error("tt_score_cells_plan: workspace %zu < required %zu", workspace_bytes, tt_score_cells_plan_workspace_bytes(B, M));
    return TT_ERR_WORKSPACE;
  }
  CellsArgs g{};
  g.cells = cells; g.count = count;
  g.capacity = (int)capacity; g.B = (int)B; g.M = (int)M;
  g.nT = (int)tt_cdiv(B, 32);
  g.nTJ = g.nT + (int)tt_cdiv(M, 32);
  g.n_pairs = (int)tt_cells_pairs(B, M);
  g.cnt = reinterpret_cast<int32_t*>((reinterpret_cast<uintptr_t>(workspace) + 255) & ~uintptr_t(255));
  g.off = plan;
  g.codes = plan + tt_cells_codes_at(B, M);
  g.dev_err = ctx->dev_err;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  cells_zero_kernel<<<(unsigned)(tt_cdiv(g.n_pairs, 256) < 1024 ? tt_cdiv(g.n_pairs, 256) : 1024), 256, 0, st>>>(g);
  TT_LAUNCH_CHECK();
  const unsigned grid = (unsigned)(tt_cdiv(capacity, 256) < 1024 ? tt_cdiv(capacity, 256) : 1024);
  cells_count_kernel<<<grid, 256, 0, st>>>(g);
  TT_LAUNCH_CHECK();
  cells_scan_kernel<<<1, kScanThreads, 0, st>>>(g);
  TT_LAUNCH_CHECK();
  cells_fill_kernel<<<grid, 256, 0, st>>>(g);
  TT_LAUNCH_CHECK();
  return TT_OK;
}

}  // extern "C"
