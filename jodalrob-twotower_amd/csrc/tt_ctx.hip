// Context, error string, ABI version.
#include "tt_common.h"
#include "tt_deferred.h"

#include <mutex>

#include <stdlib.h>
#include <string.h>

static thread_local char g_err[512] = "";
std::atomic<uint64_t> tt_launches{0};

namespace {
__global__ __launch_bounds__(kRiderThreads) void riders_kernel(tt_riders r) {
  if ((int)blockIdx.x < r.c_wg) compact_body(r.c, blockIdx.x);
  else finish2_body(r.f);
}
}  // namespace

uint32_t* tt_chain_for(tt_ctx* ctx, hipStream_t stream) {
  static std::mutex mu;
  if (!ctx || !ctx->chained || !ctx->chain) return nullptr;
  std::lock_guard<std::mutex> lock(mu);
  for (int i = 0; i < ctx->chain_used; ++i)
    if (ctx->chain_stream[i] == static_cast<void*>(stream)) return ctx->chain + (size_t)i * kChainWords;
  if (ctx->chain_used == kChainSlices) return nullptr;
  ctx->chain_stream[ctx->chain_used] = static_cast<void*>(stream);
  return ctx->chain + (size_t)(ctx->chain_used++) * kChainWords;
}

// ---- the step's queued launches (tt_deferred.h) ----
int tt_deferred_flush(tt_ctx* ctx, int mask) {
  if (!ctx) return TT_OK;
  tt_deferred& q = *ctx->dq;
  mask &= q.on; q.on &= ~mask;
  if (mask & TT_DQ_SCORE_BWD)
    if (int rc = tt_score_bwd_run(q.score, q.st[0])) return rc;
  if (mask & TT_DQ_SORT)                                 // in front of its compaction, no statistics riders
    if (int rc = tt_keyed_sort_run(q.sort, q.st[1], nullptr, 0)) return rc;
  // compaction and loss reduction: one launch where they leave together on one stream, one each otherwise
  const int c_wg = (mask & TT_DQ_COMPACT) ? q.compact_wg : 0, f_wg = (mask & TT_DQ_LOSS) ? 1 : 0;
  const bool together = c_wg && f_wg && q.st[2] == q.st[3];
  if (c_wg) {
    riders_kernel<<<c_wg + (together ? 1 : 0), kRiderThreads, 0, q.st[2]>>>(tt_riders{q.compact, c_wg, q.loss});
    TT_LAUNCH_CHECK();
  }
  if (f_wg && !together) {
    riders_kernel<<<1, kRiderThreads, 0, q.st[3]>>>(tt_riders{q.compact, 0, q.loss});
    TT_LAUNCH_CHECK();
  }
  return (mask & TT_DQ_SLABS) ? tt_gemm_tn_flush(q.st[4], &q.slabs) : TT_OK;
}

int tt_deferred_host(tt_ctx* ctx, int mask, hipStream_t st, int* mine) {
  const tt_deferred& q = *ctx->dq;
  *mine = mask & q.on;
  for (int i = 0; i < kDqSlots; ++i)
    if ((*mine & (1 << i)) && q.st[i] != st) *mine &= ~(1 << i);
  return tt_deferred_flush(ctx, mask & ~*mine);
}

int tt_deferred_queue_score_bwd(tt_ctx* ctx, hipStream_t st, const void* setup, size_t bytes, const float* dA0, const float* dA1, int64_t rows) {
  tt_deferred& q = *ctx->dq;
  if (int rc = tt_deferred_flush(ctx, TT_DQ_SCORE_BWD)) return rc;       // (one launch waits at a time)
  if (!q.score) q.score = malloc(bytes);
  TT_CHECK_ARG(q.score != nullptr, "queued score backward: out of memory");
  memcpy(q.score, setup, bytes);
  q.score_dA[0] = dA0; q.score_dA[1] = dA1; q.score_rows = rows;
  q.st[0] = st; q.on |= TT_DQ_SCORE_BWD;
  return TT_OK;
}
int tt_deferred_queue_plan(tt_ctx* ctx, hipStream_t st, const KeyedSortQueued& sort, const CompactRider& compact, int compact_wg) {
  tt_deferred& q = *ctx->dq;
  if (q.on & TT_DQ_COMPACT)                              // a second plan takes the queue's place, the older one is launched now
    if (int rc = tt_deferred_flush(ctx, TT_DQ_SCORE_BWD | TT_DQ_RIDERS)) return rc;
  q.sort = sort; q.compact = compact; q.compact_wg = compact_wg;
  q.st[1] = q.st[2] = st; q.on |= TT_DQ_SORT | TT_DQ_COMPACT;
  return TT_OK;
}
int tt_deferred_queue_loss(tt_ctx* ctx, hipStream_t st, const Finish2Rider& loss) {
  tt_deferred& q = *ctx->dq;
  if (q.on & TT_DQ_LOSS)
    if (int rc = tt_deferred_flush(ctx, TT_DQ_SCORE_BWD | TT_DQ_RIDERS)) return rc;
  q.loss = loss;
  q.st[3] = st; q.on |= TT_DQ_LOSS;
  return TT_OK;
}
int tt_deferred_queue_slabs(tt_ctx* ctx, hipStream_t st, TnPending* p) {
  if (!p || p->n == 0) return TT_OK;
  tt_deferred& q = *ctx->dq;
  TT_CHECK_ARG(!(q.on & TT_DQ_SLABS), "deferred slab reduction: the previous one was never flushed");
  q.slabs = *p;
  p->n = 0; p->maxtotal = 1;
  q.st[4] = st; q.on |= TT_DQ_SLABS;
  return TT_OK;
}

void tt_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

extern "C" {

int tt_abi_version(void) { return TT_ABI_VERSION; }

const char* tt_last_error_string(void) { return g_err; }

int tt_ctx_create(int device, tt_ctx** out) {
  TT_CHECK_ARG(out != nullptr, "tt_ctx_create: out is NULL");
  int n = 0;
  TT_HIP(hipGetDeviceCount(&n));
  TT_CHECK_ARG(device >= 0 && device < n, "tt_ctx_create: device %d out of range (%d devices)", device, n);
  hipDeviceProp_t prop;
  TT_HIP(hipGetDeviceProperties(&prop, device));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
    tt_set_error("tt_ctx_create: device %d is %s; this library is built for gfx950 (MI355X) only", device,
                 prop.gcnArchName);
    return TT_ERR_UNSUPPORTED;
  }
  tt_ctx* c = new tt_ctx();
  c->device = device;
  c->num_cus = prop.multiProcessorCount;
  c->lds_per_block = prop.sharedMemPerBlock;
  c->lookup_stamps = nullptr;
  c->lookup_stamp_slots = 0;
  c->dq = new tt_deferred();
  c->keyed_parts = 0;
  c->score_bwd_rows_min = 32768;
  c->fp8_grad = 1;
  c->bn_fin = nullptr;
  c->chain = nullptr;
  c->chain_words = 0;
  c->chain_used = 0;
  c->chained = 1;
  c->chain_spin = 1 << 22;
  c->retrieve_splits = 0;
  c->dev_err = nullptr;
  c->ho_exec = c->ho_node = c->ho_last = nullptr;
  {
    int prev = 0;
    TT_HIP(hipGetDevice(&prev));
    TT_HIP(hipSetDevice(device));
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&c->chain), sizeof(uint32_t) * (kChainWords * kChainSlices + 64));
    if (e == hipSuccess) e = hipMemset(c->chain, 0, sizeof(uint32_t) * (kChainWords * kChainSlices + 64));
    if (e == hipSuccess) c->dev_err = c->chain + (size_t)kChainWords * kChainSlices;       // (its own 256-byte line behind the pool)
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&c->bn_fin), sizeof(float) * TT_MAX_SIDES * kBnFinStride);
    (void)hipSetDevice(prev);
    if (e != hipSuccess) {
      tt_set_error("tt_ctx_create: %s", hipGetErrorString(e));
      if (c->chain) (void)hipFree(c->chain);
      delete c->dq;
      delete c;
      return TT_ERR_HIP;
    }
    c->chain_words = kChainWords;
  }
  *out = c;
  return TT_OK;
}

int tt_ctx_destroy(tt_ctx* ctx) {
  if (ctx) free(ctx->dq->score);
  if (ctx) delete ctx->dq;
  if (ctx && ctx->chain) (void)hipFree(ctx->chain);
  if (ctx && ctx->bn_fin) (void)hipFree(ctx->bn_fin);
  delete ctx;
  return TT_OK;
}

int tt_ctx_set_option(tt_ctx* ctx, int32_t option, int32_t value) {
  TT_CHECK_ARG(ctx != nullptr, "tt_ctx_set_option: NULL context");
  switch (option) {
    case TT_OPT_DEFER_SLAB_REDUCE: ctx->dq->defer_slabs = value != 0; break;
    case TT_OPT_KEYED_PARTS:
      TT_CHECK_ARG(value >= 0, "tt_ctx_set_option: TT_OPT_KEYED_PARTS needs a value >= 0");
      ctx->keyed_parts = value;
      break;
    case TT_OPT_SCORE_BWD_ROWS_MIN:
      TT_CHECK_ARG(value >= 1, "tt_ctx_set_option: TT_OPT_SCORE_BWD_ROWS_MIN needs a value >= 1");
      ctx->score_bwd_rows_min = value;
      break;
    case TT_OPT_DEFER_RIDERS:
      TT_CHECK_ARG(value >= 0 && value <= 3, "tt_ctx_set_option: TT_OPT_DEFER_RIDERS takes 0 .. 3");
      ctx->dq->defer_riders = value == 1 ? 3 : value;     // 1 = both riders (as 3), 2 = the loss reduction only
      break;
    case TT_OPT_FP8_GRAD: ctx->fp8_grad = value != 0; break;
    case TT_OPT_FUSE_SCORE_TAIL:
      ctx->dq->fuse_score_tail = value != 0;
      if (!value) return tt_deferred_flush(ctx, TT_DQ_SCORE_BWD);
      break;
    case TT_OPT_CHAINED: ctx->chained = value != 0; break;
    case TT_OPT_LOOKUP_NT: ctx->lookup_nt = value != 0; break;
    case TT_OPT_CHAIN_SPIN:
      TT_CHECK_ARG(value >= 1, "tt_ctx_set_option: TT_OPT_CHAIN_SPIN needs a value >= 1");
      ctx->chain_spin = value;
      break;
    case TT_OPT_RETRIEVE_SPLITS:
      TT_CHECK_ARG(value >= 0, "tt_ctx_set_option: TT_OPT_RETRIEVE_SPLITS needs a value >= 0");
      ctx->retrieve_splits = value;
      break;
    default: tt_set_error("tt_ctx_set_option: unknown option %d", option); return TT_ERR_INVALID_ARG;
  }
  return TT_OK;
}

int tt_ctx_check_device_errors(tt_ctx* ctx, tt_stream stream) {
  TT_CHECK_ARG(ctx != nullptr, "tt_ctx_check_device_errors: NULL context");
  if (!ctx->dev_err) return TT_OK;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  uint32_t word = 0;
  TT_HIP(hipMemcpyAsync(&word, ctx->dev_err, sizeof(word), hipMemcpyDeviceToHost, st));
  TT_HIP(hipStreamSynchronize(st));
  if (word == 0) return TT_OK;
  // clear the word and every chain slice: a launch that gave up half way leaves ready bits and a ticket behind, which the next
  // chained launch on that stream would read as prefix sums
  TT_HIP(hipMemsetAsync(ctx->chain, 0, sizeof(uint32_t) * ((size_t)kChainWords * kChainSlices + 64), st));
  TT_HIP(hipStreamSynchronize(st));
  tt_set_error("device error word 0x%x:%s%s%s%s the steps since the last check are invalid (they must be rejected)", word,
               (word & TT_DEVERR_CHAIN_TIMEOUT) ? " a chained segment-head launch gave up waiting for a predecessor tile (tt_dedup_plan / tt_dedup_plan_runs);" : "",
               (word & TT_DEVERR_ROW_RANGE) ? " a lookup decoded rows outside its table (key offsets / vocabularies that belong to another table; tt_embed_lookup_fwd / "
                                              "tt_embed_lookup_rows_fwd / tt_batch_ingest_lookup) and read the last row instead;" : "",
               (word & TT_DEVERR_CELLS_PLAN) ? " tt_score_cells_plan counted more cells than its list's capacity (its counters were disturbed): the masks of "
                                               "that step are not the list's;" : "",
               (word & TT_DEVERR_BAG_OFFSETS) ? " tt_embed_bag_fwd met bag offsets that are negative, decreasing or end beyond nnz and treated those bags as empty; "
                                                "(the same bit: tt_bag_prepare / tt_bag_store_gather refused a side whose id total exceeds its capacity or is "
                                                "not the count handed over -- its bags count as empty, no id was written);" : "");
  return TT_ERR_DEVICE;
}

int tt_handover_retarget(tt_ctx* ctx, void* graph_exec, void* node) {
  TT_CHECK_ARG(ctx != nullptr && ((graph_exec == nullptr) == (node == nullptr)), "tt_handover_retarget: NULL context / one of (graph_exec, node) NULL");
  ctx->ho_exec = graph_exec;
  ctx->ho_node = node;
  return TT_OK;
}

int tt_handover_captured_node(tt_ctx* ctx, void** node) {
  TT_CHECK_ARG(ctx != nullptr && node != nullptr, "tt_handover_captured_node: NULL argument");
  *node = ctx->ho_last;
  ctx->ho_last = nullptr;
  return TT_OK;
}

int tt_flush_deferred(tt_ctx* ctx, tt_stream) {
  TT_CHECK_ARG(ctx != nullptr, "tt_flush_deferred: NULL context");
  return tt_deferred_flush(ctx, TT_DQ_ALL);
}

int tt_flush_deferred_slabs(tt_ctx* ctx, tt_stream) {
  TT_CHECK_ARG(ctx != nullptr, "tt_flush_deferred_slabs: NULL context");
  return tt_deferred_flush(ctx, TT_DQ_SLABS);
}

int tt_deferred_pending(const tt_ctx* ctx) {
  const int on = ctx ? ctx->dq->on : 0;
  return ((on & TT_DQ_SLABS) ? 1 : 0) | ((on & TT_DQ_RIDERS) ? 2 : 0) | ((on & TT_DQ_SCORE_BWD) ? 4 : 0);
}

int tt_ctx_num_cus(const tt_ctx* ctx) { return ctx ? ctx->num_cus : 0; }

uint64_t tt_launch_count(void) { return tt_launches.load(std::memory_order_relaxed); }

}  // extern "C"
