// The step's queued launches: ONE queue in the context, ONE flush (implemented in tt_ctx.hip).  A piece of the training step that is
// not launched where it is computed waits in a SLOT here.  It runs inside another kernel's grid (a HOST: tt_deferred_host, the host's
// own launch, tt_deferred_taken) or stand-alone (tt_deferred_flush: the only place that launches queued work on its own), exactly
// once.  A slot remembers the stream it was queued on: it runs stand-alone on THAT stream whoever flushes it, and only a call on that
// stream hosts it -- its inputs are ordered there and nowhere else.  Whoever reads what a queued slot writes states the slots it
// needs in one tt_deferred_flush(ctx, mask).  A new slot: a bit, a payload, a branch of the flush and a queueing call.
#pragma once
#include "tt_common.h"
#include "tt_gemm.h"
#include "tt_riders.h"

// The slots.  BIT ORDER IS FLUSH ORDER: the score backward writes d_emb, which a flusher (tt_embed_grad_bwd behind towers that did not
// host it, the optimiser entries) may read, so it goes first; the compaction reads the sort's staging arrays, so the sort goes in
// front of it; compaction and loss reduction share one launch when they leave together; the slabs depend on none of the others.
enum : int {
  TT_DQ_SCORE_BWD = 1,   // tt_score_bwd_bf16's launch (TT_OPT_FUSE_SCORE_TAIL); host: tt_towers_mlp_bwd through tt_score_tail_bwd_launch
  TT_DQ_SORT = 2,        // the keyed plan's sort (TT_OPT_DEFER_RIDERS & 1); host: tt_towers_mlp_fwd, with the BatchNorm statistics riders
  TT_DQ_COMPACT = 4,     // the keyed plan's compaction (same option); host: tail_fwd_kernel's extra grid row
  TT_DQ_LOSS = 8,        // the symmetric score forward's last reduction (TT_OPT_DEFER_RIDERS & 2); host: tail_bwd, or gemm_back behind a hosted head
  TT_DQ_SLABS = 16,      // split-K slab reduction of the towers' weight gradients (TT_OPT_DEFER_SLAB_REDUCE); host: tt_embed_grad_bwd
  TT_DQ_RIDERS = TT_DQ_SORT | TT_DQ_COMPACT | TT_DQ_LOSS, TT_DQ_ALL = 31,
};
constexpr int kDqSlots = 5;
struct tt_deferred {
  int on = 0;                          // mask of queued slots
  hipStream_t st[kDqSlots] = {};       // per slot (index = bit number): the stream it was queued on
  // payloads.  The score backward's launch arguments are private to tt_score_bf16.hip (BwdSetup): an opaque copy, allocated on first
  // use; what a host has to compare against its own arguments lies beside it
  void* score = nullptr; const float* score_dA[2] = {}; int64_t score_rows = 0;
  KeyedSortQueued sort{};
  CompactRider compact{}; int compact_wg = 0;
  Finish2Rider loss{};
  TnPending slabs;
  int defer_slabs = 0;                 // TT_OPT_DEFER_SLAB_REDUCE
  int defer_riders = 0;                // TT_OPT_DEFER_RIDERS as a mask: 1 plan (sort + compaction), 2 loss reduction
  int fuse_score_tail = 0;             // TT_OPT_FUSE_SCORE_TAIL
};

// Launches every queued slot of `mask` stand-alone, in bit order, each on its recorded stream, and empties it.  ctx may be NULL.
int tt_deferred_flush(tt_ctx* ctx, int mask);
// A host's question: which slots of `mask` are queued on `st`?  (*mine)  A slot of `mask` queued on ANOTHER stream is not hosted: it
// is launched stand-alone over there first.  tt_deferred_taken: what the host says once its own launch has run their work.
int tt_deferred_host(tt_ctx* ctx, int mask, hipStream_t st, int* mine);
inline void tt_deferred_taken(tt_ctx* ctx, int mask) { ctx->dq->on &= ~mask; }
// One queueing call per slot (the plan's sort and compaction are queued together).  An occupied slot is displaced: the plan and
// the loss reduction first flush score backward + riders, the score backward flushes the score backward; a slab reduction that was
// never flushed is an error (its slabs live in scratch the caller has reused by now).  tt_deferred_queue_slabs empties *pending.
int tt_deferred_queue_score_bwd(tt_ctx* ctx, hipStream_t st, const void* setup, size_t bytes, const float* dA0, const float* dA1, int64_t rows);
int tt_deferred_queue_plan(tt_ctx* ctx, hipStream_t st, const KeyedSortQueued& sort, const CompactRider& compact, int compact_wg);
int tt_deferred_queue_loss(tt_ctx* ctx, hipStream_t st, const Finish2Rider& loss);
int tt_deferred_queue_slabs(tt_ctx* ctx, hipStream_t st, TnPending* pending);
// The launchers of the two payloads whose kernels live elsewhere (they know nothing of the queue): keyed_sort_kernel (tt_plan.hip)
// with bf_wg statistics riders in front of its grid (bf NULL: none); the stand-alone score backward (tt_score_bf16.hip) from the
// opaque copy of its arguments
int tt_keyed_sort_run(const KeyedSortQueued& q, hipStream_t st, const BnFinishRiders* bf, int bf_wg);
int tt_score_bwd_run(const void* setup, hipStream_t st);
