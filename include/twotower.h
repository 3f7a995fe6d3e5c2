/*
 * twotower.h -- C ABI of the MI355X-native two-tower training step (libtwotower_hip.so).
 *
 * The reference (zoongahn/jodalroB-twoTower) has no FFI: its hot path sits behind plain PyTorch
 * modules.  This header is the boundary a binding for that path would use; every entry point names
 * the reference code it replaces (paths relative to the reference root).  See INTEGRATION.md for
 * the ctypes stub a maintainer would add.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes; no torch / C++ types.
 *   - every data pointer is a DEVICE pointer borrowed from the caller (never freed / resized here);
 *     descriptor structs themselves live in HOST memory and are read during the call only.
 *   - scratch comes from the caller: <op>_workspace_bytes() + (workspace, workspace_bytes).
 *   - all work is enqueued asynchronously on `stream` (a hipStream_t); no hidden synchronisation.
 *   - returns TT_OK (0) or a negative TT_ERR_*; never throws, never exits;
 *     tt_last_error_string() gives the thread's last message.
 *   - row-major everywhere; `ld*` = leading dimension in ELEMENTS.
 */
#ifndef TWOTOWER_H_
#define TWOTOWER_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TT_ABI_VERSION 2

#define TT_OK 0
#define TT_ERR_INVALID_ARG (-1)
#define TT_ERR_HIP (-2)
#define TT_ERR_WORKSPACE (-3)
#define TT_ERR_UNSUPPORTED (-4)
#define TT_ERR_DEVICE (-5) /* tt_ctx_check_device_errors: a kernel raised the context's sticky device error word */

#define TT_F32 0
#define TT_BF16 1

#define TT_MAX_SIDES 4   /* towers fused into one lookup / gradient launch */
#define TT_MAX_HIDDEN 8  /* [Linear,ReLU,BatchNorm1d,Dropout] blocks per tower */

typedef struct tt_ctx tt_ctx; /* opaque: device id, cached device properties */
typedef void* tt_stream;      /* hipStream_t */

int tt_abi_version(void);
int tt_ctx_create(int device, tt_ctx** out);
int tt_ctx_destroy(tt_ctx* ctx);
const char* tt_last_error_string(void);
/* number of compute units of the context's device (used by callers to size synthetic work) */
int tt_ctx_num_cus(const tt_ctx* ctx);
/* kernels this library has launched (or recorded into a stream capture) so far in the process: the difference across one
 * captured step is the step's launch count (collectives and the caller's own kernels are not in it); a measurement aid */
uint64_t tt_launch_count(void);

/* Options of a context.  Three of them make an entry leave a launch QUEUED in the context instead of issuing it; one rule holds for
 * all three (tt_flush_deferred below states it: who launches what is still queued, on which stream, exactly once).
 * TT_OPT_DEFER_SLAB_REDUCE (default 0): tt_towers_mlp_bwd's one-launch first-block backward queues the split-K slab reduction of
 * its weight gradients; the next tt_embed_grad_bwd with TT_GRAD_PLANNED runs it in the first workgroups of its own launch (the two
 * are independent: one launch fewer in the step's dependent chain).  Nothing else may write the towers' workspace while bit 0 of
 * tt_deferred_pending() is set. */
#define TT_OPT_DEFER_SLAB_REDUCE 1
/* TT_OPT_KEYED_PARTS (default 0 = chosen from the batch size): workgroups per key of tt_dedup_plan_keyed* -- every value gives
 * the same plan bit for bit (tests vary it).  TT_OPT_SCORE_BWD_ROWS_MIN (default 32768): number of rows from which
 * tt_score_bwd_bf16 takes the workgroup-staged form instead of the b-split form (same results up to summation order; tests
 * force either form). */
#define TT_OPT_KEYED_PARTS 2
#define TT_OPT_SCORE_BWD_ROWS_MIN 3
/* TT_OPT_DEFER_RIDERS (default 0; 1 or 3 = both riders, 2 = only the loss reduction -- a caller that reads the plan right after
 * building it, as the sharded exchange does): tt_dedup_plan_keyed* queues the plan's compaction, and tt_score_fwd_sym_* its last reduction
 * (loss_out / out8): tt_towers_mlp_fwd / tt_towers_mlp_bwd run them in an extra grid row of their fused tail kernels (two launches
 * fewer in the step's dependent chain; same bodies: bit-identical).  Until they have run, the plan's unique_rows / seg_offsets /
 * n_unique and the forward's loss_out / out8 are NOT written.  With the compaction queued, the plan's
 * SORT waits in the queue too: tt_towers_mlp_fwd issues it behind its front kernel and in front of the fused tail, with one
 * workgroup per tower in its grid that finishes the BatchNorm batch statistics once (the tail's workgroups then read the finished
 * mean / rstd instead of merging the chunk partials each; same merge order: bit-identical); towers without the fused narrow tail
 * host neither.  `rows` must stay valid and unchanged until the sort has run.  A second queueing call launches the older occupant
 * first. */
#define TT_OPT_DEFER_RIDERS 4
/* TT_OPT_FP8_GRAD (default 1): tt_score_bwd_fp8 forms the gradient products dA = W B from e4m3 operands as well (softmax weights
 * block-scaled per row and 32 consecutive b rows, the diagonal weight kept apart in f32: tt_score_bwd_fp8 below); 0 = bf16 weights and bf16
 * B rows for those products (round 2's arithmetic, 1.5 x the matrix-pipe time). */
#define TT_OPT_FP8_GRAD 5
/* TT_OPT_CHAINED (default 1): the segment-head pass of tt_dedup_plan / tt_dedup_plan_runs runs as ONE launch, its cross-workgroup
 * prefix sum chained through a small context-owned buffer (a tile publishes its head count with a ready bit and sums its
 * predecessors'; the last one through clears the buffer); 0 = count and write as separate launches.  Same results bit for bit
 * (tests compare the two). */
#define TT_OPT_CHAINED 6
/* TT_OPT_LOOKUP_NT (default 0): tt_batch_ingest_lookup stores its bf16 rows with non-temporal stores (same bits; an A/B switch:
 * they leave L2 during the launch instead of at its end). */
#define TT_OPT_LOOKUP_NT 7
/* TT_OPT_CHAIN_SPIN (default 2^22): polls after which a tile of a chained launch stops waiting for a predecessor (it then raises
 * the device error word instead of hanging the GPU); tests lower it to provoke the error path. */
#define TT_OPT_CHAIN_SPIN 8
/* TT_OPT_RETRIEVE_SPLITS (default 0 = chosen from the shapes): catalogue splits of tt_retrieve_topk_* (clamped to
 * [1, min(32, ceil(nC / 32))]).  Every value gives the same results bit for bit (tests vary it). */
#define TT_OPT_RETRIEVE_SPLITS 9
/* TT_OPT_FUSE_SCORE_TAIL (default 0; independent of TT_OPT_DEFER_RIDERS): tt_score_bwd_bf16 leaves its launch QUEUED in the context
 * instead of launching it when the call takes the one-image transposing form at padded D = 64 (below TT_OPT_SCORE_BWD_ROWS_MIN
 * rows) with two directions over square problems of one size (Ra == Rb) -- every other entry, shape and the logQ form launch at once.
 * The next tt_towers_mlp_bwd launches it with the towers' backward head (L2-normalise backward, d_act, the output layer's gradient
 * slabs, the BN column sums) in the epilogue of its workgroups -- one launch instead of two, no round trip of d_emb, same values in
 * the same order: bit-identical -- when the fused narrow tail applies (no sync_phase), there are two towers whose last hidden width and d_out are 64,
 * the row chunks are 64 rows each (chunk x = rows 64 x .. 64 x + 63, the score workgroup's rows), it is called on the stream the
 * score backward was queued on and its d_emb[t] are exactly the queued dA of direction t.  A loss reduction queued under
 * TT_OPT_DEFER_RIDERS then rides the tail's second launch.  Otherwise tt_towers_mlp_bwd launches the queued score backward on its own
 * in front of itself.  Until then dA is NOT written.  Another queueing tt_score_bwd_bf16 and setting this option to 0 also launch a
 * score backward that is still queued. */
#define TT_OPT_FUSE_SCORE_TAIL 10
int tt_ctx_set_option(tt_ctx* ctx, int32_t option, int32_t value);
/* Device-side errors.  A kernel that cannot complete its contract without hanging or faulting the GPU (a tile of a chained
 * segment-head launch whose bounded wait for a predecessor expired; a lookup whose decoded row lies outside the table it was given
 * -- key offsets / vocabularies of another table: the launch reads the table's last row instead) raises a STICKY word in device memory owned by the context
 * (TT_DEVERR_* bits) and finishes; nothing reaches the host by itself.  tt_ctx_check_device_errors reads the word (synchronises
 * `stream`), and if it is set: clears it, zeroes the context's chain buffers, sets the error string and returns TT_ERR_DEVICE --
 * every plan built since the previous check must then be considered corrupt.  Call it where the host synchronises anyway (end of an
 * epoch, before a checkpoint, when a captured step is closed). */
#define TT_DEVERR_CHAIN_TIMEOUT 1u
#define TT_DEVERR_ROW_RANGE 2u
#define TT_DEVERR_CELLS_PLAN 4u   /* tt_score_cells_plan: its counters summed to more cells than the list's capacity */
int tt_ctx_check_device_errors(tt_ctx* ctx, tt_stream stream);
/* The hand-over launch as a node of a captured graph.  A tt_batch_ingest* call on a stream that is being captured becomes a kernel
 * node; tt_handover_captured_node hands that node out (NULL if the last call was not captured) and forgets it.  Later, between
 * tt_handover_retarget(ctx, graph_exec, node) and tt_handover_retarget(ctx, NULL, NULL), every tt_batch_ingest* call launches
 * NOTHING: it re-points `node` of the executable graph `graph_exec` (hipGraphExec_t) at the call's own kernel, grid and arguments
 * (hipGraphExecKernelNodeSetParams), so that the next launch of the graph hands over THAT batch -- launches already enqueued keep
 * theirs.  What it is for: a graph that holds SEVERAL training steps, hand-overs included (graph.GraphedTrainStep(unroll=U)): one graph
 * launch costs ~8 us on top of its nodes on this runtime (tools/probe/graph_setparams.hip), U steps per launch pay it once.
 * Reference counterpart: none (torch.compile(mode="reduce-overhead") replays one step per launch, scripts/train.py:223-225). */
int tt_handover_retarget(tt_ctx* ctx, void* graph_exec, void* node);
int tt_handover_captured_node(tt_ctx* ctx, void** node);
/* What the three queueing options (TT_OPT_DEFER_SLAB_REDUCE, TT_OPT_DEFER_RIDERS, TT_OPT_FUSE_SCORE_TAIL) leave in the context
 * runs exactly once: inside the launch of the entry that hosts it (named at each option), or on its own at the first of these
 * flush points -- tt_flush_deferred (everything); tt_embed_grad_bwd (everything; the slab reduction inside its own launch on a
 * planned workspace); every tt_adam_* / tt_rowwise_adagrad_* entry (everything, before it reads a gradient); tt_towers_mlp_bwd (a score
 * backward it cannot host).  Order: score backward, the plan's sort, its compaction and the loss reduction (one launch when they
 * leave together), slab reduction.  Streams: a queued launch runs on the stream of the call that QUEUED it, whoever flushes it, and
 * an entry hosts it only when called on that stream (otherwise it is launched on its own stream first) -- its inputs are ordered
 * there.  The `stream` argument of the two calls below therefore does not choose where queued work runs; it is kept for the ABI.
 * Switching TT_OPT_DEFER_SLAB_REDUCE or TT_OPT_DEFER_RIDERS off launches nothing by itself (call tt_flush_deferred);
 * TT_OPT_FUSE_SCORE_TAIL = 0 launches a queued score backward.  For callers that run the whole step back to back
 * (GraphedTrainStep). */
int tt_flush_deferred(tt_ctx* ctx, tt_stream stream);
/* only the queued slab reduction (the one thing that lives in the caller's shared scratch buffer) */
int tt_flush_deferred_slabs(tt_ctx* ctx, tt_stream stream);
/* bit 0: a slab reduction is queued; bit 1: the plan's sort / compaction or the loss reduction (TT_OPT_DEFER_RIDERS); bit 2: a score
 * backward (TT_OPT_FUSE_SCORE_TAIL) */
int tt_deferred_pending(const tt_ctx* ctx);

/* ------------------------------------------------------------------------------------------------
 * Categorical embedding lookup  -- replaces CategoricalEmbedder._kjt_to_dict + .forward
 * (src/towers/cat_embed.py:88-123 id unpack + clamp, :157-178 per-key nn.Embedding gather + cat)
 * and the torch.cat of src/towers/tower/base_tower.py:139 (rows are written straight into the MLP
 * input buffer at a column offset).
 *
 * All per-key tables of all towers live in ONE fused row space `table[table_rows, E]` (f32).
 * For side s, sample b, key k:   id  = ids[b*K + k]                       (sample-major KJT values)
 *                                row = key_row_offset[k] + clamp(id, 0, key_vocab[k]-1)
 *                                out[b*ld_out + k*E .. +E) = table[row*E .. +E)
 * table == NULL (with rows_out set): rows-only mode -- nothing is gathered, only rows_out is written
 * (used to route ids to the rank that owns the row when the table is sharded).
 * rows_out (optional, may be NULL): fused row of every slot, slot = side_slot_base + b*K + k with
 * side_slot_base = sum of B*K of the earlier sides -- the input of tt_dedup_plan.
 * ---------------------------------------------------------------------------------------------- */
typedef struct tt_embed_side {
  const int64_t* ids;            /* [B*K] */
  const int64_t* key_row_offset; /* [K] first fused row of key k */
  const int64_t* key_vocab;      /* [K] rows of key k (reference: metadata count + 10) */
  void* out;                     /* first output element of sample 0 / key 0 */
  int64_t ld_out;
  int32_t K;
  int32_t out_dtype; /* TT_F32 (bit-exact row copy) or TT_BF16 (round-to-nearest-even) */
} tt_embed_side;

/* Measurement hook: per-launch device-clock stamps of the lookup kernel, usable inside a captured graph (where
 * HIP events cannot bracket one kernel), without host synchronisation and WITHOUT an extra launch.
 * `ring_dev` = 8192 + n_slots * 8192 * 2 uint64 words of device memory, zero-initialised by the caller:
 *   [b], b < 8192: launch counter of workgroup b (each workgroup keeps its own: [0] = launches so far);
 *   then n_slots blocks of 8192 pairs {start, end}: block (n mod n_slots), pair b = workgroup b in launch n --
 *   start = its first instruction, end = all its stores have completed (0, 0 = workgroup not in the grid).
 *   Kernel duration of launch n = (max end - min start over the block) * 10 ns (100 MHz clock); the caller reduces.
 *   ring_dev == NULL switches the hook off.  The fused hand-over + lookup launch (tt_batch_ingest_lookup) writes the same ring:
 *   workgroup b = its linear index, the tiles (gather phase) first, the copy roles behind them. */
int tt_embed_lookup_set_profile(tt_ctx* ctx, uint64_t* ring_dev, int32_t n_slots);
int tt_embed_lookup_fwd(tt_ctx* ctx, const float* table, int64_t table_rows, int32_t E,
                        const tt_embed_side* sides, int32_t n_sides, int64_t B, int32_t* rows_out,
                        tt_stream stream);
/* The same gather + concat (cat_embed.py:157-178, base_tower.py:139) from PRECOMPUTED fused rows: rows[slot], slot = side_base +
 * b*K + k (side_base = sum of B*K of the earlier sides), already clamped -- what tt_batch_ingest / tt_batch_ingest_store leave in
 * `rows_sm` when a captured step's batch is handed over (they decode and clamp every id anyway).  sides[i] gives K / out / ld_out /
 * out_dtype (ids, key_row_offset, key_vocab are ignored and may be NULL).  Same bits in the outputs as tt_embed_lookup_fwd on the
 * ids the rows came from (test); the kernel reads a 4-byte row instead of an 8-byte id + its key's offset and vocabulary.
 * The rows are trusted to lie in [0, table_rows): the hand-over that formed them has checked them (its table_rows argument);
 * tt_embed_lookup_fwd checks the rows it decodes itself (TT_DEVERR_ROW_RANGE).
 * E = 4 x a power of two, outputs 4-element aligned (TT_ERR_UNSUPPORTED otherwise). */
int tt_embed_lookup_rows_fwd(tt_ctx* ctx, const float* table, int64_t table_rows, int32_t E,
                             const tt_embed_side* sides, int32_t n_sides, int64_t B, const int32_t* rows,
                             tt_stream stream);

/* ------------------------------------------------------------------------------------------------
 * Duplicate-row plan for the sparse gradient (a16): stable LSD radix sort of the M slot rows, then
 * segment boundaries of equal rows.  Depends on ids only, so callers run it during the forward.
 *   sorted_src[i]   slot index of the i-th smallest row (ties in ascending slot order)
 *   unique_rows[u]  u-th distinct row, ascending;   seg_offsets[u]..seg_offsets[u+1] its span
 *   n_unique[0]     number of distinct rows U (stays on the device; consumers read it there)
 * ---------------------------------------------------------------------------------------------- */
size_t tt_dedup_workspace_bytes(int64_t M);
int tt_dedup_plan(tt_ctx* ctx, const int32_t* rows, int64_t M, int64_t table_rows,
                  int32_t* sorted_src, int32_t* unique_rows, int32_t* seg_offsets, int32_t* n_unique,
                  void* workspace, size_t workspace_bytes, tt_stream stream);

/* Same plan for slot rows that come straight from tt_embed_lookup_fwd (slot = side_base + b*K + k): key k's
 * rows lie in key k's own row range, so the sort decomposes into sum(K) independent sorts of B ids.  One
 * workgroup per key sorts its B ids entirely in LDS (stable LSD radix, ballot ranking) and a second small
 * launch compacts the per-key unique lists: 2 launches instead of 3 per radix pass + 2.  Needs B <= 8192 and
 * key row ranges ascending in (side, k) order (true for the fused store); same outputs as tt_dedup_plan. */
size_t tt_dedup_keyed_workspace_bytes(int64_t M, int32_t n_keys);
int tt_dedup_plan_keyed(tt_ctx* ctx, const int32_t* rows, const int32_t* side_K /* host [n_sides] */,
                        int32_t n_sides, int64_t B, int32_t* sorted_src, int32_t* unique_rows,
                        int32_t* seg_offsets, int32_t* n_unique, void* workspace, size_t workspace_bytes,
                        tt_stream stream);

/* The same plan from rows in KEY-MAJOR order, rows_km[side_base + k*B + b] (written by tt_batch_ingest): a key's B rows are
 * one contiguous run instead of one word per K*4 bytes -- the sort's own strided load is 6.5 of a workgroup's 18 us. */
int tt_dedup_plan_keyed_km(tt_ctx* ctx, const int32_t* rows_km, const int32_t* side_K /* host [n_sides] */,
                           int32_t n_sides, int64_t B, int32_t* sorted_src, int32_t* unique_rows,
                           int32_t* seg_offsets, int32_t* n_unique, void* workspace, size_t workspace_bytes,
                           tt_stream stream);

/* The per-key plan that ALSO prepares the gradient reduction: rows with more than 64 slots (the two-row keys: thousands each)
 * are summed chunk by chunk, and the list of those rows / chunks depends on the plan only.  Built here -- into the workspace
 * tt_embed_grad_bwd will be called with (size tt_embed_grad_workspace_bytes(M, E), flag TT_GRAD_PLANNED; nobody else may touch
 * it in between) -- the reduction's row pass and chunk pass run as ONE launch instead of one after the other.
 * The list and its counters belong to the plan: the reductions over it (tt_embed_grad_bwd with TT_GRAD_PLANNED, the deferred
 * finishes) read them and leave them as they are, so any number of reductions may run over one plan (several backward passes
 * of one forward: TT_GRAD_DENSE_SET, then TT_GRAD_DENSE_ACC).  Building the plan again resets them.
 * rows_key_major: 0 = the lookup's slot-major rows, 1 = tt_batch_ingest's [key][sample] rows. */
int tt_dedup_plan_keyed_long(tt_ctx* ctx, const int32_t* rows, int32_t rows_key_major, const int32_t* side_K /* host [n_sides] */,
                             int32_t n_sides, int64_t B, int32_t E, int32_t* sorted_src, int32_t* unique_rows,
                             int32_t* seg_offsets, int32_t* n_unique, void* grad_workspace, size_t grad_workspace_bytes,
                             void* workspace, size_t workspace_bytes, tt_stream stream);

/* ------------------------------------------------------------------------------------------------
 * Embedding gradient -- replaces autograd's nn.Embedding backward (dense index_add; reference
 * builds its tables with sparse=False, src/towers/cat_embed.py:42-45; scripts/train.py:326).
 * Slot s of source i reads d_out_i[b*ld + k*E .. +E).  Atomic-free: one wave-group per distinct
 * row sums its contributions in ascending slot order; rows with more than 64 contributions are
 * summed in 64-slot chunks whose partial sums are then added in chunk order (bitwise reproducible).
 *   TT_GRAD_SPARSE     out[u*E .. +E)               = sum   (u < U; out has room for M rows)
 *   TT_GRAD_DENSE_SET  out[unique_rows[u]*E .. +E)  = sum   (caller zeroed the dense buffer)
 *   TT_GRAD_DENSE_ACC  out[unique_rows[u]*E .. +E) += sum
 *   | TT_GRAD_SHORT_SEGMENTS (flag): every row is summed by one lane group whatever its length, and the chunk passes
 *     are not launched -- for callers that know no row has many contributions (the owner side of the row exchange:
 *     at most one per rank).  Results do not depend on the flag, only the time does.
 * ---------------------------------------------------------------------------------------------- */
#define TT_GRAD_SPARSE 0
#define TT_GRAD_DENSE_SET 1
#define TT_GRAD_DENSE_ACC 2
#define TT_GRAD_SHORT_SEGMENTS 0x100
#define TT_GRAD_PLANNED 0x200 /* the workspace was handed to tt_dedup_plan_keyed_long, which left the long-row list in it */
/* with TT_GRAD_PLANNED | TT_GRAD_SPARSE: leave the long rows' chunk sums unadded (their rows of `out` are not written) -- the
 * caller completes `out` on the same workspace with tt_adam_fused_step_finish (inside the optimiser's launch: one launch
 * fewer in the step's dependent chain) or tt_embed_grad_finish, before anything else reads those rows */
#define TT_GRAD_DEFER_FINISH 0x400

typedef struct tt_grad_src {
  const void* d_out; /* gradient w.r.t. the lookup output of this side */
  int64_t ld;
  int32_t K;
  int32_t dtype; /* TT_F32 / TT_BF16 */
} tt_grad_src;

size_t tt_embed_grad_workspace_bytes(int64_t M, int32_t E);
/* counters: NULL, or 3 int32 words of device memory that are ZERO on entry and that the caller keeps (per stream) between
 * calls: the last kernel of the reduction leaves them zero again, so no zeroing launch precedes the reduction. */
int tt_embed_grad_bwd(tt_ctx* ctx, const tt_grad_src* srcs, int32_t n_srcs, int64_t B, int32_t E,
                      const int32_t* sorted_src, const int32_t* seg_offsets,
                      const int32_t* unique_rows, const int32_t* n_unique, int64_t M, int32_t mode,
                      float* out, int32_t* counters, void* workspace, size_t workspace_bytes, tt_stream stream);

/* ------------------------------------------------------------------------------------------------
 * Adam -- replaces torch.optim.Adam(lr, betas=(0.9,0.999), eps=1e-8, weight_decay coupled)
 * (scripts/train.py:231, :327).  `step` is the 1-based step count used for bias correction.
 *   tt_adam_dense_step : exact dense Adam over n contiguous elements (tower weights / small tables)
 *   tt_sparse_adam_step: the same update applied only to the U looked-up rows; entries of unique_rows that
 *   are >= table_rows are skipped (pads of the multi-GPU fixed-capacity routing) (rows not in the batch
 *                        keep weight, m and v untouched -- the documented difference to the
 *                        reference's dense update; DESIGN.md "optimiser semantics")
 * ---------------------------------------------------------------------------------------------- */
/* Graph capture: when `hparams_dev` is non-NULL the kernels read the per-step scalars from DEVICE memory
 * instead of the host arguments, so a captured launch can be replayed with a new lr / step:
 *   hparams_dev[0] = lr / (1 - beta1^step)   hparams_dev[1] = 1 / sqrt(1 - beta2^step)
 *   hparams_dev[2] = beta1  [3] = beta2  [4] = eps  [5] = weight_decay        (tt_adam_hparams fills them) */
void tt_adam_hparams(int64_t step, float lr, float beta1, float beta2, float eps, float weight_decay,
                     float out6[6]);
int tt_adam_dense_step(tt_ctx* ctx, float* p, const float* g, float* m, float* v, int64_t n,
                       int64_t step, float lr, float beta1, float beta2, float eps,
                       float weight_decay, const float* hparams_dev, tt_stream stream);
/* the same dense update over n_tensors separate tensors in one launch per 32 tensors */
typedef struct tt_adam_tensor {
  float* p;
  const float* g;
  float* m;
  float* v;
  int64_t n;
} tt_adam_tensor;
int tt_adam_multi_step(tt_ctx* ctx, const tt_adam_tensor* tensors /* host array */, int32_t n_tensors,
                       int64_t step, float lr, float beta1, float beta2, float eps,
                       float weight_decay, const float* hparams_dev, tt_stream stream);
int tt_sparse_adam_step(tt_ctx* ctx, float* table, float* m, float* v, int64_t table_rows, int32_t E,
                        const int32_t* unique_rows, const float* grad_rows, const int32_t* n_unique,
                        int64_t M, int64_t step, float lr, float beta1, float beta2, float eps,
                        float weight_decay, const float* hparams_dev, tt_stream stream);

/* tt_adam_multi_step (<= 32 tensors) and tt_sparse_adam_step with the same hyper-parameters in ONE launch: the
 * tower weights and the looked-up table rows of a step (optim.FusedAdam uses it when both share a parameter group
 * and step number). */
int tt_adam_fused_step(tt_ctx* ctx, const tt_adam_tensor* tensors, int32_t n_tensors, float* table, float* m, float* v,
                       int64_t table_rows, int32_t E, const int32_t* unique_rows, const float* grad_rows, const int32_t* n_unique, int64_t M,
                       int64_t step, float lr, float beta1, float beta2, float eps, float weight_decay,
                       const float* hparams_dev, tt_stream stream);

/* tt_adam_fused_step for a gradient whose long-row finish was deferred (TT_GRAD_DEFER_FINISH): extra workgroups add each long
 * row's chunk partials (same order as the reduction's own finish: bit-identical), store the sum into grad_rows and update that
 * table row; grad_rows is complete when the launch has run. */
int tt_adam_fused_step_finish(tt_ctx* ctx, const tt_adam_tensor* tensors, int32_t n_tensors, float* table, float* m, float* v,
                              int64_t table_rows, int32_t E, const int32_t* unique_rows, float* grad_rows, const int32_t* n_unique,
                              int64_t M, const int32_t* seg_offsets, void* grad_workspace, size_t grad_workspace_bytes,
                              int64_t step, float lr, float beta1, float beta2, float eps, float weight_decay,
                              const float* hparams_dev, tt_stream stream);

/* Row-wise Adagrad for the embedding tables (FBGEMM's EXACT_ROWWISE_ADAGRAD): ONE f32 accumulator per table row, `sum`
 * [table_rows], zero initially.  For a row w (E floats) with gradient g:
 *   g' = g + weight_decay * w   (coupled, as Adam's; only when weight_decay != 0)
 *   s += sum_j g'_j^2 / E;   w -= lr / (sqrt(s) + eps) * g'
 * The row's sum is formed in a fixed order (lane-local in column order, then an xor butterfly over the row's lanes): two
 * runs on the same inputs, and a graph replay against eager calls, give the same bits.  E <= 1024 (E <= 256 when E % 4 != 0).
 * hparams_dev: NULL, or device floats [0] = lr [1] = eps [2] = weight_decay read instead of the host scalars (graph replay).
 *   tt_rowwise_adagrad_sparse_step: the U rows of a dedup plan; entries of unique_rows >= table_rows are skipped (routing
 *                                   pads); rows not in the plan are not touched
 *   tt_rowwise_adagrad_dense_step : every row of a dense-mode [table_rows, E] store gradient */
int tt_rowwise_adagrad_sparse_step(tt_ctx* ctx, float* table, float* sum, int64_t table_rows, int32_t E,
                                   const int32_t* unique_rows, const float* grad_rows, const int32_t* n_unique, int64_t M,
                                   float lr, float eps, float weight_decay, const float* hparams_dev, tt_stream stream);
int tt_rowwise_adagrad_dense_step(tt_ctx* ctx, float* table, float* sum, const float* grad, int64_t table_rows, int32_t E,
                                  float lr, float eps, float weight_decay, const float* hparams_dev, tt_stream stream);
/* tt_adam_multi_step (<= 32 tensors, the first hyper-parameter set) and tt_rowwise_adagrad_sparse_step (the table_* set) in
 * ONE launch: the towers and the tables sit in different parameter groups.  Equal to the two separate entries. */
int tt_adam_rowwise_adagrad_fused_step(tt_ctx* ctx, const tt_adam_tensor* tensors, int32_t n_tensors, int64_t step, float lr,
                                       float beta1, float beta2, float eps, float weight_decay, const float* hparams_dev,
                                       float* table, float* sum, int64_t table_rows, int32_t E, const int32_t* unique_rows,
                                       const float* grad_rows, const int32_t* n_unique, int64_t M, float table_lr,
                                       float table_eps, float table_weight_decay, const float* table_hparams_dev,
                                       tt_stream stream);
/* the same for a gradient whose long-row finish was deferred (TT_GRAD_DEFER_FINISH): workgroups of the launch complete each
 * long row into grad_rows (bit-identical to the reduction's own finish), then reduce that row's g'^2 over all E columns and
 * update it; grad_rows is complete when the launch has run. */
int tt_adam_rowwise_adagrad_fused_step_finish(tt_ctx* ctx, const tt_adam_tensor* tensors, int32_t n_tensors, int64_t step,
                                              float lr, float beta1, float beta2, float eps, float weight_decay,
                                              const float* hparams_dev, float* table, float* sum, int64_t table_rows, int32_t E,
                                              const int32_t* unique_rows, float* grad_rows, const int32_t* n_unique, int64_t M,
                                              const int32_t* seg_offsets, void* grad_workspace, size_t grad_workspace_bytes,
                                              float table_lr, float table_eps, float table_weight_decay,
                                              const float* table_hparams_dev, tt_stream stream);
/* The deferred finish on its own (sparse mode: out = grad_rows [M, E]) -- for a consumer other than the fused optimiser. */
int tt_embed_grad_finish(tt_ctx* ctx, int32_t E, const int32_t* seg_offsets, int64_t M, float* out, void* workspace,
                         size_t workspace_bytes, tt_stream stream);

/* ------------------------------------------------------------------------------------------------
 * Tower MLP -- replaces BaseTower.forward after the lookup (src/towers/tower/base_tower.py:133-145)
 * and its autograd backward:
 *   x[:, 0:h0]      = dense W_proj^T + b_proj                 (:133; x[:, h0:] holds the lookup rows)
 *   per hidden i    : a = relu(in W_i^T + b_i); BatchNorm1d(a) (train: batch stats, biased var,
 *                     eps 1e-5, running stats momentum 0.1 with unbiased var; eval: running stats);
 *                     Dropout(p) in train mode (counter-based mask from `seed`)        (:88-93)
 *   y = h W_out^T + b_out ;  emb = y / max(||y||_2, 1e-12)                             (:97, :145)
 * ---------------------------------------------------------------------------------------------- */
typedef struct tt_tower_params {
  int32_t din, h0, kcat_e, n_hidden, d_out;
  int32_t hidden[TT_MAX_HIDDEN]; /* output width of hidden block i */
  const float* w_proj;           /* [h0, din] */
  const float* b_proj;           /* [h0] */
  const float* w[TT_MAX_HIDDEN]; /* [hidden[i], in_i], in_0 = h0 + kcat_e, in_i = hidden[i-1] */
  const float* b[TT_MAX_HIDDEN];
  const float* bn_w[TT_MAX_HIDDEN];
  const float* bn_b[TT_MAX_HIDDEN];
  float* bn_rm[TT_MAX_HIDDEN]; /* running_mean, updated by the train-mode forward */
  float* bn_rv[TT_MAX_HIDDEN]; /* running_var */
  int64_t* bn_nbt[TT_MAX_HIDDEN]; /* num_batches_tracked (+1 per train-mode forward); may be NULL */
  const float* w_out;          /* [d_out, in_last] */
  const float* b_out;
  int32_t compute_dtype; /* TT_F32: exact-f32 MFMA (parity); TT_BF16: GEMM operands rounded to bf16 (RNE) on the way
                            into LDS, f32 accumulate on v_mfma_f32_32x32x16_bf16 */
  int32_t x_dtype;       /* element type of tt_tower_acts.x  (TT_BF16 only with compute_dtype TT_BF16: the GEMMs that read x
                            round it to bf16 anyway, so results are bit-identical and x costs half the HBM bytes) */
  int32_t dx_dtype;      /* element type of tt_tower_grads.d_x (TT_BF16 only with compute_dtype TT_BF16; the per-slot row
                            gradients are then rounded to bf16 before tt_embed_grad_bwd sums them in f32) */
  int32_t flags;         /* TT_TOWER_*: 0 by default */
  /* Data-parallel BatchNorm over several ranks (SyncBN): the pass is cut at the batch-wide reduction so that the caller
   * can exchange the statistics in between (the library makes no collective calls).
   *   sync_phase 0: the whole pass (default).
   *   sync_phase 1: forward up to the local BN statistics -> acts.bn_sync_local [3][H] = (n, mean, M2) per column;
   *                 backward up to the local column sums   -> grads.s_sync_local [2][H] = (S1, S2).
   *   sync_phase 2: the rest, with the statistics of ALL ranks as acts.bn_sync_all [sync_ranks][3][H] (merged in rank
   *                 order with Chan's formula) / grads.s_sync_all [sync_ranks][2][H] (added in rank order); BN normalises
   *                 over sync_ranks * B rows, and the BN weight / bias gradients -- identical on every rank -- are stored
   *                 divided by sync_ranks so that the caller's SUM over ranks of the dense gradients leaves them right.
   * Phases 1 / 2 need a training pass over towers with exactly ONE hidden block (any width, either compute_dtype: the
   * reference's [128, 64] -> 64 on the fused tail kernels, scripts/train.py's [512, 256] -> 128 on the separate ones);
   * anything else returns TT_ERR_UNSUPPORTED. */
  int32_t sync_phase;
  int32_t sync_ranks;
  int64_t rng_row_offset; /* first global row of this rank's batch: dropout masks are drawn per GLOBAL (row, column), so a
                             split batch drops the same elements as the whole one */
  /* Optional bf16 SHADOWS of w_proj / w[i] (same shapes, RNE of the f32 values; NULL = none): the one-launch front reads them
   * instead of the f32 weights -- every 64-row workgroup re-reads its tower's weights, and the f32 copies are two thirds of the bytes
   * it moves.  The caller keeps them equal to bf16(w) (a captured step: refreshed by the hand-over launch, tt_cvt_list); results
   * are bit-identical to the f32 path, which rounds the same values on the way into LDS. */
  const void* w_proj_bf16;
  const void* w_bf16[TT_MAX_HIDDEN];
} tt_tower_params;
/* run the tail of a training pass (BN of the last block, output Linear, L2 normalise) as the separate kernels even when
   the fused form applies (last hidden width and d_out <= 64, compute_dtype TT_BF16): for A/B comparison */
#define TT_TOWER_UNFUSED_TAIL 1
#define TT_TOWER_UNFUSED_FRONT 2 /* keep projection GEMM, block GEMM and slab/statistics pass as separate launches */
#define TT_TOWER_UNFUSED_BACK 4  /* first-block weight / data gradients and the projection's weight gradient as separate launches */
#define TT_TOWER_UNFUSED_GATHER 8 /* never gather the embedding rows in the one-launch front (tt_towers_fwd_gathers answers 0) */

typedef struct tt_tower_acts { /* caller-allocated; kept between forward and backward */
  const float* dense;          /* [B, din] */
  void* x;                     /* [B, h0 + kcat_e] of params.x_dtype */
  float* pre[TT_MAX_HIDDEN];   /* [B, hidden[i]] Linear output before ReLU */
  float* act[TT_MAX_HIDDEN];   /* [B, hidden[i]] block output (after BN and dropout) */
  float* mean[TT_MAX_HIDDEN];  /* [hidden[i]] statistics used by BN in this pass */
  float* rstd[TT_MAX_HIDDEN];
  float* y;   /* [B, d_out] before normalisation */
  float* emb; /* [B, d_out] unit rows */
  void* emb_packed; /* optional, tt_score_pack_bytes(B, d_out) bytes, 16-byte aligned: on return also holds the score kernels'
                       bf16 operand images of emb (what tt_score_pack_bf16 would produce) -- written by the fused tail kernel
                       itself where that applies, by the pack kernel otherwise */
  float emb_pack_scale; /* the images hold bf16(emb_pack_scale * emb) (0 = 1): tt_score_pack_bf16's `scale` */
  float* bn_sync_local;     /* sync_phase 1 out: [3][hidden[0]] */
  const float* bn_sync_all; /* sync_phase 2 in:  [sync_ranks][3][hidden[0]] */
  int64_t bn_sync_stride;   /* floats between two ranks' triples in bn_sync_all (0 = 3 * hidden[0]): lets one all-gather
                               carry every tower's statistics */
  /* Optional: the forward GATHERS x[:, h0:] itself, inside the one-launch front, instead of finding it filled by a lookup
   * launch (all zero = x is already filled).  gather_rows are this tower's fused table rows in slot order, [B][gather_K] int32
   * (its slice of what tt_embed_lookup_rows_fwd reads); x[b, h0 + k E + e] = bf16(gather_table[gather_rows[b][k]][e]) -- the bits
   * that lookup stores -- and x is written whole, as before.  Only passes for which tt_towers_fwd_gathers() answers 1 take
   * these fields; any other pass returns TT_ERR_UNSUPPORTED when they are set. */
  const float* gather_table;  /* [rows][gather_E] f32, 16-byte aligned */
  const int32_t* gather_rows;
  int32_t gather_K;           /* keys of this tower: gather_K * gather_E == params.kcat_e */
  int32_t gather_E;           /* 8, 16, ... 256 */
} tt_tower_acts;

typedef struct tt_tower_grads { /* every buffer is overwritten, not accumulated */
  float* w_proj;
  float* b_proj;
  float* w[TT_MAX_HIDDEN];
  float* b[TT_MAX_HIDDEN];
  float* bn_w[TT_MAX_HIDDEN];
  float* bn_b[TT_MAX_HIDDEN];
  float* w_out;
  float* b_out;
  void* d_x;                     /* [B, h0 + kcat_e] of params.dx_dtype; columns [h0, ..) feed tt_embed_grad_bwd.  Columns [0, h0)
                                    (the projection output's gradient) are scratch: the bf16 path with edge-free shapes does not write them */
  float* scratch[TT_MAX_HIDDEN]; /* [B, hidden[i]] */
  float* d_y;                    /* [B, d_out] */
  float* s_sync_local;     /* sync_phase 1 out: [2][hidden[0]] */
  const float* s_sync_all; /* sync_phase 2 in:  [sync_ranks][2][hidden[0]] */
  int64_t s_sync_stride;   /* floats between two ranks' pairs in s_sync_all (0 = 2 * hidden[0]) */
} tt_tower_grads;

/* scratch for either pass (split-K slabs of the weight gradients, column-reduction partials) */
size_t tt_tower_workspace_bytes(const tt_tower_params* p, int64_t B);
/* seed_dev (may be NULL): when set, the dropout seed is read from device memory (seed + *seed_dev), so a
 * captured launch draws a new mask on every replay once the caller updates that word. */
int tt_tower_mlp_fwd(tt_ctx* ctx, const tt_tower_params* p, const tt_tower_acts* a, int64_t B,
                     int32_t train, float dropout_p, uint64_t seed, const uint64_t* seed_dev,
                     void* workspace, size_t workspace_bytes, tt_stream stream);
int tt_tower_mlp_bwd(tt_ctx* ctx, const tt_tower_params* p, const tt_tower_acts* a,
                     const float* d_emb, const tt_tower_grads* g, int64_t B, int32_t train,
                     float dropout_p, uint64_t seed, const uint64_t* seed_dev, void* workspace,
                     size_t workspace_bytes, tt_stream stream);

/* The same two passes for n towers (1..TT_MAX_SIDES) with ONE launch per layer step: every kernel takes the
 * towers' argument blocks side by side and blockIdx selects the tower ("horizontal fusion" -- each tower alone
 * fills at most half of the 256 CUs).  All towers share B and the number of hidden blocks; widths may differ.
 * Arrays are HOST arrays of n pointers; workspaces[t] >= tt_tower_workspace_bytes(p[t], B). */
int tt_towers_mlp_fwd(tt_ctx* ctx, int32_t n, const tt_tower_params* const* p, const tt_tower_acts* const* a,
                      int64_t B, int32_t train, float dropout_p, uint64_t seed, const uint64_t* seed_dev,
                      void* const* workspaces, const size_t* workspace_bytes, tt_stream stream);
/* 1 if tt_towers_mlp_fwd on exactly these arguments (gather fields of every a[t] filled in) runs the gathering front and so
 * needs no lookup launch in front of it; 0 otherwise -- then the caller clears the fields and looks the rows up as before.
 * It asks for: a training pass with sync_phase 0 that takes the one-launch front (ONE hidden block <= 64 wide, d_out <= 64,
 * bf16 compute and x, din and h0 + kcat_e multiples of 64, h0 a multiple of 32 <= 128), bf16 weight shadows on every tower,
 * gather_E a power of two in 8..256, gather_K * gather_E == kcat_e, gather_K <= 152 (the index tile fits the CU's LDS), a
 * 16-byte-aligned table, and TT_TOWER_UNFUSED_GATHER on no tower.  No device work. */
int tt_towers_fwd_gathers(int32_t n, const tt_tower_params* const* p, const tt_tower_acts* const* a, int64_t B, int32_t train);
int tt_towers_mlp_bwd(tt_ctx* ctx, int32_t n, const tt_tower_params* const* p, const tt_tower_acts* const* a,
                      const float* const* d_emb, const tt_tower_grads* const* g, int64_t B, int32_t train,
                      float dropout_p, uint64_t seed, const uint64_t* seed_dev, void* const* workspaces,
                      const size_t* workspace_bytes, tt_stream stream);

/* ------------------------------------------------------------------------------------------------
 * In-batch-negative score + symmetric softmax cross-entropy, never materialising the score matrix
 * -- replaces TwoTowerTrainTask._compute_similarity_matrix / _compute_loss / _compute_metrics
 * (src/towers/two_tower_train_task.py:99-134, :162-179), the argmax checks of
 * _verify_positive_pair_alignment (:253-276) and, through the diagonal ranks, the evaluator's
 * Recall@K / MRR (src/evaluation/evaluator.py:20-71).
 *
 * One direction:  for every row a of A[Ra, D] against all rows of Bm[Rb, D], s = <a, b> * inv_t,
 * positive column = a + diag_offset:
 *   sumexp[a] = sum_b exp(s_ab - shift)        (shift >= max s; unit rows => shift = inv_t)
 *   diag[a]   = s at the positive column
 *   rank[a]   = #{b: s_ab > diag} + #{b < positive: s_ab == diag}   (0 <=> torch.argmax hits)
 * The loss needs direction (N,C) and direction (C,N); tt_score_loss_finish combines them:
 *   out[0]=loss  out[1]=accuracy  out[2]=pos mean  out[3]=neg mean  out[4]=gap
 *   out[5]=column-direction top-1 rate  out[6]=sum of all scores;  loss_out[0] = loss (own tensor for autograd)
 * ---------------------------------------------------------------------------------------------- */
int tt_score_dir_fwd(tt_ctx* ctx, const float* A, const float* Bm, int64_t Ra, int64_t Rb, int32_t D,
                     float inv_t, float shift, int64_t diag_offset, float* sumexp, float* diag,
                     int32_t* rank, float* sumscore /* [Ra] sum_b s_ab, may be NULL */,
                     tt_stream stream);
int tt_score_loss_finish(tt_ctx* ctx, int64_t B, float shift, const float* rowsum,
                         const float* colsum, const float* diag, const int32_t* row_rank,
                         const int32_t* col_rank, const float* sumscore, float* out8,
                         float* loss_out /* [1], may be NULL */, tt_stream stream);
/* gradient of one direction's operand:
 *   dA[a] = d_loss[0] * scale * sum_b (e_ab/sumexp_a[a] + e_ab/sumexp_b[b] - 2[b == a+diag_offset]) Bm[b]
 * with e_ab = exp(s_ab - shift) and scale = inv_t / (2 * batch); call once for (N,C) -> dN and once
 * for (C,N) -> dC.  D <= 256. */
int tt_score_dir_bwd(tt_ctx* ctx, const float* A, const float* Bm, int64_t Ra, int64_t Rb, int32_t D,
                     float inv_t, float shift, int64_t diag_offset, const float* sumexp_a,
                     const float* sumexp_b, const float* d_loss, float scale, float* dA,
                     tt_stream stream);
/* ---- bf16 fast path of the same three steps: operands rounded to bf16 (round-to-nearest-even), f32
 * accumulation on v_mfma_f32_32x32x16_bf16, exp/log in f32.  tt_score_pack_bf16 writes the two bf16
 * operand images of X[R, D] (row-major, and fragment-ordered for the gradient product) into `packed`
 * (tt_score_pack_bytes(R, D) bytes, 16-byte aligned); the fwd / bwd calls take packed operands and
 * process one or two directions in ONE launch (the loss needs (N,C) and (C,N)).  D <= 256. */
typedef struct tt_score_fwd_dir {
  const void* A_packed;
  const void* B_packed;
  int64_t Ra, Rb, diag_offset;
  float* sumexp; /* [Ra] */
  float* diag;     /* [Ra] or NULL */
  int32_t* rank;   /* [Ra] or NULL */
  float* sumscore; /* [Ra] sum_b s_ab, or NULL */
  int32_t rank_mode; /* with rank != NULL: 0 or 2 = full rank; 1 = top-1 flag only (rank = 0 if the positive is the
                        row's argmax, first index winning ties, else 1) -- what the training metrics need, at a
                        quarter of the per-element work */
  float ab_scale;    /* product of the scales the two operand images were packed with (0 = 1).  When it equals
                        tt_score_unit_scale(inv_t) in EVERY direction of a call, the kernels run their "unit" form: the softmax
                        term is exp2(acc) -- one VALU op less per score -- and the fixed shift's factor goes onto the finished
                        sums.  Results (sums, diagonal, ranks, gradients) are scale-free either way. */
  float* inv_sumexp; /* [Ra] or NULL: the reciprocal tt_score_bwd_bf16 multiplies by (its inv_a / inv_b): with it the backward
                        kernel takes no reciprocals in its tile loop.  Valid for a backward call with the same ab_scale. */
} tt_score_fwd_dir;
typedef struct tt_score_bwd_dir {
  const void* A_packed;
  const void* B_packed;
  int64_t Ra, Rb, diag_offset;
  const float* sumexp_a; /* [Ra] */
  const float* sumexp_b; /* [Rb], 16-byte aligned */
  float* dA;             /* [Ra, D] f32 */
  float ab_scale;        /* as in tt_score_fwd_dir */
  float b_scale;         /* scale of the B image alone (0 = 1): dA is divided by it */
  /* sumexp_b and inv_b are read a whole 32-row tile at a time: [round_up(Rb, 32)] readable floats, the entries past Rb
     finite (and non-zero in sumexp_b); 16-byte aligned */
  const float* inv_a;    /* [Ra] / [Rb] or NULL: tt_score_fwd_dir.inv_sumexp of the A rows' direction and of the B rows' */
  const float* inv_b;    /* direction (16-byte aligned); NULL = reciprocals of sumexp_a / sumexp_b are taken in the kernel */
} tt_score_bwd_dir;
size_t tt_score_pack_bytes(int64_t R, int32_t D);
/* `scale` (0 = 1): the image holds bf16(scale * X).  Packing ONE of the two towers with tt_score_unit_scale(inv_t) =
 * inv_t * log2(e) folds the softmax's exponent scale into the MFMA (see tt_score_fwd_dir.ab_scale). */
float tt_score_unit_scale(float inv_t);
int tt_score_pack_bf16(tt_ctx* ctx, const float* X, int64_t R, int32_t D, float scale, void* packed, tt_stream stream);
/* two operands in one launch (the notice and company embeddings of a step) */
int tt_score_pack2_bf16(tt_ctx* ctx, const float* X0, int64_t R0, void* packed0, const float* X1, int64_t R1,
                        void* packed1, int32_t D, float scale0, float scale1, tt_stream stream);
int tt_score_fwd_bf16(tt_ctx* ctx, const tt_score_fwd_dir* dirs, int32_t n_dirs, int32_t D, float inv_t,
                      float shift, tt_stream stream);
int tt_score_bwd_bf16(tt_ctx* ctx, const tt_score_bwd_dir* dirs, int32_t n_dirs, int32_t D, float inv_t,
                      float shift, const float* d_loss, float scale, tt_stream stream);
/* Single-pass symmetric forward of the SQUARE training problem (B notice rows against the B company rows of the same
 * pairs; replaces two_tower_train_task.py:99-179's mm + two cross-entropies + metrics): every 32 x 32 tile of S is computed
 * once and feeds both softmax directions.  Inputs: the two packed operand images (tt_score_pack_bf16 / the tower pass);
 * ab_scale as tt_score_fwd_dir.ab_scale.  Outputs: rowsum / colsum / inv_row / inv_col are [round_up(B, 64)] (the entries past B
 * are written too -- 1 and 0 -- so that they can go straight into tt_score_bwd_bf16), diag and row_rank [B]: rowsum / colsum (shifted exp-sums, as tt_score_fwd_bf16's
 * sumexp of the two directions), inv_row / inv_col (tt_score_fwd_dir.inv_sumexp of the two directions: what
 * tt_score_bwd_bf16 takes as inv_a / inv_b), diag (s_ii / T), row_rank (want_rank != 0: 0 where the positive is the row's
 * first maximum, else 1); out8 / loss_out as tt_score_loss_finish (out8[5], the column-direction top-1 rate, is 0 here).
 * Three launches (sweep, per-row finish, scalar finish), every sum in a fixed order: bitwise reproducible.
 * workspace: tt_score_fwd_sym_workspace_bytes(B, D) bytes. */
size_t tt_score_fwd_sym_workspace_bytes(int64_t B, int32_t D);
int tt_score_fwd_sym_bf16(tt_ctx* ctx, const void* N_packed, const void* C_packed, int64_t B, int32_t D, float inv_t,
                          float shift, float ab_scale, int32_t want_rank, float* rowsum, float* colsum, float* inv_row,
                          float* inv_col, float* diag, int32_t* row_rank, float* out8, float* loss_out, void* workspace,
                          size_t workspace_bytes, tt_stream stream);
/* fp8 (OCP e4m3) form of the score kernels -- BASELINE.json configs[4] (final_embedding_dim 256, batch 65536): the S products
 * run on v_mfma_scale_f32_32x32x64_f8f6f4 (twice the bf16 MFMA rate), f32 accumulate; softmax and loss as on the bf16 path.
 * Per-tensor scale: the images hold fp8(64 * scale * x), the factor 2^6 leaves again through the instruction's block scales,
 * so ab_scale / b_scale mean what they mean in the bf16 calls.  tt_score_pack2_fp8 writes, per operand, the fp8 rows image,
 * the bf16 fragment image and the fp8 fragment image (tt_score_pack_fp8_bytes(R, D) bytes, 16-byte aligned).
 * tt_score_fwd_sym_fp8 = tt_score_fwd_sym_bf16 on such operands (same workspace).  tt_score_bwd_fp8 = tt_score_bwd_bf16 on such
 * operands, always in the workgroup-staged form, with the gradient products dA = W B
 *   TT_OPT_FP8_GRAD 1 (default): on the fp8 MFMA as well, K = 64 b rows per instruction.  The softmax weights
 *     w_ab = e_ab (1/rowsum_a + 1/colsum_b) of row a and of one BLOCK of 32 consecutive b rows (32 k .. 32 k + 31) are divided
 *     by 2^(floor(log2 m) - 7), m the block's largest weight, and rounded to e4m3 (nearest even); the power of two goes into
 *     the instruction as the block's scale.  The diagonal's weight w_aa - 2 stays out of the block (f32) and multiplies the
 *     bf16 image's row: dA[a] = sum_b q(w_ab) B8[b] + (w_aa - 2) B16[pos_a].
 *   TT_OPT_FP8_GRAD 0: bf16 weights x bf16 operand images, as tt_score_bwd_bf16.
 * Tolerance: tests/test_gpu_parity.py::test_score_fp8_vs_rounded_oracle (the f64 oracle with the same roundings). */
size_t tt_score_pack_fp8_bytes(int64_t R, int32_t D);
int tt_score_pack2_fp8(tt_ctx* ctx, const float* X0, int64_t R0, void* packed0, const float* X1, int64_t R1,
                       void* packed1, int32_t D, float scale0, float scale1, tt_stream stream);
int tt_score_fwd_sym_fp8(tt_ctx* ctx, const void* N_packed, const void* C_packed, int64_t B, int32_t D, float inv_t,
                         float shift, float ab_scale, int32_t want_rank, float* rowsum, float* colsum, float* inv_row,
                         float* inv_col, float* diag, int32_t* row_rank, float* out8, float* loss_out, void* workspace,
                         size_t workspace_bytes, tt_stream stream);
int tt_score_bwd_fp8(tt_ctx* ctx, const tt_score_bwd_dir* dirs, int32_t n_dirs, int32_t D, float inv_t,
                     float shift, const float* d_loss, float scale, tt_stream stream);
/* bf16x3 (split-bf16) form of the score kernels: near-f32 products on the bf16 MFMA.  Each f32 operand x (after its scale) is
 * written as hi + lo, hi = bf16(x), lo = bf16(x - hi) (round-to-nearest-even), and every product a b as
 * hi_a hi_b + hi_a lo_b + lo_a hi_b: three v_mfma_f32_32x32x16_bf16 chains into one f32 accumulator, in the fixed order
 * (hi_b lo_a, lo_b hi_a, hi_b hi_a).  Error per product term <= ~3 * 2^-16 |a b| (the dropped lo lo term and the two
 * residuals) against 2 * 2^-11 for TF32 operands and 2 * 2^-8 for bf16.  Softmax, loss, temperature limit (2/T <= 80) and fixed
 * shift as the bf16 calls.
 * Layout: tt_score_pack2_bf16x3 writes [hi image | lo image], each tt_score_pack_bytes(R, D) bytes in tt_score_pack_bf16's
 * layout (tt_score_pack_x3_bytes(R, D) = twice that, 16-byte aligned); the hi image is bit-identical to tt_score_pack2_bf16's,
 * padding is zero in both; `scale` as there (applied before the split).
 * tt_score_fwd_sym_bf16x3 = tt_score_fwd_sym_bf16 on such operands (same workspace); tt_score_fwd_bf16x3 = tt_score_fwd_bf16
 * (square and rectangular directions); tt_score_bwd_bf16x3 = tt_score_bwd_bf16: S recomputed as above, the f32 softmax
 * weights split in registers (w_hi = bf16(w), w_lo = bf16(w - w_hi)), dA += w_hi B_lo + w_lo B_hi + w_hi B_hi.  Shapes:
 * 1 <= D <= 256, any B >= 1 (ragged tails).  No host synchronisation; every sum in a fixed order: bitwise reproducible.
 * Tolerance: tests/test_gpu_score_bf16x3.py (against the f64 oracle and the TF32-rounded oracle). */
size_t tt_score_pack_x3_bytes(int64_t R, int32_t D);
int tt_score_pack2_bf16x3(tt_ctx* ctx, const float* X0, int64_t R0, void* packed0, const float* X1, int64_t R1,
                          void* packed1, int32_t D, float scale0, float scale1, tt_stream stream);
int tt_score_fwd_sym_bf16x3(tt_ctx* ctx, const void* N_packed, const void* C_packed, int64_t B, int32_t D, float inv_t,
                            float shift, float ab_scale, int32_t want_rank, float* rowsum, float* colsum, float* inv_row,
                            float* inv_col, float* diag, int32_t* row_rank, float* out8, float* loss_out, void* workspace,
                            size_t workspace_bytes, tt_stream stream);
int tt_score_fwd_bf16x3(tt_ctx* ctx, const tt_score_fwd_dir* dirs, int32_t n_dirs, int32_t D, float inv_t,
                        float shift, tt_stream stream);
int tt_score_bwd_bf16x3(tt_ctx* ctx, const tt_score_bwd_dir* dirs, int32_t n_dirs, int32_t D, float inv_t,
                        float shift, const float* d_loss, float scale, tt_stream stream);
/* ---- logQ sampling-bias correction of the in-batch softmax (Yi et al., RecSys 2019) ----------------------------------
 * A batch is a uniform draw of PAIRS, so an entity is sampled as a negative in proportion to its pair count and the plain
 * in-batch softmax pushes frequent entities down hardest.  With lqN[a] / lqC[b] the log sampling probabilities (<= 0) of the
 * batch's notice a and company b, and s_ab = <n_a, c_b> / T:
 *   row direction     s^_ab  = s_ab - lqC[b]        column direction   s^'_ab = s_ab - lqN[a]
 *   loss = 0.5 * [ mean_a (logsumexp_b s^_ab - s^_aa) + mean_b (logsumexp_a s^'_ab - s^'_bb) ]      (the positive corrected too)
 *   d loss / d s_ab = (1 / 2B) [ softmax_row(s^)_ab + softmax_col(s^')_ab - 2 [a == b] ]
 * Numeric form: on the fixed-shift sums of the plain entries, the row sums add e_ab w_b and the column sums e_ab u_a with
 * the sampling weights w_b = exp(-40 - lqC[b]), u_a = exp(-40 - lqN[a]) in [e^-40, 1] (lq CLAMPED to [-40, 0] first:
 * lq < -40 counts as -40, lq > 0 as 0; the constant 40 cancels in every softmax, so nothing overflows).  The loss uses
 * log w = -40 - lq exactly.  The smallest term, e^(-2/T - 40), must stay a normal float: the *_lq entries support 2/T <= 40
 * (T >= 0.05) and return TT_ERR_UNSUPPORTED above that.  Metrics (out8, diag, ranks) stay on the RAW scores -- serving
 * ranks raw scores -- and are bitwise those of the plain entry; only rowsum / colsum / inv_* / the loss / the gradients
 * change.  Per-row arrays: f32, device, 16-byte aligned.  bf16 / bf16x3 operands and the f32 parity path; no fp8 form.
 *
 * tt_score_fwd_sym_bf16_lq / _bf16x3_lq = tt_score_fwd_sym_bf16 / _bf16x3 plus lq_n / lq_c [B] (inputs) and w_n / w_c
 * [round_up(B, 64)] (outputs: u / w above per row, 0 past B) -- the backward's sampling weights.  rowsum / colsum / inv_row /
 * inv_col are the corrected sums (scaled by the constant e^-40).
 * tt_score_bwd_bf16_lq / _bf16x3_lq = tt_score_bwd_bf16 / _bf16x3 plus, per direction, the sampling weights of its A rows and
 * of its B rows (tt_score_bwd_lq: the forward's w_n / w_c -- direction (N, C): {w_n, w_c}, direction (C, N): {w_c, w_n});
 * the inv / sumexp arrays must be the _lq forward's.  Weight of (a, b): e_ab (w_b / rowsum_a + w_a / colsum_b).
 * tt_score_dir_fwd_lq = tt_score_dir_fwd with sumexp[a] = sum_b exp(s_ab - shift) exp(-40 - lq_b[b]) (lq_b [Rb]: the B rows'
 * log probabilities); tt_score_loss_finish_lq = tt_score_loss_finish with the corrected positives (lq_n, lq_c [B]);
 * tt_score_dir_bwd_lq = tt_score_dir_bwd with the weight exp(s_ab - shift) (w_b / sumexp_a[a] + w_a / sumexp_b[b]), w from
 * lq_a [Ra] / lq_b [Rb] as above. */
typedef struct tt_score_bwd_lq {
  const float* w_a; /* [Ra] sampling weights of the direction's A rows */
  const float* w_b; /* [round_up(Rb, 32)] of its B rows, read a whole 32-row tile at a time (entries past Rb finite); 16-byte aligned */
} tt_score_bwd_lq;
int tt_score_fwd_sym_bf16_lq(tt_ctx* ctx, const void* N_packed, const void* C_packed, int64_t B, int32_t D, float inv_t,
                             float shift, float ab_scale, int32_t want_rank, const float* lq_n, const float* lq_c, float* rowsum,
                             float* colsum, float* inv_row, float* inv_col, float* w_n, float* w_c, float* diag,
                             int32_t* row_rank, float* out8, float* loss_out, void* workspace, size_t workspace_bytes,
                             tt_stream stream);
int tt_score_fwd_sym_bf16x3_lq(tt_ctx* ctx, const void* N_packed, const void* C_packed, int64_t B, int32_t D, float inv_t,
                               float shift, float ab_scale, int32_t want_rank, const float* lq_n, const float* lq_c,
                               float* rowsum, float* colsum, float* inv_row, float* inv_col, float* w_n, float* w_c,
                               float* diag, int32_t* row_rank, float* out8, float* loss_out, void* workspace,
                               size_t workspace_bytes, tt_stream stream);
int tt_score_bwd_bf16_lq(tt_ctx* ctx, const tt_score_bwd_dir* dirs, const tt_score_bwd_lq* lq, int32_t n_dirs, int32_t D,
                         float inv_t, float shift, const float* d_loss, float scale, tt_stream stream);
int tt_score_bwd_bf16x3_lq(tt_ctx* ctx, const tt_score_bwd_dir* dirs, const tt_score_bwd_lq* lq, int32_t n_dirs, int32_t D,
                           float inv_t, float shift, const float* d_loss, float scale, tt_stream stream);
int tt_score_dir_fwd_lq(tt_ctx* ctx, const float* A, const float* Bm, int64_t Ra, int64_t Rb, int32_t D, float inv_t,
                        float shift, int64_t diag_offset, const float* lq_b, float* sumexp, float* diag, int32_t* rank,
                        float* sumscore, tt_stream stream);
int tt_score_loss_finish_lq(tt_ctx* ctx, int64_t B, float shift, const float* lq_n, const float* lq_c, const float* rowsum,
                            const float* colsum, const float* diag, const int32_t* row_rank, const int32_t* col_rank,
                            const float* sumscore, float* out8, float* loss_out, tt_stream stream);
int tt_score_dir_bwd_lq(tt_ctx* ctx, const float* A, const float* Bm, int64_t Ra, int64_t Rb, int32_t D, float inv_t,
                        float shift, int64_t diag_offset, const float* lq_a, const float* lq_b, const float* sumexp_a,
                        const float* sumexp_b, const float* d_loss, float scale, float* dA, tt_stream stream);
/* ---- repeated-entity mask of the in-batch softmax (TFRS: remove_accidental_hits) ---------------------------------------
 * A notice has many bidders, so one batch holds several pairs of the same notice (and of the same company): row a's other
 * known bidders, and exact copies of its positive, sit in its denominator as negatives.  With ent_n[i] / ent_c[i] the notice
 * and the company that row i of the batch stands for (any int32 values are ordinary ids), a pair (a, b), a != b, is MASKED iff
 * ent_n[a] == ent_n[b] or ent_c[a] == ent_c[b]; the diagonal never is.  The mask is symmetric.  A masked pair adds nothing to
 * row a's sum nor to column b's and gets zero softmax weight; a row whose negatives are all masked keeps its positive term, so
 * no sum is ever zero.  With M the mask and R / C the row- / column-direction logits (S, or the logQ-corrected ones above):
 *   loss = 0.5 * [ mean_a (lse_b R.masked_fill(M, -inf)[a, :] - R[a, a]) + mean_b (lse_a C.masked_fill(M, -inf)[:, b] - C[b, b]) ]
 *   d loss / d s_ab = (1 / 2B) [ softmax_row(R')_ab + softmax_col(C')_ab - 2 [a == b] ]
 * Metrics (out8[1:], diag, ranks) stay on the RAW scores, bitwise those of the plain entry; rowsum / colsum / inv_* / the loss /
 * the gradients change.  tt_score_loss_finish / _lq serve unchanged (the positive term is never masked).
 * One set of entries: ent_n / ent_c (int32, device, [round_up(B, 64)] readable, 16-byte aligned, entries past B ignored) plus
 * OPTIONAL logQ arguments -- NULL = uncorrected, non-NULL = as the *_lq entry (both or neither; then 2/T <= 40).  Square
 * problems only (Ra == Rb, diag_offset == 0, both directions the same B); bf16 operands and the f32 parity path: anything else
 * returns TT_ERR_UNSUPPORTED.
 * tt_score_fwd_sym_bf16_mask = tt_score_fwd_sym_bf16 (lq_n NULL; w_n / w_c ignored) or tt_score_fwd_sym_bf16_lq on the masked sums.
 * tt_score_bwd_bf16_mask = tt_score_bwd_bf16 (lq NULL) or tt_score_bwd_bf16_lq with zero weight for masked pairs; the inv /
 * sumexp arrays must be the masked forward's.  Always the b-split kernel form; never hosted by the towers' backward launch (a
 * queued score backward is launched in front of it).
 * tt_score_dir_fwd_mask / tt_score_dir_bwd_mask = tt_score_dir_fwd / _bwd (lq NULL) or their _lq forms, masked. */
int tt_score_fwd_sym_bf16_mask(tt_ctx* ctx, const void* N_packed, const void* C_packed, int64_t B, int32_t D, float inv_t,
                               float shift, float ab_scale, int32_t want_rank, const int32_t* ent_n, const int32_t* ent_c,
                               const float* lq_n, const float* lq_c, float* rowsum, float* colsum, float* inv_row,
                               float* inv_col, float* w_n, float* w_c, float* diag, int32_t* row_rank, float* out8,
                               float* loss_out, void* workspace, size_t workspace_bytes, tt_stream stream);
int tt_score_bwd_bf16_mask(tt_ctx* ctx, const tt_score_bwd_dir* dirs, const int32_t* ent_n, const int32_t* ent_c,
                           const tt_score_bwd_lq* lq, int32_t n_dirs, int32_t D, float inv_t, float shift,
                           const float* d_loss, float scale, tt_stream stream);
int tt_score_dir_fwd_mask(tt_ctx* ctx, const float* A, const float* Bm, int64_t Ra, int64_t Rb, int32_t D, float inv_t,
                          float shift, int64_t diag_offset, const int32_t* ent_n, const int32_t* ent_c, const float* lq_b,
                          float* sumexp, float* diag, int32_t* rank, float* sumscore, tt_stream stream);
int tt_score_dir_bwd_mask(tt_ctx* ctx, const float* A, const float* Bm, int64_t Ra, int64_t Rb, int32_t D, float inv_t,
                          float shift, int64_t diag_offset, const int32_t* ent_n, const int32_t* ent_c, const float* lq_a,
                          const float* lq_b, const float* sumexp_a, const float* sumexp_b, const float* d_loss, float scale,
                          float* dA, tt_stream stream);
/* ---- per-pair sample weights of the in-batch softmax (TFRS: sample_weight) ------------------------------------------------
 * Pair a (row a of both sides) carries a raw weight w[a].  w' = w with every entry that is not a positive finite number set
 * to 0; g_a = w'_a * B / sum(w'), all 0 when the sum is 0.  With l_a the pair's two softmax terms (row direction and column
 * direction, corrected and masked as the entries above define them):
 *   loss = (1 / B) sum_a g_a l_a                       (= sum w' l / sum w': the weighted mean)
 *   d loss / d s_ab = (1 / 2B) [ g_a softmax_row_ab + g_b softmax_col_ab - 2 g_a [a == b] ]
 * A zero-weight pair has no positive term and no softmax of its own; its rows still stand in the other pairs' sums.  rowsum /
 * colsum are the UNWEIGHTED sums, metrics (out8[1:], diag, ranks) stay on the raw scores, bitwise the plain entry's.  All-ones
 * weights give the plain loss.  Square problems, bf16 operands and the f32 parity path only; the logQ vectors and the entity ids
 * are OPTIONAL in every _pw entry (NULL = without; each pair both or neither).
 * tt_score_prepare_pw: g_out [round_up(B, 64)] (16-byte aligned; 0 past B) from w [B], one launch, fixed summation order.
 * tt_score_fwd_sym_bf16_pw: the masked symmetric forward's arguments plus g.  The loss term of row i is multiplied by g[i] and
 * inv_row[i] / inv_col[i] come out FOLDED, g[i] / rowsum_i and g[i] / colsum_i.
 * tt_score_bwd_bf16_pw: inv_a / inv_b of every direction must be that forward's folded arrays (NULL: argument error); the
 * diagonal's -2 becomes -2 g_a.  Always the b-split kernel form; never hosted by the towers' backward launch (a queued score
 * backward is launched in front of it).
 * tt_score_loss_finish_pw / tt_score_dir_bwd_pw: the f32 parity path (the directional forwards serve unchanged). */
int tt_score_prepare_pw(tt_ctx* ctx, const float* w, int64_t B, float* g_out, tt_stream stream);
int tt_score_fwd_sym_bf16_pw(tt_ctx* ctx, const void* N_packed, const void* C_packed, int64_t B, int32_t D, float inv_t,
                             float shift, float ab_scale, int32_t want_rank, const float* g, const int32_t* ent_n,
                             const int32_t* ent_c, const float* lq_n, const float* lq_c, float* rowsum, float* colsum,
                             float* inv_row, float* inv_col, float* w_n, float* w_c, float* diag, int32_t* row_rank,
                             float* out8, float* loss_out, void* workspace, size_t workspace_bytes, tt_stream stream);
int tt_score_bwd_bf16_pw(tt_ctx* ctx, const tt_score_bwd_dir* dirs, const float* g, const int32_t* ent_n,
                         const int32_t* ent_c, const tt_score_bwd_lq* lq, int32_t n_dirs, int32_t D, float inv_t, float shift,
                         const float* d_loss, float scale, tt_stream stream);
int tt_score_loss_finish_pw(tt_ctx* ctx, int64_t B, float shift, const float* g, const float* lq_n, const float* lq_c,
                            const float* rowsum, const float* colsum, const float* diag, const int32_t* row_rank,
                            const int32_t* col_rank, const float* sumscore, float* out8, float* loss_out, tt_stream stream);
int tt_score_dir_bwd_pw(tt_ctx* ctx, const float* A, const float* Bm, int64_t Ra, int64_t Rb, int32_t D, float inv_t,
                        float shift, int64_t diag_offset, const float* g, const int32_t* ent_n, const int32_t* ent_c,
                        const float* lq_a, const float* lq_b, const float* sumexp_a, const float* sumexp_b,
                        const float* d_loss, float scale, float* dA, tt_stream stream);
/* ---- shared extra negatives of the in-batch softmax (mixed negative sampling, Yang et al. 2020; DPR / ANCE hard negatives) ------
 * Besides the B company rows of its batch every notice is contrasted with M extra company rows X [M, D] (unit rows, this step's own
 * tower outputs), shared by all rows: M more COLUMNS of the row-direction softmax.  The extras have no positive and stand in no
 * column sum.  With S = N C^T / T, Z = N X^T / T and the fixed shift 1/T:
 *   row logits R[a, b] = S[a, b] - lq_c[b], Rx[a, m] = Z[a, m] - lq_x[m];  column logits as before (S[a, b] - lq_n[a])
 *   mask (ids given): in-batch pairs as the _mask entries; extra m is masked for row a iff ent_x[m] == ent_c[a] (the row's own
 *   company or a repeat of it) -- notice ids play no part for extras
 *   loss = 0.5 * [ mean_a (lse(R'[a, :] u Rx'[a, :]) - R[a, a]) + mean_b (lse_a C'[:, b] - C[b, b]) ]
 *   W = softmax over the B + M row entries (first B columns) + softmax(C', 0) - 2 I;  Wx = that row softmax's last M columns
 *   dN = (1/T)/(2B) (W C + Wx X),  dC = (1/T)/(2B) W^T N,  dX = (1/T)/(2B) Wx^T N
 * Metrics: accuracy (out8[1]) and row_rank are over the B + M raw scores, the extras BEHIND every in-batch column (a tie with an
 * extra does not beat the positive); positive / negative mean, gap, out8[6], colsum / inv_col and diag are the in-batch ones --
 * colsum and diag bit for bit those of the same call without extras.  bf16 operands and the f32 parity path.
 * Optional arguments: lq_n / lq_c (both or neither; then 2/T <= 40) with lq_x (NULL: the extras count as log q = 0); ent_n / ent_c
 * (both or neither) with ent_x (NULL: no extra is ever masked).  NULL lq_* = uncorrected, NULL ent_* = unmasked.
 *
 * tt_score_fwd_sym_bf16_xneg: tt_score_fwd_sym_bf16 (/_lq /_mask) with ONE sweep launch whose company tiles run past the in-batch
 * tiles into X_packed, a packed image of its own (tt_score_pack_bf16, scale 1) -- the extras start on a tile boundary whatever
 * B mod 32 is.  rowsum / inv_row include the extras; w_x [round_up(M, 64)] (out, 16-byte aligned): the extras' sampling weights
 * (1 without the correction, 0 past M) for the backward.  workspace: tt_score_fwd_sym_xneg_workspace_bytes(B, M, D).  Per-row
 * arrays as the _lq / _mask entries; ent_x int32 [M], lq_x f32 [M].  Bitwise reproducible.
 * tt_score_bwd_bf16_xneg: the extras' share of the backward, ONE launch over the two rectangular directions, after the square
 * backward (tt_score_bwd_bf16 / _lq / _mask on that forward's sums, which stores dN and dC): dN += (1/T)/(2B) Wx X and
 * dX = (1/T)/(2B) Wx^T N, weight of (a, m) = e_am w_x[m] inv_row[a], rounded to bf16 as the second MFMA operand.  ab_scale: the
 * scale of the notice image (the extras' image is unscaled), divided out of dX.  inv_row [round_up(B, 32)], w_x [round_up(M, 32)]
 * (16-byte aligned): that forward's; ent_c [round_up(B, 32)] / ent_x [round_up(M, 32)] (both or neither, 16-byte aligned, entries
 * past the end ignored).  `scale` = inv_t / (2 B).  Never hosted by the towers' backward launch: a queued score backward is
 * launched in front of it.
 * f32 parity path: tt_score_dir_fwd_xneg adds the extras to the row direction of tt_score_dir_fwd (/_lq /_mask): sumexp[a] +=
 * sum_m e_am w_m and rank[a] += #{m: s_am > diag[a]}, diag [B] that call's diagonal; then tt_score_loss_finish as before.
 * tt_score_dir_bwd_xneg is one rectangular direction: x_is_b != 0: A = N [Ra = B], Bm = X [Rb = M] (ent_a = ent_c, ent_b = ent_x) ->
 * dN's extra term (accumulate != 0: added to dA); x_is_b == 0: A = X, Bm = N (ent_a = ent_x, ent_b = ent_c) -> dX.  rowsum: the
 * notice rows' sums (with the extras), lq_x the extras' log probabilities or NULL. */
size_t tt_score_fwd_sym_xneg_workspace_bytes(int64_t B, int64_t M, int32_t D);
int tt_score_fwd_sym_bf16_xneg(tt_ctx* ctx, const void* N_packed, const void* C_packed, const void* X_packed, int64_t B,
                               int64_t M, int32_t D, float inv_t, float shift, float ab_scale, int32_t want_rank,
                               const int32_t* ent_n, const int32_t* ent_c, const int32_t* ent_x, const float* lq_n,
                               const float* lq_c, const float* lq_x, float* rowsum, float* colsum, float* inv_row,
                               float* inv_col, float* w_n, float* w_c, float* w_x, float* diag, int32_t* row_rank, float* out8,
                               float* loss_out, void* workspace, size_t workspace_bytes, tt_stream stream);
int tt_score_bwd_bf16_xneg(tt_ctx* ctx, const void* N_packed, const void* X_packed, int64_t B, int64_t M, int32_t D, float inv_t,
                           float shift, float ab_scale, const float* inv_row, const float* w_x, const int32_t* ent_c,
                           const int32_t* ent_x, const float* d_loss, float scale, float* dN, float* dX, tt_stream stream);
int tt_score_dir_fwd_xneg(tt_ctx* ctx, const float* N, const float* X, int64_t B, int64_t M, int32_t D, float inv_t, float shift,
                          const int32_t* ent_c, const int32_t* ent_x, const float* lq_x, const float* diag, float* sumexp,
                          int32_t* rank, tt_stream stream);
int tt_score_dir_bwd_xneg(tt_ctx* ctx, const float* A, const float* Bm, int64_t Ra, int64_t Rb, int32_t D, float inv_t, float shift,
                          int32_t x_is_b, const int32_t* ent_a, const int32_t* ent_b, const float* lq_x, const float* rowsum,
                          const float* d_loss, float scale, int32_t accumulate, float* dA, tt_stream stream);
/* ---- masked cells of the in-batch softmax: a per-step sparse list of (row, column) pairs that are never negatives ------------------
 * cells int32 [capacity, 2], rows (a, j): a in [0, B) a notice row, j in [0, B + M) a column -- j < B in-batch column j, j >= B
 * extra j - B (M = 0 without extras).  Only the first min(*count, capacity) rows are read; *count lies in DEVICE memory.  Any
 * order, duplicates allowed; cells with j == a (the positive) and cells outside the ranges are dropped.  With Omega the cleaned
 * set, R, Rx, C the row / extras / column logits of the _lq / _xneg entries:
 *   R', Rx' = R, Rx with the cells of Omega at -inf;  C' = C with the cells (a, b) of Omega, b < B, at -inf (column b loses row a)
 *   loss, W, Wx, dN, dC, dX: the _xneg formulas (the _lq / plain ones without extras) on R', Rx', C'
 * The positive is never masked, so no sum is empty.  Metrics (out8[1:], diag, row_rank) stay on the raw scores; colsum and diag of
 * a call with an empty Omega are bit for bit those of the call without cells.  bf16 operands only.
 *
 * tt_score_cells_plan: buckets the cleaned list by 32 x 32 tile pair (a / 32, j / 32); the extras' tiles start on their own boundary
 * at nT = ceil(B / 32), extra m in tile nT + m / 32, as X_packed does.  plan (out, int32, 16-byte aligned):
 * [nT * (nT + nTx) + 1] offsets, tile pairs in row-major order (notice tile, column tile), then [capacity] local codes
 * (a % 32) * 32 + (j' % 32) (j' = j, or j - B for an extra), tile pair by tile pair.  Counts and offsets are deterministic; the order
 * inside a tile pair is not (masking is idempotent).  A fixed grid over `capacity`: the call can sit in a captured graph while
 * *count and the list change between replays.  plan: tt_score_cells_plan_bytes(B, M, capacity); workspace:
 * tt_score_cells_plan_workspace_bytes(B, M) -- the tile pairs' counters, memory of the call's own (not scratch another launch of
 * the step may be using).  capacity >= 1 (a list that is always empty still needs one slot).  The two entries below take the plan's
 * `capacity` again: a span is never read past the codes array, whatever the offsets hold.
 * tt_score_fwd_sym_bf16_cells: tt_score_fwd_sym_bf16 (/_lq, /_xneg unmasked) on Omega.  X_packed NULL (then M = 0, lq_x / w_x
 * ignored) or the extras' image; lq_n / lq_c both or neither, lq_x optional with them.  workspace: tt_score_fwd_sym_workspace_bytes
 * (M = 0) or tt_score_fwd_sym_xneg_workspace_bytes.
 * tt_score_bwd_bf16_cells: the backward on that forward's sums -- the square problem (dirs as tt_score_bwd_bf16, two directions
 * (N, C) and (C, N) in this order, inv_a / inv_b optional, lq optional) and, with X_packed, the extras' two rectangular directions
 * behind it (dN +=, dX as tt_score_bwd_bf16_xneg; inv_row / w_x / dX then required).  A listed pair weighs nothing in either
 * direction.  The b-split form at every shape; never hosted by the towers' backward launch: a queued score backward is launched in
 * front of it. */
size_t tt_score_cells_plan_bytes(int64_t B, int64_t M, int64_t capacity);
size_t tt_score_cells_plan_workspace_bytes(int64_t B, int64_t M);
int tt_score_cells_plan(tt_ctx* ctx, const int32_t* cells, const int32_t* count, int64_t capacity, int64_t B, int64_t M,
                        int32_t* plan, size_t plan_bytes, void* workspace, size_t workspace_bytes, tt_stream stream);
int tt_score_fwd_sym_bf16_cells(tt_ctx* ctx, const void* N_packed, const void* C_packed, const void* X_packed, int64_t B,
                                int64_t M, int32_t D, float inv_t, float shift, float ab_scale, int32_t want_rank,
                                const int32_t* plan, int64_t capacity, const float* lq_n, const float* lq_c, const float* lq_x, float* rowsum,
                                float* colsum, float* inv_row, float* inv_col, float* w_n, float* w_c, float* w_x, float* diag,
                                int32_t* row_rank, float* out8, float* loss_out, void* workspace, size_t workspace_bytes,
                                tt_stream stream);
int tt_score_bwd_bf16_cells(tt_ctx* ctx, const tt_score_bwd_dir* dirs, const int32_t* plan, int64_t capacity, const tt_score_bwd_lq* lq,
                            const void* X_packed, int64_t M, const float* inv_row, const float* w_x, float* dX, int32_t D,
                            float inv_t, float shift, const float* d_loss, float scale, tt_stream stream);
/* Dense loss path: the loss variants the fused kernels do not cover, on the MATERIALISED score matrix --
 * label-smoothed cross-entropy (loss_type 0; two_tower_train_task.py:114-133, F.cross_entropy(label_smoothing=e) in both
 * directions) and cosine-embedding loss (loss_type 1; :135-158: F.cosine_embedding_loss of [s] against [1], positives on the
 * diagonal, negatives off it, mean over all B^2 entries).  f32 throughout, exact-f32 GEMMs, O(B^2) memory: S [B, B] (holds
 * d loss / d (N C^T) after the backward call), stats [6 B] floats and hit [2 B] int32 are caller memory kept between the calls.
 * out8 = {loss, row top-1 accuracy, positive mean, negative mean, gap, column top-1 accuracy, sum of S, 0} as
 * tt_score_loss_finish. */
size_t tt_score_dense_workspace_bytes(int64_t B, int32_t D);
int tt_score_dense_fwd(tt_ctx* ctx, const float* N, const float* Cm, int64_t B, int32_t D, float inv_t, int32_t loss_type,
                       float label_smoothing, float* S, float* stats, int32_t* hit, float* out8, float* loss_out,
                       tt_stream stream);
int tt_score_dense_bwd(tt_ctx* ctx, const float* N, const float* Cm, int64_t B, int32_t D, float inv_t, int32_t loss_type,
                       float label_smoothing, float* S, const float* stats, const float* d_loss, float* dN, float* dC,
                       void* workspace, size_t workspace_bytes, tt_stream stream);
/* dense score matrix S[Ra, Rb] = A Bm^T * inv_t (result["similarity_matrix"], predict_batch
 * "all_similarities": two_tower_train_task.py:94, :206); an empty side (Ra == 0 or Rb == 0) launches nothing and its
 * pointers may be NULL */
int tt_score_matrix(tt_ctx* ctx, const float* A, const float* Bm, int64_t Ra, int64_t Rb, int32_t D,
                    float inv_t, float* S, int64_t lds, tt_stream stream);
/* rank of the positive column of every row of a dense matrix (evaluator MRR / Recall@K on a given
 * similarity matrix: src/evaluation/evaluator.py:45-71):
 *   rank[r] = #{c: S[r,c] > S[r,r+off]} + #{c < r+off: S[r,c] == S[r,r+off]},
 *   -1 where the positive column r+off is outside [0, Ccols) (the retrieval entries' rule: such a row has no rank) */
int tt_diag_rank_rows(tt_ctx* ctx, const float* S, int64_t R, int64_t Ccols, int64_t lds,
                      int64_t diag_offset, int32_t* rank, tt_stream stream);
/* per-row top-k of a dense matrix, descending, ties -> lower column first (torch.topk use in
 * predict_batch :195 and evaluator.py:35); k <= 64.  A NaN is never selected (-inf entries are, with their own column); when a
 * row holds fewer than k non-NaN entries the remaining slots are (-inf, -1). */
int tt_topk_rows(tt_ctx* ctx, const float* S, int64_t R, int64_t Ccols, int64_t lds, int32_t k,
                 float* vals, int64_t* idx, tt_stream stream);

/* ------------------------------------------------------------------------------------------------
 * Catalogue-wide retrieval: the k best catalogue rows of every query, and optionally the rank of a given positive, in one
 * sweep over the catalogue that never writes a score to memory (what a user of the trained towers searches with; the
 * in-batch tt_score_matrix + tt_topk_rows pair only ranks the companies of one batch).
 *   queries Q [nQ, D], catalogue C [nC, D]; 1 <= D <= 256, 1 <= nC < 2^31, 0 <= k <= min(512, nC).
 *   tt_retrieve_topk_bf16: Q_packed / C_packed are tt_score_pack_bf16 images (reused as they are); the score is
 *     s(q, c) = <bf16 image row q, bf16 image row c> in f32 on v_mfma_f32_32x32x16_bf16, i.e. <Q_q, C_c> times the product of
 *     the scales the two images were packed with (pack the catalogue with inv_t and the queries with 1 for s = cos / T on
 *     L2-normalised towers; nothing is normalised here).
 *   tt_retrieve_topk_f32: plain row-major f32 Q and C; s(q, c) = inv_t * (f32 FMA chain over d = 0 .. D-1, in that order).
 * Outputs (k >= 1; vals and idx required): vals f32 [nQ, k] and idx int64 [nQ, k], per query sorted by value descending, ties
 *   to the LOWER catalogue index (tt_topk_rows's order).
 * Rank (positives != NULL, then rank != NULL, else both NULL): positives [nQ] int32 (positives_i64 = 0) or int64 (1); rank int32
 *   [nQ] = #{c : s(q,c) > s(q,p)} + #{c < p : s(q,c) == s(q,p)} (tt_diag_rank_rows's rule), -1 where p is outside [0, nC).
 *   The positive's score comes from the same instruction sequence as every other score, and the counts from the same sweep
 *   as the top-k.  k = 0 asks for ranks only (positives required).
 * Workspace: tt_retrieve_workspace_bytes(nQ, nC, D, k) bytes (0 for an invalid shape), 16-byte aligned, caller memory.  For k > 64
 *   the catalogue splits are capped so that splits x k <= 2048: the size never exceeds that of the same call with k = 64.
 * k > 64 (up to 512) runs the sweep's large-k form: same scores, order, filler and rank, one wave per workgroup with up to the
 *   CU's whole 160 KB of LDS.  A call with k <= 64 is unaffected.
 * Scores are assumed finite (a NaN score is never selected; -inf entries fill a list only when nothing better exists, idx -1).
 * Three launches on `stream` (positive scores, sweep, per-query merge), no host synchronisation and no allocation: a search
 * can be captured into a graph (one stream, no parallel branches).  Results are bitwise identical from run to run and for
 * every split count (TT_OPT_RETRIEVE_SPLITS).  A bad argument returns TT_ERR_INVALID_ARG and launches nothing.
 * ---------------------------------------------------------------------------------------------- */
size_t tt_retrieve_workspace_bytes(int64_t nQ, int64_t nC, int32_t D, int32_t k);
int tt_retrieve_topk_bf16(tt_ctx* ctx, const void* Q_packed, int64_t nQ, const void* C_packed, int64_t nC, int32_t D, int32_t k,
                          const void* positives, int32_t positives_i64, float* vals, int64_t* idx, int32_t* rank, void* workspace,
                          size_t workspace_bytes, tt_stream stream);
int tt_retrieve_topk_f32(tt_ctx* ctx, const float* Q, int64_t nQ, const float* Cm, int64_t nC, int32_t D, float inv_t, int32_t k,
                         const void* positives, int32_t positives_i64, float* vals, int64_t* idx, int32_t* rank, void* workspace,
                         size_t workspace_bytes, tt_stream stream);
/* Retrieval with per-query exclusion lists: tt_retrieve_topk_bf16 / _f32 with two more arguments after `rank`.
 *   excl_offsets int64 [nQ + 1] (excl_offsets[0] = 0, non-decreasing) and excl_rows int32 [excl_offsets[nQ]]: query q's
 *   exclusion set E_q is excl_rows[excl_offsets[q] .. excl_offsets[q+1]), ASCENDING; duplicates are allowed and rows outside
 *   [0, nC) match nothing.  Both pointers are required (8- and 4-byte aligned); a list may be empty.
 *   top-k: the k best rows of {c not in E_q} in the same order; slots beyond the eligible rows are -inf / -1.
 *   rank:  #{c not in E_q : s > s_p} + #{c not in E_q, c < p : s == s_p}; p never counts against itself, so whether p is in
 *          E_q makes no difference; -1 where p is outside [0, nC).
 * With every list empty the results are bitwise those of the plain entry; they are bitwise identical across runs and split
 * counts.  Same workspace (tt_retrieve_workspace_bytes), launches and graph capture rules as the plain entries.  A bad argument
 * returns TT_ERR_INVALID_ARG and launches nothing. */
int tt_excl_retrieve_topk_bf16(tt_ctx* ctx, const void* Q_packed, int64_t nQ, const void* C_packed, int64_t nC, int32_t D,
                               int32_t k, const void* positives, int32_t positives_i64, float* vals, int64_t* idx, int32_t* rank,
                               const int64_t* excl_offsets, const int32_t* excl_rows, void* workspace, size_t workspace_bytes,
                               tt_stream stream);
int tt_excl_retrieve_topk_f32(tt_ctx* ctx, const float* Q, int64_t nQ, const float* Cm, int64_t nC, int32_t D, float inv_t,
                              int32_t k, const void* positives, int32_t positives_i64, float* vals, int64_t* idx, int32_t* rank,
                              const int64_t* excl_offsets, const int32_t* excl_rows, void* workspace, size_t workspace_bytes,
                              tt_stream stream);
/* Retrieval with per-query attribute filters (eligibility): the exclusion entries with tags, W, q_any and q_all after `excl_rows`.
 *   tags uint32 [nC][W]: W tag words per catalogue row, 1 <= W <= 4 (up to 128 attribute bits), 16-byte aligned.
 *   q_any uint32 [nQ][W] or NULL: if any[q, :] is all zero, query q is unrestricted on this predicate; otherwise row c must share
 *     at least one bit with it: there is a w with tags[c,w] & any[q,w] != 0.
 *   q_all uint32 [nQ][W] or NULL: row c must hold every required bit: tags[c,w] & all[q,w] == all[q,w] for all w (an all-zero
 *     all[q, :] requires nothing).
 *   eligible(q, c) is the AND of the two.  A NULL mask pointer makes its predicate always true; both NULL is an argument error.
 *   The masks are 4-byte aligned.  excl_offsets and excl_rows may both be NULL here (no lists); one NULL and one not is an error.
 *   With lists, a row counts when it is eligible AND not in E_q.
 *   top-k: the k best eligible rows, value descending, ties to the lower index; slots beyond the eligible rows are -inf / -1.
 *   rank:  #{eligible c : s > s_p} + #{eligible c < p : s == s_p}; p never counts against itself, so whether p is eligible
 *          makes no difference; -1 where p is outside [0, nC).
 * (One-hot bits under `any` give "is one of these"; flag bits under `all` give "holds every one of these"; equality on a code
 * of V values is an `all` test on 2 ceil(log2 V) bits, the tag holding the code's binary digits and next to them their
 * complement, the query requiring exactly the encoding of its code and nothing for "don't care".)
 * With all-zero masks the results are bitwise those of the plain entry (with lists: of the exclusion entry); they are bitwise
 * identical across runs and split counts.  No tag of a row at or past nC is read.  Same workspace
 * (tt_retrieve_workspace_bytes), three launches on `stream`, no synchronisation, no allocation, and the graph capture rules of
 * the plain entries.  A bad argument returns TT_ERR_INVALID_ARG and launches nothing. */
int tt_filt_retrieve_topk_bf16(tt_ctx* ctx, const void* Q_packed, int64_t nQ, const void* C_packed, int64_t nC, int32_t D,
                               int32_t k, const void* positives, int32_t positives_i64, float* vals, int64_t* idx, int32_t* rank,
                               const int64_t* excl_offsets, const int32_t* excl_rows, const uint32_t* tags, int32_t W,
                               const uint32_t* q_any, const uint32_t* q_all, void* workspace, size_t workspace_bytes,
                               tt_stream stream);
int tt_filt_retrieve_topk_f32(tt_ctx* ctx, const float* Q, int64_t nQ, const float* Cm, int64_t nC, int32_t D, float inv_t,
                              int32_t k, const void* positives, int32_t positives_i64, float* vals, int64_t* idx, int32_t* rank,
                              const int64_t* excl_offsets, const int32_t* excl_rows, const uint32_t* tags, int32_t W,
                              const uint32_t* q_any, const uint32_t* q_all, void* workspace, size_t workspace_bytes,
                              tt_stream stream);
/* Retrieval under a per-query score ceiling (hard-negative mining): the exclusion entries with `ceil` after `excl_rows`.
 *   ceil f32 [nQ], required, 4-byte aligned: a row with s(q, c) >= ceil[q] never enters query q's top-k, so the k slots hold the
 *   best rows BELOW the ceiling (value descending, ties to the lower index; slots beyond them are -inf / -1).  A tie with the
 *   ceiling is removed.  ceil[q] = +inf or NaN removes nothing, -inf removes every row.
 *   rank: unchanged -- the positive's place among all rows outside E_q; the ceiling bounds the top-k only.
 *   excl_offsets and excl_rows may both be NULL (no lists); one NULL and one not is an error.
 * With every ceiling +inf the results are bitwise those of the plain entry (with lists: of the exclusion entry); they are bitwise
 * identical across runs and split counts.  Same workspace (tt_retrieve_workspace_bytes), launches and graph capture rules as the
 * plain entries.  A bad argument returns TT_ERR_INVALID_ARG and launches nothing. */
int tt_ceil_retrieve_topk_bf16(tt_ctx* ctx, const void* Q_packed, int64_t nQ, const void* C_packed, int64_t nC, int32_t D,
                               int32_t k, const void* positives, int32_t positives_i64, float* vals, int64_t* idx, int32_t* rank,
                               const int64_t* excl_offsets, const int32_t* excl_rows, const float* ceil, void* workspace,
                               size_t workspace_bytes, tt_stream stream);
int tt_ceil_retrieve_topk_f32(tt_ctx* ctx, const float* Q, int64_t nQ, const float* Cm, int64_t nC, int32_t D, float inv_t,
                              int32_t k, const void* positives, int32_t positives_i64, float* vals, int64_t* idx, int32_t* rank,
                              const int64_t* excl_offsets, const int32_t* excl_rows, const float* ceil, void* workspace,
                              size_t workspace_bytes, tt_stream stream);
/* Scores of given (query, catalogue row) pairs: out[q] = s(q, rows[q]), f32 [nQ], bit for bit the score the retrieval sweep forms
 * for that pair (the same images, scales and instruction sequence: the retrieval entries' positive-score launch, writing to the
 * caller).  rows [nQ] int32 (rows_i64 = 0) or int64 (1); NaN where rows[q] is outside [0, nC).  One launch on `stream`, no
 * workspace, no synchronisation.  Operands as tt_retrieve_topk_bf16 / _f32. */
int tt_pair_scores_bf16(tt_ctx* ctx, const void* Q_packed, int64_t nQ, const void* C_packed, int64_t nC, int32_t D,
                        const void* rows, int32_t rows_i64, float* out, tt_stream stream);
int tt_pair_scores_f32(tt_ctx* ctx, const float* Q, int64_t nQ, const float* Cm, int64_t nC, int32_t D, float inv_t,
                       const void* rows, int32_t rows_i64, float* out, tt_stream stream);

/* ------------------------------------------------------------------------------------------------
 * Generic Linear used by the one-off feature projection -- replaces FeatureProjector.forward
 * (src/torchrec_preprocess/feature_projector.py:20-28):  Y = act(X W^T + b)
 * ---------------------------------------------------------------------------------------------- */
int tt_linear_fwd(tt_ctx* ctx, const float* X, int64_t ldx, const float* W, const float* bias,
                  float* Y, int64_t ldy, int64_t M, int32_t N, int32_t K, int32_t relu,
                  tt_stream stream);

/* ------------------------------------------------------------------------------------------------
 * Batch assembly on the device -- replaces the numpy fancy-index gather of collate_fn_gpu_optimized
 * (src/towers/pairs/unified_bid_data_loader.py:630-684) and _build_batch_kjt (:827-841):
 *   dense_out[b, :] = dense_store[entity[b], :] ;  ids_out[b*K + k] = cat_store[entity[b]*K + k]
 * ---------------------------------------------------------------------------------------------- */
int tt_batch_gather(tt_ctx* ctx, const int64_t* entity, int64_t B, const float* dense_store,
                    int32_t dense_dim, const int64_t* cat_store, int32_t K, float* dense_out,
                    int64_t* ids_out, tt_stream stream);

/* ------------------------------------------------------------------------------------------------
 * Row-wise sharded tables (multi-GPU; the reference is single-process): owner(row) = row % G, local
 * index at the owner = row / G.  The U distinct rows of a duplicate-row plan are routed to their owners through
 * FIXED-CAPACITY buckets, so no size ever travels to the host and the whole exchange can sit inside a captured graph:
 *   send_ids [G, C] int32  local row index at owner g, in plan order; unused entries = pad_id[g]
 *   send_u   [G, C] int32  plan index u of each entry; unused entries = pad_u (caller: index of an all-zero row)
 *   pos_u    [M]    int32  g*C + position of plan row u; G*C for rows that did not fit -- the caller keeps row G*C of the
 *                          buffer the exchanged rows are placed from all-zero, so an overflowing step (which it must
 *                          reject: overflow[0]) never feeds a tower another row's embedding
 *   counts   [G]    int32  entries wanted per owner; overflow[0] is set to 1 when any count exceeds C (sticky: never
 *                          cleared here, the caller owns the flag)
 * tt_route_expand: idx_slot[slot] = pos_u[u] for every slot of plan row u (int64: ids of the placing lookup).
 * tt_route_bucket_expand: both in one call.
 * ---------------------------------------------------------------------------------------------- */
#define TT_MAX_RANKS 64
size_t tt_route_workspace_bytes(int64_t M, int32_t G);
int tt_route_bucket(tt_ctx* ctx, const int32_t* unique_rows, const int32_t* n_unique, int64_t M, int32_t G, int32_t C,
                    const int32_t* pad_id, int32_t pad_u, int32_t* send_ids, int32_t* send_u, int32_t* pos_u,
                    int32_t* counts, int32_t* overflow, void* workspace, size_t workspace_bytes, tt_stream stream);
int tt_route_expand(tt_ctx* ctx, const int32_t* sorted_src, const int32_t* seg_offsets, const int32_t* n_unique,
                    const int32_t* pos_u, int64_t M, int64_t* idx_slot, tt_stream stream);
int tt_route_bucket_expand(tt_ctx* ctx, const int32_t* unique_rows, const int32_t* n_unique, int64_t M, int32_t G, int32_t C,
                           const int32_t* pad_id, int32_t pad_u, int32_t* send_ids, int32_t* send_u, int32_t* pos_u,
                           int32_t* counts, int32_t* overflow, void* workspace, size_t workspace_bytes,
                           const int32_t* sorted_src, const int32_t* seg_offsets, int64_t* idx_slot, tt_stream stream);
/* Duplicate-row plan of G ASCENDING runs of C row ids each (what an owner receives: every source sends its distinct rows in
 * ascending order, pads -- the largest value -- at the end): a stable merge by binary searches instead of radix passes.
 * Same outputs as tt_dedup_plan over the concatenated runs; workspace tt_dedup_workspace_bytes(G * C).
 * row_limit > 0: ids >= row_limit are pads -- they sort to the end as ONE last group that is left out of n_unique (the
 * gradient reduction and the optimiser then never touch the thousands of pad entries); row_limit <= 0: every id counts. */
int tt_dedup_plan_runs(tt_ctx* ctx, const int32_t* rows, int32_t G, int64_t C, int64_t row_limit, int32_t* sorted_src,
                       int32_t* unique_rows, int32_t* seg_offsets, int32_t* n_unique, void* workspace,
                       size_t workspace_bytes, tt_stream stream);
/* out[i, :] = rows[i] < 0 ? 0 : table[min(rows[i], table_rows - 1), :] -- the owner's gather of requested rows and the
 * hand-over of per-row gradients into the send buckets, whose unused entries carry -1 (E a multiple of 4, 16-byte aligned
 * f32 table).  out_dtype TT_BF16: rows leave rounded to bf16 (RNE) -- bit-identical to rounding them where a bf16 tower
 * input is filled, at half the bytes on the wire. */
int tt_gather_rows(tt_ctx* ctx, const float* table, int64_t table_rows, int32_t E, const int32_t* rows, int64_t n,
                   void* out, int32_t out_dtype, tt_stream stream);

/* ------------------------------------------------------------------------------------------------
 * n (<= 8) device-to-device copies in ONE launch -- the per-step refresh of a captured step's static input
 * buffers (dense features and ids of both towers); sizes in bytes, all pointers 16-byte aligned.
 * ---------------------------------------------------------------------------------------------- */
#define TT_MAX_COPIES 8
/* f32 -> bf16 (round to nearest even) conversions that ride in a hand-over launch: dst[i][0 .. count[i]) = bf16(src[i][...]).  A captured
 * step refreshes the towers' bf16 weight shadows (tt_tower_params.w_proj_bf16 / w_bf16) this way at every hand-over, so whoever changed
 * the weights since the last step -- the captured Adam, an eager step, a checkpoint load -- the shadows are current when the replay
 * reads them.  Sources 16-byte, destinations 8-byte aligned; NULL list or n = 0: none. */
#define TT_MAX_CVT 8
typedef struct tt_cvt_list {
  int32_t n;
  int32_t reserved;
  const float* src[TT_MAX_CVT];
  void* dst[TT_MAX_CVT];
  int64_t count[TT_MAX_CVT];
} tt_cvt_list;
int tt_copy_multi(tt_ctx* ctx, int32_t n, void* const* dst, const void* const* src, const int64_t* bytes,
                  tt_stream stream);

/* Batch hand-over of a graph-replayed step in ONE launch: the n copy segments of tt_copy_multi (the batch's dense features and
 * ids into the graph's static buffers, the step scalars) and, for every side, the fused rows of the batch's ids in key-major
 * order for tt_dedup_plan_keyed_km:  rows_km[side_base + k*B + b] = key_row_offset[k] + clamp(ids[b*K + k], 0, key_vocab[k] - 1)
 * (the lookup's own id -> row rule, src/towers/cat_embed.py:114-117; side_base = sum of B*K of the earlier sides).
 * sides[i].ids is the SOURCE of the hand-over (the incoming batch); out / ld_out / out_dtype are ignored.  1 <= K <= 64 per side. */
int tt_batch_ingest(tt_ctx* ctx, int32_t n, void* const* dst, const void* const* src, const int64_t* bytes,
                    const tt_embed_side* sides, int32_t n_sides, int64_t B, int32_t* rows_km,
                    int32_t* rows_sm /* or NULL: the same rows in slot order, rows_sm[side_base + b*K + k], for tt_embed_lookup_rows_fwd */,
                    int64_t table_rows /* rows of the table the fused rows index: a row outside [0, table_rows) -- key offsets /
                                        * vocabularies of another table -- is stored as table_rows - 1 and raises TT_DEVERR_ROW_RANGE,
                                        * so no consumer of rows_km / rows_sm reads or writes out of bounds; 0: unchecked */,
                    const tt_cvt_list* cvt /* or NULL */, tt_stream stream);

/* The same hand-over STRAIGHT FROM THE DEVICE-RESIDENT FEATURE STORES (two-level gather: pair -> entity row -> dense features
 * and ids -> fused table rows) -- replaces UnifiedBidDataset.__getitem__ + collate_fn_gpu_optimized + _build_batch_kjt
 * (src/towers/pairs/unified_bid_data_loader.py:461-504, :630-684, :827-841) and the host-to-device copy of the batch
 * (scripts/train.py:261-273) with ONE launch and no intermediate batch tensors.  For side i, sample b:
 *   o = order ? order[b] : b ;  e = stores[i].entity[o * stores[i].entity_stride]      (entity row of the pair's side)
 *   dense_out[b, :]   = dense_store[e, :]                                              (f32 copy)
 *   ids_out[b*K + k]  = cat_store[e*K + k]                                             (sample-major: the KJT values())
 *   rows_km[side_base + k*B + b] = key_row_offset[k] + clamp(ids_out[b*K + k], 0, key_vocab[k] - 1)   (as tt_batch_ingest)
 * plus the n copy segments (the step scalars).  sides[i] gives K / key_row_offset / key_vocab (ids, out, ld_out, out_dtype
 * ignored); rows_km may be NULL (no key-major rows wanted).  Entity indices are expected to lie inside the stores (the
 * loader validates the pair list once: KeyError as unified_bid_data_loader.py:495-498); with stores[i].n_rows set, one that
 * does not is clamped into the store rather than read out of bounds.  Bit-identical to tt_batch_gather per
 * side followed by tt_batch_ingest (test). */
typedef struct tt_store_side {
  const int64_t* entity;     /* entity index per pair, read at [o * entity_stride] (an interleaved [P, 2] pair list: stride 2) */
  int64_t entity_stride;
  const float* dense_store;  /* [N, dense_dim] */
  const int64_t* cat_store;  /* [N, K] */
  float* dense_out;          /* [B, dense_dim] */
  int64_t* ids_out;          /* [B * K] */
  int32_t dense_dim;
  int32_t n_rows;            /* entity rows N of the store; > 0: an index outside [0, N) is clamped into it instead of read out of
                              * bounds (the loader has validated the pair list; this guards the device), 0: unchecked */
} tt_store_side;
int tt_batch_ingest_store(tt_ctx* ctx, int32_t n, void* const* dst, const void* const* src, const int64_t* bytes,
                          const tt_embed_side* sides, const tt_store_side* stores, int32_t n_sides, int64_t B,
                          const int64_t* order /* [B] or NULL */, int32_t* rows_km /* or NULL */,
                          int32_t* rows_sm /* or NULL: as tt_batch_ingest */, int64_t table_rows /* as tt_batch_ingest */,
                          const tt_cvt_list* cvt /* or NULL */, tt_stream stream);


/* Hand-over AND lookup in ONE launch: tt_batch_ingest / tt_batch_ingest_store whose tile workgroups -- they hold the batch's
 * clamped fused rows in LDS anyway -- also gather the table rows and write them into the towers' input, i.e. the hand-over
 * followed by tt_embed_lookup_fwd (src/towers/cat_embed.py:103-121, :157-178; tower/base_tower.py:133-139) without the second
 * launch, its re-read of the ids and its boundary; the dense features are copied beside the gathers.  sides[i].out / ld_out /
 * out_dtype say where side i's rows go (as in tt_embed_lookup_fwd: out = first element of sample 0 / key 0); rows_km may be
 * NULL.  E must be 8, 16, 32 or 64 (TT_ERR_UNSUPPORTED otherwise: use the two separate calls).  Results are bit-identical to
 * the two separate calls (test).  The tile workgroups write tt_embed_lookup_set_profile's stamps (gather phase). */
typedef struct tt_ingest_lookup {
  const float* table;  /* fused [table_rows, E] f32 table */
  int64_t table_rows;
  int32_t E;
  int32_t reserved;
} tt_ingest_lookup;
int tt_batch_ingest_lookup(tt_ctx* ctx, int32_t n, void* const* dst, const void* const* src, const int64_t* bytes,
                           const tt_embed_side* sides, int32_t n_sides, int64_t B, int32_t* rows_km /* or NULL */,
                           const tt_ingest_lookup* lookup, const tt_cvt_list* cvt /* or NULL */, tt_stream stream);
int tt_batch_ingest_store_lookup(tt_ctx* ctx, int32_t n, void* const* dst, const void* const* src, const int64_t* bytes,
                                 const tt_embed_side* sides, const tt_store_side* stores, int32_t n_sides, int64_t B,
                                 const int64_t* order /* [B] or NULL */, int32_t* rows_km /* or NULL */,
                                 const tt_ingest_lookup* lookup, const tt_cvt_list* cvt /* or NULL */, tt_stream stream);

/* ------------------------------------------------------------------------------------------------
 * Pooled multi-valued categorical features (embedding bags) -- no reference counterpart: the reference's bags all have
 * length one (src/towers/pairs/unified_bid_data_loader.py:835).  Same sample-major contract as the lookup above: slot =
 * side_slot_base + b*K + k names bag (b, k); the bag's ids are ids[offsets[b*K + k] .. offsets[b*K + k + 1]) (positions),
 * offsets the exclusive prefix sum of the KJT's lengths.  With every length 1 the two entries below give the bits of
 * tt_embed_lookup_fwd and of tt_embed_grad_bwd over the general plan (test).
 *
 * tt_embed_bag_fwd, for bag (b, k) of side s, ONE launch:
 *   row_p = key_row_offset[k] + clamp(ids[p], 0, key_vocab[k]-1)          for every position p of the bag
 *   sum   = table[row_p0] + table[row_p1] + ...                            f32, ascending position order
 *   out[b*ld_out + k*E .. +E) = sum (key_pool[k] == TT_POOL_SUM) | sum / length (TT_POOL_MEAN);  zeros for an empty bag;
 *                               rounded to nearest even for TT_BF16
 *   rows_out[P] = row_p, bag_of[P] = slot of the bag, P = (nnz of the earlier sides) + p       (either may be NULL)
 * Positions behind a side's last bag, [offsets[B*K], nnz), belong to no bag: they get rows_out = 0 and bag_of = -1 (the
 * gradient skips them).  The data path uses no atomics; one lane group of E/4 lanes owns a bag and adds its rows in order.
 * E % 4 == 0, 4 <= E <= 256, table 16-byte and outputs 4-element aligned (base and ld_out): TT_ERR_UNSUPPORTED otherwise, nothing
 * launched.  A decoded row outside [0, table_rows) reads the last row and raises TT_DEVERR_ROW_RANGE, as the lookup does.  A
 * bag whose offsets are negative, decreasing or end beyond nnz raises TT_DEVERR_BAG_OFFSETS and is treated as empty: nothing is
 * read through such a pair, and the positions it should have covered are not written.
 * ---------------------------------------------------------------------------------------------- */
#define TT_DEVERR_BAG_OFFSETS 8u
#define TT_POOL_SUM 0
#define TT_POOL_MEAN 1
typedef struct tt_bag_side {
  const int64_t* ids;            /* [nnz] */
  const int64_t* offsets;        /* [B*K + 1] */
  const int64_t* key_row_offset; /* [K] */
  const int64_t* key_vocab;      /* [K] */
  const int32_t* key_pool;       /* [K] TT_POOL_* */
  void* out;
  int64_t ld_out;
  int64_t nnz;
  int32_t K;
  int32_t out_dtype;             /* TT_F32 / TT_BF16 */
} tt_bag_side;
int tt_embed_bag_fwd(tt_ctx* ctx, const float* table, int64_t table_rows, int32_t E, const tt_bag_side* sides, int32_t n_sides,
                     int64_t B, int32_t* rows_out, int32_t* bag_of, tt_stream stream);

/* The bags' table gradient over the plan tt_dedup_plan built from rows_out (M = nnz; sorted_src then lists POSITIONS).  Position
 * P contributes w_P * d_out[slot bag_of[P]] to its row, w_P = 1, or inv_len[bag_of[P]] when inv_len (f32 per slot: 1 / length
 * for the mean keys' slots, 1 for the others) is not NULL; positions with bag_of < 0 contribute nothing.  Slot s of source i
 * reads d_out_i[b*ld + k*E .. +E) as in tt_embed_grad_bwd, and mode is that entry's TT_GRAD_SPARSE / TT_GRAD_DENSE_SET /
 * TT_GRAD_DENSE_ACC (no flags).  Atomic-free sums, bitwise reproducible: a row's contributions are added (one fused multiply-add
 * each) in ascending position order; rows of more than 64 contributions in 64-position chunks whose partial sums the finish of
 * tt_embed_grad_bwd adds.  E % 4 == 0, 4 <= E <= 256, out 16-byte and sources 4-element aligned (TT_ERR_UNSUPPORTED otherwise). */
size_t tt_embed_bag_grad_workspace_bytes(int64_t nnz, int32_t E);
int tt_embed_bag_grad_bwd(tt_ctx* ctx, const tt_grad_src* srcs, int32_t n_srcs, int64_t B, int32_t E, const int32_t* bag_of,
                          const float* inv_len, const int32_t* sorted_src, const int32_t* seg_offsets,
                          const int32_t* unique_rows, const int32_t* n_unique, int64_t nnz, int32_t mode, float* out,
                          void* workspace, size_t workspace_bytes, tt_stream stream);

/* ------------------------------------------------------------------------------------------------
 * The capacity form of the pooled lookup: what a captured step runs on static id buffers.  Launch geometry depends on the
 * capacities alone; how many ids are live is device data.
 *
 * tt_embed_bag_fwd_cap: tt_embed_bag_fwd with side.nnz the CAPACITY of the side's id buffer; the live count is offsets[B*K].  Pooled
 * outputs, and rows_out / bag_of of every position a bag covers, are bit for bit tt_embed_bag_fwd's.  Every other position of the
 * side -- [offsets[B*K], capacity), and any position whose bag's offsets were refused -- gets rows_out = table_rows (the PAD ROW, one
 * past the last row) and bag_of = -1, written by the whole grid in a grid-stride pass: rows_out / bag_of need no fill in front.
 * The sides lie behind one another in position space (side 1 starts at side 0's capacity).  Nothing is read from ids at a
 * position no bag covers: the tail of a static buffer holds stale ids.  table_rows < INT32_MAX.
 *
 * tt_bag_prepare, for every side (two launches, no wait between workgroups):
 *   offsets[i] = lengths[0] + ... + lengths[i-1], i in [0, B*K]                     (int64)
 *   inv_len[side_slot_base + i] = 1 / (float)lengths[i], one correctly rounded f32 division, where key_pool[i % K] is TT_POOL_MEAN
 *                                 and lengths[i] > 0; 1 otherwise                   (inv_len may be NULL)
 * A side with a negative length, with a total above `capacity`, or -- count not NULL -- with a total other than *count (the number
 * of ids the host handed over, a device word) raises TT_DEVERR_BAG_OFFSETS and gets offsets all zero: its bags count as empty and
 * nothing is read through them.  workspace: tt_bag_prepare_workspace_bytes(side_slots = B*K per side, n_sides), 8-byte aligned.
 *
 * tt_dedup_plan_pad: tt_dedup_plan over keys in [0, table_rows]; the key table_rows is the pad row.  It sorts last, stays in
 * unique_rows / seg_offsets behind the real rows (seg_offsets[n_unique] is the end of the last real row) and is NOT counted in
 * n_unique.  The sort is stable by position, so the real rows' segments list their positions in the order tt_dedup_plan gives on
 * the live positions alone.  M = 0 and M pads (n_unique = 0) are valid.  Workspace: tt_dedup_workspace_bytes(M).
 *
 * The gradient: tt_embed_bag_grad_bwd with nnz = the total capacity; it visits the first n_unique rows only, so the pad segment is
 * never read (sparse mode: out has room for capacity rows).
 * ---------------------------------------------------------------------------------------------- */
typedef struct tt_bag_lengths {
  const int64_t* lengths;        /* [B*K] */
  const int32_t* key_pool;       /* [K] TT_POOL_* (NULL allowed when inv_len is NULL) */
  const int32_t* count;          /* device word: ids handed over, or NULL */
  int64_t* offsets;              /* out [B*K + 1] */
  int64_t capacity;
  int32_t K;
} tt_bag_lengths;
int tt_embed_bag_fwd_cap(tt_ctx* ctx, const float* table, int64_t table_rows, int32_t E, const tt_bag_side* sides, int32_t n_sides,
                         int64_t B, int32_t* rows_out, int32_t* bag_of, tt_stream stream);
size_t tt_bag_prepare_workspace_bytes(const int64_t* side_slots, int32_t n_sides);
int tt_bag_prepare(tt_ctx* ctx, const tt_bag_lengths* sides, int32_t n_sides, int64_t B, float* inv_len, void* workspace,
                   size_t workspace_bytes, tt_stream stream);
int tt_dedup_plan_pad(tt_ctx* ctx, const int32_t* rows, int64_t M, int64_t table_rows, int32_t* sorted_src, int32_t* unique_rows,
                      int32_t* seg_offsets, int32_t* n_unique, void* workspace, size_t workspace_bytes, tt_stream stream);

/* ------------------------------------------------------------------------------------------------
 * Weighted bags: one f32 weight per id, in the order of ids (a KeyedJaggedTensor's weights(), torch.nn.EmbeddingBag's
 * per_sample_weights).  Bag (b, k) over positions p0 < p1 < ... of length L pools to
 *   sum:  w_p0 * row_p0 + w_p1 * row_p1 + ...
 *   mean: that sum / L -- the divisor is the NUMBER of ids, as in the unweighted mean, not the sum of the weights.  A weighted
 *         average is sum pooling over weights the caller has normalised.
 * An empty bag pools to zeros.  Weights are data, used verbatim: negative, zero and non-finite values are not special-cased.  These
 * entries form no gradient for them; tt_embed_bag_weight_grad (below) does.
 *
 * Arithmetic (f32): a bag's first position is one multiply, acc = w * x; every later one is one fused multiply-add,
 * acc = fma(w, x, acc), in ascending position order; the mean divides as the unweighted entry does (acc / (float)L, only when
 * L > 1).  With every weight 1.0 these are the bits of tt_embed_bag_fwd, a -0 row included.
 *
 * tt_embed_bag_fwd_w / tt_embed_bag_fwd_cap_w: the arguments of tt_embed_bag_fwd / tt_embed_bag_fwd_cap, and
 *   weights: HOST array of n_sides DEVICE pointers, each f32 [side.nnz] ([capacity] in the capacity form); a NULL entry is a
 *            side whose ids all weigh 1.  Read with 4-byte loads: 4-byte alignment is all they need.
 *   w_out:   f32 [all sides' positions], laid out like rows_out / bag_of; may be NULL, but not when rows_out is given and a
 *            side has weights (TT_ERR_INVALID_ARG).  For every position a bag covers w_out[P] = that position's weight, 1.0f
 *            on a side without weights.  Positions no bag covers -- trailing ids, refused offsets, the capacity form's pads --
 *            are NOT written; the gradient never reads them (bag_of < 0 there).
 * Nothing is read from weights[i] at a position no bag covers, as nothing is read from ids there.  Whatever the unweighted
 * entries refuse these refuse too, before any launch.
 *
 * tt_embed_bag_grad_bwd_w: tt_embed_bag_grad_bwd plus pos_w, f32 [nnz] (the forward's w_out), or NULL for the unweighted
 * coefficients (then the launches of tt_embed_bag_grad_bwd).  Position P contributes c_P * d_out[slot bag_of[P]]:
 * c_P = pos_w[P] when inv_len is NULL, else the one f32 product pos_w[P] * inv_len[bag_of[P]]; each contribution is one
 * acc = fma(c_P, x, acc) in plan order.  Chunking, workspace and the long-row finish are tt_embed_bag_grad_bwd's; with every
 * weight 1.0 so are the bits.  No atomics on the data path in either direction.
 * ---------------------------------------------------------------------------------------------- */
int tt_embed_bag_fwd_w(tt_ctx* ctx, const float* table, int64_t table_rows, int32_t E, const tt_bag_side* sides, int32_t n_sides,
                       int64_t B, int32_t* rows_out, int32_t* bag_of, const float* const* weights, float* w_out, tt_stream stream);
int tt_embed_bag_fwd_cap_w(tt_ctx* ctx, const float* table, int64_t table_rows, int32_t E, const tt_bag_side* sides,
                           int32_t n_sides, int64_t B, int32_t* rows_out, int32_t* bag_of, const float* const* weights,
                           float* w_out, tt_stream stream);
int tt_embed_bag_grad_bwd_w(tt_ctx* ctx, const tt_grad_src* srcs, int32_t n_srcs, int64_t B, int32_t E, const int32_t* bag_of,
                            const float* inv_len, const float* pos_w, const int32_t* sorted_src, const int32_t* seg_offsets,
                            const int32_t* unique_rows, const int32_t* n_unique, int64_t nnz, int32_t mode, float* out,
                            void* workspace, size_t workspace_bytes, tt_stream stream);

/* ------------------------------------------------------------------------------------------------
 * The batch gather out of a device-resident store of per-entity BAGS: tt_batch_ingest_store's two-level gather (pair -> entity
 * row -> features) for multi-valued features, into the sample-major bag wire format a captured bag-mode step's static buffers
 * hold.  A store keeps dense_store f32 [N, dense_dim] and its bags as CSR over (entity, key) slots: the bag of entity e, key k
 * is values[offsets[e*K + k] .. offsets[e*K + k + 1]), so an entity's K bags are ONE contiguous run of ids.  For side i,
 * sample b (o and e as in tt_batch_ingest_store; e is always clamped into [0, n_rows)):
 *   dense_out[b, :]        = dense_store[e, :]                                         (f32 copy)
 *   lengths_out[b*K + k]   = offsets[e*K + k + 1] - offsets[e*K + k]
 *   ids_out[start_b .. start_b + run_b) = values[offsets[e*K] .. offsets[(e+1)*K]),    run_b = that run's length,
 *                                         start_b = run_0 + ... + run_(b-1)            (the offsets tt_bag_prepare forms again)
 * plus the n copy segments (the step scalars: the count word of a captured step travels there -- this entry does not read it).
 * Two launches, no workgroup waits on another: lengths, dense rows, copy segments and one total per tile of tt_bag_store_tile()
 * samples; then every tile's workgroups add up the side's earlier totals, scan their tile and copy its ids -- 16-byte stores on the
 * destination's 16-byte grid fed by 16-byte loads where the source is aligned alike and by 8-byte loads otherwise (ids_out may be
 * 8 mod 16); a position is found in its tile's runs by bisection, so a long run spreads over lanes and workgroups.
 * total = run_0 + ... + run_(B-1).  With total > capacity, or total != expect when expect >= 0, NO id is written and
 * TT_DEVERR_BAG_OFFSETS is raised; lengths, dense rows and copy segments are written all the same (tt_bag_prepare then refuses
 * the side through its own checks).  Nothing is ever written at or beyond ids_out[capacity]; ids_out[total .. capacity) keeps what
 * it held.  A run that leaves [0, nnz] (offsets the store's owner did not validate) refuses the side the same way and is not read.
 * workspace: tt_bag_store_gather_workspace_bytes(B, n_sides), 8-byte aligned.  B * K < 2^31, capacity < 2^31.
 * ---------------------------------------------------------------------------------------------- */
typedef struct tt_bag_store_side {
  const int64_t* entity;     /* entity index per pair, read at [o * entity_stride] */
  int64_t entity_stride;
  const float* dense_store;  /* [N, dense_dim] */
  const int64_t* offsets;    /* [N*K + 1] */
  const int64_t* values;     /* [nnz] */
  float* dense_out;          /* [B, dense_dim] */
  int64_t* lengths_out;      /* [B*K] */
  int64_t* ids_out;          /* [capacity] */
  int64_t nnz;
  int64_t capacity;
  int64_t expect;            /* the id count the host believes (what it puts into the step's count word), or -1 */
  int32_t dense_dim;
  int32_t n_rows;            /* entity rows N of the store, >= 1 */
  int32_t K;
  int32_t reserved;
} tt_bag_store_side;
int tt_bag_store_tile(void);
size_t tt_bag_store_gather_workspace_bytes(int64_t B, int32_t n_sides);
int tt_bag_store_gather(tt_ctx* ctx, int32_t n, void* const* dst, const void* const* src, const int64_t* bytes,
                        const tt_bag_store_side* sides, int32_t n_sides, int64_t B, const int64_t* order /* [B] or NULL */,
                        void* workspace, size_t workspace_bytes, tt_stream stream);

/* tt_bag_store_gather for stores that keep one f32 weight per id (a KJT's weights(): a share, a confidence), in the order of
 * `values`.  Everything tt_bag_store_gather writes, and for a side with weights
 *   weights_out[start_b + j] = weights[offsets[e*K] + j]     for j in [0, run_b)     (a 32-bit copy, bit for bit)
 * in the same two launches: the thread that moves an id piece moves its positions' weights.  A side with weights == NULL moves
 * ids alone; a call whose sides all do is tt_bag_store_gather.  A refused side (total > capacity, total != expect, a run outside
 * [0, nnz]) gets neither ids nor weights.  Nothing is written at or beyond weights_out[capacity]; weights_out[total .. capacity)
 * keeps what it held; a source index outside [0, nnz) is not read.  weights and weights_out need 4-byte alignment, whatever
 * ids_out's is.  With nnz > 0, weights and weights_out are both set or both NULL (TT_ERR_INVALID_ARG otherwise) -- except that, as
 * ids_out, weights_out may be NULL where capacity == 0 (a batch without ids: such a side has nowhere to put a weight). */
typedef struct tt_bag_store_side_w {
  const int64_t* entity;
  int64_t entity_stride;
  const float* dense_store;
  const int64_t* offsets;
  const int64_t* values;
  float* dense_out;
  int64_t* lengths_out;
  int64_t* ids_out;
  int64_t nnz;
  int64_t capacity;
  int64_t expect;
  int32_t dense_dim;
  int32_t n_rows;
  int32_t K;
  int32_t reserved;
  const float* weights;      /* [nnz], or NULL: this side moves ids alone */
  float* weights_out;        /* [capacity] */
} tt_bag_store_side_w;
int tt_bag_store_gather_w(tt_ctx* ctx, int32_t n, void* const* dst, const void* const* src, const int64_t* bytes,
                          const tt_bag_store_side_w* sides, int32_t n_sides, int64_t B, const int64_t* order /* [B] or NULL */,
                          void* workspace, size_t workspace_bytes, tt_stream stream);

/* ------------------------------------------------------------------------------------------------
 * Gradients FOR the per-id weights of a weighted bag (torch.nn.EmbeddingBag(per_sample_weights=) differentiates with respect
 * to them), and learned position weights built on them (torchrec's PositionWeightedModule: one weight per bag position).
 *
 * tt_embed_bag_weight_grad, ONE launch over the positions of a bag plan (rows / bag_of as tt_embed_bag_fwd[_cap][_w] wrote them,
 * inv_len per slot or NULL: what tt_embed_bag_grad_bwd takes).  srcs[i] is side i's source as in tt_embed_bag_grad_bwd (f32 or
 * bf16, all requested sides alike, row stride ld); side_nnz[i] the side's positions (its capacity in the capacity form), the sides
 * lying behind one another in rows / bag_of; g_out a HOST array of n_sides DEVICE pointers, each f32 [side_nnz[i]], laid out like
 * the _w entries' `weights`.  A side whose pointer is NULL is skipped: nothing of it is read or written, its source included.
 * For position P of a requested side, slot = bag_of[P]:
 *   slot >= 0:  g[p] = c * (d[0]*x[0] + ... + d[E-1]*x[E-1]),  x = table row rows[P], d = the E columns of the slot's source row
 *               (bf16 widened exactly), c = inv_len[slot] when inv_len is given, else 1.  The forward weight is NOT a factor.
 *   slot <  0:  g[p] = 0.0f, and nothing is read through rows[P] (trailing ids, refused offsets, the capacity form's pads -- the
 *               pad row lies one past the table).  A slot outside the side or a row outside the table is treated the same way.
 * Arithmetic (f32): each of the E/4 lanes of a position forms d0*x0, then three fused multiply-adds over its 16-byte piece; the
 * lanes' partial sums are added by a fixed xor tree over the lane group (the power of two >= E/4), then one product with c.  The
 * order depends on E alone: two runs give equal bits.  No atomics, no workspace.  E % 4 == 0 and 4 <= E <= 256, the table 16-byte
 * and the sources 4-element aligned (TT_ERR_UNSUPPORTED otherwise), as the bag entries.
 *
 * Position weights: param is a flat f32 [n_param] vector; key k of a side reads param[pw_offset[k] .. pw_offset[k] + pw_len[k]),
 * pw_offset[k] = -1 for a key without position weights (pw_offset / pw_len: int32 [K] on the device).
 * tt_bag_position_weights_fwd: for position j of bag (b, k) (offsets int64 [B*K + 1], as tt_embed_bag_fwd reads them)
 *   w[p] = param[pw_offset[k] + min(j, pw_len[k] - 1)]   -- a 32-bit copy; positions at or beyond pw_len share the LAST weight
 *   w[p] = 1.0f for a key without position weights and for every position no bag covers ([offsets[B*K], nnz), refused pairs).
 * tt_bag_position_weights_bwd: d_param[e] = the sum of w[p] (here: the per-id gradient, the field `w` read instead of written)
 * over all positions of all sides that read element e, 0 for an element nobody reads.  One workgroup per element, threads striding
 * over the samples and adding their positions in ascending order, then a fixed tree: no atomics, and launch geometry and
 * order depend on the shapes alone -- two runs give equal bits.  A side with w == NULL contributes nothing.
 * ---------------------------------------------------------------------------------------------- */
int tt_embed_bag_weight_grad(tt_ctx* ctx, const float* table, int64_t table_rows, int32_t E, const tt_grad_src* srcs, int32_t n_sides,
                             int64_t B, const int32_t* rows, const int32_t* bag_of, const float* inv_len, const int64_t* side_nnz,
                             float* const* g_out, tt_stream stream);
typedef struct tt_bag_pw_side {
  const int64_t* offsets;    /* [B*K + 1] */
  const int32_t* pw_offset;  /* [K]: first element of key k in param, or -1 */
  const int32_t* pw_len;     /* [K]: max_len of key k (>= 1 where pw_offset >= 0) */
  float* w;                  /* [nnz]: fwd writes the weights; bwd reads the per-id gradient */
  int64_t nnz;
  int32_t K;
  int32_t reserved;
} tt_bag_pw_side;
int tt_bag_position_weights_fwd(tt_ctx* ctx, const float* param, int64_t n_param, const tt_bag_pw_side* sides, int32_t n_sides,
                                int64_t B, tt_stream stream);
int tt_bag_position_weights_bwd(tt_ctx* ctx, float* d_param, int64_t n_param, const tt_bag_pw_side* sides, int32_t n_sides,
                                int64_t B, tt_stream stream);

/* ------------------------------------------------------------------------------------------------
 * The pooled lookup with a position-weight SOURCE: tt_embed_bag_fwd_w / tt_embed_bag_fwd_cap_w whose sides each take their
 * weights from one of three places -- srcs[i] (a HOST array of n_sides entries):
 *   weights != NULL:  a per-id array, exactly the _w entries' weights[i];
 *   param != NULL:    the position-weight parameter, f32 [n_param] with the key directory pw_offset / pw_len (int32 [K], device):
 *                     position j of a bag of key k weighs param[clamp(pw_offset[k] + min(j, pw_len[k] - 1), 0 .. n_param - 1)],
 *                     1.0f where pw_offset[k] < 0 -- the index of tt_bag_position_weights_fwd, formed inside the lookup's launch
 *                     from the key and the position in the bag it already holds: no expansion launch, no search over the offsets;
 *   neither:          the side's ids all weigh 1.
 * Both on one side: TT_ERR_INVALID_ARG.  A param needs pw_offset, pw_len and 1 <= n_param < 2^31 (TT_ERR_INVALID_ARG) and 4-byte
 * alignment (TT_ERR_UNSUPPORTED).  The sides of one launch may differ in their source.  The value goes through the _w entries'
 * arithmetic and into w_out (required with rows_out when any side has a source).  out, rows_out, bag_of and w_out at every
 * position a bag covers are bit for bit what tt_bag_position_weights_fwd followed by tt_embed_bag_fwd[_cap]_w writes; in the
 * capacity form positions no bag covers keep (pad row, -1).  A call without any param launches the _w kernel.  ONE launch.
 * (`_posw`, not `_pw`: that suffix names the score entries' pair-weight family.)
 * ---------------------------------------------------------------------------------------------- */
typedef struct tt_bag_weight_src {
  const float* weights;      /* [side.nnz] per-id weights, or NULL */
  const float* param;        /* [n_param] position-weight parameter, or NULL */
  const int32_t* pw_offset;  /* [K]: first element of key k in param, or -1 */
  const int32_t* pw_len;     /* [K]: max_len of key k */
  int64_t n_param;
} tt_bag_weight_src;
int tt_embed_bag_fwd_posw(tt_ctx* ctx, const float* table, int64_t table_rows, int32_t E, const tt_bag_side* sides, int32_t n_sides,
                        int64_t B, int32_t* rows_out, int32_t* bag_of, const tt_bag_weight_src* srcs, float* w_out, tt_stream stream);
int tt_embed_bag_fwd_cap_posw(tt_ctx* ctx, const float* table, int64_t table_rows, int32_t E, const tt_bag_side* sides,
                            int32_t n_sides, int64_t B, int32_t* rows_out, int32_t* bag_of, const tt_bag_weight_src* srcs,
                            float* w_out, tt_stream stream);

/* ------------------------------------------------------------------------------------------------
 * The ROWS-ONLY form of the pooled lookup: what a rank of the row-wise sharded step runs, whose table lives on other ranks.
 * tt_embed_bag_rows writes into rows_out / bag_of -- and tt_embed_bag_rows_w into w_out -- exactly the words tt_embed_bag_fwd[_w]
 * writes there for the same sides, bit for bit: the fused row of every position a bag covers (ids clamped as in the lookup; a row
 * outside [0, table_rows) stored as table_rows - 1 with TT_DEVERR_ROW_RANGE), (0, -1) for the positions behind a side's last
 * bag, TT_DEVERR_BAG_OFFSETS and an empty bag for a refused offset pair.  table_rows is the GLOBAL row count.  No table is
 * read and no pooled output written: a side's out / ld_out / out_dtype (and key_pool) are not looked at and may be NULL / 0.
 * The same kernel template as the lookup (a rows-only instantiation), ONE launch, no atomics on the data path, no LDS.
 * weights / w_out: as tt_embed_bag_fwd_w takes them.  There is no capacity form and no position-weight source.
 * ---------------------------------------------------------------------------------------------- */
int tt_embed_bag_rows(tt_ctx* ctx, int64_t table_rows, const tt_bag_side* sides, int32_t n_sides, int64_t B, int32_t* rows_out,
                      int32_t* bag_of, tt_stream stream);
int tt_embed_bag_rows_w(tt_ctx* ctx, int64_t table_rows, const tt_bag_side* sides, int32_t n_sides, int64_t B, int32_t* rows_out,
                        int32_t* bag_of, const float* const* weights, float* w_out, tt_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* TWOTOWER_H_ */
