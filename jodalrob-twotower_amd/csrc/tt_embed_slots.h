// What the embedding path's files (tt_embed.hip, tt_plan.hip, tt_grad.hip, tt_optim.hip, tt_route.hip) share about slots and
// rows: the workgroup size, the slot -> (side, sample, key) decoding, the row range check, the row mapping of the reduction and
// the optimisers, and the grid and size helpers of their hosts.  In an anonymous namespace, as every kernel that takes these
// types is: the kernels keep the names the profiles record.
#pragma once
#include "tt_common.h"

namespace {

constexpr int kThreads = 256;

// ------------------------------------------------------------------------------------------------
// slot decoding shared by lookup (forward) and gradient (backward)
// ------------------------------------------------------------------------------------------------
struct SideDev {
  const int64_t* ids;
  const int64_t* off;
  const int64_t* vocab;
  char* out;          // lookup output / gradient source
  int64_t ld;
  uint32_t slot_base; // first slot of this side
  int32_t K;
  int32_t dtype;
  uint32_t magic;     // floor(2^32 / K): slot -> (sample, key) without an integer division (gradient kernels)
};

struct SideSet {
  SideDev s[TT_MAX_SIDES];
  int32_t n;
  int32_t E;
  uint32_t C;          // VEC-wide chunks per row
  uint32_t total_slots;
  int32_t table_rows;  // lookup kernels: rows of the table the decoded row indexes (0: unchecked)
  uint32_t* dev_err;   // ... and the context's sticky error word (TT_DEVERR_ROW_RANGE)
};

// A decoded row that does not lie in the table: key offsets / vocabularies (device arrays the host cannot check without a
// synchronisation) that belong to another table, or precomputed rows from elsewhere.  Reading it would be a GPU memory fault;
// the launch reads the last row instead and raises the sticky error word (tt_ctx_check_device_errors -> TT_ERR_DEVICE).
__device__ __forceinline__ int64_t row_in_table(int64_t row, int32_t table_rows, uint32_t* dev_err) {
#ifdef TT_NO_ROW_CHECK                                      // measurement builds only (tools/r04_b13.sh: what the check costs)
  return row;
#endif
  if (table_rows > 0 && (uint64_t)row >= (uint64_t)table_rows) {
    if (dev_err) atomicOr(dev_err, TT_DEVERR_ROW_RANGE);
    row = table_rows - 1;
  }
  return row;
}

__device__ __forceinline__ int side_of(const SideSet& a, uint32_t slot) {
  int si = 0;
#pragma unroll
  for (int i = 1; i < TT_MAX_SIDES; ++i)
    if (i < a.n && slot >= a.s[i].slot_base) si = i;
  return si;
}

// blockDim.x for code shared between kernels (roles): blockDim.x itself goes through the device library's partial-workgroup select, which only a
// kernel body folds into one load; the builtin is that one load (HIP launches are uniform), so a role compiles as it would inline
__device__ __forceinline__ uint32_t role_threads() { return __builtin_amdgcn_workgroup_size_x(); }

// ------------------------------------------------------------------------------------------------
// host helpers
// ------------------------------------------------------------------------------------------------
inline uint32_t pow2_at_least(uint32_t x) {
  uint32_t p = 1;
  while (p < x) p <<= 1;
  return p;
}

inline int grid_for(const tt_ctx* ctx, int64_t threads_needed) {
  const int64_t cap = (int64_t)ctx->num_cus * 8;
  int64_t b = tt_cdiv(threads_needed, kThreads);
  if (b < 1) b = 1;
  return (int)(b < cap ? b : cap);
}

inline size_t align256(size_t x) { return (x + 255) & ~size_t(255); }

// the row mapping of the reduction and the optimiser: a row is C chunks of VEC floats (VEC = 4 when vec4), owned by LG lanes
inline void row_mapping(int32_t E, bool vec4, uint32_t* C, uint32_t* LG) {
  *C = (uint32_t)(vec4 ? E / 4 : E);
  *LG = pow2_at_least(*C) > 64 ? 64 : pow2_at_least(*C);
}

}  // namespace
