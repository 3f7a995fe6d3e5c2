// Learned position weights: which parameter element a bag position reads.  Shared by tt_bag_weight_grad.hip (the expansion launch and
// its backward) and tt_embed_bag.hip (the pooled lookup's position-weight source): one definition of the index and its clamp.
#pragma once
#include "tt_common.h"

// position j of a bag whose key owns param[off .. off + len): the element it reads, or -1 (the key has none): clamped into the parameter
__device__ __forceinline__ int64_t pw_index_at(int32_t off, int32_t len, int64_t j, int64_t n_param) {
  if (off < 0 || len < 1) return -1;
  int64_t e = (int64_t)off + (j < len - 1 ? j : len - 1);
  return e < n_param ? e : n_param - 1;
}

// ... of key k of a side whose directory is pw_off / pw_len (int32 [K])
__device__ __forceinline__ int64_t pw_index(const int32_t* pw_off, const int32_t* pw_len, uint32_t k, int64_t j, int64_t n_param) {
  return pw_index_at(pw_off[k], pw_len[k], j, n_param);
}
