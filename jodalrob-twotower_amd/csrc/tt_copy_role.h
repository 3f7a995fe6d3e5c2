// The copy segments every hand-over launch carries (tt_copy_multi, tt_batch_ingest*, tt_bag_store_gather): one segment per grid
// row.  Shared by tt_embed.hip and tt_bag_store.hip; in an anonymous namespace, as the kernels that take the type are.
#pragma once
#include "tt_embed_slots.h"

namespace {

struct CopyArgs {
  char* dst[TT_MAX_COPIES];
  const char* src[TT_MAX_COPIES];
  int64_t bytes[TT_MAX_COPIES];
};

// one copy segment per grid row: the 16-byte body strided over the row's workgroups, the byte tail by its first workgroup
__device__ __forceinline__ void copy_segment_role(const CopyArgs& a, int seg) {
  const int64_t n16 = a.bytes[seg] / 16, tail0 = n16 * 16;
  const float4* __restrict__ s = reinterpret_cast<const float4*>(a.src[seg]);
  float4* __restrict__ d = reinterpret_cast<float4*>(a.dst[seg]);
  const int64_t stride = (int64_t)gridDim.x * role_threads();
  for (int64_t i = (int64_t)blockIdx.x * role_threads() + threadIdx.x; i < n16; i += stride) d[i] = s[i];
  if (blockIdx.x == 0)
    for (int64_t i = tail0 + threadIdx.x; i < a.bytes[seg]; i += role_threads()) a.dst[seg][i] = a.src[seg][i];
}

}  // namespace
