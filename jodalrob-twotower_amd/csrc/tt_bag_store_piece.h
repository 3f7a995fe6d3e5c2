// Where one 16-byte piece of tt_bag_store_gather's id copy comes from: plain integer code shared by the kernel (tt_bag_store.hip)
// and a host program that walks every piece of small tiles (tests/bag_store_piece_check.cpp), so it compiles with and without hipcc.
#pragma once
#include <stdint.h>

#ifndef __HIPCC__
#define TT_PIECE_FN inline
#else
#define TT_PIECE_FN __host__ __device__ __forceinline__
#endif

constexpr int kStoreTile = 256;                       // samples per tile: one per thread

// the sample of the tile whose run holds position p, start[0] <= p < start[kStoreTile]: the last one that starts at or before p.
// The first index in [1, kStoreTile] whose start lies above p, minus one: 255 candidates halve to none in 8 steps, and the
// result lies in [0, kStoreTile - 1] whatever start[] holds.
TT_PIECE_FN int store_find(const int64_t* start, int64_t p) {
  int lo = 1, hi = kStoreTile;
  for (int it = 0; it < 8; ++it) {
    const int mid = (lo + hi) >> 1;
    const bool above = start[mid] > p;
    hi = above ? mid : hi;
    lo = above ? lo : mid + 1;
  }
  return lo - 1;
}
static_assert(kStoreTile == 256, "store_find halves 255 candidates in 8 steps");

// Piece q of the destination's 16-byte grid holds the positions p0 = 2q - A and p0 + 1 (A = 1: the destination is 8 mod 16).  Of
// the tile's positions [ts, te) it returns which of the two are live (bit 0: p0, bit 1: p0 + 1) and where their ids lie in the
// store: i0 / i1 = src[s] + (p - start[s]) for the sample s that holds p.  The caller passes pieces from (ts + A) >> 1 to
// (te - 1 + A) >> 1 only, so p0 >= ts - 1, p0 < te and p0 + 1 >= ts.
TT_PIECE_FN int store_piece(const int64_t* start, const int64_t* src, int64_t ts, int64_t te, int64_t A, int64_t q, int64_t* p0_out,
                            int64_t* i0, int64_t* i1) {
  const int64_t p0 = 2 * q - A, p1 = p0 + 1;
  const bool l0 = p0 >= ts && p0 < te, l1 = p1 >= ts && p1 < te;
  int s0 = 0;
  *p0_out = p0;
  *i0 = *i1 = 0;
  if (l0) {
    s0 = store_find(start, p0);
    *i0 = src[s0] + (p0 - start[s0]);
  }
  if (l1) {
    const int s1 = (l0 && p1 < start[s0 + 1]) ? s0 : store_find(start, p1);
    *i1 = src[s1] + (p1 - start[s1]);
  }
  return (l0 ? 1 : 0) | (l1 ? 2 : 0);
}
