// The masked-cells plan (tt_score_cells_plan, twotower.h) as the score kernels read it: per 32 x 32 tile pair (notice tile I, column
// tile Jg -- Jg < nT in-batch, Jg >= nT the extras' tile Jg - nT) a span [off[I * nTJ + Jg], off[I * nTJ + Jg + 1]) of local codes
// a_local * 32 + j_local.  Both reads of a span's ends are wave-uniform (scalar loads); a wave walks a non-empty span once per
// tile and leaves one 16-bit mask per lane, bit r = "my element r of this tile is a listed cell".
#pragma once
#include "tt_common.h"

struct TtCellsPlan {
  const int32_t* off;     // [nT * nTJ + 1]
  const int32_t* codes;   // [capacity]
  int nTJ;                // nT + nTx
  int cap;                // rows of the codes array: no span is read past it, whatever the offsets hold
};

static inline int64_t tt_cells_pairs(int64_t B, int64_t M) { return tt_cdiv(B, 32) * (tt_cdiv(B, 32) + tt_cdiv(M, 32)); }
// the codes start on a 16-byte boundary behind the offsets
static inline int64_t tt_cells_codes_at(int64_t B, int64_t M) { return (tt_cells_pairs(B, M) + 1 + 3) / 4 * 4; }
static inline TtCellsPlan tt_cells_view(const int32_t* plan, int64_t B, int64_t M, int64_t capacity) {
  return TtCellsPlan{plan, plan + tt_cells_codes_at(B, M), (int)(tt_cdiv(B, 32) + tt_cdiv(M, 32)), (int)capacity};
}

// The masked-cells backward launches (tt_score_cells.hip), called by tt_score_bwd_bf16_cells behind its argument checks: `args` is the
// caller's BwdArgs / XnegArgs (tt_score_bwd_parts.h / tt_score_bwd_bsplit.h) as bytes.
int tt_score_bwd_cells_square(const void* args, size_t args_bytes, int64_t maxRa, bool unit, bool lq, int32_t D, const int32_t* plan,
                              int64_t capacity, int64_t B, int64_t M, hipStream_t st);
int tt_score_bwd_cells_xneg(const void* args, size_t args_bytes, bool unit, int32_t D, const int32_t* plan, int64_t capacity, int64_t B,
                            int64_t M, hipStream_t st);

// The lane's mask of tile pair (I, Jg).  S tile layout of the score kernels: lane (c, h) holds, in register r, the element (lane
// index c, register row (r & 3) + 8 (r >> 2) + 4 h).  swap == false: the lanes stand for the notice rows (c = a_local) and the
// registers for the columns; swap == true (the backward's (C, N) / (X, N) directions): the other way round.
__device__ __forceinline__ unsigned tt_cells_mask(const TtCellsPlan& p, int I, int Jg, int c, int h, bool swap) {
  const int64_t at = (int64_t)I * p.nTJ + Jg;
  // (clamped to the codes array: offsets that are not a plan's -- a buffer no plan launch has filled -- read nothing out of bounds)
  const int o0 = min(max(__builtin_amdgcn_readfirstlane(p.off[at]), 0), p.cap);
  const int o1 = min(__builtin_amdgcn_readfirstlane(p.off[at + 1]), p.cap);
  unsigned km = 0;
  for (int k = o0; k < o1; ++k) {
    const int code = __builtin_amdgcn_readfirstlane(p.codes[k]);
    const int al = swap ? (code & 31) : (code >> 5), bl = swap ? (code >> 5) : (code & 31);   // lane index, register row
    const int r = (bl & 3) + 4 * (bl >> 3), hb = (bl >> 2) & 1;
    km |= (c == al && h == hb) ? (1u << r) : 0u;
  }
  return km;
}
