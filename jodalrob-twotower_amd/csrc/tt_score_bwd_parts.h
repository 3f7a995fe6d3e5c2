// Device parts of the directional score kernels of tt_score_bf16.hip: the launch arguments, the direction select, the a rows' setup,
// the formula of the softmax weight of a pair (a, b).  Each is written ONCE here, is __forceinline__ and adds no
// operation of its own: the kernels that call them compile as they did with these lines written out (profiles/NOTES.md, "score
// backward parts").  What differs between the forms stays in the kernels: how the b operands reach a wave, the pipelining of the
// second product, rows8's block scaling, the hosted tail -- and, for now, everything that works on a lane's 16-element arrays (the
// reciprocals' preparation, the ragged mask, the diagonal's -2, the conversion to fragments), the two-buffer sweep and the
// cross-wave tree and the store of dA: written as parts they changed hipcc's register allocation of the kernels that sit at an occupancy step (NOTES).
// Included by tt_score_bf16.hip and, through tt_score_bwd_bsplit.h, by tt_score_cells.hip; in an unnamed namespace as the kernels are.
#pragma once
#include "tt_score_bf16.h"
#include "tt_score_cells.h"

namespace {

using namespace ttscore;

struct DirFwd {
  const __bf16* a_rows;
  const __bf16* b_rows;
  int64_t Ra, Rb, off;
  float* sumexp;
  float* diag;
  int32_t* rank;
  float* sumscore;
  int32_t rank_mode;   // 0 none, 1 top-1 flag (rank = 0/1), 2 full rank
  float c1;            // exponent scale for this direction's products: inv_t * log2(e) / (scale the operand images carry)
  float unscale;       // product -> s / T
  float* inv_sumexp;   // optional out: 1 / (the sum as accumulated), the factor the backward kernel multiplies by
  const __bf16* a_lo;  // bf16x3 operands only: the lo rows images of A and B
  const __bf16* b_lo;
};
struct FwdArgs {
  DirFwd d[2];
  float c2, kexp;      // exponent offset (-shift * log2 e); UNIT kernels leave it out of the terms and scale the row sums by 2^c2
};

struct DirBwd {
  const __bf16* a_rows;
  const __bf16* b_rows;
  const __bf16* b_frag;
  int64_t Ra, Rb, off;
  const float* sumexp_a;
  const float* sumexp_b;
  float* dA;
  float c1;            // as DirFwd::c1
  float out_scale;     // scale / (the B image's scale)
  const float* inv_a;  // optional: DirFwd::inv_sumexp of the A rows / of the B rows (then no reciprocals in the tile loop)
  const float* inv_b;
  const char* b_frag8;  // fp8 packing only: the B rows' fp8 fragment image (score_bwd_rows8_kernel)
  const __bf16* a_lo;   // bf16x3 operands only: the lo images (rows of A, rows and fragment image of B)
  const __bf16* b_lo;
  const __bf16* b_frag_lo;
};
struct BwdArgs {
  DirBwd d[2];
  float c2, kexp;
  const float* d_loss;
  int D;
  // LQ kernels (tt_score_bwd_bf16_lq): per direction the sampling weights of the A rows and of the B rows (tt_score_bwd_lq)
  const float* wt_a[2];
  const float* wt_b[2];
  // MK kernels (tt_score_bwd_bf16_mask; the b-split form, which reads the arguments itself): the rows' notice / company ids, the same
  // two arrays for both directions (square problem)
  const int32_t* ent_n;
  const int32_t* ent_c;
  // PW kernels (tt_score_bwd_bf16_pw; the b-split form): the normalised pair weights g (tt_score_prepare_pw), one array for both
  // directions; inv_a / inv_b are then the weighted forward's folded reciprocals
  const float* pw_g;
};
// KP kernels (tt_score_bwd_bf16_cells; the b-split form): the masked cells' plan behind the other arguments, one for both directions --
// direction 1 reads a tile pair with its local coordinates swapped.  A type of its own: every other instantiation keeps its argument
// block, and with it its code, as it was.
struct BwdArgsKP : BwdArgs {
  TtCellsPlan kp;
};

// ---- the direction select ----------------------------------------------------------------------------------------------------
// The fields of direction blockIdx.y are picked with scalar selects (indexing the by-value argument with blockIdx.y made every
// field -- and with it the whole tile loop's control flow -- live in vector registers), and row counts / positions are 32-bit:
// the loop counter, the tile classification and their branches then run on the SALU.  A kernel reads the fields it needs; the
// selects of the others are dead code.
struct FwdSel {
  const __bf16 *a_rows, *b_rows, *a_lo, *b_lo;
  float *sumexp, *diag;
  int32_t* rank;
  float* sumscore;
  int32_t rank_mode;
  float c1, unscale;
  float* inv_sumexp;
  int Ra, Rb, off;
};
__device__ __forceinline__ FwdSel select_dir(const FwdArgs& args, bool d1) {
  FwdSel s;
  s.a_rows = d1 ? args.d[1].a_rows : args.d[0].a_rows;
  s.b_rows = d1 ? args.d[1].b_rows : args.d[0].b_rows;
  s.a_lo = d1 ? args.d[1].a_lo : args.d[0].a_lo;
  s.b_lo = d1 ? args.d[1].b_lo : args.d[0].b_lo;
  s.sumexp = d1 ? args.d[1].sumexp : args.d[0].sumexp;
  s.diag = d1 ? args.d[1].diag : args.d[0].diag;
  s.rank = d1 ? args.d[1].rank : args.d[0].rank;
  s.sumscore = d1 ? args.d[1].sumscore : args.d[0].sumscore;
  s.rank_mode = d1 ? args.d[1].rank_mode : args.d[0].rank_mode;
  s.c1 = d1 ? args.d[1].c1 : args.d[0].c1;
  s.unscale = d1 ? args.d[1].unscale : args.d[0].unscale;
  s.inv_sumexp = d1 ? args.d[1].inv_sumexp : args.d[0].inv_sumexp;
  s.Ra = (int)(d1 ? args.d[1].Ra : args.d[0].Ra);
  s.Rb = (int)(d1 ? args.d[1].Rb : args.d[0].Rb);
  s.off = (int)(d1 ? args.d[1].off : args.d[0].off);
  return s;
}

struct BwdSel {
  const __bf16 *a_rows, *b_rows;
  const char* b_frag8;
  const __bf16 *b_frag, *a_lo, *b_lo, *b_frag_lo;
  const float *sumexp_a, *sumexp_b;
  float* dA;
  float c1, out_scale;
  const float *inv_a, *inv_b;
  const float *wt_a, *wt_b;     // (LQ)
  int Ra, Rb, off;
};
__device__ __forceinline__ BwdSel select_dir(const BwdArgs& args, bool d1) {
  BwdSel s;
  s.a_rows = d1 ? args.d[1].a_rows : args.d[0].a_rows;
  s.b_rows = d1 ? args.d[1].b_rows : args.d[0].b_rows;
  s.b_frag8 = d1 ? args.d[1].b_frag8 : args.d[0].b_frag8;
  s.b_frag = d1 ? args.d[1].b_frag : args.d[0].b_frag;
  s.a_lo = d1 ? args.d[1].a_lo : args.d[0].a_lo;
  s.b_lo = d1 ? args.d[1].b_lo : args.d[0].b_lo;
  s.b_frag_lo = d1 ? args.d[1].b_frag_lo : args.d[0].b_frag_lo;
  s.sumexp_a = d1 ? args.d[1].sumexp_a : args.d[0].sumexp_a;
  s.sumexp_b = d1 ? args.d[1].sumexp_b : args.d[0].sumexp_b;
  s.dA = d1 ? args.d[1].dA : args.d[0].dA;
  s.c1 = d1 ? args.d[1].c1 : args.d[0].c1;
  s.out_scale = d1 ? args.d[1].out_scale : args.d[0].out_scale;
  s.inv_a = d1 ? args.d[1].inv_a : args.d[0].inv_a;
  s.inv_b = d1 ? args.d[1].inv_b : args.d[0].inv_b;
  s.wt_a = d1 ? args.wt_a[1] : args.wt_a[0];
  s.wt_b = d1 ? args.wt_b[1] : args.wt_b[0];
  s.Ra = (int)(d1 ? args.d[1].Ra : args.d[0].Ra);
  s.Rb = (int)(d1 ? args.d[1].Rb : args.d[0].Rb);
  s.off = (int)(d1 ? args.d[1].off : args.d[0].off);
  return s;
}

// ---- the a rows of a wave ------------------------------------------------------------------------------------------------------
// Lane (c, h) of a 32-row a tile stands for row a = tile's first row + c: ia = 1 / (its exp-sum as the forward accumulated it) --
// the forward's reciprocal, or taken here (kx = 2^c2 in the UNIT kernels: 1 / raw sum = 2^c2 / stored sum) --, ua its sampling
// weight (LQ), pos the column of its positive.  Rows past Ra weigh nothing.
template <bool LQ>
__device__ __forceinline__ void a_row_setup(const BwdSel& dr, float kx, int a, float& ia, float& ua, int& pos) {
  ia = a < dr.Ra ? (dr.inv_a ? dr.inv_a[a] : __builtin_amdgcn_rcpf(dr.sumexp_a[a]) * kx) : 0.f;
  if constexpr (LQ) ua = a < dr.Ra ? dr.wt_a[a] : 0.f;
  pos = a + dr.off;
}

template <int AT, int DT>
__device__ __forceinline__ void zero_acc(f32x16 (&dacc)[AT][DT]) {
#pragma unroll
  for (int i = 0; i < AT; ++i)
#pragma unroll
    for (int d = 0; d < DT; ++d)
#pragma unroll
      for (int r = 0; r < 16; ++r) dacc[i][d][r] = 0.f;
}

// ---- the softmax weight of a pair (a, b): the loss's gradient ------------------------------------------------------------------
// e_ab (1 / rowsum_a + 1 / colsum_b) from the S accumulator x: e_ab = exp2(x) in the UNIT kernels (the operand images carry the
// exponent's scale), exp2(x c1 + c2) otherwise.  LQ (tt_score_bwd_bf16_lq): e_ab (w_b / rowsum_a + w_a / colsum_b) with the sampling
// weights w of the two rows -- one multiply more.  MK (tt_score_bwd_bf16_mask): 0 for a masked pair (same_entity; the caller keeps
// the diagonal out).  THE formula: every backward form takes it from here.
template <bool UNIT, bool LQ, bool MK = false>
__device__ __forceinline__ float softmax_term(float x, float c1, float c2, float ia, float ua, float ib, float wb, bool masked = false) {
  const float e = UNIT ? __builtin_amdgcn_exp2f(x) : __builtin_amdgcn_exp2f(__builtin_fmaf(x, c1, c2));
  float w;
  if constexpr (LQ) w = e * __builtin_fmaf(ua, ib, wb * ia);
  else w = e * (ia + ib);
  if constexpr (MK) w = masked ? 0.f : w;
  return w;
}

}  // namespace
