// Single-pass symmetric forward of the in-batch-negative score + softmax-CE (two_tower_train_task.py:99-179) on the square
// training problem: S = N C^T is swept ONCE; every 32x32 tile feeds both softmax directions.
//
// The two-direction kernel of tt_score_bf16.hip computes every tile (MFMA + exp2) twice, once per direction, because a
// 32x32 MFMA result holds one index on the lanes and the other in the registers: sums over the register index are
// in-lane adds, sums over the lane index are cross-lane reductions (80 DPP steps per tile).  Here a wave keeps ONE tile J
// of company rows b as its resident operand and sweeps a chunk of notice tiles I; X[b = register][a = lane]:
//   * column direction (per b, sum over a): 16 per-lane accumulators that live across the whole sweep -- the cross-lane
//     reduction happens once per sweep, not once per tile;
//   * row direction (per a, sum over b): the in-lane sum over the 16 registers is the tile's partial for 32 rows a; it goes
//     to a wave-private LDS slot (one ds_write per tile).  After the sweep the workgroup adds the slots of its 8 waves
//     (8 tiles J) in wave order and writes ONE partial per (J-group, a) to a slab [n_groups][B].
// A second launch (finish1, B/256 workgroups) adds the slab rows in a fixed order, forms the per-row terms of the loss and
// the metrics, and leaves rowsum / colsum / their reciprocals for the backward kernel; finish2 (one workgroup) adds the
// workgroups' partial sums.  Every sum has a fixed order: results are bitwise reproducible.
//
// Top-1 accuracy: per (J, a) the tile's maximum goes to a "before the positive" or "after the positive" slot (ties before
// the positive beat it, ties after do not -- torch.argmax takes the first maximum); the diagonal tile splits per element.
// sum of all scores (negative_similarity_mean): sum_ab n_a . c_b = (sum_a n_a) . (sum_b c_b) -- finish1 adds the operand
// images' columns instead of the kernel adding 67 M products.
#include "tt_score_bf16.h"
#include "tt_deferred.h"
#include "tt_score_cells.h"

#include <stdlib.h>

namespace {

using namespace ttscore;

constexpr int kSymWaves = 8;           // tiles J per workgroup
constexpr int kFin2Fold = 32;          // partial records a workgroup of the pre-reduction (score_sym_fold_kernel) folds into one
constexpr int kSymThreads = kSymWaves * 64;

// x[lane] + x[lane ^ 32] in every lane: v_permlane32_swap exchanges the upper half of one register with the lower half of the
// other -- on two copies of x that leaves {lo, lo} and {hi, hi}.  A VALU op: no LDS round trip as __shfl_xor(x, 32) (ds_bpermute)
// (inline asm: through __builtin_amdgcn_permlane32_swap hipcc 7.2 drops the second result and adds r[0] to itself.  The
//  s_nop covers the VALU-write -> permlane-read wait states the compiler would have inserted for its own instruction)
__device__ __forceinline__ void half_swap(float x, float& lo, float& hi) {
  unsigned a = __builtin_bit_cast(unsigned, x), b = a;
  asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b));
  lo = __builtin_bit_cast(float, a);
  hi = __builtin_bit_cast(float, b);
}
__device__ __forceinline__ float half_sum(float x) {
  float p, q;
  half_swap(x, p, q);
  return p + q;
}
__device__ __forceinline__ float half_max(float x) {
  float p, q;
  half_swap(x, p, q);
  return fmaxf(p, q);
}

struct SymArgs {
  const void* a_rows;                  // notice image (rows image: bf16, or fp8 for the FP8 kernels), may carry the exponent scale
  const void* b_rows;                  // company image
  int R, nT, NI;                       // rows, 32-row tiles, notice tiles per workgroup
  int64_t Rp;                          // slab row stride (floats)
  float c1, c2;                        // non-unit form: exp2(acc * c1 + c2)
  float* rs; float* mb; float* ma;     // [n_groups][Rp]: exp-sum / max before / max after the positive, per (J group, a)
  float* cs;                           // [n_chunks][Rp]: exp-sum per (a chunk, b)
  float* diag_raw;                     // [R] the positives' products, as the MFMA delivers them
  int want_rank;
  const void* a_lo;                    // bf16x3 (X3 kernels): the lo rows images
  const void* b_lo;
  const float* lq_n;                   // LQ kernels: [R] log sampling probabilities of the notice rows a / company rows b
  const float* lq_c;
  const int32_t* ent_n;                // MK kernels: [R] notice / company ids of the rows (the same row stands for one pair)
  const int32_t* ent_c;
  // XN kernels (tt_score_fwd_sym_bf16_xneg): Rx shared extra negatives, a packed image of their own -- workgroups blockIdx.x >= ngi
  // sweep ITS tiles (nTx of them) against the notice tiles
  const void* x_rows;
  int Rx, nTx, ngi;
  const float* lq_x;                   // [Rx] log sampling probabilities of the extras (LQ) or NULL: weight 1
  const int32_t* ent_x;                // [Rx] company ids of the extras (MK) or NULL: never masked
};
// KP kernels (tt_score_fwd_sym_bf16_cells) take the masked cells' plan behind the other arguments: a type of their own, so that every
// other instantiation keeps its argument block -- and with it its code -- as it was
struct SymArgsKP : SymArgs {
  TtCellsPlan kp;
};

// Notice tiles are staged through LDS once per WORKGROUP (all 8 waves sweep the same tiles I): read straight from L2 by
// every wave, the operand stream was 4 KB per 32 x 32 tile -- 268 MB per launch at B = 8192, D = 64 -- and the kernel ran at
// the L2's ~11 TB/s, not at its VALU rate.  A stage = TS tiles (8 KB; 16 KB at D = 64 and D = 256) in the images' own fragment order, so
// the copy is verbatim (16 bytes per thread) and a wave's ds_read_b128 of a fragment is 1 KB contiguous: conflict-free.
// Double buffered, one barrier per stage; the next stage's global loads are in flight while this one is computed.
// X3: a staged tile is the hi image's tile followed by the lo image's (kImgB bytes each).
template <int KS, bool FP8, bool X3 = false>
struct SymStage {
  static constexpr int kImgB = FP8 ? KS * 512 : KS * 1024;                  // bytes of one 32-row tile of the rows image
  static constexpr int kTileB = X3 ? 2 * kImgB : kImgB;
  // tiles per stage (D = 64: 2 -> 4 tiles, half the barriers: sweep 22.2 -> 20.8 us).  8-KB tiles: 2 for bf16 D = 128; the fp8
  // D = 256 kernel holds two company tiles per wave and spills with two notice tiles' fragments in flight (256 VGPRs + scratch)
  static constexpr int TS = kTileB <= 4096 ? 4 : ((kTileB <= 8192 && !FP8) ? 2 : 1);
  static constexpr int kBytes = TS * kTileB;
  static constexpr int LPT = kBytes / (kSymThreads * 16);                   // 16-byte pieces per thread per stage
  static_assert(LPT >= 1 && LPT * kSymThreads * 16 == kBytes && kImgB % 1024 == 0, "stage must be whole 16-byte pieces, a wave's 64 inside one tile");
};

// JT company tiles per wave (fp8, D = 256: 2).  With one tile per wave and one notice tile per stage a wave meets a workgroup
// barrier every 32 x 32 tile and waits 35 % of its life (profiles/r03_pmc_configs4_fp8.json); with two, a stage's fragments feed two
// MFMA chains, the barriers and stage copies per score halve, and the slab of row partials has half the rows.  The two tiles'
// row partials are added (and their maxima joined) in registers before the slot is written: tiles J0, J0 + 1 lie on the same
// side of the positives of every notice tile but their own.
// X3: bf16x3 operands -- the S tile is mfma_s's three chains (hi_b lo_a, lo_b hi_a, hi_b hi_a): bit-identical to the directional
// x3 forward's row direction.
// LQ: logQ-corrected sums (tt_score_fwd_sym_bf16_lq): row sums add e_ab w_b, column sums e_ab u_a, with w / u the sampling weights
// of the companies / notices (tt_lq_weight).  w_b is per register -- 16 weights per lane, formed once for the resident tile J;
// u_a is per lane -- the workgroup forms the weights of its NI * 32 notice rows once, into LDS behind the stage buffers, and a
// wave reads one per swept tile.  The column accumulators take an fma where they took an add; the row partial two fma chains.  (Plain fmas, not inline asm: an
// asm fma reading the v_exp_f32 result right behind it skips the trans-use wait state the compiler inserts for its own ops.)
// MK: the repeated-entity mask (tt_score_fwd_sym_bf16_mask): e_ab of a pair a != b whose rows share a notice or a company id is zeroed
// before it enters either sum; the maxima (ranks) and the diagonal stay on the raw scores.  The a rows' two ids ride in LDS behind
// s_wn, [2][NI * 32], read one pair per swept tile; the resident tile's 2 x 16 ids are per register -- at D = 256 in LDS, [2][wave][32],
// as WLDS keeps the weights (ELDS).  Ids past R are never compared: those rows are only met on the per-element path, behind `valid`.
// XN: shared extra negatives (tt_score_fwd_sym_bf16_xneg).  The company tiles run past the in-batch ones into the extras' own image:
// a workgroup blockIdx.x >= ngi keeps 8 tiles of X resident (`isx`, workgroup-uniform).  Such a tile has no positive, so no diagonal
// and every maximum in the "after the positive" slot (a tie with an extra does not beat the positive); it feeds the row direction
// only -- the column accumulators are dropped; its LQ weight comes from lq_x (NULL: 1), its mask is ent_c[a] == ent_x[m] alone
// (NULL ent_x: never).  The row partials land in slab rows ngi .., which finish1 adds behind the in-batch ones.  The in-batch
// workgroups run the code of the form without extras: colsum and diag keep their bits.
// KP: masked cells (tt_score_fwd_sym_bf16_cells).  Per swept tile pair the wave reads the pair's two plan offsets (wave-uniform) and,
// only when the span is not empty, walks its cells into one 16-bit mask per lane (tt_cells_mask); e_ab of a listed cell is zeroed
// where masked() zeroes it -- behind ex(), in front of both sums; the maxima, dg and the rank path never see it.  The plan holds no
// diagonal cell.  An extras' tile (isx) is column tile nT + J of the plan.
template <int KS, bool UNIT, bool FP8, int JT, bool X3 = false, bool LQ = false, bool MK = false, bool XN = false, bool KP = false>
__global__ __launch_bounds__(kSymThreads) void score_fwd_sym_kernel(std::conditional_t<KP, SymArgsKP, SymArgs> g) {
  using ST = SymStage<KS, FP8, X3>;
  constexpr int TS = ST::TS, LPT = ST::LPT, kTileB = ST::kTileB, kImgB = ST::kImgB, K64 = FP8 ? KS / 4 : 1, KL = X3 ? KS : 1;
  static_assert(!X3 || (!FP8 && JT == 1), "bf16x3: bf16 images, one company tile per wave");
  static_assert(!FP8 || KS % 4 == 0, "fp8 operands come in K = 64 steps");
  extern __shared__ __attribute__((aligned(16))) float lds[];  // [3][8 waves][NI * 32] slots | 2 stage buffers
  const int lane = threadIdx.x & 63, c = lane & 31, h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int NI = g.NI, nT = g.nT, R = g.R;
  const int slots = NI * 32;
  float* s_sum = lds + (0 * kSymWaves + wave) * slots;
  float* s_mb = lds + (1 * kSymWaves + wave) * slots;
  float* s_ma = lds + (2 * kSymWaves + wave) * slots;
  char* stage = reinterpret_cast<char*>(lds + 3 * kSymWaves * slots);
  float* s_wn = reinterpret_cast<float*>(stage + 2 * ST::kBytes);   // (LQ) [NI * 32] notice weights u_a
  // (LQ, bf16x3 at D = 256: the resident tile's company weights live in LDS, [wave][32], read per tile -- in registers they spilled)
  constexpr bool WLDS = LQ && X3 && KS == 16;
  float* s_wc = s_wn + NI * 32 + wave * 32;
  static_assert(!MK || (!FP8 && !X3 && JT == 1), "the repeated-entity mask: bf16 operands only");
  static_assert(!XN || (!FP8 && !X3 && JT == 1), "extra negatives: bf16 operands only");
  static_assert(!KP || (!FP8 && !X3 && JT == 1 && !MK), "masked cells: bf16 operands only, not beside the repeated-entity mask");
  constexpr bool ELDS = MK && KS == 16;
  int* s_ean = reinterpret_cast<int*>(s_wn + (LQ ? NI * 32 + kSymWaves * 32 : 0));   // (MK) [NI * 32] notice ids of the a rows
  int* s_eac = s_ean + NI * 32;                                                       //      their company ids
  int* s_ebn = s_eac + NI * 32 + wave * 32;                                           // (ELDS) the resident tile's ids, [2][wave][32]
  int* s_ebc = s_ebn + kSymWaves * 32;
  bool isx = false;                                        // (XN) this workgroup's resident tiles are tiles of the extras' image
  if constexpr (XN) isx = (int)blockIdx.x >= g.ngi;
  const int J0 = XN ? (((int)blockIdx.x - (isx ? g.ngi : 0)) * kSymWaves + wave)
                    : ((int)blockIdx.x * kSymWaves + wave) * JT;  // this wave's company tiles J0 .. J0 + JT - 1
  const int I0 = (int)blockIdx.y * NI, I1 = min(I0 + NI, nT);
  const int nTj = XN && isx ? g.nTx : nT, Rj = XN && isx ? g.Rx : R;   // the resident side's tiles / rows
  const bool active = J0 < nTj;
  for (int i = lane; i < slots; i += 64) { s_sum[i] = 0.f; s_mb[i] = kNegBig; s_ma[i] = kNegBig; }
  float wb[JT][WLDS ? 1 : 16];                             // (LQ) company weights w_b of the resident tiles, 0 past R
  if constexpr (LQ) {
    static_assert(!FP8, "logQ correction: bf16 and bf16x3 operands only");
    for (int i = threadIdx.x; i < slots; i += kSymThreads) {
      const int a = I0 * 32 + i;
      s_wn[i] = a < R ? tt_lq_weight(g.lq_n[a]) : 0.f;    // (read after the sweep's first barrier)
    }
    if constexpr (WLDS) {
      if (lane < 32) s_wc[lane] = 32 * J0 + lane < R ? tt_lq_weight(g.lq_c[32 * J0 + lane]) : 0.f;
    } else if constexpr (XN) {
      const float* const lqj = isx ? g.lq_x : g.lq_c;      // (NULL lq_x: the extras uncorrected -- weight tt_lq_weight(0))
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int b = 32 * J0 + rowmap(r, h);
        wb[0][(WLDS ? 0 : r)] = b < Rj ? tt_lq_weight(lqj ? lqj[b] : 0.f) : 0.f;
      }
    } else {
#pragma unroll
      for (int j = 0; j < JT; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int b = 32 * (J0 + j) + rowmap(r, h);
          wb[j][(WLDS ? 0 : r)] = b < R ? tt_lq_weight(g.lq_c[b]) : 0.f;
        }
    }
  }
  [[maybe_unused]] int ebn[ELDS ? 1 : 16], ebc[ELDS ? 1 : 16];   // (MK) ids of the resident tile's rows b
  if constexpr (MK) {
    for (int i = threadIdx.x; i < slots; i += kSymThreads) {
      const int a = I0 * 32 + i;
      s_ean[i] = a < R ? g.ent_n[a] : 0;                  // (read after the sweep's first barrier)
      s_eac[i] = a < R ? g.ent_c[a] : 0;
    }
    if (XN && isx) {                                       // the extras' company ids; no notice ids (never read: `masked`)
      const bool have = g.ent_x != nullptr;
      if constexpr (ELDS) {
        if (lane < 32) {
          const int b = 32 * J0 + lane;
          s_ebn[lane] = 0;
          s_ebc[lane] = (have && b < Rj) ? g.ent_x[b] : 0;
        }
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int b = 32 * J0 + rowmap(r, h);
          ebn[(ELDS ? 0 : r)] = 0;
          ebc[(ELDS ? 0 : r)] = (have && b < Rj) ? g.ent_x[b] : 0;
        }
      }
    } else if constexpr (ELDS) {
      if (lane < 32) {
        const int b = 32 * J0 + lane;
        s_ebn[lane] = b < R ? g.ent_n[b] : 0;
        s_ebc[lane] = b < R ? g.ent_c[b] : 0;
      }
    } else {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int b = 32 * J0 + rowmap(r, h);
        ebn[(ELDS ? 0 : r)] = b < R ? g.ent_n[b] : 0;
        ebc[(ELDS ? 0 : r)] = b < R ? g.ent_c[b] : 0;
      }
    }
  }
  const bool xmask = XN && MK && isx && g.ent_x != nullptr;   // (XN) the extras carry ids
  // (MK) is (a, register r of the resident tile) a masked pair?  (the diagonal: the caller's business)
  auto masked = [&](int ean, int eac, int r) -> bool {
    if constexpr (XN) {
      if (isx) {                                           // an extra: the row's own company, or a repeat of it
        if constexpr (ELDS) return xmask && eac == s_ebc[rowmap(r, h)];
        else return xmask && eac == ebc[(ELDS ? 0 : r)];
      }
    }
    if constexpr (ELDS) return same_entity(ean, eac, s_ebn[rowmap(r, h)], s_ebc[rowmap(r, h)]);
    else return same_entity(ean, eac, ebn[(ELDS ? 0 : r)], ebc[(ELDS ? 0 : r)]);
  };
  // the company weight of register r (resident tile j)
  auto wreg = [&](int j, int r) -> float { if constexpr (WLDS) return s_wc[rowmap(r, h)]; else return wb[j][(WLDS ? 0 : r)]; };
  const float c1 = g.c1, c2 = g.c2;
  auto ex = [&](float x) { return UNIT ? __builtin_amdgcn_exp2f(x) : __builtin_amdgcn_exp2f(__builtin_fmaf(x, c1, c2)); };
  float colacc[JT][16];
#pragma unroll
  for (int j = 0; j < JT; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) colacc[j][r] = 0.f;
  bf16x8 bres[JT][FP8 ? 1 : KS];
  bf16x8 bres_lo[JT][KL];
  i32x8 bres8[JT][K64];
  const int n_full = R / 32;                               // tiles below n_full hold 32 valid rows
  bool jact[JT], jfull[JT];
  float dg_keep[JT];                                       // the positives of tile J (met once per wave, if J is in this chunk)
#pragma unroll
  for (int j = 0; j < JT; ++j) {
    jact[j] = J0 + j < nTj;
    jfull[j] = jact[j] && J0 + j < (XN ? Rj / 32 : n_full);
    dg_keep[j] = kNegBig;
    if (FP8) load_f8frag<K64>(reinterpret_cast<const char*>(g.b_rows), jact[j] ? J0 + j : 0, c, h, bres8[j]);
    else load_bfrag<(FP8 ? 1 : KS)>(reinterpret_cast<const __bf16*>(XN && isx ? g.x_rows : g.b_rows), jact[j] ? J0 + j : 0, c, h, bres[j]);
    if (X3) load_bfrag<KL>(reinterpret_cast<const __bf16*>(g.b_lo), jact[j] ? J0 + j : 0, c, h, bres_lo[j]);
  }
  // stage loader: the stage's tiles go STRAIGHT into the LDS buffer by LDS-DMA (global_load_lds_dwordx4: lane l of a wave writes
  // 16 bytes at the wave's base + 16 l), piece p = tid + 512 q of the stage at byte 16 p; tiles past the image's end are clamped
  // to its last tile (their results are never used).  Round 3: the copy used to pass through two named registers per thread and a
  // ds_write; the DMA of stage st + 1 is issued right behind the barrier that frees its buffer and has the whole stage to land.
  const int nst = (I1 - I0 + TS - 1) / TS;
  auto stage_dma = [&](int st, int buf) {
#pragma unroll
    for (int q = 0; q < LPT; ++q) {
      const int off = (q * kSymThreads + (int)threadIdx.x) * 16;           // byte offset inside the stage
      const int tl = off / kTileB;                                         // tile of the stage this piece belongs to (wave-uniform)
      const int tile = min(I0 + st * TS + tl, nT - 1);
      const int in = off - tl * kTileB;                                    // X3: >= kImgB = the lo image's tile (wave-uniform)
      const char* src = (X3 && in >= kImgB) ? reinterpret_cast<const char*>(g.a_lo) + (int64_t)tile * kImgB + (in - kImgB)
                                            : reinterpret_cast<const char*>(g.a_rows) + (int64_t)tile * kImgB + in;
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                       (__attribute__((address_space(3))) void*)(stage + buf * ST::kBytes + (q * kSymThreads + wave * 64) * 16), 16, 0, 0);
    }
  };
  stage_dma(0, 0);
  for (int st = 0; st < nst; ++st) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // this wave's pieces of stage st have landed ...
    __syncthreads();                                       // ... and everybody's; the other buffer is no longer read by anyone
    if (st + 1 < nst) stage_dma(st + 1, (st + 1) & 1);
    if (active) {
      const char* sb = stage + (st & 1) * ST::kBytes;
#pragma unroll
      for (int tl = 0; tl < TS; ++tl) {
        const int I = I0 + st * TS + tl;
        // the tile's fragments in one burst of LDS reads (left to itself hipcc reads two, waits, issues two MFMAs, reads two
        // ...: at D = 256 every second MFMA then pays a full LDS round trip), the MFMA chains behind counted lgkmcnt waits
        f32x16 acc[JT];
#pragma unroll
        for (int j = 0; j < JT; ++j)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
        if (FP8) {
          i32x8 af8[K64];
          load_f8frag<K64>(sb, tl, c, h, af8);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int s = 0; s < K64; ++s)
#pragma unroll
            for (int j = 0; j < JT; ++j) acc[j] = mfma_f8(bres8[j][s], af8[s], acc[j]);
        } else if (X3) {
          // mfma_s's order with the notice fragments read in two bursts: the lo fragments feed the first chain only
          bf16x8 af[KS];
#pragma unroll
          for (int s = 0; s < KS; ++s) af[s] = *reinterpret_cast<const bf16x8*>(sb + tl * kTileB + kImgB + ((s * 2 + h) * 32 + c) * 16);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int s = 0; s < KS; ++s) acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bres[0][s], af[s], acc[0], 0, 0, 0);
#pragma unroll
          for (int s = 0; s < KS; ++s) af[s] = *reinterpret_cast<const bf16x8*>(sb + tl * kTileB + ((s * 2 + h) * 32 + c) * 16);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int s = 0; s < KS; ++s) acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bres_lo[0][s], af[s], acc[0], 0, 0, 0);
#pragma unroll
          for (int s = 0; s < KS; ++s) acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bres[0][s], af[s], acc[0], 0, 0, 0);
        } else {
          bf16x8 af[FP8 ? 1 : KS];
#pragma unroll
          for (int s = 0; s < (FP8 ? 1 : KS); ++s) af[s] = *reinterpret_cast<const bf16x8*>(sb + (((tl * KS + s) * 2 + h) * 32 + c) * 16);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int s = 0; s < (FP8 ? 1 : KS); ++s)
#pragma unroll
            for (int j = 0; j < JT; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bres[j][s], af[s], acc[j], 0, 0, 0);
        }
        const int il = (I - I0) * 32 + c;
        const float ua = LQ ? s_wn[il] : 1.f;
        [[maybe_unused]] int ean = 0, eac = 0;
        if constexpr (MK) { ean = s_ean[il]; eac = s_eac[il]; }
        float rs_tot = 0.f, xb_tot = kNegBig, xa_tot = kNegBig;
#pragma unroll
        for (int j = 0; j < JT; ++j) {
          const int J = J0 + j;
          [[maybe_unused]] unsigned km = 0;                // (KP) this lane's listed elements of the tile pair
          if constexpr (KP) {
            if (I < I1 && jact[j]) km = tt_cells_mask(g.kp, I, (XN && isx) ? nT + J : J, c, h, false);
          }
          if (I < I1 && (I != J || (XN && isx)) && I < n_full && jfull[j]) {  // plain tile: 32 x 32 valid scores, all on one side of the positives
            float e[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) e[r] = ex(acc[j][r]);
            if constexpr (KP) {
              if (__builtin_amdgcn_ballot_w64(km != 0)) {
#pragma unroll
                for (int r = 0; r < 16; ++r) e[r] = (km >> r) & 1u ? 0.f : e[r];
              }
            }
            if constexpr (MK) {                            // (I != J: no positive in this tile)
#pragma unroll
              for (int r = 0; r < 16; ++r) e[r] = masked(ean, eac, r) ? 0.f : e[r];
            }
            if constexpr (LQ) {
              if (!(XN && isx)) {                          // (the extras stand in no column sum)
#pragma unroll
              for (int r = 0; r < 16; ++r) colacc[j][r] = __builtin_fmaf(e[r], ua, colacc[j][r]);
              }
              float t0 = e[0] * wreg(j, 0), t1 = e[8] * wreg(j, 8);
#pragma unroll
              for (int r = 1; r < 8; ++r) { t0 = __builtin_fmaf(e[r], wreg(j, r), t0); t1 = __builtin_fmaf(e[8 + r], wreg(j, 8 + r), t1); }
              rs_tot += half_sum(t0 + t1);
            } else {
            if (!(XN && isx)) {
#pragma unroll
            for (int r = 0; r < 16; ++r) colacc[j][r] = add_asm(colacc[j][r], e[r]);
            }
            float t0 = (e[0] + e[1]) + (e[2] + e[3]), t1 = (e[4] + e[5]) + (e[6] + e[7]);
            float t2 = (e[8] + e[9]) + (e[10] + e[11]), t3 = (e[12] + e[13]) + (e[14] + e[15]);
            rs_tot += half_sum((t0 + t1) + (t2 + t3));
            }
            if (g.want_rank) {
              float m = max3_asm(acc[j][0], acc[j][1], acc[j][2]);
#pragma unroll
              for (int r = 3; r < 15; r += 2) m = max3_asm(m, acc[j][r], acc[j][r + 1]);
              m = half_max(fmaxf(m, acc[j][15]));
              // every b of tile J lies before (J < I) / after the positive of every a of tile I
              if (J < I && !(XN && isx)) xb_tot = fmaxf(xb_tot, m);
              else xa_tot = fmaxf(xa_tot, m);
            }
          } else if (I < I1 && jact[j]) {                  // the diagonal tile and the ragged last tiles: per element
            const int a = 32 * I + c;
            float rsum = 0.f, xb = kNegBig, xa = kNegBig, dg = kNegBig;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const int b = 32 * J + rowmap(r, h);
              const float x = acc[j][r];
              const bool valid = b < Rj && a < R;
              float e = valid ? ex(x) : 0.f;
              if constexpr (XN) {
                if (isx) {                                 // an extra: no positive, no column sum, behind every in-batch column
                  if constexpr (MK) e = masked(ean, eac, r) ? 0.f : e;
                  if constexpr (KP) e = (km >> r) & 1u ? 0.f : e;
                  if constexpr (LQ) rsum = __builtin_fmaf(e, wreg(j, r), rsum);
                  else rsum += e;
                  xa = valid ? fmaxf(xa, x) : xa;
                  continue;
                }
              }
              if constexpr (MK) e = (b != a && masked(ean, eac, r)) ? 0.f : e;
              if constexpr (KP) e = (b != a && ((km >> r) & 1u)) ? 0.f : e;
              if constexpr (LQ) {
                colacc[j][r] = __builtin_fmaf(e, ua, colacc[j][r]);
                rsum = __builtin_fmaf(e, wreg(j, r), rsum);
              } else {
                colacc[j][r] += e;
                rsum += e;
              }
              xb = (valid && b < a) ? fmaxf(xb, x) : xb;
              xa = (valid && b > a) ? fmaxf(xa, x) : xa;
              dg = (b == a) ? x : dg;
            }
            rs_tot += half_sum(rsum);
            xb_tot = fmaxf(xb_tot, half_max(xb));
            xa_tot = fmaxf(xa_tot, half_max(xa));
            dg = half_max(dg);
            if (I == J && !(XN && isx)) dg_keep[j] = dg;                   // taken from the MFMA result itself, so ties compare bit for bit
          }
        }
        if (I < I1 && h == 0) { s_sum[il] = rs_tot; s_mb[il] = xb_tot; s_ma[il] = xa_tot; }
      }
    }
  }
  if (active && !(XN && isx)) {
#pragma unroll
    for (int j = 0; j < JT; ++j) {
      const int J = J0 + j;
      if (!jact[j]) continue;
      if (J >= I0 && J < I1 && h == 0 && 32 * J + c < R) g.diag_raw[32 * J + c] = dg_keep[j];
      // column direction: one cross-lane reduction per sweep (fixed butterfly order), lanes c == 0 hold the 32 sums
#pragma unroll
      for (int o = 16; o > 0; o >>= 1)
#pragma unroll
        for (int r = 0; r < 16; ++r) colacc[j][r] += __shfl_xor(colacc[j][r], o);
      if (c == 0) {
        float* dst = g.cs + (int64_t)blockIdx.y * g.Rp + 32 * J;
#pragma unroll
        for (int r = 0; r < 16; ++r) dst[rowmap(r, h)] = colacc[j][r];  // (rows beyond R: slab padding, never read)
      }
    }
  }
  __syncthreads();
  // row direction: the 8 waves' slots in wave order -> one partial per (J group, a)
  for (int i = threadIdx.x; i < slots; i += kSymThreads) {
    const int a = I0 * 32 + i;                              // < Rp by construction (sym_layout)
    float s = 0.f, xb = kNegBig, xa = kNegBig;
#pragma unroll
    for (int w = 0; w < kSymWaves; ++w) {
      s += lds[(0 * kSymWaves + w) * slots + i];
      xb = fmaxf(xb, lds[(1 * kSymWaves + w) * slots + i]);
      xa = fmaxf(xa, lds[(2 * kSymWaves + w) * slots + i]);
    }
    const int64_t o = (int64_t)blockIdx.x * g.Rp + a;
    g.rs[o] = s;
    if (g.want_rank) { g.mb[o] = xb; g.ma[o] = xa; }
  }
}

// finish2 reads every workgroup's partial record in ONE workgroup: 4.6 us for 128 records (B = 8192), 50 us for 1024 (B = 65536:
// 2 MB through one CU).  From 256 records on, this launch folds them 32 to one first (fixed order: record k of the fold after
// record k - 1), and finish2 adds the folded ones.
__global__ __launch_bounds__(1024) void score_sym_fold_kernel(const float* __restrict__ part, int n_wg, int stride, float* __restrict__ part2) {
  const int j = threadIdx.x;
  if (j >= stride) return;
  const int r0 = (int)blockIdx.x * kFin2Fold, r1 = min(r0 + kFin2Fold, n_wg);
  float v[kFin2Fold];
#pragma unroll
  for (int k = 0; k < kFin2Fold; ++k) v[k] = r0 + k < r1 ? part[(int64_t)(r0 + k) * stride + j] : 0.f;
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < kFin2Fold; ++k) s += v[k];
  part2[(int64_t)blockIdx.x * stride + j] = s;
}

// ---- finish1: slabs -> per-row sums, reciprocals, top-1 flags; per-workgroup partial sums of the loss terms; column sums
// of both operand images (for the sum of all scores).  64 rows per workgroup: wave q adds the slab rows g = q, q + 4, ...
// (independent loads, 8 in flight), the four partial results are combined in wave order.
constexpr int kFinRows = 64;
struct Fin1Args {
  const float* rs; const float* mb; const float* ma; const float* cs; const float* diag_raw;
  int n_groups, n_chunks, R, KS;
  int64_t Rp;
  float kexp, unscale, shift;
  int unit, want_rank;
  float* rowsum; float* colsum; float* inv_row; float* inv_col; float* diag; int32_t* row_rank;
  const void* a_rows; const void* b_rows;
  int fp8;                             // the rows images hold fp8 (tt_score_bf16.h) instead of bf16
  const void* a_lo; const void* b_lo;  // bf16x3: the lo rows images (their columns are added to the hi images')
  float* part;                         // [n_wg][4 + 2 * Dp]: l, hits, dsum, (pad), U[Dp], V[Dp]
  const float* lq_n; const float* lq_c;  // LQ: [R] log sampling probabilities of the notice / company rows
  float* w_n; float* w_c;              // LQ: their weights tt_lq_weight(lq) (0 past R): what tt_score_bwd_bf16_lq takes
  const float* pw_g;                   // PW: [round_up(R, 64)] normalised pair weights (tt_score_prepare_pw)
  const float* lq_x; float* w_x; int Rx;   // XN: the extras' log probabilities (or NULL) -> their weights [round_up(Rx, 64)], 0 past Rx
};

__device__ __forceinline__ float slab_sum4(const float* __restrict__ slab, int64_t Rp, int n, int q, int i) {
  float s = 0.f;
  for (int g0 = q; g0 < n; g0 += 32) {
    float v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = g0 + 4 * k < n ? slab[(int64_t)(g0 + 4 * k) * Rp + i] : 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) s += v[k];
  }
  return s;
}
__device__ __forceinline__ float slab_max4(const float* __restrict__ slab, int64_t Rp, int n, int q, int i) {
  float s = kNegBig;
  for (int g0 = q; g0 < n; g0 += 32) {
    float v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = g0 + 4 * k < n ? slab[(int64_t)(g0 + 4 * k) * Rp + i] : kNegBig;
#pragma unroll
    for (int k = 0; k < 8; ++k) s = fmaxf(s, v[k]);
  }
  return s;
}

// LQ: the row and column terms subtract the positive's log weight (the corrected positive s_ii - lq_i), taken exactly as
// -kLqL - lq, never as the log of a rounded weight; the weights themselves go out for the backward.
// PW (tt_score_fwd_sym_bf16_pw): row i's loss term times its pair weight g_i, and the reciprocals FOLDED, g_i / rowsum_i and
// g_i / colsum_i -- the backward's off-diagonal weights e_ab (ia + ib) and e_ab (ua ib + wb ia) are then the weighted ones as they
// stand.  rowsum / colsum stay the unweighted sums.  (g_i = 1: every product below is exact -- the plain entry's bits.)
// XN (tt_score_fwd_sym_bf16_xneg): n_groups counts the extras' slab rows too; the extras' weights w_x go out for the backward (1
// without a correction: there the weight of an extra is the bare reciprocal's factor).
template <bool LQ = false, bool PW = false, bool XN = false>
__global__ __launch_bounds__(256) void score_sym_finish1_kernel(Fin1Args f) {
  const int t = threadIdx.x, lane = t & 63, q = t >> 6;
  if constexpr (XN) {
    const int Rxp = (f.Rx + 63) / 64 * 64;
    for (int m = (int)blockIdx.x * 256 + t; m < Rxp; m += (int)gridDim.x * 256)
      f.w_x[m] = m < f.Rx ? (LQ ? tt_lq_weight(f.lq_x ? f.lq_x[m] : 0.f) : 1.f) : 0.f;
  }
  const int i = blockIdx.x * kFinRows + lane;              // slab rows are padded: i < Rp always
  const int Dp = f.KS * 16, stride = 4 + 2 * Dp;
  float* part = f.part + (int64_t)blockIdx.x * stride;
  __shared__ float red[4][4][kFinRows];                    // [quantity][wave][row]
  red[0][q][lane] = slab_sum4(f.rs, f.Rp, f.n_groups, q, i);
  red[1][q][lane] = slab_sum4(f.cs, f.Rp, f.n_chunks, q, i);
  if (f.want_rank) {
    red[2][q][lane] = slab_max4(f.mb, f.Rp, f.n_groups, q, i);
    red[3][q][lane] = slab_max4(f.ma, f.Rp, f.n_groups, q, i);
  }
  // column sums of the images over this workgroup's 2 tiles.  bf16: chunk id = (k-step * 2 + half) * 32 + row, 8 values of
  // columns 16 ks + 8 half + j.  fp8: chunk id = ((k64-step * 2 + part) * 2 + half) * 32 + row, 16 values of columns
  // 64 s + 32 half + 16 part + j (as stored: the factor 64 is taken out again below).
  __shared__ float cols[2][256];
  if (!f.fp8) {
    const int chunks = f.KS * 64;                          // per tile
    for (int img = 0; img < 2; ++img) {
      const __bf16* base = reinterpret_cast<const __bf16*>(img ? f.b_rows : f.a_rows);
      const __bf16* lo = reinterpret_cast<const __bf16*>(img ? f.b_lo : f.a_lo);
      for (int ch0 = 0; ch0 < chunks; ch0 += 256) {
        const int ch = ch0 + t;
        float acc8[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc8[j] = 0.f;
        if (ch < chunks) {
#pragma unroll
          for (int qq = 0; qq < kFinRows / 32; ++qq) {
            const int64_t tile = (int64_t)blockIdx.x * (kFinRows / 32) + qq;
            if (tile * 32 < f.R) {                         // (rows beyond R inside a tile are zero in the image)
              const bf16x8 vv = *reinterpret_cast<const bf16x8*>(base + (tile * chunks + ch) * 8);
#pragma unroll
              for (int j = 0; j < 8; ++j) acc8[j] += (float)vv[j];
              if (lo) {
                const bf16x8 vl = *reinterpret_cast<const bf16x8*>(lo + (tile * chunks + ch) * 8);
#pragma unroll
                for (int j = 0; j < 8; ++j) acc8[j] += (float)vl[j];
              }
            }
          }
        }
        // the 32 threads of a (k-step, half) group hold the 32 rows: butterfly over the low 5 lane bits
#pragma unroll
        for (int o = 16; o > 0; o >>= 1)
#pragma unroll
          for (int j = 0; j < 8; ++j) acc8[j] += __shfl_xor(acc8[j], o);
        if (ch < chunks && (t & 31) == 0) {
          const int dbase = (ch >> 5) * 8;                 // (k-step * 2 + half) * 8 = first column of the chunk
#pragma unroll
          for (int j = 0; j < 8; ++j) cols[img][dbase + j] = acc8[j];
        }
      }
    }
  } else {
    const int chunks = f.KS * 32;                          // 16-byte chunks per tile: Dp * 32 / 16
    for (int img = 0; img < 2; ++img) {
      const char* base = reinterpret_cast<const char*>(img ? f.b_rows : f.a_rows);
      for (int ch0 = 0; ch0 < chunks; ch0 += 256) {
        const int ch = ch0 + t;
        float acc16[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) acc16[j] = 0.f;
        if (ch < chunks) {
#pragma unroll
          for (int qq = 0; qq < kFinRows / 32; ++qq) {
            const int64_t tile = (int64_t)blockIdx.x * (kFinRows / 32) + qq;
            if (tile * 32 < f.R) {
              const i32x4 vv = *reinterpret_cast<const i32x4*>(base + (tile * chunks + ch) * 16);
#pragma unroll
              for (int w4 = 0; w4 < 4; ++w4) {
                acc16[4 * w4 + 0] += __builtin_amdgcn_cvt_f32_fp8(vv[w4], 0);
                acc16[4 * w4 + 1] += __builtin_amdgcn_cvt_f32_fp8(vv[w4], 1);
                acc16[4 * w4 + 2] += __builtin_amdgcn_cvt_f32_fp8(vv[w4], 2);
                acc16[4 * w4 + 3] += __builtin_amdgcn_cvt_f32_fp8(vv[w4], 3);
              }
            }
          }
        }
#pragma unroll
        for (int o = 16; o > 0; o >>= 1)
#pragma unroll
          for (int j = 0; j < 16; ++j) acc16[j] += __shfl_xor(acc16[j], o);
        if (ch < chunks && (t & 31) == 0) {
          const int g5 = ch >> 5;                          // (s * 2 + part) * 2 + half
          const int dbase = 64 * (g5 >> 2) + 32 * (g5 & 1) + 16 * ((g5 >> 1) & 1);
#pragma unroll
          for (int j = 0; j < 16; ++j) cols[img][dbase + j] = acc16[j] * (1.f / kFp8Up);
        }
      }
    }
  }
  __syncthreads();
  float l = 0.f, hit = 0.f, dsum = 0.f;
  if (q == 0) {
    if (i < f.R) {
      const float rsum = (red[0][0][lane] + red[0][1][lane]) + (red[0][2][lane] + red[0][3][lane]);
      const float csum = (red[1][0][lane] + red[1][1][lane]) + (red[1][2][lane] + red[1][3][lane]);
      const float draw = f.diag_raw[i], d = draw * f.unscale;
      if constexpr (PW) {
        f.inv_row[i] = f.pw_g[i] * (1.f / rsum);
        f.inv_col[i] = f.pw_g[i] * (1.f / csum);
      } else {
      f.inv_row[i] = 1.f / rsum;
      f.inv_col[i] = 1.f / csum;
      }
      const float rs_shifted = f.unit ? rsum * f.kexp : rsum, cs_shifted = f.unit ? csum * f.kexp : csum;
      f.rowsum[i] = rs_shifted;
      f.colsum[i] = cs_shifted;
      f.diag[i] = d;
      if constexpr (LQ) {
        const float lqn = f.lq_n[i], lqc = f.lq_c[i];
        l = (logf(rs_shifted) + f.shift - d - tt_lq_log_weight(lqc)) + (logf(cs_shifted) + f.shift - d - tt_lq_log_weight(lqn));
        f.w_n[i] = tt_lq_weight(lqn);
        f.w_c[i] = tt_lq_weight(lqc);
      } else {
        l = (logf(rs_shifted) + f.shift - d) + (logf(cs_shifted) + f.shift - d);
      }
      if constexpr (PW) l *= f.pw_g[i];
      dsum = d;
      if (f.want_rank) {
        const float xb = fmaxf(fmaxf(red[2][0][lane], red[2][1][lane]), fmaxf(red[2][2][lane], red[2][3][lane]));
        const float xa = fmaxf(fmaxf(red[3][0][lane], red[3][1][lane]), fmaxf(red[3][2][lane], red[3][3][lane]));
        const int rk = (xb < draw && xa <= draw) ? 0 : 1;
        f.row_rank[i] = rk;
        hit = rk == 0 ? 1.f : 0.f;
      }
    } else {
      // rows past the end, up to this workgroup's 64: tt_score_bwd_bf16 reads the reciprocals a whole 32-row tile at a time
      f.inv_row[i] = 0.f; f.inv_col[i] = 0.f; f.rowsum[i] = 1.f; f.colsum[i] = 1.f;
      if constexpr (LQ) { f.w_n[i] = 0.f; f.w_c[i] = 0.f; }
    }
    float v[3] = {l, hit, dsum};                           // butterfly inside the one wave that holds the rows
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
#pragma unroll
      for (int j = 0; j < 3; ++j) v[j] += __shfl_xor(v[j], o);
    if (lane == 0) { part[0] = v[0]; part[1] = v[1]; part[2] = v[2]; part[3] = 0.f; }
  }
  for (int d = t; d < 2 * Dp; d += 256) part[4 + d] = cols[d / Dp][d % Dp];
}

__global__ __launch_bounds__(kRiderThreads) void score_sym_finish2_kernel(Finish2Rider fr) { finish2_body(fr); }

// ---- tt_score_prepare_pw: raw pair weights -> g = w' B / sum(w') --------------------------------------------------------------
// One workgroup.  w' keeps the positive finite entries (a bit test: sign clear, exponent not all ones, not zero) and zeroes the
// rest.  The sum has ONE order for a given B: thread t adds w'[t], w'[t + 1024], ...; a butterfly inside each wave; the 16 wave
// sums in wave order.  A power-of-two factor on every weight scales each partial sum, the total and B / total exactly, so g keeps
// its bits.  Entries B .. round_up(B, 64) - 1 are written as 0.
constexpr int kPwThreads = 1024;
__device__ __forceinline__ float pw_clamp(float w) {
  const uint32_t u = __float_as_uint(w);
  return (u - 1u) < 0x7f7fffffu ? w : 0.f;                 // 0 < bits < 0x7f800000
}
__global__ __launch_bounds__(kPwThreads) void score_prepare_pw_kernel(const float* __restrict__ w, int B, float* __restrict__ g) {
  __shared__ float sh[kPwThreads / 64];
  __shared__ float s_k;
  const int t = threadIdx.x;
  float s = 0.f;
  for (int i = t; i < B; i += kPwThreads) s += pw_clamp(w[i]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if ((t & 63) == 0) sh[t >> 6] = s;
  __syncthreads();
  if (t == 0) {
    float tot = 0.f;
    for (int q = 0; q < kPwThreads / 64; ++q) tot += sh[q];
    s_k = tot > 0.f ? (float)B / tot : 0.f;
  }
  __syncthreads();
  const float k = s_k;
  const int Bp = (B + 63) / 64 * 64;
  for (int i = t; i < Bp; i += kPwThreads) g[i] = i < B ? pw_clamp(w[i]) * k : 0.f;
}

struct SymLayout {
  int nT, NI, n_groups, n_chunks, n_wg, Dp;
  int nTx, n_groups_x;                 // extra negatives: their tiles and J groups (0 without)
  int64_t Rp;
  size_t off_rs, off_mb, off_ma, off_cs, off_diag, off_part, off_part2, bytes;
};

// Rx extra negatives add slab rows only: NI, the chunks and with them the column sums' order are the in-batch problem's
inline SymLayout sym_layout(const tt_ctx* ctx, int64_t R, int D, int64_t Rx = 0) {
  SymLayout L;
  L.Dp = padded_d(D);
  L.nT = (int)tt_cdiv(R, 32);
  L.n_groups = (int)tt_cdiv(L.nT, kSymWaves);
  L.nTx = (int)tt_cdiv(Rx, 32);
  L.n_groups_x = (int)tt_cdiv(L.nTx, kSymWaves);
  // notice tiles per workgroup: enough workgroups for ~2 per CU, at least 4 tiles per sweep, at most 32 (LDS: 3 * 8 * NI * 128 B)
  int ni = (int)tt_cdiv((int64_t)L.nT * L.n_groups, 2 * (ctx ? ctx->num_cus : 256));
  ni = ni < 4 ? 4 : (ni > 16 ? 16 : ni);                  // 16 tiles: 48 KB of LDS slots per workgroup
  ni = (ni + 3) / 4 * 4;                                  // whole stages (a stage is 1, 2 or 4 tiles)
  L.NI = ni;
  L.n_chunks = (int)tt_cdiv(L.nT, ni);
  L.n_wg = (int)tt_cdiv(R, kFinRows);
  L.Rp = rup((int64_t)L.n_chunks * ni * 32, 256);          // slab rows cover every slot a workgroup writes (>= R)
  size_t o = 0;
  auto take = [&](size_t n) { size_t at = o; o += (n + 255) & ~size_t(255); return at; };
  L.off_rs = take(sizeof(float) * (L.n_groups + L.n_groups_x) * L.Rp);
  L.off_mb = take(sizeof(float) * (L.n_groups + L.n_groups_x) * L.Rp);
  L.off_ma = take(sizeof(float) * (L.n_groups + L.n_groups_x) * L.Rp);
  L.off_cs = take(sizeof(float) * L.n_chunks * L.Rp);
  L.off_diag = take(sizeof(float) * L.Rp);
  L.off_part = take(sizeof(float) * L.n_wg * (4 + 2 * 256));   // (sized for the widest record: fp8 operands pad D up to 64)
  L.off_part2 = take(sizeof(float) * tt_cdiv(L.n_wg, kFin2Fold) * (4 + 2 * 256));
  L.bytes = o + 256;
  return L;
}

}  // namespace

// one call of the symmetric forward: what every entry requires, the operand kind, and the optional terms grouped as they travel
struct SymCall {
  const char* who;
  Operands op;
  const void *N_packed, *C_packed;
  int64_t B;
  int32_t D;
  float inv_t, shift, ab_scale;
  int32_t want_rank;
  float *rowsum, *colsum, *inv_row, *inv_col, *diag;
  int32_t* row_rank;
  float *out8, *loss_out;
  void* workspace;
  size_t workspace_bytes;
  tt_stream stream;
  struct { const float *lq_n, *lq_c; float *w_n, *w_c; } lq;        // logQ: the log sampling probabilities in, the sampling weights out
  struct { const int32_t *ent_n, *ent_c; } ids;                      // the repeated-entity mask
  const float* pw_g;                                                 // pair weights (tt_score_prepare_pw's g)
  struct { const void* X_packed; int64_t M; const float* lq_x; const int32_t* ent_x; float* w_x; } x;   // shared extra negatives
  struct { const int32_t* plan; int64_t capacity; } cells;           // masked cells
};

// the required part of a SymCall `s` from an entry's own parameters (every entry names them alike)
#define TT_SYM_CALL(s, who_, op_)                                                                                                  \
  SymCall s{};                                                                                                                     \
  s.who = who_; s.op = op_; s.N_packed = N_packed; s.C_packed = C_packed; s.B = B; s.D = D; s.inv_t = inv_t; s.shift = shift;      \
  s.ab_scale = ab_scale; s.want_rank = want_rank; s.rowsum = rowsum; s.colsum = colsum; s.inv_row = inv_row; s.inv_col = inv_col;  \
  s.diag = diag; s.row_rank = row_rank; s.out8 = out8; s.loss_out = loss_out; s.workspace = workspace;                             \
  s.workspace_bytes = workspace_bytes; s.stream = stream

// the terms an entry is for (sym_check_terms: those it requires; the fields of the others stay NULL / 0 in its SymCall)
enum : unsigned { kTermLq = 1, kTermIds = 2, kTermPw = 4, kTermXneg = 8, kTermCells = 16 };

// every pairing and range rule of the optional terms, once
static int sym_check_terms(const SymCall& s, unsigned needs) {
  const auto& q = s.lq;
  const auto& x = s.x;
  const bool m_ok = x.M >= 1 && x.M < ((int64_t)1 << 30);
  TT_CHECK_ARG(!(needs & kTermLq) || (q.lq_n && q.lq_c && q.w_n && q.w_c), "%s: NULL argument", s.who);
  TT_CHECK_ARG(!(needs & kTermIds) || (s.ids.ent_n && s.ids.ent_c), "%s: NULL ent_n / ent_c", s.who);
  TT_CHECK_ARG(!(needs & kTermPw) || s.pw_g, "%s: NULL g", s.who);
  TT_CHECK_ARG(!(needs & kTermXneg) || (x.X_packed && x.w_x), "%s: NULL X_packed / w_x", s.who);
  TT_CHECK_ARG(!(needs & kTermCells) || (s.cells.plan && tt_aligned(s.cells.plan, 16)), "%s: plan NULL or not 16-byte aligned", s.who);
  TT_CHECK_ARG(!(needs & kTermCells) || (s.cells.capacity >= 1 && s.cells.capacity < ((int64_t)1 << 30)), "%s: bad capacity %lld", s.who,
               (long long)s.cells.capacity);
  TT_CHECK_ARG(x.X_packed ? (m_ok && x.w_x) : x.M == 0, "%s: bad M=%lld (extras need M >= 1 and w_x)", s.who, (long long)x.M);
  TT_CHECK_ARG((s.ids.ent_n != nullptr) == (s.ids.ent_c != nullptr), "%s: ent_n and ent_c go together", s.who);
  TT_CHECK_ARG(!x.ent_x || s.ids.ent_c, "%s: ent_x needs ent_n / ent_c", s.who);
  TT_CHECK_ARG((q.lq_n != nullptr) == (q.lq_c != nullptr), "%s: lq_n and lq_c go together", s.who);
  TT_CHECK_ARG(!x.lq_x || (q.lq_n && x.X_packed), "%s: lq_x needs lq_n / lq_c and the extras", s.who);
  TT_CHECK_ARG(!q.lq_n || (q.w_n && q.w_c), "%s: the logQ correction needs w_n / w_c", s.who);
  return TT_OK;
}

// padded D = 32, 64, 128, 256 -> f(tt_c<KS>), KS = D / 16 k-steps
template <class F>
static int sym_by_dp(int Dp, F&& f) {
  switch (Dp) {
    case 32: return f(tt_c<2>);
    case 64: return f(tt_c<4>);
    case 128: return f(tt_c<8>);
    default: return f(tt_c<16>);
  }
}

static int sym_forward(tt_ctx* ctx, const SymCall& s, unsigned needs = 0) {
  if (int rc = sym_check_terms(s, needs)) return rc;
  const char* who = s.who;
  const void *N_packed = s.N_packed, *C_packed = s.C_packed, *X_packed = s.x.X_packed;
  const int64_t B = s.B, M = s.x.M;
  const int32_t D = s.D;
  const float inv_t = s.inv_t, shift = s.shift;
  const bool fp8 = s.op == Operands::fp8, x3 = s.op == Operands::bf16x3;
  const bool lq = s.lq.lq_n != nullptr;                    // with lq_c, w_n and w_c (sym_check_terms); without, no weights are written
  const bool mk = s.ids.ent_n != nullptr;
  const bool xn = X_packed != nullptr;
  const bool kp = s.cells.plan != nullptr;                 // (never with ent_*: tt_score_fwd_sym_bf16_cells takes none)
  TT_CHECK_ARG(ctx && N_packed && C_packed && s.rowsum && s.colsum && s.inv_row && s.inv_col && s.diag && s.out8 && s.workspace,
               "%s: NULL argument", who);
  TT_CHECK_ARG(!s.want_rank || s.row_rank, "%s: want_rank needs row_rank", who);
  TT_CHECK_ARG(B >= 1 && B < ((int64_t)1 << 30) && D >= 1 && D <= 256, "%s: bad shape B=%lld D=%d", who, (long long)B, D);
  if (2.f * fabsf(inv_t) > 80.f) {
    tt_set_error("%s: 1/temperature = %g: fixed-shift softmax needs 2/T <= 80", who, inv_t);
    return TT_ERR_UNSUPPORTED;
  }
  if (lq && 2.f * fabsf(inv_t) > kLqMaxTwoInvT) {
    tt_set_error("%s: 1/temperature = %g: the logQ-corrected softmax needs 2/T <= %g", who, inv_t, kLqMaxTwoInvT);
    return TT_ERR_UNSUPPORTED;
  }
  tt_ctx sized = *ctx;
  sized.num_cus = 256;                                     // the layout must not depend on the device: it sizes the workspace
  SymLayout L = sym_layout(&sized, B, D, M);
  if (fp8) L.Dp = padded_d8(D);                            // (the part record is sized for 256 columns: sym_layout)
  if (s.workspace_bytes < L.bytes) {
    tt_set_error("%s: workspace %zu < required %zu", who, s.workspace_bytes, L.bytes);
    return TT_ERR_WORKSPACE;
  }
  char* ws = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(s.workspace) + 255) & ~uintptr_t(255));
  const float ab = s.ab_scale == 0.f ? 1.f : s.ab_scale;
  const bool unit = ab == inv_t * kLog2e;                  // exactly: the caller got the scale from tt_score_unit_scale(inv_t)
  SymArgsKP g{};                                           // (the kernels without cells take its SymArgs part)
  g.a_rows = fp8 ? static_cast<const void*>(view8(N_packed, B, D).rows8) : static_cast<const void*>(view(N_packed, B, D).rows);
  g.b_rows = fp8 ? static_cast<const void*>(view8(C_packed, B, D).rows8) : static_cast<const void*>(view(C_packed, B, D).rows);
  if (x3) {
    g.a_lo = view_lo(N_packed, B, D).rows;
    g.b_lo = view_lo(C_packed, B, D).rows;
  }
  g.R = (int)B; g.nT = L.nT; g.NI = L.NI; g.Rp = L.Rp;
  g.c1 = inv_t * kLog2e / ab;
  g.c2 = -shift * kLog2e;
  g.rs = reinterpret_cast<float*>(ws + L.off_rs);
  g.mb = reinterpret_cast<float*>(ws + L.off_mb);
  g.ma = reinterpret_cast<float*>(ws + L.off_ma);
  g.cs = reinterpret_cast<float*>(ws + L.off_cs);
  g.diag_raw = reinterpret_cast<float*>(ws + L.off_diag);
  g.want_rank = s.want_rank ? 1 : 0;
  g.lq_n = s.lq.lq_n;
  g.lq_c = s.lq.lq_c;
  g.ent_n = s.ids.ent_n;
  g.ent_c = s.ids.ent_c;
  if (xn) {
    g.x_rows = view(X_packed, M, D).rows;
    g.Rx = (int)M; g.nTx = L.nTx; g.ngi = L.n_groups;
    g.lq_x = s.x.lq_x; g.ent_x = s.x.ent_x;
  }
  if (kp) g.kp = tt_cells_view(s.cells.plan, B, M, s.cells.capacity);
  hipStream_t st = reinterpret_cast<hipStream_t>(s.stream);
  // fp8, D = 256: two company tiles per wave (half the workgroups along J, half the slab rows)
  const int jt = (fp8 && L.Dp == 256) ? 2 : 1;
  const int n_groups = (int)tt_cdiv(L.nT, kSymWaves * jt) + L.n_groups_x;     // (extras: bf16 operands, jt = 1)
  const dim3 grid((unsigned)n_groups, (unsigned)L.n_chunks);
  const size_t slot_bytes = sizeof(float) * 3 * kSymWaves * L.NI * 32;
  const size_t wn_bytes = sizeof(float) * (L.NI * 32 + kSymWaves * 32);   // (LQ) notice weights (+ company weights, x3 D = 256)
  const size_t ent_bytes = sizeof(int) * 2 * (L.NI * 32 + kSymWaves * 32); // (MK) the a rows' ids (+ the resident tiles', D = 256)
  // one launch per form (fp8 has neither an x3 nor an LQ form, the mask bf16 operands only); only the x3, LQ and MK forms set their LDS limit
  const auto go = [&](auto ks, auto fp8c, auto x3c, auto lqc, auto mkc, auto xnc, auto kpc) -> int {
    constexpr int JT = fp8c && ks == 16 ? 2 : 1;                  // = jt
    const size_t lds = slot_bytes + 2 * SymStage<ks, fp8c, x3c>::kBytes + (lqc ? wn_bytes : 0) + (mkc ? ent_bytes : 0);
    return tt_dispatch([&](auto u) -> int {
      if constexpr (x3c || lqc || mkc || xnc || kpc) TT_LDS_ONCE(lds, &score_fwd_sym_kernel<ks, u, fp8c, JT, x3c, lqc, mkc, xnc, kpc>);
      score_fwd_sym_kernel<ks, u, fp8c, JT, x3c, lqc, mkc, xnc, kpc><<<grid, kSymThreads, lds, st>>>(g);
      return TT_OK;
    }, unit);
  };
  const std::false_type no{};
  const std::true_type yes{};
  // the legal flag sets: cells take LQ and XN, the extras LQ and MK, the mask LQ, fp8 nothing, plain bf16 X3 and LQ
  int rc;
  if (kp) {
    rc = tt_dispatch([&](auto lqc, auto xnc) { return sym_by_dp(L.Dp, [&](auto ks) { return go(ks, no, no, lqc, no, xnc, yes); }); }, lq, xn);
  } else if (xn) {
    rc = tt_dispatch([&](auto lqc, auto mkc) { return sym_by_dp(L.Dp, [&](auto ks) { return go(ks, no, no, lqc, mkc, yes, no); }); }, lq, mk);
  } else if (mk) {
    rc = tt_dispatch([&](auto lqc) { return sym_by_dp(L.Dp, [&](auto ks) { return go(ks, no, no, lqc, yes, no, no); }); }, lq);
  } else if (fp8) {
    rc = sym_by_dp(L.Dp, [&](auto ks) -> int {
      if constexpr (ks == 2) return TT_ERR_INVALID_ARG;      // (never: padded_d8 >= 64 -- fp8 has no K = 32 form to instantiate)
      else return go(ks, yes, no, no, no, no, no);
    });
  } else {
    rc = tt_dispatch([&](auto x3c, auto lqc) { return sym_by_dp(L.Dp, [&](auto ks) { return go(ks, no, x3c, lqc, no, no, no); }); }, x3, lq);
  }
  if (rc) return rc;
  TT_LAUNCH_CHECK();
  Fin1Args f{};
  f.rs = g.rs; f.mb = g.mb; f.ma = g.ma; f.cs = g.cs; f.diag_raw = g.diag_raw;
  f.n_groups = n_groups; f.n_chunks = L.n_chunks; f.R = (int)B; f.KS = L.Dp / 16; f.Rp = L.Rp;
  f.kexp = exp2f(g.c2); f.unscale = inv_t / ab; f.shift = shift; f.unit = unit ? 1 : 0; f.want_rank = g.want_rank;
  f.rowsum = s.rowsum; f.colsum = s.colsum; f.inv_row = s.inv_row; f.inv_col = s.inv_col; f.diag = s.diag; f.row_rank = s.row_rank;
  f.a_rows = g.a_rows; f.b_rows = g.b_rows;
  f.fp8 = fp8 ? 1 : 0;
  f.a_lo = g.a_lo; f.b_lo = g.b_lo;
  f.part = reinterpret_cast<float*>(ws + L.off_part);
  f.lq_n = s.lq.lq_n; f.lq_c = s.lq.lq_c; f.w_n = lq ? s.lq.w_n : nullptr; f.w_c = lq ? s.lq.w_c : nullptr;
  f.pw_g = s.pw_g;
  f.lq_x = s.x.lq_x; f.w_x = s.x.w_x; f.Rx = (int)M;
  if (xn) tt_dispatch([&](auto lqc) { score_sym_finish1_kernel<lqc, false, true><<<(unsigned)L.n_wg, 256, 0, st>>>(f); }, lq);
  else if (s.pw_g) tt_dispatch([&](auto lqc) { score_sym_finish1_kernel<lqc, true><<<(unsigned)L.n_wg, 256, 0, st>>>(f); }, lq);
  else if (lq) score_sym_finish1_kernel<true><<<(unsigned)L.n_wg, 256, 0, st>>>(f);
  else score_sym_finish1_kernel<<<(unsigned)L.n_wg, 256, 0, st>>>(f);
  TT_LAUNCH_CHECK();
  Finish2Rider fr{f.part, L.n_wg, L.Dp, (float)B, f.unscale, s.out8, s.loss_out};
  if (L.n_wg >= 256) {                                   // large batches: fold the records 32 to one before the one-workgroup reduction
    float* part2 = reinterpret_cast<float*>(ws + L.off_part2);
    const int n2 = (int)tt_cdiv(L.n_wg, kFin2Fold);
    score_sym_fold_kernel<<<n2, 1024, 0, st>>>(f.part, L.n_wg, 4 + 2 * L.Dp, part2);
    TT_LAUNCH_CHECK();
    fr.part = part2;
    fr.n_wg = n2;
  }
  if (ctx->dq->defer_riders & 2) return tt_deferred_queue_loss(ctx, st, fr);      // rides beside the towers' tail_bwd: nothing on the device reads it
  score_sym_finish2_kernel<<<1, kRiderThreads, 0, st>>>(fr);
  TT_LAUNCH_CHECK();
  return TT_OK;
}

extern "C" {

size_t tt_score_fwd_sym_workspace_bytes(int64_t B, int32_t D) {
  if (B < 1 || D < 1 || D > 256) return 0;
  tt_ctx fake{};
  fake.num_cus = 256;
  return sym_layout(&fake, B, D).bytes;
}

int tt_score_fwd_sym_bf16(tt_ctx* ctx, const void* N_packed, const void* C_packed, int64_t B, int32_t D, float inv_t, float shift,
                          float ab_scale, int32_t want_rank, float* rowsum, float* colsum, float* inv_row, float* inv_col,
                          float* diag, int32_t* row_rank, float* out8, float* loss_out, void* workspace, size_t workspace_bytes,
                          tt_stream stream) {
  TT_SYM_CALL(s, "tt_score_fwd_sym_bf16", Operands::bf16);
  return sym_forward(ctx, s);
}

int tt_score_fwd_sym_fp8(tt_ctx* ctx, const void* N_packed, const void* C_packed, int64_t B, int32_t D, float inv_t, float shift,
                         float ab_scale, int32_t want_rank, float* rowsum, float* colsum, float* inv_row, float* inv_col,
                         float* diag, int32_t* row_rank, float* out8, float* loss_out, void* workspace, size_t workspace_bytes,
                         tt_stream stream) {
  TT_SYM_CALL(s, "tt_score_fwd_sym_fp8", Operands::fp8);
  return sym_forward(ctx, s);
}

int tt_score_fwd_sym_bf16x3(tt_ctx* ctx, const void* N_packed, const void* C_packed, int64_t B, int32_t D, float inv_t, float shift,
                            float ab_scale, int32_t want_rank, float* rowsum, float* colsum, float* inv_row, float* inv_col,
                            float* diag, int32_t* row_rank, float* out8, float* loss_out, void* workspace, size_t workspace_bytes,
                            tt_stream stream) {
  TT_SYM_CALL(s, "tt_score_fwd_sym_bf16x3", Operands::bf16x3);
  return sym_forward(ctx, s);
}

int tt_score_fwd_sym_bf16_lq(tt_ctx* ctx, const void* N_packed, const void* C_packed, int64_t B, int32_t D, float inv_t, float shift,
                             float ab_scale, int32_t want_rank, const float* lq_n, const float* lq_c, float* rowsum, float* colsum,
                             float* inv_row, float* inv_col, float* w_n, float* w_c, float* diag, int32_t* row_rank, float* out8,
                             float* loss_out, void* workspace, size_t workspace_bytes, tt_stream stream) {
  TT_SYM_CALL(s, "tt_score_fwd_sym_bf16_lq", Operands::bf16);
  s.lq = {lq_n, lq_c, w_n, w_c};
  return sym_forward(ctx, s, kTermLq);
}

int tt_score_fwd_sym_bf16x3_lq(tt_ctx* ctx, const void* N_packed, const void* C_packed, int64_t B, int32_t D, float inv_t,
                               float shift, float ab_scale, int32_t want_rank, const float* lq_n, const float* lq_c, float* rowsum,
                               float* colsum, float* inv_row, float* inv_col, float* w_n, float* w_c, float* diag, int32_t* row_rank,
                               float* out8, float* loss_out, void* workspace, size_t workspace_bytes, tt_stream stream) {
  TT_SYM_CALL(s, "tt_score_fwd_sym_bf16x3_lq", Operands::bf16x3);
  s.lq = {lq_n, lq_c, w_n, w_c};
  return sym_forward(ctx, s, kTermLq);
}

int tt_score_fwd_sym_bf16_mask(tt_ctx* ctx, const void* N_packed, const void* C_packed, int64_t B, int32_t D, float inv_t,
                               float shift, float ab_scale, int32_t want_rank, const int32_t* ent_n, const int32_t* ent_c,
                               const float* lq_n, const float* lq_c, float* rowsum, float* colsum, float* inv_row, float* inv_col,
                               float* w_n, float* w_c, float* diag, int32_t* row_rank, float* out8, float* loss_out, void* workspace,
                               size_t workspace_bytes, tt_stream stream) {
  TT_SYM_CALL(s, "tt_score_fwd_sym_bf16_mask", Operands::bf16);
  s.ids = {ent_n, ent_c};
  s.lq = {lq_n, lq_c, w_n, w_c};
  return sym_forward(ctx, s, kTermIds);
}

size_t tt_score_fwd_sym_xneg_workspace_bytes(int64_t B, int64_t M, int32_t D) {
  if (B < 1 || M < 1 || D < 1 || D > 256) return 0;
  tt_ctx fake{};
  fake.num_cus = 256;
  return sym_layout(&fake, B, D, M).bytes;
}

int tt_score_fwd_sym_bf16_xneg(tt_ctx* ctx, const void* N_packed, const void* C_packed, const void* X_packed, int64_t B, int64_t M,
                               int32_t D, float inv_t, float shift, float ab_scale, int32_t want_rank, const int32_t* ent_n,
                               const int32_t* ent_c, const int32_t* ent_x, const float* lq_n, const float* lq_c, const float* lq_x,
                               float* rowsum, float* colsum, float* inv_row, float* inv_col, float* w_n, float* w_c, float* w_x,
                               float* diag, int32_t* row_rank, float* out8, float* loss_out, void* workspace, size_t workspace_bytes,
                               tt_stream stream) {
  TT_SYM_CALL(s, "tt_score_fwd_sym_bf16_xneg", Operands::bf16);
  s.x = {X_packed, M, lq_x, ent_x, w_x};
  s.ids = {ent_n, ent_c};
  s.lq = {lq_n, lq_c, w_n, w_c};
  return sym_forward(ctx, s, kTermXneg);
}

int tt_score_prepare_pw(tt_ctx* ctx, const float* w, int64_t B, float* g_out, tt_stream stream) {
  TT_CHECK_ARG(ctx && w && g_out, "tt_score_prepare_pw: NULL argument");
  TT_CHECK_ARG(B >= 1 && B < ((int64_t)1 << 30), "tt_score_prepare_pw: bad B=%lld", (long long)B);
  score_prepare_pw_kernel<<<1, kPwThreads, 0, reinterpret_cast<hipStream_t>(stream)>>>(w, (int)B, g_out);
  TT_LAUNCH_CHECK();
  return TT_OK;
}

int tt_score_fwd_sym_bf16_pw(tt_ctx* ctx, const void* N_packed, const void* C_packed, int64_t B, int32_t D, float inv_t, float shift,
                             float ab_scale, int32_t want_rank, const float* g, const int32_t* ent_n, const int32_t* ent_c,
                             const float* lq_n, const float* lq_c, float* rowsum, float* colsum, float* inv_row, float* inv_col,
                             float* w_n, float* w_c, float* diag, int32_t* row_rank, float* out8, float* loss_out, void* workspace,
                             size_t workspace_bytes, tt_stream stream) {
  TT_SYM_CALL(s, "tt_score_fwd_sym_bf16_pw", Operands::bf16);
  s.pw_g = g;
  s.ids = {ent_n, ent_c};
  s.lq = {lq_n, lq_c, w_n, w_c};
  return sym_forward(ctx, s, kTermPw);
}

int tt_score_fwd_sym_bf16_cells(tt_ctx* ctx, const void* N_packed, const void* C_packed, const void* X_packed, int64_t B, int64_t M,
                                int32_t D, float inv_t, float shift, float ab_scale, int32_t want_rank, const int32_t* plan,
                                int64_t capacity, const float* lq_n, const float* lq_c, const float* lq_x, float* rowsum, float* colsum, float* inv_row,
                                float* inv_col, float* w_n, float* w_c, float* w_x, float* diag, int32_t* row_rank, float* out8,
                                float* loss_out, void* workspace, size_t workspace_bytes, tt_stream stream) {
  TT_SYM_CALL(s, "tt_score_fwd_sym_bf16_cells", Operands::bf16);
  s.cells = {plan, capacity};
  s.x = {X_packed, M, lq_x, nullptr, w_x};
  s.lq = {lq_n, lq_c, w_n, w_c};
  return sym_forward(ctx, s, kTermCells);
}

}  // extern "C"
