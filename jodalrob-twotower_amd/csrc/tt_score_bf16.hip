// bf16-MFMA fast path of the in-batch-negative score + symmetric softmax-CE (same maths as
// tt_score.hip, operands rounded to bf16, f32 accumulation on v_mfma_f32_32x32x16_bf16).
//
// Wave-level design (no LDS in the main loops):
//   * a wave owns 32*AT rows `a` of A and sweeps the rows `b` of Bm in 32-row tiles; the NW waves of a
//     workgroup share the same A rows and split the b tiles round-robin.
//   * the tile is computed TRANSPOSED, X = Bm_tile . A_tile^T, so an accumulator register holds
//     X[b = rowmap(reg, lane>>5)][a = lane&31]: every per-`a` quantity (1/sumexp_a, the diagonal score,
//     the running exp-sum and rank count) is ONE value per lane, and the accumulator registers of a tile,
//     converted pairwise to bf16, ARE the A operand of the second MFMA (X^T . Bm) -- no lane movement.
//   * Bm is read in two images written once per step by tt_score_pack_bf16, both in MFMA fragment order so
//     that every wave-instruction reads 1 KB contiguous (a row-major image made each load touch 32 cache
//     lines and left the kernels bound by L1 tag throughput): [tile][k-step][half][row][8] for the operands
//     of the first product, and [tile][k-step][half][d][8] whose 16-B chunks are exactly the B operand of
//     the second product in the k-permutation the accumulator registers impose.
//   * partial results of the NW waves are combined through LDS in a fixed tree order.
#include "tt_score_bwd_bsplit.h"
// measurement aid, compiled in with -DTT_POST_STAMPS only (tools/post_sweep_stamps.py): what the hosted score backward's workgroups
// do behind their sweep -- device-clock stamps of thread 0: 0 start, 1 end of its sweep, 2 the head's loads issued, 3 / 4 behind
// the reduction's two barriers, 5 the flat sums added and dA stored, 6 behind the barrier in front of the head, 8 + i behind
// barrier i of the head (tt_tail_bwd.h), 14 its end.  Written with plain vector stores, compiled out of the product.
#ifdef TT_POST_STAMPS
__device__ unsigned long long g_post_stamps[512 * 16];
#define TT_POST_STAMP(i) do { if (threadIdx.x == 0) g_post_stamps[((blockIdx.y * gridDim.x + blockIdx.x) & 511) * 16 + (i)] = __builtin_amdgcn_s_memrealtime(); } while (0)
#define TT_HEAD_STAMP(i) TT_POST_STAMP(8 + (i))
#else
#define TT_POST_STAMP(i) do { } while (0)
#endif
#include "tt_tail_bwd.h"
#include "tt_deferred.h"

#include <stdlib.h>

namespace {

template <int KS, int AT>
__device__ __forceinline__ void gemm1(const __bf16* __restrict__ b_rows, int64_t t, int c, int h, const bf16x8 (&ares)[AT][KS],
                                      f32x16 (&acc)[AT]) {
  bf16x8 bf[KS];
  load_bfrag<KS>(b_rows, t, c, h, bf);
  mfma1<KS, AT>(bf, ares, acc);
}

// ---- forward ---------------------------------------------------------------------------------------
// UNIT: every direction's exponent scale is exactly 1 (one operand image was packed times inv_t * log2 e): the softmax
// term is exp2(acc) with no multiply-add in front -- one VALU op less per score in kernels that are bound by VALU issue --
// and the constant factor 2^c2 of the fixed shift goes onto the finished row sums (|acc| <= log2(e) / T <= 58 for the
// supported temperatures: no overflow without the shift).  Rank / diagonal comparisons are scale-free.
// X3: bf16x3 operands (mfma_s); the lo images are read beside the hi ones, everything after the S tile is unchanged.
template <int KS, int AT, int NW, bool UNIT, bool X3 = false>
__global__ __launch_bounds__(NW * 64) void score_fwd_bf16_kernel(FwdArgs args) {
  constexpr int ROWS = 32 * AT, KL = X3 ? KS : 1;
  __shared__ float part_e[NW][ROWS];
  __shared__ float part_s[NW][ROWS];
  __shared__ int part_c[NW][ROWS];
  const FwdSel dr = select_dir(args, blockIdx.y != 0);
  const float c1 = dr.c1, unscale = dr.unscale, c2 = args.c2;
  float* const inv_out = dr.inv_sumexp;
  auto ex = [&](float x) { return UNIT ? __builtin_amdgcn_exp2f(x) : __builtin_amdgcn_exp2f(__builtin_fmaf(x, c1, c2)); };
  const int Ra = dr.Ra, Rb = dr.Rb, off = dr.off;
  const int a0 = (int)blockIdx.x * ROWS;
  if (a0 >= Ra) return;
  const int lane = threadIdx.x & 63, c = lane & 31, h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nT = (Rb + 31) / 32;
  bf16x8 ares[AT][KS], ares_lo[AT][KL];
#pragma unroll
  for (int i = 0; i < AT; ++i) {
    load_bfrag<KS>(dr.a_rows, a0 / 32 + i, c, h, ares[i]);
    if (X3) load_bfrag<KL>(dr.a_lo, a0 / 32 + i, c, h, ares_lo[i]);
  }
  int pos[AT];
  float dg[AT];
#pragma unroll
  for (int i = 0; i < AT; ++i) { pos[i] = a0 + 32 * i + c + off; dg[i] = kNegBig; }
  const int posmin = a0 + off, posmax = a0 + ROWS - 1 + off;
  // the diagonal scores, taken from the MFMA result itself so that ties compare bit-for-bit
  if (posmax >= 0 && posmin < Rb) {
    const int td0 = posmin > 0 ? posmin / 32 : 0;
    const int td1 = (posmax / 32) < nT - 1 ? posmax / 32 : nT - 1;
    for (int t = td0; t <= td1; ++t) {
      f32x16 acc[AT];
      bf16x8 bh[KS], bl[KL];
      load_bfrag<KS>(dr.b_rows, t, c, h, bh);
      if (X3) load_bfrag<KL>(dr.b_lo, t, c, h, bl);
      mfma_s<KS, AT, X3>(bh, bl, ares, ares_lo, acc);
#pragma unroll
      for (int i = 0; i < AT; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (32 * t + rowmap(r, h) == pos[i]) dg[i] = acc[i][r];
    }
#pragma unroll
    for (int i = 0; i < AT; ++i) dg[i] = fmaxf(dg[i], __shfl_xor(dg[i], 32));
  }
  // per-lane accumulators of this wave's share of the b tiles
  float se[AT], ss[AT], mb[AT], ma[AT];      // exp-sum, score-sum, max before / after the positive (top-1 mode)
  int cnt[AT];                                // full-rank mode
#pragma unroll
  for (int i = 0; i < AT; ++i) { se[i] = 0.f; ss[i] = 0.f; cnt[i] = 0; mb[i] = kNegBig; ma[i] = kNegBig; }
  const int mode = dr.rank ? dr.rank_mode : 0;                 // wave-uniform
  const bool want_ss = dr.sumscore != nullptr;
  // (a two-accumulator variant that issues tile t+NW's MFMAs before the epilogue of tile t measured SLOWER:
  //  199 VGPRs, 72-78 us vs 63-65 us -- kept single-buffered)
  // tile classes by index alone (two scalar compares per tile; deriving them from row positions cost ~30 SALU instructions
  // per tile): t < t_before: full tiles entirely before the workgroup's positives; t_after <= t < n_full: entirely after
  const int n_full = Rb / 32;
  const int t_before = min(posmin > 0 ? posmin / 32 : 0, n_full);
  const int t_after = posmax >= 0 ? posmax / 32 + 1 : 0;
  auto epilogue = [&](const f32x16 (&acc)[AT], int t) {
    const int b_lo = 32 * t;
    const bool before = t < t_before, after = t >= t_after && t < n_full;
    const bool full_tile = t < n_full;
    if (before || after) {
#pragma unroll
      for (int i = 0; i < AT; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) se[i] += ex(acc[i][r]);
      if (want_ss) {
#pragma unroll
        for (int i = 0; i < AT; ++i)
#pragma unroll
          for (int r = 0; r < 16; ++r) ss[i] += acc[i][r];
      }
      if (mode == 1) {            // top-1 only: running maxima, one v_max3 per two elements
        if (before) {
#pragma unroll
          for (int i = 0; i < AT; ++i)
#pragma unroll
            for (int r = 0; r < 16; r += 2) mb[i] = max3_asm(mb[i], acc[i][r], acc[i][r + 1]);
        } else {
#pragma unroll
          for (int i = 0; i < AT; ++i)
#pragma unroll
            for (int r = 0; r < 16; r += 2) ma[i] = max3_asm(ma[i], acc[i][r], acc[i][r + 1]);
        }
      } else if (mode == 2) {     // full rank: ties before the positive count, after it they do not
        if (before) {
#pragma unroll
          for (int i = 0; i < AT; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) cnt[i] += acc[i][r] >= dg[i] ? 1 : 0;
        } else {
#pragma unroll
          for (int i = 0; i < AT; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) cnt[i] += acc[i][r] > dg[i] ? 1 : 0;
        }
      }
    } else if (full_tile) {       // the tile(s) holding the positives: every b is a row, only before / after is per lane.
      // Selects, no per-element branches: one wave of every workgroup meets this tile, and the general form below (exec-mask
      // branches around every element, ~600 VALU instructions against 56 for a plain tile) made that wave the straggler.
#pragma unroll
      for (int i = 0; i < AT; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) se[i] += ex(acc[i][r]);
      if (want_ss) {
#pragma unroll
        for (int i = 0; i < AT; ++i)
#pragma unroll
          for (int r = 0; r < 16; ++r) ss[i] += acc[i][r];
      }
#pragma unroll
      for (int i = 0; i < AT; ++i) {
        const int q = pos[i] - b_lo - 4 * h;              // b < pos  <=>  (r & 3) + 8 * (r >> 2) < q
        if (mode == 1) {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int k = (r & 3) + 8 * (r >> 2);
            const float x = acc[i][r];
            mb[i] = fmaxf(mb[i], k < q ? x : kNegBig);
            ma[i] = fmaxf(ma[i], k > q ? x : kNegBig);
          }
        } else if (mode == 2) {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int k = (r & 3) + 8 * (r >> 2);
            const float x = acc[i][r];
            cnt[i] += ((k < q && x >= dg[i]) || (k > q && x > dg[i])) ? 1 : 0;
          }
        }
      }
    } else {                      // the ragged last tile (Rb not a multiple of 32): per-element care
#pragma unroll
      for (int i = 0; i < AT; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int b = b_lo + rowmap(r, h);
          const float x = acc[i][r];
          const bool valid = b < Rb, bef = valid && b < pos[i], aft = valid && b > pos[i];
          se[i] += valid ? ex(x) : 0.f;
          ss[i] += valid ? x : 0.f;
          mb[i] = bef ? fmaxf(mb[i], x) : mb[i];
          ma[i] = aft ? fmaxf(ma[i], x) : ma[i];
          cnt[i] += ((bef && x >= dg[i]) || (aft && x > dg[i])) ? 1 : 0;
        }
    }
  };
  // operand prefetch PFD tiles ahead (a ring of register buffers, the loop unrolled over it so no buffer is copied): a tile
  // is ~150 ns of work for a wave, an L2 hit several times that -- one tile of lookahead left the waves waiting on loads
  // (X3: twice the operand registers per tile -- one tile less of lookahead)
  constexpr int PFD = X3 ? (KS <= 4 ? 2 : 1) : (KS <= 4 ? 3 : (KS <= 8 ? 2 : 1));
  bf16x8 bq[PFD][KS], bql[PFD][KL];
#pragma unroll
  for (int p = 0; p < PFD; ++p)
    if (wave + p * NW < nT) {
      load_bfrag<KS>(dr.b_rows, wave + p * NW, c, h, bq[p]);
      if (X3) load_bfrag<KL>(dr.b_lo, wave + p * NW, c, h, bql[p]);
    }
  for (int t0 = wave; t0 < nT; t0 += PFD * NW) {
#pragma unroll
    for (int p = 0; p < PFD; ++p) {
      const int t = t0 + p * NW;
      if (t < nT) {                                                         // wave-uniform
        f32x16 acc[AT];
        mfma_s<KS, AT, X3>(bq[p], bql[p], ares, ares_lo, acc);
        if (t + PFD * NW < nT) {                                            // refill behind the MFMAs that read it
          load_bfrag<KS>(dr.b_rows, t + PFD * NW, c, h, bq[p]);
          if (X3) load_bfrag<KL>(dr.b_lo, t + PFD * NW, c, h, bql[p]);
        }
        epilogue(acc, t);
      }
    }
  }
  __shared__ float part_mb[NW][ROWS], part_ma[NW][ROWS];
#pragma unroll
  for (int i = 0; i < AT; ++i) {
    se[i] += __shfl_xor(se[i], 32);
    ss[i] += __shfl_xor(ss[i], 32);
    cnt[i] += __shfl_xor(cnt[i], 32);
    mb[i] = fmaxf(mb[i], __shfl_xor(mb[i], 32));
    ma[i] = fmaxf(ma[i], __shfl_xor(ma[i], 32));
    if (h == 0) {
      part_e[wave][32 * i + c] = se[i]; part_s[wave][32 * i + c] = ss[i]; part_c[wave][32 * i + c] = cnt[i];
      part_mb[wave][32 * i + c] = mb[i]; part_ma[wave][32 * i + c] = ma[i];
    }
  }
  __shared__ float dg_s[ROWS];
  if (wave == 0 && h == 0) {
#pragma unroll
    for (int i = 0; i < AT; ++i) dg_s[32 * i + c] = dg[i];
  }
  __syncthreads();
  if (threadIdx.x < ROWS) {
    const int a = a0 + threadIdx.x;
    if (a < Ra) {
      float e = 0.f, sc = 0.f, xb = kNegBig, xa = kNegBig;
      int k = 0;
#pragma unroll
      for (int w = 0; w < NW; ++w) {
        e += part_e[w][threadIdx.x]; sc += part_s[w][threadIdx.x]; k += part_c[w][threadIdx.x];
        xb = fmaxf(xb, part_mb[w][threadIdx.x]); xa = fmaxf(xa, part_ma[w][threadIdx.x]);
      }
      dr.sumexp[a] = UNIT ? e * args.kexp : e;
      if (inv_out) inv_out[a] = 1.f / e;
      if (mode == 2) dr.rank[a] = k;
      else if (mode == 1) dr.rank[a] = (xb < dg_s[threadIdx.x] && xa <= dg_s[threadIdx.x]) ? 0 : 1;
      if (dr.sumscore) dr.sumscore[a] = sc * unscale;                            // products -> sum_b s_ab / T
    }
  }
  if (wave == 0 && h == 0 && dr.diag) {
#pragma unroll
    for (int i = 0; i < AT; ++i) {
      const int a = a0 + 32 * i + c;
      if (a < Ra) dr.diag[a] = dg[i] > -1.0e38f ? dg[i] * unscale : 0.f;
    }
  }
}

// ---- backward, b-split form with ONE streamed image (D <= 64) ---------------------------------------------------------
// Ablations of the kernel above (compile-time, tools/bench_score.py, B = 8192, D = 64): full 50.0 us; without the exp2 45.9;
// without the gradient MFMAs 35.7; without ANY MFMA or exp2 32.4 -- two thirds of the time is moving the opposite side's
// operands: each workgroup streams 2 MB (the rows image for S AND the fragment-ordered image of the same values for the
// gradient product) at the ~65 GB/s a CU draws from L2.  Here only the rows image is streamed: a wave parks the tile's row
// fragments (it has them in registers for the S product) in a wave-private LDS tile [32 b][64 d] and reads the gradient
// product's operand -- 8 b-values of one column d per lane, in the accumulator's row order -- back with the transposing
// LDS read ds_read_b64_tr_b16 (a 16-lane group reads a 4-row x 16-column block, lane i gets column i).  Half the L2
// bytes for 8 KB of LDS traffic per tile.  Same values, same order of operations: bit-identical.
// Result: 45.9 -> 44.4 us in the step.  The same ablations on this kernel: full 49.1; no exp2 44.9; no gradient MFMAs 30.8;
// nothing 23.4 -- streaming is no longer the largest term; per SIMD the gradient + S MFMAs (34 GFLOP for both directions: every
// direction recomputes S) need ~20 us of the matrix pipe, the softmax VALU work ~24 us, the loads ~20 us, and a wave runs the
// three one after the other.
// LQ: as score_bwd_bf16_kernel's.
// TAIL (KS = 4, AT = 2, no LQ; TT_OPT_FUSE_SCORE_TAIL, launched by tt_towers_mlp_bwd): the workgroup goes on with the towers' backward head (tt_tail_bwd.h) of
// tower blockIdx.y, row chunk blockIdx.x -- the 64 rows of d_emb this workgroup sums.  The head's loads that depend on nothing the
// sweep produces are issued in front of the reduction (ares and the streamed tiles are dead there).  Where the other forms run the
// tree's second and third rounds and let wave 0 store dA, the reduction here is FLAT behind round one: waves
// 0 .. 3 put their sums back into the four slabs, one barrier, and thread (wave w, lane d) of all eight waves adds rows 8 w .. 8 w + 7
// of column d as (s0 + s2) + (s1 + s3) -- the tree's own association ((w0 + w4) + (w2 + w6)) + ((w1 + w5) + (w3 + w7)), bit for bit --,
// stores them to dA and keeps them: that is the thread that normalises those rows in the head.  The head's LDS lies over `red`
// (one more barrier: every wave has read the slabs).  The sweep is the same code.
// (one __global__ template for both: the sweep must compile exactly as it does without a tail)
template <bool TAIL>
struct TailHost {};
template <>
struct TailHost<true> { tttail::Batch<tttail::TailBwdArgs> batch; bool drop; float p; uint64_t seed0; const uint64_t* seed_dev; };

template <int KS, int AT, bool UNIT, bool LQ = false, bool TAIL = false>
__global__ __launch_bounds__(512) void score_bwd_tr_kernel(BwdArgs args, TailHost<TAIL> th) {
  constexpr int NW = 8, Dp = KS * 16, ROWS = 32 * AT, DT = KS / 2;
  constexpr int TLD = Dp + 8;                                   // LDS row of the parked tile: 144 B at D = 64 (conflict-free b128 writes)
  constexpr int kRedB = (NW / 2) * ROWS * Dp * 4, kParkB = NW * 32 * TLD * 2;
  static_assert(!TAIL || (KS == 4 && AT == 2 && !LQ && tttail::kTailBwdLds <= kRedB + kParkB),
                "the tail's head lies over red | park of the <4, 2> form");
  __shared__ float red_s[TAIL ? 1 : (NW / 2) * ROWS * Dp];
  __shared__ __attribute__((aligned(16))) __bf16 park_s[TAIL ? 1 : NW][32 * TLD];
  __shared__ __attribute__((aligned(16))) char smem[TAIL ? kRedB + kParkB : 16];       // TAIL: red | park as ONE buffer
  float* const red = TAIL ? reinterpret_cast<float*>(smem) : red_s;
  __bf16 (*const park)[32 * TLD] = TAIL ? reinterpret_cast<__bf16 (*)[32 * TLD]>(smem + kRedB) : park_s;
  using s16x4 = __attribute__((ext_vector_type(4))) short;
  using s16x8 = __attribute__((ext_vector_type(8))) short;
  const BwdSel dr = select_dir(args, blockIdx.y != 0);
  const float c1 = dr.c1, c2 = args.c2, kx = UNIT ? args.kexp : 1.f;
  const int Ra = dr.Ra, Rb = dr.Rb, off = dr.off;
  const float* const wt_b = dr.wt_b;
  const int a0 = (int)blockIdx.x * ROWS;
  if (a0 >= Ra) return;
  if constexpr (TAIL) TT_POST_STAMP(0);
  const int lane = threadIdx.x & 63, c = lane & 31, h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nT = (Rb + 31) / 32;
  bf16x8 ares[AT][KS];
  float ia[AT], ua[AT];
  int pos[AT];
#pragma unroll
  for (int i = 0; i < AT; ++i) {
    load_bfrag<KS>(dr.a_rows, a0 / 32 + i, c, h, ares[i]);
    a_row_setup<LQ>(dr, kx, a0 + 32 * i + c, ia[i], ua[i], pos[i]);
  }
  const int posmin = a0 + off, posmax = a0 + ROWS - 1 + off;
  f32x16 dacc[AT][DT];
  zero_acc(dacc);
  const bool have_inv = dr.inv_b != nullptr;
  const float* const ivsrc = have_inv ? dr.inv_b : dr.sumexp_b;
  const int tlast = nT - 1;
  __bf16* const tile = park[wave];
  // parked-tile addresses: write = row c, columns 16 s + 8 h; transposing read = block row q of this lane's 16-lane group,
  // columns 4 p of the group's 16 (lane 4 q + p supplies the address, lane i of the group receives column i)
  __bf16* const wr_at = tile + c * TLD + 8 * h;
  const int g16 = lane & 15, cg = (lane >> 4) & 1;
  const __bf16* const tr_at = tile + (4 * h + (g16 >> 2)) * TLD + 16 * cg + 4 * (g16 & 3);
  // LQ, D = 128: the weights are loaded behind the tile's S product, not a tile ahead (two tiles' 32 more registers spilled)
  constexpr bool WLATE = LQ && KS >= 8;
  struct Tile { bf16x8 b[KS]; float4 iv[4]; float4 wv[LQ ? 4 : 1]; };
  auto load = [&](Tile& T, int t) {
    load_bfrag<KS>(dr.b_rows, t, c, h, T.b);
#pragma unroll
    for (int q = 0; q < 4; ++q) T.iv[q] = *reinterpret_cast<const float4*>(ivsrc + 32 * t + 4 * h + 8 * q);
    if constexpr (LQ && !WLATE) {
#pragma unroll
      for (int q = 0; q < 4; ++q) T.wv[q] = *reinterpret_cast<const float4*>(wt_b + 32 * t + 4 * h + 8 * q);
    }
  };
  auto compute = [&](const Tile& T, int t) {
    const int b_lo = 32 * t;
#pragma unroll
    for (int s2 = 0; s2 < KS; ++s2) *reinterpret_cast<bf16x8*>(wr_at + 16 * s2) = T.b[s2];
    float ib[16], wb[16];
#pragma unroll
    for (int q = 0; q < 4; ++q) { ib[4 * q] = T.iv[q].x; ib[4 * q + 1] = T.iv[q].y; ib[4 * q + 2] = T.iv[q].z; ib[4 * q + 3] = T.iv[q].w; }
    if constexpr (LQ && !WLATE) {
#pragma unroll
      for (int q = 0; q < 4; ++q) { wb[4 * q] = T.wv[q].x; wb[4 * q + 1] = T.wv[q].y; wb[4 * q + 2] = T.wv[q].z; wb[4 * q + 3] = T.wv[q].w; }
    }
    if (!have_inv) {
#pragma unroll
      for (int r = 0; r < 16; ++r) ib[r] = __builtin_amdgcn_rcpf(ib[r]) * kx;
    }
    if (b_lo + 31 >= Rb) {
#pragma unroll
      for (int r = 0; r < 16; ++r) ib[r] = b_lo + rowmap(r, h) < Rb ? ib[r] : 0.f;
    }
    const bool band = !(b_lo + 31 < posmin || b_lo > posmax);
    // the gradient product's operand: for k-step s2 and column block d, rows {16 s2 + 4 h + 0..3, 16 s2 + 8 + 4 h + 0..3}
    bf16x8 bm[2][DT];
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
      for (int d = 0; d < DT; ++d) {
        const s16x4 lo4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            (__attribute__((address_space(3))) s16x4*)(tr_at + (16 * s2) * TLD + 32 * d));
        const s16x4 hi4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            (__attribute__((address_space(3))) s16x4*)(tr_at + (16 * s2 + 8) * TLD + 32 * d));
        const s16x8 v{lo4[0], lo4[1], lo4[2], lo4[3], hi4[0], hi4[1], hi4[2], hi4[3]};
        bm[s2][d] = __builtin_bit_cast(bf16x8, v);
      }
#pragma unroll
    for (int i = 0; i < AT; ++i) {
      f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
      for (int s2 = 0; s2 < KS; ++s2) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(T.b[s2], ares[i][s2], acc, 0, 0, 0);
      if constexpr (WLATE) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float4 v = *reinterpret_cast<const float4*>(wt_b + b_lo + 4 * h + 8 * q);
          wb[4 * q] = v.x; wb[4 * q + 1] = v.y; wb[4 * q + 2] = v.z; wb[4 * q + 3] = v.w;
        }
      }
      float w[16];
#pragma unroll
      for (int r = 0; r < 16; ++r)
        w[r] = softmax_term<UNIT, LQ>(acc[r], c1, c2, ia[i], ua[i], ib[r], wb[r]);
      if (b_lo + 31 >= Rb) {
#pragma unroll
        for (int r = 0; r < 16; ++r) w[r] = b_lo + rowmap(r, h) < Rb ? w[r] : 0.f;
      }
      if (band) {
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (b_lo + rowmap(r, h) == pos[i]) w[r] -= 2.f;
      }
      bf16x8 wf[2];
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
        for (int j = 0; j < 8; ++j) wf[s2][j] = (__bf16)w[8 * s2 + j];
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
        for (int d = 0; d < DT; ++d) dacc[i][d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[s2], bm[s2][d], dacc[i][d], 0, 0, 0);
    }
  };
  Tile T0, T1;                                                 // (why the sweep has this shape: score_bwd_bf16_kernel's comment)
  load(T0, min(wave, tlast));
  __builtin_amdgcn_sched_barrier(0);
  for (int t = wave; t < nT; t += 2 * NW) {
    load(T1, min(t + NW, tlast));
    compute(T0, t);
    load(T0, min(t + 2 * NW, tlast));
    if (t + NW < nT) compute(T1, t + NW);
  }
  [[maybe_unused]] tttail::TailBwdConst<512> hk;
  [[maybe_unused]] tttail::TailBwdRows<512> hv;
  [[maybe_unused]] uint64_t hseed = 0;
  if constexpr (TAIL) {
    TT_POST_STAMP(1);
    const tttail::TailBwdArgs& f = th.batch.a[blockIdx.y];
    tttail::tail_bwd_load_const<512>(f, hk);
    tttail::tail_bwd_load_rows<512, true>(f, min(f.col.B, a0 + 64), a0, hv);
    if (th.drop) hseed = tttail::seed_of(th.seed0, th.seed_dev);
    TT_POST_STAMP(2);
  }
  if constexpr (TAIL) {
    if (wave >= NW / 2) {                                        // round one of the tree
      float* slab = red + (wave - NW / 2) * ROWS * Dp;
#pragma unroll
      for (int i = 0; i < AT; ++i)
#pragma unroll
        for (int d = 0; d < DT; ++d)
#pragma unroll
          for (int r = 0; r < 16; ++r) slab[(32 * i + rowmap(r, h)) * Dp + 32 * d + c] = dacc[i][d][r];
    }
    __syncthreads();
    TT_POST_STAMP(3);
    if (wave < NW / 2) {                                         // (a lane writes the addresses it has read: no barrier between)
      float* slab = red + wave * ROWS * Dp;
#pragma unroll
      for (int i = 0; i < AT; ++i)
#pragma unroll
        for (int d = 0; d < DT; ++d)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            float* at = slab + (32 * i + rowmap(r, h)) * Dp + 32 * d + c;
            *at = dacc[i][d][r] + *at;
          }
    }
    __syncthreads();
    TT_POST_STAMP(4);
    const tttail::TailBwdArgs& f = th.batch.a[blockIdx.y];
    const float g = args.d_loss[0] * dr.out_scale;
    constexpr int R = tttail::TailBwdRows<512>::R;
    static_assert(R * NW == ROWS && Dp == 64, "thread (wave, lane): rows wave R .. wave R + R - 1 of column lane");
#pragma unroll
    for (int j = 0; j < R; ++j) {
      const float* at = red + (wave * R + j) * Dp + lane;
      const float s0 = at[0], s1 = at[ROWS * Dp], s2 = at[2 * ROWS * Dp], s3 = at[3 * ROWS * Dp];
      const float v = ((s0 + s2) + (s1 + s3)) * g;
      const int a = a0 + wave * R + j;
      if (a < Ra && lane < args.D) dr.dA[(int64_t)a * args.D + lane] = v;
      hv.de[j] = (a < f.col.B && lane < f.D) ? v : 0.f;
    }
    TT_POST_STAMP(5);
    __syncthreads();                                             // the slabs are read: the head's LDS lies over them
    TT_POST_STAMP(6);
    tttail::tail_bwd_head<512, true>(f, blockIdx.x, th.drop, th.p, hseed, smem, &hk, &hv);
  } else {
#pragma unroll
    for (int half = NW / 2; half >= 1; half >>= 1) {
      if (wave >= half && wave < 2 * half) {
        float* slab = red + (wave - half) * ROWS * Dp;
#pragma unroll
        for (int i = 0; i < AT; ++i)
#pragma unroll
          for (int d = 0; d < DT; ++d)
#pragma unroll
            for (int r = 0; r < 16; ++r) slab[(32 * i + rowmap(r, h)) * Dp + 32 * d + c] = dacc[i][d][r];
      }
      __syncthreads();
      if (wave < half) {
        const float* slab = red + wave * ROWS * Dp;
#pragma unroll
        for (int i = 0; i < AT; ++i)
#pragma unroll
          for (int d = 0; d < DT; ++d)
#pragma unroll
            for (int r = 0; r < 16; ++r) dacc[i][d][r] += slab[(32 * i + rowmap(r, h)) * Dp + 32 * d + c];
      }
      __syncthreads();
    }
    if (wave == 0) {
      const float g = args.d_loss[0] * dr.out_scale;
#pragma unroll
      for (int i = 0; i < AT; ++i)
#pragma unroll
        for (int d = 0; d < DT; ++d)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int a = a0 + 32 * i + rowmap(r, h);
            const int dd = 32 * d + c;
            if (a < Ra && dd < args.D) dr.dA[(int64_t)a * args.D + dd] = dacc[i][d][r] * g;
          }
    }
  }
}

// ---- backward, large-batch form ---------------------------------------------------------------------
// When there are enough rows a for every SIMD to own its own (Ra / 64 x directions >= ~1024), nothing has to be split along b:
// a workgroup is 4 waves, ONE per SIMD with the whole 512-register file (amdgpu_waves_per_eu(1, 1)), each wave owns two
// 32-row tiles of a -- A fragments (2 x KS) and the dA accumulators (2 x Dp / 32 tiles of 16 registers: 256 at D = 256) stay
// in registers for the whole sweep -- and ALL four waves stream the same b tiles, staged ONCE per workgroup through LDS
// (rows image + fragment image + the 32 reciprocals of a tile: 32 KB at D = 256, double buffered).  The b-split form above
// reads those 32 KB once per WAVE: 268 GB of L2 traffic at B = 65536, D = 256, which is what bounded it (15 TB/s at 23 %
// MFMA busy); here it is 34 GB.  No cross-wave reduction at the end: a wave's rows are its own.
// Inside a wave the two a tiles give the matrix pipe independent work while the VALU forms the softmax weights: S(0) S(1)
// | E(0) beside S(1) | dA(0) | E(1) beside dA(0) | dA(1).
// FP8: the S products take fp8 operands (rows images in the layout of tt_score_bf16.h, K = 64 per MFMA at twice the bf16 rate,
// half the A-fragment registers and half the staged bytes); the second products stay bf16.
// AT = 2, NWV = 4: one wave per SIMD with the whole register file; AT = 1, NWV = 8: two waves per SIMD (256 registers each:
// the hardware then runs one wave's softmax weights beside the other's MFMAs).
// LQ: as score_bwd_bf16_kernel's; the tile's 32 sampling weights ride in the stage behind its 32 reciprocals (the stage's
// 256-byte per-row slot held 128 bytes).
// (Its own copy of select_dir, a_row_setup, zero_acc and the fp8 fragment read: with them the non-unit D = 128 instantiations read the
// stage in more, smaller LDS reads and wait four or five times more per tile -- profiles/NOTES.md, "score backward parts".)
template <int KS, bool UNIT, bool FP8, int AT, int NWV, bool LQ = false>
__global__ __launch_bounds__(NWV * 64) void score_bwd_rows_kernel(BwdArgs args) {
  constexpr int NTH = NWV * 64, DT = KS / 2, Dp = KS * 16, K64 = FP8 ? KS / 4 : 1;
  constexpr int kRowsB = FP8 ? KS * 512 : KS * 1024, kFragB = KS * 1024, kIvB = 256, kStageB = kRowsB + kFragB + kIvB;
  constexpr int kPieces = (kRowsB + kFragB) / 16, kPPT = (kPieces + NTH - 1) / NTH;   // 16-byte pieces per thread per stage (last one ragged)
  static_assert(!FP8 || KS % 4 == 0, "fp8 operands come in K = 64 steps");
  // bf16 operands at D = 256: the wave's own A fragments are 64 registers beside 128 of accumulators -- they live in LDS behind
  // the two stages ([wave][k-step][lane] 16-byte pieces: 8 KB per wave) and are read back four k-steps at a time
  constexpr bool ALDS = !FP8 && KS == 16;
  extern __shared__ __attribute__((aligned(16))) char lds_raw[];
  const bool d1 = blockIdx.y != 0;
  DirBwd dr;
  dr.a_rows = d1 ? args.d[1].a_rows : args.d[0].a_rows;
  dr.b_rows = d1 ? args.d[1].b_rows : args.d[0].b_rows;
  dr.b_frag = d1 ? args.d[1].b_frag : args.d[0].b_frag;
  dr.sumexp_a = d1 ? args.d[1].sumexp_a : args.d[0].sumexp_a;
  dr.sumexp_b = d1 ? args.d[1].sumexp_b : args.d[0].sumexp_b;
  dr.dA = d1 ? args.d[1].dA : args.d[0].dA;
  const float c1 = d1 ? args.d[1].c1 : args.d[0].c1, out_scale = d1 ? args.d[1].out_scale : args.d[0].out_scale;
  const float* const inv_a = d1 ? args.d[1].inv_a : args.d[0].inv_a;
  const float* const inv_b = d1 ? args.d[1].inv_b : args.d[0].inv_b;
  const float* const wt_a = d1 ? args.wt_a[1] : args.wt_a[0];     // (LQ)
  const float* const wt_b = d1 ? args.wt_b[1] : args.wt_b[0];
  const float c2 = args.c2, kx = UNIT ? args.kexp : 1.f;
  const int Ra = (int)(d1 ? args.d[1].Ra : args.d[0].Ra), Rb = (int)(d1 ? args.d[1].Rb : args.d[0].Rb);
  const int off = (int)(d1 ? args.d[1].off : args.d[0].off);
  const int tid = threadIdx.x, lane = tid & 63, c = lane & 31, h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nT = (Rb + 31) / 32, nTa_img = (int)(rup(Ra, 64) / 32);
  const int at0 = ((int)blockIdx.x * NWV + wave) * AT;                      // this wave's first a tile
  if ((int)blockIdx.x * NWV * AT * 32 >= Ra) return;                        // (whole workgroup)
  bf16x8 ares[AT][(FP8 || ALDS) ? 1 : KS];
  i32x8 ares8[AT][K64];
  bf16x8* const a_lds = reinterpret_cast<bf16x8*>(lds_raw + 2 * kStageB) + (size_t)wave * AT * KS * 64 + lane;   // (ALDS) [a tile][k-step][lane]
  float ia[AT], ua[AT];
  int pos[AT];
#pragma unroll
  for (int i = 0; i < AT; ++i) {
    if (FP8) load_f8frag<K64>(reinterpret_cast<const char*>(dr.a_rows), min(at0 + i, nTa_img - 1), c, h, ares8[i]);
    else if (ALDS) {
      const __bf16* pa = dr.a_rows + (((int64_t)min(at0 + i, nTa_img - 1) * KS * 2 + h) * 32 + c) * 8;
#pragma unroll
      for (int s2 = 0; s2 < KS; ++s2) a_lds[(i * KS + s2) * 64] = *reinterpret_cast<const bf16x8*>(pa + s2 * 512);    // (wave-private: no barrier)
    } else load_bfrag<((FP8 || ALDS) ? 1 : KS)>(dr.a_rows, min(at0 + i, nTa_img - 1), c, h, ares[i]);
    const int a = 32 * (at0 + i) + c;
    ia[i] = a < Ra ? (inv_a ? inv_a[a] : __builtin_amdgcn_rcpf(dr.sumexp_a[a]) * kx) : 0.f;
    if constexpr (LQ) ua[i] = a < Ra ? wt_a[a] : 0.f;
    pos[i] = a + off;
  }
  const int posmin = 32 * at0 + off, posmax = 32 * (at0 + AT) - 1 + off;
  f32x16 dacc[AT][DT];
#pragma unroll
  for (int i = 0; i < AT; ++i)
#pragma unroll
    for (int d = 0; d < DT; ++d)
#pragma unroll
      for (int r = 0; r < 16; ++r) dacc[i][d][r] = 0.f;
  const bool have_inv = inv_b != nullptr;
  const float* const ivsrc = have_inv ? inv_b : dr.sumexp_b;
  // stage loader: the tile's [rows image | fragment image | 32 reciprocals] (contiguous per tile in global memory) go STRAIGHT into
  // the LDS stage by LDS-DMA (global_load_lds_dwordx4: lane l of a wave writes 16 bytes at the wave's base + 16 l), piece
  // p = tid + NTH q at offset 16 p.  Round 3: the copy used to pass through registers (up to eight 16-byte pieces per thread,
  // loaded a tile ahead and stored before the barrier): at D = 256 those 16-20 registers were the difference between 256
  // registers and 8-36 dwords of scratch per lane in the tile loop.  The DMA of tile t + 1 is issued right behind the barrier that
  // frees its buffer and has the whole tile to land; a wave waits for its own pieces (vmcnt(0)) before the next barrier.
  const char* const g_rows = reinterpret_cast<const char*>(dr.b_rows);
  const char* const g_frag = reinterpret_cast<const char*>(dr.b_frag);
  auto stage_dma = [&](int tn, int buf) {
    char* const base = lds_raw + buf * kStageB;
#pragma unroll
    for (int q = 0; q < kPPT; ++q) {
      const int p = tid + NTH * q;
      if ((q + 1) * NTH <= kPieces || p < kPieces) {
        const char* src = p < kRowsB / 16 ? g_rows + (int64_t)tn * kRowsB + p * 16 : g_frag + (int64_t)tn * kFragB + (p - kRowsB / 16) * 16;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                         (__attribute__((address_space(3))) void*)(base + (wave * 64 + NTH * q) * 16), 16, 0, 0);
      }
    }
    if (wave == 0 && lane < (LQ ? 16 : 8))
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(LQ && lane >= 8 ? wt_b + 32 * tn + 4 * (lane - 8)
                                                                                                    : ivsrc + 32 * tn + 4 * lane),
                                       (__attribute__((address_space(3))) void*)(base + kRowsB + kFragB), 16, 0, 0);
  };
  stage_dma(0, 0);
  for (int t = 0; t < nT; ++t) {
    const int nb = (t + 1) & 1;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // this wave's pieces of tile t have landed ...
    __syncthreads();                                       // ... and everybody's; buffer nb is no longer read by anyone
    if (t + 1 < nT) stage_dma(t + 1, nb);
    const char* rb = lds_raw + (t & 1) * kStageB;
    const char* fb = rb + kRowsB;
    const float* ivp = reinterpret_cast<const float*>(fb + kFragB);
    const int b_lo = 32 * t;
    // S tiles of both a tiles: the b fragments are read once, four at a time
    f32x16 acc[AT];
#pragma unroll
    for (int i = 0; i < AT; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
    if (FP8) {
#pragma unroll
      for (int s0 = 0; s0 < K64; s0 += 2) {
        i32x8 bf8[2];
#pragma unroll
        for (int j = 0; j < 2 && s0 + j < K64; ++j) {
          const char* q = rb + ((s0 + j) * 4 + h) * 512 + c * 16;
          const i32x4 lo = *reinterpret_cast<const i32x4*>(q);
          const i32x4 hi = *reinterpret_cast<const i32x4*>(q + 1024);
          bf8[j] = i32x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        }
#pragma unroll
        for (int j = 0; j < 2 && s0 + j < K64; ++j)
#pragma unroll
          for (int i = 0; i < AT; ++i) acc[i] = mfma_f8(bf8[j], ares8[i][s0 + j], acc[i]);
      }
    } else {
#pragma unroll
      for (int s0 = 0; s0 < (FP8 ? 1 : KS); s0 += 4) {
        bf16x8 bf[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) bf[j] = *reinterpret_cast<const bf16x8*>(rb + (((s0 + j) * 2 + h) * 32 + c) * 16);
        bf16x8 af[AT][4];
        if (ALDS) {
#pragma unroll
          for (int i = 0; i < AT; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) af[i][j] = a_lds[(i * KS + s0 + j) * 64];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int i = 0; i < AT; ++i)
            acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bf[j], ALDS ? af[i][j] : ares[i][(FP8 || ALDS) ? 0 : s0 + j], acc[i], 0, 0, 0);
      }
    }
    float ib[16], wb[16];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float4 v = *reinterpret_cast<const float4*>(ivp + 4 * h + 8 * q);
      ib[4 * q] = v.x; ib[4 * q + 1] = v.y; ib[4 * q + 2] = v.z; ib[4 * q + 3] = v.w;
    }
    if constexpr (LQ) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float4 v = *reinterpret_cast<const float4*>(ivp + 32 + 4 * h + 8 * q);
        wb[4 * q] = v.x; wb[4 * q + 1] = v.y; wb[4 * q + 2] = v.z; wb[4 * q + 3] = v.w;
      }
    }
    if (!have_inv) {
#pragma unroll
      for (int r = 0; r < 16; ++r) ib[r] = __builtin_amdgcn_rcpf(ib[r]) * kx;
    }
    const bool ragged = b_lo + 31 >= Rb;
    if (ragged) {
#pragma unroll
      for (int r = 0; r < 16; ++r) ib[r] = b_lo + rowmap(r, h) < Rb ? ib[r] : 0.f;
    }
    const bool band = !(b_lo + 31 < posmin || b_lo > posmax);
#pragma unroll
    for (int i = 0; i < AT; ++i) {
      float w[16];
#pragma unroll
      for (int r = 0; r < 16; ++r)
        w[r] = softmax_term<UNIT, LQ>(acc[i][r], c1, c2, ia[i], ua[i], ib[r], wb[r]);
      if (ragged) {
#pragma unroll
        for (int r = 0; r < 16; ++r) w[r] = b_lo + rowmap(r, h) < Rb ? w[r] : 0.f;
      }
      if (band) {
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (b_lo + rowmap(r, h) == pos[i]) w[r] -= 2.f;
      }
      bf16x8 wf[2];
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int j = 0; j < 8; ++j) wf[s][j] = (__bf16)w[8 * s + j];
      // second product, software-pipelined over batches of BQ fragment reads: batch k + 1 is in flight while batch k's MFMAs
      // issue -- with one wave per SIMD nobody else covers an LDS round trip.  (BQ = 2 for the bf16 D = 256 form: its two a
      // tiles' A fragments alone are 128 registers, and batches of four left 20 bytes of scratch per lane)
      constexpr int BQ = (KS == 16 && !FP8) ? 2 : 4;
      constexpr int NB1 = (DT + BQ - 1) / BQ, NBATCH = 2 * NB1;
      bf16x8 bmq[2][BQ];
      auto bm_read = [&](int k, bf16x8 (&dst)[BQ]) {
        const int s = k / NB1, d0 = BQ * (k % NB1);
#pragma unroll
        for (int j = 0; j < BQ; ++j)
          if (d0 + j < DT) dst[j] = *reinterpret_cast<const bf16x8*>(fb + (((s * 2 + h) * Dp + 32 * (d0 + j) + c) * 16));
      };
      bm_read(0, bmq[0]);
#pragma unroll
      for (int k = 0; k < NBATCH; ++k) {
        if (k + 1 < NBATCH) bm_read(k + 1, bmq[(k + 1) & 1]);
        const int s = k / NB1, d0 = BQ * (k % NB1);
#pragma unroll
        for (int j = 0; j < BQ; ++j)
          if (d0 + j < DT) dacc[i][d0 + j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[s], bmq[k & 1][j], dacc[i][d0 + j], 0, 0, 0);
      }
    }
  }
  const float g = args.d_loss[0] * out_scale;
#pragma unroll
  for (int i = 0; i < AT; ++i)
#pragma unroll
    for (int d = 0; d < DT; ++d)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int a = 32 * (at0 + i) + rowmap(r, h);
        const int dd = 32 * d + c;
        if (a < Ra && dd < args.D) dr.dA[(int64_t)a * args.D + dd] = dacc[i][d][r] * g;
      }
}

// ---- backward, large-batch form, fp8 operands for BOTH products ------------------------------------------
// score_bwd_rows_kernel<.., FP8> halves the matrix-pipe time of the S products only; two thirds of that kernel's MFMA cycles
// are the gradient products dA += W B (K = the b rows), still bf16.  Here they run on v_mfma_scale_f32_32x32x64_f8f6f4 too:
// K = 64 b rows per instruction, so the sweep goes over PAIRS of 32-row tiles, the softmax weights of a pair are converted
// to e4m3 and the b rows come from a third image of the packing (fp8 fragment image: tt_score_bf16.h).
// What makes 3 mantissa bits usable for weights that span 2^-20 .. 1 along a row is the instruction's block scale.  A lane
// (row a = c, half h) of the first operand holds 32 bytes = here: 16 weights of the pair's first tile, then 16 of its second;
// the hardware's blocks are [bytes 0..15 of both halves] scaled by lane (c, 0)'s scale register and [bytes 16..31 of both
// halves] scaled by lane (c, 1)'s (probe: tools/probe/fp8_block_scale.hip) -- i.e. one block = row a x the 32 rows of ONE b
// tile, and its two lanes meet through v_permlane32_swap.  Per block: m = largest weight, scale = 2^(floor(log2 m) - 7)
// (m / scale in [128, 256): the top of e4m3's range, 448), conversion with v_cvt_scalef32_pk_fp8_f32 (divides by the scale's
// power of two, round-to-nearest-even: same probe), the scale's exponent goes into the MFMA: MX-style dynamic block scaling,
// no a-priori bound on the weights.  Weights more than 2^16 below their block's largest flush to zero -- at most 32 x 2^-17
// of that largest one per block.
// The diagonal's weight (e_aa (1/rowsum + 1/colsum) - 2, the one weight of a row that is O(1) and carries the positive
// pair's pull) never goes through e4m3: the lane that meets it keeps it in f32, zeroes it in the block, and the epilogue
// adds (w_aa - 2) * b[pos_a] from the bf16 fragment image.
// Oracle model of this arithmetic: oracle_np.score_ce_bwd(..., block_fp8=True).
// Measured and not kept: running the gradient products of the second wave of every SIMD one pair late (at the top of the
// next pair's interval, fragment image triple-buffered) so that one wave's weights phase faces the other's MFMAs -- bit-identical,
// configs[4] step 7.88 against 7.77 ms: as in the bf16 kernels the two pipes' times add up whatever the waves' phases
// (profiles/NOTES.md).
template <int KS, bool UNIT, int AT, int NWV>
__global__ __launch_bounds__(NWV * 64) void score_bwd_rows8_kernel(BwdArgs args) {
  constexpr int NTH = NWV * 64, DT = KS / 2, Dp = KS * 16, K64 = KS / 4, NF = 2;
  // LDS: [rows-image tiles of a PAIR x 2 | fp8 fragment image of a pair x NF | 64 reciprocals x 2 | A fragments (ALDS)]
  constexpr int kRowsB = KS * 1024, kFragB = KS * 1024, kIvB = 256;
  constexpr int kFragOff = 2 * kRowsB, kIvOff = kFragOff + NF * kFragB, kALdsOff = kIvOff + 2 * kIvB;
  constexpr int kPieces = (kRowsB + kFragB) / 16, kPPT = kPieces / NTH, kRowQ = kRowsB / 16 / NTH;
  static_assert(KS % 4 == 0 && kPieces % NTH == 0 && (kRowsB / 16) % NTH == 0, "fp8 operands come in K = 64 steps; whole 16-byte pieces per thread");
  // D = 256, two waves per SIMD (256 registers each): the wave's own A fragments (32 registers) live in LDS behind the two
  // stages, [wave][k64-step][part][lane] 16-byte pieces (8 KB per wave), and are read back beside the b fragments
  constexpr bool ALDS = KS == 16;
  extern __shared__ __attribute__((aligned(16))) char lds_raw[];
  const BwdSel dr = select_dir(args, blockIdx.y != 0);
  const char* const a_rows = reinterpret_cast<const char*>(dr.a_rows);
  const char* const g_rows = reinterpret_cast<const char*>(dr.b_rows);
  const char* const g_frag = dr.b_frag8;
  const __bf16* const b_frag16 = dr.b_frag;
  float* const dA = dr.dA;
  const float c1 = dr.c1, c2 = args.c2, kx = UNIT ? args.kexp : 1.f;
  const int Ra = dr.Ra, Rb = dr.Rb, off = dr.off;
  const int tid = threadIdx.x, lane = tid & 63, c = lane & 31, h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nP = (Rb + 63) / 64, nTa_img = (int)(rup(Ra, 64) / 32);
  const int at0 = ((int)blockIdx.x * NWV + wave) * AT;
  if ((int)blockIdx.x * NWV * AT * 32 >= Ra) return;                        // (whole workgroup)
  i32x8 ares8[AT][ALDS ? 1 : K64];
  i32x4* const a_lds = reinterpret_cast<i32x4*>(lds_raw + kALdsOff) + (size_t)wave * AT * K64 * 128 + lane;
  float ia[AT], wd[AT];
  int pos[AT];
#pragma unroll
  for (int i = 0; i < AT; ++i) {
    if (ALDS) {
      const char* pa = a_rows + ((int64_t)min(at0 + i, nTa_img - 1) * K64 * 4 + h) * 512 + c * 16;
#pragma unroll
      for (int s2 = 0; s2 < K64; ++s2) {                                    // (wave-private: no barrier)
        a_lds[((i * K64 + s2) * 2) * 64] = *reinterpret_cast<const i32x4*>(pa + (s2 * 4) * 512);
        a_lds[((i * K64 + s2) * 2 + 1) * 64] = *reinterpret_cast<const i32x4*>(pa + (s2 * 4 + 2) * 512);
      }
    } else load_f8frag<(ALDS ? 1 : K64)>(a_rows, min(at0 + i, nTa_img - 1), c, h, ares8[i]);
    [[maybe_unused]] float ua;
    a_row_setup<false>(dr, kx, 32 * (at0 + i) + c, ia[i], ua, pos[i]);
    wd[i] = 0.f;                                                            // stays 0 in the lanes that never meet the diagonal
  }
  const int posmin = 32 * at0 + off, posmax = 32 * (at0 + AT) - 1 + off;
  f32x16 dacc[AT][DT];
  zero_acc(dacc);
  const bool have_inv = dr.inv_b != nullptr;
  const float* const ivsrc = have_inv ? dr.inv_b : dr.sumexp_b;
  const int iv_last = (int)rup(Rb, 32) - 4;                                  // the per-row arrays are readable up to a multiple of 32 rows
  // stage = the pair's [two rows-image tiles | fp8 fragment image | 64 reciprocals], by LDS-DMA as in score_bwd_rows_kernel
  auto stage_dma = [&](int pn, int rbuf, int fbuf) {
#pragma unroll
    for (int q = 0; q < kPPT; ++q) {
      const char* src = q < kRowQ ? g_rows + (int64_t)pn * kRowsB + (tid + NTH * q) * 16 : g_frag + (int64_t)pn * kFragB + (tid + NTH * (q - kRowQ)) * 16;
      char* dst = q < kRowQ ? lds_raw + rbuf * kRowsB + (wave * 64 + NTH * q) * 16 : lds_raw + kFragOff + fbuf * kFragB + (wave * 64 + NTH * (q - kRowQ)) * 16;
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src, (__attribute__((address_space(3))) void*)dst, 16, 0, 0);
    }
    if (wave == 0 && lane < 16)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(ivsrc + min(64 * pn + 4 * lane, iv_last)),
                                       (__attribute__((address_space(3))) void*)(lds_raw + kIvOff + rbuf * kIvB), 16, 0, 0);
  };
  i32x8 wA[AT];
  int e8[AT];
#pragma unroll
  for (int i = 0; i < AT; ++i) {
    wA[i] = i32x8{0, 0, 0, 0, 0, 0, 0, 0};
    e8[i] = 0;
  }
  // gradient products of one pair: one MFMA per 32 columns of d and a tile, K = the pair's 64 b rows; fragment d + 1 is in
  // flight while fragment d's MFMAs issue
  auto grad = [&](const char* fb) {
    i32x8 bm8[2];
    auto bm_read = [&](int d, i32x8& dst) { dst = f8frag_at(fb + (d * 4 + h) * 512 + c * 16); };
    bm_read(0, bm8[0]);
#pragma unroll
    for (int d = 0; d < DT; ++d) {
      if (d + 1 < DT) bm_read(d + 1, bm8[(d + 1) & 1]);
#pragma unroll
      for (int i = 0; i < AT; ++i)
        dacc[i][d] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(wA[i], bm8[d & 1], dacc[i][d], 0, 0, 0, e8[i], 0, kFp8ScaleE8M0);
      __builtin_amdgcn_sched_barrier(0);
    }
  };
  stage_dma(0, 0, 0);
  for (int p = 0; p < nP; ++p) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (p + 1 < nP) stage_dma(p + 1, (p + 1) & 1, (p + 1) & 1);
    const char* rb = lds_raw + (p & 1) * kRowsB;
    const char* fb = lds_raw + kFragOff + (p & 1) * kFragB;
    const float* ivp = reinterpret_cast<const float*>(lds_raw + kIvOff + (p & 1) * kIvB);
    const int b_lo = 64 * p;
    f32x16 acc[AT][2];
#pragma unroll
    for (int i = 0; i < AT; ++i)
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][t][r] = 0.f;
    // S products, software-pipelined by hand: k-step s + 1's fragments are in flight while step s's MFMAs issue (left to
    // itself hipcc hoists all 24 reads of the phase in front of the first MFMA: 96 registers, and spills accumulators)
    i32x8 bf8[2][2], af8[2][AT];
    auto s_read = [&](int s, i32x8 (&bdst)[2], i32x8 (&adst)[AT]) {
#pragma unroll
      for (int t = 0; t < 2; ++t) bdst[t] = f8frag_at(rb + t * (kRowsB / 2) + (s * 4 + h) * 512 + c * 16);
      if (ALDS) {                                                          // (its two pieces lie 64 lanes = 1024 bytes apart too)
#pragma unroll
        for (int i = 0; i < AT; ++i) adst[i] = f8frag_at(reinterpret_cast<const char*>(a_lds + ((i * K64 + s) * 2) * 64));
      }
    };
    s_read(0, bf8[0], af8[0]);
#pragma unroll
    for (int s = 0; s < K64; ++s) {
      if (s + 1 < K64) s_read(s + 1, bf8[(s + 1) & 1], af8[(s + 1) & 1]);
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int i = 0; i < AT; ++i) acc[i][t] = mfma_f8(bf8[s & 1][t], ALDS ? af8[s & 1][i] : ares8[i][ALDS ? 0 : s], acc[i][t]);
      __builtin_amdgcn_sched_barrier(0);
    }
    // (pins the MFMAs to this block: their results are first read behind the branches below, and the machine sinker otherwise
    // moves the whole chain there, behind all of the phase's reads)
#pragma unroll
    for (int i = 0; i < AT; ++i)
#pragma unroll
      for (int t = 0; t < 2; ++t) asm volatile("" : "+v"(acc[i][t]));
    const bool ragged = b_lo + 63 >= Rb;
    const bool band = !(b_lo + 63 < posmin || b_lo > posmax);
    // softmax weights of the pair, in place in the S accumulators, and the largest one this lane holds of either tile
    float wmax[AT][2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      float ib[16];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float4 v = *reinterpret_cast<const float4*>(ivp + 32 * t + 4 * h + 8 * q);
        ib[4 * q] = v.x; ib[4 * q + 1] = v.y; ib[4 * q + 2] = v.z; ib[4 * q + 3] = v.w;
      }
      if (!have_inv) {
#pragma unroll
        for (int r = 0; r < 16; ++r) ib[r] = __builtin_amdgcn_rcpf(ib[r]) * kx;
      }
#pragma unroll
      for (int i = 0; i < AT; ++i) {
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][t][r] = softmax_term<UNIT, false>(acc[i][t][r], c1, c2, ia[i], 0.f, ib[r], 0.f);
        if (ragged) {
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[i][t][r] = b_lo + 32 * t + rowmap(r, h) < Rb ? acc[i][t][r] : 0.f;
        }
        if (band) {
#pragma unroll
          for (int r = 0; r < 16; ++r)
            if (b_lo + 32 * t + rowmap(r, h) == pos[i]) {
              wd[i] = acc[i][t][r] - 2.f;
              acc[i][t][r] = 0.f;
            }
        }
        wmax[i][t] = 0.f;
#pragma unroll
        for (int r = 0; r < 16; r += 2) wmax[i][t] = max3_asm(wmax[i][t], acc[i][t][r], acc[i][t][r + 1]);
      }
    }
#pragma unroll
    for (int i = 0; i < AT; ++i) {
      // the block's two lanes: after the swap lane (c, 0) holds both halves' maxima of tile 0, lane (c, 1) those of tile 1 --
      // the tile whose scale the MFMA takes from that lane
      const auto mm = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(unsigned, wmax[i][0]), __builtin_bit_cast(unsigned, wmax[i][1]), false, false);
      const unsigned m_own = max(mm[0], mm[1]);                            // (non-negative floats order like their bit patterns)
      // scale = 2^(floor(log2 m) - 7), floored at 2^-110 (an all-zero block converts to zeros at any scale)
      const unsigned sb_own = (max(m_own, 0x0C000000u) & 0x7F800000u) - (7u << 23);
      e8[i] = (int)(sb_own >> 23);
      // tile 0's scale in every lane / tile 1's.  (Elements taken out by constant index: indexed with the unrolled loop's
      // variable, sb[t], hipcc 7.2 folds both reads to element 0 and converts both tiles with tile 0's scale.)
      const auto sb = __builtin_amdgcn_permlane32_swap(sb_own, sb_own, false, false);
      const unsigned sb0 = sb[0], sb1 = sb[1];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const float scale = __builtin_bit_cast(float, t ? sb1 : sb0);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          // (the conversion writes one 16-bit half of its destination and keeps the other.  Through the builtin the first of
          //  a word's two conversions needs a defined `old` value -- a v_mov per word, 8 of the pair's ~144 vector instructions;
          //  as inline asm its destination is write-only and the second conversion fills the other half)
          int u;
          asm("v_cvt_scalef32_pk_fp8_f32 %0, %1, %2, %3" : "=v"(u) : "v"(acc[i][t][4 * q]), "v"(acc[i][t][4 * q + 1]), "v"(scale));
          asm("v_cvt_scalef32_pk_fp8_f32 %0, %1, %2, %3 op_sel:[0,0,0,1]" : "+v"(u) : "v"(acc[i][t][4 * q + 2]), "v"(acc[i][t][4 * q + 3]), "v"(scale));
          wA[i][4 * t + q] = u;
        }
      }
    }
    grad(fb);
  }
  // epilogue: + (w_aa - 2) b[pos_a] with the bf16 image's row (a lane holds the diagonal weight of row a = its column index c,
  // the accumulators are laid out by row: one cross-lane read per register)
  const float g = args.d_loss[0] * dr.out_scale;
  const int nTb_img = (int)(rup(Rb, 64) / 32);
#pragma unroll
  for (int i = 0; i < AT; ++i) {
    const float wd_row = wd[i] + __shfl_xor(wd[i], 32);                    // one of the two halves met it (or neither: 0)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int arow = rowmap(r, h);
      const float wv = __shfl(wd_row, arow);
      const int pb = 32 * (at0 + i) + arow + off;
      const int a = 32 * (at0 + i) + arow;
      const bool diag_ok = pb >= 0 && pb < 32 * nTb_img;
      const int pbc = diag_ok ? pb : 0;
      const int t = pbc >> 5, rr = pbc & 31, s = rr >> 4, r16 = rr & 15, hh = (r16 >> 2) & 1, j = ((r16 >> 3) << 2) | (r16 & 3);
      const __bf16* prow = b_frag16 + ((((int64_t)t * 2 + s) * 2 + hh) * Dp) * 8 + j;
#pragma unroll
      for (int d = 0; d < DT; ++d) {
        const int dd = 32 * d + c;
        if (a < Ra && dd < args.D) {
          const float bv = diag_ok ? (float)prow[dd * 8] : 0.f;
          dA[(int64_t)a * args.D + dd] = __builtin_fmaf(wv, bv, dacc[i][d][r]) * g;
        }
      }
    }
  }
}

}  // namespace

// the *_lq backward entries: per-direction sampling weights into the launch arguments (lq == NULL: the plain entry)
static int bwd_lq_args(BwdArgs& a, const tt_score_bwd_lq* lq, int32_t n_dirs, float inv_t, const char* who) {
  if (!lq) return TT_OK;
  if (2.f * fabsf(inv_t) > kLqMaxTwoInvT) {
    tt_set_error("%s: 1/temperature = %g: the logQ-corrected softmax needs 2/T <= %g", who, inv_t, kLqMaxTwoInvT);
    return TT_ERR_UNSUPPORTED;
  }
  for (int i = 0; i < 2; ++i) {
    const tt_score_bwd_lq& q = lq[i < n_dirs ? i : 0];
    TT_CHECK_ARG(q.w_a && q.w_b && tt_aligned(q.w_b, 16), "%s: direction %d: w_a / w_b NULL or w_b not 16-byte aligned", who, i);
    a.wt_a[i] = q.w_a;
    a.wt_b[i] = q.w_b;
  }
  return TT_OK;
}

// (KS, AT, NW) of the two-direction forward per padded D = 32, 64, 128, 256
constexpr int kFwdTile[2][4][3] = {
    // bf16.  D <= 64: 32 rows per wave (AT = 1), 8 waves, 2 workgroups per CU measured best (43.6 us; AT = 2: 48.0, 4 waves:
    // 53.4, 16 waves: 48.7 at B = 8192)
    {{2, 2, 8}, {4, 1, 8}, {8, 2, 8}, {16, 1, 8}},
    // bf16x3.  D = 256: one wave per SIMD: the hi / lo fragments of A and of a b tile are 256 registers
    {{2, 2, 8}, {4, 1, 8}, {8, 1, 8}, {16, 1, 4}},
};

// tt_score_fwd_bf16 / tt_score_fwd_bf16x3 (x3: the operands are [hi | lo] packings)
static int fwd_bf16(tt_ctx* ctx, const tt_score_fwd_dir* dirs, int32_t n_dirs, int32_t D, float inv_t, float shift, tt_stream stream,
                    bool x3, const char* who) {
  TT_CHECK_ARG(ctx && dirs && (n_dirs == 1 || n_dirs == 2), "%s: need 1 or 2 directions", who);
  TT_CHECK_ARG(D >= 1 && D <= 256, "%s: D=%d not in [1,256]", who, D);
  if (2.f * fabsf(inv_t) > 80.f) {
    tt_set_error("%s: 1/temperature = %g: fixed-shift softmax needs 2/T <= 80", who, inv_t);
    return TT_ERR_UNSUPPORTED;
  }
  FwdArgs a{};
  int64_t maxRa = 0;
  bool unit = true;
  for (int i = 0; i < 2; ++i) {
    const tt_score_fwd_dir& d = dirs[i < n_dirs ? i : 0];
    TT_CHECK_ARG(d.A_packed && d.B_packed && d.sumexp && d.Ra >= 1 && d.Rb >= 1, "%s: bad direction %d", who, i);
    const float ab = d.ab_scale == 0.f ? 1.f : d.ab_scale;
    a.d[i] = DirFwd{view(d.A_packed, d.Ra, D).rows, view(d.B_packed, d.Rb, D).rows, d.Ra, d.Rb, d.diag_offset, d.sumexp, d.diag, d.rank, d.sumscore,
                    d.rank ? (d.rank_mode == 1 ? 1 : 2) : 0, inv_t * kLog2e / ab, inv_t / ab, d.inv_sumexp};
    if (x3) {
      a.d[i].a_lo = view_lo(d.A_packed, d.Ra, D).rows;
      a.d[i].b_lo = view_lo(d.B_packed, d.Rb, D).rows;
    }
    unit = unit && ab == inv_t * kLog2e;                // exactly: the caller got the scale from tt_score_unit_scale(inv_t)
    maxRa = d.Ra > maxRa ? d.Ra : maxRa;
  }
  a.c2 = -shift * kLog2e;
  a.kexp = exp2f(a.c2);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const auto go = [&](auto x3c, auto di) {
    constexpr int KS = kFwdTile[x3c][di][0], AT = kFwdTile[x3c][di][1], NW = kFwdTile[x3c][di][2];
    const dim3 grid((unsigned)tt_cdiv(maxRa, 32 * AT), (unsigned)n_dirs);
    tt_dispatch([&](auto u) { score_fwd_bf16_kernel<KS, AT, NW, u, x3c><<<grid, NW * 64, 0, st>>>(a); }, unit);
  };
  tt_dispatch([&](auto x3c) {
    switch (padded_d(D)) {
      case 32: return go(x3c, tt_c<0>);
      case 64: return go(x3c, tt_c<1>);
      case 128: return go(x3c, tt_c<2>);
      default: return go(x3c, tt_c<3>);
    }
  }, x3);
  TT_LAUNCH_CHECK();
  return TT_OK;
}

// ---- backward: the launch arguments of every form, then one launch per form --------------------------------------------
struct BwdSetup {
  BwdArgs a;
  int64_t maxRa;
  int n_dirs;
  bool unit, lq;
};

// checks the entry's arguments and fills the launch arguments from tt_score_bwd_dir[] (lq != NULL: the *_lq entries)
static int bwd_setup(BwdSetup& s, Operands op, tt_ctx* ctx, const tt_score_bwd_dir* dirs, const tt_score_bwd_lq* lq, int32_t n_dirs,
                     int32_t D, float inv_t, float shift, const float* d_loss, float scale, const char* who) {
  TT_CHECK_ARG(ctx && dirs && d_loss && (n_dirs == 1 || n_dirs == 2), "%s: need 1 or 2 directions", who);
  TT_CHECK_ARG(D >= 1 && D <= 256, "%s: D=%d not in [1,256]", who, D);
  s = BwdSetup{};
  if (int rc = bwd_lq_args(s.a, lq, n_dirs, inv_t, who)) return rc;
  s.n_dirs = n_dirs;
  s.unit = true;
  s.lq = lq != nullptr;
  for (int i = 0; i < 2; ++i) {
    const tt_score_bwd_dir& d = dirs[i < n_dirs ? i : 0];
    TT_CHECK_ARG(d.A_packed && d.B_packed && d.sumexp_a && d.sumexp_b && d.dA && d.Ra >= 1 && d.Rb >= 1, "%s: bad direction %d", who, i);
    if (op == Operands::bf16) {
      TT_CHECK_ARG(tt_aligned(d.sumexp_b, 16), "%s: sumexp_b must be 16-byte aligned", who);
      TT_CHECK_ARG(d.inv_b == nullptr || tt_aligned(d.inv_b, 16), "%s: inv_b must be 16-byte aligned", who);
    } else {
      TT_CHECK_ARG(tt_aligned(d.sumexp_b, 16) && (d.inv_b == nullptr || tt_aligned(d.inv_b, 16)),
                   "%s: per-row arrays must be 16-byte aligned", who);
    }
    const float ab = d.ab_scale == 0.f ? 1.f : d.ab_scale, bs = d.b_scale == 0.f ? 1.f : d.b_scale;
    DirBwd& r = s.a.d[i];
    r = DirBwd{nullptr, nullptr, nullptr, d.Ra, d.Rb, d.diag_offset, d.sumexp_a, d.sumexp_b, d.dA, inv_t * kLog2e / ab, scale / bs, d.inv_a, d.inv_b};
    if (op == Operands::fp8) {
      const PackedView8 va = view8(d.A_packed, d.Ra, D), vb = view8(d.B_packed, d.Rb, D);
      r.a_rows = reinterpret_cast<const __bf16*>(va.rows8);
      r.b_rows = reinterpret_cast<const __bf16*>(vb.rows8);
      r.b_frag = vb.frag;
      r.b_frag8 = vb.frag8;
    } else {
      const PackedView vb = view(d.B_packed, d.Rb, D);
      r.a_rows = view(d.A_packed, d.Ra, D).rows;
      r.b_rows = vb.rows;
      r.b_frag = vb.frag;
      if (op == Operands::bf16x3) {
        const PackedView vbl = view_lo(d.B_packed, d.Rb, D);
        r.a_lo = view_lo(d.A_packed, d.Ra, D).rows;
        r.b_lo = vbl.rows;
        r.b_frag_lo = vbl.frag;
      }
    }
    s.unit = s.unit && ab == inv_t * kLog2e;
    s.maxRa = d.Ra > s.maxRa ? d.Ra : s.maxRa;
  }
  s.a.c2 = -shift * kLog2e;
  s.a.kexp = exp2f(s.a.c2);
  s.a.d_loss = d_loss;
  s.a.D = D;
  return TT_OK;
}

// b-split form (score_bwd_bf16_kernel): X3 split-bf16 operands, MK the repeated-entity mask, PW pair weights
template <int KS, int AT, int NW, bool X3, bool MK = false, bool PW = false>
static void launch_bsplit(const BwdSetup& s, hipStream_t st) {
  const dim3 grid((unsigned)tt_cdiv(s.maxRa, 32 * AT), (unsigned)s.n_dirs);
  tt_dispatch([&](auto u, auto l) { score_bwd_bf16_kernel<KS, AT, NW, u, X3, l, MK, PW><<<grid, NW * 64, 0, st>>>(s.a); }, s.unit, s.lq);
}

// (KS, AT) per padded D = 32, 64, 128, 256 of the forms that run one wave per SIMD (NW = 4): two a tiles per workgroup at D <= 64 --
// half the workgroups, half the L2 bytes of the streamed b images.  f(tt_c<KS>, tt_c<AT>).
template <class F>
static void one_wave_tile(int Dp, F&& f) {
  switch (Dp) {
    case 32: f(tt_c<2>, tt_c<2>); break;
    case 64: f(tt_c<4>, tt_c<2>); break;
    case 128: f(tt_c<8>, tt_c<1>); break;
    default: f(tt_c<16>, tt_c<1>); break;
  }
}

// one streamed image, transposing LDS reads (score_bwd_tr_kernel)
template <int KS, int AT>
static void launch_tr(const BwdSetup& s, hipStream_t st) {
  const dim3 grid((unsigned)tt_cdiv(s.maxRa, 32 * AT), (unsigned)s.n_dirs);
  tt_dispatch([&](auto u, auto l) { score_bwd_tr_kernel<KS, AT, u, l><<<grid, 512, 0, st>>>(s.a, TailHost<false>{}); }, s.unit, s.lq);
}

// ---- TT_OPT_FUSE_SCORE_TAIL: a launch_tr<4, 2> launch held back in the context (slot TT_DQ_SCORE_BWD, tt_deferred.h) --------------
// Held: two directions over square problems of the same size, no logQ -- what the towers' backward can host.  Launched exactly once:
// by tt_score_tail_bwd_launch (with the towers' backward head in its epilogue) or by tt_deferred_flush (tt_score_bwd_run).
static_assert(std::is_trivially_copyable<BwdSetup>::value, "the queue keeps a byte copy of BwdSetup");

static bool bwd_hostable(const tt_ctx* ctx, const BwdSetup& s) {
  const DirBwd* d = s.a.d;
  return ctx->dq->fuse_score_tail && !s.lq && s.n_dirs == 2 && d[0].Ra == d[0].Rb && d[1].Ra == d[1].Rb && d[0].Ra == d[1].Ra;
}

int tt_score_bwd_run(const void* setup, hipStream_t st) {
  launch_tr<4, 2>(*static_cast<const BwdSetup*>(setup), st);
  TT_LAUNCH_CHECK();
  return TT_OK;
}

int tt_score_tail_bwd_launch(tt_ctx* ctx, const tttail::Batch<tttail::TailBwdArgs>& tb, bool drop, float p, uint64_t seed,
                             const uint64_t* seed_dev) {
  TT_CHECK_ARG(ctx->dq->on & TT_DQ_SCORE_BWD, "tt_score_tail_bwd_launch: no score backward is queued");
  const BwdSetup& s = *static_cast<const BwdSetup*>(ctx->dq->score);
  hipStream_t st = ctx->dq->st[0];
  tt_deferred_taken(ctx, TT_DQ_SCORE_BWD);
  const dim3 grid((unsigned)tt_cdiv(s.maxRa, 64), 2);
  tt_dispatch([&](auto u) { score_bwd_tr_kernel<4, 2, u, false, true><<<grid, 512, 0, st>>>(s.a, TailHost<true>{tb, drop, p, seed, seed_dev}); }, s.unit);
  TT_LAUNCH_CHECK();
  return TT_OK;
}

// workgroup-staged form (score_bwd_rows_kernel); FP8: fp8 S operands (no logQ form)
template <int KS, bool FP8, int AT, int NWV>
static int launch_rows(tt_ctx* ctx, const BwdSetup& s, hipStream_t st) {
  const dim3 grid((unsigned)tt_cdiv(s.maxRa, 32 * AT * NWV), (unsigned)s.n_dirs);
  const size_t lds = 2 * (size_t)((FP8 ? KS * 512 : KS * 1024) + KS * 1024 + 256) + (!FP8 && KS == 16 ? (size_t)NWV * AT * KS * 1024 : 0);
  const auto go = [&](auto u, auto l) -> int {
    TT_LDS_ONCE(lds, &score_bwd_rows_kernel<KS, u, FP8, AT, NWV, l>);
    score_bwd_rows_kernel<KS, u, FP8, AT, NWV, l><<<grid, NWV * 64, lds, st>>>(s.a);
    return TT_OK;
  };
  if constexpr (FP8) return tt_dispatch([&](auto u) { return go(u, std::false_type{}); }, s.unit);
  else return tt_dispatch(go, s.unit, s.lq);
}

// fp8 operands for both products (score_bwd_rows8_kernel)
template <int KS, int AT, int NWV>
static int launch_rows8(tt_ctx* ctx, const BwdSetup& s, hipStream_t st) {
  const dim3 grid((unsigned)tt_cdiv(s.maxRa, 32 * AT * NWV), (unsigned)s.n_dirs);
  const size_t lds = (size_t)4 * KS * 1024 + 512 + (KS == 16 ? (size_t)NWV * AT * KS * 512 : 0);
  return tt_dispatch([&](auto u) -> int {
    TT_LDS_ONCE(lds, &score_bwd_rows8_kernel<KS, u, AT, NWV>);
    score_bwd_rows8_kernel<KS, u, AT, NWV><<<grid, NWV * 64, lds, st>>>(s.a);
    return TT_OK;
  }, s.unit);
}

// tt_score_bwd_bf16 and, with lq != NULL, tt_score_bwd_bf16_lq
static int bwd_bf16(tt_ctx* ctx, const tt_score_bwd_dir* dirs, const tt_score_bwd_lq* lq, int32_t n_dirs, int32_t D, float inv_t,
                    float shift, const float* d_loss, float scale, tt_stream stream, const char* who) {
  BwdSetup s;
  if (int rc = bwd_setup(s, Operands::bf16, ctx, dirs, lq, n_dirs, D, inv_t, shift, d_loss, scale, who)) return rc;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int Dp = padded_d(D);
  // enough rows for every SIMD to own 64 of them: the workgroup-staged form (no split along b, operands shared through LDS)
  if (s.maxRa >= ctx->score_bwd_rows_min && Dp >= 64) {
    // D = 256: one a tile per wave with its A fragments in LDS (16 KB per wave: four waves beside the two 33-KB stages) -- with
    // two a tiles per wave the A fragments (128 registers) and the accumulators (256) filled the whole file and hipcc shuttled
    // hundreds of values between AGPRs, VGPRs and scratch (20-116 bytes of scratch per lane in the tile loop)
    const int rc = Dp == 64 ? launch_rows<4, false, 2, 4>(ctx, s, st)
                   : Dp == 128 ? launch_rows<8, false, 2, 4>(ctx, s, st) : launch_rows<16, false, 1, 4>(ctx, s, st);
    if (rc) return rc;
  } else if (Dp == 32) {
    launch_bsplit<2, 2, 8, false>(s, st);
  } else if (Dp == 64) {
    if (bwd_hostable(ctx, s))                             // TT_OPT_FUSE_SCORE_TAIL: tt_towers_mlp_bwd launches it, or a flush
      return tt_deferred_queue_score_bwd(ctx, st, &s, sizeof(s), s.a.d[0].dA, s.a.d[1].dA, s.maxRa);
    if (int rc = tt_deferred_flush(ctx, TT_DQ_SCORE_BWD)) return rc;      // (a queued one goes in front of this launch)
    launch_tr<4, 2>(s, st);
  } else if (Dp == 128) {                                 // the one-image form, one a tile per workgroup
    launch_tr<8, 1>(s, st);
  } else {
    launch_bsplit<16, 1, 4, false>(s, st);
  }
  TT_LAUNCH_CHECK();
  return TT_OK;
}

// the optional terms of the square backward entries (tt_score_bwd_bf16_mask / _pw / _cells); `term` names the entry's own in messages
struct SquareTerms {
  const char* term;
  const int32_t *ent_n, *ent_c;          // the repeated-entity mask (both or neither)
  const float* g;                        // pair weights (with them, the weighted forward's folded reciprocals are required)
  const int32_t* plan;                   // masked cells, with the extras' share behind them:
  int64_t capacity, M;
  const void* X_packed;
  const float *inv_row, *w_x;
  float* dX;
};

static XnegArgs xneg_args(const PackedView& vn, const PackedView& vx, int64_t B, int64_t M, const float* inv_row, const float* w_x,
                          const int32_t* ent_c, const int32_t* ent_x, float* dN, float* dX, int32_t D, float inv_t, float shift,
                          const float* d_loss, float scale, float ab) {
  XnegArgs a{};
  a.d[0] = XnegDir{vn.rows, vx.rows, vx.frag, (int)B, (int)M, inv_row, w_x, ent_c, ent_x, dN, scale, 1};          // B image = X: unscaled
  a.d[1] = XnegDir{vx.rows, vn.rows, vn.frag, (int)M, (int)B, w_x, inv_row, ent_x, ent_c, dX, scale / ab, 0};     // B image = the notices'
  a.c1 = inv_t * kLog2e / ab;
  a.c2 = -shift * kLog2e;
  a.d_loss = d_loss;
  a.D = D;
  return a;
}

// tt_score_bwd_bf16_mask / _pw / _cells: the square problem with the repeated-entity mask, per-pair sample weights or masked cells (lq
// NULL: uncorrected).  One form for every shape, the b-split kernel: it takes any B and D <= 256 and the ids ride with its streamed
// tiles.  Masked instantiations of the transposing and the workgroup-staged forms: not built (profiles/NOTES.md, "repeated-entity
// mask").  One wave per SIMD, as the bf16x3 launches -- the b ids of two tiles in flight are 64 registers.  Never queued for the
// towers' backward launch: a queued score backward goes in front of it.  Pair weights: the reciprocals must be the weighted forward's
// -- without them the kernel would form unweighted ones from the sums.  Cells: the kernels, their tiles and their launches are
// tt_score_cells.hip's, with X_packed the extras' two rectangular directions behind the square ones, all on one plan.
static int bwd_square_terms(tt_ctx* ctx, const tt_score_bwd_dir* dirs, const SquareTerms& t, const tt_score_bwd_lq* lq, int32_t n_dirs,
                            int32_t D, float inv_t, float shift, const float* d_loss, float scale, tt_stream stream, const char* who) {
  TT_CHECK_ARG((t.ent_n != nullptr) == (t.ent_c != nullptr), "%s: ent_n and ent_c go together", who);
  TT_CHECK_ARG(!t.ent_n || (tt_aligned(t.ent_n, 16) && tt_aligned(t.ent_c, 16)), "%s: ent_n / ent_c not 16-byte aligned", who);
  BwdSetup s;
  if (int rc = bwd_setup(s, Operands::bf16, ctx, dirs, lq, n_dirs, D, inv_t, shift, d_loss, scale, who)) return rc;
  for (int i = 0; i < n_dirs; ++i) {
    if (dirs[i].Ra != dirs[i].Rb || dirs[i].diag_offset != 0 || dirs[i].Ra != dirs[0].Ra) {
      tt_set_error("%s: %s the square problem only (Ra == Rb, diag_offset == 0)", who, t.term);
      return TT_ERR_UNSUPPORTED;
    }
    TT_CHECK_ARG(!t.g || (dirs[i].inv_a && dirs[i].inv_b), "%s: direction %d: inv_a / inv_b (the weighted forward's folded reciprocals) are required",
                 who, i);
  }
  s.a.ent_n = t.ent_n;
  s.a.ent_c = t.ent_c;
  s.a.pw_g = t.g;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (!t.plan) {
    if (int rc = tt_deferred_flush(ctx, TT_DQ_SCORE_BWD)) return rc;
    const int Dp = padded_d(D);
    if (t.g) tt_dispatch([&](auto m) { one_wave_tile(Dp, [&](auto ks, auto at) { launch_bsplit<ks, at, 4, false, m, true>(s, st); }); }, t.ent_n != nullptr);
    else one_wave_tile(Dp, [&](auto ks, auto at) { launch_bsplit<ks, at, 4, false, true>(s, st); });
    TT_LAUNCH_CHECK();
    return TT_OK;
  }
  const int64_t B = dirs[0].Ra, M = t.M;
  TT_CHECK_ARG(dirs[0].dA != dirs[1].dA && dirs[0].A_packed == dirs[1].B_packed && dirs[1].A_packed == dirs[0].B_packed,
               "%s: the directions must be (N, C) and (C, N)", who);
  if (t.X_packed) {
    TT_CHECK_ARG(M >= 1 && M < ((int64_t)1 << 30) && t.inv_row && t.w_x && t.dX, "%s: the extras need M >= 1, inv_row, w_x and dX", who);
    TT_CHECK_ARG(tt_aligned(t.inv_row, 16) && tt_aligned(t.w_x, 16), "%s: inv_row / w_x must be 16-byte aligned", who);
  } else {
    TT_CHECK_ARG(M == 0, "%s: M = %lld without X_packed", who, (long long)M);
  }
  if (int rc = tt_deferred_flush(ctx, TT_DQ_SCORE_BWD)) return rc;
  // the KP instantiations live in tt_score_cells.hip (tt_score_bwd_bsplit.h): the launch arguments go over as bytes, as a queued
  // score backward's do (both translation units build BwdArgs / XnegArgs from the same header)
  static_assert(std::is_trivially_copyable<BwdArgs>::value && std::is_trivially_copyable<XnegArgs>::value, "the arguments travel as bytes");
  if (int rc = tt_score_bwd_cells_square(&s.a, sizeof(s.a), s.maxRa, s.unit, s.lq, D, t.plan, t.capacity, B, M, st)) return rc;
  if (!t.X_packed) return TT_OK;
  const float ab = dirs[0].ab_scale == 0.f ? 1.f : dirs[0].ab_scale;
  const XnegArgs a = xneg_args(view(dirs[0].A_packed, B, D), view(t.X_packed, M, D), B, M, t.inv_row, t.w_x, nullptr, nullptr, dirs[0].dA,
                               t.dX, D, inv_t, shift, d_loss, scale, ab);
  return tt_score_bwd_cells_xneg(&a, sizeof(a), s.unit, D, t.plan, t.capacity, B, M, st);
}

// tt_score_bwd_bf16_xneg: one launch of score_bwd_xneg_kernel over (N, X) -> dN += and (X, N) -> dX, on the one-wave-per-SIMD tiles.
// Never queued for the towers' backward launch; a queued score backward goes in front of it (it stores the dN this launch adds to).
static int bwd_bf16_xneg(tt_ctx* ctx, const void* N_packed, const void* X_packed, int64_t B, int64_t M, int32_t D, float inv_t, float shift,
                         float ab_scale, const float* inv_row, const float* w_x, const int32_t* ent_c, const int32_t* ent_x,
                         const float* d_loss, float scale, float* dN, float* dX, tt_stream stream, const char* who) {
  TT_CHECK_ARG(ctx && N_packed && X_packed && inv_row && w_x && d_loss && dN && dX, "%s: NULL argument", who);
  TT_CHECK_ARG(B >= 1 && B < ((int64_t)1 << 30) && M >= 1 && M < ((int64_t)1 << 30) && D >= 1 && D <= 256, "%s: bad shape B=%lld M=%lld D=%d", who,
               (long long)B, (long long)M, D);
  TT_CHECK_ARG(tt_aligned(inv_row, 16) && tt_aligned(w_x, 16), "%s: inv_row / w_x must be 16-byte aligned", who);
  TT_CHECK_ARG((ent_c != nullptr) == (ent_x != nullptr), "%s: ent_c and ent_x go together", who);
  TT_CHECK_ARG(!ent_c || (tt_aligned(ent_c, 16) && tt_aligned(ent_x, 16)), "%s: ent_c / ent_x not 16-byte aligned", who);
  if (2.f * fabsf(inv_t) > 80.f) {
    tt_set_error("%s: 1/temperature = %g: fixed-shift softmax needs 2/T <= 80", who, inv_t);
    return TT_ERR_UNSUPPORTED;
  }
  const float ab = ab_scale == 0.f ? 1.f : ab_scale;
  const XnegArgs a = xneg_args(view(N_packed, B, D), view(X_packed, M, D), B, M, inv_row, w_x, ent_c, ent_x, dN, dX, D, inv_t, shift, d_loss,
                               scale, ab);
  const bool unit = ab == inv_t * kLog2e;
  const int64_t maxRa = B > M ? B : M;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (int rc = tt_deferred_flush(ctx, TT_DQ_SCORE_BWD)) return rc;
  one_wave_tile(padded_d(D), [&](auto ks, auto at) {
    const dim3 grid((unsigned)tt_cdiv(maxRa, 32 * at), 2);
    tt_dispatch([&](auto u, auto m) { score_bwd_xneg_kernel<ks, at, 4, u, m><<<grid, 4 * 64, 0, st>>>(a); }, unit, ent_c != nullptr);
  });
  TT_LAUNCH_CHECK();
  return TT_OK;
}

// tt_score_bwd_bf16x3 and, with lq != NULL, tt_score_bwd_bf16x3_lq.
// One form for every shape: the b-split kernel (the rows and fragment images streamed per wave, no LDS in the tile loop).  It
// takes any B and D <= 256 with no operand staging of its own -- the transposing form's parked tiles (100 KB of LDS) and the
// workgroup-staged form's stages would both double for the lo images.  One wave per SIMD (4 waves): the hi and lo operands of
// two b tiles in flight need more than the 256 registers a wave gets at two waves per SIMD.
static int bwd_bf16x3(tt_ctx* ctx, const tt_score_bwd_dir* dirs, const tt_score_bwd_lq* lq, int32_t n_dirs, int32_t D, float inv_t,
                      float shift, const float* d_loss, float scale, tt_stream stream, const char* who) {
  BwdSetup s;
  if (int rc = bwd_setup(s, Operands::bf16x3, ctx, dirs, lq, n_dirs, D, inv_t, shift, d_loss, scale, who)) return rc;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  one_wave_tile(padded_d(D), [&](auto ks, auto at) { launch_bsplit<ks, at, 4, true>(s, st); });
  TT_LAUNCH_CHECK();
  return TT_OK;
}

extern "C" {

float tt_score_unit_scale(float inv_t) { return inv_t * kLog2e; }

int tt_score_fwd_bf16(tt_ctx* ctx, const tt_score_fwd_dir* dirs, int32_t n_dirs, int32_t D, float inv_t, float shift,
                      tt_stream stream) {
  return fwd_bf16(ctx, dirs, n_dirs, D, inv_t, shift, stream, false, "tt_score_fwd_bf16");
}

int tt_score_bwd_bf16(tt_ctx* ctx, const tt_score_bwd_dir* dirs, int32_t n_dirs, int32_t D, float inv_t, float shift,
                      const float* d_loss, float scale, tt_stream stream) {
  return bwd_bf16(ctx, dirs, nullptr, n_dirs, D, inv_t, shift, d_loss, scale, stream, "tt_score_bwd_bf16");
}

int tt_score_bwd_bf16_lq(tt_ctx* ctx, const tt_score_bwd_dir* dirs, const tt_score_bwd_lq* lq, int32_t n_dirs, int32_t D,
                         float inv_t, float shift, const float* d_loss, float scale, tt_stream stream) {
  TT_CHECK_ARG(lq, "tt_score_bwd_bf16_lq: NULL lq");
  return bwd_bf16(ctx, dirs, lq, n_dirs, D, inv_t, shift, d_loss, scale, stream, "tt_score_bwd_bf16_lq");
}

int tt_score_bwd_bf16_mask(tt_ctx* ctx, const tt_score_bwd_dir* dirs, const int32_t* ent_n, const int32_t* ent_c,
                           const tt_score_bwd_lq* lq, int32_t n_dirs, int32_t D, float inv_t, float shift, const float* d_loss,
                           float scale, tt_stream stream) {
  TT_CHECK_ARG(ent_n && ent_c, "tt_score_bwd_bf16_mask: ent_n / ent_c NULL or not 16-byte aligned");
  SquareTerms t{"the repeated-entity mask covers"};
  t.ent_n = ent_n; t.ent_c = ent_c;
  return bwd_square_terms(ctx, dirs, t, lq, n_dirs, D, inv_t, shift, d_loss, scale, stream, "tt_score_bwd_bf16_mask");
}

int tt_score_bwd_bf16_pw(tt_ctx* ctx, const tt_score_bwd_dir* dirs, const float* g, const int32_t* ent_n, const int32_t* ent_c,
                         const tt_score_bwd_lq* lq, int32_t n_dirs, int32_t D, float inv_t, float shift, const float* d_loss,
                         float scale, tt_stream stream) {
  TT_CHECK_ARG(g, "tt_score_bwd_bf16_pw: NULL g");
  SquareTerms t{"pair weights cover"};
  t.g = g; t.ent_n = ent_n; t.ent_c = ent_c;
  return bwd_square_terms(ctx, dirs, t, lq, n_dirs, D, inv_t, shift, d_loss, scale, stream, "tt_score_bwd_bf16_pw");
}

int tt_score_bwd_bf16_xneg(tt_ctx* ctx, const void* N_packed, const void* X_packed, int64_t B, int64_t M, int32_t D, float inv_t,
                           float shift, float ab_scale, const float* inv_row, const float* w_x, const int32_t* ent_c,
                           const int32_t* ent_x, const float* d_loss, float scale, float* dN, float* dX, tt_stream stream) {
  return bwd_bf16_xneg(ctx, N_packed, X_packed, B, M, D, inv_t, shift, ab_scale, inv_row, w_x, ent_c, ent_x, d_loss, scale, dN, dX, stream,
                       "tt_score_bwd_bf16_xneg");
}

int tt_score_bwd_bf16_cells(tt_ctx* ctx, const tt_score_bwd_dir* dirs, const int32_t* plan, int64_t capacity, const tt_score_bwd_lq* lq,
                            const void* X_packed, int64_t M, const float* inv_row, const float* w_x, float* dX, int32_t D, float inv_t, float shift,
                            const float* d_loss, float scale, tt_stream stream) {
  TT_CHECK_ARG(plan && tt_aligned(plan, 16), "tt_score_bwd_bf16_cells: plan NULL or not 16-byte aligned");
  TT_CHECK_ARG(capacity >= 1 && capacity < ((int64_t)1 << 30), "tt_score_bwd_bf16_cells: bad capacity %lld", (long long)capacity);
  SquareTerms t{"masked cells cover"};
  t.plan = plan; t.capacity = capacity; t.M = M; t.X_packed = X_packed; t.inv_row = inv_row; t.w_x = w_x; t.dX = dX;
  return bwd_square_terms(ctx, dirs, t, lq, 2, D, inv_t, shift, d_loss, scale, stream, "tt_score_bwd_bf16_cells");
}

int tt_score_bwd_fp8(tt_ctx* ctx, const tt_score_bwd_dir* dirs, int32_t n_dirs, int32_t D, float inv_t, float shift,
                     const float* d_loss, float scale, tt_stream stream) {
  BwdSetup s;
  if (int rc = bwd_setup(s, Operands::fp8, ctx, dirs, nullptr, n_dirs, D, inv_t, shift, d_loss, scale, "tt_score_bwd_fp8")) return rc;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int Dp = padded_d8(D);
  // D = 256: two waves per SIMD, one a tile each (the 128 accumulator registers of a 32 x 256 block leave room for nothing
  // more); narrower: one wave per SIMD with two a tiles.
  int rc;
  if (ctx->fp8_grad)                                       // TT_OPT_FP8_GRAD (default): e4m3 gradient products, block-scaled weights
    rc = Dp == 64 ? launch_rows8<4, 2, 4>(ctx, s, st) : Dp == 128 ? launch_rows8<8, 2, 4>(ctx, s, st) : launch_rows8<16, 1, 8>(ctx, s, st);
  else
    rc = Dp == 64    ? launch_rows<4, true, 2, 4>(ctx, s, st)
         : Dp == 128 ? launch_rows<8, true, 2, 4>(ctx, s, st) : launch_rows<16, true, 1, 8>(ctx, s, st);
  if (rc) return rc;
  TT_LAUNCH_CHECK();
  return TT_OK;
}

// ---- bf16x3 (split-bf16) operands: [hi image | lo image] packings, three bf16 MFMAs per product ------------------------
int tt_score_fwd_bf16x3(tt_ctx* ctx, const tt_score_fwd_dir* dirs, int32_t n_dirs, int32_t D, float inv_t, float shift,
                        tt_stream stream) {
  return fwd_bf16(ctx, dirs, n_dirs, D, inv_t, shift, stream, true, "tt_score_fwd_bf16x3");
}

int tt_score_bwd_bf16x3(tt_ctx* ctx, const tt_score_bwd_dir* dirs, int32_t n_dirs, int32_t D, float inv_t, float shift,
                        const float* d_loss, float scale, tt_stream stream) {
  return bwd_bf16x3(ctx, dirs, nullptr, n_dirs, D, inv_t, shift, d_loss, scale, stream, "tt_score_bwd_bf16x3");
}

int tt_score_bwd_bf16x3_lq(tt_ctx* ctx, const tt_score_bwd_dir* dirs, const tt_score_bwd_lq* lq, int32_t n_dirs, int32_t D,
                           float inv_t, float shift, const float* d_loss, float scale, tt_stream stream) {
  TT_CHECK_ARG(lq, "tt_score_bwd_bf16x3_lq: NULL lq");
  return bwd_bf16x3(ctx, dirs, lq, n_dirs, D, inv_t, shift, d_loss, scale, stream, "tt_score_bwd_bf16x3_lq");
}

#ifdef TT_POST_STAMPS
int tt_debug_post_stamps(unsigned long long* host_out /* [512 * 16] */) {
  return hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_post_stamps), sizeof(unsigned long long) * 512 * 16, 0, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -2;
}
#endif

}  // extern "C"
