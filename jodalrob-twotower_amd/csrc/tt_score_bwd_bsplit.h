// The b-split backward kernels of the bf16 score path -- score_bwd_bf16_kernel (the square problem) and score_bwd_xneg_kernel (the
// extras' two rectangular directions) -- with the MFMA chains they share with the forward.  A header because two translation units
// instantiate them: tt_score_bf16.hip every form it launched before, tt_score_cells.hip the masked-cells (KP) forms.  Kept apart on
// purpose: the kernels of tt_score_bf16.hip sit at occupancy steps and hipcc's register allocation of one moves when another
// instantiation joins its module (profiles/NOTES.md, "masked cells").  In an unnamed namespace, as the kernels were.
#pragma once
#include "tt_score_bwd_parts.h"

namespace {

template <int KS, int AT>
__device__ __forceinline__ void mfma1(const bf16x8 (&bf)[KS], const bf16x8 (&ares)[AT][KS], f32x16 (&acc)[AT]) {
#pragma unroll
  for (int i = 0; i < AT; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
#pragma unroll
  for (int s = 0; s < KS; ++s)
#pragma unroll
    for (int i = 0; i < AT; ++i) acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bf[s], ares[i][s], acc[i], 0, 0, 0);
}

// bf16x3: S tile = hi_b lo_a + lo_b hi_a + hi_b hi_a, three chains into ONE accumulator in this fixed order (the small
// correction terms first).  The same order in every x3 kernel: the forward, the sym forward and the backward recompute
// bit-identical S tiles.  X3 = false: mfma1.
template <int KS, int AT, bool X3>
__device__ __forceinline__ void mfma_s(const bf16x8 (&bh)[KS], const bf16x8 (&bl)[X3 ? KS : 1], const bf16x8 (&ah)[AT][KS],
                                       const bf16x8 (&al)[AT][X3 ? KS : 1], f32x16 (&acc)[AT]) {
  if constexpr (!X3) {
    mfma1<KS, AT>(bh, ah, acc);
  } else {
#pragma unroll
    for (int i = 0; i < AT; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
#pragma unroll
    for (int s = 0; s < KS; ++s)
#pragma unroll
      for (int i = 0; i < AT; ++i) acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bh[s], al[i][s], acc[i], 0, 0, 0);
#pragma unroll
    for (int s = 0; s < KS; ++s)
#pragma unroll
      for (int i = 0; i < AT; ++i) acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bl[s], ah[i][s], acc[i], 0, 0, 0);
#pragma unroll
    for (int s = 0; s < KS; ++s)
#pragma unroll
      for (int i = 0; i < AT; ++i) acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bh[s], ah[i][s], acc[i], 0, 0, 0);
  }
}

// ---- backward --------------------------------------------------------------------------------------
// One tile's worth of streamed operands: the b tile's fragments for the first product, its fragment-ordered image for the
// second, and the 16 softmax reciprocals (or exp-sums) of its rows this lane half needs.
// X3: the lo images' fragments as well (bl, bml).
// LQ: the 16 sampling weights of those rows as well (wv).
// MK: their 16 notice ids and 16 company ids as well (en, ec).
template <int KS, bool X3 = false, bool LQ = false, bool MK = false>
struct BwdTile {
  static constexpr int KL = X3 ? KS : 1, DL = X3 ? KS / 2 : 1;
  bf16x8 b[KS];
  bf16x8 bl[KL];
  bf16x8 bm[2][KS / 2];
  bf16x8 bml[2][DL];
  float4 iv[4];
  float4 wv[LQ ? 4 : 1];
  int4 en[MK ? 4 : 1], ec[MK ? 4 : 1];
};

template <int KS, bool X3, bool LQ, bool MK = false>
__device__ __forceinline__ void bwd_tile_load(BwdTile<KS, X3, LQ, MK>& T, const __bf16* __restrict__ b_rows, const __bf16* __restrict__ b_frag,
                                              const float* __restrict__ ivsrc, int t, int c, int h,
                                              const __bf16* __restrict__ b_lo = nullptr, const __bf16* __restrict__ b_frag_lo = nullptr,
                                              const float* __restrict__ wsrc = nullptr, const int32_t* __restrict__ ensrc = nullptr,
                                              const int32_t* __restrict__ ecsrc = nullptr) {
  constexpr int Dp = KS * 16, DT = KS / 2;
  load_bfrag<KS>(b_rows, t, c, h, T.b);
  if constexpr (X3) load_bfrag<KS>(b_lo, t, c, h, T.bl);
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int d = 0; d < DT; ++d) {
      const int64_t o = ((((int64_t)t * 2 + s) * 2 + h) * Dp + 32 * d + c) * 8;
      T.bm[s][d] = *reinterpret_cast<const bf16x8*>(b_frag + o);
      if constexpr (X3) T.bml[s][d] = *reinterpret_cast<const bf16x8*>(b_frag_lo + o);
    }
#pragma unroll
  for (int q = 0; q < 4; ++q) T.iv[q] = *reinterpret_cast<const float4*>(ivsrc + 32 * t + 4 * h + 8 * q);
  if constexpr (LQ) {
#pragma unroll
    for (int q = 0; q < 4; ++q) T.wv[q] = *reinterpret_cast<const float4*>(wsrc + 32 * t + 4 * h + 8 * q);
  }
  if constexpr (MK) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      T.en[q] = *reinterpret_cast<const int4*>(ensrc + 32 * t + 4 * h + 8 * q);
      T.ec[q] = *reinterpret_cast<const int4*>(ecsrc + 32 * t + 4 * h + 8 * q);
    }
  }
}

// Structure of the tile loop: TWO operand buffers, the loop unrolled over them, every load issued unconditionally (past the
// wave's last tile: that tile again) and in a fixed order.  The first version prefetched under `if (t + NW < nT)` and loaded
// the reciprocals inside the tile body: hipcc then cannot count the loads in flight and drained them all (s_waitcnt
// vmcnt(0)) twice per tile -- the prefetch never overlapped anything and the kernel ran at a third of its issue rate.
// The per-row reciprocal arrays must be readable up to a multiple of 32 rows (tt_score_bwd_dir).
// X3 (tt_score_bwd_bf16x3): S recomputed with mfma_s from the hi / lo images; the f32 softmax weights are split in registers,
// w_hi = bf16(w), w_lo = bf16(w - w_hi), and dA += w_hi B_lo + w_lo B_hi + w_hi B_hi (in this order, per b tile).
// LQ (tt_score_bwd_bf16_lq): the weight of (a, b) is e_ab (w_b / rowsum_a + w_a / colsum_b) with the sampling weights w of the
// two rows -- one multiply more per element than e_ab (1 / rowsum_a + 1 / colsum_b).
// MK (tt_score_bwd_bf16_mask; square problems, bf16 operands): a pair whose rows share a notice or a company id weighs nothing
// (softmax_term); the b tile's ids travel with its operands, a tile ahead -- at D = 256 they are loaded behind the S product, as the
// LQ weights are there.  One wave per SIMD in every masked instantiation (launch_bsplit_mk): the ids of two tiles in flight are
// 64 registers more.
// PW (tt_score_bwd_bf16_pw; square problems, bf16 operands): per-pair sample weights.  inv_a / inv_b are the weighted forward's
// folded reciprocals g / sum, so every off-diagonal weight is right as softmax_term forms it; the only new work is the diagonal,
// -2 g_a in place of -2 (before the weight is rounded to bf16), g_a one more value loaded at the a rows' setup.
// KP (tt_score_bwd_bf16_cells; square problems, bf16 operands): masked cells.  Per (a tile, b tile) the wave reads the tile pair's two
// plan offsets and walks a non-empty span into one 16-bit mask per lane (tt_cells_mask); a listed pair gets zero weight behind
// softmax_term, in both directions -- direction 1 (the company rows' gradient) reads the pair (b tile, a tile) with its coordinates
// swapped.  The plan holds no diagonal cell.  One b tile in flight at D = 256, as MK and PW.
template <int KS, int AT, int NW, bool UNIT, bool X3 = false, bool LQ = false, bool MK = false, bool PW = false, bool KP = false>
__global__ __launch_bounds__(NW * 64) void score_bwd_bf16_kernel(std::conditional_t<KP, BwdArgsKP, BwdArgs> args) {
  constexpr int Dp = KS * 16, ROWS = 32 * AT, DT = KS / 2, KL = X3 ? KS : 1;
  static_assert(!MK || !X3, "the repeated-entity mask: bf16 operands only");
  static_assert(!PW || !X3, "pair weights: bf16 operands only");
  static_assert(!KP || (!X3 && !MK && !PW), "masked cells: bf16 operands only, on their own");
  __shared__ float red[(NW / 2) * ROWS * Dp];
  // (this kernel's own copy of select_dir, a_row_setup and zero_acc, and its own sweep, tree and store: through the parts its
  //  D = 256 instantiations change their scratch size, and the forward's registers move with them -- profiles/NOTES.md)
  const bool d1 = blockIdx.y != 0;
  DirBwd dr;
  dr.a_rows = d1 ? args.d[1].a_rows : args.d[0].a_rows;
  dr.b_rows = d1 ? args.d[1].b_rows : args.d[0].b_rows;
  dr.b_frag = d1 ? args.d[1].b_frag : args.d[0].b_frag;
  dr.a_lo = d1 ? args.d[1].a_lo : args.d[0].a_lo;
  dr.b_lo = d1 ? args.d[1].b_lo : args.d[0].b_lo;
  dr.b_frag_lo = d1 ? args.d[1].b_frag_lo : args.d[0].b_frag_lo;
  dr.sumexp_a = d1 ? args.d[1].sumexp_a : args.d[0].sumexp_a;
  dr.sumexp_b = d1 ? args.d[1].sumexp_b : args.d[0].sumexp_b;
  dr.dA = d1 ? args.d[1].dA : args.d[0].dA;
  const float c1 = d1 ? args.d[1].c1 : args.d[0].c1, out_scale = d1 ? args.d[1].out_scale : args.d[0].out_scale;
  const float* const inv_a = d1 ? args.d[1].inv_a : args.d[0].inv_a;
  const float* const inv_b = d1 ? args.d[1].inv_b : args.d[0].inv_b;
  const float* const wt_a = d1 ? args.wt_a[1] : args.wt_a[0];     // (LQ)
  const float* const wt_b = d1 ? args.wt_b[1] : args.wt_b[0];
  const float c2 = args.c2, kx = UNIT ? args.kexp : 1.f;     // without the forward's reciprocals: 1 / raw sum = 2^c2 / stored sum
  const int Ra = (int)(d1 ? args.d[1].Ra : args.d[0].Ra), Rb = (int)(d1 ? args.d[1].Rb : args.d[0].Rb);
  const int off = (int)(d1 ? args.d[1].off : args.d[0].off);
  const int a0 = (int)blockIdx.x * ROWS;
  if (a0 >= Ra) return;
  const int lane = threadIdx.x & 63, c = lane & 31, h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nT = (Rb + 31) / 32;
  bf16x8 ares[AT][KS], ares_lo[AT][KL];
  float ia[AT], ua[AT];
  int pos[AT];
  [[maybe_unused]] int ean[AT], eac[AT];                       // (MK) the a rows' notice / company ids
  [[maybe_unused]] float ga[AT];                               // (PW) the a rows' pair weights
#pragma unroll
  for (int i = 0; i < AT; ++i) {
    load_bfrag<KS>(dr.a_rows, a0 / 32 + i, c, h, ares[i]);
    if (X3) load_bfrag<KL>(dr.a_lo, a0 / 32 + i, c, h, ares_lo[i]);
    const int a = a0 + 32 * i + c;
    ia[i] = a < Ra ? (inv_a ? inv_a[a] : __builtin_amdgcn_rcpf(dr.sumexp_a[a]) * kx) : 0.f;
    if constexpr (LQ) ua[i] = a < Ra ? wt_a[a] : 0.f;
    if constexpr (MK) { ean[i] = a < Ra ? args.ent_n[a] : 0; eac[i] = a < Ra ? args.ent_c[a] : 0; }
    if constexpr (PW) ga[i] = a < Ra ? args.pw_g[a] : 0.f;
    pos[i] = a + off;
  }
  const int posmin = a0 + off, posmax = a0 + ROWS - 1 + off;
  f32x16 dacc[AT][DT];
#pragma unroll
  for (int i = 0; i < AT; ++i)
#pragma unroll
    for (int d = 0; d < DT; ++d)
#pragma unroll
      for (int r = 0; r < 16; ++r) dacc[i][d][r] = 0.f;
  const bool have_inv = inv_b != nullptr;                      // wave-uniform
  const float* const ivsrc = have_inv ? inv_b : dr.sumexp_b;
  const int tlast = nT - 1;
  constexpr bool WLATE = LQ && KS == 16;                       // LQ, D = 256: weights loaded behind the S product, not a tile ahead
  constexpr bool ELATE = MK && KS == 16;                       // MK, D = 256: the ids likewise
  [[maybe_unused]] const int32_t* const ent_n = args.ent_n;
  [[maybe_unused]] const int32_t* const ent_c = args.ent_c;
  auto compute = [&](const BwdTile<KS, X3, LQ && !WLATE, MK && !ELATE>& T, int t) {
    const int b_lo = 32 * t;
    float ib[16], wb[16];
    [[maybe_unused]] int ebn[16], ebc[16];                     // (MK) the b rows' ids, in the accumulator's row order
    if constexpr (MK && !ELATE) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        ebn[4 * q] = T.en[q].x; ebn[4 * q + 1] = T.en[q].y; ebn[4 * q + 2] = T.en[q].z; ebn[4 * q + 3] = T.en[q].w;
        ebc[4 * q] = T.ec[q].x; ebc[4 * q + 1] = T.ec[q].y; ebc[4 * q + 2] = T.ec[q].z; ebc[4 * q + 3] = T.ec[q].w;
      }
    }
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
    if (b_lo + 31 >= Rb) {                                     // the ragged last tile: rows past the end weigh nothing
#pragma unroll
      for (int r = 0; r < 16; ++r) ib[r] = b_lo + rowmap(r, h) < Rb ? ib[r] : 0.f;
    }
    const bool band = !(b_lo + 31 < posmin || b_lo > posmax);
#pragma unroll
    for (int i = 0; i < AT; ++i) {
      f32x16 acc;
      if constexpr (X3) {
        f32x16 a1[1];
        mfma_s<KS, 1, true>(T.b, T.bl, reinterpret_cast<const bf16x8(&)[1][KS]>(ares[i]), reinterpret_cast<const bf16x8(&)[1][KL]>(ares_lo[i]), a1);
        acc = a1[0];
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
        for (int s = 0; s < KS; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(T.b[s], ares[i][s], acc, 0, 0, 0);
      }
      if constexpr (WLATE) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float4 v = *reinterpret_cast<const float4*>(wt_b + b_lo + 4 * h + 8 * q);
          wb[4 * q] = v.x; wb[4 * q + 1] = v.y; wb[4 * q + 2] = v.z; wb[4 * q + 3] = v.w;
        }
      }
      if constexpr (ELATE) {
        if (i == 0) {
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int4 vn = *reinterpret_cast<const int4*>(ent_n + b_lo + 4 * h + 8 * q);
            const int4 vc = *reinterpret_cast<const int4*>(ent_c + b_lo + 4 * h + 8 * q);
            ebn[4 * q] = vn.x; ebn[4 * q + 1] = vn.y; ebn[4 * q + 2] = vn.z; ebn[4 * q + 3] = vn.w;
            ebc[4 * q] = vc.x; ebc[4 * q + 1] = vc.y; ebc[4 * q + 2] = vc.z; ebc[4 * q + 3] = vc.w;
          }
        }
      }
      float w[16];
      if constexpr (MK) {
        if (band) {                                            // the tile(s) of the positives: the diagonal is never masked
#pragma unroll
          for (int r = 0; r < 16; ++r)
            w[r] = softmax_term<UNIT, LQ, true>(acc[r], c1, c2, ia[i], ua[i], ib[r], wb[r],
                                                same_entity(ean[i], eac[i], ebn[r], ebc[r]) && b_lo + rowmap(r, h) != pos[i]);
        } else {
#pragma unroll
          for (int r = 0; r < 16; ++r)
            w[r] = softmax_term<UNIT, LQ, true>(acc[r], c1, c2, ia[i], ua[i], ib[r], wb[r], same_entity(ean[i], eac[i], ebn[r], ebc[r]));
        }
      } else {
#pragma unroll
      for (int r = 0; r < 16; ++r)
        w[r] = softmax_term<UNIT, LQ>(acc[r], c1, c2, ia[i], ua[i], ib[r], wb[r]);
      }
      if constexpr (KP) {                                      // direction 0: (notice tile, company tile) = (a tile, b tile)
        const int ta = a0 / 32 + i;
        const unsigned km = 32 * ta < Ra ? tt_cells_mask(args.kp, d1 ? t : ta, d1 ? ta : t, c, h, d1) : 0u;   // (AT = 2: a tile past the end)
        if (__builtin_amdgcn_ballot_w64(km != 0)) {
#pragma unroll
          for (int r = 0; r < 16; ++r) w[r] = (km >> r) & 1u ? 0.f : w[r];
        }
      }
      if (b_lo + 31 >= Rb) {
#pragma unroll
        for (int r = 0; r < 16; ++r) w[r] = b_lo + rowmap(r, h) < Rb ? w[r] : 0.f;
      }
      if (band) {
        if constexpr (PW) {
#pragma unroll
          for (int r = 0; r < 16; ++r)
            if (b_lo + rowmap(r, h) == pos[i]) w[r] = __builtin_fmaf(-2.f, ga[i], w[r]);
        } else {
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (b_lo + rowmap(r, h) == pos[i]) w[r] -= 2.f;
        }
      }
      bf16x8 wf[2], wl[2];
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          wf[s][j] = (__bf16)w[8 * s + j];
          if (X3) wl[s][j] = (__bf16)sub_nc(w[8 * s + j], (float)wf[s][j]);
        }
      if constexpr (X3) {
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
          for (int d = 0; d < DT; ++d) dacc[i][d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[s], T.bml[s][d], dacc[i][d], 0, 0, 0);
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
          for (int d = 0; d < DT; ++d) dacc[i][d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wl[s], T.bm[s][d], dacc[i][d], 0, 0, 0);
      }
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int d = 0; d < DT; ++d) dacc[i][d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[s], T.bm[s][d], dacc[i][d], 0, 0, 0);
    }
  };
  BwdTile<KS, X3, LQ && !WLATE, MK && !ELATE> T0, T1;
  if constexpr ((X3 || MK || PW || KP) && KS == 16) {          // x3 / MK / PW / KP, D = 256: one tile in flight (x3: two are 544 registers;
                                                               // PW without ids: two spilled 20-36 bytes per lane, as the plain form does)
    for (int t = wave; t < nT; t += NW) {
      bwd_tile_load<KS, X3, LQ && !WLATE>(T0, dr.b_rows, dr.b_frag, ivsrc, t, c, h, dr.b_lo, dr.b_frag_lo, wt_b, ent_n, ent_c);
      compute(T0, t);
    }
  } else {
  bwd_tile_load<KS, X3, LQ && !WLATE>(T0, dr.b_rows, dr.b_frag, ivsrc, min(wave, tlast), c, h, dr.b_lo, dr.b_frag_lo, wt_b, ent_n, ent_c);
  __builtin_amdgcn_sched_barrier(0);                           // (issue order pinned: see the forward kernels)
  for (int t = wave; t < nT; t += 2 * NW) {
    bwd_tile_load<KS, X3, LQ && !WLATE>(T1, dr.b_rows, dr.b_frag, ivsrc, min(t + NW, tlast), c, h, dr.b_lo, dr.b_frag_lo, wt_b, ent_n, ent_c);
    compute(T0, t);
    bwd_tile_load<KS, X3, LQ && !WLATE>(T0, dr.b_rows, dr.b_frag, ivsrc, min(t + 2 * NW, tlast), c, h, dr.b_lo, dr.b_frag_lo, wt_b, ent_n, ent_c);
    if (t + NW < nT) compute(T1, t + NW);
  }
  }
  // fixed-order tree over the NW waves: upper half writes, lower half adds
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
    const float g = args.d_loss[0] * out_scale;
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

// ---- backward of the shared extra negatives (tt_score_bwd_bf16_xneg): the b-split form over two RECTANGULAR directions ------------
// Direction 0: the notice rows a against the extras m -> dN's extra term (added to what the square backward stored); direction 1: the
// extras against the notice rows -> dX.  The weight of (a, m) is the one-sided case of softmax_term, e_am w_x[m] / rowsum_a: the
// extras stand in no column sum, so there is no second reciprocal and nothing is loaded for it.  Per direction fa is the per-row
// factor of its A rows and fb that of its B rows (direction 0: the forward's inv_row and w_x, direction 1 the other way round): the
// weight is e fa fb in both.  No positive.  MK: a pair is masked iff the notice row's company id equals the extra's (ea / eb, loaded
// behind the S product as ELATE does).  Sweep, tree and store as score_bwd_bf16_kernel's.
struct XnegDir {
  const __bf16* a_rows;
  const __bf16* b_rows;
  const __bf16* b_frag;
  int Ra, Rb;
  const float* fa;     // [Ra]
  const float* fb;     // [round_up(Rb, 32)], 16-byte aligned
  const int32_t* ea;   // (MK) [Ra]
  const int32_t* eb;   // (MK) [round_up(Rb, 32)], 16-byte aligned
  float* dA;
  float out_scale;
  int accumulate;      // dA += instead of dA =
};
struct XnegArgs {
  XnegDir d[2];
  float c1, c2;
  const float* d_loss;
  int D;
};
struct XnegArgsKP : XnegArgs {   // (KP; a type of its own, as BwdArgsKP)
  TtCellsPlan kp;      // the masked cells' plan; nT: the in-batch tiles, in front of the extras' in its column index
  int nT;
};

// KP (tt_score_bwd_bf16_cells): the extras' cells of the plan -- direction 0 reads tile pair (a tile, nT + b tile), direction 1
// (nT + a tile's pair of the b tile) with its coordinates swapped; a listed pair weighs nothing.
template <int KS, int AT, int NW, bool UNIT, bool MK, bool KP = false>
__global__ __launch_bounds__(NW * 64) void score_bwd_xneg_kernel(std::conditional_t<KP, XnegArgsKP, XnegArgs> args) {
  constexpr int Dp = KS * 16, ROWS = 32 * AT, DT = KS / 2;
  __shared__ float red[(NW / 2) * ROWS * Dp];
  const bool d1 = blockIdx.y != 0;
  const __bf16* const a_rows = d1 ? args.d[1].a_rows : args.d[0].a_rows;
  const __bf16* const b_rows = d1 ? args.d[1].b_rows : args.d[0].b_rows;
  const __bf16* const b_frag = d1 ? args.d[1].b_frag : args.d[0].b_frag;
  const float* const fa = d1 ? args.d[1].fa : args.d[0].fa;
  const float* const fb = d1 ? args.d[1].fb : args.d[0].fb;
  [[maybe_unused]] const int32_t* const ea = d1 ? args.d[1].ea : args.d[0].ea;
  [[maybe_unused]] const int32_t* const eb = d1 ? args.d[1].eb : args.d[0].eb;
  float* const dA = d1 ? args.d[1].dA : args.d[0].dA;
  const float out_scale = d1 ? args.d[1].out_scale : args.d[0].out_scale;
  const bool accumulate = (d1 ? args.d[1].accumulate : args.d[0].accumulate) != 0;
  const int Ra = d1 ? args.d[1].Ra : args.d[0].Ra, Rb = d1 ? args.d[1].Rb : args.d[0].Rb;
  const float c1 = args.c1, c2 = args.c2;
  const int a0 = (int)blockIdx.x * ROWS;
  if (a0 >= Ra) return;
  const int lane = threadIdx.x & 63, c = lane & 31, h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nT = (Rb + 31) / 32;
  bf16x8 ares[AT][KS];
  float ia[AT];
  [[maybe_unused]] int eaa[AT];
#pragma unroll
  for (int i = 0; i < AT; ++i) {
    load_bfrag<KS>(a_rows, a0 / 32 + i, c, h, ares[i]);
    const int a = a0 + 32 * i + c;
    ia[i] = a < Ra ? fa[a] : 0.f;
    if constexpr (MK) eaa[i] = a < Ra ? ea[a] : 0;
  }
  f32x16 dacc[AT][DT];
  zero_acc(dacc);
  const int tlast = nT - 1;
  auto compute = [&](const BwdTile<KS>& T, int t) {
    const int b_lo = 32 * t;
    float ib[16];
#pragma unroll
    for (int q = 0; q < 4; ++q) { ib[4 * q] = T.iv[q].x; ib[4 * q + 1] = T.iv[q].y; ib[4 * q + 2] = T.iv[q].z; ib[4 * q + 3] = T.iv[q].w; }
    if (b_lo + 31 >= Rb) {                                     // the ragged last tile: rows past the end weigh nothing
#pragma unroll
      for (int r = 0; r < 16; ++r) ib[r] = b_lo + rowmap(r, h) < Rb ? ib[r] : 0.f;
    }
    [[maybe_unused]] int ebb[16];
#pragma unroll
    for (int i = 0; i < AT; ++i) {
      f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
      for (int s = 0; s < KS; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(T.b[s], ares[i][s], acc, 0, 0, 0);
      if constexpr (MK) {
        if (i == 0) {
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int4 v = *reinterpret_cast<const int4*>(eb + b_lo + 4 * h + 8 * q);
            ebb[4 * q] = v.x; ebb[4 * q + 1] = v.y; ebb[4 * q + 2] = v.z; ebb[4 * q + 3] = v.w;
          }
        }
      }
      float w[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float e = UNIT ? __builtin_amdgcn_exp2f(acc[r]) : __builtin_amdgcn_exp2f(__builtin_fmaf(acc[r], c1, c2));
        w[r] = e * (ia[i] * ib[r]);
        if constexpr (MK) w[r] = eaa[i] == ebb[r] ? 0.f : w[r];
      }
      if constexpr (KP) {
        const int ta = a0 / 32 + i;
        const unsigned km = 32 * ta < Ra ? tt_cells_mask(args.kp, d1 ? t : ta, args.nT + (d1 ? ta : t), c, h, d1) : 0u;
        if (__builtin_amdgcn_ballot_w64(km != 0)) {
#pragma unroll
          for (int r = 0; r < 16; ++r) w[r] = (km >> r) & 1u ? 0.f : w[r];
        }
      }
      bf16x8 wf[2];
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int j = 0; j < 8; ++j) wf[s][j] = (__bf16)w[8 * s + j];
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int d = 0; d < DT; ++d) dacc[i][d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[s], T.bm[s][d], dacc[i][d], 0, 0, 0);
    }
  };
  BwdTile<KS> T0, T1;
  if constexpr (KS == 16) {                                    // D = 256: one tile in flight, as the masked square form
    for (int t = wave; t < nT; t += NW) {
      bwd_tile_load<KS, false, false>(T0, b_rows, b_frag, fb, t, c, h);
      compute(T0, t);
    }
  } else {
    bwd_tile_load<KS, false, false>(T0, b_rows, b_frag, fb, min(wave, tlast), c, h);
    __builtin_amdgcn_sched_barrier(0);
    for (int t = wave; t < nT; t += 2 * NW) {
      bwd_tile_load<KS, false, false>(T1, b_rows, b_frag, fb, min(t + NW, tlast), c, h);
      compute(T0, t);
      bwd_tile_load<KS, false, false>(T0, b_rows, b_frag, fb, min(t + 2 * NW, tlast), c, h);
      if (t + NW < nT) compute(T1, t + NW);
    }
  }
  // fixed-order tree over the NW waves: upper half writes, lower half adds
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
    const float g = args.d_loss[0] * out_scale;
#pragma unroll
    for (int i = 0; i < AT; ++i)
#pragma unroll
      for (int d = 0; d < DT; ++d)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int a = a0 + 32 * i + rowmap(r, h);
          const int dd = 32 * d + c;
          if (a < Ra && dd < args.D) {
            float* const p = dA + (int64_t)a * args.D + dd;
            const float v = dacc[i][d][r] * g;
            *p = accumulate ? *p + v : v;                      // (dN: the square backward's term first, then this one)
          }
        }
  }
}

}  // namespace
