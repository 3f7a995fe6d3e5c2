// The backward head of the towers' fused narrow tail as ONE device body with two hosts (as tt_riders.h does for the riders):
// tail_bwd_kernel (tt_tower.hip: 1024-thread workgroups, d_emb read from global memory) and score_bwd_tr_kernel<4, 2, UNIT, false, true>
// (tt_score_bf16.hip: the score backward's 512-thread workgroups, whose flat final reduction leaves every thread the 8 values of
// d_emb the head wants from it, in registers -- no kernel boundary, no 4 MB round trip).  Only the elementwise phases depend on the thread count
// (thread (c, rq) owns rows rq + NT / 64 * j); everything whose order matters -- the two MFMA chains, the cs column sums, the
// ordered S1 / S2 sums, the sh[.][0..3] merges -- runs in the first four waves in one fixed order: bit-identical results.
#pragma once
#include "tt_common.h"

// measurement aid: a host built with phase stamps (tt_score_bf16.hip under -DTT_POST_STAMPS) defines TT_HEAD_STAMP in front of this
// header; the head then stamps behind each of its barriers
#ifndef TT_HEAD_STAMP
#define TT_HEAD_STAMP(i) do { } while (0)
#endif

namespace tttail {

constexpr float kNormEps = 1e-12f;

__device__ __forceinline__ float dropout_scale(bool on, float p, uint64_t seed, uint64_t idx) {
  if (!on) return 1.f;
  return tt_uniform01(seed, idx) >= p ? 1.f / (1.f - p) : 0.f;
}
__device__ __forceinline__ uint64_t seed_of(uint64_t seed, const uint64_t* seed_dev) { return seed_dev ? seed + seed_dev[0] : seed; }

template <typename A>
struct Batch {
  A a[TT_MAX_SIDES];
};

// ---- deterministic two-stage column sums of the BatchNorm backward ------------------------------
//   da = d_act * dropscale ; xhat from pre ; S1 = sum da, S2 = sum da * xhat
struct ColArgs {
  const float* x; int64_t ldx;
  const float* pre; const float* mean; const float* rstd;
  uint64_t salt;
  int B, H, rows_per_chunk, nchunks;
  float* partial; float* out0; float* out1;
  int64_t pstride = 0;   // floats between chunks when READING partial (0 = 2 * H)
  float out_scale = 1.f; // colsum_finish_kernel: S1 / S2 are stored times this (1 / ranks under SyncBN); the raw sums go to sums_raw
  float* sums_raw = nullptr;   // optional [2 * H]: the unscaled S1 | S2 for bn_bwd_apply_kernel
};

// a product that is rounded on its own (HIP's __fmul_rn is a plain `*`, which the compiler still contracts)
__device__ __forceinline__ float mul_rn(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}

using tl_f32x16 = __attribute__((ext_vector_type(16))) float;
using tl_bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
constexpr int kTailLd = 72;      // bf16 elements per LDS row of a 64-wide operand tile (144 B: aligned 16-B fragments)
constexpr int kTailLdF = 65;     // f32 row stride of the staging tiles

// (C) backward head: L2-normalise backward -> d_y; d_act = d_y . W_out; the chunk's share of the output-layer weight /
// bias gradients (d_y^T . act, column sums of d_y) into slabs; per-chunk BN column sums S1 / S2.  One workgroup per
// row chunk (the chunks of colsum_partial_kernel), 64 rows at a time.  d_act leaves the head already multiplied by
// the dropout scale (tail_bwd_apply_kernel does not regenerate the mask).
struct TailBwdArgs {
  const float* y; const float* emb; const float* d_emb; float* d_y; int D;
  const float* w_out; const float* act; float* d_act;
  ColArgs col;                       // x / ldx unused: d_act is taken from the tile
  float* w_slab; float* b_slab;      // [nchunks][D * H], [nchunks][D]
};

// LDS of the head, from a caller-supplied 16-byte-aligned buffer: dyA [row][d] | dyT [d][row] | (XH f32 tile aliases these two
// once the MFMAs are done) ; Wn [h][d] ; actT [h][row] ; DY (d_y, then d_act, of the 64 rows) ; sh
constexpr int kTailBwdLds = 2 * (2 * 64 * kTailLd) + 2 * (64 * kTailLd) + 2 * (64 * kTailLd) + 4 * (64 * kTailLdF) + 4 * (3 * 4 * 64);
static_assert(sizeof(float) * 64 * kTailLdF <= sizeof(__bf16) * 2 * 64 * kTailLd, "XH must fit over dyA | dyT");

// what a workgroup of NT threads loads for the head: the part that depends on nothing but the launch's arguments ...
template <int NT>
struct TailBwdConst {
  static constexpr int R = 64 * 64 / NT;              // rows (and W_out rows) per thread
  float w[R], mean, rstd;
};
// ... and 64 rows' worth of y, emb (d_emb unless the host brings it), act and pre
template <int NT>
struct TailBwdRows {
  static constexpr int R = 64 * 64 / NT;
  float yv[R], e[R], de[R], av[R], pr[R];
};

template <int NT>
__device__ __forceinline__ void tail_bwd_load_const(const TailBwdArgs& f, TailBwdConst<NT>& k) {
  constexpr int NWV = NT / 64, R = TailBwdConst<NT>::R;
  const int H = f.col.H, D = f.D;
  const int c = threadIdx.x & 63, rq = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < R; ++j) {                         // W_out [D, H]: element (k = d, n = h) -> Wn[h][d]
    const int d = rq + NWV * j;
    k.w[j] = f.w_out[(int64_t)min(d, D - 1) * H + min(c, H - 1)];
  }
  k.mean = c < H ? f.col.mean[c] : 0.f;
  k.rstd = c < H ? f.col.rstd[c] : 0.f;
}

// rows b0 .. b0 + 63 (below r1).  L2 part: one wave per row as l2norm_bwd_kernel, R independent rows per wave in flight;
// act / pre: thread (c, rq), rows rq + NWV j
template <int NT, bool REGS>
__device__ __forceinline__ void tail_bwd_load_rows(const TailBwdArgs& f, int r1, int b0, TailBwdRows<NT>& v) {
  constexpr int NWV = NT / 64, R = TailBwdRows<NT>::R;
  const int H = f.col.H, D = f.D;
  const int c = threadIdx.x & 63, rq = threadIdx.x >> 6;
  const int lane = c, wave = rq;
#pragma unroll
  for (int j = 0; j < R; ++j) {
    const int r = b0 + wave * R + j;
    const bool ok = r < r1 && lane < D;                 // (unconditional loads at clamped addresses: a load under a per-lane
    const int64_t i = (int64_t)min(r, r1 - 1) * D + min(lane, D - 1);   //  condition is waited for before the next is issued)
    const float v0 = f.y[i], v1 = f.emb[i];
    v.yv[j] = ok ? v0 : 0.f;
    v.e[j] = ok ? v1 : 0.f;
    if constexpr (!REGS) {
      const float v2 = f.d_emb[i];
      v.de[j] = ok ? v2 : 0.f;
    }
  }
#pragma unroll
  for (int j = 0; j < R; ++j) {                         // thread (c, rq): rows rq + NWV j of act / pre
    const int r = b0 + rq + NWV * j;
    const bool ok = c < H && r < r1;
    const int64_t i = (int64_t)min(r, r1 - 1) * H + min(c, H - 1);
    const float v0 = f.act[i], v1 = f.col.pre[i];
    v.av[j] = ok ? v0 : 0.f;
    v.pr[j] = ok ? v1 : 0.f;
  }
}

// The head of row chunk `chunk` on a workgroup of NT threads (1024 or 512).  smem: kTailBwdLds bytes.
// REGS: the chunk is 64 rows (rows_per_chunk == 64) and pk / pv were loaded by the caller (tail_bwd_load_const /
// tail_bwd_load_rows<NT, true> of the chunk's rows) -- ahead of whatever it had to wait for --, which also left d_emb in pv->de:
// thread (lane, wave) holds rows wave R + j of column lane, zero past the chunk's last row and past D.  smem is free when the body starts.
template <int NT, bool REGS>
__device__ __forceinline__ void tail_bwd_head(const TailBwdArgs& f, int chunk, bool drop, float p, uint64_t seed, char* smem,
                                              const TailBwdConst<NT>* pk, const TailBwdRows<NT>* pv) {
  static_assert(NT == 1024 || NT == 512, "the ordered parts run in the first four waves; the rest splits 64 rows over NT / 64");
  constexpr int NWV = NT / 64, R = 64 * 64 / NT;
  const ColArgs& a = f.col;
  const int H = a.H, D = f.D;
  __bf16* dy2 = reinterpret_cast<__bf16*>(smem);
  __bf16* Wn = dy2 + 2 * 64 * kTailLd;
  __bf16* actT = Wn + 64 * kTailLd;
  float* DY = reinterpret_cast<float*>(actT + 64 * kTailLd);
  float (*sh)[4][64] = reinterpret_cast<float (*)[4][64]>(DY + 64 * kTailLdF);
  __bf16* dyA = dy2;
  __bf16* dyT = dy2 + 64 * kTailLd;
  float* XH = reinterpret_cast<float*>(dy2);
  const int t = threadIdx.x, c = t & 63, rq = t >> 6;
  const int lane = c, wave = rq;
  const int r0 = chunk * a.rows_per_chunk, r1 = min(a.B, r0 + a.rows_per_chunk);
  TailBwdConst<NT> k;
  if constexpr (REGS) k = *pk;
  else tail_bwd_load_const<NT>(f, k);
#pragma unroll
  for (int j = 0; j < R; ++j) {
    const int d = rq + NWV * j;
    Wn[c * kTailLd + d] = (__bf16)((d < D && c < H) ? k.w[j] : 0.f);
  }
  const float mean = k.mean, rstd = k.rstd;
  tl_f32x16 accw;
#pragma unroll
  for (int i = 0; i < 16; ++i) accw[i] = 0.f;
  float s0 = 0.f, s1 = 0.f, cs = 0.f;
  for (int b0 = r0; b0 < r1; b0 += 64) {
    // 1. d_y of rows b0 .. b0 + 63: one wave per row as l2norm_bwd_kernel, R independent rows per wave in flight
    TailBwdRows<NT> v;
    if constexpr (REGS) {
      v = *pv;
    } else {
      tail_bwd_load_rows<NT, false>(f, r1, b0, v);
    }
    float ss[R], dot[R], xh[R], sc[R];
#pragma unroll
    for (int j = 0; j < R; ++j) {
      ss[j] = mul_rn(v.yv[j], v.yv[j]);
      dot[j] = mul_rn(v.e[j], v.de[j]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
      for (int j = 0; j < R; ++j) {
        ss[j] += __shfl_xor(ss[j], o);
        dot[j] += __shfl_xor(dot[j], o);
      }
    }
#pragma unroll
    for (int j = 0; j < R; ++j) {
      const int row = wave * R + j, r = b0 + row;
      const float nrm = sqrtf(ss[j]);
      const float den = fmaxf(nrm, kNormEps);
      float out = nrm > kNormEps ? (v.de[j] - v.e[j] * dot[j]) / den : v.de[j] / den;
      if (r < r1 && lane < D) f.d_y[(int64_t)r * D + lane] = out;
      else out = 0.f;
      DY[row * kTailLdF + lane] = out;
      dyA[row * kTailLd + lane] = (__bf16)out;
      dyT[lane * kTailLd + row] = (__bf16)out;
    }
#pragma unroll
    for (int j = 0; j < R; ++j) {
      const int row = rq + NWV * j, r = b0 + row;
      actT[c * kTailLd + row] = (__bf16)v.av[j];
      xh[j] = (fmaxf(v.pr[j], 0.f) - mean) * rstd;
      sc[j] = (c < H && r < r1) ? dropout_scale(drop, p, seed, a.salt + (uint64_t)((int64_t)r * H + c)) : 0.f;
    }
    __syncthreads();
    TT_HEAD_STAMP(0);
    // 2. bias-gradient column sums of d_y, data gradient d_act = d_y . W_out, weight-gradient tile += d_y^T . act
    const int wr = (wave >> 1) & 1, wc = wave & 1, li = lane & 31, lh = lane >> 5;
    tl_f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    if (wave < 4) {
      if (c < D) {
#pragma unroll
        for (int j = 0; j < 16; ++j) cs += DY[(rq + 4 * j) * kTailLdF + c];
      }
#pragma unroll
      for (int s2 = 0; s2 < 4; ++s2) {
        const int ko = 16 * s2 + 8 * lh;
        const tl_bf16x8 a1 = *reinterpret_cast<const tl_bf16x8*>(dyA + (wr * 32 + li) * kTailLd + ko);
        const tl_bf16x8 b1 = *reinterpret_cast<const tl_bf16x8*>(Wn + (wc * 32 + li) * kTailLd + ko);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b1, acc, 0, 0, 0);
        const tl_bf16x8 a2 = *reinterpret_cast<const tl_bf16x8*>(dyT + (wr * 32 + li) * kTailLd + ko);
        const tl_bf16x8 b2 = *reinterpret_cast<const tl_bf16x8*>(actT + (wc * 32 + li) * kTailLd + ko);
        accw = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2, b2, accw, 0, 0, 0);
      }
    }
    __syncthreads();                                     // DY (as d_y), dyA and dyT have been read
    TT_HEAD_STAMP(1);
    if (wave < 4) {
      const int n = wc * 32 + li;
#pragma unroll
      for (int r = 0; r < 16; ++r) DY[(wr * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh) * kTailLdF + n] = acc[r];
    }
    __syncthreads();
    TT_HEAD_STAMP(2);
    // 3. d_act (times the dropout scale) out; da and xhat staged for the ordered column sums
#pragma unroll
    for (int j = 0; j < R; ++j) {
      const int row = rq + NWV * j, r = b0 + row;
      const float da = DY[row * kTailLdF + c] * sc[j];
      if (c < H && r < r1) f.d_act[(int64_t)r * H + c] = da;
      DY[row * kTailLdF + c] = da;
      XH[row * kTailLdF + c] = xh[j];
    }
    __syncthreads();
    TT_HEAD_STAMP(3);
    if (t < 256 && c < H) {                              // colsum_partial_kernel's order: rows r0 + rq, + 4, ...
      const int nrow = min(64, r1 - b0);
      for (int row = rq; row < nrow; row += 4) {
        const float da = DY[row * kTailLdF + c];
        s0 += da;
        s1 += da * XH[row * kTailLdF + c];
      }
    }
    __syncthreads();
    TT_HEAD_STAMP(4);
  }
  if (t < 256) {
    sh[0][rq][c] = s0;
    sh[1][rq][c] = s1;
    sh[2][rq][c] = cs;
  }
  __syncthreads();
  TT_HEAD_STAMP(5);
  if (t < 64) {
    if (c < H) {
      float* q = a.partial + (int64_t)chunk * 2 * H;
      q[c] = ((sh[0][0][c] + sh[0][1][c]) + sh[0][2][c]) + sh[0][3][c];
      q[H + c] = ((sh[1][0][c] + sh[1][1][c]) + sh[1][2][c]) + sh[1][3][c];
    }
    if (c < D) f.b_slab[(int64_t)chunk * D + c] = ((sh[2][0][c] + sh[2][1][c]) + sh[2][2][c]) + sh[2][3][c];
  }
  if (wave < 4) {
    const int wr = wave >> 1, wc = wave & 1, li = lane & 31, lh = lane >> 5;
    float* ws = f.w_slab + (int64_t)chunk * D * H;
    const int n = wc * 32 + li;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = wr * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
      if (m < D && n < H) ws[(int64_t)m * H + n] = accw[r];
    }
  }
  TT_HEAD_STAMP(6);
}

}  // namespace tttail

// ---- the score backward held back for the towers' backward (TT_OPT_FUSE_SCORE_TAIL; slot TT_DQ_SCORE_BWD of tt_deferred.h) ---------
// it and the towers' backward head as ONE launch (score_bwd_tr_kernel<4, 2, UNIT, false, true>, tt_score_bf16.hip) on its stream; takes the slot
int tt_score_tail_bwd_launch(tt_ctx* ctx, const tttail::Batch<tttail::TailBwdArgs>& tb, bool drop, float p, uint64_t seed,
                             const uint64_t* seed_dev);
