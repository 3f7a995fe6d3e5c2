// In-batch-negative score + symmetric softmax cross-entropy without materialising the BxB score
// matrix.  One "direction" = 64 rows of A per workgroup swept against every row of Bm in 128-column
// tiles: S tile on v_mfma_f32_32x32x2_f32 (exact f32 fmaf chain), exp / row sums / diagonal rank in
// the accumulator registers; the backward recomputes the tile, forms the softmax weights in
// registers, passes them through LDS and contracts them with the same Bm tile on MFMA.
// Row sums use a fixed shift (unit-norm rows => |s| <= 1/T), so no running maximum is needed and all
// reductions have a fixed order (bitwise reproducible).
#include "tt_gemm.h"

namespace {

constexpr int kThreads = 256;
constexpr int RB = 64;        // rows of A per workgroup
constexpr int CB = 128;       // columns (rows of Bm) per tile
constexpr int DK = 64;        // feature chunk staged in LDS
constexpr int LDK = DK + 1;   // odd stride: conflict-free fragment reads, 2-way (free) staging writes
constexpr int LDW = CB + 1;
using f32x16 = __attribute__((ext_vector_type(16))) float;

__device__ __forceinline__ int rowmap(int r, int lh) { return (r & 3) + 8 * (r >> 2) + 4 * lh; }

// stage rows [r0, r0+ROWS) x features [d0, d0+DK) of P[R, D] into S[ROWS][LDK] (zero padded)
template <int ROWS, bool VEC>
__device__ __forceinline__ void stage(const float* __restrict__ P, int64_t R, int D, int64_t r0, int d0, float* __restrict__ S, int t) {
#pragma unroll
  for (int p = 0; p < ROWS / 16; ++p) {
    const int row = p * 16 + (t >> 4), kq = (t & 15) * 4;
    const int64_t gr = r0 + row;
    const int d = d0 + kq;
    float v[4];
    if (VEC && gr < R && d + 3 < D) {
      const float4 q = *reinterpret_cast<const float4*>(P + gr * D + d);
      v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = (gr < R && d + j < D) ? P[gr * D + d + j] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) S[row * LDK + kq + j] = v[j];
  }
}

// S tile: wave (wr, wc) computes rows wr*32..+32 x cols wc*64..+64 as two 32x32 accumulators
__device__ __forceinline__ void mfma_s_chunk(const float* __restrict__ As, const float* __restrict__ Bs, int wr, int wc, int li, int lh,
                                             f32x16& acc0, f32x16& acc1) {
#pragma unroll 8
  for (int k = 0; k < DK; k += 2) {
    const float a = As[(wr * 32 + li) * LDK + k + lh];
    const float b0 = Bs[(wc * 64 + li) * LDK + k + lh];
    const float b1 = Bs[(wc * 64 + 32 + li) * LDK + k + lh];
    acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b0, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b1, acc1, 0, 0, 0);
  }
}

__device__ __forceinline__ float half_sum(float x) {   // sum over the 32 lanes sharing lane>>5
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) x += __shfl_xor(x, o);
  return x;
}
__device__ __forceinline__ int half_sum_i(int x) {
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) x += __shfl_xor(x, o);
  return x;
}

// the diagonal score as the same k-ordered fmaf chain the MFMA evaluates
__device__ __forceinline__ float diag_score(const float* __restrict__ A, const float* __restrict__ Bm, int64_t a, int64_t b, int D, float inv_t) {
  float acc = 0.f;
  for (int k = 0; k < D; ++k) acc = __builtin_fmaf(A[a * D + k], Bm[b * D + k], acc);
  return acc * inv_t;
}

// LQ (tt_score_dir_fwd_lq): sumexp adds exp(s - shift) w_b, w_b = tt_lq_weight(lq_b[b]) the B row's sampling weight
// MK (tt_score_dir_fwd_mask; square, diag_off == 0): a pair a != b whose rows share a notice or a company id adds nothing to sumexp;
// the diagonal, the ranks and the score sums stay on the raw scores
// XN (tt_score_dir_fwd_xneg): the B rows are shared extra negatives -- rows without a positive.  The A rows' diagonals come IN
// (diag_in, the in-batch direction's), sumexp and rank are ADDED to: sumexp[a] += sum_m e_am w_m, rank[a] += #{m: s_am > diag[a]} (an
// extra sits behind every in-batch column: a tie does not beat the positive).  The mask (MK) is the company-only compare
// ent_c[a] == ent_x[m]; LQ weighs with lq_b = the extras' log probabilities.  No diag, no score sum out.
template <bool VEC, bool LQ = false, bool MK = false, bool XN = false>
__global__ __launch_bounds__(kThreads) void score_dir_fwd_kernel(const float* __restrict__ A, const float* __restrict__ Bm, int64_t Ra,
                                                                int64_t Rb, int D, float inv_t, float shift, int64_t diag_off,
                                                                float* __restrict__ sumexp, float* __restrict__ diag_out,
                                                                int32_t* __restrict__ rank_out, float* __restrict__ sumscore,
                                                                const float* __restrict__ lq_b = nullptr,
                                                                const int32_t* __restrict__ ent_n = nullptr,
                                                                const int32_t* __restrict__ ent_c = nullptr,
                                                                const int32_t* __restrict__ ent_x = nullptr,
                                                                const float* __restrict__ diag_in = nullptr) {
  __shared__ float As[RB * LDK];
  __shared__ float Bs[CB * LDK];
  __shared__ float diag_s[RB];
  __shared__ float part_e[2][RB];
  __shared__ float part_s[2][RB];
  __shared__ int part_r[2][RB];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wr = wave & 1, wc = wave >> 1, li = lane & 31, lh = lane >> 5;
  const int64_t r0 = (int64_t)blockIdx.x * RB;
  const int nch = (D + DK - 1) / DK;
  if (t < RB) {
    const int64_t a = r0 + t, b = a + diag_off;
    if constexpr (XN) diag_s[t] = a < Ra ? diag_in[a] : 0.f;
    else
    diag_s[t] = (a < Ra && b >= 0 && b < Rb) ? diag_score(A, Bm, a, b, D, inv_t) : 0.f;
  }
  if (nch == 1) stage<RB, VEC>(A, Ra, D, r0, 0, As, t);
  __syncthreads();
  float dg[16], se[16], ss[16];
  int rk[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    dg[r] = diag_s[wr * 32 + rowmap(r, lh)];
    se[r] = 0.f; ss[r] = 0.f; rk[r] = 0;
  }
  [[maybe_unused]] int ean[16], eac[16];                  // (MK) ids of this lane's 16 rows a
  if constexpr (MK) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t a = r0 + wr * 32 + rowmap(r, lh);
      ean[r] = (!XN && a < Ra) ? ent_n[a] : 0;
      eac[r] = a < Ra ? ent_c[a] : 0;
    }
  }
  for (int64_t c0 = 0; c0 < Rb; c0 += CB) {
    f32x16 acc0, acc1;
#pragma unroll
    for (int i = 0; i < 16; ++i) { acc0[i] = 0.f; acc1[i] = 0.f; }
    for (int ch = 0; ch < nch; ++ch) {
      __syncthreads();                                   // previous tile's readers are done
      if (nch > 1) stage<RB, VEC>(A, Ra, D, r0, ch * DK, As, t);
      stage<CB, VEC>(Bm, Rb, D, c0, ch * DK, Bs, t);
      __syncthreads();
      mfma_s_chunk(As, Bs, wr, wc, li, lh, acc0, acc1);
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int64_t col = c0 + wc * 64 + h * 32 + li;
      const bool cv = col < Rb;
      const float wb = LQ && cv ? tt_lq_weight(lq_b[col]) : 1.f;
      [[maybe_unused]] int ebn = 0, ebc = 0;
      if constexpr (MK && XN) ebc = cv ? ent_x[col] : 0;
      else if constexpr (MK) { ebn = cv ? ent_n[col] : 0; ebc = cv ? ent_c[col] : 0; }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float s = (h == 0 ? acc0[r] : acc1[r]) * inv_t;
        const int64_t pos = r0 + wr * 32 + rowmap(r, lh) + diag_off;
        if constexpr (XN) {
          if (cv) {
            float e = __expf(s - shift);
            if constexpr (MK) e = eac[r] == ebc ? 0.f : e;
            if constexpr (LQ) se[r] += e * wb;
            else se[r] += e;
            rk[r] += s > dg[r] ? 1 : 0;
          }
        } else if constexpr (MK) {
          // the plain instantiations' contractions written out (hipcc fuses s - shift and ss += s with the product s = acc / T there,
          // and does not behind the select here): an inert mask gives the plain entry's sums and metrics bit for bit
          if (cv) {
            const float x = h == 0 ? acc0[r] : acc1[r];
            float e = __expf(__builtin_fmaf(x, inv_t, -shift));
            e = (col != pos && ((ean[r] == ebn) | (eac[r] == ebc))) ? 0.f : e;
            if constexpr (LQ) se[r] += e * wb;
            else se[r] += e;
            ss[r] = __builtin_fmaf(x, inv_t, ss[r]);
            rk[r] += (s > dg[r] || (s == dg[r] && col < pos)) ? 1 : 0;
          }
        } else if (cv) {
          if constexpr (LQ) se[r] += __expf(s - shift) * wb;
          else se[r] += __expf(s - shift);
          ss[r] += s;
          rk[r] += (s > dg[r] || (s == dg[r] && col < pos)) ? 1 : 0;
        }
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const float e = half_sum(se[r]), s = half_sum(ss[r]);
    const int k = half_sum_i(rk[r]);
    if (li == 0) {
      const int row = wr * 32 + rowmap(r, lh);
      part_e[wc][row] = e; part_s[wc][row] = s; part_r[wc][row] = k;
    }
  }
  __syncthreads();
  if constexpr (XN) {
    if (t < RB && r0 + t < Ra) {
      sumexp[r0 + t] += part_e[0][t] + part_e[1][t];       // (the in-batch sum first, then the extras')
      rank_out[r0 + t] += part_r[0][t] + part_r[1][t];
    }
    return;
  }
  if (t < RB && r0 + t < Ra) {
    sumexp[r0 + t] = part_e[0][t] + part_e[1][t];
    diag_out[r0 + t] = diag_s[t];
    rank_out[r0 + t] = part_r[0][t] + part_r[1][t];
    if (sumscore) sumscore[r0 + t] = part_s[0][t] + part_s[1][t];
  }
}

// backward of one direction; NCH = ceil(D / 64) feature chunks kept as MFMA accumulators.
// LQ (tt_score_dir_bwd_lq): the weight of (a, b) is exp(s - shift) (w_b / sumexp_a + w_a / sumexp_b), w the sampling weights
// MK (tt_score_dir_bwd_mask; square, diag_off == 0): a masked pair (score_dir_fwd_kernel) weighs nothing
// PW (tt_score_dir_bwd_pw; square, diag_off == 0): per-pair sample weights g -- the reciprocals are g_a / sumexp_a and g_b / sumexp_b,
// the diagonal's -2 is -2 g_a
// XN (tt_score_dir_bwd_xneg): one rectangular direction of the shared extra negatives -- rows without a positive and the one-sided
// weight e_ab fa[a] fb[b]: on the side of the notices f = 1 / rowsum (sumexp_a or sumexp_b, the other NULL), on the side of the
// extras f = their sampling weight (LQ: lq_a or lq_b, the other NULL) or 1.  MK: the company-only compare ent_n[a] == ent_c[b] (here
// the A rows' and the B rows' company ids).  pw_g != NULL: dA += (dN's extra term, behind the square backward's).
template <int NCH, bool VEC, bool LQ = false, bool MK = false, bool PW = false, bool XN = false>
__global__ __launch_bounds__(kThreads) void score_dir_bwd_kernel(const float* __restrict__ A, const float* __restrict__ Bm, int64_t Ra,
                                                                int64_t Rb, int D, float inv_t, float shift, int64_t diag_off,
                                                                const float* __restrict__ sumexp_a, const float* __restrict__ sumexp_b,
                                                                const float* __restrict__ d_loss, float scale, float* __restrict__ dA,
                                                                const float* __restrict__ lq_a = nullptr, const float* __restrict__ lq_b = nullptr,
                                                                const int32_t* __restrict__ ent_n = nullptr,
                                                                const int32_t* __restrict__ ent_c = nullptr,
                                                                const float* __restrict__ pw_g = nullptr) {
  __shared__ float As[RB * LDK];
  __shared__ float Bs[CB * LDK];
  __shared__ float Ws[RB * LDW];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wr = wave & 1, wc = wave >> 1, li = lane & 31, lh = lane >> 5;
  const int64_t r0 = (int64_t)blockIdx.x * RB;
  if (NCH == 1) stage<RB, VEC>(A, Ra, D, r0, 0, As, t);
  float ia[16], ua[16];
  [[maybe_unused]] int ean[16], eac[16];
  [[maybe_unused]] float ga[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int64_t a = r0 + wr * 32 + rowmap(r, lh);
    if constexpr (XN) {
      ia[r] = a < Ra ? (sumexp_a ? 1.f / sumexp_a[a] : ((LQ && lq_a) ? tt_lq_weight(lq_a[a]) : 1.f)) : 0.f;
      if constexpr (MK) ean[r] = a < Ra ? ent_n[a] : 0;
      continue;
    }
    ia[r] = a < Ra ? 1.f / sumexp_a[a] : 0.f;
    if constexpr (PW) { ga[r] = a < Ra ? pw_g[a] : 0.f; ia[r] *= ga[r]; }
    if constexpr (LQ) ua[r] = a < Ra ? tt_lq_weight(lq_a[a]) : 0.f;
    if constexpr (MK) { ean[r] = a < Ra ? ent_n[a] : 0; eac[r] = a < Ra ? ent_c[a] : 0; }
  }
  f32x16 dacc[NCH];
#pragma unroll
  for (int c = 0; c < NCH; ++c)
#pragma unroll
    for (int i = 0; i < 16; ++i) dacc[c][i] = 0.f;
  for (int64_t c0 = 0; c0 < Rb; c0 += CB) {
    f32x16 acc0, acc1;
#pragma unroll
    for (int i = 0; i < 16; ++i) { acc0[i] = 0.f; acc1[i] = 0.f; }
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
      __syncthreads();
      if (NCH > 1) stage<RB, VEC>(A, Ra, D, r0, ch * DK, As, t);
      stage<CB, VEC>(Bm, Rb, D, c0, ch * DK, Bs, t);
      __syncthreads();
      mfma_s_chunk(As, Bs, wr, wc, li, lh, acc0, acc1);
    }
    // softmax weights of this tile -> LDS in [row][col] order
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int cl = wc * 64 + h * 32 + li;
      const int64_t col = c0 + cl;
      const bool cv = col < Rb;
      float ib;
      if constexpr (XN) ib = cv ? (sumexp_b ? 1.f / sumexp_b[col] : ((LQ && lq_b) ? tt_lq_weight(lq_b[col]) : 1.f)) : 0.f;
      else ib = cv ? 1.f / sumexp_b[col] : 0.f;
      if constexpr (PW) ib *= cv ? pw_g[col] : 0.f;
      const float wb = (LQ && !XN && cv) ? tt_lq_weight(lq_b[col]) : 0.f;
      [[maybe_unused]] int ebn = 0, ebc = 0;
      if constexpr (MK && XN) ebc = cv ? ent_c[col] : 0;
      else if constexpr (MK) { ebn = cv ? ent_n[col] : 0; ebc = cv ? ent_c[col] : 0; }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = wr * 32 + rowmap(r, lh);
        const float s = (h == 0 ? acc0[r] : acc1[r]) * inv_t;
        float w = 0.f;
        if constexpr (XN) {
          if (cv) {
            w = __expf(s - shift) * (ia[r] * ib);
            if constexpr (MK) { if (ean[r] == ebc) w = 0.f; }
          }
        } else
        if (cv) {
          if constexpr (LQ) w = __expf(s - shift) * (wb * ia[r] + ua[r] * ib);
          else w = __expf(s - shift) * (ia[r] + ib);
          if constexpr (PW) {
            if (col == r0 + row + diag_off) w = __builtin_fmaf(-2.f, ga[r], w);
            else if constexpr (MK) { if ((ean[r] == ebn) | (eac[r] == ebc)) w = 0.f; }
          } else if constexpr (MK) {
            // (the diagonal as the plain instantiations compile it: e (ia + ib) - 2 in one fma -- an inert mask gives their bits)
            if (col == r0 + row + diag_off) {
              if constexpr (!LQ) w = __builtin_fmaf(ia[r] + ib, __expf(s - shift), -2.f);
              else w -= 2.f;
            } else if ((ean[r] == ebn) | (eac[r] == ebc)) w = 0.f;
          } else
          if (col == r0 + row + diag_off) w -= 2.f;
        }
        Ws[row * LDW + cl] = w;
      }
    }
    // dA[:, chunk] += W[64 x 128] . Bm_tile[128 x 64]; wave (wr, wc) -> rows wr*32.., features wc*32..
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
      __syncthreads();                                   // Ws complete (ch == 0) / Bs readers done (ch > 0)
      if (NCH > 1) {
        stage<CB, VEC>(Bm, Rb, D, c0, ch * DK, Bs, t);
        __syncthreads();
      }
#pragma unroll 8
      for (int kb = 0; kb < CB; kb += 2) {
        const float a = Ws[(wr * 32 + li) * LDW + kb + lh];
        const float b = Bs[(kb + lh) * LDK + wc * 32 + li];
        dacc[ch] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, dacc[ch], 0, 0, 0);
      }
    }
  }
  const float g = d_loss[0] * scale;
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch) {
    const int d = ch * DK + wc * 32 + li;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t a = r0 + wr * 32 + rowmap(r, lh);
      if constexpr (XN) {
        if (a < Ra && d < D) {
          const float v = dacc[ch][r] * g;
          dA[a * D + d] = pw_g ? dA[a * D + d] + v : v;
        }
      } else
      if (a < Ra && d < D) dA[a * D + d] = dacc[ch][r] * g;
    }
  }
}

// loss + metrics from the per-row results of both directions (one workgroup, fixed-order sums)
__global__ __launch_bounds__(1024) void loss_finish_kernel(int64_t B, float shift, const float* __restrict__ rowsum,
                                                           const float* __restrict__ colsum, const float* __restrict__ diag,
                                                           const int32_t* __restrict__ row_rank, const int32_t* __restrict__ col_rank,
                                                           const float* __restrict__ sumscore, float* __restrict__ out,
                                                           float* __restrict__ loss_out) {
  __shared__ float sh5[5][16];
  float l = 0.f, hit = 0.f, chit = 0.f, dsum = 0.f, tot = 0.f;
#pragma unroll 4
  for (int64_t i = threadIdx.x; i < B; i += blockDim.x) {
    const float d = diag[i];
    l += (logf(rowsum[i]) + shift - d) + (logf(colsum[i]) + shift - d);
    hit += row_rank[i] == 0 ? 1.f : 0.f;
    chit += col_rank[i] == 0 ? 1.f : 0.f;
    dsum += d;
    tot += sumscore ? sumscore[i] : 0.f;
  }
  // the five sums together: butterfly inside the wave, one LDS exchange, fixed order across the 16 waves
  float v[5] = {l, hit, chit, dsum, tot};
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
#pragma unroll
    for (int j = 0; j < 5; ++j) v[j] += __shfl_xor(v[j], o);
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int j = 0; j < 5; ++j) sh5[j][threadIdx.x >> 6] = v[j];
  __syncthreads();
  if (threadIdx.x == 0) {
    const int nw = (blockDim.x + 63) >> 6;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      float t = 0.f;
      for (int w = 0; w < nw; ++w) t += sh5[j][w];
      v[j] = t;
    }
    l = v[0]; hit = v[1]; chit = v[2]; dsum = v[3]; tot = v[4];
  }
  if (threadIdx.x == 0) {
    const float fb = (float)B;
    const float pos = dsum / fb;
    const float neg = (tot - dsum) / (fb * fb - fb);       // mean over the off-diagonal (nan for B == 1, as torch)
    out[0] = 0.5f * l / fb;
    out[1] = hit / fb;
    out[2] = pos;
    out[3] = neg;
    out[4] = pos - neg;
    out[5] = chit / fb;
    out[6] = tot;
    out[7] = 0.f;
    if (loss_out) loss_out[0] = out[0];
  }
}

// tt_score_loss_finish_lq: loss_finish_kernel with each direction's term less the log weight of its positive (-kLqL - lq, exactly)
__global__ __launch_bounds__(1024) void loss_finish_lq_kernel(int64_t B, float shift, const float* __restrict__ rowsum,
                                                           const float* __restrict__ colsum, const float* __restrict__ diag,
                                                           const int32_t* __restrict__ row_rank, const int32_t* __restrict__ col_rank,
                                                           const float* __restrict__ sumscore, float* __restrict__ out,
                                                           float* __restrict__ loss_out, const float* __restrict__ lq_n,
                                                           const float* __restrict__ lq_c) {
  __shared__ float sh5[5][16];
  float l = 0.f, hit = 0.f, chit = 0.f, dsum = 0.f, tot = 0.f;
#pragma unroll 4
  for (int64_t i = threadIdx.x; i < B; i += blockDim.x) {
    const float d = diag[i];
    l += (logf(rowsum[i]) + shift - d - tt_lq_log_weight(lq_c[i])) + (logf(colsum[i]) + shift - d - tt_lq_log_weight(lq_n[i]));
    hit += row_rank[i] == 0 ? 1.f : 0.f;
    chit += col_rank[i] == 0 ? 1.f : 0.f;
    dsum += d;
    tot += sumscore ? sumscore[i] : 0.f;
  }
  // the five sums together: butterfly inside the wave, one LDS exchange, fixed order across the 16 waves
  float v[5] = {l, hit, chit, dsum, tot};
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
#pragma unroll
    for (int j = 0; j < 5; ++j) v[j] += __shfl_xor(v[j], o);
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int j = 0; j < 5; ++j) sh5[j][threadIdx.x >> 6] = v[j];
  __syncthreads();
  if (threadIdx.x == 0) {
    const int nw = (blockDim.x + 63) >> 6;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      float t = 0.f;
      for (int w = 0; w < nw; ++w) t += sh5[j][w];
      v[j] = t;
    }
    l = v[0]; hit = v[1]; chit = v[2]; dsum = v[3]; tot = v[4];
  }
  if (threadIdx.x == 0) {
    const float fb = (float)B;
    const float pos = dsum / fb;
    const float neg = (tot - dsum) / (fb * fb - fb);       // mean over the off-diagonal (nan for B == 1, as torch)
    out[0] = 0.5f * l / fb;
    out[1] = hit / fb;
    out[2] = pos;
    out[3] = neg;
    out[4] = pos - neg;
    out[5] = chit / fb;
    out[6] = tot;
    out[7] = 0.f;
    if (loss_out) loss_out[0] = out[0];
  }
}

// tt_score_loss_finish_pw: each pair's two terms times its weight g_i (tt_score_prepare_pw); LQ as loss_finish_lq_kernel.  The
// metrics are the unweighted ones.  (g_i = 1: the product is exact -- the bits of the kernels above.)
template <bool LQ>
__global__ __launch_bounds__(1024) void loss_finish_pw_kernel(int64_t B, float shift, const float* __restrict__ rowsum,
                                                              const float* __restrict__ colsum, const float* __restrict__ diag,
                                                              const int32_t* __restrict__ row_rank, const int32_t* __restrict__ col_rank,
                                                              const float* __restrict__ sumscore, float* __restrict__ out,
                                                              float* __restrict__ loss_out, const float* __restrict__ lq_n,
                                                              const float* __restrict__ lq_c, const float* __restrict__ pw_g) {
  __shared__ float sh5[5][16];
  float l = 0.f, hit = 0.f, chit = 0.f, dsum = 0.f, tot = 0.f;
#pragma unroll 4
  for (int64_t i = threadIdx.x; i < B; i += blockDim.x) {
    const float d = diag[i];
    float li;
    if constexpr (LQ) li = (logf(rowsum[i]) + shift - d - tt_lq_log_weight(lq_c[i])) + (logf(colsum[i]) + shift - d - tt_lq_log_weight(lq_n[i]));
    else li = (logf(rowsum[i]) + shift - d) + (logf(colsum[i]) + shift - d);
    l += pw_g[i] * li;
    hit += row_rank[i] == 0 ? 1.f : 0.f;
    chit += col_rank[i] == 0 ? 1.f : 0.f;
    dsum += d;
    tot += sumscore ? sumscore[i] : 0.f;
  }
  float v[5] = {l, hit, chit, dsum, tot};
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
#pragma unroll
    for (int j = 0; j < 5; ++j) v[j] += __shfl_xor(v[j], o);
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int j = 0; j < 5; ++j) sh5[j][threadIdx.x >> 6] = v[j];
  __syncthreads();
  if (threadIdx.x == 0) {
    const int nw = (blockDim.x + 63) >> 6;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      float t = 0.f;
      for (int w = 0; w < nw; ++w) t += sh5[j][w];
      v[j] = t;
    }
    const float fb = (float)B;
    const float pos = v[3] / fb;
    const float neg = (v[4] - v[3]) / (fb * fb - fb);
    out[0] = 0.5f * v[0] / fb;
    out[1] = v[1] / fb;
    out[2] = pos;
    out[3] = neg;
    out[4] = pos - neg;
    out[5] = v[2] / fb;
    out[6] = v[4];
    out[7] = 0.f;
    if (loss_out) loss_out[0] = out[0];
  }
}

// ---- dense loss path: label-smoothed cross-entropy and cosine-embedding loss on the MATERIALISED score matrix --------
// (two_tower_train_task.py:114-160; neither is used by scripts/train.py -- the fused kernels cover the default loss only).
// S [B, B] = N C^T / T in memory; everything f32, fixed summation orders.
//   CE with smoothing e:  row term  lse_r[a] - (1 - e) s_aa - (e / B) sum_b s_ab   (F.cross_entropy(label_smoothing=e)),
//                         the same over columns; loss = (mean row term + mean column term) / 2
//   cosine embedding:     F.cosine_embedding_loss on the 1-vectors [s] vs [1]: cos = s / sqrt((s^2 + 1e-12)(1 + 1e-12));
//                         positives (diagonal) 1 - cos, negatives max(0, cos); mean over all B^2 entries
constexpr float kCosEps = 1e-12f;
__device__ __forceinline__ float cos1(float s) { return s / sqrtf((s * s + kCosEps) * (1.f + kCosEps)); }
__device__ __forceinline__ float dcos1(float s) {                 // d cos / d s = eps (s^2 + eps)^(-3/2) / sqrt(1 + eps)
  const float q = s * s + kCosEps;
  return kCosEps / (q * sqrtf(q) * sqrtf(1.f + kCosEps));
}

// one wave per row: max / first argmax, logsumexp, plain sum, cosine loss sum of the row
__global__ __launch_bounds__(kThreads) void dense_row_stats_kernel(const float* __restrict__ S, int64_t B, float* __restrict__ lse,
                                                                  float* __restrict__ sum, float* __restrict__ cosl,
                                                                  float* __restrict__ diag, int32_t* __restrict__ hit) {
  const int lane = threadIdx.x & 63;
  const int64_t a = (int64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
  if (a >= B) return;
  const float* row = S + a * B;
  float m = -INFINITY;
  int64_t mi = B;
  for (int64_t b = lane; b < B; b += 64) {
    const float v = row[b];
    if (v > m) { m = v; mi = b; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float m2 = __shfl_xor(m, o);
    const int64_t i2 = (int64_t)__shfl_xor((int)mi, o);
    if (m2 > m || (m2 == m && i2 < mi)) { m = m2; mi = i2; }
  }
  float e = 0.f, t = 0.f, cl = 0.f;
  for (int64_t b = lane; b < B; b += 64) {
    const float v = row[b];
    e += expf(v - m);
    t += v;
    const float c = cos1(v);
    cl += b == a ? 1.f - c : fmaxf(c, 0.f);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { e += __shfl_xor(e, o); t += __shfl_xor(t, o); cl += __shfl_xor(cl, o); }
  if (lane == 0) {
    lse[a] = m + logf(e);
    sum[a] = t;
    cosl[a] = cl;
    diag[a] = row[a];
    hit[a] = mi == a ? 1 : 0;
  }
}

// one thread per column: online logsumexp and plain sum down the column (coalesced across the threads of a wave)
__global__ __launch_bounds__(kThreads) void dense_col_stats_kernel(const float* __restrict__ S, int64_t B, float* __restrict__ lse,
                                                                  float* __restrict__ sum, int32_t* __restrict__ hit) {
  const int64_t b = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (b >= B) return;
  float m = -INFINITY, e = 0.f, t = 0.f;
  int64_t mi = B;
  for (int64_t a = 0; a < B; ++a) {
    const float v = S[a * B + b];
    if (v > m) { e = e * expf(m - v) + 1.f; m = v; mi = a; }      // strict >: the first maximal row, as torch.argmax
    else e += expf(v - m);
    t += v;
  }
  lse[b] = m + logf(e);
  sum[b] = t;
  hit[b] = mi == b ? 1 : 0;
}

// loss + metrics (one workgroup, fixed order).  stats = [lse_r | sum_r | lse_c | sum_c | cos_r | diag] (B each)
__global__ __launch_bounds__(1024) void dense_finish_kernel(int64_t B, int loss_type, float smooth, const float* __restrict__ stats,
                                                            const int32_t* __restrict__ hit, float* __restrict__ out,
                                                            float* __restrict__ loss_out) {
  __shared__ float sh4[5][16];
  const float* lse_r = stats; const float* sum_r = stats + B; const float* lse_c = stats + 2 * B; const float* sum_c = stats + 3 * B;
  const float* cos_r = stats + 4 * B; const float* diag = stats + 5 * B;
  const float fb = (float)B;
  float l = 0.f, h = 0.f, ds = 0.f, tot = 0.f, hc = 0.f;
  for (int64_t i = threadIdx.x; i < B; i += blockDim.x) {
    const float d = diag[i];
    if (loss_type == 0) l += (lse_r[i] - (1.f - smooth) * d - smooth / fb * sum_r[i]) + (lse_c[i] - (1.f - smooth) * d - smooth / fb * sum_c[i]);
    else l += cos_r[i];
    h += hit[i] ? 1.f : 0.f;
    hc += hit[B + i] ? 1.f : 0.f;
    ds += d;
    tot += sum_r[i];
  }
  float v[5] = {l, h, ds, tot, hc};
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
#pragma unroll
    for (int j = 0; j < 5; ++j) v[j] += __shfl_xor(v[j], o);
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int j = 0; j < 5; ++j) sh4[j][threadIdx.x >> 6] = v[j];
  __syncthreads();
  if (threadIdx.x == 0) {
    const int nw = (blockDim.x + 63) >> 6;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      float t = 0.f;
      for (int w = 0; w < nw; ++w) t += sh4[j][w];
      v[j] = t;
    }
    const float pos = v[2] / fb, neg = (v[3] - v[2]) / (fb * fb - fb);
    out[0] = loss_type == 0 ? 0.5f * v[0] / fb : v[0] / (fb * fb);
    out[1] = v[1] / fb;
    out[2] = pos; out[3] = neg; out[4] = pos - neg;
    out[5] = v[4] / fb; out[6] = v[3]; out[7] = 0.f;
    if (loss_out) loss_out[0] = out[0];
  }
}

// S -> d loss / d (N C^T) in place (the 1 / T of S = N C^T / T included), times the incoming gradient
__global__ __launch_bounds__(kThreads) void dense_grad_kernel(float* __restrict__ S, int64_t B, int loss_type, float smooth, float inv_t,
                                                             const float* __restrict__ stats, const float* __restrict__ d_loss) {
  const float* lse_r = stats; const float* lse_c = stats + 2 * B;
  const float fb = (float)B, g = d_loss[0] * inv_t;
  const int64_t total = B * B;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kThreads) {
    const int64_t a = i / B, b = i - a * B;
    const float v = S[i];
    float d;
    if (loss_type == 0) {
      const float onehot = a == b ? 1.f - smooth : 0.f;
      d = 0.5f / fb * ((expf(v - lse_r[a]) - onehot - smooth / fb) + (expf(v - lse_c[b]) - onehot - smooth / fb));
    } else {
      const float dc = dcos1(v);
      d = (a == b ? -dc : (cos1(v) > 0.f ? dc : 0.f)) / (fb * fb);
    }
    S[i] = d * g;
  }
}

// top-k per row: one wave per row, k selection passes over the row in the total order
// (value descending, column ascending) -- no marking, no scratch
__global__ __launch_bounds__(kThreads) void topk_rows_kernel(const float* __restrict__ S, int64_t R, int64_t C, int64_t lds, int k,
                                                            float* __restrict__ vals, int64_t* __restrict__ idx) {
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= R) return;
  const float* s = S + row * lds;
  float pv = __builtin_inff();
  int64_t pi = -1;
  for (int j = 0; j < k; ++j) {
    float bv = -__builtin_inff();
    int64_t bi = INT64_MAX;
    for (int64_t c = lane; c < C; c += 64) {
      const float v = s[c];
      const bool after_prev = v < pv || (v == pv && c > pi);
      const bool better = v > bv || (v == bv && c < bi);
      if (after_prev && better) { bv = v; bi = c; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o);
      const int64_t oi = __shfl_xor(bi, o);
      if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    if (lane == 0) {
      vals[row * k + j] = bv;
      idx[row * k + j] = bi == INT64_MAX ? -1 : bi;
    }
    pv = bv; pi = bi;
  }
}

__global__ __launch_bounds__(kThreads) void diag_rank_rows_kernel(const float* __restrict__ S, int64_t R, int64_t C, int64_t lds,
                                                                 int64_t off, int32_t* __restrict__ rank) {
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= R) return;
  const int64_t pos = row + off;
  const float* s = S + row * lds;
  if (pos < 0 || pos >= C) {                     // no positive in this row: -1, as the retrieval entries (0 would be a perfect rank)
    if (lane == 0) rank[row] = -1;
    return;
  }
  int cnt = 0;
  const float d = s[pos];
  for (int64_t c = lane; c < C; c += 64) {
    const float v = s[c];
    cnt += (v > d || (v == d && c < pos)) ? 1 : 0;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
  if (lane == 0) rank[row] = cnt;
}

inline bool vec_ok(const float* p, int D) { return tt_aligned(p, 16) && (D % 4 == 0); }

}  // namespace

// tt_score_dir_fwd and, with lq_b != NULL, tt_score_dir_fwd_lq (arguments checked by the entries)
static int dir_fwd(const float* A, const float* Bm, int64_t Ra, int64_t Rb, int32_t D, float inv_t, float shift, int64_t diag_offset,
                   const float* lq_b, float* sumexp, float* diag, int32_t* rank, float* sumscore, tt_stream stream,
                   const int32_t* ent_n = nullptr, const int32_t* ent_c = nullptr) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const unsigned grid = (unsigned)tt_cdiv(Ra, RB);
  if (ent_n) {                                           // tt_score_dir_fwd_mask
    tt_dispatch([&](auto vec, auto lq) {
      score_dir_fwd_kernel<vec, lq, true><<<grid, kThreads, 0, st>>>(A, Bm, Ra, Rb, D, inv_t, shift, diag_offset, sumexp, diag, rank, sumscore,
                                                                     lq_b, ent_n, ent_c);
    }, vec_ok(A, D) && vec_ok(Bm, D), lq_b != nullptr);
    TT_LAUNCH_CHECK();
    return TT_OK;
  }
  tt_dispatch([&](auto vec, auto lq) {
    score_dir_fwd_kernel<vec, lq><<<grid, kThreads, 0, st>>>(A, Bm, Ra, Rb, D, inv_t, shift, diag_offset, sumexp, diag, rank, sumscore, lq_b);
  }, vec_ok(A, D) && vec_ok(Bm, D), lq_b != nullptr);
  TT_LAUNCH_CHECK();
  return TT_OK;
}

// tt_score_loss_finish and, with lq_n / lq_c != NULL, tt_score_loss_finish_lq
static int loss_finish(int64_t B, float shift, const float* lq_n, const float* lq_c, const float* rowsum, const float* colsum,
                       const float* diag, const int32_t* row_rank, const int32_t* col_rank, const float* sumscore, float* out8,
                       float* loss_out, tt_stream stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (lq_n) loss_finish_lq_kernel<<<1, 1024, 0, st>>>(B, shift, rowsum, colsum, diag, row_rank, col_rank, sumscore, out8, loss_out, lq_n, lq_c);
  else loss_finish_kernel<<<1, 1024, 0, st>>>(B, shift, rowsum, colsum, diag, row_rank, col_rank, sumscore, out8, loss_out);
  TT_LAUNCH_CHECK();
  return TT_OK;
}

// tt_score_dir_bwd and, with lq_a / lq_b != NULL, tt_score_dir_bwd_lq
static int dir_bwd(const float* A, const float* Bm, int64_t Ra, int64_t Rb, int32_t D, float inv_t, float shift, int64_t diag_offset,
                   const float* lq_a, const float* lq_b, const float* sumexp_a, const float* sumexp_b, const float* d_loss, float scale,
                   float* dA, tt_stream stream, const int32_t* ent_n = nullptr, const int32_t* ent_c = nullptr,
                   const float* pw_g = nullptr) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const unsigned grid = (unsigned)tt_cdiv(Ra, RB);
  const auto go = [&](auto nch) {
    if (pw_g) {                                          // tt_score_dir_bwd_pw
      tt_dispatch([&](auto vec, auto lq, auto mk) {
        score_dir_bwd_kernel<nch, vec, lq, mk, true><<<grid, kThreads, 0, st>>>(A, Bm, Ra, Rb, D, inv_t, shift, diag_offset, sumexp_a, sumexp_b,
                                                                                 d_loss, scale, dA, lq_a, lq_b, ent_n, ent_c, pw_g);
      }, vec_ok(A, D) && vec_ok(Bm, D), lq_a != nullptr, ent_n != nullptr);
      return;
    }
    if (ent_n) {                                         // tt_score_dir_bwd_mask
      tt_dispatch([&](auto vec, auto lq) {
        score_dir_bwd_kernel<nch, vec, lq, true><<<grid, kThreads, 0, st>>>(A, Bm, Ra, Rb, D, inv_t, shift, diag_offset, sumexp_a, sumexp_b,
                                                                             d_loss, scale, dA, lq_a, lq_b, ent_n, ent_c);
      }, vec_ok(A, D) && vec_ok(Bm, D), lq_a != nullptr);
      return;
    }
    tt_dispatch([&](auto vec, auto lq) {
      score_dir_bwd_kernel<nch, vec, lq><<<grid, kThreads, 0, st>>>(A, Bm, Ra, Rb, D, inv_t, shift, diag_offset, sumexp_a, sumexp_b, d_loss,
                                                                     scale, dA, lq_a, lq_b);
    }, vec_ok(A, D) && vec_ok(Bm, D), lq_a != nullptr);
  };
  switch ((D + DK - 1) / DK) {
    case 1: go(tt_c<1>); break;
    case 2: go(tt_c<2>); break;
    case 3: go(tt_c<3>); break;
    default: go(tt_c<4>); break;
  }
  TT_LAUNCH_CHECK();
  return TT_OK;
}

extern "C" {

int tt_score_dir_fwd(tt_ctx* ctx, const float* A, const float* Bm, int64_t Ra, int64_t Rb, int32_t D, float inv_t, float shift,
                     int64_t diag_offset, float* sumexp, float* diag, int32_t* rank, float* sumscore, tt_stream stream) {
  TT_CHECK_ARG(ctx && A && Bm && sumexp && diag && rank, "tt_score_dir_fwd: NULL argument");
  TT_CHECK_ARG(Ra >= 1 && Rb >= 1 && D >= 1, "tt_score_dir_fwd: bad shape");
  TT_CHECK_ARG(Ra < ((int64_t)1 << 31) && Rb < ((int64_t)1 << 31), "tt_score_dir_fwd: too many rows");
  if (2.f * fabsf(inv_t) > 80.f) {
    tt_set_error("tt_score_dir_fwd: 1/temperature = %g: fixed-shift softmax needs 2/T <= 80", inv_t);
    return TT_ERR_UNSUPPORTED;
  }
  return dir_fwd(A, Bm, Ra, Rb, D, inv_t, shift, diag_offset, nullptr, sumexp, diag, rank, sumscore, stream);
}

int tt_score_loss_finish(tt_ctx* ctx, int64_t B, float shift, const float* rowsum, const float* colsum, const float* diag,
                         const int32_t* row_rank, const int32_t* col_rank, const float* sumscore, float* out8, float* loss_out,
                         tt_stream stream) {
  TT_CHECK_ARG(ctx && rowsum && colsum && diag && row_rank && col_rank && out8, "tt_score_loss_finish: NULL argument");
  TT_CHECK_ARG(B >= 1, "tt_score_loss_finish: B < 1");
  return loss_finish(B, shift, nullptr, nullptr, rowsum, colsum, diag, row_rank, col_rank, sumscore, out8, loss_out, stream);
}

int tt_score_dir_bwd(tt_ctx* ctx, const float* A, const float* Bm, int64_t Ra, int64_t Rb, int32_t D, float inv_t, float shift,
                     int64_t diag_offset, const float* sumexp_a, const float* sumexp_b, const float* d_loss, float scale, float* dA,
                     tt_stream stream) {
  TT_CHECK_ARG(ctx && A && Bm && sumexp_a && sumexp_b && d_loss && dA, "tt_score_dir_bwd: NULL argument");
  TT_CHECK_ARG(Ra >= 1 && Rb >= 1 && D >= 1, "tt_score_dir_bwd: bad shape");
  if (D > 4 * DK) {
    tt_set_error("tt_score_dir_bwd: D=%d > %d not supported", D, 4 * DK);
    return TT_ERR_UNSUPPORTED;
  }
  return dir_bwd(A, Bm, Ra, Rb, D, inv_t, shift, diag_offset, nullptr, nullptr, sumexp_a, sumexp_b, d_loss, scale, dA, stream);
}

int tt_score_dir_fwd_lq(tt_ctx* ctx, const float* A, const float* Bm, int64_t Ra, int64_t Rb, int32_t D, float inv_t, float shift,
                        int64_t diag_offset, const float* lq_b, float* sumexp, float* diag, int32_t* rank, float* sumscore,
                        tt_stream stream) {
  TT_CHECK_ARG(ctx && A && Bm && lq_b && sumexp && diag && rank, "tt_score_dir_fwd_lq: NULL argument");
  TT_CHECK_ARG(Ra >= 1 && Rb >= 1 && D >= 1, "tt_score_dir_fwd_lq: bad shape");
  TT_CHECK_ARG(Ra < ((int64_t)1 << 31) && Rb < ((int64_t)1 << 31), "tt_score_dir_fwd_lq: too many rows");
  if (2.f * fabsf(inv_t) > kLqMaxTwoInvT) {
    tt_set_error("tt_score_dir_fwd_lq: 1/temperature = %g: the logQ-corrected softmax needs 2/T <= %g", inv_t, kLqMaxTwoInvT);
    return TT_ERR_UNSUPPORTED;
  }
  return dir_fwd(A, Bm, Ra, Rb, D, inv_t, shift, diag_offset, lq_b, sumexp, diag, rank, sumscore, stream);
}

int tt_score_loss_finish_lq(tt_ctx* ctx, int64_t B, float shift, const float* lq_n, const float* lq_c, const float* rowsum,
                            const float* colsum, const float* diag, const int32_t* row_rank, const int32_t* col_rank,
                            const float* sumscore, float* out8, float* loss_out, tt_stream stream) {
  TT_CHECK_ARG(ctx && lq_n && lq_c && rowsum && colsum && diag && row_rank && col_rank && out8, "tt_score_loss_finish_lq: NULL argument");
  TT_CHECK_ARG(B >= 1, "tt_score_loss_finish_lq: B < 1");
  return loss_finish(B, shift, lq_n, lq_c, rowsum, colsum, diag, row_rank, col_rank, sumscore, out8, loss_out, stream);
}

int tt_score_dir_bwd_lq(tt_ctx* ctx, const float* A, const float* Bm, int64_t Ra, int64_t Rb, int32_t D, float inv_t, float shift,
                        int64_t diag_offset, const float* lq_a, const float* lq_b, const float* sumexp_a, const float* sumexp_b,
                        const float* d_loss, float scale, float* dA, tt_stream stream) {
  TT_CHECK_ARG(ctx && A && Bm && lq_a && lq_b && sumexp_a && sumexp_b && d_loss && dA, "tt_score_dir_bwd_lq: NULL argument");
  TT_CHECK_ARG(Ra >= 1 && Rb >= 1 && D >= 1, "tt_score_dir_bwd_lq: bad shape");
  if (D > 4 * DK) {
    tt_set_error("tt_score_dir_bwd_lq: D=%d > %d not supported", D, 4 * DK);
    return TT_ERR_UNSUPPORTED;
  }
  if (2.f * fabsf(inv_t) > kLqMaxTwoInvT) {
    tt_set_error("tt_score_dir_bwd_lq: 1/temperature = %g: the logQ-corrected softmax needs 2/T <= %g", inv_t, kLqMaxTwoInvT);
    return TT_ERR_UNSUPPORTED;
  }
  return dir_bwd(A, Bm, Ra, Rb, D, inv_t, shift, diag_offset, lq_a, lq_b, sumexp_a, sumexp_b, d_loss, scale, dA, stream);
}

// the masked directional entries: square problems only; lq NULL = uncorrected
static int mask_dir_check(const char* who, int64_t Ra, int64_t Rb, int64_t diag_offset, float inv_t, bool lq) {
  if (Ra != Rb || diag_offset != 0) {
    tt_set_error("%s: the repeated-entity mask covers the square problem only (Ra == Rb, diag_offset == 0)", who);
    return TT_ERR_UNSUPPORTED;
  }
  if (2.f * fabsf(inv_t) > (lq ? kLqMaxTwoInvT : 80.f)) {
    tt_set_error("%s: 1/temperature = %g: needs 2/T <= %g", who, inv_t, lq ? kLqMaxTwoInvT : 80.f);
    return TT_ERR_UNSUPPORTED;
  }
  return TT_OK;
}

int tt_score_dir_fwd_mask(tt_ctx* ctx, const float* A, const float* Bm, int64_t Ra, int64_t Rb, int32_t D, float inv_t, float shift,
                          int64_t diag_offset, const int32_t* ent_n, const int32_t* ent_c, const float* lq_b, float* sumexp,
                          float* diag, int32_t* rank, float* sumscore, tt_stream stream) {
  TT_CHECK_ARG(ctx && A && Bm && ent_n && ent_c && sumexp && diag && rank, "tt_score_dir_fwd_mask: NULL argument");
  TT_CHECK_ARG(Ra >= 1 && Rb >= 1 && D >= 1, "tt_score_dir_fwd_mask: bad shape");
  TT_CHECK_ARG(Ra < ((int64_t)1 << 31) && Rb < ((int64_t)1 << 31), "tt_score_dir_fwd_mask: too many rows");
  if (int rc = mask_dir_check("tt_score_dir_fwd_mask", Ra, Rb, diag_offset, inv_t, lq_b != nullptr)) return rc;
  return dir_fwd(A, Bm, Ra, Rb, D, inv_t, shift, diag_offset, lq_b, sumexp, diag, rank, sumscore, stream, ent_n, ent_c);
}

int tt_score_dir_bwd_mask(tt_ctx* ctx, const float* A, const float* Bm, int64_t Ra, int64_t Rb, int32_t D, float inv_t, float shift,
                          int64_t diag_offset, const int32_t* ent_n, const int32_t* ent_c, const float* lq_a, const float* lq_b,
                          const float* sumexp_a, const float* sumexp_b, const float* d_loss, float scale, float* dA, tt_stream stream) {
  TT_CHECK_ARG(ctx && A && Bm && ent_n && ent_c && sumexp_a && sumexp_b && d_loss && dA, "tt_score_dir_bwd_mask: NULL argument");
  TT_CHECK_ARG((lq_a != nullptr) == (lq_b != nullptr), "tt_score_dir_bwd_mask: lq_a and lq_b go together");
  TT_CHECK_ARG(Ra >= 1 && Rb >= 1 && D >= 1, "tt_score_dir_bwd_mask: bad shape");
  if (D > 4 * DK) {
    tt_set_error("tt_score_dir_bwd_mask: D=%d > %d not supported", D, 4 * DK);
    return TT_ERR_UNSUPPORTED;
  }
  if (int rc = mask_dir_check("tt_score_dir_bwd_mask", Ra, Rb, diag_offset, inv_t, lq_a != nullptr)) return rc;
  return dir_bwd(A, Bm, Ra, Rb, D, inv_t, shift, diag_offset, lq_a, lq_b, sumexp_a, sumexp_b, d_loss, scale, dA, stream, ent_n, ent_c);
}

// the extra-negative entries of the f32 parity path (include/twotower.h): rows without a positive, the company-only mask
int tt_score_dir_fwd_xneg(tt_ctx* ctx, const float* N, const float* X, int64_t B, int64_t M, int32_t D, float inv_t, float shift,
                          const int32_t* ent_c, const int32_t* ent_x, const float* lq_x, const float* diag, float* sumexp,
                          int32_t* rank, tt_stream stream) {
  TT_CHECK_ARG(ctx && N && X && diag && sumexp && rank, "tt_score_dir_fwd_xneg: NULL argument");
  TT_CHECK_ARG(B >= 1 && M >= 1 && D >= 1, "tt_score_dir_fwd_xneg: bad shape");
  TT_CHECK_ARG(B < ((int64_t)1 << 31) && M < ((int64_t)1 << 31), "tt_score_dir_fwd_xneg: too many rows");
  TT_CHECK_ARG((ent_c != nullptr) == (ent_x != nullptr), "tt_score_dir_fwd_xneg: ent_c and ent_x go together");
  if (2.f * fabsf(inv_t) > (lq_x ? kLqMaxTwoInvT : 80.f)) {
    tt_set_error("tt_score_dir_fwd_xneg: 1/temperature = %g: needs 2/T <= %g", inv_t, lq_x ? kLqMaxTwoInvT : 80.f);
    return TT_ERR_UNSUPPORTED;
  }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  tt_dispatch([&](auto vec, auto lq, auto mk) {
    score_dir_fwd_kernel<vec, lq, mk, true><<<(unsigned)tt_cdiv(B, RB), kThreads, 0, st>>>(N, X, B, M, D, inv_t, shift, 0, sumexp, nullptr, rank,
                                                                                          nullptr, lq_x, nullptr, ent_c, ent_x, diag);
  }, vec_ok(N, D) && vec_ok(X, D), lq_x != nullptr, ent_c != nullptr);
  TT_LAUNCH_CHECK();
  return TT_OK;
}

int tt_score_dir_bwd_xneg(tt_ctx* ctx, const float* A, const float* Bm, int64_t Ra, int64_t Rb, int32_t D, float inv_t, float shift,
                          int32_t x_is_b, const int32_t* ent_a, const int32_t* ent_b, const float* lq_x, const float* rowsum,
                          const float* d_loss, float scale, int32_t accumulate, float* dA, tt_stream stream) {
  TT_CHECK_ARG(ctx && A && Bm && rowsum && d_loss && dA, "tt_score_dir_bwd_xneg: NULL argument");
  TT_CHECK_ARG(Ra >= 1 && Rb >= 1 && D >= 1, "tt_score_dir_bwd_xneg: bad shape");
  TT_CHECK_ARG((ent_a != nullptr) == (ent_b != nullptr), "tt_score_dir_bwd_xneg: ent_a and ent_b go together");
  if (D > 4 * DK) {
    tt_set_error("tt_score_dir_bwd_xneg: D=%d > %d not supported", D, 4 * DK);
    return TT_ERR_UNSUPPORTED;
  }
  if (2.f * fabsf(inv_t) > (lq_x ? kLqMaxTwoInvT : 80.f)) {
    tt_set_error("tt_score_dir_bwd_xneg: 1/temperature = %g: needs 2/T <= %g", inv_t, lq_x ? kLqMaxTwoInvT : 80.f);
    return TT_ERR_UNSUPPORTED;
  }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const float* const se_a = x_is_b ? rowsum : nullptr;     // the notices' side carries the reciprocal, the extras' side the weight
  const float* const se_b = x_is_b ? nullptr : rowsum;
  const float* const lq_a = x_is_b ? nullptr : lq_x;
  const float* const lq_b = x_is_b ? lq_x : nullptr;
  const float* const acc_flag = accumulate ? d_loss : nullptr;   // (the kernel's pw_g slot: non-NULL = add to dA)
  const auto go = [&](auto nch) {
    tt_dispatch([&](auto vec, auto lq, auto mk) {
      score_dir_bwd_kernel<nch, vec, lq, mk, false, true><<<(unsigned)tt_cdiv(Ra, RB), kThreads, 0, st>>>(
          A, Bm, Ra, Rb, D, inv_t, shift, 0, se_a, se_b, d_loss, scale, dA, lq_a, lq_b, ent_a, ent_b, acc_flag);
    }, vec_ok(A, D) && vec_ok(Bm, D), lq_x != nullptr, ent_a != nullptr);
  };
  switch ((D + DK - 1) / DK) {
    case 1: go(tt_c<1>); break;
    case 2: go(tt_c<2>); break;
    case 3: go(tt_c<3>); break;
    default: go(tt_c<4>); break;
  }
  TT_LAUNCH_CHECK();
  return TT_OK;
}

// the pair-weight entries of the f32 parity path: g from tt_score_prepare_pw; ids and logQ vectors optional
int tt_score_loss_finish_pw(tt_ctx* ctx, int64_t B, float shift, const float* g, const float* lq_n, const float* lq_c,
                            const float* rowsum, const float* colsum, const float* diag, const int32_t* row_rank,
                            const int32_t* col_rank, const float* sumscore, float* out8, float* loss_out, tt_stream stream) {
  TT_CHECK_ARG(ctx && g && rowsum && colsum && diag && row_rank && col_rank && out8, "tt_score_loss_finish_pw: NULL argument");
  TT_CHECK_ARG((lq_n != nullptr) == (lq_c != nullptr), "tt_score_loss_finish_pw: lq_n and lq_c go together");
  TT_CHECK_ARG(B >= 1, "tt_score_loss_finish_pw: B < 1");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  tt_dispatch([&](auto lq) {
    loss_finish_pw_kernel<lq><<<1, 1024, 0, st>>>(B, shift, rowsum, colsum, diag, row_rank, col_rank, sumscore, out8, loss_out, lq_n, lq_c, g);
  }, lq_n != nullptr);
  TT_LAUNCH_CHECK();
  return TT_OK;
}

int tt_score_dir_bwd_pw(tt_ctx* ctx, const float* A, const float* Bm, int64_t Ra, int64_t Rb, int32_t D, float inv_t, float shift,
                        int64_t diag_offset, const float* g, const int32_t* ent_n, const int32_t* ent_c, const float* lq_a,
                        const float* lq_b, const float* sumexp_a, const float* sumexp_b, const float* d_loss, float scale, float* dA,
                        tt_stream stream) {
  TT_CHECK_ARG(ctx && A && Bm && g && sumexp_a && sumexp_b && d_loss && dA, "tt_score_dir_bwd_pw: NULL argument");
  TT_CHECK_ARG((ent_n != nullptr) == (ent_c != nullptr), "tt_score_dir_bwd_pw: ent_n and ent_c go together");
  TT_CHECK_ARG((lq_a != nullptr) == (lq_b != nullptr), "tt_score_dir_bwd_pw: lq_a and lq_b go together");
  TT_CHECK_ARG(Ra >= 1 && Rb >= 1 && D >= 1, "tt_score_dir_bwd_pw: bad shape");
  if (D > 4 * DK) {
    tt_set_error("tt_score_dir_bwd_pw: D=%d > %d not supported", D, 4 * DK);
    return TT_ERR_UNSUPPORTED;
  }
  if (Ra != Rb || diag_offset != 0) {
    tt_set_error("tt_score_dir_bwd_pw: pair weights cover the square problem only (Ra == Rb, diag_offset == 0)");
    return TT_ERR_UNSUPPORTED;
  }
  if (2.f * fabsf(inv_t) > (lq_a ? kLqMaxTwoInvT : 80.f)) {
    tt_set_error("tt_score_dir_bwd_pw: 1/temperature = %g: needs 2/T <= %g", inv_t, lq_a ? kLqMaxTwoInvT : 80.f);
    return TT_ERR_UNSUPPORTED;
  }
  return dir_bwd(A, Bm, Ra, Rb, D, inv_t, shift, diag_offset, lq_a, lq_b, sumexp_a, sumexp_b, d_loss, scale, dA, stream, ent_n, ent_c, g);
}

int tt_score_matrix(tt_ctx* ctx, const float* A, const float* Bm, int64_t Ra, int64_t Rb, int32_t D, float inv_t, float* S,
                    int64_t lds, tt_stream stream) {
  TT_CHECK_ARG(ctx && (Ra == 0 || Rb == 0 || (A && Bm && S)), "tt_score_matrix: NULL argument");
  TT_CHECK_ARG(Ra >= 0 && Rb >= 0 && D >= 1 && lds >= Rb, "tt_score_matrix: bad shape");
  TT_CHECK_ARG(Ra < ((int64_t)1 << 31) && Rb < ((int64_t)1 << 31), "tt_score_matrix: too many rows");
  return tt_gemm_nt(reinterpret_cast<hipStream_t>(stream), A, D, Bm, D, nullptr, S, lds, Ra, Rb, D, false, inv_t);
}

int tt_diag_rank_rows(tt_ctx* ctx, const float* S, int64_t R, int64_t Ccols, int64_t lds, int64_t diag_offset, int32_t* rank,
                      tt_stream stream) {
  TT_CHECK_ARG(ctx && (R == 0 || (S && rank)), "tt_diag_rank_rows: NULL argument");
  TT_CHECK_ARG(R >= 0 && Ccols >= 1 && lds >= Ccols, "tt_diag_rank_rows: bad shape");
  if (R == 0) return TT_OK;
  diag_rank_rows_kernel<<<(unsigned)tt_cdiv(R, 4), kThreads, 0, reinterpret_cast<hipStream_t>(stream)>>>(S, R, Ccols, lds, diag_offset, rank);
  TT_LAUNCH_CHECK();
  return TT_OK;
}

int tt_topk_rows(tt_ctx* ctx, const float* S, int64_t R, int64_t Ccols, int64_t lds, int32_t k, float* vals, int64_t* idx,
                 tt_stream stream) {
  TT_CHECK_ARG(ctx && (R == 0 || (S && vals && idx)), "tt_topk_rows: NULL argument");
  TT_CHECK_ARG(R >= 0 && Ccols >= 1 && lds >= Ccols, "tt_topk_rows: bad shape");
  TT_CHECK_ARG(k >= 1 && k <= 64 && k <= Ccols, "tt_topk_rows: k=%d not in [1, min(64, %lld)]", k, (long long)Ccols);
  if (R == 0) return TT_OK;
  topk_rows_kernel<<<(unsigned)tt_cdiv(R, 4), kThreads, 0, reinterpret_cast<hipStream_t>(stream)>>>(S, R, Ccols, lds, k, vals, idx);
  TT_LAUNCH_CHECK();
  return TT_OK;
}

size_t tt_score_dense_workspace_bytes(int64_t B, int32_t D) {
  if (B < 1 || D < 1) return 0;
  return tt_gemm_tn_workspace_bytes(B, D, B) + 256;
}

int tt_score_dense_fwd(tt_ctx* ctx, const float* N, const float* Cm, int64_t B, int32_t D, float inv_t, int32_t loss_type,
                       float label_smoothing, float* S, float* stats, int32_t* hit, float* out8, float* loss_out, tt_stream stream) {
  TT_CHECK_ARG(ctx && N && Cm && S && stats && hit && out8, "tt_score_dense_fwd: NULL argument");
  TT_CHECK_ARG(B >= 1 && B < ((int64_t)1 << 24) && D >= 1, "tt_score_dense_fwd: bad shape");
  TT_CHECK_ARG(loss_type == 0 || loss_type == 1, "tt_score_dense_fwd: loss_type %d (0 = cross entropy, 1 = cosine embedding)", loss_type);
  TT_CHECK_ARG(label_smoothing >= 0.f && label_smoothing <= 1.f, "tt_score_dense_fwd: label_smoothing not in [0, 1]");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (int rc = tt_gemm_nt(st, N, D, Cm, D, nullptr, S, B, B, B, D, false, inv_t)) return rc;
  dense_row_stats_kernel<<<(unsigned)tt_cdiv(B, kThreads / 64), kThreads, 0, st>>>(S, B, stats, stats + B, stats + 4 * B, stats + 5 * B, hit);
  TT_LAUNCH_CHECK();
  dense_col_stats_kernel<<<(unsigned)tt_cdiv(B, kThreads), kThreads, 0, st>>>(S, B, stats + 2 * B, stats + 3 * B, hit + B);
  TT_LAUNCH_CHECK();
  dense_finish_kernel<<<1, 1024, 0, st>>>(B, loss_type, label_smoothing, stats, hit, out8, loss_out);
  TT_LAUNCH_CHECK();
  return TT_OK;
}

int tt_score_dense_bwd(tt_ctx* ctx, const float* N, const float* Cm, int64_t B, int32_t D, float inv_t, int32_t loss_type,
                       float label_smoothing, float* S, const float* stats, const float* d_loss, float* dN, float* dC,
                       void* workspace, size_t workspace_bytes, tt_stream stream) {
  TT_CHECK_ARG(ctx && N && Cm && S && stats && d_loss && dN && dC && workspace, "tt_score_dense_bwd: NULL argument");
  TT_CHECK_ARG(B >= 1 && D >= 1 && (loss_type == 0 || loss_type == 1), "tt_score_dense_bwd: bad arguments");
  if (workspace_bytes < tt_score_dense_workspace_bytes(B, D)) {
    tt_set_error("tt_score_dense_bwd: workspace %zu < required %zu", workspace_bytes, tt_score_dense_workspace_bytes(B, D));
    return TT_ERR_WORKSPACE;
  }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  int64_t blocks = tt_cdiv(B * B, kThreads);
  if (blocks > 8192) blocks = 8192;
  dense_grad_kernel<<<(unsigned)blocks, kThreads, 0, st>>>(S, B, loss_type, label_smoothing, inv_t, stats, d_loss);
  TT_LAUNCH_CHECK();
  GemmNN nn{S, B, Cm, D, dN, D, B, D, B};                                 // dN = dS . C
  if (int rc = tt_gemm_nn_batched(st, &nn, 1)) return rc;
  GemmTN tn{S, B, N, D, dC, D, B, D, B, workspace, workspace_bytes, nullptr};       // dC = dS^T . N
  return tt_gemm_tn_batched(st, &tn, 1);
}

}  // extern "C"
