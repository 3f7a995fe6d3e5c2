// Tower MLP (BaseTower.forward after the lookup, and its backward): Linear layers on the f32 MFMA
// GEMM tiles of tt_gemm.hip, BatchNorm1d statistics as deterministic two-stage column reductions,
// ReLU / BN / dropout / L2-normalise as fused elementwise and row-wise kernels.
#include "tt_deferred.h"
#include "tt_tail_bwd.h"

namespace {

using namespace tttail;   // Batch, ColArgs, dropout_scale, seed_of, mul_rn, the tail tiles' constants, TailBwdArgs (tt_tail_bwd.h)

constexpr int kThreads = 256;
// (column statistics of relu(pre) -- Wf, wf_combine, the canonical merge order wf_lane_merge, kMaxChunks -- live in tt_riders.h:
// the statistics rider in the keyed sort's launch shares them)

// grid (colblocks of 64, nchunks, towers); thread = (column, row-lane of 4)
struct BnStatArgs {
  const float* pre; int B, H, rows_per_chunk, nchunks; float* partial; float* mean; float* rstd; float* rm; float* rv; int64_t* nbt;
  int64_t pstride = 0;   // floats between chunks when READING partial (0 = 3 * H); chunks are always written densely
};

__global__ __launch_bounds__(kThreads) void bn_stats_partial_kernel(Batch<BnStatArgs> batch) {
  const BnStatArgs& a = batch.a[blockIdx.z];
  const int H = a.H;
  if ((int)blockIdx.x * 64 >= H || (int)blockIdx.y >= a.nchunks) return;
  __shared__ Wf sh[4][64];
  const int c = blockIdx.x * 64 + (threadIdx.x & 63), rl = threadIdx.x >> 6;
  const int r0 = blockIdx.y * a.rows_per_chunk, r1 = min(a.B, r0 + a.rows_per_chunk);
  // per thread: sums of (x - x0) and (x - x0)^2 over its <= a few dozen rows, x0 = its first value (no division
  // and no dependent chain per element; the shift keeps the tiny-sample variance free of cancellation), turned
  // into (n, mean, M2) once and merged with Chan's formula from there on
  Wf w{0.f, 0.f, 0.f};
  if (c < H && r0 + rl < r1) {
    const float x0 = fmaxf(a.pre[(int64_t)(r0 + rl) * H + c], 0.f);
    float s = 0.f, q = 0.f, cnt = 0.f;
#pragma unroll 16
    for (int r = r0 + rl; r < r1; r += 4) {
      const float d = fmaxf(a.pre[(int64_t)r * H + c], 0.f) - x0;
      s += d;
      q += d * d;
      cnt += 1.f;
    }
    w.n = cnt;
    w.mean = x0 + s / cnt;
    w.m2 = fmaxf(q - s * (s / cnt), 0.f);
  }
  sh[rl][threadIdx.x & 63] = w;
  __syncthreads();
  if (rl == 0 && c < H) {
    Wf o = sh[0][threadIdx.x];
    o = wf_combine(o, sh[1][threadIdx.x]);
    o = wf_combine(o, sh[2][threadIdx.x]);
    o = wf_combine(o, sh[3][threadIdx.x]);
    float* p = a.partial + (int64_t)blockIdx.y * 3 * H;
    p[c] = o.n; p[H + c] = o.mean; p[2 * H + c] = o.m2;
  }
}

// finish: workgroup = 64 columns x 4 chunk-lanes; lane j combines chunks j, j+4, ... (all loads first), then the
// four partial results are combined in lane order (fixed order => reproducible)
__global__ __launch_bounds__(kThreads) void bn_stats_finish_kernel(Batch<BnStatArgs> batch) {
  const BnStatArgs& a = batch.a[blockIdx.y];
  const int H = a.H;
  if ((int)blockIdx.x * 64 >= H) return;
  __shared__ Wf sh[4][64];
  const int c = blockIdx.x * 64 + (threadIdx.x & 63), jl = threadIdx.x >> 6;
  Wf o{0.f, 0.f, 0.f};
  if (c < H) {
    Wf v[kMaxChunks / 4];
#pragma unroll
    for (int i = 0; i < kMaxChunks / 4; ++i) {
      const int k = jl + 4 * i;
      const float* p = a.partial + (int64_t)k * (a.pstride ? a.pstride : 3 * H);
      v[i] = k < a.nchunks ? Wf{p[c], p[H + c], p[2 * H + c]} : Wf{0.f, 0.f, 0.f};
    }
    o = wf_lane_merge(v);
  }
  sh[jl][threadIdx.x & 63] = o;
  __syncthreads();
  if (jl != 0 || c >= H) return;
  o = wf_combine(wf_combine(sh[0][threadIdx.x], sh[1][threadIdx.x]), wf_combine(sh[2][threadIdx.x], sh[3][threadIdx.x]));
  const float var = o.n > 0.f ? o.m2 / o.n : 0.f;
  a.mean[c] = o.mean;
  a.rstd[c] = 1.f / sqrtf(var + kBnEps);
  if (a.rm) {   // nn.BatchNorm1d: momentum 0.1, unbiased variance in the running estimate
    a.rm[c] = (1.f - kBnMomentum) * a.rm[c] + kBnMomentum * o.mean;
    a.rv[c] = (1.f - kBnMomentum) * a.rv[c] + kBnMomentum * (o.n > 1.f ? o.m2 / (o.n - 1.f) : var);
  }
  if (a.nbt && c == 0) a.nbt[0] += 1;
}

__global__ void bn_eval_prepare_kernel(Batch<BnStatArgs> batch) {
  const BnStatArgs& a = batch.a[blockIdx.y];
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < a.H) {
    a.mean[c] = a.rm[c];
    a.rstd[c] = 1.f / sqrtf(a.rv[c] + kBnEps);
  }
}

struct BnApplyArgs {
  const float* pre; int64_t total; int H; const float* mean; const float* rstd; const float* g; const float* b;
  uint64_t salt; float* act;
};

__global__ __launch_bounds__(kThreads) void bn_apply_kernel(Batch<BnApplyArgs> batch, bool drop, float p, uint64_t seed0,
                                                           const uint64_t* __restrict__ seed_dev) {
  const BnApplyArgs& a = batch.a[blockIdx.y];
  const uint64_t seed = drop ? seed_of(seed0, seed_dev) : 0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int H = a.H;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.total; i += stride) {
    const int c = (int)(i % H);
    const float x = fmaxf(a.pre[i], 0.f);
    const float y = (x - a.mean[c]) * a.rstd[c] * a.g[c] + a.b[c];
    a.act[i] = y * dropout_scale(drop, p, seed, a.salt + (uint64_t)i);
  }
}

// ---- deterministic two-stage column sums of the BatchNorm backward (ColArgs: tt_tail_bwd.h) -------

__global__ __launch_bounds__(kThreads) void colsum_partial_kernel(Batch<ColArgs> batch, bool drop, float p, uint64_t seed0,
                                                                 const uint64_t* __restrict__ seed_dev) {
  const ColArgs& a = batch.a[blockIdx.z];
  const int H = a.H;
  if ((int)blockIdx.x * 64 >= H || (int)blockIdx.y >= a.nchunks) return;
  __shared__ float sh[2][4][64];
  const int c = blockIdx.x * 64 + (threadIdx.x & 63), rl = threadIdx.x >> 6;
  const int r0 = blockIdx.y * a.rows_per_chunk, r1 = min(a.B, r0 + a.rows_per_chunk);
  float s0 = 0.f, s1 = 0.f;
  const uint64_t seed = drop ? seed_of(seed0, seed_dev) : 0;
  if (c < H) {
#pragma unroll 16
    for (int r = r0 + rl; r < r1; r += 4) {
      const int64_t i = (int64_t)r * H + c;
      const float da = a.x[(int64_t)r * a.ldx + c] * dropout_scale(drop, p, seed, a.salt + (uint64_t)i);
      const float xh = (fmaxf(a.pre[i], 0.f) - a.mean[c]) * a.rstd[c];
      s0 += da;
      s1 += da * xh;
    }
  }
  sh[0][rl][threadIdx.x & 63] = s0;
  sh[1][rl][threadIdx.x & 63] = s1;
  __syncthreads();
  if (rl == 0 && c < H) {
    float* q = a.partial + (int64_t)blockIdx.y * 2 * H;
    q[c] = ((sh[0][0][threadIdx.x] + sh[0][1][threadIdx.x]) + sh[0][2][threadIdx.x]) + sh[0][3][threadIdx.x];
    q[H + c] = ((sh[1][0][threadIdx.x] + sh[1][1][threadIdx.x]) + sh[1][2][threadIdx.x]) + sh[1][3][threadIdx.x];
  }
}

__global__ __launch_bounds__(kThreads) void colsum_finish_kernel(Batch<ColArgs> batch) {
  const ColArgs& a = batch.a[blockIdx.y];
  const int H = a.H;
  if ((int)blockIdx.x * 64 >= H) return;
  __shared__ float sh[2][4][64];
  const int c = blockIdx.x * 64 + (threadIdx.x & 63), jl = threadIdx.x >> 6;
  float s0 = 0.f, s1 = 0.f;
  if (c < H) {
    float v0[kMaxChunks / 4], v1[kMaxChunks / 4];
#pragma unroll
    for (int i = 0; i < kMaxChunks / 4; ++i) {
      const int k = jl + 4 * i;
      const float* q = a.partial + (int64_t)k * (a.pstride ? a.pstride : 2 * H);
      v0[i] = k < a.nchunks ? q[c] : 0.f;
      v1[i] = k < a.nchunks ? q[H + c] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < kMaxChunks / 4; ++i) { s0 += v0[i]; s1 += v1[i]; }
  }
  sh[0][jl][threadIdx.x & 63] = s0;
  sh[1][jl][threadIdx.x & 63] = s1;
  __syncthreads();
  if (jl != 0 || c >= H) return;
  const float t0 = (sh[0][0][threadIdx.x] + sh[0][1][threadIdx.x]) + (sh[0][2][threadIdx.x] + sh[0][3][threadIdx.x]);
  const float t1 = (sh[1][0][threadIdx.x] + sh[1][1][threadIdx.x]) + (sh[1][2][threadIdx.x] + sh[1][3][threadIdx.x]);
  a.out0[c] = t0 * a.out_scale;
  a.out1[c] = t1 * a.out_scale;
  if (a.sums_raw) { a.sums_raw[c] = t0; a.sums_raw[H + c] = t1; }
}

// BN backward apply, in place on the gradient buffer:  d_act -> d_pre
//   train: d_a = g rstd (da - S1/B - xhat S2/B)   eval: d_a = da g rstd ;   d_pre = d_a [pre > 0]
struct BnBwdArgs {
  float* d; const float* pre; int64_t total; int H; float invB;
  const float* mean; const float* rstd; const float* g; const float* S1; const float* S2; uint64_t salt;
};

__global__ __launch_bounds__(kThreads) void bn_bwd_apply_kernel(Batch<BnBwdArgs> batch, bool train, bool drop, float p, uint64_t seed0,
                                                               const uint64_t* __restrict__ seed_dev) {
  const BnBwdArgs& a = batch.a[blockIdx.y];
  const uint64_t seed = drop ? seed_of(seed0, seed_dev) : 0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int H = a.H;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.total; i += stride) {
    const int c = (int)(i % H);
    const float pr = a.pre[i];
    const float da = a.d[i] * dropout_scale(drop, p, seed, a.salt + (uint64_t)i);
    float dv;
    if (train) {
      const float xh = (fmaxf(pr, 0.f) - a.mean[c]) * a.rstd[c];
      dv = a.g[c] * a.rstd[c] * (da - a.S1[c] * a.invB - xh * (a.S2[c] * a.invB));
    } else {
      dv = da * a.g[c] * a.rstd[c];
    }
    a.d[i] = pr > 0.f ? dv : 0.f;
  }
}

// ---- row-wise L2 normalise: one wave per row ---------------------------------------------------
__device__ __forceinline__ float wave_sum(float x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
  return x;
}

struct NormArgs { const float* y; const float* emb_in; const float* d_emb; int B, D; float* out; };

__global__ __launch_bounds__(kThreads) void l2norm_fwd_kernel(Batch<NormArgs> batch) {
  const NormArgs& a = batch.a[blockIdx.y];
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63, D = a.D;
  if (row >= a.B) return;
  float ss = 0.f;
  for (int c = lane; c < D; c += 64) {
    const float v = a.y[(int64_t)row * D + c];
    ss += v * v;
  }
  const float den = fmaxf(sqrtf(wave_sum(ss)), kNormEps);
  for (int c = lane; c < D; c += 64) a.out[(int64_t)row * D + c] = a.y[(int64_t)row * D + c] / den;
}

__global__ __launch_bounds__(kThreads) void l2norm_bwd_kernel(Batch<NormArgs> batch) {
  const NormArgs& a = batch.a[blockIdx.y];
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63, D = a.D;
  if (row >= a.B) return;
  float ss = 0.f, dot = 0.f;
  for (int c = lane; c < D; c += 64) {
    const int64_t i = (int64_t)row * D + c;
    ss += a.y[i] * a.y[i];
    dot += a.emb_in[i] * a.d_emb[i];
  }
  const float nrm = sqrtf(wave_sum(ss));
  dot = wave_sum(dot);
  const float den = fmaxf(nrm, kNormEps);
  for (int c = lane; c < D; c += 64) {
    const int64_t i = (int64_t)row * D + c;
    a.out[i] = nrm > kNormEps ? (a.d_emb[i] - a.emb_in[i] * dot) / den : a.d_emb[i] / den;
  }
}

// The same arithmetic (same per-lane column sets, same fma chains, same butterflies: bit-identical) for widths that are a
// multiple of 64 up to 256, with RW rows per wave whose loads are all issued before the first reduction -- the one-row-at-a-time
// kernels above keep 1-4 loads in flight per lane and stream at 1.9 TB/s (B = 65536, D = 256: 72 / 107 us per tower).
template <int NC, int RW>
__global__ __launch_bounds__(kThreads) void l2norm_fwd_fast_kernel(Batch<NormArgs> batch) {
  const NormArgs& a = batch.a[blockIdx.y];
  const int lane = threadIdx.x & 63, D = 64 * NC;
  const int row0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * RW;
  if (row0 >= a.B) return;
  float v[RW][NC];
#pragma unroll
  for (int r = 0; r < RW; ++r)
#pragma unroll
    for (int j = 0; j < NC; ++j) v[r][j] = row0 + r < a.B ? a.y[(int64_t)(row0 + r) * D + lane + 64 * j] : 0.f;
#pragma unroll
  for (int r = 0; r < RW; ++r) {
    float ss = mul_rn(v[r][0], v[r][0]);
#pragma unroll
    for (int j = 1; j < NC; ++j) ss = __builtin_fmaf(v[r][j], v[r][j], ss);
    const float den = fmaxf(sqrtf(wave_sum(ss)), kNormEps);
    if (row0 + r < a.B) {
#pragma unroll
      for (int j = 0; j < NC; ++j) a.out[(int64_t)(row0 + r) * D + lane + 64 * j] = v[r][j] / den;
    }
  }
}

template <int NC, int RW>
__global__ __launch_bounds__(kThreads) void l2norm_bwd_fast_kernel(Batch<NormArgs> batch) {
  const NormArgs& a = batch.a[blockIdx.y];
  const int lane = threadIdx.x & 63, D = 64 * NC;
  const int row0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * RW;
  if (row0 >= a.B) return;
  float y[RW][NC], e[RW][NC], d[RW][NC];
#pragma unroll
  for (int r = 0; r < RW; ++r)
#pragma unroll
    for (int j = 0; j < NC; ++j) {
      const bool ok = row0 + r < a.B;
      const int64_t i = (int64_t)(row0 + r) * D + lane + 64 * j;
      y[r][j] = ok ? a.y[i] : 0.f;
      e[r][j] = ok ? a.emb_in[i] : 0.f;
      d[r][j] = ok ? a.d_emb[i] : 0.f;
    }
#pragma unroll
  for (int r = 0; r < RW; ++r) {
    float ss = mul_rn(y[r][0], y[r][0]), dot = mul_rn(e[r][0], d[r][0]);
#pragma unroll
    for (int j = 1; j < NC; ++j) {
      ss = __builtin_fmaf(y[r][j], y[r][j], ss);
      dot = __builtin_fmaf(e[r][j], d[r][j], dot);
    }
    const float nrm = sqrtf(wave_sum(ss));
    dot = wave_sum(dot);
    const float den = fmaxf(nrm, kNormEps);
    if (row0 + r < a.B) {
#pragma unroll
      for (int j = 0; j < NC; ++j)
        a.out[(int64_t)(row0 + r) * D + lane + 64 * j] = nrm > kNormEps ? (d[r][j] - e[r][j] * dot) / den : d[r][j] / den;
    }
  }
}

// widths of all towers of the batch equal and in {64, 128, 192, 256}: the multi-row kernels
template <bool BWD>
static bool launch_l2norm_fast(hipStream_t st, const Batch<NormArgs>& na, int n, int64_t B) {
  const int D = na.a[0].D;
  for (int t = 1; t < n; ++t)
    if (na.a[t].D != D || na.a[t].B != na.a[0].B) return false;
  if (D % 64 != 0 || D < 64 || D > 256) return false;
  constexpr int RW = BWD ? 2 : 4;
  const dim3 grid((unsigned)tt_cdiv(B, 4 * RW), (unsigned)n);
  auto launch = [&](auto kernel) { kernel<<<grid, kThreads, 0, st>>>(na); };
#define TT_L2(NC)                                        \
  do {                                                   \
    if (BWD) launch(l2norm_bwd_fast_kernel<NC, RW>);     \
    else launch(l2norm_fwd_fast_kernel<NC, RW>);         \
  } while (0)
  switch (D / 64) {
    case 1: TT_L2(1); break;
    case 2: TT_L2(2); break;
    case 3: TT_L2(3); break;
    default: TT_L2(4); break;
  }
#undef TT_L2
  return true;
}

// ---- fused narrow tail -------------------------------------------------------------------------
// When the last hidden block and the output are at most 64 wide (the [128, 64] towers of the reference's config)
// everything after the block's Linear is a few MB of data in a chain of ~5 us launches: slab reduction, BN
// statistics (2), BN apply, the 64x64 output Linear, L2 normalise -- and the mirror image in the backward pass.
// Training with bf16 GEMM operands, that chain runs as two kernels per pass (the split is the batch-wide reduction
// of the BN statistics).  Arithmetic and summation order follow the unfused kernels above step for step (the forward
// and the BN gradients come out bit-identical); only the output-layer weight / bias gradients are summed over
// different row chunks.  Workgroups of 1024 threads cover 64 rows: thread (c, rq) = column c, rows rq + 16 j; the
// ordered column reductions run on the first 256 threads (c, rl) exactly as in the unfused kernels.
constexpr int kTailThreads = 1024;

// (A) finish the split-K block GEMM (slabs + bias -> pre) and take the per-chunk BN statistics of relu(pre) in the same
// pass over the rows: slab_reduce_kernel + bn_stats_partial_kernel.  grid (nchunks, towers)
struct HeadArgs { const float* slabs; int64_t slab_stride; int splits; const float* bias; float* pre; BnStatArgs s; };

__global__ __launch_bounds__(kTailThreads) void tail_head_kernel(Batch<HeadArgs> batch) {
  const HeadArgs& h = batch.a[blockIdx.y];
  const BnStatArgs& a = h.s;
  const int H = a.H;
  if ((int)blockIdx.x >= a.nchunks) return;
  __shared__ float X[64 * kTailLdF];
  __shared__ Wf sh[4][64];
  const int t = threadIdx.x, c = t & 63, rq = t >> 6;
  const int r0 = blockIdx.x * a.rows_per_chunk, r1 = min(a.B, r0 + a.rows_per_chunk);
  const float bias = (h.bias && c < H) ? h.bias[c] : 0.f;
  float x0 = 0.f, s = 0.f, q = 0.f, cnt = 0.f;
  for (int b0 = r0; b0 < r1; b0 += 64) {
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (c < H) {
#pragma unroll 4
      for (int z = 0; z < h.splits; ++z) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int r = b0 + rq + 16 * j;
          if (r < r1) v[j] += h.slabs[(int64_t)z * h.slab_stride + (int64_t)r * H + c];
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int row = rq + 16 * j, r = b0 + row;
        if (r < r1) {
          const float o = v[j] + bias;
          h.pre[(int64_t)r * H + c] = o;
          X[row * kTailLdF + c] = fmaxf(o, 0.f);
        }
      }
    }
    __syncthreads();
    if (t < 256 && c < H) {               // rq = row lane: rows r0 + rq, + 4, ... in bn_stats_partial_kernel's order
      const int nrow = min(64, r1 - b0);
      for (int row = rq; row < nrow; row += 4) {
        const float xv = X[row * kTailLdF + c];
        if (cnt == 0.f) x0 = xv;
        const float d = xv - x0;
        s += d;
        q += d * d;
        cnt += 1.f;
      }
    }
    __syncthreads();
  }
  if (t < 256) {
    Wf w{0.f, 0.f, 0.f};
    if (c < H && cnt > 0.f) {
      w.n = cnt;
      w.mean = x0 + s / cnt;
      w.m2 = fmaxf(q - s * (s / cnt), 0.f);
    }
    sh[rq][c] = w;
  }
  __syncthreads();
  if (t < 64 && c < H) {
    Wf o = sh[0][c];
    o = wf_combine(o, sh[1][c]);
    o = wf_combine(o, sh[2][c]);
    o = wf_combine(o, sh[3][c]);
    float* p = a.partial + (int64_t)blockIdx.x * 3 * H;
    p[c] = o.n; p[H + c] = o.mean; p[2 * H + c] = o.m2;
  }
}

// (A') the whole front of a one-block tower in ONE launch: dense projection (x[:, 0:h0] = dense . W_proj^T + b_proj, stored
// bf16), the block's Linear over x = [projection | looked-up rows] and the chunk BN statistics of relu(pre) -- the
// projection GEMM, the split-K block GEMM and tail_head_kernel above (3 dependent launches, 12.6 + 12.6 + 9.4 us at
// B = 8192: 77 MB of traffic of which 34 MB are split-K slabs written and read back).  One 512-thread workgroup per
// 64-row block (the BN chunks).  Operands go through LDS in 128-wide k stages: every thread loads 16-byte pieces of whole
// rows (coalesced: a fragment-shaped load straight from global memory -- one row per lane -- was tried first and ran at a
// quarter of the texture-address rate, 50 us), rounds f32 to bf16 on the way in, and the loads run THREE stages ahead of
// the MFMAs in registers -- all unconditional (a piece past the end re-reads the thread's own first piece and is zeroed),
// so the compiler can count them.  Bound: a CU draws L2-resident bytes at ~70 GB/s (MI355X_MICROARCH.md) and every
// workgroup re-reads its tower's f32 weights -- 426 KB of the 637 KB a notice workgroup moves: ~9 us.  The block GEMM's first stages are requested before the projection is computed.  K is split over the
// waves of the block GEMM (4 tiles x 2 k-halves; the projection's 8 tiles take a wave each), the partial tiles are added
// through LDS in a fixed order: reproducible, but not bit-identical to the split-K GEMM path.  The projection tile goes to x AND stays in
// LDS as the block GEMM's operand for k < h0.
// Needs: din <= 256, din and h0 + K E multiples of 64, h0 a multiple of 32 and <= 128, H <= 64.  grid (nchunks, towers)
struct FrontArgs {
  const float* dense; int64_t ld_dense; int din;
  const float* w_proj; const float* b_proj; int h0;
  uint16_t* x; int64_t ldx; int kx;
  const float* w; const float* bias; float* pre;
  BnStatArgs s;
  const uint16_t* w_proj16; const uint16_t* w16;   // W16: bf16 shadows of w_proj / w (tt_tower_params.w_proj_bf16 / w_bf16)
  const float* table; const int32_t* rows; int K, E;   // GATHER: the table, this side's fused rows [B][K] (slot order), keys, row width
};
constexpr int kFS = 136;                                         // bf16 elements per LDS row of a 128-wide k stage
constexpr int kFrontThreads = 512;                               // 8 waves at up to 256 registers: three stages of loads in flight
constexpr int kFrontA = 64 * kFS * 2, kFrontB = 128 * kFS * 2;   // bytes of one A / B stage buffer
constexpr int kFrontLds = 2 * kFrontA + 2 * kFrontB + kFrontA + 4 * 64 * 12;
constexpr int kFrontLdsMax = 160 * 1024;                         // with the GATHER form's index tile (64 x K fused rows) behind it

using tl_bf16x4 = __attribute__((ext_vector_type(4))) __bf16;
__device__ __forceinline__ void front_put4(__bf16* dst, const float4& v, bool live) {
  tl_bf16x4 o;
  o[0] = (__bf16)(live ? v.x : 0.f); o[1] = (__bf16)(live ? v.y : 0.f);
  o[2] = (__bf16)(live ? v.z : 0.f); o[3] = (__bf16)(live ? v.w : 0.f);
  *reinterpret_cast<tl_bf16x4*>(dst) = o;
}

// uniform base + 32-bit byte offset: the global_load "saddr" form, one VGPR of address per load instead of two
template <typename T>
__device__ __forceinline__ T front_ld(const void* base, uint32_t off) {
  return *reinterpret_cast<const T*>(reinterpret_cast<const char*>(base) + off);
}

// W16 (round 4): the weights come as bf16 shadows -- pieces of 8 elements laid out like the x pieces (row (t >> 4) + 32 pass,
// k = 8 (t & 15)), copied into LDS as they are: 213 of the 637 KB a notice workgroup moved were the f32 halves of values it rounded
// to bf16 anyway, and the 112 registers of weight pieces in flight become 56 (no scratch).  Same bits in LDS, same results.
//
// GATHER: the embedding rows are gathered HERE instead of by a lookup launch in front (tt_embed_lookup_rows_fwd): the 16-byte
// piece of x at k >= h0 is 8 consecutive f32 of table row rows[b][(k - h0) / E], loaded as two float4 on the x pieces' schedule
// (three stages ahead, a dead piece re-reads a live address and is zeroed), rounded with tt_f2bf and packed as the lookup's
// 32-byte-lane store does on the way into the A stage -- the same bits in LDS -- and stored to x[:, h0:] by the thread that
// converted it: x stays the complete output gemm_back and the row gradients read, while the lookup's write of it, its write-back,
// this kernel's re-read and one launch go.  The block's 64 x K fused rows wait in an LDS tile behind the statistics area
// (one coalesced read, issued in front of the projection's loads).  E a power of two >= 8: a piece never straddles two rows.
template <bool W16, bool GATHER = false>
__global__ __launch_bounds__(kFrontThreads) void tower_front_kernel(Batch<FrontArgs> batch) {
  const FrontArgs& f = batch.a[blockIdx.y];
  const BnStatArgs& a = f.s;
  const int H = a.H, B = a.B, h0 = f.h0, din = f.din, kx = f.kx;
  if ((int)blockIdx.x >= a.nchunks) return;
  extern __shared__ __attribute__((aligned(16))) char front_smem[];
  __bf16* bufA = reinterpret_cast<__bf16*>(front_smem);                              // [2][64][kFS]
  __bf16* bufB = reinterpret_cast<__bf16*>(front_smem + 2 * kFrontA);                // [2][128][kFS]
  __bf16* Pt = reinterpret_cast<__bf16*>(front_smem + 2 * kFrontA + 2 * kFrontB);    // [64][kFS] projection tile
  Wf (*sh)[64] = reinterpret_cast<Wf (*)[64]>(front_smem + 3 * kFrontA + 2 * kFrontB);
  float* part = reinterpret_cast<float*>(bufB);                                      // partial tiles (after the MFMAs): 32 KB
  int32_t* idxs = reinterpret_cast<int32_t*>(front_smem + kFrontLds);                // GATHER: [64][K] fused rows of the block
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, li = lane & 31, lh = lane >> 5;
  const int c = t & 63, rq = t >> 6;
  const int r0 = blockIdx.x * a.rows_per_chunk, r1 = min(B, r0 + a.rows_per_chunk);
  const float bias = (f.bias && c < H) ? f.bias[c] : 0.f;
  // piece of an f32 stage: row (t >> 5) + 16 pass, k = 4 (t & 31); piece of a bf16 stage: row (t >> 4) + 32 pass, k = 8 (t & 15)
  const int frow = t >> 5, fk = 4 * (t & 31), xrow = t >> 4, xk = 8 * (t & 15);
  // ADDRESS columns of a thread's first piece: a 64-wide operand (din = 64, kx = 64) fills only half of the 128-wide first stage,
  // and the lanes of the other half must re-read columns that exist -- unclamped, their piece of the LAST row lay up to 256 bytes
  // behind the end of the buffer (harmless for the result: those columns are zeroed on the way into LDS; a fault when the
  // buffer ends a mapping)
  const int fkp = din >= 128 ? fk : (fk & 63), fkb = kx >= 128 ? fk : (fk & 63), xkb = kx >= 128 ? xk : (xk & 63);
  const int xkp = din >= 128 ? xk : (xk & 63);
  const int ns2 = 3 * ((kx + 383) / 384);                       // block stages, padded to the unroll of 3 (pad stages are zeros)
  const int pn = (wave >> 1) * 32 + li;                         // this lane's projection column
  const float bp = pn < h0 ? f.b_proj[pn] : 0.f;
  float x0 = 0.f, s = 0.f, q = 0.f, cnt = 0.f;
  const int gK = GATHER ? f.K : 0, gE = GATHER ? f.E : 8, gsh = __builtin_ctz(gE), gke = kx - h0;
  // GATHER: where this thread's piece `ps` of block stage `st` lies in the table (a dead piece -- below h0 or past kx -- reads
  // the piece of the sample's first key at the lane's own column: a live address, never ONE for the whole grid)
  auto gather_src = [&](int st, int ps) -> const float4* {
    const int kr = 128 * st + xk - h0;
    const int kk = (kr >= 0 && kr < gke) ? kr : (xk & (gE - 1));
    const int64_t row = idxs[(xrow + 32 * ps) * gK + (kk >> gsh)];
    return reinterpret_cast<const float4*>(f.table + row * gE + (kk & (gE - 1)));
  };
  for (int b0 = r0; b0 < r1; b0 += 64) {
    int32_t gi[4];                                          // GATHER: the block's fused rows, 512 per pass (past the batch: its last row's last key)
    if (GATHER) {
      const int64_t g0 = (int64_t)b0 * gK, glast = (int64_t)B * gK - 1;
#pragma unroll
      for (int j = 0; j < 4; ++j) gi[j] = f.rows[min(g0 + min(t + 512 * j, 64 * gK - 1), glast)];
    }
    // ---- everything that can be requested now: the projection's two stages, the block GEMM's first three ----
    constexpr int NPB = W16 ? 4 : 8, NQB = W16 ? 2 : 4;     // weight pieces per thread and stage: projection / block
    float4 pa[2][4], pb[2][NPB];                            // (W16: the float4 holds 8 bf16 -- moved, never computed on)
    uint32_t oa[4], ob[NPB];                                // byte offsets of this thread's rows (k = fk)
#pragma unroll
    for (int ps = 0; ps < 4; ++ps) oa[ps] = (uint32_t)(min(b0 + frow + 16 * ps, B - 1) * (int)f.ld_dense + fkp) * 4u;
#pragma unroll
    for (int ps = 0; ps < NPB; ++ps)
      ob[ps] = W16 ? (uint32_t)(min(xrow + 32 * ps, h0 - 1) * din + xkp) * 2u : (uint32_t)(min(frow + 16 * ps, h0 - 1) * din + fkp) * 4u;
#pragma unroll
    for (int st = 0; st < 2; ++st) {
      // a piece past the end re-reads this thread's own first piece (discarded): never ONE address for the whole grid
      const uint32_t ko = 128 * st + fk < din ? 512u * st : 0u;
      const uint32_t ko16 = 128 * st + xk < din ? 256u * st : 0u;
#pragma unroll
      for (int ps = 0; ps < 4; ++ps) pa[st][ps] = front_ld<float4>(f.dense, oa[ps] + ko);
#pragma unroll
      for (int ps = 0; ps < NPB; ++ps) pb[st][ps] = W16 ? front_ld<float4>(f.w_proj16, ob[ps] + ko16) : front_ld<float4>(f.w_proj, ob[ps] + ko);
    }
    uint4 qa[3][2];
    float4 qg[3][2][2];                                     // GATHER: the x pieces as the f32 they are gathered from
    float4 qb[3][NQB];
    uint32_t ox[2], ow[NQB];
    if (GATHER) {                                           // the index tile: every gather of this block reads it
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (t + 512 * j < 64 * gK) idxs[t + 512 * j] = gi[j];
      for (int i = t + 2048; i < 64 * gK; i += 512) idxs[i] = f.rows[min((int64_t)b0 * gK + i, (int64_t)B * gK - 1)];   // (K > 32)
      __syncthreads();
    }
#pragma unroll
    for (int ps = 0; ps < 2; ++ps) ox[ps] = (uint32_t)(min(b0 + xrow + 32 * ps, B - 1) * (int)f.ldx + xkb) * 2u;
#pragma unroll
    for (int ps = 0; ps < NQB; ++ps)
      ow[ps] = W16 ? (uint32_t)(min(xrow + 32 * ps, H - 1) * kx + xkb) * 2u : (uint32_t)(min(frow + 16 * ps, H - 1) * kx + fkb) * 4u;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int ka = 128 * u + xk, kb = 128 * u + fk;
#pragma unroll
      for (int ps = 0; ps < 2; ++ps) {
        if (GATHER) {
          qg[u][ps][0] = qg[u][ps][1] = float4{0.f, 0.f, 0.f, 0.f};
          if (128 * u + 128 > h0) {                         // (a stage wholly below h0 is the projection tile's: nothing to gather)
            const float4* src = gather_src(u, ps);
            qg[u][ps][0] = src[0]; qg[u][ps][1] = src[1];
          }
        } else {
          qa[u][ps] = front_ld<uint4>(f.x, ox[ps] + (ka < kx ? 256u * u : 0u));
        }
      }
#pragma unroll
      for (int ps = 0; ps < NQB; ++ps)
        qb[u][ps] = W16 ? front_ld<float4>(f.w16, ow[ps] + (ka < kx ? 256u * u : 0u)) : front_ld<float4>(f.w, ow[ps] + (kb < kx ? 512u * u : 0u));
    }
    __builtin_amdgcn_sched_barrier(0);                      // 36 loads in flight before the first one is waited for
    // ---- projection: wave = tile (rt, ct) of the 64 x h0 block, whole K ----
    {
      const int rt = wave & 1, ct = wave >> 1;
      tl_f32x16 acc;
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
      for (int st = 0; st < 2; ++st) {
        const bool live = 128 * st + fk < din, live16 = 128 * st + xk < din;
#pragma unroll
        for (int ps = 0; ps < 4; ++ps) front_put4(bufA + st * 64 * kFS + (frow + 16 * ps) * kFS + fk, pa[st][ps], live);
#pragma unroll
        for (int ps = 0; ps < NPB; ++ps) {
          if (W16) *reinterpret_cast<float4*>(bufB + st * 128 * kFS + (xrow + 32 * ps) * kFS + xk) = live16 ? pb[st][ps] : float4{0.f, 0.f, 0.f, 0.f};
          else front_put4(bufB + st * 128 * kFS + (frow + 16 * ps) * kFS + fk, pb[st][ps], live);
        }
      }
      {                                                     // third block stage, into the registers the projection just freed
        const int ka = 256 + xk, kb = 256 + fk;
#pragma unroll
        for (int ps = 0; ps < 2; ++ps) {
          if (GATHER) {
            const float4* src = gather_src(2, ps);
            qg[2][ps][0] = src[0]; qg[2][ps][1] = src[1];
          } else {
            qa[2][ps] = front_ld<uint4>(f.x, ox[ps] + (ka < kx ? 512u : 0u));
          }
        }
#pragma unroll
        for (int ps = 0; ps < NQB; ++ps)
          qb[2][ps] = W16 ? front_ld<float4>(f.w16, ow[ps] + (ka < kx ? 512u : 0u)) : front_ld<float4>(f.w, ow[ps] + (kb < kx ? 1024u : 0u));
      }
      __syncthreads();
#pragma unroll
      for (int st = 0; st < 2; ++st) {
        const __bf16* A = bufA + st * 64 * kFS;
        const __bf16* Bm = bufB + st * 128 * kFS;
        if (128 * st < din) {
#pragma unroll
          for (int s2 = 0; s2 < 8; ++s2) {
            const int k = 16 * s2 + 8 * lh;
            const tl_bf16x8 av = *reinterpret_cast<const tl_bf16x8*>(A + (rt * 32 + li) * kFS + k);
            const tl_bf16x8 bv = *reinterpret_cast<const tl_bf16x8*>(Bm + (ct * 32 + li) * kFS + k);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, bv, acc, 0, 0, 0);
          }
        }
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = rt * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        if (pn < h0) Pt[m * kFS + pn] = (__bf16)(acc[r] + bp);
      }
      __syncthreads();                                      // Pt complete; the stage buffers are free again
#pragma unroll
      for (int ps = 0; ps < 2; ++ps)                        // the projection tile -> x[:, 0:h0], 16 bytes per piece
        if (xk < h0 && b0 + xrow + 32 * ps < r1)
          *reinterpret_cast<uint4*>(f.x + (int64_t)(b0 + xrow + 32 * ps) * f.ldx + xk) =
              *reinterpret_cast<const uint4*>(Pt + (xrow + 32 * ps) * kFS + xk);
    }
    // ---- block Linear: tile (rt, nh) of the 64 x 64 block, k-half kq = MFMA k-steps 4 kq .. 4 kq + 3 of each stage ----
    {
      const int tile = wave & 3, kq = wave >> 2, rt = tile & 1, nh = tile >> 1;
      tl_f32x16 acc;
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[i] = 0.f;
      for (int s0 = 0; s0 < ns2; s0 += 3) {
#pragma unroll
        for (int u = 0; u < 3; ++u) {
          const int st = s0 + u;
          __bf16* A = bufA + (st & 1) * 64 * kFS;
          __bf16* Bm = bufB + (st & 1) * 128 * kFS;
#pragma unroll
          for (int ps = 0; ps < 2; ++ps) {
            if (GATHER) {                                   // rounded and packed as lookup_wave_kernel's 32-byte lanes do; this thread owns the piece of x
              const float4 lo = qg[u][ps][0], hi = qg[u][ps][1];
              const bool live = 128 * st + xk >= h0 && 128 * st + xk < kx;
              uint4 o;
              o.x = (uint32_t)tt_f2bf(lo.x) | ((uint32_t)tt_f2bf(lo.y) << 16);
              o.y = (uint32_t)tt_f2bf(lo.z) | ((uint32_t)tt_f2bf(lo.w) << 16);
              o.z = (uint32_t)tt_f2bf(hi.x) | ((uint32_t)tt_f2bf(hi.y) << 16);
              o.w = (uint32_t)tt_f2bf(hi.z) | ((uint32_t)tt_f2bf(hi.w) << 16);
              *reinterpret_cast<uint4*>(A + (xrow + 32 * ps) * kFS + xk) = live ? o : uint4{0u, 0u, 0u, 0u};
              if (live && b0 + xrow + 32 * ps < r1)
                *reinterpret_cast<uint4*>(f.x + (int64_t)(b0 + xrow + 32 * ps) * f.ldx + 128 * st + xk) = o;
            } else {
              *reinterpret_cast<uint4*>(A + (xrow + 32 * ps) * kFS + xk) = (128 * st + xk < kx) ? qa[u][ps] : uint4{0u, 0u, 0u, 0u};
            }
          }
#pragma unroll
          for (int ps = 0; ps < NQB; ++ps) {
            if (W16) *reinterpret_cast<float4*>(Bm + (xrow + 32 * ps) * kFS + xk) = (128 * st + xk < kx) ? qb[u][ps] : float4{0.f, 0.f, 0.f, 0.f};
            else front_put4(Bm + (frow + 16 * ps) * kFS + fk, qb[u][ps], 128 * st + fk < kx);
          }
          __syncthreads();
          {                                                 // three stages ahead, into the registers just stored
            const int ka = 128 * (st + 3) + xk, kb = 128 * (st + 3) + fk;
#pragma unroll
            for (int ps = 0; ps < 2; ++ps) {
              if (GATHER) {
                const float4* src = gather_src(st + 3, ps);
                qg[u][ps][0] = src[0]; qg[u][ps][1] = src[1];
              } else {
                qa[u][ps] = front_ld<uint4>(f.x, ox[ps] + (ka < kx ? 256u * (uint32_t)(st + 3) : 0u));
              }
            }
#pragma unroll
            for (int ps = 0; ps < NQB; ++ps)
              qb[u][ps] = W16 ? front_ld<float4>(f.w16, ow[ps] + (ka < kx ? 256u * (uint32_t)(st + 3) : 0u))
                              : front_ld<float4>(f.w, ow[ps] + (kb < kx ? 512u * (uint32_t)(st + 3) : 0u));
          }
#pragma unroll
          for (int s2 = 0; s2 < 4; ++s2) {
            const int kl = 16 * (4 * kq + s2), kglob = 128 * st + kl;
            const __bf16* asrc = kglob < h0 ? Pt + (rt * 32 + li) * kFS + kglob + 8 * lh : A + (rt * 32 + li) * kFS + kl + 8 * lh;
            const tl_bf16x8 av = *reinterpret_cast<const tl_bf16x8*>(asrc);
            const tl_bf16x8 bv = *reinterpret_cast<const tl_bf16x8*>(Bm + (nh * 32 + li) * kFS + kl + 8 * lh);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, bv, acc, 0, 0, 0);
          }
        }
      }
      __syncthreads();                                    // last stage read: bufB becomes the partial-tile area [2][64][64]
      const int n = nh * 32 + li;
#pragma unroll
      for (int r = 0; r < 16; ++r) part[(kq * 64 + rt * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh) * 64 + n] = acc[r];
    }
    __syncthreads();
    // ---- k-halves added in order + bias -> pre; relu tile (aliases part[0]: each thread overwrites what it read) ----
    if (c < H) {
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int row = rq + 8 * j;
        v[j] = (part[row * 64 + c] + part[(64 + row) * 64 + c]) + bias;
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int row = rq + 8 * j, r = b0 + row;
        if (r < r1) f.pre[(int64_t)r * H + c] = v[j];
        part[row * 64 + c] = fmaxf(v[j], 0.f);
      }
    }
    __syncthreads();
    if (t < 256 && c < H) {               // as tail_head_kernel / bn_stats_partial_kernel: rows rq, rq + 4, ... of the block
      const int nrow = min(64, r1 - b0);
      for (int row = rq; row < nrow; row += 4) {
        const float xv = part[row * 64 + c];
        if (cnt == 0.f) x0 = xv;
        const float d = xv - x0;
        s += d;
        q += d * d;
        cnt += 1.f;
      }
    }
    __syncthreads();
  }
  if (t < 256) {
    Wf w{0.f, 0.f, 0.f};
    if (c < H && cnt > 0.f) {
      w.n = cnt;
      w.mean = x0 + s / cnt;
      w.m2 = fmaxf(q - s * (s / cnt), 0.f);
    }
    sh[rq][c] = w;
  }
  __syncthreads();
  if (t < 64 && c < H) {
    Wf o = sh[0][c];
    o = wf_combine(o, sh[1][c]);
    o = wf_combine(o, sh[2][c]);
    o = wf_combine(o, sh[3][c]);
    float* p = a.partial + (int64_t)blockIdx.x * 3 * H;
    p[c] = o.n; p[H + c] = o.mean; p[2 * H + c] = o.m2;
  }
}

// (B) BN statistics finish (every workgroup, same order as bn_stats_finish_kernel) + BN apply + dropout + output Linear
// (one 64 x 64 x 64 bf16 MFMA tile) + L2 normalise, for 64 rows per workgroup.  grid (cdiv(B, 64), towers)
struct TailFwdArgs {
  BnStatArgs s;
  const float* g; const float* b; uint64_t salt; float* act;
  const float* w_out; const float* b_out; int D; float* y; float* emb;
  __bf16* pk_rows; __bf16* pk_frag; int Dp; float pk_scale;   // optional: the score kernels' two operand images of emb (tt_score_pack_bf16)
  const float* fin = nullptr;   // tail_fwd_kernel<true>: [2][H] mean, rstd, finished by the statistics rider in the keyed sort's launch
};

static_assert(kTailThreads == kRiderThreads, "the riders run in the tail kernels' workgroups");
// (cr_wg > 0: the FIRST grid row -- dispatched first: not every workgroup of the launch is resident at once -- is the keyed plan's
// compaction riding in this launch: tt_riders.h)
// Round 4: at most 64 registers, so that TWO of these 1024-thread workgroups share a CU: the launch is 256 tail workgroups plus the
// riding compaction's grid row, and at 116 registers (one workgroup per CU) the riders' row -- dispatched first -- made half the
// tail workgroups wait for a CU (18.6 us for a 10-us chain).  The 96 registers were the chunk statistics' partials, all in flight at
// once: every thread now fetches and merges ONE sub-chain of eight chunks (wf_lane_merge's order), all 1024 threads taking part.
// measurement aid, compiled in with -DTT_TAIL_STAMPS only (tools/r04_tail_stamps.py): phase stamps of the tail kernels' workgroups
#ifdef TT_TAIL_STAMPS
__device__ unsigned long long g_tail_stamps[2][512 * 8];
#define TT_TAIL_STAMP(k, i) do { if (threadIdx.x == 0) g_tail_stamps[k][((blockIdx.y * gridDim.x + blockIdx.x) & 511) * 8 + (i)] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define TT_TAIL_STAMP(k, i) do { } while (0)
#endif

// FIN: the statistics arrive finished (f.fin: one workgroup per tower has merged the chunk partials in front of the keyed sort, whose
// launch lies between tower_front and this one) -- 2 * H floats per workgroup instead of 3 * H * nchunks, no merge, no triples in LDS.
template <bool FIN>
__global__ __launch_bounds__(kTailThreads) __attribute__((amdgpu_waves_per_eu(8, 8)))
void tail_fwd_kernel(Batch<TailFwdArgs> batch, bool drop, float p, uint64_t seed0,
                     const uint64_t* __restrict__ seed_dev, CompactRider cr, int cr_wg) {
  if (cr_wg > 0 && blockIdx.y == 0) {
    if ((int)blockIdx.x < cr_wg) compact_body(cr, blockIdx.x);
    return;
  }
  const TailFwdArgs& f = batch.a[blockIdx.y - (cr_wg > 0 ? 1 : 0)];
  const BnStatArgs& a = f.s;
  const int H = a.H, D = f.D, B = a.B;
  const int m0 = blockIdx.x * 64;
  if (m0 >= B) return;
  TT_TAIL_STAMP(0, 0);
  __shared__ Wf sh[FIN ? 1 : 16][64];
  __shared__ float s_mean[64], s_rstd[64];
  __shared__ __attribute__((aligned(16))) __bf16 As[64 * kTailLd];
  __shared__ __attribute__((aligned(16))) __bf16 Bs[64 * kTailLd];
  __shared__ float Y[64 * kTailLdF];
  const int t = threadIdx.x, c = t & 63, rq = t >> 6;
  // the rows' pre-activations are in flight while the statistics settle
  float pre[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int r = m0 + rq + 16 * j;
    const float v = a.pre[(int64_t)min(r, B - 1) * H + min(c, H - 1)];     // (clamped address, no branch around the load)
    pre[j] = (c < H && r < B) ? v : 0.f;
  }
  float fm = 0.f, fr = 0.f;
  if (FIN) {                                             // every thread fetches its column's pair: no LDS, no barrier before the apply
    const float v0 = f.fin[min(c, H - 1)], v1 = f.fin[H + min(c, H - 1)];
    fm = c < H ? v0 : 0.f;
    fr = c < H ? v1 : 0.f;
  } else {                                               // thread (c, rq): sub-chain rq >> 2 of chunk lane rq & 3 (wf_lane_merge's order)
    sh[rq][c] = bn_finish_subchain(a.partial, a.pstride ? a.pstride : 3 * H, a.nchunks, H, c, rq);
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {                          // W_out [D, H] -> Bs[n][k]
    const int n = rq + 16 * j;
    const float w = f.w_out[(int64_t)min(n, D - 1) * H + min(c, H - 1)];
    Bs[n * kTailLd + c] = (__bf16)((n < D && c < H) ? w : 0.f);
  }
  if (!FIN) {
    __syncthreads();
    TT_TAIL_STAMP(0, 1);
    if (t < 64 && c < H) {
      bn_finish_column(sh, c, blockIdx.x == 0, a.mean, a.rstd, a.rm, a.rv, a.nbt, fm, fr);
      s_mean[c] = fm;
      s_rstd[c] = fr;
    }
    __syncthreads();
  } else {
    TT_TAIL_STAMP(0, 1);
  }
  TT_TAIL_STAMP(0, 2);
  {
    const uint64_t seed = drop ? seed_of(seed0, seed_dev) : 0;
    const float mean = FIN ? fm : (c < H ? s_mean[c] : 0.f), rstd = FIN ? fr : (c < H ? s_rstd[c] : 0.f);
    const float g = c < H ? f.g[c] : 0.f, bb = c < H ? f.b[c] : 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int row = rq + 16 * j, r = m0 + row;
      float v = 0.f;
      if (c < H && r < B) {
        const int64_t i = (int64_t)r * H + c;
        const float x = fmaxf(pre[j], 0.f);
        const float yv = (x - mean) * rstd * g + bb;
        v = yv * dropout_scale(drop, p, seed, f.salt + (uint64_t)i);
        f.act[i] = v;
      }
      As[row * kTailLd + c] = (__bf16)v;
    }
  }
  __syncthreads();
  TT_TAIL_STAMP(0, 3);
  const int lane = t & 63, wave = t >> 6;
  if (wave < 4) {
    const int wr = wave >> 1, wc = wave & 1, li = lane & 31, lh = lane >> 5;
    tl_f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
    for (int s2 = 0; s2 < 4; ++s2) {
      const tl_bf16x8 av = *reinterpret_cast<const tl_bf16x8*>(As + (wr * 32 + li) * kTailLd + 16 * s2 + 8 * lh);
      const tl_bf16x8 bv = *reinterpret_cast<const tl_bf16x8*>(Bs + (wc * 32 + li) * kTailLd + 16 * s2 + 8 * lh);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, bv, acc, 0, 0, 0);
    }
    const int n = wc * 32 + li;
    const float bv = n < D ? f.b_out[n] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = wr * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
      Y[m * kTailLdF + n] = acc[r] + bv;
    }
  }
  __syncthreads();
  TT_TAIL_STAMP(0, 4);
  // one wave per row as l2norm_fwd_kernel, four independent rows per wave in flight.  mul_rn: a plain v * v is
  // contracted into the first butterfly add (fma(v, v, partner's square)), which leaves the two partners -- and so the
  // lanes of one row -- with differently rounded sums
  float v[4], den[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    v[j] = lane < D ? Y[(wave * 4 + j) * kTailLdF + lane] : 0.f;
    den[j] = mul_rn(v[j], v[j]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int j = 0; j < 4; ++j) den[j] += __shfl_xor(den[j], o);
  }
  float e[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int r = m0 + wave * 4 + j;
    const float d = fmaxf(sqrtf(den[j]), kNormEps);
    e[j] = 0.f;
    if (r < B && lane < D) {
      e[j] = v[j] / d;
      f.y[(int64_t)r * D + lane] = v[j];
      f.emb[(int64_t)r * D + lane] = e[j];
    }
  }
  if (f.pk_rows && lane < f.Dp) {
    // the unit rows straight into the score kernels' operand images (layouts: pack_bf16_kernel in tt_score_bf16.hip; padding
    // rows and columns are written as zeros, this workgroup owns rows m0 .. m0 + 63 of both images):
    //   rows image  [tile][k-step][half][row in tile][8]  -- element (row, d): chunk ((t * Dp/16 + d/16) * 2 + (d%16)/8) * 32 + row%32
    //   frag image  [tile][s][h][d][8]                    -- element (row, d): 8 rows of one column; this wave's 4 rows are 4 adjacent slots
    const int Dp = f.Dp, d = lane;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int row = m0 + wave * 4 + j;
      const int64_t c = (((int64_t)(row >> 5) * (Dp >> 4) + (d >> 4)) * 2 + ((d >> 3) & 1)) * 32 + (row & 31);
      f.pk_rows[c * 8 + (d & 7)] = (__bf16)(e[j] * f.pk_scale);
    }
    const int row0 = m0 + wave * 4, rr = row0 & 31, q = rr & 15;
    const int64_t fi = (((int64_t)(row0 >> 5) * 2 + (rr >> 4)) * 2 + ((q & 7) >> 2)) * Dp + d;
    using bf16x4 = __attribute__((ext_vector_type(4))) __bf16;
    bf16x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = (__bf16)(e[j] * f.pk_scale);
    *reinterpret_cast<bf16x4*>(f.pk_frag + fi * 8 + (q >> 3) * 4) = o;
  }
#ifdef TT_TAIL_STAMPS
  __builtin_amdgcn_s_waitcnt(0);
  __syncthreads();
  TT_TAIL_STAMP(0, 5);
#endif
}

// (B') the same kernel for wider towers: last hidden width H <= 256, output D <= 128 (scripts/train.py's own [512, 256] -> 128).
// 64 rows per workgroup as above; the column-wise parts run over H / 64 column blocks, the output Linear is a [64 x H] . [H x D]
// product on 8 waves (one 32 x 32 tile each, the whole K in one MFMA chain: the order of gemm_bf16_kernel without split-K),
// a lane of the L2-normalise owns D / 64 columns.  Statistics finish, BN apply and the normalise keep the separate kernels'
// arithmetic and order.  Dynamic LDS: A tile [64][H + 8] bf16 | W_out [D][H + 8] bf16 | Y [64][D + 1] f32 | statistics.
constexpr int kWideH = 256, kWideD = 128;
constexpr int kWideLds = 64 * (kWideH + 8) * 2 + kWideD * (kWideH + 8) * 2 + 64 * (kWideD + 1) * 4 + 4 * 4 * 64 * 12 + 2 * kWideH * 4;

__global__ __launch_bounds__(kTailThreads) void tail_fwd_wide_kernel(Batch<TailFwdArgs> batch, bool drop, float p, uint64_t seed0,
                                                                    const uint64_t* __restrict__ seed_dev) {
  const TailFwdArgs& f = batch.a[blockIdx.y];
  const BnStatArgs& a = f.s;
  const int H = a.H, D = f.D, B = a.B;
  const int m0 = blockIdx.x * 64;
  if (m0 >= B) return;
  const int Hp = (H + 15) & ~15;                             // K of the output product: H padded to the MFMA's 16 (pad columns are zeros)
  const int ldA = Hp + 8;                                    // bf16 elements per LDS row of the A tile and of W_out
  extern __shared__ __attribute__((aligned(16))) char wide_smem[];
  __bf16* As = reinterpret_cast<__bf16*>(wide_smem);                                   // [64][ldA]
  __bf16* Bs = As + 64 * (kWideH + 8);                                                  // [D][ldA]
  float* Y = reinterpret_cast<float*>(Bs + kWideD * (kWideH + 8));                      // [64][D + 1]
  Wf (*sh)[4][64] = reinterpret_cast<Wf (*)[4][64]>(Y + 64 * (kWideD + 1));             // [4 column blocks][4 chunk lanes][64]
  float* s_mean = reinterpret_cast<float*>(sh + 4);
  float* s_rstd = s_mean + kWideH;
  const int t = threadIdx.x, c = t & 63, rq = t >> 6;
  const int HB = (H + 63) / 64;
  // statistics: thread = (column block t >> 8, chunk lane (t >> 6) & 3, column): the order of bn_stats_finish_kernel
  {
    const int cb = t >> 8, jl = (t >> 6) & 3, col = cb * 64 + c;
    Wf o{0.f, 0.f, 0.f};
    if (cb < HB && col < H) {
      Wf v[kMaxChunks / 4];
      const int64_t ps = a.pstride ? a.pstride : 3 * H;
#pragma unroll
      for (int i = 0; i < kMaxChunks / 4; ++i) {
        const int k = jl + 4 * i;
        const float* q = a.partial + (int64_t)k * ps;
        v[i] = k < a.nchunks ? Wf{q[col], q[H + col], q[2 * H + col]} : Wf{0.f, 0.f, 0.f};
      }
      o = wf_lane_merge(v);
    }
    sh[cb][jl][c] = o;
  }
  // W_out [D, H] -> Bs[n][k] (coalesced along k); columns H .. Hp - 1 of both operand tiles are zeros
  for (int e = t; e < D * H; e += kTailThreads) {
    const int n = e / H, k = e - n * H;
    Bs[n * ldA + k] = (__bf16)f.w_out[e];
  }
  for (int e = t; e < (D + 64) * (Hp - H); e += kTailThreads) {
    const int r = e / (Hp - H), k = H + e % (Hp - H);
    if (r < D) Bs[r * ldA + k] = (__bf16)0.f;
    else As[(r - D) * ldA + k] = (__bf16)0.f;
  }
  __syncthreads();
  if (t < 256) {
    const int col = t;                                        // one thread per column finishes its four chunk lanes
    if (col < H) {
      const int cb = col >> 6, cc = col & 63;
      const Wf o = wf_combine(wf_combine(sh[cb][0][cc], sh[cb][1][cc]), wf_combine(sh[cb][2][cc], sh[cb][3][cc]));
      const float var = o.n > 0.f ? o.m2 / o.n : 0.f;
      const float rstd = 1.f / sqrtf(var + kBnEps);
      s_mean[col] = o.mean;
      s_rstd[col] = rstd;
      if (blockIdx.x == 0) {
        a.mean[col] = o.mean;
        a.rstd[col] = rstd;
        if (a.rm) {
          a.rm[col] = (1.f - kBnMomentum) * a.rm[col] + kBnMomentum * o.mean;
          a.rv[col] = (1.f - kBnMomentum) * a.rv[col] + kBnMomentum * (o.n > 1.f ? o.m2 / (o.n - 1.f) : var);
        }
        if (a.nbt && col == 0) a.nbt[0] += 1;
      }
    }
  }
  __syncthreads();
  {
    const uint64_t seed = drop ? seed_of(seed0, seed_dev) : 0;
    for (int cb = 0; cb < HB; ++cb) {
      const int col = cb * 64 + c;
      const bool on = col < H;
      const float mean = on ? s_mean[col] : 0.f, rstd = on ? s_rstd[col] : 0.f;
      const float g = on ? f.g[col] : 0.f, bb = on ? f.b[col] : 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int row = rq + 16 * j, r = m0 + row;
        float v = 0.f;
        if (on && r < B) {
          const int64_t i = (int64_t)r * H + col;
          const float x = fmaxf(a.pre[i], 0.f);
          const float yv = (x - mean) * rstd * g + bb;
          v = yv * dropout_scale(drop, p, seed, f.salt + (uint64_t)i);
          f.act[i] = v;
        }
        if (on) As[row * ldA + col] = (__bf16)v;
      }
    }
  }
  __syncthreads();
  const int lane = t & 63, wave = t >> 6;
  const int DT = (D + 31) / 32;                               // 32-column tiles of the output (<= 4)
  if (wave < 2 * DT) {
    const int wr = wave & 1, wc = wave >> 1, li = lane & 31, lh = lane >> 5;
    tl_f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    const int nrow = min(wc * 32 + li, D - 1);                // (columns past D: a valid row of W_out, result discarded)
    for (int k0 = 0; k0 < Hp; k0 += 16) {
      const tl_bf16x8 av = *reinterpret_cast<const tl_bf16x8*>(As + (wr * 32 + li) * ldA + k0 + 8 * lh);
      const tl_bf16x8 bv = *reinterpret_cast<const tl_bf16x8*>(Bs + nrow * ldA + k0 + 8 * lh);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, bv, acc, 0, 0, 0);
    }
    const int n = wc * 32 + li;
    const float bo = n < D ? f.b_out[n] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = wr * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
      if (n < D) Y[m * (kWideD + 1) + n] = acc[r] + bo;
    }
  }
  __syncthreads();
  // one wave per row as l2norm_fwd_kernel, four rows per wave in flight; a lane owns columns lane and lane + 64
  float v[4][2], den[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float ssq = 0.f;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int col = lane + 64 * u;
      v[j][u] = col < D ? Y[(wave * 4 + j) * (kWideD + 1) + col] : 0.f;
    }
    // per-lane partial in column order (lane, lane + 64), then the butterfly: l2norm_fwd_kernel's order
    ssq = __builtin_fmaf(v[j][1], v[j][1], mul_rn(v[j][0], v[j][0]));    // l2norm_fwd_kernel's contracted `ss += v * v` over lane, lane + 64
    den[j] = ssq;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int j = 0; j < 4; ++j) den[j] += __shfl_xor(den[j], o);
  }
  float e[4][2];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int r = m0 + wave * 4 + j;
    const float d = fmaxf(sqrtf(den[j]), kNormEps);
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int col = lane + 64 * u;
      e[j][u] = 0.f;
      if (r < B && col < D) {
        e[j][u] = v[j][u] / d;
        f.y[(int64_t)r * D + col] = v[j][u];
        f.emb[(int64_t)r * D + col] = e[j][u];
      }
    }
  }
  if (f.pk_rows) {
    const int Dp = f.Dp;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int d = lane + 64 * u;
      if (d >= Dp) continue;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int row = m0 + wave * 4 + j;
        const int64_t cidx = (((int64_t)(row >> 5) * (Dp >> 4) + (d >> 4)) * 2 + ((d >> 3) & 1)) * 32 + (row & 31);
        f.pk_rows[cidx * 8 + (d & 7)] = (__bf16)(e[j][u] * f.pk_scale);
      }
      const int row0 = m0 + wave * 4, rr = row0 & 31, q = rr & 15;
      const int64_t fi = (((int64_t)(row0 >> 5) * 2 + (rr >> 4)) * 2 + ((q & 7) >> 2)) * Dp + d;
      using bf16x4 = __attribute__((ext_vector_type(4))) __bf16;
      bf16x4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = (__bf16)(e[j][u] * f.pk_scale);
      *reinterpret_cast<bf16x4*>(f.pk_frag + fi * 8 + (q >> 3) * 4) = o;
    }
  }
}

// (C) backward head (tt_tail_bwd.h: tail_bwd_head, the body this kernel shares with score_bwd_tr_kernel's TAIL form).  grid (nchunks, towers)
// (fr_on: the FIRST grid row is one workgroup running the symmetric score forward's loss reduction -- tt_riders.h)
__global__ __launch_bounds__(kTailThreads) void tail_bwd_kernel(Batch<TailBwdArgs> batch, bool drop, float p, uint64_t seed0,
                                                               const uint64_t* __restrict__ seed_dev, Finish2Rider fr, int fr_on) {
  if (fr_on && blockIdx.y == 0) {
    if (blockIdx.x == 0) finish2_body(fr);
    return;
  }
  const TailBwdArgs& f = batch.a[blockIdx.y - fr_on];
  if ((int)blockIdx.x >= f.col.nchunks) return;
  __shared__ __attribute__((aligned(16))) char smem[kTailBwdLds];
  const uint64_t seed = drop ? seed_of(seed0, seed_dev) : 0;
  tail_bwd_head<kTailThreads, false>(f, blockIdx.x, drop, p, seed, smem, nullptr, nullptr);
}

// (D) S1 / S2 finish (every workgroup, colsum_finish_kernel's order) + BN backward apply in place on the (already
// dropout-scaled) d_act, 64 rows per workgroup.  grid (cdiv(B, 64), towers)
struct TailApplyArgs {
  ColArgs col; BnBwdArgs bn;
  const float* w_slab; const float* b_slab; int D; float* g_w_out; float* g_b_out;   // [slab_chunks][D * H], [slab_chunks][D] -> [D, H], [D]
  int slab_chunks;      // row chunks of tail_bwd_kernel on THIS rank (col.nchunks counts ranks when the sums come from all ranks)
  float out_scale;      // BN weight / bias gradients are stored times this (1 / ranks under SyncBN: see twotower.h)
};

// (fr_on: the FIRST grid row is one workgroup running the symmetric score forward's loss reduction, as in tail_bwd_kernel -- its
// host when the score backward's launch runs the backward head and the pass has no first-block launch (gemm_back_kernel) to leave it to)
__global__ __launch_bounds__(kTailThreads) void tail_bwd_apply_kernel(Batch<TailApplyArgs> batch, Finish2Rider fr, int fr_on) {
  if (fr_on && blockIdx.y == 0) {
    if (blockIdx.x == 0) finish2_body(fr);
    return;
  }
  const TailApplyArgs& ta = batch.a[blockIdx.y - fr_on];
  const ColArgs& a = ta.col;
  const BnBwdArgs& b = ta.bn;
  const int H = a.H, B = a.B;
  const int t = threadIdx.x, c = t & 63, rq = t >> 6;
  const int m0 = blockIdx.x * 64;
  if (m0 >= B) return;
  __shared__ float sh[2][4][64];
  __shared__ float S[2][64];
  __shared__ float red[12][64];
  // output-layer weight / bias gradients: the per-chunk slabs of tail_bwd_kernel summed in a fixed order, 64 elements
  // per workgroup, by the 768 threads that are idle while the first 256 finish S1 / S2 -- thread (e, zl): slabs zl,
  // zl + 12, ...; then the 12 partial sums in order (wave 1)
  const int DH = ta.D * H, total = DH + ta.D, nseg = (total + 63) / 64;
  auto slab_partial = [&](int seg) {
    const int e = seg * 64 + c, zl = rq - 4;
    float v[(kMaxChunks + 11) / 12];
#pragma unroll
    for (int i = 0; i < (kMaxChunks + 11) / 12; ++i) {
      const int z = zl + 12 * i;
      v[i] = (e < total && z < ta.slab_chunks) ? (e < DH ? ta.w_slab[(int64_t)z * DH + e] : ta.b_slab[(int64_t)z * ta.D + (e - DH)]) : 0.f;
    }
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < (kMaxChunks + 11) / 12; ++i) sum += v[i];
    red[zl][c] = sum;
  };
  auto slab_final = [&](int seg) {
    const int e = seg * 64 + c;
    if (e < total) {
      float o = 0.f;
#pragma unroll
      for (int k = 0; k < 12; ++k) o += red[k][c];
      if (e < DH) ta.g_w_out[e] = o;
      else ta.g_b_out[e - DH] = o;
    }
  };
  float pr[4], da[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int r = m0 + rq + 16 * j;
    const bool ok = c < H && r < B;
    const int64_t i = (int64_t)min(r, B - 1) * H + min(c, H - 1);          // (clamped address, no branch around the loads)
    const float v0 = b.pre[i], v1 = b.d[i];
    pr[j] = ok ? v0 : 0.f;
    da[j] = ok ? v1 : 0.f;
  }
  if (t < 256) {
    float s0 = 0.f, s1 = 0.f;
    if (c < H) {
      float v0[kMaxChunks / 4], v1[kMaxChunks / 4];
      const int64_t ps = a.pstride ? a.pstride : 2 * H;
#pragma unroll
      for (int i = 0; i < kMaxChunks / 4; ++i) {
        const int k = rq + 4 * i;
        const float* q = a.partial + (int64_t)k * ps;
        v0[i] = k < a.nchunks ? q[c] : 0.f;
        v1[i] = k < a.nchunks ? q[H + c] : 0.f;
      }
#pragma unroll
      for (int i = 0; i < kMaxChunks / 4; ++i) { s0 += v0[i]; s1 += v1[i]; }
    }
    sh[0][rq][c] = s0;
    sh[1][rq][c] = s1;
  } else if ((int)blockIdx.x < nseg) {
    slab_partial(blockIdx.x);
  }
  __syncthreads();
  if (t < 64 && c < H) {
    const float t0 = (sh[0][0][c] + sh[0][1][c]) + (sh[0][2][c] + sh[0][3][c]);
    const float t1 = (sh[1][0][c] + sh[1][1][c]) + (sh[1][2][c] + sh[1][3][c]);
    S[0][c] = t0;
    S[1][c] = t1;
    if (blockIdx.x == 0) { a.out0[c] = t0 * ta.out_scale; a.out1[c] = t1 * ta.out_scale; }
  } else if (rq == 1 && (int)blockIdx.x < nseg) {
    slab_final(blockIdx.x);
  }
  __syncthreads();
  if (c < H) {
    const float mean = b.mean[c], rstd = b.rstd[c], g = b.g[c], S1 = S[0][c], S2 = S[1][c];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int r = m0 + rq + 16 * j;
      if (r < B) {
        const float xh = (fmaxf(pr[j], 0.f) - mean) * rstd;
        const float dv = g * rstd * (da[j] - S1 * b.invB - xh * (S2 * b.invB));
        b.d[(int64_t)r * H + c] = pr[j] > 0.f ? dv : 0.f;
      }
    }
  }
  // fewer row blocks than slab segments (B < 64 * nseg): the remaining segments in further rounds
  for (int seg = blockIdx.x + gridDim.x; seg < nseg; seg += gridDim.x) {
    if (t >= 256) slab_partial(seg);
    __syncthreads();
    if (rq == 1) slab_final(seg);
    __syncthreads();
  }
}

// (C') wide backward tail (last hidden width <= kWideH, output <= kWideD): L2-normalise backward, the data gradient
// d_act = d_y . W_out on MFMA (dropout scale applied) and the per-chunk BN column sums S1 / S2 taken from the accumulators, in
// one launch -- l2norm_bwd_kernel + the data-gradient GEMM + colsum_partial_kernel.  The weight gradient d_y^T . act stays the
// split-K GEMM (per-chunk slabs of [D x H] would be 17 MB per tower here).  At most 128 chunks per tower exist, so a workgroup
// has its CU to itself: 8 waves with up to 256 registers each.  Wave w owns columns 32 w .. 32 w + 31 of every 64-row block
// (two 32 x 32 accumulator tiles); its W_out operand fragments are loaded straight from global memory -- a lane's 8 k-values are
// 8 rows of the row-major [D, H] matrix, each load coalesced over the 32 columns -- converted once and kept in registers for
// the whole chunk, so W_out is read once per workgroup and never staged.  Only d_y goes through LDS.  grid (nchunks, towers)
constexpr int kWbLd = kWideD + 8;                                      // bf16 per LDS row of the d_y tile (K = D)
constexpr int kWideBwdThreads = 512;
static_assert(kWideH == 32 * (kWideBwdThreads / 64), "one 32-column strip per wave");

__global__ __launch_bounds__(kWideBwdThreads) void tail_bwd_wide_kernel(Batch<TailBwdArgs> batch, bool drop, float p, uint64_t seed0,
                                                                       const uint64_t* __restrict__ seed_dev) {
  const TailBwdArgs& f = batch.a[blockIdx.y];
  const ColArgs& a = f.col;
  const int H = a.H, D = f.D;
  if ((int)blockIdx.x >= a.nchunks) return;
  __shared__ __attribute__((aligned(16))) __bf16 dyA[64 * kWbLd];      // d_y rows of the current block (k = d)
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int Dp = (D + 15) & ~15;                                        // K zero-padded to whole MFMA steps
  const int r0 = blockIdx.x * a.rows_per_chunk, r1 = min(a.B, r0 + a.rows_per_chunk);
  const uint64_t seed = drop ? seed_of(seed0, seed_dev) : 0;
  const int li = lane & 31, lh = lane >> 5;
  const int n = wave * 32 + li;
  const bool col_ok = n < H, wave_on = wave * 32 < H;
  const int ncl = min(n, H - 1);
  tl_bf16x8 bw[kWideD / 16];                                            // B operand: element (k = d, n = h) = W_out[d][h]
  if (wave_on) {
    float wq[kWideD / 16][8];
#pragma unroll
    for (int ks = 0; ks < kWideD / 16; ++ks)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int d = 16 * ks + 8 * lh + e;
        wq[ks][e] = f.w_out[(int64_t)min(d, D - 1) * H + ncl];          // (clamped address, masked below: no branch around a load)
      }
#pragma unroll
    for (int ks = 0; ks < kWideD / 16; ++ks)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int d = 16 * ks + 8 * lh + e;
        bw[ks][e] = (__bf16)((d < D && col_ok) ? wq[ks][e] : 0.f);
      }
  }
  const float mean = a.mean[ncl], rstd = a.rstd[ncl];
  float s0 = 0.f, s1 = 0.f;
  for (int b0 = r0; b0 < r1; b0 += 64) {
    // 1. d_y of rows b0 .. b0 + 63 (l2norm_bwd_kernel's arithmetic): wave w rows 8 w + j, lane columns lane, lane + 64
    float yv[8][2], e[8][2], de[8][2], pr[2][16];
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int r = b0 + wave * 8 + j, col = lane + 64 * u;
        const bool ok = r < r1 && col < D;
        const int64_t i = (int64_t)min(r, r1 - 1) * D + min(col, D - 1);
        const float v0 = f.y[i], v1 = f.emb[i], v2 = f.d_emb[i];
        yv[j][u] = ok ? v0 : 0.f;
        e[j][u] = ok ? v1 : 0.f;
        de[j][u] = ok ? v2 : 0.f;
      }
    if (wave_on) {
#pragma unroll
      for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {                  // pre at this lane's accumulator positions
          const int row = b0 + rt * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
          pr[rt][r] = a.pre[(int64_t)min(row, r1 - 1) * H + ncl];       // (rows / columns past the end never reach a sum: da = 0)
        }
    }
    float ss[8], dot[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      ss[j] = fmaf(yv[j][1], yv[j][1], mul_rn(yv[j][0], yv[j][0]));
      dot[j] = fmaf(e[j][1], de[j][1], mul_rn(e[j][0], de[j][0]));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        ss[j] += __shfl_xor(ss[j], o);
        dot[j] += __shfl_xor(dot[j], o);
      }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int row = wave * 8 + j, r = b0 + row;
      const float nrm = sqrtf(ss[j]);
      const float den = fmaxf(nrm, kNormEps);
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int col = lane + 64 * u;
        float out = nrm > kNormEps ? (de[j][u] - e[j][u] * dot[j]) / den : de[j][u] / den;
        if (r < r1 && col < D) f.d_y[(int64_t)r * D + col] = out;
        else out = 0.f;
        if (col < Dp) dyA[row * kWbLd + col] = (__bf16)out;
      }
    }
    __syncthreads();
    // 2. d_act tiles on MFMA; dropout scale, store, column sums straight from the accumulators (rows in accumulator order)
    if (wave_on) {
#pragma unroll
      for (int rt = 0; rt < 2; ++rt) {
        tl_f32x16 acc;
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
        for (int ks = 0; ks < kWideD / 16; ++ks)
          if (16 * ks < Dp) {
            const tl_bf16x8 a1 = *reinterpret_cast<const tl_bf16x8*>(dyA + (rt * 32 + li) * kWbLd + 16 * ks + 8 * lh);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, bw[ks], acc, 0, 0, 0);
          }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = b0 + rt * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
          const bool ok = col_ok && row < r1;
          const int64_t i = (int64_t)row * H + n;
          const float da = ok ? acc[r] * dropout_scale(drop, p, seed, a.salt + (uint64_t)i) : 0.f;
          if (ok) f.d_act[i] = da;
          s0 += da;
          s1 += da * ((fmaxf(pr[rt][r], 0.f) - mean) * rstd);
        }
      }
    }
    __syncthreads();                                     // dyA is rewritten by the next block
  }
  s0 += __shfl_xor(s0, 32);
  s1 += __shfl_xor(s1, 32);
  if (lh == 0 && col_ok) {
    float* q = a.partial + (int64_t)blockIdx.x * 2 * H;
    q[n] = s0;
    q[H + n] = s1;
  }
}

// (D') wide backward apply: S1 / S2 finish (every workgroup, colsum_finish_kernel's order) + BN backward apply in place on the
// already dropout-scaled d_act, 64 rows per workgroup: thread (c, rq) = column c < 256, rows rq + 4 j.  grid (cdiv(B, 64), towers)
__global__ __launch_bounds__(kTailThreads) void tail_bwd_apply_wide_kernel(Batch<TailApplyArgs> batch) {
  const TailApplyArgs& ta = batch.a[blockIdx.y];
  const ColArgs& a = ta.col;
  const BnBwdArgs& b = ta.bn;
  const int H = a.H, B = a.B;
  const int t = threadIdx.x, c = t & 255, rq = t >> 8;
  const int m0 = blockIdx.x * 64;
  if (m0 >= B) return;
  __shared__ float sh[2][4][kWideH];
  float pr[16], da[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int64_t i = (int64_t)min(m0 + rq + 4 * j, B - 1) * H + min(c, H - 1);      // (clamped: stores are guarded below)
    pr[j] = b.pre[i];
    da[j] = b.d[i];
  }
  float s0 = 0.f, s1 = 0.f;
  {
    const int64_t ps = a.pstride ? a.pstride : 2 * H;
    const int cc = min(c, H - 1);
#pragma unroll
    for (int half = 0; half < 2; ++half) {              // chunks rq, rq + 4, ... in order, 32 loads in flight at a time
      float v0[kMaxChunks / 8], v1[kMaxChunks / 8];
#pragma unroll
      for (int i = 0; i < kMaxChunks / 8; ++i) {
        const int k = rq + 4 * (i + half * (kMaxChunks / 8));
        const float* q = a.partial + (int64_t)min(k, a.nchunks - 1) * ps;
        const float x0 = q[cc], x1 = q[H + cc];
        v0[i] = k < a.nchunks ? x0 : 0.f;
        v1[i] = k < a.nchunks ? x1 : 0.f;
      }
#pragma unroll
      for (int i = 0; i < kMaxChunks / 8; ++i) { s0 += v0[i]; s1 += v1[i]; }
    }
  }
  sh[0][rq][c] = s0;
  sh[1][rq][c] = s1;
  __syncthreads();
  if (c < H) {
    const float S1 = (sh[0][0][c] + sh[0][1][c]) + (sh[0][2][c] + sh[0][3][c]);
    const float S2 = (sh[1][0][c] + sh[1][1][c]) + (sh[1][2][c] + sh[1][3][c]);
    if (blockIdx.x == 0 && rq == 0) { a.out0[c] = S1 * ta.out_scale; a.out1[c] = S2 * ta.out_scale; }
    const float mean = b.mean[c], rstd = b.rstd[c], g = b.g[c];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int r = m0 + rq + 4 * j;
      if (r < B) {
        const float xh = (fmaxf(pr[j], 0.f) - mean) * rstd;
        const float dv = g * rstd * (da[j] - S1 * b.invB - xh * (S2 * b.invB));
        b.d[(int64_t)r * H + c] = pr[j] > 0.f ? dv : 0.f;
      }
    }
  }
}

// SyncBN phase 1: this rank's chunk statistics merged (bn_stats_finish_kernel's order) into ONE (n, mean, M2) triple per
// column, and its column sums S1 / S2 into one pair -- what the caller exchanges between the ranks.  grid (1, towers)
struct LocalArgs { const float* partial; int nchunks, H; float* out; };

__global__ __launch_bounds__(kThreads) void tail_local_stats_kernel(Batch<LocalArgs> batch) {
  const LocalArgs& a = batch.a[blockIdx.y];
  const int H = a.H;
  if ((int)blockIdx.x * 64 >= H) return;
  __shared__ Wf sh[4][64];
  const int cl = threadIdx.x & 63, c = blockIdx.x * 64 + cl, jl = threadIdx.x >> 6;
  Wf o{0.f, 0.f, 0.f};
  if (c < H) {
    Wf v[kMaxChunks / 4];
#pragma unroll
    for (int i = 0; i < kMaxChunks / 4; ++i) {
      const int k = jl + 4 * i;
      const float* q = a.partial + (int64_t)k * 3 * H;
      v[i] = k < a.nchunks ? Wf{q[c], q[H + c], q[2 * H + c]} : Wf{0.f, 0.f, 0.f};
    }
    o = wf_lane_merge(v);
  }
  sh[jl][cl] = o;
  __syncthreads();
  if (jl == 0 && c < H) {
    o = wf_combine(wf_combine(sh[0][cl], sh[1][cl]), wf_combine(sh[2][cl], sh[3][cl]));
    a.out[c] = o.n; a.out[H + c] = o.mean; a.out[2 * H + c] = o.m2;
  }
}

__global__ __launch_bounds__(kThreads) void tail_local_colsum_kernel(Batch<LocalArgs> batch) {
  const LocalArgs& a = batch.a[blockIdx.y];
  const int H = a.H;
  if ((int)blockIdx.x * 64 >= H) return;
  __shared__ float sh[2][4][64];
  const int cl = threadIdx.x & 63, c = blockIdx.x * 64 + cl, jl = threadIdx.x >> 6;
  float s0 = 0.f, s1 = 0.f;
  if (c < H) {
    float v0[kMaxChunks / 4], v1[kMaxChunks / 4];
#pragma unroll
    for (int i = 0; i < kMaxChunks / 4; ++i) {
      const int k = jl + 4 * i;
      const float* q = a.partial + (int64_t)k * 2 * H;
      v0[i] = k < a.nchunks ? q[c] : 0.f;
      v1[i] = k < a.nchunks ? q[H + c] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < kMaxChunks / 4; ++i) { s0 += v0[i]; s1 += v1[i]; }
  }
  sh[0][jl][cl] = s0;
  sh[1][jl][cl] = s1;
  __syncthreads();
  if (jl == 0 && c < H) {
    a.out[c] = (sh[0][0][cl] + sh[0][1][cl]) + (sh[0][2][cl] + sh[0][3][cl]);
    a.out[H + c] = (sh[1][0][cl] + sh[1][1][cl]) + (sh[1][2][cl] + sh[1][3][cl]);
  }
}

// ---- host side ---------------------------------------------------------------------------------
inline int ew_grid(const tt_ctx* ctx, int64_t n, int towers) {
  const int64_t cap = (int64_t)ctx->num_cus * 8 / (towers > 0 ? towers : 1);
  int64_t b = tt_cdiv(n, kThreads);
  return (int)(b < 1 ? 1 : (b < cap ? b : cap));
}

inline int chunks_for(int64_t B, int H) {
  int64_t n = 512 / tt_cdiv(H, 64);
  if (n > kMaxChunks) n = kMaxChunks;
  const int64_t mx = tt_cdiv(B, 64);
  if (n > mx) n = mx;
  return (int)(n < 1 ? 1 : n);
}

struct WsLayout {
  char* gemm;
  size_t gemm_bytes;
  char* tn[TT_MAX_HIDDEN + 2];        // own slab region per weight-gradient GEMM (0 = projection, 1 + i = block i, last = output):
  size_t tn_bytes[TT_MAX_HIDDEN + 2]; // their reductions are deferred into one launch at the end of the backward pass
  float* col;
  size_t col_bytes;
  size_t total;
};

inline int in_width(const tt_tower_params* p, int i) { return i == 0 ? p->h0 + p->kcat_e : p->hidden[i - 1]; }
inline int last_width(const tt_tower_params* p) { return p->n_hidden == 0 ? p->h0 + p->kcat_e : p->hidden[p->n_hidden - 1]; }

// the fused narrow tail (tail_*_kernel) applies to a training pass with bf16 GEMM operands whose last hidden block and
// output are at most 64 wide
inline bool tail_shape_ok(const tt_tower_params* p) {
  return p->n_hidden >= 1 && p->hidden[p->n_hidden - 1] <= 64 && p->d_out <= 64;
}
inline bool tail_fusable(int n, const tt_tower_params* const* P, int train) {
  if (!train || P[0]->compute_dtype != TT_BF16) return false;
  for (int t = 0; t < n; ++t)
    if (!tail_shape_ok(P[t]) || (P[t]->flags & TT_TOWER_UNFUSED_TAIL)) return false;
  return true;
}
// the one-launch front (tower_front_kernel): fused tail + ONE hidden block + bf16 tower input, projection width a multiple of
// 32 and at most 128, 16-byte-aligned rows everywhere
inline bool front_fusable(int n, const tt_tower_params* const* P, const tt_tower_acts* const* A) {
  for (int t = 0; t < n; ++t) {
    const tt_tower_params* p = P[t];
    const int kx = p->h0 + p->kcat_e;
    if (p->n_hidden != 1 || p->x_dtype != TT_BF16 || (p->flags & TT_TOWER_UNFUSED_FRONT)) return false;
    if (p->h0 % 32 != 0 || p->h0 > 128 || p->din % 64 != 0 || p->din > 256 || kx % 64 != 0) return false;
    if (!tt_aligned(A[t]->dense, 16) || !tt_aligned(A[t]->x, 16) || !tt_aligned(p->w_proj, 16) || !tt_aligned(p->w[0], 16)) return false;
  }
  return true;
}
// the front reads bf16 shadows of both weights (its one block is block 0)
inline bool front_w16(const tt_tower_params* p) {
  return p->w_proj_bf16 && p->w_bf16[0] && tt_aligned(p->w_proj_bf16, 16) && tt_aligned(p->w_bf16[0], 16);
}
inline bool wants_gather(const tt_tower_acts* a) { return a->gather_table || a->gather_rows || a->gather_K || a->gather_E; }
// the gathering front (tower_front_kernel<true, true>): the one-launch front of a whole training pass on bf16 shadows, every
// tower with a table of 16-byte-aligned rows of E = 8, 16, ... 256 floats (a 16-byte piece of x never straddles two rows), its
// fused rows, x[:, h0:] exactly K rows wide and an index tile that fits behind the kernel's own LDS
inline bool front_gathers(int n, const tt_tower_params* const* P, const tt_tower_acts* const* A, int64_t B, int train) {
  if (B < 1 || !tail_fusable(n, P, train) || !front_fusable(n, P, A)) return false;
  for (int t = 0; t < n; ++t) {
    const tt_tower_params* p = P[t]; const tt_tower_acts* a = A[t];
    if (p->sync_phase != 0 || (p->flags & TT_TOWER_UNFUSED_GATHER) || !front_w16(p)) return false;
    if (!a->gather_table || !a->gather_rows || !tt_aligned(a->gather_table, 16) || !tt_aligned(a->gather_rows, 4)) return false;
    const int K = a->gather_K, E = a->gather_E;
    if (K < 1 || E < 8 || E > 256 || (E & (E - 1)) != 0 || (int64_t)K * E != p->kcat_e) return false;
    if (kFrontLds + 64 * (int64_t)K * (int64_t)sizeof(int32_t) > kFrontLdsMax) return false;
  }
  return true;
}
// the wide forward tail (tail_fwd_wide_kernel): training, bf16 operands, last hidden width <= 256, output <= 128 -- shapes the
// narrow fused tail does not take
inline bool wide_tail_ok(int n, const tt_tower_params* const* P, int train) {
  if (!train || P[0]->compute_dtype != TT_BF16) return false;
  for (int t = 0; t < n; ++t) {
    const tt_tower_params* p = P[t];
    if (p->n_hidden < 1 || p->hidden[p->n_hidden - 1] > kWideH || p->d_out > kWideD || (p->flags & TT_TOWER_UNFUSED_TAIL)) return false;
  }
  return true;
}
inline size_t tail_slab_bytes(const tt_tower_params* p) {   // per-chunk output-layer gradient slabs of tail_bwd_kernel
  return sizeof(float) * (size_t)kMaxChunks * ((size_t)p->d_out * p->hidden[p->n_hidden - 1] + (size_t)p->d_out) + 256;
}

inline WsLayout ws_layout(const tt_tower_params* p, int64_t B, char* base) {
  size_t g = tt_gemm_tn_workspace_bytes(p->h0, p->din, B);
  int hmax = p->d_out > p->h0 ? p->d_out : p->h0;
  for (int i = 0; i < p->n_hidden; ++i) {
    const size_t b = tt_gemm_tn_workspace_bytes(p->hidden[i], in_width(p, i), B);
    g = b > g ? b : g;
    hmax = p->hidden[i] > hmax ? p->hidden[i] : hmax;
  }
  const size_t b = tt_gemm_tn_workspace_bytes(p->d_out, last_width(p), B);
  g = b > g ? b : g;
  {                                                    // split-K slabs of the forward GEMMs (largest output)
    int nmax = p->h0 > p->d_out ? p->h0 : p->d_out;
    for (int i = 0; i < p->n_hidden; ++i) nmax = p->hidden[i] > nmax ? p->hidden[i] : nmax;
    const size_t f = tt_gemm_nt_workspace_bytes(B, nmax, 0);
    g = f > g ? f : g;
  }
  WsLayout w;
  w.gemm_bytes = (g + 255) & ~size_t(255);
  w.col_bytes = sizeof(float) * 3 * (size_t)hmax * (size_t)kMaxChunks + 256;
  w.gemm = base;
  w.col = reinterpret_cast<float*>(base ? base + w.gemm_bytes : nullptr);
  size_t o = w.gemm_bytes + ((w.col_bytes + 255) & ~size_t(255));
  for (int l = 0; l < p->n_hidden + 2; ++l) {
    size_t nb = l == 0 ? tt_gemm_tn_workspace_bytes(p->h0, p->din, B)
              : l == p->n_hidden + 1 ? tt_gemm_tn_workspace_bytes(p->d_out, last_width(p), B)
                                     : tt_gemm_tn_workspace_bytes(p->hidden[l - 1], in_width(p, l - 1), B);
    if (l == p->n_hidden + 1 && tail_shape_ok(p) && tail_slab_bytes(p) > nb) nb = tail_slab_bytes(p);
    if (l == 0 && p->n_hidden >= 1) {                   // the one-launch first-block backward keeps its G slabs here
      const size_t gb = tt_gemm_back_g_workspace_bytes(p->hidden[0], p->h0, p->din, B);
      nb = gb > nb ? gb : nb;
    }
    w.tn[l] = base ? base + o : nullptr;
    w.tn_bytes[l] = (nb + 255) & ~size_t(255);
    o += w.tn_bytes[l];
  }
  w.total = o;
  return w;
}

int check_params(const tt_tower_params* p, const char* who) {
  TT_CHECK_ARG(p, "%s: params NULL", who);
  TT_CHECK_ARG(p->n_hidden >= 0 && p->n_hidden <= TT_MAX_HIDDEN, "%s: n_hidden=%d not in [0,%d]", who, p->n_hidden, TT_MAX_HIDDEN);
  TT_CHECK_ARG(p->din >= 1 && p->h0 >= 1 && p->kcat_e >= 0 && p->d_out >= 1, "%s: bad dims", who);
  TT_CHECK_ARG(p->w_proj && p->b_proj && p->w_out && p->b_out, "%s: NULL projection/output weights", who);
  for (int i = 0; i < p->n_hidden; ++i) {
    TT_CHECK_ARG(p->hidden[i] >= 1, "%s: hidden[%d] < 1", who, i);
    TT_CHECK_ARG(p->w[i] && p->b[i] && p->bn_w[i] && p->bn_b[i] && p->bn_rm[i] && p->bn_rv[i], "%s: NULL block %d params", who, i);
  }
  return TT_OK;
}

int check_batch(int32_t n, const tt_tower_params* const* P, int64_t B, float dropout_p, void* const* ws, const size_t* wsb,
                const char* who) {
  TT_CHECK_ARG(n >= 1 && n <= TT_MAX_SIDES && P && ws && wsb, "%s: need 1..%d towers", who, TT_MAX_SIDES);
  TT_CHECK_ARG(B >= 0 && B < ((int64_t)1 << 24), "%s: B=%lld out of range", who, (long long)B);
  TT_CHECK_ARG(dropout_p >= 0.f && dropout_p < 1.f, "%s: dropout_p=%f not in [0,1)", who, dropout_p);
  for (int t = 0; t < n; ++t) {
    if (int rc = check_params(P[t], who)) return rc;
    TT_CHECK_ARG(P[t]->n_hidden == P[0]->n_hidden, "%s: towers fused into one launch must have the same number of hidden blocks", who);
    TT_CHECK_ARG(P[t]->compute_dtype == P[0]->compute_dtype, "%s: towers fused into one launch must share compute_dtype", who);
    TT_CHECK_ARG((P[t]->x_dtype == TT_F32 && P[t]->dx_dtype == TT_F32) || P[t]->compute_dtype == TT_BF16,
                 "%s: bf16 x / d_x need compute_dtype TT_BF16", who);
    TT_CHECK_ARG((P[t]->x_dtype == TT_F32 || P[t]->x_dtype == TT_BF16) && (P[t]->dx_dtype == TT_F32 || P[t]->dx_dtype == TT_BF16),
                 "%s: bad x_dtype / dx_dtype", who);
    TT_CHECK_ARG(P[t]->sync_phase == P[0]->sync_phase && P[t]->sync_phase >= 0 && P[t]->sync_phase <= 2, "%s: bad / mixed sync_phase", who);
    TT_CHECK_ARG(P[t]->sync_phase == 0 || (P[t]->sync_ranks >= 1 && P[t]->sync_ranks <= kMaxChunks), "%s: sync_ranks=%d not in [1, %d]", who,
                 P[t]->sync_ranks, kMaxChunks);
    if (B > 0 && (!ws[t] || wsb[t] < tt_tower_workspace_bytes(P[t], B))) {
      tt_set_error("%s: workspace of tower %d: %zu < required %zu", who, t, wsb[t], tt_tower_workspace_bytes(P[t], B));
      return TT_ERR_WORKSPACE;
    }
  }
  return TT_OK;
}

// ---- the two passes: state, per-block argument builders, GEMM items, the SyncBN cut, the fused paths ----------------------------
// What one call of tt_towers_mlp_fwd / _bwd works on, built once per call (G, d_emb: backward only)
struct Pass {
  tt_ctx* ctx; hipStream_t st; int n;
  const tt_tower_params* const* P; const tt_tower_acts* const* A; const tt_tower_grads* const* G; const float* const* d_emb;
  int64_t B; WsLayout ws[TT_MAX_SIDES];
  bool train, drop; float dropout_p; uint64_t seed; const uint64_t* seed_dev;
  int phase, nh; bool bf16;
};
inline Pass make_pass(tt_ctx* ctx, tt_stream stream, int n, const tt_tower_params* const* P, const tt_tower_acts* const* A,
                      const tt_tower_grads* const* G, const float* const* d_emb, int64_t B, int32_t train, float dropout_p, uint64_t seed,
                      const uint64_t* seed_dev, void* const* workspaces) {
  Pass p{ctx, reinterpret_cast<hipStream_t>(stream), n, P, A, G, d_emb, B, {}, train != 0, train && dropout_p > 0.f, dropout_p, seed, seed_dev,
         P[0]->sync_phase, P[0]->n_hidden, P[0]->compute_dtype == TT_BF16};
  for (int t = 0; t < n; ++t) p.ws[t] = ws_layout(P[t], B, reinterpret_cast<char*>(workspaces[t]));
  return p;
}
int check_sync_phase(const Pass& p, const char* who) {
  if (p.phase == 0) return TT_OK;
  if (p.nh != 1 || !p.train) {
    tt_set_error("%s: sync_phase %d needs a training pass over towers with exactly one hidden block (the pass is cut at its BatchNorm)", who, p.phase);
    return TT_ERR_UNSUPPORTED;
  }
  for (int t = 0; t < p.n; ++t) {
    const float* buf = p.G ? (!p.G[t] ? nullptr : p.phase == 1 ? p.G[t]->s_sync_local : p.G[t]->s_sync_all)
                           : (p.phase == 1 ? p.A[t]->bn_sync_local : p.A[t]->bn_sync_all);
    TT_CHECK_ARG(buf != nullptr, "%s: NULL SyncBN buffer", who);
  }
  return TT_OK;
}
// The dropout salt of hidden block i of tower slot t.  Dropout element index = GLOBAL row * H + column: the rank's first row enters
// through the salt.  Restated by oracle/oracle_np.py (dropout_salt) and tests/test_oracle_golden.py (the mask tests).
inline uint64_t block_salt(const tt_tower_params* p, int t, int i) {
  return (((uint64_t)(i + 1) << 40) ^ ((uint64_t)t << 52)) + (uint64_t)p->rng_row_offset * (uint64_t)p->hidden[i];
}
// Layers are numbered 0 .. nh: hidden block i, then the output Linear as layer nh.  Layer i reads layer_in (in_width wide) and its
// backward writes the gradient of that input to d_in; block i's own gradient (d_act, then d_pre in place) is d_in of layer i + 1.
inline const float* layer_in(const Pass& p, int i, int t) { return i == 0 ? reinterpret_cast<const float*>(p.A[t]->x) : p.A[t]->act[i - 1]; }
inline float* d_in(const Pass& p, int i, int t) { return i == 0 ? reinterpret_cast<float*>(p.G[t]->d_x) : p.G[t]->scratch[i - 1]; }
inline int block_chunks(const Pass& p, int i, int t) { return chunks_for(p.B, p.P[t]->hidden[i]); }
struct BlockDims { int hmax = 1, cmax = 1; int64_t tmax = 1; };   // of block i over the towers: widest, most chunks, most elements
inline BlockDims block_dims(const Pass& p, int i) {
  BlockDims d;
  for (int t = 0; t < p.n; ++t) {
    const int H = p.P[t]->hidden[i], nchunks = block_chunks(p, i, t);
    d.hmax = H > d.hmax ? H : d.hmax;
    d.cmax = nchunks > d.cmax ? nchunks : d.cmax;
    d.tmax = p.B * H > d.tmax ? p.B * H : d.tmax;
  }
  return d;
}
inline BnStatArgs bn_stat_args(const Pass& p, int i, int t) {
  const tt_tower_params* P = p.P[t]; const tt_tower_acts* A = p.A[t];
  const int nchunks = block_chunks(p, i, t);
  return BnStatArgs{A->pre[i], (int)p.B, P->hidden[i], (int)tt_cdiv(p.B, nchunks), nchunks, p.ws[t].col, A->mean[i], A->rstd[i],
                    P->bn_rm[i], P->bn_rv[i], P->bn_nbt[i]};
}
inline BnApplyArgs bn_apply_args(const Pass& p, int i, int t) {
  const tt_tower_params* P = p.P[t]; const tt_tower_acts* A = p.A[t];
  return BnApplyArgs{A->pre[i], p.B * P->hidden[i], P->hidden[i], A->mean[i], A->rstd[i], P->bn_w[i], P->bn_b[i], block_salt(P, t, i), A->act[i]};
}
// S1 = sum da -> bn bias grad ; S2 = sum da*xhat -> bn weight grad  (x: where da is read; the tail kernels take it from their tile)
inline ColArgs col_args(const Pass& p, int i, int t, const float* x, int64_t ldx) {
  const tt_tower_acts* A = p.A[t];
  const int nchunks = block_chunks(p, i, t);
  return ColArgs{x, ldx, A->pre[i], A->mean[i], A->rstd[i], block_salt(p.P[t], t, i), (int)p.B, p.P[t]->hidden[i], (int)tt_cdiv(p.B, nchunks),
                 nchunks, p.ws[t].col, p.G[t]->bn_b[i], p.G[t]->bn_w[i]};
}
inline BnBwdArgs bn_bwd_args(const Pass& p, int i, int t) {
  const tt_tower_params* P = p.P[t]; const tt_tower_acts* A = p.A[t];
  return BnBwdArgs{d_in(p, i + 1, t), A->pre[i], p.B * P->hidden[i], P->hidden[i], 1.f / (float)p.B, A->mean[i], A->rstd[i], P->bn_w[i],
                   p.G[t]->bn_b[i], p.G[t]->bn_w[i], block_salt(P, t, i)};
}
int check_block_grads(const Pass& p, int i) {
  for (int t = 0; t < p.n; ++t)
    TT_CHECK_ARG(p.G[t]->w[i] && p.G[t]->b[i] && p.G[t]->bn_w[i] && p.G[t]->bn_b[i], "tt_towers_mlp_bwd: NULL gradient buffers of block %d", i);
  return TT_OK;
}
// GEMM items, complete as they come out.  Forward, C[B, N] = A[B, K] . W[N, K]^T + bias:
inline GemmNT nt_item(const Pass& p, int t, const float* A, const float* W, const float* bias, float* C, int64_t ldc, int N, int K) {
  GemmNT g{A, K, W, K, bias, C, ldc, p.B, N, K, false, 1.f};
  g.bf16 = p.bf16; g.workspace = p.ws[t].gemm; g.workspace_bytes = p.ws[t].gemm_bytes;
  return g;
}
// Backward of layer i from its output gradient dY [B, M] (d_y, or block i's d_pre):  dW [M, N] = dY^T . in (+ the bias gradient, its
// column sums) into workspace slot 1 + i, and d_in [B, N] = dY . W
inline GemmTN tn_item(const Pass& p, int t, int slot, const float* A, int64_t lda, const float* Bm, float* C, int M, int N, float* colsum) {
  GemmTN g{A, lda, Bm, N, C, N, M, N, p.B, p.ws[t].tn[slot], p.ws[t].tn_bytes[slot], colsum};
  g.bf16 = p.bf16;
  return g;
}
int launch_layer_nt(const Pass& p, int i, NtDeferred* defer) {
  GemmNT nt[TT_MAX_SIDES];
  const bool out = i == p.nh;
  for (int t = 0; t < p.n; ++t) {
    const tt_tower_params* P = p.P[t];
    const int N = out ? P->d_out : P->hidden[i];
    nt[t] = nt_item(p, t, layer_in(p, i, t), out ? P->w_out : P->w[i], out ? P->b_out : P->b[i], out ? p.A[t]->y : p.A[t]->pre[i], N, N, in_width(P, i));
    nt[t].a_bf16 = i == 0 && P->x_dtype == TT_BF16;
    nt[t].defer = defer ? &defer[t] : nullptr;
  }
  return tt_gemm_nt_batched(p.st, nt, p.n);
}
int launch_layer_bwd(const Pass& p, int i, TnPending* pend, bool data_grad = true) {
  GemmTN tn[TT_MAX_SIDES]; GemmNN nn[TT_MAX_SIDES];
  const bool out = i == p.nh;
  for (int t = 0; t < p.n; ++t) {
    const tt_tower_params* P = p.P[t]; const tt_tower_grads* g = p.G[t];
    const int M = out ? P->d_out : P->hidden[i], N = in_width(P, i);
    const float* dY = out ? g->d_y : d_in(p, i + 1, t);
    tn[t] = tn_item(p, t, 1 + i, dY, M, layer_in(p, i, t), out ? g->w_out : g->w[i], M, N, out ? g->b_out : g->b[i]);
    tn[t].b_bf16 = i == 0 && P->x_dtype == TT_BF16;
    nn[t] = GemmNN{dY, M, out ? P->w_out : P->w[i], N, d_in(p, i, t), N, p.B, N, M};
    nn[t].bf16 = p.bf16; nn[t].c_bf16 = i == 0 && P->dx_dtype == TT_BF16;
  }
  if (int rc = tt_gemm_tn_batched(p.st, tn, p.n, pend)) return rc;
  return data_grad ? tt_gemm_nn_batched(p.st, nn, p.n) : TT_OK;
}

// ---- SyncBN: the pass is cut at its one BatchNorm (twotower.h: sync_phase).  Phase 1 hands this rank's chunk-merged statistics
// (forward) / column sums (backward) to the caller and stops; phase 2 continues with every rank's share as one "chunk" each
int sync_hand_out_stats(const Pass& p, const Batch<BnStatArgs>& bs, int hmax) {
  Batch<LocalArgs> la{};
  for (int t = 0; t < p.n; ++t) la.a[t] = LocalArgs{bs.a[t].partial, bs.a[t].nchunks, bs.a[t].H, p.A[t]->bn_sync_local};
  tail_local_stats_kernel<<<dim3((unsigned)tt_cdiv(hmax, 64), (unsigned)p.n), kThreads, 0, p.st>>>(la);
  TT_LAUNCH_CHECK();
  return TT_OK;
}
inline void sync_take_rank_stats(const Pass& p, Batch<BnStatArgs>& bs) {
  for (int t = 0; t < p.n; ++t) {
    bs.a[t].partial = const_cast<float*>(p.A[t]->bn_sync_all); bs.a[t].nchunks = p.P[t]->sync_ranks; bs.a[t].pstride = p.A[t]->bn_sync_stride;
  }
}
int sync_hand_out_colsums(const Pass& p, const Batch<ColArgs>& cols, int gx) {
  Batch<LocalArgs> la{};
  for (int t = 0; t < p.n; ++t) la.a[t] = LocalArgs{cols.a[t].partial, cols.a[t].nchunks, cols.a[t].H, p.G[t]->s_sync_local};
  tail_local_colsum_kernel<<<dim3((unsigned)gx, (unsigned)p.n), kThreads, 0, p.st>>>(la);
  TT_LAUNCH_CHECK();
  return TT_OK;
}
// S1 / S2 of every rank, one "chunk" each, over ranks * B rows; returns 1 / ranks, the scale of the stored BN weight / bias gradients.
// The tail apply kernels (raw == nullptr) finish the sums in every workgroup, use them from there and scale what they store by
// TailApplyArgs::out_scale, so their caller takes the return value and `col` is a copy beside the one the head used.  The separate
// kernels pass S1 / S2 through memory: colsum_finish_kernel stores the gradients scaled (col.out_scale) and the unscaled sums
// bn_bwd_apply_kernel needs go to `raw`.  That is the one difference between the three places this was written out, and it is on purpose.
inline float sync_take_rank_colsums(const Pass& p, ColArgs& col, BnBwdArgs& bn, int t, float* raw) {
  const int ranks = p.P[t]->sync_ranks;
  col.partial = const_cast<float*>(p.G[t]->s_sync_all); col.nchunks = ranks; col.pstride = p.G[t]->s_sync_stride;
  bn.invB = 1.f / ((float)p.B * (float)ranks);
  if (raw) { col.out_scale = 1.f / (float)ranks; col.sums_raw = raw; bn.S1 = raw; bn.S2 = raw + col.H; }
  return 1.f / (float)ranks;
}

// ---- forward paths --------------------------------------------------------------------------------------------------------------
// the score kernels' two operand images of emb, written by the tail itself (tt_score_pack_bf16's layout)
inline void pack_target(const Pass& p, TailFwdArgs& tf, int t) {
  if (!p.A[t]->emb_packed) return;
  tf.Dp = p.P[t]->d_out <= 32 ? 32 : (p.P[t]->d_out <= 64 ? 64 : 128);
  tf.pk_rows = reinterpret_cast<__bf16*>(p.A[t]->emb_packed);
  tf.pk_frag = tf.pk_rows + tt_cdiv(p.B, 64) * 64 * tf.Dp;
  tf.pk_scale = p.A[t]->emb_pack_scale == 0.f ? 1.f : p.A[t]->emb_pack_scale;
}
inline Batch<TailFwdArgs> tail_fwd_args(const Pass& p, int i, const Batch<BnStatArgs>& bs) {
  Batch<TailFwdArgs> tf{};
  for (int t = 0; t < p.n; ++t) {
    const tt_tower_params* P = p.P[t];
    tf.a[t] = TailFwdArgs{bs.a[t], P->bn_w[i], P->bn_b[i], block_salt(P, t, i), p.A[t]->act[i], P->w_out, P->b_out, P->d_out,
                          p.A[t]->y, p.A[t]->emb, nullptr, nullptr, 0, 1.f};
    pack_target(p, tf.a[t], t);
  }
  return tf;
}
// The fused narrow tail (tail_fusable) from block i's pre-activations -- or, behind a split-K block GEMM, its slabs `nd` -- to the
// unit rows: the chunk statistics in the same pass as slabs (+ bias) -> pre, then everything else in one kernel.  Ends the pass.
int fwd_narrow_tail(const Pass& p, int i, Batch<BnStatArgs>& bs, const NtDeferred* nd, bool front, bool gather, const BlockDims& dim) {
  tt_ctx* ctx = p.ctx; hipStream_t st = p.st; const int n = p.n;
  if (p.phase != 2) {
    if (front) {                                      // projection + block Linear + chunk statistics in one launch
      Batch<FrontArgs> fb{};
      bool w16 = true;                                // every tower brings bf16 shadows of both weights (16-byte aligned)
      int kmax = 0;
      for (int t = 0; t < n; ++t) {
        const tt_tower_params* P = p.P[t]; const tt_tower_acts* A = p.A[t];
        const int wx = P->h0 + P->kcat_e;
        fb.a[t] = FrontArgs{A->dense, P->din, P->din, P->w_proj, P->b_proj, P->h0, reinterpret_cast<uint16_t*>(A->x), wx, wx, P->w[i], P->b[i],
                            A->pre[i], bs.a[t], reinterpret_cast<const uint16_t*>(P->w_proj_bf16), reinterpret_cast<const uint16_t*>(P->w_bf16[i]),
                            A->gather_table, A->gather_rows, A->gather_K, A->gather_E};
        w16 = w16 && front_w16(P);
        kmax = A->gather_K > kmax ? A->gather_K : kmax;
      }
      if (gather) {                                   // (front_gathers: every tower brings shadows, rows and a table)
        const int lds = kFrontLds + 64 * kmax * (int)sizeof(int32_t);     // + the index tile of the tower with the most keys
        TT_LDS_ONCE(kFrontLdsMax, tower_front_kernel<true, true>);
        tower_front_kernel<true, true><<<dim3((unsigned)dim.cmax, (unsigned)n), kFrontThreads, lds, st>>>(fb);
      } else if (w16) {
        TT_LDS_ONCE(kFrontLds, tower_front_kernel<true>);
        tower_front_kernel<true><<<dim3((unsigned)dim.cmax, (unsigned)n), kFrontThreads, kFrontLds, st>>>(fb);
      } else {
        TT_LDS_ONCE(kFrontLds, tower_front_kernel<false>);
        tower_front_kernel<false><<<dim3((unsigned)dim.cmax, (unsigned)n), kFrontThreads, kFrontLds, st>>>(fb);
      }
    } else if (nd[0].splits > 0) {
      Batch<HeadArgs> hb{};
      for (int t = 0; t < n; ++t) hb.a[t] = HeadArgs{nd[t].slabs, nd[t].slab_stride, nd[t].splits, p.P[t]->b[i], p.A[t]->pre[i], bs.a[t]};
      tail_head_kernel<<<dim3((unsigned)dim.cmax, (unsigned)n), kTailThreads, 0, st>>>(hb);
    } else {
      bn_stats_partial_kernel<<<dim3(1, (unsigned)dim.cmax, (unsigned)n), kThreads, 0, st>>>(bs);
    }
    TT_LAUNCH_CHECK();
  }
  if (p.phase == 1) return sync_hand_out_stats(p, bs, dim.hmax);
  if (p.phase == 2) sync_take_rank_stats(p, bs);
  Batch<TailFwdArgs> tf = tail_fwd_args(p, i, bs);
  bool fin = false;
  int mine = 0;                                     // of the keyed plan (TT_OPT_DEFER_RIDERS): what this call hosts
  if (int rc = tt_deferred_host(ctx, TT_DQ_SORT | TT_DQ_COMPACT, st, &mine)) return rc;
  if (mine & TT_DQ_SORT) {
    // the keyed plan's sort has been held back for this place: behind the front kernel, with one workgroup per tower in its
    // grid that finishes the chunk statistics once -- the tail then reads 2 * H floats per workgroup
    BnFinishRiders bf{};
    fin = p.phase == 0 && ctx->bn_fin != nullptr;     // (SyncBN's second half merges rank triples: in the tail, as before)
    for (int t = 0; t < n && fin; ++t) {
      const BnStatArgs& s = bs.a[t];
      bf.r[t] = BnFinishRider{s.partial, s.pstride ? s.pstride : 3 * s.H, s.nchunks, s.H, s.mean, s.rstd, s.rm, s.rv, s.nbt,
                              ctx->bn_fin + t * kBnFinStride};
      tf.a[t].fin = bf.r[t].out;
    }
    if (int rc = tt_keyed_sort_run(ctx->dq->sort, st, &bf, fin ? n : 0)) return rc;
  }
  const int cr_wg = (mine & TT_DQ_COMPACT) ? ctx->dq->compact_wg : 0;      // a queued plan compaction rides in one extra grid row
  const int64_t gx = tt_cdiv(p.B, 64) > cr_wg ? tt_cdiv(p.B, 64) : cr_wg;
  const dim3 grid((unsigned)gx, (unsigned)(n + (cr_wg > 0 ? 1 : 0)));
  if (fin) tail_fwd_kernel<true><<<grid, kTailThreads, 0, st>>>(tf, p.drop, p.dropout_p, p.seed, p.seed_dev, ctx->dq->compact, cr_wg);
  else tail_fwd_kernel<false><<<grid, kTailThreads, 0, st>>>(tf, p.drop, p.dropout_p, p.seed, p.seed_dev, ctx->dq->compact, cr_wg);
  tt_deferred_taken(ctx, mine);
  TT_LAUNCH_CHECK();
  return TT_OK;
}
// The wide tail (wide_tail_ok) behind the chunk statistics of block i: statistics finish + BN apply + dropout + output Linear +
// L2 normalise + the score kernels' operand images in one launch.  Ends the pass.
int fwd_wide_tail(const Pass& p, int i, const Batch<BnStatArgs>& bs) {
  tt_ctx* ctx = p.ctx;
  TT_LDS_ONCE(kWideLds, tail_fwd_wide_kernel);
  tail_fwd_wide_kernel<<<dim3((unsigned)tt_cdiv(p.B, 64), (unsigned)p.n), kTailThreads, kWideLds, p.st>>>(tail_fwd_args(p, i, bs), p.drop, p.dropout_p, p.seed, p.seed_dev);
  TT_LAUNCH_CHECK();
  return TT_OK;
}

// ---- backward paths -------------------------------------------------------------------------------------------------------------
// First block + projection as ONE launch (tt_gemm.h: GemmBack; d_pre of block 0 arrives in scratch[0]): its items, and whether the
// pass takes it.  Asked once per call, before the tail: the tail leaves a queued loss reduction to that launch.
bool back_items(const Pass& p, GemmBack* gb) {
  if (p.nh < 1 || !p.bf16) return false;
  for (int t = 0; t < p.n; ++t) {
    const tt_tower_params* P = p.P[t]; const tt_tower_grads* g = p.G[t];
    const int wx = P->h0 + P->kcat_e;
    if (P->flags & TT_TOWER_UNFUSED_BACK) return false;
    gb[t] = GemmBack{g->scratch[0], P->hidden[0], p.A[t]->x, wx, wx, P->x_dtype == TT_BF16, p.A[t]->dense, P->din, P->din,
                     P->w[0], P->h0, reinterpret_cast<float*>(g->d_x), wx, P->dx_dtype == TT_BF16, g->w[0], g->b[0],
                     g->w_proj, g->b_proj, p.ws[t].tn[1], p.ws[t].tn_bytes[1], p.ws[t].tn[0], p.ws[t].tn_bytes[0], p.B};
    gb[t].w16 = P->w_bf16[0];
  }
  return tt_gemm_back_supported(gb, p.n);
}
// which launch of the pass runs a queued loss reduction (the symmetric score forward's, TT_DQ_LOSS) in an extra grid row
enum LossHost { kLossNobody, kLossTailBwd, kLossGemmBack, kLossTailBwdApply };
// The fused narrow tail's backward: L2-normalise backward, both output-layer GEMMs and the BN column sums of the last block in one
// kernel; the BN backward apply (after the batch-wide S1 / S2) in a second.  *loss: who hosts a queued loss reduction.
int bwd_narrow_tail(const Pass& p, bool back, LossHost* loss) {
  tt_ctx* ctx = p.ctx; hipStream_t st = p.st; const int n = p.n, i = p.nh - 1;
  if (int rc = check_block_grads(p, i)) return rc;
  Batch<ColArgs> cb{}; Batch<TailBwdArgs> tb{}; Batch<TailApplyArgs> tp{};
  for (int t = 0; t < n; ++t) {
    const tt_tower_params* P = p.P[t]; const tt_tower_grads* g = p.G[t];
    const int H = P->hidden[i], D = P->d_out;
    cb.a[t] = col_args(p, i, t, nullptr, 0);
    const int nchunks = cb.a[t].nchunks;
    float* w_slab = reinterpret_cast<float*>((reinterpret_cast<uintptr_t>(p.ws[t].tn[p.nh + 1]) + 255) & ~uintptr_t(255));
    float* b_slab = w_slab + (size_t)nchunks * D * H;
    tb.a[t] = TailBwdArgs{p.A[t]->y, p.A[t]->emb, p.d_emb[t], g->d_y, D, P->w_out, p.A[t]->act[i], d_in(p, p.nh, t), cb.a[t], w_slab, b_slab};
    tp.a[t] = TailApplyArgs{cb.a[t], bn_bwd_args(p, i, t), w_slab, b_slab, D, g->w_out, g->b_out, nchunks, 1.f};
    if (p.phase == 2) tp.a[t].out_scale = sync_take_rank_colsums(p, tp.a[t].col, tp.a[t].bn, t, nullptr);
  }
  // a score backward that waits in the context (TT_OPT_FUSE_SCORE_TAIL) runs the head in its own launch when its workgroups
  // are the head's: two towers, H = D = 64, 64-row chunks numbered like its 64-row tiles, its dA exactly d_emb in tower order
  int mine = 0;                                       // of the score backward and the loss reduction: what is queued on this stream
  if (int rc = tt_deferred_host(ctx, TT_DQ_SCORE_BWD | TT_DQ_LOSS, st, &mine)) return rc;
  bool hosted = false;
  if (mine & TT_DQ_SCORE_BWD) {
    hosted = p.phase == 0 && n == 2 && ctx->dq->score_rows == p.B && ctx->dq->score_dA[0] == p.d_emb[0] && ctx->dq->score_dA[1] == p.d_emb[1];
    for (int t = 0; hosted && t < n; ++t)
      hosted = tb.a[t].D == 64 && tb.a[t].col.H == 64 && tb.a[t].col.rows_per_chunk == 64 && tb.a[t].col.nchunks == (int)tt_cdiv(p.B, 64);
    if (hosted) {
      if (int rc = tt_score_tail_bwd_launch(ctx, tb, p.drop, p.dropout_p, p.seed, p.seed_dev)) return rc;
    } else if (int rc = tt_deferred_flush(ctx, TT_DQ_SCORE_BWD)) {
      return rc;
    }
  }
  // a queued loss reduction rides in tail_bwd's extra grid row; where the score backward ran the head (512-thread workgroups) it
  // waits for the first block's launch -- only the host reads it, and tail_bwd_apply's workgroups are on the step's chain
  // -- or, in a pass without that launch, rides in tail_bwd_apply's extra grid row.  (SyncBN's second half launches no tail_bwd and
  // hosts no score backward: the reduction stays queued.)
  *loss = !(mine & TT_DQ_LOSS) ? kLossNobody : hosted ? (back ? kLossGemmBack : kLossTailBwdApply) : p.phase != 2 ? kLossTailBwd : kLossNobody;
  if (p.phase != 2 && !hosted) {
    const int fr_on = *loss == kLossTailBwd;
    tail_bwd_kernel<<<dim3((unsigned)block_dims(p, i).cmax, (unsigned)(n + fr_on)), kTailThreads, 0, st>>>(tb, p.drop, p.dropout_p, p.seed, p.seed_dev, ctx->dq->loss, fr_on);
    tt_deferred_taken(ctx, TT_DQ_LOSS & mine);
    TT_LAUNCH_CHECK();
  }
  if (p.phase == 1) return sync_hand_out_colsums(p, cb, 1);        // (fused tail: H <= 64)
  const int fr_here = *loss == kLossTailBwdApply;
  tail_bwd_apply_kernel<<<dim3((unsigned)tt_cdiv(p.B, 64), (unsigned)(n + fr_here)), kTailThreads, 0, st>>>(tp, ctx->dq->loss, fr_here);
  if (fr_here) tt_deferred_taken(ctx, TT_DQ_LOSS);
  TT_LAUNCH_CHECK();
  return TT_OK;
}
// The wide tail's backward head: L2-normalise backward, the output layer's data-gradient GEMM and the BN column sums of the last
// block in one kernel (the weight-gradient GEMM stays the split-K one); column-sum finish + BN backward apply in a second, in
// the block loop
int bwd_wide_head(const Pass& p, TnPending* pend) {
  const int i = p.nh - 1;
  Batch<TailBwdArgs> tb{};
  for (int t = 0; t < p.n; ++t)
    tb.a[t] = TailBwdArgs{p.A[t]->y, p.A[t]->emb, p.d_emb[t], p.G[t]->d_y, p.P[t]->d_out, p.P[t]->w_out, nullptr, d_in(p, p.nh, t),
                          col_args(p, i, t, nullptr, 0), nullptr, nullptr};
  tail_bwd_wide_kernel<<<dim3((unsigned)block_dims(p, i).cmax, (unsigned)p.n), kWideBwdThreads, 0, p.st>>>(tb, p.drop, p.dropout_p, p.seed, p.seed_dev);
  TT_LAUNCH_CHECK();
  return launch_layer_bwd(p, p.nh, pend, false);
}
// First block + projection: three independent products of d_pre in ONE launch (tt_gemm.h: GemmBack); the projection's gradients
// come out of the slab-reduction launch, d_x[:, 0:h0] is not materialised.  Ends the pass.
int bwd_first_block_back(const Pass& p, const GemmBack* gb, TnPending* pend, bool with_loss) {
  tt_ctx* ctx = p.ctx;
  int mine = 0;
  if (with_loss)
    if (int rc = tt_deferred_host(ctx, TT_DQ_LOSS, p.st, &mine)) return rc;
  if (int rc = tt_gemm_back_batched(p.st, gb, p.n, pend, (mine & TT_DQ_LOSS) ? &ctx->dq->loss : nullptr)) return rc;
  tt_deferred_taken(ctx, mine & TT_DQ_LOSS);
  if (ctx->dq->defer_slabs) return tt_deferred_queue_slabs(ctx, p.st, pend);     // rides in tt_embed_grad_bwd's launch
  return tt_gemm_tn_flush(p.st, pend);
}

}  // namespace

extern "C" {

size_t tt_tower_workspace_bytes(const tt_tower_params* p, int64_t B) {
  if (!p || p->n_hidden < 0 || p->n_hidden > TT_MAX_HIDDEN) return 0;
  return ws_layout(p, B, nullptr).total;
}

int tt_towers_mlp_fwd(tt_ctx* ctx, int32_t n, const tt_tower_params* const* P, const tt_tower_acts* const* A, int64_t B,
                      int32_t train, float dropout_p, uint64_t seed, const uint64_t* seed_dev, void* const* workspaces,
                      const size_t* workspace_bytes, tt_stream stream) {
  TT_CHECK_ARG(ctx && A, "tt_towers_mlp_fwd: NULL argument");
  if (int rc = check_batch(n, P, B, dropout_p, workspaces, workspace_bytes, "tt_towers_mlp_fwd")) return rc;
  if (B == 0) return TT_OK;
  for (int t = 0; t < n; ++t)
    TT_CHECK_ARG(A[t] && A[t]->dense && A[t]->x && A[t]->y && A[t]->emb, "tt_towers_mlp_fwd: NULL activation buffers");
  const Pass p = make_pass(ctx, stream, n, P, A, nullptr, nullptr, B, train, dropout_p, seed, seed_dev, workspaces);
  hipStream_t st = p.st;
  if (int rc = check_sync_phase(p, "tt_towers_mlp_fwd")) return rc;
  const int nh = p.nh, phase = p.phase;
  const bool fused = tail_fusable(n, P, train);
  const bool front = fused && front_fusable(n, P, A);    // projection + block Linear + chunk statistics in one launch
  const bool gather = front_gathers(n, P, A, B, train);  // ... and the embedding rows of x gathered in it
  for (int t = 0; t < n && !gather; ++t)                 // nobody else fills x[:, h0:]: the caller asks tt_towers_fwd_gathers first
    if (wants_gather(A[t])) {
      tt_set_error("tt_towers_mlp_fwd: gather fields set on a pass that cannot gather (tt_towers_fwd_gathers says which can)");
      return TT_ERR_UNSUPPORTED;
    }
  if (phase != 2 && !front) {
    GemmNT nt[TT_MAX_SIDES];                              // x[:, 0:h0] = dense W_proj^T + b_proj        (base_tower.py:133)
    for (int t = 0; t < n; ++t) {
      nt[t] = nt_item(p, t, A[t]->dense, P[t]->w_proj, P[t]->b_proj, reinterpret_cast<float*>(A[t]->x), P[t]->h0 + P[t]->kcat_e, P[t]->h0, P[t]->din);
      nt[t].c_bf16 = P[t]->x_dtype == TT_BF16;
    }
    if (int rc = tt_gemm_nt_batched(st, nt, n)) return rc;
  }
  NtDeferred nd[TT_MAX_SIDES];
  for (int i = 0; i < nh; ++i) {
    const bool tail = fused && i == nh - 1;
    Batch<BnStatArgs> bs{}; Batch<BnApplyArgs> ba{};
    for (int t = 0; t < n; ++t) {
      TT_CHECK_ARG(A[t]->pre[i] && A[t]->act[i] && A[t]->mean[i] && A[t]->rstd[i], "tt_towers_mlp_fwd: NULL buffers of block %d", i);
      bs.a[t] = bn_stat_args(p, i, t);
      ba.a[t] = bn_apply_args(p, i, t);
    }
    const BlockDims dim = block_dims(p, i);
    if (phase != 2 && !(front && tail))
      if (int rc = launch_layer_nt(p, i, tail ? nd : nullptr)) return rc;
    if (tail) return fwd_narrow_tail(p, i, bs, nd, front, gather, dim);
    if (train) {
      if (phase != 2) {
        bn_stats_partial_kernel<<<dim3((unsigned)tt_cdiv(dim.hmax, 64), (unsigned)dim.cmax, (unsigned)n), kThreads, 0, st>>>(bs);
        TT_LAUNCH_CHECK();
      }
      if (phase == 1) return sync_hand_out_stats(p, bs, dim.hmax);       // SyncBN on the separate kernels (any width)
      if (phase == 2) sync_take_rank_stats(p, bs);
      if (i == nh - 1 && !fused && wide_tail_ok(n, P, train)) return fwd_wide_tail(p, i, bs);
      bn_stats_finish_kernel<<<dim3((unsigned)tt_cdiv(dim.hmax, 64), (unsigned)n), kThreads, 0, st>>>(bs);
      TT_LAUNCH_CHECK();
    } else {
      bn_eval_prepare_kernel<<<dim3((unsigned)tt_cdiv(dim.hmax, 256), (unsigned)n), 256, 0, st>>>(bs);
      TT_LAUNCH_CHECK();
    }
    bn_apply_kernel<<<dim3((unsigned)ew_grid(ctx, dim.tmax, n), (unsigned)n), kThreads, 0, st>>>(ba, p.drop, dropout_p, seed, seed_dev);
    TT_LAUNCH_CHECK();
  }
  // output Linear, L2 normalise; emb_packed is honoured on every path: here by the pack kernel
  if (int rc = launch_layer_nt(p, nh, nullptr)) return rc;
  Batch<NormArgs> na{};
  for (int t = 0; t < n; ++t) na.a[t] = NormArgs{A[t]->y, nullptr, nullptr, (int)B, P[t]->d_out, A[t]->emb};
  if (!launch_l2norm_fast<false>(st, na, n, B)) l2norm_fwd_kernel<<<dim3((unsigned)tt_cdiv(B, 4), (unsigned)n), kThreads, 0, st>>>(na);
  TT_LAUNCH_CHECK();
  for (int t = 0; t < n; ++t)
    if (A[t]->emb_packed)
      if (int rc = tt_score_pack_bf16(ctx, A[t]->emb, B, P[t]->d_out, A[t]->emb_pack_scale, A[t]->emb_packed, stream)) return rc;
  return TT_OK;
}

int tt_towers_fwd_gathers(int32_t n, const tt_tower_params* const* P, const tt_tower_acts* const* A, int64_t B, int32_t train) {
  if (n < 1 || n > TT_MAX_SIDES || !P || !A) return 0;
  for (int t = 0; t < n; ++t)
    if (!P[t] || !A[t] || P[t]->n_hidden < 0 || P[t]->n_hidden > TT_MAX_HIDDEN || !A[t]->dense || !A[t]->x) return 0;
  for (int t = 0; t < n; ++t)
    if (P[t]->n_hidden != P[0]->n_hidden || P[t]->compute_dtype != P[0]->compute_dtype) return 0;
  return front_gathers(n, P, A, B, train) ? 1 : 0;
}

int tt_towers_mlp_bwd(tt_ctx* ctx, int32_t n, const tt_tower_params* const* P, const tt_tower_acts* const* A,
                      const float* const* d_emb, const tt_tower_grads* const* G, int64_t B, int32_t train, float dropout_p,
                      uint64_t seed, const uint64_t* seed_dev, void* const* workspaces, const size_t* workspace_bytes,
                      tt_stream stream) {
  TT_CHECK_ARG(ctx && A && G && d_emb, "tt_towers_mlp_bwd: NULL argument");
  if (int rc = check_batch(n, P, B, dropout_p, workspaces, workspace_bytes, "tt_towers_mlp_bwd")) return rc;
  TT_CHECK_ARG(B >= 1, "tt_towers_mlp_bwd: B < 1");
  for (int t = 0; t < n; ++t) {
    const tt_tower_grads* g = G[t];
    TT_CHECK_ARG(A[t] && g && d_emb[t] && g->w_proj && g->b_proj && g->w_out && g->b_out && g->d_x && g->d_y,
                 "tt_towers_mlp_bwd: NULL gradient buffers");
  }
  const Pass p = make_pass(ctx, stream, n, P, A, G, d_emb, B, train, dropout_p, seed, seed_dev, workspaces);
  hipStream_t st = p.st;
  const int nh = p.nh, phase = p.phase;
  const bool fused = tail_fusable(n, P, train);
  const bool wide = !fused && wide_tail_ok(n, P, train);  // tail_bwd_wide_kernel + tail_bwd_apply_wide_kernel
  if (int rc = check_sync_phase(p, "tt_towers_mlp_bwd")) return rc;
  // a score backward held back for this pass (TT_OPT_FUSE_SCORE_TAIL) writes d_emb: only the fused narrow tail can host it
  if (!(fused && phase == 0))
    if (int rc = tt_deferred_flush(ctx, TT_DQ_SCORE_BWD)) return rc;
  if (!fused && !wide && phase != 2) {
    Batch<NormArgs> na{};
    for (int t = 0; t < n; ++t) na.a[t] = NormArgs{A[t]->y, A[t]->emb, d_emb[t], (int)B, P[t]->d_out, G[t]->d_y};
    if (!launch_l2norm_fast<true>(st, na, n, B)) l2norm_bwd_kernel<<<dim3((unsigned)tt_cdiv(B, 4), (unsigned)n), kThreads, 0, st>>>(na);
    TT_LAUNCH_CHECK();
  }
  for (int t = 0; t < n; ++t) TT_CHECK_ARG(d_in(p, nh, t), "tt_towers_mlp_bwd: NULL scratch buffer");
  // the slab reductions of all weight-gradient GEMMs run as ONE launch at the end (nothing in this pass reads them)
  TnPending pend;
  GemmBack gb[TT_MAX_SIDES];
  const bool back = back_items(p, gb);                   // the first block's one launch: decided once, for the tail and for block 0
  LossHost loss = kLossNobody;
  // the output layer (and, in the tails, the last block's column sums)
  if (fused) {
    if (int rc = bwd_narrow_tail(p, back, &loss)) return rc;
    if (phase == 1) return TT_OK;                         // SyncBN: the column sums are handed out, the pass stops
  } else if (wide) {
    if (phase != 2)
      if (int rc = bwd_wide_head(p, &pend)) return rc;
  } else if (phase != 2) {
    if (int rc = launch_layer_bwd(p, nh, &pend)) return rc;
  }
  for (int i = nh - 1; i >= 0; --i) {
    const bool last = i == nh - 1;
    if (int rc = check_block_grads(p, i)) return rc;
    Batch<ColArgs> cb{}; Batch<BnBwdArgs> bb{};
    for (int t = 0; t < n; ++t) {
      cb.a[t] = col_args(p, i, t, d_in(p, i + 1, t), P[t]->hidden[i]);
      bb.a[t] = bn_bwd_args(p, i, t);
    }
    const BlockDims dim = block_dims(p, i);
    if (wide && last && phase != 1) {
      // the column sums of tail_bwd_wide_kernel (phase 2: of every rank, one "chunk" each) finished and applied in one launch
      Batch<TailApplyArgs> tp{};
      for (int t = 0; t < n; ++t) {
        tp.a[t] = TailApplyArgs{cb.a[t], bb.a[t], nullptr, nullptr, P[t]->d_out, nullptr, nullptr, 0, 1.f};
        if (phase == 2) tp.a[t].out_scale = sync_take_rank_colsums(p, tp.a[t].col, tp.a[t].bn, t, nullptr);
      }
      tail_bwd_apply_wide_kernel<<<dim3((unsigned)tt_cdiv(B, 64), (unsigned)n), kTailThreads, 0, st>>>(tp);
      TT_LAUNCH_CHECK();
    } else if (!(fused && last)) {                        // (the narrow tail has applied the last block's BN backward)
      if (phase != 2 && !(wide && last)) {
        colsum_partial_kernel<<<dim3((unsigned)tt_cdiv(dim.hmax, 64), (unsigned)dim.cmax, (unsigned)n), kThreads, 0, st>>>(cb, p.drop, dropout_p, seed, seed_dev);
        TT_LAUNCH_CHECK();
      }
      if (phase == 1) {                                   // SyncBN on the separate kernels: hand this rank's column sums out and stop
        if (int rc = tt_gemm_tn_flush(st, &pend)) return rc;     // (the output layer's weight-gradient slabs)
        return sync_hand_out_colsums(p, cb, (int)tt_cdiv(dim.hmax, 64));
      }
      if (phase == 2)
        for (int t = 0; t < n; ++t)                       // (the third third of the column workspace is free here)
          sync_take_rank_colsums(p, cb.a[t], bb.a[t], t, p.ws[t].col + 2 * (size_t)dim.hmax * kMaxChunks);
      colsum_finish_kernel<<<dim3((unsigned)tt_cdiv(dim.hmax, 64), (unsigned)n), kThreads, 0, st>>>(cb);
      TT_LAUNCH_CHECK();
      bn_bwd_apply_kernel<<<dim3((unsigned)ew_grid(ctx, dim.tmax, n), (unsigned)n), kThreads, 0, st>>>(bb, p.train, p.drop, dropout_p, seed, seed_dev);
      TT_LAUNCH_CHECK();
    }
    for (int t = 0; t < n; ++t) TT_CHECK_ARG(d_in(p, i, t), "tt_towers_mlp_bwd: NULL scratch buffer");
    if (i == 0 && back) return bwd_first_block_back(p, gb, &pend, loss == kLossGemmBack);
    if (int rc = launch_layer_bwd(p, i, &pend)) return rc;
  }
  // dense projection: from d_x[:, 0:h0]
  GemmTN tn[TT_MAX_SIDES];
  for (int t = 0; t < n; ++t) {
    tn[t] = tn_item(p, t, 0, reinterpret_cast<const float*>(G[t]->d_x), P[t]->h0 + P[t]->kcat_e, A[t]->dense, G[t]->w_proj, P[t]->h0, P[t]->din,
                    G[t]->b_proj);
    tn[t].a_bf16 = P[t]->dx_dtype == TT_BF16;
  }
  if (int rc = tt_gemm_tn_batched(st, tn, n, &pend)) return rc;
  // (not deferred like the one-launch first-block backward above: at these widths the slabs are HBM traffic, not launch
  //  latency -- measured 0.508 ms per step either way at scripts/train.py's [512, 256] -> 128)
  return tt_gemm_tn_flush(st, &pend);
}

int tt_tower_mlp_fwd(tt_ctx* ctx, const tt_tower_params* p, const tt_tower_acts* a, int64_t B, int32_t train, float dropout_p,
                     uint64_t seed, const uint64_t* seed_dev, void* workspace, size_t workspace_bytes, tt_stream stream) {
  return tt_towers_mlp_fwd(ctx, 1, &p, &a, B, train, dropout_p, seed, seed_dev, &workspace, &workspace_bytes, stream);
}

int tt_tower_mlp_bwd(tt_ctx* ctx, const tt_tower_params* p, const tt_tower_acts* a, const float* d_emb, const tt_tower_grads* g,
                     int64_t B, int32_t train, float dropout_p, uint64_t seed, const uint64_t* seed_dev, void* workspace,
                     size_t workspace_bytes, tt_stream stream) {
  return tt_towers_mlp_bwd(ctx, 1, &p, &a, &d_emb, &g, B, train, dropout_p, seed, seed_dev, &workspace, &workspace_bytes, stream);
}

int tt_linear_fwd(tt_ctx* ctx, const float* X, int64_t ldx, const float* W, const float* bias, float* Y, int64_t ldy, int64_t M,
                  int32_t N, int32_t K, int32_t relu, tt_stream stream) {
  TT_CHECK_ARG(ctx && (M == 0 || (X && W && Y)), "tt_linear_fwd: NULL argument");
  TT_CHECK_ARG(M >= 0 && N >= 1 && K >= 1 && ldx >= K && ldy >= N, "tt_linear_fwd: bad shape");
  TT_CHECK_ARG(M < ((int64_t)1 << 31), "tt_linear_fwd: M too large");
  return tt_gemm_nt(reinterpret_cast<hipStream_t>(stream), X, ldx, W, K, bias, Y, ldy, M, N, K, relu != 0);
}

}  // extern "C"

#ifdef TT_TAIL_STAMPS
extern "C" int tt_debug_tail_stamps(int which, unsigned long long* host_out /* [512 * 8] */) {
  return hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_tail_stamps), sizeof(unsigned long long) * 512 * 8,
                             sizeof(unsigned long long) * 512 * 8 * (size_t)which, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -2;
}
#endif
