// The score kernels' operand images, written once per step: the bf16 packing ([rows image | fragment image], tt_score_bf16.h), its
// bf16x3 variant ([hi | lo]) and the fp8 packing ([fp8 rows image | bf16 fragment image | fp8 fragment image]).  Shares nothing with
// the sweeps of tt_score_bf16.hip / tt_score_sym.hip but the layouts.
#include "tt_score_bf16.h"

namespace {

using namespace ttscore;

// ---- pack ------------------------------------------------------------------------------------------
struct PackArgs { const float* X; int64_t R, Rp; __bf16* rows; __bf16* frag; float scale; __bf16* rows_lo; __bf16* frag_lo; };
struct PackBatch { PackArgs a[2]; };

// X3 (bf16x3 packing): also the lo images, bf16(p - hi) of p = scale x, in the same layout.
template <bool X3>
__global__ __launch_bounds__(256) void pack_bf16_kernel(PackBatch batch, int D, int Dp) {
  const PackArgs& pa = batch.a[blockIdx.y];
  const float* __restrict__ X = pa.X;
  const int64_t R = pa.R, Rp = pa.Rp;
  __bf16* __restrict__ rows = pa.rows;
  __bf16* __restrict__ frag = pa.frag;
  const float sc = pa.scale;
  const int64_t nchunk = Rp * Dp / 8;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < 2 * nchunk; c += stride) {
    bf16x8 v, vl;
    if (c < nchunk) {                                   // k-fragment image [t][k-step][half][row in tile][8]
      const int ci = (int)(c & 31), hh = (int)((c >> 5) & 1);
      const int64_t q = c >> 6;
      const int ks = (int)(q % (Dp / 16));
      const int64_t row = 32 * (q / (Dp / 16)) + ci;
      const int d0 = 16 * ks + 8 * hh;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float p = (row < R && d0 + j < D) ? X[row * D + d0 + j] * sc : 0.f;
        v[j] = (__bf16)p;
        if (X3) vl[j] = (__bf16)sub_nc(p, (float)v[j]);
      }
      *reinterpret_cast<bf16x8*>(rows + c * 8) = v;
      if (X3) *reinterpret_cast<bf16x8*>(pa.rows_lo + c * 8) = vl;
    } else {                                            // fragment-ordered image [t][s][h][d][8]
      const int64_t f = c - nchunk;
      const int d = (int)(f % Dp);
      const int64_t rest = f / Dp;
      const int h = (int)(rest & 1), s = (int)((rest >> 1) & 1);
      const int64_t t = rest >> 2;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int64_t row = 32 * t + 16 * s + 8 * (j >> 2) + 4 * h + (j & 3);
        const float p = (row < R && d < D) ? X[row * D + d] * sc : 0.f;
        v[j] = (__bf16)p;
        if (X3) vl[j] = (__bf16)sub_nc(p, (float)v[j]);
      }
      *reinterpret_cast<bf16x8*>(frag + f * 8) = v;
      if (X3) *reinterpret_cast<bf16x8*>(pa.frag_lo + f * 8) = vl;
    }
  }
}

// ---- fp8 pack: [fp8 rows image | bf16 fragment image | fp8 fragment image] (tt_score_bf16.h) ----------------
// saturating: past e4m3's largest finite value the conversion would give NaN (64 * scale * x reaches 448 once |x| / T > 4.85,
// e.g. a row with one dominant coordinate at T = 0.2)
__device__ __forceinline__ float fp8_clamp(float v) { return __builtin_fminf(__builtin_fmaxf(v, -448.f), 448.f); }

__global__ __launch_bounds__(256) void pack_fp8_kernel(PackBatch batch, int D, int Dp) {
  const PackArgs& pa = batch.a[blockIdx.y];
  const float* __restrict__ X = pa.X;
  const int64_t R = pa.R, Rp = pa.Rp;
  char* __restrict__ rows8 = reinterpret_cast<char*>(pa.rows);
  __bf16* __restrict__ frag = pa.frag;
  const float sc = pa.scale;
  const int64_t n8 = Rp * Dp / 16, nfr = Rp * Dp / 8;      // 16-byte chunks of the rows image / of the bf16 fragment image
  char* __restrict__ frag8 = reinterpret_cast<char*>(frag) + Rp * Dp * 2;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int cpt = Dp * 2;                                   // fp8 chunks per 32-row tile
  for (int64_t ci = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; ci < 2 * n8 + nfr; ci += stride) {
    if (ci >= n8 + nfr) {                                   // fp8 fragment image [P][d][part][h][c][16]
      const int64_t f = ci - n8 - nfr;
      const int64_t P = f / (Dp * 4);
      const int w = (int)(f - P * (Dp * 4)), c = w & 31, h = (w >> 5) & 1, part = (w >> 6) & 1, d = w >> 7;
      const int col = 32 * d + c;
      i32x4 o;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int64_t row = 64 * P + 32 * part + rowmap(4 * q + j, h);
          v[j] = (row < R && col < D) ? fp8_clamp(X[row * D + col] * sc * kFp8Up) : 0.f;
        }
        int u = __builtin_amdgcn_cvt_pk_fp8_f32(v[0], v[1], 0, false);
        u = __builtin_amdgcn_cvt_pk_fp8_f32(v[2], v[3], u, true);
        o[q] = u;
      }
      *reinterpret_cast<i32x4*>(frag8 + f * 16) = o;
    } else if (ci < n8) {
      const int64_t t = ci / cpt;
      const int w = (int)(ci - t * cpt), row_in = w & 31, g5 = w >> 5;
      const int d0 = 64 * (g5 >> 2) + 32 * (g5 & 1) + 16 * ((g5 >> 1) & 1);
      const int64_t row = 32 * t + row_in;
      float v[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) v[j] = (row < R && d0 + j < D) ? fp8_clamp(X[row * D + d0 + j] * sc * kFp8Up) : 0.f;
      i32x4 o;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        int u = __builtin_amdgcn_cvt_pk_fp8_f32(v[4 * q], v[4 * q + 1], 0, false);
        u = __builtin_amdgcn_cvt_pk_fp8_f32(v[4 * q + 2], v[4 * q + 3], u, true);
        o[q] = u;
      }
      *reinterpret_cast<i32x4*>(rows8 + ci * 16) = o;
    } else {                                               // fragment-ordered bf16 image [t][s][h][d][8], as pack_bf16_kernel
      const int64_t f = ci - n8;
      const int d = (int)(f % Dp);
      const int64_t rest = f / Dp;
      const int h = (int)(rest & 1), s = (int)((rest >> 1) & 1);
      const int64_t t = rest >> 2;
      bf16x8 v;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int64_t row = 32 * t + 16 * s + 8 * (j >> 2) + 4 * h + (j & 3);
        v[j] = (__bf16)((row < R && d < D) ? X[row * D + d] * sc : 0.f);
      }
      *reinterpret_cast<bf16x8*>(frag + f * 8) = v;
    }
  }
}


// The same three images from ONE read of X: a workgroup stages 64 rows (a tile pair) in LDS -- coalesced, 16 bytes per lane -- and
// every thread then assembles 16-byte chunks of the images from there.  pack_fp8_kernel reads X once per image, the rows image
// with 64 different rows per wave-instruction (536 MB of traffic for 134 MB of input at B = 65536, D = 256: 179 us).  Same
// arithmetic per element: bit-identical images (tests compare the packed buffers with torch's conversion).
constexpr int kPackTileRows = 64, kPackPad = 4;
__global__ __launch_bounds__(256) void pack_fp8_tile_kernel(PackBatch batch, int D, int Dp) {
  extern __shared__ __attribute__((aligned(16))) float xt[];          // [64][Dp + 4]
  const PackArgs& pa = batch.a[blockIdx.y];
  const float* __restrict__ X = pa.X;
  const int64_t R = pa.R, Rp = pa.Rp;
  const int64_t P = blockIdx.x;
  if (P * kPackTileRows >= Rp) return;
  char* __restrict__ rows8 = reinterpret_cast<char*>(pa.rows);
  __bf16* __restrict__ frag = pa.frag;
  char* __restrict__ frag8 = reinterpret_cast<char*>(frag) + Rp * Dp * 2;
  const float sc = pa.scale;
  const int ld = Dp + kPackPad, tid = threadIdx.x;
  // stage: rows 64 P .. 64 P + 63, columns [0, Dp); zero outside [0, R) x [0, D)
  if (D == Dp && (reinterpret_cast<uintptr_t>(X) & 15) == 0) {
    const int per_row = Dp / 4;
    for (int e = tid; e < kPackTileRows * per_row; e += 256) {
      const int r = e / per_row, c4 = e - r * per_row;
      const int64_t row = P * kPackTileRows + r;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (row < R) v = reinterpret_cast<const float4*>(X + row * D)[c4];
      *reinterpret_cast<float4*>(xt + r * ld + 4 * c4) = v;
    }
  } else {
    for (int e = tid; e < kPackTileRows * Dp; e += 256) {
      const int r = e / Dp, c = e - r * Dp;
      const int64_t row = P * kPackTileRows + r;
      xt[r * ld + c] = (row < R && c < D) ? X[row * D + c] : 0.f;
    }
  }
  __syncthreads();
  // fp8 rows image: tiles 2 P, 2 P + 1; chunk w of a tile = (row w & 31, group w >> 5)
  const int cpt = Dp * 2;
  for (int e = tid; e < 2 * cpt; e += 256) {
    const int t = e / cpt, w = e - t * cpt, row_in = w & 31, g5 = w >> 5;
    const int d0 = 64 * (g5 >> 2) + 32 * (g5 & 1) + 16 * ((g5 >> 1) & 1);
    const float* src = xt + (32 * t + row_in) * ld + d0;
    i32x4 o;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float4 v = *reinterpret_cast<const float4*>(src + 4 * q);
      int u = __builtin_amdgcn_cvt_pk_fp8_f32(fp8_clamp(v.x * sc * kFp8Up), fp8_clamp(v.y * sc * kFp8Up), 0, false);
      u = __builtin_amdgcn_cvt_pk_fp8_f32(fp8_clamp(v.z * sc * kFp8Up), fp8_clamp(v.w * sc * kFp8Up), u, true);
      o[q] = u;
    }
    *reinterpret_cast<i32x4*>(rows8 + ((2 * P + t) * cpt + w) * 16) = o;
  }
  // bf16 fragment image [t][s][h][d][8]
  for (int e = tid; e < 8 * Dp; e += 256) {
    const int d = e % Dp, rest = e / Dp, h = rest & 1, s2 = (rest >> 1) & 1, t = rest >> 2;
    bf16x8 v;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (__bf16)(xt[(32 * t + 16 * s2 + 8 * (j >> 2) + 4 * h + (j & 3)) * ld + d] * sc);
    *reinterpret_cast<bf16x8*>(frag + ((((2 * P + t) * 2 + s2) * 2 + h) * Dp + d) * 8) = v;
  }
  // fp8 fragment image [P][d][part][h][c][16]
  for (int e = tid; e < 4 * Dp; e += 256) {
    const int c = e & 31, h = (e >> 5) & 1, part = (e >> 6) & 1, d = e >> 7;
    const int col = 32 * d + c;
    i32x4 o;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = fp8_clamp(xt[(32 * part + rowmap(4 * q + j, h)) * ld + col] * sc * kFp8Up);
      int u = __builtin_amdgcn_cvt_pk_fp8_f32(v[0], v[1], 0, false);
      u = __builtin_amdgcn_cvt_pk_fp8_f32(v[2], v[3], u, true);
      o[q] = u;
    }
    *reinterpret_cast<i32x4*>(frag8 + (P * (Dp * 4) + e) * 16) = o;
  }
}

}  // namespace

extern "C" {

size_t tt_score_pack_bytes(int64_t R, int32_t D) {
  if (R < 0 || D < 1 || D > 256) return 0;
  return (size_t)(4 * rup(R > 0 ? R : 1, 64) * padded_d(D));
}

int tt_score_pack2_bf16(tt_ctx* ctx, const float* X0, int64_t R0, void* packed0, const float* X1, int64_t R1, void* packed1,
                        int32_t D, float scale0, float scale1, tt_stream stream) {
  TT_CHECK_ARG(ctx && X0 && packed0, "tt_score_pack_bf16: NULL argument");
  TT_CHECK_ARG(R0 >= 1 && D >= 1 && (X1 == nullptr || (packed1 && R1 >= 1)), "tt_score_pack_bf16: bad shape");
  if (D > 256) {
    tt_set_error("tt_score_pack_bf16: D=%d > 256 not supported", D);
    return TT_ERR_UNSUPPORTED;
  }
  TT_CHECK_ARG(tt_aligned(packed0, 16) && tt_aligned(packed1, 16), "tt_score_pack_bf16: packed buffers must be 16-byte aligned");
  const int Dp = padded_d(D);
  PackBatch b{};
  const int n = X1 ? 2 : 1;
  int64_t maxchunks = 1;
  for (int i = 0; i < n; ++i) {
    const int64_t R = i ? R1 : R0, Rp = rup(R, 64);     // a workgroup reads up to 64 consecutive rows of its operand
    __bf16* base = reinterpret_cast<__bf16*>(i ? packed1 : packed0);
    const float sc = i ? scale1 : scale0;
    b.a[i] = PackArgs{i ? X1 : X0, R, Rp, base, base + Rp * Dp, sc == 0.f ? 1.f : sc};
    const int64_t chunks = 2 * Rp * Dp / 8;
    maxchunks = chunks > maxchunks ? chunks : maxchunks;
  }
  int64_t grid = tt_cdiv(maxchunks, 256);
  const int64_t cap = (int64_t)ctx->num_cus * 4;
  if (grid > cap) grid = cap;
  pack_bf16_kernel<false><<<dim3((unsigned)grid, (unsigned)n), 256, 0, reinterpret_cast<hipStream_t>(stream)>>>(b, D, Dp);
  TT_LAUNCH_CHECK();
  return TT_OK;
}

int tt_score_pack_bf16(tt_ctx* ctx, const float* X, int64_t R, int32_t D, float scale, void* packed, tt_stream stream) {
  return tt_score_pack2_bf16(ctx, X, R, packed, nullptr, 0, nullptr, D, scale, 1.f, stream);
}

size_t tt_score_pack_fp8_bytes(int64_t R, int32_t D) {
  if (R < 0 || D < 1 || D > 256) return 0;
  return (size_t)(4 * rup(R > 0 ? R : 1, 64) * padded_d8(D));
}

int tt_score_pack2_fp8(tt_ctx* ctx, const float* X0, int64_t R0, void* packed0, const float* X1, int64_t R1, void* packed1,
                       int32_t D, float scale0, float scale1, tt_stream stream) {
  TT_CHECK_ARG(ctx && X0 && packed0, "tt_score_pack2_fp8: NULL argument");
  TT_CHECK_ARG(R0 >= 1 && D >= 1 && D <= 256 && (X1 == nullptr || (packed1 && R1 >= 1)), "tt_score_pack2_fp8: bad shape");
  TT_CHECK_ARG(tt_aligned(packed0, 16) && tt_aligned(packed1, 16), "tt_score_pack2_fp8: packed buffers must be 16-byte aligned");
  const int Dp = padded_d8(D);
  PackBatch b{};
  const int n = X1 ? 2 : 1;
  int64_t maxchunks = 1;
  for (int i = 0; i < n; ++i) {
    const int64_t R = i ? R1 : R0, Rp = rup(R, 64);
    char* base = reinterpret_cast<char*>(i ? packed1 : packed0);
    const float sc = i ? scale1 : scale0;
    b.a[i] = PackArgs{i ? X1 : X0, R, Rp, reinterpret_cast<__bf16*>(base), reinterpret_cast<__bf16*>(base + Rp * Dp), sc == 0.f ? 1.f : sc};
    const int64_t chunks = 2 * (Rp * Dp / 16) + Rp * Dp / 8;
    maxchunks = chunks > maxchunks ? chunks : maxchunks;
  }
  int64_t maxRp = 0;
  for (int i = 0; i < n; ++i) maxRp = b.a[i].Rp > maxRp ? b.a[i].Rp : maxRp;
  if (maxRp >= 4096) {                                   // enough tile pairs to fill the chip: one read of X through LDS
    const size_t lds = (size_t)kPackTileRows * (Dp + kPackPad) * sizeof(float);
    TT_LDS_ONCE(lds, &pack_fp8_tile_kernel);
    pack_fp8_tile_kernel<<<dim3((unsigned)(maxRp / kPackTileRows), (unsigned)n), 256, lds, reinterpret_cast<hipStream_t>(stream)>>>(b, D, Dp);
    TT_LAUNCH_CHECK();
    return TT_OK;
  }
  int64_t grid = tt_cdiv(maxchunks, 256);
  const int64_t cap = (int64_t)ctx->num_cus * 4;
  if (grid > cap) grid = cap;
  pack_fp8_kernel<<<dim3((unsigned)grid, (unsigned)n), 256, 0, reinterpret_cast<hipStream_t>(stream)>>>(b, D, Dp);
  TT_LAUNCH_CHECK();
  return TT_OK;
}

// ---- bf16x3 (split-bf16) operands: [hi image | lo image] packings, three bf16 MFMAs per product ------------------------
size_t tt_score_pack_x3_bytes(int64_t R, int32_t D) { return 2 * tt_score_pack_bytes(R, D); }

int tt_score_pack2_bf16x3(tt_ctx* ctx, const float* X0, int64_t R0, void* packed0, const float* X1, int64_t R1, void* packed1,
                          int32_t D, float scale0, float scale1, tt_stream stream) {
  TT_CHECK_ARG(ctx && X0 && packed0, "tt_score_pack2_bf16x3: NULL argument");
  TT_CHECK_ARG(R0 >= 1 && D >= 1 && D <= 256 && (X1 == nullptr || (packed1 && R1 >= 1)), "tt_score_pack2_bf16x3: bad shape");
  TT_CHECK_ARG(tt_aligned(packed0, 16) && tt_aligned(packed1, 16), "tt_score_pack2_bf16x3: packed buffers must be 16-byte aligned");
  const int Dp = padded_d(D);
  PackBatch b{};
  const int n = X1 ? 2 : 1;
  int64_t maxchunks = 1;
  for (int i = 0; i < n; ++i) {
    const int64_t R = i ? R1 : R0, Rp = rup(R, 64);
    __bf16* base = reinterpret_cast<__bf16*>(i ? packed1 : packed0);
    __bf16* lo = reinterpret_cast<__bf16*>(reinterpret_cast<char*>(base) + x3_half_bytes(R, D));
    const float sc = i ? scale1 : scale0;
    b.a[i] = PackArgs{i ? X1 : X0, R, Rp, base, base + Rp * Dp, sc == 0.f ? 1.f : sc, lo, lo + Rp * Dp};
    const int64_t chunks = 2 * Rp * Dp / 8;
    maxchunks = chunks > maxchunks ? chunks : maxchunks;
  }
  int64_t grid = tt_cdiv(maxchunks, 256);
  const int64_t cap = (int64_t)ctx->num_cus * 4;
  if (grid > cap) grid = cap;
  pack_bf16_kernel<true><<<dim3((unsigned)grid, (unsigned)n), 256, 0, reinterpret_cast<hipStream_t>(stream)>>>(b, D, Dp);
  TT_LAUNCH_CHECK();
  return TT_OK;
}

}  // extern "C"
