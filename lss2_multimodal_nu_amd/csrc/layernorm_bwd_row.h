// The row arithmetic, partial sums and row split of the LayerNorm backward (C = 256, one wave per row, 4 channels per
// lane), shared by layernorm_bwd_kernel (K11, linear_grad.hip) and add_dropout_ln_bwd_kernel (K12,
// transformer_pointwise.hip): one text, so both give the same bits for the same row.
#pragma once
#include <algorithm>

#include "lss_device.h"

namespace {

constexpr int LN_C = 256;
constexpr int LN_MAXGROUPS = 1024;

// One row held by a whole wave (v: the input, gr: the incoming gradient, gm: gamma; this lane's 4 channels) -> this
// lane's 4 input gradients; adds the row's terms to dg (dgamma) and dbt (dbeta).
__device__ __forceinline__ f32x4 ln_bwd_row(const f32x4 v, const f32x4 gr, const f32x4 gm, float eps, f32x4& dg,
                                            f32x4& dbt) {
  // mean and 1 / sigma exactly as layernorm_kernel computes them
  const float mean = lss_wave_sum(v[0] + v[1] + v[2] + v[3]) * (1.f / LN_C);
  const f32x4 d = (f32x4){v[0] - mean, v[1] - mean, v[2] - mean, v[3] - mean};
  const float var = lss_wave_sum(d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + d[3] * d[3]) * (1.f / LN_C);
  const float inv = rsqrtf(var + eps);
  const f32x4 xh = (f32x4){d[0] * inv, d[1] * inv, d[2] * inv, d[3] * inv};
  const f32x4 ag = (f32x4){gr[0] * gm[0], gr[1] * gm[1], gr[2] * gm[2], gr[3] * gm[3]};
  const float m1 = lss_wave_sum(ag[0] + ag[1] + ag[2] + ag[3]) * (1.f / LN_C);
  const float m2 = lss_wave_sum(ag[0] * xh[0] + ag[1] * xh[1] + ag[2] * xh[2] + ag[3] * xh[3]) * (1.f / LN_C);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    dg[i] += gr[i] * xh[i];
    dbt[i] += gr[i];
  }
  return (f32x4){(ag[0] - m1 - xh[0] * m2) * inv, (ag[1] - m1 - xh[1] * m2) * inv, (ag[2] - m1 - xh[2] * m2) * inv,
                 (ag[3] - m1 - xh[3] * m2) * inv};
}

// The four waves' (2, 256) sums, added in wave order, as the workgroup's partial vector.
__device__ __forceinline__ void ln_bwd_write_partial(float (*red)[2 * LN_C], const f32x4 dg, const f32x4 dbt,
                                                     float* __restrict__ part) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    red[wave][4 * lane + i] = dg[i];
    red[wave][LN_C + 4 * lane + i] = dbt[i];
  }
  __syncthreads();
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    const int e = tid + 256 * m;
    part[(size_t)blockIdx.x * (2 * LN_C) + e] = ((red[0][e] + red[1][e]) + red[2][e]) + red[3][e];
  }
}

// x[i] = the S partials of element i added in split order (four interleaved chains, fixed final tree)
__device__ __forceinline__ float lg_sum_splits(const float* __restrict__ p, int S, size_t stride) {
  float s[4] = {0.f, 0.f, 0.f, 0.f};
  int k = 0;
  for (; k + 4 <= S; k += 4) {
#pragma unroll
    for (int i = 0; i < 4; ++i) s[i] += p[(size_t)(k + i) * stride];
  }
#pragma unroll
  for (int i = 0; i < 3; ++i)
    if (k + i < S) s[i] += p[(size_t)(k + i) * stride];
  return (s[0] + s[1]) + (s[2] + s[3]);
}

// out[0 .. 255] = dgamma, out[256 .. 511] = dbeta: the groups' partials in group order
__global__ __launch_bounds__(256) void layernorm_bwd_reduce_kernel(const float* __restrict__ part, int G,
                                                                   float* __restrict__ dgamma,
                                                                   float* __restrict__ dbeta) {
  const int e = blockIdx.x * 256 + threadIdx.x;  // grid of 2
  const float s = lg_sum_splits(part + e, G, (size_t)(2 * LN_C));
  if (e < LN_C) dgamma[e] = s;
  else dbeta[e - LN_C] = s;
}

struct LnSplit {
  long long rpg;
  int G;
};

inline LnSplit ln_split(long long rows) {
  LnSplit sp;
  const long long want = std::min<long long>((rows + 3) / 4, LN_MAXGROUPS);
  sp.rpg = (rows + want - 1) / want;
  sp.G = (int)((rows + sp.rpg - 1) / sp.rpg);
  return sp;
}

}  // namespace
