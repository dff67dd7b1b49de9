// K12: the pointwise remainder of the BEV transformer's training step as four streaming kernels (replaces the GELU,
// dropout and residual-add ATen ops, and their autograd nodes, of ref src/transformer_modules.py:207-208, 211-213).
//
// lss_gelu_dropout_fwd     y = bf16(gelu(h) m)                      (tokens, d_ff) hidden, bf16 in and out
// lss_gelu_dropout_bwd     dh = bf16(dy m (Phi(h) + h phi(h)))
//   8 bf16 per lane and step (16-B loads and stores), one Philox call per step, capped grid with a grid-stride loop.
//   erf by Abramowitz & Stegun 7.1.26 (lss_device.h: the text the forward GEMM epilogues use); its exp(-x^2), x = h / sqrt 2, IS
//   exp(-h^2 / 2): the backward's phi(h) costs no second exponential.  h = +-3e38: h^2 = inf, exp = 0, h phi = 0.
// lss_add_dropout_ln_fwd   s = res + a m (fp32),  y = LayerNorm(s)   rows of 256, one wave per row, 4 channels per lane
//   layernorm_kernel's two-pass arithmetic (bev_transformer.hip) on s: what the backward recomputes.
// lss_add_dropout_ln_bwd   lss_layernorm_bwd on s (layernorm_bwd_row.h: the same row arithmetic, partials and second
//   stage) with a second output da = ds m.  This file is compiled like linear_grad.hip (no SLP vectorisation), so the
//   shared rows contract to the same FMAs: ds, dgamma and dbeta equal lss_layernorm_bwd's on the same s bit for bit, and
//   forward and backward here agree on mean and 1 / sigma.  (lss_layernorm_fwd is compiled with SLP packing and fuses
//   other products: its y on the same s agrees within rounding, not in every bit.)
//
// The mask m in {0, scale} is recomputed from the device-resident seed in both directions (dropout_philox.h); it is
// applied as a MULTIPLY, so a non-finite value under a dropped element propagates as torch's mask multiply does.  A lane
// of the row kernels holds half of a call's 8 elements: lanes 2 i and 2 i + 1 run the same call (the row kernels move
// 14 - 18 bytes per element, the hidden kernels 4 - 6: that is where a call per 8 elements matters).
// No LDS beyond the (2, 256) x 4 partial sums of the backward, no scratch, no atomics.
#include <algorithm>

#include "dropout_philox.h"
#include "layernorm_bwd_row.h"
#include "lss_device.h"

namespace {

constexpr int PW_MAXBLOCKS = 2048;  // 256 CUs x 8 workgroups (cdna_hip_programming.md, Guideline 11)

__device__ __forceinline__ LssPhiloxKey pw_key(const unsigned long long* __restrict__ seed) {
  return lss_philox_key(seed[0], seed[1]);
}

// n8 = n / 8 steps of 8 elements; step q is Philox call q
template <bool DROP, bool BWD>
__global__ __launch_bounds__(256) void gelu_dropout_kernel(const uint4* __restrict__ h, const uint4* __restrict__ dy,
                                                           unsigned int n8, unsigned int thr, float scale,
                                                           const unsigned long long* __restrict__ seed,
                                                           uint4* __restrict__ out) {
  LssPhiloxKey key = {0u, 0u, 0u, 0u};
  if (DROP) key = pw_key(seed);
  const unsigned int stride = gridDim.x * 256u;
  // q + stride cannot wrap: n8 <= 2^29 and stride <= 2^19
  for (unsigned int q = blockIdx.x * 256u + threadIdx.x; q < n8; q += stride) {
    float v[8], g[8], o[8];
    lss_unpack8(h[q], v);
    if (BWD) lss_unpack8(dy[q], g);
    uint32_t w[4];
    if (DROP) lss_dropout_words(key, q, w);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float m = DROP ? lss_dropout_mul(w, j, thr, scale) : 1.f;
      if (BWD) o[j] = DROP ? g[j] * m * lss_gelu_grad(v[j]) : g[j] * lss_gelu_grad(v[j]);
      else o[j] = DROP ? lss_gelu(v[j]) * m : lss_gelu(v[j]);
    }
    out[q] = lss_pack8(o);
  }
}

// multipliers of this lane's 4 channels of `row`: element e = row * 256 + 4 lane + i lies in call e >> 3
template <bool DROP>
__device__ __forceinline__ f32x4 pw_row_mask(const LssPhiloxKey& key, long long row, int lane, unsigned int thr,
                                             float scale) {
  if (!DROP) return (f32x4){1.f, 1.f, 1.f, 1.f};
  uint32_t w[4];
  lss_dropout_words(key, (uint32_t)(row * (LN_C / 8)) + (uint32_t)(lane >> 1), w);
  const int j0 = (lane & 1) * 4;
  return (f32x4){lss_dropout_mul(w, j0, thr, scale), lss_dropout_mul(w, j0 + 1, thr, scale),
                 lss_dropout_mul(w, j0 + 2, thr, scale), lss_dropout_mul(w, j0 + 3, thr, scale)};
}

template <bool DROP, typename TR, typename TA>
__global__ __launch_bounds__(256) void add_dropout_ln_fwd_kernel(const TR* __restrict__ res, const TA* __restrict__ a,
                                                                 long long rows, unsigned int thr, float scale,
                                                                 const unsigned long long* __restrict__ seed,
                                                                 const float* __restrict__ gamma,
                                                                 const float* __restrict__ beta, float eps,
                                                                 float* __restrict__ s, float* __restrict__ y) {
  const int lane = threadIdx.x & 63;
  LssPhiloxKey key = {0u, 0u, 0u, 0u};
  if (DROP) key = pw_key(seed);
  const f32x4 g = *reinterpret_cast<const f32x4*>(gamma + 4 * lane);
  const f32x4 bt = *reinterpret_cast<const f32x4*>(beta + 4 * lane);
  // whole waves per row: the shuffles see all 64 lanes
  for (long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); row < rows; row += (long long)gridDim.x * 4) {
    const f32x4 r = lss_load4<TR>(res + row * LN_C + 4 * lane);
    const f32x4 av = lss_load4<TA>(a + row * LN_C + 4 * lane);
    f32x4 v;
    if (DROP) {
      const f32x4 m = pw_row_mask<true>(key, row, lane, thr, scale);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
#pragma clang fp contract(off)  // one multiply, one add: no FMA
        v[i] = r[i] + av[i] * m[i];
      }
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = r[i] + av[i];
    }
    lss_store4(s + row * LN_C + 4 * lane, v);
    // layernorm_kernel's arithmetic
    const float mean = lss_wave_sum(v[0] + v[1] + v[2] + v[3]) * (1.f / LN_C);
    const f32x4 d = (f32x4){v[0] - mean, v[1] - mean, v[2] - mean, v[3] - mean};
    const float var = lss_wave_sum(d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + d[3] * d[3]) * (1.f / LN_C);
    const float inv = rsqrtf(var + eps);
    lss_store4(y + row * LN_C + 4 * lane, (f32x4){d[0] * inv * g[0] + bt[0], d[1] * inv * g[1] + bt[1],
                                                 d[2] * inv * g[2] + bt[2], d[3] * inv * g[3] + bt[3]});
  }
}

template <bool DROP, typename TG, typename TA>
__global__ __launch_bounds__(256) void add_dropout_ln_bwd_kernel(const float* __restrict__ s, const TG* __restrict__ dy,
                                                                 const float* __restrict__ gamma, long long rows,
                                                                 long long rpg, float eps, unsigned int thr,
                                                                 float scale,
                                                                 const unsigned long long* __restrict__ seed,
                                                                 float* __restrict__ ds, TA* __restrict__ da,
                                                                 float* __restrict__ part) {
  __shared__ float red[4][2 * LN_C];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  LssPhiloxKey key = {0u, 0u, 0u, 0u};
  if (DROP) key = pw_key(seed);
  const long long r0 = (long long)blockIdx.x * rpg, r1 = min(rows, r0 + rpg);
  const f32x4 gm = *reinterpret_cast<const f32x4*>(gamma + 4 * lane);
  f32x4 dg = (f32x4){0.f, 0.f, 0.f, 0.f}, dbt = (f32x4){0.f, 0.f, 0.f, 0.f};
  for (long long row = r0 + wave; row < r1; row += 4) {
    const f32x4 v = lss_load4<float>(s + row * LN_C + 4 * lane);
    const f32x4 gr = lss_load4<TG>(dy + row * LN_C + 4 * lane);
    const f32x4 dx = ln_bwd_row(v, gr, gm, eps, dg, dbt);
    lss_store4(ds + row * LN_C + 4 * lane, dx);
    const f32x4 m = pw_row_mask<DROP>(key, row, lane, thr, scale);
    lss_store4(da + row * LN_C + 4 * lane,
              DROP ? (f32x4){dx[0] * m[0], dx[1] * m[1], dx[2] * m[2], dx[3] * m[3]} : dx);
  }
  ln_bwd_write_partial(red, dg, dbt, part);
}

inline bool pw_dt_ok(int dt) { return dt == LSS_DT_F32 || dt == LSS_DT_BF16; }

inline bool pw_thr_ok(int thr) { return thr >= 0 && thr <= 65535; }
// a NULL seed or thr == 0: identity
inline bool pw_drop(int thr, const void* seed) { return seed != nullptr && thr != 0; }

int gelu_dropout_launch(bool bwd, const void* h, const void* dy, long long n, int thr, float scale,
                        const long long* seed, void* out, void* stream) {
  LSS_CHECK_PTR(h); LSS_CHECK_PTR(out);
  if (bwd) LSS_CHECK_PTR(dy);
  if (!lss_gelu_dropout_ok(n) || !pw_thr_ok(thr)) return LSS_E_SHAPE;
  if (out == h || out == dy) return LSS_E_LAYOUT;  // the kernels read through __restrict__ pointers
  if (!lss_aligned(h, 16) || !lss_aligned(out, 16) || !lss_aligned(dy, 16) || !lss_aligned(seed, 8)) return LSS_E_ALIGN;
  const bool drop = pw_drop(thr, seed);
  const unsigned int n8 = (unsigned int)(n / 8);
  const dim3 grid(std::min<unsigned int>((n8 + 255u) / 256u, PW_MAXBLOCKS));
  hipStream_t st = lss_stream(stream);
#define LSS_GD(DROP, BWD)                                                                                         \
  hipLaunchKernelGGL((gelu_dropout_kernel<DROP, BWD>), grid, dim3(256), 0, st, static_cast<const uint4*>(h),      \
                     static_cast<const uint4*>(dy), n8, (unsigned int)thr, scale, reinterpret_cast<const unsigned long long*>(seed), \
                     static_cast<uint4*>(out))
  if (drop && bwd) LSS_GD(true, true);
  else if (drop) LSS_GD(true, false);
  else if (bwd) LSS_GD(false, true);
  else LSS_GD(false, false);
#undef LSS_GD
  return lss_launch_status();
}

}  // namespace

extern "C" int lss_gelu_dropout_ok(long long n) { return n >= 8 && n <= (1LL << 32) && n % 8 == 0; }

extern "C" int lss_gelu_dropout_fwd(const void* h, long long n, int thr, float scale, const long long* seed, void* y,
                                    void* stream) {
  return gelu_dropout_launch(false, h, nullptr, n, thr, scale, seed, y, stream);
}

extern "C" int lss_gelu_dropout_bwd(const void* h, const void* dy, long long n, int thr, float scale,
                                    const long long* seed, void* dh, void* stream) {
  return gelu_dropout_launch(true, h, dy, n, thr, scale, seed, dh, stream);
}

extern "C" int lss_add_dropout_ln_ok(long long rows, int C) { return rows >= 1 && rows <= (1LL << 22) && C == LN_C; }

extern "C" size_t lss_add_dropout_ln_bwd_workspace_bytes(long long rows) {
  if (!lss_add_dropout_ln_ok(rows, LN_C)) return 0;
  return (size_t)ln_split(rows).G * 2 * LN_C * sizeof(float);
}

extern "C" int lss_add_dropout_ln_fwd(const void* res, int res_dt, const void* a, int a_dt, long long rows, int C,
                                      int thr, float scale, const long long* seed, const float* gamma,
                                      const float* beta, float eps, float* s, float* y, void* stream) {
  LSS_CHECK_PTR(res); LSS_CHECK_PTR(a); LSS_CHECK_PTR(gamma); LSS_CHECK_PTR(beta); LSS_CHECK_PTR(s); LSS_CHECK_PTR(y);
  if (!lss_add_dropout_ln_ok(rows, C) || !pw_thr_ok(thr)) return LSS_E_SHAPE;
  const bool drop = pw_drop(thr, seed);
  if (!pw_dt_ok(res_dt) || !pw_dt_ok(a_dt)) return LSS_E_LAYOUT;
  if (!lss_aligned(seed, 8) || !lss_aligned(res, 16) || !lss_aligned(a, 16) || !lss_aligned(gamma, 16) || !lss_aligned(beta, 16) ||
      !lss_aligned(s, 16) || !lss_aligned(y, 16))
    return LSS_E_ALIGN;
  const dim3 grid((unsigned int)std::min<long long>((rows + 3) / 4, PW_MAXBLOCKS));
  hipStream_t st = lss_stream(stream);
  typedef unsigned short bf;
#define LSS_ALF(DROP, TR, TA)                                                                                   \
  hipLaunchKernelGGL((add_dropout_ln_fwd_kernel<DROP, TR, TA>), grid, dim3(256), 0, st,                         \
                     static_cast<const TR*>(res), static_cast<const TA*>(a), rows, (unsigned int)thr, scale,    \
                     reinterpret_cast<const unsigned long long*>(seed), gamma, beta, eps, s, y)
  switch ((drop ? 4 : 0) | (res_dt == LSS_DT_BF16 ? 2 : 0) | (a_dt == LSS_DT_BF16 ? 1 : 0)) {
    case 0: LSS_ALF(false, float, float); break;
    case 1: LSS_ALF(false, float, bf); break;
    case 2: LSS_ALF(false, bf, float); break;
    case 3: LSS_ALF(false, bf, bf); break;
    case 4: LSS_ALF(true, float, float); break;
    case 5: LSS_ALF(true, float, bf); break;
    case 6: LSS_ALF(true, bf, float); break;
    default: LSS_ALF(true, bf, bf); break;
  }
#undef LSS_ALF
  return lss_launch_status();
}

extern "C" int lss_add_dropout_ln_bwd(const float* s, const void* dy, int dy_dt, const float* gamma, long long rows,
                                      int C, float eps, int thr, float scale, const long long* seed,
                                      void* workspace, size_t workspace_bytes, float* ds, void* da, int da_dt,
                                      float* dgamma, float* dbeta, void* stream) {
  LSS_CHECK_PTR(s); LSS_CHECK_PTR(dy); LSS_CHECK_PTR(gamma); LSS_CHECK_PTR(workspace);
  LSS_CHECK_PTR(ds); LSS_CHECK_PTR(da); LSS_CHECK_PTR(dgamma); LSS_CHECK_PTR(dbeta);
  if (!lss_add_dropout_ln_ok(rows, C) || !pw_thr_ok(thr)) return LSS_E_SHAPE;
  const bool drop = pw_drop(thr, seed);
  if (!pw_dt_ok(dy_dt) || !pw_dt_ok(da_dt)) return LSS_E_LAYOUT;
  if (!lss_aligned(seed, 8) || !lss_aligned(s, 16) || !lss_aligned(dy, 16) || !lss_aligned(gamma, 16) || !lss_aligned(ds, 16) ||
      !lss_aligned(da, 16) || !lss_aligned(workspace, 16) || !lss_aligned(dgamma, 4) || !lss_aligned(dbeta, 4))
    return LSS_E_ALIGN;
  if (workspace_bytes < lss_add_dropout_ln_bwd_workspace_bytes(rows)) return LSS_E_WORKSPACE;
  const LnSplit sp = ln_split(rows);
  float* part = static_cast<float*>(workspace);
  hipStream_t st = lss_stream(stream);
  typedef unsigned short bf;
#define LSS_ALB(DROP, TG, TA)                                                                                       \
  hipLaunchKernelGGL((add_dropout_ln_bwd_kernel<DROP, TG, TA>), dim3(sp.G), dim3(256), 0, st, s,                    \
                     static_cast<const TG*>(dy), gamma, rows, sp.rpg, eps, (unsigned int)thr, scale,                \
                     reinterpret_cast<const unsigned long long*>(seed), ds, static_cast<TA*>(da), part)
  switch ((drop ? 4 : 0) | (dy_dt == LSS_DT_BF16 ? 2 : 0) | (da_dt == LSS_DT_BF16 ? 1 : 0)) {
    case 0: LSS_ALB(false, float, float); break;
    case 1: LSS_ALB(false, float, bf); break;
    case 2: LSS_ALB(false, bf, float); break;
    case 3: LSS_ALB(false, bf, bf); break;
    case 4: LSS_ALB(true, float, float); break;
    case 5: LSS_ALB(true, float, bf); break;
    case 6: LSS_ALB(true, bf, float); break;
    default: LSS_ALB(true, bf, bf); break;
  }
#undef LSS_ALB
  const int lrc = lss_launch_status();
  if (lrc != 0) return lrc;
  hipLaunchKernelGGL(layernorm_bwd_reduce_kernel, dim3(2), dim3(256), 0, st, part, sp.G, dgamma, dbeta);
  return lss_launch_status();
}
