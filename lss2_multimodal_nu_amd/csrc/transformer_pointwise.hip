// K12: the pointwise remainder of the BEV transformer's training step as streaming kernels (replaces the GELU, dropout
// and residual-add ATen ops, and their autograd nodes, of ref src/transformer_modules.py:207-208, 211-213), and with it
// the LayerNorm backward of K11 (the NativeLayerNormBackward nodes of ref src/transformer_modules.py:77-84, 170-215):
// every training row kernel of the transformer's LayerNorms is in this file.
//
// lss_gelu_dropout_fwd     y = bf16(gelu(h) m)                      (tokens, d_ff) hidden, bf16 in and out
// lss_gelu_dropout_bwd     dh = bf16(dy m (Phi(h) + h phi(h)))
//   8 bf16 per lane and step (16-B loads and stores), one Philox call per step, capped grid with a grid-stride loop.
//   erf by Abramowitz & Stegun 7.1.26 (lss_device.h: the text the forward GEMM epilogues use); its exp(-x^2), x = h / sqrt 2, IS
//   exp(-h^2 / 2): the backward's phi(h) costs no second exponential.  h = +-3e38: h^2 = inf, exp = 0, h phi = 0.
// lss_add_dropout_ln_fwd   s = res + a m (fp32),  y = LayerNorm(s)   rows of 256, one wave per row, 4 channels per lane
// lss_layernorm_bwd        backward of lss_layernorm_fwd (the forward saves only its input):
//     xhat = (x - mean) / sigma,   a = g gamma,   dx = (a - mean(a) - xhat mean(a xhat)) / sigma
//     dgamma = sum_rows g xhat,    dbeta = sum_rows g
// lss_add_dropout_ln_bwd   the same on s, with a second output da = ds m
//   One kernel template and one launcher serve both backward entries; the plain form has no mask and no second output
//   at compile time.  A workgroup walks a row range (wave w: rows r0 + w, r0 + w + 4, ..), its four waves' (2, 256) sums
//   are added in wave order and written as one partial vector; layernorm_bwd_reduce_kernel adds the workgroups'
//   partials in order.  Row ranges: groups = min(ceil(rows / 4), 1024), rows per group = ceil(rows / groups).
//
// Rounding of the rows.  Forward and backward take mean and 1 / sigma from ONE text, ln_stats, and the row functions
// are written with contraction off and every fused multiply-add as an explicit fmaf: their bits do not depend on the
// vectoriser, on a build flag or on the instantiation.  So ds, dgamma and dbeta of lss_add_dropout_ln_bwd equal
// lss_layernorm_bwd's on the same s bit for bit, and forward and backward here agree on mean and 1 / sigma.  The
// inference kernel (layernorm_kernel, bev_transformer.hip) has the same two-pass formula but rounds otherwise: it
// rounds the mean before subtracting it and adds rounded squares, where ln_stats never rounds the mean and chains the
// squares through FMAs.  Its y on the same input agrees within rounding, not in every bit.
//
// The mask m in {0, scale} is recomputed from the device-resident seed in both directions (dropout_philox.h); it is
// applied as a MULTIPLY, so a non-finite value under a dropped element propagates as torch's mask multiply does.  A lane
// of the row kernels holds half of a call's 8 elements: lanes 2 i and 2 i + 1 run the same call (the row kernels move
// 14 - 18 bytes per element, the hidden kernels 4 - 6: that is where a call per 8 elements matters).
// No LDS beyond the (2, 256) x 4 partial sums of the backward, no scratch, no atomics.
#include <algorithm>
#include <type_traits>

#include "dropout_philox.h"
#include "lss_device.h"

namespace {

constexpr int PW_MAXBLOCKS = 2048;  // 256 CUs x 8 workgroups (cdna_hip_programming.md, Guideline 11)
constexpr int LN_C = 256;
constexpr int LN_MAXGROUPS = 1024;

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

// ---- LayerNorm rows (C = 256): a whole wave holds one row, 4 channels per lane.  Contraction is off in these
// functions and every fusion is spelled fmaf: the program text says which products round.

// v -> d = v - mean (the mean is never rounded: d_i = fma(sum, -1 / C, v_i)) and inv = 1 / sigma
__device__ __forceinline__ void ln_stats(const f32x4 v, float eps, f32x4& d, float& inv) {
#pragma clang fp contract(off)
  const float sum = lss_wave_sum(v[0] + v[1] + v[2] + v[3]);
#pragma unroll
  for (int i = 0; i < 4; ++i) d[i] = fmaf(sum, -1.f / LN_C, v[i]);
  // the chain starts at channel 1: the order is part of the bits
  const float sq = fmaf(d[3], d[3], fmaf(d[2], d[2], fmaf(d[0], d[0], d[1] * d[1])));
  inv = rsqrtf(fmaf(lss_wave_sum(sq), 1.f / LN_C, eps));
}

__device__ __forceinline__ f32x4 ln_fwd_row(const f32x4 v, const f32x4 g, const f32x4 bt, float eps) {
#pragma clang fp contract(off)
  f32x4 d, y;
  float inv;
  ln_stats(v, eps, d, inv);
#pragma unroll
  for (int i = 0; i < 4; ++i) y[i] = fmaf(g[i], d[i] * inv, bt[i]);
  return y;
}

// One row (v: the input, gr: the incoming gradient, gm: gamma; this lane's 4 channels) -> this lane's 4 input
// gradients; adds the row's terms to dg (dgamma) and dbt (dbeta).
__device__ __forceinline__ f32x4 ln_bwd_row(const f32x4 v, const f32x4 gr, const f32x4 gm, float eps, f32x4& dg,
                                            f32x4& dbt) {
#pragma clang fp contract(off)
  f32x4 d, xh, ag, c, dx;
  float inv;
  ln_stats(v, eps, d, inv);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    xh[i] = d[i] * inv;
    ag[i] = gr[i] * gm[i];
  }
  // sum of a = g gamma: channel 0 enters rounded, the others as exact products
  const float sa = lss_wave_sum(fmaf(gr[3], gm[3], fmaf(gr[2], gm[2], fmaf(gr[1], gm[1], ag[0]))));
  const float m2 =
      lss_wave_sum(fmaf(ag[3], xh[3], fmaf(ag[2], xh[2], fmaf(ag[0], xh[0], ag[1] * xh[1])))) * (1.f / LN_C);
  // c = a - mean(a): channel 0 takes the rounded product and the unrounded mean, the others the reverse
  const float nm1 = sa * (-1.f / LN_C);
  c[0] = fmaf(sa, -1.f / LN_C, ag[0]);
#pragma unroll
  for (int i = 1; i < 4; ++i) c[i] = fmaf(gr[i], gm[i], nm1);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    dg[i] = fmaf(gr[i], xh[i], dg[i]);
    dbt[i] += gr[i];
    dx[i] = inv * fmaf(-xh[i], m2, c[i]);
  }
  return dx;
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
    lss_store4(y + row * LN_C + 4 * lane, ln_fwd_row(v, g, bt, eps));
  }
}

struct LnNoOut {};  // TA of the plain LayerNorm backward: no mask, no second output

// dx = LayerNorm backward of dy at x; with a second output, da = dx m
template <bool DROP, typename TX, typename TG, typename TD, typename TA>
__global__ __launch_bounds__(256) void layernorm_bwd_kernel(const TX* __restrict__ x, const TG* __restrict__ dy,
                                                            const float* __restrict__ gamma, long long rows,
                                                            long long rpg, float eps, unsigned int thr, float scale,
                                                            const unsigned long long* __restrict__ seed,
                                                            TD* __restrict__ dx, TA* __restrict__ da,
                                                            float* __restrict__ part) {
  __shared__ float red[4][2 * LN_C];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  LssPhiloxKey key = {0u, 0u, 0u, 0u};
  if (DROP) key = pw_key(seed);
  const long long r0 = (long long)blockIdx.x * rpg, r1 = min(rows, r0 + rpg);
  const f32x4 gm = *reinterpret_cast<const f32x4*>(gamma + 4 * lane);
  f32x4 dg = (f32x4){0.f, 0.f, 0.f, 0.f}, dbt = (f32x4){0.f, 0.f, 0.f, 0.f};
  for (long long row = r0 + wave; row < r1; row += 4) {  // whole waves: the shuffles of ln_bwd_row see all 64 lanes
    const f32x4 v = lss_load4<TX>(x + row * LN_C + 4 * lane);
    const f32x4 gr = lss_load4<TG>(dy + row * LN_C + 4 * lane);
    const f32x4 g = ln_bwd_row(v, gr, gm, eps, dg, dbt);
    lss_store4(dx + row * LN_C + 4 * lane, g);
    if constexpr (!std::is_same_v<TA, LnNoOut>) {
      const f32x4 m = pw_row_mask<DROP>(key, row, lane, thr, scale);
      lss_store4(da + row * LN_C + 4 * lane, DROP ? (f32x4){g[0] * m[0], g[1] * m[1], g[2] * m[2], g[3] * m[3]} : g);
    }
  }
  ln_bwd_write_partial(red, dg, dbt, part);
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

size_t ln_bwd_ws_bytes(long long rows) { return (size_t)ln_split(rows).G * 2 * LN_C * sizeof(float); }

// Both LayerNorm-backward entries.  fused: lss_add_dropout_ln_bwd (x = s and dx = ds are fp32, da is the second
// output); else lss_layernorm_bwd (da, thr and seed are unused).
int ln_bwd_launch(bool fused, const void* x, int x_dt, const void* dy, int dy_dt, const float* gamma, long long rows,
                  int C, float eps, int thr, float scale, const long long* seed, void* workspace,
                  size_t workspace_bytes, void* dx, int dx_dt, void* da, int da_dt, float* dgamma, float* dbeta,
                  void* stream) {
  LSS_CHECK_PTR(x); LSS_CHECK_PTR(dy); LSS_CHECK_PTR(gamma); LSS_CHECK_PTR(workspace);
  LSS_CHECK_PTR(dx); LSS_CHECK_PTR(dgamma); LSS_CHECK_PTR(dbeta);
  if (fused) LSS_CHECK_PTR(da);
  if (fused ? !lss_add_dropout_ln_ok(rows, C) || !pw_thr_ok(thr) : !lss_layernorm_bwd_ok(rows, C)) return LSS_E_SHAPE;
  if (!pw_dt_ok(x_dt) || !pw_dt_ok(dy_dt) || !pw_dt_ok(dx_dt) || !pw_dt_ok(da_dt)) return LSS_E_LAYOUT;
  if (!lss_aligned(seed, 8) || !lss_aligned(x, 16) || !lss_aligned(dy, 16) || !lss_aligned(gamma, 16) ||
      !lss_aligned(dx, 16) || !lss_aligned(da, 16) || !lss_aligned(workspace, 16) || !lss_aligned(dgamma, 4) ||
      !lss_aligned(dbeta, 4))
    return LSS_E_ALIGN;
  if (workspace_bytes < ln_bwd_ws_bytes(rows)) return LSS_E_WORKSPACE;
  const LnSplit sp = ln_split(rows);
  float* part = static_cast<float*>(workspace);
  hipStream_t st = lss_stream(stream);
  typedef unsigned short bf;
#define LSS_LNB(DROP, TX, TG, TD, TA)                                                                              \
  hipLaunchKernelGGL((layernorm_bwd_kernel<DROP, TX, TG, TD, TA>), dim3(sp.G), dim3(256), 0, st,                   \
                     static_cast<const TX*>(x), static_cast<const TG*>(dy), gamma, rows, sp.rpg, eps,              \
                     (unsigned int)thr, scale, reinterpret_cast<const unsigned long long*>(seed),                  \
                     static_cast<TD*>(dx), static_cast<TA*>(da), part)
  const int b2 = dy_dt == LSS_DT_BF16 ? 2 : 0;
  if (!fused) {
    switch ((x_dt == LSS_DT_BF16 ? 4 : 0) | b2 | (dx_dt == LSS_DT_BF16 ? 1 : 0)) {
      case 0: LSS_LNB(false, float, float, float, LnNoOut); break;
      case 1: LSS_LNB(false, float, float, bf, LnNoOut); break;
      case 2: LSS_LNB(false, float, bf, float, LnNoOut); break;
      case 3: LSS_LNB(false, float, bf, bf, LnNoOut); break;
      case 4: LSS_LNB(false, bf, float, float, LnNoOut); break;
      case 5: LSS_LNB(false, bf, float, bf, LnNoOut); break;
      case 6: LSS_LNB(false, bf, bf, float, LnNoOut); break;
      default: LSS_LNB(false, bf, bf, bf, LnNoOut); break;
    }
  } else {
    switch ((pw_drop(thr, seed) ? 4 : 0) | b2 | (da_dt == LSS_DT_BF16 ? 1 : 0)) {
      case 0: LSS_LNB(false, float, float, float, float); break;
      case 1: LSS_LNB(false, float, float, float, bf); break;
      case 2: LSS_LNB(false, float, bf, float, float); break;
      case 3: LSS_LNB(false, float, bf, float, bf); break;
      case 4: LSS_LNB(true, float, float, float, float); break;
      case 5: LSS_LNB(true, float, float, float, bf); break;
      case 6: LSS_LNB(true, float, bf, float, float); break;
      default: LSS_LNB(true, float, bf, float, bf); break;
    }
  }
#undef LSS_LNB
  const int rc = lss_launch_status();
  if (rc != 0) return rc;
  hipLaunchKernelGGL(layernorm_bwd_reduce_kernel, dim3(2), dim3(256), 0, st, part, sp.G, dgamma, dbeta);
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
  return lss_add_dropout_ln_ok(rows, LN_C) ? ln_bwd_ws_bytes(rows) : 0;
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
  return ln_bwd_launch(true, s, LSS_DT_F32, dy, dy_dt, gamma, rows, C, eps, thr, scale, seed, workspace,
                       workspace_bytes, ds, LSS_DT_F32, da, da_dt, dgamma, dbeta, stream);
}

extern "C" int lss_layernorm_bwd_ok(long long rows, int C) {
  return rows >= 1 && rows < (1LL << 31) && C == LN_C;
}

extern "C" size_t lss_layernorm_bwd_workspace_bytes(long long rows) {
  return lss_layernorm_bwd_ok(rows, LN_C) ? ln_bwd_ws_bytes(rows) : 0;
}

extern "C" int lss_layernorm_bwd(const void* x, int x_dt, const void* dy, int dy_dt, const float* gamma,
                                 long long rows, int C, float eps, void* workspace, size_t workspace_bytes, void* dx,
                                 int dx_dt, float* dgamma, float* dbeta, void* stream) {
  return ln_bwd_launch(false, x, x_dt, dy, dy_dt, gamma, rows, C, eps, 0, 1.f, nullptr, workspace, workspace_bytes,
                       dx, dx_dt, nullptr, LSS_DT_F32, dgamma, dbeta, stream);
}
