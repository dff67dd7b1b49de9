// K14: the six-token tail of the vovnet model at inference (VoVNetBEVTransformer.forward behind `scene_tokens`):
// the pooled BEV token and camera_transformer -> bev_fusion -> unified_predictor on (B, N <= 8, 256) tokens.
//
// bev_pool_kernel: column sums of an NHWC map (B, R, 256), bf16 or fp32, into fp32 partials (B, P, 256).  Workgroup
//   (p, b) takes the contiguous rows [p R / P, (p + 1) R / P) of sample b; a thread owns one 16-byte piece of a row
//   (8 bf16 / 4 fp32 channels) and every 8th / 4th row of the range, POOL_U row loads in flight in POOL_U accumulator
//   sets; the sets, then the row groups (through LDS), are added in a fixed order.  No atomics, no fp32 copy of the map.
//
// camera_tail_kernel: one workgroup of 512 threads per sample, ONE launch.  Every parameter is read where the modules
//   keep it (fp32, row-major [out][in]) through the descriptor passed by value; tokens and activations stay in LDS.
//     1  x  = tok + cam_embed[ids]
//     2  x1 = LN(x + out_proj(softmax(q k^T / 8) v))            4 heads of 64, the maximum subtracted
//     3  x2 = LN(x1 + W2 gelu(W1 x1 + b1) + b2)                 erf GELU, hidden width 512
//     4  x3 = LN(x2 + c),  c = Wo (Wv bev + bv) + bo            cross-attention over ONE key: its softmax is exactly 1,
//                                                               so the output is the value row for every query and head
//                                                               and the q / k projections are never read
//     5  z0 = sum_n softmax(camera_weights)_n x3[n];  z1 = gelu(LN(Wa z0 + ba));  z2 = gelu(LN(Wb z1 + bb));
//        action = Wact z2 + b;  description = Wdesc z2 + b
//   Stages 1-3 are skipped when cam_embed is NULL, stage 4 when ca_in_w is NULL.  Stage 4 equals the library for finite
//   operands; a non-finite q . k makes the library's row NaN and this one not.
//   A linear layer: a wave owns output rows, its 64 lanes split K in 16-byte pieces (coalesced rows), the per-lane
//   partial sums of 8 tokens (or of 8 rows of a single vector) are folded by a transposing butterfly: fixed order, no
//   atomics, nothing depends on B - a sample's result is the same in any batch.  LayerNorm: biased variance, two-pass.
#include "lss_device.h"

namespace {

constexpr int CT_D = 256;       // token width
constexpr int CT_FF = 512;      // hidden width of the FFN and of the predictor
constexpr int CT_NMAX = 8;      // tokens per sample the LDS rows are laid out for
constexpr int CT_THREADS = 512;
constexpr int CT_WAVES = CT_THREADS / 64;
constexpr int CT_HEADS = 4, CT_HD = 64;
constexpr int POOL_U = 4;       // row loads a thread of bev_pool_kernel keeps in flight
constexpr int POOL_MAX_PARTS = 256;

// ---------------------------------------------------------------------------------------------------------------------
template <typename T>
struct PoolPiece;
template <>
struct PoolPiece<unsigned short> {
  static constexpr int N = 8;
  static __device__ __forceinline__ void add(const uint4& v, float (&acc)[8]) {
    float f[8];
    lss_unpack8(v, f);
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] += f[e];
  }
};
template <>
struct PoolPiece<float> {
  static constexpr int N = 4;
  static __device__ __forceinline__ void add(const uint4& v, float (&acc)[4]) {
    acc[0] += __builtin_bit_cast(float, v.x);
    acc[1] += __builtin_bit_cast(float, v.y);
    acc[2] += __builtin_bit_cast(float, v.z);
    acc[3] += __builtin_bit_cast(float, v.w);
  }
};

template <typename T>
__global__ __launch_bounds__(256) void bev_pool_kernel(const T* __restrict__ map, long long R, int P,
                                                       float* __restrict__ partials) {
  constexpr int CPT = PoolPiece<T>::N;  // channels per thread: one 16-byte load
  constexpr int TPR = CT_D / CPT;       // threads per row
  constexpr int G = 256 / TPR;          // row groups of the workgroup
  __shared__ float part[G][CT_D];
  const int tid = threadIdx.x, p = blockIdx.x, b = blockIdx.y;
  const int g = tid / TPR, c0 = (tid % TPR) * CPT;
  const long long r0 = (long long)p * R / P, r1 = (long long)(p + 1) * R / P;
  const T* base = map + (size_t)b * (size_t)R * CT_D + c0;
  float acc[POOL_U][CPT];
#pragma unroll
  for (int u = 0; u < POOL_U; ++u)
#pragma unroll
    for (int e = 0; e < CPT; ++e) acc[u][e] = 0.f;
  long long r = r0 + g;
  for (; r + (POOL_U - 1) * G < r1; r += POOL_U * G) {
    uint4 v[POOL_U];
#pragma unroll
    for (int u = 0; u < POOL_U; ++u) v[u] = *reinterpret_cast<const uint4*>(base + (size_t)(r + u * G) * CT_D);
#pragma unroll
    for (int u = 0; u < POOL_U; ++u) PoolPiece<T>::add(v[u], acc[u]);
  }
  for (; r < r1; r += G) PoolPiece<T>::add(*reinterpret_cast<const uint4*>(base + (size_t)r * CT_D), acc[0]);
#pragma unroll
  for (int e = 0; e < CPT; ++e) part[g][c0 + e] = (acc[0][e] + acc[1][e]) + (acc[2][e] + acc[3][e]);
  __syncthreads();
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < G; ++k) s += part[k][tid];
  partials[((size_t)b * P + p) * CT_D + tid] = s;
}
static_assert(POOL_U == 4, "the accumulator sets are added as (0 + 1) + (2 + 3)");

// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float ct_gelu(float v) { return 0.5f * v * (1.f + erff(v * 0.70710678118654752f)); }

// Sum each of v[0..7] over the 64 lanes; lane l gets the total of v[(l >> 3) & 7].  Each step halves the values a lane
// carries by handing the other half to its partner: 10 exchanges instead of 48, the same fixed tree for every value.
__device__ __forceinline__ float ct_reduce8(const float (&v)[8], int lane) {
  const bool b5 = (lane & 32) != 0, b4 = (lane & 16) != 0, b3 = (lane & 8) != 0;
  float w[4], u[2];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float keep = b5 ? v[4 + i] : v[i], send = b5 ? v[i] : v[4 + i];
    w[i] = keep + __shfl_xor(send, 32, 64);
  }
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const float keep = b4 ? w[2 + i] : w[i], send = b4 ? w[i] : w[2 + i];
    u[i] = keep + __shfl_xor(send, 16, 64);
  }
  const float keep = b3 ? u[1] : u[0], send = b3 ? u[0] : u[1];
  float t = keep + __shfl_xor(send, 8, 64);
  t += __shfl_xor(t, 4, 64);
  t += __shfl_xor(t, 2, 64);
  t += __shfl_xor(t, 1, 64);
  return t;
}

// ys[n * ystride + o] = act(bias[o] + sum_k W[o][k] xs[n * xstride + k]) for the CT_NMAX token rows, o < O.
// A wave takes R rows per pass (R row loads in flight); the token rows live in registers for the whole call.
template <int K, bool GELU>
__device__ __forceinline__ void ct_linear8(const float* __restrict__ W, const float* __restrict__ bias, int O,
                                           const float* xs, int xstride, float* ys, int ystride) {
  constexpr int KV = K / 256;  // 16-byte pieces of a row per lane
  constexpr int R = 8 / KV;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  f32x4 x[CT_NMAX][KV];
#pragma unroll
  for (int n = 0; n < CT_NMAX; ++n)
#pragma unroll
    for (int q = 0; q < KV; ++q) x[n][q] = *reinterpret_cast<const f32x4*>(xs + n * xstride + q * 256 + lane * 4);
  for (int o0 = wave * R; o0 < O; o0 += CT_WAVES * R) {
    f32x4 w[R][KV];
    float bv[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int o = min(o0 + r, O - 1);
#pragma unroll
      for (int q = 0; q < KV; ++q) w[r][q] = *reinterpret_cast<const f32x4*>(W + (size_t)o * K + q * 256 + lane * 4);
      bv[r] = bias[o];
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      float acc[CT_NMAX];
#pragma unroll
      for (int n = 0; n < CT_NMAX; ++n) {
        acc[n] = 0.f;
#pragma unroll
        for (int q = 0; q < KV; ++q)
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[n] = fmaf(w[r][q][e], x[n][q][e], acc[n]);
      }
      float t = ct_reduce8(acc, lane) + bv[r];
      if (GELU) t = ct_gelu(t);
      if (o0 + r < O && (lane & 7) == 0) ys[(lane >> 3) * ystride + o0 + r] = t;
    }
  }
}

// ys[o] = bias[o] + sum_k W[o][k] xs[k], o < O, for ONE vector: a wave takes R rows per pass, 8 at a time through the
// same butterfly.
template <int K>
__device__ __forceinline__ void ct_linear1(const float* __restrict__ W, const float* __restrict__ bias, int O,
                                           const float* xs, float* ys) {
  constexpr int KV = K / 256;
  constexpr int R = 16 / KV;  // rows per pass
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  f32x4 x[KV];
#pragma unroll
  for (int q = 0; q < KV; ++q) x[q] = *reinterpret_cast<const f32x4*>(xs + q * 256 + lane * 4);
  for (int o0 = wave * R; o0 < O; o0 += CT_WAVES * R) {
    f32x4 w[R][KV];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int q = 0; q < KV; ++q)
        w[r][q] = *reinterpret_cast<const f32x4*>(W + (size_t)min(o0 + r, O - 1) * K + q * 256 + lane * 4);
#pragma unroll
    for (int r0 = 0; r0 < R; r0 += 8) {
      float acc[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        acc[j] = 0.f;
#pragma unroll
        for (int q = 0; q < KV; ++q)
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[j] = fmaf(w[r0 + j][q][e], x[q][e], acc[j]);
      }
      const float t = ct_reduce8(acc, lane);
      const int o = o0 + r0 + (lane >> 3);
      if (o < O && (lane & 7) == 0) ys[o] = t + bias[o];
    }
  }
}

// out[c] = act(gamma[c] (v[c] - mean) / sqrt(var + eps) + beta[c]), v = x + add, over C channels by ONE wave.
// Two passes: the mean, then the centred squares (biased variance).  out may be x.
template <int C, bool GELU>
__device__ __forceinline__ void ct_layernorm(const float* x, const float* add, const float* __restrict__ gamma,
                                             const float* __restrict__ beta, float eps, float* out) {
  constexpr int E = C / 64;
  const int lane = threadIdx.x & 63;
  float v[E], s = 0.f;
#pragma unroll
  for (int e = 0; e < E; ++e) {
    v[e] = x[e * 64 + lane] + (add ? add[e * 64 + lane] : 0.f);
    s += v[e];
  }
  const float mean = lss_wave_sum(s) * (1.f / C);
  float q = 0.f;
#pragma unroll
  for (int e = 0; e < E; ++e) {
    v[e] -= mean;
    q = fmaf(v[e], v[e], q);
  }
  const float rstd = 1.f / sqrtf(lss_wave_sum(q) * (1.f / C) + eps);
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const float y = fmaf(v[e] * rstd, gamma[e * 64 + lane], beta[e * 64 + lane]);
    out[e * 64 + lane] = GELU ? ct_gelu(y) : y;
  }
}

__global__ __launch_bounds__(CT_THREADS) void camera_tail_kernel(const lss_camera_tail_desc_t a) {
  __shared__ __attribute__((aligned(16))) float X[CT_NMAX * CT_D];        // the tokens
  __shared__ __attribute__((aligned(16))) float BIG[CT_NMAX * 3 * CT_D];  // q | k | v, then the hidden rows
  __shared__ __attribute__((aligned(16))) float T[CT_NMAX * CT_D];        // attention output, FFN output
  __shared__ float S[CT_HEADS * CT_NMAX * CT_NMAX];                       // scores -> probabilities
  __shared__ __attribute__((aligned(16))) float V0[CT_FF], V1[CT_FF];     // the single-vector stages ping-pong
  const int tid = threadIdx.x, wave = tid >> 6, b = blockIdx.x, N = a.N;

  // 1: tokens (+ camera embedding); rows N .. 7 are zero and never leave LDS
  for (int i = tid; i < CT_NMAX * CT_D; i += CT_THREADS) {
    const int n = i >> 8, c = i & 255;
    float v = 0.f;
    if (n < N) {
      v = a.tokens[((size_t)b * N + n) * CT_D + c];
      if (a.cam_embed) {
        long long id = a.ids ? a.ids[(size_t)b * N + n] : n;
        id = id < 0 ? 0 : (id >= a.n_embed ? a.n_embed - 1 : id);  // a bad id never reads outside the table
        v += a.cam_embed[(size_t)id * CT_D + c];
      }
    }
    X[i] = v;
  }
  __syncthreads();

  if (a.cam_embed) {
    // 2: self-attention
    ct_linear8<CT_D, false>(a.sa_in_w, a.sa_in_b, 3 * CT_D, X, CT_D, BIG, 3 * CT_D);
    __syncthreads();
    if (tid < CT_HEADS * CT_NMAX * CT_NMAX) {
      const int h = tid >> 6, i = (tid >> 3) & 7, j = tid & 7;
      float s = 0.f;
      if (i < N && j < N) {
        const float* q = BIG + i * 3 * CT_D + h * CT_HD;
        const float* k = BIG + j * 3 * CT_D + CT_D + h * CT_HD;
#pragma unroll 8
        for (int d = 0; d < CT_HD; ++d) s = fmaf(q[d], k[d], s);
      }
      S[tid] = s * 0.125f;
    }
    __syncthreads();
    if (tid < CT_HEADS * CT_NMAX && (tid & 7) < N) {
      float* row = S + tid * CT_NMAX;  // (h, i)
      float m = row[0];
      for (int j = 1; j < N; ++j) m = fmaxf(m, row[j]);
      float e[CT_NMAX], sum = 0.f;
#pragma unroll
      for (int j = 0; j < CT_NMAX; ++j) {
        e[j] = j < N ? expf(row[j] - m) : 0.f;
        sum += e[j];
      }
      const float inv = 1.f / sum;
#pragma unroll
      for (int j = 0; j < CT_NMAX; ++j) row[j] = e[j] * inv;
    }
    __syncthreads();
    for (int i = tid; i < CT_NMAX * CT_D; i += CT_THREADS) {
      const int n = i >> 8, c = i & 255, h = c >> 6;
      float o = 0.f;
      if (n < N)
        for (int j = 0; j < N; ++j) o = fmaf(S[(h * CT_NMAX + n) * CT_NMAX + j], BIG[j * 3 * CT_D + 2 * CT_D + c], o);
      T[i] = o;
    }
    __syncthreads();
    ct_linear8<CT_D, false>(a.sa_out_w, a.sa_out_b, CT_D, T, CT_D, BIG, CT_D);
    __syncthreads();
    if (wave < N) ct_layernorm<CT_D, false>(X + wave * CT_D, BIG + wave * CT_D, a.norm1_w, a.norm1_b, a.eps_cam, X + wave * CT_D);
    __syncthreads();
    // 3: feed-forward
    ct_linear8<CT_D, true>(a.ffn1_w, a.ffn1_b, CT_FF, X, CT_D, BIG, CT_FF);
    __syncthreads();
    ct_linear8<CT_FF, false>(a.ffn2_w, a.ffn2_b, CT_D, BIG, CT_FF, T, CT_D);
    __syncthreads();
    if (wave < N) ct_layernorm<CT_D, false>(X + wave * CT_D, T + wave * CT_D, a.norm2_w, a.norm2_b, a.eps_cam, X + wave * CT_D);
    __syncthreads();
  }

  if (a.ca_in_w) {
    // 4: the BEV token = scale * the parts in order (two contiguous halves, eight chains each), then Wv, Wo
    {
      const int c = tid & 255, seg = tid >> 8, P = a.bev_parts, half = (P + 1) / 2;
      const int p0 = min(seg * half, P), p1 = min(p0 + half, P);
      const float* src = a.bev + (size_t)b * P * CT_D + c;
      float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      int p = p0;
      for (; p + 8 <= p1; p += 8) {
#pragma unroll
        for (int i = 0; i < 8; ++i) s[i] += src[(size_t)(p + i) * CT_D];
      }
#pragma unroll
      for (int i = 0; i < 7; ++i)
        if (p + i < p1) s[i] += src[(size_t)(p + i) * CT_D];
      T[seg * CT_D + c] = ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]));
    }
    __syncthreads();
    if (tid < CT_D) V0[tid] = a.bev_scale * (T[tid] + T[CT_D + tid]);
    __syncthreads();
    ct_linear1<CT_D>(a.ca_in_w + (size_t)2 * CT_D * CT_D, a.ca_in_b + 2 * CT_D, CT_D, V0, V1);  // the value rows
    __syncthreads();
    ct_linear1<CT_D>(a.ca_out_w, a.ca_out_b, CT_D, V1, V0);
    __syncthreads();
    if (wave < N) ct_layernorm<CT_D, false>(X + wave * CT_D, V0, a.norm3_w, a.norm3_b, a.eps_fuse, X + wave * CT_D);
    __syncthreads();
  }

  // 5: the predictor
  if (tid < CT_D) {
    float m = a.cam_w[0];
    for (int n = 1; n < N; ++n) m = fmaxf(m, a.cam_w[n]);
    float e[CT_NMAX], sum = 0.f;
#pragma unroll
    for (int n = 0; n < CT_NMAX; ++n) {
      e[n] = n < N ? expf(a.cam_w[n] - m) : 0.f;
      sum += e[n];
    }
    const float inv = 1.f / sum;
    float z = 0.f;
#pragma unroll
    for (int n = 0; n < CT_NMAX; ++n)
      if (n < N) z = fmaf(e[n] * inv, X[n * CT_D + tid], z);
    V0[tid] = z;
  }
  __syncthreads();
  ct_linear1<CT_D>(a.enc1_w, a.enc1_b, CT_FF, V0, V1);
  __syncthreads();
  if (wave == 0) ct_layernorm<CT_FF, true>(V1, nullptr, a.ln1_w, a.ln1_b, a.eps_pred, V1);
  __syncthreads();
  ct_linear1<CT_FF>(a.enc2_w, a.enc2_b, CT_D, V1, V0);
  __syncthreads();
  if (wave == 0) ct_layernorm<CT_D, true>(V0, nullptr, a.ln2_w, a.ln2_b, a.eps_pred, V0);
  __syncthreads();
  ct_linear1<CT_D>(a.act_w, a.act_b, a.n_action, V0, a.action + (size_t)b * a.n_action);
  ct_linear1<CT_D>(a.desc_w, a.desc_b, a.n_desc, V0, a.description + (size_t)b * a.n_desc);
}

int tail_shape_ok(int B, int N, int n_action, int n_desc) {
  if (B < 1 || B > 65535 || N < 1 || N > CT_NMAX) return LSS_E_SHAPE;
  if (n_action < 1 || n_action > 16 || n_desc < 1 || n_desc > 16) return LSS_E_SHAPE;
  return 1;
}

}  // namespace

extern "C" int lss_camera_tail_ok(int B, int N, int n_action, int n_desc) {
  return tail_shape_ok(B, N, n_action, n_desc);
}

extern "C" int lss_bev_pool_parts(int B, long long R) {
  if (B < 1 || B > 65535 || R < 1 || R > (1ll << 32)) return LSS_E_SHAPE;
  // a function of R alone, so a sample's sums do not depend on its batch: 64 rows or more per workgroup, and at most
  // POOL_MAX_PARTS parts, which fill the chip at B = 1 and keep the tail's sum over the parts short
  const long long p = R / 64;
  return (int)(p < 1 ? 1 : (p > POOL_MAX_PARTS ? POOL_MAX_PARTS : p));
}

extern "C" int lss_bev_pool_fwd(const void* map, int dt, int B, long long R, int C, int parts, float* partials,
                                void* stream) {
  LSS_CHECK_PTR(map);
  LSS_CHECK_PTR(partials);
  if (lss_bev_pool_parts(B, R) < 1 || C != CT_D || parts < 1 || parts > POOL_MAX_PARTS) return LSS_E_SHAPE;
  if (dt != 0 && dt != 1) return LSS_E_LAYOUT;
  if (!lss_aligned(map, 16) || !lss_aligned(partials, 4)) return LSS_E_ALIGN;
  const dim3 grid((unsigned)parts, (unsigned)B);
  if (dt == 1)
    hipLaunchKernelGGL(bev_pool_kernel<unsigned short>, grid, dim3(256), 0, lss_stream(stream),
                       static_cast<const unsigned short*>(map), R, parts, partials);
  else
    hipLaunchKernelGGL(bev_pool_kernel<float>, grid, dim3(256), 0, lss_stream(stream), static_cast<const float*>(map), R,
                       parts, partials);
  return lss_launch_status();
}

extern "C" int lss_camera_tail_fwd(const lss_camera_tail_desc_t* d, void* stream) {
  LSS_CHECK_PTR(d);
  // the predictor and the outputs are always there; a stage is given whole or not at all
  const void* always[] = {d->tokens, d->cam_w,  d->enc1_w, d->enc1_b, d->ln1_w,  d->ln1_b,  d->enc2_w,     d->enc2_b,
                          d->ln2_w,  d->ln2_b,  d->act_w,  d->act_b,  d->desc_w, d->desc_b, d->action,     d->description};
  const void* cam[] = {d->cam_embed, d->sa_in_w, d->sa_in_b, d->sa_out_w, d->sa_out_b, d->norm1_w, d->norm1_b,
                       d->ffn1_w,    d->ffn1_b,  d->ffn2_w,  d->ffn2_b,   d->norm2_w,  d->norm2_b};
  const void* fuse[] = {d->ca_in_w, d->ca_in_b, d->ca_out_w, d->ca_out_b, d->norm3_w, d->norm3_b, d->bev};
  for (const void* p : always) LSS_CHECK_PTR(p);
  int ncam = 0, nfuse = 0;
  for (const void* p : cam) ncam += p != nullptr;
  for (const void* p : fuse) nfuse += p != nullptr;
  if ((ncam != 0 && ncam != 13) || (nfuse != 0 && nfuse != 7)) return LSS_E_NULL;
  if (tail_shape_ok(d->B, d->N, d->n_action, d->n_desc) != 1) return LSS_E_SHAPE;
  if (ncam != 0 && (d->n_embed < 1 || (d->ids == nullptr && d->n_embed < d->N))) return LSS_E_SHAPE;
  if (nfuse != 0 && (d->bev_parts < 1 || d->bev_parts > POOL_MAX_PARTS)) return LSS_E_SHAPE;
  // 16-byte row loads: the tokens and the matrices; 4 bytes for every other fp32 operand, 8 for the ids
  const void* rows[] = {d->tokens, d->sa_in_w, d->sa_out_w, d->ffn1_w, d->ffn2_w, d->ca_in_w,
                        d->ca_out_w, d->enc1_w, d->enc2_w,  d->act_w,  d->desc_w};
  for (const void* p : rows)
    if (!lss_aligned(p, 16)) return LSS_E_ALIGN;
  for (const void* p : always)
    if (!lss_aligned(p, 4)) return LSS_E_ALIGN;
  for (const void* p : cam)
    if (!lss_aligned(p, 4)) return LSS_E_ALIGN;
  for (const void* p : fuse)
    if (!lss_aligned(p, 4)) return LSS_E_ALIGN;
  if (!lss_aligned(d->ids, 8)) return LSS_E_ALIGN;
  hipLaunchKernelGGL(camera_tail_kernel, dim3((unsigned)d->B), dim3(CT_THREADS), 0, lss_stream(stream), *d);
  return lss_launch_status();
}
