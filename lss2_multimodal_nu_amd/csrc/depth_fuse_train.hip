// Training-mode tail of MultiScaleDepthNet, forward and backward, fp32 throughout.
// replaces: src/model_vovnet_transformer.py:61-69 under model.train() - F.interpolate (bilinear, align_corners=False)
//           of the C4 logits, torch.cat, the fusion 1x1 conv, BatchNorm2d with batch statistics, ReLU - and the
//           autograd nodes of those five ops (the library's 1x1 convolution backward among them).
//
//   x[p] = [d3[p], up(d4)[p]]   (2 D values per pixel p; never stored)
//   z    = W x + b              (the conv bias stays in z: running_mean needs no correction)
//   u    = relu(gamma (z - mean) invstd + beta),  mean / biased var over the M = BN H W pixels
//   backward from du, g = du [u > 0], zh = (z - mean) invstd:
//     dbeta = sum g, dgamma = sum g zh, dz = gamma invstd (g - dbeta / M - zh dgamma / M),
//     dW = sum_p dz (x) x (x recomputed), d(d3) = (W^T dz)[:D], d(d4) = up^T (W^T dz)[D:]
//
// Work split: one wave per pixel, lane d owns depth bin d (D <= 64), as depth_fuse_softmax_kernel; a workgroup walks
// a contiguous run of pixels, its four waves side by side.  Every sum over pixels is taken per wave or per
// workgroup, written as a partial, and added up in a fixed order by the NEXT kernel (bn_train.hip's pattern): no
// atomics, no hand-off inside a kernel, bit-reproducible.  Everything summed is taken about pixel 0: z = p + W (x - x0)
// with p = W x0 + b, the statistics from z - p, dW from dz (x) (x - x0) - so a channel whose mean dwarfs its spread
// keeps its variance, and logits that share a large level cost dW no digits.  up^T is a gather: a coarse pixel walks the fine pixels
// that can name it and asks lss_bilinear_src, the forward's own coordinate function, for each.
// Forward: 3 launches (z + partials, finalize, normalise); backward: 4 (partials, finalize, dz + W^T dz + dW
// partials, dW finalize + gather).
#include "lss_device.h"

namespace {

constexpr int DFT_MAX_BLOCKS = 64;   // workgroups of the pixel-walking kernels (4 waves each)
constexpr int DFT_LANES = 64;        // channel slots of a partial (D <= 64)
constexpr int DFT_X = 128;           // input slots of the fusion conv per pixel (2 D <= 128), zero past 2 D

inline int dft_blocks(long long M) {
  long long b = (M + 31) / 32;
  return (int)(b < 1 ? 1 : (b > DFT_MAX_BLOCKS ? DFT_MAX_BLOCKS : b));
}

// workspace, in floats
struct DftWs {
  size_t part, small, gup, dwpart, total;
};
inline DftWs dft_ws(long long M, int D) {
  const size_t nblk = (size_t)dft_blocks(M);
  DftWs w;
  w.part = 0;                                            // [nblk][2][64]   per-workgroup channel sums
  w.small = w.part + nblk * 2 * DFT_LANES;               // [3][64]         pivot | mean(g), mean(g zh), gamma invstd
  w.gup = w.small + 3 * DFT_LANES;                       // [BN][D][H][W]   (W^T dz)[D:] on the fine grid
  w.dwpart = w.gup + (size_t)M * D;                      // [nblk * 4][128][64]  per-wave dW partials
  w.total = w.dwpart + nblk * 4 * DFT_X * DFT_LANES;
  return w;
}

// the fusion weights transposed into LDS: wt[k][n] = W[n][k], rows padded to D + 1
__device__ __forceinline__ void dft_load_wt(const float* __restrict__ w, int D, float* wt) {
  for (int e = threadIdx.x; e < D * 2 * D; e += 256) {
    const int n = e / (2 * D), k = e % (2 * D);
    wt[k * (D + 1) + n] = w[e];
  }
}

// x of pixel gp into this wave's LDS row, less this lane's share (ca, cb) of a per-input constant: x[d] = d3 - ca,
// x[D + d] = up(d4) - cb; slots past 2 D stay as the caller left them
__device__ __forceinline__ void dft_load_x(const float* __restrict__ d3, const float* __restrict__ d4, int D, int H,
                                           int W, int H4, int W4, float rh, float rw, long long gp, int lane,
                                           float ca, float cb, float* x) {
  const int HW = H * W;
  const int bn = (int)(gp / HW), pix = (int)(gp % HW);
  const int oh = pix / W, ow = pix % W;
  int h0, h1, w0, w1;
  float lh0, lh1, lw0, lw1;
  lss_bilinear_src(rh, oh, H4, h0, h1, lh0, lh1);
  lss_bilinear_src(rw, ow, W4, w0, w1, lw0, lw1);
  if (lane < D) {
    const float* c = d4 + ((size_t)bn * D + lane) * ((size_t)H4 * W4);
    const float up = lh0 * (lw0 * c[h0 * W4 + w0] + lw1 * c[h0 * W4 + w1]) +
                     lh1 * (lw0 * c[h1 * W4 + w0] + lw1 * c[h1 * W4 + w1]);
    x[lane] = d3[((size_t)bn * D + lane) * HW + pix] - ca;
    x[D + lane] = up - cb;
  }
}

// row `lane` of W x
__device__ __forceinline__ float dft_wx(const float* wt, const float* x, int D, int lane) {
  float a = 0.f;
  for (int k = 0; k < 2 * D; ++k) a = fmaf(wt[k * (D + 1) + lane], x[k], a);
  return a;
}

// the four waves' channel sums -> part[blk][0 | 1][64], added in wave order
__device__ __forceinline__ void dft_store_partials(float s1, float s2, float* red, float* __restrict__ part) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  red[(wave * 2) * DFT_LANES + lane] = s1;
  red[(wave * 2 + 1) * DFT_LANES + lane] = s2;
  __syncthreads();
  if (tid < 2 * DFT_LANES) {
    const int which = tid >> 6;
    float s = 0.f;
    for (int w = 0; w < 4; ++w) s += red[(w * 2 + which) * DFT_LANES + lane];
    part[((size_t)blockIdx.x * 2 + which) * DFT_LANES + lane] = s;
  }
}

// sum over the nblk partials of channel c by one wave: lane l takes blocks l, l + 64, ..., then a fixed xor tree
__device__ __forceinline__ void dft_sum_partials(const float* __restrict__ part, int nblk, int c, float& s1,
                                                 float& s2) {
  const int lane = threadIdx.x & 63;
  float a = 0.f, b = 0.f;
  for (int k = lane; k < nblk; k += 64) {
    a += part[((size_t)k * 2) * DFT_LANES + c];
    b += part[((size_t)k * 2 + 1) * DFT_LANES + c];
  }
  s1 = lss_wave_sum(a);
  s2 = lss_wave_sum(b);
}

// forward 1: z for every pixel, and per-workgroup sums of (z - p), (z - p)^2 about the pivot p = z of pixel 0
__global__ __launch_bounds__(256) void dft_fwd_z_kernel(const float* __restrict__ d3, const float* __restrict__ d4,
                                                        const float* __restrict__ w, const float* __restrict__ bias,
                                                        int D, int H, int W, int H4, int W4, float rh, float rw,
                                                        long long M, long long per, float* __restrict__ z,
                                                        float* __restrict__ part, float* __restrict__ pivot) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* wt = lds;                          // [2D][D + 1]
  float* vec = wt + 2 * D * (D + 1);        // [4 waves][2D]
  float* red = vec + 4 * 2 * D;             // [4 waves][2][64]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int HW = H * W;
  float* x = vec + wave * 2 * D;
  dft_load_wt(w, D, wt);
  dft_load_x(d3, d4, D, H, W, H4, W4, rh, rw, 0, lane, 0.f, 0.f, x);   // every wave: pixel 0, the same bits everywhere
  __syncthreads();
  // x0 = x of pixel 0 and p = W x0 + b: every other pixel is computed as z = p + W (x - x0), so what is summed - for z
  // and for the statistics - is of the size of the spread however large the logits' common level is
  const float xa0 = lane < D ? x[lane] : 0.f, xb0 = lane < D ? x[D + lane] : 0.f;
  const float piv = lane < D ? dft_wx(wt, x, D, lane) + bias[lane] : 0.f;
  if (blockIdx.x == 0 && wave == 0 && lane < D) pivot[lane] = piv;
  __syncthreads();
  const long long p0 = (long long)blockIdx.x * per, p1 = p0 + per < M ? p0 + per : M;
  float s1 = 0.f, s2 = 0.f;
  for (long long base = p0; base < p1; base += 4) {   // uniform trip count over the workgroup
    const long long gp = base + wave;
    const bool live = gp < p1;
    dft_load_x(d3, d4, D, H, W, H4, W4, rh, rw, live ? gp : p0, lane, xa0, xb0, x);
    __syncthreads();
    if (live && lane < D) {
      const float d = dft_wx(wt, x, D, lane);   // z - p
      z[((size_t)(gp / HW) * D + lane) * HW + (size_t)(gp % HW)] = piv + d;
      s1 += d;
      s2 = fmaf(d, d, s2);
    }
    __syncthreads();
  }
  dft_store_partials(s1, s2, red, part);
}

// forward 2 (one workgroup): batch statistics and the running estimates
__global__ __launch_bounds__(256) void dft_fwd_finalize_kernel(const float* __restrict__ part, int nblk, long long M,
                                                               int D, const float* __restrict__ pivot, float eps,
                                                               float momentum, float* __restrict__ running_mean,
                                                               float* __restrict__ running_var,
                                                               float* __restrict__ save_mean,
                                                               float* __restrict__ save_invstd) {
  for (int c = threadIdx.x >> 6; c < D; c += 4) {   // one wave per channel
    float s1, s2;
    dft_sum_partials(part, nblk, c, s1, s2);
    if ((threadIdx.x & 63) != 0) continue;
    const float inv_m = 1.f / (float)M;
    const float dm = s1 * inv_m;
    const float mean = pivot[c] + dm;
    const float var = fmaxf(s2 * inv_m - dm * dm, 0.f);
    save_mean[c] = mean;
    save_invstd[c] = rsqrtf(var + eps);
    running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * mean;
    running_var[c] = (1.f - momentum) * running_var[c] + momentum * (var * ((float)M / (float)(M - 1)));
  }
}

// forward 3: u = relu(gamma (z - mean) invstd + beta) over the (BN, D, HW) tensor
__global__ __launch_bounds__(256) void dft_fwd_apply_kernel(const float* __restrict__ z,
                                                            const float* __restrict__ mean,
                                                            const float* __restrict__ invstd,
                                                            const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, long long n, int D, int HW,
                                                            float* __restrict__ u) {
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
    const int c = (int)((e / HW) % D);
    u[e] = fmaxf(fmaf((z[e] - mean[c]) * invstd[c], gamma[c], beta[c]), 0.f);
  }
}

// backward 1: per-workgroup sums of g and g zh
__global__ __launch_bounds__(256) void dft_bwd_sums_kernel(const float* __restrict__ du, const float* __restrict__ u,
                                                           const float* __restrict__ z,
                                                           const float* __restrict__ mean,
                                                           const float* __restrict__ invstd, int D, int HW,
                                                           long long M, long long per, float* __restrict__ part) {
  __shared__ float red[4 * 2 * DFT_LANES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long p0 = (long long)blockIdx.x * per, p1 = p0 + per < M ? p0 + per : M;
  float s1 = 0.f, s2 = 0.f;
  if (lane < D) {
    const float mu = mean[lane], is = invstd[lane];
    for (long long gp = p0 + wave; gp < p1; gp += 4) {
      const size_t e = ((size_t)(gp / HW) * D + lane) * HW + (size_t)(gp % HW);
      const float g = u[e] > 0.f ? du[e] : 0.f;
      s1 += g;
      s2 = fmaf(g, (z[e] - mu) * is, s2);
    }
  }
  dft_store_partials(s1, s2, red, part);
}

// backward 2 (one workgroup): dbeta, dgamma and the coefficients of dz
__global__ __launch_bounds__(256) void dft_bwd_finalize_kernel(const float* __restrict__ part, int nblk, long long M,
                                                               int D, const float* __restrict__ gamma,
                                                               const float* __restrict__ invstd,
                                                               float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                               float* __restrict__ coef) {
  for (int c = threadIdx.x >> 6; c < D; c += 4) {
    float s1, s2;
    dft_sum_partials(part, nblk, c, s1, s2);
    if ((threadIdx.x & 63) != 0) continue;
    dbeta[c] = s1;
    dgamma[c] = s2;
    const float inv_m = 1.f / (float)M;
    coef[c] = s1 * inv_m;
    coef[DFT_LANES + c] = s2 * inv_m;
    coef[2 * DFT_LANES + c] = gamma[c] * invstd[c];
  }
}

// backward 3: dz per pixel (never stored), W^T dz -> d(d3) and the fine-grid gradient of up(d4), per-wave partials
// of dW = sum dz (x) (x - x0) with x recomputed
__global__ __launch_bounds__(256) void dft_bwd_dz_kernel(const float* __restrict__ du, const float* __restrict__ u,
                                                         const float* __restrict__ z, const float* __restrict__ d3,
                                                         const float* __restrict__ d4, const float* __restrict__ w,
                                                         const float* __restrict__ mean,
                                                         const float* __restrict__ invstd,
                                                         const float* __restrict__ coef, int D, int H, int W, int H4,
                                                         int W4, float rh, float rw, long long M, long long per,
                                                         float* __restrict__ dd3, float* __restrict__ gup,
                                                         float* __restrict__ dwpart) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* vec = lds;                          // [4 waves][128]  x, zero past 2 D
  float* dzv = vec + 4 * DFT_X;              // [4 waves][64]   dz, zero past D
  float* wt = dzv + 4 * DFT_LANES;           // [2D][D + 1]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int HW = H * W;
  float* x = vec + wave * DFT_X;
  float* dzw = dzv + wave * DFT_LANES;
  dft_load_wt(w, D, wt);
  x[lane] = 0.f;
  x[64 + lane] = 0.f;
  float mu = 0.f, is = 0.f, cg = 0.f, cgz = 0.f, gi = 0.f;
  if (lane < D) {
    mu = mean[lane];
    is = invstd[lane];
    cg = coef[lane];
    cgz = coef[DFT_LANES + lane];
    gi = coef[2 * DFT_LANES + lane];
  }
  float acc[DFT_X];
#pragma unroll
  for (int k = 0; k < DFT_X; ++k) acc[k] = 0.f;
  __syncthreads();
  // dW is summed as dz (x) (x - x0), x0 = x of pixel 0: sum_p dz is exactly zero per channel (the BatchNorm backward
  // removes the mean of its own output), so the dropped (sum dz) (x) x0 is zero - and with it goes the cancellation
  // noise that term carries in fp32 when the logits share a large level
  dft_load_x(d3, d4, D, H, W, H4, W4, rh, rw, 0, lane, 0.f, 0.f, x);
  __syncthreads();
  const float xa0 = lane < D ? x[lane] : 0.f, xb0 = lane < D ? x[D + lane] : 0.f;
  __syncthreads();
  const long long p0 = (long long)blockIdx.x * per, p1 = p0 + per < M ? p0 + per : M;
  for (long long base = p0; base < p1; base += 4) {   // uniform trip count over the workgroup
    const long long gp = base + wave;
    const bool live = gp < p1;
    const long long q = live ? gp : p0;
    const int bn = (int)(q / HW), pix = (int)(q % HW);
    dft_load_x(d3, d4, D, H, W, H4, W4, rh, rw, q, lane, xa0, xb0, x);
    float dz = 0.f;
    if (live && lane < D) {
      const size_t e = ((size_t)bn * D + lane) * HW + pix;
      const float g = u[e] > 0.f ? du[e] : 0.f;
      const float zh = (z[e] - mu) * is;
      dz = gi * (g - cg - zh * cgz);
    }
    dzw[lane] = dz;
    __syncthreads();
    // W^T dz: lane k takes inputs k and k + 64
    if (live) {
      for (int r = 0; r < 2; ++r) {
        const int k = lane + 64 * r;
        if (k < 2 * D) {
          float a = 0.f;
          for (int d = 0; d < D; ++d) a = fmaf(wt[k * (D + 1) + d], dzw[d], a);
          if (k < D) dd3[((size_t)bn * D + k) * HW + pix] = a;
          else gup[((size_t)bn * D + (k - D)) * HW + pix] = a;
        }
      }
    }
    // dW row `lane`: dz (x) x over all 128 slots (x is zero past 2 D, dz is zero on a dead pixel)
#pragma unroll
    for (int k4 = 0; k4 < DFT_X / 4; ++k4) {
      const f32x4 xv = *reinterpret_cast<const f32x4*>(x + 4 * k4);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[4 * k4 + j] = fmaf(dz, xv[j], acc[4 * k4 + j]);
    }
    __syncthreads();
  }
  float* out = dwpart + ((size_t)blockIdx.x * 4 + wave) * DFT_X * DFT_LANES;
#pragma unroll
  for (int k = 0; k < DFT_X; ++k)
    if (k < 2 * D) out[k * DFT_LANES + lane] = acc[k];
}

// backward 4: blocks [0, nfin) add the per-wave dW partials in wave order; the rest gather d(d4) = up^T gup
__global__ __launch_bounds__(256) void dft_bwd_tail_kernel(const float* __restrict__ dwpart, int nwave, int nfin,
                                                           const float* __restrict__ gup, int D, int H, int W, int H4,
                                                           int W4, float rh, float rw, long long n4,
                                                           float* __restrict__ dw, float* __restrict__ dd4) {
  if ((int)blockIdx.x < nfin) {
    const int e = blockIdx.x * 256 + threadIdx.x;   // k * 64 + d
    const int k = e >> 6, d = e & 63;
    if (k >= 2 * D || d >= D) return;
    float s = 0.f;
    for (int p = 0; p < nwave; ++p) s += dwpart[(size_t)p * DFT_X * DFT_LANES + e];
    dw[d * 2 * D + k] = s;
    return;
  }
  const long long idx = (long long)(blockIdx.x - nfin) * 256 + threadIdx.x;   // (bn, d, h4, w4)
  if (idx >= n4) return;
  const int w4 = (int)(idx % W4), h4 = (int)((idx / W4) % H4);
  const size_t img = (size_t)(idx / ((long long)H4 * W4));   // bn * D + d
  // a superset of the fine rows / columns whose taps can be h4 / w4: source coordinate in [h4 - 1, h4 + 1), one more
  // on either side for the rounding of this estimate; lss_bilinear_src decides
  const float fh0 = ((float)h4 - 0.5f) / rh - 0.5f, fh1 = ((float)h4 + 1.5f) / rh - 0.5f;
  const float fw0 = ((float)w4 - 0.5f) / rw - 0.5f, fw1 = ((float)w4 + 1.5f) / rw - 0.5f;
  const int oh_lo = (int)fminf(fmaxf(floorf(fh0) - 1.f, 0.f), (float)(H - 1));
  const int oh_hi = (int)fminf(fmaxf(ceilf(fh1) + 1.f, 0.f), (float)(H - 1));
  const int ow_lo = (int)fminf(fmaxf(floorf(fw0) - 1.f, 0.f), (float)(W - 1));
  const int ow_hi = (int)fminf(fmaxf(ceilf(fw1) + 1.f, 0.f), (float)(W - 1));
  const float* g = gup + img * ((size_t)H * W);
  float s = 0.f;
  for (int oh = oh_lo; oh <= oh_hi; ++oh) {
    int h0, h1;
    float lh0, lh1;
    lss_bilinear_src(rh, oh, H4, h0, h1, lh0, lh1);
    const float wh = (h0 == h4 ? lh0 : 0.f) + (h1 == h4 ? lh1 : 0.f);   // both taps when the upper one is clamped
    if (h0 != h4 && h1 != h4) continue;
    for (int ow = ow_lo; ow <= ow_hi; ++ow) {
      int w0, w1;
      float lw0, lw1;
      lss_bilinear_src(rw, ow, W4, w0, w1, lw0, lw1);
      if (w0 != w4 && w1 != w4) continue;
      const float ww = (w0 == w4 ? lw0 : 0.f) + (w1 == w4 ? lw1 : 0.f);
      s = fmaf(wh * ww, g[(size_t)oh * W + ow], s);
    }
  }
  dd4[idx] = s;
}

// every refusal, before any launch
inline int dft_check(int BN, int D, int H, int W, int H4, int W4, long long& M) {
  LSS_CHECK_POS(BN); LSS_CHECK_POS(D); LSS_CHECK_POS(H); LSS_CHECK_POS(W); LSS_CHECK_POS(H4); LSS_CHECK_POS(W4);
  if (D > 64) return LSS_E_SHAPE;
  M = (long long)BN * H * W;
  if (M < 2 || M >= (1LL << 31)) return LSS_E_SHAPE;              // a batch statistic needs two values
  if ((long long)BN * D * H4 * W4 >= (1LL << 31)) return LSS_E_SHAPE;
  return 0;
}

inline int dft_ew_grid(long long n) {
  const long long g = (n + 255) / 256;
  return (int)(g > 16384 ? 16384 : (g < 1 ? 1 : g));
}

}  // namespace

extern "C" size_t lss_depth_fuse_train_workspace_bytes(int BN, int D, int H, int W) {
  long long M;
  if (dft_check(BN, D, H, W, 1, 1, M) != 0) return 0;
  return dft_ws(M, D).total * sizeof(float);
}

extern "C" int lss_depth_fuse_train_fwd(const float* d3, const float* d4, const float* w_fusion, const float* bias,
                                        const float* gamma, const float* beta, float* running_mean,
                                        float* running_var, float momentum, float eps, int BN, int D, int H, int W,
                                        int H4, int W4, void* workspace, size_t workspace_bytes, float* z, float* u,
                                        float* save_mean, float* save_invstd, void* stream) {
  LSS_CHECK_PTR(d3); LSS_CHECK_PTR(d4); LSS_CHECK_PTR(w_fusion); LSS_CHECK_PTR(bias); LSS_CHECK_PTR(gamma);
  LSS_CHECK_PTR(beta); LSS_CHECK_PTR(running_mean); LSS_CHECK_PTR(running_var); LSS_CHECK_PTR(workspace);
  LSS_CHECK_PTR(z); LSS_CHECK_PTR(u); LSS_CHECK_PTR(save_mean); LSS_CHECK_PTR(save_invstd);
  long long M;
  const int rc = dft_check(BN, D, H, W, H4, W4, M);
  if (rc != 0) return rc;
  const DftWs ws = dft_ws(M, D);
  if (workspace_bytes < ws.total * sizeof(float)) return LSS_E_WORKSPACE;
  if (!lss_aligned(workspace, 16)) return LSS_E_ALIGN;
  float* base = static_cast<float*>(workspace);
  float* part = base + ws.part;
  float* pivot = base + ws.small;
  hipStream_t st = lss_stream(stream);
  const int nblk = dft_blocks(M);
  const long long per = (M + nblk - 1) / nblk;
  // ATen: scale = (float)in / out for align_corners=False with an explicit output size
  const float rh = (float)H4 / (float)H, rw = (float)W4 / (float)W;
  const size_t lds_bytes = ((size_t)2 * D * (D + 1) + 4 * 2 * D + 4 * 2 * DFT_LANES) * sizeof(float);
  hipLaunchKernelGGL(dft_fwd_z_kernel, dim3(nblk), dim3(256), lds_bytes, st, d3, d4, w_fusion, bias, D, H, W, H4, W4,
                     rh, rw, M, per, z, part, pivot);
  hipLaunchKernelGGL(dft_fwd_finalize_kernel, dim3(1), dim3(256), 0, st, part, nblk, M, D, pivot, eps, momentum,
                     running_mean, running_var, save_mean, save_invstd);
  const long long n = M * D;
  hipLaunchKernelGGL(dft_fwd_apply_kernel, dim3(dft_ew_grid(n)), dim3(256), 0, st, z, save_mean, save_invstd, gamma,
                     beta, n, D, H * W, u);
  return lss_launch_status();
}

extern "C" int lss_depth_fuse_train_bwd(const float* du, const float* u, const float* z, const float* d3,
                                        const float* d4, const float* w_fusion, const float* gamma,
                                        const float* save_mean, const float* save_invstd, int BN, int D, int H, int W,
                                        int H4, int W4, void* workspace, size_t workspace_bytes, float* dd3,
                                        float* dd4, float* dw, float* dgamma, float* dbeta, void* stream) {
  LSS_CHECK_PTR(du); LSS_CHECK_PTR(u); LSS_CHECK_PTR(z); LSS_CHECK_PTR(d3); LSS_CHECK_PTR(d4);
  LSS_CHECK_PTR(w_fusion); LSS_CHECK_PTR(gamma); LSS_CHECK_PTR(save_mean); LSS_CHECK_PTR(save_invstd);
  LSS_CHECK_PTR(workspace); LSS_CHECK_PTR(dd3); LSS_CHECK_PTR(dd4); LSS_CHECK_PTR(dw); LSS_CHECK_PTR(dgamma);
  LSS_CHECK_PTR(dbeta);
  long long M;
  const int rc = dft_check(BN, D, H, W, H4, W4, M);
  if (rc != 0) return rc;
  const DftWs ws = dft_ws(M, D);
  if (workspace_bytes < ws.total * sizeof(float)) return LSS_E_WORKSPACE;
  if (!lss_aligned(workspace, 16)) return LSS_E_ALIGN;
  float* base = static_cast<float*>(workspace);
  float* part = base + ws.part;
  float* coef = base + ws.small;
  float* gup = base + ws.gup;
  float* dwpart = base + ws.dwpart;
  hipStream_t st = lss_stream(stream);
  const int nblk = dft_blocks(M);
  const long long per = (M + nblk - 1) / nblk;
  const float rh = (float)H4 / (float)H, rw = (float)W4 / (float)W;
  hipLaunchKernelGGL(dft_bwd_sums_kernel, dim3(nblk), dim3(256), 0, st, du, u, z, save_mean, save_invstd, D, H * W, M,
                     per, part);
  hipLaunchKernelGGL(dft_bwd_finalize_kernel, dim3(1), dim3(256), 0, st, part, nblk, M, D, gamma, save_invstd, dgamma,
                     dbeta, coef);
  const size_t lds_bytes = ((size_t)4 * DFT_X + 4 * DFT_LANES + 2 * D * (D + 1)) * sizeof(float);
  hipLaunchKernelGGL(dft_bwd_dz_kernel, dim3(nblk), dim3(256), lds_bytes, st, du, u, z, d3, d4, w_fusion, save_mean,
                     save_invstd, coef, D, H, W, H4, W4, rh, rw, M, per, dd3, gup, dwpart);
  const int nfin = lss_cdiv(2 * D * DFT_LANES, 256);
  const long long n4 = (long long)BN * D * H4 * W4;
  hipLaunchKernelGGL(dft_bwd_tail_kernel, dim3(nfin + lss_cdiv(n4, 256)), dim3(256), 0, st, dwpart, nblk * 4, nfin,
                     gup, D, H, W, H4, W4, rh, rw, n4, dw, dd4);
  return lss_launch_status();
}
