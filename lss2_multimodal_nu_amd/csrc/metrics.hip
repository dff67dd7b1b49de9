// Validation metrics of the segmentation head in one pass (SURVEY.md L1 helpers).
// replaces: ConfusionMatrix.update (src/tools.py:541-551: mask, n*a + b, bincount, reshape, +=) together with
//           `preds.argmax(1)` and `loss_fn(preds, binimgs).item() * preds.shape[0]` of get_val_info
//           (src/tools.py:281-282) / get_val_info_new (:322).
// One read of the (B, C, HW) logits gives, per pixel, the first maximal class p (torch.argmax's rule: a NaN counts
// as the maximum and the first NaN wins) and the weighted NLL term; a pixel whose target t is outside [0, C) counts
// nowhere and carries loss weight 0.  Nothing is written per pixel and nothing is added atomically in global memory:
// every workgroup leaves ONE C x C block of u32 counts and two fp32 sums in the workspace, and a one-workgroup
// finalize adds the blocks into the caller's running int64 matrix and reduces the sums in a fixed order, so the
// counts are exact and the loss is bit-reproducible.
// Counting: with C <= 8 every thread keeps all C*C bins in registers (predicated increments: the background bin takes
// most pixels, and same-address LDS atomics would serialise); with C <= 16 the bins live in one LDS histogram per wave.
#include "lss_common.h"

namespace {

constexpr int SE_MAXC = 16;
constexpr int SE_BLOCKS = 128;  // 128 x 256 threads x 4 pixels = 131072 pixels per grid-stride round
constexpr int SE_THREADS = 256;

__device__ __forceinline__ unsigned se_wave_sum_u32(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += (unsigned)__shfl_xor((int)v, o, 64);
  return v;
}

// The C*C bins of one thread (REG) or of one wave (LDS histogram `hist[wave]`).
template <int CT, bool REG>
struct SegBins {
  unsigned c[REG ? CT * CT : 1];
  unsigned* wave_hist;

  __device__ __forceinline__ void init(unsigned (*hist)[CT * CT]) {
    const int tid = threadIdx.x;
    wave_hist = hist[tid >> 6];
    if (REG) {
#pragma unroll
      for (int b = 0; b < CT * CT; ++b) c[b] = 0u;
    } else {
      for (int e = tid; e < 4 * CT * CT; e += SE_THREADS) (&hist[0][0])[e] = 0u;
      __syncthreads();
    }
  }
  // bin < CT*CT whenever ok
  __device__ __forceinline__ void add(int bin, bool ok) {
    if (REG) {
#pragma unroll
      for (int b = 0; b < CT * CT; ++b) c[b] += (ok && bin == b) ? 1u : 0u;
    } else if (ok) {
      atomicAdd(&wave_hist[bin], 1u);  // LDS
    }
  }
  // hist[wave][b] = the wave's count of bin b; ends behind a barrier
  __device__ __forceinline__ void to_lds() {
    if (REG) {
      const int lane = threadIdx.x & 63;
#pragma unroll
      for (int b = 0; b < CT * CT; ++b) {
        const unsigned s = se_wave_sum_u32(c[b]);
        if (lane == 0) wave_hist[b] = s;
      }
    }
    __syncthreads();
  }
};

// partial layout in the workspace, nblk = gridDim.x: u32 counts [nblk][C*C], u32 invalid [nblk], fp32 sums [nblk][2]
__device__ __forceinline__ unsigned* se_part_invalid(unsigned* ws, int nblk, int CC) { return ws + (size_t)nblk * CC; }
__device__ __forceinline__ float* se_part_sums(unsigned* ws, int nblk, int CC) {
  return reinterpret_cast<float*>(ws + (size_t)nblk * (CC + 1));
}

template <int CT>
__device__ __forceinline__ void se_store_block(unsigned (*hist)[CT * CT], int CC, unsigned inv, float s_loss, float s_w,
                                               bool want_loss, unsigned* ws) {
  __shared__ float fred[2][4];
  __shared__ unsigned ired[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  inv = se_wave_sum_u32(inv);
  s_loss = lss_wave_sum(s_loss);
  s_w = lss_wave_sum(s_w);
  if (lane == 0) {
    ired[wave] = inv;
    fred[0][wave] = s_loss;
    fred[1][wave] = s_w;
  }
  __syncthreads();
  const int nblk = gridDim.x;
  if (tid < CC) ws[(size_t)blockIdx.x * CC + tid] = (hist[0][tid] + hist[1][tid]) + (hist[2][tid] + hist[3][tid]);
  if (tid == 0) {
    se_part_invalid(ws, nblk, CC)[blockIdx.x] = (ired[0] + ired[1]) + (ired[2] + ired[3]);
    if (want_loss) {
      float* fp = se_part_sums(ws, nblk, CC) + 2 * blockIdx.x;
      fp[0] = (fred[0][0] + fred[0][1]) + (fred[0][2] + fred[0][3]);
      fp[1] = (fred[1][0] + fred[1][1]) + (fred[1][2] + fred[1][3]);
    }
  }
}

// One pixel: v[0..C) its logits, t its target.
template <int CT, bool REG>
__device__ __forceinline__ void se_pixel(const float (&v)[CT], long long t, int C, const float (&wc)[CT], bool want_loss,
                                         SegBins<CT, REG>& bins, float& s_loss, float& s_w) {
  int best = 0;
  float bv = v[0], mx = v[0];
#pragma unroll
  for (int c = 1; c < CT; ++c)
    if (c < C) {
      if (!(bv != bv) && (v[c] > bv || v[c] != v[c])) {
        best = c;
        bv = v[c];
      }
      mx = fmaxf(mx, v[c]);
    }
  const bool ok = t >= 0 && t < C;
  bins.add(ok ? (int)t * C + best : -1, ok);
  if (want_loss) {
    float se = 0.f, xt = 0.f, wt = 0.f;
#pragma unroll
    for (int c = 0; c < CT; ++c)
      if (c < C) {
        se += expf(v[c] - mx);
        if (ok && c == (int)t) {
          xt = v[c];
          wt = wc[c];
        }
      }
    // log(sum) - (x_t - max): no quotient that underflows, and no cancellation against a large max (loss.hip)
    s_loss += ok ? wt * (logf(se) - (xt - mx)) : 0.f;
    s_w += wt;
  }
}

// VEC: HW % 4 == 0 and the pointers allow it - a thread takes 4 consecutive pixels of one image: per class one 16-byte
// (fp32) or 8-byte (bf16) load, and two 16-byte loads of targets.
template <int CT, bool BF16, bool VEC>
__global__ __launch_bounds__(SE_THREADS) void seg_eval_kernel(const void* __restrict__ xv,
                                                              const long long* __restrict__ tgt,
                                                              const float* __restrict__ w, int C, long long HW,
                                                              long long n, unsigned* __restrict__ ws) {
  constexpr bool REG = CT <= 8;
  __shared__ unsigned hist[4][CT * CT];
  SegBins<CT, REG> bins;
  bins.init(hist);
  const bool want_loss = w != nullptr;
  float wc[CT];
#pragma unroll
  for (int c = 0; c < CT; ++c) wc[c] = (want_loss && c < C) ? w[c] : 0.f;
  float s_loss = 0.f, s_w = 0.f;
  const long long first = (long long)blockIdx.x * SE_THREADS + threadIdx.x, stride = (long long)gridDim.x * SE_THREADS;
  if (VEC) {
    for (long long q = first; q < n / 4; q += stride) {
      const long long i = 4 * q, b = i / HW, p = i - b * HW;
      const size_t base = (size_t)b * C * HW + p;
      float v[4][CT];
#pragma unroll
      for (int c = 0; c < CT; ++c)
        if (c < C) {
          if (BF16) {
            const uint2 r = *reinterpret_cast<const uint2*>(static_cast<const unsigned short*>(xv) + base + (size_t)c * HW);
            v[0][c] = lss_bf2f((unsigned short)(r.x & 0xffff));
            v[1][c] = lss_bf2f((unsigned short)(r.x >> 16));
            v[2][c] = lss_bf2f((unsigned short)(r.y & 0xffff));
            v[3][c] = lss_bf2f((unsigned short)(r.y >> 16));
          } else {
            const float4 r = *reinterpret_cast<const float4*>(static_cast<const float*>(xv) + base + (size_t)c * HW);
            v[0][c] = r.x; v[1][c] = r.y; v[2][c] = r.z; v[3][c] = r.w;
          }
        }
      const longlong2 t01 = *reinterpret_cast<const longlong2*>(tgt + i);
      const longlong2 t23 = *reinterpret_cast<const longlong2*>(tgt + i + 2);
      se_pixel<CT, REG>(v[0], t01.x, C, wc, want_loss, bins, s_loss, s_w);
      se_pixel<CT, REG>(v[1], t01.y, C, wc, want_loss, bins, s_loss, s_w);
      se_pixel<CT, REG>(v[2], t23.x, C, wc, want_loss, bins, s_loss, s_w);
      se_pixel<CT, REG>(v[3], t23.y, C, wc, want_loss, bins, s_loss, s_w);
    }
  } else {
    for (long long i = first; i < n; i += stride) {
      const long long b = i / HW, p = i - b * HW;
      const size_t base = (size_t)b * C * HW + p;
      float v[CT];
#pragma unroll
      for (int c = 0; c < CT; ++c)
        if (c < C)
          v[c] = BF16 ? lss_bf2f(static_cast<const unsigned short*>(xv)[base + (size_t)c * HW])
                      : static_cast<const float*>(xv)[base + (size_t)c * HW];
      se_pixel<CT, REG>(v, tgt[i], C, wc, want_loss, bins, s_loss, s_w);
    }
  }
  bins.to_lds();
  se_store_block<CT>(hist, C * C, 0u, s_loss, s_w, want_loss, ws);
}

// Label mode: the prediction comes from an int64 label tensor.  A prediction outside [0, C) on a counted target goes
// to the `invalid` count, not into the matrix.
template <int CT>
__global__ __launch_bounds__(SE_THREADS) void seg_eval_labels_kernel(const long long* __restrict__ pred,
                                                                     const long long* __restrict__ tgt, int C,
                                                                     long long n, unsigned* __restrict__ ws) {
  constexpr bool REG = CT <= 8;
  __shared__ unsigned hist[4][CT * CT];
  SegBins<CT, REG> bins;
  bins.init(hist);
  unsigned inv = 0u;
  for (long long i = (long long)blockIdx.x * SE_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * SE_THREADS) {
    const long long t = tgt[i], p = pred[i];
    const bool ok = t >= 0 && t < C, pok = p >= 0 && p < C;
    bins.add((ok && pok) ? (int)t * C + (int)p : -1, ok && pok);
    inv += (ok && !pok) ? 1u : 0u;
  }
  bins.to_lds();
  se_store_block<CT>(hist, C * C, inv, 0.f, 0.f, false, ws);
}

// One workgroup.  confmat[e] += sum over the workgroups' blocks (thread e); wave 0 then sums the invalid counts and the
// float partials: lane i takes partials i, i + 64, ... in order, then a fixed shuffle tree.  batch_loss = a / b (NaN
// when every target was ignored, as torch's); loss_acc += (double)batch_loss * B, the reference's
// `total_loss += loss.item() * preds.shape[0]` without the host round trip.
__global__ __launch_bounds__(SE_THREADS) void seg_eval_finalize_kernel(const unsigned* __restrict__ ws, int nblk, int CC,
                                                                       int B, bool want_loss,
                                                                       long long* __restrict__ confmat,
                                                                       long long* __restrict__ invalid,
                                                                       float* __restrict__ batch_loss,
                                                                       double* __restrict__ loss_acc) {
  const int tid = threadIdx.x;
  if (tid < CC) {
    long long s = 0;
    for (int k = 0; k < nblk; ++k) s += (long long)ws[(size_t)k * CC + tid];
    confmat[tid] += s;
  }
  if (tid >= 64) return;
  const unsigned* ip = ws + (size_t)nblk * CC;
  const float* fp = reinterpret_cast<const float*>(ws + (size_t)nblk * (CC + 1));
  unsigned inv = 0u;  // < 2^31 in total (n < 2^31)
  float a = 0.f, b = 0.f;
  for (int k = tid; k < nblk; k += 64) {
    inv += ip[k];
    if (want_loss) {
      a += fp[2 * k];
      b += fp[2 * k + 1];
    }
  }
  inv = se_wave_sum_u32(inv);
  a = lss_wave_sum(a);
  b = lss_wave_sum(b);
  if (tid == 0) {
    if (invalid != nullptr) invalid[0] += (long long)inv;
    if (want_loss) {
      const float loss = a / b;
      batch_loss[0] = loss;
      if (loss_acc != nullptr) loss_acc[0] = loss_acc[0] + (double)loss * (double)B;
    }
  }
}

int se_grid(long long work_items) {
  const long long g = (work_items + SE_THREADS - 1) / SE_THREADS;
  return (int)(g > SE_BLOCKS ? SE_BLOCKS : g);
}

template <int CT>
void se_launch_logits(int dtype, bool vec, int grid, hipStream_t st, const void* x, const long long* t, const float* w,
                      int C, long long HW, long long n, unsigned* ws) {
  if (dtype == LSS_DT_BF16) {
    if (vec) hipLaunchKernelGGL((seg_eval_kernel<CT, true, true>), dim3(grid), dim3(SE_THREADS), 0, st, x, t, w, C, HW, n, ws);
    else hipLaunchKernelGGL((seg_eval_kernel<CT, true, false>), dim3(grid), dim3(SE_THREADS), 0, st, x, t, w, C, HW, n, ws);
  } else {
    if (vec) hipLaunchKernelGGL((seg_eval_kernel<CT, false, true>), dim3(grid), dim3(SE_THREADS), 0, st, x, t, w, C, HW, n, ws);
    else hipLaunchKernelGGL((seg_eval_kernel<CT, false, false>), dim3(grid), dim3(SE_THREADS), 0, st, x, t, w, C, HW, n, ws);
  }
}

}  // namespace

extern "C" size_t lss_seg_eval_workspace_bytes(int C) {
  if (C <= 0 || C > SE_MAXC) return 0;
  return (size_t)SE_BLOCKS * (C * C + 1 + 2) * 4;
}

extern "C" int lss_seg_eval_update(const void* logits, int dtype, const long long* target, const float* class_weight,
                                   int B, int C, long long HW, void* workspace, size_t workspace_bytes,
                                   long long* confmat, float* batch_loss, double* loss_acc, void* stream) {
  LSS_CHECK_PTR(logits); LSS_CHECK_PTR(target); LSS_CHECK_PTR(workspace); LSS_CHECK_PTR(confmat);
  if (class_weight != nullptr) LSS_CHECK_PTR(batch_loss);
  LSS_CHECK_POS(B); LSS_CHECK_POS(C);
  if (HW <= 0 || C > SE_MAXC || HW >= (1LL << 31) || (long long)B * HW >= (1LL << 31)) return LSS_E_SHAPE;
  if (dtype != LSS_DT_F32 && dtype != LSS_DT_BF16) return LSS_E_LAYOUT;
  const uintptr_t esz = dtype == LSS_DT_BF16 ? 2 : 4;
  if (!lss_aligned(logits, esz) || !lss_aligned(target, 8) || !lss_aligned(workspace, 4) || !lss_aligned(confmat, 8) ||
      !lss_aligned(class_weight, 4) || !lss_aligned(batch_loss, 4) || !lss_aligned(loss_acc, 8))
    return LSS_E_ALIGN;
  if (workspace_bytes < lss_seg_eval_workspace_bytes(C)) return LSS_E_WORKSPACE;
  const long long n = (long long)B * HW;
  const bool vec = HW % 4 == 0 && lss_aligned(logits, 4 * esz) && lss_aligned(target, 16);
  const int grid = se_grid(vec ? n / 4 : n);
  hipStream_t st = lss_stream(stream);
  unsigned* ws = static_cast<unsigned*>(workspace);
  if (C <= 4) se_launch_logits<4>(dtype, vec, grid, st, logits, target, class_weight, C, HW, n, ws);
  else if (C <= 8) se_launch_logits<8>(dtype, vec, grid, st, logits, target, class_weight, C, HW, n, ws);
  else se_launch_logits<16>(dtype, vec, grid, st, logits, target, class_weight, C, HW, n, ws);
  hipLaunchKernelGGL(seg_eval_finalize_kernel, dim3(1), dim3(SE_THREADS), 0, st, ws, grid, C * C, B,
                     class_weight != nullptr, confmat, (long long*)nullptr, batch_loss, loss_acc);
  return lss_launch_status();
}

extern "C" int lss_seg_eval_update_labels(const long long* pred, const long long* target, long long n, int C,
                                          void* workspace, size_t workspace_bytes, long long* confmat,
                                          long long* invalid, void* stream) {
  LSS_CHECK_PTR(pred); LSS_CHECK_PTR(target); LSS_CHECK_PTR(workspace); LSS_CHECK_PTR(confmat); LSS_CHECK_PTR(invalid);
  LSS_CHECK_POS(C);
  if (n <= 0 || C > SE_MAXC || n >= (1LL << 31)) return LSS_E_SHAPE;
  if (!lss_aligned(pred, 8) || !lss_aligned(target, 8) || !lss_aligned(workspace, 4) || !lss_aligned(confmat, 8) ||
      !lss_aligned(invalid, 8))
    return LSS_E_ALIGN;
  if (workspace_bytes < lss_seg_eval_workspace_bytes(C)) return LSS_E_WORKSPACE;
  const int grid = se_grid(n);
  hipStream_t st = lss_stream(stream);
  unsigned* ws = static_cast<unsigned*>(workspace);
  if (C <= 4) hipLaunchKernelGGL(seg_eval_labels_kernel<4>, dim3(grid), dim3(SE_THREADS), 0, st, pred, target, C, n, ws);
  else if (C <= 8) hipLaunchKernelGGL(seg_eval_labels_kernel<8>, dim3(grid), dim3(SE_THREADS), 0, st, pred, target, C, n, ws);
  else hipLaunchKernelGGL(seg_eval_labels_kernel<16>, dim3(grid), dim3(SE_THREADS), 0, st, pred, target, C, n, ws);
  hipLaunchKernelGGL(seg_eval_finalize_kernel, dim3(1), dim3(SE_THREADS), 0, st, ws, grid, C * C, 1, false, confmat,
                     invalid, (float*)nullptr, (double*)nullptr);
  return lss_launch_status();
}
