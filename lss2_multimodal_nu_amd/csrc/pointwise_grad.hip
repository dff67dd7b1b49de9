// Backward of a pointwise (1x1) conv  y[b, m, p] = sum_k w[m, k] x[b, k, p] + bias[m]  (ref: the ConvolutionBackward
// of src/model_vovnet_transformer.py:31,39,82,97 and src/modules.py:83), from the output gradient g:
//     dx[b, k, p] = sum_m w[m, k] g[b, m, p]
//     dw[m, k]    = sum_b sum_p g[b, m, p] x[b, k, p]
//     db[m]       = sum_b sum_p g[b, m, p]
// fp32 operands, fp32 accumulation on v_mfma_f32_32x32x2_f32 (exact fp32 FMA chains; bf16 x is widened exactly).
// g is channel-major (BN, ., HW) with an image stride: K7's (BN, D + C, HW) result is read where it lies, one channel
// range per call.  x / dx are fp32 NCHW (BN, K, HW) or NHWC rows (BN*HW, K) in fp32 / bf16.  Below, j = b HW + p is the
// flat pixel index ("column"), J = BN HW.
//
// Three kernels:
//   pw_dx_kernel      one wave = 32 columns x 128 input channels (four 32 x 32 accumulators), reduction over M two rows
//                     per MFMA.  Both operands come straight from global memory in the MFMA's own lane order (w rows
//                     and g rows are contiguous along the 32 lanes of a half-wave): no LDS.  The NHWC form swaps the
//                     A and B operands, which transposes the accumulator tile, so that both layouts store 128-B runs.
//   pw_dw_kernel      one workgroup = 64 input channels x all M (padded to 32s) x one slice of the columns; the
//                     reduction index is the contiguous one of g (and of NCHW x), so 32-column chunks go through LDS
//                     and are read back transposed (row pitch 33); the next chunk's global loads are in flight behind
//                     the MFMAs of the current one.  The slice's partial dw tile and (k block 0 only) partial db go
//                     to the workspace.
//   pw_finalize_kernel  dw / db = the slices' partials added in slice order.
// The summation order is a function of the shape alone: no float atomics, same bits run to run.  Padding rows and
// columns are zero-SELECTED (never multiplied by zero), so a non-finite g element reaches exactly the outputs the
// formulas above give it.
#include <algorithm>

#include "lss_common.h"

namespace {

constexpr int MAXM = 192;  // M padded to 32s: at most 6 row tiles
constexpr int PITCH = 33;

template <int LAYOUT>
__device__ __forceinline__ float load_x(const void* x, size_t i) {
  if (LAYOUT == LSS_PW_NHWC_BF16) return lss_bf2f(static_cast<const unsigned short*>(x)[i]);
  return static_cast<const float*>(x)[i];
}
template <int LAYOUT>
__device__ __forceinline__ void store_x(void* x, size_t i, float v) {
  if (LAYOUT == LSS_PW_NHWC_BF16) static_cast<unsigned short*>(x)[i] = lss_f2bf(v);
  else static_cast<float*>(x)[i] = v;
}

// accumulator row of register r in a 32 x 32 tile (column = lane & 31)
__device__ __forceinline__ int acc_row(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }

template <int LAYOUT>
__global__ __launch_bounds__(256) void pw_dx_kernel(const float* __restrict__ g, long long g_bstride,
                                                    const float* __restrict__ w, int J, int HW, int K, int M,
                                                    int nkc, int nwaves, void* __restrict__ dx) {
  const int lane = threadIdx.x & 63, l31 = lane & 31, half = lane >> 5;
  const int wid = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (wid >= nwaves) return;  // whole waves; the kernel has no barrier
  const int ct = wid / nkc, k0 = (wid % nkc) * 128;
  const int nt = min(4, (K - k0) >> 5);
  const int j = ct * 32 + l31;
  const bool jv = j < J;
  const int jc = jv ? j : J - 1;
  const int b = jc / HW, p = jc - b * HW;
  const float* gp = g + (size_t)b * g_bstride + p;
  const float* wp = w + k0 + l31;
  f32x16 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
#pragma unroll 4
  for (int m0 = 0; m0 < M; m0 += 2) {
    const int m = m0 + half;
    const bool mv = m < M;
    const int mc = mv ? m : M - 1;
    const float gl = gp[(size_t)mc * HW];
    const float gv = (mv && jv) ? gl : 0.f;
    float wv[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const float wl = wp[(size_t)mc * K + (t < nt ? 32 * t : 0)];
      wv[t] = mv ? wl : 0.f;
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      if (t < nt) {
        if (LAYOUT == LSS_PW_NCHW_F32) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(wv[t], gv, acc[t], 0, 0, 0);
        else acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(gv, wv[t], acc[t], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    if (t >= nt) continue;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = acc_row(r, half);
      if (LAYOUT == LSS_PW_NCHW_F32) {  // tile (row = k, column = j)
        const int k = k0 + 32 * t + row;
        if (jv) static_cast<float*>(dx)[((size_t)b * K + k) * HW + p] = acc[t][r];
      } else {                          // tile (row = j, column = k)
        const int jr = ct * 32 + row;
        if (jr < J) store_x<LAYOUT>(dx, (size_t)jr * K + k0 + 32 * t + l31, acc[t][r]);
      }
    }
  }
}

// columns [c0, c1) in 32-column chunks; workspace: part[s][M][K] partial dw, then dbp[s][MAXM] partial db
template <int LAYOUT>
__global__ __launch_bounds__(256) void pw_dw_kernel(const float* __restrict__ g, long long g_bstride,
                                                    const void* __restrict__ x, int J, int HW, int K, int M,
                                                    int cps, int nch, int want_dw, float* __restrict__ part,
                                                    float* __restrict__ dbp) {
  __shared__ float gs[MAXM * PITCH];
  __shared__ float xs[64 * PITCH];
  const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, half = lane >> 5, wave = tid >> 6;
  const int kt = wave & 1, mh = wave >> 1;  // wave: k tile kt of the block's 64 channels, row tiles mh, mh + 2, mh + 4
  const int k0 = blockIdx.x * 64, s = blockIdx.y;
  const int ntm = (M + 31) >> 5, mpad = ntm * 32;
  const int c0 = s * cps, c1 = min(c0 + cps, nch);
  const int jj = tid & 31, r0 = tid >> 5;  // staging: this thread's column of the chunk, first row
  constexpr bool NCHW = LAYOUT == LSS_PW_NCHW_F32;

  float gr[MAXM / 8], xr[8], xd[16];
  auto fetch = [&](int c) {
    const int j = c * 32 + jj;
    const bool jv = j < J;
    const int jc = jv ? j : J - 1;
    const int b = jc / HW, p = jc - b * HW;
    const float* gp = g + (size_t)b * g_bstride + p;
#pragma unroll
    for (int i = 0; i < MAXM / 8; ++i) {
      const int m = r0 + 8 * i;
      gr[i] = 0.f;
      if (m < mpad) {
        const float v = gp[(size_t)min(m, M - 1) * HW];
        gr[i] = (jv && m < M) ? v : 0.f;
      }
    }
    if (!want_dw) return;
    if (NCHW) {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float v = static_cast<const float*>(x)[((size_t)b * K + k0 + r0 + 8 * i) * HW + p];
        xr[i] = jv ? v : 0.f;
      }
    } else {  // rows are contiguous along k: the MFMA's B operand straight from global, one value per 2-column step
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int jx = c * 32 + 2 * i + half;
        const float v = load_x<LAYOUT>(x, (size_t)min(jx, J - 1) * K + k0 + 32 * kt + l31);
        xd[i] = jx < J ? v : 0.f;
      }
    }
  };

  f32x16 acc[3];
#pragma unroll
  for (int t = 0; t < 3; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  float dbacc = 0.f;

  if (c0 < c1) fetch(c0);
  for (int c = c0; c < c1; ++c) {
#pragma unroll
    for (int i = 0; i < MAXM / 8; ++i)
      if (r0 + 8 * i < mpad) gs[(r0 + 8 * i) * PITCH + jj] = gr[i];
    float xc[16];
    if (NCHW) {
      if (want_dw)
#pragma unroll
        for (int i = 0; i < 8; ++i) xs[(r0 + 8 * i) * PITCH + jj] = xr[i];
    } else {
#pragma unroll
      for (int i = 0; i < 16; ++i) xc[i] = xd[i];
    }
    __syncthreads();
    if (c + 1 < c1) fetch(c + 1);
    if (blockIdx.x == 0 && tid < mpad) {
#pragma unroll 8
      for (int q = 0; q < 32; ++q) dbacc += gs[tid * PITCH + q];
    }
    if (want_dw) {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int jr = 2 * i + half;
        const float bv = NCHW ? xs[(32 * kt + l31) * PITCH + jr] : xc[i];
#pragma unroll
        for (int t = 0; t < 3; ++t) {
          const int mt = mh + 2 * t;
          if (mt < ntm) {
            const float av = gs[(32 * mt + l31) * PITCH + jr];
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[t], 0, 0, 0);
          }
        }
      }
    }
    __syncthreads();
  }

  if (want_dw) {
    float* o = part + (size_t)s * M * K + k0 + 32 * kt + l31;
#pragma unroll
    for (int t = 0; t < 3; ++t) {
      const int mt = mh + 2 * t;
      if (mt >= ntm) continue;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = 32 * mt + acc_row(r, half);
        if (m < M) o[(size_t)m * K] = acc[t][r];
      }
    }
  }
  if (blockIdx.x == 0 && tid < mpad) dbp[(size_t)s * MAXM + tid] = dbacc;
}

__global__ __launch_bounds__(256) void pw_finalize_kernel(const float* __restrict__ part,
                                                          const float* __restrict__ dbp, int S, int MK, int M,
                                                          float* __restrict__ dw, float* __restrict__ db) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (dw != nullptr && i < MK) {
    float a = 0.f;
    for (int s = 0; s < S; ++s) a += part[(size_t)s * MK + i];
    dw[i] = a;
  }
  if (db != nullptr && i < M) {
    float a = 0.f;
    for (int s = 0; s < S; ++s) a += dbp[(size_t)s * MAXM + i];
    db[i] = a;
  }
}

struct Split {
  int nch, cps, S;
};

// column slices of the dw / db reduction: about one workgroup per CU over (K / 64 channel blocks) x S slices
inline Split split_of(int BN, int K, int HW) {
  Split sp;
  sp.nch = lss_cdiv((long long)BN * HW, 32);
  const int want = std::max(1, std::min(sp.nch, 256 / (K / 64)));
  sp.cps = lss_cdiv(sp.nch, want);
  sp.S = lss_cdiv(sp.nch, sp.cps);
  return sp;
}

}  // namespace

extern "C" int lss_pointwise_conv_bwd_ok(int BN, int K, int M, int HW) {
  if (BN <= 0 || K <= 0 || M <= 0 || HW <= 0) return 0;
  if (K % 64 != 0 || K > 1024 || M > MAXM) return 0;
  if (BN > 4096 || (long long)BN * HW > (1LL << 22)) return 0;
  return 1;
}

extern "C" size_t lss_pointwise_conv_bwd_workspace_bytes(int BN, int K, int M, int HW) {
  if (!lss_pointwise_conv_bwd_ok(BN, K, M, HW)) return 0;
  const Split sp = split_of(BN, K, HW);
  return (size_t)sp.S * ((size_t)M * K + MAXM) * sizeof(float);
}

extern "C" int lss_pointwise_conv_bwd(const float* g, int g_ch_off, long long g_bstride, const void* x, int x_layout,
                                      const float* w, int BN, int K, int M, int HW, void* workspace,
                                      size_t workspace_bytes, void* dx, float* dw, float* db, void* stream) {
  LSS_CHECK_PTR(g);
  if (dx != nullptr) LSS_CHECK_PTR(w);
  if (dw != nullptr) LSS_CHECK_PTR(x);
  if (x_layout != LSS_PW_NCHW_F32 && x_layout != LSS_PW_NHWC_F32 && x_layout != LSS_PW_NHWC_BF16) return LSS_E_LAYOUT;
  if (!lss_pointwise_conv_bwd_ok(BN, K, M, HW)) return LSS_E_SHAPE;
  if (g_ch_off < 0 || g_bstride < ((long long)g_ch_off + M) * HW) return LSS_E_SHAPE;
  const int esz = x_layout == LSS_PW_NHWC_BF16 ? 2 : 4;
  if ((reinterpret_cast<uintptr_t>(g) & 3) || (reinterpret_cast<uintptr_t>(w) & 3) ||
      (reinterpret_cast<uintptr_t>(x) & (esz - 1)) || (reinterpret_cast<uintptr_t>(dx) & (esz - 1)) ||
      (reinterpret_cast<uintptr_t>(dw) & 3) || (reinterpret_cast<uintptr_t>(db) & 3) ||
      (reinterpret_cast<uintptr_t>(workspace) & 3))
    return LSS_E_ALIGN;
  const bool reduce = dw != nullptr || db != nullptr;
  if (reduce) {
    LSS_CHECK_PTR(workspace);
    if (workspace_bytes < lss_pointwise_conv_bwd_workspace_bytes(BN, K, M, HW)) return LSS_E_WORKSPACE;
  }
  hipStream_t st = lss_stream(stream);
  const int J = BN * HW;
  const float* gc = g + (size_t)g_ch_off * HW;
  int rc = 0;
  if (dx != nullptr) {
    const int nkc = lss_cdiv(K, 128), nwaves = lss_cdiv(J, 32) * nkc;
    const dim3 grid(lss_cdiv(nwaves, 4)), block(256);
    if (x_layout == LSS_PW_NCHW_F32)
      hipLaunchKernelGGL(pw_dx_kernel<LSS_PW_NCHW_F32>, grid, block, 0, st, gc, g_bstride, w, J, HW, K, M, nkc,
                         nwaves, dx);
    else if (x_layout == LSS_PW_NHWC_F32)
      hipLaunchKernelGGL(pw_dx_kernel<LSS_PW_NHWC_F32>, grid, block, 0, st, gc, g_bstride, w, J, HW, K, M, nkc,
                         nwaves, dx);
    else
      hipLaunchKernelGGL(pw_dx_kernel<LSS_PW_NHWC_BF16>, grid, block, 0, st, gc, g_bstride, w, J, HW, K, M, nkc,
                         nwaves, dx);
    if ((rc = lss_launch_status())) return rc;
  }
  if (reduce) {
    const Split sp = split_of(BN, K, HW);
    float* part = static_cast<float*>(workspace);
    float* dbp = part + (size_t)sp.S * M * K;
    const int want_dw = dw != nullptr;
    const dim3 grid(want_dw ? K / 64 : 1, sp.S), block(256);
    if (x_layout == LSS_PW_NCHW_F32)
      hipLaunchKernelGGL(pw_dw_kernel<LSS_PW_NCHW_F32>, grid, block, 0, st, gc, g_bstride, x, J, HW, K, M, sp.cps,
                         sp.nch, want_dw, part, dbp);
    else if (x_layout == LSS_PW_NHWC_F32)
      hipLaunchKernelGGL(pw_dw_kernel<LSS_PW_NHWC_F32>, grid, block, 0, st, gc, g_bstride, x, J, HW, K, M, sp.cps,
                         sp.nch, want_dw, part, dbp);
    else
      hipLaunchKernelGGL(pw_dw_kernel<LSS_PW_NHWC_BF16>, grid, block, 0, st, gc, g_bstride, x, J, HW, K, M, sp.cps,
                         sp.nch, want_dw, part, dbp);
    if ((rc = lss_launch_status())) return rc;
    const int n = std::max(want_dw ? M * K : 0, M);
    hipLaunchKernelGGL(pw_finalize_kernel, dim3(lss_cdiv(n, 256)), dim3(256), 0, st, part, dbp, sp.S, M * K, M, dw,
                       db);
    if ((rc = lss_launch_status())) return rc;
  }
  return 0;
}
