// Device primitives shared by the gfx950 kernels: one text each, so kernels that must agree bit for bit cannot drift.
// Everything is __device__ __forceinline__, keeps no state and needs no macro before inclusion.  Include at file scope
// (not inside a namespace).  A new kernel file takes its primitives from here ("Device primitives").
#pragma once
#include "lss_common.h"

typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(8))) short s16x8;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;  // __bf16 elements; lss_common.h's bf16x8 is 8 x short

// ---- LDS-DMA, counted waits, barriers

// One 16-B LDS-DMA piece per lane: global -> LDS with no register hop.  The destination is the WAVE's base, lane l
// lands at base + 16 l (lane-linear): any swizzle goes on the source address.
__device__ __forceinline__ void lss_glds16(const void* gsrc, void* lds_wave_base) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gsrc,
                                   (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}
// Wait until at most N of this wave's vector-memory operations (LDS-DMA pieces included) are outstanding: the younger
// N stay in flight.
template <int N>
__device__ __forceinline__ void lss_wait_vmcnt() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
__device__ __forceinline__ void lss_wait_lgkm0() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
// Workgroup barrier that orders LDS traffic only.  __syncthreads() also drains vmcnt(0), which would expose the
// latency of the prefetch loads that are meant to stay in flight across it (cdna_hip_programming.md section 5,
// "Pipelining across barriers"); what must have landed is waited for with a counted lss_wait_vmcnt in front.
__device__ __forceinline__ void lss_lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

// x of the lane a DPP control selects (quad_perm / row_mirror / row_half_mirror: all inside a row of 16)
template <int CTRL>
__device__ __forceinline__ float lss_dpp_f32(float x) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), CTRL, 0xf, 0xf, false));
}

// ---- bf16 pieces.  (conv_mfma.hip's blend_bf16x8 and conv_ring.hip's rk_pack_bf2 / rk_blend are deliberately
// different: the packed-f32 and the scalar-FMA, one-v_cvt_pk_bf16_f32 forms of the upsample blend.)

// 8 consecutive bf16 of a 16-byte piece <-> 8 x fp32
__device__ __forceinline__ void lss_unpack8(const uint4& v, float (&f)[8]) {
  const unsigned int u[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    f[2 * k] = lss_bf2f((unsigned short)(u[k] & 0xffff));
    f[2 * k + 1] = lss_bf2f((unsigned short)(u[k] >> 16));
  }
}
__device__ __forceinline__ uint4 lss_pack8(const float (&f)[8]) {
  uint4 o;
  o.x = lss_pack_bf2(f[0], f[1]); o.y = lss_pack_bf2(f[2], f[3]);
  o.z = lss_pack_bf2(f[4], f[5]); o.w = lss_pack_bf2(f[6], f[7]);
  return o;
}

// 4 consecutive channels of a float or bf16 row <-> f32x4 (one 16-B or 8-B access)
template <typename T>
__device__ __forceinline__ f32x4 lss_load4(const T* p);
template <>
__device__ __forceinline__ f32x4 lss_load4<float>(const float* p) {
  return *reinterpret_cast<const f32x4*>(p);
}
template <>
__device__ __forceinline__ f32x4 lss_load4<unsigned short>(const unsigned short* p) {
  const uint2 v = *reinterpret_cast<const uint2*>(p);
  return (f32x4){lss_bf2f((unsigned short)(v.x & 0xffff)), lss_bf2f((unsigned short)(v.x >> 16)),
                 lss_bf2f((unsigned short)(v.y & 0xffff)), lss_bf2f((unsigned short)(v.y >> 16))};
}
__device__ __forceinline__ void lss_store4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }
__device__ __forceinline__ void lss_store4(unsigned short* p, f32x4 v) {
  uint2 o;
  o.x = lss_pack_bf2(v[0], v[1]);
  o.y = lss_pack_bf2(v[2], v[3]);
  *reinterpret_cast<uint2*>(p) = o;
}

// ---- fixed-order sum of split partials (the second stages of linear_grad.hip and of the LayerNorm backward in
// transformer_pointwise.hip)

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

// ---- erf and GELU. The GEMM epilogue (linear_mfma.hip), the fused FFN (ffn_fused.hip) and the training forward and
// backward (transformer_pointwise.hip) all take the polynomial from here: the fp64 tests rely on their agreement.
// (conv_mfma.hip's conv_act keeps libm's erff: the fp32 parity path.)

// erf by Abramowitz & Stegun 7.1.26 (|error| <= 1.5e-7, far below a bf16 ulp): libm's erff costs ~40 VALU
// instructions per element, which on a 1024-wide GELU layer is as much time as the GEMM itself.  e = exp(-x^2) is
// handed back: with x = h / sqrt 2 it IS exp(-h^2 / 2), so the GELU backward's phi(h) costs no second exponential.
__device__ __forceinline__ float lss_erf_as(float x, float& e) {
  const float ax = fabsf(x);
  const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, ax, 1.f));  // v_rcp_f32 (1 ulp); __frcp_rn is a 12-instruction IEEE division
  float p = fmaf(1.061405429f, t, -1.453152027f);
  p = fmaf(p, t, 1.421413741f);
  p = fmaf(p, t, -0.284496736f);
  p = fmaf(p, t, 0.254829592f);
  e = __expf(-ax * ax);
  return copysignf(1.f - p * t * e, x);
}
__device__ __forceinline__ float lss_erf_as(float x) {
  float e;
  return lss_erf_as(x, e);
}
__device__ __forceinline__ float lss_gelu(float v) { return 0.5f * v * (1.f + lss_erf_as(v * 0.70710678118654752f)); }
// d gelu / dv = Phi(v) + v phi(v).  v = +-3e38: v^2 = inf, exp = 0, v phi = 0.
__device__ __forceinline__ float lss_gelu_grad(float v) {
  float e;
  const float erf = lss_erf_as(v * 0.70710678118654752f, e);
  return fmaf(v, e * 0.3989422804014327f, 0.5f * (1.f + erf));
}

// ---- MFMA operand by transposed LDS read (conv_wgrad.hip, linear_grad.hip): rows of 64 channels = 128 B per
// position (pixel or token) lie as they do in memory, and the K dimension of the product is the POSITION.

// XOR swizzle of a position's 32-B channel blocks: bit 1 | bit 3 << 1 of the position
__device__ __forceinline__ int lss_tr_swz(int pos) { return ((pos >> 1) & 1) | (((pos >> 3) & 1) << 1); }
// 4 positions x 16 channels, transposed: this lane's channel at the 4 positions
__device__ __forceinline__ s16x4 lss_tr16(const unsigned char* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)p);
}
// one v_mfma_f32_16x16x32_bf16 operand: this lane's channel at 4 + 4 positions
__device__ __forceinline__ bf16x8_t lss_tr_frag(const unsigned char* lo, const unsigned char* hi) {
  const s16x4 a = lss_tr16(lo), b = lss_tr16(hi);
  const s16x8 v = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
  return __builtin_bit_cast(bf16x8_t, v);
}
