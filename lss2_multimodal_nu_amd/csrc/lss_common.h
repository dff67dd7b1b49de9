// Shared helpers of the gfx950 kernels (device + host side of the C ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "../../include/lss_hip.h"

#define LSS_WAVE 64

#define LSS_CHECK_PTR(p) \
  do {                   \
    if ((p) == nullptr) return LSS_E_NULL; \
  } while (0)

#define LSS_CHECK_POS(v) \
  do {                   \
    if ((v) <= 0) return LSS_E_SHAPE; \
  } while (0)

// Status of the launch just enqueued.  hipGetLastError: a returned failure is also CLEARED, so that one failed LSS
// launch (bad configuration, LDS size) does not stay latched in the thread and get reported again by every later
// LSS entry - or by the host framework's next launch check, attributed to the wrong op.  The host
// framework reads its own launches' status right after each of them, so nothing of its is pending here.
static inline int lss_launch_status() {
  hipError_t e = hipGetLastError();
  return (e == hipSuccess || e == hipErrorNotReady) ? 0 : (int)e;  // NotReady: a pending event query, not a launch error
}

static inline hipStream_t lss_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

static inline int lss_cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }

// is p a multiple of a (a power of two)?
static inline bool lss_aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// Developer switches from the environment.  Each call reads the environment: a site that tests flip in-process calls
// these per launch, a site that may not change within a process keeps the result in a `static const`.
// A switch that is on by default: unset or non-zero.
static inline bool lss_env_on(const char* name) {
  const char* e = getenv(name);
  return e == nullptr || atoi(e) != 0;
}
// A switch that is off by default: set and non-zero.
static inline bool lss_env_set_on(const char* name) {
  const char* e = getenv(name);
  return e != nullptr && atoi(e) != 0;
}
// A device address in hex (the diagnostics' stamp / counter buffers), or null when unset.
static inline unsigned long long* lss_env_device_ptr(const char* name) {
  const char* e = getenv(name);
  return e ? reinterpret_cast<unsigned long long*>(strtoull(e, nullptr, 16)) : nullptr;
}

typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(8))) short bf16x8;
typedef __attribute__((ext_vector_type(4))) short bf16x4;

// fp32 -> bf16 round-to-nearest-even via the hardware cast (keeps NaN a NaN,
// MI355X_MICROARCH.md "Correctness boundaries").
__device__ __forceinline__ unsigned short lss_f2bf(float f) {
  __bf16 h = (__bf16)f;
  return __builtin_bit_cast(unsigned short, h);
}
__device__ __forceinline__ float lss_bf2f(unsigned short u) {
  return __builtin_bit_cast(float, ((unsigned int)u) << 16);
}
__device__ __forceinline__ unsigned int lss_pack_bf2(float lo, float hi) {
  return (unsigned int)lss_f2bf(lo) | ((unsigned int)lss_f2bf(hi) << 16);
}

// XCD-aware block order (cdna_hip_programming.md T1): workgroups are dealt round-robin to the 8 XCDs, so block `bid` of
// `nwg` takes list position t such that XCD k works on the k-th contiguous eighth of the list - neighbours in the list
// share ONE L2.  Bijective for any grid size.
__device__ __forceinline__ int lss_xcd_order(int bid, int nwg) {
  const int xcd = bid & 7, q8 = nwg >> 3, r8 = nwg & 7;
  return (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (bid >> 3);
}

// Source taps of output index `o` of a bilinear resize with align_corners=False, exactly as ATen's
// area_pixel_compute_source_index: r = (float)n_in / n_out, the coordinate clamped at 0, the upper tap clamped to the
// last input index.  The inference tail (depthnet.hip) and the training tail with its adjoint (depth_fuse_train.hip)
// all take their taps from here, so forward, recomputation and gather cannot disagree.
__device__ __forceinline__ void lss_bilinear_src(float r, int o, int n_in, int& i0, int& i1, float& l0, float& l1) {
  float s = r * ((float)o + 0.5f) - 0.5f;
  s = s < 0.f ? 0.f : s;
  i0 = (int)s;
  i1 = i0 + (i0 < n_in - 1 ? 1 : 0);
  l1 = s - (float)i0;
  l0 = 1.f - l1;
}

__device__ __forceinline__ float lss_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float lss_wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
