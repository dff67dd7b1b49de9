// The dropout mask of the transformer's pointwise training kernels (K12, transformer_pointwise.hip): THE definition.
// Masks are never stored: forward and backward recompute them from a 16-byte device-resident seed.
//
//   seed     int64[2] on the device = {key, stream}, read as unsigned.
//   counter  element e (linear index in the contiguous tensor) belongs to call q = e >> 3:
//            Philox4x32-10, key (lo32(key), hi32(key)), counter (q, 0, lo32(stream), hi32(stream)),
//            multipliers 0xD2511F53 / 0xCD9E8D57, Weyl constants 0x9E3779B9 / 0xBB67AE85.
//   piece    w = out[(e & 7) >> 1];  piece = (e & 1) ? w >> 16 : w & 0xffff.
//   keep     piece >= thr,  thr = round(p * 65536) in 1 .. 65535;  p_eff = thr / 65536,  scale = 1 / (1 - p_eff).
//
// One call serves 8 elements: its 32-bit multiplies are the expensive part of a streaming kernel (16-bit pieces halve
// them against one word per element).  tests/transformer_pointwise_ref.py restates all of this in numpy.
#pragma once
#include <stdint.h>

#ifndef __HIPCC__
#define LSS_PHILOX_FN static inline
#else
#define LSS_PHILOX_FN __host__ __device__ inline __attribute__((always_inline))
#endif

struct LssPhiloxKey {
  uint32_t k0, k1, s0, s1;  // key lo / hi, stream lo / hi
};

LSS_PHILOX_FN LssPhiloxKey lss_philox_key(unsigned long long key, unsigned long long stream) {
  return LssPhiloxKey{(uint32_t)key, (uint32_t)(key >> 32), (uint32_t)stream, (uint32_t)(stream >> 32)};
}

LSS_PHILOX_FN void lss_philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                      uint32_t out[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// the four words of call q
LSS_PHILOX_FN void lss_dropout_words(const LssPhiloxKey& k, uint32_t q, uint32_t out[4]) {
  lss_philox4x32_10(q, 0u, k.s0, k.s1, k.k0, k.k1, out);
}

// multiplier of element j (0 .. 7) of a call: 0 or scale
LSS_PHILOX_FN float lss_dropout_mul(const uint32_t w[4], int j, uint32_t thr, float scale) {
  const uint32_t word = w[j >> 1];
  const uint32_t piece = (j & 1) ? word >> 16 : word & 0xffffu;
  return piece >= thr ? scale : 0.f;
}
