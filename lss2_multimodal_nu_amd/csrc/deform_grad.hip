// Backward of the deformable-attention sampling core (ref: src/transformer_modules.py:117-156: softmax over the
// points, sampling locations with clamp(0, 1), bilinear zero-padded grid_sample at align_corners=False, weighted sum).
// The forward is lss_deform_attn_pts_fwd (bev_transformer.hip).  Activations are fp32 token rows (B, H*W, 256),
// value in the same NHWC layout; offsets_logits (B*H*W, 192) = [offsets (head, point, xy) | logits (head, point)].
//
// Three kernels:
//   deform_grad_ol_kernel   d_offsets_logits, GATHER form: the forward's mapping (wave = 2 tokens, lane = 32 tok +
//                           4 head + sub, sub owning 8 channels of its head).  Per point the lane dots d_out with its 8
//                           channels of each of the 4 taps; the quad sums give g_p = d_out . sample_p and the two
//                           bilinear derivatives; the softmax backward is one more quad sum.  No atomics.
//   deform_absmax_kernel    per sample: the largest FINITE |d_out| (integer max of the magnitude bits), which fixes
//                           that sample's fixed-point scale.
//   deform_scatter_kernel   d_value, SCATTER form, summed in int64 fixed point (integer addition is associative, so
//                           the bits do not depend on the order the adds arrive in - no float atomics anywhere).  One
//                           workgroup per (16 x 16 token tile, head, 8-channel slice) of one sample accumulates into an
//                           LDS window of the tile plus a 9-pixel margin (34 x 34 cells x 8 channels x 8 B = 72 KiB,
//                           two workgroups per CU) with ds_add_u64; taps outside the window go to global int64 adds
//                           directly; the window's non-zero elements are then added to the sample's global int64 sums.
//   deform_convert_kernel   int64 sums -> fp32 d_value (flagged elements -> NaN).
// Fixed point: a (token, head) puts total weight <= 1 into its head's plane (softmax weights sum to 1, bilinear weights
// to <= 1), so one element's sum is at most N max|d_out| for N tokens.  With max|d_out| < 2^e the scale
// 2^(F - e), F = min(62 - ceil(log2 N), 50), cannot overflow 2^63 (nor can the per-add rounding, <= 1/2 step per add);
// the cap at 50 keeps each add's magnitude below 2^51, the range of the magic-number rounding (splat.hip).  Scales are
// per sample, so sample i's bits are independent of the rest of the batch.  A non-finite product (a non-finite d_out
// element, or a non-finite weight) is not added: its (cell, channel) bit is set in a flag word and the element comes
// out NaN - the scale ignores non-finite values, so every other element keeps its clean-run bits.
#include <algorithm>

#include "lss_common.h"

namespace {

constexpr int TC = 256;
constexpr double FX_MAGIC = 6755399441055744.0;          // 1.5 * 2^52
constexpr long long FX_MAGIC_BITS = 0x4338000000000000LL;  // its bit pattern

// one sampling point: top-left tap, bilinear weights, clamp masks - the forward's arithmetic (make_taps)
struct Pt {
  int x0, y0;
  float wx0, wx1, wy0, wy1;
  float mx, my;  // 1 where clamp(0, 1) passed the gradient (inclusive bounds, as torch.clamp's backward)
};

__device__ __forceinline__ Pt locate(float offx, float offy, float rx, float ry, int H, int W) {
  const float fH = (float)H;
  float lx = rx + offx / fH, ly = ry + offy / fH;
  Pt p;
  p.mx = (lx >= 0.f && lx <= 1.f) ? 1.f : 0.f;
  p.my = (ly >= 0.f && ly <= 1.f) ? 1.f : 0.f;
  lx = fminf(fmaxf(lx, 0.f), 1.f);
  ly = fminf(fmaxf(ly, 0.f), 1.f);
  const float gx = lx * 2.0f - 1.0f, gy = ly * 2.0f - 1.0f;
  const float px = ((gx + 1.f) * (float)W - 1.f) / 2.f;
  const float py = ((gy + 1.f) * (float)H - 1.f) / 2.f;
  const float x0f = floorf(px), y0f = floorf(py);
  p.x0 = (int)x0f;
  p.y0 = (int)y0f;
  p.wx1 = px - x0f;
  p.wx0 = (x0f + 1.f) - px;
  p.wy1 = py - y0f;
  p.wy0 = (y0f + 1.f) - py;
  return p;
}

__device__ __forceinline__ float dot8(const float* __restrict__ p, const float (&g)[8]) {
  const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
  return ((a[0] * g[0] + a[1] * g[1]) + (a[2] * g[2] + a[3] * g[3])) +
         ((b[0] * g[4] + b[1] * g[5]) + (b[2] * g[6] + b[3] * g[7]));
}

__device__ __forceinline__ float quad_sum(float v) {
  v += __shfl_xor(v, 1, 64);
  return v + __shfl_xor(v, 2, 64);
}

// d_offsets_logits.  lane (tok, head, sub) prepares points 2 sub, 2 sub + 1 of its (token, head) as the forward does;
// the taps of all 8 points are then visited by the 4 lanes of the quad (parameters broadcast by shuffle).
__global__ __launch_bounds__(256) void deform_grad_ol_kernel(const float* __restrict__ value,
                                                             const float* __restrict__ ol,
                                                             const float* __restrict__ ref_pts, long long ref_bstr,
                                                             const float* __restrict__ d_out, int B, int H, int W,
                                                             float* __restrict__ d_ol) {
  const int lane = threadIdx.x & 63, tok = lane >> 5, head = (lane >> 2) & 7, sub = lane & 3;
  const long long rows = (long long)B * H * W;
  const long long want = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * 2 + tok;
  const bool live = want < rows;
  const long long row = live ? want : rows - 1;  // a tail half-wave redoes the last token (and does not store)
  const long long HW = (long long)H * W;
  const int t = (int)(row % HW);
  const int b = (int)(row / HW);
  const float* r = ol + row * 192;
  const f32x4 off = *reinterpret_cast<const f32x4*>(r + 16 * head + 4 * sub);
  const float2 lg = *reinterpret_cast<const float2*>(r + 128 + 8 * head + 2 * sub);
  float mx = fmaxf(lg.x, lg.y);
  mx = fmaxf(mx, __shfl_xor(mx, 1, 64));
  mx = fmaxf(mx, __shfl_xor(mx, 2, 64));
  const float e0 = expf(lg.x - mx), e1 = expf(lg.y - mx);
  const float sum = quad_sum(e0 + e1);
  const float aw0 = e0 / sum, aw1 = e1 / sum;
  const float2 rp = *reinterpret_cast<const float2*>(ref_pts + (size_t)b * ref_bstr + 2 * (size_t)t);
  const Pt pa = locate(off[0], off[1], rp.x, rp.y, H, W);
  const Pt pb = locate(off[2], off[3], rp.x, rp.y, H, W);

  float g[8];
  {
    const float* go = d_out + row * TC + head * 32 + 8 * sub;
    const f32x4 u = *reinterpret_cast<const f32x4*>(go), v = *reinterpret_cast<const f32x4*>(go + 4);
    g[0] = u[0]; g[1] = u[1]; g[2] = u[2]; g[3] = u[3];
    g[4] = v[0]; g[5] = v[1]; g[6] = v[2]; g[7] = v[3];
  }
  const float* vb = value + (size_t)b * HW * TC + head * 32 + 8 * sub;
  // per point p = 2 q + half, summed over the quad (each lane holds 8 of the head's 32 channels):
  //   G  = d_out . sample_p                          (sample without the attention weight)
  //   PX = d_out . d sample_p / d px,  PY = ... / d py   (pixel coordinates; out-of-image taps are zeros)
  // lane sub keeps the values of its own two points (q == sub).  The loop stays rolled: 16 loads in flight per step.
  float ga = 0.f, gb = 0.f, xa = 0.f, xb = 0.f, ya = 0.f, yb = 0.f;
#pragma unroll 1
  for (int q = 0; q < 4; ++q) {
    const int src = (lane & ~3) | q;
    float G[2], PX[2], PY[2];
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const Pt& m = half ? pb : pa;
      const int x0 = __shfl(m.x0, src, 64), y0 = __shfl(m.y0, src, 64);
      const float wx0 = __shfl(m.wx0, src, 64), wx1 = __shfl(m.wx1, src, 64);
      const float wy0 = __shfl(m.wy0, src, 64), wy1 = __shfl(m.wy1, src, 64);
      const bool xin0 = x0 >= 0 && x0 < W, xin1 = x0 + 1 >= 0 && x0 + 1 < W;
      const bool yin0 = y0 >= 0 && y0 < H, yin1 = y0 + 1 >= 0 && y0 + 1 < H;
      const int cx0 = min(max(x0, 0), W - 1), cx1 = min(max(x0 + 1, 0), W - 1);
      const int cy0 = min(max(y0, 0), H - 1), cy1 = min(max(y0 + 1, 0), H - 1);
      const float t00 = dot8(vb + (size_t)(cy0 * W + cx0) * TC, g);
      const float t01 = dot8(vb + (size_t)(cy0 * W + cx1) * TC, g);
      const float t10 = dot8(vb + (size_t)(cy1 * W + cx0) * TC, g);
      const float t11 = dot8(vb + (size_t)(cy1 * W + cx1) * TC, g);
      const float d00 = (xin0 && yin0) ? t00 : 0.f, d01 = (xin1 && yin0) ? t01 : 0.f;
      const float d10 = (xin0 && yin1) ? t10 : 0.f, d11 = (xin1 && yin1) ? t11 : 0.f;
      G[half] = quad_sum(wy0 * (wx0 * d00 + wx1 * d01) + wy1 * (wx0 * d10 + wx1 * d11));
      PX[half] = quad_sum(wy0 * (d01 - d00) + wy1 * (d11 - d10));
      PY[half] = quad_sum(wx0 * (d10 - d00) + wx1 * (d11 - d01));
    }
    if (sub == q) {
      ga = G[0]; gb = G[1];
      xa = PX[0]; xb = PX[1];
      ya = PY[0]; yb = PY[1];
    }
  }
  // softmax backward over the 8 points: dlogit_p = aw_p (g_p - sum_q aw_q g_q)
  const float s = quad_sum(aw0 * ga + aw1 * gb);
  // chain to the offsets: px = lx W - 1/2, lx = ref + off / H  ->  d offx = (W / H) dL/dpx;  d offy = dL/dpy
  const float rWH = (float)W / (float)H;
  const f32x4 doff = (f32x4){pa.mx * (aw0 * xa) * rWH, pa.my * (aw0 * ya), pb.mx * (aw1 * xb) * rWH,
                             pb.my * (aw1 * yb)};
  if (live) {
    float* o = d_ol + row * 192;
    *reinterpret_cast<f32x4*>(o + 16 * head + 4 * sub) = doff;
    *reinterpret_cast<float2*>(o + 128 + 8 * head + 2 * sub) = make_float2(aw0 * (ga - s), aw1 * (gb - s));
  }
}

// maxbits[b] = bits of the largest finite |d_out| of sample b (positive floats order as their bit patterns)
__global__ __launch_bounds__(256) void deform_absmax_kernel(const float* __restrict__ d_out, long long n4,
                                                            unsigned int* __restrict__ maxbits) {
  const int b = blockIdx.y;
  const f32x4* p = reinterpret_cast<const f32x4*>(d_out) + (size_t)b * n4;
  int m = 0;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
    const f32x4 v = p[i];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      // a scalar copy first: __builtin_bit_cast of the vector ELEMENT v[k] read element 0 for every k (the compiled loop
      // loaded one dword of the four), so three quarters of d_out never reached the maximum
      const float f = v[k];
      const int a = __builtin_bit_cast(int, f) & 0x7fffffff;
      m = (a < 0x7f800000) ? max(m, a) : m;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = max(m, __shfl_xor(m, o, 64));
  if ((threadIdx.x & 63) == 0 && m > 0) atomicMax(&maxbits[b], (unsigned int)m);
}

// scale exponent F - e of sample b (see the file comment)
__device__ __forceinline__ int fx_shift(unsigned int maxbits, int lgN) {
  int e = 0;
  frexpf(__builtin_bit_cast(float, maxbits), &e);  // max < 2^e (e = 0 for an all-zero gradient)
  return min(62 - lgN, 50) - e;
}

constexpr int TS = 16;             // token tile edge
constexpr int RAD = 9;             // window margin: |offset| <= 8 px (the reference's initial offsets) + the 2nd tap
constexpr int TWN = TS + 2 * RAD;  // window edge (cells)
constexpr int NCELL = TWN * TWN;
constexpr int CS = 8;              // channels per workgroup (a slice of the head's 32)

__global__ __launch_bounds__(256) void deform_scatter_kernel(const float* __restrict__ ol,
                                                             const float* __restrict__ ref_pts, long long ref_bstr,
                                                             const float* __restrict__ d_out, int b, int H, int W,
                                                             const unsigned int* __restrict__ maxbits, int lgN,
                                                             unsigned long long* __restrict__ sums,
                                                             unsigned int* __restrict__ flags) {
  __shared__ unsigned long long win[CS * NCELL];  // channel-major: a wave's adds to one point hit adjacent cells
  const int tid = threadIdx.x;
  const int tiles_x = (W + TS - 1) / TS;
  const int tx0 = (blockIdx.x % tiles_x) * TS, ty0 = (blockIdx.x / tiles_x) * TS;
  const int head = blockIdx.y / (32 / CS), c0 = head * 32 + (blockIdx.y % (32 / CS)) * CS;
  const int ox = tx0 - RAD, oy = ty0 - RAD;
  for (int i = tid; i < CS * NCELL; i += 256) win[i] = 0ull;
  const double scale = ldexp(1.0, fx_shift(maxbits[b], lgN));
  __syncthreads();

  const int x = tx0 + (tid & (TS - 1)), y = ty0 + tid / TS;
  if (x < W && y < H) {
    const long long HW = (long long)H * W;
    const int t = y * W + x;
    const long long row = (long long)b * HW + t;
    const float* r = ol + row * 192;
    float lg[8], off[16];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(r + 16 * head + 4 * k);
      off[4 * k] = v[0]; off[4 * k + 1] = v[1]; off[4 * k + 2] = v[2]; off[4 * k + 3] = v[3];
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(r + 128 + 8 * head + 4 * k);
      lg[4 * k] = v[0]; lg[4 * k + 1] = v[1]; lg[4 * k + 2] = v[2]; lg[4 * k + 3] = v[3];
    }
    // the forward's softmax, same association (pairs, then the quad butterfly)
    const float mx = fmaxf(fmaxf(fmaxf(lg[0], lg[1]), fmaxf(lg[2], lg[3])), fmaxf(fmaxf(lg[4], lg[5]), fmaxf(lg[6], lg[7])));
    float e[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) e[k] = expf(lg[k] - mx);
    const float sum = ((e[0] + e[1]) + (e[2] + e[3])) + ((e[4] + e[5]) + (e[6] + e[7]));
    float g[CS];
    double gd[CS];
    bool gfin = true;
    {
      const float* go = d_out + row * TC + c0;
      const f32x4 u = *reinterpret_cast<const f32x4*>(go), v = *reinterpret_cast<const f32x4*>(go + 4);
      g[0] = u[0]; g[1] = u[1]; g[2] = u[2]; g[3] = u[3];
      g[4] = v[0]; g[5] = v[1]; g[6] = v[2]; g[7] = v[3];
#pragma unroll
      for (int c = 0; c < CS; ++c) {
        gd[c] = (double)g[c];
        gfin = gfin && (fabsf(g[c]) <= 3.402823466e38f);
      }
    }
    const float2 rp = *reinterpret_cast<const float2*>(ref_pts + (size_t)b * ref_bstr + 2 * (size_t)t);
    unsigned long long* gs = sums + c0;
    auto tap = [&](int xi, int yi, float w) {
      const int lx = xi - ox, ly = yi - oy;
      const bool inwin = (unsigned)lx < (unsigned)TWN && (unsigned)ly < (unsigned)TWN;
      const size_t gcell = (size_t)(yi * W + xi);
      if (gfin && fabsf(w) <= 3.402823466e38f) {
        const double wd = (double)w * scale;
#pragma unroll
        for (int c = 0; c < CS; ++c) {
          const unsigned long long v = (unsigned long long)(
              __builtin_bit_cast(long long, __builtin_fma(gd[c], wd, FX_MAGIC)) - FX_MAGIC_BITS);
          if (inwin) atomicAdd(&win[c * NCELL + ly * TWN + lx], v);
          else atomicAdd(&gs[gcell * TC + c], v);
        }
      } else {  // a non-finite factor: flag the products that are not finite, add the others
#pragma unroll
        for (int c = 0; c < CS; ++c) {
          const float prod = g[c] * w;
          if (!(fabsf(prod) <= 3.402823466e38f)) {
            atomicOr(&flags[gcell * 8 + head], 1u << ((c0 & 31) + c));
          } else {
            const unsigned long long v = (unsigned long long)(
                __builtin_bit_cast(long long, __builtin_fma(gd[c], (double)w * scale, FX_MAGIC)) - FX_MAGIC_BITS);
            if (inwin) atomicAdd(&win[c * NCELL + ly * TWN + lx], v);
            else atomicAdd(&gs[gcell * TC + c], v);
          }
        }
      }
    };
#pragma unroll 1
    for (int p = 0; p < 8; ++p) {
      const float aw = e[p] / sum;
      const Pt q = locate(off[2 * p], off[2 * p + 1], rp.x, rp.y, H, W);
      const bool xin0 = q.x0 >= 0 && q.x0 < W, xin1 = q.x0 + 1 >= 0 && q.x0 + 1 < W;
      const bool yin0 = q.y0 >= 0 && q.y0 < H, yin1 = q.y0 + 1 >= 0 && q.y0 + 1 < H;
      if (xin0 && yin0) tap(q.x0, q.y0, q.wx0 * q.wy0 * aw);
      if (xin1 && yin0) tap(q.x0 + 1, q.y0, q.wx1 * q.wy0 * aw);
      if (xin0 && yin1) tap(q.x0, q.y0 + 1, q.wx0 * q.wy1 * aw);
      if (xin1 && yin1) tap(q.x0 + 1, q.y0 + 1, q.wx1 * q.wy1 * aw);
    }
  }
  __syncthreads();
  // flush: the non-zero window elements, 8 channels of a cell = one 64-B run of the global sums
  for (int i = tid; i < CS * NCELL; i += 256) {
    const int cell = i / CS, c = i % CS;
    const unsigned long long v = win[c * NCELL + cell];
    const int xi = ox + cell % TWN, yi = oy + cell / TWN;
    if (v != 0ull && xi >= 0 && xi < W && yi >= 0 && yi < H) atomicAdd(&sums[(size_t)(yi * W + xi) * TC + c0 + c], v);
  }
}

// d_value = sums / scale (flagged elements NaN), 4 elements per thread
__global__ __launch_bounds__(256) void deform_convert_kernel(const unsigned long long* __restrict__ sums,
                                                             const unsigned int* __restrict__ flags, long long n4,
                                                             const unsigned int* __restrict__ maxbits, int b, int lgN,
                                                             float* __restrict__ d_value) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  const double inv = ldexp(1.0, -fx_shift(maxbits[b], lgN));
  const ulonglong2 a = reinterpret_cast<const ulonglong2*>(sums)[2 * i];
  const ulonglong2 c = reinterpret_cast<const ulonglong2*>(sums)[2 * i + 1];
  const unsigned int fl = flags[i >> 3] >> ((i & 7) * 4);
  const unsigned long long s[4] = {a.x, a.y, c.x, c.y};
  f32x4 o;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    o[k] = ((fl >> k) & 1u) ? __builtin_nanf("") : (float)((double)(long long)s[k] * inv);
  reinterpret_cast<f32x4*>(d_value)[i] = o;
}

// Zero fill as a KERNEL, not hipMemsetAsync: inside a captured graph the memset nodes of this entry (two identical ones
// per call from B = 2 on) did not survive a relaunch - sample 1's d_value came out wrong from the second replay on,
// while graphs of kernel nodes alone replay bit-equal.  n16 16-byte words.
__global__ __launch_bounds__(256) void deform_zero_kernel(uint4* __restrict__ p, size_t n16) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (size_t)gridDim.x * 256)
    p[i] = make_uint4(0u, 0u, 0u, 0u);
}
__global__ void deform_zero_words_kernel(unsigned int* __restrict__ p, int n) {
  for (int i = threadIdx.x; i < n; i += blockDim.x) p[i] = 0u;
}

inline int ceil_log2(long long n) {
  int k = 0;
  while ((1LL << k) < n) ++k;
  return k;
}

}  // namespace

extern "C" size_t lss_deform_attn_bwd_workspace_bytes(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0) return 0;
  const size_t HW = (size_t)H * W;
  return HW * TC * 8 + HW * 8 * 4 + (size_t)B * 4;  // one sample's int64 sums + flag words, then B max slots
}

extern "C" int lss_deform_attn_bwd(const float* value, const float* offsets_logits, const float* ref_pts,
                                   long long ref_bstride, const float* d_out, int B, int H, int W, int n_heads,
                                   int n_points, int C, void* workspace, size_t workspace_bytes, float* d_value,
                                   float* d_offsets_logits, void* stream) {
  LSS_CHECK_PTR(value); LSS_CHECK_PTR(offsets_logits); LSS_CHECK_PTR(ref_pts); LSS_CHECK_PTR(d_out);
  LSS_CHECK_PTR(workspace); LSS_CHECK_PTR(d_value); LSS_CHECK_PTR(d_offsets_logits);
  LSS_CHECK_POS(B); LSS_CHECK_POS(H); LSS_CHECK_POS(W);
  if (n_heads != 8 || n_points != 8 || C != TC) return LSS_E_SHAPE;
  if (ref_bstride < 0) return LSS_E_SHAPE;
  const long long HW = (long long)H * W, rows = (long long)B * HW;
  if (rows >= (1LL << 31) || B > 65535) return LSS_E_SHAPE;
  if (!lss_aligned(value, 16) || !lss_aligned(offsets_logits, 16) || !lss_aligned(d_out, 16) || !lss_aligned(workspace, 16) ||
      !lss_aligned(d_value, 16) || !lss_aligned(d_offsets_logits, 16))
    return LSS_E_ALIGN;
  if ((reinterpret_cast<uintptr_t>(ref_pts) & 7) != 0 || (ref_bstride & 1) != 0) return LSS_E_ALIGN;
  if (workspace_bytes < lss_deform_attn_bwd_workspace_bytes(B, H, W)) return LSS_E_WORKSPACE;
  hipStream_t st = lss_stream(stream);
  unsigned long long* sums = static_cast<unsigned long long*>(workspace);
  unsigned int* flags = reinterpret_cast<unsigned int*>(sums + HW * TC);
  unsigned int* maxbits = flags + HW * 8;
  const int lgN = ceil_log2(HW);
  const long long n4 = HW * TC / 4;
  const size_t n16 = (size_t)HW * (TC * 8 + 8 * 4) / 16;

  hipLaunchKernelGGL(deform_grad_ol_kernel, dim3(lss_cdiv(rows, 8)), dim3(256), 0, st, value, offsets_logits,
                     ref_pts, ref_bstride, d_out, B, H, W, d_offsets_logits);
  int rc = lss_launch_status();
  if (rc) return rc;
  hipLaunchKernelGGL(deform_zero_words_kernel, dim3(1), dim3(256), 0, st, maxbits, B);
  if ((rc = lss_launch_status())) return rc;
  hipLaunchKernelGGL(deform_absmax_kernel, dim3((unsigned)std::min<long long>(lss_cdiv(n4, 256), 256), B), dim3(256),
                     0, st, d_out, n4, maxbits);
  if ((rc = lss_launch_status())) return rc;
  const int tiles = lss_cdiv(H, TS) * lss_cdiv(W, TS);
  // samples one after another through one sample's sums (the workspace stays B-independent)
  for (int b = 0; b < B; ++b) {
    hipLaunchKernelGGL(deform_zero_kernel, dim3((unsigned)std::min<size_t>((n16 + 255) / 256, 4096)), dim3(256), 0, st,
                       reinterpret_cast<uint4*>(sums), n16);  // the sums and the flag words behind them
    if ((rc = lss_launch_status())) return rc;
    hipLaunchKernelGGL(deform_scatter_kernel, dim3(tiles, 8 * (32 / CS)), dim3(256), 0, st, offsets_logits, ref_pts,
                       ref_bstride, d_out, b, H, W, maxbits, lgN, sums, flags);
    if ((rc = lss_launch_status())) return rc;
    hipLaunchKernelGGL(deform_convert_kernel, dim3(lss_cdiv(n4, 256)), dim3(256), 0, st, sums, flags, n4, maxbits, b,
                       lgN, d_value + (size_t)b * HW * TC);
    if ((rc = lss_launch_status())) return rc;
  }
  return 0;
}
