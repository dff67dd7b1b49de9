// K8: BevEncode convolutions as implicit GEMM on MFMA, NHWC activations.
//
//   out[m, co] = act( scale[co] * sum_{tap, ci} in[pix(m) + tap, ci] * w[tap, co, ci]
//                     + shift[co] + residual[m, co] )
// m = (b, oy, ox) output pixel.  `in` is x, or - fused into the operand gather -
// cat([x2, bilinear_upsample_align_corners(x, up)], channel) of the reference's
// `Up.forward` (src/modules.py:22-26) and of `up2[0]` (src/modules.py:110-111).
//
// Kernel `conv_direct_kernel` (all shapes): 256 threads = 4 waves; the workgroup
// computes 128 output pixels x 64 output channels, wave w the pixel rows
// [32w, 32w+32) against both 32-wide channel tiles:
//   bf16: v_mfma_f32_32x32x16_bf16, A[row r][k = 8h + j]  B[k = 8h + j][col c]
//   f32 : v_mfma_f32_32x32x2_f32,   A[row r][k = h]       B[k = h][col c]
// (r = c = lane & 31, h = lane >> 5).  Operand fragments are loaded straight
// from global memory in 16-B pieces: within a K block every lane half h owns a
// contiguous run of channels (32 bf16 / 4 f32) and k-step s consumes its s-th
// piece on BOTH operands, so activations (NHWC) and weights ([tap][co][ci]) keep
// their natural layouts - only the order of the K summation is permuted.
#include "conv_launch.h"
#include "lss_device.h"

namespace {

struct ConvArgs {
  const void* x;
  const void* x2;
  const void* w;
  const float* scale;
  const float* shift;
  const void* residual;
  void* y;
  float* stats;
  int B, H, W;  // spatial size of x (low-res source when up > 1)
  int Cx, C2, up;
  int Hin, Win;  // H*up, W*up: the conv's input plane
  int Cin;       // C2 + Cx
  int Cout, KH, KW, stride, pad;
  int Ho, Wo, M;
  int relu;     // activation: 0 none, 1 ReLU, 2 GELU (erf form)
  int out_f32;  // bf16 kernels: write y as fp32
  int wt;       // epilogue stores write through (sc1): nothing left dirty in L2 at the kernel boundary
  // two convs over the same input in one launch (a BasicBlock's stride-2 conv1 and its 1x1
  // downsample): output channels [0, split) go to y, [split, Cout) to y2, each dense; the
  // activation applies to channels below relu_n only.  split, relu_n are multiples of the 128-wide tile.
  void* y2;
  int split, relu_n;
  float ry, rx;  // (H-1)/(Hin-1), (W-1)/(Win-1) for the align_corners upsample
  // optional fused 1x1 head (ref: src/modules.py:115 up2[4]): out[b,k,oy,ox] =
  // head_b[k] + sum_co act(...)[co] * head_w[k, co]; NCHW fp32; needs Cout == BN
  const float* head_w;
  const float* head_b;
  float* head_out;
  int head_n;
  // diagnostics (tools/conv_phase_stamps.py): 8 x 100-MHz s_memrealtime stamps per workgroup, or null
  unsigned long long* stamps;
  int src_lds;  // MODE 1, KC = 32: the low-res source patch of a chunk is staged in LDS (see SRC below)
};

// libm's erff, not lss_gelu's polynomial: the fp32 parity path runs through here
__device__ __forceinline__ float conv_act(float v, int act) {
  if (act == 1) return fmaxf(v, 0.f);
  if (act == 2) return 0.5f * v * (1.f + erff(v * 0.70710678118654752f));
  return v;
}

template <typename T>
struct Frag;
template <>
struct Frag<unsigned short> {  // bf16: 8 channels per 16-B piece
  typedef bf16x8 type;
  static constexpr int PIECE = 8;    // channels per 16-B piece
  static constexpr int KBLOCK = 64;  // channels per K block (2 halves x 4 pieces)
};
template <>
struct Frag<float> {
  typedef f32x4 type;
  static constexpr int PIECE = 4;
  static constexpr int KBLOCK = 8;  // 2 halves x 1 piece (4 k-steps of 2)
};

__device__ __forceinline__ f32x4 lerp4(f32x4 a, f32x4 b, float t) {
  f32x4 r;
#pragma unroll
  for (int i = 0; i < 4; ++i) r[i] = a[i] + t * (b[i] - a[i]);
  return r;
}

// bilinear blend of four 8-channel bf16 pieces in the four-weight form, on (lo, hi)
// channel pairs: float2 arithmetic maps to v_pk_mul_f32 / v_pk_fma_f32.  One rounding to bf16.
// (conv_ring.hip's rk_blend is the scalar-FMA form of the same blend, on purpose.)
__device__ __forceinline__ f32x2 unpack_bf2(unsigned int u) {
  f32x2 v;
  v[0] = __builtin_bit_cast(float, u << 16);
  v[1] = __builtin_bit_cast(float, u & 0xffff0000u);
  return v;
}
__device__ __forceinline__ uint4 blend_bf16x8(const uint4& q00, const uint4& q01, const uint4& q10,
                                              const uint4& q11, float lx, float ly) {
  const float w11 = lx * ly, w10 = ly - w11, w01 = lx - w11, w00 = 1.f - lx - ly + w11;
  const unsigned int* u00 = reinterpret_cast<const unsigned int*>(&q00);
  const unsigned int* u01 = reinterpret_cast<const unsigned int*>(&q01);
  const unsigned int* u10 = reinterpret_cast<const unsigned int*>(&q10);
  const unsigned int* u11 = reinterpret_cast<const unsigned int*>(&q11);
  uint4 out;
  unsigned int* o = reinterpret_cast<unsigned int*>(&out);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f32x2 r = unpack_bf2(u00[i]) * w00;
    r = __builtin_elementwise_fma(unpack_bf2(u01[i]), (f32x2){w01, w01}, r);
    r = __builtin_elementwise_fma(unpack_bf2(u10[i]), (f32x2){w10, w10}, r);
    r = __builtin_elementwise_fma(unpack_bf2(u11[i]), (f32x2){w11, w11}, r);
    o[i] = lss_pack_bf2(r[0], r[1]);
  }
  return out;
}

// 16-B piece (bf16: 8 ch, f32: 4 ch) of pixel (b, iy, ix) of the conv's virtual
// input, channel offset c (multiple of the piece size, never straddling x2 | x).
template <typename T, bool FUSED>
__device__ __forceinline__ uint4 load_in_piece(const ConvArgs& a, int b, int iy, int ix, int c) {
  if (!FUSED) {
    const T* p = reinterpret_cast<const T*>(a.x) + (((size_t)b * a.H + iy) * a.W + ix) * a.Cx + c;
    return *reinterpret_cast<const uint4*>(p);
  }
  if (c < a.C2) {
    const T* p = reinterpret_cast<const T*>(a.x2) + (((size_t)b * a.Hin + iy) * a.Win + ix) * a.C2 + c;
    return *reinterpret_cast<const uint4*>(p);
  }
  c -= a.C2;
  // nn.Upsample(bilinear, align_corners=True): src = dst * (in-1)/(out-1)
  const float sy = a.ry * (float)iy, sx = a.rx * (float)ix;
  const int y0 = (int)sy, x0 = (int)sx;
  const int y1 = y0 + (y0 < a.H - 1 ? 1 : 0), x1 = x0 + (x0 < a.W - 1 ? 1 : 0);
  const float ly = sy - (float)y0, lx = sx - (float)x0;
  const T* base = reinterpret_cast<const T*>(a.x) + (size_t)b * a.H * a.W * a.Cx + c;
  const uint4 q00 = *reinterpret_cast<const uint4*>(base + ((size_t)y0 * a.W + x0) * a.Cx);
  const uint4 q01 = *reinterpret_cast<const uint4*>(base + ((size_t)y0 * a.W + x1) * a.Cx);
  const uint4 q10 = *reinterpret_cast<const uint4*>(base + ((size_t)y1 * a.W + x0) * a.Cx);
  const uint4 q11 = *reinterpret_cast<const uint4*>(base + ((size_t)y1 * a.W + x1) * a.Cx);
  uint4 out;
  if (sizeof(T) == 4) {
    const f32x4 top = lerp4(__builtin_bit_cast(f32x4, q00), __builtin_bit_cast(f32x4, q01), lx);
    const f32x4 bot = lerp4(__builtin_bit_cast(f32x4, q10), __builtin_bit_cast(f32x4, q11), lx);
    out = __builtin_bit_cast(uint4, lerp4(top, bot, ly));
  } else {
    const unsigned int* u00 = reinterpret_cast<const unsigned int*>(&q00);
    const unsigned int* u01 = reinterpret_cast<const unsigned int*>(&q01);
    const unsigned int* u10 = reinterpret_cast<const unsigned int*>(&q10);
    const unsigned int* u11 = reinterpret_cast<const unsigned int*>(&q11);
    unsigned int* o = reinterpret_cast<unsigned int*>(&out);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float r[2];
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) {
        const int sh = hh * 16;
        const float v00 = lss_bf2f((unsigned short)(u00[i] >> sh)), v01 = lss_bf2f((unsigned short)(u01[i] >> sh));
        const float v10 = lss_bf2f((unsigned short)(u10[i] >> sh)), v11 = lss_bf2f((unsigned short)(u11[i] >> sh));
        const float top = v00 + lx * (v01 - v00), bot = v10 + lx * (v11 - v10);
        r[hh] = top + ly * (bot - top);
      }
      o[i] = lss_pack_bf2(r[0], r[1]);
    }
  }
  return out;
}

// BN statistics of channel c (both kernels): the lane halves h = 0, 1 hold the sums s1 = sum raw, s2 = sum raw^2 over
// different pixel rows of the same channel; half 0 adds the pair's totals to stats[c], stats[Cout + c]
__device__ __forceinline__ void bn_stats_add(float* stats, int Cout, int c, int h, bool cok, float s1, float s2) {
  s1 += __shfl_xor(s1, 32, 64);
  s2 += __shfl_xor(s2, 32, 64);
  if (h == 0 && cok) {
    atomicAdd(stats + c, s1);
    atomicAdd(stats + Cout + c, s2);
  }
}

template <typename T, bool FUSED>
__global__ __launch_bounds__(256) void conv_direct_kernel(ConvArgs a) {
  constexpr int PIECE = Frag<T>::PIECE;
  constexpr int KBLOCK = Frag<T>::KBLOCK;
  constexpr int NPIECE = KBLOCK / 2 / PIECE;  // pieces per lane half per K block (4 / 1)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int m0 = blockIdx.x * 128 + wave * 32;
  const int n0 = blockIdx.y * 64;
  const int m = m0 + r;
  const bool m_ok = m < a.M;
  int b = 0, oy = 0, ox = 0;
  if (m_ok) {
    b = m / (a.Ho * a.Wo);
    const int rem = m - b * (a.Ho * a.Wo);
    oy = rem / a.Wo;
    ox = rem - oy * a.Wo;
  }
  const T* wbase = reinterpret_cast<const T*>(a.w);
  const int co0 = n0 + r, co1 = n0 + 32 + r;
  const bool c0_ok = co0 < a.Cout, c1_ok = co1 < a.Cout;

  f32x16 acc0, acc1;
#pragma unroll
  for (int i = 0; i < 16; ++i) { acc0[i] = 0.f; acc1[i] = 0.f; }

  for (int ky = 0; ky < a.KH; ++ky) {
    const int iy = oy * a.stride - a.pad + ky;
    for (int kx = 0; kx < a.KW; ++kx) {
      const int ix = ox * a.stride - a.pad + kx;
      const bool in_ok = m_ok && iy >= 0 && iy < a.Hin && ix >= 0 && ix < a.Win;
      const int tap = ky * a.KW + kx;
      const T* w0 = wbase + ((size_t)tap * a.Cout + co0) * a.Cin;
      const T* w1 = wbase + ((size_t)tap * a.Cout + co1) * a.Cin;
      for (int cb = 0; cb < a.Cin; cb += KBLOCK) {
        const int c = cb + h * (KBLOCK / 2);
        uint4 av[NPIECE], b0[NPIECE], b1[NPIECE];
#pragma unroll
        for (int s = 0; s < NPIECE; ++s) {
          av[s] = make_uint4(0, 0, 0, 0);
          b0[s] = make_uint4(0, 0, 0, 0);
          b1[s] = make_uint4(0, 0, 0, 0);
          const bool k_ok = c + s * PIECE < a.Cin;  // bf16 rows of Cin % 64 == 32 channels end inside the last block
          if (in_ok && k_ok) av[s] = load_in_piece<T, FUSED>(a, b, iy, ix, c + s * PIECE);
          if (c0_ok && k_ok) b0[s] = *reinterpret_cast<const uint4*>(w0 + c + s * PIECE);
          if (c1_ok && k_ok) b1[s] = *reinterpret_cast<const uint4*>(w1 + c + s * PIECE);
        }
        if (sizeof(T) == 2) {
#pragma unroll
          for (int s = 0; s < NPIECE; ++s) {
            const bf16x8 fa = __builtin_bit_cast(bf16x8, av[s]);
            acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, __builtin_bit_cast(bf16x8, b0[s]), acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, __builtin_bit_cast(bf16x8, b1[s]), acc1, 0, 0, 0);
          }
        } else {
          const f32x4 fa = __builtin_bit_cast(f32x4, av[0]);
          const f32x4 f0 = __builtin_bit_cast(f32x4, b0[0]);
          const f32x4 f1 = __builtin_bit_cast(f32x4, b1[0]);
#pragma unroll
          for (int s = 0; s < 4; ++s) {
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[s], f0[s], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[s], f1[s], acc1, 0, 0, 0);
          }
        }
      }
    }
  }

  // epilogue: D[row = (i&3) + 8*(i>>2) + 4*h][col = r]
  T* y = reinterpret_cast<T*>(a.y);
  const T* res = reinterpret_cast<const T*>(a.residual);
#pragma unroll
  for (int nt = 0; nt < 2; ++nt) {
    const int co = nt == 0 ? co0 : co1;
    const bool cok = nt == 0 ? c0_ok : c1_ok;
    const float sc = (cok && a.scale) ? a.scale[co] : 1.f;
    const float sh = (cok && a.shift) ? a.shift[co] : 0.f;
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int row = (i & 3) + 8 * (i >> 2) + 4 * h;
      const int mm = m0 + row;
      const float raw = nt == 0 ? acc0[i] : acc1[i];
      if (mm < a.M && cok) {
        s1 += raw;
        s2 += raw * raw;
        float v = raw * sc + sh;
        const size_t o = (size_t)mm * a.Cout + co;
        if (res) v += (sizeof(T) == 2) ? lss_bf2f(reinterpret_cast<const unsigned short*>(res)[o])
                                       : reinterpret_cast<const float*>(res)[o];
        v = conv_act(v, a.relu);
        if (sizeof(T) == 2 && !a.out_f32) reinterpret_cast<unsigned short*>(y)[o] = lss_f2bf(v);
        else reinterpret_cast<float*>(y)[o] = v;
      }
    }
    if (a.stats) bn_stats_add(a.stats, a.Cout, co, h, cok, s1, s2);
  }
}

// ---------------------------------------------------------------------------
// conv_lds_kernel: the bf16 convolutions of BevEncode (3x3 / stride 1 carries 95 % of its FLOPs; the
// stride-2 3x3 / 7x7 run as stride-1 convs over the four parity phases, MODE 2).  Output-stationary,
// LDS-tiled:
//   * workgroup (256 threads; 2 per CU, 3 with KC = 32) = TH x 16 output pixels x BN output channels
//     of one image; a wave owns RT x 2 tiles of v_mfma_f32_32x32x16_bf16 (RT = 2: 4 pixel rows x 64
//     channels, 64 accumulator registers; RT = 1 for grids that would leave CUs idle);
//   * per KC-channel chunk (64, or 32 for the fused-gather layers) of the input the (TH+2) x 18 halo'd
//     patch is gathered ONCE into LDS (the fused bilinear-upsample / concat gather runs here, once per
//     element instead of once per tap; its low-res source window is itself staged by LDS-DMA, see
//     SRC) and re-used by all taps through shifted ds_read_b128 windows;
//   * per (chunk, tap) step the BN x KC weight slab streams global -> LDS by LDS-DMA
//     (global_load_lds_dwordx4, no VGPR round trip) into a 3-slot ring, two steps ahead of the
//     MFMAs; the step barrier is a raw s_barrier behind a COUNTED vmcnt, so the younger slab stays in
//     flight across it;
//   * KSP = 2 (512 threads): two 4-wave groups split the input channels of one tile (grids of at most
//     256 workgroups); the epilogue stages the fp32 tile in LDS and stores 16-B pieces (write-through),
//     optionally reducing a fused 1x1 head instead.
// LDS images: patch positions are KC*2 + 16 B apart (the 16-B pad) and patch rows are padded to a
// multiple of 256 B, which makes the two pixel rows of a 32-row MFMA tile land on complementary bank
// sets (conflict-free ds_read_b128); weight rows are KC*2 B, XOR-swizzled in 16-B pieces on the DMA's
// SOURCE address (the DMA destination is lane-linear) and on the read address.
//
// MODE 0: plain NHWC input, stride 1.  MODE 1: fused [x2 | bilinear-upsampled x] input.
// MODE 2: stride-2 conv as a stride-1 conv over the 4 parity phases of the input
// (space-to-depth done by the gather: chunk -> (phase, 64-channel block); weights
// come pre-arranged as [tap'][co][phase*Cx + c] from lss_conv2d_pack_weights_s2d).
// KH x KW = taps of the stride-1 problem, PAD = patch rows/cols before the output pixel.
// RT = 32-pixel MFMA row tiles per wave (2: 4 image rows x 64 channels per wave, the
// throughput shape; 1: 2 image rows, half the work per workgroup - used when the RT = 2
// grid would leave CUs idle, where the per-workgroup critical path is what counts).
// HEAD: the epilogue reduces the fused 1x1 head instead of storing the activation (its own instantiation: the
// head and the store path each keep only their own operands live - the store path's residual prefetch and
// the head's operand fragments together overflowed the 168-register budget of the KC = 32 kernels).
// (Variants built, measured and removed in round 3 - numbers in DESIGN.md section 4: PFB = blend of the next chunk
// under the last taps' MFMAs, PSP = pixel-split pairs on one weight ring, 64-channel tall tiles, mixed full / half
// height launches, s_setprio around the MFMA groups, a 3-slot ring for KC = 32.  The big layers now run on the
// loader / consumer kernel of conv_ring.hip at the sizes it takes; this kernel keeps them at small batch.)
constexpr int LSS_CONV_RING32 = 4;  // ring slots of the KC = 32 kernels

// Everything one instantiation of the tile kernel knows at compile time: the tile, its LDS images and their sizes,
// the work per thread.  The kernel sizes its LDS from SMEM_BYTES; every phase below reads its constants here.
template <int RT_, int BN_, int MODE_, int KH_, int KW_, int PAD_, int KC_ = 64, int KSP_ = 1, bool HEAD_ = false, int TPS_ = 1>
struct TileCfg {
  static constexpr int RT = RT_, BN = BN_, MODE = MODE_, KH = KH_, KW = KW_, PAD = PAD_, KC = KC_, KSP = KSP_, TPS = TPS_;
  static constexpr bool HEAD = HEAD_;
  // KSP = 2: intra-workgroup split-K for grids that cannot fill the chip (layer2/layer3: 112-208
  // workgroups of 18-36 latency-bound steps on 256 CUs).  512 threads = two 4-wave groups, each
  // with its own weight ring and patch, each taking half of the input-channel chunks; the second
  // group's accumulators meet the first's through LDS before the (unchanged) epilogue.  Halves
  // the main loop at the same workgroup count; barriers stay workgroup-wide (both groups run the
  // same step sequence).
  static_assert(KSP == 1 || (KSP == 2 && KC == 64), "KSP");
  // TPS = taps per step.  2: a step is TWO taps against a double slab - half the steps (barrier + counted wait + slot
  // hand-over each) per chunk.  For the 7x7 / 2 stem, whose 64 steps carry only 8 MFMAs per wave each: phase stamps put
  // a step at 0.43 us against 0.13 us of MFMA issue.  Needs an even tap count and the 24 KB more LDS (BN = 64 only).
  static_assert(TPS == 1 || (TPS == 2 && (KH * KW) % 2 == 0 && KSP == 1 && MODE != 1), "TPS");
  // KC = input channels per (chunk, tap) step.  64: the default.  32: half-depth slabs and patch
  // (39 KB of LDS, <= 168 VGPRs) so THREE workgroups share a CU - used for the big stride-1 layers,
  // whose 728 / 1300 tiles then run in one / two full rounds instead of 1.4 / 2.5 on 512 slots.
  static_assert(KC == 64 || KC == 32, "KC");
  static constexpr int PPP = KC / 8;   // 16-B pieces per patch position
  static constexpr int KS = KC / 16;   // MFMA k-steps per tap
  static constexpr int PSH = KC == 64 ? 3 : 2;  // log2(PPP)
  static constexpr int TH = (4 / (BN / 64)) * RT * 2;  // image rows per workgroup
  static constexpr bool FUSED = MODE == 1;
  static constexpr int NT = KH * KW;
  static constexpr int NS = NT / TPS;  // steps per chunk
  static constexpr int TW = 16, IW = TW + KW - 1, IH = TH + KH - 1, POSB = KC * 2 + 16;
  static constexpr int IROWB = (IW * POSB + 255) / 256 * 256;  // 2816 (KC = 64), 1536 (KC = 32)
  static constexpr int IN_BYTES = IH * IROWB;
  static constexpr int NPIECE = IH * IW * PPP;  // 16-B pieces of the patch
  static constexpr int W1_BYTES = BN * KC * 2;      // slab of one tap
  static constexpr int W_BYTES = TPS * W1_BYTES;    // slab of one step
  static constexpr int BPT = W1_BYTES / 1024;  // 1-KiB DMA blocks per tap
  static constexpr int WPT = W_BYTES / 4096;  // LDS-DMA instructions per wave per step (1 KiB each)
  static constexpr int NWV = 4;               // waves that share one slab
  static constexpr int WCOLS = BN / 64;  // waves along the channel axis
  static constexpr int IPT = (NPIECE + 255) / 256;  // 16-B patch pieces per thread per chunk
  static constexpr int OLD = BN + 4;  // fp32 row stride of the epilogue's staged output tile
  // the epilogue stages the fp32 output tile in LDS: whole (KC = 64) or in two halves of TH/2 rows
  static constexpr int EPH = KC == 32 ? 2 : 1;
  static constexpr int OUT_BYTES = (TH / EPH) * 16 * OLD * 4;  // per pixel group
  // Weight ring: 3 slots = slabs two steps ahead of the MFMAs; the KC = 32 kernels (half-length steps, three
  // workgroups per CU) keep 4 slots = three steps ahead: a timing build that re-read one L1-hot slab ran them 9-13 %
  // faster while the KC = 64 kernel did not move, i.e. their shorter steps exposed the L2 round trip of the slab.
  static constexpr int NSL = KC == 32 ? LSS_CONV_RING32 : 3, LA = NSL - 1;
  static constexpr int WYOUNG = (LA - 1) * WPT;  // DMA instructions of the slabs younger than the next step's
  static constexpr int PF_ST = NS >= 5 ? NS - 4 : 0;  // the step at which the next patch's loads are issued
  static constexpr int GROUP_BYTES = (NSL * W_BYTES + IN_BYTES + 1023) / 1024 * 1024;  // ring + patch of one K-split group
  // SRC (fused upsample, KC = 32): the low-res pixels a chunk's patch is interpolated from - at most
  // SRC_H x SRC_W source positions for scale factors >= 2 - are copied ONCE per chunk into LDS by
  // LDS-DMA while the previous chunk's taps run, and the 4-corner blend then reads LDS: 2 DMA
  // instructions per wave instead of 12 scattered global loads per thread in the synchronous
  // chunk-boundary phase (measured: that phase was 17 % of the fused convs).
  static constexpr bool SRC = FUSED && KC == 32;
  static constexpr int SRC_H = (IH - 1) / 2 + 3, SRC_W = (IW - 1) / 2 + 3;  // 7 x 11 for the 10 x 18 patch
  static constexpr int SRC_PIECES = SRC ? (SRC_H * SRC_W * PPP + 63) / 64 : 0;  // 1-KiB DMA pieces per chunk (5)
  static constexpr int SRC_DMA = (SRC_PIECES + 3) / 4;  // DMA instructions per chunk of the wave that issues most (wave 0)
  static constexpr int SRC_BYTES = SRC_PIECES * 1024;
  static constexpr int NG = FUSED ? IPT : 1, NSRC = SRC ? SRC_DMA : 1;  // lengths of g_off / g_w and src_o (FusedPieces)
  static constexpr int MAIN_BYTES = KSP * GROUP_BYTES > OUT_BYTES ? KSP * GROUP_BYTES : OUT_BYTES;
  static constexpr int SMEM_BYTES = MAIN_BYTES + SRC_BYTES;
  static_assert(SMEM_BYTES <= (KSP == 2 ? 160 : (KC == 32 ? 53 : 80)) * 1024, "workgroups per CU vs 160 KiB of LDS");
  static_assert(!SRC || NS > LA, "the source copies retire at step LA");
  static_assert(KC == 64 || (RT == 2 && BN == 128 && MODE != 2), "KC = 32 is built for the RT = 2, BN = 128 stride-1 tiles");
  // Output pieces.  A piece = 8 consecutive channels (16 B of bf16) of one pixel; 256 threads cover PPJ pixels x CG
  // channel groups per pass, so a thread's pixel column, channel group and first row never change: every per-pass
  // address is one base + a compile-time offset.
  static constexpr int CG = BN / 8;              // 16-B channel groups per pixel
  static constexpr int PPJ = 256 / CG;           // pixels per pass
  static constexpr int RPJ = PPJ / 16;           // image rows per pass
  static constexpr int HROWS = TH / EPH;         // image rows per staged half (EPH = 2: KC = 32, see OUT_BYTES)
  static constexpr int HPIECES = HROWS * 16 * CG;
  static constexpr int EPJ = HPIECES / 256;      // passes per half
  static_assert(HPIECES % 256 == 0 && PPJ % 16 == 0, "half tiles split evenly over the threads");
  // EARLY_RES: the residual rows of the launch-bound layers (RT = 1: 152-190 registers, room for 16 more) are
  // requested at the top of the LAST chunk's taps instead of at the top of the epilogue: phase stamps put the store
  // phase of the residual layers at 1.6-1.7 us against 1.0-1.1 us for the same tile without a residual - the loads,
  // issued ~0.6 us before their first use, were still in flight when the store loop wanted them.
  static constexpr bool EARLY_RES = RT == 1 && EPH == 1 && !HEAD;
  static constexpr int NRES = HEAD ? 1 : EPJ;  // residual pieces a thread holds
};

// 16-B piece q of the patch -> its row, its column and its channel piece
struct PatchPiece {
  int py, px, part;
};
template <class C>
__device__ __forceinline__ PatchPiece patch_piece(int q) {
  const int pos = q >> C::PSH, part = q & (C::PPP - 1);
  const int py = pos / C::IW, px = pos - py * C::IW;
  return {py, px, part};
}

// the four corners at p00, +dx, +dy, +dy+dx (in units of P: bytes of the LDS source window, elements of x), blended
// with the 16-bit fixed-point weights gw = lx | ly << 16
template <typename P>
__device__ __forceinline__ uint4 blend_corners(const P* p00, int dx, int dy, const unsigned int& gw) {
  const uint4 q00 = *reinterpret_cast<const uint4*>(p00);
  const uint4 q01 = *reinterpret_cast<const uint4*>(p00 + dx);
  const uint4 q10 = *reinterpret_cast<const uint4*>(p00 + dy);
  const uint4 q11 = *reinterpret_cast<const uint4*>(p00 + dy + dx);
  return blend_bf16x8(q00, q01, q10, q11, (float)(gw & 0xffff) * (1.f / 65536.f), (float)(gw >> 16) * (1.f / 65536.f));
}

// Fused 1x1 head ON THE MATRIX PIPE (ref src/modules.py:115, up2[4]; at most 16 classes), on the HROWS image rows from
// oyh of the staged fp32 tile: per image row one 16 x 16 x BN product
// out[pixel][k] = sum_c relu(act[pixel][c]) * head_w[k][c]  on v_mfma_f32_16x16x32_bf16.
// Both operands are split into bf16 hi + lo parts (x = hi + lo to 16 significant bits) and the three
// products hi*hi, hi*lo, lo*hi are accumulated in fp32, so the result keeps the accuracy of the fp32
// head it replaces (the dropped lo*lo term is 2^-16 relative) while the VALU work per pixel falls from
// ~60 FMA / DPP instructions to ~12 conversions.  A: lane (r = pixel, q) <- 8 consecutive channels of the
// fp32 tile in LDS (2 ds_read_b128); B: lane (k = lane & 15, q) <- 8 consecutive weights of class k from
// global (L1-resident: 2 KiB); D: lane (k, q) holds pixels 4q..4q+3 of the row = ONE 16-B NCHW store.
template <class C>
__device__ __forceinline__ void head_mfma(const ConvArgs& a, const float* otile, int b, int oyh, int ox0, int lane,
                                          int wave) {
  constexpr int BN = C::BN;
  const int hr = lane & 15, hq = lane >> 4;
  for (int row = wave; row < C::HROWS; row += 4) {
    const int oy = oyh + row;
    f32x4 hacc = {0.f, 0.f, 0.f, 0.f};
    const float* arow = otile + (row * 16 + hr) * C::OLD + hq * 8;
    const float* wrow = a.head_w + (size_t)min(hr, a.head_n - 1) * BN + hq * 8;
    // rolled: one k-step's 16 operand floats live at a time (the other half-tile's waves still hold their
    // 64 accumulator registers here, and the 168-register budget of three workgroups per CU is what counts)
#pragma unroll 1
    for (int s = 0; s < BN / 32; ++s) {
      bf16x8 xh, xl, wh, wl;
      {
        f32x4 w0 = *reinterpret_cast<const f32x4*>(wrow + s * 32);
        f32x4 w1 = *reinterpret_cast<const f32x4*>(wrow + s * 32 + 4);
        if (hr >= a.head_n) { w0 = (f32x4){0.f, 0.f, 0.f, 0.f}; w1 = w0; }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float wv = j < 4 ? w0[j & 3] : w1[j & 3];
          const unsigned short whi = lss_f2bf(wv);
          wh[j] = (short)whi;
          wl[j] = (short)lss_f2bf(wv - lss_bf2f(whi));
        }
      }
      {
        const f32x4 x0 = *reinterpret_cast<const f32x4*>(arow + s * 32);
        const f32x4 x1 = *reinterpret_cast<const f32x4*>(arow + s * 32 + 4);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float xv = j < 4 ? x0[j & 3] : x1[j & 3];
          if (a.relu) xv = fmaxf(xv, 0.f);
          const unsigned short xhi = lss_f2bf(xv);
          xh[j] = (short)xhi;
          xl[j] = (short)lss_f2bf(xv - lss_bf2f(xhi));
        }
      }
      hacc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xl, wh, hacc, 0, 0, 0);
      hacc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xh, wl, hacc, 0, 0, 0);
      hacc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xh, wh, hacc, 0, 0, 0);
    }
    if (hr < a.head_n && oy < a.Ho) {
      const float hb = a.head_b[hr];
      float* op = a.head_out + (((size_t)b * a.head_n + hr) * a.Ho + oy) * a.Wo + ox0 + hq * 4;
      if ((a.Wo & 3) == 0 && ox0 + hq * 4 + 4 <= a.Wo) {
        *reinterpret_cast<f32x4*>(op) = (f32x4){hacc[0] + hb, hacc[1] + hb, hacc[2] + hb, hacc[3] + hb};
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (ox0 + hq * 4 + i < a.Wo) op[i] = hacc[i] + hb;
      }
    }
  }
}

// fused 1x1 head, VALU form (more than 16 classes): the CG = BN / 8 lanes that hold the channels of one pixel reduce
// their partial dot products with DPP row operations; the activation itself is never stored
template <class C>
__device__ __forceinline__ void head_valu(const ConvArgs& a, const float* otile, int b, int oyh, int ox0, int tid) {
  constexpr int CG = C::CG, OLD = C::OLD;
  for (int e = tid; e < C::HROWS * 16 * CG; e += 256) {
    const int pl = e / CG, hc8 = e % CG;
    const int oy = oyh + (pl >> 4), hx = ox0 + (pl & 15);
    const f32x4 v0 = *reinterpret_cast<const f32x4*>(otile + pl * OLD + hc8 * 8);
    const f32x4 v1 = *reinterpret_cast<const f32x4*>(otile + pl * OLD + hc8 * 8 + 4);
    float v[8] = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
    if (a.relu) {
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] = fmaxf(v[k], 0.f);
    }
    for (int k = 0; k < a.head_n; ++k) {
      const float* hw = a.head_w + k * C::BN + hc8 * 8;
      float part = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) part = fmaf(v[j], hw[j], part);
      // sum over the CG lanes of the pixel on DPP row operations (no LDS round trips): lane ^ 1,
      // lane ^ 2, then - every quad now holding its sum - the other quad of the 8 (row_half_mirror)
      // and the other half of the 16 (row_mirror)
      part += lss_dpp_f32<0xB1>(part);
      part += lss_dpp_f32<0x4E>(part);
      part += lss_dpp_f32<0x141>(part);
      if (CG == 16) part += lss_dpp_f32<0x140>(part);
      if (hc8 == 0 && oy < a.Ho && hx < a.Wo)
        a.head_out[(((size_t)b * a.head_n + k) * a.Ho + oy) * a.Wo + hx] = part + a.head_b[k];
    }
  }
}

// The tile body: one workgroup's output tile.  The phases that carry the accumulators, the parked patch registers and
// the ring slot are lambdas of this ONE function, in the order they run: coordinates, fragment offsets, weight-slab
// issue, fused-gather set-up, the gathers, output pieces, prologue, main loop, K-split hand-over, staging, statistics,
// head or store.  (As separate functions taking that state by reference each is optimised on its own before it is
// inlined; measured: accumulators re-formed as one 32-float vector, the last chunk peeled, 12-168 B of new scratch.)
template <int RT, int BN, int MODE, int KH, int KW, int PAD, int KC = 64, int KSP = 1, bool HEAD = false, int TPS = 1>
__device__ __forceinline__ void conv_lds_tile(const ConvArgs& a, int tilesX, int tilesY, unsigned char* smem) {
  using C = TileCfg<RT, BN, MODE, KH, KW, PAD, KC, KSP, HEAD, TPS>;
  constexpr int PPP = C::PPP, KS = C::KS, PSH = C::PSH, TH = C::TH, NS = C::NS, TW = C::TW, IW = C::IW, IH = C::IH;
  constexpr int POSB = C::POSB, IROWB = C::IROWB, W1_BYTES = C::W1_BYTES, W_BYTES = C::W_BYTES, BPT = C::BPT, WPT = C::WPT;
  constexpr int NWV = C::NWV, WCOLS = C::WCOLS, IPT = C::IPT, OLD = C::OLD, EPH = C::EPH, NSL = C::NSL, LA = C::LA;
  constexpr int GROUP_BYTES = C::GROUP_BYTES, SRC_H = C::SRC_H, SRC_W = C::SRC_W, SRC_PIECES = C::SRC_PIECES;
  constexpr int SRC_DMA = C::SRC_DMA, MAIN_BYTES = C::MAIN_BYTES, WYOUNG = C::WYOUNG, PF_ST = C::PF_ST;
  constexpr int CG = C::CG, PPJ = C::PPJ, RPJ = C::RPJ, HROWS = C::HROWS, EPJ = C::EPJ;
  constexpr bool FUSED = C::FUSED, SRC = C::SRC, EARLY_RES = C::EARLY_RES;
  const int bid = blockIdx.x, nwg = gridDim.x, nblk_y = blockIdx.y;
  const int grp = KSP == 2 ? (int)(threadIdx.x >> 8) : 0;  // K-split group of this wave
  unsigned char* w_tile = smem + grp * GROUP_BYTES;
  unsigned char* in_tile = w_tile + NSL * W_BYTES;
  unsigned char* src_tile = smem + MAIN_BYTES;  // SRC only

  const int tid = threadIdx.x & 255, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, h = lane >> 5;
  // XCD-aware tile order (cdna_hip_programming.md T1): workgroups are dealt round-robin to
  // the 8 XCDs, so give XCD k the k-th contiguous eighth of the tile list (= a band of image
  // rows): neighbouring tiles then share halo rows through ONE L2 instead of every L2
  // pulling the whole input from the Infinity Cache.  Bijective for any grid size.
  int t = lss_xcd_order(bid, nwg);
  const int tx = t % tilesX; t /= tilesX;
  const int ty = t % tilesY;
  const int b = t / tilesY;
  const int oy0 = ty * TH, ox0 = tx * TW, n0 = nblk_y * BN;
  const int wc = wave % WCOLS, wr = wave / WCOLS;
  const int prow0 = wr * (2 * RT);
  auto stamp = [&](int k) {
    if (a.stamps != nullptr && threadIdx.x == 0)
      a.stamps[((size_t)nblk_y * nwg + bid) * 8 + k] = __builtin_amdgcn_s_memrealtime();
  };
  stamp(0);

  int aoff[RT], boff[2][4];
#pragma unroll
  for (int i = 0; i < RT; ++i) aoff[i] = (prow0 + 2 * i + (r >> 4)) * IROWB + (r & 15) * POSB + h * KC;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int row = wc * 64 + i * 32 + r;
#pragma unroll
    for (int s4 = 0; s4 < KS; ++s4)
      boff[i][s4] = KC == 64 ? row * 128 + (((4 * h + s4) ^ ((row >> 1) & 7)) << 4)
                             : row * 64 + (((2 * h + s4) ^ ((row >> 2) & 3)) << 4);
  }
  f32x16 acc[RT][2];
#pragma unroll
  for (int i = 0; i < RT; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  const unsigned short* wg = reinterpret_cast<const unsigned short*>(a.w);
  const int nchunks = a.Cin / KC / KSP;  // K chunks of this group
  const int cbase = grp * nchunks;        // first chunk of this group
  const int nsteps = nchunks * NS;
  uint4 ireg[IPT];
  // One 1-KiB LDS-DMA block (index i of this wave) of the weight slab of step `st` of chunk `chunk` -> ring slot:
  // lane l of DMA block k lands at byte k*1024 + l*16, i.e. row 8k + (l >> 3), 16-B slot l & 7, which must hold
  // channel piece slot ^ swz(row)
  auto issue_w1 = [&](int st, int chunk, int slot, int i) {  // st = step inside the chunk
    const int blk = i * NWV + wave;
    const int tap = st * TPS + (TPS == 1 ? 0 : blk / BPT), rblk = TPS == 1 ? blk : blk % BPT;
    const int row = KC == 64 ? rblk * 8 + (lane >> 3) : rblk * 16 + (lane >> 2);
    const int part = KC == 64 ? (lane & 7) ^ ((row >> 1) & 7) : (lane & 3) ^ ((row >> 2) & 3);
    const int co = min(n0 + row, a.Cout - 1);  // rows past Cout: any valid address (never stored)
    lss_glds16(wg + ((size_t)tap * a.Cout + co) * a.Cin + (cbase + chunk) * KC + part * 8,
           w_tile + slot * W_BYTES + blk * 1024);
  };
  auto issue_w = [&](int step, int slot) {  // the whole slab of `step`, counted over this group's chunks
#pragma unroll
    for (int i = 0; i < WPT; ++i) issue_w1(step % NS, step / NS, slot, i);
  };
  // MODE 1: the bilinear source coordinates of a patch piece depend only on its position,
  // not on the chunk, so each thread resolves its IPT pieces ONCE (element offset of the
  // top-left corner, +x / +y corner strides, the two blend weights, the skip-tensor
  // offset) and every chunk boundary is then 4 loads + blend + one LDS store per piece.
  // (Recomputing them per chunk cost ~11k cycles per boundary in 64-bit address math -
  // measured: 35 us of the fused up2 conv.)
  // Two VGPRs per piece: g_off = element offset of the top-left corner (a multiple of 8)
  // with flags in its 3 low bits (1: +x corner exists, 2: +y corner exists, 4: inside
  // the image); g_w = the blend weights as 16-bit fixed point (lx | ly << 16).
  int g_off[FUSED ? IPT : 1];
  unsigned int g_w[FUSED ? IPT : 1];
  // SRC: g_off holds the BYTE offset of the top-left corner inside src_tile instead (a multiple of
  // 16, same flags); src_o[i] = element offset of the source pixel this lane's i-th DMA piece copies
  const bool use_src = SRC && a.src_lds != 0;
  const int sy0 = (int)(a.ry * (float)max(oy0 - PAD, 0)), sx0 = (int)(a.rx * (float)max(ox0 - PAD, 0));
  int src_o[SRC ? SRC_DMA : 1];
  if (SRC) {
#pragma unroll
    for (int i = 0; i < SRC_DMA; ++i) {
      const int q = (i * 4 + wave) * 64 + lane;
      const int pos = min(q >> PSH, SRC_H * SRC_W - 1), part = q & (PPP - 1);  // pieces past the patch: any valid pixel
      const int sr = pos / SRC_W, sc = pos - sr * SRC_W;
      src_o[i] = ((b * a.H + min(sy0 + sr, a.H - 1)) * a.W + min(sx0 + sc, a.W - 1)) * a.Cx + part * 8;
    }
  }
  if (FUSED) {
#pragma unroll
    for (int i = 0; i < IPT; ++i) {
      const int q = tid + i * 256;
      g_off[i] = 0; g_w[i] = 0;
      if (q < IH * IW * PPP) {
        const auto [py, px, part] = patch_piece<C>(q);
        const int iy = oy0 - PAD + py, ix = ox0 - PAD + px;
        if (iy >= 0 && iy < a.Hin && ix >= 0 && ix < a.Win) {
          const float sy = a.ry * (float)iy, sx = a.rx * (float)ix;
          const int y0 = (int)sy, x0 = (int)sx;
          const unsigned int wy = (unsigned int)((sy - (float)y0) * 65536.f + 0.5f);
          const unsigned int wx = (unsigned int)((sx - (float)x0) * 65536.f + 0.5f);
          g_w[i] = min(wx, 65535u) | (min(wy, 65535u) << 16);
          const int flags = (x0 < a.W - 1 ? 1 : 0) | (y0 < a.H - 1 ? 2 : 0) | 4;
          if (use_src) g_off[i] = ((((y0 - sy0) * SRC_W + (x0 - sx0)) * PPP + part) * 16) | flags;
          else g_off[i] = (((b * a.H + y0) * a.W + x0) * a.Cx + part * 8) | flags;
        }
      }
    }
  }
  auto gather_fused = [&](int chunk) {
    const unsigned short* xp = reinterpret_cast<const unsigned short*>(a.x);
    const unsigned short* x2p = reinterpret_cast<const unsigned short*>(a.x2);
    const int c0 = (cbase + chunk) * KC;
    const bool skip = c0 < a.C2;  // chunk of the skip tensor x2: plain copy
    const int dxs = a.Cx, dys = a.W * a.Cx;
#pragma unroll 2
    for (int i = 0; i < IPT; ++i) {
      const int q = tid + i * 256;
      if (q >= IH * IW * PPP) continue;
      const auto [py, px, part] = patch_piece<C>(q);
      uint4 v = make_uint4(0, 0, 0, 0);
      if (g_off[i] & 4) {
        if (skip) {
          const int iy = oy0 - PAD + py, ix = ox0 - PAD + px;
          v = *reinterpret_cast<const uint4*>(x2p + ((b * a.Hin + iy) * a.Win + ix) * a.C2 + c0 + part * 8);
        } else if (use_src) {  // corners from the LDS source window: byte strides
          v = blend_corners(src_tile + (g_off[i] & ~15), (g_off[i] & 1) ? PPP * 16 : 0,
                            (g_off[i] & 2) ? SRC_W * PPP * 16 : 0, g_w[i]);
        } else {  // corners from global memory: element strides
          v = blend_corners(xp + (g_off[i] & ~7) + (c0 - a.C2), (g_off[i] & 1) ? dxs : 0, (g_off[i] & 2) ? dys : 0, g_w[i]);
        }
      }
      *reinterpret_cast<uint4*>(in_tile + py * IROWB + px * POSB + part * 16) = v;
    }
  };
  // SRC: source pixels of `chunk` -> src_tile (lane l of DMA block k lands at byte k*1024 + l*16)
  auto issue_src = [&](int chunk) {
    const unsigned short* xp = reinterpret_cast<const unsigned short*>(a.x);
    const int cx = (cbase + chunk) * KC - a.C2;
#pragma unroll
    for (int i = 0; i < (SRC ? SRC_DMA : 0); ++i)
      if (i * 4 + wave < SRC_PIECES) lss_glds16(xp + src_o[i] + cx, src_tile + (i * 4 + wave) * 1024);
  };
  // does `chunk` read the upsampled tensor through src_tile?
  auto src_chunk = [&](int chunk) { return use_src && chunk < nchunks && (cbase + chunk) * KC >= a.C2; };

  // input patch of one 64-channel chunk of a plain (or phase-plane) input: 16-B loads, unrolled so they can be parked
  // in registers (prefetch)
  auto gather_in = [&](int chunk, bool to_lds) {
#pragma unroll
    for (int i = 0; i < IPT; ++i) {
      const int q = tid + i * 256;
      uint4 v = make_uint4(0, 0, 0, 0);
      if (q < IH * IW * PPP) {
        const auto [py, px, part] = patch_piece<C>(q);
        int iy = oy0 - PAD + py, ix = ox0 - PAD + px, cc = cbase + chunk;
        if (MODE == 2) {  // (iy, ix) are phase-plane coordinates; chunk -> (phase, channel block)
          const int nblk = a.Cx / KC;
          const int ph = cc / nblk;
          cc = cc - ph * nblk;
          iy = 2 * iy + (ph >> 1);
          ix = 2 * ix + (ph & 1);
        }
        if (iy >= 0 && iy < a.Hin && ix >= 0 && ix < a.Win)
          v = load_in_piece<unsigned short, false>(a, b, iy, ix, cc * KC + part * 8);
        if (to_lds) *reinterpret_cast<uint4*>(in_tile + py * IROWB + px * POSB + part * 16) = v;
      }
      if (!to_lds) ireg[i] = v;
    }
  };
  auto store_in = [&]() {
#pragma unroll
    for (int i = 0; i < IPT; ++i) {
      const int q = tid + i * 256;
      if (q < IH * IW * PPP) {
        const auto [py, px, part] = patch_piece<C>(q);
        *reinterpret_cast<uint4*>(in_tile + py * IROWB + px * POSB + part * 16) = ireg[i];
      }
    }
  };

  // per-lane epilogue constants, fetched now so their latency is long gone by the epilogue
  float esc[2], esh[2];
#pragma unroll
  for (int ct = 0; ct < 2; ++ct) {
    const int co = n0 + wc * 64 + ct * 32 + r;
    const bool cok = co < a.Cout;
    esc[ct] = (cok && a.scale) ? a.scale[co] : 1.f;
    esh[ct] = (cok && a.shift) ? a.shift[co] : 0.f;
  }

  // Output pieces of this thread (TileCfg::CG), used by the epilogue; computed here because the residual rows of the
  // launch-bound layers are requested from inside the main loop, see EARLY_RES.
  const int pix0 = tid / CG, c8 = tid % CG;
  const int ox = ox0 + (pix0 & 15), oyb = oy0 + (pix0 >> 4);
  const int co = n0 + c8 * 8;
  const bool col_ok = grp == 0 && ox < a.Wo && co < a.Cout;
  const size_t pixb = ((size_t)b * a.Ho + oyb) * a.Wo + ox;  // pixel index of pass 0 of half 0
  const int rstep = a.Wo * a.Cout;                            // residual elements per image row
  const unsigned short* res = reinterpret_cast<const unsigned short*>(a.residual);
  const bool res_vec = !HEAD && res != nullptr && col_ok && (a.Cout & 7) == 0 && co + 8 <= a.Cout;
  uint4 rres[HEAD ? 1 : EPJ];
  auto load_residual = [&](int half) {
    if (!HEAD) {
      const unsigned short* rb = res + pixb * a.Cout + co;
#pragma unroll
      for (int j = 0; j < EPJ; ++j) {
        const int row = half * HROWS + j * RPJ;
        rres[j] = make_uint4(0, 0, 0, 0);
        if (res_vec && oyb + row < a.Ho) rres[j] = *reinterpret_cast<const uint4*>(rb + row * rstep);
      }
    }
  };

  // prologue: W(0), W(1) on their way; patch of chunk 0
  if (src_chunk(0)) issue_src(0);
  issue_w(0, 0);
#pragma unroll
  for (int q = 1; q < LA; ++q)
    if (nsteps > q) issue_w(q, q);
  if (src_chunk(0)) {
    lss_wait_vmcnt<0>();
    lss_lds_barrier();  // the source pixels of chunk 0 are in LDS for every wave
  }
  if (FUSED) gather_fused(0);
  else gather_in(0, true);
  lss_wait_vmcnt<0>();
  lss_lds_barrier();
  stamp(1);

  // Main loop.  The NT taps of a chunk are fully unrolled (static patch offsets and
  // fragment double buffer); the ring slot advances at run time.  Rolling prefetch:
  // while the 4 MFMAs of one k-step run, the 2 A + 2 B fragments of the NEXT k-step
  // are already in flight (32 fragment VGPRs in total), and one DMA block of the slab
  // two steps ahead is issued per k-step, so LDS latency and DMA issue hide behind
  // MFMAs.
  bf16x8 fa[2][RT], fb[2][2];  // [k-step parity][tile]
  auto read_a = [&](int buf, int tap, int s4) {
    const int toff = (tap / KW) * IROWB + (tap % KW) * POSB + s4 * 16;
#pragma unroll
    for (int i = 0; i < RT; ++i) fa[buf][i] = *reinterpret_cast<const bf16x8*>(in_tile + aoff[i] + toff);
  };
  auto read_b = [&](int buf, int slot, int ks) {  // ks = k-step inside the step: tap ks / KS of the slab
    const unsigned char* wbuf = w_tile + slot * W_BYTES + (ks / KS) * W1_BYTES;
    fb[buf][0] = *reinterpret_cast<const bf16x8*>(wbuf + boff[0][ks % KS]);
    fb[buf][1] = *reinterpret_cast<const bf16x8*>(wbuf + boff[1][ks % KS]);
  };
  int slot = 0;  // ring slot of the current step's slab
  for (int chunk = 0; chunk < nchunks; ++chunk) {
    const bool last_chunk = chunk + 1 == nchunks;
    const bool srcq = src_chunk(chunk + 1);  // this chunk's tap 0 also sends the next chunk's source pixels
    if (EARLY_RES && last_chunk) load_residual(0);  // (younger than every DMA piece the counted waits below name)
    read_a(0, 0, 0);
    read_b(0, slot, 0);
#pragma unroll
    for (int st = 0; st < NS; ++st) {
      // slab LA steps ahead: step st+LA of this chunk, or st+LA-NS of the next one
      const int t2 = (st + LA) % NS;
      const int c2 = chunk + (st + LA) / NS;
      const bool more = c2 < nchunks;
      const bool prefetch = !FUSED && st == PF_ST && !last_chunk;
      const int slot2 = slot >= 1 ? slot - 1 : NSL - 1;  // (slot + LA) % NSL
#pragma unroll
      for (int ks = 0; ks < KS * TPS; ++ks) {
        const int cur = ks & 1, nxt = cur ^ 1;
        if (ks < KS * TPS - 1) {
          read_a(nxt, st * TPS + (ks + 1) / KS, (ks + 1) % KS);
          read_b(nxt, slot, ks + 1);
        } else if (st < NS - 1) {
          read_a(nxt, (st + 1) * TPS, 0);  // next step's weights are only readable after the barrier
        }
        // keep the prefetch reads AHEAD of this k-step's MFMAs (hipcc's scheduler would
        // otherwise sink them next to their use and expose the LDS latency again)
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < RT; ++i) {
          acc[i][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[cur][i], fb[cur][0], acc[i][0], 0, 0, 0);
          acc[i][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[cur][i], fb[cur][1], acc[i][1], 0, 0, 0);
        }
        if (more && ks < WPT) issue_w1(t2, c2, slot2, ks);
      }
      // after this step's weight pieces, so that (like them) the copies have two steps to land: the
      // counted waits of step 0 and step 1 leave them in flight, the wait of step 2 retires them
      if (SRC && st == 0 && srcq) issue_src(chunk + 1);
      if (prefetch) gather_in(chunk + 1, false);  // next patch -> registers
      if (st == NS - 1 && !last_chunk) {
        lss_lds_barrier();  // every wave is done with this chunk's patch
        if (FUSED) gather_fused(chunk + 1);
        else store_in();
      }
      // W(step+1) must have landed in every wave's share before anyone reads it; only the
      // DMA (and patch loads) issued during THIS step may stay in flight
      // (younger than W(step+1): the slabs of steps step+2 .. step+LA, and - in steps 0 .. LA-1 of a chunk - the source
      // copies issued in its step 0: one per wave, two for the waves that carry the pieces past the fourth)
      if (prefetch) lss_wait_vmcnt<WYOUNG + IPT>();
      else if (SRC && st < LA && srcq && more) {
        if (SRC_DMA == 2 && wave + 4 < SRC_PIECES) lss_wait_vmcnt<WYOUNG + 2>();
        else lss_wait_vmcnt<WYOUNG + (SRC_DMA >= 1 ? 1 : 0)>();
      }
      else if (more) lss_wait_vmcnt<WYOUNG>();
      else lss_wait_vmcnt<0>();
      lss_lds_barrier();
      slot = slot == NSL - 1 ? 0 : slot + 1;
      if (st < NS - 1) read_b(0, slot, 0);
    }
  }

  // epilogue.  D[row = (i&3) + 8*(i>>2) + 4*h][col = r]: a lane holds ONE output
  // channel of 16 pixels, so storing from registers would be 2-B scattered stores.
  // Instead: scale/shift in registers -> fp32 tile in LDS (the ring + patch area is
  // free now) -> every thread picks up 8 consecutive channels of a pixel, adds the
  // residual (one 16-B load), ReLU, rounds to bf16 once, and stores 16 B.
  float* otile = reinterpret_cast<float*>(smem);
  stamp(2);
  // (the loop's final lss_lds_barrier already guarantees every wave is done reading LDS)
  if (KSP == 2) {
    // split-K: the second group's partial sums meet the first group's through LDS (same lane ->
    // same element in both groups, so only the group hand-over needs barriers)
    auto part_at = [&](int ct, int rt, int i) -> float& {  // where accumulator (ct, rt, i) of this lane meets its twin
      const int row = (i & 3) + 8 * (i >> 2) + 4 * h;
      return otile[((prow0 + 2 * rt + (row >> 4)) * 16 + (row & 15)) * OLD + wc * 64 + ct * 32 + r];
    };
#pragma unroll
    for (int g = 1; g >= 0; --g) {  // group 1 writes, then group 0 adds
      if (grp == g) {
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
          for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
              if (g == 1) part_at(ct, rt, i) = acc[rt][ct][i];
              else acc[rt][ct][i] += part_at(ct, rt, i);
            }
      }
      lss_lds_barrier();  // g == 0: the partials are consumed before group 0 restages the tile below
    }
  }
  // (the epilogue of the launch-bound layers is instruction-issue time, not bandwidth)
  // dual-output launches: this workgroup's channel block belongs to y (columns [0, split)) or y2
  const bool second = a.y2 != nullptr && n0 >= a.split;
  const int ycol0 = second ? a.split : 0;                                   // first channel of the tensor
  const int ycw = a.y2 == nullptr ? a.Cout : (second ? a.Cout - a.split : a.split);  // its channel count
  const int eact = n0 < a.relu_n ? a.relu : 0;
  const bool vec_ok = (ycw & 7) == 0 && co + 8 <= a.Cout;  // 16-B aligned, whole channel group
  const int ystep = a.Wo * ycw;                               // output elements per image row
  // residual rows of ONE staged half: requested at the top of the half's iteration, before its accumulators are
  // staged, so the loads fly during the LDS write / barrier / read-back instead of stalling the store loop.  (Per
  // half, not for the whole tile: 16 instead of 32 live registers in the 168-register KC = 32 kernels.)  The RT = 1
  // kernels have requested them inside the main loop already (EARLY_RES).
  unsigned short* y = reinterpret_cast<unsigned short*>(second ? a.y2 : a.y);
  const size_t obase = pixb * ycw + (co - ycol0);
  const __amdgpu_buffer_rsrc_t yrsrc =
      __builtin_amdgcn_make_buffer_rsrc(y, 0, a.wt ? (int)((size_t)a.M * ycw * 2) : 0, 0x00020000);
  // staging address of this lane: D[row = (i&3) + 8*(i>>2) + 4*h][col = r], and (i&3) + 4*h < 16, so
  // pixel = (2*rt + (i>>3))*16 + (i&3) + 8*((i>>2)&1) + 4*h: lane part + compile-time part
  float* const ost = otile + (prow0 * 16 + 4 * h) * OLD + wc * 64 + r;
#pragma unroll
  for (int half = 0; half < EPH; ++half) {
    const bool mine = grp == 0 && (EPH == 1 || (prow0 / HROWS) == half);  // this wave's rows belong to the half
    if (!EARLY_RES) load_residual(half);
    if (mine) {
#pragma unroll
      for (int ct = 0; ct < 2; ++ct) {
        const float sc = esc[ct], sh = esh[ct];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            const int pc = (2 * rt + (i >> 3)) * 16 + (i & 3) + 8 * ((i >> 2) & 1) - half * HROWS * 16;
            ost[pc * OLD + ct * 32] = acc[rt][ct][i] * sc + sh;
          }
      }
      if (!HEAD && a.stats) {
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {
          const int cs = n0 + wc * 64 + ct * 32 + r;
          const bool cok = cs < a.Cout;
          float s1 = 0.f, s2 = 0.f;
#pragma unroll
          for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
              const int row = (i & 3) + 8 * (i >> 2) + 4 * h;
              const int sy = oy0 + prow0 + 2 * rt + (row >> 4), sx = ox0 + (row & 15);
              if (cok && sy < a.Ho && sx < a.Wo) {
                const float raw = acc[rt][ct][i];
                s1 += raw;
                s2 += raw * raw;
              }
            }
          bn_stats_add(a.stats, a.Cout, cs, h, cok, s1, s2);
        }
      }
    }
    lss_lds_barrier();
    if (half == 0) stamp(3);
    if (grp != 0) {
      // second K-split group: its sums were handed over above; it only keeps the barriers company
    } else if (HEAD && a.head_n <= 16) {
      head_mfma<C>(a, otile, b, oy0 + half * HROWS, ox0, lane, wave);
    } else if (HEAD) {
      head_valu<C>(a, otile, b, oy0 + half * HROWS, ox0, tid);
    } else if (col_ok) {
      const float* const ord = otile + pix0 * OLD + c8 * 8;
#pragma unroll
      for (int j = 0; j < EPJ; ++j) {
        const int row = half * HROWS + j * RPJ;  // image row of this pass relative to oyb
        if (oyb + row >= a.Ho) continue;
        const f32x4 v0 = *reinterpret_cast<const f32x4*>(ord + j * PPJ * OLD);
        const f32x4 v1 = *reinterpret_cast<const f32x4*>(ord + j * PPJ * OLD + 4);
        float v[8] = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
        const size_t o = obase + (size_t)(row * ystep);
        if (vec_ok) {
          if (res_vec) {
            const uint4 rv = rres[j];
            const unsigned int ru[4] = {rv.x, rv.y, rv.z, rv.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              v[2 * k] += lss_bf2f((unsigned short)(ru[k] & 0xffff));
              v[2 * k + 1] += lss_bf2f((unsigned short)(ru[k] >> 16));
            }
          } else if (res) {
            const unsigned short* rp = res + (pixb * a.Cout + co) + (size_t)(row * rstep);
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] += lss_bf2f(rp[k]);
          }
          if (eact == 1) {
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = fmaxf(v[k], 0.f);
          } else if (eact == 2) {
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = conv_act(v[k], 2);
          }
          if (a.out_f32) {
            float* yf = reinterpret_cast<float*>(second ? a.y2 : a.y) + o;
            *reinterpret_cast<f32x4*>(yf) = (f32x4){v[0], v[1], v[2], v[3]};
            *reinterpret_cast<f32x4*>(yf + 4) = (f32x4){v[4], v[5], v[6], v[7]};
          } else {
            uint4 ov;
            ov.x = lss_pack_bf2(v[0], v[1]); ov.y = lss_pack_bf2(v[2], v[3]);
            ov.z = lss_pack_bf2(v[4], v[5]); ov.w = lss_pack_bf2(v[6], v[7]);
            if (a.wt) {
              // write-through (sc1) 16-B store: a dependent kernel boundary otherwise pays
              // (dirty bytes / 6 TB/s) for the L2 write-back (MI355X_MICROARCH.md, row 'boundary')
              __builtin_amdgcn_raw_buffer_store_b128((u32x4){ov.x, ov.y, ov.z, ov.w}, yrsrc, (int)(o * 2), 0, 16);
            } else {
              *reinterpret_cast<uint4*>(y + o) = ov;
            }
          }
        } else {
          // ragged channel counts: element by element
          const size_t ro = (pixb * a.Cout + co) + (size_t)(row * rstep);
          for (int k = 0; k < 8 && co + k < a.Cout; ++k) {
            float t = v[k];
            if (res) t += lss_bf2f(res[ro + k]);
            t = conv_act(t, eact);
            if (a.out_f32) reinterpret_cast<float*>(second ? a.y2 : a.y)[o + k] = t;
            else y[o + k] = lss_f2bf(t);
          }
        }
      }
    }
    if (half + 1 < EPH) lss_lds_barrier();  // everyone has read this half before the next one is staged
  }
  if (a.stamps != nullptr) {
    stamp(4);
    lss_wait_vmcnt<0>();  // stores acknowledged
    stamp(5);
  }
}

template <int RT, int BN, int MODE, int KH, int KW, int PAD, int KC = 64, int KSP = 1, bool HEAD = false, int TPS = 1>
__global__ __launch_bounds__(256 * KSP, KSP == 2 ? 1 : (KC == 32 ? 3 : 2)) void conv_lds_kernel(ConvArgs a, int tilesX,
                                                                                                  int tilesY) {
  __shared__ __attribute__((aligned(1024))) unsigned char smem[TileCfg<RT, BN, MODE, KH, KW, PAD, KC, KSP, HEAD, TPS>::SMEM_BYTES];
  conv_lds_tile<RT, BN, MODE, KH, KW, PAD, KC, KSP, HEAD, TPS>(a, tilesX, tilesY, smem);
}

// OIHW fp32 -> [tap][co][ci] in T
template <typename T>
__global__ void pack_weights_kernel(const float* __restrict__ w, int Cout, int Cin, int KHW,
                                    T* __restrict__ out) {
  const size_t n = (size_t)Cout * Cin * KHW;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (size_t)gridDim.x * 256) {
    const int ci = e % Cin;
    const size_t t = e / Cin;
    const int co = t % Cout;
    const int tap = t / Cout;
    const float v = w[((size_t)co * Cin + ci) * KHW + tap];
    if (sizeof(T) == 2) reinterpret_cast<unsigned short*>(out)[e] = lss_f2bf(v);
    else reinterpret_cast<float*>(out)[e] = v;
  }
}

// OIHW fp32 (k x k, stride 2, pad p) -> [tap'][co][phase*Cin + ci] bf16 of the
// equivalent stride-1 conv over the 4 parity phases: input row 2*oy + ky - p =
// 2*(oy + ty) + py with py = (ky - p) & 1, ty = (ky - p - py) / 2.
__global__ void pack_weights_s2d_kernel(const float* __restrict__ w, int Cout, int Cin, int K, int pad,
                                        int KT, int tmin, unsigned short* __restrict__ out) {
  const size_t n = (size_t)KT * KT * Cout * 4 * Cin;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (size_t)gridDim.x * 256) {
    const int ci = e % Cin;
    size_t t = e / Cin;
    const int ph = t % 4; t /= 4;
    const int co = t % Cout; t /= Cout;
    const int tx = t % KT, ty = t / KT;
    const int ky = 2 * (ty + tmin) + (ph >> 1) + pad, kx = 2 * (tx + tmin) + (ph & 1) + pad;
    float v = 0.f;
    if (ky >= 0 && ky < K && kx >= 0 && kx < K) v = w[(((size_t)co * Cin + ci) * K + ky) * K + kx];
    out[e] = lss_f2bf(v);
  }
}

// floor((0 - p) / 2) .. floor((k - 1 - p) / 2): tap range of the phase-plane conv
inline int s2d_tmin(int pad) { return -((pad + 1) / 2); }
inline int s2d_taps(int K, int pad) {
  const int hi = (K - 1 - pad) >= 0 ? (K - 1 - pad) / 2 : -((pad - K + 2) / 2);
  return hi - s2d_tmin(pad) + 1;
}

// May the KC = 32 fused kernel stage its low-res source pixels in LDS?  Its 10 x 18 patch must map
// into the SRC_H x SRC_W = 7 x 11 source window: floor(9 ry) + 2 <= 7 and floor(17 rx) + 2 <= 11.
inline int conv_src_lds_ok(const ConvArgs& a) {
  if (!lss_env_on("LSS_CONV_SRC")) return 0;
  return a.up >= 2 && a.ry * 9.f < 4.99f && a.rx * 17.f < 8.99f;
}

// Which conv_lds_kernel a conv takes and on what grid: decided here for launch_conv_lds and for the fused head (whose
// tile is always RT = 2).  BN = 64 for narrow layers, else 128; RT = 2 (throughput shape) unless that grid would leave
// the 256 CUs under-filled, in which case half-height workgroups (RT = 1) shorten the per-workgroup critical path
// instead.  Every switch is read on every call.
struct TilePlan {
  int rt, kc, ksp, tps, src_lds;
  int tilesX, tilesY;
  dim3 grid;
};
TilePlan conv_tile_plan(const ConvArgs& a, int MODE, int KH, bool head) {
  TilePlan p = {2, 64, 1, 1, 0};
  const bool narrow = a.Cout <= 64;
  const int th2 = narrow ? 16 : 8;
  const int nblk = lss_cdiv(a.Cout, narrow ? 64 : 128);
  p.tilesX = lss_cdiv(a.Wo, 16);
  if (!head) {
    const long long nwg2 = (long long)p.tilesX * lss_cdiv(a.Ho, th2) * a.B * nblk;
    p.rt = nwg2 < 384 ? 1 : 2;
    if (const char* e = getenv("LSS_CONV_RT")) p.rt = atoi(e) == 1 ? 1 : 2;
  }
  p.tilesY = lss_cdiv(a.Ho, p.rt == 2 ? th2 : th2 / 2);
  p.grid = dim3(p.tilesX * p.tilesY * a.B, nblk);
  if (narrow) {
    if (p.rt == 1 && MODE == 2 && KH == 4) p.tps = 2;  // the 7x7 / 2 stem: two taps per step
    return p;
  }
  // Half-depth steps, three workgroups per CU.  Measured (same box, B = 4): the fused
  // upsample/concat convs gain (up1.conv0 100 -> 83 us, up2.1 141 -> 133 us: the third workgroup
  // fills the synchronous gather phases), the plain 3x3 loses 5 % (half-depth steps double the
  // barriers per MFMA) - so MODE 1 takes KC = 32 by default, MODE 0 keeps 64.  LSS_CONV_KC overrides; the head has
  // no plain KC = 32 form, so there the switch can only take KC = 32 away.
  bool kc32 = MODE == 1;
  if (const char* e = getenv("LSS_CONV_KC")) kc32 = (kc32 || !head) && atoi(e) == 32;
  if (kc32 && MODE != 2 && KH == 3 && p.rt == 2 && a.Cx % 32 == 0 && a.C2 % 32 == 0) {
    p.kc = 32;
    p.src_lds = MODE == 1 ? conv_src_lds_ok(a) : 0;
  } else if (p.rt == 1) {
    // Grids that cannot even give every CU one workgroup (layer2 / layer3 at batch 4): split the
    // K loop over two 4-wave groups inside the workgroup - half the latency-bound steps each.
    const long long nwg1 = (long long)p.grid.x * p.grid.y;
    const bool ksplit = MODE != 1 && nwg1 <= 256 && (a.Cin / 64) % 2 == 0 && a.Cin >= 128;
    if (ksplit && lss_env_on("LSS_CONV_KSPLIT")) p.ksp = 2;
  }
  return p;
}

template <int RT, int BN, int MODE, int KH, int KW, int PAD, int KC = 64, int KSP = 1, bool HEAD = false, int TPS = 1>
void launch_tile(ConvArgs a, const TilePlan& p, hipStream_t st) {
  a.src_lds = p.src_lds;
  hipLaunchKernelGGL((conv_lds_kernel<RT, BN, MODE, KH, KW, PAD, KC, KSP, HEAD, TPS>), p.grid, dim3(256 * KSP), 0, st, a,
                     p.tilesX, p.tilesY);
}

// the plan's instantiation, among those this (MODE, taps) has
template <int MODE, int KH, int KW, int PAD>
void launch_conv_lds(const ConvArgs& a, hipStream_t st) {
  const TilePlan p = conv_tile_plan(a, MODE, KH, false);
  if (a.Cout <= 64) {
    if constexpr (MODE == 2 && KH == 4) {
      if (p.tps == 2) return launch_tile<1, 64, MODE, KH, KW, PAD, 64, 1, false, 2>(a, p, st);
    } else if (p.rt == 1) {
      return launch_tile<1, 64, MODE, KH, KW, PAD>(a, p, st);
    }
    return launch_tile<2, 64, MODE, KH, KW, PAD>(a, p, st);
  }
  if constexpr (MODE != 2 && KH == 3) {
    if (p.kc == 32) return launch_tile<2, 128, MODE, KH, KW, PAD, 32>(a, p, st);
  }
  if constexpr (MODE != 1) {
    if (p.ksp == 2) return launch_tile<1, 128, MODE, KH, KW, PAD, 64, 2>(a, p, st);
  }
  if (p.rt == 2) launch_tile<2, 128, MODE, KH, KW, PAD>(a, p, st);
  else launch_tile<1, 128, MODE, KH, KW, PAD>(a, p, st);
}

// LSS_CONV_WT=0: write-back epilogue stores.  Read on every call, like every switch here: tests flip them in-process
inline bool conv_wt_from_env() { return lss_env_on("LSS_CONV_WT"); }

// The one fill of ConvArgs: geometry, activation word (`act` = ACT_* | LSS_OUT_F32), write-through, align_corners
// ratios.  An entry checks its own arguments, calls this, then sets what only it has.  rc: 0 or LSS_E_SHAPE (no
// output pixel, or 2^31 and more of them).
struct ConvFill {
  int rc;
  ConvArgs a;
};
ConvFill conv_args_fill(const void* x, const void* x2, const void* w, const float* scale, const float* shift,
                        const void* residual, void* y, float* stats, int B, int H, int W, int Cx, int C2, int up,
                        int Cout, int KH, int KW, int stride, int pad, int act) {
  ConvFill f = {};  // zero: one output (y2, split), no fused head (head_*), no LDS source staging (src_lds)
  f.rc = LSS_E_SHAPE;
  ConvArgs& a = f.a;
  a.stamps = lss_env_device_ptr("LSS_CONV_STAMPS");  // u64 buffer, 8 entries per workgroup: switches the phase stamps on
  a.x = x; a.x2 = x2; a.w = w; a.scale = scale; a.shift = shift; a.residual = residual;
  a.y = y; a.stats = stats;
  a.B = B; a.H = H; a.W = W; a.Cx = Cx; a.C2 = C2; a.up = up;
  a.Hin = H * up; a.Win = W * up; a.Cin = Cx + C2;
  a.Cout = Cout; a.KH = KH; a.KW = KW; a.stride = stride; a.pad = pad;
  a.Ho = (a.Hin + 2 * pad - KH) / stride + 1;
  a.Wo = (a.Win + 2 * pad - KW) / stride + 1;
  if (a.Ho <= 0 || a.Wo <= 0) return f;
  const long long M = (long long)B * a.Ho * a.Wo;
  if (M >= (1LL << 31)) return f;
  a.M = (int)M;
  a.relu = act & 3;
  a.out_f32 = (act & LSS_OUT_F32) != 0;
  a.wt = conv_wt_from_env() && (unsigned long long)a.M * a.Cout * 2 < (1ULL << 31);
  a.relu_n = a.Cout;
  // read by the fused-gather (MODE 1) code only; 1 where up == 1
  a.ry = a.Hin > 1 ? (float)(H - 1) / (float)(a.Hin - 1) : 0.f;
  a.rx = a.Win > 1 ? (float)(W - 1) / (float)(a.Win - 1) : 0.f;
  f.rc = 0;
  return f;
}

}  // namespace

extern "C" size_t lss_conv2d_s2d_packed_weight_bytes(int Cout, int Cin, int K, int pad) {
  if (Cout <= 0 || Cin <= 0 || K <= 0 || pad < 0) return 0;
  const int kt = s2d_taps(K, pad);
  return (size_t)kt * kt * Cout * 4 * Cin * 2;
}

extern "C" int lss_conv2d_pack_weights_s2d(const float* w_oihw, int Cout, int Cin, int K, int pad,
                                           void* w_packed, void* stream) {
  LSS_CHECK_PTR(w_oihw); LSS_CHECK_PTR(w_packed);
  LSS_CHECK_POS(Cout); LSS_CHECK_POS(Cin); LSS_CHECK_POS(K);
  if (pad < 0) return LSS_E_SHAPE;
  const int kt = s2d_taps(K, pad);
  const size_t n = (size_t)kt * kt * Cout * 4 * Cin;
  const int grid = (int)((n + 255) / 256 > 4096 ? 4096 : (n + 255) / 256);
  hipLaunchKernelGGL(pack_weights_s2d_kernel, dim3(grid), dim3(256), 0, lss_stream(stream), w_oihw, Cout,
                     Cin, K, pad, kt, s2d_tmin(pad), reinterpret_cast<unsigned short*>(w_packed));
  return lss_launch_status();
}

extern "C" size_t lss_conv2d_packed_weight_bytes(int Cout, int Cin, int KH, int KW, int dt) {
  if (Cout <= 0 || Cin <= 0 || KH <= 0 || KW <= 0) return 0;
  return (size_t)Cout * Cin * KH * KW * (dt == LSS_DT_BF16 ? 2 : 4);
}

extern "C" int lss_conv2d_pack_weights(const float* w_oihw, int Cout, int Cin, int KH, int KW,
                                       int dt, void* w_packed, void* stream) {
  LSS_CHECK_PTR(w_oihw); LSS_CHECK_PTR(w_packed);
  LSS_CHECK_POS(Cout); LSS_CHECK_POS(Cin); LSS_CHECK_POS(KH); LSS_CHECK_POS(KW);
  const size_t n = (size_t)Cout * Cin * KH * KW;
  const int grid = (int)((n + 255) / 256 > 4096 ? 4096 : (n + 255) / 256);
  if (dt == LSS_DT_BF16)
    hipLaunchKernelGGL(pack_weights_kernel<unsigned short>, dim3(grid), dim3(256), 0,
                       lss_stream(stream), w_oihw, Cout, Cin, KH * KW,
                       reinterpret_cast<unsigned short*>(w_packed));
  else if (dt == LSS_DT_F32)
    hipLaunchKernelGGL(pack_weights_kernel<float>, dim3(grid), dim3(256), 0, lss_stream(stream),
                       w_oihw, Cout, Cin, KH * KW, reinterpret_cast<float*>(w_packed));
  else
    return LSS_E_LAYOUT;
  return lss_launch_status();
}

extern "C" int lss_conv2d_fwd(const void* x, const void* x2, const void* w_packed,
                              const float* scale, const float* shift, const void* residual,
                              void* y, float* stats, int B, int H, int W, int Cx, int C2, int up,
                              int Cout, int KH, int KW, int stride, int pad, int relu, int dt,
                              void* stream) {
  LSS_CHECK_PTR(x); LSS_CHECK_PTR(w_packed); LSS_CHECK_PTR(y);
  LSS_CHECK_POS(B); LSS_CHECK_POS(H); LSS_CHECK_POS(W); LSS_CHECK_POS(Cx); LSS_CHECK_POS(Cout);
  LSS_CHECK_POS(KH); LSS_CHECK_POS(KW); LSS_CHECK_POS(stride); LSS_CHECK_POS(up);
  if (pad < 0 || C2 < 0) return LSS_E_SHAPE;
  if (dt != LSS_DT_F32 && dt != LSS_DT_BF16) return LSS_E_LAYOUT;
  if (C2 > 0 && x2 == nullptr) return LSS_E_NULL;
  if (relu & LSS_W_KS) {  // KS-packed weights: the K-split one-pass kernel of the launch-bound layers, or nothing
    if (dt != LSS_DT_BF16 || KH != 3 || KW != 3 || stride != 1 || pad != 1 || stats != nullptr || C2 != 0 || up != 1 ||
        (relu & ~(LSS_W_KS | 1)) != 0)
      return LSS_E_SHAPE;
    // write-back stores here (LSS_KS_WT=1: write-through like the other kernels): 5 MB of output per launch at most,
    // read back by the next launch - measured in a dependent chain 9.47 / 8.22 / 7.48 -> 9.07 / 8.11 / 7.36 us per launch
    const bool wt_ks = lss_env_set_on("LSS_KS_WT");
    return lss_conv_ks_launch(x, w_packed, scale, shift, residual, y, B, H, W, Cx, Cout, relu & 1, wt_ks ? 1 : 0,
                              lss_stream(stream));
  }
  if (relu & LSS_W_RING) {  // ring-packed weights: the loader / consumer kernel, or nothing
    if (dt != LSS_DT_BF16 || KH != 3 || KW != 3 || stride != 1 || pad != 1 || residual != nullptr || stats != nullptr ||
        (relu & ~(LSS_W_RING | 1)) != 0)
      return LSS_E_SHAPE;
    return lss_conv_ring_launch(x, x2, w_packed, scale, shift, y, nullptr, nullptr, nullptr, 0, B, H, W, Cx, C2, up, Cout,
                                relu & 1, conv_wt_from_env() ? 1 : 0, lss_stream(stream));
  }
  // K blocks never straddle the x2 | upsample(x) boundary.  A plain bf16 input may end in half a K block
  // (Cin % 64 == 32): the GEMM kernel of the 1x1 layers stages 32-channel slabs, and the direct kernel leaves the
  // missing half of its last block at zero
  const bool fused = (up > 1) || (C2 > 0);
  const int kblock = dt == LSS_DT_BF16 ? (fused ? 64 : 32) : 8;
  if (Cx % kblock != 0 || C2 % kblock != 0) return LSS_E_SHAPE;
  const ConvFill f = conv_args_fill(x, x2, w_packed, scale, shift, residual, y, stats, B, H, W, Cx, C2, up, Cout, KH, KW,
                                    stride, pad, relu);
  if (f.rc != 0) return f.rc;
  const ConvArgs& a = f.a;
  const long long M = a.M;
  const bool head_major = (relu & LSS_OUT_HEAD_MAJOR32) != 0;
  if (a.relu == 3 || (relu & ~(3 | LSS_OUT_F32 | LSS_OUT_HEAD_MAJOR32)) != 0) return LSS_E_LAYOUT;
  dim3 grid(lss_cdiv(M, 128), lss_cdiv(Cout, 64));
  if (grid.y > 65535) return LSS_E_SHAPE;
  hipStream_t st = lss_stream(stream);
  if (dt == LSS_DT_BF16 && KH == 3 && KW == 3 && stride == 1 && pad == 1 && a.Cin % 64 == 0 &&
      getenv("LSS_CONV_DIRECT") == nullptr) {
    if (fused) launch_conv_lds<1, 3, 3, 1>(a, st);
    else launch_conv_lds<0, 3, 3, 1>(a, st);
    return lss_launch_status();
  }
  // 2x2 / pad 1 and 4x4 / pad 2, stride 1: the data gradients of the 3x3 / 2 and 7x7 / 2 convs over phase planes
  // (lss_conv2d_pack_weights_s2_dgrad) - same tile kernel, other tap counts
  if (dt == LSS_DT_BF16 && stride == 1 && !fused && KH == KW && a.Cin % 64 == 0 && a.stats == nullptr &&
      ((KH == 2 && pad == 1) || (KH == 4 && pad == 2)) && getenv("LSS_CONV_DIRECT") == nullptr) {
    if (KH == 2) launch_conv_lds<0, 2, 2, 1>(a, st);
    else launch_conv_lds<0, 4, 4, 2>(a, st);
    return lss_launch_status();
  }
  // 1x1 / stride 1: the token-major linear layers of the BEV transformer and the 1x1 convs
  // a 1x1 / stride-1 conv over NHWC is a row-major GEMM over the B*H*W pixel rows
  // (linear_mfma.hip): the token-major linear layers of the BEV transformer and the 1x1
  // convs around it.  Narrow outputs (the 4-class heads: a 128-wide tile would be 97 % padding)
  // and the BN-statistics variant stay on the direct kernel below.
  if (dt == LSS_DT_BF16 && KH == 1 && KW == 1 && stride == 1 && pad == 0 && !fused && a.Cin % 32 == 0 &&
      a.Cout >= 64 && a.stats == nullptr && getenv("LSS_CONV_DIRECT") == nullptr)
    return lss_linear_bf16_launch(x, w_packed, scale, shift, residual, y, M, Cout, a.Cin, a.relu, a.out_f32,
                                  head_major ? a.Ho * a.Wo : 0, st);
  if (head_major) return LSS_E_LAYOUT;  // only the GEMM kernel writes that layout
  if (dt == LSS_DT_BF16) {
    if (fused) hipLaunchKernelGGL((conv_direct_kernel<unsigned short, true>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((conv_direct_kernel<unsigned short, false>), grid, dim3(256), 0, st, a);
  } else {
    if (fused) hipLaunchKernelGGL((conv_direct_kernel<float, true>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((conv_direct_kernel<float, false>), grid, dim3(256), 0, st, a);
  }
  return lss_launch_status();
}

// Stride-2 k x k conv (k = 3 pad 1, or k = 7 pad 3) on the LDS-tiled kernel through
// the phase-plane (space-to-depth) form; `w_s2d` from lss_conv2d_pack_weights_s2d.
static int conv2d_s2_impl(const void* x, const void* w_s2d, const float* scale, const float* shift,
                          const void* residual, void* y, float* stats, int B, int H, int W, int Cx, int Cout,
                          int K, int pad, int relu, void* y2, int split, int relu_n, void* stream) {
  LSS_CHECK_PTR(x); LSS_CHECK_PTR(w_s2d); LSS_CHECK_PTR(y);
  LSS_CHECK_POS(B); LSS_CHECK_POS(H); LSS_CHECK_POS(W); LSS_CHECK_POS(Cx); LSS_CHECK_POS(Cout);
  if (!((K == 3 && pad == 1) || (K == 7 && pad == 3) || (K == 1 && pad == 0))) return LSS_E_SHAPE;
  if (Cx % 64 != 0) return LSS_E_SHAPE;
  ConvFill f = conv_args_fill(x, nullptr, w_s2d, scale, shift, residual, y, stats, B, H, W, Cx, 0, 1, Cout, K, K, 2, pad,
                              relu & 3);
  if (f.rc != 0) return f.rc;
  ConvArgs& a = f.a;
  // the K loop runs over the four parity phases; K = 1 reads phase (0,0) only, so it runs over that phase alone
  // and the weights are the plain [1][Cout][Cx] pack
  a.Cin = K == 1 ? Cx : 4 * Cx;
  a.y2 = y2; a.split = split; a.relu_n = y2 ? relu_n : a.Cout;
  hipStream_t st = lss_stream(stream);
  if (K == 7) launch_conv_lds<2, 4, 4, 2>(a, st);
  else if (K == 3) launch_conv_lds<2, 2, 2, 1>(a, st);
  else launch_conv_lds<2, 1, 1, 0>(a, st);
  return lss_launch_status();
}

extern "C" int lss_conv2d_s2_fwd(const void* x, const void* w_s2d, const float* scale,
                                 const float* shift, const void* residual, void* y, float* stats,
                                 int B, int H, int W, int Cx, int Cout, int K, int pad, int relu,
                                 void* stream) {
  return conv2d_s2_impl(x, w_s2d, scale, shift, residual, y, stats, B, H, W, Cx, Cout, K, pad, relu, nullptr, 0, 0,
                        stream);
}

// Two stride-2 convs over the same input in ONE launch: output channels [0, split) -> y (with the
// activation), [split, Cout) -> y2 (no activation).  A BasicBlock's 3x3/2 conv1 and its 1x1/2
// downsample (embedded at the centre tap of a 3x3 frame so both share the phase-plane weight
// layout; ref: torchvision BasicBlock.forward, `out = relu(bn1(conv1(x)))`, `identity =
// downsample(x)`): the downsample's own launch (8.5 us) and its kernel boundary disappear.
extern "C" int lss_conv2d_s2_dual_fwd(const void* x, const void* w_s2d, const float* scale, const float* shift,
                                      void* y, void* y2, int B, int H, int W, int Cx, int Cout, int split, int K,
                                      int pad, int relu, void* stream) {
  LSS_CHECK_PTR(y2);
  if (split <= 0 || split >= Cout || split % 128 != 0 || (Cout - split) % 8 != 0) return LSS_E_SHAPE;
  return conv2d_s2_impl(x, w_s2d, scale, shift, nullptr, y, nullptr, B, H, W, Cx, Cout, K, pad, relu, y2, split,
                        split, stream);
}

// 3x3 / stride 1 / pad 1 conv (optionally with the fused upsample / concat gather)
// + scale/shift + ReLU + a fused 1x1 head, output NCHW fp32 (B, head_n, Ho, Wo).
// BevEncode's last two layers (ref: src/modules.py:110-116, up2[0..4]) in one launch:
// the 128-channel 200x200 activation and the NHWC->NCHW pass never touch HBM.
extern "C" int lss_conv2d_head_fwd(const void* x, const void* x2, const void* w_packed,
                                   const float* scale, const float* shift, const float* head_w,
                                   const float* head_b, float* out, int B, int H, int W, int Cx,
                                   int C2, int up, int Cout, int head_n, int relu, void* stream) {
  LSS_CHECK_PTR(x); LSS_CHECK_PTR(w_packed); LSS_CHECK_PTR(head_w); LSS_CHECK_PTR(head_b);
  LSS_CHECK_PTR(out);
  LSS_CHECK_POS(B); LSS_CHECK_POS(H); LSS_CHECK_POS(W); LSS_CHECK_POS(Cx); LSS_CHECK_POS(up);
  LSS_CHECK_POS(head_n);
  if (relu & LSS_W_RING) {
    if ((relu & ~(LSS_W_RING | 1)) != 0) return LSS_E_SHAPE;
    if (C2 > 0 && x2 == nullptr) return LSS_E_NULL;
    return lss_conv_ring_launch(x, x2, w_packed, scale, shift, nullptr, head_w, head_b, out, head_n, B, H, W, Cx, C2, up,
                                Cout, relu & 1, 0, lss_stream(stream));
  }
  if ((Cout != 128 && Cout != 64) || C2 < 0 || Cx % 64 != 0 || C2 % 64 != 0 || head_n > 64) return LSS_E_SHAPE;
  if (Cout == 64 && (up != 1 || C2 != 0)) return LSS_E_SHAPE;  // the 64-wide tile has no fused-gather form
  if (C2 > 0 && x2 == nullptr) return LSS_E_NULL;
  ConvFill f = conv_args_fill(x, x2, w_packed, scale, shift, nullptr, nullptr, nullptr, B, H, W, Cx, C2, up, Cout, 3, 3, 1,
                              1, relu & 3);
  if (f.rc != 0) return f.rc;
  ConvArgs& a = f.a;
  a.head_w = head_w; a.head_b = head_b; a.head_out = out; a.head_n = head_n;
  const bool fused = (up > 1) || (C2 > 0);
  hipStream_t st = lss_stream(stream);
  // the fused-gather form takes the 32-channel steps (three workgroups per CU), as in launch_conv_lds
  const TilePlan p = conv_tile_plan(a, fused ? 1 : 0, 3, true);
  if (p.kc == 32) launch_tile<2, 128, 1, 3, 3, 1, 32, 1, true>(a, p, st);
  else if (fused) launch_tile<2, 128, 1, 3, 3, 1, 64, 1, true>(a, p, st);
  else if (Cout == 64) launch_tile<2, 64, 0, 3, 3, 1, 64, 1, true>(a, p, st);
  else launch_tile<2, 128, 0, 3, 3, 1, 64, 1, true>(a, p, st);
  return lss_launch_status();
}

extern "C" int lss_conv2d_sequence(const lss_conv_launch_t* L, int n, void* stream) {
  LSS_CHECK_PTR(L);
  if (n < 0) return LSS_E_SHAPE;
  for (int i = 0; i < n; ++i) {
    const lss_conv_launch_t& c = L[i];
    int rc;
    if (c.kind == 0)
      rc = lss_conv2d_fwd(c.x, c.x2, c.w, c.scale, c.shift, c.residual, c.y, c.stats, c.B, c.H, c.W, c.Cx,
                          c.C2, c.up, c.Cout, c.KH, c.KW, c.stride, c.pad, c.relu, c.dt, stream);
    else if (c.kind == 1)
      rc = lss_conv2d_s2_fwd(c.x, c.w, c.scale, c.shift, c.residual, c.y, c.stats, c.B, c.H, c.W, c.Cx,
                             c.Cout, c.KH, c.pad, c.relu, stream);
    else if (c.kind == 2)
      rc = lss_conv2d_head_fwd(c.x, c.x2, c.w, c.scale, c.shift, c.head_w, c.head_b, c.head_out, c.B, c.H,
                               c.W, c.Cx, c.C2, c.up, c.Cout, c.head_n, c.relu, stream);
    else if (c.kind == 3)
      rc = lss_conv2d_s2_dual_fwd(c.x, c.w, c.scale, c.shift, c.y, c.y2, c.B, c.H, c.W, c.Cx, c.Cout, c.split, c.KH,
                                  c.pad, c.relu, stream);
    else if (c.kind == 4)
      rc = lss_conv2d_ks_s2_dual_fwd(c.x, c.w, c.scale, c.shift, c.y, c.y2, c.B, c.H, c.W, c.Cx, c.Cout, c.relu, stream);
    else if (c.kind == 5)
      rc = lss_conv2d_ks_stem_fwd(c.x, c.w, c.scale, c.shift, c.y, c.B, c.H, c.W, c.Cx, c.Cout, c.relu, stream);
    else
      rc = LSS_E_LAYOUT;
    if (rc != 0) return rc;
  }
  return 0;
}
