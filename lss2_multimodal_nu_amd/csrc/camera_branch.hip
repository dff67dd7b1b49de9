// K13  the camera branch of the vovnet model at inference: c3 -> scene tokens (include/lss_hip.h, "K13").
//
// tapconv_kernel: one implicit GEMM for every conv of the branch - the two dilated 3x3 pyramid convs, the fusion 1x1,
// the 1x1 and the three atrous 3x3 convs of the ASPP and its projection.  A launch carries up to four BRANCHES
// (weight image, kernel size, dilation, scale, shift, output channel offset) that read the same NHWC bf16 input and
// write channel slices of one wider NHWC bf16 buffer, so neither torch.cat of the reference is ever materialised.
//
//   * Live taps.  Tap (ky, kx) of a 3x3 conv with dilation d reads only zero padding when |ky d| >= H or |kx d| >= W.
//     The host entry derives the list of live taps from (H, W, d) and the kernel walks only those: on an 8 x 22 map
//     the ASPP rates 12 / 24 / 36 keep 3 / 1 / 1 of their 9 taps.  A live tap still zero-fills where it leaves the
//     map, and its source index is formed from (row, column) inside ONE image, so it never reads the neighbour.
//   * Tiling.  Workgroup = 256 threads = one image x one branch x 64 output channels; it walks the image's pixels in
//     tiles of 64 and, per tile, the K dimension (live taps x Cin) in steps of 64 channels.  Wave = 32 channels x 32
//     pixels = 2 x 2 tiles of v_mfma_f32_16x16x32_bf16 with the WEIGHTS as the A operand: a lane then holds four
//     consecutive output channels of one pixel, i.e. one 8-B NHWC store.  Both operands are staged through registers
//     into a two-slot LDS ring (rows padded to 144 B: the 16 rows of a ds_read_b128 fall on distinct banks); the loads
//     of step s + 1 are in flight while step s is multiplied, one barrier per step.
//   * Means.  Because a workgroup owns a whole image, the per-image channel mean is workgroup-local: the epilogue
//     parks each tile's fp32 values in LDS and ONE thread per channel adds the tile's VALID rows in row order into a
//     running sum - rows of a partial tile are skipped (relu(shift) != 0 there).  No float atomics, no dependence of
//     any tile shape on BN: the result is bit-identical run to run and for any batch the image sits in.
//
// pool_bias_kernel: the ASPP pooling branch.  The bilinear upsample of a 1 x 1 map is a per-image constant, so the
// branch is g = relu(bn(W_g . mean_hw(p))) (BN, Cg) and enters the projection as the per-image bias W_j[:, pool] . g:
// two small fp32 mat-vecs per image, eight outputs per wave and pass, lanes over K, butterfly sum (fixed order).
#include "lss_device.h"

namespace {

constexpr int TM = 64, TN = 64, TK = 64;  // pixels, output channels, input channels per step
constexpr int LDR = 2 * TK + 16;          // bytes per staged LDS row (padded)
constexpr int OP_BYTES = TM * LDR;        // one operand of one slot
constexpr int SLOT_BYTES = 2 * OP_BYTES;  // [pixels | weights]
constexpr int SLD = TN + 4;               // fp32 row of the mean tile
static_assert(TM * SLD * 4 <= 2 * SLOT_BYTES, "the mean tile reuses the ring");
constexpr int PB_J = 8;                   // outputs a wave of pool_bias_kernel carries per pass

struct TapBranch {
  const unsigned short* w;  // [tap][Cout][Cin] bf16
  const float* scale;       // (Cout) or null
  const float* shift;       // (Cout) or null
  unsigned long long taps;  // live tap indices (ky * 3 + kx; 0 for a 1x1), 4 bits each
  int ntap, ksize, dil, ch_off;
};

struct TapArgs {
  const unsigned short* x;  // (BN, H, W, Cin) bf16
  unsigned short* y;        // (BN, H, W, y_stride) bf16 or null
  const float* img_bias;    // (BN, Cout) or null
  float* means;             // (BN, Cout) or null
  TapBranch br[4];
  int BN, H, W, Cin, Cout, nbranch, y_stride, relu;
};

__global__ __launch_bounds__(256) void tapconv_kernel(TapArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * SLOT_BYTES];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ntn = a.Cout / TN;
  int bid = blockIdx.x;
  const int n0 = (bid % ntn) * TN;
  bid /= ntn;
  const int bi = bid % a.nbranch, img = bid / a.nbranch;
  // the branch by uniform selects (a dynamic index into the by-value argument would put it on the stack)
  const unsigned short* bw = a.br[0].w;
  const float* bscale = a.br[0].scale;
  const float* bshift = a.br[0].shift;
  unsigned long long taps = a.br[0].taps;
  int ntap = a.br[0].ntap, ksize = a.br[0].ksize, dil = a.br[0].dil, ch_off = a.br[0].ch_off;
#pragma unroll
  for (int b = 1; b < 4; ++b)
    if (bi == b) {
      bw = a.br[b].w; bscale = a.br[b].scale; bshift = a.br[b].shift; taps = a.br[b].taps;
      ntap = a.br[b].ntap; ksize = a.br[b].ksize; dil = a.br[b].dil; ch_off = a.br[b].ch_off;
    }
  const int H = a.H, W = a.W, Cin = a.Cin, HW = H * W;
  const int ncb = Cin / TK, nsteps = ntap * ncb;

  // staging: thread -> rows srow, srow + 32 of both operands, 16-B piece spc
  const int srow = tid >> 3, spc = tid & 7;
  const unsigned short* ximg = a.x + (size_t)img * HW * Cin + spc * 8;
  const unsigned short* wrow = bw + (size_t)(n0 + srow) * Cin + spc * 8;
  const size_t wtap = (size_t)a.Cout * Cin;
  const int st_off = srow * LDR + spc * 16;

  // fragments: weights are A (rows = output channels), pixels are B
  const int wr = wave >> 1, wc = wave & 1;
  const int fr = lane & 15, fq = lane >> 4;
  const int a_off = OP_BYTES + (wr * 32 + fr) * LDR + fq * 16;
  const int b_off = (wc * 32 + fr) * LDR + fq * 16;

  float colsum = 0.f;  // threads 0..63: running sum of channel n0 + tid over the image's pixels
  for (int m0 = 0; m0 < HW; m0 += TM) {
    int ph[2], pw[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int m = m0 + srow + 32 * i;
      ph[i] = m < HW ? m / W : -(1 << 20);  // a row past the image is outside the map for every tap
      pw[i] = m < HW ? m - ph[i] * W : 0;
    }
    // Step s + 1 waits in these four registers while step s is multiplied.  A pixel piece is always loaded from an
    // address inside the image (the source clamped into the map) and zeroed by a select: no branch around a load.
    uint4 ra0, ra1, rb0, rb1;
    auto pixel_piece = [&](int h, int w, int dy, int dx, int cb) -> uint4 {
      const int hs = h + dy, ws = w + dx;
      const bool in = hs >= 0 && hs < H && ws >= 0 && ws < W;
      const int hc = min(max(hs, 0), H - 1), wcl = min(max(ws, 0), W - 1);
      const uint4 v = *reinterpret_cast<const uint4*>(ximg + (size_t)(hc * W + wcl) * Cin + cb * TK);
      return in ? v : make_uint4(0, 0, 0, 0);
    };
#define TAPCONV_FETCH(s_)                                                                             \
  do {                                                                                                \
    const int ti_ = (s_) / ncb, cb_ = (s_) - ti_ * ncb;                                               \
    const int tap_ = (int)((taps >> (4 * ti_)) & 15);                                                 \
    const int dy_ = ksize == 3 ? (tap_ / 3 - 1) * dil : 0, dx_ = ksize == 3 ? (tap_ % 3 - 1) * dil : 0; \
    const unsigned short* wp_ = wrow + (size_t)tap_ * wtap + cb_ * TK;                                \
    rb0 = *reinterpret_cast<const uint4*>(wp_);                                                       \
    rb1 = *reinterpret_cast<const uint4*>(wp_ + (size_t)32 * Cin);                                    \
    ra0 = pixel_piece(ph[0], pw[0], dy_, dx_, cb_);                                                   \
    ra1 = pixel_piece(ph[1], pw[1], dy_, dx_, cb_);                                                   \
  } while (0)
#define TAPCONV_STASH(slot_)                                               \
  do {                                                                     \
    unsigned char* sb_ = smem + (slot_) * SLOT_BYTES + st_off;             \
    *reinterpret_cast<uint4*>(sb_) = ra0;                                  \
    *reinterpret_cast<uint4*>(sb_ + 32 * LDR) = ra1;                       \
    *reinterpret_cast<uint4*>(sb_ + OP_BYTES) = rb0;                       \
    *reinterpret_cast<uint4*>(sb_ + OP_BYTES + 32 * LDR) = rb1;            \
  } while (0)

    f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    TAPCONV_FETCH(0);
    TAPCONV_STASH(0);
    __syncthreads();
    for (int s = 0; s < nsteps; ++s) {
      if (s + 1 < nsteps) TAPCONV_FETCH(s + 1);
      const unsigned char* base = smem + (s & 1) * SLOT_BYTES;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        bf16x8_t fw[2], fx[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          fw[i] = *reinterpret_cast<const bf16x8_t*>(base + a_off + i * 16 * LDR + ks * 64);
          fx[i] = *reinterpret_cast<const bf16x8_t*>(base + b_off + i * 16 * LDR + ks * 64);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fw[i], fx[j], acc[i][j], 0, 0, 0);
      }
      // the other slot was last read in step s - 1, and every wave has passed that step's barrier
      if (s + 1 < nsteps) TAPCONV_STASH((s + 1) & 1);
      __syncthreads();
    }

    // D[channel 4 fq + e][pixel fr]: four consecutive channels of one pixel per lane
    float* tile = reinterpret_cast<float*>(smem);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int cl = wr * 32 + i * 16 + 4 * fq, co = n0 + cl;
      const f32x4 sc = bscale ? lss_load4<float>(bscale + co) : (f32x4){1.f, 1.f, 1.f, 1.f};
      const f32x4 sh = bshift ? lss_load4<float>(bshift + co) : (f32x4){0.f, 0.f, 0.f, 0.f};
      const f32x4 ib = a.img_bias ? lss_load4<float>(a.img_bias + (size_t)img * a.Cout + co) : (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int ml = wc * 32 + j * 16 + fr, m = m0 + ml;
        f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float t = (acc[i][j][e] + ib[e]) * sc[e] + sh[e];
          if (a.relu) t = fmaxf(t, 0.f);
          if (a.y) t = lss_bf2f(lss_f2bf(t));  // the mean is taken over the values as stored
          v[e] = t;
        }
        if (a.y && m < HW) lss_store4(a.y + ((size_t)img * HW + m) * a.y_stride + ch_off + co, v);
        if (a.means) lss_store4(tile + ml * SLD + cl, v);
      }
    }
    if (a.means) {
      __syncthreads();
      if (tid < TN) {
        const int nv = min(TM, HW - m0);  // rows of a partial tile do not enter the mean
        for (int r = 0; r < nv; ++r) colsum += tile[r * SLD + tid];
      }
      __syncthreads();  // the tile is the ring: read before the next pixel tile is staged
    }
  }
  if (a.means && tid < TN) a.means[(size_t)img * a.Cout + n0 + tid] = colsum / (float)HW;
}

// g[img][c] = relu(scale[c] * (wg[c, :] . mean[img, :]) + shift[c]),  bias[img][o] = wj[o, :] . g[img, :]
__global__ __launch_bounds__(256) void pool_bias_kernel(const float* __restrict__ mean, const float* __restrict__ wg,
                                                        const float* __restrict__ scale, const float* __restrict__ shift,
                                                        const float* __restrict__ wj, int C, int Cg, int Cout,
                                                        float* __restrict__ g, float* __restrict__ bias) {
  __shared__ float sm[1024], sg[1024];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, img = blockIdx.x;
  for (int k = tid; k < C; k += 256) sm[k] = mean[(size_t)img * C + k];
  __syncthreads();
  // PB_J outputs per pass: their K chains and butterflies are independent, so their latencies overlap; each output's
  // own summation order (one lane per 64th of K, then the butterfly) does not depend on PB_J
  for (int c0 = wave * PB_J; c0 < Cg; c0 += 4 * PB_J) {
    float s[PB_J];
#pragma unroll
    for (int j = 0; j < PB_J; ++j) s[j] = 0.f;
    for (int k = lane; k < C; k += 64) {
      const float m = sm[k];
#pragma unroll
      for (int j = 0; j < PB_J; ++j) s[j] += wg[(size_t)min(c0 + j, Cg - 1) * C + k] * m;
    }
#pragma unroll
    for (int j = 0; j < PB_J; ++j) {
      const int c = c0 + j;
      float v = lss_wave_sum(s[j]);
      if (c < Cg) {
        v = fmaxf(v * (scale ? scale[c] : 1.f) + (shift ? shift[c] : 0.f), 0.f);
        if (lane == 0) {
          sg[c] = v;
          if (g) g[(size_t)img * Cg + c] = v;
        }
      }
    }
  }
  __syncthreads();
  for (int o0 = wave * PB_J; o0 < Cout; o0 += 4 * PB_J) {
    float s[PB_J];
#pragma unroll
    for (int j = 0; j < PB_J; ++j) s[j] = 0.f;
    for (int k = lane; k < Cg; k += 64) {
      const float gk = sg[k];
#pragma unroll
      for (int j = 0; j < PB_J; ++j) s[j] += wj[(size_t)min(o0 + j, Cout - 1) * Cg + k] * gk;
    }
#pragma unroll
    for (int j = 0; j < PB_J; ++j) {
      const float v = lss_wave_sum(s[j]);
      if (o0 + j < Cout && lane == 0) bias[(size_t)img * Cout + o0 + j] = v;
    }
  }
}

int shape_ok(int BN, int H, int W, int Cin, int Cout) {
  if (BN < 1 || BN > 65535 || H < 1 || W < 1 || H > 1024 || W > 1024 || H * W > 65536) return LSS_E_SHAPE;
  if (Cin < 64 || Cin > 4096 || Cin % 64 != 0 || Cout < 64 || Cout > 1024 || Cout % 64 != 0) return LSS_E_SHAPE;
  return 1;
}

}  // namespace

extern "C" int lss_tapconv_ok(int BN, int H, int W, int Cin, int Cout) { return shape_ok(BN, H, W, Cin, Cout); }

extern "C" int lss_tapconv_fwd(const lss_tapconv_desc_t* d, void* stream) {
  LSS_CHECK_PTR(d);
  LSS_CHECK_PTR(d->x);
  if (d->y == nullptr && d->means == nullptr) return LSS_E_NULL;
  if (d->nbranch < 1 || d->nbranch > 4) return LSS_E_SHAPE;
  for (int b = 0; b < d->nbranch; ++b) LSS_CHECK_PTR(d->branch[b].w);
  if (shape_ok(d->BN, d->H, d->W, d->Cin, d->Cout) != 1) return LSS_E_SHAPE;
  if (d->relu != 0 && d->relu != 1) return LSS_E_LAYOUT;
  // a per-image bias or mean belongs to ONE (BN, Cout) map
  if ((d->img_bias != nullptr || d->means != nullptr) && d->nbranch != 1) return LSS_E_SHAPE;
  if (d->y != nullptr && (d->y_stride < d->Cout || d->y_stride % 4 != 0)) return LSS_E_SHAPE;
  TapArgs a;
  for (int b = 0; b < d->nbranch; ++b) {
    const lss_tapconv_branch_t& s = d->branch[b];
    if (s.ksize != 1 && s.ksize != 3) return LSS_E_LAYOUT;
    if (s.dilation < 1 || s.dilation > 1024) return LSS_E_SHAPE;
    if (d->y != nullptr && (s.ch_off < 0 || s.ch_off % 4 != 0 || s.ch_off + d->Cout > d->y_stride)) return LSS_E_SHAPE;
    if (!lss_aligned(s.w, 16) || !lss_aligned(s.scale, 16) || !lss_aligned(s.shift, 16)) return LSS_E_ALIGN;
    TapBranch& t = a.br[b];
    t.w = static_cast<const unsigned short*>(s.w);
    t.scale = s.scale;
    t.shift = s.shift;
    t.ksize = s.ksize;
    t.dil = s.dilation;
    t.ch_off = d->y != nullptr ? s.ch_off : 0;
    t.taps = 0;
    t.ntap = 0;
    if (s.ksize == 1) {
      t.ntap = 1;  // tap 0 of a [1][Cout][Cin] image
    } else {
      for (int tap = 0; tap < 9; ++tap) {
        const long long dy = (long long)(tap / 3 - 1) * s.dilation, dx = (long long)(tap % 3 - 1) * s.dilation;
        if (llabs(dy) >= d->H || llabs(dx) >= d->W) continue;  // reads zero padding only
        t.taps |= (unsigned long long)tap << (4 * t.ntap);
        ++t.ntap;
      }
    }
  }
  for (int b = d->nbranch; b < 4; ++b) a.br[b] = a.br[0];
  if (!lss_aligned(d->x, 16) || !lss_aligned(d->y, 8) || !lss_aligned(d->img_bias, 16) || !lss_aligned(d->means, 4))
    return LSS_E_ALIGN;
  a.x = static_cast<const unsigned short*>(d->x);
  a.y = static_cast<unsigned short*>(d->y);
  a.img_bias = d->img_bias;
  a.means = d->means;
  a.BN = d->BN; a.H = d->H; a.W = d->W; a.Cin = d->Cin; a.Cout = d->Cout;
  a.nbranch = d->nbranch; a.y_stride = d->y_stride; a.relu = d->relu;
  const long long nwg = (long long)d->BN * d->nbranch * (d->Cout / TN);
  hipLaunchKernelGGL(tapconv_kernel, dim3((unsigned)nwg), dim3(256), 0, lss_stream(stream), a);
  return lss_launch_status();
}

extern "C" int lss_camera_pool_bias_fwd(const float* mean, const float* wg, const float* scale, const float* shift,
                                        const float* wj, int BN, int C, int Cg, int Cout, float* g, float* bias,
                                        void* stream) {
  LSS_CHECK_PTR(mean); LSS_CHECK_PTR(wg); LSS_CHECK_PTR(wj); LSS_CHECK_PTR(bias);
  if (BN < 1 || BN > 65535 || C < 1 || C > 1024 || Cg < 1 || Cg > 1024 || Cout < 1 || Cout > 4096) return LSS_E_SHAPE;
  if (!lss_aligned(mean, 4) || !lss_aligned(wg, 4) || !lss_aligned(scale, 4) || !lss_aligned(shift, 4) ||
      !lss_aligned(wj, 4) || !lss_aligned(g, 4) || !lss_aligned(bias, 4))
    return LSS_E_ALIGN;
  hipLaunchKernelGGL(pool_bias_kernel, dim3((unsigned)BN), dim3(256), 0, lss_stream(stream), mean, wg, scale, shift, wj,
                     C, Cg, Cout, g, bias);
  return lss_launch_status();
}
