// K16  training of the vovnet camera branch: what the tap-list conv of K13 (camera_branch.hip) lacks for a backward
// pass (include/lss_hip.h, "K16").  The input gradient of such a conv is lss_tapconv_fwd itself on the flipped and
// transposed weight image; here are the weight gradient and the gradient of the per-image bias.
//
// tapconv_wgrad_kernel   dw[o][c][tap] = sum_{img, h, w} dy[img, h, w, o] x[img, h + ky d, w + kx d, c]  (live taps)
//   The contraction index is the PIXEL, the slow dimension of both NHWC operands.  As in K9w (conv_wgrad.hip) and K11
//   (linear_grad.hip) both are staged position-major as they lie and transposed on the way into the matrix core by
//   `ds_read_b64_tr_b16`; there is no channel-major copy anywhere.
//   * Workgroup = 256 threads = one 64 (o) x 64 (c) tile of dw, ALL live taps, over one contiguous range of images.
//     Per image it stages two LDS images, 128 B per pixel: channels c0 .. c0+63 of x and o0 .. o0+63 of dy (the 32-B
//     channel tiles XOR-swizzled by lss_tr_swz, K9w's layout).  Then one barrier, the MFMAs, one barrier: a plain
//     barrier kernel, no flag words, nothing to time out.
//   * One x image serves every tap.  A lane of a transposed read supplies the address of ONE pixel row, so the tap's
//     shift is applied per lane: the lane that stands for pixel (h, w) of dy points at pixel (h + ky d, w + kx d) of
//     the x image, formed from (row, column) inside the image - no row wrap, no neighbouring image - or at the ZERO
//     ROW behind the image when that leaves the map.  Pixels at and beyond H W of the last 32-pixel step are zero
//     rows of dy and zero-row reads of x: they add exact zeros.  All 256 threads run every transposed read (EXEC all
//     ones; the tap loop is unrolled and its guard is workgroup-uniform), every address is a multiple of 8 B.
//   * Wave = a 32 (o) x 32 (c) quarter of the tile = 2 x 2 tiles of v_mfma_f32_16x16x32_bf16 per live tap (K = 32
//     pixels), the dy fragments of a step shared by all taps; up to 9 x 4 accumulator tiles (144 registers) live over
//     the whole image range, so the images of a range are added in image order inside the accumulator.
//   * The tile goes to the workspace as part[split][live tap][Cout][Cin]; tapconv_wgrad_reduce_kernel adds the splits
//     in split order (lg_sum_splits), writes OIHW and writes exactly 0 for a dead tap.  No float atomics.
//   Split rule (a function of the shape alone): tiles = (Cout / 64)(Cin / 64), want = clamp(512 / tiles, 1, BN),
//   per = ceil(BN / want) images per workgroup, splits = ceil(BN / per).
//
// tapconv_bias_grad_kernel   dbias[img, o] = sum over the image's pixels of dz[img, h, w, o]
//   Workgroup = one image x 64 channels; thread = 8 channels of pixels r, r + 32, ... (fp32 chains in pixel order), the
//   32 chains of a channel added in chain order through LDS.
#include <algorithm>

#include "lss_device.h"

namespace {

constexpr int TW_MAXP = 224;                         // pixel rows of one LDS image: H W rounded up to 32 may not exceed it
constexpr int TW_ROW = 128;                          // bytes per pixel row: 64 channels
constexpr int TW_X_BYTES = (TW_MAXP + 1) * TW_ROW;   // + the zero row
constexpr int TW_DY_BYTES = TW_MAXP * TW_ROW;
constexpr int TW_MAXWG = 512;
static_assert(TW_X_BYTES + TW_DY_BYTES <= 64 * 1024, "two images of one picture in 64 KiB of LDS");

struct TapWgradArgs {
  const unsigned short* x;   // (BN, H, W, Cin) bf16
  const unsigned short* dy;  // (BN, H, W, Cout) bf16
  float* part;               // [split][live tap][Cout][Cin]
  unsigned long long taps;   // live tap indices (ky * 3 + kx; 0 for a 1x1), 4 bits each, ascending
  int ntap, ksize, dil;
  int BN, H, W, Cin, Cout;
  int per;                   // images per split
};

// byte offset of pixel row `pos`, 16-channel tile `ct`, inside an LDS image
__device__ __forceinline__ int tw_off(int pos, int ct) { return pos * TW_ROW + ((ct ^ lss_tr_swz(pos)) << 5); }

__global__ __launch_bounds__(256) void tapconv_wgrad_kernel(const TapWgradArgs a) {
  __shared__ __attribute__((aligned(1024))) unsigned char smem[TW_X_BYTES + TW_DY_BYTES];
  unsigned char* sx = smem;
  unsigned char* sd = smem + TW_X_BYTES;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ntc = a.Cin >> 6, nto = a.Cout >> 6;
  int bid = blockIdx.x;
  const int c0 = (bid % ntc) * 64;
  bid /= ntc;
  const int o0 = (bid % nto) * 64;
  const int split = bid / nto;
  const int H = a.H, W = a.W, HW = H * W;
  const int HWp = (HW + 31) & ~31, nks = HWp >> 5;   // HWp <= TW_MAXP (lss_tapconv_wgrad_ok)
  const int img0 = split * a.per, img1 = min(a.BN, img0 + a.per);
  const int ntap = a.ntap;

  // rows no image ever fills, zeroed once: HW .. HWp of x (HWp is the zero row), HW .. HWp - 1 of dy
  const uint4 zero4 = make_uint4(0u, 0u, 0u, 0u);
  for (int idx = tid; idx < (HWp + 1 - HW) * 8; idx += 256)
    *reinterpret_cast<uint4*>(sx + (HW + (idx >> 3)) * TW_ROW + (idx & 7) * 16) = zero4;
  for (int idx = tid; idx < (HWp - HW) * 8; idx += 256)
    *reinterpret_cast<uint4*>(sd + (HW + (idx >> 3)) * TW_ROW + (idx & 7) * 16) = zero4;

  // transposed reads: lane (g, q, p) supplies pixel 8 g + 4 h + q of a 32-pixel step, channels 16 ct + 4 p .. + 3, and
  // receives channel 16 ct + (lane & 15) at pixels 8 g + 4 h .. + 3 - the 16x16x32 operand's k = 8 g .. 8 g + 7
  const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
  const int wr = wave >> 1, wc = wave & 1;

  f32x4 acc[9][2][2];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[t][i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  for (int img = img0; img < img1; ++img) {
    if (img != img0) __syncthreads();  // every wave has left the previous image's reads
    const unsigned short* xi = a.x + (size_t)img * HW * a.Cin + c0;
    const unsigned short* di = a.dy + (size_t)img * HW * a.Cout + o0;
    for (int idx = tid; idx < HW * 8; idx += 256) {
      const int pos = idx >> 3, c = idx & 7;
      const int off = tw_off(pos, c >> 1) + (c & 1) * 16;
      *reinterpret_cast<uint4*>(sx + off) = *reinterpret_cast<const uint4*>(xi + (size_t)pos * a.Cin + 8 * c);
      *reinterpret_cast<uint4*>(sd + off) = *reinterpret_cast<const uint4*>(di + (size_t)pos * a.Cout + 8 * c);
    }
    __syncthreads();

    for (int ks = 0; ks < nks; ++ks) {
      int pa[2], ph[2], pw[2];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        pa[h] = ks * 32 + 8 * g + 4 * h + q;
        ph[h] = pa[h] < HW ? pa[h] / W : -(1 << 20);  // a pixel past the image is outside the map for every tap
        pw[h] = pa[h] < HW ? pa[h] - ph[h] * W : 0;
      }
      bf16x8_t fd[2];
#pragma unroll
      for (int i = 0; i < 2; ++i)
        fd[i] = lss_tr_frag(sd + tw_off(pa[0], wr * 2 + i) + p * 8, sd + tw_off(pa[1], wr * 2 + i) + p * 8);
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        if (t < ntap) {  // workgroup-uniform
          const int tap = (int)((a.taps >> (4 * t)) & 15);
          const int dyo = a.ksize == 3 ? (tap / 3 - 1) * a.dil : 0, dxo = a.ksize == 3 ? (tap % 3 - 1) * a.dil : 0;
          int src[2];
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const int hs = ph[h] + dyo, ws = pw[h] + dxo;
            src[h] = (hs >= 0 && hs < H && ws >= 0 && ws < W) ? hs * W + ws : HWp;
          }
          bf16x8_t fx[2];
#pragma unroll
          for (int j = 0; j < 2; ++j)
            fx[j] = lss_tr_frag(sx + tw_off(src[0], wc * 2 + j) + p * 8, sx + tw_off(src[1], wc * 2 + j) + p * 8);
#pragma unroll
          for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
              acc[t][i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fd[i], fx[j], acc[t][i][j], 0, 0, 0);
        }
      }
    }
  }

  // D[o = 4 g + r][c = lane & 15]
  const size_t plane = (size_t)a.Cout * a.Cin;
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    if (t < ntap) {
      float* out = a.part + ((size_t)split * ntap + t) * plane;
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int o = o0 + wr * 32 + i * 16 + 4 * g + r, c = c0 + wc * 32 + j * 16 + (lane & 15);
            out[(size_t)o * a.Cin + c] = acc[t][i][j][r];
          }
    }
  }
}

// dw[o][c][tap] (OIHW) = the S partials of a live tap added in split order; exactly 0 for a dead tap
__global__ __launch_bounds__(256) void tapconv_wgrad_reduce_kernel(const float* __restrict__ part, int S, int ntap,
                                                                   unsigned long long taps, int kk, int OC,
                                                                   float* __restrict__ dw) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= OC) return;
  int s = 0;  // the list is ascending
  for (int tap = 0; tap < kk; ++tap) {
    float v = 0.f;
    if (s < ntap && (int)((taps >> (4 * s)) & 15) == tap) {
      v = lg_sum_splits(part + (size_t)s * OC + i, S, (size_t)ntap * OC);
      ++s;
    }
    dw[(size_t)i * kk + tap] = v;
  }
}

__global__ __launch_bounds__(256) void tapconv_bias_grad_kernel(const unsigned short* __restrict__ dz, int HW, int Cout,
                                                                float* __restrict__ dbias) {
  __shared__ float red[32 * 64];
  const int tid = threadIdx.x, r = tid >> 3, c = tid & 7;
  const int nto = Cout >> 6;
  const int img = blockIdx.x / nto, o0 = (blockIdx.x % nto) * 64;
  const unsigned short* base = dz + (size_t)img * HW * Cout + o0 + 8 * c;
  float s[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) s[e] = 0.f;
  for (int pos = r; pos < HW; pos += 32) {
    float v[8];
    lss_unpack8(*reinterpret_cast<const uint4*>(base + (size_t)pos * Cout), v);
#pragma unroll
    for (int e = 0; e < 8; ++e) s[e] += v[e];
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) red[r * 64 + c * 8 + e] = s[e];
  __syncthreads();
  if (tid < 64) {
    float t = 0.f;
    for (int i = 0; i < 32; ++i) t += red[i * 64 + tid];
    dbias[(size_t)img * Cout + o0 + tid] = t;
  }
}

inline bool tw_channels_ok(int Cin, int Cout) {
  return Cin >= 64 && Cin <= 4096 && Cin % 64 == 0 && Cout >= 64 && Cout <= 1024 && Cout % 64 == 0;
}

struct TapList {
  unsigned long long taps;
  int ntap;
};

// the live taps of lss_tapconv_fwd: |ky d| < H and |kx d| < W
inline TapList tw_live_taps(int H, int W, int ksize, int dilation) {
  TapList l = {0ull, 0};
  if (ksize == 1) {
    l.ntap = 1;
    return l;
  }
  for (int tap = 0; tap < 9; ++tap) {
    const long long dy = (long long)(tap / 3 - 1) * dilation, dx = (long long)(tap % 3 - 1) * dilation;
    if (llabs(dy) >= H || llabs(dx) >= W) continue;
    l.taps |= (unsigned long long)tap << (4 * l.ntap);
    ++l.ntap;
  }
  return l;
}

struct TapSplit {
  int per, S;
};

inline TapSplit tw_split(int BN, int Cin, int Cout) {
  const int tiles = (Cin / 64) * (Cout / 64);
  const int want = std::max(1, std::min(BN, TW_MAXWG / tiles));
  TapSplit sp;
  sp.per = lss_cdiv(BN, want);
  sp.S = lss_cdiv(BN, sp.per);
  return sp;
}

inline bool tw_dilation_ok(int dilation) { return dilation >= 1 && dilation <= 1024; }

}  // namespace

extern "C" int lss_tapconv_wgrad_ok(int BN, int H, int W, int Cin, int Cout) {
  if (BN < 1 || BN > 65535 || H < 1 || W < 1 || H > TW_MAXP || W > TW_MAXP || H * W > TW_MAXP) return LSS_E_SHAPE;
  return tw_channels_ok(Cin, Cout) ? 1 : LSS_E_SHAPE;
}

extern "C" size_t lss_tapconv_wgrad_workspace_bytes(int BN, int H, int W, int Cin, int Cout, int ksize, int dilation) {
  if (lss_tapconv_wgrad_ok(BN, H, W, Cin, Cout) != 1 || (ksize != 1 && ksize != 3) || !tw_dilation_ok(dilation))
    return 0;
  const TapSplit sp = tw_split(BN, Cin, Cout);
  return (size_t)sp.S * tw_live_taps(H, W, ksize, dilation).ntap * Cout * Cin * sizeof(float);
}

extern "C" int lss_tapconv_wgrad(const void* x, const void* dy, int BN, int H, int W, int Cin, int Cout, int ksize,
                                 int dilation, void* workspace, size_t workspace_bytes, float* dw, void* stream) {
  LSS_CHECK_PTR(x); LSS_CHECK_PTR(dy); LSS_CHECK_PTR(workspace); LSS_CHECK_PTR(dw);
  if (lss_tapconv_wgrad_ok(BN, H, W, Cin, Cout) != 1) return LSS_E_SHAPE;
  if (ksize != 1 && ksize != 3) return LSS_E_LAYOUT;
  if (!tw_dilation_ok(dilation)) return LSS_E_SHAPE;
  if (!lss_aligned(x, 16) || !lss_aligned(dy, 16) || !lss_aligned(workspace, 16) || !lss_aligned(dw, 4))
    return LSS_E_ALIGN;
  if (workspace_bytes < lss_tapconv_wgrad_workspace_bytes(BN, H, W, Cin, Cout, ksize, dilation)) return LSS_E_WORKSPACE;
  const TapSplit sp = tw_split(BN, Cin, Cout);
  const TapList tl = tw_live_taps(H, W, ksize, dilation);
  TapWgradArgs a;
  a.x = static_cast<const unsigned short*>(x);
  a.dy = static_cast<const unsigned short*>(dy);
  a.part = static_cast<float*>(workspace);
  a.taps = tl.taps; a.ntap = tl.ntap; a.ksize = ksize; a.dil = dilation;
  a.BN = BN; a.H = H; a.W = W; a.Cin = Cin; a.Cout = Cout;
  a.per = sp.per;
  hipStream_t st = lss_stream(stream);
  hipLaunchKernelGGL(tapconv_wgrad_kernel, dim3((unsigned)((Cin / 64) * (Cout / 64) * sp.S)), dim3(256), 0, st, a);
  const int rc = lss_launch_status();
  if (rc != 0) return rc;
  const int OC = Cout * Cin;
  hipLaunchKernelGGL(tapconv_wgrad_reduce_kernel, dim3(lss_cdiv(OC, 256)), dim3(256), 0, st, a.part, sp.S, tl.ntap,
                     tl.taps, ksize * ksize, OC, dw);
  return lss_launch_status();
}

extern "C" int lss_tapconv_bias_grad(const void* dz, int BN, int H, int W, int Cout, float* dbias, void* stream) {
  LSS_CHECK_PTR(dz); LSS_CHECK_PTR(dbias);
  if (BN < 1 || BN > 65535 || H < 1 || W < 1 || H > 1024 || W > 1024 || H * W > 65536) return LSS_E_SHAPE;
  if (Cout < 64 || Cout > 1024 || Cout % 64 != 0) return LSS_E_SHAPE;
  if (!lss_aligned(dz, 16) || !lss_aligned(dbias, 4)) return LSS_E_ALIGN;
  hipLaunchKernelGGL(tapconv_bias_grad_kernel, dim3((unsigned)(BN * (Cout / 64))), dim3(256), 0, lss_stream(stream),
                     static_cast<const unsigned short*>(dz), H * W, Cout, dbias);
  return lss_launch_status();
}
