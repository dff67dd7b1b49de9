// K8k: the launch-bound 3x3 / stride-1 convolutions of BevEncode - resnet18's layer1 / layer2 / layer3 at 100^2 x 64,
// 50^2 x 128, 25^2 x 256 (ref src/modules.py:104-106, 123-125 + torchvision BasicBlock: conv3x3 - BN - ReLU - conv3x3 -
// BN - (+identity) - ReLU) - as ONE PASS per workgroup, without a K loop.
//
// Why another kernel.  On the tile kernel (conv_mfma.hip) these ten launches cost 10.5-14.9 us each for 1.2 us of MFMA
// work (profiles/r03_conv_phase_stamps.txt): a workgroup walks 9-36 (chunk, tap) steps, each a weight slab by LDS-DMA,
// a barrier and 12 ds_read_b128 per wave for 8 MFMAs - the steps are LDS-read bound (96 KiB of fragment reads per step
// and CU against 512 MFMA cycles) and latency bound (0.37-0.46 us per step against 0.11 us of MFMA issue), and the grids
// (112-364 workgroups) leave half of the chip idle.  Deeper weight rings did not move them (profiles/r04_deep_ring_ab.txt).
// Here the work is cut so that EVERYTHING a workgroup needs is on the CU before the first MFMA, and the K dimension is
// split over the WAVES of the workgroup instead of over steps:
//   * workgroup = PB flattened pixels of one image (80 / 160 / 320) x 32 output channels x the whole K = 9 Cin;
//     256 workgroups at batch 4 for all three layers (one per CU, one round);
//   * the input patch - the <= 5 image rows the pixels span plus one halo row above and below, all Cin channels,
//     zero-padded - goes to LDS by LDS-DMA ONCE (91-98 KiB: [32-channel chunk][16-channel half][position][32 B], so that
//     the B fragment of 16 consecutive pixels is one conflict-free 1-KiB read for every tap shift);
//   * the weights never touch LDS: wave w owns a K part (layer3: chunks 2w, 2w + 1 x 9 taps = 18 k-steps of 32; layer2:
//     chunk w x 9 taps; layer1: 2 K parts x 2 pixel halves) and keeps its A fragments - 2 channel tiles x 9-18 k-steps
//     x 4 registers - in REGISTERS for the whole launch, loaded with fully coalesced 16-B-per-lane loads from a pack
//     that has exactly this image (lss_conv2d_pack_weights_ks);
//   * main phase: for every k-step the wave reads the B fragment of each of its 5-10 pixel tiles from LDS (one
//     ds_read_b128 = 16 pixels x 32 channels) and issues two v_mfma_f32_16x16x32_bf16 against the two channel tiles:
//     0.5 KiB of LDS reads per MFMA - the ratio of the ring kernel (section 4c) - no barrier, no flag, no DMA inside;
//   * the K parts meet through LDS once (fp32, fixed order kp = 0, 1, 2, 3: deterministic), each wave finishing a
//     quarter of the pixel tiles - its own part of those stays in registers, only the foreign parts cross LDS (below:
//     ks_slot_tile) -: folded BatchNorm scale / shift, residual, ReLU, one 16-B store per lane - the rows of
//     channel tile t are the channels {8 q + 4 t + i}, so lane (q, n) ends with 8 CONSECUTIVE channels of pixel n and
//     the four q lanes of a pixel write 64 contiguous bytes (no LDS staging of the output tile).
// No inter-workgroup communication, no bounded waits: nothing here can hang.
#include <type_traits>

#include "conv_launch.h"
#include "lss_device.h"

namespace {

constexpr int KS_ROWS = 7;        // patch rows: the <= 5 image rows a pixel block spans + the halo row above and below
constexpr int KS_POSB = 64;       // bytes per patch position and chunk (32 channels bf16)
constexpr int KS_LDS_MAX = 160 * 1024;

// Where the B-fragment reads of k-step s + 1 go (all three kernels).  Interleaved: tile j's read behind tile j's MFMAs
// of k-step s - it issues while the matrix pipe works, PXT - 1 reads are outstanding at every MFMA group and the counted
// lgkmcnt fits the 4-bit counter.  Clustered (-DKS_READS_CLUSTER, tools/build_diag_libs.sh KS_CLUSTER: the form the
// kernels had first, kept for same-box A/B): all PXT reads in front of the MFMAs of k-step s - at one wave per SIMD
// nothing issues MFMAs while the cluster issues, and the four waves' clusters hit the LDS array at the same moment, so
// its 128 B / clk and the matrix pipe take turns instead of overlapping ("Reads between the MFMAs").
#ifdef KS_READS_CLUSTER
constexpr bool KS_READS_INTERLEAVED = false;
#else
constexpr bool KS_READS_INTERLEAVED = true;
#endif
#ifdef KS_DIAG_NOREAD   // timing-only diagnostic build: the fragments are read once
constexpr bool KS_READS = false;
#else
constexpr bool KS_READS = true;
#endif

__device__ __attribute__((aligned(128))) unsigned char lss_ks_zero_page[128];  // source of out-of-image patch pieces

// Input patch -> LDS by LDS-DMA: [chunk][channel half][position][32 B]; a piece = 32 positions of one half; patch
// position (pr, pc) of `rows` x `pitch` (padded to nposp) is input pixel map(pr, pc) or, outside the image, the zero page
// (row / column of a lane's position advance by 64 positions per piece - no per-piece division: the first version
// spent ~60 VALU instructions of address arithmetic in front of every DMA instruction.  Staging the pieces through
// registers instead - plain 16-B loads, 24 in flight per wave, one ds_write_b128 each - was built and measured: the
// same 3-4 us from kernel entry to "patch and weights on the CU" (layer3 7.2 -> 8.2 us per launch): what bounds this
// phase is the 130-240 KiB every one of the 256 CUs pulls through its 64-B-per-clock L1 path at the same moment,
// 33-62 MB out of the L2s in ~3 us, not the way the requests are issued.)
// Layout and bank conflicts.  A ds_read_b128 is served in four groups of 16 lanes ({0-3, 12-15, 20-27}, {4-11, 16-19,
// 28-31}, ...: MI355X_MICROARCH.md, LDS) against a 256-B window of banks.  With 64 B per position (the four channel
// pieces side by side) the window is four positions and the lanes of a group that share a piece index - pixels n and
// n + 12, n + 4 and n + 8 - fall on the same 16 B: 2-way conflicts on every read.  With the two channel HALVES of a
// chunk in separate planes of 32 B per position the window is eight positions, a group's lanes of piece pair (0, 1) or
// (2, 3) cover sixteen different 16-B cells for ANY alignment of the 16 pixels - every tap shift - and the address is
// plane + position * 32 + (piece & 1) * 16: no arithmetic beyond the tap offset.  What that bought, measured (main
// phase, layer1 / 2 / 3, tools/bench_ks.py --stamps): 64-B positions with the conflicts 2.60 / 2.56 / 2.36 us; the same
// with an XOR swizzle of the piece index (conflict-free, four VALU instructions per read next to back-to-back MFMAs)
// 3.20 / 3.16 / 2.72; this layout 2.54 / 2.48 / 2.32 - and the two timing-only builds of tools/build_diag_libs.sh say
// why the conflicts never mattered: the 180 MFMAs of a wave alone (KS_NOREAD) take 2.06 / 2.04 / 1.84 us, the 90
// fragment reads alone (KS_NOMFMA) 1.20 / 1.28 / 1.36: the phase is the matrix pipe plus the quarter of the reads that
// does not hide behind it, at one wave per SIMD.
template <int NCH, class Map>
__device__ __forceinline__ void ks_fill_patch(unsigned char* smem, const unsigned short* ximg, int Cin, int H, int W,
                                              int rows, int pitch, int nposp, int wave, int lane, Map map) {
  const int ppc = nposp >> 4;                       // pieces per chunk: nposp / 32 position blocks x 2 halves
  const int q64 = 64 / pitch, r64 = 64 - q64 * pitch;  // wave-uniform
  const int h = wave & 1;                           // this wave's pieces: position blocks (wave >> 1) + 2 k of half h
  const int pos0 = 32 * (wave >> 1) + (lane >> 1);
  int pr = pos0 / pitch, pc = pos0 - pr * pitch;
  const unsigned char* zsrc = lss_ks_zero_page + (lane & 7) * 16;
  const unsigned short* xb = ximg + (2 * h + (lane & 1)) * 8;
  for (int i = wave; i < ppc; i += 4) {
    int iy, ix;
    map(pr, pc, iy, ix);
    const bool in = pr < rows && iy >= 0 && iy < H && ix >= 0 && ix < W;
    const unsigned short* src = xb + (in ? (iy * W + ix) * Cin : 0);
#pragma unroll
    for (int c = 0; c < NCH; ++c)
      lss_glds16(in ? (const void*)(src + c * 32) : (const void*)zsrc,
                smem + ((size_t)(c * 2 + h) * nposp + 32 * (i >> 1)) * 32);
    pr += q64; pc += r64;
    if (pc >= pitch) { pc -= pitch; ++pr; }
  }
}

// Diagnostics (LSS_KS_STAMPS=<hex device address>, tools/bench_ks.py --stamps): 8 slots per workgroup - 100-MHz
// s_memrealtime stamps 0-6 written by thread 0, slot 7 the shader-clock cycles of the main phase.  base null: nothing.
struct KsStamps {
  unsigned long long* base;
  int tid;
  unsigned long long clk_main = 0;
  __device__ __forceinline__ void stamp(int k) const {
    if (base != nullptr && tid == 0) base[(size_t)blockIdx.x * 8 + k] = __builtin_amdgcn_s_memrealtime();
  }
  __device__ __forceinline__ void main_begin() {
    if (base != nullptr) clk_main = __builtin_amdgcn_s_memtime();
  }
  // first / last: the accumulators the MFMA chain ends in (stamp 3 waits until it has retired)
  __device__ __forceinline__ void main_end(const f32x4& first, const f32x4& last) const {
    if (base != nullptr) asm volatile("s_nop 0" ::"v"(first), "v"(last));
    stamp(3);
    if (base != nullptr && tid == 0) base[(size_t)blockIdx.x * 8 + 7] = __builtin_amdgcn_s_memtime() - clk_main;
  }
  __device__ __forceinline__ void drain() const {
    if (base != nullptr) {
      stamp(5);
      lss_wait_vmcnt<0>();  // stores acknowledged
      stamp(6);
    }
  }
};

// lss_pack8 as the vector type the write-through buffer store takes
__device__ __forceinline__ u32x4 ks_pack8(const float (&v)[8]) {
  const uint4 o = lss_pack8(v);
  return (u32x4){o.x, o.y, o.z, o.w};
}

// epilogue constants of a lane's 8 consecutive channels ch .. ch + 7 (null scale: 1, null shift: 0)
__device__ __forceinline__ void ks_load_affine(const float* scale, const float* shift, int ch, float (&sc)[8], float (&sh)[8]) {
  f32x4 s0 = {1.f, 1.f, 1.f, 1.f}, s1 = s0, h0 = {0.f, 0.f, 0.f, 0.f}, h1 = h0;
  if (scale) { s0 = *reinterpret_cast<const f32x4*>(scale + ch); s1 = *reinterpret_cast<const f32x4*>(scale + ch + 4); }
  if (shift) { h0 = *reinterpret_cast<const f32x4*>(shift + ch); h1 = *reinterpret_cast<const f32x4*>(shift + ch + 4); }
#pragma unroll
  for (int i = 0; i < 4; ++i) { sc[i] = s0[i]; sc[4 + i] = s1[i]; sh[i] = h0[i]; sh[4 + i] = h1[i]; }
}

// The K parts meet through LDS - the FOREIGN ones only.  Wave (kp, ph) finishes the tiles j = kp, kp + NKW, .. of its
// pixel part; it keeps its own accumulators of those tiles in registers and writes to LDS only the tiles another wave
// finishes (the part[] layout is the one of the full exchange, a wave's own cells are simply never written or read).
// So that "the tiles a wave finishes" are the same REGISTERS in every wave, each wave walks the pixel tiles of its part
// rotated by its kp: accumulator slot i holds tile (i + kp) mod PXT.  The finished tiles are then the slots 0, NKW,
// 2 NKW, .. (slot k NKW is tile kp + k NKW; where that is >= PXT the rotation has wrapped to a tile another wave
// finishes and the slot is sent like the others) - no register is chosen at run time, one copy of the code serves all
// waves, and what depends on kp is addresses.
__device__ __forceinline__ int ks_slot_tile(int slot, int kp, int pxt) {
  const int t = slot + kp;
  return t >= pxt ? t - pxt : t;
}

// per-lane patch offsets of a wave's pixel tiles by slot: pixel n of tile t of the pixel part is pixel pl0 + 16 t of the
// block (pl0 = first pixel of the part + n), x_first + that many pixels into image rows of W pixels; a patch row is
// rowpitch positions.  Pixels past the block's end (npx pixels) read its last one.
template <int PXT>
__device__ __forceinline__ void ks_slot_offsets(int (&ab)[PXT], int kp, int pl0, int x_first, int npx, int W,
                                                int rowpitch, int laneoff) {
  const int plast = npx - 1;
  const int yl = (x_first + plast) / W, xl = x_first + plast - yl * W;   // wave-uniform
  const int y0 = (x_first + pl0) / W, x0 = x_first + pl0 - y0 * W;       // tile 0: where the rotation wraps to
  int t = ks_slot_tile(0, kp, PXT);                                      // slot 0 (kp can be PXT: three tiles, four K parts)
  int pl = pl0 + t * 16;
  int y = (x_first + pl) / W, x = x_first + pl - y * W;
#pragma unroll
  for (int i = 0; i < PXT; ++i) {
    const bool live = pl < npx;
    ab[i] = ((live ? y : yl) * rowpitch + (live ? x : xl)) * 32 + laneoff;
    pl += 16; x += 16;
    if (x >= W) { x -= W; ++y; }
    if (++t == PXT) { t = 0; pl = pl0; x = x0; y = y0; }   // wave-uniform
  }
}

// the K parts of one (tile, channel tile, lane) cell meet: own is the finishing wave's part, g[] the NKW - 1 foreign
// parts in the order of their kp; POS = the place of the own part among them.  Summed in the fixed order kp = 0 ..
// NKW - 1 with the own part at its own position: the fp32 adds of a sum over all NKW parts read from LDS.
template <int NKW, int POS>
__device__ __forceinline__ f32x4 ks_sum_parts(const f32x4& own, const f32x4 (&g)[NKW - 1]) {
  f32x4 sum = POS == 0 ? own : g[0];
#pragma unroll
  for (int q = 1; q < NKW; ++q) {
    const f32x4 pv = q == POS ? own : g[q > POS ? q - 1 : q];
#pragma unroll
    for (int i = 0; i < 4; ++i) sum[i] += pv[i];
  }
  return sum;
}

// all NKW parts of a cell from LDS (p0 is part kp = 0, part kp lies kstride further), summed in the same fixed order:
// the full exchange, kept where keeping the own part in registers did not pay (stride-2 mode with four K parts)
template <int NKW>
__device__ __forceinline__ f32x4 ks_sum_lds(const f32x4* p0, int kstride) {
  f32x4 sum = p0[0];
#pragma unroll
  for (int k = 1; k < NKW; ++k) {
    const f32x4 pv = p0[k * kstride];
#pragma unroll
    for (int i = 0; i < 4; ++i) sum[i] += pv[i];
  }
  return sum;
}

// f(POS) for the wave's kp, a wave-uniform branch around the adds alone.  kp = 0 and kp = 1 share POS = 0: they differ
// in the order of the operands of the FIRST add only, and a + b is b + a bit for bit - so two K parts need no branch.
template <int NKW, class F>
__device__ __forceinline__ void ks_for_pos(int kp, F&& f) {
  if constexpr (NKW == 2) f(std::integral_constant<int, 0>{});
  else if (kp < 2) f(std::integral_constant<int, 0>{});
  else if (kp == 2) f(std::integral_constant<int, 2>{});
  else f(std::integral_constant<int, 3>{});
}

// the epilogue of 8 consecutive channels: fma(v, scale, shift) (+ the residual pair words rv) -> ReLU -> bf16; one
// function for the stride-1 and the stride-2 kernels, and the contraction WRITTEN OUT so that the bits do not hang on
// what the optimiser fuses.  RES = false: no add at all - adding 0.f would turn -0.f into 0.f.  split0: channel 0 of
// the eight rounds its product before the shift is added.  That is what conv1's output (y) of the stride-2 kernel has
// computed since the kernel exists - its `v * sc + sh` was compiled to FMAs except for the first element of every group
// of eight, which the SLP vectoriser paired with a K-part add (v_mul, then v_pk_add) - and outputs do not move here.
// A change that is allowed to move bits should delete split0 and fuse every channel.
template <bool RES>
__device__ __forceinline__ u32x4 ks_finish8(float (&v)[8], const float (&sc)[8], const float (&sh)[8], const uint4& rv,
                                            bool relu, bool split0) {
  const unsigned int ru[4] = {rv.x, rv.y, rv.z, rv.w};
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    float r;
    if (split0 && i == 0) {
#pragma clang fp contract(off)
      const float p = v[i] * sc[i];
      r = p + sh[i];
    } else {
      r = __builtin_fmaf(v[i], sc[i], sh[i]);
    }
    if constexpr (RES) r += lss_bf2f((unsigned short)((i & 1) ? ru[i >> 1] >> 16 : ru[i >> 1] & 0xffff));
    v[i] = relu ? fmaxf(r, 0.f) : r;
  }
  return ks_pack8(v);
}

struct KsArgs {
  const unsigned short* x;        // (B, H, W, Cin) bf16 NHWC
  const unsigned char* w;         // lss_conv2d_pack_weights_ks
  const float* scale;             // folded BatchNorm (or null: 1)
  const float* shift;             // (or null: 0)
  const unsigned short* residual; // (B, H, W, Cout) bf16 NHWC or null
  unsigned short* y;              // (B, H, W, Cout) bf16 NHWC
  int B, H, W, Cin, Cout, relu, wt;
  int PB;                         // pixels per workgroup
  int npb;                        // pixel blocks per image
  int nposp;                      // patch positions per chunk, padded to a multiple of 32
  int ncb;                        // 32-channel output blocks
  unsigned long long* stamps;     // KsStamps base, or null
};

// KSW: k-steps (32 input channels x one tap) per wave; NKW: K parts; PXT: 16-pixel tiles per wave.  NKW * NPW = 4 waves.
template <int KSW, int NKW, int PXT>
__global__ __launch_bounds__(256, 1) void conv_ks_kernel(const KsArgs a) {
  static_assert(KSW % 9 == 0 && (NKW == 4 || NKW == 2), "a wave's K part is whole chunks of nine taps");
  static_assert(PXT >= NKW - 1, "ks_slot_tile: slot + kp < 2 PXT");
  constexpr int NPW = 4 / NKW;          // pixel parts
  constexpr int CPW = KSW / 9;          // 32-channel chunks per wave
  constexpr int NT = PXT * NPW;         // pixel tiles of the workgroup
  extern __shared__ __attribute__((aligned(1024))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kp = wave % NKW, ph = wave / NKW;  // K part, pixel part
  const int n = lane & 15, kq = lane >> 4;
  KsStamps st = {a.stamps, tid};
  st.stamp(0);

  // ---- which block: XCD-aware order, channel blocks of one pixel block adjacent (they share the input patch) ----
  const int t = lss_xcd_order(blockIdx.x, gridDim.x);
  const int cb = t % a.ncb;
  const int pbg = t / a.ncb;
  const int b = pbg / a.npb, pb = pbg - b * a.npb;
  const int HW = a.H * a.W, WP = a.W + 2;
  const int p0 = pb * a.PB;                       // first pixel of the block (flattened, inside image b)
  const int y_first = p0 / a.W;                   // patch row 0 = image row y_first - 1

  // ---- input patch -> LDS: the identity map with a one-pixel halo ----
  ks_fill_patch<NKW * KSW / 9>(smem, a.x + (size_t)b * HW * a.Cin, a.Cin, a.H, a.W, KS_ROWS, WP, a.nposp, wave, lane,
                               [&](int pr, int pc, int& iy, int& ix) { iy = y_first - 1 + pr; ix = pc - 1; });

  // ---- weights: this wave's KSW x 2 A fragments, straight into registers (coalesced 1-KiB loads) ----
  // Only the first WPRE k-steps are requested here; the main phase requests k-step s + WPRE while it computes k-step s
  // (two 1-KiB loads per 10-20 MFMAs: nothing next to the LDS-DMA burst of the prologue).  The prologue is a fill-rate
  // problem - every CU pulls its patch AND its 72-144 KiB of weights at once, ~70 GB/s per CU - so bytes that can
  // arrive during the MFMAs should: with everything requested up front (-DKS_WPRE_ALL, the first form of this kernel)
  // kernel entry -> operands landed took 3.0-3.6 us of the 7-9.  (Requesting the tail here WITHOUT waiting for it cannot be
  // written with the LDS-DMA builtin - hipcc drains vmcnt(0) at the first use of any load while a piece is outstanding -
  // and would buy 0.12-0.20 us of the main phase at most: DESIGN.md section 4e, profiles/r20_ks_tile2d_ab.txt.)
#ifdef KS_WPRE_ALL
  constexpr int WPRE = KSW;
#else
  constexpr int WPRE = KSW >= 18 ? 8 : 5;
#endif
  bf16x8 wf[KSW][2];
  const unsigned char* wp = a.w + ((size_t)(cb * NKW + kp) * KSW * 2) * 1024 + lane * 16;
  auto load_w = [&](int s) {
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) wf[s][ct] = *reinterpret_cast<const bf16x8*>(wp + (s * 2 + ct) * 1024);
  };
#pragma unroll
  for (int s = 0; s < WPRE; ++s) load_w(s);

  // ---- per-lane patch offsets of the wave's pixel tiles (pixel n of the tile in slot i; tap (ky, kx) adds (ky WP + kx)
  // 64) ---- and the residual pieces of the tiles this wave will finish (requested now: long landed when the epilogue
  // wants them)
  const int npx = min(a.PB, HW - p0);
  int ab[PXT];
  ks_slot_offsets<PXT>(ab, kp, ph * PXT * 16 + n, p0 - y_first * a.W, npx, a.W, WP,
                       (kq >> 1) * a.nposp * 32 + (kq & 1) * 16);
  st.stamp(1);  // every request (weights, patch pieces) has been issued
  constexpr int NOWN = (PXT + NKW - 1) / NKW;   // tiles a wave finishes: j = kp, kp + NKW, ...
  const int ch = cb * 32 + kq * 8;             // this lane's 8 consecutive output channels
  // (bounds-checked buffer loads, no branch: a null residual is an empty buffer, a dead tile or pixel an offset past
  // its end - both read zeros.  A load under a branch made hipcc wait for it - vmcnt(0), the whole patch - on the spot.)
  const __amdgpu_buffer_rsrc_t rrsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<unsigned short*>(a.residual), 0, a.residual ? (int)((size_t)a.B * HW * a.Cout * 2) : 0, 0x00020000);
  // ob[k]: byte offset of this lane's 8 channels of its pixel of finished tile k in y (and the residual), or KS_DEAD -
  // a slot past the wave's tiles or a pixel past the block's end
  constexpr int KS_DEAD = 0x7ffffff0;
  int ob[NOWN];
  uint4 rres[NOWN];
#pragma unroll
  for (int k = 0; k < NOWN; ++k) {
    const int j = kp + k * NKW;
    const int pl = (ph * PXT + j) * 16 + n;
    ob[k] = j < PXT && pl < npx ? (int)((((size_t)b * HW + p0 + pl) * a.Cout + ch) * 2) : KS_DEAD;
    const u32x4 rv = __builtin_amdgcn_raw_buffer_load_b128(rrsrc, ob[k], 0, 0);
    rres[k] = make_uint4(rv[0], rv[1], rv[2], rv[3]);
  }
  // epilogue constants of this lane's 8 consecutive channels, requested with everything else: 16 registers through
  // the main phase.  Requested after it - between the two barriers of the exchange, where they used to be - their
  // latency WAS the tail: whatever the exchange did not cover, the epilogue waited for (profiles/r15_ks_tail_ab.txt).
  float sc[8], sh[8];
  ks_load_affine(a.scale, a.shift, ch, sc, sh);
  f32x4 acc[PXT][2];
#pragma unroll
  for (int j = 0; j < PXT; ++j) {
    acc[j][0] = (f32x4){0.f, 0.f, 0.f, 0.f};
    acc[j][1] = (f32x4){0.f, 0.f, 0.f, 0.f};
  }
  lss_wait_vmcnt<0>();  // the patch pieces (and the weight fragments) have landed
  __syncthreads();
  st.stamp(2);

  // ---- main phase: KSW k-steps x PXT pixel tiles x 2 channel tiles, nothing but LDS reads and MFMAs ----
  // ONE wave per SIMD: nobody else hides an LDS round trip, so the pixel fragments of k-step s + 1 are requested while
  // k-step s computes (two fragment sets by k-step parity) - tile j's behind tile j's MFMA pair (KS_READS_INTERLEAVED,
  // above).  The sched_barriers pin that order: left alone hipcc sinks the requests next to their use and waits with
  // lgkmcnt(0) in front of every MFMA pair, i.e. one exposed LDS latency per 32 matrix cycles.
  bf16x8 fb[2][PXT];
  auto load_frag = [&](int buf, int s, int j) {
    const unsigned char* cbase = smem + (size_t)(kp * CPW + s / 9) * a.nposp * KS_POSB;
    const int tap = s % 9;
    fb[buf][j] = *reinterpret_cast<const bf16x8*>(cbase + ab[j] + ((tap / 3) * WP + (tap % 3)) * 32);
  };
  st.main_begin();
#pragma unroll
  for (int j = 0; j < PXT; ++j) load_frag(0, 0, j);
#pragma unroll
  for (int s = 0; s < KSW; ++s) {
    if (s + WPRE < KSW) load_w(s + WPRE);
    if constexpr (KS_READS && !KS_READS_INTERLEAVED) {
      if (s + 1 < KSW)
#pragma unroll
        for (int j = 0; j < PXT; ++j) load_frag((s + 1) & 1, s + 1, j);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int j = 0; j < PXT; ++j) {
#ifdef KS_DIAG_NOMFMA
      asm volatile("" :: "v"(fb[s & 1][j]), "v"(wf[s][0]), "v"(wf[s][1]));
#else
      acc[j][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[s][0], fb[s & 1][j], acc[j][0], 0, 0, 0);
      acc[j][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[s][1], fb[s & 1][j], acc[j][1], 0, 0, 0);
#endif
      if constexpr (KS_READS && KS_READS_INTERLEAVED) {
        if (s + 1 < KSW) load_frag((s + 1) & 1, s + 1, j);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
  }

  // ---- the K parts meet: part[kp][tile][ct][lane] (16 B each), summed in the fixed order kp = 0 .. NKW - 1 ----
  // (a wave writes only the slots another wave finishes; the barrier in front stays: the exchange reuses the patch's LDS)
  st.main_end(acc[0][0], acc[PXT - 1][1]);
  __syncthreads();  // every wave is done reading the patch: its LDS is free
  f32x4* part = reinterpret_cast<f32x4*>(smem);
#pragma unroll
  for (int i = 0; i < PXT; ++i) {
    if (i % NKW == 0 && kp + i < PXT) continue;  // wave-uniform: this wave finishes the slot itself, from its registers
    const int tile = ph * PXT + ks_slot_tile(i, kp, PXT);
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) part[((kp * NT + tile) * 2 + ct) * 64 + lane] = acc[i][ct];
  }
  __syncthreads();
  st.stamp(4);
  // wave (kp, ph) finishes the tiles ph * PXT + j, j = kp + k NKW < PXT: slot k NKW.  Every foreign part of every such
  // tile is requested before the first add (a slot that wrapped reads the last tile's cells and stores nothing).
  const __amdgpu_buffer_rsrc_t yrsrc = __builtin_amdgcn_make_buffer_rsrc(
      a.y, 0, a.wt ? (int)((size_t)a.B * HW * a.Cout * 2) : 0, 0x00020000);
  f32x4 fp[NOWN][2][NKW - 1];
#pragma unroll
  for (int k = 0; k < NOWN; ++k) {
    const int tile = ph * PXT + min(kp + k * NKW, PXT - 1);
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
      for (int m = 0; m < NKW - 1; ++m)
        fp[k][ct][m] = part[(((m < kp ? m : m + 1) * NT + tile) * 2 + ct) * 64 + lane];
  }
  __builtin_amdgcn_sched_barrier(0);
  f32x4 sum[NOWN][2];
  ks_for_pos<NKW>(kp, [&](auto pos) __attribute__((always_inline)) {
#pragma unroll
    for (int k = 0; k < NOWN; ++k)
#pragma unroll
      for (int ct = 0; ct < 2; ++ct) sum[k][ct] = ks_sum_parts<NKW, decltype(pos)::value>(acc[k * NKW][ct], fp[k][ct]);
  });
#pragma unroll
  for (int k = 0; k < NOWN; ++k) {
    float v[8];
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
      for (int i = 0; i < 4; ++i) v[4 * ct + i] = sum[k][ct][i];
    const u32x4 ov = ks_finish8<true>(v, sc, sh, rres[k], a.relu != 0, false);
    if (ob[k] != KS_DEAD) {                              // dead tiles and pixels compute, no store
      if (a.wt) __builtin_amdgcn_raw_buffer_store_b128(ov, yrsrc, ob[k], 0, 16);  // write-through
      else *reinterpret_cast<u32x4*>(reinterpret_cast<unsigned char*>(a.y) + ob[k]) = ov;
    }
  }
  st.drain();
}

// OIHW fp32 -> the kernel's register image, bf16: [co block of 32][K part][k-step][channel tile][lane][8], where k-step
// S = kp * KSW + s covers chunk S / 9 (32 input channels) of tap S % 9, A-fragment lane (kq = lane >> 4, m = lane & 15)
// holds W[co = cb * 32 + 8 (m >> 2) + 4 ct + (m & 3)][ci = 32 chunk + 8 kq .. + 8][tap]
// dgrad = 1: the image of the TRANSPOSED, tap-flipped weights (the input-gradient conv: Cout x Cin here are the
// gradient conv's own output / input channels, w is the forward layer's (Cin, Cout, 3, 3))
__global__ void pack_weights_ks_kernel(const float* __restrict__ w, int Cout, int Cin, unsigned short* __restrict__ out,
                                       int dgrad) {
  const size_t ntot = (size_t)Cout * Cin * 9;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < ntot; e += (size_t)gridDim.x * 256) {
    const int j = e & 7;
    size_t r = e >> 3;
    const int l = r & 63; r >>= 6;
    const int ct = r & 1; r >>= 1;
    const int nks = (Cin >> 5) * 9;        // k-steps of the whole K
    const int S = r % nks;
    const int cb = r / nks;
    const int m = l & 15, kq = l >> 4;
    const int co = cb * 32 + 8 * (m >> 2) + 4 * ct + (m & 3);
    const int ci = (S / 9) * 32 + kq * 8 + j;
    out[e] = lss_f2bf(dgrad ? w[((size_t)ci * Cout + co) * 9 + (8 - S % 9)] : w[((size_t)co * Cin + ci) * 9 + (S % 9)]);
  }
}

// ---- host side shared by the three modes ----
// LSS_CONV_KS=0 switches every mode of this file off (the *_ok functions answer 0)
bool ks_enabled() { return lss_env_on("LSS_CONV_KS"); }

// grid of a weight-pack kernel over n elements (256 threads, grid-stride)
int ks_pack_grid(size_t n) { return (int)((n + 255) / 256 > 4096 ? 4096 : (n + 255) / 256); }

// every pointer 16-byte aligned (null passes)
template <class... P>
bool ks_aligned16(const P*... p) {
  return (lss_aligned(p, 16) && ...);
}

// one launch of kernel K: the dynamic-LDS attribute is set once per instantiation and device
template <auto K, class Args>
int ks_launch(int grid, int lds, const Args& a, hipStream_t st) {
  static bool attr_set[64] = {};
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = -1;
  if (dev < 0 || !attr_set[dev]) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(K), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       KS_LDS_MAX);
    if (e != hipSuccess) return (int)e;
    if (dev >= 0) attr_set[dev] = true;
  }
  hipLaunchKernelGGL(K, dim3(grid), dim3(256), lds, st, a);
  return lss_launch_status();
}

// A plan: is (shape) a case, the launch geometry, and the kernel's arguments with every shape-derived field filled in
// (the entry adds the pointers and flags).
struct KsPlan {
  int ok, lds, grid, variant;  // variant 0: <18, 4, 5> (Cin 256), 1: <9, 4, 10> (128), 2: <9, 2, 10> (64)
  KsArgs a;
};

KsPlan ks_plan(int B, int H, int W, int Cin, int Cout) {
  KsPlan pl = {};
  KsArgs& p = pl.a;
  if (B <= 0 || H <= 0 || W < 4 || Cout <= 0 || Cout % 32 != 0) return pl;
  if (Cin == 256) { pl.variant = 0; p.PB = 80; }
  else if (Cin == 128) { pl.variant = 1; p.PB = 160; }
  else if (Cin == 64) { pl.variant = 2; p.PB = 320; }
  else return pl;
  p.B = B; p.H = H; p.W = W; p.Cin = Cin; p.Cout = Cout;
  const long long HW = (long long)H * W;
  // (a 2-D pixel tile instead of the flattened block - 25 x 13 at Cin 64, 52 KiB of patch against 92 - was built and
  // measured 0.45 us per launch SLOWER: the fill is not priced per byte.  DESIGN.md section 4e)
  if (p.PB > 4 * W + 1) return pl;                   // a pixel block spans at most five image rows
  p.npb = (int)((HW + p.PB - 1) / p.PB);
  p.ncb = Cout / 32;
  p.nposp = (KS_ROWS * (W + 2) + 31) / 32 * 32;
  const int patch = (Cin / 32) * p.nposp * KS_POSB;
  if (patch > 112 * 1024) return pl;                 // (with the 80-KiB partial tiles of the K parts in the same LDS)
  const int ntile = p.PB / 16;
  const int red = (pl.variant == 2 ? 2 : 4) * ntile * 2 * 1024;   // the K parts' partial tiles
  pl.lds = patch > red ? patch : red;
  if (pl.lds > KS_LDS_MAX) return pl;
  const long long grid = (long long)B * p.npb * p.ncb;
  // one workgroup per CU: worth it where the tile kernel's grid leaves the chip under-filled (at most two rounds here)
  if (grid < 64 || grid > 512) return pl;
  if ((long long)B * HW * (Cin > Cout ? Cin : Cout) >= (1LL << 30)) return pl;
  pl.grid = (int)grid;
  pl.ok = 1;
  return pl;
}

// ---------------------------------------------------------------------------------------------------------------------
// Stride-2 mode: the entry of a downsampling BasicBlock (layer2.0 / layer3.0) - conv1 3x3 / stride 2 / pad 1 + BN + ReLU
// AND the 1x1 / stride 2 downsample + BN over the same input - as one launch of the same one-pass form.  K is exactly
// 9 Cin for the 3x3 and Cin for the 1x1 (the phase-plane form on the tile kernel walks 16 (tap, phase) steps for each).
//   * patch: 7 input rows (3 output rows: a pixel block of PB <= 2 Wo + 1 flattened output pixels spans at most three)
//     with the COLUMNS DE-INTERLEAVED BY PARITY while they are filled: a patch row is [E: columns 2 j, j < Wo]
//     [O: columns 2 j - 1, j <= Wo] (pitch 2 Wo + 1 positions; O[0] and, for odd W, O[Wo] come from the zero page).  The B
//     fragment of 16 consecutive output pixels at tap (ky, kx) is then 16 consecutive positions again: lane base
//     2 (oy - r0) pitch + ox, wave-uniform tap offset ky pitch + {Wo, 0, Wo + 1}[kx] - the cell layout and the bank
//     behaviour of the stride-1 kernel;
//   * workgroup = 3 NPW pixel tiles x 64 output channels (four channel tiles) of BOTH outputs; wave (kp, ph) owns the
//     nine taps of 32-channel chunk kp (Cin 64: 2 K parts x 2 pixel halves of 48; Cin 128: 4 K parts x 48 pixels): 36 +
//     4 A fragments in registers, 12 + 12 accumulators;
//   * the 1x1 rides on the centre tap: at k-step 4 the wave holds the B fragments it needs and issues 12 more MFMAs
//     against the downsample's A fragments into the second accumulator set - no LDS read of its own;
//   * both accumulator sets meet through LDS in the fixed order kp = 0 .. NKW - 1 (NKW = 2: the foreign parts of each
//     tile, 48 KiB; NKW = 4: all 96 KiB of partial tiles) and leave
//     through the same epilogue: scale / shift (channels [0, Cout) of the arrays: y, [Cout, 2 Cout): y2), ReLU on y only.
struct KsS2Args {
  const unsigned short* x;        // (B, H, W, Cin) bf16 NHWC
  const unsigned char* w;         // lss_conv2d_pack_weights_ks_s2_dual
  const float* scale;             // (2 Cout) folded BatchNorm of conv1 | downsample (or null: 1)
  const float* shift;             // (or null: 0)
  unsigned short* y;              // (B, Ho, Wo, Cout) bf16 NHWC: act(conv3x3 / 2)
  unsigned short* y2;             // (B, Ho, Wo, Cout): conv1x1 / 2, no activation
  int B, H, W, Cin, Cout, relu;
  int Ho, Wo, pitch;              // patch row pitch in positions: 2 Wo + 1
  int PB, npb, nposp, ncb;        // as KsArgs; ncb: 64-channel output blocks
  unsigned long long* stamps;     // as KsArgs
};

constexpr int KS2_PXT = 3;        // 16-pixel tiles per wave
constexpr int KS2_CT = 4;         // channel tiles per workgroup (64 output channels)

template <int NKW>
__global__ __launch_bounds__(256, 1) void conv_ks_s2_dual_kernel(const KsS2Args a) {
  static_assert(NKW == 4 || NKW == 2, "one 32-channel chunk of nine taps per K part");
  constexpr int NPW = 4 / NKW, PXT = KS2_PXT, CT = KS2_CT, NT = PXT * NPW, NCH = NKW;
  // OWN: the finishing wave keeps its own K part in registers (foreign parts only through LDS, slots rotated by kp, as
  // in the stride-1 kernel).  With four K parts and three tiles a wave finishes at most one tile and the fourth none:
  // measured slower there (profiles/r15_ks_tail_ab.txt), so NKW = 4 keeps the full exchange and tile order.
  constexpr bool OWN = NKW == 2;
  extern __shared__ __attribute__((aligned(1024))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kp = wave % NKW, ph = wave / NKW;
  const int n = lane & 15, kq = lane >> 4;
  KsStamps st = {a.stamps, tid};
  st.stamp(0);

  const int t = lss_xcd_order(blockIdx.x, gridDim.x);
  const int cb = t % a.ncb;
  const int pbg = t / a.ncb;
  const int b = pbg / a.npb, pb = pbg - b * a.npb;
  const int HWo = a.Ho * a.Wo, WP = a.pitch;
  const int p0 = pb * a.PB;                       // first output pixel of the block (flattened, inside image b)
  const int r0 = p0 / a.Wo;                       // patch row 0 = input row 2 r0 - 1

  // ---- input patch -> LDS, columns de-interleaved: position (pr, pc) <- input (2 r0 - 1 + pr, pc < Wo ? 2 pc : 2 (pc - Wo) - 1)
  ks_fill_patch<NCH>(smem, a.x + (size_t)b * a.H * a.W * a.Cin, a.Cin, a.H, a.W, KS_ROWS, WP, a.nposp, wave, lane,
                     [&](int pr, int pc, int& iy, int& ix) {
                       iy = 2 * r0 - 1 + pr; ix = pc < a.Wo ? 2 * pc : 2 * (pc - a.Wo) - 1;
                     });

  // ---- weights: nine 3x3 k-steps (streamed as in the stride-1 kernel) + the 1x1 k-step, four channel tiles each ----
  constexpr int WPRE = 4;
  bf16x8 wf[9][CT], wd[CT];
  const unsigned char* wp = a.w + ((size_t)(cb * NKW + kp) * 10 * CT) * 1024 + lane * 16;
  auto load_w = [&](int s) {
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) wf[s][ct] = *reinterpret_cast<const bf16x8*>(wp + (s * CT + ct) * 1024);
  };
#pragma unroll
  for (int s = 0; s < WPRE; ++s) load_w(s);
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) wd[ct] = *reinterpret_cast<const bf16x8*>(wp + (9 * CT + ct) * 1024);

  const int npx = min(a.PB, HWo - p0);
  const int rot = OWN ? kp : 0;
  int ab[PXT];   // by slot, as in the stride-1 kernel; an output row is two patch rows
  ks_slot_offsets<PXT>(ab, rot, ph * PXT * 16 + n, p0 - r0 * a.Wo, npx, a.Wo, 2 * WP,
                       (kq >> 1) * a.nposp * 32 + (kq & 1) * 16);
  st.stamp(1);
  f32x4 acc[PXT][CT], acc2[PXT][CT];
#pragma unroll
  for (int j = 0; j < PXT; ++j)
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      acc[j][ct] = (f32x4){0.f, 0.f, 0.f, 0.f};
      acc2[j][ct] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
  lss_wait_vmcnt<0>();
  __syncthreads();
  st.stamp(2);

  // ---- main phase: 9 k-steps x PXT pixel tiles x 4 channel tiles, + the 1x1's 4 PXT MFMAs on the centre tap ----
  bf16x8 fb[2][PXT];
  auto load_frag = [&](int buf, int s, int j) {
    const unsigned char* cbase = smem + (size_t)kp * a.nposp * KS_POSB;
    const int ky = s / 3, kx = s % 3;
    const int toff = (ky * WP + (kx == 1 ? 0 : kx == 0 ? a.Wo : a.Wo + 1)) * 32;
    fb[buf][j] = *reinterpret_cast<const bf16x8*>(cbase + ab[j] + toff);
  };
  st.main_begin();
#pragma unroll
  for (int j = 0; j < PXT; ++j) load_frag(0, 0, j);
#pragma unroll
  for (int s = 0; s < 9; ++s) {
    if (s + WPRE < 9) load_w(s + WPRE);
    if constexpr (!KS_READS_INTERLEAVED) {
      if (s + 1 < 9)
#pragma unroll
        for (int j = 0; j < PXT; ++j) load_frag((s + 1) & 1, s + 1, j);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int j = 0; j < PXT; ++j) {
#pragma unroll
      for (int ct = 0; ct < CT; ++ct)
        acc[j][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[s][ct], fb[s & 1][j], acc[j][ct], 0, 0, 0);
      if constexpr (KS_READS_INTERLEAVED) {
        if (s + 1 < 9) load_frag((s + 1) & 1, s + 1, j);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    if (s == 4) {
#pragma unroll
      for (int j = 0; j < PXT; ++j)
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
          acc2[j][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wd[ct], fb[0][j], acc2[j][ct], 0, 0, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
  }

  // ---- the K parts meet: part[output][kp][tile][ct][lane], summed in the fixed order kp = 0 .. NKW - 1 ----
  st.main_end(acc[0][0], acc[PXT - 1][CT - 1]);
  __syncthreads();  // every wave is done reading the patch: its LDS is free
  f32x4* part = reinterpret_cast<f32x4*>(smem);
#pragma unroll
  for (int i = 0; i < PXT; ++i) {
    if (OWN && i % NKW == 0 && kp + i < PXT) continue;  // wave-uniform: finished here, from the registers
    const int tile = ph * PXT + ks_slot_tile(i, rot, PXT);
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      part[(((0 * NKW + kp) * NT + tile) * CT + ct) * 64 + lane] = acc[i][ct];
      part[(((1 * NKW + kp) * NT + tile) * CT + ct) * 64 + lane] = acc2[i][ct];
    }
  }
  // epilogue constants: [output][channel group g of 32][8 consecutive channels cb 64 + 32 g + 8 kq ..] - 64 per lane,
  // requested here: in the prologue they sit in front of its vmcnt(0) and cost the fill 0.3-0.4 us (measured)
  float sc[2][2][8], sh[2][2][8];
#pragma unroll
  for (int o = 0; o < 2; ++o)
#pragma unroll
    for (int g = 0; g < 2; ++g)
      ks_load_affine(a.scale, a.shift, o * a.Cout + cb * 64 + g * 32 + kq * 8, sc[o][g], sh[o][g]);
  __syncthreads();
  st.stamp(4);
  // wave (kp, ph) finishes the tiles ph * PXT + j, j = kp + k NKW < PXT (slot k NKW), both outputs; every foreign part
  // is requested before the first add
  constexpr int NOWN = (PXT + NKW - 1) / NKW;
  if constexpr (!OWN) {
    // full exchange: wave (kp, ph) finishes the tiles ph * PXT + j with j % NKW == kp from the NKW parts in LDS
#pragma unroll
    for (int k = 0; k < NOWN; ++k) {
      const int j = kp + k * NKW;
      if (j >= PXT) break;  // wave-uniform
      const int tile = ph * PXT + j;
      const int pl = tile * 16 + n;
      const bool live = pl < npx;
      const size_t opix = ((size_t)b * HWo + p0 + (live ? pl : 0)) * a.Cout + cb * 64 + kq * 8;
#pragma unroll
      for (int o = 0; o < 2; ++o)
#pragma unroll
        for (int g = 0; g < 2; ++g) {
          float v[8];
#pragma unroll
          for (int tt = 0; tt < 2; ++tt) {
            const f32x4 sum = ks_sum_lds<NKW>(part + ((o * NKW * NT + tile) * CT + 2 * g + tt) * 64 + lane, NT * CT * 64);
#pragma unroll
            for (int i = 0; i < 4; ++i) v[4 * tt + i] = sum[i];
          }
          // (the source form this instantiation has always had, not ks_finish8: written out, the same values compile
          // to ~40 more VALU instructions here, 0.08 us per launch in the kernel trace)
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            v[i] = v[i] * sc[o][g][i] + sh[o][g][i];
            if (o == 0 && a.relu) v[i] = fmaxf(v[i], 0.f);
          }
          if (live) *reinterpret_cast<u32x4*>((o == 0 ? a.y : a.y2) + opix + g * 32) = ks_pack8(v);
        }
    }
    st.drain();
    return;
  }
  f32x4 fp[NOWN][2][CT][NKW - 1];
#pragma unroll
  for (int k = 0; k < NOWN; ++k) {
    const int tile = ph * PXT + min(kp + k * NKW, PXT - 1);
#pragma unroll
    for (int o = 0; o < 2; ++o)
#pragma unroll
      for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int m = 0; m < NKW - 1; ++m)
          fp[k][o][ct][m] = part[(((o * NKW + (m < kp ? m : m + 1)) * NT + tile) * CT + ct) * 64 + lane];
  }
  __builtin_amdgcn_sched_barrier(0);
  f32x4 sum[NOWN][2][CT];
  ks_for_pos<NKW>(kp, [&](auto pos) __attribute__((always_inline)) {
#pragma unroll
    for (int k = 0; k < NOWN; ++k)
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        sum[k][0][ct] = ks_sum_parts<NKW, decltype(pos)::value>(acc[k * NKW][ct], fp[k][0][ct]);
        sum[k][1][ct] = ks_sum_parts<NKW, decltype(pos)::value>(acc2[k * NKW][ct], fp[k][1][ct]);
      }
  });
#pragma unroll
  for (int k = 0; k < NOWN; ++k) {
    const int j = kp + k * NKW;
    const int pl = (ph * PXT + j) * 16 + n;
    const bool live = j < PXT && pl < npx;               // dead tiles and pixels compute on a clamped address, no store
    const size_t opix = ((size_t)b * HWo + p0 + (live ? pl : 0)) * a.Cout + cb * 64 + kq * 8;
#pragma unroll
    for (int o = 0; o < 2; ++o)
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        float v[8];
#pragma unroll
        for (int tt = 0; tt < 2; ++tt)
#pragma unroll
          for (int i = 0; i < 4; ++i) v[4 * tt + i] = sum[k][o][2 * g + tt][i];
        const u32x4 ov = ks_finish8<false>(v, sc[o][g], sh[o][g], make_uint4(0, 0, 0, 0), o == 0 && a.relu, o == 0);
        if (live) *reinterpret_cast<u32x4*>((o == 0 ? a.y : a.y2) + opix + g * 32) = ov;
      }
  }
  st.drain();
}

// w1 (Cout, Cin, 3, 3) + wd (Cout, Cin) fp32 -> the stride-2 kernel's register image, bf16:
// [co block of 64][32-channel chunk kp][k-step s: nine taps, then the 1x1][channel tile ct][lane][8]; A-fragment lane
// (kq, m) of tile ct holds W[co = cb 64 + 32 (ct >> 1) + 8 (m >> 2) + 4 (ct & 1) + (m & 3)][ci = 32 kp + 8 kq .. + 8]
__global__ void pack_weights_ks_s2_dual_kernel(const float* __restrict__ w1, const float* __restrict__ wd, int Cout,
                                               int Cin, unsigned short* __restrict__ out) {
  const size_t ntot = (size_t)Cout * Cin * 10;
  const int nch = Cin >> 5;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < ntot; e += (size_t)gridDim.x * 256) {
    const int j = e & 7;
    size_t r = e >> 3;
    const int l = r & 63; r >>= 6;
    const int ct = r & 3; r >>= 2;
    const int s = r % 10; r /= 10;
    const int kp = r % nch;
    const int cb = r / nch;
    const int m = l & 15, kq = l >> 4;
    const int co = cb * 64 + 32 * (ct >> 1) + 8 * (m >> 2) + 4 * (ct & 1) + (m & 3);
    const int ci = kp * 32 + kq * 8 + j;
    out[e] = lss_f2bf(s < 9 ? w1[((size_t)co * Cin + ci) * 9 + s] : wd[(size_t)co * Cin + ci]);
  }
}

struct KsS2Plan {
  int ok, lds, grid, nkw;
  KsS2Args a;
};

KsS2Plan ks_s2_plan(int B, int H, int W, int Cin, int Cout) {
  KsS2Plan pl = {};
  KsS2Args& p = pl.a;
  if (B <= 0 || H < 2 || W < 4 || Cout <= 0 || Cout % 64 != 0) return pl;
  if (Cin == 128) pl.nkw = 4;
  else if (Cin == 64) pl.nkw = 2;
  else return pl;
  p.B = B; p.H = H; p.W = W; p.Cin = Cin; p.Cout = Cout;
  p.Ho = (H - 1) / 2 + 1; p.Wo = (W - 1) / 2 + 1;
  p.pitch = 2 * p.Wo + 1;
  p.PB = 16 * KS2_PXT * (4 / pl.nkw);
  if (p.PB > 2 * p.Wo + 1) return pl;                // a pixel block spans at most three output rows
  const long long HWo = (long long)p.Ho * p.Wo;
  p.npb = (int)((HWo + p.PB - 1) / p.PB);
  p.ncb = Cout / 64;
  p.nposp = (KS_ROWS * p.pitch + 31) / 32 * 32;
  const int patch = (Cin / 32) * p.nposp * KS_POSB;
  if (patch > 112 * 1024) return pl;
  const int red = 2 * pl.nkw * (p.PB / 16) * KS2_CT * 1024;   // the K parts' partial tiles of both outputs
  pl.lds = patch > red ? patch : red;
  if (pl.lds > KS_LDS_MAX) return pl;
  const long long grid = (long long)B * p.npb * p.ncb;
  if (grid < 64 || grid > 512) return pl;
  if ((long long)B * H * W * Cin >= (1LL << 30) || (long long)B * HWo * Cout >= (1LL << 30)) return pl;
  pl.grid = (int)grid;
  pl.ok = 1;
  return pl;
}

// ---------------------------------------------------------------------------------------------------------------------
// Stem mode: BevEncode.conv1 - 64 -> Cout, 7x7 / stride 2 / pad 3 + folded BN + ReLU - as one pass.  K is exactly
// 49 taps x 2 chunks of 32 channels = 98 k-steps (the phase-plane form on the tile kernel walks 4 x 16 = 64 (phase, tap)
// positions per channel, 15 of them zeros).
//   * workgroup = a TWO-DIMENSIONAL tile of 12 output rows x 16 output columns x 64 output channels (a 7-row halo of
//     whole image rows does not fit LDS); every MFMA pixel tile is one 16-column row segment;
//   * patch: 29 input rows x 37 input columns x 64 channels, filled once by LDS-DMA (zero page outside the image), the
//     COLUMNS DE-INTERLEAVED BY PARITY: a patch row is [E: relative columns 0, 2, .. 36][O: 1, 3, .. 35] (pitch 37), so the B
//     fragment of an output row segment at tap (ky, kx) is 16 consecutive positions: lane base 2 row pitch + n,
//     wave-uniform tap offset ky pitch + (kx even ? kx / 2 : 19 + kx / 2).  Rows stay interleaved: a tile never mixes
//     output rows, so 2 row + ky is an address, not a stride.  Cells as in the other modes ([chunk][16-channel half]
//     [position][32 B]): the same conflict-free 1-KiB reads for every tap shift.  1 088 positions x 128 B = 136 KiB;
//   * the weights (392 KiB per 64 output channels) stream: a rolling window of A fragments in registers, k-step s + 8
//     requested while k-step s computes, straight from a pack that has this image;
//   * work split 2 x 2, no reduction: wave (g, ph) owns channel tiles 2 g, 2 g + 1 and tile rows 6 ph .. 6 ph + 5 and
//     walks the whole K: 6 ds_read_b128 and 2 x 1 KiB of weights for 12 MFMAs per k-step (0.5 KiB of LDS reads per MFMA,
//     the ratio of the other modes; 2 KiB of weights per 12 MFMAs and wave = ~32 B / clk of the CU's 64-B L1 path).
//     Every output element is one wave's sum in one fixed order: bit-reproducible;
//   * epilogue straight from the accumulators: scale / shift / ReLU, 16-B stores of 8 consecutive channels.
constexpr int ST_TH = 12, ST_TW = 16;                    // output tile
constexpr int ST_PR = 2 * ST_TH + 5, ST_PW = 2 * ST_TW + 5;  // patch rows, row pitch in positions (29, 37)
constexpr int ST_NE = ST_TW + 3;                         // even-column plane of a patch row (19), then the odd one (18)
constexpr int ST_NPOSP = (ST_PR * ST_PW + 31) / 32 * 32; // 1 088
constexpr int ST_LDS = 2 * ST_NPOSP * KS_POSB;           // 139 264 B
constexpr int ST_KS = 98;                                // k-steps: S = tap * 2 + chunk
constexpr int ST_WPRE = 8;                               // k-steps of weights in flight
constexpr int ST_PXT = ST_TH / 2;                        // row segments per wave

struct KsStemArgs {
  const unsigned short* x;        // (B, H, W, 64) bf16 NHWC
  const unsigned char* w;         // lss_conv2d_pack_weights_ks_stem
  const float* scale;             // (Cout) folded BatchNorm (or null: 1)
  const float* shift;             // (or null: 0)
  unsigned short* y;              // (B, Ho, Wo, Cout) bf16 NHWC
  int B, H, W, Cout, relu;
  int Ho, Wo, nty, ntx, ncb;      // tiles per image (rows, columns), 64-channel output blocks
  unsigned long long* stamps;     // as KsArgs
};

__global__ __launch_bounds__(256, 1) void conv_ks_stem_kernel(const KsStemArgs a) {
  constexpr int PXT = ST_PXT, Cin = 64;
  extern __shared__ __attribute__((aligned(1024))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = wave & 1, ph = wave >> 1;       // channel half (32 of the 64), row half of the tile
  const int n = lane & 15, kq = lane >> 4;
  KsStamps st = {a.stamps, tid};
  st.stamp(0);

  const int t = lss_xcd_order(blockIdx.x, gridDim.x);
  const int cb = t % a.ncb;
  const int tg = t / a.ncb;
  const int npi = a.nty * a.ntx;
  const int b = tg / npi, ti = tg - b * npi;
  const int ty = ti / a.ntx, tx = ti - ty * a.ntx;
  const int oy0 = ty * ST_TH, ox0 = tx * ST_TW;
  const int iy0 = 2 * oy0 - 3, ix0 = 2 * ox0 - 3;  // input row / column of patch row 0 / relative column 0

  // ---- input patch -> LDS, columns de-interleaved: position (pr, pc) <- input (iy0 + pr, ix0 + (pc < 19 ? 2 pc : 2 (pc - 19) + 1))
  ks_fill_patch<2>(smem, a.x + (size_t)b * a.H * a.W * Cin, Cin, a.H, a.W, ST_PR, ST_PW, ST_NPOSP, wave, lane,
                   [&](int pr, int pc, int& iy, int& ix) {
                     iy = iy0 + pr; ix = ix0 + (pc < ST_NE ? 2 * pc : 2 * (pc - ST_NE) + 1);
                   });

  // ---- weights: the first ST_WPRE k-steps of this wave's two channel tiles; the window never closes ----
  bf16x8 wf[ST_KS][2];
  const unsigned char* wp = a.w + ((size_t)cb * ST_KS * 4 + 2 * g) * 1024 + lane * 16;
  auto load_w = [&](int s) {
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) wf[s][ct] = *reinterpret_cast<const bf16x8*>(wp + (s * 4 + ct) * 1024);
  };
#pragma unroll
  for (int s = 0; s < ST_WPRE; ++s) load_w(s);

  // lane base of row segment 0 of this wave; segment j adds 2 j pitch positions, tap (ky, kx) its wave-uniform offset
  const int ab0 = (2 * (ph * PXT) * ST_PW + n) * 32 + (kq >> 1) * ST_NPOSP * 32 + (kq & 1) * 16;
  st.stamp(1);
  f32x4 acc[PXT][2];
#pragma unroll
  for (int j = 0; j < PXT; ++j) {
    acc[j][0] = (f32x4){0.f, 0.f, 0.f, 0.f};
    acc[j][1] = (f32x4){0.f, 0.f, 0.f, 0.f};
  }
  // epilogue constants of this lane's 8 consecutive channels, requested with everything else
  const int ch = cb * 64 + g * 32 + kq * 8;
  float sc[8], sh[8];
  ks_load_affine(a.scale, a.shift, ch, sc, sh);
  lss_wait_vmcnt<0>();  // the patch pieces have landed
  __syncthreads();
  st.stamp(2);

  // ---- main phase: 98 k-steps x 6 row segments x 2 channel tiles, LDS reads, weight requests and MFMAs only ----
  bf16x8 fb[2][PXT];
  auto load_frag = [&](int buf, int s, int j) {
    const int tap = s >> 1, ky = tap / 7, kx = tap % 7;
    const int toff = (ky * ST_PW + ((kx & 1) ? ST_NE + (kx >> 1) : (kx >> 1))) * 32;
    const unsigned char* cbase = smem + (size_t)(s & 1) * 2 * ST_NPOSP * 32 + ab0 + toff;
    fb[buf][j] = *reinterpret_cast<const bf16x8*>(cbase + j * (2 * ST_PW * 32));
  };
  st.main_begin();
#pragma unroll
  for (int j = 0; j < PXT; ++j) load_frag(0, 0, j);
#pragma unroll
  for (int s = 0; s < ST_KS; ++s) {
    if (s + ST_WPRE < ST_KS) load_w(s + ST_WPRE);
    if constexpr (!KS_READS_INTERLEAVED) {
      if (s + 1 < ST_KS)
#pragma unroll
        for (int j = 0; j < PXT; ++j) load_frag((s + 1) & 1, s + 1, j);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int j = 0; j < PXT; ++j) {
      acc[j][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[s][0], fb[s & 1][j], acc[j][0], 0, 0, 0);
      acc[j][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[s][1], fb[s & 1][j], acc[j][1], 0, 0, 0);
      if constexpr (KS_READS_INTERLEAVED) {
        if (s + 1 < ST_KS) load_frag((s + 1) & 1, s + 1, j);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  st.main_end(acc[0][0], acc[PXT - 1][1]);
  st.stamp(4);  // (no K parts to meet)

  // ---- epilogue: lane (kq, n) holds channels ch .. ch + 7 of pixel (oy0 + 6 ph + j, ox0 + n) ----
  const int ox = ox0 + n;
#pragma unroll
  for (int j = 0; j < PXT; ++j) {
    const int oy = oy0 + ph * PXT + j;
    float v[8];
#pragma unroll
    for (int i = 0; i < 4; ++i) { v[i] = acc[j][0][i]; v[4 + i] = acc[j][1][i]; }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      v[i] = v[i] * sc[i] + sh[i];
      if (a.relu) v[i] = fmaxf(v[i], 0.f);
    }
    if (oy < a.Ho && ox < a.Wo)
      *reinterpret_cast<u32x4*>(a.y + (((size_t)b * a.Ho + oy) * a.Wo + ox) * a.Cout + ch) = ks_pack8(v);
  }
  st.drain();
}

// w (Cout, 64, 7, 7) fp32 -> the stem kernel's register image, bf16: [co block of 64][k-step S = tap * 2 + chunk]
// [channel tile ct][lane][8]; A-fragment lane (kq, m) of tile ct holds
// W[co = cb 64 + 32 (ct >> 1) + 8 (m >> 2) + 4 (ct & 1) + (m & 3)][ci = 32 chunk + 8 kq .. + 8][tap = ky 7 + kx]
__global__ void pack_weights_ks_stem_kernel(const float* __restrict__ w, int Cout, unsigned short* __restrict__ out) {
  const size_t ntot = (size_t)Cout * 64 * 49;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < ntot; e += (size_t)gridDim.x * 256) {
    const int j = e & 7;
    size_t r = e >> 3;
    const int l = r & 63; r >>= 6;
    const int ct = r & 3; r >>= 2;
    const int S = r % ST_KS;
    const int cb = r / ST_KS;
    const int m = l & 15, kq = l >> 4;
    const int co = cb * 64 + 32 * (ct >> 1) + 8 * (m >> 2) + 4 * (ct & 1) + (m & 3);
    const int ci = (S & 1) * 32 + kq * 8 + j;
    out[e] = lss_f2bf(w[((size_t)co * 64 + ci) * 49 + (S >> 1)]);
  }
}

struct KsStemPlan {
  int ok, grid;
  KsStemArgs a;
};

KsStemPlan ks_stem_plan(int B, int H, int W, int Cin, int Cout) {
  KsStemPlan pl = {};
  KsStemArgs& p = pl.a;
  if (B <= 0 || H <= 0 || W <= 0 || Cin != 64 || Cout <= 0 || Cout % 64 != 0) return pl;
  p.B = B; p.H = H; p.W = W; p.Cout = Cout;
  p.Ho = (H - 1) / 2 + 1; p.Wo = (W - 1) / 2 + 1;
  if (p.Ho < ST_TH || p.Wo < ST_TW) return pl;         // at least one whole tile
  p.nty = (p.Ho + ST_TH - 1) / ST_TH; p.ntx = (p.Wo + ST_TW - 1) / ST_TW;
  p.ncb = Cout / 64;
  const long long grid = (long long)B * p.nty * p.ntx * p.ncb;
  // one workgroup per CU in ONE round; below 32 workgroups the tile kernel's smaller tiles spread wider
  if (grid < 32 || grid > 256) return pl;
  if ((long long)B * H * W * Cin >= (1LL << 30) || (long long)B * p.Ho * p.Wo * Cout >= (1LL << 30)) return pl;
  pl.grid = (int)grid;
  pl.ok = 1;
  return pl;
}

}  // namespace

// Is (shape) a case for the K-split one-pass kernel?  3x3 / stride 1 / pad 1, bf16, Cin in {64, 128, 256}, Cout a
// multiple of 32, an image narrow enough for a pixel block to span five rows, and a grid of 64-512 workgroups.
extern "C" int lss_conv2d_ks_ok(int B, int H, int W, int Cin, int Cout) {
  return ks_enabled() && ks_plan(B, H, W, Cin, Cout).ok;
}

extern "C" size_t lss_conv2d_ks_packed_weight_bytes(int Cout, int Cin) {
  if (Cout <= 0 || Cout % 32 != 0 || (Cin != 64 && Cin != 128 && Cin != 256)) return 0;
  return (size_t)Cout * Cin * 9 * 2;
}

extern "C" int lss_conv2d_pack_weights_ks(const float* w_oihw, int Cout, int Cin, void* w_packed, void* stream) {
  LSS_CHECK_PTR(w_oihw); LSS_CHECK_PTR(w_packed);
  if (lss_conv2d_ks_packed_weight_bytes(Cout, Cin) == 0) return LSS_E_SHAPE;
  hipLaunchKernelGGL(pack_weights_ks_kernel, dim3(ks_pack_grid((size_t)Cout * Cin * 9)), dim3(256), 0, lss_stream(stream), w_oihw, Cout, Cin,
                     reinterpret_cast<unsigned short*>(w_packed), 0);
  return lss_launch_status();
}

// weights of the input-gradient conv of a 3x3 / stride-1 layer, K-split image: w_oihw is the FORWARD layer's
// (Cout, Cin, 3, 3); the gradient conv maps Cout -> Cin channels with the taps flipped
extern "C" int lss_conv2d_pack_weights_ks_dgrad(const float* w_oihw, int Cout, int Cin, void* w_packed, void* stream) {
  LSS_CHECK_PTR(w_oihw); LSS_CHECK_PTR(w_packed);
  if (lss_conv2d_ks_packed_weight_bytes(Cin, Cout) == 0) return LSS_E_SHAPE;
  hipLaunchKernelGGL(pack_weights_ks_kernel, dim3(ks_pack_grid((size_t)Cout * Cin * 9)), dim3(256), 0, lss_stream(stream), w_oihw, Cin, Cout,
                     reinterpret_cast<unsigned short*>(w_packed), 1);
  return lss_launch_status();
}

// launcher behind lss_conv2d_fwd when the weights are KS-packed (LSS_W_KS)
int lss_conv_ks_launch(const void* x, const void* w_ks, const float* scale, const float* shift, const void* residual,
                       void* y, int B, int H, int W, int Cin, int Cout, int relu, int wt, hipStream_t st) {
  KsPlan p = ks_plan(B, H, W, Cin, Cout);
  if (!p.ok) return LSS_E_SHAPE;
  if (relu != 0 && relu != 1) return LSS_E_LAYOUT;
  if (!ks_aligned16(x, y, w_ks, residual)) return LSS_E_ALIGN;
  KsArgs& a = p.a;
  a.x = reinterpret_cast<const unsigned short*>(x);
  a.w = reinterpret_cast<const unsigned char*>(w_ks);
  a.scale = scale; a.shift = shift;
  a.residual = reinterpret_cast<const unsigned short*>(residual);
  a.y = reinterpret_cast<unsigned short*>(y);
  a.relu = relu; a.wt = wt;
  a.stamps = lss_env_device_ptr("LSS_KS_STAMPS");
  if (p.variant == 0) return ks_launch<conv_ks_kernel<18, 4, 5>>(p.grid, p.lds, a, st);
  if (p.variant == 1) return ks_launch<conv_ks_kernel<9, 4, 10>>(p.grid, p.lds, a, st);
  return ks_launch<conv_ks_kernel<9, 2, 10>>(p.grid, p.lds, a, st);
}

// Stride-2 mode (conv1 3x3 / 2 + the 1x1 / 2 downsample of a BasicBlock in one launch): is (shape) a case?  bf16, Cin in
// {64, 128}, Cout a multiple of 64, an output 48-63 (Cin 64) / 24-31 (Cin 128) pixels wide - the 7-row patch fits LDS
// and a pixel block of 96 / 48 spans at most three output rows - and a grid of 64-512 workgroups.
extern "C" int lss_conv2d_ks_s2_dual_ok(int B, int H, int W, int Cin, int Cout) {
  return ks_enabled() && ks_s2_plan(B, H, W, Cin, Cout).ok;
}

extern "C" size_t lss_conv2d_ks_s2_dual_packed_weight_bytes(int Cout, int Cin) {
  if (Cout <= 0 || Cout % 64 != 0 || (Cin != 64 && Cin != 128)) return 0;
  return (size_t)Cout * Cin * 10 * 2;
}

extern "C" int lss_conv2d_pack_weights_ks_s2_dual(const float* w1_oihw, const float* wd_oi, int Cout, int Cin,
                                                  void* w_packed, void* stream) {
  LSS_CHECK_PTR(w1_oihw); LSS_CHECK_PTR(wd_oi); LSS_CHECK_PTR(w_packed);
  if (lss_conv2d_ks_s2_dual_packed_weight_bytes(Cout, Cin) == 0) return LSS_E_SHAPE;
  hipLaunchKernelGGL(pack_weights_ks_s2_dual_kernel, dim3(ks_pack_grid((size_t)Cout * Cin * 10)), dim3(256), 0, lss_stream(stream), w1_oihw, wd_oi, Cout,
                     Cin, reinterpret_cast<unsigned short*>(w_packed));
  return lss_launch_status();
}

extern "C" int lss_conv2d_ks_s2_dual_fwd(const void* x, const void* w_packed, const float* scale, const float* shift,
                                         void* y, void* y2, int B, int H, int W, int Cin, int Cout, int relu,
                                         void* stream) {
  LSS_CHECK_PTR(x); LSS_CHECK_PTR(w_packed); LSS_CHECK_PTR(y); LSS_CHECK_PTR(y2);
  KsS2Plan p = ks_s2_plan(B, H, W, Cin, Cout);
  if (!p.ok) return LSS_E_SHAPE;
  if (relu != 0 && relu != 1) return LSS_E_LAYOUT;
  if (!ks_aligned16(x, y, y2, w_packed, scale, shift)) return LSS_E_ALIGN;
  KsS2Args& a = p.a;
  a.x = reinterpret_cast<const unsigned short*>(x);
  a.w = reinterpret_cast<const unsigned char*>(w_packed);
  a.scale = scale; a.shift = shift;
  a.y = reinterpret_cast<unsigned short*>(y);
  a.y2 = reinterpret_cast<unsigned short*>(y2);
  a.relu = relu;
  a.stamps = lss_env_device_ptr("LSS_KS_STAMPS");
  return p.nkw == 4 ? ks_launch<conv_ks_s2_dual_kernel<4>>(p.grid, p.lds, a, lss_stream(stream))
                    : ks_launch<conv_ks_s2_dual_kernel<2>>(p.grid, p.lds, a, lss_stream(stream));
}

// Stem mode (7x7 / stride 2 / pad 3, Cin 64, one launch): is (shape) a case?  bf16, Cout a multiple of 64, at least one
// 12 x 16 tile of outputs, and a grid of 32-256 workgroups (one round; the hires workload's 442 stay on the tile kernel).
extern "C" int lss_conv2d_ks_stem_ok(int B, int H, int W, int Cin, int Cout) {
  return ks_enabled() && ks_stem_plan(B, H, W, Cin, Cout).ok;
}

extern "C" size_t lss_conv2d_ks_stem_packed_weight_bytes(int Cout, int Cin) {
  if (Cout <= 0 || Cout % 64 != 0 || Cin != 64) return 0;
  return (size_t)Cout * Cin * 49 * 2;
}

extern "C" int lss_conv2d_pack_weights_ks_stem(const float* w_oihw, int Cout, int Cin, void* w_packed, void* stream) {
  LSS_CHECK_PTR(w_oihw); LSS_CHECK_PTR(w_packed);
  if (lss_conv2d_ks_stem_packed_weight_bytes(Cout, Cin) == 0) return LSS_E_SHAPE;
  hipLaunchKernelGGL(pack_weights_ks_stem_kernel, dim3(ks_pack_grid((size_t)Cout * Cin * 49)), dim3(256), 0, lss_stream(stream), w_oihw, Cout,
                     reinterpret_cast<unsigned short*>(w_packed));
  return lss_launch_status();
}

extern "C" int lss_conv2d_ks_stem_fwd(const void* x, const void* w_packed, const float* scale, const float* shift,
                                      void* y, int B, int H, int W, int Cin, int Cout, int relu, void* stream) {
  LSS_CHECK_PTR(x); LSS_CHECK_PTR(w_packed); LSS_CHECK_PTR(y);
  KsStemPlan p = ks_stem_plan(B, H, W, Cin, Cout);
  if (!p.ok) return LSS_E_SHAPE;
  if (relu != 0 && relu != 1) return LSS_E_LAYOUT;
  if (!ks_aligned16(x, y, w_packed, scale, shift)) return LSS_E_ALIGN;
  KsStemArgs& a = p.a;
  a.x = reinterpret_cast<const unsigned short*>(x);
  a.w = reinterpret_cast<const unsigned char*>(w_packed);
  a.scale = scale; a.shift = shift;
  a.y = reinterpret_cast<unsigned short*>(y);
  a.relu = relu;
  a.stamps = lss_env_device_ptr("LSS_KS_STAMPS");
  return ks_launch<conv_ks_stem_kernel>(p.grid, ST_LDS, a, lss_stream(stream));
}
