// K15  the TXT half of BEV_TXT at inference behind the ASPP: BevPost and the fused heads (include/lss_hip.h, "K15").
//
// bev_post_kernel: crop -> 3x3 conv, stride (2, 1), padding 1 -> folded BatchNorm -> ReLU -> MaxPool (5, 4), fp32.
//   The BEV map is read where it lies through element strides; workgroup = one pooled row of one sample x BP_TW crop
//   columns.  The 11 crop rows x (BP_TW + 2) columns x Cb channels the tile's 5 conv rows read are parked in LDS with
//   the zero padding already in place (a position outside the CROP is zero, whatever the map holds there); a thread
//   then owns one pooled output (channel, column): its 20 conv values are fp32 FMA chains in (channel, ky, kx) order
//   and it keeps their maximum.  No atomics, nothing depends on B.
//
// txt_heads_tile_kernel (launch A): workgroup = (16-pixel tile, slot, sample), 256 threads.
//   1  the embedder's 3x3 conv over image b ncams + cam[slot] on v_mfma_f32_16x16x32_bf16, fragments straight from
//      global memory (the tile's 16 pixels x 256 channels are 8 KB, a tap of weights 16 KB: there is nothing to reuse
//      through LDS).  WEIGHTS are the A operand, so a lane ends with four consecutive channels of one pixel.  Wave w
//      takes channel tile w & 1 and the 32-channel K blocks 4 (w >> 1) .. 4 (w >> 1) + 3 of every live tap; the two K
//      halves are added through LDS, half 0 + half 1.  A tap that leaves the map zero-fills from (row, column) inside
//      ONE image; a tap that cannot reach the map at all (|ky| >= H or |kx| >= W) is skipped.
//   2  scale, shift, ReLU in fp32 - NOT rounded to bf16 - and the tile's bev_post values next to them: V[32 + Cp][16]
//      in LDS, rows of a partial last tile zero.
//   3  the Linear's columns c HW + m of the tile: 16 lanes (the pixels) x 16 groups (channel c = group, group + 16,
//      group + 32), fp32 FMA, eight outputs per pass; the pixel lanes are folded by a butterfly, the groups through LDS
//      in ascending order.  An E-wide fp32 partial goes to the workspace.
// txt_heads_sum_kernel (launch B): workgroup = sample.  y[slot] = bias + the tile partials in ascending tile order,
//   then the predictors, one thread per output, e ascending.
// No float atomics, no workgroup waits for another, no tile shape or order depends on B.
#include "lss_device.h"

namespace {

constexpr int BP_TW = 64;              // crop columns per workgroup of bev_post_kernel (16 pooled columns)
constexpr int BP_ROWS = 11;            // crop rows 10 ho - 1 .. 10 ho + 9 feed conv rows 5 ho .. 5 ho + 4
constexpr int BP_LW = BP_TW + 2;       // staged columns: one of halo each side
constexpr int BP_MAXC = 8, BP_MAXO = 16;
constexpr int TH_EC = 32;              // embedder channels
constexpr int TH_C = 256;              // scene channels
constexpr int TH_TM = 16;              // pixels per tile
constexpr int TH_MAXP = 8, TH_MAXE = 64, TH_MAXSLOT = 8, TH_MAXCLS = 16;
constexpr int TH_EJ = 8;               // linear outputs per pass

struct BevPostArgs {
  const float* x;
  long long sb, sc, sh, sw;
  const float *w, *scale, *shift;
  float* y;
  int h0, w0, Cb, Hc, Wc, Co, Ho, Wo;
};

__global__ __launch_bounds__(256) void bev_post_kernel(BevPostArgs a) {
  __shared__ float xs[BP_MAXC * BP_ROWS * BP_LW];
  __shared__ float ws[BP_MAXO * BP_MAXC * 9];
  const int tid = threadIdx.x;
  const int wt = blockIdx.x, ho = blockIdx.y, b = blockIdx.z;
  const int Cb = a.Cb, Co = a.Co;
  const int r0 = 10 * ho - 1, c0 = wt * BP_TW - 1;  // crop coordinates of the staged corner
  const float* base = a.x + (long long)b * a.sb + (long long)a.h0 * a.sh + (long long)a.w0 * a.sw;
  const bool ch_fast = a.sc < a.sw;  // channels-last memory: neighbouring threads take neighbouring channels
  const int n = Cb * BP_ROWS * BP_LW;
  for (int i = tid; i < n; i += 256) {
    int c, r, col;
    if (ch_fast) {
      c = i % Cb;
      col = (i / Cb) % BP_LW;
      r = i / (Cb * BP_LW);
    } else {
      col = i % BP_LW;
      r = (i / BP_LW) % BP_ROWS;
      c = i / (BP_LW * BP_ROWS);
    }
    const int hh = r0 + r, ww = c0 + col;
    float v = 0.f;  // the padding is around the crop
    if (hh >= 0 && hh < a.Hc && ww >= 0 && ww < a.Wc) v = base[(long long)c * a.sc + (long long)hh * a.sh + (long long)ww * a.sw];
    xs[(c * BP_ROWS + r) * BP_LW + col] = v;
  }
  for (int i = tid; i < Co * Cb * 9; i += 256) ws[i] = a.w[i];
  __syncthreads();
  const int nwl = min(BP_TW / 4, a.Wo - wt * (BP_TW / 4));  // pooled columns of this tile
  for (int item = tid; item < Co * nwl; item += 256) {
    const int co = item / nwl, wl = item - co * nwl;
    const float sc = a.scale[co], sh = a.shift[co];
    const float* wk = ws + co * Cb * 9;
    float m = 0.f;  // every candidate is a ReLU output
    for (int i = 0; i < 5; ++i) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float acc = 0.f;
        for (int c = 0; c < Cb; ++c) {
          const float* xp = xs + (c * BP_ROWS + 2 * i) * BP_LW + 4 * wl + j;
#pragma unroll
          for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) acc = fmaf(xp[ky * BP_LW + kx], wk[c * 9 + ky * 3 + kx], acc);
        }
        m = fmaxf(m, fmaxf(fmaf(acc, sc, sh), 0.f));
      }
    }
    a.y[(((size_t)b * Co + co) * a.Ho + ho) * a.Wo + wt * (BP_TW / 4) + wl] = m;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
struct HeadSet {
  const unsigned short* ew;  // [9][32][256] bf16
  const float *esc, *esh;    // (32)
  const float *lw, *lb;      // (E, (32 + Cp) HW), (E)
};

struct HeadsArgs {
  const unsigned short* scene;  // (B ncams, H, W, 256) bf16
  const float* bev_post;        // (B, Cp, H, W)
  HeadSet set[2];               // front, side
  const float *f1_w, *f1_b, *f2_w, *f2_b, *lr_w, *lr_b;
  float *part, *act, *desc;
  int cams[TH_MAXSLOT];
  int B, ncams, n_slots, H, W, Cp, E, n_act, n_desc_f, ntiles;
};

__global__ __launch_bounds__(256) void txt_heads_tile_kernel(HeadsArgs a) {
  __shared__ __attribute__((aligned(16))) float P[2][TH_EC][TH_TM];  // the two K halves of the conv
  __shared__ float V[TH_EC + TH_MAXP][TH_TM];                        // what the Linear multiplies
  __shared__ float G[16][TH_MAXE];                                   // the channel groups' sums
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tile = blockIdx.x, slot = blockIdx.y, b = blockIdx.z;
  const int H = a.H, W = a.W, HW = H * W, m0 = tile * TH_TM;
  // the set by uniform selects (a dynamic index into the by-value argument would put it on the stack)
  HeadSet hs = a.set[0];
  if (slot != 0) hs = a.set[1];
  int cam = a.cams[0];
#pragma unroll
  for (int s = 1; s < TH_MAXSLOT; ++s)
    if (slot == s) cam = a.cams[s];
  const unsigned short* img = a.scene + ((size_t)b * a.ncams + cam) * HW * TH_C;

  // 1: the conv.  A = weights [channel fr of the tile][k], B = pixels [k][pixel fr], D[channel 4 fq + e][pixel fr]
  {
    const int fr = lane & 15, fq = lane >> 4;
    const int ct = wave & 1, kh = wave >> 1;
    const int m = m0 + fr;
    const int ph = m < HW ? m / W : -4, pw = m < HW ? m - (m / W) * W : 0;  // a row past the image is outside for every tap
    const unsigned short* wl = hs.ew + (size_t)(ct * 16 + fr) * TH_C + kh * 128 + fq * 8;
    f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int ky = t / 3 - 1, kx = t % 3 - 1;
      if ((ky != 0 && H < 2) || (kx != 0 && W < 2)) continue;  // reads zero padding only (uniform)
      const int hh = ph + ky, ww = pw + kx;
      const bool in = hh >= 0 && hh < H && ww >= 0 && ww < W;
      const int hc = min(max(hh, 0), H - 1), wc = min(max(ww, 0), W - 1);  // the address stays inside the image
      const unsigned short* xp = img + (size_t)(hc * W + wc) * TH_C + kh * 128 + fq * 8;
      const unsigned short* wp = wl + (size_t)t * TH_EC * TH_C;
      uint4 xv[4], wv[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        wv[q] = *reinterpret_cast<const uint4*>(wp + q * 32);
        const uint4 v = *reinterpret_cast<const uint4*>(xp + q * 32);
        xv[q] = in ? v : make_uint4(0, 0, 0, 0);
      }
#pragma unroll
      for (int q = 0; q < 4; ++q)
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, wv[q]), __builtin_bit_cast(bf16x8_t, xv[q]),
                                                      acc, 0, 0, 0);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) P[kh][ct * 16 + 4 * fq + e][fr] = acc[e];
  }
  __syncthreads();

  // 2: V = [relu(scale conv + shift) | bev_post], zero in the rows of a partial tile
  const int C = TH_EC + a.Cp;
  for (int i = tid; i < C * TH_TM; i += 256) {
    const int c = i >> 4, p = i & 15, m = m0 + p;
    float v = 0.f;
    if (m < HW) {
      if (c < TH_EC)
        v = fmaxf(fmaf(P[0][c][p] + P[1][c][p], hs.esc[c], hs.esh[c]), 0.f);
      else
        v = a.bev_post[((size_t)b * a.Cp + (c - TH_EC)) * HW + m];
    }
    V[c][p] = v;
  }
  __syncthreads();

  // 3: the Linear over the tile's columns
  {
    const int p = tid & 15, g = tid >> 4, E = a.E;
    const bool live = m0 + p < HW;  // columns past HW do not exist
    const size_t K = (size_t)C * HW;
    float v[3];
    size_t off[3];
    bool on[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int c = g + 16 * k;
      on[k] = live && c < C;
      v[k] = on[k] ? V[c][p] : 0.f;
      off[k] = on[k] ? (size_t)c * HW + m0 + p : 0;
    }
    for (int e0 = 0; e0 < E; e0 += TH_EJ) {
      float wv[TH_EJ][3];
#pragma unroll
      for (int j = 0; j < TH_EJ; ++j) {
        const float* row = hs.lw + (size_t)min(e0 + j, E - 1) * K;
#pragma unroll
        for (int k = 0; k < 3; ++k) wv[j][k] = on[k] ? row[off[k]] : 0.f;
      }
#pragma unroll
      for (int j = 0; j < TH_EJ; ++j) {
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < 3; ++k) s = fmaf(wv[j][k], v[k], s);
        s += __shfl_xor(s, 8, 64);
        s += __shfl_xor(s, 4, 64);
        s += __shfl_xor(s, 2, 64);
        s += __shfl_xor(s, 1, 64);
        if (p == 0 && e0 + j < E) G[g][e0 + j] = s;
      }
    }
  }
  __syncthreads();
  if (tid < a.E) {
    float s = 0.f;
#pragma unroll
    for (int g = 0; g < 16; ++g) s += G[g][tid];
    a.part[(((size_t)b * a.n_slots + slot) * a.ntiles + tile) * a.E + tid] = s;
  }
}

__global__ __launch_bounds__(TH_MAXSLOT * TH_MAXE) void txt_heads_sum_kernel(HeadsArgs a) {
  __shared__ float Y[TH_MAXSLOT][TH_MAXE];
  const int tid = threadIdx.x, b = blockIdx.x, E = a.E;
  {
    const int s = tid / TH_MAXE, e = tid % TH_MAXE;
    if (s < a.n_slots && e < E) {
      const float* p = a.part + ((size_t)b * a.n_slots + s) * a.ntiles * E + e;
      float y = 0.f;
      for (int t = 0; t < a.ntiles; ++t) y += p[(size_t)t * E];
      Y[s][e] = y + (s == 0 ? a.set[0].lb : a.set[1].lb)[e];
    }
  }
  __syncthreads();
  const int n_desc = a.n_desc_f + a.n_slots - 1;
  if (tid < a.n_act + n_desc) {
    const float *w, *y = Y[0];
    float bias;
    float* out;
    if (tid < a.n_act) {  // predictorf2 -> act
      w = a.f2_w + (size_t)tid * E; bias = a.f2_b[tid]; out = a.act + (size_t)b * a.n_act + tid;
    } else if (tid < a.n_act + a.n_desc_f) {  // predictorf1 -> desc[:, :n_desc_f]
      const int j = tid - a.n_act;
      w = a.f1_w + (size_t)j * E; bias = a.f1_b[j]; out = a.desc + (size_t)b * n_desc + j;
    } else {  // predictorlr on side slot s -> desc[:, n_desc_f + s - 1]
      const int s = tid - a.n_act - a.n_desc_f + 1;
      w = a.lr_w; bias = a.lr_b[0]; y = Y[s]; out = a.desc + (size_t)b * n_desc + a.n_desc_f + s - 1;
    }
    float v = 0.f;
    for (int e = 0; e < E; ++e) v = fmaf(w[e], y[e], v);
    *out = v + bias;
  }
}

int heads_shape_ok(int B, int ncams, int n_slots, int H, int W, int Cp, int E, int n_act, int n_desc_f) {
  if (B < 1 || B > 65535 || ncams < 1 || ncams > 64 || n_slots < 1 || n_slots > TH_MAXSLOT) return LSS_E_SHAPE;
  if (H < 1 || W < 1 || H > 1024 || W > 1024 || H * W > 65536) return LSS_E_SHAPE;
  if (Cp < 1 || Cp > TH_MAXP || E < 1 || E > TH_MAXE) return LSS_E_SHAPE;
  if (n_act < 1 || n_act > TH_MAXCLS || n_desc_f < 1 || n_desc_f > TH_MAXCLS) return LSS_E_SHAPE;
  return 1;
}

}  // namespace

extern "C" int lss_bev_post_fwd(const float* x, long long sb, long long sc, long long sh, long long sw, int Hm, int Wm,
                                int h0, int w0, int B, int Cb, int Hc, int Wc, const float* w, const float* scale,
                                const float* shift, int Co, float* y, void* stream) {
  LSS_CHECK_PTR(x); LSS_CHECK_PTR(w); LSS_CHECK_PTR(scale); LSS_CHECK_PTR(shift); LSS_CHECK_PTR(y);
  if (B < 1 || B > 65535 || Cb < 1 || Cb > BP_MAXC || Co < 1 || Co > BP_MAXO) return LSS_E_SHAPE;
  if (Hm < 1 || Wm < 1 || Hm > 65536 || Wm > 65536 || Hc < 1 || Wc < 1 || h0 < 0 || w0 < 0) return LSS_E_SHAPE;
  if ((long long)h0 + Hc > Hm || (long long)w0 + Wc > Wm) return LSS_E_SHAPE;  // the crop lies inside the map
  const int Ho = (((Hc - 1) / 2) + 1) / 5, Wo = Wc / 4;
  if (Ho < 1 || Wo < 1 || Ho > 65535) return LSS_E_SHAPE;
  if (sb < 0 || sc < 0 || sh < 0 || sw < 0) return LSS_E_LAYOUT;
  if (!lss_aligned(x, 4) || !lss_aligned(w, 4) || !lss_aligned(scale, 4) || !lss_aligned(shift, 4) || !lss_aligned(y, 4))
    return LSS_E_ALIGN;
  BevPostArgs a;
  a.x = x; a.sb = sb; a.sc = sc; a.sh = sh; a.sw = sw;
  a.w = w; a.scale = scale; a.shift = shift; a.y = y;
  a.h0 = h0; a.w0 = w0; a.Cb = Cb; a.Hc = Hc; a.Wc = Wc; a.Co = Co; a.Ho = Ho; a.Wo = Wo;
  const dim3 grid((unsigned)lss_cdiv(Wo, BP_TW / 4), (unsigned)Ho, (unsigned)B);
  hipLaunchKernelGGL(bev_post_kernel, grid, dim3(256), 0, lss_stream(stream), a);
  return lss_launch_status();
}

extern "C" int lss_txt_heads_ok(int B, int ncams, int n_slots, int H, int W, int Cp, int E, int n_act, int n_desc_f) {
  return heads_shape_ok(B, ncams, n_slots, H, W, Cp, E, n_act, n_desc_f);
}

extern "C" size_t lss_txt_heads_workspace_bytes(int B, int n_slots, int H, int W, int E) {
  if (heads_shape_ok(B, 1, n_slots, H, W, 1, E, 1, 1) != 1) return 0;
  return (size_t)B * n_slots * lss_cdiv((long long)H * W, TH_TM) * E * sizeof(float);
}

extern "C" int lss_txt_heads_fwd(const lss_txt_heads_desc_t* d, void* stream) {
  LSS_CHECK_PTR(d);
  const void* always[] = {d->scene, d->bev_post, d->front.embed_w, d->front.embed_scale, d->front.embed_shift,
                          d->front.lin_w, d->front.lin_b, d->f1_w, d->f1_b, d->f2_w, d->f2_b, d->workspace, d->act, d->desc};
  const void* side[] = {d->side.embed_w, d->side.embed_scale, d->side.embed_shift, d->side.lin_w, d->side.lin_b, d->lr_w,
                        d->lr_b};
  for (const void* p : always) LSS_CHECK_PTR(p);
  if (heads_shape_ok(d->B, d->ncams, d->n_slots, d->H, d->W, d->Cp, d->E, d->n_act, d->n_desc_f) != 1) return LSS_E_SHAPE;
  if (d->n_slots > 1)  // the side set is read only when a side slot exists
    for (const void* p : side) LSS_CHECK_PTR(p);
  for (int s = 0; s < d->n_slots; ++s)
    if (d->cams[s] < 0 || d->cams[s] >= d->ncams) return LSS_E_SHAPE;
  // 16-byte fragment loads: the scene map and the weight images; 4 bytes for every fp32 operand
  if (!lss_aligned(d->scene, 16) || !lss_aligned(d->front.embed_w, 16) || !lss_aligned(d->side.embed_w, 16))
    return LSS_E_ALIGN;
  for (const void* p : always)
    if (!lss_aligned(p, 4)) return LSS_E_ALIGN;
  for (const void* p : side)
    if (!lss_aligned(p, 4)) return LSS_E_ALIGN;
  if (d->workspace_bytes < lss_txt_heads_workspace_bytes(d->B, d->n_slots, d->H, d->W, d->E)) return LSS_E_WORKSPACE;
  HeadsArgs a;
  const lss_txt_heads_set_t* src[2] = {&d->front, d->n_slots > 1 ? &d->side : &d->front};
  for (int i = 0; i < 2; ++i) {
    a.set[i].ew = static_cast<const unsigned short*>(src[i]->embed_w);
    a.set[i].esc = src[i]->embed_scale;
    a.set[i].esh = src[i]->embed_shift;
    a.set[i].lw = src[i]->lin_w;
    a.set[i].lb = src[i]->lin_b;
  }
  a.scene = static_cast<const unsigned short*>(d->scene);
  a.bev_post = d->bev_post;
  a.f1_w = d->f1_w; a.f1_b = d->f1_b; a.f2_w = d->f2_w; a.f2_b = d->f2_b; a.lr_w = d->lr_w; a.lr_b = d->lr_b;
  a.part = static_cast<float*>(d->workspace);
  a.act = d->act; a.desc = d->desc;
  for (int s = 0; s < TH_MAXSLOT; ++s) a.cams[s] = s < d->n_slots ? d->cams[s] : 0;
  a.B = d->B; a.ncams = d->ncams; a.n_slots = d->n_slots; a.H = d->H; a.W = d->W; a.Cp = d->Cp; a.E = d->E;
  a.n_act = d->n_act; a.n_desc_f = d->n_desc_f;
  a.ntiles = lss_cdiv((long long)d->H * d->W, TH_TM);
  hipLaunchKernelGGL(txt_heads_tile_kernel, dim3((unsigned)a.ntiles, (unsigned)d->n_slots, (unsigned)d->B), dim3(256), 0,
                     lss_stream(stream), a);
  int st = lss_launch_status();
  if (st != 0) return st;
  hipLaunchKernelGGL(txt_heads_sum_kernel, dim3((unsigned)d->B), dim3(TH_MAXSLOT * TH_MAXE), 0, lss_stream(stream), a);
  return lss_launch_status();
}
