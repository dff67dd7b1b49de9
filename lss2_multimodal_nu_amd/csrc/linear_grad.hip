// K11: the weight gradient of the BEV transformer's linears (replaces the AddmmBackward nodes that `loss.backward()`,
// ref train_vovnet_transformer.py:210, runs for the nn.Linear of ref src/transformer_modules.py:77-84, 170-215).  The
// input gradient of a linear is the forward GEMM on the transposed weight (linear_mfma.hip) and needs nothing here; the
// LayerNorm backward of K11 lies with the other training row kernels in transformer_pointwise.hip.
//
// lss_linear_wgrad      dw[n, k] = sum_t dy[t, n] x[t, k],  db[n] = sum_t dy[t, n]     (y = x W^T + b, bf16 operands)
//   The contraction index is the TOKEN index, the slow dimension of both operands.  As in K9w (conv_wgrad.hip) both
//   tensors are read token-major as they lie and transposed on the way into the matrix core by `ds_read_b64_tr_b16`.
//   Workgroup = one 64 (n) x 64 (k) output tile over one range of tokens; 4 waves.  A stage is 128 tokens: 16 KiB of dy
//   columns n0 .. n0+63 and 16 KiB of x columns k0 .. k0+63.  Wave w owns tokens 32 w .. 32 w + 31 of every stage:
//   8 + 8 transposed reads feed the 4 x 4 tiles of v_mfma_f32_16x16x32_bf16 (64 accumulator registers, 0.5 KiB of LDS
//   per MFMA as in K9w).  The four waves' accumulators are added in wave order through LDS at the end, and the tile goes
//   to the workspace as partial[split][N][K]; linear_wgrad_reduce_kernel adds the splits in split order.
//   Pipeline: plain double buffer.  The global loads of stage s + 1 are issued into registers before the MFMAs of stage
//   s, stored to the other LDS buffer after them, ONE workgroup barrier per stage.  No flag words, nothing to time out.
//   LDS image (both operands, K9w's): token-major, 128 B per token = four 32-B channel tiles, the tile index
//   XOR-swizzled by f(t) = bit1(t) | bit3(t) << 1, so the 8 tokens a 32-lane half reads fall in 8 different 8-bank
//   groups.  LDS = 2 buffers x 2 operands x 16 KiB = 64 KiB (two workgroups per CU); the end-of-kernel reduction reuses it.
//   Tail: tokens at and beyond T are zero-SELECTED in the staging registers (never loaded, never multiplied by zero
//   outside the MFMA): they add exact zeros.  All 256 threads run every transposed read (EXEC all ones); the read
//   addresses are multiples of 8 B.
//   db: the workgroups of k tile 0 add up the dy pieces they stage (from the staging registers, fp32), 32 partial sums
//   per column, added in a fixed order through LDS at the end: db costs no second pass over dy.
//   Split rule (a function of (T, N, K) alone): stages = ceil(T / 128), tiles = (N / 64)(K / 64),
//   want = clamp(512 / tiles, 1, stages), per = ceil(stages / want), splits = ceil(stages / per).  No float atomics.
#include <algorithm>

#include "lss_device.h"

namespace {

constexpr int LG_TOK = 128;           // tokens per stage
constexpr int LG_BLK = 32 * 128;      // 4096 B: 32 tokens x 64 channels
constexpr int LG_OPER = 4 * LG_BLK;   // one operand of a stage
constexpr int LG_BUF = 2 * LG_OPER;   // dy then x
constexpr int LG_MAXWG = 512;         // two workgroups per CU

struct LinWgradArgs {
  const unsigned short* x;   // (T, K) bf16
  const unsigned short* dy;  // (T, N) bf16
  float* part;               // [splits][N][K]
  float* dbp;                // [splits][N]
  int T, N, K;
  int ntk;      // k tiles of the grid (1 when only db is asked for)
  int nstage;   // ceil(T / 128)
  int per;      // stages per split
  int want_dw, want_db;
};

__global__ __launch_bounds__(256) void linear_wgrad_kernel(const LinWgradArgs a) {
  __shared__ __attribute__((aligned(1024))) unsigned char smem[2 * LG_BUF];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ntn = a.N >> 6;
  int bid = blockIdx.x;
  const int kt = bid % a.ntk; bid /= a.ntk;
  const int nt = bid % ntn;
  const int split = bid / ntn;
  const int n0 = nt * 64, k0 = kt * 64;
  const int st0 = split * a.per;
  const int nst = min(a.per, a.nstage - st0);  // >= 1 by construction of the grid
  const bool do_dw = a.want_dw != 0;           // workgroup-uniform, as is do_db
  const bool do_db = a.want_db != 0 && kt == 0;

  // staging: thread = token p32 of each of the stage's four 32-token blocks, 16-B piece c of its 128-B row
  const int p32 = tid >> 3, c = tid & 7;
  const int soff = p32 * 128 + (((c >> 1) ^ lss_tr_swz(p32)) << 5) + (c & 1) * 16;
  uint4 rd[4], rx[4];
  auto fetch = [&](int st) {
    const long long tb = (long long)(st0 + st) * LG_TOK + p32;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long long t = tb + 32 * j;
      const bool ok = t < a.T;
      rd[j] = make_uint4(0u, 0u, 0u, 0u);
      rx[j] = make_uint4(0u, 0u, 0u, 0u);
      if (ok) rd[j] = *reinterpret_cast<const uint4*>(a.dy + (size_t)t * a.N + n0 + 8 * c);
      if (ok && do_dw) rx[j] = *reinterpret_cast<const uint4*>(a.x + (size_t)t * a.K + k0 + 8 * c);
    }
  };
  float dbacc[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) dbacc[e] = 0.f;
  auto put = [&](int buf) {
    unsigned char* b = smem + buf * LG_BUF + soff;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      *reinterpret_cast<uint4*>(b + j * LG_BLK) = rd[j];
      if (do_dw) *reinterpret_cast<uint4*>(b + LG_OPER + j * LG_BLK) = rx[j];
    }
    if (do_db) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const unsigned int w4[4] = {rd[j].x, rd[j].y, rd[j].z, rd[j].w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {  // lss_unpack8's loop with the adds inside (unpacking first moves the schedule)
          dbacc[2 * e] += lss_bf2f((unsigned short)(w4[e] & 0xffffu));
          dbacc[2 * e + 1] += lss_bf2f((unsigned short)(w4[e] >> 16));
        }
      }
    }
  };

  // transposed reads: lane (g, q, p) supplies token 8 g + 4 h + q, channels 16 ct + 4 p .. + 3 and receives channel
  // 16 ct + (lane & 15) at tokens 8 g + 4 h .. + 3 - the 16x16x32 operand's k = 8 g .. 8 g + 7
  const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
  int roff[2][4];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int pa = 8 * g + 4 * h + q;
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) roff[h][ct] = pa * 128 + ((ct ^ lss_tr_swz(pa)) << 5) + p * 8;
  }
  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  fetch(0);
  put(0);
  __syncthreads();
  for (int s = 0; s < nst; ++s) {
    const bool more = s + 1 < nst;
    if (more) fetch(s + 1);
    if (do_dw) {
      const unsigned char* db_ = smem + (s & 1) * LG_BUF + wave * LG_BLK;
      const unsigned char* xb = db_ + LG_OPER;
      bf16x8_t fa[4], fb[4];
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) fa[ct] = lss_tr_frag(db_ + roff[0][ct], db_ + roff[1][ct]);
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) fb[ct] = lss_tr_frag(xb + roff[0][ct], xb + roff[1][ct]);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i], fb[j], acc[i][j], 0, 0, 0);
    }
    // the other buffer was last read in iteration s - 1, which every wave has left (the barrier below)
    if (more) put((s + 1) & 1);
    __syncthreads();
  }

  // the four waves' tiles, added in wave order: red[wave][row n][column k ^ swizzle] fp32 over the staging buffers
  float* red = reinterpret_cast<float*>(smem);
  if (do_dw) {
    const int n = lane & 15;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = i * 16 + 4 * g + r, col = (j * 16 + n) ^ (g << 4);  // ((row >> 2) & 3) == g
          red[wave * 4096 + row * 64 + col] = acc[i][j][r];
        }
    __syncthreads();
    float* out = a.part + (size_t)split * a.N * a.K + (size_t)n0 * a.K + k0;
#pragma unroll
    for (int m = 0; m < 16; ++m) {
      const int e = tid + 256 * m, row = e >> 6, col = e & 63;
      const int pe = row * 64 + (col ^ (((row >> 2) & 3) << 4));
      out[(size_t)row * a.K + col] = ((red[pe] + red[4096 + pe]) + red[8192 + pe]) + red[12288 + pe];
    }
    __syncthreads();
  }
  if (do_db) {
#pragma unroll
    for (int e = 0; e < 8; ++e) red[p32 * 64 + c * 8 + e] = dbacc[e];
    __syncthreads();
    if (tid < 64) {
      float s = 0.f;
      for (int i = 0; i < 32; ++i) s += red[i * 64 + tid];
      a.dbp[(size_t)split * a.N + n0 + tid] = s;
    }
  }
}

__global__ __launch_bounds__(256) void linear_wgrad_reduce_kernel(const float* __restrict__ part,
                                                                  const float* __restrict__ dbp, int S, int NK, int N,
                                                                  float* __restrict__ dw, float* __restrict__ db) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (dw != nullptr && i < NK) dw[i] = lg_sum_splits(part + i, S, (size_t)NK);
  if (db != nullptr && i < N) db[i] = lg_sum_splits(dbp + i, S, (size_t)N);
}

struct LinSplit {
  int nstage, per, S;
};

inline LinSplit lin_split(int T, int N, int K) {
  LinSplit sp;
  sp.nstage = lss_cdiv(T, LG_TOK);
  const int tiles = (N / 64) * (K / 64);
  const int want = std::max(1, std::min(sp.nstage, LG_MAXWG / tiles));
  sp.per = lss_cdiv(sp.nstage, want);
  sp.S = lss_cdiv(sp.nstage, sp.per);
  return sp;
}

}  // namespace

extern "C" int lss_linear_wgrad_ok(int T, int N, int K) {
  if (T < 1 || T > (1 << 22)) return 0;
  if (N < 64 || N > 1024 || K < 64 || K > 1024 || N % 64 != 0 || K % 64 != 0) return 0;
  return 1;
}

extern "C" size_t lss_linear_wgrad_workspace_bytes(int T, int N, int K) {
  if (!lss_linear_wgrad_ok(T, N, K)) return 0;
  const LinSplit sp = lin_split(T, N, K);
  return (size_t)sp.S * ((size_t)N * K + N) * sizeof(float);
}

extern "C" int lss_linear_wgrad(const void* x, const void* dy, int T, int N, int K, void* workspace,
                                size_t workspace_bytes, float* dw, float* db, void* stream) {
  LSS_CHECK_PTR(dy);
  LSS_CHECK_PTR(workspace);
  if (dw != nullptr) LSS_CHECK_PTR(x);
  if (dw == nullptr && db == nullptr) return LSS_E_NULL;
  if (!lss_linear_wgrad_ok(T, N, K)) return LSS_E_SHAPE;
  if (!lss_aligned(x, 16) || !lss_aligned(dy, 16) || !lss_aligned(workspace, 16) || !lss_aligned(dw, 4) ||
      !lss_aligned(db, 4))
    return LSS_E_ALIGN;
  if (workspace_bytes < lss_linear_wgrad_workspace_bytes(T, N, K)) return LSS_E_WORKSPACE;
  const LinSplit sp = lin_split(T, N, K);
  LinWgradArgs a;
  a.x = static_cast<const unsigned short*>(x);
  a.dy = static_cast<const unsigned short*>(dy);
  a.part = static_cast<float*>(workspace);
  a.dbp = a.part + (size_t)sp.S * N * K;
  a.T = T; a.N = N; a.K = K;
  a.ntk = dw != nullptr ? K / 64 : 1;
  a.nstage = sp.nstage;
  a.per = sp.per;
  a.want_dw = dw != nullptr;
  a.want_db = db != nullptr;
  hipStream_t st = lss_stream(stream);
  hipLaunchKernelGGL(linear_wgrad_kernel, dim3(a.ntk * (N / 64) * sp.S), dim3(256), 0, st, a);
  int rc = lss_launch_status();
  if (rc != 0) return rc;
  const int n = std::max(dw != nullptr ? N * K : 0, N);
  hipLaunchKernelGGL(linear_wgrad_reduce_kernel, dim3(lss_cdiv(n, 256)), dim3(256), 0, st, a.part, a.dbp, sp.S, N * K,
                     N, dw, db);
  return lss_launch_status();
}
