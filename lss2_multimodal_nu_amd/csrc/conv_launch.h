// Internal (not part of the C ABI): the launchers one conv translation unit calls in another.  The defining file and
// the calling file both include this, so a changed signature is a compile error and not a link-time surprise.
#pragma once
#include "lss_common.h"

// linear_mfma.hip.  The 1x1 / stride-1 dispatch of lss_conv2d_fwd (conv_mfma.hip).
int lss_linear_bf16_launch(const void* x, const void* w, const float* scale, const float* shift,
                           const void* residual, void* y, long long M, int N, int K, int act,
                           int out_f32, int group_hw, hipStream_t st);
// linear_mfma.hip, split-K mode.  The transposed-operand weight-gradient GEMM of lss_conv2d_wgrad (conv_grad.hip).
int lss_wgrad_gemm_launch(const void* dyt, const void* const xt[3], float* partial, int M, int N,
                          long long ld, long long split_k, int nsplit, int ntap, long long tap_row,
                          hipStream_t st);

// conv_ring.hip.  lss_conv2d_fwd / lss_conv2d_head_fwd (conv_mfma.hip) when the weights are ring-packed.
int lss_conv_ring_launch(const void* x, const void* x2, const void* w_ring, const float* scale, const float* shift,
                         void* y, const float* head_w, const float* head_b, float* head_out, int head_n, int B, int H,
                         int W, int Cx, int C2, int up, int Cout, int relu, int wt, hipStream_t st);
// conv_ks.hip.  lss_conv2d_fwd (conv_mfma.hip) when the weights are KS-packed.
int lss_conv_ks_launch(const void* x, const void* w_ks, const float* scale, const float* shift, const void* residual,
                       void* y, int B, int H, int W, int Cin, int Cout, int relu, int wt, hipStream_t st);

// conv_wgrad.hip.  The direct weight-gradient kernel (NHWC operands as they lie, transposed reads) behind
// lss_conv2d_wgrad (conv_grad.hip); 0 splits = not a case for it.
int lss_wgrad_direct_splits(int B, int H, int W, int Cin, int Cout);
int lss_wgrad_direct_launch(const void* x, const void* dy, int B, int H, int W, int Cin, int Cout, float* partial,
                            hipStream_t st);
int lss_wgrad_taps4x4_launch(const void* x, const void* dy, int B, int H, int W, int Cin, int Cout, float* partial,
                             hipStream_t st);
