"""fp64 references, DERIVED error bounds, cases and planted errors for the per-element tests of the forward convs on the
tile kernel (csrc/conv_mfma.hip: conv_lds_kernel in all its instantiations, conv_direct_kernel) and the ring kernel
(csrc/conv_ring.hip, six instantiations) - tests/test_conv_fwd_gpu.py on the GPU, tests/test_conv_fwd_ref_cpu.py for
this helper itself.  Everything here is fp64 (or an explicit float32 emulation) on the CPU; u = 2^-24; no bound is
measured on a kernel.

The operation.  out = act(scale * conv(xin, w) + shift + residual), xin = x or cat([x2, up(x1)]) with `up` the bilinear
align_corners upsample by an integer factor (blended operand rounded ONCE to bf16 by the bf16 kernels); optionally a
1x1 head behind it: logits[k] = head_b[k] + sum_c head_w[k, c] out[c], fp32 NCHW.

EXACT cases (`kind == "exact"`).  Integer operands (x, x2, residual in [-3, 3], weights in [-2, 2], head weights in
[-2, 2], no scale / shift): every product and every partial sum is a multiple of the operand granularity g and below
2^24 g, so any fp32 summation order gives the same bits (`_assert_exact` proves it from sum |x| |w| / g < 2^24).  The
kernel must `torch.equal` the fp64 value rounded once to the output type (bf16 round to nearest even, as lss_f2bf; fp32
for dt = 0 and the heads).  The tile kernel's head splits activation and head weight into bf16 hi + lo: an integer
below 2^16 splits exactly (hi = 8 leading bits, the remainder has at most 8), so that head is exact too.
The fused upsample is exact under two constructions:
  (a) dyadic ratios: up = 3 and H, W in {3, 11, 43}: (H - 1) / (3 H - 1) = 1/4, 5/16, 21/64.  fl(ry) is exact,
      fl(ry * iy) is exact, the fraction is a multiple of 2^-6 (so the 16-bit fixed point holds it), the four weights
      and the four-term sum have at most 12 + 3 bits: all exact in fp32.  `blend_f32` (the kernels' arithmetic in
      float32) must equal the fp64 blend bit for bit, which `_virtual_input` asserts for every such case.  The blended
      operand then has granularity 2^-8 (11 x 11) or 2^-10 (11 x 43) before AND after its bf16 rounding.
  (b) x1 constant per (image, channel): weights that sum to 1 within a few ulp blend a small integer c to within a few
      ulp of c, which rounds to c (again asserted on `blend_f32`).  Any `up`; covers up = 2, 4 and the ring's 2 x 2-tile
      layout whose sizes are never dyadic.  x2 carries the spatial information there.

BOUND cases (`kind == "bound"`): bf16-valued randn operands, scale in [0.5, 1.5], shift ~ 0.1 randn.
  dot product   |acc - ref| <= (K + 2) u S, S = sum |x w| over the K = taps * Cin terms, any order (depth_head_ref).
  epilogue      both kernels evaluate act(acc * scale + shift (+ residual)) (conv_mfma.hip: `acc * sc + sh` staged in
                fp32, then `v += residual`, then the activation, then ONE bf16 rounding; conv_ring.hip:690: the same
                without a residual):  E_pre = |scale| E_acc + 2 u (|scale| (|acc| + E_acc) + |shift|),
                E_t = E_pre + u (|pre| + E_pre + |residual|); ReLU is 1-Lipschitz.  bf16 output: the exact half ulp
                (`bf16_out_bound`).
  head          tile kernel (conv_mfma.hip: head_mfma): the fp32 activation is NOT rounded to bf16; activation and head
                weight are each split x = hi + lo (+ e_x), |lo| <= 2^-8 |x|, |e_x| <= 2^-8 |lo| <= 2^-16 |x|, and
                hi hi + hi lo + lo hi is accumulated in fp32: the dropped lo lo and the two e terms are at most
                3 * 2^-16 (1 + 2^-7) |x w| per product; 3 Cout products + bias:
                    E = sum |hw| E_act + (3.1 * 2^-16 + (3 Cout + 3) u) S_h,   S_h = sum |hw| (|act| + E_act) + |hb|.
                ring kernel (conv_ring.hip:725-770): fp32 FMAs of the fp32 activation, shuffles, one LDS exchange:
                    E = sum |hw| E_act + (Cout + 3) u S_h.
  fused upsample  a bound that allows every blended operand half a bf16 ulp is useless (10 % of an output), so the
                operands are PINNED: v = the fp64 blend, dv = its pre-rounding error bound, an operand is AMBIGUOUS
                when bf16(v - dv) != bf16(v + dv), every other has one possible value:
                    E_acc = (K + 2) u S + sum over ambiguous k of |w_k| (bf16(v + dv) - bf16(v - dv)).
                dv.  The kernels take sy = fl(ry * iy), ry = fl((H - 1) / (Hin - 1)): two roundings, |sy' - sy| <=
                2 u sy (1 + u) <= 2.1 u (H - 1).  y0 = (int) sy' and sy' - y0 is exact.  The fraction is stored as
                wy = (unsigned)(f * 65536 + 0.5), clamped to 65535: the fp32 sum moves it by at most 2^-8 units, the
                truncation rounds to nearest (1/2 unit = 2^-17), the clamp costs at most one unit where f >= 1 - 2^-17:
                |ly' - ly| <= delta_y = 2^-16 + 2^-23 + 2.1 u (H - 1), the same for x.  (conv_direct_kernel keeps the
                unquantised fraction: a smaller error.)  The interpolant is continuous and piecewise linear; inside a
                cell |dv / dly| <= the range of the four corners, and where the true fraction lies within delta of 0
                or 1 the computed cell may be the neighbour, so there the range runs over the 4 x 4 neighbourhood:
                    dv = (delta_y + delta_x) range + 32 u qmax,   qmax = the largest corner magnitude.
                32 u qmax covers the arithmetic of either form.  Four-weight form (tile MODE 1 and ring): the weights
                w11 = lx ly, w10 = ly - w11, w01 = lx - w11, w00 = 1 - lx - ly + w11 carry absolute errors of at most
                u, 2u, 2u, 4u (16 u qmax in the sum at the very most), the product and three FMAs at most
                4 u sum w |q| <= 4 u qmax.  Lerp form (conv_direct_kernel): top = a + lx (b - a) is a difference, a
                product and a sum of magnitudes up to 2 qmax, 2 qmax, 3 qmax: 7 u qmax, the same for bot, and
                top + ly (bot - top) adds 14 + 2 + 2 + 3 u qmax: 28 u qmax.
                Condition (asserted by the CPU test on every committed case, not a measurement): at most
                AMBIGUOUS_CAP = 5 % of the blended operands are ambiguous.  randn x1 gives 11 - 19 %; the cases use
                x1 = a per-channel offset of magnitude in [1, 3] + 0.25 randn (below 1 %).
                dt = 0 rounds nothing: E_acc = (K + 2) u S + sum |w_k| dv_k.
  BN statistics stats[c] += sum_m raw, stats[Cout + c] += sum_m raw^2 over the M pixels (fp32 partial sums, shuffles and
                atomics in any order, onto the carried accumulator c0): with e = E_acc,
                    E_1 = sum e + (M + 2) u (sum (|raw| + e) + |c0|),
                    E_2 = sum (2 |raw| e + e^2 + u (|raw| + e)^2) + (M + 2) u (sum (|raw| + e)^2 + |c0|).

`check` (depth_head_ref) asserts an elementwise bound and returns the two metrics of `train_node_ref.errors`.

Planted errors (`plant=`): a deliberately wrong copy of the reference; a case that cannot show one raises
`NotExercised`.  The CPU test proves `check` rejects each on a committed case and the exact cases reject it by
inequality.

Which kernel a case reaches.  `tile_inst` / `ring_inst` repeat the dispatch of launch_conv_lds, lss_conv2d_fwd,
lss_conv2d_head_fwd, conv2d_s2_impl, lss_conv2d_ring_ok and lss_conv_ring_launch (workgroup counts, the T22 condition)
and `make_inputs` asserts that the result is the instantiation named in the case table, so a case cannot drift onto
another kernel silently.  The switches of a case (`env`) are read by the library on every call.  The narrow RT = 1
7x7 / 2 stem always takes two taps per step: its one-tap form lds<1,64,2,4,64,1,0,1> is not built, so no case may name
it.
Instantiation names: lds<RT,BN,MODE,KH,KC,KSP,HEAD,TPS>[+src] = conv_lds_kernel<RT, BN, MODE, KH, KH, PAD, KC, KSP,
HEAD, TPS> (+src: the low-res source window staged in LDS); direct<bf16|f32,fused|plain> = conv_direct_kernel;
ring<MODE,HEAD,NSL,T22> = conv_ring_kernel.
"""
import collections
import functools

import numpy as np
import torch
import torch.nn.functional as F

from depth_head_ref import NotExercised, TINY, U32, check  # noqa: F401  (re-exported)
from train_node_ref import errors  # noqa: F401
from transformer_gemm_ref import AMBIGUOUS_CAP, bf16_out_bound, bf16_rn, bf16_trunc, f32_out_bound  # noqa: F401

F32, BF16 = 0, 1
PLANTS = ("edge_column_shifted", "source_row_off_below_first_strip", "align_corners_false", "concat_halves_swapped",
          "pieces_swapped_in_chunk", "last_chunk_dropped_in_last_tile", "shift_before_scale",
          "residual_after_activation", "relu_on_second_output", "phases_01_10_swapped", "head_bias_of_class_0",
          "bf16_truncated")

_FIELDS = ("name kernel inst entry kind B H W Cx C2 up Cout K pad stride residual relu affine head_n dt wpack env x1 "
           "split stats")
Case = collections.namedtuple("Case", _FIELDS)


def _c(name, kernel, inst, entry, kind, B, H, W, Cx, Cout, C2=0, up=1, K=3, pad=1, stride=1, residual=False,
       relu=False, head_n=0, dt=BF16, wpack="plain", env=(), x1=None, split=0, stats=False):
    if x1 is None:
        x1 = "int" if kind == "exact" else ("offset" if up > 1 else "real")
    return Case(name, kernel, inst, entry, kind, B, H, W, Cx, C2, up, Cout, K, pad, stride, residual, relu,
                kind == "bound", head_n, dt, wpack, tuple(sorted(dict(env).items())), x1, split, stats)


RT1, RT2 = ("LSS_CONV_RT", "1"), ("LSS_CONV_RT", "2")
KS0, KS1 = ("LSS_CONV_KSPLIT", "0"), ("LSS_CONV_KSPLIT", "1")
KC32, KC64 = ("LSS_CONV_KC", "32"), ("LSS_CONV_KC", "64")
SRC0, WT0, DIRECT = ("LSS_CONV_SRC", "0"), ("LSS_CONV_WT", "0"), ("LSS_CONV_DIRECT", "1")
E, Bd = "exact", "bound"

# name, kernel, instantiation the case is meant to reach, entry (s1 = ops.conv2d_nhwc, s2 = conv2d_s2_nhwc, dual =
# conv2d_s2_dual_nhwc, head = conv3x3_head_nchw), kind, B, H, W (of x: the low-res source when up > 1), Cx, Cout, ...;
# env = the switches that select the instantiation
CASES = [
    # ---- tile kernel, MODE 0, 3x3 / s1 ------------------------------------------------------------------------------
    # ragged Cout: scalar stores
    _c("t0_narrow_rt1", "tile", "lds<1,64,0,3,64,1,0,1>", "s1", E, 1, 13, 21, 64, 44, env=[RT1]),
    _c("t0_narrow_rt2_res", "tile", "lds<2,64,0,3,64,1,0,1>", "s1", E, 2, 19, 17, 64, 64, env=[RT2], residual=True,
       relu=True),
    _c("t0_wide_rt1_c128", "tile", "lds<1,128,0,3,64,1,0,1>", "s1", E, 1, 11, 23, 128, 72, env=[RT1, KS0]),
    _c("t0_wide_rt1_c128_ksplit", "tile", "lds<1,128,0,3,64,2,0,1>", "s1", E, 1, 11, 23, 128, 72, env=[RT1, KS1]),
    _c("t0_wide_rt1_c256_res", "tile", "lds<1,128,0,3,64,1,0,1>", "s1", E, 2, 9, 19, 256, 128, env=[RT1, KS0],
       residual=True, relu=True),
    _c("t0_wide_rt1_c256_ksplit_res", "tile", "lds<1,128,0,3,64,2,0,1>", "s1", E, 2, 9, 19, 256, 128, env=[RT1, KS1],
       residual=True, relu=True),
    _c("t0_wide_rt2_res", "tile", "lds<2,128,0,3,64,1,0,1>", "s1", E, 2, 9, 37, 64, 136, env=[RT2], residual=True),
    _c("t0_wide_rt2_kc32", "tile", "lds<2,128,0,3,32,1,0,1>", "s1", E, 2, 9, 37, 64, 136, env=[RT2, KC32], relu=True),
    _c("t0_wide_rt2_writeback", "tile", "lds<2,128,0,3,64,1,0,1>", "s1", E, 1, 17, 33, 64, 128, env=[RT2, WT0]),
    # ---- MODE 0, the stride-2 data-gradient forms (weights: ops.pack_conv_weight_s2_dgrad of a (Cx, Cout/4, K, K) conv) ---
    _c("t0_2x2_dgrad", "tile", "lds<1,64,0,2,64,1,0,1>", "s1", E, 2, 9, 13, 64, 64, K=2, pad=1, wpack="s2_dgrad"),
    _c("t0_4x4_dgrad", "tile", "lds<1,128,0,4,64,1,0,1>", "s1", E, 1, 11, 9, 64, 128, K=4, pad=2, wpack="s2_dgrad"),
    _c("t0_4x4_dgrad_rt2", "tile", "lds<2,128,0,4,64,1,0,1>", "s1", E, 1, 11, 9, 64, 128, K=4, pad=2,
       wpack="s2_dgrad", env=[RT2]),
    # ---- MODE 1: fused gather ---------------------------------------------------------------------------------------
    _c("t1_kc32_src_dyadic", "tile", "lds<2,128,1,3,32,1,0,1>+src", "s1", E, 1, 11, 11, 64, 128, C2=64, up=3,
       env=[RT2]),
    _c("t1_kc32_nosrc_dyadic", "tile", "lds<2,128,1,3,32,1,0,1>", "s1", E, 1, 11, 11, 64, 128, C2=64, up=3,
       env=[RT2, SRC0]),
    _c("t1_kc64_dyadic", "tile", "lds<2,128,1,3,64,1,0,1>", "s1", E, 1, 11, 11, 64, 128, C2=64, up=3, env=[RT2, KC64]),
    _c("t1_rt1_dyadic_nox2", "tile", "lds<1,128,1,3,64,1,0,1>", "s1", E, 2, 11, 11, 64, 72, up=3, env=[RT1], relu=True),
    _c("t1_kc32_src_dyadic_wide", "tile", "lds<2,128,1,3,32,1,0,1>+src", "s1", E, 1, 11, 43, 64, 128, up=3, env=[RT2]),
    _c("t1_narrow_rt2_dyadic", "tile", "lds<2,64,1,3,64,1,0,1>", "s1", E, 1, 11, 11, 64, 40, C2=64, up=3, env=[RT2]),
    _c("t1_kc32_src_const_up2", "tile", "lds<2,128,1,3,32,1,0,1>+src", "s1", E, 2, 9, 13, 64, 128, C2=64, up=2,
       env=[RT2], x1="const"),
    _c("t1_kc32_nosrc_const_up4", "tile", "lds<2,128,1,3,32,1,0,1>", "s1", E, 1, 5, 7, 128, 128, C2=64, up=4,
       env=[RT2, SRC0], x1="const", residual=True),
    _c("t1_rt1_const_up2", "tile", "lds<1,128,1,3,64,1,0,1>", "s1", E, 1, 9, 13, 64, 128, C2=64, up=2, env=[RT1],
       x1="const"),
    # ---- MODE 2: stride 2 over phase planes -------------------------------------------------------------------------
    _c("t2_k1", "tile", "lds<1,128,2,1,64,1,0,1>", "s2", E, 2, 17, 21, 64, 72, K=1, pad=0, stride=2),
    _c("t2_k3_res", "tile", "lds<1,64,2,2,64,1,0,1>", "s2", E, 2, 17, 21, 64, 64, K=3, pad=1, stride=2, residual=True,
       relu=True),
    _c("t2_k3_wide_ksplit", "tile", "lds<1,128,2,2,64,2,0,1>", "s2", E, 1, 19, 33, 64, 128, K=3, pad=1, stride=2),
    _c("t2_k3_wide_rt2", "tile", "lds<2,128,2,2,64,1,0,1>", "s2", E, 1, 19, 33, 64, 128, K=3, pad=1, stride=2,
       env=[RT2], residual=True),
    _c("t2_k7_stem_tps2", "tile", "lds<1,64,2,4,64,1,0,2>", "s2", E, 1, 21, 37, 64, 64, K=7, pad=3, stride=2,
       relu=True),
    _c("t2_k7_stem_rt2", "tile", "lds<2,64,2,4,64,1,0,1>", "s2", E, 1, 21, 37, 64, 64, K=7, pad=3, stride=2, env=[RT2]),
    _c("t2_dual", "tile", "lds<1,128,2,2,64,2,0,1>", "dual", E, 2, 17, 23, 64, 192, K=3, pad=1, stride=2, relu=True,
       split=128),
    _c("t2_dual_rt2", "tile", "lds<2,128,2,2,64,1,0,1>", "dual", E, 2, 17, 23, 64, 192, K=3, pad=1, stride=2,
       relu=True, split=128, env=[RT2]),
    # ---- HEAD -------------------------------------------------------------------------------------------------------
    _c("h_c64_n1", "tile", "lds<2,64,0,3,64,1,1,1>", "head", E, 2, 19, 21, 64, 64, head_n=1, relu=True),
    # Wo % 4 == 0: 16-B stores
    _c("h_c128_n4", "tile", "lds<2,128,0,3,64,1,1,1>", "head", E, 1, 13, 36, 64, 128, head_n=4, relu=True),
    # more than 16 classes: the VALU head (head_valu); Cout 64 = 8 lanes per pixel, the reduction without its last step
    _c("h_c128_n17", "tile", "lds<2,128,0,3,64,1,1,1>", "head", E, 1, 9, 17, 64, 128, head_n=17, relu=True),
    _c("h_c64_n20", "tile", "lds<2,64,0,3,64,1,1,1>", "head", E, 1, 9, 17, 64, 64, head_n=20, relu=True),
    # (a head splits its fp32 activation into 8 + 8 bits: integers below 2^16, so the fused head cases use
    # construction (b))
    _c("h_fused_kc32_n4", "tile", "lds<2,128,1,3,32,1,1,1>+src", "head", E, 1, 11, 11, 64, 128, C2=64, up=3, head_n=4,
       relu=True, x1="const"),
    _c("h_fused_kc64_n1", "tile", "lds<2,128,1,3,64,1,1,1>", "head", E, 1, 9, 13, 64, 128, C2=64, up=2, head_n=1,
       relu=True, env=[KC64], x1="const"),
    # ---- conv_direct_kernel -----------------------------------------------------------------------------------------
    # Cin % 64 == 32
    _c("d_bf16_cin96", "direct", "direct<bf16,plain>", "s1", E, 2, 11, 13, 96, 40, residual=True, relu=True),
    _c("d_1x1_narrow", "direct", "direct<bf16,plain>", "s1", E, 2, 9, 15, 64, 24, K=1, pad=0),
    _c("d_1x1_stats", "direct", "direct<bf16,plain>", "s1", E, 1, 9, 15, 64, 64, K=1, pad=0, stats=True),
    _c("d_f32_plain", "direct", "direct<f32,plain>", "s1", E, 2, 9, 11, 24, 20, dt=F32, residual=True, relu=True),
    _c("d_f32_fused_dyadic", "direct", "direct<f32,fused>", "s1", E, 1, 3, 11, 16, 20, C2=8, up=3, dt=F32),
    _c("d_bf16_fused_dyadic", "direct", "direct<bf16,fused>", "s1", E, 1, 11, 11, 64, 72, C2=64, up=3, env=[DIRECT]),
    _c("d_bf16_fused_const_up4", "direct", "direct<bf16,fused>", "s1", E, 1, 5, 7, 64, 40, C2=64, up=4, env=[DIRECT],
       x1="const"),
    # ---- ring kernel: the smallest grids lss_conv2d_ring_ok takes ---------------------------------------------------
    # 7 x 7 ragged strips
    _c("r_plain_one_chunk", "ring", "ring<0,0,8,0>", "s1", E, 8, 27, 131, 32, 128, wpack="ring", relu=True),
    _c("r_plain_writeback", "ring", "ring<0,0,8,0>", "s1", E, 8, 26, 121, 32, 128, wpack="ring", env=[WT0]),
    _c("r_plain_three_chunks_co256", "ring", "ring<0,0,8,0>", "s1", E, 4, 27, 131, 96, 256, wpack="ring"),
    _c("r_plain_dgrad", "ring", "ring<0,0,8,0>", "s1", E, 8, 27, 131, 64, 128, wpack="ring_dgrad"),
    _c("r_plain_head_n3", "ring", "ring<0,1,8,0>", "head", E, 8, 27, 131, 64, 128, wpack="ring", head_n=3, relu=True),
    _c("r_fused_strip_dyadic", "ring", "ring<1,0,7,0>", "s1", E, 7, 11, 43, 32, 128, up=3, wpack="ring"),
    _c("r_fused_strip_const_up4", "ring", "ring<1,0,7,0>", "s1", E, 8, 7, 33, 64, 128, C2=32, up=4, wpack="ring",
       x1="const", relu=True),
    _c("r_fused_strip_head_const_up2", "ring", "ring<1,1,7,0>", "head", E, 8, 13, 65, 96, 128, C2=32, up=2,
       wpack="ring", head_n=2, relu=True, x1="const"),
    _c("r_fused_t22_const", "ring", "ring<1,0,7,1>", "s1", E, 6, 16, 80, 32, 128, C2=32, up=2, wpack="ring",
       x1="const"),
    _c("r_fused_t22_head_const", "ring", "ring<1,1,7,1>", "head", E, 6, 16, 80, 64, 128, up=2, wpack="ring", head_n=4,
       relu=True, x1="const"),
    # ---- derived bounds on real-valued operands: one per family -----------------------------------------------------
    _c("b_t0_rt2_res", "tile", "lds<2,128,0,3,64,1,0,1>", "s1", Bd, 2, 9, 37, 128, 136, env=[RT2], residual=True,
       relu=True),
    _c("b_t0_ksplit_stats", "tile", "lds<1,128,0,3,64,2,0,1>", "s1", Bd, 1, 11, 23, 128, 72, env=[RT1, KS1],
       stats=True),
    _c("b_t0_4x4_dgrad", "tile", "lds<1,128,0,4,64,1,0,1>", "s1", Bd, 1, 11, 9, 64, 128, K=4, pad=2, wpack="s2_dgrad"),
    _c("b_t1_kc32_src_up2", "tile", "lds<2,128,1,3,32,1,0,1>+src", "s1", Bd, 1, 9, 13, 64, 128, C2=64, up=2,
       env=[RT2], relu=True),
    _c("b_t1_kc64_up4", "tile", "lds<2,128,1,3,64,1,0,1>", "s1", Bd, 1, 5, 7, 64, 72, C2=64, up=4, env=[RT2, KC64],
       residual=True),
    _c("b_t2_k1_stats", "tile", "lds<1,128,2,1,64,1,0,1>", "s2", Bd, 2, 17, 21, 64, 72, K=1, pad=0, stride=2,
       stats=True),
    _c("b_t2_k3_stats_res", "tile", "lds<1,64,2,2,64,1,0,1>", "s2", Bd, 2, 17, 21, 64, 64, K=3, pad=1, stride=2,
       stats=True, residual=True, relu=True),
    _c("b_t2_k7_stats", "tile", "lds<1,64,2,4,64,1,0,2>", "s2", Bd, 1, 21, 37, 64, 64, K=7, pad=3, stride=2,
       stats=True, relu=True),
    _c("b_t2_dual", "tile", "lds<1,128,2,2,64,2,0,1>", "dual", Bd, 2, 17, 23, 64, 192, K=3, pad=1, stride=2,
       relu=True, split=128),
    _c("b_h_c128_n4", "tile", "lds<2,128,0,3,64,1,1,1>", "head", Bd, 1, 13, 36, 64, 128, head_n=4, relu=True),
    _c("b_h_fused_kc32_n1", "tile", "lds<2,128,1,3,32,1,1,1>+src", "head", Bd, 1, 9, 13, 64, 128, C2=64, up=2,
       head_n=1, relu=True),
    _c("b_d_1x1_stats", "direct", "direct<bf16,plain>", "s1", Bd, 1, 9, 15, 64, 64, K=1, pad=0, stats=True, relu=True),
    _c("b_d_bf16_cin96", "direct", "direct<bf16,plain>", "s1", Bd, 2, 11, 13, 96, 40, residual=True, relu=True),
    _c("b_d_f32_fused", "direct", "direct<f32,fused>", "s1", Bd, 1, 5, 7, 16, 20, C2=8, up=4, dt=F32, relu=True),
    _c("b_d_bf16_fused", "direct", "direct<bf16,fused>", "s1", Bd, 1, 9, 13, 64, 40, C2=64, up=2, env=[DIRECT]),
    _c("b_r_plain_co256", "ring", "ring<0,0,8,0>", "s1", Bd, 4, 27, 131, 64, 256, wpack="ring", relu=True),
    _c("b_r_plain_head_n4", "ring", "ring<0,1,8,0>", "head", Bd, 8, 27, 131, 32, 128, wpack="ring", head_n=4,
       relu=True),
    _c("b_r_fused_strip_up4", "ring", "ring<1,0,7,0>", "s1", Bd, 8, 7, 33, 32, 128, C2=32, up=4, wpack="ring",
       relu=True),
    _c("b_r_fused_t22_head", "ring", "ring<1,1,7,1>", "head", Bd, 6, 16, 80, 32, 128, C2=32, up=2, wpack="ring",
       head_n=2, relu=True),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
EXACT_CASES = [c for c in CASES if c.kind == "exact"]
BOUND_CASES = [c for c in CASES if c.kind == "bound"]
# the exact MODE 0 / MODE 1 tile cases are run once more on conv_direct_kernel (LSS_CONV_DIRECT=1; the stride-2 and head
# entries have no direct form)
DIRECT_REPEATS = [c for c in EXACT_CASES if c.kernel == "tile" and c.entry == "s1"]


def _cdiv(a, b):
    return -(-a // b)


def _gen(name):
    return torch.Generator().manual_seed(sum((i + 1) * ord(ch) for i, ch in enumerate(name)))


def out_hw(c):
    Hin, Win = c.H * c.up, c.W * c.up
    return (Hin + 2 * c.pad - c.K) // c.stride + 1, (Win + 2 * c.pad - c.K) // c.stride + 1


# ----------------------------------------------------------------------------------------------------------------------
# the dispatch, repeated
# ----------------------------------------------------------------------------------------------------------------------
def _ratio32(n_in, n_out):
    return np.float32(n_in - 1) / np.float32(n_out - 1) if n_out > 1 else np.float32(0)


def tile_inst(c, env=None):
    """The kernel lss_conv2d_fwd / _s2_fwd / _s2_dual_fwd / _head_fwd launches for the case (plain-packed weights)."""
    env = dict(c.env) if env is None else env
    on = lambda k: k not in env or int(env[k]) != 0  # noqa: E731  (lss_env_on)
    fused = c.up > 1 or c.C2 > 0
    Cin = c.Cx + c.C2
    Ho, Wo = out_hw(c)
    ry, rx = _ratio32(c.H, c.H * c.up), _ratio32(c.W, c.W * c.up)
    f32 = np.float32
    src_ok = on("LSS_CONV_SRC") and c.up >= 2 and ry * f32(9) < f32(4.99) and rx * f32(17) < f32(8.99)   # conv_src_lds_ok
    if c.entry == "head":
        assert c.Cout in (64, 128) and c.Cx % 64 == 0 and c.C2 % 64 == 0 and c.head_n <= 64 and c.dt == BF16
        assert c.Cout == 128 or not fused
        kc32 = fused and ("LSS_CONV_KC" not in env or env["LSS_CONV_KC"] == "32")
        return "lds<2,%d,%d,3,%d,1,1,1>%s" % (c.Cout, int(fused), 32 if kc32 else 64, "+src" if kc32 and src_ok else "")
    if c.entry in ("s2", "dual"):
        assert c.Cx % 64 == 0 and (c.K, c.pad) in ((1, 0), (3, 1), (7, 3)) and c.stride == 2 and not fused
        if c.entry == "dual":
            assert 0 < c.split < c.Cout and c.split % 128 == 0 and (c.Cout - c.split) % 8 == 0 and c.K == 3
        mode, KH, cin_k = 2, {1: 1, 3: 2, 7: 4}[c.K], (c.Cx if c.K == 1 else 4 * c.Cx)
    else:
        direct = "direct<%s,%s>" % ("bf16" if c.dt == BF16 else "f32", "fused" if fused else "plain")
        kblock = (64 if fused else 32) if c.dt == BF16 else 8
        assert c.Cx % kblock == 0 and c.C2 % kblock == 0 and c.stride == 1
        tile_ok = c.dt == BF16 and "LSS_CONV_DIRECT" not in env and Cin % 64 == 0
        if tile_ok and (c.K, c.pad) == (3, 1):
            mode, KH = int(fused), 3
        elif tile_ok and not fused and not c.stats and (c.K, c.pad) in ((2, 1), (4, 2)):
            mode, KH = 0, c.K
        elif c.dt == BF16 and (c.K, c.pad) == (1, 0) and not fused and Cin % 32 == 0 and c.Cout >= 64 and not c.stats \
                and "LSS_CONV_DIRECT" not in env:
            return "linear_mfma"
        else:
            return direct
        cin_k = Cin
    tilesX, narrow = _cdiv(Wo, 16), c.Cout <= 64
    th2 = 16 if narrow else 8
    nblk = _cdiv(c.Cout, 64 if narrow else 128)
    rt = 1 if tilesX * _cdiv(Ho, th2) * c.B * nblk < 384 else 2
    if "LSS_CONV_RT" in env:
        rt = 1 if int(env["LSS_CONV_RT"]) == 1 else 2
    if narrow:
        tps = 2 if (rt == 1 and mode == 2 and KH == 4) else 1
        return "lds<%d,64,%d,%d,64,1,0,%d>" % (rt, mode, KH, tps)
    kc32 = mode == 1
    if "LSS_CONV_KC" in env:
        kc32 = env["LSS_CONV_KC"] == "32"
    kc32 = kc32 and mode != 2 and KH == 3 and rt == 2 and c.Cx % 32 == 0 and c.C2 % 32 == 0
    if rt == 2:
        return "lds<2,128,%d,%d,%d,1,0,1>%s" % (mode, KH, 32 if kc32 else 64, "+src" if kc32 and mode == 1 and src_ok else "")
    nwg1 = tilesX * _cdiv(Ho, th2 // 2) * c.B * nblk
    ksplit = mode != 1 and nwg1 <= 256 and (cin_k // 64) % 2 == 0 and cin_k >= 128 and on("LSS_CONV_KSPLIT")
    return "lds<1,128,%d,%d,64,%d,0,1>" % (mode, KH, 2 if ksplit else 1)


def ring_ok(c):
    """lss_conv2d_ring_ok."""
    if c.Cout % 128 or c.Cx % 32 or c.C2 % 32 or (c.head_n > 0 and (c.Cout != 128 or c.head_n > 4)):
        return False
    fused, Hin, Win = c.up > 1 or c.C2 > 0, c.H * c.up, c.W * c.up
    if fused:
        if c.up < 2:
            return False
        ry, rx = _ratio32(c.H, Hin), _ratio32(c.W, Win)
        if int(ry * np.float32(5) + np.float32(0.999)) + 2 > 5 or int(rx * np.float32(21) + np.float32(0.999)) + 2 > 14:
            return False
    strips = c.B * _cdiv(Hin, 4) * _cdiv(Win, 20)
    return strips // 4 * (c.Cout // 128) >= 96


def ring_inst(c):
    """The instantiation lss_conv_ring_launch takes."""
    assert ring_ok(c) and (c.K, c.pad, c.stride, c.dt) == (3, 1, 1, BF16) and not c.residual and not c.stats, c.name
    fused, Hin, Win = c.up > 1 or c.C2 > 0, c.H * c.up, c.W * c.up
    ry, rx = _ratio32(c.H, Hin), _ratio32(c.W, Win)
    t22 = fused and Hin % 8 == 0 and Win % 40 == 0 and int(ry * np.float32(9) + np.float32(0.999)) + 2 <= 7 \
        and int(rx * np.float32(41) + np.float32(0.999)) + 2 <= 23
    return "ring<%d,%d,%d,%d>" % (int(fused), int(c.head_n > 0), 7 if fused else 8, int(t22))


def expected_inst(c, env=None):
    return ring_inst(c) if c.kernel == "ring" else tile_inst(c, env)


# ----------------------------------------------------------------------------------------------------------------------
# inputs
# ----------------------------------------------------------------------------------------------------------------------
def _ints(shape, g, lim):
    return torch.randint(-lim, lim + 1, shape, generator=g).float()


@functools.lru_cache(maxsize=None)
def make_inputs(name):
    """x (B,H,W,Cx), x2 (B,Hin,Win,C2) | None, residual (B,Ho,Wo,Cout) | None in the case's dtype, NHWC; w (fp32 OIHW:
    what the case's pack function is handed); scale, shift (Cout) | None; head_w (n, Cout), head_b (n) | None; stats0
    (2 Cout) | None: the carried accumulator.  Cached: shared, never written to."""
    c = BY_NAME[name]
    assert expected_inst(c) == c.inst, (c.name, expected_inst(c), c.inst)
    g = _gen(name.replace("_ksplit", "").replace("nosrc", "src"))   # on / off pairs share their operands
    tdt = torch.bfloat16 if c.dt == BF16 else torch.float32
    exact = c.kind == "exact"
    Hin, Win = c.H * c.up, c.W * c.up
    Ho, Wo = out_hw(c)
    Cin = c.Cx + c.C2
    if c.x1 == "int":
        x = _ints((c.B, c.H, c.W, c.Cx), g, 3)
    elif c.x1 == "const":
        x = _ints((c.B, 1, 1, c.Cx), g, 3).expand(c.B, c.H, c.W, c.Cx).contiguous()
    elif c.x1 == "offset":
        off = (1.0 + 2.0 * torch.rand(1, 1, 1, c.Cx, generator=g)) * (2.0 * torch.randint(0, 2, (1, 1, 1, c.Cx), generator=g) - 1.0)
        x = off + 0.25 * torch.randn(c.B, c.H, c.W, c.Cx, generator=g)
    else:
        x = torch.randn(c.B, c.H, c.W, c.Cx, generator=g)
    x2 = res = None
    if c.C2:
        x2 = _ints((c.B, Hin, Win, c.C2), g, 3) if exact else torch.randn(c.B, Hin, Win, c.C2, generator=g)
    if c.residual:
        res = _ints((c.B, Ho, Wo, c.Cout), g, 3) if exact else torch.randn(c.B, Ho, Wo, c.Cout, generator=g)
    if c.wpack == "s2_dgrad":      # forward conv (Cx, Cout / 4, Kf, Kf), stride 2; this case runs its data gradient
        wshape = (c.Cx, c.Cout // 4, {2: 3, 4: 7}[c.K], {2: 3, 4: 7}[c.K])
    elif c.wpack == "ring_dgrad":  # forward conv (Cx, Cout, 3, 3); this case runs its data gradient
        wshape = (c.Cx, c.Cout, 3, 3)
    else:
        wshape = (c.Cout, Cin, c.K, c.K)
    if exact:
        wlim = 1 if (c.up == 3 and c.W == 43 and Cin > 128) else 2
        w = _ints(wshape, g, wlim)
    else:
        w = (torch.randn(wshape, generator=g) * (Cin * c.K * c.K) ** -0.5).bfloat16().float() if c.dt == BF16 else \
            torch.randn(wshape, generator=g) * (Cin * c.K * c.K) ** -0.5
    scale = shift = head_w = head_b = stats0 = None
    if c.affine or c.entry in ("dual", "head"):
        if exact:
            scale, shift = torch.ones(c.Cout), torch.zeros(c.Cout)
        else:
            scale, shift = torch.rand(c.Cout, generator=g) + 0.5, 0.1 * torch.randn(c.Cout, generator=g)
    if c.head_n:
        if exact:
            head_w, head_b = _ints((c.head_n, c.Cout), g, 2), _ints((c.head_n,), g, 3)
        else:
            head_w, head_b = torch.randn(c.head_n, c.Cout, generator=g) * c.Cout ** -0.5, torch.randn(c.head_n, generator=g)
    if c.stats:
        stats0 = torch.zeros(2 * c.Cout) if exact else torch.cat([torch.randn(c.Cout, generator=g), torch.rand(c.Cout, generator=g)])
    cast = lambda t: None if t is None else t.to(tdt).contiguous()  # noqa: E731
    return dict(x=cast(x), x2=cast(x2), residual=cast(res), w=w.contiguous(), scale=scale, shift=shift, head_w=head_w,
                head_b=head_b, stats0=stats0)


def effective_weight(c, w):
    """(Cout, Cin, K, K) fp64 of the stride-`c.stride` correlation the kernel runs: the case's weight as its pack
    function lays it out, written here independently of the pack kernels (values rounded to bf16 as they are)."""
    w = w.double() if c.dt == F32 else w.bfloat16().double()
    if c.wpack == "ring_dgrad":   # dX = conv(dY, w^T flipped)
        return w.transpose(0, 1).flip(2, 3).contiguous()
    if c.wpack == "s2_dgrad":
        # csrc/conv_grad.hip: dX[2j + py] = sum_d dY[j - d] w[ky = 2d + py + p], tap t reads dY[j - dmax + t]; the
        # stride-1 conv's own padding is KT / 2, so tap t reads row j - KT / 2 + t: output row j' = j + KT / 2 - dmax
        Co, Ci, Kf, _ = w.shape
        p, KT = {3: 1, 7: 3}[Kf], c.K
        dmax = (Kf - 1 - p) // 2
        out = torch.zeros(2, 2, Ci, Co, KT, KT, dtype=torch.float64)
        for ty in range(KT):
            for tx in range(KT):
                for py in range(2):
                    for px in range(2):
                        ky, kx = 2 * (dmax - ty) + py + p, 2 * (dmax - tx) + px + p
                        if 0 <= ky < Kf and 0 <= kx < Kf:
                            out[py, px, :, :, ty, tx] = w[:, :, ky, kx].t()
        return out.reshape(4 * Ci, Co, KT, KT)
    return w


# ----------------------------------------------------------------------------------------------------------------------
# the fused upsample
# ----------------------------------------------------------------------------------------------------------------------
def _axis64(n_in, n_out):
    """(i0, i1, frac) of align_corners source coordinates o (n_in - 1) / (n_out - 1), exactly (integer arithmetic)."""
    o = np.arange(n_out, dtype=np.int64)
    den = max(n_out - 1, 1)
    num = o * (n_in - 1)
    i0 = num // den
    i1 = np.minimum(i0 + 1, n_in - 1)
    return i0, i1, (num - i0 * den).astype(np.float64) / den


def _axis32(n_in, n_out):
    """The kernels' float32 coordinates and 16-bit fractions (conv_mfma.hip: the g_w set-up of conv_lds_tile, conv_ring.hip:336-341)."""
    r = _ratio32(n_in, n_out)
    s = (r * np.arange(n_out).astype(np.float32)).astype(np.float32)
    i0 = s.astype(np.int64)
    f = (s - i0.astype(np.float32)).astype(np.float32)
    q = np.minimum((f * np.float32(65536.0) + np.float32(0.5)).astype(np.float32).astype(np.int64), 65535)
    return i0, i0 + (i0 < n_in - 1), (q.astype(np.float32) * np.float32(1.0 / 65536.0)).astype(np.float32)


def _corners(x, y0, y1, x0, x1):
    """x (B,H,W,C) -> the four corner tensors (B,Ho,Wo,C)."""
    y0, y1, x0, x1 = (torch.from_numpy(np.asarray(a)) for a in (y0, y1, x0, x1))
    r0, r1 = x[:, y0], x[:, y1]
    return r0[:, :, x0], r0[:, :, x1], r1[:, :, x0], r1[:, :, x1]


def blend64(x, up, align_corners=True):
    """Bilinear upsample of x (B,H,W,C) fp64 by `up`, hand-written gather; returns (v, range, qmax) with range / qmax
    the spread / largest magnitude of the corners an operand may be blended from (module docstring)."""
    B, H, W, C = x.shape
    if not align_corners:
        v = F.interpolate(x.permute(0, 3, 1, 2), scale_factor=up, mode="bilinear", align_corners=False)
        return v.permute(0, 2, 3, 1).contiguous(), None, None
    y0, y1, fy = _axis64(H, H * up)
    x0, x1, fx = _axis64(W, W * up)
    q = _corners(x, y0, y1, x0, x1)
    ly, lx = torch.from_numpy(fy).view(1, -1, 1, 1), torch.from_numpy(fx).view(1, 1, -1, 1)
    v = (1 - ly) * ((1 - lx) * q[0] + lx * q[1]) + ly * ((1 - lx) * q[2] + lx * q[3])
    st = torch.stack(q)
    hi, lo, qmax = st.amax(0), st.amin(0), st.abs().amax(0)
    # where the true fraction is within delta of a cell edge the kernel may blend in the neighbouring cell
    dy, dx = blend_delta(H), blend_delta(W)
    near_y, near_x = (fy < dy) | (fy > 1 - dy), (fx < dx) | (fx > 1 - dx)
    xp = x.permute(0, 3, 1, 2)
    pad = F.pad(xp, (1, 2, 1, 2), mode="replicate")
    big_hi = F.max_pool2d(pad, 4, 1).permute(0, 2, 3, 1)      # [i, j] = max over rows i - 1 .. i + 2, cols j - 1 .. j + 2
    big_lo = -F.max_pool2d(-pad, 4, 1).permute(0, 2, 3, 1)
    big_abs = F.max_pool2d(pad.abs(), 4, 1).permute(0, 2, 3, 1)
    iy, ix = torch.from_numpy(y0), torch.from_numpy(x0)
    near = torch.from_numpy(near_y).view(1, -1, 1, 1) | torch.from_numpy(near_x).view(1, 1, -1, 1)
    hi = torch.where(near, big_hi[:, iy][:, :, ix], hi)
    lo = torch.where(near, big_lo[:, iy][:, :, ix], lo)
    qmax = torch.where(near, big_abs[:, iy][:, :, ix], qmax)
    return v, hi - lo, qmax


def blend_delta(n_in):
    """delta of the module docstring for an axis of n_in source positions."""
    return 2.0 ** -16 + 2.0 ** -23 + 2.1 * U32 * (n_in - 1)


def _fma32(a, b, c):
    return (a.double() * b.double() + c.double()).float()


def blend_f32(x, up):
    """The kernels' blend of bf16-valued x (B,H,W,C), operation by operation in float32 (conv_ring.hip:113-135 =
    conv_mfma.hip: blend_bf16x8): 16-bit fractions, the four-weight form, a product and three FMAs.  NOT rounded to bf16."""
    B, H, W, C = x.shape
    y0, y1, ly = _axis32(H, H * up)
    x0, x1, lx = _axis32(W, W * up)
    q00, q01, q10, q11 = _corners(x.float(), y0, y1, x0, x1)
    ly, lx = torch.from_numpy(ly).view(1, -1, 1, 1), torch.from_numpy(lx).view(1, 1, -1, 1)
    w11 = lx * ly
    w10, w01 = ly - w11, lx - w11
    w00 = 1.0 - lx - ly + w11
    assert w00.dtype == torch.float32
    r = q00 * w00
    r = _fma32(q01, w01.expand_as(r), r)
    r = _fma32(q10, w10.expand_as(r), r)
    return _fma32(q11, w11.expand_as(r), r)


Vin = collections.namedtuple("Vin", "mid lo hi dv amb g share")


def _virtual_input(c, ins, plant=None):
    """The conv's input (B, Cin, Hin, Win) fp64 NCHW as the kernel multiplies it: mid (the reference value), lo / hi
    (the two bf16 values an ambiguous blended operand may take; equal elsewhere), dv (dt = 0: the unrounded operand's
    error), amb, g = the operand granularity of an exact case, share = the ambiguous share of the blended operands."""
    x = ins["x"].double()
    x2 = None if ins["x2"] is None else ins["x2"].double()
    g, share = 1.0, 0.0
    if c.up == 1:
        assert x2 is None
        if plant in ("source_row_off_below_first_strip", "align_corners_false", "concat_halves_swapped"):
            raise NotExercised("no fused gather")
        mid = x.permute(0, 3, 1, 2)
        z = torch.zeros_like(mid)
        return Vin(mid, mid, mid, z, z.bool(), g, share)
    const = c.x1 == "const"
    if plant == "align_corners_false":
        if const:
            raise NotExercised("a constant map blends to itself under either convention")
        v, rng, qmax = blend64(x, c.up, align_corners=False)[0], None, None
    else:
        v, rng, qmax = blend64(x, c.up)
    if plant == "source_row_off_below_first_strip":
        if const or c.H * c.up <= 4:
            raise NotExercised("needs a second strip and a map that varies")
        xs = torch.cat([x[:, 1:], x[:, -1:]], 1)
        v = v.clone()
        v[:, 4:] = blend64(xs, c.up)[0][:, 4:]
    if c.kind == "exact":
        if plant is None:   # the construction makes the kernels' own arithmetic exact
            assert torch.equal(blend_f32(x, c.up).double(), v) or const, c.name
            if const:
                assert torch.equal(bf16_rn(blend_f32(x, c.up).double()), x[:, :1, :1].expand_as(v)), c.name
                v = x[:, :1, :1].expand_as(v).contiguous()
        elif const:
            v = x[:, :1, :1].expand_as(v).contiguous()
        # ratios 1/4, 5/16, 21/64 -> fractions on a 2^-2, 2^-4, 2^-6 grid per axis; the bf16 rounding keeps the grid
        g = 1.0 if const else 2.0 ** -({3: 2, 11: 4, 43: 6}[c.H] + {3: 2, 11: 4, 43: 6}[c.W])
        dv = torch.zeros_like(v)
    else:
        dv = (blend_delta(c.H) + blend_delta(c.W)) * rng + 32.0 * U32 * qmax if rng is not None else torch.zeros_like(v)
    if c.dt == F32:
        lo = hi = mid = v
        amb = torch.zeros_like(v).bool()
    else:
        lo, hi, mid = bf16_rn(v - dv), bf16_rn(v + dv), bf16_rn(v)
        amb = lo != hi
        share = float(amb.double().mean())
        dv = torch.zeros_like(v)
    parts = lambda u: [u] if x2 is None else ([u, x2] if plant == "concat_halves_swapped" else [x2, u])  # noqa: E731
    if plant == "concat_halves_swapped" and x2 is None:
        raise NotExercised("no skip tensor")
    cat = lambda u, fill=None: torch.cat(parts(u) if fill is None else  # noqa: E731
                                         [p if p is u else torch.full_like(p, fill) for p in parts(u)], 3).permute(0, 3, 1, 2)
    ambc = cat(amb.double(), 0.0) > 0
    return Vin(cat(mid), cat(lo), cat(hi), cat(dv, 0.0), ambc, g, share)


# ----------------------------------------------------------------------------------------------------------------------
# the reference
# ----------------------------------------------------------------------------------------------------------------------
def _assert_exact(xabs, wabs, g, c):
    """Every product and partial sum of the conv is a multiple of g and below 2^24 g: exact in fp32 in any order."""
    assert bool((xabs / g == torch.round(xabs / g)).all()) and bool((wabs == torch.round(wabs)).all()), c.name
    S = F.conv2d(xabs, wabs, None, c.stride, c.pad)
    assert float(S.max()) / g < 2.0 ** 24, (c.name, float(S.max()) / g)
    return S


def _swap_pieces(t):
    """Channels (dim 1): 8-channel pieces 1 and 2 of every 32-channel chunk exchanged."""
    C = t.shape[1]
    if C % 32:
        raise NotExercised("no whole 32-channel chunk")
    idx = torch.arange(C).view(-1, 4, 8)[:, [0, 2, 1, 3]].reshape(-1)
    return t[:, idx]


def _swap_phases(t):
    """(B,C,H,W) -> phase planes (0,1) and (1,0) exchanged, on the image padded with zeros to even sizes."""
    B, C, H, W = t.shape
    t = F.pad(t, (0, W % 2, 0, H % 2))
    out = t.clone()
    out[:, :, 0::2, 1::2] = t[:, :, 1::2, 0::2]
    out[:, :, 1::2, 0::2] = t[:, :, 0::2, 1::2]
    return out


Ref = collections.namedtuple("Ref", "out bound out2 bound2 stats stats_bound share raw S")


def expected(c, t, strict=True):
    """An exact case's fp64 reference rounded once to the output type (strict: the fp64 value is an fp32 number)."""
    f = t.float()
    assert not strict or torch.equal(f.double(), t), c.name
    return f if (c.dt == F32 or c.head_n) else f.bfloat16()


def ref_conv(c, ins, plant=None):
    """The case's outputs UNROUNDED in fp64 in the layout the op returns (NHWC; head: (B, n, Ho, Wo)) and their bounds
    (zero for an exact case).  out2 / bound2: the second tensor of the dual form.  stats / stats_bound: (2 Cout)."""
    if plant is not None and plant not in PLANTS:
        raise ValueError(plant)
    exact = c.kind == "exact"
    vin = _virtual_input(c, ins, plant)
    w = effective_weight(c, ins["w"])
    assert tuple(w.shape) == (c.Cout, c.Cx + c.C2, c.K, c.K), (c.name, tuple(w.shape))
    Ho, Wo = out_hw(c)
    xin = vin.mid
    if plant == "pieces_swapped_in_chunk":
        xin = _swap_pieces(xin)
    conv = lambda a, b: F.conv2d(a, b, None, c.stride, c.pad)  # noqa: E731
    if plant == "phases_01_10_swapped":
        if c.stride != 2 or c.K == 1:
            raise NotExercised("needs more than one phase plane")
        raw = conv(_swap_phases(xin), w)[:, :, :Ho, :Wo]
    else:
        raw = conv(xin, w)
    assert tuple(raw.shape) == (c.B, c.Cout, Ho, Wo)
    if plant == "edge_column_shifted":   # the last output column reads its patch one column to the left
        raw = raw.clone()
        raw[..., -1] = conv(torch.roll(xin, 1, 3), w)[..., -1]
    if plant == "last_chunk_dropped_in_last_tile":
        xz = xin.clone()
        xz[:, -32:] = 0.0
        r0, c0 = (Ho - 1) // 4 * 4, (Wo - 1) // 16 * 16
        raw = raw.clone()
        raw[-1, :, r0:, c0:] = conv(xz[-1:], w)[0, :, r0:, c0:]
    K = w[0].numel()
    xabs = torch.maximum(vin.lo.abs(), vin.hi.abs())
    if exact:
        S = _assert_exact(xabs, w.abs(), vin.g, c) if plant is None else conv(xabs, w.abs())
        Eacc = torch.zeros_like(raw)
        assert not bool(vin.amb.any())
    else:
        S = conv(xabs, w.abs())
        Eacc = (K + 2) * U32 * S + conv((vin.hi - vin.lo) * vin.amb + vin.dv, w.abs())
    stats = stats_bound = None
    if c.stats:
        M = c.B * Ho * Wo
        c0 = ins["stats0"].double()
        a = raw.abs() + Eacc
        s1, s2 = raw.sum((0, 2, 3)) + c0[:c.Cout], (raw * raw).sum((0, 2, 3)) + c0[c.Cout:]
        E1 = Eacc.sum((0, 2, 3)) + (M + 2) * U32 * (a.sum((0, 2, 3)) + c0[:c.Cout].abs())
        E2 = (2 * raw.abs() * Eacc + Eacc * Eacc + U32 * a * a).sum((0, 2, 3)) \
            + (M + 2) * U32 * ((a * a).sum((0, 2, 3)) + c0[c.Cout:].abs())
        stats, stats_bound = torch.cat([s1, s2]), torch.cat([E1, E2]) + TINY
    ch = lambda t: t.double().view(1, -1, 1, 1)  # noqa: E731
    sc = ch(ins["scale"]) if ins["scale"] is not None else ch(torch.ones(c.Cout))
    sh = ch(ins["shift"]) if ins["shift"] is not None else ch(torch.zeros(c.Cout))
    if plant == "shift_before_scale":
        if ins["scale"] is None or exact:
            raise NotExercised("needs a scale and a shift")
        pre = sc * (raw + sh)
    else:
        pre = sc * raw + sh
    Ep = torch.zeros_like(raw) if exact else sc.abs() * Eacc + 2.0 * U32 * (sc.abs() * (raw.abs() + Eacc) + sh.abs())
    res = None if ins["residual"] is None else ins["residual"].double().permute(0, 3, 1, 2)
    late = plant == "residual_after_activation"
    if late and (res is None or not c.relu):
        raise NotExercised("needs a residual and an activation")
    t = pre
    if res is not None and not late:
        t = pre + res
        if not exact:
            Ep = Ep + U32 * (pre.abs() + Ep + res.abs())
    out = t
    if c.relu:
        out = torch.relu(t)
        if c.entry == "dual" and plant != "relu_on_second_output":
            out = torch.cat([out[:, :c.split], t[:, c.split:]], 1)
    if plant == "relu_on_second_output" and not (c.entry == "dual" and c.relu):
        raise NotExercised("no second output")
    if late:
        out = out + res
    if c.head_n:
        if plant == "bf16_truncated":
            raise NotExercised("fp32 output is not rounded")
        hw, hb = ins["head_w"].double(), ins["head_b"].double()
        if plant == "head_bias_of_class_0":
            if c.head_n < 2:
                raise NotExercised("one class")
            hb = hb[:1].expand(c.head_n)
        logits = torch.einsum("kc,bchw->bkhw", hw, out) + hb.view(1, -1, 1, 1)
        if exact:
            Sh = torch.einsum("kc,bchw->bkhw", hw.abs(), out.abs()) + hb.abs().view(1, -1, 1, 1)
            assert plant is not None or (float(Sh.max()) / vin.g < 2.0 ** 24 and float(out.abs().max()) / vin.g < 2.0 ** 16), c.name
            return Ref(logits, torch.zeros_like(logits), None, None, None, None, vin.share, raw, S)
        Sh = torch.einsum("kc,bchw->bkhw", hw.abs(), out.abs() + Ep) + hb.abs().view(1, -1, 1, 1)
        lin = torch.einsum("kc,bchw->bkhw", hw.abs(), Ep)
        Eh = lin + ((3.1 * 2.0 ** -16 + (3 * c.Cout + 3) * U32) if c.kernel == "tile" else (c.Cout + 3) * U32) * Sh
        return Ref(logits, f32_out_bound(Eh), None, None, None, None, vin.share, raw, S)
    if plant == "head_bias_of_class_0":
        raise NotExercised("no head")
    if plant == "bf16_truncated":
        if c.dt == F32:
            raise NotExercised("fp32 output is not rounded")
        out = bf16_trunc(out)
    bound = torch.zeros_like(out) if exact else (f32_out_bound(Ep) if c.dt == F32 else bf16_out_bound(out, Ep))
    nhwc = lambda a: a.permute(0, 2, 3, 1).contiguous()  # noqa: E731
    if c.entry == "dual":
        return Ref(nhwc(out[:, :c.split]), nhwc(bound[:, :c.split]), nhwc(out[:, c.split:]), nhwc(bound[:, c.split:]),
                   stats, stats_bound, vin.share, raw, S)
    return Ref(nhwc(out), nhwc(bound), None, None, stats, stats_bound, vin.share, raw, S)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The unplanted reference of a case: computed once, shared, never written to."""
    return ref_conv(BY_NAME[name], make_inputs(name))


# ----------------------------------------------------------------------------------------------------------------------
# a second, independent derivation (F.interpolate + F.unfold) and a float32 emulation of the correct arithmetic
# ----------------------------------------------------------------------------------------------------------------------
def ref_conv_second(c, ins):
    """act(scale * conv + shift + residual) (before the head, NCHW, unrounded operands) from F.interpolate and an
    im2col matrix product; the pack layouts (s2_dgrad, ring_dgrad) through autograd of the forward conv instead."""
    x = ins["x"].double().permute(0, 3, 1, 2)
    if c.up > 1:
        x = F.interpolate(x, scale_factor=c.up, mode="bilinear", align_corners=True)
        if c.dt == BF16:
            x = bf16_rn(x)
    if ins["x2"] is not None:
        x = torch.cat([ins["x2"].double().permute(0, 3, 1, 2), x], 1)
    w = ins["w"].double() if c.dt == F32 else ins["w"].bfloat16().double()
    Ho, Wo = out_hw(c)
    if c.wpack == "ring_dgrad":
        xin = torch.zeros(c.B, c.Cout, c.H, c.W, dtype=torch.float64, requires_grad=True)
        F.conv2d(xin, w, None, 1, 1).backward(x)
        raw = xin.grad
    elif c.wpack == "s2_dgrad":
        # dY (B, Cx, H, W) is the gradient of a (2H, 2W) -> (H, W) stride-2 conv; the kernel's output rows / columns
        # s .. s + H - 1 (s = 1) hold the phase planes of dX, the rest reach past the input
        Kf = w.shape[2]
        xin = torch.zeros(c.B, w.shape[1], 2 * c.H, 2 * c.W, dtype=torch.float64, requires_grad=True)
        F.conv2d(xin, w, None, 2, {3: 1, 7: 3}[Kf]).backward(x)
        dx = xin.grad.reshape(c.B, -1, c.H, 2, c.W, 2).permute(0, 3, 5, 1, 2, 4).reshape(c.B, -1, c.H, c.W)
        return dx   # the interior [1 : 1 + H, 1 : 1 + W] of the kernel's (H + 1, W + 1) output
    else:
        cols = F.unfold(x, c.K, 1, c.pad, c.stride)
        raw = (w.reshape(c.Cout, -1) @ cols).reshape(c.B, c.Cout, Ho, Wo)
    return raw


def emulate_f32(c, ins):
    """The correct arithmetic in float32 (operands rounded where the kernels round them, torch's fp32 conv as ONE
    possible summation order): what `check` must accept.  Returns the tensors of Ref.out / out2 / stats."""
    x = ins["x"].float()
    if c.up > 1:
        v = blend_f32(ins["x"], c.up)
        if c.dt == F32:   # lerp form of conv_direct_kernel, unquantised fractions
            xx = ins["x"].float()
            y0, y1, _ = _axis32(c.H, c.H * c.up)
            x0, x1, _ = _axis32(c.W, c.W * c.up)
            sy = _ratio32(c.H, c.H * c.up) * np.arange(c.H * c.up).astype(np.float32)
            sx = _ratio32(c.W, c.W * c.up) * np.arange(c.W * c.up).astype(np.float32)
            ly = torch.from_numpy((sy - y0.astype(np.float32)).astype(np.float32)).view(1, -1, 1, 1)
            lx = torch.from_numpy((sx - x0.astype(np.float32)).astype(np.float32)).view(1, 1, -1, 1)
            q = _corners(xx, y0, y1, x0, x1)
            top, bot = q[0] + lx * (q[1] - q[0]), q[2] + lx * (q[3] - q[2])
            v = top + ly * (bot - top)
        x = v.bfloat16().float() if c.dt == BF16 else v
    if ins["x2"] is not None:
        x = torch.cat([ins["x2"].float(), x], 3)
    w = effective_weight(c, ins["w"]).float()
    raw = F.conv2d(x.permute(0, 3, 1, 2), w, None, c.stride, c.pad)
    ch = lambda t: t.view(1, -1, 1, 1)  # noqa: E731
    v = raw
    if ins["scale"] is not None:
        v = raw * ch(ins["scale"]) + ch(ins["shift"])
    if ins["residual"] is not None:
        v = v + ins["residual"].float().permute(0, 3, 1, 2)
    if c.relu:
        v = torch.cat([torch.relu(v[:, :c.split]), v[:, c.split:]], 1) if c.entry == "dual" else torch.relu(v)
    stats = None
    if c.stats:
        stats = torch.cat([raw.sum((0, 2, 3)), (raw * raw).sum((0, 2, 3))]) + ins["stats0"]
    if c.head_n:
        hw = ins["head_w"]
        if c.kernel == "tile":   # bf16 hi + lo split of both operands, lo lo dropped
            sp = lambda t: (t.bfloat16().float(), (t - t.bfloat16().float()).bfloat16().float())  # noqa: E731
            (vh, vl), (wh, wl) = sp(v), sp(hw)
            e = lambda a, b: torch.einsum("kc,bchw->bkhw", a, b)  # noqa: E731
            return e(wh, vl) + e(wl, vh) + e(wh, vh) + ins["head_b"].view(1, -1, 1, 1), None, None
        return torch.einsum("kc,bchw->bkhw", hw, v) + ins["head_b"].view(1, -1, 1, 1), None, None
    if c.dt == BF16:
        v = v.bfloat16()
    v = v.permute(0, 2, 3, 1).contiguous()
    if c.entry == "dual":
        return v[..., :c.split].contiguous(), v[..., c.split:].contiguous(), stats
    return v, None, stats
