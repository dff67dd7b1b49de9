"""fp64 references, DERIVED error bounds, cases and planted errors for the tests of the vovnet depth-head kernels alone
(tests/test_depth_heads_gpu.py on the GPU, tests/test_depth_head_ref_cpu.py for this helper itself):

  K2v          lss_camencode_v2_fwd        ops.camencode_v2        ref_camencode_v2
  K2           lss_depthnet_softmax_fwd    ops.depthnet_softmax    ref_depthnet_softmax
  fusion tail  lss_depth_fuse_softmax_fwd  ops.depth_fuse_softmax  ref_depth_fuse_softmax

Rounding points.  Each reference computes in fp64 from exactly the operands the kernel multiplies:
  math = F32    nothing is rounded; a bf16 hidden map enters at its own bf16 values (widened exactly).
  math = BF16   the activations (hidden, c3 / x) and the weights are rounded to bf16, round to nearest even
                (`.bfloat16()`, what lss_f2bf does), the products are exact in fp32 and accumulate in fp32.
                Biases are never rounded.
  fusion tail   no operand is rounded.  The source index and the four interpolation weights are computed in float32
                exactly as the kernel and ATen write them (rh = float32(H4) / float32(H),
                sh = max(rh * (oh + 0.5f) - 0.5f, 0), h1 = h0 + (h0 < H4 - 1), lh1 = sh - h0, lh0 = 1 - lh1); everything
                after that is fp64.

Bounds (u = 2^-24, the unit roundoff of fp32).  None is measured.
  dot product   Any fp32 evaluation of a K-term dot product plus bias - any order, with or without FMA - satisfies
                |got - ref| <= (K + 2) u S elementwise with S = sum_k |x_k w_k| + |b|  (Higham, gamma_(K+1) S, and
                (K + 1) u / (1 - (K + 1) u) < (K + 2) u for K <= 768).  That is the bound of logits and context rows.
                The kernels' summation trees are far shallower than K (four K quarters of K / 16 chained MFMAs each),
                which is the room that also holds the rounding of (logit - max), at most 2 u max S, in the softmax.
  softmax       eps = the largest logit bound over the pixel.  Perturbing every logit by at most eps moves a probability
                by a factor within exp(+-2 eps); expf (1 ulp = 2u), the D-term sum (D - 1 additions of terms that carry
                expf's 2u) and the division (u) add at most (D + 8) u:  |got - ref| <= ref (2 eps + (D + 8) u) + 2^-126.
                The last term is the smallest normal fp32 number: a probability below it may be flushed to zero or
                lose bits as a denormal (pre-activations of 120 give exp(-120) = 8e-53).
  fusion tail   up = lh0 (lw0 c00 + lw1 c01) + lh1 (lw0 c10 + lw1 c11) is three levels of fp32 multiply-add on operands
                the reference shares bit for bit: error <= 4 u U with U the same expression over |c|.  If the compiler
                contracts rh * (oh + 0.5f) - 0.5f into an FMA, sh moves by at most one ulp of t = fl(rh (oh + 0.5f))
                (t - 0.5f is exact for t >= 0.5; below 0.5 both forms clamp to 0); the bilinear interpolant is
                continuous and piecewise linear with slope at most 2 max|c| per unit of sh, so the index / weight
                change moves `up` by at most (ulp(t_h) + ulp(t_w)) 2 Cmax, Cmax = max |c| over the channel's coarse map:
                    E_up = 4 u U + 2 Cmax (ulp(t_h) + ulp(t_w)).
                a = sum_k w[n, k] x[k] over x = [d3, up] is a 2D-term dot product without bias:
                    E_a = (2D + 2) u sum_k |w x| + sum_k |w[n, D + k]| E_up[k].
                v = max(a scale + shift, 0), with or without FMA, and the ReLU is 1-Lipschitz:
                    E_v = |scale| E_a + 2 u (|a scale| + |shift|).
                The softmax bound above then takes eps = max E_v + u/2 max v over the pixel (the second term is the
                rounding of v - max, written out here because E_v has no slack to hold it: the kernel's 2D-term chain
                is sequential).

`check(got, ref, bound)` asserts the elementwise bound and returns the two metrics of `train_node_ref.errors`.

Planted errors (`plant=`): a deliberately wrong copy of the reference; every one moves an output by a whole product or
a whole bf16 ulp, orders of magnitude more than the bounds, and the CPU test proves `check` rejects each.  A case that
cannot exercise a plant raises `NotExercised`.
"""
import collections
import math as _math

import numpy as np
import torch

from train_node_ref import errors

U32 = 2.0 ** -24
TINY = 2.0 ** -126
F32, BF16 = 0, 1   # the `math` / dtype codes of the C ABI (ops.DT_F32, ops.DT_BF16)
MATH_NAME = {F32: "f32", BF16: "bf16"}

HEAD_PLANTS = ("dropped_k", "last_depth_row_zeroed", "context_bias_from_depth_bias", "softmax_over_padded_rows",
               "bf16_truncated", "partial_tile_pixel_from_previous_image")
FUSE_PLANTS = ("align_corners", "fusion_halves_swapped", "no_relu", "h1_unclamped")


class NotExercised(Exception):
    """The case cannot show this planted error (the plant names the reason)."""


# ----------------------------------------------------------------------------------------------------------------------
# cases
# ----------------------------------------------------------------------------------------------------------------------
V2Case = collections.namedtuple("V2Case", "name BN fH fW Cd Cf D C")
V2_CASES = [
    V2Case("3_8_production_k", 2, 5, 7, 256, 768, 41, 128),   # HW = 35: two full tiles and a 3-pixel tile; BN stride
    V2Case("3_4", 1, 3, 3, 64, 64, 33, 64),                   # one partial tile; f32 single K block; lower D edge of ntd = 3
    V2Case("3_0", 2, 4, 4, 128, 0, 48, 0),                    # HW = 16 exactly; D fills its tiles; no context
    V2Case("4_8", 1, 5, 7, 128, 128, 64, 113),                # D = 64; C not a multiple of 16
    V2Case("4_4", 1, 3, 6, 192, 64, 49, 49),                  # f32 only: three K blocks; both lower edges
    V2Case("4_0", 2, 1, 17, 256, 0, 57, 0),                   # one pixel into the second tile
    V2Case("1_1_c16", 1, 3, 3, 64, 64, 5, 16),                # ntd = ntc = 1
    V2Case("1_1_c3", 1, 3, 3, 64, 64, 16, 3),
    V2Case("1_0", 3, 2, 2, 128, 0, 1, 0),                     # D = 1: probabilities exactly 1
    # the bf16-math instantiations the shapes above leave out (their Cd or Cf is no multiple of 128)
    V2Case("3_4_k128", 1, 3, 3, 128, 128, 40, 50),
    V2Case("4_4_k128", 1, 2, 5, 128, 128, 50, 64),
    V2Case("1_1_k128", 1, 3, 3, 128, 128, 9, 9),
]
# (what, D, C, Cd, Cf, math): every one is refused by lss_camencode_v2_fwd; the rest of the shape is (1, 3, 3)
V2_REFUSED = [("D17", 17, 64, 64, 64, F32), ("D32", 32, 64, 64, 64, F32), ("D65", 65, 64, 64, 64, F32),
              ("C32", 41, 32, 64, 64, F32), ("C129", 41, 129, 64, 64, F32), ("Cd96", 41, 64, 96, 64, F32),
              ("bf16_Cd64", 41, 64, 64, 128, BF16), ("bf16_Cf192", 41, 64, 128, 192, BF16)]

FuseCase = collections.namedtuple("FuseCase", "name BN D H W H4 W4 gain shift")
FUSE_CASES = [
    FuseCase("production_2x", 2, 41, 8, 22, 4, 11, 1.0, None),
    FuseCase("odd_35_pixels", 1, 41, 5, 7, 3, 3, 1.0, None),      # non-integer ratios; three dead waves
    FuseCase("d64_equal_sizes", 1, 64, 3, 5, 3, 5, 1.0, None),    # every lane live; weights exactly 0 or 1
    FuseCase("d1_coarse_1x1", 3, 1, 2, 3, 1, 1, 1.0, None),       # both clamps at once
    FuseCase("coarse_taller", 1, 5, 6, 6, 9, 4, 1.0, None),
    FuseCase("gain_30", 1, 41, 7, 9, 2, 4, 30.0, None),           # pre-activations up to about 120
    FuseCase("all_cut", 1, 41, 4, 4, 2, 2, 1.0, -100.0),          # every bin cut to 0: uniform 1/D exactly
]

K2Case = collections.namedtuple("K2Case", "name BN Cin fH fW D C math")
K2_CASES = [
    K2Case("f32_one_block", 2, 64, 3, 5, 41, 64, F32),
    K2Case("f32_odd_tail", 2, 192, 3, 5, 41, 64, F32),            # three 16-deep blocks per wave: the odd tail
    K2Case("bf16_k128", 1, 128, 3, 3, 5, 64, BF16),
    K2Case("bf16_k768", 2, 768, 5, 7, 41, 128, BF16),
]


def v2_tiles(c):
    """(ntd, ntc): the LSS_V2_CASE pair a case instantiates."""
    return (c.D + 15) // 16, (c.C + 15) // 16


def v2_modes(c):
    """The math modes lss_camencode_v2_fwd accepts for the case: a wave's K quarter in 16- (f32) or 32-deep blocks."""
    ok = lambda m: c.Cd % m == 0 and (c.C == 0 or c.Cf % m == 0)  # noqa: E731
    return [m for m, q in ((F32, 64), (BF16, 128)) if ok(q)]


def default_math(c, hidden_dtype):
    """What ops.camencode_v2 promises for math=None: the hidden map's own precision when the shapes allow."""
    return BF16 if hidden_dtype == torch.bfloat16 and BF16 in v2_modes(c) else F32


def _gen(name):
    return torch.Generator().manual_seed(sum((i + 1) * ord(ch) for i, ch in enumerate(name)))


def make_v2_inputs(c, hidden_dtype=torch.float32):
    """hidden (BN,fH,fW,Cd) NHWC, wd (D,Cd), bd (D), c3 (BN,Cf,fH,fW) | None, wf (C,Cf) | None, bf (C) | None."""
    g = _gen(c.name)
    hidden = torch.randn(c.BN, c.fH, c.fW, c.Cd, generator=g).to(hidden_dtype)
    wd = torch.randn(c.D, c.Cd, generator=g) / c.Cd ** 0.5
    bd = 0.1 * torch.randn(c.D, generator=g)
    if c.C == 0:
        return hidden, wd, bd, None, None, None
    c3 = torch.randn(c.BN, c.Cf, c.fH, c.fW, generator=g)
    wf = torch.randn(c.C, c.Cf, generator=g) / c.Cf ** 0.5
    bf = 0.1 * torch.randn(c.C, generator=g)
    return hidden, wd, bd, c3, wf, bf


def make_k2_inputs(c):
    g = _gen(c.name)
    x = torch.randn(c.BN, c.Cin, c.fH, c.fW, generator=g)
    w = torch.randn(c.D + c.C, c.Cin, generator=g) / c.Cin ** 0.5
    b = 0.1 * torch.randn(c.D + c.C, generator=g)
    return x, w, b


def make_fuse_inputs(c):
    """d3 (BN,D,H,W), d4 (BN,D,H4,W4), w (D,2D), scale (D), shift (D)."""
    g = _gen(c.name)
    d3 = torch.randn(c.BN, c.D, c.H, c.W, generator=g)
    d4 = torch.randn(c.BN, c.D, c.H4, c.W4, generator=g)
    w = torch.randn(c.D, 2 * c.D, generator=g) / (2 * c.D) ** 0.5
    scale = (torch.rand(c.D, generator=g) + 0.5) * c.gain
    shift = 0.5 * torch.randn(c.D, generator=g) * c.gain
    if c.shift is not None:
        shift = torch.full((c.D,), float(c.shift))
    return d3, d4, w, scale, shift


# ----------------------------------------------------------------------------------------------------------------------
# the 1x1 heads
# ----------------------------------------------------------------------------------------------------------------------
Heads = collections.namedtuple("Heads", "logits prob feat S_logits S_feat bound_logits bound_prob bound_feat depth "
                                        "bound_depth")


def _operand(t, math, plant):
    """fp64 copy of what the kernel multiplies."""
    if math == BF16 and t.dtype != torch.bfloat16:
        t = t.float()
        if plant == "bf16_truncated":
            t = (t.contiguous().view(torch.int32) & -65536).view(torch.float32)
        else:
            t = t.bfloat16()
    return t.double()


def softmax_bound(prob, logit_bound, D, dim, extra=0.0):
    eps = logit_bound.amax(dim, keepdim=True) + extra
    return prob * (2.0 * eps + (D + 8) * U32) + TINY


def _dot(x, w, b):
    """x (BN,HW,K), w (N,K), b (N) in fp64 -> value and magnitude sum, both (BN,HW,N)."""
    return x @ w.t() + b, x.abs() @ w.abs().t() + b.abs()


def _heads(xd, wd, bd, xf, wf, bf, fH, fW, softmax, math, plant, bias_c_plant):
    """xd (BN,HW,Kd) and xf (BN,HW,Kf) | None are the pixel rows of the two products."""
    if plant is not None and plant not in HEAD_PLANTS:
        raise ValueError(plant)
    BN, HW, Kd = xd.shape
    D = wd.shape[0]
    if plant == "bf16_truncated" and math != BF16:
        raise NotExercised("fp32 math rounds no operand")
    xd64, wd64 = _operand(xd, math, plant), _operand(wd, math, plant)
    if plant == "dropped_k":   # k index 5 of wave 2's K quarter
        xd64 = xd64.clone()
        xd64[..., 2 * (Kd // 4) + 5] = 0.0
    logits, S = _dot(xd64, wd64, bd.double())
    if plant == "last_depth_row_zeroed":   # the weight row is never loaded: the logit is its bias
        logits = logits.clone()
        logits[..., D - 1] = bd.double()[D - 1]
    z = logits
    if plant == "softmax_over_padded_rows":
        pad = 16 * ((D + 15) // 16) - D
        if pad == 0:
            raise NotExercised("D fills its 16-row tiles")
        z = torch.cat([logits, logits.new_zeros(BN, HW, pad)], 2)
    prob = torch.softmax(z, 2)[..., :D]
    feat = Sf = None
    if xf is not None:
        Kf = xf.shape[2]
        xf64, wf64 = _operand(xf, math, plant), _operand(wf, math, plant)
        feat, Sf = _dot(xf64, wf64, bf.double())
        if plant == "context_bias_from_depth_bias":
            feat = feat - bf.double() + bias_c_plant
    elif plant == "context_bias_from_depth_bias":
        raise NotExercised("no context projection")
    if plant == "partial_tile_pixel_from_previous_image":
        if HW % 16 == 0 or BN < 2:
            raise NotExercised("needs a partial last tile and a previous image")
        logits, prob = logits.clone(), prob.clone()
        logits[1:, HW - 1], prob[1:, HW - 1] = logits[:-1, HW - 1].clone(), prob[:-1, HW - 1].clone()
        if feat is not None:
            feat = feat.clone()
            feat[1:, HW - 1] = feat[:-1, HW - 1].clone()
    bl = (Kd + 2) * U32 * S
    nchw = lambda t: t.permute(0, 2, 1).reshape(BN, D, fH, fW)  # noqa: E731
    logits, prob, S, bl, bp = nchw(logits), nchw(prob), nchw(S), nchw(bl), nchw(softmax_bound(prob, bl, D, 2))
    bfeat = None if feat is None else (Kf + 2) * U32 * Sf
    return Heads(logits, prob, feat, S, Sf, bl, bp, bfeat, prob if softmax else logits, bp if softmax else bl)


def ref_camencode_v2(hidden, wd, bd, c3, wf, bf, softmax=True, math=F32, plant=None):
    """K2v.  hidden (BN,fH,fW,Cd) fp32 | bf16, wd (D,Cd), bd (D), c3 (BN,Cf,fH,fW) | None, wf (C,Cf), bf (C).
    Returns Heads: logits, prob (BN,D,fH,fW); feat (BN,HW,C) | None; S_* = sum_k |x_k w_k| + |b| per element; the derived
    bounds; depth / bound_depth = what the kernel returns for `softmax`."""
    BN, fH, fW, Cd = hidden.shape
    xf = None if c3 is None else c3.reshape(BN, c3.shape[1], fH * fW).permute(0, 2, 1)
    bias_c = None
    if plant == "context_bias_from_depth_bias" and c3 is not None:   # bias_c read at bias_d: depth bias c (0 past D)
        bias_c = torch.zeros(wf.shape[0], dtype=torch.float64)
        n = min(wf.shape[0], bd.numel())
        bias_c[:n] = bd.double()[:n]
    return _heads(hidden.reshape(BN, fH * fW, Cd), wd.reshape(wd.shape[0], -1), bd, xf,
                  None if wf is None else wf.reshape(wf.shape[0], -1), bf, fH, fW, softmax, math, plant, bias_c)


def ref_depthnet_softmax(x, w, b, D, C, math=F32, plant=None):
    """K2.  x (BN,Cin,fH,fW) fp32, w (D+C,Cin), b (D+C).  Rounding points: x and w.  Returns Heads (softmax always)."""
    BN, Cin, fH, fW = x.shape
    rows = x.reshape(BN, Cin, fH * fW).permute(0, 2, 1)
    w = w.reshape(D + C, Cin)
    return _heads(rows, w[:D], b[:D], rows, w[D:], b[D:], fH, fW, True, math, plant, b.double()[:C])


# ----------------------------------------------------------------------------------------------------------------------
# the fusion tail
# ----------------------------------------------------------------------------------------------------------------------
Fuse = collections.namedtuple("Fuse", "v prob up S_a U bound_v bound_prob")


def source_index(n_out, n_in, dtype=np.float32, align_corners=False):
    """(i0, i1, l0, l1, ulp) of one axis, in `dtype` arithmetic as depth_fuse_softmax_kernel and ATen's
    area_pixel_compute_source_index write it; ulp = spacing of t = r (o + 0.5) where an FMA could move the index."""
    o = np.arange(n_out).astype(dtype)
    if align_corners:
        r = dtype(n_in - 1) / dtype(n_out - 1) if n_out > 1 else dtype(0)
        t = r * o
        s = t
    else:
        r = dtype(n_in) / dtype(n_out)
        t = r * (o + dtype(0.5))
        s = np.maximum(t - dtype(0.5), dtype(0))
    assert t.dtype == dtype and s.dtype == dtype
    i0 = s.astype(np.int64)
    i1 = i0 + (i0 < n_in - 1)
    l1 = s - i0.astype(dtype)
    l0 = dtype(1) - l1
    ulp = np.where(t >= dtype(0.5), np.spacing(t), dtype(0))
    return i0, i1, l0.astype(np.float64), l1.astype(np.float64), ulp.astype(np.float64)


def ref_depth_fuse_softmax(d3, d4, w, scale, shift, plant=None, coord_dtype=np.float32):
    """softmax_D(relu(scale * (w @ [d3, up(d4)]) + shift)).  Returns Fuse: v = the PRE-activation (before the ReLU),
    prob, the upsampled coarse map, S_a = sum |w x|, U = the blend over |d4|, and the derived bounds of relu(v), prob.
    coord_dtype=np.float64 is ATen's arithmetic for a double tensor (ties this function to F.interpolate)."""
    if plant is not None and plant not in FUSE_PLANTS:
        raise ValueError(plant)
    BN, D, H, W = d3.shape
    H4, W4 = d4.shape[2:]
    t64 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64))  # noqa: E731
    ac = plant == "align_corners"
    if ac and ((H4, W4) == (H, W) or (H4 == 1 and W4 == 1)):
        raise NotExercised("both conventions give the same coordinates")
    h0, h1, lh0, lh1, uh = source_index(H, H4, coord_dtype, ac)
    w0, w1, lw0, lw1, uw = source_index(W, W4, coord_dtype, ac)
    c = d4.double()
    if plant == "h1_unclamped":
        if not bool(((h0 == H4 - 1) & (lh1 > 0)).any()):
            raise NotExercised("no output row blends past the last coarse row")
        # row H4 of a channel = row 0 of the next channel in memory (zeros past the tensor)
        nxt = torch.cat([c.reshape(BN * D, H4, W4)[1:, :1], c.new_zeros(1, 1, W4)], 0).reshape(BN, D, 1, W4)
        c = torch.cat([c, nxt], 2)
        h1 = h0 + 1
    ih0, ih1, iw0, iw1 = (torch.from_numpy(i) for i in (h0, h1, w0, w1))
    lh0, lh1 = t64(lh0).view(H, 1), t64(lh1).view(H, 1)
    lw0, lw1 = t64(lw0).view(1, W), t64(lw1).view(1, W)

    def blend(m):
        r0, r1 = m[:, :, ih0], m[:, :, ih1]
        return lh0 * (lw0 * r0[..., iw0] + lw1 * r0[..., iw1]) + lh1 * (lw0 * r1[..., iw0] + lw1 * r1[..., iw1])

    up, U = blend(c), blend(c.abs())
    cmax = d4.double().abs().amax((2, 3), keepdim=True)
    E_up = 4 * U32 * U + 2 * cmax * (t64(uh).view(H, 1) + t64(uw).view(1, W))
    w64 = w.double().reshape(D, 2 * D)
    if plant == "fusion_halves_swapped":
        w64 = torch.cat([w64[:, D:], w64[:, :D]], 1)
    x = torch.cat([d3.double(), up], 1)
    a = torch.einsum("nk,bkhw->bnhw", w64, x)
    S_a = torch.einsum("nk,bkhw->bnhw", w64.abs(), x.abs())
    E_a = (2 * D + 2) * U32 * S_a + torch.einsum("nk,bkhw->bnhw", w64[:, D:].abs(), E_up)
    sc, sf = scale.double().view(1, D, 1, 1), shift.double().view(1, D, 1, 1)
    v = a * sc + sf
    E_v = sc.abs() * E_a + 2 * U32 * ((a * sc).abs() + sf.abs())
    act = v if plant == "no_relu" else torch.relu(v)
    prob = torch.softmax(act, 1)
    bp = softmax_bound(prob, E_v, D, 1, extra=0.5 * U32 * act.abs().amax(1, keepdim=True))
    return Fuse(v, prob, up, S_a, U, E_v, bp)


# ----------------------------------------------------------------------------------------------------------------------
def check(got, ref, bound, what=""):
    """Asserts |got - ref| <= bound elementwise (and that got is finite); returns (max |a - b| / max |b|,
    ||a - b|| / ||b||)."""
    got = got.detach().double().cpu()
    assert got.shape == ref.shape == bound.shape, (what, got.shape, ref.shape, bound.shape)
    assert bool(torch.isfinite(got).all()), "%s: %d non-finite elements" % (what, int((~torch.isfinite(got)).sum()))
    d = (got - ref).abs()
    bad = d > bound
    if bool(bad.any()):
        ratio = torch.where(bad, d / bound.clamp_min(1e-300), d.new_zeros(()))
        i = int(ratio.argmax())
        idx = tuple(int(v) for v in np.unravel_index(i, tuple(d.shape)))
        raise AssertionError("%s: %d of %d elements outside the derived bound; worst at %s: got %.9g ref %.9g "
                             "|diff| %.3e bound %.3e" % (what, int(bad.sum()), d.numel(), idx, float(got[idx]),
                                                         float(ref[idx]), float(d[idx]), float(bound[idx])))
    return errors(got, ref)


def sum_to_one_bound(D):
    """A column of fp32 probabilities e_d / sum: each carries the division's u, their fp32 or fp64 re-summation at most
    (D - 1) u more: (D + 8) u as in the softmax bound."""
    return (D + 8) * U32


assert _math.isclose(U32, float(np.finfo(np.float32).eps) / 2)
